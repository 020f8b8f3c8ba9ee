// decode_ms_soft_f64.hip -- decode_ms::<f64> with soft output (/root/reference/src/decoder.rs:78-86, :377): the soft-output forms
// of the f64 register kernels of decode_ms_f64_reg.hip and of the workspace kernel (decode_ms_f64_ws.hpp), three objects
// (Makefile: -DF64_PART=0/1/2) as for the hard-only kernels.
//
// The in-place register kernels (`variant` | 32; TM8192's default) keep the marginals of the exchanged columns only as sign words
// in LDS, so they have no soft form: an explicit in-place variant is refused (hipErrorInvalidConfiguration), and the DEFAULT soft
// decode of a code whose tuned kernel is in place (F64_TUNED: TM8192) runs the workspace kernel -- its non-in-place register
// kernel would need 176 KB of LDS, more than a CU has.
#include "decode_ms_launch.hpp"
#include "decode_ms_tables.hpp"
#if F64_PART == 0
#define LDPC_F64_WS_SOFT
#include "decode_ms_f64_ws.hpp"
#endif

namespace ldpc {

#ifndef F64_PART
#error "compile with -DF64_PART=0, 1 or 2"
#endif
#define F64_CAT2(a, b) a##b
#define F64_CAT(a, b) F64_CAT2(a, b)

#if F64_PART == 0
hipError_t launch_decode_ms_soft_f64_reg_1(int, int, int, const double *, double *, uint8_t *, uint32_t *, uint8_t *, size_t, uint32_t, hipStream_t);
hipError_t launch_decode_ms_soft_f64_reg_2(int, int, int, const double *, double *, uint8_t *, uint32_t *, uint8_t *, size_t, uint32_t, hipStream_t);
#endif

// ipt / lean select the instantiation; hipErrorInvalidConfiguration if it has no soft form
#if F64_PART == 0
static hipError_t launch_decode_ms_soft_f64_reg(
#else
hipError_t F64_CAT(launch_decode_ms_soft_f64_reg_, F64_PART)(
#endif
int code, int ipt, int lean, const double *llrs, double *app, uint8_t *output, uint32_t *iters,
                                         uint8_t *success, size_t batch, uint32_t maxiters, hipStream_t stream)
{
#define F64_CFG(CODE, IPT, LEAN)                                                                                     \
    if (code == CODE && ipt == IPT && lean == LEAN)                                                                  \
        return launch_cfg<CODE, double, IPT, LEAN, true>(llrs, output, iters, success, batch, maxiters, stream, 0u, app);
    // (the register kernels of decode_ms_f64_reg.hip without the in-place ones, LEAN == 2)
#if F64_PART == 0
    F64_CFG(TC128, 1, 0)  F64_CFG(TC128, 1, 1)
    F64_CFG(TC256, 1, 0)  F64_CFG(TC256, 1, 1)
    F64_CFG(TC512, 1, 0)  F64_CFG(TC512, 1, 1)
    if (code == TM1280 || code == TM1536 || code == TM2048)
        return launch_decode_ms_soft_f64_reg_1(code, ipt, lean, llrs, app, output, iters, success, batch, maxiters, stream);
    return launch_decode_ms_soft_f64_reg_2(code, ipt, lean, llrs, app, output, iters, success, batch, maxiters, stream);
#elif F64_PART == 1
    F64_CFG(TM1280, 1, 0) F64_CFG(TM1280, 1, 1)
    F64_CFG(TM1536, 1, 0) F64_CFG(TM1536, 1, 1)
    F64_CFG(TM2048, 1, 0) F64_CFG(TM2048, 1, 1)
    return hipErrorInvalidConfiguration;
#else
    F64_CFG(TM5120, 1, 1)  F64_CFG(TM5120, 2, 1)
    F64_CFG(TM6144, 1, 1)  F64_CFG(TM6144, 2, 1) F64_CFG(TM6144, 2, 0)
    return hipErrorInvalidConfiguration;
#endif
#undef F64_CFG
}

#if F64_PART == 0
// variant: as launch_decode_ms<double> (decode_ms_f64.hip), but in place (| 32) is refused and a tuned in-place default becomes 100
template <>
hipError_t launch_decode_ms_soft<double>(int code, int variant, const double *llrs, double *app, uint8_t *output, uint32_t *iters,
                                         uint8_t *success, size_t batch, uint32_t maxiters, hipStream_t stream)
{
    if (batch == 0) return hipSuccess;
    if (!valid_code(code)) return hipErrorInvalidValue;
    if (variant >= 0) variant &= ~VARIANT_FLAGS;
    if (variant == 0) variant = (F64_TUNED[code] & 32) ? 100 : F64_TUNED[code];
    if (variant != 100) {
        if (variant & 32) return hipErrorInvalidConfiguration;
        return launch_decode_ms_soft_f64_reg(code, variant & 15, (variant & 16) ? 1 : 0, llrs, app, output, iters, success, batch, maxiters, stream);
    }
    switch (code) {
        case TC128:  return launch_f64<TC128>(llrs, output, iters, success, batch, maxiters, stream, app);
        case TC256:  return launch_f64<TC256>(llrs, output, iters, success, batch, maxiters, stream, app);
        case TC512:  return launch_f64<TC512>(llrs, output, iters, success, batch, maxiters, stream, app);
        case TM1280: return launch_f64<TM1280>(llrs, output, iters, success, batch, maxiters, stream, app);
        case TM1536: return launch_f64<TM1536>(llrs, output, iters, success, batch, maxiters, stream, app);
        case TM2048: return launch_f64<TM2048>(llrs, output, iters, success, batch, maxiters, stream, app);
        case TM5120: return launch_f64<TM5120>(llrs, output, iters, success, batch, maxiters, stream, app);
        case TM6144: return launch_f64<TM6144>(llrs, output, iters, success, batch, maxiters, stream, app);
        case TM8192: return launch_f64<TM8192, 1024, 256>(llrs, output, iters, success, batch, maxiters, stream, app);
        default: return hipErrorInvalidValue;
    }
}
#endif

}  // namespace ldpc
