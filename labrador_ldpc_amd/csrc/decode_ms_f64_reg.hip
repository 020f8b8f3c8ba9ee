// decode_ms_f64_reg.hip -- f64 instantiations of the register-resident min-sum kernel
// (decode_ms::<f64>, /root/reference/src/decoder.rs:78-86, :347-475) for the codes whose f64 exchange
// arrays fit the 160 KB of LDS; TM8192 (176 KB with an array of marginals) runs the in-place variant
// (LEAN == 2, 152 KB).  The workspace kernel of decode_ms_f64.hip remains as variant 100.
// With -DLDPC_SOFT=1 (decode_ms_soft_f64_<part>.o): the soft-output forms of the kernels that have one; object 0 of those also holds
// the soft-output workspace kernel and the dispatch (decode_ms_f64_ws.hpp), which the hard-only form has in decode_ms_f64.o.
#include "decode_ms_launch.hpp"

namespace ldpc {

// The instantiations are compiled as three objects (Makefile: -DF64_PART=0/1/2) to keep the build parallel.
#ifndef F64_PART
#error "compile with -DF64_PART=0, 1 or 2"
#endif

template <>
hipError_t launch_decode_ms_f64_reg<LDPC_SOFT, F64_PART>(int code, int ipt, int lean, const double *llrs, double *app, uint8_t *output,
                                                         uint32_t *iters, uint8_t *success, size_t batch, uint32_t maxiters, hipStream_t stream)
{
#define F64_CFG(CODE, IPT, LEAN)                                                                                     \
    if (code == CODE && ipt == IPT && lean == LEAN)                                                                  \
        return launch_cfg<CODE, double, IPT, LEAN, LDPC_SOFT>(llrs, output, iters, success, batch, maxiters, stream, 0u, app);
// the in-place kernels keep the marginals of the exchanged columns only as sign words in LDS: no soft form
#if LDPC_SOFT
#define F64_CFG_IN_PLACE(CODE, IPT)
#else
#define F64_CFG_IN_PLACE(CODE, IPT) F64_CFG(CODE, IPT, 2)
#endif
#if F64_PART == 0
    F64_CFG(TC128, 1, 0)  F64_CFG(TC128, 1, 1)
    F64_CFG(TC256, 1, 0)  F64_CFG(TC256, 1, 1)
    F64_CFG(TC512, 1, 0)  F64_CFG(TC512, 1, 1)
    if (code == TM1280 || code == TM1536 || code == TM2048)
        return launch_decode_ms_f64_reg<LDPC_SOFT, 1>(code, ipt, lean, llrs, app, output, iters, success, batch, maxiters, stream);
    return launch_decode_ms_f64_reg<LDPC_SOFT, 2>(code, ipt, lean, llrs, app, output, iters, success, batch, maxiters, stream);
#elif F64_PART == 1
    F64_CFG(TM1280, 1, 0) F64_CFG(TM1280, 1, 1) F64_CFG_IN_PLACE(TM1280, 1)
    F64_CFG(TM1536, 1, 0) F64_CFG(TM1536, 1, 1)
    F64_CFG(TM2048, 1, 0) F64_CFG(TM2048, 1, 1) F64_CFG_IN_PLACE(TM2048, 1)
    return hipErrorInvalidConfiguration;
#else
    F64_CFG(TM5120, 1, 1)  F64_CFG(TM5120, 2, 1) F64_CFG_IN_PLACE(TM5120, 1)
    F64_CFG(TM6144, 1, 1)  F64_CFG(TM6144, 2, 1) F64_CFG(TM6144, 2, 0) F64_CFG_IN_PLACE(TM6144, 1)
    F64_CFG_IN_PLACE(TM8192, 2)  F64_CFG_IN_PLACE(TM8192, 4)
    return hipErrorInvalidConfiguration;
#endif
#undef F64_CFG
#undef F64_CFG_IN_PLACE
}

}  // namespace ldpc

#if LDPC_SOFT && F64_PART == 0         // (after the specialization above, which the dispatch calls)
#include "decode_ms_f64_ws.hpp"
#endif
