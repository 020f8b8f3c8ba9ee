// decode_ms_f64.hip -- f64 min-sum decoder (decode_ms::<f64>, /root/reference/src/decoder.rs:78-86,
// :347-475; C entry capi/src/lib.rs:121-127).
//
// By default every code runs the register-resident kernel of decode_ms_kernel.hpp with 64-bit
// registers and LDS elements (decode_ms_f64_reg.hip): plain for the small codes, register-lean for
// TM2048 / TM5120, "in place" (no array of marginals, v kept as sign/zero bit masks) for TM6144 and
// TM8192, whose f64 exchange arrays would not fit the LDS otherwise.  f64 LLRs are the least used
// variant of the reference's API; the kernel below is the general fallback (`variant` 100, 10-100x
// slower) that trades
// speed for generality: one workgroup per codeword, marginals in LDS, the per-edge messages u and v
// in a global-memory workspace (edge e = block * M + check index: coalesced), per-check minima in
// registers of the thread that owns the check.  Same block lists, same arithmetic order:
//   variable phase  thread x of block column c:  va = llr + sum of u over its blocks in list order
//                   (decoder.rs:382-383, :408; the check index of a block is the closed-form
//                   inverse of the block's rotation)
//   check phase     thread i of block row r:     decoder.rs:419-447 for its edges in order, then
//                   decoder.rs:391-405 (next u) from the row's (min1, min2, sign)
// Results equal the reference's bit for bit (IEEE f64 add/sub, no contraction).
#include "decode_ms_f64_ws.hpp"
#include "decode_ms_tables.hpp"

namespace ldpc {

hipError_t launch_decode_ms_f64_reg(int code, int ipt, int lean, const double *llrs, uint8_t *output, uint32_t *iters,
                                    uint8_t *success, size_t batch, uint32_t maxiters, hipStream_t stream);

// the tuned default per code: F64_TUNED (decode_ms_tables.hpp)

// only the plain register kernel holds its f64 LLRs in registers (kernel_reads_llrs_once)
template <>
bool decode_ms_reads_llrs_once<double>(int code, int variant)
{
    if (variant != 0 || !valid_code(code)) return false;
    return (F64_TUNED[code] & (16 | 32)) == 0;
}

// variant: 0 = tuned default; 100 = the workspace kernel above; otherwise the register kernel with
// IPT = variant & 15, the register-lean check phase if variant & 16, in-place messages if variant & 32.
template <>
hipError_t launch_decode_ms<double>(int code, int variant, const double *llrs, uint8_t *output, uint32_t *iters,
                                    uint8_t *success, size_t batch, uint32_t maxiters, hipStream_t stream)
{
    if (batch == 0) return hipSuccess;
    if (!valid_code(code)) return hipErrorInvalidValue;
    if (variant >= 0) variant &= ~VARIANT_FLAGS;           // (the f64 kernels always draw from the launch's queue)
    if (variant == 0) variant = F64_TUNED[code];
    if (variant != 100)
        return launch_decode_ms_f64_reg(code, variant & 15, (variant & 32) ? 2 : ((variant & 16) ? 1 : 0), llrs, output, iters, success, batch,
                                        maxiters, stream);
    switch (code) {
        case TC128:  return launch_f64<TC128>(llrs, output, iters, success, batch, maxiters, stream);
        case TC256:  return launch_f64<TC256>(llrs, output, iters, success, batch, maxiters, stream);
        case TC512:  return launch_f64<TC512>(llrs, output, iters, success, batch, maxiters, stream);
        case TM1280: return launch_f64<TM1280>(llrs, output, iters, success, batch, maxiters, stream);
        case TM1536: return launch_f64<TM1536>(llrs, output, iters, success, batch, maxiters, stream);
        case TM2048: return launch_f64<TM2048>(llrs, output, iters, success, batch, maxiters, stream);
        case TM5120: return launch_f64<TM5120>(llrs, output, iters, success, batch, maxiters, stream);
        case TM6144: return launch_f64<TM6144>(llrs, output, iters, success, batch, maxiters, stream);
        case TM8192: return launch_f64<TM8192, 1024, 256>(llrs, output, iters, success, batch, maxiters, stream);   // 0.122 vs 0.081 M/s at 256 threads x 1024 workgroups
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ldpc
