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
#include "decode_ms_f64_ws.hpp"        // the workspace kernel and the f64 dispatch

namespace ldpc {

// only the plain register kernel holds its f64 LLRs in registers (kernel_reads_llrs_once)
template <>
bool decode_ms_reads_llrs_once<double>(int code, int variant)
{
    if (variant != 0 || !valid_code(code)) return false;
    return (F64_TUNED[code] & (16 | 32)) == 0;
}

}  // namespace ldpc
