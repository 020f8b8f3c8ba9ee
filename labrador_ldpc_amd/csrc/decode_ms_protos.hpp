// decode_ms_protos.hpp -- the min-sum launchers that cross translation units, declared once: capi.hip calls them, the decode_ms_*.hip
// units define them, and both sides include this header, so a signature that drifts from its definition does not compile.
// Declarations only: capi.hip must not see the kernels (decode_ms_kernel.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace ldpc {

// Launch the decoder for `batch` frames on `stream`.  `variant` = 0 picks the tuned default
// IPT (indices per thread) for the code; a positive value requests that IPT explicitly and
// yields hipErrorInvalidConfiguration if it was not instantiated.  VARIANT_STATIC added to either
// distributes the codewords over the workgroups by a fixed stride instead of through the launch's queue.
// SOFT: the soft-output kernels, which also write every codeword's marginals (decoder.rs:377) to `app` [batch][n + p] in the
// LLR type (nullptr without SOFT); hipErrorInvalidConfiguration for a `variant` whose kernel has no soft form (the header lists them).
template <class T, bool SOFT>
hipError_t launch_decode_ms(int code, int variant, const T *llrs, T *app, uint8_t *output, uint32_t *iters,
                            uint8_t *success, size_t batch, uint32_t maxiters, hipStream_t stream);

// Will launch_decode_ms<T, false>(code, variant, ...) read every LLR from memory exactly once?  (false for explicit variants, which
// are not second-guessed, and for forced two-pass NaN handling, whose second kernel reads the first one's marks.)
template <class T>
bool decode_ms_reads_llrs_once(int code, int variant);

const char *decode_ms_i8_kernel_name(int code, int variant, size_t batch);      // decode_ms_i8.hip

// The bit-sliced i8 flooding kernels of the TM codes with normalized / offset check messages (decode_ms_bs_corrected.hip, DESIGN.md
// 4.14): every stored row minimum m becomes max(((scale_num * m + ((1 << scale_shift) >> 1)) >> scale_shift) - offset, 0); the three
// are the caller's, already range-checked (capi.hip).  The bit-sliced kernel at every batch size, lockstep forms; llrs and output
// 4-byte aligned (the caller checks).  hipErrorInvalidConfiguration for a TC code.
hipError_t launch_decode_ms_bitsliced_corrected(int code, const int8_t *llrs, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                                uint32_t maxiters, uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                                                hipStream_t stream);

// The bit-sliced i8 flooding kernels of the one-wave TM codes with soft output (decode_ms_bs_soft.hip): app [batch][n + p]
// i8, the saturating marginals, beside the three hard results.  The lockstep soft kernel at every batch size; llrs and output 4-byte,
// app 16-byte aligned (the caller checks).  hipErrorInvalidConfiguration for any other code (bs::bitsliced_soft_code).
hipError_t launch_decode_ms_bitsliced_soft(int code, const int8_t *llrs, int8_t *app, uint8_t *output, uint32_t *iters, uint8_t *success,
                                           size_t batch, uint32_t maxiters, hipStream_t stream);

// The same kernels with normalized / offset check messages as well (decode_ms_bs_corrected_soft.hip): app is the
// saturating marginal of the corrected decoder at the caller's triple (already range-checked), the hard three are
// launch_decode_ms_bitsliced_corrected's.  The identity triple runs the offset-only form.  Alignments and codes as above.
hipError_t launch_decode_ms_bitsliced_corrected_soft(int code, const int8_t *llrs, int8_t *app, uint8_t *output, uint32_t *iters,
                                                     uint8_t *success, size_t batch, uint32_t maxiters, uint32_t scale_num,
                                                     uint32_t scale_shift, uint32_t offset, hipStream_t stream);

// The bit-sliced i8 flooding kernels of the one-wave TM codes reading f32 LLRs (decode_ms_bs_quantised.hip): the loader
// quantises every LLR to i8 by the rule of llr_quantise.hpp at (scale, lim), already range-checked; per frame the three results are
// those of the i8 kernel -- plain, or corrected at the caller's triple -- on the frame quantised that way.  Lockstep kernels at every
// batch size; llrs 16-byte, output 4-byte aligned (the caller checks).  hipErrorInvalidConfiguration for any other code
// (bs::bitsliced_soft_code) and in a 16-plane experiment build.
hipError_t launch_decode_ms_bitsliced_quantised(int code, const float *llrs, uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                                uint32_t maxiters, float scale, int lim, hipStream_t stream);
hipError_t launch_decode_ms_bitsliced_quantised_corrected(int code, const float *llrs, uint8_t *output, uint32_t *iters, uint8_t *success,
                                                          size_t batch, uint32_t maxiters, float scale, int lim, uint32_t scale_num,
                                                          uint32_t scale_shift, uint32_t offset, hipStream_t stream);

// The bit-sliced i8 flooding kernels of the one-wave TM codes reading PACKED HARD DECISIONS (decode_ms_bs_hard.hip):
// input [batch][n / 8] packed bits MSB first, erasures nullptr or the same shape; the loader builds the planes of the i8 frame that is 0
// where erased, else -magnitude where the bit is set, else +magnitude (1 .. 127, already range-checked); per frame the three results are
// those of the i8 kernel -- plain, or corrected at the caller's triple -- on that frame.  Lockstep kernels at every batch size; input,
// erasures and output 4-byte aligned (the caller checks input and erasures at 4, output at 8).  hipErrorInvalidConfiguration for any other code (bs::bitsliced_soft_code)
// and in a 16-plane experiment build.
hipError_t launch_decode_ms_bitsliced_hard(int code, const uint8_t *input, const uint8_t *erasures, uint8_t *output, uint32_t *iters,
                                           uint8_t *success, size_t batch, uint32_t maxiters, uint32_t magnitude, hipStream_t stream);
hipError_t launch_decode_ms_bitsliced_hard_corrected(int code, const uint8_t *input, const uint8_t *erasures, uint8_t *output, uint32_t *iters,
                                                     uint8_t *success, size_t batch, uint32_t maxiters, uint32_t magnitude, uint32_t scale_num,
                                                     uint32_t scale_shift, uint32_t offset, hipStream_t stream);

// ... with soft output as well (decode_ms_bs_quantised_soft.hip): the four results are those of
// launch_decode_ms_bitsliced_soft / launch_decode_ms_bitsliced_corrected_soft on the frame quantised that way, app [batch][n + p] i8
// 16-byte aligned.
hipError_t launch_decode_ms_bitsliced_quantised_soft(int code, const float *llrs, int8_t *app, uint8_t *output, uint32_t *iters,
                                                     uint8_t *success, size_t batch, uint32_t maxiters, float scale, int lim, hipStream_t stream);
hipError_t launch_decode_ms_bitsliced_quantised_corrected_soft(int code, const float *llrs, int8_t *app, uint8_t *output, uint32_t *iters,
                                                               uint8_t *success, size_t batch, uint32_t maxiters, float scale, int lim,
                                                               uint32_t scale_num, uint32_t scale_shift, uint32_t offset, hipStream_t stream);

// The flooding schedule on f32 LLRs with normalized / offset check messages (decode_ms_flooding_corrected_f32.hip):
// the code's default f32 kernel with the correction step; scale and offset are the caller's, already range-checked (capi.hip).
// app == nullptr launches the hard form.  `variant` 0 only: anything else is hipErrorInvalidConfiguration (EUNSUPPORTED).
hipError_t launch_decode_ms_flooding_corrected(int code, int variant, const float *llrs, float *app, uint8_t *output, uint32_t *iters,
                                               uint8_t *success, size_t batch, uint32_t maxiters, float scale, float offset,
                                               hipStream_t stream);

// The layered schedule (decode_ms_layered_f32.hip).  app == nullptr launches the hard form.  `variant` 0 is the only kernel of every
// layered launcher: anything else is hipErrorInvalidConfiguration (EUNSUPPORTED).
hipError_t launch_decode_ms_layered(int code, int variant, const float *llrs, float *app, uint8_t *output, uint32_t *iters,
                                    uint8_t *success, size_t batch, uint32_t maxiters, hipStream_t stream);
// ... with normalized / offset check messages (decode_ms_corrected_f32.hip): scale and offset are the caller's, already
// range-checked (capi.hip)
hipError_t launch_decode_ms_layered_corrected(int code, int variant, const float *llrs, float *app, uint8_t *output, uint32_t *iters,
                                              uint8_t *success, size_t batch, uint32_t maxiters, float scale, float offset,
                                              hipStream_t stream);
// ... in fixed point (decode_ms_fixed_layered.hip), T = int8_t / int16_t: the marginals are int32
template <class T>
hipError_t launch_decode_ms_layered_fixed(int code, int variant, const T *llrs, int32_t *app, uint8_t *output, uint32_t *iters,
                                          uint8_t *success, size_t batch, uint32_t maxiters, hipStream_t stream);
// ... in fixed point with normalized / offset check messages (decode_ms_fixed_corrected.hip): every message magnitude m becomes
// max(((scale_num * m + ((1 << scale_shift) >> 1)) >> scale_shift) - offset, 0); the three are the caller's, already range-checked
// (capi.hip)
template <class T>
hipError_t launch_decode_ms_layered_fixed_corrected(int code, int variant, const T *llrs, int32_t *app, uint8_t *output, uint32_t *iters,
                                                    uint8_t *success, size_t batch, uint32_t maxiters, uint32_t scale_num,
                                                    uint32_t scale_shift, uint32_t offset, hipStream_t stream);
// ... in fixed point from f32 LLRs (decode_ms_fixed_quantised.hip): the loader quantises every LLR to T by the rule of
// llr_quantise.hpp at (scale, lim); `corrected` chooses the form with the correction step, else the triple is not read
template <class T>
hipError_t launch_decode_ms_layered_fixed_quantised(int code, int variant, const float *llrs, int32_t *app, uint8_t *output,
                                                    uint32_t *iters, uint8_t *success, size_t batch, uint32_t maxiters, float scale,
                                                    int lim, bool corrected, uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                                                    hipStream_t stream);
// ... the f32 layered schedule from f16 / bf16 LLRs (decode_ms_half_layered.hip), H = f16_llr / bf16_llr: the loader widens every
// LLR by the rule of llr_widen.hpp; always the form with the correction step, (1, 0) for the plain entries
template <class H>
hipError_t launch_decode_ms_half_layered(int code, int variant, const H *llrs, float *app, uint8_t *output, uint32_t *iters,
                                         uint8_t *success, size_t batch, uint32_t maxiters, float scale, float offset, hipStream_t stream);

}  // namespace ldpc
