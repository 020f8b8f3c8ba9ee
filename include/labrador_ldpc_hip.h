/* labrador_ldpc_hip.h -- C ABI of liblabrador_ldpc_hip.so, the MI355X (gfx950) min-sum decoder.
 *
 * Drop-in boundary for the decode_ms path of adamgreig/labrador-ldpc.  The first part mirrors
 * the reference's C API symbol for symbol (reference: capi/include/labrador_ldpc.h,
 * implemented in capi/src/lib.rs); the second part adds the batched entry points the GPU
 * path sits behind.  All paths below are relative to the reference repository.
 *
 * Conventions kept from the reference (capi/README.md:84-101, src/lib.rs:15-17):
 *   - the caller owns every buffer; lengths are implied by `code`, never passed;
 *   - packed bit buffers are MSB-first inside each byte (src/decoder.rs:459, :490, :506);
 *   - functions are re-entrant; concurrent calls on disjoint buffers are safe.
 * Differences, all deliberate:
 *   - an out-of-range `code` is undefined behaviour in the reference (it is the Rust enum
 *     itself, src/codes/mod.rs:37-66); here size queries return 0, decoders return false /
 *     a negative status and write nothing;
 *   - decode_ms runs on the GPU.  If no usable HIP device or kernel is available the
 *     decoders FAIL (false / negative status, message via labrador_ldpc_hip_last_error());
 *     there is no CPU fallback for the hot path;
 *   - the `working` / `working_u8` arguments of the single-codeword decoders are accepted
 *     for source compatibility and not touched (all message state lives in GPU registers/LDS).
 */
#ifndef LABRADOR_LDPC_HIP_H
#define LABRADOR_LDPC_HIP_H

#include <stddef.h>
#include <stdint.h>
#include <stdbool.h>

#ifdef __cplusplus
extern "C" {
#endif

/* capi/include/labrador_ldpc.h:19-29 == #[repr(C)] enum LDPCCode, src/codes/mod.rs:37-66 */
enum labrador_ldpc_code {
    LABRADOR_LDPC_CODE_TC128    = 0,
    LABRADOR_LDPC_CODE_TC256    = 1,
    LABRADOR_LDPC_CODE_TC512    = 2,
    LABRADOR_LDPC_CODE_TM1280   = 3,
    LABRADOR_LDPC_CODE_TM1536   = 4,
    LABRADOR_LDPC_CODE_TM2048   = 5,
    LABRADOR_LDPC_CODE_TM5120   = 6,
    LABRADOR_LDPC_CODE_TM6144   = 7,
    LABRADOR_LDPC_CODE_TM8192   = 8,
};

/* --------------------------------------------------------------------------------------
 * Compile-time sizes for static allocation (capi/include/labrador_ldpc.h:30-115; used by the
 * reference's C client capi/examples/example.c:23-37).  Every quantity Q in
 *   N  K  BF_WORKING_LEN  MS_WORKING_LEN  MS_WORKING_U8_LEN  OUTPUT_LEN
 * is available as LABRADOR_LDPC_<Q>_<code> and as LABRADOR_LDPC_<Q>(CODE), where CODE may itself
 * be a macro naming a code (two-level expansion), and LABRADOR_LDPC_CODE(CODE) gives the enum
 * constant.  Values follow src/codes/mod.rs:109-241 / src/decoder.rs:93-116:
 *   BF_WORKING_LEN = n+p, MS_WORKING_LEN = 2E+3n+3p-2k, MS_WORKING_U8_LEN = (n+p-k)/8,
 *   OUTPUT_LEN = (n+p)/8
 * and are checked against the labrador_ldpc_*_len() functions by tests/test_c_boundary.py.
 * Reference quirks: its header spells the TM6144 entries of the four *_LEN families "_TM6140"
 * (labrador_ldpc.h:76,:88,:100,:112) and gives LABRADOR_LDPC_N_TM6144 the value 6140 (:52), which
 * is wrong (n = 6144, src/codes/mod.rs:203-213).  Here the _TM6140 spellings are kept as aliases
 * so existing sources compile, _TM6144 spellings are added so the (CODE) forms work for TM6144,
 * and N_TM6144 carries the correct value 6144.
 * -------------------------------------------------------------------------------------- */
#define LABRADOR_LDPC_PASTE_(FAMILY, CODE)   FAMILY##CODE
#define LABRADOR_LDPC_CODE(CODE)              LABRADOR_LDPC_PASTE_(LABRADOR_LDPC_CODE_, CODE)
#define LABRADOR_LDPC_N(CODE)                 LABRADOR_LDPC_PASTE_(LABRADOR_LDPC_N_, CODE)
#define LABRADOR_LDPC_K(CODE)                 LABRADOR_LDPC_PASTE_(LABRADOR_LDPC_K_, CODE)
#define LABRADOR_LDPC_BF_WORKING_LEN(CODE)    LABRADOR_LDPC_PASTE_(LABRADOR_LDPC_BF_WORKING_LEN_, CODE)
#define LABRADOR_LDPC_MS_WORKING_LEN(CODE)    LABRADOR_LDPC_PASTE_(LABRADOR_LDPC_MS_WORKING_LEN_, CODE)
#define LABRADOR_LDPC_MS_WORKING_U8_LEN(CODE) LABRADOR_LDPC_PASTE_(LABRADOR_LDPC_MS_WORKING_U8_LEN_, CODE)
#define LABRADOR_LDPC_OUTPUT_LEN(CODE)        LABRADOR_LDPC_PASTE_(LABRADOR_LDPC_OUTPUT_LEN_, CODE)
/* the reference's one-argument helper spellings (labrador_ldpc.h:42, :53, ...), kept for sources that use them */
#define LABRADOR_LDPC_CODE_(CODE)              LABRADOR_LDPC_CODE_##CODE
#define LABRADOR_LDPC_N_(CODE)                 LABRADOR_LDPC_N_##CODE
#define LABRADOR_LDPC_K_(CODE)                 LABRADOR_LDPC_K_##CODE
#define LABRADOR_LDPC_BF_WORKING_LEN_(CODE)    LABRADOR_LDPC_BF_WORKING_LEN_##CODE
#define LABRADOR_LDPC_MS_WORKING_LEN_(CODE)    LABRADOR_LDPC_MS_WORKING_LEN_##CODE
#define LABRADOR_LDPC_MS_WORKING_U8_LEN_(CODE) LABRADOR_LDPC_MS_WORKING_U8_LEN_##CODE
#define LABRADOR_LDPC_OUTPUT_LEN_(CODE)        LABRADOR_LDPC_OUTPUT_LEN_##CODE

/* TC128: n=128 k=64 punctured=0 edges=512 */
#define LABRADOR_LDPC_N_TC128                   (128)
#define LABRADOR_LDPC_K_TC128                   (64)
#define LABRADOR_LDPC_BF_WORKING_LEN_TC128      (128)
#define LABRADOR_LDPC_MS_WORKING_LEN_TC128      (1280)
#define LABRADOR_LDPC_MS_WORKING_U8_LEN_TC128   (8)
#define LABRADOR_LDPC_OUTPUT_LEN_TC128          (16)

/* TC256: n=256 k=128 punctured=0 edges=1024 */
#define LABRADOR_LDPC_N_TC256                   (256)
#define LABRADOR_LDPC_K_TC256                   (128)
#define LABRADOR_LDPC_BF_WORKING_LEN_TC256      (256)
#define LABRADOR_LDPC_MS_WORKING_LEN_TC256      (2560)
#define LABRADOR_LDPC_MS_WORKING_U8_LEN_TC256   (16)
#define LABRADOR_LDPC_OUTPUT_LEN_TC256          (32)

/* TC512: n=512 k=256 punctured=0 edges=2048 */
#define LABRADOR_LDPC_N_TC512                   (512)
#define LABRADOR_LDPC_K_TC512                   (256)
#define LABRADOR_LDPC_BF_WORKING_LEN_TC512      (512)
#define LABRADOR_LDPC_MS_WORKING_LEN_TC512      (5120)
#define LABRADOR_LDPC_MS_WORKING_U8_LEN_TC512   (32)
#define LABRADOR_LDPC_OUTPUT_LEN_TC512          (64)

/* TM1280: n=1280 k=1024 punctured=128 edges=4992 */
#define LABRADOR_LDPC_N_TM1280                  (1280)
#define LABRADOR_LDPC_K_TM1280                  (1024)
#define LABRADOR_LDPC_BF_WORKING_LEN_TM1280     (1408)
#define LABRADOR_LDPC_MS_WORKING_LEN_TM1280     (12160)
#define LABRADOR_LDPC_MS_WORKING_U8_LEN_TM1280  (48)
#define LABRADOR_LDPC_OUTPUT_LEN_TM1280         (176)

/* TM1536: n=1536 k=1024 punctured=256 edges=5888 */
#define LABRADOR_LDPC_N_TM1536                  (1536)
#define LABRADOR_LDPC_K_TM1536                  (1024)
#define LABRADOR_LDPC_BF_WORKING_LEN_TM1536     (1792)
#define LABRADOR_LDPC_MS_WORKING_LEN_TM1536     (15104)
#define LABRADOR_LDPC_MS_WORKING_U8_LEN_TM1536  (96)
#define LABRADOR_LDPC_OUTPUT_LEN_TM1536         (224)

/* TM2048: n=2048 k=1024 punctured=512 edges=7680 */
#define LABRADOR_LDPC_N_TM2048                  (2048)
#define LABRADOR_LDPC_K_TM2048                  (1024)
#define LABRADOR_LDPC_BF_WORKING_LEN_TM2048     (2560)
#define LABRADOR_LDPC_MS_WORKING_LEN_TM2048     (20992)
#define LABRADOR_LDPC_MS_WORKING_U8_LEN_TM2048  (192)
#define LABRADOR_LDPC_OUTPUT_LEN_TM2048         (320)

/* TM5120: n=5120 k=4096 punctured=512 edges=19968 */
#define LABRADOR_LDPC_N_TM5120                  (5120)
#define LABRADOR_LDPC_K_TM5120                  (4096)
#define LABRADOR_LDPC_BF_WORKING_LEN_TM5120     (5632)
#define LABRADOR_LDPC_MS_WORKING_LEN_TM5120     (48640)
#define LABRADOR_LDPC_MS_WORKING_U8_LEN_TM5120  (192)
#define LABRADOR_LDPC_OUTPUT_LEN_TM5120         (704)

/* TM6144: n=6144 k=4096 punctured=1024 edges=23552 */
#define LABRADOR_LDPC_N_TM6144                  (6144)
#define LABRADOR_LDPC_K_TM6144                  (4096)
#define LABRADOR_LDPC_BF_WORKING_LEN_TM6144     (7168)
#define LABRADOR_LDPC_MS_WORKING_LEN_TM6144     (60416)
#define LABRADOR_LDPC_MS_WORKING_U8_LEN_TM6144  (384)
#define LABRADOR_LDPC_OUTPUT_LEN_TM6144         (896)
/* reference spellings of the four entries above (labrador_ldpc.h:76, :88, :100, :112) */
#define LABRADOR_LDPC_BF_WORKING_LEN_TM6140     LABRADOR_LDPC_BF_WORKING_LEN_TM6144
#define LABRADOR_LDPC_MS_WORKING_LEN_TM6140     LABRADOR_LDPC_MS_WORKING_LEN_TM6144
#define LABRADOR_LDPC_MS_WORKING_U8_LEN_TM6140  LABRADOR_LDPC_MS_WORKING_U8_LEN_TM6144
#define LABRADOR_LDPC_OUTPUT_LEN_TM6140         LABRADOR_LDPC_OUTPUT_LEN_TM6144

/* TM8192: n=8192 k=4096 punctured=2048 edges=30720 */
#define LABRADOR_LDPC_N_TM8192                  (8192)
#define LABRADOR_LDPC_K_TM8192                  (4096)
#define LABRADOR_LDPC_BF_WORKING_LEN_TM8192     (10240)
#define LABRADOR_LDPC_MS_WORKING_LEN_TM8192     (83968)
#define LABRADOR_LDPC_MS_WORKING_U8_LEN_TM8192  (768)
#define LABRADOR_LDPC_OUTPUT_LEN_TM8192         (1280)

/* ======================================================================================
 * Part 1 -- the reference's 21 symbols, same names, signatures and meaning.
 * ====================================================================================== */

/* capi/include/labrador_ldpc.h:118, :121  (capi/src/lib.rs:15-23) */
size_t labrador_ldpc_code_n(enum labrador_ldpc_code code);
size_t labrador_ldpc_code_k(enum labrador_ldpc_code code);

/* capi/include/labrador_ldpc.h:124-135  (capi/src/lib.rs:48-66; src/decoder.rs:93-116) */
size_t labrador_ldpc_bf_working_len(enum labrador_ldpc_code code);
size_t labrador_ldpc_ms_working_u8_len(enum labrador_ldpc_code code);
size_t labrador_ldpc_ms_working_len(enum labrador_ldpc_code code);
size_t labrador_ldpc_output_len(enum labrador_ldpc_code code);

/* capi/include/labrador_ldpc.h:143, :151-152  (capi/src/lib.rs:25-46; src/encoder.rs:293-315).
 * Host-side systematic encoder: first k/8 bytes are data, the rest is written with parity. */
void labrador_ldpc_encode(enum labrador_ldpc_code code, uint8_t *codeword);
void labrador_ldpc_copy_encode(enum labrador_ldpc_code code, const uint8_t *data, uint8_t *codeword);

/* capi/include/labrador_ldpc.h:167-170  (capi/src/lib.rs:68-81; src/decoder.rs:243-301).
 * Bit-flipping decoder (with the erasure pre-pass for punctured codes), one codeword, host
 * pointers, on the GPU.  `input` n/8 bytes, `output` output_len bytes, `working` is accepted and
 * not touched, `iters_run` may be NULL. */
bool labrador_ldpc_decode_bf(enum labrador_ldpc_code code, const uint8_t *input, uint8_t *output,
                             uint8_t *working, size_t max_iters, size_t *iters_run);

/* capi/include/labrador_ldpc.h:193-208  (capi/src/lib.rs:83-127; src/decoder.rs:347-475).
 * One codeword, host pointers; runs the same kernels as the batched calls with batch = 1
 * (every LLR type incl. f64: the register-resident kernels).
 * `llrs` n entries, `output` output_len bytes, `iters_run` may be NULL. */
bool labrador_ldpc_decode_ms_i8 (enum labrador_ldpc_code code, const int8_t  *llrs, uint8_t *output,
                                 int8_t  *working, uint8_t *working_u8, size_t max_iters, size_t *iters_run);
bool labrador_ldpc_decode_ms_i16(enum labrador_ldpc_code code, const int16_t *llrs, uint8_t *output,
                                 int16_t *working, uint8_t *working_u8, size_t max_iters, size_t *iters_run);
bool labrador_ldpc_decode_ms_f32(enum labrador_ldpc_code code, const float   *llrs, uint8_t *output,
                                 float   *working, uint8_t *working_u8, size_t max_iters, size_t *iters_run);
bool labrador_ldpc_decode_ms_f64(enum labrador_ldpc_code code, const double  *llrs, uint8_t *output,
                                 double  *working, uint8_t *working_u8, size_t max_iters, size_t *iters_run);

/* decode_ms::<i32> (src/decoder.rs:60-68): the crate's generic accepts i32 LLRs; the reference's C API does
 * not export it (capi/src/lib.rs:97-127 stops at i8/i16/f32/f64).  Same contract as the four above, with the
 * i32 forms of the LLR helpers below and labrador_ldpc_decode_ms_batch_i32 in part 2. */
bool labrador_ldpc_decode_ms_i32(enum labrador_ldpc_code code, const int32_t *llrs, uint8_t *output,
                                 int32_t *working, uint8_t *working_u8, size_t max_iters, size_t *iters_run);
void labrador_ldpc_hard_to_llrs_i32(enum labrador_ldpc_code code, const uint8_t *input, int32_t *llrs);
void labrador_ldpc_llrs_to_hard_i32(enum labrador_ldpc_code code, const int32_t *llrs, uint8_t *output);

/* capi/include/labrador_ldpc.h:219-226  (capi/src/lib.rs:129-153; src/decoder.rs:484-493) */
void labrador_ldpc_hard_to_llrs_i8 (enum labrador_ldpc_code code, const uint8_t *input, int8_t  *llrs);
void labrador_ldpc_hard_to_llrs_i16(enum labrador_ldpc_code code, const uint8_t *input, int16_t *llrs);
void labrador_ldpc_hard_to_llrs_f32(enum labrador_ldpc_code code, const uint8_t *input, float   *llrs);
void labrador_ldpc_hard_to_llrs_f64(enum labrador_ldpc_code code, const uint8_t *input, double  *llrs);

/* capi/include/labrador_ldpc.h:237-244  (capi/src/lib.rs:155-179; src/decoder.rs:498-509) */
void labrador_ldpc_llrs_to_hard_i8 (enum labrador_ldpc_code code, const int8_t  *llrs, uint8_t *output);
void labrador_ldpc_llrs_to_hard_i16(enum labrador_ldpc_code code, const int16_t *llrs, uint8_t *output);
void labrador_ldpc_llrs_to_hard_f32(enum labrador_ldpc_code code, const float   *llrs, uint8_t *output);
void labrador_ldpc_llrs_to_hard_f64(enum labrador_ldpc_code code, const double  *llrs, uint8_t *output);

/* ======================================================================================
 * Part 2 -- batched GPU entry points (no counterpart in the reference; what a caller that
 * loops over labrador_ldpc_decode_ms_* per frame, e.g. perftest/src/main.rs:9-29, moves to).
 * ====================================================================================== */

/* status codes */
#define LABRADOR_LDPC_HIP_OK            0
#define LABRADOR_LDPC_HIP_EINVAL      (-1)   /* bad code / NULL pointer / misaligned buffer */
#define LABRADOR_LDPC_HIP_ENODEV      (-2)   /* no HIP device, or the device is not gfx950 */
#define LABRADOR_LDPC_HIP_ERUNTIME    (-3)   /* a HIP runtime call failed */
#define LABRADOR_LDPC_HIP_EUNSUPPORTED (-4)  /* valid request this build has no kernel for */

#define LABRADOR_LDPC_HIP_MEM_HOST    0      /* buffers are host memory; the call stages them */
#define LABRADOR_LDPC_HIP_MEM_DEVICE  1      /* buffers are device memory resident on `device` */

#define LABRADOR_LDPC_HIP_DEVICE_CURRENT (-1)  /* the calling thread's current HIP device */
#define LABRADOR_LDPC_HIP_DEVICE_ALL     (-2)  /* MEM_HOST only: shard the batch over every gfx950 device */

/* ABI of the batched entry points.  3 = `struct labrador_ldpc_hip_opts` starts with `struct_size` (this header).
 * (1 = the 24-byte struct of library 0.1.0, 2 = 0.2.0's 32-byte struct with n_devices / devices appended and no way for the
 * library to tell the two apart -- a 0.1.0 client handed 0.2.0 its padding as n_devices.  Both are gone: the shared object
 * carries the soname liblabrador_ldpc_hip.so.3, and labrador_ldpc_hip_abi_version() lets a dlopen() client check.) */
#define LABRADOR_LDPC_HIP_ABI 3

/* Zero-initialise, then set what you need: `struct labrador_ldpc_hip_opts o = {0};` means device 0, host memory, default
 * stream, tuned kernel.  `struct_size` is what makes the struct growable: the library reads a field only if it lies inside
 * the first `struct_size` bytes and takes every field beyond as zero, so a client built against THIS header keeps working
 * with a later library whose struct has grown.  0 (what `= {0}` leaves) stands for this header's layout up to and
 * including `devices`; LABRADOR_LDPC_HIP_OPTS_INIT sets it to the client's own sizeof, which is what a client should use
 * from now on. */
struct labrador_ldpc_hip_opts {
    size_t struct_size; /* sizeof(struct labrador_ldpc_hip_opts) as the CALLER compiled it, or 0 (see above) */
    int   device;     /* HIP device ordinal, LABRADOR_LDPC_HIP_DEVICE_CURRENT or _ALL */
    int   memory;     /* LABRADOR_LDPC_HIP_MEM_HOST or _DEVICE */
    void *stream;     /* hipStream_t to launch on; NULL = the default stream.  With MEM_DEVICE
                         the call only enqueues work and returns (asynchronous); with MEM_HOST
                         it returns after the results are in the host buffers. */
    int   variant;    /* enum labrador_ldpc_hip_variant below; 0 = the tuned default.  Every variant returns identical results. */
    int   n_devices;  /* > 0: shard a MEM_HOST batch over devices[0 .. n_devices) (`device` is ignored) */
    const int *devices; /* HIP ordinals; an ordinal may repeat (that many host pipelines on it, at most four at a time: further
                           repeats queue behind them) */
};
#define LABRADOR_LDPC_HIP_OPTS_INIT { sizeof(struct labrador_ldpc_hip_opts) }

/* `variant`: which of the library's decode_ms kernels a batched call runs.  0 is what callers want; the others exist so that the
 * tuned choice can be A/B-ed against its alternatives (all return identical results; a value that was not built for the code and
 * LLR type yields LABRADOR_LDPC_HIP_EUNSUPPORTED).  One kernel value, optionally OR-ed with flags. */
enum labrador_ldpc_hip_variant {
    LABRADOR_LDPC_HIP_VARIANT_DEFAULT       = 0,    /* the tuned kernel for (code, LLR type, batch size) */
    LABRADOR_LDPC_HIP_VARIANT_IPT1          = 1,    /* f32-pipe kernel (messages as f32 / f64 / i32 registers), one index per thread */
    LABRADOR_LDPC_HIP_VARIANT_IPT2          = 2,    /* ... two indices per thread (t, t + M/2) */
    LABRADOR_LDPC_HIP_VARIANT_IPT4          = 4,    /* ... four */
    LABRADOR_LDPC_HIP_VARIANT_LEAN          = 16,   /* OR-ed with IPTn: the register-lean check phase (one check row at a time) */
    LABRADOR_LDPC_HIP_VARIANT_PAIR          = 32,   /* adjacent-index pair ownership (TM8192, TM2048); f64: OR-ed with IPTn = in-place messages */
    LABRADOR_LDPC_HIP_VARIANT_BITSLICE      = 64,   /* i8 LLRs, TM codes: the bit-sliced kernel whatever the batch size */
    LABRADOR_LDPC_HIP_VARIANT_F64_WORKSPACE = 100,  /* f64: the general kernel with its messages in a device workspace */
    /* flags */
    LABRADOR_LDPC_HIP_VARIANT_STATIC        = 256,  /* fixed-stride distribution of the codewords instead of the launch's queue; with
                                                       BITSLICE: the lockstep kernel instead of the slot-refill one (TM1536, TM1280: by
                                                       name at any batch size, in the default dispatch from 65 536 frames up) */
    LABRADOR_LDPC_HIP_VARIANT_NAN_ONE_PASS  = 512,  /* TM5120 / TM1280 f32: NaN LLRs handled inside the one kernel ... */
    LABRADOR_LDPC_HIP_VARIANT_NAN_TWO_PASS  = 1024  /* ... or by a second launch over marked codewords (the default from ~1000 frames) */
};

/* Multi-GPU (the reference's analogue is perftest/src/main.rs:39-45, one worker per
 * core over independent frames): with MEM_HOST buffers and a device set -- `device` ==
 * LABRADOR_LDPC_HIP_DEVICE_ALL or a `devices` list -- the batched calls split the batch into
 * contiguous slices (labrador_ldpc_hip_shard_range), one per listed device, and run every slice
 * through that device's own copy/kernel/copy pipeline on a worker thread of the library.  No data
 * moves between devices and there is no collective; results land in the caller's buffers exactly
 * as in the single-device call.  `stream` must be NULL.  The first failing slice's status is
 * returned (its text, prefixed with the device, via labrador_ldpc_hip_last_error()). */

/* Decode `batch` independent frames.
 *   llrs    [batch][n]            row-major, n = labrador_ldpc_code_n(code)
 *   output  [batch][output_len]   hard bits incl. punctured parity, MSB first
 *   iters   [batch]               0-based index of the converging iteration, or max_iters
 *   success [batch]               1 if all parity checks were satisfied, else 0
 * Per frame the three results equal what labrador_ldpc_decode_ms_* returns for that frame.
 * `opts` may be NULL (host memory, current device, default stream).  With MEM_DEVICE,
 * `output` must be 8-byte aligned.  Returns a status code. */
int labrador_ldpc_decode_ms_batch_f32(enum labrador_ldpc_code code, const float *llrs, uint8_t *output,
                                      uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                      const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_batch_i8 (enum labrador_ldpc_code code, const int8_t *llrs, uint8_t *output,
                                      uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                      const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_batch_i16(enum labrador_ldpc_code code, const int16_t *llrs, uint8_t *output,
                                      uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                      const struct labrador_ldpc_hip_opts *opts);
/* i32 (src/decoder.rs:60-68): saturating 32-bit integer arithmetic on the GPU. */
int labrador_ldpc_decode_ms_batch_i32(enum labrador_ldpc_code code, const int32_t *llrs, uint8_t *output,
                                      uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                      const struct labrador_ldpc_hip_opts *opts);
/* f64: same results contract.  By default the register-resident kernels with 64-bit registers and LDS elements (plain for the
 * small codes, register-lean for TM2048 / TM5120, in-place messages for TM6144 / TM8192); `variant`
 * LABRADOR_LDPC_HIP_VARIANT_F64_WORKSPACE (100) names the general fallback that keeps the per-edge messages in a device workspace
 * allocated per call (10-100x slower; csrc/decode_ms_f64.hip). */
int labrador_ldpc_decode_ms_batch_f64(enum labrador_ldpc_code code, const double *llrs, uint8_t *output,
                                      uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                      const struct labrador_ldpc_hip_opts *opts);

/* Soft output: the same decode, returning besides the hard results the decoder's a-posteriori LLR (the marginal) of every variable.
 *   app     [batch][n + p]        app[f][j] = the reference's va[j] (src/decoder.rs:377, :382-383, :408) when decode_ms returns for
 *                                 frame f: the marginals of the converging iteration, or of iteration max_iters - 1 on failure;
 *                                 all zero for max_iters = 0 (:374).  n + p = labrador_ldpc_bf_working_len(code); punctured
 *                                 variables come last.  The LLR type: integer types saturate as the reference does (i8 reaches
 *                                 -128); float types equal the reference's values with -0.0 returned as +0.0, and hold a NaN
 *                                 exactly where the reference's va does -- at the NaN LLRs.
 *   output, iters, success        exactly as labrador_ldpc_decode_ms_batch_* (per frame, what the hard-only call returns).
 * Memory modes, device sets, `stream`, argument checks and `variant` as labrador_ldpc_decode_ms_batch_*; with MEM_DEVICE `app` must be
 * 16-byte aligned (and `output` 8-byte aligned).  Kernels (DESIGN.md "Soft output"):
 *   - f32, i16, i32: the soft forms of the hard-only call's kernels -- every variant that call accepts;
 *   - i8: the f32-pipe i8 kernels (those the hard-only call takes for unaligned buffers) whatever the batch size;
 *     LABRADOR_LDPC_HIP_VARIANT_BITSLICE (64) returns LABRADOR_LDPC_HIP_EUNSUPPORTED here: the bit-sliced kernels' soft form is an
 *     entry of its own, labrador_ldpc_decode_ms_bitsliced_soft_batch_i8 below (same results, the bit-sliced rate);
 *   - f64: the register kernels, except the in-place ones (variant | LABRADOR_LDPC_HIP_VARIANT_PAIR), which keep only the signs of
 *     most marginals: an explicit in-place variant returns LABRADOR_LDPC_HIP_EUNSUPPORTED, and TM8192, whose tuned f64 kernel is
 *     in place, runs the workspace kernel (LABRADOR_LDPC_HIP_VARIANT_F64_WORKSPACE) by default.
 * Returns a status code. */
int labrador_ldpc_decode_ms_soft_batch_f32(enum labrador_ldpc_code code, const float *llrs, float *app,
                                           uint8_t *output, uint32_t *iters, uint8_t *success,
                                           size_t batch, size_t max_iters, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_soft_batch_i8 (enum labrador_ldpc_code code, const int8_t *llrs, int8_t *app,
                                           uint8_t *output, uint32_t *iters, uint8_t *success,
                                           size_t batch, size_t max_iters, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_soft_batch_i16(enum labrador_ldpc_code code, const int16_t *llrs, int16_t *app,
                                           uint8_t *output, uint32_t *iters, uint8_t *success,
                                           size_t batch, size_t max_iters, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_soft_batch_i32(enum labrador_ldpc_code code, const int32_t *llrs, int32_t *app,
                                           uint8_t *output, uint32_t *iters, uint8_t *success,
                                           size_t batch, size_t max_iters, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_soft_batch_f64(enum labrador_ldpc_code code, const double *llrs, double *app,
                                           uint8_t *output, uint32_t *iters, uint8_t *success,
                                           size_t batch, size_t max_iters, const struct labrador_ldpc_hip_opts *opts);

/* Soft output from the BIT-SLICED i8 kernels.  Per frame, `app`, `output`, `iters` and `success` equal what
 * labrador_ldpc_decode_ms_soft_batch_i8 returns, bit for bit: the reference's va, saturating, reaching -128; all zero for
 * max_iters = 0.  The kernel is the lockstep bit-sliced kernel of the code in its soft form -- it keeps the seven magnitude planes of
 * every block column's marginal beside the hard word and turns them back into bytes at the end -- at EVERY batch size: no crossover to
 * the f32-pipe kernels, as for labrador_ldpc_decode_ms_corrected_batch_i8.
 * Codes: TM1536, TM2048, TM6144 and TM8192.  A TC code, and any `variant` but 0, return LABRADOR_LDPC_HIP_EUNSUPPORTED; so do TM1280
 * and TM5120, whose text says that the two-wave kernels have no soft form.
 * Rates on one MI355X (device-resident, 2 dB, cap 25), against labrador_ldpc_decode_ms_soft_batch_i8 on the same frames:
 *   TM8192 18.87 against 8.11 M codewords/s (2.33 x); TM2048 64.6 against 37.0 (1.75 x); TM6144 11.84 against 6.59 (1.80 x); TM1536
 *   46.7 against 33.4 (1.40 x) -- faster on all four, at 0.83 / 0.82 / 0.64 / 0.64 of the hard lockstep bit-sliced kernel's rate.
 * Order of the checks: code, empty batch (OK, touches nothing), NULL buffers -- `app` included -- (EINVAL), variant and code family
 * (EUNSUPPORTED) -- all before any device work.  With LABRADOR_LDPC_HIP_MEM_DEVICE `llrs` must be 4-byte, `output` 8-byte and `app`
 * 16-byte aligned (EINVAL); the input is always copied in.  Host buffers are staged with `app` as the fourth output; device sets
 * shard; asynchronous on opts->stream with MEM_DEVICE -- all as labrador_ldpc_decode_ms_soft_batch_i8.
 * The form with normalized / offset check messages is labrador_ldpc_decode_ms_bitsliced_corrected_soft_batch_i8 below.  There is no
 * _multi, single-frame, slot-refill or two-wave form; on f32 LLRs: labrador_ldpc_decode_ms_bitsliced_quantised_soft_batch_i8.  Returns
 * a status code. */
int labrador_ldpc_decode_ms_bitsliced_soft_batch_i8(enum labrador_ldpc_code code, const int8_t *llrs, int8_t *app, uint8_t *output,
                                                    uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                                    const struct labrador_ldpc_hip_opts *opts);

/* Soft output from the bit-sliced i8 kernels WITH normalized / offset check messages: the entry above at a triple.
 * Per frame, `output`, `iters` and `success` equal what labrador_ldpc_decode_ms_corrected_batch_i8 returns at the same
 * (scale_num, scale_shift, offset), bit for bit, and
 *   app  [batch][n + p] int8   is the marginal va of that corrected decoder: saturating, reaching -128; all zero for max_iters = 0;
 *                              punctured variables last.  A converged frame carries va of its converging iteration, any other frame va
 *                              of the last iteration.
 * The triple's meaning and ranges are labrador_ldpc_decode_ms_corrected_batch_i8's: scale_shift <= 8, 1 <= scale_num <= 1 <<
 * scale_shift, offset <= 127 (EINVAL otherwise).  At an identity triple -- (1, 0, 0), or any (1 << s, s, 0) -- the entry still runs
 * its own kernel, in the offset-only form, and all four results equal labrador_ldpc_decode_ms_bitsliced_soft_batch_i8's bit for bit.
 * Kernels: the lockstep soft kernels of TM1536, TM2048, TM6144 and TM8192 with the correction step, one form per multiplier width as
 * for the hard corrected entry, at every batch size.  Rates: DESIGN.md 4.18.
 * Order of the checks: code, empty batch (OK, touches nothing), NULL buffers -- `app` included -- (EINVAL), the triple (EINVAL),
 * variant and code family (EUNSUPPORTED, with the texts of labrador_ldpc_decode_ms_bitsliced_soft_batch_i8: TM1280 and TM5120 are told
 * that the two-wave kernels have no soft form) -- all before any device work.  With LABRADOR_LDPC_HIP_MEM_DEVICE `llrs` must be
 * 4-byte, `output` 8-byte and `app` 16-byte aligned (EINVAL).  Memory modes, device sets and `stream` as that entry.
 * There is no _multi, single-frame, slot-refill or two-wave form; on f32 LLRs:
 * labrador_ldpc_decode_ms_bitsliced_quantised_corrected_soft_batch_i8.  Returns a status code. */
int labrador_ldpc_decode_ms_bitsliced_corrected_soft_batch_i8(enum labrador_ldpc_code code, const int8_t *llrs, int8_t *app,
                                                              uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                                              size_t max_iters, uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                                                              const struct labrador_ldpc_hip_opts *opts);

/* Layered schedule (f32; for i8 and i16 LLRs see the fixed-point calls further down): block-row layered min-sum decoding instead
 * of the reference's flooding schedule.  Block row r of the prototype (a "layer": 4 for the TC codes, 3 for the TM codes) updates
 * its checks from marginals that already hold the new messages of rows 0 .. r-1 of the same sweep; a sweep is one pass over every
 * layer, and the decode stops at the first sweep whose marginals satisfy every check.  Same arithmetic as decode_ms::<f32> (plain IEEE adds and subtracts, self-correction, min-sum with the FLT_MAX
 * cap); DESIGN.md 4.5 states the semantics the results are pinned to.  Not the reference's iteration trace: fewer sweeps than its
 * iterations, and a lower frame error rate at the same cap.
 *   output      hard decisions of the returned sweep's marginals, as labrador_ldpc_decode_ms_batch_f32;
 *   iters       the 0-based index of the succeeding sweep, or max_iters on failure (0 for max_iters = 0);
 *   success     1 when every check is satisfied;
 *   app         (soft form) the marginals of the returned sweep, [batch][n + p]: -0.0 returned as +0.0, NaN exactly at NaN LLRs;
 *               all zero for max_iters = 0.
 * A NaN LLR gives the hard results of a +inf LLR.  Arguments, memory modes, device sets, `stream` and alignment rules as
 * labrador_ldpc_decode_ms_batch_f32 / labrador_ldpc_decode_ms_soft_batch_f32.  `variant` 0 is the only kernel; any other value returns
 * LABRADOR_LDPC_HIP_EUNSUPPORTED.  Returns a status code. */
int labrador_ldpc_decode_ms_layered_batch_f32(enum labrador_ldpc_code code, const float *llrs, uint8_t *output,
                                              uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                              const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_soft_batch_f32(enum labrador_ldpc_code code, const float *llrs, float *app,
                                                   uint8_t *output, uint32_t *iters, uint8_t *success,
                                                   size_t batch, size_t max_iters, const struct labrador_ldpc_hip_opts *opts);

/* Layered schedule with normalized / offset min-sum (f32; the fixed-point calls have their own form further down).
 * Plain min-sum overestimates the magnitude of a check message; these calls are the two layered calls above with one step added.
 * Where a layer forms an edge's new message, its magnitude m (min1 or min2 of the check, capped at FLT_MAX) becomes
 *     t  = scale * m         one IEEE f32 multiply, rounded
 *     t  = t - offset        one IEEE f32 subtract, rounded (never fused with the multiply)
 *     m' = t > 0 ? t : +0.0
 * and the signs are applied to m' as they are to m.  Which of min1 / min2 an edge takes is decided on the uncorrected values;
 * everything else (self-correction, accumulation order, LLR canonicalisation, the stop rule, iters, success, output, app,
 * max_iters = 0) is the layered contract unchanged.
 *   scale   0 < scale <= 1, unit-free ("normalized min-sum");
 *   offset  0 <= offset <= FLT_MAX ("offset min-sum"), in the UNITS OF THE LLRS: a value that suits LLRs of the form +-1 + noise does
 *           not suit the same frames scaled by 2 / sigma^2, and a value that helps one code and noise level can hurt at another.
 * One pair per call.  A NaN, an infinity or a value outside these ranges returns LABRADOR_LDPC_HIP_EINVAL (the message names the
 * parameter), decided with the other argument checks before any device work -- and before the batch is looked at, so an empty batch
 * with a bad pair is refused too (the fixed-point calls further down check their triple after the buffers, and an empty batch
 * returns OK whatever the triple).  With scale = 1 and offset = 0 the step is the identity
 * and the results equal those of the plain layered calls bit for bit, app included.  The library chooses no default: DESIGN.md 4.6
 * gives measured starting points.  Everything else as labrador_ldpc_decode_ms_layered_batch_f32 /
 * labrador_ldpc_decode_ms_layered_soft_batch_f32.  Returns a status code. */
int labrador_ldpc_decode_ms_layered_corrected_batch_f32(enum labrador_ldpc_code code, const float *llrs, uint8_t *output,
                                                        uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                                        float scale, float offset, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_corrected_soft_batch_f32(enum labrador_ldpc_code code, const float *llrs, float *app,
                                                             uint8_t *output, uint32_t *iters, uint8_t *success,
                                                             size_t batch, size_t max_iters, float scale, float offset,
                                                             const struct labrador_ldpc_hip_opts *opts);

/* Layered schedule in fixed point (i8 and i16 LLRs): the block-row layered schedule above for quantised LLRs, with a
 * contract of its own.  T_MAX is 127 (i8) or 32767 (i16).  An LLR is read as clamp(input, -T_MAX, T_MAX) (only the type's minimum
 * changes).  A marginal is the LLR (0 for a punctured variable) plus the check messages of the variable's edges, summed EXACTLY in
 * int32 (a variable has at most 6 edges, so |marginal| <= 7 * T_MAX and the order of the sum cannot matter).  Where a layer forms
 * an edge's new variable message, nv = clamp(marginal - u, -T_MAX, T_MAX) -- the only saturation of the decoder -- followed by the
 * self-correction of decode_ms; a check message is the exclusive minimum of the other |v| of its check (T_MAX where absent) with
 * their sign product.  Unlike decode_ms::<i8> / ::<i16>, no single add saturates: like the f32 layered calls this is not the
 * reference's iteration trace.
 *   output, iters, success   as the f32 layered calls;
 *   app         (soft form) the marginals of the returned sweep, ALWAYS int32, [batch][n + p]; all zero for max_iters = 0.
 * Arguments, memory modes, device sets, `stream` and alignment rules as the f32 layered calls (a device `app` 16-byte aligned).
 * `variant` 0 is the only kernel; any other value returns LABRADOR_LDPC_HIP_EUNSUPPORTED.  Returns a status code. */
int labrador_ldpc_decode_ms_layered_fixed_batch_i8(enum labrador_ldpc_code code, const int8_t *llrs, uint8_t *output,
                                                   uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                                   const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_fixed_batch_i16(enum labrador_ldpc_code code, const int16_t *llrs, uint8_t *output,
                                                    uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                                    const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_fixed_soft_batch_i8(enum labrador_ldpc_code code, const int8_t *llrs, int32_t *app,
                                                        uint8_t *output, uint32_t *iters, uint8_t *success,
                                                        size_t batch, size_t max_iters, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_fixed_soft_batch_i16(enum labrador_ldpc_code code, const int16_t *llrs, int32_t *app,
                                                         uint8_t *output, uint32_t *iters, uint8_t *success,
                                                         size_t batch, size_t max_iters, const struct labrador_ldpc_hip_opts *opts);

/* Fixed-point layered schedule with normalized / offset min-sum (i8 and i16): the four calls above with one step
 * added, in integers.  Where a layer forms an edge's new message, its magnitude m (min1 or min2 of the check, 0 <= m <= T_MAX) becomes
 *     t  = (scale_num * m + ((1 << scale_shift) >> 1)) >> scale_shift      exact in 32 bits; ROUND HALF UP (scale_shift = 0 adds nothing)
 *     m' = max(t - offset, 0)
 * and the signs are applied to m' as they are to m, a zero m' included.  Which of min1 / min2 an edge takes is decided on the
 * uncorrected values; everything else (the clamp of nv, self-correction, the exact int32 marginals, the stop rule, iters, success,
 * output, the int32 app, max_iters = 0) is the fixed-point layered contract unchanged.
 *   scale_shift  0 .. 8: the scale is the dyadic fraction scale_num / (1 << scale_shift);
 *   scale_num    1 .. 1 << scale_shift (a scale in (0, 1]);
 *   offset       0 .. T_MAX of the LLR type (127 / 32767), in the UNITS OF THE LLRS, which here are units of the caller's quantiser:
 *                an offset that helps one code and noise level can hurt at another.
 * One triple per call.  A value outside these ranges returns LABRADOR_LDPC_HIP_EINVAL (the message names the parameter), decided with
 * the other argument checks, after the buffers and before any device work.  m' <= m, so every bound of the fixed-point contract
 * holds.  (1 << k, k, 0) is the identity for every k: the results then equal those of the plain fixed-point calls bit for bit, app
 * included.  The library chooses no default: DESIGN.md 4.8 gives measured starting points (13 / 16 for i8 at 8 / 31).  Everything
 * else as the four calls above.  Returns a status code. */
int labrador_ldpc_decode_ms_layered_fixed_corrected_batch_i8(enum labrador_ldpc_code code, const int8_t *llrs, uint8_t *output,
                                                             uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                                             uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                                                             const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_fixed_corrected_batch_i16(enum labrador_ldpc_code code, const int16_t *llrs, uint8_t *output,
                                                              uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                                              uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                                                              const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_fixed_corrected_soft_batch_i8(enum labrador_ldpc_code code, const int8_t *llrs, int32_t *app,
                                                                  uint8_t *output, uint32_t *iters, uint8_t *success,
                                                                  size_t batch, size_t max_iters, uint32_t scale_num,
                                                                  uint32_t scale_shift, uint32_t offset,
                                                                  const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_fixed_corrected_soft_batch_i16(enum labrador_ldpc_code code, const int16_t *llrs, int32_t *app,
                                                                   uint8_t *output, uint32_t *iters, uint8_t *success,
                                                                   size_t batch, size_t max_iters, uint32_t scale_num,
                                                                   uint32_t scale_shift, uint32_t offset,
                                                                   const struct labrador_ldpc_hip_opts *opts);

/* Two-stage ("cascade") decoding: the flooding decoder first, the layered decoder on the frames it fails.  Per frame
 * f, exactly, as a composition of the entry points above:
 *     (o1, i1, s1) = labrador_ldpc_decode_ms_batch_<T> on frame f at cap max_iters, kernel opts->variant
 *     if s1:  output, iters, success, stage = o1, i1, 1, 0
 *     else:   (o2, i2, s2) = f32:      labrador_ldpc_decode_ms_layered_corrected_batch_f32 at (scale, offset)
 *                            i8 / i16: labrador_ldpc_decode_ms_layered_fixed_corrected_batch_<T> at (scale_num, scale_shift, offset)
 *                            on the ORIGINAL LLRs of frame f at cap max_sweeps, variant 0
 *             output, iters, success, stage = o2, i2, s2, 1
 *   stage   [batch]   which stage's results the frame carries: 0 = flooding, 1 = layered
 *   iters   [batch]   in that stage's own unit: the flooding decoder's 0-based iteration index, or the layered sweep index
 * A frame both stages fail carries stage 2's results: its last sweep's hard bits, iters = max_sweeps, success = 0.  max_iters = 0
 * sends every frame to stage 2 (the layered entry's results, stage all 1); max_sweeps = 0 gives every frame stage 1 failed the
 * layered entry's own answer to max_iters = 0: zero output, iters 0, success 0.  (1, 0) and (1 << k, k, 0) are the identity
 * corrections: plain layered min-sum.  `opts->variant` chooses the stage-1 kernel as in labrador_ldpc_decode_ms_batch_*; stage 2
 * has one kernel.  Hard output only; labrador_ldpc_decode_ms_cascade_soft_batch_* below add the marginals.
 * Arguments are checked in this order, all before any device work: `code`; for f32 the range of (scale, offset); an empty batch is
 * OK whatever the pointers; a NULL buffer, `stage` included, is EINVAL; for i8 / i16 the ranges of the triple.  With MEM_DEVICE
 * `output` must be 8-byte aligned; `llrs` need only be aligned to its element (a 16-byte aligned `llrs` is gathered faster).
 * With MEM_DEVICE the call is NOT purely asynchronous: it waits on opts->stream once per launch slice (2^30 frames) for the number
 * of frames stage 1 failed, and returns with the last slice's stage 2 and the copy of its results enqueued on that stream, so the
 * results are valid once the stream is synchronised, as for every other MEM_DEVICE call.  It must not be called on a stream that
 * is being captured into a graph.  Everything else (host buffers, device sets) as labrador_ldpc_decode_ms_batch_*.  Returns a
 * status code. */
int labrador_ldpc_decode_ms_cascade_batch_f32(enum labrador_ldpc_code code, const float *llrs, uint8_t *output, uint32_t *iters,
                                              uint8_t *success, uint8_t *stage, size_t batch, size_t max_iters, size_t max_sweeps,
                                              float scale, float offset, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_cascade_batch_i8 (enum labrador_ldpc_code code, const int8_t *llrs, uint8_t *output, uint32_t *iters,
                                              uint8_t *success, uint8_t *stage, size_t batch, size_t max_iters, size_t max_sweeps,
                                              uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                                              const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_cascade_batch_i16(enum labrador_ldpc_code code, const int16_t *llrs, uint8_t *output, uint32_t *iters,
                                              uint8_t *success, uint8_t *stage, size_t batch, size_t max_iters, size_t max_sweeps,
                                              uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                                              const struct labrador_ldpc_hip_opts *opts);

/* Flooding schedule with normalized / offset min-sum (f32 only): labrador_ldpc_decode_ms_batch_f32 and
 * labrador_ldpc_decode_ms_soft_batch_f32 -- the reference's decode_ms::<f32>, iteration for iteration -- with one step added.  Where an
 * iteration forms an edge's check message, its magnitude m (min2 of the check if |v| of the edge equals min1, else min1: the
 * previous iteration's minima, capped at FLT_MAX; zero in iteration 0) becomes
 *     t  = scale * m         one IEEE f32 multiply, rounded
 *     t  = t - offset        one IEEE f32 subtract, rounded (never fused with the multiply)
 *     m' = t > 0 ? t : +0.0
 * and the signs are applied to m' as they are to m.  Which of min1 / min2 an edge takes is decided on the uncorrected values;
 * everything else (self-correction, accumulation order, the NaN and -0.0 rules, the stop rule, iters as the 0-based index of the
 * converging iteration and max_iters on failure, success, output, app, max_iters = 0) is the flooding contract unchanged.
 *   scale   0 < scale <= 1, unit-free ("normalized min-sum");
 *   offset  0 <= offset <= FLT_MAX ("offset min-sum"), in the UNITS OF THE LLRS, as for the layered calls above.  The TM codes'
 *           punctured variables start at 0, and every message into them is a minimum over their neighbours' first messages: an
 *           offset above those (0.3 for LLRs of the form +-1 + noise at 1.7 dB on TM2048) zeroes them for good and no frame decodes.
 * One pair per call.  A NaN, an infinity or a value outside these ranges returns LABRADOR_LDPC_HIP_EINVAL (the message names the
 * parameter), decided with the other argument checks before any device work -- and before the batch is looked at, so an empty batch
 * with a bad pair is refused too.  With scale = 1 and offset = 0 the step is the identity and the results equal those of
 * labrador_ldpc_decode_ms_batch_f32 / labrador_ldpc_decode_ms_soft_batch_f32 bit for bit, app included.  The library chooses no
 * default: DESIGN.md 4.13 gives measured starting points ((0.8125, 0) and (1, 0.1) on TM2048).
 * One kernel per code -- the code's default f32 flooding kernel with the step -- so `variant` 0 is the only one: any other value
 * returns LABRADOR_LDPC_HIP_EUNSUPPORTED with the argument checks, before any device work.  The input is always copied in (host
 * buffers are never read across the link).  Arguments, memory modes, device sets, `stream` and alignment rules as
 * labrador_ldpc_decode_ms_batch_f32 / labrador_ldpc_decode_ms_soft_batch_f32 (a device `app` 16-byte aligned, a NULL `app` is
 * EINVAL).  There is no _multi, single-frame, integer, f64, f16 or bf16 form.  Returns a status code. */
int labrador_ldpc_decode_ms_corrected_batch_f32(enum labrador_ldpc_code code, const float *llrs, uint8_t *output, uint32_t *iters,
                                                uint8_t *success, size_t batch, size_t max_iters, float scale, float offset,
                                                const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_corrected_soft_batch_f32(enum labrador_ldpc_code code, const float *llrs, float *app, uint8_t *output,
                                                     uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                                     float scale, float offset, const struct labrador_ldpc_hip_opts *opts);

/* The f32 cascade with a corrected stage 1: labrador_ldpc_decode_ms_cascade_batch_f32 whose stage 1 is
 * labrador_ldpc_decode_ms_corrected_batch_f32 at (flooding_scale, flooding_offset); stage 2 -- the layered decoder at (scale, offset)
 * on the original LLRs of the frames stage 1 failed -- `stage`, `iters` and everything else are that call's.  Both pairs are
 * range-checked before the batch is looked at (a bad one is EINVAL even with an empty batch).  With flooding_scale = 1 and
 * flooding_offset = 0 the call IS labrador_ldpc_decode_ms_cascade_batch_f32, opts->variant included; with any other stage-1 pair
 * `variant` 0 is the only stage-1 kernel and any other value returns LABRADOR_LDPC_HIP_EUNSUPPORTED before any device work.
 * Returns a status code. */
int labrador_ldpc_decode_ms_cascade_corrected_batch_f32(enum labrador_ldpc_code code, const float *llrs, uint8_t *output,
                                                        uint32_t *iters, uint8_t *success, uint8_t *stage, size_t batch,
                                                        size_t max_iters, size_t max_sweeps, float flooding_scale,
                                                        float flooding_offset, float scale, float offset,
                                                        const struct labrador_ldpc_hip_opts *opts);

/* Normalized / offset min-sum on the FLOODING schedule for i8 LLRs, in integers: the flooding decoder of
 * labrador_ldpc_decode_ms_batch_i8 -- the reference's decode_ms::<i8>, iteration for iteration, with its saturating i8 arithmetic and
 * |-128| = 127 -- with one step added.  Where an iteration forms an edge's check message, its magnitude m (min2 of the check if |v|
 * of the edge equals min1, else min1: the previous iteration's minima, 0 <= m <= 127; zero in iteration 0) becomes
 *     t  = (scale_num * m + ((1 << scale_shift) >> 1)) >> scale_shift     exact; round half up; scale_shift = 0 adds nothing
 *     m' = max(t - offset, 0)
 * and the signs are applied to m' as they are to m.  Which of min1 / min2 an edge takes is decided on the uncorrected values;
 * everything else (self-correction, accumulation order, the stop rule, iters, success, output, max_iters = 0) is the flooding
 * contract unchanged.  The triple and its ranges are those of labrador_ldpc_decode_ms_layered_fixed_corrected_batch_i8:
 *   scale_shift  0 .. 8;   scale_num  1 .. 1 << scale_shift (the scale scale_num / 2^scale_shift in (0, 1]);
 *   offset       0 .. 127, in the UNITS OF THE QUANTISED LLRS.  The TM codes' punctured variables start at 0, and every message into
 *                them is a minimum over their neighbours' first messages: an offset above those zeroes them for good and no frame
 *                decodes.  The library chooses no default: DESIGN.md 4.14 gives measured starting points.
 * A value outside these ranges returns LABRADOR_LDPC_HIP_EINVAL (the message names the parameter).  With scale_num = 1 << scale_shift
 * and offset = 0 the step is the identity and the results equal those of labrador_ldpc_decode_ms_batch_i8 bit for bit.
 * A kernel is built per multiplier width: a scale of 1 (the offset alone), a scale with at most four fractional bits (13/16, 3/4,
 * 7/8 ...), and any other scale.  The first two were measured (the offset alone costs 2 - 4 % of the plain kernel's
 * rate, a four-bit scale 6 - 26 %); a scale with MORE than four fractional bits selects the widest kernel, whose rate has not been
 * measured -- it executes about twice the four-bit form's additional instructions.
 * The kernels are the BIT-SLICED kernels of the six TM codes with the step, at every batch size (no crossover to another kernel
 * family, the identity triple included): a TC code, and any `variant` but 0, return LABRADOR_LDPC_HIP_EUNSUPPORTED.  Order of the
 * checks: code, empty batch (OK), NULL buffers, the triple, variant and code family -- all before any device work.  With
 * LABRADOR_LDPC_HIP_MEM_DEVICE `llrs` must be 4-byte aligned (EINVAL) and `output` 8-byte aligned; the input is always copied in.
 * Arguments, memory modes, device sets and `stream` as labrador_ldpc_decode_ms_batch_i8.  Hard output only; there is no _multi,
 * single-frame, i16 or i32 form.  Returns a status code. */
int labrador_ldpc_decode_ms_corrected_batch_i8(enum labrador_ldpc_code code, const int8_t *llrs, uint8_t *output, uint32_t *iters,
                                               uint8_t *success, size_t batch, size_t max_iters, uint32_t scale_num,
                                               uint32_t scale_shift, uint32_t offset, const struct labrador_ldpc_hip_opts *opts);

/* The i8 cascades with a corrected stage 1: labrador_ldpc_decode_ms_cascade_batch_i8 /
 * labrador_ldpc_decode_ms_cascade_quantised_batch_i8 whose stage 1 is labrador_ldpc_decode_ms_corrected_batch_i8 at
 * (flooding_scale_num, flooding_scale_shift, flooding_offset); stage 2 -- the fixed-point layered decoder at (scale_num,
 * scale_shift, offset) on the original (quantised) LLRs of the frames stage 1 failed -- `stage`, `iters` and everything else are
 * those calls'.  Both triples are range-checked where those calls check theirs, the stage-1 triple first.  With an identity stage-1
 * triple (flooding_scale_num = 1 << flooding_scale_shift, flooding_offset = 0) the call IS the plain cascade: any code,
 * opts->variant included.  With any other stage-1 triple stage 1 is the bit-sliced kernel with the step: a TC code, and any
 * `variant` but 0, return LABRADOR_LDPC_HIP_EUNSUPPORTED before any device work, and with LABRADOR_LDPC_HIP_MEM_DEVICE the i8 `llrs`
 * of the first call must be 4-byte aligned.  Returns a status code. */
int labrador_ldpc_decode_ms_cascade_corrected_batch_i8(enum labrador_ldpc_code code, const int8_t *llrs, uint8_t *output, uint32_t *iters,
                                                       uint8_t *success, uint8_t *stage, size_t batch, size_t max_iters,
                                                       size_t max_sweeps, uint32_t flooding_scale_num, uint32_t flooding_scale_shift,
                                                       uint32_t flooding_offset, uint32_t scale_num, uint32_t scale_shift,
                                                       uint32_t offset, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_cascade_quantised_corrected_batch_i8(enum labrador_ldpc_code code, const float *llrs, uint8_t *output,
                                                                 uint32_t *iters, uint8_t *success, uint8_t *stage, size_t batch,
                                                                 size_t max_iters, size_t max_sweeps, float scale, int lim,
                                                                 uint32_t flooding_scale_num, uint32_t flooding_scale_shift,
                                                                 uint32_t flooding_offset, uint32_t scale_num, uint32_t scale_shift,
                                                                 uint32_t offset, const struct labrador_ldpc_hip_opts *opts);

/* The cascade with SOFT OUTPUT: labrador_ldpc_decode_ms_cascade_batch_<T> that also returns every frame's
 * a-posteriori LLRs.  Per frame f, exactly, the two separate soft calls composed:
 *     (a1, o1, i1, s1) = labrador_ldpc_decode_ms_soft_batch_<T> on frame f at cap max_iters, kernel opts->variant
 *                        (f32 with a stage-1 pair other than (1, 0): labrador_ldpc_decode_ms_corrected_soft_batch_f32 at
 *                        (flooding_scale, flooding_offset))
 *     if s1:  app, output, iters, success, stage = a1, o1, i1, 1, 0
 *     else:   (a2, o2, i2, s2) = f32:      labrador_ldpc_decode_ms_layered_corrected_soft_batch_f32 at (scale, offset)
 *                                i8 / i16: labrador_ldpc_decode_ms_layered_fixed_corrected_soft_batch_<T> at (scale_num, scale_shift, offset)
 *                                on the ORIGINAL LLRs of frame f at cap max_sweeps, variant 0
 *             app, output, iters, success, stage = a2, o2, i2, s2, 1
 * output, iters, success and stage equal, bit for bit, what the hard cascade entry of the same type and arguments returns (for f32,
 * labrador_ldpc_decode_ms_cascade_corrected_batch_f32: the one soft entry carries both pairs, and at the identity stage-1 pair it is
 * the plain cascade made soft).
 *   app  [batch][n + p]   punctured variables last, as for the other soft entries.
 *        f32: float.  The +-0 and NaN rules are those of the stage the frame carries (labrador_ldpc_decode_ms_soft_batch_f32,
 *             labrador_ldpc_decode_ms_layered_soft_batch_f32).
 *        i8 / i16: int32_t, the marginal type of the fixed-point layered decoder.  A stage-0 frame holds the flooding decoder's
 *             SATURATING marginal of the LLR type, sign-extended (-128 .. 127, -32768 .. 32767); a stage-1 frame holds the layered
 *             decoder's EXACT int32 sum, which may lie far outside that range.  `stage` says which: two frames' marginals are
 *             comparable only within a stage.
 * max_iters = 0: stage 1 fails every frame with zero marginals, and every frame goes to stage 2 (stage all 1, app the layered
 * decoder's).  max_sweeps = 0: the frames stage 1 failed carry what the layered soft entry returns at cap 0.
 * The integer entries here take no stage-1 correction (labrador_ldpc_decode_ms_cascade_bitsliced_corrected_soft_batch_i8 below is the
 * i8 soft cascade that does).  Soft i8 on the TM codes runs the
 * f32-pipe i8 kernel here, as labrador_ldpc_decode_ms_soft_batch_i8 does: THE FIRST STAGE OF THE i8 SOFT CASCADE ON A TM CODE
 * THEREFORE RUNS AT THE f32-PIPE RATE in this entry, not at the bit-sliced rate of the hard cascade;
 * labrador_ldpc_decode_ms_cascade_bitsliced_soft_batch_i8 below is the same cascade with the bit-sliced soft kernel as its first stage
 * (DESIGN.md 4.16).  `variant` 64 (the bit-sliced kernels) returns LABRADOR_LDPC_HIP_EUNSUPPORTED here with the soft flooding entry's text.
 * Checks, in the hard cascade's order and with its texts: `code`; for f32 both pairs, before the batch is looked at; an empty batch
 * is OK and touches nothing; a NULL buffer, `app` and `stage` included, is EINVAL; for i8 / i16 the triple; f32 with a stage-1 pair
 * other than (1, 0) and `variant` != 0 is EUNSUPPORTED -- all before any device work.  With MEM_DEVICE `output` must be 8-byte and
 * `app` 16-byte aligned (EINVAL).  Synchronisation of opts->stream, host buffers, device sets and everything else as
 * labrador_ldpc_decode_ms_cascade_batch_*; LABRADOR_LDPC_HIP_CASCADE_CHUNK also bounds the chunks of frames in which the integer
 * entries run stage 1 (its marginals pass through a bounded workspace on their way to int32).  There is no quantised (f32-in), f16 /
 * bf16 or _multi form.  Returns a status code. */
int labrador_ldpc_decode_ms_cascade_soft_batch_f32(enum labrador_ldpc_code code, const float *llrs, float *app, uint8_t *output,
                                                   uint32_t *iters, uint8_t *success, uint8_t *stage, size_t batch, size_t max_iters,
                                                   size_t max_sweeps, float flooding_scale, float flooding_offset, float scale,
                                                   float offset, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_cascade_soft_batch_i8 (enum labrador_ldpc_code code, const int8_t *llrs, int32_t *app, uint8_t *output,
                                                   uint32_t *iters, uint8_t *success, uint8_t *stage, size_t batch, size_t max_iters,
                                                   size_t max_sweeps, uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                                                   const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_cascade_soft_batch_i16(enum labrador_ldpc_code code, const int16_t *llrs, int32_t *app, uint8_t *output,
                                                   uint32_t *iters, uint8_t *success, uint8_t *stage, size_t batch, size_t max_iters,
                                                   size_t max_sweeps, uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                                                   const struct labrador_ldpc_hip_opts *opts);

/* labrador_ldpc_decode_ms_cascade_soft_batch_i8 with labrador_ldpc_decode_ms_bitsliced_soft_batch_i8 as stage 1: all
 * five results equal that entry's bit for bit -- a stage-0 frame's int32 marginal is the sign-extended saturating one -- with the first
 * stage at the bit-sliced kernels' rate.  That entry's checks, and on top of them: TM1536, TM2048, TM6144 and TM8192 and `variant` 0
 * only (any other is LABRADOR_LDPC_HIP_EUNSUPPORTED before any device work; TM1280 and TM5120 with the text that the two-wave kernels
 * have no soft form), and with LABRADOR_LDPC_HIP_MEM_DEVICE `llrs` 4-byte aligned (EINVAL).  Chunking
 * (LABRADOR_LDPC_HIP_CASCADE_CHUNK) and synchronisation as that entry.  The form with a stage-1 triple is
 * labrador_ldpc_decode_ms_cascade_bitsliced_corrected_soft_batch_i8 below, the one on f32 LLRs
 * labrador_ldpc_decode_ms_cascade_bitsliced_quantised_soft_batch_i8.  There is no _multi form.  Returns a status code. */
int labrador_ldpc_decode_ms_cascade_bitsliced_soft_batch_i8(enum labrador_ldpc_code code, const int8_t *llrs, int32_t *app,
                                                            uint8_t *output, uint32_t *iters, uint8_t *success, uint8_t *stage,
                                                            size_t batch, size_t max_iters, size_t max_sweeps, uint32_t scale_num,
                                                            uint32_t scale_shift, uint32_t offset,
                                                            const struct labrador_ldpc_hip_opts *opts);

/* The entry above with a STAGE-1 TRIPLE: labrador_ldpc_decode_ms_bitsliced_corrected_soft_batch_i8 at
 * (flooding_scale_num, flooding_scale_shift, flooding_offset) and cap max_iters as stage 1, then, on the original LLRs of the frames
 * it failed, labrador_ldpc_decode_ms_layered_fixed_corrected_soft_batch_i8 at (scale_num, scale_shift, offset) and cap max_sweeps --
 * per frame exactly the composition of those two calls.  `output`, `iters`, `success` and `stage` equal, bit for bit, what
 * labrador_ldpc_decode_ms_cascade_corrected_batch_i8 returns for the same arguments; `app` is int32 as for the other integer soft
 * cascades: a stage-0 row is the corrected flooding decoder's saturating int8 marginal sign-extended, a stage-1 row the layered
 * decoder's exact sum.  An identity stage-1 triple runs the plain bit-sliced soft kernel, i.e. the entry above.
 * Checks: both triples where labrador_ldpc_decode_ms_cascade_corrected_batch_i8 checks them, stage 1's first (EINVAL); then TM1536,
 * TM2048, TM6144 and TM8192 and `variant` 0 only, with the texts of the entry above (EUNSUPPORTED) -- all before any device work; with
 * LABRADOR_LDPC_HIP_MEM_DEVICE `llrs` 4-byte, `output` 8-byte and `app` 16-byte aligned (EINVAL).  Chunking
 * (LABRADOR_LDPC_HIP_CASCADE_CHUNK) and synchronisation as the entry above.  On f32 LLRs:
 * labrador_ldpc_decode_ms_cascade_bitsliced_quantised_soft_batch_i8.  There is no _multi form.  Returns a status code. */
int labrador_ldpc_decode_ms_cascade_bitsliced_corrected_soft_batch_i8(enum labrador_ldpc_code code, const int8_t *llrs, int32_t *app,
                                                                      uint8_t *output, uint32_t *iters, uint8_t *success, uint8_t *stage,
                                                                      size_t batch, size_t max_iters, size_t max_sweeps,
                                                                      uint32_t flooding_scale_num, uint32_t flooding_scale_shift,
                                                                      uint32_t flooding_offset, uint32_t scale_num, uint32_t scale_shift,
                                                                      uint32_t offset, const struct labrador_ldpc_hip_opts *opts);

/* Device-resident batches on SEVERAL GPUs with one call (the reference's analogue: one job over all workers,
 * perftest/src/main.rs:39-52; capi/src/lib.rs:83-95 for the buffers' meaning).  Part i is frames[i] frames whose four buffers --
 * llrs[i], output[i] (8-byte aligned), iters[i], success[i], laid out as in labrador_ldpc_decode_ms_batch_* -- are DEVICE memory
 * resident on HIP device devices[i]; an ordinal may repeat (several parts on one GPU: up to four run concurrently, more queue
 * behind them) and frames[i] may be 0.  Every part is
 * enqueued by the library's persistent worker thread of its device (pinned to the GPU's NUMA node) on a stream of the library's own
 * and the call returns when ALL parts are decoded; work the caller enqueued on its own streams for these buffers must be complete
 * before the call.  No data crosses between devices and there is no collective.  Returns the first failing part's status
 * (labrador_ldpc_hip_last_error() names the part and its device). */
int labrador_ldpc_decode_ms_batch_f32_multi(enum labrador_ldpc_code code, size_t n_parts, const int *devices, const float *const *llrs,
                                            uint8_t *const *output, uint32_t *const *iters, uint8_t *const *success,
                                            const size_t *frames, size_t max_iters, int variant);
int labrador_ldpc_decode_ms_batch_i8_multi (enum labrador_ldpc_code code, size_t n_parts, const int *devices, const int8_t *const *llrs,
                                            uint8_t *const *output, uint32_t *const *iters, uint8_t *const *success,
                                            const size_t *frames, size_t max_iters, int variant);
int labrador_ldpc_decode_ms_batch_i16_multi(enum labrador_ldpc_code code, size_t n_parts, const int *devices, const int16_t *const *llrs,
                                            uint8_t *const *output, uint32_t *const *iters, uint8_t *const *success,
                                            const size_t *frames, size_t max_iters, int variant);
int labrador_ldpc_decode_ms_batch_i32_multi(enum labrador_ldpc_code code, size_t n_parts, const int *devices, const int32_t *const *llrs,
                                            uint8_t *const *output, uint32_t *const *iters, uint8_t *const *success,
                                            const size_t *frames, size_t max_iters, int variant);
int labrador_ldpc_decode_ms_batch_f64_multi(enum labrador_ldpc_code code, size_t n_parts, const int *devices, const double *const *llrs,
                                            uint8_t *const *output, uint32_t *const *iters, uint8_t *const *success,
                                            const size_t *frames, size_t max_iters, int variant);

/* Batched bit-flipping decoder (src/decoder.rs:243-301), the batched form of
 * labrador_ldpc_decode_bf:  input [batch][n/8], output [batch][output_len], iters [batch]
 * (bit-flipping iterations + erasure iterations, or that sum's maximum on failure), success [batch]. */
int labrador_ldpc_decode_bf_batch(enum labrador_ldpc_code code, const uint8_t *input, uint8_t *output,
                                  uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                  const struct labrador_ldpc_hip_opts *opts);

/* Batched systematic encoder on the GPU: codewords[f] = copy_encode(data[f]) for every frame
 * (src/encoder.rs:293-315; the per-frame C entry is labrador_ldpc_copy_encode above).
 *   data      [batch][k/8]   MSB-first bytes
 *   codewords [batch][n/8]   first k/8 bytes = data, rest = parity
 * Host or device buffers per opts->memory (device buffers 4-byte aligned); asynchronous with
 * MEM_DEVICE.  Returns a status code. */
int labrador_ldpc_encode_batch(enum labrador_ldpc_code code, const uint8_t *data, uint8_t *codewords,
                               size_t batch, const struct labrador_ldpc_hip_opts *opts);

/* Batched LLR helpers: the data formats either side of decode_ms for whole batches -- hard_to_llrs
 * (src/decoder.rs:484-493; per-frame C entries capi/src/lib.rs:129-153) and llrs_to_hard (src/decoder.rs:498-509;
 * capi/src/lib.rs:155-179), frame after frame:
 *   input / output  [batch][n/8]  packed bits, MSB first
 *   llrs            [batch][n]    -1 for a set bit, +1 for a clear one; a bit is set where the LLR is < 0
 * With opts->memory == MEM_DEVICE the conversion is a streaming kernel on opts->stream (asynchronous; llrs
 * 16-byte aligned), so that hard decisions produced on the device (encode_batch, decode_bf_batch,
 * a decode_ms_batch output) feed decode_ms_batch without leaving HBM.  With host buffers (opts NULL or MEM_HOST) the
 * frames are converted in place by the library's host code -- the data is there and the loop is cheaper than the PCIe
 * crossing; opts->device / devices are ignored.  Returns a status code. */
int labrador_ldpc_hard_to_llrs_batch_i8 (enum labrador_ldpc_code code, const uint8_t *input, int8_t  *llrs, size_t batch, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_hard_to_llrs_batch_i16(enum labrador_ldpc_code code, const uint8_t *input, int16_t *llrs, size_t batch, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_hard_to_llrs_batch_i32(enum labrador_ldpc_code code, const uint8_t *input, int32_t *llrs, size_t batch, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_hard_to_llrs_batch_f32(enum labrador_ldpc_code code, const uint8_t *input, float   *llrs, size_t batch, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_hard_to_llrs_batch_f64(enum labrador_ldpc_code code, const uint8_t *input, double  *llrs, size_t batch, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_llrs_to_hard_batch_i8 (enum labrador_ldpc_code code, const int8_t  *llrs, uint8_t *output, size_t batch, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_llrs_to_hard_batch_i16(enum labrador_ldpc_code code, const int16_t *llrs, uint8_t *output, size_t batch, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_llrs_to_hard_batch_i32(enum labrador_ldpc_code code, const int32_t *llrs, uint8_t *output, size_t batch, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_llrs_to_hard_batch_f32(enum labrador_ldpc_code code, const float   *llrs, uint8_t *output, size_t batch, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_llrs_to_hard_batch_f64(enum labrador_ldpc_code code, const double  *llrs, uint8_t *output, size_t batch, const struct labrador_ldpc_hip_opts *opts);

/* Quantised LLRs from f32 soft values: how a receiver that holds float LLRs reaches the integer decoders -- the
 * flooding i8 / i16 kernels, the fixed-point layered entries and the integer cascade.  For an f32 LLR x, `scale` (finite, > 0) and
 * `lim` (0 <= lim <= 127 for i8, <= 32767 for i16), the library's one rule (the channel's, labrador_ldpc_hip_awgn_i8):
 *     p = scale * x                     one f32 multiply, nothing fused into it
 *     q = 0                             if p is NaN: an erasure
 *       = clamp(rint(p), -lim, lim)     otherwise; rint to nearest, ties to even
 * +-inf and products beyond the integer range clamp to +-lim; -0.0 gives 0.
 *   llrs [batch][n]  f32      q [batch][n]  int8_t / int16_t
 * With host buffers (opts NULL or MEM_HOST) the frames are quantised where they lie by the library's host code, which follows the
 * rule exactly (the data is there and the loop is cheaper than the crossing); opts->device / devices are ignored.  With MEM_DEVICE
 * it is a streaming kernel on opts->stream, asynchronous; `llrs` and `q` must be 16-byte aligned (EINVAL, checked before the device
 * is selected).  Arguments are checked in this order, all before any device work: `code`; `scale` and `lim`; an empty batch is OK
 * whatever the pointers; a NULL buffer; opts->memory.  Returns a status code. */
int labrador_ldpc_quantise_llrs_batch_i8 (enum labrador_ldpc_code code, const float *llrs, int8_t  *q, size_t batch, float scale, int lim,
                                          const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_quantise_llrs_batch_i16(enum labrador_ldpc_code code, const float *llrs, int16_t *q, size_t batch, float scale, int lim,
                                          const struct labrador_ldpc_hip_opts *opts);

/* The call a receiver makes: decode f32 LLRs through the integer flooding kernels.  Per frame f, exactly,
 *     labrador_ldpc_decode_ms_batch_<T> on (labrador_ldpc_quantise_llrs_batch_<T> of frame f at (scale, lim))
 * at cap max_iters and kernel opts->variant (LABRADOR_LDPC_HIP_VARIANT_BITSLICE included, for i8): output, iters and success are
 * that entry's, bit for bit.  Host f32 rows cross the link as they are and are quantised on the device; with device sets the frames
 * are sharded as for every batched entry.  The quantised rows live in a workspace of the library's (per calling thread and device,
 * grow-only), filled and decoded in chunks of what fits 256 MiB of quantised LLRs, at least 8192 frames
 * (LABRADOR_LDPC_HIP_QUANT_CHUNK=<frames> lowers that, for tests).  Arguments are checked in this order, all before any device
 * work: `code`; `scale` and `lim`; an empty batch is OK whatever the pointers; a NULL buffer.  With MEM_DEVICE `output` must be
 * 8-byte and `llrs` 16-byte aligned, and the call is asynchronous on opts->stream; calls of one thread on different streams are
 * ordered on the workspace by the library.  It must not be called on a stream that is being captured into a graph.  A variant the
 * integer type has no kernel for is EUNSUPPORTED, as in labrador_ldpc_decode_ms_batch_*.  Hard output only; the layered entries and
 * the cascade have f32-input forms of their own below (labrador_ldpc_decode_ms_layered_quantised_*, _cascade_quantised_*).  Returns a
 * status code. */
int labrador_ldpc_decode_ms_quantised_batch_i8 (enum labrador_ldpc_code code, const float *llrs, uint8_t *output, uint32_t *iters,
                                                uint8_t *success, size_t batch, size_t max_iters, float scale, int lim,
                                                const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_quantised_batch_i16(enum labrador_ldpc_code code, const float *llrs, uint8_t *output, uint32_t *iters,
                                                uint8_t *success, size_t batch, size_t max_iters, float scale, int lim,
                                                const struct labrador_ldpc_hip_opts *opts);

/* f32 LLRs through the fixed-point layered decoders.  Per frame f, exactly,
 *     labrador_ldpc_decode_ms_layered_fixed_corrected_{,soft_}batch_<T> at (scale_num, scale_shift, offset), variant 0,
 *     on (labrador_ldpc_quantise_llrs_batch_<T> of frame f at (scale, lim))
 * at cap max_iters: output, iters, success and `app` (int32 [batch][n + p], the soft forms) are that entry's, bit for bit, for every
 * f32 input -- +-0, +-inf, NaN (an erasure), denormals and ties included.  The quantiser sits in the kernel's loader, which reads
 * every LLR once as it fills the marginals: there is no quantised copy of the batch, no workspace and no synchronisation, so with
 * MEM_DEVICE the call is asynchronous on opts->stream like the fixed-point entries themselves.  An identity triple (1 << k, k, 0)
 * runs the plain kernel form, whose results are the same.  Host f32 rows cross the link as they are; device sets shard the frames as
 * for every batched entry.
 * Arguments are checked in this order, all before any device work: `code`; `scale` and `lim`; an empty batch is OK whatever the
 * pointers; a NULL buffer (`app` included, where the entry has it); the ranges of the triple; opts->variant != 0 is EUNSUPPORTED.
 * With MEM_DEVICE `output` must be 8-byte and `app` 16-byte aligned; `llrs` need only be aligned to a float (the kernel loads
 * single elements).  Returns a status code. */
int labrador_ldpc_decode_ms_layered_quantised_batch_i8 (enum labrador_ldpc_code code, const float *llrs, uint8_t *output, uint32_t *iters,
                                                        uint8_t *success, size_t batch, size_t max_iters, float scale, int lim,
                                                        uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                                                        const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_quantised_batch_i16(enum labrador_ldpc_code code, const float *llrs, uint8_t *output, uint32_t *iters,
                                                        uint8_t *success, size_t batch, size_t max_iters, float scale, int lim,
                                                        uint32_t scale_num, uint32_t scale_shift, uint32_t offset,
                                                        const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_quantised_soft_batch_i8 (enum labrador_ldpc_code code, const float *llrs, int32_t *app, uint8_t *output,
                                                             uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                                             float scale, int lim, uint32_t scale_num, uint32_t scale_shift,
                                                             uint32_t offset, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_quantised_soft_batch_i16(enum labrador_ldpc_code code, const float *llrs, int32_t *app, uint8_t *output,
                                                             uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                                             float scale, int lim, uint32_t scale_num, uint32_t scale_shift,
                                                             uint32_t offset, const struct labrador_ldpc_hip_opts *opts);

/* f32 LLRs through the integer cascade: the call a receiver wants -- f32 in, the fast integer flooding kernels on
 * every frame, the fixed-point layered decoder on the frames they fail.  Per frame f, exactly,
 *     labrador_ldpc_decode_ms_cascade_batch_<T> at (max_iters, max_sweeps, scale_num, scale_shift, offset), stage 1 at opts->variant
 *     (LABRADOR_LDPC_HIP_VARIANT_BITSLICE included, for i8), on (labrador_ldpc_quantise_llrs_batch_<T> of frame f at (scale, lim))
 * with output, iters, success and stage as that entry's, bit for bit.  The f32 rows are quantised in chunks into the workspace of
 * labrador_ldpc_decode_ms_quantised_batch_* (LABRADOR_LDPC_HIP_QUANT_CHUNK), every chunk runs the cascade on its quantised rows, and
 * stage 2 gathers the failed frames from those (1 or 2 bytes per LLR, not 4) through the cascade's own workspace
 * (LABRADOR_LDPC_HIP_CASCADE_CHUNK); calls of one thread on different streams are ordered on both workspaces by the library.
 * Arguments are checked in this order, all before any device work: `code`; `scale` and `lim`; an empty batch is OK whatever the
 * pointers; a NULL buffer, `stage` included; the ranges of the triple.  With MEM_DEVICE `output` must be 8-byte and `llrs` 16-byte
 * aligned (the streaming quantiser reads 16-byte pieces).  With MEM_DEVICE the call is NOT purely asynchronous: it SYNCHRONISES
 * opts->stream ONCE PER CHUNK, for the number of frames stage 1 failed, and returns with the last chunk's stage 2 enqueued, so the
 * results are valid once the stream is synchronised.  It MUST NOT be called on a stream that is being captured into a graph.
 * Hard output only.  Returns a status code. */
int labrador_ldpc_decode_ms_cascade_quantised_batch_i8 (enum labrador_ldpc_code code, const float *llrs, uint8_t *output, uint32_t *iters,
                                                        uint8_t *success, uint8_t *stage, size_t batch, size_t max_iters,
                                                        size_t max_sweeps, float scale, int lim, uint32_t scale_num,
                                                        uint32_t scale_shift, uint32_t offset, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_cascade_quantised_batch_i16(enum labrador_ldpc_code code, const float *llrs, uint8_t *output, uint32_t *iters,
                                                        uint8_t *success, uint8_t *stage, size_t batch, size_t max_iters,
                                                        size_t max_sweeps, float scale, int lim, uint32_t scale_num,
                                                        uint32_t scale_shift, uint32_t offset, const struct labrador_ldpc_hip_opts *opts);

/* f32 LLRs through the bit-sliced i8 flooding kernels' OWN LOADER: the quantiser sits where the kernel reads its
 * LLRs, so there is no quantised copy of the batch, no workspace and no chunk loop -- one launch per slice, and with MEM_DEVICE the
 * first two calls are asynchronous on opts->stream with nothing to wait for.  Per frame f, exactly,
 *     _bitsliced_quantised_batch_i8             labrador_ldpc_decode_ms_batch_i8
 *     _bitsliced_quantised_corrected_batch_i8   labrador_ldpc_decode_ms_corrected_batch_i8 at (scale_num, scale_shift, offset)
 *     _cascade_bitsliced_quantised_batch_i8     labrador_ldpc_decode_ms_cascade_quantised_corrected_batch_i8 at the same arguments
 * on (labrador_ldpc_quantise_llrs_batch_i8 of frame f at (scale, lim)) at cap max_iters: output, iters, success -- and `stage` -- are
 * that entry's, bit for bit, for every f32 input, +-0, +-inf, NaN (an erasure), denormals and ties included.  An identity triple
 * (1 << k, k, 0) runs the plain kernel.  The cascade's stage 1 reads the caller's f32 rows, the failed frames' f32 rows are gathered
 * through the cascade's workspace (LABRADOR_LDPC_HIP_CASCADE_CHUNK) and stage 2 is the fixed-point layered decoder whose loader
 * quantises (labrador_ldpc_decode_ms_layered_quantised_batch_i8) at the stage-2 triple; like every cascade it SYNCHRONISES
 * opts->stream once per launch slice and must not be called on a stream that is being captured into a graph.
 * Lockstep kernels of the four one-wave codes TM1536, TM2048, TM6144 and TM8192 at every batch size, kernel variant 0 only.
 * Arguments are checked in this order, all before any device work: `code`; `scale` and `lim`; an empty batch is OK whatever the
 * pointers; a NULL buffer (`stage` included, where the entry has it); opts->variant != 0, a TC code, TM1280 or TM5120 is
 * EUNSUPPORTED; the ranges of the triples, stage 1's first.  With MEM_DEVICE `output` must be 8-byte and `llrs` 16-byte aligned.
 * Host f32 rows go through the one batched call path and cross the link as f32; device sets shard the frames as for every batched
 * entry.  Hard output only (the soft forms follow).  The older quantised entries keep their two-pass route.  Returns a status code. */
int labrador_ldpc_decode_ms_bitsliced_quantised_batch_i8(enum labrador_ldpc_code code, const float *llrs, uint8_t *output, uint32_t *iters,
                                                         uint8_t *success, size_t batch, size_t max_iters, float scale, int lim,
                                                         const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_bitsliced_quantised_corrected_batch_i8(enum labrador_ldpc_code code, const float *llrs, uint8_t *output,
                                                                   uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                                                   float scale, int lim, uint32_t scale_num, uint32_t scale_shift,
                                                                   uint32_t offset, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_cascade_bitsliced_quantised_batch_i8(enum labrador_ldpc_code code, const float *llrs, uint8_t *output,
                                                                 uint32_t *iters, uint8_t *success, uint8_t *stage, size_t batch,
                                                                 size_t max_iters, size_t max_sweeps, float scale, int lim,
                                                                 uint32_t flooding_scale_num, uint32_t flooding_scale_shift,
                                                                 uint32_t flooding_offset, uint32_t scale_num, uint32_t scale_shift,
                                                                 uint32_t offset, const struct labrador_ldpc_hip_opts *opts);

/* ... WITH SOFT OUTPUT: the three entries above returning every frame's a-posteriori LLRs as well -- what an iterative
 * demapper or equaliser that holds f32 LLRs calls.  The soft bit-sliced kernels with the quantiser in their loader: no quantised copy
 * of the batch, no workspace and no chunk loop in the first two, one launch per slice, asynchronous on opts->stream with MEM_DEVICE.
 * Per frame f, exactly, in `app`, `output`, `iters`, `success` (and `stage`),
 *     _bitsliced_quantised_soft_batch_i8             labrador_ldpc_decode_ms_bitsliced_soft_batch_i8
 *     _bitsliced_quantised_corrected_soft_batch_i8   labrador_ldpc_decode_ms_bitsliced_corrected_soft_batch_i8 at (scale_num, scale_shift,
 *                                                    offset)
 *     _cascade_bitsliced_quantised_soft_batch_i8     labrador_ldpc_decode_ms_cascade_bitsliced_corrected_soft_batch_i8 at the two triples
 *                                                    (an identity stage-1 triple: labrador_ldpc_decode_ms_cascade_bitsliced_soft_batch_i8)
 * on (labrador_ldpc_quantise_llrs_batch_i8 of frame f at (scale, lim)), bit for bit, for every f32 input, +-0, +-inf, NaN (an erasure),
 * denormals and ties included; the hard results are therefore also those of the three entries above.
 *   app  flooding: [batch][n + p] int8, the decoder's saturating marginal va, reaching -128; all zero for max_iters = 0; punctured
 *        variables last.  A converged frame carries va of its converging iteration, any other frame va of the last iteration.
 *        cascade: [batch][n + p] int32 -- a stage-0 frame carries the flooding marginal sign-extended, a stage-1 frame the layered
 *        decoder's exact sum (labrador_ldpc_decode_ms_cascade_soft_batch_i8 has the rest); comparable only within a stage.
 * An identity triple (1 << k, k, 0) runs the plain kernel.  The cascade's stage 1 reads the caller's f32 rows and writes int8 marginals
 * into the cascade's workspace, widened from there into `app`; the failed frames' f32 rows are gathered
 * (LABRADOR_LDPC_HIP_CASCADE_CHUNK) and stage 2 is labrador_ldpc_decode_ms_layered_quantised_soft_batch_i8's kernel at the stage-2
 * triple; like every cascade it SYNCHRONISES opts->stream once per launch slice and must not be called on a stream that is being
 * captured into a graph.
 * Lockstep kernels of the four one-wave codes TM1536, TM2048, TM6144 and TM8192 at every batch size, kernel variant 0 only.
 * Arguments are checked in this order, all before any device work: `code`; `scale` and `lim`; an empty batch is OK whatever the
 * pointers; a NULL buffer (`app` included, and `stage` where the entry has it); opts->variant != 0, a TC code, TM1280 or TM5120 is
 * EUNSUPPORTED with a text that names the four codes; the ranges of the triples, stage 1's first.  With MEM_DEVICE `output` must be
 * 8-byte and `llrs` and `app` 16-byte aligned (EINVAL).  Host f32 rows go through the one batched call path and cross the link as f32,
 * `app` comes back as a further output; device sets shard the frames as for every batched entry.  There is no _multi, single-frame,
 * i16, slot-refill or two-wave form.  Returns a status code. */
int labrador_ldpc_decode_ms_bitsliced_quantised_soft_batch_i8(enum labrador_ldpc_code code, const float *llrs, int8_t *app, uint8_t *output,
                                                              uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters, float scale,
                                                              int lim, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_bitsliced_quantised_corrected_soft_batch_i8(enum labrador_ldpc_code code, const float *llrs, int8_t *app,
                                                                        uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                                                        size_t max_iters, float scale, int lim, uint32_t scale_num,
                                                                        uint32_t scale_shift, uint32_t offset,
                                                                        const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_cascade_bitsliced_quantised_soft_batch_i8(enum labrador_ldpc_code code, const float *llrs, int32_t *app,
                                                                      uint8_t *output, uint32_t *iters, uint8_t *success, uint8_t *stage,
                                                                      size_t batch, size_t max_iters, size_t max_sweeps, float scale, int lim,
                                                                      uint32_t flooding_scale_num, uint32_t flooding_scale_shift,
                                                                      uint32_t flooding_offset, uint32_t scale_num, uint32_t scale_shift,
                                                                      uint32_t offset, const struct labrador_ldpc_hip_opts *opts);

/* PACKED HARD DECISIONS through the bit-sliced i8 flooding kernels' OWN LOADER: what a hard-decision receiver calls
 * instead of labrador_ldpc_hard_to_llrs_batch_i8 into a buffer of n bytes per frame followed by labrador_ldpc_decode_ms_batch_i8.  A
 * packed frame already is the kernels' sign plane, so there is no expanded copy of the batch, no workspace and no chunk loop -- one
 * launch per slice, and with MEM_DEVICE the call is asynchronous on opts->stream with nothing to wait for and may be captured into a
 * graph.
 *   input     [batch][n / 8]  packed bits, MSB first, as labrador_ldpc_decode_bf_batch and labrador_ldpc_hard_to_llrs_batch_* take them
 *   erasures  NULL, or [batch][n / 8] in the same packing: a set bit marks a position the receiver knows to be bad
 *   magnitude 1 .. 127: the confidence every unerased position goes in with.  At 1 -- the reference's hard_to_llrs -- the integer
 *             correction is a no-op ((13 * 1 + 8) >> 4 == 1); at 127 the saturating sums clip at once.
 * Per frame f, exactly,
 *     _bitsliced_hard_batch_i8             labrador_ldpc_decode_ms_batch_i8
 *     _bitsliced_hard_corrected_batch_i8   labrador_ldpc_decode_ms_corrected_batch_i8 at (scale_num, scale_shift, offset)
 * on the i8 frame e, e[j] = 0 if bit j of `erasures` is set, else -magnitude if bit j of `input` is set, else +magnitude, at cap
 * max_iters: output, iters and success are that entry's, bit for bit.  With magnitude 1 and no mask e is
 * labrador_ldpc_hard_to_llrs_batch_i8's frame.  An identity triple (1 << k, k, 0) runs the plain kernel.
 * Lockstep kernels of the four one-wave codes TM1536, TM2048, TM6144 and TM8192 at every batch size, kernel variant 0 only.
 * Arguments are checked in this order, all before any device work: `code`; `magnitude` (EINVAL, with the value in the text); an empty
 * batch is OK whatever the pointers; a NULL `input`, `output`, `iters` or `success` (`erasures` may be NULL); opts->variant != 0, a TC
 * code, TM1280 or TM5120 is EUNSUPPORTED with a text that names the four codes; the ranges of the triple.  With MEM_DEVICE `output`
 * must be 8-byte and `input` and `erasures` 4-byte aligned (EINVAL): the loader reads one dword per lane.  Host rows go through the one
 * batched call path and cross the link packed, n / 8 bytes per frame and twice that with a mask; device sets shard the frames as for
 * every batched entry.  There is no _multi, single-frame, i16, soft-output, cascade, slot-refill or two-wave form.  Returns a status
 * code. */
int labrador_ldpc_decode_ms_bitsliced_hard_batch_i8(enum labrador_ldpc_code code, const uint8_t *input, const uint8_t *erasures,
                                                    uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                                    int magnitude, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_bitsliced_hard_corrected_batch_i8(enum labrador_ldpc_code code, const uint8_t *input, const uint8_t *erasures,
                                                              uint8_t *output, uint32_t *iters, uint8_t *success, size_t batch,
                                                              size_t max_iters, int magnitude, uint32_t scale_num, uint32_t scale_shift,
                                                              uint32_t offset, const struct labrador_ldpc_hip_opts *opts);

/* Half-precision LLRs to the f32 decoders: what a caller whose soft values exist only as IEEE binary16 (f16) or
 * bfloat16 (bf16) -- a learned demapper's tensors, frames kept in 2 bytes per LLR -- passes instead of an f32 copy.  Both formats
 * travel as their raw bits, `const uint16_t *`.  The library's one widening rule, widen(h), an f32:
 *     f16     the exact value: subnormals become the f32 normals they equal, +-0 stays +-0, +-inf stays +-inf; a NaN becomes the
 *             QUIET f32 NaN of the same sign (payload bits shifted left by 13, bit 22 set)
 *     bf16    (uint32_t)h << 16 reinterpreted as f32; nothing else, a signalling NaN stays what it is
 *   llrs [batch][n]  uint16_t      out [batch][n]  f32
 * With host buffers (opts NULL or MEM_HOST) the frames are widened where they lie by the library's host code, which follows the rule
 * exactly; opts->device / devices are ignored.  With MEM_DEVICE it is a streaming kernel on opts->stream, asynchronous; `llrs` and
 * `out` must be 16-byte aligned (EINVAL, checked before the device is selected).  Arguments are checked in this order, all before
 * any device work: `code`; an empty batch is OK whatever the pointers; a NULL buffer; opts->memory.  Returns a status code. */
int labrador_ldpc_widen_llrs_batch_f16 (enum labrador_ldpc_code code, const uint16_t *llrs, float *out, size_t batch,
                                        const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_widen_llrs_batch_bf16(enum labrador_ldpc_code code, const uint16_t *llrs, float *out, size_t batch,
                                        const struct labrador_ldpc_hip_opts *opts);

/* The flooding f32 decoders on half-precision rows.  Per frame f, exactly,
 *     labrador_ldpc_decode_ms_batch_f32 / labrador_ldpc_decode_ms_soft_batch_f32 on (widen of frame f)
 * at cap max_iters and kernel opts->variant: output, iters, success and `app` (f32 [batch][n + p], the soft forms) are that entry's,
 * bit for bit, for every input -- +-0, subnormals, +-inf and NaN included.  Host rows cross the link AS HALVES and are widened on the
 * device; with device sets the frames are sharded as for every batched entry.  The widened rows live in a workspace of the
 * library's (per calling thread and device, grow-only, the one of labrador_ldpc_decode_ms_quantised_batch_*), filled and decoded in
 * chunks of what fits 256 MiB of f32 LLRs, at least 8192 frames (LABRADOR_LDPC_HIP_WIDEN_CHUNK=<frames> lowers that, for tests).
 * Arguments are checked as by the f32 entry, in its order and with its texts, all before any device work: `code`; an empty batch is
 * OK whatever the pointers; a NULL buffer (`app` included, where the entry has it).  With MEM_DEVICE `output` must be 8-byte, `app`
 * 16-byte and `llrs` 16-byte aligned (the streaming pass reads 16-byte pieces), and the call is asynchronous on opts->stream; calls
 * of one thread on different streams are ordered on the workspace by the library.  It must not be called on a stream that is being
 * captured into a graph.  A variant the f32 decoder has no kernel for is EUNSUPPORTED, as in labrador_ldpc_decode_ms_batch_f32.
 * Returns a status code. */
int labrador_ldpc_decode_ms_batch_f16 (enum labrador_ldpc_code code, const uint16_t *llrs, uint8_t *output, uint32_t *iters, uint8_t *success,
                                       size_t batch, size_t max_iters, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_batch_bf16(enum labrador_ldpc_code code, const uint16_t *llrs, uint8_t *output, uint32_t *iters, uint8_t *success,
                                       size_t batch, size_t max_iters, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_soft_batch_f16 (enum labrador_ldpc_code code, const uint16_t *llrs, float *app, uint8_t *output, uint32_t *iters,
                                            uint8_t *success, size_t batch, size_t max_iters, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_soft_batch_bf16(enum labrador_ldpc_code code, const uint16_t *llrs, float *app, uint8_t *output, uint32_t *iters,
                                            uint8_t *success, size_t batch, size_t max_iters, const struct labrador_ldpc_hip_opts *opts);

/* The layered f32 decoders on half-precision rows.  Per frame f, exactly, the f32 entry of the same name on (widen of frame f):
 * output, iters, success and `app` (f32, the soft forms) are that entry's, bit for bit, with the same ranges of `scale` and
 * `offset`.  The widening sits in the kernel's loader, which reads every LLR as it fills its LDS copy: there is no widened copy of
 * the batch, no workspace and no synchronisation, so with MEM_DEVICE the call is asynchronous on opts->stream like the f32 entries
 * themselves.  The plain entries run the corrected kernel at (1, 0), whose results are the plain kernel's.  Host rows
 * cross the link as halves; device sets shard the frames as for every batched entry.
 * Arguments are checked in this order, all before any device work: `code`; for the corrected entries the ranges of `scale` and
 * `offset`; an empty batch is OK whatever the pointers; a NULL buffer (`app` included, where the entry has it); opts->variant != 0
 * is EUNSUPPORTED (with the f32 entries' text; those say it only after their device checks).  With MEM_DEVICE `output` must be 8-byte
 * and `app` 16-byte aligned; `llrs` need only be 2-byte aligned (the kernel loads single elements).  Returns a status code. */
int labrador_ldpc_decode_ms_layered_batch_f16 (enum labrador_ldpc_code code, const uint16_t *llrs, uint8_t *output, uint32_t *iters,
                                               uint8_t *success, size_t batch, size_t max_iters, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_batch_bf16(enum labrador_ldpc_code code, const uint16_t *llrs, uint8_t *output, uint32_t *iters,
                                               uint8_t *success, size_t batch, size_t max_iters, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_soft_batch_f16 (enum labrador_ldpc_code code, const uint16_t *llrs, float *app, uint8_t *output,
                                                    uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                                    const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_soft_batch_bf16(enum labrador_ldpc_code code, const uint16_t *llrs, float *app, uint8_t *output,
                                                    uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters,
                                                    const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_corrected_batch_f16 (enum labrador_ldpc_code code, const uint16_t *llrs, uint8_t *output, uint32_t *iters,
                                                         uint8_t *success, size_t batch, size_t max_iters, float scale, float offset,
                                                         const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_corrected_batch_bf16(enum labrador_ldpc_code code, const uint16_t *llrs, uint8_t *output, uint32_t *iters,
                                                         uint8_t *success, size_t batch, size_t max_iters, float scale, float offset,
                                                         const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_corrected_soft_batch_f16 (enum labrador_ldpc_code code, const uint16_t *llrs, float *app, uint8_t *output,
                                                              uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters, float scale,
                                                              float offset, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_layered_corrected_soft_batch_bf16(enum labrador_ldpc_code code, const uint16_t *llrs, float *app, uint8_t *output,
                                                              uint32_t *iters, uint8_t *success, size_t batch, size_t max_iters, float scale,
                                                              float offset, const struct labrador_ldpc_hip_opts *opts);

/* The f32 cascade on half-precision rows.  Per frame f, exactly,
 *     labrador_ldpc_decode_ms_cascade_batch_f32 at (max_iters, max_sweeps, scale, offset), stage 1 at opts->variant, on (widen of
 *     frame f)
 * with output, iters, success and stage as that entry's, bit for bit.  The rows are widened in chunks into the workspace of the
 * flooding entries above (LABRADOR_LDPC_HIP_WIDEN_CHUNK), every chunk runs the cascade on its f32 rows, and stage 2 gathers the
 * failed frames from those through the cascade's own workspace (LABRADOR_LDPC_HIP_CASCADE_CHUNK) into the f32 layered kernels; calls
 * of one thread on different streams are ordered on both workspaces by the library.  Arguments are checked in this order, all before
 * any device work: `code`; the ranges of `scale` and `offset`; an empty batch is OK whatever the pointers; a NULL buffer, `stage`
 * included.  With MEM_DEVICE `output` must be 8-byte and `llrs` 16-byte aligned.  With MEM_DEVICE the call is NOT purely
 * asynchronous: like the f32 cascade it SYNCHRONISES opts->stream for the number of frames stage 1 failed, here ONCE PER CHUNK, and
 * returns with the last chunk's stage 2 enqueued, so the results are valid once the stream is synchronised.  It MUST NOT be called
 * on a stream that is being captured into a graph.  Hard output only.  Returns a status code. */
int labrador_ldpc_decode_ms_cascade_batch_f16 (enum labrador_ldpc_code code, const uint16_t *llrs, uint8_t *output, uint32_t *iters,
                                               uint8_t *success, uint8_t *stage, size_t batch, size_t max_iters, size_t max_sweeps, float scale,
                                               float offset, const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_decode_ms_cascade_batch_bf16(enum labrador_ldpc_code code, const uint16_t *llrs, uint8_t *output, uint32_t *iters,
                                               uint8_t *success, uint8_t *stage, size_t batch, size_t max_iters, size_t max_sweeps, float scale,
                                               float offset, const struct labrador_ldpc_hip_opts *opts);

/* Synthetic AWGN frames on the device (harness side of the path; what perftest's ms_trial does
 * per frame at perftest/src/main.rs:10-18, batched): frame f takes codeword (f mod pool) of
 * `codewords` ([pool][n/8] bytes, MSB first), maps bit b to 1-2b, adds sigma*N(0,1) from a
 * counter-based generator keyed by (seed, f, sample), and writes
 *   f32: the sample itself;   i8: clamp(rint(scale*sample), -lim, lim), 0 <= lim <= 127 -- the f32 product rounded to the
 *        nearest integer, ties to even.
 * The generator is Philox4x32-10 (Salmon et al., SC'11).  Samples 4q .. 4q+3 of frame f come from the one block with the
 * counter (q, frame_lo, frame_hi, 0) = (q, f mod 2^32, f div 2^32, 0) and the key (seed_lo, seed_hi) = (seed mod 2^32,
 * seed div 2^32).  Its output words (x, y) make samples 4q and 4q+1, (z, w) make 4q+2 and 4q+3: from a pair (a, b),
 * u1 = ((a >> 8) + 1) / 2^24, u2 = (b >> 8) / 2^24, r = sqrt(-2 ln u1), and the two normals are r cos(2 pi u2) then
 * r sin(2 pi u2), evaluated in f32 (so |N| <= 5.77).  A host can regenerate any frame from (seed, f) alone;
 * tests/channel_reference.py does, and the tests hold the device to it sample by sample.
 * All pointers are DEVICE memory (opts->memory is ignored), llrs 16-byte aligned; asynchronous on opts->stream. */
int labrador_ldpc_hip_awgn_f32(enum labrador_ldpc_code code, const uint8_t *codewords, size_t pool,
                               float *llrs, size_t batch, float sigma, uint64_t seed,
                               const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_hip_awgn_i8 (enum labrador_ldpc_code code, const uint8_t *codewords, size_t pool,
                               int8_t *llrs, size_t batch, float sigma, float scale, int lim,
                               uint64_t seed, const struct labrador_ldpc_hip_opts *opts);
/* The same for frames [first_frame, first_frame + batch) of a larger job: frame f of the call is global frame
 * first_frame + f -- it takes codeword ((first_frame + f) mod pool) and the generator stream of that global index --
 * so the shards of a job generated on N devices are, byte for byte, the slices of the buffer one call with
 * first_frame = 0 writes (labrador_ldpc_hip_awgn_f32 / _i8 are these with first_frame = 0).  This is what makes an
 * N-GPU run of the harness decode the very frames of the one-GPU run (perftest/src/main.rs:39-52: one job, N workers). */
int labrador_ldpc_hip_awgn_f32_at(enum labrador_ldpc_code code, const uint8_t *codewords, size_t pool,
                                  float *llrs, uint64_t first_frame, size_t batch, float sigma, uint64_t seed,
                                  const struct labrador_ldpc_hip_opts *opts);
int labrador_ldpc_hip_awgn_i8_at (enum labrador_ldpc_code code, const uint8_t *codewords, size_t pool,
                                  int8_t *llrs, uint64_t first_frame, size_t batch, float sigma, float scale, int lim,
                                  uint64_t seed, const struct labrador_ldpc_hip_opts *opts);

/* Harness diagnostic: the shader clock (MHz) `device` (an ordinal or LABRADOR_LDPC_HIP_DEVICE_CURRENT) holds under a full-chip
 * VALU load lasting `busy_ms` milliseconds (0.01 .. 1000): the advance of the shader-clock counter against the 100 MHz
 * real-time counter, median over the workgroups.  Synchronous, default stream.  A multi-GPU harness prints it per worker
 * beside the worker's rate (perftest/src/main.rs:39-52 aggregates workers it assumes equal; GPUs of one node are not).
 * Returns a status code. */
int labrador_ldpc_hip_shader_clock_mhz(int device, double busy_ms, double *mhz);

/* Edge stream CRC of this library's own code tables, computed like the reference's
 * test_iter_parity (src/codes/mod.rs:508-533).  Lets a test pin the tables the kernels are
 * generated from against the reference's nine known answers without a GPU. */
uint32_t labrador_ldpc_hip_edge_crc(enum labrador_ldpc_code code);

/* The parity-check edges (check, variable) of this library's code tables in the order of the reference's
 * LDPCCode::iter_paritychecks() (src/codes/mod.rs:435-441, body :275-362; variables n .. n+p-1 are the
 * punctured ones).  Writes up to `cap` pairs (either array may be NULL) and returns the number of edges
 * (= paritycheck_sum, src/codes/mod.rs:405-409); 0 for a bad code. */
size_t labrador_ldpc_hip_edges(enum labrador_ldpc_code code, uint16_t *checks, uint16_t *variables, size_t cap);

/* The contiguous slice [*first, *first + *count) of `batch` frames that part `index` of `parts`
 * takes in a sharded call (slices differ by at most one frame).  Returns a status code. */
int labrador_ldpc_hip_shard_range(size_t batch, size_t parts, size_t index, size_t *first, size_t *count);

/* Number of HIP devices usable by this library (gfx950 only); 0 if none. Never fails. */
int labrador_ldpc_hip_device_count(void);

/* Human-readable description of the calling thread's last failure ("" if none).  The reference-shaped single-frame calls
 * (labrador_ldpc_decode_ms_*, labrador_ldpc_decode_bf) keep the reference's signature and can only return `false` when the
 * library could not run at all (no GPU, a HIP failure, a bad code): they then zero `output`, set *iters_run = max_iters, and
 * leave the reason here -- check it to tell "did not converge" from "did not run" (with LABRADOR_LDPC_HIP_VERBOSE=1 in the
 * environment the reason is also written to stderr, once per distinct failure site). */
const char *labrador_ldpc_hip_last_error(void);

/* Library version string. */
const char *labrador_ldpc_hip_version(void);

/* Identity of the loaded library's BUILD: 16 hex digits, a hash of what determines the code object -- the sources of
 * labrador_ldpc_amd/csrc, this header, the compiler flags and the compiler's version (csrc/build_id.sh) -- not of the produced
 * bytes, which hipcc does not reproduce bit for bit.  Two builds of one source tree report one id; any source or flag edit
 * changes it.  Profiles record the id they were collected on (profiles/hbm_traffic.json, bench.py). */
const char *labrador_ldpc_hip_build_id(void);

/* Name of the kernel labrador_ldpc_decode_ms_batch_i8 launches for a 4-byte-aligned device batch of `batch` frames with this
 * `variant` ("decode_ms_bs_kernel" / "decode_ms_bs_refill_kernel" / "decode_ms_bs_split_kernel" / "decode_ms_bs_split_refill_kernel": bit-sliced; "decode_ms_pair_kernel" /
 * "decode_ms_kernel": the f32-pipe kernels) -- the default dispatch depends on the batch size; harnesses label their
 * measurements with it.  The launcher and this function share one predicate (csrc/decode_ms_i8.hip: pick_i8_kernel).
 * "" for a bad code and for a request this build has no kernel for (the batched call then returns LABRADOR_LDPC_HIP_EUNSUPPORTED);
 * buffers that are NOT 4-byte aligned never take the bit-sliced kernels (default dispatch: the f32-pipe kernel of the code;
 * `variant` 64: EUNSUPPORTED). */
const char *labrador_ldpc_hip_decode_ms_i8_kernel(enum labrador_ldpc_code code, int variant, size_t batch);

/* The LABRADOR_LDPC_HIP_ABI the loaded library was built with: a client that dlopen()s the library compares it with its
 * own header's before passing a struct labrador_ldpc_hip_opts. */
int labrador_ldpc_hip_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LABRADOR_LDPC_HIP_H */
