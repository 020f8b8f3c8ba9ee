// decode_ms_tables.hpp -- which f32-pipe kernels exist per (code, LLR type): the default number of indices per thread and the
// alternatives a `variant` may name.  One table per type serves the hard-only dispatch (decode_ms_<type>.hip), its
// decode_ms_reads_llrs_once and the soft-output dispatch (decode_ms_soft_<type>.hip), so the three cannot drift apart.
#pragma once

#include "codes.hpp"

#define LDPC_TABLE_F32(X) \
    X(TC128,  float, 1) \
    X(TC256,  float, 1) \
    X(TC512,  float, 1) \
    X(TM1280, float, 1) \
    X(TM1536, float, 1, 2) \
    X(TM2048, float, 1, 2) \
    X(TM5120, float, 1) \
    X(TM6144, float, 1, 2) \
    X(TM8192, float, 2, 4)

#define LDPC_TABLE_I8(X) \
    X(TC128,  int8_t, 1) \
    X(TC256,  int8_t, 1) \
    X(TC512,  int8_t, 1) \
    X(TM1280, int8_t, 1) \
    X(TM1536, int8_t, 1, 2) \
    X(TM2048, int8_t, 1) \
    X(TM5120, int8_t, 1) \
    X(TM6144, int8_t, 1, 2) \
    X(TM8192, int8_t, 2)

#define LDPC_TABLE_I16(X) \
    X(TC128,  int16_t, 1) \
    X(TC256,  int16_t, 1) \
    X(TC512,  int16_t, 1) \
    X(TM1280, int16_t, 1) \
    X(TM1536, int16_t, 1, 2) \
    X(TM2048, int16_t, 1) \
    X(TM5120, int16_t, 1) \
    X(TM6144, int16_t, 1, 2) \
    X(TM8192, int16_t, 2)

#define LDPC_TABLE_I32(X) \
    X(TC128,  int32_t, 1) \
    X(TC256,  int32_t, 1) \
    X(TC512,  int32_t, 1) \
    X(TM1280, int32_t, 1) \
    X(TM1536, int32_t, 1) \
    X(TM2048, int32_t, 1) \
    X(TM5120, int32_t, 1) \
    X(TM6144, int32_t, 1) \
    X(TM8192, int32_t, 2)

namespace ldpc {
// f64: the tuned register kernel per code, as a `variant` (IPT | 16 = register-lean | 32 = in place; decode_ms_f64.hip)
// (re-measured on round 3's kernels, tools/f64_variants.py, M codewords/s: TM1280 plain 18.2 / lean 25.6 / in place 21.3; TM6144 in
// place 3.37 / lean 4.04 / lean with two indices 3.82; TM1536 plain 19.5 = lean 19.4; the TC codes plain)
static constexpr int F64_TUNED[NUM_CODES] = {1, 1, 1, 17, 1, 17, 17, 17, 34};
}  // namespace ldpc
