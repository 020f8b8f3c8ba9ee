// decode_ms_ops.hpp -- the arithmetic of the min-sum decoders per LLR type (Ops<T>: DecodeFrom, decoder.rs:22-86), the exclusive
// minimum of a check row built on it, and the conversion of a marginal back to the LLR type.  Shared by the flooding kernels
// (decode_ms_kernel.hpp, decode_ms_pair.hpp) and the layered ones (decode_ms_layered.hpp, decode_ms_fixed_layered.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstdint>
#include <type_traits>

#include "decode_ms_util.hpp"

namespace ldpc {

// ---- arithmetic per LLR type: DecodeFrom, decoder.rs:22-86 ----------------------------------
// Register values are kept so that "negative" (hard_bit, decoder.rs:49/:76) is exactly bit 31
// of the 32-bit pattern: true for two's-complement ints, and true for floats because no
// value in this kernel is ever -0.0 (LLRs are canonicalised with +0.0 on load; sums and
// differences of such values cannot produce -0.0; see DESIGN.md "signed zeros").
template <class T> struct Ops;

template <> struct Ops<float> {                       // decoder.rs:69-77
    using R = float;                                   // register type
    using E = float;                                   // LDS exchange element type
    LDPC_DEV static R zero() { return 0.0f; }
    LDPC_DEV static R maxval() { return FLT_MAX; }                              // :72
    // -0.0 -> +0.0, and every NaN -> +inf.
    // NaN LLRs: the reference's hard_bit is `x < 0.0` (:76), false for a NaN whatever its sign bit, while this kernel reads
    // "negative" from bit 31, so a sign-carrying NaN must not reach the registers.  Clearing that bit on the common path
    // (compare + select, integer bit tricks, an asm bundle, a ballot and a cold fix-up branch: all tried) cost the kernels at
    // their register limit 20-50 spilled registers.  But a NaN LLR and a +inf LLR are THE SAME INPUT to decode_ms -- every
    // output bit, the iteration count and the success flag agree:
    //   * the marginal is NaN + u resp. inf + u, for ever (u is finite: +-min1 / min2 <= maxval, :391-405): never `< 0`, so
    //     hard bit 0 (:457, :469) and no contribution to the parity (:445);
    //   * every message along the variable's edges is NaN - u resp. inf - u = the same again; it is kept by the
    //     self-correction (old v is 0, then itself: `hard_bit() ==` holds, :422), is never `< 0` (no sign contribution, :439),
    //     and its magnitude NaN resp. inf passes neither `< min1` nor `< min2` (:430, :433) nor `== min1` (:391): the checks
    //     see an edge that takes no part in the minima, and its own u is min1 either way.
    // So the load maps NaN to +inf with one v_min_f32 -- minNum(NaN, inf) = inf; the add before it quiets a signalling NaN,
    // which minNum would otherwise turn into a quiet NaN.  +inf LLRs were always part of the contract (tests since round 1).
    // (Written with the builtin, not as inline asm: an asm statement between a load and its use makes the compiler wait
    // for every LLR load on the spot -- ten serialised L2 round trips per variable phase in the register-lean kernel.)
    LDPC_DEV static R load(float x) { return __builtin_fminf(x + 0.0f, __builtin_inff()); }
    // LATE canonicalisation, for the kernels where the load-time form does not come for free.  Without the NaN mapping the
    // compiler never materialised `llr = raw + 0.0`: it kept the raw registers and folded the `+ 0.0` into the copy that starts
    // each marginal's accumulation.  A two-operation load() cannot be folded that way; it becomes a second set of values, and
    // the two kernels that sit at a forced register limit (TM1280 f32 at 168, the register-lean TM5120 f32 at 128) spilled
    // 20-45 more registers for it (-17 % / -16 %, profiles/r03_kbench/kb4.txt).  Those kernels keep the RAW LLR (keep_raw), add
    // it as it is, and canonicalise the finished marginal instead: raw + u1 + ... equals llr + u1 + ... as a VALUE at every
    // step (a -0.0 addend behaves like +0.0 unless everything is -0.0), `+ 0.0` then turns a -0.0 result into +0.0, and a NaN
    // LLR leaves a NaN marginal, which min(., inf) maps to the +inf marginal a +inf LLR would have left.  One more v_min per
    // transmitted column and iteration, no extra registers.
    LDPC_DEV static R canon_late(R x) { return __builtin_fminf(x + 0.0f, __builtin_inff()); }
    LDPC_DEV static R keep_raw(float x) { return x; }
    LDPC_DEV static R load_nonan(float x) { return x + 0.0f; }                   // first of two NaN passes (NONAN in the kernel body): -0.0 -> +0.0 only
    LDPC_DEV static float store(R x) { return x; }
    LDPC_DEV static R from_lds(float x) { return x; }                           // already canonical
    LDPC_DEV static int bits(R x) { return __float_as_int(x); }
    static constexpr bool SIGN_WORD_IS_BIT31_ONLY = true;      // (the register-lean check phases form it from raw bits themselves)
    LDPC_DEV static int sign_word(R x) { return __float_as_int(x) & (int)0x80000000; }     // bit 31 of a message, alone
    LDPC_DEV static R add(R a, R b) { return a + b; }                           // :74
    LDPC_DEV static R sub(R a, R b) { return a - b; }                           // :75
    LDPC_DEV static R sub_nv(R a, R b) { return a - b; }                        // the new v of an edge (:421)
    LDPC_DEV static R mag(R x) { return __builtin_fabsf(x); }                   // :73 (may be +inf)
    // min of magnitudes.  AX/AY/AZ say whether the operand is a signed message whose magnitude is
    // meant (the |x| source modifier is free) or already a magnitude.  Written as asm so that the
    // operation tree of exclusive_min() is emitted as designed: through fminf() LLVM re-associates
    // it into ~50 % more v_min ops plus canonicalising v_max ops.
    template <bool AX, bool AY>
    LDPC_DEV static R min2(R x, R y)
    {
        R d;
        if constexpr (AX && AY) asm("v_min_f32_e64 %0, |%1|, |%2|" : "=v"(d) : "v"(x), "v"(y));
        else if constexpr (AX) asm("v_min_f32_e64 %0, |%1|, %2" : "=v"(d) : "v"(x), "v"(y));
        else if constexpr (AY) asm("v_min_f32_e64 %0, %1, |%2|" : "=v"(d) : "v"(x), "v"(y));
        else asm("v_min_f32_e32 %0, %1, %2" : "=v"(d) : "v"(x), "v"(y));
        return d;
    }
    // min(maxval, ...): the cap comes from an SGPR
    template <bool AX>
    LDPC_DEV static R min2_cap(R x)
    {
        R d;
        const float cap = FLT_MAX;
        if constexpr (AX) asm("v_min_f32_e64 %0, |%1|, %2" : "=v"(d) : "v"(x), "s"(cap));
        else asm("v_min_f32_e32 %0, %2, %1" : "=v"(d) : "v"(x), "s"(cap));
        return d;
    }
    template <bool AX, bool AY>
    LDPC_DEV static R min3_cap(R x, R y)
    {
        R d;
        const float cap = FLT_MAX;
        if constexpr (AX && AY) asm("v_min3_f32 %0, |%1|, |%2|, %3" : "=v"(d) : "v"(x), "v"(y), "s"(cap));
        else if constexpr (!AX && !AY) asm("v_min3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(x), "v"(y), "s"(cap));
        else d = min2_cap<false>(min2<AX, AY>(x, y));
        return d;
    }
    template <bool AX, bool AY, bool AZ>
    LDPC_DEV static R min3(R x, R y, R z)
    {
        R d;
        if constexpr (AX && AY && AZ) asm("v_min3_f32 %0, |%1|, |%2|, |%3|" : "=v"(d) : "v"(x), "v"(y), "v"(z));
        else if constexpr (AX && AY) asm("v_min3_f32 %0, |%1|, |%2|, %3" : "=v"(d) : "v"(x), "v"(y), "v"(z));
        else if constexpr (!AX && !AY && !AZ) asm("v_min3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(x), "v"(y), "v"(z));
        else d = min2<false, AZ>(min2<AX, AY>(x, y), z);
        return d;
    }
    // magnitude `m` (>= 0) with the sign taken from bit 31 of `s`
    LDPC_DEV static R with_sign(R m, int s)
    {
        return __int_as_float((__float_as_int(m) & 0x7FFFFFFF) | (s & (int)0x80000000));
    }
    LDPC_DEV static R select_zero(bool z, R x) { return z ? 0.0f : x; }
    // x where p is not a negative non-zero number, else +0: "bits(p) <= 0x80000000" as the borrow of an integer
    // subtraction (an I-class VOP2 operation that pairs with the F and I classes) instead of a float compare (C class)
    LDPC_DEV static R keep_unless_negative(R p, R x)
    {
        // (the same through __builtin_usub_overflow, which lets the compiler place the wait states, measures within
        // +-1 % of this bundle on every kernel)
        R r;
        asm("v_subrev_co_u32_e32 %0, vcc, %2, %1\n\ts_nop 1\n\tv_cndmask_b32_e32 %0, 0, %3, vcc"
            : "=&v"(r) : "v"(p), "s"(0x80000001u), "v"(x) : "vcc");
        return r;
    }
    // Self-correction test of decoder.rs:422: drop nv iff old != 0 and sign(nv) != sign(old).
    // `old` with its sign flipped when nv is negative is a negative NON-ZERO float exactly then
    // (old is never -0.0), so one three-input bit op (old ^ (nv & 0x80000000)) and one float
    // compare decide it; "-0.0 < 0" is false, which is the old == 0 case.  (A NaN nv -- always the positive quiet
    // one, see load() -- leaves t = old: dropped iff old < 0, kept otherwise, as `NaN.hard_bit() == old.hard_bit()`.)
    LDPC_DEV static bool drop(R nv, R old)
    {
        const int t = __builtin_amdgcn_bitop3_b32(__float_as_int(old), __float_as_int(nv), (int)0x80000000, 0x78);
        return __int_as_float(t) < 0.0f;
    }
    // Self-correction as a CLAMP (FORM 2 / 3).  "Keep nv iff it lies on old's side of zero (any side if old == 0)" is
    // v = median(nv, 0, X) for any X with X = nv when old == 0 and, when old != 0, the sign of old and |X| >= |nv|.
    //   FORM 2:  X = fma(old, big, nv)   (one v_fma_f32: full rate on gfx950, tools/ubench/valu_rate.hip) -- needs
    //            big * |old| > |nv| for every nonzero old and every nv of the decode, which the caller guarantees (integer
    //            messages: big = 2^20; f32: the tightened range vote, nocap_limit_for());
    //   FORM 3:  X = nv + mul_legacy(old, inf): +-inf for every nonzero old (denormals included), 0 * inf = 0 under
    //            the legacy rule, so no range condition beyond "nothing is NaN or infinite".
    // (A form 5 -- the same decision without a median, s = clamp01(1 + nv * old * 2^100), v = nv * s + 0: three full-rate
    // operations, none of the 4-cycle class -- lost on every kernel where it was tried and is retired: docs/experiments.md.)
    // One v_med3_f32 replaces the compare and the select of forms 0 / 1, and with them the VCC round trip between the two
    // (two wait states on gfx950): sub, fma, med3 instead of sub, mul, cmp, cndmask.  Per edge update 0.94 ns against
    // 1.13-1.25 ns per instruction slot in the micro-benchmark (profiles/r03_final/valu_rate.txt).
    template <int FORM>
    LDPC_DEV static R clamp_to_side(R nv, R old, float big)
    {
        static_assert(FORM == 2 || FORM == 3, "clamp forms of the self-correction: 2, 3 (6: integer messages only, IntOps)");
        R x, r;
        if constexpr (FORM == 2) {
            asm("v_fma_f32 %0, %1, %2, %3" : "=v"(x) : "s"(big), "v"(old), "v"(nv));
        } else {
            asm("v_mul_legacy_f32_e64 %0, %1, %2" : "=v"(x) : "v"(old), "s"(__builtin_inff()));
            x = x + nv;
        }
        asm("v_med3_f32 %0, %1, 0, %2" : "=v"(r) : "v"(nv), "v"(x));
        return r;
    }
    // nv, or +0 where drop(nv, old)  (zeroing by EXEC predication instead of v_cndmask measured slower:
    // EXEC writes stall the VALU -- DESIGN.md 4.4)
    // FORM: 0 = compare + select, 1 = the select through keep_unless_negative (chosen per kernel, see selfcorr_form())
    // (the clamp forms need a guarantee about the values: self_correct_b)
    template <int FORM>
    LDPC_DEV static R self_correct(R nv, R old)
    {
        if constexpr (FORM == 1) {
            const int t = __builtin_amdgcn_bitop3_b32(__float_as_int(old), __float_as_int(nv), (int)0x80000000, 0x78);
            return keep_unless_negative(__int_as_float(t), nv);
        } else {
            return select_zero(drop(nv, old), nv);
        }
    }
    // The same for codewords whose LLRs passed the range vote (BOUNDED: every |LLR| <= nocap_limit and every
    // nonzero |LLR| >= 2^-20, see begin_codeword): "old != 0 and the signs differ" is then exactly "nv * old < 0".
    // No value is infinite (the nocap bound), and every value of the decode is a multiple of g = 2^(e_min - 23),
    // e_min >= -20 the exponent of the smallest nonzero |LLR| (sums and differences of multiples of g round to
    // multiples of g), so a nonzero value is at least 2^-43 and a product of two cannot underflow; nv == 0 gives
    // v = 0 whichever way the test goes.  An F-class v_mul_f32 in place of the VOP3 bit operation: +1 %.
    // FORM 2 / 3: the clamp forms above (FORM 2 with big = 2^126: the launch's limit then also keeps
    // 2^126 * 2^-43 above every magnitude of the decode, nocap_limit_for()).
    template <bool BOUNDED, int FORM = 0>
    LDPC_DEV static R self_correct_b(R nv, R old)
    {
        if constexpr (BOUNDED && FORM >= 2) {
            return clamp_to_side<FORM>(nv, old, 0x1p126f);
        } else if constexpr (BOUNDED) {
            float p;
            asm("v_mul_f32_e32 %0, %1, %2" : "=v"(p) : "v"(nv), "v"(old));
            if constexpr (FORM == 1) return keep_unless_negative(p, nv);
            else return select_zero(p < 0.0f, nv);
        } else {
            return self_correct<(FORM == 1 ? 1 : 0)>(nv, old);
        }
    }
    // m >= 0 has bit 31 clear, so "m with sign s_all ^ s_own" is one three-input XOR of sign words
    LDPC_DEV static R apply_sign(R m, int s_all, int s_own)
    {
        return __int_as_float(__builtin_amdgcn_bitop3_b32(__float_as_int(m), s_all, s_own, 0x96));
    }
};

// f64 LLRs (decoder.rs:78-86): two VGPRs per value, the sign is bit 31 of the HIGH word, so the
// sign-word machinery (bits / apply_sign) works on that word; no -0.0 either (load adds +0.0).
// Plain expressions instead of pinned instruction trees: f64 is the least used variant and its
// VALU ops are quarter rate whatever the tree looks like.
template <> struct Ops<double> {
    using R = double;
    using E = double;
    LDPC_DEV static R zero() { return 0.0; }
    LDPC_DEV static R maxval() { return DBL_MAX; }
    LDPC_DEV static R load(double x) { return __builtin_fmin(x + 0.0, __builtin_inf()); }      // -0.0 -> +0.0, NaN -> +inf: see Ops<float>::load
    LDPC_DEV static R canon_late(R x) { return __builtin_fmin(x + 0.0, __builtin_inf()); }
    LDPC_DEV static R keep_raw(double x) { return x; }
    LDPC_DEV static R load_nonan(double x) { return x + 0.0; }
    LDPC_DEV static double store(R x) { return x; }
    LDPC_DEV static R from_lds(double x) { return x; }
    LDPC_DEV static int bits(R x) { return __double2hiint(x); }
    static constexpr bool SIGN_WORD_IS_BIT31_ONLY = true;
    LDPC_DEV static int sign_word(R x) { return __double2hiint(x) & (int)0x80000000; }
    LDPC_DEV static R add(R a, R b) { return a + b; }
    LDPC_DEV static R sub(R a, R b) { return a - b; }
    LDPC_DEV static R sub_nv(R a, R b) { return a - b; }
    LDPC_DEV static R mag(R x) { return __builtin_fabs(x); }
    template <bool AX, bool AY>
    LDPC_DEV static R min2(R x, R y)
    {
        const R a = AX ? __builtin_fabs(x) : x, b = AY ? __builtin_fabs(y) : y;
        return __builtin_fmin(a, b);              // v_min_f64: a NaN operand is ignored, as the reference's `<` does (:430-434)
    }
    template <bool AX> LDPC_DEV static R min2_cap(R x) { return min2<AX, false>(x, DBL_MAX); }
    template <bool AX, bool AY> LDPC_DEV static R min3_cap(R x, R y) { return min2<false, false>(min2<AX, AY>(x, y), DBL_MAX); }
    template <bool AX, bool AY, bool AZ>
    LDPC_DEV static R min3(R x, R y, R z) { return min2<false, AZ>(min2<AX, AY>(x, y), z); }
    template <int FORM>
    LDPC_DEV static R self_correct(R nv, R old)                                  // decoder.rs:422-425
    {
        return (old != 0.0 && (nv < 0.0) != (old < 0.0)) ? 0.0 : nv;
    }
    template <bool BOUNDED, int FORM = 0> LDPC_DEV static R self_correct_b(R nv, R old) { return self_correct<0>(nv, old); }
    LDPC_DEV static R apply_sign(R m, int s_all, int s_own)
    {
        return __hiloint2double(__double2hiint(m) ^ s_all ^ s_own, __double2loint(m));
    }
};

// Integer LLR types run on the float pipeline: i8/i16 values and every intermediate of the
// algorithm are integers of magnitude <= 2^16, which f32 represents exactly, so saturating
// add/sub (decoder.rs:47-48, :56-57) are an f32 add/sub followed by a clamp, and all the sign-bit
// and exclusive-minimum machinery of the f32 path applies unchanged.  saturating_abs(-2^(b-1)) =
// 2^(b-1)-1 (decoder.rs:46, :55) falls out of capping the exclusive minimum at maxval.
template <class I, int LO, int HI> struct IntOps : Ops<float> {     // decoder.rs:42-59
    LDPC_DEV static R maxval() { return (float)HI; }
    LDPC_DEV static R load(I x) { return (float)(int)x; }                       // never -0.0
    LDPC_DEV static R canon_late(R x) { return x; }
    LDPC_DEV static R keep_raw(I x) { return (float)(int)x; }
    LDPC_DEV static R load_nonan(I x) { return (float)(int)x; }
    LDPC_DEV static R clamp(R x) { return __builtin_amdgcn_fmed3f(x, (float)LO, (float)HI); }
    LDPC_DEV static R add(R a, R b) { return clamp(a + b); }                    // saturating_add
    LDPC_DEV static R sub(R a, R b) { return clamp(a - b); }                    // saturating_sub
    // The new v of an edge, decoder.rs:421, WITHOUT the clamp of saturating_sub: v is only ever used through its
    // sign, its zero-ness (both unchanged by the clamp) and min(|v|, maxval) inside the capped exclusive minimum
    // (saturating_abs of the clamped value IS min(|a - b|, maxval), whichever end clamped), so the clamp is dead
    // work; a - b is exact in f32 (|a - b| < 2^17).  One v_med3 less per edge and iteration.
    LDPC_DEV static R sub_nv(R a, R b) { return a - b; }
    LDPC_DEV static R mag(R x) { return __builtin_fminf(__builtin_fabsf(x), (float)HI); }   // saturating_abs
    // (the sign word of an integer message as 0.0 * x = +-0.0 -- a float multiply instead of a v_and -- measures 0 to -2 %:
    // profiles/r03_kbench/kb19_sign_by_mul.txt)
    // Self-correction test of decoder.rs:422 for integer-valued messages: old != 0 and the signs differ exactly
    // when the product is negative -- |nv|, |old| < 2^17, so the f32 product can neither underflow to zero nor
    // lose its sign (it may round), and nv == 0 gives v = 0 whichever way the test goes.  An F-class v_mul_f32
    // (co-issues with the 4-cycle instructions of other waves) instead of the VOP3 bit operation of the f32 path,
    // where the same trick would need a vote on the LLR range (+1 %).
    LDPC_DEV static bool drop(R nv, R old)
    {
        float p;
        asm("v_mul_f32_e32 %0, %1, %2" : "=v"(p) : "v"(nv), "v"(old));
        return p < 0.0f;
    }
    // FORM 2 / 3: the clamp forms of Ops<float>::clamp_to_side -- exact for every integer message: |nv| < 2^17 and a
    // nonzero |old| >= 1, so 2^20 * |old| > |nv| always
    // FORM 6: the decision without a median.  Integer messages are zero or at least 1 in magnitude, so nv * old is <= -1 when
    // the signs differ, >= 1 when they agree and 0 when either is zero: s = clamp01(fma(nv, old, 1)) is 0 / 1 / 1 with no scale
    // factor, and v = fma(nv, s, 0) (the + 0 keeps a dropped negative nv from becoming -0.0).  Two full-rate instructions per
    // update and no 4-cycle one (form 2: fma + med3).  The product is below 2^33 and rounds, but never across zero.
    template <int FORM>
    LDPC_DEV static R self_correct(R nv, R old)
    {
        if constexpr (FORM == 6) {
            float sel, r;
            asm("v_fma_f32 %0, %1, %2, 1.0 clamp" : "=v"(sel) : "v"(nv), "v"(old));
            asm("v_fma_f32 %0, %1, %2, 0" : "=v"(r) : "v"(nv), "v"(sel));
            return r;
        } else if constexpr (FORM >= 2) {
            return Ops<float>::clamp_to_side<FORM>(nv, old, 0x1p20f);
        } else if constexpr (FORM == 1) {
            float p;
            asm("v_mul_f32_e32 %0, %1, %2" : "=v"(p) : "v"(nv), "v"(old));
            return Ops<float>::keep_unless_negative(p, nv);
        } else {
            return Ops<float>::select_zero(drop(nv, old), nv);
        }
    }
    template <bool BOUNDED, int FORM = 0> LDPC_DEV static R self_correct_b(R nv, R old) { return self_correct<FORM>(nv, old); }
    template <bool AX>
    LDPC_DEV static R min2_cap(R x)
    {
        R d;
        const float cap = (float)HI;
        if constexpr (AX) asm("v_min_f32_e64 %0, |%1|, %2" : "=v"(d) : "v"(x), "s"(cap));
        else asm("v_min_f32_e32 %0, %2, %1" : "=v"(d) : "v"(x), "s"(cap));
        return d;
    }
    template <bool AX, bool AY>
    LDPC_DEV static R min3_cap(R x, R y)
    {
        R d;
        const float cap = (float)HI;
        if constexpr (AX && AY) asm("v_min3_f32 %0, |%1|, |%2|, %3" : "=v"(d) : "v"(x), "v"(y), "s"(cap));
        else if constexpr (!AX && !AY) asm("v_min3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(x), "v"(y), "s"(cap));
        else d = min2_cap<false>(Ops<float>::min2<AX, AY>(x, y));
        return d;
    }
};
template <> struct Ops<int8_t>  : IntOps<int8_t, -128, 127> {};
template <> struct Ops<int16_t> : IntOps<int16_t, -32768, 32767> {};

// i32 LLRs (decoder.rs:60-68): genuine 32-bit integer arithmetic -- the f32 pipeline is exact only to 2^24.
// Saturating add/sub are v_add_i32 / v_sub_i32 with the clamp bit.  Those, every integer min / max / compare and the three-operand
// integer forms issue at HALF the rate of v_xor / v_sub_u32 / v_ashrrev / v_bitop3 on gfx950 (tools/ubench/wide_rate.hip: 1.8 against
// 0.95 ns per wave-instruction and SIMD), which is why decode_ms::<i32> runs at about half decode_ms::<f32>'s rate (f32 add / sub / fma
// are full rate, |x| is a free source modifier there and the sign application one v_bitop3).  Round 6 moved what it could to
// full-rate operations (TM8192 i32 4.24 -> see profiles/r06_final/rates_all_codes.txt):
//   * the self-correction without a compare (self_correct below: four full-rate operations for xor + two v_cmp + s_and + select);
//   * the MAGNITUDE as the wrapping |x| (one v_sub_u32 + one v_max_i32 instead of v_sub_i32 clamp + v_max_i32).  It wraps where
//     saturating_abs saturates -- |INT_MIN| comes out as 0x80000000 instead of INT_MAX (:64) -- so magnitudes are compared UNSIGNED and
//     every exclusive minimum is capped at maxval = INT_MAX (which decoder.rs:414-415 does anyway: min1 / min2 start there):
//     min(sat|a|, ...) = min_u32(wrap|a|, INT_MAX, ...).  The cap rides in a v_min3_u32's third operand except on rows of degree 2 and
//     4-6 (one operation more per three edges).
//   (Sign words as x >> 31 -- which would also save the shift in apply_sign -- were measured at the compiler: 118 spilled registers
//   in the TM8192 pair kernel against 1; not adopted.)
// "Negative" is bit 31, so the sign-word machinery applies unchanged.  The LDS element is a 4-byte container (float) holding the
// integer's bits, which lets the pair kernel's 64-bit accesses carry it.
template <> struct Ops<int32_t> {
    using R = int;
    using E = float;
    LDPC_DEV static R zero() { return 0; }
    LDPC_DEV static R maxval() { return 0x7FFFFFFF; }                           // :63
    LDPC_DEV static R load(int32_t x) { return x; }
    LDPC_DEV static R canon_late(R x) { return x; }
    LDPC_DEV static R keep_raw(int32_t x) { return x; }
    LDPC_DEV static R load_nonan(int32_t x) { return x; }
    LDPC_DEV static float store(R x) { return __int_as_float(x); }
    LDPC_DEV static R from_lds(float x) { return __float_as_int(x); }
    LDPC_DEV static int bits(R x) { return x; }
    static constexpr bool SIGN_WORD_IS_BIT31_ONLY = true;
    LDPC_DEV static int sign_word(R x) { return x & (int)0x80000000; }
    LDPC_DEV static R add(R a, R b) { R d; asm("v_add_i32 %0, %1, %2 clamp" : "=v"(d) : "v"(a), "v"(b)); return d; }   // :65
    LDPC_DEV static R sub(R a, R b) { R d; asm("v_sub_i32 %0, %1, %2 clamp" : "=v"(d) : "v"(a), "v"(b)); return d; }   // :66
    LDPC_DEV static R sub_nv(R a, R b) { return sub(a, b); }                    // (32-bit: the clamp is what keeps it from wrapping)
    // |x| as an UNSIGNED word (wraps INT_MIN to 0x80000000 where :64 saturates to INT_MAX): see above
    LDPC_DEV static R mag(R x) { const R s = x >> 31; return (R)((unsigned)(x ^ s) - (unsigned)s); }
    LDPC_DEV static R umin(R a, R b) { return (unsigned)b < (unsigned)a ? b : a; }
    template <bool AX, bool AY>
    LDPC_DEV static R min2(R x, R y)
    {
        const R a = AX ? mag(x) : x, b = AY ? mag(y) : y;
        return umin(a, b);
    }
    template <bool AX> LDPC_DEV static R min2_cap(R x) { return umin(AX ? mag(x) : x, maxval()); }
    template <bool AX, bool AY> LDPC_DEV static R min3_cap(R x, R y) { return umin(min2<AX, AY>(x, y), maxval()); }
    template <bool AX, bool AY, bool AZ>
    LDPC_DEV static R min3(R x, R y, R z) { return min2<false, AZ>(min2<AX, AY>(x, y), z); }
    // decoder.rs:422-425: v = 0 where the old v is non-zero and of the other sign, else nv -- without a compare: bit 31 of
    // (nv ^ old) & (old | -old) says "drop" (old | -old has bit 31 set exactly for old != 0, INT_MIN included); an arithmetic shift
    // spreads it over the word and it is cleared out of nv: v_sub_u32, v_bitop3, v_ashrrev, v_bitop3 -- all full rate
    template <int FORM>
    LDPC_DEV static R self_correct(R nv, R old)
    {
        const int negold = (int)(0u - (unsigned)old);
        const int drop = __builtin_amdgcn_bitop3_b32(nv, old, negold, 0x2C) >> 31;          // (a ^ b) & (b | c)
        return __builtin_amdgcn_bitop3_b32(nv, drop, drop, 0x30);                           // a & ~b
    }
    template <bool BOUNDED, int FORM = 0> LDPC_DEV static R self_correct_b(R nv, R old) { return self_correct<0>(nv, old); }
    // m >= 0 negated when the product of the other edges' signs is negative (:398-405)
    LDPC_DEV static R apply_sign(R m, int s_all, int s_own)
    {
        const int k = (s_all ^ s_own) >> 31;                                     // 0 or -1
        return (m ^ k) - k;
    }
};

// e[i] = min(maxval, min over j != i of a[j]).  Equals what decoder.rs:391-395 selects from
// (min1, min2): min2 if |v_i| is a smallest magnitude of the check, min1 otherwise -- and
// min1/min2 start at maxval (decoder.rs:414-415) and are only replaced by strictly smaller
// values (:430-434), hence the clamp.  Elements are grouped in threes so that one min3 per
// element finishes the job: ~1.7 operations per edge at degree 6, ~1.9 at degree 18.
template <class O, int D, bool ABS, bool CAP = true>
LDPC_DEV void exclusive_min(const typename O::R (&a)[D], typename O::R (&e)[D])
{
    // CAP = false: the caller guarantees that every magnitude is below maxval (then the clamp is the
    // identity); only checks of degree >= 4 save operations by it
    using R = typename O::R;
    const R MX = O::maxval();
    if constexpr (D == 1) {
        e[0] = MX;
    } else if constexpr (D == 2) {
        if constexpr (CAP) {
            e[0] = O::template min2_cap<ABS>(a[1]);
            e[1] = O::template min2_cap<ABS>(a[0]);
        } else {
            e[0] = ABS ? O::mag(a[1]) : a[1];
            e[1] = ABS ? O::mag(a[0]) : a[0];
        }
    } else if constexpr (D == 3) {
        e[0] = O::template min3_cap<ABS, ABS>(a[1], a[2]);
        e[1] = O::template min3_cap<ABS, ABS>(a[0], a[2]);
        e[2] = O::template min3_cap<ABS, ABS>(a[0], a[1]);
    } else {
        constexpr int G = (D + 2) / 3;
        R t[G], x[G];
        static_for<0, G>([&](auto g_) LDPC_INLINE {
            constexpr int g = decltype(g_)::value, n = (3 * g + 3 <= D) ? 3 : D - 3 * g;
            if constexpr (n == 3) t[g] = O::template min3<ABS, ABS, ABS>(a[3 * g], a[3 * g + 1], a[3 * g + 2]);
            else if constexpr (n == 2) t[g] = O::template min2<ABS, ABS>(a[3 * g], a[3 * g + 1]);
            else t[g] = ABS ? O::mag(a[3 * g]) : a[3 * g];
        });
        exclusive_min<O, G, false, CAP>(t, x);
        static_for<0, G>([&](auto g_) LDPC_INLINE {
            constexpr int g = decltype(g_)::value, n = (3 * g + 3 <= D) ? 3 : D - 3 * g;
            if constexpr (n == 3) {
                e[3 * g]     = O::template min3<ABS, ABS, false>(a[3 * g + 1], a[3 * g + 2], x[g]);
                e[3 * g + 1] = O::template min3<ABS, ABS, false>(a[3 * g],     a[3 * g + 2], x[g]);
                e[3 * g + 2] = O::template min3<ABS, ABS, false>(a[3 * g],     a[3 * g + 1], x[g]);
            } else if constexpr (n == 2) {
                e[3 * g]     = O::template min2<ABS, false>(a[3 * g + 1], x[g]);
                e[3 * g + 1] = O::template min2<ABS, false>(a[3 * g],     x[g]);
            } else {
                e[3 * g] = x[g];
            }
        });
    }
}

// The two halves of exclusive_min() for a caller that finishes some elements later (decode_ms_pair.hpp, DEFER): the partial minimum
// x[g] "over the other groups" that element J's group is finished with (nothing to keep for D <= 3), and e[J] from it -- the same
// instruction with the same operand order as exclusive_min() issues for that element, so the value is the same bit for bit.
template <int D>
constexpr bool exclusive_min_has_part() { return D >= 4; }

template <class O, int D, bool ABS, bool CAP, int GRP>
LDPC_DEV typename O::R exclusive_min_part(const typename O::R (&a)[D])
{
    static_assert(D >= 4, "rows of degree <= 3 are finished from their elements alone");
    using R = typename O::R;
    constexpr int G = (D + 2) / 3;
    R t[G], x[G];
    static_for<0, G>([&](auto g_) LDPC_INLINE {
        constexpr int g = decltype(g_)::value, n = (3 * g + 3 <= D) ? 3 : D - 3 * g;
        if constexpr (n == 3) t[g] = O::template min3<ABS, ABS, ABS>(a[3 * g], a[3 * g + 1], a[3 * g + 2]);
        else if constexpr (n == 2) t[g] = O::template min2<ABS, ABS>(a[3 * g], a[3 * g + 1]);
        else t[g] = ABS ? O::mag(a[3 * g]) : a[3 * g];
    });
    exclusive_min<O, G, false, CAP>(t, x);
    return x[GRP];
}

template <class O, int D, bool ABS, int J>
LDPC_DEV typename O::R exclusive_min_finish(const typename O::R (&a)[D], typename O::R xg)
{
    static_assert(D >= 3, "rows of degree 1 and 2 have nothing to finish");
    constexpr int g = J / 3, n = (3 * g + 3 <= D) ? 3 : D - 3 * g;
    constexpr int o0 = 3 * g + (J % 3 == 0 ? 1 : 0), o1 = 3 * g + (J % 3 == 2 ? 1 : 2);    // the other two of a full group, in order
    if constexpr (D == 3) return O::template min3_cap<ABS, ABS>(a[o0], a[o1]);
    else if constexpr (n == 3) return O::template min3<ABS, ABS, false>(a[o0], a[o1], xg);
    else if constexpr (n == 2) return O::template min2<ABS, false>(a[3 * g + 1 - J % 3], xg);
    else return xg;
}

// A marginal as an element of the LLR type: the integer types' registers hold exact integers inside the type's range (IntOps),
// the others are the type itself.
template <class T, class R>
LDPC_DEV T soft_value(R x)
{
    if constexpr (std::is_same_v<T, int8_t> || std::is_same_v<T, int16_t>) return (T)(int)x;
    else return (T)x;
}

}  // namespace ldpc
