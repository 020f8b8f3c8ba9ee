// decode_ms_bs_plan.hpp -- what an instantiation of the bit-sliced i8 min-sum decoder (decode_ms_bitslice.hpp) is built with, per code,
// and the table the dispatch (decode_ms_i8.hip) and the launchers (decode_ms_bs.hip) read it through.
//
// Plain C++ (codes.hpp and the settings alone): the GPU build, the host dispatch and tests/c/bitslice_emu.cpp read the same text.
// The settings behind the members (BS_*): decode_ms_tuning.hpp.
#pragma once

#include "codes.hpp"
#include "decode_ms_tuning.hpp"

namespace ldpc {
namespace bs {

// the codes the bit-sliced kernels exist for: the CCSDS TM (AR4JA) codes.  (The TC codes' circulants are not quarter-wise rotations.)
constexpr bool bitsliced_code(int code) { return code >= TM1280 && code <= TM8192; }

// the codes the soft-output form of those kernels exists for (decode_ms_bs_soft.hip): the one-wave codes -- not the two rate-4/5 codes,
// whose two-wave kernels have none
constexpr bool bitsliced_soft_code(int code) { return code == TM1536 || code == TM2048 || code == TM6144 || code == TM8192; }

enum class Rate { R12, R23, R45 };

template <int CODE>
struct BsPlan {
    static_assert(bitsliced_code(CODE), "TM codes only");
    // The rate class, from the prototype: 15 / 24 / 39 edges.  Everything below follows from it, from the code's size, or is a measured
    // per-code figure.
    static constexpr int EDGES = CODES[CODE].proto->n_blocks;
    static constexpr Rate RATE = EDGES > 30 ? Rate::R45 : EDGES > 20 ? Rate::R23 : Rate::R12;
    static constexpr int W = CODES[CODE].m / 32;        // lanes per codeword
    static constexpr int G = 64 / W;                    // codewords per wave (per pair of waves: TWO_WAVES)
    static constexpr int per_rate(int r12, int r23, int r45) { return RATE == Rate::R12 ? r12 : RATE == Rate::R23 ? r23 : r45; }

    // the rate-4/5 codes (39 edges: 218 planes of state before any temporary) exist only in the two-waves-per-group form
    // (decode_ms_bitslice_split.hpp); the one-wave geometry of such a code (Geo<CODE, -1>: the bit-flipping decoder's layout, the
    // whole-codeword helpers) takes this plan as well -- no kernel runs the min-sum iteration in that form
    static constexpr bool TWO_WAVES = RATE == Rate::R45;

    // M = 128 (TM1280): a quarter is ONE lane and a codeword one quad of lanes, so the lane permutation of a pi_k block is a rotation of
    // the quad by theta_k -- a DPP quad_perm on a v_mov_b32 (no LDS, no latency; nothing at all for theta_k = 0) instead of a
    // ds_bpermute_b32, which at two waves per SIMD costs the SIMD ~4.4 x a VALU instruction (profiles/r04_kbench/sdwa_rate.txt).
    static constexpr bool QUAD = W == 4;

    // PIPE: a permutation job's eight ds_bpermute are issued one job AHEAD of their use.
    // BS_PIPE bit 0: the two-wave kernels, bit 1: rate 2/3, bit 2: rate 1/2 (which has no registers for it: 21-23 spilled values, -3 %).
    // What it buys is not hidden latency -- the SIMD's other wave hid that already -- but ONE s_waitcnt per job instead of one per
    // plane: a job's results have long arrived when they are collected (profiles/r05_kbench/permute_pipeline.txt: +1.2 ... +1.9 %).
    static constexpr bool PIPE = (per_rate(4, 2, 1) & BS_PIPE) != 0 && !QUAD;

    // KEEP: an exchanged edge's u is needed twice, at check alignment: permuted into the marginal (variable side) and subtracted from the
    // permuted marginal (check side).  For the first KEEP exchanged edges of a block column the (sign, magnitude ^ sign) planes formed
    // for the variable side are KEPT for the check side instead of formed again (the seven XORs and whatever of the row-state multiplexer
    // the compiler did not carry over by itself; the registers exist: the kept planes die at the start of the check side, before its peak).
    // Measured +0.4 ... +2 % on every code (profiles/r05_kbench/permute_pipeline.txt).
    static constexpr int KEEP = per_rate(BS_KEEP_R12, BS_KEEP_R23, BS_KEEP_SPLIT);

    // PINNED: every state update of the rate-2/3 codes is pinned to its place in the program (Decoder::pin_update): without that the
    // instruction selector's data-flow order keeps values whose next use is an iteration away live to the end of the block.  The
    // rate-1/2 codes fit their registers without the pins and run 6 % faster with the freedom (TM8192 16.9 against 15.9 M codewords/s);
    // the two-wave form of the rate-4/5 codes measured 36.8 (no pins) against 36.3 / 34.4 (profiles/r04_kbench/split_rate.txt).
    static constexpr bool PINNED = per_rate(BS_PINNED_R12, BS_PINNED_R23, BS_PINNED_SPLIT) != 0;

    // HARD_LDS: hard decisions in LDS instead of one register per block column (one ds_write per column and iteration; a read as well
    // where a wave holds several codewords, whose finished ones keep their decisions): the rate-1/2 codes, which that brings under the
    // 168 registers of three waves per SIMD.  (In registers, on the final schedule: TM8192 20.83 against 20.49, TM2048 71.84 / 97.62
    // against 72.01 / 98.17 M codewords/s -- inside the run-to-run spread; profiles/r05_kbench/bs_occupancy.txt, run 8, "hl0".)
    static constexpr bool HARD_LDS = RATE == Rate::R12 && BS_HARD_LDS != 0;

    // NZ_LDS: rate 1/2 (three waves per SIMD, 168 registers): the "v != 0" plane of the first NZ_LDS edges lives in LDS -- read once and
    // written once per iteration, at the edge's check side -- in the part of the staging slab that the hard-decision words leave free
    // during the iterations: four planes the register allocator would otherwise keep in scratch (spilled values 11/14 -> 8/10; TM8192 i8
    // +2...+3.5 %, TM2048 +1.5 %).  More than the slab holds costs a wave per CU: 6 planes -3 % (profiles/r05_kbench/spill_leak.txt).
    static constexpr int NZ_LDS = HARD_LDS ? BS_NZ_LDS : 0;

    // waves per SIMD the kernel is compiled for.  Rate 1/2 (TM2048, TM8192): THREE -- 168 registers -- since round 5: a row's running
    // state replaces its old state with the row's last edge, block row 0 finishes first, the hard decisions live in LDS
    // (decode_ms_bitslice.hpp, "schedule of an iteration").  Rate 2/3 and the two-wave kernels: two (256 registers).
    static constexpr int WAVES_PER_SIMD = per_rate(BS_WAVES_R12, 2, 2);

    // REFILL: the build carries a slot-refill kernel for this code (decode_refill / decode_refill_split: a finished codeword's lanes take
    // the next frame at once) and the dispatch uses it.  Eight and sixteen slots (TM1536, TM1280): adopted, 1.31 x / 1.275 x.  Four
    // slots lose little to the lockstep and the per-slot events cost more: TM2048 -1 ... -4 % (its codeword passes the staging slab in
    // two pieces -- the "v != 0" planes of the active slots live behind the hard-decision words), TM5120 -4 % (4 dB) / -8 % (2 dB);
    // built, bit-exact, off (profiles/r06_kbench/slot_refill_r06.txt; BS_REFILL_R12 / BS_REFILL_TM5120 build them).  One or two slots: none.
    static constexpr bool REFILL = G >= 8 || (G == 4 && per_rate(BS_PLANES == 8 && BS_REFILL_R12, 0, BS_REFILL_TM5120) != 0);

    // UNIT: which of the two compile units of decode_ms_bs.hip builds the code's kernels: 1 = the default machine scheduler, 2 = -mllvm
    // -amdgpu-sched-strategy=iterative-ilp, which is worth +2 % on the two-wave kernels and +0.5 % on rate 2/3 but costs the rate-1/2
    // kernels (168 registers, spilling) 2.5 % (profiles/r05_kbench/permute_pipeline.txt, section 7).
    static constexpr int UNIT = per_rate(1, 2, 2);

    // SOFT_LDS, SOFT_WAVES_PER_SIMD: the soft form (Decoder<..., SOFT>, decode_ms_bs_soft.hip) keeps the seven magnitude
    // planes of every block column's marginal beside the hard word: NCOLS x 7 planes, 35 (rate 1/2) or 49 (rate 2/3) -- in REGISTERS, or
    // in LDS behind the wave's other areas (NCOLS x 7 x 256 bytes: 8 960 / 12 544), written once per iteration and column (read and
    // selected as well where a wave holds several codewords).
    // Rate 1/2: REGISTERS, at two waves per SIMD (196 / 212 registers, no spill; LDS stays the plain kernel's): TM8192 18.87, TM2048
    // 64.61 M codewords/s.  In LDS the wave needs 21 504 bytes -- seven waves per CU, stated as one per SIMD -- and pays the LDS
    // traffic: 16.55 / 56.61.
    // Rate 2/3: the plain kernels need 233 registers at two waves per SIMD, so 49 more planes exist only at ONE wave per SIMD (283
    // registers) or in LDS -- 30 720 bytes per wave, five waves per CU, which the launch bounds can only state as one per SIMD as well
    // (two would promise eight).  LDS: TM6144 11.84, TM1536 46.73; registers at one wave per SIMD 11.02 / 43.71.
    // (One MI355X, 2 dB, cap 25, tools/bs_soft_rate.py: DESIGN.md 4.16 and docs/experiments.md.)
    static constexpr bool SOFT_LDS = per_rate(BS_SOFT_LDS_R12, BS_SOFT_LDS_R23, 0) != 0;
    static constexpr int SOFT_WAVES_PER_SIMD = per_rate(SOFT_LDS ? 1 : 2, 1, 0);         // (0: the two-wave kernels have no soft form)

    // MIN_GROUPS: groups of G codewords from which the bit-sliced kernel is faster per call than the f32-pipe kernels, which it then
    // replaces in the default dispatch (tools/bs_crossover.py, profiles/r05_kbench/bs_crossover.txt: TM8192 and TM1280 cross at 1024
    // groups, TM6144 and TM5120 at 768, TM2048 and TM1536 at 2048)
    static constexpr int MIN_GROUPS = (CODE == TM8192 || CODE == TM1280) ? 1024 : (CODE == TM6144 || CODE == TM5120) ? 768 : 2048;
};

// Waves per SIMD a corrected form (decode_ms_bs_corrected.hip, decode_ms_bs_quantised.hip) is compiled for: the plan's -- but for the
// rate-1/2 codes' forms with a multiply, which at the plan's three (168 registers) carry 13 to 20 scratch instructions inside the
// iteration where the plain kernels carry none: those are built for two.
template <int CODE, int MULBITS>
constexpr int corrected_waves_per_simd() { return BsPlan<CODE>::RATE == Rate::R12 && MULBITS > 0 ? 2 : BsPlan<CODE>::WAVES_PER_SIMD; }

// ---- the plan as the dispatch reads it at run time: one row per code (the TC codes' rows: no bit-sliced kernel, at any batch size) ----
struct BsDispatch {
    bool built = false, two_waves = false, refill = false;
    int unit = 0;
    size_t min_batch = ~(size_t)0;              // MIN_GROUPS x G frames
};
template <int CODE>
constexpr BsDispatch dispatch_row()
{
    using PLAN = BsPlan<CODE>;
    return {true, PLAN::TWO_WAVES, PLAN::REFILL, PLAN::UNIT, (size_t)PLAN::MIN_GROUPS * PLAN::G};
}
inline constexpr BsDispatch BS_DISPATCH[NUM_CODES] = {{}, {}, {}, dispatch_row<TM1280>(), dispatch_row<TM1536>(), dispatch_row<TM2048>(),
                                                      dispatch_row<TM5120>(), dispatch_row<TM6144>(), dispatch_row<TM8192>()};

// Today's table, so that a change of the plan is a visible edit here as well
#ifndef LDPC_TUNING_OVERRIDES_ALLOWED
static_assert(BsPlan<TM1280>::TWO_WAVES && BsPlan<TM5120>::TWO_WAVES && !BsPlan<TM1536>::TWO_WAVES && !BsPlan<TM6144>::TWO_WAVES &&
              !BsPlan<TM2048>::TWO_WAVES && !BsPlan<TM8192>::TWO_WAVES, "TM1280 and TM5120 are two-wave");
static_assert(BsPlan<TM1280>::REFILL && BsPlan<TM1536>::REFILL && !BsPlan<TM2048>::REFILL && !BsPlan<TM5120>::REFILL &&
              !BsPlan<TM6144>::REFILL && !BsPlan<TM8192>::REFILL, "TM1280 and TM1536 refill");
static_assert(BsPlan<TM2048>::WAVES_PER_SIMD == 3 && BsPlan<TM8192>::WAVES_PER_SIMD == 3 && BsPlan<TM1280>::WAVES_PER_SIMD == 2 &&
              BsPlan<TM1536>::WAVES_PER_SIMD == 2 && BsPlan<TM5120>::WAVES_PER_SIMD == 2 && BsPlan<TM6144>::WAVES_PER_SIMD == 2,
              "rate 1/2 builds at 3 waves per SIMD, the rest at 2");
static_assert(BsPlan<TM2048>::UNIT == 1 && BsPlan<TM8192>::UNIT == 1 && BsPlan<TM1280>::UNIT == 2 && BsPlan<TM1536>::UNIT == 2 &&
              BsPlan<TM5120>::UNIT == 2 && BsPlan<TM6144>::UNIT == 2, "TM2048 and TM8192 in unit 1, the rest in unit 2");
static_assert(!BsPlan<TM2048>::SOFT_LDS && !BsPlan<TM8192>::SOFT_LDS && BsPlan<TM1536>::SOFT_LDS && BsPlan<TM6144>::SOFT_LDS,
              "the soft form keeps its planes in registers on rate 1/2, in LDS on rate 2/3");
#endif

}  // namespace bs
}  // namespace ldpc
