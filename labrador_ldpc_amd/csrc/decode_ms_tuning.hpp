// decode_ms_tuning.hpp -- the tuned settings of the min-sum kernels, in one place.
//
// A LIBRARY build uses exactly the values below: a stray -DLDPC_... or -DBS_... in the build's flags stops it here instead of shipping a
// mistuned decoder.  Same-process A/B experiments on these settings, and the timing diagnostics that leave pieces of the decoder out, live
// outside the library: tools/kbench/ applies its overlay (tools/kbench/diag_overlay.patch) to a COPY of these sources and builds its
// own binaries from that (tools/kb_build.sh); nothing of it is visible to the library's translation units.
#pragma once

#ifndef LDPC_TUNING_OVERRIDES_ALLOWED
#if defined(LDPC_QUARTER_SPECIALISE) || defined(LDPC_NOCAP) || defined(LDPC_LOCAL_IN_VAR) || defined(LDPC_PRIO) || defined(LDPC_PRIO_ROWS) || \
    defined(LDPC_PRIO_ROWS_LEAN) || defined(LDPC_PRIO_VAR) || defined(LDPC_TM2048_WAVES) || defined(LDPC_PAIR_LOCAL_IN_VAR) || \
    defined(LDPC_PRIO_ROWS_PAIR) || defined(LDPC_SELFCORR_CARRY) || defined(LDPC_WAVE_VERDICT) || defined(LDPC_WG_VERDICT) || \
    defined(LDPC_PEEL_FIRST) || defined(LDPC_SELFCORR_MED3) || defined(LDPC_PAIR_SELFCORR_MED3) || defined(LDPC_LEAN_CH) || \
    defined(LDPC_PAIR_HOIST) || defined(LDPC_PAIR_HOIST_F32) || defined(LDPC_PAIR_EARLY_U) || defined(LDPC_PAIR_EARLY_U_F32) || \
    defined(LDPC_PAIR_DEFER_LOCAL) || defined(LDPC_PAIR_DEFER_LOCAL_F32) || defined(LDPC_PAIR_LOCAL_IN_VAR_DEFER) || \
    defined(BS_PLANES) || defined(BS_PIPE) || defined(BS_KEEP_SPLIT) || defined(BS_KEEP_R23) || defined(BS_KEEP_R12) || \
    defined(BS_PINNED_R12) || defined(BS_PINNED_R23) || defined(BS_PINNED_SPLIT) || defined(BS_HARD_LDS) || defined(BS_NZ_LDS) || defined(BS_WAVES_R12) || \
    defined(BS_REFILL_TM5120) || defined(BS_REFILL_R12) || defined(BS_SOFT_LDS_R12) || defined(BS_SOFT_LDS_R23)
#error "the LDPC_* and BS_* tuning switches are fixed in a library build (kernel experiments: tools/kbench/, tools/bs_alt_build.sh)"
#endif
#endif

// ---- decode_ms_kernel.hpp ---------------------------------------------------------------------------------
// Quarter-specialised bodies (one copy per starting quarter, every pi_k constant a literal): 2 = for
// workgroups spanning two or four quarters (+4.6 % on TM8192), 1 = two only, 0 = off.
#ifndef LDPC_QUARTER_SPECIALISE
#define LDPC_QUARTER_SPECIALISE 2
#endif
// Self-correction select through the borrow of an integer subtraction (I class) instead of a float compare (C class):
// -1 = per code (selfcorr_carry_default()), 0 = off, 1 = i8/i16, 2 = f32 too.
#ifndef LDPC_SELFCORR_CARRY
#define LDPC_SELFCORR_CARRY -1
#endif
// Self-correction as a clamp, v = med3(nv, 0, nv + old * big) (Ops<float>::clamp_to_side): -1 = per kernel
// (selfcorr_med3()), 0 = off, 2 = v_fma form, 3 = v_mul_legacy form (6, two full-rate operations and no median: integer messages only).
#ifndef LDPC_SELFCORR_MED3
#define LDPC_SELFCORR_MED3 -1
#endif
#ifndef LDPC_PAIR_SELFCORR_MED3
#define LDPC_PAIR_SELFCORR_MED3 -1
#endif
// Codewords inside one wave (TC codes): barrier-free verdict at the top of the check phase, skipping the rest of the
// phase on success (WAVE_VERDICT in the kernel body).
#ifndef LDPC_WAVE_VERDICT
#define LDPC_WAVE_VERDICT 1
#endif
// iteration 0 as a pass of its own (u = v = 0 folded): -1 = per kernel (peel_first_default()), 0 / 1 = force
#ifndef LDPC_PEEL_FIRST
#define LDPC_PEEL_FIRST -1
#endif
// the same for multi-wave codewords through a third barrier per iteration: -1 = per code and type (WG_VERDICT_SET)
#ifndef LDPC_WG_VERDICT
#define LDPC_WG_VERDICT -1
#endif
// f32: clamp-free check phase for codewords whose LLRs are bounded (NOCAP_POSSIBLE in the kernel body).
#ifndef LDPC_NOCAP
#define LDPC_NOCAP 1
#endif
// Local-edge updates done at the end of the variable phase: -1 = per kernel (local_in_var_default()).
#ifndef LDPC_LOCAL_IN_VAR
#define LDPC_LOCAL_IN_VAR -1
#endif
// Progress-based wave priority.  VALU issue is arbitrated by priority, then age, so the oldest wave
// of a SIMD runs ahead and the youngest arrives last at every barrier, the last stretch of each
// phase with the SIMD half empty.  Lowering a wave's priority as it advances through a phase
// lets the laggards catch up.  The schedule that measured best keeps priority 3 through the edge
// updates and steps down over the last check rows (LDPC_PRIO_ROWS; a sweep of a dozen schedules spans
// 6.06-6.40 M codewords/s on TM8192, the inverted one 5.54): TM8192 5.61 -> 6.40, TM6144 9.64 ->
// 10.83, TM2048 46.9 -> 48.1, TM5120 13.76 -> 14.02 M codewords/s.  Only for codewords of 8 or more waves
// (PRIO_WAVES in the kernel): with one or two waves per codeword it costs (TC512 -7 %, TM1280 -1 %).
// 0 = off, 1 = with a scheduling barrier at each step, 2 = plain.
#ifndef LDPC_PRIO
#define LDPC_PRIO 2
#endif
#ifndef LDPC_PRIO_ROWS
#define LDPC_PRIO_ROWS {2, 2, 1, 1, 1, 0}        // priority during the last six (index, check row) steps of the check phase
#endif
// edges per request chunk of the register-lean check phase (check_phase_lean)
#ifndef LDPC_LEAN_CH
#define LDPC_LEAN_CH 6
#endif
#ifndef LDPC_PRIO_ROWS_LEAN
#define LDPC_PRIO_ROWS_LEAN {3, 3, 3, 2, 1, 0}   // the same for the register-lean check phase
#endif
#ifndef LDPC_PRIO_VAR
#define LDPC_PRIO_VAR 2                          // priority of the first half of the (short) variable phase
#endif
// Waves per SIMD the TM2048 kernels' register allocation must leave room for (min_waves_per_simd()).
#ifndef LDPC_TM2048_WAVES
#define LDPC_TM2048_WAVES 6
#endif

// ---- decode_ms_pair.hpp (each measured with tools/kbench.hip -DKPAIR=1 on TM8192) ---------------------------
// How many of the thread's local-edge updates (of 14 on TM8192) are done at the end of the variable phase
// (LDS-bound: the VALU idles there) instead of at the start of the check phase (VALU-bound), where the
// rest still covers the latency of the marginal reads.  f32 0/3/5/7/9/14 -> 7.04 / 7.07 / 7.24 / 7.41 /
// 7.32 / 7.26 M codewords/s in round 1; re-swept after the multiply form of the self-correction test
// (round 2): 5/6/7/8/9/11 -> 7.23 / 7.30 / 7.40 / 7.49 / 7.41 / 7.14; i8 3/4/5/6/7 -> 6.70 / 6.79 / 6.75 / 6.76 /
// 6.73.  Round 3, with the clamp form of the self-correction (cheaper updates): f32 6/7/8/9/10/12 -> 8.00 / 8.03 / 8.30 / 8.28 /
// 8.33 / 8.15; i8 2/4/6/8 -> 7.43 / 7.45 / 7.35 / 7.55.  -1 = per type (10 for f32, 8 else).
#ifndef LDPC_PAIR_LOCAL_IN_VAR
#define LDPC_PAIR_LOCAL_IN_VAR -1
#endif
// LDS addresses of the loop (the exchanged edges' wired addresses, the variable phase's own position) kept in registers across the
// iterations: LDPC_PAIR_HOIST -1 = per instantiation (PairPlan::HOIST: the hard-output f32 kernels), 0 / 1 = force for every
// instantiation (off / on: formed once per kernel); LDPC_PAIR_HOIST_F32 = 0 / 1 for the adopted instantiations.
#ifndef LDPC_PAIR_HOIST
#define LDPC_PAIR_HOIST -1
#endif
#ifndef LDPC_PAIR_HOIST_F32
#define LDPC_PAIR_HOIST_F32 1
#endif
// How many of the variable phase's exchanged-u reads the loop head issues before it has the previous pass's verdict (EARLY in
// decode_ms_pair_body; only the instantiations with hoisted addresses can): LDPC_PAIR_EARLY_U -1 = per instantiation
// (LDPC_PAIR_EARLY_U_F32 for the adopted ones), 0 = off, n = the first n the phase consumes (at most all of them).
#ifndef LDPC_PAIR_EARLY_U
#define LDPC_PAIR_EARLY_U -1
#endif
#ifndef LDPC_PAIR_EARLY_U_F32
#define LDPC_PAIR_EARLY_U_F32 8
#endif
// How many of the thread's local edges (of 14 on TM8192, in the order of pair_defer_rank) finish their check message at the next
// loop head, under the verdict's LDS round trip, instead of at the VALU-bound end of the check phase (DEFER in decode_ms_pair_body;
// only the instantiations with early u reads have that window): LDPC_PAIR_DEFER_LOCAL -1 = per instantiation
// (LDPC_PAIR_DEFER_LOCAL_F32 for the adopted ones), 0 = off, n = the first n.
#ifndef LDPC_PAIR_DEFER_LOCAL
#define LDPC_PAIR_DEFER_LOCAL -1
#endif
#ifndef LDPC_PAIR_DEFER_LOCAL_F32
#define LDPC_PAIR_DEFER_LOCAL_F32 6
#endif
// LDPC_PAIR_LOCAL_IN_VAR of the instantiations that defer (the two settings were swept together on TM8192: K / LOCAL_IN_VAR 0/10 9.45,
// 0/12 9.48, 0/14 9.50, 4/10 9.46, 4/12 9.37, 4/14 9.52, 5/12 9.55, 6/10 9.40, 6/12 9.65-9.68, 6/13 9.60, 6/14 9.55, 7/12 9.56,
// 8/12 9.56, 8/14 9.45, 10/8 9.13, 10/10 9.18, 10/12 9.40, 11/10 9.09 M codewords/s; docs/experiments.md)
#ifndef LDPC_PAIR_LOCAL_IN_VAR_DEFER
#define LDPC_PAIR_LOCAL_IN_VAR_DEFER 12
#endif

// Wave priority over the six (check row, index) steps of the check phase; 3 before them.  A dozen
// alternatives, also per quarter, measured 6.4-6.75 against 6.75 for this one.
#ifndef LDPC_PRIO_ROWS_PAIR
#define LDPC_PRIO_ROWS_PAIR {3, 3, 2, 2, 1, 0}
#endif

// ---- decode_ms_bitslice.hpp (what an instantiation makes of these, and what each was measured at: BsPlan, decode_ms_bs_plan.hpp;
// alternative builds beside the library's objects: tools/bs_alt_build.sh, which defines LDPC_TUNING_OVERRIDES_ALLOWED) ----------------
// Bit planes of a message / marginal (two's complement).  8 = i8, what the library ships.  The kernel text is written for PL planes: a
// build with -DBS_PLANES=16 decodes with i16 saturation (the experiment behind DESIGN.md section 7: sign-extended i8 LLRs through the
// i8 loader, checked against the i16 oracle in tests/test_bitslice_emu.py) -- twice the instructions and registers per edge.
#ifndef BS_PLANES
#define BS_PLANES 8
#endif
// The next permutation job's ds_bpermute issued behind the current job's arithmetic (BsPlan::PIPE), a bit per class of kernel:
// bit 0 = the two-wave kernels, bit 1 = rate 2/3, bit 2 = rate 1/2.
#ifndef BS_PIPE
#define BS_PIPE 3
#endif
// Exchanged edges per block column whose (sign, magnitude ^ sign) planes are kept from the variable side for the check side
// (BsPlan::KEEP), per class of kernel.
#ifndef BS_KEEP_SPLIT
#define BS_KEEP_SPLIT 3
#endif
#ifndef BS_KEEP_R23
#define BS_KEEP_R23 3
#endif
#ifndef BS_KEEP_R12
#define BS_KEEP_R12 3
#endif
// State updates pinned to their place in the program (BsPlan::PINNED), per class of kernel: 0 / 1.
#ifndef BS_PINNED_R12
#define BS_PINNED_R12 0
#endif
#ifndef BS_PINNED_R23
#define BS_PINNED_R23 1
#endif
#ifndef BS_PINNED_SPLIT
#define BS_PINNED_SPLIT 0
#endif
// Rate 1/2: hard decisions in LDS instead of one register per block column (BsPlan::HARD_LDS): 0 / 1.
#ifndef BS_HARD_LDS
#define BS_HARD_LDS 1
#endif
// Rate 1/2: how many edges' "v != 0" planes live in LDS instead of registers (BsPlan::NZ_LDS; none without BS_HARD_LDS).
#ifndef BS_NZ_LDS
#define BS_NZ_LDS 4
#endif
// Rate 1/2: waves per SIMD the kernels are compiled for (BsPlan::WAVES_PER_SIMD).
#ifndef BS_WAVES_R12
#define BS_WAVES_R12 3
#endif
// Slot refill for the codes with four slots, built and measured slower (BsPlan::REFILL): 1 = build and dispatch it.
#ifndef BS_REFILL_TM5120
#define BS_REFILL_TM5120 0
#endif
#ifndef BS_REFILL_R12
#define BS_REFILL_R12 0
#endif
// The soft form's kept marginal planes (BsPlan::SOFT_LDS), per class of kernel: 0 = in registers, 1 = in LDS.
#ifndef BS_SOFT_LDS_R12
#define BS_SOFT_LDS_R12 0
#endif
#ifndef BS_SOFT_LDS_R23
#define BS_SOFT_LDS_R23 1
#endif
