// decode_ms_pair.hpp -- min-sum decoder (decode_ms<T>, /root/reference/src/decoder.rs:347-475) with
// PAIR ownership: thread t owns the ADJACENT indices 2t and 2t+1 (check 2t, 2t+1 of every block row
// and variable 2t, 2t+1 of every block column) instead of t and t + M/2 as decode_ms_kernel.hpp does.
//
// Why: the LDS, not the VALU, bounds the variable phase of the big codes, and a
// ds_write_b32 costs twice a ds_read_b32.  With adjacent indices
//   * every access at the thread's own position (u reads and marginal stores of the variable phase)
//     is one 64-bit LDS operation for both indices;
//   * a pi_k block rotates a quarter by phi: the images of 2t and 2t+1 are adjacent, and when phi is
//     EVEN they form an aligned pair -- one ds_read_b64 / ds_write_b64 and ONE address for both edges;
//     for odd phi the two marginals are read as halves of two aligned pairs and the two messages keep their
//     32-bit stores (20 of the 32 (block, quarter) rotations of TM8192 are even);
//   * both indices of a thread lie in the same quarter, so every rotation constant is a literal after
//     one wave-uniform branch on the quarter (four copies of the body).
// Everything else -- arithmetic, order of accumulation, exclusive minima, sign words, flags, persistent
// workgroups, wave priorities -- is decode_ms_kernel.hpp's, whose helpers are used here.  Results are
// identical bit for bit (tests/test_gpu_parity.py runs this kernel as a `variant`).
//
// Preconditions (static_asserts): 4-byte register/LDS element types (f32, i8, i16), every exchanged
// block a pi_k, M/8 a multiple of 64 (the 64 lanes of a wave = 128 indices stay inside one quarter).
#pragma once

#include "decode_ms_kernel.hpp"

// Tuned settings (LDPC_PAIR_*, LDPC_PRIO_ROWS_PAIR): decode_ms_tuning.hpp; what an instantiation makes of them: PairPlan.

namespace ldpc {

typedef float ldpc_f2 __attribute__((ext_vector_type(2)));

template <int CODE, class T>
struct PairGeometry {
    static constexpr int M = CODES[CODE].m;
    static constexpr int NT = M / 2;                         // threads per codeword = workgroup size
    static constexpr int NX = count_exchanged(*CODES[CODE].proto);
    static constexpr int NXC = count_exch_cols(*CODES[CODE].proto);
    static constexpr int OUT_LEN = CODES[CODE].output_len();
    static constexpr int LDS_BYTES = ((NX + NXC) * M * 4 + 16 + 15) / 16 * 16;      // exchange slots + two flags, the clamp vote, the next-codeword word
    static_assert(M % 512 == 0 && NT <= 1024, "pair ownership needs M/8 >= 64 lanes per quarter and <= 1024 threads");
};

// rank of local edge (S, B) among a thread's local edges, index-major
constexpr int pair_local_rank(const Prototype &p, int S, int B)
{
    int nloc = 0, r = 0;
    for (int b = 0; b < p.n_blocks; ++b)
        if (blk_local(p.blk[b])) { if (b < B) ++r; ++nloc; }
    return S * nloc + r;
}

constexpr bool all_exchanged_are_pi(const Prototype &p)
{
    for (int b = 0; b < p.n_blocks; ++b)
        if (!blk_local(p.blk[b]) && p.blk[b].kind != BLK_P) return false;
    return true;
}

// The k-th exchange slot the variable phase reads (it walks the block columns in order, and a column's blocks in order), as a block
// number; -1 past the last one.
constexpr int pair_var_read_block(const Prototype &p, int k)
{
    for (int c = 0; c < p.n_cols; ++c)
        for (int b = 0; b < p.n_blocks; ++b)
            if (p.blk[b].col == c && exch_slot(p, b) >= 0 && k-- == 0) return b;
    return -1;
}
constexpr int pair_var_read_rank(const Prototype &p, int B)
{
    for (int k = 0; k < p.n_blocks; ++k)
        if (pair_var_read_block(p, k) == B) return k;
    return -1;
}

// Deferred local edges (PairPlan::DEFER).  The order in which a thread's local edges are deferred: by check row, then index, then
// block -- the edges of one (row, index) share the one sign word that is kept for them, and are taken together.
constexpr int pair_defer_rank(const Prototype &p, int S, int B)
{
    int r = 0;
    for (int b = 0; b < p.n_blocks; ++b)
        if (blk_local(p.blk[b])) {
            if (p.blk[b].row < p.blk[B].row) r += 2;
            else if (p.blk[b].row == p.blk[B].row) r += (S == 1 ? 1 : 0) + (b < B ? 1 : 0);
        }
    return r;
}
constexpr bool pair_deferred(const Prototype &p, int S, int B, int defer)
{
    return blk_local(p.blk[B]) && pair_defer_rank(p, S, B) < defer;
}
// whether the j-th edge of `row` is the first deferred one of its group of three (exclusive_min's groups)
constexpr bool pair_defer_first_of_group(const Prototype &p, int S, int row, int j, int defer)
{
    for (int k = j / 3 * 3; k < j; ++k)
        if (pair_deferred(p, S, row_block(p, row, k), defer)) return false;
    return true;
}
constexpr int count_local(const Prototype &p)
{
    int c = 0;
    for (int b = 0; b < p.n_blocks; ++b) c += blk_local(p.blk[b]) ? 1 : 0;
    return c;
}

// What one instantiation of decode_ms_pair_body is built with.  Each member depends on the ones above it alone: no early reads without
// hoisted addresses, no deferral without early reads, deferral only on the hard-output, uncorrected f32 form.  The settings behind them
// (LDPC_PAIR_*): decode_ms_tuning.hpp.
template <int CODE, class T, bool SOFT, bool CORRECTED>
struct PairPlan {
    static constexpr int NX = PairGeometry<CODE, T>::NX;                        // exchanged u slots = u reads of a variable phase
    static constexpr int NLOCAL = 2 * count_local(*CODES[CODE].proto);          // local edges of a thread
    static constexpr int at_most(int want, int have) { return want < have ? want : have; }
    // The adopted instantiations: the hard-output f32 kernels (forms 2 and 3).  The soft, the corrected and the i8 / i16 instantiations
    // keep the per-phase addresses and their device code: none of them has been measured with the hoist (docs/experiments.md, "Pair
    // kernel: LDS addresses out of the iteration loop").
    static constexpr bool HARD_F32 = std::is_same_v<T, float> && !SOFT && !CORRECTED;

    // HOIST: the LDS addresses of the loop stay in registers across the iterations (formed once per kernel, hoist_addresses() in the
    // body) instead of being formed again in every phase.  The nine wired addresses of the exchanged edges and the variable phase's own
    // position depend on the thread and the quarter body alone.  Formed per phase (the opaque `tq` of the body's phases) they are 37 of the 290 full-rate VALU instructions
    // per wave and iteration of a VALU-bound loop: a shift per phase, an add and a mask per rotation read, and a v_or / v_add of
    // 0x10000 for every block that lies past the 16-bit offset of a ds instruction (the compiler folds the block offsets it can
    // see into the instructions and is left with those).  Hoisted, each address is formed once, carries the lds_bias() of its
    // block and is made opaque, so that the compiler neither re-forms it per phase nor splits the block offset off it again:
    // every access of the loop reaches its block through the instruction's offset alone, 253-257 VALU instructions per
    // iteration.  The check phase held these registers over its whole length already (the u stores reuse the read addresses), so
    // the loop's peak pressure does not move; see forget_llrs() for what the allocator parked in scratch around the loop at first.
    // Measurements: docs/experiments.md, "Pair kernel: LDS addresses out of the iteration loop".
    static constexpr bool HOIST = (LDPC_PAIR_HOIST >= 0 ? LDPC_PAIR_HOIST : HARD_F32 ? LDPC_PAIR_HOIST_F32 : 0) != 0;

    // EARLY: how many of the variable phase's exchanged-u reads the loop head issues before it has the verdict on the previous pass.
    // Only the instantiations with hoisted addresses can: the reads go out on the hoisted bases.
    // The loop head tested the previous pass's verdict -- one LDS word, a full LDS round trip for every wave of the CU at the same
    // moment, right behind a barrier and with nothing else resident -- and only then issued the variable phase's u reads: two round trips
    // in series.  The u reads do not depend on the verdict (nobody writes a u slot before the next check phase, behind another barrier;
    // on the exit path the epilogue ends with a barrier and the next codeword's peeled pass writes no u slot before its own), so the
    // first EARLY of them go out right behind the verdict's read and the head waits for the verdict alone (lgkmcnt(EARLY): LDS returns
    // in order).  The reads are inline asm -- as plain loads the compiler sinks them back below the branch -- so the compiler does not
    // know that their destinations are pending.  What keeps that safe:
    //   * continuing path: each pair is first touched by an asm that waits for it ("+v"), in front of its addition, with a count of its
    //     own (the k-th is back once no more than EARLY - 1 - k operations are outstanding, whatever the compiler issued behind it), so
    //     that the additions start while the later pairs are still on their way.  Nothing may use, copy or spill a pair between its
    //     read and that wait;
    //   * exit path: the pairs are dead there and their registers are reused (fetch_llrs writes VGPRs under vmcnt, which does not order
    //     against a pending LDS return), so lgkmcnt is drained behind the loop, before the next codeword's LLR loads are issued, and
    //     nothing on the way there may write one of those registers;
    //     (both: tests/test_pair_loop_head.py walks every path from the head to the covering wait in the disassembly)
    //   * a counted wait is sound for LDS alone: no scalar memory load may be outstanding at the head (there is none in the loops);
    //   * a value out of an asm is divergent to the compiler: the verdict goes through readfirstlane so that the exit stays a scalar
    //     branch and not an EXEC-masked region (decode_ms_launch.hpp on what those cost TM6144).
    // Only loads move: va, the marginal stores and the local-edge updates stay behind the verdict (the epilogue needs the previous
    // pass's va), and the order of the additions is unchanged.  Measurements: docs/experiments.md, "Pair kernel: the u reads ahead of
    // the verdict".
    // The drain: the loop leaves its head with u reads outstanding, whose destination registers are dead to the compiler and about to
    // be reused.  (Drained behind iterate() and not in front of the `break`: an asm in the loop's exit block changes the shape of the
    // loop, 844 spilled VGPRs.)  Nothing between the exit branch and that wait may write one of them.
    // MAINTENANCE CONSTRAINT: the source cannot enforce that.  Between the loop's exit branch and the drain the compiler schedules
    // what it likes (today: scalar moves, and in form 2 two v_mov_b32 of constants into other registers) into registers it
    // believes free, the pending pairs' among them.  The only guard is tests/test_pair_loop_head.py, which walks the
    // exit path in the disassembly of every loop of forms 2 and 3 and fails when an instruction there names a pending register.
    // Any statement added between iterate() and the drain, any change to what the loop leaves live, and any compiler upgrade has to
    // pass that test before it runs; if it cannot, set LDPC_PAIR_EARLY_U_F32 to 0 and leave the asm alone.
    static constexpr int EARLY = !HOIST ? 0 : at_most(LDPC_PAIR_EARLY_U >= 0 ? LDPC_PAIR_EARLY_U : LDPC_PAIR_EARLY_U_F32, NX);
    static_assert(EARLY >= 0 && EARLY <= 15, "lgkmcnt counts to 15");

    // DEFER: how many of the thread's local edges leave their check message unfinished at the end of the check phase and finish it at
    // the next loop head, behind the early u reads.  Only the instantiations with early reads have that window.
    // While the head waits for the verdict behind its EARLY reads, the VALU of the whole CU idles (all 16 waves stand at the
    // same place, one LDS round trip behind a barrier), and directly on the other side of that barrier, in the VALU-bound end of the
    // check phase where the slowest wave holds up the rest, sit instructions the barrier does not need: the last v_min3_f32 and the
    // sign application of the LOCAL edges' check messages, which no other thread reads and whose first consumer is this thread's own
    // variable phase, behind the verdict.  The first DEFER local edges (pair_defer_rank) leave them out of the check phase -- of the
    // peeled pass too -- and the head finishes them between its last early read and the verdict's wait.  Kept across the barrier for
    // that: the row's sign word per (row, index) with a deferred edge, and for a row of degree >= 4 the partial minimum over the other
    // groups (exclusive_min_part) per group with one; the edge's own u register is free meanwhile, and v does not change between the
    // check phase and the head.  The finished value is the same instruction on the same operands as exclusive_min's, so results are
    // bit-identical.  On the exit path the finished values are dead (the epilogue reads va alone).  The instructions name neither a
    // pending u pair nor the verdict (tests/test_pair_loop_head.py), and each result is pinned: left alone, the compiler sinks
    // them below the exit branch, behind the wait (tests/test_pair_deferred_local.py).  Measurements: docs/experiments.md, "Pair
    // kernel: local edges finished at the loop head".
    static constexpr int DEFER = EARLY == 0 ? 0 : at_most(LDPC_PAIR_DEFER_LOCAL >= 0 ? LDPC_PAIR_DEFER_LOCAL : LDPC_PAIR_DEFER_LOCAL_F32, NLOCAL);
    static_assert(DEFER == 0 || (EARLY > 0 && HARD_F32), "deferred local edges: the instantiations with early u reads");

    // LOCAL_IN_VAR: how many of the thread's local-edge updates run at the end of the variable phase instead of at the start of the
    // check phase.  (With deferred edges the head's window and the variable phase's tail share one LDS-bound stretch, and the best split
    // moved: re-swept together, LDPC_PAIR_LOCAL_IN_VAR_DEFER; the other instantiations keep their 10 / 8.)
    static constexpr int LOCAL_IN_VAR = LDPC_PAIR_LOCAL_IN_VAR >= 0 ? LDPC_PAIR_LOCAL_IN_VAR
                                        : DEFER > 0 ? LDPC_PAIR_LOCAL_IN_VAR_DEFER : (std::is_same_v<T, float> ? 10 : 8);

    // FETCH_EARLY: where the next codeword's LLR loads are issued: before this one's epilogue (4-byte LLRs; the epilogue covers part of
    // their latency) or at the top of its own turn (i8 / i16: the early loads' raw bytes are spilled across the epilogue at the
    // 128-register budget -- which also waits for them on the spot -- 48 spilled registers against 3; fetching a column's two adjacent
    // narrow LLRs with ONE load into ONE register halves what the early fetch keeps alive, and still spills 23 registers against 6:
    // 8.00 -> 7.71, profiles/r03_kbench/kb22_pair_packed_fetch.txt).
    static constexpr bool FETCH_EARLY = sizeof(T) >= 4;
};

// FORM: the self-correction's form (Ops::self_correct): 0 = compare + select, 2 / 3 = the clamp forms
// SOFT: the soft-output form (decode_ms_body's SOFT): the two adjacent marginals of a thread go to `app` as one store.
// CORRECTED: normalized / offset min-sum (decode_ms_body's CORRECTED): m -> max(corr_scale * m - corr_offset, 0) on
// every check message's magnitude, before the signs go on.
template <int CODE, class T, int JW, int FORM, bool SOFT = false, bool CORRECTED = false>
LDPC_DEV void decode_ms_pair_body(const T *__restrict__ llrs, uint8_t *__restrict__ output,
                                  uint32_t *__restrict__ iters_out, uint8_t *__restrict__ success_out,
                                  uint32_t batch, uint32_t maxiters, float nocap_limit, uint32_t *claim, char *lds,
                                  T *__restrict__ app = nullptr, float corr_scale = 1.0f, float corr_offset = 0.0f)
{
    static_assert(!CORRECTED || std::is_same_v<T, float>, "the correction step is built for f32 messages");
    using GEO = PairGeometry<CODE, T>;
    using O = Ops<T>;
    using R = typename O::R;
    static_assert(sizeof(R) == 4 && sizeof(typename O::E) == 4, "pair kernel: 4-byte message types");
    constexpr Prototype P = *CODES[CODE].proto;
    static_assert(all_exchanged_are_pi(P), "pair kernel: exchanged blocks must be pi_k");
    constexpr int M = GEO::M, NT = GEO::NT, NB = P.n_blocks, NROWS = P.n_rows, NCOLS = P.n_cols;
    constexpr int N = CODES[CODE].n, NTX = N / M, NX = GEO::NX, NXC = GEO::NXC;
    constexpr int Q = M / 4, IPT = 2;
    constexpr int BLK_BYTES = M * 4, FLAG_OFF = (NX + NXC) * BLK_BYTES;
    // HOIST, EARLY, DEFER, LOCAL_IN_VAR, FETCH_EARLY: PairPlan, with what each costs, buys and needs to stay safe
    using PLAN = PairPlan<CODE, T, SOFT, CORRECTED>;
    constexpr bool HOIST = PLAN::HOIST, FETCH_EARLY = PLAN::FETCH_EARLY;
    constexpr int EARLY = PLAN::EARLY, DEFER = PLAN::DEFER, LOCAL_IN_VAR = PLAN::LOCAL_IN_VAR;
    [[maybe_unused]] constexpr bool PRIO_WAVES = true;     // the name LDPC_SETPRIO tests (decode_ms_kernel.hpp): a pair codeword has 8 or 16 waves

    const int t = (int)(threadIdx.x & (M / 8 - 1)) + JW * (M / 8);
    __builtin_assume(t >= 0 && t < NT);
    // (a copy of `batch` for the codeword loop and the queue, kept on purpose: with the parameter in its place the lambdas capture one
    // variable less, and the soft-output f32 kernels come out with two VGPRs, the hard-output ones with two SGPR pairs, numbered the
    // other way round -- docs/experiments.md, "The pair kernel without its refuted paths")
    const uint32_t n_groups = batch;
    uint32_t cw = blockIdx.x;

    auto lds1 = [&](int off) LDPC_INLINE -> float & { return *reinterpret_cast<float *>(lds + off); };
    auto lds2 = [&](int off) LDPC_INLINE -> ldpc_f2 & { return *reinterpret_cast<ldpc_f2 *>(lds + off); };
    auto flag_at = [&](uint32_t which) LDPC_INLINE -> int & { return *reinterpret_cast<int *>(lds + FLAG_OFF + 4 * (which & 1)); };
    auto cap_flag = [&]() LDPC_INLINE -> int & { return *reinterpret_cast<int *>(lds + FLAG_OFF + 8); };
    constexpr bool NOCAP_POSSIBLE = std::is_same_v<T, float>;

    // Rotation of block B for this body's quarter JW: phi, and where the even/odd split puts the edges.
    // Byte address (inside the block region, biased as in decode_ms_kernel.hpp) of the variable that check
    // 2t + S is wired to; tb8 = 8 * t.  For even phi the address of S = 1 is that of S = 0 plus 4.
    auto even_c = [](int B) constexpr { return (phi_of(P.blk[B].val, JW, M) & 1) == 0; };
    auto wire = [&](auto B_, auto S_, int tb8) LDPC_INLINE -> int {
        constexpr int B = decltype(B_)::value, S = decltype(S_)::value;
        constexpr int K = P.blk[B].val;
        constexpr int base = (((theta_of(K) + JW) & 3) * Q) * 4 + lds_bias(P, B, BLK_BYTES);
        return ((tb8 + (phi_of(K, JW, M) + S) * 4) & (Q * 4 - 1)) | base;
    };

    // ---- state ---------------------------------------------------------------------------------------
    R u[IPT][NB], v[IPT][NB], va[IPT][NCOLS], llr[IPT][NTX];
    int fnext = 0;                               // EARLY: the byte address of flag_at(it) for the check phase (see `fsel` in iterate)
    (void)fnext;
    ldpc_f2 upre[EARLY > 0 ? EARLY : 1];         // EARLY: the u pairs requested at the loop head, in the variable phase's order
    (void)upre;
    int dsg[IPT][NROWS];                         // DEFER: the sign word of (index, row), for its deferred edges
    R dx[IPT][NROWS][(NB + 2) / 3];              // DEFER: exclusive_min_part of (index, row, group of three), for its deferred edges
    (void)dsg; (void)dx;
    T lraw[IPT][NTX];

    auto fetch_llrs = [&](uint32_t c) LDPC_INLINE {
        unsigned tu = (unsigned)t;
        asm volatile("" : "+v"(tu));
        const uint32_t cc = c < batch ? c : batch - 1;
        static_for<0, NTX>([&](auto C_) LDPC_INLINE {
            constexpr int C = decltype(C_)::value;
            const T *src = (llrs + (size_t)cc * N) + (unsigned)(C * M);
            lraw[0][C] = src[2 * tu];
            lraw[1][C] = src[2 * tu + 1];
        });
    };

    // HOIST: the workgroup's last codeword fetches no successor, and on that path the raw LLRs would keep their old values -- which
    // made them live across the iterations next to `llr` (eight registers, the first thing the allocator parks in scratch when the
    // hoisted addresses take theirs: 4 + 4 dwordx2 spill instructions per codeword and clamp mode).  An empty asm that "writes" them
    // there ends that live range; no instruction is issued for it.
    auto forget_llrs = [&]() LDPC_INLINE {
        static_for<0, IPT>([&](auto S_) LDPC_INLINE {
            static_for<0, NTX>([&](auto C_) LDPC_INLINE {
                if constexpr (sizeof(T) == 4) { T &x = lraw[decltype(S_)::value][decltype(C_)::value]; asm volatile("" : "=v"(x)); }
            });
        });
    };
    (void)forget_llrs;
    // HOIST: had[S][B] = wire(B, S) as request_marginals() forms it; vb[0] = 8t for the blocks below 64 KB, vb[1] = 8t + 64 KB for
    // the rest (the variable phase touches every block of the region at the thread's own position)
    constexpr int VB_HI = 0x10000;
    int had[IPT][NB], vb[2];
    (void)had; (void)vb;
    auto hoist_addresses = [&]() LDPC_INLINE {
        int tq = t;
        asm volatile("" : "+v"(tq));
        const int tb8 = tq * 8;
        vb[0] = tb8;
        asm volatile("" : "+v"(vb[0]));
        if constexpr (FLAG_OFF > VB_HI) {
            vb[1] = tb8 + VB_HI;
            asm volatile("" : "+v"(vb[1]));
        }
        static_for<0, NB>([&](auto B_) LDPC_INLINE {
            constexpr int B = decltype(B_)::value;
            if constexpr (exch_slot(P, B) >= 0) {
                // both regions of the block within the 16-bit offset of the biased address (the + 4: the odd rotations' first store)
                constexpr int lo = lds_bias(P, B, BLK_BYTES);
                static_assert(lds_xu_off(P, exch_slot(P, B), BLK_BYTES) - lo + 4 < 0x10000 && lds_xva_off(P, col_slot(P, P.blk[B].col), BLK_BYTES) - lo + 4 < 0x10000);
                if constexpr (even_c(B)) {
                    had[0][B] = wire(B_, IC<0>{}, tb8);
                } else {
                    had[0][B] = wire(B_, IC<-1>{}, tb8);
                    had[1][B] = wire(B_, IC<1>{}, tb8);
                    asm volatile("" : "+v"(had[1][B]));
                }
                asm volatile("" : "+v"(had[0][B]));
            }
        });
    };
    // the thread's own position in the block at byte offset `off` of the region
    auto own = [&](auto OFF_) LDPC_INLINE -> int {
        constexpr int off = decltype(OFF_)::value;
        if constexpr (off < VB_HI) return vb[0] + off;
        else return vb[1] + (off - VB_HI);
    };
    (void)own;

    auto begin_codeword = [&]() LDPC_INLINE {
        // (a copy of t, once the address of the exchange slots' zeroing that the peeled first pass made unnecessary: one v_mov_b32
        // per codeword, kept so that every instantiation's device code stays what was measured)
        int tq = t;
        asm volatile("" : "+v"(tq));
        static_for<0, IPT>([&](auto S_) LDPC_INLINE {
            constexpr int S = decltype(S_)::value;
            static_for<0, NB>([&](auto B_) LDPC_INLINE {
                constexpr int B = decltype(B_)::value;
                u[S][B] = O::zero();                                                   // decoder.rs:374
                v[S][B] = O::zero();
            });
            static_for<0, NCOLS>([&](auto C_) LDPC_INLINE { va[S][decltype(C_)::value] = O::zero(); });
            static_for<0, NTX>([&](auto C_) LDPC_INLINE { llr[S][decltype(C_)::value] = O::load(lraw[S][decltype(C_)::value]); });
        });
        if (t < 2) flag_at(t) = 0;
        // f32: the clamp of the exclusive minimum at FLT_MAX (decoder.rs:414-415) can only bite if some
        // magnitude reaches FLT_MAX, i.e. if an LLR is infinite or so large that sums overflow.  With every
        // |LLR| <= nocap_limit (derived from max_iters by the host: nocap_limit_for(), decode_ms_launch.hpp)
        // nothing can, and the check phase runs without the clamp operations (8 of 76 min-class
        // instructions per thread and iteration).
        if constexpr (NOCAP_POSSIBLE) {
            bool big = false;
            static_for<0, IPT>([&](auto S_) LDPC_INLINE {
                static_for<0, NTX>([&](auto C_) LDPC_INLINE {
                    const R a = O::mag(llr[decltype(S_)::value][decltype(C_)::value]);
                    big |= !(a <= nocap_limit) || (a != 0.0f && a < 0x1p-20f);     // NaN counts as out of range
                });
            });
            if (__ballot(big) != 0 && (t & 63) == 0) cap_flag() = 1;
        }
    };

    // BND_: the codeword passed the LLR range vote (it runs the clamp-free copy of the loop), which also makes
    // the multiply form of the self-correction test exact (Ops<float>::self_correct_b)
    auto edge_update = [&](auto S_, auto B_, R x, auto BND_) LDPC_INLINE {
        constexpr int S = decltype(S_)::value, B = decltype(B_)::value;
        const R nv = O::sub_nv(x, u[S][B]);                                            // :421
        // the clamp forms need a guarantee about the values: integer messages always have it, f32 only the codewords of the
        // clamp-free loop (they passed the range vote)
        constexpr bool BND = decltype(BND_)::value != 0;
        constexpr int F = (FORM >= 2 && (BND || sizeof(T) <= 2)) ? FORM : 0;
        v[S][B] = O::template self_correct_b<BND, F>(nv, v[S][B]);                     // :422-425
    };

    // DEFER: the check messages of the deferred local edges, from what the last check phase kept (see DEFER above)
    auto finish_deferred = [&]() LDPC_INLINE {
        static_for<0, NROWS>([&](auto R_) LDPC_INLINE {
            constexpr int Rw = decltype(R_)::value;
            constexpr int D = row_degree(P, Rw);
            static_for<0, IPT>([&](auto S_) LDPC_INLINE {
                constexpr int S = decltype(S_)::value;
                R a[D];
                static_for<0, D>([&](auto J_) LDPC_INLINE { a[decltype(J_)::value] = v[S][row_block(P, Rw, decltype(J_)::value)]; });
                static_for<0, D>([&](auto J_) LDPC_INLINE {
                    constexpr int J = decltype(J_)::value;
                    constexpr int B = row_block(P, Rw, J);
                    if constexpr (pair_deferred(P, S, B, DEFER)) {
                        R xg = O::zero();
                        if constexpr (exclusive_min_has_part<D>()) xg = dx[S][Rw][J / 3];
                        const R e = exclusive_min_finish<O, D, true, J>(a, xg);
                        u[S][B] = O::apply_sign(e, dsg[S][Rw], O::sign_word(v[S][B]));
                        asm volatile("" : "+v"(u[S][B]));
                    }
                });
            });
        });
    };
    (void)finish_deferred;

    // ---- variable phase: marginals (decoder.rs:382-383, :408) -------------------------------------
    // FIRST_: iteration 0, a pass of its own: u == 0 and v == 0, see decode_ms_kernel.hpp PEEL_FIRST
    auto variable_phase = [&](auto BND_, auto FIRST_) LDPC_INLINE {
        constexpr bool FIRST = decltype(FIRST_)::value != 0;
        constexpr bool PRE = EARLY > 0 && !FIRST;    // the loop head has requested the first EARLY u pairs (request_u_early)
        (void)PRE;
        int tq = t;
        if constexpr (HOIST == 0) asm volatile("" : "+v"(tq));   // opaque per phase (no address hoisting), but visibly a multiple of 8 below
        const int tb8 = tq * 8;
        (void)tb8;
        LDPC_SETPRIO(LDPC_PRIO_VAR);
        static_for<0, NCOLS>([&](auto C_) LDPC_INLINE {
            constexpr int C = decltype(C_)::value;
            if constexpr (C == NCOLS / 2) LDPC_SETPRIO(0);
            R acc0 = O::zero(), acc1 = O::zero();
            if constexpr (C < NTX) { acc0 = llr[0][C]; acc1 = llr[1][C]; }
            if constexpr (!FIRST)
            static_for<0, NB>([&](auto B_) LDPC_INLINE {
                constexpr int B = decltype(B_)::value;
                if constexpr (P.blk[B].col == C) {
                    constexpr int slot = exch_slot(P, B);
                    if constexpr (slot >= 0) {
                        ldpc_f2 up;
                        constexpr int rank = pair_var_read_rank(P, B);
                        if constexpr (PRE && rank < EARLY) {
                            // requested at the loop head: wait until no more than the reads behind this one are outstanding
                            ldpc_f2 &x = upre[rank];
                            asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(x) : "n"(EARLY - 1 - rank));
                            up = x;
                        }
                        else if constexpr (HOIST != 0) up = lds2(own(IC<lds_xu_off(P, slot, BLK_BYTES)>{}));
                        else up = lds2(lds_xu_off(P, slot, BLK_BYTES) + tb8);
                        acc0 = O::add(acc0, O::from_lds(up.x));
                        acc1 = O::add(acc1, O::from_lds(up.y));
                    } else {
                        acc0 = O::add(acc0, u[0][B]);
                        acc1 = O::add(acc1, u[1][B]);
                    }
                }
            });
            va[0][C] = acc0;
            va[1][C] = acc1;
            constexpr int cs = col_slot(P, C);
            if constexpr (cs >= 0) {
                if constexpr (HOIST != 0) lds2(own(IC<lds_xva_off(P, cs, BLK_BYTES)>{})) = ldpc_f2{O::store(acc0), O::store(acc1)};
                else lds2(lds_xva_off(P, cs, BLK_BYTES) + tb8) = ldpc_f2{O::store(acc0), O::store(acc1)};
            }
        });
        // the local-edge part of the check update for the first LDPC_PAIR_LOCAL_IN_VAR indices, while the
        // marginal stores drain (this phase is LDS-bound, the check phase VALU-bound)
        static_for<0, IPT>([&](auto S_) LDPC_INLINE {
            static_for<0, NB>([&](auto B_) LDPC_INLINE {
                constexpr int S = decltype(S_)::value, B = decltype(B_)::value;
                if constexpr (exch_slot(P, B) < 0 && pair_local_rank(P, S, B) < LOCAL_IN_VAR) {
                    if constexpr (FIRST) v[S][B] = va[S][P.blk[B].col];
                    else edge_update(S_, B_, va[S][P.blk[B].col], BND_);
                }
            });
        });
    };

    // An odd rotation's S = 0 message goes to the HIGH half of the aligned pair its first read address names.  (A constant of the body
    // and not a literal in the store, on purpose: the store's lambdas capture it, as they captured the switch of the retired 32-bit form,
    // and without that capture the hard-output f32 kernels come out with the loops' register copies in another order --
    // docs/experiments.md, "The pair kernel without its refuted paths".)
    constexpr bool ODD_S0_HIGH = true;
    // ---- check phase (decoder.rs:414-450 and :391-405 of the next iteration) -------------------------
    auto check_phase = [&](uint32_t it, auto CAP_, auto FIRST_) LDPC_INLINE {
        constexpr bool CAP = decltype(CAP_)::value != 0;
        constexpr bool FIRST = decltype(FIRST_)::value != 0;
        constexpr int BND = (!CAP && NOCAP_POSSIBLE) ? 1 : 0;
        int par_any = 0;
        int tq = t;
        if constexpr (HOIST == 0) asm volatile("" : "+v"(tq));   // opaque per phase (no address hoisting), but visibly a multiple of 8 below
        const int tb8 = tq * 8;
        (void)tb8;
        LDPC_SETPRIO(3);
        R xs[IPT][NB];
        int ad[IPT][NB];
        auto request_marginals = [&]() LDPC_INLINE {
        static_for<0, NB>([&](auto B_) LDPC_INLINE {                                   // (1) request the exchanged marginals
            constexpr int B = decltype(B_)::value;
            constexpr int slot = exch_slot(P, B);
            if constexpr (slot >= 0) {
                constexpr int cs = col_slot(P, P.blk[B].col);
                constexpr int off = lds_xva_off(P, cs, BLK_BYTES) - lds_bias(P, B, BLK_BYTES);
                if constexpr (HOIST != 0) {
                    ad[0][B] = had[0][B];
                    if constexpr (!even_c(B)) ad[1][B] = had[1][B];
                }
                if constexpr (even_c(B)) {
                    if constexpr (HOIST == 0) ad[0][B] = wire(B_, IC<0>{}, tb8);
                    const ldpc_f2 xp = lds2(off + ad[0][B]);
                    xs[0][B] = O::from_lds(xp.x);
                    xs[1][B] = O::from_lds(xp.y);
                } else {
                    // odd phi: the two marginals are the HIGH half of one aligned pair and the LOW half of the next.
                    // Two ds_read_b64 of those pairs (2 LDS cycles each, conflict-free) instead of two
                    // ds_read_b32 whose 8-byte lane stride is a 2-way bank conflict (4 cycles each).
                    if constexpr (HOIST == 0) {
                        ad[0][B] = wire(B_, IC<-1>{}, tb8);             // aligned pair (2t + phi - 1, 2t + phi)
                        ad[1][B] = wire(B_, IC<1>{}, tb8);              // aligned pair (2t + phi + 1, 2t + phi + 2), wraps with the quarter
                    }
                    const ldpc_f2 lo = lds2(off + ad[0][B]), hi = lds2(off + ad[1][B]);
                    xs[0][B] = O::from_lds(lo.y);
                    xs[1][B] = O::from_lds(hi.x);
                }
            }
        });
        };
        auto local_edges = [&]() LDPC_INLINE {
        static_for<0, IPT>([&](auto S_) LDPC_INLINE {                                  // (2) local edges
            static_for<0, NB>([&](auto B_) LDPC_INLINE {
                constexpr int S = decltype(S_)::value, B = decltype(B_)::value;
                if constexpr (exch_slot(P, B) < 0 && pair_local_rank(P, S, B) >= LOCAL_IN_VAR) {
                    if constexpr (FIRST) v[S][B] = va[S][P.blk[B].col];
                    else edge_update(S_, B_, va[S][P.blk[B].col], IC<BND>{});
                }
            });
        });
        };
        request_marginals();
        __builtin_amdgcn_sched_barrier(0);
        local_edges();
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, IPT>([&](auto S_) LDPC_INLINE {                                  // (3) exchanged edges
            static_for<0, NB>([&](auto B_) LDPC_INLINE {
                constexpr int S = decltype(S_)::value, B = decltype(B_)::value;
                if constexpr (exch_slot(P, B) >= 0) {
                    if constexpr (FIRST) v[S][B] = xs[S][B];
                    else edge_update(S_, B_, xs[S][B], IC<BND>{});
                }
            });
        });
        static_for<0, NROWS>([&](auto R_) LDPC_INLINE {                                // (4) per check row, both indices
            constexpr int Rw = decltype(R_)::value;
            constexpr int D = row_degree(P, Rw);
            static_for<0, IPT>([&](auto S_) LDPC_INLINE {
                constexpr int S = decltype(S_)::value;
                {   // (per-quarter tables against the age bias of the issue arbitration all measured <= this uniform one)
                    constexpr int prio_rows[6] = LDPC_PRIO_ROWS_PAIR;
                    constexpr int step = Rw * IPT + S, nsteps = IPT * NROWS;
                    constexpr int k = step - (nsteps - 6);
                    constexpr int now = k >= 0 ? prio_rows[k] : 3, before = (step > 0 && k >= 1) ? prio_rows[k - 1] : 3;
                    if constexpr (now != before) LDPC_SETPRIO(now);
                }
                R a[D], e[D];
                int sr[D], xw[D];
                static_for<0, D>([&](auto J_) LDPC_INLINE {
                    constexpr int J = decltype(J_)::value;
                    constexpr int B = row_block(P, Rw, J);
                    a[J] = v[S][B];
                    sr[J] = O::sign_word(v[S][B]);                                     // :439-441
                    if constexpr (exch_slot(P, B) >= 0) xw[J] = O::bits(xs[S][B]);     // :445-447
                    else xw[J] = O::bits(va[S][P.blk[B].col]);
                });
                const int sgn = xor_reduce<D>(sr), par = xor_reduce<D>(xw);
                exclusive_min<O, D, true, CAP>(a, e);                                  // :391-395, :430-435
                if constexpr (CORRECTED)
                    static_for<0, D>([&](auto J_) LDPC_INLINE {
                        constexpr int J = decltype(J_)::value;
                        e[J] = __builtin_fmaxf(__fsub_rn(__fmul_rn(corr_scale, e[J]), corr_offset), 0.0f);
                    });
                if constexpr (DEFER > 0) {
                    // what finish_deferred() needs of this (index, row)
                    bool any = false;
                    static_for<0, D>([&](auto J_) LDPC_INLINE {
                        constexpr int J = decltype(J_)::value;
                        if constexpr (pair_deferred(P, S, row_block(P, Rw, J), DEFER)) {
                            any = true;
                            // (the first deferred edge of a group keeps the group's partial minimum)
                            constexpr bool first = pair_defer_first_of_group(P, S, Rw, J, DEFER);
                            if constexpr (exclusive_min_has_part<D>() && first) {
                                dx[S][Rw][J / 3] = exclusive_min_part<O, D, true, CAP, J / 3>(a);
                            }
                        }
                    });
                    if (any) dsg[S][Rw] = sgn;
                }
                static_for<0, D>([&](auto J_) LDPC_INLINE {
                    constexpr int J = decltype(J_)::value;
                    constexpr int B = row_block(P, Rw, J);
                    if constexpr (pair_deferred(P, S, B, DEFER)) return;                              // finish_deferred(), at the next loop head
                    u[S][B] = O::apply_sign(e[J], sgn, sr[J]);                         // :398-405
                    constexpr int slot = exch_slot(P, B);
                    if constexpr (slot >= 0) {
                        constexpr int off = lds_xu_off(P, slot, BLK_BYTES) - lds_bias(P, B, BLK_BYTES);
                        if constexpr (!even_c(B)) lds1(off + ad[S][B] + (ODD_S0_HIGH && S == 0 ? 4 : 0)) = O::store(u[S][B]);
                        else if constexpr (S == 1) lds2(off + ad[0][B]) = ldpc_f2{O::store(u[0][B]), O::store(u[1][B])};
                    }
                });
                par_any |= par;
            });
        });
        if constexpr (EARLY > 0 && !FIRST) { if (par_any < 0) *reinterpret_cast<int *>(lds + fnext) = 1; }     // flag_at(it) = 1
        else if (par_any < 0) flag_at(it) = 1;
    };

    // ---- persistent loop over codewords ----------------------------------------------------------------
    if (t == 0) cap_flag() = 0;
    if constexpr (HOIST != 0) hoist_addresses();
    LDPC_SYNC();
    if (FETCH_EARLY && blockIdx.x < n_groups) fetch_llrs(blockIdx.x);
    // Dynamic distribution of the codewords (claim != nullptr): see decode_ms_body in decode_ms_kernel.hpp.  Thread 0
    // draws a ticket at the start of each decode; the codeword it names, gridDim.x + ticket, is this workgroup's NEXT
    // one.  The returning register is collected after the first pass (collect_claim) into one LDS word, which every wave
    // reads when the decode ends -- many barriers later -- in time for the early LLR fetch.
    const bool dyn = claim != nullptr && maxiters != 0;
    uint32_t ticket = 0;
    int *const next_word = reinterpret_cast<int *>(lds + FLAG_OFF + 12);
    auto collect_claim = [&]() LDPC_INLINE {
        if constexpr (JW == 0) {
            if (dyn && t == 0) {
                *next_word = (int)(gridDim.x + ticket);
                if (ticket == n_groups - 1) __hip_atomic_store(claim, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the launch's last draw
            }
        }
    };
    for (uint32_t g = blockIdx.x; g < n_groups;) {
        cw = (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
        if constexpr (JW == 0) {
            if (dyn && t == 0) ticket = __hip_atomic_fetch_add(claim, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if constexpr (!FETCH_EARLY) fetch_llrs(cw);   // (FETCH_EARLY: this codeword's LLR loads were issued behind the previous epilogue)
        begin_codeword();
        bool done = false, ok = false;
        uint32_t iters = maxiters;
        // the iterations, as one loop per clamp mode (two check phases inside ONE loop cost 330 spilled VGPRs)
        auto iterate = [&](auto CAP_) LDPC_INLINE {
            // iteration 0, a pass of its own (u = v = 0 folded, no exchange slot to zero)
            if (maxiters == 0) { done = true; return; }
            variable_phase(IC<(decltype(CAP_)::value == 0 && NOCAP_POSSIBLE) ? 1 : 0>{}, IC<1>{});
            LDPC_SYNC();
            check_phase(0u, CAP_, IC<1>{});
            collect_claim();
            if constexpr (EARLY > 0) {
                // fsel: the byte address of flag_at(it - 1), toggled once per pass and pinned to the scalar unit.  Derived from `it`
                // and handed to an asm, the address pulls `it`, the cap test and both flag addresses into VGPRs in three of the four
                // quarter bodies (v_add / v_and / v_xor / v_or with the flags' offset as a literal, per iteration).
                // (`it` is declared in front of `fsel`: the other way round the two loop-carried scalars swap their SGPRs)
                uint32_t it = 1;
                int fsel = FLAG_OFF;
                for (;; ++it) {
                    asm volatile("" : "+s"(it));     // (pinned like fsel: the cap test stays an s_cmp, not a VGPR countdown)
                    LDPC_SYNC();
                    int fl, fa;                      // (fa: the address as a VGPR, kept for the store below -- no second v_mov_b32)
                    asm volatile("" : "+s"(fsel));
                    asm volatile("v_mov_b32 %0, %2\n\tds_read_b32 %1, %0" : "=&v"(fa), "=v"(fl) : "s"(fsel));          // flag_at(it - 1)
                    static_for<0, EARLY>([&](auto K_) LDPC_INLINE {
                        constexpr int K = decltype(K_)::value;
                        constexpr int off = lds_xu_off(P, exch_slot(P, pair_var_read_block(P, K)), BLK_BYTES);
                        static_assert((off < VB_HI ? off : off - VB_HI) < 0x10000);
                        ldpc_f2 &x = upre[K];
                        const int &base = vb[off < VB_HI ? 0 : 1];          // (an asm operand inside a generic lambda: a named reference)
                        asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(x) : "v"(base), "n"(off < VB_HI ? off : off - VB_HI));
                    });
                    if constexpr (DEFER > 0) {
                        __builtin_amdgcn_sched_barrier(0);
                        finish_deferred();
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(fl) : "n"(EARLY));          // the verdict alone
                    if (__builtin_amdgcn_readfirstlane(fl) == 0) { done = true; ok = true; iters = it - 1; }   // :453-463
                    else if (it == maxiters) { done = true; }
                    if (done) break;                 // (with reads outstanding: drained behind iterate(), see there)
                    variable_phase(IC<(decltype(CAP_)::value == 0 && NOCAP_POSSIBLE) ? 1 : 0>{}, IC<0>{});
                    LDPC_SYNC();
                    if (t == 0) *reinterpret_cast<int *>(lds + fa) = 0;                   // flag_at(it - 1) = 0
                    fsel ^= 4;
                    asm volatile("" : "+s"(fsel));
                    fnext = fsel;
                    check_phase(it, CAP_, IC<0>{});
                }
            } else
            // (the `it > 0` tests stay: the compiler cannot rule out a 32-bit wrap of `it`, and without them the device code of every
            // instantiation that runs this loop moves)
            for (uint32_t it = 1;; ++it) {
                if (it > 0) LDPC_SYNC();
                if (it > 0 && flag_at(it - 1) == 0) { done = true; ok = true; iters = it - 1; }   // :453-463
                else if (it == maxiters) { done = true; }
                if (done) break;
                variable_phase(IC<(decltype(CAP_)::value == 0 && NOCAP_POSSIBLE) ? 1 : 0>{}, IC<0>{});
                LDPC_SYNC();
                if (it > 0 && t == 0) flag_at(it - 1) = 0;
                check_phase(it, CAP_, IC<0>{});
            }
        };
        LDPC_SYNC();                              // the flags and the clamp vote are visible
        if constexpr (NOCAP_POSSIBLE) {
            if (__builtin_amdgcn_readfirstlane(cap_flag()) != 0) iterate(IC<1>{});
            else iterate(IC<0>{});
        } else {
            iterate(IC<1>{});
        }
        // EARLY: the drain of the u reads that the loop left outstanding.  MAINTENANCE CONSTRAINT (PairPlan::EARLY): no statement between
        // iterate() and this wait without tests/test_pair_loop_head.py.
        if constexpr (EARLY > 0) {
            asm volatile("s_waitcnt lgkmcnt(0)");
            __builtin_amdgcn_sched_barrier(0);
        }
        // the next codeword's LLR loads, issued before this one's epilogue (fixed cost per codeword 2.55 -> 2.12 us)
        const uint32_t g_next = dyn ? (uint32_t)__builtin_amdgcn_readfirstlane(*next_word) : g + gridDim.x;
        if (FETCH_EARLY && g_next < n_groups) fetch_llrs(g_next);
        else if constexpr (HOIST != 0 && FETCH_EARLY && sizeof(T) == 4) forget_llrs();
        // hard decisions, MSB first (decoder.rs:455-461 / :467-473): lane l of a wave holds positions
        // 128w + 2l and 128w + 2l + 1, so the two ballots are interleaved bit by bit (scalar unit:
        // s_bitreplicate doubles every bit), then bit-reversed per byte
        static_for<0, NCOLS>([&](auto C_) LDPC_INLINE {
            constexpr int C = decltype(C_)::value;
            const unsigned long long ev = __ballot(O::bits(va[0][C]) < 0), od = __ballot(O::bits(va[1][C]) < 0);
            unsigned long long w[2];
            static_for<0, 2>([&](auto H_) LDPC_INLINE {
                constexpr int H = decltype(H_)::value;
                unsigned long long re, ro;
                const unsigned e32 = (unsigned)(ev >> (32 * H)), o32 = (unsigned)(od >> (32 * H));
                asm("s_bitreplicate_b64_b32 %0, %1" : "=s"(re) : "s"(e32));
                asm("s_bitreplicate_b64_b32 %0, %1" : "=s"(ro) : "s"(o32));
                const unsigned long long il = (re & 0x5555555555555555ull) | (ro & 0xAAAAAAAAAAAAAAAAull);   // bit p = position 64H + p
                const unsigned lo = __builtin_bswap32(__builtin_bitreverse32((unsigned)il));
                const unsigned hi = __builtin_bswap32(__builtin_bitreverse32((unsigned)(il >> 32)));
                w[H] = (unsigned long long)lo | ((unsigned long long)hi << 32);
            });
            // soft output (decoder.rs:377): marginals 2t and 2t + 1 of the column as one 2 x sizeof(T)-byte store; NaN LLRs put back
            // as in decode_ms_body -- only a wave holding a +inf marginal of the column reads its LLRs again and stores once more
            if constexpr (SOFT) {
                struct alignas(2 * sizeof(T)) Pair { T e, o; };
                unsigned tu = (unsigned)t;
                asm volatile("" : "+v"(tu));    // (no lane offset hoisted out of the codeword loop into a live VGPR)
                Pair *const dst_app = reinterpret_cast<Pair *>(app + (size_t)cw * (NCOLS * M) + C * M + 2 * tu);
                Pair pr{soft_value<T>(va[0][C]), soft_value<T>(va[1][C])};
                *dst_app = pr;
                if constexpr (std::is_floating_point_v<T> && C < NTX) {
                    if (__ballot(va[0][C] == __builtin_inff() || va[1][C] == __builtin_inff()) != 0) {
                        const T *src = (llrs + (size_t)cw * N) + (unsigned)(C * M) + 2 * tu;
                        const T x0 = src[0], x1 = src[1];
                        pr.e = x0 != x0 ? x0 : pr.e;
                        pr.o = x1 != x1 ? x1 : pr.o;
                        *dst_app = pr;
                    }
                }
            }
            if ((t & 63) == 0) {
                unsigned long long *dst = reinterpret_cast<unsigned long long *>((output + (size_t)cw * GEO::OUT_LEN) + (C * M + 2 * t) / 8);
                dst[0] = w[0];
                dst[1] = w[1];
            }
        });
        if (t == 0) { iters_out[cw] = iters; success_out[cw] = ok ? 1 : 0; cap_flag() = 0; }
        LDPC_SYNC();
        g = g_next;
    }
}

// Self-correction form of the pair kernel.  The clamp forms (Ops<float>::clamp_to_side) replace the compare and the select by
// one v_med3_f32: TM8192 f32 7.56 -> 8.32 (form 2) / 8.07 (form 3) / 8.04 (form 5), i8 7.11 -> 7.78 M codewords/s (same-process
// A/B, profiles/r03_kbench/kb1.txt, kb10_forms.txt; identical outputs).  Form 2 is the faster one but narrows the f32 range vote
// (nocap_limit_for): the launcher uses it while that limit leaves room for real LLRs and form 3 beyond.
template <class T>
constexpr int pair_form_default()
{
    if (LDPC_PAIR_SELFCORR_MED3 >= 0) return LDPC_PAIR_SELFCORR_MED3;
    if (sizeof(T) <= 2) return 6;                // integer messages: two full-rate operations (IntOps::self_correct; i8 7.78 -> 7.99)
    return (sizeof(T) > 4 || std::is_same_v<T, int32_t>) ? 0 : 2;
}

template <int CODE, class T, int FORM = pair_form_default<T>()>
__global__ void __launch_bounds__((PairGeometry<CODE, T>::NT))
decode_ms_pair_kernel(const T *__restrict__ llrs, uint8_t *__restrict__ output, uint32_t *__restrict__ iters_out,
                      uint8_t *__restrict__ success_out, uint32_t batch, uint32_t maxiters, float nocap_limit, uint32_t *claim)
{
    using GEO = PairGeometry<CODE, T>;
    __shared__ __attribute__((aligned(16))) char lds[GEO::LDS_BYTES];
    const int jw = __builtin_amdgcn_readfirstlane((int)threadIdx.x) / (GEO::M / 8);          // quarter of this wave's indices
    if (jw == 0) decode_ms_pair_body<CODE, T, 0, FORM>(llrs, output, iters_out, success_out, batch, maxiters, nocap_limit, claim, lds);
    else if (jw == 1) decode_ms_pair_body<CODE, T, 1, FORM>(llrs, output, iters_out, success_out, batch, maxiters, nocap_limit, claim, lds);
    else if (jw == 2) decode_ms_pair_body<CODE, T, 2, FORM>(llrs, output, iters_out, success_out, batch, maxiters, nocap_limit, claim, lds);
    else decode_ms_pair_body<CODE, T, 3, FORM>(llrs, output, iters_out, success_out, batch, maxiters, nocap_limit, claim, lds);
}

// The soft-output form of decode_ms_pair_kernel (a kernel of its own: the hard-only one keeps its argument list and code).
template <int CODE, class T, int FORM = pair_form_default<T>()>
__global__ void __launch_bounds__((PairGeometry<CODE, T>::NT))
soft_decode_ms_pair_kernel(const T *__restrict__ llrs, T *__restrict__ app, uint8_t *__restrict__ output, uint32_t *__restrict__ iters_out,
                           uint8_t *__restrict__ success_out, uint32_t batch, uint32_t maxiters, float nocap_limit, uint32_t *claim)
{
    using GEO = PairGeometry<CODE, T>;
    __shared__ __attribute__((aligned(16))) char lds[GEO::LDS_BYTES];
    const int jw = __builtin_amdgcn_readfirstlane((int)threadIdx.x) / (GEO::M / 8);
    if (jw == 0) decode_ms_pair_body<CODE, T, 0, FORM, true>(llrs, output, iters_out, success_out, batch, maxiters, nocap_limit, claim, lds, app);
    else if (jw == 1) decode_ms_pair_body<CODE, T, 1, FORM, true>(llrs, output, iters_out, success_out, batch, maxiters, nocap_limit, claim, lds, app);
    else if (jw == 2) decode_ms_pair_body<CODE, T, 2, FORM, true>(llrs, output, iters_out, success_out, batch, maxiters, nocap_limit, claim, lds, app);
    else decode_ms_pair_body<CODE, T, 3, FORM, true>(llrs, output, iters_out, success_out, batch, maxiters, nocap_limit, claim, lds, app);
}

}  // namespace ldpc
