// decode_ms_layered.hpp -- block-row layered min-sum decoding of f32 LLR batches for gfx950 (MI355X).
//
// The flooding kernels (decode_ms_kernel.hpp, decode_ms_pair.hpp) run the reference's schedule: every check of an iteration reads
// marginals a whole iteration old.  This kernel runs a LAYERED schedule: block row r of the prototype (a "layer") updates its checks
// from marginals that already hold the new messages of rows 0 .. r-1 of the same sweep.  The contract, per sweep:
//
//     for every layer r in ascending order:
//         va[j] = llr[j] (0 for punctured j) + the u of j's edges in edge order        (for the variables the layer touches)
//         for every edge e = (c, j) of layer r:  nv = va[j] - u[e];  v[e] = self-corrected nv   (decoder.rs:421-426)
//         u[e] = exclusive minimum of the other |v| of its check (capped at FLT_MAX), with their sign product  (decoder.rs:391-441)
//     va = llr + sum of u; the sweep succeeds when every check's parity over hard(va) is 0
//
// Layout.  One codeword per NT = M / IPT threads (IPT: the flooding default's indices per thread, LDPC_TABLE_F32), index-aligned
// ownership as in the flooding kernels: a thread owns index i (and i + NT, ...) and with it check i of every block row -- the v of its
// edges live in registers for the whole decode.  The u of every edge live in LDS at the position of their VARIABLE: u of edge
// (block b, check index i) at U[b][f_b(i)], f_b the block's shift or pi_k.  The marginal of variable (column C, index k) is then
// llr + U[b0][k] + U[b1][k] + ... over the blocks of column C in block order -- the reference's edge order restricted to the
// variable -- read by whichever thread needs it, so no marginal array is kept and the accumulation order is the reference's.
// A layer is one compute step (marginals from U, new v, exclusive minima, new u in registers), a barrier (a row's cells with two or
// three terms read each other's u), the u stores, and a barrier; a sweep ends with a parity pass (hard bits of every variable to
// LDS, barrier, per-check parities and a vote word, barrier).  Codewords of one wave (the TC codes) need no s_barrier: LDS
// operations of one wave complete in order, so the hand-offs are an lgkmcnt wait.
//
// LLRs are copied into LDS once per codeword, -0.0 read as +0.0 and NaN as +inf (Ops<float>::load; the hard results of a NaN LLR are
// those of a +inf LLR); the soft form puts the NaN back where the LLR is one, and returns +0.0 for -0.0.  Hard bits are kept as one
// bit per variable, written by a ballot per wave and codeword (TM8192: 120 KB of u, 32 KB of LLRs and 1.25 KB of bits).
#pragma once

#include "decode_ms_ops.hpp"         // Ops<float>, exclusive_min; static_for, row_block, pi_dev, LDPC_SYNC
#include "decode_ms_tables.hpp"      // LDPC_TABLE_F32: the flooding default's indices per thread
#include "llr_widen.hpp"             // widen_llr: the rule of the half-precision loader

namespace ldpc {

// the flooding default's indices per thread (first column of LDPC_TABLE_F32)
#define LDPC_LAYERED_IPT_CASE(CODE, T, DEF, ...) case CODE: return DEF;
constexpr int layered_ipt(int code)
{
    switch (code) {
        LDPC_TABLE_F32(LDPC_LAYERED_IPT_CASE)
        default: return 1;
    }
}
#undef LDPC_LAYERED_IPT_CASE

template <int CODE>
struct LayeredGeometry {
    static constexpr Prototype P = *CODES[CODE].proto;
    static constexpr int IPT = layered_ipt(CODE);
    static constexpr int M = CODES[CODE].m;
    static constexpr int N = CODES[CODE].n;
    static constexpr int NP = CODES[CODE].n + CODES[CODE].p;
    static constexpr int NT = M / IPT;                       // threads per codeword
    static constexpr int G = NT >= 64 ? 1 : 64 / NT;         // codewords per workgroup
    static constexpr int WG = NT * G;
    static constexpr int NB = P.n_blocks, NROWS = P.n_rows, NCOLS = P.n_cols, NTX = N / M;
    static constexpr int OUT_LEN = CODES[CODE].output_len();
    // per codeword: U [NB][M] f32 | LLR [N] f32 | hard bits [NCOLS * M] (bit x of the array = variable x) | two vote words
    static constexpr int U_OFF = 0;
    static constexpr int L_OFF = NB * M * 4;
    static constexpr int H_OFF = L_OFF + N * 4;
    static constexpr int F_OFF = H_OFF + (NCOLS * M / 8 + 7) / 8 * 8;
    static constexpr int HW = NT < 64 ? NT : 64;             // bits one ballot store writes (a wave, or a codeword inside one)
    static constexpr int CW_BYTES = (F_OFF + 8 + 15) / 16 * 16;
    static constexpr size_t LDS_BYTES = (size_t)G * CW_BYTES + 16;
    static_assert(M % IPT == 0 && NT >= 16 && (NT & (NT - 1)) == 0 && NT % 8 == 0, "bad IPT");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

// variable index (inside its column) of check index i in block B
template <int CODE, int B>
LDPC_DEV int layered_map(int i)
{
    constexpr Block blk = CODES[CODE].proto->blk[B];
    constexpr int M = CODES[CODE].m;
    if constexpr (blk.kind == BLK_I) return (i + blk.val) & (M - 1);
    else return pi_dev<blk.val, M>(i, i >> ilog2(M / 4));
}

// workgroup (or, for one-wave workgroups, wave) hand-off of LDS data
template <int WG>
LDPC_DEV void layered_sync()
{
    if constexpr (WG <= 64) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    else LDPC_SYNC();
}

// CORRECTED: normalized / offset min-sum -- every message magnitude m becomes max(scale * m - offset, +0.0), a rounded
// f32 multiply and a rounded f32 subtract (0 < scale <= 1, 0 <= offset <= FLT_MAX, checked by capi.hip: m is finite, so neither an
// infinity nor a NaN can arise).  `scale` and `offset` are wave-uniform kernel arguments; without CORRECTED they are not read.
// SRC: the element type of `llrs` -- float, or f16_llr / bf16_llr: then the two places that read an LLR, the loader
// and the soft form's second look at a NaN, widen it by widen_llr (llr_widen.hpp), and everything behind them is the same code on the
// same values.
template <int CODE, bool SOFT, bool CORRECTED = false, class SRC = float>
LDPC_DEV void decode_ms_layered_body(const SRC *__restrict__ llrs, float *__restrict__ app, uint8_t *__restrict__ output,
                                     uint32_t *__restrict__ iters_out, uint8_t *__restrict__ success_out, uint32_t batch,
                                     uint32_t maxiters, uint32_t *claim, char *lds, float scale = 1.0f, float offset = 0.0f)
{
    using GEO = LayeredGeometry<CODE>;
    using O = Ops<float>;
    constexpr Prototype P = GEO::P;
    constexpr int M = GEO::M, NT = GEO::NT, G = GEO::G, WG = GEO::WG, IPT = GEO::IPT, NB = GEO::NB, NROWS = GEO::NROWS,
                  NCOLS = GEO::NCOLS, NTX = GEO::NTX, N = GEO::N, NP = GEO::NP, OUT_LEN = GEO::OUT_LEN;

    const int tid = (int)threadIdx.x;
    const int g = tid / NT;                                  // codeword slot of this thread in the workgroup
    const int t = tid % NT;
    char *const cw = lds + g * GEO::CW_BYTES;
    float *const U = reinterpret_cast<float *>(cw + GEO::U_OFF);
    float *const LL = reinterpret_cast<float *>(cw + GEO::L_OFF);
    const uint32_t *const H = reinterpret_cast<const uint32_t *>(cw + GEO::H_OFF);
    int *const vote = reinterpret_cast<int *>(cw + GEO::F_OFF);
    int *const next_word = reinterpret_cast<int *>(lds + G * GEO::CW_BYTES);

    const uint32_t n_groups = (batch + G - 1) / G;
    // the launch's queue (decode_ms_launch.hpp, claim_counter) for workgroups of 8 waves and more: every decode draws once, so the draws
    // of a launch number exactly n_groups and the holder of the last ticket puts the head back to zero; a fixed stride otherwise
    const bool dyn = claim != nullptr;
    uint32_t grp = blockIdx.x;
    while (grp < n_groups) {
        const uint32_t frame = grp * G + g;
        const bool live = frame < batch;                     // (a partial last group: slots beyond the batch decode zeros, store nothing)
        const SRC *const L = llrs + (size_t)(live ? frame : 0) * N;
        if (dyn && tid == 0) *next_word = (int)(gridDim.x + __hip_atomic_fetch_add(claim, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (maxiters == 0) {
            // decoder.rs:374: nothing iterates -- output zero, iters 0, no success, every marginal zero
            if (live) {
                for (int x = t; x < OUT_LEN; x += NT) output[(size_t)frame * OUT_LEN + x] = 0;
                if constexpr (SOFT) for (int x = t; x < NP; x += NT) app[(size_t)frame * NP + x] = 0.0f;
                if (t == 0) { iters_out[frame] = 0; success_out[frame] = 0; }
            }
        } else {
            // ---- a codeword: u = v = 0 (decoder.rs:374), LLRs canonicalised into LDS
            float v[IPT][NB];
            static_for<0, IPT>([&](auto q_) LDPC_INLINE {
                constexpr int q = decltype(q_)::value;
                static_for<0, NB>([&](auto b_) LDPC_INLINE { v[q][decltype(b_)::value] = 0.0f; });
            });
            for (int x = t; x < NB * M; x += NT) U[x] = 0.0f;
            for (int x = t; x < N; x += NT) LL[x] = live ? O::load(widen_llr(L[x])) : 0.0f;
            if (t == 0) { vote[0] = 0; vote[1] = 0; }
            auto llr_at = [&](auto col_, int k) LDPC_INLINE -> float {
                constexpr int col = decltype(col_)::value;
                if constexpr (col >= NTX) return 0.0f;
                else return LL[col * M + k];
            };
            // marginal of variable (col, k): the LLR, then the u of the column's blocks in block order
            auto marginal = [&](auto col_, int k) LDPC_INLINE -> float {
                constexpr int col = decltype(col_)::value;
                float a = llr_at(col_, k);
                static_for<0, NB>([&](auto b_) LDPC_INLINE {
                    constexpr int b = decltype(b_)::value;
                    if constexpr (P.blk[b].col == col) a = O::add(a, U[b * M + k]);
                });
                return a;
            };
            layered_sync<WG>();

            bool done = !live;                               // this codeword's results are stored (per codeword slot)
            for (uint32_t it = 0; it < maxiters; ++it) {
                // ---- the layers
                static_for<0, NROWS>([&](auto r_) LDPC_INLINE {
                    constexpr int r = decltype(r_)::value;
                    constexpr int D = row_degree(P, r);
                    float nu[IPT][D];
                    // the thread index, opaque to the compiler once per layer: the layer's indices and LDS addresses are recomputed here
                    // (a few VALU operations) instead of being hoisted out of the sweep loop, where they would hold ~2 registers per edge
                    int tl = t;
                    asm volatile("" : "+v"(tl));
                    static_for<0, IPT>([&](auto q_) LDPC_INLINE {
                        constexpr int q = decltype(q_)::value;
                        const int i = tl + q * NT;
                        float vr[D], e[D];
                        int sgn = 0;
                        static_for<0, D>([&](auto j_) LDPC_INLINE {
                            constexpr int j = decltype(j_)::value, b = row_block(P, r, j), col = P.blk[b].col;
                            const int k = layered_map<CODE, b>(i);
                            const float va = marginal(IC<col>{}, k);
                            const float nv = O::sub(va, U[b * M + k]);
                            const float old = v[q][b];
                            const float nvv = ((nv < 0.0f) == (old < 0.0f) || old == 0.0f) ? nv : 0.0f;      // decoder.rs:421-426
                            v[q][b] = nvv;
                            vr[j] = nvv;
                            sgn ^= __float_as_int(nvv);
                        });
                        exclusive_min<O, D, true, true>(vr, e);
                        static_for<0, D>([&](auto j_) LDPC_INLINE {
                            constexpr int j = decltype(j_)::value;
                            // which of min1 / min2 the edge takes was decided on the uncorrected |v|; t is never -0.0 or NaN
                            if constexpr (CORRECTED) e[j] = __builtin_fmaxf(__fsub_rn(__fmul_rn(scale, e[j]), offset), 0.0f);
                            // sign product of the OTHER edges of the check: the whole product times this edge's own sign
                            nu[q][j] = __int_as_float(__float_as_int(e[j]) | ((sgn ^ __float_as_int(vr[j])) & (int)0x80000000));
                        });
                    });
                    layered_sync<WG>();                      // every marginal of the layer read before its u change
                    static_for<0, IPT>([&](auto q_) LDPC_INLINE {
                        constexpr int q = decltype(q_)::value;
                        const int i = tl + q * NT;
                        static_for<0, D>([&](auto j_) LDPC_INLINE {
                            constexpr int j = decltype(j_)::value, b = row_block(P, r, j);
                            U[b * M + layered_map<CODE, b>(i)] = nu[q][j];
                        });
                    });
                    if constexpr (r == 0) { if (t == 0) vote[(it + 1) & 1] = 0; }     // the next sweep's vote word (read two barriers ago)
                    layered_sync<WG>();
                });
                // ---- end of sweep: marginals, hard bits, parities (decoder.rs:436-453)
                float va[IPT][NCOLS];
                int tp = t;
                asm volatile("" : "+v"(tp));
                static_for<0, IPT>([&](auto q_) LDPC_INLINE {
                    constexpr int q = decltype(q_)::value;
                    const int k = tp + q * NT;
                    static_for<0, NCOLS>([&](auto c_) LDPC_INLINE {
                        constexpr int c = decltype(c_)::value;
                        va[q][c] = marginal(c_, k);
                        // lanes run along k: the ballot's bits [g * NT, g * NT + HW) are variables k .. k + HW - 1 of this codeword
                        const unsigned long long hb = __ballot(va[q][c] < 0.0f) >> ((tid & 63) & ~(GEO::HW - 1));
                        if ((k & (GEO::HW - 1)) == 0) {
                            char *const h = cw + GEO::H_OFF + (c * M + k) / 8;
                            if constexpr (GEO::HW == 64) *reinterpret_cast<unsigned long long *>(h) = hb;
                            else if constexpr (GEO::HW == 32) *reinterpret_cast<uint32_t *>(h) = (uint32_t)hb;
                            else *reinterpret_cast<uint16_t *>(h) = (uint16_t)hb;
                        }
                    });
                });
                layered_sync<WG>();
                int par = 0;
                static_for<0, IPT>([&](auto q_) LDPC_INLINE {
                    constexpr int q = decltype(q_)::value;
                    const int i = tp + q * NT;
                    static_for<0, NROWS>([&](auto r_) LDPC_INLINE {
                        constexpr int r = decltype(r_)::value;
                        int pr = 0;
                        static_for<0, row_degree(P, r)>([&](auto j_) LDPC_INLINE {
                            constexpr int b = row_block(P, r, decltype(j_)::value);
                            const int x = P.blk[b].col * M + layered_map<CODE, b>(i);
                            pr ^= (int)(H[x >> 5] >> (x & 31));
                        });
                        par |= pr & 1;
                    });
                });
                if (par) vote[it & 1] = 1;
                layered_sync<WG>();
                const bool ok = vote[it & 1] == 0;
                const bool last = it + 1 == maxiters;
                const bool fin = !done && (ok || last);
                // ---- a finished codeword's results: hard bits of va (MSB first, decoder.rs:457-459), iters, success, marginals
                if (__ballot(fin) != 0) {
                    const int lane = tid & 63;
                    static_for<0, IPT>([&](auto q_) LDPC_INLINE {
                        constexpr int q = decltype(q_)::value;
                        const int k = t + q * NT;
                        static_for<0, NCOLS>([&](auto c_) LDPC_INLINE {
                            constexpr int c = decltype(c_)::value;
                            const unsigned long long bits = __ballot(va[q][c] < 0.0f);          // bit l = lane l
                            if (fin && (k & 7) == 0)
                                output[(size_t)frame * OUT_LEN + (c * M + k) / 8] =
                                    (uint8_t)(__builtin_bitreverse32((unsigned)(bits >> lane) & 0xFFu) >> 24);
                            if constexpr (SOFT) {
                                if (fin) {
                                    float s = va[q][c] + 0.0f;                                  // (-0.0 -> +0.0)
                                    // only a NaN or +inf LLR makes a +inf marginal (every u is finite): look at the LLR again there
                                    if constexpr (c < NTX) {
                                        if (s == __builtin_inff()) { const float raw = widen_llr(L[c * M + k]); if (raw != raw) s = raw; }
                                    }
                                    app[(size_t)frame * NP + c * M + k] = s;
                                }
                            }
                        });
                    });
                    if (fin && t == 0) { iters_out[frame] = ok ? it : maxiters; success_out[frame] = ok ? 1 : 0; }
                }
                done = done || fin;
                if (__ballot(!done) == 0) break;
            }
        }
        // next group: the queue's ticket (drawn at the start of this one) or the fixed stride
        if (dyn) grp = (uint32_t)__builtin_amdgcn_readfirstlane(*next_word);
        else grp += gridDim.x;
        if (dyn && tid == 0 && grp - gridDim.x == n_groups - 1) __hip_atomic_store(claim, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        layered_sync<WG>();                                  // every read of this codeword's LDS done before the next one's set-up
    }
}

template <int CODE, bool SOFT>
__global__ void __launch_bounds__(LayeredGeometry<CODE>::WG)
decode_ms_layered_kernel(const float *__restrict__ llrs, float *__restrict__ app, uint8_t *__restrict__ output,
                         uint32_t *__restrict__ iters_out, uint8_t *__restrict__ success_out, uint32_t batch, uint32_t maxiters,
                         uint32_t *claim)
{
    __shared__ __attribute__((aligned(16))) char lds[LayeredGeometry<CODE>::LDS_BYTES];
    decode_ms_layered_body<CODE, SOFT>(llrs, app, output, iters_out, success_out, batch, maxiters, claim, lds);
}

// The same body with the correction step, under a name of its own (decode_ms_corrected_f32.hip): the plain kernels above keep
// their symbols, their arguments and their instructions.
template <int CODE, bool SOFT>
__global__ void __launch_bounds__(LayeredGeometry<CODE>::WG)
decode_ms_corrected_kernel(const float *__restrict__ llrs, float *__restrict__ app, uint8_t *__restrict__ output,
                           uint32_t *__restrict__ iters_out, uint8_t *__restrict__ success_out, uint32_t batch, uint32_t maxiters,
                           uint32_t *claim, float scale, float offset)
{
    __shared__ __attribute__((aligned(16))) char lds[LayeredGeometry<CODE>::LDS_BYTES];
    decode_ms_layered_body<CODE, SOFT, true>(llrs, app, output, iters_out, success_out, batch, maxiters, claim, lds, scale, offset);
}

}  // namespace ldpc
