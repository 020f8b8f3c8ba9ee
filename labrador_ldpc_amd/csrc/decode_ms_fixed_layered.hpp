// decode_ms_fixed_layered.hpp -- block-row layered min-sum decoding of i8 and i16 LLR batches for gfx950 (MI355X).
//
// The schedule of decode_ms_layered.hpp in fixed point, with a contract of its own.  T_MAX = 127 / 32767, per sweep:
//
//     for every layer r in ascending order:
//         va[j] = llr[j] (0 for punctured j) + the u of j's edges, exact in i32          (llr: the input with T's minimum as -T_MAX)
//         for every edge e = (c, j) of layer r:  nv = clamp(va[j] - u[e], -T_MAX, T_MAX);  v[e] = self-corrected nv
//         u[e] = exclusive minimum of the other |v| of its check, with their sign product
//     va = llr + sum of u; the sweep succeeds when every check's parity over hard(va) is 0
//
// Every sum is an exact integer sum, so the order in which a marginal is formed cannot matter, and the kernel is free to keep it:
//
//   * one MARGINAL per variable in LDS (i32 [n + p] per codeword, initialised to the LLRs).  An edge reads its variable's marginal
//     once and applies u_new - u_old to it.  Where the layer's cell holds one block, the variable has exactly one edge in the layer:
//     the owning thread reads, computes and writes, with no hand-off.  Where a cell holds two or three terms, every edge has to see
//     the layer-start marginal: those deltas wait for a barrier and land by an LDS integer add (exact in any order).
//   * no u array, no v array and no LLR copy.  A thread owns check index i (and i + NT, ...) of every block row, and holds each
//     check COMPRESSED in registers: min1, min2, the position of the first minimum, the sign bit of every v and a "v is zero" bit
//     of every v.  u_old of edge j is rebuilt from that: (pos == j ? min2 : min1), negative when the parity of the signs differs
//     from v's own sign (a tie is harmless: then min2 == min1).  The self-correction needs only v's old sign and its zero bit.
//     Three registers per check instead of one per edge, and TM8192's 120 KB of u become 40 KB of marginals.
//   * the end of a sweep needs no hard-bit array: a check's parity is the sign bit of the XOR of its variables' marginals, read
//     straight from LDS (one read per edge, where the f32 kernel read the column sums, wrote bits, synchronised and read bits).
//     Hard bits are formed once, by a ballot per wave, when a codeword's results are stored.
//
// The marginals stay i32 for i8 LLRs too (7 * 127 would fit i16): the deltas of the two- and three-term cells land by ds_add_u32,
// and there is no 16-bit LDS add -- a packed add would carry from one marginal into its neighbour.
//
// Kept from the f32 layered kernel: the geometry (NT = M / IPT threads per codeword, G codewords per 64-thread workgroup for the
// small codes), one-wave codewords synchronised by an lgkmcnt wait, the launch queue for workgroups of eight waves and more, the
// partial last group, max_iters = 0, and the vote word per sweep.
#pragma once

#include "decode_ms_layered.hpp"
#include "llr_quantise.hpp"              // quantise_llr: the rule of the f32-source loader

namespace ldpc {

// how many blocks of block row `row` lie in block column `col` (the terms of that cell of the prototype)
constexpr int cell_terms(const Prototype &p, int row, int col)
{
    int c = 0;
    for (int b = 0; b < p.n_blocks; ++b) c += (p.blk[b].row == row && p.blk[b].col == col) ? 1 : 0;
    return c;
}
// the number of edges of a check of block row `row` that lie in cells of more than one term
constexpr int row_shared_edges(const Prototype &p, int row)
{
    int c = 0;
    for (int b = 0; b < p.n_blocks; ++b) c += (p.blk[b].row == row && cell_terms(p, row, p.blk[b].col) > 1) ? 1 : 0;
    return c;
}

// the position of edge `j` of block row `row` among the row's edges in cells of more than one term
constexpr int shared_edge_index(const Prototype &p, int row, int j)
{
    int c = 0;
    for (int jj = 0; jj < j; ++jj) c += cell_terms(p, row, p.blk[row_block(p, row, jj)].col) > 1 ? 1 : 0;
    return c;
}

template <int CODE>
struct LayeredFixedGeometry {
    using F32 = LayeredGeometry<CODE>;
    static constexpr Prototype P = F32::P;
    static constexpr int IPT = F32::IPT, M = F32::M, N = F32::N, NP = F32::NP, NT = F32::NT, G = F32::G, WG = F32::WG, NB = F32::NB,
                         NROWS = F32::NROWS, NCOLS = F32::NCOLS, NTX = F32::NTX, OUT_LEN = F32::OUT_LEN;
    // per codeword: marginals [NCOLS * M] i32 | two vote words
    static constexpr int A_OFF = 0;
    static constexpr int F_OFF = NCOLS * M * 4;
    static constexpr int CW_BYTES = (F_OFF + 8 + 15) / 16 * 16;
    static constexpr size_t LDS_BYTES = (size_t)G * CW_BYTES + 16;
    static_assert(NP == NCOLS * M && NP % NT == 0 && N % NT == 0, "one marginal per variable, whole rounds of the codeword's threads");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

// bit `j` of `w` as 0 or -1
template <int J>
LDPC_DEV int bit_mask(uint32_t w)
{
    return (int)(w << (31 - J)) >> 31;
}

// CORRECTED: normalized / offset min-sum in integers -- every message magnitude m becomes
//     max(((scale_num * m + ((1 << scale_shift) >> 1)) >> scale_shift) - offset, 0)              (round half up, then the offset)
// with 0 <= scale_shift <= 8, 1 <= scale_num <= 1 << scale_shift and 0 <= offset <= T_MAX, checked by capi.hip: the product is at
// most 256 * 32767 + 128 and the result at most m.  A check is held as its two minima, so the step is taken ONCE PER CHECK, on min1
// and min2 as they go into the registers -- the minima themselves were taken on the uncorrected |v| -- and every message of the check
// is built from the corrected pair, now (u_new) and on the next visit (u_old); equal minima correct to equal values, so a tie stays
// harmless.  The three parameters are wave-uniform kernel arguments; without CORRECTED they are not read.
//
// SRC: the element type of `llrs` -- T itself, or float: then the loader, the one place that reads an LLR, quantises
// it to T by quantise_llr (llr_quantise.hpp) with the wave-uniform (scale, flim), and everything behind the loader is the same code
// on the same values.  With SRC = T the two are not read.
template <int CODE, class T, bool SOFT, bool CORRECTED = false, class SRC = T>
LDPC_DEV void decode_ms_layered_fixed_body(const SRC *__restrict__ llrs, int32_t *__restrict__ app, uint8_t *__restrict__ output,
                                           uint32_t *__restrict__ iters_out, uint8_t *__restrict__ success_out, uint32_t batch,
                                           uint32_t maxiters, uint32_t *claim, char *lds, uint32_t scale_num = 1, uint32_t scale_shift = 0,
                                           uint32_t offset = 0, float scale = 0.0f, float flim = 0.0f)
{
    using GEO = LayeredFixedGeometry<CODE>;
    constexpr Prototype P = GEO::P;
    constexpr int M = GEO::M, NT = GEO::NT, G = GEO::G, WG = GEO::WG, IPT = GEO::IPT, NROWS = GEO::NROWS, NCOLS = GEO::NCOLS, N = GEO::N,
                  NP = GEO::NP, OUT_LEN = GEO::OUT_LEN;
    constexpr int TMAX = sizeof(T) == 1 ? 127 : 32767;
    static_assert(std::is_same_v<T, int8_t> || std::is_same_v<T, int16_t>, "i8 or i16 LLRs");
    static_assert(std::is_same_v<SRC, T> || std::is_same_v<SRC, float>, "LLRs of T, or f32 LLRs quantised to T by the loader");

    const int tid = (int)threadIdx.x;
    const int g = tid / NT;                                  // codeword slot of this thread in the workgroup
    const int t = tid % NT;
    char *const cw = lds + g * GEO::CW_BYTES;
    int *const A = reinterpret_cast<int *>(cw + GEO::A_OFF);
    int *const vote = reinterpret_cast<int *>(cw + GEO::F_OFF);
    int *const next_word = reinterpret_cast<int *>(lds + G * GEO::CW_BYTES);

    const uint32_t n_groups = (batch + G - 1) / G;
    // the launch's queue (decode_ms_launch.hpp, claim_counter) or a fixed stride, as in decode_ms_layered_body
    const bool dyn = claim != nullptr;
    uint32_t grp = blockIdx.x;
    while (grp < n_groups) {
        const uint32_t frame = grp * G + g;
        const bool live = frame < batch;                     // (a partial last group: slots beyond the batch decode zeros, store nothing)
        const SRC *const L = llrs + (size_t)(live ? frame : 0) * N;
        if (dyn && tid == 0) *next_word = (int)(gridDim.x + __hip_atomic_fetch_add(claim, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (maxiters == 0) {
            // nothing iterates: output zero, iters 0, no success, every marginal zero
            if (live) {
                // (wave-uniform trip counts: NT divides NP)
                for (int x0 = 0; x0 < OUT_LEN; x0 += NT) { if (x0 + t < OUT_LEN) output[(size_t)frame * OUT_LEN + x0 + t] = 0; }
                if constexpr (SOFT) for (int x0 = 0; x0 < NP; x0 += NT) app[(size_t)frame * NP + x0 + t] = 0;
                if (t == 0) { iters_out[frame] = 0; success_out[frame] = 0; }
            }
        } else {
            // ---- a codeword: u = v = 0, so every check is (min1 = min2 = 0, no sign, every v zero) and a marginal is its LLR
            // mn: min1 | min2 << 16.  sg: the sign bits of the check's v (bit j: edge j of the row), the first minimum's position in
            // bits 27 .. 31.  zr: bit j = v of edge j is zero.
            uint32_t mn[IPT][NROWS], sg[IPT][NROWS], zr[IPT][NROWS];
            static_for<0, IPT>([&](auto q_) LDPC_INLINE {
                constexpr int q = decltype(q_)::value;
                static_for<0, NROWS>([&](auto r_) LDPC_INLINE {
                    constexpr int r = decltype(r_)::value;
                    mn[q][r] = 0;
                    sg[q][r] = 0;
                    zr[q][r] = (1u << row_degree(P, r)) - 1u;
                });
            });
            // A float row's rounds lie further apart than a load's immediate offset reaches, so each round has an offset of its own.
            // The thread index is made opaque here, as it is once per layer below: the offsets are formed per codeword, next to their
            // loads, instead of being held in registers (or in scratch) across the whole kernel.
            int tq = t;
            if constexpr (std::is_same_v<SRC, float>) asm volatile("" : "+v"(tq));
            for (int x0 = 0; x0 < NP; x0 += NT) {            // (a wave-uniform trip count: NT divides NP and N)
                int l = 0;
                // (a slot beyond the batch reads frame 0 and drops it: no divergent branch)
                if constexpr (std::is_same_v<SRC, float>) { if (x0 < N) l = (int)quantise_llr<T>(L[x0 + tq], scale, flim); }
                else { if (x0 < N) l = (int)L[x0 + t]; }
                l = live ? l : 0;
                A[x0 + t] = l < -TMAX ? -TMAX : l;           // (only T's minimum changes)
            }
            if (t == 0) { vote[0] = 0; vote[1] = 0; }
            layered_sync<WG>();

            bool done = !live;                               // this codeword's results are stored (per codeword slot)
            for (uint32_t it = 0; it < maxiters; ++it) {
                // ---- the layers
                static_for<0, NROWS>([&](auto r_) LDPC_INLINE {
                    constexpr int r = decltype(r_)::value;
                    constexpr int D = row_degree(P, r);
                    constexpr int DS = row_shared_edges(P, r);            // edges in cells of two or three terms
                    static_assert(D >= 2 && D <= 27, "the sign bits and the position share a word");
                    constexpr uint32_t DMASK = (1u << D) - 1u;
                    int sh_x[IPT][DS > 0 ? DS : 1], sh_d[IPT][DS > 0 ? DS : 1];
                    // the thread index, opaque to the compiler once per layer (decode_ms_layered_body: addresses are recomputed per
                    // layer instead of being held across the sweep loop)
                    int tl = t;
                    asm volatile("" : "+v"(tl));
                    static_for<0, IPT>([&](auto q_) LDPC_INLINE {
                        constexpr int q = decltype(q_)::value;
                        const int i = tl + q * NT;
                        const uint32_t o_sg = sg[q][r], o_zr = zr[q][r];
                        const int o_m1 = (int)(mn[q][r] & 0xFFFFu), o_m2 = (int)(mn[q][r] >> 16), o_pos = (int)(o_sg >> 27);
                        // bit j: the old u of edge j is negative -- the sign product of the OTHER edges times v's own sign
                        const uint32_t o_neg = o_sg ^ (0u - (uint32_t)(__builtin_popcount(o_sg & DMASK) & 1));
                        int x[D], m[D], uo[D], nv[D];
                        uint32_t k1 = ((uint32_t)TMAX << 5) | 31u, k2 = k1, n_sg = 0, n_zr = 0, r_sg = 0;
                        static_for<0, D>([&](auto j_) LDPC_INLINE {
                            constexpr int j = decltype(j_)::value, b = row_block(P, r, j), col = P.blk[b].col;
                            x[j] = col * M + layered_map<CODE, b>(i);
                            m[j] = A[x[j]];                  // the layer-start marginal
                            const int mag = o_pos == j ? o_m2 : o_m1;
                            const int s = bit_mask<j>(o_neg);
                            uo[j] = (mag ^ s) - s;
                            const int w = m[j] - uo[j];
                            nv[j] = w < -TMAX ? -TMAX : (w > TMAX ? TMAX : w);
                            r_sg |= ((uint32_t)nv[j] >> 31) << j;
                        });
                        // self-correction, for the whole check at once: nv is dropped where its side differs from the old v's and
                        // the old v was not zero
                        const uint32_t drop = (r_sg ^ o_sg) & ~o_zr;
                        static_for<0, D>([&](auto j_) LDPC_INLINE {
                            constexpr int j = decltype(j_)::value;
                            const int v = nv[j] & ~bit_mask<j>(drop);
                            const uint32_t a = (uint32_t)(v < 0 ? -v : v);
                            // minima as keys |v| << 5 | j: the smallest key holds min1 and a position of it, the second smallest min2
                            const uint32_t key = (a << 5) | (uint32_t)j;
                            const uint32_t hi = k1 > key ? k1 : key;
                            k2 = k2 < hi ? k2 : hi;
                            k1 = k1 < key ? k1 : key;
                            n_zr |= (a < 1u ? 1u : 0u) << j;
                        });
                        n_sg = r_sg & ~drop & DMASK;
                        int n_m1 = (int)(k1 >> 5), n_m2 = (int)(k2 >> 5);
                        const int n_pos = (int)(k1 & 31u);
                        if constexpr (CORRECTED) {
                            // (a multiply, an add, a shift, a subtract and a max, twice per check)
                            const uint32_t half = (1u << scale_shift) >> 1;
                            const int t1 = (int)((scale_num * (uint32_t)n_m1 + half) >> scale_shift) - (int)offset;
                            const int t2 = (int)((scale_num * (uint32_t)n_m2 + half) >> scale_shift) - (int)offset;
                            n_m1 = t1 > 0 ? t1 : 0;
                            n_m2 = t2 > 0 ? t2 : 0;
                        }
                        const uint32_t n_neg = n_sg ^ (0u - (uint32_t)(__builtin_popcount(n_sg) & 1));
                        mn[q][r] = (uint32_t)n_m1 | ((uint32_t)n_m2 << 16);
                        sg[q][r] = n_sg | ((uint32_t)n_pos << 27);
                        zr[q][r] = n_zr;
                        static_for<0, D>([&](auto j_) LDPC_INLINE {
                            constexpr int j = decltype(j_)::value, b = row_block(P, r, j), col = P.blk[b].col;
                            const int mag = n_pos == j ? n_m2 : n_m1;
                            const int s = bit_mask<j>(n_neg);
                            const int delta = ((mag ^ s) - s) - uo[j];
                            if constexpr (cell_terms(P, r, col) == 1) {
                                A[x[j]] = m[j] + delta;      // the only edge of this variable in the layer
                            } else {
                                constexpr int js = shared_edge_index(P, r, j);
                                sh_x[q][js] = x[j];
                                sh_d[q][js] = delta;
                            }
                        });
                    });
                    if constexpr (DS > 0) {
                        layered_sync<WG>();                  // every marginal of the layer's shared cells read before a delta lands
                        static_for<0, IPT>([&](auto q_) LDPC_INLINE {
                            constexpr int q = decltype(q_)::value;
                            static_for<0, DS>([&](auto s_) LDPC_INLINE {
                                constexpr int s = decltype(s_)::value;
                                (void)__hip_atomic_fetch_add(&A[sh_x[q][s]], sh_d[q][s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            });
                        });
                    }
                    layered_sync<WG>();
                    if constexpr (r == 0) { if (t == 0) vote[(it + 1) & 1] = 0; }     // the next sweep's vote word (last read a barrier ago)
                });
                // ---- end of sweep: a check's parity is the sign of the XOR of its variables' marginals
                int tp = t;
                asm volatile("" : "+v"(tp));
                int par = 0;
                static_for<0, IPT>([&](auto q_) LDPC_INLINE {
                    constexpr int q = decltype(q_)::value;
                    const int i = tp + q * NT;
                    static_for<0, NROWS>([&](auto r_) LDPC_INLINE {
                        constexpr int r = decltype(r_)::value;
                        int pr = 0;
                        static_for<0, row_degree(P, r)>([&](auto j_) LDPC_INLINE {
                            constexpr int b = row_block(P, r, decltype(j_)::value);
                            pr ^= A[P.blk[b].col * M + layered_map<CODE, b>(i)];
                        });
                        par |= pr;
                    });
                });
                if (par < 0) vote[it & 1] = 1;
                layered_sync<WG>();
                const bool ok = vote[it & 1] == 0;
                const bool last = it + 1 == maxiters;
                const bool fin = !done && (ok || last);
                // ---- a finished codeword's results: hard bits of the marginals (MSB first), iters, success, marginals
                if (__ballot(fin) != 0) {
                    const int lane = tid & 63;
                    int va[IPT][NCOLS];
                    static_for<0, IPT>([&](auto q_) LDPC_INLINE {
                        constexpr int q = decltype(q_)::value;
                        const int k = t + q * NT;
                        static_for<0, NCOLS>([&](auto c_) LDPC_INLINE {
                            constexpr int c = decltype(c_)::value;
                            va[q][c] = A[c * M + k];
                            const unsigned long long bits = __ballot(va[q][c] < 0);             // bit l = lane l
                            if (fin && (k & 7) == 0)
                                output[(size_t)frame * OUT_LEN + (c * M + k) / 8] =
                                    (uint8_t)(__builtin_bitreverse32((unsigned)(bits >> lane) & 0xFFu) >> 24);
                        });
                    });
                    if constexpr (SOFT) {
                        if (fin) {
                            static_for<0, IPT>([&](auto q_) LDPC_INLINE {
                                constexpr int q = decltype(q_)::value;
                                static_for<0, NCOLS>([&](auto c_) LDPC_INLINE {
                                    constexpr int c = decltype(c_)::value;
                                    app[(size_t)frame * NP + c * M + t + q * NT] = va[q][c];
                                });
                            });
                        }
                    }
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

template <int CODE, class T, bool SOFT>
__global__ void __launch_bounds__(LayeredFixedGeometry<CODE>::WG)
decode_ms_layered_fixed_kernel(const T *__restrict__ llrs, int32_t *__restrict__ app, uint8_t *__restrict__ output,
                               uint32_t *__restrict__ iters_out, uint8_t *__restrict__ success_out, uint32_t batch, uint32_t maxiters,
                               uint32_t *claim)
{
    __shared__ __attribute__((aligned(16))) char lds[LayeredFixedGeometry<CODE>::LDS_BYTES];
    decode_ms_layered_fixed_body<CODE, T, SOFT>(llrs, app, output, iters_out, success_out, batch, maxiters, claim, lds);
}

// The same body with the correction step, as kernels of their own (decode_ms_fixed_corrected.hip): the plain kernels above keep
// their symbols, their arguments and their instructions.
template <int CODE, class T, bool SOFT>
__global__ void __launch_bounds__(LayeredFixedGeometry<CODE>::WG)
decode_ms_layered_fixed_corrected_kernel(const T *__restrict__ llrs, int32_t *__restrict__ app, uint8_t *__restrict__ output,
                                         uint32_t *__restrict__ iters_out, uint8_t *__restrict__ success_out, uint32_t batch,
                                         uint32_t maxiters, uint32_t *claim, uint32_t scale_num, uint32_t scale_shift, uint32_t offset)
{
    __shared__ __attribute__((aligned(16))) char lds[LayeredFixedGeometry<CODE>::LDS_BYTES];
    decode_ms_layered_fixed_body<CODE, T, SOFT, true>(llrs, app, output, iters_out, success_out, batch, maxiters, claim, lds, scale_num,
                                                      scale_shift, offset);
}

}  // namespace ldpc
