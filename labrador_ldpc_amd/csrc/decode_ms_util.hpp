// decode_ms_util.hpp -- what every decoder kernel of this library shares and none of them tunes: the inlining and barrier
// macros, the compile-time loop, the analysis of a code's prototype matrix, and the pi_k index map.  Depends on codes.hpp only.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "codes.hpp"

#define LDPC_INLINE __attribute__((always_inline))
// Workgroup barrier for LDS hand-offs.  Written out (instead of __syncthreads()) so that it waits
// for LDS operations only and not for the LLR loads in flight, which are counted in vmcnt.
#define LDPC_SYNC() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#define LDPC_DEV __device__ __forceinline__

namespace ldpc {

// ---- compile-time loop ------------------------------------------------------------------
template <int N> struct IC { static constexpr int value = N; constexpr operator int() const { return N; } };
template <int B, int E, class F>
LDPC_DEV void static_for(F &&f)
{
    if constexpr (B < E) { f(IC<B>{}); static_for<B + 1, E>(f); }
}

// XOR of D words with three-input XORs (v_bitop3_b32 issues at the fast VALU rate on gfx950)
template <int D>
LDPC_DEV int xor_reduce(const int (&w)[D])
{
    int acc = w[0];
    static_for<0, (D - 1) / 2>([&](auto I_) LDPC_INLINE {
        constexpr int i = 1 + 2 * decltype(I_)::value;
        acc = __builtin_amdgcn_bitop3_b32(acc, w[i], w[i + 1], 0x96);
    });
    if constexpr (D % 2 == 0) acc ^= w[D - 1];
    return acc;
}

// acc ^ w[0] ^ ... ^ w[N - 1], two words per v_bitop3_b32 (a running `acc ^= w` costs one v_xor per word)
template <int N, int D>
LDPC_DEV int xor_into(int acc, const int (&w)[D])
{
    static_assert(N <= D);
    static_for<0, N / 2>([&](auto I_) LDPC_INLINE {
        constexpr int i = 2 * decltype(I_)::value;
        acc = __builtin_amdgcn_bitop3_b32(acc, w[i], w[i + 1], 0x96);
    });
    if constexpr (N % 2 == 1) acc ^= w[N - 1];
    return acc;
}

// ---- prototype analysis -------------------------------------------------------------------
constexpr bool blk_local(const Block &b) { return b.kind == BLK_I && b.val == 0; }
constexpr int count_exchanged(const Prototype &p)
{
    int c = 0;
    for (int b = 0; b < p.n_blocks; ++b) c += blk_local(p.blk[b]) ? 0 : 1;
    return c;
}
// slot of block b among the exchanged (non-local) blocks, -1 if local
constexpr int exch_slot(const Prototype &p, int b)
{
    if (blk_local(p.blk[b])) return -1;
    int c = 0;
    for (int i = 0; i < b; ++i) c += blk_local(p.blk[i]) ? 0 : 1;
    return c;
}
constexpr bool col_exchanged(const Prototype &p, int col)
{
    for (int b = 0; b < p.n_blocks; ++b)
        if (p.blk[b].col == col && !blk_local(p.blk[b])) return true;
    return false;
}
constexpr int count_exch_cols(const Prototype &p)
{
    int c = 0;
    for (int col = 0; col < p.n_cols; ++col) c += col_exchanged(p, col) ? 1 : 0;
    return c;
}
// slot of block column `col` among the columns whose marginals are exchanged, -1 if none
constexpr int col_slot(const Prototype &p, int col)
{
    if (!col_exchanged(p, col)) return -1;
    int c = 0;
    for (int i = 0; i < col; ++i) c += col_exchanged(p, i) ? 1 : 0;
    return c;
}
constexpr int row_degree(const Prototype &p, int row)
{
    int c = 0;
    for (int b = 0; b < p.n_blocks; ++b) c += p.blk[b].row == row ? 1 : 0;
    return c;
}
// block index of the j-th block of block row `row`
constexpr int row_block(const Prototype &p, int row, int j)
{
    for (int b = 0; b < p.n_blocks; ++b)
        if (p.blk[b].row == row && j-- == 0) return b;
    return -1;
}

// rank of local edge (S, B) among a thread's local edges, index-major
constexpr int local_edge_rank(const Prototype &p, int S, int B)
{
    int nloc = 0, r = 0;
    for (int b = 0; b < p.n_blocks; ++b)
        if (blk_local(p.blk[b])) { if (b < B) ++r; ++nloc; }
    return S * nloc + r;
}

// pi_k(i) for check index i whose quarter j = i / (M/4) the caller supplies: a literal when a
// thread's indices never leave a quarter, a wave-uniform scalar when waves do not straddle
// quarters (then the selects below are scalar), a per-lane value otherwise.
template <int K, int M>
LDPC_DEV int pi_dev(int i, int j)
{
    constexpr int LQ = ilog2(M / 4), Q = M / 4;
    constexpr int P0 = phi_of(K, 0, M), P1 = phi_of(K, 1, M), P2 = phi_of(K, 2, M), P3 = phi_of(K, 3, M);
    constexpr int TH = theta_of(K);
    int phi;
    if constexpr (Q <= 256) {
        // the four rotations of a block (each < Q <= 256) packed into one literal and picked by a bit-field
        // extract: one VALU operation.  Written as a chain of selects on the per-lane quarter the compiler
        // emitted EXEC-masked branches, one pair per quarter and edge (119 of them in the TM1280 kernel).
        constexpr unsigned PACK = (unsigned)P0 | ((unsigned)P1 << 8) | ((unsigned)P2 << 16) | ((unsigned)P3 << 24);
        phi = (int)__builtin_amdgcn_ubfe(PACK, (unsigned)j * 8u, 8u);
    } else {
        // rotations up to 16 bits: two literals, one select on bit 1 of the quarter, one bit-field extract
        constexpr unsigned LO = (unsigned)P0 | ((unsigned)P1 << 16), HI = (unsigned)P2 | ((unsigned)P3 << 16);
        const unsigned w = (j & 2) ? HI : LO;
        phi = (int)__builtin_amdgcn_ubfe(w, ((unsigned)j & 1u) * 16u, 16u);
    }
    return (((TH + j) & 3) << LQ) + ((phi + i) & (Q - 1));
}

}  // namespace ldpc
