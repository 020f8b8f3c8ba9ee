"""TM8192 f32 through the default dispatch -- the pair kernel, whose hard-output f32 instantiations keep their LDS addresses in
registers across the iterations and the codewords (csrc/decode_ms_pair.hpp, HOIST) -- against the CPU oracle, bit for bit: hard
bits, iteration counts, success flags.

What an address formed earlier can get wrong shows only when a workgroup goes on to another codeword, so the large batch has 520
frames: more than twice the 256 workgroups an MI355X holds of this kernel, every persistent workgroup decodes at least two of them
and the launch's queue hands the later ones out.  The batch interleaves ordinary 2 dB frames with frames that fail the LLR range
vote (one LLR of 3e38, of inf, of NaN) and one all-zero frame, so that a workgroup alternates between the clamped and the
clamp-free copy of the loop from codeword to codeword.  max_iters 0, 1 and 2 end inside or right behind the peeled first pass; 25
runs the v_fma form of the self-correction (form 2) and 29 is the first count at which the launcher takes the v_mul_legacy form
(form 3: nocap_limit_for(29, true) = 2^1 < 8, csrc/decode_ms_launch.hpp).

The hoist is gated on the message type and the output form, so the TM2048 f32 pair kernels (`variant` 32) have it too: one batch of
theirs, 4200 frames of the same mixture (its workgroups are a quarter of TM8192's size; more than twice the at most 2048 that can be
resident), at 25 and 29 iterations."""
import numpy as np
import pytest

import oracle
from labrador_ldpc_amd import LDPCCode

pytestmark = pytest.mark.gpu

CODE = LDPCCode.TM8192
MAXITERS = (0, 1, 2, 25, 29)
ORDINARY = 12
FRAMES = 520                                     # > 2 x 256 resident workgroups


def _pool(code, seed, frames, maxiters):
    """The distinct frames, their oracle results per max_iters (computed once, never modified), and `frames` pool indices."""
    rng = np.random.default_rng(seed)
    n = code.n()
    llrs, _ = oracle.awgn_llrs(code, rng, ORDINARY + 4, 2.0, np.float32)
    big, inf, nan, zero = ORDINARY, ORDINARY + 1, ORDINARY + 2, ORDINARY + 3
    llrs[big, int(rng.integers(0, n))] = np.float32(3e38)
    llrs[inf, int(rng.integers(0, n))] = np.float32(np.inf)
    llrs[nan, int(rng.integers(0, n))] = np.float32(np.nan)
    llrs[zero, :] = 0.0
    llrs.setflags(write=False)
    # ordinary, out of range, ordinary, out of range, ...: the kind changes with every frame; the all-zero frame once
    idx = np.empty(frames, dtype=np.int64)
    idx[0::2] = rng.integers(0, ORDINARY, len(idx[0::2]))
    idx[1::2] = np.resize(np.array([big, inf, nan]), len(idx[1::2]))
    idx[259] = zero
    ref = {m: oracle.decode_ms_batch(code, llrs, m)[:3] for m in maxiters}
    return llrs, idx, ref


@pytest.fixture(scope="module")
def pool():
    return _pool(CODE, 0x8192ADD5, FRAMES, MAXITERS)


def _compare(code, pool, batch, maxiters, variant=0):
    llrs, idx, ref = pool
    i = idx[:batch]
    out_g, it_g, ok_g = code.decode_ms_batch(np.ascontiguousarray(llrs[i]), maxiters, variant=variant)
    out_c, it_c, ok_c = (a[i] for a in ref[maxiters])
    bad = np.nonzero((it_g != it_c) | (ok_g != ok_c) | (out_g != out_c).any(axis=1))[0]
    assert bad.size == 0, (f"{code.name} max_iters {maxiters}, batch {batch}: {bad.size} frames differ, first {bad[0]} (pool entry {i[bad[0]]}): "
                           f"gpu(it={it_g[bad[0]]}, ok={ok_g[bad[0]]}) cpu(it={it_c[bad[0]]}, ok={ok_c[bad[0]]})")


@pytest.mark.parametrize("maxiters", MAXITERS)
@pytest.mark.parametrize("batch", (1, 3, FRAMES))
def test_tm8192_f32_default_dispatch_matches_the_oracle(pool, batch, maxiters):
    _compare(CODE, pool, batch, maxiters)


@pytest.mark.parametrize("maxiters", (25, 29))
def test_tm2048_f32_pair_variant_matches_the_oracle(maxiters):
    _compare(LDPCCode.TM2048, _pool(LDPCCode.TM2048, 0x2048ADD5 + maxiters, 4200, (maxiters,)), 4200, maxiters, variant=32)


def test_the_batch_exercises_both_copies_of_the_loop_and_both_outcomes(pool):
    """What the comparison above rests on: at 25 iterations the ordinary frames mostly converge after several passes (the loop ran),
    and the pool holds frames of every kind."""
    llrs, idx, ref = pool
    _, it, ok = ref[25]
    assert ok[:ORDINARY].sum() >= ORDINARY // 2 and (it[:ORDINARY][ok[:ORDINARY] != 0] >= 3).all()
    assert set(idx.tolist()) >= set(range(ORDINARY, ORDINARY + 4))
