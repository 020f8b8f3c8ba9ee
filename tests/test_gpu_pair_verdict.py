"""TM8192 f32 through the default dispatch -- the pair kernel, whose hard-output f32 instantiations request the variable phase's
exchanged u before they have the previous pass's verdict (csrc/decode_ms_pair.hpp, EARLY) -- against the CPU oracle, bit for bit:
hard bits, iteration counts, success flags.

What the change can get wrong sits at the loop head, so the pool of distinct frames holds every way the head can go (iteration
counts of the oracle, asserted by the last test of this file from the oracle's results alone):

  * the all-zero frame: success with iters 0, the first trip through the head;
  * frames at 40 dB: iters 1, the second trip;
  * frames at 12 dB: iters 1 and 2; at 7 dB: 3-4; at 4 dB: 7-8; at 2 dB: 15-19 at a cap of 25;
  * frames at -1 dB: they never converge, so the loop ends on the cap, at caps 1, 2, 3 and 25;
  * one frame each with an LLR of 3e38, of inf and of NaN: they fail the LLR range vote and run the clamped copy of the loop.

The caps are 1, 2, 3, 25 and 29 (from 29 on the launcher takes the v_mul_legacy form of the self-correction, form 3), and for two
of the 2 dB frames k and k + 1, k being the frame's own iteration count at cap 25: the oracle fails it with iters = k at cap k and
passes it with iters = k at cap k + 1, where the verdict and the cap are met at the same head.  Both outcomes of the oracle are
asserted before the comparison.

An exit with reads outstanding shows only when the workgroup goes on to another codeword, so the large batch has 520 frames -- more
than twice the 256 workgroups an MI355X holds of this kernel -- with the kinds interleaved: a persistent workgroup goes from every kind
of exit into a codeword of another kind.  The gate is on the message type and the output form, so the TM2048 f32 pair kernels
(`variant` 32) have the change too: one batch of theirs, 4200 frames of the same mixture, at caps 25 and 29."""
import numpy as np
import pytest

import oracle
from labrador_ldpc_amd import LDPCCode

pytestmark = pytest.mark.gpu

CODE = LDPCCode.TM8192
CAPS = (1, 2, 3, 25, 29)
FRAMES = 520                                     # > 2 x 256 resident workgroups
# (kind, Eb/N0 in dB, frames); the order of the kinds is the order in which a batch interleaves them
KINDS = (("2dB", 2.0, 8), ("-1dB", -1.0, 2), ("zero", None, 1), ("40dB", 40.0, 2), ("clamped", 2.0, 3), ("12dB", 12.0, 6),
         ("7dB", 7.0, 4), ("4dB", 4.0, 4))


def _pool(code, seed, frames, caps):
    """The distinct frames, {kind: their pool indices}, their oracle results per cap (computed once, never modified) and `frames`
    pool indices that go through the kinds in turn."""
    rng = np.random.default_rng(seed)
    n = code.n()
    parts, where, at = [], {}, 0
    for kind, db, count in KINDS:
        if db is None:
            part = np.zeros((count, n), np.float32)
        else:
            part, _ = oracle.awgn_llrs(code, rng, count, db, np.float32)
        if kind == "clamped":
            for f, x in enumerate((3e38, np.inf, np.nan)):
                part[f, int(rng.integers(0, n))] = np.float32(x)
        parts.append(part)
        where[kind] = list(range(at, at + count))
        at += count
    llrs = np.concatenate(parts)
    llrs.setflags(write=False)
    turn = [where[kind] for kind, _, _ in KINDS]
    idx = np.array([turn[j % len(turn)][(j // len(turn)) % len(turn[j % len(turn)])] for j in range(frames)], dtype=np.int64)
    ref = {cap: oracle.decode_ms_batch(code, llrs, cap)[:3] for cap in caps}
    return llrs, where, idx, ref


@pytest.fixture(scope="module")
def pool():
    # (the seed is one of those at which the oracle's results hold every kind: the last test of this file)
    return _pool(CODE, 0x8192EB4, FRAMES, CAPS)


def _compare(code, llrs, idx, ref, batch, cap, variant=0):
    i = idx[:batch]
    out_g, it_g, ok_g = code.decode_ms_batch(np.ascontiguousarray(llrs[i]), cap, variant=variant)
    out_c, it_c, ok_c = (a[i] for a in ref)
    bad = np.nonzero((it_g != it_c) | (ok_g != ok_c) | (out_g != out_c).any(axis=1))[0]
    assert bad.size == 0, (f"{code.name} cap {cap}, batch {batch}: {bad.size} frames differ, first {bad[0]} (pool entry {i[bad[0]]}): "
                           f"gpu(it={it_g[bad[0]]}, ok={ok_g[bad[0]]}) cpu(it={it_c[bad[0]]}, ok={ok_c[bad[0]]})")


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("batch", (1, 3, FRAMES))
def test_tm8192_f32_default_dispatch_matches_the_oracle(pool, batch, cap):
    llrs, _, idx, ref = pool
    _compare(CODE, llrs, idx, ref[cap], batch, cap)


def test_the_verdict_and_the_cap_met_at_the_same_head(pool):
    """Two 2 dB frames with different iteration counts k at cap 25: at cap k the loop ends on the cap one pass short of the verdict,
    at cap k + 1 the verdict and the cap are met at the same head."""
    llrs, where, idx, ref = pool
    it25 = ref[25][1]
    frames = sorted(where["2dB"], key=lambda f: (it25[f], f))
    chosen = (frames[0], frames[-1])
    assert it25[chosen[0]] != it25[chosen[1]]
    for f in chosen:
        k = int(it25[f])
        for cap, want_ok in ((k, 0), (k + 1, 1)):
            r = oracle.decode_ms_batch(CODE, llrs, cap)[:3]
            assert r[1][f] == k and r[2][f] == want_ok, (f, cap, r[1][f], r[2][f])
            _compare(CODE, llrs, idx, r, FRAMES, cap)


@pytest.mark.parametrize("cap", (25, 29))
def test_tm2048_f32_pair_variant_matches_the_oracle(cap):
    llrs, _, idx, ref = _pool(LDPCCode.TM2048, 0x2048EAD + cap, 4200, (cap,))
    _compare(LDPCCode.TM2048, llrs, idx, ref[cap], 4200, cap, variant=32)


def test_the_pool_holds_every_way_the_loop_head_can_go(pool):
    """From the oracle's results alone."""
    llrs, where, idx, ref = pool
    it, ok = {cap: ref[cap][1] for cap in CAPS}, {cap: ref[cap][2] for cap in CAPS}
    plain = [f for kind in where if kind != "clamped" for f in where[kind]]
    # the range vote (begin_codeword; nocap_limit_for() >= 8 at every cap run here) sends these through the clamp-free copy of the loop
    mag = np.abs(llrs[plain])
    assert (mag < 8.0).all() and ((mag == 0.0) | (mag >= 2.0 ** -20)).all()
    for cap in CAPS:
        assert (it[cap][where["zero"]] == 0).all() and (ok[cap][where["zero"]] == 1).all()
    assert (it[25][where["40dB"]] == 1).all() and ok[25][where["40dB"]].all()
    assert set(it[25][where["12dB"]]) == {1, 2} and ok[25][where["12dB"]].all()
    assert set(it[25][where["7dB"]]) <= {3, 4} and ok[25][where["7dB"]].all()
    assert set(it[25][where["4dB"]]) <= {7, 8} and ok[25][where["4dB"]].all()
    assert ((it[25][where["2dB"]] >= 15) & (it[25][where["2dB"]] <= 19)).all() and ok[25][where["2dB"]].all()
    for cap in (1, 2, 3, 25):
        assert (it[cap][where["-1dB"]] == cap).all() and not ok[cap][where["-1dB"]].any()
    big, inf, nan = where["clamped"]
    assert llrs[big].max() == np.float32(3e38) and np.isinf(llrs[inf]).sum() == 1 and np.isnan(llrs[nan]).sum() == 1
    assert set(idx.tolist()) == set(range(len(llrs)))
    assert all(idx[j] in where[KINDS[j % len(KINDS)][0]] for j in range(FRAMES))         # neighbours in a batch differ in kind
