"""TM8192 f32 through the default dispatch -- the pair kernel, whose hard-output f32 instantiations finish the check messages of
some local edges at the NEXT loop head, from a sign word and a partial minimum kept across the barrier (csrc/decode_ms_pair.hpp,
DEFER) -- against the CPU oracle, bit for bit: hard bits, iteration counts, success flags.

What deferral can get wrong is state carried over a barrier and over a codeword boundary: a head that finishes with what an earlier
pass or an earlier codeword kept, a peeled pass that leaves an edge unfinished which the first head does not pick up.  The pool of
distinct frames is that of tests/test_gpu_pair_verdict.py (built the same way, from another seed): the all-zero frame, frames at 40,
12, 7, 4, 2 and -1 dB, and one frame each with an LLR of 3e38, of inf and of NaN, which fail the LLR range vote and run the clamped
copy of the loop.  A batch interleaves the kinds in the OPPOSITE order to that file's, so a persistent workgroup meets other
successions than there: from an exit on the cap into an immediate success, from a clamped codeword into a clamp-free one.

Caps 0, 1, 2, 3, 4, 25 and 29 (from 29 on the launcher takes form 3 of the self-correction): cap 0 never reaches a head; at cap 1
the peeled pass defers and nobody finishes; cap 2 has the first head that finishes what the peeled pass left.  Batches of 1, 3 and
520 frames (more than twice the 256 workgroups an MI355X holds of this kernel).  The gate is on the early u reads, so the TM2048 f32
pair kernels (`variant` 32) defer too: one batch of theirs, 4200 frames of the same mixture, at caps 25 and 29."""
import numpy as np
import pytest

import oracle
from labrador_ldpc_amd import LDPCCode

pytestmark = pytest.mark.gpu

CODE = LDPCCode.TM8192
CAPS = (0, 1, 2, 3, 4, 25, 29)
FRAMES = 520                                     # > 2 x 256 resident workgroups
# (kind, Eb/N0 in dB, frames); the order of the kinds is the order in which a batch interleaves them
KINDS = (("4dB", 4.0, 4), ("7dB", 7.0, 4), ("12dB", 12.0, 6), ("clamped", 2.0, 3), ("40dB", 40.0, 2), ("zero", None, 1),
         ("-1dB", -1.0, 2), ("2dB", 2.0, 8))


def _pool(code, seed, frames, caps):
    """The distinct frames, {kind: their pool indices}, `frames` pool indices that go through the kinds in turn and the oracle's
    results per cap (computed once, never modified)."""
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
    return _pool(CODE, 0x8192DEF, FRAMES, CAPS)


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


@pytest.mark.parametrize("cap", (25, 29))
def test_tm2048_f32_pair_variant_matches_the_oracle(cap):
    llrs, _, idx, ref = _pool(LDPCCode.TM2048, 0x2048DEF + cap, 4200, (cap,))
    _compare(LDPCCode.TM2048, llrs, idx, ref[cap], 4200, cap, variant=32)


def test_the_pool_holds_every_kind_of_exit(pool):
    """From the oracle's results alone."""
    llrs, where, idx, ref = pool
    it, ok = {cap: ref[cap][1] for cap in CAPS}, {cap: ref[cap][2] for cap in CAPS}
    plain = [f for kind in where if kind != "clamped" for f in where[kind]]
    # the range vote (begin_codeword; nocap_limit_for() >= 8 at every cap run here) sends these through the clamp-free copy of the loop
    mag = np.abs(llrs[plain])
    assert (mag < 8.0).all() and ((mag == 0.0) | (mag >= 2.0 ** -20)).all()
    # success before any pass (iters 0), at the first head (iters 1), a few heads on, and late
    for cap in CAPS[1:]:
        assert (it[cap][where["zero"]] == 0).all() and (ok[cap][where["zero"]] == 1).all()
    assert (it[25][where["40dB"]] == 1).all() and ok[25][where["40dB"]].all()
    assert set(it[25][where["12dB"]]) <= {1, 2} and ok[25][where["12dB"]].all()
    assert set(it[25][where["7dB"]]) <= {3, 4, 5, 6} and ok[25][where["7dB"]].all()
    assert ((it[25][where["4dB"]] >= 6) & (it[25][where["4dB"]] <= 9)).all() and ok[25][where["4dB"]].all()
    assert ((it[25][where["2dB"]] >= 12) & (it[25][where["2dB"]] <= 24)).all() and ok[25][where["2dB"]].all()
    # the cap: no pass at all, the peeled pass alone, one head that finishes what it left, and on
    noisy = where["-1dB"] + where["2dB"]
    assert (it[0] == 0).all() and not ok[0][noisy].any()
    for cap in (1, 2, 3, 4, 25):
        assert (it[cap][where["-1dB"]] == cap).all() and not ok[cap][where["-1dB"]].any()
    for cap in (1, 2, 3, 4):
        assert (it[cap][where["2dB"]] == cap).all() and not ok[cap][where["2dB"]].any()
    # success at the very head where a lower cap ends the loop: 40 dB at caps 1 and 2
    assert (it[1][where["40dB"]] == 1).all() and not ok[1][where["40dB"]].any() and ok[2][where["40dB"]].all()
    big, inf, nan = where["clamped"]
    assert llrs[big].max() == np.float32(3e38) and np.isinf(llrs[inf]).sum() == 1 and np.isnan(llrs[nan]).sum() == 1
    assert set(idx.tolist()) == set(range(len(llrs)))
    assert all(idx[j] in where[KINDS[j % len(KINDS)][0]] for j in range(FRAMES))         # neighbours in a batch differ in kind
