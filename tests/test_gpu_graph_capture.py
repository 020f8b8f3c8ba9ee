"""Graph-captured calls and the queue-less path of every kernel family ("Semantics to know about": a MEM_DEVICE call
only enqueues work on its stream and can be captured into a HIP graph after one warm-up call; a captured launch takes the fixed stride).

One harness (tests/captured.py) for every case: the call eagerly on input set A, which is the warm-up and, on a plain stream, the
queue-fed launch; one capture on one stream; a replay into sentinels; the next input sets copied into the same buffers and replayed;
the last replay once more with nothing touched.  Every result is compared bit for bit with the project's CPU statements
(tests/oracle.py and the restatements), never with a GPU result; that the replay equals the eager call is asserted on top.

  * test_entry_*: every MEM_DEVICE entry the header does not keep out of captures, through its LDPCCode method, on G + 1 frames (G
    codewords per workgroup or wave group: a partial last group) at caps 0, 1 and 25.  The sets are windows of G + 1 frames over a
    small pool that mixes converging, failing and edge-valued frames (f32: a NaN frame and a +-inf frame too); as many windows as the
    pool needs to pass through whole, two at the least.
  * test_many_groups_*: the launchers whose fixed-stride loop no other test reaches (launch_layered and launch_flooding_corrected with
    workgroups of 512 threads and more), the slot-refill codes, whose capture runs the lockstep kernel, and decode_bf_batch, whose
    capture runs the byte kernel on a wrapped grid: more codeword groups than one round of the un-queued grid.
  * the same batches without a graph: in a child process under LABRADOR_LDPC_HIP_STATIC=1, and on hipStreamPerThread.
  * one receiver chain of five calls in one graph.

The cascades, decode_ms_quantised_batch without bitsliced=True and the half-precision flooding entries are never called under capture
here: the header forbids it."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):               # (the child process of test_many_groups_under_the_static_switch runs this file)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import captured  # noqa: E402
import edge_frames  # noqa: E402
from entry_table import (BS_GROUP, C, CAPS, QUANT, TRIPLE, decode_reference, decoder_results, entries, ffs, flooding_structure,  # noqa: E402
                         host_rows, pool_of, small_pool, small_reference, streaming_cases, torch_dtype, triple_kw, windows)
import hard_frames  # noqa: E402
import labrador_ldpc_amd as la  # noqa: E402
import oracle  # noqa: E402
import quantise_restatement as qr  # noqa: E402

pytestmark = pytest.mark.gpu

MANY_CAP = 20
HIP_STREAM_PER_THREAD = 2                                    # the handle's value in HIP


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the graph-capture GPU tests need a gfx950 device")
    torch.cuda.set_device(0)


# ---- the entries on G + 1 frames ----------------------------------------------------------------------------------------------------------
ENTRIES = entries()


def named(ref, idx, soft):
    d = {"output": ref[0][idx], "iters": ref[1][idx], "success": ref[2][idx]}
    if soft:
        d["app"] = ref[3][idx]
    return d


@pytest.mark.parametrize("cap", CAPS, ids=lambda c: f"cap{c}")
@pytest.mark.parametrize("entry", ENTRIES, ids=[e.id for e in ENTRIES])
def test_entry_replays_on_other_frames(entry, cap):
    """G + 1 frames through the entry: eagerly, captured, replayed on the same and on other frames (module docstring).  Cap 0 launches
    without a queue word for a reason of its own and is a case of its own."""
    import torch
    code, frames = entry.code, entry.g + 1
    pool = small_pool(code, entry.kind)[0]
    ref = small_reference(entry.family, code, entry.kind, cap, entry.params)
    x = torch.empty((frames, code.n()), dtype=torch_dtype(entry.kind), device="cuda")
    app_dtype = x.dtype if entry.app == "same" else torch_dtype(entry.app)
    results = decoder_results(code, frames, entry.soft, app_dtype)
    bufs = dict(results)
    sets = windows(len(pool), frames)
    case = captured.host_case(lambda: entry.call(code, x, cap, bufs), [x], results, [[host_rows(pool[i], entry.kind)] for i in sets],
                              [named(ref, i, entry.soft) for i in sets])
    captured.run(case, f"{entry.id} cap {cap}")


# ---- the streaming kernels ----------------------------------------------------------------------------------------------------------------
STREAMING_IDS = (["decode_bf_batch-cap%d-%s" % (cap, c) for cap in (0, 1, 20) for c in ("TM2048", "TC256")]
                 + ["encode_batch-" + c for c in ("TC256", "TM2048", "TM5120")]
                 + ["%s-%s-TM1280" % (m, s) for s in ("f32", "f64", "i8", "i16", "i32") for m in ("hard_to_llrs_batch", "llrs_to_hard_batch")]
                 + ["%s-%s" % (m, c) for c in ("TC256", "TM6144") for m in ("quantise_llrs_batch-i8", "quantise_llrs_batch-i16",
                                                                           "widen_llrs_batch-f16", "widen_llrs_batch-bf16")])


@pytest.mark.parametrize("name", STREAMING_IDS)
def test_entry_streaming_kernel_replays_on_other_frames(name):
    """Five frames through a streaming kernel, as test_entry_replays_on_other_frames.  decode_bf_batch at this size is the byte kernel
    eagerly and under capture; the switch between its kernels is test_many_groups_replay's."""
    cases = streaming_cases()
    assert sorted(cases) == sorted(STREAMING_IDS)
    captured.run(captured.host_case(*cases[name][1]()), name)


# ---- more groups than one round of the un-queued grid --------------------------------------------------------------------------------------
class Many:
    """One batch of section "the fixed-stride loop": wg, g: threads and codewords per workgroup (the bit-sliced codes and decode_bf:
    None, and `frames` given)."""

    def __init__(self, name, code, kind, wg, g, call, family, params, soft, app="same", frames=None, refill=False):
        self.id = f"{name}-{code.name}"
        self.code, self.kind, self.wg, self.g, self.call, self.family, self.params = code, kind, wg, g, call, family, params
        self.soft, self.app, self.frames, self.refill = soft, app, frames, refill


def layered_wg(code):
    nt = code.submatrix_size() // (2 if code == C.TM8192 else 1)
    return nt


def many_cases():
    out = []
    kw = dict(scale=0.8125, offset=0.0)
    for code in (C.TM2048, C.TM8192):                        # launch_layered, f32: one index per thread, two
        out.append(Many("decode_ms_layered_soft_batch-scale", code, "f32", layered_wg(code), 1,
                        lambda c, x, cap, b, s: c.decode_ms_layered_soft_batch(x, cap, stream=s, **b, **kw), "layered", (0.8125, 0.0), True))
    out.append(Many("decode_ms_layered_fixed_soft_batch-i8-13-4-0", C.TM2048, "i8", layered_wg(C.TM2048), 1,
                    lambda c, x, cap, b, s: c.decode_ms_layered_fixed_soft_batch(x, cap, stream=s, **b, **triple_kw(TRIPLE)), "fixed", TRIPLE,
                    True, app="i32"))
    out.append(Many("decode_ms_layered_fixed_batch-i16", C.TM8192, "i16", layered_wg(C.TM8192), 1,
                    lambda c, x, cap, b, s: c.decode_ms_layered_fixed_batch(x, cap, stream=s, **b), "fixed", None, False))
    out.append(Many("decode_ms_layered_quantised_soft_batch-i8-13-4-0", C.TM8192, "q-i8", layered_wg(C.TM8192), 1,
                    lambda c, x, cap, b, s: c.decode_ms_layered_quantised_soft_batch(x, "i8", *QUANT["i8"], cap, stream=s, **b, **triple_kw(TRIPLE)),
                    "quantised-layered", ("i8", TRIPLE), True, app="i32"))
    for code in (C.TM8192, C.TM2048):                        # launch_flooding_corrected: the pair form (M / 2 threads a frame), one index per thread
        out.append(Many("decode_ms_soft_batch-scale", code, "f32", code.submatrix_size() // (2 if code == C.TM8192 else 1), 1,
                        lambda c, x, cap, b, s: c.decode_ms_soft_batch(x, cap, stream=s, **b, **kw), "flooding-corrected", (0.8125, 0.0), True))
    for code in (C.TM1536, C.TM1280):                        # the default i8 dispatch from 65 536 frames up: slot refill, lockstep under capture
        out.append(Many("decode_ms_batch-i8-refill", code, "i8", None, BS_GROUP[code],
                        lambda c, x, cap, b, s: c.decode_ms_batch(x, cap, stream=s, **b), "bitsliced", (127, None), False,
                        frames=65536 + 3 * BS_GROUP[code] + 3, refill=True))
    # decode_bf_batch above 65 536 frames: the bit-sliced kernel eagerly, the byte kernel on a wrapped grid where there is no queue word
    out.append(Many("decode_bf_batch", C.TM1280, "bf", None, 16, lambda c, x, cap, b, s: c.decode_bf_batch(x, cap, stream=s, **b), "bf", None,
                    False, frames=65536 + 4099))
    return out


MANY = many_cases()
_SHARED = {}                                                 # id -> (pool, kinds, reference): the child process reads the parent's


def many_pool(case):
    """(pool of 24 frames, kind of each, CPU reference at cap 20); decode_bf: hard_frames' 48 words at its 20 iterations"""
    if case.id in _SHARED:
        return _SHARED[case.id]
    code = case.code
    if case.family == "bf":
        words, res, cls = hard_frames.bf_pool(code)
        assert hard_frames.BF_ITERS == MANY_CAP
        got = (words, cls, res)
    else:
        pool, kinds = pool_of(code, case.kind, 8, 0xB16 + int(code))
        if case.kind in ("f32", "q-i8"):                     # eight edge-valued frames, a NaN and a +-inf frame among them: 24 in all
            keep = np.ones(len(pool), bool)
            keep[np.flatnonzero(kinds == 2)[-2:]] = False
            pool, kinds = np.ascontiguousarray(pool[keep]), kinds[keep]
        assert len(pool) == 24
        ref = decode_reference(case.family, code, pool, MANY_CAP, case.params)[:4]
        assert ref[2][kinds == 0].all() and not ref[2][kinds == 1].any(), (case.id, ref[2].tolist())
        got = (pool, kinds, ref)
    _SHARED[case.id] = got
    return got


def check_device(tag, idx, results, dref, chunk=1 << 15):
    """edge_frames.check_on_device for whichever of app, output, iters and success the call has: every frame against its pool entry's
    reference, gathered on the device a chunk of frames at a time"""
    import torch
    for s in range(0, len(idx), chunk):
        i = idx[s: s + chunk]
        bad = torch.zeros(len(i), dtype=torch.bool, device=idx.device)
        for name, t in results:
            a, e = t[s: s + chunk], dref[name][i]
            if a.dtype.is_floating_point:
                na, nb = torch.isnan(a), torch.isnan(e)
                d = (na != nb) | (~na & ~nb & (a != e))
            else:
                d = a != e
            bad |= d.any(dim=1) if d.ndim == 2 else d
        nbad = int(bad.sum())
        assert nbad == 0, f"{tag}: {nbad} frames differ from the CPU reference, first {s + int(torch.nonzero(bad)[0])}"


def many_case(case, stream=None):
    """The captured.Case of a many-groups batch: two index draws (A, B) from the pool of reference frames, gathered into one input
    tensor on the device, compared on the device."""
    import torch
    code = case.code
    pool, kinds, ref = many_pool(case)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = case.g
    if case.frames is None:
        bound = edge_frames.grid_bound(case.wg, g, False, cus)
        frames = bound + bound // 16 + 3
        assert (frames + g - 1) // g > bound // g
    else:
        frames = case.frames
        assert frames > 65536 and frames % g
    rng = np.random.default_rng(0x6A + int(code))
    draw = (lambda: hard_frames.draw(kinds, frames, g, rng)) if case.family == "bf" else (lambda: edge_frames.batch_of(pool, np.arange(len(pool)) % 5, frames, g, rng))
    idx = [torch.from_numpy(draw()).cuda() for _ in range(2)]
    pool_d = torch.from_numpy(np.array(pool)).cuda()
    x = torch.empty((frames, pool.shape[1]), dtype=pool_d.dtype, device="cuda")
    app_dtype = None if not case.soft else x.dtype if case.app == "same" else torch_dtype(case.app)
    results = decoder_results(code, frames, case.soft, app_dtype)
    bufs = dict(results)
    dref = {"output": torch.from_numpy(ref[0]).cuda(), "iters": torch.from_numpy(np.asarray(ref[1]).astype(np.int32)).cuda(),
            "success": torch.from_numpy(ref[2]).cuda()}
    if case.soft:
        dref["app"] = torch.from_numpy(ref[3]).cuda()

    def inputs_are(k, chunk=1 << 15):
        return all(torch.equal(captured.bits(x[s: s + chunk]), captured.bits(pool_d)[idx[k][s: s + chunk]]) for s in range(0, frames, chunk))

    return captured.Case(lambda: case.call(code, x, MANY_CAP, bufs, stream), [x], results, 2,
                         lambda k: torch.index_select(pool_d, 0, idx[k], out=x), lambda tag, k: check_device(tag, idx[k], results, dref),
                         inputs_are)


def i8_kernel(code, batch):
    return la.lib.labrador_ldpc_hip_decode_ms_i8_kernel(int(code), 0, batch).decode()


@pytest.mark.parametrize("case", MANY, ids=[m.id for m in MANY])
def test_many_groups_replay(case):
    """A sixteenth more codeword groups than the largest un-queued grid holds, a partial last group, frames of mixed kinds from a pool
    of 24 (48 for decode_bf): the eager call draws from the queue (the slot-refill codes: the refill kernel; decode_bf: the bit-sliced
    kernel), the replays run the fixed stride (the lockstep kernel; the byte kernel, whose 65 536 workgroups take a second frame)."""
    import torch
    if case.refill:
        assert i8_kernel(case.code, case.frames).endswith("refill_kernel"), i8_kernel(case.code, case.frames)
    if case.family == "bf":                                  # decode_bf.hip: the bit-sliced kernel from 256 groups of 64 / (M / 32) codewords up
        assert case.frames >= 256 * (64 // (case.code.submatrix_size() // 32))
    captured.run(many_case(case), case.id)
    torch.cuda.empty_cache()


def run_many_eagerly(stream=None, say=lambda line: None):
    """every many-groups batch, both index draws, without a graph"""
    import torch
    for case in MANY:
        c = many_case(case, stream)
        for k in range(c.sets):
            captured.run_eager(c, f"{case.id} (set {k})", k)
        say(case.id)
        del c
        torch.cuda.empty_cache()


def test_many_groups_under_the_static_switch(tmp_path):
    """The batches of test_many_groups_replay eagerly in one fresh process under LABRADOR_LDPC_HIP_STATIC=1 (the library reads it once):
    the fixed stride without the runtime's graph machinery, so that a failure of the graph cases can be told from a failure of the loop.
    The child reads this process's pools and references from a file, stops at the first mismatch and prints the case.
    Measured on an MI355X: 3.2 s for the child, interpreter start and imports included (CHILD_SECONDS); the timeout is four times that."""
    ref_file = str(tmp_path / "refs.npz")
    arrays = {}
    for case in MANY:
        pool, kinds, ref = many_pool(case)
        arrays.update({f"{case.id}/pool": pool, f"{case.id}/kinds": kinds, **{f"{case.id}/ref{j}": r for j, r in enumerate(ref)}})
    np.savez(ref_file, **arrays)
    env = dict(os.environ, LABRADOR_LDPC_HIP_STATIC="1")
    t0 = time.monotonic()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), ref_file], env=env, capture_output=True, text=True, cwd=ROOT,
                       timeout=CHILD_TIMEOUT)
    print(f"child process: {time.monotonic() - t0:.1f} s\n{r.stdout[-3000:]}")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert all(f"ok {case.id}\n" in r.stdout for case in MANY), r.stdout[-3000:]


CHILD_SECONDS = 3.2                                          # the child's run time on an MI355X, measured
CHILD_TIMEOUT = 4 * CHILD_SECONDS


def test_many_groups_on_the_per_thread_default_stream():
    """The same batches with opts->stream = hipStreamPerThread (the LDPCCode methods hand `stream` to the entry as it is): the
    launchers treat that handle like a capture and never give it a queue word.  Inputs and sentinels are written by torch before,
    results read after, a device-wide synchronisation each."""
    import torch
    opts = la._device_opts(torch.empty(1, device="cuda"), HIP_STREAM_PER_THREAD)
    assert opts.stream == HIP_STREAM_PER_THREAD and opts.memory == la.MEM_DEVICE      # what the raw symbol is handed
    run_many_eagerly(stream=HIP_STREAM_PER_THREAD)


# ---- one receiver chain --------------------------------------------------------------------------------------------------------------------
def test_receiver_chain_of_five_calls_in_one_graph():
    """TM2048: awgn_frames -> quantise_llrs_batch -> decode_ms_corrected_fixed_batch at (13, 4, 0), and from the quantised soft values
    llrs_to_hard_batch -> decode_bf_batch (decode_ms_corrected_fixed_batch returns no marginals, so the hard slicer takes the decoder's
    soft input).  The seed is baked into a capture: one graph per seed, replayed alternately over the same buffers.  The channel is
    held to its float64 reference under that reference's own criterion (tests/test_gpu_channel_reference.py) and is the eager call's
    bit for bit; every later stage equals its CPU statement on the stage before."""
    import torch
    from test_gpu_channel_reference import _check_f32
    code, frames, sigma, cap, bf_cap = C.TM2048, 4 * BS_GROUP[C.TM2048] + 1, 0.83, 25, 20
    rng = np.random.default_rng(0xC4A1)
    cws = np.stack([oracle.copy_encode(code, rng.integers(0, 256, code.k() // 8, dtype=np.uint8)) for _ in range(8)])
    cws_d = torch.from_numpy(cws).cuda()
    n = code.n()
    t = lambda shape, dtype: torch.empty(shape, dtype=dtype, device="cuda")                                          # noqa: E731
    llrs, q, hard = t((frames, n), torch.float32), t((frames, n), torch.int8), t((frames, n // 8), torch.uint8)
    ms, bf = decoder_results(code, frames, False, None), decoder_results(code, frames, False, None)
    everything = [("llrs", llrs), ("quantised", q), ("hard", hard)] + [("ms " + k, v) for k, v in ms] + [("bf " + k, v) for k, v in bf]

    def chain(seed):
        code.awgn_frames(cws_d, frames, sigma, seed=seed, dtype="f32", out=llrs)
        code.quantise_llrs_batch(llrs, "i8", 8.0, 31, out=q)
        code.decode_ms_corrected_fixed_batch(q, *TRIPLE, cap, **dict(ms))
        code.llrs_to_hard_batch(q, output=hard)
        code.decode_bf_batch(hard, bf_cap, **dict(bf))

    def sentinels():
        captured.fill_sentinels([(k.split()[-1], v) for k, v in everything])

    seeds, graphs, eager, refs = (1234, 98765), {}, {}, {}
    for seed in seeds:
        sentinels()
        chain(seed)
        torch.cuda.synchronize()
        eager[seed] = [v.clone() for _, v in everything]
        y = llrs.cpu().numpy()
        _check_f32(code, cws, 0, frames, sigma, seed, y, f"receiver chain, seed {seed}")
        want_q = qr.quantise(y, np.int8, 8.0, 31)
        want_ms = ffs.decode(flooding_structure(code, ffs), want_q, cap, *TRIPLE)[:3]
        want_hard = np.stack([oracle.llrs_to_hard(code, r) for r in want_q])
        want_bf = [oracle.decode_bf(code, w, bf_cap) for w in want_hard]
        refs[seed] = {"llrs": y, "quantised": want_q, "hard": want_hard, "ms output": want_ms[0], "ms iters": want_ms[1], "ms success": want_ms[2],
                      "bf output": np.stack([w[2] for w in want_bf]), "bf iters": np.array([w[1] for w in want_bf], np.uint32),
                      "bf success": np.array([w[0] for w in want_bf], np.uint8)}
        assert 0 < int(want_ms[2].sum()) < frames, "the chain's frames should both converge and fail"
        captured.check_host(f"receiver chain, seed {seed}, eager", everything, refs[seed])
        graphs[seed] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[seed]):
            chain(seed)
    for rep in range(2):
        for seed in seeds:
            sentinels()
            graphs[seed].replay()
            torch.cuda.synchronize()
            captured.check_host(f"receiver chain, seed {seed}, replay {rep}", everything, refs[seed])
            for (name, v), e in zip(everything, eager[seed]):
                assert torch.equal(captured.bits(v), captured.bits(e)), f"seed {seed}, replay {rep}: {name} differs from the eager chain's"
    assert torch.equal(cws_d.cpu(), torch.from_numpy(cws))


# ---- the child process of test_many_groups_under_the_static_switch -------------------------------------------------------------------------
def child(ref_file):
    import torch
    if os.environ.get("LABRADOR_LDPC_HIP_STATIC") != "1":
        print("LABRADOR_LDPC_HIP_STATIC is not set")
        return 2
    z = np.load(ref_file)
    for case in MANY:
        _SHARED[case.id] = (z[f"{case.id}/pool"], z[f"{case.id}/kinds"], tuple(z[f"{case.id}/ref{j}"] for j in range(4 if f"{case.id}/ref3" in z else 3)))
    if la.device_count() < 1 or not torch.cuda.is_available():
        print("no gfx950 device")
        return 2
    torch.cuda.set_device(0)
    try:
        run_many_eagerly(say=lambda line: print("ok " + line, flush=True))
    except AssertionError as e:
        print(f"MISMATCH {e}", flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(child(sys.argv[1]))
