"""captured.py -- the one harness of tests/test_gpu_graph_capture.py: library calls run eagerly, captured into a HIP graph and replayed
over the same buffers on other frames.

TEST INFRASTRUCTURE ONLY.  A Case holds a callable that issues library calls on torch's current stream, the preallocated device tensors
those calls read (`inputs`) and write (`results`, by name), a way to put input set k into the inputs (`load`) and a way to hold the
results to the CPU reference of set k (`check`).  run() is the sequence; run_eager() its first two steps, for the processes and streams
that reach the fixed stride without a graph."""
from __future__ import annotations

import numpy as np

SENTINEL = {"output": 0xEE, "success": 7, "app": -77777}


def fill_sentinels(results):
    """0xEE, -2, 7 and -77777 in the style of tests/test_gpu_quantised_layered.py (int8: -77, int16: -7777); every other word of `iters` is
    0xFFFFFFFF, the two-pass NaN mark, which no call may take for its own."""
    import torch
    for name, t in results:
        if name == "iters":
            t.fill_(-2)
            t[::2] = -1
        elif name in SENTINEL and t.dtype not in (torch.int8, torch.int16):
            t.fill_(SENTINEL[name])
        elif t.dtype == torch.uint8:
            t.fill_(0xEE)
        elif t.dtype == torch.int8:
            t.fill_(-77)
        elif t.dtype == torch.int16:
            t.fill_(-7777)
        else:
            t.fill_(-77777)


def bits(t):
    """a tensor as integer words of its element size: equality of these is equality bit for bit"""
    import torch
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_values(a, b):
    """tensors equal as values, NaN exactly where the other has NaN (include/labrador_ldpc_hip.h's rule for `app`)"""
    import torch
    if a.dtype.is_floating_point:
        na, nb = torch.isnan(a), torch.isnan(b)
        return bool((na == nb).all()) and bool((a[~na] == b[~nb]).all())
    return torch.equal(a, b)


def host(t):
    import torch
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    a = t.cpu().numpy()
    return a.view(np.uint32) if t.dtype == torch.int32 and a.ndim == 1 else a


def check_host(tag, results, ref):
    """`results` [(name, tensor)] against `ref` {name: numpy array}: exact; floats as values with NaN exactly where the reference has
    NaN (layered_helpers.same_app, and bad_frames of tests/test_gpu_soft_edges.py to name the frames)."""
    for name, t in results:
        got, want = host(t), np.asarray(ref[name])
        assert got.shape == want.shape, (tag, name, got.shape, want.shape)
        if got.dtype.kind == "f":
            na, nb = np.isnan(got), np.isnan(want)
            bad = (na != nb) | (~na & ~nb & (got != want))
        else:
            bad = got.astype(np.int64) != want.astype(np.int64)
        bad = np.flatnonzero(bad.reshape(len(want), -1).any(axis=1))
        assert bad.size == 0, f"{tag}: {name} differs from the CPU reference in frames {bad[:8].tolist()} ({bad.size} of {len(want)})"


class Case:
    """call(): the library calls, every result buffer passed in.  inputs: [tensor].  results: [(name, tensor)].  sets: how many input
    sets there are (A, B, ...).  load(k): set k into `inputs`, in place.  check(tag, k): the results against the CPU reference of set
    k.  inputs_are(k): the inputs still hold set k, bit for bit."""

    def __init__(self, call, inputs, results, sets, load, check, inputs_are):
        self.call, self.inputs, self.results, self.sets = call, inputs, results, sets
        self.load, self.check, self.inputs_are = load, check, inputs_are


def host_case(call, inputs, results, sets, refs):
    """A Case whose input sets are host arrays (`sets`: one list of arrays or CPU tensors per set, in the order of `inputs`) and whose
    references are {name: numpy array} per set."""
    import torch

    def as_tensor(x):
        return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))

    staged = [[as_tensor(x) for x in s] for s in sets]

    def load(k):
        for t, x in zip(inputs, staged[k]):
            assert t.shape == x.shape and t.dtype == x.dtype, (t.shape, x.shape, t.dtype, x.dtype)
            t.copy_(x)

    def inputs_are(k):
        return all(torch.equal(bits(t).cpu(), bits(x)) for t, x in zip(inputs, staged[k]))

    return Case(call, inputs, results, len(sets), load, lambda tag, k: check_host(tag, results, refs[k]), inputs_are)


def run_eager(case, tag, k=0):
    """Set k through the callable as it stands (on a plain stream this is the queue-fed launch), into sentinels, against the reference."""
    import torch
    case.load(k)
    fill_sentinels(case.results)
    torch.cuda.synchronize()
    case.call()
    torch.cuda.synchronize()
    case.check(f"{tag}: eager", k)
    assert case.inputs_are(k), f"{tag}: the eager call changed its inputs"


def run(case, tag):
    """Eager on A (the warm-up the documentation asks for) against A's reference; one capture, on one stream; replay into sentinels: A's
    reference and the eager results; then every further set copied into the inputs in place and replayed; the last replay once more
    with nothing touched; the inputs unchanged at the end."""
    import torch
    assert case.sets >= 2
    run_eager(case, tag)
    eager = [t.clone() for _, t in case.results]
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):                        # (torch captures on one side stream: what `call` enqueues is a linear chain)
        allocations = torch.cuda.memory_stats()["allocation.all.allocated"]
        case.call()
        allocations -= torch.cuda.memory_stats()["allocation.all.allocated"]
    assert allocations == 0, f"{tag}: the call allocated {-allocations} tensors while it was captured"
    fill_sentinels(case.results)
    graph.replay()
    torch.cuda.synchronize()
    case.check(f"{tag}: first replay", 0)
    for (name, t), e in zip(case.results, eager):
        assert same_values(t, e), f"{tag}: {name} of the replay differs from the eager call's"
    del eager
    for k in range(1, case.sets):
        case.load(k)
        fill_sentinels(case.results)
        graph.replay()
        torch.cuda.synchronize()
        case.check(f"{tag}: replay on set {k}", k)
    graph.replay()                                       # nothing refilled: a queue word, a mark or a slab left behind shows here
    torch.cuda.synchronize()
    case.check(f"{tag}: replay on set {case.sets - 1} again", case.sets - 1)
    assert case.inputs_are(case.sets - 1), f"{tag}: the replays changed their inputs"
    del graph
