"""Every batched entry of the C ABI on every route of the one batched call path (csrc/capi_frame.hpp, csrc/capi_staging.hpp).

The entries differ from one another only in their buffer description -- the bytes per item of each buffer, the place of `app` behind
an optional `stage`, the optional second input, rows of n / 8 -- and a wrong description shows only where an item offset is not zero
or a padding boundary is crossed.  So each entry of tests/entry_table.py's table (every batched symbol of the header, once on its
smallest code; the bit-sliced ones on TM1536 too) runs on each route tests/call_routes.py picks a batch for:

  r1 direct (and r1-group: one codeword group, the call that may be completed by a ticket), r2 small, r3 one chunk, r4 pipelined
  (three chunks, a ragged last one), r5 one device launch (G + 1 frames), r6 launch slices of 8 (17 frames; r6-16: TM1280, 33 frames
  in slices of 16; r6-ws: the workspace entries with their workspace's chunk at 5 as well), r7 a device set [0, 0] (on the small
  batch, on 17 frames, and on shards that are pipelined themselves).

A case calls through the LDPCCode method (host bf16 rows, which numpy cannot hold, through the symbol) into the caller's result
buffers, which hold one spare row past the batch; results and spare row start as sentinels (iters -2, bytes 0xEE, floats a NaN of a
pattern no decoder makes).  Every result row is compared with the CPU statement of the entry's family -- exactly; float marginals as
values with NaN exactly where the statement has NaN, as edge_frames.check_on_device compares them --, the spare rows must still hold
the sentinel and the inputs must be unchanged.  The batches are drawn from small pools by committed seeds such that a pointer left
behind, or advanced by another buffer's stride, cannot give the right answer (tests/test_call_routes_host.py).

test_small_routes_in_processes_without_the_direct_call_and_without_the_ticket runs the r1 and r2 cases again in a fresh process under
LABRADOR_LDPC_HIP_NO_DIRECT=1, then under LABRADOR_LDPC_HIP_NO_NOTIFY=1 (both are read once per process)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import call_routes as rt
import edge_frames
import entry_table as et
import guarded_buffers as gb
import labrador_ldpc_amd as la

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = et.route_entries()
PICKED = [c for e in ENTRIES for c in rt.cases(e)]
CASES = [c for c in PICKED if isinstance(c, rt.Case)]
VARIABLES = (rt.CHUNK, rt.MAX_LAUNCH) + tuple(et.WORKSPACE_CHUNK.values())


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the route tests need a gfx950 device")
    torch.cuda.set_device(0)


def sentinels(entry, rows):
    """{name: numpy array [rows, ...]} of the entry's results, every element a sentinel"""
    out = {}
    for name, dt, row in entry.results:
        a = np.empty((rows,) + ((row,) if row else ()), dt)
        if name == "iters":
            a[...] = -2
        elif dt.kind == "f":
            a.view(np.uint32 if dt.itemsize == 4 else np.uint64)[...] = et.SENTINEL_NAN[dt]
        else:
            a.view(np.uint8)[...] = 0xEE
        out[name] = a
    return out


def first_bad_row(got, want):
    """the first row of `got` that differs from `want`, or None: integers exactly, floats as values with NaN where `want` has NaN"""
    if got.dtype.kind == "f":
        na, nb = np.isnan(got), np.isnan(want)
        bad = (na != nb) | (~na & ~nb & (got != want))
    else:
        bad = got != want
    bad = np.flatnonzero(bad.reshape(len(want), -1).any(axis=1))
    return None if bad.size == 0 else (int(bad[0]), int(bad.size))


def run_case(case, monkeypatch):
    import torch
    entry, n = case.entry, case.batch
    idx = rt.draw(case)
    ref = entry.reference()
    for name in VARIABLES:
        if name in case.env:
            monkeypatch.setenv(name, str(case.env[name]))
        else:
            monkeypatch.delenv(name, raising=False)
    rows = [np.ascontiguousarray(p[idx]) for p in entry.pool()]
    fresh = sentinels(entry, n + 1)
    if case.device:
        inputs = [et.host_rows(x, entry.kind).cuda() if entry.kind in ("f16", "bf16") else torch.from_numpy(x).cuda() for x in rows]
        bufs = {name: torch.from_numpy(a).cuda() for name, a in fresh.items()}
        kw = {name: b[:n] for name, b in bufs.items()}
    else:
        inputs = rows
        bufs = {name: a.copy() for name, a in fresh.items()}
        kw = dict({name: b[:n] for name, b in bufs.items()}, devices=case.devices)
    frozen = [gb.frozen(x, f"input {k}") for k, x in enumerate(inputs)]
    entry.method(entry.code, inputs, kw)
    if case.device:
        torch.cuda.synchronize()
    got = {name: b.cpu().numpy() if case.device else b for name, b in bufs.items()}
    tag = f"{case.id} ({n} frames, {case.env or 'no variables'})"
    for name, _, _ in entry.results:
        bad = first_bad_row(got[name][:n], ref[name][idx])
        assert bad is None, f"{tag}: {name} differs from the CPU statement in {bad[1]} rows, first {bad[0]} (pieces start at {case.starts[:8]})"
    for name, a in fresh.items():
        assert got[name][n:].tobytes() == a[n:].tobytes(), f"{tag}: the spare row of {name} was written"
    for f in frozen:
        f.check()
    if case.device and [name for name, _, _ in entry.results] == ["output", "iters", "success", "app"]:
        idx_d = torch.from_numpy(idx).cuda()
        dref = tuple(torch.tensor(ref[name]).cuda() for name in ("output", "iters", "success", "app"))
        edge_frames.check_on_device(tag, idx_d, tuple(kw[name] for name in ("app", "output", "iters", "success")), dref)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_entry_on_route(case, monkeypatch):
    run_case(case, monkeypatch)


def test_only_the_direct_call_is_ever_out_of_reach():
    """what tests/test_call_routes_host.py asserts of the picker, said here of the matrix that ran"""
    skipped = [c for c in PICKED if isinstance(c, rt.Unreachable)]
    assert all(c.route == "r1" for c in skipped), [(c.id, c.reason) for c in skipped]


# ---- the small routes without the direct call, and without the completion ticket ------------------------------------------------------------
SMALL_ROUTES = "r1] or r1-group] or r2]"
CHILD_SECONDS = 7.6                                          # a child's run time on an MI355X, measured: interpreter start, imports, 221 cases
CHILD_TIMEOUT = 8 * CHILD_SECONDS


def test_small_routes_in_processes_without_the_direct_call_and_without_the_ticket():
    """LABRADOR_LDPC_HIP_NO_DIRECT=1: every call of up to 64 KiB is copied in and out of the pinned block like the small call, so the
    copy-out form is the only one; LABRADOR_LDPC_HIP_NO_NOTIFY=1: the direct calls synchronise their stream.  One fresh pytest process
    per variable, one after the other, on this file's r1, r1-group and r2 cases."""
    for name in ("LABRADOR_LDPC_HIP_NO_DIRECT", "LABRADOR_LDPC_HIP_NO_NOTIFY"):
        if os.environ.get(name):
            return
    expected = sum(1 for c in CASES if c.route in ("r1", "r1-group", "r2"))
    for name in ("LABRADOR_LDPC_HIP_NO_DIRECT", "LABRADOR_LDPC_HIP_NO_NOTIFY"):
        t0 = time.monotonic()
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                            os.path.abspath(__file__) + "::test_entry_on_route", "-k", SMALL_ROUTES],
                           env=dict(os.environ, **{name: "1"}), capture_output=True, text=True, cwd=ROOT, timeout=CHILD_TIMEOUT)
        print(f"{name}: child process {time.monotonic() - t0:.1f} s\n{r.stdout[-1500:]}")
        assert r.returncode == 0, f"{name}=1:\n" + r.stdout[-3000:] + r.stderr[-3000:]
        assert f"{expected} passed" in r.stdout, f"{name}=1: not the {expected} small-route cases:\n" + r.stdout[-1500:]
