"""The soft two-stage decode on the GPU (labrador_ldpc_decode_ms_cascade_soft_batch_{f32,i8,i16}; LDPCCode.decode_ms_cascade_soft_batch
and decode_ms_cascade_fixed_soft_batch) against its contract: per frame, exactly the composition of the library's own
separate soft entries -- decode_ms_soft_batch, then the soft layered decoder of the type on the frames it failed -- put together in
numpy (tests/cascade_soft_restatement.compose_soft), and for TC128, TM1280 and TM2048 also the CPU statement.  Output, iters, success
and stage are compared exactly, and with the hard cascade's; marginals exactly for the integers and as values for float32 (NaN equals
NaN, -0.0 equals +0.0).  The frames are those fixed in tests/cascade_soft_restatement.py and checked in tests/test_cascade_soft_host.py."""
import ctypes
import functools

import numpy as np
import pytest

import cascade_soft_restatement as csr
from cascade_soft_restatement import same_soft
import edge_frames
import guarded_buffers as gb
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
from layered_helpers import quantise
import oracle

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
CPU_CODES = (LDPCCode.TC128, LDPCCode.TM1280, LDPCCode.TM2048)
# (code, LLR type, setting): a setting is {} (both stages plain), a stage-1 pair or a stage-2 correction
F32_SETTINGS = ({}, dict(flooding=(0.8125, 0.0)), dict(correction=(1.0, 0.5)))
INT_SETTINGS = ({}, dict(correction=(13, 4, 1)))
CASES = ([(c, np.float32, s) for c in (LDPCCode.TC128, LDPCCode.TM1280) for s in F32_SETTINGS] + [(LDPCCode.TM8192, np.float32, {})] +
         [(c, np.int8, s) for c in (LDPCCode.TC128, LDPCCode.TM1280, LDPCCode.TM2048) for s in INT_SETTINGS] +
         [(LDPCCode.TM2048, np.int16, s) for s in INT_SETTINGS])


def case_id(case):
    code, dtype, setting = case
    tail = "-".join(f"{k}_" + "_".join(str(x) for x in v) for k, v in setting.items())
    return f"{code.name}-{np.dtype(dtype).name}" + ("-" + tail if tail else "")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the soft cascade GPU tests need a gfx950 device")
    torch.cuda.set_device(0)


def is_float(x):
    return str(x.dtype) in ("float32", "torch.float32")


def keywords(llrs, correction=None, flooding=None):
    kw = {}
    if correction is not None:
        kw = dict(scale=correction[0], offset=correction[1]) if is_float(llrs) else dict(scale_num=correction[0], scale_shift=correction[1],
                                                                                       offset=correction[2])
    if flooding is not None:
        kw.update(flooding_scale=flooding[0], flooding_offset=flooding[1])
    return kw


def to_numpy(res):
    import torch
    return tuple(r.cpu().numpy().view(np.uint32) if r.dtype == torch.int32 and r.ndim == 1 else r.cpu().numpy() for r in res)


def soft_cascade(code, llrs, max_iters, max_sweeps, correction=None, flooding=None, device=False, **kw):
    """The call under test on host buffers, or (device=True) on device buffers; numpy results either way."""
    method = code.decode_ms_cascade_soft_batch if is_float(llrs) else code.decode_ms_cascade_fixed_soft_batch
    if not device:
        return method(llrs, max_iters, max_sweeps, **keywords(llrs, correction, flooding), **kw)
    import torch
    res = method(torch.from_numpy(np.array(llrs)).cuda(), max_iters, max_sweeps, **keywords(llrs, correction, flooding), **kw)
    torch.cuda.synchronize()
    return to_numpy(res)


def hard_cascade(code, llrs, max_iters, max_sweeps, correction=None, flooding=None, **kw):
    method = code.decode_ms_cascade_batch if is_float(llrs) else code.decode_ms_cascade_fixed_batch
    return method(llrs, max_iters, max_sweeps, **keywords(llrs, correction, flooding), **kw)


def separate(code, correction=None, flooding=None):
    """The library's own two soft entries as functions of (llrs, cap) -> (output, iters, success, app), for compose_soft."""
    def first(llrs, cap):
        scale, offset = flooding or (1.0, 0.0)
        app, out, it, ok = code.decode_ms_soft_batch(llrs, cap, scale=scale, offset=offset)
        return out, it, ok, app

    def second(llrs, cap):
        if llrs.dtype == np.float32:
            scale, offset = correction or (1.0, 0.0)
            app, out, it, ok = code.decode_ms_layered_soft_batch(llrs, cap, scale=scale, offset=offset)
        else:
            num, shift, offset = correction or (None, None, None)
            app, out, it, ok = code.decode_ms_layered_fixed_soft_batch(llrs, cap, scale_num=num, scale_shift=shift, offset=offset)
        return out, it, ok, app
    return first, second


def composed(code, llrs, max_iters, max_sweeps, correction=None, flooding=None):
    return csr.compose_soft(*separate(code, correction, flooding), llrs, max_iters, max_sweeps)


@functools.lru_cache(maxsize=None)
def plain_reference(code, dtype, caps):
    """The composition of the separate entries on the fixed frames, both stages plain: computed once, read-only, shared."""
    ref = composed(code, csr.frames(code, dtype), *caps)
    for x in ref:
        x.setflags(write=False)
    return ref


def same_hard(got, want, what=""):
    for name, g, w in zip(("output", "iters", "success", "stage"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and (g.view(np.uint8) == w.view(np.uint8)).all(), (what, name)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_equals_the_composition(case):
    """At caps (3, 20) and (25, 25): both stages carry frames; host and device calls give the composition of the two separate soft
    calls, all five arrays; their hard four are the hard cascade's bit for bit; on three codes the composition is the CPU statement."""
    code, dtype, setting = case
    llrs = csr.frames(code, dtype)
    for caps in csr.CAPS:
        want = composed(code, llrs, *caps, **setting) if setting else plain_reference(code, dtype, caps)
        stage = want[4]
        print(f"{case_id(case)} caps {caps}: {int((stage == 0).sum())} frames of stage 0, {int(stage.sum())} of stage 1, "
              f"{int((want[3] == 0).sum())} failed by both")
        mixed = 0 < int(stage.sum()) < len(stage)
        assert mixed
        if caps[0] == 3 and code != LDPCCode.TM8192:
            assert int(stage.sum()) > 64                                        # the compaction's places cross a wave
        host = soft_cascade(code, llrs, *caps, **setting)
        same_soft(host, want, f"host buffers, caps {caps}")
        same_soft(soft_cascade(code, llrs, *caps, device=True, **setting), want, f"device buffers, caps {caps}")
        same_hard(host[1:], hard_cascade(code, llrs, *caps, **setting), f"the hard cascade, caps {caps}")
        if code in CPU_CODES:
            same_soft(want, csr.cascade_soft(code, llrs, *caps, **setting), f"the composition against the CPU statement, caps {caps}")


@pytest.mark.parametrize("code,dtype", [(LDPCCode.TM1280, np.float32), (LDPCCode.TM1280, np.int8), (LDPCCode.TM2048, np.int16)],
                         ids=lambda x: x.name if isinstance(x, LDPCCode) else np.dtype(x).name)
def test_chunks(code, dtype, monkeypatch):
    """LABRADOR_LDPC_HIP_CASCADE_CHUNK=5: several stage-2 chunks with their dense marginals and, for the integers, 151 = 30 * 5 + 1
    frames of stage 1 in widen chunks, the last one partial; launch slices of 16 frames, and both: the results of the unset run."""
    llrs = csr.frames(code, dtype)
    caps = csr.CAPS[0]
    want = plain_reference(code, dtype, caps)
    assert len(llrs) % 5 == 1 and want[4].sum() > 10
    for env in (dict(LABRADOR_LDPC_HIP_CASCADE_CHUNK="5"), dict(LABRADOR_LDPC_HIP_MAX_LAUNCH="16"),
                dict(LABRADOR_LDPC_HIP_CASCADE_CHUNK="5", LABRADOR_LDPC_HIP_MAX_LAUNCH="16")):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            same_soft(soft_cascade(code, llrs, *caps, device=True), want, f"device buffers, {env}")
            same_soft(soft_cascade(code, llrs, *caps), want, f"host buffers, {env}")
    with monkeypatch.context() as m:                          # host buffers staged in chunks of 32 frames: five outputs, two staging sets
        m.setenv("LABRADOR_LDPC_HIP_CHUNK", "32")
        m.setenv("LABRADOR_LDPC_HIP_CASCADE_CHUNK", "5")
        reps = 1 + (1 << 20) // llrs.nbytes                   # (past the small-call path: more than 1 MiB)
        big = np.ascontiguousarray(np.tile(llrs, (reps, 1)))
        same_soft(soft_cascade(code, big, *caps), tuple(np.tile(x, (reps,) + (1,) * (x.ndim - 1)) for x in want), "staged chunks")


@pytest.mark.parametrize("dtype", (np.float32, np.int8, np.int16), ids=lambda t: np.dtype(t).name)
def test_caps_of_zero_and_clean_batches(dtype):
    """max_iters = 0: `stage` all 1 and every result, `app` included, the layered soft entry's.  max_sweeps = 0: the composition.  A
    batch flooding decodes completely (clean codewords): `stage` all 0, `app` the flooding soft entry's, the dense path never entered."""
    code = LDPCCode.TM1280
    llrs = csr.frames(code, dtype)[:49]
    first, second = separate(code)
    layered = second(llrs, 25)
    clean = np.ascontiguousarray(oracle.awgn_llrs(code, np.random.default_rng(9), 33, 12.0, np.float32)[0])
    clean = clean if dtype == np.float32 else quantise(clean, dtype, 8, 31)
    flooding = first(clean, 25)
    assert flooding[2].all()
    for device in (False, True):
        got = soft_cascade(code, llrs, 0, 25, device=device)
        same_soft(got, (layered[3], layered[0], layered[1], layered[2], np.ones(49, np.uint8)), "max_iters = 0")
        same_soft(soft_cascade(code, llrs, 3, 0, device=device), composed(code, llrs, 3, 0), "max_sweeps = 0")
        got = soft_cascade(code, clean, 25, 25, device=device)
        app1 = flooding[3] if dtype == np.float32 else flooding[3].astype(np.int32)
        same_soft(got, (app1, flooding[0], flooding[1], flooding[2], np.zeros(33, np.uint8)), "clean codewords")


def test_nan_llrs_in_each_stage():
    """A frame of tests/edge_frames.py (its denormal one, which both decoders decode) with NaNs where its LLRs were positive -- the
    kernels read a NaN LLR as +inf, so the frame still decodes: at cap 25 flooding decodes it (stage 0, flooding's NaN rule), at
    max_iters = 0 the layered decoder does (stage 1, its rule).  Either way a NaN marginal exactly at each NaN LLR, beside ordinary
    frames of both stages."""
    code = LDPCCode.TM1280
    row = edge_frames.whole_frame_rows(code, np.float32, np.random.default_rng(77), 7.0)[4].copy()
    at = np.flatnonzero(row > 0)[[3, 100, 200]]
    row[at] = np.nan
    llrs = np.array(csr.frames(code, np.float32)[:37])
    llrs[11] = row
    for caps, stage in (((25, 25), 0), ((0, 25), 1)):
        want = composed(code, llrs, *caps)
        assert want[4][11] == stage and want[3][11] == 1
        assert np.flatnonzero(np.isnan(want[0][11])).tolist() == at.tolist()
        same_soft(want, csr.cascade_soft(code, llrs, *caps), f"the CPU statement, caps {caps}")
        for device in (False, True):
            same_soft(soft_cascade(code, llrs, *caps, device=device), want, f"caps {caps}, device {device}")


def saturating_batch(code):
    """6 codewords at the type's limits (every LLR -128 or 127: the reference's saturating sums stay there), 6 full-scale frames of
    random sign from tests/edge_frames.py, 45 ordinary ones."""
    clean = np.where(oracle.awgn_llrs(code, np.random.default_rng(6), 6, 12.0, np.float32)[0] > 0, 127, -128).astype(np.int8)
    full = edge_frames.integer_range_rows(code, np.int8, np.random.default_rng(5), 6)[:6]
    return np.ascontiguousarray(np.concatenate([clean, full, csr.frames(code, np.int8)[:45]]))


def test_i8_rows_that_saturate():
    """Full-scale int8 codewords, which flooding decodes at once with marginals pinned at -128 / 127, beside frames of stage 1 whose
    exact layered sums lie beyond +-127, in one batch: `app` holds both, each in its frame's rows."""
    code = LDPCCode.TM1280
    llrs = saturating_batch(code)
    want = composed(code, llrs, 3, 20)
    app, stage = want[0], want[4]
    assert app.dtype == np.int32
    s0, s1 = app[stage == 0], app[stage == 1]
    print(f"stage 0: marginals {s0.min()} .. {s0.max()}; stage 1: {s1.min()} .. {s1.max()}")
    assert not stage[:6].any() and s0.min() == -128 and s0.max() == 127 and s1.min() < -128 and s1.max() > 127
    same_soft(want, csr.cascade_soft(code, llrs, 3, 20), "the CPU statement")
    for device in (False, True):
        same_soft(soft_cascade(code, llrs, 3, 20, device=device), want, f"device {device}")


def test_variant_64_has_no_soft_form():
    """The bit-sliced kernels have no soft form: `variant` 64 is EUNSUPPORTED with the soft flooding entry's text."""
    code = LDPCCode.TM1280
    llrs = csr.frames(code, np.int8)[:17]
    for device in (False, True):
        with pytest.raises(la.LdpcHipError, match="status -4.*no soft-output form"):
            soft_cascade(code, llrs, 3, 20, variant=64, device=device)


def test_half_precision_llrs_are_refused():
    """float32 only: float16 and bfloat16 device tensors raise LdpcHipError, as on the other f32-only paths."""
    import torch
    code = LDPCCode.TC128
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(la.LdpcHipError, match="no batched kernel"):
            code.decode_ms_cascade_soft_batch(torch.ones((2, code.n()), dtype=dt, device="cuda"), 10)


CONTAINED = [(LDPCCode.TM1280, np.float32), (LDPCCode.TM1280, np.int8), (LDPCCode.TM2048, np.int16)]


@pytest.mark.parametrize("on_device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("code,dtype", CONTAINED, ids=lambda x: x.name if isinstance(x, LDPCCode) else np.dtype(x).name)
def test_writes_stay_inside_the_result_rows(code, dtype, on_device):
    """G + 1 = 17 frames into guarded `app` (16-byte aligned on the device, to its element on the host), `output`, `iters`, `success`
    and `stage`: every guard band intact, `llrs` unchanged, the results those of the composition."""
    import torch
    B, V = 17, code.n() + code.punctured_bits()
    device = torch.device("cuda", 0) if on_device else None
    want = tuple(x[:B] for x in plain_reference(code, dtype, csr.CAPS[0]))
    assert 0 < want[4].sum() < B
    llrs, g_llrs = gb.guarded_copy(csr.frames(code, dtype)[:B], 0, device)
    keep = gb.frozen(llrs, "llrs")
    app_dtype = np.float32 if dtype == np.float32 else np.int32
    app, g_app = gb.guarded(B, (V,), app_dtype, 0 if on_device else 4, device, name="app", app=True)
    out, g_out = gb.guarded(B, (code.output_len(),), np.uint8, 8 if on_device else 1, device, name="output")
    it, g_it = gb.guarded(B, (), np.int32 if on_device else np.uint32, 4, device, name="iters", prefill=-2 if on_device else 0xFFFFFFFE)
    ok, g_ok = gb.guarded(B, (), np.uint8, 1, device, name="success")
    stage, g_stage = gb.guarded(B, (), np.uint8, 1, device, name="stage")
    method = code.decode_ms_cascade_soft_batch if dtype == np.float32 else code.decode_ms_cascade_fixed_soft_batch
    res = method(llrs, *csr.CAPS[0], app=app, output=out, iters=it, success=ok, stage=stage)
    if on_device:
        torch.cuda.synchronize()
        res = to_numpy(res)
    same_soft(res, want, "guarded rows")
    for g in (g_llrs, g_app, g_out, g_it, g_ok, g_stage):
        g.check()
    keep.check()


def raw_call(code, dtype, ptrs, batch, stream):
    suf = {np.float32: "f32", np.int8: "i8", np.int16: "i16"}[dtype]
    fn = getattr(la.lib, "labrador_ldpc_decode_ms_cascade_soft_batch_" + suf)
    opts = la.HipOpts(0, la.MEM_DEVICE, stream, 0, 0, None)
    tail = (1.0, 0.0, 1.0, 0.0) if dtype == np.float32 else (1, 0, 0)
    return fn(int(code), *ptrs, batch, *csr.CAPS[0], *tail, ctypes.byref(opts))


@pytest.mark.parametrize("dtype", (np.float32, np.int8), ids=lambda t: np.dtype(t).name)
def test_misaligned_device_app_is_refused(dtype):
    """A device `app` 4 bytes off a 16-byte boundary is EINVAL with the alignment text, and nothing is written."""
    import torch
    code, B = LDPCCode.TM1280, 17
    V = code.n() + code.punctured_bits()
    d = torch.from_numpy(np.array(csr.frames(code, dtype)[:B])).cuda()
    wide = torch.full((B * V * 4 + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    out = torch.full((B, code.output_len()), 0xEE, dtype=torch.uint8, device="cuda")
    it = torch.full((B,), -2, dtype=torch.int32, device="cuda")
    ok, stage = (torch.full((B,), 7, dtype=torch.uint8, device="cuda") for _ in range(2))
    assert wide.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    st = raw_call(code, dtype, (d.data_ptr(), wide.data_ptr() + 4, out.data_ptr(), it.data_ptr(), ok.data_ptr(), stage.data_ptr()), B,
                  torch.cuda.current_stream().cuda_stream)
    assert st == EINVAL and "app buffer must be 16-byte aligned" in la.last_error()
    torch.cuda.synchronize()
    assert bool((wide == 0xEE).all()) and bool((out == 0xEE).all()) and bool((it == -2).all()) and bool((ok == 7).all()) and bool((stage == 7).all())


@pytest.mark.parametrize("dtype", (np.float32, np.int8), ids=lambda t: np.dtype(t).name)
def test_streams_and_device_sets(dtype):
    """A caller's stream, synchronised once; two calls back to back on two streams of one thread and a third on the first again --
    the later ones' widen block, list and dense rows reuse the workspace the earlier ones' are still using; devices=[0, 0]."""
    import torch
    code = LDPCCode.TM1280
    caps = csr.CAPS[0]
    llrs = csr.frames(code, dtype)
    want = plain_reference(code, dtype, caps)
    method = code.decode_ms_cascade_soft_batch if dtype == np.float32 else code.decode_ms_cascade_fixed_soft_batch
    cuts = ((0, 151), (20, 131), (60, 100))
    d = [torch.from_numpy(np.array(llrs[a:b])).cuda() for a, b in cuts]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    with torch.cuda.stream(streams[0]):
        got = method(d[0], *caps, stream=streams[0].cuda_stream)
    streams[0].synchronize()
    same_soft(to_numpy(got), want, "a caller's stream")
    got = []
    for i, x in enumerate(d):
        s = streams[i % 2]
        with torch.cuda.stream(s):
            got.append(method(x, *caps, stream=s.cuda_stream))
    for s in streams:
        s.synchronize()
    for g, (a, b) in zip(got, cuts):
        same_soft(to_numpy(g), tuple(x[a:b] for x in want), f"two streams, frames {a} .. {b}")
    same_soft(soft_cascade(code, llrs, *caps, devices=[0, 0]), want, "devices=[0, 0]")
