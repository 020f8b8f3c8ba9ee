"""Where the min-sum decoders write (tests/guarded_buffers.py): every result array of every call is a view into the middle of a larger
allocation with a guard band on either side, placed at the LEAST alignment the header admits for it, and the input is kept for
comparison.  After the call every result row equals the reference's exactly (the oracle for the flooding kernels, the committed
restatements for the layered families, the definitions for the LLR conversions -- never a second call of the library), every band
still holds its fill, and the input is byte for byte what it was.

Batch sizes 1, 3, 5, 9, 17 and 33 are one more than a power of two: for every codeword-group size from 2 to 32 the last group then has
exactly one live slot (1 serves a group of one), and 15 leaves one dead slot.  The frames of a batch come from a pool of eight per
(code, LLR type) -- two codewords, two that converge after a few iterations, two of noise, and two special ones (floats: a NaN at
index n - 1, every seventh LLR +inf; integers: the type's minimum everywhere, full scale of random sign) -- decoded once by the
reference.

Sections: A the flooding kernels, every variant, hard and soft; B flooding from an `llrs` base one element past a 16-byte boundary (and
the i8 dispatch's fallback from the bit-sliced kernel); C the two launches of the register-lean kernels' NaN handling; D the layered,
fixed-point, fused quantised and cascade entries and the LLR conversions; E device batches cut into launch slices, whose fourth output
`app` has an element size of its own; F host batches through the chunked staging pipeline with four outputs."""
import numpy as np
import pytest

import guarded_buffers as gb
import labrador_ldpc_amd as la
import layered_corrected_restatement as lcr
import layered_fixed_corrected_restatement as fcr
import layered_fixed_restatement as fr
import layered_restatement as lr
import oracle
import quantise_restatement as qr
import quantised_layered_restatement as qlr
from kernel_inventory import F32_VARIANTS, F64_IN_PLACE, F64_VARIANTS
from labrador_ldpc_amd import LDPCCode, LdpcHipError
from layered_helpers import structure

pytestmark = pytest.mark.gpu

ALL = list(LDPCCode)
TM = [c for c in ALL if c.name.startswith("TM")]
CAP = 12
SIZES = (1, 3, 5, 9, 15, 17, 33)
DTYPES = [np.float32, np.float64, np.int8, np.int16, np.int32]
# integer scales and limits as in tests/test_gpu_parity.py
INT_SCALE = {np.dtype(np.int8): (8.0, 31), np.dtype(np.int16): (64.0, 4095), np.dtype(np.int32): (3e8, 2 ** 31 - 1)}
QUANT = {np.dtype(np.int8): ("i8", 8.0, 31), np.dtype(np.int16): ("i16", 64.0, 4095)}
TRIPLE = (13, 4, 0)
PAIR = (0.8125, 0.0)
# base of each result view, bytes past a 16-byte boundary: output 8 mod 16, iters 4 mod 8, success and stage odd, app 0 mod 16
LEAD = {"output": 8, "iters": 4, "success": 1, "stage": 1, "app": 0}
BS, STATIC = 64, 256
CLEAN, CONVERGING, NOISE, SPECIAL_A, SPECIAL_B = (0, 1), (2, 3), (4, 5), 6, 7          # pool indices by kind

ids_of = lambda v: v.name if isinstance(v, LDPCCode) else np.dtype(v).name if isinstance(v, type) else str(v)     # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if la.device_count() < 1 or not torch.cuda.is_available():
        pytest.fail("the containment tests need a gfx950 device")
    torch.cuda.set_device(0)


# ---------------------------------------------------------------------------------------------------------------- frames and references

_POOLS, _REFS = {}, {}


def frame_pool(code, dtype):
    """The eight frames of (code, dtype), by kind: [0, 1] codewords already (30 dB), [2, 3] converging after a few iterations, [4, 5]
    noise alone, [6] and [7] the special ones.  Which candidate frames are the converging ones is decided by the oracle."""
    dt = np.dtype(dtype)
    key = (code, dt)
    if key in _POOLS:
        return _POOLS[key]
    rng = np.random.default_rng(0xC0DE + 16 * int(code) + DTYPES.index(dt.type))
    n = code.n()
    kw = dict(zip(("scale", "lim"), INT_SCALE[dt])) if dt.kind == "i" else {}
    clean = oracle.awgn_llrs(code, rng, 2, 30.0, dt, **kw)[0]
    cand = oracle.awgn_llrs(code, rng, 32, {0: 5.0, 1: 4.5, 2: 4.0}.get(int(code), 3.5), dt, **kw)[0]
    r = oracle.decode_ms_batch(code, cand, CAP)
    late = np.flatnonzero((r[2] == 1) & (r[1] >= 2))
    assert late.size >= 4, f"{code.name} {dt}: too few candidate frames converge after a few iterations"
    if dt.kind == "f":
        noise = (2.0 * rng.standard_normal((2, n))).astype(dt)
        a, b = cand[late[2]].copy(), cand[late[3]].copy()
        a[n - 1] = np.nan
        b[::7] = np.inf
    else:
        info = np.iinfo(dt)
        lim = INT_SCALE[dt][1]
        noise = rng.integers(-lim, lim, (2, n), endpoint=True).astype(dt)
        a = np.full(n, info.min, dt)
        b = np.where(rng.random(n) < 0.5, info.max, info.min).astype(dt)
    pool = np.ascontiguousarray(np.concatenate([clean, cand[late[:2]], noise, a[None], b[None]]))
    pool.setflags(write=False)
    _POOLS[key] = pool
    return pool


class Ref:
    """A reference's results for a pool, by name, with a copy on the device made on first use."""

    def __init__(self, output, iters, success, app=None, stage=None):
        self.host = {"output": output, "iters": np.ascontiguousarray(iters).astype(np.int32), "success": success}
        if app is not None:
            self.host["app"] = app
        if stage is not None:
            self.host["stage"] = stage
        for v in self.host.values():
            v.setflags(write=False)
        self._dev = None

    def rows(self, idx, names, device):
        if device is None:
            return {k: self.host[k][idx] for k in names}
        import torch
        if self._dev is None:
            self._dev = {k: torch.from_numpy(np.array(v)).cuda() for k, v in self.host.items()}
        i = torch.from_numpy(np.asarray(idx, dtype=np.int64)).cuda()
        return {k: self._dev[k][i] for k in names}


def reference(kind, code, dtype):
    """The reference of entry family `kind` on the pool of (code, dtype), computed once per module."""
    dt = np.dtype(dtype)
    key = (kind, code, dt)
    if key in _REFS:
        return _REFS[key]
    if kind == "flooding":
        out, it, ok, va = oracle.decode_ms_soft_batch(code, frame_pool(code, dt), CAP)
        r = Ref(out, it, ok, va)
    elif kind == "layered":
        r = Ref(*lr.decode_layered(structure(code), frame_pool(code, np.float32), CAP)[:4])
    elif kind == "layered_corrected":
        r = Ref(*lcr.decode_layered_corrected(structure(code), frame_pool(code, np.float32), CAP, *PAIR)[:4])
    elif kind == "fixed":
        r = Ref(*fr.decode_fixed(structure(code, fr.Structure), frame_pool(code, dt), CAP)[:4])
    elif kind == "fixed_corrected":
        r = Ref(*fcr.decode_fixed_corrected(structure(code, fr.Structure), frame_pool(code, dt), CAP, *TRIPLE)[:4])
    elif kind == "quantised":                                # dt: the integer type the f32 pool is decoded through
        r = Ref(*qr.decode_quantised(code, frame_pool(code, np.float32), dt.type, *QUANT[dt][1:], CAP))
    elif kind == "layered_quantised":
        r = Ref(*qlr.layered_quantised(code, frame_pool(code, np.float32), dt.type, *QUANT[dt][1:], CAP, TRIPLE)[:4])
    elif kind == "cascade_quantised":
        out, it, ok, stage = qlr.cascade_quantised(code, frame_pool(code, np.float32), dt.type, *QUANT[dt][1:], CAP, CAP, TRIPLE)
        r = Ref(out, it, ok, stage=stage)
    else:
        raise KeyError(kind)
    _REFS[key] = r
    return r


def batch_indices(B, pool_len=8):
    """Pool indices of a batch of B frames.  (j * 3 + B // 2) mod 8 walks every kind, and the kind of the LAST frame varies with B:
    over SIZES it is a codeword, a failing frame and special frame 6 at least once each (test_the_last_frame_varies)."""
    return (np.arange(B) * 3 + B // 2) % pool_len


def test_the_last_frame_varies():
    """What the sizes are chosen for, asserted and not assumed: over SIZES the last frame of a batch is a failing frame, a frame that
    is done at the first verdict and the NaN frame (integers: the frame of the type's minimum) at least once each -- for every type on
    a packed code, a register-lean code and a pair-kernel code -- and the pool's kinds are what their names say."""
    last = {int(batch_indices(B)[-1]) for B in SIZES}
    assert last & set(NOISE) and last & set(CLEAN) and SPECIAL_A in last, last
    for code in (LDPCCode.TC128, LDPCCode.TM1280, LDPCCode.TM8192):
        for dtype in DTYPES:
            pool, ref = frame_pool(code, dtype), reference("flooding", code, dtype).host
            it, ok = ref["iters"], ref["success"]
            assert (ok[list(CLEAN)] == 1).all() and (it[list(CLEAN)] <= (1 if code.punctured_bits() else 0)).all(), (code, dtype, it)
            assert (ok[list(CONVERGING)] == 1).all() and (it[list(CONVERGING)] >= 2).all(), (code, dtype, it)
            assert (ok[list(NOISE)] == 0).all() and (it[list(NOISE)] == CAP).all(), (code, dtype, it)
            if np.dtype(dtype).kind == "f":
                assert np.isnan(pool[SPECIAL_A, code.n() - 1]) and np.isnan(pool).sum() == 1 and np.isinf(pool[SPECIAL_B, ::7]).all()
                assert np.isnan(ref["app"][SPECIAL_A, code.n() - 1]) and np.isnan(ref["app"]).sum() == 1
            else:
                assert (pool[SPECIAL_A] == np.iinfo(dtype).min).all() and (np.abs(pool[SPECIAL_B].astype(np.int64)) >= np.iinfo(dtype).max).all()
            lasts = [int(batch_indices(B)[-1]) for B in SIZES]
            assert any(not ok[i] for i in lasts) and any(ok[i] and it[i] <= 1 for i in lasts) and SPECIAL_A in lasts


# ---------------------------------------------------------------------------------------------------------------- one guarded call

def _differing_rows(got, want):
    """Indices of the rows of `got` that differ from `want` (both numpy or both torch; floats as values, NaN where NaN)."""
    torch_like = gb._is_torch(got)
    if torch_like:
        import torch
        xp_isnan, floating = torch.isnan, got.dtype.is_floating_point
    else:
        xp_isnan, floating = np.isnan, got.dtype.kind == "f"
    if floating:
        na, nb = xp_isnan(got), xp_isnan(want)
        bad = (na != nb) | (~na & ~nb & (got != want))
    else:
        bad = got != want
    if bad.ndim > 1:
        bad = bad.reshape(bad.shape[0], -1).any(1) if not torch_like else bad.reshape(bad.shape[0], -1).any(dim=1)
    if not bool(bad.any()):
        return []
    return [int(i) for i in (bad.nonzero().reshape(-1) if torch_like else np.flatnonzero(bad))[:8]]


def guarded_call(tag, call, llrs, want, *, llrs_lead=0, device="cuda", app_dtype=None, iters_prefill=-2, refused=False):
    """`call(llrs_view, **result_views)` with every result named in `want` (name -> expected rows) a guarded view at its least
    alignment and `llrs` (numpy [B, n]) copied into a guarded view `llrs_lead` bytes past a 16-byte boundary.  After ONE synchronise:
    every row equals `want`, every band holds, the input is unchanged.  refused=True: the call must answer EUNSUPPORTED instead, and
    then have written nothing at all."""
    B = len(llrs)
    x, gx = gb.guarded_copy(llrs, llrs_lead, device, name="llrs")
    keep = gb.frozen(x, "llrs")
    views, guards = {}, [gx]
    for name, rows in want.items():
        dtype = (app_dtype or llrs.dtype) if name == "app" else np.int32 if name == "iters" else np.uint8
        views[name], g = gb.guarded(B, tuple(rows.shape[1:]), dtype, LEAD[name], device, name=name, app=name == "app",
                                    prefill=iters_prefill if name == "iters" else None)
        guards.append(g)
    if device is not None:
        import torch
        torch.cuda.synchronize()
    if refused:
        with pytest.raises(LdpcHipError, match="status -4"):
            call(x, **views)
    else:
        call(x, **views)
    if device is not None:
        torch.cuda.synchronize()
    problems = []
    for name, rows in want.items():
        if refused:
            raw = views[name].reshape(-1).view(torch.uint8 if device is not None else np.uint8)
            fill = 0xEE if name != "iters" else None
            if fill is not None and not bool((raw == fill).all()):
                problems.append(f"{name}: a refused call wrote into the view")
            continue
        bad = _differing_rows(views[name], rows)
        if bad:
            problems.append(f"{name}: rows {bad} of {B} differ from the reference")
    for g in guards:
        try:
            g.check()
        except AssertionError as e:
            problems.append(str(e))
    try:
        keep.check()
    except AssertionError as e:
        problems.append(str(e))
    assert not problems, f"{tag}, {B} frames: " + "; ".join(problems)
    return views


def pool_call(tag, call, kind, code, dtype, B, names, *, pool_dtype=None, idx=None, **kw):
    """guarded_call on a batch of B pool frames against reference(kind, code, dtype)."""
    idx = batch_indices(B) if idx is None else idx
    device = kw.get("device", "cuda")
    pool = frame_pool(code, pool_dtype or dtype)
    want = reference(kind, code, dtype).rows(idx, names, device)
    return guarded_call(tag, call, pool[idx], want, **kw)


HARD = ("output", "iters", "success")
SOFT = ("app",) + HARD


# ---------------------------------------------------------------------------------------------------------------- A

def flooding_variants(code, dtype):
    """(variants to try, those of them that must run) for the hard-only flooding call."""
    dt = np.dtype(dtype)
    if dt == np.float32:
        return F32_VARIANTS[code], F32_VARIANTS[code]
    if dt == np.float64:
        return F64_VARIANTS[code] + F64_IN_PLACE[code], F64_VARIANTS[code] + F64_IN_PLACE[code]
    if dt == np.int8:
        v = (0, 32 if code == LDPCCode.TM8192 else 1, STATIC)
        if code in TM:
            v += (BS,)
        if code in (LDPCCode.TM1536, LDPCCode.TM1280):
            v += (BS | STATIC,)
        return v, (0, STATIC) + ((BS,) if code in TM else ()) + ((BS | STATIC,) if BS | STATIC in v else ())
    v = (0, STATIC) + ((2,) if 2 in F32_VARIANTS[code] else ()) + ((32,) if code in (LDPCCode.TM8192, LDPCCode.TM2048) else ())
    return v, (0, STATIC)


def soft_refuses(code, dtype, variant):
    """The soft call's refusals as the header lists them: the bit-sliced i8 kernels and the in-place f64 ones keep no marginals."""
    dt = np.dtype(dtype)
    return (dt == np.int8 and variant & ~STATIC == BS) or (dt == np.float64 and variant in F64_IN_PLACE[code])


COUNTS = {}                                                   # (section, family) -> [ran, skipped as unsupported]


def count(section, ran, skipped=0):
    c = COUNTS.setdefault(section, [0, 0])
    c[0] += ran
    c[1] += skipped
    print(f"containment inventory: {section}: {c[0]} (code, type, variant, form) combinations ran, {c[1]} skipped as unsupported")


def hard_call(code, variant):
    return lambda x, **r: code.decode_ms_batch(x, CAP, variant=variant, **r)


def soft_call(code, variant):
    return lambda x, **r: code.decode_ms_soft_batch(x, CAP, variant=variant, **r)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_of)
@pytest.mark.parametrize("code", ALL, ids=ids_of)
def test_flooding_every_kernel(code, dtype):
    """Every variant the hard-only call accepts for (code, type), hard and soft, at every size.  `llrs` and `app` keep 16 bytes;
    `output` is at 8 mod 16, `iters` at 4 mod 8, `success` at an odd address."""
    variants, required = flooding_variants(code, dtype)
    ran, skipped = [], []
    for variant in variants:
        tag = f"{code.name} {np.dtype(dtype).name} variant {variant}"
        try:
            pool_call(tag + " hard", hard_call(code, variant), "flooding", code, dtype, SIZES[0], HARD)
        except LdpcHipError as e:
            assert "status -4" in str(e) and variant not in required, f"{tag}: {e}"
            skipped.append(variant)
            continue
        for B in SIZES[1:]:
            pool_call(tag + " hard", hard_call(code, variant), "flooding", code, dtype, B, HARD)
        ran.append((variant, "hard"))
        if soft_refuses(code, dtype, variant):
            pool_call(tag + " soft (refused)", soft_call(code, variant), "flooding", code, dtype, 5, SOFT, refused=True)
            continue
        for B in SIZES:
            pool_call(tag + " soft", soft_call(code, variant), "flooding", code, dtype, B, SOFT)
        ran.append((variant, "soft"))
    assert all((v, "hard") in ran for v in required), f"{code.name} {np.dtype(dtype).name}: ran {ran}, skipped {skipped}"
    assert all((v, "soft") in ran for v in required if not soft_refuses(code, dtype, v))
    if np.dtype(dtype) == np.int8 and code in TM:
        assert sum(1 for v, form in ran if v & ~STATIC == BS) >= 1, "no bit-sliced kernel ran"
    count(f"A flooding {np.dtype(dtype).name}", len(ran), 2 * len(skipped))


# ---------------------------------------------------------------------------------------------------------------- B

B_CODES = [LDPCCode.TC128, LDPCCode.TM1280, LDPCCode.TM2048, LDPCCode.TM5120, LDPCCode.TM8192]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_of)
@pytest.mark.parametrize("code", B_CODES, ids=ids_of)
def test_flooding_from_an_element_aligned_llrs(code, dtype):
    """The header asks of a device `llrs` only its element's alignment: the base one element past a 16-byte boundary, default kernel
    and fixed stride, hard and soft."""
    lead = np.dtype(dtype).itemsize
    for variant in (0, STATIC):
        tag = f"{code.name} {np.dtype(dtype).name} variant {variant} llrs at {lead} mod 16"
        for B in SIZES:
            pool_call(tag + " hard", hard_call(code, variant), "flooding", code, dtype, B, HARD, llrs_lead=lead)
            pool_call(tag + " soft", soft_call(code, variant), "flooding", code, dtype, B, SOFT, llrs_lead=lead)
    count(f"B element-aligned llrs {np.dtype(dtype).name}", 4)


def smallest_bitsliced_batch(code):
    """The smallest batch for which the library names a bit-sliced kernel for the default dispatch of i8 (0: never)."""
    name = lambda b: la.lib.labrador_ldpc_hip_decode_ms_i8_kernel(int(code), 0, b).decode()      # noqa: E731
    hi = 1 << 20
    if not name(hi).startswith("decode_ms_bs"):
        return 0
    lo = 0                                                    # name(lo) is not bit-sliced, name(hi) is
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if name(mid).startswith("decode_ms_bs") else (mid, hi)
    return hi


def test_no_bitsliced_kernel_for_the_tc_codes():
    assert smallest_bitsliced_batch(LDPCCode.TC128) == 0 and all(smallest_bitsliced_batch(c) > 0 for c in TM)


@pytest.mark.parametrize("code", [c for c in B_CODES if c in TM], ids=ids_of)
def test_i8_fallback_from_the_bitsliced_kernel_for_an_odd_llrs(code):
    """At the smallest batch the default dispatch decodes on the bit-sliced kernel, whose loads are dwords, an `llrs` at an odd address
    must fall back to the f32-pipe kernel and return the oracle's bytes; the same frames from an aligned base too."""
    B = smallest_bitsliced_batch(code)
    assert B > 1 and la.lib.labrador_ldpc_hip_decode_ms_i8_kernel(int(code), 0, B).decode().startswith("decode_ms_bs")
    assert not la.lib.labrador_ldpc_hip_decode_ms_i8_kernel(int(code), 0, B - 1).decode().startswith("decode_ms_bs")
    idx = batch_indices(B)
    for lead in (0, 1):
        pool_call(f"{code.name} i8 default dispatch, llrs at {lead} mod 16", hard_call(code, 0), "flooding", code, np.int8, B, HARD, idx=idx,
                  llrs_lead=lead)
    count("B i8 bit-sliced fallback", 2)


# ---------------------------------------------------------------------------------------------------------------- C

@pytest.mark.parametrize("variant", [512, 1024])
@pytest.mark.parametrize("code", [LDPCCode.TM5120, LDPCCode.TM1280], ids=ids_of)
def test_two_launches_per_call(code, variant):
    """The register-lean f32 kernels mark a codeword with a NaN in `iters` (0xFFFFFFFF) for a second launch: the NaN frame first, last
    and both, `iters` prefilled with the mark itself -- no mark may survive in the view and none may appear in a band."""
    import torch
    others = np.array([i for i in range(8) if i != SPECIAL_A])
    for B in (1, 2, 17):
        for where in ({0}, {B - 1}, {0, B - 1}):
            idx = others[(np.arange(B) * 3 + B // 2) % len(others)]
            idx[list(where)] = SPECIAL_A
            for names, call in ((HARD, hard_call(code, variant)), (SOFT, soft_call(code, variant))):
                views = pool_call(f"{code.name} f32 variant {variant} NaN frame at {sorted(where)} {'soft' if 'app' in names else 'hard'}",
                                  call, "flooding", code, np.float32, B, names, idx=idx, iters_prefill=-1)
                assert not bool((views["iters"] == -1).any()), "a NaN mark survived in iters"
    torch.cuda.synchronize()
    count("C two NaN launches f32", 2)


# ---------------------------------------------------------------------------------------------------------------- D

D_CODES = [LDPCCode.TC128, LDPCCode.TC256, LDPCCode.TM1536, LDPCCode.TM8192]


def other_entries(code):
    """(name, call, result names, reference kind, reference dtype, pool dtype, bytes `llrs` is past 16, app dtype): `llrs` at the least
    alignment the entry's header paragraph admits -- its element where the paragraph says so, 16 bytes where it asks for them."""
    E = []
    E.append(("layered f32 hard", lambda x, **r: code.decode_ms_layered_batch(x, CAP, **r), HARD, "layered", np.float32, np.float32, 4, None))
    E.append(("layered f32 soft", lambda x, **r: code.decode_ms_layered_soft_batch(x, CAP, **r), SOFT, "layered", np.float32, np.float32, 4, None))
    E.append(("layered corrected f32 hard", lambda x, **r: code.decode_ms_layered_batch(x, CAP, scale=PAIR[0], offset=PAIR[1], **r), HARD,
              "layered_corrected", np.float32, np.float32, 4, None))
    E.append(("layered corrected f32 soft", lambda x, **r: code.decode_ms_layered_soft_batch(x, CAP, scale=PAIR[0], offset=PAIR[1], **r), SOFT,
              "layered_corrected", np.float32, np.float32, 4, None))
    t = dict(zip(("scale_num", "scale_shift", "offset"), TRIPLE))
    for dt in (np.int8, np.int16):
        suf, scale, lim = QUANT[np.dtype(dt)]
        E.append((f"layered fixed corrected {suf} hard", lambda x, **r: code.decode_ms_layered_fixed_batch(x, CAP, **t, **r), HARD,
                  "fixed_corrected", dt, dt, np.dtype(dt).itemsize, None))
        E.append((f"layered fixed corrected {suf} soft", lambda x, **r: code.decode_ms_layered_fixed_soft_batch(x, CAP, **t, **r), SOFT,
                  "fixed_corrected", dt, dt, np.dtype(dt).itemsize, np.int32))
        q = dict(dtype=suf, scale=scale, lim=lim, maxiters=CAP)
        E.append((f"quantised flooding {suf}", lambda x, q=q, **r: code.decode_ms_quantised_batch(x, **q, **r), HARD,
                  "quantised", dt, np.float32, 0, None))
        E.append((f"layered quantised {suf} hard", lambda x, q=q, **r: code.decode_ms_layered_quantised_batch(x, **q, **t, **r), HARD,
                  "layered_quantised", dt, np.float32, 4, None))
        E.append((f"layered quantised {suf} soft", lambda x, q=q, **r: code.decode_ms_layered_quantised_soft_batch(x, **q, **t, **r), SOFT,
                  "layered_quantised", dt, np.float32, 4, np.int32))
        E.append((f"cascade quantised {suf}", lambda x, q=q, **r: code.decode_ms_cascade_quantised_batch(x, **q, max_sweeps=CAP, **t, **r),
                  HARD + ("stage",), "cascade_quantised", dt, np.float32, 0, None))
    return E


@pytest.mark.parametrize("entry", range(16), ids=[e[0].replace(" ", "-") for e in other_entries(LDPCCode.TC128)])
@pytest.mark.parametrize("code", D_CODES, ids=ids_of)
def test_the_other_decoders(code, entry):
    """The layered f32 entries, their corrected forms at (0.8125, 0.0), the fixed-point layered entries at (13, 4, 0), the fused
    quantised flooding, layered and cascade entries (`stage` guarded too): the same guards, placements and sizes."""
    name, call, names, kind, ref_dtype, pool_dtype, lead, app_dtype = other_entries(code)[entry]
    for B in SIZES:
        pool_call(f"{code.name} {name}", call, kind, code, ref_dtype, B, names, pool_dtype=pool_dtype, llrs_lead=lead, app_dtype=app_dtype)
    count(f"D {name.rsplit(' ', 1)[0] if name.endswith(('hard', 'soft')) else name}", 1)


def test_the_other_decoders_see_every_kind_of_frame():
    """The layered references on the pools are not all of one kind: frames that succeed and frames that fail, and a second stage that
    is taken and one that is not."""
    for code in D_CODES:
        for kind, dt in (("layered", np.float32), ("layered_corrected", np.float32), ("fixed_corrected", np.int8), ("fixed_corrected", np.int16),
                         ("quantised", np.int8), ("layered_quantised", np.int16)):
            ok = reference(kind, code, dt).host["success"]
            assert ok.any() and not ok.all(), (code, kind)
        stage = reference("cascade_quantised", code, np.int8).host["stage"]
        assert stage.any() and not stage.all(), code


LLR_DT = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "f32": np.float32, "f64": np.float64}


@pytest.mark.parametrize("dt", list(LLR_DT))
@pytest.mark.parametrize("code", [LDPCCode.TC128, LDPCCode.TM8192], ids=ids_of)
def test_llr_conversions(code, dt):
    """hard_to_llrs_batch into a guarded `llrs` (16 bytes, as the header asks) and llrs_to_hard_batch into a guarded `output` at an odd
    address (the entry checks only its `llrs`), against the definitions of tests/test_llr_batch.py."""
    import torch
    from test_llr_batch import _bits, _corner_llrs, _expected_llrs
    dtype = LLR_DT[dt]
    for B in (1, 3, 1000):
        bits = _bits(code, B, 11 + B)
        d_bits, g_bits = gb.guarded_copy(bits, 1, "cuda", name="bits")
        keep_bits = gb.frozen(d_bits, "bits")
        llrs, g_llrs = gb.guarded(B, (code.n(),), dtype, 0, "cuda", name="llrs")
        x = _corner_llrs(code, B, dtype, 13 + B)
        d_x, g_x = gb.guarded_copy(x, 0, "cuda", name="llrs (input)")
        keep_x = gb.frozen(d_x, "llrs (input)")
        out, g_out = gb.guarded(B, (code.n() // 8,), np.uint8, 1, "cuda", name="output")
        torch.cuda.synchronize()
        code.hard_to_llrs_batch(d_bits, dt, llrs=llrs)
        code.llrs_to_hard_batch(d_x, output=out)
        torch.cuda.synchronize()
        assert torch.equal(llrs, torch.from_numpy(_expected_llrs(bits, dtype)).cuda()), f"{code.name} {dt} {B}: hard_to_llrs_batch"
        assert torch.equal(out, torch.from_numpy(np.packbits(x < 0, axis=1)).cuda()), f"{code.name} {dt} {B}: llrs_to_hard_batch"
        for c in (g_bits, g_llrs, g_x, g_out, keep_bits, keep_x):
            c.check()
    count("D llr_convert", 2)


# ---------------------------------------------------------------------------------------------------------------- E

def sliced_entries():
    """(name, code, call, reference kind, reference dtype, pool dtype, llrs lead, app dtype): soft entries whose `app` differs in element
    size from the LLRs (int32 from int8 / from f32 quantised to int16) or not."""
    c1, c2, c3 = LDPCCode.TM1280, LDPCCode.TC128, LDPCCode.TC256
    suf, scale, lim = QUANT[np.dtype(np.int16)]
    t = dict(zip(("scale_num", "scale_shift", "offset"), TRIPLE))
    return [("flooding f32 TM1280", c1, soft_call(c1, 0), "flooding", np.float32, np.float32, 4, None),
            ("flooding i8 TC128", c2, soft_call(c2, 0), "flooding", np.int8, np.int8, 1, None),
            ("layered f32 TC256", c3, lambda x, **r: c3.decode_ms_layered_soft_batch(x, CAP, **r), "layered", np.float32, np.float32, 4, None),
            ("layered fixed i8 TM1280", c1, lambda x, **r: c1.decode_ms_layered_fixed_soft_batch(x, CAP, **r), "fixed", np.int8, np.int8, 1, np.int32),
            ("layered fixed i8 TC128", c2, lambda x, **r: c2.decode_ms_layered_fixed_soft_batch(x, CAP, **r), "fixed", np.int8, np.int8, 1, np.int32),
            ("layered quantised i16 TM1280", c1,
             lambda x, **r: c1.decode_ms_layered_quantised_soft_batch(x, dtype=suf, scale=scale, lim=lim, maxiters=CAP, **t, **r),
             "layered_quantised", np.int16, np.float32, 4, np.int32)]


@pytest.mark.parametrize("entry", range(6), ids=[e[0].replace(" ", "-") for e in sliced_entries()])
def test_launch_slices_carry_the_fourth_output(entry, monkeypatch):
    """LABRADOR_LDPC_HIP_MAX_LAUNCH=16 cuts device batches of 16, 17 and 40 frames into one, two and three launches; the offset of each
    slice into `app` is in ITS element size.  The same frames without the variable: both runs equal the reference."""
    name, code, call, kind, ref_dtype, pool_dtype, lead, app_dtype = sliced_entries()[entry]
    for B in (16, 17, 40):
        with monkeypatch.context() as m:
            m.setenv("LABRADOR_LDPC_HIP_MAX_LAUNCH", "16")
            pool_call(f"{name}, slices of 16", call, kind, code, ref_dtype, B, SOFT, pool_dtype=pool_dtype, llrs_lead=lead, app_dtype=app_dtype)
        pool_call(f"{name}, one launch", call, kind, code, ref_dtype, B, SOFT, pool_dtype=pool_dtype, llrs_lead=lead, app_dtype=app_dtype)
    count("E sliced soft entries", 1)


# ---------------------------------------------------------------------------------------------------------------- F

def chunked_entries():
    code = LDPCCode.TM1280
    return [("flooding f32", soft_call(code, 0), "flooding", np.float32, None),
            ("flooding i8", soft_call(code, 0), "flooding", np.int8, None),
            ("layered fixed i8", lambda x, **r: code.decode_ms_layered_fixed_soft_batch(x, CAP, **r), "fixed", np.int8, np.int32),
            ("layered f32", lambda x, **r: code.decode_ms_layered_soft_batch(x, CAP, **r), "layered", np.float32, None)]


@pytest.mark.parametrize("frames,devices", [(300, None), (301, None), (600, None), (1501, None), (1501, [0, 0])],
                         ids=["300", "301", "600", "1501", "1501-two-pipelines"])
@pytest.mark.parametrize("entry", range(4), ids=[e[0].replace(" ", "-") for e in chunked_entries()])
def test_four_outputs_through_the_chunked_host_pipeline(entry, frames, devices, monkeypatch):
    """LABRADOR_LDPC_HIP_CHUNK=300: host batches of one chunk, one chunk and a frame, two chunks and five and a frame go through the
    staging pipeline with `app` -- the largest buffer of the call -- as the fourth output; once more over two pipelines of one
    device.  numpy result views with guard bands; `llrs` unchanged."""
    name, call, kind, dtype, app_dtype = chunked_entries()[entry]
    monkeypatch.setenv("LABRADOR_LDPC_HIP_CHUNK", "300")
    run = call if devices is None else (lambda x, **r: call(x, devices=devices, **r))
    pool_call(f"TM1280 {name} host, chunks of 300" + (f", devices {devices}" if devices else ""), run, kind, LDPCCode.TM1280, dtype, frames,
              SOFT, device=None, app_dtype=app_dtype, llrs_lead=np.dtype(dtype).itemsize)
    if frames == 1501:
        count("F chunked host pipeline", 1)
