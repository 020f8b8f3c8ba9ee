"""entry_table.py -- the table of the library's batched entries, their small input pools and their CPU statements, shared by the
graph-capture tests (tests/test_gpu_graph_capture.py) and the route tests (tests/call_routes.py, tests/test_call_routes_host.py,
tests/test_gpu_call_routes.py).  TEST INFRASTRUCTURE ONLY.  Importing it touches no GPU.

  * the pools: pool_of() mixes converging, failing and edge-valued frames of an LLR type; small_pool() is the 8 (6) frames of a code
    and type, small_values() what the reference decodes of them; windows() walks a pool in consecutive index sets;
  * decode_reference() / small_reference(): each kernel family's CPU statement (tests/oracle.py and the restatements);
  * Entry / entries(): the MEM_DEVICE entries that may be captured into a graph, on the codes the graph-capture tests run;
    streaming_cases(): the streaming kernels' cases of those tests;
  * RouteEntry / route_entries(): EVERY batched symbol of the header that runs on the one batched call path (csrc/capi_frame.hpp),
    once on the smallest code it has a kernel for -- the bit-sliced ones on TM1536 as well, whose group of 8 codewords meets a launch
    slice of 8 exactly -- with its Python call, its result names and dtypes, the bytes per item of every buffer as the header states
    the shapes, and its CPU statement on its pool.  EXCLUDED says which batched symbols are not in it and why.

A new batched entry is added to route_entries() once; tests/test_call_routes_host.py fails until it is, and tests/test_gpu_call_routes.py
then runs it on every route."""
import functools

import numpy as np

import bs_hard_frames
import cascade_restatement as cr
import cascade_soft_restatement as cs
import edge_frames
import flooding_corrected_restatement as flc
import flooding_fixed_corrected_soft_restatement as ffs
import hard_frames
import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode
import layered_corrected_restatement as lcr
import layered_fixed_corrected_restatement as fcr
import layered_fixed_restatement as fr
import layered_helpers
import layered_restatement as lr
import oracle
import quantise_restatement as qr
import quantised_layered_restatement as qlr
from test_gpu_half_llrs import round_to, widen
from test_gpu_layered_fixed import codewords_per_workgroup
from test_gpu_quantised_layered import PARAMS as QUANT, edge_rows
from test_gpu_soft_edges import flooding_grid_bound

C = LDPCCode
CAPS = (0, 1, 25)
NP = {"f32": np.float32, "f64": np.float64, "i8": np.int8, "i16": np.int16, "i32": np.int32}
PAIR = (0.8125, 0.125)                                      # (scale, offset) of the f32 corrections on G + 1 frames
TRIPLE = (13, 4, 0)
BS_GROUP = {C.TM1280: 16, C.TM1536: 8, C.TM2048: 4, C.TM5120: 4, C.TM6144: 2, C.TM8192: 1}     # BsPlan<CODE>::G
ONE_WAVE = (C.TM1536, C.TM2048, C.TM6144, C.TM8192)
TWO_WAVES = (C.TM1280, C.TM5120)
BS = 64                                                      # LABRADOR_LDPC_HIP_VARIANT_BITSLICE


# ---- input pools --------------------------------------------------------------------------------------------------------------------------
def awgn(code, rng, frames, ebn0, kind):
    if kind == "i32":
        return oracle.awgn_llrs(code, rng, frames, ebn0, np.int32, scale=3e8, lim=2 ** 31 - 1)[0]
    return oracle.awgn_llrs(code, rng, frames, ebn0, NP.get(kind, np.float32))[0]


def float_extras(code, rng, dt):
    """one frame with NaN LLRs and one with +inf and -inf ones"""
    x = oracle.awgn_llrs(code, rng, 2, 3.0, dt)[0]
    x[0, rng.choice(code.n(), 5, replace=False)] = np.nan
    x[1, ::7] = np.inf
    x[1, 3::11] = -np.inf
    return x


def pool_of(code, kind, each, seed):
    """(frames, kind of each): `each` converging frames at 4 dB (kind 0), `each` at 0 dB that never converge (1), `each` edge-valued
    (2: edge_frames' rows of the type; "q-i8" / "q-i16", f32 for the quantiser at that type's scale: edge_rows of
    tests/test_gpu_quantised_layered.py), and for f32 / f64 a NaN and a +-inf frame (3); interleaved by kind."""
    rng = np.random.default_rng(seed)
    conv, fail = awgn(code, rng, each, 4.0, kind), awgn(code, rng, each, 0.0, kind)
    if kind.startswith("q-"):
        parts = [conv, fail, edge_rows(code, kind[2:], rng, each), float_extras(code, rng, np.float32)]
    elif kind in ("f32", "f64"):
        rows = edge_frames.whole_frame_rows(code, NP[kind], rng)
        parts = [conv, fail, rows[[5, 3, 2, 8, 4, 0, 1, 6, 7][:each]], float_extras(code, rng, NP[kind])]
    else:
        rows = edge_frames.integer_range_rows(code, NP[kind], rng, 3)
        parts = [conv, fail, rows[np.arange(each) * (len(rows) // each) % len(rows)]]
    kinds = np.concatenate([np.full(len(x), k) for k, x in enumerate(parts)])
    order = np.argsort(np.concatenate([np.arange(len(x)) for x in parts]), kind="stable")
    x = np.ascontiguousarray(np.concatenate(parts)[order])
    x.setflags(write=False)
    return x, kinds[order]


@functools.lru_cache(maxsize=None)
def small_pool(code, kind):
    """8 frames (f32, f64, q-*) or 6 (integers) for the G + 1 cases.  "f16" / "bf16": the f32 pool rounded to the format, as
    (bits uint16, kinds); small_values() widens them."""
    if kind in ("f16", "bf16"):
        x, kinds = small_pool(code, "f32")
        with np.errstate(over="ignore"):
            return round_to(x, kind), kinds
    return pool_of(code, kind, 2, 0xCA90 + 64 * int(code) + sorted(list(NP) + ["q-i8", "q-i16"]).index(kind))


def small_values(code, kind):
    """what the reference decodes: the pool, widened where it is halves"""
    x = small_pool(code, kind)[0]
    return widen(x, kind) if kind in ("f16", "bf16") else x


_ST = {}


def flooding_structure(code, module):
    if (module, code) not in _ST:
        _ST[module, code] = module.Structure(int(code)) if module is flc else module.structure(int(code))
    return _ST[module, code]


def decode_reference(family, code, y, cap, params):
    """(output, iters, success, marginals) of `family`'s CPU statement on the frames y"""
    if family == "flooding":
        return oracle.decode_ms_soft_batch(code, y, cap)
    if family == "flooding-corrected":
        return flc.decode_flooding_corrected(flooding_structure(code, flc), y, cap, *params)
    if family == "layered":
        st = layered_helpers.structure(code, lr.Structure)
        return lr.decode_layered(st, y, cap) if params is None else lcr.decode_layered_corrected(st, y, cap, *params)
    if family == "fixed":
        st = layered_helpers.structure(code, fr.Structure)
        return (fr.decode_fixed(st, y, cap) if qlr.identity(params) else fcr.decode_fixed_corrected(st, y, cap, *params))[:4]
    if family == "quantised-layered":
        suf, triple = params
        return qlr.layered_quantised(code, y, NP[suf], *QUANT[suf], cap, triple)[:4]
    if family == "bitsliced":                                # i8 flooding; f32 frames go through the quantiser's statement first
        lim, triple = params
        q = y if y.dtype == np.int8 else qr.quantise(y, np.int8, 8.0, lim)
        if triple is None:
            return oracle.decode_ms_soft_batch(code, q, cap)
        return ffs.decode(flooding_structure(code, ffs), q, cap, *triple)
    raise KeyError(family)


@functools.lru_cache(maxsize=None)
def small_reference(family, code, kind, cap, params):
    ref = decode_reference(family, code, small_values(code, kind), cap, params)
    kinds = small_pool(code, kind)[1]
    if cap == max(CAPS):                                     # the pool still exercises early exit and full-length decodes
        assert ref[2][kinds == 0].all(), (family, code.name, kind, params, "a 4 dB frame fails", ref[2].tolist())
        assert not ref[2][kinds == 1].any(), (family, code.name, kind, params, "a 0 dB frame converges", ref[2].tolist())
        assert (ref[1][kinds == 1] == cap).all()
    return ref


def windows(pool_len, frames):
    """index sets of `frames` consecutive pool entries (wrapping), enough of them to pass through the whole pool, two at the least"""
    count = max(2, -(-pool_len // frames))
    return [np.arange(k * frames, (k + 1) * frames) % pool_len for k in range(count)]


# ---- the entries on G + 1 frames ----------------------------------------------------------------------------------------------------------
class Entry:
    def __init__(self, name, code, kind, g, call, family, params, soft, app="same", note=""):
        self.id = "-".join(x for x in (name, kind, note, code.name) if x)
        self.code, self.kind, self.g, self.call, self.family, self.params, self.soft, self.app = code, kind, g, call, family, params, soft, app


def triple_kw(t):
    return {} if t is None else dict(scale_num=t[0], scale_shift=t[1], offset=t[2])


def entries():
    out = []
    layered_g = lambda c: layered_helpers.layered_grid_bound(c, 1)[1]                                              # noqa: E731
    # flooding soft output, the f32-pipe kernels
    for kind, codes in (("f32", (C.TC256, C.TM8192)), ("i8", (C.TC256, C.TM8192)), ("i16", (C.TC256, C.TM8192)),
                        ("i32", (C.TC256, C.TM8192)), ("f64", (C.TC256,))):
        for code in codes:
            out.append(Entry("decode_ms_soft_batch", code, kind, flooding_grid_bound(code, NP[kind], 0, 1)[1],
                             lambda c, x, cap, b: c.decode_ms_soft_batch(x, cap, **b), "flooding", None, True))
    # layered f32, plain and corrected; f16 / bf16 through the same methods (the loader widens)
    for kind, codes in (("f32", (C.TC128, C.TM2048, C.TM8192)), ("f16", (C.TC128, C.TM2048)), ("bf16", (C.TC128, C.TM2048))):
        for code in codes:
            for pair in (None, PAIR):
                kw = {} if pair is None else dict(scale=pair[0], offset=pair[1])
                note = "plain" if pair is None else "scale-offset"
                out.append(Entry("decode_ms_layered_batch", code, kind, layered_g(code),
                                 lambda c, x, cap, b, kw=kw: c.decode_ms_layered_batch(x, cap, **b, **kw), "layered", pair, False, note=note))
                out.append(Entry("decode_ms_layered_soft_batch", code, kind, layered_g(code),
                                 lambda c, x, cap, b, kw=kw: c.decode_ms_layered_soft_batch(x, cap, **b, **kw), "layered", pair, True,
                                 app="f32", note=note))
    # fixed-point layered: the plain entry, an identity triple and (13, 4, 0); then the same behind the quantising loader
    for code in (C.TC128, C.TM8192):
        for kind in ("i8", "i16"):
            for triple, note in ((None, "plain"), ((16, 4, 0), "identity"), (TRIPLE, "13-4-0")):
                kw = triple_kw(triple)
                out.append(Entry("decode_ms_layered_fixed_batch", code, kind, codewords_per_workgroup(code),
                                 lambda c, x, cap, b, kw=kw: c.decode_ms_layered_fixed_batch(x, cap, **b, **kw), "fixed", triple, False, note=note))
                out.append(Entry("decode_ms_layered_fixed_soft_batch", code, kind, codewords_per_workgroup(code),
                                 lambda c, x, cap, b, kw=kw: c.decode_ms_layered_fixed_soft_batch(x, cap, **b, **kw), "fixed", triple, True,
                                 app="i32", note=note))
            for triple, note in ((None, "plain"), (TRIPLE, "13-4-0")):
                kw, suf = triple_kw(triple), kind
                out.append(Entry("decode_ms_layered_quantised_batch", code, "q-" + suf, codewords_per_workgroup(code),
                                 lambda c, x, cap, b, kw=kw, suf=suf: c.decode_ms_layered_quantised_batch(x, suf, *QUANT[suf], cap, **b, **kw),
                                 "quantised-layered", (suf, triple), False, note=note))
                out.append(Entry("decode_ms_layered_quantised_soft_batch", code, "q-" + suf, codewords_per_workgroup(code),
                                 lambda c, x, cap, b, kw=kw, suf=suf: c.decode_ms_layered_quantised_soft_batch(x, suf, *QUANT[suf], cap, **b, **kw),
                                 "quantised-layered", (suf, triple), True, app="i32", note=note))
    # corrected f32 flooding
    for code in (C.TC256, C.TM2048, C.TM8192):
        kw = dict(scale=PAIR[0], offset=PAIR[1])
        g = flooding_grid_bound(code, np.float32, 0, 1)[1]
        out.append(Entry("decode_ms_batch", code, "f32", g, lambda c, x, cap, b, kw=kw: c.decode_ms_batch(x, cap, **b, **kw),
                         "flooding-corrected", PAIR, False, note="scale-offset"))
        out.append(Entry("decode_ms_soft_batch", code, "f32", g, lambda c, x, cap, b, kw=kw: c.decode_ms_soft_batch(x, cap, **b, **kw),
                         "flooding-corrected", PAIR, True, note="scale-offset"))
    # bit-sliced i8, the one-wave codes
    for code in ONE_WAVE:
        g = BS_GROUP[code]
        out.append(Entry("decode_ms_corrected_fixed_batch", code, "i8", g,
                         lambda c, x, cap, b: c.decode_ms_corrected_fixed_batch(x, *TRIPLE, cap, **b), "bitsliced", (127, TRIPLE), False))
        for triple, note in ((None, "plain"), (TRIPLE, "corrected")):
            kw = triple_kw(triple)
            out.append(Entry("decode_ms_bitsliced_soft_batch", code, "i8", g,
                             lambda c, x, cap, b, kw=kw: c.decode_ms_bitsliced_soft_batch(x, cap, **b, **kw), "bitsliced", (127, triple), True,
                             note=note))
            out.append(Entry("decode_ms_quantised_batch", code, "q-i8", g,
                             lambda c, x, cap, b, kw=kw: c.decode_ms_quantised_batch(x, "i8", 8.0, 31, cap, bitsliced=True, **b, **kw),
                             "bitsliced", (31, triple), False, note="bitsliced-" + note))
            out.append(Entry("decode_ms_bitsliced_quantised_soft_batch", code, "q-i8", g,
                             lambda c, x, cap, b, kw=kw: c.decode_ms_bitsliced_quantised_soft_batch(x, 8.0, 31, cap, **b, **kw),
                             "bitsliced", (31, triple), True, app="i8", note=note))
    # bit-sliced i8, two waves per group: the hard entries there are
    for code in TWO_WAVES:
        g = BS_GROUP[code]
        out.append(Entry("decode_ms_batch", code, "i8", g, lambda c, x, cap, b: c.decode_ms_batch(x, cap, variant=BS, **b),
                         "bitsliced", (127, None), False, note="bitsliced"))
        out.append(Entry("decode_ms_corrected_fixed_batch", code, "i8", g,
                         lambda c, x, cap, b: c.decode_ms_corrected_fixed_batch(x, *TRIPLE, cap, **b), "bitsliced", (127, TRIPLE), False))
    return out


def torch_dtype(kind):
    import torch
    return {"f32": torch.float32, "f64": torch.float64, "i8": torch.int8, "i16": torch.int16, "i32": torch.int32, "f16": torch.float16,
            "bf16": torch.bfloat16, "q-i8": torch.float32, "q-i16": torch.float32}[kind]


def host_rows(x, kind):
    """pool rows as the CPU tensor that is copied into the device input (halves: the format's bits reinterpreted)"""
    import torch
    if kind in ("f16", "bf16"):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int16)).view(torch_dtype(kind))
    return torch.from_numpy(np.ascontiguousarray(x))


def decoder_results(code, frames, soft, app_dtype):
    import torch
    res = []
    if soft:
        res.append(("app", torch.empty((frames, code.n() + code.punctured_bits()), dtype=app_dtype, device="cuda")))
    return res + [("output", torch.empty((frames, code.output_len()), dtype=torch.uint8, device="cuda")),
                  ("iters", torch.empty((frames,), dtype=torch.int32, device="cuda")),
                  ("success", torch.empty((frames,), dtype=torch.uint8, device="cuda"))]


# ---- the streaming kernels ----------------------------------------------------------------------------------------------------------------
def streaming_cases():
    """id -> (code, build): build() returns (call, inputs, results, sets, refs) of captured.host_case"""
    import torch
    cases = {}

    def put(name, code, build):
        cases[f"{name}-{code.name}"] = (code, build)

    def tensor(shape, dtype):
        return torch.empty(shape, dtype=dtype, device="cuda")

    def bf(code, cap):
        words, _, _ = hard_frames.bf_pool(code)
        res = hard_frames.bf_results(code, cap)
        sets = [np.array([0, 16, 32, 1, 17]), np.array([33, 2, 18, 34, 3]), np.array([40, 41, 20, 21, 5])]
        x = tensor((5, code.n() // 8), torch.uint8)
        results = decoder_results(code, 5, False, None)
        return (lambda: code.decode_bf_batch(x, cap, **dict(results)), [x], results, [[words[i]] for i in sets],
                [{"output": res[0][i], "iters": res[1][i], "success": res[2][i]} for i in sets])

    for cap in (0, 1, 20):
        put(f"decode_bf_batch-cap{cap}", C.TM2048, functools.partial(bf, C.TM2048, cap))
        put(f"decode_bf_batch-cap{cap}", C.TC256, functools.partial(bf, C.TC256, cap))

    def encode(code):
        data, cws = hard_frames.enc_pool(code)
        sets = [np.arange(0, 5), np.arange(5, 10), np.arange(59, 64)]
        x, y = tensor((5, code.k() // 8), torch.uint8), tensor((5, code.n() // 8), torch.uint8)
        return (lambda: code.encode_batch(x, codewords=y), [x], [("codewords", y)], [[data[i]] for i in sets], [{"codewords": cws[i]} for i in sets])

    for code in (C.TC256, C.TM2048, C.TM5120):
        put("encode_batch", code, functools.partial(encode, code))

    def hard_to_llrs(code, suf):
        _, cws = hard_frames.enc_pool(code)
        sets = [np.arange(0, 5), np.arange(11, 16)]
        x, y = tensor((5, code.n() // 8), torch.uint8), tensor((5, code.n()), torch_dtype(suf))
        want = [np.stack([oracle.hard_to_llrs(code, w, NP[suf]) for w in cws[i]]) for i in sets]
        return (lambda: code.hard_to_llrs_batch(x, suf, llrs=y), [x], [("llrs", y)], [[cws[i]] for i in sets], [{"llrs": w} for w in want])

    def llrs_to_hard(code, suf):
        pool = small_pool(code, suf)[0]
        sets = windows(len(pool), 5)
        x, y = tensor((5, code.n()), torch_dtype(suf)), tensor((5, code.n() // 8), torch.uint8)
        want = [np.stack([oracle.llrs_to_hard(code, r) for r in pool[i]]) for i in sets]
        return (lambda: code.llrs_to_hard_batch(x, output=y), [x], [("hard", y)], [[pool[i]] for i in sets], [{"hard": w} for w in want])

    for suf in ("f32", "f64", "i8", "i16", "i32"):
        put(f"hard_to_llrs_batch-{suf}", C.TM1280, functools.partial(hard_to_llrs, C.TM1280, suf))
        put(f"llrs_to_hard_batch-{suf}", C.TM1280, functools.partial(llrs_to_hard, C.TM1280, suf))

    def quantise(code, suf):
        pool = small_pool(code, "q-" + suf)[0]
        sets = windows(len(pool), 5)
        scale, lim = QUANT[suf]
        x, y = tensor((5, code.n()), torch.float32), tensor((5, code.n()), torch_dtype(suf))
        return (lambda: code.quantise_llrs_batch(x, suf, scale, lim, out=y), [x], [("quantised", y)], [[pool[i]] for i in sets],
                [{"quantised": qr.quantise(pool[i], NP[suf], scale, lim)} for i in sets])

    def widen_rows(code, fmt):
        bits = small_pool(code, fmt)[0]
        sets = windows(len(bits), 5)
        x, y = tensor((5, code.n()), torch_dtype(fmt)), tensor((5, code.n()), torch.float32)
        return (lambda: code.widen_llrs_batch(x, out=y), [x], [("widened", y)], [[host_rows(bits[i], fmt)] for i in sets],
                [{"widened": widen(bits[i], fmt)} for i in sets])

    for code in (C.TC256, C.TM6144):
        for suf in ("i8", "i16"):
            put(f"quantise_llrs_batch-{suf}", code, functools.partial(quantise, code, suf))
        for fmt in ("f16", "bf16"):
            put(f"widen_llrs_batch-{fmt}", code, functools.partial(widen_rows, code, fmt))
    return cases


# ---- every batched symbol, for the route tests ----------------------------------------------------------------------------------------------
# Batched symbols that do not run on the batched call path, by prefix, each with its reason.  tests/test_call_routes_host.py holds
# every name of la.SYMBOLS that contains "batch" to this list or to route_entries(), and this list to these families.
EXCLUDED = {
    "labrador_ldpc_hard_to_llrs_batch_": "a converter on convert_call: no staging, host buffers are converted where they lie",
    "labrador_ldpc_llrs_to_hard_batch_": "a converter on convert_call: no staging, host buffers are converted where they lie",
    "labrador_ldpc_quantise_llrs_batch_": "a converter on convert_call: no staging, host buffers are converted where they lie",
    "labrador_ldpc_widen_llrs_batch_": "a converter on convert_call: no staging, host buffers are converted where they lie",
    "_multi": "takes device-resident parts, one per device, on the workers' own path: no memory mode, no host staging",
}

CAP, SWEEPS = 25, 20                                         # max_iters of every decode here; max_sweeps of the cascades
HARD_MAGNITUDE = {"plain": 1, "corrected": bs_hard_frames.CORRECTED_MAGNITUDE}
LAYERED_PAIR = (0.875, 0.0)                                  # stage 2 of the f32 cascades that carry PAIR for stage 1
LAYERED_TRIPLE = (14, 4, 1)                                  # stage 2 of the integer cascades that carry TRIPLE for stage 1
SENTINEL_NAN = {np.dtype(np.float32): 0x7FC0EEEE, np.dtype(np.float64): 0x7FF8EEEEEEEEEEEE}
WORKSPACE_CHUNK = {"cascade": "LABRADOR_LDPC_HIP_CASCADE_CHUNK", "quantised": "LABRADOR_LDPC_HIP_QUANT_CHUNK",
                   "widened": "LABRADOR_LDPC_HIP_WIDEN_CHUNK"}


class RouteEntry:
    """One batched symbol on one code.
    symbol: the C name.  code, kind: the code and the kind of its input rows (an LLR type, "q-i8" / "q-i16": f32 for the quantiser,
    "packed": hard decisions, "bf": decode_bf's words, "data": the encoder's blocks).  g: codewords per workgroup or wave group.
    method(code, inputs, kw): the call through LDPCCode; `inputs` numpy arrays (host) or torch tensors (device), `kw` the result buffers
    by keyword and, for host arrays, `devices`.  results: [(name, numpy dtype, elements per item)] in the order the C ABI stages them
    (output, iters, success, [stage], [app]); in_bytes / out_bytes: the bytes per item of the inputs and of those outputs.
    pool(): the inputs' pool rows, [(array [P, row])]; reference(): {result name: [P, ...]} of the CPU statement on the pool.
    workspace: the workspace whose chunk variable (WORKSPACE_CHUNK) cuts the entry's launch slices further, or None.
    bitsliced: a bit-sliced i8 kernel decodes (stage 1 of) the call."""

    def __init__(self, symbol, code, kind, method, reference, app=None, stage=False, workspace=None, bitsliced=False, note="", masked=False,
                 results=None, pool=None, g=None):
        self.symbol, self.code, self.kind, self.method, self.workspace, self.bitsliced, self.masked = symbol, code, kind, method, workspace, bitsliced, masked
        self.id = "-".join(x for x in (symbol[len("labrador_ldpc_"):], note, code.name) if x)
        self.g = g if g is not None else BS_GROUP[code] if bitsliced else codewords_per_workgroup(code)
        n, np_len = code.n(), code.n() + code.punctured_bits()
        if results is None:
            results = [("output", np.uint8, code.output_len()), ("iters", np.int32, 0), ("success", np.uint8, 0)]
            if stage:
                results.append(("stage", np.uint8, 0))
            if app is not None:
                results.append(("app", app, np_len))
        self.results = [(name, np.dtype(dt), row) for name, dt, row in results]
        self.out_bytes = tuple(dt.itemsize * max(row, 1) for _, dt, row in self.results)
        row = {"packed": n // 8, "bf": n // 8, "data": code.k() // 8, "f16": 2 * n, "bf16": 2 * n, "q-i8": 4 * n, "q-i16": 4 * n}
        self.in_bytes = (row[kind] if kind in row else n * np.dtype(NP[kind]).itemsize,) * (2 if masked else 1)
        self._pool, self._reference = pool, reference

    @functools.lru_cache(maxsize=None)
    def pool(self):
        if self._pool is not None:
            return self._pool()
        return (small_pool(self.code, self.kind)[0],)

    @functools.lru_cache(maxsize=None)
    def reference(self):
        ref = {k: np.ascontiguousarray(v) for k, v in self._reference().items()}
        assert sorted(ref) == sorted(name for name, _, _ in self.results), (self.id, sorted(ref))
        for name, dt, row in self.results:                   # in the dtype of the caller's buffer: a statement may count in another integer
            v = ref[name]
            if v.dtype != dt:
                assert v.dtype.kind in "iub" and dt.kind in "iu", (self.id, name, v.dtype, dt)
                ref[name] = v.astype(dt)
                assert (ref[name].astype(np.int64) == v.astype(np.int64)).all(), (self.id, name)
            assert ref[name].shape == (len(self.pool()[0]),) + ((row,) if row else ()), (self.id, name, ref[name].shape)
            ref[name].setflags(write=False)
        return ref


def _hard(ref):
    return {"output": ref[0], "iters": ref[1], "success": ref[2]}


def _soft(ref):
    return dict(_hard(ref), app=ref[3])


def _staged(ref):
    return dict(_hard(ref), stage=ref[3])


def _staged_soft(ref):
    return {"app": ref[0], "output": ref[1], "iters": ref[2], "success": ref[3], "stage": ref[4]}


def half_host_call(symbol, code, bits, kw, extra=()):
    """`symbol` on HOST rows of raw half bits: numpy has no bfloat16, so LDPCCode offers no host bf16 rows and the route tests call the
    C symbol as LDPCCode._batch_call does: llrs, [app], output, iters, success, [stage], batch, max_iters, extra, opts."""
    import ctypes
    kw = dict(kw)
    opts, keep = la._host_opts(None, 0, kw.pop("devices", None))
    bufs = [kw[k] for k in ("app", "output", "iters", "success", "stage") if k in kw]
    assert len(bufs) == len(kw) and bits.dtype == np.uint16 and bits.flags.c_contiguous
    status = getattr(la.lib, symbol)(int(code), bits.ctypes.data, *(b.ctypes.data for b in bufs), len(bits), CAP, *extra, ctypes.byref(opts))
    del keep
    assert status == 0, (symbol, status, la.last_error())


def route_entries():
    out = []
    small, bs_small, bs_all = C.TC128, C.TM1280, (C.TM1280, C.TM1536)
    P = "labrador_ldpc_decode_ms_"

    def values(code, kind):
        return small_values(code, kind)

    def quantised(code, suf, lim=None):
        scale, qlim = QUANT[suf] if lim is None else (8.0, lim)
        return qr.quantise(values(code, "q-" + suf), NP[suf], scale, qlim)

    def family(fam, code, kind, params, soft):
        return lambda: (_soft if soft else _hard)(decode_reference(fam, code, values(code, kind), CAP, params))

    def half(method, symbol, fmt, extra=()):
        """the method on f16 rows (host: as numpy float16) and on device tensors; host bf16 rows through the symbol itself"""
        def call(c, inputs, kw):
            x = inputs[0]
            if isinstance(x, np.ndarray):
                if fmt == "bf16":
                    return half_host_call(symbol, c, x, kw, extra)
                x = x.view(np.float16)
            return method(c, x, kw)
        return call

    # -- flooding, hard and soft, every LLR type; f16 / bf16 through the widening workspace
    for t in ("f32", "f64", "i8", "i16", "i32"):
        out.append(RouteEntry(P + "batch_" + t, small, t, lambda c, x, kw: c.decode_ms_batch(x[0], CAP, **kw),
                              lambda t=t: _hard(oracle.decode_ms_batch(small, values(small, t), CAP))))
        out.append(RouteEntry(P + "soft_batch_" + t, small, t, lambda c, x, kw: c.decode_ms_soft_batch(x[0], CAP, **kw),
                              family("flooding", small, t, None, True), app=NP[t]))
    for fmt in ("f16", "bf16"):
        out.append(RouteEntry(P + "batch_" + fmt, small, fmt, half(lambda c, x, kw: c.decode_ms_batch(x, CAP, **kw), P + "batch_" + fmt, fmt),
                              lambda fmt=fmt: _hard(oracle.decode_ms_batch(small, values(small, fmt), CAP)), workspace="widened"))
        out.append(RouteEntry(P + "soft_batch_" + fmt, small, fmt,
                              half(lambda c, x, kw: c.decode_ms_soft_batch(x, CAP, **kw), P + "soft_batch_" + fmt, fmt),
                              family("flooding", small, fmt, None, True), app=np.float32, workspace="widened"))
    # -- corrected f32 flooding
    pair = dict(scale=PAIR[0], offset=PAIR[1])
    out.append(RouteEntry(P + "corrected_batch_f32", small, "f32", lambda c, x, kw: c.decode_ms_batch(x[0], CAP, **kw, **pair),
                          family("flooding-corrected", small, "f32", PAIR, False)))
    out.append(RouteEntry(P + "corrected_soft_batch_f32", small, "f32", lambda c, x, kw: c.decode_ms_soft_batch(x[0], CAP, **kw, **pair),
                          family("flooding-corrected", small, "f32", PAIR, True), app=np.float32))
    # -- layered f32, and f16 / bf16 through the same kernels' widening loader
    for t in ("f32", "f16", "bf16"):
        wrap = (lambda m, s, e=(): lambda c, x, kw: m(c, x[0], kw)) if t == "f32" else (lambda m, s, e=(), t=t: half(m, s, t, e))
        out.append(RouteEntry(P + "layered_batch_" + t, small, t,
                              wrap(lambda c, x, kw: c.decode_ms_layered_batch(x, CAP, **kw), P + "layered_batch_" + t),
                              family("layered", small, t, None, False)))
        out.append(RouteEntry(P + "layered_soft_batch_" + t, small, t,
                              wrap(lambda c, x, kw: c.decode_ms_layered_soft_batch(x, CAP, **kw), P + "layered_soft_batch_" + t),
                              family("layered", small, t, None, True), app=np.float32))
        out.append(RouteEntry(P + "layered_corrected_batch_" + t, small, t,
                              wrap(lambda c, x, kw: c.decode_ms_layered_batch(x, CAP, **kw, **pair), P + "layered_corrected_batch_" + t, PAIR),
                              family("layered", small, t, PAIR, False)))
        out.append(RouteEntry(P + "layered_corrected_soft_batch_" + t, small, t,
                              wrap(lambda c, x, kw: c.decode_ms_layered_soft_batch(x, CAP, **kw, **pair),
                                   P + "layered_corrected_soft_batch_" + t, PAIR),
                              family("layered", small, t, PAIR, True), app=np.float32))
    # -- fixed-point layered, and the same behind the quantising loader
    triple = triple_kw(TRIPLE)
    for t in ("i8", "i16"):
        out.append(RouteEntry(P + "layered_fixed_batch_" + t, small, t, lambda c, x, kw: c.decode_ms_layered_fixed_batch(x[0], CAP, **kw),
                              family("fixed", small, t, None, False)))
        out.append(RouteEntry(P + "layered_fixed_soft_batch_" + t, small, t, lambda c, x, kw: c.decode_ms_layered_fixed_soft_batch(x[0], CAP, **kw),
                              family("fixed", small, t, None, True), app=np.int32))
        out.append(RouteEntry(P + "layered_fixed_corrected_batch_" + t, small, t,
                              lambda c, x, kw: c.decode_ms_layered_fixed_batch(x[0], CAP, **kw, **triple), family("fixed", small, t, TRIPLE, False)))
        out.append(RouteEntry(P + "layered_fixed_corrected_soft_batch_" + t, small, t,
                              lambda c, x, kw: c.decode_ms_layered_fixed_soft_batch(x[0], CAP, **kw, **triple),
                              family("fixed", small, t, TRIPLE, True), app=np.int32))
        out.append(RouteEntry(P + "layered_quantised_batch_" + t, small, "q-" + t,
                              lambda c, x, kw, t=t: c.decode_ms_layered_quantised_batch(x[0], t, *QUANT[t], CAP, **kw, **triple),
                              family("quantised-layered", small, "q-" + t, (t, TRIPLE), False)))
        out.append(RouteEntry(P + "layered_quantised_soft_batch_" + t, small, "q-" + t,
                              lambda c, x, kw, t=t: c.decode_ms_layered_quantised_soft_batch(x[0], t, *QUANT[t], CAP, **kw, **triple),
                              family("quantised-layered", small, "q-" + t, (t, TRIPLE), True), app=np.int32))
        # the fused quantise + flooding call: the quantiser's workspace
        out.append(RouteEntry(P + "quantised_batch_" + t, small, "q-" + t,
                              lambda c, x, kw, t=t: c.decode_ms_quantised_batch(x[0], t, *QUANT[t], CAP, **kw),
                              lambda t=t: _hard(oracle.decode_ms_batch(small, quantised(small, t), CAP)), workspace="quantised"))
    # -- the bit-sliced i8 kernels: `variant` 64 of the plain entry and the corrected entry on TM1280 and TM1536, the rest on TM1536
    for code in bs_all:
        out.append(RouteEntry(P + "batch_i8", code, "i8", lambda c, x, kw: c.decode_ms_batch(x[0], CAP, variant=BS, **kw),
                              family("bitsliced", code, "i8", (127, None), False), bitsliced=True, note="variant64"))
        out.append(RouteEntry(P + "corrected_batch_i8", code, "i8", lambda c, x, kw: c.decode_ms_corrected_fixed_batch(x[0], *TRIPLE, CAP, **kw),
                              family("bitsliced", code, "i8", (127, TRIPLE), False), bitsliced=True))
    one = C.TM1536
    out.append(RouteEntry(P + "bitsliced_soft_batch_i8", one, "i8", lambda c, x, kw: c.decode_ms_bitsliced_soft_batch(x[0], CAP, **kw),
                          family("bitsliced", one, "i8", (127, None), True), app=np.int8, bitsliced=True))
    out.append(RouteEntry(P + "bitsliced_corrected_soft_batch_i8", one, "i8",
                          lambda c, x, kw: c.decode_ms_bitsliced_soft_batch(x[0], CAP, **kw, **triple),
                          family("bitsliced", one, "i8", (127, TRIPLE), True), app=np.int8, bitsliced=True))
    out.append(RouteEntry(P + "bitsliced_quantised_batch_i8", one, "q-i8",
                          lambda c, x, kw: c.decode_ms_quantised_batch(x[0], "i8", 8.0, 31, CAP, bitsliced=True, **kw),
                          family("bitsliced", one, "q-i8", (31, None), False), bitsliced=True))
    out.append(RouteEntry(P + "bitsliced_quantised_corrected_batch_i8", one, "q-i8",
                          lambda c, x, kw: c.decode_ms_quantised_batch(x[0], "i8", 8.0, 31, CAP, bitsliced=True, **kw, **triple),
                          family("bitsliced", one, "q-i8", (31, TRIPLE), False), bitsliced=True))
    out.append(RouteEntry(P + "bitsliced_quantised_soft_batch_i8", one, "q-i8",
                          lambda c, x, kw: c.decode_ms_bitsliced_quantised_soft_batch(x[0], 8.0, 31, CAP, **kw),
                          family("bitsliced", one, "q-i8", (31, None), True), app=np.int8, bitsliced=True))
    out.append(RouteEntry(P + "bitsliced_quantised_corrected_soft_batch_i8", one, "q-i8",
                          lambda c, x, kw: c.decode_ms_bitsliced_quantised_soft_batch(x[0], 8.0, 31, CAP, **kw, **triple),
                          family("bitsliced", one, "q-i8", (31, TRIPLE), True), app=np.int8, bitsliced=True))
    # -- the packed hard-decision entries, with and without the mask: bs_hard_frames' rows, where masked and unmasked rows alternate
    hard_pool = lambda: bs_hard_frames.frames(one.name)      # (build_frames at the module's committed seed, built once)  # noqa: E731
    for form, kw3 in (("plain", {}), ("corrected", triple)):
        for masked in (False, True):
            magnitude = HARD_MAGNITUDE[form]

            def call(c, x, kw, magnitude=magnitude, kw3=kw3, masked=masked):
                return c.decode_ms_hard_batch(x[0], CAP, magnitude, erasures=x[1] if masked else None, **kw, **kw3)

            def ref(form=form, masked=masked, magnitude=magnitude):
                x, m = hard_pool()
                e = bs_hard_frames.expand(x, m if masked else None, magnitude)
                if form == "plain":
                    return _hard(oracle.decode_ms_batch(one, e, CAP))
                return _hard(bs_hard_frames.corrected_statement.decode(bs_hard_frames.corrected_statement.structure(int(one)), e, CAP, *TRIPLE))

            out.append(RouteEntry(P + "bitsliced_hard_" + ("batch_i8" if form == "plain" else "corrected_batch_i8"), one, "packed", call, ref,
                                  bitsliced=True, masked=masked, note="masked" if masked else "unmasked",
                                  pool=(lambda: hard_pool()) if masked else (lambda: hard_pool()[:1])))
            if masked:
                out[-1].unmasked = out[-2]                   # the same rows without their mask
    # -- the cascades.  Every pool holds 4 dB frames, which stage 1 decodes, and 0 dB frames, which go to stage 2.
    def stage1_f32(code, flooding):
        if flooding is None:
            return cs.flooding_soft(code)
        return lambda l, cap: flc.decode_flooding_corrected(flooding_structure(code, flc), l, cap, *flooding)

    def stage1_int(code, flooding):
        if flooding is None:
            return cs.flooding_soft(code)
        return lambda l, cap: ffs.decode(flooding_structure(code, ffs), l, cap, *flooding)

    def hard_cascade(code, y, first, correction):
        return lambda: _staged(cr.compose(first, cr.layered(code, correction), y(), CAP, SWEEPS))

    def soft_cascade(code, y, first, correction):
        return lambda: _staged_soft(cs.compose_soft(first, cr.layered(code, correction), y(), CAP, SWEEPS))

    cascade_pair = dict(scale=LAYERED_PAIR[0], offset=LAYERED_PAIR[1])
    flooding_pair = dict(flooding_scale=PAIR[0], flooding_offset=PAIR[1])
    for t in ("f32", "f16", "bf16"):
        m = lambda c, x, kw: c.decode_ms_cascade_batch(x, CAP, SWEEPS, **kw, **cascade_pair)                         # noqa: E731
        out.append(RouteEntry(P + "cascade_batch_" + t, small, t,
                              (lambda c, x, kw, m=m: m(c, x[0], kw)) if t == "f32" else half(m, P + "cascade_batch_" + t, t, (SWEEPS, *LAYERED_PAIR)),
                              hard_cascade(small, lambda t=t: values(small, t), stage1_f32(small, None), LAYERED_PAIR), stage=True,
                              workspace="cascade"))
    out.append(RouteEntry(P + "cascade_corrected_batch_f32", small, "f32",
                          lambda c, x, kw: c.decode_ms_cascade_batch(x[0], CAP, SWEEPS, **kw, **cascade_pair, **flooding_pair),
                          hard_cascade(small, lambda: values(small, "f32"), stage1_f32(small, PAIR), LAYERED_PAIR), stage=True,
                          workspace="cascade"))
    out.append(RouteEntry(P + "cascade_soft_batch_f32", small, "f32",
                          lambda c, x, kw: c.decode_ms_cascade_soft_batch(x[0], CAP, SWEEPS, **kw, **cascade_pair, **flooding_pair),
                          soft_cascade(small, lambda: values(small, "f32"), stage1_f32(small, PAIR), LAYERED_PAIR), app=np.float32, stage=True,
                          workspace="cascade"))
    for t in ("i8", "i16"):
        out.append(RouteEntry(P + "cascade_batch_" + t, small, t, lambda c, x, kw: c.decode_ms_cascade_fixed_batch(x[0], CAP, SWEEPS, **kw, **triple),
                              hard_cascade(small, lambda t=t: values(small, t), stage1_int(small, None), TRIPLE), stage=True, workspace="cascade"))
        out.append(RouteEntry(P + "cascade_soft_batch_" + t, small, t,
                              lambda c, x, kw: c.decode_ms_cascade_fixed_soft_batch(x[0], CAP, SWEEPS, **kw, **triple),
                              soft_cascade(small, lambda t=t: values(small, t), stage1_int(small, None), TRIPLE), app=np.int32, stage=True,
                              workspace="cascade"))
        out.append(RouteEntry(P + "cascade_quantised_batch_" + t, small, "q-" + t,
                              lambda c, x, kw, t=t: c.decode_ms_cascade_quantised_batch(x[0], t, *QUANT[t], CAP, SWEEPS, **kw, **triple),
                              hard_cascade(small, lambda t=t: quantised(small, t), stage1_int(small, None), TRIPLE), stage=True,
                              workspace="cascade"))
    layered3 = triple_kw(LAYERED_TRIPLE)
    flooding3 = dict(flooding_scale_num=TRIPLE[0], flooding_scale_shift=TRIPLE[1], flooding_offset=TRIPLE[2])
    for code in bs_all:                                      # stage 1: the corrected bit-sliced kernels of the TM codes
        out.append(RouteEntry(P + "cascade_corrected_batch_i8", code, "i8",
                              lambda c, x, kw: c.decode_ms_cascade_fixed_batch(x[0], CAP, SWEEPS, **kw, **layered3, **flooding3),
                              hard_cascade(code, lambda code=code: values(code, "i8"), stage1_int(code, TRIPLE), LAYERED_TRIPLE), stage=True,
                              workspace="cascade", bitsliced=True))
        out.append(RouteEntry(P + "cascade_quantised_corrected_batch_i8", code, "q-i8",
                              lambda c, x, kw: c.decode_ms_cascade_quantised_batch(x[0], "i8", 8.0, 31, CAP, SWEEPS, **kw, **layered3, **flooding3),
                              hard_cascade(code, lambda code=code: quantised(code, "i8", 31), stage1_int(code, TRIPLE), LAYERED_TRIPLE),
                              stage=True, workspace="cascade", bitsliced=True))
    out.append(RouteEntry(P + "cascade_bitsliced_soft_batch_i8", one, "i8",
                          lambda c, x, kw: c.decode_ms_cascade_fixed_soft_batch(x[0], CAP, SWEEPS, bitsliced=True, **kw, **layered3),
                          soft_cascade(one, lambda: values(one, "i8"), stage1_int(one, None), LAYERED_TRIPLE), app=np.int32, stage=True,
                          workspace="cascade", bitsliced=True))
    out.append(RouteEntry(P + "cascade_bitsliced_corrected_soft_batch_i8", one, "i8",
                          lambda c, x, kw: c.decode_ms_cascade_fixed_soft_batch(x[0], CAP, SWEEPS, bitsliced=True, **kw, **layered3, **flooding3),
                          soft_cascade(one, lambda: values(one, "i8"), stage1_int(one, TRIPLE), LAYERED_TRIPLE), app=np.int32, stage=True,
                          workspace="cascade", bitsliced=True))
    out.append(RouteEntry(P + "cascade_bitsliced_quantised_batch_i8", one, "q-i8",
                          lambda c, x, kw: c.decode_ms_cascade_quantised_batch(x[0], "i8", 8.0, 31, CAP, SWEEPS, bitsliced=True, **kw, **layered3,
                                                                               **flooding3),
                          hard_cascade(one, lambda: quantised(one, "i8", 31), stage1_int(one, TRIPLE), LAYERED_TRIPLE), stage=True,
                          workspace="cascade", bitsliced=True))
    out.append(RouteEntry(P + "cascade_bitsliced_quantised_soft_batch_i8", one, "q-i8",
                          lambda c, x, kw: c.decode_ms_cascade_bitsliced_quantised_soft_batch(x[0], 8.0, 31, CAP, SWEEPS, **kw, **layered3,
                                                                                              **flooding3),
                          soft_cascade(one, lambda: quantised(one, "i8", 31), stage1_int(one, TRIPLE), LAYERED_TRIPLE), app=np.int32, stage=True,
                          workspace="cascade", bitsliced=True))
    # -- the bit-flipping decoder and the encoder
    bf_iters = hard_frames.BF_ITERS
    out.append(RouteEntry("labrador_ldpc_decode_bf_batch", small, "bf", lambda c, x, kw: c.decode_bf_batch(x[0], bf_iters, **kw),
                          lambda: _hard(hard_frames.bf_pool(small)[1]), pool=lambda: (hard_frames.bf_pool(small)[0],)))
    out.append(RouteEntry("labrador_ldpc_encode_batch", small, "data", lambda c, x, kw: c.encode_batch(x[0], **kw),
                          lambda: {"codewords": hard_frames.enc_pool(small)[1]}, pool=lambda: (hard_frames.enc_pool(small)[0],),
                          results=[("codewords", np.uint8, small.n() // 8)]))
    ids = [e.id for e in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return out
