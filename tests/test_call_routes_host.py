"""The route tests' own ground, checked without a GPU: the thresholds tests/call_routes.py sizes its batches by are the source's; every
batched symbol of the header is in tests/entry_table.py's table or excluded with a reason; every entry has a batch on every route;
and every batch -- drawn from the entry's pool by its committed seed -- is one on which a pointer that is not advanced, or advanced
by another buffer's stride, cannot reproduce the CPU statement (call_routes.conditions)."""
import os
import re

import numpy as np
import pytest

import call_routes as rt
import entry_table as et
import labrador_ldpc_amd as la

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = et.route_entries()
ROUTES = ("r1", "r2", "r3", "r4", "r5", "r6", "r7-small", "r7-17", "r7-chunks")


def source(name):
    with open(os.path.join(ROOT, "labrador_ldpc_amd", "csrc", name)) as f:
        return f.read()


def test_thresholds_and_slice_rule_match_the_source():
    """SMALL_CALL_BYTES and DIRECT_CALL_BYTES as csrc/capi_staging.hpp writes them; the small call is asked for before the chunk is
    looked at, on in_pad + the padded outputs; max_launch_frames() takes at least 8 and multiples of 8.  A change of any of these
    fails here, and tests/call_routes.py is then sized again."""
    text = source("capi_staging.hpp")
    m = re.search(r"constexpr size_t SMALL_CALL_BYTES = (\d+)u << (\d+), DIRECT_CALL_BYTES = (\d+)u << (\d+);", text)
    assert m, "the thresholds are no longer written as two shifts in one line"
    small, direct = int(m[1]) << int(m[2]), int(m[3]) << int(m[4])
    assert (small, direct) == (rt.SMALL_CALL_BYTES, rt.DIRECT_CALL_BYTES)
    assert rt.R1_MAX_BYTES < direct < rt.R2_MIN_BYTES <= rt.R2_MAX_BYTES < small < rt.R3_MIN_BYTES
    body = text[text.index("int host_pipeline("):]
    at_small, at_direct = body.index("if (in_pad + out_off[NOUT] <= SMALL_CALL_BYTES)"), body.index("in_pad + out_off[NOUT] <= DIRECT_CALL_BYTES")
    assert at_small < at_direct < body.index("chunk_items(in_bytes_per_item + in2_bytes_per_item)")
    for line in ("out_off[o + 1] = (out_off[o] + items * outs[o].bytes_per_item + 15) / 16 * 16;",
                 "in1_total = items * in_bytes_per_item, in1_pad = (in1_total + 15) / 16 * 16, in2_total = items * in2_bytes_per_item;",
                 "in_total = in2 ? in1_pad + in2_total : in1_total, in_pad = (in_total + 15) / 16 * 16;"):
        assert line in body, line
    slices = text[text.index("size_t max_launch_frames()"):text.index("hipError_t for_launch_slices(")]
    assert f"if (v >= {rt.SLICE} && (size_t)v <= MAX_LAUNCH_FRAMES && v % {rt.SLICE} == 0) return (size_t)v;" in slices
    chunk = text[text.index("size_t chunk_items("):text.index("template <int NOUT, class Launch>")]
    assert "((size_t)128 << 20) / (in_bytes_per_item ? in_bytes_per_item : 1)" in chunk and "if (c < 8192) c = 8192;" in chunk \
        and "if (c > 262144) c = 262144;" in chunk
    for name in set(et.WORKSPACE_CHUNK.values()) | {rt.CHUNK, rt.MAX_LAUNCH}:
        assert any(f'"{name}"' in source(f) for f in ("capi_staging.hpp", "capi_cascade.hpp", "capi_quantise.hpp", "capi_widen.hpp")), name


def test_every_batched_symbol_is_in_the_table_or_excluded_with_a_reason():
    batched = [n for n in la.SYMBOLS if "batch" in n]
    in_table = {e.symbol for e in ENTRIES}
    assert in_table <= set(batched), sorted(in_table - set(batched))

    def excluded(name):
        return [p for p in et.EXCLUDED if (name.endswith(p) if p.startswith("_") else name.startswith(p))]

    for name in batched:
        assert (name in in_table) != bool(excluded(name)), f"{name}: add it to entry_table.route_entries() (or, with a reason, to EXCLUDED)"
    # the exclusions are the converters on convert_call and the *_multi entries, and stay those
    assert sorted(et.EXCLUDED) == ["_multi", "labrador_ldpc_hard_to_llrs_batch_", "labrador_ldpc_llrs_to_hard_batch_",
                                   "labrador_ldpc_quantise_llrs_batch_", "labrador_ldpc_widen_llrs_batch_"]
    assert all(len(reason) > 20 for reason in et.EXCLUDED.values())


def test_every_entry_has_a_batch_on_every_route():
    """At most one entry of a symbol may lack the direct call (a frame past its byte count); routes 2 to 7 are never skipped.  The
    batches are where the arithmetic says (cases() asserts that as it picks them); the bit-sliced entries run on TM1536, those of
    TM1280 at slices of 16 as well; the workspace entries at a workspace chunk of 5."""
    no_direct = {}
    for e in ENTRIES:
        picked = rt.cases(e)
        ids = [c.route for c in picked]
        assert len(set(ids)) == len(ids)
        assert all(r in ids for r in ROUTES), (e.id, ids)
        for c in picked:
            if isinstance(c, rt.Unreachable):
                assert c.route == "r1" and c.reason, (c.id, "only the direct call may be out of reach")
                no_direct.setdefault(e.symbol, []).append(e.id)
        assert ("r6-ws" in ids) == (e.workspace is not None) and ("r6-16" in ids) == (e.bitsliced and e.code.name == "TM1280")
    assert all(len(v) <= 1 for v in no_direct.values()), no_direct
    bitsliced = {e.symbol for e in ENTRIES if e.bitsliced}
    assert bitsliced <= {e.symbol for e in ENTRIES if e.bitsliced and e.code.name == "TM1536"}
    assert {e.workspace for e in ENTRIES} == set(et.WORKSPACE_CHUNK) | {None}


@pytest.mark.parametrize("entry", ENTRIES, ids=[e.id for e in ENTRIES])
def test_buffer_descriptions_and_batches(entry):
    """The bytes per item the entry states are those of its pool rows and of its reference's rows; every batch of it meets
    call_routes.conditions at its committed seed."""
    pool, ref = entry.pool(), entry.reference()
    assert tuple(p[0].nbytes for p in pool) == entry.in_bytes
    assert tuple(ref[name][0].nbytes for name, _, _ in entry.results) == entry.out_bytes
    assert [name for name, _, _ in entry.results][:3] in (["output", "iters", "success"], ["codewords"])
    code = entry.code
    assert rt.total(entry, 3) == rt.in_pad(entry, 3) + rt.out_total(entry, 3) and rt.in_pad(entry, 3) % 16 == 0
    if "app" in ref:
        assert ref["app"].shape[1] == code.n() + code.punctured_bits() and entry.results[-1][0] == "app"
    for case in rt.cases(entry):
        if isinstance(case, rt.Unreachable):
            continue
        idx = rt.draw(case)
        assert idx.shape == (case.batch,) and 0 <= idx.min() and idx.max() < len(pool[0])
        assert np.array_equal(idx, rt.draw(case)), "the draw is not a function of the case and its seed"
        missing = rt.conditions(case, idx)
        assert not missing, f"{case.id} at seed {rt.seed_of(case)}: {missing}"
        if case.route in ("r4", "r6", "r6-16", "r6-ws", "r7-17", "r7-chunks", "r7-small"):
            assert len(case.starts) >= 2, case.id
    unknown = set(rt.RESEED) - {c.id for e in ENTRIES for c in rt.cases(e)}
    assert not unknown, unknown


def test_a_periodic_draw_is_refused():
    """pool length 8 against slices of 8: conditions() names the rows that repeat"""
    entry = next(e for e in ENTRIES if e.id == "decode_ms_soft_batch_f32-TC128")
    case = next(c for c in rt.cases(entry) if c.route == "r6")
    assert len(entry.pool()[0]) == 8
    missing = rt.conditions(case, np.arange(case.batch) % 8)
    assert any("rows from 8 on equal those from 0 on" in m for m in missing), missing
