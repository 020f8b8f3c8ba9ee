"""call_routes.py -- which way a batched call takes through the one host frame of the C ABI (batched_call in csrc/capi_frame.hpp,
host_pipeline and for_launch_slices in csrc/capi_staging.hpp, run_sharded), and one batch per way for every entry of
tests/entry_table.py.  TEST INFRASTRUCTURE ONLY.  Importing it touches no GPU.

The frame chooses from the call's memory mode, its byte count and the environment.  The arithmetic, restated from host_pipeline:
in_pad is input 1 padded to 16 bytes, plus input 2 if there is one, padded again; out_total the sum of the outputs, each padded to 16;
T = in_pad + out_total.

  r1  host, direct       T <= DIRECT_CALL_BYTES: the kernel writes (and may read) the mapped pinned block
  r2  host, small        T <= SMALL_CALL_BYTES: pinned staging, one device block, one synchronisation
  r3  host, one chunk    T > SMALL_CALL_BYTES, items <= chunk: pageable copies on the caller's stream
  r4  host, pipelined    T > SMALL_CALL_BYTES, items > LABRADOR_LDPC_HIP_CHUNK: two staging sets, three streams, a collector thread
  r5  device, one launch
  r6  device, slices     batch > LABRADOR_LDPC_HIP_MAX_LAUNCH: every slice starts at Buffers::from(f0)
  r7  device set         devices=[...]: every shard re-enters the frame at Buffers::from(f0) on a worker thread

host_pipeline asks for the small call BEFORE it looks at the chunk: a batch of T <= SMALL_CALL_BYTES is staged whole whatever
LABRADOR_LDPC_HIP_CHUNK says.  So the pipelined cases here size their chunk c -- a multiple of 8 -- by the entry: the smallest at
which the 2 c + c / 2 + 1 frames (three chunks, a ragged last one, staging set 0 used again) are past R3_MIN_BYTES.

The margins (R1_MAX_BYTES against DIRECT_CALL_BYTES, R2_MIN_BYTES, R3_MIN_BYTES) keep a batch from landing on the wrong side of a
threshold through the paddings; nothing else depends on them.  tests/test_call_routes_host.py holds the two thresholds and the slice
rule to the source text."""
import ctypes
import zlib

import numpy as np

from entry_table import WORKSPACE_CHUNK
import labrador_ldpc_amd as la

DIRECT_CALL_BYTES, SMALL_CALL_BYTES = 64 << 10, 1 << 20      # csrc/capi_staging.hpp
R1_MAX_BYTES, R2_MIN_BYTES, R2_MAX_BYTES, R3_MIN_BYTES = 48 << 10, 128 << 10, 512 << 10, 5 << 18
SLICE = 8                                                    # max_launch_frames(): at least 8, a multiple of 8
CHUNK, MAX_LAUNCH = "LABRADOR_LDPC_HIP_CHUNK", "LABRADOR_LDPC_HIP_MAX_LAUNCH"
WORKSPACE_CHUNK_FRAMES = 5
DEVICES = [0, 0]


def pad16(b):
    return (b + 15) // 16 * 16


def in_pad(entry, items):
    t = items * entry.in_bytes[0]
    if len(entry.in_bytes) == 2:
        t = pad16(t) + items * entry.in_bytes[1]
    return pad16(t)


def out_total(entry, items):
    return sum(pad16(items * b) for b in entry.out_bytes)


def total(entry, items):
    return in_pad(entry, items) + out_total(entry, items)


def default_chunk(entry):
    """chunk_items() without the variable: about 128 MiB of input, 8192 .. 262144 frames"""
    return min(max((128 << 20) // sum(entry.in_bytes), 8192), 262144)


def smallest(entry, least):
    """the smallest batch with T >= least"""
    b = max(1, least // total(entry, 1) - 2)
    while total(entry, b) < least:
        b += 1
    assert b == 1 or total(entry, b - 1) < least
    return b


def shard_starts(batch, parts):
    """(first, count) of every shard, asked of the library"""
    out = []
    for k in range(parts):
        first, count = ctypes.c_size_t(), ctypes.c_size_t()
        assert la.lib.labrador_ldpc_hip_shard_range(batch, parts, k, ctypes.byref(first), ctypes.byref(count)) == 0
        out.append((first.value, count.value))
    return out


class Case:
    """One batch of one entry on one route.  route: its id.  env: the variables of the call.  device: device tensors, else numpy arrays.
    devices: the device set of a host call, or None.  starts: every offset at which the route starts a slice, a chunk or a shard (0
    first)."""

    def __init__(self, entry, route, batch, env=None, device=False, devices=None, starts=(0,)):
        self.entry, self.route, self.batch, self.env, self.device, self.devices = entry, route, batch, dict(env or {}), device, devices
        self.starts = sorted(set(starts))
        assert self.starts[0] == 0 and self.starts[-1] < batch
        self.id = f"{entry.id}-{route}"


class Unreachable:
    def __init__(self, entry, route, reason):
        self.entry, self.route, self.reason, self.id = entry, route, reason, f"{entry.id}-{route}"


def pipelined_chunk(entry):
    c = SLICE
    while total(entry, 2 * c + c // 2 + 1) < R3_MIN_BYTES:
        c += SLICE
    return c


def cases(entry):
    """[Case | Unreachable] of an entry: one per route, and the further combinations of tests/test_gpu_call_routes.py"""
    out = []
    if total(entry, 1) > R1_MAX_BYTES:
        out.append(Unreachable(entry, "r1", f"one frame of {entry.code.name} is {total(entry, 1)} bytes: past the direct call's "
                                            f"{DIRECT_CALL_BYTES} or inside the margin above {R1_MAX_BYTES}"))
    else:
        b = smallest(entry, R1_MAX_BYTES + 1) - 1
        assert b >= 1 and total(entry, b) <= R1_MAX_BYTES < DIRECT_CALL_BYTES
        out.append(Case(entry, "r1", b))
        if total(entry, entry.g) <= R1_MAX_BYTES:            # one codeword group: one workgroup, which may hand back a completion ticket
            out.append(Case(entry, "r1-group", entry.g))
    b2 = smallest(entry, R2_MIN_BYTES)
    assert DIRECT_CALL_BYTES < R2_MIN_BYTES <= total(entry, b2) <= R2_MAX_BYTES < SMALL_CALL_BYTES and b2 <= default_chunk(entry)
    out.append(Case(entry, "r2", b2))
    b3 = smallest(entry, R3_MIN_BYTES)
    assert total(entry, b3) > SMALL_CALL_BYTES and b3 <= default_chunk(entry)
    out.append(Case(entry, "r3", b3))
    c = pipelined_chunk(entry)
    b4 = 2 * c + c // 2 + 1
    assert total(entry, b4) > SMALL_CALL_BYTES
    out.append(Case(entry, "r4", b4, {CHUNK: c}, starts=(0, c, 2 * c)))
    out.append(Case(entry, "r5", entry.g + 1, device=True))
    out.append(Case(entry, "r6", 2 * SLICE + 1, {MAX_LAUNCH: SLICE}, device=True, starts=(0, SLICE, 2 * SLICE)))
    if entry.bitsliced and entry.code.name == "TM1280":      # 16 codewords per group: slices of one group, 33 frames
        out.append(Case(entry, "r6-16", 33, {MAX_LAUNCH: 16}, device=True, starts=(0, 16, 32)))
    if entry.workspace is not None:                          # the workspace cuts every slice again, at its own stride
        w = WORKSPACE_CHUNK_FRAMES
        out.append(Case(entry, "r6-ws", 2 * SLICE + 1, {MAX_LAUNCH: SLICE, WORKSPACE_CHUNK[entry.workspace]: w}, device=True,
                        starts=[s + k for s in (0, SLICE, 2 * SLICE) for k in range(0, SLICE, w) if s + k < 2 * SLICE + 1]))
    out.append(Case(entry, "r7-small", b2, devices=DEVICES, starts=[f for f, _ in shard_starts(b2, len(DEVICES))]))
    # 17 frames at a chunk of 8: shards of 9 and 8 frames, each a small call of its own at an odd offset
    out.append(Case(entry, "r7-17", 2 * SLICE + 1, {CHUNK: SLICE}, devices=DEVICES,
                    starts=[f for f, _ in shard_starts(2 * SLICE + 1, len(DEVICES))]))
    # ... and shards that are pipelined themselves: every worker thread with its own staging sets and collector
    out.append(Case(entry, "r7-chunks", 2 * b4, {CHUNK: c}, devices=DEVICES,
                    starts=[f + k * c for f, n in shard_starts(2 * b4, len(DEVICES)) for k in range(-(-n // c))]))
    return out


# ---- the frames of a case -------------------------------------------------------------------------------------------------------------------
# The batch of a case is drawn from the entry's pool by a seeded index vector: seed 0 unless RESEED names another, found on the CPU
# (conditions() below) and committed here.
RESEED = {
    'decode_bf_batch-TC128-r5': 1,
    'decode_ms_batch_bf16-TC128-r6': 8, 'decode_ms_batch_bf16-TC128-r6-ws': 10,
    'decode_ms_batch_f16-TC128-r5': 1, 'decode_ms_batch_f16-TC128-r6': 2, 'decode_ms_batch_f16-TC128-r6-ws': 53,
    'decode_ms_batch_f32-TC128-r6': 6, 'decode_ms_batch_f32-TC128-r7-17': 1,
    'decode_ms_batch_f64-TC128-r6': 13, 'decode_ms_batch_i16-TC128-r6': 8, 'decode_ms_batch_i8-TC128-r6': 5,
    'decode_ms_batch_i8-variant64-TM1280-r6': 2, 'decode_ms_batch_i8-variant64-TM1280-r6-16': 2, 'decode_ms_batch_i8-variant64-TM1536-r6': 2,
    'decode_ms_bitsliced_hard_batch_i8-masked-TM1536-r6': 2, 'decode_ms_bitsliced_hard_batch_i8-unmasked-TM1536-r6': 2,
    'decode_ms_bitsliced_hard_corrected_batch_i8-masked-TM1536-r5': 1, 'decode_ms_bitsliced_hard_corrected_batch_i8-masked-TM1536-r6': 1,
    'decode_ms_bitsliced_hard_corrected_batch_i8-unmasked-TM1536-r6': 4,
    'decode_ms_bitsliced_quantised_batch_i8-TM1536-r6': 5, 'decode_ms_bitsliced_quantised_corrected_batch_i8-TM1536-r6': 8,
    'decode_ms_bitsliced_quantised_corrected_soft_batch_i8-TM1536-r6': 4, 'decode_ms_bitsliced_quantised_soft_batch_i8-TM1536-r6': 1,
    'decode_ms_bitsliced_soft_batch_i8-TM1536-r6': 2,
    'decode_ms_cascade_batch_bf16-TC128-r6': 3, 'decode_ms_cascade_batch_f16-TC128-r6': 1, 'decode_ms_cascade_batch_f16-TC128-r6-ws': 16,
    'decode_ms_cascade_batch_f32-TC128-r6': 4, 'decode_ms_cascade_batch_f32-TC128-r6-ws': 2,
    'decode_ms_cascade_batch_i16-TC128-r6-ws': 8, 'decode_ms_cascade_batch_i8-TC128-r6': 1, 'decode_ms_cascade_batch_i8-TC128-r6-ws': 8,
    'decode_ms_cascade_bitsliced_corrected_soft_batch_i8-TM1536-r6-ws': 1, 'decode_ms_cascade_bitsliced_quantised_batch_i8-TM1536-r6-ws': 36,
    'decode_ms_cascade_bitsliced_quantised_soft_batch_i8-TM1536-r6': 7, 'decode_ms_cascade_bitsliced_quantised_soft_batch_i8-TM1536-r6-ws': 10,
    'decode_ms_cascade_bitsliced_soft_batch_i8-TM1536-r6': 8, 'decode_ms_cascade_bitsliced_soft_batch_i8-TM1536-r6-ws': 4,
    'decode_ms_cascade_corrected_batch_f32-TC128-r6-ws': 7,
    'decode_ms_cascade_corrected_batch_i8-TM1280-r6-ws': 5, 'decode_ms_cascade_corrected_batch_i8-TM1280-r7-17': 1,
    'decode_ms_cascade_corrected_batch_i8-TM1536-r6': 1, 'decode_ms_cascade_corrected_batch_i8-TM1536-r6-ws': 2,
    'decode_ms_cascade_corrected_batch_i8-TM1536-r7-17': 1,
    'decode_ms_cascade_quantised_batch_i16-TC128-r6': 13, 'decode_ms_cascade_quantised_batch_i16-TC128-r6-ws': 39,
    'decode_ms_cascade_quantised_batch_i8-TC128-r6': 3, 'decode_ms_cascade_quantised_batch_i8-TC128-r6-ws': 11,
    'decode_ms_cascade_quantised_corrected_batch_i8-TM1280-r6': 3, 'decode_ms_cascade_quantised_corrected_batch_i8-TM1280-r6-ws': 3,
    'decode_ms_cascade_quantised_corrected_batch_i8-TM1280-r7-17': 1,
    'decode_ms_cascade_quantised_corrected_batch_i8-TM1536-r6': 27, 'decode_ms_cascade_quantised_corrected_batch_i8-TM1536-r6-ws': 13,
    'decode_ms_cascade_soft_batch_i16-TC128-r6': 4, 'decode_ms_cascade_soft_batch_i16-TC128-r6-ws': 1,
    'decode_ms_cascade_soft_batch_i8-TC128-r6': 8, 'decode_ms_cascade_soft_batch_i8-TC128-r6-ws': 8,
    'decode_ms_corrected_batch_f32-TC128-r6': 9, 'decode_ms_corrected_batch_i8-TM1280-r6': 3, 'decode_ms_corrected_batch_i8-TM1280-r6-16': 20,
    'decode_ms_corrected_soft_batch_f32-TC128-r6': 1,
    'decode_ms_layered_batch_bf16-TC128-r6': 12, 'decode_ms_layered_batch_f16-TC128-r5': 3, 'decode_ms_layered_batch_f16-TC128-r6': 3,
    'decode_ms_layered_corrected_batch_f16-TC128-r5': 1, 'decode_ms_layered_corrected_batch_f16-TC128-r6': 2,
    'decode_ms_layered_corrected_batch_f32-TC128-r6': 1, 'decode_ms_layered_corrected_soft_batch_bf16-TC128-r6': 2,
    'decode_ms_layered_fixed_batch_i16-TC128-r6': 2, 'decode_ms_layered_fixed_corrected_batch_i16-TC128-r5': 1,
    'decode_ms_layered_fixed_corrected_batch_i16-TC128-r6': 1, 'decode_ms_layered_fixed_corrected_batch_i8-TC128-r6': 2,
    'decode_ms_layered_fixed_corrected_soft_batch_i16-TC128-r6': 8, 'decode_ms_layered_fixed_corrected_soft_batch_i16-TC128-r7-17': 1,
    'decode_ms_layered_fixed_soft_batch_i16-TC128-r6': 1, 'decode_ms_layered_fixed_soft_batch_i8-TC128-r6': 5,
    'decode_ms_layered_quantised_batch_i16-TC128-r6': 2, 'decode_ms_layered_quantised_batch_i8-TC128-r6': 1,
    'decode_ms_layered_quantised_soft_batch_i16-TC128-r6': 1, 'decode_ms_layered_quantised_soft_batch_i8-TC128-r6': 7,
    'decode_ms_layered_soft_batch_bf16-TC128-r6': 9, 'decode_ms_layered_soft_batch_f16-TC128-r6': 4, 'decode_ms_layered_soft_batch_f32-TC128-r6': 1,
    'decode_ms_quantised_batch_i16-TC128-r6': 14, 'decode_ms_quantised_batch_i16-TC128-r6-ws': 27,
    'decode_ms_quantised_batch_i8-TC128-r6': 1, 'decode_ms_quantised_batch_i8-TC128-r6-ws': 28,
    'decode_ms_soft_batch_bf16-TC128-r6-ws': 3, 'decode_ms_soft_batch_f16-TC128-r6': 2, 'decode_ms_soft_batch_f16-TC128-r6-ws': 11,
    'decode_ms_soft_batch_f32-TC128-r6': 7, 'decode_ms_soft_batch_f64-TC128-r6': 1, 'decode_ms_soft_batch_i16-TC128-r6': 3,
    'decode_ms_soft_batch_i32-TC128-r6': 3, 'decode_ms_soft_batch_i8-TC128-r6': 5,
    # one codeword group
    'decode_ms_cascade_batch_f16-TC128-r1-group': 1, 'decode_ms_cascade_corrected_batch_f32-TC128-r1-group': 2,
    'decode_ms_cascade_quantised_batch_i16-TC128-r1-group': 1, 'decode_ms_cascade_soft_batch_i8-TC128-r1-group': 2,
    'decode_ms_layered_batch_bf16-TC128-r1-group': 1, 'decode_ms_layered_batch_f32-TC128-r1-group': 1,
    'decode_ms_layered_corrected_batch_f16-TC128-r1-group': 2, 'decode_ms_layered_corrected_batch_f32-TC128-r1-group': 3,
    'decode_ms_layered_fixed_corrected_soft_batch_i8-TC128-r1-group': 1, 'decode_ms_layered_soft_batch_f16-TC128-r1-group': 3,
    'decode_ms_quantised_batch_i16-TC128-r1-group': 3, 'decode_ms_soft_batch_f16-TC128-r1-group': 1,
    'decode_ms_soft_batch_i16-TC128-r1-group': 1, 'decode_ms_soft_batch_i32-TC128-r1-group': 1, 'decode_ms_soft_batch_i8-TC128-r1-group': 2,
}


def seed_of(case):
    return RESEED.get(case.id, 0)


def draw(case, seed=None):
    """pool indices [batch] of a case"""
    seed = seed_of(case) if seed is None else seed
    rng = np.random.default_rng([zlib.crc32(case.id.encode()), seed])
    return rng.integers(0, len(case.entry.pool()[0]), case.batch)


def conditions(case, idx):
    """What does NOT hold of the batch `idx` of a case (empty: all is well), from the CPU statement alone.  For every offset s at which
    the route starts a slice, chunk or shard, in EVERY result the expected rows from s on differ from the expected rows from 0 on
    and from those at the boundary before s, over the length of the piece that starts at s: a pointer that is not advanced, or is
    advanced by another buffer's stride or to the piece before, cannot then reproduce the right answer.  The batch holds a succeeding
    and a failing frame; a cascade's a frame of each stage; a masked one a frame whose mask changes its result."""
    entry, ref = case.entry, case.entry.reference()
    missing = []
    ends = case.starts[1:] + [case.batch]
    for k in range(1, len(case.starts)):
        s, length = case.starts[k], ends[k] - case.starts[k]
        for other in {0, case.starts[k - 1]}:
            for name, rows in ref.items():
                if rows[idx[s:s + length]].tobytes() == rows[idx[other:other + length]].tobytes():
                    missing.append(f"{name}: the {length} rows from {s} on equal those from {other} on")
    if "success" in ref:
        ok = ref["success"][idx]
        if not (ok == 1).any() or not (ok == 0).any():
            missing.append("no succeeding or no failing frame")
    if "stage" in ref and len(set(ref["stage"][idx].tolist())) != 2:
        missing.append("not a frame of each stage")
    if entry.masked:
        plain = entry.unmasked.reference()
        if not any((ref[name][idx] != plain[name][idx]).any() for name in ref):
            missing.append("no frame whose mask changes its result")
    return missing
