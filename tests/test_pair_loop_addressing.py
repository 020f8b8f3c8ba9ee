"""A compile-time guard that needs no GPU: the iteration loops of the TM8192 f32 pair kernels form no LDS address.

decode_ms_pair_kernel<8, float, 2> and <8, float, 3> (build/csrc/decode_ms_f32_part_1.o, which the scratch guard of
tests/test_kernel_shape.py does not look at) keep the exchanged edges' wired addresses and the variable phase's own position in
registers across the iterations (csrc/decode_ms_pair.hpp, HOIST).  Formed per phase they were 37 of the 290 VALU instructions of a
VALU-bound loop: per rotation read a v_add_u32 and a v_and_b32 with the quarter-wrap literal 0x7f8 (= 4 * M / 4 - 8), and a v_or_b32
/ v_add_u32 of 0x10000 for every block that lies past the 16-bit offset of a ds instruction.

A loop is a backward branch that spans exactly two s_barrier (tools/loop_mix.py).  Per loop: no scratch instruction, no v_and_b32
with 0x7f8, no v_or_b32 / v_add_u32 whose literal is a block offset (a multiple of 0x800 at or above 0x10000).

Counts.  The clamp-free loops of the form-2 kernel (no v_min_f32; the loops the benchmark runs) hold at most 264 VALU instructions:
the parent had 279-291 on this toolchain, compile-only trials of the hoist reached 252-263, and the bound is that with one
instruction of slack (this build: 253-257).  The other copies of the loop differ from those in their ARITHMETIC alone -- the clamped
copy has the eight v_min_f32 of the FLT_MAX clamp and the compare / select form of the self-correction (v_cmp + v_cndmask + a
wider v_bitop3 share instead of v_fma + v_med3: 38 more in the parent, 328 against 290), the form-3 kernel's clamp-free copy a
v_mul_legacy + v_add instead of the v_fma (30 more, one per edge) -- so each of them is held to 264 plus its own surplus in the
arithmetic instruction classes over the form-2 clamp-free copy, computed here from the disassembly; whatever it spends outside
those classes (moves, integer adds, masks: what an address costs) counts against the 264 in full.  (The figure 264 was set from the
form-2 loops; held as a flat bound it would refuse the form-3 clamp-free copy for the 30 instructions of its self-correction
form, 283-287 in all, none of which is addressing.)

The gate of the hoist is on the message type and the output form, not on the code, so the TM2048 f32 pair kernels (`variant` 32,
build/csrc/decode_ms_f32_part_2.o; quarter-wrap literal 0x1f8, no block past 64 KB) are adopted with it and held to the same
assertions: same prototype shape, the same 30 edges per thread, 253-259 instructions in their clamp-free form-2 loops against 264-280
before."""
import collections
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

BOUND = 264
# the float / logic classes of the check and variable phases' arithmetic; everything else a loop issues on the VALU is bookkeeping
ARITH = re.compile(r"^v_(min|max|med3|fma|fmac|mul|add_f32|sub_f32|cmp\w*_f32|cndmask|bitop3)")


# (object, code number in the kernel's mangled name, quarter-wrap literal 4 * M / 4 - 8)
KERNELS = {"TM8192": ("decode_ms_f32_part_1.o", 8, 0x7f8), "TM2048": ("decode_ms_f32_part_2.o", 5, 0x1f8)}


@pytest.fixture(scope="module")
def built_objects():
    """The objects are built the way tests/test_kernel_shape.py builds them (`make` is a no-op when they are current)."""
    import subprocess
    if not os.path.exists("/opt/rocm/bin/hipcc") or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.fail("hipcc / llvm-objdump missing: the loop-addressing guard cannot run in this environment")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "labrador_ldpc_amd", "csrc"), "-j", str(min(8, os.cpu_count() or 1))],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.fixture(scope="module", params=sorted(KERNELS))
def pair_loops(request, built_objects):
    """({form: [instruction list of each loop]}, quarter-wrap literal) of the two hard-output f32 pair kernels of one code"""
    import loop_mix
    name, code, wrap = KERNELS[request.param]
    obj = os.path.join(ROOT, "build", "csrc", name)
    found = {}
    for kernel, spans in loop_mix.spans_of(obj, f"decode_ms_pair_kernelILi{code}EfLi").items():
        m = re.search(rf"decode_ms_pair_kernelILi{code}EfLi(\d)E", kernel)
        found[int(m.group(1))] = [sp for _, _, sp in spans]
    assert set(found) == {2, 3}, sorted(found)
    # four quarter bodies x two clamp modes, each at least once (the compiler's loop rotation adds backward branches of the same loop)
    assert all(len(v) >= 8 for v in found.values()), {k: len(v) for k, v in found.items()}
    return found, wrap


def _valu(sp):
    return [t for t in sp if t.startswith("v_")]


def _arith(sp):
    return sum(1 for t in _valu(sp) if ARITH.match(t))


def _clamp_free(sp):
    return not any(t.startswith("v_min_f32") for t in sp)


def test_no_address_is_formed_inside_an_iteration_loop(pair_loops):
    pair_loops, wrap = pair_loops
    for form, loops in pair_loops.items():
        for sp in loops:
            assert not any(t.startswith("scratch_") for t in sp), f"form {form}: scratch traffic inside an iteration loop"
            wraps = [t for t in sp if t.startswith("v_and_b32") and re.search(rf"\b{wrap:#x}\b", t)]
            assert not wraps, f"form {form}: quarter-wrap mask inside an iteration loop: {wraps[:3]}"
            blocks = [t for t in sp if t.startswith(("v_or_b32", "v_add_u32"))
                      and any(int(x, 16) >= 0x10000 and int(x, 16) % 0x800 == 0 for x in re.findall(r"\b0x[0-9a-f]+\b", t))]
            assert not blocks, f"form {form}: block offset formed inside an iteration loop: {blocks[:3]}"


def test_valu_instructions_per_iteration(pair_loops):
    pair_loops, _ = pair_loops
    free2 = [sp for sp in pair_loops[2] if _clamp_free(sp)]
    assert free2 and any(not _clamp_free(sp) for sp in pair_loops[2]) and any(_clamp_free(sp) for sp in pair_loops[3])
    report = collections.Counter()
    for sp in free2:
        report[("form 2", "clamp-free", len(_valu(sp)))] += 1
        assert len(_valu(sp)) <= BOUND, f"form 2, clamp-free loop: {len(_valu(sp))} VALU instructions"
    # the full loop of a quarter body is the copy with the most arithmetic (a rotated copy's backward branch can span less)
    arith_ref = max(_arith(sp) for sp in free2)
    for form, loops in pair_loops.items():
        for sp in loops:
            surplus = _arith(sp) - arith_ref
            report[(f"form {form}", "clamp-free" if _clamp_free(sp) else "clamped", len(_valu(sp)), f"bound {BOUND + surplus}")] += 1
            assert len(_valu(sp)) <= BOUND + surplus, \
                f"form {form}, {'clamp-free' if _clamp_free(sp) else 'clamped'} loop: {len(_valu(sp))} VALU instructions, {surplus} of them its form's own arithmetic"
    print(sorted(report.items()))
