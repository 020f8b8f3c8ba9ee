"""A compile-time guard that needs no GPU: where the check messages of the deferred local edges are finished.

decode_ms_pair_kernel<8, float, 2 | 3> (build/csrc/decode_ms_f32_part_1.o) and <5, float, 2 | 3> (TM2048, `variant` 32,
decode_ms_f32_part_2.o) leave the last v_min3_f32 and the sign application (v_bitop3_b32) of K of a thread's 14 local edges out of
the VALU-bound end of the check phase and issue them at the next loop head, between the last early u read and the wait for the
previous pass's verdict, where the VALU of the whole CU idles (csrc/decode_ms_pair.hpp, DEFER; K = LDPC_PAIR_DEFER_LOCAL_F32 of
csrc/decode_ms_tuning.hpp).  Written as plain C++ the compiler sinks that work below the loop's exit branch, behind the wait, or could
hoist it back above the barrier; neither shows in any result.  A loop is a backward branch that spans exactly two s_barrier
(tools/loop_mix.py); per loop of both forms of both codes:

  * between the last ds_read_b64 of the head (those between the verdict's ds_read_b32 and the exit branch) and the first wait on
    lgkmcnt behind it there are at least K v_min3_f32 and at least K v_bitop3_b32;
  * from the check phase's last ds_write to the backward branch there are at most 16 - K v_bitop3_b32: the parent's loops held 14 to
    16 there, one per local edge and up to two of the last exchanged row.

Opcode placement only: what the instructions compute is the business of tests/test_gpu_pair_deferred.py."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (object, code number in the kernel's mangled name)
KERNELS = {"TM8192": ("decode_ms_f32_part_1.o", 8), "TM2048": ("decode_ms_f32_part_2.o", 5)}
LOCAL_EDGES = 14                                 # per thread, both codes (the rate-1/2 prototype: 7 local blocks, two indices)
PARENT_TAIL_BITOP3 = 16                          # the most any loop held behind its last ds_write before the deferral


def _tuned(name):
    text = open(os.path.join(ROOT, "labrador_ldpc_amd", "csrc", "decode_ms_tuning.hpp")).read()
    return int(re.search(rf"^#define {name} (-?\d+)\s*$", text, re.M).group(1))


@pytest.fixture(scope="module")
def deferred():
    """K of the library build: every instantiation with early u reads has the same"""
    assert _tuned("LDPC_PAIR_DEFER_LOCAL") == -1 and _tuned("LDPC_PAIR_EARLY_U") == -1 and _tuned("LDPC_PAIR_EARLY_U_F32") > 0
    k = _tuned("LDPC_PAIR_DEFER_LOCAL_F32")
    assert 0 <= k <= LOCAL_EDGES
    return k


@pytest.fixture(scope="module")
def built_objects():
    """The objects are built the way tests/test_kernel_shape.py builds them (`make` is a no-op when they are current)."""
    import subprocess
    if not os.path.exists("/opt/rocm/bin/hipcc") or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.fail("hipcc / llvm-objdump missing: the deferred-edge guard cannot run in this environment")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "labrador_ldpc_amd", "csrc"), "-j", str(min(8, os.cpu_count() or 1))],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.fixture(scope="module", params=sorted(KERNELS))
def pair_loops(request, built_objects):
    """{form: [instruction list of each loop]} of the two hard-output f32 pair kernels of one code"""
    import loop_mix
    name, code = KERNELS[request.param]
    found = {}
    for kernel, spans in loop_mix.spans_of(os.path.join(ROOT, "build", "csrc", name), f"decode_ms_pair_kernelILi{code}EfLi").items():
        found[int(re.search(rf"decode_ms_pair_kernelILi{code}EfLi(\d)E", kernel).group(1))] = [sp for _, _, sp in spans]
    assert set(found) == {2, 3}, sorted(found)
    # four quarter bodies x two clamp modes, each at least once (the compiler's loop rotation adds backward branches of the same loop)
    assert all(len(v) >= 8 for v in found.values()), {k: len(v) for k, v in found.items()}
    return found


def _count(instrs, opcode):
    return sum(1 for t in instrs if t.startswith(opcode))


def test_the_deferred_work_sits_between_the_last_early_read_and_the_verdicts_wait(pair_loops, deferred):
    for form, loops in pair_loops.items():
        for sp in loops:
            verdicts = [i for i, t in enumerate(sp) if t.startswith("ds_read_b32")]
            assert len(verdicts) == 1, f"form {form}: {len(verdicts)} ds_read_b32 in an iteration loop"
            branch = next(i for i in range(verdicts[0], len(sp)) if sp[i].startswith("s_cbranch"))
            reads = [i for i in range(verdicts[0] + 1, branch) if sp[i].startswith("ds_read_b64")]
            assert reads, f"form {form}: no early u read at the loop head"
            wait = next(i for i in range(reads[-1] + 1, len(sp)) if sp[i].startswith("s_waitcnt") and "lgkmcnt" in sp[i])
            assert wait < branch, f"form {form}: the verdict is not waited for in front of the exit branch"
            window = sp[reads[-1] + 1:wait]
            got = (_count(window, "v_min3_f32"), _count(window, "v_bitop3_b32"))
            assert got[0] >= deferred and got[1] >= deferred, \
                f"form {form}: {got[0]} v_min3_f32 and {got[1]} v_bitop3_b32 under the verdict's round trip, {deferred} edges deferred"


def test_the_end_of_the_check_phase_holds_correspondingly_fewer(pair_loops, deferred):
    for form, loops in pair_loops.items():
        for sp in loops:
            last_write = max(i for i, t in enumerate(sp) if t.startswith("ds_write"))
            tail = _count(sp[last_write + 1:], "v_bitop3_b32")
            assert tail <= PARENT_TAIL_BITOP3 - deferred, \
                f"form {form}: {tail} v_bitop3_b32 behind the check phase's last ds_write, {deferred} edges deferred"
