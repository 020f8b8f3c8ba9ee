"""A compile-time guard that needs no GPU: the head of the iteration loops of the hard-output f32 pair kernels.

decode_ms_pair_kernel<8, float, 2 | 3> (build/csrc/decode_ms_f32_part_1.o) and <5, float, 2 | 3> (TM2048, `variant` 32,
decode_ms_f32_part_2.o) issue the variable phase's exchanged-u reads right behind the read of the previous pass's verdict word and
wait for the verdict alone (csrc/decode_ms_pair.hpp, EARLY): one LDS round trip per iteration, not two in series.  The reads are
inline asm, so the compiler does not know that their destination registers are pending, and the verdict is a value out of an asm,
which the compiler takes for divergent.  A loop is a backward branch that spans exactly two s_barrier (tools/loop_mix.py); per loop:

  * exactly one ds_read_b32, the verdict;
  * at least one ds_read_b64 / ds_read2* between the verdict and the next s_cbranch*;
  * the first wait on lgkmcnt behind the verdict leaves at least one operation outstanding;
  * that branch tests a scalar condition (s_cbranch_scc* / s_cbranch_vcc*) and no s_and_saveexec lies in front of it: the loop exit
    is no EXEC-masked region;
  * no scalar memory load in the loop (lgkmcnt returns in order for LDS alone: a counted wait with one outstanding would be unsafe).

And on every path from the verdict on -- through the variable phase, and out of the loop to the drain in front of the epilogue -- no
instruction names a destination register of an early read before a wait on lgkmcnt that covers the read: the k-th of E early reads
is back once no more than E - 1 - k operations are outstanding.  A use, a copy or a spill before that would take a stale value;
a write on the exit path, where the registers are dead to the compiler, would be overwritten by the returning read."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (object, code number in the kernel's mangled name)
KERNELS = {"TM8192": ("decode_ms_f32_part_1.o", 8), "TM2048": ("decode_ms_f32_part_2.o", 5)}
WIDE_READ = ("ds_read_b64", "ds_read2")


@pytest.fixture(scope="module")
def built_objects():
    """The objects are built the way tests/test_kernel_shape.py builds them (`make` is a no-op when they are current)."""
    import subprocess
    if not os.path.exists("/opt/rocm/bin/hipcc") or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.fail("hipcc / llvm-objdump missing: the loop-head guard cannot run in this environment")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "labrador_ldpc_amd", "csrc"), "-j", str(min(8, os.cpu_count() or 1))],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.fixture(scope="module", params=sorted(KERNELS))
def pair_kernels(request, built_objects):
    """{form: (the kernel's instructions as (text, index of the branch target or None), [(first, last) of each loop])}"""
    import disasm
    import loop_mix
    name, code = KERNELS[request.param]
    obj = os.path.join(ROOT, "build", "csrc", name)
    bodies = disasm.kernels(obj)
    found = {}
    for kernel, spans in loop_mix.spans_of(obj, f"decode_ms_pair_kernelILi{code}EfLi").items():
        m = re.search(rf"decode_ms_pair_kernelILi{code}EfLi(\d)E", kernel)
        body = bodies[kernel]
        index = {addr: i for i, (addr, _, _) in enumerate(body)}
        instrs = [(text, index.get(body[0][0] + tgt) if tgt is not None else None) for _, text, tgt in body]
        for first, last, sp in spans:
            assert [t for t, _ in instrs[first:last + 1]] == sp          # the two tools number the instructions alike
        found[int(m.group(1))] = (instrs, [(first, last) for first, last, _ in spans])
    assert set(found) == {2, 3}, sorted(found)
    # four quarter bodies x two clamp modes, each at least once (the compiler's loop rotation adds backward branches of the same loop)
    assert all(len(loops) >= 8 for _, loops in found.values()), {k: len(v[1]) for k, v in found.items()}
    return found


def _loops(pair_kernels):
    for form, (instrs, loops) in pair_kernels.items():
        for first, last in loops:
            yield form, instrs, first, last


def _head(instrs, first, last):
    """(index of the verdict's read, index of the next conditional branch)"""
    verdicts = [i for i in range(first, last + 1) if instrs[i][0].startswith("ds_read_b32")]
    assert len(verdicts) == 1, f"{len(verdicts)} ds_read_b32 in an iteration loop"
    branch = next(i for i in range(verdicts[0], last + 1) if instrs[i][0].startswith("s_cbranch"))
    return verdicts[0], branch


def _lgkmcnt(text):
    m = re.search(r"lgkmcnt\((\d+)\)", text) if text.startswith("s_waitcnt") else None
    return int(m.group(1)) if m else None


def _vgprs(text):
    regs = set()
    for lo, hi in re.findall(r"\bv\[(\d+):(\d+)\]", text):
        regs |= set(range(int(lo), int(hi) + 1))
    return regs | {int(r) for r in re.findall(r"\bv(\d+)\b", text)}


def test_the_u_reads_are_issued_before_the_verdict_is_tested(pair_kernels):
    for form, instrs, first, last in _loops(pair_kernels):
        verdict, branch = _head(instrs, first, last)
        between = [t for t, _ in instrs[verdict + 1:branch]]
        assert any(t.startswith(WIDE_READ) for t in between), f"form {form}: no u read between the verdict's read and its branch"
        waits = [n for n in (_lgkmcnt(t) for t, _ in instrs[verdict + 1:last + 1]) if n is not None]
        assert waits and waits[0] >= 1, f"form {form}: the verdict's wait drains lgkmcnt: {waits[:1]}"


def test_the_loop_exit_is_a_scalar_branch(pair_kernels):
    for form, instrs, first, last in _loops(pair_kernels):
        verdict, branch = _head(instrs, first, last)
        assert instrs[branch][0].startswith(("s_cbranch_scc", "s_cbranch_vcc")), f"form {form}: {instrs[branch][0]}"
        assert not any(t.startswith("s_and_saveexec") for t, _ in instrs[verdict:branch]), f"form {form}: EXEC-masked loop exit"


def test_no_scalar_memory_load_in_the_loops(pair_kernels):
    for form, instrs, first, last in _loops(pair_kernels):
        loads = [t for t, _ in instrs[first:last + 1] if t.startswith(("s_load_", "s_buffer_load_"))]
        assert not loads, f"form {form}: scalar memory load inside an iteration loop: {loads[:3]}"


def test_no_pending_register_is_touched_before_its_wait(pair_kernels):
    for form, instrs, first, last in _loops(pair_kernels):
        verdict, branch = _head(instrs, first, last)
        early = [_vgprs(t.split(",")[0]) for t, _ in instrs[verdict + 1:branch] if t.startswith(WIDE_READ)]
        n_early = len(early)
        assert all(len(r) == 2 for r in early) and len(set().union(*early)) == 2 * n_early, early
        # the reads issued up to each point of the head, then every path from the branch on; state = outstanding early reads' registers
        pending, issued = set(), 0
        for i in range(verdict + 1, branch + 1):
            t = instrs[i][0]
            if t.startswith(WIDE_READ):
                assert not (_vgprs(t) - early[issued]) & pending, f"form {form}: {t}"
                pending |= early[issued]
                issued += 1
                continue
            n = _lgkmcnt(t)
            if n is not None and n < issued:
                pending &= set().union(*early[issued - n:issued]) if n > 0 else set()
            assert not _vgprs(t) & pending, f"form {form}: `{t}` names the destination of a pending u read (head)"
        todo, seen = [(branch + 1, frozenset(pending)), (instrs[branch][1], frozenset(pending))], set()
        while todo:
            i, pend = todo.pop()
            while pend and (i, pend) not in seen:
                seen.add((i, pend))
                assert i is not None and i < len(instrs), f"form {form}: a path from the loop head leaves the kernel's listing"
                t, target = instrs[i]
                n = _lgkmcnt(t)
                if n is not None and n < n_early:
                    pend = frozenset(set().union(*early[n_early - n:]) & pend) if n > 0 else frozenset()
                assert not _vgprs(t) & pend, f"form {form}: `{t}` (instruction {i}) names the destination of a pending u read"
                assert not t.startswith(("s_endpgm", "s_setpc", "s_swappc")), f"form {form}: {t} with u reads pending"
                if t.startswith("s_branch"):
                    i = target
                else:
                    if t.startswith("s_cbranch"):
                        todo.append((target, pend))
                    i += 1
