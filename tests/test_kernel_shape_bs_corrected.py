"""What the correction step may cost the bit-sliced kernels in registers, read from the built objects without a GPU:
between the first and the last ds_bpermute_b32 of a kernel (TM1280: DPP move) -- the definition of "the iteration" of
tests/test_kernel_shape.py -- every corrected kernel carries at most the scratch instructions of the PLAIN kernel of the same code,
counted here from decode_ms_bs_{1,2}.o, plus 4: two more spilled values, which is what the step's temporaries can cost at the
register peak.  The plain two-wave kernels carry none, so theirs is 0 + 4."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def kernels():
    """{object stem: {kernel symbol: [instruction text]}} of the plain and the corrected bit-sliced objects (`make` first: a no-op when
    they are current)."""
    if not os.path.exists("/opt/rocm/bin/hipcc") or not os.path.exists(f"{LLVM}/llvm-objdump"):
        pytest.fail("hipcc / llvm-objdump missing: the kernel-shape guards cannot run in this environment")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "labrador_ldpc_amd", "csrc"), "-j", str(min(8, os.cpu_count() or 1))],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    tmp = tempfile.mkdtemp()
    out = {}
    for stem in ("decode_ms_bs_1", "decode_ms_bs_2", "decode_ms_bs_corrected_1", "decode_ms_bs_corrected_2"):
        obj = os.path.join(ROOT, "build", "csrc", stem + ".o")
        subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={tmp}/{stem}.fat", obj, "/dev/null"])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={tmp}/{stem}.fat", f"--output={tmp}/{stem}.co", "--unbundle"])
        cur, table = None, {}
        for line in subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", f"{tmp}/{stem}.co"], text=True).split("\n"):
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = m.group(1)
                table[cur] = []
            elif cur and "\t" in line:
                table[cur].append(line.split("//")[0].strip())
        out[stem] = table
    return out


def iteration(body, code):
    move = "v_mov_b32_dpp" if code == 3 else "ds_bpermute_b32"            # TM1280 rotates lanes with DPP quad moves
    at = [i for i, t in enumerate(body) if t.startswith(move)]
    assert len(at) >= 100
    return body[at[0]:at[-1]]


def scratch_in_iteration(body, code):
    return sum(1 for t in iteration(body, code) if t.startswith("scratch_"))


def test_corrected_kernels_carry_at_most_the_plain_kernels_scratch_plus_four(kernels):
    plain = {}
    for unit in (1, 2):
        for name, body in kernels[f"decode_ms_bs_{unit}"].items():
            m = re.search(r"decode_ms_bs_(split_)?kernelILi(\d)E", name)
            if m:
                plain[int(m.group(2))] = scratch_in_iteration(body, int(m.group(2)))
    assert sorted(plain) == [3, 4, 5, 6, 7, 8]                             # TM1280 .. TM8192, lockstep forms
    seen = []
    for unit in (1, 2):
        for name, body in kernels[f"decode_ms_bs_corrected_{unit}"].items():
            m = re.search(r"decode_ms_bsc_(split_)?kernelILi(\d)ELi(\d)E", name)
            if not m:
                continue
            code, mulbits = int(m.group(2)), int(m.group(3))
            assert bool(m.group(1)) == (code in (3, 6)), name              # the two-wave form for TM1280 and TM5120, and only for them
            n = scratch_in_iteration(body, code)
            print(f"{name}: {n} scratch instructions inside the iteration (plain kernel of the code: {plain[code]})")
            assert n <= plain[code] + 4, f"{name}: {n} scratch instructions inside the iteration, the plain kernel has {plain[code]}"
            loop = iteration(body, code)
            assert sum(1 for t in loop if t.startswith("v_bitop3_b32")) > 0.5 * len(loop) - 200, name     # ... which is Boolean arithmetic
            seen.append((code, mulbits))
    assert sorted(seen) == [(c, m) for c in (3, 4, 5, 6, 7, 8) for m in (0, 4, 8)]


def test_the_new_names_do_not_contain_the_plain_kernels(kernels):
    """tests/test_kernel_shape.py counts the plain kernels by name in decode_ms_bs_{1,2}.o; the corrected kernels must neither be
    counted there nor carry those names."""
    for unit in (1, 2):
        for name in kernels[f"decode_ms_bs_corrected_{unit}"]:
            assert "decode_ms_bs_kernel" not in name and "decode_ms_bs_split_kernel" not in name and "refill_kernel" not in name, name
        for name in kernels[f"decode_ms_bs_{unit}"]:
            assert "decode_ms_bsc_" not in name, name


def test_resources_beside_the_plain_kernels(kernels):
    """Registers, spills and LDS as DESIGN.md 4.14 tabulates them: LDS is the plain kernel's (the step needs none), the forms without a
    multiply keep the plain kernels' register budget, and only the rate-1/2 forms with one are built for two waves per SIMD."""
    import kernel_resources
    rows = {}
    for obj, dem, v, sp, s, lds, scr in kernel_resources.resources("build/csrc/decode_ms_bs*.o"):
        m = re.search(r"decode_ms_(bsc?)_(split_)?kernel<(\d)(?:, (\d))?>", dem)
        if m:
            rows[(m.group(1), int(m.group(3)), int(m.group(4) or -1))] = (int(v), int(sp), int(lds))
    for code in (3, 4, 5, 6, 7, 8):
        pv, psp, plds = rows[("bs", code, -1)]
        for mulbits in (0, 4, 8):
            v, sp, lds = rows[("bsc", code, mulbits)]
            print(f"code {code} mulbits {mulbits}: vgpr {v} spill {sp} lds {lds}   (plain: vgpr {pv} spill {psp} lds {plds})")
            assert lds == plds
            if code in (5, 8):
                assert v <= (168 if mulbits == 0 else 256)
            if mulbits == 0:
                assert sp <= psp + 2
