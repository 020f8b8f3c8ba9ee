"""What the corrected soft form costs the bit-sliced kernels, read from the built objects with
tools/kernel_resources.py and the disassembly, without a GPU: each of the twelve kernels -- four one-wave codes, three multiplier widths
-- exists exactly once, in the unit its plan names; uses at most 256 VGPRs; carries inside the iteration (from the first to the last
ds_bpermute_b32) at most the scratch instructions of the PLAIN kernel of its code plus 4 (the rule of DESIGN.md 4.14); and with the
waves it is compiled for on each of a CU's four SIMDs fits the CU's 160 KB of LDS.  Its name cannot be taken for a plain, a corrected
or a soft kernel's by the tests that find those by name."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LLVM = "/opt/rocm/lib/llvm/bin"

CODES = {4: "TM1536", 5: "TM2048", 7: "TM6144", 8: "TM8192"}
MULBITS = (0, 4, 8)
# waves per SIMD a form is compiled for: the soft plan's (BsPlan::SOFT_WAVES_PER_SIMD), every form
WAVES = {4: 1, 5: 2, 7: 1, 8: 2}
UNIT = {4: 2, 5: 1, 7: 2, 8: 1}                              # BsPlan::UNIT
LDS_PER_CU = 163840
FORBIDDEN = ("decode_ms_bs_kernel", "decode_ms_bs_split_kernel", "refill_kernel", "decode_ms_bsc_", "decode_ms_bsa_")
OBJECTS = ("decode_ms_bs_corrected_soft_1.o", "decode_ms_bs_corrected_soft_2.o")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists("/opt/rocm/bin/hipcc") or not os.path.exists(f"{LLVM}/llvm-objdump"):
        pytest.fail("hipcc / llvm-objdump missing: the kernel-shape guards cannot run in this environment")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "labrador_ldpc_amd", "csrc"), "-j", str(min(8, os.cpu_count() or 1))],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.fixture(scope="module")
def rows(built):
    """[(object, demangled name, vgprs, spilled, lds)] of every kernel of the bit-sliced objects"""
    import kernel_resources
    return [(obj, dem, int(v), int(sp), int(lds)) for obj, dem, v, sp, s, lds, scr in kernel_resources.resources("build/csrc/decode_ms_bs*.o")]


@pytest.fixture(scope="module")
def bodies(built):
    """{object stem: {kernel symbol: [instruction text]}} of the plain and the corrected soft objects"""
    tmp = tempfile.mkdtemp()
    out = {}
    for stem in ("decode_ms_bs_1", "decode_ms_bs_2", "decode_ms_bs_corrected_soft_1", "decode_ms_bs_corrected_soft_2"):
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


def test_twelve_kernels_each_once_in_its_unit_within_registers_and_lds(rows):
    seen, soft = {}, {}
    for obj, dem, v, sp, lds in rows:
        m = re.search(r"decode_ms_bsca_kernel<(\d), (\d)>", dem)
        if m:
            key = (int(m.group(1)), int(m.group(2)))
            assert obj in OBJECTS, (obj, dem)
            assert key not in seen, f"{dem} is built twice"
            seen[key] = (obj, v, sp, lds)
        m = re.search(r"decode_ms_bsa_kernel<(\d)>", dem)
        if m:
            soft[int(m.group(1))] = (v, sp, lds)
    assert sorted(seen) == [(c, m) for c in sorted(CODES) for m in MULBITS], sorted(seen)
    for (code, mulbits), (obj, v, sp, lds) in sorted(seen.items()):
        sv, ssp, slds = soft[code]
        print(f"{CODES[code]} mulbits {mulbits}: vgpr {v} spill {sp} lds {lds} at {WAVES[code]} waves/SIMD ({obj})   plain soft: vgpr {sv} spill {ssp} lds {slds}")
        assert obj == f"decode_ms_bs_corrected_soft_{UNIT[code]}.o"
        assert v <= 256, f"{CODES[code]}/{mulbits}: {v} VGPRs"
        assert lds * 4 * WAVES[code] <= LDS_PER_CU, f"{CODES[code]}/{mulbits}: {lds} bytes of LDS x {4 * WAVES[code]} waves per CU"
        assert lds == slds                                   # (the step needs no LDS: the soft layout's)


def iteration(body):
    at = [i for i, t in enumerate(body) if t.startswith("ds_bpermute_b32")]
    assert len(at) >= 100
    return body[at[0]:at[-1]]


def test_scratch_inside_the_iteration_is_at_most_the_plain_kernels_plus_four(bodies):
    plain = {}
    for unit in (1, 2):
        for name, body in bodies[f"decode_ms_bs_{unit}"].items():
            m = re.search(r"decode_ms_bs_kernelILi(\d)E", name)
            if m and int(m.group(1)) in CODES:
                plain[int(m.group(1))] = sum(1 for t in iteration(body) if t.startswith("scratch_"))
    assert sorted(plain) == sorted(CODES)
    seen = []
    for unit in (1, 2):
        for name, body in bodies[f"decode_ms_bs_corrected_soft_{unit}"].items():
            m = re.search(r"decode_ms_bsca_kernelILi(\d)ELi(\d)E", name)
            if not m:
                continue
            code, mulbits = int(m.group(1)), int(m.group(2))
            loop = iteration(body)
            n = sum(1 for t in loop if t.startswith("scratch_"))
            print(f"{name}: {n} scratch instructions inside the iteration (plain kernel of the code: {plain[code]})")
            assert n <= plain[code] + 4, f"{name}: {n} scratch instructions inside the iteration, the plain kernel has {plain[code]}"
            assert sum(1 for t in loop if t.startswith("v_bitop3_b32")) > 0.5 * len(loop) - 200, name     # ... which is Boolean arithmetic
            seen.append((code, mulbits))
    assert sorted(seen) == [(c, m) for c in sorted(CODES) for m in MULBITS]


def test_the_new_names_are_nobody_elses(rows):
    seen = 0
    for obj, dem, v, sp, lds in rows:
        if obj in OBJECTS:
            seen += 1
            assert "decode_ms_bsca_kernel<" in dem and not any(f in dem for f in FORBIDDEN), dem
        else:
            assert "decode_ms_bsca_" not in dem, (obj, dem)                 # (the other objects keep the kernels they had)
    assert seen == 12
    assert not any(o.startswith("decode_ms_bs_soft_") for o in OBJECTS)     # (tests/test_kernel_shape_bs_soft.py counts four kernels there)
