"""What the packed hard-decision loader costs the bit-sliced kernels, read from the built objects with
tools/kernel_resources.py, without a GPU: each of the sixteen kernels -- four one-wave codes, the plain form and three multiplier widths
of the corrected one -- exists exactly once, in the object of its code's unit; its VGPR count allows the waves per SIMD it is built
for; its LDS is the plain kernel's of the code; it has no more spilled registers than the i8-source kernel of the same form; and its
name cannot be taken for another kernel's by the tests that find those by name.  The metadata only: no instruction text is read."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LLVM = "/opt/rocm/lib/llvm/bin"

CODES = {4: "TM1536", 5: "TM2048", 7: "TM6144", 8: "TM8192"}
MULBITS = (0, 4, 8)
UNIT = {4: 2, 5: 1, 7: 2, 8: 1}                              # BsPlan::UNIT
PLAN_WAVES = {4: 2, 5: 3, 7: 2, 8: 3}                        # BsPlan::WAVES_PER_SIMD
RATE12 = (5, 8)
VGPRS_PER_SIMD = 512
FORBIDDEN = ("decode_ms_bs_kernel", "decode_ms_bs_split_kernel", "refill_kernel", "decode_ms_bsc_", "decode_ms_bsa_", "decode_ms_bsca_",
             "decode_ms_bsq_", "decode_ms_bsqc_", "decode_ms_bsqa_", "decode_ms_bsqca_")
OBJECTS = ("decode_ms_bs_hard_1.o", "decode_ms_bs_hard_2.o")


def waves(code, mulbits):
    """waves per SIMD a form is compiled for: mulbits None is the plain form (the plan's), else corrected_waves_per_simd()"""
    return 2 if mulbits and code in RATE12 else PLAN_WAVES[code]


@pytest.fixture(scope="module")
def rows():
    """[(object, demangled name, vgprs, spilled, lds)] of every kernel of the bit-sliced objects"""
    if not os.path.exists("/opt/rocm/bin/hipcc") or not os.path.exists(f"{LLVM}/llvm-objdump"):
        pytest.fail("hipcc / llvm-objdump missing: the kernel-shape guards cannot run in this environment")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "labrador_ldpc_amd", "csrc"), "-j", str(min(8, os.cpu_count() or 1))],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for o in OBJECTS:
        assert os.path.exists(os.path.join(ROOT, "build", "csrc", o)), f"{o} is not built"
    import kernel_resources
    return [(obj, dem, int(v), int(sp), int(lds)) for obj, dem, v, sp, s, lds, scr in kernel_resources.resources("build/csrc/decode_ms_bs*.o")]


def test_sixteen_kernels_each_once_in_its_unit_within_registers_lds_and_spills(rows):
    seen, plain, corrected = {}, {}, {}
    for obj, dem, v, sp, lds in rows:
        m = re.search(r"decode_ms_bsh_kernel<(\d)>", dem) or re.search(r"decode_ms_bshc_kernel<(\d), (\d)>", dem)
        if m:
            key = (int(m.group(1)), int(m.group(2)) if m.lastindex == 2 else None)
            assert obj in OBJECTS, (obj, dem)
            assert key not in seen, f"{dem} is built twice"
            seen[key] = (obj, v, sp, lds)
        m = re.search(r"decode_ms_bs_kernel<(\d)>", dem)
        if m:
            plain[int(m.group(1))] = (v, sp, lds)
        m = re.search(r"decode_ms_bsc_kernel<(\d), (\d)>", dem)
        if m:
            corrected[(int(m.group(1)), int(m.group(2)))] = (v, sp, lds)
    assert sorted(seen, key=str) == sorted([(c, m) for c in CODES for m in (None,) + MULBITS], key=str), sorted(seen, key=str)
    for (code, mulbits), (obj, v, sp, lds) in sorted(seen.items(), key=str):
        iv, isp, ilds = plain[code] if mulbits is None else corrected[(code, mulbits)]
        w = waves(code, mulbits)
        print(f"{CODES[code]} {'plain' if mulbits is None else 'mulbits %d' % mulbits}: vgpr {v} spill {sp} lds {lds} at {w} waves/SIMD ({obj})"
              f"   i8 source: vgpr {iv} spill {isp} lds {ilds}")
        assert obj == f"decode_ms_bs_hard_{UNIT[code]}.o"
        assert v <= VGPRS_PER_SIMD // w // 8 * 8, f"{CODES[code]}/{mulbits}: {v} VGPRs do not allow {w} waves per SIMD"
        assert lds == plain[code][2], f"{CODES[code]}/{mulbits}: {lds} bytes of LDS, the plain kernel has {plain[code][2]}"
        assert sp <= isp, f"{CODES[code]}/{mulbits}: {sp} spilled registers, the i8-source kernel of the form has {isp}"


def test_the_new_names_are_nobody_elses(rows):
    seen = 0
    for obj, dem, v, sp, lds in rows:
        if obj in OBJECTS:
            seen += 1
            assert ("decode_ms_bsh_kernel<" in dem or "decode_ms_bshc_kernel<" in dem) and not any(f in dem for f in FORBIDDEN), dem
        else:
            assert "decode_ms_bsh_" not in dem and "decode_ms_bshc_" not in dem, (obj, dem)      # (the other objects keep the kernels they had)
    assert seen == 16
