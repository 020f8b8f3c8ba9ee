"""What the soft form costs the bit-sliced kernels in registers and LDS, read from the built objects with
tools/kernel_resources.py, without a GPU: each of the four soft kernels exists exactly once across decode_ms_bs_soft_{1,2}.o, fits the
registers of the waves per SIMD it is built for and, with that many waves on each of a CU's four SIMDs, the CU's 160 KB of LDS; and
its name cannot be taken for a plain or a corrected kernel's by the tests that find those by name."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CODES = {4: "TM1536", 5: "TM2048", 7: "TM6144", 8: "TM8192"}
# waves per SIMD the soft kernel of a code is built for (BsPlan::SOFT_WAVES_PER_SIMD) and the plain kernel's (BsPlan::WAVES_PER_SIMD)
SOFT_WAVES = {4: 1, 5: 2, 7: 1, 8: 2}
PLAIN_WAVES = {4: 2, 5: 3, 7: 2, 8: 3}
VGPR_LIMIT = {3: 168, 2: 256, 1: 512}
LDS_PER_CU = 163840
FORBIDDEN = ("decode_ms_bs_kernel", "decode_ms_bs_split_kernel", "refill_kernel", "decode_ms_bsc_")


@pytest.fixture(scope="module")
def rows():
    """[(object, demangled name, vgprs, spilled, lds)] of every kernel of the bit-sliced objects (`make` first: a no-op when current)"""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.fail("hipcc missing: the kernel-shape guards cannot run in this environment")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "labrador_ldpc_amd", "csrc"), "-j", str(min(8, os.cpu_count() or 1))],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    import kernel_resources
    return [(obj, dem, int(v), int(sp), int(lds)) for obj, dem, v, sp, s, lds, scr in kernel_resources.resources("build/csrc/decode_ms_bs*.o")]


def test_each_soft_kernel_exists_once_and_fits_what_it_is_built_for(rows):
    soft, plain = {}, {}
    for obj, dem, v, sp, lds in rows:
        m = re.search(r"decode_ms_bsa_kernel<(\d)>", dem)
        if m:
            assert obj in ("decode_ms_bs_soft_1.o", "decode_ms_bs_soft_2.o"), (obj, dem)
            assert int(m.group(1)) not in soft, f"{dem} is built twice"
            soft[int(m.group(1))] = (obj, v, sp, lds)
        m = re.search(r"decode_ms_bs_kernel<(\d)>", dem)
        if m and obj in ("decode_ms_bs_1.o", "decode_ms_bs_2.o"):
            plain[int(m.group(1))] = (v, sp, lds)
    assert sorted(soft) == sorted(CODES), sorted(soft)
    for code, name in CODES.items():
        obj, v, sp, lds = soft[code]
        pv, psp, plds = plain[code]
        waves = SOFT_WAVES[code]
        print(f"{name}: soft vgpr {v} spill {sp} lds {lds} at {waves} waves/SIMD ({obj})   plain vgpr {pv} spill {psp} lds {plds} at {PLAIN_WAVES[code]}")
        assert obj == ("decode_ms_bs_soft_1.o" if code in (5, 8) else "decode_ms_bs_soft_2.o")       # (BsPlan::UNIT)
        assert v <= VGPR_LIMIT[waves], f"{name}: {v} registers do not allow {waves} waves per SIMD"
        assert lds * 4 * waves <= LDS_PER_CU, f"{name}: {lds} bytes of LDS x {4 * waves} waves per CU"
        assert lds >= plds
        if waves == PLAIN_WAVES[code]:
            assert sp <= psp, f"{name}: {sp} spilled registers, the plain kernel has {psp}"


def test_soft_kernel_names_are_nobody_elses(rows):
    seen = 0
    for obj, dem, v, sp, lds in rows:
        if obj.startswith("decode_ms_bs_soft_"):
            seen += 1
            assert not any(f in dem for f in FORBIDDEN), dem
        else:
            assert "decode_ms_bsa_" not in dem, (obj, dem)             # (the plain and the corrected objects keep the kernels they had)
    assert seen == 4
