"""What the f32 loader costs the bit-sliced SOFT kernels, read from the two new objects with tools/kernel_resources.py
and the disassembly, without a GPU: each of the sixteen kernels -- four one-wave codes, the plain form and three multiplier widths of
the corrected one -- exists exactly once, in the object of its code's unit; its LDS equals the soft kernel's of the same code; its
VGPRs plus AGPRs are within what its launch bounds promise, at most 256 in every case; it spills nothing; and it carries no scratch
instruction between the first and the last lane permutation (ds_bpermute_b32), the rule of tests/test_kernel_shape.py.  Its name
cannot be taken for another kernel's by the tests that find those by name."""
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
FORMS = [(c, m) for c in sorted(CODES) for m in (None,) + MULBITS]
UNIT = {4: 2, 5: 1, 7: 2, 8: 1}                              # BsPlan::UNIT
WAVES = {4: 1, 5: 2, 7: 1, 8: 2}                             # BsPlan::SOFT_WAVES_PER_SIMD, every form
REGISTERS_PER_SIMD = 512
LDS_PER_CU = 163840
FORBIDDEN = ("decode_ms_bs_kernel", "decode_ms_bs_split_kernel", "refill_kernel", "decode_ms_bsc_", "decode_ms_bsa_", "decode_ms_bsca_",
             "decode_ms_bsq_", "decode_ms_bsqc_")
OBJECTS = ("decode_ms_bs_quantised_soft_1.o", "decode_ms_bs_quantised_soft_2.o")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists("/opt/rocm/bin/hipcc") or not os.path.exists(f"{LLVM}/llvm-objdump"):
        pytest.fail("hipcc / llvm-objdump missing: the kernel-shape guards cannot run in this environment")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "labrador_ldpc_amd", "csrc"), "-j", str(min(8, os.cpu_count() or 1))],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for o in OBJECTS:
        assert os.path.exists(os.path.join(ROOT, "build", "csrc", o)), f"{o} is not built"


@pytest.fixture(scope="module")
def rows(built):
    """[(object, demangled name, vgprs, spilled, lds, scratch bytes, agprs)] of every kernel of the bit-sliced objects"""
    import kernel_resources
    return [(obj, dem, int(v), int(sp), int(lds), int(scr), int(a))
            for obj, dem, v, sp, s, lds, scr, a in kernel_resources.resources("build/csrc/decode_ms_bs*.o", agprs=True)]


def key_of(m):
    return int(m.group(1)), None if m.group(2) is None else int(m.group(2))


def test_sixteen_kernels_each_once_in_its_unit_within_registers_and_lds(rows):
    seen, soft = {}, {}
    for obj, dem, v, sp, lds, scr, a in rows:
        m = re.search(r"decode_ms_bsqc?a_kernel<(\d)(?:, (\d))?>", dem)
        if m:
            assert obj in OBJECTS, (obj, dem)
            assert key_of(m) not in seen, f"{dem} is built twice"
            assert ("bsqca" in dem) == (m.group(2) is not None), dem
            seen[key_of(m)] = (obj, v, sp, lds, scr, a)
        m = re.search(r"decode_ms_bsa_kernel<(\d)>", dem)
        if m:
            soft[int(m.group(1))] = (v, sp, lds)
    assert sorted(seen, key=str) == sorted(FORMS, key=str), sorted(seen, key=str)
    for code, mulbits in FORMS:
        obj, v, sp, lds, scr, a = seen[(code, mulbits)]
        sv, ssp, slds = soft[code]
        w = WAVES[code]
        print(f"{CODES[code]} {'plain' if mulbits is None else 'mulbits %d' % mulbits}: vgpr {v} agpr {a} spill {sp} lds {lds} scratch {scr} at "
              f"{w} waves/SIMD ({obj})   soft kernel of the code: vgpr {sv} spill {ssp} lds {slds}")
        assert obj == f"decode_ms_bs_quantised_soft_{UNIT[code]}.o"
        assert lds == slds, f"{CODES[code]}/{mulbits}: {lds} bytes of LDS, the soft kernel has {slds}"
        assert lds * 4 * w <= LDS_PER_CU, f"{CODES[code]}/{mulbits}: {lds} bytes of LDS x {4 * w} waves per CU"
        assert v + a <= min(256, REGISTERS_PER_SIMD // w // 8 * 8), f"{CODES[code]}/{mulbits}: {v} VGPRs + {a} AGPRs at {w} waves per SIMD"
        assert sp == 0 and scr == 0, f"{CODES[code]}/{mulbits}: {sp} spilled registers, {scr} bytes of scratch"


def test_no_scratch_instruction_between_the_first_and_the_last_lane_permutation(built):
    tmp = tempfile.mkdtemp()
    seen = []
    for o in OBJECTS:
        stem = o[:-2]
        subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={tmp}/{stem}.fat", os.path.join(ROOT, "build", "csrc", o),
                               "/dev/null"])
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
        for name, body in table.items():
            m = re.search(r"decode_ms_bsqc?a_kernelILi(\d)E(?:Li(\d)E)?", name)
            if not m:
                continue
            at = [i for i, t in enumerate(body) if t.startswith("ds_bpermute_b32")]
            assert len(at) >= 100, name
            loop = body[at[0]:at[-1]]
            n = sum(1 for t in loop if t.startswith("scratch_"))
            print(f"{name}: {n} scratch instructions among the {len(loop)} between the first and the last ds_bpermute_b32")
            assert n == 0, f"{name}: {n} scratch instructions inside the iteration"
            assert sum(1 for t in loop if t.startswith("v_bitop3_b32")) > 0.5 * len(loop) - 200, name     # ... which is Boolean arithmetic
            seen.append(key_of(m))
    assert sorted(seen, key=str) == sorted(FORMS, key=str)


def test_the_new_names_are_nobody_elses(rows):
    seen = 0
    for obj, dem, *_ in rows:
        if obj in OBJECTS:
            seen += 1
            assert ("decode_ms_bsqa_kernel<" in dem or "decode_ms_bsqca_kernel<" in dem) and not any(f in dem for f in FORBIDDEN), dem
        else:
            assert "decode_ms_bsqa_" not in dem and "decode_ms_bsqca_" not in dem, (obj, dem)  # (the other objects keep the kernels they had)
    assert seen == 16
    # (tests/test_kernel_shape_bs_soft.py and _bs_corrected_soft.py count the kernels of the objects whose names begin like this)
    assert not any(o.startswith(("decode_ms_bs_soft_", "decode_ms_bs_corrected_soft_", "decode_ms_bs_quantised_1", "decode_ms_bs_quantised_2"))
                   for o in OBJECTS)
