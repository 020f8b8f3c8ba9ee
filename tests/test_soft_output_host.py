"""CPU-side checks of the soft-output entry points (labrador_ldpc_decode_ms_soft_batch_*): the header declares them, the library
exports them, their argument checks answer before any device work, and the soft-output kernels -- compiled into objects of their
own -- pass the same compile-time guards as the hard-only ones (uniform control flow, no scratch traffic in the iteration loops).
No compute calls need a GPU."""
import ctypes
import glob
import os
import re
import sys

import numpy as np
import pytest

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
TYPES = {"f32": ("float", np.float32), "i8": ("int8_t", np.int8), "i16": ("int16_t", np.int16), "i32": ("int32_t", np.int32),
         "f64": ("double", np.float64)}
EINVAL, OK = -1, 0


def test_header_declares_the_five_soft_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "labrador_ldpc_hip.h")).read(), flags=re.S)
    for suf, (ctype, _) in TYPES.items():
        pat = (rf"int\s+labrador_ldpc_decode_ms_soft_batch_{suf}\s*\(\s*enum labrador_ldpc_code code,\s*const {ctype} \*llrs,\s*"
               rf"{ctype} \*app,\s*uint8_t \*output,\s*uint32_t \*iters,\s*uint8_t \*success,\s*size_t batch,\s*size_t max_iters,\s*"
               rf"const struct labrador_ldpc_hip_opts \*opts\s*\)\s*;")
        assert re.search(pat, src), f"labrador_ldpc_decode_ms_soft_batch_{suf} missing or with another signature"


def test_library_exports_the_soft_entry_points():
    dll = ctypes.CDLL(la.LIB_PATH)
    for suf in TYPES:
        assert hasattr(dll, f"labrador_ldpc_decode_ms_soft_batch_{suf}")
        assert f"labrador_ldpc_decode_ms_soft_batch_{suf}" in la.SYMBOLS


@pytest.mark.parametrize("suf", list(TYPES))
def test_argument_checks_come_before_any_device_work(suf):
    """As labrador_ldpc_decode_ms_batch_*: a bad code and a NULL buffer (app included) are EINVAL, batch == 0 is OK -- whether or
    not a GPU is present, since nothing is launched."""
    fn = getattr(la.lib, f"labrador_ldpc_decode_ms_soft_batch_{suf}")
    dt = TYPES[suf][1]
    code = LDPCCode.TC128
    llrs = np.ones((1, code.n()), dt)
    app = np.zeros((1, code.n() + code.punctured_bits()), dt)
    out = np.zeros((1, code.output_len()), np.uint8)
    it = np.zeros(1, np.uint32)
    ok = np.zeros(1, np.uint8)
    p = [a.ctypes.data for a in (llrs, app, out, it, ok)]
    assert fn(9, *p, 1, 10, None) == EINVAL
    assert fn(-1, *p, 1, 10, None) == EINVAL
    assert "out of range" in la.last_error()
    assert fn(int(code), p[0], None, p[2], p[3], p[4], 1, 10, None) == EINVAL
    assert "NULL" in la.last_error()
    for i in (0, 2, 3, 4):
        q = list(p)
        q[i] = None
        assert fn(int(code), *q, 1, 10, None) == EINVAL
    assert fn(int(code), *p, 0, 10, None) == OK
    assert fn(int(code), None, None, None, None, None, 0, 10, None) == OK      # (nothing to decode: no buffer is looked at)
    assert (app == 0).all() and (out == 0).all()


def test_python_binding_checks_the_app_buffer():
    code = LDPCCode.TM1280
    llrs = np.ones((2, code.n()), np.float32)
    with pytest.raises(ValueError):
        code.decode_ms_soft_batch(llrs, app=np.zeros((2, code.n()), np.float32))                      # n, not n + p
    with pytest.raises(ValueError):
        code.decode_ms_soft_batch(llrs, app=np.zeros((2, code.n() + code.punctured_bits()), np.float64))   # dtype of llrs
    with pytest.raises(ValueError):
        code.decode_ms_soft_batch(llrs[:, :-1])


@pytest.fixture(scope="module")
def soft_objects():
    """The soft-output objects (build/csrc/decode_ms_soft_*.o), built here if need be (`make` is a no-op when current)."""
    import subprocess
    if not os.path.exists("/opt/rocm/bin/hipcc") or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.fail("hipcc / llvm-objdump missing: the kernel-shape guards cannot run in this environment")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "labrador_ldpc_amd", "csrc"), "-j", str(min(8, os.cpu_count() or 1))],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    objs = sorted(glob.glob(os.path.join(ROOT, "build", "csrc", "decode_ms_soft_*.o")))
    assert len(objs) == 10, objs          # f32 (dispatch + 3 parts), i8, i16, i32, f64 (3 parts)
    return objs


def test_soft_kernels_live_in_their_own_objects(soft_objects):
    import scan_kernels
    soft = scan_kernels.scan("build/csrc/decode_ms_soft_*.o")
    names = {k for _, k in soft}
    assert sum("soft_decode_ms_kernel" in k for k in names) >= 30
    assert sum("soft_decode_ms_pair_kernel" in k for k in names) >= 5
    assert any("soft_decode_ms_f64_kernel" in k for k in names)
    hard = scan_kernels.scan("build/csrc/decode_ms_[fi]*.o") | scan_kernels.scan("build/csrc/decode_ms_bs_*.o")
    assert hard and not any("soft_" in k for _, k in hard), "a soft-output kernel in a hard-only object"


def test_soft_kernels_have_uniform_control_flow(soft_objects):
    """tests/test_kernel_shape.py's bound, per soft kernel: 16 EXEC-guarded regions, 40 for the f64 register kernels."""
    import scan_kernels
    table = scan_kernels.scan("build/csrc/decode_ms_soft_*.o")
    assert len(table) >= 40

    def bound(name):
        return 40 if "decode_ms_kernelILi" in name and "EdLi" in name else 16
    bad = {k: v for k, v in table.items() if v[1] > bound(k[1]) and "decode_ms_f64_kernel" not in k[1]}
    assert not bad, f"soft kernels with EXEC-masked loops: {bad}"


def test_no_spill_traffic_inside_the_soft_iteration_loops(soft_objects):
    """As tests/test_kernel_shape.py for the hard-only kernels: no scratch instruction in an f32 / i8 / i16 / i32 soft kernel's
    iteration loop (the soft epilogue must not push values out of registers across the loop).  A span that holds another one is the
    path AROUND the loop taken once per codeword; TC512 f32 at four waves per SIMD reloads one spilled value there in its hard-only
    form and two in its soft form (the thread index and its LDS offset, once per codeword), hence 2 for those spans.
    One known exception, like the f64 kernels of the large codes in the hard-only guard: TM8192 i32 with two indices per thread
    (`variant` 2, not the default -- that is the pair kernel, checked here): 127 registers and no spill hard-only, the soft form
    needs one more than the 128 of four waves per SIMD."""
    import loop_mix
    seen = 0
    objs = [o for o in soft_objects if "soft_f64" not in os.path.basename(o)]
    for obj in objs:
        for kernel, spans in loop_mix.spans_of(obj, "decode_ms").items():
            if "soft_decode_ms_kernelILi8EiLi2E" in kernel:
                continue
            seen += len(spans)
            for first, last, sp in spans:
                n = sum(1 for t in sp if t.startswith("scratch_"))
                outer = any((f2, l2) != (first, last) and first <= f2 and l2 <= last for f2, l2, _ in spans)
                assert n <= (2 if outer else 0), f"{os.path.basename(obj)} {kernel}: {n} scratch instructions inside an iteration loop"
    assert seen >= 100
