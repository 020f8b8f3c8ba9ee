"""What the tests of the three layered decoders share (tests/test_gpu_layered*.py, tests/test_layered*_host.py): the restatement's
structure per code, the comparison of marginals, the launch geometry, the quantiser, and the built object and disassembled kernels of
the kernel-shape guards."""
import os
import subprocess
import sys

import numpy as np

import edge_frames
from labrador_ldpc_amd import LDPCCode
import layered_restatement as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import disasm  # noqa: E402

_ST = {}


def structure(code, make=lr.Structure):
    """The restatement's structure of `code`, built once (`make`: layered_restatement.Structure or a subclass of it)."""
    if (make, code) not in _ST:
        _ST[make, code] = make(int(code))
    return _ST[make, code]


def same_app(a, b):
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a[~na] == b[~nb]).all())


def layered_grid_bound(code, cus):
    """(most frames one round of the layered launch's persistent grid can hold, codewords per group, queue-fed?): LayeredGeometry<CODE>
    (the flooding default's indices per thread: 2 for TM8192, 1 otherwise), the launch's queue for workgroups of 512 threads and more."""
    nt = code.submatrix_size() // (2 if code == LDPCCode.TM8192 else 1)
    g = 64 // nt if nt < 64 else 1
    wg = nt * g
    return edge_frames.grid_bound(wg, g, wg >= 512, cus), g, wg >= 512


def quantise(y, dtype, scale, lim):
    return np.clip(np.rint(np.float32(scale) * y), -lim, lim).astype(dtype)


def built_object(name):
    """build/csrc/<name> of an up-to-date build, for the kernel-shape guards."""
    import pytest
    if not os.path.exists("/opt/rocm/bin/hipcc") or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.fail("hipcc / llvm-objdump missing: the kernel-shape guards cannot run in this environment")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "labrador_ldpc_amd", "csrc"), "-j", str(min(8, os.cpu_count() or 1))],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    obj = os.path.join(ROOT, "build", "csrc", name)
    assert os.path.exists(obj)
    return obj


def kernels(obj, name):
    """tools/disasm.py's kernels of `obj` whose symbol contains `name`."""
    return {k: v for k, v in disasm.kernels(obj).items() if name in k}
