"""kernel_inventory.py -- which `variant` values name a built min-sum kernel, per code and LLR type, for the tests that walk every
kernel (tests/test_gpu_soft_edges.py, tests/test_gpu_parity.py, tests/test_gpu_containment.py).  TEST INFRASTRUCTURE ONLY: a new kernel
is added here once."""
from labrador_ldpc_amd import LDPCCode

# (code, f32) -> every variant with a soft form: the default, the table's alternatives, the pair kernel, the fixed stride, and the forced
# one / two NaN passes of the register-lean kernels (decode_ms_tables.hpp, decode_ms_launch.hpp)
F32_VARIANTS = {LDPCCode.TC128: (0, 256), LDPCCode.TC256: (0, 256), LDPCCode.TC512: (0, 256), LDPCCode.TM1280: (0, 256, 512, 1024),
                LDPCCode.TM1536: (0, 2, 256), LDPCCode.TM2048: (0, 2, 32, 256), LDPCCode.TM5120: (0, 256, 512, 1024),
                LDPCCode.TM6144: (0, 2, 256), LDPCCode.TM8192: (0, 2, 4, 256)}
# f64: the default, the workspace kernel (100) and the register-kernel instantiations with a soft form (not in place)
F64_VARIANTS = {LDPCCode.TC128: (0, 1, 17, 100), LDPCCode.TC256: (0, 1, 17, 100), LDPCCode.TC512: (0, 1, 17, 100),
                LDPCCode.TM1280: (0, 1, 17, 100), LDPCCode.TM1536: (0, 1, 17, 100), LDPCCode.TM2048: (0, 1, 17, 100),
                LDPCCode.TM5120: (0, 17, 18, 100), LDPCCode.TM6144: (0, 2, 17, 18, 100), LDPCCode.TM8192: (0, 100)}
F64_TUNED = (1, 1, 1, 17, 1, 17, 17, 17, 34)          # decode_ms_tables.hpp
# f64, hard-only call: the non-default register-kernel instantiations (IPT = variant & 15, register-lean check phase if variant & 16,
# in-place messages if variant & 32)
F64_HARD_VARIANTS = [(LDPCCode.TC128, 17), (LDPCCode.TC256, 17), (LDPCCode.TC512, 17), (LDPCCode.TM1280, 1), (LDPCCode.TM1280, 33),
                     (LDPCCode.TM1536, 17), (LDPCCode.TM2048, 1), (LDPCCode.TM2048, 33), (LDPCCode.TM5120, 18), (LDPCCode.TM5120, 33),
                     (LDPCCode.TM6144, 33), (LDPCCode.TM6144, 18), (LDPCCode.TM6144, 2), (LDPCCode.TM8192, 36)]
# ... those of them that keep their messages in place: no soft form
F64_IN_PLACE = {c: tuple(v for cc, v in F64_HARD_VARIANTS if cc == c and v & 32) for c in LDPCCode}
