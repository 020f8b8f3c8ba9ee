"""labrador_ldpc_amd -- MI355X (gfx950) batched min-sum LDPC decoder behind labrador-ldpc's API.

Host-side mirror of the reference crate's `LDPCCode` surface for the decode_ms path
(reference: src/codes/mod.rs:365-441 accessors, src/decoder.rs:88-116 sizes, :347-475
decode_ms, :484-509 LLR helpers, src/encoder.rs:293-315 encode/copy_encode), implemented as a
thin ctypes binding over the C ABI of ``liblabrador_ldpc_hip.so`` (include/labrador_ldpc_hip.h).

The library is required: importing this package without the built ``.so`` raises, and the
decoders raise ``LdpcHipError`` when no gfx950 device is usable.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import enum
import operator
import os
from typing import Optional, Tuple

import numpy as np

__all__ = ["LDPCCode", "LdpcHipError", "lib", "device_count", "last_error", "HipOpts", "LIB_PATH"]

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblabrador_ldpc_hip.so")


class LdpcHipError(RuntimeError):
    """A call into liblabrador_ldpc_hip.so failed (status < 0)."""


class HipOpts(ctypes.Structure):
    """struct labrador_ldpc_hip_opts (include/labrador_ldpc_hip.h)."""

    _fields_ = [("struct_size", ctypes.c_size_t), ("device", ctypes.c_int), ("memory", ctypes.c_int),
                ("stream", ctypes.c_void_p), ("variant", ctypes.c_int),
                ("n_devices", ctypes.c_int), ("devices", ctypes.POINTER(ctypes.c_int))]

    def __init__(self, device=0, memory=0, stream=None, variant=0, n_devices=0, devices=None, struct_size=None):
        # struct_size (ABI 3) tells the library how much of the struct this caller knows; fields beyond it read as zero
        super().__init__(ctypes.sizeof(HipOpts) if struct_size is None else struct_size, device, memory, stream, variant,
                         n_devices, devices)


MEM_HOST, MEM_DEVICE = 0, 1
DEVICE_CURRENT, DEVICE_ALL = -1, -2

_c = ctypes
_sz, _vp, _int = _c.c_size_t, _c.c_void_p, _c.c_int
_optp = _c.POINTER(HipOpts)

# every symbol include/labrador_ldpc_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "labrador_ldpc_code_n": (_sz, [_int]),
    "labrador_ldpc_code_k": (_sz, [_int]),
    "labrador_ldpc_bf_working_len": (_sz, [_int]),
    "labrador_ldpc_ms_working_u8_len": (_sz, [_int]),
    "labrador_ldpc_ms_working_len": (_sz, [_int]),
    "labrador_ldpc_output_len": (_sz, [_int]),
    "labrador_ldpc_encode": (None, [_int, _vp]),
    "labrador_ldpc_copy_encode": (None, [_int, _vp, _vp]),
    "labrador_ldpc_decode_bf": (_c.c_bool, [_int, _vp, _vp, _vp, _sz, _c.POINTER(_sz)]),
    "labrador_ldpc_decode_ms_i8": (_c.c_bool, [_int, _vp, _vp, _vp, _vp, _sz, _c.POINTER(_sz)]),
    "labrador_ldpc_decode_ms_i16": (_c.c_bool, [_int, _vp, _vp, _vp, _vp, _sz, _c.POINTER(_sz)]),
    "labrador_ldpc_decode_ms_i32": (_c.c_bool, [_int, _vp, _vp, _vp, _vp, _sz, _c.POINTER(_sz)]),
    "labrador_ldpc_decode_ms_f32": (_c.c_bool, [_int, _vp, _vp, _vp, _vp, _sz, _c.POINTER(_sz)]),
    "labrador_ldpc_decode_ms_f64": (_c.c_bool, [_int, _vp, _vp, _vp, _vp, _sz, _c.POINTER(_sz)]),
    "labrador_ldpc_hard_to_llrs_i8": (None, [_int, _vp, _vp]),
    "labrador_ldpc_hard_to_llrs_i16": (None, [_int, _vp, _vp]),
    "labrador_ldpc_hard_to_llrs_i32": (None, [_int, _vp, _vp]),
    "labrador_ldpc_hard_to_llrs_f32": (None, [_int, _vp, _vp]),
    "labrador_ldpc_hard_to_llrs_f64": (None, [_int, _vp, _vp]),
    "labrador_ldpc_llrs_to_hard_i8": (None, [_int, _vp, _vp]),
    "labrador_ldpc_llrs_to_hard_i16": (None, [_int, _vp, _vp]),
    "labrador_ldpc_llrs_to_hard_i32": (None, [_int, _vp, _vp]),
    "labrador_ldpc_llrs_to_hard_f32": (None, [_int, _vp, _vp]),
    "labrador_ldpc_llrs_to_hard_f64": (None, [_int, _vp, _vp]),
    "labrador_ldpc_decode_ms_batch_f32": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _optp]),
    "labrador_ldpc_decode_ms_batch_i8": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _optp]),
    "labrador_ldpc_decode_ms_batch_i16": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _optp]),
    "labrador_ldpc_decode_ms_batch_i32": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _optp]),
    "labrador_ldpc_decode_ms_batch_f64": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _optp]),
    **{f"labrador_ldpc_decode_ms_soft_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _optp]) for t in ("f32", "i8", "i16", "i32", "f64")},
    "labrador_ldpc_decode_ms_layered_batch_f32": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _optp]),
    "labrador_ldpc_decode_ms_layered_soft_batch_f32": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _optp]),
    "labrador_ldpc_decode_ms_layered_corrected_batch_f32": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _c.c_float, _c.c_float, _optp]),
    "labrador_ldpc_decode_ms_layered_corrected_soft_batch_f32": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _c.c_float, _c.c_float,
                                                                        _optp]),
    **{f"labrador_ldpc_decode_ms_layered_fixed_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _optp]) for t in ("i8", "i16")},
    **{f"labrador_ldpc_decode_ms_layered_fixed_soft_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _optp]) for t in ("i8", "i16")},
    **{f"labrador_ldpc_decode_ms_layered_fixed_corrected_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _c.c_uint32, _c.c_uint32,
                                                                            _c.c_uint32, _optp]) for t in ("i8", "i16")},
    **{f"labrador_ldpc_decode_ms_layered_fixed_corrected_soft_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _c.c_uint32,
                                                                                 _c.c_uint32, _c.c_uint32, _optp]) for t in ("i8", "i16")},
    "labrador_ldpc_decode_ms_cascade_batch_f32": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _c.c_float, _c.c_float, _optp]),
    # the flooding schedule with normalized / offset check messages, and the cascade with it as stage 1
    "labrador_ldpc_decode_ms_corrected_batch_f32": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _c.c_float, _c.c_float, _optp]),
    "labrador_ldpc_decode_ms_corrected_soft_batch_f32": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _c.c_float, _c.c_float, _optp]),
    "labrador_ldpc_decode_ms_cascade_corrected_batch_f32": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _c.c_float, _c.c_float,
                                                                   _c.c_float, _c.c_float, _optp]),
    **{f"labrador_ldpc_decode_ms_cascade_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _c.c_uint32, _c.c_uint32,
                                                             _c.c_uint32, _optp]) for t in ("i8", "i16")},
    # the cascade with soft output: `app` behind llrs; the f32 entry carries both pairs
    "labrador_ldpc_decode_ms_cascade_soft_batch_f32": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _c.c_float, _c.c_float,
                                                              _c.c_float, _c.c_float, _optp]),
    **{f"labrador_ldpc_decode_ms_cascade_soft_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _c.c_uint32,
                                                                  _c.c_uint32, _c.c_uint32, _optp]) for t in ("i8", "i16")},
    # the bit-sliced i8 flooding kernels with normalized / offset check messages, and the integer cascades with them as stage 1
    # 
    "labrador_ldpc_decode_ms_corrected_batch_i8": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _c.c_uint32, _c.c_uint32, _c.c_uint32, _optp]),
    "labrador_ldpc_decode_ms_cascade_corrected_batch_i8": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _c.c_uint32, _c.c_uint32,
                                                                  _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32, _optp]),
    "labrador_ldpc_decode_ms_cascade_quantised_corrected_batch_i8": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _c.c_float, _int,
                                                                            _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                                                            _c.c_uint32, _optp]),
    # soft output from the bit-sliced i8 kernels, and the soft i8 cascade with them as stage 1
    "labrador_ldpc_decode_ms_bitsliced_soft_batch_i8": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _optp]),
    "labrador_ldpc_decode_ms_cascade_bitsliced_soft_batch_i8": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _c.c_uint32,
                                                                       _c.c_uint32, _c.c_uint32, _optp]),
    # ... with normalized / offset check messages: the corrected soft kernels, and the soft i8 cascade with a stage-1 triple
    "labrador_ldpc_decode_ms_bitsliced_corrected_soft_batch_i8": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _c.c_uint32, _c.c_uint32,
                                                                         _c.c_uint32, _optp]),
    "labrador_ldpc_decode_ms_cascade_bitsliced_corrected_soft_batch_i8": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz,
                                                                                 _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                                                                 _c.c_uint32, _c.c_uint32, _optp]),
    **{f"labrador_ldpc_decode_ms_batch_{t}_multi": (_int, [_int, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _int]) for t in ("i8", "i16", "i32", "f32", "f64")},
    "labrador_ldpc_decode_bf_batch": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _optp]),
    "labrador_ldpc_encode_batch": (_int, [_int, _vp, _vp, _sz, _optp]),
    **{f"labrador_ldpc_hard_to_llrs_batch_{t}": (_int, [_int, _vp, _vp, _sz, _optp]) for t in ("i8", "i16", "i32", "f32", "f64")},
    **{f"labrador_ldpc_llrs_to_hard_batch_{t}": (_int, [_int, _vp, _vp, _sz, _optp]) for t in ("i8", "i16", "i32", "f32", "f64")},
    **{f"labrador_ldpc_quantise_llrs_batch_{t}": (_int, [_int, _vp, _vp, _sz, _c.c_float, _int, _optp]) for t in ("i8", "i16")},
    **{f"labrador_ldpc_decode_ms_quantised_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _c.c_float, _int, _optp]) for t in ("i8", "i16")},
    **{f"labrador_ldpc_decode_ms_layered_quantised_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _c.c_float, _int, _c.c_uint32,
                                                                       _c.c_uint32, _c.c_uint32, _optp]) for t in ("i8", "i16")},
    **{f"labrador_ldpc_decode_ms_layered_quantised_soft_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _c.c_float, _int,
                                                                            _c.c_uint32, _c.c_uint32, _c.c_uint32, _optp]) for t in ("i8", "i16")},
    **{f"labrador_ldpc_decode_ms_cascade_quantised_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _c.c_float, _int,
                                                                       _c.c_uint32, _c.c_uint32, _c.c_uint32, _optp]) for t in ("i8", "i16")},
    # f32 LLRs through the bit-sliced i8 kernels' own loader, and the i8 cascade on it
    "labrador_ldpc_decode_ms_bitsliced_quantised_batch_i8": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _c.c_float, _int, _optp]),
    "labrador_ldpc_decode_ms_bitsliced_quantised_corrected_batch_i8": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _c.c_float, _int,
                                                                              _c.c_uint32, _c.c_uint32, _c.c_uint32, _optp]),
    "labrador_ldpc_decode_ms_cascade_bitsliced_quantised_batch_i8": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _c.c_float, _int,
                                                                            _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                                                            _c.c_uint32, _optp]),
    # ... with soft output: `app` behind `llrs`
    "labrador_ldpc_decode_ms_bitsliced_quantised_soft_batch_i8": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _c.c_float, _int, _optp]),
    "labrador_ldpc_decode_ms_bitsliced_quantised_corrected_soft_batch_i8": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _c.c_float, _int,
                                                                                   _c.c_uint32, _c.c_uint32, _c.c_uint32, _optp]),
    "labrador_ldpc_decode_ms_cascade_bitsliced_quantised_soft_batch_i8": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz,
                                                                                 _c.c_float, _int, _c.c_uint32, _c.c_uint32, _c.c_uint32,
                                                                                 _c.c_uint32, _c.c_uint32, _c.c_uint32, _optp]),
    # packed hard decisions through the bit-sliced i8 kernels' own loader: `erasures` behind `input`, `magnitude` behind max_iters
    # 
    "labrador_ldpc_decode_ms_bitsliced_hard_batch_i8": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _int, _optp]),
    "labrador_ldpc_decode_ms_bitsliced_hard_corrected_batch_i8": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _int, _c.c_uint32,
                                                                         _c.c_uint32, _c.c_uint32, _optp]),
    # f16 / bf16 LLRs, as raw bits, to the f32 decoders
    **{f"labrador_ldpc_widen_llrs_batch_{t}": (_int, [_int, _vp, _vp, _sz, _optp]) for t in ("f16", "bf16")},
    **{f"labrador_ldpc_decode_ms_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _optp]) for t in ("f16", "bf16")},
    **{f"labrador_ldpc_decode_ms_soft_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _optp]) for t in ("f16", "bf16")},
    **{f"labrador_ldpc_decode_ms_layered_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _optp]) for t in ("f16", "bf16")},
    **{f"labrador_ldpc_decode_ms_layered_soft_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _optp]) for t in ("f16", "bf16")},
    **{f"labrador_ldpc_decode_ms_layered_corrected_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _sz, _sz, _c.c_float, _c.c_float, _optp])
       for t in ("f16", "bf16")},
    **{f"labrador_ldpc_decode_ms_layered_corrected_soft_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _c.c_float, _c.c_float,
                                                                            _optp]) for t in ("f16", "bf16")},
    **{f"labrador_ldpc_decode_ms_cascade_batch_{t}": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _c.c_float, _c.c_float, _optp])
       for t in ("f16", "bf16")},
    "labrador_ldpc_hip_awgn_f32": (_int, [_int, _vp, _sz, _vp, _sz, _c.c_float, _c.c_uint64, _optp]),
    "labrador_ldpc_hip_awgn_i8": (_int, [_int, _vp, _sz, _vp, _sz, _c.c_float, _c.c_float, _int,
                                         _c.c_uint64, _optp]),
    "labrador_ldpc_hip_awgn_f32_at": (_int, [_int, _vp, _sz, _vp, _c.c_uint64, _sz, _c.c_float, _c.c_uint64, _optp]),
    "labrador_ldpc_hip_awgn_i8_at": (_int, [_int, _vp, _sz, _vp, _c.c_uint64, _sz, _c.c_float, _c.c_float, _int,
                                            _c.c_uint64, _optp]),
    "labrador_ldpc_hip_edge_crc": (_c.c_uint32, [_int]),
    "labrador_ldpc_hip_edges": (_sz, [_int, _vp, _vp, _sz]),
    "labrador_ldpc_hip_shard_range": (_int, [_sz, _sz, _sz, _c.POINTER(_sz), _c.POINTER(_sz)]),
    "labrador_ldpc_hip_device_count": (_int, []),
    "labrador_ldpc_hip_last_error": (_c.c_char_p, []),
    "labrador_ldpc_hip_version": (_c.c_char_p, []),
    "labrador_ldpc_hip_build_id": (_c.c_char_p, []),
    "labrador_ldpc_hip_abi_version": (_int, []),
    "labrador_ldpc_hip_shader_clock_mhz": (_int, [_int, _c.c_double, _c.POINTER(_c.c_double)]),
    "labrador_ldpc_hip_decode_ms_i8_kernel": (_c.c_char_p, [_int, _int, _sz]),
}


def _preload_hip_runtime() -> str:
    """liblabrador_ldpc_hip.so is linked without the HIP runtime; supply ONE for the process.

    If torch is installed, its bundled libamdhip64.so is used (found without importing torch), so
    that this library and torch share one runtime -- device pointers, streams and events are then
    interchangeable, whichever is imported first.  Otherwise the system ROCm runtime is used."""
    import importlib.util
    cands = []
    try:
        spec = importlib.util.find_spec("torch")
        if spec and spec.submodule_search_locations:
            cands.append(os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so"))
    except Exception:
        pass
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cands += [os.path.join(rocm, "lib", "libamdhip64.so"), "libamdhip64.so"]
    errs = []
    for c in cands:
        if os.path.isabs(c) and not os.path.exists(c):
            continue
        try:
            ctypes.CDLL(c, mode=ctypes.RTLD_GLOBAL)
            return c
        except OSError as e:      # try the next candidate
            errs.append(f"{c}: {e}")
    raise ImportError("no HIP runtime (libamdhip64.so) could be loaded: " + "; ".join(errs))


def _load() -> ctypes.CDLL:
    global LIB_PATH
    LIB_PATH = os.environ.get("LABRADOR_LDPC_HIP_LIB", LIB_PATH)
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C labrador_ldpc_amd/csrc -j8`.  The HIP library is required (no CPU fallback).")
    global HIP_RUNTIME
    HIP_RUNTIME = _preload_hip_runtime()
    dll = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(dll, name)          # AttributeError if the .so does not export it
        fn.restype, fn.argtypes = res, args
    return dll


HIP_RUNTIME = ""
lib = _load()


def device_count() -> int:
    return int(lib.labrador_ldpc_hip_device_count())


def last_error() -> str:
    return lib.labrador_ldpc_hip_last_error().decode()


def _check(status: int) -> None:
    if status != 0:
        raise LdpcHipError(f"status {status}: {last_error()}")


_NP_SUFFIX = {np.dtype(np.float32): "f32", np.dtype(np.int8): "i8", np.dtype(np.int16): "i16",
              np.dtype(np.int32): "i32", np.dtype(np.float64): "f64"}
_NP_DTYPE = {v: k for k, v in _NP_SUFFIX.items()}
_TORCH_DTYPE: dict = {}
# The half-precision LLR types, a table of their own: only the methods that say so take them (the f32 decoders'
# batched calls and widen_llrs_batch); everything else keeps refusing them through _NP_SUFFIX.  numpy has no bfloat16, so host bf16
# buffers are not offered from Python (np.uint16 is not taken for one).
_NP_HALF_SUFFIX = {np.dtype(np.float16): "f16"}


def _torch_dtypes() -> dict:
    """suffix -> torch dtype, built on first use: torch stays an optional import"""
    if not _TORCH_DTYPE:
        import torch
        _TORCH_DTYPE.update(f32=torch.float32, i8=torch.int8, i16=torch.int16, i32=torch.int32, f64=torch.float64)
    return _TORCH_DTYPE


_DECODE_MS_FN: dict = {}
_SIZES: dict = {}


def _sizes(code) -> Tuple[int, int]:
    """(n, output_len) of a code, asked of the library once"""
    v = _SIZES.get(code)
    if v is None:
        v = _SIZES[code] = (code.n(), code.output_len())
    return v


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _ptr(a) -> int:
    return a.data_ptr() if _is_torch(a) else a.ctypes.data


def _suffix(a) -> str:
    if _is_torch(a):
        return {v: k for k, v in _torch_dtypes().items()}[a.dtype]
    return _NP_SUFFIX[a.dtype]


def _half_suffix(a):
    """"f16" / "bf16" for a half-precision array or tensor, None for anything else"""
    if _is_torch(a):
        import torch
        return {torch.float16: "f16", torch.bfloat16: "bf16"}.get(a.dtype)
    return _NP_HALF_SUFFIX.get(a.dtype)


def _host_opts(stream, variant: int, devices):
    """opts for host (numpy) buffers.  `devices`: None = the current device, "all" = every gfx950
    device, or a sequence of HIP ordinals (may repeat) to shard the batch over."""
    if devices is None:
        return HipOpts(DEVICE_CURRENT, MEM_HOST, stream, variant, 0, None), None
    if stream is not None:
        raise ValueError("a device set runs on the library's own streams: stream must be None")
    if isinstance(devices, str):
        if devices != "all":
            raise ValueError('devices must be None, "all" or a sequence of device ordinals')
        return HipOpts(DEVICE_ALL, MEM_HOST, None, variant, 0, None), None
    devs = [int(d) for d in devices]
    if not devs:
        raise ValueError("empty device list")
    arr = (ctypes.c_int * len(devs))(*devs)
    return HipOpts(DEVICE_CURRENT, MEM_HOST, None, variant, len(devs), arr), arr   # keep arr alive during the call


def _device_opts(tensor, stream, variant: int = 0):
    """opts for buffers resident on `tensor`'s device; `stream` None = torch's current stream of that device"""
    import torch
    dev = tensor.device
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    return HipOpts(dev.index if dev.index is not None else -1, MEM_DEVICE, stream, variant, 0, None)


def _result_buffer(buf, like, shape, kind: str, name: str, exact: bool = False):
    """The result buffer `name` of a call whose input is `like`: `buf` once it is checked, or, for None, a new one where `like`
    lives (a torch tensor's device, or the host as a numpy array).  kind: a dtype suffix.  exact=False is for the decoders' u8 and
    i32 outputs (_check_result_buffer; a new numpy `iters` is uint32); exact=True for a buffer in a dtype the caller chose."""
    torch_like = _is_torch(like)
    if torch_like:
        import torch
        dt = torch.uint8 if kind == "u8" else _torch_dtypes()[kind]
    else:
        dt = _NP_DTYPE[kind] if exact else np.dtype({"u8": np.uint8, "i32": np.uint32}[kind])
    if buf is None:
        return torch.empty(shape, dtype=dt, device=like.device) if torch_like else np.empty(shape, dtype=dt)
    if not exact:
        _check_result_buffer(buf, like, shape, kind, name)
    elif torch_like:
        if not (_is_torch(buf) and buf.device == like.device and buf.dtype == dt and tuple(buf.shape) == shape and buf.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {dt} tensor of shape {shape} on {like.device}")
    elif not (isinstance(buf, np.ndarray) and buf.dtype == dt and buf.shape == shape and buf.flags.c_contiguous and buf.flags.writeable):
        raise ValueError(f"{name} must be a writable C-contiguous {dt} array of shape {shape}")
    return buf


def _check_result_buffer(buf, like, shape, kinds, name: str):
    """A caller-supplied result buffer is handed to the C ABI as a raw pointer: refuse anything the
    kernel or the copy-out would overrun or misinterpret."""
    if _is_torch(like):
        import torch
        ok_dtypes = {"u8": (torch.uint8,), "i32": (torch.int32, getattr(torch, "uint32", torch.int32))}[kinds]
        if not _is_torch(buf) or buf.device != like.device:
            raise ValueError(f"{name} must be a torch tensor on {like.device}")
        if buf.dtype not in ok_dtypes or tuple(buf.shape) != shape or not buf.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {kinds} tensor of shape {shape}")
    else:
        ok_dtypes = {"u8": (np.uint8,), "i32": (np.uint32, np.int32)}[kinds]
        if not isinstance(buf, np.ndarray) or buf.dtype not in [np.dtype(d) for d in ok_dtypes]:
            raise ValueError(f"{name} must be a numpy array of dtype {kinds}")
        if buf.shape != shape or not buf.flags.c_contiguous or not buf.flags.writeable:
            raise ValueError(f"{name} must be a writable C-contiguous array of shape {shape}")


# (submatrix_size, circulant_size) per code: src/codes/mod.rs:109-241
_SUBMATRIX = {0: (16, 16), 1: (32, 32), 2: (64, 64), 3: (128, 32), 4: (256, 64), 5: (512, 128),
              6: (512, 128), 7: (1024, 256), 8: (2048, 512)}


class StageOneTripleError(ValueError, TypeError):
    """decode_ms_cascade_fixed_soft_batch was given a flooding_* keyword without bitsliced=True.  A ValueError -- the keywords exist,
    the combination does not -- that is a TypeError as well, which is what the call raised while the method had no such keywords:
    a caller that catches either keeps working."""


def _fixed_correction(scale_num, scale_shift, offset):
    """The (scale_num, scale_shift, offset) of a corrected fixed-point layered call, or None when none of them is given (the plain
    call).  The ranges are the library's to check; here only what ctypes would wrap into a uint32_t without a word is refused."""
    if scale_num is None and scale_shift is None and offset is None:
        return None
    shift = operator.index(0 if scale_shift is None else scale_shift)
    # (a scale_shift out of range is refused by the library before it looks at scale_num: the default only has to exist)
    triple = (operator.index(1 << min(max(shift, 0), 8) if scale_num is None else scale_num), shift,
              operator.index(0 if offset is None else offset))
    for name, v in zip(("scale_num", "scale_shift", "offset"), triple):
        if not 0 <= v < 1 << 32:
            raise ValueError(f"{name} does not fit a uint32_t")
    return triple


class LDPCCode(enum.IntEnum):
    """`enum LDPCCode` (src/codes/mod.rs:37-66) with the crate's method names."""

    TC128 = 0
    TC256 = 1
    TC512 = 2
    TM1280 = 3
    TM1536 = 4
    TM2048 = 5
    TM5120 = 6
    TM6144 = 7
    TM8192 = 8

    # ---- parameters: src/codes/mod.rs:381-409 ----
    def n(self) -> int:
        return int(lib.labrador_ldpc_code_n(int(self)))

    def k(self) -> int:
        return int(lib.labrador_ldpc_code_k(int(self)))

    def punctured_bits(self) -> int:
        return self.output_len() * 8 - self.n()

    def submatrix_size(self) -> int:
        return _SUBMATRIX[int(self)][0]

    def circulant_size(self) -> int:
        return _SUBMATRIX[int(self)][1]

    def paritycheck_sum(self) -> int:
        return (self.decode_ms_working_len() - 3 * self.n() - 3 * self.punctured_bits() + 2 * self.k()) // 2

    def iter_paritychecks(self):
        """(check, variable) index arrays of every parity-check edge in the crate's iteration order
        (src/codes/mod.rs:435-441), from the tables the kernels are generated from."""
        E = self.paritycheck_sum()
        chk, var = np.empty(E, dtype=np.uint16), np.empty(E, dtype=np.uint16)
        got = lib.labrador_ldpc_hip_edges(int(self), chk.ctypes.data, var.ctypes.data, E)
        assert got == E
        return chk, var

    # ---- sizes: src/decoder.rs:93-116 ----
    def decode_bf_working_len(self) -> int:
        return int(lib.labrador_ldpc_bf_working_len(int(self)))

    def decode_ms_working_len(self) -> int:
        return int(lib.labrador_ldpc_ms_working_len(int(self)))

    def decode_ms_working_u8_len(self) -> int:
        return int(lib.labrador_ldpc_ms_working_u8_len(int(self)))

    def output_len(self) -> int:
        return int(lib.labrador_ldpc_output_len(int(self)))

    # ---- encoder: src/encoder.rs:293-315 ----
    def encode(self, codeword: np.ndarray) -> np.ndarray:
        """Set the parity bytes of `codeword` (n/8 bytes, first k/8 = data) in place."""
        cw = _as_u8(codeword, self.n() // 8, "codeword must be n bits long")
        lib.labrador_ldpc_encode(int(self), cw.ctypes.data)
        return cw

    def copy_encode(self, data: np.ndarray, codeword: np.ndarray) -> np.ndarray:
        d = _as_u8(data, self.k() // 8, "data must be k bits long")
        cw = _as_u8(codeword, self.n() // 8, "codeword must be n bits long")
        lib.labrador_ldpc_copy_encode(int(self), d.ctypes.data, cw.ctypes.data)
        return cw

    # ---- LLR helpers: src/decoder.rs:484-509 ----
    def hard_to_llrs(self, input: np.ndarray, llrs: np.ndarray) -> None:
        inp = _as_u8(input, self.n() // 8, "input.len() != n/8")
        if llrs.shape != (self.n(),):
            raise ValueError("llrs.len() != n")
        getattr(lib, "labrador_ldpc_hard_to_llrs_" + _suffix(llrs))(int(self), inp.ctypes.data, llrs.ctypes.data)

    def llrs_to_hard(self, llrs: np.ndarray, output: np.ndarray) -> None:
        if llrs.shape != (self.n(),):
            raise ValueError("llrs.len() != n")
        out = _as_u8(output, self.n() // 8, "output.len() != n/8")
        getattr(lib, "labrador_ldpc_llrs_to_hard_" + _suffix(llrs))(int(self), llrs.ctypes.data, out.ctypes.data)

    # ---- min-sum decoder: src/decoder.rs:347-475 ----
    def decode_ms(self, llrs: np.ndarray, output: np.ndarray, working: Optional[np.ndarray] = None,
                  working_u8: Optional[np.ndarray] = None, maxiters: int = 50) -> Tuple[bool, int]:
        """One codeword on the GPU.  Returns (success, iterations) like the crate.

        Length checks mirror the asserts of src/decoder.rs:356-359; `working`/`working_u8`
        are optional here (the GPU keeps all message state on chip) but are length-checked
        when given."""
        if not isinstance(llrs, np.ndarray) or llrs.dtype not in _NP_SUFFIX:
            raise ValueError("llrs must be a numpy array of dtype int8, int16, int32, float32 or float64")
        # (a call is ~12 us in the library: the sizes come from a per-code cache and the addresses from __array_interface__, not
        # from three more trips through ctypes and two `.ctypes` objects -- 17 -> 14 us per call through this wrapper)
        n, out_len = _sizes(self)
        if llrs.shape != (n,):
            raise ValueError("llrs.len() != n")
        out = _as_u8(output, out_len, "output.len() != (n+p)/8")
        if working is not None and working.shape != (self.decode_ms_working_len(),):
            raise ValueError("working.len() incorrect")
        if working_u8 is not None and working_u8.shape != (self.decode_ms_working_u8_len(),):
            raise ValueError("working_u8 != (n+p-k)/8")
        if not llrs.flags.c_contiguous:
            llrs = np.ascontiguousarray(llrs)
        iters = ctypes.c_size_t(0)
        fn = _DECODE_MS_FN.get(llrs.dtype)
        if fn is None:
            fn = _DECODE_MS_FN[llrs.dtype] = getattr(lib, "labrador_ldpc_decode_ms_" + _NP_SUFFIX[llrs.dtype])
        ok = fn(int(self), llrs.__array_interface__["data"][0], out.__array_interface__["data"][0],
                working.ctypes.data if working is not None else None,
                working_u8.ctypes.data if working_u8 is not None else None,
                maxiters, ctypes.byref(iters))
        if not ok:
            err = last_error()
            if err:
                raise LdpcHipError(err)
        return bool(ok), int(iters.value)

    def decode_ms_batch(self, llrs, maxiters: int = 50, output=None, iters=None, success=None,
                        variant: int = 0, stream: Optional[int] = None, devices=None, scale: float = 1.0, offset: float = 0.0):
        """Decode `llrs[batch, n]`.

        numpy arrays are host buffers (the call stages them and returns when results are
        back; `devices="all"` or a list of HIP ordinals shards the batch over several GPUs);
        torch CUDA tensors are device-resident buffers: the call only enqueues the
        kernel on the tensor's device, on `stream` (default: torch's current stream).
        Returns (output[batch, output_len] u8, iters[batch] u32/i32, success[batch] u8).

        Half-precision LLRs -- a numpy float16 array, a torch float16 or bfloat16 tensor -- are decoded by the float32 kernels
        (labrador_ldpc_decode_ms_batch_f16 / _bf16): per frame exactly this call on the frame widened to float32.
        Host rows cross the link as halves; a device tensor must be 16-byte aligned.  The same holds for decode_ms_soft_batch,
        decode_ms_layered_batch, decode_ms_layered_soft_batch and decode_ms_cascade_batch; their `app` is float32.

        `scale`, `offset`: normalized / offset min-sum on this, the flooding schedule (labrador_ldpc_decode_ms_corrected_batch_f32,
        DESIGN.md 4.13) -- every check message magnitude m becomes max(scale * m - offset, 0).  0 < scale <= 1; offset >= 0 is in the
        units of the LLRs.  The library checks the ranges (LdpcHipError).  The defaults are plain min-sum and call the plain entry
        point; any other pair takes float32 LLRs only (another dtype, float16 and bfloat16 included, raises LdpcHipError) and
        `variant` 0 only."""
        if scale == 1.0 and offset == 0.0:
            return self._batch_call("labrador_ldpc_decode_ms_batch_", llrs, maxiters, output, iters, success, variant, stream, devices,
                                    half=True)
        return self._batch_call("labrador_ldpc_decode_ms_corrected_batch_", llrs, maxiters, output, iters, success, variant, stream,
                                devices, extra=(float(scale), float(offset)), types=("f32",))

    def decode_ms_layered_batch(self, llrs, maxiters: int = 50, output=None, iters=None, success=None,
                                variant: int = 0, stream: Optional[int] = None, devices=None, scale: float = 1.0, offset: float = 0.0):
        """decode_ms_batch with the block-row LAYERED schedule instead of the reference's flooding one (f32 LLRs only;
        labrador_ldpc_decode_ms_layered_batch_f32): each block row updates its checks from marginals that already
        hold the new messages of the rows before it, so a decode takes fewer sweeps and fails less often at the same cap.
        `iters` counts sweeps (0-based index of the succeeding one, maxiters on failure).  Buffers, `stream` and `devices` as
        decode_ms_batch; `variant` 0 is the only kernel.  Returns (output, iters, success).

        `scale`, `offset`: normalized / offset min-sum (labrador_ldpc_decode_ms_layered_corrected_batch_f32) -- every
        check message magnitude m becomes max(scale * m - offset, 0).  0 < scale <= 1; offset >= 0 is in the units of the LLRs, so
        a value that suits one LLR scaling does not suit another.  The library checks the ranges (LdpcHipError).  The defaults are
        plain min-sum and call the plain entry point."""
        if scale == 1.0 and offset == 0.0:
            return self._batch_call("labrador_ldpc_decode_ms_layered_batch_", llrs, maxiters, output, iters, success, variant, stream,
                                    devices, half=True)
        return self._batch_call("labrador_ldpc_decode_ms_layered_corrected_batch_", llrs, maxiters, output, iters, success, variant,
                                stream, devices, extra=(float(scale), float(offset)), half=True)

    def decode_ms_layered_fixed_batch(self, llrs, maxiters: int = 50, output=None, iters=None, success=None,
                                      variant: int = 0, stream: Optional[int] = None, devices=None,
                                      scale_num: Optional[int] = None, scale_shift: Optional[int] = None, offset: Optional[int] = None):
        """The block-row layered schedule in FIXED POINT, for int8 and int16 LLRs (labrador_ldpc_decode_ms_layered_fixed_batch_i8 /
        _i16).  A contract of its own: marginals are exact int32 sums, the only saturation is the clamp of a new
        variable message to +-T_MAX (127 / 32767), and an LLR equal to the type's minimum is read as -T_MAX.  `iters` counts sweeps
        as decode_ms_layered_batch does.  Buffers, `stream` and `devices` as decode_ms_batch; `variant` 0 is the only kernel.
        Returns (output, iters, success).

        `scale_num`, `scale_shift`, `offset`: normalized / offset min-sum in integers
        (labrador_ldpc_decode_ms_layered_fixed_corrected_batch_i8 / _i16) -- every check message magnitude m becomes
        max(((scale_num * m + ((1 << scale_shift) >> 1)) >> scale_shift) - offset, 0): the scale scale_num / 2^scale_shift in (0, 1]
        with 0 <= scale_shift <= 8, rounded half up, then an offset of 0 .. T_MAX in the units of the quantised LLRs.  The library
        checks the ranges (LdpcHipError).  With none of the three given the call is plain min-sum through the plain entry point; with
        any of them given, the others default to scale_num = 1 << scale_shift, scale_shift = 0 and offset = 0."""
        extra = _fixed_correction(scale_num, scale_shift, offset)
        if extra is None:
            return self._batch_call("labrador_ldpc_decode_ms_layered_fixed_batch_", llrs, maxiters, output, iters, success, variant,
                                    stream, devices)
        return self._batch_call("labrador_ldpc_decode_ms_layered_fixed_corrected_batch_", llrs, maxiters, output, iters, success, variant,
                                stream, devices, extra=extra)

    def decode_ms_layered_fixed_soft_batch(self, llrs, maxiters: int = 50, app=None, output=None, iters=None, success=None,
                                           variant: int = 0, stream: Optional[int] = None, devices=None,
                                           scale_num: Optional[int] = None, scale_shift: Optional[int] = None, offset: Optional[int] = None):
        """decode_ms_layered_fixed_batch with soft output (labrador_ldpc_decode_ms_layered_fixed_soft_batch_i8 / _i16): also the
        marginals of the returned sweep, ALWAYS int32 whatever the LLR type.  Returns (app[batch, n + p] int32, output, iters,
        success).  `scale_num`, `scale_shift` and `offset` as decode_ms_layered_fixed_batch
        (labrador_ldpc_decode_ms_layered_fixed_corrected_soft_batch_i8 / _i16)."""
        extra = _fixed_correction(scale_num, scale_shift, offset)
        if extra is None:
            return self._batch_call("labrador_ldpc_decode_ms_layered_fixed_soft_batch_", llrs, maxiters, output, iters, success, variant,
                                    stream, devices, soft=True, app=app, app_dtype="i32")
        return self._batch_call("labrador_ldpc_decode_ms_layered_fixed_corrected_soft_batch_", llrs, maxiters, output, iters, success,
                                variant, stream, devices, soft=True, app=app, app_dtype="i32", extra=extra)

    def decode_ms_cascade_batch(self, llrs, maxiters: int = 50, max_sweeps: Optional[int] = None, output=None, iters=None, success=None,
                                stage=None, variant: int = 0, stream: Optional[int] = None, devices=None, scale: float = 1.0,
                                offset: float = 0.0, flooding_scale: float = 1.0, flooding_offset: float = 0.0):
        """Two-stage decoding of f32 LLRs (labrador_ldpc_decode_ms_cascade_batch_f32): decode_ms_batch at cap
        `maxiters` and kernel `variant`, then decode_ms_layered_batch at cap `max_sweeps` (None = `maxiters`) and (`scale`,
        `offset`) on the original LLRs of the frames the first stage failed.  `stage[batch]` u8 says whose results a frame carries
        (0 = flooding, 1 = layered) and `iters` is in that stage's unit.  Buffers, `stream` and `devices` as decode_ms_batch, but
        with device buffers the call waits on the stream once for the first stage before it returns with the second enqueued.
        Returns (output, iters, success, stage).

        `flooding_scale`, `flooding_offset`: the first stage as decode_ms_batch at that (`scale`, `offset`) pair
        (labrador_ldpc_decode_ms_cascade_corrected_batch_f32): float32 LLRs and `variant` 0 only.  The defaults
        are the plain first stage through the entry point above."""
        if flooding_scale == 1.0 and flooding_offset == 0.0:
            return self._batch_call("labrador_ldpc_decode_ms_cascade_batch_", llrs, maxiters, output, iters, success, variant, stream,
                                    devices, extra=(maxiters if max_sweeps is None else max_sweeps, float(scale), float(offset)),
                                    stage=stage, with_stage=True, types=("f32",), half=True)
        return self._batch_call("labrador_ldpc_decode_ms_cascade_corrected_batch_", llrs, maxiters, output, iters, success, variant, stream,
                                devices, extra=(maxiters if max_sweeps is None else max_sweeps, float(flooding_scale),
                                                float(flooding_offset), float(scale), float(offset)),
                                stage=stage, with_stage=True, types=("f32",))

    def decode_ms_corrected_fixed_batch(self, llrs, scale_num: int, scale_shift: int, offset: int, maxiters: int = 50, output=None,
                                        iters=None, success=None, stream: Optional[int] = None, devices=None):
        """Flooding min-sum on int8 LLRs with normalized / offset check messages in integers
        (labrador_ldpc_decode_ms_corrected_batch_i8): decode_ms_batch on int8 with one step added -- every check
        message magnitude m becomes max(((scale_num * m + ((1 << scale_shift) >> 1)) >> scale_shift) - offset, 0), the triple as
        decode_ms_layered_fixed_batch has it.  The bit-sliced kernels of the TM codes at every batch size: a TC code, or any dtype but
        int8, raises LdpcHipError.  With device buffers `llrs` must be 4-byte aligned.  Buffers, `stream` and `devices` as
        decode_ms_batch.  Returns (output, iters, success)."""
        return self._batch_call("labrador_ldpc_decode_ms_corrected_batch_", llrs, maxiters, output, iters, success, 0, stream, devices,
                                extra=_fixed_correction(scale_num, scale_shift, offset), types=("i8",))

    def decode_ms_cascade_fixed_batch(self, llrs, maxiters: int = 50, max_sweeps: Optional[int] = None, output=None, iters=None,
                                      success=None, stage=None, variant: int = 0, stream: Optional[int] = None, devices=None,
                                      scale_num: Optional[int] = None, scale_shift: Optional[int] = None, offset: Optional[int] = None,
                                      flooding_scale_num: Optional[int] = None, flooding_scale_shift: Optional[int] = None,
                                      flooding_offset: Optional[int] = None):
        """decode_ms_cascade_batch for int8 and int16 LLRs (labrador_ldpc_decode_ms_cascade_batch_i8 / _i16): the second stage is
        decode_ms_layered_fixed_batch with its `scale_num`, `scale_shift` and `offset` (none given: plain min-sum).

        `flooding_scale_num`, `flooding_scale_shift`, `flooding_offset`: the first stage as decode_ms_corrected_fixed_batch at that
        triple (labrador_ldpc_decode_ms_cascade_corrected_batch_i8): int8 LLRs only; with a triple other than an
        identity, the TM codes and `variant` 0 only.  None given: the plain first stage through the entry point above."""
        flooding = _fixed_correction(flooding_scale_num, flooding_scale_shift, flooding_offset)
        if flooding is not None:
            return self._batch_call("labrador_ldpc_decode_ms_cascade_corrected_batch_", llrs, maxiters, output, iters, success, variant,
                                    stream, devices,
                                    extra=(maxiters if max_sweeps is None else max_sweeps, *flooding,
                                           *(_fixed_correction(scale_num, scale_shift, offset) or (1, 0, 0))), stage=stage, with_stage=True,
                                    types=("i8",))
        return self._batch_call("labrador_ldpc_decode_ms_cascade_batch_", llrs, maxiters, output, iters, success, variant, stream, devices,
                                extra=(maxiters if max_sweeps is None else max_sweeps,
                                       *(_fixed_correction(scale_num, scale_shift, offset) or (1, 0, 0))), stage=stage, with_stage=True,
                                types=("i8", "i16"))

    def decode_ms_cascade_soft_batch(self, llrs, maxiters: int = 50, max_sweeps: Optional[int] = None, app=None, output=None, iters=None,
                                     success=None, stage=None, variant: int = 0, stream: Optional[int] = None, devices=None,
                                     scale: float = 1.0, offset: float = 0.0, flooding_scale: float = 1.0, flooding_offset: float = 0.0):
        """decode_ms_cascade_batch with soft output (labrador_ldpc_decode_ms_cascade_soft_batch_f32): also every
        frame's marginals from the stage it carries -- per frame exactly decode_ms_soft_batch at (`flooding_scale`,
        `flooding_offset`), and for the frames it failed decode_ms_layered_soft_batch at (`scale`, `offset`).  float32 LLRs only.
        Buffers, `stream` and `devices` as decode_ms_cascade_batch.  Returns (app[batch, n + p] float32 -- punctured variables
        last --, output, iters, success, stage); the last four are what decode_ms_cascade_batch returns."""
        return self._batch_call("labrador_ldpc_decode_ms_cascade_soft_batch_", llrs, maxiters, output, iters, success, variant, stream,
                                devices, soft=True, app=app,
                                extra=(maxiters if max_sweeps is None else max_sweeps, float(flooding_scale), float(flooding_offset),
                                       float(scale), float(offset)),
                                stage=stage, with_stage=True, types=("f32",))

    def decode_ms_cascade_fixed_soft_batch(self, llrs, maxiters: int = 50, max_sweeps: Optional[int] = None, app=None, output=None,
                                           iters=None, success=None, stage=None, variant: int = 0, stream: Optional[int] = None,
                                           devices=None, scale_num: Optional[int] = None, scale_shift: Optional[int] = None,
                                           offset: Optional[int] = None, bitsliced: bool = False,
                                           flooding_scale_num: Optional[int] = None, flooding_scale_shift: Optional[int] = None,
                                           flooding_offset: Optional[int] = None):
        """decode_ms_cascade_fixed_batch with soft output, for int8 and int16 LLRs (labrador_ldpc_decode_ms_cascade_soft_batch_i8 /
        _i16).  `app` is ALWAYS int32: a stage-0 frame holds the flooding decoder's saturating marginal of the LLR
        type, sign-extended; a stage-1 frame the layered decoder's exact sum -- marginals are comparable only within a stage.  There
        is no first-stage triple, and on a TM code the int8 first stage is the soft flooding kernel, not the bit-sliced one --
        unless `bitsliced` asks for it (labrador_ldpc_decode_ms_cascade_bitsliced_soft_batch_i8, DESIGN.md 4.16: the first stage as
        decode_ms_bitsliced_soft_batch; same results bit for bit; int8 LLRs, TM1536 / TM2048 / TM6144 / TM8192 and `variant` 0 only,
        device `llrs` 4-byte aligned).

        `flooding_scale_num`, `flooding_scale_shift`, `flooding_offset`: with `bitsliced`, the first stage as
        decode_ms_bitsliced_soft_batch at that triple (labrador_ldpc_decode_ms_cascade_bitsliced_corrected_soft_batch_i8, DESIGN.md
        4.18); the four hard results are decode_ms_cascade_fixed_batch's at the same arguments.  Without `bitsliced` a ValueError
        (StageOneTripleError, also a TypeError as before the keywords existed): a corrected soft first stage exists only bit-sliced.  None given: the entries above.
        Returns (app[batch, n + p] int32, output, iters, success, stage)."""
        flooding = _fixed_correction(flooding_scale_num, flooding_scale_shift, flooding_offset)
        if flooding is not None:
            if not bitsliced:
                raise StageOneTripleError("a corrected soft first stage exists only bit-sliced: flooding_scale_num, flooding_scale_shift "
                                          "and flooding_offset need bitsliced=True")
            return self._batch_call("labrador_ldpc_decode_ms_cascade_bitsliced_corrected_soft_batch_", llrs, maxiters, output, iters, success,
                                    variant, stream, devices, soft=True, app=app, app_dtype="i32",
                                    extra=(maxiters if max_sweeps is None else max_sweeps, *flooding,
                                           *(_fixed_correction(scale_num, scale_shift, offset) or (1, 0, 0))),
                                    stage=stage, with_stage=True, types=("i8",))
        if bitsliced:
            return self._batch_call("labrador_ldpc_decode_ms_cascade_bitsliced_soft_batch_", llrs, maxiters, output, iters, success, variant,
                                    stream, devices, soft=True, app=app, app_dtype="i32",
                                    extra=(maxiters if max_sweeps is None else max_sweeps,
                                           *(_fixed_correction(scale_num, scale_shift, offset) or (1, 0, 0))),
                                    stage=stage, with_stage=True, types=("i8",))
        return self._batch_call("labrador_ldpc_decode_ms_cascade_soft_batch_", llrs, maxiters, output, iters, success, variant, stream,
                                devices, soft=True, app=app, app_dtype="i32",
                                extra=(maxiters if max_sweeps is None else max_sweeps,
                                       *(_fixed_correction(scale_num, scale_shift, offset) or (1, 0, 0))),
                                stage=stage, with_stage=True, types=("i8", "i16"))

    def _batch_call(self, prefix, llrs, maxiters, output, iters, success, variant, stream, devices, soft=False, app=None, extra=(),
                    app_dtype=None, with_stage=False, stage=None, types=None, fn_name=None, half=False):
        # soft: the call also writes the marginals to `app` [batch, n + p], which comes back first
        # app_dtype: the dtype of `app` as a suffix ("i32"); None = the dtype of `llrs`
        # extra: arguments of the entry point between max_iters and opts
        # with_stage: the call also writes `stage` [batch] u8, which comes back last
        # types: the LLR types (suffixes) this method takes where the prefix has entries for more; None = whatever the prefix has
        # fn_name: the entry point itself, where the type of `llrs` does not choose it (the caller has checked that type)
        # half: float16 / bfloat16 `llrs` choose the prefix's _f16 / _bf16 entry, whose `app` is float32
        if not (_is_torch(llrs) or isinstance(llrs, np.ndarray)):
            raise ValueError("llrs must be a numpy array (host) or a torch CUDA tensor (device)")
        if llrs.ndim != 2 or llrs.shape[1] != self.n():
            raise ValueError("llrs must be [batch, n]")
        batch, np_len = llrs.shape[0], self.n() + self.punctured_bits()
        half_suffix = _half_suffix(llrs) if half else None
        try:
            if half_suffix is not None:
                fn, app_dtype = getattr(lib, prefix + half_suffix), "f32"
            elif fn_name is not None:
                fn = getattr(lib, fn_name)
            else:
                fn = getattr(lib, prefix + _suffix(llrs), None) if types is None or _suffix(llrs) in types else None
        except KeyError:
            fn = None
        if fn is None:
            raise LdpcHipError(f"no batched kernel for dtype {llrs.dtype}")
        keep = None
        if _is_torch(llrs):
            if not llrs.is_cuda:
                raise ValueError("torch tensors must live on the GPU (use numpy for host buffers)")
            if not llrs.is_contiguous():
                raise ValueError("llrs must be contiguous")
            if devices is not None:
                raise ValueError("device-resident buffers live on one device; `devices` is for host buffers")
            opts = _device_opts(llrs, stream, variant)
        else:
            llrs = np.ascontiguousarray(llrs)
        if soft:
            app = _result_buffer(app, llrs, (batch, np_len), app_dtype or _suffix(llrs), "app", exact=True)
        if not _is_torch(llrs):
            opts, keep = _host_opts(stream, variant, devices)
        output = _result_buffer(output, llrs, (batch, self.output_len()), "u8", "output")
        iters = _result_buffer(iters, llrs, (batch,), "i32", "iters")
        success = _result_buffer(success, llrs, (batch,), "u8", "success")
        results = (app, output, iters, success) if soft else (output, iters, success)
        if with_stage:
            results += (_result_buffer(stage, llrs, (batch,), "u8", "stage"),)
        _check(fn(int(self), _ptr(llrs), *(_ptr(r) for r in results), batch, maxiters, *extra, ctypes.byref(opts)))
        del keep
        return results

    def decode_ms_soft_batch(self, llrs, maxiters: int = 50, app=None, output=None, iters=None, success=None,
                             variant: int = 0, stream: Optional[int] = None, devices=None, scale: float = 1.0, offset: float = 0.0):
        """decode_ms_batch with soft output: also the decoder's a-posteriori LLR of every variable, the reference's `va`
        (src/decoder.rs:377) when decode_ms returns (labrador_ldpc_decode_ms_soft_batch_*).

        Buffers and `devices` / `stream` as in decode_ms_batch.  Returns (app[batch, n + p] in the dtype of `llrs` -- punctured
        variables last --, output[batch, output_len] u8, iters[batch] u32/i32, success[batch] u8); output, iters and success are
        what decode_ms_batch returns.  `scale` and `offset` as decode_ms_batch (labrador_ldpc_decode_ms_corrected_soft_batch_f32)."""
        if scale == 1.0 and offset == 0.0:
            return self._batch_call("labrador_ldpc_decode_ms_soft_batch_", llrs, maxiters, output, iters, success, variant, stream, devices,
                                    soft=True, app=app, half=True)
        return self._batch_call("labrador_ldpc_decode_ms_corrected_soft_batch_", llrs, maxiters, output, iters, success, variant, stream,
                                devices, soft=True, app=app, extra=(float(scale), float(offset)), types=("f32",))

    def decode_ms_bitsliced_soft_batch(self, llrs, maxiters: int = 50, app=None, output=None, iters=None, success=None,
                                       stream: Optional[int] = None, devices=None, scale_num: Optional[int] = None,
                                       scale_shift: Optional[int] = None, offset: Optional[int] = None):
        """decode_ms_soft_batch on int8 LLRs from the bit-sliced kernels (labrador_ldpc_decode_ms_bitsliced_soft_batch_i8, DESIGN.md
        4.16): the same four results bit for bit -- the marginals saturate as the reference's do and reach -128 -- at the bit-sliced
        kernels' rate, whatever the batch size.  TM1536, TM2048, TM6144 and TM8192 only: any other code, or any dtype but int8,
        raises LdpcHipError.  With device buffers `llrs` must be 4-byte and `app` 16-byte aligned.  Buffers, `stream` and `devices`
        as decode_ms_batch.  Returns (app[batch, n + p] int8 -- punctured variables last --, output, iters, success).

        `scale_num`, `scale_shift`, `offset`: normalized / offset min-sum, the triple as decode_ms_layered_fixed_batch resolves it
        (labrador_ldpc_decode_ms_bitsliced_corrected_soft_batch_i8): output, iters and success are
        decode_ms_corrected_fixed_batch's at that triple and `app` is that decoder's marginal.  None given: the entry above."""
        extra = _fixed_correction(scale_num, scale_shift, offset)
        if extra is not None:
            return self._batch_call("labrador_ldpc_decode_ms_bitsliced_corrected_soft_batch_", llrs, maxiters, output, iters, success, 0, stream,
                                    devices, soft=True, app=app, extra=extra, types=("i8",))
        return self._batch_call("labrador_ldpc_decode_ms_bitsliced_soft_batch_", llrs, maxiters, output, iters, success, 0, stream, devices,
                                soft=True, app=app, types=("i8",))

    def decode_ms_layered_soft_batch(self, llrs, maxiters: int = 50, app=None, output=None, iters=None, success=None,
                                     variant: int = 0, stream: Optional[int] = None, devices=None, scale: float = 1.0, offset: float = 0.0):
        """decode_ms_layered_batch with soft output (labrador_ldpc_decode_ms_layered_soft_batch_f32): also the marginals of the
        returned sweep.  Buffers and return shapes as decode_ms_soft_batch: (app[batch, n + p], output, iters, success).  `scale`
        and `offset` as decode_ms_layered_batch (labrador_ldpc_decode_ms_layered_corrected_soft_batch_f32)."""
        if scale == 1.0 and offset == 0.0:
            return self._batch_call("labrador_ldpc_decode_ms_layered_soft_batch_", llrs, maxiters, output, iters, success, variant, stream,
                                    devices, soft=True, app=app, half=True)
        return self._batch_call("labrador_ldpc_decode_ms_layered_corrected_soft_batch_", llrs, maxiters, output, iters, success, variant,
                                stream, devices, soft=True, app=app, extra=(float(scale), float(offset)), half=True)

    def decode_ms_batch_multi(self, parts, maxiters: int = 50, variant: int = 0):
        """Decode several device-resident batches -- one torch CUDA tensor `llrs[frames_i, n]` per part, each on its own (or the
        same) GPU -- with ONE call: every part is enqueued by the library's worker of its device and the call returns when all
        results are in place (labrador_ldpc_decode_ms_batch_*_multi; the reference's harness shape, one job over all workers,
        perftest/src/main.rs:39-52).  Returns a list of (output, iters, success) tensors, one triple per part."""
        import torch
        parts = list(parts)
        if not parts:
            return []
        if not all(_is_torch(p) and p.is_cuda and p.is_contiguous() and p.ndim == 2 and p.shape[1] == self.n() for p in parts):
            raise ValueError("every part must be a contiguous torch CUDA tensor [frames, n]")
        if len({p.dtype for p in parts}) != 1:
            raise ValueError("all parts must have one LLR type")
        fn = getattr(lib, "labrador_ldpc_decode_ms_batch_" + _suffix(parts[0]) + "_multi")
        res = [(torch.empty((p.shape[0], self.output_len()), dtype=torch.uint8, device=p.device),
                torch.empty((p.shape[0],), dtype=torch.int32, device=p.device),
                torch.empty((p.shape[0],), dtype=torch.uint8, device=p.device)) for p in parts]
        # The library's streams know nothing of torch's: what produced the inputs must be done.  Only torch's CURRENT stream of each
        # device is waited for here -- a caller that filled a part on another stream synchronises that stream itself before the call.
        for p in parts:
            torch.cuda.current_stream(p.device).synchronize()
        n = len(parts)
        arr = lambda vals, t: (t * n)(*vals)
        # get_device(): the ordinal the memory lives on, also for a tensor made on torch.device("cuda") (index None) while another
        # GPU than 0 is current (round 5 advice: `index or 0` sent such a part to device 0)
        devs = arr([p.get_device() for p in parts], ctypes.c_int)
        _check(fn(int(self), n, devs, arr([_ptr(p) for p in parts], ctypes.c_void_p), arr([_ptr(r[0]) for r in res], ctypes.c_void_p),
                  arr([_ptr(r[1]) for r in res], ctypes.c_void_p), arr([_ptr(r[2]) for r in res], ctypes.c_void_p),
                  arr([p.shape[0] for p in parts], ctypes.c_size_t), maxiters, variant))
        return res

    # ---- bit-flipping decoder: src/decoder.rs:243-301 ----
    def decode_bf(self, input: np.ndarray, output: np.ndarray, working: Optional[np.ndarray] = None,
                  maxiters: int = 50) -> Tuple[bool, int]:
        """One codeword on the GPU; (success, iterations) like the crate (length checks of :247-249)."""
        inp = _as_u8(input, self.n() // 8, "input.len() != n/8")
        out = _as_u8(output, self.output_len(), "output.len != (n+p)/8")
        if working is not None and working.shape != (self.decode_bf_working_len(),):
            raise ValueError("working.len() incorrect")
        iters = ctypes.c_size_t(0)
        ok = lib.labrador_ldpc_decode_bf(int(self), inp.ctypes.data, out.ctypes.data, None, maxiters, ctypes.byref(iters))
        err = last_error()
        if not ok and err:
            raise LdpcHipError(err)
        return bool(ok), int(iters.value)

    def decode_bf_batch(self, input, maxiters: int = 50, stream: Optional[int] = None, devices=None, output=None, iters=None,
                        success=None):
        """input[batch, n/8] -> (output[batch, output_len], iters[batch], success[batch]).
        numpy = host buffers, torch CUDA uint8 tensors = device buffers (asynchronous).  `output`, `iters`, `success`: the caller's
        result buffers, as decode_ms_batch takes them (None = new ones); with all three given the call allocates nothing, which is
        what a stream under graph capture needs."""
        if input.ndim != 2 or input.shape[1] != self.n() // 8:
            raise ValueError("input must be [batch, n/8]")
        batch = input.shape[0]
        if _is_torch(input):
            import torch
            if not (input.is_cuda and input.dtype == torch.uint8 and input.is_contiguous()):
                raise ValueError("input must be a contiguous uint8 CUDA tensor")
            opts = _device_opts(input, stream)
        else:
            input = np.ascontiguousarray(input, dtype=np.uint8)
            opts, _keep = _host_opts(stream, 0, devices)
        output = _result_buffer(output, input, (batch, self.output_len()), "u8", "output")
        iters = _result_buffer(iters, input, (batch,), "i32", "iters")
        success = _result_buffer(success, input, (batch,), "u8", "success")
        _check(lib.labrador_ldpc_decode_bf_batch(int(self), _ptr(input), _ptr(output), _ptr(iters), _ptr(success),
                                                 batch, maxiters, ctypes.byref(opts)))
        return output, iters, success

    def encode_batch(self, data, codewords=None, stream: Optional[int] = None, devices=None):
        """Batched `copy_encode`: data[batch, k/8] -> codewords[batch, n/8] on the GPU.
        numpy = host buffers (synchronous), torch CUDA uint8 tensors = device buffers (asynchronous)."""
        if data.ndim != 2 or data.shape[1] != self.k() // 8:
            raise ValueError("data must be [batch, k/8]")
        batch = data.shape[0]
        if _is_torch(data):
            import torch
            if not (data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous()):
                raise ValueError("data must be a contiguous uint8 CUDA tensor")
            opts = _device_opts(data, stream)
        else:
            data = np.ascontiguousarray(data, dtype=np.uint8)
            opts, _keep = _host_opts(stream, 0, devices)
        codewords = _result_buffer(codewords, data, (batch, self.n() // 8), "u8", "codewords")
        _check(lib.labrador_ldpc_encode_batch(int(self), _ptr(data), _ptr(codewords), batch, ctypes.byref(opts)))
        return codewords

    # ---- LLR helpers, batched (src/decoder.rs:484-509 frame after frame) ----
    def hard_to_llrs_batch(self, input, dtype="f32", llrs=None, stream: Optional[int] = None):
        """input[batch, n/8] packed bits -> llrs[batch, n] of +-1 (`dtype`: "i8", "i16", "i32", "f32", "f64").
        torch CUDA uint8 tensor = on the device, asynchronous on the stream; numpy = host code."""
        if input.ndim != 2 or input.shape[1] != self.n() // 8:
            raise ValueError("input must be [batch, n/8]")
        batch = input.shape[0]
        if dtype not in _NP_DTYPE:
            raise KeyError(dtype)
        if _is_torch(input):
            import torch
            if not (input.is_cuda and input.dtype == torch.uint8 and input.is_contiguous()):
                raise ValueError("input must be a contiguous uint8 CUDA tensor")
            opts = _device_opts(input, stream)
        else:
            input = np.ascontiguousarray(input, dtype=np.uint8)
            opts = HipOpts(DEVICE_CURRENT, MEM_HOST, None, 0, 0, None)
        llrs = _result_buffer(llrs, input, (batch, self.n()), dtype, "llrs", exact=True)
        _check(getattr(lib, "labrador_ldpc_hard_to_llrs_batch_" + dtype)(int(self), _ptr(input), _ptr(llrs), batch, ctypes.byref(opts)))
        return llrs

    def llrs_to_hard_batch(self, llrs, output=None, stream: Optional[int] = None):
        """llrs[batch, n] -> output[batch, n/8] packed hard decisions (bit set where the LLR is < 0)."""
        if llrs.ndim != 2 or llrs.shape[1] != self.n():
            raise ValueError("llrs must be [batch, n]")
        batch = llrs.shape[0]
        if _is_torch(llrs):
            if not (llrs.is_cuda and llrs.is_contiguous()):
                raise ValueError("llrs must be a contiguous CUDA tensor")
            opts = _device_opts(llrs, stream)
        else:
            if llrs.dtype not in _NP_SUFFIX:
                raise ValueError("llrs dtype must be one of int8, int16, int32, float32, float64")
            llrs = np.ascontiguousarray(llrs)
            opts = HipOpts(DEVICE_CURRENT, MEM_HOST, None, 0, 0, None)
        output = _result_buffer(output, llrs, (batch, self.n() // 8), "u8", "output")
        _check(getattr(lib, "labrador_ldpc_llrs_to_hard_batch_" + _suffix(llrs))(int(self), _ptr(llrs), _ptr(output), batch, ctypes.byref(opts)))
        return output

    # ---- packed hard decisions to the bit-sliced i8 min-sum kernels ----
    def decode_ms_hard_batch(self, input, maxiters: int = 50, magnitude: int = 1, erasures=None, output=None, iters=None, success=None,
                             stream: Optional[int] = None, devices=None, scale_num: Optional[int] = None,
                             scale_shift: Optional[int] = None, offset: Optional[int] = None):
        """Decode packed hard decisions `input[batch, n/8]` (MSB first, as decode_bf_batch takes them) by min-sum on the bit-sliced i8
        kernels, whose loader reads the packed rows itself (labrador_ldpc_decode_ms_bitsliced_hard_batch_i8): per frame exactly
        decode_ms_batch on the int8 frame that is 0 where the bit of `erasures[batch, n/8]` is set, else -magnitude where the bit of
        `input` is set, else +magnitude -- without that frame ever existing.  `magnitude` 1 .. 127 (1 is hard_to_llrs_batch's frame);
        `erasures` None = no position erased.  `scale_num`, `scale_shift`, `offset`: the normalized / offset check messages of
        decode_ms_corrected_fixed_batch (labrador_ldpc_decode_ms_bitsliced_hard_corrected_batch_i8); none given: the plain entry.
        numpy = host buffers, which cross the link packed; torch CUDA uint8 tensors = device buffers (asynchronous on `stream`, 4-byte
        aligned, may be captured into a graph).  TM1536, TM2048, TM6144 and TM8192.  Returns (output, iters, success)."""
        if not (_is_torch(input) or isinstance(input, np.ndarray)):
            raise ValueError("input must be a numpy array (host) or a torch CUDA tensor (device)")
        if input.ndim != 2 or input.shape[1] != self.n() // 8:
            raise ValueError("input must be [batch, n/8]")
        batch = input.shape[0]
        if erasures is not None:
            if not (_is_torch(erasures) or isinstance(erasures, np.ndarray)) or _is_torch(erasures) != _is_torch(input) \
                    or tuple(erasures.shape) != tuple(input.shape):
                raise ValueError("erasures must be of input's kind and shape")
        if not _is_torch(input):                         # (packed bits: a cast would change them without a word)
            for name, a in (("input", input), ("erasures", erasures)):
                if a is not None and a.dtype != np.uint8:
                    raise ValueError(f"{name} must be a uint8 array of packed bits, not {a.dtype}")
        if _is_torch(input):
            import torch
            for name, t in (("input", input), ("erasures", erasures)):
                if t is not None and not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.device == input.device):
                    raise ValueError(f"{name} must be a contiguous uint8 CUDA tensor" + ("" if t is input else " on input's device"))
            opts = _device_opts(input, stream)
        else:
            input = np.ascontiguousarray(input)
            if erasures is not None:
                erasures = np.ascontiguousarray(erasures)
            opts, _keep = _host_opts(stream, 0, devices)
        output = _result_buffer(output, input, (batch, self.output_len()), "u8", "output")
        iters = _result_buffer(iters, input, (batch,), "i32", "iters")
        success = _result_buffer(success, input, (batch,), "u8", "success")
        triple = _fixed_correction(scale_num, scale_shift, offset)
        fn = getattr(lib, "labrador_ldpc_decode_ms_bitsliced_hard_" + ("batch_i8" if triple is None else "corrected_batch_i8"))
        _check(fn(int(self), _ptr(input), None if erasures is None else _ptr(erasures), _ptr(output), _ptr(iters), _ptr(success), batch,
                  maxiters, operator.index(magnitude), *(triple or ()), ctypes.byref(opts)))
        return output, iters, success

    # ---- f32 soft values to the integer decoders ----
    def quantise_llrs_batch(self, llrs, dtype="i8", scale: float = 8.0, lim: Optional[int] = None, out=None, stream: Optional[int] = None):
        """llrs[batch, n] float32 -> out[batch, n] of `dtype` ("i8", "i16") by the library's one quantisation rule
        (labrador_ldpc_quantise_llrs_batch_i8 / _i16): clamp(rint(scale * x), -lim, lim) on the f32 product, ties to even, NaN -> 0.
        `lim` None is the type's maximum (127 / 32767).  numpy = the library's host loop; a torch CUDA float32 tensor = the kernel,
        asynchronous on `stream` (`llrs` and `out` 16-byte aligned).  The library checks `scale` and `lim` (LdpcHipError)."""
        np_dtype = _quantised_dtype(dtype)
        if not (_is_torch(llrs) or isinstance(llrs, np.ndarray)):
            raise ValueError("llrs must be a numpy array (host) or a torch CUDA tensor (device)")
        if llrs.ndim != 2 or llrs.shape[1] != self.n():
            raise ValueError("llrs must be [batch, n]")
        if _suffix_or_none(llrs) != "f32":
            raise ValueError("llrs must be float32")
        batch = llrs.shape[0]
        if _is_torch(llrs):
            if not (llrs.is_cuda and llrs.is_contiguous()):
                raise ValueError("llrs must be a contiguous float32 CUDA tensor")
            opts = _device_opts(llrs, stream)
        else:
            llrs = np.ascontiguousarray(llrs)
            opts = HipOpts(DEVICE_CURRENT, MEM_HOST, None, 0, 0, None)
        out = _result_buffer(out, llrs, (batch, self.n()), dtype, "out", exact=True)
        lim = int(np.iinfo(np_dtype).max) if lim is None else operator.index(lim)
        _check(getattr(lib, "labrador_ldpc_quantise_llrs_batch_" + dtype)(int(self), _ptr(llrs), _ptr(out), batch, float(scale), lim,
                                                                          ctypes.byref(opts)))
        return out

    # ---- f16 / bf16 soft values to the f32 decoders ----
    def widen_llrs_batch(self, llrs, out=None, stream: Optional[int] = None):
        """llrs[batch, n] float16 (numpy, torch) or bfloat16 (torch) -> out[batch, n] float32 by the library's one widening rule
        (labrador_ldpc_widen_llrs_batch_f16 / _bf16): f16 to its exact value, a NaN to the quiet NaN of its sign and payload; bf16 to
        its bits << 16.  numpy = the library's host loop; a torch CUDA tensor = the kernel, asynchronous on `stream` (`llrs` and
        `out` 16-byte aligned).  The decoders take halves themselves; this is for a caller that wants the float32 rows."""
        if not (_is_torch(llrs) or isinstance(llrs, np.ndarray)):
            raise ValueError("llrs must be a numpy array (host) or a torch CUDA tensor (device)")
        if llrs.ndim != 2 or llrs.shape[1] != self.n():
            raise ValueError("llrs must be [batch, n]")
        suffix = _half_suffix(llrs)
        if suffix is None:
            raise ValueError("llrs must be float16 or bfloat16")
        batch = llrs.shape[0]
        if _is_torch(llrs):
            if not (llrs.is_cuda and llrs.is_contiguous()):
                raise ValueError("llrs must be a contiguous CUDA tensor")
            opts = _device_opts(llrs, stream)
        else:
            llrs = np.ascontiguousarray(llrs)
            opts = HipOpts(DEVICE_CURRENT, MEM_HOST, None, 0, 0, None)
        out = _result_buffer(out, llrs, (batch, self.n()), "f32", "out", exact=True)
        _check(getattr(lib, "labrador_ldpc_widen_llrs_batch_" + suffix)(int(self), _ptr(llrs), _ptr(out), batch, ctypes.byref(opts)))
        return out

    def decode_ms_quantised_batch(self, llrs, dtype="i8", scale: float = 8.0, lim: Optional[int] = None, maxiters: int = 50, output=None,
                                  iters=None, success=None, variant: int = 0, stream: Optional[int] = None, devices=None,
                                  bitsliced: bool = False, scale_num: Optional[int] = None, scale_shift: Optional[int] = None,
                                  offset: Optional[int] = None):
        """Decode float32 `llrs[batch, n]` through the integer flooding kernels of `dtype` ("i8", "i16") in one call
        (labrador_ldpc_decode_ms_quantised_batch_i8 / _i16): per frame exactly decode_ms_batch on quantise_llrs_batch(llrs, dtype,
        scale, lim), at kernel `variant`.  Buffers, `stream` and `devices` as decode_ms_batch; host rows cross the link as float32
        and are quantised on the device.  Returns (output, iters, success).

        `bitsliced=True`: the bit-sliced i8 kernels read the float32 rows themselves and quantise in their loader
        (labrador_ldpc_decode_ms_bitsliced_quantised_batch_i8) -- the same results bit for bit, in one launch without
        a quantised copy of the batch; TM1536, TM2048, TM6144 and TM8192, `dtype` "i8" and `variant` 0 only.  With it `scale_num`,
        `scale_shift` and `offset` give the normalized / offset check messages of decode_ms_corrected_batch
        (labrador_ldpc_decode_ms_bitsliced_quantised_corrected_batch_i8)."""
        np_dtype = _quantised_dtype(dtype)
        if (_is_torch(llrs) or isinstance(llrs, np.ndarray)) and _suffix_or_none(llrs) != "f32":
            raise ValueError("llrs must be float32")
        lim = int(np.iinfo(np_dtype).max) if lim is None else operator.index(lim)
        triple = _fixed_correction(scale_num, scale_shift, offset)
        if not bitsliced:
            if triple is not None:
                raise ValueError("scale_num, scale_shift and offset need bitsliced=True")
        else:
            if dtype != "i8":
                raise ValueError(f"bitsliced=True decodes dtype i8 only, not {dtype}")
            if variant != 0:
                raise ValueError("bitsliced=True has kernel variant 0 only")
            name = "labrador_ldpc_decode_ms_bitsliced_quantised_" + ("batch_i8" if triple is None else "corrected_batch_i8")
            return self._batch_call(None, llrs, maxiters, output, iters, success, 0, stream, devices,
                                    extra=(float(scale), lim, *(triple or ())), fn_name=name)
        return self._batch_call(None, llrs, maxiters, output, iters, success, variant, stream, devices, extra=(float(scale), lim),
                                fn_name="labrador_ldpc_decode_ms_quantised_batch_" + dtype)

    def _quantised_call(self, name, llrs, dtype, scale, lim, triple, maxiters, output, iters, success, variant, stream, devices,
                        caps=(), flooding=(), **kw):
        """the f32-input calls behind the fixed-point layered decoders and the integer cascade: `dtype` chooses the entry; `caps`
        (the cascade's max_sweeps), the quantiser's pair and the triple (none given: the identity) go behind maxiters"""
        np_dtype = _quantised_dtype(dtype)
        if (_is_torch(llrs) or isinstance(llrs, np.ndarray)) and _suffix_or_none(llrs) != "f32":
            raise ValueError("llrs must be float32")
        lim = int(np.iinfo(np_dtype).max) if lim is None else operator.index(lim)
        extra = (*caps, float(scale), lim, *flooding, *(_fixed_correction(*triple) or (1, 0, 0)))
        return self._batch_call(None, llrs, maxiters, output, iters, success, variant, stream, devices, extra=extra, fn_name=name + dtype,
                                **kw)

    def decode_ms_layered_quantised_batch(self, llrs, dtype="i8", scale: float = 8.0, lim: Optional[int] = None, maxiters: int = 50,
                                          output=None, iters=None, success=None, variant: int = 0, stream: Optional[int] = None,
                                          devices=None, scale_num: Optional[int] = None, scale_shift: Optional[int] = None,
                                          offset: Optional[int] = None):
        """Decode float32 `llrs[batch, n]` through the fixed-point layered decoder of `dtype` ("i8", "i16") in one call
        (labrador_ldpc_decode_ms_layered_quantised_batch_i8 / _i16): per frame exactly decode_ms_layered_fixed_batch
        with `scale_num`, `scale_shift` and `offset` on quantise_llrs_batch(llrs, dtype, scale, lim).  The kernel quantises as it
        loads: no quantised copy of the batch exists, and with device buffers the call is asynchronous on `stream`.  Buffers,
        `stream` and `devices` as decode_ms_batch; `variant` 0 is the only kernel.  Returns (output, iters, success)."""
        return self._quantised_call("labrador_ldpc_decode_ms_layered_quantised_batch_", llrs, dtype, scale, lim,
                                    (scale_num, scale_shift, offset), maxiters, output, iters, success, variant, stream, devices)

    def decode_ms_layered_quantised_soft_batch(self, llrs, dtype="i8", scale: float = 8.0, lim: Optional[int] = None, maxiters: int = 50,
                                               app=None, output=None, iters=None, success=None, variant: int = 0,
                                               stream: Optional[int] = None, devices=None, scale_num: Optional[int] = None,
                                               scale_shift: Optional[int] = None, offset: Optional[int] = None):
        """decode_ms_layered_quantised_batch with soft output (labrador_ldpc_decode_ms_layered_quantised_soft_batch_i8 / _i16): also
        the marginals of the returned sweep, int32 in the units of the quantised LLRs.  Returns (app[batch, n + p] int32, output,
        iters, success), as decode_ms_layered_fixed_soft_batch on the quantised frames."""
        return self._quantised_call("labrador_ldpc_decode_ms_layered_quantised_soft_batch_", llrs, dtype, scale, lim,
                                    (scale_num, scale_shift, offset), maxiters, output, iters, success, variant, stream, devices,
                                    soft=True, app=app, app_dtype="i32")

    def decode_ms_cascade_quantised_batch(self, llrs, dtype="i8", scale: float = 8.0, lim: Optional[int] = None, maxiters: int = 50,
                                          max_sweeps: Optional[int] = None, output=None, iters=None, success=None, stage=None,
                                          variant: int = 0, stream: Optional[int] = None, devices=None, scale_num: Optional[int] = None,
                                          scale_shift: Optional[int] = None, offset: Optional[int] = None,
                                          flooding_scale_num: Optional[int] = None, flooding_scale_shift: Optional[int] = None,
                                          flooding_offset: Optional[int] = None, bitsliced: bool = False):
        """Decode float32 `llrs[batch, n]` through the integer cascade of `dtype` ("i8", "i16") in one call
        (labrador_ldpc_decode_ms_cascade_quantised_batch_i8 / _i16): per frame exactly decode_ms_cascade_fixed_batch
        -- flooding at cap `maxiters` and kernel `variant`, then the fixed-point layered decoder at cap `max_sweeps` (None =
        `maxiters`) and the triple on the frames it failed -- on quantise_llrs_batch(llrs, dtype, scale, lim).  With device buffers
        `llrs` must be 16-byte aligned, the call waits on the stream once per chunk of frames, and it must not run on a stream under
        capture.  Returns (output, iters, success, stage).

        `flooding_scale_num`, `flooding_scale_shift`, `flooding_offset`: the first stage's triple, as decode_ms_cascade_fixed_batch
        has it (labrador_ldpc_decode_ms_cascade_quantised_corrected_batch_i8): `dtype` "i8" only.

        `bitsliced=True`: both stages read float32 rows and quantise in their loaders
        (labrador_ldpc_decode_ms_cascade_bitsliced_quantised_batch_i8) -- the same four results bit for bit without a
        quantised copy of the batch; TM1536, TM2048, TM6144 and TM8192, `dtype` "i8" and `variant` 0 only."""
        flooding = _fixed_correction(flooding_scale_num, flooding_scale_shift, flooding_offset)
        if bitsliced:
            if dtype != "i8":
                raise ValueError(f"bitsliced=True decodes dtype i8 only, not {dtype}")
            if variant != 0:
                raise ValueError("bitsliced=True has kernel variant 0 only")
            return self._quantised_call("labrador_ldpc_decode_ms_cascade_bitsliced_quantised_batch_", llrs, dtype, scale, lim,
                                        (scale_num, scale_shift, offset), maxiters, output, iters, success, 0, stream, devices,
                                        caps=(maxiters if max_sweeps is None else max_sweeps,), flooding=flooding or (1, 0, 0), stage=stage,
                                        with_stage=True)
        if flooding is not None:
            if dtype != "i8":
                _quantised_dtype(dtype)
                raise LdpcHipError(f"no corrected first stage for dtype {dtype} (i8 only)")
            return self._quantised_call("labrador_ldpc_decode_ms_cascade_quantised_corrected_batch_", llrs, dtype, scale, lim,
                                        (scale_num, scale_shift, offset), maxiters, output, iters, success, variant, stream, devices,
                                        caps=(maxiters if max_sweeps is None else max_sweeps,), flooding=flooding, stage=stage,
                                        with_stage=True)
        return self._quantised_call("labrador_ldpc_decode_ms_cascade_quantised_batch_", llrs, dtype, scale, lim,
                                    (scale_num, scale_shift, offset), maxiters, output, iters, success, variant, stream, devices,
                                    caps=(maxiters if max_sweeps is None else max_sweeps,), stage=stage, with_stage=True)

    def _bitsliced_quantised_soft_call(self, name, llrs, maxiters, extra, app, app_dtype, output, iters, success, stream, devices, **kw):
        """the float32-input soft calls on the bit-sliced int8 kernels: `name` is the entry, `extra` what goes
        behind maxiters; any dtype but float32 has no kernel"""
        if (_is_torch(llrs) or isinstance(llrs, np.ndarray)) and _suffix_or_none(llrs) != "f32":
            raise LdpcHipError(f"no batched kernel for dtype {llrs.dtype} (float32 only)")
        return self._batch_call(None, llrs, maxiters, output, iters, success, 0, stream, devices, soft=True, app=app, app_dtype=app_dtype,
                                extra=extra, fn_name=name, **kw)

    def decode_ms_bitsliced_quantised_soft_batch(self, llrs, scale: float, lim: int, maxiters: int = 50, app=None, output=None, iters=None,
                                                 success=None, stream: Optional[int] = None, devices=None,
                                                 scale_num: Optional[int] = None, scale_shift: Optional[int] = None,
                                                 offset: Optional[int] = None):
        """Decode float32 `llrs[batch, n]` on the bit-sliced int8 kernels WITH soft output in one call
        (labrador_ldpc_decode_ms_bitsliced_quantised_soft_batch_i8): per frame exactly decode_ms_bitsliced_soft_batch on
        quantise_llrs_batch(llrs, "i8", scale, lim), all four results bit for bit.  The kernel quantises as it loads: no quantised
        copy of the batch exists, and with device buffers the call is one launch, asynchronous on `stream`.  TM1536, TM2048, TM6144
        and TM8192 only; float32 numpy arrays or torch tensors only -- any other dtype raises LdpcHipError.  With device buffers
        `llrs` and `app` must be 16-byte aligned.  Buffers, `stream` and `devices` as decode_ms_batch.

        `scale_num`, `scale_shift`, `offset`: normalized / offset min-sum, the triple as decode_ms_bitsliced_soft_batch takes it
        (labrador_ldpc_decode_ms_bitsliced_quantised_corrected_soft_batch_i8).  None given: the plain entry.
        Returns (app[batch, n + p] int8 -- punctured variables last --, output, iters, success)."""
        triple = _fixed_correction(scale_num, scale_shift, offset)
        name = "labrador_ldpc_decode_ms_bitsliced_quantised_" + ("soft_batch_i8" if triple is None else "corrected_soft_batch_i8")
        return self._bitsliced_quantised_soft_call(name, llrs, maxiters, (float(scale), operator.index(lim), *(triple or ())), app, "i8",
                                                   output, iters, success, stream, devices)

    def decode_ms_cascade_bitsliced_quantised_soft_batch(self, llrs, scale: float, lim: int, maxiters: int = 50,
                                                         max_sweeps: Optional[int] = None, app=None, output=None, iters=None, success=None,
                                                         stage=None, stream: Optional[int] = None, devices=None,
                                                         flooding_scale_num: Optional[int] = None, flooding_scale_shift: Optional[int] = None,
                                                         flooding_offset: Optional[int] = None, scale_num: Optional[int] = None,
                                                         scale_shift: Optional[int] = None, offset: Optional[int] = None):
        """Decode float32 `llrs[batch, n]` through the soft int8 cascade whose first stage is decode_ms_bitsliced_quantised_soft_batch
        (labrador_ldpc_decode_ms_cascade_bitsliced_quantised_soft_batch_i8): per frame exactly
        decode_ms_cascade_fixed_soft_batch(bitsliced=True) at the same caps and triples on quantise_llrs_batch(llrs, "i8", scale, lim),
        all five results bit for bit, without a quantised copy of the batch.  `flooding_*` is the first stage's triple, `scale_num`,
        `scale_shift` and `offset` the layered stage's; none given: the identity.  `max_sweeps` None = `maxiters`.  Codes, dtypes and
        alignments as decode_ms_bitsliced_quantised_soft_batch; the call waits on the stream once per launch slice and must not run
        on a stream under capture.  Returns (app[batch, n + p] int32, output, iters, success, stage)."""
        extra = (maxiters if max_sweeps is None else max_sweeps, float(scale), operator.index(lim),
                 *(_fixed_correction(flooding_scale_num, flooding_scale_shift, flooding_offset) or (1, 0, 0)),
                 *(_fixed_correction(scale_num, scale_shift, offset) or (1, 0, 0)))
        return self._bitsliced_quantised_soft_call("labrador_ldpc_decode_ms_cascade_bitsliced_quantised_soft_batch_i8", llrs, maxiters, extra,
                                                   app, "i32", output, iters, success, stream, devices, stage=stage, with_stage=True)

    # ---- synthetic channel (harness) ----
    def awgn_frames(self, codewords, batch: int, sigma: float, seed: int, dtype="f32",
                    scale: float = 8.0, lim: int = 31, out=None, stream: Optional[int] = None, first_frame: int = 0):
        """Fill `out[batch, n]` (device tensor) with BPSK+AWGN LLRs of the device-resident
        codeword pool `codewords[pool, n/8]` (see labrador_ldpc_hip_awgn_*_at): frames
        [first_frame, first_frame + batch) of the job `seed` names -- a shard generated with its own
        first_frame equals that slice of the whole job's buffer byte for byte."""
        import torch
        if not (codewords.is_cuda and codewords.dtype == torch.uint8 and codewords.is_contiguous()):
            raise ValueError("codewords must be a contiguous uint8 CUDA tensor [pool, n/8]")
        if dtype not in ("f32", "i8"):
            raise KeyError(dtype)
        out = _result_buffer(out, codewords, (batch, self.n()), dtype, "out", exact=True)
        opts = _device_opts(codewords, stream)
        if dtype == "f32":
            _check(lib.labrador_ldpc_hip_awgn_f32_at(int(self), codewords.data_ptr(), codewords.shape[0],
                                                     out.data_ptr(), first_frame, batch, sigma, seed, ctypes.byref(opts)))
        else:
            _check(lib.labrador_ldpc_hip_awgn_i8_at(int(self), codewords.data_ptr(), codewords.shape[0],
                                                    out.data_ptr(), first_frame, batch, sigma, scale, lim, seed,
                                                    ctypes.byref(opts)))
        return out


def _quantised_dtype(dtype) -> np.dtype:
    """the numpy dtype of a quantiser's `dtype` argument: "i8" or "i16", anything else is KeyError like the neighbours'"""
    if dtype not in ("i8", "i16"):
        raise KeyError(dtype)
    return _NP_DTYPE[dtype]


def _suffix_or_none(a):
    try:
        return _suffix(a)
    except KeyError:
        return None


def _as_u8(a: np.ndarray, length: int, msg: str) -> np.ndarray:
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 1 or not a.flags.c_contiguous:
        raise ValueError("expected a contiguous 1-D uint8 numpy array")
    if a.shape[0] != length:
        raise ValueError(msg)
    return a
