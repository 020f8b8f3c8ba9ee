"""What the fixtures of the six tests/test_bitslice*_emu.py share: build the CPU emulators (tests/c/bitslice*_emu.cpp, one shared object
per code: fully unrolled 64-lane code, half a minute to two minutes each at -O1) and load them."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "labrador_ldpc_amd", "csrc")
BACKEND = os.path.join(ROOT, "tests", "c", "bitslice_emu_backend.hpp")


def build(source, deps, names, flags=(), variants=None):
    """tests/c/<source> into build/lib<stem>_<name>.so for every code name, -> {name: ctypes.CDLL}.  A library older than the source, the
    shared backend header or one of `deps` (headers of csrc) is rebuilt, all stale ones in parallel: one g++ each; a compiler that
    fails fails the caller.  flags: further compiler flags.  variants {tag: name -> flags of that variant}: a library per name and
    tag, build/lib<stem>_<name>_<tag>.so, -> {(name, tag): ctypes.CDLL}."""
    source = os.path.join(ROOT, "tests", "c", source)
    stem = os.path.splitext(os.path.basename(source))[0]
    src = [source, BACKEND] + [os.path.join(CSRC, d) for d in deps]
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    libs, jobs = {}, []
    for name in names:
        for tag, more in (variants or {None: lambda name: []}).items():
            lib = os.path.join(ROOT, "build", f"lib{stem}_{name}.so" if tag is None else f"lib{stem}_{name}_{tag}.so")
            libs[name if tag is None else (name, tag)] = lib
            if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in src):
                jobs.append(subprocess.Popen(["g++", "-O1", "-std=c++20", "-shared", "-fPIC", f"-DEMU_CODE={name}", "-I" + CSRC] + list(flags) +
                                             list(more(name)) + [source, "-o", lib]))
    assert all(j.wait() == 0 for j in jobs)
    return {key: ctypes.CDLL(lib) for key, lib in libs.items()}
