"""Scan the code objects of the built library for signs of a mis-structured kernel: the count of EXEC-masked
loops (s_cbranch_execnz) per kernel.  The decode kernels' control flow is wave-uniform by construction (scalar
branches on the quarter a wave works on, on the verdict, on the clamp mode); when the compiler fails to see that,
or turns a per-lane select chain into branches, it emits EXEC-masked regions and loops -- correct, and 1.7x
(TM1280, round 2) to 100x (pair kernel on TM6144) slower.  A handful are legitimate (the sub-wave codeword
handling of the TC codes, the guarded epilogue stores).
    python tools/scan_kernels.py            # table of every kernel in build/csrc/decode_ms_*.o"""
import glob, os, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import disasm
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scan(pattern="build/csrc/decode_ms_*.o"):
    """{(object, kernel): (instructions, exec loops)}"""
    out = {}
    for obj in sorted(glob.glob(os.path.join(ROOT, pattern))):
        for kernel, body in disasm.kernels(obj).items():
            out[(os.path.basename(obj), kernel)] = [len(body), sum(text.startswith("s_cbranch_execnz") for _, text, _ in body)]
    return out


if __name__ == "__main__":
    for (obj, k), (n, loops) in scan().items():
        print(f"{obj:24s} {k[:64]:64s} {n:6d} instructions  {loops:4d} exec loops{'   <== look at this one' if loops > 16 else ''}")
