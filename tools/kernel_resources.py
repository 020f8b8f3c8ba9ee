"""VGPRs, spilled VGPRs, SGPRs, LDS bytes and scratch of every kernel in build/csrc/*.o (from the code objects' metadata notes).
    python tools/kernel_resources.py [substring ...]      # only kernels whose demangled name contains every substring
    python tools/kernel_resources.py --table NAME         # a named table (TABLES): a family's kernels beside the ones they are held against"""
import glob, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"

# name -> (objects, the family's kernel, the kernel of the same code it stands beside, waves per SIMD it is compiled for by code)
TABLES = {
    # the f32-reading soft kernels beside the soft kernels of the i8 source (4.16): the soft plan's placement
    "bs_quantised_soft": ("build/csrc/decode_ms_bs*soft_?.o", r"decode_ms_bsqc?a_kernel<(\d)(?:, (\d))?>", r"decode_ms_bsc?a_kernel<(\d)(?:, (\d))?>",
                          {4: 1, 5: 2, 7: 1, 8: 2}),
}
CODE_NAMES = {4: "TM1536", 5: "TM2048", 7: "TM6144", 8: "TM8192"}


def resources(pattern="build/csrc/*.o", agprs=False):
    """rows of (object, demangled name, vgprs, spilled, sgprs, lds, scratch), all text; with `agprs` an eighth field, the AGPR count"""
    rows = []
    for obj in sorted(glob.glob(os.path.join(ROOT, pattern))):
        tmp = tempfile.mkdtemp()
        r = subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={tmp}/fat", obj, "/dev/null"], capture_output=True)
        if r.returncode != 0:
            continue
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={tmp}/fat", f"--output={tmp}/co", "--unbundle"])
        notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", f"{tmp}/co"], text=True)
        for blk in notes.split("  - .agpr_count:")[1:]:
            get = lambda k: (re.search(rf"\.{k}:\s+(\S+)", blk) or [None, "?"])[1]
            name = get("name")
            dem = subprocess.check_output(["c++filt", name], text=True).strip()
            row = (os.path.basename(obj), dem, get("vgpr_count"), get("vgpr_spill_count"), get("sgpr_count"),
                   get("group_segment_fixed_size"), get("private_segment_fixed_size"))
            rows.append(row + (blk.split()[0],) if agprs else row)
    return rows


def table(name):
    """[(code, multiplier bits or None, waves per SIMD, the kernel's (vgprs, agprs, spilled, lds, scratch), the same of the kernel beside it)]"""
    pattern, mine, theirs, waves = TABLES[name]
    new, old = {}, {}
    for obj, dem, v, sp, s, lds, scr, a in resources(pattern, agprs=True):
        for rx, into in ((mine, new), (theirs, old)):
            m = re.search(rx, dem)
            if m:
                into[(int(m.group(1)), None if m.group(2) is None else int(m.group(2)))] = tuple(int(x) for x in (v, a, sp, lds, scr))
    return [(c, mb, waves[c], new[(c, mb)], old.get((c, mb))) for c, mb in sorted(new, key=lambda k: (k[0], -1 if k[1] is None else k[1]))]


if __name__ == "__main__":
    want = sys.argv[1:]
    if want[:1] == ["--table"]:
        if len(want) != 2 or want[1] not in TABLES:
            sys.exit(f"tables: {', '.join(TABLES)}")
        for code, mb, w, new, old in table(want[1]):
            fmt = lambda r: "-" if r is None else f"vgpr {r[0]:>3d} agpr {r[1]:>2d} spill {r[2]:>2d} lds {r[3]:>6d} scratch {r[4]:>3d}"
            print(f"{CODE_NAMES[code]} {'plain' if mb is None else 'mulbits %d' % mb:9s} waves/SIMD {w}   {fmt(new)}   beside: {fmt(old)}")
        sys.exit(0)
    for obj, dem, v, sp, s, lds, scr in resources():
        short = re.sub(r"^void ldpc::", "", dem).split("(")[0]
        if all(w in short for w in want):
            print(f"{obj:26s} {short:64s} vgpr {v:>4s} spill {sp:>4s} sgpr {s:>4s} lds {lds:>7s} scratch {scr:>5s}")
