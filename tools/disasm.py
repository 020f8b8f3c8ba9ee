"""The gfx950 kernels of one object file of the build, disassembled: what the kernel-shape guards of the tests and tools/scan_kernels.py
read.  `.hip_fatbin` dumped, the gfx950 code object unbundled, `llvm-objdump -d`."""
import re
import subprocess
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(obj):
    """{kernel symbol: [(address, instruction text, branch target or None)]}; a branch target is an offset from the kernel's start."""
    tmp = tempfile.mkdtemp()
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={tmp}/fat", obj, "/dev/null"])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={tmp}/fat",
                           f"--output={tmp}/co", "--unbundle"])
    dis = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", f"{tmp}/co"], text=True).split("\n")
    out, cur = {}, None
    for line in dis:
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur and "//" in line:
            text, tail = line.split("//", 1)
            tgt = re.search(r"<[^>]*\+0x([0-9a-f]+)>", tail)
            out[cur].append((int(tail.split(":")[0].strip(), 16), text.strip(), int(tgt.group(1), 16) if tgt else None))
    return out
