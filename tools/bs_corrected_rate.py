"""Rate of the corrected bit-sliced i8 kernels (labrador_ldpc_decode_ms_corrected_batch_i8) on the frames of tools/bs_ab.py,
every repetition kept, with a digest of every output and the frames failed:
    python tools/bs_corrected_rate.py [frames-of-TM8192-size] [NUM,SHIFT,OFFSET ...] [case ...]
The yardstick is tools/bs_ab.py (the plain bit-sliced kernel, `variant` 64) on the same frames and cap, which runs against any build:
    LABRADOR_LDPC_HIP_LIB=<the parent commit's library> python tools/bs_ab.py <frames> TM8192 TM2048 TM5120"""
import sys, os, hashlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from labrador_ldpc_amd import LDPCCode
args = sys.argv[1:]
frames = int(args.pop(0)) if args and args[0].isdigit() else 262144
triples = [tuple(int(x) for x in a.split(",")) for a in args if "," in a] or [(13, 4, 0), (1, 0, 0)]
want = [a for a in args if "," not in a]
dev = torch.device("cuda", 0)
CASES = (("TM8192", 2.0), ("TM2048", 2.0), ("TM5120", 4.0), ("TM6144", 3.0), ("TM1536", 3.0), ("TM1280", 4.0))
for name, ebn0 in CASES:
    if want and name not in want:
        continue
    code = LDPCCode[name]
    rng = np.random.default_rng(1)
    pool = np.zeros((64, code.n() // 8), np.uint8)
    for i in range(64):
        code.copy_encode(rng.integers(0, 256, code.k() // 8, dtype=np.uint8), pool[i])
    sigma = float(np.sqrt(1.0 / (2.0 * (code.k() / code.n()) * 10.0 ** (ebn0 / 10.0))))
    fr = frames * 8192 // code.n()
    llrs8 = code.awgn_frames(torch.from_numpy(pool).to(dev), fr, sigma, seed=5, dtype="i8")
    for triple in triples:
        out = code.decode_ms_corrected_fixed_batch(llrs8, *triple, maxiters=25)
        torch.cuda.synchronize()
        rates = []
        for rep in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(3):
                out = code.decode_ms_corrected_fixed_batch(llrs8, *triple, maxiters=25)
            b.record(); torch.cuda.synchronize()
            rates.append(fr / (a.elapsed_time(b) / 3) / 1e3)
        h = hashlib.sha256()
        for t in out:
            h.update(t.cpu().numpy().tobytes())
        print(f"{name} {ebn0} dB {fr} frames {triple}  M codewords/s {' '.join(f'{r:.2f}' for r in rates)}  mean iters "
              f"{float(out[1].double().mean()):.2f}  failed {int((out[2] == 0).sum())}  digest {h.hexdigest()[:16]}", flush=True)
