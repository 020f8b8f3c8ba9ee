"""Soft output against hard-only decoding: rates of labrador_ldpc_decode_ms_soft_batch_* and labrador_ldpc_decode_ms_batch_* on the
SAME device-resident AWGN frames (awgn_frames, 2 dB, 25 iterations), in one process, alternating the two calls.
    python tools/soft_rate.py [frames]          -> one JSON line: per case both rates (M codewords/s), their ratio and the kernels
Cases: TC512 / TM2048 / TM8192 f32 (soft and hard on the same kernel family) and TM8192 i8 (soft on the f32-pipe kernel, hard on the
bit-sliced kernel the default dispatch takes at this batch size).  Default 1 048 576 frames per case."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode

FRAMES = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
EBN0, MAXITERS, REPS = 2.0, 25, 3


def kernels(code, dtype, frames):
    if dtype == "i8":
        hard = la.lib.labrador_ldpc_hip_decode_ms_i8_kernel(int(code), 0, frames).decode()
    else:
        hard = "decode_ms_pair_kernel" if code == LDPCCode.TM8192 else "decode_ms_kernel"
    soft = "soft_decode_ms_pair_kernel" if code == LDPCCode.TM8192 else "soft_decode_ms_kernel"
    return hard, soft


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"frames": FRAMES, "ebn0_db": EBN0, "maxiters": MAXITERS, "library_build": la.lib.labrador_ldpc_hip_build_id().decode(),
           "cases": []}
    for name, dtype in (("TC512", "f32"), ("TM2048", "f32"), ("TM8192", "f32"), ("TM8192", "i8")):
        code = LDPCCode[name]
        rng = np.random.default_rng(1)
        pool = np.zeros((64, code.n() // 8), np.uint8)
        for i in range(64):
            code.copy_encode(rng.integers(0, 256, code.k() // 8, dtype=np.uint8), pool[i])
        sigma = float(np.sqrt(1.0 / (2.0 * (code.k() / code.n()) * 10.0 ** (EBN0 / 10.0))))
        llrs = code.awgn_frames(torch.from_numpy(pool).to(dev), FRAMES, sigma, seed=5, dtype=dtype)
        out = torch.empty((FRAMES, code.output_len()), dtype=torch.uint8, device=dev)
        it = torch.empty(FRAMES, dtype=torch.int32, device=dev)
        ok = torch.empty(FRAMES, dtype=torch.uint8, device=dev)
        out_s, it_s, ok_s = torch.empty_like(out), torch.empty_like(it), torch.empty_like(ok)
        app = torch.empty((FRAMES, code.n() + code.punctured_bits()), dtype=llrs.dtype, device=dev)
        hard = lambda: code.decode_ms_batch(llrs, MAXITERS, output=out, iters=it, success=ok)
        soft = lambda: code.decode_ms_soft_batch(llrs, MAXITERS, app=app, output=out_s, iters=it_s, success=ok_s)
        hard(), soft()                                  # warm-up (and the occupancy queries)
        torch.cuda.synchronize()
        best = {"hard": 1e9, "soft": 1e9}
        for _ in range(REPS):
            for key, fn in (("hard", hard), ("soft", soft)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                best[key] = min(best[key], a.elapsed_time(b))
        same = bool(torch.equal(out, out_s) and torch.equal(it, it_s) and torch.equal(ok, ok_s))
        hk, sk = kernels(code, dtype, FRAMES)
        hr, sr = FRAMES / best["hard"] / 1e3, FRAMES / best["soft"] / 1e3
        res["cases"].append({"code": name, "dtype": dtype, "hard_mcw_s": round(hr, 3), "soft_mcw_s": round(sr, 3),
                             "soft_over_hard": round(sr / hr, 4), "hard_kernel": hk, "soft_kernel": sk,
                             "hard_ms": round(best["hard"], 3), "soft_ms": round(best["soft"], 3),
                             "mean_iters": round(float(it.double().mean()), 3), "success_rate": round(float(ok.double().mean()), 4),
                             "hard_results_identical": same})
        del llrs, out, it, ok, out_s, it_s, ok_s, app
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
