"""Layered against flooding min-sum decoding: rate, mean passes and frame error rate of labrador_ldpc_decode_ms_layered_batch_f32 and
labrador_ldpc_decode_ms_batch_f32 on the SAME device-resident AWGN frames (awgn_frames, f32, 25 iterations), in one process,
alternating the two calls.
    python tools/layered_rate.py [frames]       -> one JSON line: per case both rates (M codewords/s), mean passes, FER and the kernels
Passes: a flooding decode that succeeds at iteration index i made i message passes (iteration 0 checks the LLRs themselves); a layered
decode that succeeds at sweep index i made i + 1 sweeps; a failure counts as 25 either way.  Cases: TC512 3 dB, TM2048 1.7 and 2 dB,
TM8192 2 dB.  Default 1 048 576 frames per case (TM8192: a quarter of that)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode

FRAMES = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
MAXITERS, REPS = 25, 3
CASES = (("TC512", 3.0), ("TM2048", 1.7), ("TM2048", 2.0), ("TM8192", 2.0))


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"frames": FRAMES, "maxiters": MAXITERS, "library_build": la.lib.labrador_ldpc_hip_build_id().decode(), "cases": []}
    for name, ebn0 in CASES:
        code = LDPCCode[name]
        frames = FRAMES // 4 if code == LDPCCode.TM8192 else FRAMES
        rng = np.random.default_rng(1)
        pool = np.zeros((64, code.n() // 8), np.uint8)
        for i in range(64):
            code.copy_encode(rng.integers(0, 256, code.k() // 8, dtype=np.uint8), pool[i])
        sigma = float(np.sqrt(1.0 / (2.0 * (code.k() / code.n()) * 10.0 ** (ebn0 / 10.0))))
        llrs = code.awgn_frames(torch.from_numpy(pool).to(dev), frames, sigma, seed=5, dtype="f32")
        out = {k: torch.empty((frames, code.output_len()), dtype=torch.uint8, device=dev) for k in ("flooding", "layered")}
        it = {k: torch.empty(frames, dtype=torch.int32, device=dev) for k in ("flooding", "layered")}
        ok = {k: torch.empty(frames, dtype=torch.uint8, device=dev) for k in ("flooding", "layered")}
        calls = {"flooding": lambda: code.decode_ms_batch(llrs, MAXITERS, output=out["flooding"], iters=it["flooding"], success=ok["flooding"]),
                 "layered": lambda: code.decode_ms_layered_batch(llrs, MAXITERS, output=out["layered"], iters=it["layered"],
                                                                 success=ok["layered"])}
        for fn in calls.values():                       # warm-up (and the occupancy queries)
            fn()
        torch.cuda.synchronize()
        best = {k: 1e9 for k in calls}
        for _ in range(REPS):
            for key, fn in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                best[key] = min(best[key], a.elapsed_time(b))
        case = {"code": name, "ebn0_db": ebn0, "frames": frames,
                "kernels": {"flooding": "decode_ms_pair_kernel" if code == LDPCCode.TM8192 else "decode_ms_kernel",
                            "layered": "decode_ms_layered_kernel"}}
        for key in calls:
            succ = ok[key].to(torch.int64)
            passes = torch.where(succ == 1, it[key].to(torch.int64) + (1 if key == "layered" else 0), torch.full_like(succ, MAXITERS))
            case[key] = {"mcw_s": round(frames / best[key] / 1e3, 3), "ms": round(best[key], 3),
                         "mean_passes": round(float(passes.double().mean()), 3), "fer": float(1.0 - succ.double().mean())}
        case["layered_over_flooding"] = round(case["layered"]["mcw_s"] / case["flooding"]["mcw_s"], 4)
        res["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
        del llrs, out, it, ok
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
