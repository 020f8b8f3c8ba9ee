"""Fixed-point layered min-sum decoding against the f32 layered and the flooding kernels: rate, mean passes and failures of
labrador_ldpc_decode_ms_layered_fixed_batch_i8 / _i16 next to labrador_ldpc_decode_ms_layered_batch_f32, labrador_ldpc_decode_ms_batch_f32
and labrador_ldpc_decode_ms_batch_i8, on device-resident AWGN frames (cap 25), in one process, the calls alternated.
    python tools/layered_fixed_rate.py [frames] [reps]      -> one JSON line: per case and decoder the rates of every repetition
                                                               (M codewords/s), their best and spread, mean passes and failures
The f32 frames are awgn_frames(dtype="f32"); the i8 frames are the i8 channel kernel's quantisation (8 / 31) of the same job seed,
and the i16 frames are those widened.  Passes: a flooding decode that succeeds at iteration index i made i passes, a layered one at
sweep index i made i + 1; a failure counts as 25.  Cases: TC512 3 dB, TM2048 1.7 and 2 dB, TM8192 2 dB.  Default
1 048 576 frames per case (TM8192: a quarter of that) and 5 repetitions.  The yardstick of DESIGN.md 4.7 is the f32 layered kernel:
`fixed_i8_over_layered_f32` is the ratio of the best rates, `layered_f32_spread` the (max - min) / max of that kernel's repetitions."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode

FRAMES = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
MAXITERS = 25
CASES = (("TC512", 3.0), ("TM2048", 1.7), ("TM2048", 2.0), ("TM8192", 2.0))
LAYERED = ("layered_f32", "fixed_i8", "fixed_i16")


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"frames": FRAMES, "maxiters": MAXITERS, "reps": REPS, "library_build": la.lib.labrador_ldpc_hip_build_id().decode(), "cases": []}
    for name, ebn0 in CASES:
        code = LDPCCode[name]
        frames = FRAMES // 4 if code == LDPCCode.TM8192 else FRAMES
        rng = np.random.default_rng(1)
        pool = np.zeros((64, code.n() // 8), np.uint8)
        for i in range(64):
            code.copy_encode(rng.integers(0, 256, code.k() // 8, dtype=np.uint8), pool[i])
        sigma = float(np.sqrt(1.0 / (2.0 * (code.k() / code.n()) * 10.0 ** (ebn0 / 10.0))))
        cw = torch.from_numpy(pool).to(dev)
        f32 = code.awgn_frames(cw, frames, sigma, seed=5, dtype="f32")
        i8 = code.awgn_frames(cw, frames, sigma, seed=5, dtype="i8", scale=8.0, lim=31)
        i16 = i8.to(torch.int16)
        keys = ("flooding_f32", "layered_f32", "flooding_i8", "fixed_i8", "fixed_i16")
        out = {k: torch.empty((frames, code.output_len()), dtype=torch.uint8, device=dev) for k in keys}
        it = {k: torch.empty(frames, dtype=torch.int32, device=dev) for k in keys}
        ok = {k: torch.empty(frames, dtype=torch.uint8, device=dev) for k in keys}

        def call(method, llrs, k):
            return lambda: method(llrs, MAXITERS, output=out[k], iters=it[k], success=ok[k])
        calls = {"flooding_f32": call(code.decode_ms_batch, f32, "flooding_f32"),
                 "layered_f32": call(code.decode_ms_layered_batch, f32, "layered_f32"),
                 "flooding_i8": call(code.decode_ms_batch, i8, "flooding_i8"),
                 "fixed_i8": call(code.decode_ms_layered_fixed_batch, i8, "fixed_i8"),
                 "fixed_i16": call(code.decode_ms_layered_fixed_batch, i16, "fixed_i16")}
        for fn in calls.values():                       # warm-up (and the occupancy queries)
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(REPS):
            for key, fn in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ms[key].append(a.elapsed_time(b))
        case = {"code": name, "ebn0_db": ebn0, "frames": frames}
        for key in calls:
            succ = ok[key].to(torch.int64)
            passes = torch.where(succ == 1, it[key].to(torch.int64) + (1 if key in LAYERED else 0), torch.full_like(succ, MAXITERS))
            rates = [frames / t / 1e3 for t in ms[key]]
            case[key] = {"mcw_s": round(max(rates), 3), "mcw_s_reps": [round(r, 3) for r in rates],
                         "spread": round((max(rates) - min(rates)) / max(rates), 4),
                         "mean_passes": round(float(passes.double().mean()), 3), "failures": int((succ == 0).sum())}
        for key in ("fixed_i8", "fixed_i16"):
            case[f"{key}_over_layered_f32"] = round(case[key]["mcw_s"] / case["layered_f32"]["mcw_s"], 4)
            case[f"{key}_over_flooding_i8"] = round(case[key]["mcw_s"] / case["flooding_i8"]["mcw_s"], 4)
        case["layered_f32_over_flooding_f32"] = round(case["layered_f32"]["mcw_s"] / case["flooding_f32"]["mcw_s"], 4)
        case["layered_f32_spread"] = case["layered_f32"]["spread"]
        res["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
        del f32, i8, i16, out, it, ok, calls
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
