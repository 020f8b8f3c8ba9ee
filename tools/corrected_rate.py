"""Normalized / offset min-sum on the layered schedule: what the correction costs and what it buys.  Rate, mean passes and frame error
rate of flooding, plain layered and corrected layered decoding -- (1, 0), (0.8125, 0) and (1, 0.1) -- on the SAME device-resident AWGN
frames (awgn_frames, f32, y = +-1 + noise, 25 iterations), in one process, the calls alternated.
    python tools/corrected_rate.py [frames]     -> one JSON line: per case and decoder M codewords/s (best and worst of the
                                                   repetitions), mean passes and FER
Cost: corrected (1, 0) makes exactly the sweeps of plain layered decoding, so `unit_over_layered` is the price of the added instructions
and kernel arguments alone; `layered_spread` (worst / best of the plain call's repetitions) is what a difference has to exceed.
Passes: a flooding success at iteration i is i message passes, a layered success at sweep i is i + 1; a failure counts 25.  Cases: TC512
3 dB, TM2048 1.7 and 2 dB, TM8192 2 dB.  Default 1 048 576 frames per case (TM8192: a quarter of that)."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode

FRAMES = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
MAXITERS, REPS = 25, 5
CASES = (("TC512", 3.0), ("TM2048", 1.7), ("TM2048", 2.0), ("TM8192", 2.0))
CORRECTED = {"corrected_1_0": (1.0, 0.0), "corrected_0.8125_0": (0.8125, 0.0), "corrected_1_0.1": (1.0, 0.1)}
KEYS = ("flooding", "layered") + tuple(CORRECTED)


def corrected_call(code, llrs, out, it, ok, scale, offset):
    """The corrected symbol itself (the Python keywords at (1, 0) call the plain one)."""
    opts = la.HipOpts(llrs.device.index, la.MEM_DEVICE, torch.cuda.current_stream(llrs.device).cuda_stream, 0, 0, None)
    st = la.lib.labrador_ldpc_decode_ms_layered_corrected_batch_f32(int(code), llrs.data_ptr(), out.data_ptr(), it.data_ptr(), ok.data_ptr(),
                                                                    llrs.shape[0], MAXITERS, scale, offset, ctypes.byref(opts))
    assert st == 0, la.last_error()


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
        llrs = code.awgn_frames(torch.from_numpy(pool).to(dev), frames, sigma, seed=5, dtype="f32")
        out = {k: torch.empty((frames, code.output_len()), dtype=torch.uint8, device=dev) for k in KEYS}
        it = {k: torch.empty(frames, dtype=torch.int32, device=dev) for k in KEYS}
        ok = {k: torch.empty(frames, dtype=torch.uint8, device=dev) for k in KEYS}
        calls = {"flooding": lambda: code.decode_ms_batch(llrs, MAXITERS, output=out["flooding"], iters=it["flooding"], success=ok["flooding"]),
                 "layered": lambda: code.decode_ms_layered_batch(llrs, MAXITERS, output=out["layered"], iters=it["layered"],
                                                                 success=ok["layered"])}
        for key, (scale, offset) in CORRECTED.items():
            calls[key] = lambda key=key, scale=scale, offset=offset: corrected_call(code, llrs, out[key], it[key], ok[key], scale, offset)
        for fn in calls.values():                       # warm-up (and the occupancy queries)
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(REPS):
            for key, fn in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                times[key].append(a.elapsed_time(b))
        same = all(torch.equal(x["layered"], x["corrected_1_0"]) for x in (out, it, ok))
        case = {"code": name, "ebn0_db": ebn0, "frames": frames, "unit_equals_layered": bool(same)}
        for key in calls:
            succ = ok[key].to(torch.int64)
            passes = torch.where(succ == 1, it[key].to(torch.int64) + (0 if key == "flooding" else 1), torch.full_like(succ, MAXITERS))
            best, worst = min(times[key]), max(times[key])
            case[key] = {"mcw_s": round(frames / best / 1e3, 3), "mcw_s_worst": round(frames / worst / 1e3, 3), "ms": round(best, 3),
                         "mean_passes": round(float(passes.double().mean()), 3), "fer": float(1.0 - succ.double().mean())}
        case["layered_spread"] = round(case["layered"]["mcw_s_worst"] / case["layered"]["mcw_s"], 4)
        case["unit_over_layered"] = round(case["corrected_1_0"]["mcw_s"] / case["layered"]["mcw_s"], 4)
        for key in ("corrected_0.8125_0", "corrected_1_0.1"):
            case[key + "_over_layered"] = round(case[key]["mcw_s"] / case["layered"]["mcw_s"], 4)
        res["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
        del llrs, out, it, ok
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
