"""Soft output from the bit-sliced i8 kernels (labrador_ldpc_decode_ms_bitsliced_soft_batch_i8): what it runs at, beside
the kernels it is measured against -- SAME device-resident AWGN frames (awgn_frames, 2 dB, cap 25), one process, the calls alternating,
the median of REPS timed repeats after a warm-up of each.
    python tools/bs_soft_rate.py [frames-of-TM8192-size] [code ...]     -> one JSON line
Per code (TM1536, TM2048, TM6144, TM8192; about `frames` x 8192 LLRs each):
    a  the hard bit-sliced LOCKSTEP kernel          decode_ms_batch(variant = 64 | 256)
    b  the hard default dispatch                    decode_ms_batch()
    c  the f32-pipe soft entry, THE YARDSTICK       decode_ms_soft_batch()            (labrador_ldpc_decode_ms_soft_batch_i8)
    d  the new entry                                decode_ms_bitsliced_soft_batch()
and d / c (the figure of merit), d / a (the price of the marginals), with a check that c and d returned the same four arrays.
The OTHER placement of the kept planes (BsPlan::SOFT_LDS) is a build of its own: compile decode_ms_bs_soft.hip for both units with
-DLDPC_TUNING_OVERRIDES_ALLOWED -DBS_SOFT_LDS_R12=1 -DBS_SOFT_LDS_R23=0, link those two objects with the rest of build/csrc/*.o, and
run this tool again with LABRADOR_LDPC_HIP_LIB=<that library>: the line's "library" names what was measured."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode

args = sys.argv[1:]
FRAMES = int(args.pop(0)) if args and args[0].isdigit() else 1 << 20
NAMES = args or ["TM8192", "TM2048", "TM6144", "TM1536"]
EBN0, MAXITERS, REPS = 2.0, 25, 5


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"frames_of_tm8192_size": FRAMES, "ebn0_db": EBN0, "maxiters": MAXITERS, "reps": REPS, "library": la.LIB_PATH,
           "library_build": la.lib.labrador_ldpc_hip_build_id().decode(), "cases": []}
    for name in NAMES:
        code = LDPCCode[name]
        frames = FRAMES * 8192 // code.n()
        rng = np.random.default_rng(1)
        pool = np.zeros((64, code.n() // 8), np.uint8)
        for i in range(64):
            code.copy_encode(rng.integers(0, 256, code.k() // 8, dtype=np.uint8), pool[i])
        sigma = float(np.sqrt(1.0 / (2.0 * (code.k() / code.n()) * 10.0 ** (EBN0 / 10.0))))
        llrs = code.awgn_frames(torch.from_numpy(pool).to(dev), frames, sigma, seed=5, dtype="i8")
        bufs = {k: (torch.empty((frames, code.output_len()), dtype=torch.uint8, device=dev), torch.empty(frames, dtype=torch.int32, device=dev),
                    torch.empty(frames, dtype=torch.uint8, device=dev)) for k in "abcd"}
        app = {k: torch.empty((frames, code.n() + code.punctured_bits()), dtype=torch.int8, device=dev) for k in "cd"}
        hard = lambda k, variant: code.decode_ms_batch(llrs, MAXITERS, output=bufs[k][0], iters=bufs[k][1], success=bufs[k][2], variant=variant)
        forms = {"a": lambda: hard("a", 64 | 256),
                 "b": lambda: hard("b", 0),
                 "c": lambda: code.decode_ms_soft_batch(llrs, MAXITERS, app=app["c"], output=bufs["c"][0], iters=bufs["c"][1], success=bufs["c"][2]),
                 "d": lambda: code.decode_ms_bitsliced_soft_batch(llrs, MAXITERS, app=app["d"], output=bufs["d"][0], iters=bufs["d"][1],
                                                                  success=bufs["d"][2])}
        for fn in forms.values():                       # warm-up (and the occupancy queries)
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in forms}
        for _ in range(REPS):
            for k, fn in forms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ms[k].append(a.elapsed_time(b))
        rate = {k: frames / statistics.median(v) / 1e3 for k, v in ms.items()}
        same = bool(torch.equal(app["c"], app["d"]) and all(torch.equal(x, y) for x, y in zip(bufs["c"], bufs["d"])) and
                    all(torch.equal(x, y) for x, y in zip(bufs["a"], bufs["d"])))
        res["cases"].append({"code": name, "frames": frames,
                             "a_hard_lockstep_mcw_s": round(rate["a"], 3), "b_hard_default_mcw_s": round(rate["b"], 3),
                             "c_soft_f32_pipe_mcw_s": round(rate["c"], 3), "d_soft_bitsliced_mcw_s": round(rate["d"], 3),
                             "d_over_c": round(rate["d"] / rate["c"], 3), "d_over_a": round(rate["d"] / rate["a"], 3),
                             "spread_d": round((max(ms["d"]) - min(ms["d"])) / statistics.median(ms["d"]), 4),
                             "hard_default_kernel": la.lib.labrador_ldpc_hip_decode_ms_i8_kernel(int(code), 0, frames).decode(),
                             "mean_iters": round(float(bufs["d"][1].double().mean()), 3),
                             "success_rate": round(float(bufs["d"][2].double().mean()), 4), "results_identical": same})
        del llrs, bufs, app, forms
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
