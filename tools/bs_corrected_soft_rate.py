"""Soft output from the corrected bit-sliced i8 kernels (labrador_ldpc_decode_ms_bitsliced_corrected_soft_batch_i8): what it
runs at, beside the kernels it is measured against -- SAME device-resident AWGN frames (awgn_frames, 2 dB, cap 25), one process, the
calls alternating, the median of REPS timed repeats after a warm-up of each, every case with its spread ((max - min) / median).
    python tools/bs_corrected_soft_rate.py [frames-of-TM8192-size] [code ...]     -> one JSON line
Per code (TM1536, TM2048, TM6144, TM8192; about `frames` x 8192 LLRs each):
    soft        the plain soft bit-sliced entry, THE YARDSTICK      decode_ms_bitsliced_soft_batch()      (its kernel is untouched)
    hard  t     the hard corrected entry at triple t                decode_ms_corrected_fixed_batch(*t)
    new   t     the new entry at triple t                           decode_ms_bitsliced_soft_batch(scale_num=, scale_shift=, offset=)
for t = (1,0,0) -- the offset-only form at an identity --, (1,0,1) -- the offset alone -- and (13,4,0) -- a four-bit multiplier; with a
check that new t and hard t returned the same three hard arrays and that new (1,0,0) returned the plain soft entry's four.
Nothing here is a gate, and nothing was tuned on it."""
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
TRIPLES = ((1, 0, 0), (1, 0, 1), (13, 4, 0))


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
        keys = ["soft"] + [f"{kind}{t}" for t in TRIPLES for kind in ("hard", "new")]
        bufs = {k: (torch.empty((frames, code.output_len()), dtype=torch.uint8, device=dev), torch.empty(frames, dtype=torch.int32, device=dev),
                    torch.empty(frames, dtype=torch.uint8, device=dev)) for k in keys}
        app = {k: torch.empty((frames, code.n() + code.punctured_bits()), dtype=torch.int8, device=dev) for k in keys if not k.startswith("hard")}
        res_kw = lambda k: dict(output=bufs[k][0], iters=bufs[k][1], success=bufs[k][2])            # noqa: E731
        forms = {"soft": lambda: code.decode_ms_bitsliced_soft_batch(llrs, MAXITERS, app=app["soft"], **res_kw("soft"))}
        for t in TRIPLES:
            forms[f"hard{t}"] = lambda t=t: code.decode_ms_corrected_fixed_batch(llrs, *t, maxiters=MAXITERS, **res_kw(f"hard{t}"))
            forms[f"new{t}"] = lambda t=t: code.decode_ms_bitsliced_soft_batch(llrs, MAXITERS, app=app[f"new{t}"], scale_num=t[0], scale_shift=t[1],
                                                                               offset=t[2], **res_kw(f"new{t}"))
        for fn in forms.values():                       # warm-up
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
        spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in ms.items()}
        same = bool(all(torch.equal(x, y) for t in TRIPLES for x, y in zip(bufs[f"hard{t}"], bufs[f"new{t}"])) and
                    torch.equal(app["soft"], app["new(1, 0, 0)"]) and all(torch.equal(x, y) for x, y in zip(bufs["soft"], bufs["new(1, 0, 0)"])))
        case = {"code": name, "frames": frames, "results_identical": same}
        for k in forms:
            case[k] = {"mcw_s": round(rate[k], 3), "spread": round(spread[k], 4), "over_soft": round(rate[k] / rate["soft"], 3),
                       "mean_iters": round(float(bufs[k][1].double().mean()), 3), "success_rate": round(float(bufs[k][2].double().mean()), 4)}
        res["cases"].append(case)
        del llrs, bufs, app, forms
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
