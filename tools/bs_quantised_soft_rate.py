"""Soft output from the f32-reading bit-sliced i8 kernels next to the two-step route they replace and to the hard entry (DESIGN.md
4.20), on device-resident f32 frames, in one process, the calls alternated inside every repetition and every repetition kept.
    python tools/bs_quantised_soft_rate.py [--codes TM8192,TM2048,TM1536,TM6144] [--reps 5] [--inner 20] [--frames CODE=N,...]
                                                             -> one JSON line (every case also to stderr as it finishes)
A repetition times `inner` calls back to back between two events (one call is a few milliseconds: too short a window to measure),
and every entry runs one untimed repetition first.
Per code, at 2 dB, cap 25, i8 at scale 8 / lim 31:
`flooding`, once without a triple and once at (13, 4, 0) --
(a) soft_f32   labrador_ldpc_decode_ms_bitsliced_quantised_[corrected_]soft_batch_i8 on the f32 frames: the new entry;
(b) two_step   the route it replaces: labrador_ldpc_quantise_llrs_batch_i8 into a buffer of the caller's, then
               labrador_ldpc_decode_ms_bitsliced_[corrected_]soft_batch_i8 on it -- THE YARDSTICK;
(c) hard_f32   labrador_ldpc_decode_ms_bitsliced_quantised_[corrected_]batch_i8: the same kernel without the marginals.
`cascade` at (13, 4, 0) / (13, 4, 0) -- soft_f32: labrador_ldpc_decode_ms_cascade_bitsliced_quantised_soft_batch_i8; hard_f32:
labrador_ldpc_decode_ms_cascade_bitsliced_quantised_batch_i8.
The tool ASSERTS that (a) and (b) return identical arrays, all four, and that the hard results of (a) and (c) are the same.  Per entry:
the best repetition, `reps` (all of them) and `spread` ((max - min) / max: what a difference has to exceed).  No pass mark on the
rates: the numbers go to DESIGN.md 4.20.
Default frames: TM8192 32 768, TM2048 131 072, TM6144 32 768, TM1536 131 072."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode

MAXITERS = 25
SCALE, LIM = 8.0, 31
EBN0 = 2.0
FRAMES = {"TM8192": 32768, "TM2048": 131072, "TM6144": 32768, "TM1536": 131072}
TRIPLE = dict(scale_num=13, scale_shift=4, offset=0)
T1 = dict(flooding_scale_num=13, flooding_scale_shift=4, flooding_offset=0)
T2 = dict(scale_num=13, scale_shift=4, offset=0)


def timed(calls, reps, inner):
    """ms per call of every entry in every repetition (`inner` calls each), the entries alternated"""
    ms = {k: [] for k in calls}
    for r in range(reps + 1):                           # (repetition 0: warm-up, the occupancy queries, the workspaces, the clocks)
        for key, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r:
                ms[key].append(a.elapsed_time(b) / inner)
    return ms


def summary(values, digits=3):
    return {"best": round(max(values), digits), "reps": [round(v, digits) for v in values],
            "spread": round((max(values) - min(values)) / max(values), 4)}


def frames_of(code, ebn0, frames, dev):
    rng = np.random.default_rng(1)
    pool = np.zeros((64, code.n() // 8), np.uint8)
    for i in range(64):
        code.copy_encode(rng.integers(0, 256, code.k() // 8, dtype=np.uint8), pool[i])
    sigma = float(np.sqrt(1.0 / (2.0 * (code.k() / code.n()) * 10.0 ** (ebn0 / 10.0))))
    return code.awgn_frames(torch.from_numpy(pool).to(dev), frames, sigma, seed=5, dtype="f32")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--codes", default="TM8192,TM2048,TM1536,TM6144")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed repetition")
    ap.add_argument("--frames", default="", help="CODE=N,... overrides of the default frame counts")
    args = ap.parse_args()
    frames_by_code = dict(FRAMES)
    for item in filter(None, args.frames.split(",")):
        k, v = item.split("=")
        frames_by_code[k] = int(v)
    if args.reps < 1 or args.inner < 1:
        ap.error("bad reps or inner")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)                          # (no device: the tool ends here -- there is nothing else to time)
    res = {"maxiters": MAXITERS, "reps": args.reps, "inner": args.inner, "scale": SCALE, "lim": LIM, "ebn0_db": EBN0, "triple": [13, 4, 0],
           "cascade_triples": [[13, 4, 0], [13, 4, 0]], "library_build": la.lib.labrador_ldpc_hip_build_id().decode(),
           "flooding": [], "flooding_corrected": [], "cascade": []}
    for name in args.codes.split(","):
        code = LDPCCode[name]
        frames = frames_by_code[name]
        npv = code.n() + code.punctured_bits()
        y = frames_of(code, EBN0, frames, dev)
        qbuf = torch.empty((frames, code.n()), dtype=torch.int8, device=dev)          # the two-step route's buffer of its own
        for group in ("flooding", "flooding_corrected", "cascade"):
            keys = ("soft_f32", "hard_f32") if group == "cascade" else ("soft_f32", "two_step", "hard_f32")
            triple = TRIPLE if group == "flooding_corrected" else {}
            app = {k: torch.empty((frames, npv), dtype=torch.int32 if group == "cascade" else torch.int8, device=dev) for k in keys if k != "hard_f32"}
            out = {k: torch.empty((frames, code.output_len()), dtype=torch.uint8, device=dev) for k in keys}
            it = {k: torch.empty(frames, dtype=torch.int32, device=dev) for k in keys}
            ok = {k: torch.empty(frames, dtype=torch.uint8, device=dev) for k in keys}
            stage = {k: torch.zeros(frames, dtype=torch.uint8, device=dev) for k in keys}

            def call(k):
                kw = dict(output=out[k], iters=it[k], success=ok[k])
                if group == "cascade":
                    if k == "soft_f32":
                        return lambda: code.decode_ms_cascade_bitsliced_quantised_soft_batch(y, SCALE, LIM, MAXITERS, app=app[k], stage=stage[k], **kw,
                                                                                             **T1, **T2)
                    return lambda: code.decode_ms_cascade_quantised_batch(y, "i8", SCALE, LIM, MAXITERS, stage=stage[k], bitsliced=True, **kw, **T1, **T2)
                if k == "soft_f32":
                    return lambda: code.decode_ms_bitsliced_quantised_soft_batch(y, SCALE, LIM, MAXITERS, app=app[k], **kw, **triple)
                if k == "two_step":
                    def two_step():
                        code.quantise_llrs_batch(y, "i8", SCALE, LIM, out=qbuf)
                        code.decode_ms_bitsliced_soft_batch(qbuf, MAXITERS, app=app[k], **kw, **triple)
                    return two_step
                return lambda: code.decode_ms_quantised_batch(y, "i8", SCALE, LIM, MAXITERS, bitsliced=True, **kw, **triple)
            ms = timed({k: call(k) for k in keys}, args.reps, args.inner)
            case = {"code": name, "frames": frames}
            if group != "cascade":
                case["equals_two_step"] = all(torch.equal(x["soft_f32"], x["two_step"]) for x in (app, out, it, ok))
                assert case["equals_two_step"], f"{name} {group}: the new entry and the two-step route differ"
            case["hard_results_equal_hard_f32"] = all(torch.equal(x["soft_f32"], x["hard_f32"]) for x in (out, it, ok, stage))
            assert case["hard_results_equal_hard_f32"], f"{name} {group}: the hard results differ from the hard entry's"
            for k in keys:
                case[k] = {"mcw_s": summary([frames / t / 1e3 for t in ms[k]]), "failures": int((ok[k] == 0).sum())}
            if group == "cascade":
                case["frames_at_stage_2"] = int(stage[keys[0]].sum())
            for base in keys[1:]:
                case[f"soft_f32_over_{base}"] = round(case["soft_f32"]["mcw_s"]["best"] / case[base]["mcw_s"]["best"], 4)
            res[group].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
            del app, out, it, ok, stage
        del y, qbuf
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
