"""Packed hard decisions through the bit-sliced i8 kernels' own loader next to the two-step route it replaces and the pre-expanded
ceiling, in one process, the calls alternated inside every repetition and every repetition kept.
    python tools/bs_hard_rate.py [--codes TM8192,TM2048,TM1536,TM6144] [--reps 5] [--inner 20] [--host-inner 3] [--frames CODE=N,...]
                                                             -> one JSON line (every case also to stderr as it finishes)
A repetition times `inner` calls back to back -- device buffers between two events (one call is a few milliseconds: too short a window
to measure), host buffers, whose calls are synchronous, on the host's clock -- and every entry runs one untimed repetition first.
Per code, awgn_frames at 2 dB reduced to their signs (llrs_to_hard_batch), cap 25, magnitude 1, no mask:
(a) `device` -- packed (labrador_ldpc_decode_ms_bitsliced_hard_batch_i8 on the packed frames), two_step
    (labrador_ldpc_hard_to_llrs_batch_i8 into a preallocated buffer, then labrador_ldpc_decode_ms_batch_i8: the route the entry replaces)
    and expanded (labrador_ldpc_decode_ms_batch_i8 on rows expanded beforehand: the ceiling).
(b) `host` -- packed and two_step again with numpy buffers: n / 8 bytes per frame cross the link, against n.
`equals_two_step`: the new entry's results equal the two-step route's bit for bit.  Per entry: the best repetition, `reps` (all of
them) and `spread` ((max - min) / max: what a difference has to exceed).
(c) `harness` -- labrador_ldpc_amd.perftest on TM2048 hard input at magnitude 16, plain against (13, 4, 0), on the same frames: trials,
    bit errors and frame errors per Eb/N0.
No pass mark: the numbers go to DESIGN.md 4.21.  Default frames: TM8192 32 768, TM2048 131 072, TM6144 32 768, TM1536 131 072."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode, perftest

MAXITERS = 25
MAGNITUDE = 1
EBN0 = 2.0
FRAMES = {"TM8192": 32768, "TM2048": 131072, "TM6144": 32768, "TM1536": 131072}
HARNESS = dict(code="TM2048", magnitude=16, triple=(13, 4, 0), ebn0_db=(3.0, 3.5, 4.0), frames=131072)


def timed(calls, reps, inner, events):
    """ms per call of every entry in every repetition (`inner` calls each), the entries alternated"""
    ms = {k: [] for k in calls}
    for r in range(reps + 1):                           # (repetition 0: warm-up, the occupancy queries, the staging buffers, the clocks)
        for key, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if r:
                ms[key].append((a.elapsed_time(b) if events else (t1 - t0) * 1e3) / inner)
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
    return code.llrs_to_hard_batch(code.awgn_frames(torch.from_numpy(pool).to(dev), frames, sigma, seed=5, dtype="f32"))


def case_of(name, frames, where, keys, calls, results, reps, inner):
    ms = timed(calls, reps, inner, events=where == "device")
    case = {"code": name, "frames": frames}
    for other in keys[1:]:
        case[f"equals_{other}"] = all(bool((np.asarray(a.cpu() if hasattr(a, "cpu") else a) == np.asarray(b.cpu() if hasattr(b, "cpu") else b)).all())
                                      for a, b in zip(results[keys[0]], results[other]))
    for k in keys:
        ok = results[k][2]
        case[k] = {"mcw_s": summary([frames / t / 1e3 for t in ms[k]]), "failures": int((ok == 0).sum())}
    for base in keys[1:]:
        case[f"packed_over_{base}"] = round(case[keys[0]]["mcw_s"]["best"] / case[base]["mcw_s"]["best"], 4)
    print(json.dumps({where: case}), file=sys.stderr, flush=True)
    return case


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--codes", default="TM8192,TM2048,TM1536,TM6144")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed repetition, device buffers")
    ap.add_argument("--host-inner", type=int, default=3, help="calls per timed repetition, host buffers")
    ap.add_argument("--frames", default="", help="CODE=N,... overrides of the default frame counts")
    ap.add_argument("--no-harness", action="store_true", help="leave the perftest pair out")
    args = ap.parse_args()
    frames_by_code = dict(FRAMES)
    for item in filter(None, args.frames.split(",")):
        k, v = item.split("=")
        frames_by_code[k] = int(v)
    if args.reps < 1 or args.inner < 1 or args.host_inner < 1:
        ap.error("bad reps or inner")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)                          # (no device: the tool ends here -- there is nothing else to time)
    res = {"maxiters": MAXITERS, "reps": args.reps, "inner": args.inner, "host_inner": args.host_inner, "magnitude": MAGNITUDE, "ebn0_db": EBN0,
           "library_build": la.lib.labrador_ldpc_hip_build_id().decode(), "device": [], "host": [], "harness": []}
    for name in args.codes.split(","):
        code = LDPCCode[name]
        frames = frames_by_code[name]
        x = frames_of(code, EBN0, frames, dev)
        # device buffers
        keys = ("packed", "two_step", "expanded")
        r = {k: (torch.empty((frames, code.output_len()), dtype=torch.uint8, device=dev), torch.empty(frames, dtype=torch.int32, device=dev),
                 torch.empty(frames, dtype=torch.uint8, device=dev)) for k in keys}
        kw = {k: dict(output=r[k][0], iters=r[k][1], success=r[k][2]) for k in keys}
        e = code.hard_to_llrs_batch(x, "i8")
        work = torch.empty_like(e)

        def two_step():
            code.hard_to_llrs_batch(x, "i8", llrs=work)
            code.decode_ms_batch(work, MAXITERS, **kw["two_step"])
        calls = {"packed": lambda: code.decode_ms_hard_batch(x, MAXITERS, MAGNITUDE, **kw["packed"]), "two_step": two_step,
                 "expanded": lambda: code.decode_ms_batch(e, MAXITERS, **kw["expanded"])}
        res["device"].append(case_of(name, frames, "device", keys, calls, r, args.reps, args.inner))
        del r, kw, e, work
        # host buffers
        keys = ("packed", "two_step")
        hx = x.cpu().numpy()
        r = {k: (np.empty((frames, code.output_len()), np.uint8), np.empty(frames, np.uint32), np.empty(frames, np.uint8)) for k in keys}
        kw = {k: dict(output=r[k][0], iters=r[k][1], success=r[k][2]) for k in keys}
        hwork = np.empty((frames, code.n()), np.int8)

        def host_two_step():
            code.hard_to_llrs_batch(hx, "i8", llrs=hwork)
            code.decode_ms_batch(hwork, MAXITERS, **kw["two_step"])
        calls = {"packed": lambda: code.decode_ms_hard_batch(hx, MAXITERS, MAGNITUDE, **kw["packed"]), "two_step": host_two_step}
        res["host"].append(case_of(name, frames, "host", keys, calls, r, args.reps, args.host_inner))
        del r, kw, hwork, hx, x
        torch.cuda.empty_cache()
    if not args.no_harness:
        code = LDPCCode[HARNESS["code"]]
        t = HARNESS["triple"]
        for ebn0 in HARNESS["ebn0_db"]:
            point = {"code": code.name, "ebn0_db": ebn0, "magnitude": HARNESS["magnitude"], "maxiters": MAXITERS}
            for key, kw in (("plain", {}), ("corrected_13_4_0", dict(flooding_scale_num=t[0], flooding_scale_shift=t[1], flooding_fixed_offset=t[2]))):
                trials, bits, errors, _, fe = perftest.ms_trials(code, ebn0, "ebn0", MAXITERS, HARNESS["frames"], max_bits=0, max_errors=10 ** 12,
                                                                 seed=1, llr="hard", hard_magnitude=HARNESS["magnitude"], **kw)
                point[key] = {"trials": trials, "bit_errors": errors, "frame_errors": fe}
            res["harness"].append(point)
            print(json.dumps({"harness": point}), file=sys.stderr, flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
