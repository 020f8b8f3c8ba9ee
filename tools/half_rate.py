"""The half-precision entries next to their f32 yardsticks, in one process, the calls alternated inside every
repetition and every repetition kept.
    python tools/half_rate.py [reps] [--host-frames N]     -> one JSON line (every case also to stderr as it finishes)
(a) `device` -- TM8192 with 32 768 frames and TM2048 with 131 072, at 2 dB, cap 25, device-resident: flooding_f16 (decode_ms_batch on
    the float16 tensor) beside flooding_f32 (decode_ms_batch on its float32 widening), and layered_f16 beside layered_f32
    (decode_ms_layered_batch at (0.8125, 0)).  The f32 entries are the yardsticks.  The pairs must agree bit for bit (`equal`).
(b) `host` -- numpy TM8192 frames (16 384 by default), given as float16 and as float32 through decode_ms_batch: wall-clock time of the
    whole call, which stages the rows across the link.
Per entry: the best repetition, `reps` (all of them) and `spread` ((max - min) / max: what a difference has to exceed).  Per pair the
half rate over the f32 rate.  No pass mark: the numbers go to DESIGN.md 4.12.  Default 5 repetitions."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode

MAXITERS = 25
CASES = (("TM8192", 2.0, 32768), ("TM2048", 2.0, 131072))
CORRECTION = dict(scale=0.8125, offset=0.0)


def timed(calls, reps, wall=False):
    """ms of every call in every repetition, the calls alternated; `wall`: host time of a synchronous call, else stream time"""
    for fn in calls.values():                           # warm-up (and the occupancy queries, the workspace, the staging memory)
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for key, fn in calls.items():
            if wall:
                t0 = time.perf_counter()
                fn()
                ms[key].append((time.perf_counter() - t0) * 1e3)
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[key].append(a.elapsed_time(b))
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
    ap.add_argument("reps", nargs="?", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=16384)
    args = ap.parse_args()
    if args.reps < 1 or args.host_frames < 1:
        ap.error("bad reps or frames")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)                          # (no device: the tool ends here -- there is nothing else to time)
    res = {"maxiters": MAXITERS, "reps": args.reps, "correction": [0.8125, 0.0],
           "library_build": la.lib.labrador_ldpc_hip_build_id().decode(), "device": [], "host": None}

    # (a) device-resident: the half entries beside the f32 entries on the widened frames
    for name, ebn0, frames in CASES:
        code = LDPCCode[name]
        h = frames_of(code, ebn0, frames, dev).to(torch.float16)
        w = code.widen_llrs_batch(h)
        keys = ("flooding_f16", "flooding_f32", "layered_f16", "layered_f32")
        out = {k: torch.empty((frames, code.output_len()), dtype=torch.uint8, device=dev) for k in keys}
        it = {k: torch.empty(frames, dtype=torch.int32, device=dev) for k in keys}
        ok = {k: torch.empty(frames, dtype=torch.uint8, device=dev) for k in keys}

        def call(k):
            x = h if k.endswith("f16") else w
            kw = dict(output=out[k], iters=it[k], success=ok[k])
            if k.startswith("flooding"):
                return lambda: code.decode_ms_batch(x, MAXITERS, **kw)
            return lambda: code.decode_ms_layered_batch(x, MAXITERS, **kw, **CORRECTION)
        ms = timed({k: call(k) for k in keys}, args.reps)
        case = {"code": name, "ebn0_db": ebn0, "frames": frames,
                "equal": all(torch.equal(x[f"{s}_f16"], x[f"{s}_f32"]) for s in ("flooding", "layered") for x in (out, it, ok))}
        for k in keys:
            case[k] = {"mcw_s": summary([frames / t / 1e3 for t in ms[k]]), "failures": int((ok[k] == 0).sum())}
        for s in ("flooding", "layered"):
            case[f"{s}_f16_over_f32"] = round(case[f"{s}_f16"]["mcw_s"]["best"] / case[f"{s}_f32"]["mcw_s"]["best"], 4)
        res["device"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
        del h, w, out, it, ok
        torch.cuda.empty_cache()

    # (b) host rows: the same frames as float16 and as float32 through the staged call
    code = LDPCCode.TM8192
    frames = args.host_frames
    y16 = frames_of(code, 2.0, frames, dev).to(torch.float16).cpu().numpy()
    y32 = y16.astype(np.float32)
    keys = ("host_f16", "host_f32")
    out = {k: np.empty((frames, code.output_len()), np.uint8) for k in keys}
    it = {k: np.empty(frames, np.uint32) for k in keys}
    ok = {k: np.empty(frames, np.uint8) for k in keys}
    calls = {k: (lambda k=k, x=x: code.decode_ms_batch(x, MAXITERS, output=out[k], iters=it[k], success=ok[k]))
             for k, x in (("host_f16", y16), ("host_f32", y32))}
    ms = timed(calls, args.reps, wall=True)
    case = {"code": "TM8192", "ebn0_db": 2.0, "frames": frames,
            "equal": all(np.array_equal(x["host_f16"], x["host_f32"]) for x in (out, it, ok))}
    for k in keys:
        case[k] = {"mcw_s": summary([frames / t / 1e3 for t in ms[k]]), "failures": int((ok[k] == 0).sum())}
    case["host_f16_over_f32"] = round(case["host_f16"]["mcw_s"]["best"] / case["host_f32"]["mcw_s"]["best"], 4)
    res["host"] = case
    print(json.dumps(case), file=sys.stderr, flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
