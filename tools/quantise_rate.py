"""The quantiser and the fused quantise-and-decode next to their yardsticks, on device-resident frames, in one process,
the calls alternated inside every repetition and every repetition kept.
    python tools/quantise_rate.py [frames] [reps]     -> one JSON line (every case also to stderr as it finishes)
(a) `stream` -- on one buffer of f32 AWGN frames (TM8192, 2 dB): quantise_i8 and quantise_i16 (labrador_ldpc_quantise_llrs_batch_*)
    beside llrs_to_hard_f32 (labrador_ldpc_llrs_to_hard_batch_f32), the streaming kernel of the same shape that reads the same bytes.
    GB/s counts the bytes a call reads and writes: 4 + 1, 4 + 2 and 4 + 1/8 per LLR.
(b) `decode` -- TM8192 at 2 dB and TM2048 at 2 dB, cap 25: fused_i8 (labrador_ldpc_decode_ms_quantised_batch_i8 at 8 / 31 on the f32
    frames), flooding_i8 (labrador_ldpc_decode_ms_batch_i8 on those frames quantised beforehand by the library) and flooding_f32
    (labrador_ldpc_decode_ms_batch_f32 on the f32 frames).  fused_i8 and flooding_i8 must agree bit for bit (`fused_equals_two_calls`).
Per entry: the best repetition, `reps` (all of them) and `spread` ((max - min) / max: what a difference has to exceed).  Per decode case
the fused rate over each yardstick.  No pass mark: the numbers go to DESIGN.md 4.10.  Default 262 144 frames (TM8192: a quarter of
that for the decoders) and 5 repetitions.
    python tools/quantise_rate.py --layered [reps]    -> one JSON line: the f32-input layered and cascade entries
TM8192 with 32 768 frames and TM2048 with 131 072, at 2 dB, cap 25, i8 at 8 / 31 and (13, 4, 0), the calls alternated as above:
(c) `layered` -- layered_fused (labrador_ldpc_decode_ms_layered_quantised_batch_i8 on the f32 frames) beside layered_two_calls
    (labrador_ldpc_quantise_llrs_batch_i8 into a caller's buffer, then labrador_ldpc_decode_ms_layered_fixed_corrected_batch_i8) and
    layered_prequantised (the latter alone, on frames quantised beforehand).
(d) `cascade` -- cascade_fused (labrador_ldpc_decode_ms_cascade_quantised_batch_i8) beside cascade_two_calls (the quantiser, then
    labrador_ldpc_decode_ms_cascade_batch_i8) and flooding_fused (labrador_ldpc_decode_ms_quantised_batch_i8: flooding alone).
The fused results must equal the two calls' bit for bit (`fused_equals_two_calls`)."""
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
CASES = (("TM8192", 2.0), ("TM2048", 2.0))


def timed(calls, reps):
    """ms of every call in every repetition, the calls alternated"""
    for fn in calls.values():                           # warm-up (and the occupancy queries, and the workspace)
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for key, fn in calls.items():
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


LAYERED_CASES = (("TM8192", 2.0, 32768), ("TM2048", 2.0, 131072))
TRIPLE = dict(scale_num=13, scale_shift=4, offset=0)


def layered_main(reps, dev):
    """(c) and (d): the f32-input layered and cascade entries beside the two calls they compose and their yardsticks"""
    res = {"maxiters": MAXITERS, "reps": reps, "scale": SCALE, "lim": LIM, "triple": [13, 4, 0],
           "library_build": la.lib.labrador_ldpc_hip_build_id().decode(), "layered": [], "cascade": []}
    for name, ebn0, frames in LAYERED_CASES:
        code = LDPCCode[name]
        y = frames_of(code, ebn0, frames, dev)
        q = code.quantise_llrs_batch(y, "i8", SCALE, LIM)
        q2 = torch.empty_like(q)
        groups = {"layered": ("layered_fused", "layered_two_calls", "layered_prequantised"),
                  "cascade": ("cascade_fused", "cascade_two_calls", "flooding_fused")}
        for group, keys in groups.items():
            out = {k: torch.empty((frames, code.output_len()), dtype=torch.uint8, device=dev) for k in keys}
            it = {k: torch.empty(frames, dtype=torch.int32, device=dev) for k in keys}
            ok = {k: torch.empty(frames, dtype=torch.uint8, device=dev) for k in keys}
            stage = {k: torch.zeros(frames, dtype=torch.uint8, device=dev) for k in keys}

            def call(k):
                kw = dict(output=out[k], iters=it[k], success=ok[k])
                if k == "layered_fused":
                    return lambda: code.decode_ms_layered_quantised_batch(y, "i8", SCALE, LIM, MAXITERS, **kw, **TRIPLE)
                if k == "layered_two_calls":
                    return lambda: code.decode_ms_layered_fixed_batch(code.quantise_llrs_batch(y, "i8", SCALE, LIM, out=q2), MAXITERS, **kw, **TRIPLE)
                if k == "layered_prequantised":
                    return lambda: code.decode_ms_layered_fixed_batch(q, MAXITERS, **kw, **TRIPLE)
                if k == "cascade_fused":
                    return lambda: code.decode_ms_cascade_quantised_batch(y, "i8", SCALE, LIM, MAXITERS, stage=stage[k], **kw, **TRIPLE)
                if k == "cascade_two_calls":
                    return lambda: code.decode_ms_cascade_fixed_batch(code.quantise_llrs_batch(y, "i8", SCALE, LIM, out=q2), MAXITERS,
                                                                      stage=stage[k], **kw, **TRIPLE)
                return lambda: code.decode_ms_quantised_batch(y, "i8", SCALE, LIM, MAXITERS, **kw)
            ms = timed({k: call(k) for k in keys}, reps)
            case = {"code": name, "ebn0_db": ebn0, "frames": frames,
                    "fused_equals_two_calls": all(torch.equal(x[keys[0]], x[keys[1]]) for x in (out, it, ok, stage))}
            for k in keys:
                case[k] = {"mcw_s": summary([frames / t / 1e3 for t in ms[k]]), "failures": int((ok[k] == 0).sum())}
            if group == "cascade":
                case["frames_at_stage_2"] = int(stage[keys[0]].sum())
            for base in keys[1:]:
                case[f"{keys[0]}_over_{base}"] = round(case[keys[0]]["mcw_s"]["best"] / case[base]["mcw_s"]["best"], 4)
            res[group].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
            del out, it, ok, stage
        del y, q, q2
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("frames", nargs="?", type=int, default=None)
    ap.add_argument("reps", nargs="?", type=int, default=5)
    ap.add_argument("--layered", action="store_true", help="the f32-input layered and cascade entries instead (one argument: reps)")
    args = ap.parse_args()
    if args.layered:
        reps = args.frames if args.frames is not None else 5       # (the only positional argument of this mode)
        if reps < 1:
            ap.error("bad reps")
        torch.cuda.set_device(torch.device("cuda", 0))
        return layered_main(reps, torch.device("cuda", 0))
    if args.frames is None:
        args.frames = 1 << 18
    if args.frames < 4 or args.reps < 1:
        ap.error("bad frames or reps")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)                          # (no device: the tool ends here -- there is nothing else to time)
    res = {"frames": args.frames, "maxiters": MAXITERS, "reps": args.reps, "scale": SCALE, "lim": LIM,
           "library_build": la.lib.labrador_ldpc_hip_build_id().decode(), "stream": None, "decode": []}

    # (a) the quantiser as a streaming kernel
    code = LDPCCode.TM8192
    y = frames_of(code, 2.0, args.frames, dev)
    count = y.numel()
    q8, q16 = torch.empty(y.shape, dtype=torch.int8, device=dev), torch.empty(y.shape, dtype=torch.int16, device=dev)
    bits = torch.empty((args.frames, code.n() // 8), dtype=torch.uint8, device=dev)
    calls = {"quantise_i8": lambda: code.quantise_llrs_batch(y, "i8", SCALE, LIM, out=q8),
             "quantise_i16": lambda: code.quantise_llrs_batch(y, "i16", 64.0, 2047, out=q16),
             "llrs_to_hard_f32": lambda: code.llrs_to_hard_batch(y, output=bits)}
    nbytes = {"quantise_i8": 5.0 * count, "quantise_i16": 6.0 * count, "llrs_to_hard_f32": 4.125 * count}
    ms = timed(calls, args.reps)
    stream = {"code": "TM8192", "frames": args.frames, "f32_bytes": 4 * count}
    for k in calls:
        stream[k] = {"gb_s": summary([nbytes[k] / t / 1e6 for t in ms[k]], 1), "us": [round(t * 1e3, 1) for t in ms[k]]}
    for k in ("quantise_i8", "quantise_i16"):            # time against the yardstick's, best against best
        stream[f"{k}_time_over_llrs_to_hard_f32"] = round(min(ms[k]) / min(ms["llrs_to_hard_f32"]), 4)
    res["stream"] = stream
    print(json.dumps(stream), file=sys.stderr, flush=True)
    del y, q8, q16, bits, calls
    torch.cuda.empty_cache()

    # (b) the fused decode beside the decode of frames quantised beforehand and the f32 decode
    for name, ebn0 in CASES:
        code = LDPCCode[name]
        frames = args.frames // 4 if code == LDPCCode.TM8192 else args.frames
        y = frames_of(code, ebn0, frames, dev)
        q = code.quantise_llrs_batch(y, "i8", SCALE, LIM)
        keys = ("fused_i8", "flooding_i8", "flooding_f32")
        out = {k: torch.empty((frames, code.output_len()), dtype=torch.uint8, device=dev) for k in keys}
        it = {k: torch.empty(frames, dtype=torch.int32, device=dev) for k in keys}
        ok = {k: torch.empty(frames, dtype=torch.uint8, device=dev) for k in keys}

        def call(k):
            if k == "fused_i8":
                return lambda: code.decode_ms_quantised_batch(y, "i8", SCALE, LIM, MAXITERS, output=out[k], iters=it[k], success=ok[k])
            x = q if k == "flooding_i8" else y
            return lambda: code.decode_ms_batch(x, MAXITERS, output=out[k], iters=it[k], success=ok[k])
        ms = timed({k: call(k) for k in keys}, args.reps)
        case = {"code": name, "ebn0_db": ebn0, "frames": frames,
                "fused_equals_two_calls": all(torch.equal(x["fused_i8"], x["flooding_i8"]) for x in (out, it, ok))}
        for k in keys:
            case[k] = {"mcw_s": summary([frames / t / 1e3 for t in ms[k]]), "failures": int((ok[k] == 0).sum())}
        for base in ("flooding_i8", "flooding_f32"):
            case[f"fused_i8_over_{base}"] = round(case["fused_i8"]["mcw_s"]["best"] / case[base]["mcw_s"]["best"], 4)
        res["decode"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
        del y, q, out, it, ok
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
