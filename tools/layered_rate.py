"""The layered decoders next to each other and to the flooding kernels: rate, mean passes and failures of every decoder below on
device-resident AWGN frames (cap 25), in one process, the calls alternated inside every repetition.
    python tools/layered_rate.py [frames] [reps] [--decoders a,b,...]     -> one JSON line
Decoders (default: all):
    flooding_f32                                          labrador_ldpc_decode_ms_batch_f32
    layered_f32                                           labrador_ldpc_decode_ms_layered_batch_f32
    corrected_1_0, corrected_0.8125_0, corrected_1_0.1    labrador_ldpc_decode_ms_layered_corrected_batch_f32 at that (scale, offset): the C
                                                          symbol itself, since the Python keywords route (1, 0) to the plain entry
    flooding_f32_13_16, flooding_f32_o0.1                 labrador_ldpc_decode_ms_corrected_batch_f32 at (0.8125, 0) / (1, 0.1): the flooding
                                                          schedule with normalized / offset check messages
    flooding_i8                                           labrador_ldpc_decode_ms_batch_i8
    fixed_i8, fixed_i16                                   labrador_ldpc_decode_ms_layered_fixed_batch_i8 / _i16
    fixed_i8_16_4_0, fixed_i8_13_4_0, fixed_i8_16_4_1     labrador_ldpc_decode_ms_layered_fixed_corrected_batch_i8 at that (scale_num,
                                                          scale_shift, offset), on the i8 frames
    cascade_f32, cascade_i8, cascade_i8_13_4_0            labrador_ldpc_decode_ms_cascade_batch_f32 / _i8: flooding, then the
                                                          layered decoder (plain; i8 at (13, 4, 0)) on the frames it failed, cap 25 each
    cascade_f32_fc                                        labrador_ldpc_decode_ms_cascade_corrected_batch_f32: cascade_f32 with its first
                                                          stage at (0.8125, 0)
    cascade_i16                                           labrador_ldpc_decode_ms_cascade_batch_i16, plain second stage
    cascade_soft_f32, cascade_soft_i8, cascade_soft_i16   labrador_ldpc_decode_ms_cascade_soft_batch_* (DESIGN.md 4.15): the cascade of the type
                                                          with every frame's marginals, both stages plain
    soft_flooding_f32, soft_flooding_i8, soft_flooding_i16  labrador_ldpc_decode_ms_soft_batch_*: the first of the two soft calls a caller
                                                          composes without the soft cascade (the second runs on the failed frames only)
The f32 frames are awgn_frames(dtype="f32"); the i8 frames are the i8 channel kernel's quantisation (8 / 31) of the same job seed, and
the i16 frames are those widened.  Passes: a flooding decode that succeeds at iteration index i made i passes, a layered one at sweep
index i made i + 1; a failure counts as 25.  Cases: TC512 3 dB, TM2048 1.7 and 2 dB, TM8192 2 dB.  Default 1 048 576
frames per case (TM8192: a quarter of that) and 5 repetitions.
Per decoder: `mcw_s` (M codewords/s, the best repetition), `mcw_s_reps`, `spread` ((max - min) / max of the repetitions: what a
difference has to exceed), `mean_passes`, `failures`, `fer`.  Per case: `unit_equals_layered` (corrected (1, 0) makes exactly the sweeps
of plain layered decoding, so its ratio is the price of the added instructions and kernel arguments alone), `identity_equals_fixed` (the
same for fixed_i8_16_4_0 against fixed_i8), every decoder's rate `_over_layered_f32`, every layered decoder's over its flooding
counterpart's, and every corrected fixed decoder's `_over_fixed_i8`.  A cascade decoder also reports `stage2_share`, the share of frames its
first stage failed, counts a frame's passes as its flooding iterations plus, for those, 25 and its sweeps, and has its rate over its
flooding counterpart's and over its layered counterpart's (`CASCADE`).  The corrected flooding decoders have their rate
`_over_flooding_f32`, the plain kernel of the same run, and cascade_f32_fc also `_over_cascade_f32`.  A soft cascade has its rate over
the hard cascade of its type and over the soft flooding decoder of its type, and `hard_equals_cascade`: its output, iters, success and
stage equal the hard cascade's."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import labrador_ldpc_amd as la
from labrador_ldpc_amd import LDPCCode

MAXITERS = 25
CASES = (("TC512", 3.0), ("TM2048", 1.7), ("TM2048", 2.0), ("TM8192", 2.0))
CORRECTED = {"corrected_1_0": (1.0, 0.0), "corrected_0.8125_0": (0.8125, 0.0), "corrected_1_0.1": (1.0, 0.1)}
FIXED_CORRECTED = {"fixed_i8_16_4_0": (16, 4, 0), "fixed_i8_13_4_0": (13, 4, 0), "fixed_i8_16_4_1": (16, 4, 1)}
FLOODING_CORRECTED = {"flooding_f32_13_16": (0.8125, 0.0), "flooding_f32_o0.1": (1.0, 0.1)}
# decoder -> (its frames, its flooding counterpart; None: it is a flooding decoder)
DECODERS = {"flooding_f32": ("f32", None), **{k: ("f32", None) for k in FLOODING_CORRECTED}, "layered_f32": ("f32", "flooding_f32"), **{k: ("f32", "flooding_f32") for k in CORRECTED},
            "flooding_i8": ("i8", None), "fixed_i8": ("i8", "flooding_i8"), "fixed_i16": ("i16", "flooding_i8"),
            **{k: ("i8", "flooding_i8") for k in FIXED_CORRECTED},
            "cascade_f32": ("f32", "flooding_f32"), "cascade_f32_fc": ("f32", "flooding_f32"), "cascade_i8": ("i8", "flooding_i8"), "cascade_i8_13_4_0": ("i8", "flooding_i8"),
            "cascade_i16": ("i16", "flooding_i8"), "cascade_soft_f32": ("f32", "flooding_f32"), "cascade_soft_i8": ("i8", "flooding_i8"),
            "cascade_soft_i16": ("i16", "flooding_i8"),
            "soft_flooding_f32": ("f32", None), "soft_flooding_i8": ("i8", None), "soft_flooding_i16": ("i16", None)}
# cascade decoder -> (its layered counterpart, the fixed-point correction of its second stage)
CASCADE = {"cascade_f32": ("layered_f32", None), "cascade_f32_fc": ("layered_f32", None), "cascade_i8": ("fixed_i8", None), "cascade_i8_13_4_0": ("fixed_i8_13_4_0", (13, 4, 0)),
           "cascade_i16": ("fixed_i16", None), "cascade_soft_f32": ("layered_f32", None), "cascade_soft_i8": ("fixed_i8", None),
           "cascade_soft_i16": ("fixed_i16", None)}
# soft cascade -> (the hard cascade of its type, the soft flooding decoder of its type)
CASCADE_SOFT = {f"cascade_soft_{t}": (f"cascade_{t}", f"soft_flooding_{t}") for t in ("f32", "i8", "i16")}
SOFT_FLOODING = tuple(v[1] for v in CASCADE_SOFT.values())


def corrected_call(code, llrs, out, it, ok, scale, offset):
    """The corrected symbol itself (the Python keywords at (1, 0) call the plain one)."""
    opts = la.HipOpts(llrs.device.index, la.MEM_DEVICE, torch.cuda.current_stream(llrs.device).cuda_stream, 0, 0, None)
    st = la.lib.labrador_ldpc_decode_ms_layered_corrected_batch_f32(int(code), llrs.data_ptr(), out.data_ptr(), it.data_ptr(), ok.data_ptr(),
                                                                    llrs.shape[0], MAXITERS, scale, offset, ctypes.byref(opts))
    assert st == 0, la.last_error()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("frames", nargs="?", type=int, default=1 << 20)
    ap.add_argument("reps", nargs="?", type=int, default=5)
    ap.add_argument("--decoders", default=",".join(DECODERS), help="comma-separated, of: " + ", ".join(DECODERS))
    args = ap.parse_args()
    keys = tuple(args.decoders.split(","))
    if not keys or any(k not in DECODERS for k in keys) or len(set(keys)) != len(keys) or args.frames < 4 or args.reps < 1:
        ap.error("bad frames, reps or --decoders")
    pools = {}
    for name, _ in CASES:
        code, rng = LDPCCode[name], np.random.default_rng(1)
        pools[name] = np.zeros((64, code.n() // 8), np.uint8)
        for i in range(64):
            code.copy_encode(rng.integers(0, 256, code.k() // 8, dtype=np.uint8), pools[name][i])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)                          # (no device: the tool ends here -- there is nothing else to time)
    res = {"frames": args.frames, "maxiters": MAXITERS, "reps": args.reps, "decoders": list(keys),
           "library_build": la.lib.labrador_ldpc_hip_build_id().decode(), "cases": []}
    for name, ebn0 in CASES:
        code = LDPCCode[name]
        frames = args.frames // 4 if code == LDPCCode.TM8192 else args.frames
        sigma = float(np.sqrt(1.0 / (2.0 * (code.k() / code.n()) * 10.0 ** (ebn0 / 10.0))))
        cw = torch.from_numpy(pools[name]).to(dev)
        llrs = {}
        if any(DECODERS[k][0] == "f32" for k in keys):
            llrs["f32"] = code.awgn_frames(cw, frames, sigma, seed=5, dtype="f32")
        if any(DECODERS[k][0] != "f32" for k in keys):
            llrs["i8"] = code.awgn_frames(cw, frames, sigma, seed=5, dtype="i8", scale=8.0, lim=31)
            llrs["i16"] = llrs["i8"].to(torch.int16)
        out = {k: torch.empty((frames, code.output_len()), dtype=torch.uint8, device=dev) for k in keys}
        it = {k: torch.empty(frames, dtype=torch.int32, device=dev) for k in keys}
        ok = {k: torch.empty(frames, dtype=torch.uint8, device=dev) for k in keys}
        stage = {k: torch.empty(frames, dtype=torch.uint8, device=dev) for k in keys if k in CASCADE}
        np_len = code.n() + code.punctured_bits()
        app = {k: torch.empty((frames, np_len), dtype=torch.int32 if k in CASCADE_SOFT and k != "cascade_soft_f32" else llrs[DECODERS[k][0]].dtype,
                              device=dev) for k in keys if k in CASCADE_SOFT or k in SOFT_FLOODING}

        def call(k):
            x = llrs[DECODERS[k][0]]
            if k in CORRECTED:
                return lambda: corrected_call(code, x, out[k], it[k], ok[k], *CORRECTED[k])
            if k in FLOODING_CORRECTED:
                scale, offset = FLOODING_CORRECTED[k]
                return lambda: code.decode_ms_batch(x, MAXITERS, output=out[k], iters=it[k], success=ok[k], scale=scale, offset=offset)
            if k in FIXED_CORRECTED:
                num, shift, offset = FIXED_CORRECTED[k]
                return lambda: code.decode_ms_layered_fixed_batch(x, MAXITERS, output=out[k], iters=it[k], success=ok[k], scale_num=num,
                                                                  scale_shift=shift, offset=offset)
            if k in SOFT_FLOODING:
                return lambda: code.decode_ms_soft_batch(x, MAXITERS, app=app[k], output=out[k], iters=it[k], success=ok[k])
            if k in CASCADE_SOFT:
                method = code.decode_ms_cascade_soft_batch if k == "cascade_soft_f32" else code.decode_ms_cascade_fixed_soft_batch
                return lambda: method(x, MAXITERS, app=app[k], output=out[k], iters=it[k], success=ok[k], stage=stage[k])
            if k in CASCADE:
                if k == "cascade_f32":
                    return lambda: code.decode_ms_cascade_batch(x, MAXITERS, output=out[k], iters=it[k], success=ok[k], stage=stage[k])
                if k == "cascade_f32_fc":
                    return lambda: code.decode_ms_cascade_batch(x, MAXITERS, output=out[k], iters=it[k], success=ok[k], stage=stage[k],
                                                                flooding_scale=0.8125)
                num, shift, offset = CASCADE[k][1] or (None, None, None)
                return lambda: code.decode_ms_cascade_fixed_batch(x, MAXITERS, output=out[k], iters=it[k], success=ok[k], stage=stage[k],
                                                                  scale_num=num, scale_shift=shift, offset=offset)
            method = (code.decode_ms_batch if DECODERS[k][1] is None else
                      code.decode_ms_layered_batch if k == "layered_f32" else code.decode_ms_layered_fixed_batch)
            return lambda: method(x, MAXITERS, output=out[k], iters=it[k], success=ok[k])
        calls = {k: call(k) for k in keys}
        for fn in calls.values():                       # warm-up (and the occupancy queries)
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in keys}
        for _ in range(args.reps):
            for key, fn in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ms[key].append(a.elapsed_time(b))
        case = {"code": name, "ebn0_db": ebn0, "frames": frames}
        if "layered_f32" in keys and "corrected_1_0" in keys:
            case["unit_equals_layered"] = all(torch.equal(x["layered_f32"], x["corrected_1_0"]) for x in (out, it, ok))
        if "fixed_i8" in keys and "fixed_i8_16_4_0" in keys:
            case["identity_equals_fixed"] = all(torch.equal(x["fixed_i8"], x["fixed_i8_16_4_0"]) for x in (out, it, ok))
        for key in keys:
            succ = ok[key].to(torch.int64)
            if key in CASCADE:                          # a frame of stage 2 had MAXITERS flooding iterations before its sweeps
                second = stage[key].to(torch.int64)
                passes = torch.where(succ == 1, it[key].to(torch.int64) + second, torch.full_like(succ, MAXITERS)) + MAXITERS * second
            else:
                passes = torch.where(succ == 1, it[key].to(torch.int64) + (0 if DECODERS[key][1] is None else 1),
                                     torch.full_like(succ, MAXITERS))
            rates = [frames / t / 1e3 for t in ms[key]]
            case[key] = {"mcw_s": round(max(rates), 3), "mcw_s_reps": [round(r, 3) for r in rates],
                         "spread": round((max(rates) - min(rates)) / max(rates), 4),
                         "mean_passes": round(float(passes.double().mean()), 3), "failures": int((succ == 0).sum()),
                         "fer": float(1.0 - succ.double().mean())}
            if key in CASCADE:
                case[key]["stage2_share"] = float(stage[key].double().mean())
            if key in CASCADE_SOFT and CASCADE_SOFT[key][0] in keys:
                case[key]["hard_equals_cascade"] = all(torch.equal(x[key], x[CASCADE_SOFT[key][0]]) for x in (out, it, ok, stage))
        for key in keys:
            for base in ("layered_f32", DECODERS[key][1], "fixed_i8" if key in FIXED_CORRECTED else None, CASCADE.get(key, (None,))[0],
                         "flooding_f32" if key in FLOODING_CORRECTED else None, "cascade_f32" if key == "cascade_f32_fc" else None,
                         *CASCADE_SOFT.get(key, ())):
                if base in keys and base != key:
                    case[f"{key}_over_{base}"] = round(case[key]["mcw_s"] / case[base]["mcw_s"], 4)
        res["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
        del llrs, out, it, ok, stage, app, calls
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
