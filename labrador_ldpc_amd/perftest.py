"""BER Monte-Carlo of the min-sum decoder -- the GPU counterpart of the reference's perftest binary.

Reference: perftest/src/main.rs.  There every rayon worker loops `ms_trial` (:9-29): random bytes ->
encode -> hard_to_llrs (+-1) -> add Normal(0, sigma) noise -> decode_ms (100 iterations) -> count bit
errors in the first k bits, until trials*k > 5e7 or errors > 5000 (:50); one CSV line per SNR (:62):
    code,snr,trials,bits,errors,ber
Here a trial batch runs entirely on the device: labrador_ldpc_encode_batch -> labrador_ldpc_hip_awgn_f32
-> labrador_ldpc_decode_ms_batch_f32, errors counted with torch bit ops (plumbing).  `--schedule layered` decodes with
labrador_ldpc_decode_ms_layered_batch_f32 instead (block-row layered schedule), so both FER curves can be drawn
from the same frames; the default, flooding, is the reference's decoder and keeps the output unchanged.  `--scale` / `--offset`
(layered schedule only) decode with normalized / offset check messages (labrador_ldpc_decode_ms_layered_corrected_batch_f32,
DESIGN.md 4.6); `--offset` is in the units of the LLRs, which here are +-1 + noise.  `--llr i8` / `--llr i16` (layered schedule only)
quantise the frames on the device -- labrador_ldpc_hip_awgn_i8's clamp(rint(`--llr-scale` * y), +-`--llr-lim`), widened for i16 --
and decode them with the fixed-point layered decoder (labrador_ldpc_decode_ms_layered_fixed_batch_i8 / _i16); f32 is
the default and leaves everything else as it was.  `--fixed-scale NUM/DEN` / `--fixed-offset INT` (with `--llr i8` / `i16` only) decode
those frames with normalized / offset check messages in integers (labrador_ldpc_decode_ms_layered_fixed_corrected_batch_i8 / _i16,
DESIGN.md 4.8): DEN is a power of two of at most 256, and the offset is in units of the quantiser.  `--schedule cascade` decodes with the two-stage
entries (labrador_ldpc_decode_ms_cascade_batch_f32 / _i8 / _i16): the flooding decoder at `--maxiters`, then the layered
decoder of the LLR type at `--max-sweeps` (default: `--maxiters`) on the frames it failed, with the layered schedule's options.  `--from-f32` (with `--llr i8` / `i16`
and `--schedule layered` / `cascade`) generates the f32 frames of the f32 branch instead and decodes them through the f32-input entries
(labrador_ldpc_decode_ms_layered_quantised_batch_* / _cascade_quantised_batch_*), which quantise at `--llr-scale` /
`--llr-lim` themselves; without the flag nothing changes.  `--llr f16` / `--llr bf16` (any schedule, with the f32 branch's options)
round the f32 frames of the f32 branch to the format on the device and decode them through the half-precision entries
(labrador_ldpc_decode_ms_batch_f16 / _bf16 and their layered and cascade neighbours): what keeping LLRs in two
bytes costs in BER.  `--flooding-scale` / `--flooding-offset` (`--schedule flooding` or `cascade`, `--llr f32` only) give the flooding
decoder -- the whole decode, or the cascade's first stage -- normalized / offset check messages
(labrador_ldpc_decode_ms_corrected_batch_f32 / labrador_ldpc_decode_ms_cascade_corrected_batch_f32); the offset is in
the units of the LLRs, as `--offset`; anywhere else they are a ValueError, and the defaults change nothing.
`--fixed-flooding-scale NUM/DEN` / `--fixed-flooding-offset INT` (`--llr i8` with `--schedule flooding` or `cascade`, `--from-f32`
included on the cascade) give the i8 flooding decoder -- the whole decode, which without them has no i8 form here, or the cascade's
first stage -- normalized / offset check messages in integers (labrador_ldpc_decode_ms_corrected_batch_i8 /
labrador_ldpc_decode_ms_cascade_corrected_batch_i8 / _cascade_quantised_corrected_batch_i8, DESIGN.md 4.14: the bit-sliced kernels of
the TM codes); NUM/DEN and the offset as `--fixed-scale` / `--fixed-offset`; anywhere else they are a ValueError.
`--bitsliced-loader` (with `--from-f32 --llr i8` and `--schedule flooding` or `cascade`) decodes the f32 frames through the bit-sliced
kernels' own loader (labrador_ldpc_decode_ms_bitsliced_quantised_batch_i8 / _corrected_batch_i8 /
labrador_ldpc_decode_ms_cascade_bitsliced_quantised_batch_i8, DESIGN.md 4.19: TM1536, TM2048, TM6144, TM8192); on the flooding schedule
it is the only `--from-f32` decode, with or without `--fixed-flooding-scale` / `--fixed-flooding-offset`.
`--llr hard` (`--schedule flooding` only) reduces the f32 frames of the f32 branch to their signs on the device
(labrador_ldpc_llrs_to_hard_batch_f32) and decodes the packed bits at `--hard-magnitude M` (1 .. 127, default 1) through the bit-sliced
kernels' packed loader (labrador_ldpc_decode_ms_bitsliced_hard_batch_i8 / _corrected_batch_i8, DESIGN.md 4.21: TM1536, TM2048, TM6144,
TM8192), with or without `--fixed-flooding-scale` / `--fixed-flooding-offset`: what a hard-decision receiver gets from min-sum.

Noise conventions:
  --noise perftest  sigma = 10^(-snr_db/10), what the reference calls "snr" (perftest/src/main.rs:15)
  --noise ebn0      sigma^2 = 1 / (2 R 10^(EbN0/10)), R = k/n (textbook Eb/N0; what bench.py uses)

    python -m labrador_ldpc_amd.perftest --code TC512 --noise perftest
"""
from __future__ import annotations

import argparse
import sys

import numpy as np


FLOAT_LLRS = ("f32", "f16", "bf16")                                          # the f32 decoders' inputs; the others are quantised


def sigma_for(code, snr_db: float, noise: str) -> float:
    if noise == "perftest":
        return float(1.0 / 10.0 ** (snr_db / 10.0))
    return float(np.sqrt(1.0 / (2.0 * (code.k() / code.n()) * 10.0 ** (snr_db / 10.0))))


def ms_trials(code, snr_db: float, noise: str = "perftest", maxiters: int = 100, batch: int = 65536,
              max_bits: float = 5e7, max_errors: int = 5000, seed: int = 1, device: int = 0, schedule: str = "flooding",
              scale: float = 1.0, offset: float = 0.0, llr: str = "f32", llr_scale: float = 8.0, llr_lim: int = 31,
              scale_num=None, scale_shift=None, fixed_offset=None, max_sweeps=None, from_f32: bool = False,
              flooding_scale: float = 1.0, flooding_offset: float = 0.0, flooding_scale_num=None, flooding_scale_shift=None,
              flooding_fixed_offset=None, bitsliced_loader: bool = False, hard_magnitude: int = 1):
    """One SNR point.  Returns (trials, bits, errors, ber, frame_errors).  `schedule`: "flooding" (decode_ms_batch, the
    reference's decoder) or "layered" (decode_ms_layered_batch).  `scale`, `offset`: the layered schedule's normalized / offset
    min-sum correction (the defaults are plain min-sum); the flooding decoder has none.  `llr`: "f32", or "i8" / "i16" for the
    fixed-point layered decoder on frames quantised as clamp(rint(llr_scale * y), +-llr_lim) (layered schedule, no float correction).
    `scale_num`, `scale_shift`, `fixed_offset`: the fixed-point decoder's integer correction (decode_ms_layered_fixed_batch's
    scale_num, scale_shift and offset; quantised LLRs only; None, the default, is plain min-sum).  `schedule` "cascade"
    (decode_ms_cascade_batch / decode_ms_cascade_fixed_batch): flooding at `maxiters`, then the layered decoder of `llr` with the
    layered schedule's options at `max_sweeps` (None: `maxiters`) on the frames flooding failed.  `from_f32` (quantised LLRs,
    layered or cascade): the frames are the f32 frames of the f32 branch, decoded through decode_ms_layered_quantised_batch /
    decode_ms_cascade_quantised_batch at (`llr_scale`, `llr_lim`).  `llr` "f16" / "bf16": the f32 branch with its frames rounded
    to the format (to nearest, ties to even) and handed to the same methods as half-precision tensors.  `flooding_scale`,
    `flooding_offset`: the FLOODING decoder's normalized / offset min-sum correction (decode_ms_batch's `scale` and `offset`; the
    flooding schedule and the cascade's first stage, f32 LLRs only; the defaults are plain min-sum).  `flooding_scale_num`,
    `flooding_scale_shift`, `flooding_fixed_offset`: the i8 flooding decoder's integer correction (decode_ms_corrected_fixed_batch's
    triple; `llr` "i8" on the flooding schedule -- the only i8 flooding decode here -- and as the cascade's first stage, `from_f32`
    included there; None, the default, is none).  `bitsliced_loader` (`from_f32`, `llr` "i8", flooding or cascade): the f32 frames go
    through decode_ms_quantised_batch / decode_ms_cascade_quantised_batch with bitsliced=True -- on the flooding schedule with the
    flooding triple, if one is given.  `llr` "hard" (flooding schedule only): the f32 frames reduced to their signs by
    llrs_to_hard_batch and decoded by decode_ms_hard_batch at `hard_magnitude`, with the flooding triple, if one is given; nothing else
    goes with it."""
    if llr == "hard" and (schedule != "flooding" or from_f32 or bitsliced_loader or max_sweeps is not None or scale != 1.0 or offset != 0.0
                          or flooding_scale != 1.0 or flooding_offset != 0.0
                          or not (scale_num is None and scale_shift is None and fixed_offset is None)):
        raise ValueError("hard LLRs belong to the flooding schedule, with hard_magnitude and the i8 flooding triple alone")
    if llr != "hard" and hard_magnitude != 1:
        raise ValueError("hard_magnitude belongs to hard LLRs")
    if bitsliced_loader and not (from_f32 and llr == "i8" and schedule in ("flooding", "cascade")):
        raise ValueError("bitsliced_loader belongs to from_f32 with i8 LLRs on the flooding schedule and the cascade")
    fixed_flooding = not (flooding_scale_num is None and flooding_scale_shift is None and flooding_fixed_offset is None)
    if fixed_flooding and llr != "hard" and (llr != "i8" or schedule == "layered" or (from_f32 and schedule != "cascade" and not bitsliced_loader)):
        raise ValueError("flooding_scale_num, flooding_scale_shift and flooding_fixed_offset belong to i8 LLRs on the flooding schedule "
                         "and the cascade")
    if fixed_flooding and schedule == "flooding" and not (scale_num is None and scale_shift is None and fixed_offset is None):
        raise ValueError("scale_num, scale_shift and fixed_offset belong to the layered schedule and the cascade's second stage")
    if schedule not in ("flooding", "layered", "cascade"):
        raise ValueError(f"unknown schedule {schedule!r}")
    if schedule == "flooding" and (scale != 1.0 or offset != 0.0):
        raise ValueError("scale and offset belong to the layered schedule")
    if schedule != "cascade" and max_sweeps is not None:
        raise ValueError("max_sweeps belongs to the cascade")
    if llr not in FLOAT_LLRS + ("i8", "i16", "hard"):
        raise ValueError(f"unknown LLR type {llr!r}")
    if llr not in FLOAT_LLRS + ("hard",) and ((schedule == "flooding" and not fixed_flooding and not bitsliced_loader) or scale != 1.0
                                               or offset != 0.0):
        raise ValueError("quantised LLRs belong to the layered schedule without scale and offset")
    if llr in FLOAT_LLRS and not (scale_num is None and scale_shift is None and fixed_offset is None):
        raise ValueError("scale_num, scale_shift and fixed_offset belong to the quantised LLRs of the layered schedule")
    if from_f32 and (llr in FLOAT_LLRS or (schedule == "flooding" and not bitsliced_loader)):
        raise ValueError("from_f32 belongs to the quantised LLRs of the layered schedule and the cascade")
    if (flooding_scale != 1.0 or flooding_offset != 0.0) and (schedule == "layered" or llr != "f32"):
        raise ValueError("flooding_scale and flooding_offset belong to the flooding schedule and the cascade on f32 LLRs")
    import torch
    from . import _fixed_correction
    flooding_kw = {}
    if fixed_flooding:
        flooding_kw = dict(zip(("flooding_scale_num", "flooding_scale_shift", "flooding_offset"),
                               _fixed_correction(flooding_scale_num, flooding_scale_shift, flooding_fixed_offset)))
    dev = torch.device("cuda", device)
    k8 = code.k() // 8
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    sigma = sigma_for(code, snr_db, noise)
    popcnt = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int64, device=dev)
    trials = errors = frame_errors = 0
    rounds = 0
    while trials * code.k() <= max_bits and errors <= max_errors:
        data = torch.randint(0, 256, (batch, k8), dtype=torch.uint8, device=dev, generator=g)
        cw = code.encode_batch(data)                                         # perftest/src/main.rs:10-12
        if from_f32:                                                         # the f32 branch's frames, quantised by the decoder's loader
            llrs = code.awgn_frames(cw, batch, sigma, seed=(seed << 20) + rounds)
            if schedule == "flooding":                                       # (the bit-sliced loader: checked above)
                triple = dict(zip(("scale_num", "scale_shift", "offset"), flooding_kw.values()))
                out = code.decode_ms_quantised_batch(llrs, llr, llr_scale, llr_lim, maxiters, bitsliced=True, **triple)[0]
            else:
                decode = code.decode_ms_cascade_quantised_batch if schedule == "cascade" else code.decode_ms_layered_quantised_batch
                out = decode(llrs, llr, llr_scale, llr_lim, maxiters, scale_num=scale_num, scale_shift=scale_shift, offset=fixed_offset,
                             **({"max_sweeps": max_sweeps, **flooding_kw, **({"bitsliced": True} if bitsliced_loader else {})}
                                if schedule == "cascade" else {}))[0]
        elif llr == "hard":                                                  # the f32 branch's frames, reduced to their signs
            hard = code.llrs_to_hard_batch(code.awgn_frames(cw, batch, sigma, seed=(seed << 20) + rounds))
            triple = dict(zip(("scale_num", "scale_shift", "offset"), flooding_kw.values()))
            out = code.decode_ms_hard_batch(hard, maxiters, hard_magnitude, **triple)[0]
        elif llr not in FLOAT_LLRS:                                          # the same noise, quantised by the i8 channel kernel
            llrs = code.awgn_frames(cw, batch, sigma, seed=(seed << 20) + rounds, dtype="i8", scale=llr_scale, lim=llr_lim)
            if schedule == "flooding":                                       # (i8 with a flooding triple: checked above)
                out = code.decode_ms_corrected_fixed_batch(llrs, *flooding_kw.values(), maxiters=maxiters)[0]
            else:
                decode = code.decode_ms_cascade_fixed_batch if schedule == "cascade" else code.decode_ms_layered_fixed_batch
                out = decode(llrs if llr == "i8" else llrs.to(torch.int16), maxiters, scale_num=scale_num, scale_shift=scale_shift,
                             offset=fixed_offset, **({"max_sweeps": max_sweeps, **flooding_kw} if schedule == "cascade" else {}))[0]
        else:
            llrs = code.awgn_frames(cw, batch, sigma, seed=(seed << 20) + rounds)  # :13-18 (frame f <- codeword f)
            if llr != "f32":                                                 # the same frames as the format keeps them
                llrs = llrs.to(torch.float16 if llr == "f16" else torch.bfloat16)
            if schedule == "cascade":
                out = code.decode_ms_cascade_batch(llrs, maxiters, max_sweeps, scale=scale, offset=offset, flooding_scale=flooding_scale,
                                                   flooding_offset=flooding_offset)[0]
            elif schedule == "layered":
                out, _, _ = code.decode_ms_layered_batch(llrs, maxiters, scale=scale, offset=offset)
            else:
                out, _, _ = code.decode_ms_batch(llrs, maxiters, scale=flooding_scale, offset=flooding_offset)      # :22
        diff = out[:, :k8] ^ data                                            # :23-28
        per_frame = popcnt[diff.long()].sum(dim=1)
        errors += int(per_frame.sum())
        frame_errors += int((per_frame > 0).sum())
        trials += batch
        rounds += 1
    bits = trials * code.k()
    ber = max(1, errors) / bits                                              # :59-61
    return trials, bits, errors, ber, frame_errors


def fixed_scale(text: str):
    """`NUM/DEN` -> (scale_num, scale_shift): DEN a power of two of at most 256, 1 <= NUM <= DEN."""
    try:
        num, den = (int(x) for x in text.split("/"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not NUM/DEN")
    if den < 1 or den > 256 or den & (den - 1) or not 1 <= num <= den:
        raise argparse.ArgumentTypeError(f"{text!r}: DEN must be a power of two of at most 256 and 1 <= NUM <= DEN")
    return num, den.bit_length() - 1


def main(argv=None):
    from . import LDPCCode
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--code", default="TC512")                               # perftest/src/main.rs:69
    ap.add_argument("--snrs", default="0.8,0.9,1.0,1.1,1.2,1.3,1.4,1.5,1.6,1.7,1.8,1.9,2.0,2.1,2.2")   # :68
    ap.add_argument("--noise", choices=["perftest", "ebn0"], default="perftest")
    ap.add_argument("--maxiters", type=int, default=100)                     # :22
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--max-bits", type=float, default=5e7)
    ap.add_argument("--max-errors", type=int, default=5000)
    ap.add_argument("--schedule", choices=["flooding", "layered", "cascade"], default="flooding")
    ap.add_argument("--max-sweeps", type=int, default=None, help="cap of the second stage (--schedule cascade; default: --maxiters)")
    ap.add_argument("--scale", type=float, default=1.0, help="normalized min-sum factor, 0 < scale <= 1 (--schedule layered)")
    ap.add_argument("--offset", type=float, default=0.0, help="offset min-sum term in LLR units, >= 0 (--schedule layered)")
    ap.add_argument("--flooding-scale", type=float, default=1.0,
                    help="normalized min-sum factor of the flooding decoder, 0 < scale <= 1 (--schedule flooding / cascade, --llr f32)")
    ap.add_argument("--flooding-offset", type=float, default=0.0,
                    help="offset min-sum term of the flooding decoder in LLR units, >= 0 (--schedule flooding / cascade, --llr f32)")
    ap.add_argument("--llr", choices=["f32", "f16", "bf16", "i8", "i16", "hard"], default="f32",
                    help="LLR type; i8 / i16: the fixed-point layered decoder on quantised frames (--schedule layered); "
                         "f16 / bf16: the f32 frames rounded to the format, through the half-precision entries; "
                         "hard: the f32 frames' signs as packed bits, through the bit-sliced kernels' packed loader (--schedule flooding)")
    ap.add_argument("--hard-magnitude", type=int, default=1, metavar="M", help="the LLR magnitude of a hard decision, 1 .. 127 (--llr hard)")
    ap.add_argument("--llr-scale", type=float, default=8.0, help="quantiser: clamp(rint(scale * y), +-lim) (--llr i8 / i16)")
    ap.add_argument("--llr-lim", type=int, default=31, help="quantiser limit, at most 127 (--llr i8 / i16)")
    ap.add_argument("--fixed-scale", type=fixed_scale, default=None, metavar="NUM/DEN",
                    help="fixed-point normalized min-sum factor, DEN a power of two of at most 256 (--llr i8 / i16)")
    ap.add_argument("--fixed-offset", type=int, default=None, metavar="INT",
                    help="fixed-point offset min-sum term in units of the quantiser, >= 0 (--llr i8 / i16)")
    ap.add_argument("--fixed-flooding-scale", type=fixed_scale, default=None, metavar="NUM/DEN",
                    help="fixed-point normalized min-sum factor of the i8 flooding decoder (--llr i8, --schedule flooding / cascade)")
    ap.add_argument("--fixed-flooding-offset", type=int, default=None, metavar="INT",
                    help="fixed-point offset min-sum term of the i8 flooding decoder, >= 0 (--llr i8, --schedule flooding / cascade)")
    ap.add_argument("--from-f32", action="store_true",
                    help="generate f32 frames and decode them through the f32-input entries (--llr i8 / i16, --schedule layered / cascade)")
    ap.add_argument("--bitsliced-loader", action="store_true",
                    help="decode the f32 frames through the bit-sliced kernels' own loader (--from-f32 --llr i8, --schedule flooding / cascade)")
    args = ap.parse_args(argv)
    if args.llr == "hard" and (args.schedule != "flooding" or args.from_f32 or args.bitsliced_loader or args.flooding_scale != 1.0
                               or args.flooding_offset != 0.0 or args.fixed_scale is not None or args.fixed_offset is not None):
        ap.error("--llr hard needs --schedule flooding and takes --hard-magnitude, --fixed-flooding-scale and --fixed-flooding-offset alone")
    if args.llr != "hard" and args.hard_magnitude != 1:
        ap.error("--hard-magnitude needs --llr hard")
    if args.bitsliced_loader and not (args.from_f32 and args.llr == "i8" and args.schedule in ("flooding", "cascade")):
        ap.error("--bitsliced-loader needs --from-f32 --llr i8 and --schedule flooding or cascade")
    if args.from_f32 and (args.llr in FLOAT_LLRS or (args.schedule == "flooding" and not args.bitsliced_loader)):
        ap.error("--from-f32 needs --llr i8 / i16 and --schedule layered or cascade")
    if args.schedule == "flooding" and (args.scale != 1.0 or args.offset != 0.0):
        ap.error("--scale and --offset need --schedule layered")
    if args.schedule != "cascade" and args.max_sweeps is not None:
        ap.error("--max-sweeps needs --schedule cascade")
    fixed_flooding = args.fixed_flooding_scale is not None or args.fixed_flooding_offset is not None
    if args.llr not in FLOAT_LLRS + ("hard",) and ((args.schedule == "flooding" and not fixed_flooding and not args.bitsliced_loader) or args.scale != 1.0 or args.offset != 0.0):
        ap.error("--llr i8 / i16 needs --schedule layered without --scale and --offset")
    if args.llr in FLOAT_LLRS and (args.fixed_scale is not None or args.fixed_offset is not None):
        ap.error("--fixed-scale and --fixed-offset need --schedule layered --llr i8 / i16")
    if args.fixed_offset is not None and args.fixed_offset < 0:
        ap.error("--fixed-offset must be >= 0")
    scale_num, scale_shift = args.fixed_scale if args.fixed_scale is not None else (None, None)
    fl_num, fl_shift = args.fixed_flooding_scale if args.fixed_flooding_scale is not None else (None, None)
    code = LDPCCode[args.code]
    for snr in (float(x) for x in args.snrs.split(",")):
        trials, bits, errors, ber, fe = ms_trials(code, snr, args.noise, args.maxiters, args.batch,
                                                  args.max_bits, args.max_errors, schedule=args.schedule,
                                                  scale=args.scale, offset=args.offset, llr=args.llr,
                                                  llr_scale=args.llr_scale, llr_lim=args.llr_lim, scale_num=scale_num,
                                                  scale_shift=scale_shift, fixed_offset=args.fixed_offset, max_sweeps=args.max_sweeps,
                                                  from_f32=args.from_f32, flooding_scale=args.flooding_scale,
                                                  flooding_offset=args.flooding_offset, flooding_scale_num=fl_num,
                                                  flooding_scale_shift=fl_shift, flooding_fixed_offset=args.fixed_flooding_offset,
                                                  bitsliced_loader=args.bitsliced_loader, hard_magnitude=args.hard_magnitude)
        print(f"{code.name},{snr:.2f},{trials},{bits},{max(1, errors)},{ber:.5e}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
