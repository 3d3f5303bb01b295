#!/usr/bin/env python3
"""Times the fp16 optimizer step against the bf16 one on the same element counts, in one process.

  fp16 step:  rpo_sumsq_partial (fp16) + the sum of its partials, rpo_loss_scale_update, rpo_adamw_step_scaled
  bf16 step:  rpo_sumsq_partial (bf16) + the sum of its partials, the torch clip ops, rpo_adamw_step

Both as `FlatAdamW.step()` runs them (the gradient memset included), and the AdamW and sum-of-squares launches alone through
the C ABI.  Element counts: BGE-small, BGE-base and XLM-R-large parameter counts, and the 1.236 G of optim.hip's own comment.

Protocol: every shape is warmed up; a sample is `--iters` back-to-back calls between two device events at the largest count and
proportionally more at the smaller ones (iters x 1.236 G / n: every sample spans about the same traffic, so that a window is
never a handful of 10-microsecond launches); the two dtypes
alternate inside every round, `--rounds` rounds; reported per call: median, min and max over the rounds.  The spread of the
bf16 samples is the yardstick for any fp16 - bf16 difference.  A gradient buffer of at most 256 MB (BGE-small, BGE-base) fits in
the memory-side cache: its sum-of-squares figure is flagged `sumsq_in_cache` and is not an HBM figure.  Needs a GPU (no fallback).  Writes one JSON file.

    python tools/adamw_f16_bench.py --out profiles/adamw_f16_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [("bge-small", 33_360_000), ("bge-base", 109_482_240), ("xlm-r-large", 559_890_432), ("1.236G", 1_236_000_000)]


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def summary(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw_f16_bench.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default=",".join(n for n, _ in SIZES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adamw_f16_bench needs a GPU: a CPU timing says nothing about the kernels")
    from rankpo_amd import _lib
    from rankpo_amd.train_step import FlatAdamW
    lib, dev = _lib.load(), "cuda:0"
    stream = torch.cuda.current_stream(dev).cuda_stream
    result = {"device": torch.cuda.get_device_name(0), "iters_at_largest": args.iters, "rounds": args.rounds, "sizes": {}}
    for name, n in SIZES:
        if name not in args.sizes.split(","):
            continue
        n = n // 8 * 8
        iters = max(args.iters, args.iters * SIZES[-1][1] // n)
        opts = {}
        for key, dtype in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
            p = torch.nn.Parameter((0.02 * torch.randn(n, device=dev)).to(dtype))
            opts[key] = FlatAdamW([p], lr=1e-5, weight_decay=0.01, max_grad_norm=1.0)
        g32 = 1e-3 * torch.randn(n, device=dev)

        def fill(o):                                          # gradients as a backward under the loss scale leaves them
            s = 1.0 if o.scaler is None else float(o.scaler.init_scale)
            o.reducer.flat.copy_(g32 * s)

        def calls(o):
            dt, a = o.dt, (1e-5, 0.9, 0.999, 1e-8, 0.01)
            ptrs = (o.flat_param.data_ptr(), o.master.data_ptr(), o.reducer.flat.data_ptr(), o.exp_avg.data_ptr(),
                    o.exp_avg_sq.data_ptr())
            one = torch.ones(1, device=dev)
            if o.scaler is None:
                adamw = lambda: lib.rpo_adamw_step(*ptrs, n, dt, *a, 0.1, 0.001, one.data_ptr(), stream)        # noqa: E731
            else:
                adamw = lambda: lib.rpo_adamw_step_scaled(*ptrs, n, dt, *a, o.ls_state.data_ptr(), stream)       # noqa: E731
            sumsq = lambda: lib.rpo_sumsq_partial(ptrs[2], n, dt, o._partial.data_ptr(), o._nblk, stream)        # noqa: E731
            return {"step": o.step, "adamw": adamw, "sumsq": sumsq}
        fns = {k: calls(o) for k, o in opts.items()}
        for k, o in opts.items():                             # warm up every shape and call; leave a non-skipping state
            fill(o)
            o.step()
            fill(o)
            for w, f in fns[k].items():
                rc = f()
                if rc not in (None, 0):
                    sys.exit(f"{k} {w} launch failed with status {rc}")
        torch.cuda.synchronize()
        if opts["fp16"].loss_scale_state()["skipped_steps"]:
            sys.exit("the fp16 warm-up step overflowed: the timed AdamW launches would be skipped ones")
        samples = {k: {w: [] for w in fns[k]} for k in fns}
        for r in range(args.rounds):
            for what in ("step", "adamw", "sumsq"):
                for k in (("bf16", "fp16") if r % 2 == 0 else ("fp16", "bf16")):
                    samples[k][what].append(timed(fns[k][what], iters))
        st = opts["fp16"].loss_scale_state()
        if st["skipped_steps"]:
            sys.exit(f"fp16 steps were skipped during timing: {st}")
        entry = {"n": n, "iters": iters, "bytes_adamw": n * 28, "bytes_sumsq": n * 2, "sumsq_in_cache": n * 2 <= 256 * 2 ** 20}
        for k in samples:
            entry[k] = {w: summary(x) for w, x in samples[k].items()}
            entry[k]["adamw_TBps"] = n * 28 / entry[k]["adamw"]["median_ms"] * 1e-9
        b, f = entry["bf16"], entry["fp16"]
        entry["adamw_fp16_minus_bf16_ms"] = f["adamw"]["median_ms"] - b["adamw"]["median_ms"]
        entry["adamw_bf16_spread_ms"] = b["adamw"]["max_ms"] - b["adamw"]["min_ms"]
        entry["step_fp16_minus_bf16_ms"] = f["step"]["median_ms"] - b["step"]["median_ms"]
        entry["step_bf16_spread_ms"] = b["step"]["max_ms"] - b["step"]["min_ms"]
        result["sizes"][name] = entry
        print(f"{name:12s} n {n:>13,d}  step bf16 {b['step']['median_ms']:.3f} fp16 {f['step']['median_ms']:.3f} ms | adamw bf16 "
              f"{b['adamw']['median_ms']:.3f} [{b['adamw']['min_ms']:.3f}, {b['adamw']['max_ms']:.3f}] fp16 {f['adamw']['median_ms']:.3f} "
              f"[{f['adamw']['min_ms']:.3f}, {f['adamw']['max_ms']:.3f}] ms | sumsq bf16 {b['sumsq']['median_ms']:.3f} fp16 "
              f"{f['sumsq']['median_ms']:.3f} ms", flush=True)
        del opts, fns, g32
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
