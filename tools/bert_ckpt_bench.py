"""Forward + backward time and peak memory of `ModelForTraining` on BERT-family encoders under gradient checkpointing: what the
reference's `--gradient_checkpointing` gives today (padded path, torch.utils.checkpoint) against checkpointing on the packed native
step (`gradient_checkpointing_enable(packed=True)`), and the price or gain of the fused hidden dropout it rests on.  Same process,
same weights, the arms alternating.

    python tools/bert_ckpt_bench.py --out profiles/bert_ckpt_bench.json      # every case -> one JSON line
    python tools/bert_ckpt_bench.py --only base-spread --arms b --reps 2     # one case, one arm (for rocprofv3)

Arms:  a  padded + checkpointing (the bare flag)            b  packed + checkpointing (packed=True)
       c  packed, no checkpointing, `_hidden_dropout`      d  as c with encoder.BERT_FUSED_HIDDEN_DROPOUT
Random-weight BGE-small (d 384, head_dim 32) and BGE-base (d 768, head_dim 64), fp16 storage, dropout 0.1 (hidden and attention),
the batches of tools/bert_train_bench.py: 64 passage rows of uniform 16..512 ("spread") or all 512 ("full") tokens, 8 query rows.
Timing: HIP events around `--steps` steps, `--warmup` untimed steps per arm first, then `--reps` (7) rounds over the arms in turn;
an arm's figure is the median over its rounds, its spread (max - min) / median.  Memory: torch.cuda.max_memory_allocated over an
arm's timed steps, reset before each round (weights and the batch included: the same for every arm).  Every group of steps runs
under a watchdog (`--limit` seconds): a step that hangs ends the process instead of waiting.
"""
import argparse
import faulthandler
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bert_train_bench import make_batch  # noqa: E402  (the batches of that tool)

ARMS = {"a": dict(ckpt="bare", fused=False), "b": dict(ckpt="packed", fused=False),
        "c": dict(ckpt=None, fused=False), "d": dict(ckpt=None, fused=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--queries", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=float, default=60.0, help="seconds a group of steps may take before the process ends")
    ap.add_argument("--only", default=None, help="one case, e.g. base-spread")
    ap.add_argument("--arms", default="abcd")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bert_ckpt_bench.py measures on the GPU"
    import rankpo_amd
    from rankpo_amd import encoder as PE

    archs = {"small": dict(hidden_size=384, intermediate_size=1536, num_attention_heads=12),
             "base": dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12)}
    arms = [a for a in "abcd" if a in args.arms]
    results = {}
    for arch, kw in archs.items():
        for mix in ("spread", "full"):
            case = f"{arch}-{mix}"
            if args.only and case != args.only:
                continue
            torch.manual_seed(0)
            rs = np.random.RandomState(0)
            cfg = PE.bge_small_config(num_hidden_layers=12, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, **kw)
            enc = PE.build_encoder(cfg)
            model = rankpo_amd.ModelForTraining(encoder=enc.to("cuda:0").to(torch.float16), temperature=0.02).train()
            lens = rs.randint(16, 513, size=args.batch) if mix == "spread" else np.full(args.batch, 512)
            batch = make_batch(rs, cfg.vocab_size, lens, args.queries, "cuda:0")

            def steps(arm, n):
                spec = ARMS[arm]
                model.model.gradient_checkpointing = spec["ckpt"] is not None
                model.model.checkpoint_packed = spec["ckpt"] == "packed"
                PE.BERT_FUSED_HIDDEN_DROPOUT = spec["fused"]
                faulthandler.dump_traceback_later(args.limit, exit=True)     # the time limit of this group of steps
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    model.zero_grad(set_to_none=True)
                    out = model(**batch)
                    (out.loss * 256.0).backward()
                e1.record()
                e1.synchronize()
                faulthandler.cancel_dump_traceback_later()
                return e0.elapsed_time(e1) / n, torch.cuda.max_memory_allocated() / 2 ** 20, float(out.loss.detach())
            times, mem, loss = ({a: [] for a in arms} for _ in range(3))
            for a in arms:                                                # warm-up: code objects, GEMM selection, allocator
                steps(a, args.warmup)
            for _ in range(args.reps):
                for a in arms:
                    t, m, l = steps(a, args.steps)
                    times[a].append(t), mem[a].append(m), loss[a].append(l)
            model.model.gradient_checkpointing = model.model.checkpoint_packed = PE.BERT_FUSED_HIDDEN_DROPOUT = False
            res = {"tokens": int(lens.sum()), "padded_tokens": int(args.batch * lens.max())}
            for a in arms:
                med = float(np.median(times[a]))
                res[a] = {"ms_per_step": med, "all_ms": times[a], "spread": (max(times[a]) - min(times[a])) / med,
                          "peak_mib": max(mem[a]), "loss": loss[a][-1], **{k: v for k, v in ARMS[a].items()}}
            for num, den in (("a", "b"), ("c", "b"), ("c", "d")):           # time of `num` / time of `den`: > 1 = `den` is faster
                if num in res and den in res:
                    res[f"time_{num}_over_{den}"] = res[num]["ms_per_step"] / res[den]["ms_per_step"]
                    res[f"beyond_spread_{num}_{den}"] = bool(max(times[den]) < min(times[num]) or max(times[num]) < min(times[den]))
                    res[f"peak_mib_{num}_over_{den}"] = res[num]["peak_mib"] / res[den]["peak_mib"]
            results[case] = res
            print(f"{case}: " + ", ".join(f"{a} {res[a]['ms_per_step']:.1f} ms (spread {res[a]['spread']:.1%}) {res[a]['peak_mib']:.0f} MiB"
                                          for a in arms), file=sys.stderr, flush=True)
            del model, enc
            torch.cuda.empty_cache()
    line = json.dumps({"bench": "bert_ckpt", "dtype": "float16", "batch": args.batch, "queries": args.queries, "dropout": 0.1,
                       "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
                       "device": torch.cuda.get_device_name(0), "cases": results})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
