"""Forward + backward time of `ModelForTraining` on BERT-family encoders: the packed native training step
(`BertEncoder.pooled_cls_train`, bert_ops.hip) against the padded PyTorch path (`encoder.BERT_NATIVE_TRAIN = False`), same
process, same weights, the arms alternating.

    python tools/bert_train_bench.py                         # every case -> one JSON line (and --out FILE)
    python tools/bert_train_bench.py --only base-spread-p0.1 --native-only --reps 2     # one case, native arm (for rocprofv3)

Random-weight BGE-small (d 384, head_dim 32) and BGE-base (d 768, head_dim 64) architectures, fp16 storage (the reference's BGE
fine-tuning setup).  One step = one tower pair: the passage side holds `batch` = 64 rows of the length mix, the query side 8
rows of 16..32 tokens; InfoNCE loss, loss.backward().  Length mixes: uniform 16..512 ("spread") and all 512 ("full"); dropout 0 and 0.1 (hidden and attention).
Timing: HIP events around the whole step, `--warmup` untimed steps per arm, then `--reps` repeats of `--steps` steps per arm,
alternating; the figure of an arm is the median over its repeats and the spread is (max - min) / median over them.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def make_batch(rs, vocab, lens_p, n_q, device):
    def side(lens):
        L = int(max(lens))
        ids = np.zeros((len(lens), L), dtype=np.int64)
        m = np.zeros((len(lens), L), dtype=np.int64)
        for i, n in enumerate(lens):
            ids[i, :n] = rs.randint(1000, vocab, size=int(n))
            ids[i, 0] = 101                                              # [CLS]
            m[i, :n] = 1
        return {"input_ids": torch.from_numpy(ids).to(device), "attention_mask": torch.from_numpy(m).to(device)}
    return {"query": side(rs.randint(16, 33, size=n_q)), "passage": side(lens_p)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--queries", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="one case, e.g. base-spread-p0.1")
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bert_train_bench.py measures on the GPU"
    assert args.batch % args.queries == 0
    import rankpo_amd
    from rankpo_amd import encoder as PE

    archs = {"small": dict(hidden_size=384, intermediate_size=1536, num_attention_heads=12),
             "base": dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12)}
    results = {}
    for arch, kw in archs.items():
        for mix in ("spread", "full"):
            for p in (0.0, 0.1):
                case = f"{arch}-{mix}-p{p:g}"
                if args.only and case != args.only:
                    continue
                torch.manual_seed(0)
                rs = np.random.RandomState(0)
                cfg = PE.bge_small_config(num_hidden_layers=12, hidden_dropout_prob=p, attention_probs_dropout_prob=p, **kw)
                enc = PE.build_encoder(cfg)
                model = rankpo_amd.ModelForTraining(encoder=enc.to("cuda:0").to(torch.float16), temperature=0.02).train()
                lens = rs.randint(16, 513, size=args.batch) if mix == "spread" else np.full(args.batch, 512)
                batch = make_batch(rs, cfg.vocab_size, lens, args.queries, "cuda:0")
                arms = ["native"] if args.native_only else ["native", "padded"]

                def steps(arm, n):
                    PE.BERT_NATIVE_TRAIN = arm == "native"
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(n):
                        model.zero_grad(set_to_none=True)
                        out = model(**batch)
                        (out.loss * 256.0).backward()
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1) / n, float(out.loss.detach())
                times, loss = {a: [] for a in arms}, {}
                for a in arms:                                            # warm-up: code objects, GEMM selection, allocator
                    loss[a] = steps(a, args.warmup)[1]
                for _ in range(args.reps):
                    for a in arms:
                        times[a].append(steps(a, args.steps)[0])
                PE.BERT_NATIVE_TRAIN = True
                res = {"tokens": int(lens.sum()), "padded_tokens": int(args.batch * lens.max())}
                for a in arms:
                    med = float(np.median(times[a]))
                    res[a] = {"ms_per_step": med, "all_ms": times[a], "spread": (max(times[a]) - min(times[a])) / med,
                              "loss": loss[a]}
                if "padded" in res:
                    res["speedup"] = res["padded"]["ms_per_step"] / res["native"]["ms_per_step"]
                    res["faster_beyond_spread"] = bool(max(times["native"]) < min(times["padded"]))
                results[case] = res
                print(f"{case}: " + ", ".join(f"{a} {res[a]['ms_per_step']:.1f} ms (spread {res[a]['spread']:.1%})" for a in arms)
                      + (f", speedup {res['speedup']:.2f}x" if "speedup" in res else ""), file=sys.stderr, flush=True)
                del model, enc
                torch.cuda.empty_cache()
    line = json.dumps({"bench": "bert_train", "dtype": "float16", "batch": args.batch, "queries": args.queries,
                       "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
                       "device": torch.cuda.get_device_name(0), "cases": results})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
