"""Time and peak memory of the embedding-table gradients of the packed BERT / XLM-R training step: the stock atomic `index_add_`
into f32 tables (switch off) against `ops.embed_grad_sorted` (encoder.BERT_DETERMINISTIC_EMBED_GRAD on).  Same process, same
weights, same batch, the two arms alternating.

    python tools/embed_grad_bench.py --out profiles/embed_grad_bench.json      # every case -> one JSON line
    python tools/embed_grad_bench.py --only small-spread --reps 2

Cases: BGE-small (30522 x 384 word table, 12 blocks), BGE-base (30522 x 768, 12 blocks) and XLM-R large (250002 x 1024, 24 blocks:
bge-m3's backbone), random weights, fp16 storage, dropout 0.1, 64 passage rows of uniform 16..512 ("spread") or all 512 ("full")
tokens and 8 query rows.  Token ids are log-uniform over the vocabulary (frequency ~ 1 / rank, as text is), [CLS] first: what decides
how many rows of ds meet in one table row.
Per arm, the median over `--reps` (7) rounds, the arms in turn inside a round, after `--warmup` untimed rounds; all rounds of the
backward alone come before the first step of a case:
  embed_bwd_ms   the backward of `ops.bert_embed_ln_train` alone (LayerNorm backward kernel + the three table gradients) on the
                 passage tower's pack, HIP events around `--inner` backwards
  step_ms        forward + backward of `ModelForTraining`, HIP events around `--steps` steps (host packing and, switch on, the
                 plans included)
  *_peak_mib     torch.cuda.max_memory_allocated over those (weights and batch included: the same for both arms), and
  *_over_start_mib  the same minus what was allocated when the group began (gradients dropped first): what the group itself adds
and `plan_host_ms`: the host time of the `ops.embed_grad_plan` calls for the passage tower (part of step_ms when on).  Once per
case, at the timed size: whether two backwards of an arm return equal word-table bits, and the distance between the arms' results.
No pass mark: the sorted form is there for bit-reproducibility and the missing f32 table, not for speed.
"""
import argparse
import faulthandler
import gc
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def make_side(rs, vocab, lens, device):
    L = int(max(lens))
    ids, m = np.zeros((len(lens), L), dtype=np.int64), np.zeros((len(lens), L), dtype=np.int64)
    for i, n in enumerate(lens):
        ids[i, :n] = np.minimum(1000 + np.floor((vocab - 1000) ** rs.rand(int(n))).astype(np.int64), vocab - 1)
        ids[i, 0] = 101
        m[i, :n] = 1
    return {"input_ids": torch.from_numpy(ids).to(device), "attention_mask": torch.from_numpy(m).to(device)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--queries", type=int, default=8)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a timed group may take before the process ends")
    ap.add_argument("--only", default=None, help="one case, e.g. xlmr-full")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "embed_grad_bench.py measures on the GPU"
    import rankpo_amd
    from rankpo_amd import encoder as PE, ops
    dev = "cuda:0"
    archs = {"small": lambda: PE.bge_small_config(hidden_size=384, intermediate_size=1536, num_attention_heads=12),
             "base": lambda: PE.bge_small_config(hidden_size=768, intermediate_size=3072, num_attention_heads=12),
             "xlmr": lambda: PE.xlm_roberta_config(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)}
    results = {}
    for arch, mk in archs.items():
        if args.only and not args.only.startswith(arch + "-"):
            continue
        torch.manual_seed(0)
        cfg = mk()
        enc = PE.build_encoder(cfg).to(torch.float16).to(dev)
        model = rankpo_amd.ModelForTraining(encoder=enc, temperature=0.02).train()
        emb = enc.embeddings
        for mix in ("spread", "full"):
            case = f"{arch}-{mix}"
            if args.only and case != args.only:
                continue
            rs = np.random.RandomState(0)
            lens = rs.randint(16, 513, size=args.batch) if mix == "spread" else np.full(args.batch, 512)
            batch = {"query": make_side(rs, cfg.vocab_size, rs.randint(16, 33, size=args.queries), dev),
                     "passage": make_side(rs, cfg.vocab_size, lens, dev)}

            def timed(fn, n):
                faulthandler.dump_traceback_later(args.limit, exit=True)
                model.zero_grad(set_to_none=True)                            # gradients of the group before are not this one's
                gc.collect()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                start = torch.cuda.memory_allocated()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    fn()
                e1.record()
                e1.synchronize()
                faulthandler.cancel_dump_traceback_later()
                peak = torch.cuda.max_memory_allocated()
                return e0.elapsed_time(e1) / n, peak / 2 ** 20, (peak - start) / 2 ** 20

            def step():
                model.zero_grad(set_to_none=True)
                out = model(**batch)
                (out.loss * 256.0).backward()

            def embed_arm(on):
                """The embedding op on the passage pack with its graph kept: () -> one backward."""
                PE.BERT_DETERMINISTIC_EMBED_GRAD = on
                pk = enc._pack_upload(batch["passage"]["input_ids"], batch["passage"]["attention_mask"].cpu(), None, train=True)
                tables = (emb.word_embeddings.weight, emb.token_type_embeddings.weight, emb.position_embeddings.weight)
                y = ops.bert_embed_ln_train(pk.ids, pk.pos, pk.tts, *tables, emb.LayerNorm.weight, emb.LayerNorm.bias,
                                            emb.LayerNorm.eps, emb.word_embeddings.padding_idx, 0.0, 0, pk.embed_plans)
                dy = torch.randn(y.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).to(y.dtype)

                def bwd():
                    model.zero_grad(set_to_none=True)
                    y.backward(dy, retain_graph=True)
                return bwd, pk
            bwd, word_grad = {}, {}
            for on in (False, True):
                bwd[on], pk = embed_arm(on)
                word_grad[on] = []
                for _ in range(2):                                           # the results at the timed size, twice per arm
                    bwd[on]()
                    word_grad[on].append(emb.word_embeddings.weight.grad.clone())
            same = {on: bool(torch.equal(*word_grad[on])) for on in (False, True)}
            rel = float((word_grad[True][0].double() - word_grad[False][0].double()).norm() / word_grad[False][0].double().norm())
            del word_grad
            host_ids = [t.cpu() for t in (pk.ids, pk.pos)]
            t0 = time.perf_counter()
            for _ in range(5):
                for t in host_ids:
                    ops.embed_grad_plan(t)
            plan_ms = (time.perf_counter() - t0) / 5 * 1e3
            keys = ("embed_bwd_ms", "embed_bwd_peak_mib", "embed_bwd_over_start_mib", "step_ms", "step_peak_mib", "step_over_start_mib")
            rec = {on: {k: [] for k in keys} for on in (False, True)}
            for group, fn_of, n in ((keys[:3], lambda on: bwd[on], args.inner), (keys[3:], lambda on: step, args.steps)):
                for r in range(args.warmup + args.reps):                     # all rounds of the backward alone, then all of the step
                    for on in (False, True):
                        PE.BERT_DETERMINISTIC_EMBED_GRAD = on
                        figures = timed(fn_of(on), n)
                        if r >= args.warmup:
                            for k, v in zip(group, figures):
                                rec[on][k].append(v)
            PE.BERT_DETERMINISTIC_EMBED_GRAD = False
            res = {"tokens": int(lens.sum()), "table": [cfg.vocab_size, cfg.hidden_size], "blocks": cfg.num_hidden_layers,
                   "distinct_word_ids": int(torch.unique(pk.ids).numel()), "plan_host_ms": plan_ms,
                   "word_grad_two_calls_equal_bits": {"off": same[False], "on": same[True]}, "word_grad_on_vs_off_rel_norm": rel}
            for on in (False, True):
                a = rec[on]
                res["on" if on else "off"] = {
                    "embed_bwd_ms": float(np.median(a["embed_bwd_ms"])), "embed_bwd_all_ms": a["embed_bwd_ms"],
                    "embed_bwd_peak_mib": max(a["embed_bwd_peak_mib"]), "embed_bwd_over_start_mib": max(a["embed_bwd_over_start_mib"]),
                    "step_ms": float(np.median(a["step_ms"])), "step_all_ms": a["step_ms"], "step_peak_mib": max(a["step_peak_mib"]),
                    "step_over_start_mib": max(a["step_over_start_mib"])}
            for k in ("embed_bwd_ms", "step_ms"):
                res[f"{k}_on_over_off"] = res["on"][k] / res["off"][k]
                lo, hi = rec[True][k], rec[False][k]
                res[f"{k}_beyond_spread"] = bool(max(lo) < min(hi) or max(hi) < min(lo))
            results[case] = res
            print(f"{case}: " + ", ".join(
                f"{n} bwd {res[n]['embed_bwd_ms']:.3f} ms / {res[n]['embed_bwd_peak_mib']:.0f} MiB "
                f"(+{res[n]['embed_bwd_over_start_mib']:.0f}), step {res[n]['step_ms']:.1f} ms / {res[n]['step_peak_mib']:.0f} MiB"
                for n in ("off", "on")) + f", plans {plan_ms:.2f} ms on the host",
                file=sys.stderr, flush=True)
            del bwd, pk, batch
            model.zero_grad(set_to_none=True)
            torch.cuda.empty_cache()
        del model, enc, emb
        torch.cuda.empty_cache()
    line = json.dumps({"bench": "embed_grad", "dtype": "float16", "batch": args.batch, "queries": args.queries, "dropout": 0.1,
                       "chunk": ops.EMBED_GRAD_CHUNK, "steps": args.steps, "inner": args.inner, "warmup": args.warmup,
                       "reps": args.reps, "device": torch.cuda.get_device_name(0), "cases": results})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
