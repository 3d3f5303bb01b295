"""Throughput of `ModelForInference.encode` on a float32 Llama encoder: the f32 attention kernel of the packed pass
(`LlamaEncoder.f32_attention`, causal_attn_f32.hip) against the per-sequence SDPA loop it replaces (switch off), same process,
same weights, alternating.

    python tools/llama_encode_f32_bench.py                     # every case -> profiles/llama_encode_f32_bench.json
    python tools/llama_encode_f32_bench.py --only 1b-passages --on-only --reps 2   # one case, the new path only (for rocprofv3)

Random-weight cuts of the Llama-3.2-1B block (d 2048, 32 / 8 heads, head_dim 64, ff 8192; 4 layers) and of the Llama-3-8B block
(d 4096, 32 / 8 heads, head_dim 128, ff 14336; 2 layers), float32 storage (what `ModelForInference` loads without use_fp16 /
use_bf16), batch 64, pre-tokenised input: the tokenizer only looks up prepared rows, so the time is the encoder's.  The length
mixes of bench_inference.py: queries of 640..1280 tokens and passages of 2048..4096, the first row of each full length.
Per case: sentences/s of both arms (median of --reps runs, with every run listed), torch.cuda.max_memory_allocated of each arm,
the largest difference between the arms' rows, and the attention kernel alone (device time by events) against the 157.3 TFLOP/s
of v_mfma_f32_16x16x4_f32 under the work model 4 hd nh sum(visible (query, key) pairs)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from bert_encode_bench import F32_MFMA_PEAK, PreTok  # noqa: E402  (tools/ is the script's directory)


def visible_pairs(lens_q, lens_k):
    """(query, key) pairs the bottom-right aligned causal mask lets through, summed over the sequences."""
    lq, lk = np.asarray(lens_q, dtype=np.float64), np.asarray(lens_k, dtype=np.float64)
    return float((lq * (lk - lq) + lq * (lq + 1) / 2).sum())


def attn_kernel_alone(cfg, lens, batch, reps, max_batches=2):
    """`ops.causal_attn_f32` by itself on one block's shapes for the first batches of `lens`: random q|k|v as column blocks of one
    buffer, the two work lists encode() builds (full blocks; the last block's one query per sequence), device time by events,
    median of reps passes."""
    from rankpo_amd import ops
    nh, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    nq, nk = nh * hd, nkv * hd
    dev = "cuda:0"
    jobs, flop_full, flop_last = [], 0.0, 0.0
    for i in range(0, min(len(lens), max_batches * batch), batch):
        ln = [int(n) for n in lens[i:i + batch]]
        T, N = sum(ln), len(ln)
        qkv = torch.randn(T, nq + 2 * nk, device=dev)
        q, k, v = qkv[:, :nq].view(T, nh, hd), qkv[:, nq:nq + nk].view(T, nkv, hd), qkv[:, nq + nk:].view(T, nkv, hd)
        cu = torch.tensor([0] + np.cumsum(ln).tolist(), dtype=torch.int32, device=dev)
        ql = torch.randn(N, nh, hd, device=dev)
        jobs.append((q, k, v, cu, ops.causal_attn_f32_tile_table(ln, ln, dev), ql, torch.arange(N + 1, dtype=torch.int32, device=dev),
                     ops.causal_attn_f32_tile_table([1] * N, ln, dev)))
        flop_full += 4.0 * hd * nh * visible_pairs(ln, ln)
        flop_last += 4.0 * hd * nh * visible_pairs([1] * N, ln)
    scale = hd ** -0.5
    res = {"batches": len(jobs)}
    for name, flop in (("full", flop_full), ("last_query", flop_last)):
        secs = []
        for r in range(reps + 1):                                              # the first pass warms up
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for q, k, v, cu, tiles, ql, cu1, tiles1 in jobs:
                if name == "full":
                    ops.causal_attn_f32(q, k, v, cu, cu, tiles, scale)
                else:
                    ops.causal_attn_f32(ql, k, v, cu1, cu, tiles1, scale)
            t1.record()
            torch.cuda.synchronize()
            if r:
                secs.append(t0.elapsed_time(t1) * 1e-3)
        t = float(np.median(secs))
        res[name] = {"seconds": t, "flop": flop, "tflops": flop / t / 1e12, "fraction_of_f32_mfma_peak": flop / t / F32_MFMA_PEAK,
                     "all_s": secs}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=128)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="one case: 1b-queries, 1b-passages, 8b-queries, 8b-passages")
    ap.add_argument("--on-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "llama_encode_f32_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "llama_encode_f32_bench.py measures on the GPU"
    import rankpo_amd
    from rankpo_amd import encoder as PE

    # a 32 768-row embedding table: the table's size is no part of what is measured
    archs = {"1b": lambda: PE.llama_3_2_1b_config(num_hidden_layers=4, vocab_size=32768),
             "8b": lambda: PE.llama_3_8b_config(num_hidden_layers=2, vocab_size=32768)}
    mixes = {"queries": 1280, "passages": 4096}
    results = {}
    for arch, make in archs.items():
        torch.manual_seed(0)
        cfg = make()
        enc = PE.build_encoder(cfg)
        for mix, L in mixes.items():
            case = f"{arch}-{mix}"
            if args.only and case != args.only:
                continue
            rs = np.random.RandomState(11 if mix == "queries" else 12)
            lens = rs.randint(L // 2, L + 1, size=args.sentences)
            lens[0] = L
            rows = [rs.randint(1000, cfg.vocab_size, size=int(n)) for n in lens]
            inf = rankpo_amd.ModelForInference(encoder=enc, tokenizer=PreTok(rows), device=0)
            assert next(inf.model.parameters()).dtype == torch.float32
            texts = [str(i) for i in range(len(rows))]
            arms = ["on"] if args.on_only else ["on", "off"]
            outs, times, peak = {}, {a: [] for a in arms}, {}

            def run(arm):
                inf.model.f32_attention = arm == "on"
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                o = inf.encode(texts, batch_size=args.batch, max_length=L, convert_to_numpy=False)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                peak[arm] = max(peak.get(arm, 0), torch.cuda.max_memory_allocated())
                return o, dt
            for a in arms:                                                 # warm-up: code objects, GEMM selection
                outs[a] = run(a)[0]
            for _ in range(args.reps):
                for a in arms:
                    times[a].append(run(a)[1])
            inf.model.f32_attention = False
            tok = int(lens.sum())
            res = {"layers": cfg.num_hidden_layers, "max_length": L, "tokens": tok, "longest_row": int(lens.max()),
                   "attn_flop_per_block": 4.0 * cfg.head_dim * cfg.num_attention_heads * visible_pairs(lens, lens)}
            for a in arms:
                t = float(np.median(times[a]))
                res[a] = {"seconds": t, "sentences_per_s": len(rows) / t, "tokens_per_s": tok / t, "all_s": times[a],
                          "spread": (max(times[a]) - min(times[a])) / t, "max_memory_allocated": int(peak[a])}
            if "off" in res:
                res["speedup"] = res["off"]["seconds"] / res["on"]["seconds"]
                res["max_abs_diff_vs_off"] = (outs["on"].float() - outs["off"].float()).abs().max().item()
            del outs
            torch.cuda.empty_cache()
            if not args.on_only:                                           # --on-only: nothing but encode() in a profile
                res["attn_kernel"] = attn_kernel_alone(cfg, lens, args.batch, args.reps)
            results[case] = res
            print(f"{case}: " + ", ".join(f"{a} {res[a]['sentences_per_s']:.1f} sent/s ({res[a]['max_memory_allocated'] / 2 ** 30:.1f} GiB)"
                                         for a in arms)
                  + (f", speedup {res['speedup']:.2f}x, max |diff| {res['max_abs_diff_vs_off']:.2e}" if "speedup" in res else "")
                  + (f", attention kernel {res['attn_kernel']['full']['tflops']:.1f} TFLOP/s" if "attn_kernel" in res else ""),
                  file=sys.stderr, flush=True)
            del inf
            torch.cuda.empty_cache()
    doc = {"bench": "llama_encode_f32", "dtype": "float32", "batch": args.batch, "sentences": args.sentences, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "f32_mfma_peak_flops": F32_MFMA_PEAK, "cases": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
