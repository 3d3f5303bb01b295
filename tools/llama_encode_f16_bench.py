"""Throughput of `ModelForInference.encode(use_fp16=True)` on a Llama encoder: the native fp16 pass (`LlamaEncoder.native_fp16`:
causal_attn_f16.hip and the fp16 RMSNorm / RoPE / SwiGLU row kernels) against the path it replaces (switch off:
`aten._flash_attention_forward`, F.rms_norm, the eager rotary chain, two GEMMs + silu * mul), same process, same weights,
alternating.

    python tools/llama_encode_f16_bench.py                     # every case -> profiles/llama_encode_f16_bench.json
    python tools/llama_encode_f16_bench.py --only 1b-passages --on-only --reps 2   # one case, the new path only (for rocprofv3)

Random-weight cuts of the Llama-3.2-1B block (d 2048, 32 / 8 heads, head_dim 64, ff 8192; 4 layers) and of the Llama-3-8B block
(d 4096, 32 / 8 heads, head_dim 128, ff 14336; 2 layers), fp16 storage, batch 64, pre-tokenised input: the tokenizer only looks up
prepared rows, so the time is the encoder's.  The length mixes of bench_inference.py: queries of 640..1280 tokens and passages of
2048..4096, the first row of each full length.
Per case: sentences/s of both arms (median of --reps runs, with every run listed), torch.cuda.max_memory_allocated of each arm,
the largest difference between the arms' rows, and the attention kernel alone (device time by events) under the work model
4 hd nh sum(visible (query, key) pairs): against the 2.5 PFLOP/s dense 16-bit MFMA peak, beside the switch-off attention op
(`aten._flash_attention_forward`) on the same tensors and, as a yardstick, beside the project's own bf16 kernel
(`ops.flash_attn_varlen_fwd`) on the same values cast to bf16."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from bert_encode_bench import PreTok  # noqa: E402  (tools/ is the script's directory)
from llama_encode_f32_bench import visible_pairs  # noqa: E402

MFMA16_PEAK = 2.5e15        # dense fp16 / bf16 MFMA peak of one MI355X, FLOP/s


def _timed(fn, reps):
    secs = []
    for r in range(reps + 1):                                                  # the first pass warms up
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        if r:
            secs.append(t0.elapsed_time(t1) * 1e-3)
    return float(np.median(secs)), secs


def attn_kernel_alone(cfg, lens, batch, reps, max_batches=2):
    """`ops.causal_attn_f16` by itself on one block's shapes for the first batches of `lens`: random q|k|v as column blocks of one
    fp16 buffer, the two work lists encode() builds (full blocks; the last block's one query per sequence); beside it the stock
    flash op on the same tensors and the bf16 hand kernel on the same values cast to bf16.  Device time by events, median of reps
    passes."""
    from rankpo_amd import ops
    nh, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    nq, nk = nh * hd, nkv * hd
    dev = "cuda:0"
    jobs, flop_full, flop_last = [], 0.0, 0.0
    for i in range(0, min(len(lens), max_batches * batch), batch):
        ln = [int(n) for n in lens[i:i + batch]]
        T, N = sum(ln), len(ln)
        qkv = torch.randn(T, nq + 2 * nk, device=dev).half()
        views = lambda x: (x[:, :nq].view(T, nh, hd), x[:, nq:nq + nk].view(T, nkv, hd), x[:, nq + nk:].view(T, nkv, hd))
        cu = torch.tensor([0] + np.cumsum(ln).tolist(), dtype=torch.int32, device=dev)
        jobs.append(dict(qkv=views(qkv), bf=views(qkv.bfloat16()), cu=cu, max_len=max(ln),
                         tiles=ops.causal_attn_f16_tile_table(ln, ln, dev), ql=torch.randn(N, nh, hd, device=dev).half(),
                         cu1=torch.arange(N + 1, dtype=torch.int32, device=dev),
                         tiles1=ops.causal_attn_f16_tile_table([1] * N, ln, dev),
                         bf_tiles=ops.attn_tile_table(ln, dev, nh, nkv),
                         bf_fwd_tiles=ops.attn_fwd_tile_table(ln, dev, nh, nkv, hd)))
        flop_full += 4.0 * hd * nh * visible_pairs(ln, ln)
        flop_last += 4.0 * hd * nh * visible_pairs([1] * N, ln)
    scale = hd ** -0.5
    flash = torch.ops.aten._flash_attention_forward

    def full_f16():
        for j in jobs:
            ops.causal_attn_f16(*j["qkv"], j["cu"], j["cu"], j["tiles"], scale)

    def full_flash():
        for j in jobs:
            flash(*j["qkv"], j["cu"], j["cu"], j["max_len"], j["max_len"], 0.0, True, False)

    def full_bf16():
        for j in jobs:
            if j["bf_fwd_tiles"] is not None:
                ops.flash_attn_varlen_fwd(*j["bf"], j["cu"], j["bf_fwd_tiles"], scale, q_block=64, want_lse=False)
            else:
                ops.flash_attn_varlen_fwd(*j["bf"], j["cu"], j["bf_tiles"], scale, want_lse=False)

    def last_f16():
        for j in jobs:
            ops.causal_attn_f16(j["ql"], j["qkv"][1], j["qkv"][2], j["cu1"], j["cu"], j["tiles1"], scale)

    def last_flash():
        for j in jobs:
            flash(j["ql"], j["qkv"][1], j["qkv"][2], j["cu1"], j["cu"], 1, j["max_len"], 0.0, False, False)

    res = {"batches": len(jobs)}
    for name, flop, arms in (("full", flop_full, (("kernel", full_f16), ("flash_attention_forward", full_flash),
                                                   ("bf16_hand_kernel", full_bf16))),
                             ("last_query", flop_last, (("kernel", last_f16), ("flash_attention_forward", last_flash)))):
        r = {"flop": flop}
        for arm, fn in arms:
            t, secs = _timed(fn, reps)
            r[arm] = {"seconds": t, "tflops": flop / t / 1e12, "fraction_of_mfma16_peak": flop / t / MFMA16_PEAK, "all_s": secs}
        r["kernel_over_flash"] = r["flash_attention_forward"]["seconds"] / r["kernel"]["seconds"]
        if "bf16_hand_kernel" in r:
            r["kernel_over_bf16_hand_kernel"] = r["bf16_hand_kernel"]["seconds"] / r["kernel"]["seconds"]
        res[name] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=128)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="one case: 1b-queries, 1b-passages, 8b-queries, 8b-passages")
    ap.add_argument("--on-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "llama_encode_f16_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "llama_encode_f16_bench.py measures on the GPU"
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
            inf = rankpo_amd.ModelForInference(encoder=enc, tokenizer=PreTok(rows), device=0, use_fp16=True)
            assert next(inf.model.parameters()).dtype == torch.float16
            texts = [str(i) for i in range(len(rows))]
            arms = ["on"] if args.on_only else ["on", "off"]
            outs, times, peak = {}, {a: [] for a in arms}, {}

            def run(arm):
                inf.model.native_fp16 = arm == "on"
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
            inf.model.native_fp16 = False
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
            ak = res.get("attn_kernel", {}).get("full")
            print(f"{case}: " + ", ".join(f"{a} {res[a]['sentences_per_s']:.1f} sent/s ({res[a]['max_memory_allocated'] / 2 ** 30:.1f} GiB)"
                                         for a in arms)
                  + (f", speedup {res['speedup']:.2f}x, max |diff| {res['max_abs_diff_vs_off']:.2e}" if "speedup" in res else "")
                  + (f", attention kernel {ak['kernel']['tflops']:.1f} TFLOP/s, flash op {ak['flash_attention_forward']['tflops']:.1f}, "
                     f"bf16 hand kernel {ak['bf16_hand_kernel']['tflops']:.1f}" if ak else ""),
                  file=sys.stderr, flush=True)
            del inf
            torch.cuda.empty_cache()
    doc = {"bench": "llama_encode_f16", "dtype": "float16", "batch": args.batch, "sentences": args.sentences, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "mfma16_peak_flops": MFMA16_PEAK, "cases": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
