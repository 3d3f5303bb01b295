"""Throughput of `ModelForInference.encode` on BERT-family encoders: the packed native forward (`BertEncoder.pooled_cls`,
bert_ops.hip) against the padded PyTorch path (`encoder.BERT_NATIVE = False`), same process, same weights, alternating.

    python tools/bert_encode_bench.py                        # every case, one JSON line
    python tools/bert_encode_bench.py --only base-spread --native-only --reps 2   # one case, native path only (for rocprofv3)
    python tools/bert_encode_bench.py --dtype f32             # an f32 encoder: the packed f32 path (packed_f32=True) against
                                                              # the padded f32 path, plus the f32 attention kernel on its own

Random-weight BGE-small (d 384, 12 x 12 heads, head_dim 32) and BGE-base (d 768, head_dim 64) architectures, fp16 storage
(the reference's BGE setup; --dtype f32: float32 storage, ModelForInference's own default), batch 64, max_length 512, pre-tokenised input: the tokenizer only looks up prepared rows, so the
time is the encoder's.  Two length mixes: uniform 16..512 ("spread") and all 512 ("full").  The work model printed with each
case is what the roofline figures of profiles/ are computed from: attention FLOP = 4 hd nh sum(len_q len_k) over the blocks
(the last block: one query per sequence), LayerNorm / GELU bytes = what the kernels read and write.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


class PreTok:
    """Tokenizer stand-in over prepared rows: the 'text' is the row index; returns right-padded int64 ids + mask."""
    pad_token = "[PAD]"
    padding_side = "right"

    def __init__(self, rows):
        self.rows = rows

    def __call__(self, texts, padding=True, truncation=True, max_length=512, return_tensors="pt"):
        sel = [self.rows[int(t)][:max_length] for t in texts]
        L = max(len(r) for r in sel)
        ids = np.zeros((len(sel), L), dtype=np.int64)
        m = np.zeros((len(sel), L), dtype=np.int64)
        for i, r in enumerate(sel):
            ids[i, :len(r)] = r
            m[i, :len(r)] = 1
        return {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(m)}


def work_model(cfg, lens, batch, es=2):
    """FLOP / bytes the new kernels must move for one pass over `lens` (per the module docstring); es = bytes per element."""
    d, nh, ff, nl = cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size, cfg.num_hidden_layers
    hd = d // nh
    lens = np.asarray(lens, dtype=np.float64)
    T = lens.sum()
    attn_flop = 4 * hd * nh * ((nl - 1) * (lens ** 2).sum() + lens.sum())
    N = len(lens)
    ln_rows = (nl - 1) * 2 * T + 2 * N
    return {"tokens": int(T), "attn_flop": float(attn_flop),
            "layernorm_bytes": float(ln_rows * d * es * 3),                # a + b read, y written
            "gelu_bytes": float(((nl - 1) * T + N) * ff * es * 2),         # read + write in place
            "embed_ln_bytes": float(T * d * es * 4)}                       # word + type + position rows read, y written


F32_MFMA_PEAK = 157.3e12       # v_mfma_f32_16x16x4_f32 on the MI355X, FLOP/s


def attn_kernel_alone(cfg, lens, batch, reps):
    """The f32 attention kernel by itself on one block's shapes: the first 16 batches of `lens` (random q|k|v as column blocks of
    one buffer, the work lists encode() builds), device time by events, median of reps passes over those batches."""
    from rankpo_amd import ops
    d, nh = cfg.hidden_size, cfg.num_attention_heads
    hd = d // nh
    jobs, flop = [], 0.0
    for i in range(0, min(len(lens), 16 * batch), batch):
        ln = [int(n) for n in lens[i:i + batch]]
        T = sum(ln)
        qkv = torch.randn(T, 3 * d, device="cuda:0")
        q, k, v = (qkv[:, j * d:(j + 1) * d].view(T, nh, hd) for j in range(3))
        cu = torch.tensor([0] + np.cumsum(ln).tolist(), dtype=torch.int32, device="cuda:0")
        jobs.append((q, k, v, cu, ops.bidir_attn_tile_table(ln, ln, "cuda:0")))
        flop += 4.0 * hd * nh * float((np.asarray(ln, dtype=np.float64) ** 2).sum())
    scale = hd ** -0.5
    secs = []
    for r in range(reps + 1):                                              # the first pass warms up
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for q, k, v, cu, tiles in jobs:
            ops.bidir_attn_fwd(q, k, v, cu, cu, tiles, scale)
        t1.record()
        torch.cuda.synchronize()
        if r:
            secs.append(t0.elapsed_time(t1) * 1e-3)
    t = float(np.median(secs))
    return {"batches": len(jobs), "seconds": t, "flop": flop, "tflops": flop / t / 1e12,
            "fraction_of_f32_mfma_peak": flop / t / F32_MFMA_PEAK, "all_s": secs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="one case: small-spread, small-full, base-spread, base-full")
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--dtype", choices=["fp16", "f32"], default="fp16",
                    help="storage of the encoder; f32: the packed f32 path against the padded f32 path")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bert_encode_bench.py measures on the GPU"
    import rankpo_amd
    from rankpo_amd import encoder as PE

    archs = {"small": dict(hidden_size=384, intermediate_size=1536, num_attention_heads=12),
             "base": dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12)}
    rs = np.random.RandomState(0)
    mixes = {"spread": rs.randint(16, 513, size=args.sentences), "full": np.full(args.sentences, 512)}
    results = {}
    for arch, kw in archs.items():
        torch.manual_seed(0)
        cfg = PE.bge_small_config(num_hidden_layers=12, **kw)
        enc = PE.build_encoder(cfg)
        for mix, lens in mixes.items():
            case = f"{arch}-{mix}"
            if args.only and case != args.only:
                continue
            rows = [rs.randint(1000, cfg.vocab_size, size=int(n)) for n in lens]
            for r in rows:
                r[0] = 101                                                  # [CLS]
            f32 = args.dtype == "f32"
            inf = rankpo_amd.ModelForInference(encoder=enc, tokenizer=PreTok(rows), use_fp16=not f32, device=0, packed_f32=f32)
            texts = [str(i) for i in range(len(rows))]
            arms = ["native"] if args.native_only else ["native", "stock"]
            outs, times = {}, {a: [] for a in arms}

            def run(arm):
                PE.BERT_NATIVE = arm == "native"
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                o = inf.encode(texts, batch_size=args.batch, max_length=512, convert_to_numpy=False)
                torch.cuda.synchronize()
                return o, time.perf_counter() - t0
            for a in arms:                                                 # warm-up: code objects, GEMM selection
                outs[a] = run(a)[0]
            for _ in range(args.reps):
                for a in arms:
                    times[a].append(run(a)[1])
            PE.BERT_NATIVE = True
            tok = int(lens.sum())
            res = {"work": work_model(cfg, lens, args.batch, 4 if f32 else 2)}
            for a in arms:
                t = float(np.median(times[a]))
                res[a] = {"seconds": t, "sentences_per_s": len(rows) / t, "tokens_per_s": tok / t, "all_s": times[a]}
            if "stock" in res:
                res["speedup"] = res["stock"]["seconds"] / res["native"]["seconds"]
                diff = (outs["native"].float() - outs["stock"].float()).abs().max().item()
                res["max_abs_diff_vs_stock"] = diff
            if f32 and not args.native_only:                               # --native-only: nothing but encode() in a profile
                res["attn_kernel"] = attn_kernel_alone(cfg, lens, args.batch, args.reps)
            results[case] = res
            print(f"{case}: " + ", ".join(f"{a} {res[a]['sentences_per_s']:.0f} sent/s" for a in arms)
                  + (f", speedup {res['speedup']:.2f}x, max |diff| {res['max_abs_diff_vs_stock']:.2e}" if "speedup" in res else "")
                  + (f", f32 attention kernel {res['attn_kernel']['tflops']:.1f} TFLOP/s" if "attn_kernel" in res else ""),
                  file=sys.stderr, flush=True)
            del inf
            torch.cuda.empty_cache()
    print(json.dumps({"bench": "bert_encode", "dtype": "float32" if args.dtype == "f32" else "float16", "batch": args.batch, "max_length": 512,
                      "sentences": args.sentences, "device": torch.cuda.get_device_name(0), "cases": results}))


if __name__ == "__main__":
    main()
