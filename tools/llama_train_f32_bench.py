"""Forward + backward of `ModelForTraining` on a float32 Llama encoder: the f32 attention kernels of the packed training pass
(`LlamaEncoder.f32_attention_train`: causal_attn_f32.hip with lse, causal_attn_f32_bwd.hip) against the per-sequence SDPA loop
differentiated by autograd (switch off), same process, same weights, alternating.

    python tools/llama_train_f32_bench.py                      # both cases -> profiles/llama_train_f32_bench.json
    python tools/llama_train_f32_bench.py --only 1b --on-only --reps 2     # one case, the new path only (for rocprofv3)

Random-weight cuts of the Llama-3.2-1B block (d 2048, 32 / 8 heads, head_dim 64, ff 8192; 4 layers) and of the Llama-3-8B block
(d 4096, 32 / 8 heads, head_dim 128, ff 14336; 2 layers), float32 storage (what `ModelForTraining` loads when no dtype is given).
The contrastive batch of bench.py: 8 queries of 640..1280 tokens and 40 passages of 2048..4096, the first row of each side full
length, in-batch negatives, T = 0.02; --queries / --passages shrink it, and the batch used is recorded.  No optimizer.
Per case: ms per step of both arms (median of --reps runs, with every run listed, and the spread), torch.cuda.max_memory_allocated
of each arm, the largest relative difference between the arms' gradients (Frobenius, per parameter), and the two backward kernels
alone (one call of rpo_causal_attn_bwd_f32 per form, device time by events) against the 157.3 TFLOP/s of v_mfma_f32_16x16x4_f32
under the work model 10 hd nh sum(visible (query, key) pairs) -- five products per pair; the kernels recompute S in both, so
they EXECUTE seven (14 hd nh per pair), which is recorded beside it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from bert_encode_bench import F32_MFMA_PEAK  # noqa: E402  (tools/ is the script's directory)
from llama_encode_f32_bench import visible_pairs  # noqa: E402


def synth_side(cfg, n, L, rs, dev):
    """bench.py's synthetic side: ids in [1000, vocab - 1000), right padded, lengths in [L / 2, L], the first row full."""
    lens = rs.randint(L // 2, L + 1, size=n)
    lens[0] = L
    ids = torch.from_numpy(rs.randint(1000, cfg.vocab_size - 1000, size=(n, L)))
    m = (torch.arange(L)[None, :] < torch.from_numpy(lens)[:, None]).long()
    return {"input_ids": (ids * m + (cfg.pad_token_id or 0) * (1 - m)).to(dev), "attention_mask": m.to(dev)}, lens


def bwd_kernels_alone(cfg, lens, reps):
    """`ops.causal_attn_f32_bwd` by itself on one block's shapes: random q|k|v as column blocks of one buffer, the forward's
    real out / lse, a random dout; the full form and the last block's one query per sequence."""
    from rankpo_amd import ops
    nh, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    nq, nk = nh * hd, nkv * hd
    dev = "cuda:0"
    ln = [int(n) for n in lens]
    T, N = sum(ln), len(ln)
    qkv = torch.randn(T, nq + 2 * nk, device=dev)
    q, k, v = qkv[:, :nq].view(T, nh, hd), qkv[:, nq:nq + nk].view(T, nkv, hd), qkv[:, nq + nk:].view(T, nkv, hd)
    cu = torch.tensor([0] + np.cumsum(ln).tolist(), dtype=torch.int32, device=dev)
    cu1 = torch.arange(N + 1, dtype=torch.int32, device=dev)
    scale = hd ** -0.5
    res = {}
    for name, qq, cq, lq in (("full", q, cu, ln), ("last_query", torch.randn(N, nh, hd, device=dev), cu1, [1] * N)):
        tiles, k_tiles = ops.causal_attn_f32_tile_table(lq, ln, dev), ops.causal_attn_f32_key_tile_table(lq, ln, dev)
        out, lse = ops.causal_attn_f32(qq, k, v, cq, cu, tiles, scale, want_lse=True)
        dout = torch.randn_like(out)
        secs = []
        for r in range(reps + 1):                                              # the first pass warms up
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            ops.causal_attn_f32_bwd(qq, k, v, out, lse, dout, cq, cu, tiles, k_tiles, scale)
            t1.record()
            torch.cuda.synchronize()
            if r:
                secs.append(t0.elapsed_time(t1) * 1e-3)
        t = float(np.median(secs))
        flop = 10.0 * hd * nh * visible_pairs(lq, ln)
        res[name] = {"seconds": t, "flop": flop, "tflops": flop / t / 1e12, "fraction_of_f32_mfma_peak": flop / t / F32_MFMA_PEAK,
                     "executed_flop": 1.4 * flop, "executed_fraction_of_f32_mfma_peak": 1.4 * flop / t / F32_MFMA_PEAK, "all_s": secs}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8)
    ap.add_argument("--passages", type=int, default=40)
    ap.add_argument("--q-len", type=int, default=1280)
    ap.add_argument("--p-len", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="one case: 1b, 8b")
    ap.add_argument("--on-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "llama_train_f32_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "llama_train_f32_bench.py measures on the GPU"
    assert args.reps >= 5 or args.on_only, "the median of at least 5 runs"
    assert args.passages % args.queries == 0
    import rankpo_amd
    from rankpo_amd import encoder as PE

    # a 32 768-row embedding table: the table's size is no part of what is measured
    archs = {"1b": lambda: PE.llama_3_2_1b_config(num_hidden_layers=4, vocab_size=32768),
             "8b": lambda: PE.llama_3_8b_config(num_hidden_layers=2, vocab_size=32768)}
    results = {}
    for case, make in archs.items():
        if args.only and case != args.only:
            continue
        torch.manual_seed(0)
        cfg = make()
        model = rankpo_amd.ModelForTraining(encoder=PE.build_encoder(cfg).to("cuda:0"), temperature=0.02).train()
        assert next(model.parameters()).dtype == torch.float32
        rs = np.random.RandomState(21)
        query, lens_q = synth_side(cfg, args.queries, args.q_len, rs, "cuda:0")
        passage, lens_p = synth_side(cfg, args.passages, args.p_len, rs, "cuda:0")
        lens = np.concatenate([lens_q, lens_p])
        arms = ["on"] if args.on_only else ["on", "off"]
        times, peak, loss = {a: [] for a in arms}, {}, {}

        def run(arm):
            model.model.f32_attention_train = arm == "on"
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            out = model(query=query, passage=passage)
            out.loss.backward()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            peak[arm] = max(peak.get(arm, 0), torch.cuda.max_memory_allocated())
            loss[arm] = out.loss.item()
            return dt
        grads = {}
        for a in arms:                                                 # warm-up: code objects, GEMM selection; and the gradients
            run(a)
            grads[a] = {k: p.grad.detach().clone() for k, p in model.model.named_parameters()}
        rel = None
        if "off" in grads:
            rel = max(((grads["on"][k].double() - g.double()).norm() / g.double().norm().clamp_min(1e-300)).item()
                      for k, g in grads["off"].items())
        del grads
        torch.cuda.empty_cache()
        for a in arms:                                                 # the allocator refills its cache: not a timed run
            run(a)
        for _ in range(args.reps):
            for a in arms:
                times[a].append(run(a))
        model.model.f32_attention_train = False
        model.zero_grad(set_to_none=True)
        tok = int(lens.sum())
        res = {"layers": cfg.num_hidden_layers, "queries": args.queries, "passages": args.passages, "q_len": args.q_len,
               "p_len": args.p_len, "tokens": tok, "longest_row": int(lens.max()),
               "attn_bwd_flop_per_block": 10.0 * cfg.head_dim * cfg.num_attention_heads * visible_pairs(lens, lens)}
        for a in arms:
            t = float(np.median(times[a]))
            res[a] = {"ms_per_step": t * 1e3, "all_ms": [x * 1e3 for x in times[a]], "spread": (max(times[a]) - min(times[a])) / t,
                      "max_memory_allocated": int(peak[a]), "loss": loss[a]}
        if "off" in res:
            res["speedup"] = res["off"]["ms_per_step"] / res["on"]["ms_per_step"]
            res["max_rel_grad_diff_vs_off"] = rel
        del model
        torch.cuda.empty_cache()
        if not args.on_only:                                               # --on-only: nothing but the step in a profile
            res["bwd_kernels"] = bwd_kernels_alone(cfg, lens, args.reps)
        results[case] = res
        print(f"{case}: " + ", ".join(f"{a} {res[a]['ms_per_step']:.0f} ms ({res[a]['max_memory_allocated'] / 2 ** 30:.1f} GiB)"
                                     for a in arms)
              + (f", speedup {res['speedup']:.2f}x, max rel. gradient diff {rel:.2e}" if "speedup" in res else "")
              + (f", backward kernels {res['bwd_kernels']['full']['tflops']:.1f} TFLOP/s" if "bwd_kernels" in res else ""),
              file=sys.stderr, flush=True)
    doc = {"bench": "llama_train_f32", "dtype": "float32", "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "f32_mfma_peak_flops": F32_MFMA_PEAK, "cases": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
