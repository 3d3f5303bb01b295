"""Forward + backward of `ModelForTraining` on a float16 Llama encoder: the fp16 attention kernels of the packed training pass
(`LlamaEncoder.native_fp16_train`: causal_attn_f16.hip with lse, causal_attn_f16_bwd.hip) against
`aten._flash_attention_forward` differentiated by PyTorch's flash backward (switch off: the behaviour without the switch), same
process, same weights, alternating.

    python tools/llama_train_f16_bench.py                      # both cases -> profiles/llama_train_f16_bench.json
    python tools/llama_train_f16_bench.py --only 1b --on-only --reps 2     # one case, the new path only (for rocprofv3)
    python tools/llama_train_f16_bench.py --kernels-only --lib other.so --out x.json   # the two kernels alone, another build

Random-weight cuts of the Llama-3.2-1B block (d 2048, 32 / 8 heads, head_dim 64, ff 8192; 4 layers) and of the Llama-3-8B block
(d 4096, 32 / 8 heads, head_dim 128, ff 14336; 2 layers), float16 storage.  The contrastive batch of bench.py: 8 queries of
640..1280 tokens and 40 passages of 2048..4096, the first row of each side full length, in-batch negatives, T = 0.02; --queries /
--passages shrink it, and the batch used is recorded.  No optimizer; the backward runs on loss.float() x --loss-scale (static).
Per case: ms per step of both arms (median of --reps runs, with every run listed, and the spread), torch.cuda.max_memory_allocated
of each arm, whether every gradient was finite, the largest relative difference between the arms' gradients (Frobenius, per
parameter), and the backward alone on one block's shapes (device time by events): `ops.causal_attn_f16_bwd` (both kernels, one
call) against `aten._flash_attention_backward` on the same values (contiguous copies, its own forward's out and lse) and against the
backward of `ops.flash_attn_varlen` on the same values cast to bf16, under the work model 10 hd nh sum(visible (query, key)
pairs) -- five products per pair; the fp16 kernels recompute S in both, so they execute seven."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from llama_encode_f16_bench import MFMA16_PEAK, _timed  # noqa: E402  (tools/ is the script's directory)
from llama_encode_f32_bench import visible_pairs  # noqa: E402
from llama_train_f32_bench import synth_side  # noqa: E402


def bwd_kernels_alone(cfg, lens, reps):
    """The attention backward by itself on one block's shapes: random q|k|v as column blocks of one fp16 buffer, each arm on its
    own forward's out / lse, one random dout; the full form for all three arms, the last block's one query per sequence for the
    fp16 kernels and the flash op."""
    from rankpo_amd import ops
    nh, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    nq, nk = nh * hd, nkv * hd
    dev = "cuda:0"
    ln = [int(n) for n in lens]
    T, N, mx = sum(ln), len(ln), max(int(n) for n in lens)
    qkv = torch.randn(T, nq + 2 * nk, device=dev).half()
    views = lambda x: (x[:, :nq].view(T, nh, hd), x[:, nq:nq + nk].view(T, nkv, hd), x[:, nq + nk:].view(T, nkv, hd))
    q, k, v = views(qkv)
    cu = torch.tensor([0] + np.cumsum(ln).tolist(), dtype=torch.int32, device=dev)
    cu1 = torch.arange(N + 1, dtype=torch.int32, device=dev)
    scale = hd ** -0.5
    flash_f, flash_b = torch.ops.aten._flash_attention_forward, torch.ops.aten._flash_attention_backward
    res = {}
    for name, qq, cq, lq, mq, causal in (("full", q, cu, ln, mx, True),
                                         ("last_query", torch.randn(N, nh, hd, device=dev).half(), cu1, [1] * N, 1, False)):
        tiles, k_tiles = ops.causal_attn_f16_tile_table(lq, ln, dev), ops.causal_attn_f16_key_tile_table(lq, ln, dev)
        out, lse = ops.causal_attn_f16(qq, k, v, cq, cu, tiles, scale, want_lse=True)
        dout = torch.randn(out.shape, device=dev).half()
        arms = [("kernel", lambda: ops.causal_attn_f16_bwd(qq, k, v, out, lse, dout, cq, cu, tiles, k_tiles, scale))]
        qc, kc, vc = qq.contiguous(), k.contiguous(), v.contiguous()
        fo = flash_f(qc, kc, vc, cq, cu, mq, mx, 0.0, causal, False, scale=scale)
        dout3, z = dout.view(-1, nh, hd), torch.zeros((), dtype=torch.int64, device=dev)      # no dropout: the philox words are unused
        arms.append(("flash_attention_backward",
                     lambda: flash_b(dout3, qc, kc, vc, fo[0], fo[1], cq, cu, mq, mx, 0.0, causal, z, z, scale=scale)))
        if name == "full":
            qb, kb, vb = (t.detach().requires_grad_() for t in views(qkv.bfloat16()))
            ob = ops.flash_attn_varlen(qb, kb, vb, cu, ops.attn_tile_table(ln, dev, nh, nkv), mx, scale,
                                       k_tiles=ops.attn_key_tile_table(ln, dev, nkv,
                                                                       ops.ATTN_KEY_BLOCK if hd == 64 else ops.ATTN_KEY_BLOCK_HD128),
                                       key_block=ops.ATTN_KEY_BLOCK if hd == 64 else ops.ATTN_KEY_BLOCK_HD128,
                                       fwd_tiles=ops.attn_fwd_tile_table(ln, dev, nh, nkv, hd))
            db = dout.bfloat16().view(ob.shape)
            arms.append(("bf16_hand_kernels", lambda: torch.autograd.grad(ob, (qb, kb, vb), db, retain_graph=True)))
        flop = 10.0 * hd * nh * visible_pairs(lq, ln)
        r = {"flop": flop, "executed_flop_of_kernel": 1.4 * flop}
        for arm, fn in arms:
            t, secs = _timed(fn, reps)
            r[arm] = {"seconds": t, "tflops": flop / t / 1e12, "fraction_of_mfma16_peak": flop / t / MFMA16_PEAK, "all_s": secs}
        r["kernel_over_flash"] = r["flash_attention_backward"]["seconds"] / r["kernel"]["seconds"]
        if "bf16_hand_kernels" in r:
            r["kernel_over_bf16_hand_kernels"] = r["bf16_hand_kernels"]["seconds"] / r["kernel"]["seconds"]
        res[name] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8)
    ap.add_argument("--passages", type=int, default=40)
    ap.add_argument("--q-len", type=int, default=1280)
    ap.add_argument("--p-len", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loss-scale", type=float, default=256.0)
    ap.add_argument("--only", default=None, help="one case: 1b, 8b")
    ap.add_argument("--on-only", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="the backward kernels alone, no model step")
    ap.add_argument("--lib", default=None, help="another build of librankpo_hip.so (an A/B of compiler flags)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "llama_train_f16_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "llama_train_f16_bench.py measures on the GPU"
    assert args.reps >= 5 or args.on_only, "the median of at least 5 runs"
    assert args.passages % args.queries == 0
    import rankpo_amd
    from rankpo_amd import _lib
    from rankpo_amd import encoder as PE
    if args.lib:                       # the package loaded its own build on import: every op asks _lib.load(), so swap what it returns
        _lib.LIB_PATH, _lib._lib = os.path.abspath(args.lib), None
        _lib.load()

    # a 32 768-row embedding table: the table's size is no part of what is measured
    archs = {"1b": lambda: PE.llama_3_2_1b_config(num_hidden_layers=4, vocab_size=32768),
             "8b": lambda: PE.llama_3_8b_config(num_hidden_layers=2, vocab_size=32768)}
    results = {}
    for case, make in archs.items():
        if args.only and case != args.only:
            continue
        torch.manual_seed(0)
        cfg = make()
        rs = np.random.RandomState(21)
        query, lens_q = synth_side(cfg, args.queries, args.q_len, rs, "cuda:0")
        passage, lens_p = synth_side(cfg, args.passages, args.p_len, rs, "cuda:0")
        lens = np.concatenate([lens_q, lens_p])
        if args.kernels_only:
            results[case] = {"bwd_kernels": bwd_kernels_alone(cfg, lens, args.reps)}
            b = results[case]["bwd_kernels"]["full"]
            print(f"{case}: backward kernels {b['kernel']['seconds'] * 1e3:.2f} ms, flash {b['kernel_over_flash']:.2f}x", file=sys.stderr,
                  flush=True)
            continue
        model = rankpo_amd.ModelForTraining(encoder=PE.build_encoder(cfg).to("cuda:0", torch.float16), temperature=0.02).train()
        assert next(model.parameters()).dtype == torch.float16
        assert not model.model.native_fp16_train and not PE.LLAMA_FP16_NATIVE_TRAIN          # "off" is the code without the switch
        arms = ["on"] if args.on_only else ["on", "off"]
        times, peak, loss = {a: [] for a in arms}, {}, {}

        def run(arm):
            model.model.native_fp16_train = arm == "on"
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            out = model(query=query, passage=passage)
            (out.loss.float() * args.loss_scale).backward()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            peak[arm] = max(peak.get(arm, 0), torch.cuda.max_memory_allocated())
            loss[arm] = out.loss.item()
            return dt
        grads = {}
        for a in arms:                                                 # warm-up: code objects, GEMM selection; and the gradients
            run(a)
            grads[a] = {k: p.grad.detach().clone() for k, p in model.model.named_parameters()}
        finite = {a: all(bool(torch.isfinite(g).all()) for g in grads[a].values()) for a in arms}
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
        model.model.native_fp16_train = False
        model.zero_grad(set_to_none=True)
        tok = int(lens.sum())
        res = {"layers": cfg.num_hidden_layers, "queries": args.queries, "passages": args.passages, "q_len": args.q_len,
               "p_len": args.p_len, "tokens": tok, "longest_row": int(lens.max()), "loss_scale": args.loss_scale,
               "attn_bwd_flop_per_block": 10.0 * cfg.head_dim * cfg.num_attention_heads * visible_pairs(lens, lens)}
        for a in arms:
            t = float(np.median(times[a]))
            res[a] = {"ms_per_step": t * 1e3, "all_ms": [x * 1e3 for x in times[a]], "spread": (max(times[a]) - min(times[a])) / t,
                      "max_memory_allocated": int(peak[a]), "loss": loss[a], "gradients_finite": finite[a]}
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
              + (f", backward kernels {res['bwd_kernels']['full']['kernel']['tflops']:.1f} TFLOP/s, "
                 f"{res['bwd_kernels']['full']['kernel_over_flash']:.2f}x flash" if "bwd_kernels" in res else ""),
              file=sys.stderr, flush=True)
    doc = {"bench": "llama_train_f16", "dtype": "float16", "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "mfma16_peak_flops": MFMA16_PEAK, "library": os.path.basename(args.lib) if args.lib else "librankpo_hip.so",
           "cases": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
