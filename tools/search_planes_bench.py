"""Search time of an f32 `FlatIPIndex` whose values are exact in neither 16-bit type: the f32 MFMA kernel through the score matrix
(`f32_planes=False`, the default) against the plane-walking 16-bit frame (`f32_planes=True`: three bf16 planes per value, six plane
pairs per score, fused filter step), same process, same corpus, the arms alternating.

    python tools/search_planes_bench.py --out profiles/search_planes_bench.json

Corpus 10^6 x 2048 and 10^6 x 384, f32, normalised randn; 4 x 256 queries (one pass of 1024 rows, as faiss_search regroups them);
k = 100.  Timing: HIP events around `--searches` searches, `--warmup` untimed searches per arm, then `--reps` repeats per arm,
alternating; the figure of an arm is the median over its repeats, the spread (max - min) / median.  The query split is part of the
plane arm's search and is timed with it; the corpus split is paid once when the index is built and is reported on its own.
Accuracy: max |score - f64 score| of both arms on a sample of 4096 random corpus rows (the arms' own kernels on one chunk that holds them).
Model (per search, d the embedding width, Q queries, N corpus rows): planes 6 x 2 Q N d FLOP on the bf16 MFMA and 6 d N bytes of corpus
read per pass; f32 kernel 2 Q N d FLOP on the f32 MFMA, 4 d N bytes of corpus plus 8 Q N bytes of score matrix written and read."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, nargs="+", default=[2048, 384])
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--searches", type=int, default=3, help="searches per timed repeat")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "search_planes_bench.py measures on the GPU"
    assert args.reps >= 7
    from rankpo_amd import ops
    from rankpo_amd.retrieval import FlatIPIndex
    dev = "cuda:0"
    results = {}
    for d in args.dims:
        g = torch.Generator(device=dev).manual_seed(d)
        corpus = torch.empty(args.rows, d, device=dev)
        for r0 in range(0, args.rows, 1 << 17):                      # (piecewise: no second full-size temporary)
            piece = torch.randn(min(1 << 17, args.rows - r0), d, generator=g, device=dev)
            corpus[r0:r0 + piece.shape[0]] = torch.nn.functional.normalize(piece, dim=-1)
        q = torch.nn.functional.normalize(torch.randn(args.queries, d, generator=g, device=dev), dim=-1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        arms = {"f32": FlatIPIndex(corpus, device=dev)}
        e0.record()
        arms["planes"] = FlatIPIndex(corpus, device=dev, f32_planes=True)   # (its exact_in_16 probes run again: part of the build)
        e1.record()
        e1.synchronize()
        build_ms = e0.elapsed_time(e1)
        assert arms["f32"].emb16 is None and arms["f32"].emb_planes is None and arms["planes"].emb_planes is not None
        e0.record()
        ops.split_bf16x3(corpus)
        e1.record()
        e1.synchronize()
        split_ms = e0.elapsed_time(e1)

        def searches(arm, n):
            e0.record()
            for _ in range(n):
                out = arms[arm].search(q, args.k)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / n, out
        times, outs = {a: [] for a in arms}, {}
        for a in arms:
            outs[a] = searches(a, args.warmup)[1]
        for _ in range(args.reps):
            for a in arms:
                times[a].append(searches(a, args.searches)[0])
        assert arms["planes"].fused_overflows == 0
        # accuracy on a sample: the arms' kernels against f64
        # (the frame takes >= 192 tiles: the sample rows are scored at the head of a block of random rows that large)
        block = max(args.sample, -(-192 // -(-args.queries // 256)) * 256)
        rows = torch.randperm(args.rows, generator=g, device=dev)[:block]
        sample = corpus[rows].contiguous()
        f64 = q.double() @ sample[:args.sample].double().T
        qp, fq = ops.split_bf16x3(q)
        sp, fs = ops.split_bf16x3(sample)
        assert int(fq.item()) == 0 and int(fs.item()) == 0
        err = {"f32": float((ops.similarity(q, sample)[:, :args.sample].double() - f64).abs().max()),
               "planes": float((ops.similarity_f32_planes(qp, sp)[:, :args.sample].double() - f64).abs().max())}
        same = float((outs["f32"][1] == outs["planes"][1]).float().mean())
        res = {"rows": args.rows, "d": d, "index_build_ms_planes": build_ms, "corpus_split_ms": split_ms,
               "same_indices": same, "max_abs_score_diff": float((outs["f32"][0] - outs["planes"][0]).abs().max())}
        for a in arms:
            med = float(np.median(times[a]))
            res[a] = {"ms_per_search": med, "all_ms": times[a], "spread": (max(times[a]) - min(times[a])) / med,
                      "max_err_vs_f64_sample": err[a]}
        res["speedup"] = res["f32"]["ms_per_search"] / res["planes"]["ms_per_search"]
        res["faster_beyond_spread"] = bool(max(times["planes"]) < min(times["f32"]))
        flop = 2.0 * args.queries * args.rows * d
        res["model"] = {"planes_bf16_mfma_tflops": 6 * flop / res["planes"]["ms_per_search"] / 1e9,
                        "planes_corpus_bytes": 6 * d * args.rows,
                        "f32_mfma_tflops": flop / res["f32"]["ms_per_search"] / 1e9,
                        "f32_corpus_bytes": 4 * d * args.rows, "f32_score_matrix_bytes": 8 * args.queries * args.rows}
        results[f"d{d}"] = res
        print(f"d {d}: f32 {res['f32']['ms_per_search']:.2f} ms (spread {res['f32']['spread']:.1%}), planes "
              f"{res['planes']['ms_per_search']:.2f} ms (spread {res['planes']['spread']:.1%}), speedup {res['speedup']:.2f}x; "
              f"max err vs f64: f32 {err['f32']:.2e}, planes {err['planes']:.2e}; same indices {same:.4f}", file=sys.stderr, flush=True)
        del arms, corpus, sample, f64, outs
        torch.cuda.empty_cache()
    line = json.dumps({"bench": "search_planes", "queries": args.queries, "k": args.k, "searches": args.searches,
                       "warmup": args.warmup, "reps": args.reps, "device": torch.cuda.get_device_name(0), "cases": results})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
