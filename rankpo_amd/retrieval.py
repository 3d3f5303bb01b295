"""Exact inner-product retrieval + ranking metrics ("next" row f3 of SURVEY.md §8; reference: src/utils.py:38-153,
used by src/evaluate.py and src/get_hard_negatives.py through FAISS `IndexFlatIP`).

`FlatIPIndex.search` is the flat-index search: the corpus is walked in chunks; scores = Q C_chunk^T come from the HIP
similarity kernel of the hot path (f32 storage -> f32 MFMA, like FAISS' sgemm; bf16 MFMA with f32 sums when every value is
exact in bf16) and `rpo_topk_merge` folds every chunk's
scores into the k winners per query (value descending, ties by the smaller corpus index) -- the [nq, ntotal] score matrix is
never materialised, so the corpus size is bounded by the embeddings alone (288 GB of HBM: ~35 M rows of d = 2048 in f32; the
16-bit copy of an f32 index that is exact in bf16 / fp16 is taken only while it fits beside it).  `compute_metrics` keeps the reference's definitions (its non-standard Recall denominator
`max(min(cutoff, len(pred), len(label)), 1)`, the flattened "naive AUC") but computes them on one boolean hit matrix.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import ops


def exact_in_16(x, dtype=torch.bfloat16):
    """x (f32, on the GPU) as `dtype` (bf16 / fp16) if EVERY value survives f32 -> dtype -> f32 unchanged, else None.  fp16 subnormals
    count as exact: v_mfma_f32_16x16x32_f16 multiplies them exactly (tests/test_gpu_kernels.py pins that; a normalized d = 384
    embedding has one in a thousand values below 2^-14).  One device flag, one sync."""
    if x.dtype != torch.float32 or not x.is_cuda or x.numel() == 0:
        return None
    free, _ = torch.cuda.mem_get_info(x.device)
    if free + torch.cuda.memory_reserved(x.device) - torch.cuda.memory_allocated(x.device) < 2 * x.numel() + (2 << 30):
        return None                                                 # an index that fills the HBM keeps its one copy and the f32 kernel
    h = torch.empty(x.shape, dtype=dtype, device=x.device)
    ok = torch.ones((), dtype=torch.bool, device=x.device)
    step = max(1, (1 << 27) // max(1, x.shape[-1]))                 # ~0.5 GB of f32 per piece
    for r0 in range(0, x.shape[0], step):
        piece = x[r0:r0 + step]
        h[r0:r0 + step] = piece
        ok &= (h[r0:r0 + step].float() == piece).all()
    return h if bool(ok.item()) else None


def exact_in_bf16(x):
    return exact_in_16(x, torch.bfloat16)


def exact_in_planes(x):
    """x (f32 [rows, d] on the GPU, d % 64 == 0) as three bf16 planes [rows, 3 d] = h | m | l with x == h + m + l (ops.split_bf16x3) if
    that holds for EVERY value with planes that are normal or zero, else None.  Memory rule of `exact_in_16` (6 bytes per value);
    one device flag, one sync."""
    if x.dtype != torch.float32 or not x.is_cuda or x.dim() != 2 or x.numel() == 0 or x.shape[1] % 64 != 0:
        return None
    free, _ = torch.cuda.mem_get_info(x.device)
    if free + torch.cuda.memory_reserved(x.device) - torch.cuda.memory_allocated(x.device) < 6 * x.numel() + (2 << 30):
        return None
    planes, inexact = ops.split_bf16x3(x)
    return None if int(inexact.item()) else planes


class _Frame(NamedTuple):
    """How one search scores: the operands and the names of the ops (looked up on `ops` at call time) of one kernel frame."""
    q: torch.Tensor             # the queries as the frame takes them
    corpus: Optional[torch.Tensor]      # the corpus likewise, chunked by rows; None: the plain kernel on `emb` only
    takes: Optional[str]        # operand predicate asked per chunk; None: decided for all chunks up front
    scores: str                 # the frame's score matrix of a chunk
    step: Optional[str]         # the fused filter step
    step_args: dict
    planes: bool                # the plane frame: one schedule (the fused one) for every walk


class FlatIPIndex:
    """Stands where the reference builds `faiss.IndexFlatIP` (utils.py:38-51): keeps the corpus embeddings on the GPU.

    An f32 index (the reference's dtype) whose embeddings are exactly representable in bf16 -- what `ModelForInference.encode` hands
    over when the encoder computes in bf16, as scripts/evaluate/run_evaluate.sh runs it -- or in fp16 (`use_fp16`, the BGE setup) keeps
    a 16-bit copy (`emb16`) and scores queries that are exact in that type too with the 16-bit MFMA kernel frame: the products are exact in f32 and the sums are f32 sums, i.e.
    an f32 inner product in that kernel's summation order (as FAISS' sgemm has its own), at 16 x the f32 MFMA rate and with the
    fused filter step.  Scores stay f32, unrounded.  Anything else (values or queries not exact in bf16) takes the f32 kernel --
    unless `f32_planes` is set: then an f32 index with d % 64 == 0 that is exact in neither type keeps its values as three bf16 planes
    (`emb_planes`, [ntotal, 3 d]: x == h + m + l, `exact_in_planes`) and the same frame walks six plane pairs per score, smallest terms
    first -- exact products, f32 sums in the frame's order, the fused filter step; what it leaves out (the pairs ml, lm, ll) is below
    2^-23 |q_i c_i| per element, the rounding of an f32 multiply.  ONE value whose planes leave the normal range (non-zero and below
    ~2^-110 in magnitude, where l turns subnormal) declines the planes for the whole index, silently: check `emb_planes`.
    Off by default: measured numbers in DESIGN.md."""

    candidate_fill = 0.25       # fused search: expected survivors per row and chunk / candidate slots (chunk_schedule)

    def __init__(self, embeddings, device="cuda:0", dtype=torch.float32, chunk_rows: int = 262144, split=None, exact16: bool = True,
                 f32_planes: bool = False):
        e = torch.as_tensor(np.asarray(embeddings, dtype=np.float32) if not torch.is_tensor(embeddings) else embeddings)
        self.emb = e.to(device=device, dtype=dtype).contiguous()
        self.ntotal = self.emb.shape[0]
        self.chunk_rows = chunk_rows
        self.split = split                  # winner lists per query row in the selection kernel; None: by the batch size (search)
        # queries scored per pass over the corpus: every pass streams the whole corpus out of HBM, so a batch of 256 (the reference's
        # faiss_search default) sits at the machine balance (256 FLOP per corpus byte) while 1024 reads the corpus a quarter as
        # often and is MFMA-bound; `faiss_search` regroups the caller's batches up to this many rows (rows are independent: same result)
        self.query_rows_per_pass = 1024
        self.fused = True                   # the fused filter step where it applies (search); False: always through the score matrix
        self.fused_overflows = 0            # searches redone because a candidate list ran over
        # f32 index, values exact in bf16 (a --bf16 encoder run) or in fp16 (--fp16): see above
        self.emb16 = None
        if exact16 and self.emb.shape[1] % 64 == 0:                  # (exact16 = False: never take the 16-bit copy, half an index more of HBM)
            self.emb16 = exact_in_16(self.emb, torch.bfloat16)
            if self.emb16 is None:
                self.emb16 = exact_in_16(self.emb, torch.float16)
        # f32 index exact in neither 16-bit type, on request: three bf16 planes (class docstring); None: nothing changes
        self.emb_planes = exact_in_planes(self.emb) if f32_planes and self.emb16 is None else None

    def chunk_schedule(self, nq: int, k: int, fused: bool = True):
        """[(first row, end row)] of the corpus chunks a search of nq query rows walks.  Plain: `chunk_rows` at a time.  Fused: the
        only chunk that still needs its score matrix and a selection pass over it is the FIRST (it fills the winners), so it is made
        as small as the 256 x 256 scoring kernel admits (>= 192 tiles, >= k rows: 12,288 rows at 1024 queries).  A later chunk of n
        rows behind c seen rows brings ~k n / c survivors per row (exchangeable scores): n grows with c so that this stays at a
        quarter of the candidate list (`candidate_fill`: 2.56 c at k = 100; at k = 1024, where the lists hold 3 k, never below the
        first chunk's size, i.e. a third of the list), up to chunk_rows.  Measured at 10^6 x 2048, 1024 queries, k = 100: lists
        1/8, 1/4, 1/2 full 3.86 / 3.82 / 3.85 ms (gpurun_out/r6_N) -- a chunk with more survivors pays for them in the filter's
        epilogue what it saves in launches.  A tail too small for the kernel is joined to the last chunk.
        An index that holds `emb_planes` cuts every schedule -- also that of a search which falls through to the f32 kernel -- so
        that a chunk's planes stay below 4 GB: below the default chunk_rows only for d > 2730."""
        chunk_rows = self.chunk_rows
        planes = getattr(self, "emb_planes", None) is not None
        if planes:                                                  # a chunk's planes (6 d bytes per row) stay below 4 GB: 32-bit piece offsets
            chunk_rows = max(256, min(chunk_rows, ((1 << 32) - 1) // (6 * self.emb.shape[1]) // 256 * 256))
        plain = [(c0, min(c0 + chunk_rows, self.ntotal)) for c0 in range(0, self.ntotal, chunk_rows)]
        if not fused or not (self.emb.dtype == torch.bfloat16 or getattr(self, "emb16", None) is not None or planes) or nq <= 0:
            return plain
        first = max(-(-192 // -(-nq // 256)), -(-k // 256)) * 256
        if 2 * first > min(chunk_rows, self.ntotal) or not ops.search_filter_ok(nq, first, self.emb.shape[1]):
            return plain
        out, c = [(0, first)], first
        while c < self.ntotal:
            n = max(first, int(c * ops.search_candidate_cap(k) * self.candidate_fill / k) // 256 * 256)
            n = min(n, chunk_rows, self.ntotal - c)
            if self.ntotal - (c + n) < first:
                n = self.ntotal - c
            out.append((c, c + n))
            c += n
        return out

    def search(self, queries, k: int):
        """(scores f32 [nq, k], corpus indices int64 [nq, k]), best first; k is clamped to the corpus size."""
        q = torch.as_tensor(np.asarray(queries, dtype=np.float32) if not torch.is_tensor(queries) else queries)
        q = q.to(device=self.emb.device, dtype=self.emb.dtype).contiguous()
        k = min(k, self.ntotal)
        if k > ops.TOPK_MAX_K:
            raise ValueError(f"FlatIPIndex.search: k <= {ops.TOPK_MAX_K}")
        # `split` winner lists per query row (rpo_topk_merge_split) would put more selection blocks on the chip than the few hundred
        # queries of a batch (the reference searches 256 at a time, utils.py:58-80) -- measured, it LOSES: every list pays its own
        # bootstrap and its own re-selections (10^6 x 2048 corpus, 4 x 256 queries, k = 100: 8.6 ms with 4 lists per row against
        # 5.65 with one, gpurun_out/r6_D).  One list per row unless the caller says otherwise.
        split = 1 if self.split is None else int(self.split)
        # Fused step (round 6, bf16 index): once the winners hold k real entries, a chunk's scores are compared with each row's k-th
        # winner inside the scoring kernel and only the survivors leave the chip -- no [nq, chunk] score matrix (512 MB per chunk at
        # 1024 queries), no second pass over it.  A candidate list that runs over (a corpus whose later rows keep beating everything
        # before them) raises the workspace's flag and the search is redone the plain way.
        fused = self.fused and split == 1
        fr = self._planes_frame(q, k) if getattr(self, "emb_planes", None) is not None else None
        if fr is None:
            # f32 index exact in bf16 / fp16 + queries exact in that type: the 16-bit kernel frame with f32 scores (class docstring)
            q16 = exact_in_16(q, self.emb16.dtype) if self.emb16 is not None and q.shape[0] > 0 else None
            if q16 is not None:
                fr = _Frame(q16, self.emb16, "search_filter_takes", "similarity_f32", "search_step", {"round_scores": False}, False)
            elif self.emb.dtype == torch.bfloat16:
                fr = _Frame(q, self.emb, "search_filter_takes", "similarity", "search_step", {"round_scores": True}, False)
            else:
                fr = _Frame(q, None, None, "similarity", None, {}, False)
        # the plane frame keeps the fused schedule whatever the walk; the others take it for a fused walk only
        sched = self.chunk_schedule(q.shape[0], k, fr.planes or (fused and fr.corpus is not None))
        top, idx, ws = self._walk(q, k, split, fr, sched, fused)
        if ws is not None and int(ws.overflow.item()):              # redo through the score matrix: planes on the same chunks, else plain
            self.fused_overflows += 1
            top, idx, _ = self._walk(q, k, split, fr, sched if fr.planes else self.chunk_schedule(q.shape[0], k, False), False)
        return ops.topk_finish(top, idx, split)

    def _walk(self, q, k, split, fr, sched, fused):
        """One pass over the chunks of `sched` with the frame `fr`: (winners, indices, the fused steps' workspace or None).  A chunk the
        frame takes goes through the fused step once the winners hold k entries (fused), else through the frame's score matrix +
        topk_merge; a chunk it does not take through `similarity` on the index's own rows."""
        top = idx = ws = None
        for c0, c1 in sched:
            chunk = fr.corpus[c0:c1] if fr.corpus is not None else None
            takes = chunk is not None and (fr.takes is None or getattr(ops, fr.takes)(fr.q, chunk))
            if fused and c0 >= k and takes:
                ws = ws or ops.SearchWorkspace(q.shape[0], k, q.device)
                getattr(ops, fr.step)(fr.q, chunk, c0, top, idx, ws, **fr.step_args)
                continue
            scores = getattr(ops, fr.scores)(fr.q, chunk) if takes else ops.similarity(q, self.emb[c0:c1])   # [nq, chunk]  (HIP MFMA kernel)
            top, idx = ops.topk_merge(scores, c0, top, idx, k, split=split)     # HIP selection kernel
        return top, idx, ws

    def _planes_frame(self, q, k):
        """The frame of a search on `emb_planes`: the queries are split per call; None (search goes on to the other frames) when they
        are not exact in three planes or a chunk of the fused schedule is not of a shape the plane frame takes.  The first chunk goes
        through the frame's score matrix + topk_merge, the later ones through the fused step (fused) or the score matrix too, so
        every score of a search comes out of one summation order."""
        if q.shape[0] == 0 or q.shape[1] != self.emb.shape[1]:
            return None
        qp, inexact = ops.split_bf16x3(q)
        if int(inexact.item()):
            return None
        if not all(ops.search_planes_takes(qp, self.emb_planes[c0:c1]) for c0, c1 in self.chunk_schedule(q.shape[0], k, True)):
            return None
        return _Frame(qp, self.emb_planes, None, "similarity_f32_planes", "search_step_planes", {}, True)


def create_faiss_index(embeddings, device="cuda:0", f32_planes: bool = False):
    """Name kept from the reference (utils.py:38).  f32_planes: FlatIPIndex's opt-in plane frame for f32 embeddings."""
    return FlatIPIndex(embeddings, device=device, f32_planes=f32_planes)


def faiss_search(index: FlatIPIndex, query_embedding, topk: int = 100, batch_size: int = 256):
    """utils.py:58-80: batched search, returns (scores float32 [N, k], indices int64 [N, k]) as numpy arrays."""
    all_scores, all_indices = [], []
    batch_size = max(int(batch_size), int(getattr(index, "query_rows_per_pass", batch_size)))
    for i in range(0, len(query_embedding), batch_size):
        s, ix = index.search(query_embedding[i:i + batch_size], topk)
        all_scores.append(s)
        all_indices.append(ix)
    return torch.cat(all_scores).cpu().numpy(), torch.cat(all_indices).cpu().numpy()


def compute_metrics(preds, preds_scores, labels, cutoffs: Sequence[int] = (1, 5, 10, 20, 100)):
    """MRR / Recall / AUC / nDCG at cutoffs with the reference's definitions (utils.py:87-153), computed on ONE boolean hit
    matrix instead of per-query Python loops:

      hit[i, j]  = preds[i][j] is one of labels[i]
      MRR@c      = mean_i ( 1 / r_i  if r_i <= c else 0 ),  r_i = 1-based rank of the first hit of query i
      Recall@c   = mean_i ( #distinct ids of preds[i][:c] that are labels / max(min(c, len(preds[i]), len(labels[i])), 1) )
                   (the reference's non-standard denominator; len(labels[i]) counts duplicates, the numerator does not)
      AUC@c      = roc_auc_score over the flattened first c columns of (hit, score)  ("naive AUC")
      nDCG@c     = sklearn ndcg_score(hit, score, k=c)

    Returns a dict in the reference's key order: all MRR@, then Recall@, AUC@, nDCG@.  preds may be ragged for MRR / Recall;
    AUC / nDCG need a rectangular [N, k] prediction matrix, as in the reference."""
    import warnings
    from sklearn.metrics import ndcg_score, roc_auc_score
    n = len(preds)
    if n != len(labels):
        raise AssertionError(f"compute_metrics: {n} prediction rows but {len(labels)} label rows")
    cut = np.asarray(list(cutoffs), dtype=np.int64)
    plen = np.fromiter((len(r) for r in preds), dtype=np.int64, count=n)
    llen = np.fromiter((len(r) for r in labels), dtype=np.int64, count=n)
    width = int(plen.max()) if n else 0
    if n and int(plen.min()) < int(cut.max()):
        warnings.warn(f"compute_metrics: some queries have fewer than {int(cut.max())} predictions", stacklevel=2)

    # ids of any hashable / comparable kind -> dense codes; (row, code) -> one int64 key per entry
    flat_p = np.concatenate([np.asarray(r).reshape(-1) for r in preds]) if width else np.zeros(0, dtype=np.int64)
    flat_l = np.concatenate([np.asarray(r).reshape(-1) for r in labels]) if llen.sum() else flat_p[:0]
    _, codes = np.unique(np.concatenate([flat_p, flat_l]), return_inverse=True)
    ncode = int(codes.max()) + 1 if codes.size else 1
    prow = np.repeat(np.arange(n), plen)
    pkey = prow * ncode + codes[:flat_p.size]
    lkey = np.repeat(np.arange(n), llen) * ncode + codes[flat_p.size:]
    pcol = np.arange(flat_p.size) - np.repeat(np.cumsum(plen) - plen, plen)
    hit = np.zeros((n, width), dtype=bool)
    hit[prow, pcol] = np.isin(pkey, lkey)
    # first occurrence of an id inside its own row (a repeated prediction counts once towards Recall)
    order = np.argsort(pkey, kind="stable")
    dup = np.zeros(flat_p.size, dtype=bool)
    dup[order[1:]] = pkey[order[1:]] == pkey[order[:-1]]
    fresh = np.zeros((n, width), dtype=bool)
    fresh[prow, pcol] = ~dup

    metrics = {}
    rank = np.where(hit.any(1), hit.argmax(1) + 1, np.iinfo(np.int64).max) if width else np.full(n, np.iinfo(np.int64).max)
    rr = np.where(rank[:, None] <= cut[None, :], 1.0 / np.minimum(rank, 2 ** 40)[:, None], 0.0)          # [n, cutoffs]
    for c, v in zip(cut, rr.mean(0) if n else np.zeros(len(cut))):
        metrics[f"MRR@{int(c)}"] = v
    found = np.concatenate([np.zeros((n, 1), dtype=np.int64), np.cumsum(hit & fresh, axis=1)], 1)        # found[:, j]: in the first j
    upto = np.minimum(cut[None, :], plen[:, None])
    denom = np.maximum(np.minimum(upto, llen[:, None]), 1)
    rec = np.take_along_axis(found, upto, 1) / denom
    for c, v in zip(cut, rec.mean(0) if n else np.zeros(len(cut))):
        metrics[f"Recall@{int(c)}"] = v
    hard = hit.astype(int)
    sc = np.asarray(preds_scores)
    for c in cut:
        metrics[f"AUC@{int(c)}"] = roc_auc_score(hard[:, :c].ravel(), sc[:, :c].ravel())
    for c in cut:
        metrics[f"nDCG@{int(c)}"] = ndcg_score(hard, sc, k=int(c))
    return metrics
