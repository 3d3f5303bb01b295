"""torch.autograd wrappers around the C ABI (include/rankpo_hip.h).

PyTorch is plumbing here: it owns device memory and streams; every computation of the scoring hot path is
done by librankpo_hip.so.  There is no fallback: tensors must live on a HIP device.
"""
from __future__ import annotations

import ctypes as C
import functools
import threading
from dataclasses import dataclass
from typing import NamedTuple

import torch

from . import _lib
from ._lib import (RPO_DT_BF16, RPO_DT_F16, RPO_DT_F32, RPO_LOSS_HINGE, RPO_LOSS_SIGMOID, RPO_NUM_METRICS, RPO_POOL_CLS,
                   RPO_POOL_LAST, RPO_TARGET_FIRST, RPO_TARGET_INBATCH, METRIC_KEYS, RankPOParams, check)

F_NORMALIZE_EPS = 1e-12  # torch.nn.functional.normalize default (modeling.py:236)


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return RPO_DT_F32
    if t.dtype == torch.bfloat16:
        return RPO_DT_BF16
    if t.dtype == torch.float16:     # scoring kernels only (pool / normalize, similarity + InfoNCE, RankPO, top-k): the reference's
        return RPO_DT_F16            # fp16 BGE setup (configs/ds_zero1_config_bge.json:2-11, modeling.py:453-454); f32 accumulation
    raise TypeError(f"rankpo_amd HIP kernels take float32, bfloat16 or float16 tensors, got {t.dtype}")


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("rankpo_amd scoring ops run only on a HIP device (no CPU fallback); "
                               f"got a tensor on {t.device}")


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------
# (1) pooling + normalisation
# ------------------------------------------------------------------------------------------------
class _PoolNormalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, mask, pool_mode, normalize, eps):
        _need_gpu(h, mask)
        lib = _lib.load()
        if h.dim() != 3:
            raise ValueError(f"last_hidden_state must be [N, L, d], got {tuple(h.shape)}")
        if h.stride(2) != 1:
            h = h.contiguous()
        N, L, d = h.shape
        if pool_mode == RPO_POOL_LAST:
            if mask is None or tuple(mask.shape) != (N, L):
                raise ValueError("attention_mask must be [N, L] for last-token pooling")
            mask = mask.to(torch.int64).contiguous()
        out = torch.empty((N, d), dtype=h.dtype, device=h.device)
        idx = torch.empty((N,), dtype=torch.int32, device=h.device)
        norm = torch.empty((N,), dtype=torch.float32, device=h.device)
        with torch.cuda.device(h.device):
            check(lib.rpo_pool_normalize_fwd(h.data_ptr(), h.stride(0), h.stride(1), _p(mask), N, L, d, _dt(h),
                                             pool_mode, int(normalize), eps, out.data_ptr(), idx.data_ptr(),
                                             norm.data_ptr(), _stream(h)), "rpo_pool_normalize_fwd")
        ctx.save_for_backward(out, idx, norm)
        ctx.meta = (N, L, d, int(normalize), eps)
        ctx.mark_non_differentiable(idx)
        return out, idx

    @staticmethod
    def backward(ctx, grad_out, _grad_idx):
        out, idx, norm = ctx.saved_tensors
        N, L, d, normalize, eps = ctx.meta
        lib = _lib.load()
        g = grad_out.contiguous()
        dh = torch.empty((N, L, d), dtype=out.dtype, device=out.device)   # written in full by the kernel
        with torch.cuda.device(out.device):
            check(lib.rpo_pool_normalize_bwd(g.data_ptr(), out.data_ptr(), idx.data_ptr(), norm.data_ptr(), N, L, d,
                                             _dt(out), normalize, eps, dh.data_ptr(), None, _stream(out)),
                  "rpo_pool_normalize_bwd")
        return dh, None, None, None, None


def pool_normalize(last_hidden_state, attention_mask, mode: str = "last", normalize: bool = True,
                   eps: float = F_NORMALIZE_EPS, return_index: bool = False):
    """modeling.py:224-236: last-token (mode='last') or CLS (mode='cls') pooling + optional F.normalize."""
    pm = {"last": RPO_POOL_LAST, "cls": RPO_POOL_CLS}[mode]
    out, idx = _PoolNormalize.apply(last_hidden_state, attention_mask, pm, normalize, eps)
    return (out, idx) if return_index else out


# ------------------------------------------------------------------------------------------------
# (2) similarity + InfoNCE
# ------------------------------------------------------------------------------------------------
def _workspace(lib, Q, P, d, dt, device):
    n = lib.rpo_infonce_workspace_bytes(Q, P, d, dt)
    return torch.empty((max(n, 256),), dtype=torch.uint8, device=device), n


_GEMM_BWD_MIN_PAIRS = 256 * 1024     # own-rows x columns above which the backward switches to dS + 2 GEMMs


class _InfoNCE(torch.autograd.Function):
    """loss, scores = f(q_local, p_local ; q_all, p_all).  q_all / p_all are the (possibly gathered) matrices the
    loss is computed on; rows [q_row0, +len(q_local)) / [p_row0, +len(p_local)) of them are q_local / p_local.
    Gradients flow to q_local / p_local only (modeling.py:374-377 semantics)."""

    @staticmethod
    def forward(ctx, q_local, p_local, q_all, p_all, temperature, target_mode, q_row0, p_row0):
        _need_gpu(q_all, p_all)
        lib = _lib.load()
        q_all = q_all.contiguous()
        p_all = p_all.contiguous()
        if q_all.dtype != p_all.dtype:
            raise TypeError("query and passage embeddings must share a dtype")
        Q, d = q_all.shape
        P = p_all.shape[0]
        dt = _dt(q_all)
        G = P // Q
        shape = (Q, P) if target_mode == RPO_TARGET_INBATCH else (Q, G)
        scores = torch.empty(shape, dtype=q_all.dtype, device=q_all.device)
        lse = torch.empty((Q,), dtype=torch.float32, device=q_all.device)
        loss = torch.empty((), dtype=torch.float32, device=q_all.device)
        ws, nws = _workspace(lib, Q, P, d, dt, q_all.device)
        with torch.cuda.device(q_all.device):
            check(lib.rpo_infonce_fwd(q_all.data_ptr(), p_all.data_ptr(), Q, P, d, dt, temperature, target_mode,
                                      scores.data_ptr(), lse.data_ptr(), loss.data_ptr(), ws.data_ptr(), nws,
                                      _stream(q_all)), "rpo_infonce_fwd")
        ctx.save_for_backward(q_all, p_all, scores, lse)
        ctx.meta = (Q, P, d, dt, temperature, target_mode, q_row0, q_local.shape[0], p_row0, p_local.shape[0])
        ctx.mark_non_differentiable(scores)
        return loss, scores

    @staticmethod
    def backward(ctx, grad_loss, _grad_scores):
        q_all, p_all, scores, lse = ctx.saved_tensors
        Q, P, d, dt, temperature, target_mode, q_row0, q_rows, p_row0, p_rows = ctx.meta
        lib = _lib.load()
        need_q, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gl = grad_loss.to(torch.float32).contiguous()
        if target_mode == RPO_TARGET_INBATCH and max(q_rows * P, p_rows * Q) >= _GEMM_BWD_MIN_PAIRS:
            # large problems: the HIP kernel writes dS (and dS^T); dq = dS p and dp = dS^T q are then two plain
            # GEMMs, which is what the vendor GEMM library is for (MFMA-bound, ~1.2 PFLOP/s through hipBLASLt)
            ds = torch.empty((q_rows, P), dtype=q_all.dtype, device=q_all.device) if need_q else None
            dst = torch.empty((p_rows, Q), dtype=q_all.dtype, device=q_all.device) if need_p else None
            with torch.cuda.device(q_all.device):
                check(lib.rpo_infonce_ds(scores.data_ptr(), lse.data_ptr(), gl.data_ptr(), Q, P, dt, temperature,
                                         q_row0, q_rows if need_q else 0, p_row0, p_rows if need_p else 0, _p(ds),
                                         _p(dst), _stream(q_all)), "rpo_infonce_ds")
            dq = _bwd_product(ds, p_all) if need_q else None
            dp = _bwd_product(dst, q_all) if need_p else None
            return dq, dp, None, None, None, None, None, None
        dq = torch.empty((q_rows, d), dtype=q_all.dtype, device=q_all.device) if need_q else None
        dp = torch.empty((p_rows, d), dtype=q_all.dtype, device=q_all.device) if need_p else None
        if need_q or need_p:
            with torch.cuda.device(q_all.device):
                check(lib.rpo_infonce_bwd(q_all.data_ptr(), p_all.data_ptr(), scores.data_ptr(), lse.data_ptr(),
                                          gl.data_ptr(), Q, P, d, dt, temperature, target_mode, q_row0, q_rows,
                                          p_row0, p_rows, _p(dq), _p(dp), None, 0, _stream(q_all)),
                      "rpo_infonce_bwd")
        return dq, dp, None, None, None, None, None, None


# The two products of the large backward: "hip" = the forward's own MFMA frame (rpo_sim_gemm_nt), "blaslt" = torch.matmul ->
# hipBLASLt (rounds 1-4), "auto" = whichever the sweep measured at least as fast (profiles/r05_sweep_fwd_bwd.md: the two meet at
# reductions of 16384 -- 2.106 vs 2.096 ms at 16384^2 x 2048, 3.657 vs 3.640 at x 4096 -- and the library wins below, where the
# hand-written path's five launches (dS, two transposes, two products) show: 0.252 vs 0.229 ms at 4096^2 x 4096).
INFONCE_BWD_GEMM = "auto"
INFONCE_BWD_HIP_MIN_K = 16384


def sim_gemm_nt(b, a):
    """b [M, K] a [N, K]^T -> [M, N] (bf16, both operands contiguous along K): sim_tile256_kernel's frame with a plain epilogue."""
    lib = _lib.load()
    M, K = b.shape
    N = a.shape[0]
    c = torch.empty((M, N), dtype=b.dtype, device=b.device)
    with torch.cuda.device(b.device):
        check(lib.rpo_sim_gemm_nt(a.data_ptr(), N, a.stride(0), b.data_ptr(), M, b.stride(0), K, c.data_ptr(), c.stride(0),
                                  _stream(b)), "rpo_sim_gemm_nt")
    return c


def sim_gemm_nt_takes(rows, K, d, ld_ds, ds_ptr=0, bf16=True) -> bool:
    """Whether `rpo_sim_gemm_nt` accepts dS [rows, K] (row stride ld_ds) x X^T [d, K] -> [rows, d]: the C entry point's own
    conditions (csrc/infonce.hip), restated so that the dispatch never hands it a problem it answers with RPO_ERR_UNSUPPORTED --
    bf16; a reduction that is a multiple of the 64-element K-step; 16-byte pieces (row strides % 8, aligned bases); and operands
    below 4 GiB each, because the kernel addresses its LDS-DMA pieces by 32-bit byte offsets (a dS of 32768 x 65536 bf16 is 4 GiB:
    `ds @ x_all` has to take it, as it did before the hand-written arm existed -- advisor, round 5)."""
    return bool(bf16 and K % 64 == 0 and d % 8 == 0 and ld_ds % 8 == 0 and ld_ds >= K and ds_ptr % 16 == 0
                and rows * ld_ds * 2 < 2 ** 32 and d * K * 2 < 2 ** 32 and rows > 0 and d > 0)


def _bwd_product(ds, x_all):
    """ds [rows, K] @ x_all [K, d]: dq = dS p_all or dp = dS^T q_all.  On the hand-written path the embeddings are transposed
    first (rpo_transpose: 2 K d bytes each way, ~1 % of the product's time at sweep sizes) so that both operands are contiguous
    along the reduction, the layout of the forward kernel's LDS-DMA staging."""
    K, d = x_all.shape
    want_hip = INFONCE_BWD_GEMM == "hip" or (INFONCE_BWD_GEMM == "auto" and K >= INFONCE_BWD_HIP_MIN_K)
    if (want_hip and ds.stride(1) == 1 and x_all.dtype == ds.dtype
            and sim_gemm_nt_takes(ds.shape[0], K, d, ds.stride(0), ds.data_ptr(), ds.dtype == torch.bfloat16)):
        return sim_gemm_nt(ds, transpose2d(x_all))
    return ds @ x_all


def infonce_loss(q_local, p_local, temperature: float, use_inbatch_neg: bool = True, q_all=None, p_all=None,
                 q_row0: int = 0, p_row0: int = 0):
    """modeling.py:292-314.  Returns (loss f32 scalar, temperature-scaled scores)."""
    mode = RPO_TARGET_INBATCH if use_inbatch_neg else RPO_TARGET_FIRST
    if q_all is None:
        q_all, p_all = q_local.detach(), p_local.detach()
    return _InfoNCE.apply(q_local, p_local, q_all, p_all, float(temperature), mode, int(q_row0), int(p_row0))


def similarity(q, p):
    """modeling.py:252 / :321 on 2-D inputs: q @ p.T in the storage dtype (no temperature, no loss)."""
    _need_gpu(q, p)
    lib = _lib.load()
    q = q.contiguous()
    p = p.contiguous()
    Q, d = q.shape
    P = p.shape[0]
    scores = torch.empty((Q, P), dtype=q.dtype, device=q.device)
    with torch.cuda.device(q.device):
        check(lib.rpo_infonce_fwd(q.data_ptr(), p.data_ptr(), Q, P, d, _dt(q), 1.0,
                                  RPO_TARGET_INBATCH, scores.data_ptr(), None, None, None, 0, _stream(q)),
              "rpo_infonce_fwd(eval)")
    return scores


# ------------------------------------------------------------------------------------------------
# (3) RankPO
# ------------------------------------------------------------------------------------------------
@dataclass
class RankPOConfig:
    beta: float = 0.1
    temperature: float = 1.0
    gamma_beta_ratio: float = 0.0
    label_smoothing: float = 0.0
    rankpo_weight: float = 1.0
    sft_weight: float = 0.0
    loss_type: str = "sigmoid"
    reference_free: bool = False

    def to_c(self) -> RankPOParams:
        if self.loss_type not in ("sigmoid", "hinge"):   # rankpo_trainer.py:563-566
            raise ValueError(f"Unknown loss type: {self.loss_type}. Should be one of ['sigmoid', 'hinge']")
        return RankPOParams(self.beta, self.temperature, self.gamma_beta_ratio, self.label_smoothing,
                            self.rankpo_weight, self.sft_weight,
                            RPO_LOSS_SIGMOID if self.loss_type == "sigmoid" else RPO_LOSS_HINGE,
                            int(bool(self.reference_free)))


class _RankPO(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, p, ref_chosen, ref_rejected, cfg: RankPOConfig):
        _need_gpu(q, p, ref_chosen, ref_rejected)
        lib = _lib.load()
        q = q.contiguous()
        p = p.contiguous()
        B, d = q.shape
        if p.shape[0] != 2 * B:
            raise ValueError(f"RankPO needs 2 passages (chosen, rejected) per query: got {p.shape[0]} for B={B}")
        dev = q.device
        f32 = dict(dtype=torch.float32, device=dev)
        scores = torch.empty((B, 2), **f32)
        losses = torch.empty((B,), **f32)
        loss = torch.empty((), **f32)
        metrics = torch.empty((RPO_NUM_METRICS,), **f32)
        dscores = torch.empty((B, 2), **f32)
        rc = None if ref_chosen is None else ref_chosen.to(torch.float32).contiguous()
        rr = None if ref_rejected is None else ref_rejected.to(torch.float32).contiguous()
        prm = cfg.to_c()
        with torch.cuda.device(dev):
            check(lib.rpo_rankpo_fwd(q.data_ptr(), p.data_ptr(), _p(rc), _p(rr), B, d, _dt(q), C.byref(prm),
                                     scores.data_ptr(), losses.data_ptr(), loss.data_ptr(), metrics.data_ptr(),
                                     dscores.data_ptr(), _stream(q)), "rpo_rankpo_fwd")
        ctx.save_for_backward(q, p, dscores)
        ctx.mark_non_differentiable(scores, losses, metrics)
        return loss, scores, losses, metrics

    @staticmethod
    def backward(ctx, grad_loss, *_):
        q, p, dscores = ctx.saved_tensors
        lib = _lib.load()
        B, d = q.shape
        need_q, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gl = grad_loss.to(torch.float32).contiguous()
        dq = torch.empty_like(q) if need_q else None
        dp = torch.empty_like(p) if need_p else None
        if need_q or need_p:
            with torch.cuda.device(q.device):
                check(lib.rpo_rankpo_bwd(q.data_ptr(), p.data_ptr(), dscores.data_ptr(), gl.data_ptr(), B, d,
                                         _dt(q), _p(dq), _p(dp), _stream(q)), "rpo_rankpo_bwd")
        return dq, dp, None, None, None


def rankpo_loss_metrics(q, p, cfg: RankPOConfig, ref_chosen=None, ref_rejected=None):
    """rankpo_trainer.py:458-520 on embeddings.  Returns (loss, scores[B,2] f32, losses[B], metrics[9] f32);
    `metrics` stays on the device (slot order = _lib.METRIC_KEYS) so that logging costs ONE host copy."""
    return _RankPO.apply(q, p, ref_chosen, ref_rejected, cfg)


# ------------------------------------------------------------------------------------------------
# (5) fused elementwise pieces of the Llama block (used by rankpo_amd/encoder.py on HIP tensors)
# ------------------------------------------------------------------------------------------------
def _swiglu_fwd(lib, gu, prod, rows, ff):
    es = gu.element_size()
    with torch.cuda.device(gu.device):
        check(lib.rpo_swiglu_fwd(gu.data_ptr(), gu.data_ptr() + ff * es, prod.data_ptr(), rows, ff, 2 * ff, ff, _dt(gu),
                                 _stream(gu)), "rpo_swiglu_fwd")
    return prod


LINEAR_TN = True      # input-gradient GEMMs against a transposed copy of the weight (`_LinearTN`); bench.py --no-linear-tn
WGRAD_MIXED = True    # weight-gradient GEMMs with the smaller operand transposed first (`wgrad`); bench.py --no-wgrad-mixed
SWIGLU_DGU_T = True   # ... and d(gate|up) transposed as well, for the gate|up weight gradient; bench.py --no-dgu-t
SWIGLU_DGU_T_DEFAULT_MAX_BYTES = 6 * 2 ** 30
SWIGLU_DGU_T_MAX_BYTES = SWIGLU_DGU_T_DEFAULT_MAX_BYTES   # the [2 ff, T] buffer is optional: taken up to this size (cfg 2: 5.1 GB; the Llama-3-8B
                                       # shape needs 13 GB and runs at 88 % of HBM on one GPU: a caller that KNOWS its headroom may raise it --
                                       # rankpo_amd.memory's plan (`gradient_checkpointing_enable()`) and bench.py's measured pre-size step do)
SWIGLU_PROD_T = True  # SwiGLU backward writes the recomputed product transposed for the down projection's weight gradient; bench.py --no-prod-t
WGRAD_SPLIT_T = 4     # chunks of the token reduction for the small-output weight gradients (0 / 1: one GEMM); bench.py --wgrad-split


def transpose2d(x):
    """x [R, C] (row stride free, unit column stride) -> contiguous [C, R], by the HBM-bound HIP kernel (`.t().contiguous()`
    moves 0.35 TB/s on the encoder's operand shapes)."""
    _need_gpu(x)
    lib = _lib.load()
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("transpose2d: a 2-D tensor with contiguous rows")
    R, C_ = x.shape
    out = torch.empty((C_, R), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.rpo_transpose(x.data_ptr(), out.data_ptr(), R, C_, x.stride(0), R, _dt(x), _stream(x)), "rpo_transpose")
    return out


WGRAD_DY_T_HITS = 0   # weight gradients that used a transposed copy of dY left by the kernel that produced dY (tests read it)


def wgrad(dy2, x2, dy_t=None):
    """dW [n, k] = dy2[T, n]^T x2[T, k] (reduction over the tokens).  hipBLASLt's kernels for two operands that are both
    strided along the reduction reach 0.9-1.2 PFLOP/s on the block's shapes, with ONE operand contiguous along it 1.36-1.39
    (tools/probe_wgrad.py): when one operand is at most half of the other (gate|up: x, down: dy), a transposed copy of the
    smaller one (0.25 ms, HBM-bound) buys 0.7-1.1 ms of GEMM time; at 2 : 3 (q|k|v) the copy costs what it saves and at
    1 : 1 (o) autograd's layout is the fastest."""
    n, k = dy2.shape[1], x2.shape[1]
    if dy_t is not None and tuple(dy_t.shape) == (n, dy2.shape[0]) and dy_t.dtype == dy2.dtype and x2.stride(1) == 1:
        # the producer of dy (the SwiGLU backward) left its transposed copy [n, T]: both operands contiguous along the tokens
        global WGRAD_DY_T_HITS
        WGRAD_DY_T_HITS += 1
        return torch.nn.functional.linear(dy_t, transpose2d(x2))                    # [n, T] x [k, T]^T -> [n, k]
    if WGRAD_MIXED and dy2.is_cuda and dy2.dtype == torch.bfloat16 and dy2.stride(1) == 1 and x2.stride(1) == 1:
        if n >= 2 * k:
            return dy2.t() @ transpose2d(x2).t()          # x is the smaller operand
        if k >= 2 * n:
            return transpose2d(dy2) @ x2                   # dy is the smaller operand
        # Round 4: q|k|v [3072, 2048] and o [2048, 2048] are 96 / 64 output tiles of 256 x 256 on 256 CUs, and hipBLASLt runs
        # them at 0.78-1.16 PFLOP/s in EVERY operand layout (tools/probe_wgrad.py).  The token reduction cut into S chunks as
        # ONE batched GEMM with float32 partial products, summed afterwards, fills the chip: 1.88 -> 1.71 ms and 1.29 -> 1.12 ms
        # at T = 151 552 (tools/probe_wgrad_splitk.py); the float32 partials are rounded to bf16 once, as the single GEMM's
        # accumulator is (relative difference to it 8e-5: summation order).
        T, S = dy2.shape[0], WGRAD_SPLIT_T
        if S > 1 and T >= 32768 and T % S == 0 and n * k <= 8 * 1024 * 1024 and dy2.is_contiguous() and x2.is_contiguous():
            if _bmm_f32_out_ok(dy2.device):
                part = torch.bmm(dy2.view(S, T // S, n).transpose(1, 2), x2.view(S, T // S, k), out_dtype=torch.float32)
                return part.sum(0).to(dy2.dtype)
    return dy2.t() @ x2


_BMM_F32_OUT = {}


def _bmm_f32_out_ok(device) -> bool:
    """Does this torch / backend run `bmm(bf16, bf16, out_dtype=float32)`?  Probed ONCE per device on a tiny problem, catching
    whatever it raises (a torch without the keyword: TypeError; a backend that rejects bf16 -> f32: RuntimeError /
    NotImplementedError); the split weight gradient is gated on the cached answer instead of a try / except per call."""
    key = str(device)
    if key not in _BMM_F32_OUT:
        try:
            a = torch.ones(2, 8, 16, dtype=torch.bfloat16, device=device)
            r = torch.bmm(a.transpose(1, 2), a, out_dtype=torch.float32)
            _BMM_F32_OUT[key] = bool(r.dtype == torch.float32 and float(r[0, 0, 0]) == 8.0)
        except Exception:
            _BMM_F32_OUT[key] = False
    return _BMM_F32_OUT[key]


def _wt(w):
    """W^T as a contiguous matrix (operand of the input-gradient GEMM in the forward's layout)."""
    return transpose2d(w) if w.is_cuda and w.dtype in (torch.bfloat16, torch.float16, torch.float32) and w.stride(1) == 1 else w.t().contiguous()


class _LinearTN(torch.autograd.Function):
    """y = x W^T (W [n, k], the nn.Linear layout) whose input gradient dX = dY W is computed against a transposed COPY of W:
    hipBLASLt's kernels for that operand layout (both operands contiguous along the reduction, the forward's layout) run
    12-18 % faster than the ones torch's own backward gets (1.23-1.58 vs 1.11-1.36 PFLOP/s on the block's four shapes,
    tools/probe_dgrad.py); the weight gradient goes through `wgrad`."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return torch.nn.functional.linear(x, w)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.nn.functional.linear(dy, _wt(w))
        if ctx.needs_input_grad[1]:
            # `_rpo_transposed`: set on the gradient tensor by the kernel that produced it (`_SwiGLUDown.backward`); the attribute
            # travels with the tensor object through the autograd engine.  It is STAMPED with the tensor's version counter and
            # data pointer at production: were the projection output ever given a second consumer (or a hook that edits the
            # gradient in place), the engine would accumulate into this very tensor object and the transposed copy would be
            # stale -- the stamp no longer matches and the slower layout runs on the tensor as it is (advisor, round 4).  A miss
            # costs time, a false match cannot happen.
            dy_t = None
            tag = getattr(dy, "_rpo_transposed", None)
            if tag is not None and tag[1] == dy._version and tag[2] == dy.data_ptr():
                dy_t = tag[0]
            dw = wgrad(dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1]), dy_t)
        return dx, dw


def linear(x, w, bias=None):
    """F.linear; on HIP tensors without bias and with gradients enabled the backward uses `_LinearTN`."""
    if (bias is None and x.is_cuda and torch.is_grad_enabled() and (x.requires_grad or w.requires_grad)
            and LINEAR_TN):
        return _LinearTN.apply(x, w)
    return torch.nn.functional.linear(x, w, bias)


class recomputing:
    """Context of a checkpointed block's RECOMPUTATION (torch.utils.checkpoint's `context_fn`, encoder._run_layers): what a block
    computes last -- the SwiGLU product and the down projection, `_SwiGLUDown.forward` -- feeds nothing the backward reads (the
    checkpoint keeps the recomputed SAVED tensors and drops the block's outputs), so under this context that forward returns an
    uninitialised tensor of the right shape instead: one [tokens, ff] pass and one GEMM per checkpointed block and step less
    (Llama-3-8B at 206 848 tokens: 17 of a block's ~56 ms of recomputation)."""
    _tls = threading.local()      # per thread: autograd runs the recomputation on ITS thread, and only that thread's forwards are recomputations

    @staticmethod
    def active():
        return getattr(recomputing._tls, "depth", 0) > 0

    def __enter__(self):
        recomputing._tls.depth = getattr(recomputing._tls, "depth", 0) + 1
        return self

    def __exit__(self, *exc):
        recomputing._tls.depth -= 1
        return False


class _SwiGLUDown(torch.autograd.Function):
    """y = (silu(g) * u) @ W^T with gu = [g | u] the output of ONE fused gate|up projection.  Saves gu and W only: the
    [tokens, ff] product (the largest activation of the block) is recomputed by one fused pass in backward."""

    @staticmethod
    def forward(ctx, gu, weight, last_in_block=False):
        lib = _lib.load()
        gu = gu.contiguous()
        ff = gu.shape[-1] // 2
        rows = gu.numel() // (2 * ff)
        ctx.save_for_backward(gu, weight)
        # the output of a recomputed block is never read -- IF this call is what the checkpointed function computes last (the caller
        # says so: `last_in_block`, advisor round 5; a thread-wide "a recomputation is running" alone would also hit an MLP in the
        # middle of a longer checkpointed segment).  POISON_SKIPPED_OUTPUT (tests): NaNs instead of uninitialised memory, so that
        # anything that does read it shows.
        if SKIP_RECOMPUTED_OUTPUT and last_in_block and recomputing.active():
            out = torch.empty(gu.shape[:-1] + (weight.shape[0],), dtype=gu.dtype, device=gu.device)
            return out.fill_(float("nan")) if POISON_SKIPPED_OUTPUT else out
        prod = _swiglu_fwd(lib, gu, torch.empty(gu.shape[:-1] + (ff,), dtype=gu.dtype, device=gu.device), rows, ff)
        return torch.nn.functional.linear(prod, weight)

    @staticmethod
    def backward(ctx, dy):
        gu, weight = ctx.saved_tensors
        lib = _lib.load()
        dy = dy.contiguous()
        ff = gu.shape[-1] // 2
        rows = gu.numel() // (2 * ff)
        es = gu.element_size()
        # dprod first; ONE pass then reads g, u, dprod and writes dg, du AND the recomputed product over dprod (6 units of
        # [T, ff] traffic instead of 3 + 5 for a separate recompute), which the weight gradient consumes afterwards
        if LINEAR_TN:
            dprod = torch.nn.functional.linear(dy, _wt(weight))   # dy @ W through the faster operand layout (see _LinearTN)
        else:
            dprod = dy @ weight
        dgu = torch.empty_like(gu)                            # [dg | du]: the gradient of the fused projection output
        want_dw = ctx.needs_input_grad[1]
        dy2 = dy.reshape(-1, dy.shape[-1])
        n = dy2.shape[1]
        # Round 4: the recomputed product written TRANSPOSED [ff, T], so that the weight gradient dW [n, ff] = dY^T prod has BOTH
        # operands contiguous along the token reduction (hipBLASLt: 1.57 instead of 1.37 PFLOP/s on the down projection's shape,
        # tools/probe_wgrad.py) -- the same bytes stored, through an LDS tile (csrc/encoder_ops.hip, swiglu_bwd_t_kernel)
        if (want_dw and SWIGLU_PROD_T and WGRAD_MIXED and gu.dtype == torch.bfloat16 and ff >= 2 * n and rows >= 4096
                and rows % 8 == 0):
            prod_t = torch.empty((ff, rows), dtype=gu.dtype, device=gu.device)
            # ... and d(gate|up) ALSO transposed (an extra store, unlike the product) for the weight gradient of the fused gate|up
            # projection, the last one with a strided operand: 7.49 -> 6.34 ms of GEMM for ~0.9 ms of kernel; handed over as an
            # attribute of the gradient tensor (the next backward node is that projection's `_LinearTN`).  Skipped when the
            # [2 ff, T] buffer is large (cfg 5 runs at 88 % of HBM).
            dgu_t = None
            if SWIGLU_DGU_T and 2 * ff * rows * es <= SWIGLU_DGU_T_MAX_BYTES:
                dgu_t = torch.empty((2 * ff, rows), dtype=gu.dtype, device=gu.device)
            with torch.cuda.device(gu.device):
                check(lib.rpo_swiglu_bwd_t(gu.data_ptr(), gu.data_ptr() + ff * es, dprod.data_ptr(), dgu.data_ptr(),
                                           dgu.data_ptr() + ff * es, prod_t.data_ptr(), _p(dgu_t), rows, ff, 2 * ff, ff, 2 * ff,
                                           rows, _dt(gu), _stream(gu)), "rpo_swiglu_bwd_t")
            if dgu_t is not None:                             # stamped AFTER the kernel wrote dgu (version and pointer as handed on)
                dgu._rpo_transposed = (dgu_t, dgu._version, dgu.data_ptr())
            del dprod, dgu_t
            return dgu, torch.nn.functional.linear(transpose2d(dy2), prod_t), None      # [n, T] x [ff, T]^T -> [n, ff]
        with torch.cuda.device(gu.device):
            check(lib.rpo_swiglu_bwd(gu.data_ptr(), gu.data_ptr() + ff * es, dprod.data_ptr(), dgu.data_ptr(),
                                     dgu.data_ptr() + ff * es, dprod.data_ptr() if want_dw else None, rows, ff, 2 * ff,
                                     ff, 2 * ff, ff, _dt(gu), _stream(gu)), "rpo_swiglu_bwd")
        dW = None
        if want_dw:
            prod = dprod                                      # overwritten in place by the kernel
            dW = wgrad(dy2, prod.reshape(-1, ff))
        return dgu, dW, None


def swiglu_down(gu, weight, last_in_block: bool = False):
    """last_in_block: this product is the LAST thing the enclosing (possibly checkpointed) function computes, i.e. nothing that
    saves tensors for backward consumes it inside that function; only then may a recomputation skip it (`recomputing`)."""
    return _SwiGLUDown.apply(gu, weight, bool(last_in_block))


class fp16_native:
    """Context of a packed no-grad pass of an fp16 LlamaEncoder that opted in to the fp16 row kernels (encoder.LLAMA_FP16_NATIVE /
    LlamaEncoder.native_fp16): inside it, and only with grad mode off, `fused_encoder_ops_ok` / `fused_norm_ok` accept fp16 HIP
    tensors, which sends RMSNorm, RoPE and SwiGLU to the fp16 forward instantiations of rpo_add_rmsnorm_fwd / rpo_rope /
    rpo_swiglu_fwd (there are no fp16 backward entries).  Outside it an fp16 tensor is refused as before."""
    _tls = threading.local()      # per thread, as `recomputing`

    @staticmethod
    def active():
        return getattr(fp16_native._tls, "depth", 0) > 0

    def __enter__(self):
        fp16_native._tls.depth = getattr(fp16_native._tls, "depth", 0) + 1
        return self

    def __exit__(self, *exc):
        fp16_native._tls.depth -= 1
        return False


def _fp16_rows_ok(x) -> bool:
    return x.dtype == torch.float16 and x.is_cuda and fp16_native.active() and not torch.is_grad_enabled()


def fused_encoder_ops_ok(x, head_dim=None) -> bool:
    if _fp16_rows_ok(x):
        return head_dim is None or (head_dim % 2 == 0 and (head_dim // 2) % 8 == 0)
    if not x.is_cuda or x.dtype not in (torch.float32, torch.bfloat16):
        return False
    v = 8 if x.dtype == torch.bfloat16 else 4
    return head_dim is None or (head_dim % 2 == 0 and (head_dim // 2) % v == 0)


class _AddRMSNorm(torch.autograd.Function):
    """(x, delta, w) -> (x_new, y) with x_new = x + delta, y = rmsnorm(x_new) * w; delta may be None (then only y is
    returned).  One HIP pass forward, one backward (which also folds in the gradient arriving on x_new)."""

    @staticmethod
    def forward(ctx, x, delta, weight, eps):
        lib = _lib.load()
        x = x.contiguous()
        d = x.shape[-1]
        rows = x.numel() // d
        y = torch.empty_like(x)
        rstd = torch.empty((rows,), dtype=torch.float32, device=x.device)
        x_new = torch.empty_like(x) if delta is not None else x
        if delta is not None:
            delta = delta.contiguous()
        with torch.cuda.device(x.device):
            check(lib.rpo_add_rmsnorm_fwd(x.data_ptr(), _p(delta), weight.data_ptr(), eps, _p(x_new if delta is not None else None),
                                          y.data_ptr(), rstd.data_ptr(), rows, d, _dt(x), _stream(x)), "rpo_add_rmsnorm_fwd")
        ctx.save_for_backward(x_new, weight, rstd)
        ctx.has_delta = delta is not None
        if delta is None:
            return y
        return x_new, y

    @staticmethod
    def backward(ctx, *grads):
        x_new, weight, rstd = ctx.saved_tensors
        lib = _lib.load()
        if ctx.has_delta:
            dres, dy = grads
        else:
            dres, dy = None, grads[0]
        d = x_new.shape[-1]
        rows = x_new.numel() // d
        if dy is None:                      # only the residual output was used
            return dres, (dres if ctx.has_delta else None), None, None
        dy = dy.contiguous()
        dres = None if dres is None else dres.contiguous()
        dx = torch.empty_like(x_new)
        nw = lib.rpo_add_rmsnorm_waves(rows)
        dwp = torch.empty((nw, d), dtype=torch.float32, device=x_new.device)
        with torch.cuda.device(x_new.device):
            check(lib.rpo_add_rmsnorm_bwd(dy.data_ptr(), x_new.data_ptr(), weight.data_ptr(), rstd.data_ptr(), _p(dres),
                                          dx.data_ptr(), dwp.data_ptr(), rows, d, _dt(x_new), _stream(x_new)),
                  "rpo_add_rmsnorm_bwd")
        dw = dwp.sum(0).to(weight.dtype) if ctx.needs_input_grad[2] else None
        return dx, (dx if ctx.has_delta else None), dw, None


def add_rmsnorm(x, delta, weight, eps):
    """Returns (x + delta, rmsnorm(x + delta) * weight); with delta None returns (x, rmsnorm(x) * weight)."""
    if delta is None:
        return x, _AddRMSNorm.apply(x, None, weight, eps)
    return _AddRMSNorm.apply(x, delta, weight, eps)


def fused_norm_ok(x) -> bool:
    if _fp16_rows_ok(x):
        return x.shape[-1] % 8 == 0 and x.shape[-1] // 8 <= 64 * 8
    if not x.is_cuda or x.dtype not in (torch.float32, torch.bfloat16):
        return False
    v = 8 if x.dtype == torch.bfloat16 else 4
    d = x.shape[-1]
    return d % v == 0 and d // v <= 64 * 8


class _Rope(torch.autograd.Function):
    """In-place rotary embedding of the first `heads` heads of every row of a projection output x [..., row_len]
    (x is the fresh output of a Linear -- e.g. the fused q|k|v projection with heads = n_q + n_kv -- nothing else reads
    it).  cos / sin: f32 [period, head_dim / 2]; flat row r uses table row r % period."""

    @staticmethod
    def forward(ctx, x, cos, sin, heads, head_dim, grad_inplace):
        lib = _lib.load()
        row_len = x.shape[-1]
        rows = x.numel() // row_len
        with torch.cuda.device(x.device):
            check(lib.rpo_rope(x.data_ptr(), x.data_ptr(), row_len, cos.data_ptr(), sin.data_ptr(), rows, heads,
                               head_dim, cos.shape[0], _dt(x), 0, _stream(x)), "rpo_rope")
        ctx.mark_dirty(x)
        ctx.save_for_backward(cos, sin)
        ctx.meta = (heads, head_dim, grad_inplace)
        return x

    @staticmethod
    def backward(ctx, g):
        cos, sin = ctx.saved_tensors
        heads, head_dim, grad_inplace = ctx.meta
        lib = _lib.load()
        g = g.contiguous()
        row_len = g.shape[-1]
        rows = g.numel() // row_len
        # grad_inplace: the caller guarantees that the incoming gradient is a private buffer (the encoder's is: the attention
        # backward's fresh d(q|k|v)), so the inverse rotation runs in place and the columns beyond the rotated heads (the v
        # part of a fused projection) simply stay; otherwise they are carried over by a copy (1.6 GB per block on cfg 2).
        if grad_inplace:
            out = g
        else:
            out = torch.empty_like(g) if heads * head_dim == row_len else g.clone()
        with torch.cuda.device(g.device):
            check(lib.rpo_rope(g.data_ptr(), out.data_ptr(), row_len, cos.data_ptr(), sin.data_ptr(), rows, heads,
                               head_dim, cos.shape[0], _dt(g), 1, _stream(g)), "rpo_rope(bwd)")
        return out, None, None, None, None, None


def rope_(x, cos, sin, heads, head_dim, grad_inplace: bool = False):
    if not x.is_contiguous():
        raise ValueError("rope_ needs the contiguous output of the projection")
    return _Rope.apply(x, cos, sin, heads, head_dim, grad_inplace)


# ------------------------------------------------------------------------------------------------
# (6) causal variable-length flash attention, head_dim 64 (encoder side)
# ------------------------------------------------------------------------------------------------
def attn_tile_table(lens, device, num_heads: int = 0, num_kv_heads: int = 0, block_m: int = 128, heads_per_block: int = 1):
    """The query-tile work list of the forward and dQ kernels (block = 128 queries of one (sequence, head)).

    num_heads == 0: int32 [ntiles, 2] = (sequence id, first query row), heaviest (latest) tiles first; the kernels run one
    block per (entry, head).
    num_heads > 0 (what the encoder uses): int32 [n, 3] = (sequence id, first query row, head) dealt to the 8 XCDs -- the
    kernels give the blocks b, b + 8, ... (one XCD under round-robin dispatch) the (b % 8)-th eighth of the list, in order.
    The (sequence, kv head) groups go round-robin, longest sequence first, to the eighths (with 8 kv heads: XCD x gets kv head
    x of every sequence, so the eighths are equal by construction); inside an eighth a group's tiles follow each other, latest
    (heaviest) first, its q heads interleaved: the blocks an XCD runs at one time stream the SAME K / V rows through its L2.
    Eighths are padded to equal length with entries the kernels skip (first query row 2^30)."""
    import numpy as np
    if num_heads <= 0:
        tiles = [(s, q0) for s, n in enumerate(lens) for q0 in range(0, n, block_m)]
        tiles.sort(key=lambda t: -t[1])
        return torch.tensor(tiles, dtype=torch.int32).to(device, non_blocking=True)
    H = num_kv_heads if num_kv_heads > 0 else num_heads
    rep = num_heads // H
    if rep % heads_per_block:
        raise ValueError("attn_tile_table: heads_per_block must divide the q heads per kv head")
    lens_np = np.asarray(lens, dtype=np.int64)
    order = np.argsort(-lens_np, kind="stable")                       # sequences, longest first
    nt_seq = (lens_np[order] + block_m - 1) // block_m                   # query tiles per sequence (rank order)
    gid = np.arange(len(order) * H)                                      # group = (rank, kv head), dealt round-robin
    chunks = []
    for x in range(8):
        g = gid[x::8]
        rank, hk = g // H, g % H
        nt = nt_seq[rank]
        tot = int(nt.sum())
        gi = np.repeat(np.arange(len(g)), nt)                            # group index of every tile
        pos = np.arange(tot) - np.repeat(np.cumsum(nt) - nt, nt)
        q0 = (nt[gi] - 1 - pos) * block_m                                # latest tile of the group first
        seq = order[rank][gi]
        nb = rep // heads_per_block                                       # blocks per (tile, kv head): each serves heads_per_block q heads
        e = np.stack([np.repeat(seq, nb), np.repeat(q0, nb),
                      np.repeat(hk[gi] * rep, nb) + np.tile(np.arange(nb) * heads_per_block, tot)], 1).astype(np.int32)
        chunks.append(e)
    per = max(len(c) for c in chunks)
    pad = np.array([[0, 1 << 30, 0]], dtype=np.int32)
    out = [np.concatenate([c, np.repeat(pad, per - len(c), 0)], 0) for c in chunks]
    return torch.from_numpy(np.concatenate(out, 0)).to(device, non_blocking=True)


# head dims whose forward runs the one-wave-per-SIMD kernel by default where the head grouping allows.  The kernel exists for 64 as
# well (same source, fa_fwd64w_kernel; tests cover it) and LOSES there: 0.280 against 0.313 of the MFMA peak for fa_fwd_kernel on
# the cfg-2 passage batch (same run) -- head_dim 64 has half the matrix work per exponential, its loop is bound by the vector
# instructions' issue slots, and a second wave per SIMD fills what one wave leaves at barriers and LDS waits
# (profiles/r05_fa_fwd128w_ladder.md).
FWD_ONE_WAVE_HEAD_DIMS = (128,)
SKIP_RECOMPUTED_OUTPUT = True   # see `recomputing`; False: the A/B arm of `bench.py --recompute-output`
POISON_SKIPPED_OUTPUT = False   # tests: a skipped output is filled with NaN instead of left uninitialised


def attn_fwd_tile_table(lens, device, num_heads: int, num_kv_heads: int, head_dim: int, force: bool = False):
    """The FORWARD kernel's own work list where it has one: a head_dim of FWD_ONE_WAVE_HEAD_DIMS (force: 64 or 128) with a multiple
    of 4 q heads per kv head -> entries of 64 queries x 4 q heads (`attn_tile_table(..., block_m=64, heads_per_block=4)`; pass it as
    `fwd_tiles`, the forward then runs with q_block = 64: the one-wave-per-SIMD kernels); otherwise None (the forward walks the
    128-row list the dQ kernel walks)."""
    H = num_kv_heads if num_kv_heads > 0 else num_heads
    if head_dim not in ((64, 128) if force else FWD_ONE_WAVE_HEAD_DIMS) or num_heads <= 0 or num_heads % H or (num_heads // H) % 4:
        return None
    return attn_tile_table(lens, device, num_heads, num_kv_heads, block_m=64, heads_per_block=4)


def _check_rope_tables(rope, hd, who):
    rc, rs = rope
    if (rc.dtype != torch.float32 or rs.dtype != torch.float32 or rc.shape != rs.shape or rc.dim() != 2
            or rc.shape[1] * 2 != hd or not rc.is_contiguous() or not rs.is_contiguous()):
        raise ValueError(f"{who}: rope must be (cos, sin), contiguous f32 [period, head_dim / 2]")


def _rope_args(rope):
    """(cos pointer, sin pointer, period) of the C entries' rope arguments; rope = (cos, sin) or None."""
    return (None, None, 0) if rope is None else (rope[0].data_ptr(), rope[1].data_ptr(), rope[0].shape[0])


def _fwd_work(tiles, fwd_tiles):
    """(work list, its q_block) of the forward: its own list of 64-query entries where it has one, else the 128-row list."""
    return (tiles, 128) if fwd_tiles is None else (fwd_tiles, 64)


def flash_attn_varlen_fwd(q, k, v, cu_seqlens, tiles, scale, padded_lse_len: int = 0, num_seqs: int = 0, rope=None, q_block: int = 128,
                          want_lse: bool = True):
    """q [T, nh, hd], k / v [T, nkv, hd], hd = 64 or 128 (last two dims contiguous, token stride free); returns
    (out [T, nh, hd] bf16, lse f32: [nh, T], or [num_seqs, nh, padded_lse_len] when padded_lse_len > 0; None with
    want_lse=False: the forward-only entry, no row statistics are allocated or written).  rope = (cos, sin),
    f32 [period, hd / 2]: q arrives UN-rotated and the kernel rotates it IN PLACE (k must arrive rotated), see the header.
    q_block = the query rows per entry of `tiles`: 128, or 64 for a list from `attn_fwd_tile_table` (entries of 64 queries x 4 q
    heads: the one-wave-per-SIMD forward)."""
    lib = _lib.load()
    if rope is not None:
        _check_rope_tables(rope, q.shape[-1], "flash_attn_varlen_fwd")
    T, nh, hd = q.shape
    nkv = k.shape[1]
    if (q.dtype != torch.bfloat16 or hd not in (64, 128) or q.stride(2) != 1 or q.stride(1) != hd or k.stride(1) != hd
            or v.stride(1) != hd):
        raise ValueError("flash_attn_varlen_fwd: bf16, head_dim 64 or 128, heads contiguous inside a token row")
    out = torch.empty((T, nh, hd), dtype=q.dtype, device=q.device)
    if not want_lse:
        lse = None
    elif padded_lse_len > 0:
        lse = torch.zeros((num_seqs, nh, padded_lse_len), dtype=torch.float32, device=q.device)
    else:
        lse = torch.empty((nh, T), dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device):
        check(lib.rpo_flash_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0), v.stride(0),
                                     cu_seqlens.data_ptr(), tiles.data_ptr(), tiles.shape[0], tiles.shape[1], T, nh, nkv, hd, scale,
                                     out.data_ptr(), nh * hd, _p(lse), padded_lse_len, *_rope_args(rope), q_block, _stream(q)),
              "rpo_flash_attn_fwd")
    return out, lse


ATTN_KEY_BLOCK_HD128 = 128   # keys per block of the head_dim-128 dK/dV kernel
ATTN_KEY_BLOCK = 256     # keys per entry of the dK/dV work list (256: one-wave-per-SIMD kernel; 64: the 8-wave kernel)
# dK/dV schedule.  False: heaviest blocks of every XCD's eighth first, ascending sweep (round 1).  True: the key blocks of a
# (sequence, kv head) side by side on one XCD, all sweeping the query slices DOWNWARDS from the last one, so that the group's Q / dO
# slices are fetched from HBM once and served from that XCD's L2 to the other blocks.  Measured INSIDE the training step, same box
# (`bench.py --dkdv-heaviest-first` / `--dkdv-tail f`): head_dim 64 heaviest-first 7.93 ms per backward call, group order with a
# heaviest-first tail of 35 % / 60 % / ~100 % of the work 8.22 / 8.12 / 8.02; head_dim 128 heaviest-first 15.61, pure group order
# 14.75, tails of 20 % / 35 % 14.75 / 14.87.  (Stand-alone A/Bs on one batch of long rows, tools/fa_tiles_ab.py, ranked the 35 % tail
# first at both head dims -- 7.22 vs 7.64 ms at head_dim 128 -- and did not carry over to the step: the defaults follow the step.)
ATTN_SWEEP_DOWN = False
ATTN_SWEEP_DOWN_HD128 = True
ATTN_GROUP_TAIL = 0.0          # fraction of every XCD's work that runs heaviest-first BEHIND the group-ordered part (0: pure group order)


def attn_key_block(head_dim: int) -> int:
    """The keys per entry of the dK/dV work list that a head_dim (64 or 128) takes by default; read from the switches at call time."""
    return ATTN_KEY_BLOCK if head_dim == 64 else ATTN_KEY_BLOCK_HD128


def attn_key_tile_table(lens, device, num_kv_heads: int, block_n: int = ATTN_KEY_BLOCK, group_order=None):
    """int32 [n, 3] = (sequence id, kv head, first key of a key block): the key blocks of one (sequence, kv head) read the same
    Q / dO rows and are placed on one XCD by the kernel's block -> entry map.  block_n = 256 keys (default, the
    one-wave-per-SIMD dK/dV kernel at head_dim 64), 64 (the 8-wave kernel, A/B) or 128 (`ATTN_KEY_BLOCK_HD128`: the head_dim-128
    dK/dV kernel).  group_order: False = heaviest blocks of an XCD's eighth first, True = groups contiguous, a fraction f = groups
    contiguous with the last f of the eighth's work heaviest-first (an A/B knob: `ATTN_GROUP_TAIL`); whoever builds a table with another block_n than the default passes the same key_block to
    `flash_attn_varlen(_qkv)` as well -- it is an argument of the C call, not an environment switch."""
    if block_n not in (64, 128, 256):
        raise ValueError("attn_key_tile_table: block_n must be 64, 128 or 256")
    if group_order is None:
        group_order = (ATTN_GROUP_TAIL or True) if (ATTN_SWEEP_DOWN_HD128 if block_n == 128 else ATTN_SWEEP_DOWN) else False
    return _attn_key_tile_table(lens, device, num_kv_heads, block_n, group_order)


def _attn_key_tile_table(lens, device, num_kv_heads, block_n, group_order=False):
    import numpy as np
    if block_n == 64:
        parts = []
        for s, n in enumerate(lens):
            k0 = np.arange(0, n, block_n, dtype=np.int32)
            for h in range(num_kv_heads):
                parts.append(np.stack([np.full_like(k0, s), np.full_like(k0, h), k0], 1))
        return torch.from_numpy(np.concatenate(parts, 0)).to(device, non_blocking=True)
    # The kernel gives XCD x (blocks x, x + 8, ...) the x-th eighth of the table, in order.  One workgroup per CU and work
    # per block ~ (len - first key): deal the (sequence, kv head) groups, longest first, round-robin to the 8 XCDs (equal
    # eighths when there are 8 kv heads: one head of every sequence each; a group stays on ONE XCD), run the heaviest
    # blocks of an eighth first (the tail of a launch is one light block, not one heavy one), and pad the eighths to equal
    # length with entries whose first key lies past every sequence (such a workgroup exits at once).  Vectorised: this runs
    # on the host between the length sync and the first launch of every step.
    lens_np = np.asarray(lens, dtype=np.int64)
    order = np.argsort(-lens_np, kind="stable")                        # sequences, longest first
    nblk = (lens_np[order] + block_n - 1) // block_n                     # key blocks per sequence
    seq_rep = np.repeat(order, nblk)                                     # one row per (sequence, key block)
    first = np.concatenate([np.arange(0, n, block_n) for n in lens_np[order]]) if len(order) else np.zeros(0, np.int64)
    rank_rep = np.repeat(np.arange(len(order)), nblk)                    # rank of the sequence in the sorted order
    H = num_kv_heads
    seqs = np.tile(seq_rep, H)
    heads = np.repeat(np.arange(H), len(seq_rep))
    k0s = np.tile(first, H)
    xcd = (np.tile(rank_rep, H) * H + heads) % 8                          # group index (rank, head), dealt round-robin
    work = lens_np[seqs] - k0s
    chunks = []
    for x in range(8):
        sel = np.nonzero(xcd == x)[0]
        if not group_order:                     # heaviest blocks of the eighth first (round 1's schedule)
            sel = sel[np.argsort(-work[sel], kind="stable")]
        elif group_order is not True:           # a fraction f in (0, 1): group order, but the LAST f of the eighth's work heaviest first
            # (group order ends in one group's blocks of very unequal weight, with the XCD's other CUs idle behind the heavy
            # ones; the heaviest-first tail ends in the lightest blocks)
            csum = np.cumsum(work[sel])
            cut = int(np.searchsorted(csum, (1.0 - float(group_order)) * csum[-1])) if len(sel) else 0
            tail = sel[cut:]
            sel = np.concatenate([sel[:cut], tail[np.argsort(-work[tail], kind="stable")]])
        # group_order: index order = (kv head, sequence longest first, first key ascending): the key blocks of a
        # (sequence, kv head) stay next to each other, heaviest first (pairs with sweep_down=True of the kernel)
        chunks.append(np.stack([seqs[sel], heads[sel], k0s[sel]], 1).astype(np.int32))
    per = max(len(c) for c in chunks)
    pad = np.array([[0, 0, 1 << 30]], dtype=np.int32)
    out = [np.concatenate([c, np.repeat(pad, per - len(c), 0)], 0) for c in chunks]
    return torch.from_numpy(np.concatenate(out, 0)).to(device, non_blocking=True)


def flash_attn_varlen_bwd(q, k, v, out, dout, lse, cu_seqlens, q_tiles, k_tiles, scale, grads=None,
                          key_block: int = ATTN_KEY_BLOCK, sweep_down=None, rope=None, q_block: int = 128):
    """grads: optional preallocated (dq, dk, dv) [T, heads, hd] views with arbitrary token strides (e.g. the three column
    blocks of ONE fused d(q|k|v) buffer).  key_block: keys per entry of `k_tiles` (`attn_key_tile_table`'s block_n): 256 or 64 at
    head_dim 64, 128 at head_dim 128.  rope = (cos, sin), f32 [period, hd / 2] (the tables q and k were rotated with): dq / dk
    come back as the gradients w.r.t. the PRE-rotary q / k (inverse rotation in the kernels' epilogues, include/rankpo_hip.h).
    q_block = the query rows per entry of `q_tiles`: 128, or 64 (head_dim 64: a list of 64-query x 4-head entries,
    `attn_tile_table(..., block_m=64, heads_per_block=4)`, for the one-wave-per-SIMD dQ kernel)."""
    lib = _lib.load()
    if rope is not None:
        _check_rope_tables(rope, q.shape[-1], "flash_attn_varlen_bwd")
    if sweep_down is None:
        sweep_down = ATTN_SWEEP_DOWN_HD128 if key_block == 128 else ATTN_SWEEP_DOWN
    T, nh, hd = q.shape
    nkv = k.shape[1]
    dout = dout.contiguous()
    if grads is None:
        dq = torch.empty((T, nh, hd), dtype=q.dtype, device=q.device)
        dk = torch.empty((T, nkv, hd), dtype=q.dtype, device=q.device)
        dv = torch.empty((T, nkv, hd), dtype=q.dtype, device=q.device)
    else:
        dq, dk, dv = grads
        for t, h in ((dq, nh), (dk, nkv), (dv, nkv)):
            if t.shape != (T, h, hd) or t.stride(2) != 1 or t.stride(1) != hd or t.dtype != q.dtype:
                raise ValueError("flash_attn_varlen_bwd: gradient views must be [T, heads, head_dim] with contiguous heads")
    delta = torch.empty((2, nh, T), dtype=torch.float32, device=q.device)     # scratch: -delta | -lse / scale
    with torch.cuda.device(q.device):
        check(lib.rpo_flash_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr(),
                                     q.stride(0), k.stride(0), v.stride(0), out.stride(0), dout.stride(0),
                                     cu_seqlens.data_ptr(), q_tiles.data_ptr(), q_tiles.shape[0], q_tiles.shape[1], k_tiles.data_ptr(),
                                     k_tiles.shape[0], key_block, int(bool(sweep_down)), T, nh, nkv, hd, scale, lse.data_ptr(), delta.data_ptr(),
                                     dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dq.stride(0), dk.stride(0), dv.stride(0),
                                     *_rope_args(rope), q_block, _stream(q)), "rpo_flash_attn_bwd")
    return dq, dk, dv


class _FlashAttnVarlen(torch.autograd.Function):
    """Causal varlen attention, head_dim 64 / 128: hand-written HIP forward and backward (k_tiles given, built with the
    key_block that is passed along), or HIP forward + PyTorch's flash-attention backward op on the saved (out, padded lse) when
    k_tiles is None."""

    @staticmethod
    def forward(ctx, q, k, v, cu, tiles, k_tiles, max_len, scale, key_block, fwd_tiles=None):
        own_bwd = k_tiles is not None
        work, q_block = _fwd_work(tiles, fwd_tiles)
        out, lse = flash_attn_varlen_fwd(q, k, v, cu, work, scale, padded_lse_len=0 if own_bwd else max_len,
                                         num_seqs=cu.numel() - 1, q_block=q_block)
        ctx.save_for_backward(q, k, v, out, lse, cu, tiles, k_tiles if own_bwd else cu)
        ctx.meta = (max_len, scale, own_bwd, key_block)
        return out

    @staticmethod
    def backward(ctx, go):
        q, k, v, out, lse, cu, tiles, k_tiles = ctx.saved_tensors
        max_len, scale, own_bwd, key_block = ctx.meta
        if own_bwd:
            dq, dk, dv = flash_attn_varlen_bwd(q, k, v, out, go, lse, cu, tiles, k_tiles, scale, key_block=key_block)
        else:
            z = torch.zeros((), dtype=torch.int64, device=q.device)
            dq, dk, dv = torch.ops.aten._flash_attention_backward(go.contiguous(), q, k, v, out, lse, cu, cu, max_len,
                                                                  max_len, 0.0, True, z, z, scale=scale)
        return dq, dk, dv, None, None, None, None, None, None, None


def flash_attn_varlen(q, k, v, cu, tiles, max_len, scale, k_tiles=None, key_block: int = ATTN_KEY_BLOCK, fwd_tiles=None):
    if not (torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad)):
        # nothing will differentiate this: the forward kernel alone, no row statistics (no padded zero-filled lse per layer)
        work, q_block = _fwd_work(tiles, fwd_tiles)
        return flash_attn_varlen_fwd(q, k, v, cu, work, scale, want_lse=False, q_block=q_block)[0]
    return _FlashAttnVarlen.apply(q, k, v, cu, tiles, k_tiles, max_len, scale, key_block, fwd_tiles)


def _qkv_views(x, nh, nkv, hd):
    """The q | k | v column blocks of a fused buffer x [T, (nh + 2 nkv) * hd] as [T, heads, hd] views."""
    nq, nk = nh * hd, nkv * hd
    return (x[:, :nq].unflatten(1, (nh, hd)), x[:, nq:nq + nk].unflatten(1, (nkv, hd)),
            x[:, nq + nk:].unflatten(1, (nkv, hd)))


def _rope_heads_(x, cos, sin, head0, heads, hd):
    """`rpo_rope` in place on the heads [head0, head0 + heads) of every row of a fused buffer x [T, W]."""
    ptr = x.data_ptr() + head0 * hd * x.element_size()
    with torch.cuda.device(x.device):
        check(_lib.load().rpo_rope(ptr, ptr, x.shape[1], cos.data_ptr(), sin.data_ptr(), x.shape[0], heads, hd, cos.shape[0],
                                   _dt(x), 0, _stream(x)), "rpo_rope")


def _check_qkv(who, qkv, nh, nkv, hd, flat: bool = False):
    """head_dim 64 / 128 and a contiguous fused buffer of that width; flat: exactly [T, W], else leading dims are allowed."""
    if hd not in (64, 128):
        raise ValueError(f"{who}: head_dim must be 64 or 128")
    if (flat and qkv.dim() != 2) or qkv.shape[-1] != (nh + 2 * nkv) * hd or not qkv.is_contiguous():
        raise ValueError(f"{who}: qkv must be a contiguous [{'' if flat else '..., '}T, (nh + 2 nkv) * head_dim] tensor")


class _FlashAttnVarlenQKV(torch.autograd.Function):
    """Same attention on the output of ONE fused q|k|v projection, [T, (nh + 2 nkv) * hd] (hd = 64 or 128): the kernels read
    q / k / v as strided column blocks and the backward writes dq / dk / dv straight into the column blocks of one d(q|k|v)
    buffer, which is the operand of the projection's gradient GEMMs (no split / cat copies: the cat moved 1.6 GB per block on the
    cfg-2 passage tower).  cos / sin None: `qkv` arrives rotated.  cos / sin given: rotary embedding + attention as ONE autograd
    node on the FRESH projection output: forward = `rpo_rope` in place on its q and k heads, or with fold_forward on its k heads
    only, then the attention forward, which rotates (and writes back) the q block it loads anyway; backward = the attention
    backward with the INVERSE rotation folded into the dQ / dK epilogues (f32, before the one rounding to bf16), so d(q|k|v) comes
    back w.r.t. the pre-rotary projection output and no separate pass re-reads and re-rounds the q / k gradient (0.28 ms per block
    on cfg 2); the rotated buffer is the node's second output."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, nh, nkv, cu, tiles, k_tiles, scale, key_block, fold_forward=False, fwd_tiles=None):
        x = qkv.view(-1, qkv.shape[-1])                      # [T, W]; `qkv` itself may carry leading batch dims ([1, T, W])
        hd = x.shape[1] // (nh + 2 * nkv)
        rope = None if cos is None else (cos, sin)
        if rope is not None:
            # fold_forward: the rotary pass covers the k heads only (column block [nh hd, (nh + nkv) hd)): q is rotated by the
            # attention forward itself, by the block that owns it (flash_attn_varlen_fwd's `rope`)
            _rope_heads_(x, cos, sin, nh if fold_forward else 0, nkv if fold_forward else nh + nkv, hd)
            # autograd wants a tensor modified in place among the outputs, and it must not be a view made outside (hence the
            # caller's own tensor, not a reshaped view of it)
            ctx.mark_dirty(qkv)
            ctx.set_materialize_grads(False)
        work, q_block = _fwd_work(tiles, fwd_tiles)
        out, lse = flash_attn_varlen_fwd(*_qkv_views(x, nh, nkv, hd), cu, work, scale, padded_lse_len=0, num_seqs=cu.numel() - 1,
                                         rope=rope if fold_forward else None, q_block=q_block)
        ctx.save_for_backward(qkv, out, lse, cu, tiles, k_tiles, *(rope or ()))
        ctx.meta = (nh, nkv, hd, scale, key_block)
        return out if rope is None else (out, qkv)

    @staticmethod
    def backward(ctx, go, g_rotated=None):
        if g_rotated is not None:
            raise RuntimeError("rope_flash_attn_varlen_qkv: the rotated q|k|v buffer is internal, nothing may use it downstream")
        qkv, out, lse, cu, tiles, k_tiles, *rope = ctx.saved_tensors
        nh, nkv, hd, scale, key_block = ctx.meta
        W = qkv.shape[-1]
        dqkv = torch.empty_like(qkv)
        flash_attn_varlen_bwd(*_qkv_views(qkv.view(-1, W), nh, nkv, hd), out, go, lse, cu, tiles, k_tiles, scale,
                              grads=_qkv_views(dqkv.view(-1, W), nh, nkv, hd), key_block=key_block, rope=tuple(rope) or None)
        return (dqkv,) + (None,) * 11


def rope_flash_attn_varlen_qkv(qkv, cos, sin, num_heads, num_kv_heads, cu, tiles, k_tiles, scale, key_block=None,
                               head_dim: int = 64, fold_forward: bool = True, fwd_tiles=None):
    """qkv: the FRESH output of the fused q|k|v projection, [T, (num_heads + 2 num_kv_heads) * head_dim] (leading dims of size 1
    allowed: [1, T, W]; pass the projection's own tensor, not a reshaped view of it) bf16, contiguous, NOT yet rotated (it is
    rotated in place here); cos / sin: f32 [period, head_dim / 2] (row t % period for token t) -> attention
    output [T, num_heads, head_dim].  The gradient that comes back is w.r.t. the un-rotated projection output."""
    _check_qkv("rope_flash_attn_varlen_qkv", qkv, num_heads, num_kv_heads, head_dim)
    if key_block is None:
        key_block = attn_key_block(head_dim)
    if key_block == 64:
        raise ValueError("rope_flash_attn_varlen_qkv: the 64-key dK/dV kernel has no rotary epilogue; use rope_ + flash_attn_varlen_qkv")
    return _FlashAttnVarlenQKV.apply(qkv, cos, sin, num_heads, num_kv_heads, cu, tiles, k_tiles, scale, key_block,
                                     bool(fold_forward), fwd_tiles)[0]


FWD_ONLY_CALLS = 0    # forward-only fused rotary + attention calls so far (tests read it: the inference surface ran the hand-written path)


def rope_flash_attn_varlen_qkv_fwd(qkv, cos, sin, num_heads, num_kv_heads, cu, tiles, scale, head_dim: int = 64, fwd_tiles=None):
    """The FORWARD-ONLY entry of `rope_flash_attn_varlen_qkv` (no autograd node, for `torch.no_grad()` / `inference_mode()`
    callers: ModelForInference.encode, modeling.py:473-554; the RankPO ref_model, rankpo_trainer.py:468-477; eval-mode scoring):
    `rpo_rope` in place on the k heads of the fresh projection output, then the attention forward, which rotates the q block it
    loads anyway; no key-block table, no lse buffer.  Same kernels and same arithmetic as the training forward."""
    global FWD_ONLY_CALLS
    _check_qkv("rope_flash_attn_varlen_qkv_fwd", qkv, num_heads, num_kv_heads, head_dim)
    if torch.is_grad_enabled() and qkv.requires_grad:
        raise RuntimeError("rope_flash_attn_varlen_qkv_fwd is forward-only; use rope_flash_attn_varlen_qkv under autograd")
    x = qkv.view(-1, qkv.shape[-1])
    _rope_heads_(x, cos, sin, num_heads, num_kv_heads, head_dim)
    FWD_ONLY_CALLS += 1
    work, q_block = _fwd_work(tiles, fwd_tiles)
    return flash_attn_varlen_fwd(*_qkv_views(x, num_heads, num_kv_heads, head_dim), cu, work, scale, rope=(cos, sin),
                                 q_block=q_block, want_lse=False)[0]


def flash_attn_varlen_qkv(qkv, num_heads, num_kv_heads, cu, tiles, k_tiles, scale, key_block=None, head_dim: int = 64, fwd_tiles=None):
    """qkv: [T, (num_heads + 2 num_kv_heads) * head_dim] bf16, contiguous rows -> out [T, num_heads, head_dim]; head_dim 64
    or 128; key_block (None: the head_dim's default) = the block_n `k_tiles` was built with; fwd_tiles: the forward's own list
    (`attn_fwd_tile_table`) or None."""
    _check_qkv("flash_attn_varlen_qkv", qkv, num_heads, num_kv_heads, head_dim, flat=True)
    if key_block is None:
        key_block = attn_key_block(head_dim)
    return _FlashAttnVarlenQKV.apply(qkv, None, None, num_heads, num_kv_heads, cu, tiles, k_tiles, scale, key_block, False,
                                     fwd_tiles)


# ------------------------------------------------------------------------------------------------
# (7) one-query-per-sequence attention of the last block (encoder side)
# ------------------------------------------------------------------------------------------------
def last_query_attn_ok(q, kv, num_heads: int, num_kv_heads: int, head_dim: int) -> bool:
    return (q.is_cuda and q.dtype == torch.bfloat16 and kv.dtype == torch.bfloat16 and head_dim in (64, 128)
            and num_heads % num_kv_heads == 0 and num_heads // num_kv_heads in (1, 2, 4))


class _LastQueryAttn(torch.autograd.Function):
    """out[n] = softmax(scale q_n K_n^T) V_n for ONE query per sequence (its last token: no mask) on packed K / V that are the
    two column halves of the fused k|v projection output `kv` [T, 2 nkv hd] (k rotated in place already).  The backward writes
    ONE d(k|v) buffer of the same layout (no split / cat copies) and dq."""

    @staticmethod
    def forward(ctx, q, kv, cu, nkv, hd, scale):
        lib = _lib.load()
        N, nh = q.shape[0], q.shape[1]
        kv2 = kv.view(-1, kv.shape[-1])
        if q.stride(2) != 1 or q.stride(1) != hd or kv2.stride(1) != 1 or kv2.shape[1] != 2 * nkv * hd:
            raise ValueError("last_query_attn: q [N, nh, hd] with contiguous heads, kv [T, 2 nkv hd] with contiguous rows")
        out = torch.empty((N, nh, hd), dtype=q.dtype, device=q.device)
        lse = torch.empty((N, nh), dtype=torch.float32, device=q.device)
        es = kv2.element_size()
        with torch.cuda.device(q.device):
            check(lib.rpo_lastq_attn_fwd(q.data_ptr(), q.stride(0), kv2.data_ptr(), kv2.data_ptr() + nkv * hd * es, kv2.stride(0),
                                         kv2.stride(0), cu.data_ptr(), N, nh, nkv, hd, scale, out.data_ptr(), nh * hd,
                                         lse.data_ptr(), _stream(q)), "rpo_lastq_attn_fwd")
        ctx.save_for_backward(q, kv, cu, out, lse)
        ctx.meta = (nkv, hd, scale)
        return out

    @staticmethod
    def backward(ctx, go):
        q, kv, cu, out, lse = ctx.saved_tensors
        nkv, hd, scale = ctx.meta
        lib = _lib.load()
        N, nh = q.shape[0], q.shape[1]
        go = go.contiguous()
        kv2 = kv.view(-1, kv.shape[-1])
        dq = torch.empty((N, nh, hd), dtype=q.dtype, device=q.device)
        dkv = torch.empty_like(kv)                              # every row of both halves is written by the kernel
        d2 = dkv.view(-1, kv.shape[-1])
        es = kv2.element_size()
        with torch.cuda.device(q.device):
            check(lib.rpo_lastq_attn_bwd(q.data_ptr(), q.stride(0), kv2.data_ptr(), kv2.data_ptr() + nkv * hd * es, kv2.stride(0),
                                         kv2.stride(0), cu.data_ptr(), N, nh, nkv, hd, scale, out.data_ptr(), nh * hd,
                                         go.data_ptr(), nh * hd, lse.data_ptr(), dq.data_ptr(), nh * hd, d2.data_ptr(),
                                         d2.data_ptr() + nkv * hd * es, d2.stride(0), d2.stride(0), _stream(q)),
                  "rpo_lastq_attn_bwd")
        return dq, dkv, None, None, None, None


def last_query_attn(q, kv, cu, num_kv_heads: int, head_dim: int, scale: float):
    """q [N, nh, hd] (rotated), kv [..., T, 2 nkv hd] = the fused k|v projection output with k rotated; cu int32 [N + 1]
    -> [N, nh, hd].  Sequence n's query attends to ALL keys of sequence n."""
    if not kv.is_contiguous() or cu.numel() != q.shape[0] + 1:
        raise ValueError("last_query_attn: kv must be contiguous and cu_seqlens must have one entry per query + 1")
    return _LastQueryAttn.apply(q, kv, cu, num_kv_heads, head_dim, float(scale))


# ------------------------------------------------------------------------------------------------
# (9) packed forward of the BERT / XLM-R block (BertEncoder.pooled_cls; no autograd: forward only).  bf16 / fp16 tensors go to the
# entries of header section (9), float32 tensors to the f32-storage entries of section (9b).
# ------------------------------------------------------------------------------------------------
BIDIR_ATTN_Q_BLOCK = 32      # query rows per work-list entry of rpo_bidir_attn_fwd (the only format the kernel takes)
BERT_HEAD_DIMS = (32, 64)


def bidir_attn_tile_list(lens_q, lens_k, q_block: int = BIDIR_ATTN_Q_BLOCK):
    """The work list of `bidir_attn_fwd` as a host numpy int32 [n, 2] = (sequence id, first query row): one entry per
    (sequence, block of q_block queries), sequences with the most keys first (their entries are the longest-running ones)."""
    import numpy as np
    lq = np.asarray(lens_q, dtype=np.int64)
    lk = np.asarray(lens_k, dtype=np.int64)
    order = np.argsort(-lk, kind="stable")
    nt = (lq[order] + q_block - 1) // q_block
    seq = np.repeat(order, nt)
    q0 = (np.arange(int(nt.sum())) - np.repeat(np.cumsum(nt) - nt, nt)) * q_block
    return np.stack([seq, q0], 1).astype(np.int32).reshape(-1, 2)


EMBED_GRAD_CHUNK = 32        # rows of ds per work item of rpo_embed_grad_sorted: a table row that T tokens hit is summed by T / 32 waves


class EmbedGradPlan(NamedTuple):
    """`embed_grad_plan`'s result (int32 numpy arrays), or the same with order / chunks / multi on the device (`embed_grad_plan_to`,
    `BertEncoder._pack_upload`): what `embed_grad_sorted` takes."""
    order: object        # [T] the stable ascending sort of the ids: packed-token indices
    seg_ids: object      # [S] the distinct ids, ascending
    seg_start: object    # [S + 1] segment s = order[seg_start[s]:seg_start[s + 1]], the tokens whose id is seg_ids[s]
    chunks: object       # [C, 4] (id, first position in order, rows <= chunk, slot): slot = -1 for the only chunk of its segment,
    #                      else its workspace row; a segment's chunks are consecutive, from its first row, with consecutive slots
    multi: object        # [M, 3] (id, first slot, chunks) of the segments with several chunks
    n_partials: int      # slots in all


def embed_grad_plan(ids, chunk: int = EMBED_GRAD_CHUNK) -> EmbedGradPlan:
    """The host plan of `embed_grad_sorted` for the ids [T] of the packed tokens (host tensor or array; the caller has checked them
    against their table).  It fixes the order of every sum from the ids alone: see `embed_grad_sorted`."""
    import numpy as np
    if chunk < 1:
        raise ValueError("embed_grad_plan: chunk must be >= 1")
    a = np.asarray(ids, dtype=np.int64).reshape(-1)
    T = a.shape[0]
    if T and (int(a.min()) < 0 or int(a.max()) >= 1 << 31):
        raise ValueError("embed_grad_plan: ids must be table rows, 0 <= id < 2^31")
    # numpy's stable sort of 16-bit keys is a radix sort: low half, then high half = the stable sort of the whole key, several times
    # faster than the merge sort it runs on wider keys (the plan is host time in front of the step)
    order = np.argsort((a & 0xffff).astype(np.uint16), kind="stable")
    if T and int(a.max()) >= 1 << 16:
        order = order[np.argsort((a >> 16).astype(np.uint16)[order], kind="stable")]
    s = a[order]
    first = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]])) if T else np.zeros(0, np.int64)
    seg_start = np.concatenate([first, [T]]).astype(np.int64)
    seg_ids = s[first]
    nch = (np.diff(seg_start) + chunk - 1) // chunk                          # chunks per segment
    seg_of = np.repeat(np.arange(len(first)), nch)
    k = np.arange(int(nch.sum())) - np.repeat(np.cumsum(nch) - nch, nch)     # a chunk's index inside its segment
    start = seg_start[seg_of] + k * chunk
    rows = np.minimum(chunk, seg_start[seg_of + 1] - start)
    is_multi = nch > 1
    held = np.where(is_multi, nch, 0)
    slot0 = np.cumsum(held) - held
    slot = np.where(is_multi[seg_of], slot0[seg_of] + k, -1)
    i32 = lambda x, *shape: np.ascontiguousarray(x, dtype=np.int32).reshape(*shape)
    return EmbedGradPlan(i32(order, -1), i32(seg_ids, -1), i32(seg_start, -1),
                         i32(np.stack([seg_ids[seg_of], start, rows, slot], 1), -1, 4),
                         i32(np.stack([seg_ids[is_multi], slot0[is_multi], nch[is_multi]], 1), -1, 3), int(held.sum()))


def embed_grad_plan_parts(plan: EmbedGradPlan):
    """The arrays of a host plan that the kernel reads, flat, as host int32 tensors: what goes into an upload."""
    return [torch.from_numpy(plan.order), torch.from_numpy(plan.chunks).reshape(-1), torch.from_numpy(plan.multi).reshape(-1)]


def embed_grad_plan_views(plan: EmbedGradPlan, order, chunks, multi) -> EmbedGradPlan:
    """The plan with the device views of its uploaded parts (flat, as `embed_grad_plan_parts` lists them) in place."""
    return plan._replace(order=order, chunks=chunks.view(-1, 4), multi=multi.view(-1, 3))


def embed_grad_plan_to(plan: EmbedGradPlan, device) -> EmbedGradPlan:
    """One pinned upload of a host plan (tests, tools; the training step puts its plans into the upload it makes anyway)."""
    parts = embed_grad_plan_parts(plan)
    buf = torch.cat(parts).pin_memory().to(device, non_blocking=True)
    n = [p.numel() for p in parts]
    return embed_grad_plan_views(plan, buf[:n[0]], buf[n[0]:n[0] + n[1]], buf[n[0] + n[1]:])


def bidir_attn_tile_table(lens_q, lens_k, device, q_block: int = BIDIR_ATTN_Q_BLOCK):
    return torch.from_numpy(bidir_attn_tile_list(lens_q, lens_k, q_block)).to(device, non_blocking=True)


def bidir_attn_fwd(q, k, v, cu_q, cu_k, tiles, scale, want_lse: bool = False):
    """Non-causal variable-length attention: q [Tq, nh, hd], k / v [Tk, nh, hd] (heads contiguous, token stride free: column
    blocks of one fused projection output), cu_q / cu_k int32 [N + 1], tiles from `bidir_attn_tile_table(lens_q, lens_k)`.
    Returns (out [Tq, nh * hd], lse f32 [nh, Tq] or None)."""
    lib = _lib.load()
    Tq, nh, hd = q.shape
    for t in (q, k, v):
        if t.stride(2) != 1 or t.stride(1) != hd:
            raise ValueError("bidir_attn_fwd: heads must be contiguous inside a token row")
    out = torch.empty((Tq, nh * hd), dtype=q.dtype, device=q.device)
    lse = torch.empty((nh, Tq), dtype=torch.float32, device=q.device) if want_lse else None
    if q.dtype == torch.float32:             # f32 storage: the entries of header section (9b)
        with torch.cuda.device(q.device):
            check(lib.rpo_bidir_attn_fwd_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0), v.stride(0),
                                             cu_q.data_ptr(), cu_k.data_ptr(), tiles.data_ptr(), tiles.shape[0], tiles.shape[1],
                                             BIDIR_ATTN_Q_BLOCK, Tq, nh, k.shape[1], hd, float(scale), out.data_ptr(), nh * hd,
                                             _p(lse), _stream(q)), "rpo_bidir_attn_fwd_f32")
        return out, lse
    with torch.cuda.device(q.device):
        check(lib.rpo_bidir_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0), v.stride(0),
                                     cu_q.data_ptr(), cu_k.data_ptr(), tiles.data_ptr(), tiles.shape[0], tiles.shape[1],
                                     BIDIR_ATTN_Q_BLOCK, Tq, nh, k.shape[1], hd, _dt(q), float(scale), out.data_ptr(), nh * hd,
                                     _p(lse), _stream(q)), "rpo_bidir_attn_fwd")
    return out, lse


# ------------------------------------------------------------------------------------------------
# (9c)-(9f) causal grouped-query attention of the packed Llama pass on f32 and on fp16 storage (opt-in: encoder.LLAMA_F32_ATTENTION
# / _TRAIN, encoder.LLAMA_FP16_NATIVE / _TRAIN): forward, backward and the autograd Function over the pair.  Header sections
# (9c)-(9f), rankpo_amd/csrc/causal_attn_{f32,f32_bwd,f16,f16_bwd}.hip.  ONE implementation, driven by a per-dtype record; the
# public names of both dtypes are bindings of it.
# ------------------------------------------------------------------------------------------------
CAUSAL_ATTN_F32_Q_BLOCK = 32             # query (and key) rows per work-list entry (the only format the kernels take)
CAUSAL_ATTN_F32_HEAD_DIMS = (64, 128)
CAUSAL_ATTN_F32_GROUPS = (1, 2, 4, 8)    # query heads per kv head
CAUSAL_ATTN_F16_Q_BLOCK = CAUSAL_ATTN_F32_Q_BLOCK    # one list format, one set of shapes
CAUSAL_ATTN_F16_HEAD_DIMS = CAUSAL_ATTN_F32_HEAD_DIMS
CAUSAL_ATTN_F16_GROUPS = CAUSAL_ATTN_F32_GROUPS


class _CausalAttnKind(NamedTuple):
    """What differs between the f32 and the fp16 instantiation on the host."""
    tag: str             # f32 / f16: the entries are rpo_causal_attn_{fwd,bwd}_<tag>, the raw ops <name> and <name>_bwd
    dtype: torch.dtype
    stride_mult: int     # elements per 16 bytes: token strides are multiples of it
    ws_tail: tuple       # the backward's workspace is f32 [nh, Tq, *ws_tail]: (delta, 1 / L') pairs for f32, delta for fp16
    fused_grads: bool    # dq / dk / dv as column blocks of ONE [T, (nh + 2 nkv) hd] buffer (dq + fused dk|dv where Tq != Tk), as
    #                      the q|k|v projection output lies; False: three contiguous tensors

    @property
    def name(self):
        return "causal_attn_" + self.tag


_CAUSAL_F32 = _CausalAttnKind("f32", torch.float32, 4, (2,), False)
_CAUSAL_F16 = _CausalAttnKind("f16", torch.float16, 8, (), True)


def _causal_attn_block_list(name, lens_q, lens_k, of_keys: bool):
    """Host numpy int32 [n, 2] = (sequence id, first row): one entry per (sequence, block of 32 queries), or of 32 keys with
    `of_keys` (sequences without queries included: their dk / dv rows are zero-filled).  Query i of a sequence sees the keys
    j <= i + (lk - lq).  The longest-running entries come first: a query entry runs until the last visible key of its last query,
    a key entry walks the queries that see its first key, lq - max(0, k0 - (lk - lq)) of them."""
    import numpy as np
    blk = CAUSAL_ATTN_F32_Q_BLOCK
    lq = np.asarray(lens_q, dtype=np.int64).reshape(-1)
    lk = np.asarray(lens_k, dtype=np.int64).reshape(-1)
    if lq.shape != lk.shape:
        raise ValueError(f"{name}: one query length and one key length per sequence")
    if (lq > lk).any() or (lq < 0).any():
        raise ValueError(f"{name}: 0 <= lens_q[n] <= lens_k[n] is required (bottom-right aligned causal mask)")
    nt = ((lk if of_keys else lq) + blk - 1) // blk
    seq = np.repeat(np.arange(len(lq)), nt)
    r0 = (np.arange(int(nt.sum())) - np.repeat(np.cumsum(nt) - nt, nt)) * blk
    shift = (lk - lq)[seq]
    work = lq[seq] - np.maximum(0, r0 - shift) if of_keys else np.minimum(r0 + blk, lq[seq]) - 1 + shift
    order = np.argsort(-work, kind="stable")
    return np.stack([seq[order], r0[order]], 1).astype(np.int32).reshape(-1, 2)


def _tile_upload(table, device):
    """A host work list on the device: a pinned, asynchronous upload (nothing waits for it on the host)."""
    t = torch.from_numpy(table)
    if torch.device(device).type == "cuda":
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


def causal_attn_f32_tile_list(lens_q, lens_k):
    """The work list of `causal_attn_f32` / `_f16`: `_causal_attn_block_list` over the queries.  lens_q[n] > lens_k[n] (a query in
    front of every key) raises ValueError."""
    return _causal_attn_block_list("causal_attn_f32_tile_list", lens_q, lens_k, False)


def causal_attn_f32_key_tile_list(lens_q, lens_k):
    """The key work list of `causal_attn_f32_bwd` / `_f16_bwd`: `_causal_attn_block_list` over the keys.  Raises ValueError in the
    cases `causal_attn_f32_tile_list` does."""
    return _causal_attn_block_list("causal_attn_f32_key_tile_list", lens_q, lens_k, True)


def causal_attn_f32_tile_table(lens_q, lens_k, device):
    return _tile_upload(causal_attn_f32_tile_list(lens_q, lens_k), device)


def causal_attn_f32_key_tile_table(lens_q, lens_k, device):
    return _tile_upload(causal_attn_f32_key_tile_list(lens_q, lens_k), device)


def causal_attn_f32_shape_ok(num_heads: int, num_kv_heads: int, head_dim: int) -> bool:
    return (head_dim in CAUSAL_ATTN_F32_HEAD_DIMS and num_kv_heads > 0 and num_heads % num_kv_heads == 0
            and num_heads // num_kv_heads in CAUSAL_ATTN_F32_GROUPS)


def _causal_attn_ok(kind, q, k, v) -> bool:
    """What the entries of `kind` take, restated: its dtype on a HIP device, q [Tq, nh, hd] and k / v [Tk, nkv, hd] with heads
    contiguous inside a token row, head_dim 64 or 128, nh / nkv in (1, 2, 4, 8), 16-byte aligned with token strides a multiple of
    16 bytes."""
    if not all(t.is_cuda and t.dtype == kind.dtype and t.dim() == 3 for t in (q, k, v)):
        return False
    hd = q.shape[2]
    if k.shape != v.shape or k.shape[2] != hd or not causal_attn_f32_shape_ok(q.shape[1], k.shape[1], hd):
        return False
    return all(t.stride(2) == 1 and t.stride(1) == hd and t.stride(0) % kind.stride_mult == 0 and t.stride(0) > 0
               and t.data_ptr() % 16 == 0 for t in (q, k, v))


def _causal_attn_check(kind, fn, q, k, v, cu_q, cu_k, *lists):
    if not _causal_attn_ok(kind, q, k, v):
        raise ValueError(f"{fn}: {str(kind.dtype)[6:]} HIP tensors [T, heads, head_dim] with head_dim in (64, 128), 1 / 2 / 4 / 8 "
                         f"query heads per kv head, heads contiguous, 16-byte aligned, token strides % {kind.stride_mult} == 0")
    if (cu_q.numel() != cu_k.numel() or cu_q.dtype != torch.int32 or cu_k.dtype != torch.int32
            or not all(t.dtype == torch.int32 and t.dim() == 2 and t.shape[1] == 2 and t.is_contiguous() for t in lists)):
        raise ValueError(f"{fn}: cu_q / cu_k int32 [N + 1], {' / '.join(['tiles', 'k_tiles'][:len(lists)])} int32 [n, 2]")


def _causal_attn_fwd(kind, q, k, v, cu_q, cu_k, tiles, scale, want_lse: bool = False):
    """Causal grouped-query variable-length attention: q [Tq, nh, hd], k / v [Tk, nkv, hd] (heads contiguous, token stride free:
    column blocks of one fused projection output), cu_q / cu_k int32 [N + 1] on the device, tiles from
    `causal_attn_f32_tile_table(lens_q, lens_k)` (which checks lens_q <= lens_k).  Query i of sequence n sees its keys
    j <= i + (lk - lq).  Returns (out [Tq, nh * hd] of q's dtype, lse f32 [nh, Tq] or None).  Forward only: no autograd node."""
    _causal_attn_check(kind, kind.name, q, k, v, cu_q, cu_k, tiles)
    entry = "rpo_causal_attn_fwd_" + kind.tag
    Tq, nh, hd = q.shape
    out = torch.empty((Tq, nh * hd), dtype=q.dtype, device=q.device)
    lse = torch.empty((nh, Tq), dtype=torch.float32, device=q.device) if want_lse else None
    with torch.cuda.device(q.device):
        check(getattr(_lib.load(), entry)(q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0), v.stride(0),
                                          cu_q.data_ptr(), cu_k.data_ptr(), tiles.data_ptr(), tiles.shape[0], tiles.shape[1],
                                          CAUSAL_ATTN_F32_Q_BLOCK, cu_q.numel() - 1, nh, k.shape[1], hd, float(scale),
                                          out.data_ptr(), nh * hd, _p(lse), _stream(q)), entry)
    return out, lse


def _causal_attn_bwd(kind, q, k, v, out, lse, dout, cu_q, cu_k, tiles, k_tiles, scale):
    """The gradients of the forward: (dq [Tq, nh, hd], dk [Tk, nkv, hd], dv [Tk, nkv, hd]) of q's dtype (fp16: column blocks of
    ONE fused buffer, see `_CausalAttnKind.fused_grads`), from its inputs, its results (out [Tq, nh * hd], lse f32 [nh, Tq]) and
    dout (the shape of out or of q).  tiles as the forward's, k_tiles from `causal_attn_f32_key_tile_table` on the same lengths.
    One entry, two launches (dQ, then dK/dV), no atomics: deterministic, and independent of what else is packed in the batch.
    The raw op: no autograd node."""
    fn = kind.name + "_bwd"
    _causal_attn_check(kind, fn, q, k, v, cu_q, cu_k, tiles, k_tiles)
    Tq, nh, hd = q.shape
    Tk, nkv, _ = k.shape
    if (out.dtype != kind.dtype or dout.dtype != kind.dtype or lse.dtype != torch.float32 or out.numel() != q.numel()
            or dout.numel() != q.numel() or lse.shape != (nh, Tq) or not lse.is_contiguous()):
        raise ValueError(f"{fn}: out / dout {str(kind.dtype)[6:]} [Tq, nh * hd], lse float32 [nh, Tq] contiguous")

    def rows(t):       # [Tq, nh * hd] with contiguous rows, 16-byte aligned, token stride a multiple of 16 bytes: as it is, else a copy
        t = t.reshape(Tq, nh * hd)                      # a view wherever the strides allow one
        if t.stride(1) != 1 or t.stride(0) % kind.stride_mult or t.stride(0) <= 0 or t.data_ptr() % 16:
            t = t.contiguous()
        return t
    out, dout = rows(out), rows(dout)
    new = lambda *shape: torch.empty(shape, dtype=kind.dtype, device=q.device)
    if not kind.fused_grads:
        dq, dk, dv = new(Tq, nh, hd), new(Tk, nkv, hd), new(Tk, nkv, hd)
    elif Tq == Tk:     # self-attention: one fused gradient buffer, as the q|k|v projection output lies
        dq, dk, dv = (t.view(Tq, -1, hd) for t in new(Tq, (nh + 2 * nkv) * hd).split([nh * hd, nkv * hd, nkv * hd], 1))
    else:
        dq = new(Tq, nh, hd)
        dk, dv = (t.view(Tk, nkv, hd) for t in new(Tk, 2 * nkv * hd).split(nkv * hd, 1))
    ws = torch.empty((nh, Tq) + kind.ws_tail, dtype=torch.float32, device=q.device)
    entry = "rpo_causal_attn_bwd_" + kind.tag
    with torch.cuda.device(q.device):
        check(getattr(_lib.load(), entry)(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr(), q.stride(0),
                                          k.stride(0), v.stride(0), out.stride(0), dout.stride(0), lse.data_ptr(), cu_q.data_ptr(),
                                          cu_k.data_ptr(), tiles.data_ptr(), tiles.shape[0], k_tiles.data_ptr(), k_tiles.shape[0],
                                          tiles.shape[1], CAUSAL_ATTN_F32_Q_BLOCK, cu_q.numel() - 1, nh, nkv, hd, float(scale),
                                          dq.data_ptr(), dq.stride(0), dk.data_ptr(), dk.stride(0), dv.data_ptr(), dv.stride(0),
                                          ws.data_ptr(), _stream(q)), entry)
    return dq, dk, dv


class _CausalAttnTrain(torch.autograd.Function):
    """The forward with lse and ONE backward call, through the module's public names of `kind` (what a test or tool wraps)."""

    @staticmethod
    def forward(ctx, kind, q, k, v, cu_q, cu_k, tiles, k_tiles, scale):
        out, lse = globals()[kind.name](q, k, v, cu_q, cu_k, tiles, scale, want_lse=True)
        ctx.save_for_backward(q, k, v, out, lse, cu_q, cu_k, tiles, k_tiles)
        ctx.kind, ctx.scale = kind, scale
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, cu_q, cu_k, tiles, k_tiles = ctx.saved_tensors
        dq, dk, dv = globals()[ctx.kind.name + "_bwd"](q, k, v, out, lse, dout, cu_q, cu_k, tiles, k_tiles, ctx.scale)
        return None, dq, dk, dv, None, None, None, None, None


def _causal_attn_train(kind, q, k, v, cu_q, cu_k, tiles, k_tiles, scale):
    """The forward with a gradient: an autograd Function over (q, k, v), column-block views of the fused projection output
    included.  Forward: the raw forward with want_lse=True (the same deterministic kernel, also when a checkpointed block
    recomputes it); saved: q, k, v, out, lse and the lists; backward: ONE call of the raw backward (dout of any stride: made
    contiguous only if needed).  Returns out [Tq, nh * hd]."""
    return _CausalAttnTrain.apply(kind, q, k, v, cu_q, cu_k, tiles, k_tiles, scale)


def _bind(impl, kind):
    f = functools.partial(impl, kind)
    f.__doc__ = f"`{impl.__name__}` on {str(kind.dtype)[6:]} storage.\n\n{impl.__doc__}"
    return f


causal_attn_f32_ok, causal_attn_f16_ok = _bind(_causal_attn_ok, _CAUSAL_F32), _bind(_causal_attn_ok, _CAUSAL_F16)
causal_attn_f32, causal_attn_f16 = _bind(_causal_attn_fwd, _CAUSAL_F32), _bind(_causal_attn_fwd, _CAUSAL_F16)
causal_attn_f32_bwd, causal_attn_f16_bwd = _bind(_causal_attn_bwd, _CAUSAL_F32), _bind(_causal_attn_bwd, _CAUSAL_F16)
causal_attn_f32_train, causal_attn_f16_train = _bind(_causal_attn_train, _CAUSAL_F32), _bind(_causal_attn_train, _CAUSAL_F16)
causal_attn_f16_shape_ok = causal_attn_f32_shape_ok
causal_attn_f16_tile_list, causal_attn_f16_tile_table = causal_attn_f32_tile_list, causal_attn_f32_tile_table
causal_attn_f16_key_tile_list, causal_attn_f16_key_tile_table = causal_attn_f32_key_tile_list, causal_attn_f32_key_tile_table


def add_layernorm(a, b, weight, bias, eps, out=None):
    """LayerNorm(a + b) * weight + bias over the last dim of 2-D row-strided a / b (b may be None); a + b rounded to the storage
    dtype first.  out: [rows, d] (row stride free) or None (a new contiguous tensor)."""
    lib = _lib.load()
    rows, d = a.shape
    if out is None:
        out = torch.empty((rows, d), dtype=a.dtype, device=a.device)
    for t in (a, b, out):
        if t is not None and t.stride(1) != 1:
            raise ValueError("add_layernorm: rows must be contiguous")
    if a.dtype == torch.float32:
        with torch.cuda.device(a.device):
            check(lib.rpo_add_layernorm_fwd_f32(a.data_ptr(), a.stride(0), _p(b), b.stride(0) if b is not None else 0,
                                                weight.data_ptr(), bias.data_ptr(), float(eps), out.data_ptr(), out.stride(0),
                                                rows, d, _stream(a)), "rpo_add_layernorm_fwd_f32")
        return out
    with torch.cuda.device(a.device):
        check(lib.rpo_add_layernorm_fwd(a.data_ptr(), a.stride(0), _p(b), b.stride(0) if b is not None else 0,
                                        weight.data_ptr(), bias.data_ptr(), float(eps), out.data_ptr(), out.stride(0), rows, d,
                                        _dt(a), _stream(a)), "rpo_add_layernorm_fwd")
    return out


def gelu_(x):
    """Exact erf GELU in place over a 2-D row-strided x; returns x."""
    lib = _lib.load()
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("gelu_: 2-D with contiguous rows")
    if x.dtype == torch.float32:
        with torch.cuda.device(x.device):
            check(lib.rpo_gelu_fwd_f32(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), _stream(x)), "rpo_gelu_fwd_f32")
        return x
    with torch.cuda.device(x.device):
        check(lib.rpo_gelu_fwd(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), _dt(x), _stream(x)), "rpo_gelu_fwd")
    return x


def bert_embed_ln(ids, pos, token_types, word, type_emb, pos_emb, weight, bias, eps):
    """(word[ids] + type_emb[token_types]) + pos_emb[pos], then LayerNorm: ids / pos / token_types int32 [T] on the device
    (token_types None: type 0) -> [T, d].  The caller checks the index ranges (the kernel clamps)."""
    lib = _lib.load()
    T, d = ids.shape[0], word.shape[1]
    for t in (word, type_emb, pos_emb):
        if not t.is_contiguous():
            raise ValueError("bert_embed_ln: embedding tables must be contiguous")
    out = torch.empty((T, d), dtype=word.dtype, device=word.device)
    if word.dtype == torch.float32:
        with torch.cuda.device(word.device):
            check(lib.rpo_bert_embed_ln_fwd_f32(ids.data_ptr(), _p(token_types), pos.data_ptr(), T, word.data_ptr(), word.shape[0],
                                                type_emb.data_ptr(), type_emb.shape[0], pos_emb.data_ptr(), pos_emb.shape[0],
                                                weight.data_ptr(), bias.data_ptr(), float(eps), out.data_ptr(), d, d,
                                                _stream(word)), "rpo_bert_embed_ln_fwd_f32")
        return out
    with torch.cuda.device(word.device):
        check(lib.rpo_bert_embed_ln_fwd(ids.data_ptr(), _p(token_types), pos.data_ptr(), T, word.data_ptr(), word.shape[0],
                                        type_emb.data_ptr(), type_emb.shape[0], pos_emb.data_ptr(), pos_emb.shape[0],
                                        weight.data_ptr(), bias.data_ptr(), float(eps), out.data_ptr(), d, d, _dt(word),
                                        _stream(word)), "rpo_bert_embed_ln_fwd")
    return out


# ------------------------------------------------------------------------------------------------
# (10) packed TRAINING step of the BERT / XLM-R block (BertEncoder.pooled_cls_train): autograd over bert_ops.hip.  GEMMs stay
# F.linear under torch's autograd.
# ------------------------------------------------------------------------------------------------
def bidir_attn_key_tile_list(lens_q, lens_k, k_block: int = BIDIR_ATTN_Q_BLOCK):
    """The work list of the dK/dV kernel of `bidir_attn_bwd` as a host numpy int32 [n, 2] = (sequence id, first key row): one
    entry per (sequence, block of k_block keys), sequences with the most queries first (their entries run longest)."""
    return bidir_attn_tile_list(lens_k, lens_q, k_block)


def bert_layer_seed(seed: int, layer: int) -> int:
    """The attention-dropout seed of block `layer` for a call's `seed`: seed + layer * 0x9E3779B97F4A7C15 mod 2^64 (an odd
    multiplier: distinct layers get distinct seeds)."""
    return (int(seed) + int(layer) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def bert_hidden_seed(seed: int) -> int:
    """The seed of the hidden-dropout sites (fused into the row kernels) for a call's `seed`: seed + 0xD1B54A32D192ED03 mod 2^64.
    The offset is no multiple i * 0x9E3779B97F4A7C15 mod 2^64 with i < 4096 (tests/test_hidden_dropout_host.py), so it equals no
    `bert_layer_seed(seed, i)` of an encoder of fewer than 4096 blocks: attention and hidden dropout never share a Philox key."""
    return (int(seed) + 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF


def bert_hidden_site(block: int = -1, ffn: bool = False) -> int:
    """Site index of a hidden dropout: 0 = the embedding output (block < 0), 1 + 2 i = after the attention output dense of block
    i, 2 + 2 i = after its FFN output dense."""
    return 0 if block < 0 else 1 + 2 * int(block) + int(bool(ffn))


def hidden_dropout_scale(p_drop: float) -> float:
    """1 / (1 - p_drop) as the f32 value the kernels multiply by (the attention dropout's convention); 1.0 when p_drop quantises
    to no dropout (p_drop < 2^-17)."""
    if not 0.0 <= p_drop < 1.0:
        raise ValueError("hidden_dropout_scale: p_drop must lie in [0, 1)")
    return float(_lib.load().rpo_hidden_dropout_scale(float(p_drop)))


def hidden_dropout_mask(row0: int, rows: int, d: int, p_drop: float, seed: int, site: int, device):
    """The keep mask (uint8 [rows, d], 1 = kept) of the fused hidden dropout for rows row0.. of `site`; `seed` as handed to the
    kernels (`bert_hidden_seed` of the call's seed).  Tests and diagnostics: the product never calls it."""
    lib = _lib.load()
    mask = torch.empty((rows, d), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        check(lib.rpo_hidden_dropout_mask(row0, rows, d, float(p_drop), int(seed), int(site), mask.data_ptr(),
                                          torch.cuda.current_stream(device).cuda_stream), "rpo_hidden_dropout_mask")
    return mask


def _heads_ok(who, hd, *ts):
    for t in ts:
        if t.stride(2) != 1 or t.stride(1) != hd:
            raise ValueError(f"{who}: heads must be contiguous inside a token row")


def bidir_attn_train_fwd(q, k, v, cu_q, cu_k, tiles, scale, p_drop: float = 0.0, seed: int = 0):
    """`bidir_attn_fwd` with attention-probability dropout (p_drop = 0: none); always returns (out, lse): lse and the row sums
    come from the undropped probabilities, out = (P * keep / (1 - p_drop)) V with keep from `bidir_attn_dropout_mask`'s function."""
    lib = _lib.load()
    Tq, nh, hd = q.shape
    _heads_ok("bidir_attn_train_fwd", hd, q, k, v)
    out = torch.empty((Tq, nh * hd), dtype=q.dtype, device=q.device)
    lse = torch.empty((nh, Tq), dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device):
        check(lib.rpo_bidir_attn_train_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0), v.stride(0),
                                           cu_q.data_ptr(), cu_k.data_ptr(), tiles.data_ptr(), tiles.shape[0], tiles.shape[1],
                                           BIDIR_ATTN_Q_BLOCK, Tq, nh, k.shape[1], hd, _dt(q), float(scale), float(p_drop),
                                           int(seed), out.data_ptr(), nh * hd, lse.data_ptr(), _stream(q)),
              "rpo_bidir_attn_train_fwd")
    return out, lse


def bidir_attn_bwd(q, k, v, out, dout, lse, cu_q, cu_k, q_tiles, k_tiles, scale, dq, dk, dv, p_drop: float = 0.0, seed: int = 0):
    """Backward of `bidir_attn_fwd` / `bidir_attn_train_fwd` into dq / dk / dv ([T, nh, hd] views, token stride free: column
    blocks of one fused gradient buffer).  k_tiles from `bidir_attn_key_tile_list`.  Returns (dq, dk, dv)."""
    lib = _lib.load()
    Tq, nh, hd = q.shape
    _heads_ok("bidir_attn_bwd", hd, q, k, v, dq, dk, dv)
    if out.stride(1) != 1 or dout.stride(1) != 1:
        raise ValueError("bidir_attn_bwd: out / dout rows must be contiguous")
    with torch.cuda.device(q.device):
        check(lib.rpo_bidir_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), k.stride(0), v.stride(0),
                                     out.data_ptr(), out.stride(0), dout.data_ptr(), dout.stride(0), lse.data_ptr(),
                                     cu_q.data_ptr(), cu_k.data_ptr(), q_tiles.data_ptr(), q_tiles.shape[0], k_tiles.data_ptr(),
                                     k_tiles.shape[0], q_tiles.shape[1], BIDIR_ATTN_Q_BLOCK, Tq, nh, k.shape[1], hd, _dt(q),
                                     float(scale), float(p_drop), int(seed), dq.data_ptr(), dq.stride(0), dk.data_ptr(),
                                     dk.stride(0), dv.data_ptr(), dv.stride(0), _stream(q)), "rpo_bidir_attn_bwd")
    return dq, dk, dv


def bidir_attn_dropout_mask(q_row0: int, k_row0: int, len_q: int, len_k: int, num_heads: int, p_drop: float, seed: int, device,
                            head0: int = 0):
    """The keep mask (uint8 [num_heads, len_q, len_k], 1 = kept) the attention kernels use for packed query rows q_row0.. and
    packed key rows k_row0.. of one sequence.  Tests and diagnostics: the product never calls it."""
    lib = _lib.load()
    mask = torch.empty((num_heads, len_q, len_k), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        check(lib.rpo_bidir_attn_dropout_mask(q_row0, k_row0, len_q, len_k, head0, num_heads, float(p_drop), int(seed),
                                              mask.data_ptr(), torch.cuda.current_stream(device).cuda_stream),
              "rpo_bidir_attn_dropout_mask")
    return mask


class _BidirAttn(torch.autograd.Function):
    """Packed bidirectional attention over ONE fused projection output.  `kv` None: a = q|k|v [T, 3 d] (self-attention of every
    token); else a = q [Nq, d] and kv = k|v [T, 2 d] (the last block: one CLS query per sequence).  The backward writes the
    gradient of each fused buffer in place of its column blocks: no concatenation."""

    @staticmethod
    def forward(ctx, a, kv, nh, cu_q, cu_k, q_tiles, k_tiles, scale, p_drop, seed):
        d = a.shape[1] if kv is not None else a.shape[1] // 3
        hd = d // nh
        ctx.dims = (nh, hd, d, float(scale), float(p_drop), int(seed))
        q, k, v = _BidirAttn._views(a, kv, nh, hd, d)
        out, lse = bidir_attn_train_fwd(q, k, v, cu_q, cu_k, q_tiles, scale, p_drop, seed)
        ctx.save_for_backward(a, kv, out, lse, cu_q, cu_k, q_tiles, k_tiles)
        return out

    @staticmethod
    def _views(a, kv, nh, hd, d):
        if kv is None:
            return tuple(a[:, j * d:(j + 1) * d].view(-1, nh, hd) for j in range(3))
        return a.view(-1, nh, hd), kv[:, :d].view(-1, nh, hd), kv[:, d:].view(-1, nh, hd)

    @staticmethod
    def backward(ctx, go):
        a, kv, out, lse, cu_q, cu_k, q_tiles, k_tiles = ctx.saved_tensors
        nh, hd, d, scale, p_drop, seed = ctx.dims
        go = go if go.stride(1) == 1 and go.stride(0) % 8 == 0 and go.data_ptr() % 16 == 0 else go.contiguous()
        da = torch.empty_like(a)
        dkv = None if kv is None else torch.empty_like(kv)
        q, k, v = _BidirAttn._views(a, kv, nh, hd, d)
        dq, dk, dv = _BidirAttn._views(da, dkv, nh, hd, d)
        bidir_attn_bwd(q, k, v, out, go, lse, cu_q, cu_k, q_tiles, k_tiles, scale, dq, dk, dv, p_drop, seed)
        return (da, dkv) + (None,) * 8


def bidir_attn(a, kv, num_heads, cu_q, cu_k, q_tiles, k_tiles, scale, p_drop: float = 0.0, seed: int = 0):
    """Differentiable packed bidirectional attention (see `_BidirAttn`) -> [Tq, d]."""
    if not a.is_contiguous() or (kv is not None and not kv.is_contiguous()):
        raise ValueError("bidir_attn: the fused projection outputs must be contiguous")
    return _BidirAttn.apply(a, kv, num_heads, cu_q, cu_k, q_tiles, k_tiles, scale, p_drop, seed)


def _layernorm_bwd(s, dy, name, launch, *outs):
    """Shared body of the two wrappers below: `launch(lib, dy, ds, dgamma_partial, dbeta_partial)` is the entry's status with the
    made-contiguous dy, the fresh ds and the two per-block partial buffers -> (ds, *outs, dgamma, dbeta)."""
    lib = _lib.load()
    rows, d = s.shape
    dy = dy if dy.stride(1) == 1 and dy.stride(0) % 8 == 0 and dy.data_ptr() % 16 == 0 else dy.contiguous()
    ds = torch.empty((rows, d), dtype=s.dtype, device=s.device)
    if rows == 0:
        z = torch.zeros((d,), dtype=torch.float32, device=s.device)
        return (ds, *outs, z, z.clone())
    nb = lib.rpo_layernorm_bwd_blocks(rows)
    part = torch.empty((2, nb, d), dtype=torch.float32, device=s.device)
    with torch.cuda.device(s.device):
        check(launch(lib, dy, ds, part[0], part[1]), name)
    sums = part.sum(1)
    return (ds, *outs, sums[0], sums[1])


def layernorm_bwd(s, weight, dy, eps):
    """(ds, dgamma, dbeta) of y = LayerNorm(s) * weight + bias from the stored rounded sum s [rows, d]; dgamma / dbeta f32."""
    rows, d = s.shape
    return _layernorm_bwd(s, dy, "rpo_layernorm_bwd", lambda lib, dy, ds, dg, db_: lib.rpo_layernorm_bwd(
        s.data_ptr(), s.stride(0), weight.data_ptr(), dy.data_ptr(), dy.stride(0), float(eps), ds.data_ptr(), d, dg.data_ptr(),
        db_.data_ptr(), rows, d, _dt(s), _stream(s)))


def layernorm_drop_bwd(s, weight, dy, eps, p_drop, seed, site_in: int = -1, site_out: int = -1):
    """`layernorm_bwd` with the fused hidden dropout -> (ds, db or None, dgamma, dbeta).  site_in >= 0: dy is dropped (site_in)
    as it is loaded; site_out >= 0: db = the dropped rounded ds (site_out), the gradient of the addend that was dropped."""
    rows, d = s.shape
    db = torch.empty((rows, d), dtype=s.dtype, device=s.device) if site_out >= 0 else None
    return _layernorm_bwd(s, dy, "rpo_layernorm_drop_bwd", lambda lib, dy, ds, dg, db_: lib.rpo_layernorm_drop_bwd(
        s.data_ptr(), s.stride(0), weight.data_ptr(), dy.data_ptr(), dy.stride(0), float(eps), ds.data_ptr(), d, _p(db), d,
        dg.data_ptr(), db_.data_ptr(), rows, d, _dt(s), float(p_drop), int(seed), int(site_in), int(site_out), _stream(s)), db)


class _AddLayerNorm(torch.autograd.Function):
    """y = LayerNorm(a + b) * weight + bias (b may be None) with the backward kernel: ds is the gradient of both addends.
    p_drop > 0 (b required): y = LayerNorm(a + dropout(b)) with the hidden dropout of `site` inside the forward and backward
    kernels (`hidden_dropout_mask`'s function: nothing but s is saved)."""

    @staticmethod
    def forward(ctx, a, b, weight, bias, eps, p_drop=0.0, seed=0, site=0):
        lib = _lib.load()
        rows, d = a.shape
        for t in (a, b):
            if t is not None and t.stride(1) != 1:
                raise ValueError("add_layernorm_train: rows must be contiguous")
        y = torch.empty((rows, d), dtype=a.dtype, device=a.device)
        s = torch.empty((rows, d), dtype=a.dtype, device=a.device)
        ctx.drop = (float(p_drop), int(seed), int(site)) if p_drop > 0 else None
        with torch.cuda.device(a.device):
            if ctx.drop is None:
                check(lib.rpo_add_layernorm_train_fwd(a.data_ptr(), a.stride(0), _p(b), b.stride(0) if b is not None else 0,
                                                      weight.data_ptr(), bias.data_ptr(), float(eps), y.data_ptr(), d, s.data_ptr(),
                                                      d, rows, d, _dt(a), _stream(a)), "rpo_add_layernorm_train_fwd")
            else:
                if b is None:
                    raise ValueError("add_layernorm_train: p_drop > 0 needs the addend b that is dropped")
                check(lib.rpo_add_layernorm_drop_fwd(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), weight.data_ptr(),
                                                     bias.data_ptr(), float(eps), y.data_ptr(), d, s.data_ptr(), d, rows, d,
                                                     _dt(a), *ctx.drop, _stream(a)), "rpo_add_layernorm_drop_fwd")
        ctx.save_for_backward(s, weight)
        ctx.eps, ctx.has_b = float(eps), b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        s, weight = ctx.saved_tensors
        if ctx.drop is None:
            ds, dg, db = layernorm_bwd(s, weight, dy, ctx.eps)
            dadd = ds if ctx.has_b else None
        else:
            p_drop, seed, site = ctx.drop
            ds, dadd, dg, db = layernorm_drop_bwd(s, weight, dy, ctx.eps, p_drop, seed, site_out=site)
        return ds, dadd, dg.to(weight.dtype), db.to(weight.dtype), None, None, None, None


def add_layernorm_train(a, b, weight, bias, eps, p_drop: float = 0.0, seed: int = 0, site: int = 0):
    """Differentiable `add_layernorm` -> a new contiguous [rows, d].  p_drop > 0: LayerNorm(a + dropout(b)), the dropout of
    hidden site `site` fused into the kernels (`seed`: `bert_hidden_seed` of the call's seed); p_drop == 0: as before."""
    return _AddLayerNorm.apply(a, b, weight, bias, eps, p_drop, seed, site)


def embed_grad_sorted(ds, plan: EmbedGradPlan, table_rows: int, padding_idx=None):
    """The gradient of an embedding table from ds [T, d] (bf16 / fp16) and the plan of the T ids (`embed_grad_plan`, on ds's device:
    `embed_grad_plan_to`) -> a new zero-filled [table_rows, d] of ds's dtype with every row that occurs in the ids written once
    (row `padding_idx` stays zero).  No atomics and no f32 table; the order of every sum follows from the ids alone, so equal
    inputs give equal bits: per chunk of the plan the rows of ds are added one after the other in f32, in ascending packed-token
    order, onto 0; an id with one chunk is rounded once; an id with several chunks has its f32 chunk sums added one after the
    other in chunk order onto 0 (second launch) and rounded once."""
    lib = _lib.load()
    T, d = ds.shape
    if plan.order.shape[0] != T:
        raise ValueError("embed_grad_sorted: the plan was built for another number of tokens")
    ds = ds if ds.stride(1) == 1 and ds.stride(0) % 8 == 0 and ds.data_ptr() % 16 == 0 else ds.contiguous()
    out = torch.zeros((table_rows, d), dtype=ds.dtype, device=ds.device)
    if T == 0:
        return out
    ws_elems = lib.rpo_embed_grad_workspace_elems(plan.n_partials, d)
    ws = torch.empty((ws_elems,), dtype=torch.float32, device=ds.device) if ws_elems else None
    with torch.cuda.device(ds.device):
        check(lib.rpo_embed_grad_sorted(ds.data_ptr(), ds.stride(0), T, d, _dt(ds), plan.order.data_ptr(), plan.chunks.data_ptr(),
                                        plan.chunks.shape[0], plan.multi.data_ptr() if plan.multi.shape[0] else None,
                                        plan.multi.shape[0], plan.n_partials, out.data_ptr(), d, table_rows,
                                        -1 if padding_idx is None else int(padding_idx), _p(ws), ws_elems, _stream(ds)),
              "rpo_embed_grad_sorted")
    return out


class _BertEmbedLayerNorm(torch.autograd.Function):
    """`bert_embed_ln` with a backward: the LayerNorm backward kernel, then ds scattered into the three tables.  plans: None, or the
    `EmbedGradPlan`s (word, position, token type or None) of ids / pos / token_types on the device: the table gradients then come
    from `embed_grad_sorted`."""

    @staticmethod
    def forward(ctx, ids, pos, token_types, word, type_emb, pos_emb, weight, bias, eps, padding_idx, p_drop=0.0, seed=0,
                plans=None):
        lib = _lib.load()
        T, d = ids.shape[0], word.shape[1]
        for t in (word, type_emb, pos_emb):
            if not t.is_contiguous():
                raise ValueError("bert_embed_ln_train: embedding tables must be contiguous")
        y = torch.empty((T, d), dtype=word.dtype, device=word.device)
        s = torch.empty((T, d), dtype=word.dtype, device=word.device)
        ctx.drop = (float(p_drop), int(seed), bert_hidden_site()) if p_drop > 0 else None
        with torch.cuda.device(word.device):
            if ctx.drop is None:
                check(lib.rpo_bert_embed_ln_train_fwd(ids.data_ptr(), _p(token_types), pos.data_ptr(), T, word.data_ptr(),
                                                      word.shape[0], type_emb.data_ptr(), type_emb.shape[0], pos_emb.data_ptr(),
                                                      pos_emb.shape[0], weight.data_ptr(), bias.data_ptr(), float(eps),
                                                      y.data_ptr(), d, s.data_ptr(), d, d, _dt(word), _stream(word)),
                      "rpo_bert_embed_ln_train_fwd")
            else:
                check(lib.rpo_bert_embed_ln_drop_fwd(ids.data_ptr(), _p(token_types), pos.data_ptr(), T, word.data_ptr(),
                                                     word.shape[0], type_emb.data_ptr(), type_emb.shape[0], pos_emb.data_ptr(),
                                                     pos_emb.shape[0], weight.data_ptr(), bias.data_ptr(), float(eps),
                                                     y.data_ptr(), d, s.data_ptr(), d, d, _dt(word), *ctx.drop, _stream(word)),
                      "rpo_bert_embed_ln_drop_fwd")
        ctx.save_for_backward(s, weight, ids, pos, token_types)
        ctx.eps, ctx.padding_idx = float(eps), padding_idx
        ctx.tables = (word.shape, type_emb.shape, pos_emb.shape)
        ctx.plans = plans
        return y

    @staticmethod
    def backward(ctx, dy):
        s, weight, ids, pos, token_types = ctx.saved_tensors
        if ctx.drop is None:
            ds, dg, db = layernorm_bwd(s, weight, dy, ctx.eps)
        else:
            p_drop, seed, site = ctx.drop
            ds, _, dg, db = layernorm_drop_bwd(s, weight, dy, ctx.eps, p_drop, seed, site_in=site)
        if ctx.plans is not None:
            # the deterministic form: every touched table row is one f32 sum in an order fixed by the ids, written once in the
            # storage dtype (`embed_grad_sorted`); no f32 table
            p_word, p_pos, p_type = ctx.plans
            dword = dpos = dtype_emb = None
            if ctx.needs_input_grad[3]:
                dword = embed_grad_sorted(ds, p_word, ctx.tables[0][0], ctx.padding_idx)
            if ctx.needs_input_grad[4]:
                if token_types is None:                    # type 0 for every token: one row, a deterministic reduction already
                    dtype_emb = torch.zeros(ctx.tables[1], dtype=s.dtype, device=ds.device)
                    dtype_emb[0] = ds.float().sum(0).to(s.dtype)
                else:
                    dtype_emb = embed_grad_sorted(ds, p_type, ctx.tables[1][0])
            if ctx.needs_input_grad[5]:
                dpos = embed_grad_sorted(ds, p_pos, ctx.tables[2][0])
            return (None, None, None, dword, dtype_emb, dpos, dg.to(weight.dtype), db.to(weight.dtype), None, None, None, None,
                    None)
        # Embedding gradient = plumbing: stock index_add_ of ds into f32 tables.  It is atomic-based (the order of the adds into one
        # row is not fixed), like the padded path's own embedding backward; every other gradient of the native step is deterministic.
        # Cost: one dense f32 [rows, d] table per embedding and call plus its storage-dtype copy (the word table of XLM-R /
        # bge-m3, 250002 x 1024: 1 GB f32 + 0.5 GB): twice the bytes of the padded path's storage-dtype dense gradient, bought
        # for sums of many token rows that do not round after every add.
        ds32 = ds.float()

        def scatter(shape, idx):
            return torch.zeros(shape, dtype=torch.float32, device=ds.device).index_add_(0, idx.long(), ds32)
        dword = dpos = dtype_emb = None
        if ctx.needs_input_grad[3]:
            dword = scatter(ctx.tables[0], ids)
            if ctx.padding_idx is not None:
                dword[ctx.padding_idx].zero_()             # nn.Embedding(padding_idx=..) keeps that row's gradient at zero
            dword = dword.to(s.dtype)
        if ctx.needs_input_grad[4]:
            if token_types is None:                        # type 0 for every token
                dtype_emb = torch.zeros(ctx.tables[1], dtype=torch.float32, device=ds.device)
                dtype_emb[0] = ds32.sum(0)
            else:
                dtype_emb = scatter(ctx.tables[1], token_types)
            dtype_emb = dtype_emb.to(s.dtype)
        if ctx.needs_input_grad[5]:
            dpos = scatter(ctx.tables[2], pos).to(s.dtype)
        return None, None, None, dword, dtype_emb, dpos, dg.to(weight.dtype), db.to(weight.dtype), None, None, None, None, None


def bert_embed_ln_train(ids, pos, token_types, word, type_emb, pos_emb, weight, bias, eps, padding_idx=None, p_drop: float = 0.0,
                        seed: int = 0, plans=None):
    """Differentiable `bert_embed_ln` (gradients to the three tables and the LayerNorm parameters).  p_drop > 0: the output is
    dropped (hidden site 0, `seed`: `bert_hidden_seed` of the call's seed) inside the kernels; p_drop == 0: as before.
    plans = (word, position, token type or None) `EmbedGradPlan`s of ids / pos / token_types on the device: the table gradients
    are `embed_grad_sorted`'s (bit-reproducible, no f32 table); None: the stock atomic scatter."""
    if plans is not None and (len(plans) != 3 or plans[0] is None or plans[1] is None or (plans[2] is None) != (token_types is None)):
        raise ValueError("bert_embed_ln_train: plans = (word, position, token type) plans, the last None exactly when token_types is")
    return _BertEmbedLayerNorm.apply(ids, pos, token_types, word, type_emb, pos_emb, weight, bias, eps, padding_idx, p_drop, seed,
                                     plans)


def gelu_out(u):
    """Exact erf GELU out of place over a 2-D row-strided u -> a new contiguous tensor (u survives for the backward)."""
    lib = _lib.load()
    if u.dim() != 2 or u.stride(1) != 1:
        raise ValueError("gelu_out: 2-D with contiguous rows")
    h = torch.empty(u.shape, dtype=u.dtype, device=u.device)
    with torch.cuda.device(u.device):
        check(lib.rpo_gelu_out_fwd(u.data_ptr(), u.stride(0), h.data_ptr(), h.stride(0), u.shape[0], u.shape[1], _dt(u),
                                   _stream(u)), "rpo_gelu_out_fwd")
    return h


def gelu_bwd(u, dh):
    """du = dh * (Phi(u) + u phi(u)) -> a new contiguous tensor."""
    lib = _lib.load()
    dh = dh if dh.stride(1) == 1 and dh.stride(0) % 8 == 0 and dh.data_ptr() % 16 == 0 else dh.contiguous()
    du = torch.empty(u.shape, dtype=u.dtype, device=u.device)
    with torch.cuda.device(u.device):
        check(lib.rpo_gelu_bwd(u.data_ptr(), u.stride(0), dh.data_ptr(), dh.stride(0), du.data_ptr(), du.stride(0), u.shape[0],
                               u.shape[1], _dt(u), _stream(u)), "rpo_gelu_bwd")
    return du


class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u):
        ctx.save_for_backward(u)
        return gelu_out(u)

    @staticmethod
    def backward(ctx, dh):
        (u,) = ctx.saved_tensors
        return gelu_bwd(u, dh)


def gelu(u):
    """Differentiable exact erf GELU (HIP forward and backward)."""
    return _Gelu.apply(u)


# ------------------------------------------------------------------------------------------------
# (8) exact top-k over score chunks (retrieval, "next" row f3)
# ------------------------------------------------------------------------------------------------
TOPK_MAX_K = 1024


def _winners_ok(best_val, best_idx, lists: int, k: int) -> bool:
    """best_val / best_idx are contiguous f32 / int64 [lists, k]."""
    return best_val.shape == (lists, k) and best_idx.shape == (lists, k) and best_val.is_contiguous() and best_idx.is_contiguous() \
        and best_val.dtype == torch.float32 and best_idx.dtype == torch.int64


def topk_merge(scores, col0: int, best_val=None, best_idx=None, k: int = 100, split: int = 1):
    """Merges the top-k of `scores` ([rows, cols] f32 / bf16 / fp16, the chunk of corpus rows [col0, col0 + cols)) into the winners
    so far (`best_val` f32 [rows * split, k], `best_idx` int64 [rows * split, k]; None: start).  Order: value descending, ties by
    the smaller corpus index.  split > 1: `split` winner lists per score row, list r * split + s over a column segment of the
    chunk (rpo_topk_merge_split: more blocks than query rows); `topk_finish` merges them at the end of the search.  Returns
    (best_val, best_idx), updated in place when given."""
    _need_gpu(scores)
    lib = _lib.load()
    if scores.dim() != 2 or scores.stride(1) != 1:
        raise ValueError("topk_merge: scores must be [rows, cols] with contiguous columns")
    if not 0 < k <= TOPK_MAX_K:
        raise ValueError(f"topk_merge: k must be in 1..{TOPK_MAX_K}")
    if split < 1:
        raise ValueError("topk_merge: split >= 1")
    rows, cols = scores.shape
    first = best_val is None
    if first:
        best_val = torch.empty((rows * split, k), dtype=torch.float32, device=scores.device)
        best_idx = torch.empty((rows * split, k), dtype=torch.int64, device=scores.device)
    elif not _winners_ok(best_val, best_idx, rows * split, k):
        raise ValueError("topk_merge: best_val / best_idx must be contiguous f32 / int64 [rows * split, k]")
    with torch.cuda.device(scores.device):
        check(lib.rpo_topk_merge_split(scores.data_ptr(), scores.stride(0), rows, cols, int(col0), k, _dt(scores), int(split),
                                       best_val.data_ptr(), best_idx.data_ptr(), int(first), _stream(scores)),
              "rpo_topk_merge_split")
    return best_val, best_idx


def topk_finish(best_val, best_idx, split: int):
    """[rows * split, k] winner lists -> [rows, k]: the k best of a row's `split` lists, value descending, ties by the smaller
    corpus index (the lists are disjoint column ranges, so this IS the row's top-k).  rows x split x k elements: two stable sorts."""
    if split == 1:
        return best_val, best_idx
    k = best_val.shape[1]
    v = best_val.view(-1, split * k)
    i = best_idx.view(-1, split * k)
    o = torch.sort(i, dim=1, stable=True).indices                    # index ascending ...
    v, i = v.gather(1, o), i.gather(1, o)
    o = torch.sort(v, dim=1, descending=True, stable=True).indices   # ... then value descending, stable: ties keep the smaller index first
    return v.gather(1, o)[:, :k].contiguous(), i.gather(1, o)[:, :k].contiguous()


TOPK_SLOTS = 4096           # topk.hip: kTopkSlots (winners + candidates of one re-selection)


def search_candidate_cap(k: int) -> int:
    """Candidate slots per query row and corpus chunk of the fused search step: a chunk as large as everything seen before it brings
    ~k survivors per row on average (exchangeable scores); 3 k, at least 1024, leaves overflow to adversarial corpora (which fall
    back to the score-matrix path: FlatIPIndex.search)."""
    return max(1, min(TOPK_SLOTS - k, max(1024, 3 * k)))


def search_filter_ok(nq: int, rows: int, d: int) -> bool:
    """rpo_sim_topk_filter_ok: a bf16 [nq, d] x [rows, d] problem is one the 256 x 256 scoring kernel takes (shape only)."""
    return bool(_lib.load().rpo_sim_topk_filter_ok(int(nq), int(rows), int(d)))


def _frame_takes(q, p, dtypes, cols_per_d: int, shape_ok) -> bool:
    """Operands of the 256 x 256 frame: two contiguous, 16-byte aligned [rows, cols_per_d * d] matrices of one of `dtypes`, and a
    problem the C shape predicate `shape_ok(Q, P, d)` admits."""
    if not (q.dtype in dtypes and p.dtype == q.dtype and q.dim() == 2 and p.dim() == 2 and q.is_contiguous() and p.is_contiguous()
            and q.shape[1] == p.shape[1] and q.shape[1] % cols_per_d == 0 and q.data_ptr() % 16 == 0 and p.data_ptr() % 16 == 0):
        return False
    return bool(shape_ok(q.shape[0], p.shape[0], q.shape[1] // cols_per_d))


def search_filter_takes(q, p) -> bool:
    """Shapes rpo_sim_topk_filter takes: bf16 (or, with f32 scores, fp16) rows, 16-byte aligned, and a problem `similarity` scores
    with the same 256 x 256 kernel (rpo_sim_topk_filter_ok: > 64 query rows, d % 64 == 0, >= 192 tiles, operands below 4 GB) -- so
    the fused step changes no bit."""
    return _frame_takes(q, p, (torch.bfloat16, torch.float16), 1, _lib.load().rpo_sim_topk_filter_ok)


class SearchWorkspace:
    """Candidate lists of the fused search step for `rows` query rows: values, corpus indices, per-row counters (zero between steps)
    and the overflow flag."""

    def __init__(self, rows: int, k: int, device):
        self.rows, self.k, self.cap = rows, k, search_candidate_cap(k)
        self.cand_val = torch.empty((rows, self.cap), dtype=torch.float32, device=device)
        self.cand_idx = torch.empty((rows, self.cap), dtype=torch.int64, device=device)
        self.cand_cnt = torch.zeros((rows,), dtype=torch.int32, device=device)
        self.overflow = torch.zeros((1,), dtype=torch.int32, device=device)


def similarity_f32(q, p):
    """f32 scores [Q, P] of bf16 (or fp16) operands, UNROUNDED f32 sums in the 256 x 256 scoring frame's summation order (rpo_sim_scores_f32):
    the score matrix of an f32 index whose embeddings are exact in bf16 (retrieval.FlatIPIndex).  Shapes: search_filter_takes."""
    _need_gpu(q, p)
    if not search_filter_takes(q, p):
        raise ValueError("similarity_f32: bf16 [rows, d] operands of a shape the 256 x 256 scoring kernel takes (search_filter_takes)")
    return _scores_f32("rpo_sim_scores_f32", q, p, q.shape[1], _dt(q))


def _scores_f32(entry: str, q, p, d: int, *dtype):
    """f32 [Q, P] out of the frame's score-matrix entry `entry` (rpo_sim_scores_f32 takes the operands' dtype behind d, the plane
    entry none); the caller has asked the operand predicate."""
    scores = torch.empty((q.shape[0], p.shape[0]), dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device):
        check(getattr(_lib.load(), entry)(q.data_ptr(), p.data_ptr(), q.shape[0], p.shape[0], d, *dtype, scores.data_ptr(),
                                          scores.stride(0), _stream(q)), entry)
    return scores


def _search_step(who: str, entry: str, q, p, d: int, dtype, col0: int, round_scores, best_val, best_idx, ws):
    """The fused step behind `search_step` / `search_step_planes`: the workspace check, the filter entry `entry` on [rows, d] x
    [P, d] (`dtype` / `round_scores`: the arguments rpo_sim_topk_filter has behind d and behind k, empty for the plane entry), and
    rpo_topk_merge_candidates.  The caller has asked the operand predicate."""
    lib = _lib.load()
    rows, k = q.shape[0], best_val.shape[1]
    if (ws.rows, ws.k) != (rows, k) or not _winners_ok(best_val, best_idx, rows, k):
        raise ValueError(f"{who}: best_val / best_idx must be contiguous f32 / int64 [rows, k] matching the workspace")
    with torch.cuda.device(q.device):
        st = _stream(q)
        check(getattr(lib, entry)(q.data_ptr(), p.data_ptr(), rows, p.shape[0], d, *dtype, int(col0), k, *round_scores,
                                  best_val.data_ptr(), best_idx.data_ptr(), ws.cand_val.data_ptr(), ws.cand_idx.data_ptr(),
                                  ws.cand_cnt.data_ptr(), ws.cap, st), entry)
        check(lib.rpo_topk_merge_candidates(ws.cand_val.data_ptr(), ws.cand_idx.data_ptr(), ws.cand_cnt.data_ptr(), rows, ws.cap, k,
                                            best_val.data_ptr(), best_idx.data_ptr(), ws.overflow.data_ptr(), st),
              "rpo_topk_merge_candidates")
    return best_val, best_idx


def search_step(q, p, col0: int, best_val, best_idx, ws: SearchWorkspace, round_scores: bool = True):
    """One corpus chunk of the exact search WITHOUT its score matrix: rpo_sim_topk_filter (scores in the MFMA accumulators, survivors of
    each row's k-th winner appended to the row's candidate list) + rpo_topk_merge_candidates (lists -> winners).  best_val / best_idx
    [rows, k] are updated in place and must hold k real winners per row; `ws.overflow` is raised when a list ran over (the result is
    then incomplete: the caller redoes the search through `similarity` + `topk_merge`).  round_scores: the score is the sum rounded
    to bf16 once (what `similarity` stores for a bf16 index); False: the f32 sum itself (an f32 index exact in bf16: `similarity_f32`)."""
    _need_gpu(q, p)
    if not search_filter_takes(q, p) or (q.dtype == torch.float16 and round_scores):
        raise ValueError("search_step: bf16 [rows, d] operands (fp16 with round_scores=False) of a shape the 256 x 256 scoring kernel takes "
                         "(search_filter_takes)")
    return _search_step("search_step", "rpo_sim_topk_filter", q, p, q.shape[1], (_dt(q),), col0, (int(bool(round_scores)),),
                        best_val, best_idx, ws)


# ---- the same search on three bf16 planes of f32 operands (an f32 index that is exact in neither 16-bit type) ----
def split_bf16x3_ref(x):
    """Pure-torch statement of `split_bf16x3` (works on CPU tensors; what the kernel is tested against): (planes bf16 [..., 3 d] = h | m | l, inexact bool scalar tensor) with
    h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), round to nearest even, residuals in f32.  inexact: some element is not finite,
    its planes do not add up to it in f32, or a plane is a bf16 subnormal (the frame's premise is planes that are normal or zero)."""
    x = x.float()
    h = x.to(torch.bfloat16)
    r1 = x - h.float()
    m = r1.to(torch.bfloat16)
    r2 = r1 - m.float()
    l = r2.to(torch.bfloat16)
    planes = torch.cat([h, m, l], dim=-1)
    tiny = torch.finfo(torch.bfloat16).tiny                           # 2^-126, the smallest normal (bf16 has f32's exponent range)
    mag = planes.float().abs()
    sub = (mag > 0) & (mag < tiny)
    inexact = (~torch.isfinite(x)).any() | ~((h.float() + m.float() + l.float()) == x).all() | sub.any()
    return planes, inexact


def split_bf16x3(x):
    """(planes bf16 [rows, 3 d] = h | m | l per row, inexact int32 [1] device flag) of x f32 [rows, d], d % 64 == 0 (rpo_split_bf16x3;
    in torch: split_bf16x3_ref).  The flag is nonzero when the planes do not represent x exactly; reading it is the caller's sync."""
    _need_gpu(x)
    lib = _lib.load()
    if x.dtype != torch.float32 or x.dim() != 2 or not x.is_contiguous() or x.shape[0] == 0 or x.shape[1] % 64 != 0 or x.data_ptr() % 16:
        raise ValueError("split_bf16x3: contiguous, 16-byte aligned f32 [rows, d] with rows > 0 and d % 64 == 0")
    rows, d = x.shape
    planes = torch.empty((rows, 3 * d), dtype=torch.bfloat16, device=x.device)
    flag = torch.zeros((1,), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.rpo_split_bf16x3(x.data_ptr(), d, rows, d, planes.data_ptr(), 3 * d, flag.data_ptr(), _stream(x)), "rpo_split_bf16x3")
    return planes, flag


def search_planes_takes(qp, cp) -> bool:
    """Shapes the plane-walking frame takes: bf16 [rows, 3 d] planes (split_bf16x3), contiguous and 16-byte aligned, of a problem
    rpo_sim_planes_ok admits: search_filter_takes' shapes applied to d, each operand's planes below 4 GB."""
    return _frame_takes(qp, cp, (torch.bfloat16,), 3, _lib.load().rpo_sim_planes_ok)


def similarity_f32_planes(qp, cp):
    """f32 scores [Q, P] of f32 operands given as bf16 planes: exact products of the six leading plane pairs, f32 sums in the
    256 x 256 frame's order, smallest terms first (rpo_sim_scores_f32_planes).  Shapes: search_planes_takes."""
    _need_gpu(qp, cp)
    if not search_planes_takes(qp, cp):
        raise ValueError("similarity_f32_planes: bf16 [rows, 3 d] planes of a shape the plane-walking frame takes (search_planes_takes)")
    return _scores_f32("rpo_sim_scores_f32_planes", qp, cp, qp.shape[1] // 3)


def search_step_planes(qp, cp, col0: int, best_val, best_idx, ws: SearchWorkspace):
    """`search_step(round_scores=False)` on planes: rpo_sim_topk_filter_planes + rpo_topk_merge_candidates; the scores are those of
    `similarity_f32_planes`, bit for bit."""
    _need_gpu(qp, cp)
    if not search_planes_takes(qp, cp):
        raise ValueError("search_step_planes: bf16 [rows, 3 d] planes of a shape the plane-walking frame takes (search_planes_takes)")
    return _search_step("search_step_planes", "rpo_sim_topk_filter_planes", qp, cp, qp.shape[1] // 3, (), col0, (), best_val, best_idx, ws)


__all__ = ["sim_gemm_nt", "pool_normalize", "topk_merge", "topk_finish", "search_step", "similarity_f32", "search_filter_takes", "search_filter_ok", "SearchWorkspace",
           "split_bf16x3", "split_bf16x3_ref", "similarity_f32_planes", "search_step_planes", "search_planes_takes",
           "search_candidate_cap", "linear", "transpose2d", "wgrad", "infonce_loss", "similarity", "rankpo_loss_metrics", "RankPOConfig", "METRIC_KEYS",
           "swiglu_down", "rope_", "fused_encoder_ops_ok", "add_rmsnorm", "fused_norm_ok",
           "flash_attn_varlen", "flash_attn_varlen_qkv", "last_query_attn", "last_query_attn_ok", "rope_flash_attn_varlen_qkv", "rope_flash_attn_varlen_qkv_fwd", "flash_attn_varlen_fwd", "flash_attn_varlen_bwd", "attn_tile_table", "attn_fwd_tile_table", "recomputing",
           "attn_key_tile_table"]
