"""Minimal training step around the hot path ("next" row f2 of SURVEY.md §8; reference: HF Trainer loop copied in
contrastive_trainer.py:487-612 + DeepSpeed ZeRO-1 bf16, scripts/train/run_contrastive.sh:33-44).

  micro-steps:  loss = model(**batch)["loss"]; loss.backward()      (GAS of them, negatives are per micro-batch)
  boundary:     gradient mean over ranks  (FlatGradAllReducer: async bucketed RCCL all-reduce during backward; or, with
                `partition_optimizer`, reduce-scatter + AdamW on this rank's 1 / W of the state + all-gather of the parameters)
                global-norm clip (1.0)   -> one device scalar, no host sync
                AdamW (lr 1e-5, cosine, warmup 0.1) -> ONE rpo_adamw_step launch over the flat parameter space
                (bf16 parameters + f32 master / m / v), gradients zeroed by one memset.

fp16 parameters (the reference's BGE run, configs/ds_zero1_config_bge.json) train under DeepSpeed's dynamic loss scaler, kept
on the device: `micro_step` backpropagates loss * scale with the scale read from a device state block, the gradient sum of
squares (always taken: it is the overflow check) feeds ONE one-thread launch (rpo_loss_scale_update) that decides skip / clip
factor / next scale, and rpo_adamw_step_scaled obeys that block.  No host read anywhere: `TrainStep.loss_scale_state()` is the
only call that syncs.  Update rule (`LossScaleConfig`; growth factor 2):

    on overflow:  if hysteresis == 1 or cur_hysteresis == 1: scale = max(scale / 2, min_scale)   else: cur_hysteresis -= 1
                  good_steps = 0;  the step is skipped (parameters, master, m, v untouched)
    else:         good_steps += 1;  if consecutive_hysteresis: cur_hysteresis = hysteresis
                  if good_steps % window == 0: { if not consecutive_hysteresis: cur_hysteresis = hysteresis;  scale *= 2 }

Deliberate deviation from DeepSpeed: the LR schedule advances with `global_step` on skipped steps too (DeepSpeed holds its
scheduler on a skipped step).  Holding it needs the skip verdict on the host, i.e. a sync per step; the price of not syncing is
a few warm-up steps at the start of a run, while the initial scale comes down.  Bias correction is NOT affected: it follows
the device's count of applied steps.  An overflow at the minimum scale, where DeepSpeed raises, is counted (`floor_hits`).

Everything here is stream-ordered; `step()` returns the detached device loss so that logging decides when to sync.
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass
from typing import Callable, Dict, Iterable, Optional, Union

import torch
import torch.distributed as dist
from torch import nn

from . import _lib
from ._lib import (RPO_DT_BF16, RPO_DT_F16, RPO_DT_F32, RPO_LS_APPLIED_STEPS, RPO_LS_CUR_HYSTERESIS, RPO_LS_FLOOR_HITS,
                   RPO_LS_GOOD_STEPS, RPO_LS_NORM, RPO_LS_SCALE, RPO_LS_SKIPPED_STEPS, RPO_LS_WORDS, check)
from .distributed import FlatGradAllReducer


def cosine_with_warmup(step: int, total_steps: int, warmup_steps: int) -> float:
    """transformers' get_cosine_schedule_with_warmup multiplier (lr_scheduler_type cosine, warmup_ratio 0.1)."""
    if step < warmup_steps:
        return step / max(1, warmup_steps)
    prog = (step - warmup_steps) / max(1, total_steps - warmup_steps)
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * prog)))


@dataclass
class LossScaleConfig:
    """fp16 loss scaling, DeepSpeed's knobs (the "fp16" block of its config).  Defaults = the reference's BGE run
    (configs/ds_zero1_config_bge.json:2-11).  dynamic=False: the scale stays at `init_scale`; an overflow still skips the step."""
    init_scale: float = 2.0 ** 16
    window: int = 1000
    hysteresis: int = 2
    consecutive_hysteresis: bool = False
    min_scale: float = 1.0
    dynamic: bool = True

    def __post_init__(self):
        if not (self.init_scale > 0 and math.isfinite(self.init_scale)):
            raise ValueError(f"loss scale must be positive and finite, got {self.init_scale}")
        if self.window < 1 or self.hysteresis < 1 or not self.min_scale > 0:
            raise ValueError(f"loss scale window and hysteresis must be >= 1 and min_scale > 0, got {self}")

    @classmethod
    def from_deepspeed(cls, path_or_dict) -> "LossScaleConfig":
        """From a DeepSpeed config (a path or the parsed dict) with an "fp16" block: loss_scale 0 = dynamic from
        2^initial_scale_power, anything else = static at that value.  Keys missing from the block take DeepSpeed's defaults; a
        config without the block, or a non-numeric value such as "auto", is a ValueError."""
        cfg = path_or_dict
        if not isinstance(cfg, dict):
            with open(cfg) as f:
                cfg = json.load(f)
        f16 = cfg.get("fp16") if isinstance(cfg, dict) else None
        if not isinstance(f16, dict):
            raise ValueError('LossScaleConfig.from_deepspeed: the config has no "fp16" block')

        def num(key, default, kind):
            v = f16.get(key, default)
            if isinstance(v, bool) or not isinstance(v, (int, float)):       # e.g. "auto": the launcher's to fill in, not ours
                raise ValueError(f'LossScaleConfig.from_deepspeed: fp16.{key} must be a number, got {v!r}')
            return kind(v)
        static = num("loss_scale", 0, float)
        return cls(init_scale=static if static > 0 else 2.0 ** num("initial_scale_power", 16, int),
                   window=num("loss_scale_window", 1000, int), hysteresis=num("hysteresis", 2, int),
                   consecutive_hysteresis=bool(f16.get("consecutive_hysteresis", False)),
                   min_scale=num("min_loss_scale", 1, float), dynamic=not static > 0)

    @classmethod
    def resolve(cls, loss_scale, dtype) -> Optional["LossScaleConfig"]:
        """The `loss_scale` argument of FlatAdamW / TrainStep: None | float (static) | "dynamic" | LossScaleConfig.  fp16
        parameters default to the reference's dynamic configuration; bf16 / f32 parameters take no loss scale."""
        if dtype != torch.float16:
            if loss_scale is not None:
                raise ValueError(f"loss_scale is for float16 parameters; {dtype} parameters take loss_scale=None")
            return None
        if loss_scale is None or (isinstance(loss_scale, str) and loss_scale == "dynamic"):
            return cls()
        if isinstance(loss_scale, cls):
            return loss_scale
        if isinstance(loss_scale, (int, float)) and not isinstance(loss_scale, bool):
            return cls(init_scale=float(loss_scale), dynamic=False)
        raise ValueError(f"loss_scale must be None, a number, 'dynamic' or a LossScaleConfig, got {loss_scale!r}")


_LS_INT_KEYS = (("cur_hysteresis", RPO_LS_CUR_HYSTERESIS), ("good_steps", RPO_LS_GOOD_STEPS),
                ("applied_steps", RPO_LS_APPLIED_STEPS), ("skipped_steps", RPO_LS_SKIPPED_STEPS), ("floor_hits", RPO_LS_FLOOR_HITS))


class FlatAdamW:
    """AdamW over one flat parameter buffer; parameters and gradients are views into flat storage.

    partition=True (with more than one rank): the optimizer state is PARTITIONED over the ranks, the xGMI-native form of what the
    reference configures as DeepSpeed ZeRO stage 1 (configs/ds_zero1_config_llama.json:10-12).  Every gradient bucket is
    reduce-scattered instead of all-reduced (rank r gets the summed shard r of every bucket), rank r keeps float32 master / m / v
    for ITS shards only (12 B/parameter / W instead of 12 B/parameter: 90 GB -> 11 GB per GPU for Llama-3-8B at W = 8) and runs
    AdamW on them, then the bf16 parameters are all-gathered bucket by bucket.  Bytes on the wire = the all-reduce's (a ring
    all-reduce IS a reduce-scatter + an all-gather).  Same sums, same element-wise update as the replicated path; the global
    gradient norm is summed shard-wise first, so the two paths agree to float32 summation order (the 2- / 4-rank tests assert
    equal parameters after 3 steps to that tolerance, and identical replicas)."""

    def __init__(self, params: Iterable[nn.Parameter], lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 max_grad_norm: Optional[float] = 1.0, bucket_mb: float = 512.0, force_collectives: bool = False,
                 partition: bool = False, loss_scale: Union[None, float, str, LossScaleConfig] = None):
        params = list(params)
        dist_on = dist.is_available() and dist.is_initialized()
        self.partition = bool(partition) and dist_on and (dist.get_world_size() > 1 or force_collectives)
        self.reducer = FlatGradAllReducer(params, bucket_mb=bucket_mb, force_collectives=force_collectives, shard=self.partition)
        r = self.reducer
        dev, dtype = r.flat.device, r.flat.dtype
        if dtype not in (torch.bfloat16, torch.float16, torch.float32):
            raise TypeError(f"unsupported parameter dtype {dtype}")
        self.dt = {torch.bfloat16: RPO_DT_BF16, torch.float16: RPO_DT_F16, torch.float32: RPO_DT_F32}[dtype]
        self.scaler = LossScaleConfig.resolve(loss_scale, dtype)          # None unless the parameters are fp16
        low = dtype != torch.float32                                       # 16-bit parameters keep an f32 master copy
        # flat parameter storage in the same layout as the gradients; parameters become views of it
        self.flat_param = torch.zeros(r.numel, dtype=dtype, device=dev)
        for p, o in zip(r.order, r.offsets):
            v = self.flat_param[o:o + p.numel()].view_as(p)
            v.copy_(p.data)
            p.data = v
        # optimizer state: the whole flat space, or (partition) this rank's shard of every bucket, back to back
        n_state = r.shard_numel if self.partition else r.numel
        self.state_numel = n_state
        if self.partition:
            own = torch.cat([self._param_shard(b) for b in range(len(r.buckets))])
            self.master = own.float() if low else None
        else:
            self.master = self.flat_param.float() if low else None
        self.exp_avg = torch.zeros(n_state, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n_state, dtype=torch.float32, device=dev)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.max_grad_norm = max_grad_norm
        self.t = 0
        self._nblk = 1024
        self._partial = torch.empty(self._nblk, dtype=torch.float32, device=dev)
        self.last_grad_norm = None
        # loss-scale state block (include/rankpo_hip.h rpo_ls_word): 16 words, f32 scale / mult / norm + int32 counters
        self.ls_state = None
        if self.scaler is not None:
            self.ls_state = torch.zeros(RPO_LS_WORDS, dtype=torch.int32, device=dev)
            self.load_loss_scale_state({"scale": self.scaler.init_scale, "cur_hysteresis": self.scaler.hysteresis})

    # -- loss-scale state -------------------------------------------------------------------------------------------------------
    @property
    def loss_scale(self) -> Optional[torch.Tensor]:
        """The device scalar (f32) the next backward is scaled by; None without loss scaling."""
        return None if self.ls_state is None else self.ls_state.view(torch.float32)[RPO_LS_SCALE]

    def loss_scale_state(self) -> Dict:
        """Host copy of the scaler's state (SYNCS: one device-to-host copy of the block)."""
        if self.ls_state is None:
            raise RuntimeError("no loss scaling: the parameters are not float16")
        w = self.ls_state.cpu()
        out = {"scale": float(w.view(torch.float32)[RPO_LS_SCALE])}
        out.update({k: int(w[i]) for k, i in _LS_INT_KEYS})
        return out

    def load_loss_scale_state(self, state: Dict):
        """Set the block from a `loss_scale_state()` dict (missing counters = 0); the per-step words (skip, mult, norm) reset."""
        if self.ls_state is None:
            raise RuntimeError("no loss scaling: the parameters are not float16")
        w = torch.zeros(RPO_LS_WORDS, dtype=torch.int32)
        w.view(torch.float32)[RPO_LS_SCALE] = float(state["scale"])
        for k, i in _LS_INT_KEYS:
            w[i] = int(state.get(k, 0))
        self.ls_state.copy_(w)

    def _param_shard(self, b: int) -> torch.Tensor:
        """This rank's slice of bucket b of the flat parameter buffer."""
        r = self.reducer
        s, e, _ = r.buckets[b]
        n = (e - s) // r.world
        return self.flat_param[s + r.rank * n:s + (r.rank + 1) * n]

    # -- the three kernel calls (tensors in, launch on the current stream); the CPU tests of the partition logic replace them ------
    def _sumsq(self, g: torch.Tensor) -> torch.Tensor:
        """sum of squares of g as a device scalar (f32)."""
        if not g.is_cuda:
            raise RuntimeError("FlatAdamW runs on a HIP device only (no CPU fallback)")
        lib = _lib.load()
        with torch.cuda.device(g.device):
            check(lib.rpo_sumsq_partial(g.data_ptr(), g.numel(), self.dt, self._partial.data_ptr(), self._nblk,
                                        torch.cuda.current_stream(g.device).cuda_stream), "rpo_sumsq_partial")
        return self._partial.sum()

    def _scale_update(self, ss: torch.Tensor, pre_scale: float):
        """fp16 only.  ss: device f32 [1], the sum of squares of the SCALED gradient over all ranks.  Rewrites `ls_state`: skip,
        norm, mult for this step; scale, hysteresis and counters for the next (rpo_loss_scale_update)."""
        if not ss.is_cuda:
            raise RuntimeError("FlatAdamW runs on a HIP device only (no CPU fallback)")
        c = self.scaler
        with torch.cuda.device(ss.device):
            check(_lib.load().rpo_loss_scale_update(ss.data_ptr(), self.ls_state.data_ptr(), pre_scale,
                                                    self.max_grad_norm if self.max_grad_norm is not None else 0.0,
                                                    int(c.dynamic), c.window, c.hysteresis, int(c.consecutive_hysteresis),
                                                    c.min_scale, torch.cuda.current_stream(ss.device).cuda_stream),
                  "rpo_loss_scale_update")

    def _adamw(self, param, master, grad, m, v, lr, bc1, bc2, scale):
        """bc1 / bc2 / scale are None with fp16 parameters: multiplier, skip flag and step count then come from `ls_state`."""
        if not param.is_cuda:
            raise RuntimeError("FlatAdamW runs on a HIP device only (no CPU fallback)")
        lib = _lib.load()
        b1, b2 = self.betas
        if self.scaler is not None:
            with torch.cuda.device(param.device):
                check(lib.rpo_adamw_step_scaled(param.data_ptr(), master.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(),
                                                param.numel(), self.dt, lr, b1, b2, self.eps, self.weight_decay,
                                                self.ls_state.data_ptr(), torch.cuda.current_stream(param.device).cuda_stream),
                      "rpo_adamw_step_scaled")
            return
        with torch.cuda.device(param.device):
            check(lib.rpo_adamw_step(param.data_ptr(), None if master is None else master.data_ptr(), grad.data_ptr(),
                                     m.data_ptr(), v.data_ptr(), param.numel(), self.dt, lr, b1, b2, self.eps, self.weight_decay,
                                     bc1, bc2, scale.data_ptr(), torch.cuda.current_stream(param.device).cuda_stream),
                  "rpo_adamw_step")

    def _grad_sumsq(self) -> torch.Tensor:
        """Sum of squares of the (rank-summed) gradient as a device f32 [1]."""
        if self.partition:
            # every rank holds 1 / W of the summed gradient: local sum of squares, then ONE scalar all-reduce
            ss = self._sumsq(self.reducer.grad_shards).reshape(1).clone()
            dist.all_reduce(ss, op=dist.ReduceOp.SUM)
            return ss
        return self._sumsq(self.reducer.flat).reshape(1)

    def grad_norm(self, pre_scale: float) -> torch.Tensor:
        """||pre_scale * grad||_2 of the (rank-summed) gradient as a device scalar.  With fp16 parameters the stored gradient
        carries the loss scale and may hold inf / NaN: the result is divided by the device scale (non-finite after an overflow);
        `step` itself takes norm and verdict from the state block (`last_grad_norm`), not from here."""
        norm = self._grad_sumsq()[0].sqrt() * pre_scale
        return norm if self.scaler is None else norm / self.loss_scale

    def step(self, grad_scale: float = 1.0, lr_mult: float = 1.0):
        """grad_scale: constant factor on the accumulated gradients (1/GAS/world)."""
        r = self.reducer
        self.t += 1                                                        # ATTEMPTED steps (fp16: the device counts the applied ones)
        lr = self.lr * lr_mult
        if self.scaler is not None:
            # fp16: the sum of squares always runs -- it is the overflow check.  Every rank holds the same all-reduced gradient
            # (replicated state) or the same all-reduced scalar (partitioned state), so every rank's one-thread update reaches
            # the same skip verdict and the same next scale with no further collective.
            self._scale_update(self._grad_sumsq(), grad_scale)
            self.last_grad_norm = self.ls_state.view(torch.float32)[RPO_LS_NORM].clone()    # unscaled; non-finite when skipped
            bc1 = bc2 = scale = None
        else:
            scale = torch.full((1,), grad_scale, dtype=torch.float32, device=r.flat.device)
            if self.max_grad_norm is not None:
                norm = self.grad_norm(grad_scale)
                self.last_grad_norm = norm
                scale = scale * torch.clamp(self.max_grad_norm / (norm + 1e-6), max=1.0)   # clip_grad_norm_ semantics
            b1, b2 = self.betas
            bc1, bc2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
        if not self.partition:
            self._adamw(self.flat_param, self.master, r.flat, self.exp_avg, self.exp_avg_sq, lr, bc1, bc2, scale)
            r.zero_()
            return
        works = []
        for b, (s, e, _) in enumerate(r.buckets):
            o, n = r.shard_offsets[b], (e - s) // r.world
            own = self._param_shard(b)
            self._adamw(own, None if self.master is None else self.master[o:o + n], r.grad_shards[o:o + n],
                        self.exp_avg[o:o + n], self.exp_avg_sq[o:o + n], lr, bc1, bc2, scale)
            works.append(self._all_gather_bucket(b, own))          # in flight while the next bucket's AdamW runs; a skipped
                                                                   # fp16 step gathers the unchanged shards all the same
        self._wait_gathers(works)
        r.zero_()

    def _wait_gathers(self, works):
        """Launch stream waits for the parameter all-gathers (no host sync); a method of its own so that bench.py can bracket it."""
        for w in works:
            if w is not None:
                w.wait()

    def _all_gather_bucket(self, b: int, own: torch.Tensor):
        """Every rank's updated shard of bucket b -> the whole bucket of the flat parameter buffer, on every rank."""
        r = self.reducer
        s, e, _ = r.buckets[b]
        if dist.get_backend() == "nccl":
            # in place: `own` IS slice `rank` of the output (NCCL's in-place all-gather form)
            return dist.all_gather_into_tensor(self.flat_param[s:e], own, async_op=True)
        from .distributed import _all_gather_into
        n = (e - s) // r.world
        _all_gather_into(self.flat_param[s:e].view(r.world, n), own.clone())     # gloo: host tensors, or staged through the host
        return None


class TrainStep:
    """loss_fn(batch) -> scalar loss tensor (e.g. `lambda b: model(**b)["loss"]` or `trainer.compute_loss`)."""

    def __init__(self, params, loss_fn: Callable[[Dict], torch.Tensor], *, lr=1e-5, weight_decay=0.0,
                 max_grad_norm=1.0, gradient_accumulation_steps=1, total_steps=1000, warmup_ratio=0.1,
                 bucket_mb=512.0, force_collectives=False, partition_optimizer=False,
                 loss_scale: Union[None, float, str, LossScaleConfig] = None):
        """loss_scale (float16 parameters only): None or "dynamic" = the reference's dynamic scaler, a number = static, or a
        `LossScaleConfig` (e.g. `LossScaleConfig.from_deepspeed(path)`).  Other parameter dtypes take None."""
        self.opt = FlatAdamW(params, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                             bucket_mb=bucket_mb, force_collectives=force_collectives, partition=partition_optimizer,
                             loss_scale=loss_scale)
        self.loss_fn = loss_fn
        self.gas = gradient_accumulation_steps
        self.total_steps = total_steps
        self.warmup_steps = int(math.ceil(total_steps * warmup_ratio))
        self.global_step = 0
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self._in_optimizer = False       # True while opt.step runs: an exception there leaves half-updated moments (no retry)

    def micro_step(self, batch, last: bool) -> torch.Tensor:
        """Forward + backward of one micro-batch.  Returns the detached, UNSCALED loss in the dtype `loss_fn` returned it in; with
        fp16 parameters the backward runs on `loss.float() * scale` (f32, so the product itself cannot saturate)."""
        if last:
            self.opt.reducer.arm()
        loss = self.loss_fn(batch)
        scale = self.opt.loss_scale
        if scale is None:
            loss.backward()
        else:
            (loss.float() * scale).backward()            # fp16: the device scalar of the state block, no host read
        return loss.detach()

    def loss_scale_state(self) -> Dict:
        """{scale, cur_hysteresis, good_steps, applied_steps, skipped_steps, floor_hits} of the fp16 loss scaler.  SYNCS -- the
        only call of this class that does."""
        return self.opt.loss_scale_state()

    def state_dict(self) -> Dict:
        """Step counters and, with fp16 parameters, the loss scaler's block (syncs).  Parameters and moments are saved by the
        checkpoint code, not here."""
        out = {"global_step": self.global_step, "attempted_steps": self.opt.t}
        if self.opt.scaler is not None:
            out["loss_scale"] = self.opt.loss_scale_state()
        return out

    def load_state_dict(self, state: Dict):
        self.global_step = int(state["global_step"])
        self.opt.t = int(state["attempted_steps"])
        if self.opt.scaler is not None:
            self.opt.load_loss_scale_state(state["loss_scale"])
        elif state.get("loss_scale") is not None:
            raise ValueError("the state holds a loss scale but the parameters are not float16")

    def abort_step(self):
        """After an exception inside `step` (e.g. an out-of-memory error the caller answers by checkpointing more blocks): drop
        the half-accumulated gradients and the reducer's armed state, so that the next `step` starts clean.  The optimizer's
        moments and step count are untouched (the failed step never reached `opt.step`).  An exception that came out of `opt.step`
        itself (the clip-norm or all-gather temporaries running out of memory) is NOT retryable -- master weights and moments may
        be half-updated -- and is refused here: the caller's `except` re-raises."""
        if self._in_optimizer:
            raise RuntimeError("TrainStep.abort_step: the step failed inside the optimizer update; its state may be half-updated and "
                               "the step cannot be retried")
        r = self.opt.reducer
        r.reset()
        for p, o in zip(r.order, r.offsets):                   # every .grad is the parameter's view of the flat buffer again
            p.grad = r.flat[o:o + p.numel()].view_as(p)

    def step(self, batches) -> torch.Tensor:
        """`batches`: a list of GAS micro-batches (or a single batch when GAS == 1)."""
        if isinstance(batches, dict):
            batches = [batches]
        assert len(batches) == self.gas
        tot = None
        for i, b in enumerate(batches):
            l = self.micro_step(b, last=(i == self.gas - 1))
            tot = l if tot is None else tot + l
        inv_world = self.opt.reducer.finish()
        mult = cosine_with_warmup(self.global_step, self.total_steps, self.warmup_steps)   # HF: scheduler steps after the optimizer
        self._in_optimizer = True
        self.opt.step(grad_scale=inv_world / self.gas, lr_mult=mult)
        self._in_optimizer = False
        self.global_step += 1
        return tot / self.gas
