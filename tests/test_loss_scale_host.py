"""CPU tests of fp16 training's host side: `LossScaleConfig` parsing, the construction rules of `FlatAdamW` / `TrainStep` for
float16 parameters, and the step logic around the three kernel calls (`_sumsq`, `_scale_update`, `_adamw`), which torch
stand-ins with the same contract replace here -- as tests/test_host_logic.py does for the bf16 / f32 optimizer -- so that it
runs on CPU tensors and on gloo ranks.

`Rule` below is the specification of the scaler (DeepSpeed's DynamicLossScaler with growth factor 2) in plain Python.  The
stand-in for `_scale_update` applies it to the product's state block; the tests then hold the product's host-visible
behaviour -- `loss_scale_state()`, skipped steps leaving every parameter bit-identical, the attempted-step count, the unscaled
gradient norm, agreement between ranks -- against scripted overflow patterns, with the expected scales also written out as
literals so that the rule itself is pinned.  The HIP kernel is held against the same `Rule` in tests/test_gpu_loss_scale.py."""
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import test_host_logic as H            # the bf16 / f32 stand-ins and the gloo spawning pattern of the existing CPU tests

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DS_CONFIG = os.path.join(ROOT, "tests", "golden", "ds_zero1_config_bge.json")


class Rule:
    """The scaler's update rule, word for word."""

    def __init__(self, cfg):
        self.cfg, self.scale, self.cur_hysteresis = cfg, float(cfg.init_scale), cfg.hysteresis
        self.good_steps = self.applied_steps = self.skipped_steps = self.floor_hits = 0

    def update(self, overflow):
        c = self.cfg
        self.skipped_steps += bool(overflow)
        self.applied_steps += not overflow
        if not c.dynamic:                                    # static: the scale is frozen, an overflow still skips
            return
        if overflow:
            self.floor_hits += self.scale <= c.min_scale
            if c.hysteresis == 1 or self.cur_hysteresis == 1:
                self.scale = max(self.scale / 2, c.min_scale)
            else:
                self.cur_hysteresis -= 1
            self.good_steps = 0
        else:
            self.good_steps += 1
            if c.consecutive_hysteresis:
                self.cur_hysteresis = c.hysteresis
            if self.good_steps % c.window == 0:
                if not c.consecutive_hysteresis:
                    self.cur_hysteresis = c.hysteresis
                self.scale *= 2

    def state(self):
        return {k: (float if k == "scale" else int)(getattr(self, k)) for k in
                ("scale", "cur_hysteresis", "good_steps", "applied_steps", "skipped_steps", "floor_hits")}


def cpu_fp16_kernels(FlatAdamW):
    """torch stand-ins for FlatAdamW's three launches with float16 parameters (rpo_sumsq_partial, rpo_loss_scale_update,
    rpo_adamw_step_scaled; include/rankpo_hip.h (4), (4b)); bf16 / f32 optimizers keep test_host_logic's stand-ins."""
    from rankpo_amd._lib import RPO_LS_APPLIED_STEPS, RPO_LS_MULT, RPO_LS_NORM, RPO_LS_SKIP
    H._cpu_optimizer_kernels(FlatAdamW)
    plain_adamw = FlatAdamW._adamw

    def scale_update(self, ss, pre_scale):
        rule = Rule(self.scaler)
        rule.__dict__.update(self.loss_scale_state())
        ssv, s, mgn = float(ss), rule.scale, self.max_grad_norm
        overflow = not math.isfinite(ssv)
        norm = math.sqrt(ssv) * pre_scale / s
        clip = min(1.0, mgn / (norm + 1e-6)) if mgn is not None and mgn > 0 else 1.0
        rule.update(overflow)
        self.load_loss_scale_state(rule.state())
        f = self.ls_state.view(torch.float32)
        f[RPO_LS_NORM], f[RPO_LS_MULT] = norm, 0.0 if overflow else pre_scale / s * clip
        self.ls_state[RPO_LS_SKIP] = int(overflow)

    def adamw(self, param, master, grad, m, v, lr, bc1, bc2, scale):
        if self.scaler is None:
            return plain_adamw(self, param, master, grad, m, v, lr, bc1, bc2, scale)
        assert bc1 is None and bc2 is None and scale is None      # fp16: everything comes from the state block
        if int(self.ls_state[RPO_LS_SKIP]):
            return
        t, (b1, b2) = int(self.ls_state[RPO_LS_APPLIED_STEPS]), self.betas
        plain_adamw(self, param, master, grad, m, v, lr, 1.0 - b1 ** t, 1.0 - b2 ** t,
                    self.ls_state.view(torch.float32)[RPO_LS_MULT])
    FlatAdamW._scale_update, FlatAdamW._adamw = scale_update, adamw


@pytest.fixture
def cpu_kernels(monkeypatch):
    from rankpo_amd.train_step import FlatAdamW
    for name in ("_sumsq", "_adamw", "_scale_update"):         # restored after the test: the stand-ins are class-wide
        monkeypatch.setattr(FlatAdamW, name, getattr(FlatAdamW, name))
    cpu_fp16_kernels(FlatAdamW)


def _mlp(dtype=torch.float16, seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(24, 40), torch.nn.Tanh(), torch.nn.Linear(40, 13), torch.nn.Tanh(),
                               torch.nn.Linear(13, 5)).to(dtype)


# ------------------------------------------------------------------------------------------------ config
def test_config_from_deepspeed():
    from rankpo_amd import LossScaleConfig
    c = LossScaleConfig.from_deepspeed(DS_CONFIG)
    assert (c.init_scale, c.window, c.hysteresis, c.consecutive_hysteresis, c.min_scale, c.dynamic) == \
        (2.0 ** 16, 1000, 2, False, 1.0, True)
    assert c == LossScaleConfig()                               # the defaults ARE the reference's BGE run
    s = LossScaleConfig.from_deepspeed({"fp16": {"enabled": True, "loss_scale": 128}})
    assert s.dynamic is False and s.init_scale == 128.0
    d = LossScaleConfig.from_deepspeed({"fp16": {"loss_scale": 0, "initial_scale_power": 12, "loss_scale_window": 50,
                                                 "hysteresis": 1, "consecutive_hysteresis": True, "min_loss_scale": 4}})
    assert (d.init_scale, d.window, d.hysteresis, d.consecutive_hysteresis, d.min_scale, d.dynamic) == (4096.0, 50, 1, True, 4.0, True)
    for bad_cfg, msg in (({"bf16": {"enabled": True}}, 'no "fp16" block'), ({"fp16": {"loss_scale": "auto"}}, "fp16.loss_scale"),
                         ({"fp16": {"initial_scale_power": "auto"}}, "fp16.initial_scale_power"), ({"loss_scale": 0}, 'no "fp16" block')):
        with pytest.raises(ValueError, match=msg):
            LossScaleConfig.from_deepspeed(bad_cfg)
    for bad in (dict(init_scale=0.0), dict(window=0), dict(hysteresis=0), dict(min_scale=0.0), dict(init_scale=float("inf"))):
        with pytest.raises(ValueError):
            LossScaleConfig(**bad)


# ------------------------------------------------------------------------------------------------ construction
def test_construction_rules(cpu_kernels):
    from rankpo_amd import LossScaleConfig, TrainStep
    from rankpo_amd.memory import optimizer_state_bytes
    net = _mlp()
    ts = TrainStep(net.parameters(), lambda b: net(b).float().pow(2).mean())
    assert ts.opt.scaler == LossScaleConfig.from_deepspeed(DS_CONFIG) and ts.opt.scaler.dynamic
    assert ts.opt.master is not None and ts.opt.master.dtype == torch.float32 and ts.opt.flat_param.dtype == torch.float16
    assert ts.loss_scale_state() == {"scale": 65536.0, "cur_hysteresis": 2, "good_steps": 0, "applied_steps": 0,
                                     "skipped_steps": 0, "floor_hits": 0}
    for given, want in (("dynamic", LossScaleConfig()), (512, LossScaleConfig(init_scale=512.0, dynamic=False)),
                        (LossScaleConfig(window=7), LossScaleConfig(window=7))):
        n2 = _mlp()
        assert TrainStep(n2.parameters(), lambda b: None, loss_scale=given).opt.scaler == want
    for bad in ("static", True, [1.0]):
        with pytest.raises(ValueError):
            n2 = _mlp()
            TrainStep(n2.parameters(), lambda b: None, loss_scale=bad)
    for dtype in (torch.bfloat16, torch.float32):
        for given in (128.0, "dynamic", LossScaleConfig()):
            n3 = _mlp(dtype)
            with pytest.raises(ValueError, match="loss_scale"):
                TrainStep(n3.parameters(), lambda b: None, loss_scale=given)
        n3 = _mlp(dtype)
        plain = TrainStep(n3.parameters(), lambda b: None)
        assert plain.opt.scaler is None and plain.opt.ls_state is None and plain.opt.loss_scale is None
        with pytest.raises(RuntimeError):
            plain.loss_scale_state()
    # the HBM plan prices an fp16 encoder's optimizer state like bf16: 2 + 2 B/param of parameters and gradients + 12 of state
    es16 = torch.empty((), dtype=torch.float16).element_size()
    assert optimizer_state_bytes(1000, es16, 1, False) == 1000 * 16 == optimizer_state_bytes(1000, 2, 1, False)


# ------------------------------------------------------------------------------------------------ the update rule, driven
O, G = True, False
# window 4, hysteresis 2, consecutive_hysteresis False, scale 16, floor 4
PATTERN = [O,              # first overflow: hysteresis 2 -> 1, scale HELD, step skipped
           O,              # second: halved -> 8
           G, G, G, G,     # growth exactly at good_steps % 4 == 0 -> 16, hysteresis refilled there (and only there)
           O,              # 2 -> 1, held
           G, G, G,        # three good steps refill nothing ...
           O,              # ... so this one halves at once -> 8
           O,              # -> 4 = the floor
           O, O,           # clamped at 4: floor_hits 1, 2
           G, G, G, G, G, G, G, G]      # -> 8 after four, -> 16 after eight
SCALES = [16, 8, 8, 8, 8, 16, 16, 16, 16, 16, 8, 4, 4, 4, 4, 4, 4, 8, 8, 8, 8, 16]
HYST = [1, 1, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2]
FLOOR = [0] * 12 + [1, 2] + [2] * 8


def _drive(ts, net, cfg, pattern, boom):
    """Run the pattern; after every step the product's state must equal the rule's, a skipped step must leave every buffer
    bit-identical, an applied one must move the parameters."""
    rule = Rule(cfg)
    gen = torch.Generator().manual_seed(5)
    seen = []
    for i, overflow in enumerate(pattern):
        boom[0] = float("inf") if overflow else 1.0
        opt = ts.opt
        before = [t.clone() for t in (opt.flat_param, opt.master, opt.exp_avg, opt.exp_avg_sq)]
        loss = ts.step([torch.randn(6, 24, generator=gen).half()])
        rule.update(overflow)
        st = ts.loss_scale_state()
        assert st == rule.state(), (i, st, rule.state())
        after = (opt.flat_param, opt.master, opt.exp_avg, opt.exp_avg_sq)
        if overflow:
            assert all(torch.equal(a, b) for a, b in zip(after, before)), i
            assert not math.isfinite(float(opt.last_grad_norm)) and not math.isfinite(float(loss))
        else:
            assert not torch.equal(opt.flat_param, before[0]) and math.isfinite(float(opt.last_grad_norm)), i
            assert math.isfinite(float(loss)) and float(loss) < 10.0          # the UNSCALED loss comes back
        assert opt.reducer.flat.abs().sum() == 0                               # gradients zeroed, skipped or not
        assert opt.t == i + 1 and ts.global_step == i + 1                      # attempted steps; the schedule advances regardless
        assert float(opt.loss_scale) == st["scale"]
        seen.append(st)
    return seen


def test_update_rule_through_train_step(cpu_kernels):
    from rankpo_amd import LossScaleConfig, TrainStep
    cfg = LossScaleConfig(init_scale=16.0, window=4, hysteresis=2, consecutive_hysteresis=False, min_scale=4.0)
    net, boom = _mlp(), [1.0]
    ts = TrainStep(net.parameters(), lambda b: net(b).float().pow(2).mean() * boom[0], lr=1e-2, max_grad_norm=0.5,
                   total_steps=100, warmup_ratio=0.0, loss_scale=cfg)
    seen = _drive(ts, net, cfg, PATTERN, boom)
    assert [s["scale"] for s in seen] == SCALES
    assert [s["cur_hysteresis"] for s in seen] == HYST
    assert [s["floor_hits"] for s in seen] == FLOOR
    assert seen[-1]["skipped_steps"] == sum(PATTERN) and seen[-1]["applied_steps"] == len(PATTERN) - sum(PATTERN)
    # consecutive_hysteresis True: every good step refills; hysteresis 1: every overflow halves
    for cfg2, pattern, scales in (
            (LossScaleConfig(init_scale=16.0, window=4, hysteresis=2, consecutive_hysteresis=True, min_scale=1.0),
             [O, G, O, O, G], [16, 16, 16, 8, 8]),
            (LossScaleConfig(init_scale=16.0, window=2, hysteresis=1, min_scale=1.0), [O, O, G, G, G], [8, 4, 4, 8, 8])):
        net2 = _mlp()
        ts2 = TrainStep(net2.parameters(), lambda b: net2(b).float().pow(2).mean() * boom[0], lr=1e-2, warmup_ratio=0.0, loss_scale=cfg2)
        assert [s["scale"] for s in _drive(ts2, net2, cfg2, pattern, boom)] == scales


def test_static_scale_skips_but_never_moves(cpu_kernels):
    from rankpo_amd import LossScaleConfig, TrainStep
    net, boom = _mlp(), [1.0]
    ts = TrainStep(net.parameters(), lambda b: net(b).float().pow(2).mean() * boom[0], lr=1e-2, max_grad_norm=None, warmup_ratio=0.0,
                   loss_scale=32.0)
    seen = _drive(ts, net, LossScaleConfig(init_scale=32.0, dynamic=False), [G, O, G, O, O, G], boom)
    assert all(s["scale"] == 32.0 and s["good_steps"] == 0 and s["cur_hysteresis"] == 2 and s["floor_hits"] == 0 for s in seen)
    assert seen[-1]["applied_steps"] == 3 and seen[-1]["skipped_steps"] == 3


def test_scale_reaches_the_backward_and_leaves_the_update(cpu_kernels):
    """The gradients in the flat buffer are scale x the plain ones (seen by `_sumsq`), the reported norm and the update are
    not: two static scales give the same norm and the same parameters, to fp16 rounding of the gradients."""
    from rankpo_amd.train_step import FlatAdamW, TrainStep
    runs = {}
    for scale in (1.0, 64.0):
        net = _mlp()
        seen = []
        inner = FlatAdamW._sumsq
        ts = TrainStep(net.parameters(), lambda b: net(b).float().pow(2).mean(), lr=1e-2, max_grad_norm=0.05, warmup_ratio=0.0,
                       loss_scale=scale)
        ts.opt._sumsq = lambda g: seen.append(float(inner(ts.opt, g))) or inner(ts.opt, g)
        gen = torch.Generator().manual_seed(9)
        for _ in range(3):
            ts.step([torch.randn(6, 24, generator=gen).half()])
        runs[scale] = (seen, float(ts.opt.last_grad_norm), ts.opt.master.clone())
    (ss1, n1, w1), (ss64, n64, w64) = runs[1.0], runs[64.0]
    assert float(ts.opt.grad_norm(1.0)) == 0.0                 # the public norm divides the scale out (gradients are zeroed here)
    assert ss64[0] == pytest.approx(64.0 ** 2 * ss1[0], rel=1e-2) and n64 == pytest.approx(n1, rel=1e-2)
    assert n1 > 0.05                                            # clipping was active
    assert (w1 - w64).abs().max() < 1e-3 and (w1 - ts.opt.flat_param.float()).abs().max() < 1e-3


def test_state_dict_round_trip(cpu_kernels):
    from rankpo_amd import LossScaleConfig, TrainStep
    cfg = LossScaleConfig(init_scale=16.0, window=4, min_scale=4.0)
    net, boom = _mlp(), [1.0]
    ts = TrainStep(net.parameters(), lambda b: net(b).float().pow(2).mean() * boom[0], lr=1e-2, warmup_ratio=0.0, loss_scale=cfg)
    _drive(ts, net, cfg, PATTERN[:9], boom)
    sd = ts.state_dict()
    assert sd["global_step"] == 9 and sd["attempted_steps"] == 9 and sd["loss_scale"] == ts.loss_scale_state()
    net2 = _mlp()
    ts2 = TrainStep(net2.parameters(), lambda b: None, loss_scale=cfg)
    ts2.load_state_dict(sd)
    assert ts2.state_dict() == sd and ts2.opt.t == 9
    net3 = _mlp(torch.bfloat16)
    with pytest.raises(ValueError):
        TrainStep(net3.parameters(), lambda b: None).load_state_dict(sd)


# ------------------------------------------------------------------------------------------------ two gloo ranks
def _overflow_worker(rank, world, port, ret):
    """ONE rank's gradient holds an inf: every rank skips (replicated and partitioned state), counts it, and the replicas stay
    bit-identical -- the all-reduced gradient (or the all-reduced sum of squares) is the same on every rank, so no extra
    collective carries the verdict."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from rankpo_amd.train_step import FlatAdamW, LossScaleConfig, TrainStep
        cpu_fp16_kernels(FlatAdamW)
        why = []
        cfg = LossScaleConfig(init_scale=16.0, window=4, hysteresis=1)
        for part in (False, True):
            net, boom = _mlp(), [1.0]
            ts = TrainStep(net.parameters(), lambda b: net(b).float().pow(2).mean() * boom[0], lr=1e-2, max_grad_norm=0.5,
                           gradient_accumulation_steps=2, total_steps=10, warmup_ratio=0.0, bucket_mb=1e-3,
                           partition_optimizer=part, loss_scale=cfg)
            opt = ts.opt
            assert opt.partition == part and len(opt.reducer.buckets) >= 2
            gen = torch.Generator().manual_seed(100 + rank)
            rule = Rule(cfg)
            for step, overflow in enumerate([G, G, O, G]):
                boom[0] = float("inf") if overflow and rank == 1 else 1.0       # rank 0's own gradient is finite
                before = opt.flat_param.clone()
                ts.step([torch.randn(6, 24, generator=gen).half() for _ in range(2)])
                rule.update(overflow)
                if ts.loss_scale_state() != rule.state():
                    why.append(("state", part, step, ts.loss_scale_state(), rule.state()))
                if overflow != torch.equal(opt.flat_param, before):
                    why.append(("skip", part, step))
                lo, hi = opt.flat_param.float().clone(), opt.flat_param.float().clone()
                dist.all_reduce(lo, op=dist.ReduceOp.MIN)
                dist.all_reduce(hi, op=dist.ReduceOp.MAX)
                if not (torch.equal(lo, hi) and bool(torch.isfinite(hi).all())):
                    why.append(("replicas", part, step))
        ret[rank] = not why
        if why:
            ret[f"why{rank}"] = why
    finally:
        dist.destroy_process_group()


def test_gloo_one_rank_overflows_every_rank_skips():
    import socket
    world = 2
    ret = mp.Manager().dict()
    with socket.socket() as sock:                              # a port the system hands out: nothing fixed to collide on
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    mp.spawn(_overflow_worker, args=(world, port, ret), nprocs=world, join=True)
    assert all(ret.get(r) for r in range(world)), dict(ret)
