"""fp16 training on the device: the fp16 gradient sum of squares (the overflow check), the one-thread loss-scale update
(rpo_loss_scale_update), the AdamW step that obeys its state block (rpo_adamw_step_scaled), `FlatAdamW` / `TrainStep` with
float16 parameters (rankpo_amd/csrc/optim.hip, rankpo_amd/train_step.py).

References: float64 from the exact stored inputs and the f32 scalars the C ABI receives; the scaler's rule as the plain-Python
`Rule` of tests/test_loss_scale_host.py.  Bounds are the ones of the bf16 / f32 optimizer tests (the per-block sum-of-squares
bound and the AdamW m / v / w bounds of tests/test_gpu_encoder_ops_parity.py, the FlatAdamW-vs-torch tolerance of
tests/test_gpu_encoder.py): the arithmetic and the f32 state are the same."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_encoder_ops_parity as P                  # check_elem, the AdamW / sumsq constants and their bounds
from test_loss_scale_host import Rule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
U = P.U
f32 = P.f32


def _lib():
    from rankpo_amd import _lib as L
    return L.load()


def _L():
    from rankpo_amd import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _state_block(rule, skip=0, mult=0.0, norm=0.0):
    """A device state block (rpo_ls_word layout) holding `rule`'s state."""
    L = _L()
    w = torch.zeros(L.RPO_LS_WORDS, dtype=torch.int32)
    f = w.view(torch.float32)
    f[L.RPO_LS_SCALE], f[L.RPO_LS_MULT], f[L.RPO_LS_NORM] = rule.scale, mult, norm
    w[L.RPO_LS_SKIP] = skip
    for k, i in (("good_steps", L.RPO_LS_GOOD_STEPS), ("cur_hysteresis", L.RPO_LS_CUR_HYSTERESIS),
                 ("applied_steps", L.RPO_LS_APPLIED_STEPS), ("skipped_steps", L.RPO_LS_SKIPPED_STEPS),
                 ("floor_hits", L.RPO_LS_FLOOR_HITS)):
        w[i] = getattr(rule, k)
    return w.to(DEV)


def _read_block(blk):
    L = _L()
    w = blk.cpu()
    f = w.view(torch.float32)
    return {"scale": float(f[L.RPO_LS_SCALE]), "mult": float(f[L.RPO_LS_MULT]), "norm": float(f[L.RPO_LS_NORM]),
            "skip": int(w[L.RPO_LS_SKIP]), "good_steps": int(w[L.RPO_LS_GOOD_STEPS]),
            "cur_hysteresis": int(w[L.RPO_LS_CUR_HYSTERESIS]), "applied_steps": int(w[L.RPO_LS_APPLIED_STEPS]),
            "skipped_steps": int(w[L.RPO_LS_SKIPPED_STEPS]), "floor_hits": int(w[L.RPO_LS_FLOOR_HITS]),
            "reserved": w[9:].tolist()}


# ============================================================================================================ sum of squares
SUMSQ_CASES = [4 * 9573,                                  # n % 8 == 4: a 4-element tail; 19 active blocks
               4004,                                      # 500 vectors: 2 active blocks, 1022 idle
               8 * 1024 * 1024 * 5 + 3,                   # 5120 vectors per block: the 4-deep loop, a 3-element tail
               P.ADAM_BIG]                                # 3 x 10^8 (n % 8 == 4)


def _sumsq(x):
    part = torch.full((P.SUMSQ_NBLK,), NAN, dtype=torch.float32, device=DEV)
    assert _lib().rpo_sumsq_partial(x.data_ptr(), x.numel(), _L().RPO_DT_F16, part.data_ptr(), P.SUMSQ_NBLK, _stream()) == 0
    torch.cuda.synchronize()
    return part


@pytest.mark.parametrize("n", SUMSQ_CASES)
def test_sumsq_f16_parity_and_overflow_detection(n):
    """Every block's partial against float64 over the contiguous chunk it owns, by the per-block bound of the bf16 / f32 test;
    idle blocks exactly 0; one inf / one NaN at the first, a middle and the last element makes the total non-finite; a buffer of
    the largest finite fp16 value everywhere stays finite (squares summed in f32 cannot overflow)."""
    V = 8
    nv = n // V
    assert n % V, "a tail for block 0"
    x = torch.randn(n, device=DEV, generator=P._gen(n % 997)).half()
    x[nv * V:] = P.SUMSQ_TAIL
    part = _sumsq(x)
    per = P._cdiv(P._cdiv(nv, P.SUMSQ_NBLK), 256) * 256
    active = P._cdiv(nv, per)
    ref = torch.zeros(P.SUMSQ_NBLK, dtype=torch.float64, device=DEV)
    body = x[:nv * V]
    step = max(1, (1 << 25) // (per * V))
    for b0 in range(0, active, step):
        b1 = min(active, b0 + step)
        full = min(b1, nv // per)
        if full > b0:
            ref[b0:full] = body[b0 * per * V:full * per * V].to(torch.float64).square().view(full - b0, per * V).sum(1)
        if b1 > full:
            ref[full] = body[full * per * V:].to(torch.float64).square().sum()
    tail = x[nv * V:].to(torch.float64).square().sum()
    ref[0] += tail
    c = per * V / 1024 + 3 * V + 12                       # the bound of test_sumsq_partial_parity: same loop, same V as bf16
    assert tail > 100 * c * U * ref[0], "the tail must be visible above block 0's bound"
    P.check_elem("fp16 sumsq partials", part, ref, c * U * ref)
    if active < P.SUMSQ_NBLK:
        assert (part[active:] == 0).all()
    assert math.isfinite(float(part.sum()))
    for pos in (0, n // 2, n - 1):
        for bad in (float("inf"), NAN):
            keep = x[pos].clone()
            x[pos] = bad
            total = float(_sumsq(x).sum())
            x[pos] = keep
            assert not math.isfinite(total), (pos, bad, total)
    x.fill_(65504.0)
    total = float(_sumsq(x).sum())
    print(f"\nn {n}: total of 65504^2 everywhere = {total:.6e}")
    assert math.isfinite(total) and total == pytest.approx(n * 65504.0 ** 2, rel=1e-5)


def test_sumsq_and_adamw_entries_keep_their_verdicts():
    """rpo_adamw_step still refuses fp16 (the scaled entry serves it); the scaled entry refuses what it does not take."""
    L, lib = _L(), _lib()
    n = 1024
    h = torch.zeros(n, dtype=torch.float16, device=DEV)
    f = [torch.zeros(n, dtype=torch.float32, device=DEV) for _ in range(3)]
    blk = _state_block(Rule(_cfg()))
    a = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert lib.rpo_adamw_step(h.data_ptr(), f[0].data_ptr(), h.data_ptr(), f[1].data_ptr(), f[2].data_ptr(), n, L.RPO_DT_F16,
                              *a, 1.0, 1.0, None, _stream()) == -1
    def scaled(dt=L.RPO_DT_F16, master=f[0].data_ptr(), state=blk.data_ptr(), nn=n):
        return lib.rpo_adamw_step_scaled(h.data_ptr(), master, h.data_ptr(), f[1].data_ptr(), f[2].data_ptr(), nn, dt, *a, state,
                                         _stream())
    assert scaled(master=None) == -1 and scaled(state=None) == -1 and scaled(dt=7) == -1 and scaled(nn=0) == -1
    assert scaled(dt=L.RPO_DT_BF16) == P.RPO_ERR_UNSUPPORTED and scaled(dt=L.RPO_DT_F32) == P.RPO_ERR_UNSUPPORTED
    assert scaled(nn=n - 2) == P.RPO_ERR_UNSUPPORTED and scaled(state=blk.data_ptr() + 4) == P.RPO_ERR_UNSUPPORTED
    ss = torch.ones(1, device=DEV)
    def upd(pre=1.0, window=4, hyst=2, mins=1.0, state=blk.data_ptr()):
        return lib.rpo_loss_scale_update(ss.data_ptr(), state, pre, 1.0, 1, window, hyst, 0, mins, _stream())
    assert upd(pre=0.0) == -1 and upd(window=0) == -1 and upd(hyst=0) == -1 and upd(mins=0.0) == -1 and upd(state=None) == -1
    assert upd() == 0 and scaled() == 0
    torch.cuda.synchronize()


# ============================================================================================================ the update kernel
def _cfg(**kw):
    from rankpo_amd import LossScaleConfig
    return LossScaleConfig(**kw)


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


UPDATE_CASES = [  # (config, max_grad_norm, pre_scale, overflow probability)
    (dict(init_scale=2.0 ** 16, window=4, hysteresis=2, consecutive_hysteresis=False, min_scale=1.0), 1.0, 1.0 / 8, 0.3),
    (dict(init_scale=2.0 ** 10, window=3, hysteresis=3, consecutive_hysteresis=True, min_scale=2.0 ** -3), 0.5, 1.0 / 3, 0.45),
    (dict(init_scale=2.0 ** 8, window=2, hysteresis=1, min_scale=4.0), 0.0, 1.0, 0.5),
    (dict(init_scale=2.0 ** 20, window=1000, hysteresis=2, min_scale=1.0), 1.0, 1.0 / 48, 0.1),
    (dict(init_scale=512.0, dynamic=False), 1.0, 0.25, 0.3),
]


@pytest.mark.parametrize("case", range(len(UPDATE_CASES)))
def test_loss_scale_update_kernel_matches_the_rule(case):
    """150 scripted steps per configuration: every state word equal to the Python rule's (the scale is a power of two
    throughout, so f32 holds it exactly); skip as scripted; mult and norm against float64 within 2 f32 ulps.

    The 2 ulps: the kernel evaluates norm = sqrt(ss) * (pre / s) and mult = (pre / s) * min(1, mgn / (norm + 1e-6)) in f64 --
    at most 7 operations of relative error 2^-53 each, about 2^-26 of an f32 ulp -- and rounds each to f32 ONCE: 1/2 ulp.  A
    kernel doing the same in f32 would round norm twice (1 ulp) and mult five times (sqrt, the product, the sum, the quotient,
    the product: 2.5 ulp of the larger binade), so 2 ulps is also what separates the two; measured: <= 0.5 (printed)."""
    kw, mgn, pre, p_over = UPDATE_CASES[case]
    cfg = _cfg(**kw)
    lib, rs = _lib(), np.random.RandomState(40 + case)
    rule = Rule(cfg)
    blk = _state_block(rule, skip=1, mult=NAN, norm=NAN)
    ss = torch.zeros(1, device=DEV)
    pre32, mgn32 = f32(pre), f32(mgn)
    worst, scales, floor_seen = 0.0, set(), 0
    for step in range(150):
        overflow = bool(rs.rand() < p_over)
        ssv = [float("inf"), NAN][step % 2] if overflow else f32(10.0 ** rs.uniform(-6, 12))
        ss.fill_(ssv)
        s = rule.scale
        assert lib.rpo_loss_scale_update(ss.data_ptr(), blk.data_ptr(), pre, mgn, int(cfg.dynamic), cfg.window, cfg.hysteresis,
                                         int(cfg.consecutive_hysteresis), cfg.min_scale, _stream()) == 0
        rule.update(overflow)
        got = _read_block(blk)
        want = rule.state()
        assert {k: got[k] for k in want} == want, (step, got, want)
        assert got["skip"] == int(overflow) and got["reserved"] == [0] * 7, (step, got)
        if overflow:
            assert not math.isfinite(got["norm"]) and got["mult"] == 0.0, (step, got)
        else:
            norm = math.sqrt(ssv) * pre32 / s
            mult = pre32 / s * (min(1.0, mgn32 / (norm + 1e-6)) if mgn32 > 0 else 1.0)
            for name, g, r in (("norm", got["norm"], norm), ("mult", got["mult"], mult)):
                e = abs(g - r) / _ulp32(r)
                worst = max(worst, e)
                assert e <= 2.0, (step, name, g, r, e)
            if mgn32 <= 0:
                assert got["mult"] == f32(pre32 / s)
        scales.add(got["scale"])
        floor_seen = got["floor_hits"]
    print(f"\ncase {case}: worst |mult, norm error| {worst:.3f} ulp; {len(scales)} distinct scales; skipped "
          f"{rule.skipped_steps}, floor hits {floor_seen}")
    assert rule.skipped_steps > 5 and rule.applied_steps > 50
    assert (len(scales) == 1) == (not cfg.dynamic)
    if case == 2:
        assert floor_seen > 0, "the floor case must reach the floor"


# ============================================================================================================ fp16 AdamW
ADAM_MID = 4 * (256 * 4099 + 17)                          # 4.2 M: 4100 blocks, a partial last one; n % 8 == 4
ADAMW_CASES = [(P.ADAM_N, 1, 0.37), (P.ADAM_N, 5000, 2.5 / 1024), (ADAM_MID, 5000, 0.37), (ADAM_MID, 37, 1.0 / 65536)]


def _adam_inputs(n, seed):
    """The inputs of test_adamw_step_parity with fp16 parameters and gradients; every buffer is NaN-prefilled, then its first n
    elements are initialised (the elements behind n keep the NaN: nothing may touch them)."""
    gen = P._gen(seed)
    N = n + P.ADAM_PAD

    def buf(x, dt=torch.float32):
        b = torch.full((N,), NAN, dtype=dt, device=DEV)
        b[:n] = x
        return b
    w0 = buf(0.05 * torch.randn(n, device=DEV, generator=gen))
    gval = torch.randn(n, device=DEV, generator=gen) * 10.0 ** (-4 * torch.rand(n, device=DEV, generator=gen))
    m0 = buf(1e-3 * torch.randn(n, device=DEV, generator=gen))
    v0 = buf((1e-3 * torch.randn(n, device=DEV, generator=gen)).square())
    i = torch.arange(n, device=DEV)
    zero = i % 8 == 3                                      # zero moments ...
    m0[:n][zero] = 0
    v0[:n][zero] = 0
    gval[i % 16 == 3] = 0                                  # ... with a zero gradient
    gval[i % 16 == 11] *= 1e-9                             # ... with a gradient whose sqrt(v) is below eps (0 or subnormal in fp16)
    grad = buf(gval.half(), torch.float16)
    param = buf(w0[:n].half(), torch.float16)
    return w0, m0, v0, grad, param


def _scaled_step(param, master, grad, m, v, n, blk):
    a = P.ADAM
    rc = _lib().rpo_adamw_step_scaled(param.data_ptr(), master.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n,
                                      _L().RPO_DT_F16, a["lr"], a["beta1"], a["beta2"], a["eps"], a["wd"], blk.data_ptr(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,t,mult", ADAMW_CASES, ids=[f"n{n}-t{t}-mult{m:.3g}" for n, t, m in ADAMW_CASES])
def test_adamw_f16_scaled_parity(n, t, mult):
    """One rpo_adamw_step_scaled against float64 AdamW on the same f32 state, with the multiplier and the applied-step count
    read from the device block (bias corrections 1 - beta^t from the f32 betas the ABI receives, rounded to f32 once, as the
    kernel's f64 powers give them); m / v / master by the bounds of test_adamw_step_parity; the fp16 parameter bit-equal to
    master.half(); the elements behind n untouched."""
    assert n % 4 == 0 and (n // 4) % 256 != 0 and n % 8 == 4
    w0, m0, v0, grad, param = _adam_inputs(n, n % 1000 + t)
    master, m, v = w0.clone(), m0.clone(), v0.clone()
    p_before, g_before = param.clone(), grad.clone()
    rule = Rule(_cfg())
    rule.applied_steps = t
    blk = _state_block(rule, skip=0, mult=mult)
    blk_before = blk.clone()
    _scaled_step(param, master, grad, m, v, n, blk)
    assert torch.equal(blk, blk_before), "the AdamW step wrote the state block"
    for name, b, b0 in (("m", m, m0), ("v", v, v0), ("master", master, w0), ("param", param, p_before)):
        assert torch.equal(_bits(b[n:]), _bits(b0[n:])), f"{name}: elements behind n written"
    assert torch.equal(_bits(grad), _bits(g_before))
    assert torch.equal(_bits(param[:n]), _bits(master[:n].half())), "fp16 parameter != RNE(f32 master)"
    a = P.ADAM
    lr, b1, b2, eps, wd = (f32(a[k]) for k in ("lr", "beta1", "beta2", "eps", "wd"))
    bc1, bc2, gsv = f32(1.0 - b1 ** t), f32(1.0 - b2 ** t), f32(mult)
    step, decay = lr / bc1, 1.0 - lr * wd
    eps_dom = 0
    ch = 1 << 22
    for c0 in range(0, n, ch):
        sl = slice(c0, min(n, c0 + ch))
        f = torch.float64
        gk = grad[sl].to(f) * gsv
        mo, vo, wo = m0[sl].to(f), v0[sl].to(f), w0[sl].to(f)
        m_ref = b1 * mo + (1 - b1) * gk
        v_ref = b2 * vo + (1 - b2) * gk * gk
        sq = v_ref.sqrt() / math.sqrt(bc2)
        denom = sq + eps
        upd = step * m_ref / denom
        w_ref = wo * decay - upd
        eps_dom += int((sq < eps).sum())
        b_m = 3 * U * (b1 * mo.abs() + (1 - b1) * gk.abs())          # the three bounds of test_adamw_step_parity, unchanged
        b_v = 5 * U * v_ref
        b_w = 2 * U * (wo * decay).abs() + step * b_m / denom + 12 * U * upd.abs() + U * w_ref.abs()
        P.check_elem(f"m [{c0}..]", m[sl], m_ref, b_m)
        P.check_elem(f"v [{c0}..]", v[sl], v_ref, b_v)
        P.check_elem(f"w [{c0}..]", master[sl], w_ref, b_w)
    assert eps_dom > 0 and wd > 0 and gsv != 1.0
    assert not torch.equal(param[:n], p_before[:n])


def test_adamw_f16_skip_writes_nothing():
    """skip = 1: param, master, m and v are bit-identical to their NaN-prefilled-and-then-initialised inputs, whatever the
    block's multiplier and step count hold."""
    n = ADAM_MID
    w0, m0, v0, grad, param = _adam_inputs(n, 77)
    master, m, v, p0 = w0.clone(), m0.clone(), v0.clone(), param.clone()
    rule = Rule(_cfg())
    blk = _state_block(rule, skip=1, mult=NAN)               # applied_steps 0, mult NaN: neither may be consumed
    _scaled_step(param, master, grad, m, v, n, blk)
    for name, b, b0 in (("param", param, p0), ("master", master, w0), ("m", m, m0), ("v", v, v0)):
        assert torch.equal(_bits(b), _bits(b0)), name
    rule.applied_steps = 1
    blk2 = _state_block(rule, skip=0, mult=1.0)
    _scaled_step(param, master, grad, m, v, n, blk2)         # the same call with skip = 0 does write
    assert not torch.equal(_bits(master[:n]), _bits(w0[:n])) and bool(torch.isfinite(master[:n]).all())


# ============================================================================================================ FlatAdamW
def test_flat_adamw_f16_matches_torch_adamw():
    """3 steps, clipping active, static scale 128: torch.optim.AdamW on an f32 master copy fed grad.float() * mult (the
    device's multiplier: 1 / scale and the clip factor) must land where FlatAdamW's f32 master does, by the tolerance of
    test_flat_adamw_matches_torch_adamw; the fp16 parameters are the rounded master."""
    from rankpo_amd.train_step import FlatAdamW
    L = _L()
    torch.manual_seed(8)
    net = torch.nn.Sequential(torch.nn.Linear(37, 29), torch.nn.Linear(29, 11)).to(DEV).half()
    ref = torch.nn.Sequential(torch.nn.Linear(37, 29), torch.nn.Linear(29, 11)).to(DEV)
    ref.load_state_dict({k: v.float() for k, v in net.state_dict().items()})
    opt = FlatAdamW(net.parameters(), lr=1e-2, weight_decay=0.01, max_grad_norm=0.5, loss_scale=128.0)
    ropt = torch.optim.AdamW(ref.parameters(), lr=1e-2, weight_decay=0.01, eps=1e-8)
    index = {id(p): opt.reducer.offsets[i] for i, p in enumerate(opt.reducer.order)}
    for step in range(3):
        x = torch.randn(16, 37, device=DEV)
        (net(x.half()).float().pow(2).sum() * opt.loss_scale).backward()
        grads = [p.grad.float().clone() for p in net.parameters()]
        norm64 = math.sqrt(sum(float(g.double().square().sum()) for g in grads)) / 128.0
        pub = float(opt.grad_norm(1.0))                      # the public norm: unscaled too
        opt.step()
        st = _read_block(opt.ls_state)
        assert st["skip"] == 0 and st["applied_steps"] == step + 1 and st["scale"] == 128.0
        assert 0 < st["mult"] < 1.0 / 128.0 and st["norm"] > 0.5, st          # clipping was active
        assert float(opt.last_grad_norm) == st["norm"]
        # norm and multiplier against float64 from the saved gradients, so that the reference below does not lean on the device's
        # clip factor: the sum of squares is an f32 sum of ~1400 terms (relative (n / 1024 + 36) u <= 2^-18 by the sumsq test's
        # bound, halved by the root), the rest is rounded once
        assert abs(st["norm"] - norm64) <= 2.0 ** -18 * norm64 and abs(pub - norm64) <= 2.0 ** -18 * norm64, (st["norm"], pub, norm64)
        mult64 = (1.0 / 128.0) * min(1.0, 0.5 / (norm64 + 1e-6))
        assert abs(st["mult"] - mult64) <= 2.0 ** -18 * mult64, (st["mult"], mult64)
        for q, g in zip(ref.parameters(), grads):
            q.grad = g * st["mult"]
        ropt.step()
        ropt.zero_grad()
        for p, q in zip(net.parameters(), ref.parameters()):
            o = index[id(p)]
            m = opt.master[o:o + p.numel()].view_as(p)
            assert (m - q).abs().max() < 2e-5 * max(1.0, q.abs().max().item()), step
            assert p.grad.abs().sum() == 0
            assert torch.equal(p.data, m.half())
            q.data.copy_(m)                                  # keep both in lockstep
    assert opt.t == 3


# ============================================================================================================ end to end, exact
def _mlp(seed=3):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(64, 96), torch.nn.Tanh(), torch.nn.Linear(96, 48), torch.nn.Tanh(),
                               torch.nn.Linear(48, 8)).to(DEV).half()


def test_train_step_dynamic_settles_and_then_equals_static_bit_for_bit():
    """An fp16 MLP whose initial scale, 2^30, saturates the fp16 gradients to inf: the scaler comes down exactly as the rule
    says (first overflow held by the hysteresis, then one halving per step), the parameters do not move meanwhile, and from the
    settled scale on the run is bit-identical to a static run at that scale from the same weights and batches -- same
    applied_steps, hence the same bias correction (the static arm is given the dynamic arm's schedule position: the LR schedule
    advances on skipped steps too)."""
    from rankpo_amd import LossScaleConfig, TrainStep
    P0 = 30
    cfg = LossScaleConfig(init_scale=2.0 ** P0, window=1000, hysteresis=2, min_scale=1.0)
    gen = torch.Generator(device=DEV).manual_seed(11)
    n_after = 5
    batches = [torch.randn(32, 64, device=DEV, generator=gen).half() for _ in range(40)]

    def make(loss_scale):
        net = _mlp()
        ts = TrainStep(net.parameters(), lambda b: net(b).float().pow(2).mean(), lr=1e-3, weight_decay=0.01, max_grad_norm=1.0,
                       total_steps=100, warmup_ratio=0.1, loss_scale=loss_scale)
        return net, ts
    net, ts = make(cfg)
    w_init = ts.opt.flat_param.clone()
    rule = Rule(cfg)
    history, k = [], None
    for i in range(len(batches) - n_after):
        before = [t.clone() for t in (ts.opt.flat_param, ts.opt.master, ts.opt.exp_avg, ts.opt.exp_avg_sq)]
        ts.step([batches[i]])
        overflow = not math.isfinite(float(ts.opt.last_grad_norm))
        rule.update(overflow)
        st = ts.loss_scale_state()
        assert st == rule.state(), (i, st, rule.state())
        history.append(st["scale"])
        if not overflow:
            k = i
            break
        for a, b in zip((ts.opt.flat_param, ts.opt.master, ts.opt.exp_avg, ts.opt.exp_avg_sq), before):
            assert torch.equal(a, b), i
    assert k is not None and k >= 3, history                  # 2^30 did overflow, several times
    settled = history[-1]
    # the rule's prediction for k consecutive overflows from 2^30 with hysteresis 2: held once, then halved k - 1 times
    assert history == [2.0 ** P0] + [2.0 ** (P0 - j) for j in range(1, k)] + [2.0 ** (P0 - (k - 1))], history
    st = ts.loss_scale_state()
    assert st["skipped_steps"] == k and st["applied_steps"] == 1 and st["floor_hits"] == 0 and st["cur_hysteresis"] == 1
    assert ts.opt.t == k + 1 and ts.global_step == k + 1
    print(f"\nsettled at 2^{int(math.log2(settled))} after {k} skipped steps")
    for i in range(k + 1, k + n_after):
        ts.step([batches[i]])
    # the overflow was the gradients' own: twice the settled scale still overflows on that batch, statically
    net2, ts2 = make(2 * settled)
    ts2.step([batches[k]])
    assert ts2.loss_scale_state()["skipped_steps"] == 1 and torch.equal(ts2.opt.flat_param, w_init)
    # static arm at the settled scale, from the same weights, the same batches, the same schedule position
    net3, ts3 = make(settled)
    assert torch.equal(ts3.opt.flat_param, w_init)
    ts3.global_step = k
    for i in range(k, k + n_after):
        ts3.step([batches[i]])
    a, b = ts.loss_scale_state(), ts3.loss_scale_state()
    assert a["applied_steps"] == b["applied_steps"] == n_after and b["skipped_steps"] == 0 and a["scale"] == b["scale"] == settled
    for name in ("flat_param", "master", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(ts.opt, name), getattr(ts3.opt, name)), name
    assert not torch.equal(ts.opt.flat_param, w_init) and bool(torch.isfinite(ts.opt.master).all())


# ============================================================================================================ end to end, BGE
class TrainSpy:
    """Counts the native packed backward (ops.bidir_attn_bwd) and the padded path's attention (F.scaled_dot_product_attention):
    the spy of tests/test_gpu_bert_train.py."""

    def __init__(self):
        self.n = {"bidir_attn_bwd": 0, "sdpa": 0}

    def __enter__(self):
        from rankpo_amd import ops as o
        self._bwd, self._sdpa = o.bidir_attn_bwd, F.scaled_dot_product_attention

        def bwd(*a, **kw):
            self.n["bidir_attn_bwd"] += 1
            return self._bwd(*a, **kw)

        def sdpa(*a, **kw):
            self.n["sdpa"] += 1
            return self._sdpa(*a, **kw)
        o.bidir_attn_bwd, F.scaled_dot_product_attention = bwd, sdpa
        return self

    def __exit__(self, *exc):
        from rankpo_amd import ops as o
        o.bidir_attn_bwd, F.scaled_dot_product_attention = self._bwd, self._sdpa
        return False


def test_bge_fp16_train_step_with_the_reference_scaler():
    """A BGE-small-shaped fp16 ModelForTraining, dropout 0, 6 TrainStep steps with the reference's default scaler on the native
    packed path.  The dynamic arm against a static arm at its final scale (same number of applied steps, same schedule
    position): embedding gradients are accumulated in an order that is not fixed, so the yardstick is two runs of the static
    arm against each other; per tensor the dynamic arm may be at most 2 x that far from a static run (bit-equal where the
    static arm reproduces itself)."""
    import test_gpu_bert_train as T
    from rankpo_amd import TrainStep
    steps = 6
    _, cfg, _, _ = T._make("bge-small", torch.float16, 0.0, 23)
    batch = T._batch(np.random.RandomState(7), cfg)
    gb = {k: {kk: vv.to(DEV) for kk, vv in v.items()} for k, v in batch.items()}

    def arm(loss_scale, n_steps, start):
        _, _, _, model = T._make("bge-small", torch.float16, 0.0, 23)
        ts = TrainStep(model.parameters(), lambda b: model(**b)["loss"], lr=2e-4, total_steps=100, warmup_ratio=0.0,
                       loss_scale=loss_scale)
        ts.global_step = start
        losses, scales = [], []
        with TrainSpy() as spy:
            for _ in range(n_steps):
                losses.append(ts.step([gb]))
                scales.append(ts.opt.loss_scale.clone())
        with torch.no_grad():                                 # outside the spy: a no-grad forward in training mode is the padded path's
            final = model(**gb)["loss"].float()
        return model, ts, [float(x) for x in losses], [float(s) for s in scales], float(final), spy.n

    model, ts, losses, scales, final, n = arm(None, steps, 0)
    st = ts.loss_scale_state()
    print(f"\ndynamic arm: losses {losses} -> {final}; scales {scales}; state {st}")
    assert n["bidir_attn_bwd"] == steps * 2 * cfg.num_hidden_layers and n["sdpa"] == 0, n      # the native packed step ran
    assert st["skipped_steps"] + st["applied_steps"] == steps and st["applied_steps"] >= 1
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    skipped = st["skipped_steps"]
    assert final < losses[skipped], (final, losses)           # after the last applied step < before the first applied one
    # the overflows of a descent from 2^16 come first; the applied steps then all ran at the final scale
    assert scales[skipped:] == [st["scale"]] * (steps - skipped) and st["good_steps"] == st["applied_steps"], (scales, st)
    statics = [arm(st["scale"], st["applied_steps"], skipped) for _ in range(2)]
    for _, ts_s, _, _, _, n_s in statics:
        s2 = ts_s.loss_scale_state()
        assert s2["applied_steps"] == st["applied_steps"] and s2["skipped_steps"] == 0 and n_s["sdpa"] == 0
    names = [k for k, _ in model.named_parameters()]
    pa, pb, pd = ({k: v.detach() for k, v in m.named_parameters()} for m in (statics[0][0], statics[1][0], model))
    worst = None
    for k in names:
        d_static = float((pa[k].double() - pb[k].double()).norm())
        d_dyn = float((pd[k].double() - pa[k].double()).norm())
        if worst is None or d_dyn - 2 * d_static > worst[1] - 2 * worst[2]:
            worst = (k, d_dyn, d_static)
    tot_s = math.sqrt(sum(float((pa[k].double() - pb[k].double()).norm()) ** 2 for k in names))
    tot_d = math.sqrt(sum(float((pd[k].double() - pa[k].double()).norm()) ** 2 for k in names))
    print(f"distance dynamic-static {tot_d:.3e}, static-static {tot_s:.3e} (all parameters); worst tensor {worst[0]}: "
          f"dynamic-static {worst[1]:.3e}, static-static {worst[2]:.3e}")
    for k in names:
        d_static = float((pa[k].double() - pb[k].double()).norm())
        d_dyn = float((pd[k].double() - pa[k].double()).norm())
        assert d_dyn <= 2 * d_static, (k, d_dyn, d_static)
