"""float64 parity of the loss head (csrc/infonce.hip, csrc/rankpo.hip and the grouped-dot kernel they share) on hard logits: every
forward path of the dispatch (tests/loss_parity_util.py mirrors it; tests/test_loss_parity_host.py proves the case table reaches
every path) x {f32, bf16, f16} x regimes in which a missing max subtraction, a wrong maximum in softmax_merge or a padding column
in a row sum is a catastrophe rather than a perturbation.

What is asserted per case (util docstring for every number introduced here):
  (a) scores against the float64 oracle on the stored inputs with the reference's rounding points;
  (b) lse (read from the autograd node) and loss against the float64 max-subtracted logsumexp / CE of the RETURNED scores,
      inside the derived float32 bounds; everything finite;
  (c) gradients of 0.37 * loss against dS p and dS^T q in float64 from the returned scores, at the existing shape tests'
      tolerances: f32 2e-4, bf16 2^-7, f16 2^-9 of the largest entry.
"""
import numpy as np
import pytest
import torch

import loss_parity_util as U
from oracle import scoring_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
GRAD_TOL = {"f32": 2e-4, "bf16": 2.0 ** -7, "f16": 2.0 ** -9}          # test_infonce_forward_backward_shapes, test_gpu_f16.py
GEMM_GRAD_TOL = {"f32": 3e-4, "bf16": 2.0 ** -6, "f16": 2.0 ** -7}     # test_infonce_backward_gemm_form; test_gpu_f16.py (`big`)


@pytest.fixture(autouse=True)
def _stop_on_device_error():
    """A device error ends the session: nothing more is started on a GPU that has just faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:                                     # noqa: BLE001 -- whatever the runtime raises
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def ops():
    from rankpo_amd import ops as o
    return o


def dev(x, tag, grad=False, aligned=True):
    """x on the device in the storage dtype; aligned=False: one element into a larger allocation (data_ptr() % 16 != 0)."""
    v = torch.tensor(np.asarray(x), dtype=torch.float32).to(TORCH[tag])
    if aligned:
        out = v.to(DEV)
    else:
        big = torch.zeros(v.numel() + 8, dtype=TORCH[tag], device=DEV)
        out = big[1:1 + v.numel()].view(v.shape)
        out.copy_(v)
        assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out.requires_grad_(grad)


def npf(x):
    return x.detach().float().cpu().numpy().astype(np.float64)


def relmax(a, b, floor=0.0):
    return np.abs(a - b).max() / max(np.abs(b).max(), floor, 1e-30)


def _check_forward(loss, lse_t, s, exp, tgt, tag, name):
    """(a) and (b); returns the float64 CE of the returned scores."""
    assert np.isfinite(s).all() and np.isfinite(loss) and np.isfinite(lse_t).all(), name
    r = U.score_errors(s, exp, tag)
    print(f"\n{name}: scores {r:.3f} of the tolerance", end="")
    assert r <= 1.0, (name, "scores", r)
    ce = U.ce_from_scores(s, tgt)
    r_lse = float((np.abs(lse_t - ce["lse"]) / U.lse_bound(ce)).max())
    r_loss = abs(loss - ce["loss"]) / U.loss_bound(ce)
    print(f", lse {r_lse:.3f}, loss {r_loss:.3f} of the bound (loss {loss:.4f})", end="")
    assert r_lse <= 1.0, (name, "lse", r_lse)
    assert r_loss <= 1.0, (name, "loss", r_loss, loss, ce["loss"])
    return ce


def _check_grads(dq, dp, ds, dq_ref, dp_ref, qv, pv, tag, regime, name, tol, gemm_K=None):
    assert np.isfinite(dq).all() and np.isfinite(dp).all(), name
    # `flat`: every p row is the same vector u, so dq_i = u sum_j dS_ij = 0 in closed form and the reference holds only float64
    # noise.  The kernel's own rounding is relative to the terms of that sum: the error is measured against
    # max_i sum_j |dS_ij| * max |p| there (the same tolerance number), and against the largest reference entry everywhere else.
    floor_q = np.abs(ds).sum(-1).max() * np.abs(pv).max() if regime == "flat" else 0.0
    extra_q = extra_p = 0.0
    if gemm_K is not None and tag == "f16":
        # dS + two GEMMs form in fp16: dS itself is stored in fp16, whose subnormals are 2^-24 apart (test_gpu_f16.py notes it), so
        # each of the K terms of a product carries up to 2^-25 of absolute error, coherent when all entries are equal (`flat`).
        extra_q = gemm_K[0] * 2.0 ** -25 * np.abs(pv).max()
        extra_p = gemm_K[1] * 2.0 ** -25 * np.abs(qv).max()
    eq = (np.abs(dq - dq_ref).max() - extra_q) / max(np.abs(dq_ref).max(), floor_q, 1e-30)
    ep = (np.abs(dp - dp_ref).max() - extra_p) / max(np.abs(dp_ref).max(), 1e-30)
    print(f", dq {eq / tol:.3f}, dp {ep / tol:.3f} of the tolerance", end="")
    assert eq < tol, (name, "dq", eq, tol)
    assert ep < tol, (name, "dp", ep, tol)


def _run_inbatch(Q, P, d, tag, regime, aligned=True, window=None, tol=None, gemm=False):
    label, bc = U.infonce_path(Q, P, d, tag, aligned)
    qn, pn, T, mk = U.infonce_regime(regime, Q, P, d, bc)
    name = f"{Q}x{P}x{d} {tag} {regime} [{label}]"
    o = ops()
    if window is None:
        q, p = dev(qn, tag, True, aligned), dev(pn, tag, True, aligned)
        qv, pv = npf(q), npf(p)
        loss, scores = o.infonce_loss(q, p, T)
        q0, qr, p0, pr = 0, Q, 0, P
        ql, pl = q, p
    else:
        q0, qr, p0, pr = window
        qa, pa = dev(qn, tag), dev(pn, tag)
        qv, pv = npf(qa), npf(pa)
        ql, pl = qa[q0:q0 + qr].clone().requires_grad_(True), pa[p0:p0 + pr].clone().requires_grad_(True)
        loss, scores = o.infonce_loss(ql, pl, T, True, q_all=qa, p_all=pa, q_row0=q0, p_row0=p0)
    lse_t = npf(loss.grad_fn.saved_tensors[3])
    (loss * U.GL).backward()
    s = npf(scores)
    exp = U.expected_scores(R.similarity(qv, pv), T, tag)
    ce = _check_forward(loss.item(), lse_t, s, exp, mk["target"], tag, name)
    if regime == "flat":
        assert abs(loss.item() - np.log(P)) <= U.loss_bound(ce), (name, loss.item(), np.log(P))
    ds, dq_ref, dp_ref = U.softmax_grads(s, ce, mk["target"], T, U.GL, qv, pv)
    _check_grads(npf(ql.grad), npf(pl.grad), ds, dq_ref[q0:q0 + qr], dp_ref[p0:p0 + pr], qv, pv, tag, regime, name,
                 tol or GRAD_TOL[tag], gemm_K=(P, Q) if gemm else None)
    return loss


INBATCH = [(c, tag, r) for c in U.INFONCE_CASES for tag in U.DTYPES if tag in c[3] for r in U.INFONCE_REGIMES]


@pytest.mark.parametrize("case,tag,regime", INBATCH, ids=[f"{U.case_id(c)}-{t}-{r}" for c, t, r in INBATCH])
def test_infonce_parity_every_path(case, tag, regime):
    """Every forward path x dtype x regime; problems of 256 Ki pairs and more take the dS + two GEMMs backward, whose dS is rounded
    to the storage dtype first: their tolerances are test_infonce_backward_gemm_form's (and test_gpu_f16.py's for fp16)."""
    Q, P, d, _, aligned = case
    gemm = Q * P >= ops()._GEMM_BWD_MIN_PAIRS
    _run_inbatch(Q, P, d, tag, regime, aligned, tol=GEMM_GRAD_TOL[tag] if gemm else None, gemm=gemm)


@pytest.mark.parametrize("arm", ["hip", "blaslt"])
@pytest.mark.parametrize("tag", U.DTYPES)
@pytest.mark.parametrize("regime", U.INFONCE_REGIMES)
def test_infonce_parity_gemm_form_backward(regime, tag, arm, monkeypatch):
    """(512, 1536, 128) through the dS + two GEMMs backward on both INFONCE_BWD_GEMM arms, in every regime."""
    o = ops()
    monkeypatch.setattr(o, "INFONCE_BWD_GEMM", arm)
    calls = []
    real = o.sim_gemm_nt
    monkeypatch.setattr(o, "sim_gemm_nt", lambda b, a: (calls.append(tuple(b.shape)), real(b, a))[1])
    Q, P, d = U.GEMM_CASE
    assert Q * P >= o._GEMM_BWD_MIN_PAIRS
    _run_inbatch(Q, P, d, tag, regime, tol=GEMM_GRAD_TOL[tag], gemm=True)
    assert len(calls) == (2 if arm == "hip" and tag == "bf16" else 0), calls      # the hand-written frame ran where it applies


@pytest.mark.parametrize("tag", U.DTYPES)
@pytest.mark.parametrize("regime", U.INFONCE_REGIMES)
def test_infonce_parity_own_row_window(regime, tag):
    """q_all / p_all with non-zero q_row0 / p_row0: gradients for the own rows only, in every regime."""
    Q, P, d, win = U.WINDOW_CASE
    _run_inbatch(Q, P, d, tag, regime, window=win)


@pytest.mark.parametrize("tag", U.DTYPES)
def test_infonce_hot_twice_is_bit_identical(tag):
    """A multi-block skinny launch (ticket finalize) twice in a row on the same `hot` inputs -- two ticket slots --: the same bits."""
    Q, P, d = U.TWICE_CASE
    assert U.infonce_path(Q, P, d, tag)[0] == "skinny-multi"
    a = _run_inbatch(Q, P, d, tag, "hot")
    b = _run_inbatch(Q, P, d, tag, "hot")
    assert a.item() == b.item()


FIRST = [(c, tag, r) for c in U.FIRST_CASES for tag in U.DTYPES for r in U.FIRST_REGIMES]


@pytest.mark.parametrize("case,tag,regime", FIRST, ids=[f"{c[0]}x{c[1]}x{c[2]}-{t}-{r}" for c, t, r in FIRST])
def test_infonce_parity_first_target(case, tag, regime):
    """RPO_TARGET_FIRST (use_inbatch_neg=False): grouped dots (vector and scalar arm), first_finalize_kernel (B = 300: two trips of
    its row loop) and infonce_first_bwd_kernel; the same three assertions on the [B, G] scores."""
    B, G, d = case
    qn, pn, T, mk = U.first_regime(regime, B, G, d)
    name = f"first {B}x{G}x{d} {tag} {regime}"
    q, p = dev(qn, tag, True), dev(pn, tag, True)
    qv, pv = npf(q), npf(p)
    loss, scores = ops().infonce_loss(q, p, T, use_inbatch_neg=False)
    assert tuple(scores.shape) == (B, G)
    lse_t = npf(loss.grad_fn.saved_tensors[3])
    (loss * U.GL).backward()
    s = npf(scores)
    exp = U.expected_scores(np.einsum("bd,bgd->bg", qv, pv.reshape(B, G, d)), T, tag)
    tgt = np.zeros(B, dtype=np.int64)
    ce = _check_forward(loss.item(), lse_t, s, exp, tgt, tag, name)
    if regime == "flat":
        assert abs(loss.item() - np.log(G)) <= U.loss_bound(ce), (name, loss.item(), np.log(G))
    if regime == "hot" and G > 1:
        assert (ce["rowloss"][mk["planted"] == 0] < 1e-6).all() and (ce["rowloss"][mk["planted"] != 0] > 100).all()
    ds, dq_ref, dp_ref = U.softmax_grads(s, ce, tgt, T, U.GL, qv, pv, first_G=G)
    if G == 1:                                             # one column: dS == 0 exactly, so are the gradients
        assert not npf(q.grad).any() and not npf(p.grad).any()
        return
    _check_grads(npf(q.grad), npf(p.grad), ds, dq_ref, dp_ref, qv, pv, tag, regime, name, GRAD_TOL[tag])


# ------------------------------------------------------------------------------------------------------------------ RankPO
# test_rankpo_golden (f32, bf16) and test_rankpo_golden_vs_reference_16_bit (f16: scores and loss as bf16, gradients 8 u = 2^-8)
RANKPO_TOL = {"f32": dict(loss=(2e-5, 1e-6), grad=1e-4), "bf16": dict(loss=(3e-5, 1e-6), grad=2.0 ** -7),
              "f16": dict(loss=(3e-5, 1e-6), grad=2.0 ** -8)}
F16_MAX = 65504.0
RANKPO = [(sh, tag, name) for sh in U.RANKPO_SHAPES for tag in U.DTYPES for name in U.RANKPO_REGIMES]


def _rankpo_grad_check(got, ref, tag, what, scale):
    """|got - ref| <= tol * (largest entry) + 2^-23 * scale (+ 2^-25 in fp16).  `scale` is the size of a gradient entry whose sigmoid
    / softmax factor is 1: gl (beta w_rankpo + w_sft) / (B T) max |x|.  The kernel forms those factors in float32 (`expf(t0 - lse)
    - 1.f`, `sigmoidf`), i.e. with an absolute error of an ulp32 of 1, so a batch whose every row is saturated (B = 1 in `sat`: the
    true gradient is 1e-24 of the scale) comes back as exact zeros; fp16 also flushes below its smallest subnormal 2^-24.
    fp16 under grad_loss = 2^12 in the saturated regimes: entries of the true gradient beyond the fp16 range (65504) must come back
    at least that large (inf), with the right sign; the rest is compared as usual."""
    if tag == "f16":
        over = np.abs(ref) > F16_MAX * (1 + 2.0 ** -10)
        if over.any():
            assert (np.abs(got[over]) >= F16_MAX).all() and (np.sign(got[over]) == np.sign(ref[over])).all(), what
        near = (np.abs(ref) > F16_MAX * (1 - 2.0 ** -10)) & ~over          # within an ulp of the range's end: either side
        keep = ~over & ~near
        if not keep.any():
            return
        got, ref = got[keep], ref[keep]
    assert np.isfinite(got).all(), what
    allowed = RANKPO_TOL[tag]["grad"] * np.abs(ref).max() + 2.0 ** -23 * scale + (2.0 ** -25 if tag == "f16" else 0.0)
    assert np.abs(got - ref).max() <= allowed, (what, np.abs(got - ref).max(), allowed)


@pytest.mark.parametrize("shape,tag,name", RANKPO, ids=[f"{s[0]}x{s[1]}{'' if s[2] else '-unaligned'}-{t}-{n}" for s, t, n in RANKPO])
def test_rankpo_parity(shape, tag, name):
    """rpo_rankpo_fwd / rpo_rankpo_bwd through ops.rankpo_loss_metrics against R.rankpo_batch_loss_metrics on the stored inputs:
    scores, per-row losses, loss, every metric, dq and dp under grad_loss = 1 and 2^12, dq-only and dp-only calls; and the per-row
    losses / the loss against the float64 formulas on the RETURNED scores inside the derived float32 bound (util docstring)."""
    from rankpo_amd._lib import METRIC_KEYS
    B, d, aligned = shape
    cfg = U.rankpo_config(name)
    qn, pn, rcn, rrn, mk = U.rankpo_regime(name, B, d, tag)
    o = ops()
    c_cfg = o.RankPOConfig(**cfg)
    rc = None if rcn is None else dev(rcn, "f32")
    rr = None if rrn is None else dev(rrn, "f32")
    tol = RANKPO_TOL[tag]
    ref = None
    for gl, need_q, need_p in ((1.0, True, True), (4096.0, True, True), (1.0, False, True), (1.0, True, False)):
        q, p = dev(qn, tag, need_q, aligned), dev(pn, tag, need_p, aligned)
        loss, scores, losses, metrics = o.rankpo_loss_metrics(q, p, c_cfg, rc, rr)
        (loss * gl).backward()
        assert (q.grad is not None) == need_q and (p.grad is not None) == need_p
        if ref is None:
            np.testing.assert_array_equal(npf(q), qn)             # the builder's values are exact in the storage dtype
            ref = R.rankpo_batch_loss_metrics(qn, pn, rcn, rrn, **cfg)
            s, lb, m = npf(scores), npf(losses), npf(metrics)
            assert np.isfinite(s).all() and np.isfinite(lb).all() and np.isfinite(m).all() and np.isfinite(loss.item())
            np.testing.assert_allclose(s, ref["scores"], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(lb, ref["losses"], rtol=2e-5, atol=2e-6)
            np.testing.assert_allclose(loss.item(), ref["loss"], rtol=tol["loss"][0], atol=tol["loss"][1])
            for i, k in enumerate(METRIC_KEYS):
                np.testing.assert_allclose(m[i], ref["metrics"].get(k, 0.0), rtol=2e-5, atol=2e-6, err_msg=k)
            # the finalize kernel alone: float64 formulas on the scores it was given
            l64, sft64, bound = U.rankpo_rows_f64(s, rcn, rrn, cfg)
            r_row = float((np.abs(lb - l64) / bound).max())
            loss64 = cfg["rankpo_weight"] * l64.mean() + (cfg["sft_weight"] * sft64.mean() if cfg["sft_weight"] > 0 else 0.0)
            r_loss = abs(loss.item() - loss64) / U.rankpo_loss_bound(l64, sft64, bound, cfg)
            print(f"\nrankpo {B}x{d} {tag} {name}: rows {r_row:.3f}, loss {r_loss:.3f} of the bound (loss {loss.item():.4f})", end="")
            assert r_row <= 1.0 and r_loss <= 1.0, (r_row, r_loss)
            if mk["kink"].any():                                  # exactly on the hinge kink: loss 0, gradient 0
                assert not lb[mk["kink"]].any()
                assert not npf(q.grad)[mk["kink"]].any() and not npf(p.grad)[np.repeat(mk["kink"], 2)].any()
        scale = gl * (cfg["beta"] * cfg["rankpo_weight"] + cfg["sft_weight"]) / (B * cfg["temperature"])
        if need_q:
            _rankpo_grad_check(npf(q.grad), gl * ref["dq"], tag, (name, "dq", gl), scale * np.abs(pn).max())
        if need_p:
            _rankpo_grad_check(npf(p.grad), gl * ref["dp"], tag, (name, "dp", gl), scale * np.abs(qn).max())
