"""CPU tests of `ops.split_bf16x3_ref`, the oracle of the split kernel behind FlatIPIndex(f32_planes=True): an f32 value as three bf16
planes h | m | l with x == h + m + l, and the cases in which that is reported not to hold."""
import torch

from rankpo_amd.ops import split_bf16x3_ref


def _values(n=100_000, seed=0):
    """n f32 values with full 24-bit significands, exponents spread over -100 .. 100, both signs."""
    g = torch.Generator().manual_seed(seed)
    mant = 1.0 + torch.rand(n, generator=g, dtype=torch.float64)
    e = torch.randint(-100, 101, (n,), generator=g)
    sign = torch.randint(0, 2, (n,), generator=g) * 2 - 1
    return (sign * mant * torch.pow(torch.tensor(2.0, dtype=torch.float64), e)).float()


def test_three_planes_add_up_to_the_value_bit_for_bit():
    x = _values()
    planes, inexact = split_bf16x3_ref(x[:, None])
    assert planes.dtype == torch.bfloat16 and planes.shape == (x.numel(), 3) and not bool(inexact)
    h, m, l = (planes[:, i].float() for i in range(3))
    s = h + m + l                                                      # f32 sums, in this order
    assert torch.equal(s.view(torch.int32), x.view(torch.int32))
    assert int((m != 0).sum()) > 90_000 and int((l != 0).sum()) > 90_000          # (all three planes are live)


def test_each_plane_is_its_own_bf16_rounding_and_the_residuals_shrink():
    x = _values(seed=1)
    planes, _ = split_bf16x3_ref(x[:, None])
    h, m, l = (planes[:, i].float() for i in range(3))
    assert torch.equal(planes[:, 0], x.to(torch.bfloat16))
    assert torch.equal(planes[:, 1], (x - h).to(torch.bfloat16))
    assert torch.equal(planes[:, 2], (x - h - m).to(torch.bfloat16))
    assert bool((m.abs() <= 2.0 ** -8 * x.abs()).all()) and bool((l.abs() <= 2.0 ** -16 * x.abs()).all())


def test_layout_is_h_m_l_per_row():
    x = _values(4 * 64, seed=2).view(4, 64)
    planes, inexact = split_bf16x3_ref(x)
    assert planes.shape == (4, 192) and not bool(inexact)
    assert torch.equal(planes[:, :64], x.to(torch.bfloat16))
    assert torch.equal(planes[:, :64].float() + planes[:, 64:128].float() + planes[:, 128:].float(), x)


def test_zeros_are_exact():
    x = torch.tensor([[0.0, -0.0, 1.0, -3.5]])
    planes, inexact = split_bf16x3_ref(x)
    assert not bool(inexact) and torch.equal(planes[:, :4].float(), x) and not bool(planes[:, 4:].float().any())


def test_underflowing_planes_and_non_finite_values_are_reported():
    ok = _values(64, seed=3)[None, :]
    assert not bool(split_bf16x3_ref(ok)[1])
    for bad in (2.0 ** -130 * 1.2345,                                  # the planes underflow: h + m + l != x
                2.0 ** -130,                                           # h is a bf16 subnormal (the sum holds, the premise does not)
                1.2345 * 2.0 ** -118,                                  # h normal, l a subnormal
                float("inf"), float("-inf"), float("nan")):
        x = ok.clone()
        x[0, 17] = bad
        assert bool(split_bf16x3_ref(x)[1]), bad
    x = ok.clone()
    x[0, 17] = torch.finfo(torch.float32).max                           # rounds up to inf in bf16
    assert bool(split_bf16x3_ref(x)[1])
