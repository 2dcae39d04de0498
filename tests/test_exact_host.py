"""The exact-arithmetic method of tests/_exact.py, proved on the CPU: on the generators' outputs torch's own fp32
convolutions - forward, input gradient, weight gradient - equal float64 bit for bit, in two different summation
orders, at the largest geometries tests/test_hip_exact.py uses; the precondition accepts those inputs and rejects an
oversized one; the generators' values survive bf16 storage."""
import pytest
import torch
import torch.nn.functional as TF

import _exact as E

# B, K, H, W, N, k, stride, pad, dil: the largest dense geometries of test_hip_kernels.CONV_CASES (the LDS-tiled 3x3
# weight gradient over 20 000 - 25 000 pixels, the widest reductions) and the largest depthwise one (N = 0)
GEOMS = [
    (2, 64, 96, 128, 19, 3, 1, 1, 1),
    (1, 128, 128, 160, 12, 3, 1, 1, 1),
    (1, 32, 130, 131, 16, 3, 1, 2, 2),
    (2, 64, 64, 64, 64, 3, 1, 1, 1),
    (1, 160, 4, 5, 960, 1, 1, 0, 1),
    (2, 3, 33, 37, 32, 3, 2, 1, 1),
    (1, 64, 30, 200, 0, 5, 1, 24, 12),
]


def _case(geom):
    B, K, H, W, N, k, s, p, d = geom
    groups = 1
    if N == 0:
        N, groups = K, K
    x = E.ints(B, K, H, W, seed=1)
    w = E.ints(N, K // groups, k, k, seed=2)
    Ho, Wo = (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1
    dy = E.ints(B, N, Ho, Wo, seed=3)
    return x, w, dy, (s, p, d, groups)


def _conv_all(x, w, dy, cfg):
    """forward, input gradient, weight gradient of conv2d in the dtype of the inputs"""
    s, p, d, groups = cfg
    y = TF.conv2d(x, w, None, s, p, d, groups)
    dx = torch.nn.grad.conv2d_input(x.shape, w, dy, s, p, d, groups)
    dw = torch.nn.grad.conv2d_weight(x, w.shape, dy, s, p, d, groups)
    return y, dx, dw


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "B{}K{}_{}x{}_N{}_k{}s{}p{}d{}".format(*g))
def test_fp32_convolutions_equal_float64_in_two_summation_orders(geom):
    x, w, dy, cfg = _case(geom)
    groups = cfg[3]
    E.assert_exactly_summable(lambda a, b, c: _conv_all(a, b, c, cfg), [x, w, dy], 1.0, "conv")
    ref = _conv_all(x.double(), w.double(), dy.double(), cfg)
    got = _conv_all(x, w, dy, cfg)
    for g, r, what in zip(got, ref, ("forward", "input gradient", "weight gradient")):
        E.assert_bitwise(g, r, what)
    # another summation order: batch reversed, channels permuted (input channels for a dense conv)
    B, K = x.shape[0], x.shape[1]
    pb = torch.arange(B - 1, -1, -1)
    pk = torch.randperm(K, generator=torch.Generator().manual_seed(4))
    xp = x[pb][:, pk].contiguous()
    dyp = dy[pb].contiguous()
    if groups == 1:
        wp = w[:, pk].contiguous()
    else:
        wp, dyp = w[pk].contiguous(), dyp[:, pk].contiguous()
    y, dx, dw = _conv_all(xp, wp, dyp, cfg)
    inv_b, inv_k = torch.argsort(pb), torch.argsort(pk)
    if groups == 1:
        y, dx, dw = y[inv_b], dx[inv_b][:, inv_k], dw[:, inv_k]
    else:
        y, dx, dw = y[inv_b][:, inv_k], dx[inv_b][:, inv_k], dw[inv_k]
    for g, r, what in zip((y, dx, dw), ref, ("forward", "input gradient", "weight gradient")):
        E.assert_bitwise(g, r, what + " (permuted order)")


def test_the_precondition_rejects_an_oversized_input():
    x, w, dy, cfg = _case(GEOMS[0])
    with pytest.raises(AssertionError):
        E.assert_exactly_summable(lambda a, b, c: _conv_all(a, b, c, cfg), [x * 64, w, dy * 64], 1.0, "oversized")
    # ... and a unit that is too fine for the magnitudes (values of 3 in units of 2^-24)
    with pytest.raises(AssertionError):
        E.assert_exactly_summable(lambda a: a, [torch.full((4,), 3.0)], 2.0 ** -24, "fine unit")
    with pytest.raises(AssertionError):
        E.assert_stats_summable(torch.full((1, 2, 4096, 4096), 2.0), 1.0, "statistics")
    E.assert_stats_summable(E.ints(2, 8, 64, 64, seed=5), 1.0, "statistics")


def test_the_oversized_input_really_rounds_in_fp32():
    """the bound is not vacuous: past it torch's fp32 weight gradient does leave the float64 value"""
    x = torch.full((1, 1, 4200, 4200), 1.0)
    x[0, 0, 0, 0] = 0.5
    dy = torch.ones(1, 1, 4200, 4200)
    got = torch.nn.grad.conv2d_weight(x, (1, 1, 1, 1), dy)
    ref = torch.nn.grad.conv2d_weight(x.double(), (1, 1, 1, 1), dy.double())
    with pytest.raises(AssertionError):
        E.assert_exactly_summable(lambda a, b: torch.nn.grad.conv2d_weight(a, (1, 1, 1, 1), b), [x, dy], 0.5, "big")
    assert float(got) != float(ref)


def test_generated_values_survive_bf16_storage():
    vals = [E.ints(3, 5, 7, seed=1), E.ints(100, lo=-127, hi=127, seed=2), E.halves(64, seed=3),
            E.ints(64, lo=-1, hi=1, density=0.3, seed=4), E.ints(64, lo=-4, hi=4, unit=64.0, seed=5),
            E.pow2(32, -3, 3, seed=6)] + E.bn_vectors(32, 7, tie=True) + E.bn_vectors(32, 8, tie=False)
    for v in vals:
        assert v.dtype == torch.float32
        assert torch.equal(v.to(torch.bfloat16).float(), v)
    assert torch.equal(E.ints(3, 5, seed=9), E.ints(3, 5, seed=9))  # seeded
    h = E.halves(1000, seed=10)
    assert bool(((h * 2) % 2 == 1).all())
    assert float(E.ints(1000, lo=-1, hi=1, density=0.2, seed=11).abs().mean()) < 0.3


def test_assert_bitwise_reports_the_first_difference():
    ref = torch.arange(6.0).double().view(2, 3)
    E.assert_bitwise(ref.float(), ref, "same")
    got = ref.float().clone()
    got[1, 0] += 2.0 ** -20
    got[1, 2] = 0.0
    with pytest.raises(AssertionError) as info:
        E.assert_bitwise(got, ref, "dx")
    msg = str(info.value)
    assert "dx" in msg and "2 of 6" in msg and "(1, 0)" in msg
    # bf16 (steps of 2 above 256): round to nearest even of the exact value, not truncation - 257 -> 256 (128 steps,
    # even), 259 -> 260 (130 steps), 258 stays, 261 -> 260
    exact = torch.tensor([257.0, 259.0, 258.0, 261.0]).double()
    rne = torch.tensor([256.0, 260.0, 258.0, 260.0]).to(torch.bfloat16)
    E.assert_bitwise(rne, exact, "rounded")
    trunc = torch.tensor([256.0, 258.0, 258.0, 260.0]).to(torch.bfloat16)
    with pytest.raises(AssertionError):
        E.assert_bitwise(trunc, exact, "truncated")
    with pytest.raises(AssertionError):
        E.assert_bitwise(torch.tensor([float("nan")]), torch.tensor([0.0]).double(), "nan")


def test_the_bf16_comparison_overlooks_the_sign_of_a_zero_and_nothing_else():
    """-0 counts as +0 on either side (a masked gradient g * 0 is -0 for a negative g, and == does not see that in
    fp32 either); the smallest subnormal, a flipped sign of a non-zero value and a NaN are still differences"""
    bf = torch.bfloat16
    zeros = torch.tensor([0.0, -0.0, 0.0, -0.0])
    E.assert_bitwise(zeros.to(bf), torch.tensor([0.0, 0.0, -0.0, -0.0]).double(), "zeros")
    E.assert_bitwise(zeros, torch.tensor([0.0, 0.0, -0.0, -0.0]).double(), "zeros, fp32")
    tiny = torch.tensor([1], dtype=torch.int16).view(bf)  # (the smallest positive subnormal)
    assert float(tiny) > 0
    for got, ref in ((tiny, torch.zeros(1)), (-tiny, torch.zeros(1)), (torch.zeros(1).to(bf), tiny.float()),
                     (torch.tensor([-1.0]).to(bf), torch.ones(1)), (torch.tensor([float("nan")]).to(bf), torch.zeros(1)),
                     (torch.tensor([-0.0]).to(bf), torch.tensor([float("nan")]))):
        with pytest.raises(AssertionError):
            E.assert_bitwise(got, ref.double(), "not a zero")
