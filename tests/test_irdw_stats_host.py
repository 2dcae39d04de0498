"""tests/_irdw_stats_ref.py on the host: the float64 reference of nasseg_irdw_stats is torch's own training-mode
BatchNorm of conv2d(pro(x), w1) in float64, and its input generator delivers the regime the GPU test asserts in."""
import pytest
import torch
import torch.nn.functional as TF

import _irdw_stats_ref as R


@pytest.mark.parametrize("case", [((2, 16, 96, 7, 9), 1, 50.0), ((1, 8, 48, 5, 13), 2, 10.0),
                                  ((3, 24, 144, 6, 5), 0, 200.0), ((1, 4, 16, 9, 8), 3, 50.0)],
                         ids=lambda c: "{}to{}_pro{}_ratio{:g}".format(c[0][1], c[0][2], c[1], c[2]))
def test_reference_is_float64_batch_norm_of_the_expansion(case):
    (B, K, C, H, W), pro, ratio = case
    x, w1, (isc, ish, iact) = R.make_inputs(B, K, C, H, W, ratio, pro, seed=3)
    g = torch.Generator().manual_seed(5)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    eps, mom = 1e-5, 0.1
    got = R.statistics(x, w1, isc, ish, iact, gamma, beta, eps, mom, rm0, rv0)
    # pro(x): float64 holds the 48-bit product of two fp32 numbers exactly; the sum is then rounded to fp32 like the
    # kernels' fused multiply-add rounds it
    xt = x.double()
    if pro:
        xt = (xt * isc.double().view(1, K, 1, 1) + ish.double().view(1, K, 1, 1)).float().double()
        if iact:
            xt = TF.relu6(xt) if iact == R.ACT_RELU6 else TF.relu(xt)
    z = TF.conv2d(xt, w1.double())
    rm, rv = rm0.double().clone(), rv0.double().clone()
    y = TF.batch_norm(z, rm, rv, gamma.double(), beta.double(), True, R.f32(mom), R.f32(eps))
    assert torch.allclose(got["z1"], z, rtol=1e-13, atol=1e-12)
    assert torch.allclose(got["mean"], z.mean((0, 2, 3)), rtol=1e-13, atol=1e-13)
    assert torch.allclose(got["var"], z.var((0, 2, 3), unbiased=False), rtol=1e-10, atol=0.0)
    assert torch.allclose(got["invstd"], 1.0 / torch.sqrt(got["var"] + R.f32(eps)), rtol=1e-14, atol=0.0)
    mine = got["scale"].view(1, C, 1, 1) * z + got["shift"].view(1, C, 1, 1)
    # (scale * z + shift cancels |mean| / std = some hundreds of units of the normalised value: 1e-9 is 1e7 ulp of it)
    assert float((mine - y).abs().max()) < 1e-9
    assert torch.allclose(got["running_mean"], rm, rtol=1e-12, atol=1e-13)
    assert torch.allclose(got["running_var"], rv, rtol=1e-10, atol=0.0)


@pytest.mark.parametrize("pro", R.PROS)
@pytest.mark.parametrize("ratio", [10.0, 50.0, 200.0])
@pytest.mark.parametrize("geom", [(1, 16, 96, 7, 9), (1, 4, 16, 33, 31), (2, 24, 144, 31, 17)],
                         ids=lambda g: "B{}_{}to{}_{}x{}".format(*g))
def test_generator_delivers_the_regime(geom, ratio, pro):
    B, K, C, H, W = geom
    x, w1, (isc, ish, iact) = R.make_inputs(B, K, C, H, W, ratio, pro)
    assert tuple(w1.shape) == (C, K, 1, 1) and x.dtype == w1.dtype == torch.float32
    assert (isc is None) == (ish is None) == (pro == 0) and iact == max(pro - 1, 0)
    xt = R.prologue(x, isc, ish, iact)
    mean, std = xt.mean((0, 2, 3)), xt.std((0, 2, 3))
    live = std > 0  # (a ReLU clamps the channels with a negative mean to a constant 0)
    if pro == 2:
        assert int(live.sum()) >= (K + 1) // 2 and bool((xt[:, ~live] == 0).all()) and bool((mean[live] > 0).all())
    else:
        assert bool(live.all())
    if pro == 3:
        assert 2.0 * 0.97 < float(mean.min()) and float(mean.max()) < 4.0 * 1.03 and float(xt.max()) < 6.0
    else:
        assert 0.35 < float(std[live].min()) and float(std[live].max()) < 1.95
    r = mean[live].abs() / std[live]
    # (M >= 63 samples: the sample deviation is within 30 % of the channel's, the sample mean within half a deviation)
    assert ratio * 0.7 < float(r.min()) and float(r.max()) < ratio * 1.4
    worst, vmin = R.regime(x, w1, (isc, ish, iact))
    assert vmin > 0.0
    if ratio == 200.0:
        assert worst > 100.0, "no output channel of the expansion with |mean| > 100 std ({:.1f})".format(worst)


def test_bf16_storage_keeps_the_regime():
    """x rounded to bf16 is what the kernels read: without a prologue the rounding step is of the deviation's own size
    (2^-8 of 200 deviations) - the stored map still has a mean some hundred times its deviation"""
    x, w1, pa = R.make_inputs(2, 24, 144, 31, 17, 200.0, 0)
    worst, vmin = R.regime(x.to(torch.bfloat16).float(), w1, pa)
    assert worst > 100.0 and vmin > 0.0


def test_ulp32():
    v = torch.tensor([1.0, -3.0, 489.5, 1e-3], dtype=torch.float64)
    assert R.ulp32(v).tolist() == [2.0 ** -23, 2.0 ** -22, 2.0 ** -15, 2.0 ** -33]
