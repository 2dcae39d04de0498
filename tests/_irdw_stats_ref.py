"""Float64 restatement of nasseg_irdw_stats (csrc/irdw.hip): the train-mode BatchNorm statistics of InvertedResidual's
expansion z1 = W1 pro(x), and the inputs that put them in the regime |mean| >> std.

The prologue is the one fp32 fused multiply-add the kernels perform - float32(float64(x) * float64(scale) +
float64(shift)), then the clamp - and everything after it is float64: z1 itself, a two-pass mean / variance, invstd,
scale, shift and the running statistics.  ``eps`` and ``momentum`` enter as the fp32 values the C ABI passes.
Shared by tests/test_irdw_stats_host.py (no GPU) and tests/test_hip_irdw.py."""
import torch

ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2
# prologues of the generator: 0 none, 1 affine (linear bottleneck), 2 affine + ReLU, 3 affine + ReLU6
PROS = (0, 1, 2, 3)


def f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def prologue(x, in_scale, in_shift, in_act):
    """pro(x) for x (B, K, H, W) as stored (fp32, or bf16 widened): fp32 values, returned in float64"""
    v = x.double()
    if in_scale is not None or in_shift is not None or in_act != ACT_NONE:
        K = x.shape[1]
        sc = torch.ones(K) if in_scale is None else in_scale
        sh = torch.zeros(K) if in_shift is None else in_shift
        v = (v * sc.double().view(1, K, 1, 1) + sh.double().view(1, K, 1, 1)).float()  # (the FMA's one rounding)
        if in_act == ACT_RELU:
            v = v.clamp(min=0.0)
        elif in_act == ACT_RELU6:
            v = v.clamp(min=0.0, max=6.0)
        else:
            assert in_act == ACT_NONE
        v = v.double()
    return v


def expansion(x, w1, in_scale, in_shift, in_act):
    """z1 = W1 pro(x) in float64: (B, C, H, W)"""
    C, K = w1.shape[0], w1.shape[1]
    return torch.einsum("bkhw,ck->bchw", prologue(x, in_scale, in_shift, in_act), w1.double().view(C, K))


def statistics(x, w1, in_scale, in_shift, in_act, gamma, beta, eps, momentum, running_mean, running_var):
    """-> dict of float64 tensors: mean, var (biased), invstd, scale, shift, running_mean, running_var - and z1"""
    z = expansion(x, w1, in_scale, in_shift, in_act)
    B, C, H, W = z.shape
    M = B * H * W
    mean = z.mean(dim=(0, 2, 3))
    var = ((z - mean.view(1, C, 1, 1)) ** 2).mean(dim=(0, 2, 3))
    e, m = f32(eps), f32(momentum)
    invstd = 1.0 / torch.sqrt(var + e)
    g = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    b = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    scale = g * invstd
    unbiased = var * M / (M - 1) if M > 1 else var
    return {"mean": mean, "var": var, "invstd": invstd, "scale": scale, "shift": b - mean * scale,
            "running_mean": (1.0 - m) * running_mean.double() + m * mean,
            "running_var": (1.0 - m) * running_var.double() + m * unbiased, "z1": z}


def make_inputs(B, K, C, H, W, ratio, pro, seed=0):
    """-> x (B, K, H, W), w1 (C, K, 1, 1), (in_scale, in_shift, in_act), all fp32: every channel of pro(x) has a
    deviation in [0.5, 1.5) and a mean of sign * ratio deviations.  The large mean sits in x without a prologue and in
    in_shift with one (x is then N(0, 1) and in_scale the deviation).  ReLU: at least half of the channels have a
    positive mean - the others are clamped to a constant 0 - so that every output channel keeps a variance.  ReLU6:
    mean in [2, 4], deviation mean / ratio, so that the clamp leaves the values alone.  w1 = randn / sqrt(K)."""
    assert pro in PROS and ratio >= 8.0
    g = torch.Generator().manual_seed(seed)
    std = torch.rand(K, generator=g) + 0.5
    sign = torch.where(torch.rand(K, generator=g) > 0.5, 1.0, -1.0)
    order = torch.randperm(K, generator=g)
    lift = 2.0 + 2.0 * torch.rand(K, generator=g)
    if pro == 2:
        sign[order[:(K + 1) // 2]] = 1.0
    if pro == 3:
        sign, std = torch.ones(K), lift / ratio
        mean = lift
    else:
        mean = sign * ratio * std
    n = torch.randn(B, K, H, W, generator=g)
    w1 = torch.randn(C, K, 1, 1, generator=g) / K ** 0.5
    if pro == 0:
        return n * std.view(1, K, 1, 1) + mean.view(1, K, 1, 1), w1, (None, None, ACT_NONE)
    return n, w1, (std, mean, pro - 1)


def regime(x, w1, pro_args):
    """(largest |mean| / std over the output channels, smallest variance over the output channels) of z1"""
    z = expansion(x, w1, *pro_args)
    mean, var = z.mean(dim=(0, 2, 3)), z.var(dim=(0, 2, 3), unbiased=False)
    assert float(var.min()) > 0.0, "an output channel of the expansion is constant"
    return float((mean.abs() / var.sqrt()).max()), float(var.min())


def ulp32(v):
    """the spacing of fp32 numbers at |v| (float64 tensor -> float64 tensor)"""
    a = v.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()
