"""Torch-CPU restatement of the depth criterion with its scale-invariant log and gradient-matching terms
(F.depth_criterion; definition: include/nasseg.h, "Depth terms"): float64 by default, slices, masks and ``abs``,
gradients from autograd.  It starts from the same fp32 inputs as the kernels (a bf16 prediction is widened exactly
before it comes here) and takes the fp32 values of ``pred_min`` and the valid range, which are what the kernels get.
Shared by tests/test_depth_terms_host.py (no GPU) and tests/test_hip_depth_terms.py."""
import torch
import torch.nn.functional as TF

INF = float("inf")
# The bound of the GPU tests, derived - not measured: with |ln| < 8 and logf within 2 ulp, r is off by at most 2^-19;
# a term (a mean of r^2, or of |r_j - r_i|) is then off by at most 2 * 8 * 2^-19 = 2^-15.  A wrong neighbour, count or
# stride moves a term by far more.
TERM_TOL = 2.0 ** -15
GRAD_TOL = 2.0 ** -15   # of the largest |gradient| of the float64 reference, per element
BF16_TOL = 2.0 ** -8    # added per element for bf16 storage: one rounding of the stored value
SIGN_BAND = 1e-4        # |r_i - r_j| below this: the sign is decided by fp32 rounding of r
SIGN_SHARE = 0.02       # such pixels may be at most this share of the valid ones


def f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def make_inputs(B, h, w, H, W, seed=0):
    """-> pred (B, 1, h, w), target (B, H, W), fp32: t uniform in [0.5, 8] with 20 % holes (0, NaN or inf, in equal
    shares); p = the sampled t * exp(N(0, 0.3)), 3 % of the p from {-1, 0, 5e-4}: at or below pred_min"""
    g = torch.Generator().manual_seed(seed)
    t = 0.5 + 7.5 * torch.rand(B, H, W, generator=g)
    hole = torch.rand(B, H, W, generator=g) < 0.2
    kind = torch.randint(0, 3, (B, H, W), generator=g)
    t[hole & (kind == 0)] = 0.0
    t[hole & (kind == 1)] = float("nan")
    t[hole & (kind == 2)] = INF
    ts = sample(t, h, w)
    ts = torch.where(torch.isfinite(ts) & (ts > 0), ts, torch.ones_like(ts))
    p = ts * torch.exp(0.3 * torch.randn(B, h, w, generator=g))
    low = torch.rand(B, h, w, generator=g) < 0.03
    vals = torch.tensor([-1.0, 0.0, 5e-4])[torch.randint(0, 3, (B, h, w), generator=g)]
    p[low] = vals[low]
    return p[:, None].contiguous(), t


def sample(target, h, w):
    """the target pixel every prediction pixel meets: F.interpolate(mode="nearest") -> (B, h, w)"""
    return TF.interpolate(target[:, None], size=(h, w), mode="nearest")[:, 0]


def criterion(pred, target, valid_min=0.0, valid_max=INF, berhu_weight=1.0, silog_weight=None, silog_lambda=0.5,
              grad_weight=None, grad_scales=4, pred_min=1e-3, dtype=torch.float64):
    """pred (B, 1, h, w) - fp32, or ``dtype`` with requires_grad for a gradient; target (B, H, W) fp32.  -> dict:
    total, berhu, D, L_gm (0-dim ``dtype``, differentiable), n, M (list of K ints), r and pc = max(p, pred_min)
    (B, h, w; None when n == 0), ts (the sampled target, fp32) and valid (B, h, w bool)"""
    B, _, h, w = pred.shape
    p = pred[:, 0].to(dtype)
    ts = sample(target, h, w)
    valid = torch.isfinite(ts) & (ts > f32(valid_min)) & (ts <= f32(valid_max))  # (decided in fp32, as the kernels)
    n = int(valid.sum())
    zero = p.sum() * 0.0
    sw = 0.0 if silog_weight is None else silog_weight
    gw = 0.0 if grad_weight is None else grad_weight
    K = grad_scales
    if n == 0:
        return dict(total=zero, berhu=zero, D=zero, L_gm=zero, n=0, M=[0] * K, r=None, valid=valid, pc=None, ts=ts)
    t = torch.where(valid, ts, torch.ones_like(ts)).to(dtype)
    # berHu (c is a constant in backward)
    d = (p[valid] - t[valid]).abs()
    c = 0.2 * d.max().detach()
    berhu = torch.where(d <= c, d, (d * d + c * c) / (2 * c)).mean() if float(c) > 0 else d.mean()
    # residual: a clamped pixel (p <= pred_min) is a constant
    pm = torch.tensor(f32(pred_min), dtype=dtype)
    pc = torch.where(p > pm, p, pm)
    r = torch.log(pc) - torch.log(t)
    rv = r[valid]
    D = (rv * rv).mean() - silog_lambda * rv.mean() ** 2
    L, M = zero, []
    for k in range(K):
        s = 2 ** k
        rk, vk = r[:, ::s, ::s], valid[:, ::s, ::s]  # the grid G_k: its neighbours at stride s are its own
        M.append(int(vk.sum()))
        if M[-1] == 0:
            continue
        Sk = ((rk[:, :, 1:] - rk[:, :, :-1]).abs() * (vk[:, :, 1:] & vk[:, :, :-1])).sum()
        Sk = Sk + ((rk[:, 1:, :] - rk[:, :-1, :]).abs() * (vk[:, 1:, :] & vk[:, :-1, :])).sum()
        L = L + Sk / M[-1]
    total = berhu_weight * berhu + sw * D + gw * L
    return dict(total=total, berhu=berhu, D=D, L_gm=L, n=n, M=M, r=r.detach(), valid=valid, pc=pc.detach(), ts=ts)


def ill_conditioned(ref, K, band=SIGN_BAND):
    """(B, h, w) bool from the dict of ``criterion``: the pixels that touch a neighbour pair (both valid, at one of
    the K strides, on its grid) whose |r_i - r_j| is below ``band`` in float64 - the sign of such a difference is
    decided by the fp32 rounding of r.  A pair whose two INPUTS are the same bits - the same clamped prediction against
    the same sampled target, as neighbours under a smaller target or bf16 storage often are - is not such a pair: its
    two residuals are one fp32 number whatever logf's rounding, and sign(0) = 0 is exact; it stays in the comparison."""
    r, valid, pc, ts = ref["r"], ref["valid"], ref["pc"], ref["ts"]
    out = torch.zeros_like(valid)

    def mark(ok, a, b):
        """a, b: slices (of every map alike) that select the two ends of each pair"""
        close = ((rk[a] - rk[b]).abs() < band) & vk[a] & vk[b] & ~((pk[a] == pk[b]) & (tk[a] == tk[b]))
        ok[a] |= close
        ok[b] |= close

    for k in range(K):
        s = 2 ** k
        rk, vk, pk, tk, ok = (m[:, ::s, ::s] for m in (r, valid, pc, ts, out))  # (ok: a view, written through)
        lo, hi, all_ = slice(None, -1), slice(1, None), slice(None)
        mark(ok, (all_, all_, hi), (all_, all_, lo))
        mark(ok, (all_, hi, all_), (all_, lo, all_))
    return out


def loss_and_grad(pred, target, upstream=1.0, dtype=torch.float64, **kw):
    """-> (the dict of ``criterion``, d(upstream * total)/dpred as (B, 1, h, w) ``dtype``)"""
    p = pred.to(dtype).clone().requires_grad_(True)
    out = criterion(p, target, dtype=dtype, **kw)
    (out["total"] * upstream).backward()
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}, p.grad
