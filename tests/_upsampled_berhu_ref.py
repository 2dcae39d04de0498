"""Torch-CPU restatement of the full-size berHu (F.berhu_loss_upsampled; definition: include/nasseg.h, "Full-size
berHu"): TF.interpolate(mode="bilinear", align_corners=False) of the prediction to the target's size, the validity
mask, c = 0.2 max d detached, the mean over the valid target pixels.  Used through autograd, in fp32 and float64, by
tests/test_upsampled_berhu_host.py (no GPU) and tests/test_hip_upsampled_berhu.py."""
import torch
import torch.nn.functional as TF

# (B, h, w, H, W): the smallest shapes at which each part of the kernels can go wrong
CASES = [
    (2, 5, 7, 19, 26),       # ragged up-sampling
    (1, 8, 16, 32, 64),      # integer x4
    (1, 3, 4, 96, 128),      # x32: the split footprint, and a map thinner than a tile
    (1, 9, 11, 4, 5),        # down-sampling
    (1, 1, 1, 7, 9),         # one prediction pixel
    (2, 6, 5, 6, 5),         # equal sizes
    (1, 1, 6, 5, 23),        # one row, mixed up and down
    (3, 17, 23, 101, 75),    # several tiles with ragged edges, several images
    (2, 33, 47, 130, 187),   # halos on all sides
]
SPARSE_CASES = [(3, 17, 23, 101, 75), (1, 3, 4, 96, 128)]
SPARSE_VALID = {(3, 17, 23, 101, 75): 1042, (1, 3, 4, 96, 128): 533}  # valid pixels sparse_target leaves

# the GPU tests' tolerances (test_masked_berhu_against_torch_autograd's): the loss within LOSS_RTOL * max(1, |ref|),
# the gradient of loss * GRAD_SCALE within GRAD_ATOL + GRAD_RTOL * |ref|
LOSS_RTOL, GRAD_ATOL, GRAD_RTOL, GRAD_SCALE = 1e-5, 1e-7, 1e-4, 1.3
MIN_GAP = 1e-5  # no valid pixel may have |v - t| below it: sign(v - t) is then the same in any fp32 evaluation


def make_inputs(B, h, w, H, W, seed=7):
    """the recipe of tests/test_hip_depth.py: pred in [0.3, 10), gt in [0, 10) with 10 % holes (0), every 997th
    pixel NaN and every 1013th (from 5) +inf"""
    g = torch.Generator().manual_seed(seed)
    pred = 0.3 + 9.7 * torch.rand(B, 1, h, w, generator=g)
    gt = 10 * torch.rand(B, H, W, generator=g)
    gt[torch.rand(B, H, W, generator=g) < 0.1] = 0.0
    flat = gt.view(-1)
    flat[::997] = float("nan")
    flat[5::1013] = float("inf")
    return pred, gt


def sparse_target(gt, seed=11):
    """95 % of the pixels of ``gt`` (holes or not) set to 0: a LiDAR-style map"""
    g = torch.Generator().manual_seed(seed)
    out = gt.clone()
    out[torch.rand(gt.shape, generator=g) >= 0.05] = 0.0
    return out


def valid_mask(gt, valid_min=0.0, valid_max=float("inf")):
    return torch.isfinite(gt) & (gt > valid_min) & (gt <= valid_max)


def upsampled(pred, size):
    """(B, H, W): the prediction (B, 1, h, w) at the target's size, in the prediction's dtype"""
    return TF.interpolate(pred, size=tuple(size), mode="bilinear", align_corners=False)[:, 0]


def berhu_upsampled(pred, gt, valid_min=0.0, valid_max=float("inf")):
    """-> (loss (differentiable in pred), c, v (B, H, W) detached, valid (B, H, W)); pred float32 or float64, the
    arithmetic in its dtype"""
    v = upsampled(pred, gt.shape[1:])
    valid = valid_mask(gt, valid_min, valid_max)
    if not bool(valid.any()):
        return pred.sum() * 0.0, 0.0, v.detach(), valid
    d = (v[valid] - gt.to(pred.dtype)[valid]).abs()
    c = 0.2 * d.max().detach()
    loss = torch.where(d <= c, d, (d * d + c * c) / (2 * c)).mean()
    return loss, float(c), v.detach(), valid


def loss_and_grad(pred, gt, valid_min=0.0, valid_max=float("inf"), dtype=torch.float32, scale=GRAD_SCALE):
    """-> dict(loss, grad of loss * scale (B, 1, h, w), c, v, valid, gap = the smallest |v - t| over valid pixels)"""
    p = pred.detach().to(dtype).clone().requires_grad_(True)
    loss, c, v, valid = berhu_upsampled(p, gt, valid_min, valid_max)
    (loss * scale).backward()
    gap = float((v[valid] - gt.to(dtype)[valid]).abs().min()) if bool(valid.any()) else float("inf")
    return dict(loss=float(loss.detach()), grad=p.grad.detach(), c=c, v=v, valid=valid, gap=gap)


_MEMO = {}


def reference(case, sparse=False, valid_max=float("inf"), bf16=False, dtype=torch.float32):
    """``loss_and_grad`` on the seed-7 inputs of ``case``, computed once per argument set and shared between the
    tests (nothing of the result may be modified).  ``bf16``: on the bf16-rounded prediction.  Adds pred and gt."""
    key = (tuple(case), sparse, valid_max, bf16, dtype)
    if key not in _MEMO:
        pred, gt = make_inputs(*case)
        if sparse:
            gt = sparse_target(gt)
        if bf16:
            pred = pred.to(torch.bfloat16).float()
        ref = loss_and_grad(pred, gt, 0.0, valid_max, dtype)
        ref.update(pred=pred, gt=gt)
        _MEMO[key] = ref
    return _MEMO[key]


def bf16_ulps(a, b):
    """largest distance between two bf16 tensors in units in the last place (+0 and -0 are the same number)"""
    def ordered(t):
        bits = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(bits < 0, -(bits & 0x7FFF), bits)

    return int((ordered(a) - ordered(b)).abs().max())
