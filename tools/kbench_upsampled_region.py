"""The full-size cross-entropy with the Dice term at the labels' size (csrc/loss_up.hip: nasseg_ce_up_region_fwd /
_bwd; F.cross_entropy_upsampled(region="dice")) on the MI355X beside
  composed   the only way to the same loss without it, from the project's own kernels on the same box:
             F.bilinear_resize of the logits to the labels' size, then F.cross_entropy_select(region="dice") there;
  ce_only    the fused cross-entropy alone (F.cross_entropy_upsampled without a region): what the term costs.

Logits 4 x 19 x 256 x 512 -> labels 1024 x 2048 (the headline step's main head) and 16 x 21 x 81 x 81 -> 321 x 321,
fp32 and bf16, class weights, OHEM (thresh = 0.7, min_kept = 100000); uint8 labels with 20 % ignored, 60 % of the
logits pixels confident (the inputs of tools/kbench_upsampled_ce.py).
``*_us``: device time of one forward + backward through autograd, recorded into a hipGraph and replayed (HIP events
around the replays); the three forms alternate five times: the MEDIAN of each, and ``spread`` = max / min of its five.
``fwd_us`` / ``bwd_us``: the fused pair's two entry points alone (medians).
``*_peak_mb``: growth of torch.cuda.max_memory_allocated over one host-launched forward + backward of each.

usage (GPU box): python tools/kbench_upsampled_region.py [headline|small]   One JSON line per measurement."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import nas_segm_amd  # noqa: E402,F401
from kbench_upsampled_ce import DEV, SELECT, SHAPES, emit, inputs, peak_mb, replayed_us  # noqa: E402
from nas_segm_amd import functional as F  # noqa: E402
from nas_segm_amd._lib import current_stream, lib, ptr  # noqa: E402

REGION = dict(region="dice", region_weight=0.5)
ROUNDS = 5


def run(lshape, tshape, dtype):
    B, C, h, w = lshape
    H, W = tshape
    logits, labels, wt = inputs(lshape, tshape, dtype)
    leaf = logits.detach().requires_grad_(True)

    def fused_pair():
        return torch.autograd.grad(F.cross_entropy_upsampled(leaf, labels, wt, **SELECT, **REGION), leaf)[0]

    def composed_pair():
        up = F.bilinear_resize(leaf, (H, W))
        return torch.autograd.grad(F.cross_entropy_select(up, labels, wt, **SELECT, **REGION), leaf)[0]

    def ce_only_pair():
        return torch.autograd.grad(F.cross_entropy_upsampled(leaf, labels, wt, **SELECT), leaf)[0]

    # the fused pair's two entry points alone
    sel = F._select_config("kbench_upsampled_region", SELECT["thresh"], SELECT["min_kept"], 0.0)
    alpha, beta, smooth, all_classes, rw = F._region_config("kbench_upsampled_region", "dice", 1.0, "present", 0.5)
    dims = (B, h, w, C, H, W)
    scal = [torch.empty((), device=DEV) for _ in range(3)]
    stats, counts = torch.empty(2, device=DEV), torch.empty(3, dtype=torch.int64, device=DEV)
    pl, lse, gdot = (torch.empty(B, H, W, device=DEV) for _ in range(3))
    coef, sums = torch.empty(2 * C, device=DEV), torch.empty(2 * C, device=DEV)
    ncls = torch.empty(C + 1, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.query("nasseg_ce_up_region_workspace", *dims), device=DEV)
    d = torch.empty_like(logits)
    k = lambda op: F._k(op, logits)  # noqa: E731

    def fwd():
        lib.call(k("nasseg_ce_up_region_fwd"), ptr(logits), ptr(labels), 1, ptr(wt), *dims, 255, 1, *sel, alpha, beta,
                 smooth, all_classes, rw, *[ptr(s) for s in scal], ptr(stats), ptr(counts), ptr(pl), ptr(lse),
                 ptr(coef), ptr(sums), ptr(ncls), ptr(gdot), ptr(ws), current_stream())

    def bwd():
        lib.call(k("nasseg_ce_up_region_bwd"), ptr(logits), ptr(labels), 1, ptr(wt), ptr(pl), ptr(lse), ptr(stats),
                 ptr(coef), ptr(gdot), None, 1, rw, *dims, 255, ptr(d), current_stream())

    fwd()
    forms = (("fused", fused_pair), ("composed", composed_pair), ("ce_only", ce_only_pair), ("fwd", fwd), ("bwd", bwd))
    times = {name: [] for name, _ in forms}
    for _ in range(ROUNDS):  # alternate: other work shares the box
        for name, fn in forms:
            times[name].append(replayed_us(fn))
    g_fused, g_comp = fused_pair().float(), composed_pair().float()
    l_fused = float(F.cross_entropy_upsampled(logits, labels, wt, **SELECT, **REGION))
    l_comp = float(F.cross_entropy_select(F.bilinear_resize(logits, (H, W)), labels, wt, **SELECT, **REGION))
    gdiff = float((g_fused - g_comp).abs().max() / g_comp.abs().max())
    del g_fused, g_comp
    peaks = {name: round(peak_mb(fn), 1) for name, fn in forms[:3]}
    med = {name: statistics.median(v) for name, v in times.items()}
    emit(logits=list(lshape), labels=list(tshape), dtype=str(dtype).split(".")[-1],
         fused_us=round(med["fused"], 1), composed_us=round(med["composed"], 1), ce_only_us=round(med["ce_only"], 1),
         x_composed=round(med["fused"] / med["composed"], 3), x_ce_only=round(med["fused"] / med["ce_only"], 3),
         fwd_us=round(med["fwd"], 1), bwd_us=round(med["bwd"], 1),
         spread={name: round(max(v) / min(v), 3) for name, v in times.items()},
         fused_peak_mb=peaks["fused"], composed_peak_mb=peaks["composed"], ce_only_peak_mb=peaks["ce_only"],
         loss=round(l_fused, 6), loss_composed=round(l_comp, 6), grad_diff_over_max=gdiff)


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    shapes = {"headline": SHAPES[:1], "small": SHAPES[1:]}.get(what, SHAPES)
    for lshape, tshape in shapes:
        for dtype in (torch.float32, torch.bfloat16):
            run(lshape, tshape, dtype)


if __name__ == "__main__":
    main()
