"""The cross-entropy with a region-overlap term (csrc/loss.hip: nasseg_ce_region_fwd / _bwd) on the MI355X beside
the cross-entropy alone (nasseg_ce_sel_fwd / _bwd, unchanged entry points) and beside the region term composed from
torch ops, on the same box: logits of 4 x 19 x 256 x 512 and 16 x 21 x 81 x 81, fp32 and bf16, uint8 labels with 20 %
ignored, 60 % of the valid pixels confident.

  combined  class weights, thresh = 0.7, min_kept = 100000, + 0.5 * soft Jaccard (smooth = 1, present classes)
  ce        the same criterion without the region term
  region    the region term alone (F.region_overlap_loss's launches)
  torch     the region term as a user would write it: softmax, one_hot, three sums, the formula, autograd

Device times of forward + backward: 10 forward + backward pairs recorded into a hipGraph and replayed (HIP events
around the replays).  ``x_ce``: combined / ce; ``x_torch``: region / torch and, for what a user pays in all,
``combined_vs_ce_plus_torch``: combined / (ce + torch).
usage (GPU box): python tools/kbench_region_loss.py [small|cells|all]   One JSON line per shape and storage type."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import nas_segm_amd  # noqa: E402,F401
from nas_segm_amd import functional as F  # noqa: E402
from nas_segm_amd._lib import current_stream, lib, ptr  # noqa: E402

DEV = "cuda:0"
SHAPES = {"small": (4, 19, 256, 512), "cells": (16, 21, 81, 81)}
SELECT = dict(thresh=0.7, min_kept=100000)
REGION = dict(region="jaccard", region_weight=0.5, region_smooth=1.0, region_classes="present")


def emit(**kw):
    print(json.dumps(kw), flush=True)


def replayed_us(fn, n=10, reps=10):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(n):
            fn()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / (n * reps)


def inputs(shape, dtype):
    B, C, H, W = shape
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(B, H, W, C, device=DEV, generator=g)
    t = torch.randint(0, C, (B, H, W), device=DEV, generator=g)
    boost = torch.rand(B, H, W, device=DEV, generator=g) < 0.6
    x.scatter_add_(3, t[..., None], 6.0 * boost[..., None].float())
    t[torch.rand(B, H, W, device=DEV, generator=g) < 0.2] = 255
    return x.to(dtype).permute(0, 3, 1, 2), t.to(torch.uint8), torch.rand(C, device=DEV, generator=g) + 0.5


def torch_region(logits, labels, smooth=1.0):
    """soft Jaccard over the present classes, valid pixels only, without a host synchronisation"""
    C = logits.shape[1]
    valid = labels != 255
    q = torch.softmax(logits.float(), 1) * valid[:, None]
    y = torch.nn.functional.one_hot(torch.where(valid, labels, torch.zeros_like(labels)).long(), C)
    y = y.permute(0, 3, 1, 2) * valid[:, None]
    inter, s, n = (q * y).sum((0, 2, 3)), q.sum((0, 2, 3)), y.sum((0, 2, 3)).float()
    present = (n > 0).float()
    t = (inter + smooth) / (s + n - inter + smooth)
    return 1.0 - (t * present).sum() / present.sum().clamp(min=1.0)


def run(name, dtype):
    shape = SHAPES[name]
    B, C, H, W = shape
    P = B * H * W
    logits, labels, w = inputs(shape, dtype)
    d = torch.empty_like(logits)
    s = current_stream
    sel = F._select_config("kbench_region_loss", SELECT["thresh"], SELECT["min_kept"], 0.0)
    rcfg = F._region_config("kbench_region_loss", REGION["region"], REGION["region_smooth"], REGION["region_classes"],
                            REGION["region_weight"])
    loss, lce, lreg = (torch.empty((), device=DEV) for _ in range(3))
    stats, counts = torch.empty(2, device=DEV), torch.empty(3, dtype=torch.int64, device=DEV)
    pl = torch.empty(P, device=DEV)
    coef, sums = torch.empty(2 * C, device=DEV), torch.empty(2 * C, device=DEV)
    ncls = torch.empty(C + 1, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.query("nasseg_ce_region_workspace", C), device=DEV)
    ws_sel = torch.empty(lib.query("nasseg_ce_sel_workspace"), device=DEV)
    k = lambda op: F._k(op, logits)  # noqa: E731

    def region_pair(with_ce):
        cfg = sel if with_ce else (0, float("inf"), 0, 0.0)
        lib.call(k("nasseg_ce_region_fwd"), ptr(logits), ptr(labels), 1, ptr(w) if with_ce else None, P, C, 255,
                 int(with_ce), *cfg, *rcfg[:4], rcfg[4] if with_ce else 1.0, ptr(loss), ptr(lce), ptr(lreg),
                 ptr(stats), ptr(counts), ptr(pl), ptr(coef), ptr(sums), ptr(ncls), ptr(ws), s())
        lib.call(k("nasseg_ce_region_bwd"), ptr(logits), ptr(labels), 1, ptr(w) if with_ce else None, ptr(pl),
                 ptr(stats), ptr(coef), None, int(with_ce), rcfg[4] if with_ce else 1.0, P, C, 255, ptr(d), s())

    def ce_pair():
        lib.call(k("nasseg_ce_sel_fwd"), ptr(logits), ptr(labels), 1, ptr(w), P, C, 255, *sel, ptr(loss), ptr(stats),
                 ptr(counts), ptr(pl), ptr(ws_sel), s())
        lib.call(k("nasseg_ce_sel_bwd"), ptr(logits), ptr(labels), 1, ptr(w), ptr(pl), ptr(stats), None, P, C, 255,
                 ptr(d), s())

    leaf = logits.detach().requires_grad_(True)

    def torch_pair():
        torch.autograd.grad(torch_region(leaf, labels), leaf)

    # alternate the three twice and keep the smaller time of each: other work shares the box
    t_comb, t_ce, t_reg = [], [], []
    for _ in range(2):
        t_comb.append(replayed_us(lambda: region_pair(True)))
        t_ce.append(replayed_us(ce_pair))
        t_reg.append(replayed_us(lambda: region_pair(False)))
    torch.cuda.synchronize()
    mine = float(lreg)
    t_torch = replayed_us(torch_pair, n=3, reps=5)
    theirs = float(torch_region(leaf.detach(), labels))
    comb, ce, reg = min(t_comb), min(t_ce), min(t_reg)
    emit(shape=list(shape), dtype=str(dtype).split(".")[-1], combined_us=round(comb, 1), ce_us=round(ce, 1),
         region_us=round(reg, 1), torch_us=round(t_torch, 1), x_ce=round(comb / ce, 3),
         x_torch=round(reg / t_torch, 3), combined_vs_ce_plus_torch=round(comb / (ce + t_torch), 3),
         spread=[round(max(v) / min(v), 3) for v in (t_comb, t_ce, t_reg)], loss_region=round(mine, 6),
         loss_region_torch=round(theirs, 6), n_kept=int(counts[2]))


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    for name in (SHAPES if what == "all" else [what]):
        for dtype in (torch.float32, torch.bfloat16):
            run(name, dtype)


if __name__ == "__main__":
    main()
