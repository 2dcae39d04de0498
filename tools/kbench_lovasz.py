"""The Lovasz-Softmax term (csrc/lovasz.hip: nasseg_lovasz_fwd / _bwd) on the MI355X: alone, on top of the
cross-entropy, and beside the published composition in torch ops on the same box: logits of 4 x 19 x 256 x 512 (the
headline step's main head) and 16 x 21 x 81 x 81, fp32 and bf16, uint8 labels with 20 % ignored, 60 % of the valid
pixels confident.

  lovasz    the term alone (F.lovasz_softmax_loss's launches)
  combined  class weights, thresh = 0.7, min_kept = 100000, + 0.5 * Lovasz: the launches of the one autograd node
  ce        the same criterion without the term
  torch     the term as published: per class abs error, torch.sort, cumsum, jaccard[1:] -= jaccard[:-1], dot, autograd
            (written without a host synchronisation: invalid pixels carry error 0, absent classes are masked)

Device times of forward + backward: pairs recorded into a hipGraph and replayed (HIP events around the replays).
``x_ce``: combined / ce; ``x_torch``: lovasz / torch.  The yardstick is the torch composition.
``step``: images/s of the headline training step (bench.py's model and batch, engine.graphed.GraphedSegmenterStep)
with SegmCrossEntropy(lovasz_weight=0.5) beside the plain criterion, same process.
usage (GPU box): python tools/kbench_lovasz.py [small|cells|all|step]   One JSON line per measurement."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import nas_segm_amd  # noqa: E402,F401
from nas_segm_amd import functional as F  # noqa: E402
from nas_segm_amd._lib import current_stream, lib, ptr  # noqa: E402

DEV = "cuda:0"
SHAPES = {"small": (4, 19, 256, 512), "cells": (16, 21, 81, 81)}
SELECT = dict(thresh=0.7, min_kept=100000)
LW = 0.5


def emit(**kw):
    print(json.dumps(kw), flush=True)


def replayed_us(fn, n=5, reps=5):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
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


def torch_lovasz(logits, labels):
    """lovasz_softmax_flat over the present classes, valid pixels only, without a host synchronisation"""
    C = logits.shape[1]
    valid = (labels != 255).reshape(-1)
    probas = torch.softmax(logits.float(), 1).permute(0, 2, 3, 1).reshape(-1, C)
    lab = labels.reshape(-1).long()
    total = probas.new_zeros(())
    present = probas.new_zeros(())
    for c in range(C):
        fg = ((lab == c) & valid).float()
        errors = torch.where(valid, (fg - probas[:, c]).abs(), torch.zeros_like(fg))
        errors_sorted, perm = torch.sort(errors, 0, descending=True)
        gt = fg[perm]
        gts = gt.sum()
        inter = gts - gt.cumsum(0)
        union = gts + (1.0 - gt).cumsum(0)
        jac = 1.0 - inter / union
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        here = (gts > 0).float()
        total = total + here * torch.dot(errors_sorted, jac)
        present = present + here
    return total / present.clamp(min=1.0)


def run(name, dtype):
    shape = SHAPES[name]
    B, C, H, W = shape
    P = B * H * W
    logits, labels, w = inputs(shape, dtype)
    d = torch.empty_like(logits)
    s = current_stream
    sel = F._select_config("kbench_lovasz", SELECT["thresh"], SELECT["min_kept"], 0.0)
    base, loss, llov = (torch.empty((), device=DEV) for _ in range(3))
    stats, counts = torch.empty(2, device=DEV), torch.empty(3, dtype=torch.int64, device=DEV)
    pl = torch.empty(P, device=DEV)
    errors, coef = torch.empty(P, C, device=DEV), torch.empty(P, C, device=DEV)
    ncls = torch.empty(C + 1, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.query("nasseg_lovasz_workspace", P, C), device=DEV)
    ws_sel = torch.empty(lib.query("nasseg_ce_sel_workspace"), device=DEV)
    k = lambda op: F._k(op, logits)  # noqa: E731

    def ce_pair():
        lib.call(k("nasseg_ce_sel_fwd"), ptr(logits), ptr(labels), 1, ptr(w), P, C, 255, *sel, ptr(base), ptr(stats),
                 ptr(counts), ptr(pl), ptr(ws_sel), s())
        lib.call(k("nasseg_ce_sel_bwd"), ptr(logits), ptr(labels), 1, ptr(w), ptr(pl), ptr(stats), None, P, C, 255,
                 ptr(d), s())

    def lovasz_fwd(on_base):
        lib.call(k("nasseg_lovasz_fwd"), ptr(logits), ptr(labels), 1, P, C, 255, 0, LW if on_base else 1.0,
                 ptr(base) if on_base else None, ptr(loss), ptr(llov), ptr(errors), ptr(coef), None, ptr(ncls), ptr(ws),
                 s())

    def lovasz_bwd(on_base):
        lib.call(k("nasseg_lovasz_bwd"), ptr(logits), ptr(labels), 1, ptr(coef), None, LW if on_base else 1.0,
                 int(on_base), P, C, 255, ptr(d), s())

    def lovasz_pair():
        lovasz_fwd(False)
        lovasz_bwd(False)

    def combined_pair():
        lib.call(k("nasseg_ce_sel_fwd"), ptr(logits), ptr(labels), 1, ptr(w), P, C, 255, *sel, ptr(base), ptr(stats),
                 ptr(counts), ptr(pl), ptr(ws_sel), s())
        lovasz_fwd(True)
        lib.call(k("nasseg_ce_sel_bwd"), ptr(logits), ptr(labels), 1, ptr(w), ptr(pl), ptr(stats), None, P, C, 255,
                 ptr(d), s())
        lovasz_bwd(True)

    leaf = logits.detach().requires_grad_(True)

    def torch_pair():
        torch.autograd.grad(torch_lovasz(leaf, labels), leaf)

    # alternate twice and keep the smaller time of each: other work shares the box
    t_comb, t_ce, t_lov, t_fwd = [], [], [], []
    for _ in range(2):
        t_comb.append(replayed_us(combined_pair))
        t_ce.append(replayed_us(ce_pair))
        t_lov.append(replayed_us(lovasz_pair))
        t_fwd.append(replayed_us(lambda: lovasz_fwd(False)))
    lovasz_pair()
    torch.cuda.synchronize()
    mine = float(llov)
    t_torch = replayed_us(torch_pair, n=2, reps=3)
    theirs = float(torch_lovasz(leaf.detach(), labels))
    comb, ce, lov = min(t_comb), min(t_ce), min(t_lov)
    emit(shape=list(shape), dtype=str(dtype).split(".")[-1], lovasz_us=round(lov, 1), lovasz_fwd_us=round(min(t_fwd), 1),
         combined_us=round(comb, 1), ce_us=round(ce, 1), torch_us=round(t_torch, 1), x_ce=round(comb / ce, 3),
         x_torch=round(lov / t_torch, 3), spread=[round(max(v) / min(v), 3) for v in (t_comb, t_ce, t_lov)],
         loss_lovasz=round(mine, 6), loss_lovasz_torch=round(theirs, 6),
         workspace_mb=round(4 * lib.query("nasseg_lovasz_workspace", P, C) / 2 ** 20, 1))


def step(steps=20, warmup=5):
    import bench
    from nas_segm_amd.engine.graphed import GraphedSegmenterStep
    from nas_segm_amd.nn import SegmCrossEntropy

    wl = bench.WORKLOADS["headline"]
    image, mask = bench.synthetic_batch(wl[3], wl[4], wl[5], 0, DEV, wl[2])
    for name, crit in (("plain", None), ("lovasz_weight=0.5", SegmCrossEntropy(lovasz_weight=LW)),
                       ("plain again", None)):
        segmenter, net = bench.build_model(DEV, "headline")
        segmenter.train()
        oe = torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-5)
        od = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
        extra = {} if crit is None else {"segm_crit": crit.prepare(DEV)}
        graphed = GraphedSegmenterStep(segmenter, image, mask, oe, od, 255, 3.0, 3.0, -1, capture_optimisers=True,
                                       **extra)
        for _ in range(warmup):
            loss = graphed.step(image, mask)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = graphed.step(image, mask)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lay = graphed.layout or {}
        emit(step="headline {}x3x{}x{}".format(wl[3], wl[4], wl[5]), criterion=name,
             images_per_sec=round(wl[3] * steps / dt, 2), ms_per_step=round(1e3 * dt / steps, 3), loss=float(loss),
             lanes=lay.get("lanes"), steps=steps, warmup=warmup)
        del graphed, segmenter, net, oe, od
        torch.cuda.empty_cache()


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what == "step":
        return step()
    for name in (SHAPES if what == "all" else [what]):
        for dtype in (torch.float32, torch.bfloat16):
            run(name, dtype)


if __name__ == "__main__":
    main()
