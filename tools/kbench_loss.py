"""The class-weighted / hard-example-mined cross-entropy (csrc/loss.hip: nasseg_ce_sel_fwd / _bwd) on the MI355X
beside the plain loss (nasseg_ce_fwd / _bwd) on the same box: fp32 logits of 4 x 19 x 256 x 512, 4 x 19 x 1024 x 2048
and 16 x 21 x 81 x 81, uint8 labels with 20 % ignored, 60 % of the valid pixels confident (thresh = 0.7 splits the set).

  plain          nasseg_ce_fwd, nasseg_ce_bwd
  weights        class weights, no selection
  thresh         thresh = 0.7, min_kept = 100000 (the usual OHEM setting)
  keep_fraction  keep_fraction = 0.25, min_kept = 1 (top-k bootstrapping)

Device times: 10 calls recorded into a hipGraph and replayed (HIP events around the replays), forward and backward
apart; ``x_plain``: the ratio to the plain kernel's time; ``fwd_bytes`` / ``bwd_bytes``: what the launches must move
(logits, labels, pixel_loss written once and read by the three histogram passes and the sum pass; backward: logits in,
gradient out, labels, pixel_loss) and the GB/s that makes.
usage (GPU box): python tools/kbench_loss.py [small|large|cells|all]   One JSON line per shape and configuration."""
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
SHAPES = {"small": (4, 19, 256, 512), "large": (4, 19, 1024, 2048), "cells": (16, 21, 81, 81)}
CONFIGS = {"weights": dict(weights=True), "thresh": dict(thresh=0.7, min_kept=100000),
           "keep_fraction": dict(keep_fraction=0.25, min_kept=1)}


def emit(**kw):
    print(json.dumps(kw), flush=True)


def replayed_us(fn, n=10, reps=10):
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


def inputs(shape):
    B, C, H, W = shape
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(B, H, W, C, device=DEV, generator=g)
    t = torch.randint(0, C, (B, H, W), device=DEV, generator=g)
    boost = torch.rand(B, H, W, device=DEV, generator=g) < 0.6
    x.scatter_add_(3, t[..., None], 6.0 * boost[..., None].float())
    t[torch.rand(B, H, W, device=DEV, generator=g) < 0.2] = 255
    return x.permute(0, 3, 1, 2), t.to(torch.uint8), torch.rand(C, device=DEV, generator=g) + 0.5


def run(name):
    shape = SHAPES[name]
    B, C, H, W = shape
    P = B * H * W
    logits, labels, w = inputs(shape)
    d = torch.empty_like(logits)
    s = current_stream
    out = torch.empty(2, device=DEV)
    ws = torch.empty(lib.query("nasseg_ce_workspace"), device=DEV)
    plain_fwd = replayed_us(lambda: lib.call("nasseg_ce_fwd", ptr(logits), ptr(labels), 1, P, C, 255, ptr(out),
                                             ptr(ws), s()))
    plain_bwd = replayed_us(lambda: lib.call("nasseg_ce_bwd", ptr(logits), ptr(labels), 1, ptr(out), None, P, C, 255,
                                             ptr(d), s()))
    fwd_bytes, bwd_bytes = P * (4 * C + 1), P * (8 * C + 1)
    emit(shape=list(shape), config="plain", fwd_us=round(plain_fwd, 1), bwd_us=round(plain_bwd, 1),
         fwd_gbs=round(fwd_bytes / plain_fwd * 1e-3, 1), bwd_gbs=round(bwd_bytes / plain_bwd * 1e-3, 1))
    loss, stats = torch.empty((), device=DEV), torch.empty(2, device=DEV)
    counts = torch.empty(3, dtype=torch.int64, device=DEV)
    pl = torch.empty(P, device=DEV)
    ws = torch.empty(lib.query("nasseg_ce_sel_workspace"), device=DEV)
    for key, cfg in CONFIGS.items():
        cfg = dict(cfg)
        weight = w if cfg.pop("weights", False) else None
        sel = F._select_config("kbench_loss", cfg.get("thresh"), cfg.get("min_kept", 0), cfg.get("keep_fraction", 0.0))
        fwd = replayed_us(lambda: lib.call("nasseg_ce_sel_fwd", ptr(logits), ptr(labels), 1, ptr(weight), P, C, 255,
                                           *sel, ptr(loss), ptr(stats), ptr(counts), ptr(pl), ptr(ws), s()))
        bwd = replayed_us(lambda: lib.call("nasseg_ce_sel_bwd", ptr(logits), ptr(labels), 1, ptr(weight), ptr(pl),
                                           ptr(stats), None, P, C, 255, ptr(d), s()))
        torch.cuda.synchronize()
        passes = 5 if sel[0] else 2  # pixel_loss: written once; read by 3 histogram passes (selection) + the sum pass
        fb, bb = fwd_bytes + P * (4 * passes + 1), bwd_bytes + 4 * P
        emit(shape=list(shape), config=key, fwd_us=round(fwd, 1), bwd_us=round(bwd, 1),
             fwd_x_plain=round(fwd / plain_fwd, 3), bwd_x_plain=round(bwd / plain_bwd, 3),
             fwd_bytes_x_plain=round(fb / fwd_bytes, 3), fwd_gbs=round(fb / fwd * 1e-3, 1),
             bwd_gbs=round(bb / bwd * 1e-3, 1), counts=counts.tolist(), tau=round(float(stats[1]), 6),
             loss=round(float(loss), 6))


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    for name in (SHAPES if what == "all" else [what]):
        run(name)


if __name__ == "__main__":
    main()
