"""The full-size berHu (csrc/depth.hip: nasseg_berhu_up_fwd / _bwd; F.berhu_loss_upsampled) on the MI355X beside the
composition it replaces, from the project's own kernels on the same box: F.bilinear_resize of the prediction to the
target's size, then F.berhu_loss_masked at equal sizes.

  cells   forward + backward of both at the heads of BASELINE config 5: predictions 8 x 1 x {120x160, 60x80, 30x40,
          15x20} against a 8 x 480 x 640 target, fp32 and bf16, the target with 10 % holes and once more with 5 % of
          its pixels valid.
          ``fused_us`` / ``composed_us``: device time of one forward + backward through autograd, recorded into a
          hipGraph and replayed (HIP events around the replays; alternated twice, the smaller time of each);
          ``fwd_us``: nasseg_berhu_up_fwd alone; ``bwd_us``: nasseg_berhu_up_bwd alone with the group size chosen from
          the shapes (``group``); ``bwd_group_us``: the same entry point at every group size - group 1 is one thread
          per prediction pixel; ``x``: fused / composed; ``fused_peak_mb`` / ``composed_peak_mb``: growth of
          torch.cuda.max_memory_allocated over one host-launched forward + backward of each.
  step    ms per replayed training step at config 5's shape (bench.WORKLOADS["depth480"]'s network and batch,
          engine.graphed.GraphedSegmenterStep) with BerHuLoss() beside BerHuLoss(full_size=True): the one-head network
          bench.py times, and the same decoder with its three auxiliary heads (aux_weight 0.15) - five alternating
          runs each, the medians and each side's min-max spread.

usage (GPU box): python tools/kbench_upsampled_berhu.py [cells|step] [fp32|bf16|both]   One JSON line per measurement.
(tools/gpu.sh kbench OUT kbench_upsampled_berhu.py keeps the table in OUT's log directory.)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import nas_segm_amd  # noqa: E402,F401
from nas_segm_amd import functional as F  # noqa: E402
from nas_segm_amd._lib import current_stream, lib, ptr  # noqa: E402

DEV = "cuda:0"
B, H, W = 8, 480, 640
HEADS = ((120, 160), (60, 80), (30, 40), (15, 20))
GROUPS = (1, 4, 16, 64, 256)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
STEPS = int(os.environ.get("KBENCH_STEPS", "20"))


def emit(**kw):
    print(json.dumps(kw), flush=True)


def replayed_us(fn, n=10, reps=10):
    """device time of one ``fn()``: n calls recorded into a hipGraph, ``reps`` replays timed by HIP events"""
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


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 2 ** 20


def inputs(h, w, dtype, valid_share):
    """pred in [0.3, 10), target in (0, 10) of which ``valid_share`` is kept (the rest: 0 = a hole)"""
    g = torch.Generator(device=DEV).manual_seed(0)
    pred = (0.3 + 9.7 * torch.rand(B, 1, h, w, device=DEV, generator=g)).to(dtype)
    gt = 1e-3 + 10 * torch.rand(B, H, W, device=DEV, generator=g)
    gt[torch.rand(B, H, W, device=DEV, generator=g) >= valid_share] = 0.0
    return pred, gt


def chosen_group(h, w):
    """the group size nasseg_berhu_up_bwd picks at group = 0 (csrc/depth.hip: up_bwd_group)"""
    fy = -(-2 * H // h) if H > h else (1 if H == h else 2)
    fx = -(-2 * W // w) if W > w else (1 if W == w else 2)
    group = 1
    while group < 256 and fy * fx > 16 * group:
        group *= 4
    return group


def run(h, w, name, valid_share):
    pred, gt = inputs(h, w, DTYPES[name], valid_share)
    leaf = pred.detach().requires_grad_(True)

    def fused_pair():
        return torch.autograd.grad(F.berhu_loss_upsampled(leaf, gt), leaf)[0]

    def composed_pair():
        up = F.bilinear_resize(leaf, (H, W))
        return torch.autograd.grad(F.berhu_loss_masked(up, gt), leaf)[0]

    # the fused pair's two entry points alone
    dims = (B, h, w, H, W, 0.0, float("inf"))
    out = torch.empty(3, device=DEV)
    ws = torch.empty(lib.query("nasseg_berhu_up_workspace", B, h, w, H, W), device=DEV)
    d = torch.empty_like(pred)
    k = lambda op: F._k(op, pred)  # noqa: E731

    def fwd():
        lib.call(k("nasseg_berhu_up_fwd"), ptr(pred), ptr(gt), *dims, ptr(out), ptr(ws), current_stream())

    def bwd(group=0):
        lib.call(k("nasseg_berhu_up_bwd"), ptr(pred), ptr(gt), ptr(out), None, *dims, group, ptr(d), current_stream())

    fwd()
    t_fused, t_comp, t_fwd, t_bwd = [], [], [], []
    t_group = {grp: [] for grp in GROUPS}
    for _ in range(2):  # alternate twice and keep the smaller time of each: other work shares the box
        t_fused.append(replayed_us(fused_pair))
        t_comp.append(replayed_us(composed_pair))
        t_fwd.append(replayed_us(fwd))
        t_bwd.append(replayed_us(bwd))
        for grp in GROUPS:
            t_group[grp].append(replayed_us(lambda: bwd(grp)))
    by_group = {grp: min(v) for grp, v in t_group.items()}
    g_fused, g_comp = fused_pair().float(), composed_pair().float()
    l_fused = float(F.berhu_loss_upsampled(pred, gt))
    l_comp = float(F.berhu_loss_masked(F.bilinear_resize(pred, (H, W)), gt))
    gdiff = float((g_fused - g_comp).abs().max() / g_comp.abs().max())
    del g_fused, g_comp
    m_fused, m_comp = peak_mb(fused_pair), peak_mb(composed_pair)
    fused, comp = min(t_fused), min(t_comp)
    emit(pred=[B, 1, h, w], target=[B, H, W], dtype=name, valid_share=valid_share, fused_us=round(fused, 1),
         composed_us=round(comp, 1), x=round(fused / comp, 3), fwd_us=round(min(t_fwd), 1),
         bwd_us=round(min(t_bwd), 1), bwd_group_us={str(grp): round(v, 1) for grp, v in by_group.items()},
         group=chosen_group(h, w), spread=[round(max(v) / min(v), 3) for v in (t_fused, t_comp)],
         fused_peak_mb=round(m_fused, 2), composed_peak_mb=round(m_comp, 2), loss=round(l_fused, 6),
         loss_composed=round(l_comp, 6), grad_diff_over_max=gdiff)


def cells(names):
    for h, w in HEADS:
        for name in names:
            for valid_share in (0.9, 0.05):
                run(h, w, name, valid_share)


def step(names):
    import bench
    from nas_segm_amd.engine import RankParallel, Segmenter
    from nas_segm_amd.engine.graphed import GraphedSegmenterStep
    from nas_segm_amd.nn import BerHuLoss
    from nas_segm_amd.nn.encoders import mbv2
    from nas_segm_amd.nn.micro_decoders import MicroDecoder

    def four_heads():
        torch.manual_seed(0)
        enc = mbv2(pretrained=False)
        dec = MicroDecoder(list(enc.out_sizes), 1, bench.WORKLOADS["depth480"][1], agg_size=64, repeats=2,
                           aux_cell=True)
        return RankParallel(Segmenter(enc, dec).to(DEV))

    for name in names:
        dtype = DTYPES[name]
        image, _ = bench.synthetic_batch(B, H, W, 0, DEV, 1)
        image = image.to(dtype)
        _, gt = inputs(1, 1, dtype, 0.9)
        for heads, aux_weight in ((1, -1), (4, 0.15)):
            segmenter = bench.build_model(DEV, "depth480")[0] if heads == 1 else four_heads()
            segmenter.train()
            net = segmenter.module
            oe = torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-5)
            od = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
            with torch.no_grad():
                main, aux = segmenter(image)
            sizes = [list(main.shape[2:])] + [list(a.shape[2:]) for a in (aux if aux_weight > 0 else [])]
            del main, aux
            steppers = {kind: GraphedSegmenterStep(segmenter, image, gt, oe, od, 255, 3.0, 3.0, aux_weight,
                                                   depth_crit=BerHuLoss(0.0, full_size=(kind == "full_size")))
                        for kind in ("nearest", "full_size")}

            def timed(stepper):
                stepper.step(image, gt)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(STEPS):
                    stepper.step(image, gt)
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0) / STEPS

            runs = {kind: [] for kind in steppers}
            for _ in range(5):  # (alternating: drift of the box hits both sides alike)
                for kind, stepper in steppers.items():
                    runs[kind].append(timed(stepper))
            med = {kind: statistics.median(v) for kind, v in runs.items()}
            spread = {kind: max(v) - min(v) for kind, v in runs.items()}
            emit(bench="step", dtype=name, heads=heads, aux_weight=aux_weight, head_sizes=sizes, steps_per_run=STEPS,
                 nearest_ms=[round(v, 3) for v in runs["nearest"]], full_size_ms=[round(v, 3) for v in runs["full_size"]],
                 nearest_median_ms=round(med["nearest"], 3), full_size_median_ms=round(med["full_size"], 3),
                 nearest_spread_ms=round(spread["nearest"], 3), full_size_spread_ms=round(spread["full_size"], 3),
                 median_difference_ms=round(med["full_size"] - med["nearest"], 3),
                 within_spread=bool(abs(med["full_size"] - med["nearest"]) <= max(spread.values())))
            del steppers, segmenter, net, oe, od
            torch.cuda.empty_cache()


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "cells"
    which = sys.argv[2] if len(sys.argv) > 2 else "both"
    names = ["fp32", "bf16"] if which == "both" else [which]
    {"cells": cells, "step": step}[what](names)


if __name__ == "__main__":
    main()
