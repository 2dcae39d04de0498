"""The full-size cross-entropy (csrc/loss_up.hip: nasseg_ce_up_fwd / _bwd; F.cross_entropy_upsampled) on the MI355X
beside the composition it replaces, from the project's own kernels on the same box: F.bilinear_resize of the logits to
the labels' size, then F.cross_entropy_select there.

  cells   forward + backward of both, logits 4 x 19 x 256 x 512 -> labels 1024 x 2048 (the headline step's main head)
          and 16 x 21 x 81 x 81 -> 321 x 321, fp32 and bf16, class weights, with and without OHEM (thresh = 0.7,
          min_kept = 100000); uint8 labels with 20 % ignored, 60 % of the logits pixels confident.
          ``fused_us`` / ``composed_us``: device time of one forward + backward through autograd, recorded into a
          hipGraph and replayed (HIP events around the replays; alternated twice, the smaller time of each);
          ``fwd_us`` / ``bwd_us``: the two entry points of the fused pair alone; ``x``: fused / composed;
          ``fused_peak_mb`` / ``composed_peak_mb``: growth of torch.cuda.max_memory_allocated over one host-launched
          forward + backward of each.
  step    images/s of the headline training step (bench.py's model and batch, engine.graphed.GraphedSegmenterStep)
          with SegmCrossEntropy(full_size=True) beside the plain criterion, same process.

usage (GPU box): python tools/kbench_upsampled_ce.py [cells|step]   One JSON line per measurement."""
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
SHAPES = (((4, 19, 256, 512), (1024, 2048)), ((16, 21, 81, 81), (321, 321)))
SELECT = dict(thresh=0.7, min_kept=100000)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def replayed_us(fn, n=3, reps=5):
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


def inputs(lshape, tshape, dtype):
    """logits with 60 % of their pixels confident (+6 on a class of their own), labels that follow the nearest logits
    pixel's class except for 30 % drawn afresh, 20 % ignored"""
    B, C, h, w = lshape
    H, W = tshape
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(B, h, w, C, device=DEV, generator=g)
    tl = torch.randint(0, C, (B, h, w), device=DEV, generator=g)
    boost = torch.rand(B, h, w, device=DEV, generator=g) < 0.6
    x.scatter_add_(3, tl[..., None], 6.0 * boost[..., None].float())
    iy = (torch.arange(H, device=DEV) * h // H).clamp(max=h - 1)
    ix = (torch.arange(W, device=DEV) * w // W).clamp(max=w - 1)
    t = tl[:, iy][:, :, ix].contiguous()
    fresh = torch.rand(B, H, W, device=DEV, generator=g) < 0.3
    t = torch.where(fresh, torch.randint(0, C, (B, H, W), device=DEV, generator=g), t)
    t[torch.rand(B, H, W, device=DEV, generator=g) < 0.2] = 255
    logits = x.to(dtype).permute(0, 3, 1, 2)
    return logits, t.to(torch.uint8), torch.rand(C, device=DEV, generator=g) + 0.5


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 2 ** 20


def run(lshape, tshape, dtype, select):
    B, C, h, w = lshape
    H, W = tshape
    logits, labels, wt = inputs(lshape, tshape, dtype)
    cfg = SELECT if select else {}
    leaf = logits.detach().requires_grad_(True)

    def fused_pair():
        return torch.autograd.grad(F.cross_entropy_upsampled(leaf, labels, wt, **cfg), leaf)[0]

    def composed_pair():
        up = F.bilinear_resize(leaf, (H, W))
        return torch.autograd.grad(F.cross_entropy_select(up, labels, wt, **cfg), leaf)[0]

    # the fused pair's two entry points alone
    sel = F._select_config("kbench_upsampled_ce", cfg.get("thresh"), cfg.get("min_kept", 0), 0.0)
    dims = (B, h, w, C, H, W)
    loss, stats = torch.empty((), device=DEV), torch.empty(2, device=DEV)
    counts = torch.empty(3, dtype=torch.int64, device=DEV)
    pl, lse = torch.empty(B, H, W, device=DEV), torch.empty(B, H, W, device=DEV)
    ws = torch.empty(lib.query("nasseg_ce_up_workspace", *dims), device=DEV)
    d = torch.empty_like(logits)
    k = lambda op: F._k(op, logits)  # noqa: E731

    def fwd():
        lib.call(k("nasseg_ce_up_fwd"), ptr(logits), ptr(labels), 1, ptr(wt), *dims, 255, *sel, ptr(loss), ptr(stats),
                 ptr(counts), ptr(pl), ptr(lse), ptr(ws), current_stream())

    def bwd():
        lib.call(k("nasseg_ce_up_bwd"), ptr(logits), ptr(labels), 1, ptr(wt), ptr(pl), ptr(lse), ptr(stats), None,
                 *dims, 255, ptr(d), current_stream())

    fwd()
    t_fused, t_comp, t_fwd, t_bwd = [], [], [], []
    for _ in range(2):  # alternate twice and keep the smaller time of each: other work shares the box
        t_fused.append(replayed_us(fused_pair))
        t_comp.append(replayed_us(composed_pair))
        t_fwd.append(replayed_us(fwd))
        t_bwd.append(replayed_us(bwd))
    g_fused, g_comp = fused_pair().float(), composed_pair().float()
    l_fused = float(F.cross_entropy_upsampled(logits, labels, wt, **cfg))
    l_comp = float(F.cross_entropy_select(F.bilinear_resize(logits, (H, W)), labels, wt, **cfg))
    gdiff = float((g_fused - g_comp).abs().max() / g_comp.abs().max())
    del g_fused, g_comp
    m_fused, m_comp = peak_mb(fused_pair), peak_mb(composed_pair)
    fused, comp = min(t_fused), min(t_comp)
    emit(logits=list(lshape), labels=list(tshape), dtype=str(dtype).split(".")[-1], ohem=bool(select),
         fused_us=round(fused, 1), composed_us=round(comp, 1), x=round(fused / comp, 3), fwd_us=round(min(t_fwd), 1),
         bwd_us=round(min(t_bwd), 1), spread=[round(max(v) / min(v), 3) for v in (t_fused, t_comp)],
         fused_peak_mb=round(m_fused, 1), composed_peak_mb=round(m_comp, 1), loss=round(l_fused, 6),
         loss_composed=round(l_comp, 6), grad_diff_over_max=gdiff)


def step(steps=20, warmup=5):
    import bench
    from nas_segm_amd.engine.graphed import GraphedSegmenterStep
    from nas_segm_amd.nn import SegmCrossEntropy

    wl = bench.WORKLOADS["headline"]
    image, mask = bench.synthetic_batch(wl[3], wl[4], wl[5], 0, DEV, wl[2])
    for name, crit in (("plain", None), ("full_size=True", SegmCrossEntropy(full_size=True)), ("plain again", None)):
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
    what = sys.argv[1] if len(sys.argv) > 1 else "cells"
    if what == "step":
        return step()
    for lshape, tshape in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            for select in (False, True):
                run(lshape, tshape, dtype, select)


if __name__ == "__main__":
    main()
