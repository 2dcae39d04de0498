"""The depth criterion with its scale-invariant log and gradient-matching terms (csrc/depth.hip:
nasseg_depth_terms_fwd / _bwd; F.depth_criterion) on the MI355X beside the same definition composed from torch ops on
the device (tests/_depth_terms_ref.py, in fp32 on the GPU: nearest sampling, masks, logs, slices, ``abs``, autograd).

  heads   forward + backward per head at the shapes of BASELINE config 5: predictions 8 x 1 x {120x160, 60x80, 30x40,
          15x20} (the main head and the x8 / x16 / x32 heads) against a 8 x 480 x 640 target with 20 % holes, fp32 and
          bf16, berhu_weight 1, silog_weight 1, grad_weight 0.5, 4 scales.
          ``native_us`` / ``torch_us``: device time of one forward + backward through autograd, recorded into a
          hipGraph and replayed (HIP events around the replays; alternated twice, the smaller time of each);
          ``berhu_us``: F.berhu_loss_masked alone, the same way - what the terms are added to; ``fwd_us`` / ``bwd_us``:
          the two new entry points alone; ``x``: native / torch; ``spread``: larger / smaller of the two alternations.
  step    ms per replayed training step at config 5's shape (bench.WORKLOADS["depth480"]'s network and batch,
          engine.graphed.GraphedSegmenterStep) with BerHuLoss(0.0) beside BerHuLoss(0.0, silog_weight=1.0,
          grad_weight=0.5): the one-head network bench.py times, and the same decoder with its three auxiliary heads
          (aux_weight 0.15) - five alternating runs each, the medians and each side's min-max spread; ``plain_calls``:
          the entry points the plain criterion launches for its loss, asserted to be nasseg_[bf16_]berhu_masked_fwd and
          _bwd, once each: what it launched before the terms' arguments existed.

usage (GPU box): python tools/kbench_depth_terms.py [heads|step] [fp32|bf16|both]   One JSON line per measurement."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import nas_segm_amd  # noqa: E402,F401
import _depth_terms_ref as R  # noqa: E402
from nas_segm_amd import functional as F  # noqa: E402
from nas_segm_amd._lib import current_stream, lib, ptr  # noqa: E402

DEV = "cuda:0"
B, H, W = 8, 480, 640
HEADS = ((120, 160), (60, 80), (30, 40), (15, 20))
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
STEPS = int(os.environ.get("KBENCH_STEPS", "20"))
TERMS = dict(berhu_weight=1.0, silog_weight=1.0, silog_lambda=0.5, grad_weight=0.5, grad_scales=4)


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


def inputs(h, w, dtype):
    pred, gt = R.make_inputs(B, h, w, H, W, seed=0)
    return pred.to(dtype).to(DEV), gt.to(DEV)


def torch_criterion(pred, gt):
    """the reference's definition in fp32 on the device, the masks' counts kept as tensors (the reference's
    ``int(valid.sum())`` reads the device, which a capture refuses)"""
    p = pred[:, 0].float()
    ts = R.sample(gt, p.shape[1], p.shape[2])
    valid = torch.isfinite(ts) & (ts > 0)
    t = torch.where(valid, ts, torch.ones_like(ts))
    n = valid.sum().clamp(min=1)
    d = (p - t).abs() * valid
    c = (0.2 * d.max().detach()).clamp(min=1e-30)
    berhu = (torch.where(d <= c, d, (d * d + c * c) / (2 * c)) * valid).sum() / n
    pm = torch.full_like(p, R.f32(1e-3))
    r = (torch.log(torch.where(p > pm, p, pm)) - torch.log(t)) * valid
    mean = r.sum() / n
    D = (r * r).sum() / n - TERMS["silog_lambda"] * mean * mean
    L = 0.0
    for k in range(TERMS["grad_scales"]):
        s = 2 ** k
        rk, vk = r[:, ::s, ::s], valid[:, ::s, ::s]
        Sk = ((rk[:, :, 1:] - rk[:, :, :-1]).abs() * (vk[:, :, 1:] & vk[:, :, :-1])).sum()
        Sk = Sk + ((rk[:, 1:, :] - rk[:, :-1, :]).abs() * (vk[:, 1:, :] & vk[:, :-1, :])).sum()
        L = L + Sk / vk.sum().clamp(min=1)
    return TERMS["berhu_weight"] * berhu + TERMS["silog_weight"] * D + TERMS["grad_weight"] * L


def run(h, w, name):
    pred, gt = inputs(h, w, DTYPES[name])
    leaf = pred.detach().requires_grad_(True)

    def native_pair():
        return torch.autograd.grad(F.depth_criterion(leaf, gt, **TERMS), leaf)[0]

    def torch_pair():
        return torch.autograd.grad(torch_criterion(leaf, gt), leaf)[0]

    def berhu_pair():
        return torch.autograd.grad(F.berhu_loss_masked(leaf, gt), leaf)[0]

    dims = (B, h, w, H, W, 0.0, float("inf"))
    conf = (R.f32(1e-3), 0.5, 4)
    berhu, out = torch.empty(3, device=DEV), torch.empty(16, device=DEV)
    resid = torch.empty(B, h, w, device=DEV)
    ws_b = torch.empty(lib.query("nasseg_berhu_masked_workspace"), device=DEV)
    ws = torch.empty(lib.query("nasseg_depth_terms_workspace"), device=DEV)
    d = torch.empty_like(pred)
    k = lambda op: F._k(op, pred)  # noqa: E731
    lib.call(k("nasseg_berhu_masked_fwd"), ptr(pred), ptr(gt), *dims, ptr(berhu), ptr(ws_b), current_stream())

    def fwd():
        lib.call(k("nasseg_depth_terms_fwd"), ptr(pred), ptr(gt), *dims, *conf, ptr(berhu), 1.0, 1.0, 0.5, ptr(resid),
                 ptr(out), ptr(ws), current_stream())

    def bwd():
        lib.call(k("nasseg_depth_terms_bwd"), ptr(pred), ptr(gt), ptr(resid), ptr(berhu), ptr(out), None, *dims, *conf,
                 1.0, 1.0, 0.5, ptr(d), current_stream())

    fwd()
    times = {key: [] for key in ("native", "torch", "berhu", "fwd", "bwd")}
    fns = {"native": native_pair, "torch": torch_pair, "berhu": berhu_pair, "fwd": fwd, "bwd": bwd}
    for _ in range(2):  # alternate twice and keep the smaller time of each: other work shares the box
        for key, fn in fns.items():
            times[key].append(replayed_us(fn))
    g_native, g_torch = native_pair().float(), torch_pair().float()
    l_native, l_torch = float(F.depth_criterion(pred, gt, **TERMS)), float(torch_criterion(pred, gt))
    best = {key: min(v) for key, v in times.items()}
    emit(pred=[B, 1, h, w], target=[B, H, W], dtype=name, native_us=round(best["native"], 1),
         torch_us=round(best["torch"], 1), x=round(best["native"] / best["torch"], 3),
         berhu_us=round(best["berhu"], 1), fwd_us=round(best["fwd"], 1), bwd_us=round(best["bwd"], 1),
         spread={key: round(max(v) / min(v), 3) for key, v in times.items()}, loss=round(l_native, 6),
         loss_torch=round(l_torch, 6), grad_diff_over_max=float((g_native - g_torch).abs().max() / g_torch.abs().max()))


def heads(names):
    for h, w in HEADS:
        for name in names:
            run(h, w, name)


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
        gt = inputs(1, 1, dtype)[1]
        for n_heads, aux_weight in ((1, -1), (4, 0.15)):
            segmenter = bench.build_model(DEV, "depth480")[0] if n_heads == 1 else four_heads()
            segmenter.train()
            net = segmenter.module
            oe = torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-5)
            od = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
            crits = {"plain": BerHuLoss(0.0), "terms": BerHuLoss(0.0, silog_weight=1.0, grad_weight=0.5)}
            # what the plain criterion launches for its loss
            seen, real = [], lib.call
            lib.call = lambda name_, *a: (seen.append(name_), real(name_, *a))[1]
            try:
                with torch.no_grad():
                    main, aux = segmenter(image)
                del seen[:]
                loss = crits["plain"](main.detach().requires_grad_(True), gt)
                loss.backward()
            finally:
                del lib.call
            plain_calls = sorted(set(seen))
            # ... which are the two entry points the criterion launched before it had the terms' arguments
            expected = sorted(F._k(n_, main) for n_ in ("nasseg_berhu_masked_fwd", "nasseg_berhu_masked_bwd"))
            assert plain_calls == expected and len(seen) == 2, (seen, expected)
            del main, aux, loss
            steppers = {kind: GraphedSegmenterStep(segmenter, image, gt, oe, od, 255, 3.0, 3.0, aux_weight,
                                                   depth_crit=crit) for kind, crit in crits.items()}

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
            emit(bench="step", dtype=name, heads=n_heads, aux_weight=aux_weight, steps_per_run=STEPS,
                 plain_ms=[round(v, 3) for v in runs["plain"]], terms_ms=[round(v, 3) for v in runs["terms"]],
                 plain_median_ms=round(med["plain"], 3), terms_median_ms=round(med["terms"], 3),
                 plain_spread_ms=round(spread["plain"], 3), terms_spread_ms=round(spread["terms"], 3),
                 median_difference_ms=round(med["terms"] - med["plain"], 3),
                 within_spread=bool(abs(med["terms"] - med["plain"]) <= max(spread.values())), plain_calls=plain_calls,
                 plain_calls_as_before=plain_calls == expected)
            del steppers, segmenter, net, oe, od
            torch.cuda.empty_cache()


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "heads"
    which = sys.argv[2] if len(sys.argv) > 2 else "both"
    names = ["fp32", "bf16"] if which == "both" else [which]
    {"heads": heads, "step": step}[what](names)


if __name__ == "__main__":
    main()
