"""The depth path (csrc/depth.hip, csrc/depth_eval.hip) on the MI355X at BASELINE config 5's shape: predictions
8 x 1 x 120 x 160, ground truth 8 x 480 x 640 with 10 % holes, fp32 and bf16 storage.

  metrics  us per F.depth_metrics call beside its traffic floor (the ground truth read once + the prediction).
  loss     us per forward + backward of F.berhu_loss_masked (480x640 target) beside F.berhu_loss (a target made at
           the prediction's size).
  step     ms per replayed training step of bench.WORKLOADS["depth480"] (one network, one process):
           GraphedSegmenterStep(loss_fn=F.berhu_loss) on a prediction-sized target against
           GraphedSegmenterStep(depth_crit=BerHuLoss()) on the 480x640 target with holes - five alternating runs
           each, the medians, each side's min-max spread and the difference of the medians.

Device times: 20 calls recorded into a hipGraph and replayed (HIP events around the replays) - and, beside them, the
same calls launched from the host, which is what bounds them there (KBENCH_ITERS calls, default 50); steps: wall clock
around KBENCH_STEPS (default 20) replays, synchronised.
usage (GPU box): python tools/kbench_depth.py [metrics|loss|step|all] [fp32|bf16|both]   One JSON line each.
(tools/gpu.sh kbench OUT kbench_depth.py keeps the table in OUT's log directory.)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
import nas_segm_amd  # noqa: E402,F401
from nas_segm_amd import functional as F  # noqa: E402
from nas_segm_amd.engine.graphed import GraphedSegmenterStep  # noqa: E402
from nas_segm_amd.nn import BerHuLoss  # noqa: E402

DEV = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "50"))
STEPS = int(os.environ.get("KBENCH_STEPS", "20"))
B, h, w, H, W = 8, 120, 160, 480, 640
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def emit(**kw):
    print(json.dumps(kw), flush=True)


def device_us(fn, n=ITERS, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n


def replayed_us(fn, n=20, reps=20):
    """device time of one ``fn()``: n calls recorded into a hipGraph, the replay timed (no host work between launches)"""
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
    return device_us(graph.replay, n=reps, warm=2) / n


def inputs(dtype):
    g = torch.Generator().manual_seed(0)
    pred = (0.3 + 9.7 * torch.rand(B, 1, h, w, generator=g)).to(DEV).to(dtype)
    gt = 10 * torch.rand(B, H, W, generator=g)
    gt[torch.rand(B, H, W, generator=g) < 0.1] = 0.0
    small = (10 * torch.rand(B, 1, h, w, generator=g)).to(DEV).to(dtype)
    return pred, gt.to(DEV), small


def metrics(names):
    for name in names:
        pred, gt, _ = inputs(DTYPES[name])
        acc = torch.zeros(12, dtype=torch.float64, device=DEV)
        call = lambda: F.depth_metrics(pred, gt, 1e-3, 10.0, acc=acc)  # noqa: E731
        host_us = device_us(call)
        us = replayed_us(call)
        nbytes = gt.numel() * 4 + pred.numel() * pred.element_size()
        emit(bench="metrics", dtype=name, replayed_us=round(us, 1), host_launched_us=round(host_us, 1), bytes=nbytes,
             floor_us=round(nbytes / bench.HBM_ACHIEVABLE_GBS * 1e-3, 2), gbs=round(nbytes / us * 1e-3, 1))


def loss(names):
    for name in names:
        pred, gt, small = inputs(DTYPES[name])
        pred.requires_grad_(True)

        def masked():
            pred.grad = None
            F.berhu_loss_masked(pred, gt).backward()

        def plain():
            pred.grad = None
            F.berhu_loss(pred, small).backward()

        emit(bench="loss", dtype=name, masked_fwd_bwd_us=round(replayed_us(masked), 1),
             unmasked_fwd_bwd_us=round(replayed_us(plain), 1),
             masked_host_launched_us=round(device_us(masked), 1), unmasked_host_launched_us=round(device_us(plain), 1))


def step(names):
    for name in names:
        dtype = DTYPES[name]
        segmenter, net = bench.build_model(DEV, "depth480")
        segmenter.train()
        oe = torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-5)
        od = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
        image, _ = bench.synthetic_batch(B, H, W, 0, DEV, 1)
        image = image.to(dtype)
        _, gt, _ = inputs(dtype)
        with torch.no_grad():  # (the unmasked loss wants a target of the prediction's own shape, as bench.py makes it)
            shape = segmenter(image)[0].shape
        small = (torch.rand(shape, device=DEV) * 10.0).to(dtype).contiguous(memory_format=torch.channels_last)
        plain = GraphedSegmenterStep(segmenter, image, small, oe, od, 255, 3.0, 3.0, -1, loss_fn=F.berhu_loss)
        masked = GraphedSegmenterStep(segmenter, image, gt, oe, od, 255, 3.0, 3.0, -1, depth_crit=BerHuLoss())

        def run(stepper, target):
            stepper.step(image, target)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                stepper.step(image, target)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / STEPS

        runs = {"unmasked": [], "masked": []}
        for _ in range(5):  # (alternating: drift of the box hits both sides alike)
            runs["unmasked"].append(run(plain, small))
            runs["masked"].append(run(masked, gt))
        med = {k: statistics.median(v) for k, v in runs.items()}
        spread = {k: max(v) - min(v) for k, v in runs.items()}
        emit(bench="step", dtype=name, steps_per_run=STEPS, prediction=list(shape[2:]),
             unmasked_ms=[round(v, 3) for v in runs["unmasked"]], masked_ms=[round(v, 3) for v in runs["masked"]],
             unmasked_median_ms=round(med["unmasked"], 3), masked_median_ms=round(med["masked"], 3),
             unmasked_spread_ms=round(spread["unmasked"], 3), masked_spread_ms=round(spread["masked"], 3),
             median_difference_ms=round(med["masked"] - med["unmasked"], 3),
             within_spread=bool(med["masked"] - med["unmasked"] <= max(spread.values())))
        del plain, masked, segmenter, net
        torch.cuda.empty_cache()


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    which = sys.argv[2] if len(sys.argv) > 2 else "both"
    names = ["fp32", "bf16"] if which == "both" else [which]
    table = {"metrics": metrics, "loss": loss, "step": step}
    for key in (table if what == "all" else [what]):
        table[key](names)


if __name__ == "__main__":
    main()
