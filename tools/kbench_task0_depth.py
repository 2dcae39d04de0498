"""The decoder-only (task0) DEPTH step on the MI355X at BASELINE config 5's shape - batch 8, 480 x 640 targets, the
depth480 decoder with its three auxiliary heads (aux_weight 0.15) - for BerHuLoss(0.0) and BerHuLoss(0.0,
full_size=True), fp32 and bf16 storage, all in ONE process:

  task0_indexed   engine.graphed.GraphedTask0Step(depth_crit=): the berHu kernels read the full-size maps of the cache
                  in place through the step's row index (nasseg_berhu_*_rows_*) - what train_task0 replays;
  task0_gathered  the same step with the batch's maps gathered first (F.gather_rows of cache["depth"], 9.8 MB per
                  step) and the un-indexed loss: the A/B of the indexed kernels;
  end_to_end      engine.graphed.GraphedSegmenterStep(depth_crit=) on the images themselves: the stage a depth
                  candidate was trained by alone before.

Per line: images/s from the median of five alternating runs of KBENCH_STEPS (20) replayed steps each, every run's
ms per step, each side's min-max spread, and ``calls``: nasseg entry-point calls of one host-launched forward + loss +
backward of the two task0 forms.

usage (GPU box): python tools/kbench_task0_depth.py [fp32|bf16|both]   One JSON line per crit mode and dtype.
(tools/gpu.sh kbench OUT kbench_task0_depth.py keeps the table in OUT's log directory.)"""
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
from nas_segm_amd._lib import lib  # noqa: E402

DEV = "cuda:0"
B, H, W = 8, 480, 640
N_CACHE = 32
AUX_WEIGHT = 0.15
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
STEPS = int(os.environ.get("KBENCH_STEPS", "20"))


def emit(**kw):
    print(json.dumps(kw), flush=True)


def build():
    import bench
    from nas_segm_amd.engine import RankParallel, Segmenter
    from nas_segm_amd.nn.encoders import mbv2
    from nas_segm_amd.nn.micro_decoders import MicroDecoder

    torch.manual_seed(0)
    enc = mbv2(pretrained=False)
    dec = MicroDecoder(list(enc.out_sizes), 1, bench.WORKLOADS["depth480"][1], agg_size=64, repeats=2, aux_cell=True)
    return RankParallel(Segmenter(enc, dec).to(DEV))


def samples(dtype):
    """N_CACHE single samples: depth in (0, 10) with 10 % holes (0)"""
    g = torch.Generator().manual_seed(0)
    out = []
    for _ in range(N_CACHE):
        gt = 1e-3 + 10 * torch.rand(1, H, W, generator=g)
        gt[torch.rand(1, H, W, generator=g) < 0.1] = 0.0
        out.append({"image": torch.randn(1, 3, H, W, generator=g).to(dtype), "mask": gt})
    return out


def gathered_loss(cache, index, decoder, crit, aux_weight):
    """trainer_common.task0_depth_loss with the batch's maps gathered into a copy and the un-indexed loss"""
    from nas_segm_amd.engine.trainer_common import _heads, cache_feature_keys

    feats = [F.gather_rows(cache[k], index) for k in cache_feature_keys(cache)]
    target = F.gather_rows(cache["depth"], index)
    output, aux_outs = _heads(decoder(feats))
    loss = crit(output, target)
    for aux_out in aux_outs:
        loss = loss + crit(aux_out, target) * aux_weight
    return loss


def calls_of(fn):
    """nasseg entry-point calls of one ``fn()``"""
    count = [0]
    real = lib.call

    def counting(name, *args):
        count[0] += 1
        return real(name, *args)

    lib.call = counting
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        del lib.call  # (back to the class's method)
    return count[0]


def run(name, full_size):
    from nas_segm_amd.engine import graphed
    from nas_segm_amd.engine.trainer import populate_task0
    from nas_segm_amd.engine.trainer_common import task0_depth_loss
    from nas_segm_amd.nn import BerHuLoss

    dtype = DTYPES[name]
    crit = BerHuLoss(0.0, full_size=full_size)
    segmenter = build()
    net = segmenter.module
    data = samples(dtype)
    cache = populate_task0.__wrapped__(segmenter, data, None, N_CACHE, task="depth")
    segmenter.train()
    oe = torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-5)
    od = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
    image = torch.cat([s["image"] for s in data[:B]]).to(DEV).contiguous(memory_format=torch.channels_last)
    gt = torch.cat([s["mask"] for s in data[:B]]).to(DEV)
    index = torch.randperm(N_CACHE, generator=torch.Generator().manual_seed(1))[:B].to(DEV)
    params = list(net.decoder.parameters())

    def host(loss_fn):
        for p in params:
            p.grad = None
        loss_fn(cache, index, net.decoder, crit, AUX_WEIGHT).backward()

    calls = {"task0_indexed": calls_of(lambda: host(task0_depth_loss)),
             "task0_gathered": calls_of(lambda: host(gathered_loss))}

    class Gathered(graphed.GraphedTask0Step):
        def _forward_loss(self):
            return gathered_loss(self.cache, self.index, self.decoder, self.depth_crit, self.aux_weight)

    steppers = {
        "task0_indexed": graphed.GraphedTask0Step(cache, segmenter, od, B, 255, 3.0, AUX_WEIGHT, depth_crit=crit),
        "task0_gathered": Gathered(cache, segmenter, od, B, 255, 3.0, AUX_WEIGHT, depth_crit=crit),
        "end_to_end": graphed.GraphedSegmenterStep(segmenter, image, gt, oe, od, 255, 3.0, 3.0, AUX_WEIGHT,
                                                   depth_crit=crit),
    }
    host_index = index.cpu()
    step = {kind: ((lambda s=s: s.step(image, gt)) if kind == "end_to_end" else (lambda s=s: s.step(host_index)))
            for kind, s in steppers.items()}

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / STEPS

    runs = {kind: [] for kind in step}
    for _ in range(5):  # (alternating: drift of the box hits every side alike)
        for kind, fn in step.items():
            runs[kind].append(timed(fn))
    med = {kind: statistics.median(v) for kind, v in runs.items()}
    emit(bench="task0_depth", dtype=name, crit="berhu_up" if full_size else "berhu", batch=B, target=[H, W],
         cache_rows=N_CACHE, aux_weight=AUX_WEIGHT, steps_per_run=STEPS, runs=5,
         images_per_s={kind: round(1e3 * B / v, 1) for kind, v in med.items()},
         median_ms={kind: round(v, 3) for kind, v in med.items()},
         spread_ms={kind: round(max(v) - min(v), 3) for kind, v in runs.items()},
         ms={kind: [round(x, 3) for x in v] for kind, v in runs.items()}, calls=calls,
         indexed_over_gathered=round(med["task0_indexed"] / med["task0_gathered"], 4),
         layouts={kind: s.layout.get("mode") if isinstance(s.layout, dict) else None for kind, s in steppers.items()})
    del steppers, step, segmenter, net, cache
    torch.cuda.empty_cache()


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    for name in (["fp32", "bf16"] if which == "both" else [which]):
        for full_size in (False, True):
            run(name, full_size)


if __name__ == "__main__":
    main()
