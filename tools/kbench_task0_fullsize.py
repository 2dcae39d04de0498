"""The decoder-only (task0) step on FULL-SIZE labels on the MI355X at bench.py's ``task0`` workload shape - CVPR arch0,
21 classes, batch 64, 256 x 256, aux_weight 0.15, a cache of 16 batches - with nn.SegmCrossEntropy(full_size=True),
fp32 and bf16 storage, all in ONE process:

  task0_indexed   engine.graphed.GraphedTask0Step(segm_crit=): the full-size cross-entropy reads the labels of
                  cache["y_full"] in place through the step's row index (nasseg_ce_up_rows_*) - what train_task0
                  replays;
  task0_gathered  the same step with the batch's labels gathered first (F.gather_rows of cache["y_full"]) and the
                  un-indexed loss: the A/B of the indexed kernels;
  task0_plain     the replayed step with the plain softmax/NLL on cache["y"], the labels at the logits' size: the
                  step train_task0 ran before (less work per label pixel - reported, not a yardstick).

Per line: images/s from the median of five alternating runs of KBENCH_STEPS (20) replayed steps each, every run's
ms per step, each side's min-max spread, the bytes of cache["y_full"] and of one gathered batch of it, and ``calls``:
nasseg entry-point calls of one host-launched forward + loss + backward of the three forms.

usage (GPU box): python tools/kbench_task0_fullsize.py [fp32|bf16|both] [uint8|int64]   One JSON line per dtype.
(tools/gpu.sh kbench OUT kbench_task0_fullsize.py keeps the table in OUT's log directory.)"""
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
AUX_WEIGHT = 0.15
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
LABELS = {"uint8": torch.uint8, "int64": torch.int64}
STEPS = int(os.environ.get("KBENCH_STEPS", "20"))


def emit(**kw):
    print(json.dumps(kw), flush=True)


def samples(dtype, ldtype, batch, n_batches, classes, H, W):
    """the loader of bench.py's task0 workload, with a band of ignored pixels as its synthetic_batch has"""
    g = torch.Generator().manual_seed(100)
    out = []
    for _ in range(n_batches):
        mask = torch.randint(0, classes, (batch, H, W), generator=g)
        mask[:, H // 2: H // 2 + 5, :] = 255
        out.append({"image": torch.randn(batch, 3, H, W, generator=g).to(dtype), "mask": mask.to(ldtype)})
    return out


def gathered_loss(cache, index, decoder, crit, aux_weight):
    """trainer_common.task0_full_size_loss with the batch's labels gathered into a copy and the un-indexed loss"""
    from nas_segm_amd.engine.trainer_common import _heads, cache_feature_keys

    feats = [F.gather_rows(cache[k], index) for k in cache_feature_keys(cache)]
    target = F.gather_rows(cache["y_full"], index)
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


def run(name, label_name):
    import bench
    from nas_segm_amd.engine import graphed
    from nas_segm_amd.engine.trainer import populate_task0
    from nas_segm_amd.engine.trainer_common import task0_loss
    from nas_segm_amd.nn import SegmCrossEntropy

    dtype, ldtype = DTYPES[name], LABELS[label_name]
    _, _, classes, B, H, W = bench.WORKLOADS["task0"][:6]
    n_cache = 16 * B
    crit = SegmCrossEntropy(full_size=True).prepare(DEV)
    segmenter, net = bench.build_model(DEV, "task0")
    cache = populate_task0.__wrapped__(segmenter, samples(dtype, ldtype, B, n_cache // B, classes, H, W), None, n_cache,
                                       full_size_labels=True)
    segmenter.train()
    od = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
    index = torch.randperm(n_cache, generator=torch.Generator().manual_seed(1))[:B].to(DEV)
    params = list(net.decoder.parameters())

    def host(loss_fn):
        for p in params:
            p.grad = None
        loss_fn().backward()

    calls = {
        "task0_indexed": calls_of(lambda: host(lambda: task0_loss(cache, index, net.decoder, 255, AUX_WEIGHT,
                                                                  segm_crit=crit))),
        "task0_gathered": calls_of(lambda: host(lambda: gathered_loss(cache, index, net.decoder, crit, AUX_WEIGHT))),
        "task0_plain": calls_of(lambda: host(lambda: task0_loss(cache, index, net.decoder, 255, AUX_WEIGHT))),
    }

    class Gathered(graphed.GraphedTask0Step):
        def _forward_loss(self):
            return gathered_loss(self.cache, self.index, self.decoder, self.segm_crit, self.aux_weight)

    steppers = {
        "task0_indexed": graphed.GraphedTask0Step(cache, segmenter, od, B, 255, 3.0, AUX_WEIGHT, segm_crit=crit),
        "task0_gathered": Gathered(cache, segmenter, od, B, 255, 3.0, AUX_WEIGHT, segm_crit=crit),
        "task0_plain": graphed.GraphedTask0Step(cache, segmenter, od, B, 255, 3.0, AUX_WEIGHT),
    }
    host_index = index.cpu()
    step = {kind: (lambda s=s: s.step(host_index)) for kind, s in steppers.items()}

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
    y_full = cache["y_full"]
    emit(bench="task0_fullsize", dtype=name, labels=label_name, crit="ce_up", batch=B, size=[H, W],
         logits=list(cache["out_size"]), classes=classes, cache_rows=n_cache, aux_weight=AUX_WEIGHT,
         y_full_bytes=y_full.numel() * y_full.element_size(),
         gathered_bytes_per_step=B * H * W * y_full.element_size(), steps_per_run=STEPS, runs=5,
         images_per_s={kind: round(1e3 * B / v, 1) for kind, v in med.items()},
         median_ms={kind: round(v, 3) for kind, v in med.items()},
         spread_ms={kind: round(max(v) - min(v), 3) for kind, v in runs.items()},
         ms={kind: [round(x, 3) for x in v] for kind, v in runs.items()}, calls=calls,
         indexed_over_gathered=round(med["task0_indexed"] / med["task0_gathered"], 4),
         indexed_over_plain=round(med["task0_indexed"] / med["task0_plain"], 4),
         layouts={kind: s.layout.get("mode") if isinstance(s.layout, dict) else None for kind, s in steppers.items()})
    del steppers, step, segmenter, net, cache
    torch.cuda.empty_cache()


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    label_name = sys.argv[2] if len(sys.argv) > 2 else "uint8"
    for name in (["fp32", "bf16"] if which == "both" else [which]):
        run(name, label_name)


if __name__ == "__main__":
    main()
