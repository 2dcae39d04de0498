"""The decoder-only step with the reference's search defaults - distillation and Polyak averaging on
(src/utils/default_args.py:47-50: DO_KD, DO_POLYAK, KD_COEFF 0.3; src/main_search.py:455-458: kd_crit =
nn.MSELoss()) - against the step bench.py --workload task0 times, on bench.py's task0 shape: CVPR arch0 search
decoder (agg 48, aux cells), 256x256 crops, batch 64, a cache of 1024 samples, plus a synthetic fp32 kd_y of the
logits' shape.  Adam decoder, clip 3.0, aux 0.15, kd_coeff 0.3, Polyak decay 0.9.

  a  legacy           a plain-function MSE kd_crit (host launches, ATen MSE) + _polyak_update (2 launches per tensor)
  b  native, host     nn.MSELoss() fused into nasseg_ce_mse_* + nasseg_polyak, NASSEG_GRAPH=0
  c  native, replayed the same, the step replayed from a hipGraph (what train_task0 now does by itself)
  d  bench task0      no distillation, no Polyak, replayed: bench.py --workload task0

The variants alternate within each round (warm-up steps, then timed steps between device synchronisations); the
median of the rounds is reported, with GPU kernels per step counted by torch.profiler over one step.

usage (GPU box): python tools/kbench_task0_kd.py [--rounds 5] [--steps 20] [--warmup 3] [--only abcd]
One JSON line per variant, then a summary line, on stdout."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import nas_segm_amd  # noqa: E402,F401
from bench import WORKLOADS, build_model  # noqa: E402
from nas_segm_amd.engine import trainer  # noqa: E402

DEV = torch.device("cuda", 0)
KD_COEFF, DECAY, CLIP, AUX = 0.3, 0.9, 3.0, 0.15
NAMES = {"a": "legacy: function kd_crit + _polyak_update", "b": "native KD + Polyak, host-launched",
         "c": "native KD + Polyak, replayed", "d": "bench task0: no KD, no Polyak, replayed"}


def _mse(inp, tgt):
    return torch.nn.functional.mse_loss(inp, tgt)


def make_variants(only):
    batch, H, W = WORKLOADS["task0"][3:6]
    classes = WORKLOADS["task0"][2]
    segmenter, net = build_model(DEV, "task0")
    n_cache = 16 * batch
    g = torch.Generator().manual_seed(100)
    loader = [{"image": torch.randn(batch, 3, H, W, generator=g),
               "mask": torch.randint(0, classes, (batch, H, W), generator=g)} for _ in range(n_cache // batch)]
    Xy = trainer.populate_task0(segmenter, loader, None, n_cache, do_kd=False)
    assert not isinstance(Xy, int), "populate_task0 failed"
    del loader
    h, w = Xy["out_size"]
    kd_y = torch.randn((n_cache, classes, h, w), generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    Xy_kd = dict(Xy)
    Xy_kd["kd_y"] = kd_y
    segmenter.train()
    decoder = net.decoder
    avg = [p.data.clone() for p in decoder.parameters()]
    rng = np.random.RandomState(0)
    variants = {}
    env = os.environ.get("NASSEG_GRAPH")

    def optim():
        return torch.optim.Adam(decoder.parameters(), lr=3e-3, weight_decay=1e-5)

    def build(key, mode, cache, do_kd, crit, polyak):
        os.environ["NASSEG_GRAPH"] = mode
        step = trainer.make_task0_step(cache, segmenter, optim(), batch, 255, CLIP, AUX, False, do_kd, KD_COEFF, crit)
        replayed = getattr(step, "__self__", None) is not None

        def run():
            loss = step(rng.permutation(n_cache)[:batch])
            if polyak is not None:
                polyak()
            return loss

        variants[key] = (run, replayed)

    if "a" in only:
        build("a", "auto", Xy_kd, True, _mse, lambda: trainer._polyak_update(decoder.parameters(), avg, DECAY))
    if "b" in only:
        build("b", "0", Xy_kd, True, torch.nn.MSELoss(), lambda: trainer._polyak(decoder, avg, DECAY))
    if "c" in only:
        build("c", "1", Xy_kd, True, torch.nn.MSELoss(), lambda: trainer._polyak(decoder, avg, DECAY))
    if "d" in only:
        build("d", "auto", Xy, False, None, None)
    if env is None:
        os.environ.pop("NASSEG_GRAPH", None)
    else:
        os.environ["NASSEG_GRAPH"] = env
    return variants, batch


def kernels_per_step(run):
    """GPU kernels one step dispatches (torch.profiler's device activity; a replayed graph's kernels included)"""
    from torch.profiler import ProfilerActivity, profile

    run()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    n = 0
    for e in prof.events():
        if getattr(e, "device_type", None) == torch.autograd.DeviceType.CUDA:
            n += 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="abcd")
    ap.add_argument("--no-count", action="store_true", help="skip the kernel count (runs under rocprofv3)")
    args = ap.parse_args()
    variants, batch = make_variants(args.only)
    ips = dict((k, []) for k in variants)
    for r in range(args.rounds):
        for k, (run, _) in variants.items():
            for _ in range(args.warmup):
                run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                run()
            torch.cuda.synchronize()
            ips[k].append(batch * args.steps / (time.perf_counter() - t0))
    counts = {}
    if not args.no_count:
        for k, (run, _) in variants.items():
            counts[k] = kernels_per_step(run)
    med = {}
    for k, (run, replayed) in variants.items():
        med[k] = statistics.median(ips[k])
        print(json.dumps({"variant": k, "what": NAMES[k], "replayed": replayed, "images_per_s": round(med[k], 1),
                          "ms_per_step": round(1e3 * batch / med[k], 3),
                          "rounds": [round(v, 1) for v in ips[k]], "kernels_per_step": counts.get(k)}))
    summary = {"batch": batch, "rounds": args.rounds, "steps": args.steps}
    if "c" in med and "d" in med:
        summary["c_over_d"] = round(med["c"] / med["d"], 4)
    if "a" in med and "c" in med:
        summary["c_over_a"] = round(med["c"] / med["a"], 4)
    if "b" in med and "c" in med:
        summary["c_over_b"] = round(med["c"] / med["b"], 4)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
