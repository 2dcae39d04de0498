"""The device augmentation (csrc/augment.hip, data/device.py) on the MI355X:

  kernel   us per batch of nasseg_augment (device events, packed batch already on the device) for the WACV search
           training pipeline (ResizeScale(1024, 0.7, 1.4, longer) -> RandomMirror -> RandomCrop(321) -> Normalise,
           32 samples), its validation pipeline (resize to 1024 x 512, CentralCrop(512), 32 samples) and a
           4 x 2048 x 1024 full-size batch; fp32 and bf16.
  loader   images/s of create_loaders (host augmentation + the engine's copy / cast to the device) against
           create_device_loaders, WACV training pipeline, batch 32, 16 workers, on synthetic 2048 x 1024 PNGs written
           to a temporary directory.  The first batch (worker start-up) is not counted.

  --depth  the depth twins: us per batch of nasseg_augment_depth at 32 x 320 x 320 (DepthResizeScale(320, 0.7, 1.4)
           -> RandomMirror -> RandomCrop(320) on 640 x 480 sources; fp32 and bf16 image), and images/s of
           create_depth_loaders against create_device_depth_loaders on synthetic 640 x 480 RGB + 16-bit depth PNG
           pairs written to a temporary directory (batch 32, 16 workers, first batch not counted).

  --colour the ColourJitter launches (nasseg_augment_colour, with --depth nasseg_augment_depth_colour).  kernel: us per
           batch of the colour launch beside the plain launch ON THE SAME PACKED BATCH (WACV search training shape; the
           --depth shape), every sample jittered (matrix and table): 9 rounds alternating the two, 200 launches each,
           median and min / max over the rounds.  loader: the two loaders with args.colour_jitter set.

usage (GPU box): python tools/kbench_augment.py [kernel|loader|all] [--depth] [--colour]   (KBENCH_BATCHES: loader
batches, default 24).  One JSON line per measurement on stdout."""
import json
import os
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import nas_segm_amd  # noqa: E402,F401
from nas_segm_amd import functional as F  # noqa: E402
from nas_segm_amd.data import datasets as D  # noqa: E402
from nas_segm_amd.data import device as dev  # noqa: E402

DEV = "cuda:0"
MEAN = np.array([0.485, 0.456, 0.406]).reshape((1, 1, 3))
STD = np.array([0.229, 0.224, 0.225]).reshape((1, 1, 3))
NORM = (1.0 / 255, MEAN, STD)


def synthetic(rng, h=1024, w=2048):
    """a street-scene-like image: smooth gradients and blocks plus a little noise, and a label map of blocks"""
    yy, xx = np.mgrid[0:h, 0:w]
    img = 100 + 80 * np.sin(xx[:, :, None] / (90.0 + 17 * np.arange(3)) + yy[:, :, None] / 70.0 + rng.rand())
    img += rng.randint(-6, 7, img.shape)
    msk = ((xx // 128 + yy // 96 * 3 + rng.randint(19)) % 19).astype(np.uint8)
    return np.clip(img, 0, 255).astype(np.uint8), msk


def pipelines():
    trn = D.Compose([D.ResizeScale(1024, 0.7, 1.4, True), D.RandomMirror(), D.RandomCrop(321), D.Normalise(*NORM),
                     D.ToTensor()])
    val = D.Compose([D.ResizeScale(1024, 1, 1, True), D.CentralCrop(512), D.Normalise(*NORM), D.ToTensor()])
    full = D.Compose([D.ResizeScale(2048, 1, 1, True), D.Normalise(*NORM), D.ToTensor()])
    return {"wacv_train_b32": (trn, 32), "wacv_val_b32": (val, 32), "full_2048x1024_b4": (full, 4)}


def time_kernel(n=50):
    rng = np.random.RandomState(0)
    sources = [synthetic(rng) for _ in range(4)]
    for name, (pipe, B) in pipelines().items():
        np.random.seed(0)
        batch = dev.collate([dev.plan_sample(pipe, *sources[i % 4]) for i in range(B)])
        Ho, Wo = (int(v) for v in batch["size"])
        up = {k: batch[k].to(DEV) for k in ("src", "desc", "taps")}
        for dtype in (torch.float32, torch.bfloat16):
            lut = batch["lut"].to(dtype).to(DEV)
            for _ in range(3):
                F.augment(up["src"], up["desc"], up["taps"], lut, Ho, Wo)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                F.augment(up["src"], up["desc"], up["taps"], lut, Ho, Wo)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / n * 1e3
            out_bytes = B * Ho * Wo * (3 * (4 if dtype == torch.float32 else 2) + 1)
            print(json.dumps({"kernel": name, "dtype": str(dtype)[6:], "B": B, "Ho": Ho, "Wo": Wo, "us": round(us, 1),
                              "src_MB": round(up["src"].numel() / 1e6, 2),
                              "out_GBps": round(out_bytes / us / 1e3, 1)}), flush=True)


JITTER = dict(brightness=0.2, contrast=0.3, gamma=0.2, saturation=0.5, hue=0.05)


def colour_tables(B):
    """[B][12] / [B][3][256] on the device: one draw of ColourJitter(**JITTER) per sample, all of them jittered"""
    op = D.ColourJitter(**JITTER)
    tabs = [dev.colour_tables(types.SimpleNamespace(colour=op.draw())) for _ in range(B)]
    return (torch.from_numpy(np.stack([t["colour"] for t in tabs])).to(DEV),
            torch.from_numpy(np.stack([t["ctab"] for t in tabs])).to(DEV))


def alternate(launches, rounds=9, n=200):
    """{name: [us per launch of each round]}: the launches warmed up, then timed in turn, ``rounds`` times"""
    for fn in launches.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in launches}
    for _ in range(rounds):
        for name, fn in launches.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) / n * 1e3)
    return us


def report_colour(kernel, dtype, B, Ho, Wo, us):
    med = {k: float(np.median(v)) for k, v in us.items()}
    print(json.dumps({"kernel": kernel, "dtype": str(dtype)[6:], "B": B, "Ho": Ho, "Wo": Wo,
                      "plain_us": round(med["plain"], 1), "plain_min_max": [round(min(us["plain"]), 1),
                                                                            round(max(us["plain"]), 1)],
                      "colour_us": round(med["colour"], 1), "colour_min_max": [round(min(us["colour"]), 1),
                                                                               round(max(us["colour"]), 1)],
                      "colour_over_plain": round(med["colour"] / med["plain"], 3)}), flush=True)


def time_colour_kernel():
    rng = np.random.RandomState(0)
    sources = [synthetic(rng) for _ in range(4)]
    pipe, B = pipelines()["wacv_train_b32"]
    np.random.seed(0)
    batch = dev.collate([dev.plan_sample(pipe, *sources[i % 4]) for i in range(B)])
    Ho, Wo = (int(v) for v in batch["size"])
    up = {k: batch[k].to(DEV) for k in ("src", "desc", "taps")}
    colour, ctab = colour_tables(B)
    for dtype in (torch.float32, torch.bfloat16):
        lut = batch["lut"].to(dtype).to(DEV)
        us = alternate({"plain": lambda: F.augment(up["src"], up["desc"], up["taps"], lut, Ho, Wo),
                        "colour": lambda: F.augment_colour(up["src"], up["desc"], up["taps"], colour, ctab, lut, Ho,
                                                           Wo)})
        report_colour("wacv_train_b32", dtype, B, Ho, Wo, us)


def time_depth_colour_kernel():
    rng = np.random.RandomState(0)
    sources = [synthetic_depth(rng) for _ in range(4)]
    pipe = D.Compose([D.DepthResizeScale(320, 0.7, 1.4), D.RandomMirror(), D.RandomCrop(320), D.Normalise(*NORM),
                      D.ToTensor()])
    B = 32
    np.random.seed(0)
    batch = dev.collate_depth([dev.plan_depth_sample(pipe, *sources[i % 4]) for i in range(B)])
    Ho, Wo = (int(v) for v in batch["size"])
    up = {k: batch[k].to(DEV) for k in ("src", "desc", "taps", "params")}
    colour, ctab = colour_tables(B)
    for dtype in (torch.float32, torch.bfloat16):
        lut = batch["lut"].to(dtype).to(DEV)
        us = alternate({"plain": lambda: F.augment_depth(up["src"], up["desc"], up["taps"], lut, up["params"], 1e-3,
                                                         Ho, Wo),
                        "colour": lambda: F.augment_depth_colour(up["src"], up["desc"], up["taps"], colour, ctab, lut,
                                                                 up["params"], 1e-3, Ho, Wo)})
        report_colour("depth_train_b32", dtype, B, Ho, Wo, us)


def time_loaders(n_batches, colour=False):
    from nas_segm_amd.data import create_loaders
    from nas_segm_amd.engine.trainer import _labels, _to_device_image

    rng = np.random.RandomState(1)
    with tempfile.TemporaryDirectory() as tmp:
        from PIL import Image

        n_files = 32
        for i in range(n_files):
            img, msk = synthetic(rng)
            Image.fromarray(img).save(os.path.join(tmp, "i{}.png".format(i)), compress_level=1)
            Image.fromarray(msk).save(os.path.join(tmp, "m{}.png".format(i)), compress_level=1)
        B = 32
        lst = os.path.join(tmp, "train.lst")
        with open(lst, "w") as fh:
            fh.write("".join("i{0}.png\tm{0}.png\n".format(i % n_files) for i in range((n_batches + 1) * B)))
        args = types.SimpleNamespace(
            train_dir=tmp, val_dir=tmp, train_list=lst, val_list=lst + ".val", meta_train_prct=80,
            resize_side=[1024], low_scale=0.7, high_scale=1.4, resize_longer_side=True, crop_size=[321],
            val_resize_side=1024, val_crop_size=512, normalise_params=list(NORM), batch_size=[B], val_batch_size=B,
            num_workers=16, colour_jitter=JITTER if colour else None)
        with open(args.val_list, "w") as fh:
            fh.write("i0.png\tm0.png\n")
        results = {}
        for name in ("host", "device"):
            loader = (create_loaders(args) if name == "host" else dev.create_device_loaders(args, device=DEV))[0]
            # (workers started with spawn: none of them inherits this process's open device)
            (loader.loader if name == "device" else loader).multiprocessing_context = "spawn"
            np.random.seed(0)
            t0, seen = None, 0
            for sample in loader:
                if name == "host":
                    image = _to_device_image(sample["image"], torch.device(DEV))
                    mask = _labels(sample["mask"], torch.device(DEV))
                else:
                    image, mask = sample["image"], sample["mask"]
                torch.cuda.synchronize()
                if t0 is None:
                    t0 = time.perf_counter()
                else:
                    seen += image.shape[0]
            dt = time.perf_counter() - t0
            results[name] = seen / dt
            print(json.dumps({"loader": name, "colour": colour, "workers": 16, "batch": B, "images": seen,
                              "s": round(dt, 2), "images_per_s": round(seen / dt, 1), "image": list(image.shape),
                              "dtype": str(image.dtype)[6:]}), flush=True)
        print(json.dumps({"loader": "device_over_host", "ratio": round(results["device"] / results["host"], 2)}))


def synthetic_depth(rng, h=480, w=640):
    """an indoor-like pair: the image of ``synthetic`` and 16-bit counts (millimetres) of a tilted plane with noise
    and holes (0) along an edge and in specks"""
    img, _ = synthetic(rng, h, w)
    yy, xx = np.mgrid[0:h, 0:w]
    counts = 1500 + 4 * xx + 3 * yy + rng.randint(-20, 21, (h, w))
    counts[:, :12] = 0
    counts[rng.rand(h, w) < 0.03] = 0
    return img, counts.astype(np.uint16)


def depth_args(tmp, lst, B, workers):
    return types.SimpleNamespace(
        train_dir=tmp, val_dir=tmp, train_list=lst, val_list=lst + ".val", meta_train_prct=80, resize_side=[320],
        low_scale=0.7, high_scale=1.4, resize_longer_side=False, crop_size=[320], val_resize_side=480,
        val_crop_size=480, normalise_params=list(NORM), batch_size=[B], val_batch_size=B, num_workers=workers)


def time_depth_kernel(n=50):
    rng = np.random.RandomState(0)
    sources = [synthetic_depth(rng) for _ in range(4)]
    pipe = D.Compose([D.DepthResizeScale(320, 0.7, 1.4), D.RandomMirror(), D.RandomCrop(320), D.Normalise(*NORM),
                      D.ToTensor()])
    B = 32
    np.random.seed(0)
    batch = dev.collate_depth([dev.plan_depth_sample(pipe, *sources[i % 4]) for i in range(B)])
    Ho, Wo = (int(v) for v in batch["size"])
    up = {k: batch[k].to(DEV) for k in ("src", "desc", "taps", "params")}
    for dtype in (torch.float32, torch.bfloat16):
        lut = batch["lut"].to(dtype).to(DEV)
        args = (up["src"], up["desc"], up["taps"], lut, up["params"], 1e-3, Ho, Wo)
        for _ in range(3):
            F.augment_depth(*args)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            F.augment_depth(*args)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / n * 1e3
        out_bytes = B * Ho * Wo * (3 * (4 if dtype == torch.float32 else 2) + 4)
        print(json.dumps({"kernel": "depth_train_b32", "dtype": str(dtype)[6:], "B": B, "Ho": Ho, "Wo": Wo,
                          "us": round(us, 1), "src_MB": round(up["src"].numel() / 1e6, 2),
                          "out_GBps": round(out_bytes / us / 1e3, 1)}), flush=True)


def time_depth_loaders(n_batches, colour=False):
    from nas_segm_amd.data import create_depth_loaders
    from nas_segm_amd.engine.trainer import _depth_target, _to_device_image

    rng = np.random.RandomState(1)
    with tempfile.TemporaryDirectory() as tmp:
        from PIL import Image

        n_files = 32
        for i in range(n_files):
            img, counts = synthetic_depth(rng)
            Image.fromarray(img).save(os.path.join(tmp, "i{}.png".format(i)), compress_level=1)
            Image.fromarray(counts).save(os.path.join(tmp, "d{}.png".format(i)), compress_level=1)
        B = 32
        lst = os.path.join(tmp, "train.lst")
        with open(lst, "w") as fh:
            fh.write("".join("i{0}.png\td{0}.png\n".format(i % n_files) for i in range((n_batches + 1) * B)))
        args = depth_args(tmp, lst, B, 16)
        args.colour_jitter = JITTER if colour else None
        with open(args.val_list, "w") as fh:
            fh.write("i0.png\td0.png\n")
        results = {}
        for name in ("host", "device"):
            loader = (create_depth_loaders(args) if name == "host"
                      else dev.create_device_depth_loaders(args, device=DEV))[0]
            # (workers started with spawn: none of them inherits this process's open device)
            (loader.loader if name == "device" else loader).multiprocessing_context = "spawn"
            np.random.seed(0)
            t0, seen = None, 0
            for sample in loader:
                if name == "host":
                    image = _to_device_image(sample["image"], torch.device(DEV))
                    target = _depth_target(sample["mask"], torch.device(DEV))
                else:
                    image, target = sample["image"], sample["mask"]
                torch.cuda.synchronize()
                if t0 is None:
                    t0 = time.perf_counter()
                else:
                    seen += image.shape[0]
            dt = time.perf_counter() - t0
            results[name] = seen / dt
            print(json.dumps({"depth_loader": name, "colour": colour, "workers": 16, "batch": B, "images": seen, "s": round(dt, 2),
                              "images_per_s": round(seen / dt, 1), "image": list(image.shape),
                              "dtype": str(image.dtype)[6:], "target": str(target.dtype)[6:]}), flush=True)
        print(json.dumps({"depth_loader": "device_over_host",
                          "ratio": round(results["device"] / results["host"], 2)}))


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a not in ("--depth", "--colour")]
    depth, colour = "--depth" in sys.argv[1:], "--colour" in sys.argv[1:]
    what = argv[0] if argv else "all"
    if what in ("kernel", "all"):
        if colour:
            (time_depth_colour_kernel if depth else time_colour_kernel)()
        else:
            (time_depth_kernel if depth else time_kernel)()
    if what in ("loader", "all"):
        (time_depth_loaders if depth else time_loaders)(int(os.environ.get("KBENCH_BATCHES", "24")), colour)
