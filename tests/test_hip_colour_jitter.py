"""ColourJitter on the GPU (csrc/augment.hip: nasseg_augment_colour, nasseg_augment_depth_colour): the batches of the
host pipeline bit for bit after the engine's dtype cast (fp32 and bf16), for label and depth samples, through the
loaders, and the plain launch's image when the colour tables are the identity."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN = np.array([0.485, 0.456, 0.406]).reshape((1, 1, 3))
STD = np.array([0.229, 0.224, 0.225]).reshape((1, 1, 3))
DTYPES = (torch.float32, torch.bfloat16)
JITTER = dict(brightness=0.25, contrast=0.4, gamma=0.3, saturation=0.8, hue=0.15, p=0.5)
FILL = (124.4, 116, 104)


def mods():
    from nas_segm_amd.data import datasets, device

    return datasets, device


def equal(got, want):
    """exact equality of values (the device image is channels_last, the host one NCHW)"""
    return got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape) and torch.equal(got.cpu(), want.cpu())


def sample(h, w, seed):
    rng = np.random.RandomState(seed)
    return (rng.rand(h, w, 3) * 255).astype(np.uint8), (rng.rand(h, w) * 21).astype(np.uint8)


def sources(rows=None, cols=None):
    return [(img[:rows, :cols], msk[:rows, :cols]) for img, msk in (sample(37, 53, 0), sample(41, 29, 1),
                                                                    sample(37, 53, 2))]


def cases():
    """name -> (operations before Normalise, sources, output size)"""
    D, _ = mods()
    cj = D.ColourJitter(**JITTER)
    return {
        "24x32": ([D.ResizeScale(10, 1.2, 1.2), D.RandomMirror(), D.RandomCrop(32), cj], sources(rows=20), (24, 32)),
        # 323 pixels: one full block of 256 threads and a ragged one; 228 pixels: a single ragged block
        "17x19_ragged_block": ([D.RandomMirror(), D.RandomCrop(32), cj], sources(17, 19), (17, 19)),
        "12x19_one_ragged_block": ([D.RandomMirror(), D.RandomCrop(32), cj], sources(12, 19), (12, 19)),
        "40x40_pad_before": ([D.ResizeScale(10, 0.8, 1.2), D.Pad(44, FILL, 255), cj, D.RandomMirror(),
                              D.RandomCrop(40)], sources(), (40, 40)),
        "40x40_pad_after": ([D.ResizeScale(10, 0.8, 1.2), D.RandomCrop(22), cj, D.Pad(40, FILL, 255)], sources(),
                            (40, 40)),
        "24x32_clipping_extremes": ([D.ResizeScale(10, 1.2, 1.2), D.RandomCrop(32),
                                     D.ColourJitter(0.5, 0.9, 0.9, 3.0, 0.5)], sources(rows=20), (24, 32)),
    }


def planned(name):
    """(host samples, device samples) of one case under a seed that gives jittered and identity samples (chosen on the
    host; the extremes case jitters every sample)"""
    D, dev = mods()
    ops, srcs, size = cases()[name]
    pipe = D.Compose(ops + [D.Normalise(1.0 / 255, MEAN, STD), D.ToTensor()])
    for seed in range(100):
        np.random.seed(seed)
        plans = [dev.plan_sample(pipe, img, msk) for img, msk in srcs]
        kinds = {bool(p["colour"][9]) for p in plans}
        if kinds == {True, False} or (name.endswith("extremes") and kinds == {True}):
            break
    else:
        raise AssertionError("no seed with both kinds of samples")
    state = np.random.get_state()
    np.random.seed(seed)
    host = [pipe({"image": img, "mask": msk}) for img, msk in srcs]
    assert np.array_equal(np.random.get_state()[1], state[1])
    assert all(tuple(p["size"]) == size for p in plans)
    return host, plans


@pytest.mark.parametrize("name", ["24x32", "17x19_ragged_block", "12x19_one_ragged_block", "40x40_pad_before",
                                  "40x40_pad_after", "24x32_clipping_extremes"])
def test_run_batch_equals_the_host_pipeline(name):
    _, dev = mods()
    host, plans = planned(name)
    batch = dev.collate(plans)
    if "pad" in name:  # fill pixels are in the batch
        assert (batch["taps"][:, :8 * 80].reshape(3, 80, 8)[:, :, 0] < 0).any()
    for dtype in DTYPES:
        out = dev.run_batch(batch, torch.device(DEV), dtype)
        assert out["image"].is_contiguous(memory_format=torch.channels_last) and out["mask"].dtype == torch.uint8
        for b, h in enumerate(host):
            assert equal(out["image"][b], h["image"].to(dtype)), (name, dtype, b)
            assert equal(out["mask"][b], h["mask"]), (name, b)


def _files(tmp_path, n, depth=False):
    from PIL import Image

    rng = np.random.RandomState(1)
    lines = []
    for i in range(n):
        h, w = 50 + 3 * i, 70 - 2 * i
        img = (rng.rand(h, w) * 255).astype(np.uint8) if i % 4 == 3 else (rng.rand(h, w, 3) * 255).astype(np.uint8)
        Image.fromarray(img).save(str(tmp_path / "i{}.png".format(i)))
        if depth:
            counts = (rng.rand(h, w) * 9000).astype(np.uint16)
            counts[rng.rand(h, w) < 0.05] = 0
            Image.fromarray(counts).save(str(tmp_path / "m{}.png".format(i)))
        else:
            Image.fromarray((rng.rand(h, w) * 21).astype(np.uint8)).save(str(tmp_path / "m{}.png".format(i)))
        lines.append("i{}.png\tm{}.png\n".format(i, i))
    (tmp_path / "train.lst").write_text("".join(lines))
    (tmp_path / "val.lst").write_text("".join(lines[:4]))
    return types.SimpleNamespace(
        train_dir=str(tmp_path), val_dir=str(tmp_path), train_list=str(tmp_path / "train.lst"),
        val_list=str(tmp_path / "train.lst"), meta_train_prct=80, resize_side=[40], low_scale=0.7, high_scale=1.4,
        resize_longer_side=False, crop_size=[32], val_resize_side=40, val_crop_size=32,
        normalise_params=[1.0 / 255, MEAN, STD], batch_size=[4], val_batch_size=2, num_workers=0,
        colour_jitter=dict(JITTER))


def test_run_depth_batch_equals_the_host_samples(tmp_path):
    from nas_segm_amd.data import create_depth_loaders

    _, dev = mods()
    args = _files(tmp_path, 8, depth=True)
    torch.manual_seed(0)
    host_part = create_depth_loaders(args)[0].dataset
    torch.manual_seed(0)
    dev_part = dev.create_device_depth_loaders(args, device=DEV)[0].dataset
    assert host_part.indices == dev_part.indices
    assert [type(op).__name__ for op in dev_part.dataset.transform_trn.transforms][3] == "ColourJitter"
    np.random.seed(3)
    host = [host_part[i] for i in range(4)]
    np.random.seed(3)
    plans = [dev_part[i] for i in range(4)]
    batch = dev.collate_depth(plans)
    assert len(set(batch["colour"][:, 9].tolist())) == 2  # jittered and identity samples (p = 0.5, seed 3)
    for dtype in DTYPES:
        out = dev.run_depth_batch(batch, torch.device(DEV), dtype, 1e-3)
        assert out["mask"].dtype == torch.float32
        for b, h in enumerate(host):
            assert equal(out["image"][b], h["image"].to(dtype)), (dtype, b)
            assert equal(out["mask"][b], h["mask"]), b


@pytest.mark.parametrize("search", [True, False])
def test_loaders_yield_the_host_batches(tmp_path, search):
    from nas_segm_amd.data import create_loaders
    from nas_segm_amd.engine.trainer import _set_stage

    _, dev = mods()
    args = _files(tmp_path, 12)
    if not search:
        args.val_list = str(tmp_path / "val.lst")
    torch.manual_seed(0)
    h_trn, h_val, h_search = create_loaders(args)
    torch.manual_seed(0)
    d_trn, d_val, d_search = dev.create_device_loaders(args, device=DEV)
    assert h_search == d_search == search
    for stage, (h_loader, d_loader) in (("train", (h_trn, d_trn)), ("val", (h_val, d_val))):
        for loader in (h_loader, d_loader):
            _set_stage(loader, stage)
        torch.manual_seed(7)
        np.random.seed(7)
        want = list(h_loader)
        torch.manual_seed(7)
        np.random.seed(7)
        got = list(d_loader)
        assert len(want) == len(got) > 0
        for h, d in zip(want, got):
            assert equal(d["image"], h["image"].to(torch.float32)) and equal(d["mask"], h["mask"])


def test_identity_colour_is_the_plain_launch():
    from nas_segm_amd import functional as F

    D, dev = mods()
    ops, srcs, (Ho, Wo) = cases()["40x40_pad_before"]
    pipe = D.Compose([op for op in ops if not isinstance(op, D.ColourJitter)]
                     + [D.Normalise(1.0 / 255, MEAN, STD), D.ToTensor()])
    np.random.seed(0)
    batch = dev.collate([dev.plan_sample(pipe, img, msk) for img, msk in srcs])
    up = {k: batch[k].to(DEV) for k in ("src", "desc", "taps")}
    colour = torch.tensor([[4096, 0, 0, 0, 4096, 0, 0, 0, 4096, 0, 0, 0]] * 3, dtype=torch.int32, device=DEV)
    ctab = torch.arange(256, dtype=torch.uint8, device=DEV).repeat(3, 3, 1).contiguous()
    for dtype in DTYPES:
        lut = batch["lut"].to(dtype).to(DEV)
        image, mask = F.augment(up["src"], up["desc"], up["taps"], lut, Ho, Wo)
        image_c, mask_c = F.augment_colour(up["src"], up["desc"], up["taps"], colour, ctab, lut, Ho, Wo)
        assert image_c.is_contiguous(memory_format=torch.channels_last)
        assert equal(image_c, image) and equal(mask_c, mask)
        # the unit matrix applied is the identity too
        unit = colour.clone()
        unit[:, 9] = 1
        assert equal(F.augment_colour(up["src"], up["desc"], up["taps"], unit, ctab, lut, Ho, Wo)[0], image)


def test_argument_checks():
    from nas_segm_amd import NassegError
    from nas_segm_amd import functional as F

    D, dev = mods()
    pipe = D.Compose([D.DepthResizeScale(10, 1.0, 1.0), D.RandomCrop(24), D.ColourJitter(**JITTER),
                      D.Normalise(1.0 / 255, MEAN, STD), D.ToTensor()])
    np.random.seed(0)
    rng = np.random.RandomState(0)
    label = dev.collate([dev.plan_sample(pipe, img, msk) for img, msk in sources()])
    depth = dev.collate_depth([dev.plan_depth_sample(pipe, img, rng.randint(0, 9000, msk.shape).astype(np.uint16))
                               for img, msk in sources()])
    Ho, Wo = 24, 24

    def calls(batch, fn, tail):
        up = {k: batch[k].to(DEV) for k in ("src", "desc", "taps", "colour", "ctab")}
        lut = batch["lut"].to(torch.float32).to(DEV)

        def call(colour=up["colour"], ctab=up["ctab"], wo=Wo):
            return fn(up["src"], up["desc"], up["taps"], colour, ctab, lut, *(tail + (Ho, wo)))

        call()  # (the batch itself is fine)
        wide = torch.zeros((3, 24), dtype=torch.int32, device=DEV)
        tall = torch.zeros((3, 3, 512), dtype=torch.uint8, device=DEV)
        bad = [dict(colour=up["colour"].to(torch.int64)), dict(colour=up["colour"].float()),
               dict(colour=up["colour"][:, :9].contiguous()), dict(colour=up["colour"][:2]),
               dict(colour=wide[:, ::2]), dict(colour=up["colour"].cpu()),
               dict(ctab=up["ctab"].to(torch.int8)), dict(ctab=up["ctab"].to(torch.int32)),
               dict(ctab=up["ctab"][:, 0].contiguous()), dict(ctab=up["ctab"][:2]), dict(ctab=tall[:, :, ::2]),
               dict(ctab=up["ctab"].reshape(3, 768)), dict(wo=Wo + 1)]
        for kw in bad:
            with pytest.raises(NassegError):
                call(**kw)

    calls(label, F.augment_colour, ())
    calls(depth, F.augment_depth_colour, (depth["params"].to(DEV), 1e-3))
    torch.cuda.synchronize()
