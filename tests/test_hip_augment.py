"""The device augmentation (data/device.py + csrc/augment.hip) on the GPU: the batches of the host pipeline, bit for
bit after the engine's dtype cast (fp32 and bf16), on the reference's golden dataset fixtures, on full-size
sources, through the loaders, and through one training epoch and one validation."""
import types

import numpy as np
import pytest
import torch

from _util import build_product_net, load_json, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NPZ = load_npz("data.npz")
META = load_json("data_meta.json")
MEAN = np.array([0.485, 0.456, 0.406]).reshape((1, 1, 3))
STD = np.array([0.229, 0.224, 0.225]).reshape((1, 1, 3))
DTYPES = (torch.float32, torch.bfloat16)


def mods():
    from nas_segm_amd.data import datasets, device

    return datasets, device


def equal(got, want):
    """exact equality of values (the device image is channels_last, the host one NCHW)"""
    return got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape) and torch.equal(got.cpu(), want.cpu())


def on_device(samples, dtype):
    _, dev = mods()
    out = dev.run_batch(dev.collate(samples), torch.device(DEV), dtype)
    assert out["image"].is_contiguous(memory_format=torch.channels_last) and out["mask"].dtype == torch.uint8
    return out


def test_golden_dataset_fixtures(tmp_path):
    from PIL import Image

    D, dev = mods()
    for i, (a, b) in enumerate(META["names"]):
        Image.fromarray(NPZ["file{}/image".format(i)]).save(str(tmp_path / a))
        Image.fromarray(NPZ["file{}/mask".format(i)]).save(str(tmp_path / b))
    (tmp_path / "two.lst").write_text("".join("{}\t{}\n".format(a, b) for a, b in META["names"]))
    norm = D.Normalise(1.0 / 255, MEAN, STD)
    trn = D.Compose([D.ResizeShorter(16), D.CentralCrop(30), D.RandomCrop(24), norm, D.ToTensor()])
    val = D.Compose([D.CentralCrop(32), norm, D.ToTensor()])
    ds = dev.DevicePascalDataset(str(tmp_path / "two.lst"), str(tmp_path), trn, val)

    def check(samples, keys):
        for dtype in DTYPES:
            out = on_device(samples, dtype)
            for b, key in enumerate(keys):
                want = torch.from_numpy(NPZ[key + "/image"]).to(dtype)
                assert equal(out["image"][b], want), (key, dtype)
                assert equal(out["mask"][b], torch.from_numpy(NPZ[key + "/mask"])), key

    np.random.seed(9)
    check([ds[i] for i in range(3)], ["ds_trn{}".format(i) for i in range(3)])
    ds.set_stage("val")
    check([ds[i] for i in range(3)], ["ds_val{}".format(i) for i in range(3)])
    ds.set_stage("train")
    ds.set_config(20, 8)
    np.random.seed(10)
    check([ds[2]], ["ds_cfg"])


@pytest.mark.parametrize("scale", [0.5, 1.0, 1.37, 2.0])
def test_full_size_sources(scale):
    D, dev = mods()
    rng = np.random.RandomState(int(scale * 100))
    # smooth content plus noise: the resize's coefficients of every sign matter, and saturation is reached
    yy, xx = np.mgrid[0:1024, 0:2048]
    base = 127.5 + 127.5 * np.sin(xx[:, :, None] / (37.0 + 11 * np.arange(3)) + yy[:, :, None] / 53.0)
    pipe = D.Compose([D.ResizeScale(1024, scale, scale), D.Pad(1100, (124.4, 116, 104), 255), D.RandomMirror(),
                      D.RandomCrop(1024), D.Normalise(1.0 / 255, MEAN, STD), D.ToTensor()])
    host, plans = [], []
    for k in range(2):
        img = np.clip(base + rng.randint(-40, 41, base.shape), 0, 255).astype(np.uint8)
        msk = rng.randint(0, 21, (1024, 2048)).astype(np.uint8)
        np.random.seed(k)
        host.append(pipe({"image": img, "mask": msk}))
        state = np.random.get_state()
        np.random.seed(k)
        plans.append(dev.plan_sample(pipe, img, msk))
        assert np.array_equal(np.random.get_state()[1], state[1])
    for dtype in DTYPES:
        out = on_device(plans, dtype)
        for b, h in enumerate(host):
            assert equal(out["image"][b], h["image"].to(dtype)), (scale, dtype, b)
            assert equal(out["mask"][b], h["mask"]), (scale, b)


def _files(tmp_path, n):
    from PIL import Image

    rng = np.random.RandomState(1)
    lines = []
    for i in range(n):
        h, w = 50 + 3 * i, 70 - 2 * i
        img = (rng.rand(h, w) * 255).astype(np.uint8) if i % 4 == 3 else (rng.rand(h, w, 3) * 255).astype(np.uint8)
        Image.fromarray(img).save(str(tmp_path / "i{}.png".format(i)))
        Image.fromarray((rng.rand(h, w) * 21).astype(np.uint8)).save(str(tmp_path / "m{}.png".format(i)))
        lines.append("i{}.png\tm{}.png\n".format(i, i))
    (tmp_path / "train.lst").write_text("".join(lines))
    (tmp_path / "val.lst").write_text("".join(lines[:4]))
    return types.SimpleNamespace(
        train_dir=str(tmp_path), val_dir=str(tmp_path), train_list=str(tmp_path / "train.lst"),
        val_list=str(tmp_path / "train.lst"), meta_train_prct=80, resize_side=[40], low_scale=0.7, high_scale=1.4,
        resize_longer_side=False, crop_size=[32], val_resize_side=40, val_crop_size=32,
        normalise_params=[1.0 / 255, MEAN, STD], batch_size=[4], val_batch_size=2, num_workers=0)


def _both(args, dtype=torch.float32):
    from nas_segm_amd.data import create_loaders

    _, dev = mods()
    torch.manual_seed(0)
    host = create_loaders(args)
    torch.manual_seed(0)
    device = dev.create_device_loaders(args, device=DEV, dtype=dtype)
    return host, device


def _epoch_equal(host_loader, dev_loader, seed, dtype=torch.float32):
    torch.manual_seed(seed)
    np.random.seed(seed)
    want = list(host_loader)
    torch.manual_seed(seed)
    np.random.seed(seed)
    got = list(dev_loader)
    assert len(want) == len(got) > 0
    for h, d in zip(want, got):
        assert equal(d["image"], h["image"].to(dtype)) and equal(d["mask"], h["mask"])
    return len(got)


@pytest.mark.parametrize("search", [True, False])
def test_loaders_yield_the_host_batches(tmp_path, search):
    from nas_segm_amd.engine.trainer import _set_stage

    args = _files(tmp_path, 12)
    if not search:
        args.val_list = str(tmp_path / "val.lst")
    (h_trn, h_val, h_search), (d_trn, d_val, d_search) = _both(args)
    assert h_search == d_search == search
    assert len(h_trn) == len(d_trn) and len(h_val) == len(d_val)
    for epoch in range(2):
        for loader in (h_trn, d_trn):
            _set_stage(loader, "train")
        _epoch_equal(h_trn, d_trn, epoch)
        for loader in (h_val, d_val):
            _set_stage(loader, "val")
        _epoch_equal(h_val, d_val, 10 + epoch)
    # the search script between tasks (src/main_search.py:559-568)
    for loader in (h_trn, d_trn):
        loader.batch_sampler.batch_size = 3
        ds = loader.dataset.dataset if search else loader.dataset
        ds.set_config(24, 30)
        _set_stage(loader, "train")
    assert _epoch_equal(h_trn, d_trn, 5) == len(h_trn)
    assert next(iter(d_trn))["image"].shape[2:] == (24, 24)


def test_bf16_loader(tmp_path):
    args = _files(tmp_path, 8)
    (h_trn, _, _), (d_trn, _, _) = _both(args, torch.bfloat16)
    _epoch_equal(h_trn, d_trn, 3, torch.bfloat16)


def test_one_epoch_and_validation_from_either_loader(tmp_path, monkeypatch):
    from nas_segm_amd.engine import RankParallel
    from nas_segm_amd.engine import trainer
    from nas_segm_amd.engine.inference import validate

    monkeypatch.setenv("NASSEG_GRAPH", "0")
    args = _files(tmp_path, 12)
    genotype = [[[3, 0, 1], [4, 1, 1], [3, 1, 1]],
                [[0, 1, 0, 0, 1], [2, 1, 2, 1, 0], [3, 1, 1, 1, 0], [1, 1, 2, 0, 0],
                 [3, 0, 2, 0, 0], [5, 3, 2, 1, 0], [0, 5, 0, 1, 0]]]
    losses = []
    orig = trainer.F.log_softmax_nll

    def rec(logits, target, ignore_index=255):
        v = orig(logits, target, ignore_index)
        losses.append(float(v.detach()))
        return v

    monkeypatch.setattr(trainer.F, "log_softmax_nll", rec)

    class Crit(object):
        ignore_index = 255

    def run(train_loader, val_loader):
        del losses[:]
        net = build_product_net("template", genotype, 21, dict(agg_size=32, repeats=1), 0)
        segmenter = RankParallel(net.to(DEV))
        optim_enc = torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-5)
        optim_dec = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
        torch.manual_seed(4)
        np.random.seed(4)
        trainer.train_segmenter.__wrapped__(segmenter, train_loader, optim_enc, optim_dec, 0, Crit(), False, 3.0,
                                            3.0, False, print_every=100)
        reward = validate.__wrapped__(segmenter, val_loader, 0, 0, num_classes=21, print_every=100,
                                      omit_classes=[0])
        return list(losses), {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, reward

    (h_trn, h_val, _), (d_trn, d_val, _) = _both(args)
    h_losses, h_sd, h_reward = run(h_trn, h_val)
    d_losses, d_sd, d_reward = run(d_trn, d_val)
    assert len(h_losses) == len(h_trn) > 0 and h_losses == d_losses
    assert all(torch.equal(h_sd[k], d_sd[k]) for k in h_sd)
    assert h_reward == d_reward


@pytest.mark.parametrize("kind", ["label", "depth"])
def test_a_window_outside_src_is_read_as_fill(kind):
    """Whatever the descriptor holds, no load leaves ``src``: a window that does not lie inside it is read as fill.
    Three 17 x 19 samples (323 pixels: a full block of 256 threads and a ragged one), identity taps, every pixel
    live; one field of sample 1's descriptor - its windows lie in the middle of ``src`` - is changed at a time.  The
    half of sample 1 whose window it is becomes that half's fill, exactly (lut[c][fill byte c]; the mask fill;
    params[1][1] NOT divided by the zoom); everything else is the unmodified launch's, bit for bit.  ``src`` is a
    slice of a larger buffer with 4096 bytes on either side that hold a value no fill has, so a wrong read would be
    a wrong value and never an access out of bounds."""
    from nas_segm_amd import functional as F

    D, dev = mods()
    Ho, Wo, guard, elem = 17, 19, 4096, 1 if kind == "label" else 2
    img_fill, msk_fill, depth_fill, guard_byte = (11, 22, 33), 200, 7.5, 238
    pipe = D.Compose([D.Normalise(1.0 / 255, MEAN, STD), D.ToTensor()])
    rng = np.random.RandomState(0)
    images = [(rng.rand(Ho, Wo, 3) * 255).astype(np.uint8) for _ in range(3)]
    if kind == "label":  # labels below 21, counts of at most 4.5 m after the zoom: no live value is a fill
        batch = dev.collate([dev.plan_sample(pipe, img, (rng.rand(Ho, Wo) * 21).astype(np.uint8)) for img in images])
    else:
        batch = dev.collate_depth([dev.plan_depth_sample(pipe, img, rng.randint(1, 9000, (Ho, Wo)).astype(np.uint16))
                                   for img in images])
        params = torch.tensor([[2.0, depth_fill]] * 3, dtype=torch.float32, device=DEV)
    assert tuple(batch["size"]) == (Ho, Wo) and bool((batch["taps"] >= 0).all())
    field = {name: i for i, name in enumerate(dev.Desc._fields)}
    desc = batch["desc"].clone()
    desc[:, field["img_fill"]] = img_fill[0] | img_fill[1] << 8 | img_fill[2] << 16
    desc[:, field["msk_fill"]] = msk_fill
    n = batch["src"].numel()
    img_bytes, msk_bytes = 3 * Ho * Wo, elem * Ho * Wo
    assert n == 3 * (img_bytes + msk_bytes)
    assert desc[1].tolist()[:6] == [img_bytes + msk_bytes, 2 * img_bytes + msk_bytes, Ho, Wo, 3 * Wo, elem * Wo]
    big = torch.full((guard + n + guard,), guard_byte, dtype=torch.uint8, device=DEV)
    src = big[guard: guard + n]
    src.copy_(batch["src"])
    taps = batch["taps"].to(DEV)
    IMAGE, TARGET = 0, 1
    changes = [("msk_off", -1, {TARGET}), ("msk_off", n - msk_bytes + elem, {TARGET}),
               ("msk_ld", elem * Wo - 1, {TARGET}),
               ("img_off", -1, {IMAGE}), ("img_off", n - img_bytes + 3, {IMAGE}), ("img_ld", 3 * Wo - 1, {IMAGE}),
               ("h", 0, {IMAGE, TARGET})]

    for dtype in DTYPES:
        lut = batch["lut"].to(dtype).to(DEV)

        def launch(d):
            if kind == "label":
                return F.augment(src, d.to(DEV), taps, lut, Ho, Wo)
            return F.augment_depth(src, d.to(DEV), taps, lut, params, 1e-3, Ho, Wo)

        fills = (torch.stack([lut[c, v] for c, v in enumerate(img_fill)]).view(3, 1, 1).expand(3, Ho, Wo),
                 torch.full((Ho, Wo), msk_fill, dtype=torch.uint8) if kind == "label"
                 else torch.full((Ho, Wo), depth_fill, dtype=torch.float32))
        base = launch(desc)
        for half in (IMAGE, TARGET):  # (the unmodified launch holds no fill pixel)
            assert not bool((base[half][1].cpu() == fills[half].cpu()).all(dim=0).any() if half == IMAGE
                            else (base[half][1].cpu() == fills[half]).any())
        for name, value, filled in changes:
            d = desc.clone()
            d[1, field[name]] = value
            got = launch(d)
            for half in (IMAGE, TARGET):
                for b in range(3):
                    want = fills[half] if b == 1 and half in filled else base[half][b]
                    assert equal(got[half][b], want), (kind, dtype, name, value, half, b)
    assert bool((big[:guard] == guard_byte).all()) and bool((big[guard + n:] == guard_byte).all())
