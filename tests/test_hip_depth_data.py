"""Depth targets of the device data pipeline (data/device.py + csrc/augment.hip: nasseg_augment_depth) on the GPU:
the batches of the host pipeline (data/datasets.py: _load_depth, DepthResizeScale), bit for bit - the image after
the engine's dtype cast (fp32 and bf16), the fp32 target in every bit -, through the kernel, through the loaders,
and through one depth training epoch and one validation."""
import types

import numpy as np
import pytest
import torch

from _util import build_product_net

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN = np.array([0.485, 0.456, 0.406]).reshape((1, 1, 3))
STD = np.array([0.229, 0.224, 0.225]).reshape((1, 1, 3))
DTYPES = (torch.float32, torch.bfloat16)
SCALE = 1e-3
SIZES = ((37, 53), (41, 65))  # odd heights and widths: a source shipped whole is 3 h w, an odd number of bytes
SCALES = (0.5, 1.0, 1.37, 2.0)
# seeds of the two samples per scale, chosen on the CPU with the host pipeline alone so that the cases bite (``cases``
# asserts it): both mirror outcomes, fill and gathered pixels, counts 0 and 65535 among the gathered ones, count
# windows that start at an odd byte of the packed batch
SEEDS = {0.5: (0, 1), 1.0: (2, 3), 1.37: (4, 5), 2.0: (6, 7)}


def mods():
    from nas_segm_amd.data import datasets, device

    return datasets, device


def equal(got, want):
    """exact equality of values (the device image is channels_last, the host one NCHW)"""
    return got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape) and torch.equal(got.cpu(), want.cpu())


def sample(h, w, seed):
    rng = np.random.RandomState(seed)
    img = (rng.rand(h, w, 3) * 255).astype(np.uint8)
    counts = rng.randint(1, 65535, (h, w)).astype(np.uint16)
    counts[rng.rand(h, w) < 0.15] = 0
    counts[rng.rand(h, w) < 0.15] = 65535
    return img, counts


def metres(counts, scale=SCALE):
    return counts.astype(np.float32) * np.float32(scale)


def pipeline(s):
    D, _ = mods()
    return D.Compose([D.DepthResizeScale(20, s, s), D.Pad(60, (124.4, 116, 104), 0), D.RandomMirror(),
                      D.RandomCrop(48), D.Normalise(1.0 / 255, MEAN, STD), D.ToTensor()])


def host_and_plans(pipe, sources, seeds):
    """the host pipeline's samples and the device plans of the sources, from the same random state"""
    _, dev = mods()
    host, plans = [], []
    for (img, counts), seed in zip(sources, seeds):
        np.random.seed(seed)
        host.append(pipe({"image": img, "mask": metres(counts)}))
        state = np.random.get_state()
        np.random.seed(seed)
        plans.append(dev.plan_depth_sample(pipe, img, counts))
        assert np.array_equal(np.random.get_state()[1], state[1])
    return host, plans


def on_device(plans, dtype, depth_scale=SCALE):
    _, dev = mods()
    out = dev.run_depth_batch(dev.collate_depth(plans), torch.device(DEV), dtype, depth_scale)
    assert out["image"].is_contiguous(memory_format=torch.channels_last) and out["image"].dtype == dtype
    assert out["mask"].dtype == torch.float32 and out["mask"].is_contiguous()
    return out


@pytest.fixture(scope="module")
def cases():
    """{scale: (host samples, device plans)}, computed once on the host - and the inventory of what they exercise"""
    out = {}
    _, dev = mods()
    mirrored, fill, live, zero, top, divisors, odd = set(), 0, 0, 0, 0, set(), 0
    for s in SCALES:
        sources = [sample(h, w, 100 + seed) for (h, w), seed in zip(SIZES, SEEDS[s])]
        host, plans = out[s] = host_and_plans(pipeline(s), sources, SEEDS[s])
        odd += int((dev.collate_depth(plans)["desc"][:, 1] % 2).sum())  # count windows that start at an odd byte
        for seed, h, p in zip(SEEDS[s], host, plans):
            np.random.seed(seed)
            np.random.uniform(s, s)                    # DepthResizeScale's draw
            mirrored.add(int(np.random.randint(2)))    # RandomMirror's
            Ho, Wo = p["size"]
            my, mx = p["taps"][8 * (Ho + Wo): 8 * (Ho + Wo) + Ho], p["taps"][8 * (Ho + Wo) + Ho:]
            gathered = (my >= 0)[:, None] & (mx >= 0)[None, :]
            target = h["mask"].numpy()
            zoom = p["params"][0]
            fill += int((~gathered).sum())
            live += int(gathered.sum())
            zero += int((target[gathered] == 0).sum())
            top += int((target[gathered] == np.float32(65535) * np.float32(SCALE) / zoom).sum())
            divisors.add(float(zoom))
    assert mirrored == {0, 1} and fill > 0 and live > 0 and zero > 0 and top > 0
    assert any(d != 1.0 for d in divisors) and 1.0 in divisors and odd > 0
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("s", SCALES)
def test_kernel_against_the_host_pipeline(cases, s, dtype):
    host, plans = cases[s]
    out = on_device(plans, dtype)
    for b, h in enumerate(host):
        assert h["mask"].dtype == torch.float32
        assert equal(out["image"][b], h["image"].to(dtype)), (s, dtype, b)
        assert equal(out["mask"][b], h["mask"]), (s, dtype, b)


@pytest.mark.parametrize("pad", ["seven", "zero", "none"])
def test_fill_pixels_are_written_undivided(pad):
    D, dev = mods()
    s = 2.0
    # 21 x 25 and 25 x 21 sources: 42 x 50 and 50 x 42 after the zoom, inside the 60 x 60 frame of the Pad
    ops = [D.DepthResizeScale(10, s, s)]
    if pad != "none":
        ops.append(D.Pad(60, (1, 2, 3), 7 if pad == "seven" else 0))
    ops += [D.RandomMirror(), D.CentralCrop(36 if pad == "none" else 56), D.Normalise(1.0 / 255, MEAN, STD),
            D.ToTensor()]
    sources = [sample(h, w, 50 + k) for k, (h, w) in enumerate(((21, 25), (25, 21)))]
    for _, counts in sources:
        counts[counts == 0] = 1  # (no holes here: every 0.0 below is fill)
    host, plans = host_and_plans(D.Compose(ops), sources, (0, 1))
    assert all(p["params"][0] == np.float32(2.0) for p in plans)
    for dtype in DTYPES:
        out = on_device(plans, dtype)
        got = out["mask"].cpu().numpy()
        for b, h in enumerate(host):
            assert equal(out["mask"][b], h["mask"]) and equal(out["image"][b], h["image"].to(dtype))
        if pad == "none":
            assert (got > 0).all()
            continue
        want = np.float32(7.0 if pad == "seven" else 0.0)
        # sample 0: 9 rows / 5 columns of fill on each side of the 60 x 60 frame, of which the crop takes 2 away;
        # the border is the fill itself - not fill / 2
        assert (got[0, :7] == want).all() and (got[0, -7:] == want).all()
        assert (got[0, :, :3] == want).all() and (got[0, :, -3:] == want).all()
        inner = got[0, 7:-7, 3:-3]
        assert (inner != want).all() and (inner > 0).all() and (inner <= np.float32(65.535 / 2)).all()


def _files(tmp_path, n):
    from PIL import Image

    lines = []
    for i in range(n):
        h, w = 51 + 2 * i, 69 - 2 * i
        img, counts = sample(h, w, 200 + i)
        Image.fromarray(img[:, :, 0] if i % 4 == 3 else img).save(str(tmp_path / "i{}.png".format(i)))
        Image.fromarray(counts).save(str(tmp_path / "d{}.png".format(i)))
        lines.append("i{0}.png\td{0}.png\n".format(i))
    (tmp_path / "train.lst").write_text("".join(lines))
    (tmp_path / "val.lst").write_text("".join(lines[:4]))
    return types.SimpleNamespace(
        train_dir=str(tmp_path), val_dir=str(tmp_path), train_list=str(tmp_path / "train.lst"),
        val_list=str(tmp_path / "train.lst"), meta_train_prct=80, resize_side=[40], low_scale=0.7, high_scale=1.4,
        resize_longer_side=False, crop_size=[32], val_resize_side=40, val_crop_size=32,
        normalise_params=[1.0 / 255, MEAN, STD], batch_size=[4], val_batch_size=2, num_workers=0)


def _both(args, dtype=torch.float32, **kw):
    from nas_segm_amd.data import create_depth_loaders

    _, dev = mods()
    torch.manual_seed(0)
    host = create_depth_loaders(args, **kw)
    torch.manual_seed(0)
    device = dev.create_device_depth_loaders(args, device=DEV, dtype=dtype, **kw)
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
        assert h["mask"].dtype == torch.float32
        assert equal(d["image"], h["image"].to(dtype)) and equal(d["mask"], h["mask"])
    return len(got)


@pytest.mark.parametrize("search", [True, False])
def test_depth_loaders_yield_the_host_batches(tmp_path, search):
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
    # the search script between tasks
    for loader in (h_trn, d_trn):
        loader.batch_sampler.batch_size = 3
        ds = loader.dataset.dataset if search else loader.dataset
        ds.set_config(24, 30)
        _set_stage(loader, "train")
    assert _epoch_equal(h_trn, d_trn, 5) == len(h_trn)
    batch = next(iter(d_trn))
    assert batch["image"].shape[2:] == (24, 24) and tuple(batch["mask"].shape) == (3, 24, 24)


def test_bf16_depth_loader_another_scale_and_no_zoom(tmp_path):
    args = _files(tmp_path, 8)
    (h_trn, _, _), (d_trn, _, _) = _both(args, torch.bfloat16, depth_scale=1.0 / 256)
    _epoch_equal(h_trn, d_trn, 3, torch.bfloat16)
    (h_trn, _, _), (d_trn, _, _) = _both(args, torch.bfloat16, zoom_depth=False)
    _epoch_equal(h_trn, d_trn, 4, torch.bfloat16)


def test_one_depth_epoch_and_validation_from_either_loader(tmp_path, monkeypatch):
    from nas_segm_amd.engine import trainer
    from nas_segm_amd.engine.inference import validate_depth
    from nas_segm_amd.nn import BerHuLoss

    monkeypatch.setenv("NASSEG_GRAPH", "0")
    args = _files(tmp_path, 12)
    genotype = [[[3, 0, 1], [4, 1, 1], [3, 1, 1]],
                [[0, 1, 0, 0, 1], [2, 1, 2, 1, 0], [3, 1, 1, 1, 0], [1, 1, 2, 0, 0],
                 [3, 0, 2, 0, 0], [5, 3, 2, 1, 0], [0, 5, 0, 1, 0]]]
    losses = []
    real_value = trainer._loss_value
    monkeypatch.setattr(trainer, "_loss_value", lambda s, loss: losses.append(real_value(s, loss)) or losses[-1])
    crit = BerHuLoss(valid_min=0.0)

    def run(train_loader, val_loader):
        del losses[:]
        net = build_product_net("template", genotype, 1, dict(agg_size=32, repeats=1), 0)
        segmenter = net.to(DEV)
        optim_enc = torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-5)
        optim_dec = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
        torch.manual_seed(4)
        np.random.seed(4)
        trainer.train_segmenter.__wrapped__(segmenter, train_loader, optim_enc, optim_dec, 0, crit, False, 3.0,
                                            3.0, False, print_every=100)
        reward = validate_depth.__wrapped__(segmenter, val_loader, 0, 0, min_depth=1e-3, max_depth=80.0,
                                            print_every=100, reward_fn=lambda sc: sc["rmse"])  # (never 0)
        return list(losses), {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, reward

    (h_trn, h_val, _), (d_trn, d_val, _) = _both(args)
    h_losses, h_sd, h_reward = run(h_trn, h_val)
    d_losses, d_sd, d_reward = run(d_trn, d_val)
    assert len(h_losses) == len(h_trn) > 0 and h_losses == d_losses
    assert all(np.isfinite(v) and v > 0 for v in h_losses)
    assert all(torch.equal(h_sd[k], d_sd[k]) for k in h_sd)
    assert h_reward == d_reward and np.isfinite(h_reward) and h_reward > 0


def test_augment_depth_argument_checks():
    """on the host, before any launch: nothing below reaches the kernel"""
    from nas_segm_amd import functional as F
    from nas_segm_amd._lib import NassegError

    _, dev = mods()
    sources = [sample(h, w, 100 + seed) for (h, w), seed in zip(SIZES, SEEDS[1.0])]
    _, plans = host_and_plans(pipeline(1.0), sources, SEEDS[1.0])
    batch = dev.collate_depth(plans)
    Ho, Wo = (int(v) for v in batch["size"])
    good = {k: batch[k].to(DEV) for k in ("src", "desc", "taps", "params")}
    good["lut"] = batch["lut"].to(torch.float32).to(DEV)

    def call(**kw):
        a = dict(good, **kw)
        return F.augment_depth(a["src"], a["desc"], a["taps"], a["lut"], a["params"], SCALE, Ho, Wo)

    image, target = call()
    assert tuple(image.shape) == (2, 3, Ho, Wo) and tuple(target.shape) == (2, Ho, Wo)
    wide_taps = torch.zeros((2, 2 * 9 * (Ho + Wo)), dtype=torch.int32, device=DEV)[:, ::2]
    assert not wide_taps.is_contiguous() and wide_taps.shape == good["taps"].shape
    bad = [
        dict(params=good["params"].double()), dict(params=good["params"].to(torch.bfloat16)),
        dict(params=good["params"][:1]), dict(params=good["params"].reshape(-1)),
        dict(params=torch.ones((2, 3), device=DEV)), dict(params=torch.ones((2, 4), device=DEV)[:, ::2]),
        dict(taps=wide_taps), dict(taps=good["taps"].long()),
        dict(desc=good["desc"][:0], taps=good["taps"][:0], params=good["params"][:0]),  # B = 0
        dict(lut=good["lut"].double()), dict(src=good["src"].to(torch.int8)),
        dict(params=good["params"].cpu()),
    ]
    for kw in bad:
        with pytest.raises(NassegError):
            call(**kw)
    with pytest.raises(NassegError):
        F.augment_depth(good["src"], good["desc"], good["taps"], good["lut"], good["params"], SCALE, Ho, Wo + 1)
