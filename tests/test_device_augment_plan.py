"""The host half of the device augmentation (data/device.py), no GPU: plans, tables and packed batches.

A small numpy executor below does what csrc/augment.hip does with a packed batch (integer bicubic from the tap
tables, nearest mask, the Normalise table); for every pipeline it must give the host pipeline's float64 output
bit for bit and leave ``np.random`` where the host pipeline leaves it."""
import types

import numpy as np
import pytest
import torch

from _util import load_npz

NPZ = load_npz("data.npz")
MEAN = np.array([0.485, 0.456, 0.406]).reshape((1, 1, 3))
STD = np.array([0.229, 0.224, 0.225]).reshape((1, 1, 3))


def mods():
    from nas_segm_amd.data import datasets, device

    return datasets, device


def execute(batch):
    """numpy model of nasseg_augment on a collated batch -> (float64 B x 3 x Ho x Wo, uint8 B x Ho x Wo)"""
    src, desc, taps, lut = (batch[k].numpy() for k in ("src", "desc", "taps", "lut"))
    Ho, Wo = (int(v) for v in batch["size"])
    images, masks = [], []
    for b in range(desc.shape[0]):
        io, mo, h, w, ild, mld, ifill, mfill = (int(v) for v in desc[b])
        img = src[io: io + h * ild].reshape(h, w, 3).astype(np.int64)
        msk = src[mo: mo + h * mld].reshape(h, w)
        t = taps[b]
        ty, tx = t[:8 * Ho].reshape(Ho, 8), t[8 * Ho: 8 * (Ho + Wo)].reshape(Wo, 8)
        my, mx = t[8 * (Ho + Wo): 8 * (Ho + Wo) + Ho], t[8 * (Ho + Wo) + Ho:]
        live = (ty[:, 0] >= 0)[:, None] & (tx[:, 0] >= 0)[None, :]
        yi, xi = np.maximum(ty[:, :4], 0), np.maximum(tx[:, :4], 0)
        rows = sum(img[:, xi[:, j], :] * tx[None, :, 4 + j, None] for j in range(4))  # h x Wo x 3
        out = sum(rows[yi[:, k], :, :] * ty[:, 4 + k, None, None].astype(np.int64) for k in range(4))
        v = np.clip((out + (1 << 21)) >> 22, 0, 255)
        fill = np.array([ifill & 255, (ifill >> 8) & 255, (ifill >> 16) & 255])
        v = np.where(live[:, :, None], v, fill[None, None, :])
        images.append(np.stack([lut[c][v[:, :, c]] for c in range(3)]))
        mlive = (my >= 0)[:, None] & (mx >= 0)[None, :]
        masks.append(np.where(mlive, msk[np.maximum(my, 0)][:, np.maximum(mx, 0)], mfill).astype(np.uint8))
    return np.stack(images), np.stack(masks)


def host_run(pipeline, image, mask, seed):
    np.random.seed(seed)
    out = pipeline({"image": image, "mask": mask})
    return out["image"].numpy(), out["mask"].numpy(), np.random.get_state()


def device_run(pipeline, image, mask, seed):
    _, dev = mods()
    np.random.seed(seed)
    s = dev.plan_sample(pipeline, image, mask)
    state = np.random.get_state()
    img, msk = execute(dev.collate([s]))
    return img[0], msk[0], state, s


def states_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def check(pipeline, image, mask, seed):
    hi, hm, hs = host_run(pipeline, image, mask, seed)
    di, dm, ds, s = device_run(pipeline, image, mask, seed)
    assert hi.dtype == np.float64 and hi.shape == di.shape and np.array_equal(hi, di)
    assert hm.shape == dm.shape and np.array_equal(hm, dm)
    assert states_equal(hs, ds)
    return s


def sample(h, w, seed, grey=False):
    rng = np.random.RandomState(seed)
    img = (rng.rand(h, w) if grey else rng.rand(h, w, 3)) * 255
    img = img.astype(np.uint8)
    if grey:  # (what _load_rgb makes of a grey-scale file)
        img = np.repeat(img[:, :, None], 3, axis=2)
    return img, (rng.rand(h, w) * 21).astype(np.uint8)


def args(**kw):
    a = dict(resize_side=[40], low_scale=0.7, high_scale=1.4, resize_longer_side=False, crop_size=[32],
             val_resize_side=40, val_crop_size=32, normalise_params=[1.0 / 255, MEAN, STD])
    a.update(kw)
    return types.SimpleNamespace(**a)


def pipelines(a):
    from nas_segm_amd.data import loaders as L

    return L._pipeline(L._TRAIN_OPS, a), L._pipeline(L._VAL_OPS, a)


@pytest.mark.parametrize("longer", [False, True])
def test_loader_pipelines_over_many_seeds(longer):
    trn, val = pipelines(args(resize_longer_side=longer))
    for seed in range(40):
        img, msk = sample(45 + seed % 7, 61 - seed % 5, seed)
        check(trn, img, msk, seed)
        check(val, img, msk, 1000 + seed)


@pytest.mark.parametrize("scale", [0.3, 0.5, 0.77, 1.0, 1.37, 2.0, 2.5])
def test_scales(scale):
    D, _ = mods()
    norm = D.Normalise(1.0 / 255, MEAN, STD)
    img, msk = sample(53, 38, 5)
    for crop in (16, 48, 200):
        pipe = D.Compose([D.ResizeScale(10, scale, scale), D.RandomMirror(), D.RandomCrop(crop), norm, D.ToTensor()])
        for seed in range(6):
            check(pipe, img, msk, seed)


def test_both_mirror_outcomes():
    D, _ = mods()
    pipe = D.Compose([D.RandomMirror(), D.Normalise(1.0 / 255, MEAN, STD), D.ToTensor()])
    img, msk = sample(20, 31, 2)
    flips = set()
    for seed in range(12):
        check(pipe, img, msk, seed)
        np.random.seed(seed)
        flips.add(np.random.randint(2))
    assert flips == {0, 1}


def test_crops_larger_than_the_image_and_a_negative_central_top():
    D, _ = mods()
    norm = D.Normalise(1.0 / 255, MEAN, STD)
    img, msk = sample(21, 33, 3)
    for ops in ([D.RandomCrop(64)], [D.CentralCrop(40)], [D.CentralCrop(26)],
                [D.ResizeScale(10, 0.5, 0.5), D.CentralCrop(30)], [D.ResizeScale(10, 1.6, 1.6), D.RandomCrop(100)]):
        check(D.Compose(ops + [norm, D.ToTensor()]), img, msk, 7)


@pytest.mark.parametrize("fill", [(0, 0, 0), (124.9, 116, 104), (255, 1, 17)])
def test_pad_after_a_resize(fill):
    D, _ = mods()
    img, msk = sample(29, 44, 4)
    pipe = D.Compose([D.ResizeScale(10, 0.6, 1.8), D.Pad(70, fill, 255), D.RandomMirror(), D.RandomCrop(60),
                      D.Normalise(1.0 / 255, MEAN, STD), D.ToTensor()])
    for seed in range(8):
        check(pipe, img, msk, seed)
    pipe = D.Compose([D.ResizeShorter(40), D.Pad(51, fill, 7), D.CentralCrop(50), D.Normalise(1.0 / 255, MEAN, STD),
                      D.ToTensor()])
    check(pipe, img, msk, 0)


def test_grey_scale_inputs_and_the_golden_dataset_pipelines():
    D, _ = mods()
    norm = D.Normalise(1.0 / 255, MEAN, STD)
    trn = D.Compose([D.ResizeShorter(16), D.CentralCrop(30), D.RandomCrop(24), norm, D.ToTensor()])
    val = D.Compose([D.CentralCrop(32), norm, D.ToTensor()])
    img, msk = sample(40, 36, 6, grey=True)
    for pipe in pipelines(args()) + (trn, val):
        check(pipe, img, msk, 3)
    for i in range(3):
        img = NPZ["file{}/image".format(i)]
        if img.ndim == 2:
            img = np.repeat(img[:, :, None], 3, axis=2)
        for pipe in (trn, val):
            check(pipe, img, NPZ["file{}/mask".format(i)], 9 + i)


def test_set_config_between_calls(tmp_path):
    from PIL import Image

    D, dev = mods()
    for i in range(3):
        img, msk = sample(50 + 4 * i, 70 - 3 * i, i)
        Image.fromarray(img).save(str(tmp_path / "i{}.png".format(i)))
        Image.fromarray(msk).save(str(tmp_path / "m{}.png".format(i)))
    (tmp_path / "l.lst").write_text("".join("i{0}.png\tm{0}.png\n".format(i) for i in range(3)))
    a = args()
    host = D.PascalCustomDataset(str(tmp_path / "l.lst"), str(tmp_path), *pipelines(a))
    devd = dev.DevicePascalDataset(str(tmp_path / "l.lst"), str(tmp_path), *pipelines(a))
    for crop, side in ((32, 40), (20, 30), (44, 66)):
        for ds in (host, devd):
            ds.set_config(crop, side)
        for i in range(3):
            np.random.seed(i)
            h = host[i]
            np.random.seed(i)
            img, msk = execute(dev.collate([devd[i]]))
            assert np.array_equal(h["image"].numpy(), img[0]) and np.array_equal(h["mask"].numpy(), msk[0])
            assert img.shape[2:] == (crop, crop)


def test_batches_pack_and_unpack():
    D, dev = mods()
    trn, _ = pipelines(args())
    samples, want = [], []
    for i in range(5):
        img, msk = sample(44 + i, 50 + 2 * i, i)
        hi, hm, _ = host_run(trn, img, msk, i)
        want.append((hi, hm))
        np.random.seed(i)
        samples.append(dev.plan_sample(trn, img, msk))
    batch = dev.collate(samples)
    assert batch["src"].dtype == torch.uint8 and batch["desc"].shape == (5, dev.DESC_FIELDS)
    img, msk = execute(batch)
    for b, (hi, hm) in enumerate(want):
        assert np.array_equal(img[b], hi) and np.array_equal(msk[b], hm)
    np.random.seed(0)
    odd = dev.plan_sample(D.Compose([D.CentralCrop(20), trn.transforms[3], D.ToTensor()]), *sample(30, 30, 0))
    with pytest.raises(RuntimeError):
        dev.collate(samples[:2] + [odd])


def test_the_upload_is_only_the_window_the_taps_reach():
    D, dev = mods()
    img, msk = sample(512, 1024, 1)
    for seed in range(10):
        trn, val = pipelines(args(resize_side=[300], crop_size=[160], val_resize_side=300, val_crop_size=256))
        for pipe in (trn, val):
            np.random.seed(seed)
            s = dev.plan_sample(pipe, img, msk)
            Ho, Wo = s["size"]
            t = s["taps"]
            ty, tx = t[:8 * Ho].reshape(Ho, 8), t[8 * Ho: 8 * (Ho + Wo)].reshape(Wo, 8)
            my, mx = t[8 * (Ho + Wo): 8 * (Ho + Wo) + Ho], t[8 * (Ho + Wo) + Ho:]
            h, w = s["mask"].shape
            assert s["image"].shape == (h, w, 3)
            # every row / column of the window is reached, and nothing outside it is
            assert set(np.r_[ty[:, :4].ravel(), my]) == set(range(h))
            assert set(np.r_[tx[:, :4].ravel(), mx]) <= set(range(w)) and tx[:, :4].min() == 0
            assert max(tx[:, :4].max(), mx.max()) == w - 1
            assert h * w < 0.5 * img.shape[0] * img.shape[1]


def test_refused_pipelines_raise_when_built(tmp_path):
    D, dev = mods()
    (tmp_path / "l.lst").write_text("a.png\tb.png\n")
    norm, tt = D.Normalise(1.0 / 255, MEAN, STD), D.ToTensor()

    class Blur(D.SampleOp):
        def apply(self, image, mask):
            return image, mask

    bad = [
        [D.ResizeScale(10, 1, 2), D.ResizeShorter(20), norm, tt],           # two resizes
        [D.RandomCrop(20), D.ResizeScale(10, 1, 2), norm, tt],              # a resize after a window op
        [D.RandomMirror(), D.ResizeShorter(20), norm, tt],
        [D.Pad(40, (0, 0, 0), 255), D.ResizeShorter(20), norm, tt],
        [D.RandomCrop(20), tt],                                             # no Normalise
        [D.RandomCrop(20), norm],                                           # no ToTensor
        [norm, D.RandomCrop(20), tt],                                       # Normalise not last
        [D.RandomCrop(20), tt, norm],
        [Blur(), D.RandomCrop(20), norm, tt],                               # unknown operation
    ]
    for ops in bad:
        with pytest.raises(ValueError):
            dev.DevicePascalDataset(str(tmp_path / "l.lst"), str(tmp_path), D.Compose(ops), None)
        with pytest.raises(ValueError):
            dev.DevicePascalDataset(str(tmp_path / "l.lst"), str(tmp_path), None, D.Compose(ops))
    dev.DevicePascalDataset(str(tmp_path / "l.lst"), str(tmp_path), *pipelines(args()))


def test_refused_samples_raise_when_they_arrive(tmp_path):
    from PIL import Image

    D, dev = mods()
    trn, val = pipelines(args())
    img, msk = sample(40, 40, 0)
    for image, mask in ((img.astype(np.float32), msk), (np.concatenate([img, img[:, :, :1]], 2), msk),
                        (img, msk.astype(np.int32)), (img, msk[:-1])):
        with pytest.raises(ValueError):
            dev.plan_sample(trn, image, mask)
    # through the dataset: an RGBA file, and a grey-scale file that works
    Image.fromarray(np.concatenate([img, img[:, :, :1]], 2)).save(str(tmp_path / "rgba.png"))
    Image.fromarray(img[:, :, 0]).save(str(tmp_path / "grey.png"))
    Image.fromarray(msk).save(str(tmp_path / "m.png"))
    (tmp_path / "l.lst").write_text("rgba.png\tm.png\ngrey.png\tm.png\n")
    ds = dev.DevicePascalDataset(str(tmp_path / "l.lst"), str(tmp_path), trn, val)
    with pytest.raises(ValueError):
        ds[0]
    np.random.seed(0)
    out = execute(dev.collate([ds[1]]))
    host = D.PascalCustomDataset(str(tmp_path / "l.lst"), str(tmp_path), trn, val)
    np.random.seed(0)
    h = host[1]
    assert np.array_equal(out[0][0], h["image"].numpy()) and np.array_equal(out[1][0], h["mask"].numpy())


def test_loader_forwards_what_the_search_script_touches(tmp_path):
    from PIL import Image

    _, dev = mods()
    for i in range(6):
        img, msk = sample(50, 60, i)
        Image.fromarray(img).save(str(tmp_path / "i{}.png".format(i)))
        Image.fromarray(msk).save(str(tmp_path / "m{}.png".format(i)))
    (tmp_path / "l.lst").write_text("".join("i{0}.png\tm{0}.png\n".format(i) for i in range(6)))
    a = args(train_dir=str(tmp_path), val_dir=str(tmp_path), train_list=str(tmp_path / "l.lst"),
             val_list=str(tmp_path / "l.lst"), meta_train_prct=50, batch_size=[2], val_batch_size=1, num_workers=0)
    trn, val, do_search = dev.create_device_loaders(a)
    assert do_search and len(trn) == 1 and len(val) == 3
    trn.batch_sampler.batch_size = 1
    assert len(trn) == 3
    trn.dataset.dataset.set_config(20, 30)
    assert trn.dataset.dataset.transform_trn.transforms[2].crop_size == 20
    with pytest.raises(ValueError):
        dev.DeviceLoader(trn.loader, dtype=torch.float16)


def test_install_dropin_data_on_device():
    import os
    import subprocess
    import sys

    code = ("import nas_segm_amd; names = nas_segm_amd.install_dropin(data_on_device=True);"
            "from data.loaders import create_loaders;"
            "from nas_segm_amd.data import device; assert create_loaders is device.create_loaders;"
            "nas_segm_amd.install_dropin(data=True);"
            "from data.loaders import create_loaders as host;"
            "from nas_segm_amd.data import loaders; assert host is loaders.create_loaders; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
