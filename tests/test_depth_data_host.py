"""Depth targets in the data pipelines, no GPU: 16-bit depth files (``_load_depth``), the zoom that divides its target
(``DepthResizeScale``), ``create_depth_loaders``, and the host half of the device path (``plan_depth_sample``,
``collate_depth``).  Every comparison is exact: both sides make the same correctly rounded fp32 operations on the
same integers.

A small numpy executor below does with a packed depth batch what nasseg_augment_depth does with its target half:
gather the little-endian counts by the nearest indices, one fp32 product, one fp32 quotient, the fill - undivided -
where an index is -1."""
import types

import numpy as np
import pytest
import torch

MEAN = np.array([0.485, 0.456, 0.406]).reshape((1, 1, 3))
STD = np.array([0.229, 0.224, 0.225]).reshape((1, 1, 3))
SCALE = 1e-3


def mods():
    from nas_segm_amd.data import datasets, device

    return datasets, device


def sample(h, w, seed):
    """a uint8 image and uint16 counts that hold holes (0), the largest count and everything between"""
    rng = np.random.RandomState(seed)
    img = (rng.rand(h, w, 3) * 255).astype(np.uint8)
    counts = rng.randint(0, 65536, (h, w)).astype(np.uint16)
    counts[rng.rand(h, w) < 0.1] = 0
    counts[rng.rand(h, w) < 0.1] = 65535
    return img, counts


def metres(counts, scale=SCALE):
    return counts.astype(np.float32) * np.float32(scale)


def states_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def save_png(path, arr):
    from PIL import Image

    Image.fromarray(arr).save(str(path))


# ---------------------------------------------------------------------------------------------------------------
# 1. _load_depth
# ---------------------------------------------------------------------------------------------------------------
def test_load_depth_round_trip_and_refusals(tmp_path):
    from PIL import Image

    D, _ = mods()
    _, counts = sample(23, 31, 0)
    counts[0, :2] = (0, 65535)
    save_png(tmp_path / "d.png", counts)
    assert np.array(Image.open(str(tmp_path / "d.png"))).dtype == np.uint16
    for scale in (1e-3, 1.0 / 256, 0.25):
        got = D._load_depth(str(tmp_path / "d.png"), scale)
        assert got.dtype == np.float32 and got.shape == counts.shape
        assert np.array_equal(got, counts.astype(np.float32) * np.float32(scale))
        assert got[0, 0] == 0.0 and got[0, 1] == np.float32(65535) * np.float32(scale)
    # mode I (int32) within the 16-bit range is taken as well
    Image.fromarray(counts.astype(np.int32)).save(str(tmp_path / "i.tif"))
    assert np.array(Image.open(str(tmp_path / "i.tif"))).dtype == np.int32
    assert np.array_equal(D._load_depth(str(tmp_path / "i.tif"), SCALE), metres(counts))
    # refused: an RGB file, a uint8 file, int32 values outside [0, 65535], floats
    save_png(tmp_path / "rgb.png", np.zeros((5, 6, 3), np.uint8))
    save_png(tmp_path / "u8.png", np.zeros((5, 6), np.uint8))
    big = counts.astype(np.int32)
    big[3, 3] = 70000
    Image.fromarray(big).save(str(tmp_path / "big.tif"))
    neg = counts.astype(np.int32)
    neg[3, 3] = -1
    Image.fromarray(neg).save(str(tmp_path / "neg.tif"))
    Image.fromarray(counts.astype(np.float32)).save(str(tmp_path / "f.tif"))
    for name in ("rgb.png", "u8.png", "big.tif", "neg.tif", "f.tif"):
        with pytest.raises(ValueError) as err:
            D._load_depth(str(tmp_path / name), SCALE)
        assert name in str(err.value)


# ---------------------------------------------------------------------------------------------------------------
# 2. DepthResizeScale
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("longer", [False, True])
def test_depth_resize_scale_is_resize_scale_with_a_divided_target(longer):
    D, _ = mods()
    img, counts = sample(37, 53, 1)
    m = metres(counts)
    limited = set()
    # shorter side 37, longer side 53: resize_side 30 never limits the shorter side at scales >= 0.9 and always
    # limits the longer one; resize_side 60 the other way round
    for resize_side in (30, 60):
        for seed in range(6):
            plain, deep = (cls(resize_side, 0.9, 1.5, longer) for cls in (D.ResizeScale, D.DepthResizeScale))
            np.random.seed(seed)
            want_img, want_msk = plain.apply(img, m)
            state = np.random.get_state()
            np.random.seed(seed)
            got_img, got_msk = deep.apply(img, m)
            assert states_equal(np.random.get_state(), state)
            np.random.seed(seed)
            drawn = np.random.uniform(0.9, 1.5)
            side = 53 if longer else 37
            fires = side * drawn > resize_side if longer else side * drawn < resize_side
            s = resize_side * 1.0 / side if fires else drawn
            limited.add(bool(fires))
            assert np.array_equal(got_img, want_img) and got_img.dtype == np.uint8
            assert got_msk.dtype == np.float32 and got_msk.shape == want_msk.shape
            assert np.array_equal(got_msk, D.resize_nearest(m, s) / np.float32(s))
            assert np.array_equal(want_msk, D.resize_nearest(m, s))  # (the plain one does not divide)
            assert np.all(got_msk[want_msk == 0] == 0)               # holes stay holes
            if fires:
                assert not np.array_equal(got_msk, D.resize_nearest(m, drawn) / np.float32(drawn))
    assert limited == {False, True}
    assert issubclass(D.DepthResizeScale, D.ResizeScale)


def test_the_untouched_operations_carry_a_float32_target():
    D, _ = mods()
    img, counts = sample(37, 53, 2)
    pipe = D.Compose([D.DepthResizeScale(20, 1.37, 1.37), D.Pad(90, (1, 2, 3), 7.5), D.RandomMirror(),
                      D.RandomCrop(48), D.Normalise(1.0 / 255, MEAN, STD), D.ToTensor()])
    np.random.seed(0)
    out = pipe({"image": img, "mask": metres(counts)})
    assert out["mask"].dtype == torch.float32 and tuple(out["mask"].shape) == (48, 48)
    assert tuple(out["image"].shape) == (3, 48, 48)


# ---------------------------------------------------------------------------------------------------------------
# 3. create_depth_loaders
# ---------------------------------------------------------------------------------------------------------------
def _files(tmp_path, n):
    sources = []
    lines = []
    for i in range(n):
        img, counts = sample(50 + 3 * i, 70 - 2 * i, 10 + i)
        save_png(tmp_path / "i{}.png".format(i), img)
        save_png(tmp_path / "d{}.png".format(i), counts)
        lines.append("i{0}.png\td{0}.png\n".format(i))
        sources.append((img, counts))
    (tmp_path / "train.lst").write_text("".join(lines))
    (tmp_path / "val.lst").write_text("".join(lines[:4]))
    args = types.SimpleNamespace(
        train_dir=str(tmp_path), val_dir=str(tmp_path), train_list=str(tmp_path / "train.lst"),
        val_list=str(tmp_path / "train.lst"), meta_train_prct=80, resize_side=[40], low_scale=0.7, high_scale=1.4,
        resize_longer_side=False, crop_size=[32], val_resize_side=40, val_crop_size=32,
        normalise_params=[1.0 / 255, MEAN, STD], batch_size=[4], val_batch_size=2, num_workers=0)
    return args, sources


def _stage(loader, stage):
    ds = loader.dataset
    (ds.dataset if hasattr(ds, "dataset") else ds).set_stage(stage)


def test_create_depth_loaders_search_split_and_batches(tmp_path):
    from nas_segm_amd.data import create_depth_loaders, create_loaders
    from torch.utils.data import random_split

    D, _ = mods()
    args, _ = _files(tmp_path, 10)
    torch.manual_seed(3)
    trn, val, do_search = create_depth_loaders(args)
    state = torch.random.get_rng_state()
    torch.manual_seed(3)
    want = random_split(list(range(10)), [8, 2])
    assert torch.equal(torch.random.get_rng_state(), state)  # one random_split draw
    torch.manual_seed(3)
    seg_trn, _, _ = create_loaders(args)  # the segmentation loaders split the list the same way
    assert do_search and trn.dataset.dataset is val.dataset.dataset
    assert list(trn.dataset.indices) == list(want[0].indices) == list(seg_trn.dataset.indices)
    assert list(val.dataset.indices) == list(want[1].indices)
    ds = trn.dataset.dataset
    assert isinstance(ds, D.DepthDataset) and ds.depth_scale == 1e-3
    kinds = [type(op) for op in ds.transform_trn.transforms]
    assert kinds == [D.DepthResizeScale, D.RandomMirror, D.RandomCrop, D.Normalise, D.ToTensor]
    assert [type(op) for op in ds.transform_val.transforms] == [D.ResizeScale, D.CentralCrop, D.Normalise, D.ToTensor]
    assert len(trn) == 2 and len(val) == 1 and trn.drop_last and val.drop_last
    torch.manual_seed(0)
    np.random.seed(0)
    batches = list(trn)
    assert len(batches) == 2
    for b in batches:
        assert b["image"].dtype == torch.float64 and tuple(b["image"].shape) == (4, 3, 32, 32)
        assert b["mask"].dtype == torch.float32 and tuple(b["mask"].shape) == (4, 32, 32)
    # the search script between tasks: set_config, then an epoch at the new crop
    ds.set_config(24, 30)
    assert ds.transform_trn.transforms[0].resize_side == 30 and ds.transform_trn.transforms[2].crop_size == 24
    b = next(iter(trn))
    assert tuple(b["image"].shape) == (4, 3, 24, 24) and tuple(b["mask"].shape) == (4, 24, 24)
    assert b["mask"].dtype == torch.float32
    # zoom_depth=False: the plain ResizeScale at position 0
    trn0, _, _ = create_depth_loaders(args, zoom_depth=False)
    assert type(trn0.dataset.dataset.transform_trn.transforms[0]) is D.ResizeScale


def test_create_depth_loaders_separate_lists_and_true_metres_in_validation(tmp_path):
    from nas_segm_amd.data import create_depth_loaders

    D, _ = mods()
    args, sources = _files(tmp_path, 6)
    args.val_list = str(tmp_path / "val.lst")
    args.val_resize_side = 80  # every file's shorter side is below 80: the validation resize enlarges
    args.val_crop_size = 64
    trn, val, do_search = create_depth_loaders(args, depth_scale=1.0 / 256)
    assert not do_search and trn.dataset is not val.dataset and len(trn.dataset) == 6 and len(val.dataset) == 4
    assert val.dataset.transform_trn is None and val.dataset.depth_scale == 1.0 / 256
    _stage(val, "val")
    got = torch.cat([b["mask"] for b in val])
    assert got.dtype == torch.float32 and tuple(got.shape) == (4, 64, 64)
    for i in range(4):
        img, counts = sources[i]
        s = 80 * 1.0 / min(counts.shape)
        m = D.resize_nearest(metres(counts, 1.0 / 256), s)  # plain nearest-resized metres: never divided
        assert s > 1.0 and m.shape[0] >= 64 and m.shape[1] >= 64
        top, left = (m.shape[0] - 64) // 2, (m.shape[1] - 64) // 2
        assert np.array_equal(got[i].numpy(), m[top: top + 64, left: left + 64])
    # a single-column list has no depth files
    (tmp_path / "one.lst").write_text("i0.png\ni1.png\n")
    with pytest.raises(ValueError):
        D.DepthDataset(str(tmp_path / "one.lst"), str(tmp_path))
    # no pipeline (another stage): the raw arrays
    ds = D.DepthDataset(args.val_list, args.val_dir)
    raw = ds[2]
    assert np.array_equal(raw["image"], sources[2][0]) and np.array_equal(raw["mask"], metres(sources[2][1]))


# ---------------------------------------------------------------------------------------------------------------
# 4. plan_depth_sample / collate_depth
# ---------------------------------------------------------------------------------------------------------------
def execute_target(batch, depth_scale):
    """numpy model of the target half of nasseg_augment_depth on a collated depth batch -> float32 B x Ho x Wo"""
    src, desc, taps, params = (batch[k].numpy() for k in ("src", "desc", "taps", "params"))
    assert src.dtype == np.uint8 and params.dtype == np.float32 and params.shape == (desc.shape[0], 2)
    Ho, Wo = (int(v) for v in batch["size"])
    out = []
    for b in range(desc.shape[0]):
        _, mo, h, w, _, mld, _, _ = (int(v) for v in desc[b])
        assert mld >= 2 * w and mo + (h - 1) * mld + 2 * w <= src.size
        rows = np.stack([src[mo + y * mld: mo + y * mld + 2 * w] for y in range(h)]).astype(np.int64)
        counts = rows[:, 0::2] | (rows[:, 1::2] << 8)  # two byte loads, little endian
        t = taps[b]
        my, mx = t[8 * (Ho + Wo): 8 * (Ho + Wo) + Ho], t[8 * (Ho + Wo) + Ho:]
        live = (my >= 0)[:, None] & (mx >= 0)[None, :]
        zoom, fill = params[b]
        gathered = counts[np.maximum(my, 0)][:, np.maximum(mx, 0)].astype(np.float32)
        value = (gathered * np.float32(depth_scale)) / zoom
        assert value.dtype == np.float32
        out.append(np.where(live, value, fill).astype(np.float32))
    return np.stack(out)


def _pipe(D, s, fill=7.5, pad=True, zoom=True):
    resize = (D.DepthResizeScale if zoom else D.ResizeScale)(20, s, s)
    ops = [resize] + ([D.Pad(60, (124.4, 116, 104), fill)] if pad else []) + [
        D.RandomMirror(), D.RandomCrop(48), D.Normalise(1.0 / 255, MEAN, STD), D.ToTensor()]
    return D.Compose(ops)


def test_plan_depth_sample_against_the_host_pipeline():
    D, dev = mods()
    seen = {"fill": 0, "live": 0, "odd": 0}
    cases = [(s, pad, zoom, fill) for s in (0.5, 1.0, 1.37, 2.0)
             for pad, zoom, fill in ((True, True, 7.5), (True, True, 0), (False, True, 0), (True, False, 3))]
    for s, pad, zoom, fill in cases:
        pipe = _pipe(D, s, fill, pad, zoom)
        plans, want = [], []
        for k, (h, w) in enumerate(((37, 53), (41, 65))):
            img, counts = sample(h, w, 20 + k)
            np.random.seed(k)
            want.append(pipe({"image": img, "mask": metres(counts)}))
            state = np.random.get_state()
            np.random.seed(k)
            p = dev.plan_depth_sample(pipe, img, counts)
            assert states_equal(np.random.get_state(), state)
            plans.append(p)
            # the image half is the label-map planner's: same window, taps, fill and table (what nasseg_augment
            # makes of them is tests/test_device_augment_plan.py's subject)
            np.random.seed(k)
            q = dev.plan_sample(pipe, img, np.zeros((h, w), np.uint8))
            assert np.array_equal(p["image"], q["image"]) and np.array_equal(p["taps"], q["taps"])
            assert p["fill"][0] == q["fill"][0] and np.array_equal(p["lut"], q["lut"]) and p["size"] == q["size"]
            assert p["mask"].dtype == np.dtype("<u2") and p["image"].shape[:2] == p["mask"].shape
            limited = 20 * 1.0 / min(h, w) if min(h, w) * s < 20 else s  # (37 x 53 at 0.5: the limit fires)
            assert p["params"].dtype == np.float32
            assert p["params"][0] == (np.float32(limited) if zoom else np.float32(1.0))
            assert p["params"][1] == (np.float32(fill) if pad else np.float32(0.0))
        if plans[0]["size"] != plans[1]["size"]:  # (without a pad a small sample can stay below the crop)
            batches = [dev.collate_depth([p]) for p in plans]
        else:
            batches = [dev.collate_depth(plans)]
        got = [t for b in batches for t in execute_target(b, SCALE)]
        for b, host in enumerate(want):
            assert np.array_equal(got[b], host["mask"].numpy()), (s, pad, zoom, b)
        seen["odd"] += sum(int((b["desc"][:, 1] % 2).sum()) for b in batches)
        if pad and fill:
            seen["fill"] += sum(int((t == np.float32(fill)).sum()) for t in got)
            seen["live"] += sum(int((t != np.float32(fill)).sum()) for t in got)
    # between them the cases unpacked count windows that start at an odd byte (a window of odd height and width is
    # 3 h w = an odd number of image bytes), wrote fill and gathered counts
    assert seen["odd"] > 0 and seen["live"] > 0 and seen["fill"] > 0


def test_plan_depth_sample_refusals_and_the_uint8_planner_stays_closed():
    D, dev = mods()
    pipe = _pipe(D, 1.0)
    img, counts = sample(37, 53, 3)
    for bad in (counts.astype(np.uint8), metres(counts), counts.astype(np.int32), counts[:-1], counts[:, :, None],
                counts.tolist()):
        with pytest.raises(ValueError) as err:
            dev.plan_depth_sample(pipe, img, bad)
        assert "depth target" in str(err.value)
    with pytest.raises(ValueError):
        dev.plan_depth_sample(pipe, img.astype(np.float32), counts)
    with pytest.raises(ValueError):
        dev.plan_depth_sample(pipe, img[:, :, :1], counts)
    # the label-map planner keeps refusing everything that is not uint8
    with pytest.raises(ValueError):
        dev.plan_sample(pipe, img, counts)
    with pytest.raises(ValueError):
        dev.plan_sample(pipe, img, metres(counts))
    # check_pipeline's rules hold for the new resize
    norm, tt = D.Normalise(1.0 / 255, MEAN, STD), D.ToTensor()
    for ops in ([D.DepthResizeScale(10, 1, 2), D.ResizeShorter(20), norm, tt],
                [D.ResizeScale(10, 1, 2), D.DepthResizeScale(10, 1, 2), norm, tt],
                [D.RandomCrop(20), D.DepthResizeScale(10, 1, 2), norm, tt],
                [D.Pad(40, (0, 0, 0), 0), D.DepthResizeScale(10, 1, 2), norm, tt]):
        with pytest.raises(ValueError):
            dev.check_pipeline(D.Compose(ops))
    dev.check_pipeline(pipe)


def test_device_depth_dataset_plans_what_the_host_dataset_computes(tmp_path):
    D, dev = mods()
    from nas_segm_amd.data import loaders as L

    args, _ = _files(tmp_path, 5)
    torch.manual_seed(1)
    h_trn, h_val, _ = L.create_depth_loaders(args, depth_scale=0.002)
    torch.manual_seed(1)
    d_trn, d_val, do_search = dev.create_device_depth_loaders(args, depth_scale=0.002)
    assert do_search and len(d_trn) == len(h_trn) and len(d_val) == len(h_val)
    assert list(d_trn.dataset.indices) == list(h_trn.dataset.indices)
    assert isinstance(d_trn, dev.DeviceDepthLoader) and d_trn.depth_scale == 0.002
    host, devd = h_trn.dataset.dataset, d_trn.dataset.dataset
    assert isinstance(devd, dev.DeviceDepthDataset) and isinstance(devd, D.DepthDataset)
    for stage, crop in (("train", 32), ("val", 32), ("train", 20)):
        for ds in (host, devd):
            ds.set_stage(stage)
            if crop == 20:
                ds.set_config(20, 30)
        for i in range(5):
            np.random.seed(i)
            want = host[i]
            state = np.random.get_state()
            np.random.seed(i)
            got = execute_target(dev.collate_depth([devd[i]]), 0.002)
            assert states_equal(np.random.get_state(), state)
            assert got.shape[1:] == (crop, crop) and np.array_equal(got[0], want["mask"].numpy())
    with pytest.raises(ValueError):
        dev.DeviceDepthLoader(d_trn.loader, dtype=torch.float16)
