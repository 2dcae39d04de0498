"""ColourJitter on the host (data/datasets.py) and its device plan (data/device.py), no GPU.

The jitter is defined in integers and host-made tables: a 12-bit fixed-point colour matrix (saturation, hue) and a
256-entry point table (brightness, contrast, gamma).  The tests restate both independently (Python integers, Python
floats), pin the order of the ``np.random`` draws, and run a numpy executor of the colour launch (what
csrc/augment.hip does with a packed batch) against the host pipeline: same float64 batches bit for bit, same
``np.random`` state afterwards."""
import math
import types

import numpy as np
import pytest
import torch

MEAN = np.array([0.485, 0.456, 0.406]).reshape((1, 1, 3))
STD = np.array([0.229, 0.224, 0.225]).reshape((1, 1, 3))
YIQ = [[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]]


def mods():
    from nas_segm_amd.data import datasets, device

    return datasets, device


def norm_ops():
    D, _ = mods()
    return [D.Normalise(1.0 / 255, MEAN, STD), D.ToTensor()]


def sample(h, w, seed):
    rng = np.random.RandomState(seed)
    return (rng.rand(h, w, 3) * 255).astype(np.uint8), (rng.rand(h, w) * 21).astype(np.uint8)


def states_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ---------------------------------------------------------------------------
# independent restatements
# ---------------------------------------------------------------------------
def matrix_restated(s, h):
    """rint(4096 inv(T) R T) with the product written out"""
    T = np.array(YIQ, np.float64)
    co, si = s * math.cos(2 * math.pi * h), s * math.sin(2 * math.pi * h)
    R = np.array([[1, 0, 0], [0, co, -si], [0, si, co]], np.float64)
    return np.rint(4096 * np.linalg.inv(T).dot(R).dot(T)).astype(np.int64)


def pixel_restated(Mq, v):
    """one pixel through the matrix in Python integers (// 4096 floors: the arithmetic shift)"""
    return [min(max((sum(int(Mq[c][k]) * int(v[k]) for k in range(3)) + 2048) // 4096, 0), 255) for c in range(3)]


def table_restated(b, c, g):
    out = []
    for v in range(256):
        x = v + 255.0 * b
        x = (x - 128.0) * c + 128.0
        x = 255.0 * (min(max(x, 0.0), 255.0) / 255.0) ** g
        out.append(int(min(max(round(x), 0), 255)))  # round(): half to even, as rint
    return out


def execute(batch):
    """numpy model of nasseg_augment_colour (nasseg_augment without "colour") on a collated batch
    -> (float64 B x 3 x Ho x Wo, uint8 B x Ho x Wo)"""
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
        if "colour" in batch:
            words, ctab = batch["colour"][b].numpy(), batch["ctab"][b].numpy()
            assert words.dtype == np.int32 and words.shape == (12,) and ctab.dtype == np.uint8
            assert ctab.shape == (3, 256) and words[10] == 0 and words[11] == 0
            if words[9]:
                q = np.clip(words[:9].astype(np.int32), -(1 << 15), 1 << 15).reshape(3, 3)
                m = np.stack([(q[c, 0] * v[:, :, 0] + q[c, 1] * v[:, :, 1] + q[c, 2] * v[:, :, 2] + 2048) >> 12
                              for c in range(3)], axis=2)
                v = np.clip(m, 0, 255)
            v = np.stack([ctab[c][v[:, :, c]] for c in range(3)], axis=2).astype(np.int64)
        fill = np.array([ifill & 255, (ifill >> 8) & 255, (ifill >> 16) & 255])
        v = np.where(live[:, :, None], v, fill[None, None, :])
        images.append(np.stack([lut[c][v[:, :, c]] for c in range(3)]))
        mlive = (my >= 0)[:, None] & (mx >= 0)[None, :]
        masks.append(np.where(mlive, msk[np.maximum(my, 0)][:, np.maximum(mx, 0)], mfill).astype(np.uint8))
    return np.stack(images), np.stack(masks)


# ---------------------------------------------------------------------------
# construction, arguments, draws
# ---------------------------------------------------------------------------
def test_arguments_are_checked_at_construction():
    D, _ = mods()
    for bad in (dict(brightness=-0.1), dict(contrast=-0.1), dict(contrast=1.0), dict(gamma=1.0), dict(gamma=-1),
                dict(saturation=3.01), dict(saturation=-0.5), dict(hue=0.51), dict(hue=-0.1), dict(p=-0.01),
                dict(p=1.01)):
        with pytest.raises(ValueError):
            D.ColourJitter(**bad)
    D.ColourJitter(brightness=2.0, contrast=0.99, gamma=0.99, saturation=3.0, hue=0.5, p=0.0)
    from nas_segm_amd import data

    assert data.ColourJitter is D.ColourJitter and issubclass(D.ColourJitter, D.SampleOp)


def test_images_are_checked_and_the_mask_passes_through():
    D, _ = mods()
    op = D.ColourJitter(0.2, 0.2, 0.2, 0.2, 0.1)
    img, msk = sample(9, 11, 0)
    for image in (img.astype(np.float32), img.astype(np.int32), img[:, :, 0], img[:, :, :2],
                  np.concatenate([img, img[:, :, :1]], 2)):
        with pytest.raises(ValueError):
            op.apply(image, msk)
    depth = np.random.RandomState(0).rand(9, 11).astype(np.float32)
    for target in (msk, depth):
        out, same = op.apply(img, target)
        assert same is target and out.dtype == np.uint8 and out.shape == img.shape
    assert op({"image": img, "mask": msk})["mask"] is msk


def test_draw_order():
    D, _ = mods()
    mags = dict(brightness=0.3, contrast=0.4, gamma=0.5, saturation=0.6, hue=0.2)
    for seed in range(6):
        rng = np.random.RandomState(seed)
        u = rng.uniform()
        assert u < 1.0
        b, c, g = rng.uniform(-0.3, 0.3), rng.uniform(0.6, 1.4), rng.uniform(0.5, 1.5)
        s, h = rng.uniform(0.4, 1.6), rng.uniform(-0.2, 0.2)
        np.random.seed(seed)
        Mq, Tab = D.ColourJitter(**mags).draw()
        assert states_equal(np.random.get_state(), rng.get_state())
        assert np.array_equal(Mq, matrix_restated(s, h)) and Mq.shape == (3, 3)
        assert Tab.shape == (3, 256) and Tab.dtype == np.uint8
        assert all(Tab[ch].tolist() == table_restated(b, c, g) for ch in range(3))
    # a component of magnitude 0 draws nothing: only saturation (floor at 0) and brightness here
    rng = np.random.RandomState(3)
    rng.uniform()
    b, s = rng.uniform(-0.1, 0.1), rng.uniform(0.0, 3.5)
    np.random.seed(3)
    Mq, Tab = D.ColourJitter(brightness=0.1, saturation=2.5).draw()
    assert states_equal(np.random.get_state(), rng.get_state())
    assert np.array_equal(Mq, matrix_restated(s, 0.0)) and Tab[0].tolist() == table_restated(b, 1.0, 1.0)


def test_zero_magnitudes_and_the_identity_draw():
    D, _ = mods()
    img, msk = sample(13, 17, 1)
    # all magnitudes 0: one draw (u), no stage, the image itself
    rng = np.random.RandomState(5)
    rng.uniform()
    np.random.seed(5)
    assert D.ColourJitter().draw() == (None, None)
    assert states_equal(np.random.get_state(), rng.get_state())
    out, _ = D.ColourJitter().apply(img, msk)
    assert np.array_equal(out, img)
    # u >= p: one number, nothing more, the image unchanged
    op = D.ColourJitter(0.3, 0.3, 0.3, 0.3, 0.3, p=0.5)
    kinds = set()
    for seed in range(12):
        rng = np.random.RandomState(seed)
        u = rng.uniform()
        np.random.seed(seed)
        out, _ = op.apply(img, msk)
        kinds.add(u >= 0.5)
        if u >= 0.5:
            assert out is img and states_equal(np.random.get_state(), rng.get_state())
        else:
            assert not np.array_equal(out, img) and not states_equal(np.random.get_state(), rng.get_state())
    assert kinds == {True, False}
    np.random.seed(0)
    assert D.ColourJitter(0.3, 0.3, 0.3, 0.3, 0.3, p=0.0).draw() == (None, None)


# ---------------------------------------------------------------------------
# the matrix and the table
# ---------------------------------------------------------------------------
def pixels():
    rng = np.random.RandomState(2)
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    primaries = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255],
                          [0, 0, 0], [255, 255, 255]], np.uint8)
    return np.concatenate([(rng.rand(300, 3) * 256).astype(np.uint8), ramp, primaries])


GRID = [(s, h) for s in (0.0, 0.3, 1.0, 1.7, 3.0) for h in (-0.5, -0.31, 0.0, 0.125, 0.5)]


def test_matrix_is_the_documented_one_and_bounded():
    D, _ = mods()
    for s, h in GRID:
        Mq = D.colour_matrix(s, h)
        assert Mq.dtype == np.int64 and np.array_equal(Mq, matrix_restated(s, h))
        assert np.abs(Mq).max() <= D.COLOUR_COEF_MAX == 1 << 15
        assert np.abs(Mq).sum(axis=1).max() * 255 < 8.5e6
    assert np.array_equal(D.colour_matrix(1.0, 0.0), 4096 * np.eye(3, dtype=np.int64))


def test_a_full_turn_is_the_identity_and_grey_stays_grey():
    D, _ = mods()
    px = pixels()
    for turn in (-1.0, 1.0):
        assert np.array_equal(D.colour_apply(px, D.colour_matrix(1.0, turn), None), px)
    grey = px[300:556]
    for s, h in GRID:
        assert np.array_equal(D.colour_apply(grey, D.colour_matrix(s, h), None), grey), (s, h)


def test_no_saturation_is_luma():
    D, _ = mods()
    px = pixels()
    luma = np.rint(px.astype(np.float64).dot(np.array(YIQ[0])))
    for h in (-0.5, 0.0, 0.2):
        out = D.colour_apply(px, D.colour_matrix(0.0, h), None).astype(np.float64)
        assert np.abs(out - luma[:, None]).max() <= 1


def test_matrix_arithmetic_in_python_integers_and_both_clip_ends():
    D, _ = mods()
    px = pixels()
    for s, h in GRID:
        Mq = D.colour_matrix(s, h)
        got = D.colour_apply(px, Mq, None)
        assert got.dtype == np.uint8
        assert got.tolist() == [pixel_restated(Mq, v) for v in px]
    # saturated primaries at the extremes: sums below 0 (the shift of a negative number) and above 255
    primaries = px[556:562]
    for h in (-0.5, 0.5):
        Mq = D.colour_matrix(3.0, h)
        raw = [[(sum(int(Mq[c][k]) * int(v[k]) for k in range(3)) + 2048) // 4096 for c in range(3)]
               for v in primaries]
        assert min(min(r) for r in raw) < 0 and max(max(r) for r in raw) > 255
        got = D.colour_apply(primaries, Mq, None)
        assert got.min() == 0 and got.max() == 255 and got.tolist() == [pixel_restated(Mq, v) for v in primaries]


@pytest.mark.parametrize("b,c,g", [(0.0, 1.0, 1.0), (0.2, 1.0, 1.0), (-0.35, 1.0, 1.0), (0.0, 1.6, 1.0),
                                   (0.0, 0.3, 1.0), (0.0, 1.0, 0.45), (0.0, 1.0, 1.8), (0.13, 1.31, 0.77),
                                   (-0.6, 1.9, 1.5), (1.5, 0.5, 0.5)])
def test_point_table(b, c, g):
    D, _ = mods()
    tab = D.point_table(b, c, g)
    assert tab.dtype == np.uint8 and tab.shape == (256,) and tab.tolist() == table_restated(b, c, g)
    if (b, c, g) == (0.0, 1.0, 1.0):
        assert tab.tolist() == list(range(256))
    px = pixels()
    Tab = np.repeat(tab[None], 3, axis=0)
    assert np.array_equal(D.colour_apply(px, None, Tab), tab[px])


# ---------------------------------------------------------------------------
# the device plan: a numpy executor of the colour launch against the host pipeline
# ---------------------------------------------------------------------------
JITTER = dict(brightness=0.25, contrast=0.4, gamma=0.3, saturation=0.8, hue=0.15, p=0.5)
FILL = (124.4, 116, 104)


def plan_pipelines():
    D, _ = mods()
    out = {}
    for scale in (0.7, 1.0, 1.37):
        out["resize_{}".format(scale)] = [D.ResizeScale(10, scale, scale), D.RandomCrop(20), D.ColourJitter(**JITTER)]
    out["jitter_before_pad"] = [D.ResizeScale(10, 0.8, 1.2), D.RandomCrop(22), D.ColourJitter(**JITTER),
                                D.Pad(30, FILL, 255), D.RandomCrop(28)]
    out["jitter_after_pad"] = [D.ResizeScale(10, 0.8, 1.2), D.Pad(64, FILL, 255), D.ColourJitter(**JITTER),
                               D.RandomMirror(), D.RandomCrop(60)]
    out["mirror_crop"] = [D.RandomMirror(), D.RandomCrop(24), D.ColourJitter(**JITTER)]
    out["jitter_first"] = [D.ColourJitter(**JITTER), D.RandomMirror(), D.RandomCrop(24)]
    out["extremes"] = [D.RandomCrop(24), D.ColourJitter(0.5, 0.9, 0.9, 3.0, 0.5)]
    return {k: D.Compose(v + norm_ops()) for k, v in out.items()}


def sources():
    return [sample(37, 53, 0), sample(41, 29, 1), sample(37, 53, 2)]


def batch_seed(pipeline):
    """the first seed under which a batch of three has jittered and identity samples (p = 0.5)"""
    n_before = [type(op).__name__ for op in pipeline.transforms].index("ColourJitter")
    for seed in range(100):
        np.random.seed(seed)
        kinds = set()
        _, dev = mods()
        for img, msk in sources():
            kinds.add(bool(dev.plan_sample(pipeline, img, msk)["colour"][9]))
        if kinds == {True, False}:
            return seed
    raise AssertionError("no seed with both kinds ({} operations before the jitter)".format(n_before))


@pytest.mark.parametrize("name", ["resize_0.7", "resize_1.0", "resize_1.37", "jitter_before_pad", "jitter_after_pad",
                                  "mirror_crop", "jitter_first", "extremes"])
def test_executor_equals_the_host_pipeline(name):
    _, dev = mods()
    pipeline = plan_pipelines()[name]
    seed = 0 if name == "extremes" else batch_seed(pipeline)
    np.random.seed(seed)
    host = [pipeline({"image": img, "mask": msk}) for img, msk in sources()]
    host_state = np.random.get_state()
    np.random.seed(seed)
    samples = [dev.plan_sample(pipeline, img, msk) for img, msk in sources()]
    assert states_equal(np.random.get_state(), host_state)
    batch = dev.collate(samples)
    assert batch["colour"].shape == (3, 12) and batch["colour"].dtype.is_floating_point is False
    assert batch["ctab"].shape == (3, 3, 256) and batch["ctab"].numpy().dtype == np.uint8
    applied = batch["colour"][:, 9].tolist()
    ramp = np.arange(256, dtype=np.uint8)
    identity = [not a and all(np.array_equal(batch["ctab"][b, c].numpy(), ramp) for c in range(3))
                for b, a in enumerate(applied)]
    if name != "extremes":
        assert True in identity and False in identity  # (p = 0.5: both kinds in the batch)
    images, masks = execute(batch)
    for b, h in enumerate(host):
        want = h["image"].numpy()
        assert want.dtype == np.float64 and want.shape == images[b].shape
        assert np.array_equal(images[b], want), (name, b)
        assert np.array_equal(masks[b], h["mask"].numpy())
    if name == "extremes":  # sums below 0 and above 255 among the live pixels (no resize: the uploaded windows)
        raw = []
        for b in range(3):
            io, _, h, w = (int(v) for v in batch["desc"][b, :4])
            px = batch["src"].numpy()[io: io + 3 * h * w].reshape(-1, 3).astype(np.int64)
            raw.append((px.dot(batch["colour"][b, :9].numpy().reshape(3, 3).astype(np.int64).T) + 2048) >> 12)
        assert all(applied) and min(r.min() for r in raw) < 0 and max(r.max() for r in raw) > 255


def test_a_pad_before_the_jitter_has_its_fill_jittered_and_one_after_has_not():
    D, dev = mods()
    op = D.ColourJitter(**dict(JITTER, p=1.0))
    img, msk = sample(20, 20, 4)
    plain = int(np.uint8(124)) | 116 << 8 | 104 << 16
    np.random.seed(1)
    before = dev.plan_sample(D.Compose([D.Pad(30, FILL, 255), op] + norm_ops()), img, msk)
    np.random.seed(1)
    after = dev.plan_sample(D.Compose([op, D.Pad(30, FILL, 255)] + norm_ops()), img, msk)
    np.random.seed(1)
    Mq, Tab = op.draw()
    want = D.colour_apply(np.array([124, 116, 104], np.uint8), Mq, Tab)
    assert before["fill"][0] == int(want[0]) | int(want[1]) << 8 | int(want[2]) << 16 != plain
    assert after["fill"][0] == plain
    assert np.array_equal(before["colour"], after["colour"]) and np.array_equal(before["ctab"], after["ctab"])


def test_depth_samples_carry_the_tables_and_match_the_host():
    D, dev = mods()
    pipe = D.Compose([D.DepthResizeScale(10, 0.8, 1.3), D.RandomMirror(), D.RandomCrop(24),
                      D.ColourJitter(**JITTER)] + norm_ops())
    rng = np.random.RandomState(3)
    counts = [rng.randint(0, 9000, img.shape[:2]).astype(np.uint16) for img, _ in sources()]
    seed = batch_seed(pipe)
    np.random.seed(seed)
    host = [pipe({"image": img, "mask": c.astype(np.float32) * np.float32(1e-3)})
            for (img, _), c in zip(sources(), counts)]
    host_state = np.random.get_state()
    np.random.seed(seed)
    samples = [dev.plan_depth_sample(pipe, img, c) for (img, _), c in zip(sources(), counts)]
    assert states_equal(np.random.get_state(), host_state)
    batch = dev.collate_depth(samples)
    assert set(batch) == {"src", "desc", "taps", "lut", "size", "params", "colour", "ctab"}
    # the image half through the executor (the "mask" windows hold counts: only the image is compared here)
    desc = batch["desc"].numpy().copy()
    desc[:, 1], desc[:, 5] = desc[:, 0], desc[:, 3]  # (any window of h x w bytes will do for the unused mask)
    images, _ = execute(dict(batch, desc=torch.from_numpy(desc)))
    for b, h in enumerate(host):
        assert np.array_equal(images[b], h["image"].numpy())


# ---------------------------------------------------------------------------
# refusals, keys, loaders
# ---------------------------------------------------------------------------
def test_check_pipeline_refusals():
    D, dev = mods()
    cj = lambda: D.ColourJitter(**JITTER)  # noqa: E731
    norm, tt = norm_ops()
    cases = [
        ([cj(), D.ResizeScale(10, 1, 2), D.RandomCrop(20), norm, tt], "before a resize"),
        ([cj(), D.ResizeShorter(20), norm, tt], "before a resize"),
        ([D.ResizeScale(10, 1, 2), cj(), D.RandomCrop(20), cj(), norm, tt], "at most one ColourJitter"),
        ([D.RandomCrop(20), norm, cj(), tt], "after Normalise"),
        ([D.RandomCrop(20), norm, tt, cj()], "after Normalise"),
    ]
    messages = set()
    for ops, text in cases:
        with pytest.raises(ValueError) as e:
            dev.check_pipeline(D.Compose(ops))
        assert text in str(e.value), (text, str(e.value))
        messages.add(text)
    assert len(messages) == 3
    # allowed: crops, mirror and pad on either side
    dev.check_pipeline(D.Compose([D.ResizeScale(10, 1, 2), D.Pad(30, FILL, 255), cj(), D.RandomMirror(),
                                  D.RandomCrop(20), norm, tt]))
    dev.check_pipeline(D.Compose([D.RandomMirror(), D.RandomCrop(20), cj(), D.Pad(30, FILL, 255), norm, tt]))


def test_mixed_batches_are_refused_and_plain_batches_keep_their_keys():
    D, dev = mods()
    norm, tt = norm_ops()
    img, msk = sample(30, 30, 0)
    np.random.seed(0)
    plain = dev.plan_sample(D.Compose([D.RandomCrop(20), norm, tt]), img, msk)
    jittered = dev.plan_sample(D.Compose([D.RandomCrop(20), D.ColourJitter(**JITTER), norm, tt]), img, msk)
    assert set(plain) == {"image", "mask", "taps", "fill", "lut", "size"}
    assert set(jittered) == set(plain) | {"colour", "ctab"}
    assert set(dev.collate([plain, plain])) == {"src", "desc", "taps", "lut", "size"}
    assert set(dev.collate([jittered, jittered])) == {"src", "desc", "taps", "lut", "size", "colour", "ctab"}
    for mixed in ([plain, jittered], [jittered, plain]):
        with pytest.raises(RuntimeError):
            dev.collate(mixed)
    counts = np.zeros((30, 30), np.uint16)
    depth = dev.plan_depth_sample(D.Compose([D.RandomCrop(20), norm, tt]), img, counts)
    assert set(dev.collate_depth([depth])) == {"src", "desc", "taps", "lut", "size", "params"}
    # an identity draw still carries both: the unit matrix not applied, the ramp
    np.random.seed(0)
    s = dev.plan_sample(D.Compose([D.ColourJitter(0.5, p=0.0), norm, tt]), img, msk)
    assert s["colour"].dtype == np.int32 and s["colour"].tolist() == [4096, 0, 0, 0, 4096, 0, 0, 0, 4096, 0, 0, 0]
    assert s["ctab"].dtype == np.uint8 and np.array_equal(s["ctab"], np.repeat(np.arange(256)[None], 3, axis=0))


def loader_args(tmp_path, **kw):
    from PIL import Image

    rng = np.random.RandomState(1)
    lines = []
    for i in range(6):
        Image.fromarray((rng.rand(50, 60, 3) * 255).astype(np.uint8)).save(str(tmp_path / "i{}.png".format(i)))
        Image.fromarray((rng.rand(50, 60) * 21).astype(np.uint8)).save(str(tmp_path / "m{}.png".format(i)))
        Image.fromarray((rng.rand(50, 60) * 9000).astype(np.uint16)).save(str(tmp_path / "d{}.png".format(i)))
        lines.append((i, i))
    (tmp_path / "l.lst").write_text("".join("i{}.png\tm{}.png\n".format(*ln) for ln in lines))
    (tmp_path / "d.lst").write_text("".join("i{}.png\td{}.png\n".format(*ln) for ln in lines))
    a = dict(train_dir=str(tmp_path), val_dir=str(tmp_path), train_list=str(tmp_path / "l.lst"),
             val_list=str(tmp_path / "l.lst"), meta_train_prct=50, resize_side=[40], low_scale=0.7, high_scale=1.4,
             resize_longer_side=False, crop_size=[32], val_resize_side=40, val_crop_size=32,
             normalise_params=[1.0 / 255, MEAN, STD], batch_size=[2], val_batch_size=1, num_workers=0)
    a.update(kw)
    return types.SimpleNamespace(**a)


def kinds_of(loader, which):
    ds = loader.dataset.dataset
    return [type(op).__name__ for op in getattr(ds, which).transforms]


TRAIN_KINDS = ["ResizeScale", "RandomMirror", "RandomCrop", "Normalise", "ToTensor"]
VAL_KINDS = ["ResizeScale", "CentralCrop", "Normalise", "ToTensor"]


@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("device", [False, True])
def test_loaders_build_the_op_at_position_three(tmp_path, depth, device):
    from nas_segm_amd import data

    _, dev = mods()
    create = {(False, False): data.create_loaders, (True, False): data.create_depth_loaders,
              (False, True): dev.create_device_loaders, (True, True): dev.create_device_depth_loaders}[(depth, device)]
    lst = str(tmp_path / ("d.lst" if depth else "l.lst"))
    first = "DepthResizeScale" if depth else "ResizeScale"
    for kw in ({}, {"colour_jitter": None}):
        trn, val, _ = create(loader_args(tmp_path, train_list=lst, val_list=lst, **kw))
        assert kinds_of(trn, "transform_trn") == [first] + TRAIN_KINDS[1:]
        assert kinds_of(val, "transform_val") == VAL_KINDS
    trn, val, _ = create(loader_args(tmp_path, train_list=lst, val_list=lst, colour_jitter=dict(JITTER)))
    assert kinds_of(trn, "transform_trn") == [first] + TRAIN_KINDS[1:3] + ["ColourJitter"] + TRAIN_KINDS[3:]
    assert kinds_of(val, "transform_val") == VAL_KINDS
    ds = trn.dataset.dataset
    op = ds.transform_trn.transforms[3]
    assert (op.brightness, op.contrast, op.gamma, op.saturation, op.hue, op.p) == (0.25, 0.4, 0.3, 0.8, 0.15, 0.5)
    ds.set_config(20, 30)
    assert ds.transform_trn.transforms[0].resize_side == 30 and ds.transform_trn.transforms[2].crop_size == 20
    np.random.seed(0)
    batch = next(iter(trn.loader if device else trn))
    if device:
        assert batch["colour"].shape == (2, 12) and batch["ctab"].shape == (2, 3, 256)
        assert tuple(int(v) for v in batch["size"]) == (20, 20)
    else:
        assert batch["image"].shape == (2, 3, 20, 20)
