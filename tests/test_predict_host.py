"""Prediction without a device: the dsize form of the INTER_CUBIC restatement (data/datasets.resize_cubic_to, the
yardstick of csrc/predict.hip), the tables the wrappers upload, the prepare_img table of F.prepare_image, and the
argument checks of engine/predict.Predictor."""
import gc
import weakref

import numpy as np
import pytest
import torch

import nas_segm_amd  # noqa: F401
from nas_segm_amd import functional as F
from nas_segm_amd.data import datasets as D
from nas_segm_amd.data import device as ddev
from nas_segm_amd.engine.inference import Predictor

# the reference's prepare_img (src/utils/helpers.py), restated
IMG_SCALE = 1.0 / 255
IMG_MEAN = np.array([0.485, 0.456, 0.406]).reshape((1, 1, 3))
IMG_STD = np.array([0.229, 0.224, 0.225]).reshape((1, 1, 3))


def prepare_img(img):
    return (img * IMG_SCALE - IMG_MEAN) / IMG_STD


def rand(*shape, seed=0):
    return np.random.RandomState(seed).randn(*shape).astype(np.float32)


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("shape", [(13, 21), (9, 17, 19)])
def test_dsize_form_equals_the_scale_form_at_integral_factors(s, shape):
    a = rand(*shape, seed=s)
    got = D.resize_cubic_to(a, (round(shape[0] * s), round(shape[1] * s)))
    want = D.resize_cubic(a, s)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _torch_bicubic(a, size):
    t = torch.from_numpy(np.ascontiguousarray(np.moveaxis(a, 2, 0)))[None]
    out = torch.nn.functional.interpolate(t, size=size, mode="bicubic", align_corners=False)
    return np.moveaxis(out[0].numpy(), 0, 2)


@pytest.mark.parametrize("src, dst", [((81, 81), (321, 321)), ((97, 129), (161, 241)), ((161, 241), (40, 61)),
                                      ((33, 47), (101, 75))])
def test_dsize_form_agrees_with_torch_bicubic(src, dst):
    """Keys' A = -0.75, half-pixel centres and a replicated border in both: the same published formula (the fp32
    coordinates and weights are rounded differently: a few ulps of the weights, 1e-5 of the range)"""
    a = rand(src[0], src[1], 3, seed=1)
    got = D.resize_cubic_to(a, dst)
    want = _torch_bicubic(a, dst)
    assert got.shape == want.shape == (dst[0], dst[1], 3)
    assert np.abs(got - want).max() <= 3e-5 * np.abs(want).max()


def test_dsize_form_agrees_with_torch_bicubic_at_full_size():
    """256x512 -> 1024x2048 (the logits of a 2048x1024 image back to its size), compared on a crop"""
    a = rand(256, 512, 1, seed=2)
    got = D.resize_cubic_to(a, (1024, 2048))
    want = _torch_bicubic(a, (1024, 2048))
    crop = (slice(0, 96), slice(1900, 2048))
    assert np.abs(got[crop] - want[crop]).max() <= 3e-5 * np.abs(want).max()
    assert np.abs(got - want).max() <= 3e-5 * np.abs(want).max()


def test_identity_taps_give_the_input_back():
    a = rand(19, 23, 5, seed=3) * 1e6
    assert np.array_equal(D.resize_cubic_to(a, (19, 23)), a)
    taps, coef = F.cubic_tables_host(19, 23, 19, 23)
    assert np.array_equal(coef.reshape(-1, 4), np.tile(np.float32([0, 1, 0, 0]), (19 + 23, 1)))
    assert np.array_equal(taps.reshape(-1, 4)[:, 1], np.concatenate([np.arange(19), np.arange(23)]))


def test_dsize_form_refuses_integer_images():
    with pytest.raises(TypeError):
        D.resize_cubic_to(np.zeros((4, 4, 3), np.uint8), (8, 8))


@pytest.mark.parametrize("h, w, H, W", [(64, 128, 256, 512), (81, 81, 321, 321), (97, 129, 40, 50), (7, 9, 7, 9)])
def test_uploaded_tables_are_the_cubic_taps(h, w, H, W):
    taps, coef = F.cubic_tables_host(h, w, H, W)
    assert taps.dtype == np.int32 and coef.dtype == np.float32 and taps.shape == coef.shape == (4 * (H + W),)
    iy, wy = D._cubic_taps(h, H, H / h)
    ix, wx = D._cubic_taps(w, W, W / w)
    assert np.array_equal(taps, np.concatenate([iy.ravel(), ix.ravel()]))
    assert np.array_equal(coef, np.concatenate([wy.ravel(), wx.ravel()]))
    assert taps.min() >= 0 and taps[:4 * H].max() < h and taps[4 * H:].max() < w


def test_prepare_img_table_is_prepare_img_bit_for_bit():
    """for every uint8 value and channel: the table F.prepare_image maps through, cast as the kernel receives it,
    equals torch.tensor(prepare_img(img)).float() (and its bf16 rounding)"""
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)  # 256 x 1 x 3
    want = torch.tensor(prepare_img(ramp)[:, 0, :].T.copy()).float()  # [3][256]
    table = torch.from_numpy(ddev.prepare_img_table())
    assert table.dtype == torch.float64 and tuple(table.shape) == (3, 256)
    got = table.float()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got.to(torch.bfloat16).view(torch.int16), want.to(torch.bfloat16).view(torch.int16))


def _net():
    return torch.nn.Conv2d(3, 4, 1)


def test_predictor_refuses_bad_arguments():
    m = _net()
    with pytest.raises(ValueError):
        Predictor(m, task="classify")
    with pytest.raises(ValueError):
        Predictor(m, dtype=torch.float16)
    with pytest.raises(ValueError):
        Predictor(m, graph="always")
    with pytest.raises(ValueError):
        Predictor(m, graph=1)
    with pytest.raises(ValueError):
        Predictor(object())
    pred = Predictor(m.eval())
    img = np.zeros((5, 7, 3), np.uint8)
    for bad in [(0, 5), (5,), (5, 7, 3), "image", (2.5, 3), (-1, 4)]:
        with pytest.raises(ValueError):
            pred(img, out_size=bad)
    for bad in [np.zeros((5, 7, 3), np.float32), np.zeros((5, 7), np.uint8), np.zeros((5, 7, 4), np.uint8),
                np.zeros((1, 2, 5, 7, 3), np.uint8), np.zeros((0, 7, 3), np.uint8)]:
        with pytest.raises(ValueError):
            pred(bad)
    with pytest.raises(ValueError):
        pred.logits(torch.zeros(1, 4, 5, 7))


def test_predictor_refuses_a_model_in_training_mode():
    m = _net().train()
    with pytest.raises(ValueError, match="training"):
        Predictor(m)(np.zeros((5, 7, 3), np.uint8))
    with pytest.raises(ValueError, match="training"):
        Predictor(m).logits(torch.zeros(1, 3, 5, 7))


def test_predictor_does_not_keep_its_model_alive():
    m = _net().eval()
    pred = Predictor(m)
    ref = weakref.ref(m)
    del m
    gc.collect()
    assert ref() is None
    with pytest.raises(ReferenceError):
        pred(np.zeros((5, 7, 3), np.uint8))
