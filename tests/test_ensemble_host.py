"""The test-time ensemble without a device: the view-size rule, the tables F.fuse_views uploads (mirrored columns,
the bilinear taps), the new prototypes of include/nasseg.h, the argument checks of Predictor and validate, and the
float64 restatement the device tests compare with (tests/_ensemble_ref.py)."""
import numpy as np
import pytest
import torch

import _ensemble_ref as R
import nas_segm_amd  # noqa: F401
from nas_segm_amd import functional as F
from nas_segm_amd._lib import HEADER_PATH, pointer_access
from nas_segm_amd.data import datasets as D
from nas_segm_amd.engine.inference import Predictor, validate
from nas_segm_amd.engine.predict import ensemble_views
from nas_segm_amd.ffi_gen import prototypes


@pytest.mark.parametrize("n, s, want", [(7, 0.5, 4), (5, 0.5, 3), (1, 0.1, 1), (1024, 0.75, 768), (161, 1.5, 242),
                                        (241, 0.75, 181), (2048, 1.75, 3584), (3, 1.0, 3), (10, 0.04, 1)])
def test_view_size_rule(n, s, want):
    assert F.view_size(n, s) == want == R.view_size(n, s)
    assert isinstance(F.view_size(n, s), int)


@pytest.mark.parametrize("mode, T", [("cubic", 4), ("bilinear", 2)])
def test_mirrored_column_tables_are_the_plain_ones_reversed_in_the_source(mode, T):
    shapes, H, W = [(9, 13), (21, 30), (9, 13)], 37, 52
    taps, coef, dims = F.fuse_tables_host(shapes, [False, True, True], H, W, mode)
    plain, coef0, dims0 = F.fuse_tables_host(shapes, [False, False, False], H, W, mode)
    n = T * (H + W)
    assert taps.dtype == np.int32 and coef.dtype == np.float32 and taps.shape == coef.shape == (3 * n,)
    assert dims.tolist() == dims0.tolist() == [[9, 13, 0], [21, 30, n], [9, 13, 2 * n]]
    assert np.array_equal(coef, coef0)
    single = F.cubic_tables_host if mode == "cubic" else F.linear_tables_host
    for v, (h, w) in enumerate(shapes):
        t, c = single(h, w, H, W)
        assert np.array_equal(plain[v * n:(v + 1) * n], t) and np.array_equal(coef[v * n:(v + 1) * n], c)
        rows, cols = taps[v * n:v * n + T * H], taps[v * n + T * H:(v + 1) * n]
        assert np.array_equal(rows, t[:T * H])
        assert np.array_equal(cols, w - 1 - t[T * H:] if v else t[T * H:])
        assert cols.min() >= 0 and cols.max() < w


@pytest.mark.parametrize("h, w, H, W", [(9, 13, 37, 52), (40, 50, 11, 17), (7, 9, 7, 9), (1, 1, 5, 4)])
def test_bilinear_tables_are_interpolate_without_aligned_corners(h, w, H, W):
    taps, coef = F.linear_tables_host(h, w, H, W)
    assert taps.shape == coef.shape == (2 * (H + W),)
    assert taps.min() >= 0 and taps[:2 * H].max() < h and taps[2 * H:].max() < w
    a = np.random.RandomState(h + W).randn(h, w, 3).astype(np.float32)
    iy, ix = taps[:2 * H].reshape(H, 2), taps[2 * H:].reshape(W, 2)
    wy, wx = coef[:2 * H].reshape(H, 2).astype(np.float64), coef[2 * H:].reshape(W, 2).astype(np.float64)
    rows = a[:, ix[:, 0]] * wx[None, :, 0, None] + a[:, ix[:, 1]] * wx[None, :, 1, None]
    got = rows[iy[:, 0]] * wy[:, 0, None, None] + rows[iy[:, 1]] * wy[:, 1, None, None]
    t = torch.from_numpy(np.ascontiguousarray(np.moveaxis(a, 2, 0)))[None].double()
    want = torch.nn.functional.interpolate(t, size=(H, W), mode="bilinear", align_corners=False)[0]
    want = np.moveaxis(want.numpy(), 0, 2)
    assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    assert np.abs(R.resize_linear_to(a, (H, W)) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    if (h, w) == (H, W):
        assert np.array_equal(got, a.astype(np.float64))


def test_the_new_prototypes_are_in_the_header_with_their_twins():
    protos = {p.name: p for p in prototypes(HEADER_PATH)}
    acc = pointer_access()
    for name in ("view_image", "fuse_views"):
        base, twin = protos["nasseg_" + name], protos["nasseg_bf16_" + name]
        assert base.ret == twin.ret == "int" and len(base.args) == len(twin.args)
        assert [a.name for a in base.args] == [a.name for a in twin.args] and base.args[-1].name == "stream"
    for prefix in ("nasseg_", "nasseg_bf16_"):
        names = [a.name for a in protos[prefix + "fuse_views"].args]
        kinds = {names[i]: k for i, k in acc[prefix + "fuse_views"]}
        assert kinds == {"views": "t", "dims": "r", "taps": "r", "coef": "r", "gt": "r", "labels": "w", "probs": "w",
                         "cm": "w", "mean": "w"}
        names = [a.name for a in protos[prefix + "view_image"].args]
        assert {names[i]: k for i, k in acc[prefix + "view_image"]} == {"x": "r", "y": "w"}
    views = protos["nasseg_bf16_fuse_views"].args[1]
    assert views.ctype == "const nasseg_bf16_t* const*" and views.levels == 2


class _Untouchable(object):
    """a model / loader that fails the test when anything is asked of it"""

    def __getattr__(self, name):
        raise AssertionError("touched .{} before the arguments were checked".format(name))


BAD_VIEWS = [((), False), ((0.0, 1.0), False), ((-1.0,), False), ((float("nan"),), False), ((float("inf"),), True),
             ((1.0, 0.5, 1.0), False), ("wide", False), (None, True), ((1.0,), "yes"), ((1.0,), 1),
             (tuple(0.5 + 0.125 * i for i in range(17)), False), (tuple(0.5 + 0.125 * i for i in range(9)), True)]


@pytest.mark.parametrize("scales, flip", BAD_VIEWS, ids=lambda v: repr(v)[:24])
def test_predictor_and_validate_refuse_bad_views_before_any_device_work(scales, flip):
    with pytest.raises(ValueError):
        Predictor(torch.nn.Conv2d(3, 4, 1).eval(), scales=scales, flip=flip)
    if scales is None:
        scales = ()  # (None is validate's single forward)
    with pytest.raises(ValueError):
        validate.__wrapped__(_Untouchable(), _Untouchable(), 0, 0, num_classes=4, scales=scales, flip=flip)


def test_validate_refuses_flip_without_scales_and_accepted_views_are_ordered():
    with pytest.raises(ValueError):
        validate.__wrapped__(_Untouchable(), _Untouchable(), 0, 0, num_classes=4, flip=True)
    assert ensemble_views((1.0,), False) == ((1.0, False),)
    assert ensemble_views([0.5, 1, 1.5], True) == ((0.5, False), (0.5, True), (1.0, False), (1.0, True),
                                                    (1.5, False), (1.5, True))
    assert len(ensemble_views(tuple(0.5 + 0.125 * i for i in range(8)), True)) == 16
    pred = Predictor(torch.nn.Conv2d(3, 4, 1).eval(), scales=(0.75, 1.0), flip=True)
    assert pred.scales == (0.75, 1.0) and pred.flip is True and len(pred.views) == 4
    assert Predictor(torch.nn.Conv2d(3, 4, 1).eval()).views == ((1.0, False),)
    with pytest.raises(ValueError):
        pred(np.zeros((5, 7, 3), np.uint8), out_size="model")
    with pytest.raises(ValueError):
        Predictor(torch.nn.Conv2d(3, 1, 1).eval(), task="depth").probabilities(np.zeros((5, 7, 3), np.uint8))


@pytest.mark.parametrize("C", [1, 19])
def test_the_restatement_with_the_single_plain_view_is_the_notebook_post_processing(C):
    z = np.random.RandomState(C).randn(13, 17, C).astype(np.float32) * 3
    size = (41, 50)
    up = D.resize_cubic_to(z, size)
    probs = R.mean_probabilities([z], [False], size, "cubic")
    assert probs.dtype == np.float64 and probs.shape == (41, 50, C)
    assert np.allclose(probs.sum(axis=2), 1.0, atol=1e-12)
    assert np.array_equal(R.labels_of(probs), np.argmax(up, axis=2).astype(np.uint8))
    assert np.array_equal(R.mean_map([z], [False], size), up.astype(np.float64))
    # a mirrored view of the mirrored map is the plain view
    assert np.array_equal(R.mean_probabilities([z[:, ::-1]], [True], size), probs)
    # two views: the mean of the two softmaxes
    z2 = np.random.RandomState(C + 1).randn(7, 9, C).astype(np.float32)
    both = R.mean_probabilities([z, z2], [False, False], size)
    want = 0.5 * (probs + R.softmax(D.resize_cubic_to(z2, size).astype(np.float64)))
    assert np.abs(both - want).max() < 1e-15
