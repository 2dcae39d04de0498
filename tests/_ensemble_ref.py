"""Float64 host restatement of the test-time ensemble (csrc/ensemble.hip, F.fuse_views): per view the logit map is
un-mirrored, resampled to the output size, soft-maxed over the classes; the probabilities are averaged and the label
is numpy's argmax of the average.

Cubic mode resamples with data/datasets.resize_cubic_to - the pinned fp32 yardstick of csrc/predict.hip, which the
kernel reproduces bit for bit - and widens the result.  Bilinear mode applies the two taps and fp32 weights per axis
of F.linear_tables_host (the tables the kernel is handed: F.interpolate's align_corners=False coordinates in fp32,
checked against torch in test_ensemble_host.py) in float64: an fp32 coordinate is off by about n_src * 2^-24, which
no arithmetic after it can take back, so the weights belong to the statement and the sums are what is restated.
Everything after the resampling is float64."""
import math

import numpy as np

from nas_segm_amd.data import datasets as D


def view_size(n, s):
    return max(1, int(math.floor(n * s + 0.5)))


def _linear_axis(n_src, n_dst):
    d = np.arange(n_dst, dtype=np.float64)
    src = d if n_src == n_dst else np.maximum((d + 0.5) * (float(n_src) / float(n_dst)) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_src - 1)
    i1 = np.minimum(i0 + 1, n_src - 1)
    l1 = np.clip(src - i0, 0.0, 1.0)
    return i0, i1, l1


def resize_linear_to(a, size):
    """float64 bilinear resize, align_corners=False, of an h x w x C array to size = (H, W)"""
    a = np.asarray(a, np.float64)
    y0, y1, ly = _linear_axis(a.shape[0], size[0])
    x0, x1, lx = _linear_axis(a.shape[1], size[1])
    rows = a[:, x0] * (1.0 - lx)[None, :, None] + a[:, x1] * lx[None, :, None]
    return rows[y0] * (1.0 - ly)[:, None, None] + rows[y1] * ly[:, None, None]


def resize_tables_to(a, size):
    """float64 h x w x C -> H x W x C through the fp32 tables of F.linear_tables_host: horizontal pass, then
    vertical"""
    from nas_segm_amd import functional as F

    a = np.asarray(a, np.float64)
    H, W = size
    taps, coef = F.linear_tables_host(a.shape[0], a.shape[1], H, W)
    iy, ix = taps[:2 * H].reshape(H, 2), taps[2 * H:].reshape(W, 2)
    wy, wx = coef[:2 * H].reshape(H, 2).astype(np.float64), coef[2 * H:].reshape(W, 2).astype(np.float64)
    rows = a[:, ix[:, 0]] * wx[None, :, 0, None] + a[:, ix[:, 1]] * wx[None, :, 1, None]
    return rows[iy[:, 0]] * wy[:, 0, None, None] + rows[iy[:, 1]] * wy[:, 1, None, None]


def resampled(view, mirrored, size, mode):
    """one view h x w x C (fp32; a bf16 view widened by the caller) -> float64 H x W x C at the output size"""
    a = np.asarray(view)
    if mirrored:
        a = a[:, ::-1]
    if mode == "cubic":
        return D.resize_cubic_to(np.ascontiguousarray(a, np.float32), size).astype(np.float64)
    if mode == "bilinear":
        return resize_tables_to(a, size)
    raise ValueError(mode)


def softmax(r):
    e = np.exp(r - r.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def mean_probabilities(views, mirrored, size, mode="cubic"):
    """float64 H x W x C: the mean over the views of softmax(resampled view), added in view order"""
    total = None
    for v, m in zip(views, mirrored):
        p = softmax(resampled(v, m, size, mode))
        total = p if total is None else total + p
    return total / len(views)


def mean_map(views, mirrored, size, mode="cubic"):
    """float64 H x W x C: the mean over the views of the resampled maps (depth: no softmax)"""
    total = None
    for v, m in zip(views, mirrored):
        r = resampled(v, m, size, mode)
        total = r if total is None else total + r
    return total / len(views)


def labels_of(probs):
    return np.argmax(probs, axis=-1).astype(np.uint8)


def top2_gap(probs):
    top2 = np.sort(probs, axis=-1)[..., -2:]
    return top2[..., 1] - top2[..., 0]


def check_labels(got, probs, max_fraction=1e-4, max_gap=1e-5):
    """the rule of test_argmax_confusion_fused_upsample: at most ``max_fraction`` of the pixels differ from the
    reference's labels, each with a float64 top-2 gap of the mean probability below ``max_gap``.  Returns the number
    of differing pixels."""
    diff = np.asarray(got) != labels_of(probs)
    if diff.any():
        assert diff.mean() <= max_fraction, "{} of the labels differ".format(diff.mean())
        assert top2_gap(probs)[diff].max() < max_gap, "a label differs at a top-2 gap of {}".format(
            top2_gap(probs)[diff].max())
    return int(diff.sum())
