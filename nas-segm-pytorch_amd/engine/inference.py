"""Validation -> reward (mirrors src/engine/inference.py:18-97).

The reference copies full-resolution logits to the host, arg-maxes with numpy
and loops over pixels in Cython.  Here the bilinear up-sampling to label size,
the argmax (lowest index wins ties), the ``gt < num_classes`` filter and the
confusion-matrix update are one HIP kernel; only the (n, n) int64 matrix leaves
the device.  The metric arithmetic afterwards is unchanged.
"""
import logging

import numpy as np
import torch

from .. import functional as F
from ..helpers.miou_utils import compute_iu, compute_ius_accs
from ..helpers.utils import try_except
from .predict import Predictor  # noqa: F401  (the reference's inference notebooks, on the device)
from .predict import ensemble_views, view_inputs

logger = logging.getLogger(__name__)


def reward_from_cm(cm, omit_classes=(0,)):
    """(reward, miou, macc, mfwiou): geometric mean of mean-IoU, mean accuracy and
    frequency-weighted IoU over classes that are present (IoU <= 1, the 2.0
    sentinel marks absent ones) and not omitted (inference.py:78-91)."""
    ious, n_pixels, accs = compute_ius_accs(cm)
    present = np.array([i for i, iu in enumerate(ious) if iu <= 1.0])
    present = np.setdiff1d(present, list(omit_classes))
    p_ious, p_pix, p_accs = ious[present], n_pixels[present], accs[present]
    miou = np.mean(p_ious)
    macc = np.mean(p_accs)
    mfwiou = np.sum(p_ious * p_pix) / np.sum(p_pix)
    metrics = [miou, macc, mfwiou]
    reward = np.prod(metrics) ** (1.0 / len(metrics))
    return reward, miou, macc, mfwiou


def _set_val_stage(val_loader):
    ds = getattr(val_loader, "dataset", None)
    if ds is not None:
        try:
            ds.set_stage("val")
        except AttributeError:
            sub = getattr(ds, "dataset", None)
            if sub is not None and hasattr(sub, "set_stage"):
                sub.set_stage("val")


def depth_scores(acc):
    """The scores of a depth network from the 12 sums of ``F.depth_metrics`` (a tensor or an array; host arithmetic):
    n, abs_rel = mean |p-g|/g, sq_rel = mean (p-g)^2/g, rmse, rmse_log = sqrt(mean l^2), log10 = mean |log10 p -
    log10 g|, silog = sqrt(mean l^2 - mean(l)^2) with l = ln p - ln g, and d1 / d2 / d3 = the fractions of pixels
    with max(p/g, g/p) < 1.25, 1.25^2, 1.25^3.  Every score is 0.0 for n == 0."""
    a = acc.detach().cpu().numpy() if torch.is_tensor(acc) else np.asarray(acc)
    a = a.astype(np.float64).reshape(-1)
    n = float(a[0])
    names = ("abs_rel", "sq_rel", "rmse", "rmse_log", "log10", "silog", "d1", "d2", "d3")
    if n <= 0:
        return dict({"n": 0.0}, **{k: 0.0 for k in names})
    mean_l, mean_l2 = a[6] / n, a[7] / n
    return {
        "n": n,
        "abs_rel": float(a[3] / n),
        "sq_rel": float(a[4] / n),
        "rmse": float(np.sqrt(a[2] / n)),
        "rmse_log": float(np.sqrt(mean_l2)),
        "log10": float(a[5] / n),
        "silog": float(np.sqrt(max(mean_l2 - mean_l * mean_l, 0.0))),
        "d1": float(a[8] / n),
        "d2": float(a[9] / n),
        "d3": float(a[10] / n),
    }


def depth_reward(scores):
    """geometric mean of the three threshold accuracies (in [0, 1], higher is better): combined the way
    ``reward_from_cm`` combines its three segmentation scores"""
    return float((scores["d1"] * scores["d2"] * scores["d3"]) ** (1.0 / 3.0))


@try_except
def validate_depth(segmenter, val_loader, epoch, epoch2, min_depth=1e-3, max_depth=10.0, print_every=10,
                   reward_fn=None):
    """Evaluate a depth candidate; returns the scalar reward (``reward_fn(scores)``, default ``depth_reward``).
    ``validate`` for a one-channel head: the up-sampling to the ground truth's size, the validity mask and every sum
    of the scores are one HIP kernel (F.depth_metrics); only the 12 doubles leave the device."""
    _set_val_stage(val_loader)
    segmenter.eval()
    model = segmenter.module if hasattr(segmenter, "module") else segmenter
    device = next(model.parameters()).device
    acc = torch.zeros((12,), device=device, dtype=torch.float64)
    try:
        with torch.no_grad():
            for i, sample in enumerate(val_loader):
                image = sample["image"]
                image = image.to(device=device, dtype=torch.bfloat16 if image.dtype == torch.bfloat16
                                 else torch.float32).contiguous(memory_format=torch.channels_last)
                gt = sample["mask"].to(device=device, dtype=torch.float32)
                output = segmenter(image)
                if isinstance(output, tuple):
                    output, _ = output
                F.depth_metrics(output, gt, min_depth, max_depth, acc=acc)
                if i % print_every == 0:
                    logger.info(" Val epoch: {} [{}/{}]\tRMSE: {:.3f}".format(
                        epoch, i, len(val_loader), depth_scores(acc)["rmse"]))
    except Exception:  # (as in validate: the peers wait in the all-reduce of the sums)
        if hasattr(segmenter, "reduce_sums"):
            segmenter.reduce_sums(acc, failed=True)
        raise
    if hasattr(segmenter, "reduce_sums"):
        segmenter.reduce_sums(acc)
    scores = depth_scores(acc)
    reward = float(reward_fn(scores)) if reward_fn is not None else depth_reward(scores)
    logger.info((" Val epoch: {}/{}\tabs rel: {:.4f}\tRMSE: {:.4f}\tlog10: {:.4f}\tsilog: {:.4f}\t"
                 "d1/d2/d3: {:.3f}/{:.3f}/{:.3f}\tReward: {:.3f}").format(
                     epoch, epoch2, scores["abs_rel"], scores["rmse"], scores["log10"], scores["silog"],
                     scores["d1"], scores["d2"], scores["d3"], reward))
    return reward


@try_except
def validate(segmenter, val_loader, epoch, epoch2, num_classes=-1, print_every=10,
             omit_classes=[0], scales=None, flip=False):
    """Evaluate the candidate; returns the scalar reward.

    ``scales`` (None: one forward per batch, as the reference) / ``flip``: score the test-time ensemble instead -
    per batch one forward per view (engine/predict.ensemble_views: the image resized bilinearly to each scale, and
    mirrored) and ONE F.fuse_views launch that up-samples every view bilinearly to the ground truth's size,
    averages the class probabilities, takes the argmax and updates the confusion matrix."""
    views = None if scales is None else ensemble_views(scales, flip, "validate")
    if scales is None and flip is not False:
        raise ValueError("validate: flip needs scales (scales=(1.0,) for the mirrored pair alone)")
    ds = getattr(val_loader, "dataset", None)
    if ds is not None:
        try:
            ds.set_stage("val")
        except AttributeError:
            sub = getattr(ds, "dataset", None)
            if sub is not None and hasattr(sub, "set_stage"):
                sub.set_stage("val")
    segmenter.eval()
    model = segmenter.module if hasattr(segmenter, "module") else segmenter
    device = next(model.parameters()).device
    cm = torch.zeros((num_classes, num_classes), device=device, dtype=torch.int64)
    try:
        with torch.no_grad():
            for i, sample in enumerate(val_loader):
                image = sample["image"].to(device=device, dtype=torch.float32).contiguous(
                    memory_format=torch.channels_last)
                gt = sample["mask"].to(device).to(torch.uint8)  # astype(np.uint8) in the reference
                if views is not None:
                    outputs = [segmenter(x) for x in view_inputs(image, views)]
                    outputs = [o[0] if isinstance(o, tuple) else o for o in outputs]
                    F.fuse_views(outputs, gt.shape[1:], [m for _, m in views], mode="bilinear", gt=gt,
                                 n_classes=num_classes, cm=cm)
                else:
                    output = segmenter(image)
                    if isinstance(output, tuple):
                        output, _ = output
                    F.argmax_confusion(output, gt, num_classes, cm=cm)
                if i % print_every == 0:
                    logger.info(" Val epoch: {} [{}/{}]\tMean IoU: {:.3f}".format(
                        epoch, i, len(val_loader),
                        np.mean([iu for iu in compute_iu(cm) if iu <= 1.0])))
    except Exception:  # (not only RuntimeError: a loader error on one rank must not strand its peers)
        # data parallel: the peers will wait in the confusion-matrix all-reduce - take part in
        # it with the failure flag set so that every rank scores this candidate 0
        if hasattr(segmenter, "reduce_confusion"):
            segmenter.reduce_confusion(cm, failed=True)
        raise
    if hasattr(segmenter, "reduce_confusion"):
        segmenter.reduce_confusion(cm)
    cm_host = cm.cpu().numpy()
    ious, _, accs = compute_ius_accs(cm_host)
    logger.info(" IoUs: {}, accs: {}".format(ious, accs))
    reward, miou, macc, mfwiou = reward_from_cm(cm_host, omit_classes)
    logger.info((" Val epoch: {}/{}\tMean IoU: {:.3f}\tMean FW-IoU: {:.3f}\t"
                 "Mean Acc: {:.3f}\tReward: {:.3f}").format(epoch, epoch2, miou, mfwiou, macc, reward))
    return reward
