"""Helpers shared by the eager steps (trainer.py) and the hipGraph steppers (graphed.py): one forward + loss per
step kind, so that a replayed step records exactly what a host-launched one launches."""
from torch import nn

from .. import functional as F


def inner(segmenter):
    return segmenter.module if hasattr(segmenter, "module") else segmenter


def clip_and_step(groups, native=None):
    """groups: [(parameters, max_norm, optimiser)] - per-sub-module gradient-norm clipping, then
    the optimiser steps (src/engine/trainer.py:163-166,258-268).  Plain torch.optim.SGD / Adam objects on a HIP
    device are stepped by nasseg_optim_step (engine/optim_native.py: two launches, the optimisers' own state);
    anything else by torch.  ``native``: the NativeStep to use (a hipGraph stepper's own) instead of the one
    cached on the optimisers."""
    if native is not None:
        native.step()
        return
    # (a caller may hand generators - model.parameters(): both the native path and torch's walk them)
    groups = [(p if isinstance(p, (list, tuple)) else list(p), m, o) for p, m, o in groups]
    from .optim_native import native_clip_and_step

    if native_clip_and_step(groups):
        return
    for params, max_norm, _ in groups:
        if max_norm > 0:
            nn.utils.clip_grad_norm_(params, max_norm)
    for _, _, optim in groups:
        if optim is not None:
            optim.step()


def _heads(output):
    """(logits, [auxiliary logits]) of a segmenter's or a decoder's output"""
    return output if isinstance(output, tuple) else (output, [])


def _head_loss(logits, target, ignore_index, segm_crit):
    """the loss of one head: F.log_softmax_nll, or ``segm_crit`` (an nn.SegmCrossEntropy with class weights,
    hard-example selection or a region-overlap term - every head selects among, and sums over, its own pixels)"""
    if segm_crit is None:
        return F.log_softmax_nll(logits, target, ignore_index)
    return segm_crit(logits, target)


def _full_size(segm_crit):
    """does the criterion take the loss at the labels' own size (nn.SegmCrossEntropy(full_size=True))?"""
    return bool(getattr(segm_crit, "full_size", False))


def segmentation_loss(output, aux_outs, target, ignore_index, aux_weight, loss=None, segm_crit=None):
    """LogSoftmax + NLL of the main head (``loss``: that term already computed, with the distillation term added)
    + aux_weight * those of the auxiliary heads, each resized to the labels' size, when aux_weight > 0.
    A full-size criterion (``_full_size``) up-samples inside its kernels: every head goes in at its own size against
    the same label map, as in ``depth_loss``."""
    if loss is None:
        loss = _head_loss(output, target, ignore_index, segm_crit)
    if aux_weight > 0:
        for aux_out in aux_outs:
            if not _full_size(segm_crit):
                aux_out = F.bilinear_resize(aux_out, target.size()[1:])
            loss = loss + _head_loss(aux_out, target, ignore_index, segm_crit) * aux_weight
    return loss


def task1_loss(segmenter, image, target, ignore_index, aux_weight, segm_crit=None):
    """forward + loss of the end-to-end step: the labels nearest-resized to the logits' size - or, for a full-size
    criterion, left as they are"""
    output, aux_outs = _heads(segmenter(image))
    if not _full_size(segm_crit):
        target = F.nearest_label_resize(target, output.size()[2:])
    return segmentation_loss(output, aux_outs, target, ignore_index, aux_weight, segm_crit=segm_crit)


def depth_loss(output, aux_outs, target, crit, aux_weight):
    """``crit`` (nn.BerHuLoss: the masked berHu) of the main head + aux_weight * that of every auxiliary head when
    aux_weight > 0.  Every head is compared with the SAME full-size target: the kernel samples it at the head's own
    size - or, for ``BerHuLoss(full_size=True)``, up-samples the head to it - so nothing is resized here
    (src/engine/trainer.py:245-250 resizes each head to the target instead)."""
    loss = crit(output, target)
    if aux_weight > 0:
        for aux_out in aux_outs:
            loss = loss + crit(aux_out, target) * aux_weight
    return loss


def task1_depth_loss(segmenter, image, target, crit, aux_weight):
    """forward + loss of the end-to-end DEPTH step: target fp32 (B, H, W) at the image's size, holes included"""
    output, aux_outs = _heads(segmenter(image))
    return depth_loss(output, aux_outs, target, crit, aux_weight)


def cache_feature_keys(cache):
    """the encoder-feature entries of the task0 cache (engine/trainer.py: populate_task0)"""
    return [k for k in cache.keys() if k not in ("y", "y_full", "depth", "kd_y", "out_size")]


def require_full_size_labels(caller, cache, segm_crit):
    """a full-size criterion trains on the cache's full-size labels: without them, a ValueError - raised by the task0
    steps before they touch anything else of their arguments"""
    if _full_size(segm_crit) and "y_full" not in cache:
        raise ValueError("{}: a full-size criterion (SegmCrossEntropy(full_size=True)) needs the cache's full-size "
                         "labels, and this cache holds labels at the logits' size only - make it with "
                         "populate_task0(..., full_size_labels=True)".format(caller))


def check_cache_rows(idx, cache, caller):
    """the reference's Xy_train[k][train_idx] raises here (src/engine/trainer.py:132-137); the gather kernel's
    clamp is a memory-safety net only"""
    n_rows = int(cache["y" if "y" in cache else "depth"].shape[0])
    if not idx.is_cuda and idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n_rows):
        raise IndexError("{}: cache row index out of range [0, {})".format(caller, n_rows))


def task0_loss(cache, index, decoder, ignore_index, aux_weight, kd_coeff=None, kd_crit=None, fuse_kd=True,
               segm_crit=None):
    """forward + loss of the decoder-only step on the cache rows ``index`` (an int64 device tensor): gather, decoder,
    bilinear resize to ``out_size``, softmax/NLL, distillation term, aux heads.  kd_coeff None: no distillation term.
    ``fuse_kd``: the teacher rows are gathered after the resize and kd_coeff * MSE runs fused with the softmax/NLL
    (F.log_softmax_nll_mse refuses a teacher of another shape) - given a ``kd_crit``, only when the rows have the
    logits' shape.  Otherwise kd_coeff * kd_crit(output, teacher rows) runs from the host - always with a
    ``segm_crit`` (class weights / hard-example selection: there is no fused distillation term for it).
    A full-size ``segm_crit`` (``_full_size``): ``task0_full_size_loss`` instead."""
    if _full_size(segm_crit):
        return task0_full_size_loss(cache, index, decoder, segm_crit, aux_weight, kd_coeff, kd_crit)
    feats = [F.gather_rows(cache[k], index) for k in cache_feature_keys(cache)]
    target = F.gather_rows(cache["y"], index)
    output, aux_outs = _heads(decoder(feats))
    output = F.bilinear_resize(output, cache["out_size"])
    loss = None
    if kd_coeff is not None:
        kd_y = F.gather_rows(cache["kd_y"], index) if fuse_kd and segm_crit is None else None
        if kd_y is not None and (kd_crit is None or kd_y.shape == output.shape):
            loss, mse = F.log_softmax_nll_mse(output, target, kd_y, ignore_index)
            loss = loss + kd_coeff * mse
        else:
            loss = _head_loss(output, target, ignore_index, segm_crit)
            kd_y = kd_y if kd_y is not None else F.gather_rows(cache["kd_y"], index)
            loss = loss + kd_coeff * kd_crit(output, kd_y)
    return segmentation_loss(output, aux_outs, target, ignore_index, aux_weight, loss, segm_crit)


def task0_full_size_loss(cache, index, decoder, segm_crit, aux_weight, kd_coeff=None, kd_crit=None):
    """forward + loss of the decoder-only step with a full-size criterion (nn.SegmCrossEntropy(full_size=True)) on the
    cache rows ``index``: gather the feature rows, decoder, ``segm_crit`` of the main head + aux_weight * that of
    every auxiliary head when aux_weight > 0 - as ``task0_depth_loss``, the labels left where they are: the kernels
    read image b's full-size labels from ``cache["y_full"]`` through ``index``, so no head is resized and no labels
    are gathered.  kd_coeff not None: + kd_coeff * kd_crit(the main head resized to ``out_size``, teacher rows),
    launched from the host as written (the fused CE + MSE kernel is for the plain softmax/NLL at the logits' size)."""
    feats = [F.gather_rows(cache[k], index) for k in cache_feature_keys(cache)]
    output, aux_outs = _heads(decoder(feats))
    labels = cache["y_full"]
    loss = segm_crit(output, labels, rows=index)
    if kd_coeff is not None:
        kd_y = F.gather_rows(cache["kd_y"], index)
        loss = loss + kd_coeff * kd_crit(F.bilinear_resize(output, cache["out_size"]), kd_y)
    if aux_weight > 0:
        for aux_out in aux_outs:
            loss = loss + segm_crit(aux_out, labels, rows=index) * aux_weight
    return loss


def task0_depth_loss(cache, index, decoder, crit, aux_weight):
    """forward + loss of the decoder-only DEPTH step on the cache rows ``index`` (an int64 device tensor): gather the
    feature rows, decoder, ``crit`` (nn.BerHuLoss) of the main head + aux_weight * that of every auxiliary head when
    aux_weight > 0 - ``depth_loss`` with the targets left where they are: the kernels read image b's full-size map
    from ``cache["depth"]`` through ``index``, so no head is resized and no gathered target is written (with
    ``full_size=True`` the heads are up-sampled inside the kernels)."""
    feats = [F.gather_rows(cache[k], index) for k in cache_feature_keys(cache)]
    output, aux_outs = _heads(decoder(feats))
    depth = cache["depth"]
    loss = crit(output, depth, rows=index)
    if aux_weight > 0:
        for aux_out in aux_outs:
            loss = loss + crit(aux_out, depth, rows=index) * aux_weight
    return loss
