"""Criteria the reference has no training loss for: the depth head's, and the segmentation heads' with class
weights and hard-example mining."""
import torch
from torch import nn

from .. import functional as F


class BerHuLoss(nn.Module):
    """Reverse-Huber criterion of a depth head: ``F.berhu_loss_masked`` (absent from the reference; Laina et al.
    2016, eq. 2).  forward(pred (B, 1, h, w), target (B, H, W) fp32 at any size, holes where the target is not
    finite or outside ``(valid_min, valid_max]``) -> 0-dim loss.  Handed to ``engine.trainer.train_segmenter`` as
    ``segm_crit`` it selects the depth step.
    ``full_size=True``: ``F.berhu_loss_upsampled`` instead - the prediction is up-sampled bilinearly to the target
    inside the kernels and the loss is taken over the TARGET's valid pixels, every one of them: the resolution
    ``validate_depth`` scores at (without it, each prediction pixel sees the one target pixel nearest sampling
    picks).  The training steps hand every head the same full-size target either way.
    ``silog_weight`` / ``grad_weight`` (numbers; None: no such term): the loss becomes ``F.depth_criterion`` -
    ``berhu_weight * berHu + silog_weight * D + grad_weight * L_gm`` over the same valid pixels, with
    r = ln max(pred, pred_min) - ln target: D = mean(r^2) - silog_lambda * mean(r)^2 is the scale-invariant log term
    (Eigen et al. 2014; ``validate_depth``'s ``silog`` is sqrt(D) at silog_lambda = 1 - the root is left out so that
    the gradient stays finite at a perfect prediction) and L_gm the gradient-matching term over ``grad_scales``
    strides 1, 2, 4, ... (MegaDepth, MiDaS), which rewards sharp depth edges: the surrogates of what a depth
    candidate is scored on.  A pixel with pred <= pred_min gets no gradient from the two terms; they sit on top of
    the berHu, which still pulls such a pixel up.  The terms are defined at the prediction's size only: with
    ``full_size=True`` they are a ValueError, and so are ``valid_min < 0``, a ``silog_lambda`` outside [0, 1],
    ``grad_scales`` outside 1..8, ``pred_min <= 0`` and a negative weight.  With both weights None the criterion
    is, launch for launch, the one it was without them."""

    def __init__(self, valid_min=0.0, valid_max=float("inf"), full_size=False, *, berhu_weight=1.0, silog_weight=None,
                 silog_lambda=0.5, grad_weight=None, grad_scales=4, pred_min=1e-3):
        super(BerHuLoss, self).__init__()
        self.valid_min = float(valid_min)
        self.valid_max = float(valid_max)
        self.full_size = bool(full_size)
        self.berhu_weight = berhu_weight
        self.silog_weight = silog_weight
        self.silog_lambda = silog_lambda
        self.grad_weight = grad_weight
        self.grad_scales = grad_scales
        self.pred_min = pred_min
        if self.has_terms:
            if self.full_size:
                raise ValueError("BerHuLoss: full_size=True has no scale-invariant or gradient-matching term (those "
                                 "terms are defined at the prediction's size only)")
        elif float(berhu_weight) != 1.0:
            raise ValueError("BerHuLoss: berhu_weight weighs the berHu against silog_weight / grad_weight; without "
                             "one of them it would be ignored (got {})".format(berhu_weight))
        # (the logarithms need valid_min >= 0 only where a term takes them)
        F._depth_terms_config("BerHuLoss", self.valid_min if self.has_terms else 0.0, **self._terms())

    @property
    def has_terms(self):
        return self.silog_weight is not None or self.grad_weight is not None

    def _terms(self):
        """the keyword arguments of ``F.depth_criterion`` for the terms this criterion has"""
        return {name: getattr(self, name) for name in ("berhu_weight", "silog_weight", "silog_lambda", "grad_weight",
                                                       "grad_scales", "pred_min")}

    def config(self):
        """what a recorded step carries by value (the stepper cache's key, engine/trainer.py): the loss kind and
        the two bounds, which are kernel arguments - and, with a term, the terms' values, which are too"""
        cfg = ("berhu_up" if self.full_size else "berhu", self.valid_min, self.valid_max)
        if self.has_terms:
            cfg = cfg + (("terms", self.berhu_weight, self.silog_weight, self.silog_lambda, self.grad_weight,
                          self.grad_scales, self.pred_min),)
        return cfg

    def forward(self, pred, target, rows=None):
        """``rows`` (an int64 device tensor, one entry per image): ``target`` is a cache (N, H, W) and image b meets
        ``target[rows[b]]``, read in place (the task0 depth cache)"""
        if self.has_terms:
            return F.depth_criterion(pred, target, self.valid_min, self.valid_max, rows=rows, **self._terms())
        loss = F.berhu_loss_upsampled if self.full_size else F.berhu_loss_masked
        if rows is None:
            return loss(pred, target, self.valid_min, self.valid_max)
        return loss(pred, target, self.valid_min, self.valid_max, rows=rows)

    def extra_repr(self):
        s = "valid_min={}, valid_max={}".format(self.valid_min, self.valid_max)
        if self.full_size:
            s += ", full_size=True"
        if self.has_terms:
            s += ", berhu_weight={}, silog_weight={}, silog_lambda={}, grad_weight={}, grad_scales={}, pred_min={}".format(
                self.berhu_weight, self.silog_weight, self.silog_lambda, self.grad_weight, self.grad_scales,
                self.pred_min)
        return s


class SegmCrossEntropy(nn.Module):
    """LogSoftmax + NLL of (B, C, H, W) logits with class weights and online hard-example mining:
    ``F.cross_entropy_select`` (definition: INTEGRATION.md, "Losses").  forward(logits, target (B, H, W) uint8 or
    int64) -> 0-dim loss.  ``weight``: (C,) class weights, a buffer (made fp32 on the logits' device at first use);
    ``thresh``: pixels whose target probability is below it are hard; ``min_kept`` / ``keep_fraction``: at least so
    many / such a share of the valid pixels are kept.  Selection is active iff one of the three is given and then
    needs ``min_kept >= 1``.  ``thresh=0.7, min_kept=100000``: the usual OHEM cross-entropy;
    ``keep_fraction=0.25, min_kept=1``: top-k bootstrapping.  Handed to ``engine.trainer.train_segmenter`` /
    ``train_task0`` as ``segm_crit`` it is the loss of every head; with neither weights nor selection those steps
    run the plain ``F.log_softmax_nll`` as ever.  ``thresh``, ``min_kept`` and ``keep_fraction`` may be changed
    between steps.
    ``region`` ("jaccard" | "dice" | ("tversky", alpha, beta)): ``region_weight`` times the soft Jaccard / Dice /
    Tversky loss over all valid pixels is added (``F.region_overlap_loss`` with ``smooth=region_smooth,
    classes=region_classes``), computed by the same two passes over the logits - the usual ``CE + lambda * Dice``.
    Such a criterion is the loss of every head even without weights or selection.
    ``lovasz_weight`` (a number; None: no such term): ``lovasz_weight`` times the Lovasz-Softmax loss over all valid
    pixels is added (``F.lovasz_softmax_loss`` with ``classes=lovasz_classes``), sorted on the device inside the same
    autograd node - the usual ``CE + Lovasz``.  Such a criterion, too, is the loss of every head.
    ``full_size=True``: ``F.cross_entropy_upsampled`` instead - ``target`` comes at ANY size (the full-size label
    map), the logits are up-sampled bilinearly to it inside the kernels and the loss, class weights and selection
    included, is taken over the label pixels: the resolution ``validate`` scores at.  The training steps then hand
    every head, at its own size, the labels as they are (nothing is resized).  Such a criterion is the loss of every
    head even without weights or selection; it has no Lovasz term, and a region term only with
    ``region_at="labels"``.  ``train_task0`` takes it on a cache
    made with ``populate_task0(..., full_size_labels=True)``: ``forward(logits, cache, rows=index)`` reads image b's
    labels at ``cache[rows[b]]`` in place (``F.cross_entropy_upsampled(rows=)``).
    ``region_at`` ("logits" | "labels"; needs ``full_size=True`` and a ``region``): where the region term's sums are
    taken.  "labels": over the label pixels, on the up-sampled rows, fused like the cross-entropy
    (``F.cross_entropy_upsampled(region=...)``) - ``CE + lambda * Dice`` where the score is taken, with ``rows=`` as
    well.  "logits" (the default) is the term of ``F.cross_entropy_select``, which a full-size criterion cannot
    have: a ValueError, as before."""

    def __init__(self, weight=None, ignore_index=255, thresh=None, min_kept=0, keep_fraction=0.0, region=None,
                 region_weight=1.0, region_smooth=1.0, region_classes="present", lovasz_weight=None,
                 lovasz_classes="present", full_size=False, region_at="logits"):
        super(SegmCrossEntropy, self).__init__()
        if weight is not None:
            weight = torch.as_tensor(weight)
            if weight.dim() != 1 or weight.numel() == 0:
                raise ValueError("SegmCrossEntropy: weight must be 1-D, one entry per class (got shape {})".format(
                    tuple(weight.shape)))
        self.register_buffer("weight", weight)
        self.ignore_index = int(ignore_index)
        self.thresh = thresh
        self.min_kept = min_kept
        self.keep_fraction = keep_fraction
        self.region = tuple(region) if isinstance(region, list) else region
        self.region_weight = region_weight
        self.region_smooth = region_smooth
        self.region_classes = region_classes
        self.lovasz_weight = lovasz_weight
        self.lovasz_classes = lovasz_classes
        F._segm_config("SegmCrossEntropy", thresh, min_kept, keep_fraction, **self._terms())
        if lovasz_weight is None and lovasz_classes not in ("present", "all"):
            raise ValueError("SegmCrossEntropy: lovasz_classes must be \"present\" or \"all\" (got {!r})".format(
                lovasz_classes))
        if region_at not in ("logits", "labels"):
            raise ValueError("SegmCrossEntropy: region_at must be \"logits\" or \"labels\" (got {!r})".format(region_at))
        if region_at == "labels" and not (full_size and region is not None):
            raise ValueError("SegmCrossEntropy: region_at=\"labels\" takes the region term over the full-size labels "
                             "and needs full_size=True and a region")
        if full_size and (lovasz_weight is not None or (region is not None and region_at != "labels")):
            raise ValueError("SegmCrossEntropy: full_size=True has no region or Lovasz term (those terms are defined "
                             "at the logits' size only; region_at=\"labels\" takes the region term at the labels' "
                             "size)")
        self.full_size = bool(full_size)
        self.region_at = region_at

    def _terms(self):
        """the keyword arguments of ``F.cross_entropy_select`` for the terms this criterion has"""
        names = ()
        if self.region is not None:
            names += ("region", "region_weight", "region_smooth", "region_classes")
        if self.lovasz_weight is not None:
            names += ("lovasz_weight", "lovasz_classes")
        return {name: getattr(self, name) for name in names}

    @property
    def selects(self):
        return self.thresh is not None or self.min_kept > 0 or self.keep_fraction > 0

    def config(self):
        """what a recorded step carries by value or by address (the stepper caches' key, engine/trainer.py)"""
        cfg = ("ce_sel", id(self.weight) if self.weight is not None else None, self.ignore_index, self.thresh,
               self.min_kept, self.keep_fraction)
        if self.region is not None:  # (the term's four values are kernel arguments: recorded by value)
            cfg = cfg + (("region", self.region, self.region_weight, self.region_smooth, self.region_classes),)
        if self.lovasz_weight is not None:
            cfg = cfg + (("lovasz", self.lovasz_weight, self.lovasz_classes),)
        if self.full_size:  # (another loss kind: other launches, labels at another size)
            cfg = cfg + (("full_size",),)
        if self.region_at == "labels":  # (and another again: the region term's own launches)
            cfg = cfg + (("region_at", "labels"),)
        return cfg

    def prepare(self, device):
        """the weights as the kernels read them: fp32, on ``device`` (a float64 or host vector is converted once,
        here - never inside a step that is being recorded)"""
        w = self.weight
        if w is not None and (w.dtype != torch.float32 or w.device != torch.device(device)):
            self.weight = w.to(device=device, dtype=torch.float32)
        return self

    def forward(self, logits, target, rows=None):
        """``rows`` (an int64 device tensor, one entry per image; ``full_size=True`` only): ``target`` is a label
        cache (N, H, W) and image b meets ``target[rows[b]]``, read in place (the task0 cache's ``'y_full'``)"""
        if rows is not None and not self.full_size:
            raise ValueError("SegmCrossEntropy: rows= reads a full-size label cache in place and needs "
                             "full_size=True (at the logits' size the step gathers its labels)")
        self.prepare(logits.device)
        loss = F.cross_entropy_upsampled if self.full_size else F.cross_entropy_select
        if rows is None:
            return loss(logits, target, self.weight, self.ignore_index, self.thresh, self.min_kept,
                        self.keep_fraction, **self._terms())
        return loss(logits, target, self.weight, self.ignore_index, self.thresh, self.min_kept, self.keep_fraction,
                    rows=rows, **self._terms())

    def extra_repr(self):
        s = "classes={}, ignore_index={}, thresh={}, min_kept={}, keep_fraction={}".format(
            None if self.weight is None else self.weight.numel(), self.ignore_index, self.thresh, self.min_kept,
            self.keep_fraction)
        if self.region is not None:
            s += ", region={!r}, region_weight={}, region_smooth={}, region_classes={!r}".format(
                self.region, self.region_weight, self.region_smooth, self.region_classes)
        if self.lovasz_weight is not None:
            s += ", lovasz_weight={}, lovasz_classes={!r}".format(self.lovasz_weight, self.lovasz_classes)
        if self.full_size:
            s += ", full_size=True"
        if self.region_at == "labels":
            s += ", region_at='labels'"
        return s
