"""Candidate training: end-to-end step (task1), decoder-only step on cached
encoder features (task0) and the feature cache itself.

Step semantics follow src/engine/trainer.py (populate_task0 :17-74, train_task0
:78-175, train_segmenter :179-283): LogSoftmax(dim 1) + NLL(ignore 255, mean over
valid pixels), auxiliary heads weighted by ``aux_weight``, per-sub-module
gradient-norm clipping, separate encoder / decoder optimisers, optional Polyak
averaging, one host sync per step for the loss value.  Differences are confined
to where the work runs: forward, backward and loss are nasseg HIP kernels;
gradients of data-parallel replicas are all-reduced over RCCL before clipping.
"""
import contextlib
import logging
import os
import time
import weakref

import numpy as np
import torch
from torch import nn

from .. import functional as F
from ..helpers.utils import AverageMeter, try_except
from ..nn.losses import BerHuLoss, SegmCrossEntropy
from ..nn.modules import TREE_VERSION
from . import graphed
from .trainer_common import (cache_feature_keys, check_cache_rows, require_full_size_labels, task0_depth_loss,
                             task0_loss, task1_depth_loss, task1_loss)
from .trainer_common import clip_and_step as _clip_and_step
from .trainer_common import inner as _inner

logger = logging.getLogger(__name__)

# NASSEG_NATIVE_KD=0: the distillation term of the decoder-only step is always the caller's kd_crit, launched from the
# host (A/B measurements); otherwise an nn.MSELoss() runs fused with the softmax/NLL (``native_kd``)
NATIVE_KD = os.environ.get("NASSEG_NATIVE_KD", "1") != "0"


def _set_stage(loader, stage):
    ds = getattr(loader, "dataset", None)
    if ds is None:
        return
    try:
        ds.set_stage(stage)
    except AttributeError:
        sub = getattr(ds, "dataset", None)
        if sub is not None and hasattr(sub, "set_stage"):
            sub.set_stage(stage)


def _freeze_bn(module):
    for m in module.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.eval()


def _ignore_index(segm_crit):
    return int(getattr(segm_crit, "ignore_index", 255))


def _to_device_image(image, device):
    # fp32 like the reference; a loader that already yields bfloat16 images selects the bf16
    # activation-storage twins of every kernel (include/nasseg.h)
    dtype = torch.bfloat16 if image.dtype == torch.bfloat16 else torch.float32
    return image.to(device=device, dtype=dtype, non_blocking=True).contiguous(
        memory_format=torch.channels_last)


def _model_device(module):
    return next(module.parameters()).device


def _labels(mask, device):
    if mask.dtype not in (torch.uint8, torch.int64):
        mask = mask.to(torch.int64)
    return mask.to(device, non_blocking=True)


def _depth_crit(segm_crit):
    """the criterion itself when it selects the depth step (an nn.BerHuLoss: fp32 full-size targets, masked berHu
    at the prediction's size or, with ``full_size=True``, at the target's), else None: softmax/NLL on class labels,
    as ever"""
    return segm_crit if isinstance(segm_crit, BerHuLoss) else None


_MAPPED_CRITS = weakref.WeakKeyDictionary()  # nn.NLLLoss with class weights -> its SegmCrossEntropy


def _segm_crit(segm_crit, device=None):
    """the criterion that replaces the plain softmax/NLL of every head, else None (F.log_softmax_nll with the
    criterion's ``ignore_index``, as ever).  An nn.SegmCrossEntropy with class weights, hard-example selection, a
    region-overlap term or a Lovasz-Softmax term, or one that takes the loss at the labels' full size
    (``full_size=True``), is that criterion itself; an nn.NLLLoss (nn.NLLLoss2d where torch has it) with ``weight`` and
    mean reduction - the one-line change to src/main_search.py:435 - is mapped to the equivalent SegmCrossEntropy,
    once per criterion and weight tensor.  ``device``: the weights are made fp32 there now (not inside a step being recorded)."""
    crit = None
    if isinstance(segm_crit, SegmCrossEntropy):
        if (segm_crit.weight is not None or segm_crit.selects or segm_crit.region is not None
                or segm_crit.lovasz_weight is not None or segm_crit.full_size):
            crit = segm_crit
    elif (isinstance(segm_crit, nn.NLLLoss) and segm_crit.weight is not None
          and getattr(segm_crit, "reduction", "mean") == "mean"):
        key = (id(segm_crit.weight), int(segm_crit.ignore_index))
        hit = _MAPPED_CRITS.get(segm_crit)
        if hit is None or hit[0] != key:
            hit = (key, SegmCrossEntropy(weight=segm_crit.weight.detach(), ignore_index=segm_crit.ignore_index))
            _MAPPED_CRITS[segm_crit] = hit
        crit = hit[1]
    if crit is not None and device is not None:
        crit.prepare(device)
    return crit


def _depth_target(mask, device):
    """a depth map goes to the device as it is - fp32 (B, H, W), holes (0 / NaN / inf) included"""
    return mask.to(device=device, dtype=torch.float32, non_blocking=True)


def _polyak_update(params, avg_param, decay):
    with torch.no_grad():
        for p, avg_p in zip(params, avg_param):
            avg_p.mul_(decay).add_(p.data, alpha=1.0 - decay)


def _polyak(module, avg_param, decay):
    """Polyak averaging after a step: one nasseg_polyak launch for all of ``module``'s parameters
    (engine/optim_native.py: polyak_update) where they qualify and NASSEG_NATIVE_OPTIM is not 0, else
    ``_polyak_update``"""
    from .optim_native import polyak_update

    if not polyak_update(module, lambda: list(module.parameters()), avg_param, decay):
        _polyak_update(module.parameters(), avg_param, decay)


def native_kd(kd_crit, kd_y, out_size):
    """Is the distillation term ``kd_crit(output, kd_y)`` of the decoder-only step computed by
    F.log_softmax_nll_mse, fused with the softmax/NLL (and, with the step, replayed from a hipGraph)?  Only for
    exactly ``nn.MSELoss(reduction="mean")`` - what src/main_search.py:455-458 makes - and an fp32 4-D teacher cache
    of the logits' size that needs no gradient.  Anything else (another criterion, a subclass, a plain function,
    another reduction) keeps being called as the caller wrote it."""
    return (NATIVE_KD and type(kd_crit) is nn.MSELoss and kd_crit.reduction == "mean" and torch.is_tensor(kd_y)
            and kd_y.dtype == torch.float32 and kd_y.dim() == 4 and tuple(kd_y.shape[2:]) == tuple(out_size)
            and not kd_y.requires_grad)


def _zero_grads(segmenter, optimisers):
    """every ``param.grad`` back to None (not zeros): deferred_wgrad relies on autograd ADOPTING
    the fresh gradient tensors of backward"""
    if hasattr(segmenter, "attach_flat_grads") and getattr(segmenter, "world_size", 1) > 1:
        segmenter.attach_flat_grads()
    else:
        for o in optimisers:
            if o is not None:
                o.zero_grad(set_to_none=True)


def _distributed(segmenter):
    return getattr(segmenter, "world_size", 1) > 1


def _loss_value(segmenter, loss):
    """the per-step host synchronisation (``loss.item()`` in the reference); data parallel, the
    same copy brings the peers' status: PeerFailure if one of them failed in this step"""
    if _distributed(segmenter):
        return segmenter.check_peers(loss)
    return loss.item()


def _syncs(segmenter):
    return getattr(segmenter, "sync_count", 0)


def _tell_peers(segmenter, exc, syncs_before=None, last_step=False):
    """Data parallel, this rank is leaving its step loop with ``exc``: take part - once per
    failure - in the gradient collective its peers are (or will be) waiting in, with zeros and
    the failure status, so that they abandon the candidate too (RankParallel's failure
    protocol).  ``syncs_before``: segmenter.sync_count at the start of the step - if this rank
    has already joined the step's collective (the failure came later: clipping, the optimiser)
    the flag reaches the peers in the NEXT step's collective and they all stop there; after the
    epoch's last step there is no such collective and the flag goes into the end-of-epoch handshake the
    peers are about to make (RankParallel.epoch_status).  A PeerFailure needs no telling: every healthy
    rank raised it at the same point."""
    from .segmenter import PeerFailure

    if not _distributed(segmenter) or isinstance(exc, PeerFailure) or getattr(exc, "_nasseg_peers_told", False):
        return
    try:
        exc._nasseg_peers_told = True
    except AttributeError:
        pass
    if last_step and syncs_before is not None and _syncs(segmenter) > syncs_before:
        segmenter.epoch_status(failed=True)  # (the peers are on their way to the end-of-epoch handshake)
        return
    segmenter.sync_gradients(failed=True)


@contextlib.contextmanager
def _step_failure(segmenter):
    """the inner step: a failure before this rank joined the step's gradient collective is told to the peers
    waiting in it; a later one - clipping, the optimiser - is the caller's to announce (the epoch loop)"""
    syncs = _syncs(segmenter)
    try:
        yield
    except Exception as e:
        if _syncs(segmenter) == syncs:
            _tell_peers(segmenter, e)
        raise


def _as_rank_failure(segmenter, exc):
    """what the step loop re-raises: data parallel, an exception that ``try_except`` would let through (not
    a RuntimeError) becomes a RankFailure, so that this rank scores the candidate 0 like the peers it just
    told - instead of ending its process while they go on to the next collective"""
    from .segmenter import RankFailure

    if not _distributed(segmenter) or isinstance(exc, RuntimeError):
        return exc
    wrapped = RankFailure("{}: {}".format(type(exc).__name__, exc))
    wrapped.__cause__ = exc
    return wrapped


def _epoch_handshake(segmenter):
    """after the last step of a training epoch (data parallel only): see RankParallel.epoch_status"""
    if _distributed(segmenter):
        segmenter.epoch_status()


def _agreed_count(segmenter, n):
    """the smallest ``n`` over the data-parallel ranks (loaders / cache shards of unequal length
    would otherwise issue different numbers of gradient all-reduces); ``n`` itself otherwise"""
    if not _distributed(segmenter) or n is None:
        return n
    import torch.distributed as dist

    t = torch.tensor([int(n)], device=_model_device(_inner(segmenter)), dtype=torch.int64)
    if dist.get_backend(getattr(segmenter, "process_group", None)) == "gloo":
        t = t.cpu()
    dist.all_reduce(t, op=dist.ReduceOp.MIN, group=getattr(segmenter, "process_group", None))
    return int(t.item())


def _replays(segmenter, device, n_pixels):
    """does this step run as a hipGraph replay?  (device memory only; engine/graphed.py: auto_graph)"""
    return device.type == "cuda" and graphed.auto_graph(segmenter, n_pixels)


def _bn_modes(module):
    return tuple(m.training for m in module.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm))


_STEPPERS_PER_CANDIDATE = 2  # captured shapes kept per candidate (the usual batch + a last, smaller one)


def _trainable_signature(params, optimisers):
    """what a captured graph has baked in besides shapes: which parameters receive gradients and
    which tensors the optimisers step on (frozen / unfrozen parameters or edited param_groups
    between epochs need a new capture)"""
    return (tuple(p.requires_grad for p in params),
            tuple(tuple(id(q) for g in o.param_groups for q in g["params"]) for o in optimisers if o is not None))


def _cached_stepper(owner, slot, base_key, shape_key, build):
    """The hipGraph steppers of one candidate: ``base_key`` = everything a capture depends on
    except the batch's shape (optimisers, module tree, BatchNorm modes, trainable set ...) - when
    it changes all steppers are dropped; ``shape_key`` selects among at most
    _STEPPERS_PER_CANDIDATE captured shapes.  A shape beyond that (or one whose capture failed
    once) returns None: that batch is launched from the host instead of paying two warm-up
    passes and a capture for a batch that comes once per epoch."""
    ent = getattr(owner, slot, None)
    if ent is None or ent[0] != base_key:
        ent = (base_key, {})
        setattr(owner, slot, ent)
    steppers = ent[1]
    if shape_key in steppers:
        stepper = steppers[shape_key]
        if stepper is None or not stepper.stale():
            return stepper
        # (optimisers inside the graph and a schedule moved lr / weight decay / a clip norm: those are recorded by
        #  value - record the step again instead of failing in the middle of an epoch)
        del steppers[shape_key]
    if len(steppers) >= _STEPPERS_PER_CANDIDATE:
        return None
    try:
        stepper = build()
    except RuntimeError as e:  # e.g. HIP out of memory while capturing: launch from the host
        logger.warning(" hipGraph capture failed (%s): launching from the host", e)
        stepper = None
    steppers[shape_key] = stepper
    return stepper


def _task0_stepper(Xy_train, segmenter, optim_dec, batch_size, ignore, dec_grad_clip, aux_weight, kd_coeff=None,
                   segm_crit=None, depth_crit=None):
    """kd_coeff: None - no distillation term; else the coefficient of the fused nn.MSELoss term (``native_kd``);
    segm_crit: ``_segm_crit``'s; depth_crit: the nn.BerHuLoss of the depth step on a depth cache"""
    model = _inner(segmenter)
    base = (TREE_VERSION[0], id(optim_dec), ignore, dec_grad_clip, aux_weight, _bn_modes(model.decoder),
            _trainable_signature(list(model.decoder.parameters()), (optim_dec,)))
    if kd_coeff is not None:
        base = base + (("kd_mse", float(kd_coeff)),)
    extra = {}
    if segm_crit is not None:  # (threshold, min_kept and keep_fraction are kernel arguments: recorded by value)
        base = base + (segm_crit.config(),)
        extra["segm_crit"] = segm_crit
    if depth_crit is not None:  # (the loss kind; valid_min and valid_max are kernel arguments: recorded by value)
        base = base + ((id(depth_crit),) + depth_crit.config(),)
        extra["depth_crit"] = depth_crit
    shape = (batch_size, tuple((k, v.data_ptr(), tuple(v.shape)) for k, v in Xy_train.items() if k != "out_size"))
    return _cached_stepper(model, "_nasseg_task0_stepper", base, shape, lambda: graphed.GraphedTask0Step(
        Xy_train, segmenter, optim_dec, batch_size, ignore, dec_grad_clip, aux_weight, kd_coeff=kd_coeff, **extra))


def _segmenter_stepper(segmenter, image, target, optim_enc, optim_dec, ignore, enc_grad_clip, dec_grad_clip,
                       aux_weight, depth_crit=None, segm_crit=None):
    model = _inner(segmenter)
    base = (TREE_VERSION[0], id(optim_enc), id(optim_dec), ignore, enc_grad_clip, dec_grad_clip, aux_weight,
            _bn_modes(model), _trainable_signature(list(model.parameters()), (optim_enc, optim_dec)))
    extra = {}
    if depth_crit is not None:  # (the loss kind, and what the recorded launches carry by value)
        base = base + ((id(depth_crit),) + depth_crit.config(),)
        extra["depth_crit"] = depth_crit
    if segm_crit is not None:
        base = base + (segm_crit.config(),)
        extra["segm_crit"] = segm_crit
    shape = (tuple(image.shape), image.dtype, tuple(target.shape), target.dtype)
    return _cached_stepper(model, "_nasseg_task1_stepper", base, shape, lambda: graphed.GraphedSegmenterStep(
        segmenter, image, target, optim_enc, optim_dec, ignore, enc_grad_clip, dec_grad_clip, aux_weight, **extra))


@try_except
def populate_task0(segmenter, train_loader, kd_net, n_train, do_kd=False, task="segm", full_size_labels=False):
    """Run the encoder (eval, no grad, one image at a time) over ``n_train``
    samples and keep its feature maps, the nearest-resized labels and optionally
    the teacher's logits on the device.  Returns the cache dict
    {0..S-1: (N,C,h,w), 'y': (N,h,w) int64, ['kd_y'], 'out_size': (h,w)}.

    The cache is DEVICE-RESIDENT and NHWC: every entry keeps the reference's (N, C, h, w) shape
    and is stored channels_last, pre-allocated for ``n_train`` samples on the first batch and
    filled in place by copy kernels (no list of slices, no torch.stack, no layout change), so
    that a training step gathers its batch with one nasseg_gather_rows per entry.  Data
    parallel, every rank caches the samples of ITS loader: the cache is sharded.

    task="depth": the masks are depth maps; instead of 'y' the cache gets 'depth': (N, H, W) fp32, the loader's maps
    as they arrive - full size, holes (0 / NaN / inf) included, bit for bit, nothing resized: the berHu kernels of
    the decoder-only depth step read them in place through the batch's row index (``train_task0`` with an
    nn.BerHuLoss).  All maps must share one (H, W) - the cache is one tensor - and there is no distillation term for
    depth: otherwise ValueError.

    full_size_labels=True (task="segm"): beside 'y' the cache gets 'y_full': (N, H, W), the loader's masks as they go
    to the device - uint8 or int64, full size, bit for bit, nothing resized: the full-size cross-entropy of the
    decoder-only step reads them in place through the batch's row index (``train_task0`` with an
    nn.SegmCrossEntropy(full_size=True)).  All masks must share one (H, W), else ValueError; every other entry is what
    it is without the flag.  With task="depth" (whose cache is full-size as it is) a ValueError."""
    if task not in ("segm", "depth"):
        raise ValueError("populate_task0: task must be 'segm' or 'depth' (got {!r})".format(task))
    if full_size_labels and task == "depth":
        raise ValueError("populate_task0: full_size_labels belongs to task=\"segm\" (the depth cache holds full-size "
                         "maps as it is)")
    if task == "depth" and do_kd:
        raise ValueError("populate_task0: there is no distillation term for depth (do_kd with task=\"depth\")")
    cache = {}
    segmenter.eval()
    _set_stage(train_loader, "train")
    if hasattr(train_loader, "batch_sampler") and train_loader.batch_sampler is not None:
        train_loader.batch_sampler.batch_size = 1
    model = _inner(segmenter)
    device = _model_device(model)

    def slot(key, like, seen, b):
        """rows [seen, seen+b) of cache[key] (allocated on first use for n_train + b - 1 rows:
        the loop below stops at the first batch that reaches n_train)"""
        if key not in cache:
            shape = (n_train + b - 1,) + tuple(like.shape[1:])
            cache[key] = (torch.empty(shape, device=device, dtype=like.dtype, memory_format=torch.channels_last)
                          if like.dim() == 4 else torch.empty(shape, device=device, dtype=like.dtype))
        return cache[key][seen:seen + b]

    def store(key, t, seen):
        F.copy_into(slot(key, t, seen, t.shape[0]), t)

    with torch.no_grad():
        seen = 0
        for sample in train_loader:
            image = _to_device_image(sample["image"], device)
            b = image.size(0)
            feats = model.encoder(image)
            for i, f in enumerate(feats):
                store(i, f, seen)
            size = feats[0].size()[2:]
            if task == "depth":
                depth = _depth_target(sample["mask"], device)
                if depth.dim() != 3 or depth.shape[0] != b or (
                        "depth" in cache and tuple(depth.shape[1:]) != tuple(cache["depth"].shape[1:])):
                    raise ValueError("populate_task0: depth maps of one size (b, H, W) expected - the cache is one "
                                     "tensor (got {}{})".format(tuple(depth.shape), ", cached {}".format(
                                         tuple(cache["depth"].shape[1:])) if "depth" in cache else ""))
                slot("depth", depth, seen, b).copy_(depth)  # (a plain device copy: every bit, NaN payloads included)
            else:
                labels = _labels(sample["mask"], device)
                F.nearest_label_resize(labels, size, out=slot(
                    "y", torch.empty((1,) + tuple(size), dtype=torch.int64), seen, b))
                if full_size_labels:
                    if labels.dim() != 3 or labels.shape[0] != b or (
                            "y_full" in cache and (tuple(labels.shape[1:]) != tuple(cache["y_full"].shape[1:])
                                                   or labels.dtype != cache["y_full"].dtype)):
                        raise ValueError("populate_task0: full-size labels of one size (b, H, W) and one dtype "
                                         "expected - the cache is one tensor (got {} {}{})".format(
                                             labels.dtype, tuple(labels.shape), ", cached {} {}".format(
                                                 cache["y_full"].dtype, tuple(cache["y_full"].shape[1:]))
                                             if "y_full" in cache else ""))
                    slot("y_full", labels, seen, b).copy_(labels)  # (a plain device copy: every bit)
            if do_kd:
                # (the teacher runs in fp32 whatever the candidate's activation storage)
                store("kd_y", F.bilinear_resize(kd_net(image if image.dtype == torch.float32 else image.float()),
                                                size), seen)
            seen += b
            if seen >= n_train:
                logger.info(" Populated Xy_train, N = {}".format(seen))
                for k in list(cache):
                    cache[k] = cache[k][:seen]
                cache["out_size"] = size
                if task == "depth":
                    d = cache["depth"]
                    logger.info(" Depth cache: {} maps of {} x {}, fp32, {:.1f} MiB".format(
                        d.shape[0], d.shape[1], d.shape[2], d.numel() * d.element_size() / 2.0 ** 20))
                if full_size_labels:
                    d = cache["y_full"]
                    logger.info(" Full-size label cache: {} maps of {} x {}, {}, {:.1f} MiB".format(
                        d.shape[0], d.shape[1], d.shape[2], str(d.dtype).replace("torch.", ""),
                        d.numel() * d.element_size() / 2.0 ** 20))
                break
        else:
            for k in list(cache):  # (loader exhausted first - as in the reference, no 'out_size' then)
                cache[k] = cache[k][:seen]
    return cache


def make_task0_step(Xy_train, segmenter, optim_dec, batch_size, ignore_index=255, dec_grad_clip=0.0, aux_weight=0,
                    freeze_bn=False, do_kd=False, kd_coeff=0.0, kd_crit=None, segm_crit=None, depth_crit=None):
    """step(batch_idx) -> device loss: one decoder-only training step on the cache rows
    ``batch_idx`` (a host array of ``batch_size`` indices).  Small batches are launch-bound, so the
    step is replayed from a hipGraph where that wins (engine/graphed.py: auto_graph; the stepper
    lives with the model for as long as cache, decoder, BatchNorm modes, optimiser and distillation
    coefficient stay the same); otherwise - and always with a distillation criterion other than
    ``nn.MSELoss()`` (``native_kd``), or data parallel - it is launched from the host: gather the
    batch (one kernel per cache entry), decoder forward, bilinear resize to ``out_size``,
    softmax/NLL [+ kd_coeff * MSE to the cached teacher logits, one fused kernel] (+ aux heads),
    backward, [all-reduce], clip, optimiser.
    ``segm_crit`` (``_segm_crit``'s: class weights / hard-example selection / region term): the loss of every head; with
    distillation as well the step is launched from the host and ``kd_crit`` is called as written.
    ``depth_crit`` (an nn.BerHuLoss, on a cache with a 'depth' entry - populate_task0(task="depth")): the depth step
    instead - gather the feature rows, decoder, the criterion of every head against the full-size maps of the cache,
    read in place through the batch's rows (trainer_common.task0_depth_loss): nothing is resized, no target batch is
    gathered; replayed or launched from the host by the same rule.
    A full-size ``segm_crit`` (nn.SegmCrossEntropy(full_size=True), on a cache with a 'y_full' entry -
    populate_task0(full_size_labels=True); without one a ValueError): likewise, every head at its own size against
    the full-size labels of the cache, read in place through the batch's rows (trainer_common.task0_full_size_loss);
    with distillation the step is launched from the host and ``kd_crit`` meets the main head resized to ``out_size``."""
    require_full_size_labels("make_task0_step", Xy_train, segm_crit)
    decoder = _inner(segmenter).decoder
    feat = Xy_train[cache_feature_keys(Xy_train)[0]]
    out_size = tuple(Xy_train["out_size"])
    device = Xy_train["depth" if depth_crit is not None else "y"].device
    dec_params = list(decoder.parameters())
    pack_memo = F.PackMemo()
    n_pixels = batch_size * int(feat.shape[2]) * int(feat.shape[3]) * 16
    fused_kd = do_kd and segm_crit is None and native_kd(kd_crit, Xy_train.get("kd_y"), out_size)
    extra = {} if segm_crit is None else {"segm_crit": segm_crit}
    if depth_crit is not None:
        if "depth" not in Xy_train or do_kd or segm_crit is not None:
            raise ValueError("make_task0_step: depth_crit needs a depth cache (populate_task0(task=\"depth\")) and "
                             "goes with neither distillation nor a segmentation criterion")
        extra = {"depth_crit": depth_crit}
    if (not do_kd or fused_kd) and _replays(segmenter, device, n_pixels):
        stepper = _task0_stepper(Xy_train, segmenter, optim_dec, batch_size, ignore_index, dec_grad_clip,
                                 aux_weight, kd_coeff if fused_kd else None, **extra)
        if stepper is not None:
            return stepper.step

    def step(batch_idx):
        with _step_failure(segmenter):
            idx = torch.as_tensor(batch_idx, dtype=torch.int64)
            check_cache_rows(idx, Xy_train, "train_task0")
            idx = idx.to(device, non_blocking=True)
            with F.packed_once(pack_memo):  # (one weight re-pack launch per step)
                if depth_crit is not None:
                    loss = task0_depth_loss(Xy_train, idx, decoder, depth_crit, aux_weight)
                else:
                    loss = task0_loss(Xy_train, idx, decoder, ignore_index, aux_weight, kd_coeff if do_kd else None,
                                      kd_crit, fused_kd, **extra)
                _zero_grads(segmenter, (optim_dec,))
                with F.deferred_wgrad(params=dec_params, second_stream=False):  # (crops of the feature cache: launch-bound)
                    loss.backward()
            if _distributed(segmenter):
                # the feature cache is sharded: every rank steps on its own cached samples and the
                # decoder gradients are averaged (the reference runs this stage on one GPU)
                segmenter.sync_gradients()
            _clip_and_step([(dec_params, dec_grad_clip, optim_dec)])
        return loss

    return step


@try_except
def train_task0(Xy_train, segmenter, optim_dec, epoch, segm_crit, kd_crit, batch_size, freeze_bn,
                do_kd, kd_coeff, dec_grad_clip, do_polyak, avg_param=None, polyak_decay=0.9,
                aux_weight=0):
    """Decoder-only epoch over the cached encoder features (trainer.py:78-175).
    An nn.BerHuLoss on a cache with a 'depth' entry (populate_task0(task="depth")): the decoder-only DEPTH epoch.
    An nn.SegmCrossEntropy(full_size=True) on a cache with a 'y_full' entry (populate_task0(full_size_labels=True)):
    the loss of every head is taken at the labels' full size, where ``validate`` scores."""
    depth_crit = _depth_crit(segm_crit)
    depth_cache = "depth" in Xy_train
    if depth_crit is not None and not depth_cache:
        raise ValueError("train_task0: on this cache depth candidates are trained end to end only (train_segmenter) - "
                         "it holds class labels, not depth maps; populate_task0(..., task=\"depth\") makes the cache "
                         "of full-size depth maps a BerHuLoss trains the decoder on")
    if depth_cache and depth_crit is None:
        raise ValueError("train_task0: a depth cache (populate_task0(task=\"depth\")) needs an nn.BerHuLoss as "
                         "segm_crit (got {!r})".format(segm_crit))
    if depth_cache and do_kd:
        raise ValueError("train_task0: there is no distillation term for depth (do_kd with a depth cache)")
    if depth_crit is None:
        require_full_size_labels("train_task0", Xy_train, segm_crit)
    decoder = _inner(segmenter).decoder
    # (data parallel the cache is sharded: every rank must issue the same number of gradient
    #  all-reduces, so the shards agree on the smallest of their sizes first)
    n_examples = _agreed_count(segmenter, Xy_train[0].size(0))
    batch_size = min(batch_size, n_examples)
    n_passes = n_examples // batch_size
    indices = np.arange(n_examples)
    batch_time, losses = AverageMeter(), AverageMeter()
    decoder.train()
    if freeze_bn:
        _freeze_bn(decoder)
    np.random.shuffle(indices)
    step = make_task0_step(Xy_train, segmenter, optim_dec, batch_size, _ignore_index(segm_crit), dec_grad_clip,
                           aux_weight, freeze_bn, do_kd, kd_coeff, kd_crit,
                           None if depth_cache else _segm_crit(segm_crit, Xy_train["y"].device),
                           **({"depth_crit": depth_crit} if depth_cache else {}))
    for i in range(n_passes):
        start = time.time()
        syncs = _syncs(segmenter)
        try:
            loss = step(indices[i * batch_size:(i + 1) * batch_size])
        except Exception as e:
            _tell_peers(segmenter, e, syncs, i == n_passes - 1)
            raise _as_rank_failure(segmenter, e)
        losses.update(_loss_value(segmenter, loss))
        batch_time.update(time.time() - start)
        if do_polyak:
            _polyak(decoder, avg_param, polyak_decay)
    _epoch_handshake(segmenter)
    logger.info(" Train epoch: {}\tAvg. Loss: {:.3f}\tAvg. Time: {:.3f}".format(
        epoch, losses.avg, batch_time.avg))


def segmenter_step(segmenter, image, target, optim_enc, optim_dec, ignore_index=255,
                   enc_grad_clip=0.0, dec_grad_clip=0.0, aux_weight=-1, depth_crit=None, segm_crit=None):
    """One end-to-end training step on device tensors; returns the (device) loss.

    forward -> nearest-resize labels to the logits' size -> fused log-softmax/NLL
    (+ weighted aux heads) -> backward -> gradient all-reduce (if data parallel)
    -> per-sub-module norm clipping -> optimiser steps.
    ``depth_crit`` (an nn.BerHuLoss): the depth step instead - ``target`` is the fp32 (B, H, W) depth map and the
    loss is the masked berHu of every head against it (trainer_common.task1_depth_loss).
    ``segm_crit``: any segmentation criterion - one with class weights, selection or a region term (``_segm_crit``)
    is the loss of every head, anything else leaves the plain softmax/NLL with ``ignore_index``.
    """
    segm_crit = _segm_crit(segm_crit, image.device)
    model = _inner(segmenter)
    cached = getattr(model, "_nasseg_step_params", None)
    if cached is None or cached[0] != TREE_VERSION[0]:
        # a candidate's module tree is fixed: walk it once, not every step (and again when a
        # sub-module was swapped - TemplateDecoder._reset_clf bumps the version)
        cached = (TREE_VERSION[0], (list(model.encoder.parameters()), list(model.decoder.parameters())))
        model._nasseg_step_params = cached
        model._nasseg_pack_memo = F.PackMemo()
    groups = cached[1]
    with _step_failure(segmenter):
        # the parameters are constant until the optimiser steps below: all chains' weights are
        # re-packed by one launch at the start of the step
        with F.packed_once(model._nasseg_pack_memo):
            if depth_crit is not None:
                loss = task1_depth_loss(segmenter, image, target, depth_crit, aux_weight)
            else:
                loss = task1_loss(segmenter, image, target, ignore_index, aux_weight, segm_crit)
            _zero_grads(segmenter, (optim_enc, optim_dec))
            # gradients were just cleared: the second stages of all weight-gradient reductions run
            # batched when backward is through
            # (a step small enough to be worth replaying from a hipGraph is launch-bound when it is not: no second stream)
            side = image.shape[0] * image.shape[2] * image.shape[3] > graphed.AUTO_GRAPH_MAX_PIXELS
            with F.deferred_wgrad(params=groups[0] + groups[1], second_stream=side):
                loss.backward()
        finish_step(segmenter, groups, optim_enc, optim_dec, enc_grad_clip, dec_grad_clip)
    return loss


def finish_step(segmenter, groups, optim_enc, optim_dec, enc_grad_clip, dec_grad_clip):
    """What follows backward in a training step (src/engine/trainer.py:255-268): average the
    gradients over the data-parallel ranks (one RCCL all-reduce; the reference's DataParallel
    sums replica gradients on GPU 0), clip the encoder's and the decoder's gradient norms
    separately, step both optimisers.  groups = (encoder parameters, decoder parameters)."""
    if hasattr(segmenter, "sync_gradients"):
        segmenter.sync_gradients()
    _clip_and_step([(groups[0], enc_grad_clip, optim_enc), (groups[1], dec_grad_clip, optim_dec)])


@try_except
def train_segmenter(segmenter, train_loader, optim_enc, optim_dec, epoch, segm_crit, freeze_bn,
                    enc_grad_clip, dec_grad_clip, do_polyak, print_every=10, aux_weight=-1,
                    avg_param=None, polyak_decay=0.99):
    """End-to-end epoch (trainer.py:179-283)."""
    _set_stage(train_loader, "train")
    segmenter.train()
    if freeze_bn:
        _freeze_bn(segmenter)
    batch_time, losses = AverageMeter(), AverageMeter()
    ignore = _ignore_index(segm_crit)
    depth_crit = _depth_crit(segm_crit)
    extra = {} if depth_crit is None else {"depth_crit": depth_crit}  # (any other criterion: exactly as ever)
    device = _model_device(_inner(segmenter))
    weighted = None if depth_crit is not None else _segm_crit(segm_crit, device)
    if weighted is not None:  # (class weights / hard-example selection: the loss of every head)
        extra = {"segm_crit": weighted}
    # data parallel: the ranks agree on the number of steps (loaders of unequal length would leave
    # the longer ones waiting in an all-reduce), and a rank that fails ANYWHERE in its step - the
    # loader, the copy to the device, the optimiser - tells its peers before it leaves (_tell_peers)
    n_steps = _agreed_count(segmenter, len(train_loader) if hasattr(train_loader, "__len__") else None)
    batches = iter(train_loader)
    i = 0
    while n_steps is None or i < n_steps:
        start = time.time()
        syncs = _syncs(segmenter)
        try:
            try:
                sample = next(batches)
            except StopIteration:
                break
            image = _to_device_image(sample["image"], device)
            target = _labels(sample["mask"], device) if depth_crit is None else _depth_target(sample["mask"], device)
            stepper = None
            if _replays(segmenter, device, image.shape[0] * image.shape[2] * image.shape[3]):
                # launch-bound sizes: forward + loss + backward replayed from a hipGraph captured on
                # this candidate's first batch (bit-identical to the eager step)
                stepper = _segmenter_stepper(segmenter, image, target, optim_enc, optim_dec, ignore,
                                             enc_grad_clip, dec_grad_clip, aux_weight, **extra)
            if stepper is not None:
                loss = stepper.step(image, target)
            else:
                loss = segmenter_step(segmenter, image, target, optim_enc, optim_dec, ignore,
                                      enc_grad_clip, dec_grad_clip, aux_weight, **extra)
            if do_polyak:
                _polyak(segmenter, avg_param, polyak_decay)
        except Exception as e:
            _tell_peers(segmenter, e, syncs, n_steps is not None and i == n_steps - 1)
            raise _as_rank_failure(segmenter, e)
        losses.update(_loss_value(segmenter, loss))
        batch_time.update(time.time() - start)
        if i % print_every == 0:
            logger.info(" Train epoch: {} [{}/{}]\tAvg. Loss: {:.3f}\tAvg. Time: {:.3f}".format(
                epoch, i, len(train_loader), losses.avg, batch_time.avg))
        i += 1
    _epoch_handshake(segmenter)
