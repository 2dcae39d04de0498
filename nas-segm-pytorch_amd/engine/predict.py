"""Prediction: a network on an image -> a label map or a depth map, on the device (the reference's other public use:
tests/test_inference.py and the notebooks under examples/inference/).

The notebooks run ``model(img)[0]`` on ``prepare_img(img)``, copy the logits to the host, resize them with
``cv2.resize(logits, orig_size, interpolation=cv2.INTER_CUBIC)`` and take the argmax (segmentation) or keep the map
(NYUD depth).  ``Predictor`` does the same three steps on the device - ``F.prepare_image`` (nasseg_augment with an
identity plan), the eval forward, ``F.resize_cubic_argmax`` / ``F.resize_cubic`` (csrc/predict.hip) - bit for bit
against that host pipeline restated in numpy (data/datasets.resize_cubic_to); only the uint8 image goes to the
device and only the labels (or the depth map) come back.

Test-time ensemble (``scales=``, ``flip=``): the network runs on the image at several scales and on the mirrored
image (``F.view_image``), and ONE launch (``F.fuse_views``, csrc/ensemble.hip) brings every result back to the
output size, soft-maxes it, averages and takes the argmax - no view is stored at full resolution.  The default,
``scales=(1.0,), flip=False``, is the single forward above, unchanged.

At batch 1 an eval forward is several hundred small launches, so a shape seen twice is recorded into a hipGraph
(``torch.cuda.CUDAGraph``, as engine/graphed.py records training steps) and replayed: one host-to-device copy into
the capture's static uint8 buffer, one replay, one clone of the output.  Replayed and host-launched calls run the
same kernels in the same order: their results are identical.
"""
import collections
import gc
import os
import weakref

import numpy as np
import torch
from torch import nn

from .. import functional as F
from . import graphed

TASKS = ("segm", "depth")
DTYPES = (torch.float32, torch.bfloat16)
MAX_CAPTURES = 4  # hipGraphs one Predictor keeps (least recently used first out); each owns a private memory pool
_SEEN_KEPT = 64   # shapes whose calls `graph="auto"` counts


def ensemble_views(scales, flip, who="Predictor"):
    """The views (scale, mirrored) of a test-time ensemble, in the order their probabilities are added: per scale
    the plain view, then (``flip``) the mirrored one.  Scales: a non-empty sequence of positive finite numbers
    without duplicates; at most F.MAX_VIEWS views."""
    import math

    if not isinstance(flip, (bool, np.bool_)):
        raise ValueError("{}: flip must be True or False (got {!r})".format(who, flip))
    try:
        scales = tuple(float(s) for s in scales)
    except (TypeError, ValueError):
        raise ValueError("{}: scales must be a sequence of numbers (got {!r})".format(who, scales))
    if not scales or any(not math.isfinite(s) or s <= 0 for s in scales):
        raise ValueError("{}: scales must be a non-empty sequence of positive finite numbers (got {!r})".format(
            who, scales))
    if len(set(scales)) != len(scales):
        raise ValueError("{}: a scale is given twice (got {!r})".format(who, scales))
    n = len(scales) * (2 if flip else 1)
    if n > F.MAX_VIEWS:
        raise ValueError("{}: {} views (scales{}), at most {} are fused".format(
            who, n, " x 2 for mirroring" if flip else "", F.MAX_VIEWS))
    return tuple((s, m) for s in scales for m in ((False, True) if flip else (False,)))


def view_inputs(x, views):
    """the network inputs of ``views`` for the normalised image x (B x 3 x H x W): the view (1.0, False) is x
    itself, every other one F.view_image launch"""
    H, W = x.shape[2:]
    return [x if (s == 1.0 and not m) else F.view_image(x, (F.view_size(H, s), F.view_size(W, s)), m)
            for s, m in views]


def _first(output):
    """the logits of a network whose output is logits or (logits, aux ...)"""
    return output[0] if isinstance(output, (tuple, list)) else output


def _check_out_size(out_size):
    if out_size is None or (isinstance(out_size, str) and out_size == "model"):
        return out_size
    try:
        H, W = (int(s) for s in out_size)
        ok = H > 0 and W > 0 and (H, W) == tuple(out_size)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("Predictor: out_size must be None, 'model' or two positive integers (got {!r})".format(
            out_size))
    return (H, W)


class _Capture(object):
    """One shape of one Predictor call, recorded into a hipGraph: ``static`` (input buffer) -> ``output``.  Holds no
    module: parameters and BatchNorm buffers are read by address, ``signature`` says which."""

    def __init__(self, run, static, src, signature):
        self.static = static
        static.copy_(src)
        self.signature = signature
        self.keep = {}              # device tables the recorded launches read (their cache may drop them)
        self.memo = F.PackMemo()    # (owns the packed-weight buffers the graph reads)
        # warm-up outside the capture: lazy initialisation, the tables, the pack plans
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with F.packed_once(self.memo):
                run(static, self.keep)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        # no garbage collection while the stream is capturing (engine/graphed.py: a collected cycle may free another
        # graph inside the capture)
        self.graph = torch.cuda.CUDAGraph()
        gc.collect()
        enabled = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(self.graph):
                with F.packed_once(self.memo):
                    self.output = run(static, self.keep)
        finally:
            if enabled:
                gc.enable()

    def __call__(self, src):
        self.static.copy_(src)
        self.graph.replay()
        return self.output.clone()


class Predictor(object):
    """``Predictor(model, task="segm")(img)`` -> labels; ``task="depth"`` -> the depth map.

    model   a Segmenter (or any module whose output is logits or (logits, aux)) in eval mode, on the device.
            Held weakly: a Predictor does not keep a candidate alive.
    task    "segm": uint8 labels, argmax over the classes (at most 256) of the cubic-resized logits;
            "depth": fp32, channel 0 of the cubic-resized output.
    dtype   torch.float32 or torch.bfloat16: the storage of the network's activations (labels stay uint8 and depth
            stays fp32).
    graph   "auto": a shape (batch, image size, out_size, dtype) is replayed from a hipGraph from its second call on,
            when B*H*W <= engine.graphed.AUTO_GRAPH_MAX_PIXELS and NASSEG_GRAPH is not "0" ("1": every shape);
            True: from the first call; False: always launched from the host.
    scales, flip   the test-time ensemble: one view per scale (its input max(1, floor(n s + 0.5)) on a side, resized
            bilinearly) and, ``flip``, its mirror image; at most 16 views.  Labels: the argmax of the mean over the
            views of softmax(cubic-resized logits) (at most 64 classes); depth: the mean of the cubic-resized maps.
            One hipGraph holds every forward and the fusion; "auto" counts the pixels of all views.  The default
            (1.0,), False is the single forward.

    ``pred(img, out_size=None)``: img a uint8 H x W x 3 or B x H x W x 3 numpy array or tensor (host or device);
    out_size None: the image's size, "model": the network's output size, (H, W): any other.  Returns a device tensor
    (H, W) or (B, H, W).  ``pred.logits(x)``: the network's first output for a normalised B x 3 x H x W float x.
    ``pred.probabilities(img, out_size=None)`` (segmentation): the fp32 mean over the views of the class
    probabilities, (C, H, W) or (B, C, H, W).
    """

    def __init__(self, model, task="segm", dtype=torch.float32, graph="auto", max_captures=MAX_CAPTURES,
                 scales=(1.0,), flip=False):
        if task not in TASKS:
            raise ValueError("Predictor: task must be one of {} (got {!r})".format(TASKS, task))
        if dtype not in DTYPES:
            raise ValueError("Predictor: dtype must be torch.float32 or torch.bfloat16 (got {!r})".format(dtype))
        if not (graph is True or graph is False or (isinstance(graph, str) and graph == "auto")):
            raise ValueError("Predictor: graph must be 'auto', True or False (got {!r})".format(graph))
        if not isinstance(model, nn.Module):
            raise ValueError("Predictor: model must be a torch.nn.Module (got {})".format(type(model).__name__))
        self.views = ensemble_views(scales, flip)
        self.scales, self.flip = tuple(s for s, m in self.views if not m), bool(flip)
        self._model = weakref.ref(model)
        self.task, self.dtype, self.graph = task, dtype, graph
        self.max_captures = max(1, int(max_captures))
        self._captures = collections.OrderedDict()
        self._seen = collections.OrderedDict()
        self._memo = F.PackMemo()  # (host-launched calls: one re-pack launch for all chains)

    # -- public ---------------------------------------------------------------------
    def __call__(self, img, out_size=None):
        out_size = _check_out_size(out_size)
        img, squeeze = self._image(img)
        B, H, W = (int(s) for s in img.shape[:3])
        size = (H, W) if out_size is None else out_size
        if self.views == ((1.0, False),):
            out = self._run(("predict", B, H, W, size), img, B * H * W, lambda m: self._predict_fn(m, size))
        else:
            out = self._run_views("ensemble", img, size, probs=False)
        return out[0] if squeeze else out

    def probabilities(self, img, out_size=None):
        """the mean over the views of softmax(cubic-resized logits): fp32 (C, H, W) or (B, C, H, W)"""
        if self.task != "segm":
            raise ValueError("Predictor.probabilities: a {} network has no classes".format(self.task))
        out_size = _check_out_size(out_size)
        img, squeeze = self._image(img)
        out = self._run_views("probabilities", img, tuple(img.shape[1:3]) if out_size is None else out_size,
                              probs=True)
        return out[0] if squeeze else out

    def logits(self, x):
        """the network's first output (a fresh tensor) for x: a normalised B x 3 x H x W float tensor"""
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3 or not x.is_floating_point():
            raise ValueError("Predictor.logits: expected a float B x 3 x H x W tensor (got {})".format(
                tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
        B, _, H, W = (int(s) for s in x.shape)
        return self._run(("logits", B, H, W), x, B * H * W, self._logits_fn)

    @property
    def captures(self):
        """keys of the shapes held as hipGraphs, least recently used first"""
        return list(self._captures)

    # -- the computation (host-launched, or recorded once and replayed) --------------
    def _predict_fn(self, model, size):
        segm = self.task == "segm"

        def run(img, keep):
            if "plan" not in keep:
                keep["plan"] = F.prepare_plan(img.device, *img.shape[:3], dtype=self.dtype)
            x = F.prepare_image(img, self.dtype, plan=keep["plan"])
            logits = _first(model(x))
            if not torch.is_tensor(logits) or logits.dim() != 4:
                raise ValueError("Predictor: the network's output is not B x C x h x w logits")
            B, C, h, w = logits.shape
            if segm and C > 256:
                raise ValueError("Predictor: {} classes do not fit uint8 labels (at most 256)".format(C))
            H, W = (h, w) if size == "model" else size
            if "tables" not in keep:
                keep["tables"] = F.cubic_tables(logits.device, h, w, H, W)
            if segm:
                return F.resize_cubic_argmax(logits, (H, W), tables=keep["tables"])
            return F.resize_cubic(logits, (H, W), tables=keep["tables"])[:, 0]

        return run

    def _run_views(self, what, img, size, probs):
        if size == "model":
            raise ValueError("Predictor: out_size='model' needs the single view (1.0, False): the views of an "
                             "ensemble differ in size")
        B, H, W = (int(s) for s in img.shape[:3])
        size = (int(size[0]), int(size[1]))
        n_pixels = B * sum(F.view_size(H, s) * F.view_size(W, s) for s, _ in self.views)
        return self._run((what, B, H, W, size, self.scales, self.flip), img, n_pixels,
                         lambda m: self._views_fn(m, size, probs))

    def _views_fn(self, model, size, probs):
        segm = self.task == "segm"
        mirrored = [m for _, m in self.views]

        def run(img, keep):
            if "plan" not in keep:
                keep["plan"] = F.prepare_plan(img.device, *img.shape[:3], dtype=self.dtype)
            x = F.prepare_image(img, self.dtype, plan=keep["plan"])
            outs = []
            for xv in view_inputs(x, self.views):
                z = _first(model(xv))
                if not torch.is_tensor(z) or z.dim() != 4:
                    raise ValueError("Predictor: the network's output is not B x C x h x w logits")
                outs.append(z)
            C = outs[0].shape[1]
            if C > F.MAX_FUSE_CLASSES:
                raise ValueError("Predictor: an ensemble fuses at most {} channels (got {})".format(
                    F.MAX_FUSE_CLASSES, C))
            if "fuse" not in keep:
                keep["fuse"] = F.fuse_tables(x.device, [z.shape[2:] for z in outs], mirrored, size[0], size[1])
            if not segm:
                return F.fuse_views_mean(outs, size, mirrored, tables=keep["fuse"])[:, 0]
            if probs:
                return F.fuse_views(outs, size, mirrored, return_probs=True, tables=keep["fuse"])[1]
            return F.fuse_views(outs, size, mirrored, tables=keep["fuse"])

        return run

    def _logits_fn(self, model):
        def run(x, keep):
            return _first(model(x))

        return run

    def _run(self, key, src, n_pixels, make_fn):
        model = self._live_model()
        device = self._device(model)
        key = key + (self.dtype,)
        with torch.no_grad():
            if self._replays(key, n_pixels):
                sig = self._signature(model)
                cap = self._captures.get(key)
                if cap is not None and cap.signature != sig:
                    self._captures.clear()  # (parameters or buffers moved: every capture reads stale addresses)
                    cap = None
                if cap is None:
                    cap = self._record(key, make_fn(model), self._static(key, src, device), src, sig)
                self._captures.move_to_end(key)
                return cap(src)
            with F.packed_once(self._memo):
                return make_fn(model)(self._upload(key, src, device), {})

    def _record(self, key, run, static, src, sig):
        while len(self._captures) >= self.max_captures:
            self._captures.popitem(last=False)
        cap = _Capture(run, static, src, sig)
        self._captures[key] = cap
        return cap

    def _replays(self, key, n_pixels):
        if self.graph is False:
            return False
        if self.graph == "auto":
            mode = os.environ.get("NASSEG_GRAPH", "auto")
            if mode == "0" or (mode != "1" and n_pixels > graphed.AUTO_GRAPH_MAX_PIXELS):
                return False
            calls = self._seen.pop(key, 0) + 1
            self._seen[key] = calls
            while len(self._seen) > _SEEN_KEPT:
                self._seen.popitem(last=False)
            if calls < 2 and key not in self._captures:
                return False
        return True

    # -- inputs ------------------------------------------------------------------
    @staticmethod
    def _image(img):
        """-> (B x H x W x 3 uint8 array or tensor, squeeze)"""
        if torch.is_tensor(img):
            shape, dtype = tuple(img.shape), img.dtype
            ok = dtype == torch.uint8
        else:
            img = np.asarray(img)
            shape, dtype = img.shape, img.dtype
            ok = dtype == np.uint8
        if not ok or len(shape) not in (3, 4) or shape[-1] != 3 or 0 in shape:
            raise ValueError("Predictor: expected a uint8 H x W x 3 or B x H x W x 3 image (got {} {})".format(
                dtype, shape))
        if not torch.is_tensor(img):
            img = torch.from_numpy(np.ascontiguousarray(img))
        squeeze = len(shape) == 3
        if squeeze:
            img = img[None]
        return img, squeeze

    def _upload(self, key, src, device):
        if key[0] == "logits":
            return src.to(device=device, dtype=self.dtype).contiguous(memory_format=torch.channels_last)
        return src.to(device).contiguous()

    def _static(self, key, src, device):
        if key[0] == "logits":
            return torch.empty(tuple(src.shape), device=device, dtype=self.dtype, memory_format=torch.channels_last)
        return torch.empty(tuple(src.shape), device=device, dtype=torch.uint8)

    # -- the model -----------------------------------------------------------------
    def _live_model(self):
        model = self._model()
        if model is None:
            self._captures.clear()
            raise ReferenceError("Predictor: its model no longer exists (a Predictor holds its model weakly)")
        if model.training:
            self._captures.clear()
            raise ValueError("Predictor: the model is in training mode - call model.eval() first (a prediction "
                             "must not update BatchNorm statistics)")
        return model

    @staticmethod
    def _device(model):
        for t in model.parameters():
            if not t.is_cuda:
                raise F.NassegError("Predictor: the model is on {}, not on a HIP device".format(t.device))
            return t.device
        raise ValueError("Predictor: the model has no parameters")

    @staticmethod
    def _signature(model):
        """what a replay reads by address: every parameter and buffer (address, shape, dtype)"""
        return tuple((t.data_ptr(), tuple(t.shape), t.dtype)
                     for ts in (model.parameters(), model.buffers()) for t in ts)
