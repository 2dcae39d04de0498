"""The sample pipelines of datasets.py on the GPU: same batches, bit for bit after the engine's dtype cast.

The DataLoader workers still decode the files (PIL) and still draw every ``np.random`` number in the order the host
operations draw them, but instead of resampling the whole image they only *plan*: each operation maps a per-axis
list of coordinates of the resized image (crops slice it, a mirror reverses it, a pad adds -1 entries for its
fill), and the plan ends as tables - four source indices and OpenCV's four 11-bit coefficients per output row and
column, built by ``datasets._cubic_taps``, and the nearest source index of the mask.  A worker ships only the
source rows and columns those tables reach; ``DeviceLoader`` uploads a packed batch and one launch of
``functional.augment`` (csrc/augment.hip) computes OpenCV's fixed-point bicubic in integers - exact in any
order - and maps each uint8 result through a table of ``Normalise`` evaluated on the host in float64 and cast to
the requested dtype there.  The host path (datasets.py, loaders.py) is untouched; ``create_device_loaders`` is its
opt-in twin.

Pipelines the kernel cannot reproduce are refused (ValueError) when the dataset is built: more than one resize,
a resize after a window operation (crop, mirror, pad), more than one pad, ``Normalise`` and ``ToTensor`` not the
last two operations, more than one ``ColourJitter``, one before a resize or after ``Normalise``, an operation this
module does not know.  Samples it cannot reproduce are refused when they
arrive: images that are not 3-channel uint8 (the float branch of resize_cubic; RGBA), masks that are not 2-D uint8
of the image's size.

Depth (``create_device_depth_loaders``, the twin of ``loaders.create_depth_loaders``): the target is a map of 16-bit
counts, shipped as little-endian bytes; ``functional.augment_depth`` gathers it with the mask's nearest indices and
writes fp32 metres - count * depth_scale, divided by the fp32 zoom factor where the resize is a DepthResizeScale -
with the two correctly rounded fp32 operations the host pipeline makes, so the targets are the host's bit for bit
too.  ``plan_sample`` keeps refusing every mask that is not uint8; depth samples go through ``plan_depth_sample``.

Colour (``datasets.ColourJitter``): its planner makes the operation's draws through the operation's own ``draw()`` and
the sample carries the integer colour matrix and the byte table (``colour_tables``); ``functional.augment_colour`` /
``augment_depth_colour`` apply them to every live pixel between the resampling and the Normalise table, in integers, so
these batches are the host's bit for bit too.  Batches of pipelines without the operation are packed and launched as
before.
"""
import collections
import os

import numpy as np
import torch

from . import datasets as D
from . import loaders as L

_IDENTITY_COEF = np.array([0, D._COEF_SCALE, 0, 0], np.int64)  # (2048 * 2048 * v + 2^21) >> 22 == v
# a sample's descriptor, int64 [DESC_FIELDS]: offsets, window height / width, row strides (bytes), fills, in the order
# of the enum in csrc/augment.hip, which defines it
Desc = collections.namedtuple("Desc", "img_off msk_off h w img_ld msk_ld img_fill msk_fill")
DESC_FIELDS = len(Desc._fields)


# ---------------------------------------------------------------------------
# the plan of one sample
# ---------------------------------------------------------------------------
class _Plan(object):
    """Coordinates along each axis of the image the host pipeline holds at this point: entries of the resized
    image (of the source while no resize ran), -1 for a pad's fill."""

    def __init__(self, height, width):
        self.src_shape = (height, width)
        self.scale = None  # resize factor, once a resize ran
        self.rows = np.arange(height, dtype=np.int64)
        self.cols = np.arange(width, dtype=np.int64)
        self.img_fill = np.zeros(3, np.uint8)
        self.msk_fill = 0
        self.zoom = np.float32(1.0)  # what a depth target is divided by (a DepthResizeScale's factor, in fp32)
        self.depth_fill = np.float32(0.0)  # a pad's fill of a depth target
        self.lut = None
        self.colour = None  # (Mq, Tab) of a ColourJitter's draw, once one ran

    @property
    def shape(self):
        return len(self.rows), len(self.cols)

    def resize(self, scale):
        H, W = self.src_shape
        self.scale = scale
        self.rows = np.arange(D._out_size(H, scale), dtype=np.int64)
        self.cols = np.arange(D._out_size(W, scale), dtype=np.int64)

    def window(self, top, left, height, width):
        # D._window's slices, on the coordinates: a negative top counts from the end there and here
        self.rows = self.rows[top: top + height]
        self.cols = self.cols[left: left + width]


def _plan_resize_scale(op, plan):
    scale = np.random.uniform(op.low_scale, op.high_scale)
    side = (max if op.longer else min)(plan.shape)
    beyond = side * scale > op.resize_side if op.longer else side * scale < op.resize_side
    if beyond:
        scale = op.resize_side * 1.0 / side
    plan.resize(scale)


def _plan_depth_resize_scale(op, plan):
    _plan_resize_scale(op, plan)
    plan.zoom = np.float32(plan.scale)  # D.DepthResizeScale's divisor: the limited factor


def _plan_resize_shorter(op, plan):
    shortest = min(plan.shape)
    if shortest < op.shorter_side:
        plan.resize(op.shorter_side * 1.0 / shortest)


def _plan_mirror(op, plan):
    if np.random.randint(2):
        plan.cols = plan.cols[::-1]


def _plan_random_crop(op, plan):
    n_rows, n_cols = plan.shape
    height, width = (min(n, op.crop_size) for n in (n_rows, n_cols))
    top = np.random.randint(0, n_rows - height + 1)
    left = np.random.randint(0, n_cols - width + 1)
    plan.window(top, left, height, width)


def _plan_central_crop(op, plan):
    side = op.crop_size
    plan.window((plan.shape[0] - side) // 2, (plan.shape[1] - side) // 2, side, side)


def _plan_pad(op, plan):
    rows, cols = (max(0, (op.size - n + 1) // 2) for n in plan.shape)
    fill = -np.ones(rows, np.int64), -np.ones(cols, np.int64)
    plan.rows = np.concatenate([fill[0], plan.rows, fill[0]])
    plan.cols = np.concatenate([fill[1], plan.cols, fill[1]])
    # cast as D._framed casts: the image's fill per channel to uint8, the mask's to the mask's dtype (uint8)
    plan.img_fill = np.broadcast_to(np.asarray(op.img_val[:3]).astype(np.uint8), (3,)).copy()
    plan.msk_fill = int(np.asarray(op.msk_val).astype(np.uint8))
    plan.depth_fill = np.float32(op.msk_val)  # (a float32 target: D._framed casts to float32)


def normalise_table(op):
    """float64 [3][256]: what ``op.apply`` makes of the uint8 value v in channel c (the same expression on a
    ramp; Normalise is elementwise, so each entry is the one a pixel of value v gets)"""
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)
    out, _ = op.apply(ramp, None)
    out = np.asarray(out)
    if out.shape != (256, 1, 3):
        raise ValueError("Normalise parameters must broadcast per channel (got a result of shape {})".format(
            out.shape))
    return np.ascontiguousarray(out[:, 0, :].T)


# the reference's prepare_img (src/utils/helpers.py): what its inference path feeds a network
IMG_SCALE = 1.0 / 255
IMG_MEAN = np.array([0.485, 0.456, 0.406]).reshape((1, 1, 3))
IMG_STD = np.array([0.229, 0.224, 0.225]).reshape((1, 1, 3))


def prepare_img_table():
    """float64 [3][256]: prepare_img of the uint8 value v in channel c (functional.prepare_image's table)"""
    return normalise_table(D.Normalise(IMG_SCALE, IMG_MEAN, IMG_STD))


def _plan_normalise(op, plan):
    plan.lut = normalise_table(op)


def _plan_to_tensor(op, plan):
    pass


def _plan_colour(op, plan):
    """the op's own draws (``draw``: the method ``apply`` calls).  The kernel jitters live pixels only, so a fill
    that is already there - a Pad BEFORE the op: the host jitters its border too - goes through the same integer
    function here; a Pad after the op sets its fill afterwards and leaves it as it is."""
    Mq, Tab = op.draw()
    if Mq is not None and np.abs(Mq).max() > D.COLOUR_COEF_MAX:
        raise ValueError("device pipeline: colour coefficients beyond 2^15 ({})".format(Mq.tolist()))
    plan.colour = (Mq, Tab)
    plan.img_fill = D.colour_apply(plan.img_fill, Mq, Tab)


_CTAB_IDENTITY = np.repeat(np.arange(256, dtype=np.uint8)[None, :], 3, axis=0)


def colour_tables(p):
    """{"colour": int32 [12] = the 9 coefficients row-major, 1 / 0: apply the matrix, 0, 0; "ctab": uint8 [3][256],
    the identity ramp when the draw made no table} of a plan whose pipeline has a ColourJitter, else {}"""
    if p.colour is None:
        return {}
    Mq, Tab = p.colour
    words = np.zeros(12, np.int32)
    words[:9] = ((1 << 12) * np.eye(3, dtype=np.int64) if Mq is None else Mq).ravel()
    words[9] = Mq is not None
    return {"colour": words, "ctab": np.ascontiguousarray(_CTAB_IDENTITY if Tab is None else Tab, dtype=np.uint8)}


_PLANNERS = {
    D.ResizeScale: _plan_resize_scale,
    D.DepthResizeScale: _plan_depth_resize_scale,
    D.ResizeShorter: _plan_resize_shorter,
    D.RandomMirror: _plan_mirror,
    D.RandomCrop: _plan_random_crop,
    D.CentralCrop: _plan_central_crop,
    D.Pad: _plan_pad,
    D.Normalise: _plan_normalise,
    D.ToTensor: _plan_to_tensor,
    D.ColourJitter: _plan_colour,
}
_RESIZES = (D.ResizeScale, D.DepthResizeScale, D.ResizeShorter)
_WINDOWS = (D.RandomMirror, D.RandomCrop, D.CentralCrop, D.Pad)


def check_pipeline(pipeline):
    """ValueError unless the kernel reproduces ``pipeline`` (a Compose or a list of operations) exactly."""
    ops = list(getattr(pipeline, "transforms", pipeline))
    for op in ops:
        if type(op) not in _PLANNERS:
            raise ValueError("device pipeline: no device plan for {}".format(type(op).__name__))
    kinds = [type(op) for op in ops]
    jitters = [i for i, k in enumerate(kinds) if k is D.ColourJitter]
    if len(jitters) > 1:
        raise ValueError("device pipeline: at most one ColourJitter")
    if jitters and any(k in _RESIZES for k in kinds[jitters[0]:]):
        raise ValueError("device pipeline: a ColourJitter before a resize (the kernel applies colour after "
                         "resampling, and the two do not commute)")
    if jitters and D.Normalise in kinds[:jitters[0]]:
        raise ValueError("device pipeline: a ColourJitter after Normalise")
    if len(ops) < 2 or kinds[-2] is not D.Normalise or kinds[-1] is not D.ToTensor:
        raise ValueError("device pipeline: Normalise and ToTensor must be the last two operations")
    if kinds.count(D.Normalise) != 1 or kinds.count(D.ToTensor) != 1:
        raise ValueError("device pipeline: one Normalise and one ToTensor")
    resizes = [i for i, k in enumerate(kinds) if k in _RESIZES]
    if len(resizes) > 1:
        raise ValueError("device pipeline: at most one resize")
    if resizes and any(k in _WINDOWS for k in kinds[:resizes[0]]):
        raise ValueError("device pipeline: a resize after a crop, mirror or pad")
    if kinds.count(D.Pad) > 1:
        raise ValueError("device pipeline: at most one Pad")
    return ops


def _check_image(image):
    if not isinstance(image, np.ndarray) or image.dtype != np.uint8:
        raise ValueError("device pipeline: images must be uint8 (got {})".format(getattr(image, "dtype", image)))
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("device pipeline: images must be HxWx3 (got {})".format(image.shape))


def check_sample(image, mask):
    """ValueError for samples the kernel does not reproduce"""
    _check_image(image)
    if not isinstance(mask, np.ndarray) or mask.dtype != np.uint8:
        raise ValueError("device pipeline: masks must be uint8 (got {})".format(getattr(mask, "dtype", mask)))
    if mask.shape != image.shape[:2]:
        raise ValueError("device pipeline: the mask must be HxW of its image (got {} for {})".format(
            mask.shape, image.shape))


def plan(pipeline, height, width):
    """Run the planners of ``pipeline`` on a height x width source: the random draws of the host operations,
    in their order, and the attributes each operation has NOW."""
    p = _Plan(height, width)
    for op in getattr(pipeline, "transforms", pipeline):
        planner = _PLANNERS.get(type(op))
        if planner is None:
            raise ValueError("device pipeline: no device plan for {}".format(type(op).__name__))
        planner(op, p)
    return p


def _nearest(n_src, n_dst, scale):
    """D.resize_nearest's source indices along one axis"""
    inv = 1.0 / scale
    return np.minimum(np.floor(np.arange(n_dst) * inv).astype(np.int64), n_src - 1)


def tables(p):
    """-> (row window (r0, r1), column window (c0, c1), int32 taps [9 (Ho + Wo)]) of a finished plan: image taps
    [Ho][4 + 4] and [Wo][4 + 4], then mask indices [Ho] and [Wo], all rebased to the window"""
    axes = []
    for coords, n_src in ((p.rows, p.src_shape[0]), (p.cols, p.src_shape[1])):
        live = coords >= 0
        c = np.where(live, coords, 0)
        if p.scale is None:
            idx = np.repeat(c[:, None], 4, axis=1)
            coef = np.broadcast_to(_IDENTITY_COEF, (len(c), 4))
            near = c
        else:
            n_dst = D._out_size(n_src, p.scale)
            iy, wy = D._cubic_taps(n_src, n_dst, p.scale)
            idx = iy[c]
            coef = np.clip(np.rint(wy[c] * D._COEF_SCALE), -32768, 32767).astype(np.int64)
            near = _nearest(n_src, n_dst, p.scale)[c]
        reached = np.concatenate([idx[live].ravel(), near[live]])
        lo, hi = (int(reached.min()), int(reached.max()) + 1) if reached.size else (0, 1)
        idx = np.where(live[:, None], idx - lo, -1)
        near = np.where(live, near - lo, -1)
        axes.append(((lo, hi), np.concatenate([idx, coef], 1), near))
    (rwin, ty, my), (cwin, tx, mx) = axes
    taps = np.concatenate([ty.ravel(), tx.ravel(), my, mx]).astype(np.int32)
    return rwin, cwin, taps


# ---------------------------------------------------------------------------
# dataset, batches, loader
# ---------------------------------------------------------------------------
def _check_pipelines(*pipelines):
    for pipeline in pipelines:
        if pipeline is not None:
            check_pipeline(pipeline)


def _stage_pipeline(dataset):
    """the pipeline of the dataset's current stage, or ValueError"""
    pipeline = getattr(dataset, dataset._PIPELINE_OF_STAGE.get(dataset.stage, ""), None)
    if pipeline is None:
        raise ValueError("device pipeline: stage {!r} has no pipeline".format(dataset.stage))
    return pipeline


class DeviceDepthDataset(D.DepthDataset):
    """DepthDataset whose samples are plans (``plan_depth_sample``): the workers decode the image and the 16-bit
    depth file - the counts stay integers; the metres are made on the GPU - and plan the stage's pipeline."""

    def __init__(self, data_file, data_dir, transform_trn=None, transform_val=None, depth_scale=1e-3):
        _check_pipelines(transform_trn, transform_val)
        super(DeviceDepthDataset, self).__init__(data_file, data_dir, transform_trn, transform_val, depth_scale)

    def __getitem__(self, idx):
        image_file, depth_file = self._files(idx)
        pipeline = _stage_pipeline(self)
        return plan_depth_sample(pipeline, D._load_rgb(image_file), D._load_depth_counts(depth_file))


class DevicePascalDataset(D.PascalCustomDataset):
    """PascalCustomDataset whose samples are plans: ``__getitem__`` (in the DataLoader workers) decodes the files,
    plans the stage's pipeline and returns {"image": uint8 window of the source, "mask": its window, "taps",
    "fill", "lut", "size"}; ``collate`` packs a batch, ``DeviceLoader`` runs it on the GPU."""

    def __init__(self, data_file, data_dir, transform_trn=None, transform_val=None):
        _check_pipelines(transform_trn, transform_val)
        super(DevicePascalDataset, self).__init__(data_file, data_dir, transform_trn, transform_val)

    def __getitem__(self, idx):
        image_file, mask_file = (os.path.join(self.root_dir, name) for name in self.datalist[idx])
        image = D._load_rgb(image_file)
        mask = D._load_mask(mask_file, image_file != mask_file)
        return plan_sample(_stage_pipeline(self), image, mask)


def _planned(pipeline, image):
    """-> (the plan, the window of the source it reaches as (row slice, column slice), the image's packed fill, the
    image half of the device sample) of a checked image under ``pipeline``; the caller adds "mask", "fill" and what
    else its target needs"""
    p = plan(pipeline, image.shape[0], image.shape[1])
    (r0, r1), (c0, c1), taps = tables(p)
    window = (slice(r0, r1), slice(c0, c1))
    img_fill = int(p.img_fill[0]) | int(p.img_fill[1]) << 8 | int(p.img_fill[2]) << 16
    return p, window, img_fill, {"image": np.ascontiguousarray(image[window]), "taps": taps, "lut": p.lut,
                                 "size": p.shape, **colour_tables(p)}


def plan_sample(pipeline, image, mask):
    """the device sample of (image, mask) under ``pipeline``"""
    check_sample(image, mask)
    p, window, img_fill, sample = _planned(pipeline, image)
    return dict(sample, mask=np.ascontiguousarray(mask[window]), fill=(img_fill, p.msk_fill))


def plan_depth_sample(pipeline, image, counts):
    """the device sample of (image, 16-bit depth counts) under ``pipeline``: ``plan_sample``'s, with the window of
    the counts as "mask" (little-endian uint16) and "params" = fp32 (zoom, fill): what the target is divided by (a
    DepthResizeScale's factor, else 1) and what a Pad's fill pixels become (its ``msk_val``, else 0)."""
    _check_image(image)
    if not isinstance(counts, np.ndarray) or counts.dtype != np.uint16 or counts.ndim != 2:
        raise ValueError("device pipeline: depth targets must be 2-D uint16 counts (got {} of {})".format(
            getattr(counts, "shape", None), getattr(counts, "dtype", type(counts).__name__)))
    if counts.shape != image.shape[:2]:
        raise ValueError("device pipeline: the depth target must be HxW of its image (got {} for {})".format(
            counts.shape, image.shape))
    p, window, img_fill, sample = _planned(pipeline, image)
    return dict(sample, mask=np.ascontiguousarray(counts[window], dtype="<u2"), fill=(img_fill, 0),
                params=np.array([p.zoom, p.depth_fill], np.float32))


def collate(samples):
    """a list of device samples -> {"src": uint8 [bytes], "desc": int64 [B][8], "taps": int32 [B][9 (Ho + Wo)],
    "lut": float64 [3][256], "size": int64 [2]} (tensors the DataLoader can pin); samples of a pipeline with a
    ColourJitter add "colour": int32 [B][12] and "ctab": uint8 [B][3][256]"""
    size = tuple(samples[0]["size"])
    if any(tuple(s["size"]) != size for s in samples):
        raise RuntimeError("device pipeline: samples of one batch differ in size: {}".format(
            [tuple(s["size"]) for s in samples]))
    if size[0] == 0 or size[1] == 0:
        raise RuntimeError("device pipeline: empty samples ({})".format(size))
    lut = samples[0]["lut"]
    if any(not np.array_equal(s["lut"], lut) for s in samples):
        raise RuntimeError("device pipeline: samples of one batch were normalised differently")
    desc = np.zeros((len(samples), DESC_FIELDS), np.int64)
    chunks, off = [], 0
    for i, s in enumerate(samples):
        img, msk = s["image"], s["mask"]
        h, w = msk.shape
        # (row strides in bytes: uint8 label maps, or the little-endian uint16 counts of a depth sample)
        desc[i] = Desc(img_off=off, msk_off=off + img.nbytes, h=h, w=w, img_ld=3 * w, msk_ld=msk.itemsize * w,
                       img_fill=s["fill"][0], msk_fill=s["fill"][1])
        chunks += [img.reshape(-1), msk.reshape(-1).view(np.uint8)]
        off += img.nbytes + msk.nbytes
    batch = {"src": torch.from_numpy(np.concatenate(chunks)), "desc": torch.from_numpy(desc),
             "taps": torch.from_numpy(np.stack([s["taps"] for s in samples])), "lut": torch.from_numpy(lut),
             "size": torch.tensor(size, dtype=torch.int64)}
    jittered = ["colour" in s for s in samples]
    if any(jittered):
        if not all(jittered):
            raise RuntimeError("device pipeline: samples with and without a ColourJitter in one batch")
        batch["colour"] = torch.from_numpy(np.stack([s["colour"] for s in samples]).astype(np.int32))
        batch["ctab"] = torch.from_numpy(np.stack([s["ctab"] for s in samples]).astype(np.uint8))
    return batch


def collate_depth(samples):
    """a list of depth samples -> ``collate``'s batch, the count windows packed as bytes wherever they fall (no
    padding: the kernel reads a count as two bytes), plus "params": float32 [B][2]"""
    batch = collate(samples)
    batch["params"] = torch.from_numpy(np.stack([s["params"] for s in samples]).astype(np.float32))
    return batch


def run_batch(batch, device, dtype):
    """one packed batch -> {"image": B x 3 x Ho x Wo channels_last ``dtype``, "mask": B x Ho x Wo uint8} on
    ``device`` (uploads on the current stream, one augment launch: augment_colour for the batches of a pipeline with
    a ColourJitter)"""
    from .. import functional as F

    Ho, Wo, up = _uploaded(batch, device, dtype, ("src", "desc", "taps", "colour", "ctab"))
    if "colour" in up:
        image, mask = F.augment_colour(up["src"], up["desc"], up["taps"], up["colour"], up["ctab"], up["lut"], Ho, Wo)
    else:
        image, mask = F.augment(up["src"], up["desc"], up["taps"], up["lut"], Ho, Wo)
    return {"image": image, "mask": mask}


def run_depth_batch(batch, device, dtype, depth_scale):
    """one packed depth batch -> {"image": B x 3 x Ho x Wo channels_last ``dtype``, "mask": B x Ho x Wo float32
    metres} on ``device`` (uploads on the current stream, one augment_depth launch: augment_depth_colour for the
    batches of a pipeline with a ColourJitter)"""
    from .. import functional as F

    Ho, Wo, up = _uploaded(batch, device, dtype, ("src", "desc", "taps", "params", "colour", "ctab"))
    if "colour" in up:
        image, target = F.augment_depth_colour(up["src"], up["desc"], up["taps"], up["colour"], up["ctab"],
                                               up["lut"], up["params"], depth_scale, Ho, Wo)
    else:
        image, target = F.augment_depth(up["src"], up["desc"], up["taps"], up["lut"], up["params"], depth_scale,
                                        Ho, Wo)
    return {"image": image, "mask": target}


def _uploaded(batch, device, dtype, keys):
    """-> (Ho, Wo, those of ``keys`` the packed batch has, on ``device``, and its "lut" as ``dtype`` there): the
    uploads of the two functions above, on the current stream"""
    Ho, Wo = (int(v) for v in batch["size"])
    lut = batch["lut"].to(dtype)  # (on the host: the cast of torch.from_numpy(host image).to(dtype))
    up = {k: batch[k].to(device, non_blocking=True) for k in keys if k in batch}
    up["lut"] = lut.to(device, non_blocking=True)
    return Ho, Wo, up


class DeviceLoader(object):
    """A DataLoader of device samples whose batches come out augmented on the GPU.  ``dataset``,
    ``batch_sampler``, ``__len__`` and every other attribute are the wrapped DataLoader's."""

    def __init__(self, loader, device=None, dtype=torch.float32):
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("device pipeline: images are float32 or bfloat16 (got {})".format(dtype))
        self.loader = loader
        self.device = torch.device(device) if device is not None else None
        self.dtype = dtype

    def __len__(self):
        return len(self.loader)

    def __getattr__(self, name):
        if name == "loader":  # (not set yet: unpickling)
            raise AttributeError(name)
        return getattr(self.loader, name)

    def __iter__(self):
        device = self.device or torch.device("cuda", torch.cuda.current_device())
        for batch in self.loader:
            yield self.run(batch, device)

    def run(self, batch, device):
        return run_batch(batch, device, self.dtype)


class DeviceDepthLoader(DeviceLoader):
    """DeviceLoader for the packed batches of a DeviceDepthDataset"""

    def __init__(self, loader, device=None, dtype=torch.float32, depth_scale=1e-3):
        super(DeviceDepthLoader, self).__init__(loader, device, dtype)
        self.depth_scale = depth_scale

    def run(self, batch, device):
        return run_depth_batch(batch, device, self.dtype, self.depth_scale)


def create_device_loaders(args, device=None, dtype=torch.float32):
    """create_loaders(args) (loaders.py) with the augmentation on the GPU: the same ``args`` fields, search-mode
    split, shuffling and drop_last, the same batches (``image`` as ``dtype`` on ``device``, channels_last)
    -> (train_loader, val_loader, do_search)."""
    def loader(part, batch_size, shuffle, args):
        return DeviceLoader(L._loader(part, batch_size, shuffle, args, collate), device, dtype)

    return L._split_loaders(args, DevicePascalDataset, L._train_pipeline, loader, "data (device augmentation)")


def create_device_depth_loaders(args, device=None, dtype=torch.float32, depth_scale=1e-3, zoom_depth=True):
    """create_depth_loaders(args, depth_scale, zoom_depth) (loaders.py) with the augmentation on the GPU: the same
    ``args`` fields, search-mode split, shuffling and drop_last, the same batches (``image`` as ``dtype`` on
    ``device``, channels_last; ``mask`` float32 metres on ``device``) -> (train_loader, val_loader, do_search)."""
    def loader(part, batch_size, shuffle, args):
        return DeviceDepthLoader(L._loader(part, batch_size, shuffle, args, collate_depth), device, dtype, depth_scale)

    return L._split_loaders(args, lambda *files_and_pipelines: DeviceDepthDataset(*files_and_pipelines, depth_scale),
                            lambda a: L._depth_train_pipeline(a, zoom_depth), loader,
                            "depth data (device augmentation)")


def create_loaders(args):
    """the reference's entry point (src/data/loaders.py) on the device path: install_dropin(data_on_device=True)
    resolves ``from data.loaders import create_loaders`` here"""
    return create_device_loaders(args)
