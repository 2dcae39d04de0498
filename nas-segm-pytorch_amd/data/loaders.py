"""``create_loaders(args)`` of the search (src/data/loaders.py:21-108) without torchvision: the two sample
pipelines as data (operation, arguments taken from ``args``), the list-file datasets, the meta-train / meta-val
split of search mode, torch DataLoaders."""
import logging

from torch.utils.data import DataLoader, random_split

from . import datasets as D

log = logging.getLogger(__name__)

# (operation, argument getters).  The POSITIONS matter: PascalCustomDataset.set_config rewrites operation 0
# (ResizeScale) and operation 2 (RandomCrop) of the training pipeline.
_TRAIN_OPS = (
    (D.ResizeScale, lambda a: (a.resize_side[0], a.low_scale, a.high_scale, a.resize_longer_side)),
    (D.RandomMirror, lambda a: ()),
    (D.RandomCrop, lambda a: (a.crop_size[0],)),
    (D.Normalise, lambda a: tuple(a.normalise_params)),
    (D.ToTensor, lambda a: ()),
)
_VAL_OPS = (
    (D.ResizeScale, lambda a: (a.val_resize_side, 1, 1, a.resize_longer_side)),
    (D.CentralCrop, lambda a: (a.val_crop_size,)),
    (D.Normalise, lambda a: tuple(a.normalise_params)),
    (D.ToTensor, lambda a: ()),
)


def _pipeline(table, args):
    return D.Compose([op(*getter(args)) for op, getter in table])


def _train_pipeline(args):
    """the training pipeline; with ``args.colour_jitter`` (a dict of ColourJitter's keywords; optional) that
    operation at position 3 - after RandomCrop, before Normalise: positions 0 and 2 stay what set_config rewrites"""
    pipeline = _pipeline(_TRAIN_OPS, args)
    jitter = getattr(args, "colour_jitter", None)
    if jitter is not None:
        pipeline.transforms.insert(3, D.ColourJitter(**jitter))
    return pipeline


def _loader(dataset, batch_size, shuffle, args, collate_fn=None):
    return DataLoader(dataset, batch_size=batch_size, shuffle=shuffle, num_workers=args.num_workers,
                      pin_memory=True, drop_last=True, collate_fn=collate_fn)


def _split_loaders(args, dataset, train_pipeline, loader, word):
    """The body of every create_*loaders, here and in device.py -> (train_loader, val_loader, do_search).
    ``dataset(list file, directory, training pipeline or None, validation pipeline)`` makes a dataset,
    ``train_pipeline(args)`` the training pipeline, ``loader(dataset, batch_size, shuffle, args)`` a loader; ``word``
    starts the log line."""
    val_ops = _pipeline(_VAL_OPS, args)
    full = dataset(args.train_list, args.train_dir, train_pipeline(args), val_ops)
    do_search = args.train_list == args.val_list
    if do_search:
        n_train = int(len(full) * args.meta_train_prct / 100.0)
        train_part, val_part = random_split(full, [n_train, len(full) - n_train])
    else:
        train_part = full
        val_part = dataset(args.val_list, args.val_dir, None, val_ops)
    log.info(word + ": %d training / %d validation samples (%s)", len(train_part), len(val_part),
             "search split" if do_search else "separate lists")
    return (loader(train_part, args.batch_size[0], True, args), loader(val_part, args.val_batch_size, False, args),
            do_search)


def create_loaders(args):
    """-> (train_loader, val_loader, do_search).  ``args``: train_dir, val_dir, train_list, val_list,
    meta_train_prct, resize_side[0], low_scale, high_scale, resize_longer_side, crop_size[0], val_resize_side,
    val_crop_size, normalise_params = (scale, mean, std), batch_size[0], val_batch_size, num_workers; optionally
    colour_jitter (ColourJitter's keywords as a dict: that operation in the training pipeline, never in validation).
    Search mode (``do_search``) is train_list == val_list: ``meta_train_prct`` percent of that one list train the
    candidates and the rest scores them (one ``random_split`` draw from torch's global generator); both halves
    share the dataset object, whose stage the engine switches.  Otherwise the validation list is its own dataset.
    Both loaders drop the last incomplete batch; only the training loader shuffles."""
    return _split_loaders(args, D.PascalCustomDataset, _train_pipeline, _loader, "data")


def _depth_train_pipeline(args, zoom_depth):
    """the training pipeline with a DepthResizeScale at position 0 (``zoom_depth``), else as it is"""
    pipeline = _train_pipeline(args)
    if zoom_depth:
        op = pipeline.transforms[0]
        pipeline.transforms[0] = D.DepthResizeScale(op.resize_side, op.low_scale, op.high_scale, op.longer)
    return pipeline


def create_depth_loaders(args, depth_scale=1e-3, zoom_depth=True):
    """``create_loaders`` for depth: the list files name ``image<TAB>depth`` pairs, depth files hold 16-bit counts
    (metres = count * ``depth_scale``, 0 = hole) -> (train_loader, val_loader, do_search) whose batches are
    {"image": float B x 3 x H x W, "mask": float32 B x H x W metres} - what ``train_segmenter`` with an
    nn.BerHuLoss and ``validate_depth`` take.  The same ``args`` fields, search-mode split (one ``random_split``
    draw), shuffling and drop_last.  ``zoom_depth``: the training pipeline's random zoom divides the target by its
    factor (DepthResizeScale); the validation pipeline never does - its scores are in true metres."""
    return _split_loaders(args, lambda *files_and_pipelines: D.DepthDataset(*files_and_pipelines, depth_scale),
                          lambda a: _depth_train_pipeline(a, zoom_depth), _loader, "depth data")
