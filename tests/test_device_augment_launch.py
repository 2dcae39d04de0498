"""The launches of functional.augment / augment_depth / augment_colour / augment_depth_colour, no GPU: every kernel
launch replaced by a recorder (tensors stay host memory), each function makes ONE launch of its own entry point and
every argument sits where include/nasseg.h declares it."""
import numpy as np
import pytest
import torch

import nas_segm_amd  # noqa: F401
from nas_segm_amd import functional as F
from nas_segm_amd._lib import HEADER_PATH
from nas_segm_amd.data import datasets as D
from nas_segm_amd.data import device as dev
from nas_segm_amd.ffi_gen import prototypes

MEAN = np.array([0.485, 0.456, 0.406]).reshape((1, 1, 3))
STD = np.array([0.229, 0.224, 0.225]).reshape((1, 1, 3))
JITTER = dict(brightness=0.25, contrast=0.4, gamma=0.3, saturation=0.8, hue=0.15, p=0.5)
HO, WO, DEPTH_SCALE, STREAM = 24, 24, 1e-3, 1234


@pytest.fixture(scope="module")
def batches():
    """one 3-sample label batch and one 3-sample depth batch, 24 x 24 output, of a pipeline with a ColourJitter"""
    pipe = D.Compose([D.DepthResizeScale(10, 1.0, 1.0), D.RandomCrop(24), D.ColourJitter(**JITTER),
                      D.Normalise(1.0 / 255, MEAN, STD), D.ToTensor()])
    rng = np.random.RandomState(0)
    images = [(rng.rand(h, w, 3) * 255).astype(np.uint8) for h, w in ((37, 53), (41, 29), (37, 53))]
    np.random.seed(0)
    label = dev.collate([dev.plan_sample(pipe, img, (rng.rand(*img.shape[:2]) * 21).astype(np.uint8))
                         for img in images])
    depth = dev.collate_depth([dev.plan_depth_sample(pipe, img, rng.randint(0, 9000, img.shape[:2]).astype(np.uint16))
                               for img in images])
    assert tuple(label["size"]) == tuple(depth["size"]) == (HO, WO)
    return {"label": label, "depth": depth}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["augment", "augment_depth", "augment_colour", "augment_depth_colour"])
def test_one_launch_with_the_arguments_of_the_header(monkeypatch, batches, name, dtype):
    calls = []
    monkeypatch.setattr(F.lib, "call", lambda entry, *a: (calls.append((entry, a)), 0)[1])
    monkeypatch.setattr(F, "require_device", lambda *a: None)
    monkeypatch.setattr(F, "current_stream", lambda: STREAM)

    batch = dict(batches["depth" if "depth" in name else "label"])
    batch["lut"] = batch["lut"].to(dtype)
    colour = (batch["colour"], batch["ctab"]) if "colour" in name else ()
    depth = (batch["params"], DEPTH_SCALE) if "depth" in name else ()
    image, target = getattr(F, name)(batch["src"], batch["desc"], batch["taps"], *colour, batch["lut"], *depth, HO, WO)

    assert image.dtype == dtype and tuple(image.shape) == (3, 3, HO, WO)
    assert image.is_contiguous(memory_format=torch.channels_last)
    assert target.dtype == (torch.float32 if depth else torch.uint8) and tuple(target.shape) == (3, HO, WO)

    assert len(calls) == 1
    entry, args = calls[0]
    assert entry == ("nasseg_" if dtype == torch.float32 else "nasseg_bf16_") + name
    proto = {p.name: p for p in prototypes(HEADER_PATH)}[entry]
    assert len(args) == len(proto.args)
    got = {a.name: v for a, v in zip(proto.args, args)}
    tensors = dict(batch, image=image, mask=target, target=target)
    scalars = {"src_bytes": batch["src"].numel(), "depth_scale": DEPTH_SCALE, "B": 3, "Ho": HO, "Wo": WO,
               "stream": STREAM}
    pointers = [a.name for a in proto.args if a.levels and a.name != "stream"]
    assert set(pointers) == ({"src", "desc", "taps", "lut", "image"} | ({"colour", "ctab"} if colour else set())
                             | ({"params", "target"} if depth else {"mask"}))
    for arg in pointers:
        assert got[arg] == tensors[arg].data_ptr(), arg
    for arg in set(got) - set(pointers):
        assert got[arg] == scalars[arg] and type(got[arg]) is type(scalars[arg]), arg
    assert len({got[a] for a in pointers}) == len(pointers)  # (no two arguments share a tensor)
