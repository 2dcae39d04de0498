"""Prediction on the device (csrc/predict.hip, F.prepare_image, engine/predict.Predictor) against the reference's
inference pipeline restated on the host: prepare_img in float64, the eval forward, cv2's float INTER_CUBIC resize to
the image's size (data/datasets.resize_cubic_to) and numpy's argmax - bit for bit - and replayed from a hipGraph
against host-launched, bit for bit."""
import numpy as np
import pytest
import torch

from _util import build_product_net, load_json

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16

IMG_SCALE = 1.0 / 255
IMG_MEAN = np.array([0.485, 0.456, 0.406]).reshape((1, 1, 3))
IMG_STD = np.array([0.229, 0.224, 0.225]).reshape((1, 1, 3))


def prepare_img(img):  # the reference's src/utils/helpers.py
    return (img * IMG_SCALE - IMG_MEAN) / IMG_STD


def F():
    from nas_segm_amd import functional

    return functional


def D():
    from nas_segm_amd.data import datasets

    return datasets


def Predictor(*a, **k):
    from nas_segm_amd.engine.inference import Predictor as P

    return P(*a, **k)


def host_resize(x, size):
    """x: B x C x h x w tensor -> fp32 numpy B x H x W x C through resize_cubic_to (bf16 widened first)"""
    a = x.detach().float().cpu().permute(0, 2, 3, 1).numpy()
    return np.stack([D().resize_cubic_to(s, size) for s in a])


def logits_of(B, C, h, w, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, h, w, generator=g) * scale
    return x.to(dtype).to(DEV).contiguous(memory_format=torch.channels_last)


CASES = [  # B, C, h, w, H, W
    (1, 19, 64, 128, 256, 512),   # 4x up
    (2, 21, 81, 81, 321, 321),    # the notebooks' VOC size
    (1, 11, 97, 129, 40, 50),     # down
    (2, 1, 33, 47, 101, 75),      # odd sizes, depth
    (1, 256, 9, 11, 37, 29),      # the most classes uint8 labels hold
    (2, 19, 31, 45, 31, 45),      # identity
    (1, 1, 17, 23, 17, 23),       # identity, depth
]


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("scale", [1.0, 1e20], ids=["randn", "large"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_resize_cubic_and_argmax_are_the_host_restatement(case, scale, dtype):
    B, C, h, w, H, W = case
    x = logits_of(B, C, h, w, seed=sum(case), scale=scale, dtype=dtype)
    want = host_resize(x, (H, W))  # B x H x W x C
    y = F().resize_cubic(x, (H, W))
    assert y.dtype == torch.float32 and tuple(y.shape) == (B, C, H, W)
    assert y.is_contiguous(memory_format=torch.channels_last)
    got = y.permute(0, 2, 3, 1).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    labels = F().resize_cubic_argmax(x, (H, W))
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (B, H, W)
    assert np.array_equal(labels.cpu().numpy(), np.argmax(want, axis=3).astype(np.uint8))
    if (h, w) == (H, W):
        assert np.array_equal(got, x.float().permute(0, 2, 3, 1).cpu().numpy())


def test_argmax_ties_take_the_lowest_index_and_257_classes_are_refused():
    x = torch.zeros(2, 9, 13, 17)
    x[1, 3] = 2.0
    x[1, 7] = 2.0
    x = x.to(DEV).contiguous(memory_format=torch.channels_last)
    labels = F().resize_cubic_argmax(x, (29, 31)).cpu()
    assert bool((labels[0] == 0).all()) and bool((labels[1] == 3).all())
    with pytest.raises(F().NassegError):
        F().resize_cubic_argmax(logits_of(1, 257, 5, 5, seed=0), (9, 9))
    assert tuple(F().resize_cubic(logits_of(1, 257, 5, 5, seed=0), (9, 9)).shape) == (1, 257, 9, 9)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_prepare_image_is_prepare_img(dtype):
    img = np.random.RandomState(4).randint(0, 256, (2, 37, 53, 3)).astype(np.uint8)
    got = F().prepare_image(torch.from_numpy(img).to(DEV), dtype)
    assert got.dtype == dtype and tuple(got.shape) == (2, 3, 37, 53)
    assert got.is_contiguous(memory_format=torch.channels_last)
    want = torch.tensor(prepare_img(img).transpose(0, 3, 1, 2)).float().to(dtype)
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(got.cpu().contiguous().view(bits), want.contiguous().view(bits))


def net_of(name, seed=0):
    rec = load_json("nets_meta.json")[name]
    return build_product_net(rec["kind"], rec["genotype"], rec["classes"], rec["dec_kwargs"], seed).to(DEV).eval()


def image(seed, h=161, w=241):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def notebook(net, img, dtype=torch.float32):
    """the reference notebooks' pipeline, host post-processing: logits copied out, cv2 resize restated, argmax"""
    x = torch.tensor(prepare_img(img).transpose(2, 0, 1)[None]).float()
    with torch.no_grad():
        out = net(x.to(DEV).to(dtype).contiguous(memory_format=torch.channels_last))
    out = out[0] if isinstance(out, tuple) else out
    return host_resize(out, img.shape[:2])[0]  # H x W x C


@pytest.mark.parametrize("name", ["wacv_arch0", "cvpr_arch0", "cvpr_arch2_depth"])
def test_predictor_is_the_notebook_pipeline_and_replays_bit_identically(name):
    net = net_of(name)
    task = "depth" if name.endswith("depth") else "segm"
    img = image(1)
    eager, replay = Predictor(net, task=task, graph=False), Predictor(net, task=task, graph=True)
    a, b = eager(img), replay(img)
    assert a.is_cuda and tuple(a.shape) == img.shape[:2]
    want = notebook(net, img)
    if task == "segm":
        assert a.dtype == torch.uint8
        assert np.array_equal(a.cpu().numpy(), np.argmax(want, axis=2).astype(np.uint8))
    else:
        assert a.dtype == torch.float32
        assert np.array_equal(a.cpu().numpy().view(np.uint32), want[:, :, 0].view(np.uint32))
    assert torch.equal(a, b) and len(replay.captures) == 1
    assert torch.equal(replay(img), a)  # (the replay, not the capture's first run)
    # at the model's resolution: tests/test_inference.py's post-processing
    x = torch.tensor(prepare_img(img).transpose(2, 0, 1)[None]).float().to(DEV)
    la, lb = eager.logits(x), replay.logits(x)
    assert torch.equal(la, lb) and torch.equal(replay.logits(x), la)
    with torch.no_grad():
        ref = net(x.contiguous(memory_format=torch.channels_last))
    ref = ref[0] if isinstance(ref, tuple) else ref
    assert torch.equal(la, ref)
    m_a, m_b = eager(img, out_size="model"), replay(img, out_size="model")
    assert torch.equal(m_a, m_b) and tuple(m_a.shape) == tuple(la.shape[2:])
    if task == "segm":
        assert np.array_equal(m_a.cpu().numpy(), la[0].cpu().numpy().argmax(axis=0).astype(np.uint8))
    else:
        assert torch.equal(m_a, la[0, 0])


def test_a_replay_follows_its_inputs_and_parameters():
    """(on the depth network: its fp32 map moves with every input and weight - the labels of a randomly initialised
    segmentation network can be one class everywhere)"""
    net = net_of("cvpr_arch2_depth")
    eager, replay = Predictor(net, task="depth", graph=False), Predictor(net, task="depth", graph=True)
    i1, i2 = image(1), image(2)
    assert torch.equal(replay(i1), eager(i1))
    assert torch.equal(replay(i2), eager(i2)) and not torch.equal(eager(i1), eager(i2))
    # batch of two from the device
    both = torch.from_numpy(np.stack([i1, i2])).to(DEV)
    assert torch.equal(replay(both), eager(both))
    assert len(replay.captures) == 2
    # in-place new weights: the same captures read them
    before = eager(i1)
    net.load_state_dict(net_of("cvpr_arch2_depth", seed=1).state_dict())
    after = eager(i1)
    assert not torch.equal(before, after)
    assert torch.equal(replay(i1), after) and len(replay.captures) == 2
    # another shape: a new capture; the old one still right
    i3 = image(3, 97, 129)
    assert torch.equal(replay(i3), eager(i3)) and len(replay.captures) == 3
    assert torch.equal(replay(i1), after)
    # replaced parameter tensors: never replayed against the old addresses
    with torch.no_grad():
        for p in net.parameters():
            p.data = p.data * 0.75
    fresh = eager(i1)
    assert not torch.equal(fresh, after)
    assert torch.equal(replay(i1), fresh)
    # training mode is refused, and eval mode records again
    net.train()
    with pytest.raises(ValueError):
        replay(i1)
    with pytest.raises(ValueError):
        eager(i1)
    net.eval()
    assert torch.equal(replay(i1), fresh)


def test_auto_replays_from_the_second_call_and_keeps_a_bounded_number_of_captures():
    net = net_of("wacv_arch0")
    pred = Predictor(net)
    eager = Predictor(net, graph=False)
    img = image(5, 65, 97)
    first = pred(img)
    assert pred.captures == []
    assert torch.equal(pred(img), first) and len(pred.captures) == 1
    graphed = Predictor(net, graph=True, max_captures=3)
    for h in (33, 41, 49, 57, 65):
        im = image(h, h, 97)
        assert torch.equal(graphed(im), eager(im))
        assert len(graphed.captures) <= 3
    assert len(graphed.captures) == 3


@pytest.mark.parametrize("name", ["wacv_arch0", "cvpr_arch2_depth"])
def test_bf16_predictions_track_fp32(name):
    """bf16 activations: replayed equals host-launched bit for bit; labels agree with fp32 wherever fp32's top-2
    margin exceeds twice the largest difference of the two resized logit maps (an argmax cannot flip there)"""
    net = net_of(name)
    task = "depth" if name.endswith("depth") else "segm"
    img = image(7)
    p16 = Predictor(net, task=task, dtype=BF, graph=False)
    a = p16(img)
    assert torch.equal(Predictor(net, task=task, dtype=BF, graph=True)(img), a)
    f32, b16 = notebook(net, img), notebook(net, img, BF)
    d = float(np.abs(f32 - b16).max())
    assert d <= 0.05 * float(np.abs(f32).max()), d
    if task == "depth":
        assert a.dtype == torch.float32
        assert np.array_equal(a.cpu().numpy(), b16[:, :, 0])
        return
    assert np.array_equal(a.cpu().numpy(), np.argmax(b16, axis=2).astype(np.uint8))
    top2 = np.sort(f32, axis=2)[:, :, -2:]
    sure = (top2[:, :, 1] - top2[:, :, 0]) > 2 * d
    ref = np.argmax(f32, axis=2).astype(np.uint8)
    assert np.array_equal(a.cpu().numpy()[sure], ref[sure])
