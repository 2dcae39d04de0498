"""CPU-only checks of the full-size cross-entropy: the float64 restatement (tests/_upsampled_ce_ref.py) against torch's
float64 interpolate + cross_entropy + autograd, what the kernel's fp32 source coordinate costs, the criterion's
``full_size`` option, and what the engine hands a full-size criterion (untouched labels, every head at its own size)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF
from torch import nn

import _upsampled_ce_ref as U

# (logits (B, h, w), labels (H, W), C): up by ragged factors, integer factors, down, mixed, degenerate
SHAPES = (((2, 5, 7), (19, 26), 19), ((1, 8, 16), (32, 64), 21), ((1, 9, 11), (4, 5), 5), ((1, 3, 12), (11, 5), 7),
          ((1, 1, 1), (7, 9), 3), ((1, 4, 6), (1, 1), 4), ((1, 1, 6), (5, 23), 19), ((2, 6, 5), (6, 5), 6))


def torch_reference(x, t, w):
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    up = TF.interpolate(xt, size=tuple(t.shape[1:]), mode="bilinear", align_corners=False)
    loss = TF.cross_entropy(up, torch.from_numpy(t.astype(np.int64)), ignore_index=255,
                            weight=None if w is None else torch.from_numpy(w.astype(np.float64)))
    (grad,) = torch.autograd.grad(loss, xt)
    return loss.item(), grad.permute(0, 2, 3, 1).numpy(), up.detach().permute(0, 2, 3, 1).numpy()


def test_restatement_with_float64_coordinates_equals_torch():
    for lshape, tshape, C in SHAPES:
        x32, t, w = U.make_case(lshape, tshape, C, 3)
        x = x32.astype(np.float64)
        for weight in (None, w):
            ref = U.upsampled(x, t, weight, coeff_dtype=np.float64)
            loss, grad, up = torch_reference(x, t, weight)
            assert np.abs(ref["v"] - up).max() <= 1e-10
            assert abs(ref["loss"] - loss) <= 1e-10 * abs(loss)
            assert np.abs(ref["grad"] - grad).max() <= 1e-10
            assert ref["n_kept"] == ref["n"] == int((t != 255).sum()) and ref["tau"] == -np.inf


def test_fp32_coordinates_stay_within_what_the_coordinate_explains():
    """The kernel's coordinate src = scale * (dst + 0.5) - 0.5 is fp32: scale carries a relative error of eps32 / 2 and
    the result is rounded once more, so |src - exact| <= eps32 * (max coordinate + 1), and each of the two axes moves an
    interpolated value by at most that times the largest difference of neighbouring logits.  The second weight
    l0 = 1 - l1 is rounded as well (half an eps32): per axis the value moves by at most eps32 / 2 * max |x| more."""
    eps32 = float(np.finfo(np.float32).eps)
    for lshape, tshape, C in SHAPES:
        x32, t, w = U.make_case(lshape, tshape, C, 4)
        x = x32.astype(np.float64)
        a = U.upsampled(x, t, w, coeff_dtype=np.float32)
        b = U.upsampled(x, t, w, coeff_dtype=np.float64)
        dmax = max([float(np.abs(np.diff(x, axis=ax)).max()) for ax in (1, 2) if x.shape[ax] > 1] + [0.0])
        bound = 2.0 * eps32 * (max(lshape[1], lshape[2]) + 1) * dmax + eps32 * float(np.abs(x).max())
        got = float(np.abs(a["v"] - b["v"]).max())
        print(lshape, tshape, "max |v32 - v64|", got, "bound", bound)
        assert got <= bound
        if tuple(lshape[1:]) == tuple(tshape):  # equal sizes are the identity in both
            assert np.array_equal(a["v"], x) and np.array_equal(b["v"], x)
        # |d loss / d v| sums to at most 2 over a pixel's channels, and the loss is a weighted mean of the pixels'
        assert abs(a["loss"] - b["loss"]) <= 2.0 * bound + 1e-15


def test_the_gradient_is_the_transpose_of_the_interpolation():
    """sum(dx * e) == sum(g * interpolate(e)) for any e: the explicit double sum is the adjoint of the three lines"""
    rng = np.random.RandomState(0)
    for (B, h, w), (H, W), C in SHAPES:
        cy, cx = U.coeffs(H, h), U.coeffs(W, w)
        g, e = rng.randn(B, H, W, C), rng.randn(B, h, w, C)
        lhs = (U.gather(g, U.weight_matrix(cy, h), U.weight_matrix(cx, w)) * e).sum()
        rhs = (g * U.interpolate(e, cy, cx)).sum()
        assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(rhs))
        for co in (cy, cx):  # the two weights of a label coordinate add up to 1 (in fp32: exactly or one rounding)
            assert np.abs(co[2] + co[3] - 1.0).max() <= 2.0 ** -24


def test_down_sampling_leaves_logits_no_label_pixel_touches():
    x32, t, w = U.make_case((1, 9, 11), (4, 5), 19, 0)
    ref = U.upsampled(x32.astype(np.float64), t, w)
    touched = U.weight_matrix(U.coeffs(4, 9), 9).any(axis=0)[:, None] & U.weight_matrix(U.coeffs(5, 11), 11).any(axis=0)
    assert (~touched).any() and not ref["grad"][0][~touched].any()


def test_fp32_restatement_is_close_to_float64():
    x32, t, w = U.make_case((2, 5, 7), (19, 26), 19, 0)
    ref = U.upsampled(x32.astype(np.float64), t, w, thresh=0.7, min_kept=50)
    loss, grad, pl = U.upsampled_fp32(x32, t, ref["kept"], w)
    assert abs(loss - ref["loss"]) <= 1e-5 * ref["loss"]
    assert np.abs(grad - ref["grad"]).max() <= 1e-5 * np.abs(ref["grad"]).max()
    assert np.abs(pl - ref["pixel_loss"])[ref["kept"]].max() <= 1e-4
    assert 0 < ref["n_kept"] < ref["n"]


# ---------------------------------------------------------------------------------------------------------------
# the criterion and the engine
# ---------------------------------------------------------------------------------------------------------------
def test_full_size_option_of_the_criterion():
    from nas_segm_amd.nn import SegmCrossEntropy

    w = torch.tensor([1.0, 2.0, 0.5])
    for kw in (dict(), dict(weight=w), dict(thresh=0.7, min_kept=5, keep_fraction=0.1, ignore_index=250)):
        plain, full = SegmCrossEntropy(**kw), SegmCrossEntropy(full_size=True, **kw)
        assert plain.full_size is False and full.full_size is True
        if "weight" in kw:  # (the key carries the weight BUFFER's identity)
            full.weight = plain.weight
        assert full.config() == plain.config() + (("full_size",),) and full.config()[-1] == ("full_size",)
        assert full.extra_repr() == plain.extra_repr() + ", full_size=True" and "full_size" not in plain.extra_repr()
        assert "full_size=True" in repr(full)
    # full_size=False is today's criterion: the tuple as it was before the option existed
    crit = SegmCrossEntropy(thresh=0.7, min_kept=5, keep_fraction=0.1, ignore_index=250)
    assert crit.config() == ("ce_sel", None, 250, 0.7, 5, 0.1)
    assert SegmCrossEntropy(region="dice").config()[-1][0] == "region"
    assert crit.extra_repr() == "classes=None, ignore_index=250, thresh=0.7, min_kept=5, keep_fraction=0.1"
    for kw in (dict(region="dice"), dict(region=("tversky", 0.3, 0.7)), dict(lovasz_weight=1.0),
               dict(region="jaccard", lovasz_weight=0.5),
               dict(thresh=0.7), dict(thresh=0.7, min_kept=0), dict(keep_fraction=1.5, min_kept=1), dict(min_kept=-1),
               dict(thresh=1.0, min_kept=1)):
        with pytest.raises(ValueError):
            SegmCrossEntropy(full_size=True, **kw)
    SegmCrossEntropy(full_size=False, region="dice", lovasz_weight=1.0)  # (the terms stay available at the logits' size)


def test_full_size_criterion_reaches_the_new_function_and_the_plain_one_does_not(monkeypatch):
    from nas_segm_amd import functional as F
    from nas_segm_amd.nn import SegmCrossEntropy

    calls = []
    monkeypatch.setattr(F, "cross_entropy_upsampled", lambda *a, **k: calls.append(("up", a[2:], k)) or "U")
    monkeypatch.setattr(F, "cross_entropy_select", lambda *a, **k: calls.append(("sel", a[2:], k)) or "S")
    x, t = torch.zeros(1, 3, 2, 2), torch.zeros(1, 8, 8, dtype=torch.int64)
    assert SegmCrossEntropy(full_size=True, thresh=0.7, min_kept=5, ignore_index=9)(x, t) == "U"
    assert SegmCrossEntropy(thresh=0.7, min_kept=5, ignore_index=9)(x, t) == "S"
    assert calls == [("up", (None, 9, 0.7, 5, 0.0), {}), ("sel", (None, 9, 0.7, 5, 0.0), {})]


def test_the_function_refuses_a_bad_selection_triple_before_anything_else():
    from nas_segm_amd import functional as F

    x, t = torch.zeros(1, 3, 2, 2), torch.zeros(1, 8, 8, dtype=torch.int64)
    for kw in (dict(thresh=0.7), dict(thresh=1.0, min_kept=1), dict(keep_fraction=1.5, min_kept=1), dict(min_kept=-1)):
        with pytest.raises(ValueError, match="cross_entropy_upsampled"):
            F.cross_entropy_upsampled(x, t, **kw)
    with pytest.raises(F.NassegError):  # (valid arguments, host tensors: there is no CPU fallback)
        F.cross_entropy_upsampled(x, t)


def test_segm_crit_dispatch_and_task0_refusal():
    from nas_segm_amd.engine.graphed import GraphedTask0Step
    from nas_segm_amd.engine.trainer import _segm_crit, train_task0
    from nas_segm_amd.nn import SegmCrossEntropy

    full = SegmCrossEntropy(full_size=True)
    assert not full.selects and full.weight is None
    assert _segm_crit(full) is full and _segm_crit(full, "cpu") is full
    assert _segm_crit(SegmCrossEntropy()) is None  # (as ever)
    sel = SegmCrossEntropy(full_size=True, thresh=0.7, min_kept=3)
    assert _segm_crit(sel) is sel
    with pytest.raises(ValueError, match="full-size"):
        train_task0.__wrapped__({}, None, None, 0, full, None, 2, False, False, 0.0, 0.0, False)
    with pytest.raises(ValueError, match="full-size"):
        GraphedTask0Step({}, None, None, 2, segm_crit=full)


def test_task1_loss_hands_a_full_size_criterion_untouched_labels_and_every_head_at_its_own_size(monkeypatch):
    from nas_segm_amd import functional as F
    from nas_segm_amd.engine.trainer_common import segmentation_loss, task1_loss

    resized = []
    monkeypatch.setattr(F, "nearest_label_resize", lambda t, size, out=None: resized.append(("labels", tuple(size))) or
                        TF.interpolate(t[:, None].float(), size=tuple(size), mode="nearest").long()[:, 0])
    monkeypatch.setattr(F, "bilinear_resize", lambda x, size: resized.append(("head", tuple(size))) or
                        TF.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False))

    class Crit(nn.Module):
        def __init__(self, full_size):
            super(Crit, self).__init__()
            self.full_size = full_size
            self.seen = []

        def forward(self, logits, target):
            self.seen.append((tuple(logits.shape), tuple(target.shape), target.data_ptr()))
            return logits.sum() * 0.0 + float(len(self.seen))

    main, aux = torch.zeros(2, 5, 4, 6), [torch.zeros(2, 5, 2, 3), torch.zeros(2, 5, 1, 2)]
    target = torch.zeros(2, 16, 24, dtype=torch.int64)

    def net(image):
        return main, aux

    full = Crit(True)
    loss = task1_loss(net, None, target, 255, 0.5, full)
    assert resized == []
    assert full.seen == [((2, 5, 4, 6), (2, 16, 24), target.data_ptr()), ((2, 5, 2, 3), (2, 16, 24), target.data_ptr()),
                         ((2, 5, 1, 2), (2, 16, 24), target.data_ptr())]
    assert float(loss) == 1.0 + 0.5 * 2.0 + 0.5 * 3.0
    full = Crit(True)
    task1_loss(net, None, target, 255, 0, full)  # (no auxiliary term without a weight)
    assert len(full.seen) == 1 and resized == []

    normal = Crit(False)
    task1_loss(net, None, target, 255, 0.5, normal)
    assert resized == [("labels", (4, 6)), ("head", (4, 6)), ("head", (4, 6))]
    assert [s[:2] for s in normal.seen] == [((2, 5, 4, 6), (2, 4, 6))] * 3
    # a criterion without the attribute (any callable a caller wrote before the option existed) is a normal one
    del resized[:]
    segmentation_loss(main, aux, torch.zeros(2, 4, 6, dtype=torch.int64), 255, 0.5, segm_crit=lambda x, t: x.sum())
    assert resized == [("head", (4, 6)), ("head", (4, 6))]
