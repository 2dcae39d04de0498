"""CPU-only checks of what the segmentation losses share on the host (nas_segm_amd.functional): every loss refuses a
bad target or bad class weights under ITS OWN name - the checks live in one place, F._segm_inputs, which runs before
any library call - and cross_entropy_select's keyword arguments become the configurations of its three terms."""
import pytest
import torch

B, C, H, W = 2, 5, 4, 6


def _logits():
    return torch.zeros(B, C, H, W)


def _labels(shape=(B, H, W), dtype=torch.int64):
    return torch.zeros(shape, dtype=dtype)


@pytest.fixture
def F(monkeypatch):
    """the functional module with host tensors let through to the argument checks (they come first; a call that
    passed them would need the library)"""
    from nas_segm_amd import functional

    monkeypatch.setattr(functional, "require_device", lambda *tensors: None)
    return functional


# name -> (the call with (logits, target, weight), does it take class weights?)
LOSSES = {
    "log_softmax_nll": (lambda F, x, t, w: F.log_softmax_nll(x, t), False),
    "log_softmax_nll_mse": (lambda F, x, t, w: F.log_softmax_nll_mse(x, t, torch.zeros_like(x)), False),
    "cross_entropy_select": (lambda F, x, t, w: F.cross_entropy_select(x, t, w), True),
    "cross_entropy_select+region": (lambda F, x, t, w: F.cross_entropy_select(x, t, w, region="dice"), True),
    "cross_entropy_select+lovasz": (lambda F, x, t, w: F.cross_entropy_select(x, t, w, lovasz_weight=0.5), True),
    "cross_entropy_select+both": (
        lambda F, x, t, w: F.cross_entropy_select(x, t, w, thresh=0.7, min_kept=3, region="jaccard", lovasz_weight=1.0),
        True),
    "region_overlap_loss": (lambda F, x, t, w: F.region_overlap_loss(x, t), False),
    "lovasz_softmax_loss": (lambda F, x, t, w: F.lovasz_softmax_loss(x, t, return_parts=True), False),
    "cross_entropy_upsampled": (lambda F, x, t, w: F.cross_entropy_upsampled(x, t, w), True),
}


def _refused(F, name, target, weight=None):
    call, _ = LOSSES[name]
    with pytest.raises(F.NassegError) as e:
        call(F, _logits(), target, weight)
    assert str(e.value).startswith(name.split("+")[0] + ": "), str(e.value)
    return str(e.value)


@pytest.mark.parametrize("name", sorted(LOSSES))
def test_a_bad_target_is_refused_under_the_name_of_the_function_called(F, name):
    full_size = name == "cross_entropy_upsampled"
    # the full-size loss takes labels of any size, but of the logits' batch and with three dimensions
    shapes = ((B + 1, H, W), (B, H, W, 1), (B, 0, W)) if full_size else ((B, H, W + 1), (B, H * W), (B + 1, H, W))
    for shape in shapes:
        msg = _refused(F, name, _labels(shape))
        assert str(shape) in msg
        assert ("must be uint8 or int64 of shape" if full_size else "does not match logits") in msg
    for dtype in (torch.int32, torch.float32, torch.bool):
        assert "labels must be int64 or uint8" in _refused(F, name, _labels(dtype=dtype))


@pytest.mark.parametrize("name", sorted(n for n in LOSSES if LOSSES[n][1]))
def test_bad_class_weights_are_refused_under_the_name_of_the_function_called(F, name):
    for weight in (torch.ones(C + 1), torch.ones(C - 1), torch.ones(1, C), torch.ones(C, dtype=torch.float64),
                   torch.ones(C, dtype=torch.int64)):
        msg = _refused(F, name, _labels(), weight)
        assert "the class weights must be fp32 of shape ({},)".format(C) in msg


def test_segm_inputs_hands_back_what_the_kernels_read(F):
    x = torch.randn(B, C, H, W)
    w = torch.ones(2 * C)[::2]
    for dtype, esz in ((torch.int64, 8), (torch.uint8, 1)):
        logits, target, got_esz, weight = F._segm_inputs("f", x, _labels((B, W, H), dtype).transpose(1, 2), w)
        assert logits.is_contiguous(memory_format=torch.channels_last) and torch.equal(logits, x)
        assert target.is_contiguous() and target.dtype == dtype and got_esz == esz
        assert weight.is_contiguous() and torch.equal(weight, w)
    assert F._segm_inputs("f", x, _labels(), None)[3] is None
    big = (B, 3 * H, 2 * W + 1)
    assert F._segm_inputs("f", x, _labels(big), None, same_size=False)[1].shape == big
    with pytest.raises(F.NassegError, match="^f: target"):
        F._segm_inputs("f", x, _labels((B, 3 * H, W)), None)


def test_segm_inputs_refuses_host_tensors():
    from nas_segm_amd import functional as Fn

    with pytest.raises(Fn.NassegError, match="no CPU"):
        Fn._segm_inputs("f", _logits(), _labels(), None)


def test_keywords_become_the_three_configurations():
    from nas_segm_amd import functional as Fn
    from nas_segm_amd.nn import SegmCrossEntropy

    who = "cross_entropy_select"
    select = dict(thresh=0.7, min_kept=50, keep_fraction=0.25)
    region = dict(region=("tversky", 0.3, 0.7), region_weight=2.0, region_smooth=0.5, region_classes="all")
    lovasz = dict(lovasz_weight=0.5, lovasz_classes="all")
    want_sel = Fn._select_config(who, 0.7, 50, 0.25)
    want_reg = Fn._region_config(who, ("tversky", 0.3, 0.7), 0.5, "all", 2.0)
    want_lov = Fn._lovasz_config(who, 0.5, "all")
    assert Fn._segm_config(who) == (Fn._select_config(who, None, 0, 0.0), None, None)
    assert Fn._segm_config(who, **select) == (want_sel, None, None)
    assert Fn._segm_config(who, **dict(select, **region)) == (want_sel, want_reg, None)
    assert Fn._segm_config(who, **dict(select, **lovasz)) == (want_sel, None, want_lov)
    assert Fn._segm_config(who, **dict(region, **lovasz)) == (Fn._select_config(who, None, 0, 0.0), want_reg, want_lov)
    everything = dict(select, **dict(region, **lovasz))
    assert Fn._segm_config(who, **everything) == (want_sel, want_reg, want_lov)
    # positionally, in the order of cross_entropy_select's own parameters
    assert Fn._segm_config(who, 0.7, 50, 0.25, ("tversky", 0.3, 0.7), 2.0, 0.5, "all", 0.5, "all") == (
        want_sel, want_reg, want_lov)
    assert Fn._segm_config(who, region="dice")[1] == Fn._region_config(who, "dice", 1.0, "present", 1.0)
    assert Fn._segm_config(who, lovasz_weight=2)[2] == Fn._lovasz_config(who, 2, "present")
    # a term that is absent is not looked at; one that is present is checked as its own function checks it
    assert Fn._segm_config(who, region_classes="some", lovasz_classes="some") == Fn._segm_config(who)
    for bad in (dict(thresh=0.7), dict(region="iou"), dict(region="dice", region_classes="some"),
                dict(region="dice", region_classes="all", region_smooth=0.0), dict(lovasz_weight=float("nan")),
                dict(lovasz_weight=1.0, lovasz_classes="some")):
        with pytest.raises(ValueError, match="^" + who + ": "):
            Fn._segm_config(who, **bad)
    # the criterion hands its attributes to the same function: the keywords of the terms it has, and no others
    crit = SegmCrossEntropy(**everything)
    assert crit._terms() == dict(region, **lovasz)
    assert Fn._segm_config(who, crit.thresh, crit.min_kept, crit.keep_fraction, **crit._terms()) == (
        want_sel, want_reg, want_lov)
    assert SegmCrossEntropy(**select)._terms() == {} and SegmCrossEntropy(**dict(select, **lovasz))._terms() == lovasz
    assert SegmCrossEntropy(region=["tversky", 0.3, 0.7])._terms()["region"] == ("tversky", 0.3, 0.7)
