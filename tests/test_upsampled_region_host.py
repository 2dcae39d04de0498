"""CPU-only checks of the region-overlap term at the labels' size: the refusals of ``SegmCrossEntropy(region_at=)``
and of the two functions (raised before anything touches the device, under the caller's own name), the stepper key
and repr, what the criterion hands ``F.cross_entropy_upsampled``, and the consistency of the composed float64
restatement tests/_upsampled_region_ref.py (equal sizes; a central finite difference)."""
import numpy as np
import pytest
import torch

import _region_loss_ref as R
import _upsampled_ce_ref as U
import _upsampled_region_ref as UR

REGION_KW = dict(region="dice", region_weight=0.5, region_smooth=2.0, region_classes="all")


def crit(**kw):
    from nas_segm_amd.nn import SegmCrossEntropy

    return SegmCrossEntropy(**kw)


def test_region_at_refusals():
    # a region term on a full-size criterion stays refused unless it is asked for at the labels' size
    with pytest.raises(ValueError, match="region_at=\"labels\""):
        crit(full_size=True, region="dice")
    with pytest.raises(ValueError, match="region_at=\"labels\""):
        crit(full_size=True, region="dice", region_at="logits")
    for kw in (dict(region="dice"), dict(full_size=True), dict(), dict(full_size=False, region="jaccard")):
        with pytest.raises(ValueError, match="needs full_size=True and a region"):
            crit(region_at="labels", **kw)
    for bad in ("pixels", None, 1, "LABELS"):
        with pytest.raises(ValueError, match="region_at must be"):
            crit(full_size=True, region="dice", region_at=bad)
    for kw in (dict(lovasz_weight=1.0), dict(lovasz_weight=0.5, region="dice")):
        with pytest.raises(ValueError, match="Lovasz"):
            crit(full_size=True, region_at="labels", **dict(dict(region="dice"), **kw))
    with pytest.raises(ValueError, match="Lovasz"):
        crit(full_size=True, lovasz_weight=1.0)
    # the region's own argument errors come first, as at the logits' size
    with pytest.raises(ValueError, match="SegmCrossEntropy: region must be"):
        crit(full_size=True, region="iou", region_at="labels")
    with pytest.raises(ValueError, match="classes=\"all\" needs smooth > 0"):
        crit(full_size=True, region="dice", region_smooth=0.0, region_classes="all", region_at="labels")
    ok = crit(full_size=True, region_at="labels", **REGION_KW)
    assert ok.full_size is True and ok.region_at == "labels" and crit().region_at == "logits"


def test_function_errors_carry_the_callers_name_and_come_before_the_device():
    from nas_segm_amd import functional as F

    x, t = torch.zeros(1, 3, 2, 2), torch.zeros(1, 8, 8, dtype=torch.int64)
    for kw in (dict(region="iou"), dict(region=("tversky", 0.0, 0.0)), dict(region="dice", region_smooth=-1.0),
               dict(region="dice", region_classes="some"), dict(region="dice", region_weight=float("nan")),
               dict(region="dice", region_smooth=0.0, region_classes="all"), dict(region="dice", thresh=0.7)):
        with pytest.raises(ValueError, match="^cross_entropy_upsampled: "):
            F.cross_entropy_upsampled(x, t, **kw)
    for kw in (dict(region="iou"), dict(region=("tversky", 1.0)), dict(smooth=-1.0), dict(classes="some"),
               dict(smooth=0.0, classes="all")):
        with pytest.raises(ValueError, match="^region_overlap_loss_upsampled: "):
            F.region_overlap_loss_upsampled(x, t, **kw)
    # valid arguments, host tensors: there is no CPU fallback
    with pytest.raises(F.NassegError, match="HIP device"):
        F.cross_entropy_upsampled(x, t, region="dice")
    with pytest.raises(F.NassegError, match="HIP device"):
        F.region_overlap_loss_upsampled(x, t)
    with pytest.raises(F.NassegError, match="region_overlap_loss_upsampled: rows must be"):
        F.region_overlap_loss_upsampled(x, torch.zeros(5, 8, 8, dtype=torch.uint8), rows=[0])


def test_config_and_repr_are_unchanged_for_every_existing_kind_and_distinct_for_labels():
    w = torch.tensor([1.0, 2.0, 0.5])
    # the tuples and reprs as they were before the keyword existed
    assert crit(thresh=0.7, min_kept=5, keep_fraction=0.1, ignore_index=250).config() == (
        "ce_sel", None, 250, 0.7, 5, 0.1)
    assert crit(region="dice", region_weight=0.5).config() == (
        "ce_sel", None, 255, None, 0, 0.0, ("region", "dice", 0.5, 1.0, "present"))
    assert crit(lovasz_weight=2.0, lovasz_classes="all").config()[-1] == ("lovasz", 2.0, "all")
    assert crit(full_size=True).config() == ("ce_sel", None, 255, None, 0, 0.0, ("full_size",))
    assert crit(full_size=True).extra_repr() == (
        "classes=None, ignore_index=255, thresh=None, min_kept=0, keep_fraction=0.0, full_size=True")
    assert crit(region="dice").extra_repr() == (
        "classes=None, ignore_index=255, thresh=None, min_kept=0, keep_fraction=0.0, region='dice', "
        "region_weight=1.0, region_smooth=1.0, region_classes='present'")
    for kw in (dict(), dict(weight=w), dict(thresh=0.7, min_kept=5), dict(region="dice"), dict(lovasz_weight=1.0),
               dict(full_size=True), dict(full_size=True, thresh=0.7, min_kept=5)):
        c = crit(**kw)
        assert "region_at" not in c.extra_repr() and "region_at" not in repr(c.config())
    low, full = crit(**REGION_KW), crit(full_size=True, region_at="labels", **REGION_KW)
    assert full.config() == low.config() + (("full_size",), ("region_at", "labels"))
    assert full.extra_repr() == low.extra_repr() + ", full_size=True, region_at='labels'"
    keys = {crit().config(), low.config(), full.config(), crit(full_size=True).config(),
            crit(full_size=True, region_at="labels", **dict(REGION_KW, region_weight=0.25)).config()}
    assert len(keys) == 5  # (a step recorded for one kind is never replayed for another)
    # _terms(): what a criterion at the logits' size hands cross_entropy_select is what it handed before
    assert low._terms() == REGION_KW and crit()._terms() == {} and full._terms() == REGION_KW
    assert crit(lovasz_weight=1.0)._terms() == dict(lovasz_weight=1.0, lovasz_classes="present")


def test_the_criterion_hands_the_four_region_keywords_to_the_fused_function(monkeypatch):
    from nas_segm_amd import functional as F

    calls = []
    monkeypatch.setattr(F, "cross_entropy_upsampled", lambda *a, **k: calls.append(("up", a[2:], k)) or "U")
    monkeypatch.setattr(F, "cross_entropy_select", lambda *a, **k: calls.append(("sel", a[2:], k)) or "S")
    x, t = torch.zeros(2, 3, 2, 2), torch.zeros(2, 8, 8, dtype=torch.int64)
    cache, rows = torch.zeros(5, 8, 8, dtype=torch.uint8), torch.tensor([4, 1])
    full = crit(full_size=True, region_at="labels", thresh=0.7, min_kept=5, ignore_index=9, **REGION_KW)
    assert full(x, t) == "U" and full(x, cache, rows=rows) == "U"
    plain = crit(full_size=True, thresh=0.7, min_kept=5, ignore_index=9)
    assert plain(x, t) == "U" and plain(x, cache, rows=rows) == "U"
    assert crit(thresh=0.7, min_kept=5, ignore_index=9, **REGION_KW)(x, t) == "S"
    head = (None, 9, 0.7, 5, 0.0)
    assert calls == [("up", head, REGION_KW), ("up", head, dict(REGION_KW, rows=rows)),
                     ("up", head, {}), ("up", head, {"rows": rows}),  # (a plain full-size criterion: as today)
                     ("sel", head, REGION_KW)]


def test_signatures():
    import inspect

    from nas_segm_amd import functional as F

    p = inspect.signature(F.cross_entropy_upsampled).parameters
    assert list(p)[:9] == ["logits", "target", "weight", "ignore_index", "thresh", "min_kept", "keep_fraction",
                           "return_parts", "rows"]  # (as before; the new keywords follow)
    assert [(k, p[k].default) for k in list(p)[9:]] == [("region", None), ("region_weight", 1.0),
                                                        ("region_smooth", 1.0), ("region_classes", "present")]
    p = inspect.signature(F.region_overlap_loss_upsampled).parameters
    assert [(k, v.default) for k, v in list(p.items())[2:]] == [
        ("region", "jaccard"), ("smooth", 1.0), ("classes", "present"), ("ignore_index", 255),
        ("return_parts", False), ("rows", None)]


# ---------------------------------------------------------------------------------------------------------------
# the restatement's own consistency
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", R.PARAM_SETS)
def test_at_equal_sizes_the_composition_is_the_restatement_at_the_logits_size(params):
    region, smooth, classes = params
    x, t, w = U.make_case((2, 6, 5), (6, 5), 7, 1)
    kw = dict(region=region, region_weight=0.4, smooth=smooth, classes=classes)
    for sel in ({}, dict(thresh=0.7, min_kept=10)):
        got = UR.upsampled_region(x, t, w, **dict(sel, **kw))
        want = R.combined(x.reshape(-1, 7).astype(np.float64), t.reshape(-1), w, **dict(sel, **kw))
        assert got["loss"] == want["loss"] and got["loss_region"] == float(want["region"]["loss"])
        assert np.array_equal(got["grad"].reshape(-1, 7), want["grad"])
        assert np.array_equal(got["N"], want["region"]["N"]) and np.array_equal(got["I"], want["region"]["I"])
    alone = UR.upsampled_region(x, t, with_ce=False, **kw)
    rg = R.evaluate(x.reshape(-1, 7).astype(np.float64), t.reshape(-1), region, smooth, classes)
    assert alone["loss"] == 0.4 * float(rg["loss"]) and alone["loss_ce"] is None
    assert np.array_equal(alone["grad"].reshape(-1, 7), 0.4 * rg["grad"])


@pytest.mark.parametrize("params", R.PARAM_SETS)
def test_the_gradient_is_the_finite_difference_of_the_loss(params):
    region, smooth, classes = params
    x32, t, w = U.make_case((2, 5, 7), (19, 26), 5, 2)
    x = x32.astype(np.float64)
    kw = dict(region=region, region_weight=0.7, smooth=smooth, classes=classes)
    for with_ce in (True, False):  # (no selection: the kept set is a constant of the gradient, not of the difference)
        ref = UR.upsampled_region(x, t, w, with_ce=with_ce, **kw)
        rng = np.random.RandomState(3)
        for _ in range(6):
            idx = tuple(rng.randint(0, n) for n in x.shape)
            eps = 1e-5
            hi, lo = x.copy(), x.copy()
            hi[idx] += eps
            lo[idx] -= eps
            fd = (UR.upsampled_region(hi, t, w, with_ce=with_ce, **kw)["loss"] -
                  UR.upsampled_region(lo, t, w, with_ce=with_ce, **kw)["loss"]) / (2 * eps)
            assert abs(fd - ref["grad"][idx]) <= 1e-8 + 1e-6 * abs(ref["grad"][idx]), (idx, fd, ref["grad"][idx])


def test_the_fp32_restatement_is_close_to_float64():
    x, t, w = U.make_case((2, 5, 7), (19, 26), 19, 0)
    for region, smooth, classes in R.PARAM_SETS:
        kw = dict(region=region, region_weight=0.5, smooth=smooth, classes=classes)
        ref = UR.upsampled_region(x, t, w, **kw)
        own = UR.upsampled_region_fp32(x, t, ref["kept"], w, **kw)
        assert abs(own["loss"] - ref["loss"]) <= 1e-5 * ref["loss"]
        assert abs(own["loss_region"] - ref["loss_region"]) <= 1e-5 * ref["loss_region"]
        assert np.abs(own["grad"] - ref["grad"]).max() <= 1e-5 * np.abs(ref["grad"]).max()
        assert np.abs(own["S"] - ref["S"]).max() <= 1e-5 * ref["S"].max()
