"""CPU-only checks of the region-overlap term (soft Jaccard / Dice / Tversky): the float64 restatement
(tests/_region_loss_ref.py) against torch float64 autograd of the textbook formula, the argument checks of the
criterion and the functional, and how the engine routes a criterion that carries the term."""
import numpy as np
import pytest
import torch
from torch import nn

import _region_loss_ref as R


def _inputs(P, C, seed, ignored=0.2):
    rng = np.random.RandomState(seed)
    x = rng.randn(P, C) * 3.0
    t = rng.randint(0, C, size=P)
    t[rng.rand(P) < ignored] = 255
    return x, t


def _textbook(x, t, region, smooth, classes):
    """1 - mean over K of (I + s) / (I + a FP + b FN + s), FP = S - I, FN = N - I, by torch float64 autograd"""
    a, b = R.alpha_beta(region)
    C = x.shape[1]
    xt = torch.from_numpy(x).requires_grad_(True)
    valid = torch.from_numpy((t != 255) & (t >= 0) & (t < C))
    q = torch.softmax(xt, 1)[valid]
    y = torch.nn.functional.one_hot(torch.from_numpy(t)[valid], C).double()
    I, S, N = (q * y).sum(0), q.sum(0), y.sum(0)
    T = (I + smooth) / (I + a * (S - I) + b * (N - I) + smooth)
    K = torch.ones(C, dtype=torch.bool) if classes == "all" else N > 0
    if int(K.sum()) == 0:
        return 0.0, np.zeros_like(x)
    loss = 1.0 - T[K].mean()
    (grad,) = torch.autograd.grad(loss, xt)
    return loss.item(), grad.numpy()


@pytest.mark.parametrize("absent", [False, True])
@pytest.mark.parametrize("C", [19, 21, 64])
def test_restatement_equals_torch_float64_autograd(C, absent):
    x, t = _inputs(2 * 13 * 17, C, C)
    if absent:
        t = R.drop_odd_classes(t)
    for region, smooth, classes in R.PARAM_SETS:
        ref = R.evaluate(x, t, region, smooth, classes)
        loss, grad = _textbook(x, t, region, smooth, classes)
        gmax = float(np.abs(grad).max())
        assert gmax > 0
        assert abs(ref["loss"] - loss) <= 1e-12 * gmax, (region, ref["loss"], loss)
        assert float(np.abs(ref["grad"] - grad).max()) <= 1e-12 * gmax, region
        assert not ref["grad"][~ref["valid"]].any()
        present = np.array([(t == c).any() for c in range(C)])
        assert np.array_equal(ref["N"] > 0, present)
        assert np.array_equal(ref["K"], np.ones(C, bool) if classes == "all" else present)
        if absent:
            assert 2 <= int(present.sum()) < C
            assert int(present.sum()) == (C + 1) // 2


def test_no_valid_pixel_is_zero_loss_and_zero_gradient():
    x, t = _inputs(40, 7, 1)
    for labels in (np.full(40, 255), np.full(40, 7), np.full(40, -1)):
        ref = R.evaluate(x, labels, "jaccard", 1.0, "present")
        assert ref["loss"] == 0.0 and not ref["grad"].any() and not ref["K"].any()
        ref = R.evaluate(x, labels, "dice", 0.0, "present")
        assert ref["loss"] == 0.0 and not ref["grad"].any()


def test_zero_region_weight_is_the_plain_restatement():
    import _segm_loss_ref as CE

    x, t = _inputs(300, 19, 2)
    w = np.random.RandomState(3).rand(19) + 0.5
    plain = CE.cross_entropy_select(x, t, w, thresh=0.7, min_kept=20)
    both = R.combined(x, t, w, thresh=0.7, min_kept=20, region="dice", region_weight=0.0)
    assert both["loss"] == plain["loss"] and np.array_equal(both["grad"], plain["grad"])
    half = R.combined(x, t, w, thresh=0.7, min_kept=20, region="dice", region_weight=0.5)
    assert half["loss"] == plain["loss"] + 0.5 * R.evaluate(x, t, "dice")["loss"]
    assert float(np.abs(half["grad"] - plain["grad"]).max()) > 0


BAD = [dict(region=("tversky", 0.0, 0.0)), dict(region=("tversky", -0.1, 0.5)), dict(region=("tversky", 0.5, -0.1)),
       dict(region="jaccard", region_smooth=-1.0), dict(region="dice", region_smooth=0.0, region_classes="all"),
       dict(region="lovasz"), dict(region=("tversky", 0.5)), dict(region=("focal", 0.5, 0.5)),
       dict(region="jaccard", region_classes="some"), dict(region="jaccard", region_weight=float("nan"))]


def test_constructor_and_functional_refuse_what_the_definition_has_no_meaning_for():
    from nas_segm_amd import functional as F
    from nas_segm_amd.nn import SegmCrossEntropy

    x, t = torch.zeros(1, 3, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64)  # (refused before any device is asked for)
    for kw in BAD:
        with pytest.raises(ValueError):
            SegmCrossEntropy(**kw)
        with pytest.raises(ValueError):
            F.cross_entropy_select(x, t, **kw)
        alone = {k[len("region_"):] if k.startswith("region_") else k: v for k, v in kw.items()}
        if "weight" in alone:
            continue
        with pytest.raises(ValueError):
            F.region_overlap_loss(x, t, **alone)
    crit = SegmCrossEntropy(region=["tversky", 0.3, 0.7], region_weight=0.5, region_smooth=0.0)
    assert crit.region == ("tversky", 0.3, 0.7) and not crit.selects and crit.weight is None
    assert "region=" in crit.extra_repr() and "region" not in SegmCrossEntropy(min_kept=3).extra_repr()
    SegmCrossEntropy(region="dice", region_smooth=0.0)  # (smooth = 0 is fine with the present classes)
    SegmCrossEntropy(region=("tversky", 0.0, 1.0), region_classes="all")


def test_segm_crit_routes_a_region_only_criterion_as_non_plain():
    from nas_segm_amd.engine.trainer import _ignore_index, _segm_crit
    from nas_segm_amd.nn import SegmCrossEntropy

    assert _segm_crit(SegmCrossEntropy()) is None
    for kw in (dict(region="jaccard"), dict(region="dice", region_weight=0.0), dict(region=("tversky", 0.3, 0.7)),
               dict(region="dice", thresh=0.7, min_kept=3), dict(region="dice", weight=[1.0, 2.0])):
        crit = SegmCrossEntropy(**kw)
        assert _segm_crit(crit) is crit
    assert _ignore_index(SegmCrossEntropy(region="dice", ignore_index=7)) == 7


def test_config_without_a_region_is_unchanged_and_with_one_carries_its_four_values():
    from nas_segm_amd.nn import SegmCrossEntropy

    w = torch.tensor([1.0, 2.0, 0.5])
    crit = SegmCrossEntropy(weight=w, ignore_index=11, thresh=0.7, min_kept=3, keep_fraction=0.25)
    assert crit.config() == ("ce_sel", id(crit.weight), 11, 0.7, 3, 0.25)  # (what the parent commit returns)
    assert SegmCrossEntropy().config() == ("ce_sel", None, 255, None, 0, 0.0)
    assert crit.extra_repr() == "classes=3, ignore_index=11, thresh=0.7, min_kept=3, keep_fraction=0.25"
    base = dict(region="dice", region_weight=0.5, region_smooth=1.0, region_classes="present")
    a = SegmCrossEntropy(**base)
    assert a.config() == SegmCrossEntropy(**base).config() and a.config() != SegmCrossEntropy().config()
    assert a.config()[:6] == SegmCrossEntropy().config()
    for change in (dict(region="jaccard"), dict(region=("tversky", 0.5, 0.5)), dict(region_weight=0.25),
                   dict(region_smooth=0.5), dict(region_classes="all")):
        assert SegmCrossEntropy(**dict(base, **change)).config() != a.config(), change
    a.region_weight = 0.75  # (changed between steps: a new key for the stepper caches)
    assert a.config() != SegmCrossEntropy(**base).config()


def test_steps_call_the_criterion_with_its_region_term(monkeypatch):
    """the functional module patched as tests/test_segm_loss_host.py patches it: a region-only criterion reaches
    F.cross_entropy_select with its four values, through the step and through the epoch"""
    import torch.nn.functional as TF

    from nas_segm_amd import functional as F
    from nas_segm_amd.engine import Segmenter
    from nas_segm_amd.engine.trainer import segmenter_step, train_segmenter
    from nas_segm_amd.nn import SegmCrossEntropy

    calls = []

    def nll(logits, target, ignore_index=255):
        calls.append(("nll", ignore_index))
        return TF.nll_loss(TF.log_softmax(logits, 1), target, ignore_index=ignore_index)

    def ce_sel(logits, target, weight=None, ignore_index=255, thresh=None, min_kept=0, keep_fraction=0.0, **region):
        calls.append(("sel", ignore_index, thresh, min_kept, keep_fraction, tuple(sorted(region.items()))))
        return TF.cross_entropy(logits, target, weight=weight, ignore_index=ignore_index)

    monkeypatch.setattr(F, "log_softmax_nll", nll)
    monkeypatch.setattr(F, "cross_entropy_select", ce_sel)
    monkeypatch.setattr(F, "nearest_label_resize", lambda t, size, out=None: TF.interpolate(
        t[:, None].float(), size=tuple(size), mode="nearest").long()[:, 0])
    monkeypatch.setattr(F, "bilinear_resize", lambda x, size: x)

    class Enc(nn.Module):
        def __init__(self):
            super(Enc, self).__init__()
            self.conv = nn.Conv2d(3, 4, 3, stride=2, padding=1)

        def forward(self, x):
            return [torch.relu(self.conv(x))]

    class Dec(nn.Module):
        def __init__(self):
            super(Dec, self).__init__()
            self.clf = nn.Conv2d(4, 5, 1)

        def forward(self, feats):
            return self.clf(feats[0])

    def run(crit, through_epoch):
        torch.manual_seed(3)
        net = Segmenter(Enc(), Dec())
        oe = torch.optim.SGD(net.encoder.parameters(), lr=0.1)
        od = torch.optim.SGD(net.decoder.parameters(), lr=0.1)
        g = torch.Generator().manual_seed(5)
        batch = {"image": torch.randn(2, 3, 8, 12, generator=g), "mask": torch.randint(0, 5, (2, 8, 12), generator=g)}
        del calls[:]
        if through_epoch:
            assert train_segmenter.__wrapped__(net, [batch], oe, od, 0, crit, False, 3.0, 3.0, False) is None
        else:
            segmenter_step(net, batch["image"], batch["mask"], oe, od, 255, 3.0, 3.0, segm_crit=crit)
        return list(calls)

    want = (("region", "dice"), ("region_classes", "all"), ("region_smooth", 2.0), ("region_weight", 0.5))
    for through_epoch in (False, True):
        assert run(SegmCrossEntropy(), through_epoch) == [("nll", 255)]
        crit = SegmCrossEntropy(region="dice", region_weight=0.5, region_smooth=2.0, region_classes="all")
        assert run(crit, through_epoch) == [("sel", 255, None, 0, 0.0, want)]
        assert run(SegmCrossEntropy(min_kept=9), through_epoch) == [("sel", 255, None, 9, 0.0, ())]


def test_evaluate_candidate_hands_the_region_criterion_to_the_epoch(monkeypatch):
    from nas_segm_amd.engine import search
    from nas_segm_amd.nn import SegmCrossEntropy

    class Model(nn.Module):
        def __init__(self):
            super(Model, self).__init__()
            self.encoder, self.decoder = nn.Linear(2, 2), nn.Linear(2, 2)

    class Holder(object):
        module = Model()

    seen = []
    monkeypatch.setattr(search, "build_candidate", lambda *a, **k: Holder())
    monkeypatch.setattr(search, "train_segmenter", lambda seg, batches, oe, od, epoch, crit, *a, **k: seen.append(crit))
    monkeypatch.setattr(search, "validate", lambda *a, **k: 0.5)
    crit = SegmCrossEntropy(region="jaccard", region_weight=0.5)
    assert search.evaluate_candidate([], [], [], device="cpu", segm_crit=crit) == 0.5
    assert seen[0] is crit and seen[0].region == "jaccard"
