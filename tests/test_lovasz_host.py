"""CPU-only checks of the Lovasz-Softmax term: the float64 restatement (tests/_lovasz_ref.py) against a torch float64
autograd composition of the published formula (sort, cumsum, jaccard[1:] -= jaccard[:-1], dot), its closed forms, its
tie rule, the argument checks of the criterion and the functional, and how the engine routes a criterion with the term."""
import numpy as np
import pytest
import torch
from torch import nn

import _lovasz_ref as L
import _region_loss_ref as R


def make_case(shape, C, seed, absent=False):
    """the inputs of tests/test_hip_lovasz.py's make_case (logits and labels)"""
    B, H, W = shape
    P = B * H * W
    rng = np.random.RandomState(seed)
    x = np.clip(rng.randn(P, C), -12.0, 12.0).astype(np.float32)
    t = rng.randint(0, C, size=P)
    ignored = rng.rand(P) < 0.2
    boost = (rng.rand(P) < 0.6) & ~ignored
    x[np.arange(P)[boost], t[boost]] += np.float32(6.0)
    t[ignored] = 255
    return x.astype(np.float64), (R.drop_odd_classes(t) if absent else t)


def published(x, t, classes):
    """the public implementation's lovasz_softmax_flat, in float64 under autograd"""
    C = x.shape[1]
    xt = torch.from_numpy(x).requires_grad_(True)
    valid = torch.from_numpy(L.valid_mask(t, C))
    probas = torch.softmax(xt, 1)[valid]
    labels = torch.from_numpy(t)[valid]
    losses = []
    for c in range(C):
        fg = (labels == c).double()
        if classes == "present" and fg.sum() == 0:
            continue
        errors_sorted, perm = torch.sort((fg - probas[:, c]).abs(), 0, descending=True)
        gt_sorted = fg[perm]
        gts = gt_sorted.sum()
        intersection = gts - gt_sorted.cumsum(0)
        union = gts + (1 - gt_sorted).cumsum(0)
        jaccard = 1.0 - intersection / union
        if len(gt_sorted) > 1:
            jaccard[1:] = jaccard[1:] - jaccard[:-1]
        losses.append(torch.dot(errors_sorted, jaccard.detach()))
    loss = torch.stack(losses).mean()
    (grad,) = torch.autograd.grad(loss, xt)
    return loss.item(), grad.numpy()


@pytest.mark.parametrize("classes", ["present", "all"])
@pytest.mark.parametrize("absent", [False, True])
@pytest.mark.parametrize("C", [19, 21, 64])
def test_restatement_equals_the_published_formula_under_float64_autograd(C, absent, classes):
    x, t = make_case((2, 13, 17), C, C, absent)
    ref = L.evaluate(x, t, classes)
    v = ref["valid"]
    # tie-free, and the fp32 order is the float64 order: otherwise the two would differ by the order alone
    for c in np.nonzero(ref["K"])[0]:
        e64 = ref["errors"][v, c]
        assert len(np.unique(e64.astype(np.float32))) == len(e64)
        assert np.array_equal(np.argsort(-e64, kind="stable"), np.argsort(-e64.astype(np.float32), kind="stable"))
    loss, grad = published(x, t, classes)
    gmax = float(np.abs(grad).max())
    assert gmax > 0 and abs(ref["loss"] - loss) <= 1e-8 * abs(loss)
    assert float(np.abs(ref["grad"] - grad).max()) <= 1e-12 * gmax
    assert not ref["grad"][~v].any()
    present = np.array([(t == c).any() for c in range(C)])
    assert np.array_equal(ref["K"], np.ones(C, bool) if classes == "all" else present)
    assert (ref["rank"][~v] == -1).all() and (ref["rank"][v][:, ~ref["K"]] == -1).all()
    assert all(sorted(ref["rank"][v, c].tolist()) == list(range(int(v.sum()))) for c in np.nonzero(ref["K"])[0])


def test_closed_forms_are_the_jaccard_differences():
    rng = np.random.RandomState(0)
    for n, Nc in ((1, 0), (1, 1), (7, 0), (50, 1), (200, 60), (1000, 999)):
        fg = np.zeros(n, bool)
        fg[rng.permutation(n)[:Nc]] = True
        g, d = L.lovasz_gradient(fg, Nc), L.jaccard_differences(fg, Nc)
        assert float(np.abs(g - d).max()) <= 4e-16, (n, Nc)
        assert abs(g.sum() - 1.0) <= 1e-12  # (they telescope to J_n = 1)
    g = L.lovasz_gradient(np.zeros(5, bool), 0)  # an absent class: 1 at the first position, 0 after
    assert g.tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]


def test_tie_rule_descending_errors_then_ascending_index():
    E = np.array([[0.5], [0.25], [0.5], [0.0], [0.5], [0.25], [9.0]], np.float32)
    E = np.concatenate([E, 1.0 - E.clip(0, 1)], axis=1)
    t = np.array([0, 1, 1, 0, 0, 1, 255])
    ref = L.from_errors(E, t, "all")
    assert ref["rank"][:, 0].tolist() == [0, 3, 1, 5, 2, 4, -1]
    assert ref["N"].tolist() == [3, 3] and ref["valid"].tolist() == [True] * 6 + [False]
    # class 0 in its order, by hand: pixels 0, 2, 4 (0.5), 1, 5 (0.25), 3 (0)
    fg = (t[[0, 2, 4, 1, 5, 3]] == 0)
    g = L.lovasz_gradient(fg, 3)
    want = float(np.sum(E[[0, 2, 4, 1, 5, 3], 0].astype(np.float64) * g))
    assert ref["loss_c"][0] == want
    assert ref["coef"][0, 0] == -g[0] / 2 and ref["coef"][2, 0] == g[1] / 2 and not ref["coef"][6].any()
    # -0.0 ties with +0.0; nothing valid: zero
    assert L.from_errors(np.array([[-0.0, 0.0], [0.0, 0.0]], np.float32), np.array([0, 1]))["rank"][:, 0].tolist() == [0, 1]
    none = L.from_errors(E, np.full(7, 255), "all")
    assert none["loss"] == 0.0 and not none["coef"].any() and (none["rank"] == -1).all() and none["K"].all()


BAD = [dict(lovasz_weight=float("nan")), dict(lovasz_weight=float("inf")), dict(lovasz_weight=-float("inf")),
       dict(lovasz_weight="much"), dict(lovasz_weight=0.5, lovasz_classes="some"),
       dict(lovasz_weight=0.5, lovasz_classes=None)]


def test_constructor_and_functional_refuse_what_the_definition_has_no_meaning_for():
    from nas_segm_amd import functional as F
    from nas_segm_amd.nn import SegmCrossEntropy

    x, t = torch.zeros(1, 3, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64)  # (refused before any device is asked for)
    for kw in BAD:
        with pytest.raises(ValueError):
            SegmCrossEntropy(**kw)
        with pytest.raises(ValueError):
            F.cross_entropy_select(x, t, **kw)
    with pytest.raises(ValueError):
        F.lovasz_softmax_loss(x, t, classes="some")
    with pytest.raises(ValueError):
        F.lovasz_from_errors(x.permute(0, 2, 3, 1), t, classes="some")
    with pytest.raises(ValueError):
        SegmCrossEntropy(region="lovasz")  # (the term has a keyword of its own)
    with pytest.raises(ValueError):
        SegmCrossEntropy(lovasz_classes="some")
    crit = SegmCrossEntropy(lovasz_weight=0.5)
    crit.lovasz_weight = float("nan")  # (changed between steps: refused at the call)
    with pytest.raises(ValueError):
        crit(x, t)
    crit.lovasz_weight, crit.lovasz_classes = 0.5, "most"
    with pytest.raises(ValueError):
        crit(x, t)
    ok = SegmCrossEntropy(lovasz_weight=0, lovasz_classes="all")
    assert ok.lovasz_weight == 0 and not ok.selects and ok.weight is None and ok.region is None


def test_config_and_repr_without_the_term_are_unchanged_and_with_it_carry_both_values():
    from nas_segm_amd.nn import SegmCrossEntropy

    w = torch.tensor([1.0, 2.0, 0.5])
    crit = SegmCrossEntropy(weight=w, ignore_index=11, thresh=0.7, min_kept=3, keep_fraction=0.25)
    assert crit.config() == ("ce_sel", id(crit.weight), 11, 0.7, 3, 0.25)  # (what the parent commit returns)
    assert crit.extra_repr() == "classes=3, ignore_index=11, thresh=0.7, min_kept=3, keep_fraction=0.25"
    reg = SegmCrossEntropy(region="dice", region_weight=0.5)
    assert reg.config()[6:] == (("region", "dice", 0.5, 1.0, "present"),) and "lovasz" not in reg.extra_repr()
    a = SegmCrossEntropy(lovasz_weight=0.5)
    assert a.config() == SegmCrossEntropy().config() + (("lovasz", 0.5, "present"),)
    assert a.extra_repr() == SegmCrossEntropy().extra_repr() + ", lovasz_weight=0.5, lovasz_classes='present'"
    assert SegmCrossEntropy(lovasz_weight=0.25).config() != a.config()
    assert SegmCrossEntropy(lovasz_weight=0.5, lovasz_classes="all").config() != a.config()
    both = SegmCrossEntropy(region="dice", region_weight=0.5, lovasz_weight=0.5, lovasz_classes="all")
    assert both.config() == reg.config() + (("lovasz", 0.5, "all"),)
    assert both.extra_repr().endswith("region_classes='present', lovasz_weight=0.5, lovasz_classes='all'")
    a.lovasz_weight = 0.75  # (changed between steps: a new key for the stepper caches)
    assert a.config() != SegmCrossEntropy(lovasz_weight=0.5).config()


def test_segm_crit_routes_a_lovasz_only_criterion_as_non_plain():
    from nas_segm_amd.engine.trainer import _ignore_index, _segm_crit
    from nas_segm_amd.nn import SegmCrossEntropy

    assert _segm_crit(SegmCrossEntropy()) is None
    for kw in (dict(lovasz_weight=0.5), dict(lovasz_weight=0.0), dict(lovasz_weight=1, lovasz_classes="all"),
               dict(lovasz_weight=0.5, thresh=0.7, min_kept=3), dict(lovasz_weight=0.5, region="dice")):
        crit = SegmCrossEntropy(**kw)
        assert _segm_crit(crit) is crit
    assert _ignore_index(SegmCrossEntropy(lovasz_weight=0.5, ignore_index=7)) == 7


def test_steps_hand_the_two_keywords_through_only_when_set(monkeypatch):
    """the functional module patched as tests/test_region_loss_host.py patches it"""
    import torch.nn.functional as TF

    from nas_segm_amd import functional as F
    from nas_segm_amd.engine import Segmenter
    from nas_segm_amd.engine.trainer import segmenter_step, train_segmenter
    from nas_segm_amd.nn import SegmCrossEntropy

    calls = []

    def nll(logits, target, ignore_index=255):
        calls.append(("nll", ignore_index))
        return TF.nll_loss(TF.log_softmax(logits, 1), target, ignore_index=ignore_index)

    def ce_sel(logits, target, weight=None, ignore_index=255, thresh=None, min_kept=0, keep_fraction=0.0, **terms):
        calls.append(("sel", ignore_index, thresh, min_kept, keep_fraction, tuple(sorted(terms.items()))))
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

    lov = (("lovasz_classes", "all"), ("lovasz_weight", 0.5))
    reg = (("region", "dice"), ("region_classes", "present"), ("region_smooth", 1.0), ("region_weight", 0.25))
    for through_epoch in (False, True):
        assert run(SegmCrossEntropy(), through_epoch) == [("nll", 255)]
        assert run(SegmCrossEntropy(min_kept=9), through_epoch) == [("sel", 255, None, 9, 0.0, ())]
        crit = SegmCrossEntropy(lovasz_weight=0.5, lovasz_classes="all")
        assert run(crit, through_epoch) == [("sel", 255, None, 0, 0.0, lov)]
        crit = SegmCrossEntropy(region="dice", region_weight=0.25)
        assert run(crit, through_epoch) == [("sel", 255, None, 0, 0.0, reg)]
        crit = SegmCrossEntropy(region="dice", region_weight=0.25, lovasz_weight=0.5, lovasz_classes="all", min_kept=4)
        assert run(crit, through_epoch) == [("sel", 255, None, 4, 0.0, tuple(sorted(lov + reg)))]


def test_evaluate_candidate_hands_the_lovasz_criterion_to_the_epoch(monkeypatch):
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
    crit = SegmCrossEntropy(lovasz_weight=0.5)
    assert search.evaluate_candidate([], [], [], device="cpu", segm_crit=crit) == 0.5
    assert seen[0] is crit and seen[0].lovasz_weight == 0.5
