"""CPU-only checks of the class-weighted / hard-example-mined cross-entropy: the float64 restatement
(tests/_segm_loss_ref.py) against torch and against its own definition, the criterion's argument checks, and which
criteria the engine hands to the new kernels (everything else keeps calling F.log_softmax_nll)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF
from torch import nn

import _segm_loss_ref as R


def _inputs(P, C, seed, ignored=0.2):
    rng = np.random.RandomState(seed)
    x = rng.randn(P, C) * 3.0
    t = rng.randint(0, C, size=P)
    t[rng.rand(P) < ignored] = 255
    return x, t, rng.rand(C) + 0.5


def test_restatement_with_weights_equals_torch_cross_entropy():
    for P, C, seed in ((442, 19, 0), (97, 21, 1), (64, 64, 2)):
        x, t, w = _inputs(P, C, seed)
        xt = torch.from_numpy(x).requires_grad_(True)
        for weight in (None, w):
            ref = R.cross_entropy_select(x, t, weight)
            want = TF.cross_entropy(xt, torch.from_numpy(t), ignore_index=255,
                                    weight=None if weight is None else torch.from_numpy(weight))
            (grad,) = torch.autograd.grad(want, xt)
            assert abs(ref["loss"] - want.item()) <= 1e-12 * abs(want.item())
            assert np.abs(ref["grad"] - grad.numpy()).max() <= 1e-12
            assert ref["n_kept"] == ref["n"] == int((t != 255).sum()) and ref["tau"] == -np.inf


def test_restatement_all_ignored_is_nan():
    x, t, w = _inputs(16, 5, 3)
    ref = R.cross_entropy_select(x, np.full(16, 255), w)
    assert np.isnan(ref["loss"]) and ref["n"] == 0


def test_min_kept_beyond_the_valid_pixels_is_the_plain_mean():
    x, t, w = _inputs(300, 19, 4)
    plain = R.cross_entropy_select(x, t, w)
    sel = R.cross_entropy_select(x, t, w, min_kept=10 ** 6)
    assert sel["k"] == sel["n"] == sel["n_kept"] == plain["n"]
    assert sel["loss"] == plain["loss"] and np.array_equal(sel["grad"], plain["grad"])
    assert sel["tau"] == plain["pixel_loss"][plain["pixel_loss"] >= 0].min()


def test_every_pixel_tied_at_tau_is_kept():
    # logits of two kinds only: the losses take two values, and k falls in the middle of the lower one's ties
    C, P = 7, 200
    x = np.zeros((P, C))
    t = np.zeros(P, np.int64)
    x[:60, 1] = 4.0   # 60 hard pixels (the target is not the largest score)
    t[190:] = 255     # 10 ignored
    ref = R.cross_entropy_select(x, t, None, min_kept=100)
    lo = np.log(float(C))
    assert ref["k"] == 100 and ref["n"] == 190
    assert abs(ref["tau"] - lo) < 1e-12 and ref["n_kept"] == 190  # all 130 ties kept, not 40 of them
    ref = R.cross_entropy_select(x, t, None, min_kept=60)
    assert ref["n_kept"] == 60 and ref["tau"] > lo
    ref = R.cross_entropy_select(x, t, None, thresh=0.5, min_kept=1)  # -log(0.5) lies between the two values
    assert ref["n_kept"] == 190 and ref["tau"] == np.float64(np.float32(-np.log(0.5)))
    tau, k, n, kept = R.threshold(np.array([2.0, -1.0, 2.0, 1.0, 2.0], np.float32), np.inf, 2, 0.0)
    assert (tau, k, n, kept) == (np.float32(2.0), 2, 4, 3)
    assert R.select_k(10, 1, 0.25) == 3 and R.select_k(10, 5, 0.25) == 5 and R.select_k(3, 5, 1.0) == 3


def test_constructor_refuses_what_the_definition_has_no_meaning_for():
    from nas_segm_amd.nn import SegmCrossEntropy

    for kw in (dict(thresh=0.7), dict(keep_fraction=0.25), dict(thresh=0.7, min_kept=0),  # selection, min_kept < 1
               dict(thresh=0.0, min_kept=1), dict(thresh=1.0, min_kept=1), dict(thresh=-0.1, min_kept=1),
               dict(keep_fraction=-0.1, min_kept=1), dict(keep_fraction=1.5, min_kept=1), dict(min_kept=-1),
               dict(weight=torch.ones(3, 2)), dict(weight=torch.tensor(1.0))):
        with pytest.raises(ValueError):
            SegmCrossEntropy(**kw)
    crit = SegmCrossEntropy(weight=[1.0, 2.0, 3.0], thresh=0.7, min_kept=5, keep_fraction=0.1, ignore_index=250)
    assert "weight" in dict(crit.named_buffers()) and crit.ignore_index == 250 and crit.selects
    assert not SegmCrossEntropy().selects and SegmCrossEntropy().weight is None
    assert SegmCrossEntropy(keep_fraction=1.0, min_kept=1).selects


def test_segm_crit_dispatch():
    from nas_segm_amd.engine.trainer import _ignore_index, _segm_crit
    from nas_segm_amd.nn import BerHuLoss, SegmCrossEntropy

    class Crit(object):
        ignore_index = 255

    w = torch.tensor([1.0, 2.0, 0.5], dtype=torch.float64)
    for plain in (nn.NLLLoss(ignore_index=255), SegmCrossEntropy(), SegmCrossEntropy(ignore_index=7), Crit(), None,
                  BerHuLoss(), nn.NLLLoss(weight=w, reduction="sum"), nn.CrossEntropyLoss(weight=w)):
        assert _segm_crit(plain) is None
    assert _ignore_index(SegmCrossEntropy(ignore_index=7)) == 7
    for own in (SegmCrossEntropy(weight=w), SegmCrossEntropy(min_kept=3), SegmCrossEntropy(thresh=0.7, min_kept=3)):
        assert _segm_crit(own) is own
    given = nn.NLLLoss(weight=w, ignore_index=11)
    mapped = _segm_crit(given, "cpu")
    assert isinstance(mapped, SegmCrossEntropy) and not mapped.selects and mapped.ignore_index == 11
    assert mapped.weight.dtype == torch.float32 and torch.equal(mapped.weight, w.float())  # (prepared: fp32)
    assert _segm_crit(given, "cpu") is mapped and mapped.config() == _segm_crit(given).config()  # one per criterion
    given.weight = w * 2
    assert _segm_crit(given) is not mapped
    if hasattr(nn, "NLLLoss2d"):
        assert isinstance(_segm_crit(nn.NLLLoss2d(weight=w, ignore_index=255)), SegmCrossEntropy)
    a, b = SegmCrossEntropy(thresh=0.7, min_kept=3), SegmCrossEntropy(thresh=0.7, min_kept=3)
    assert a.config() == b.config()
    b.min_kept = 4
    assert a.config() != b.config()


def test_steps_call_the_plain_loss_for_plain_criteria_and_the_criterion_otherwise(monkeypatch):
    """the functional module patched as tests/test_distributed_cpu.py patches it: a plain criterion still reaches
    F.log_softmax_nll by name, a weighted one reaches F.cross_entropy_select"""
    from nas_segm_amd import functional as F
    from nas_segm_amd.engine import Segmenter
    from nas_segm_amd.engine.trainer import segmenter_step, train_segmenter
    from nas_segm_amd.nn import SegmCrossEntropy

    calls = []

    def nll(logits, target, ignore_index=255):
        calls.append(("nll", ignore_index))
        return TF.nll_loss(TF.log_softmax(logits, 1), target, ignore_index=ignore_index)

    def ce_sel(logits, target, weight=None, ignore_index=255, thresh=None, min_kept=0, keep_fraction=0.0):
        calls.append(("sel", ignore_index, thresh, min_kept, keep_fraction))
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
        batch["mask"][:, :2] = 255
        del calls[:]
        if through_epoch:
            assert train_segmenter.__wrapped__(net, [batch], oe, od, 0, crit, False, 3.0, 3.0, False) is None
        else:
            segmenter_step(net, batch["image"], batch["mask"], oe, od, 255, 3.0, 3.0, segm_crit=crit)
        return list(calls), torch.cat([p.detach().reshape(-1) for p in net.parameters()])

    w = torch.tensor([1.0, 3.0, 0.25, 2.0, 1.5])
    for through_epoch in (False, True):
        c_plain, p_plain = run(nn.NLLLoss(ignore_index=255), through_epoch)
        c_none, p_none = run(SegmCrossEntropy(), through_epoch)
        assert c_plain == [("nll", 255)] and c_none == [("nll", 255)] and torch.equal(p_plain, p_none)
        c_w, p_w = run(nn.NLLLoss(weight=w, ignore_index=255), through_epoch)
        c_own, p_own = run(SegmCrossEntropy(weight=w), through_epoch)
        assert c_w == [("sel", 255, None, 0, 0.0)] and c_own == c_w
        assert torch.equal(p_w, p_own) and not torch.equal(p_w, p_plain)  # (the weights are honoured)
        c_sel, _ = run(SegmCrossEntropy(thresh=0.7, min_kept=9, keep_fraction=0.5), through_epoch)
        assert c_sel == [("sel", 255, 0.7, 9, 0.5)]


def test_evaluate_candidate_hands_the_criterion_to_the_epoch(monkeypatch):
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
    crit = SegmCrossEntropy(thresh=0.7, min_kept=10)
    assert search.evaluate_candidate([], [], [], device="cpu", segm_crit=crit) == 0.5
    assert search.evaluate_candidate([], [], [], device="cpu") == 0.5
    assert seen[0] is crit and seen[1].ignore_index == 255 and not isinstance(seen[1], nn.Module)
