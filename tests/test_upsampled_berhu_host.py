"""CPU-only checks of the full-size berHu: the fp32 restatement (tests/_upsampled_berhu_ref.py) against the float64
one within the GPU test's tolerances - which pins those tolerances without a GPU - and the option's way through the
criterion module, ``evaluate_candidate`` and the stepper cache."""
import pytest
import torch
from torch import nn

import _upsampled_berhu_ref as U


def _within_gpu_tolerances(a, b, what):
    """``a`` (fp32) against ``b`` (float64) by the GPU test's rule; returns the shares of the two tolerances used"""
    loss_share = abs(a["loss"] - b["loss"]) / (U.LOSS_RTOL * max(1.0, abs(b["loss"])))
    err = (a["grad"].double() - b["grad"]).abs()
    grad_share = float((err / (U.GRAD_ATOL + U.GRAD_RTOL * b["grad"].abs())).max())
    print(what, "valid", int(b["valid"].sum()), "gap", b["gap"], "loss share", loss_share, "grad share", grad_share)
    assert loss_share <= 1.0 and grad_share <= 1.0, (what, loss_share, grad_share)
    return loss_share, grad_share


@pytest.mark.parametrize("case", U.CASES, ids=str)
def test_fp32_restatement_stays_within_the_gpu_tolerances_of_float64(case):
    for kw in (dict(), dict(valid_max=5.0), dict(bf16=True)):
        a, b = U.reference(case, **kw), U.reference(case, dtype=torch.float64, **kw)
        assert torch.equal(a["valid"], b["valid"]) and 0 < int(b["valid"].sum()) < b["valid"].numel()
        # the condition of the fp32 comparisons: no valid pixel sits where rounding could turn sign(v - t); on the
        # bf16-rounded prediction (compared to one bf16 ulp) the two precisions at least agree on every sign
        if not kw.get("bf16"):
            assert b["gap"] >= U.MIN_GAP and a["gap"] >= U.MIN_GAP, (case, kw, a["gap"], b["gap"])
        gt, valid = a["gt"], a["valid"]
        assert torch.equal(torch.sign(a["v"][valid] - gt[valid]).double(), torch.sign(b["v"][valid] - gt.double()[valid]))
        _within_gpu_tolerances(a, b, (case, kw))
    full, tight = U.reference(case), U.reference(case, valid_max=5.0)
    assert int(tight["valid"].sum()) < int(full["valid"].sum())


@pytest.mark.parametrize("case", U.SPARSE_CASES, ids=str)
def test_sparse_targets_leave_the_stated_pixels_and_stay_within_the_tolerances(case):
    a, b = U.reference(case, sparse=True), U.reference(case, sparse=True, dtype=torch.float64)
    assert int(b["valid"].sum()) == U.SPARSE_VALID[case]
    assert b["gap"] >= U.MIN_GAP
    _within_gpu_tolerances(a, b, (case, "sparse"))
    # prediction pixels no valid target pixel reaches: exact zeros, the same ones in both precisions
    assert torch.equal(a["grad"] == 0, b["grad"] == 0)
    if case == (3, 17, 23, 101, 75):
        assert bool((b["grad"] == 0).any()) and bool((b["grad"] != 0).any())


def test_equal_sizes_are_the_masked_loss_at_the_predictions_size():
    pred, gt = U.make_inputs(2, 6, 5, 6, 5)
    ref = U.reference((2, 6, 5, 6, 5), dtype=torch.float64)
    assert torch.equal(ref["v"], pred[:, 0].double())  # (interpolation to the same size is the identity)
    valid = ref["valid"]
    d = (pred[:, 0].double() - gt.double())[valid].abs()
    c = 0.2 * d.max()
    want = torch.where(d <= c, d, (d * d + c * c) / (2 * c)).mean()
    assert abs(ref["loss"] - float(want)) <= 1e-12 and float(ref["grad"][:, 0][~valid].abs().max()) == 0.0


def test_full_size_option_of_the_criterion(monkeypatch):
    from nas_segm_amd import functional as F
    from nas_segm_amd.nn import BerHuLoss

    plain, full = BerHuLoss(valid_min=0.0, valid_max=5.0), BerHuLoss(valid_min=0.0, valid_max=5.0, full_size=True)
    assert plain.full_size is False and full.full_size is True and BerHuLoss().full_size is False
    assert plain.config() == ("berhu", 0.0, 5.0) and full.config() == ("berhu_up", 0.0, 5.0)
    assert BerHuLoss(full_size=True).config() == ("berhu_up", 0.0, float("inf"))
    assert plain.extra_repr() == "valid_min=0.0, valid_max=5.0"  # (as it was before the option existed)
    assert full.extra_repr() == plain.extra_repr() + ", full_size=True"
    assert "full_size=True" in repr(full) and "full_size" not in repr(plain)
    calls = []
    monkeypatch.setattr(F, "berhu_loss_upsampled", lambda *a: calls.append(("up",) + a[2:]) or "U")
    monkeypatch.setattr(F, "berhu_loss_masked", lambda *a: calls.append(("masked",) + a[2:]) or "M")
    pred, gt = torch.zeros(1, 1, 2, 2), torch.ones(1, 8, 8)
    assert full(pred, gt) == "U" and plain(pred, gt) == "M" and BerHuLoss(1.5)(pred, gt) == "M"
    assert calls == [("up", 0.0, 5.0), ("masked", 0.0, 5.0), ("masked", 1.5, float("inf"))]


def test_the_function_checks_its_arguments_and_has_no_cpu_fallback():
    from nas_segm_amd import functional as F

    with pytest.raises(F.NassegError):  # (valid arguments, host tensors)
        F.berhu_loss_upsampled(torch.zeros(1, 1, 2, 2), torch.ones(1, 8, 8))


def test_evaluate_candidate_checks_depth_crit_before_anything_is_built(monkeypatch):
    from nas_segm_amd.engine import search
    from nas_segm_amd.nn import BerHuLoss, SegmCrossEntropy

    seen = []

    def no_build(*a, **k):
        seen.append(k.get("task", "segm"))
        raise RuntimeError("stop here")  # (scored 0, as every candidate that cannot be built)

    monkeypatch.setattr(search, "build_candidate", no_build)
    for bad in (SegmCrossEntropy(), nn.L1Loss(), "berhu", lambda p, t: p.sum()):
        for task in ("depth", "segm"):
            with pytest.raises(ValueError, match="depth_crit"):
                search.evaluate_candidate([], [], [], task=task, depth_crit=bad)
    with pytest.raises(ValueError, match="depth_crit"):  # (a depth criterion is no segmentation criterion)
        search.evaluate_candidate([], [], [], task="segm", depth_crit=BerHuLoss(full_size=True))
    assert seen == []
    assert search.evaluate_candidate([], [], [], task="depth", depth_crit=BerHuLoss(0.0, full_size=True)) == 0.0
    assert search.evaluate_candidate([], [], [], task="depth") == 0.0  # (the default stays)
    assert seen == ["depth", "depth"]


def test_evaluate_depth_candidate_hands_the_criterion_to_both_paths(monkeypatch):
    from nas_segm_amd.engine import search
    from nas_segm_amd.nn import BerHuLoss

    class Net(nn.Module):
        def __init__(self):
            super(Net, self).__init__()
            self.encoder, self.decoder = nn.Conv2d(3, 1, 1), nn.Conv2d(1, 1, 1)

    class Wrapped(object):
        module = Net()

    got = []
    monkeypatch.setattr(search, "build_candidate", lambda *a, **k: Wrapped())
    monkeypatch.setattr(search, "train_segmenter", lambda seg, tb, oe, od, ep, crit, *a, **k: got.append(("eager", crit)))

    class Stepper(object):
        def __init__(self, *a, **k):
            got.append(("graphed", k["depth_crit"]))

        def step(self, image, depth):
            pass

    monkeypatch.setattr(search, "GraphedSegmenterStep", Stepper)
    monkeypatch.setattr(search, "validate_depth", lambda *a, **k: 0.5)
    batches = [{"image": torch.zeros(1, 3, 4, 4), "mask": torch.ones(1, 4, 4)}]
    crit = BerHuLoss(0.0, full_size=True)
    for graphed in (False, True):
        assert search.evaluate_candidate([], batches, batches, device="cpu", task="depth", graphed=graphed,
                                         depth_crit=crit) == 0.5
        assert search.evaluate_candidate([], batches, batches, device="cpu", task="depth", graphed=graphed) == 0.5
    assert [k for k, _ in got] == ["eager", "eager", "graphed", "graphed"]
    assert got[0][1] is crit and got[2][1] is crit
    for _, default in (got[1], got[3]):
        assert isinstance(default, BerHuLoss) and default.config() == ("berhu", 0.0, float("inf"))


def test_the_stepper_cache_never_replays_one_kind_of_depth_step_for_the_other(monkeypatch):
    from nas_segm_amd.engine import graphed, trainer
    from nas_segm_amd.nn import BerHuLoss

    built = []

    class Stepper(object):
        def __init__(self, *a, **k):
            built.append(k["depth_crit"].config())

        def stale(self):
            return False

    monkeypatch.setattr(graphed, "GraphedSegmenterStep", Stepper)
    net = nn.Sequential(nn.Conv2d(3, 1, 1), nn.BatchNorm2d(1))
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    image, target = torch.zeros(2, 3, 8, 8), torch.ones(2, 8, 8)
    args = (net, image, target, opt, opt, 255, 3.0, 3.0, 0.15)
    full, plain = BerHuLoss(0.0, full_size=True), BerHuLoss(0.0)
    a = trainer._segmenter_stepper(*args, depth_crit=full)
    assert trainer._segmenter_stepper(*args, depth_crit=full) is a and built == [("berhu_up", 0.0, float("inf"))]
    b = trainer._segmenter_stepper(*args, depth_crit=plain)
    assert b is not a and built[1:] == [("berhu", 0.0, float("inf"))]
    assert trainer._segmenter_stepper(*args, depth_crit=plain) is b and len(built) == 2
    # the key is the criterion's config(), not its identity alone: the same object switched over is another step
    plain.full_size = True
    c = trainer._segmenter_stepper(*args, depth_crit=plain)
    assert c is not b and built[2:] == [("berhu_up", 0.0, float("inf"))]
    plain.valid_max = 5.0
    assert trainer._segmenter_stepper(*args, depth_crit=plain) is not c and built[3:] == [("berhu_up", 0.0, 5.0)]


def test_train_task0_keeps_refusing_a_depth_criterion():
    from nas_segm_amd.engine.trainer import train_task0
    from nas_segm_amd.nn import BerHuLoss

    with pytest.raises(ValueError, match="end to end"):
        train_task0.__wrapped__({}, None, None, 0, BerHuLoss(full_size=True), None, 2, False, False, 0.0, 0.0, False)
