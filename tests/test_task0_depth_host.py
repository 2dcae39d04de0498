"""CPU-only checks of the decoder-only depth stage: the depth cache's place in the task0 helpers, the refusals of
``train_task0`` / ``populate_task0`` / ``evaluate_candidate``, the stepper cache's key and the ``rows=`` keyword's
argument checks (the kernels themselves: tests/test_hip_task0_depth.py)."""
import pytest
import torch
from torch import nn


def _depth_cache(n=4):
    return {0: torch.zeros(n, 8, 3, 4), 1: torch.zeros(n, 16, 2, 2), "depth": torch.ones(n, 12, 16),
            "out_size": (3, 4)}


def _label_cache(n=4):
    return {0: torch.zeros(n, 8, 3, 4), "y": torch.zeros(n, 3, 4, dtype=torch.int64), "out_size": (3, 4)}


def test_cache_feature_keys_ignores_the_depth_maps():
    from nas_segm_amd.engine.trainer_common import cache_feature_keys

    assert cache_feature_keys(_depth_cache()) == [0, 1]
    assert cache_feature_keys(_label_cache()) == [0]
    both = dict(_depth_cache(), y=torch.zeros(4, 3, 4, dtype=torch.int64), kd_y=torch.zeros(4, 2, 3, 4))
    assert cache_feature_keys(both) == [0, 1]


def test_check_cache_rows_counts_the_rows_of_a_depth_cache():
    from nas_segm_amd.engine.trainer_common import check_cache_rows

    cache = _depth_cache(4)
    assert "y" not in cache
    check_cache_rows(torch.tensor([3, 0, 3]), cache, "t")
    check_cache_rows(torch.zeros(0, dtype=torch.int64), cache, "t")
    for bad in ([4], [-1], [0, 1, 7]):
        with pytest.raises(IndexError, match=r"\[0, 4\)"):
            check_cache_rows(torch.tensor(bad), cache, "t")
    with pytest.raises(IndexError, match=r"\[0, 4\)"):  # (a label cache: as ever)
        check_cache_rows(torch.tensor([4]), _label_cache(4), "t")


def test_train_task0_refusals():
    from nas_segm_amd.engine.trainer import train_task0
    from nas_segm_amd.nn import BerHuLoss, SegmCrossEntropy

    run = train_task0.__wrapped__
    tail = (None, 2, False, False, 0.0, 3.0, False)
    # a depth criterion without a depth cache: an empty cache, a label cache - today's refusal, and how to get one
    for cache in ({}, _label_cache()):
        for crit in (BerHuLoss(), BerHuLoss(0.0, full_size=True)):
            with pytest.raises(ValueError, match="end to end") as e:
                run(cache, None, None, 0, crit, *tail)
            assert 'populate_task0(..., task="depth")' in str(e.value)
    # a depth cache with any other criterion
    for crit in (type("C", (), {"ignore_index": 255})(), SegmCrossEntropy(), nn.NLLLoss(), None):
        with pytest.raises(ValueError, match="BerHuLoss"):
            run(_depth_cache(), None, None, 0, crit, *tail)
    # distillation with a depth cache
    with pytest.raises(ValueError, match="distillation"):
        run(_depth_cache(), None, None, 0, BerHuLoss(), nn.MSELoss(), 2, False, True, 0.5, 3.0, False)


def test_populate_task0_refuses_distillation_for_depth_and_unknown_tasks():
    from nas_segm_amd.engine.trainer import populate_task0

    with pytest.raises(ValueError, match="distillation"):
        populate_task0.__wrapped__(None, [], None, 4, do_kd=True, task="depth")
    with pytest.raises(ValueError, match="task"):
        populate_task0.__wrapped__(None, [], None, 4, task="normals")


def test_the_task0_stepper_key_follows_the_depth_criterions_config(monkeypatch):
    from nas_segm_amd.engine import graphed, trainer
    from nas_segm_amd.nn import BerHuLoss

    built = []

    class Stepper(object):
        def __init__(self, *a, **k):
            built.append((k["depth_crit"].config(), sorted(k)))

        def stale(self):
            return False

    monkeypatch.setattr(graphed, "GraphedTask0Step", Stepper)

    class Net(nn.Module):
        def __init__(self):
            super(Net, self).__init__()
            self.decoder = nn.Sequential(nn.Conv2d(8, 1, 1), nn.BatchNorm2d(1))

    net = Net()
    opt = torch.optim.SGD(net.decoder.parameters(), lr=0.1)
    cache = _depth_cache()
    args = (cache, net, opt, 2, 255, 3.0, 0.15)
    plain, full = BerHuLoss(0.0), BerHuLoss(0.0, full_size=True)
    a = trainer._task0_stepper(*args, depth_crit=plain)
    assert trainer._task0_stepper(*args, depth_crit=plain) is a
    assert built == [(("berhu", 0.0, float("inf")), ["depth_crit", "kd_coeff"])]
    b = trainer._task0_stepper(*args, depth_crit=full)
    assert b is not a and built[1][0] == ("berhu_up", 0.0, float("inf"))
    assert trainer._task0_stepper(*args, depth_crit=full) is b and len(built) == 2
    # the key is the criterion's config(), not its identity alone: the bounds are recorded by value
    full.valid_max = 5.0
    c = trainer._task0_stepper(*args, depth_crit=full)
    assert c is not b and built[2][0] == ("berhu_up", 0.0, 5.0)
    full.full_size = False
    assert trainer._task0_stepper(*args, depth_crit=full) is not c and built[3][0] == ("berhu", 0.0, 5.0)
    # ... and not the config alone: another criterion object of the same config is another step
    net2 = Net()
    opt2 = torch.optim.SGD(net2.decoder.parameters(), lr=0.1)
    del built[:]
    c1, c2 = BerHuLoss(0.0), BerHuLoss(0.0)
    x = trainer._task0_stepper(cache, net2, opt2, 2, 255, 3.0, 0.15, depth_crit=c1)
    y = trainer._task0_stepper(cache, net2, opt2, 2, 255, 3.0, 0.15, depth_crit=c2)
    assert x is not y and len(built) == 2


def test_the_steps_refuse_a_depth_criterion_without_a_depth_cache():
    from nas_segm_amd.engine.graphed import GraphedTask0Step
    from nas_segm_amd.engine.trainer import make_task0_step
    from nas_segm_amd.nn import BerHuLoss

    class Net(nn.Module):
        def __init__(self):
            super(Net, self).__init__()
            self.decoder = nn.Conv2d(8, 1, 1)

    net = Net()
    with pytest.raises(ValueError, match="depth cache"):
        GraphedTask0Step(_label_cache(), net, None, 2, depth_crit=BerHuLoss())
    with pytest.raises(ValueError, match="depth cache"):
        GraphedTask0Step(_depth_cache(), net, None, 2, kd_coeff=0.5, depth_crit=BerHuLoss())
    with pytest.raises(ValueError, match="depth cache"):
        make_task0_step(_depth_cache(), net, None, 2, do_kd=True, depth_crit=BerHuLoss())


def test_rows_checks_its_arguments_and_has_no_cpu_fallback(monkeypatch):
    from nas_segm_amd import functional as F
    from nas_segm_amd.nn import BerHuLoss

    pred, cache = torch.zeros(2, 1, 2, 2), torch.ones(5, 8, 8)
    rows = torch.tensor([4, 0])
    for fn in (F.berhu_loss_masked, F.berhu_loss_upsampled):
        with pytest.raises(F.NassegError, match="HIP device"):  # (valid arguments, host tensors)
            fn(pred, cache, rows=rows)
        for bad in ([5, 0], [0, -1]):  # (a host index can be checked without a synchronisation: it is)
            with pytest.raises(IndexError, match=r"\[0, 5\)"):
                fn(pred, cache, rows=torch.tensor(bad))
        with pytest.raises(F.NassegError, match="rows"):
            fn(pred, cache, rows=rows.to(torch.int32))
        with pytest.raises(F.NassegError, match="rows"):
            fn(pred, cache, rows=torch.tensor([[4, 0]]))
        with pytest.raises(F.NassegError, match="one cache row per image"):
            fn(pred, cache, rows=torch.tensor([4, 0, 1]))
        with pytest.raises(F.NassegError, match="fp32 cache"):
            fn(pred, cache.double(), rows=rows)
        with pytest.raises(F.NassegError, match="fp32 cache"):
            fn(pred, cache[0], rows=rows)
    # the criterion hands ``rows`` through, and only when it is given (the plain call keeps its four arguments)
    calls = []
    monkeypatch.setattr(F, "berhu_loss_masked", lambda *a, **k: calls.append(("masked", a[2:], k)) or "M")
    monkeypatch.setattr(F, "berhu_loss_upsampled", lambda *a, **k: calls.append(("up", a[2:], k)) or "U")
    plain, full = BerHuLoss(0.0, 5.0), BerHuLoss(0.0, 5.0, full_size=True)
    assert plain(pred, cache, rows=rows) == "M" and full(pred, cache, rows) == "U" and plain(pred, cache) == "M"
    assert calls == [("masked", (0.0, 5.0), {"rows": rows}), ("up", (0.0, 5.0), {"rows": rows}),
                     ("masked", (0.0, 5.0), {})]
    assert plain.config() == ("berhu", 0.0, 5.0) and full.config() == ("berhu_up", 0.0, 5.0)


def test_evaluate_candidate_checks_task0_epochs_before_anything_is_built(monkeypatch):
    from nas_segm_amd.engine import search

    seen = []

    def no_build(*a, **k):
        seen.append(k.get("task", "segm"))
        raise RuntimeError("stop here")

    monkeypatch.setattr(search, "build_candidate", no_build)
    for task in ("depth", "segm"):
        for bad in (-1, -3, 1.5, "2", None, True):
            with pytest.raises(ValueError, match="task0_epochs"):
                search.evaluate_candidate([], [], [], task=task, task0_epochs=bad)
    assert seen == []
    assert search.evaluate_candidate([], [], [], task="depth", task0_epochs=2) == 0.0
    assert search.evaluate_candidate([], [], [], task="segm", task0_epochs=0) == 0.0
    assert seen == ["depth", "segm"]


def test_evaluate_candidate_runs_the_decoder_only_stage_first(monkeypatch):
    from nas_segm_amd.engine import search
    from nas_segm_amd.nn import BerHuLoss

    class Net(nn.Module):
        def __init__(self):
            super(Net, self).__init__()
            self.encoder, self.decoder = nn.Conv2d(3, 1, 1), nn.Conv2d(1, 1, 1)

    class Wrapped(object):
        module = Net()

        def train(self):
            log.append(("train-mode",))

    log = []
    monkeypatch.setattr(search, "build_candidate", lambda *a, **k: Wrapped())
    monkeypatch.setattr(search, "populate_task0",
                        lambda seg, tb, kd, n, **k: log.append(("populate", n, k)) or {"depth": None})
    monkeypatch.setattr(search, "train_task0", lambda Xy, seg, od, ep, crit, kd, bs, *a, **k: log.append(
        ("task0", ep, crit, bs, a, k)))
    monkeypatch.setattr(search, "train_segmenter", lambda seg, tb, oe, od, ep, crit, *a, **k: log.append(("task1", ep)))
    monkeypatch.setattr(search, "validate_depth", lambda *a, **k: 0.5)
    monkeypatch.setattr(search, "validate", lambda *a, **k: 0.25)
    batches = [{"image": torch.zeros(3, 3, 4, 4), "mask": torch.ones(3, 4, 4)}] * 2
    crit = BerHuLoss(0.0, full_size=True)
    kw = dict(device="cpu", ctrl_version="cvpr", aux_weight=0.15)
    assert search.evaluate_candidate([], batches, batches, task="depth", depth_crit=crit, task0_epochs=2, epochs=1,
                                     **kw) == 0.5
    assert [e[0] for e in log] == ["populate", "task0", "task0", "train-mode", "task1"]
    assert log[0][1:] == (6, {"task": "depth"})  # (every sample of the batches)
    assert [e[1] for e in log[1:3]] == [0, 1] and all(e[2] is crit and e[3] == 3 for e in log[1:3])
    assert log[1][4] == (False, False, 0.0, 3.0, False) and log[1][5] == {"aux_weight": 0.15}
    del log[:]
    assert search.evaluate_candidate([], batches, batches, task="depth", depth_crit=crit, epochs=1, **kw) == 0.5
    assert [e[0] for e in log] == ["task1"]  # (0: no such stage)
    del log[:]
    assert search.evaluate_candidate([], batches, batches, task="segm", task0_epochs=1, epochs=1, **kw) == 0.25
    assert [e[0] for e in log] == ["populate", "task0", "train-mode", "task1"] and log[0][2] == {"task": "segm"}
    # a failure inside the stage (try_except: 0) scores the candidate 0
    monkeypatch.setattr(search, "train_task0", lambda *a, **k: 0)
    assert search.evaluate_candidate([], batches, batches, task="depth", task0_epochs=1, epochs=1, **kw) == 0.0
    monkeypatch.setattr(search, "populate_task0", lambda *a, **k: 0)
    assert search.evaluate_candidate([], batches, batches, task="depth", task0_epochs=1, epochs=1, **kw) == 0.0
