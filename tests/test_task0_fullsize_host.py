"""The decoder-only (task0) stage on full-size labels, the part that needs no GPU: the refusals and their messages,
the argument checks of ``F.cross_entropy_upsampled(rows=)`` (made before anything is launched, in the order of
``_depth_inputs``), ``cache_feature_keys`` and what ``task0_loss`` hands a full-size criterion."""
import pytest
import torch
import torch.nn.functional as TF
from torch import nn


def full_crit(**kw):
    from nas_segm_amd.nn import SegmCrossEntropy

    return SegmCrossEntropy(full_size=True, **kw)


def test_a_cache_without_full_size_labels_is_refused_before_anything_else():
    from nas_segm_amd.engine.graphed import GraphedTask0Step
    from nas_segm_amd.engine.trainer import make_task0_step, train_task0

    full = full_crit()
    # (nothing else of the arguments is touched: they are all None)
    calls = {
        "train_task0": lambda cache: train_task0.__wrapped__(cache, None, None, 0, full, None, 2, False, False, 0.0,
                                                             0.0, False),
        "make_task0_step": lambda cache: make_task0_step(cache, None, None, 2, segm_crit=full),
        "GraphedTask0Step": lambda cache: GraphedTask0Step(cache, None, None, 2, segm_crit=full),
    }
    for name, call in calls.items():
        for cache in ({}, {0: None, "y": None, "out_size": (4, 4)}):
            with pytest.raises(ValueError) as e:
                call(cache)
            text = str(e.value)
            assert text.startswith(name + ":") and "full-size" in text, text
            assert "populate_task0(..., full_size_labels=True)" in text, text
    # a cache that has them passes the check (and fails later, on the None it was given for a model)
    for call in calls.values():
        with pytest.raises(Exception) as e:
            call({0: None, "y": torch.zeros(1, 2, 2, dtype=torch.int64), "y_full": None, "out_size": (2, 2)})
        assert "full-size" not in str(e.value)


def test_full_size_labels_belong_to_the_segmentation_cache():
    from nas_segm_amd.engine.trainer import populate_task0

    with pytest.raises(ValueError, match="populate_task0: full_size_labels"):
        populate_task0.__wrapped__(None, None, None, 1, task="depth", full_size_labels=True)
    with pytest.raises(ValueError, match="task must be"):  # (as ever, and first)
        populate_task0.__wrapped__(None, None, None, 1, task="flow", full_size_labels=True)
    import inspect

    names = list(inspect.signature(populate_task0.__wrapped__).parameters)
    assert names[-2:] == ["task", "full_size_labels"]  # (at the end: callers pass the others by position)
    assert inspect.signature(populate_task0.__wrapped__).parameters["full_size_labels"].default is False


def test_rows_need_a_full_size_criterion(monkeypatch):
    from nas_segm_amd import functional as F
    from nas_segm_amd.nn import SegmCrossEntropy

    calls = []
    monkeypatch.setattr(F, "cross_entropy_upsampled", lambda *a, **k: calls.append(("up", a[2:], k)) or "U")
    monkeypatch.setattr(F, "cross_entropy_select", lambda *a, **k: calls.append(("sel", a[2:], k)) or "S")
    x, cache = torch.zeros(2, 3, 2, 2), torch.zeros(5, 8, 8, dtype=torch.uint8)
    rows = torch.tensor([4, 1])
    for kw in (dict(), dict(thresh=0.7, min_kept=5), dict(region="dice")):
        with pytest.raises(ValueError, match="SegmCrossEntropy: rows="):
            SegmCrossEntropy(**kw)(x, cache, rows=rows)
    assert calls == []
    assert SegmCrossEntropy(full_size=True, thresh=0.7, min_kept=5, ignore_index=9)(x, cache, rows=rows) == "U"
    assert SegmCrossEntropy(full_size=True, thresh=0.7, min_kept=5, ignore_index=9)(x, cache, rows=None) == "U"
    assert calls == [("up", (None, 9, 0.7, 5, 0.0), {"rows": rows}), ("up", (None, 9, 0.7, 5, 0.0), {})]


def test_the_argument_checks_of_rows():
    from nas_segm_amd import functional as F

    x = torch.zeros(2, 3, 2, 2)
    cache = torch.zeros(5, 8, 8, dtype=torch.uint8)
    rows = torch.tensor([4, 1])

    def refused(match, x=x, cache=cache, rows=rows, error=F.NassegError, named=True, **kw):
        with pytest.raises(error, match=match) as e:
            F.cross_entropy_upsampled(x, cache, rows=rows, **kw)
        assert not named or "cross_entropy_upsampled" in str(e.value)

    refused("rows must be a contiguous 1-D int64 tensor", rows=rows.to(torch.int32))
    refused("rows must be a contiguous 1-D int64 tensor", rows=rows.view(1, 2))
    refused("rows must be a contiguous 1-D int64 tensor", rows=torch.tensor([4, 0, 1])[::2])
    refused("rows must be a contiguous 1-D int64 tensor", rows=[4, 1])
    refused("uint8 or int64 cache of shape \\(N, H, W\\)", cache=cache.float())
    refused("uint8 or int64 cache of shape \\(N, H, W\\)", cache=cache[0])
    refused("uint8 or int64 cache of shape \\(N, H, W\\)", cache=cache[:0])
    refused("one cache row per image", rows=rows[:1])
    refused("one cache row per image", rows=torch.tensor([4, 1, 0]))
    # a host index is checked against [0, N) BEFORE the host tensors are refused for being on the host
    refused("out of range \\[0, 5\\)", rows=torch.tensor([5, 0]), error=IndexError)
    refused("out of range \\[0, 5\\)", rows=torch.tensor([0, -1]), error=IndexError)
    refused("out of range \\[0, 5\\)", rows=torch.tensor([5, 0]), cache=cache.long(), error=IndexError)
    refused("HIP device", named=False)  # (valid arguments, host tensors: there is no CPU fallback)
    refused("HIP device", cache=cache.long(), named=False)
    # the selection triple is refused first, as without rows
    refused("min_kept", error=ValueError, thresh=0.7)
    # without rows nothing changed: the target must be the batch's
    with pytest.raises(F.NassegError, match="HIP device"):
        F.cross_entropy_upsampled(x, cache[:2])


def test_cache_feature_keys_skip_the_full_size_labels():
    from nas_segm_amd.engine.trainer_common import cache_feature_keys

    cache = {0: 0, 1: 1, "y": 2, "y_full": 3, "kd_y": 4, "out_size": (1, 1)}
    assert cache_feature_keys(cache) == [0, 1]
    del cache["y_full"]
    assert cache_feature_keys(cache) == [0, 1]
    assert cache_feature_keys({0: 0, "depth": 1, "out_size": (1, 1)}) == [0]


class Crit(nn.Module):
    """records what it is handed"""

    def __init__(self, full_size):
        super(Crit, self).__init__()
        self.full_size = full_size
        self.seen = []

    def forward(self, logits, target, rows=None):
        self.seen.append((tuple(logits.shape), target.data_ptr(), tuple(target.shape),
                          None if rows is None else rows.data_ptr()))
        return logits.sum() * 0.0 + float(len(self.seen))


def test_task0_loss_hands_a_full_size_criterion_the_cache_the_index_and_every_head_at_its_own_size(monkeypatch):
    from nas_segm_amd import functional as F
    from nas_segm_amd.engine.trainer_common import task0_loss

    events = []
    monkeypatch.setattr(F, "gather_rows", lambda src, idx, out=None: events.append(("gather", src.data_ptr())) or
                        src[idx])
    monkeypatch.setattr(F, "bilinear_resize", lambda x, size: events.append(("resize", tuple(size))) or
                        TF.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False))
    main, aux = torch.zeros(2, 5, 4, 6), [torch.zeros(2, 5, 2, 3), torch.zeros(2, 5, 1, 2)]
    cache = {0: torch.zeros(7, 3, 4, 6), 1: torch.zeros(7, 3, 2, 3), "y": torch.zeros(7, 4, 6, dtype=torch.int64),
             "y_full": torch.zeros(7, 16, 24, dtype=torch.uint8), "kd_y": torch.ones(7, 5, 4, 6), "out_size": (4, 6)}
    index = torch.tensor([6, 2])
    fed = []

    def decoder(feats):
        fed.append([tuple(f.shape) for f in feats])
        return main, aux

    y_full, idx = cache["y_full"], index.data_ptr()
    full = Crit(True)
    loss = task0_loss(cache, index, decoder, 255, 0.5, segm_crit=full)
    assert fed == [[(2, 3, 4, 6), (2, 3, 2, 3)]]
    assert events == [("gather", cache[0].data_ptr()), ("gather", cache[1].data_ptr())]  # (features only; no resize)
    assert full.seen == [((2, 5, 4, 6), y_full.data_ptr(), (7, 16, 24), idx),
                         ((2, 5, 2, 3), y_full.data_ptr(), (7, 16, 24), idx),
                         ((2, 5, 1, 2), y_full.data_ptr(), (7, 16, 24), idx)]
    assert float(loss) == 1.0 + 0.5 * 2.0 + 0.5 * 3.0
    full = Crit(True)
    task0_loss(cache, index, decoder, 255, 0, segm_crit=full)  # (no auxiliary term without a weight)
    assert len(full.seen) == 1

    # distillation: kd_coeff * kd_crit(the main head resized to out_size, the teacher's rows), from the host
    del events[:]
    full, kd_seen = Crit(True), []

    def kd_crit(out, teacher):
        kd_seen.append((tuple(out.shape), tuple(teacher.shape)))
        return ((out - teacher) ** 2).mean()

    monkeypatch.setattr(F, "log_softmax_nll_mse", lambda *a, **k: pytest.fail("the fused CE + MSE does not apply"))
    loss = task0_loss(cache, index, decoder, 255, 0.5, 0.25, kd_crit, segm_crit=full)
    assert events[2:] == [("gather", cache["kd_y"].data_ptr()), ("resize", (4, 6))] and len(events) == 4
    assert kd_seen == [((2, 5, 4, 6), (2, 5, 4, 6))] and len(full.seen) == 3
    assert float(loss) == 1.0 + 0.25 * 1.0 + 0.5 * 2.0 + 0.5 * 3.0

    # any other criterion: the step as it was - labels gathered at the logits' size, heads resized
    del events[:]
    normal = Crit(False)
    task0_loss(cache, index, decoder, 255, 0.5, segm_crit=normal)
    assert ("gather", cache["y"].data_ptr()) in events and ("gather", y_full.data_ptr()) not in events
    assert [e for e in events if e[0] == "resize"] == [("resize", (4, 6))] * 3
    assert [s[0] for s in normal.seen] == [(2, 5, 4, 6)] * 3 and all(s[2] == (2, 4, 6) and s[3] is None
                                                                    for s in normal.seen)


def test_the_task0_stage_asks_for_full_size_labels_only_for_a_full_size_criterion(monkeypatch):
    from nas_segm_amd.engine import search

    asked = []
    monkeypatch.setattr(search, "populate_task0", lambda *a, **k: asked.append(k) or 0)  # (0: try_except's failure)
    batches = [{"image": torch.zeros(2, 3, 8, 8)}]

    class Net(object):
        def train(self):
            pass

    assert search._task0_stage(Net(), batches, None, full_crit(), 1, -1, "segm") is False
    assert search._task0_stage(Net(), batches, None, search._Crit(), 1, -1, "segm") is False
    from nas_segm_amd.nn import BerHuLoss, SegmCrossEntropy

    assert search._task0_stage(Net(), batches, None, SegmCrossEntropy(thresh=0.7, min_kept=5), 1, -1, "segm") is False
    assert search._task0_stage(Net(), batches, None, BerHuLoss(0.0, full_size=True), 1, -1, "depth") is False
    assert asked == [{"task": "segm", "full_size_labels": True}, {"task": "segm"}, {"task": "segm"},
                     {"task": "depth"}]
