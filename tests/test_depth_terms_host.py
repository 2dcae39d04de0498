"""CPU-only checks of the depth criterion's scale-invariant log and gradient-matching terms: the constructor of
nn.BerHuLoss and its routing (F.berhu_loss_masked / F.berhu_loss_upsampled without a term, F.depth_criterion with
one), config() as the stepper caches' key, the header's new entry points, and the float64 reference
(tests/_depth_terms_ref.py) against a direct double loop over the definition."""
import math

import pytest
import torch

import _depth_terms_ref as R

INF = float("inf")


def test_constructor_refuses_what_the_definition_has_no_meaning_for():
    from nas_segm_amd.nn import BerHuLoss

    ok = dict(silog_weight=1.0, grad_weight=0.5)
    BerHuLoss(0.0, 8.0, **ok)
    BerHuLoss(0.0, 8.0, silog_weight=0.0, grad_weight=0.0, silog_lambda=0.0, grad_scales=1)
    BerHuLoss(0.0, 8.0, silog_weight=1.0, silog_lambda=1.0, grad_scales=8, berhu_weight=0.0)
    bad = [dict(ok, silog_lambda=-0.1), dict(ok, silog_lambda=1.5), dict(ok, silog_lambda=float("nan")),
           dict(ok, grad_scales=0), dict(ok, grad_scales=9), dict(ok, grad_scales=2.5),
           dict(ok, pred_min=0.0), dict(ok, pred_min=-1e-3), dict(ok, pred_min=INF),
           dict(ok, berhu_weight=-1.0), dict(silog_weight=-1.0), dict(grad_weight=-0.5), dict(silog_weight=INF),
           dict(berhu_weight=2.0)]  # (the last: a berHu weight without a term would be ignored)
    for kw in bad:
        with pytest.raises(ValueError):
            BerHuLoss(0.0, 8.0, **kw)
    # the logarithms need positive targets - only where a term takes them
    BerHuLoss(-1.0)
    for kw in (dict(silog_weight=1.0), dict(grad_weight=1.0)):
        with pytest.raises(ValueError, match="valid_min"):
            BerHuLoss(-1.0, **kw)
        # the terms are defined at the prediction's size only (SegmCrossEntropy: region= / lovasz_weight= alike)
        with pytest.raises(ValueError, match="full_size"):
            BerHuLoss(0.0, 8.0, True, **kw)
    with pytest.raises(TypeError):
        BerHuLoss(0.0, 8.0, False, 1.0)  # (the term arguments are keyword-only)


def test_functional_refuses_the_same_arguments_before_any_launch():
    from nas_segm_amd import functional as F

    pred, gt = torch.ones(1, 1, 2, 2), torch.ones(1, 2, 2)
    for kw in (dict(silog_lambda=2.0), dict(grad_scales=0), dict(pred_min=0.0), dict(valid_min=-1.0),
               dict(berhu_weight=-1.0), dict(silog_weight=-1.0), dict(grad_weight=-1.0)):
        with pytest.raises(ValueError):
            F.depth_criterion(pred, gt, **dict(dict(silog_weight=1.0, grad_weight=1.0), **kw))
    with pytest.raises(RuntimeError, match="HIP device"):  # (no CPU fallback)
        F.depth_criterion(pred, gt, silog_weight=1.0)
    with pytest.raises(RuntimeError, match="rows"):
        F.depth_criterion(pred, gt, silog_weight=1.0, rows=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(IndexError):
        F.depth_criterion(pred, gt, silog_weight=1.0, rows=torch.tensor([1]))


def test_default_terms_reach_the_berhu_functions_and_a_term_reaches_depth_criterion(monkeypatch):
    from nas_segm_amd import functional as F
    from nas_segm_amd.nn import BerHuLoss

    calls = []
    monkeypatch.setattr(F, "berhu_loss_masked", lambda *a, **k: calls.append(("masked", a[2:], k)) or "M")
    monkeypatch.setattr(F, "berhu_loss_upsampled", lambda *a, **k: calls.append(("up", a[2:], k)) or "U")
    monkeypatch.setattr(F, "depth_criterion", lambda *a, **k: calls.append(("terms", a[2:], k)) or "T")
    pred, gt, rows = torch.zeros(2, 1, 2, 2), torch.zeros(2, 4, 4), torch.zeros(2, dtype=torch.int64)
    assert BerHuLoss()(pred, gt) == "M" and BerHuLoss(0.0, 5.0)(pred, gt, rows=rows) == "M"
    assert BerHuLoss(0.0, 5.0, True)(pred, gt) == "U"
    assert calls == [("masked", (0.0, INF), {}), ("masked", (0.0, 5.0), {"rows": rows}), ("up", (0.0, 5.0), {})]
    del calls[:]
    crit = BerHuLoss(0.0, 5.0, silog_weight=1.0, grad_weight=0.5, grad_scales=3)
    assert crit(pred, gt) == "T" and crit(pred, gt, rows=rows) == "T"
    assert BerHuLoss(0.0, 5.0, grad_weight=0.25, berhu_weight=0.5, pred_min=1e-2)(pred, gt) == "T"
    terms = dict(berhu_weight=1.0, silog_weight=1.0, silog_lambda=0.5, grad_weight=0.5, grad_scales=3, pred_min=1e-3)
    assert calls == [
        ("terms", (0.0, 5.0), dict(terms, rows=None)), ("terms", (0.0, 5.0), dict(terms, rows=rows)),
        ("terms", (0.0, 5.0), dict(berhu_weight=0.5, silog_weight=None, silog_lambda=0.5, grad_weight=0.25,
                                   grad_scales=4, pred_min=1e-2, rows=None))]
    assert "silog_weight=1.0" in repr(crit) and "grad_scales=3" in repr(crit) and "pred_min" in repr(crit)
    assert "silog" not in repr(BerHuLoss(0.0, 5.0)) and repr(BerHuLoss(0.0, 5.0, True)).count("full_size=True") == 1


def test_config_is_unchanged_without_terms_and_differs_per_value_with_them():
    from nas_segm_amd.nn import BerHuLoss

    assert BerHuLoss().config() == ("berhu", 0.0, INF)
    assert BerHuLoss(0.0, 5.0).config() == ("berhu", 0.0, 5.0)
    assert BerHuLoss(0.0, 5.0, True).config() == ("berhu_up", 0.0, 5.0)
    base = dict(berhu_weight=1.0, silog_weight=1.0, silog_lambda=0.5, grad_weight=0.5, grad_scales=4, pred_min=1e-3)
    cfg = BerHuLoss(0.0, 5.0, **base).config()
    assert cfg[:3] == ("berhu", 0.0, 5.0) and len(cfg) == 4 and cfg == BerHuLoss(0.0, 5.0, **base).config()
    hash(cfg)  # (a dictionary key of the stepper caches)
    seen = {cfg}
    for name, other in (("berhu_weight", 0.5), ("silog_weight", 2.0), ("silog_weight", None), ("silog_lambda", 1.0),
                        ("grad_weight", 1.0), ("grad_weight", None), ("grad_scales", 2), ("pred_min", 1e-2)):
        c = BerHuLoss(0.0, 5.0, **dict(base, **{name: other})).config()
        assert c not in seen, (name, other)
        seen.add(c)
    # a weight of 0.0 is a term (the new node); None is not
    assert BerHuLoss(silog_weight=0.0).has_terms and not BerHuLoss().has_terms


def test_the_trainers_key_their_recorded_steps_on_the_terms(monkeypatch):
    """engine/trainer.py keys a recorded step on config(): two criteria that differ in a term's value never share
    a capture"""
    from nas_segm_amd.engine import trainer
    from nas_segm_amd.nn import BerHuLoss

    assert trainer._depth_crit(BerHuLoss(silog_weight=1.0)) is not None
    a, b = BerHuLoss(0.0, silog_weight=1.0), BerHuLoss(0.0, silog_weight=1.0, silog_lambda=0.85)
    assert a.config() != b.config() and a.config() != BerHuLoss(0.0).config()


def test_header_declares_the_entry_points_with_their_twins_and_constness():
    from nas_segm_amd._lib import HEADER_PATH, pointer_access
    from nas_segm_amd.ffi_gen import prototypes

    protos = {p.name: p for p in prototypes(HEADER_PATH)}
    access = pointer_access()
    assert protos["nasseg_depth_terms_workspace"].ret == "int64_t" and not protos["nasseg_depth_terms_workspace"].args
    for mid in ("", "_rows"):
        for end, written in (("fwd", {"resid", "out", "ws"}), ("bwd", {"dpred"})):
            name = "depth_terms{}_{}".format(mid, end)
            base, twin = protos["nasseg_" + name], protos["nasseg_bf16_" + name]
            assert [a.name for a in base.args] == [a.name for a in twin.args] and base.args[-1].name == "stream"
            got = {base.args[i].name for i, mode in access["nasseg_" + name] if mode == "w"}
            assert got == written, (name, got)  # (what engine/graph_dag.py orders a recorded step by)
            assert ("rows" in [a.name for a in base.args]) == bool(mid)


def direct_loops(p, t, valid, lam, K, pred_min):
    """the definition, pixel by pixel, in Python floats (float64)"""
    B, h, w = len(p), len(p[0]), len(p[0][0])
    r = [[[None] * w for _ in range(h)] for _ in range(B)]
    for b in range(B):
        for y in range(h):
            for x in range(w):
                if valid[b][y][x]:
                    r[b][y][x] = math.log(max(p[b][y][x], pred_min)) - math.log(t[b][y][x])
    rs = [v for img in r for row in img for v in row if v is not None]
    n = len(rs)
    D = sum(v * v for v in rs) / n - lam * (sum(rs) / n) ** 2
    L, M = 0.0, []
    for k in range(K):
        s, Sk, Mk = 2 ** k, 0.0, 0
        for b in range(B):
            for y in range(0, h, s):
                for x in range(0, w, s):
                    if r[b][y][x] is None:
                        continue
                    Mk += 1
                    if x + s < w and r[b][y][x + s] is not None:
                        Sk += abs(r[b][y][x + s] - r[b][y][x])
                    if y + s < h and r[b][y + s][x] is not None:
                        Sk += abs(r[b][y + s][x] - r[b][y][x])
        M.append(Mk)
        if Mk:
            L += Sk / Mk
    return D, L, n, M


def test_reference_agrees_with_a_direct_double_loop():
    g = torch.Generator().manual_seed(4)
    t = 0.5 + 7.5 * torch.rand(1, 4, 5, generator=g)
    t[0, 1, 2], t[0, 3, 0], t[0, 0, 4] = 0.0, float("nan"), INF
    p = (t.nan_to_num(1.0, 1.0).clamp(min=0.5) * torch.exp(0.3 * torch.randn(1, 4, 5, generator=g)))[:, None]
    p[0, 0, 2, 2], p[0, 0, 0, 0] = 5e-4, -1.0  # (clamped to pred_min)
    for lam, K in ((0.5, 3), (1.0, 1), (0.0, 4)):
        out = R.criterion(p, t, 0.0, 8.0, silog_weight=1.0, silog_lambda=lam, grad_weight=1.0, grad_scales=K)
        valid = out["valid"]
        assert out["n"] == 17 and not bool(valid[0, 1, 2]) and not bool(valid[0, 3, 0]) and not bool(valid[0, 0, 4])
        D, L, n, M = direct_loops(p[:, 0].double().tolist(), t.double().tolist(), valid.tolist(), lam, K, R.f32(1e-3))
        assert n == out["n"] and M == out["M"] and M[0] == 17
        assert abs(float(out["D"]) - D) < 1e-12 and abs(float(out["L_gm"]) - L) < 1e-12, (out, D, L)
        assert D > 0 and L > 0
    # the gradient: zero on holes and clamped pixels when the berHu is switched off, and autograd's otherwise
    out, grad = R.loss_and_grad(p, t, valid_min=0.0, valid_max=8.0, berhu_weight=0.0, silog_weight=1.0,
                                grad_weight=1.0, grad_scales=3)
    assert float(grad[0, 0, 1, 2]) == 0.0 and float(grad[0, 0, 2, 2]) == 0.0 and float(grad[0, 0, 0, 0]) == 0.0
    assert float(grad[0, 0, 1, 1]) != 0.0
    # no valid pixel: loss 0, gradient 0
    out, grad = R.loss_and_grad(p, torch.zeros(1, 4, 5), silog_weight=1.0, grad_weight=1.0)
    assert float(out["total"]) == 0.0 and out["n"] == 0 and float(grad.abs().max()) == 0.0


def test_seeded_inputs_keep_ill_conditioned_signs_rare():
    """the share of pixels the GPU gradient test leaves out, at its shapes and seeds 0-2: at most SIGN_SHARE"""
    for case in ((2, 13, 19, 27, 37, 3), (3, 33, 47, 96, 128, 4), (2, 16, 16, 8, 8, 2)):
        for seed in range(3):
            pred, t = R.make_inputs(*case[:5], seed=seed)
            out = R.criterion(pred, t, silog_weight=1.0, grad_weight=1.0, grad_scales=case[5])
            bad = R.ill_conditioned(out, case[5]) & out["valid"]
            assert int(bad.sum()) <= R.SIGN_SHARE * out["n"], (case, seed, int(bad.sum()), out["n"])
