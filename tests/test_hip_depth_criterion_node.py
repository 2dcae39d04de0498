"""The one autograd node of the depth losses (functional._DepthCriterion behind F.berhu_loss_masked,
F.berhu_loss_upsampled and F.depth_criterion): which entry points it launches, in which order, that ``rows`` alone
chooses the row-indexed twins, that ``rows=None`` is an ordinary argument - and that the two plain losses
F.berhu_loss and F.log_softmax_nll return a scalar of their own, which the reference's ``loss += aux_weight *
aux_loss`` may update in place.

The smallest shapes at which neither the sampling nor the row table is the identity: a (2, 1, 5, 7) prediction, 11 x 13
targets with holes of every kind, a cache of 4 rows read through rows = [3, 1].  What the kernels compute is pinned by
test_hip_depth.py, test_hip_upsampled_berhu.py, test_hip_depth_terms.py and test_hip_task0_depth.py."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
TERMS = dict(silog_weight=1.0, grad_weight=0.5)

# public function -> (forward entry points, backward entry points), fp32 names without rows (the issue's table)
LAUNCHES = {
    "berhu_loss_masked": (["nasseg_berhu_masked_fwd"], ["nasseg_berhu_masked_bwd"]),
    "berhu_loss_upsampled": (["nasseg_berhu_up_fwd"], ["nasseg_berhu_up_bwd"]),
    "depth_criterion": (["nasseg_berhu_masked_fwd", "nasseg_depth_terms_fwd"], ["nasseg_depth_terms_bwd"]),
}


def Fn():
    from nas_segm_amd import functional

    return functional


def make_cache():
    """(4, 11, 13) depths in [0.5, 8) with a NaN, an inf, a negative and a zero hole in every row"""
    g = torch.Generator().manual_seed(21)
    cache = 0.5 + 7.5 * torch.rand(4, 11, 13, generator=g)
    cache[:, 0, 3] = float("nan")
    cache[:, 4, 7] = float("inf")
    cache[:, 9, 2] = -1.5
    cache[:, 6, 11] = 0.0
    return cache.to(DEV)


def make_pred(dtype, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (0.3 + 7.7 * torch.rand(2, 1, 5, 7, generator=g)).to(dtype).to(DEV)


def twin(name, dtype, with_rows):
    """the entry point as the table spells it: ``_rows`` before _fwd / _bwd, nasseg_bf16_ for bf16 predictions"""
    if with_rows:
        name = name[:-4] + "_rows" + name[-4:]
    return name if dtype == torch.float32 else "nasseg_bf16_" + name[len("nasseg_"):]


def recorded(monkeypatch, F):
    names = []
    real = F.lib.call
    monkeypatch.setattr(F.lib, "call", lambda name, *args: names.append(name) or real(name, *args))
    return names


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("with_rows", [False, True], ids=["plain", "rows"])
@pytest.mark.parametrize("which", sorted(LAUNCHES))
def test_launch_sequence_of_the_public_depth_losses(which, with_rows, dtype, monkeypatch):
    F = Fn()
    cache = make_cache()
    rows = torch.tensor([3, 1], dtype=torch.int64, device=DEV)
    gathered = cache[rows].contiguous()
    kw = TERMS if which == "depth_criterion" else {}
    fn = getattr(F, which)
    p = make_pred(dtype).requires_grad_(True)
    names = recorded(monkeypatch, F)
    # (rows=None is passed explicitly: the node's argument list and its backward's tuple have one length)
    loss = fn(p, cache, rows=rows, **kw) if with_rows else fn(p, gathered, rows=None, **kw)
    forward = list(names)
    del names[:]
    loss.backward()
    backward = list(names)
    print(which, with_rows, dtype, forward, backward)
    want_fwd, want_bwd = LAUNCHES[which]
    assert forward == [twin(n, dtype, with_rows) for n in want_fwd]
    assert backward == [twin(n, dtype, with_rows) for n in want_bwd]
    value = float(loss.detach())
    assert loss.dim() == 0 and loss.dtype == torch.float32 and math.isfinite(value) and value > 0
    assert p.grad.dtype == dtype and float(p.grad.float().abs().max()) > 0
    if with_rows:  # (the twin reads the rows the table names: the bits of the call on the gathered copy)
        q = make_pred(dtype).requires_grad_(True)
        want = fn(q, gathered, **kw)
        want.backward()
        assert not torch.equal(gathered, cache[:2])
        assert torch.equal(loss.detach(), want.detach()) and torch.equal(p.grad, q.grad)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("sampling, with_terms", [("masked", False), ("up", False), ("masked", True)],
                         ids=["masked", "up", "terms"])
def test_the_node_takes_rows_none_and_returns_named_parts(sampling, with_terms, dtype):
    F = Fn()
    gathered = make_cache()[torch.tensor([3, 1], device=DEV)].contiguous()
    terms = F._depth_terms_config("depth_criterion", 0.0, 1.0, 1.0, 0.5, 0.5, 4, 1e-3) if with_terms else None
    p = make_pred(dtype).requires_grad_(True)
    outs = F._DepthCriterion.apply(p, gathered, 0.0, float("inf"), sampling, 0, terms, None)
    parts = F._DepthParts(*outs)
    present = ("loss", "berhu", "n_valid", "silog", "grad_match") if with_terms else ("loss", "c", "n_valid")
    assert [f for f in parts._fields if getattr(parts, f) is not None] == [f for f in parts._fields if f in present]
    for f in present:
        v = getattr(parts, f)
        assert v.dim() == 0 and v.dtype == torch.float32 and v.requires_grad == (f == "loss"), f
    valid = torch.isfinite(gathered) & (gathered > 0)
    if sampling == "up":
        assert float(parts.n_valid) == float(valid.sum())
    else:
        assert 0 < float(parts.n_valid) <= p.numel()
    parts.loss.backward()  # (a backward of another length: "returned an incorrect number of gradients")
    assert p.grad.shape == p.shape and float(p.grad.float().abs().max()) > 0
    if not with_terms:  # (the library has no terms at the target's size: the node says so)
        bad = F._depth_terms_config("depth_criterion", 0.0, 1.0, 1.0, 0.5, None, 4, 1e-3)
        with pytest.raises(F.NassegError, match="prediction's size"):
            F._DepthCriterion.apply(p, gathered, 0.0, float("inf"), "up", 0, bad, None)
        with pytest.raises(F.NassegError, match="sampling"):
            F._DepthCriterion.apply(p, gathered, 0.0, float("inf"), "nearest", 0, None, None)


def in_place(fn, a1, a2, dtype):
    """``loss += 0.15 * loss2`` on two losses of ``fn`` and the same two taken separately -> nothing; asserts the
    value and, bit for bit, both gradients"""
    p1, p2 = a1.clone().requires_grad_(True), a2.clone().requires_grad_(True)
    loss = fn(p1)
    l1 = float(loss.detach())
    loss2 = fn(p2)
    l2 = float(loss2.detach())
    loss += 0.15 * loss2
    loss.backward()
    print(dtype, "loss", l1, "loss2", l2, "sum", float(loss.detach()))
    assert float(loss.detach()) == pytest.approx(l1 + 0.15 * l2, rel=1e-6)
    q1, q2 = a1.clone().requires_grad_(True), a2.clone().requires_grad_(True)
    fn(q1).backward()
    (fn(q2) * 0.15).backward()
    assert float(q1.grad.float().abs().max()) > 0 and float(q2.grad.float().abs().max()) > 0
    assert torch.equal(p1.grad, q1.grad)  # (the in-place update did not disturb what backward reads)
    assert torch.equal(p2.grad, q2.grad)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_berhu_loss_may_be_updated_in_place(dtype):
    F = Fn()
    g = torch.Generator().manual_seed(9)
    target = (4 * torch.randn(2, 1, 5, 7, generator=g)).to(dtype).to(DEV)
    in_place(lambda p: F.berhu_loss(p, target), make_pred(dtype, 3), make_pred(dtype, 5), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_log_softmax_nll_may_be_updated_in_place(dtype):
    F = Fn()
    g = torch.Generator().manual_seed(10)
    labels = torch.randint(0, 5, (2, 6, 7), generator=g)
    labels[torch.rand(2, 6, 7, generator=g) < 0.2] = 255
    assert bool((labels == 255).any()) and bool((labels != 255).any())
    labels = labels.to(DEV)
    x1 = (2 * torch.randn(2, 5, 6, 7, generator=g)).to(dtype).to(DEV)
    x2 = (2 * torch.randn(2, 5, 6, 7, generator=g)).to(dtype).to(DEV)
    in_place(lambda x: F.log_softmax_nll(x, labels), x1, x2, dtype)
