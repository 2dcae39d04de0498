"""Class-weighted / hard-example-mined cross-entropy on the GPU (csrc/loss.hip: nasseg_ohem_threshold,
nasseg_ce_sel_fwd / _bwd; F.cross_entropy_select, nn.SegmCrossEntropy, the engine's steps) against np.sort and the
float64 restatement tests/_segm_loss_ref.py."""
import math

import numpy as np
import pytest
import torch
from torch import nn

import _segm_loss_ref as R
from _util import build_product_net, load_json

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def F():
    from nas_segm_amd import functional

    return functional


def bits(a):
    return np.asarray(a, np.float32).reshape(-1).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------
# 1. the selection alone: bit for bit against np.sort on the same fp32 array
# ---------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 255, 256, 257, 65537, 1000003]
FAMILIES = ["exponential", "all_equal", "two_values", "last_digit", "zeros_denormals", "with_holes"]


def family(name, n, rng):
    if name == "exponential":
        return rng.exponential(1.0, n).astype(np.float32)
    if name == "all_equal":
        return np.full(n, 0.6931472, np.float32)
    if name == "two_values":
        return np.where(rng.rand(n) < 0.4, np.float32(2.5), np.float32(0.125)).astype(np.float32)
    if name == "last_digit":  # 1 + i * 2^-23: the values differ in the last radix digit only (n < 2^23: exact)
        return rng.permutation((1.0 + np.arange(n, dtype=np.float64) * 2.0 ** -23).astype(np.float32))
    if name == "zeros_denormals":
        v = rng.randint(0, 1000, n).astype(np.uint32)  # bit patterns 0 .. 999: +0 and the smallest denormals
        v[rng.rand(n) < 0.3] = 0
        return v.view(np.float32)
    v = rng.exponential(1.0, n).astype(np.float32)
    v[rng.rand(n) < 0.3] = -1.0
    return v


@pytest.mark.parametrize("n", SIZES)
def test_ohem_threshold_equals_sort_bit_for_bit(n):
    Fn = F()
    rng = np.random.RandomState(n)
    calls = 0
    for name in FAMILIES:
        v = family(name, n, rng)
        dv = torch.from_numpy(v).to(DEV)
        part = np.sort(v[v >= 0])
        nv = int(part.size)
        ks = sorted(set(max(1, k) for k in (1, 2, nv // 2, nv - 1, nv)))
        if nv:
            lo, hi = float(part[0]), float(part[-1])
            t_cases = [lo / 2 if lo > 0 else -0.5, float(part[nv // 2]), float(np.float32(hi) * 2 + 1)]
        else:
            t_cases = [0.5]
        cases = [dict(min_kept=k, keep_fraction=0.0, t_loss=None) for k in ks]
        cases += [dict(min_kept=1, keep_fraction=min(1.0, k / float(nv)), t_loss=None) for k in ks if nv]
        cases += [dict(min_kept=k, keep_fraction=0.0, t_loss=t) for t in t_cases for k in (ks[len(ks) // 2], ks[-1])]
        got = [(c, Fn.ohem_threshold(dv, **c)) for c in cases]  # (no synchronisation between the launches)
        for c, (tau, counts) in got:
            t = np.float32(np.inf if c["t_loss"] is None else c["t_loss"])
            w_tau, w_k, w_n, w_kept = R.threshold(v, t, c["min_kept"], c["keep_fraction"])
            assert tau.dtype == torch.float32 and tau.dim() == 0 and counts.dtype == torch.int64
            g_tau, g_counts = tau.cpu().numpy(), counts.cpu().tolist()
            assert bits(g_tau)[0] == bits(w_tau)[0], (name, n, c, float(g_tau), float(w_tau))
            assert g_counts == [w_k, w_n, w_kept], (name, n, c, g_counts, [w_k, w_n, w_kept])
            calls += 1
    assert calls >= len(FAMILIES) * 3


def test_ohem_threshold_refuses_bad_input():
    Fn = F()
    v = torch.rand(16, device=DEV)
    with pytest.raises(Fn.NassegError):
        Fn.ohem_threshold(v.double(), min_kept=1)
    with pytest.raises(Fn.NassegError):
        Fn.ohem_threshold(v.cpu(), min_kept=1)
    with pytest.raises(ValueError):
        Fn.ohem_threshold(v, keep_fraction=0.5, min_kept=0)
    with pytest.raises(ValueError):
        Fn.ohem_threshold(v, thresh=1.5, min_kept=1)


# ---------------------------------------------------------------------------------------------------------------
# inputs of 2 - 5: [P][C] logits with |x| < 20; 20 % of the labels ignored; ``boosted`` of the valid pixels get +6 on
# their target channel, so that thresh = 0.7 (a loss of 0.357) splits the set
# ---------------------------------------------------------------------------------------------------------------
def make_case(shape, C, seed, scale=1.0, boosted=0.6, label_dtype=np.int64):
    B, H, W = shape
    P = B * H * W
    rng = np.random.RandomState(seed)
    x = np.clip(rng.randn(P, C) * scale, -12.0, 12.0).astype(np.float32)
    t = rng.randint(0, C, size=P)
    ignored = rng.rand(P) < 0.2
    boost = (rng.rand(P) < boosted) & ~ignored
    x[np.arange(P)[boost], t[boost]] += np.float32(6.0)
    t[ignored] = 255
    w = (rng.rand(C) + 0.5).astype(np.float32)
    return x, t.astype(label_dtype), w


def on_device(x, t, shape, dtype):
    """(logits (B, C, H, W) channels_last of ``dtype`` with requires_grad, labels (B, H, W), the logits' values as the
    kernels read them, float64 [P][C])"""
    B, H, W = shape
    C = x.shape[1]
    logits = torch.from_numpy(x).view(B, H, W, C).permute(0, 3, 1, 2).to(DEV).to(dtype)
    seen = logits.detach().permute(0, 2, 3, 1).reshape(-1, C).float().cpu().numpy().astype(np.float64)
    return logits.requires_grad_(True), torch.from_numpy(t).view(B, H, W).to(DEV), seen


def rows(grad):
    return grad.detach().permute(0, 2, 3, 1).reshape(-1, grad.shape[1]).float().cpu().numpy().astype(np.float64)


SMALL = (2, 13, 17)
# seeds of make_case(SMALL, C, seed) at which, for every configuration of CONFIGS and both storage types, no valid
# float64 loss lies within 1e-4 of tau except those equal to it (asserted below, on the CPU, before any launch)
SEEDS = {19: 0, 21: 0, 64: 1}
CONFIGS = [dict(), dict(thresh=0.7, min_kept=50), dict(keep_fraction=0.25, min_kept=1),
           dict(thresh=0.3, min_kept=10 ** 6)]


@pytest.mark.parametrize("label_dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [19, 21, 64])
def test_pixel_losses_and_fused_selection(C, dtype, label_dtype):
    Fn = F()
    x, t, w = make_case(SMALL, C, SEEDS[C], label_dtype=label_dtype)
    logits, labels, seen = on_device(x, t, SMALL, dtype)
    want, valid, _ = R.pixel_losses(seen, t)
    with torch.no_grad():
        loss, pl, tau, counts = Fn.cross_entropy_select(logits, labels, thresh=0.7, min_kept=50, return_parts=True)
    assert tuple(pl.shape) == SMALL and pl.dtype == torch.float32
    got = pl.cpu().numpy().reshape(-1)
    assert np.array_equal(got[~valid], np.full(int((~valid).sum()), -1.0, np.float32))
    err = float(np.abs(got[valid] - want[valid]).max())
    print("pixel_loss max err", err)
    assert err <= 1e-5  # (the fp32 error bound for |x| <= 20 is about 5e-6)
    assert (got[valid] >= 0).all()
    tau2, counts2 = Fn.ohem_threshold(pl, thresh=0.7, min_kept=50)
    assert bits(tau.cpu().numpy())[0] == bits(tau2.cpu().numpy())[0]
    assert counts.cpu().tolist() == counts2.cpu().tolist()
    n_hard = int((got[valid] >= np.float32(-np.log(0.7))).sum())
    assert 50 < n_hard < int(valid.sum())  # (the threshold does split the set)
    assert counts.cpu().tolist() == [50, int(valid.sum()), n_hard]
    # without selection: every valid pixel is kept, tau = -inf
    with torch.no_grad():
        _, pl0, tau0, counts0 = Fn.cross_entropy_select(logits, labels, return_parts=True)
    assert torch.equal(pl0, pl) and float(tau0) == -math.inf
    assert counts0.cpu().tolist() == [int(valid.sum())] * 3


def check_against_restatement(shape, C, seed, dtype, cfg, weight, scale=1.0, boosted=0.6):
    Fn = F()
    x, t, w = make_case(shape, C, seed, scale, boosted)
    w = w if weight else None
    logits, labels, seen = on_device(x, t, shape, dtype)
    ref = R.cross_entropy_select(seen, t, w, **cfg)
    gap = R.gap_to_tau(ref)
    assert gap >= 1e-4, "input unfit for this check: a loss lies {:.2e} from tau (seed {})".format(gap, seed)
    dw = None if w is None else torch.from_numpy(w).to(DEV)
    loss, pl, tau, counts = Fn.cross_entropy_select(logits, labels, dw, return_parts=True, **cfg)
    loss.backward()
    assert loss.dim() == 0 and loss.dtype == torch.float32
    assert counts.cpu().tolist() == [ref["k"], ref["n"], ref["n_kept"]], (counts.cpu().tolist(), ref["k"], ref["n"],
                                                                         ref["n_kept"])
    rel = abs(loss.item() - ref["loss"]) / abs(ref["loss"])
    grad = rows(logits.grad)
    gmax = float(np.abs(ref["grad"]).max())
    gerr = float(np.abs(grad - ref["grad"]).max())
    print("cfg", cfg, "weight", weight, "gap", gap, "loss rel err", rel, "grad err / max", gerr / gmax)
    assert rel <= 2e-6
    assert gerr <= (2e-6 if dtype == torch.float32 else 1.0 / 128) * gmax
    assert not grad[~ref["kept"]].any()  # exact zeros on every pixel that is not kept, ignored ones included
    assert logits.grad.dtype == dtype and logits.grad.is_contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("weight", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [19, 21, 64])
def test_loss_and_gradient_against_float64(C, dtype, weight):
    for cfg in CONFIGS:
        if not cfg and not weight:
            continue  # (no weights, no selection: test_identity_with_the_plain_loss)
        check_against_restatement(SMALL, C, SEEDS[C], dtype, cfg, weight)


# ---------------------------------------------------------------------------------------------------------------
# 4. grid-stride coverage: the forward wraps its 1024 workgroups at 2 x 375 x 376, the backward its 4096 tiles at
# 3 x 593 x 593.  Logits of a small spread and half of the pixels boosted: more than min_kept hard pixels, none near
# the threshold (the precondition of check_against_restatement holds with a million losses)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 375, 376), (3, 593, 593)])
def test_grid_stride_coverage(shape):
    Fn = F()
    cfg = dict(thresh=0.7, min_kept=100000)
    assert shape[0] * shape[1] * shape[2] > (1024 if shape[0] == 2 else 4096) * 256
    check_against_restatement(shape, 19, 1, torch.float32, cfg, True, scale=0.3, boosted=0.5)
    x, t, _ = make_case(shape, 19, 1, 0.3, 0.5)
    logits, labels, seen = on_device(x, t, shape, torch.float32)
    want, valid, _ = R.pixel_losses(seen, t)
    with torch.no_grad():
        _, pl, tau, counts = Fn.cross_entropy_select(logits, labels, return_parts=True, **cfg)
    got = pl.cpu().numpy().reshape(-1)
    assert (got[~valid] == -1.0).all() and float(np.abs(got[valid] - want[valid]).max()) <= 1e-5
    tau2, counts2 = Fn.ohem_threshold(pl, **cfg)
    assert bits(tau.cpu().numpy())[0] == bits(tau2.cpu().numpy())[0] and counts.cpu().tolist() == counts2.cpu().tolist()
    assert counts.cpu().tolist()[0] == 100000 and counts.cpu().tolist()[2] > 100000


# ---------------------------------------------------------------------------------------------------------------
# 5. unit weights, no selection: F.log_softmax_nll bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [19, 64])
def test_identity_with_the_plain_loss(C, dtype):
    Fn = F()
    for shape in (SMALL, (2, 150, 151)):  # (one workgroup-round, and several with a ragged last tile)
        x, t, _ = make_case(shape, C, 3)
        a, labels, _ = on_device(x, t, shape, dtype)
        b, _, _ = on_device(x, t, shape, dtype)
        plain = Fn.log_softmax_nll(a, labels, 255)
        (plain * 0.75).backward()
        for weight in (torch.ones(C, device=DEV), None):
            b.grad = None
            sel = Fn.cross_entropy_select(b, labels, weight, 255)
            (sel * 0.75).backward()
            assert torch.equal(sel.detach(), plain.detach()), (float(sel), float(plain))
            assert torch.equal(b.grad, a.grad)


# ---------------------------------------------------------------------------------------------------------------
# 6. the in-place idiom of the reference's step, and bad input
# ---------------------------------------------------------------------------------------------------------------
def test_in_place_idiom_and_bad_input():
    from nas_segm_amd.nn import SegmCrossEntropy

    Fn = F()
    x, t, w = make_case(SMALL, 19, 5)
    xa, _, _ = make_case(SMALL, 19, 6)
    crit = SegmCrossEntropy(weight=torch.from_numpy(w).double(), thresh=0.7, min_kept=50)  # (fp64, host: prepared)
    out, labels, _ = on_device(x, t, SMALL, torch.float32)
    aux, _, _ = on_device(xa, t, SMALL, torch.float32)
    loss = crit(out, labels)
    first = float(loss)
    loss += 0.15 * crit(aux, labels)
    loss.backward()
    assert crit.weight.dtype == torch.float32 and crit.weight.is_cuda
    o2, _, _ = on_device(x, t, SMALL, torch.float32)
    a2, _, _ = on_device(xa, t, SMALL, torch.float32)
    l_out, l_aux = crit(o2, labels), crit(a2, labels)
    (l_out + 0.15 * l_aux).backward()
    assert float(l_out) == first and float(loss) == float(l_out + 0.15 * l_aux)
    assert torch.equal(out.grad, o2.grad) and torch.equal(aux.grad, a2.grad)  # (nothing backward reads was disturbed)
    dw = torch.from_numpy(w).to(DEV)
    with pytest.raises(Fn.NassegError):
        Fn.cross_entropy_select(out, labels, dw[:-1])
    with pytest.raises(Fn.NassegError):
        Fn.cross_entropy_select(out, labels, dw.double())
    with pytest.raises(Fn.NassegError):
        Fn.cross_entropy_select(out, labels[:, :-1])
    with pytest.raises(Fn.NassegError):
        Fn.cross_entropy_select(out, labels.to(torch.int32))
    with pytest.raises(Fn.NassegError):
        Fn.cross_entropy_select(out, labels, dw.cpu())
    with pytest.raises(ValueError):
        Fn.cross_entropy_select(out, labels, dw, thresh=0.7)  # selection without min_kept >= 1
    # nothing valid: NaN, as nasseg_ce_fwd and torch
    assert math.isnan(float(Fn.cross_entropy_select(out.detach(), torch.full_like(labels, 255), dw, min_kept=5)))


# ---------------------------------------------------------------------------------------------------------------
# 7. engine: the smallest published net at its recorded shape
# ---------------------------------------------------------------------------------------------------------------
REC = load_json("nets_meta.json")["wacv_arch0"]


def seg_batches(n, seed):
    g = torch.Generator().manual_seed(seed)
    B, _, H, W = REC["shape"]
    out = []
    for _ in range(n):
        mask = torch.randint(0, REC["classes"], (B, H, W), generator=g)
        mask[:, :6] = 255
        out.append({"image": torch.randn(B, 3, H, W, generator=g), "mask": mask})
    return out


def fresh_net():
    return build_product_net(REC["kind"], REC["genotype"], REC["classes"], REC["dec_kwargs"], REC["seed"]).to(DEV).train()


def optimisers(net):
    return (torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-5),
            torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5))


def dev_batch(b):
    return b["image"].to(DEV).contiguous(memory_format=torch.channels_last), b["mask"].to(DEV)


def cpu_sd(module):
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


def class_weights():
    return torch.linspace(0.25, 3.0, REC["classes"])


def test_segmenter_step_honours_class_weights():
    from nas_segm_amd.engine.trainer import segmenter_step
    from nas_segm_amd.nn import SegmCrossEntropy

    x, t = dev_batch(seg_batches(1, 41)[0])

    def run(crit):
        net = fresh_net()
        oe, od = optimisers(net)
        loss = float(segmenter_step(net, x, t, oe, od, 255, 3.0, 3.0, -1, segm_crit=crit))
        return loss, cpu_sd(net)

    l_nll, sd_nll = run(nn.NLLLoss(weight=class_weights(), ignore_index=255))
    l_own, sd_own = run(SegmCrossEntropy(weight=class_weights()))
    l_plain, sd_plain = run(nn.NLLLoss(ignore_index=255))
    l_none, sd_none = run(None)
    assert l_nll == l_own and l_plain == l_none
    for k in sd_nll:
        assert torch.equal(sd_nll[k], sd_own[k]), k
        assert torch.equal(sd_plain[k], sd_none[k]), k
    assert l_nll != l_plain  # the weights are not dropped
    assert any(not torch.equal(sd_nll[k], sd_plain[k]) for k in sd_nll if k.endswith("weight"))


def test_graphed_segmenter_step_with_ohem_equals_host_launches():
    from nas_segm_amd.engine.graphed import GraphedSegmenterStep
    from nas_segm_amd.engine.trainer import segmenter_step
    from nas_segm_amd.nn import SegmCrossEntropy

    batches = [dev_batch(b) for b in seg_batches(2, 42)]
    crit = SegmCrossEntropy(weight=class_weights(), thresh=0.7, min_kept=50).prepare(DEV)

    net = fresh_net()
    oe, od = optimisers(net)
    eager = [float(segmenter_step(net, x, t, oe, od, 255, 3.0, 3.0, -1, segm_crit=crit)) for x, t in batches]
    sd0 = cpu_sd(net)
    net = fresh_net()
    oe, od = optimisers(net)
    stepper = GraphedSegmenterStep(net, batches[0][0], batches[0][1], oe, od, 255, 3.0, 3.0, -1, segm_crit=crit)
    replayed = [float(stepper.step(x, t)) for x, t in batches]
    sd1 = cpu_sd(net)
    assert eager == replayed and all(math.isfinite(v) for v in eager), (eager, replayed)
    for k in sd0:  # parameters and BatchNorm buffers
        assert torch.equal(sd0[k], sd1[k]), k


def test_graphed_task0_step_with_ohem_equals_host_launches(monkeypatch):
    from nas_segm_amd.engine.graphed import GraphedTask0Step
    from nas_segm_amd.engine.trainer import make_task0_step, populate_task0
    from nas_segm_amd.nn import SegmCrossEntropy

    singles = [{"image": b["image"][i:i + 1], "mask": b["mask"][i:i + 1]} for b in seg_batches(2, 43) for i in range(2)]
    crit = SegmCrossEntropy(thresh=0.7, min_kept=20, keep_fraction=0.25).prepare(DEV)
    order = [np.array([2, 0]), np.array([1, 3])]

    def run(graphed):
        net = fresh_net()
        Xy = populate_task0.__wrapped__(net, singles, None, 4, do_kd=False)
        net.decoder.train()
        _, od = optimisers(net)
        if graphed:
            step = GraphedTask0Step(Xy, net, od, 2, 255, 3.0, 0, segm_crit=crit).step
        else:
            monkeypatch.setenv("NASSEG_GRAPH", "0")
            step = make_task0_step(Xy, net, od, 2, 255, 3.0, 0, segm_crit=crit)
        return [float(step(idx)) for idx in order], cpu_sd(net)

    l0, sd0 = run(False)
    l1, sd1 = run(True)
    assert l0 == l1 and all(math.isfinite(v) for v in l0), (l0, l1)
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k


def test_a_changed_min_kept_is_a_new_capture():
    from nas_segm_amd.engine.trainer import _segmenter_stepper, segmenter_step
    from nas_segm_amd.nn import SegmCrossEntropy

    batches = [dev_batch(b) for b in seg_batches(2, 44)]
    kept = (40, 300)

    def host(min_kepts):
        crit = SegmCrossEntropy(min_kept=min_kepts[0]).prepare(DEV)
        net = fresh_net()
        oe, od = optimisers(net)
        out = []
        for (x, t), k in zip(batches, min_kepts):
            crit.min_kept = k
            out.append(float(segmenter_step(net, x, t, oe, od, 255, 3.0, 3.0, -1, segm_crit=crit)))
        return out

    want, unchanged = host(kept), host((kept[0], kept[0]))
    assert want[0] == unchanged[0] and want[1] != unchanged[1]  # (min_kept matters on the second batch)
    crit = SegmCrossEntropy(min_kept=kept[0]).prepare(DEV)
    net = fresh_net()
    oe, od = optimisers(net)
    args = (oe, od, 255, 3.0, 3.0, -1)
    first = _segmenter_stepper(net, batches[0][0], batches[0][1], *args, segm_crit=crit)
    assert first is not None and _segmenter_stepper(net, batches[0][0], batches[0][1], *args, segm_crit=crit) is first
    got = [float(first.step(*batches[0]))]
    crit.min_kept = kept[1]
    second = _segmenter_stepper(net, batches[1][0], batches[1][1], *args, segm_crit=crit)
    assert second is not None and second is not first
    got.append(float(second.step(*batches[1])))
    assert got == want, (got, want)


def test_train_segmenter_epoch_with_an_ohem_criterion(monkeypatch):
    from nas_segm_amd.engine import trainer
    from nas_segm_amd.nn import SegmCrossEntropy

    losses = []
    real_value = trainer._loss_value
    monkeypatch.setattr(trainer, "_loss_value", lambda s, loss: losses.append(real_value(s, loss)) or losses[-1])
    net = fresh_net()
    oe, od = optimisers(net)
    crit = SegmCrossEntropy(weight=class_weights(), thresh=0.7, min_kept=100)
    before = cpu_sd(net)
    assert trainer.train_segmenter.__wrapped__(net, seg_batches(2, 45), oe, od, 0, crit, False, 3.0, 3.0, False,
                                               print_every=100) is None
    assert len(losses) == 2 and all(math.isfinite(v) and v > 0 for v in losses), losses
    after = cpu_sd(net)
    assert any(not torch.equal(before[k], after[k]) for k in before)
