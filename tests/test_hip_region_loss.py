"""The region-overlap term (soft Jaccard / Dice / Tversky) of the segmentation criterion on the GPU (csrc/loss.hip:
nasseg_ce_region_fwd / _bwd; F.region_overlap_loss, F.cross_entropy_select(region=...), nn.SegmCrossEntropy, the
engine's steps) against the float64 restatement tests/_region_loss_ref.py, evaluated on the values the kernels read."""
import math

import numpy as np
import pytest
import torch

import _region_loss_ref as R
import _segm_loss_ref as CE
from _util import build_product_net, load_json

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def F():
    from nas_segm_amd import functional

    return functional


# ---------------------------------------------------------------------------------------------------------------
# inputs: make_case / on_device of tests/test_hip_segm_loss.py ([P][C] logits with |x| < 20, 20 % of the labels
# ignored, ``boosted`` of the valid pixels +6 on their target channel so that thresh = 0.7 splits the set)
# ---------------------------------------------------------------------------------------------------------------
def make_case(shape, C, seed, scale=1.0, boosted=0.6, label_dtype=np.int64, absent=False):
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
    if absent:
        t = R.drop_odd_classes(t)
    return x, t.astype(label_dtype), w


def on_device(x, t, shape, dtype, misaligned=False):
    """(logits (B, C, H, W) channels_last of ``dtype`` with requires_grad, labels (B, H, W), the logits' values as the
    kernels read them, float64 [P][C]).  ``misaligned``: the logits start one element into their buffer - not on a
    16-byte boundary, which the tiled kernels need"""
    B, H, W = shape
    C = x.shape[1]
    flat = torch.from_numpy(x).reshape(-1).to(DEV).to(dtype)
    if misaligned:
        buf = torch.empty(flat.numel() + 1, device=DEV, dtype=dtype)
        buf[1:].copy_(flat)
        flat = buf[1:]
        assert flat.data_ptr() % 16 != 0
    logits = flat.view(B, H, W, C).permute(0, 3, 1, 2).detach()
    assert logits.is_contiguous(memory_format=torch.channels_last)
    seen = logits.permute(0, 2, 3, 1).reshape(-1, C).float().cpu().numpy().astype(np.float64)
    return logits.requires_grad_(True), torch.from_numpy(t).view(B, H, W).to(DEV), seen


def rows(grad):
    return grad.detach().permute(0, 2, 3, 1).reshape(-1, grad.shape[1]).float().cpu().numpy().astype(np.float64)


def rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / np.maximum(np.abs(want), 1e-300)))


SMALL = (2, 13, 17)
OHEM = dict(thresh=0.7, min_kept=50)
RW = 0.5
# seeds of make_case(SMALL, C, seed, absent=...) at which, for both storage types, no valid float64 loss lies within
# 1e-4 of tau under OHEM except those equal to it (asserted below, on the CPU, before any launch)
SEEDS = {(19, False): 0, (21, False): 0, (64, False): 1, (19, True): 0, (21, True): 0, (64, True): 1}
PRESENT = {19: 10, 21: 11, 64: 32}


def grad_bound(dtype):
    return 2e-6 if dtype == torch.float32 else 1.0 / 128


def check_alone(logits, labels, seen, t, params, dtype, tag):
    Fn = F()
    region, smooth, classes = params
    ref = R.evaluate(seen, t, region, smooth, classes)
    logits.grad = None
    loss, I, S, N, K = Fn.region_overlap_loss(logits, labels, region, smooth, classes, return_parts=True)
    loss.backward()
    assert loss.dim() == 0 and loss.dtype == torch.float32 and I.dtype == S.dtype == torch.float32
    assert N.dtype == K.dtype == torch.int64 and K.dim() == 0
    assert N.cpu().tolist() == ref["N"].tolist() and int(K) == int(ref["K"].sum())
    grad = rows(logits.grad)
    gmax = float(np.abs(ref["grad"]).max())
    lerr = abs(loss.item() - ref["loss"]) / abs(ref["loss"])
    gerr = float(np.abs(grad - ref["grad"]).max()) / gmax
    pres = ref["N"] > 0  # (an absent class: I = 0 exactly; S compared on every class)
    ierr, serr = rel(I.cpu().numpy()[pres], ref["I"][pres]), rel(S.cpu().numpy(), ref["S"])
    print(tag, "alone", params, "loss rel", lerr, "grad/max", gerr, "I rel", ierr, "S rel", serr)
    assert not I.cpu().numpy()[~pres].any()
    assert lerr <= 2e-6 and ierr <= 2e-6 and serr <= 2e-6
    assert gerr <= grad_bound(dtype)
    assert not grad[~ref["valid"]].any()
    assert logits.grad.dtype == dtype and logits.grad.is_contiguous(memory_format=torch.channels_last)
    return loss.detach().clone(), I, S, N


def check_combined(logits, labels, seen, t, w, params, dtype, tag, cfg=OHEM):
    Fn = F()
    region, smooth, classes = params
    ref = R.combined(seen, t, w, region=region, region_weight=RW, smooth=smooth, classes=classes, **cfg)
    gap = CE.gap_to_tau(ref["ce"])
    assert gap >= 1e-4, "input unfit for this check: a loss lies {:.2e} from tau ({})".format(gap, tag)
    logits.grad = None
    loss, pl, tau, counts, lce, lreg = Fn.cross_entropy_select(
        logits, labels, torch.from_numpy(w).to(DEV), return_parts=True, region=region, region_weight=RW,
        region_smooth=smooth, region_classes=classes, **cfg)
    loss.backward()
    assert counts.cpu().tolist() == [ref["ce"]["k"], ref["ce"]["n"], ref["ce"]["n_kept"]]
    grad = rows(logits.grad)
    gmax = float(np.abs(ref["grad"]).max())
    errs = [abs(loss.item() - ref["loss"]) / abs(ref["loss"]), abs(lce.item() - ref["ce"]["loss"]) / ref["ce"]["loss"],
            abs(lreg.item() - ref["region"]["loss"]) / abs(ref["region"]["loss"])]
    gerr = float(np.abs(grad - ref["grad"]).max()) / gmax
    print(tag, "combined", params, "gap", gap, "loss/ce/region rel", errs, "grad/max", gerr)
    assert max(errs) <= 2e-6
    assert gerr <= grad_bound(dtype)
    assert not grad[~ref["region"]["valid"]].any()  # exact zeros on invalid pixels
    if cfg:  # (selection does not thin the region term)
        assert grad[ref["region"]["valid"] & ~ref["ce"]["kept"]].any()
    return gerr, ref


# ---------------------------------------------------------------------------------------------------------------
# 1. against float64 at the smallest shape: one ragged workgroup
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label_dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [19, 21, 64])
def test_loss_and_gradient_against_float64(C, dtype, label_dtype):
    for absent in (False, True):
        x, t, w = make_case(SMALL, C, SEEDS[(C, absent)], label_dtype=label_dtype, absent=absent)
        n_present = len(set(t[t != 255].tolist()))
        if absent:  # (on the CPU, before any launch)
            assert n_present == PRESENT[C] and 2 <= n_present < C
        else:
            assert n_present == C
        logits, labels, seen = on_device(x, t, SMALL, dtype)
        for params in R.PARAM_SETS:
            tag = "C={} {} absent={}".format(C, dtype, absent)
            check_alone(logits, labels, seen, t, params, dtype, tag)
            check_combined(logits, labels, seen, t, w, params, dtype, tag)


# ---------------------------------------------------------------------------------------------------------------
# 2. grid wrap: the forward wraps its 1024 workgroups at 2 x 375 x 376, the backward its 4096 tiles at 3 x 593 x 593
# (the caps of nasseg_ce_sel_fwd / _bwd, kept by nasseg_ce_region_fwd / _bwd).  The gradient bound is what the same
# formulas cost in plain fp32 numpy on the same input (class sums added in fp32); the kernels add theirs in fp64.
# ---------------------------------------------------------------------------------------------------------------
def wrap_case(shape):
    x, t, w = make_case(shape, 19, 1, 0.3, 0.5)
    cfg = dict(thresh=0.7, min_kept=100000)
    ce = CE.cross_entropy_select(x.astype(np.float64), t, w, **cfg)
    # the cross-entropy gradient in fp32 numpy, on the float64 kept set
    x32 = x.astype(np.float32)
    e = np.exp(x32 - x32.max(axis=1, keepdims=True))
    q = e / e.sum(axis=1, keepdims=True, dtype=np.float32)
    tt = np.where(ce["kept"], t, 0)
    wp = np.where(ce["kept"], w[tt], np.float32(0)).astype(np.float32)
    q[np.arange(len(t)), tt] -= np.float32(1)
    ce32 = (wp / wp.sum(dtype=np.float32))[:, None] * q
    return x, t, w, cfg, ce, ce32


@pytest.mark.parametrize("shape", [(2, 375, 376), (3, 593, 593)])
def test_grid_wrap(shape):
    P = shape[0] * shape[1] * shape[2]
    assert P > (1024 if shape[0] == 2 else 4096) * 256
    x, t, w, cfg, ce, ce32 = wrap_case(shape)
    assert CE.gap_to_tau(ce) >= 1e-4
    logits, labels, seen = on_device(x, t, shape, torch.float32)
    for params in (R.PARAM_SETS[0], R.PARAM_SETS[2]):
        region, smooth, classes = params
        r64 = R.evaluate(seen, t, region, smooth, classes)
        r32 = R.evaluate(x, t, region, smooth, classes, dtype=np.float32)
        want = ce["grad"] + RW * r64["grad"]
        gmax = float(np.abs(want).max())
        own = float(np.abs((ce32 + np.float32(RW) * r32["grad"]).astype(np.float64) - want).max()) / gmax
        own_region = float(np.abs(r32["grad"].astype(np.float64) - r64["grad"]).max())
        own_region /= float(np.abs(r64["grad"]).max())
        logits.grad = None
        loss, _, _, counts, lce, lreg = F().cross_entropy_select(
            logits, labels, torch.from_numpy(w).to(DEV), return_parts=True, region=region, region_weight=RW,
            region_smooth=smooth, region_classes=classes, **cfg)
        loss.backward()
        grad = rows(logits.grad)
        gerr = float(np.abs(grad - want).max()) / gmax
        lerr = abs(loss.item() - (ce["loss"] + RW * r64["loss"])) / (ce["loss"] + RW * r64["loss"])
        print(shape, params, "loss rel", lerr, "grad/max: kernels", gerr, "fp32 numpy", own, "(region term alone:",
              own_region, ")")
        assert counts.cpu().tolist() == [ce["k"], ce["n"], ce["n_kept"]] and counts.cpu().tolist()[2] > 100000
        assert lerr <= 2e-6 and abs(lreg.item() - r64["loss"]) <= 2e-6 * r64["loss"]
        assert gerr <= own
        assert not grad[~r64["valid"]].any()
        del grad, want, r64, r32


# ---------------------------------------------------------------------------------------------------------------
# 3. identities, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [19, 64])
def test_identities_bit_for_bit(C, dtype):
    Fn = F()
    for shape in (SMALL, (2, 150, 151)):
        x, t, w = make_case(shape, C, 3)
        dw = torch.from_numpy(w).to(DEV)
        for weight, cfg in ((dw, OHEM), (None, {}), (dw, {})):
            a, labels, _ = on_device(x, t, shape, dtype)
            b, _, _ = on_device(x, t, shape, dtype)
            plain = Fn.cross_entropy_select(a, labels, weight, **cfg)
            (plain * 0.75).backward()
            zero = Fn.cross_entropy_select(b, labels, weight, region="jaccard", region_weight=0, **cfg)
            (zero * 0.75).backward()
            assert torch.equal(zero.detach(), plain.detach()), (float(zero), float(plain))
            assert torch.equal(b.grad, a.grad)
            # the parts of the combined call are the two losses alone; a second call repeats the first
            b.grad = None
            both = Fn.cross_entropy_select(b, labels, weight, return_parts=True, region="dice", region_weight=RW,
                                           region_smooth=0.5, **cfg)
            both[0].backward()
            alone = Fn.region_overlap_loss(a.detach(), labels, "dice", 0.5)
            sel = Fn.cross_entropy_select(a.detach(), labels, weight, return_parts=True, **cfg)
            assert torch.equal(both[5], alone) and torch.equal(both[4], sel[0])
            assert torch.equal(both[1], sel[1]) and torch.equal(both[2], sel[2]) and torch.equal(both[3], sel[3])
            first = b.grad.clone()
            b.grad = None
            again = Fn.cross_entropy_select(b, labels, weight, return_parts=True, region="dice", region_weight=RW,
                                            region_smooth=0.5, **cfg)
            again[0].backward()
            assert all(torch.equal(p, q) for p, q in zip(both, again)) and torch.equal(b.grad, first)
            assert not torch.equal(both[0], plain.detach())  # (the term is there)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [19, 21])
def test_misaligned_logits_take_the_generic_kernels(C, dtype):
    for absent in (False, True):
        x, t, w = make_case(SMALL, C, SEEDS[(C, absent)], absent=absent)
        logits, labels, seen = on_device(x, t, SMALL, dtype, misaligned=True)
        tiled, _, _ = on_device(x, t, SMALL, dtype)
        for params in R.PARAM_SETS:
            tag = "misaligned C={} {} absent={}".format(C, dtype, absent)
            _, I, S, N = check_alone(logits, labels, seen, t, params, dtype, tag)
            check_combined(logits, labels, seen, t, w, params, dtype, tag)
            if C == 19:
                _, I2, S2, N2, _ = F().region_overlap_loss(tiled, labels, *params, return_parts=True)
                pres = N2.cpu().numpy() > 0
                assert torch.equal(N, N2) and rel(S.cpu().numpy(), S2.cpu().numpy()) <= 2e-6
                assert rel(I.cpu().numpy()[pres], I2.cpu().numpy()[pres]) <= 2e-6


# ---------------------------------------------------------------------------------------------------------------
# 4. edge cases
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [19, 64])
def test_edge_cases(C):
    Fn = F()
    x, t, w = make_case(SMALL, C, 5)
    dw = torch.from_numpy(w).to(DEV)
    # nothing valid: the term is exactly 0 with an exactly zero gradient; the combined loss is NaN, as it is today
    logits, labels, seen = on_device(x, t, SMALL, torch.float32)
    none = torch.full_like(labels, 255)
    for params in R.PARAM_SETS:
        logits.grad = None
        loss, I, S, N, K = Fn.region_overlap_loss(logits, none, *params, return_parts=True)
        loss.backward()
        assert float(loss.detach()) == 0.0 and not logits.grad.any() and int(K) == (C if params[2] == "all" else 0)
        assert not N.any() and not I.any() and not S.any()
    assert math.isnan(float(Fn.cross_entropy_select(logits.detach(), none, dw, region="jaccard")))
    assert math.isnan(float(Fn.cross_entropy_select(logits.detach(), none, dw, region="jaccard", min_kept=5)))
    # labels >= C are not valid
    t2 = t.copy()
    t2[::7] = C + 3
    t2[3::11] = 254
    for label_dtype in (np.int64, np.uint8):
        _, lab2, _ = on_device(x, t2.astype(label_dtype), SMALL, torch.float32)
        check_alone(logits, lab2, seen, t2, R.PARAM_SETS[0], torch.float32, "labels >= C")
        check_combined(logits, lab2, seen, t2, w, R.PARAM_SETS[3], torch.float32, "labels >= C", cfg={})
    assert not rows(logits.grad)[::7].any()
    # a single class present
    t3 = np.where(t == 255, 255, 2)
    _, lab3, _ = on_device(x, t3, SMALL, torch.float32)
    for params in R.PARAM_SETS:
        check_alone(logits, lab3, seen, t3, params, torch.float32, "one class")
    _, _, _, N, K = Fn.region_overlap_loss(logits, lab3, return_parts=True)
    assert int(K) == 1 and int(N[2]) == int((t3 == 2).sum()) and int(N.sum()) == int(N[2])
    # the in-place idiom of the reference's step
    from nas_segm_amd.nn import SegmCrossEntropy

    xa, _, _ = make_case(SMALL, C, 6)
    crit = SegmCrossEntropy(weight=torch.from_numpy(w), region="dice", region_weight=RW, **OHEM)
    out, _, _ = on_device(x, t, SMALL, torch.float32)
    aux, _, _ = on_device(xa, t, SMALL, torch.float32)
    loss = crit(out, labels)
    first = float(loss)
    loss += 0.15 * crit(aux, labels)
    loss.backward()
    o2, _, _ = on_device(x, t, SMALL, torch.float32)
    a2, _, _ = on_device(xa, t, SMALL, torch.float32)
    l_out, l_aux = crit(o2, labels), crit(a2, labels)
    (l_out + 0.15 * l_aux).backward()
    assert float(l_out) == first and float(loss) == float(l_out + 0.15 * l_aux)
    assert torch.equal(out.grad, o2.grad) and torch.equal(aux.grad, a2.grad)
    alone = Fn.region_overlap_loss(out.detach().requires_grad_(True), labels)
    alone += 0.15 * Fn.region_overlap_loss(aux.detach(), labels)
    alone.backward()
    with pytest.raises(Fn.NassegError):
        Fn.region_overlap_loss(out, labels[:, :-1])
    with pytest.raises(Fn.NassegError):
        Fn.region_overlap_loss(out.cpu(), labels.cpu())


# ---------------------------------------------------------------------------------------------------------------
# 5. engine: the smallest published net at its recorded shape
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


def test_graphed_segmenter_step_with_a_region_term_equals_host_launches():
    from nas_segm_amd.engine.graphed import GraphedSegmenterStep
    from nas_segm_amd.engine.trainer import segmenter_step
    from nas_segm_amd.nn import SegmCrossEntropy

    batches = [dev_batch(b) for b in seg_batches(2, 42)]
    crit = SegmCrossEntropy(region="dice", thresh=0.7, min_kept=50).prepare(DEV)

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
    net = fresh_net()
    oe, od = optimisers(net)
    plain = SegmCrossEntropy(thresh=0.7, min_kept=50).prepare(DEV)
    assert float(segmenter_step(net, *batches[0], oe, od, 255, 3.0, 3.0, -1, segm_crit=plain)) != eager[0]


def test_graphed_task0_step_with_a_region_term_equals_host_launches(monkeypatch):
    from nas_segm_amd.engine.graphed import GraphedTask0Step
    from nas_segm_amd.engine.trainer import make_task0_step, populate_task0
    from nas_segm_amd.nn import SegmCrossEntropy

    singles = [{"image": b["image"][i:i + 1], "mask": b["mask"][i:i + 1]} for b in seg_batches(2, 43) for i in range(2)]
    crit = SegmCrossEntropy(region="dice", thresh=0.7, min_kept=20).prepare(DEV)
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


def test_a_changed_region_weight_is_a_new_capture():
    from nas_segm_amd.engine.trainer import _segmenter_stepper, segmenter_step
    from nas_segm_amd.nn import SegmCrossEntropy

    batches = [dev_batch(b) for b in seg_batches(2, 44)]
    weights = (0.5, 2.0)

    def host(rws):
        crit = SegmCrossEntropy(region="dice", region_weight=rws[0]).prepare(DEV)
        net = fresh_net()
        oe, od = optimisers(net)
        out = []
        for (x, t), rw in zip(batches, rws):
            crit.region_weight = rw
            out.append(float(segmenter_step(net, x, t, oe, od, 255, 3.0, 3.0, -1, segm_crit=crit)))
        return out

    want, unchanged = host(weights), host((weights[0], weights[0]))
    assert want[0] == unchanged[0] and want[1] != unchanged[1]
    crit = SegmCrossEntropy(region="dice", region_weight=weights[0]).prepare(DEV)
    net = fresh_net()
    oe, od = optimisers(net)
    args = (oe, od, 255, 3.0, 3.0, -1)
    first = _segmenter_stepper(net, batches[0][0], batches[0][1], *args, segm_crit=crit)
    assert first is not None and _segmenter_stepper(net, batches[0][0], batches[0][1], *args, segm_crit=crit) is first
    got = [float(first.step(*batches[0]))]
    crit.region_weight = weights[1]
    second = _segmenter_stepper(net, batches[1][0], batches[1][1], *args, segm_crit=crit)
    assert second is not None and second is not first
    got.append(float(second.step(*batches[1])))
    assert got == want, (got, want)


def test_train_segmenter_epoch_with_a_region_term(monkeypatch):
    from nas_segm_amd.engine import trainer
    from nas_segm_amd.nn import SegmCrossEntropy

    losses = []
    real_value = trainer._loss_value
    monkeypatch.setattr(trainer, "_loss_value", lambda s, loss: losses.append(real_value(s, loss)) or losses[-1])

    def epoch(crit):
        del losses[:]
        net = fresh_net()
        oe, od = optimisers(net)
        assert trainer.train_segmenter.__wrapped__(net, seg_batches(2, 45), oe, od, 0, crit, False, 3.0, 3.0, False,
                                                   print_every=100) is None
        return list(losses), cpu_sd(net)

    with_term, sd1 = epoch(SegmCrossEntropy(region="jaccard", thresh=0.7, min_kept=100))
    without, sd0 = epoch(SegmCrossEntropy(thresh=0.7, min_kept=100))
    assert len(with_term) == 2 and all(math.isfinite(v) and v > 0 for v in with_term), with_term
    assert with_term != without and with_term[0] > without[0]  # (a loss in (0, 1) was added)
    assert any(not torch.equal(sd0[k], sd1[k]) for k in sd0)
