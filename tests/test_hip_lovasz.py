"""The Lovasz-Softmax term of the segmentation criterion on the GPU (csrc/lovasz.hip: nasseg_lovasz_coef / _fwd /
_bwd; F.lovasz_softmax_loss, F.lovasz_from_errors, F.cross_entropy_select(lovasz_weight=...), nn.SegmCrossEntropy, the
engine's steps) against the float64 restatement tests/_lovasz_ref.py.  The restatement takes its ORDER from the fp32
errors the device wrote (the order is the kernels' contract on the values they computed) and its values from float64
on the logits the kernels read.  Bounds: 2e-6 relative for losses, grad_bound(dtype) of the maximum for gradients,
equality for every integer (ranks, counts)."""
import math

import numpy as np
import pytest
import torch

import _lovasz_ref as L
import _region_loss_ref as R
import _segm_loss_ref as CE
from _util import build_product_net, load_json

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def F():
    from nas_segm_amd import functional

    return functional


# ---------------------------------------------------------------------------------------------------------------
# inputs: make_case / on_device of tests/test_hip_region_loss.py
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
    kernels read them, float64 [P][C]).  ``misaligned``: the logits start one element into their buffer"""
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


def flat(parts):
    return parts.detach().reshape(-1, parts.shape[-1]).cpu().numpy()


SMALL = (2, 13, 17)
OHEM = dict(thresh=0.7, min_kept=50)
LW = 0.5
# seeds of make_case(SMALL, C, seed, absent=...) of tests/test_hip_region_loss.py: no valid float64 loss lies within
# 1e-4 of tau under OHEM except those equal to it (asserted below, on the CPU, before any launch)
SEEDS = {(19, False): 0, (21, False): 0, (64, False): 1, (19, True): 0, (21, True): 0, (64, True): 1}


def grad_bound(dtype):
    return 2e-6 if dtype == torch.float32 else 1.0 / 128


def check_alone(logits, labels, seen, t, classes, dtype, tag):
    """F.lovasz_softmax_loss against the restatement; returns (loss, device errors [P][C] fp32, device ranks)"""
    logits.grad = None
    loss, errors, rank, N, K = F().lovasz_softmax_loss(logits, labels, classes, return_parts=True)
    loss.backward()
    assert loss.dim() == 0 and loss.dtype == torch.float32 and errors.dtype == torch.float32
    assert rank.dtype == torch.int32 and N.dtype == K.dtype == torch.int64 and K.dim() == 0
    assert tuple(errors.shape) == tuple(rank.shape) == tuple(labels.shape) + (logits.shape[1],)
    E, rk = flat(errors), flat(rank)
    ref = L.evaluate(seen, t, classes, errors=E)
    valid = ref["valid"]
    eerr = float(np.abs(E[valid].astype(np.float64) - ref["errors"][valid]).max()) if valid.any() else 0.0
    assert (E[~valid] == -1.0).all()
    assert np.array_equal(rk, ref["rank"]), "{}: {} ranks differ".format(tag, int((rk != ref["rank"]).sum()))
    assert N.cpu().tolist() == ref["N"].tolist() and int(K) == int(ref["K"].sum())
    grad = rows(logits.grad)
    gmax = float(np.abs(ref["grad"]).max())
    lerr = abs(loss.item() - ref["loss"]) / abs(ref["loss"]) if ref["loss"] else abs(loss.item())
    gerr = float(np.abs(grad - ref["grad"]).max()) / gmax if gmax else float(np.abs(grad).max())
    print(tag, "alone", classes, "errors abs", eerr, "loss rel", lerr, "grad/max", gerr)
    assert eerr <= 2e-6
    assert lerr <= 2e-6
    assert gerr <= grad_bound(dtype)
    assert not grad[~valid].any()
    assert logits.grad.dtype == dtype and logits.grad.is_contiguous(memory_format=torch.channels_last)
    return loss.detach().clone(), E, rk


def check_combined(logits, labels, seen, t, w, classes, E, dtype, tag, cfg=OHEM, region=None):
    kw = dict(region=region, region_weight=LW) if region is not None else {}
    ref = L.combined(seen, t, w, lovasz_weight=LW, classes=classes, errors=E, **dict(cfg, **kw))
    gap = CE.gap_to_tau(ref["ce"])
    assert gap >= 1e-4, "input unfit for this check: a loss lies {:.2e} from tau ({})".format(gap, tag)
    logits.grad = None
    out = F().cross_entropy_select(logits, labels, torch.from_numpy(w).to(DEV), return_parts=True, lovasz_weight=LW,
                                   lovasz_classes=classes, **dict(cfg, **kw))
    assert len(out) == (7 if region is not None else 6)
    loss, counts, lce, llov = out[0], out[3], out[4], out[-1]
    loss.backward()
    assert counts.cpu().tolist() == [ref["ce"]["k"], ref["ce"]["n"], ref["ce"]["n_kept"]]
    grad = rows(logits.grad)
    gmax = float(np.abs(ref["grad"]).max())
    errs = [abs(loss.item() - ref["loss"]) / abs(ref["loss"]), abs(lce.item() - ref["ce"]["loss"]) / ref["ce"]["loss"],
            abs(llov.item() - ref["lovasz"]["loss"]) / abs(ref["lovasz"]["loss"])]
    if region is not None:
        errs.append(abs(out[5].item() - ref["region"]["loss"]) / abs(ref["region"]["loss"]))
    gerr = float(np.abs(grad - ref["grad"]).max()) / gmax
    print(tag, "combined", classes, region, "gap", gap, "loss/ce/lovasz[/region] rel", errs, "grad/max", gerr)
    assert max(errs) <= 2e-6
    assert gerr <= grad_bound(dtype)
    assert not grad[~ref["lovasz"]["valid"]].any()  # exact zeros on invalid pixels
    if cfg:  # (selection does not thin the Lovasz term)
        assert grad[ref["lovasz"]["valid"] & ~ref["ce"]["kept"]].any()


# ---------------------------------------------------------------------------------------------------------------
# 1. against float64 at the smallest shape: one ragged workgroup
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label_dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [19, 21, 64])
def test_errors_ranks_loss_and_gradient_against_float64(C, dtype, label_dtype):
    for absent in (False, True):
        x, t, w = make_case(SMALL, C, SEEDS[(C, absent)], label_dtype=label_dtype, absent=absent)
        n_present = len(set(t[t != 255].tolist()))
        assert (2 <= n_present < C) if absent else n_present == C
        logits, labels, seen = on_device(x, t, SMALL, dtype)
        for classes in ("present", "all"):
            tag = "C={} {} absent={}".format(C, dtype, absent)
            _, E, _ = check_alone(logits, labels, seen, t, classes, dtype, tag)
            check_combined(logits, labels, seen, t, w, classes, E, dtype, tag)
            check_combined(logits, labels, seen, t, w, classes, E, dtype, tag, cfg={}, region="dice")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [2, 31, 32, 63])
def test_class_counts_at_which_the_kernels_change(C, dtype):
    """C <= 31: errors and backward through LDS tiles; 32 .. 63: tiled errors, one lane per row backward; 64 and more
    (above): one lane per row throughout; C = 2: the smallest the term takes"""
    x, t, w = make_case(SMALL, C, 8)
    for misaligned in (False, True):
        logits, labels, seen = on_device(x, t, SMALL, dtype, misaligned=misaligned)
        for classes in ("present", "all"):
            check_alone(logits, labels, seen, t, classes, dtype, "C={} {} misaligned={}".format(C, dtype, misaligned))


# ---------------------------------------------------------------------------------------------------------------
# 2. many workgroups, a ragged last tile, the ties fp32 softmax values have by themselves
# ---------------------------------------------------------------------------------------------------------------
MID = (2, 150, 151)


@pytest.mark.parametrize("C,dtype", [(19, torch.float32), (64, torch.float32), (19, torch.bfloat16)])
def test_many_workgroups_and_natural_ties(C, dtype):
    x, t, w = make_case(MID, C, 2)
    logits, labels, seen = on_device(x, t, MID, dtype)
    _, E, _ = check_alone(logits, labels, seen, t, "present", dtype, "mid C={} {}".format(C, dtype))
    v = L.valid_mask(t, C)
    ties = sum(int(v.sum()) - len(np.unique(E[v, c])) for c in range(C))
    print("exact fp32 ties among the valid errors:", ties)
    assert ties > 0


@pytest.mark.parametrize("C", [19, 64])
def test_identical_rows_get_identical_errors_and_the_tie_rule(C):
    """every odd pixel's row is the even pixel's before it, the labels are independent: q is a function of the row
    alone, so the pair's errors are bit-equal on every class that is the label of neither (on all classes where the
    labels agree) - thousands of exact ties that only the index breaks"""
    x, t, w = make_case(MID, C, 4)
    x[1::2] = x[0::2]
    logits, labels, seen = on_device(x, t, MID, torch.float32)
    _, E, rk = check_alone(logits, labels, seen, t, "all", torch.float32, "pairs C={}".format(C))
    a, b = E[0::2].view(np.uint32), E[1::2].view(np.uint32)
    ta, tb = t[0::2], t[1::2]
    both = L.valid_mask(ta, C) & L.valid_mask(tb, C)
    cols = np.arange(C)[None, :]
    free = both[:, None] & (cols != ta[:, None]) & (cols != tb[:, None])
    assert free.sum() > 1000 and np.array_equal(a[free], b[free])
    same = both & (ta == tb)
    assert same.any() and np.array_equal(a[same], b[same])
    ra, rb = rk[0::2], rk[1::2]
    assert (ra[free] < rb[free]).all()  # (equal errors: the lower index first)


# ---------------------------------------------------------------------------------------------------------------
# 3. 5.4 M keys: 69 tiles of 4096 per class, a ragged last one (the kernels have no grid cap: a workgroup per tile)
# ---------------------------------------------------------------------------------------------------------------
def test_large():
    shape = (2, 375, 376)
    x, t, w = make_case(shape, 19, 1, 0.3, 0.5)
    logits, labels, seen = on_device(x, t, shape, torch.float32)
    check_alone(logits, labels, seen, t, "present", torch.float32, "large")


# ---------------------------------------------------------------------------------------------------------------
# 4. the sort-and-scan half on crafted keys
# ---------------------------------------------------------------------------------------------------------------
def crafted():
    P, C = 40 * 41, 4
    rng = np.random.RandomState(7)
    t = rng.randint(0, C, size=P)
    t[rng.rand(P) < 0.1] = 255
    out = {}
    out["all equal"] = (np.full((P, C), 0.5, np.float32), t)
    low = (np.uint32(0x3F000000) | rng.randint(0, 256, size=(P, C)).astype(np.uint32)).view(np.float32)
    out["lowest mantissa byte"] = (low, t)
    pool = np.array([0.0, 1e-45, 1e-40, 1.1754942e-38, 1.0], np.float32)
    out["denormals, zeros, ones"] = (pool[rng.randint(0, len(pool), size=(P, C))], t)
    for name, e0 in (("single foreground first", 1.0), ("single foreground last", 0.0)):
        t1 = rng.randint(1, C, size=P)
        t1[rng.rand(P) < 0.1] = 255
        t1[777] = 0
        E = (rng.rand(P, C) * 0.8 + 0.1).astype(np.float32)
        E[777, 0] = e0
        out[name] = (E, t1)
    return out


@pytest.mark.parametrize("classes", ["present", "all"])
def test_from_errors_on_crafted_keys(classes):
    for name, (E, t) in crafted().items():
        ref = L.from_errors(E, t, classes)
        loss, coef, rank, N, K = F().lovasz_from_errors(torch.from_numpy(E).view(1, 40, 41, 4).to(DEV),
                                                        torch.from_numpy(t).view(1, 40, 41).to(DEV), classes)
        rk, cf = flat(rank), flat(coef).astype(np.float64)
        assert np.array_equal(rk, ref["rank"]), name
        assert N.cpu().tolist() == ref["N"].tolist() and int(K) == int(ref["K"].sum())
        nz = ref["coef"] != 0
        cerr = float(np.max(np.abs(cf[nz] - ref["coef"][nz]) / np.abs(ref["coef"][nz])))
        lerr = abs(loss.item() - ref["loss"]) / max(abs(ref["loss"]), 1e-300)
        print(name, classes, "coef rel", cerr, "loss rel", lerr)
        assert cerr <= 2e-6 and not cf[~nz].any() and lerr <= 2e-6
        if name.startswith("single foreground"):
            n = int(ref["valid"].sum())
            assert rk[777, 0] == (0 if name.endswith("first") else n - 1) and int(N[0]) == 1


# ---------------------------------------------------------------------------------------------------------------
# 5. identities, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [19, 64])
def test_identities_bit_for_bit(C, dtype):
    Fn = F()
    for shape in (SMALL, MID):
        x, t, w = make_case(shape, C, 3)
        dw = torch.from_numpy(w).to(DEV)
        for weight, cfg in ((dw, OHEM), (None, {}), (dw, dict(region="dice", region_weight=0.5))):
            a, labels, _ = on_device(x, t, shape, dtype)
            b, _, _ = on_device(x, t, shape, dtype)
            plain = Fn.cross_entropy_select(a, labels, weight, return_parts=True, **cfg)
            (plain[0] * 0.75).backward()
            zero = Fn.cross_entropy_select(b, labels, weight, lovasz_weight=0, **cfg)
            (zero * 0.75).backward()
            assert torch.equal(zero.detach(), plain[0].detach()), (float(zero), float(plain[0]))
            assert torch.equal(b.grad, a.grad)
            b.grad = None
            both = Fn.cross_entropy_select(b, labels, weight, return_parts=True, lovasz_weight=LW, **cfg)
            both[0].backward()
            alone = Fn.lovasz_softmax_loss(a.detach(), labels, return_parts=True)
            assert torch.equal(both[-1], alone[0])
            n = len(plain)
            assert all(torch.equal(p, q) for p, q in zip(plain[1:n], both[1:n]))  # pixel_loss, tau, counts[, ce, region]
            if "region" not in cfg:
                assert torch.equal(both[4], plain[0].detach())  # loss_ce
            first = b.grad.clone()
            b.grad = None
            again = Fn.cross_entropy_select(b, labels, weight, return_parts=True, lovasz_weight=LW, **cfg)
            again[0].backward()
            assert all(torch.equal(p, q) for p, q in zip(both, again)) and torch.equal(b.grad, first)
            assert not torch.equal(both[0], plain[0].detach())  # (the term is there)
            twice = Fn.lovasz_softmax_loss(a.detach(), labels, return_parts=True)
            assert all(torch.equal(p, q) for p, q in zip(alone, twice))
            # misaligned logits: the same ranks (q is a function of the row, whichever kernel reads it)
            m, _, _ = on_device(x, t, shape, dtype, misaligned=True)
            mis = Fn.lovasz_softmax_loss(m.detach(), labels, return_parts=True)
            assert torch.equal(mis[2], alone[2]) and torch.equal(mis[1], alone[1])


# ---------------------------------------------------------------------------------------------------------------
# 6. edge cases
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [19, 64])
def test_edge_cases(C):
    Fn = F()
    x, t, w = make_case(SMALL, C, 5)
    dw = torch.from_numpy(w).to(DEV)
    logits, labels, seen = on_device(x, t, SMALL, torch.float32)
    # nothing valid: exactly 0 with an exactly zero gradient in both modes; the combined loss is NaN, as it is today
    none = torch.full_like(labels, 255)
    for classes in ("present", "all"):
        logits.grad = None
        loss, errors, rank, N, K = Fn.lovasz_softmax_loss(logits, none, classes, return_parts=True)
        loss.backward()
        assert float(loss.detach()) == 0.0 and not logits.grad.any() and int(K) == (C if classes == "all" else 0)
        assert not N.any() and bool((rank == -1).all()) and bool((errors == -1).all())
    assert math.isnan(float(Fn.cross_entropy_select(logits.detach(), none, dw, lovasz_weight=LW)))
    assert math.isnan(float(Fn.cross_entropy_select(logits.detach(), none, dw, lovasz_weight=LW, min_kept=5)))
    # labels >= C are not valid
    t2 = t.copy()
    t2[::7] = C + 3
    t2[3::11] = 254
    for label_dtype in (np.int64, np.uint8):
        _, lab2, _ = on_device(x, t2.astype(label_dtype), SMALL, torch.float32)
        _, E, _ = check_alone(logits, lab2, seen, t2, "present", torch.float32, "labels >= C")
        check_combined(logits, lab2, seen, t2, w, "all", E, torch.float32, "labels >= C", cfg={})
    assert not rows(logits.grad)[::7].any()
    # a single class present; a single valid pixel
    t3 = np.where(t == 255, 255, 2)
    _, lab3, _ = on_device(x, t3, SMALL, torch.float32)
    t4 = np.full_like(t, 255)
    t4[123] = 1
    _, lab4, _ = on_device(x, t4, SMALL, torch.float32)
    for classes in ("present", "all"):
        check_alone(logits, lab3, seen, t3, classes, torch.float32, "one class")
        check_alone(logits, lab4, seen, t4, classes, torch.float32, "one pixel")
    _, _, _, N, K = Fn.lovasz_softmax_loss(logits, lab3, return_parts=True)
    assert int(K) == 1 and int(N[2]) == int((t3 == 2).sum()) and int(N.sum()) == int(N[2])
    # classes="all" with exactly one absent class: its loss_c is the largest q_c over the valid pixels, by the formulas
    # alone.  C L_all - (C - 1) L_present is that loss_c; each fp32 loss is within 2e-6 relative, so the difference
    # is within 2e-6 (C L_all + (C - 1) L_present).
    t5 = np.where(t == 3, 4, t)
    _, lab5, _ = on_device(x, t5, SMALL, torch.float32)
    ref = L.evaluate(seen, t5, "all")
    v = ref["valid"]
    assert ref["N"][3] == 0 and (np.delete(ref["N"], 3) > 0).all()
    assert abs(ref["loss_c"][3] - ref["q"][v, 3].max()) <= 1e-15
    la = float(Fn.lovasz_softmax_loss(logits.detach(), lab5, "all"))
    lp = float(Fn.lovasz_softmax_loss(logits.detach(), lab5, "present"))
    assert abs((C * la - (C - 1) * lp) - ref["q"][v, 3].max()) <= 2e-6 * (C * la + (C - 1) * lp)
    # the in-place idiom of the reference's step
    from nas_segm_amd.nn import SegmCrossEntropy

    xa, _, _ = make_case(SMALL, C, 6)
    crit = SegmCrossEntropy(weight=torch.from_numpy(w), lovasz_weight=LW, **OHEM)
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
    alone = Fn.lovasz_softmax_loss(out.detach().requires_grad_(True), labels)
    alone += 0.15 * Fn.lovasz_softmax_loss(aux.detach(), labels)
    alone.backward()
    with pytest.raises(Fn.NassegError):
        Fn.lovasz_softmax_loss(out, labels[:, :-1])
    with pytest.raises(Fn.NassegError):
        Fn.lovasz_softmax_loss(out.cpu(), labels.cpu())
    with pytest.raises(Fn.NassegError):
        Fn.cross_entropy_select(out, labels[:, :-1], lovasz_weight=LW)
    with pytest.raises(Fn.NassegError, match="2 <= C"):  # (a single class has no softmax to speak of)
        Fn.lovasz_softmax_loss(out[:, :1].contiguous(memory_format=torch.channels_last), labels)
    with pytest.raises(Fn.NassegError):
        Fn.lovasz_from_errors(torch.zeros(4, 3, device=DEV), torch.zeros(5, dtype=torch.int64, device=DEV))
    with pytest.raises(Fn.NassegError):
        Fn.lovasz_from_errors(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64))


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


def test_graphed_segmenter_step_with_a_lovasz_term_equals_host_launches():
    from nas_segm_amd.engine.graphed import GraphedSegmenterStep
    from nas_segm_amd.engine.trainer import segmenter_step
    from nas_segm_amd.nn import SegmCrossEntropy

    batches = [dev_batch(b) for b in seg_batches(2, 42)]
    crit = SegmCrossEntropy(lovasz_weight=0.5, thresh=0.7, min_kept=50).prepare(DEV)

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


def test_graphed_task0_step_with_a_lovasz_term_equals_host_launches(monkeypatch):
    from nas_segm_amd.engine.graphed import GraphedTask0Step
    from nas_segm_amd.engine.trainer import make_task0_step, populate_task0
    from nas_segm_amd.nn import SegmCrossEntropy

    singles = [{"image": b["image"][i:i + 1], "mask": b["mask"][i:i + 1]} for b in seg_batches(2, 43) for i in range(2)]
    crit = SegmCrossEntropy(lovasz_weight=0.5, thresh=0.7, min_kept=50).prepare(DEV)
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


def test_a_changed_lovasz_weight_is_a_new_capture():
    from nas_segm_amd.engine.trainer import _segmenter_stepper, segmenter_step
    from nas_segm_amd.nn import SegmCrossEntropy

    batches = [dev_batch(b) for b in seg_batches(2, 44)]
    weights = (0.5, 2.0)

    def host(lws):
        crit = SegmCrossEntropy(lovasz_weight=lws[0]).prepare(DEV)
        net = fresh_net()
        oe, od = optimisers(net)
        out = []
        for (x, t), lw in zip(batches, lws):
            crit.lovasz_weight = lw
            out.append(float(segmenter_step(net, x, t, oe, od, 255, 3.0, 3.0, -1, segm_crit=crit)))
        return out

    want, unchanged = host(weights), host((weights[0], weights[0]))
    assert want[0] == unchanged[0] and want[1] != unchanged[1]
    crit = SegmCrossEntropy(lovasz_weight=weights[0]).prepare(DEV)
    net = fresh_net()
    oe, od = optimisers(net)
    args = (oe, od, 255, 3.0, 3.0, -1)
    first = _segmenter_stepper(net, batches[0][0], batches[0][1], *args, segm_crit=crit)
    assert first is not None and _segmenter_stepper(net, batches[0][0], batches[0][1], *args, segm_crit=crit) is first
    got = [float(first.step(*batches[0]))]
    crit.lovasz_weight = weights[1]
    second = _segmenter_stepper(net, batches[1][0], batches[1][1], *args, segm_crit=crit)
    assert second is not None and second is not first
    got.append(float(second.step(*batches[1])))
    assert got == want, (got, want)


def test_train_segmenter_epoch_with_a_lovasz_term(monkeypatch):
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

    with_term, sd1 = epoch(SegmCrossEntropy(lovasz_weight=0.5, thresh=0.7, min_kept=100))
    without, sd0 = epoch(SegmCrossEntropy(thresh=0.7, min_kept=100))
    assert len(with_term) == 2 and all(math.isfinite(v) and v > 0 for v in with_term), with_term
    assert with_term != without and with_term[0] > without[0]  # (a loss in (0, 1] was added)
    assert any(not torch.equal(sd0[k], sd1[k]) for k in sd0)
