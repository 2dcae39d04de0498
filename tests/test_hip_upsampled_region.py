"""The region-overlap term at the labels' size on the GPU (csrc/loss_up.hip: nasseg_ce_up_region_fwd / _bwd and their
row-indexed twins; F.cross_entropy_upsampled(region=...), F.region_overlap_loss_upsampled,
nn.SegmCrossEntropy(region_at="labels"), the engine's steps) against the float64 restatement
tests/_upsampled_region_ref.py, evaluated on the values the kernels read.

Bounds: every relative error (the losses; I and S over their largest entry; the gradient over its largest entry) must
not exceed the larger of the project's standing bound (2e-6; 1 / 128 for a gradient stored as bf16) and 4 x the error
of the same formulas in plain fp32 numpy (UR.upsampled_region_fp32) on the same input - computed per case, on the CPU,
before any launch.  Every measured value is printed before it is asserted."""
import math

import numpy as np
import pytest
import torch

import _region_loss_ref as R
import _upsampled_ce_ref as U
import _upsampled_region_ref as UR
from _util import build_product_net, load_json
from test_hip_upsampled_ce import GEOMETRY, OHEM, RAGGED, SEEDS, nhwc, on_device, wrap_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RW = 0.5  # region_weight of the combined cases


def F():
    from nas_segm_amd import functional

    return functional


def bits(t):
    """a floating tensor as integers: NaN == NaN, -0 != 0"""
    if not t.is_floating_point():
        return t
    t = t.detach().reshape(-1) if t.dim() == 0 else t.detach()
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def region_kw(params, region_weight=RW):
    region, smooth, classes = params
    return dict(region=region, region_weight=region_weight, region_smooth=smooth, region_classes=classes)


def ref_kw(params, region_weight=RW):
    region, smooth, classes = params
    return dict(region=region, region_weight=region_weight, smooth=smooth, classes=classes)


def rel(got, want):
    want = np.asarray(want, np.float64)
    scale = float(np.abs(want).max())
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    return err / scale if scale > 0 else err


def reference(seen, t, w, params, with_ce, sel, dtype, region_weight=RW, tag=""):
    """(float64 reference, bounds per quantity) - everything on the CPU, before any launch"""
    kw = ref_kw(params, region_weight)
    ref = UR.upsampled_region(seen, t, w, with_ce=with_ce, **dict(sel, **kw))
    if sel:
        gap = U.gap_to_tau(ref["ce"])
        assert gap >= 1e-4, "input unfit for this check: a loss lies {:.2e} from tau ({})".format(gap, tag)
    own = UR.upsampled_region_fp32(seen, t, ref["kept"], w, with_ce=with_ce, **kw)
    names = ["loss", "loss_region", "I", "S", "grad"] + (["loss_ce"] if with_ce else [])
    errs = {k: rel(own[k], ref[k]) for k in names}
    bound = {k: max(2e-6, 4.0 * e) for k, e in errs.items()}
    if dtype != torch.float32:
        bound["grad"] = max(1.0 / 128, bound["grad"])
    print(tag, "fp32 numpy:", {k: float("{:.2e}".format(v)) for k, v in errs.items()})
    return ref, bound


def launch(logits, labels, wt, params, with_ce, sel, region_weight=RW, rows=None, gscale=None):
    """one forward + backward -> dict of the outputs and the gradient tensor"""
    region, smooth, classes = params
    kw = {} if rows is None else {"rows": rows}
    logits.grad = None
    out = {}
    if with_ce:
        (out["loss"], out["pixel_loss"], out["tau"], out["counts"], out["loss_ce"],
         out["loss_region"]) = F().cross_entropy_upsampled(logits, labels, wt, return_parts=True,
                                                           **dict(sel, **region_kw(params, region_weight)), **kw)
        _, out["I"], out["S"], out["N"], out["K"] = F().region_overlap_loss_upsampled(
            logits.detach(), labels, region, smooth, classes, return_parts=True, **kw)
    else:
        out["loss"], out["I"], out["S"], out["N"], out["K"] = F().region_overlap_loss_upsampled(
            logits, labels, region, smooth, classes, return_parts=True, **kw)
    loss = out["loss"]
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (loss if gscale is None else gscale * loss).backward()
    out["grad"] = logits.grad
    assert logits.grad.dtype == logits.dtype and logits.grad.is_contiguous(memory_format=torch.channels_last)
    return out


def compare(out, ref, bound, with_ce, tag, region_weight=RW, gscale=None):
    """the outputs against the reference; the term alone returns region_weight = 1 times the term"""
    grad = nhwc(out["grad"]) / (1.0 if gscale is None else gscale)
    want = ref if with_ce else dict(ref, loss=ref["loss"] / region_weight, grad=ref["grad"] / region_weight)
    got = dict(loss=float(out["loss"].detach()), I=out["I"].cpu().numpy(), S=out["S"].cpu().numpy(), grad=grad)
    got["loss_region"] = float(out["loss_region"]) if with_ce else got["loss"]
    if with_ce:
        got["loss_ce"] = float(out["loss_ce"])
    errs = {k: rel(got[k], want[k]) for k in bound}
    print(tag, "errors", {k: float("{:.2e}".format(v)) for k, v in errs.items()}, "bounds",
          {k: float("{:.2e}".format(v)) for k, v in bound.items()})
    for k in bound:
        assert errs[k] <= bound[k], (tag, k, errs[k], bound[k])
    assert out["N"].dtype == torch.int64 and out["N"].cpu().tolist() == ref["N"].tolist()
    assert int(out["K"]) == int(ref["K"].sum())
    assert not grad[want["grad"] == 0].any()  # exact zeros where the reference has zeros
    if with_ce:
        ce = ref["ce"]
        assert out["counts"].cpu().tolist() == [ce["k"], ce["n"], ce["n_kept"]]
        pl = out["pixel_loss"].cpu().numpy().astype(np.float64)
        valid = ce["pixel_loss"] >= 0
        assert np.array_equal(pl < 0, ~valid) and (pl[~valid] == -1).all()
        assert float(np.abs(pl - ce["pixel_loss"])[valid].max()) <= 2e-5


def check(x, t, w, dtype, params, mode, tag, misaligned=False, gscale=None):
    """``mode``: "alone" (the term), "ce" (cross-entropy + term), "ohem" (with class weights and selection)"""
    logits, labels, seen = on_device(x, t, dtype, misaligned)
    with_ce = mode != "alone"
    sel = OHEM if mode == "ohem" else {}
    weight = w if mode == "ohem" else None
    ref, bound = reference(seen, t, weight, params, with_ce, sel, dtype, tag=tag)
    wt = None if weight is None else torch.from_numpy(weight).to(DEV)
    out = launch(logits, labels, wt, params, with_ce, sel, gscale=gscale)
    compare(out, ref, bound, with_ce, tag, gscale=gscale)
    return out, ref


# ---------------------------------------------------------------------------------------------------------------
# 1. against float64 at the smallest ragged shape; C = 64 | 65: one | two channel chunks of the backward
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label_dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [2, 19, 21, 64, 65])
def test_losses_sums_and_gradient_against_float64(C, dtype, label_dtype):
    x, t0, w = U.make_case(RAGGED[0], RAGGED[1], C, SEEDS[C], label_dtype=label_dtype)
    seen_K = set()
    for drop in (False, True):
        t = R.drop_odd_classes(t0).astype(label_dtype) if drop else t0
        for params in R.PARAM_SETS:
            for mode in ("alone", "ce", "ohem"):
                _, ref = check(x, t, w, dtype, params, mode, "C={} {} drop={} {} {}".format(C, dtype, drop, params, mode))
                seen_K.add(int(ref["K"].sum()))
    assert len(seen_K) >= 2 or C == 2  # (present and absent classes both occur)


# ---------------------------------------------------------------------------------------------------------------
# 2. factors and degenerate geometry
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_factors_and_degenerate_geometry(name):
    assert len(GEOMETRY) == 8
    lshape, tshape, seed = GEOMETRY[name]
    x, t, w = U.make_case(lshape, tshape, 19, seed)
    for mode in ("ce", "ohem"):
        check(x, t, w, torch.float32, R.PARAM_SETS[0], mode, "{} {}".format(name, mode))


# ---------------------------------------------------------------------------------------------------------------
# 3. equal sizes: the per-pixel and cross-entropy outputs are cross_entropy_select(region=)'s bits
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_equal_sizes_against_cross_entropy_select(dtype):
    x, t, w = U.make_case((2, 13, 17), (13, 17), 19, 0)
    wt = torch.from_numpy(w).to(DEV)
    params = R.PARAM_SETS[1]
    for sel in ({}, OHEM):
        tag = "identity {} {}".format(dtype, sorted(sel))
        logits, labels, seen = on_device(x, t, dtype)
        ref, bound = reference(seen, t, w, params, True, sel, dtype, tag=tag)
        out = launch(logits, labels, wt, params, True, sel)
        compare(out, ref, bound, True, tag)
        logits.grad = None
        l0, pl0, tau0, counts0, lce0, lreg0 = F().cross_entropy_select(logits, labels, wt, return_parts=True,
                                                                      **dict(sel, **region_kw(params)))
        _, I0, S0, N0, K0 = F().region_overlap_loss(logits.detach(), labels, *params, return_parts=True)
        l0.backward()
        assert same_bits(out["pixel_loss"], pl0) and torch.equal(out["counts"], counts0)
        assert same_bits(out["tau"], tau0) and same_bits(out["loss_ce"], lce0)
        assert torch.equal(out["N"], N0) and torch.equal(out["K"], K0)
        low = dict(loss=l0, loss_ce=lce0, loss_region=lreg0, I=I0, S=S0, N=N0, K=K0, grad=logits.grad, counts=counts0,
                   pixel_loss=pl0)
        compare(low, ref, bound, True, "cross_entropy_select on the same input")


# ---------------------------------------------------------------------------------------------------------------
# 4. bit-identities
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_the_cross_entropy_part_is_cross_entropy_upsampled_bit_for_bit(dtype):
    x, t, w = U.make_case((2, 9, 10), (20, 23), 19, 0)
    wt = torch.from_numpy(w).to(DEV)
    logits, labels, _ = on_device(x, t, dtype)
    for sel in ({}, OHEM):
        logits.grad = None
        l0, pl0, tau0, counts0 = F().cross_entropy_upsampled(logits, labels, wt, return_parts=True, **sel)
        l0.backward()
        g0 = logits.grad.clone()
        for params in R.PARAM_SETS[:2]:
            out = launch(logits, labels, wt, params, True, sel)
            assert same_bits(out["loss_ce"], l0) and same_bits(out["pixel_loss"], pl0)
            assert same_bits(out["tau"], tau0) and torch.equal(out["counts"], counts0)
            assert not same_bits(out["grad"], g0)
            zero = launch(logits, labels, wt, params, True, sel, region_weight=0.0)
            assert same_bits(zero["loss"], l0) and same_bits(zero["grad"], g0) and g0.any().item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [19, 21])
def test_misaligned_logits_and_a_second_run_give_the_same_bits(C, dtype):
    x, t, w = U.make_case((2, 9, 10), (20, 23), C, {19: 0, 21: 1}[C])
    wt = torch.from_numpy(w).to(DEV)
    runs = []
    for misaligned in (False, True, False):
        logits, labels, _ = on_device(x, t, dtype, misaligned)
        out = launch(logits, labels, wt, R.PARAM_SETS[0], True, OHEM)
        runs.append([out[k].detach().clone() for k in ("loss", "loss_ce", "loss_region", "pixel_loss", "tau", "counts",
                                                       "I", "S", "N", "grad")])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert same_bits(a, b)
    assert runs[0][-1].any().item()


# ---------------------------------------------------------------------------------------------------------------
# 5. images do not leak into each other
# ---------------------------------------------------------------------------------------------------------------
def test_ignored_images_and_batches():
    x, t, w = U.make_case((3, 5, 7), (19, 26), 19, 0)
    t[1] = 255
    out, _ = check(x, t, w, torch.float32, R.PARAM_SETS[0], "ohem", "middle image ignored")
    g = out["grad"]
    assert not g[1].any().item() and g[0].any().item() and g[2].any().item()
    t[:] = 255
    logits, labels, _ = on_device(x, t, torch.float32)
    wt = torch.from_numpy(w).to(DEV)
    out = launch(logits, labels, wt, R.PARAM_SETS[0], True, {})
    assert math.isnan(out["loss"].item()) and math.isnan(out["loss_ce"].item())  # (as the cross-entropy alone)
    assert out["counts"].cpu().tolist() == [0, 0, 0] and (out["pixel_loss"] == -1).all().item()
    assert out["loss_region"].item() == 0.0 and int(out["K"]) == 0 and not out["grad"].any().item()
    for params in R.PARAM_SETS[:2]:
        alone = launch(logits, labels, None, params, False, {})
        assert same_bits(alone["loss"], torch.zeros((), device=DEV)) and not alone["grad"].any().item()
        assert not alone["N"].any().item() and int(alone["K"]) == 0


def test_a_valid_pixel_the_selection_dropped_keeps_its_region_gradient():
    # equal sizes: a label pixel reaches its own logits pixel alone, so the dropped pixels' gradient is the term's
    x, t, w = U.make_case((1, 6, 5), (6, 5), 7, 1)
    sel = dict(thresh=0.7, min_kept=3)
    out, ref = check(x, t, w, torch.float32, R.PARAM_SETS[0], "ce", "no selection")
    logits, labels, seen = on_device(x, t, torch.float32)
    ref, bound = reference(seen, t, w, R.PARAM_SETS[0], True, sel, torch.float32, tag="dropped")
    out = launch(logits, labels, torch.from_numpy(w).to(DEV), R.PARAM_SETS[0], True, sel)
    compare(out, ref, bound, True, "dropped")
    dropped = (ref["ce"]["pixel_loss"] >= 0) & ~ref["ce"]["kept"]
    assert dropped.sum() >= 3 and ref["ce"]["kept"].sum() >= 3
    assert not ref["ce"]["grad"][dropped].any()  # (the cross-entropy gives them nothing)
    g = nhwc(out["grad"])[dropped]
    want = RW * ref["region"]["grad"][dropped]
    assert (np.abs(g).max(axis=1) > 0).all() and np.abs(want).max(axis=1).min() > 0
    assert np.abs(g - want).max() <= bound["grad"] * np.abs(ref["grad"]).max()


# ---------------------------------------------------------------------------------------------------------------
# 6. grid wrap (more than 1024 x 256 label pixels) and 17 x 17 ragged backward tiles
# ---------------------------------------------------------------------------------------------------------------
def test_grid_wrap_and_ragged_tiles():
    x, t, w = wrap_case()
    assert t.size > 1024 * 256
    logits, labels, seen = on_device(x, t, torch.float32)
    sel = dict(thresh=0.7, min_kept=100000)
    ref, bound = reference(seen, t, w, R.PARAM_SETS[1], True, sel, torch.float32, tag="grid wrap")
    assert ref["ce"]["n_kept"] >= 100000
    out = launch(logits, labels, torch.from_numpy(w).to(DEV), R.PARAM_SETS[1], True, sel)
    compare(out, ref, bound, True, "grid wrap")


# ---------------------------------------------------------------------------------------------------------------
# 7. rows: a label cache read in place
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("label_dtype", [np.uint8, np.int64])
def test_rows_give_the_bits_of_the_gathered_copy(label_dtype, dtype):
    x, cache_np, w = U.make_case((5, 5, 7), (19, 26), 19, 0, label_dtype=label_dtype)
    cache_np[2] = 255  # (a wholly ignored cache row, not in the table)
    x = x[:3]
    rows = torch.tensor([4, 0, 4], dtype=torch.int64, device=DEV)  # repeated and unordered
    logits, _, _ = on_device(x, cache_np[:3], dtype)
    cache = torch.from_numpy(cache_np).to(DEV)
    before = cache.clone()
    gathered = cache[rows].contiguous()
    wt = torch.from_numpy(w).to(DEV)
    for with_ce, sel in ((True, OHEM), (True, {}), (False, {})):
        a = launch(logits, cache, wt if with_ce else None, R.PARAM_SETS[0], with_ce, sel, rows=rows, gscale=2.5)
        a = {k: v.detach().clone() for k, v in a.items() if v is not None}
        b = launch(logits, gathered, wt if with_ce else None, R.PARAM_SETS[0], with_ce, sel, gscale=2.5)
        assert set(a) == set(b)
        for k in a:
            assert same_bits(a[k], b[k]), k
        assert a["grad"].any().item()
    assert torch.equal(cache, before)


# ---------------------------------------------------------------------------------------------------------------
# 8. upstream gradient and in-place use
# ---------------------------------------------------------------------------------------------------------------
def test_upstream_gradient_scales_and_heads_add_in_place():
    from nas_segm_amd.nn import SegmCrossEntropy

    x, t, w = U.make_case(RAGGED[0], RAGGED[1], 19, SEEDS[19])
    params = R.PARAM_SETS[1]
    check(x, t, w, torch.float32, params, "ohem", "3 * loss", gscale=3.0)
    xa, _, _ = U.make_case((2, 3, 4), RAGGED[1], 19, 0)
    crit = SegmCrossEntropy(weight=torch.from_numpy(w), full_size=True, region_at="labels",
                            **dict(OHEM, **region_kw(params))).prepare(DEV)
    main, labels, seen_m = on_device(x, t, torch.float32)
    aux, _, seen_a = on_device(xa, t, torch.float32)
    rm, bm = reference(seen_m, t, w, params, True, OHEM, torch.float32, tag="main")
    ra, ba = reference(seen_a, t, w, params, True, OHEM, torch.float32, tag="aux")
    loss = crit(main, labels)
    loss += 0.15 * crit(aux, labels)
    loss.backward()
    want = rm["loss"] + 0.15 * ra["loss"]
    assert abs(loss.item() - want) <= max(bm["loss"], ba["loss"]) * want
    for name, g, ref, bound, s in (("main", main.grad, rm, bm, 1.0), ("aux", aux.grad, ra, ba, 0.15)):
        gerr = rel(nhwc(g) / s, ref["grad"])
        print("in place", name, "grad/max", gerr, "bound", bound["grad"])
        assert gerr <= bound["grad"]


# ---------------------------------------------------------------------------------------------------------------
# 9. memory: nothing of B*H*W*C elements exists
# ---------------------------------------------------------------------------------------------------------------
def test_memory_contract():
    from nas_segm_amd._lib import lib

    def ws(*dims):
        return lib.query("nasseg_ce_up_region_workspace", *dims)

    plain = lib.query("nasseg_ce_up_workspace", 1, 5, 7, 19, 19, 26)
    for C in (2, 19, 21, 65):
        fixed = ws(1, 5, 7, C, 19, 26)
        # the cross-entropy's constant (to an even count) + fp64 [3][C][1024] rows + fp64 [3][C] totals
        assert fixed == plain + plain % 2 + 2 * (3 * C * 1024 + 3 * C)
        for dims in ((4, 256, 512, C, 1024, 2048), (16, 81, 81, C, 321, 321), (1, 64, 64, C, 512, 512)):
            assert ws(*dims) == fixed  # (independent of the pixel count)
    assert ws(1, 5, 7, 1, 19, 26) == 0  # (C >= 2)
    assert ws(1, 5, 7, 19, 65536, 65536) == 0  # (B H W < 2^32)
    assert ws(0, 5, 7, 19, 19, 26) == 0 and ws(1, 5, 7, 19, 0, 26) == 0
    assert ws(1, 2 ** 27 - 8, 1, 2, 4, 4) > 0 and ws(1, 2 ** 27, 1, 2, 4, 4) == 0  # (2^24 backward tiles)
    B, C, h, H = 1, 19, 64, 512
    x, t, w = U.make_case((B, h, h), (H, H), C, 0, 0.3, 0.5)
    logits, labels, _ = on_device(x, t, torch.float32)
    wt = torch.from_numpy(w).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = F().cross_entropy_upsampled(logits, labels, wt, thresh=0.7, min_kept=100000, region="dice")
    loss.backward()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print("peak growth", growth, "bytes; one up-sampled tensor", B * H * H * C * 4)
    assert growth < B * H * H * C * 4 // 2
    assert math.isfinite(loss.item()) and logits.grad.any().item()


# ---------------------------------------------------------------------------------------------------------------
# 10. engine: a small published net with auxiliary heads at 2 x 3 x 64 x 64
# ---------------------------------------------------------------------------------------------------------------
REC = load_json("nets_meta.json")["cvpr_arch1_search"]
AUX = 0.15
CRIT_KW = dict(region="dice", region_weight=0.5)


def seg_batches(n, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        mask = torch.randint(0, REC["classes"], (2, 64, 64), generator=g)
        mask[:, :6] = 255
        out.append({"image": torch.randn(2, 3, 64, 64, generator=g), "mask": mask})
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


def labels_crit():
    from nas_segm_amd.nn import SegmCrossEntropy

    return SegmCrossEntropy(full_size=True, region_at="labels", **CRIT_KW).prepare(DEV)


def by_hand(out, auxs, t):
    want = F().cross_entropy_upsampled(out, t, None, 255, **CRIT_KW)
    for a in auxs:
        want = want + F().cross_entropy_upsampled(a, t, None, 255, **CRIT_KW) * AUX
    return want


def test_host_step_is_the_loss_composed_by_hand():
    from nas_segm_amd.engine.trainer import segmenter_step

    x, t = dev_batch(seg_batches(1, 41)[0])
    net = fresh_net()
    out, auxs = net(x)
    assert len(auxs) >= 1 and tuple(out.shape[2:]) != tuple(t.shape[1:])
    want = by_hand(out, auxs, t)
    plain = F().cross_entropy_upsampled(out, t, None, 255)
    net = fresh_net()
    oe, od = optimisers(net)
    got = segmenter_step(net, x, t, oe, od, 255, 3.0, 3.0, AUX, segm_crit=labels_crit())
    assert math.isfinite(float(got)) and float(got) == float(want) and float(want) > float(plain)


def test_graphed_segmenter_step_equals_host_launches():
    from nas_segm_amd.engine.graphed import GraphedSegmenterStep
    from nas_segm_amd.engine.trainer import segmenter_step

    batches = [dev_batch(b) for b in seg_batches(2, 42)]
    crit = labels_crit()
    net = fresh_net()
    oe, od = optimisers(net)
    eager = [float(segmenter_step(net, x, t, oe, od, 255, 3.0, 3.0, AUX, segm_crit=crit)) for x, t in batches]
    sd0 = cpu_sd(net)
    net = fresh_net()
    oe, od = optimisers(net)
    stepper = GraphedSegmenterStep(net, batches[0][0], batches[0][1], oe, od, 255, 3.0, 3.0, AUX, segm_crit=crit)
    replayed = [float(stepper.step(x, t)) for x, t in batches]
    sd1 = cpu_sd(net)
    assert eager == replayed and all(math.isfinite(v) for v in eager), (eager, replayed)
    for k in sd0:  # parameters and BatchNorm buffers
        assert torch.equal(sd0[k], sd1[k]), k


def test_train_task0_replay_equals_host_launches_and_the_step_on_gathered_labels(monkeypatch):
    from nas_segm_amd.engine import trainer
    from nas_segm_amd.engine.trainer_common import cache_feature_keys, clip_and_step

    g = torch.Generator().manual_seed(31)
    samples = []
    for _ in range(6):
        mask = torch.randint(0, REC["classes"], (1, 64, 64), generator=g)
        mask[torch.rand(1, 64, 64, generator=g) < 0.2] = 255
        samples.append({"image": torch.randn(1, 3, 64, 64, generator=g), "mask": mask.to(torch.uint8)})
    crit = labels_crit()
    real = trainer._loss_value

    def adam(net):
        return torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)

    def go(mode):
        monkeypatch.setenv("NASSEG_GRAPH", mode)
        losses = []
        monkeypatch.setattr(trainer, "_loss_value", lambda s, loss: losses.append(real(s, loss)) or losses[-1])
        net = fresh_net()
        Xy = trainer.populate_task0.__wrapped__(net, samples, None, 6, full_size_labels=True)
        od = adam(net)
        np.random.seed(6)
        assert trainer.train_task0.__wrapped__(Xy, net, od, 0, crit, None, 2, False, False, 0.0, 3.0, False,
                                               aux_weight=AUX) is None
        return list(losses), cpu_sd(net)

    l0, sd0 = go("0")
    l1, sd1 = go("1")
    print("losses", l0, l1)
    assert len(l0) == 3 and l0 == l1 and all(math.isfinite(v) and v > 0 for v in l0), (l0, l1)
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k
    # by hand: the decoder on gathered features, the un-indexed loss on the GATHERED labels
    ref = fresh_net()
    Xr = trainer.populate_task0.__wrapped__(ref, samples, None, 6, full_size_labels=True)
    oref = adam(ref)
    ref.decoder.train()
    params = list(ref.decoder.parameters())
    np.random.seed(6)
    order = np.arange(6)
    np.random.shuffle(order)
    want = []
    for i in range(3):
        idx = torch.as_tensor(order[2 * i:2 * i + 2], dtype=torch.int64).to(DEV)
        out, aux_outs = ref.decoder([F().gather_rows(Xr[k], idx) for k in cache_feature_keys(Xr)])
        loss = by_hand(out, aux_outs, Xr["y_full"][idx])
        oref.zero_grad(set_to_none=True)
        loss.backward()
        clip_and_step([(params, 3.0, oref)])
        want.append(loss.item())
    assert l0 == want, (l0, want)
    sr = cpu_sd(ref.decoder)
    for k in sr:
        assert torch.equal(sd0["decoder." + k], sr[k]), k
