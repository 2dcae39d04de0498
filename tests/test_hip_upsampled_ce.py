"""The full-size cross-entropy on the GPU (csrc/loss_up.hip: nasseg_ce_up_fwd / _bwd; F.cross_entropy_upsampled,
nn.SegmCrossEntropy(full_size=True), the engine's steps) against the float64 restatement tests/_upsampled_ce_ref.py,
evaluated on the values the kernels read.

Bounds (1., 2., 5. - 7.): the loss's relative error and the gradient's error over max |gradient| must not exceed the
larger of the project's standing bound (2e-6; 1 / 128 for a gradient stored as bf16) and 4 x the error of the same
formulas in plain fp32 numpy (U.upsampled_fp32) on the same input - 4 for another order of summation over a footprint
of up to (2f + 2)^2 terms.  Every measured value is printed before it is asserted."""
import math

import numpy as np
import pytest
import torch

import _upsampled_ce_ref as U
from _util import build_product_net, load_json

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OHEM = dict(thresh=0.7, min_kept=50)


def F():
    from nas_segm_amd import functional

    return functional


def on_device(x, t, dtype, misaligned=False):
    """(logits (B, C, h, w) channels_last of ``dtype`` with requires_grad, labels (B, H, W), the logits' values as the
    kernels read them, float64 [B][h][w][C]).  ``misaligned``: the logits start one element into their buffer."""
    B, h, w, C = x.shape
    flat = torch.from_numpy(x).reshape(-1).to(DEV).to(dtype)
    if misaligned:
        buf = torch.empty(flat.numel() + 1, device=DEV, dtype=dtype)
        buf[1:].copy_(flat)
        flat = buf[1:]
        assert flat.data_ptr() % 16 != 0
    logits = flat.view(B, h, w, C).permute(0, 3, 1, 2).detach()
    assert logits.is_contiguous(memory_format=torch.channels_last)
    seen = logits.permute(0, 2, 3, 1).float().cpu().numpy().astype(np.float64)
    return logits.requires_grad_(True), torch.from_numpy(t).to(DEV), seen


def nhwc(grad):
    return grad.detach().permute(0, 2, 3, 1).float().cpu().numpy().astype(np.float64)


def grad_bound(dtype):
    return 2e-6 if dtype == torch.float32 else 1.0 / 128


def bounds(seen, t, w, ref, dtype):
    """(loss bound, gradient bound, the fp32 restatement's own two errors) on this input"""
    l32, g32, _ = U.upsampled_fp32(seen, t, ref["kept"], w)
    gmax = float(np.abs(ref["grad"]).max())
    own_l = abs(l32 - ref["loss"]) / abs(ref["loss"])
    own_g = float(np.abs(g32 - ref["grad"]).max()) / gmax
    return max(2e-6, 4.0 * own_l), max(grad_bound(dtype), 4.0 * own_g), own_l, own_g


def compare(loss, grad, ref, lb, gb, tag):
    gmax = float(np.abs(ref["grad"]).max())
    lerr = abs(float(loss.detach()) - ref["loss"]) / abs(ref["loss"])
    gerr = float(np.abs(grad - ref["grad"]).max()) / gmax
    print(tag, "loss rel", lerr, "bound", lb, "grad/max", gerr, "bound", gb)
    assert lerr <= lb and gerr <= gb
    assert not grad[ref["grad"] == 0].any()  # exact zeros where the reference has zeros
    return lerr, gerr


def check(x, t, w, dtype, cfg, tag, misaligned=False, gscale=None):
    """forward + backward of F.cross_entropy_upsampled against float64; returns (loss, pixel_loss, grad tensor, ref)"""
    logits, labels, seen = on_device(x, t, dtype, misaligned)
    ref = U.upsampled(seen, t, w, **cfg)
    if cfg:  # (on the CPU, before any launch)
        gap = U.gap_to_tau(ref)
        assert gap >= 1e-4, "input unfit for this check: a loss lies {:.2e} from tau ({})".format(gap, tag)
    assert math.isfinite(ref["loss"]) and ref["n_kept"] >= 1, tag
    lb, gb, own_l, own_g = bounds(seen, t, w, ref, dtype)
    print(tag, "fp32 numpy: loss rel", own_l, "grad/max", own_g)
    wt = None if w is None else torch.from_numpy(w).to(DEV)
    loss, pl, tau, counts = F().cross_entropy_upsampled(logits, labels, wt, return_parts=True, **cfg)
    (loss if gscale is None else gscale * loss).backward()
    assert loss.dim() == 0 and loss.dtype == torch.float32 and pl.dtype == torch.float32
    assert tuple(pl.shape) == tuple(t.shape) and counts.dtype == torch.int64
    assert counts.cpu().tolist() == [ref["k"], ref["n"], ref["n_kept"]]
    assert logits.grad.dtype == dtype and logits.grad.is_contiguous(memory_format=torch.channels_last)
    pln = pl.cpu().numpy().astype(np.float64)
    valid = ref["pixel_loss"] >= 0
    assert np.array_equal(pln < 0, ~valid) and (pln[~valid] == -1).all()
    perr = float(np.abs(pln - ref["pixel_loss"])[valid].max())
    print(tag, "pixel_loss abs", perr)
    assert perr <= 2e-5  # (a few fp32 roundings of values below 32)
    if cfg and ref["tau"] < U.CE.t_loss_of(cfg.get("thresh")):
        assert abs(float(tau) - ref["tau"]) <= 2e-5
    grad = nhwc(logits.grad)
    if gscale is not None:
        grad = grad / gscale
    compare(loss, grad, ref, lb, gb, tag)
    return loss.detach(), pl, logits.grad, ref


# ---------------------------------------------------------------------------------------------------------------
# 1. against float64 at the smallest ragged shape: factors 3.8 and 3.71.  C = 64 | 65: one | two channel chunks of
# the backward (kUpChunk = 64).  SEEDS: seeds of U.make_case at which, for both storage types, no valid float64 loss
# lies within 1e-4 of tau under OHEM except those equal to it (asserted in check, on the CPU, before any launch)
# ---------------------------------------------------------------------------------------------------------------
RAGGED = ((2, 5, 7), (19, 26))
SEEDS = {2: 0, 19: 0, 21: 0, 64: 0, 65: 0}


@pytest.mark.parametrize("label_dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [2, 19, 21, 64, 65])
def test_loss_and_gradient_against_float64(C, dtype, label_dtype):
    x, t, w = U.make_case(RAGGED[0], RAGGED[1], C, SEEDS[C], label_dtype=label_dtype)
    for cfg in ({}, OHEM):
        for weight in (w, None):
            check(x, t, weight, dtype, cfg, "C={} {} {} weights={}".format(C, dtype, sorted(cfg), weight is not None))


# ---------------------------------------------------------------------------------------------------------------
# 2. factors and degenerate geometry
# ---------------------------------------------------------------------------------------------------------------
GEOMETRY = {
    "integer 4": ((1, 8, 16), (32, 64), 0),
    "integer 8": ((1, 4, 8), (32, 64), 0),
    "integer 16": ((1, 3, 5), (48, 80), 0),
    "down": ((1, 9, 11), (4, 5), 0),
    "up in y, down in x": ((1, 3, 12), (11, 5), 0),
    "one logit": ((1, 1, 1), (7, 9), 2),
    "one label": ((1, 4, 6), (1, 1), 0),
    "one row": ((1, 1, 6), (5, 23), 0),
}


@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_factors_and_degenerate_geometry(name):
    lshape, tshape, seed = GEOMETRY[name]
    x, t, w = U.make_case(lshape, tshape, 19, seed)
    for cfg in ({}, OHEM):
        _, _, grad, ref = check(x, t, w, torch.float32, cfg, "{} {}".format(name, sorted(cfg)))
    if name == "down":  # logits no label pixel touches: exact zeros, and they are the reference's
        untouched = ~(U.weight_matrix(U.coeffs(4, 9), 9).any(axis=0)[:, None] &
                      U.weight_matrix(U.coeffs(5, 11), 11).any(axis=0))
        g = nhwc(grad)[0]
        assert untouched.any() and not g[untouched].any() and not ref["grad"][0][untouched].any()
        assert g[~untouched].any()


# ---------------------------------------------------------------------------------------------------------------
# 3. equal sizes are the identity
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_equal_sizes_are_cross_entropy_select(dtype):
    x, t, w = U.make_case((2, 13, 17), (13, 17), 19, 0)
    wt = torch.from_numpy(w).to(DEV)
    for cfg in ({}, OHEM):
        loss, pl, grad, ref = check(x, t, w, dtype, cfg, "identity {} {}".format(dtype, sorted(cfg)))
        logits, labels, _ = on_device(x, t, dtype)
        _, _, tau, counts = F().cross_entropy_upsampled(logits, labels, wt, return_parts=True, **cfg)
        l0, pl0, tau0, counts0 = F().cross_entropy_select(logits, labels, wt, return_parts=True, **cfg)
        assert torch.equal(pl, pl0) and torch.equal(counts, counts0)
        assert torch.equal(tau.view(1).view(torch.int32), tau0.view(1).view(torch.int32))
        l0.backward()
        lb, gb, _, _ = bounds(nhwc(logits.detach()), t, w, ref, dtype)
        compare(l0.detach(), nhwc(logits.grad), ref, lb, gb, "cross_entropy_select on the same input")


# ---------------------------------------------------------------------------------------------------------------
# 4. images do not leak into each other
# ---------------------------------------------------------------------------------------------------------------
def test_an_ignored_image_gets_exact_zeros_and_an_ignored_batch_a_nan_loss():
    x, t, w = U.make_case((3, 5, 7), (19, 26), 19, 0)
    t[1] = 255
    _, _, grad, _ = check(x, t, w, torch.float32, OHEM, "middle image ignored")
    assert not grad[1].any().item() and grad[0].any().item() and grad[2].any().item()
    t[:] = 255
    logits, labels, _ = on_device(x, t, torch.float32)
    loss, pl, tau, counts = F().cross_entropy_upsampled(logits, labels, torch.from_numpy(w).to(DEV), return_parts=True)
    loss.backward()
    assert math.isnan(loss.item()) and counts.cpu().tolist() == [0, 0, 0] and (pl == -1).all().item()
    assert not logits.grad.any().item()
    import torch.nn.functional as TF

    assert math.isnan(TF.cross_entropy(torch.zeros(1, 19, 2, 2), torch.full((1, 2, 2), 255), ignore_index=255).item())


# ---------------------------------------------------------------------------------------------------------------
# 5. tile and grid edges.  The launchers' caps and tiles (csrc/loss_up.hip): the forward and the sum pass run at most
# kUpGridCap = 1024 workgroups of 256 label pixels and wrap beyond 262,144 of them - 515 x 521 = 268,315; the backward
# owns tiles of kUpTile = 8 x 8 logits pixels - 130 x 131 logits: 17 x 17 tiles, the last of each axis 2 and 3 pixels
# wide - and chunks of kUpChunk = 64 channels - C = 65 over more than one tile and more than one image below.
# ---------------------------------------------------------------------------------------------------------------
# With a quarter of a million losses no threshold keeps 1e-4 away from all of them unless the input leaves a hole
# there: small logits (scale 0.3), channel 7 raised by 6 everywhere and half of the valid labels set to 7 - those
# pixels lose about 0.04, all others about 6, and tau = -log(0.7) falls between the two.
def wrap_case():
    x, t, w = U.make_case((1, 130, 131), (515, 521), 19, 0, 0.3, 0.0)
    x[..., 7] += np.float32(6.0)
    rng = np.random.RandomState(1)
    t[(rng.rand(*t.shape) < 0.5) & (t != 255)] = 7
    return x, t, w


def test_grid_wrap_and_ragged_tiles():
    x, t, w = wrap_case()
    assert t.size > 1024 * 256
    _, _, _, ref = check(x, t, w, torch.float32, dict(thresh=0.7, min_kept=100000), "grid wrap")
    assert ref["n_kept"] >= 100000


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_channel_chunks_over_ragged_tiles_and_images(dtype):
    x, t, w = U.make_case((2, 9, 10), (20, 23), 65, 0)
    check(x, t, w, dtype, OHEM, "C=65 two chunks {}".format(dtype))


# ---------------------------------------------------------------------------------------------------------------
# 6. misaligned logits: the patch is staged element by element instead of in 16-byte vectors - the same numbers
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [19, 21])
def test_misaligned_logits_take_the_generic_staging(C, dtype):
    x, t, w = U.make_case((2, 9, 10), (20, 23), C, {19: 0, 21: 1}[C])
    l0, pl0, g0, _ = check(x, t, w, dtype, OHEM, "aligned C={} {}".format(C, dtype))
    l1, pl1, g1, _ = check(x, t, w, dtype, OHEM, "misaligned C={} {}".format(C, dtype), misaligned=True)
    assert torch.equal(l0, l1) and torch.equal(pl0, pl1) and torch.equal(g0, g1)


# ---------------------------------------------------------------------------------------------------------------
# 7. upstream gradient and in-place use
# ---------------------------------------------------------------------------------------------------------------
def test_upstream_gradient_scales_and_heads_add_in_place():
    from nas_segm_amd.nn import SegmCrossEntropy

    x, t, w = U.make_case(RAGGED[0], RAGGED[1], 19, SEEDS[19])
    check(x, t, w, torch.float32, OHEM, "3 * loss", gscale=3.0)
    xa, _, _ = U.make_case((2, 3, 4), RAGGED[1], 19, 0)
    crit = SegmCrossEntropy(weight=torch.from_numpy(w), full_size=True, **OHEM).prepare(DEV)
    main, labels, seen_m = on_device(x, t, torch.float32)
    aux, _, seen_a = on_device(xa, t, torch.float32)
    loss = crit(main, labels)
    loss += 0.15 * crit(aux, labels)
    loss.backward()
    rm, ra = U.upsampled(seen_m, t, w, **OHEM), U.upsampled(seen_a, t, w, **OHEM)
    assert U.gap_to_tau(rm) >= 1e-4 and U.gap_to_tau(ra) >= 1e-4
    assert abs(loss.item() - (rm["loss"] + 0.15 * ra["loss"])) <= 2e-6 * (rm["loss"] + 0.15 * ra["loss"])
    for name, g, ref, seen, s in (("main", main.grad, rm, seen_m, 1.0), ("aux", aux.grad, ra, seen_a, 0.15)):
        _, gb, _, _ = bounds(seen, t, w, ref, torch.float32)
        gerr = float(np.abs(nhwc(g) / s - ref["grad"]).max()) / float(np.abs(ref["grad"]).max())
        print("in place", name, "grad/max", gerr, "bound", gb)
        assert gerr <= gb


# ---------------------------------------------------------------------------------------------------------------
# 8. reproducibility
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_runs_are_bit_identical(dtype):
    x, t, w = U.make_case((2, 20, 27), (77, 101), 19, 2)
    logits, labels, _ = on_device(x, t, dtype)
    wt = torch.from_numpy(w).to(DEV)
    runs = []
    for _ in range(2):
        logits.grad = None
        loss, pl, tau, counts = F().cross_entropy_upsampled(logits, labels, wt, return_parts=True, **OHEM)
        loss.backward()
        runs.append((loss.detach().clone().view(1).view(torch.int32), pl.view(torch.int32).clone(),
                     tau.clone().view(1).view(torch.int32), counts.clone(), logits.grad.clone().view(
                         torch.int32 if dtype == torch.float32 else torch.int16)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert runs[0][4].any().item()


# ---------------------------------------------------------------------------------------------------------------
# 9. memory: nothing of B*H*W*C elements exists
# ---------------------------------------------------------------------------------------------------------------
def test_memory_contract():
    from nas_segm_amd._lib import lib

    fixed = lib.query("nasseg_ce_up_workspace", 1, 5, 7, 19, 19, 26)
    assert fixed == 3 * 1024 + lib.query("nasseg_ohem_workspace") and fixed < 16384
    # the workspace depends on the grid alone: with the two per-pixel arrays that is 2 B H W floats + a constant
    for dims in ((4, 256, 512, 19, 1024, 2048), (16, 81, 81, 21, 321, 321), (1, 64, 64, 19, 512, 512)):
        assert lib.query("nasseg_ce_up_workspace", *dims) == fixed
    assert lib.query("nasseg_ce_up_workspace", 1, 5, 7, 1, 19, 26) == 0  # (C >= 2)
    assert lib.query("nasseg_ce_up_workspace", 1, 5, 7, 19, 65536, 65536) == 0  # (B H W < 2^32)
    # the backward launches one workgroup per 8 x 8 tile and 64 channels, fewer than 2^24 of them: a map one pixel wide
    # reaches that at h = 2^27 with B h w C = 2^28 still inside its own limit
    assert lib.query("nasseg_ce_up_workspace", 1, 2 ** 27 - 8, 1, 2, 4, 4) == fixed
    assert lib.query("nasseg_ce_up_workspace", 1, 2 ** 27, 1, 2, 4, 4) == 0
    B, C, h, H = 1, 19, 64, 512
    x, t, w = U.make_case((B, h, h), (H, H), C, 0, 0.3, 0.5)
    logits, labels, _ = on_device(x, t, torch.float32)
    wt = torch.from_numpy(w).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = F().cross_entropy_upsampled(logits, labels, wt, thresh=0.7, min_kept=100000)
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


def full_crit():
    from nas_segm_amd.nn import SegmCrossEntropy

    return SegmCrossEntropy(full_size=True, thresh=0.7, min_kept=500).prepare(DEV)


def test_host_step_is_the_loss_composed_by_hand():
    from nas_segm_amd.engine.trainer import segmenter_step

    x, t = dev_batch(seg_batches(1, 41)[0])
    net = fresh_net()
    out, auxs = net(x)
    assert len(auxs) >= 1 and tuple(out.shape[2:]) != tuple(t.shape[1:])
    want = F().cross_entropy_upsampled(out, t, None, 255, 0.7, 500)
    for a in auxs:
        want = want + F().cross_entropy_upsampled(a, t, None, 255, 0.7, 500) * AUX
    net = fresh_net()
    oe, od = optimisers(net)
    got = segmenter_step(net, x, t, oe, od, 255, 3.0, 3.0, AUX, segm_crit=full_crit())
    assert math.isfinite(float(got)) and float(got) == float(want)
    net = fresh_net()
    oe, od = optimisers(net)
    from nas_segm_amd.nn import SegmCrossEntropy

    low = SegmCrossEntropy(thresh=0.7, min_kept=500).prepare(DEV)
    assert float(segmenter_step(net, x, t, oe, od, 255, 3.0, 3.0, AUX, segm_crit=low)) != float(got)


def test_graphed_segmenter_step_with_a_full_size_criterion_equals_host_launches():
    from nas_segm_amd.engine.graphed import GraphedSegmenterStep
    from nas_segm_amd.engine.trainer import segmenter_step

    batches = [dev_batch(b) for b in seg_batches(2, 42)]
    crit = full_crit()
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


def test_a_changed_full_size_is_a_new_capture():
    from nas_segm_amd.engine.trainer import _segmenter_stepper, segmenter_step

    batches = [dev_batch(b) for b in seg_batches(2, 44)]

    def host(flags):
        crit = full_crit()
        net = fresh_net()
        oe, od = optimisers(net)
        out = []
        for (x, t), flag in zip(batches, flags):
            crit.full_size = flag
            out.append(float(segmenter_step(net, x, t, oe, od, 255, 3.0, 3.0, AUX, segm_crit=crit)))
        return out

    want, unchanged = host((True, False)), host((True, True))
    assert want[0] == unchanged[0] and want[1] != unchanged[1]
    crit = full_crit()
    net = fresh_net()
    oe, od = optimisers(net)
    args = (oe, od, 255, 3.0, 3.0, AUX)
    first = _segmenter_stepper(net, batches[0][0], batches[0][1], *args, segm_crit=crit)
    assert first is not None and _segmenter_stepper(net, batches[0][0], batches[0][1], *args, segm_crit=crit) is first
    got = [float(first.step(*batches[0]))]
    crit.full_size = False
    second = _segmenter_stepper(net, batches[1][0], batches[1][1], *args, segm_crit=crit)
    assert second is not None and second is not first
    got.append(float(second.step(*batches[1])))
    assert got == want, (got, want)


def test_train_segmenter_epoch_with_a_full_size_criterion(monkeypatch):
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
                                                   print_every=100, aux_weight=AUX) is None
        return list(losses), cpu_sd(net)

    full, sd1 = epoch(SegmCrossEntropy(full_size=True, thresh=0.7, min_kept=500))
    low, sd0 = epoch(SegmCrossEntropy(thresh=0.7, min_kept=500))
    assert len(full) == 2 and all(math.isfinite(v) and v > 0 for v in full), full
    assert full != low and any(not torch.equal(sd0[k], sd1[k]) for k in sd0)
