"""The depth path on the GPU: masked berHu against a full-size target with holes (F.berhu_loss_masked,
nn.BerHuLoss), the fused depth metrics (F.depth_metrics) and the engine entry points built on them (train_segmenter
with a BerHuLoss, validate_depth, evaluate_candidate(task="depth")).

Nothing of this exists in the reference (its depth networks are inference only): parity is "unpinned", the
yardsticks are torch on the CPU and float64 numpy, written out here."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from _util import assert_close, build_product_net, load_json

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = [(2, 33, 47, 101, 75), (1, 17, 23, 17, 23), (3, 60, 80, 240, 320), (8, 120, 160, 480, 640)]
MIN_DEPTH, MAX_DEPTH = 1e-3, 10.0


def make_inputs(B, h, w, H, W, seed=7):
    """pred in [0.3, 10), gt in [0, 10) with 10 % holes (0), every 997th pixel NaN and every 1013th (from 5) +inf"""
    g = torch.Generator().manual_seed(seed)
    pred = 0.3 + 9.7 * torch.rand(B, 1, h, w, generator=g)
    gt = 10 * torch.rand(B, H, W, generator=g)
    gt[torch.rand(B, H, W, generator=g) < 0.1] = 0.0
    flat = gt.view(-1)
    flat[::997] = float("nan")
    flat[5::1013] = float("inf")
    return pred, gt


def F():
    from nas_segm_amd import functional

    return functional


# ---------------------------------------------------------------------------------------------------------------
# 1. metrics kernel against float64
# ---------------------------------------------------------------------------------------------------------------
def reference_sums(pred, gt, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH):
    """fp32 bilinear up-sampling on the CPU, then every term in numpy float64 -> (sums[8], sums of |terms|[8],
    counts[3], band): band = valid pixels whose ratio lies within 1e-5 relative of one of the thresholds"""
    H, W = gt.shape[1:]
    up = TF.interpolate(pred.float(), size=(H, W), mode="bilinear", align_corners=False)[:, 0].numpy()
    g = gt.numpy()
    valid = np.isfinite(g) & (g > np.float32(min_depth)) & (g <= np.float32(max_depth))
    p = np.clip(up, np.float32(min_depth), np.float32(max_depth))[valid].astype(np.float64)
    g = g[valid].astype(np.float64)
    ln = np.log(p) - np.log(g)
    terms = [np.ones_like(p), np.abs(p - g), (p - g) ** 2, np.abs(p - g) / g, (p - g) ** 2 / g,
             np.abs(np.log10(p) - np.log10(g)), ln, ln ** 2]
    ratio = np.maximum(p / g, g / p)
    thr = [1.25, 1.25 ** 2, 1.25 ** 3]
    counts = [int((ratio < t).sum()) for t in thr]
    near = np.zeros(p.shape, dtype=bool)
    for t in thr:
        near |= np.abs(ratio / t - 1.0) <= 1e-5
    return ([float(t.sum()) for t in terms], [float(np.abs(t).sum()) for t in terms], counts, int(near.sum()))


@pytest.mark.parametrize("case", CASES)
def test_depth_metrics_against_float64(case):
    B, h, w, H, W = case
    pred, gt = make_inputs(*case)
    sums, abs_sums, counts, band = reference_sums(pred, gt)
    n = sums[0]
    acc = F().depth_metrics(pred.to(DEV), gt.to(DEV), MIN_DEPTH, MAX_DEPTH)
    assert acc.dtype == torch.float64 and tuple(acc.shape) == (12,) and acc.is_cuda
    got = acc.cpu().numpy()
    identity = (h, w) == (H, W)
    print("case", case, "n", n, "band", band)
    for k in range(8):
        err = abs(got[k] - sums[k])
        print("  sum", k, got[k], sums[k], "rel to |terms|", err / max(abs_sums[k], 1e-300))
    for k in range(3):
        print("  count", k, got[8 + k], counts[k])
    assert got[0] == n and n > 0.8 * B * H * W
    assert band <= 1e-4 * n  # (so that the band cannot hide a failure)
    for k in range(8):
        assert abs(got[k] - sums[k]) <= (1e-9 if identity else 2e-6) * abs_sums[k], (k, got[k], sums[k])
    for k in range(3):
        assert abs(got[8 + k] - counts[k]) <= (0 if identity else band), (k, got[8 + k], counts[k], band)
    assert got[11] == 0.0


def test_depth_metrics_storage_stride_accumulation_and_reproducibility():
    Fn = F()
    case = (2, 33, 47, 101, 75)
    pred, gt = make_inputs(*case)
    gt_d = gt.to(DEV)
    # bf16 storage == the same call on its fp32 widening, bit for bit
    pb = pred.to(torch.bfloat16)
    a_bf = Fn.depth_metrics(pb.to(DEV), gt_d, MIN_DEPTH, MAX_DEPTH)
    a_wide = Fn.depth_metrics(pb.float().to(DEV), gt_d, MIN_DEPTH, MAX_DEPTH)
    assert torch.equal(a_bf, a_wide)
    # channel 0 of a 4-channel NHWC map (pixel stride 4) == the one-channel call, bit for bit - both storages
    one = Fn.depth_metrics(pred.to(DEV), gt_d, MIN_DEPTH, MAX_DEPTH)
    g = torch.Generator().manual_seed(3)
    four = torch.cat([pred, torch.randn(2, 3, 33, 47, generator=g)], 1).contiguous(memory_format=torch.channels_last)
    assert torch.equal(Fn.depth_metrics(four.to(DEV), gt_d, MIN_DEPTH, MAX_DEPTH), one)
    assert torch.equal(Fn.depth_metrics(four.to(torch.bfloat16).to(DEV), gt_d, MIN_DEPTH, MAX_DEPTH), a_bf)
    # the same call twice: identical bits
    assert torch.equal(Fn.depth_metrics(pred.to(DEV), gt_d, MIN_DEPTH, MAX_DEPTH), one)
    # two calls into one accumulator == one call on the concatenated batch
    pred2, gt2 = make_inputs(*case, seed=8)
    acc = Fn.depth_metrics(pred.to(DEV), gt_d, MIN_DEPTH, MAX_DEPTH)
    ret = Fn.depth_metrics(pred2.to(DEV), gt2.to(DEV), MIN_DEPTH, MAX_DEPTH, acc=acc)
    assert ret is acc
    both = Fn.depth_metrics(torch.cat([pred, pred2]).to(DEV), torch.cat([gt, gt2]).to(DEV), MIN_DEPTH, MAX_DEPTH)
    a, b = acc.cpu().numpy(), both.cpu().numpy()
    assert np.all(np.abs(a - b) <= 1e-12 * np.abs(b)), (a, b)
    assert a[0] == b[0] and np.array_equal(a[8:11], b[8:11])
    # a ground truth without a valid pixel leaves the accumulator as it was (slot 11 is never written)
    before = torch.arange(1, 13, dtype=torch.float64).to(DEV) * 1.5
    acc = before.clone()
    empty = torch.zeros(2, 101, 75)
    empty.view(-1)[::3] = float("nan")
    empty.view(-1)[1::3] = float("inf")
    empty.view(-1)[2::7] = 11.0  # (beyond max_depth)
    Fn.depth_metrics(pred.to(DEV), empty.to(DEV), MIN_DEPTH, MAX_DEPTH, acc=acc)
    assert torch.equal(acc, before)
    Fn.depth_metrics(pred.to(DEV), gt_d, MIN_DEPTH, MAX_DEPTH, acc=acc)
    assert float(acc[11]) == float(before[11]) and float(acc[0]) == float(before[0]) + float(one[0])
    # min_depth <= 0: refused before any launch
    for bad in (0.0, -1.0):
        acc = before.clone()
        with pytest.raises(RuntimeError):
            Fn.depth_metrics(pred.to(DEV), gt_d, bad, MAX_DEPTH, acc=acc)
        torch.cuda.synchronize()
        assert torch.equal(acc, before)
    # predictions outside [min_depth, max_depth] are clamped: any two constants far above score alike
    hi = Fn.depth_metrics(torch.full((2, 1, 33, 47), 50.0).to(DEV), gt_d, MIN_DEPTH, MAX_DEPTH)
    at = Fn.depth_metrics(torch.full((2, 1, 33, 47), 20.0).to(DEV), gt_d, MIN_DEPTH, MAX_DEPTH)
    assert torch.equal(hi, at) and float(hi[0]) == float(one[0])
    lo = Fn.depth_metrics(torch.full((2, 1, 33, 47), -3.0).to(DEV), gt_d, MIN_DEPTH, MAX_DEPTH)
    assert bool(torch.isfinite(lo).all())


# ---------------------------------------------------------------------------------------------------------------
# 2. masked berHu against torch CPU autograd
# ---------------------------------------------------------------------------------------------------------------
def reference_masked_berhu(pred, gt, valid_min=0.0, valid_max=float("inf")):
    """(loss, validity mask at the prediction's size): nearest-resized target, mask, c = 0.2 max d (detached),
    mean over valid pixels"""
    t = TF.interpolate(gt[:, None], size=tuple(pred.shape[2:]), mode="nearest")
    valid = torch.isfinite(t) & (t > valid_min) & (t <= valid_max)
    if not bool(valid.any()):
        return pred.sum() * 0.0, valid
    d = (pred[valid] - t[valid]).abs()
    c = 0.2 * d.max().detach()
    return torch.where(d <= c, d, (d * d + c * c) / (2 * c)).mean(), valid


@pytest.mark.parametrize("case", CASES)
def test_masked_berhu_against_torch_autograd(case):
    pred, gt = make_inputs(*case)
    pc = pred.clone().requires_grad_(True)
    ref, valid = reference_masked_berhu(pc, gt)
    pg = pred.clone().to(DEV).requires_grad_(True)
    out = F().berhu_loss_masked(pg, gt.to(DEV))
    assert out.dim() == 0 and out.dtype == torch.float32
    got, want = float(out.detach()), float(ref.detach())
    print("case", case, "loss", got, "ref", want, "valid", int(valid.sum()), "of", valid.numel())
    assert abs(got - want) < 1e-5 * max(1.0, abs(want))
    (ref * 1.3).backward()
    (out * 1.3).backward()
    assert_close(pg.grad, pc.grad, 1e-7, 1e-4, "dpred")
    assert 0 < int((~valid).sum()) and float(pg.grad.cpu()[~valid].abs().max()) == 0.0
    # through the criterion module: the same bits
    from nas_segm_amd.nn import BerHuLoss

    assert float(BerHuLoss()(pred.to(DEV), gt.to(DEV))) == float(out)
    # a tighter valid range is honoured (targets above 5 become holes)
    ref5, valid5 = reference_masked_berhu(pred, gt, 0.0, 5.0)
    out5 = BerHuLoss(valid_min=0.0, valid_max=5.0)(pred.to(DEV), gt.to(DEV))
    assert int(valid5.sum()) < int(valid.sum())
    assert abs(float(out5) - float(ref5)) < 1e-5 * max(1.0, abs(float(ref5)))


@pytest.mark.parametrize("case", CASES)
def test_masked_berhu_bf16_predictions(case):
    pred, gt = make_inputs(*case)
    pb = pred.to(torch.bfloat16)
    pc = pb.float().requires_grad_(True)
    ref, valid = reference_masked_berhu(pc, gt)
    pg = pb.to(DEV).requires_grad_(True)
    out = F().berhu_loss_masked(pg, gt.to(DEV))
    assert abs(float(out) - float(ref)) < 1e-5 * max(1.0, abs(float(ref)))
    ref.backward()
    out.backward()
    assert pg.grad.dtype == torch.bfloat16
    got = pg.grad.cpu().view(torch.int16).to(torch.int32)
    want = pc.grad.to(torch.bfloat16).view(torch.int16).to(torch.int32)
    assert int((got - want).abs().max()) <= 1  # (at most one bf16 ulp apart)
    assert float(pg.grad.float().cpu()[~valid].abs().max()) == 0.0


def test_masked_berhu_edge_cases_and_in_place_use():
    Fn = F()
    pred, gt = make_inputs(2, 33, 47, 101, 75)
    # no valid pixel: loss 0, gradient 0, no NaN
    holes = torch.zeros(2, 101, 75)
    holes.view(-1)[::2] = float("nan")
    holes.view(-1)[1::4] = float("inf")
    holes.view(-1)[3::4] = -1.0
    for dtype in (torch.float32, torch.bfloat16):
        pg = pred.to(dtype).to(DEV).requires_grad_(True)
        out = Fn.berhu_loss_masked(pg, holes.to(DEV))
        out.backward()
        assert float(out) == 0.0 and float(pg.grad.float().abs().max()) == 0.0
    # every finite target valid, target at the prediction's size, no holes: F.berhu_loss
    g = torch.Generator().manual_seed(9)
    target = (torch.randn(2, 1, 33, 47, generator=g) * 4)
    pa = pred.clone().to(DEV).requires_grad_(True)
    pb = pred.clone().to(DEV).requires_grad_(True)
    la = Fn.berhu_loss_masked(pa, target[:, 0].to(DEV), valid_min=float("-inf"), valid_max=float("inf"))
    lb = Fn.berhu_loss(pb, target.to(DEV))
    assert abs(float(la) - float(lb)) < 1e-5 * max(1.0, abs(float(lb)))
    (la * 1.3).backward()
    (lb * 1.3).backward()
    assert_close(pa.grad, pb.grad, 1e-7, 1e-4, "dpred vs berhu_loss")
    # the returned loss may be updated in place (the reference's ``loss += aux_weight * aux_loss``)
    pred2, _ = make_inputs(2, 17, 23, 101, 75, seed=5)
    p1 = pred.clone().to(DEV).requires_grad_(True)
    p2 = pred2.clone().to(DEV).requires_grad_(True)
    gt_d = gt.to(DEV)
    loss = Fn.berhu_loss_masked(p1, gt_d)
    l1 = float(loss)
    loss2 = Fn.berhu_loss_masked(p2, gt_d)
    loss += 0.15 * loss2
    loss.backward()
    assert float(loss) == pytest.approx(l1 + 0.15 * float(loss2), rel=1e-6)
    q1 = pred.clone().to(DEV).requires_grad_(True)
    q2 = pred2.clone().to(DEV).requires_grad_(True)
    Fn.berhu_loss_masked(q1, gt_d).backward()
    (Fn.berhu_loss_masked(q2, gt_d) * 0.15).backward()
    assert torch.equal(p1.grad, q1.grad)  # (the in-place update did not disturb what backward reads)
    assert torch.equal(p2.grad, q2.grad)
    # wrong arguments are errors, not silent conversions
    with pytest.raises(RuntimeError):
        Fn.berhu_loss_masked(pred.to(DEV), gt.to(DEV).to(torch.bfloat16))
    with pytest.raises(RuntimeError):
        Fn.berhu_loss_masked(torch.cat([pred, pred], 1).to(DEV), gt.to(DEV))


# ---------------------------------------------------------------------------------------------------------------
# 3. engine
# ---------------------------------------------------------------------------------------------------------------
REC = load_json("nets_meta.json")["cvpr_arch2_depth"]


def depth_batches(n, seed):
    g = torch.Generator().manual_seed(seed)
    B, _, H, W = REC["shape"]
    out = []
    for i in range(n):
        _, gt = make_inputs(B, 1, 1, H, W, seed=seed * 100 + i)
        out.append({"image": torch.randn(B, 3, H, W, generator=g), "mask": gt})
    return out


def fresh_net():
    assert REC["classes"] == 1 and REC["n_aux"] == 3
    return build_product_net(REC["kind"], REC["genotype"], REC["classes"], REC["dec_kwargs"], REC["seed"]).to(DEV)


def optimisers(net):
    return (torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-5),
            torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5))


def _cpu_sd(module):
    return {k: v.detach().cpu() for k, v in module.state_dict().items()}


@pytest.mark.parametrize("aux_weight", [-1, 0.15])
def test_train_segmenter_depth_step_host_launched_and_replayed(aux_weight, monkeypatch):
    from nas_segm_amd.engine import graphed, trainer
    from nas_segm_amd.nn import BerHuLoss

    batches = depth_batches(3, seed=21)
    crit = BerHuLoss(valid_min=0.0)
    made = []
    orig = graphed.GraphedSegmenterStep

    def counted(*a, **k):
        made.append(sorted(k))
        return orig(*a, **k)

    monkeypatch.setattr(graphed, "GraphedSegmenterStep", counted)
    real_value = trainer._loss_value

    def run(mode):
        monkeypatch.setenv("NASSEG_GRAPH", mode)
        del made[:]
        losses = []
        monkeypatch.setattr(trainer, "_loss_value", lambda s, loss: losses.append(real_value(s, loss)) or losses[-1])
        net = fresh_net()
        oe, od = optimisers(net)
        assert trainer.train_segmenter.__wrapped__(net, batches, oe, od, 0, crit, False, 3.0, 3.0, False,
                                                   print_every=100, aux_weight=aux_weight) is None
        return losses, _cpu_sd(net), list(made)

    l0, sd0, made0 = run("0")
    l1, sd1, made1 = run("1")
    print("aux_weight", aux_weight, "losses", l0, l1)
    assert made0 == [] and made1 == [["depth_crit"]], (made0, made1)
    assert len(l0) == 3 and all(math.isfinite(v) and v > 0 for v in l0)
    assert l0 == l1, (l0, l1)
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k
    # the first loss, by hand: the criterion on the heads of the same train-mode forward
    net = fresh_net().train()
    image = batches[0]["image"].to(DEV).contiguous(memory_format=torch.channels_last)
    target = batches[0]["mask"].to(DEV)
    with torch.no_grad():
        output, aux_outs = net(image)
        assert len(aux_outs) == 3 and all(a.shape[1] == 1 for a in aux_outs) and output.shape[1] == 1
        want = float(crit(output, target))
        if aux_weight > 0:
            want = want + sum(aux_weight * float(crit(a, target)) for a in aux_outs)
    assert abs(l0[0] - want) < 1e-5 * max(1.0, abs(want)), (l0[0], want)


def test_validate_depth_scores_and_reward():
    Fn = F()
    from nas_segm_amd.engine.inference import depth_scores, validate_depth

    net = fresh_net()
    vb = depth_batches(2, seed=22)
    reward = validate_depth(net, vb, 0, 0, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, print_every=100)
    assert not net.training
    acc = torch.zeros(12, dtype=torch.float64, device=DEV)
    with torch.no_grad():
        for b in vb:
            out = net(b["image"].to(DEV).contiguous(memory_format=torch.channels_last))[0]
            Fn.depth_metrics(out, b["mask"].to(DEV), MIN_DEPTH, MAX_DEPTH, acc=acc)
    s = depth_scores(acc)
    assert s["n"] == sum(float((torch.isfinite(b["mask"]) & (b["mask"] > MIN_DEPTH) & (b["mask"] <= MAX_DEPTH)).sum())
                         for b in vb)
    assert reward == (s["d1"] * s["d2"] * s["d3"]) ** (1.0 / 3.0)
    seen = []
    r2 = validate_depth(net, vb, 0, 0, print_every=100, reward_fn=lambda sc: seen.append(sc) or 1.0 / (1.0 + sc["rmse"]))
    assert seen == [s] and r2 == 1.0 / (1.0 + s["rmse"])

    class Broken(list):
        def __iter__(self):
            yield vb[0]
            raise RuntimeError("loader died")

    assert validate_depth(net, Broken(vb), 0, 0, print_every=100) == 0


def test_evaluate_depth_candidate_eager_and_replayed():
    from nas_segm_amd.engine.search import build_candidate, evaluate_candidate

    config = load_json("controller.json")["cvpr"]["samples"][0]["config"]
    train, val = depth_batches(2, seed=23), depth_batches(1, seed=24)
    seg = build_candidate(config, ctrl_version="cvpr", num_classes=19, agg_size=48, aux_cell=True, device=DEV,
                          task="depth")
    with torch.no_grad():
        out = seg.eval()(train[0]["image"].to(DEV).contiguous(memory_format=torch.channels_last))
    assert out[0].shape[1] == 1 and all(a.shape[1] == 1 for a in out[1])
    del seg, out
    kw = dict(ctrl_version="cvpr", agg_size=48, aux_cell=True, repeats=1, epochs=2, device=DEV, task="depth",
              min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)
    stats = {}
    torch.manual_seed(31)
    eager = evaluate_candidate(config, train, val, stats=stats, **kw)
    torch.manual_seed(31)
    replayed = evaluate_candidate(config, train, val, graphed=True, **kw)
    print("rewards", eager, replayed)
    assert 0.0 < eager <= 1.0 and stats["params"] > 0
    assert replayed == eager, (replayed, eager)


def test_train_task0_refuses_a_depth_criterion():
    from nas_segm_amd.engine.trainer import train_task0
    from nas_segm_amd.nn import BerHuLoss

    net = fresh_net()
    _, od = optimisers(net)
    with pytest.raises(ValueError, match="end to end"):
        train_task0({}, net, od, 0, BerHuLoss(), None, 2, False, False, 0.0, 3.0, False)
