"""The full-size berHu on the GPU (csrc/depth.hip: nasseg_berhu_up_fwd / _bwd; F.berhu_loss_upsampled;
nn.BerHuLoss(full_size=True)) against torch-CPU autograd (tests/_upsampled_berhu_ref.py), against the masked loss at
equal sizes, against the value ``depth_metrics`` scores, and through the engine's depth step.

Tolerances are those of test_masked_berhu_against_torch_autograd (tests/test_hip_depth.py); that torch's own fp32
evaluation uses at most 0.06 of the loss's and 0.04 of the gradient's against float64 on these inputs is checked
without a GPU by tests/test_upsampled_berhu_host.py."""
import math

import numpy as np
import pytest
import torch

import _upsampled_berhu_ref as U
from _util import assert_close, build_product_net, load_json

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
MIN_DEPTH, MAX_DEPTH = 1e-3, 10.0
GROUPS = (1, 4, 16, 64, 256)


def F():
    from nas_segm_amd import functional

    return functional


def run_gpu(pred, gt, valid_max=INF, scale=U.GRAD_SCALE, group=None):
    """-> (loss, dpred on the host, c, n_valid) of (loss * scale).backward(); ``group``: the backward's lanes per
    prediction pixel forced (None: the public function, which chooses from the shapes)"""
    pg = pred.clone().to(DEV).requires_grad_(True)
    if group is None:
        out, c, n = F().berhu_loss_upsampled(pg, gt.to(DEV), 0.0, valid_max, return_parts=True)
    else:
        parts = F()._depth_criterion(pg, gt.to(DEV), 0.0, valid_max, "up", group)
        out, c, n = parts.loss, parts.c, parts.n_valid
    assert out.dim() == 0 and out.dtype == torch.float32 and not c.requires_grad and not n.requires_grad
    (out * scale).backward()
    return float(out.detach()), pg.grad.cpu(), float(c), float(n)


def check_against(ref, loss, grad, what):
    print(what, "loss", loss, "ref", ref["loss"], "valid", int(ref["valid"].sum()), "of", ref["valid"].numel(),
          "max |dpred - ref|", float((grad.double() - ref["grad"].double()).abs().max()))
    assert abs(loss - ref["loss"]) < U.LOSS_RTOL * max(1.0, abs(ref["loss"])), (what, loss, ref["loss"])
    assert_close(grad, ref["grad"], U.GRAD_ATOL, U.GRAD_RTOL, "dpred {}".format(what))


# ---------------------------------------------------------------------------------------------------------------
# 1. against torch CPU autograd
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", U.CASES, ids=str)
def test_upsampled_berhu_against_torch_autograd(case):
    from nas_segm_amd.nn import BerHuLoss

    ref = U.reference(case)
    assert ref["gap"] >= U.MIN_GAP, (case, ref["gap"])  # (sign(v - t) is the same in any fp32 evaluation)
    loss, grad, c, n = run_gpu(ref["pred"], ref["gt"])
    check_against(ref, loss, grad, case)
    assert n == int(ref["valid"].sum()) and abs(c - ref["c"]) <= 1e-5 * ref["c"]
    # every group size of the backward is the same gradient (the public function chose one of them)
    for group in GROUPS:
        _, g, _, _ = run_gpu(ref["pred"], ref["gt"], group=group)
        assert_close(g, ref["grad"], U.GRAD_ATOL, U.GRAD_RTOL, "dpred {} group {}".format(case, group))
    # through the criterion module: the same bits; a tighter valid range is honoured (targets above 5 become holes)
    pred_d, gt_d = ref["pred"].to(DEV), ref["gt"].to(DEV)
    assert float(BerHuLoss(full_size=True)(pred_d, gt_d)) == loss
    ref5 = U.reference(case, valid_max=5.0)
    assert ref5["gap"] >= U.MIN_GAP and int(ref5["valid"].sum()) < int(ref["valid"].sum())
    pg = ref["pred"].clone().to(DEV).requires_grad_(True)
    out5 = BerHuLoss(valid_min=0.0, valid_max=5.0, full_size=True)(pg, gt_d)
    (out5 * U.GRAD_SCALE).backward()
    check_against(ref5, float(out5.detach()), pg.grad.cpu(), (case, "valid_max=5"))


@pytest.mark.parametrize("case", U.CASES, ids=str)
def test_upsampled_berhu_bf16_predictions(case):
    ref = U.reference(case, bf16=True)  # (fp32 arithmetic on the bf16-rounded prediction; gradient of loss * 1.3)
    pg = ref["pred"].to(torch.bfloat16).to(DEV).requires_grad_(True)
    out = F().berhu_loss_upsampled(pg, ref["gt"].to(DEV))
    assert abs(float(out) - ref["loss"]) < U.LOSS_RTOL * max(1.0, abs(ref["loss"]))
    (out * U.GRAD_SCALE).backward()
    assert pg.grad.dtype == torch.bfloat16
    ulps = U.bf16_ulps(pg.grad.cpu(), ref["grad"].to(torch.bfloat16))
    print("case", case, "bf16 ulps", ulps)
    assert ulps <= 1


@pytest.mark.parametrize("case", U.SPARSE_CASES, ids=str)
def test_upsampled_berhu_sparse_targets(case):
    ref = U.reference(case, sparse=True)
    assert int(ref["valid"].sum()) == U.SPARSE_VALID[case] and ref["gap"] >= U.MIN_GAP
    loss, grad, _, n = run_gpu(ref["pred"], ref["gt"])
    check_against(ref, loss, grad, (case, "sparse"))
    assert n == U.SPARSE_VALID[case]
    untouched = ref["grad"] == 0
    print("prediction pixels no valid target reaches:", int(untouched.sum()), "of", untouched.numel())
    assert float(grad[untouched].abs().max() if bool(untouched.any()) else 0.0) == 0.0
    for group in GROUPS:
        _, g, _, _ = run_gpu(ref["pred"], ref["gt"], group=group)
        assert_close(g, ref["grad"], U.GRAD_ATOL, U.GRAD_RTOL, "dpred sparse {} group {}".format(case, group))
        assert float(g[untouched].abs().max() if bool(untouched.any()) else 0.0) == 0.0


def test_equal_sizes_agree_with_the_masked_loss():
    Fn = F()
    for case in ((2, 6, 5, 6, 5), (2, 33, 47, 33, 47)):
        pred, gt = U.make_inputs(*case)
        pa = pred.clone().to(DEV).requires_grad_(True)
        pb = pred.clone().to(DEV).requires_grad_(True)
        la = Fn.berhu_loss_upsampled(pa, gt.to(DEV))
        lb = Fn.berhu_loss_masked(pb, gt.to(DEV))
        assert abs(float(la) - float(lb)) < U.LOSS_RTOL * max(1.0, abs(float(lb)))
        (la * U.GRAD_SCALE).backward()
        (lb * U.GRAD_SCALE).backward()
        assert_close(pa.grad, pb.grad, U.GRAD_ATOL, U.GRAD_RTOL, "dpred vs berhu_loss_masked {}".format(case))


# ---------------------------------------------------------------------------------------------------------------
# 2. edge cases, in-place use, reproducibility
# ---------------------------------------------------------------------------------------------------------------
def test_upsampled_berhu_edge_cases_and_in_place_use():
    Fn = F()
    case = (2, 33, 47, 130, 187)
    pred, gt = U.make_inputs(*case)
    # no valid pixel: loss 0, gradient 0, no NaN
    holes = torch.zeros(2, 130, 187)
    holes.view(-1)[::2] = float("nan")
    holes.view(-1)[1::4] = float("inf")
    holes.view(-1)[3::4] = -1.0
    for dtype in (torch.float32, torch.bfloat16):
        pg = pred.to(dtype).to(DEV).requires_grad_(True)
        out, c, n = Fn.berhu_loss_upsampled(pg, holes.to(DEV), return_parts=True)
        out.backward()
        assert float(out) == 0.0 and float(n) == 0.0 and not math.isnan(float(c))
        assert float(pg.grad.float().abs().max()) == 0.0 and not bool(torch.isnan(pg.grad.float()).any())
    # the returned loss may be updated in place (the reference's ``loss += aux_weight * aux_loss``)
    pred2, _ = U.make_inputs(2, 17, 23, 130, 187, seed=5)
    p1 = pred.clone().to(DEV).requires_grad_(True)
    p2 = pred2.clone().to(DEV).requires_grad_(True)
    gt_d = gt.to(DEV)
    loss = Fn.berhu_loss_upsampled(p1, gt_d)
    l1 = float(loss)
    loss2 = Fn.berhu_loss_upsampled(p2, gt_d)
    loss += 0.15 * loss2
    loss.backward()
    assert float(loss) == pytest.approx(l1 + 0.15 * float(loss2), rel=1e-6)
    q1 = pred.clone().to(DEV).requires_grad_(True)
    q2 = pred2.clone().to(DEV).requires_grad_(True)
    Fn.berhu_loss_upsampled(q1, gt_d).backward()
    (Fn.berhu_loss_upsampled(q2, gt_d) * 0.15).backward()
    assert torch.equal(p1.grad, q1.grad)  # (the in-place update did not disturb what backward reads)
    assert torch.equal(p2.grad, q2.grad)
    # wrong arguments are errors, not silent conversions
    with pytest.raises(RuntimeError):
        Fn.berhu_loss_upsampled(pred.to(DEV), gt.to(DEV).to(torch.bfloat16))
    with pytest.raises(RuntimeError):
        Fn.berhu_loss_upsampled(torch.cat([pred, pred], 1).to(DEV), gt.to(DEV))
    with pytest.raises(RuntimeError):
        Fn.berhu_loss_upsampled(pred.to(DEV), gt[:1].to(DEV))
    with pytest.raises(RuntimeError):
        Fn.berhu_loss_upsampled(pred.to(DEV), gt[:, None].to(DEV))
    with pytest.raises(RuntimeError):
        Fn.berhu_loss_upsampled(pred.double().to(DEV), gt.to(DEV))
    with pytest.raises(RuntimeError):  # (a NaN bound)
        Fn.berhu_loss_upsampled(pred.to(DEV), gt.to(DEV), valid_max=float("nan"))
    with pytest.raises(RuntimeError):  # (a group size the backward does not have)
        Fn._depth_criterion(pred.clone().to(DEV).requires_grad_(True), gt.to(DEV), 0.0, INF, "up", 8).loss.backward()


@pytest.mark.parametrize("case", [(1, 3, 4, 96, 128), (2, 33, 47, 130, 187)], ids=str)
def test_upsampled_berhu_is_reproducible(case):
    pred, gt = U.make_inputs(*case)
    for dtype in (torch.float32, torch.bfloat16):
        runs = []
        for _ in range(2):
            pg = pred.to(dtype).to(DEV).requires_grad_(True)
            out = F().berhu_loss_upsampled(pg, gt.to(DEV))
            (out * U.GRAD_SCALE).backward()
            runs.append((out.detach().clone(), pg.grad.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ---------------------------------------------------------------------------------------------------------------
# 3. the loss sees what the score sees
# ---------------------------------------------------------------------------------------------------------------
def test_upsampled_berhu_agrees_with_the_score():
    """A target without holes inside (min_depth, max_depth] and a prediction inside that range: the clamp of
    depth_metrics is idle, so both kernels work on the same pixels and the same up-sampled values."""
    Fn = F()
    B, h, w, H, W = 2, 17, 23, 101, 75
    g = torch.Generator().manual_seed(13)
    pred = 1.0 + 8.0 * torch.rand(B, 1, h, w, generator=g)
    gt = 0.5 + 9.0 * torch.rand(B, H, W, generator=g)
    pred_d, gt_d = pred.to(DEV), gt.to(DEV)
    loss, c, n = Fn.berhu_loss_upsampled(pred_d, gt_d, MIN_DEPTH, MAX_DEPTH, return_parts=True)
    acc = Fn.depth_metrics(pred_d, gt_d, MIN_DEPTH, MAX_DEPTH).cpu().numpy()
    assert float(n) == acc[0] == B * H * W
    # c and the loss from v, recomputed on the host (v: torch's fp32 up-sampling, a few ulps from the kernels')
    v = U.upsampled(pred, (H, W))
    d = (v - gt).abs().double()
    c_host = 0.2 * float(d.max())
    loss_host = float(torch.where(d <= c_host, d, (d * d + c_host * c_host) / (2 * c_host)).mean())
    print("c", float(c), c_host, "loss", float(loss), loss_host, "mean |v - t|", acc[1] / acc[0], float(d.mean()))
    assert abs(float(c) - c_host) <= 1e-5 * c_host and abs(float(loss) - loss_host) <= U.LOSS_RTOL * max(1.0, loss_host)
    assert abs(acc[1] / acc[0] - float(d.mean())) <= 1e-6 * float(d.mean())
    # bit for bit: with ONE valid target pixel, d is that pixel's |v - t|, c = 0.2f * d, and depth_metrics' sum of
    # |p - g| is the same difference taken in double (exact there, rounded once to fp32 in the loss) - so c must be
    # fl32(0.2f * fl32(acc[1])) for every probe: corners, edges, interior, both images
    probes = [(0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (1, H - 1, W - 1), (0, 1, 1), (1, 50, 37), (0, 3, 40),
              (1, 99, 2), (0, 47, 74), (1, 2, 73), (0, 100, 33), (1, 64, 64), (0, 31, 5), (1, 5, 31), (0, 77, 11),
              (1, 12, 70)]
    one = torch.zeros(B, H, W, device=DEV)
    for (b, Y, X) in probes:
        one.zero_()
        one[b, Y, X] = gt[b, Y, X]
        _, c1, n1 = Fn.berhu_loss_upsampled(pred_d, one, MIN_DEPTH, MAX_DEPTH, return_parts=True)
        a1 = Fn.depth_metrics(pred_d, one, MIN_DEPTH, MAX_DEPTH).cpu().numpy()
        assert float(n1) == a1[0] == 1.0
        assert np.float32(float(c1)) == np.float32(0.2) * np.float32(a1[1]), ((b, Y, X), float(c1), a1[1])


# ---------------------------------------------------------------------------------------------------------------
# 4. engine
# ---------------------------------------------------------------------------------------------------------------
REC = load_json("nets_meta.json")["cvpr_arch2_depth"]


def depth_batches(n, seed):
    g = torch.Generator().manual_seed(seed)
    B, _, H, W = REC["shape"]
    out = []
    for i in range(n):
        _, gt = U.make_inputs(B, 1, 1, H, W, seed=seed * 100 + i)
        out.append({"image": torch.randn(B, 3, H, W, generator=g), "mask": gt})
    return out


def fresh_net():
    assert REC["classes"] == 1 and REC["n_aux"] == 3
    return build_product_net(REC["kind"], REC["genotype"], REC["classes"], REC["dec_kwargs"], REC["seed"]).to(DEV)


def optimisers(net):
    return (torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-5),
            torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5))


@pytest.mark.parametrize("aux_weight", [-1, 0.15])
def test_train_segmenter_full_size_depth_step_host_launched_and_replayed(aux_weight, monkeypatch):
    from nas_segm_amd.engine import graphed, trainer
    from nas_segm_amd.nn import BerHuLoss

    batches = depth_batches(3, seed=21)
    crit = BerHuLoss(valid_min=0.0, full_size=True)
    made = []
    orig = graphed.GraphedSegmenterStep

    def counted(*a, **k):
        made.append(k["depth_crit"].config())
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
        return losses, {k: v.detach().cpu() for k, v in net.state_dict().items()}, list(made), (net, oe, od)

    l0, sd0, made0, _ = run("0")
    l1, sd1, made1, (net1, oe1, od1) = run("1")
    print("aux_weight", aux_weight, "losses", l0, l1)
    assert made0 == [] and made1 == [("berhu_up", 0.0, INF)], (made0, made1)
    assert len(l0) == 3 and all(math.isfinite(v) and v > 0 for v in l0)
    assert l0 == l1, (l0, l1)
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k
    # a fourth step on the same net with the criterion at the prediction's size: a step of its own is recorded, the
    # full-size one is not replayed for it
    plain = BerHuLoss(valid_min=0.0)
    assert trainer.train_segmenter.__wrapped__(net1, batches[:1], oe1, od1, 1, plain, False, 3.0, 3.0, False,
                                               print_every=100, aux_weight=aux_weight) is None
    assert made == [("berhu_up", 0.0, INF), ("berhu", 0.0, INF)], made
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
        at_prediction_size = float(plain(output, target))
    assert abs(l0[0] - want) < 1e-5 * max(1.0, abs(want)), (l0[0], want)
    assert at_prediction_size != float(crit(output, target))  # (the two criteria are different losses)


def test_evaluate_depth_candidate_with_the_full_size_criterion():
    from nas_segm_amd.engine.search import evaluate_candidate
    from nas_segm_amd.nn import BerHuLoss

    config = load_json("controller.json")["cvpr"]["samples"][0]["config"]
    train, val = depth_batches(2, seed=23), depth_batches(1, seed=24)
    kw = dict(ctrl_version="cvpr", agg_size=48, aux_cell=True, repeats=1, epochs=2, device=DEV, task="depth",
              min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, depth_crit=BerHuLoss(0.0, full_size=True))
    stats_e, stats_r = {}, {}
    torch.manual_seed(31)
    eager = evaluate_candidate(config, train, val, stats=stats_e, **kw)
    torch.manual_seed(31)
    replayed = evaluate_candidate(config, train, val, graphed=True, stats=stats_r, **kw)
    print("rewards", eager, replayed)
    # (a candidate that failed is scored 0 before its parameters are counted; after so few steps the reward of one
    #  that trained may be 0 as well - no pixel within 25 % yet - so "it trained" is read from ``stats``)
    assert stats_e.get("params", 0) > 0 and stats_r == stats_e
    assert math.isfinite(eager) and math.isfinite(replayed) and 0.0 <= eager <= 1.0
    assert replayed == eager, (replayed, eager)
    with pytest.raises(ValueError, match="depth_crit"):
        evaluate_candidate(config, train, val, **dict(kw, depth_crit=torch.nn.L1Loss()))
