"""Engine parity on the GPU: train_segmenter / populate_task0 / train_task0 /
validate against what the reference's own engine produced on the same inputs
(tests/golden/engine*.{npz,json}), plus full-size property checks."""
import numpy as np
import pytest
import torch

from _util import assert_checksums_close, build_product_net, checksums, load_json, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ENG_NPZ = load_npz("engine.npz")
ENG_META = load_json("engine_meta.json")


class _DS(object):
    def set_stage(self, stage):
        self.stage = stage


class Loader(object):
    def __init__(self, batches):
        self.batches = batches
        self.dataset = _DS()
        self.batch_sampler = type("BS", (), {"batch_size": 1})()

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


class _Crit(object):
    ignore_index = 255


def _cpu_sd(module):
    return {k: v.detach().cpu() for k, v in module.state_dict().items()}


def _record_losses(monkeypatch):
    from nas_segm_amd.engine import trainer

    values = []
    orig = trainer.F.log_softmax_nll

    def rec(logits, target, ignore_index=255):
        v = orig(logits, target, ignore_index)
        values.append(float(v.detach()))
        return v

    monkeypatch.setattr(trainer.F, "log_softmax_nll", rec)
    return values


@pytest.mark.parametrize("name", sorted(ENG_META))
def test_engine_matches_reference_run(name, monkeypatch):
    from nas_segm_amd.engine import RankParallel
    from nas_segm_amd.engine.inference import validate
    from nas_segm_amd.engine.trainer import populate_task0, train_segmenter, train_task0

    # (the per-call loss values are read on the host: steps launched from the host, not replayed
    #  from a hipGraph - test_engine_auto_graph_equals_host_launches covers the replayed form)
    monkeypatch.setenv("NASSEG_GRAPH", "0")
    rec = ENG_META[name]
    net = build_product_net(rec["kind"], rec["genotype"], rec["classes"], rec["dec_kwargs"], rec["seed"])
    assert_checksums_close(checksums(net.state_dict()), rec["init_checksums"], what="init")
    init = _cpu_sd(net)
    segmenter = RankParallel(net.to(DEV))
    batches = [{"image": torch.from_numpy(ENG_NPZ["{}/train/image/{}".format(name, i)]),
                "mask": torch.from_numpy(ENG_NPZ["{}/train/mask/{}".format(name, i)])} for i in range(2)]
    # default_args.py:57-66 - SGD(1e-3, 0.9, wd 1e-5) encoder, Adam(3e-3, wd 1e-5) decoder
    optim_enc = torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-5)
    optim_dec = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
    avg_param = [p.data.clone() for p in segmenter.parameters()]
    values = _record_losses(monkeypatch)
    ret = train_segmenter.__wrapped__(segmenter, Loader(batches), optim_enc, optim_dec, 0, _Crit(), False,
                                      3.0, 3.0, True, print_every=100, aux_weight=rec["aux_weight"],
                                      avg_param=avg_param, polyak_decay=0.99)
    assert ret is None
    # Tolerances: what the REFERENCE's own numbers move by when its input images are perturbed by
    # 1e-6 (make_golden.py re-runs it twice and records the largest move next to every value:
    # rec["sensitivity"]) is the floor - training through ~100 train-mode BatchNorms, ReLUs,
    # max-pools and two Adam steps amplifies fp32 rounding that much - times 3, on top of 1e-4.
    sens = rec["sensitivity"]
    bad = []

    def check(what, got, want, floor, rel=1e-4, abs_=1e-6):
        tol = rel * abs(want) + abs_ + 3.0 * floor
        if not abs(got - want) <= tol:
            bad.append("{}: {} vs {} (tol {:.3e}, floor {:.3e})".format(what, got, want, tol, floor))

    want = rec["task1_crit_values"]
    assert len(values) == len(want)
    for i, (v, w, f) in enumerate(zip(values, want, sens["task1_crit"])):
        check("task1 loss {}".format(i), v, w, f, abs_=1e-4)
    after = _cpu_sd(net)
    got = checksums(after)
    # Parameters whose gradient is ANALYTICALLY zero - the BatchNorm bias of Pool's 1x1 conv: a
    # per-channel shift that commutes with the max-pool and is removed by the BatchNorm that
    # follows - receive pure rounding noise, which Adam normalises to steps of up to lr per
    # element in a noise-dependent direction.  The reference's run identifies them (they moved by
    # < 5 % of a full Adam step per element; every other decoder tensor moved by > 60 %): for those
    # the only meaningful statement is that they stay at noise level here as well.
    full_step = {k: rec["numel"][k] * 3e-3 * len(batches) for k in rec["numel"]}
    noise = {k for k, m in rec["task1_delta_mass"].items()
             if k.startswith("decoder.") and m < 0.05 * full_step[k]}
    assert len(noise) <= 0.1 * len(rec["numel"]), len(noise)
    names = [k for k, _ in net.named_parameters()]
    for k, (s, sa) in rec["task1_checksums"].items():
        if "num_batches_tracked" in k:
            assert got[k][0] == s, k
        elif k in noise:
            moved = float((after[k] - init[k]).double().abs().sum())
            if not moved < 0.10 * full_step[k]:
                bad.append("task1 {} (zero-gradient parameter) moved by {} of a full Adam step".format(
                    k, moved / full_step[k]))
        else:
            check("task1 " + k, got[k][1], sa, sens["task1_mass"][k])
    pol = checksums({str(i): a.cpu() for i, a in enumerate(avg_param)})
    for k, (s, sa) in rec["task1_polyak_checksums"].items():
        slack = 0.02 * 0.10 * full_step[names[int(k)]] if names[int(k)] in noise else 0.0
        check("polyak " + k, pol[k][1], sa, sens["task1_polyak_mass"][k], abs_=1e-6 + slack)

    # validation reward of the trained candidate
    vb = [{"image": torch.from_numpy(ENG_NPZ["{}/val/image/{}".format(name, i)]),
           "mask": torch.from_numpy(ENG_NPZ["{}/val/mask/{}".format(name, i)])} for i in range(2)]
    reward = validate.__wrapped__(segmenter, Loader(vb), 0, 0, num_classes=rec["classes"], print_every=100,
                                  omit_classes=[0])
    assert np.isfinite(reward)
    check("reward", reward, rec["val_reward"], sens["val_reward"], rel=0.0, abs_=3e-4)

    # task0: feature cache + decoder-only epoch
    loader1 = Loader([{"image": b["image"][i:i + 1], "mask": b["mask"][i:i + 1]} for b in batches for i in range(2)])
    Xy = populate_task0.__wrapped__(segmenter, loader1, None, 4, do_kd=False)
    assert list(Xy["out_size"]) == rec["task0_out_size"]
    assert Xy["y"].dtype == torch.int64 and Xy[0].shape[0] == 4
    cache = checksums({str(k): v.cpu() for k, v in Xy.items() if k != "out_size"})
    for k, (s, sa) in rec["task0_cache_checksums"].items():
        check("cache " + k, cache[k][1], sa, sens["task0_cache_mass"][k])
    assert cache["y"] == rec["task0_cache_checksums"]["y"]  # labels are integers: exact
    optim_dec0 = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
    np.random.seed(123)
    del values[:]
    ret = train_task0.__wrapped__(Xy, segmenter, optim_dec0, 0, _Crit(), None, 2, False, False, 0.0, 3.0,
                                  False, aux_weight=max(rec["aux_weight"], 0))
    assert ret is None
    assert len(values) == len(rec["task0_crit_values"])
    for i, (v, w, f) in enumerate(zip(values, rec["task0_crit_values"], sens["task0_crit"])):
        check("task0 loss {}".format(i), v, w, f, abs_=1e-4)
    got0 = checksums(_cpu_sd(net.decoder))
    for k, (s, sa) in rec["task0_checksums"].items():
        if "num_batches_tracked" in k:
            assert got0[k][0] == s, k
        elif ("decoder." + k) not in noise:
            check("task0 " + k, got0[k][1], sa, sens["task0_mass"][k])
    assert not bad, "{} of the reference run's numbers missed:\n{}".format(len(bad), "\n".join(bad[:40]))


@pytest.mark.parametrize("name", sorted(ENG_META))
def test_engine_auto_graph_equals_host_launches(name, monkeypatch):
    """train_segmenter / populate_task0 / train_task0 pick hipGraph replay by themselves at these
    sizes (engine.graphed.auto_graph): parameters, running statistics, the feature cache and the
    reward afterwards are bit for bit those of the same calls launched from the host.  The cache
    is stored NHWC (channels_last) with the reference's shapes."""
    from nas_segm_amd.engine import RankParallel, graphed
    from nas_segm_amd.engine.inference import validate
    from nas_segm_amd.engine.trainer import populate_task0, train_segmenter, train_task0

    rec = ENG_META[name]
    batches = [{"image": torch.from_numpy(ENG_NPZ["{}/train/image/{}".format(name, i)]),
                "mask": torch.from_numpy(ENG_NPZ["{}/train/mask/{}".format(name, i)])} for i in range(2)]
    vb = [{"image": torch.from_numpy(ENG_NPZ["{}/val/image/{}".format(name, i)]),
           "mask": torch.from_numpy(ENG_NPZ["{}/val/mask/{}".format(name, i)])} for i in range(2)]
    made = []
    for cls in ("GraphedSegmenterStep", "GraphedTask0Step"):
        orig = getattr(graphed, cls)

        def counted(*a, _orig=orig, _cls=cls, **k):
            made.append(_cls)
            return _orig(*a, **k)

        monkeypatch.setattr(graphed, cls, counted)

    def run(mode):
        monkeypatch.setenv("NASSEG_GRAPH", mode)
        del made[:]
        net = build_product_net(rec["kind"], rec["genotype"], rec["classes"], rec["dec_kwargs"], rec["seed"])
        segmenter = RankParallel(net.to(DEV))
        oe = torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-5)
        od = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
        for epoch in range(2):
            assert train_segmenter.__wrapped__(segmenter, Loader(batches), oe, od, epoch, _Crit(), False, 3.0, 3.0,
                                               False, print_every=100, aux_weight=rec["aux_weight"]) is None
        reward = validate.__wrapped__(segmenter, Loader(vb), 0, 0, num_classes=rec["classes"], print_every=100,
                                      omit_classes=[0])
        loader1 = Loader([{"image": b["image"][i:i + 1], "mask": b["mask"][i:i + 1]} for b in batches for i in range(2)])
        Xy = populate_task0.__wrapped__(segmenter, loader1, None, 4, do_kd=False)
        for k, v in Xy.items():
            if k not in ("y", "out_size"):
                assert v.dim() == 4 and v.shape[0] == 4 and v.is_contiguous(memory_format=torch.channels_last), k
        od0 = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
        for epoch in range(2):
            np.random.seed(123 + epoch)
            assert train_task0.__wrapped__(Xy, segmenter, od0, epoch, _Crit(), None, 2, False, False, 0.0, 3.0, False,
                                           aux_weight=max(rec["aux_weight"], 0)) is None
        return _cpu_sd(net), reward, {str(k): v.cpu() for k, v in Xy.items() if k != "out_size"}, list(made)

    sd0, r0, c0, made0 = run("0")
    sd1, r1, c1, made1 = run("auto")
    assert made0 == [] and made1 == ["GraphedSegmenterStep", "GraphedTask0Step"], (made0, made1)
    assert r0 == r1
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k
    for k in c0:
        assert torch.equal(c0[k], c1[k]), k


def test_step_is_deterministic_run_to_run():
    """no atomics on float data anywhere: two identical steps give bit-identical gradients"""
    from nas_segm_amd import functional as F

    rec = load_json("nets_meta.json")["wacv_arch0"]
    grads = []
    for _ in range(2):
        net = build_product_net(rec["kind"], rec["genotype"], rec["classes"], rec["dec_kwargs"], 0).to(DEV).train()
        g = torch.Generator().manual_seed(5)
        x = torch.randn(2, 3, 129, 161, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
        t = torch.randint(0, 19, (2, 129, 161), generator=g).to(DEV)
        out = net(x)
        loss = F.log_softmax_nll(out, F.nearest_label_resize(t, out.shape[2:]), 255)
        loss.backward()
        grads.append(torch.cat([p.grad.reshape(-1) for p in net.parameters()]).cpu())
    assert torch.equal(grads[0], grads[1])


def test_full_size_headline_shape_properties():
    """BASELINE headline shape (WACV arch0, 1024x2048): output geometry, finite
    loss / gradients, reward-path conservation laws (size-independent properties)."""
    from nas_segm_amd import functional as F
    from nas_segm_amd.helpers.miou_utils import fast_cm

    rec = load_json("nets_meta.json")["wacv_arch0"]
    net = build_product_net(rec["kind"], rec["genotype"], rec["classes"], rec["dec_kwargs"], 0).to(DEV).train()
    B, H, W = 2, 1024, 2048
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, H, W, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    t = torch.randint(0, 19, (B, H, W), generator=g)
    t[:, 100:105] = 255
    t = t.to(DEV)
    out = net(x)
    assert tuple(out.shape) == (B, 19, 256, 512)
    tv = F.nearest_label_resize(t, out.shape[2:])
    loss = F.log_softmax_nll(out, tv, 255)
    loss.backward()
    assert torch.isfinite(loss)
    # an untrained net on random labels sits near log(19)
    assert abs(float(loss) - np.log(19.0)) < 1.0
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    # softmax-CE gradient sums to zero over classes for every valid pixel and is zero on ignored ones
    lg = out.detach().clone().requires_grad_(True)
    F.log_softmax_nll(lg, tv, 255).backward()
    per_pixel = lg.grad.sum(1)
    assert float(per_pixel.abs().max()) < 1e-6
    ign = lg.grad.permute(0, 2, 3, 1)[tv == 255]
    assert ign.numel() > 0 and float(ign.abs().max()) == 0.0
    # confusion matrix at full label resolution: total == number of valid pixels, rows == gt histogram
    gt8 = t.to(torch.uint8)
    cm = F.argmax_confusion(out.detach(), gt8, 19)
    valid = int((gt8 < 19).sum())
    assert int(cm.sum()) == valid
    hist = torch.bincount(gt8[gt8 < 19].reshape(-1).long(), minlength=19)
    assert torch.equal(cm.sum(1), hist)
    # fast_cm on identical uint8 inputs: diagonal only
    same = fast_cm(gt8.reshape(-1), gt8.reshape(-1), 19)
    assert int(same.diagonal().sum()) == valid and int(same.sum()) == valid


def test_full_size_headline_logits_match_the_oracle():
    """the BASELINE headline network at its full input size, 1x3x1024x2048, inference mode: HIP
    logits against the CPU oracle (the restatement pinned to the reference by the golden vectors)
    - the north-star bound of 1e-4, and identical arg-max labels away from near-ties"""
    from _util import oracle_forward

    rec = load_json("nets_meta.json")["wacv_arch0"]
    net = build_product_net(rec["kind"], rec["genotype"], rec["classes"], rec["dec_kwargs"], 0).eval()
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 3, 1024, 2048, generator=g)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    with torch.no_grad():
        want = oracle_forward(sd, x, rec, training=False)
        got = net.to(DEV)(x.to(DEV).contiguous(memory_format=torch.channels_last)).cpu()
    assert tuple(got.shape) == tuple(want.shape) == (1, 19, 256, 512)
    err = float((got - want).abs().max())
    assert err <= 1e-4, err
    top2 = want.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3
    assert bool((got.argmax(1) == want.argmax(1))[clear].all())


def test_linearity_of_dense_and_depthwise_conv_at_size():
    """conv(a*x + y) == a*conv(x) + conv(y) at a BASELINE-sized activation"""
    from nas_segm_amd import functional as F

    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 32, 256, 512, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    y = torch.randn(2, 32, 256, 512, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    wd = (torch.randn(32, 1, 5, 5, generator=g) * 0.2).to(DEV)
    wp = (torch.randn(64, 32, 1, 1, generator=g) * 0.2).to(DEV)
    z = F.add(F.param_sum(x, y, torch.full((32,), 0.5, device=DEV), torch.ones(32, device=DEV)), y * 0)
    for f in (lambda t: F.depthwise_conv2d(t, wd, 1, 12, 6), lambda t: F.conv2d(t, wp)):
        lhs = f(z)
        rhs = 0.5 * f(x) + f(y)
        assert float((lhs - rhs).abs().max()) < 2e-4


def test_candidate_evaluation_with_controller_samples():
    """config-4 mode: genotypes sampled by the reference controller (golden) are built,
    trained a few steps and scored on one GPU; a broken candidate scores 0"""
    from nas_segm_amd.engine.search import evaluate_candidates

    ctrl = load_json("controller.json")
    g = torch.Generator().manual_seed(3)

    def make_batches(rank):
        def batch(n_cls):
            img = torch.randn(2, 3, 97, 129, generator=g)
            m = torch.randint(0, n_cls, (2, 97, 129), generator=g).to(torch.uint8)
            return {"image": img, "mask": m}
        return [batch(19) for _ in range(2)], [batch(19)]

    configs = [s["config"] for s in ctrl["wacv"]["samples"][:2]]
    torch.manual_seed(21)  # (candidate weights are drawn from the global generator)
    rewards = evaluate_candidates(configs, make_batches, ctrl_version="wacv", num_classes=19,
                                  agg_size=48, aux_cell=False, repeats=1, omit_classes=())
    assert len(rewards) == 2 and all(np.isfinite(r) and 0.0 <= r <= 1.0 for r in rewards)
    # the same candidates trained through a hipGraph replay: identical rewards
    g.manual_seed(3)
    torch.manual_seed(21)
    replayed = evaluate_candidates(configs, make_batches, ctrl_version="wacv", num_classes=19,
                                   agg_size=48, aux_cell=False, repeats=1, omit_classes=(), graphed=True)
    assert replayed == rewards, (replayed, rewards)
    cv = [s["config"] for s in ctrl["cvpr"]["samples"][:1]]
    r2 = evaluate_candidates(cv, make_batches, ctrl_version="cvpr", num_classes=19, agg_size=48,
                             aux_cell=True, repeats=1, omit_classes=())
    assert len(r2) == 1 and np.isfinite(r2[0]) and 0.0 <= r2[0] <= 1.0


@pytest.mark.parametrize("net_name,capture_opt,plain", [("wacv_arch0", False, False), ("wacv_arch0", True, False),
                                                          ("cvpr_arch0", False, False), ("wacv_arch0", True, True),
                                                          ("cvpr_arch0", True, True), ("cvpr_arch0", False, True)])
def test_graphed_step_equals_eager_step(net_name, capture_opt, plain):
    """hipGraph replay of forward+loss+backward (optionally clip+optimisers) leaves exactly the
    parameters, running statistics and losses the eager step sequence leaves (bit for bit:
    same kernels, same order, no float atomics), over changing batches.  plain: the optimisers as the
    reference's create_optimisers makes them (no ``capturable``) - stepped by nasseg_optim_step, inside the graph
    too, with Adam's step count on the device; otherwise torch's capturable implementations."""
    from nas_segm_amd.engine.graphed import GraphedSegmenterStep
    from nas_segm_amd.engine.trainer import segmenter_step

    rec = load_json("nets_meta.json")[net_name]
    aux_w = 0.15 if rec["kind"] != "template" else -1
    g = torch.Generator().manual_seed(11)
    batches = [(torch.randn(2, 3, 97, 129, generator=g).to(DEV).contiguous(memory_format=torch.channels_last),
                torch.randint(0, rec["classes"], (2, 97, 129), generator=g).to(DEV)) for _ in range(3)]

    def run(graphed):
        net = build_product_net(rec["kind"], rec["genotype"], rec["classes"], rec["dec_kwargs"], 0).to(DEV).train()
        oe = torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-5)
        od = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5, capturable=not plain)
        losses = []
        if graphed:
            stepper = GraphedSegmenterStep(net, batches[0][0], batches[0][1], oe, od, 255, 3.0, 3.0, aux_w,
                                           capture_optimisers=capture_opt)
            assert stepper.capture_optimisers == capture_opt
            assert (stepper._native is not None) == (plain and capture_opt)
            for x, t in batches:
                losses.append(float(stepper.step(x, t)))
        else:
            for x, t in batches:
                losses.append(float(segmenter_step(net, x, t, oe, od, 255, 3.0, 3.0, aux_w)))
        if plain:  # the optimisers' state is torch's: CPU step counts that followed the device's
            steps = set(float(st["step"]) for st in od.state.values())
            assert steps == {float(len(batches))} and not any(st["step"].is_cuda for st in od.state.values())
            assert all(torch.is_tensor(st.get("momentum_buffer")) for st in oe.state.values())
        return losses, _cpu_sd(net)

    l0, sd0 = run(False)
    l1, sd1 = run(True)
    assert l0 == l1, (l0, l1)
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k


@pytest.mark.parametrize("net_name,lanes", [("cvpr_arch0", 2), ("cvpr_arch0", 4), ("wacv_arch0", 3)])
def test_lanes_replay_equals_the_line(net_name, lanes, monkeypatch):
    """A recorded step laid out as stages of independent lanes (engine/graph_dag.py: dependencies from the address
    ranges every entry point was handed, one line graph per (stage, lane), events between stages) leaves exactly
    what the line as recorded leaves - parameters, running statistics, optimiser state, losses - over changing
    batches; the layout really has side lanes (the cells of a MergeCell / the blocks of a template decoder share
    nothing, src/nn/micro_decoders.py:54-139,380-398), and every dependency sits inside a lane or points to an
    earlier stage (verified at the capture; here the layout taken is the cost model's, untimed, so that it is used
    whatever this box's clock says)."""
    from nas_segm_amd.engine import graph_dag
    from nas_segm_amd.engine.graphed import GraphedSegmenterStep

    rec = load_json("nets_meta.json")[net_name]
    aux_w = 0.15 if rec["kind"] != "template" else -1
    g = torch.Generator().manual_seed(12)
    batches = [(torch.randn(2, 3, 97, 129, generator=g).to(DEV).contiguous(memory_format=torch.channels_last),
                torch.randint(0, rec["classes"], (2, 97, 129), generator=g).to(DEV)) for _ in range(4)]
    monkeypatch.setattr(graph_dag, "TRIALS", False)

    def run(n_lanes):
        monkeypatch.setattr(graph_dag, "LANES", n_lanes)
        net = build_product_net(rec["kind"], rec["genotype"], rec["classes"], rec["dec_kwargs"], 0).to(DEV).train()
        oe = torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-5)
        od = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
        stepper = GraphedSegmenterStep(net, batches[0][0], batches[0][1], oe, od, 255, 3.0, 3.0, aux_w,
                                       capture_optimisers=True)
        losses = [float(stepper.step(x, t)) for x, t in batches]
        state = [v.detach().cpu().clone() for st in od.state.values() for v in st.values() if torch.is_tensor(v)]
        return losses, _cpu_sd(net), state, stepper

    l1, sd1, st1, line = run(1)
    assert line.plan is None
    ln, sdn, stn, laid = run(lanes)
    assert laid.plan is not None and laid.layout["forks"] >= 1 and laid.layout["side_units"] > 0, laid.layout
    assert laid.layout["lanes"] <= lanes
    assert l1 == ln, (l1, ln)
    for k in sd1:
        assert torch.equal(sd1[k], sdn[k]), k
    assert len(st1) == len(stn) and all(torch.equal(a, b) for a, b in zip(st1, stn))


def test_timed_layouts_never_lose_to_the_line():
    """with trials on (the default) the stepper keeps a layout only when its replays measured faster than the line's;
    either way the step it replays equals the host-launched one"""
    from nas_segm_amd.engine.graphed import GraphedSegmenterStep
    from nas_segm_amd.engine.trainer import segmenter_step

    rec = load_json("nets_meta.json")["cvpr_arch0"]
    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, 3, 97, 129, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    t = torch.randint(0, rec["classes"], (2, 97, 129), generator=g).to(DEV)

    def nets():
        net = build_product_net(rec["kind"], rec["genotype"], rec["classes"], rec["dec_kwargs"], 0).to(DEV).train()
        return (net, torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9),
                torch.optim.Adam(net.decoder.parameters(), lr=3e-3))

    net, oe, od = nets()
    stepper = GraphedSegmenterStep(net, x, t, oe, od, 255, 3.0, 3.0, 0.15, capture_optimisers=True)
    lay = stepper.layout
    assert lay and lay["mode"] == "stages" and lay["tried"], lay
    if stepper.plan is not None:
        assert lay["ms"] < lay["line_ms"], lay
    got = [float(stepper.step(x, t)) for _ in range(3)]
    net2, oe2, od2 = nets()
    want = [float(segmenter_step(net2, x, t, oe2, od2, 255, 3.0, 3.0, 0.15)) for _ in range(3)]
    assert got == want
    sd, sd2 = _cpu_sd(net), _cpu_sd(net2)
    for k in sd:
        assert torch.equal(sd[k], sd2[k]), k
    # the optimisers are inside the graph, their hyper-parameters recorded by value: a schedule that moves lr makes the
    # capture stale - the stepper says so (the trainer's cache asks and records a new step) and refuses to replay
    from nas_segm_amd.engine.graphed import StaleCapture

    assert not stepper.stale()
    od.param_groups[0]["lr"] = 1e-3
    assert stepper.stale()
    with pytest.raises(StaleCapture):
        stepper.step(x, t)
    od.param_groups[0]["lr"] = 3e-3
    assert not stepper.stale()
    assert float(stepper.step(x, t)) == float(segmenter_step(net2, x, t, oe2, od2, 255, 3.0, 3.0, 0.15))


def test_graphed_step_with_a_custom_loss_equals_eager():
    """GraphedSegmenterStep(loss_fn=F.berhu_loss): the depth-head step (BASELINE config 5) replayed from
    a hipGraph leaves the parameters of the same steps written out eagerly"""
    from nas_segm_amd import functional as F
    from nas_segm_amd.engine.graphed import GraphedSegmenterStep
    from nas_segm_amd.engine.trainer import _clip_and_step

    rec = load_json("nets_meta.json")["wacv_arch0"]
    g = torch.Generator().manual_seed(12)
    xs = [torch.randn(2, 3, 65, 97, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
          for _ in range(3)]

    def run(graphed):
        net = build_product_net(rec["kind"], rec["genotype"], 1, rec["dec_kwargs"], 0).to(DEV).train()
        oe = torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9)
        od = torch.optim.SGD(net.decoder.parameters(), lr=1e-3)
        with torch.no_grad():
            shape = net(xs[0]).shape
        ts = [(torch.rand(shape, generator=g) * 10).to(DEV).contiguous(memory_format=torch.channels_last)
              for _ in xs]
        losses = []
        if graphed:
            stepper = GraphedSegmenterStep(net, xs[0], ts[0], oe, od, 255, 3.0, 3.0, -1, loss_fn=F.berhu_loss)
            for x, t in zip(xs, ts):
                losses.append(float(stepper.step(x, t)))
        else:
            for x, t in zip(xs, ts):
                loss = F.berhu_loss(net(x), t)
                oe.zero_grad()
                od.zero_grad()
                loss.backward()
                _clip_and_step([(list(net.encoder.parameters()), 3.0, oe), (list(net.decoder.parameters()), 3.0, od)])
                losses.append(float(loss))
        return losses, _cpu_sd(net)

    g = torch.Generator().manual_seed(12)
    l0, sd0 = run(False)
    g = torch.Generator().manual_seed(12)
    l1, sd1 = run(True)
    assert l0 == l1, (l0, l1)
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k


def test_search_loop_with_real_candidates(tmp_path):
    """outer loop (config 4) on one GPU: genotypes + entropy/log-prob recorded from the reference
    controller feed search_loop; every candidate is built, trained and validated by
    evaluate_candidate and logged in the reference's genotype-log format"""
    from nas_segm_amd.engine.search import evaluate_candidate, search_loop

    samples = iter(load_json("controller.json")["wacv"]["samples"][:3])
    g = torch.Generator().manual_seed(4)
    train = [{"image": torch.randn(2, 3, 65, 97, generator=g),
              "mask": torch.randint(0, 19, (2, 65, 97), generator=g).to(torch.uint8)} for _ in range(2)]
    val = train[:1]

    def sample_fn():
        s = next(samples)
        return s["config"], float(s.get("entropy", 0.0)), float(s.get("log_prob", 0.0))

    def evaluate_fn(config):
        stats = {}
        r = evaluate_candidate(config, train, val, ctrl_version="wacv", num_classes=19, agg_size=48,
                               aux_cell=False, repeats=1, omit_classes=(), stats=stats)
        return r, stats.get("params", -1)

    trained = []
    path = tmp_path / "genotypes.out"
    with open(path, "w") as fo:
        hist = search_loop(sample_fn, trained.append, evaluate_fn, 3, arch_writer=fo)
    assert len(hist) == 3 and len(trained) == 3
    assert all(0.0 <= r <= 1.0 for _, r in hist)
    lines = open(path).read().strip().split("\n")
    assert len(lines) == 3 and all(l.startswith("reward: ") and ", genotype: [[" in l for l in lines)
    assert all(int(l.split("params: ")[1].split(",")[0]) > 50000 for l in lines)


def test_segmenter_step_equals_a_plain_backward_step():
    """segmenter_step defers the second stage of the weight-gradient reductions to one batched
    launch after backward; parameters after two steps equal, bit for bit, those of the same steps
    written out with an ordinary loss.backward()"""
    from nas_segm_amd import functional as F
    from nas_segm_amd.engine.trainer import _clip_and_step, segmenter_step

    rec = load_json("nets_meta.json")["wacv_arch0"]
    g = torch.Generator().manual_seed(9)
    batches = [(torch.randn(2, 3, 97, 129, generator=g).to(DEV).contiguous(memory_format=torch.channels_last),
                torch.randint(0, 19, (2, 97, 129), generator=g).to(DEV)) for _ in range(2)]

    def run(plain):
        net = build_product_net(rec["kind"], rec["genotype"], rec["classes"], rec["dec_kwargs"], 0).to(DEV).train()
        oe = torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-5)
        od = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
        for x, t in batches:
            if plain:
                out = net(x)
                loss = F.log_softmax_nll(out, F.nearest_label_resize(t, out.shape[2:]), 255)
                oe.zero_grad()
                od.zero_grad()
                loss.backward()
                _clip_and_step([(list(net.encoder.parameters()), 3.0, oe), (list(net.decoder.parameters()), 3.0, od)])
            else:
                segmenter_step(net, x, t, oe, od, 255, 3.0, 3.0, -1)
        return _cpu_sd(net)

    # ... and, from the second step on, re-packs the weights of all conv chains with one launch
    # at the start of the step (F.packed_once) instead of one per chain
    packs, call = [0], F.lib.call

    def counting(name, *args):
        packs[-1] += name == "nasseg_pack_weights"
        return call(name, *args)

    F.lib.call = counting
    try:
        batches.append(batches[0])
        a = run(False)
        packs.append(0)
        net = build_product_net(rec["kind"], rec["genotype"], rec["classes"], rec["dec_kwargs"], 0).to(DEV).train()
        oe = torch.optim.SGD(net.encoder.parameters(), lr=1e-3)
        od = torch.optim.SGD(net.decoder.parameters(), lr=1e-3)
        per_step = []
        for x, t in batches:
            packs.append(0)
            segmenter_step(net, x, t, oe, od, 255, 0.0, 0.0, -1)
            per_step.append(packs[-1])
    finally:
        F.lib.call = call
    assert per_step[0] > 10 and per_step[1] == 1 and per_step[2] == 1, per_step
    # the plan cache being emptied (it is, when it outgrows 4096 entries) must not leave a step with
    # weights packed into buffers nobody reads any more
    ref_net = build_product_net(rec["kind"], rec["genotype"], rec["classes"], rec["dec_kwargs"], 0).to(DEV).train()
    ref_net.load_state_dict(net.state_dict())
    oe2 = torch.optim.SGD(ref_net.encoder.parameters(), lr=1e-3)
    od2 = torch.optim.SGD(ref_net.decoder.parameters(), lr=1e-3)
    F._PACK_PLANS.clear()
    for x, t in batches:
        segmenter_step(net, x, t, oe, od, 255, 0.0, 0.0, -1)
        out = ref_net(x)
        loss = F.log_softmax_nll(out, F.nearest_label_resize(t, out.shape[2:]), 255)
        oe2.zero_grad()
        od2.zero_grad()
        loss.backward()
        oe2.step()
        od2.step()
    sd_a, sd_b = _cpu_sd(net), _cpu_sd(ref_net)
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), k
    b = run(True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_bench_prints_the_contract_line():
    """bench.py at a reduced size: ONE JSON line with the driver's fields; a plain run measures nothing beside the
    timed steps, --full adds the roofline of a kernel family measured live and the CPU baseline beside it"""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(*extra):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1",
                              "--batch", "2", "--height", "128", "--width", "256"] + list(extra),
                             capture_output=True, text=True, timeout=600, cwd=root)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        rec = json.loads(lines[0])
        for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                    "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
            assert key in rec, key
        assert rec["n_gpus"] == 1 and rec["steps"] == 2 and rec["warmup"] == 1 and rec["unit"] == "images/sec"
        assert rec["value"] > 0 and abs(rec["value"] * rec["ms_per_step"] / 1e3 - 2.0) < 1e-6  # batch 2 per step
        assert rec["higher_is_better"] is True and rec["scaling"] == "weak" and rec["vs_baseline"] is None
        assert rec["dtype"] == "f32" and rec["metric"].startswith("images/sec (fwd+bwd+optimizer step) WACV arch0")
        assert "workload" in rec["config"] and "model" not in rec["config"]
        return rec

    plain = run()
    assert plain["roofline"] is None and plain["cpu_baseline"] is None and plain["secondary"] is None
    rec = run("--full")
    roof = rec["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in roof, key
    assert roof["bound"] == "hbm" and roof["peak"] == 8000.0 and roof["achieved"] > 0
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-9
    cpu = rec["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in cpu, key
    assert cpu["kind"] == "port" and cpu["value"] > 0 and cpu["cores"] >= 1


def test_bench_dumps_what_its_last_timed_step_computed(tmp_path):
    """bench.py --dump-outputs at a reduced size: the last timed step's loss (the JSON line's), the parameters and
    BatchNorm buffers it left and the gradients it computed, as float32 / float64 .npy files.  A second run with the
    same arguments starts from the same inputs and weights and, the step being bit-reproducible, dumps the same bits."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(d):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1",
                              "--batch", "2", "--height", "128", "--width", "256", "--no-cpu-baseline", "--no-roofline",
                              "--pmc", "0", "--secondary", "0", "--dump-outputs", str(d)],
                             capture_output=True, text=True, timeout=600, cwd=root)
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads(out.stdout.strip().splitlines()[-1])

    rec = run(tmp_path / "a")
    files = sorted(os.listdir(tmp_path / "a"))
    got = {f[:-len(".npy")]: np.load(tmp_path / "a" / f) for f in files}
    assert rec["dumped_outputs"]["arrays"] == len(files) and not rec["dumped_outputs"]["sampled"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 10 ** 6
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert float(got["loss"][0]) == rec["config"]["loss"]
    genotype = [[[3, 0, 1], [4, 1, 1], [3, 1, 1]],
                [[0, 1, 0, 0, 1], [2, 1, 2, 1, 0], [3, 1, 1, 1, 0], [1, 1, 2, 0, 0],
                 [3, 0, 2, 0, 0], [5, 3, 2, 1, 0], [0, 5, 0, 1, 0]]]
    init = build_product_net("template", genotype, 19, dict(agg_size=64, repeats=2), 0)
    params = dict(init.named_parameters())
    assert set(got) == ({"loss"} | {"state." + k for k in init.state_dict()} | {"grad." + k for k in params})
    for k, v in init.state_dict().items():
        assert got["state." + k].shape == tuple(v.shape), k
    # the state is the one after the timed steps: the optimisers moved (almost) every parameter from its seeded start
    moved = sum(not np.array_equal(got["state." + k], v.detach().numpy()) for k, v in params.items())
    assert moved > 0.9 * len(params), (moved, len(params))
    run(tmp_path / "b")
    assert sorted(os.listdir(tmp_path / "b")) == files
    for f in files:
        assert np.array_equal(np.load(tmp_path / "b" / f), got[f[:-len(".npy")]]), f


def test_task0_with_knowledge_distillation_matches_reference_run(monkeypatch):
    """populate_task0(do_kd=True) caches the teacher's logits (bilinear to the first feature map) and
    train_task0 adds kd_coeff * kd_crit(output, kd_y) (src/engine/trainer.py:53-61,147-149): losses,
    the cached logits and the decoder after two steps against the reference's own run
    (tests/golden/engine_kd*, make_golden.py:gen_engine_kd).  The teacher is any module the caller
    hands in - here the recorded small conv net, running on torch's own GPU convolutions."""
    from nas_segm_amd.engine import RankParallel
    from nas_segm_amd.engine.trainer import populate_task0, train_task0

    monkeypatch.setenv("NASSEG_GRAPH", "0")
    rec = load_json("engine_kd_meta.json")
    npz = load_npz("engine_kd.npz")
    net = build_product_net(rec["kind"], rec["genotype"], rec["classes"], rec["dec_kwargs"], rec["seed"])
    segmenter = RankParallel(net.to(DEV))
    teacher = torch.nn.Sequential(torch.nn.Conv2d(3, 16, 3, stride=2, padding=1), torch.nn.ReLU(),
                                  torch.nn.Conv2d(16, rec["classes"], 3, stride=4, padding=1))
    teacher.load_state_dict({k[len("teacher/"):]: torch.from_numpy(npz[k]) for k in npz.files
                             if k.startswith("teacher/")})
    teacher = teacher.to(DEV).eval()
    loader = Loader([{"image": torch.from_numpy(npz["image/{}".format(i)]),
                      "mask": torch.from_numpy(npz["mask/{}".format(i)])} for i in range(4)])
    sens = rec["sensitivity"]
    bad = []

    def check(what, got, want, floor, rel=1e-4, abs_=1e-6):
        tol = rel * abs(want) + abs_ + 3.0 * floor
        if not abs(got - want) <= tol:
            bad.append("{}: {} vs {} (tol {:.3e}, floor {:.3e})".format(what, got, want, tol, floor))

    Xy = populate_task0.__wrapped__(segmenter, loader, teacher, 4, do_kd=True)
    assert list(Xy["kd_y"].shape) == rec["kd_y_shape"]
    check("cached teacher logits", checksums({"kd_y": Xy["kd_y"].float().cpu()})["kd_y"][1], rec["kd_y_checksum"][1],
          sens["kd_y"], rel=2e-5)
    values = _record_losses(monkeypatch)
    kd_values = []

    def kd_crit(inp, tgt):
        v = torch.nn.functional.mse_loss(inp, tgt)
        kd_values.append(float(v.detach()))
        return v

    optim_dec0 = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
    np.random.seed(321)
    ret = train_task0.__wrapped__(Xy, segmenter, optim_dec0, 0, _Crit(), kd_crit, 2, False, True, rec["kd_coeff"],
                                  3.0, False, aux_weight=max(rec["aux_weight"], 0))
    assert ret is None
    assert len(values) == len(rec["crit_values"]) and len(kd_values) == len(rec["kd_values"])
    for i, (v, w, f) in enumerate(zip(values, rec["crit_values"], sens["crit"])):
        check("segmentation loss {}".format(i), v, w, f, abs_=1e-4)
    for i, (v, w, f) in enumerate(zip(kd_values, rec["kd_values"], sens["kd"])):
        check("distillation loss {}".format(i), v, w, f, abs_=1e-5)
    # (zero-gradient parameters - see test_engine_matches_reference_run - are identified by the
    #  reference's end-to-end run of the same network)
    eng = ENG_META[rec["net"]]
    full_step = {k: eng["numel"][k] * 3e-3 * 2 for k in eng["numel"]}
    noise = {k for k, m in eng["task1_delta_mass"].items() if k.startswith("decoder.") and m < 0.05 * full_step[k]}
    got = checksums(_cpu_sd(net.decoder))
    for k, (s, sa) in rec["checksums"].items():
        if "num_batches_tracked" in k:
            assert got[k][0] == s, k
        elif ("decoder." + k) not in noise:
            check("decoder " + k, got[k][1], sa, sens["mass"][k])
    assert not bad, "{} of the reference run's numbers missed:\n{}".format(len(bad), "\n".join(bad[:40]))
