"""The fused distillation loss (nasseg_ce_mse_fwd / _bwd, functional.log_softmax_nll_mse), the multi-tensor Polyak
update (nasseg_polyak, engine/optim_native.PolyakStep) and the decoder-only step that uses them
(src/engine/trainer.py:144-149,167-169,270-272 with src/main_search.py:455-458's kd_crit = nn.MSELoss())."""
import copy

import numpy as np
import pytest
import torch

from _util import build_product_net, checksums, load_json, load_npz

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _F():
    from nas_segm_amd import functional as F

    return F


def _case(B, C, H, W, dtype, tdtype, seed, all_ignored=False):
    g = torch.Generator().manual_seed(seed)
    logits = (3 * torch.randn(B, C, H, W, generator=g)).to(dtype)
    teacher = 3 * torch.randn(B, C, H, W, generator=g)
    target = torch.randint(0, C, (B, H, W), generator=g)
    target[torch.rand(B, H, W, generator=g) < 0.2] = 255
    if all_ignored:
        target[:] = 255
    return logits, target.to(tdtype), teacher


def _reference(logits, target, teacher, a, b):
    """float64 on the CPU: NLL (mean over valid pixels), MSE (mean over all elements), d(a*nll + b*mse)/dlogits"""
    x = logits.double().detach().requires_grad_(True)
    t = target.long()
    valid = t != 255
    logp = torch.log_softmax(x, 1)
    picked = logp.gather(1, t.clamp(0, x.shape[1] - 1)[:, None])[:, 0]
    nll = -(picked * valid).sum() / valid.sum()
    mse = ((x - teacher.double()) ** 2).mean()
    (b * mse + (a * nll if a != 0 and bool(valid.any()) else 0)).backward()
    return float(nll), float(mse), x.grad


def _native(logits, target, teacher, a, b):
    F = _F()
    x = logits.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    tch = teacher.to(DEV).contiguous(memory_format=torch.channels_last)
    nll, mse = F.log_softmax_nll_mse(x, target.to(DEV), tch, 255)
    (a * nll + b * mse).backward() if a != 0 else (b * mse).backward()
    return float(nll.detach()), float(mse.detach()), x.grad.float().cpu()


@pytest.mark.parametrize("C", [19, 21, 64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("tdtype", [torch.int64, torch.uint8])
def test_fused_loss_against_float64(C, dtype, tdtype):
    """Values and gradients against torch in float64 on the CPU, P = 2*13*17 = 442 pixels (not a multiple of the
    256-pixel tile), 20 % ignored.  C = 64 takes the per-pixel path.  Tolerances: NLL and MSE relative 2e-6 (fp32
    accumulation of a few thousand terms); the gradient 2e-6 of its largest element in fp32, 1/128 of it in bf16
    (the gradient is stored in bf16: 8 significant bits)."""
    logits, target, teacher = _case(2, C, 13, 17, dtype, tdtype, seed=C)
    gtol = 2e-6 if dtype == torch.float32 else 2.0 ** -7
    for a, b in ((1.0, 0.0), (1.0, 0.3), (0.7, 2.5), (0.0, 1.0)):
        nll, mse, grad = _native(logits, target, teacher, a, b)
        rnll, rmse, rgrad = _reference(logits, target, teacher, a, b)
        assert abs(nll - rnll) <= 2e-6 * abs(rnll), (a, b, nll, rnll)
        assert abs(mse - rmse) <= 2e-6 * abs(rmse), (a, b, mse, rmse)
        err = float((grad.double() - rgrad).abs().max())
        assert err <= gtol * float(rgrad.abs().max()), (a, b, err, float(rgrad.abs().max()))


@pytest.mark.parametrize("C", [21, 64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_all_ignored_batch(C, dtype):
    """every pixel ignored: the NLL is 0/0 = NaN (as torch's), the MSE and its gradient are finite and the
    cross-entropy part of the gradient is zero"""
    logits, target, teacher = _case(2, C, 9, 31, dtype, torch.uint8, seed=7, all_ignored=True)
    nll, mse, grad = _native(logits, target, teacher, 1.0, 0.5)
    _, rmse, rgrad = _reference(logits, target, teacher, 0.0, 0.5)
    assert np.isnan(nll)
    assert abs(mse - rmse) <= 2e-6 * rmse
    tol = (2e-6 if dtype == torch.float32 else 2.0 ** -7) * float(rgrad.abs().max())
    assert torch.isfinite(grad).all() and float((grad.double() - rgrad).abs().max()) <= tol


@pytest.mark.parametrize("C", [19, 21, 64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("tdtype", [torch.int64, torch.uint8])
def test_nll_is_the_existing_kernels(C, dtype, tdtype):
    """the NLL and its gradient with no MSE gradient are bit-identical to F.log_softmax_nll's"""
    F = _F()
    logits, target, teacher = _case(3, C, 11, 29, dtype, tdtype, seed=100 + C)
    x1 = logits.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    x2 = logits.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    tgt = target.to(DEV)
    ref = F.log_softmax_nll(x1, tgt, 255)
    ref.backward()
    nll, mse = F.log_softmax_nll_mse(x2, tgt, teacher.to(DEV), 255)
    nll.backward()
    assert torch.equal(nll.detach().cpu(), ref.detach().cpu())
    assert torch.equal(x2.grad.float().cpu(), x1.grad.float().cpu())
    # (and with an explicit zero upstream gradient for the MSE)
    x3 = logits.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    n3, m3 = F.log_softmax_nll_mse(x3, tgt, teacher.to(DEV), 255)
    (n3 + 0.0 * m3).backward()
    assert torch.equal(x3.grad.float().cpu(), x1.grad.float().cpu())


def test_in_place_idiom_of_the_reference():
    """``loss = nll; loss += kd_coeff * mse; loss.backward()``: the outputs are tensors of their own, not views"""
    F = _F()
    logits, target, teacher = _case(2, 21, 16, 20, torch.float32, torch.int64, seed=3)
    x = logits.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    nll, mse = F.log_softmax_nll_mse(x, target.to(DEV), teacher.to(DEV), 255)
    assert nll.dim() == 0 and mse.dim() == 0 and not nll._is_view() and not mse._is_view()
    assert nll.untyped_storage().data_ptr() != mse.untyped_storage().data_ptr()
    loss = nll
    loss += 0.3 * mse
    loss.backward()
    _, _, rgrad = _reference(logits, target, teacher, 1.0, 0.3)
    assert float((x.grad.cpu().double() - rgrad).abs().max()) <= 2e-6 * float(rgrad.abs().max())


def test_refuses_a_teacher_that_does_not_fit():
    F = _F()
    logits, target, teacher = _case(2, 21, 8, 8, torch.float32, torch.int64, seed=4)
    x, tgt = logits.to(DEV), target.to(DEV)
    with pytest.raises(F.NassegError):
        F.log_softmax_nll_mse(x, tgt, teacher.to(DEV).double(), 255)
    with pytest.raises(F.NassegError):
        F.log_softmax_nll_mse(x, tgt, teacher.to(DEV).bfloat16(), 255)
    with pytest.raises(F.NassegError):
        F.log_softmax_nll_mse(x, tgt, teacher[:, :20].to(DEV), 255)
    with pytest.raises(F.NassegError):
        F.log_softmax_nll_mse(x, tgt, teacher[:1].to(DEV), 255)


@pytest.mark.parametrize("decay", [0.9, 0.99])
def test_polyak_equals_torch_bit_for_bit(decay):
    """nasseg_polyak over 300 tensors of 1, 3, 5, 4097 and 600 000 elements (one pair not 16-byte aligned) equals
    ``_polyak_update`` on the same GPU tensors bit for bit, over three steps"""
    from nas_segm_amd.engine.optim_native import PolyakStep
    from nas_segm_amd.engine.trainer import _polyak_update

    sizes = [1, 3, 5, 4097, 600000]
    g = torch.Generator().manual_seed(5)
    params = [torch.randn(sizes[i % len(sizes)], generator=g).to(DEV) for i in range(300)]
    base = torch.randn(4098, generator=g).to(DEV)
    params[3] = base[1:]  # (4097 elements 4 bytes past an aligned address: the scalar path)
    avg_native = [(p + torch.randn(p.shape, generator=g).to(DEV)).contiguous() for p in params]
    avg_torch = [a.clone() for a in avg_native]
    step = PolyakStep(params, avg_native)
    for it in range(3):
        step(decay)
        _polyak_update(params, avg_torch, decay)
        for i, (a, b) in enumerate(zip(avg_native, avg_torch)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (it, i, float((a - b).abs().max()))
        with torch.no_grad():
            for p in params:
                p.add_(torch.randn(p.shape, device=DEV) * 0.1)


# -- the decoder-only step -------------------------------------------------------------------------------------------
class _DS(object):
    def set_stage(self, stage):
        self.stage = stage


class _Loader(object):
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


def _kd_setup():
    """the recorded distillation run's network, teacher and cache (tests/golden/engine_kd*)"""
    from nas_segm_amd.engine import RankParallel
    from nas_segm_amd.engine.trainer import populate_task0

    rec = load_json("engine_kd_meta.json")
    npz = load_npz("engine_kd.npz")
    net = build_product_net(rec["kind"], rec["genotype"], rec["classes"], rec["dec_kwargs"], rec["seed"])
    teacher = torch.nn.Sequential(torch.nn.Conv2d(3, 16, 3, stride=2, padding=1), torch.nn.ReLU(),
                                  torch.nn.Conv2d(16, rec["classes"], 3, stride=4, padding=1))
    teacher.load_state_dict({k[len("teacher/"):]: torch.from_numpy(npz[k]) for k in npz.files
                             if k.startswith("teacher/")})
    batches = [{"image": torch.from_numpy(npz["image/{}".format(i)]), "mask": torch.from_numpy(npz["mask/{}".format(i)])}
               for i in range(4)]
    host_net = copy.deepcopy(net)
    segmenter = RankParallel(net.to(DEV))
    Xy = populate_task0.__wrapped__(segmenter, _Loader(batches), teacher.to(DEV).eval(), 4, do_kd=True)
    return rec, host_net, segmenter, Xy, batches


def _state(segmenter, optim):
    dec = segmenter.module.decoder if hasattr(segmenter, "module") else segmenter.decoder
    out = {"p/" + k: v.detach().clone() for k, v in dec.state_dict().items()}
    for i, (p, st) in enumerate(optim.state.items()):
        for k, v in st.items():
            out["s/{}/{}".format(i, k)] = v.detach().clone()
    return out


def test_kd_step_is_replayed_and_equals_host_launches(monkeypatch):
    """make_task0_step(do_kd=True, kd_crit=nn.MSELoss()) under NASSEG_GRAPH=1 returns a replayed stepper; five
    replayed steps and five native host-launched steps (NASSEG_GRAPH=0) from the same state agree bit for bit:
    losses, decoder parameters, BatchNorm buffers and Adam state"""
    from nas_segm_amd.engine import RankParallel
    from nas_segm_amd.engine.graphed import GraphedTask0Step
    from nas_segm_amd.engine.trainer import make_task0_step

    rec, host_net, segmenter, Xy, _ = _kd_setup()
    other = RankParallel(host_net.to(DEV))
    batches = [[0, 1], [2, 3], [1, 2], [3, 0], [0, 2]]
    results = []
    for mode, seg in (("1", segmenter), ("0", other)):
        monkeypatch.setenv("NASSEG_GRAPH", mode)
        dec = seg.module.decoder if hasattr(seg, "module") else seg.decoder
        dec.train()
        optim = torch.optim.Adam(dec.parameters(), lr=3e-3, weight_decay=1e-5)
        step = make_task0_step(Xy, seg, optim, 2, 255, 3.0, 0.15, False, True, 0.3, torch.nn.MSELoss())
        assert isinstance(getattr(step, "__self__", None), GraphedTask0Step) == (mode == "1")
        losses = [step(np.array(b)).detach().clone() for b in batches]
        torch.cuda.synchronize()
        results.append((losses, _state(seg, optim)))
    (la, sa), (lb, sb) = results
    assert all(torch.equal(a, b) for a, b in zip(la, lb)), (la, lb)
    assert sorted(sa) == sorted(sb)
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, bad[:20]


def test_recorded_kd_run_with_mse_loss_replayed(monkeypatch):
    """the reference's recorded distillation run (tests/golden/engine_kd*) with kd_crit = nn.MSELoss() and the step
    replayed: the per-step total loss - crit + kd_coeff * kd + aux_weight * (aux crits), rebuilt from the recorded
    crit_values and kd_values - and the decoder after two steps, with the tolerances of
    test_hip_engine.py::test_task0_with_knowledge_distillation_matches_reference_run"""
    from nas_segm_amd.engine import trainer

    monkeypatch.setenv("NASSEG_GRAPH", "1")
    rec, _, segmenter, Xy, _ = _kd_setup()
    sens = rec["sensitivity"]
    totals = []
    orig = trainer._loss_value

    def record(seg, loss):
        v = orig(seg, loss)
        totals.append(v)
        return v

    monkeypatch.setattr(trainer, "_loss_value", record)
    built = []
    orig_make = trainer.make_task0_step

    def make(*a, **k):
        step = orig_make(*a, **k)
        built.append(step)
        return step

    monkeypatch.setattr(trainer, "make_task0_step", make)
    net = segmenter.module if hasattr(segmenter, "module") else segmenter
    optim_dec0 = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
    np.random.seed(321)
    aux_w = max(rec["aux_weight"], 0)
    ret = trainer.train_task0.__wrapped__(Xy, segmenter, optim_dec0, 0, _Crit(), torch.nn.MSELoss(), 2, False, True,
                                          rec["kd_coeff"], 3.0, False, aux_weight=aux_w)
    assert ret is None
    from nas_segm_amd.engine.graphed import GraphedTask0Step

    assert isinstance(getattr(built[0], "__self__", None), GraphedTask0Step)
    crit, kd = rec["crit_values"], rec["kd_values"]
    per = len(crit) // len(kd)
    assert len(totals) == len(kd)
    bad = []
    for i, got in enumerate(totals):
        parts = [(1.0, crit[per * i], sens["crit"][per * i], 1e-4), (rec["kd_coeff"], kd[i], sens["kd"][i], 1e-5)]
        parts += [(aux_w, crit[per * i + j], sens["crit"][per * i + j], 1e-4) for j in range(1, per)]
        want = sum(w * v for w, v, _, _ in parts)
        tol = sum(w * (1e-4 * abs(v) + a + 3.0 * f) for w, v, f, a in parts)
        if not abs(got - want) <= tol:
            bad.append("total loss {}: {} vs {} (tol {:.3e})".format(i, got, want, tol))
    eng = load_json("engine_meta.json")[rec["net"]]
    full_step = {k: eng["numel"][k] * 3e-3 * 2 for k in eng["numel"]}
    noise = {k for k, m in eng["task1_delta_mass"].items() if k.startswith("decoder.") and m < 0.05 * full_step[k]}
    got = checksums({k: v.detach().cpu() for k, v in net.decoder.state_dict().items()})
    for k, (s, sa) in rec["checksums"].items():
        if "num_batches_tracked" in k:
            assert got[k][0] == s, k
        elif ("decoder." + k) not in noise:
            tol = 1e-4 * abs(sa) + 1e-6 + 3.0 * sens["mass"][k]
            if not abs(got[k][1] - sa) <= tol:
                bad.append("decoder {}: {} vs {} (tol {:.3e})".format(k, got[k][1], sa, tol))
    assert not bad, "\n".join(bad[:40])


@pytest.mark.parametrize("kind", ["sum", "function"])
def test_other_kd_criteria_are_called_every_step(monkeypatch, kind):
    """MSELoss(reduction="sum") and a plain function keep the host-launched step and are called once per step"""
    from nas_segm_amd.engine.trainer import make_task0_step

    monkeypatch.setenv("NASSEG_GRAPH", "1")
    rec, _, segmenter, Xy, _ = _kd_setup()
    calls = []

    def fn(inp, tgt):
        calls.append(1)
        return torch.nn.functional.mse_loss(inp, tgt)

    if kind == "sum":
        crit = torch.nn.MSELoss(reduction="sum")
        forward = crit.forward

        def counting(inp, tgt):
            calls.append(1)
            return forward(inp, tgt)

        crit.forward = counting  # (still exactly an nn.MSELoss: only its reduction keeps it off the fused path)
    else:
        crit = fn
    dec = segmenter.module.decoder if hasattr(segmenter, "module") else segmenter.decoder
    optim = torch.optim.Adam(dec.parameters(), lr=3e-3)
    step = make_task0_step(Xy, segmenter, optim, 2, 255, 3.0, 0.15, False, True, 0.3, crit)
    assert getattr(step, "__self__", None) is None
    for b in ([0, 1], [2, 3], [1, 3]):
        step(np.array(b))
    assert len(calls) == 3


def _avg_runs(monkeypatch, run):
    """what ``run()`` returns (avg_param after its epoch) with the native update, then with ``_polyak_update``"""
    from nas_segm_amd.engine import optim_native

    out = []
    for native in (True, False):
        if not native:
            monkeypatch.setattr(optim_native, "polyak_update", lambda *a, **k: False)
        out.append(run())
    monkeypatch.undo()
    return out


def test_polyak_in_the_trainers(monkeypatch):
    """train_task0 and train_segmenter with do_polyak=True: avg_param equals, bit for bit, what ``_polyak_update``
    after every step of an identical run produces"""
    from nas_segm_amd.engine import RankParallel
    from nas_segm_amd.engine.optim_native import PolyakStep
    from nas_segm_amd.engine.trainer import train_segmenter, train_task0

    rec, host_net, _, _, batches = _kd_setup()
    launched = []
    orig_call = PolyakStep.__call__

    def counting(self, decay):
        launched.append(decay)
        return orig_call(self, decay)

    monkeypatch.setattr(PolyakStep, "__call__", counting)

    def task0():
        from nas_segm_amd.engine.trainer import populate_task0

        net = copy.deepcopy(host_net).to(DEV)
        seg = RankParallel(net)
        Xy = populate_task0.__wrapped__(seg, _Loader(batches), None, 4, do_kd=False)
        avg = [p.data.clone() for p in net.decoder.parameters()]
        optim = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
        np.random.seed(5)
        train_task0.__wrapped__(Xy, seg, optim, 0, _Crit(), None, 2, False, False, 0.0, 3.0, True, avg_param=avg,
                                polyak_decay=0.9, aux_weight=0.15)
        return [a.cpu() for a in avg]

    def task1():
        net = copy.deepcopy(host_net).to(DEV)
        seg = RankParallel(net)
        avg = [p.data.clone() for p in seg.parameters()]
        o_enc = torch.optim.SGD(net.encoder.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-5)
        o_dec = torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
        train_segmenter.__wrapped__(seg, _Loader(batches), o_enc, o_dec, 0, _Crit(), False, 1.0, 3.0, True,
                                    aux_weight=0.15, avg_param=avg, polyak_decay=0.99)
        return [a.cpu() for a in avg]

    for run in (task0, task1):
        monkeypatch.setattr(PolyakStep, "__call__", counting)
        del launched[:]
        native, reference = _avg_runs(monkeypatch, run)
        assert launched, run.__name__  # (the native path did run)
        assert len(native) == len(reference)
        for i, (a, b) in enumerate(zip(native, reference)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (run.__name__, i)
