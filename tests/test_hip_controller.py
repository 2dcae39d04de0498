"""The native search controller on the device (csrc/controller.hip, functional.controller_*, rl/): rollout, backward
through time, sampling, PPO and REINFORCE against the reference's float64 records (tests/golden/controller_rollout_*)
and the float64 restatement (tests/_controller_ref.py, pinned to those records by tests/test_controller_host.py).

Tolerances are not tuned to the kernels: the yardstick of a quantity is the REFERENCE's own fp32 error against its
float64 run (both recorded); the kernel may be off from float64 by 4 x that - another summation order, expf-based
sigmoid and tanh - plus a floor of 4 fp32 ulps of the tensor's largest entry.

Measured on an MI355X, largest error against float64 as a fraction of the tensor's largest entry, reference's own
fp32 run / kernel: log-probabilities 3.0e-07 / 3.0e-07 (wacv7; 9.4e-08 / 9.4e-08 cvpr), entropy 2.9e-09 / 1.2e-07
(wacv7: two ulps of 62.5, a running fp32 sum over 44 steps); gradients from log_prob alone 1.2e-06 / 1.1e-06
(wacv_h12), from the entropy alone 1.4e-05 / 3.4e-07 (cvpr_h7; the kernel differentiates the entropy through the
logits centred on their mean, the reference through log p + H, two numbers of size log n), from the mix 1.2e-06 /
1.1e-06.  PPO replay, parameters afterwards, kernel against the record / fp32 against float64 restatement: cvpr 4.3e-06
/ 6.6e-06, wacv7 4.8e-07 / 5.1e-07, cvpr_h7 1.5e-08 / 9.7e-09, wacv_h12 2.6e-08 / 4.9e-08.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import _controller_ref as R
from _controller_ref import load_case, product

CASES = sorted(R.CASES)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
ULP = 2.0 ** -23


def tol(ref_err, truth):
    return 4.0 * ref_err + 4.0 * ULP * float(np.abs(np.asarray(truth)).max())


@functools.lru_cache(maxsize=None)
def fixture(case):
    """(meta, records, fp32 state_dict, float64 gradients {objective: {name: array}}) - computed once, never
    modified"""
    meta, data, sd = load_case(case)
    kind, kw = R.CASES[case]
    w = torch.tensor(meta["w"], dtype=torch.float64)
    grads = {}
    for obj in ("lp", "ent", "mix"):
        params = R.leaf_params(sd, torch.float64)
        lp, ent = R.evaluate(params, kind, kw, data["actions"].tolist())
        {"lp": (lp * w).sum(), "ent": ent, "mix": (lp * w).sum() + 0.3 * ent}[obj].backward()
        grads[obj] = {k: p.grad.numpy() for k, p in params.items() if p.grad is not None}
    return meta, data, sd, grads


def controller(case):
    meta, data, sd, _ = fixture(case)
    ctrl = product(*R.CASES[case])
    ctrl.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    return ctrl.to(DEV)


@pytest.mark.parametrize("case", CASES)
def test_forward_matches_the_float64_records(case):
    meta, data, sd, _ = fixture(case)
    ctrl = controller(case)
    lp, ents = ctrl.evaluate_actions(data["actions"])
    lp, ents = lp.detach().cpu().numpy().astype(np.float64), ents.detach().cpu().numpy().astype(np.float64)
    ref_lp, ref_ent = np.abs(data["lp32"] - data["lp64"]).max(), np.abs(data["ent32"] - data["ent64"]).max()
    print(case, "log_prob: reference", ref_lp, "kernel", np.abs(lp - data["lp64"]).max(), "| entropy: reference",
          ref_ent, "kernel", np.abs(ents - data["ent64"]).max())
    assert np.abs(lp - data["lp64"]).max() <= tol(ref_lp, data["lp64"])
    assert np.abs(ents - data["ent64"]).max() <= tol(ref_ent, data["ent64"])
    assert np.all(ents == ents[0])
    for b in (0, 5):  # the single-row calls give the batch's values, bit for bit
        config, e1, l1 = ctrl.evaluate(data["actions"][b].tolist())
        assert float(l1) == float(np.float32(lp[b])) and float(e1) == float(np.float32(ents[0]))
        assert ctrl.config2action(config) == data["actions"][b].tolist()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("objective", ["lp", "ent", "mix"])
def test_backward_matches_float64(case, objective):
    """every parameter's gradient through F.controller_rollout and .backward(): from log_prob alone, from entropy
    alone and from the mix; the mix also against the reference's float64 RECORD where it is kept"""
    from nas_segm_amd import functional as F

    meta, data, sd, grads = fixture(case)
    ctrl = controller(case)
    actions = torch.from_numpy(data["actions"]).to(DEV)
    entropy, lp = F.controller_rollout(ctrl.plan, ctrl.table_parameters(), actions)
    assert entropy.shape == () and lp.shape == (6,) and entropy._base is None and lp._base is None
    w = torch.tensor(meta["w"], dtype=torch.float32, device=DEV)
    if objective == "mix":
        loss = entropy
        loss *= 0.3  # (in place on the results themselves: they are no views)
        loss += (lp * w).sum()
    else:
        loss = (lp * w).sum() if objective == "lp" else entropy
    loss.backward()
    assert ctrl.enc_op.weight.grad is None
    worst = (0.0, 0.0)
    for k, p in ctrl.named_parameters():
        if k == "enc_op.weight":
            continue
        got, want = p.grad.cpu().numpy().astype(np.float64), grads[objective][k]
        ref = meta["cases"][case]["ref_err"][objective][k]
        err, top = np.abs(got - want).max(), np.abs(want).max()
        if top > 0:  # (a head with one choice has a zero gradient)
            worst = max(worst, (err / top, ref / top))
        assert err <= tol(ref, want), (k, err, ref, top)
        if objective == "mix":
            rec = data["grad64/" + k]
            assert np.abs(R.recorded(k, got) - rec).max() <= tol(ref, rec), k
    print(case, objective, "largest gradient error / largest entry: kernel {:.2e}, reference {:.2e}".format(*worst))


# small hidden sizes with many choices: a head's weight (n x H) is then wider than an LSTM weight (4H x H), the
# entry the parameter-gradient launch was once sized by alone (H = 8: 256 elements against 320; H = 5: 100 against 320)
WIDE_HEADS = {
    "h8_n40": ("wacv", dict(enc_num_layers=2, num_ops=40, num_agg_ops=2, lstm_hidden_size=8, lstm_num_layers=1,
                            dec_num_cells=1, cell_num_layers=2)),
    "h5_n64": ("cvpr", dict(enc_num_layers=2, num_ops=64, lstm_hidden_size=5, lstm_num_layers=2, dec_num_cells=1,
                            cell_num_layers=2)),
}


@pytest.mark.parametrize("case", sorted(WIDE_HEADS))
def test_backward_with_heads_wider_than_the_lstm_weights(case):
    """every gradient entry against the float64 restatement (no fixture: parameters and actions from a seed); the
    yardstick is the fp32 restatement's own distance from float64, the bound 4 x that plus 4 ulps, as above"""
    from nas_segm_amd import functional as F

    kind, kw = WIDE_HEADS[case]
    torch.manual_seed(31)
    ctrl = product(kind, kw)
    sd = {k: v.clone().numpy() for k, v in ctrl.state_dict().items()}
    heads = [(name, pos) for name, pos in R.steps_of(kind, kw) if name is not None]
    rng = np.random.RandomState(5)
    actions = np.zeros((4, ctrl.action_size()), dtype=np.int32)
    for name, pos in heads:
        actions[:, pos] = rng.randint(0, sd[name + ".weight"].shape[0], size=4)
    assert max(sd[name + ".weight"].size for name, _ in heads) > sd["rnn.weight_ih_l0"].size
    w = [0.7, -1.3, 0.4, 1.1]
    ref = {}
    for dtype in (torch.float32, torch.float64):
        params = R.leaf_params(sd, dtype)
        lp, ent = R.evaluate(params, kind, kw, actions.tolist())
        ((lp * torch.tensor(w, dtype=dtype)).sum() + 0.3 * ent).backward()
        ref[dtype] = {k: p.grad.double().numpy() for k, p in params.items() if p.grad is not None}
    ctrl = ctrl.to(DEV)
    entropy, lp = F.controller_rollout(ctrl.plan, ctrl.table_parameters(), torch.from_numpy(actions).to(DEV))
    ((lp * torch.tensor(w, device=DEV)).sum() + 0.3 * entropy).backward()
    for k, p in ctrl.named_parameters():
        if k == "enc_op.weight":
            assert p.grad is None
            continue
        got, want = p.grad.cpu().numpy().astype(np.float64), ref[torch.float64][k]
        yard = float(np.abs(ref[torch.float32][k] - want).max())
        err = float(np.abs(got - want).max())
        print(case, k, "kernel", err, "fp32 restatement", yard, "largest entry", float(np.abs(want).max()))
        assert np.all(np.isfinite(got)) and err <= tol(yard, want), (k, err, yard)


@pytest.mark.parametrize("case", CASES)
def test_sampling_is_the_float64_inverse_cdf(case):
    meta, data, sd, _ = fixture(case)
    kind, kw = R.CASES[case]
    ctrl = controller(case)
    tables = R.cdf_tables(R.leaf_params(sd, torch.float64), kind, kw)
    steps = [t for t, (name, _) in enumerate(R.steps_of(kind, kw)) if name is not None]
    T, rows = ctrl.plan.T, max(len(c) for c, _ in tables)
    u = np.full((rows + 2, T), 0.5, dtype=np.float32)
    want = np.zeros((rows + 2, ctrl.action_size()), dtype=np.int64)
    hit = [set() for _ in tables]
    for s in range(rows):
        for j, (t, (cdf, pos)) in enumerate(zip(steps, tables)):
            i = s % len(cdf)
            lo, hi = (cdf[i - 1] if i else 0.0), cdf[i]
            assert (hi - lo) / 2 >= 0.5 / 64, (case, t, i)  # the midpoint is far from both boundaries
            u[s, t] = np.float32((lo + hi) / 2)
            want[s, pos] = i
            hit[j].add(i)
    assert all(h == set(range(len(c))) for h, (c, _) in zip(hit, tables))  # every choice of every head
    u[rows, :] = 0.0
    u[rows + 1, :] = np.nextafter(np.float32(1.0), np.float32(0.0))
    for cdf, pos in tables:
        want[rows + 1, pos] = len(cdf) - 1
    ud = torch.from_numpy(u).to(DEV)
    out = ctrl.sample_given(ud)
    got = np.array([ctrl.config2action(cfg) for cfg, _, _ in out])
    assert np.array_equal(got, want)
    lp, _ = ctrl.evaluate_actions(got)
    assert torch.equal(torch.stack([o[2] for o in out]), lp.detach())  # bit for bit
    single = [ctrl.sample_given(ud[s:s + 1])[0] for s in range(rows + 2)]
    for a, b in zip(out, single):
        assert a[0] == b[0] and torch.equal(a[2], b[2]) and torch.equal(a[1], b[1])
    torch.manual_seed(4)
    first = ctrl.sample_many(3)
    torch.manual_seed(4)
    again = ctrl.sample_many(3)
    assert [c for c, _, _ in first] == [c for c, _, _ in again]  # torch.manual_seed reproduces a draw


@pytest.mark.parametrize("case", ["cvpr", "wacv_h12"])
def test_rollout_and_backward_repeat_bit_for_bit_and_under_graph_replay(case):
    from nas_segm_amd import functional as F

    meta, data, sd, _ = fixture(case)
    ctrl = controller(case)
    plan, params = ctrl.plan, [p.detach() for p in ctrl.table_parameters()]
    actions = torch.from_numpy(data["actions"]).to(DEV)
    d_lp = torch.tensor(meta["w"], dtype=torch.float32, device=DEV)
    d_ent = torch.tensor(0.3, dtype=torch.float32, device=DEV)

    def run():
        entropy, lp, saved, _, _ = F.controller_forward(plan, params, actions)
        flat = F.controller_backward(plan, params, saved, actions, None, d_lp, d_ent)
        # (the gradients are slices of `flat`; the padding between them is never written)
        return [entropy, lp] + [g.clone() for g in plan.split(flat)]

    a = [t.clone() for t in run()]
    b = [t.clone() for t in run()]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = run()
    for t in held:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, held):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert any(float(g.abs().max()) > 0 for g in a[2:])


@pytest.mark.parametrize("case", CASES)
def test_ppo_update_replays_the_record(case):
    """the recorded PPO.update with the recorded minibatch order: loss, entropy and parameters against the record;
    margin: the fp32 restatement's distance from the float64 restatement over the same update, x 4, plus 4 ulps"""
    from nas_segm_amd.rl.gradient_estimators import PPO

    meta, data, sd, _ = fixture(case)
    kind, kw = R.CASES[case]
    rec, args = meta["cases"][case], meta["ppo_args"]
    ctrl = controller(case)
    agent = PPO(ctrl, action_size=ctrl.action_size(), **args)
    actions, old, rewards = data["ppo/actions"], data["ppo/old_log_probs"], data["ppo/rewards"]
    for k in range(5):
        assert agent.update((float(rewards[k]), actions[k].tolist(), float(old[k])), is_train=False) == (-1, -1)
    order = data["ppo/order"].tolist()
    loss, entropy = agent.update((float(rewards[5]), actions[5].tolist(), float(old[5])), batches=order)
    assert agent.baseline == rec["ppo_baseline"]
    adv = rewards - rec["ppo_baseline"]
    ref = {}
    for dtype in (torch.float32, torch.float64):
        ref[dtype] = R.ppo_update(sd, kind, kw, actions.tolist(), old.astype(np.float32).astype(np.float64),
                                  adv.astype(np.float32).astype(np.float64), order, args["clip_param"],
                                  args["entropy_coef"], args["lr"], 2.0, dtype)
    l32, e32, p32 = ref[torch.float32]
    l64, e64, p64 = ref[torch.float64]
    print(case, "loss", loss, rec["ppo_loss"], l64, "entropy", entropy, rec["ppo_entropy"], e64)
    # (the loss is a mean of terms ratio x advantage, ratio near 1: its rounding scales with the largest advantage)
    assert abs(loss - rec["ppo_loss"]) <= tol(abs(l32 - l64), np.abs(adv).max())
    assert abs(entropy - rec["ppo_entropy"]) <= tol(abs(e32 - e64), e64)
    worst = (0.0, 0.0)
    for k, p in ctrl.state_dict().items():
        got, want = R.recorded(k, p.cpu().numpy()), data["ppo/after/" + k]
        dev = float((p32[k].double() - p64[k]).abs().max())
        err = float(np.abs(got - want).max())
        worst = max(worst, (err, dev))
        assert err <= tol(dev, want), (k, err, dev)
    print(case, "parameters after: kernel vs record {:.2e}, fp32 vs float64 restatement {:.2e}".format(*worst))
    assert torch.equal(ctrl.enc_op.weight.cpu(), torch.from_numpy(sd["enc_op.weight"]))


@pytest.mark.parametrize("case", ["cvpr", "wacv_h12"])
def test_ppo_is_reproduced_by_the_seed(case):
    from nas_segm_amd.rl.gradient_estimators import PPO

    meta = fixture(case)[0]

    def run():
        ctrl = controller(case)
        agent = PPO(ctrl, action_size=ctrl.action_size(), **meta["ppo_args"])
        torch.manual_seed(123)
        for k in range(20):
            config, entropy, log_prob = ctrl.sample()
            action = ctrl.config2action(config)
            agent.update((0.01 * (sum(action) % 17), action, log_prob))
        return [p.detach().clone() for p in ctrl.parameters()], agent.rollouts.actions.copy()

    (pa, aa), (pb, ab) = run(), run()
    assert np.array_equal(aa, ab) and all(torch.equal(x, y) for x, y in zip(pa, pb))
    start = controller(case)
    assert any(not torch.equal(x, y) for x, y in zip(pa, start.parameters()))


@pytest.mark.parametrize("case", ["cvpr", "wacv_h12"])
def test_reinforce_follows_the_restatement(case):
    from nas_segm_amd.rl.gradient_estimators import REINFORCE

    meta, data, sd, _ = fixture(case)
    kind, kw = R.CASES[case]
    ctrl = controller(case)
    agent = REINFORCE(ctrl, lr=1e-3, baseline_decay=0.95)
    samples = [(r, data["actions"][k].tolist()) for k, r in enumerate((0.31, 0.12, 0.45))]
    losses = []
    for reward, action in samples:
        loss, entropy = agent.update((reward, action, torch.tensor(0.0)))  # (what train_agent passes)
        losses.append(float(loss))
    l32, b32, p32 = R.reinforce_updates(sd, kind, kw, samples, 0.95, 1e-3, 2.0, torch.float32)
    l64, b64, p64 = R.reinforce_updates(sd, kind, kw, samples, 0.95, 1e-3, 2.0, torch.float64)
    assert agent.baseline == b64[-1] == b32[-1]  # python floats: exact
    for got, a, b in zip(losses, l32, l64):
        assert abs(got - b) <= tol(abs(a - b), b), (got, a, b)
    assert losses[0] == 0.0 and abs(losses[2]) > 0  # the first advantage is zero
    for k, p in ctrl.state_dict().items():
        dev = float((p32[k].double() - p64[k]).abs().max())
        err = float((p.cpu().double() - p64[k]).abs().max())
        assert err <= tol(dev, p64[k].numpy()), (k, err, dev)
    assert float((ctrl.g_emb.cpu() - torch.from_numpy(sd["g_emb"])).abs().max()) > 0


@pytest.mark.parametrize("version", ["cvpr", "wacv"])
def test_search_loop_end_to_end(version):
    """search_loop with the native agent and a fake evaluation: rewards reach the buffer in order, the parameters
    move, the sampled configs build decoders, and a saved agent continues bit for bit"""
    from nas_segm_amd.engine.search import search_loop
    from nas_segm_amd.nn.micro_decoders import MicroDecoder, TemplateDecoder
    from nas_segm_amd.rl.agent import create_agent, train_agent

    def make():
        return create_agent(enc_num_layers=4 if version == "cvpr" else 2, num_ops=11 if version == "cvpr" else 6,
                            num_agg_ops=2, lstm_hidden_size=100, lstm_num_layers=2, dec_num_cells=3,
                            cell_num_layers=4 if version == "cvpr" else 7, cell_max_repeat=4, cell_max_stride=2,
                            ctrl_lr=1e-3, ctrl_baseline_decay=0.95, ctrl_agent="ppo", ctrl_version=version,
                            device=DEV)

    def flat(x):
        return [v for item in x for v in flat(item)] if isinstance(x, list) else [x]

    def score(config):
        return (sum((i + 1) * v for i, v in enumerate(flat(config))) % 23) / 23.0

    def loop(agent, n):
        return search_loop(agent.controller.sample, lambda s: train_agent(agent, s), score, n)

    torch.manual_seed(7)
    agent = make()
    before = [p.detach().clone() for p in agent.controller.parameters()]
    history = loop(agent, 4)
    assert len(history) == 4 and agent.rollouts.step == 4
    assert np.allclose(agent.rollouts.rewards[:4, 0], [r for _, r in history], rtol=0, atol=0)
    for k, (config, reward) in enumerate(history):
        assert reward == score(config)
        assert agent.rollouts.actions[k].tolist() == agent.controller.config2action(config)
        if version == "cvpr":
            MicroDecoder([24, 32, 96, 320], 21, config, agg_size=48, aux_cell=True, repeats=1)
        else:
            TemplateDecoder([24, 32], 19, config, agg_size=48, repeats=1)
    assert any(not torch.equal(a, b) for a, b in zip(before, agent.controller.parameters()))
    state = copy.deepcopy(agent.state_dict())
    assert sorted(state) == ["baseline", "controller", "optimizer", "rollouts"]
    other = make()
    other.load_state_dict(state)
    torch.manual_seed(11)
    h1 = loop(agent, 2)
    torch.manual_seed(11)
    h2 = loop(other, 2)
    assert h1 == h2
    for a, b in zip(agent.controller.parameters(), other.controller.parameters()):
        assert torch.equal(a, b)
