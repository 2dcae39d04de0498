"""Host side of the native search controller (rl/, helpers/storage.py, csrc/controller.hip), no GPU:
the torch-op restatement (tests/_controller_ref.py) reproduces what the REFERENCE controller recorded
(tests/golden/controller_rollout_*.npz, written by golden/make_controller_golden.py) - fp32 against the fp32 records,
float64 against the float64 ones -, the modules' step tables and action maps, the rollout storage, the drop-in names
and the header entries."""
import os
import pickle

import numpy as np
import pytest
import torch

import _controller_ref as R
from _controller_ref import load_case, product
from _util import GOLDEN, load_json

CASES = sorted(R.CASES)


def test_the_fixture_files_are_small_and_cover_the_cases():
    meta = load_json("controller_rollout_meta.json")
    assert sorted(meta["cases"]) == CASES
    total = 0
    for case in CASES:
        total += os.path.getsize(os.path.join(GOLDEN, "controller_rollout_{}.npz".format(case)))
    assert total + os.path.getsize(os.path.join(GOLDEN, "controller_rollout_meta.json")) < 2e6
    kind, kw = R.CASES["cvpr"]
    assert len(R.steps_of(kind, kw)) == 23 and R.action_size(kind, kw) == 20
    kind, kw = R.CASES["wacv7"]
    assert len(R.steps_of(kind, kw)) == 48 and R.action_size(kind, kw) == 44
    assert ("dummy_stride_op", 43) in R.steps_of(kind, kw)  # the head with one choice


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_restatement_reproduces_the_reference_records(case, dtype):
    """log-probabilities, entropy and every recorded gradient entry: the fp32 restatement against the reference's
    fp32 run, the float64 one against its float64 run (large tensors: every 8th row entry by entry, every row through
    its sum).  Bounds: float64 - 1e-12 relative (two float64 programs with
    other summation orders); fp32 - the reference's own fp32-vs-float64 error of that tensor, twice (two fp32 programs,
    each that far from the exact value), plus 4 ulps of the tensor's largest entry."""
    meta, data, sd = load_case(case)
    kind, kw = R.CASES[case]
    tag = "32" if dtype == torch.float32 else "64"
    params = R.leaf_params(sd, dtype)
    actions = data["actions"].tolist()
    lp, ent = R.evaluate(params, kind, kw, actions)
    w = torch.tensor(meta["w"], dtype=dtype)
    ((lp * w).sum() + 0.3 * ent).backward()
    eps = 1e-12 if tag == "64" else 2.0 ** -23
    lp_ref, ent_ref = data["lp" + tag], data["ent" + tag]
    lp_tol = 1e-12 * 64 if tag == "64" else 2 * np.abs(data["lp32"] - data["lp64"]).max() + 4 * eps * 64
    assert np.abs(lp.detach().numpy() - lp_ref).max() <= lp_tol
    assert np.abs(float(ent) - ent_ref).max() <= lp_tol
    assert np.all(ent_ref == ent_ref[0])  # every sample of a controller has the same entropy
    assert params["enc_op.weight"].grad is None and "grad64/enc_op.weight" not in data
    checked = 0
    for k, p in params.items():
        if k == "enc_op.weight":
            continue
        got, want = R.recorded(k, p.grad.numpy()), data["grad{}/{}".format(tag, k)]
        assert got.shape == want.shape, k
        top = np.abs(want).max()
        tol = 1e-12 * top if tag == "64" else 2 * meta["cases"][case]["ref_err"]["mix"][k] + 4 * eps * top
        assert np.abs(got - want).max() <= tol, (k, np.abs(got - want).max(), tol)
        if p.numel() > R.BIG:  # every row of a large tensor, through its sum (float64 record)
            sums = data["grad64_rowsum/" + k]
            assert sums.shape == (p.shape[0],)
            assert np.abs(p.grad.double().numpy().sum(axis=1) - sums).max() <= p.shape[1] * tol, k
        checked += 1
    assert checked == len(sd) - 1


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_recorded_ppo_update(case):
    """the fp32 restatement, fed the recorded buffer and minibatch order, lands where the reference's PPO.update did:
    loss, entropy and every recorded parameter entry.  Adam divides by sqrt(v) of gradients near zero, so two fp32
    programs agree only to a fraction of the step: 1 % of the largest movement."""
    meta, data, sd = load_case(case)
    kind, kw = R.CASES[case]
    rec, args = meta["cases"][case], meta["ppo_args"]
    adv = (data["ppo/rewards"] - rec["ppo_baseline"]).astype(np.float32)
    loss, ent, after = R.ppo_update(sd, kind, kw, data["ppo/actions"].tolist(),
                                    data["ppo/old_log_probs"].astype(np.float32), adv, data["ppo/order"].tolist(),
                                    args["clip_param"], args["entropy_coef"], args["lr"], 2.0, torch.float32)
    assert abs(loss - rec["ppo_loss"]) <= 1e-5 * max(1.0, abs(rec["ppo_loss"]))
    assert abs(ent - rec["ppo_entropy"]) <= 1e-5 * abs(rec["ppo_entropy"])
    assert rec["ppo_moved"] > 1e-3
    for k, v in after.items():
        want = data["ppo/after/" + k]
        assert np.abs(R.recorded(k, v.numpy()) - want).max() <= 1e-2 * rec["ppo_moved"], k
        if v.numel() > R.BIG:  # every row, through its sum
            sums = data["ppo/after_rowsum/" + k]
            assert np.abs(v.double().numpy().sum(axis=1) - sums).max() <= v.shape[1] * 1e-2 * rec["ppo_moved"], k
    assert np.array_equal(after["enc_op.weight"].numpy(), sd["enc_op.weight"])  # no gradient: Adam skips it


@pytest.mark.parametrize("case", CASES)
def test_step_tables_and_state_dict_layout(case):
    """T, the choices per step and the action-position map of the product's table against the restatement's own
    enumeration; parameter names, shapes and ORDER against the reference's recorded state_dict"""
    meta, data, sd = load_case(case)
    kind, kw = R.CASES[case]
    ctrl = product(kind, kw)
    want = R.steps_of(kind, kw)
    plan = ctrl.plan
    assert plan.T == len(want) and plan.A == R.action_size(kind, kw) == ctrl.action_size()
    assert plan.H == R.defaults(kind, kw)["lstm_hidden_size"] and plan.L == R.defaults(kind, kw)["lstm_num_layers"]
    names = {id(m): n for n, m in ctrl.named_modules()}
    for (head, n, pos), (name, wpos) in zip(plan.steps, want):
        if name is None:
            assert (head, n, pos) == (-1, 0, -1)
        else:
            assert names[id(ctrl._heads[head])] == name and pos == wpos
            assert n == sd[name + ".weight"].shape[0] == plan.head_rows[head]
    positions = sorted(pos for _, _, pos in plan.steps if pos >= 0)
    assert positions == list(range(1 if kind == "cvpr" else 0, plan.A))  # every position once; CVPR's first: a dummy
    got = ctrl.state_dict()
    assert list(got) == list(sd)
    assert [k for k, _ in ctrl.named_parameters()] == [k for k in sd]  # (optimiser state indices line up)
    for k, v in got.items():
        assert tuple(v.shape) == sd[k].shape, k
        assert float(v.abs().max()) <= 0.1
    ctrl.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    assert len(ctrl.table_parameters()) == 1 + 4 * plan.L + 2 * plan.NH == len(plan.shapes)
    for p, shape in zip(ctrl.table_parameters(), plan.shapes):
        assert p.numel() == int(np.prod(shape))
    assert all(o % 4 == 0 for o in plan.offsets) and plan.total >= sum(plan.numels)


def test_config_action_round_trip_on_the_reference_samples():
    from nas_segm_amd.rl.micro_controllers import MicroController, TemplateController

    ctrl = load_json("controller.json")
    for s in ctrl["cvpr"]["samples"]:
        assert MicroController.config2action(s["config"]) == s["action"]
        assert MicroController.action2config(s["action"], as_sampled=True) == s["config"]
        ref_style = MicroController.action2config(s["action"])  # ([0, op] for the first layer, as evaluate makes it)
        assert ref_style[0][0] == [0, s["config"][0][0]] and ref_style[1] == s["config"][1]
        assert MicroController.config2action(ref_style) == s["action"]
    for s in ctrl["wacv"]["samples"]:
        assert TemplateController.config2action(s["config"]) == s["action"]
        assert TemplateController.action2config(s["action"], dec_block=3, ctx_block=7) == s["config"]
    assert len(MicroController.get_mock()) == 3 and len(TemplateController.get_mock()) == 4


def test_rollout_storage_insert_wraps_and_generates():
    from nas_segm_amd.helpers.storage import RolloutStorage

    st = RolloutStorage(3, 1, 4)
    assert st.actions.shape == (3, 4) and st.action_log_probs.shape == (3, 1) and st.rewards.shape == (3, 1)
    for k in range(4):
        st.insert([k, k + 1, k + 2, k + 3], torch.tensor(-1.0 - k), 0.1 * k)
    assert st.step == 1  # wrapped around: the fourth insert replaced the first
    assert st.actions[0].tolist() == [3, 4, 5, 6] and st.actions[1].tolist() == [1, 2, 3, 4]
    assert st.action_log_probs[:, 0].tolist() == [-4.0, -2.0, -3.0]
    assert np.allclose(st.rewards[:, 0], [0.3, 0.1, 0.2])
    adv = st.rewards - 0.2
    torch.manual_seed(5)
    got = list(st.generator(adv, 3))
    torch.manual_seed(5)
    order = st.batches(3)
    assert sorted(i for b in order for i in b) == [0, 1, 2] and len(got) == 3
    for (a, r, lp, ad), rows in zip(got, order):
        assert np.array_equal(a, st.actions[rows]) and np.array_equal(r, st.rewards[rows])
        assert np.array_equal(lp, st.action_log_probs[rows]) and np.array_equal(ad, adv[rows])
    back = pickle.loads(pickle.dumps(st))
    assert sorted(vars(back)) == ["action_log_probs", "actions", "num_processes", "num_steps", "rewards", "step"]
    assert np.array_equal(back.actions, st.actions)


def test_install_dropin_maps_the_controller_only_when_asked():
    import subprocess
    import sys

    code = ("import sys, nas_segm_amd; names = nas_segm_amd.install_dropin();"
            "assert not any(n in names or n in sys.modules for n in ('rl.micro_controllers', 'rl.agent', "
            "'rl.gradient_estimators', 'helpers.storage')), names;"
            "names = nas_segm_amd.install_dropin(controller=True);"
            "assert all(n in names for n in ('rl.micro_controllers', 'rl.agent', 'rl.gradient_estimators', "
            "'helpers.storage')), names;"
            "from rl.agent import create_agent, train_agent;"
            "from rl.gradient_estimators import PPO, REINFORCE;"
            "from rl.micro_controllers import MicroController, TemplateController;"
            "from helpers.storage import RolloutStorage;"
            "import nas_segm_amd.rl.agent as a; assert create_agent is a.create_agent; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


def test_header_entries_constness_and_no_bf16_twin():
    from nas_segm_amd import lib
    from nas_segm_amd._lib import HEADER_PATH, pointer_access
    from nas_segm_amd.ffi_gen import prototypes

    protos = {p.name: p for p in prototypes(HEADER_PATH)}
    new = ["nasseg_ctrl_rollout", "nasseg_ctrl_backward", "nasseg_ctrl_ppo_seed", "nasseg_ctrl_saved_floats",
           "nasseg_ctrl_work_floats"]
    for name in new:
        assert name in protos and name in lib.symbols()
        assert name.replace("nasseg_", "nasseg_bf16_") not in protos
    acc = pointer_access()
    written = {n: [protos[n].args[i].name for i, k in acc[n] if k == "w"] for n in new[:3]}
    assert written["nasseg_ctrl_rollout"] == ["sampled", "sampled_lp", "saved", "entropy", "log_prob"]
    assert written["nasseg_ctrl_backward"] == ["work", "grads"]
    assert written["nasseg_ctrl_ppo_seed"] == ["acc", "d_log_prob", "d_entropy"]
    assert lib.query("nasseg_ctrl_saved_floats", 23, 100, 2) == 23 * 2 * 600 + 23 * 192
    assert lib.query("nasseg_ctrl_work_floats", 23, 100, 2) == 23 * 2 * 400 + 23 * 64


def test_bounds_are_refused_with_the_usual_status():
    from nas_segm_amd import NassegError, lib

    def rollout(T=23, H=100, L=2, heads=13, choices=11, B=0, n=0):
        lib.call("nasseg_ctrl_rollout", 1, 1, T, H, L, heads, choices, None, None, 0, B, 20, None, n, None, None, 1, 1,
                 None, None)

    for kw, word in ((dict(H=257), "hidden size"), (dict(L=5), "LSTM layers"), (dict(T=129), "steps"),
                     (dict(choices=65), "choices"), (dict(B=1025), "action rows"), (dict(n=1025), "samples")):
        with pytest.raises(NassegError, match=word):
            rollout(**kw)
    assert word in lib.last_error()


def test_controllers_have_no_cpu_fallback():
    from nas_segm_amd import NassegError

    ctrl = product(*R.CASES["cvpr_h7"])
    with pytest.raises(NassegError):
        ctrl.sample()
    with pytest.raises(NassegError):
        ctrl.evaluate_actions([[0] * ctrl.action_size()])
