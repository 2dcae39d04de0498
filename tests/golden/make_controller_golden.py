"""Generate tests/golden/controller_rollout_<case>.npz + controller_rollout_meta.json from the REFERENCE controller.

Runs only where the reference tree is (like make_golden.py); the reference is imported unmodified, nothing of it is
written into the repository - only inputs and recorded results.

    NASSEG_REFERENCE=<checkout of the reference> python tests/golden/make_controller_golden.py

Per case of tests/_controller_ref.CASES:
  state/<name>       the full state_dict.  The initial values are rounded to multiples of 2^-17 (exact in fp32, still
                     uniform in +-0.1) and stored as int16 counts of that unit.
  actions            6 actions the reference sampled; lp32 / ent32: its fp32 log_prob and entropy per action; lp64 /
                     ent64: the same from the module cast to float64.
  grad{32,64}/<name>  every parameter's gradient (none for enc_op.weight) of sum_b w_b log_prob_b + 0.3 entropy for
                     the fixed weights ``w``, from the fp32 module and from the module cast to float64.  Tensors of
                     more than 4096 elements keep every 8th row, and of the float64 gradient the sum of EVERY row
                     (grad64_rowsum/<name>): the fixture stays below 2 MB in all, one file per case.  The meta file
                     has, per tensor, the largest absolute difference between the reference's fp32 and float64
                     gradients over ALL entries - the yardstick of the GPU tests - for this objective ("mix") and for
                     its two halves alone ("lp" = sum_b w_b log_prob_b, "ent" = entropy).
  ppo/...            one recorded PPO.update (num_steps=6, num_mini_batch=3: minibatches of two rows; clip_param 0.1,
                     entropy_coef 0.01, lr 1e-3) on a full buffer: the buffer, the baseline, the minibatch order, the
                     returned loss and entropy, every parameter afterwards (large ones: every 8th row, and every
                     row's sum in float64, ppo/after_rowsum/<name>).
"""
import copy
import json
import os
import sys

import numpy as np

np.int = int  # src/helpers/storage.py:20 uses the removed alias

REF = os.environ.get("NASSEG_REFERENCE", "")  # a checkout of DrSleep/nas-segm-pytorch
if not os.path.isdir(os.path.join(REF, "src", "rl")):
    raise SystemExit("set NASSEG_REFERENCE to a checkout of the reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(REF, "src"), REF, os.path.dirname(OUT)]

import torch  # noqa: E402
from torch.utils.data.sampler import BatchSampler, SubsetRandomSampler  # noqa: E402

import _controller_ref as R  # noqa: E402

UNIT = 2.0 ** -17
W = [0.7, -1.3, 0.4, 1.1, -0.6, 0.9]
PPO_ARGS = dict(clip_param=0.1, lr=1e-3, baseline_decay=0.95, num_mini_batch=3, num_steps=6, entropy_coef=0.01)


def build(kind, kw):
    from rl.micro_controllers import MicroController, TemplateController

    ctrl = (MicroController if kind == "cvpr" else TemplateController)(**kw)
    with torch.no_grad():
        for p in ctrl.parameters():
            p.copy_(torch.round(p / UNIT) * UNIT)
    return ctrl


def objectives(ctrl, actions, dtype):
    log_probs, entropies = ctrl.evaluate_actions(np.asarray(actions))
    w = torch.tensor(W, dtype=dtype)
    lp = (log_probs * w).sum()
    return {"lp": lp, "ent": entropies[0], "mix": lp + 0.3 * entropies[0]}, log_probs, entropies


def gradients(ctrl, actions, dtype):
    out = {}
    for name in ("lp", "ent", "mix"):
        ctrl.zero_grad()
        objectives(ctrl, actions, dtype)[0][name].backward()
        out[name] = {k: p.grad.detach().clone().numpy() for k, p in ctrl.named_parameters() if p.grad is not None}
    return out


def main():
    from rl.gradient_estimators import PPO

    meta = {"unit": UNIT, "w": W, "ppo_args": PPO_ARGS, "row_stride": R.ROW_STRIDE, "big": R.BIG, "cases": {}}
    for case, (kind, kw) in R.CASES.items():
        torch.manual_seed(2024)
        ctrl = build(kind, kw)
        store = {}
        for k, v in ctrl.state_dict().items():
            counts = np.round(v.numpy().astype(np.float64) / UNIT)
            assert np.abs(counts).max() < 32768 and np.array_equal(counts * UNIT, v.numpy().astype(np.float64))
            store["state/" + k] = counts.astype(np.int16)
        samples = [ctrl.sample() for _ in range(6)]
        actions = [[int(a) for a in ctrl.config2action(cfg)] for cfg, _, _ in samples]
        store["actions"] = np.asarray(actions, dtype=np.int32)
        with torch.no_grad():
            _, lp32, ent32 = objectives(ctrl, actions, torch.float32)
        store["lp32"], store["ent32"] = lp32.numpy(), ent32.numpy()
        g32 = gradients(ctrl, actions, torch.float32)
        torch.set_default_dtype(torch.float64)  # (the reference makes its zero state with the default dtype)
        try:
            ctrl64 = copy.deepcopy(ctrl).double()
            with torch.no_grad():
                _, lp64, ent64 = objectives(ctrl64, actions, torch.float64)
            g64 = gradients(ctrl64, actions, torch.float64)
        finally:
            torch.set_default_dtype(torch.float32)
        store["lp64"], store["ent64"] = lp64.numpy(), ent64.numpy()
        ref_err = {}
        for obj in g32:
            ref_err[obj] = {}
            for k in g32[obj]:
                ref_err[obj][k] = float(np.abs(g32[obj][k].astype(np.float64) - g64[obj][k]).max())
                if obj == "mix":
                    store["grad32/" + k] = R.recorded(k, g32[obj][k])
                    store["grad64/" + k] = R.recorded(k, g64[obj][k])
                    if g64[obj][k].size > R.BIG:
                        store["grad64_rowsum/" + k] = g64[obj][k].sum(axis=1)
        # one recorded PPO update on a full buffer
        agent = PPO(copy.deepcopy(ctrl), action_size=ctrl.action_size(), **PPO_ARGS)
        rewards = [0.31, 0.12, 0.45, 0.27, 0.38, 0.2]
        for k in range(5):
            agent.update((rewards[k], actions[k], samples[k][2]), is_train=False)
        torch.manual_seed(77)
        order = list(BatchSampler(SubsetRandomSampler(range(6)), 2, drop_last=False))
        torch.manual_seed(77)
        loss, entropy = agent.update((rewards[5], actions[5], samples[5][2]))
        store["ppo/actions"] = agent.rollouts.actions.astype(np.int32)
        store["ppo/old_log_probs"] = agent.rollouts.action_log_probs[:, 0]
        store["ppo/rewards"] = agent.rollouts.rewards[:, 0]
        store["ppo/order"] = np.asarray(order, dtype=np.int32)
        for k, v in agent.controller.state_dict().items():
            store["ppo/after/" + k] = R.recorded(k, v.numpy())
            if v.numel() > R.BIG:
                store["ppo/after_rowsum/" + k] = v.numpy().astype(np.float64).sum(axis=1)
        # the recorded order IS the one the update used: the fp32 restatement lands on the same parameters
        sd = {k: v.numpy() for k, v in ctrl.state_dict().items()}
        adv = agent.rollouts.rewards[:, 0] - agent.baseline
        _, _, after = R.ppo_update(sd, kind, kw, actions, agent.rollouts.action_log_probs[:, 0].astype(np.float32),
                                   adv.astype(np.float32), order, PPO_ARGS["clip_param"], PPO_ARGS["entropy_coef"],
                                   PPO_ARGS["lr"], 2.0, torch.float32)
        moved = max(float((agent.controller.state_dict()[k] - ctrl.state_dict()[k]).abs().max()) for k in after)
        apart = max(float((agent.controller.state_dict()[k] - after[k]).abs().max()) for k in after)
        assert apart < 1e-2 * moved, (case, apart, moved)
        meta["cases"][case] = {"kind": kind, "kwargs": kw, "ref_err": ref_err, "ppo_loss": float(loss),
                               "ppo_entropy": float(entropy), "ppo_baseline": float(agent.baseline),
                               "ppo_apart": apart, "ppo_moved": moved}
        path = os.path.join(OUT, "controller_rollout_{}.npz".format(case))
        np.savez_compressed(path, **store)
        print(case, os.path.getsize(path), "bytes; restatement apart", apart, "of", moved)
    json.dump(meta, open(os.path.join(OUT, "controller_rollout_meta.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
