"""Time the native search controller against the same update written in torch ops.

    python tools/kbench_controller.py [--rounds 5] [--cpu-threads 16]

Per controller - CVPR (MicroController(4, 11): T = 23) and the 7-layer WACV (TemplateController(4, 11, 2,
cell_num_layers=7): T = 48), both H = 100, L = 2 - one full PPO.update on a full buffer (100 minibatches of one row):

  native      rl.gradient_estimators.PPO.update: rollout, seed, backward, clip + Adam per minibatch, no host
              synchronisation inside, one read-back;
  torch-gpu   the same update in torch ops (nn.LSTM called step by step, Linear, softmax, clip_grad_norm_, Adam) on
              the device;
  torch-cpu   the same on the host CPU with --cpu-threads threads.

Five rounds, the three variants in turn within a round (so that drift hits all alike), the median per variant; host
clock around work that ends in a device synchronise.  Also the latency of one sample() (torch.rand, one controller
launch, one copy).  Prints one JSON line.  Needs a HIP device: it does not fall back.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nas_segm_amd.engine.optim_native import cached_stepper  # noqa: E402
from nas_segm_amd.rl.gradient_estimators import PPO  # noqa: E402
from nas_segm_amd.rl.micro_controllers import MicroController, TemplateController  # noqa: E402


class TorchController(nn.Module):
    """the controller in torch ops: the product module's parameters (copied), its step table for the order of heads"""

    def __init__(self, ctrl):
        super(TorchController, self).__init__()
        H, L = ctrl.lstm_hidden_size, ctrl.lstm_num_layers
        self.rnn = nn.LSTM(H, H, L)
        self.heads = nn.ModuleList([nn.Linear(H, h.out_features) for h in ctrl._heads])
        self.g_emb = nn.Parameter(ctrl.g_emb.detach().clone().cpu())
        with torch.no_grad():
            for k, v in ctrl.rnn.state_dict().items():
                getattr(self.rnn, k).copy_(v)
            for mine, theirs in zip(self.heads, ctrl._heads):
                mine.weight.copy_(theirs.weight)
                mine.bias.copy_(theirs.bias)
        self.steps, self.H, self.L = ctrl.plan.steps, H, L

    def evaluate_actions(self, actions):
        log_probs = []
        for row in actions:
            inputs = self.g_emb
            hidden = (torch.zeros(self.L, 1, self.H, device=inputs.device),
                      torch.zeros(self.L, 1, self.H, device=inputs.device))
            entropy, log_prob = 0, 0
            for head, n, pos in self.steps:
                output, hidden = self.rnn(inputs, hidden)
                inputs = output
                if head < 0:
                    continue
                logits = self.heads[head](output.squeeze(0))
                p, lp = torch.softmax(logits, dim=-1), torch.log_softmax(logits, dim=-1)
                entropy = entropy - (p * lp).sum()
                log_prob = log_prob + lp[0, int(row[pos])]
            log_probs.append(log_prob.view(1))
        return torch.cat(log_probs), entropy


def torch_update(model, optim, actions, old, adv, batches, clip, device):
    old_t = torch.from_numpy(old).float().to(device)
    adv_t = torch.from_numpy(adv).float().to(device)
    loss_sum = 0.0
    losses = []
    for rows in batches:
        lp, entropy = model.evaluate_actions(actions[rows])
        ratio = torch.exp(lp - old_t[rows])
        surr1 = ratio * adv_t[rows]
        surr2 = torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv_t[rows]
        loss = -torch.min(surr1, surr2).mean()
        optim.zero_grad()
        loss.backward()
        nn.utils.clip_grad_norm_(model.parameters(), 2.0)
        optim.step()
        losses.append(loss.detach())
    loss_sum = float(torch.stack(losses).sum())  # (one read-back, like the native update)
    return loss_sum / len(batches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cpu-threads", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_controller needs a HIP device")
    torch.set_num_threads(args.cpu_threads)
    dev = torch.device("cuda", 0)
    result = {"rounds": args.rounds, "cpu_threads": args.cpu_threads}
    for name, make in (("cvpr", lambda: MicroController(4, 11)),
                       ("wacv7", lambda: TemplateController(4, 11, 2, cell_num_layers=7))):
        torch.manual_seed(0)
        ctrl = make().to(dev)
        agent = PPO(ctrl, clip_param=0.1, lr=1e-4, baseline_decay=0.95, action_size=ctrl.action_size())
        for k, (config, _, log_prob) in enumerate(ctrl.sample_many(99)):  # fill the buffer
            agent.update((0.01 * (k % 37), ctrl.config2action(config), log_prob), is_train=False)
        config, _, log_prob = ctrl.sample()
        sample = (0.2, ctrl.config2action(config), log_prob)
        ro = agent.rollouts
        baselines = {"torch_gpu": TorchController(ctrl).to(dev), "torch_cpu": TorchController(ctrl)}
        optims = {k: torch.optim.Adam(m.parameters(), lr=1e-4) for k, m in baselines.items()}

        def native():
            agent.update(sample)
            torch.cuda.synchronize()

        def with_torch(which):
            batches = [[i] for i in torch.randperm(100).tolist()]
            adv = (ro.rewards - agent.baseline)[:, 0]
            torch_update(baselines[which], optims[which], ro.actions, ro.action_log_probs[:, 0], adv, batches, 0.1,
                         dev if which == "torch_gpu" else torch.device("cpu"))
            torch.cuda.synchronize()

        variants = [("native", native), ("torch_gpu", lambda: with_torch("torch_gpu")),
                    ("torch_cpu", lambda: with_torch("torch_cpu"))]
        native()
        # (the number below is the native path's: both optimiser launches are nasseg_optim_step's)
        assert agent.native_optim and cached_stepper(agent.optimizer) is not None, "nasseg_optim_step declined"
        with_torch("torch_gpu")  # warm-up (the CPU variant needs none worth its seconds)
        times = {k: [] for k, _ in variants}
        for _ in range(args.rounds):
            for k, fn in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[k].append(time.perf_counter() - t0)
        lat = []
        for _ in range(50):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctrl.sample()
            lat.append(time.perf_counter() - t0)
        result[name] = {"T": ctrl.plan.T,
                        "update_ms": {k: round(1e3 * statistics.median(v), 3) for k, v in times.items()},
                        "update_ms_all": {k: [round(1e3 * t, 3) for t in v] for k, v in times.items()},
                        "sample_us": round(1e6 * statistics.median(lat), 1)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
