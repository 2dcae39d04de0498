"""REINFORCE and PPO for controller training (src/rl/gradient_estimators.py) on the device.

The same defaults, ``state_dict`` keys and host-side randomness (the minibatch order comes from the reference's
``BatchSampler(SubsetRandomSampler)`` under torch's default generator).  What differs is where a PPO update runs: the
rollout buffer and the minibatch order are uploaded once per ``update``; every minibatch is then four library calls -
rollout, PPO seed, backward, clip + Adam (engine/optim_native.native_clip_and_step) - without a host
synchronisation, and the loss and entropy sums are read back once at the end.
"""
import warnings

import numpy as np
import torch

from .. import functional as F
from ..engine.optim_native import native_clip_and_step
from ..helpers.storage import RolloutStorage


def _table_grads(controller, flat):
    """p.grad of every parameter the kernels read := its slice of ``flat``; anything else (enc_op.weight) gets no
    gradient, as in the reference, so Adam and the clip norm skip it"""
    table = controller.table_parameters()
    ids = set(id(p) for p in table)
    for p, g in zip(table, controller.plan.split(flat)):
        p.grad = g.view_as(p)
    for p in controller.parameters():
        if id(p) not in ids:
            p.grad = None


def _clip_and_step(owner, groups):
    """clip + Adam in the two launches of nasseg_optim_step (engine/optim_native.py).  Where that declines - another
    optimiser configuration, state it cannot take over (a device-side ``step`` after a foreign load_state_dict),
    NASSEG_NATIVE_OPTIM=0 - torch's own clip_grad_norm_ and step run instead, on the device but with more launches
    and a host synchronisation per clip: ``owner.native_optim`` says which one ran, and the first such step warns."""
    native = native_clip_and_step(groups)
    if not native:
        if getattr(owner, "native_optim", None) is not False:
            warnings.warn("controller update: nasseg_optim_step declined, torch's clip_grad_norm_ / Adam.step run")
        for params, max_norm, optim in groups:
            torch.nn.utils.clip_grad_norm_(params, max_norm)
            optim.step()
    owner.native_optim = native


class REINFORCE(object):
    """REINFORCE gradient estimator with a moving-average baseline."""

    def __init__(self, controller, lr, baseline_decay, max_grad_norm=2.0):
        self.baseline = None
        self.decay = baseline_decay
        self.controller = controller
        self.optimizer = torch.optim.Adam(controller.parameters(), lr=lr)
        self.max_grad_norm = max_grad_norm

    def update(self, sample):
        """One gradient step for the controller and the baseline's update.  sample = (reward, action, log_prob) as
        ``train_agent`` passes it (the reference's ``update`` unpacks four values from it and three from
        ``evaluate``, and raises); -> (loss, entropy)"""
        reward, action = sample[0], sample[1]
        _, entropy, log_prob = self.controller.evaluate(action)
        if self.baseline is None:
            self.baseline = reward
        else:
            self.baseline = self.decay * self.baseline + (1 - self.decay) * reward
        adv = reward - self.baseline
        loss = -log_prob * adv
        for p in self.controller.parameters():
            p.grad = None
        loss.backward()
        _clip_and_step(self, [(list(self.controller.parameters()), self.max_grad_norm, self.optimizer)])
        return loss.detach(), entropy.detach()

    def state_dict(self):
        return {"baseline": self.baseline, "controller": self.controller.state_dict(),
                "optimizer": self.optimizer.state_dict()}

    def load_state_dict(self, states):
        self.controller.load_state_dict(states["controller"])
        self.baseline = states["baseline"]
        self.optimizer.load_state_dict(states["optimizer"])


class PPO(object):
    """Proximal Policy Optimization with a rollout buffer."""

    def __init__(self, controller, clip_param, lr, baseline_decay, action_size=18, ppo_epoch=1, num_mini_batch=100,
                 max_grad_norm=2.0, entropy_coef=0, num_steps=100, num_processes=1):
        self.ppo_epoch = ppo_epoch
        self.controller = controller
        self.optimizer = torch.optim.Adam(controller.parameters(), lr=lr)
        self.num_mini_batch = num_mini_batch
        self.clip_param = clip_param
        self.max_grad_norm = max_grad_norm
        self.entropy_coef = entropy_coef
        self.rollouts = RolloutStorage(num_steps, num_processes, action_size)
        self.baseline = None
        self.decay = baseline_decay
        self._flat = None

    def state_dict(self):
        return {"baseline": self.baseline, "rollouts": self.rollouts, "controller": self.controller.state_dict(),
                "optimizer": self.optimizer.state_dict()}

    def load_state_dict(self, states):
        """(a checkpoint without "rollouts" - the reference's old format, which it refills from genotypes.out
        through an ``evaluate`` call that raises - is refused)"""
        if "rollouts" not in states:
            raise ValueError("PPO.load_state_dict: the checkpoint has no rollout buffer")
        self.controller.load_state_dict(states["controller"])
        self.optimizer.load_state_dict(states["optimizer"])
        self.baseline = states["baseline"]
        self.rollouts = states["rollouts"]

    def update(self, sample, is_train=True, batches=None):
        """sample = (reward, action, log_prob): insert it, then ``ppo_epoch`` passes over the buffer in minibatches.
        ``batches``: the minibatches' row indices (one list per minibatch, all epochs in a row) instead of a fresh
        draw.  -> (mean action loss, mean entropy) over ppo_epoch * num_mini_batch updates."""
        reward, action, log_prob = sample
        if self.baseline is None:
            self.baseline = reward
        else:
            self.baseline = self.decay * self.baseline + (1 - self.decay) * reward
        self.rollouts.insert(action, log_prob, reward)
        if not is_train:
            return -1, -1
        controller = self.controller
        plan, params = controller.plan, controller.table_parameters()
        F.require_device(*params)
        device = params[0].device
        advantages = self.rollouts.rewards - self.baseline
        if batches is None:
            batches = [b for _ in range(self.ppo_epoch) for b in self.rollouts.batches(self.num_mini_batch)]
        # uploaded once per update: the buffer (actions, old log-probabilities, advantages) and the minibatch order
        actions = torch.from_numpy(self.rollouts.actions.astype(np.int32)).to(device)
        old = torch.from_numpy(self.rollouts.action_log_probs[:, 0].astype(np.float32)).to(device)
        adv = torch.from_numpy(advantages[:, 0].astype(np.float32)).to(device)
        order = torch.tensor([i for b in batches for i in b], dtype=torch.int32).to(device)
        widest = max(len(b) for b in batches)
        acc = torch.zeros(2, device=device, dtype=torch.float32)
        d_lp = torch.empty(widest, device=device, dtype=torch.float32)
        d_ent = torch.empty((), device=device, dtype=torch.float32)
        if self._flat is None or self._flat.device != device or self._flat.numel() != plan.total:
            self._flat = torch.zeros(plan.total, device=device, dtype=torch.float32)
        work = torch.empty(F.lib.query("nasseg_ctrl_work_floats", plan.T, plan.H, plan.L), device=device,
                           dtype=torch.float32)
        _table_grads(controller, self._flat)
        groups = [(list(controller.parameters()), self.max_grad_norm, self.optimizer)]
        first = 0
        with torch.no_grad():
            for b in batches:
                rows = order[first:first + len(b)]
                first += len(b)
                entropy, lp, saved, _, _ = F.controller_forward(plan, params, actions, rows)
                F.controller_ppo_seed(lp, entropy, old, adv, rows, self.clip_param, self.entropy_coef, acc,
                                      d_lp[:len(b)], d_ent)
                F.controller_backward(plan, params, saved, actions, rows, d_lp[:len(b)], d_ent, self._flat, work)
                _clip_and_step(self, groups)
        for p in controller.parameters():
            p.grad = None  # (slices of a buffer the next update overwrites: nothing stale for a later backward())
        loss_epoch, entropy_epoch = acc.tolist()  # (the update's one read-back)
        num_updates = self.ppo_epoch * self.num_mini_batch
        return loss_epoch / num_updates, entropy_epoch / num_updates
