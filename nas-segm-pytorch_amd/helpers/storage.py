"""Rollout storage for PPO (src/helpers/storage.py): the same fields and attribute names, so that a pickled buffer of
either implementation loads in the other."""
import numpy as np
from torch.utils.data.sampler import BatchSampler, SubsetRandomSampler


class RolloutStorage(object):
    """Rollout storage for NAS: policy gradient without value predictions."""

    def __init__(self, num_steps, num_processes, action_size):
        """
        Args:
          num_steps: rollout length
          num_processes: samples per step
          action_size: flattened segmenter configuration
        """
        self.action_log_probs = np.zeros((num_steps * num_processes, 1))
        self.actions = np.zeros((num_steps * num_processes, action_size), dtype=int)
        self.rewards = np.zeros((num_steps * num_processes, 1))
        self.num_steps = num_steps
        self.num_processes = num_processes
        self.step = 0

    def insert(self, action, log_prob, reward):
        inds = range(self.step * self.num_processes, (self.step + 1) * self.num_processes)
        self.actions[inds] = action
        self.action_log_probs[inds] = log_prob.item() if hasattr(log_prob, "item") else float(log_prob)
        self.rewards[inds] = reward
        self.step = (self.step + 1) % self.num_steps

    def batches(self, num_mini_batch):
        """the minibatches' row indices, drawn as the reference draws them: BatchSampler over a SubsetRandomSampler of
        the whole buffer (torch's default generator)"""
        batch_size = self.rewards.shape[0]
        mini_batch_size = batch_size // num_mini_batch
        return list(BatchSampler(SubsetRandomSampler(range(batch_size)), mini_batch_size, drop_last=False))

    def generator(self, advantages, num_mini_batch):
        """Yields (actions_batch, rewards_batch, old_actions_log_probs_batch, adv_targ) per minibatch."""
        for indices in self.batches(num_mini_batch):
            yield (self.actions[indices], self.rewards[indices], self.action_log_probs[indices], advantages[indices])
