"""Reinforcement-learning agent of the search (src/rl/agent.py): the controller, on the device, with its gradient
estimator."""
from .gradient_estimators import PPO, REINFORCE


def create_agent(enc_num_layers, num_ops, num_agg_ops, lstm_hidden_size, lstm_num_layers, dec_num_cells,
                 cell_num_layers, cell_max_repeat, cell_max_stride, ctrl_lr, ctrl_baseline_decay, ctrl_agent,
                 ctrl_version="cvpr", device="cuda"):
    """The reference's arguments (src/rl/agent.py:6-70) plus ``device``: the controller lives there (there is no CPU
    fallback).  ctrl_version: 'cvpr' (MicroController) or 'wacv' (TemplateController); ctrl_agent: 'ppo' or
    'reinforce'."""
    if ctrl_version == "cvpr":
        from .micro_controllers import MicroController as Controller
    elif ctrl_version == "wacv":
        from .micro_controllers import TemplateController as Controller
    else:
        raise ValueError("ctrl_version must be 'cvpr' or 'wacv' (got {!r})".format(ctrl_version))
    controller = Controller(
        enc_num_layers=enc_num_layers, num_ops=num_ops, num_agg_ops=num_agg_ops, lstm_hidden_size=lstm_hidden_size,
        lstm_num_layers=lstm_num_layers, dec_num_cells=dec_num_cells, cell_num_layers=cell_num_layers,
        cell_max_repeat=cell_max_repeat, cell_max_stride=cell_max_stride).to(device)
    if ctrl_agent == "ppo":
        return PPO(controller, clip_param=0.1, lr=ctrl_lr, baseline_decay=ctrl_baseline_decay,
                   action_size=controller.action_size())
    if ctrl_agent == "reinforce":
        return REINFORCE(controller, lr=ctrl_lr, baseline_decay=ctrl_baseline_decay)
    raise ValueError("ctrl_agent must be 'ppo' or 'reinforce' (got {!r})".format(ctrl_agent))


def train_agent(agent, sample):
    """Training controller: sample = (config, reward, entropy, log_prob) -> (loss, entropy) of the update"""
    config, reward, entropy, log_prob = sample
    action = agent.controller.config2action(config)
    return agent.update((reward, action, log_prob))
