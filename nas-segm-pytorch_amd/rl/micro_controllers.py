"""The search controllers of src/rl/micro_controllers.py on the device.

``MicroController`` (CVPR) and ``TemplateController`` (WACV) keep the reference's constructor arguments, parameter
names and shapes - their ``state_dict`` loads into the reference's classes and back, the unused ``enc_op`` included -
and its methods.  What differs is how they run: in both controllers the LSTM's next input is its own previous output,
so no step's distribution depends on a sampled action, and the whole T-step rollout is ONE kernel launch
(functional.controller_rollout / controller_sample, csrc/controller.hip) instead of T calls of nn.LSTM, a Linear and
two softmaxes each.  ``sample()`` is ``torch.rand`` for the uniforms, that launch and one device-to-host copy;
``sample_many(n)`` samples n candidates from the same rollout; ``evaluate`` / ``evaluate_actions`` are one launch
whatever the number of action rows, and one autograd node.

The modules must live on a HIP device: there is no CPU fallback.
"""
import torch
import torch.nn as nn

from .. import functional as F


class _LSTMParams(nn.Module):
    """The parameters of nn.LSTM(hidden, hidden, layers) under nn.LSTM's names, shapes and order (gates i, f, g, o);
    the kernels read them in place."""

    def __init__(self, hidden, layers):
        super(_LSTMParams, self).__init__()
        for k in range(layers):
            for name, shape in (("weight_ih", (4 * hidden, hidden)), ("weight_hh", (4 * hidden, hidden)),
                                ("bias_ih", (4 * hidden,)), ("bias_hh", (4 * hidden,))):
                self.register_parameter("{}_l{}".format(name, k), nn.Parameter(torch.zeros(*shape)))


class _Controller(nn.Module):
    """What the two controllers share: the plan (step table, step <-> action-position map: built once per module),
    the launches, the reference's method names."""

    def _finish(self, steps, heads):
        """steps: [(head module or None, position in an action row or -1)] in rollout order"""
        index = {id(h): j for j, h in enumerate(heads)}
        table = [(-1, 0, -1) if h is None else (index[id(h)], h.out_features, pos) for h, pos in steps]
        # (plain attributes, not buffers: the state_dict stays the reference's)
        self._heads = list(heads)
        self.plan = F.ControllerPlan(table, self.lstm_hidden_size, self.lstm_num_layers,
                                     [h.out_features for h in heads], self._action_len)
        self.reset_parameters()

    def action_size(self):
        return self._action_len

    def reset_parameters(self):
        init_range = 0.1
        for param in self.parameters():
            param.data.uniform_(-init_range, init_range)

    def table_parameters(self):
        """the parameters the kernels read, in the plan's table order (enc_op is not among them)"""
        params = [self.g_emb]
        for k in range(self.lstm_num_layers):
            params += [getattr(self.rnn, "{}_l{}".format(n, k)) for n in ("weight_ih", "weight_hh", "bias_ih",
                                                                          "bias_hh")]
        for h in self._heads:
            params += [h.weight, h.bias]
        return params

    def _actions(self, actions):
        """action rows (a list, a numpy array, a tensor) as the int32 device tensor (rows, action_size)"""
        device = self.g_emb.device
        if not torch.is_tensor(actions):
            actions = torch.as_tensor(actions)
        actions = actions.reshape(-1, self._action_len)
        return actions.to(device=device, dtype=torch.int32).contiguous()

    def sample_many(self, n, generator=None):
        """n candidates from ONE rollout -> [(config, entropy, log_prob)]; entropy and log_prob are 0-dim device
        tensors without a graph, as the search loop hands them on"""
        g_emb = self.g_emb
        F.require_device(g_emb)
        u = torch.rand((int(n), self.plan.T), device=g_emb.device, dtype=torch.float32, generator=generator)
        return self.sample_given(u)

    def sample_given(self, u):
        """``sample_many`` for given uniforms u (n, T): step t of candidate s takes the first index whose cumulative
        probability exceeds u[s, t]"""
        actions, log_probs, entropy = F.controller_sample(self.plan, self.table_parameters(), u)
        rows = actions.cpu().tolist()  # (the one device-to-host copy)
        return [(self.action2config(row, dec_block=self.dec_num_cells, ctx_block=self.cell_num_layers,
                                    as_sampled=True), entropy, log_probs[s]) for s, row in enumerate(rows)]

    def sample(self):
        return self.sample_many(1)[0]

    def forward(self, config=None):
        if config is None:
            return self.sample()
        action = self.config2action(config)
        entropy, log_probs = F.controller_rollout(self.plan, self.table_parameters(), self._actions(action))
        return config, entropy, log_probs[0]

    def evaluate(self, action):
        """entropy and log-probability of one action row -> (config, entropy, log_prob)"""
        if torch.is_tensor(action):
            action = action.tolist()
        action = [int(a) for a in action]
        config = self.action2config(action, dec_block=self.dec_num_cells, ctx_block=self.cell_num_layers)
        entropy, log_probs = F.controller_rollout(self.plan, self.table_parameters(), self._actions(action))
        return config, entropy, log_probs[0]

    def evaluate_actions(self, actions_batch, rows=None):
        """-> (log_probs (B,), entropies (B,)) of the B action rows, one launch, one autograd node (the steps'
        distributions do not depend on the actions: every row has the same entropy)"""
        actions = self._actions(actions_batch)
        entropy, log_probs = F.controller_rollout(self.plan, self.table_parameters(), actions, rows)
        return log_probs, entropy.expand(log_probs.shape[0])


class MicroController(_Controller):
    """Stack LSTM controller based on ENAS, sampling the decoder's cell and connections
    (src/rl/micro_controllers.py:10-330)."""

    def __init__(self, enc_num_layers, num_ops, lstm_hidden_size=100, lstm_num_layers=2, dec_num_cells=3,
                 cell_num_layers=4, **kwargs):
        super(MicroController, self).__init__()
        self.cell_num_layers = cell_num_layers
        self.dec_num_cells = dec_num_cells
        self.enc_num_layers = enc_num_layers
        self.lstm_hidden_size = lstm_hidden_size
        self.lstm_num_layers = lstm_num_layers
        # 2 connections per decoder block, 2 connections + 2 ops per cell layer but the first, (dummy, op) for that one
        self._action_len = 2 * dec_num_cells + 2 * (cell_num_layers - 1) + 2 + 2 * (cell_num_layers - 1)

        self.rnn = _LSTMParams(lstm_hidden_size, lstm_num_layers)
        self.enc_op = nn.Embedding(num_ops, lstm_hidden_size)
        self.linear_op = nn.Linear(lstm_hidden_size, num_ops)
        self.g_emb = nn.Parameter(torch.zeros(1, 1, lstm_hidden_size))
        self.conn_fcs = nn.ModuleList([nn.Linear(lstm_hidden_size, enc_num_layers + i)
                                       for i in range(dec_num_cells) for _ in range(2)])
        self.ctx_fcs = nn.ModuleList([nn.Linear(lstm_hidden_size, 1 + 3 * i)
                                      for i in range(cell_num_layers - 1) for _ in range(2)])

        # the rollout does the connections first and the cell last; an action row lists the cell first (its first
        # position a dummy 0 without a step) and the connections last
        steps = [(None, -1)] * enc_num_layers
        conn_base = 4 * (cell_num_layers - 1) + 2
        for layer in range(dec_num_cells):
            for i in range(2):
                steps.append((self.conn_fcs[2 * layer + i], conn_base + 2 * layer + i))
        steps.append((self.linear_op, 1))
        for layer in range(1, cell_num_layers):
            base = (layer - 1) * 4 + 2
            steps += [(self.ctx_fcs[2 * layer - 2 + i], base + i) for i in range(2)]
            steps += [(self.linear_op, base + 2 + i) for i in range(2)]
        self._finish(steps, [self.linear_op] + list(self.conn_fcs) + list(self.ctx_fcs))

    @staticmethod
    def get_mock():
        arc_seq = [[[0], [1, 2, 3, 4], [1, 2, 3, 4], [1, 2, 3, 4]], [[0, 1], [2, 3], [4, 5]]]
        return arc_seq, 6, -1.4

    @staticmethod
    def config2action(config):
        ctx, conns = config
        action = []
        for idx, cell in enumerate(ctx):
            if idx == 0:
                # a sampled config holds the op alone, one from action2config [0, op]
                op = cell[-1] if isinstance(cell, (list, tuple)) else cell
                action += [0, op]
            else:
                action += list(cell[:4])
        for conn in conns:
            action += [conn[0], conn[1]]
        return action

    @staticmethod
    def action2config(action, enc_end=0, dec_block=3, ctx_block=4, as_sampled=False):
        """as_sampled: the first cell layer as ``sample`` returns it (the op alone) instead of [0, op]"""
        ctx = []
        for i in range(ctx_block):
            if i == 0:
                ctx.append(action[1] if as_sampled else [action[0], action[1]])
            else:
                ctx.append([action[(i - 1) * 4 + 2 + j] for j in range(4)])
        conns = [[action[4 * (ctx_block - 1) + 2 + 2 * i], action[4 * (ctx_block - 1) + 3 + 2 * i]]
                 for i in range(dec_block)]
        return [ctx, conns]


class TemplateController(_Controller):
    """Stacked LSTM-based controller for TemplateDecoder: the templates first, then the structure with repeats and
    strides (src/rl/micro_controllers.py:333-621)."""

    def __init__(self, enc_num_layers, num_ops, num_agg_ops, lstm_hidden_size=100, lstm_num_layers=2,
                 dec_num_cells=3, cell_num_layers=3, cell_max_repeat=4, cell_max_stride=2, **kwargs):
        super(TemplateController, self).__init__()
        self.enc_num_layers = enc_num_layers
        self.lstm_num_layers = lstm_num_layers
        self.lstm_hidden_size = lstm_hidden_size
        self.dec_num_cells = dec_num_cells
        self.cell_num_layers = cell_num_layers

        self.rnn = _LSTMParams(lstm_hidden_size, lstm_num_layers)
        self.enc_op = nn.Embedding(num_ops, lstm_hidden_size)
        self.linear_op = nn.Linear(lstm_hidden_size, num_ops)
        self.linear_agg_op = nn.Linear(lstm_hidden_size, num_agg_ops)
        self.template_op = nn.Linear(lstm_hidden_size, dec_num_cells)
        self.repeat_op = nn.Linear(lstm_hidden_size, cell_max_repeat)
        self.stride_op = nn.Linear(lstm_hidden_size, cell_max_stride)
        self.dummy_stride_op = nn.Linear(lstm_hidden_size, 1)  # always predicting a single stride
        self.g_emb = nn.Parameter(torch.zeros(1, 1, lstm_hidden_size))
        self._action_len = 3 * dec_num_cells + 5 * cell_num_layers
        self.ctx_fcs = nn.ModuleList([nn.Linear(lstm_hidden_size, enc_num_layers + i)
                                      for i in range(cell_num_layers) for _ in range(2)])

        steps = [(None, -1)] * enc_num_layers
        for layer in range(dec_num_cells):
            steps += [(self.linear_op, 3 * layer), (self.linear_op, 3 * layer + 1),
                      (self.linear_agg_op, 3 * layer + 2)]
        for layer in range(cell_num_layers):
            base = 3 * dec_num_cells + 5 * layer
            stride = self.dummy_stride_op if layer >= cell_num_layers // 2 else self.stride_op
            steps += [(self.ctx_fcs[2 * layer], base), (self.ctx_fcs[2 * layer + 1], base + 1),
                      (self.template_op, base + 2), (self.repeat_op, base + 3), (stride, base + 4)]
        self._finish(steps, [self.linear_op, self.linear_agg_op, self.template_op, self.repeat_op, self.stride_op,
                             self.dummy_stride_op] + list(self.ctx_fcs))

    @staticmethod
    def get_mock():
        return None, [[[0, 0, 0]], [[0, 0, 0, 0, 0]]], 6, -1.4

    @staticmethod
    def config2action(config):
        decoder, structure = config
        action = []
        for cell in decoder:
            action += list(cell)
        for block in structure:
            action += list(block)
        return action

    @staticmethod
    def action2config(action, enc_end=0, dec_block=3, ctx_block=3, num_ops_per_template=3, num_actions_per_layer=5,
                      as_sampled=False):
        action = list(action)
        decoder = [action[i * num_ops_per_template:(i + 1) * num_ops_per_template] for i in range(dec_block)]
        action = action[dec_block * num_ops_per_template:]
        structure = [action[j * num_actions_per_layer:(j + 1) * num_actions_per_layer] for j in range(ctx_block)]
        return [decoder, structure]
