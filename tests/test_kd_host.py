"""Host side of the fused distillation loss and the multi-tensor Polyak update (no GPU needed): which kd_crit the
decoder-only step fuses (engine/trainer.py: native_kd), the nasseg_polyak tables (engine/optim_native.py:
polyak_tables) and the new prototypes of include/nasseg.h."""

import numpy as np
import torch

from nas_segm_amd._lib import HEADER_PATH, parse_header, pointer_access
from nas_segm_amd.ffi_gen import prototypes
from nas_segm_amd.engine import trainer
from nas_segm_amd.engine.optim_native import polyak_eligible, polyak_tables

OUT = (25, 33)


def _kd_y(dtype=torch.float32, shape=(4, 21) + OUT):
    return torch.zeros(shape, dtype=dtype)


def test_native_kd_takes_exactly_a_mean_mse_loss():
    assert trainer.native_kd(torch.nn.MSELoss(), _kd_y(), OUT)
    assert trainer.native_kd(torch.nn.MSELoss(reduction="mean"), _kd_y(), list(OUT))


def test_native_kd_refuses_everything_else():
    class MyMSE(torch.nn.MSELoss):
        pass

    def fn(inp, tgt):
        return torch.nn.functional.mse_loss(inp, tgt)

    for crit in (torch.nn.MSELoss(reduction="sum"), torch.nn.MSELoss(reduction="none"), MyMSE(), fn,
                 torch.nn.L1Loss(), None):
        assert not trainer.native_kd(crit, _kd_y(), OUT), crit
    crit = torch.nn.MSELoss()
    assert not trainer.native_kd(crit, _kd_y(torch.bfloat16), OUT)
    assert not trainer.native_kd(crit, _kd_y(torch.float64), OUT)
    assert not trainer.native_kd(crit, _kd_y(shape=(4, 21, 25, 32)), OUT)
    assert not trainer.native_kd(crit, _kd_y(shape=(4, 21 * 25 * 33)), OUT)
    assert not trainer.native_kd(crit, None, OUT)
    assert not trainer.native_kd(crit, _kd_y().requires_grad_(True), OUT)


def test_native_kd_switch(monkeypatch):
    monkeypatch.setattr(trainer, "NATIVE_KD", False)
    assert not trainer.native_kd(torch.nn.MSELoss(), _kd_y(), OUT)


def test_polyak_tables_from_shapes():
    chunk = 4096
    numels = [1, 3, 5, 4096, 4097, 600000, 8192]
    pairs = [(0x10000 + 256 * i, 0x900000 + 512 * i + (4 if i == 2 else 0), n) for i, n in enumerate(numels)]
    table, chunks = polyak_tables(pairs, chunk)
    assert table.dtype == np.int64 and table.shape == (len(numels), 4)
    assert chunks.dtype == np.int32 and chunks.shape[1] == 2
    assert list(table[:, 0]) == [p for p, _, _ in pairs] and list(table[:, 1]) == [a for _, a, _ in pairs]
    assert list(table[:, 2]) == numels
    assert list(table[:, 3]) == [0 if i == 2 else 1 for i in range(len(numels))]  # (bit 0: both 16-byte aligned)
    want = [(t, off) for t, n in enumerate(numels) for off in range(0, n, chunk)]
    assert [tuple(c) for c in chunks] == want
    assert len(want) == sum((n + chunk - 1) // chunk for n in numels)
    # every element of every tensor is in exactly one chunk
    for t, n in enumerate(numels):
        offs = chunks[chunks[:, 0] == t, 1]
        assert offs[0] == 0 and all(np.diff(offs) == chunk) and n - offs[-1] <= chunk


def test_polyak_tables_empty():
    table, chunks = polyak_tables([], 4096)
    assert table.shape == (0, 4) and chunks.shape == (0, 2)


def test_polyak_needs_fp32_device_pairs():
    ps = [torch.zeros(3), torch.zeros(5)]
    assert not polyak_eligible(ps, [p.clone() for p in ps])  # (CPU tensors: torch's ops)
    assert not polyak_eligible(ps, [ps[0].clone()])
    assert not polyak_eligible([], [])


def test_header_entries_and_constness():
    protos = parse_header()
    acc = pointer_access()
    for name in ("nasseg_ce_mse_fwd", "nasseg_ce_mse_bwd", "nasseg_bf16_ce_mse_fwd", "nasseg_bf16_ce_mse_bwd",
                 "nasseg_ce_mse_workspace", "nasseg_polyak"):
        assert name in protos, name
    for prefix in ("nasseg_", "nasseg_bf16_"):
        # logits, target, teacher read; ce, mse, stats, ws written
        assert acc[prefix + "ce_mse_fwd"] == [(0, "r"), (1, "r"), (3, "r"), (7, "w"), (8, "w"), (9, "w"),
                                             (10, "w")], prefix
        # logits, target, teacher, stats, g_ce, g_mse read; dlogits written
        assert acc[prefix + "ce_mse_bwd"] == [(0, "r"), (1, "r"), (3, "r"), (4, "r"), (5, "r"), (6, "r"),
                                             (10, "w")], prefix
    # the Polyak table is a const int64_t* (a "read" to the recorder: its caller annotates the writes behind it)
    assert acc["nasseg_polyak"] == [(0, "r"), (2, "r")]
    args = {p.name: p.args for p in prototypes(HEADER_PATH)}
    assert [a.ctype for a in args["nasseg_polyak"]][4:6] == ["float", "float"]
    fwd = [(a.ctype, a.name) for a in args["nasseg_bf16_ce_mse_fwd"]]
    assert ("const nasseg_bf16_t*", "logits") in fwd and ("const float*", "teacher") in fwd
