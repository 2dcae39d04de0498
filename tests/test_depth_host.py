"""Host side of the depth path (no GPU): the scores computed from the 12 sums of F.depth_metrics, the all-reduce of
those sums over data-parallel ranks (gloo, world size 2) with its failure protocol, and the argument checks that
need no device."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def test_depth_scores_follow_the_formulas():
    from nas_segm_amd.engine.inference import depth_reward, depth_scores

    # three pixels written out by hand: (p, g)
    pairs = [(2.0, 1.0), (3.0, 4.0), (1.0, 1.1)]
    acc = np.zeros(12)
    for p, g in pairs:
        ln = math.log(p) - math.log(g)
        ratio = max(p / g, g / p)
        acc += [1, abs(p - g), (p - g) ** 2, abs(p - g) / g, (p - g) ** 2 / g, abs(math.log10(p) - math.log10(g)),
                ln, ln * ln, ratio < 1.25, ratio < 1.25 ** 2, ratio < 1.25 ** 3, 0]
    acc[11] = 123.0  # (reserved: must not matter)
    for given in (acc, torch.from_numpy(acc)):
        s = depth_scores(given)
        ls = [math.log(p) - math.log(g) for p, g in pairs]
        want = {
            "n": 3.0,
            "abs_rel": sum(abs(p - g) / g for p, g in pairs) / 3,
            "sq_rel": sum((p - g) ** 2 / g for p, g in pairs) / 3,
            "rmse": math.sqrt(sum((p - g) ** 2 for p, g in pairs) / 3),
            "rmse_log": math.sqrt(sum(v * v for v in ls) / 3),
            "log10": sum(abs(math.log10(p) - math.log10(g)) for p, g in pairs) / 3,
            "silog": math.sqrt(sum(v * v for v in ls) / 3 - (sum(ls) / 3) ** 2),
            "d1": 1 / 3, "d2": 2 / 3, "d3": 2 / 3,
        }
        assert set(s) == set(want)
        for k in want:
            assert s[k] == pytest.approx(want[k], rel=1e-12, abs=1e-15), k
        assert depth_reward(s) == pytest.approx((1 / 3 * 2 / 3 * 2 / 3) ** (1 / 3), rel=1e-12)


def test_depth_scores_without_a_valid_pixel_are_zero():
    from nas_segm_amd.engine.inference import depth_reward, depth_scores

    s = depth_scores(np.zeros(12))
    assert set(s) == {"n", "abs_rel", "sq_rel", "rmse", "rmse_log", "log10", "silog", "d1", "d2", "d3"}
    assert all(v == 0.0 for v in s.values()), s
    assert depth_reward(s) == 0.0


def test_silog_never_goes_negative_under_rounding():
    from nas_segm_amd.engine.inference import depth_scores

    # every pixel has the same log difference: mean(l^2) - mean(l)^2 is 0 up to rounding, never sqrt(< 0)
    l = 0.1
    acc = np.zeros(12)
    acc[0], acc[6], acc[7] = 7, 7 * l, 7 * l * l
    assert depth_scores(acc)["silog"] >= 0.0 and not math.isnan(depth_scores(acc)["silog"])


def test_berhu_criterion_selects_the_depth_step_and_task0_refuses_it():
    from nas_segm_amd.engine import trainer
    from nas_segm_amd.nn import BerHuLoss

    crit = BerHuLoss(valid_min=0.0)
    assert crit.valid_min == 0.0 and crit.valid_max == float("inf")
    assert trainer._depth_crit(crit) is crit
    assert trainer._depth_crit(type("C", (), {"ignore_index": 255})()) is None
    assert trainer._depth_crit(torch.nn.NLLLoss(ignore_index=255)) is None
    with pytest.raises(ValueError, match="end to end"):
        trainer.train_task0({}, torch.nn.Linear(1, 1), None, 0, crit, None, 2, False, False, 0.0, 3.0, False)


def test_depth_kernels_refuse_host_tensors():
    from nas_segm_amd import functional as F

    with pytest.raises(RuntimeError):
        F.berhu_loss_masked(torch.zeros(1, 1, 2, 2), torch.zeros(1, 2, 2))
    with pytest.raises(RuntimeError):
        F.depth_metrics(torch.zeros(1, 1, 2, 2), torch.zeros(1, 2, 2))


def test_search_rejects_an_unknown_task():
    from nas_segm_amd.engine.search import evaluate_candidate

    with pytest.raises(ValueError):
        evaluate_candidate([], [], [], task="normals", device="cpu")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _sums_worker(rank, world, port, q):
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from nas_segm_amd.engine import PeerFailure, RankParallel

        dp = RankParallel(torch.nn.Linear(2, 2))
        # (a) the sum, in float64: values fp32 could not hold
        acc = torch.arange(12, dtype=torch.float64) * (rank + 1) + (2.0 ** 40 + 0.5) * rank
        ret = dp.reduce_sums(acc)
        want = torch.arange(12, dtype=torch.float64) * sum(range(1, world + 1)) + (2.0 ** 40 + 0.5) * sum(range(world))
        ok_sum = ret is acc and acc.dtype == torch.float64 and torch.equal(acc, want)
        # (b) rank 1 failed: it takes part with the flag and keeps its vector; the healthy rank raises PeerFailure
        acc = torch.full((12,), float(rank + 1), dtype=torch.float64)
        raised = False
        try:
            dp.reduce_sums(acc, failed=(rank == 1))
        except PeerFailure:
            raised = True
        untouched = torch.equal(acc, torch.full((12,), float(rank + 1), dtype=torch.float64))
        # the collectives stayed paired: one more works
        probe = torch.tensor([float(rank + 1)])
        dist.all_reduce(probe)
        q.put((rank, ok_sum, raised, untouched, float(probe)))
    finally:
        dist.destroy_process_group()


def test_reduce_sums_two_processes_gloo():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sums_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, ok_sum, raised, untouched, probe in results:
        assert ok_sum and untouched and probe == 3.0, results
        assert raised == (rank == 0), results


def test_reduce_sums_single_process_is_a_noop():
    from nas_segm_amd.engine import RankParallel

    dp = RankParallel(torch.nn.Linear(2, 2))
    acc = torch.arange(12, dtype=torch.float64)
    assert dp.reduce_sums(acc) is acc and torch.equal(acc, torch.arange(12, dtype=torch.float64))
    assert dp.reduce_sums(acc, failed=True) is acc
