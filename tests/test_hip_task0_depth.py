"""The decoder-only (task0) depth stage on the GPU: the row-indexed berHu kernels (``rows=``: the target is read in
place from a cache through the batch's row index), the depth cache of ``populate_task0(task="depth")``, the depth
branch of ``train_task0`` - launched from the host and replayed - and ``evaluate_candidate(task0_epochs=)``.

Yardstick of the kernels: the un-indexed entry point on the gathered copy ``cache[rows].contiguous()`` (the index
applied by torch on the device), compared with ``torch.equal`` - no tolerance.  The un-indexed entry points are pinned
against float64 and torch autograd by test_hip_depth.py / test_hip_upsampled_berhu.py; the indexed ones claim their
bits."""
import math

import numpy as np
import pytest
import torch

from _util import build_product_net, load_json

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VMAX = 8.0  # valid: finite and 0 < t <= 8

# (B, h, w, H, W, N, rows, a cache row made all holes or None)
SHAPES = [
    (3, 7, 9, 29, 37, 7, [5, 0, 5], 0),            # repeats, unordered, ratios not integral; row 0: all holes
    (1, 1, 1, 5, 3, 2, [1], None),                 # smallest
    (4, 33, 41, 130, 161, 6, [5, 2, 0, 3], 2),     # 5 412 prediction pixels: several / many workgroups
    (2, 2, 3, 61, 80, 4, [3, 3], None),            # an x32 head: the automatic group is 256
]
IDS = ["3x7x9", "1x1x1", "4x33x41", "x32"]


def Fn():
    from nas_segm_amd import functional

    return functional


def holes_like(shape, g):
    """every kind of hole, in equal shares: 0, NaN, +inf, negative, above VMAX"""
    kind = torch.randint(0, 5, shape, generator=g)
    out = torch.zeros(shape)
    out[kind == 1] = float("nan")
    out[kind == 2] = float("inf")
    out[kind == 3] = -1.5
    out[kind == 4] = VMAX + 1.5
    return out


def make_cache(N, H, W, seed, all_holes=()):
    """valid depths in [0.1, 7.9) with about 30 % holes of every kind; every row holds other data; the rows
    ``all_holes`` hold holes only"""
    g = torch.Generator().manual_seed(seed)
    cache = 0.1 + 7.8 * torch.rand(N, H, W, generator=g)
    hole = torch.rand(N, H, W, generator=g) < 0.3
    hole[:, 0, 0] = False  # (the one target pixel the smallest prediction samples stays valid)
    cache[hole] = holes_like((N, H, W), g)[hole]
    for r in all_holes:
        cache[r] = holes_like((H, W), g)
    return cache


def make_pred(B, h, w, dtype, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (0.3 + 7.7 * torch.rand(B, 1, h, w, generator=g)).to(dtype).to(DEV)


def bits(t):
    """the tensor as integers: NaN == NaN, -0 != 0"""
    return t.view(torch.int32 if t.element_size() == 4 else (torch.int16 if t.element_size() == 2 else torch.int64))


def run(family, pred, target, rows=None, group=0, scale=2.5):
    """-> (loss, c, n_valid, dpred) of one forward + backward, ``scale`` applied upstream"""
    F = Fn()
    p = pred.clone().requires_grad_(True)
    parts = F._depth_criterion(p, target, 0.0, VMAX, family, group, rows=rows)
    loss, c, n = parts.loss, parts.c, parts.n_valid
    (scale * loss).backward()
    return loss.detach().clone(), c.detach().clone(), n.detach().clone(), p.grad


def assert_same(got, want, what):
    for name, a, b in zip(("loss", "c", "n_valid", "dpred"), got, want):
        assert a.dtype == b.dtype and torch.equal(a, b), (what, name, a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("family", ["masked", "up"])
@pytest.mark.parametrize("case", SHAPES, ids=IDS)
def test_indexed_kernels_give_the_bits_of_the_gathered_copy(case, family, dtype):
    B, h, w, H, W, N, rows, hole_row = case
    cache = make_cache(N, H, W, seed=11, all_holes=() if hole_row is None else (hole_row,)).to(DEV)
    rows_d = torch.tensor(rows, dtype=torch.int64, device=DEV)
    cache0, rows0 = cache.clone(), rows_d.clone()
    gathered = cache[rows_d].contiguous()
    assert not torch.equal(bits(gathered), bits(cache[:B]))  # (non-identity rows: ignoring them shows)
    pred = make_pred(B, h, w, dtype)
    want = run(family, pred, gathered)
    got = run(family, pred, cache, rows_d)
    print(case[:6], family, dtype, "loss", float(got[0]), "c", float(got[1]), "n_valid", float(got[2]))
    assert_same(got, want, "auto")
    assert float(want[2]) > 0 and float(want[0]) > 0 and math.isfinite(float(want[0]))
    assert got[3].dtype == dtype and float(got[3].float().abs().max()) > 0
    if hole_row is not None:  # (an all-hole row indexed together with valid ones: its image gets exact zeros)
        b = rows.index(hole_row)
        assert float(got[3][b].float().abs().max()) == 0.0
    # neither the cache nor the index is written, forward or backward
    assert torch.equal(bits(cache), bits(cache0)) and torch.equal(rows_d, rows0)
    # the public functions and the criterion module: the same bits
    F = Fn()
    from nas_segm_amd.nn import BerHuLoss

    fn = F.berhu_loss_upsampled if family == "up" else F.berhu_loss_masked
    assert torch.equal(fn(pred, cache, 0.0, VMAX, rows=rows_d), want[0])
    assert torch.equal(BerHuLoss(0.0, VMAX, full_size=family == "up")(pred, cache, rows=rows_d), want[0])
    if family == "up":
        parts = F.berhu_loss_upsampled(pred, cache, 0.0, VMAX, return_parts=True, rows=rows_d)
        assert all(torch.equal(a, b) for a, b in zip(parts, want[:3]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_indexed_upsampling_backward_every_group_and_the_upstream_scale(dtype):
    B, h, w, H, W, N, rows, hole_row = SHAPES[0]
    cache = make_cache(N, H, W, seed=12, all_holes=(hole_row,)).to(DEV)
    rows_d = torch.tensor(rows, dtype=torch.int64, device=DEV)
    gathered = cache[rows_d].contiguous()
    pred = make_pred(B, h, w, dtype)
    for group in (1, 4, 16, 64, 256):
        assert_same(run("up", pred, cache, rows_d, group), run("up", pred, gathered, None, group), group)
    # the x32 head: the automatic choice is the 256-lane group
    B, h, w, H, W, N, rows, _ = SHAPES[3]
    cache32 = make_cache(N, H, W, seed=13).to(DEV)
    rows32 = torch.tensor(rows, dtype=torch.int64, device=DEV)
    pred32 = make_pred(B, h, w, dtype)
    assert_same(run("up", pred32, cache32, rows32, 0), run("up", pred32, cache32, rows32, 256), "x32")
    # an upstream scale reaches dpred
    for family in ("masked", "up"):
        one = run(family, pred, cache, rows_d, scale=1.0)
        scaled = run(family, pred, cache, rows_d, scale=2.5)
        assert torch.equal(one[0], scaled[0]) and float(one[3].float().abs().max()) > 0
        # (fp32: a few roundings of 2^-24; bf16: each stored value is within 2^-8 of its exact one)
        tol = 1e-6 if dtype == torch.float32 else 2.0 ** -6
        assert torch.allclose(scaled[3].float(), 2.5 * one[3].float(), rtol=tol, atol=0.0)
        assert not torch.equal(scaled[3], one[3])


@pytest.mark.parametrize("family", ["masked", "up"])
def test_indexed_rows_that_are_all_holes(family):
    B, h, w, H, W, N, _, _ = SHAPES[0]
    cache = make_cache(N, H, W, seed=14, all_holes=(0, 5)).to(DEV)
    rows_d = torch.tensor([5, 0, 5], dtype=torch.int64, device=DEV)
    for dtype in (torch.float32, torch.bfloat16):
        pred = make_pred(B, h, w, dtype)
        loss, c, n, grad = run(family, pred, cache, rows_d)
        assert float(loss) == 0.0 and float(n) == 0.0 and float(grad.float().abs().max()) == 0.0
        assert not bool(torch.isnan(grad.float()).any())
        assert_same((loss, c, n, grad), run(family, pred, cache[rows_d].contiguous()), "holes")
    # (the rows not indexed are valid: a kernel that read rows 0..2 instead would see them)
    assert float(run(family, pred, cache[:3].contiguous())[2]) > 0


def test_device_refusals_of_rows():
    F = Fn()
    cache = make_cache(4, 8, 8, seed=15).to(DEV)
    pred = make_pred(2, 2, 2, torch.float32)
    rows_d = torch.tensor([3, 1], dtype=torch.int64, device=DEV)
    for fn in (F.berhu_loss_masked, F.berhu_loss_upsampled):
        with pytest.raises(RuntimeError, match="contiguous"):  # (the cache is read in place: never copied)
            fn(pred, cache.transpose(1, 2), rows=rows_d)
        with pytest.raises(RuntimeError, match="rows"):
            fn(pred, cache, rows=rows_d.to(torch.int32))
        with pytest.raises(RuntimeError, match="one cache row per image"):
            fn(pred, cache, rows=rows_d[:1])
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(pred, cache, rows=rows_d.cpu())
        with pytest.raises(IndexError):
            fn(pred, cache, rows=torch.tensor([4, 0]))


def test_cache_rows_beyond_two_to_the_31_elements():
    """rows[b] * H * W is 64-bit: row 2048 of a (2049, 1024, 1024) cache starts at element 2^31"""
    N, H, W = 2049, 1024, 1024
    need = N * H * W * 4
    free = torch.cuda.mem_get_info(torch.device(DEV))[0]
    if free < 3 * need:
        pytest.skip("torch.cuda.mem_get_info shows {:.1f} GB free: less than three times the cache's {:.1f} GB".format(
            free / 1e9, need / 1e9))
    cache = torch.empty((N, H, W), device=DEV, dtype=torch.float32)  # (only rows 0 and 2048 are written)
    two = make_cache(2, H, W, seed=16).to(DEV)
    cache[0].copy_(two[0])
    cache[2048].copy_(two[1])
    rows_d = torch.tensor([2048, 0], dtype=torch.int64, device=DEV)
    gathered = torch.stack([two[1], two[0]]).contiguous()
    pred = make_pred(2, 32, 32, torch.float32)
    for family in ("masked", "up"):
        want = run(family, pred, gathered)
        got = run(family, pred, cache, rows_d)
        print(family, "loss", float(got[0]), "n_valid", float(got[2]))
        assert float(want[2]) > 0
        assert_same(got, want, family)
    del cache


# ---------------------------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------------------------
REC = load_json("nets_meta.json")["cvpr_arch2_depth"]


def depth_samples(n, seed, batch=1):
    """n samples of {"image", "mask"}: masks in [0.1, 7.9) with about 30 % holes of every kind"""
    g = torch.Generator().manual_seed(seed)
    _, _, H, W = REC["shape"]
    return [{"image": torch.randn(batch, 3, H, W, generator=g), "mask": make_cache(batch, H, W, seed * 100 + i)}
            for i in range(n)]


def fresh_net():
    assert REC["classes"] == 1 and REC["n_aux"] == 3
    return build_product_net(REC["kind"], REC["genotype"], REC["classes"], REC["dec_kwargs"], REC["seed"]).to(DEV)


def adam(net):
    return torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)


def cpu_sd(module):
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


SAMPLES = depth_samples(6, seed=31)


def populate(net, samples=SAMPLES):
    from nas_segm_amd.engine.trainer import populate_task0

    return populate_task0.__wrapped__(net, samples, None, len(samples), task="depth")


def test_populate_task0_keeps_the_depth_maps_bit_for_bit():
    from nas_segm_amd.engine.trainer import populate_task0
    from nas_segm_amd.engine.trainer_common import cache_feature_keys

    net = fresh_net()
    Xy = populate(net)
    _, _, H, W = REC["shape"]
    assert "y" not in Xy and "kd_y" not in Xy and "out_size" in Xy
    depth = Xy["depth"]
    assert tuple(depth.shape) == (6, H, W) and depth.dtype == torch.float32 and depth.is_cuda and depth.is_contiguous()
    want = torch.cat([s["mask"] for s in SAMPLES])
    assert bool(torch.isnan(want).any()) and bool(torch.isinf(want).any()) and bool((want == 0).any())
    assert torch.equal(bits(depth.cpu()), bits(want))  # (holes included, nothing resized)
    keys = cache_feature_keys(Xy)
    assert keys == list(range(len(keys))) and len(keys) >= 1
    net.eval()
    with torch.no_grad():
        for i, s in enumerate(SAMPLES):
            feats = net.encoder(s["image"].to(DEV).contiguous(memory_format=torch.channels_last))
            assert len(feats) == len(keys)
            for k, f in zip(keys, feats):
                assert torch.equal(Xy[k][i], f[0]), (i, k)
    assert tuple(Xy["out_size"]) == tuple(feats[0].shape[2:])
    # maps of another size cannot join the cache
    odd = SAMPLES[:1] + [{"image": SAMPLES[1]["image"], "mask": SAMPLES[1]["mask"][:, :-1]}]
    with pytest.raises(ValueError, match="one size"):
        populate_task0.__wrapped__(net, odd, None, 2, task="depth")


def _record_losses(monkeypatch, trainer):
    real, losses = trainer._loss_value, []
    monkeypatch.setattr(trainer, "_loss_value", lambda s, loss: losses.append(real(s, loss)) or losses[-1])
    return losses


@pytest.mark.parametrize("aux_weight", [-1, 0.15])
@pytest.mark.parametrize("full_size", [False, True], ids=["berhu", "berhu_up"])
def test_train_task0_depth_epoch_equals_a_step_written_from_existing_pieces(full_size, aux_weight, monkeypatch):
    from nas_segm_amd.engine import trainer
    from nas_segm_amd.engine.trainer_common import cache_feature_keys, clip_and_step
    from nas_segm_amd.nn import BerHuLoss

    F = Fn()
    monkeypatch.setenv("NASSEG_GRAPH", "0")
    crit = BerHuLoss(0.0, VMAX, full_size=full_size)
    # the engine
    net = fresh_net()
    enc0 = cpu_sd(net.encoder)
    Xy = populate(net)
    od = adam(net)
    losses = _record_losses(monkeypatch, trainer)
    np.random.seed(5)
    assert trainer.train_task0.__wrapped__(Xy, net, od, 0, crit, None, 2, False, False, 0.0, 3.0, False,
                                           aux_weight=aux_weight) is None
    assert len(losses) == 3 and all(math.isfinite(v) and v > 0 for v in losses)
    enc1 = cpu_sd(net.encoder)
    for k in enc0:  # (BatchNorm buffers included: the encoder only ever ran in eval mode)
        assert torch.equal(bits(enc0[k]), bits(enc1[k])), k
    # by hand: gather_rows of the features, the decoder, the criterion on the GATHERED maps, backward, clip_and_step
    ref = fresh_net()
    Xr = populate(ref)
    oref = adam(ref)
    ref.decoder.train()
    params = list(ref.decoder.parameters())
    np.random.seed(5)
    order = np.arange(6)
    np.random.shuffle(order)
    want = []
    for i in range(3):
        idx = torch.as_tensor(order[2 * i:2 * i + 2], dtype=torch.int64).to(DEV)
        out, aux_outs = ref.decoder([F.gather_rows(Xr[k], idx) for k in cache_feature_keys(Xr)])
        target = Xr["depth"][idx]
        loss = crit(out, target)
        if aux_weight > 0:
            assert len(aux_outs) == 3
            for a in aux_outs:
                loss = loss + crit(a, target) * aux_weight
        oref.zero_grad(set_to_none=True)
        loss.backward()
        clip_and_step([(params, 3.0, oref)])
        want.append(loss.item())
    print("full_size", full_size, "aux_weight", aux_weight, "losses", losses, want)
    assert losses == want
    sd, sr = cpu_sd(net.decoder), cpu_sd(ref.decoder)
    for k in sr:
        assert torch.equal(sd[k], sr[k]), k


@pytest.mark.parametrize("full_size", [False, True], ids=["berhu", "berhu_up"])
def test_train_task0_depth_host_launches_equal_the_replay(full_size, monkeypatch):
    from nas_segm_amd.engine import graphed, trainer
    from nas_segm_amd.nn import BerHuLoss

    crit = BerHuLoss(0.0, VMAX, full_size=full_size)
    made = []
    orig = graphed.GraphedTask0Step

    def counted(*a, **k):
        made.append(k.get("depth_crit"))
        return orig(*a, **k)

    monkeypatch.setattr(graphed, "GraphedTask0Step", counted)

    def go(mode):
        monkeypatch.setenv("NASSEG_GRAPH", mode)
        del made[:]
        net = fresh_net()
        Xy = populate(net)
        od = adam(net)
        losses = _record_losses(monkeypatch, trainer)
        np.random.seed(6)
        assert trainer.train_task0.__wrapped__(Xy, net, od, 0, crit, None, 2, False, False, 0.0, 3.0, False,
                                               aux_weight=0.15) is None
        return list(losses), cpu_sd(net), list(made)

    l0, sd0, made0 = go("0")
    l1, sd1, made1 = go("1")
    print("full_size", full_size, "losses", l0, l1)
    assert made0 == [] and len(made1) == 1 and made1[0] is crit, (made0, made1)
    assert len(l0) == 3 and l0 == l1, (l0, l1)
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k


def _config():
    return load_json("controller.json")["cvpr"]["samples"][0]["config"]


def test_evaluate_depth_candidate_with_decoder_only_epochs(monkeypatch):
    from nas_segm_amd.engine.search import evaluate_candidate
    from nas_segm_amd.nn import BerHuLoss

    train, val = depth_samples(2, seed=33, batch=2), depth_samples(1, seed=34, batch=2)
    kw = dict(ctrl_version="cvpr", agg_size=48, aux_cell=True, repeats=1, epochs=1, device=DEV, task="depth",
              min_depth=1e-3, max_depth=VMAX, depth_crit=BerHuLoss(0.0, VMAX, full_size=True), task0_epochs=2)
    monkeypatch.setenv("NASSEG_GRAPH", "0")
    torch.manual_seed(41)
    np.random.seed(7)  # (train_task0 shuffles the cache rows)
    stats_e, stats_r = {}, {}
    eager = evaluate_candidate(_config(), train, val, stats=stats_e, **kw)
    monkeypatch.setenv("NASSEG_GRAPH", "1")
    torch.manual_seed(41)
    np.random.seed(7)
    replayed = evaluate_candidate(_config(), train, val, graphed=True, stats=stats_r, **kw)
    print("rewards", eager, replayed)
    assert 0.0 < eager <= 1.0 and stats_e["params"] > 0 and stats_r == stats_e
    assert replayed == eager, (replayed, eager)


def test_evaluate_candidate_without_decoder_only_epochs_is_unchanged():
    from nas_segm_amd.engine.search import evaluate_candidate

    train, val = depth_samples(2, seed=35, batch=2), depth_samples(1, seed=36, batch=2)
    kw = dict(ctrl_version="cvpr", agg_size=48, aux_cell=True, repeats=1, epochs=1, device=DEV, task="depth",
              min_depth=1e-3, max_depth=VMAX)
    stats_p, stats_z = {}, {}
    torch.manual_seed(42)
    plain = evaluate_candidate(_config(), train, val, stats=stats_p, **kw)
    torch.manual_seed(42)
    zero = evaluate_candidate(_config(), train, val, task0_epochs=0, stats=stats_z, **kw)
    print("rewards", plain, zero)
    # (stats are filled only when every stage ran: a candidate scored 0 for a failure leaves them empty)
    assert stats_p["params"] > 0 and stats_z == stats_p
    assert 0.0 <= plain <= 1.0 and zero == plain, (zero, plain)


def test_evaluate_segmentation_candidate_with_a_decoder_only_epoch(monkeypatch):
    from nas_segm_amd.engine.search import evaluate_candidate

    g = torch.Generator().manual_seed(37)
    _, _, H, W = REC["shape"]

    def batches(n):
        out = []
        for _ in range(n):
            mask = torch.randint(0, 5, (2, H, W), generator=g)
            mask[torch.rand(2, H, W, generator=g) < 0.1] = 255
            out.append({"image": torch.randn(2, 3, H, W, generator=g), "mask": mask.to(torch.uint8)})
        return out

    train, val = batches(2), batches(1)
    kw = dict(ctrl_version="cvpr", num_classes=5, agg_size=48, aux_cell=True, repeats=1, epochs=1, device=DEV,
              task0_epochs=1, omit_classes=())
    monkeypatch.setenv("NASSEG_GRAPH", "0")
    torch.manual_seed(43)
    np.random.seed(8)
    stats_e, stats_r = {}, {}
    eager = evaluate_candidate(_config(), train, val, stats=stats_e, **kw)
    monkeypatch.setenv("NASSEG_GRAPH", "1")
    torch.manual_seed(43)
    np.random.seed(8)
    replayed = evaluate_candidate(_config(), train, val, graphed=True, stats=stats_r, **kw)
    print("rewards", eager, replayed)
    # (stats are filled only when every stage ran: a candidate scored 0 for a failure leaves them empty)
    assert stats_e["params"] > 0 and stats_r == stats_e
    assert 0.0 <= eager <= 1.0 and replayed == eager, (replayed, eager)
