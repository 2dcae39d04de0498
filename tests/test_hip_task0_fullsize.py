"""The decoder-only (task0) stage on full-size labels, on the GPU: the row-indexed full-size cross-entropy
(csrc/loss_up.hip: nasseg_ce_up_rows_fwd / _bwd; ``F.cross_entropy_upsampled(rows=)``: the labels are read in place
from a cache through the batch's row index), the ``'y_full'`` entry of ``populate_task0(full_size_labels=True)``,
``train_task0`` with an ``nn.SegmCrossEntropy(full_size=True)`` - launched from the host and replayed - and
``evaluate_candidate(task0_epochs=, segm_crit=)``.

Yardstick of the kernels: the un-indexed function on the gathered copy ``cache[rows].contiguous()`` (the index
applied by torch on the device), compared with ``torch.equal`` - no tolerance.  The un-indexed entry points are pinned
against float64 by test_hip_upsampled_ce.py; the indexed ones claim their bits."""
import math

import numpy as np
import pytest
import torch

from _util import build_product_net, load_json

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IGNORE = 255
OHEM = dict(thresh=0.7, min_kept=5)

# (B, C, h, w, H, W, N, rows, a cache row made all `ignore` or None)
CASES = [
    (3, 5, 5, 7, 13, 18, 6, [4, 0, 4], 0),    # repeats, unordered, ratios not integral, partial 8 x 8 tiles
    (1, 2, 1, 1, 3, 2, 2, [1], None),         # smallest
    (2, 19, 9, 17, 9, 17, 4, [3, 1], None),   # equal sizes (the identity); a tile boundary on both axes
    (2, 70, 3, 4, 10, 9, 3, [2, 2], None),    # C > 64: two channel chunks, the element-wise staging path
    (2, 21, 12, 10, 5, 4, 5, [0, 4], None),   # labels smaller than the logits: untouched logits get exact zeros
]
IDS = ["3x5x5x7", "smallest", "identity", "C70", "shrink"]


def Fn():
    from nas_segm_amd import functional

    return functional


def make_labels(N, C, H, W, seed, dtype, all_ignore=()):
    """labels in [0, C) with about 20 % ``IGNORE``; every row holds other data; pixel (0, 0) of every row stays valid;
    the rows ``all_ignore`` hold ``IGNORE`` only"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, C, (N, H, W), generator=g)
    hole = torch.rand(N, H, W, generator=g) < 0.2
    hole[:, 0, 0] = False
    t[hole] = IGNORE
    for r in all_ignore:
        t[r] = IGNORE
    return t.to(dtype)


def make_logits(B, C, h, w, dtype, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = (3.0 * torch.randn(B, C, h, w, generator=g)).to(dtype).to(DEV)
    return x.contiguous(memory_format=torch.channels_last)


def class_weights(C):
    return (0.5 + torch.arange(C, dtype=torch.float32) / C).to(DEV)


def run(logits, target, weight, cfg, rows=None, scale=2.5):
    """-> (loss, pixel_loss, tau, counts, dlogits) of one forward + backward, ``scale`` applied upstream"""
    x = logits.clone().requires_grad_(True)
    kw = {} if rows is None else {"rows": rows}
    loss, pl, tau, counts = Fn().cross_entropy_upsampled(x, target, weight, IGNORE, return_parts=True, **cfg, **kw)
    (scale * loss).backward()
    return loss.detach().clone(), pl.clone(), tau.clone(), counts.clone(), x.grad


def bits(t):
    """a floating tensor as integers: NaN == NaN, -0 != 0"""
    if not t.is_floating_point():
        return t
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def assert_same(got, want, what):
    for name, a, b in zip(("loss", "pixel_loss", "tau", "counts", "dlogits"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b)), (what, name, a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ldtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("options", ["plain", "weights_ohem"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_indexed_kernels_give_the_bits_of_the_gathered_copy(case, options, ldtype, dtype):
    from nas_segm_amd.nn import SegmCrossEntropy

    B, C, h, w, H, W, N, rows, ignore_row = case
    cache = make_labels(N, C, H, W, 11, ldtype, () if ignore_row is None else (ignore_row,)).to(DEV)
    rows_d = torch.tensor(rows, dtype=torch.int64, device=DEV)
    cache0, rows0 = cache.clone(), rows_d.clone()
    gathered = cache[rows_d].contiguous()
    assert not torch.equal(gathered, cache[:B])  # (non-identity rows: ignoring them shows)
    weight, cfg = (None, {}) if options == "plain" else (class_weights(C), OHEM)
    x = make_logits(B, C, h, w, dtype)
    want = run(x, gathered, weight, cfg)
    got = run(x, cache, weight, cfg, rows_d)
    print(case[:7], options, ldtype, dtype, "loss", float(got[0]), "tau", float(got[2]), "counts", got[3].tolist())
    assert_same(got, want, options)
    k, n_valid, n_kept = want[3].tolist()
    assert n_valid >= 1 and n_kept >= 1 and math.isfinite(float(want[0])) and float(want[0]) > 0
    if cfg:  # (the selection and the weighted sum pass ran)
        assert k == min(OHEM["min_kept"], n_valid) and n_kept >= k and math.isfinite(float(want[2]))
    assert tuple(got[1].shape) == (B, H, W) and got[4].dtype == dtype
    assert got[4].is_contiguous(memory_format=torch.channels_last) and float(got[4].float().abs().max()) > 0
    if ignore_row is not None:  # (an all-ignore row indexed together with valid ones: its image gets exact zeros)
        b = rows.index(ignore_row)
        assert float(got[4][b].float().abs().max()) == 0.0 and bool((got[1][b] == -1).all())
    if H < h:  # (logits no label pixel touches: exact zeros, beside logits that are touched)
        assert bool((got[4].float() == 0).any())
    # neither the cache nor the index is written, forward or backward
    assert torch.equal(cache, cache0) and torch.equal(rows_d, rows0)
    # the criterion module: the same bits
    crit = SegmCrossEntropy(weight=weight, ignore_index=IGNORE, full_size=True, **cfg)
    xm = x.clone().requires_grad_(True)
    lm = crit(xm, cache, rows=rows_d)
    (2.5 * lm).backward()
    assert torch.equal(bits(lm.detach()), bits(want[0])) and torch.equal(bits(xm.grad), bits(want[4]))
    assert torch.equal(bits(crit(x, gathered)), bits(want[0]))  # (without rows: exactly as ever)


def test_an_upstream_scale_reaches_the_indexed_gradient():
    B, C, h, w, H, W, N, rows, ignore_row = CASES[0]
    cache = make_labels(N, C, H, W, 12, torch.uint8, (ignore_row,)).to(DEV)
    rows_d = torch.tensor(rows, dtype=torch.int64, device=DEV)
    x = make_logits(B, C, h, w, torch.float32)
    one = run(x, cache, class_weights(C), OHEM, rows_d, scale=1.0)
    scaled = run(x, cache, class_weights(C), OHEM, rows_d, scale=2.5)
    assert torch.equal(one[0], scaled[0]) and float(one[4].abs().max()) > 0
    # (a logit's gradient is a sum of up to (2 * 13 / 5 + 2) * (2 * 18 / 7 + 2) = 50 signed terms, each rounded a few
    #  times at 2^-24 of its own size, so the two differ by roundings relative to the LARGEST gradient, not to each
    #  value: 50 terms x 4 roundings x 2^-24 = 1.2e-5 of a sum of magnitudes taken as at most 8 times the largest)
    gmax = float(one[4].abs().max())
    err = float((scaled[4] - 2.5 * one[4]).abs().max())
    print("scale: max |d(2.5) - 2.5 d(1)|", err, "largest gradient", gmax)
    assert err <= 1e-4 * 2.5 * gmax and not torch.equal(scaled[4], one[4])


def test_device_refusals_of_rows():
    F = Fn()
    cache = make_labels(4, 5, 8, 8, 15, torch.uint8).to(DEV)
    x = make_logits(2, 5, 2, 2, torch.float32)
    rows_d = torch.tensor([3, 1], dtype=torch.int64, device=DEV)
    with pytest.raises(F.NassegError, match="cross_entropy_upsampled.*contiguous"):  # (read in place: never copied)
        F.cross_entropy_upsampled(x, cache.transpose(1, 2), rows=rows_d)
    with pytest.raises(F.NassegError, match="cross_entropy_upsampled.*rows"):
        F.cross_entropy_upsampled(x, cache, rows=rows_d.to(torch.int32))
    with pytest.raises(F.NassegError, match="cross_entropy_upsampled.*one cache row per image"):
        F.cross_entropy_upsampled(x, cache, rows=rows_d[:1])
    with pytest.raises(F.NassegError, match="cross_entropy_upsampled.*cache"):
        F.cross_entropy_upsampled(x, cache.float(), rows=rows_d)
    with pytest.raises(F.NassegError, match="HIP device"):
        F.cross_entropy_upsampled(x, cache, rows=rows_d.cpu())
    with pytest.raises(IndexError):
        F.cross_entropy_upsampled(x, cache, rows=torch.tensor([4, 0]))


def test_cache_rows_beyond_two_to_the_32_pixels():
    """rows[b] * H * W is 64-bit: row 4096 of a (4097, 1024, 1024) uint8 cache starts at pixel 2^32"""
    N, H, W, C = 4097, 1024, 1024, 3
    cache = torch.empty((N, H, W), device=DEV, dtype=torch.uint8)  # (only rows 0 and 4096 are written)
    two = make_labels(2, C, H, W, 16, torch.uint8).to(DEV)
    cache[0].copy_(two[0])
    cache[4096].copy_(two[1])
    rows_d = torch.tensor([4096, 0], dtype=torch.int64, device=DEV)
    gathered = torch.stack([two[1], two[0]]).contiguous()
    x = make_logits(2, C, 32, 32, torch.float32)
    cfg = dict(thresh=0.7, min_kept=1000)
    want = run(x, gathered, class_weights(C), cfg)
    got = run(x, cache, class_weights(C), cfg, rows_d)
    print("loss", float(got[0]), "counts", got[3].tolist())
    assert want[3].tolist()[1] > 0
    assert_same(got, want, "2^32")
    del cache


# ---------------------------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------------------------
REC = load_json("nets_meta.json")["cvpr_arch1_search"]
SIZE = 64
AUX = 0.15


def seg_samples(n, seed, batch=1, dtype=torch.uint8, classes=None):
    """n samples of {"image", "mask"}: labels with about 20 % ``IGNORE``"""
    g = torch.Generator().manual_seed(seed)
    classes = REC["classes"] if classes is None else classes
    out = []
    for i in range(n):
        image = torch.randn(batch, 3, SIZE, SIZE, generator=g)
        out.append({"image": image, "mask": make_labels(batch, classes, SIZE, SIZE, seed * 100 + i, dtype)})
    return out


def fresh_net():
    assert REC["n_aux"] == 3
    return build_product_net(REC["kind"], REC["genotype"], REC["classes"], REC["dec_kwargs"], REC["seed"]).to(DEV)


def adam(net):
    return torch.optim.Adam(net.decoder.parameters(), lr=3e-3, weight_decay=1e-5)


def cpu_sd(module):
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


def full_crit(**kw):
    from nas_segm_amd.nn import SegmCrossEntropy

    return SegmCrossEntropy(full_size=True, **dict(dict(thresh=0.7, min_kept=500), **kw)).prepare(DEV)


SAMPLES = seg_samples(6, seed=31)


def populate(net, samples=SAMPLES, **kw):
    from nas_segm_amd.engine.trainer import populate_task0

    return populate_task0.__wrapped__(net, samples, None, len(samples), **dict(dict(full_size_labels=True), **kw))


@pytest.mark.parametrize("ldtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
def test_populate_task0_keeps_the_full_size_labels_beside_every_other_entry(ldtype):
    from nas_segm_amd.engine.trainer import populate_task0
    from nas_segm_amd.engine.trainer_common import cache_feature_keys

    samples = seg_samples(4, seed=32, dtype=ldtype)
    net = fresh_net()
    Xy = populate(net, samples)
    plain = populate(net, samples, full_size_labels=False)
    assert "y_full" not in plain and set(Xy) == set(plain) | {"y_full"}
    y_full = Xy["y_full"]
    assert tuple(y_full.shape) == (4, SIZE, SIZE) and y_full.dtype == ldtype and y_full.is_cuda
    assert y_full.is_contiguous()
    assert torch.equal(y_full.cpu(), torch.cat([s["mask"] for s in samples]))  # (in order, nothing resized)
    for k in plain:
        if k == "out_size":
            assert tuple(Xy[k]) == tuple(plain[k])
        else:
            assert Xy[k].dtype == plain[k].dtype and torch.equal(Xy[k], plain[k]), k
    assert tuple(Xy["y"].shape[1:]) == tuple(Xy["out_size"]) != (SIZE, SIZE) and Xy["y"].dtype == torch.int64
    keys = cache_feature_keys(Xy)
    assert keys == list(range(len(keys))) and keys == cache_feature_keys(plain) and len(keys) >= 1
    # masks of another size cannot join the cache
    odd = samples[:1] + [{"image": samples[1]["image"], "mask": samples[1]["mask"][:, :-1]}]
    with pytest.raises(ValueError, match="one size"):
        populate_task0.__wrapped__(net, odd, None, 2, full_size_labels=True)


def _record_losses(monkeypatch, trainer):
    real, losses = trainer._loss_value, []
    monkeypatch.setattr(trainer, "_loss_value", lambda s, loss: losses.append(real(s, loss)) or losses[-1])
    return losses


def test_train_task0_epoch_equals_a_step_written_from_existing_pieces(monkeypatch):
    from nas_segm_amd.engine import trainer
    from nas_segm_amd.engine.trainer_common import cache_feature_keys, clip_and_step

    F = Fn()
    monkeypatch.setenv("NASSEG_GRAPH", "0")
    crit = full_crit()
    # the engine
    net = fresh_net()
    enc0 = cpu_sd(net.encoder)
    Xy = populate(net)
    od = adam(net)
    losses = _record_losses(monkeypatch, trainer)
    np.random.seed(5)
    assert trainer.train_task0.__wrapped__(Xy, net, od, 0, crit, None, 2, False, False, 0.0, 3.0, False,
                                           aux_weight=AUX) is None
    assert len(losses) == 3 and all(math.isfinite(v) and v > 0 for v in losses)
    enc1 = cpu_sd(net.encoder)
    for k in enc0:  # (BatchNorm buffers included: the encoder only ever ran in eval mode)
        assert torch.equal(enc0[k], enc1[k]), k
    # by hand: gather_rows of the features, the decoder, the un-indexed loss on the GATHERED labels, backward,
    # clip_and_step
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
        target = Xr["y_full"][idx]
        assert tuple(out.shape[2:]) != tuple(target.shape[1:])
        loss = F.cross_entropy_upsampled(out, target, None, IGNORE, 0.7, 500)
        assert len(aux_outs) == 3
        for a in aux_outs:
            loss = loss + F.cross_entropy_upsampled(a, target, None, IGNORE, 0.7, 500) * AUX
        oref.zero_grad(set_to_none=True)
        loss.backward()
        clip_and_step([(params, 3.0, oref)])
        want.append(loss.item())
    print("losses", losses, want)
    assert losses == want
    sd, sr = cpu_sd(net.decoder), cpu_sd(ref.decoder)
    for k in sr:
        assert torch.equal(sd[k], sr[k]), k


def test_train_task0_host_launches_equal_the_replay(monkeypatch):
    from nas_segm_amd.engine import graphed, trainer

    crit = full_crit()
    made = []
    orig = graphed.GraphedTask0Step

    def counted(*a, **k):
        made.append(k.get("segm_crit"))
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
                                               aux_weight=AUX) is None
        return list(losses), cpu_sd(net), list(made)

    l0, sd0, made0 = go("0")
    l1, sd1, made1 = go("1")
    print("losses", l0, l1)
    assert made0 == [] and len(made1) == 1 and made1[0] is crit, (made0, made1)
    assert len(l0) == 3 and l0 == l1, (l0, l1)
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k


def test_a_changed_full_size_is_a_new_task0_capture(monkeypatch):
    from nas_segm_amd.engine.trainer import _task0_stepper, make_task0_step

    idx = [np.array([4, 1]), np.array([0, 5])]

    def setup():
        net = fresh_net()
        net.decoder.train()
        return full_crit(), net, populate(net), adam(net)

    def host(flags):
        crit, net, Xy, od = setup()
        out = []
        for i, flag in zip(idx, flags):
            crit.full_size = flag
            out.append(float(make_task0_step(Xy, net, od, 2, IGNORE, 3.0, AUX, segm_crit=crit)(i)))
        return out

    monkeypatch.setenv("NASSEG_GRAPH", "0")
    want, unchanged = host((True, False)), host((True, True))
    assert want[0] == unchanged[0] and want[1] != unchanged[1]
    monkeypatch.setenv("NASSEG_GRAPH", "1")
    crit, net, Xy, od = setup()
    args = (Xy, net, od, 2, IGNORE, 3.0, AUX)
    first = _task0_stepper(*args, segm_crit=crit)
    assert first is not None and _task0_stepper(*args, segm_crit=crit) is first
    got = [float(first.step(idx[0]))]
    crit.full_size = False
    second = _task0_stepper(*args, segm_crit=crit)
    assert second is not None and second is not first
    got.append(float(second.step(idx[1])))
    assert got == want, (got, want)
    # the first capture still replays what it recorded: the full-size step, on the parameters as they now are
    crit2, net2, Xy2, od2 = setup()
    monkeypatch.setenv("NASSEG_GRAPH", "0")
    third = []
    for i, flag in zip(idx + idx[:1], (True, False, True)):
        crit2.full_size = flag
        third.append(float(make_task0_step(Xy2, net2, od2, 2, IGNORE, 3.0, AUX, segm_crit=crit2)(i)))
    assert third[:2] == want and float(first.step(idx[0])) == third[2]


def test_distillation_with_a_full_size_criterion_is_the_host_composition(monkeypatch):
    from torch import nn

    from nas_segm_amd.engine import graphed
    from nas_segm_amd.engine.trainer import make_task0_step
    from nas_segm_amd.engine.trainer_common import cache_feature_keys, task0_loss

    F = Fn()
    crit, kd_crit, kd_coeff = full_crit(), nn.MSELoss(), 0.5
    net = fresh_net()
    Xy = populate(net)
    g = torch.Generator().manual_seed(9)
    oh, ow = Xy["out_size"]
    Xy["kd_y"] = torch.randn(6, REC["classes"], oh, ow, generator=g).to(DEV).contiguous(
        memory_format=torch.channels_last)
    net.decoder.train()
    idx = torch.tensor([5, 2], dtype=torch.int64, device=DEV)

    def by_hand(kd):
        out, aux_outs = net.decoder([F.gather_rows(Xy[k], idx) for k in cache_feature_keys(Xy)])
        target = Xy["y_full"][idx]
        loss = F.cross_entropy_upsampled(out, target, None, IGNORE, 0.7, 500)
        if kd:
            loss = loss + kd_coeff * kd_crit(F.bilinear_resize(out, Xy["out_size"]), Xy["kd_y"][idx])
        for a in aux_outs:
            loss = loss + F.cross_entropy_upsampled(a, target, None, IGNORE, 0.7, 500) * AUX
        return loss

    with torch.no_grad():
        want, without = by_hand(True), by_hand(False)
        got = task0_loss(Xy, idx, net.decoder, IGNORE, AUX, kd_coeff, kd_crit, segm_crit=crit)
    print("loss", float(got), float(want), "without the term", float(without))
    assert torch.equal(got, want) and float(want) != float(without)
    # the step: launched from the host (no replayed step has the term), the same loss
    monkeypatch.setattr(graphed, "GraphedTask0Step", lambda *a, **k: pytest.fail("replayed"))
    monkeypatch.setenv("NASSEG_GRAPH", "1")
    step = make_task0_step(Xy, net, adam(net), 2, IGNORE, 3.0, AUX, False, True, kd_coeff, kd_crit, crit)
    before = cpu_sd(net.decoder)
    assert float(step(np.array([5, 2]))) == float(want)
    after = cpu_sd(net.decoder)
    assert any(not torch.equal(before[k], after[k]) for k in before)


def _config():
    return load_json("controller.json")["cvpr"]["samples"][0]["config"]


def _batches(n, seed):
    return seg_samples(n, seed, batch=2, classes=5)


def test_evaluate_candidate_with_a_full_size_decoder_only_epoch(monkeypatch):
    from nas_segm_amd.engine.inference import validate
    from nas_segm_amd.engine.search import build_candidate, evaluate_candidate
    from nas_segm_amd.engine.trainer import populate_task0, train_segmenter, train_task0

    train, val = _batches(2, 37), _batches(1, 38)
    monkeypatch.setenv("NASSEG_GRAPH", "0")

    def crit():
        from nas_segm_amd.nn import SegmCrossEntropy

        return SegmCrossEntropy(full_size=True)

    torch.manual_seed(43)
    np.random.seed(8)  # (train_task0 shuffles the cache rows)
    stats = {}
    got = evaluate_candidate(_config(), train, val, ctrl_version="cvpr", num_classes=5, agg_size=48, aux_cell=True,
                             repeats=1, epochs=1, device=DEV, omit_classes=(), stats=stats, task0_epochs=1,
                             segm_crit=crit())
    # the two stages by hand, on the same seed
    torch.manual_seed(43)
    np.random.seed(8)
    c = crit()
    segmenter = build_candidate(_config(), "cvpr", 5, 48, True, 1, DEV)
    model = segmenter.module
    oe = torch.optim.SGD(model.encoder.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-5)
    od = torch.optim.Adam(model.decoder.parameters(), lr=3e-3, weight_decay=1e-5)
    cache = populate_task0(segmenter, train, None, 4, full_size_labels=True)
    assert tuple(cache["y_full"].shape) == (4, SIZE, SIZE)
    assert train_task0(cache, segmenter, od, 0, c, None, 2, False, False, 0.0, 3.0, False, aux_weight=AUX) is None
    segmenter.train()
    assert train_segmenter(segmenter, train, oe, od, 0, c, False, 3.0, 3.0, False, print_every=10 ** 9,
                           aux_weight=AUX) is None
    want = float(validate(segmenter, val, 0, 0, num_classes=5, print_every=10 ** 9, omit_classes=[]))
    print("rewards", got, want)
    assert stats["params"] > 0 and 0.0 <= got <= 1.0 and got == want, (got, want)


def test_evaluate_candidate_without_decoder_only_epochs_is_unchanged():
    from nas_segm_amd.engine.search import evaluate_candidate
    from nas_segm_amd.nn import SegmCrossEntropy

    train, val = _batches(2, 39), _batches(1, 40)
    kw = dict(ctrl_version="cvpr", num_classes=5, agg_size=48, aux_cell=True, repeats=1, epochs=1, device=DEV,
              omit_classes=())
    stats_p, stats_z = {}, {}
    torch.manual_seed(44)
    plain = evaluate_candidate(_config(), train, val, stats=stats_p, segm_crit=SegmCrossEntropy(full_size=True), **kw)
    torch.manual_seed(44)
    zero = evaluate_candidate(_config(), train, val, task0_epochs=0, stats=stats_z,
                              segm_crit=SegmCrossEntropy(full_size=True), **kw)
    print("rewards", plain, zero)
    # (stats are filled only when every stage ran: a candidate scored 0 for a failure leaves them empty)
    assert stats_p["params"] > 0 and stats_z == stats_p
    assert 0.0 <= plain <= 1.0 and zero == plain, (zero, plain)
