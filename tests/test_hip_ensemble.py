"""The test-time ensemble on the device (csrc/ensemble.hip, F.view_image / F.fuse_views, Predictor(scales=, flip=),
validate(scales=, flip=)) against torch on the CPU (the view images), against F.resize_cubic bit for bit (the
resampling), and against the float64 host restatement of the fusion (tests/_ensemble_ref.py).

Bounds
  view images     1e-5, the tolerance of test_bilinear_resize; a bf16 result is that fp32 value rounded once to
                  nearest (8 significant bits: at most 2^-8 of the value) on top.
  probabilities   PROB_BOUND = 2e-6 against float64: four times the largest error observed on the MI355X over the
                  cases of this file - 5.4e-7 for one view (RESAMPLE_CASES: nothing is averaged, probabilities up to
                  1), 1.9e-7 over FUSION_CASES (both modes, fp32 and bf16 views), 1.4e-8 through the networks.  The
                  resampled logits are the reference's own fp32 values (cubic) or within a few roundings of them
                  (bilinear); what is left is fp32 exp, one reciprocal and V additions.  fp32 numpy against float64
                  gives 1.2e-7 on the same inputs on a CPU; the device's exp differs from the host's by a few ulp.
  labels          the rule of test_argmax_confusion_fused_upsample: at most 1e-4 of the pixels differ, each at a float64
                  top-2 gap of the mean probability below 1e-5; the inputs (normal logits, std 3) keep the pixels whose
                  gap is that small below 1e-3 of the map, so the rule is neither vacuous nor tight.
  mean map        (V + 1) * 2^-24 * max |resampled value|: V - 1 fp32 additions of values the reference has bit for
                  bit, and one division (mean_bound below).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import _ensemble_ref as R
import test_hip_predict as TP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
PROB_BOUND = 2e-6


def F():
    from nas_segm_amd import functional

    return functional


def dev(x, dtype=torch.float32):
    return x.to(dtype).to(DEV).contiguous(memory_format=torch.channels_last)


def nhwc(t):
    """device B x C x H x W -> numpy B x H x W x C (a bf16 tensor widened)"""
    return t.detach().float().permute(0, 2, 3, 1).cpu().numpy()


def views_of(B, C, shapes, seed, dtype=torch.float32, std=3.0):
    g = torch.Generator().manual_seed(seed)
    return [dev(torch.randn(B, C, h, w, generator=g) * std, dtype) for h, w in shapes]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
VIEW_CASES = [((37, 53), (74, 101)), ((37, 53), (19, 40)), ((37, 53), (37, 53)), ((64, 96), (112, 168)),
              ((5, 7), (1, 1))]


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirrored"])
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("sizes", VIEW_CASES, ids=lambda s: "{}x{}_to_{}x{}".format(*s[0], *s[1]))
def test_view_image_is_interpolate_and_flip(sizes, C, mirror, dtype):
    (hi, wi), (ho, wo) = sizes
    x = torch.randn(2, C, hi, wi, generator=torch.Generator().manual_seed(hi + C)).to(dtype)
    got = F().view_image(dev(x, dtype), (ho, wo), mirror=mirror)
    assert got.dtype == dtype and tuple(got.shape) == (2, C, ho, wo)
    assert got.is_contiguous(memory_format=torch.channels_last)
    want = TF.interpolate(x.float(), size=(ho, wo), mode="bilinear", align_corners=False)
    if mirror:
        want = want.flip(3)
    err = (got.float().cpu() - want).abs()
    tol = 1e-5 + (want.abs() * 2.0 ** -8 if dtype == BF else 0.0)
    print("view_image max err {:.3e}".format(float(err.max())))
    assert bool((err <= tol).all()), float(err.max())
    if (hi, wi) == (ho, wo) and not mirror:
        assert torch.equal(got.cpu(), x.contiguous(memory_format=torch.channels_last))


# ---------------------------------------------------------------------------------------------------------------------
RESAMPLE_CASES = [  # B, C, h, w, H, W
    (1, 19, 64, 128, 256, 512), (2, 21, 81, 81, 321, 321), (1, 11, 97, 129, 40, 50), (2, 1, 33, 47, 101, 75),
    (1, 64, 9, 11, 37, 29), (1, 64, 40, 48, 33, 35), (2, 19, 31, 45, 31, 45), (1, 40, 61, 77, 90, 131),
]


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", RESAMPLE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_one_view_is_resize_cubic_bit_for_bit(case, dtype):
    B, C, h, w, H, W = case
    (x,) = views_of(B, C, [(h, w)], seed=sum(case), dtype=dtype)
    want = F().resize_cubic(x, (H, W))
    labels, probs, mean = F().fuse_views([x], (H, W), [False], return_probs=True, return_mean=True)
    assert mean.dtype == torch.float32 and tuple(mean.shape) == (B, C, H, W)
    assert mean.is_contiguous(memory_format=torch.channels_last)
    assert np.array_equal(bits(nhwc(mean)), bits(nhwc(want)))
    assert torch.equal(F().fuse_views_mean([x], (H, W), [False]), mean)
    # a mirrored view: the resize of the flipped map
    flipped = F().resize_cubic(x.flip(3), (H, W))
    assert np.array_equal(bits(nhwc(F().fuse_views_mean([x], (H, W), [True]))), bits(nhwc(flipped)))
    # probabilities and labels of the one view: the softmax / argmax of those values
    ref = R.softmax(nhwc(want).astype(np.float64))
    err = float(np.abs(nhwc(probs) - ref).max())
    print("one view probs max err {:.3e}".format(err))
    assert err <= PROB_BOUND
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (B, H, W)
    R.check_labels(labels.cpu().numpy(), ref)
    assert torch.equal(F().fuse_views([x], (H, W), [False]), labels)


def mean_bound(views, mirrored, size, mode):
    """fp32 against float64 for the mean map (the docstring's reasoning): adding V values below rmax one by one
    rounds each partial sum S_k <= k rmax once, the division rounds once more - after the division at most
    ((V + 1) / 2 + 1) 2^-24 rmax, (V + 1) 2^-24 rmax allowed; bilinear resamples in fp32 where the reference
    resamples in float64: two products and a sum per pass, the second pass carrying the first one's error - 6
    roundings of values below the view's largest, 8 allowed"""
    rmax = max(float(np.abs(R.resampled(v, m, size, mode)).max()) for v, m in zip(views, mirrored))
    zmax = max(float(np.abs(v).max()) for v in views)
    return ((len(views) + 1) * rmax + (0.0 if mode == "cubic" else 8.0 * zmax)) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------
FUSION_CASES = [  # B, C, (H, W), view sizes, mirrored
    (1, 19, (96, 160), [(24, 40), (24, 40), (36, 60), (36, 60), (12, 20), (12, 20), (48, 80), (48, 80)],
     [False, True] * 4),
    (2, 11, (40, 50), [(97, 129), (61, 77)], [False, True]),
    (1, 21, (81, 81), [(81, 81), (41, 41), (121, 121)], [False, True, False]),
    (2, 40, (64, 96), [(16, 24), (32, 48), (8, 12), (24, 36)], [False, False, True, True]),
    (2, 1, (50, 70), [(13, 18), (25, 35)], [False, True]),
    (1, 19, (33, 47), [(80, 120), (33, 47), (9, 12), (50, 71), (21, 30)], [True, False, False, True, True]),
]


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["cubic", "bilinear"])
@pytest.mark.parametrize("case", FUSION_CASES, ids=lambda c: "C{}_{}views_{}x{}".format(c[1], len(c[3]), *c[2]))
def test_fusion_is_the_float64_restatement(case, mode, dtype):
    B, C, size, shapes, mirrored = case
    views = views_of(B, C, shapes, seed=C + len(shapes), dtype=dtype)
    labels, probs, mean = F().fuse_views(views, size, mirrored, mode=mode, return_probs=True, return_mean=True)
    assert probs.dtype == torch.float32 and tuple(probs.shape) == (B, C) + size
    host = [nhwc(v) for v in views]
    got_p, got_m, got_l = nhwc(probs), nhwc(mean), labels.cpu().numpy()
    worst, differing, near = 0.0, 0, 0.0
    for b in range(B):
        ref = R.mean_probabilities([v[b] for v in host], mirrored, size, mode)
        worst = max(worst, float(np.abs(got_p[b] - ref).max()))
        ref_m = R.mean_map([v[b] for v in host], mirrored, size, mode)
        assert np.abs(got_m[b] - ref_m).max() <= mean_bound([v[b] for v in host], mirrored, size, mode)
        if C > 1:
            near = max(near, float((R.top2_gap(ref) < 1e-5).mean()))
            differing += R.check_labels(got_l[b], ref)
        else:
            assert not got_l[b].any()
    print("fusion {} {} C={} V={}: probs max err {:.3e}, {} labels differ, near-tie share {:.1e}".format(
        mode, str(dtype)[6:], C, len(views), worst, differing, near))
    assert worst <= PROB_BOUND
    assert near <= max(1e-3, 2.0 / (size[0] * size[1]))  # (the inputs leave the label rule something to decide)
    # the same inputs give the same bits; outputs that are not asked for change nothing
    again = F().fuse_views(views, size, mirrored, mode=mode, return_probs=True)
    assert torch.equal(again[0], labels) and torch.equal(again[1], probs)
    assert torch.equal(F().fuse_views_mean(views, size, mirrored, mode=mode), mean)


def test_bilinear_single_view_labels_are_argmax_confusion():
    """two taps per axis with align_corners=False: the values nasseg_argmax_cm compares"""
    (x,) = views_of(2, 19, [(23, 31)], seed=5)
    gt = torch.randint(0, 19, (2, 90, 121), generator=torch.Generator().manual_seed(6)).to(torch.uint8).to(DEV)
    cm0, want = F().argmax_confusion(x, gt, 19, return_preds=True)
    cm1, got = F().fuse_views([x], (90, 121), [False], mode="bilinear", gt=gt, n_classes=19)
    diff = (got != want).float().mean()
    print("bilinear labels differing from argmax_cm: {:.2e}".format(float(diff)))
    assert float(diff) <= 1e-4
    assert int((cm0 - cm1).abs().sum()) <= 2 * int((got != want).sum())


@pytest.mark.parametrize("mode", ["cubic", "bilinear"])
def test_confusion_matrix_is_fast_cm_of_the_labels_of_the_same_launch(mode):
    from oracle import miou as omiou

    B, C, size = 2, 19, (70, 93)
    views = views_of(B, C, [(18, 24), (35, 47), (18, 24)], seed=9)
    mirrored = [False, False, True]
    gt = torch.randint(0, C, (B,) + size, generator=torch.Generator().manual_seed(10))
    gt[:, 5:8] = 255
    gt[1, :, 40:44] = 200
    gt = gt.to(torch.uint8)
    cm, labels = F().fuse_views(views, size, mirrored, mode=mode, gt=gt.to(DEV), n_classes=C)
    assert cm.dtype == torch.int64 and tuple(cm.shape) == (C, C)
    keep = gt.numpy() < C
    want = omiou.fast_cm(labels.cpu().numpy()[keep], gt.numpy()[keep], C)
    assert np.array_equal(cm.cpu().numpy(), want)
    assert int(cm.sum()) == int(keep.sum()) < gt.numel()
    assert torch.equal(labels, F().fuse_views(views, size, mirrored, mode=mode))
    # a second call accumulates
    cm2, labels2 = F().fuse_views(views, size, mirrored, mode=mode, gt=gt.to(DEV), n_classes=C, cm=cm)
    assert cm2 is cm and torch.equal(labels2, labels)
    assert np.array_equal(cm.cpu().numpy(), 2 * want)
    # more classes than the LDS histogram holds (n * n > 4096): global atomics, the same counts
    big, _ = F().fuse_views(views, size, mirrored, mode=mode, gt=gt.to(DEV), n_classes=80)
    keep = gt.numpy() < 80
    assert np.array_equal(big.cpu().numpy(), omiou.fast_cm(labels.cpu().numpy()[keep], gt.numpy()[keep], 80))


def test_ties_take_the_lowest_index():
    a, b = torch.zeros(2, 9, 13, 17), torch.zeros(2, 9, 7, 5)
    for x in (a, b):
        x[1, 3] = 2.0
        x[1, 7] = 2.0
    for mode in ("cubic", "bilinear"):
        labels = F().fuse_views([dev(a), dev(b)], (29, 31), [False, True], mode=mode).cpu()
        assert bool((labels[0] == 0).all()) and bool((labels[1] == 3).all())


def test_too_many_views_classes_or_matrix_rows_are_refused():
    import ctypes

    from nas_segm_amd import NassegError, lib
    from nas_segm_amd._lib import current_stream

    f = F()
    x = views_of(1, 5, [(6, 7)], seed=1)[0]
    gt = torch.zeros(1, 9, 9, dtype=torch.uint8, device=DEV)
    with pytest.raises(NassegError, match="16"):
        f.fuse_views([x] * 17, (9, 9), [False] * 17)
    with pytest.raises(NassegError, match="64"):
        f.fuse_views(views_of(1, 65, [(6, 7)], seed=1), (9, 9), [False])
    with pytest.raises(NassegError, match="256"):
        f.fuse_views([x], (9, 9), [False], gt=gt, n_classes=257)
    assert tuple(f.fuse_views([x] * 16, (9, 9), [False] * 16).shape) == (1, 9, 9)
    assert tuple(f.fuse_views(views_of(1, 64, [(6, 7)], seed=1), (9, 9), [False]).shape) == (1, 9, 9)
    # the library itself refuses them too, naming the limit
    taps, coef, dims = f.fuse_tables(x.device, [(6, 7)] * 17, [False] * 17, 9, 9)
    labels = torch.empty(1, 9, 9, dtype=torch.uint8, device=DEV)
    cm = torch.zeros(257, 257, dtype=torch.int64, device=DEV)
    hdims = (ctypes.c_int * 51)(*[int(d) for d in dims.ravel()])

    def call(n_views, C, n, cm):
        table = (ctypes.c_void_p * 17)(*[x.data_ptr()] * 17)
        lib.call("nasseg_fuse_views", n_views, table, hdims, taps.data_ptr(), coef.data_ptr(), 4, 1, C, 9, 9,
                 gt.data_ptr(), n, labels.data_ptr(), None, cm, None, current_stream())

    for args, limit in (((17, 5, 0, None), "16"), ((1, 65, 0, None), "64"), ((1, 5, 257, cm.data_ptr()), "256")):
        with pytest.raises(NassegError, match=limit):
            call(*args)
    call(1, 5, 0, None)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
SCALES = (0.75, 1.0, 1.5)


def composed(net, task, img):
    """the ensemble composed from device pieces and fused on the host: F.view_image, Predictor.logits per view,
    then the float64 restatement -> (mean probabilities | mean map) H x W x C, the bound of the mean map"""
    from nas_segm_amd.engine.predict import ensemble_views

    plain = TP.Predictor(net, task=task, graph=False)
    x = F().prepare_image(torch.from_numpy(img[None]).to(DEV))
    H, W = img.shape[:2]
    views = ensemble_views(SCALES, True)
    outs = []
    for s, m in views:
        xv = x if (s == 1.0 and not m) else F().view_image(x, (R.view_size(H, s), R.view_size(W, s)), mirror=m)
        assert tuple(xv.shape[2:]) == (R.view_size(H, s), R.view_size(W, s))
        outs.append(nhwc(plain.logits(xv))[0])
    mirrored = [m for _, m in views]
    fuse = R.mean_probabilities if task == "segm" else R.mean_map
    return fuse(outs, mirrored, (H, W), "cubic"), mean_bound(outs, mirrored, (H, W), "cubic")


@pytest.mark.parametrize("name", ["wacv_arch0", "cvpr_arch0", "cvpr_arch2_depth"])
def test_predictor_ensemble_is_the_composition_and_replays_bit_identically(name):
    net = TP.net_of(name)
    task = "depth" if name.endswith("depth") else "segm"
    img = TP.image(1)
    eager = TP.Predictor(net, task=task, graph=False, scales=SCALES, flip=True)
    replay = TP.Predictor(net, task=task, graph=True, scales=SCALES, flip=True)
    ref, depth_bound = composed(net, task, img)
    a = eager(img)
    assert a.is_cuda and tuple(a.shape) == img.shape[:2]
    if task == "segm":
        p = eager.probabilities(img)
        assert p.dtype == torch.float32 and tuple(p.shape) == (ref.shape[2],) + img.shape[:2]
        err = float(np.abs(p.permute(1, 2, 0).cpu().numpy() - ref).max())
        print("{}: probabilities max err {:.3e}".format(name, err))
        assert err <= PROB_BOUND
        assert a.dtype == torch.uint8
        R.check_labels(a.cpu().numpy(), ref)
        assert torch.equal(replay.probabilities(img), p) and torch.equal(replay.probabilities(img), p)
    else:
        assert a.dtype == torch.float32
        err = float(np.abs(a.cpu().numpy() - ref[:, :, 0]).max())
        print("{}: mean depth max err {:.3e} of {:.3e}".format(name, err, float(np.abs(ref).max())))
        assert err <= depth_bound
    b = replay(img)
    assert torch.equal(a, b) and len(replay.captures) == (2 if task == "segm" else 1)
    assert torch.equal(replay(img), a) and torch.equal(eager(img), a)
    # another output size, a batch
    both = torch.from_numpy(np.stack([img, TP.image(2)])).to(DEV)
    assert torch.equal(replay(both, out_size=(90, 130)), eager(both, out_size=(90, 130)))
    assert torch.equal(eager(both)[0], a)
    # the default Predictor is still the notebooks' pipeline
    want = TP.notebook(net, img)
    single = TP.Predictor(net, task=task)(img)
    if task == "segm":
        assert np.array_equal(single.cpu().numpy(), np.argmax(want, axis=2).astype(np.uint8))
    else:
        assert np.array_equal(bits(single.cpu().numpy()), bits(want[:, :, 0]))


def test_validate_with_views_scores_the_fused_labels():
    from nas_segm_amd.engine.inference import reward_from_cm, validate
    from nas_segm_amd.engine.predict import ensemble_views, view_inputs
    from oracle import miou as omiou

    net = TP.net_of("wacv_arch0")
    C = 19
    g = torch.Generator().manual_seed(3)
    loader = []
    for _ in range(2):
        mask = torch.randint(0, C, (2, 65, 97), generator=g)
        mask[:, 10:13] = 255
        loader.append({"image": torch.randn(2, 3, 65, 97, generator=g), "mask": mask})
    scales = (0.75, 1.0)
    got = validate.__wrapped__(net, loader, 0, 0, num_classes=C, scales=scales, flip=True)
    views = ensemble_views(scales, True)
    cm = np.zeros((C, C), np.int64)
    with torch.no_grad():
        for sample in loader:
            x = dev(sample["image"])
            outs = [net(xv) for xv in view_inputs(x, views)]
            outs = [o[0] if isinstance(o, tuple) else o for o in outs]
            labels = F().fuse_views(outs, (65, 97), [m for _, m in views], mode="bilinear").cpu().numpy()
            gt = sample["mask"].to(torch.uint8).numpy()
            cm += omiou.fast_cm(labels[gt < C], gt[gt < C], C)
    assert int(cm.sum()) == 2 * 2 * 62 * 97
    want = reward_from_cm(cm, [0])[0]
    print("validate reward {} vs {}".format(got, want))
    assert np.array_equal(np.float64(got), np.float64(want), equal_nan=True)
    # the single forward is untouched: scales=None is today's loop
    plain = validate.__wrapped__(net, loader, 0, 0, num_classes=C)
    cm1 = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    with torch.no_grad():
        for sample in loader:
            out = net(dev(sample["image"]))
            out = out[0] if isinstance(out, tuple) else out
            F().argmax_confusion(out, sample["mask"].to(torch.uint8).to(DEV), C, cm=cm1)
    assert np.array_equal(np.float64(plain), np.float64(reward_from_cm(cm1.cpu().numpy(), [0])[0]), equal_nan=True)
