"""Prediction (engine/predict.py, csrc/predict.hip) on the MI355X, batch 1, seeded weights:

  forward  ms per eval forward (Predictor.logits), host-launched against replayed from a hipGraph: WACV arch0 and
           arch1 at 1x3x1024x2048 (the reference README's latency table) and CVPR arch0 at 1x3x512x512.
  post     1x19x256x512 logits -> 1024x2048 labels: the fused cubic + argmax kernel, F.interpolate(bicubic) + argmax
           on the same device (a cost reference: its numerics differ), and the notebooks' host path (copy out, the
           numpy restatement, argmax).
  e2e      ms per pred(img) of a uint8 2048x1024 image (WACV arch0, labels at the image's size), host-launched and
           replayed.
  ensemble the test-time ensemble of WACV arch0 on a 2048x1024 image, scales 0.5 .. 1.75 in steps of 0.25 plus
           mirroring (12 views): the fused launch alone (F.fuse_views on the 12 logit maps), the same fusion composed
           from the single-view entry points (per view F.resize_cubic to full size, torch softmax and add; then
           argmax - the mirrored maps flipped outside the timed region), and pred(img) end to end, host-launched
           and replayed.

Device times: HIP events around KBENCH_ITERS calls (default 20) after 3 warm-up calls; host path: wall clock.
usage (GPU box): python tools/kbench_predict.py [forward|post|e2e|ensemble|all]   One JSON line per measurement on stdout."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import nas_segm_amd  # noqa: E402,F401
from nas_segm_amd import functional as F  # noqa: E402
from nas_segm_amd.data import datasets as D  # noqa: E402
from nas_segm_amd.engine.inference import Predictor  # noqa: E402
from _util import build_product_net, load_json  # noqa: E402

DEV = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "20"))


def net_of(name):
    rec = load_json("nets_meta.json")[name]
    return build_product_net(rec["kind"], rec["genotype"], rec["classes"], rec["dec_kwargs"], 0).to(DEV).eval()


def device_ms(fn, n=ITERS, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def emit(**kw):
    print(json.dumps(kw), flush=True)


def forward():
    for name, (h, w) in (("wacv_arch0", (1024, 2048)), ("wacv_arch1", (1024, 2048)), ("cvpr_arch0", (512, 512))):
        net = net_of(name)
        x = torch.randn(1, 3, h, w, generator=torch.Generator().manual_seed(0)).to(DEV)
        for graph in (False, True):
            pred = Predictor(net, graph=graph)
            ms = device_ms(lambda: pred.logits(x))
            emit(bench="forward", net=name, shape=[1, 3, h, w], graph=graph, ms=round(ms, 3))
        del net, pred
        torch.cuda.empty_cache()


def post():
    B, C, h, w, H, W = 1, 19, 256, 512, 1024, 2048
    x = torch.randn(B, C, h, w, generator=torch.Generator().manual_seed(0)).to(DEV).contiguous(
        memory_format=torch.channels_last)
    for dtype in (torch.float32, torch.bfloat16):
        xd = x.to(dtype)
        emit(bench="post", path="resize_cubic_argmax", dtype=str(dtype)[6:],
             us=round(1e3 * device_ms(lambda: F.resize_cubic_argmax(xd, (H, W))), 1))
        emit(bench="post", path="resize_cubic", dtype=str(dtype)[6:],
             us=round(1e3 * device_ms(lambda: F.resize_cubic(xd, (H, W))), 1))
    xc = x.contiguous()

    def interp():
        y = torch.nn.functional.interpolate(xc, size=(H, W), mode="bicubic", align_corners=False)
        return y.argmax(1).to(torch.uint8)

    emit(bench="post", path="torch_bicubic_argmax", dtype="float32", us=round(1e3 * device_ms(interp), 1))
    reps = 2
    t0 = time.perf_counter()
    for _ in range(reps):
        a = x[0].permute(1, 2, 0).cpu().numpy()
        np.argmax(D.resize_cubic_to(a, (H, W)), axis=2).astype(np.uint8)
    emit(bench="post", path="host_numpy", dtype="float32", us=round(1e6 * (time.perf_counter() - t0) / reps, 1))


def e2e():
    net = net_of("wacv_arch0")
    img = np.random.RandomState(0).randint(0, 256, (1024, 2048, 3)).astype(np.uint8)
    for graph in (False, True):
        pred = Predictor(net, graph=graph)
        ms = device_ms(lambda: pred(img))
        emit(bench="e2e", net="wacv_arch0", image=[1024, 2048], graph=graph, ms=round(ms, 3))


def ensemble():
    from nas_segm_amd.engine.predict import view_inputs

    scales = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
    H, W = 1024, 2048
    net = net_of("wacv_arch0")
    img = np.random.RandomState(0).randint(0, 256, (H, W, 3)).astype(np.uint8)
    plain = Predictor(net, graph=False)
    pred = Predictor(net, graph=False, scales=scales, flip=True)
    mirrored = [m for _, m in pred.views]
    x = F.prepare_image(torch.from_numpy(img[None]).to(DEV))
    outs = [plain.logits(xv) for xv in view_inputs(x, pred.views)]
    del x
    tables = F.fuse_tables(outs[0].device, [z.shape[2:] for z in outs], mirrored, H, W)
    fused = F.fuse_views(outs, (H, W), mirrored, tables=tables)
    emit(bench="ensemble", path="fuse_views", views=len(outs), classes=int(outs[0].shape[1]), out=[H, W],
         ms=round(device_ms(lambda: F.fuse_views(outs, (H, W), mirrored, tables=tables)), 3))
    plainly = [z.flip(3).contiguous(memory_format=torch.channels_last) if m else z for z, m in zip(outs, mirrored)]

    def composed():
        total = None
        for z in plainly:
            p = torch.softmax(F.resize_cubic(z, (H, W)), dim=1)
            total = p if total is None else total.add_(p)
        return total.argmax(1).to(torch.uint8)

    differing = float((composed() != fused).float().mean())
    emit(bench="ensemble", path="resize_cubic_softmax_add_argmax", views=len(outs), out=[H, W],
         ms=round(device_ms(composed, n=max(2, ITERS // 4), warm=1), 3), labels_differing=differing)
    del plainly, outs
    torch.cuda.empty_cache()
    for graph in (False, True):
        pred = Predictor(net, graph=graph, scales=scales, flip=True)
        ms = device_ms(lambda: pred(img), n=max(2, ITERS // 2), warm=2)
        emit(bench="ensemble", path="e2e", net="wacv_arch0", image=[H, W], views=len(pred.views), graph=graph,
             ms=round(ms, 3))
    single = Predictor(net, graph=True)
    emit(bench="ensemble", path="e2e_single_view", net="wacv_arch0", image=[H, W], graph=True,
         ms=round(device_ms(lambda: single(img)), 3))


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    emit(device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=ITERS)
    for name, fn in (("forward", forward), ("post", post), ("e2e", e2e), ("ensemble", ensemble)):
        if what in (name, "all"):
            fn()
