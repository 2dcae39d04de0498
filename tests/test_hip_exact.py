"""Exact-arithmetic tests of the HIP kernels: integer / dyadic inputs, float64 references, NO tolerance.

Every input here is a small integer or a dyadic rational (tests/_exact.py) chosen so that each product and each
partial sum - in any order - is exactly representable in fp32 (``assert_exactly_summable``: the sum of the absolute
values of an output element's terms stays below 2^24 units, computed from the reference alone).  fp32 FMA, MFMA
accumulation, slab / row partials and fp64 finalisation then all return the mathematical result, and so does a float64
CPU reference: a kernel's output must equal it BIT FOR BIT (bf16 storage: the round-to-nearest-even of it).  A dropped
tap, a mishandled ragged tile, a wrong pad or dilation offset, a wrong tie convention (ATen's: relu'(0) = 0, hardtanh'
= 0 at 0 and at 6, the first maximum of a pooling window wins), a truncating bf16 store or a lost last slab is a hard
failure here - under the max-relative tolerances of the other kernel tests it is noise.

The single comparison that is not bitwise is documented where it is made (nasseg_irdw_stats: 1 / sqrt(var + eps))."""
import contextlib
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as TF

import _exact as E
from test_hip_kernels import CONV_CASES, DW_CASES

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HUGE = 1 << 40
NAN = float("nan")
DTYPES = [torch.float32, torch.bfloat16]
_dt = lambda d: "fp32" if d == torch.float32 else "bf16"  # noqa: E731


def F():
    from nas_segm_amd import functional

    return functional


def dev(t, dtype=None):
    t = t.to(DEV)
    if dtype is not None:
        t = t.to(dtype)
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t


@contextlib.contextmanager
def knobs(**settings):
    """nasseg_<name>(value) for every setting, the previous values restored on the way out; the library's answers are
    memoised per argument list (a setter too), hence the cache is dropped around every change"""
    lib = F().lib
    prev = []
    try:
        for name, value in settings.items():
            lib._memo.clear()
            prev.append((name, lib.query("nasseg_" + name, value)))
            lib._memo.clear()
        yield
    finally:
        for name, value in reversed(prev):
            lib._memo.clear()
            # (nasseg_conv_pw_min_pixels reports its initial state as -2, which is also what sets it)
            lib.query("nasseg_" + name, value)
        lib._memo.clear()


def out_size(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def act64(t, act):
    return t if act == 0 else (TF.relu(t) if act == 1 else TF.hardtanh(t, 0.0, 6.0))


def mask64(t, act):
    """ATen's derivative of the activation: 0 at 0 (and at 6)"""
    if act == 0:
        return torch.ones_like(t)
    return ((t > 0) if act == 1 else ((t > 0) & (t < 6))).double()


def cv(v):
    return v.double().view(1, -1, 1, 1)


def rows_sum64(part, rows, cols):
    """float64 column sums of the first ``rows`` partial rows of a [rows + scratch][cols] buffer"""
    return part[:rows * cols].view(rows, cols).double().sum(0).cpu()


# ---------------------------------------------------------------------------------------------------------------
# a. dense conv through F.conv2d: forward, input / weight / bias gradients under every kernel selection
# ---------------------------------------------------------------------------------------------------------------
_conv_id = lambda c: "B{}K{}_{}x{}_N{}_k{}s{}p{}d{}b{}".format(*[int(v) for v in c])  # noqa: E731


def _conv_configs(case):
    """the kernel selections that can serve the case: the general MFMA kernel with one and with four reduction steps
    per round trip (maps of at most 8192 pixels), and for pointwise convs the persistent and the N-split kernels"""
    B, K, H, W, N, k, s, p, d, bias = case
    M = B * out_size(H, k, s, p, d) * out_size(W, k, s, p, d)
    base = dict(conv_pwn_mode=0, conv_pw_min_pixels=HUGE, conv_deep_k=1)
    cfgs = [base]
    if max(M, B * H * W) <= 8192:
        cfgs.append(dict(base, conv_deep_k=0))
    if k == 1 and s == 1 and p == 0:
        cfgs.append(dict(base, conv_pw_min_pixels=0))
        cfgs.append(dict(base, conv_pwn_mode=2))
    return cfgs


@functools.lru_cache(maxsize=2)
def _conv_reference(case):
    B, K, H, W, N, k, s, p, d, bias = case
    Ho, Wo = out_size(H, k, s, p, d), out_size(W, k, s, p, d)
    x, w, cot = E.ints(B, K, H, W, seed=3), E.ints(N, K, k, k, seed=4), E.ints(B, N, Ho, Wo, seed=6)
    b = E.ints(N, seed=5) if bias else None

    def op(x, w, cot, b=None):
        return (TF.conv2d(x, w, b, s, p, d), torch.nn.grad.conv2d_input(x.shape, w, cot, s, p, d),
                torch.nn.grad.conv2d_weight(x, w.shape, cot, s, p, d), cot.sum((0, 2, 3)))

    ins = [x, w, cot] + ([b] if bias else [])
    E.assert_exactly_summable(op, ins, 1.0, "dense conv")
    return x, w, b, cot, op(*[t.double() for t in ins])


@pytest.mark.parametrize("case", CONV_CASES, ids=_conv_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_dense_conv_is_exact_under_every_kernel_selection(case, dtype, monkeypatch):
    """forward and the three gradients of F.conv2d under every kernel selection that can serve the case; the weight
    gradient immediate and - under the first selection - with its stages deferred (F.deferred_wgrad) in every mode of
    functional.WGRAD_STREAM: 0 everything on the chain's stream, 1 / 2 / 3 the launches of large layers and / or the
    grouped small ones on the second stream"""
    f = F()
    B, K, H, W, N, k, s, p, d, bias = case
    Ho, Wo = out_size(H, k, s, p, d), out_size(W, k, s, p, d)
    x, w, b, cot, (y_ref, dx_ref, dw_ref, db_ref) = _conv_reference(case)
    pointwise = k == 1 and s == 1 and p == 0

    def run(deferred, what):
        if deferred is not None:
            monkeypatch.setattr(f, "WGRAD_STREAM", deferred)
        xg = dev(x, dtype).requires_grad_(True)
        wg = w.to(DEV).requires_grad_(True)
        bg = b.to(DEV).requires_grad_(True) if bias else None
        y = f.conv2d(xg, wg, bg, s, p, d)
        if deferred is not None:
            with f.deferred_wgrad(params=[wg]):
                y.backward(dev(cot, dtype))
        else:
            y.backward(dev(cot, dtype))
        E.assert_bitwise(y, y_ref, what + ": forward")
        E.assert_bitwise(xg.grad, dx_ref, what + ": input gradient")
        E.assert_bitwise(wg.grad, dw_ref, what + ": weight gradient")
        if bias:
            E.assert_bitwise(bg.grad, db_ref, what + ": bias gradient")

    for i, cfg in enumerate(_conv_configs(case)):
        with knobs(**cfg):
            if pointwise and cfg["conv_pwn_mode"] == 2 and N % 4 == 0 and K % 4 == 0 and N <= 256 and K <= 512:
                assert f.lib.query("nasseg_conv_pointwise_kernel", B, Ho, Wo, N, K, 1) == 2
            run(None, "{} immediate".format(cfg))
            if i == 0:
                for mode in (0, 1, 2, 3):
                    run(mode, "{} deferred, WGRAD_STREAM {}".format(cfg, mode))
    if f.lib.query("nasseg_conv_wgrad_lds3x3", B, H, W, K, Ho, Wo, N, k, k, s, p, d):
        # a class head: F.conv2d's weight gradient ran on the LDS-tiled kernel in both runs above (such layers are kept
        # out of the grouped launch); the generic kernel of the batched first stage, nasseg_conv_wgrad_many, is held to
        # the same bits
        xg, dyg = dev(x, dtype), dev(cot, dtype)
        ws = torch.full((f.lib.query("nasseg_conv_wgrad_workspace", B, Ho, Wo, N, K, k, k),), NAN, device=DEV)
        desc = (ctypes.c_int64 * 20)(f.ptr(xg), K, f.ptr(dyg), N, f.ptr(ws), 0, 0, 0, B, H, W, K, Ho, Wo, N, k, k, s, p, d)
        st = f.current_stream()
        f.lib.call(f._k("nasseg_conv_wgrad_many", xg), 1, desc, st)
        nslab = ws.numel() // (k * k * N * K)
        E.assert_bitwise(ws.view(nslab, -1).double().sum(0).view(k * k, N, K).permute(1, 2, 0).reshape(N, K, k, k),
                         dw_ref, "generic kernel: partial rows")
        dw = torch.full((N, K, k, k), NAN, device=DEV)
        parts, outs = (ctypes.c_void_p * 1)(f.ptr(ws)), (ctypes.c_void_p * 1)(f.ptr(dw))
        f.lib.call("nasseg_wgrad_finalize_many", 1, parts, outs, (ctypes.c_int * 5)(nslab, k * k, N, K, 0), st)
        E.assert_bitwise(dw, dw_ref, "generic kernel + nasseg_wgrad_finalize_many")


def test_every_dense_kernel_family_serves_some_case():
    """the selections of the test above reach the persistent and the N-split pointwise kernels, the LDS-tiled 3x3
    forward kernel and the LDS-tiled 3x3 weight gradient (asked of the library under the same settings)"""
    f = F()
    seen = set()
    for case in CONV_CASES:
        B, K, H, W, N, k, s, p, d, bias = case
        Ho, Wo = out_size(H, k, s, p, d), out_size(W, k, s, p, d)
        for cfg in _conv_configs(case):
            with knobs(**cfg):
                if k == 1 and s == 1 and p == 0:
                    seen.add("pointwise %d" % f.lib.query("nasseg_conv_pointwise_kernel", B, Ho, Wo, N, K, 1))
                    seen.add("pointwise bwd %d" % f.lib.query("nasseg_conv_pointwise_kernel", B, H, W, K, N, 2))
                if f.lib.query("nasseg_conv_fwd_lds3x3", B, Ho, Wo, N, K, k, k, s, p, d, 0):
                    seen.add("lds3x3 fwd")
                if f.lib.query("nasseg_conv_wgrad_lds3x3", B, H, W, K, Ho, Wo, N, k, k, s, p, d):
                    seen.add("lds3x3 wgrad")
    assert {"pointwise 0", "pointwise 1", "pointwise 2", "pointwise bwd 0", "pointwise bwd 1", "pointwise bwd 2",
            "lds3x3 fwd", "lds3x3 wgrad"} <= seen, sorted(seen)


@pytest.mark.parametrize("case", [
    # B, K, H, W, N, k, pad: maps of at most 8192 pixels - MobileNetV2's 960 -> 160 at 16 x 11 x 11, a K that is not a
    # multiple of 64 (nor of 16), a 3x3, a one-pixel map
    (16, 960, 11, 11, 160, 1, 0), (2, 232, 21, 21, 64, 1, 0), (4, 72, 13, 15, 48, 3, 1), (3, 40, 1, 1, 16, 1, 0),
    (1, 100, 90, 91, 24, 1, 0)], ids=lambda c: "B{}K{}_{}x{}_N{}_k{}p{}".format(*c))
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_deep_k_gives_the_same_bits_on_real_inputs(case, dtype):
    """include/nasseg.h promises bit-identical results for nasseg_conv_deep_k 0 and 1: held to it on randn inputs,
    forward and both gradients, with torch.equal"""
    f = F()
    B, K, H, W, N, k, p = case
    g = torch.Generator().manual_seed(7)
    x, w = torch.randn(B, K, H, W, generator=g), torch.randn(N, K, k, k, generator=g) / (K * k * k) ** 0.5
    cot = torch.randn(B, N, H, W, generator=g)
    got = []
    for deep in (0, 1):
        with knobs(conv_pwn_mode=0, conv_pw_min_pixels=HUGE, conv_deep_k=deep):
            xg, wg = dev(x, dtype).requires_grad_(True), w.to(DEV).requires_grad_(True)
            y = f.conv2d(xg, wg, None, 1, p, 1)
            y.backward(dev(cot, dtype))
            got.append((y.detach().clone(), xg.grad.clone(), wg.grad.clone()))
    for a, b_, what in zip(got[0], got[1], ("forward", "input gradient", "weight gradient")):
        assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b_), what


# ---------------------------------------------------------------------------------------------------------------
# b. depthwise conv through F.depthwise_conv2d
# ---------------------------------------------------------------------------------------------------------------
_dw_id = lambda c: "B{}C{}_{}x{}_k{}s{}p{}d{}".format(*c)  # noqa: E731
# relu_in: "plain" none; "tie" ReLU over integer inputs that hit 0 exactly (ATen: relu'(0) = 0); "notie" ReLU over
# integers + 1/2.  (The networks use relu_in with DilConv, k 3 / 5, only; the wrapper takes it for any kernel size)
DW_VARIANTS = [(c, v) for c in DW_CASES for v in ("plain", "tie", "notie")]


@pytest.mark.parametrize("case,variant", DW_VARIANTS, ids=lambda v: v if isinstance(v, str) else _dw_id(v))
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_depthwise_conv_is_exact(case, variant, dtype):
    f = F()
    B, C, H, W, K, s, p, d = case
    relu_in = variant != "plain"
    x = E.halves(B, C, H, W, seed=1) if variant == "notie" else E.ints(B, C, H, W, seed=1)
    w = E.ints(C, 1, K, K, seed=2)
    cot = E.ints(B, C, out_size(H, K, s, p, d), out_size(W, K, s, p, d), seed=3)
    if variant == "tie":
        assert int((x == 0).sum()) > x.numel() // 10

    def op(x, w, cot):
        return (TF.conv2d(x, w, None, s, p, d, C), torch.nn.grad.conv2d_input(x.shape, w, cot, s, p, d, C),
                torch.nn.grad.conv2d_weight(x, w.shape, cot, s, p, d, C))

    E.assert_exactly_summable(op, [x, w, cot], 0.5, "depthwise conv")
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y_ref = TF.conv2d(TF.relu(xr) if relu_in else xr, wr, None, s, p, d, C)
    y_ref.backward(cot.double())
    settings = [dict(dw_wgrad_lds=0), dict(dw_wgrad_lds=1)] if (K == 5 and s == 1) else [dict()]
    for cfg in settings:
        with knobs(**cfg):
            xg, wg = dev(x, dtype).requires_grad_(True), w.to(DEV).requires_grad_(True)
            y = f.depthwise_conv2d(xg, wg, s, p, d, relu_in=relu_in)
            y.backward(dev(cot, dtype))
            E.assert_bitwise(y, y_ref, "{}: forward".format(cfg))
            E.assert_bitwise(xg.grad, xr.grad, "{}: input gradient".format(cfg))
            E.assert_bitwise(wg.grad, wr.grad, "{}: weight gradient".format(cfg))


# ---------------------------------------------------------------------------------------------------------------
# c. nasseg_conv_fwd / nasseg_bf16_conv_fwd through the C ABI: prologue, epilogue, residual, channel slices,
#    statistics rows - per kernel family
# ---------------------------------------------------------------------------------------------------------------
GENERAL = dict(conv_pwn_mode=0, conv_pw_min_pixels=HUGE)
PERSISTENT = dict(conv_pwn_mode=0, conv_pw_min_pixels=0)
NSPLIT = dict(conv_pwn_mode=2)
FWD_CASES = [
    # family, knobs, (B, K, H, W, N, k, stride, pad, dil): per family a ragged map (pixels not a multiple of 64) and
    # a minimal one
    ("general", GENERAL, (2, 24, 13, 17, 40, 1, 1, 0, 1)), ("general", GENERAL, (3, 16, 1, 1, 32, 1, 1, 0, 1)),
    ("general", GENERAL, (2, 16, 7, 9, 24, 3, 1, 1, 1)), ("general", GENERAL, (1, 8, 13, 17, 16, 3, 2, 1, 1)),
    ("general", GENERAL, (1, 20, 5, 5, 10, 1, 1, 0, 1)),
    ("persistent", PERSISTENT, (1, 24, 13, 17, 48, 1, 1, 0, 1)), ("persistent", PERSISTENT, (2, 16, 1, 1, 32, 1, 1, 0, 1)),
    ("persistent", PERSISTENT, (1, 144, 45, 49, 24, 1, 1, 0, 1)),
    ("nsplit", NSPLIT, (1, 24, 13, 17, 48, 1, 1, 0, 1)), ("nsplit", NSPLIT, (1, 16, 1, 1, 16, 1, 1, 0, 1)),
    ("nsplit", NSPLIT, (2, 32, 50, 60, 80, 1, 1, 0, 1)),
    ("lds3x3", GENERAL, (2, 32, 9, 33, 48, 3, 1, 2, 2)), ("lds3x3", GENERAL, (1, 16, 17, 45, 20, 3, 1, 1, 1)),
    ("lds3x3", GENERAL, (1, 32, 14, 40, 64, 3, 1, 3, 3)), ("lds3x3", GENERAL, (2, 64, 20, 70, 19, 3, 1, 1, 1)),
    ("lds3x3", GENERAL, (1, 16, 8, 32, 16, 3, 1, 1, 1)), ("lds3x3", GENERAL, (1, 24, 10, 35, 13, 3, 1, 0, 1)),
    ("flat", GENERAL, (2, 3, 33, 37, 32, 3, 2, 1, 1)), ("flat", GENERAL, (1, 3, 1, 1, 8, 3, 2, 1, 1)),
]
# variant: what the call carries besides the conv
FWD_VARIANTS = ["plain_stats", "pro1_tie", "pro1_notie", "pro2_tie", "pro2_notie", "pro0", "epi0", "epi1_tie",
                "epi1_notie", "epi2_tie", "epi2_notie", "slices4", "slices_odd"]


def _stats_rows(f, B, Ho, Wo, N, K, k, s, p, d):
    if k == 1 and s == 1 and p == 0:
        return f.lib.query("nasseg_conv_fwd_stats_blocks", B, Ho, Wo, N, K, 1)
    return f.lib.query("nasseg_conv_fwd_stats_rows", B, Ho, Wo, N, K, k, k, s, p, d)


def _slab(t, ld, off, dtype):
    """device slab [B][H][W][ld] of NaN with the NCHW tensor ``t`` in channels [off, off + C)"""
    B, C, H, W = t.shape
    sl = torch.full((B, H, W, ld), NAN, device=DEV, dtype=dtype)
    sl[..., off:off + C] = t.permute(0, 2, 3, 1).to(DEV).to(dtype)
    return sl


def _slice_ptr(sl, off):
    return sl.data_ptr() + off * sl.element_size()


def _check_slab(sl, off, C, ref, what):
    """channels [off, off + C) of the slab equal ``ref`` (NCHW, float64) bit for bit, every other channel still NaN"""
    E.assert_bitwise(sl[..., off:off + C].permute(0, 3, 1, 2), ref, what)
    rest = torch.cat([sl[..., :off], sl[..., off + C:]], -1)
    assert bool(torch.isnan(rest.float()).all()), what + ": channels outside the slice were written"


def _serves_prologue(geom):
    B, K, H, W, N, k, s, p, d = geom
    return k == 1 and s == 1 and p == 0 and K % 4 == 0 and N % 4 == 0


# (a prologue is served on pointwise calls with K % 4 == 0 and N % 4 == 0 only: elsewhere ONE call asserts the refusal)
FWD_PARAMS = [pytest.param(fam, cfg, geom, v, id="{}-B{}K{}_{}x{}_N{}_k{}s{}p{}d{}-{}".format(fam, *geom, v))
              for fam, cfg, geom in FWD_CASES for v in FWD_VARIANTS
              if not v.startswith("pro") or _serves_prologue(geom) or v == "pro1_tie"]


@pytest.mark.parametrize("family,cfg,geom,variant", FWD_PARAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_conv_fwd_abi_is_exact(family, cfg, geom, variant, dtype):
    """y = out_act(out_scale * conv(in_act(in_scale * x + in_shift)) + out_shift) + res through the C ABI.  Scales are
    +-1 | +-2, shifts integers (tie: pre-activations hit 0 and 6 exactly) or integers + 1/2 (no tie); the forward
    clamps are exact either way.  Statistics rows: their float64 column sums equal the sums of z and z^2 exactly."""
    f = F()
    B, K, H, W, N, k, s, p, d = geom
    Ho, Wo = out_size(H, k, s, p, d), out_size(W, k, s, p, d)
    pro = variant.startswith("pro")
    if pro and not _serves_prologue(geom):
        variant = "refused_" + variant
    tie = not variant.endswith("notie")
    stats = variant == "plain_stats" and N % 4 == 0
    sparse = dict(lo=-1, hi=1, density=0.5) if stats else {}
    x, w = E.ints(B, K, H, W, seed=1, **sparse), E.ints(N, K, k, k, seed=2, **sparse)
    isc = ish = osc = osh = res = None
    iact = oact = 0
    if pro:
        iact = int(variant.split("pro")[1][0])
        isc, ish = E.pow2(K, 0, 1, seed=3), E.ints(K, lo=-2, hi=4, seed=4, offset=0.0 if tie else 0.5)
    if variant.startswith("epi"):
        oact = int(variant[3])
        osc, osh = E.pow2(N, 0, 1, seed=5), E.ints(N, lo=-2, hi=4, seed=6, offset=0.0 if tie else 0.5)
        res = E.ints(B, N, Ho, Wo, seed=7)
    ldx, xoff, ldy, yoff, ldres, roff = K, 0, N, 0, N + 8, 4
    if variant == "slices4":      # multiples of 4: the vector paths (bf16: the output slice sits at 8 bytes, not at 16)
        ldx, xoff, ldy, yoff = K + 12, 8, N + 8, 4
    elif variant == "slices_odd":  # strides that are no multiples of 4: the scalar paths, slices at odd offsets
        ldx, xoff, ldy, yoff = K + 6, 3, N + 5, 1

    def op(x, w, ish=None, osh=None, res=None):
        xi = x * 2 + ish.view(1, -1, 1, 1) if ish is not None else x
        z = TF.conv2d(xi, w, None, s, p, d)
        z = z * 2 + osh.view(1, -1, 1, 1) if osh is not None else z
        return z + res if res is not None else z

    E.assert_exactly_summable(lambda x, w: op(x, w, None if ish is None else ish.double().abs(),
                                              None if osh is None else osh.double().abs(),
                                              None if res is None else res.double().abs()), [x, w], 0.5, "conv_fwd")
    def tied(pre, act):
        """the 'tie' label holds: a pre-activation sits exactly on every bound of the activation (maps of a few
        pixels cannot be made to: they are left as they come)"""
        if tie and act and pre.numel() >= 512:
            assert bool((pre == 0).any()) and (act == 1 or bool((pre == 6).any()))
        if not tie and act:
            assert not bool(((pre == 0) | (pre == 6)).any())

    xi = x.double()
    if pro:
        tied(xi * cv(isc) + cv(ish), iact)
        xi = act64(xi * cv(isc) + cv(ish), iact)
    z_ref = TF.conv2d(xi, w.double(), None, s, p, d)
    y_ref = z_ref
    if osc is not None:
        pre = z_ref * cv(osc) + cv(osh)
        tied(pre, oact)
        y_ref = act64(pre, oact) + res.double()
    if stats:
        E.assert_stats_summable(z_ref, 1.0, "statistics of z")
    xs, ys = _slab(x, ldx, xoff, dtype), torch.full((B, Ho, Wo, ldy), NAN, device=DEV, dtype=dtype)
    rs = _slab(res, ldres, roff, dtype) if res is not None else None
    wd = w.to(DEV)
    st = f.current_stream()
    with knobs(**cfg):
        if family == "persistent":
            assert f.lib.query("nasseg_conv_pointwise_kernel", B, Ho, Wo, N, K, 1) == 1
        if family == "nsplit":
            assert f.lib.query("nasseg_conv_pointwise_kernel", B, Ho, Wo, N, K, 1) == 2
        if family == "lds3x3":
            assert f.lib.query("nasseg_conv_fwd_lds3x3", B, Ho, Wo, N, K, k, k, s, p, d, int(stats)) == 1
        if family == "flat":
            assert f.lib.query("nasseg_conv_fwd_pack_mode", K, k, k) == 2
        wp = f._pack_dense(wd, "fwd")
        part, rows = None, 0
        if stats:
            rows = _stats_rows(f, B, Ho, Wo, N, K, k, s, p, d)
            assert rows > 0
            part = torch.full(((rows + 64) * 2 * N,), NAN, device=DEV)
        vd = [None if v is None else v.to(DEV) for v in (isc, ish, osc, osh)]  # (kept alive across the call)

        def args(ys, ldy, yoff):
            return (_slice_ptr(xs, xoff), ldx, f.ptr(wp), _slice_ptr(ys, yoff), ldy, f.ptr(vd[0]), f.ptr(vd[1]), iact,
                    f.ptr(vd[2]), f.ptr(vd[3]), oact, _slice_ptr(rs, roff) if rs is not None else None,
                    ldres if rs is not None else 0, B, H, W, K, Ho, Wo, N, k, k, s, p, d, 0, f.ptr(part), st)

        if variant.startswith("refused"):
            with pytest.raises(RuntimeError):
                f.lib.call(f._k("nasseg_conv_fwd", xs), *args(ys, ldy, yoff))
            return
        if variant == "slices_odd" and N > 32 and family != "lds3x3":
            # outside the LDS-tiled kernel the scalar-store path serves N <= 32: the call is refused, and the output
            # goes to a stride of 4 k
            with pytest.raises(RuntimeError):
                f.lib.call(f._k("nasseg_conv_fwd", xs), *args(ys, ldy, yoff))
            assert bool(torch.isnan(ys.float()).all())
            ldy, yoff = N + 8, 4
            ys = torch.full((B, Ho, Wo, ldy), NAN, device=DEV, dtype=dtype)
        f.lib.call(f._k("nasseg_conv_fwd", xs), *args(ys, ldy, yoff))
        torch.cuda.synchronize()
    _check_slab(ys, yoff, N, y_ref, variant)
    if stats:
        zd = z_ref.permute(1, 0, 2, 3).reshape(N, -1)
        got = rows_sum64(part, rows, 2 * N)
        E.assert_bitwise(got[:N], zd.sum(1), "statistics rows: sum z")
        E.assert_bitwise(got[N:], (zd * zd).sum(1), "statistics rows: sum z^2")


# ---------------------------------------------------------------------------------------------------------------
# e. simple ops through the wrappers
# ---------------------------------------------------------------------------------------------------------------
def _three_valued(*shape, seed):
    """values from three distinct integers: every 3x3 window holds equal maxima"""
    return torch.tensor([-2.0, 1.0, 3.0])[torch.randint(0, 3, shape, generator=torch.Generator().manual_seed(seed))]


@pytest.mark.parametrize("shape", [(2, 8, 13, 17), (1, 48, 16, 16), (2, 16, 7, 9), (1, 4, 1, 1), (1, 4, 2, 3),
                                   (2, 32, 33, 64)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_max_pooling_routes_ties_to_the_first_maximum(shape, stride, dtype):
    """F.max_pool2d over maps on which every window ties: the forward is exact, the backward sends a window's gradient
    to its FIRST maximum in row-major window order, as torch's CPU kernel does"""
    f = F()
    x = _three_valued(*shape, seed=1)
    xr = x.double().requires_grad_(True)
    y_ref = TF.max_pool2d(xr, 3, stride, 1)
    cot = E.ints(*y_ref.shape, seed=2)
    E.assert_exactly_summable(lambda c: TF.conv_transpose2d(c, torch.ones(shape[1], 1, 3, 3).double(), None, stride, 1,
                                                            groups=shape[1]), [cot], 1.0, "pool backward")
    y_ref.backward(cot.double())
    for strip in ((0, 1) if stride == 1 else (1,)):
        with knobs(pool_strip=strip):
            xg = dev(x, dtype).requires_grad_(True)
            y = f.max_pool2d(xg, 3, stride, 1)
            y.backward(dev(cot, dtype))
            E.assert_bitwise(y, y_ref, "strip {}: forward".format(strip))
            E.assert_bitwise(xg.grad, xr.grad, "strip {}: gradient".format(strip))


@pytest.mark.parametrize("shape", [(2, 32, 33, 64), (1, 24, 7, 5), (3, 64, 16, 19), (2, 8, 1, 9), (1, 144, 9, 1),
                                   (1, 4, 1, 1)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_max_pooling_with_batchnorm_on_load_is_exact(shape, stride, dtype):
    """nasseg_maxpool_bn_fwd / _bwd: y = maxpool3x3(scale * z + shift) with scale +- a power of two (a negative scale
    turns the window's minima into its maxima - still the first one wins), the gradient w.r.t. the BatchNorm's output
    and the float64 sums of the rows {sum g, sum g * xhat}, strip kernels and tap gather"""
    f = F()
    B, C, H, W = shape
    Ho, Wo = out_size(H, 3, stride, 1, 1), out_size(W, 3, stride, 1, 1)
    z = _three_valued(*shape, seed=1)
    scale, shift = E.pow2(C, -1, 1, seed=2), E.ints(C, lo=-2, hi=2, seed=3)
    mean, invstd = E.ints(C, lo=-1, hi=1, seed=4), E.pow2(C, -1, 1, seed=5, signed=False)
    dy = E.ints(B, C, Ho, Wo, seed=6)
    u = (z.double() * cv(scale) + cv(shift)).requires_grad_(True)
    y_ref = TF.max_pool2d(u, 3, stride, 1)
    y_ref.backward(dy.double())
    g_ref = u.grad
    xhat = (z.double() - cv(mean)) * cv(invstd)
    E.assert_exactly_summable(lambda g, xh: ((g * xh).sum((0, 2, 3)), g.sum((0, 2, 3))), [g_ref, xhat], 0.25, "rows")
    pre = "nasseg_" if dtype == torch.float32 else "nasseg_bf16_"
    st = f.current_stream()
    zd, dyd = dev(z, dtype), dev(dy, dtype)
    vec = [v.to(DEV) for v in (scale, shift, mean, invstd)]
    for strip in ((0, 1, 2) if stride == 1 else (1,)):
        with knobs(pool_strip=strip):
            y = dev(torch.full((B, C, Ho, Wo), NAN), dtype)
            idx = torch.full((B, Ho, Wo, C), 255, device=DEV, dtype=torch.uint8)
            f.lib.call(pre + "maxpool_bn_fwd", f.ptr(zd), f.ptr(vec[0]), f.ptr(vec[1]), f.ptr(y), f.ptr(idx), B, H, W, C,
                       Ho, Wo, stride, 1, st)
            nb = f.lib.query("nasseg_maxpool_bn_bwd_blocks", B, H, W, C, 3, stride, 1)
            assert nb > 0
            part = torch.full(((nb + 64) * 2 * C,), NAN, device=DEV)
            g = dev(torch.full(shape, NAN), dtype)
            f.lib.call(pre + "maxpool_bn_bwd", f.ptr(dyd), f.ptr(idx), f.ptr(zd), f.ptr(vec[2]), f.ptr(vec[3]), f.ptr(g),
                       f.ptr(part), B, H, W, C, Ho, Wo, stride, 1, st)
            torch.cuda.synchronize()
            what = "strip {}: ".format(strip)
            E.assert_bitwise(y, y_ref, what + "forward")
            E.assert_bitwise(g, g_ref, what + "gradient")
            got = rows_sum64(part, nb, 2 * C)
            E.assert_bitwise(got[:C], g_ref.sum((0, 2, 3)), what + "rows: sum g")
            E.assert_bitwise(got[C:], (g_ref * xhat).sum((0, 2, 3)), what + "rows: sum g * xhat")


RESIZE_EXACT = [((5, 7), (10, 14)), ((4, 5), (16, 20)), ((4, 5), (32, 40)), ((12, 16), (6, 8)), ((1, 1), (8, 8)),
                ((3, 9), (24, 18))]


def _interp64(t, size):
    return TF.interpolate(t, size=size, mode="bilinear", align_corners=False)


@pytest.mark.parametrize("sizes", RESIZE_EXACT, ids=lambda s: "{}x{}_to_{}x{}".format(*s[0], *s[1]))
@pytest.mark.parametrize("C", [8, 19])
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_bilinear_resize_is_exact_at_power_of_two_factors(sizes, C, dtype):
    """factors 2, 4, 8 up and 1/2 down: the weights are multiples of 1/16 per axis, the inputs multiples of 64, so
    every product is a multiple of 1/4 far below 2^24 of them; forward and backward (the x8 case takes the separable
    backward kernel, the others the direct one)"""
    f = F()
    (hi, wi), (ho, wo) = sizes
    x = E.ints(2, C, hi, wi, lo=-4, hi=4, unit=64.0, seed=1)
    cot = E.ints(2, C, ho, wo, lo=-4, hi=4, unit=64.0, seed=2)
    xr = x.double().requires_grad_(True)
    y_ref = _interp64(xr, (ho, wo))
    y_ref.backward(cot.double())
    E.assert_exactly_summable(lambda a: (_interp64(a, (ho, wo)),), [x], 0.25, "resize")
    E.assert_exactly_summable(lambda c: (torch.autograd.grad(_interp64(xr, (ho, wo)), xr, c)[0],), [cot], 0.25, "resize bwd")
    separable = f.lib.query("nasseg_bilinear_bwd_workspace", 2, hi, wi, C, ho, wo) > 0
    if ho <= 2 * hi:
        assert not separable  # (the single-pass gather)
    if sizes == ((4, 5), (32, 40)) and C == 8:
        assert separable  # (x8: the two-pass form)
    xg = dev(x, dtype).requires_grad_(True)
    y = f.bilinear_resize(xg, (ho, wo))
    y.backward(dev(cot, dtype))
    E.assert_bitwise(y, y_ref, "forward")
    E.assert_bitwise(xg.grad, xr.grad, "gradient")


@pytest.mark.parametrize("sizes", [((7, 9), (14, 18)), ((4, 5), (32, 40)), ((26, 34), (13, 17))],
                         ids=lambda s: "{}x{}_to_{}x{}".format(*s[0], *s[1]))
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_concat_resize_is_exact(sizes, relu, dtype):
    """F.concat_resize: a same-size input, a resized one and another same-size one into one slab, with the fused ReLU
    over values that hit 0 exactly (relu'(0) = 0)"""
    f = F()
    (hi, wi), (ho, wo) = sizes
    a = E.ints(2, 8, ho, wo, lo=-2, hi=2, unit=64.0, seed=1)
    b = E.ints(2, 12, hi, wi, lo=-2, hi=2, unit=64.0, seed=2)
    c = E.ints(2, 4, ho, wo, lo=-2, hi=2, unit=64.0, seed=3)
    cot = E.ints(2, 24, ho, wo, lo=-4, hi=4, unit=64.0, seed=4)
    ins = [t.double().requires_grad_(True) for t in (a, b, c)]
    y_ref = torch.cat([ins[0], _interp64(ins[1], (ho, wo)), ins[2]], 1)
    if relu:
        assert int((y_ref == 0).sum()) > y_ref.numel() // 20
        y_ref = TF.relu(y_ref)
    y_ref.backward(cot.double())
    E.assert_exactly_summable(lambda t: (torch.autograd.grad(_interp64(ins[1], (ho, wo)), ins[1], t[:, 8:20])[0],),
                              [cot], 0.25, "concat_resize bwd")
    gs = [dev(t, dtype).requires_grad_(True) for t in (a, b, c)]
    y = f.concat_resize(gs, (ho, wo), relu=relu)
    y.backward(dev(cot, dtype))
    E.assert_bitwise(y, y_ref, "forward")
    for g, r, what in zip(gs, ins, "abc"):
        E.assert_bitwise(g.grad, r.grad, "gradient of " + what)


# ---------------------------------------------------------------------------------------------------------------
# d. kernels that apply a BatchNorm backward on load or rebuild a tensor.  The reference is the formula of
#    include/nasseg.h, once, in float64:  g' = g * act'(scale * z + shift)  (bn_act != 0),
#    dz = scale * (g' - sums0 / M - xhat * sums1 / M)  (bn_train; else scale * g'),  xhat = (z - mean) * invstd.
#    Vectors from _exact.bn_vectors: every value a multiple of 1/2 or 1/4 with a handful of bits.  Where bn_train is
#    set the pixel count M is a power of two: a kernel may multiply by 1 / M, which is exact only then (sums are
#    integer multiples of M); the ragged maps (13 x 17 and the like) run with bn_train = 0.
# ---------------------------------------------------------------------------------------------------------------
# bn_act, tie (pre-activations hit 0 / 6 exactly: ATen's derivative there is 0) or no tie
ACT_TIE = [(0, True), (1, True), (1, False), (2, True), (2, False)]


def bn_bwd64(g, z, vec, sums, M, train, act):
    """(g', dz) of the header's formula in float64; vec = (scale, shift, mean, invstd), sums [2][C]"""
    scale, shift, mean, invstd = [cv(v) for v in vec]
    C = z.shape[1]
    gp = g.double() * mask64(z.double() * scale + shift, act)
    if not train:
        return gp, scale * gp
    xhat = (z.double() - mean) * invstd
    return gp, scale * (gp - cv(sums[:C]) / M - xhat * cv(sums[C:]) / M)


def xhat64(z, vec):
    return (z.double() - cv(vec[2])) * cv(vec[3])


def _bn_sums64(g, z, vec):
    """{sum g, sum g * xhat} per channel, and the bound of their terms"""
    xh = xhat64(z, vec)
    E.assert_exactly_summable(lambda a, b, m, i: ((a * (b + m.view(1, -1, 1, 1)) * i.view(1, -1, 1, 1)).sum((0, 2, 3)),
                                                  a.sum((0, 2, 3))), [g, z, vec[2], vec[3]], 0.125, "BatchNorm-backward rows")
    return torch.cat([g.sum((0, 2, 3)), (g * xh).sum((0, 2, 3))])


def _to_dev(vec):
    return [v.to(DEV) for v in vec]


def _pow2_pixels(train, B, H, W):
    if train:
        M = B * H * W
        assert M & (M - 1) == 0, "bn_train needs a power-of-two pixel count here"


BWD_DATA_GEOMS = [
    # B, H, W of g / z, K channels of g, N channels of dy, k, stride, pad, dil
    (2, 4, 8, 24, 64, 1, 1, 0, 1), (2, 13, 17, 24, 64, 1, 1, 0, 1), (1, 1, 1, 16, 32, 1, 1, 0, 1),
    (2, 12, 10, 64, 19, 3, 1, 1, 1), (2, 15, 13, 32, 48, 3, 2, 1, 1), (1, 45, 49, 144, 24, 1, 1, 0, 1),
    (1, 9, 11, 224, 64, 1, 1, 0, 1)]
# (the persistent and the N-split kernels serve pointwise calls only)
BWD_DATA_PARAMS = [pytest.param(g, sel, id="B{}_{}x{}_K{}N{}_k{}s{}p{}d{}-{}".format(*g, sel)) for g in BWD_DATA_GEOMS
                   for sel in ("general", "persistent", "nsplit") if sel == "general" or g[5:8] == (1, 1, 0)]


@pytest.mark.parametrize("geom,sel", BWD_DATA_PARAMS)
@pytest.mark.parametrize("act,tie", ACT_TIE)
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_dense_backward_data_with_bn_mask_is_exact(geom, sel, act, tie, dtype):
    """nasseg_conv_bwd_data_bn: g = act'(scale * z + shift) * conv_backward_data(dy) and the rows {sum g, sum g xhat}"""
    f = F()
    B, H, W, K, N, k, s, p, d = geom
    pointwise = k == 1 and s == 1 and p == 0
    Ho, Wo = out_size(H, k, s, p, d), out_size(W, k, s, p, d)
    w, dy = E.ints(N, K, k, k, seed=1, lo=-2, hi=2), E.ints(B, N, Ho, Wo, seed=2, lo=-2, hi=2, density=0.5)
    z = E.ints(B, K, H, W, seed=3)
    vec = E.bn_vectors(K, 4, tie=tie)
    E.assert_exactly_summable(lambda a, b: torch.nn.grad.conv2d_input((B, K, H, W), a, b, s, p, d), [w, dy], 1.0, "dx")
    pre = z.double() * cv(vec[0]) + cv(vec[1])
    if tie and act:
        assert bool((pre == 0).any()) and (act == 1 or bool((pre == 6).any()))
    g_ref = torch.nn.grad.conv2d_input((B, K, H, W), w.double(), dy.double(), s, p, d) * mask64(pre, act)
    sums_ref = _bn_sums64(g_ref, z.double(), vec)
    cfg = dict(general=GENERAL, persistent=PERSISTENT, nsplit=NSPLIT)[sel]
    st = f.current_stream()
    with knobs(**cfg):
        wp = f._pack_dense(w.to(DEV), 1)
        dyd, zd, vd = dev(dy, dtype), dev(z, dtype), _to_dev(vec)
        if sel == "nsplit":
            assert f.lib.query("nasseg_conv_pointwise_kernel", B, H, W, K, N, 2) == 2
        nb = f.lib.query("nasseg_conv_fwd_stats_blocks", B, H, W, K, N, 2 * int(pointwise))
        part = torch.full(((nb + 64) * 2 * K,), NAN, device=DEV)
        g = dev(torch.full((B, K, H, W), NAN), dtype)
        f.lib.call(f._k("nasseg_conv_bwd_data_bn", dyd), f.ptr(dyd), N, f.ptr(wp), f.ptr(g), K, f.ptr(zd), K, f.ptr(vd[0]),
                   f.ptr(vd[1]), f.ptr(vd[2]), f.ptr(vd[3]), act, B, Ho, Wo, N, H, W, K, k, k, s, p, d, f.ptr(part), st)
        torch.cuda.synchronize()
    E.assert_bitwise(g, g_ref, "masked input gradient")
    E.assert_bitwise(rows_sum64(part, nb, 2 * K), sums_ref, "rows {sum g, sum g * xhat}")


@pytest.mark.parametrize("case", [
    # B, C, H, W (of the conv input = g / z), K, stride, pad, dil
    (2, 24, 13, 17, 3, 1, 1, 1), (2, 32, 16, 20, 5, 1, 2, 1), (2, 16, 21, 19, 3, 1, 3, 3), (2, 32, 30, 33, 5, 1, 12, 6),
    (2, 24, 17, 23, 3, 2, 1, 1), (2, 16, 18, 22, 5, 2, 2, 1), (1, 8, 1, 1, 3, 1, 1, 1), (1, 16, 14, 97, 5, 1, 6, 3)],
    ids=_dw_id)
@pytest.mark.parametrize("act,tie", ACT_TIE)
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_depthwise_backward_data_with_bn_mask_is_exact(case, act, tie, dtype):
    """nasseg_dwconv_bwd_data_bn (through the wrapper the chains use): the masked gradient and its rows"""
    f = F()
    B, C, H, W, K, s, p, d = case
    Ho, Wo = out_size(H, K, s, p, d), out_size(W, K, s, p, d)
    w, dy, z = E.ints(C, 1, K, K, seed=1), E.ints(B, C, Ho, Wo, seed=2), E.ints(B, C, H, W, seed=3)
    vec = E.bn_vectors(C, 5, tie=tie)
    E.assert_exactly_summable(lambda a, b: torch.nn.grad.conv2d_input((B, C, H, W), a, b, s, p, d, C), [w, dy], 1.0, "dx")
    pre = z.double() * cv(vec[0]) + cv(vec[1])
    g_ref = torch.nn.grad.conv2d_input((B, C, H, W), w.double(), dy.double(), s, p, d, C) * mask64(pre, act)
    sums_ref = _bn_sums64(g_ref, z.double(), vec)
    dyd, zd, vd = dev(dy, dtype), dev(z, dtype), _to_dev(vec)
    flip = s == 1 and d * (K - 1) - p >= 0
    (wt,) = f._pack_many(dyd, [(w.to(DEV), "dwflip" if flip else "dw")])
    g, pre_rows = f._dw_backward_data(dyd, wt, K, (B, C, H, W), s, p, d, (zd, vd[0], vd[1], vd[2], vd[3], act))
    assert pre_rows is not None
    torch.cuda.synchronize()
    E.assert_bitwise(g, g_ref, "masked input gradient")
    E.assert_bitwise(rows_sum64(pre_rows[0], pre_rows[1], 2 * C), sums_ref, "rows {sum g, sum g * xhat}")


def _prologue(K, pro, tie, seed):
    """(in_scale, in_shift, in_act) of an input prologue: pro 0 none, 1 affine + ReLU, 2 affine + ReLU6"""
    if not pro:
        return None, None, 0
    return E.pow2(K, 0, 1, seed=seed), E.ints(K, lo=-2, hi=4, seed=seed + 1, offset=0.0 if tie else 0.5), pro


def _pro64(x, isc, ish, iact):
    return x.double() if isc is None else act64(x.double() * cv(isc) + cv(ish), iact)


@pytest.mark.parametrize("geom", [
    # train, (B, H, W, K, N), prologue
    (1, (2, 4, 8, 16, 96), 0), (1, (1, 2, 16, 96, 16), 2), (1, (4, 16, 16, 24, 144), 1), (0, (1, 13, 17, 144, 24), 2),
    (0, (3, 33, 31, 32, 32), 0), (0, (1, 1, 1, 16, 16), 1), (1, (1, 1, 1, 8, 12), 0)],
    ids=lambda g: "B{}_{}x{}_K{}N{}_pro{}".format(*g[1], g[2]))
@pytest.mark.parametrize("act,tie", ACT_TIE)
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_dense_weight_gradient_with_bn_backward_is_exact(geom, act, tie, dtype):
    """nasseg_conv_wgrad_bn: dz (written) and dw from dz, partial rows (dw == NULL) summed in float64"""
    f = F()
    train, (B, H, W, K, N), pro = geom
    _pow2_pixels(train, B, H, W)
    M = B * H * W
    x, g, z = E.ints(B, K, H, W, seed=1), E.ints(B, N, H, W, seed=2), E.ints(B, N, H, W, seed=3)
    vec = E.bn_vectors(N, 4, tie=tie, M=M)
    isc, ish, iact = _prologue(K, pro, tie, 9)
    xi = _pro64(x, isc, ish, iact)
    _, dz_ref = bn_bwd64(g, z, vec[:4], vec[4].double(), M, train, act)
    E.assert_exactly_summable(lambda a, b: torch.nn.grad.conv2d_weight(a, (N, K, 1, 1), b), [xi, dz_ref], 0.125, "dw")
    dw_ref = torch.nn.grad.conv2d_weight(xi, (N, K, 1, 1), dz_ref)
    xd, gd, zd, vd = dev(x, dtype), dev(g, dtype), dev(z, dtype), _to_dev(vec)
    pd = [None if v is None else v.to(DEV) for v in (isc, ish)]
    st = f.current_stream()
    nws = f.lib.query("nasseg_conv_wgrad_workspace", B, H, W, N, K, 1, 1)
    for final in (True, False):
        dz = torch.full_like(zd, NAN)
        dw = torch.full((N, K, 1, 1), NAN, device=DEV)
        ws = torch.full((nws,), NAN, device=DEV)
        f.lib.call(f._k("nasseg_conv_wgrad_bn", xd), f.ptr(xd), K, f.ptr(gd), N, f.ptr(zd), N, f.ptr(dz), N,
                   f.ptr(dw) if final else None, f.ptr(ws), f.ptr(pd[0]), f.ptr(pd[1]), iact, f.ptr(vd[0]), f.ptr(vd[1]),
                   f.ptr(vd[2]), f.ptr(vd[3]), f.ptr(vd[4]), train, act, B, H, W, K, N, st)
        torch.cuda.synchronize()
        E.assert_bitwise(dz, dz_ref, "dz")
        if final:
            E.assert_bitwise(dw, dw_ref, "dw")
        else:
            E.assert_bitwise(ws.view(-1, N * K).double().sum(0).view(N, K, 1, 1), dw_ref, "partial rows of dw")


@pytest.mark.parametrize("geom", [
    # train, (B, H, W, K, N, k, stride, pad, dil): the stem (K = 3, stride 2) and its kin, M a power of two with train
    (1, (2, 31, 63, 3, 32, 3, 2, 1, 1)), (0, (2, 33, 41, 3, 32, 3, 2, 1, 1)), (1, (1, 8, 16, 4, 16, 3, 1, 1, 1)),
    (0, (1, 1, 1, 3, 8, 3, 2, 1, 1)), (0, (2, 21, 30, 3, 24, 3, 2, 1, 1))],
    ids=lambda g: "B{}_{}x{}_K{}N{}_k{}s{}p{}d{}".format(*g[1]))
@pytest.mark.parametrize("act,tie", ACT_TIE)
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_stem_weight_gradient_with_bn_backward_is_exact(geom, act, tie, dtype):
    """nasseg_conv_wgrad_bn_flat: the BatchNorm backward applied to g on load, dz never written"""
    f = F()
    train, (B, H, W, K, N, k, s, p, d) = geom
    Ho, Wo = out_size(H, k, s, p, d), out_size(W, k, s, p, d)
    _pow2_pixels(train, B, Ho, Wo)
    M = B * Ho * Wo
    assert f.lib.query("nasseg_conv_fwd_pack_mode", K, k, k) == 2
    x, g, z = E.ints(B, K, H, W, seed=1), E.ints(B, N, Ho, Wo, seed=2), E.ints(B, N, Ho, Wo, seed=3)
    vec = E.bn_vectors(N, 4, tie=tie, M=M)
    _, dz_ref = bn_bwd64(g, z, vec[:4], vec[4].double(), M, train, act)
    E.assert_exactly_summable(lambda a, b: torch.nn.grad.conv2d_weight(a, (N, K, k, k), b, s, p, d), [x, dz_ref], 0.125, "dw")
    dw_ref = torch.nn.grad.conv2d_weight(x.double(), (N, K, k, k), dz_ref, s, p, d)
    xd, gd, zd, vd = dev(x, dtype), dev(g, dtype), dev(z, dtype), _to_dev(vec)
    st = f.current_stream()
    nws = f.lib.query("nasseg_conv_wgrad_workspace", B, Ho, Wo, N, K, k, k)
    dw, ws = torch.full((N, K, k, k), NAN, device=DEV), torch.full((nws,), NAN, device=DEV)
    f.lib.call(f._k("nasseg_conv_wgrad_bn_flat", xd), f.ptr(xd), K, f.ptr(gd), N, f.ptr(zd), N, f.ptr(dw), f.ptr(ws),
               f.ptr(vd[0]), f.ptr(vd[1]), f.ptr(vd[2]), f.ptr(vd[3]), f.ptr(vd[4]), train, act, B, H, W, K, Ho, Wo, N,
               k, k, s, p, d, st)
    torch.cuda.synchronize()
    E.assert_bitwise(dw, dw_ref, "dw")


@pytest.mark.parametrize("geom", [
    # train, (B, C, H, W, k, stride, pad, dil), prologue
    (1, (2, 24, 4, 8, 3, 1, 1, 1), 2), (1, (2, 32, 16, 32, 5, 1, 2, 1), 0), (1, (2, 96, 15, 31, 3, 2, 1, 1), 2),
    (0, (2, 16, 21, 19, 3, 1, 3, 3), 1), (0, (1, 32, 30, 33, 5, 1, 12, 6), 0), (0, (2, 16, 18, 22, 5, 2, 2, 1), 2),
    (0, (1, 8, 1, 1, 3, 1, 1, 1), 0), (0, (1, 16, 14, 97, 5, 1, 6, 3), 2)],
    ids=lambda g: _dw_id(g[1]) + "_pro{}".format(g[2]))
@pytest.mark.parametrize("act,tie", ACT_TIE)
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_depthwise_weight_gradient_with_bn_backward_is_exact(geom, act, tie, dtype):
    """nasseg_dwconv_wgrad_bn: dz (written) and the depthwise weight gradient computed from it"""
    f = F()
    train, (B, C, H, W, k, s, p, d), pro = geom
    Ho, Wo = out_size(H, k, s, p, d), out_size(W, k, s, p, d)
    _pow2_pixels(train, B, Ho, Wo)
    M = B * Ho * Wo
    assert f.lib.query("nasseg_dwconv_strip_ok", k, s, d) == 1
    x, g, z = E.ints(B, C, H, W, seed=1), E.ints(B, C, Ho, Wo, seed=2), E.ints(B, C, Ho, Wo, seed=3)
    vec = E.bn_vectors(C, 4, tie=tie, M=M)
    isc, ish, iact = _prologue(C, pro, tie, 9)
    xi = _pro64(x, isc, ish, iact)
    _, dz_ref = bn_bwd64(g, z, vec[:4], vec[4].double(), M, train, act)
    E.assert_exactly_summable(lambda a, b: torch.nn.grad.conv2d_weight(a, (C, 1, k, k), b, s, p, d, C), [xi, dz_ref], 0.125,
                              "dw")
    dw_ref = torch.nn.grad.conv2d_weight(xi, (C, 1, k, k), dz_ref, s, p, d, C)
    xd, gd, zd, vd = dev(x, dtype), dev(g, dtype), dev(z, dtype), _to_dev(vec)
    pd = [None if v is None else v.to(DEV) for v in (isc, ish)]
    st = f.current_stream()
    nws = f.lib.query("nasseg_dwconv_wgrad_workspace", B, C, Ho, Wo, k)
    dz, dw, ws = torch.full_like(zd, NAN), torch.full((C, 1, k, k), NAN, device=DEV), torch.full((nws,), NAN, device=DEV)
    f.lib.call(f._k("nasseg_dwconv_wgrad_bn", xd), f.ptr(xd), f.ptr(gd), f.ptr(zd), f.ptr(dz), f.ptr(dw), f.ptr(ws),
               f.ptr(pd[0]), f.ptr(pd[1]), iact, f.ptr(vd[0]), f.ptr(vd[1]), f.ptr(vd[2]), f.ptr(vd[3]), f.ptr(vd[4]), train,
               act, B, H, W, C, Ho, Wo, k, s, p, d, st)
    torch.cuda.synchronize()
    E.assert_bitwise(dz, dz_ref, "dz")
    E.assert_bitwise(dw, dw_ref, "dw")


@pytest.mark.parametrize("geom", [
    # train, (B, C, H, W, stride): 3x3, pad 1
    (1, (2, 96, 15, 31, 2)), (1, (2, 144, 8, 16, 1)), (0, (1, 32, 33, 40, 1)), (0, (2, 24, 17, 23, 2)), (0, (1, 16, 1, 1, 1)),
    (1, (1, 16, 1, 1, 2))], ids=lambda g: "B{}C{}_{}x{}_s{}".format(*g[1]))
@pytest.mark.parametrize("act,tie", ACT_TIE)
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_depthwise_backward_between_batchnorms_is_exact(geom, act, tie, dtype):
    """nasseg_dwconv_bwd_bn: BatchNorm backward behind the conv on load, weight gradient (and its partial rows), the
    input gradient masked with the ReLU6 of the BatchNorm in front and that BatchNorm's rows {sum ge, sum ge * xhat}"""
    f = F()
    lib, ptr = f.lib, f.ptr
    train, (B, C, H, W, s) = geom
    k, p, d = 3, 1, 1
    Ho, Wo = out_size(H, k, s, p, d), out_size(W, k, s, p, d)
    _pow2_pixels(train, B, Ho, Wo)
    M = B * Ho * Wo
    rows = lib.query("nasseg_dwconv_bwd_bn_rows", B, C, H, W, k, s, p, d)
    assert rows > 0
    xz, g, z = E.ints(B, C, H, W, seed=1), E.ints(B, C, Ho, Wo, seed=2, lo=-2, hi=2), E.ints(B, C, Ho, Wo, seed=3)
    w = E.ints(C, 1, k, k, seed=4, lo=-2, hi=2)
    ivec = E.bn_vectors(C, 5, tie=tie)
    vec = E.bn_vectors(C, 9, tie=tie, M=M)
    iact = 2
    pre_in = xz.double() * cv(ivec[0]) + cv(ivec[1])
    xi = act64(pre_in, iact)
    _, dz_ref = bn_bwd64(g, z, vec[:4], vec[4].double(), M, train, act)
    E.assert_exactly_summable(lambda a, b, c: (torch.nn.grad.conv2d_weight(a, (C, 1, k, k), b, s, p, d, C),
                                               torch.nn.grad.conv2d_input((B, C, H, W), c, b, s, p, d, C)),
                              [xi, dz_ref, w], 0.125, "dw, ge")
    dw_ref = torch.nn.grad.conv2d_weight(xi, (C, 1, k, k), dz_ref, s, p, d, C)
    ge_ref = torch.nn.grad.conv2d_input((B, C, H, W), w.double(), dz_ref, s, p, d, C) * mask64(pre_in, iact)
    sums_ref = _bn_sums64(ge_ref, xz.double(), ivec)
    xd, gd, zd = dev(xz, dtype), dev(g, dtype), dev(z, dtype)
    iv, vd = _to_dev(ivec), _to_dev(vec)
    st = f.current_stream()
    wd = w.to(DEV)
    wt = torch.empty(9 * C, device=DEV)
    lib.call("nasseg_dw_pack_weight", ptr(wd), ptr(wt), C, k, int(s == 1), st)
    ge, dw = torch.full_like(xd, NAN), torch.full((C, 1, k, k), NAN, device=DEV)
    ws = torch.full((rows * 9 * C,), NAN, device=DEV)
    part = torch.full(((rows + 64) * 2 * C,), NAN, device=DEV)
    lib.call(f._k("nasseg_dwconv_bwd_bn", xd), ptr(xd), ptr(gd), ptr(zd), ptr(wt), int(s == 1), ptr(ge), ptr(dw), ptr(ws),
             ptr(iv[0]), ptr(iv[1]), ptr(iv[2]), ptr(iv[3]), iact, ptr(vd[0]), ptr(vd[1]), ptr(vd[2]), ptr(vd[3]),
             ptr(vd[4]), train, act, B, H, W, C, Ho, Wo, k, s, p, d, ptr(part), st)
    torch.cuda.synchronize()
    E.assert_bitwise(ge, ge_ref, "masked input gradient")
    E.assert_bitwise(dw, dw_ref, "dw")
    E.assert_bitwise(ws.view(rows, 9, C).double().sum(0).t().reshape(C, 1, 3, 3), dw_ref, "partial rows of dw")
    E.assert_bitwise(rows_sum64(part, rows, 2 * C), sums_ref, "rows of the BatchNorm in front")


_T, _E = (2, 8, 16), (3, 9, 11)  # 256 pixels (a power of two: training-mode BatchNorm) / 297 (a ragged last tile)
PW_BWD_CASES = [
    # train, (B, H, W, K, N), prologue
    (1, (2, 4, 8, 16, 96), 0), (1, (4, 16, 16, 24, 144), 2), (1, (2, 16, 16, 32, 32), 1), (0, (1, 31, 33, 32, 192), 2),
    (0, (3, 9, 11, 24, 64), 0), (1, (1, 1, 1, 16, 32), 0), (0, (2, 16, 20, 224, 64), 1), (1, (2, 8, 8, 128, 32), 0),
    # Every instantiation of csrc/conv_pwbwd.hip (tests/test_dispatch_host.py holds this list to that), on the smallest
    # maps with several tiles and slabs.  The narrow kernel holds nt x kt 16-wide tiles of N x K per wave; per (nt, kt)
    # one channel pair with a prologue (the PRO and the DXS kernels) and one without, none a multiple of 16:
    # (2, 1), (3, 1), (4, 1), (6, 1), (9, 1), (12, 1)
    (1, _T + (8, 20), 1), (1, _T + (8, 36), 2), (0, _E + (4, 40), 0), (1, _T + (12, 52), 1), (0, _E + (16, 56), 0),
    (0, _E + (12, 84), 2), (1, _T + (16, 128), 2), (0, _E + (8, 112), 0), (0, _E + (12, 148), 1), (1, _T + (16, 180), 0),
    # (2, 2), (3, 2), (4, 2), (6, 2), (9, 2), (12, 2)
    (0, _E + (28, 20), 0), (1, _T + (20, 36), 1), (0, _E + (32, 44), 0), (1, _T + (28, 52), 2), (1, _T + (20, 68), 1),
    (0, _E + (24, 92), 0), (0, _E + (20, 132), 0), (0, _E + (20, 180), 0),
    # (2, 4), (3, 4), (4, 4), (6, 4)
    (1, _T + (36, 20), 2), (0, _E + (64, 28), 0), (0, _E + (40, 36), 1), (1, _T + (52, 44), 0), (1, _T + (52, 52), 1),
    (0, _E + (36, 60), 0), (0, _E + (60, 84), 2), (1, _T + (36, 68), 0),
    # the wide kernel, 2 .. 6 chunks of 64 input channels, its four waves splitting N: one N tile (three waves idle),
    # two, three and four
    (1, _T + (68, 12), 1), (0, _E + (132, 12), 2), (1, _T + (164, 52), 0), (0, _E + (196, 36), 0), (1, _T + (260, 20), 1),
    (0, _E + (320, 64), 0), (0, _E + (324, 52), 2), (1, _T + (384, 28), 0)]


def pw_bwd_kernel_ids(lib, geom):
    """{(id, prologue != 0)}: the kernels nasseg_conv_pw_bwd_bn launches over the test below for one case - z loaded
    and z rebuilt where the plan can, and the call with z == NULL where a kernel serves it"""
    _, (B, H, W, K, N), pro = geom
    ids = set()
    for rz in (0, HUGE):
        with knobs(conv_pw_bwd_rz_min_pixels=rz):
            ids.add(lib.query("nasseg_conv_pw_bwd_kernel_id", B, H, W, K, N, 0))
            ids.add(lib.query("nasseg_conv_pw_bwd_kernel_id", B, H, W, K, N, 1))
    return {(i, bool(pro)) for i in ids if i >= 0}


@pytest.mark.parametrize("geom", PW_BWD_CASES, ids=lambda g: "B{}_{}x{}_K{}N{}_pro{}".format(*g[1], g[2]))
@pytest.mark.parametrize("act,tie", ACT_TIE)
@pytest.mark.parametrize("rz", [0, HUGE], ids=["rebuild_z", "load_z"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_pointwise_backward_with_bn_in_one_kernel_is_exact(geom, act, tie, rz, dtype):
    """nasseg_conv_pw_bwd_bn: dx, dw, the partial rows finished by nasseg_wgrad_finalize_many (dw == NULL), z == NULL
    (forces the rebuild where nasseg_conv_pw_bwd_kernel_id names a kernel that can, an error elsewhere), dx_res,
    dx_stats - z loaded and z rebuilt"""
    f = F()
    lib, ptr = f.lib, f.ptr
    train, (B, H, W, K, N), pro = geom
    _pow2_pixels(train, B, H, W)
    M = B * H * W
    x, g = E.ints(B, K, H, W, seed=1, lo=-2, hi=2, density=0.6), E.ints(B, N, H, W, seed=2, lo=-2, hi=2)
    w = E.ints(N, K, 1, 1, seed=4, lo=-1, hi=1, density=min(0.5, 6.0 / K))  # (keeps |z| to a few bits whatever K)
    isc, ish, iact = _prologue(K, pro, tie, 9)
    imean, iinv = E.ints(K, lo=-1, hi=1, seed=12), E.pow2(K, -1, 1, seed=13, signed=False)
    xi = _pro64(x, isc, ish, iact)
    E.assert_exactly_summable(lambda a, b: TF.conv2d(a, b), [xi, w], 0.5, "z")
    z_ref = TF.conv2d(xi, w.double())  # (the conv's own output: the kernel may rebuild it from x and w)
    assert float(z_ref.abs().max()) <= 127 and bool((z_ref * 2 == (z_ref * 2).round()).all())
    vec = E.bn_vectors(N, 5, tie=tie, M=M)
    _, dz_ref = bn_bwd64(g, z_ref, vec[:4], vec[4].double(), M, train, act)
    skip = E.ints(B, K, H, W, seed=14)
    E.assert_exactly_summable(lambda a, b, c, e: (torch.nn.grad.conv2d_weight(a, (N, K, 1, 1), b),
                                                  torch.nn.grad.conv2d_input((B, K, H, W), c, b) + e),
                              [xi, dz_ref, w, skip], 0.125, "dw, dx")
    dw_ref = torch.nn.grad.conv2d_weight(xi, (N, K, 1, 1), dz_ref)
    dx_ref = torch.nn.grad.conv2d_input((B, K, H, W), w.double(), dz_ref)
    pre_in = x.double() * cv(isc) + cv(ish) if pro else x.double()
    xd, gd, zd = dev(x, dtype), dev(g, dtype), dev(z_ref.float(), dtype)
    assert torch.equal(zd.float().cpu().double(), z_ref)  # (bf16 stores it exactly)
    vd = _to_dev(vec)
    pd = [None if v is None else v.to(DEV) for v in (isc, ish)]
    st = f.current_stream()
    wd = w.to(DEV)
    with knobs(conv_pw_bwd_rz_min_pixels=rz):
        nsl = lib.query("nasseg_conv_pw_bwd_slabs", B, H, W, K, N)
        assert nsl > 0
        reads_z = lib.query("nasseg_conv_pw_bwd_reads_z", B, H, W, K, N)
        if rz == 0 and K <= 32 and N <= 96:
            assert not reads_z
        if rz:
            assert reads_z
        wb = torch.empty(N * K, device=DEV)
        lib.call("nasseg_conv_pack_weight", ptr(wd), ptr(wb), N, K, 1, 1, 1, st)

        def call(z, dw, dx_act, in_stats=None, res=None, what=""):
            dx = torch.full_like(xd, NAN)
            ws = torch.full((nsl * N * K,), NAN, device=DEV)
            part = torch.full(((nsl + 64) * 2 * K,), NAN, device=DEV) if in_stats else None
            lib.call(f._k("nasseg_conv_pw_bwd_bn", xd), ptr(xd), ptr(gd), ptr(z), ptr(wb), ptr(dx), ptr(dw), ptr(ws),
                     ptr(pd[0]), ptr(pd[1]), iact, dx_act, ptr(vd[0]), ptr(vd[1]), ptr(vd[2]), ptr(vd[3]), ptr(vd[4]),
                     train, act, B, H, W, K, N, ptr(in_stats[0]) if in_stats else None,
                     ptr(in_stats[1]) if in_stats else None, ptr(part), ptr(res), st)
            torch.cuda.synchronize()
            want = dx_ref * mask64(pre_in, dx_act) + (res.float().cpu().double() if res is not None else 0.0)
            E.assert_bitwise(dx, want, what + ": dx")
            if dw is not None:
                E.assert_bitwise(dw, dw_ref, what + ": dw")
            E.assert_bitwise(ws.view(nsl, N * K).double().sum(0).view(N, K, 1, 1), dw_ref, what + ": partial rows of dw")
            return ws, part, want

        call(zd, torch.full((N, K, 1, 1), NAN, device=DEV), 0, what="plain")
        ws, _, _ = call(zd, None, iact, what="dw == NULL, dx masked")
        dw = torch.full((N, K, 1, 1), NAN, device=DEV)
        parts, outs = (ctypes.c_void_p * 1)(ptr(ws)), (ctypes.c_void_p * 1)(ptr(dw))
        lib.call("nasseg_wgrad_finalize_many", 1, parts, outs, (ctypes.c_int * 5)(nsl, 1, N, K, 0), st)
        E.assert_bitwise(dw, dw_ref, "nasseg_wgrad_finalize_many over the partial rows")
        kid, kid_null = [lib.query("nasseg_conv_pw_bwd_kernel_id", B, H, W, K, N, zn) for zn in (0, 1)]
        assert kid >= 0 and (kid < 10000 and kid % 10 == 1) == (not reads_z)  # (the launch asks the same table)
        if kid_null >= 0:
            assert kid_null < 10000 and kid_null % 10 == 1  # (a kernel that rebuilds z)
            call(None, torch.full((N, K, 1, 1), NAN, device=DEV), 0, what="z == NULL")
        else:
            with pytest.raises(RuntimeError):  # (no kernel can rebuild z there)
                call(None, torch.full((N, K, 1, 1), NAN, device=DEV), 0, what="z == NULL")
        if K % 4 == 0:
            call(zd, torch.full((N, K, 1, 1), NAN, device=DEV), iact, res=dev(skip, dtype), what="dx_res")
        if K <= 64 and pro:
            iv = [imean.to(DEV), iinv.to(DEV)]
            _, part, dxm = call(zd, torch.full((N, K, 1, 1), NAN, device=DEV), iact, in_stats=iv, what="dx_stats")
            if dtype == torch.bfloat16:  # (the rows are sums of dx AS STORED - what a separate pass would read back)
                dxm = dxm.float().to(torch.bfloat16).double()
            sums_ref = _bn_sums64(dxm, x.double(), [None, None, imean, iinv])
            E.assert_bitwise(rows_sum64(part, nsl, 2 * K), sums_ref, "rows of the BatchNorm in front")


@pytest.mark.parametrize("case", [
    # B, C, N, H, W, k, stride, pad, dil
    (2, 32, 32, 13, 17, 3, 1, 1, 1), (2, 24, 48, 16, 20, 5, 1, 2, 1), (2, 48, 24, 21, 19, 3, 1, 3, 3),
    (2, 32, 64, 30, 33, 5, 1, 12, 6), (2, 24, 24, 17, 23, 3, 2, 1, 1), (2, 16, 8, 18, 22, 5, 2, 2, 1),
    (3, 8, 16, 9, 5, 3, 1, 2, 2), (1, 16, 16, 1, 1, 3, 1, 1, 1), (4, 64, 48, 70, 189, 3, 1, 1, 1)],
    ids=lambda c: "B{}C{}N{}_{}x{}_k{}s{}p{}d{}".format(*c))
@pytest.mark.parametrize("pro,tie", [(0, True), (1, True), (1, False), (2, True), (2, False)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_sepconv_stage_is_exact(case, pro, tie, dtype):
    """nasseg_sepconv_fwd: zdw = dwconv(pro(x)) (stored), y = conv1x1(zdw) with its statistics rows; and the inference
    form with the folded affine + activation epilogue.  zdw is kept to 8 significant bits, so bf16 storage holds it
    exactly whether the pointwise stage reads the stored or the unrounded value."""
    f = F()
    lib, ptr = f.lib, f.ptr
    B, C, N, H, W, k, s, p, d = case
    Ho, Wo = out_size(H, k, s, p, d), out_size(W, k, s, p, d)
    nblk = lib.query("nasseg_sepconv_blocks", B, C, Ho, Wo, N, k, s, d)
    assert nblk > 0
    big = B * Ho * Wo > 8192  # (thinner weights there: the sums of y^2 over all pixels must stay exact)
    x = E.ints(B, C, H, W, seed=1, lo=-1, hi=1)
    wdw = E.ints(C, 1, k, k, seed=2, lo=-1, hi=1, density=0.1 if big else 0.4)
    wpw = E.ints(N, C, 1, 1, seed=3, lo=-1, hi=1, density=min(0.5, (2.0 if big else 6.0) / C))
    isc, ish, iact = _prologue(C, pro, tie, 4)
    xi = _pro64(x, isc, ish, iact)
    E.assert_exactly_summable(lambda a, b, c: TF.conv2d(TF.conv2d(a, b, None, s, p, d, C), c), [xi, wdw, wpw], 0.5, "y")
    z_ref = TF.conv2d(xi, wdw.double(), None, s, p, d, C)
    assert torch.equal(z_ref.float().to(torch.bfloat16).double(), z_ref), "zdw needs more than 8 bits: thin the inputs"
    y_ref = TF.conv2d(z_ref, wpw.double())
    E.assert_stats_summable(y_ref, 0.5, "statistics of y")
    osc, osh = E.pow2(N, 0, 1, seed=6), E.ints(N, lo=-2, hi=4, seed=7, offset=0.0 if tie else 0.5)
    y2_ref = act64(y_ref * cv(osc) + cv(osh), 1 + (pro == 2))
    xd = dev(x, dtype)
    st = f.current_stream()
    wt = torch.empty(k * k * C, device=DEV)
    wdd, wpd = wdw.to(DEV), wpw.to(DEV).contiguous()
    lib.call("nasseg_dw_pack_weight", ptr(wdd), ptr(wt), C, k, 0, st)
    pd = [None if v is None else v.to(DEV) for v in (isc, ish)]
    z = dev(torch.full((B, C, Ho, Wo), NAN), dtype)
    y = dev(torch.full((B, N, Ho, Wo), NAN), dtype)
    part = torch.full((nblk * 2 * N,), NAN, device=DEV)
    lib.call(f._k("nasseg_sepconv_fwd", xd), ptr(xd), ptr(wt), ptr(wpd), ptr(z), ptr(y), ptr(pd[0]), ptr(pd[1]), iact,
             None, None, 0, B, H, W, C, Ho, Wo, N, k, s, p, d, ptr(part), st)
    y2 = dev(torch.full((B, N, Ho, Wo), NAN), dtype)
    od = [osc.to(DEV), osh.to(DEV)]
    lib.call(f._k("nasseg_sepconv_fwd", xd), ptr(xd), ptr(wt), ptr(wpd), None, ptr(y2), ptr(pd[0]), ptr(pd[1]), iact,
             ptr(od[0]), ptr(od[1]), 1 + (pro == 2), B, H, W, C, Ho, Wo, N, k, s, p, d, None, st)
    torch.cuda.synchronize()
    E.assert_bitwise(z, z_ref, "zdw")
    E.assert_bitwise(y, y_ref, "y")
    yd = y_ref.permute(1, 0, 2, 3).reshape(N, -1)
    got = part.view(nblk, 2, N).double().sum(0).cpu()
    E.assert_bitwise(got[0], yd.sum(1), "statistics rows: sum y")
    E.assert_bitwise(got[1], (yd * yd).sum(1), "statistics rows: sum y^2")
    E.assert_bitwise(y2, y2_ref, "folded epilogue")


IRDW_CASES = [
    # train of the BatchNorm behind the depthwise conv (then B * Ho * Wo is a power of two), (B, K, C, H, W, stride)
    (1, (2, 16, 96, 15, 31, 2)), (1, (2, 24, 144, 8, 16, 1)), (0, (1, 32, 192, 19, 33, 1)), (0, (2, 24, 144, 17, 23, 2)),
    (0, (1, 16, 96, 1, 1, 1)), (1, (1, 8, 48, 16, 64, 1)), (0, (2, 4, 16, 9, 29, 2)),
    # Off MobileNetV2's expansions (tests/test_dispatch_host.py holds this list to every launch shape of csrc/irdw.hip):
    # a workgroup is 64 * waves threads, waves = 4 | 3 | 2 | 1 by the divisibility of C / 16, the grid (rows, groups).
    # Two waves with one group and with five; one wave with five groups and with seven; four waves with one group and
    # with two - each at both strides, K <= 16 and K > 16; two chunks of rows and two strips of columns in either
    # direction (16 x 16 and 9 x 17 at stride 1, 31 x 31 and 17 x 33 at stride 2)
    (1, (1, 8, 32, 16, 16, 1)), (0, (1, 20, 160, 17, 33, 2)), (0, (2, 16, 80, 9, 17, 1)), (1, (1, 20, 112, 31, 31, 2)),
    (1, (1, 24, 64, 31, 31, 2)), (0, (2, 16, 128, 9, 17, 1))]
_irdw_id = lambda g: "B{}_{}to{}_{}x{}_s{}".format(*g[1])  # noqa: E731


def _irdw_inputs(geom, pro, tie):
    B, K, C, H, W, s = geom
    x = E.ints(B, K, H, W, seed=1, lo=-2, hi=2, density=0.6)
    w1 = E.ints(C, K, 1, 1, seed=2, lo=-1, hi=1, density=min(0.5, 3.0 / K))
    wd = E.ints(C, 1, 3, 3, seed=3, lo=-1, hi=1)
    isc, ish, iact = _prologue(K, pro, tie, 4)
    xi = _pro64(x, isc, ish, iact)
    E.assert_exactly_summable(lambda a, b: TF.conv2d(a, b), [xi, w1], 0.5, "z1")
    z1 = TF.conv2d(xi, w1.double())
    vec1 = E.bn_vectors(C, 6, tie=tie)
    return x, w1, wd, (isc, ish, iact), z1, vec1


@pytest.mark.parametrize("geom", IRDW_CASES, ids=_irdw_id)
@pytest.mark.parametrize("pro,act1,tie", [(0, 2, True), (1, 2, False), (2, 1, True), (1, 1, False), (0, 0, True)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_irdw_forward_is_exact(geom, pro, act1, tie, dtype):
    """nasseg_irdw_fwd: z2 = dwconv3x3(act1(bn1_scale * (W1 pro(x)) + bn1_shift)) and the statistics rows of z2"""
    f = F()
    lib, ptr = f.lib, f.ptr
    _, (B, K, C, H, W, s) = geom
    Ho, Wo = out_size(H, 3, s, 1, 1), out_size(W, 3, s, 1, 1)
    x, w1, wd, (isc, ish, iact), z1, vec1 = _irdw_inputs(geom[1], pro, tie)
    a1 = act64(z1 * cv(vec1[0]) + cv(vec1[1]), act1)
    E.assert_exactly_summable(lambda a, b: TF.conv2d(a, b, None, s, 1, 1, C), [a1, wd], 0.5, "z2")
    z2_ref = TF.conv2d(a1, wd.double(), None, s, 1, 1, C)  # (multiples of 1/2: x, W1 integers, shifts integers + 1/2)
    E.assert_stats_summable(z2_ref, 0.5, "statistics of z2")
    rows = lib.query("nasseg_irdw_rows", B, H, W, K, C, s, 0)
    assert rows > 0
    st = f.current_stream()
    xd = dev(x, dtype)
    wt = torch.empty(9 * C, device=DEV)
    wdd, w1d = wd.to(DEV), w1.to(DEV)
    lib.call("nasseg_dw_pack_weight", ptr(wdd), ptr(wt), C, 3, 0, st)
    pd = [None if v is None else v.to(DEV) for v in (isc, ish)]
    v1 = _to_dev(vec1)
    z2 = dev(torch.full((B, C, Ho, Wo), NAN), dtype)
    part = torch.full(((rows + 64) * 2 * C,), NAN, device=DEV)
    lib.call(f._k("nasseg_irdw_fwd", xd), ptr(xd), ptr(w1d), ptr(wt), ptr(z2), ptr(pd[0]), ptr(pd[1]), iact, ptr(v1[0]),
             ptr(v1[1]), act1, B, H, W, K, C, Ho, Wo, s, ptr(part), st)
    torch.cuda.synchronize()
    E.assert_bitwise(z2, z2_ref, "z2")
    zd = z2_ref.permute(1, 0, 2, 3).reshape(C, -1)
    got = rows_sum64(part, rows, 2 * C)
    E.assert_bitwise(got[:C], zd.sum(1), "statistics rows: sum z2")
    E.assert_bitwise(got[C:], (zd * zd).sum(1), "statistics rows: sum z2^2")


@pytest.mark.parametrize("geom", IRDW_CASES, ids=_irdw_id)
@pytest.mark.parametrize("pro,act1,act,tie", [(0, 2, 0, True), (1, 2, 2, True), (1, 2, 2, False), (2, 1, 1, True),
                                              (2, 1, 1, False), (0, 0, 2, True)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_irdw_backward_is_exact(geom, pro, act1, act, tie, dtype):
    """nasseg_irdw_bwd: nasseg_dwconv_bwd_bn with z1 = W1 pro(x) rebuilt from the block's input"""
    f = F()
    lib, ptr = f.lib, f.ptr
    train, (B, K, C, H, W, s) = geom
    Ho, Wo = out_size(H, 3, s, 1, 1), out_size(W, 3, s, 1, 1)
    _pow2_pixels(train, B, Ho, Wo)
    M = B * Ho * Wo
    x, w1, wd, (isc, ish, iact), z1, vec1 = _irdw_inputs(geom[1], pro, tie)
    g, z2 = E.ints(B, C, Ho, Wo, seed=11, lo=-2, hi=2), E.ints(B, C, Ho, Wo, seed=12)
    vec2 = E.bn_vectors(C, 13, tie=tie, M=M)
    pre1 = z1 * cv(vec1[0]) + cv(vec1[1])
    a1 = act64(pre1, act1)
    _, dz_ref = bn_bwd64(g, z2, vec2[:4], vec2[4].double(), M, train, act)
    E.assert_exactly_summable(lambda a, b, c: (torch.nn.grad.conv2d_weight(a, (C, 1, 3, 3), b, s, 1, 1, C),
                                               torch.nn.grad.conv2d_input((B, C, H, W), c, b, s, 1, 1, C)),
                              [a1, dz_ref, wd], 0.125, "dw, ge")
    dw_ref = torch.nn.grad.conv2d_weight(a1, (C, 1, 3, 3), dz_ref, s, 1, 1, C)
    ge_ref = torch.nn.grad.conv2d_input((B, C, H, W), wd.double(), dz_ref, s, 1, 1, C) * mask64(pre1, act1)
    sums_ref = _bn_sums64(ge_ref, z1, vec1)
    rows = lib.query("nasseg_irdw_rows", B, H, W, K, C, s, 1)
    assert rows > 0
    st = f.current_stream()
    xd, gd, zd = dev(x, dtype), dev(g, dtype), dev(z2, dtype)
    wt = torch.empty(9 * C, device=DEV)
    wdd, w1d = wd.to(DEV), w1.to(DEV)
    lib.call("nasseg_dw_pack_weight", ptr(wdd), ptr(wt), C, 3, int(s == 1), st)
    pd = [None if v is None else v.to(DEV) for v in (isc, ish)]
    v1, v2 = _to_dev(vec1), _to_dev(vec2)
    ge = dev(torch.full((B, C, H, W), NAN), dtype)
    dw = torch.full((C, 1, 3, 3), NAN, device=DEV)
    ws = torch.full((rows * 9 * C,), NAN, device=DEV)
    part = torch.full(((rows + 64) * 2 * C,), NAN, device=DEV)
    lib.call(f._k("nasseg_irdw_bwd", xd), ptr(xd), ptr(w1d), ptr(gd), ptr(zd), ptr(wt), int(s == 1), ptr(ge), ptr(dw),
             ptr(ws), ptr(pd[0]), ptr(pd[1]), iact, ptr(v1[0]), ptr(v1[1]), ptr(v1[2]), ptr(v1[3]), act1, ptr(v2[0]),
             ptr(v2[1]), ptr(v2[2]), ptr(v2[3]), ptr(v2[4]), train, act, B, H, W, K, C, Ho, Wo, s, ptr(part), st)
    torch.cuda.synchronize()
    E.assert_bitwise(ge, ge_ref, "gradient w.r.t. the expansion's BatchNorm output")
    E.assert_bitwise(dw, dw_ref, "dw")
    E.assert_bitwise(ws.view(rows, 9, C).double().sum(0).t().reshape(C, 1, 3, 3), dw_ref, "partial rows of dw")
    E.assert_bitwise(rows_sum64(part, rows, 2 * C), sums_ref, "rows of the expansion's BatchNorm")


def _ulps(got, ref64):
    """|got - ref| in units of the fp32 spacing at |ref|"""
    ref32 = ref64.float()
    ulp = (torch.nextafter(ref32.abs(), torch.full_like(ref32, float("inf"))) - ref32.abs()).double()
    return float(((got.cpu().double() - ref64).abs() / ulp).max())


@pytest.mark.parametrize("geom", [(2, 16, 96, 8, 16), (1, 24, 144, 16, 32), (4, 32, 192, 4, 4), (1, 8, 48, 1, 2),
                                  (2, 4, 16, 32, 64), (1, 20, 160, 16, 16), (2, 12, 80, 8, 16)],
                         ids=lambda g: "B{}_{}to{}_{}x{}".format(*g))
@pytest.mark.parametrize("pro,tie", [(0, True), (1, True), (2, False)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_irdw_statistics_from_the_moments_of_the_input(geom, pro, tie, dtype):
    """nasseg_irdw_stats over M = 2^n pixels of integer inputs: the mean is exact.  invstd = 1 / sqrt(var + eps), scale =
    gamma * invstd (gamma +- a power of two) and shift = beta - mean * scale are NOT bitwise - the only such comparison
    in this file: 1 / sqrt(var + eps) is not representable, so the kernel's value is the fp32 rounding of a double
    computed from the (exact) moments: half an ulp for the rounding, the rest of one ulp for sqrt and division in
    double.  beta is given the sign of -mean * scale, so that the two terms of shift do not cancel and one ulp of shift
    bounds the same two roundings.  running_mean moves by momentum * mean exactly when it starts at 0."""
    f = F()
    lib, ptr = f.lib, f.ptr
    B, K, C, H, W = geom
    M = B * H * W
    assert M & (M - 1) == 0 and M >= 2
    x, w1, _, (isc, ish, iact), z1, _ = _irdw_inputs((B, K, C, H, W, 1), pro, tie)
    mean_ref = z1.mean((0, 2, 3))
    var_ref = z1.var((0, 2, 3), unbiased=False)
    eps, mom = 1e-5, 0.125
    invstd_ref = 1.0 / (var_ref + float(torch.tensor(eps, dtype=torch.float32))).sqrt()
    gamma = E.pow2(C, -1, 1, seed=21)
    scale_ref = gamma.double() * invstd_ref
    sign = torch.where(-mean_ref * scale_ref < 0, -1.0, 1.0)
    beta = (E.ints(C, lo=0, hi=3, seed=22).double() * sign).float()
    shift_ref = beta.double() - mean_ref * scale_ref
    st = f.current_stream()
    xd = dev(x, dtype)
    pd = [None if v is None else v.to(DEV) for v in (isc, ish)]
    out = [torch.full((C,), NAN, device=DEV) for _ in range(4)]
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    nbt = torch.full((), 7, device=DEV, dtype=torch.int64)
    ws = torch.full((lib.query("nasseg_irdw_stats_workspace", K),), NAN, device=DEV)
    w1d, gd, bd = w1.to(DEV), gamma.to(DEV), beta.to(DEV)
    lib.call(f._k("nasseg_irdw_stats", xd), ptr(xd), ptr(w1d), ptr(pd[0]), ptr(pd[1]), iact, B, H, W, K, C, eps, mom,
             ptr(gd), ptr(bd), *[ptr(o) for o in out], ptr(rm), ptr(rv), ptr(nbt), ptr(ws), st)
    torch.cuda.synchronize()
    E.assert_bitwise(out[0], mean_ref, "mean")
    E.assert_bitwise(rm, mean_ref * mom, "running_mean")
    assert int(nbt) == 8
    for o, r, what in ((out[1], invstd_ref, "invstd"), (out[2], scale_ref, "scale"), (out[3], shift_ref, "shift")):
        assert bool(torch.isfinite(o).all()), what
        nz = r != 0
        u = _ulps(o.cpu()[nz], r[nz]) if bool(nz.any()) else 0.0
        assert u <= 1.0, "{}: {:.3f} ulp from the float64 value".format(what, u)
