"""Float64 host restatement of the full-size cross-entropy (csrc/loss_up.hip: nasseg_ce_up_fwd / _bwd;
F.cross_entropy_upsampled; INTEGRATION.md, "Losses").

logits x [B][h][w][C], labels t [B][H][W] at any size, optional weights [C].  For label pixel (b, Y, X):
ly = lin_coeff(Y, h/H, h, H), lx = lin_coeff(X, w/W, w, W) (csrc/resize_index.h), and for every channel
  top = l0x x00 + l1x x01,  bot = l0x x10 + l1x x11,  v = l0y top + l1y bot.
The rest is tests/_segm_loss_ref.py over the B*H*W rows v: validity, l = logsumexp(v) - v_t, the selection, the loss
and the gradient g [P][C] with respect to v; the gradient with respect to the stored logits is the explicit double sum
  dx[b][i][j][c] = sum_{Y, X} Wy(Y, i) Wx(X, j) g[(b, Y, X)][c],  Wy(Y, i) = l0y [i0(Y) == i] + l1y [i1(Y) == i].

``lin_coeff`` is restated in numpy float32 (``coeffs(..., np.float32)``) so that i0, i1, l0, l1 are the kernel's own
numbers - everything after them is float64; with ``np.float64`` the coordinates are float64 too, which is what torch's
float64 ``interpolate`` computes.  ``upsampled_fp32`` is the same formulas in plain float32 numpy (every product and sum
rounded on its own), on a given kept set: what fp32 arithmetic costs on an input, to size a bound with."""
import numpy as np

import _segm_loss_ref as CE


def coeffs(out_size, in_size, dtype=np.float32):
    """(i0, i1 int64 [out], l0, l1 float64 [out]) of lin_coeff(dst, in/out, in, out) for dst = 0 .. out - 1.
    float32: the kernel's arithmetic - scale = float32(in) / float32(out); src = scale * (dst + 0.5) - 0.5 rounded ONCE
    (the compiler contracts the multiply-add of lin_coeff into one fused operation; the product of a float32 and a
    half-integer below 2^24 is exact in float64, so rounding the float64 value is that operation); l1 = src - i0 and
    l0 = 1 - l1 in float32."""
    dst = np.arange(out_size)
    if in_size == out_size:
        return dst.copy(), dst.copy(), np.ones(out_size), np.zeros(out_size)
    if dtype == np.float32:
        scale = np.float32(in_size) / np.float32(out_size)
        src = (np.float64(scale) * (dst.astype(np.float64) + 0.5) - 0.5).astype(np.float32)
    else:
        src = np.float64(in_size) / np.float64(out_size) * (dst.astype(np.float64) + 0.5) - 0.5
    src = np.maximum(src, dtype(0))
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    l1 = np.clip(src - i0.astype(dtype), dtype(0), dtype(1)).astype(dtype)
    l0 = (dtype(1) - l1).astype(dtype)
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64)


def weight_matrix(co, in_size):
    """M [out][in] float64: M[o][i] = l0 [i0(o) == i] + l1 [i1(o) == i]"""
    i0, i1, l0, l1 = co
    M = np.zeros((len(i0), in_size), np.float64)
    np.add.at(M, (np.arange(len(i0)), i0), l0)
    np.add.at(M, (np.arange(len(i0)), i1), l1)
    return M


def interpolate(x, cy, cx, dtype=np.float64):
    """v [B][H][W][C] in ``dtype`` from x [B][h][w][C]: the three lines of the module's docstring, every product and
    sum a numpy operation of its own"""
    x = np.asarray(x, dtype)
    i0y, i1y, l0y, l1y = cy
    i0x, i1x, l0x, l1x = cx
    l0x, l1x = l0x.astype(dtype)[None, None, :, None], l1x.astype(dtype)[None, None, :, None]
    l0y, l1y = l0y.astype(dtype)[None, :, None, None], l1y.astype(dtype)[None, :, None, None]
    r0, r1 = x[:, i0y], x[:, i1y]
    top = l0x * r0[:, :, i0x] + l1x * r0[:, :, i1x]
    bot = l0x * r1[:, :, i0x] + l1x * r1[:, :, i1x]
    return l0y * top + l1y * bot


def gather(g, My, Mx):
    """dx [B][h][w][C] = sum_{Y, X} My[Y][i] Mx[X][j] g[b][Y][X][c], in the dtype of g"""
    t = np.tensordot(My.astype(g.dtype).T, g, axes=([1], [1]))  # [i][b][X][c]
    t = np.tensordot(Mx.astype(g.dtype).T, t, axes=([1], [2]))  # [j][i][b][c]
    return np.ascontiguousarray(t.transpose(2, 1, 0, 3))


def upsampled(x, t, weight=None, ignore_index=255, thresh=None, min_kept=0, keep_fraction=0.0, coeff_dtype=np.float32):
    """dict(loss, grad [B][h][w][C], pixel_loss [B][H][W], kept [B][H][W], v [B][H][W][C], tau, k, n, n_kept, ce: the
    dict of _segm_loss_ref.cross_entropy_select over the rows v) in float64"""
    x = np.asarray(x, np.float64)
    t = np.asarray(t)
    B, h, w, C = x.shape
    _, H, W = t.shape
    cy, cx = coeffs(H, h, coeff_dtype), coeffs(W, w, coeff_dtype)
    v = interpolate(x, cy, cx)
    ce = CE.cross_entropy_select(v.reshape(-1, C), t.reshape(-1), weight, ignore_index, thresh, min_kept,
                                 keep_fraction)
    grad = gather(ce["grad"].reshape(B, H, W, C), weight_matrix(cy, h), weight_matrix(cx, w))
    return dict(loss=ce["loss"], grad=grad, pixel_loss=ce["pixel_loss"].reshape(B, H, W),
                kept=ce["kept"].reshape(B, H, W), v=v, tau=ce["tau"], k=ce["k"], n=ce["n"], n_kept=ce["n_kept"],
                ce=ce)


def gap_to_tau(ref):
    return CE.gap_to_tau(ref["ce"])


def upsampled_fp32(x, t, kept, weight=None):
    """(loss, grad [B][h][w][C], pixel_loss [B][H][W]) of the same formulas in plain float32 numpy on the kept set
    ``kept`` [B][H][W] (the float64 one: a selection is not what this sizes)"""
    f = np.float32
    x = np.asarray(x, f)
    t = np.asarray(t).astype(np.int64)
    B, h, w, C = x.shape
    _, H, W = t.shape
    cy, cx = coeffs(H, h), coeffs(W, w)
    v = interpolate(x, cy, cx, f).reshape(-1, C)
    kept = np.asarray(kept).reshape(-1)
    tt = np.where(kept, t.reshape(-1), 0)
    m = v.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(v - m).sum(axis=1, keepdims=True, dtype=f)))[:, 0]
    l = lse - v[np.arange(len(tt)), tt]
    wt = np.ones(C, f) if weight is None else np.asarray(weight, f)
    wp = np.where(kept, wt[tt], f(0)).astype(f)
    sum_w = wp.sum(dtype=f)
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = (wp * np.where(kept, l, f(0))).sum(dtype=f) / sum_w
        g = np.exp(v - lse[:, None])
        g[np.arange(len(tt)), tt] -= f(1)
        g = ((wp / sum_w)[:, None] * g).astype(f)
    g[~kept] = 0
    grad = gather(g.reshape(B, H, W, C), weight_matrix(cy, h), weight_matrix(cx, w))
    return float(loss), grad.astype(np.float64), np.where(kept, l, f(-1)).reshape(B, H, W)


def nearest(out_size, in_size):
    """the source index of a nearest resize, in exact integers (used to MAKE inputs only)"""
    return np.minimum(np.arange(out_size) * in_size // out_size, in_size - 1)


def make_case(lshape, tshape, C, seed, scale=1.0, boosted=0.6, label_dtype=np.int64):
    """Inputs in the manner of make_case of tests/test_hip_region_loss.py, at two sizes: logits [B][h][w][C] with
    |x| <= 12 (+6 on the channel of its own label for ``boosted`` of the logits pixels), full-size labels [B][H][W]
    that follow the nearest logits pixel's label except for 30 % drawn afresh, 20 % of them ignored - so that
    thresh = 0.7 splits the valid pixels - and class weights in [0.5, 1.5)."""
    B, h, w = lshape
    H, W = tshape
    rng = np.random.RandomState(seed)
    p = B * h * w
    x = np.clip(rng.randn(p, C) * scale, -12.0, 12.0).astype(np.float32)
    tl = rng.randint(0, C, size=p)
    boost = rng.rand(p) < boosted
    x[np.arange(p)[boost], tl[boost]] += np.float32(6.0)
    t = tl.reshape(B, h, w)[:, nearest(H, h)][:, :, nearest(W, w)].copy()
    fresh = rng.rand(B, H, W) < 0.3
    t[fresh] = rng.randint(0, C, size=int(fresh.sum()))
    t[rng.rand(B, H, W) < 0.2] = 255
    wt = (rng.rand(C) + 0.5).astype(np.float32)
    return x.reshape(B, h, w, C), t.astype(label_dtype), wt
