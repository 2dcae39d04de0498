"""Float64 host restatement of the Lovasz-Softmax term of the segmentation criterion (csrc/lovasz.hip:
nasseg_lovasz_coef / _fwd / _bwd; F.lovasz_softmax_loss, F.lovasz_from_errors, F.cross_entropy_select(lovasz_weight=
...); INTEGRATION.md, "Losses").

logits [P][C], labels [P].  Pixel p is valid iff its label t != ignore_index and 0 <= t < C; n valid pixels,
y_pc = [t_p == c], N_c = sum y_pc, q_p = softmax(x_p), e_pc = |y_pc - q_pc|.  Per class the valid pixels are ordered by
e DESCENDING, ties by ASCENDING pixel index; position i = 1 .. n, F_i = foreground pixels among the first i,
B_i = i - F_i, U = N_c + B_i; g_i = 1 / U on a foreground pixel, (N_c - F_i) / ((U - 1) U) on a background pixel
(1 where U - 1 = 0); loss_c = sum_i e_(i) g_i; K = the classes with N_c > 0 (classes="all": every class);
loss = mean_{c in K} loss_c, 0 when n = 0.  G_pc = -+ g / |K| (- on foreground), 0 outside K;
dloss/dx_pj = q_pj (G_pj - sum_c G_pc q_pc) on valid pixels, 0 on all others.

THE ORDER IS ALWAYS TAKEN FROM THE fp32 ERROR VALUES THE CALLER HANDS OVER (np.lexsort((index, -E))): the order is
part of the kernels' contract on the values they computed, and an order from this file's own float64 errors would
differ from it in a fraction of a percent of the ranks through rounding alone.  Values and q are float64."""
import numpy as np

import _segm_loss_ref as CE


def valid_mask(labels, C, ignore_index=255):
    t = np.asarray(labels).astype(np.int64)
    return (t != ignore_index) & (t >= 0) & (t < C)


def lovasz_gradient(fg, Nc):
    """g_i (float64) of a sorted 0/1 foreground vector by the closed forms"""
    fg = np.asarray(fg, bool)
    i = np.arange(1, len(fg) + 1, dtype=np.int64)
    F = np.cumsum(fg).astype(np.int64)
    U = Nc + (i - F)
    with np.errstate(divide="ignore", invalid="ignore"):
        bg = np.where(U - 1 > 0, (Nc - F).astype(np.float64) / ((U - 1).astype(np.float64) * U.astype(np.float64)), 1.0)
    return np.where(fg, 1.0 / U.astype(np.float64), bg)


def jaccard_differences(fg, Nc):
    """J_i - J_(i-1), J_i = 1 - (N_c - F_i) / (N_c + B_i), J_0 = 0: what the closed forms restate"""
    fg = np.asarray(fg, bool)
    i = np.arange(1, len(fg) + 1, dtype=np.int64)
    F = np.cumsum(fg).astype(np.int64)
    J = 1.0 - (Nc - F).astype(np.float64) / (Nc + (i - F)).astype(np.float64)
    return np.diff(np.concatenate([[0.0], J]))


def from_errors(E, labels, classes="present", ignore_index=255, values=None):
    """dict(loss, loss_c [C], coef [P][C] float64, rank [P][C] int32 (-1: invalid pixel or class outside K), N int64
    [C], K bool [C], valid).  The order from ``E`` as fp32; the summed values ``values`` (default: E) in float64."""
    E32 = np.asarray(E, np.float32)
    P, C = E32.shape
    V = E32.astype(np.float64) if values is None else np.asarray(values, np.float64)
    t = np.asarray(labels).astype(np.int64)
    valid = valid_mask(t, C, ignore_index)
    vp = np.nonzero(valid)[0]
    n = len(vp)
    N = np.array([int((t[vp] == c).sum()) for c in range(C)], np.int64)
    K = np.ones(C, bool) if classes == "all" else N > 0
    nK = int(K.sum())
    loss_c = np.zeros(C)
    coef = np.zeros((P, C))
    rank = np.full((P, C), -1, np.int32)
    for c in np.nonzero(K)[0]:
        if n == 0:
            continue
        order = np.lexsort((vp, -E32[vp, c]))
        sp = vp[order]
        fg = t[sp] == c
        g = lovasz_gradient(fg, int(N[c]))
        loss_c[c] = float(np.sum(V[sp, c] * g))
        coef[sp, c] = np.where(fg, -g, g) / nK
        rank[sp, c] = np.arange(n, dtype=np.int32)
    loss = float(loss_c[K].sum() / nK) if nK > 0 else 0.0
    return dict(loss=loss, loss_c=loss_c, coef=coef, rank=rank, N=N, K=K, valid=valid)


def softmax_errors(logits, labels, ignore_index=255):
    """(q, |y - q|) in float64; rows of invalid pixels: q as computed, errors -1"""
    x = np.asarray(logits, np.float64)
    P, C = x.shape
    t = np.asarray(labels).astype(np.int64)
    valid = valid_mask(t, C, ignore_index)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    q = e / e.sum(axis=1, keepdims=True)
    y = np.zeros((P, C))
    y[np.arange(P)[valid], t[valid]] = 1.0
    err = np.abs(y - q)
    err[~valid] = -1.0
    return q, err


def evaluate(logits, labels, classes="present", errors=None, ignore_index=255):
    """from_errors' dict plus grad [P][C] and errors (float64 |y - q|).  ``errors``: the fp32 values that fix the
    order (the device's); default: the float64 errors rounded to fp32."""
    q, err = softmax_errors(logits, labels, ignore_index)
    E = err.astype(np.float32) if errors is None else np.asarray(errors, np.float32)
    out = from_errors(E, labels, classes, ignore_index, values=err)
    G = out["coef"]
    grad = q * (G - (G * q).sum(axis=1, keepdims=True))
    grad[~out["valid"]] = 0.0
    out.update(grad=grad, errors=err, q=q)
    return out


def combined(logits, labels, weight=None, ignore_index=255, thresh=None, min_kept=0, keep_fraction=0.0,
             lovasz_weight=1.0, classes="present", errors=None, region=None, region_weight=1.0):
    """loss_ce [+ region_weight * loss_region] + lovasz_weight * loss_lovasz in float64: dict(loss, grad, ce, lovasz,
    region (None without one))"""
    ce = CE.cross_entropy_select(logits, labels, weight, ignore_index, thresh, min_kept, keep_fraction)
    lv = evaluate(logits, labels, classes, errors, ignore_index)
    loss = ce["loss"] + lovasz_weight * lv["loss"]
    grad = ce["grad"] + lovasz_weight * lv["grad"]
    rg = None
    if region is not None:
        import _region_loss_ref as R

        rg = R.evaluate(logits, labels, region, 1.0, "present", ignore_index)
        loss = loss + region_weight * rg["loss"]
        grad = grad + region_weight * rg["grad"]
    return dict(loss=loss, grad=grad, ce=ce, lovasz=lv, region=rg)
