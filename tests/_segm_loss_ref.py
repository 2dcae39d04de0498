"""Float64 host restatement of the class-weighted, hard-example-mined cross-entropy (csrc/loss.hip:
nasseg_ce_sel_fwd / _bwd, nasseg_ohem_threshold; F.cross_entropy_select; INTEGRATION.md, "Losses").

logits [P][C], labels [P], optional weights [C].  Pixel p is valid iff its label t != ignore_index and 0 <= t < C;
l_p = logsumexp(x_p) - x_p[t].  Selection is active iff thresh is given or min_kept > 0 or keep_fraction > 0:
n = valid pixels, k = min(n, max(min_kept, ceil(keep_fraction * n))), tau = min(float32(-log(thresh)) or +inf, k-th
largest l_p); a valid pixel is kept iff l_p >= tau (ties at tau are all kept); inactive: every valid pixel is kept.
loss = sum_kept w[t] l_p / sum_kept w[t]; gradient (tau and the kept set constant) =
w[t] (softmax(x_p) - onehot(t)) / sum_kept w on kept pixels, 0 elsewhere.  Selection never looks at the weights."""
import math

import numpy as np


def t_loss_of(thresh):
    """the threshold on the loss axis, as the product computes it: float32(-log(thresh)), +inf without thresh"""
    return np.float32(np.inf) if thresh is None else np.float32(-np.log(np.float64(thresh)))


def select_k(n, min_kept, keep_fraction):
    return min(int(n), max(int(min_kept), int(math.ceil(float(keep_fraction) * float(n)))))


def pixel_losses(logits, labels, ignore_index=255):
    """(l [P] float64 with -1 on invalid pixels, valid [P] bool, softmax [P][C] float64)"""
    x = np.asarray(logits, np.float64)
    t = np.asarray(labels).astype(np.int64)
    P, C = x.shape
    valid = (t != ignore_index) & (t >= 0) & (t < C)
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    s = e.sum(axis=1, keepdims=True)
    lse = (m + np.log(s))[:, 0]
    tt = np.where(valid, t, 0)
    l = np.where(valid, lse - x[np.arange(P), tt], -1.0)
    return l, valid, e / s


def threshold(values, t_loss, min_kept, keep_fraction):
    """(tau, k, n, n_kept) over the entries of ``values`` that are >= 0, in the dtype of ``values``: np.sort on the
    same array is the whole statement"""
    v = np.asarray(values).reshape(-1)
    part = v[v >= 0]
    n = int(part.size)
    k = select_k(n, min_kept, keep_fraction)
    if n == 0:
        return v.dtype.type(t_loss), 0, 0, 0
    lk = np.sort(part)[n - k]
    tau = min(v.dtype.type(t_loss), lk)
    return tau, k, n, int((part >= tau).sum())


def cross_entropy_select(logits, labels, weight=None, ignore_index=255, thresh=None, min_kept=0, keep_fraction=0.0):
    """dict(loss, grad [P][C], pixel_loss, kept [P] bool, tau, k, n, n_kept, sum_w) in float64"""
    x = np.asarray(logits, np.float64)
    t = np.asarray(labels).astype(np.int64)
    P, C = x.shape
    l, valid, sm = pixel_losses(x, t, ignore_index)
    w = np.ones(C, np.float64) if weight is None else np.asarray(weight, np.float64)
    active = thresh is not None or min_kept > 0 or keep_fraction > 0
    n = int(valid.sum())
    if active:
        if min_kept < 1:
            raise ValueError("selection needs min_kept >= 1")
        tau, k, n, _ = threshold(l, np.float64(t_loss_of(thresh)), min_kept, keep_fraction)
        kept = valid & (l >= tau)
    else:
        tau, k, kept = -np.inf, n, valid
    tt = np.where(valid, t, 0)
    wp = np.where(kept, w[tt], 0.0)
    sum_w = wp.sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = (wp * np.where(kept, l, 0.0)).sum() / sum_w
        onehot = np.zeros((P, C), np.float64)
        onehot[np.arange(P), tt] = 1.0
        grad = (wp / sum_w)[:, None] * (sm - onehot)
    grad[~kept] = 0.0
    return dict(loss=loss, grad=grad, pixel_loss=l, kept=kept, tau=tau, k=k, n=n, n_kept=int(kept.sum()),
                sum_w=sum_w)


def gap_to_tau(ref):
    """the smallest distance to tau of a valid loss that does not equal it (inf when there is none): a selection
    on fp32 losses can only be compared with this one when that gap is far above the fp32 error of a loss"""
    l = ref["pixel_loss"]
    d = np.abs(l[(l >= 0) & (l != ref["tau"])] - ref["tau"])
    return float(d.min()) if d.size else float("inf")
