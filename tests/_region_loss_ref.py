"""Float64 host restatement of the region-overlap term (soft Jaccard / Dice / Tversky) of the segmentation criterion
(csrc/loss.hip: nasseg_ce_region_fwd / _bwd; F.region_overlap_loss, F.cross_entropy_select(region=...);
INTEGRATION.md, "Losses").

logits [P][C], labels [P].  Pixel p is valid iff its label t != ignore_index and 0 <= t < C; q_p = softmax(x_p),
y_pc = [t_p == c].  Over the valid pixels: I_c = sum q_pc y_pc, S_c = sum q_pc, N_c = sum y_pc;
D_c = (1 - a - b) I_c + a S_c + b N_c + s, T_c = (I_c + s) / D_c; K = the classes with N_c > 0 (classes="all": every
class); loss = 1 - mean_{c in K} T_c, exactly 0 with a zero gradient when K is empty.
Gradient: a_c = (D_c - (I_c + s)(1 - a - b)) / D_c^2, b_c = -(I_c + s) a / D_c^2, G_pc = -(a_c y_pc + b_c) / |K| for
c in K (0 otherwise); dloss/dx_pj = q_pj (G_pj - sum_c G_pc q_pc) on valid pixels, 0 on all others.
``evaluate(..., dtype=np.float32)`` is the same sequence of formulas in fp32 numpy: what plain fp32 rounding costs,
used only to calibrate one bound of tests/test_hip_region_loss.py."""
import numpy as np

import _segm_loss_ref as CE

# the four parameter sets of the tests: (region, smooth, classes)
PARAM_SETS = [("jaccard", 1.0, "present"), ("dice", 0.0, "present"), (("tversky", 0.3, 0.7), 1.0, "all"),
              (("tversky", 0.7, 0.3), 1e-3, "present")]


def alpha_beta(region):
    if region == "jaccard":
        return 1.0, 1.0
    if region == "dice":
        return 0.5, 0.5
    name, a, b = region
    assert name == "tversky"
    return float(a), float(b)


def evaluate(logits, labels, region="jaccard", smooth=1.0, classes="present", ignore_index=255, dtype=np.float64):
    """dict(loss, grad [P][C], I, S, N (int64), K (bool [C]), valid [P] bool), every float in ``dtype``"""
    f = dtype
    x = np.asarray(logits, f)
    t = np.asarray(labels).astype(np.int64)
    P, C = x.shape
    a, b = alpha_beta(region)
    a, b, s = f(a), f(b), f(smooth)
    valid = (t != ignore_index) & (t >= 0) & (t < C)
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    q = e / e.sum(axis=1, keepdims=True, dtype=f)
    tt = np.where(valid, t, 0)
    y = np.zeros((P, C), f)
    y[np.arange(P), tt] = 1
    y[~valid] = 0
    qv = np.where(valid[:, None], q, f(0))
    I = (qv * y).sum(axis=0, dtype=f)
    S = qv.sum(axis=0, dtype=f)
    N = y.sum(axis=0).astype(np.int64)
    K = np.ones(C, bool) if classes == "all" else N > 0
    nK = int(K.sum())
    grad = np.zeros((P, C), f)
    if nK == 0:
        return dict(loss=f(0), grad=grad, I=I, S=S, N=N, K=K, valid=valid)
    gam = f(1) - a - b
    with np.errstate(invalid="ignore", divide="ignore"):
        D = gam * I + a * S + b * N.astype(f) + s
        T = (I + s) / D
        ac = (D - (I + s) * gam) / (D * D)
        bc = -(I + s) * a / (D * D)
    loss = f(1) - T[K].sum(dtype=f) / f(nK)
    ac = np.where(K, ac, f(0))
    bc = np.where(K, bc, f(0))
    G = -(ac[None, :] * y + bc[None, :]) / f(nK)
    grad = qv * (G - (G * qv).sum(axis=1, keepdims=True, dtype=f))
    grad[~valid] = 0
    return dict(loss=f(loss), grad=grad.astype(f), I=I, S=S, N=N, K=K, valid=valid)


def combined(logits, labels, weight=None, ignore_index=255, thresh=None, min_kept=0, keep_fraction=0.0,
             region="jaccard", region_weight=1.0, smooth=1.0, classes="present"):
    """loss_ce + region_weight * loss_region in float64: dict(loss, grad, ce (CE.cross_entropy_select's dict),
    region (evaluate's dict))"""
    ce = CE.cross_entropy_select(logits, labels, weight, ignore_index, thresh, min_kept, keep_fraction)
    rg = evaluate(logits, labels, region, smooth, classes, ignore_index)
    return dict(loss=ce["loss"] + region_weight * rg["loss"], grad=ce["grad"] + region_weight * rg["grad"], ce=ce,
                region=rg)


def drop_odd_classes(labels, ignore_index=255):
    """every odd label moved to the even class below it: about half of the classes are absent"""
    t = np.asarray(labels).copy()
    odd = (t != ignore_index) & (t % 2 == 1)
    t[odd] -= 1
    return t
