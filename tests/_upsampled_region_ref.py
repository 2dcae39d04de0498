"""Float64 host restatement of the region-overlap term taken at the labels' size, alone or on top of the full-size
cross-entropy (csrc/loss_up.hip: nasseg_ce_up_region_fwd / _bwd; F.cross_entropy_upsampled(region=...),
F.region_overlap_loss_upsampled; INTEGRATION.md, "Losses").

Nothing new is defined here - the existing restatements are composed:
  v      = _upsampled_ce_ref.interpolate(x) with the kernel's fp32 coefficients (_upsampled_ce_ref.coeffs)
  region = _region_loss_ref.evaluate(v, t, ...) over the B*H*W rows v: I, S, N, K, the loss and its gradient g [P][C]
  grad   = _upsampled_ce_ref.gather(g) with the two weight matrices: the gradient with respect to the stored logits
  sum    = the dict of _upsampled_ce_ref.upsampled (the cross-entropy) + region_weight * the above.
``upsampled_region_fp32`` is the same sequence in plain float32 numpy on a given kept set: what fp32 arithmetic costs
on an input, to size the bounds of tests/test_hip_upsampled_region.py with."""
import numpy as np

import _region_loss_ref as R
import _upsampled_ce_ref as U


def region_term(x, t, region="jaccard", smooth=1.0, classes="present", ignore_index=255, dtype=np.float64,
                coeff_dtype=np.float32):
    """the term alone: _region_loss_ref.evaluate's dict over the interpolated rows, with ``grad`` [B][h][w][C] gathered
    into the logits' shape, everything after the coefficients in ``dtype``"""
    x = np.asarray(x, dtype)
    t = np.asarray(t)
    B, h, w, C = x.shape
    _, H, W = t.shape
    cy, cx = U.coeffs(H, h, coeff_dtype), U.coeffs(W, w, coeff_dtype)
    v = U.interpolate(x, cy, cx, dtype)
    rg = R.evaluate(v.reshape(-1, C), t.reshape(-1), region, smooth, classes, ignore_index, dtype)
    out = dict(rg)
    out["grad"] = U.gather(rg["grad"].reshape(B, H, W, C).astype(dtype), U.weight_matrix(cy, h), U.weight_matrix(cx, w))
    out["v"] = v
    return out


def upsampled_region(x, t, weight=None, ignore_index=255, thresh=None, min_kept=0, keep_fraction=0.0,
                     region="jaccard", region_weight=1.0, smooth=1.0, classes="present", with_ce=True,
                     coeff_dtype=np.float32):
    """dict(loss, grad [B][h][w][C], loss_ce, loss_region, I, S, N, K, region: region_term's dict, ce:
    _upsampled_ce_ref.upsampled's dict or None, kept [B][H][W]) in float64.  ``with_ce=False``: the term alone,
    loss = region_weight * loss_region."""
    x = np.asarray(x, np.float64)
    rg = region_term(x, t, region, smooth, classes, ignore_index, np.float64, coeff_dtype)
    loss, grad, ce = region_weight * float(rg["loss"]), region_weight * rg["grad"], None
    kept = rg["valid"].reshape(np.asarray(t).shape)
    if with_ce:
        ce = U.upsampled(x, t, weight, ignore_index, thresh, min_kept, keep_fraction, coeff_dtype)
        loss, grad, kept = ce["loss"] + loss, ce["grad"] + grad, ce["kept"]
    return dict(loss=loss, grad=grad, loss_ce=None if ce is None else ce["loss"], loss_region=float(rg["loss"]),
                I=rg["I"], S=rg["S"], N=rg["N"], K=rg["K"], region=rg, ce=ce, kept=kept)


def upsampled_region_fp32(x, t, kept, weight=None, region="jaccard", region_weight=1.0, smooth=1.0, classes="present",
                          with_ce=True, ignore_index=255):
    """dict(loss, grad, loss_ce, loss_region, I, S) of the same formulas in plain float32 numpy, the cross-entropy on the
    kept set ``kept`` [B][H][W] (the float64 one: a selection is not what this sizes)"""
    f = np.float32
    rg = region_term(np.asarray(x, f), t, region, smooth, classes, ignore_index, f)
    loss, grad, loss_ce = f(region_weight) * f(rg["loss"]), (f(region_weight) * rg["grad"]).astype(np.float64), None
    if with_ce:
        loss_ce, gce, _ = U.upsampled_fp32(x, t, kept, weight)
        loss = f(f(loss_ce) + loss)
        grad = (gce.astype(f) + grad.astype(f)).astype(np.float64)
    return dict(loss=float(loss), grad=grad, loss_ce=loss_ce, loss_region=float(rg["loss"]),
                I=rg["I"].astype(np.float64), S=rg["S"].astype(np.float64))
