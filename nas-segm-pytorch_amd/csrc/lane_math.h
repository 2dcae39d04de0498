// The per-lane algebra every fused kernel shares (included by common.h, after the load / store / fma4 helpers it is
// written in): storage rounding, activation masks, xhat, both forms of the BatchNorm backward, the masks of clamped
// loads and the fp32 MFMA wrapper.  A kernel that needs one of these calls it here and does not re-type it
// (tests/test_csrc_vocabulary.py holds the line).
#pragma once

// ---- storage rounding ----------------------------------------------------------------------------------------------
// The value a store to an activation tensor followed by a load would give back: bf16 round trip in the bf16 build,
// the identity in the fp32 build.  A fused kernel applies it to what it sums or feeds on after storing it, so that
// it sees the bits the unfused pass over the stored tensor would have read.
__device__ __forceinline__ float as_stored(float v) {
#ifdef NASSEG_BF16
  v = bf16_to_f32(f32_to_bf16(v));
#endif
  return v;
}
__device__ __forceinline__ float4 as_stored4(float4 v) {
#ifdef NASSEG_BF16
  v = make_float4(bf16_to_f32(f32_to_bf16(v.x)), bf16_to_f32(f32_to_bf16(v.y)), bf16_to_f32(f32_to_bf16(v.z)),
                  bf16_to_f32(f32_to_bf16(v.w)));
#endif
  return v;
}

// ---- masks ---------------------------------------------------------------------------------------------------------
// keep v where ok, +0.0 elsewhere, without a select the compiler could turn back into a branch around the producing
// load (mask = all ones / all zeros)
__device__ __forceinline__ float keep_if(float v, bool ok) {
  return __uint_as_float(__float_as_uint(v) & (0u - (unsigned)ok));
}
__device__ __forceinline__ float4 keep_if(float4 v, bool ok) {
  const unsigned m = 0u - (unsigned)ok;
  v.x = __uint_as_float(__float_as_uint(v.x) & m);
  v.y = __uint_as_float(__float_as_uint(v.y) & m);
  v.z = __uint_as_float(__float_as_uint(v.z) & m);
  v.w = __uint_as_float(__float_as_uint(v.w) & m);
  return v;
}
// act'(t) per component, and g * act'(t) with the activation as the loop-invariant scalars of act_sel.  (g * act'(t)
// with a run-time int is still written out where it is used: through a helper hipcc pairs the four products into
// v_pk_mul_f32 and the kernels' assembly changes - DESIGN 3.1.1.)
__device__ __forceinline__ float4 act_mask4(float4 t, int act) {
  return make_float4(act_mask(t.x, act), act_mask(t.y, act), act_mask(t.z, act), act_mask(t.w, act));
}
__device__ __forceinline__ float4 mask4(float4 g, float4 t, const ActSel& act) {
  return make_float4(g.x * act_mask(t.x, act), g.y * act_mask(t.y, act), g.z * act_mask(t.z, act),
                     g.w * act_mask(t.w, act));
}

// ---- BatchNorm backward ----------------------------------------------------------------------------------------------
// xhat = (z - mean) * invstd
__device__ __forceinline__ float4 xhat4(float4 z, float4 mu, float4 is) {
  return make_float4((z.x - mu.x) * is.x, (z.y - mu.y) * is.y, (z.z - mu.z) * is.z, (z.w - mu.w) * is.w);
}
// direct form, before the multiplication by scale: d - s0/M - xhat*s1/M (s0 = sum g, s1 = sum g*xhat)
__device__ __forceinline__ float4 bn_dx4(float4 d, float4 x, float4 mu, float4 is, float4 s0, float4 s1, float invM) {
  return make_float4(d.x - s0.x * invM - (x.x - mu.x) * is.x * s1.x * invM,
                     d.y - s0.y * invM - (x.y - mu.y) * is.y * s1.y * invM,
                     d.z - s0.z * invM - (x.z - mu.z) * is.z * s1.z * invM,
                     d.w - s0.w * invM - (x.w - mu.w) * is.w * s1.w * invM);
}

// fp32 MFMA: c += a (x) b over a 16 x 16 tile, 4 k-steps across the lane groups
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Coefficient form, for a kernel that turns g into dz on load: dz = ca*g' + cb*z + cd == scale*(g' - sum(g')/M -
// xhat*sum(g'*xhat)/M) with g' = g * act'(scale*z + shift) when g arrives without its activation mask (act != 0;
// cs = shift is loaded only then).  eval (train == 0): dz = scale * g'.
struct BnCoef {
  float4 ca, cb, cd, cs;
};
__device__ __forceinline__ BnCoef bn_coef(const float* scale, const float* shift, const float* mean,
                                          const float* invstd, const float* sums, int C, float invM, int train,
                                          int act, int c4) {
  BnCoef k;
  k.ca = lda4(scale + c4 * 4);
  k.cs = act ? lda4(shift + c4 * 4) : f4zero();
  k.cb = f4zero();
  k.cd = f4zero();
  if (train) {
    const float4 is = lda4(invstd + c4 * 4), mu = lda4(mean + c4 * 4);
    const float4 s0 = lda4(sums + c4 * 4), s1 = lda4(sums + C + c4 * 4);
    const float m = invM;
    k.cb = make_float4(-k.ca.x * is.x * (s1.x * m), -k.ca.y * is.y * (s1.y * m), -k.ca.z * is.z * (s1.z * m),
                       -k.ca.w * is.w * (s1.w * m));
    k.cd = make_float4(k.ca.x * (mu.x * is.x * (s1.x * m) - s0.x * m), k.ca.y * (mu.y * is.y * (s1.y * m) - s0.y * m),
                       k.ca.z * (mu.z * is.z * (s1.z * m) - s0.z * m), k.ca.w * (mu.w * is.w * (s1.w * m) - s0.w * m));
  }
  return k;
}
// the consumer: mask (a select per component), the two fused multiply-adds, and the rounding of the store the
// two-kernel form would have made
__device__ __forceinline__ float4 bn_coef_apply(float4 g, float4 z, const BnCoef& k, const ActSel& act) {
  g = mask4(g, fma4(z, k.ca, k.cs), act);
  return as_stored4(fma4(g, k.ca, fma4(z, k.cb, k.cd)));
}
// what a kernel that makes dz on load keeps of an output pixel between issuing its loads (unconditional, from a clamped
// address) and the arithmetic: g, z and whether the pixel is inside the map
struct DzRaw {
  float4 g, z;
  bool ok;
};
