// Source indices and weights of the resizes, shared by every kernel that samples a map at another size
// (resize.hip, miou.hip, loss.hip, depth_eval.hip): one definition, so that a fused kernel addresses exactly the
// pixel the stand-alone resize would have written.
#pragma once
#include "common.h"

struct Lin {
  int i0, i1;
  float l0, l1;
};
// bilinear, align_corners=False - torch's area_pixel_compute_source_index:
//   scale = in/out (fp32); src = max(scale*(dst+0.5)-0.5, 0); i0 = floor(src); i1 = i0 + (i0 < in-1);
//   l1 = src - i0; l0 = 1 - l1.  Equal sizes are the identity (weights 1 and 0).
__device__ __forceinline__ Lin lin_coeff(int dst, float scale, int in_size, int out_size) {
  Lin r;
  if (in_size == out_size) {
    r.i0 = r.i1 = dst;
    r.l0 = 1.f;
    r.l1 = 0.f;
    return r;
  }
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  r.i0 = (int)src;
  if (r.i0 > in_size - 1) r.i0 = in_size - 1;
  r.i1 = r.i0 + ((r.i0 < in_size - 1) ? 1 : 0);
  float l1 = src - (float)r.i0;
  l1 = fminf(fmaxf(l1, 0.f), 1.f);
  r.l1 = l1;
  r.l0 = 1.f - l1;
  return r;
}

// The resize itself: the four taps blended with contraction left to the compiler (resize.hip, ensemble.hip)
__device__ __forceinline__ float bilerp(float v00, float v01, float v10, float v11, const Lin& ly, const Lin& lx) {
  return ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11);
}
__device__ __forceinline__ float4 bilerp4(float4 v00, float4 v01, float4 v10, float4 v11, const Lin& ly, const Lin& lx) {
  float4 o;
  o.x = bilerp(v00.x, v01.x, v10.x, v11.x, ly, lx);
  o.y = bilerp(v00.y, v01.y, v10.y, v11.y, ly, lx);
  o.z = bilerp(v00.z, v01.z, v10.z, v11.z, ly, lx);
  o.w = bilerp(v00.w, v01.w, v10.w, v11.w, ly, lx);
  return o;
}

// The fused up-sampling criteria (loss_up.hip, depth.hip): the value, and the two halves of its transpose.
// v = ly.l0 * (lx.l0 * x00 + lx.l1 * x01) + ly.l1 * (lx.l0 * x10 + lx.l1 * x11), every product and sum rounded on
// its own (csrc/miou.hip: argmax_cm_kernel; csrc/depth_eval.hip: depth_metrics_kernel)
__device__ __forceinline__ float up_interp(float x00, float x01, float x10, float x11, const Lin& ly, const Lin& lx) {
  const float top = __fadd_rn(__fmul_rn(lx.l0, x00), __fmul_rn(lx.l1, x01));
  const float bot = __fadd_rn(__fmul_rn(lx.l0, x10), __fmul_rn(lx.l1, x11));
  return __fadd_rn(__fmul_rn(ly.l0, top), __fmul_rn(ly.l1, bot));
}
// conservative range [lo, hi] of destination coordinates whose footprint can touch source index i (csrc/resize.hip's
// dst_range: a coordinate inside it that does not touch i has weight exactly 0); scale = in/out
__device__ __forceinline__ void up_dst_range(int i, float scale, int in_size, int out_size, int& lo, int& hi) {
  if (in_size == out_size) {
    lo = hi = i;
    return;
  }
  // src(o) in [i-1, i+1)  <=>  o in [(i-0.5)/scale - 0.5, (i+1.5)/scale - 0.5)
  const float inv = 1.0f / scale;
  lo = (int)floorf(((float)i - 0.5f) * inv - 0.5f) - 1;
  hi = (int)ceilf(((float)i + 1.5f) * inv - 0.5f) + 1;
  if (lo < 0) lo = 0;
  if (hi > out_size - 1) hi = out_size - 1;
}
// weight of source index i in the destination coordinate l belongs to
__device__ __forceinline__ float up_weight(const Lin& l, int i) {
  float wt = 0.f;
  if (l.i0 == i) wt += l.l0;
  if (l.i1 == i) wt += l.l1;
  return wt;
}

// torch 'nearest': src = min(floor(dst * scale), in-1), scale = in/out (fp32)
__device__ __forceinline__ int nearest_src(int dst, float scale, int in_size) {
  int i = (int)floorf((float)dst * scale);
  if (i > in_size - 1) i = in_size - 1;
  return i;
}
