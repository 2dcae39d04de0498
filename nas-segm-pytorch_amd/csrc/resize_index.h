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

// torch 'nearest': src = min(floor(dst * scale), in-1), scale = in/out (fp32)
__device__ __forceinline__ int nearest_src(int dst, float scale, int in_size) {
  int i = (int)floorf((float)dst * scale);
  if (i > in_size - 1) i = in_size - 1;
  return i;
}
