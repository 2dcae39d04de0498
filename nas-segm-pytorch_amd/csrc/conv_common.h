// Shared pieces of the dense-convolution kernels (conv_fwd.hip, conv_wgrad.hip):
// implicit-GEMM geometry (the fp32 MFMA wrapper mfma16 and keep_if are lane_math.h's).
//
// Code-generation rules learned on gfx950 / hipcc 7.2 and followed throughout:
//  * never put a global load under a data-dependent branch: the compiler closes every
//    such block with s_waitcnt vmcnt(0), which serialises the loop on HBM latency.
//    Load from a clamped (always valid) address and zero the value with a bit mask.
//  * run-time mode flags inside hot loops become branches; make them template
//    parameters or hoist them out of the loop.
#pragma once
#include "common.h"

struct ConvGeom {
  int B, Hs, Ws;  // source (tensor being read) dims
  int Ho, Wo;     // destination dims
  int kh, kw, stride, pad, dil, transposed;
};

// source pixel index for destination pixel (b,oy,ox) and tap (ty,tx);
// -1 when the tap falls outside / on a stride hole.
__device__ __forceinline__ int src_pixel(const ConvGeom& g, int b, int oy, int ox, int ty, int tx) {
  int iy, ix;
  if (!g.transposed) {
    iy = oy * g.stride - g.pad + ty * g.dil;
    ix = ox * g.stride - g.pad + tx * g.dil;
    if (iy < 0 || iy >= g.Hs || ix < 0 || ix >= g.Ws) return -1;
  } else {
    const int ny = oy + g.pad - ty * g.dil;
    const int nx = ox + g.pad - tx * g.dil;
    if (ny < 0 || nx < 0) return -1;
    if (g.stride > 1) {
      if ((ny % g.stride) || (nx % g.stride)) return -1;
      iy = ny / g.stride;
      ix = nx / g.stride;
    } else {
      iy = ny;
      ix = nx;
    }
    if (iy >= g.Hs || ix >= g.Ws) return -1;
  }
  return (b * g.Hs + iy) * g.Ws + ix;
}
