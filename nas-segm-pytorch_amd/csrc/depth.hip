// Masked berHu (reverse Huber) loss of the depth head against a FULL-SIZE target with holes, gfx950.
//
// Not present in the reference (its depth networks are inference only; "parity unpinned"): the loss of
// nasseg_berhu_fwd (loss.hip; Laina et al. 2016, eq. 2) as a depth data set needs it -
//   * the target is the ground-truth map [B][H][W], fp32 whatever the prediction's storage, at the IMAGE's size;
//     prediction pixel (y, x) of the [B][h][w] map is compared with target[b][sy][sx], (sy, sx) = the source index
//     of F.interpolate(mode="nearest") (nearest_src, resize_index.h) - the resized target is never written;
//   * a pixel counts iff its target t is finite and valid_min < t <= valid_max (0 / NaN / inf mark holes);
//   * d = |pred - t| over valid pixels, c = 0.2 * max d, loss = sum B(d) / n_valid,
//     B(d) = d if d <= c else (d^2 + c^2) / (2c); c is a constant in the backward pass;
//   * no valid pixel: loss 0, gradient 0.  n_valid never leaves the device.
// Three passes over the prediction (workgroup maxima + counts -> c -> workgroup sums -> one fixed-order sum in
// double) and one for the gradient; no float atomics, so the same inputs give the same bits.
#include <math.h>

#include "common.h"
#include "resize_index.h"

namespace {

constexpr int kMaxGrid = 1024;  // workgroups of the reductions: ws = [1024] maxima | [1024] counts | [1024] sums

struct MaskedGeom {
  int h, w, H, W;
  float sh, sw, vmin, vmax;
};

__device__ __forceinline__ bool depth_valid(float t, float vmin, float vmax) {
  const bool finite = (__float_as_uint(t) & 0x7f800000u) != 0x7f800000u;
  return finite && t > vmin && t <= vmax;
}

// target of prediction element i of the dense [B][h][w] map
__device__ __forceinline__ float masked_target(const float* __restrict__ target, int64_t i, const MaskedGeom& g) {
  const int x = (int)(i % g.w);
  const int64_t r = i / g.w;
  const int y = (int)(r % g.h);
  const int64_t b = r / g.h;
  const int sy = nearest_src(y, g.sh, g.H);
  const int sx = nearest_src(x, g.sw, g.W);
  return target[(b * g.H + sy) * g.W + sx];
}

__global__ __launch_bounds__(256) void berhu_masked_max_kernel(const act_t* __restrict__ pred,
                                                               const float* __restrict__ target, int64_t n,
                                                               MaskedGeom g, float* __restrict__ maxpart,
                                                               float* __restrict__ cntpart) {
  __shared__ float red_m[256];
  __shared__ float red_n[256];
  float m = 0.f, cnt = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float t = masked_target(target, i, g);
    if (!depth_valid(t, g.vmin, g.vmax)) continue;
    m = fmaxf(m, fabsf(lda1(pred + i) - t));
    cnt += 1.f;  // (at most n / gridDim.x + 256 < 2^24 per workgroup: exact in fp32)
  }
  red_m[threadIdx.x] = m;
  red_n[threadIdx.x] = cnt;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red_m[threadIdx.x] = fmaxf(red_m[threadIdx.x], red_m[threadIdx.x + s]);
      red_n[threadIdx.x] += red_n[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    maxpart[blockIdx.x] = red_m[0];
    cntpart[blockIdx.x] = red_n[0];
  }
}

__global__ __launch_bounds__(256) void berhu_masked_sum_kernel(const act_t* __restrict__ pred,
                                                               const float* __restrict__ target, int64_t n,
                                                               MaskedGeom g, const float* __restrict__ maxpart,
                                                               int nblk, float* __restrict__ sumpart,
                                                               float* __restrict__ out) {
  __shared__ float red[256];
  float m = 0.f;
  for (int b = threadIdx.x; b < nblk; b += 256) m = fmaxf(m, maxpart[b]);  // (a maximum: any order, same bits)
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  const float c = 0.2f * red[0];
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) out[1] = c;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float t = masked_target(target, i, g);
    if (!depth_valid(t, g.vmin, g.vmax)) continue;
    const float d = fabsf(lda1(pred + i) - t);
    acc += (d <= c) ? d : (d * d + c * c) / (2.f * c);
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) sumpart[blockIdx.x] = red[0];
}

// out[0] = sum / n_valid (0 without a valid pixel), out[2] = n_valid.  One workgroup: thread t adds the partials of
// workgroups t, t+256, ... in fp64, then a fixed-order tree through LDS.
__global__ __launch_bounds__(256) void berhu_masked_finalize_kernel(const float* __restrict__ sumpart,
                                                                    const float* __restrict__ cntpart, int nblk,
                                                                    float* __restrict__ out) {
  __shared__ double red_s[256];
  __shared__ double red_n[256];
  double s = 0.0, n = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) {
    s += (double)sumpart[b];
    n += (double)cntpart[b];
  }
  red_s[threadIdx.x] = s;
  red_n[threadIdx.x] = n;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) {
      red_s[threadIdx.x] += red_s[threadIdx.x + k];
      red_n[threadIdx.x] += red_n[threadIdx.x + k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = red_n[0] > 0.0 ? (float)(red_s[0] / red_n[0]) : 0.f;
    out[2] = (float)red_n[0];
  }
}

// dpred = g / n_valid * (sign(diff) if |diff| <= c else diff / c) on valid pixels, exactly 0 elsewhere
__global__ __launch_bounds__(256) void berhu_masked_bwd_kernel(const act_t* __restrict__ pred,
                                                               const float* __restrict__ target,
                                                               const float* __restrict__ stats,
                                                               const float* __restrict__ gscale, int64_t n,
                                                               MaskedGeom g, act_t* __restrict__ dpred) {
  const float c = stats[1];
  const float nv = stats[2];
  const float gn = nv > 0.f ? (gscale ? gscale[0] : 1.f) / nv : 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float t = masked_target(target, i, g);
    float r = 0.f;
    if (depth_valid(t, g.vmin, g.vmax)) {
      const float d = lda1(pred + i) - t;
      const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
      r = gn * ((fabsf(d) <= c) ? sgn : d / c);
    }
    sta1(dpred + i, r);
  }
}

inline int red_grid(int64_t n) {
  int64_t b = (n + 255) / 256;
  if (b > kMaxGrid) b = kMaxGrid;
  if (b < 1) b = 1;
  return (int)b;
}

inline bool masked_geom(int B, int h, int w, int H, int W, float valid_min, float valid_max, MaskedGeom* g) {
  if (!(B > 0 && h > 0 && w > 0 && H > 0 && W > 0)) return false;
  g->h = h, g->w = w, g->H = H, g->W = W;
  g->sh = (float)H / (float)h, g->sw = (float)W / (float)w;
  g->vmin = valid_min, g->vmax = valid_max;
  return true;
}

}  // namespace

extern "C" {

#if NASSEG_FP32_ONLY
int64_t nasseg_berhu_masked_workspace(void) { return 3 * kMaxGrid; }
#endif

// pred: dense [B][h][w] (one channel), target: fp32 [B][H][W].  out[0] = loss, out[1] = c, out[2] = n_valid.
// ws: nasseg_berhu_masked_workspace() floats.
int NASSEG_FN(berhu_masked_fwd)(const act_t* pred, const float* target, int B, int h, int w, int H, int W,
                                float valid_min, float valid_max, float* out, float* ws, void* stream) {
  MaskedGeom g;
  NASSEG_REQUIRE(masked_geom(B, h, w, H, W, valid_min, valid_max, &g), "berhu_masked_fwd: bad shape");
  NASSEG_REQUIRE(pred && target && out && ws, "berhu_masked_fwd: null pointer");
  NASSEG_REQUIRE(valid_min == valid_min && valid_max == valid_max, "berhu_masked_fwd: NaN bound");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)B * h * w;
  const int grid = red_grid(n);
  float* maxpart = ws;
  float* cntpart = ws + kMaxGrid;
  float* sumpart = ws + 2 * kMaxGrid;
  hipLaunchKernelGGL(berhu_masked_max_kernel, dim3(grid), dim3(256), 0, s, pred, target, n, g, maxpart, cntpart);
  NASSEG_LAUNCH_CHECK("berhu_masked_max");
  hipLaunchKernelGGL(berhu_masked_sum_kernel, dim3(grid), dim3(256), 0, s, pred, target, n, g, maxpart, grid,
                     sumpart, out);
  NASSEG_LAUNCH_CHECK("berhu_masked_sum");
  hipLaunchKernelGGL(berhu_masked_finalize_kernel, dim3(1), dim3(256), 0, s, sumpart, cntpart, grid, out);
  NASSEG_LAUNCH_CHECK("berhu_masked_finalize");
  return NASSEG_OK;
}

// stats = out of nasseg_berhu_masked_fwd; gscale = device scalar upstream gradient (null = 1)
int NASSEG_FN(berhu_masked_bwd)(const act_t* pred, const float* target, const float* stats, const float* gscale,
                                int B, int h, int w, int H, int W, float valid_min, float valid_max, act_t* dpred,
                                void* stream) {
  MaskedGeom g;
  NASSEG_REQUIRE(masked_geom(B, h, w, H, W, valid_min, valid_max, &g), "berhu_masked_bwd: bad shape");
  NASSEG_REQUIRE(pred && target && stats && dpred, "berhu_masked_bwd: null pointer");
  const int64_t n = (int64_t)B * h * w;
  hipLaunchKernelGGL(berhu_masked_bwd_kernel, dim3(red_grid(n) * 2), dim3(256), 0, (hipStream_t)stream, pred,
                     target, stats, gscale, n, g, dpred);
  NASSEG_LAUNCH_CHECK("berhu_masked_bwd");
  return NASSEG_OK;
}

}  // extern "C"
