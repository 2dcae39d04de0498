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
// Second half of the file: the criterion at the target's size, the bilinear up-sampling of the prediction fused in
// (nasseg_berhu_up_fwd / _bwd).
// Every pass exists once, as a template on whether a ROW TABLE is present (nasseg_berhu_*_rows_*): image b of the
// prediction is then compared with image rows[b] of a larger target - the task0 depth cache - instead of image b;
// only the address of an image's target differs, so both forms give the same bits and the batch's targets are
// never gathered into a copy.
#include <math.h>

#include "common.h"
#include "resize_index.h"

namespace {

constexpr int kMaxGrid = 1024;  // workgroups of the reductions: ws = [1024] maxima | [1024] counts | [1024] sums

struct MaskedGeom {
  int h, w, H, W;
  float sh, sw, vmin, vmax;
};

// kRows false: image b of the target is image b, the table is empty - the kernels the un-indexed entry points launch
// carry nothing for it.  kRows true: the target is a cache [n_rows][H][W] and image b is its row rows[b], clamped to
// the cache as nasseg_gather_rows clamps it (a memory-safety net: the host checks).
template <bool kRows>
struct RowTable {
  const int64_t* rows;
  int64_t n_rows;
};
template <>
struct RowTable<false> {};

__device__ __forceinline__ const float* target_image(const float* __restrict__ target, const RowTable<true>& rt,
                                                     int64_t b, int64_t HW) {
  int64_t r = rt.rows[b];
  r = r < 0 ? 0 : (r >= rt.n_rows ? rt.n_rows - 1 : r);
  return target + r * HW;  // (64-bit: the cache may hold more than 2^32 elements)
}

__device__ __forceinline__ bool depth_valid(float t, float vmin, float vmax) {
  const bool finite = (__float_as_uint(t) & 0x7f800000u) != 0x7f800000u;
  return finite && t > vmin && t <= vmax;
}

// target of prediction element i of the dense [B][h][w] map
template <bool kRows>
__device__ __forceinline__ float masked_target(const float* __restrict__ target, const RowTable<kRows>& rt, int64_t i,
                                               const MaskedGeom& g) {
  const int x = (int)(i % g.w);
  const int64_t r = i / g.w;
  const int y = (int)(r % g.h);
  const int64_t b = r / g.h;
  const int sy = nearest_src(y, g.sh, g.H);
  const int sx = nearest_src(x, g.sw, g.W);
  if constexpr (!kRows) {
    return target[(b * g.H + sy) * g.W + sx];
  } else {
    return target_image(target, rt, b, (int64_t)g.H * g.W)[(int64_t)sy * g.W + sx];
  }
}

template <bool kRows>
__global__ __launch_bounds__(256) void berhu_masked_max_kernel(const act_t* __restrict__ pred,
                                                               const float* __restrict__ target, RowTable<kRows> rt,
                                                               int64_t n, MaskedGeom g, float* __restrict__ maxpart,
                                                               float* __restrict__ cntpart) {
  __shared__ float red_m[256];
  __shared__ float red_n[256];
  float m = 0.f, cnt = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float t = masked_target<kRows>(target, rt, i, g);
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

template <bool kRows>
__global__ __launch_bounds__(256) void berhu_masked_sum_kernel(const act_t* __restrict__ pred,
                                                               const float* __restrict__ target, RowTable<kRows> rt,
                                                               int64_t n, MaskedGeom g,
                                                               const float* __restrict__ maxpart,
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
    const float t = masked_target<kRows>(target, rt, i, g);
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

// dB/dd of the berHu at d = pred - t, c constant: sign(d) if |d| <= c else d / c.  The one statement of the formula
// at the prediction's size: berhu_masked_bwd_kernel and depth_terms_bwd_kernel both call it.
__device__ __forceinline__ float berhu_slope(float d, float c) {
  const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  return (fabsf(d) <= c) ? sgn : d / c;
}

// dpred = g / n_valid * (sign(diff) if |diff| <= c else diff / c) on valid pixels, exactly 0 elsewhere
template <bool kRows>
__global__ __launch_bounds__(256) void berhu_masked_bwd_kernel(const act_t* __restrict__ pred,
                                                               const float* __restrict__ target, RowTable<kRows> rt,
                                                               const float* __restrict__ stats,
                                                               const float* __restrict__ gscale, int64_t n,
                                                               MaskedGeom g, act_t* __restrict__ dpred) {
  const float c = stats[1];
  const float nv = stats[2];
  const float gn = nv > 0.f ? (gscale ? gscale[0] : 1.f) / nv : 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float t = masked_target<kRows>(target, rt, i, g);
    float r = 0.f;
    if (depth_valid(t, g.vmin, g.vmax)) {
      r = gn * berhu_slope(lda1(pred + i) - t, c);
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

// ---------------------------------------------------------------------------------------------------------------
// The same criterion taken at the TARGET's size (definition: include/nasseg.h, "full-size berHu"; INTEGRATION.md,
// "Depth"): the prediction is up-sampled bilinearly to every target pixel inside the kernels - the value
// depth_metrics_kernel (depth_eval.hip) scores, bit for bit - and never stored at that size.
//   forward   the passes above, run over the B*H*W target pixels, one lane per pixel (the target read coalesced):
//             validity first, so a hole costs one load; a valid pixel re-interpolates its value in each pass from
//             the four neighbours of the small, cache-resident prediction.  Then berhu_masked_finalize_kernel.
//   backward  a gather (as ce_up_bwd_kernel and nasseg_bilinear_bwd): a workgroup owns a T x T tile of prediction
//             pixels, stages tile + one pixel of halo in LDS, and a group of G lanes shares every pixel: the lanes
//             form a gx x gy grid that walks the pixel's target range (up_dst_range) with strides (gx, gy) - gx
//             lanes next to each other read gx consecutive targets of a row - and their partial sums are added by a
//             fixed tree through LDS.  G T T = 256; G in {1, 4, 16, 64, 256} is chosen from the shapes alone
//             (up_bwd_group): about 16 target pixels per lane, so that the x16 / x32 auxiliary heads, whose maps
//             have a few hundred pixels with footprints of thousands, still fill the device.  dpred is written once.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kUpThreads = 256;
constexpr int kUpMaxTile = 16;               // T at G = 1
constexpr int kUpPatchW = kUpMaxTile + 2;    // LDS patch: tile + halo, row stride

struct UpGeom {
  int h, w, H, W;
  float sh, sw;  // h / H, w / W: lin_coeff's scale
  float vmin, vmax;
};

// target pixel p of the dense [B][H][W] map of the BATCH (p < 2^32: up_geom) -> (b, Y, X)
__device__ __forceinline__ void up_decode(int64_t p, const UpGeom& g, uint32_t& b, int& Y, int& X) {
  const uint32_t pu = (uint32_t)p;
  const uint32_t q = pu / (uint32_t)g.W;
  X = (int)(pu - q * (uint32_t)g.W);
  b = q / (uint32_t)g.H;
  Y = (int)(q - b * (uint32_t)g.H);
}

// prediction up-sampled to target pixel (b, Y, X)
__device__ __forceinline__ float up_value(const act_t* __restrict__ pred, uint32_t b, int Y, int X, const UpGeom& g) {
  const Lin ly = lin_coeff(Y, g.sh, g.h, g.H);
  const Lin lx = lin_coeff(X, g.sw, g.w, g.W);
  const act_t* pb = pred + (int64_t)b * g.h * g.w;
  const act_t* r0 = pb + (int64_t)ly.i0 * g.w;
  const act_t* r1 = pb + (int64_t)ly.i1 * g.w;
  return up_interp(lda1(r0 + lx.i0), lda1(r0 + lx.i1), lda1(r1 + lx.i0), lda1(r1 + lx.i1), ly, lx);
}

// target pixel p of the batch: the batch's own map, or - with a row table - the pixel of the cache image its image
// selects: the 32-bit index is decoded within the batch first (into b, Y, X), the cache offset is 64-bit.  Without a
// table the caller decodes after the validity test.
template <bool kRows>
__device__ __forceinline__ float up_target(const float* __restrict__ target, const RowTable<kRows>& rt, int64_t p,
                                           const UpGeom& g, uint32_t& b, int& Y, int& X) {
  if constexpr (!kRows) {
    return target[p];
  } else {
    up_decode(p, g, b, Y, X);
    return target_image(target, rt, (int64_t)b, (int64_t)g.H * g.W)[(int64_t)Y * g.W + X];
  }
}

template <bool kRows>
__global__ __launch_bounds__(256) void berhu_up_max_kernel(const act_t* __restrict__ pred,
                                                           const float* __restrict__ target, RowTable<kRows> rt,
                                                           int64_t n, UpGeom g, float* __restrict__ maxpart,
                                                           float* __restrict__ cntpart) {
  __shared__ float red_m[256];
  __shared__ float red_n[256];
  float m = 0.f, cnt = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    uint32_t b;
    int Y, X;
    const float t = up_target<kRows>(target, rt, i, g, b, Y, X);
    if (!depth_valid(t, g.vmin, g.vmax)) continue;
    if (!kRows) up_decode(i, g, b, Y, X);  // (validity first: a hole costs one load)
    m = fmaxf(m, fabsf(up_value(pred, b, Y, X, g) - t));
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

template <bool kRows>
__global__ __launch_bounds__(256) void berhu_up_sum_kernel(const act_t* __restrict__ pred,
                                                           const float* __restrict__ target, RowTable<kRows> rt,
                                                           int64_t n, UpGeom g, const float* __restrict__ maxpart,
                                                           int nblk,
                                                           float* __restrict__ sumpart, float* __restrict__ out) {
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
    uint32_t b;
    int Y, X;
    const float t = up_target<kRows>(target, rt, i, g, b, Y, X);
    if (!depth_valid(t, g.vmin, g.vmax)) continue;
    if (!kRows) up_decode(i, g, b, Y, X);  // (validity first: a hole costs one load)
    const float d = fabsf(up_value(pred, b, Y, X, g) - t);
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

// grid: (tile x, tile y, image), flattened, x fastest.  Thread tid: pixel tid / G of the T x T tile (row-major), lane
// tid % G of its group = (lane / gx, lane % gx) of the gx x (G / gx) grid over the pixel's target range.
// dpred = gscale / n_valid * sum r Wy Wx over the valid targets of the range, r = sign(v - t) if |v - t| <= c else
// (v - t) / c; a pixel without a valid target in its range gets an exact zero.
template <bool kRows>
__global__ __launch_bounds__(256) void berhu_up_bwd_kernel(const act_t* __restrict__ pred,
                                                           const float* __restrict__ target, RowTable<kRows> rt,
                                                           const float* __restrict__ stats,
                                                           const float* __restrict__ gscale, UpGeom g, int T, int G,
                                                           int gx, int tiles_y, int tiles_x,
                                                           act_t* __restrict__ dpred) {
  __shared__ float patch[kUpPatchW * kUpPatchW];
  __shared__ float part[kUpThreads];
  const int tid = threadIdx.x;
  int wi = blockIdx.x;
  const int tx = wi % tiles_x;
  wi /= tiles_x;
  const int ty = wi % tiles_y;
  const int b = wi / tiles_y;
  const int y0 = ty * T, x0 = tx * T;
  const int ny = g.h - y0 < T ? g.h - y0 : T;  // the tile's own pixels
  const int nx = g.w - x0 < T ? g.w - x0 : T;
  const int oy = y0 > 0 ? y0 - 1 : 0, ox = x0 > 0 ? x0 - 1 : 0;  // origin of the patch: one pixel of halo, inside the map
  const int py = (y0 + ny < g.h ? y0 + ny : g.h - 1) - oy + 1;     // its rows (<= T + 2)
  const int px = (x0 + nx < g.w ? x0 + nx : g.w - 1) - ox + 1;     // its pixels per row (<= T + 2)
  for (int k = tid; k < py * px; k += kUpThreads) {
    const int r = k / px, q = k - r * px;
    patch[r * kUpPatchW + q] = lda1(pred + ((int64_t)b * g.h + oy + r) * g.w + ox + q);
  }
  __syncthreads();
  const float c = stats[1];
  const float nv = stats[2];
  const float gn = nv > 0.f ? (gscale ? gscale[0] : 1.f) / nv : 0.f;
  const int pix = tid / G, lane = tid - pix * G;
  const int iy = pix / T, jx = pix - iy * T;
  const bool own = iy < ny && jx < nx;
  const int i = y0 + iy, j = x0 + jx;
  float acc = 0.f;
  if (own) {
    const float* timg = target;  // (the image of the workgroup's b: one scalar load of the table)
    if constexpr (kRows) timg = target_image(target, rt, (int64_t)b, (int64_t)g.H * g.W);
    const int gy = G / gx;
    const int ly0 = lane / gx, lx0 = lane - ly0 * gx;
    int ylo, yhi, xlo, xhi;
    up_dst_range(i, g.sh, g.h, g.H, ylo, yhi);
    up_dst_range(j, g.sw, g.w, g.W, xlo, xhi);
    for (int Y = ylo + ly0; Y <= yhi; Y += gy) {
      const Lin ly = lin_coeff(Y, g.sh, g.h, g.H);
      const float wy = up_weight(ly, i);
      if (wy == 0.f) continue;  // (so ly.i0, ly.i1 lie in [i - 1, i + 1]: inside the patch)
      const float* r0 = patch + (ly.i0 - oy) * kUpPatchW;
      const float* r1 = patch + (ly.i1 - oy) * kUpPatchW;
      const float* trow = kRows ? timg + (int64_t)Y * g.W : target + ((int64_t)b * g.H + Y) * g.W;
      for (int X = xlo + lx0; X <= xhi; X += gx) {
        const float t = trow[X];
        if (!depth_valid(t, g.vmin, g.vmax)) continue;
        const Lin lx = lin_coeff(X, g.sw, g.w, g.W);
        const float wx = up_weight(lx, j);
        if (wx == 0.f) continue;  // (so lx.i0, lx.i1 lie in [j - 1, j + 1])
        const int a0 = lx.i0 - ox, a1 = lx.i1 - ox;
        const float d = up_interp(r0[a0], r0[a1], r1[a0], r1[a1], ly, lx) - t;
        const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        acc = fmaf(wy * wx, (fabsf(d) <= c) ? sgn : d / c, acc);
      }
    }
  }
  if (G > 1) {  // (G is the launch's: every thread of the workgroup takes the same branch)
    part[tid] = acc;
    __syncthreads();
    for (int s = G >> 1; s > 0; s >>= 1) {
      if (lane < s) part[tid] += part[tid + s];
      __syncthreads();
    }
    acc = part[tid];
  }
  if (own && lane == 0) sta1(dpred + ((int64_t)b * g.h + i) * g.w + j, gn * acc);
}

inline bool up_geom(int B, int h, int w, int H, int W, float valid_min, float valid_max, UpGeom* g) {
  if (!(B > 0 && h > 0 && w > 0 && H > 0 && W > 0)) return false;
  if ((int64_t)B * H * W >= ((int64_t)1 << 32)) return false;  // (up_value's 32-bit divisions; fp32 counts per workgroup)
  if ((int64_t)B * h * w >= ((int64_t)1 << 31)) return false;  // (the backward's grid: at most one workgroup per pixel)
  g->h = h, g->w = w, g->H = H, g->W = W;
  g->sh = (float)h / (float)H, g->sw = (float)w / (float)W;
  g->vmin = valid_min, g->vmax = valid_max;
  return true;
}

// lanes per prediction pixel in the backward: the smallest of 1, 4, 16, 64, 256 that leaves a lane at most 16 of the
// (2 H/h) x (2 W/w) target pixels a prediction pixel's weights reach (one per axis at equal size, two when
// down-sampling).  From the shapes alone.
inline int up_bwd_group(int h, int w, int H, int W) {
  const int64_t fy = H > h ? cdiv64(2 * (int64_t)H, h) : (H == h ? 1 : 2);
  const int64_t fx = W > w ? cdiv64(2 * (int64_t)W, w) : (W == w ? 1 : 2);
  int G = 1;
  while (G < kUpThreads && fy * fx > 16 * (int64_t)G) G *= 4;
  return G;
}

// ---------------------------------------------------------------------------------------------------------------
// Launches: one body per entry-point pair.  kRows false: target is the batch's own [B][H][W] map (rt unused);
// true: the cache [n_rows][H][W] and the device table of B rows.  Same geometry, same order of sums, same finalize.
// ---------------------------------------------------------------------------------------------------------------
inline bool rows_ok(const RowTable<false>&) { return true; }
inline bool rows_ok(const RowTable<true>& rt) { return rt.rows && rt.n_rows > 0; }
#define ROWS_CHECK(who) NASSEG_REQUIRE(rows_ok(rt), "%s: a row table of B entries and n_rows > 0 are expected", who)

template <bool kRows>
int masked_fwd(const char* who, const act_t* pred, const float* target, RowTable<kRows> rt, int B, int h, int w, int H,
               int W, float valid_min, float valid_max, float* out, float* ws, void* stream) {
  MaskedGeom g;
  NASSEG_REQUIRE(masked_geom(B, h, w, H, W, valid_min, valid_max, &g), "%s: bad shape", who);
  NASSEG_REQUIRE(pred && target && out && ws, "%s: null pointer", who);
  ROWS_CHECK(who);
  NASSEG_REQUIRE(valid_min == valid_min && valid_max == valid_max, "%s: NaN bound", who);
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)B * h * w;
  const int grid = red_grid(n);
  float* maxpart = ws;
  float* cntpart = ws + kMaxGrid;
  float* sumpart = ws + 2 * kMaxGrid;
  hipLaunchKernelGGL(berhu_masked_max_kernel<kRows>, dim3(grid), dim3(256), 0, s, pred, target, rt, n, g, maxpart,
                     cntpart);
  NASSEG_LAUNCH_CHECK("berhu_masked_max");
  hipLaunchKernelGGL(berhu_masked_sum_kernel<kRows>, dim3(grid), dim3(256), 0, s, pred, target, rt, n, g, maxpart,
                     grid, sumpart, out);
  NASSEG_LAUNCH_CHECK("berhu_masked_sum");
  hipLaunchKernelGGL(berhu_masked_finalize_kernel, dim3(1), dim3(256), 0, s, sumpart, cntpart, grid, out);
  NASSEG_LAUNCH_CHECK("berhu_masked_finalize");
  return NASSEG_OK;
}

template <bool kRows>
int masked_bwd(const char* who, const act_t* pred, const float* target, RowTable<kRows> rt, const float* stats,
               const float* gscale, int B, int h, int w, int H, int W, float valid_min, float valid_max, act_t* dpred,
               void* stream) {
  MaskedGeom g;
  NASSEG_REQUIRE(masked_geom(B, h, w, H, W, valid_min, valid_max, &g), "%s: bad shape", who);
  NASSEG_REQUIRE(pred && target && stats && dpred, "%s: null pointer", who);
  ROWS_CHECK(who);
  const int64_t n = (int64_t)B * h * w;
  hipLaunchKernelGGL(berhu_masked_bwd_kernel<kRows>, dim3(red_grid(n) * 2), dim3(256), 0, (hipStream_t)stream, pred,
                     target, rt, stats, gscale, n, g, dpred);
  NASSEG_LAUNCH_CHECK("berhu_masked_bwd");
  return NASSEG_OK;
}

#define UP_GEOM_CHECK(who) \
  NASSEG_REQUIRE(up_geom(B, h, w, H, W, valid_min, valid_max, &g), "%s: bad shape (B*H*W < 2^32, B*h*w < 2^31)", who)

template <bool kRows>
int up_fwd(const char* who, const act_t* pred, const float* target, RowTable<kRows> rt, int B, int h, int w, int H,
           int W, float valid_min, float valid_max, float* out, float* ws, void* stream) {
  UpGeom g;
  UP_GEOM_CHECK(who);
  NASSEG_REQUIRE(pred && target && out && ws, "%s: null pointer", who);
  ROWS_CHECK(who);
  NASSEG_REQUIRE(valid_min == valid_min && valid_max == valid_max, "%s: NaN bound", who);
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)B * H * W;
  const int grid = red_grid(n);
  float* maxpart = ws;
  float* cntpart = ws + kMaxGrid;
  float* sumpart = ws + 2 * kMaxGrid;
  hipLaunchKernelGGL(berhu_up_max_kernel<kRows>, dim3(grid), dim3(256), 0, s, pred, target, rt, n, g, maxpart,
                     cntpart);
  NASSEG_LAUNCH_CHECK("berhu_up_max");
  hipLaunchKernelGGL(berhu_up_sum_kernel<kRows>, dim3(grid), dim3(256), 0, s, pred, target, rt, n, g, maxpart, grid,
                     sumpart, out);
  NASSEG_LAUNCH_CHECK("berhu_up_sum");
  hipLaunchKernelGGL(berhu_masked_finalize_kernel, dim3(1), dim3(256), 0, s, sumpart, cntpart, grid, out);
  NASSEG_LAUNCH_CHECK("berhu_up_finalize");
  return NASSEG_OK;
}

template <bool kRows>
int up_bwd(const char* who, const act_t* pred, const float* target, RowTable<kRows> rt, const float* stats,
           const float* gscale, int B, int h, int w, int H, int W, float valid_min, float valid_max, int group,
           act_t* dpred, void* stream) {
  UpGeom g;
  UP_GEOM_CHECK(who);
  NASSEG_REQUIRE(pred && target && stats && dpred, "%s: null pointer", who);
  ROWS_CHECK(who);
  NASSEG_REQUIRE(valid_min == valid_min && valid_max == valid_max, "%s: NaN bound", who);
  NASSEG_REQUIRE(group == 0 || group == 1 || group == 4 || group == 16 || group == 64 || group == 256,
                 "%s: group must be 0, 1, 4, 16, 64 or 256 (got %d)", who, group);
  const int G = group ? group : up_bwd_group(h, w, H, W);
  int T = kUpMaxTile;  // G T T = 256
  for (int k = G; k > 1; k /= 4) T /= 2;
  const int gx = G >= 256 ? 32 : (G >= 16 ? 16 : G);
  const int tiles_y = cdiv(h, T), tiles_x = cdiv(w, T);
  const int64_t nwg = (int64_t)B * tiles_y * tiles_x;  // (<= B*h*w < 2^31: up_geom)
  hipLaunchKernelGGL(berhu_up_bwd_kernel<kRows>, dim3((unsigned)nwg), dim3(kUpThreads), 0, (hipStream_t)stream, pred,
                     target, rt, stats, gscale, g, T, G, gx, tiles_y, tiles_x, dpred);
  NASSEG_LAUNCH_CHECK("berhu_up_bwd");
  return NASSEG_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Scale-invariant log and gradient-matching terms on top of the masked berHu (definition: include/nasseg.h,
// "Depth terms"; INTEGRATION.md, "Depth"): the surrogates of what validate_depth scores, all functions of
// r = ln max(p, pred_min) - ln t over the valid pixels of nasseg_berhu_masked_fwd (same sampling, same validity).
//   forward   pass 1 (templated on the row table, as the berHu passes: only the address of an image's target
//             differs) writes the residual map r - a NaN marks an invalid pixel - and the workgroup sums of r, r^2
//             and the count; pass 2 is a stencil over r alone: every valid pixel of grid G_k (y, x multiples of 2^k)
//             counts into M_k and adds |r_j - r_i| for its right and lower neighbour at stride 2^k into S_k, all K
//             scales in one sweep; one finalize launch adds the workgroup partials in fp64 in a fixed order and writes
//             total | D | L_gm | n | m | M_0..M_7.
//   backward  one kernel, one store per pixel in the prediction's type: the berHu's part (berhu_slope, the formula
//             berhu_masked_bwd_kernel uses) plus, where p > pred_min, (1 / p) * (silog part + the signs of the up to
//             4 K neighbour differences read from r).
// No float atomics; grids from the shapes alone.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kMaxScales = 8;
constexpr int kTermParts = 3 + 2 * kMaxScales;  // ws rows of kMaxGrid floats: sum r | sum r^2 | count | S_0 | M_0 | S_1 ...
constexpr int kTermOut = 16;                    // total | D | L_gm | n | m | M_0..M_7 | 3 unused

__device__ __forceinline__ float resid_hole() { return __uint_as_float(0x7fc00000u); }
__device__ __forceinline__ bool resid_valid(float r) { return (__float_as_uint(r) & 0x7f800000u) != 0x7f800000u; }

// sum of red[0..255] into red[0]; every thread of the workgroup calls it
__device__ __forceinline__ void tree256(float* red) {
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
}

template <bool kRows>
__global__ __launch_bounds__(256) void depth_resid_kernel(const act_t* __restrict__ pred,
                                                          const float* __restrict__ target, RowTable<kRows> rt,
                                                          int64_t n, MaskedGeom g, float pred_min,
                                                          float* __restrict__ resid, float* __restrict__ part) {
  __shared__ float red[256];
  float s1 = 0.f, s2 = 0.f, cnt = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float t = masked_target<kRows>(target, rt, i, g);
    float r = resid_hole();
    if (depth_valid(t, g.vmin, g.vmax)) {
      r = logf(fmaxf(lda1(pred + i), pred_min)) - logf(t);  // (each logarithm on its own, fp32)
      s1 += r;
      s2 += r * r;
      cnt += 1.f;  // (at most n / gridDim.x + 256 < 2^24 per workgroup: exact in fp32)
    }
    resid[i] = r;
  }
  const float v[3] = {s1, s2, cnt};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    red[threadIdx.x] = v[q];
    tree256(red);
    if (threadIdx.x == 0) part[q * kMaxGrid + blockIdx.x] = red[0];
    __syncthreads();
  }
}

// part: [2 K][kMaxGrid], row 2k = S_k, row 2k + 1 = M_k of the workgroup
__global__ __launch_bounds__(256) void depth_gm_kernel(const float* __restrict__ resid, int64_t n, int h, int w, int K,
                                                       float* __restrict__ part) {
  __shared__ float red[256];
  float S[kMaxScales], M[kMaxScales];
#pragma unroll
  for (int k = 0; k < kMaxScales; ++k) S[k] = 0.f, M[k] = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float ri = resid[i];
    if (!resid_valid(ri)) continue;
    const int x = (int)(i % w);
    const int y = (int)((i / w) % h);
    bool in = true;  // (G_k+1 is a subset of G_k)
#pragma unroll
    for (int k = 0; k < kMaxScales; ++k) {
      const int s = 1 << k;
      in = in && k < K && ((x | y) & (s - 1)) == 0;
      if (in) {
        M[k] += 1.f;
        float a = 0.f;
        if (x + s < w) {  // (inside the row, so inside the image)
          const float rj = resid[i + s];
          if (resid_valid(rj)) a += fabsf(rj - ri);
        }
        if (y + s < h) {  // (inside the image)
          const float rj = resid[i + (int64_t)s * w];
          if (resid_valid(rj)) a += fabsf(rj - ri);
        }
        S[k] += a;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kMaxScales; ++k) {
    if (k < K) {  // (K is the launch's: every thread takes the same branch)
      red[threadIdx.x] = S[k];
      tree256(red);
      if (threadIdx.x == 0) part[(2 * k) * kMaxGrid + blockIdx.x] = red[0];
      __syncthreads();
      red[threadIdx.x] = M[k];
      tree256(red);
      if (threadIdx.x == 0) part[(2 * k + 1) * kMaxGrid + blockIdx.x] = red[0];
      __syncthreads();
    }
  }
}

// One workgroup: quantity q of the 3 + 2 K rows of part - thread t adds the partials of workgroups t, t + 256, ... in
// fp64, then a fixed-order tree through LDS - and thread 0 writes out (kTermOut floats).  berhu: out of
// nasseg_berhu_masked_fwd (null: no berHu in the total).
__global__ __launch_bounds__(256) void depth_terms_finalize_kernel(const float* __restrict__ part, int nblk, int K,
                                                                   float lambda, const float* __restrict__ berhu,
                                                                   float bw, float sw, float gw,
                                                                   float* __restrict__ out) {
  __shared__ double red[256];
  __shared__ double tot[kTermParts];
  const int nq = 3 + 2 * K;
  for (int q = 0; q < nq; ++q) {
    const float* p = part + (int64_t)q * kMaxGrid;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) s += (double)p[b];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
      if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
      __syncthreads();
    }
    if (threadIdx.x == 0) tot[q] = red[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double n = tot[2];
    const double m = n > 0.0 ? tot[0] / n : 0.0;
    const double D = n > 0.0 ? tot[1] / n - (double)lambda * m * m : 0.0;
    double L = 0.0;
    for (int k = 0; k < kMaxScales; ++k) {
      const double Mk = k < K ? tot[3 + 2 * k + 1] : 0.0;
      if (Mk > 0.0) L += tot[3 + 2 * k] / Mk;
      out[5 + k] = (float)Mk;
    }
    out[0] = (float)((double)bw * (berhu ? (double)berhu[0] : 0.0) + (double)sw * D + (double)gw * L);
    out[1] = (float)D;
    out[2] = (float)L;
    out[3] = (float)n;
    out[4] = (float)m;
    out[13] = out[14] = out[15] = 0.f;
  }
}

// sign(ri - rj) when j is valid, else 0; sign(0) = 0
__device__ __forceinline__ float resid_sign(float ri, float rj) {
  if (!resid_valid(rj)) return 0.f;
  return ri > rj ? 1.f : (ri < rj ? -1.f : 0.f);
}

// dpred = up * [ bw * berHu' + (p > pred_min) / p * ( sw * (2 / n)(r - lambda m)
//                + gw * sum_k [i in G_k] / M_k * sum_{j = i +- (0, s), i +- (s, 0), valid, in the image} sign(r_i - r_j) ) ]
// on valid pixels, exactly 0 elsewhere; up = gscale[0] (null: 1)
template <bool kRows>
__global__ __launch_bounds__(256) void depth_terms_bwd_kernel(const act_t* __restrict__ pred,
                                                              const float* __restrict__ target, RowTable<kRows> rt,
                                                              const float* __restrict__ resid,
                                                              const float* __restrict__ berhu,
                                                              const float* __restrict__ terms,
                                                              const float* __restrict__ gscale, int64_t n,
                                                              MaskedGeom g, float pred_min, float lambda, int K,
                                                              float bw, float sw, float gw,
                                                              act_t* __restrict__ dpred) {
  const float up = gscale ? gscale[0] : 1.f;
  const float c = berhu[1];
  const float nv = berhu[2];
  const float gb = nv > 0.f ? (up * bw) / nv : 0.f;
  const float nt = terms[3];
  const float gs = nt > 0.f ? up * sw * 2.f / nt : 0.f;
  const float lm = lambda * terms[4];
  float gk[kMaxScales];
#pragma unroll
  for (int k = 0; k < kMaxScales; ++k) {
    const float Mk = terms[5 + k];
    gk[k] = (k < K && Mk > 0.f) ? up * gw / Mk : 0.f;
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float t = masked_target<kRows>(target, rt, i, g);
    float d = 0.f;
    if (depth_valid(t, g.vmin, g.vmax)) {
      const float p = lda1(pred + i);
      d = gb * berhu_slope(p - t, c);
      const float ri = resid[i];
      if (p > pred_min && resid_valid(ri)) {  // (a clamped pixel: no gradient from the two terms)
        float acc = gs * (ri - lm);
        const int x = (int)(i % g.w);
        const int y = (int)((i / g.w) % g.h);
        bool in = true;
#pragma unroll
        for (int k = 0; k < kMaxScales; ++k) {
          const int s = 1 << k;
          in = in && k < K && ((x | y) & (s - 1)) == 0;
          if (in) {
            float sg = 0.f;
            if (x + s < g.w) sg += resid_sign(ri, resid[i + s]);
            if (x - s >= 0) sg += resid_sign(ri, resid[i - s]);
            if (y + s < g.h) sg += resid_sign(ri, resid[i + (int64_t)s * g.w]);
            if (y - s >= 0) sg += resid_sign(ri, resid[i - (int64_t)s * g.w]);
            acc = fmaf(gk[k], sg, acc);
          }
        }
        d += acc / p;
      }
    }
    sta1(dpred + i, d);
  }
}

inline bool terms_config(float valid_min, float valid_max, float pred_min, float lambda, int K, float bw, float sw,
                         float gw) {
  return valid_min >= 0.f && valid_max == valid_max && pred_min > 0.f && pred_min < INFINITY && lambda >= 0.f &&
         lambda <= 1.f && K >= 0 && K <= kMaxScales && bw >= 0.f && bw < INFINITY && sw >= 0.f && sw < INFINITY &&
         gw >= 0.f && gw < INFINITY;
}
#define TERMS_CHECK(who)                                                                                       \
  NASSEG_REQUIRE(terms_config(valid_min, valid_max, pred_min, silog_lambda, scales, berhu_weight, silog_weight, \
                              grad_weight),                                                                    \
                 "%s: valid_min >= 0, pred_min > 0, 0 <= silog_lambda <= 1, 0 <= scales <= 8 and finite weights "  \
                 ">= 0 are expected", who)

template <bool kRows>
int terms_fwd(const char* who, const act_t* pred, const float* target, RowTable<kRows> rt, int B, int h, int w, int H,
              int W, float valid_min, float valid_max, float pred_min, float silog_lambda, int scales,
              const float* berhu, float berhu_weight, float silog_weight, float grad_weight, float* resid, float* out,
              float* ws, void* stream) {
  MaskedGeom g;
  NASSEG_REQUIRE(masked_geom(B, h, w, H, W, valid_min, valid_max, &g), "%s: bad shape", who);
  NASSEG_REQUIRE(pred && target && resid && out && ws, "%s: null pointer", who);
  ROWS_CHECK(who);
  TERMS_CHECK(who);
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)B * h * w;
  const int grid = red_grid(n);
  hipLaunchKernelGGL(depth_resid_kernel<kRows>, dim3(grid), dim3(256), 0, s, pred, target, rt, n, g, pred_min, resid,
                     ws);
  NASSEG_LAUNCH_CHECK("depth_resid");
  if (scales > 0) {
    hipLaunchKernelGGL(depth_gm_kernel, dim3(grid), dim3(256), 0, s, (const float*)resid, n, h, w, scales,
                       ws + 3 * kMaxGrid);
    NASSEG_LAUNCH_CHECK("depth_gm");
  }
  hipLaunchKernelGGL(depth_terms_finalize_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, grid, scales,
                     silog_lambda, berhu, berhu_weight, silog_weight, grad_weight, out);
  NASSEG_LAUNCH_CHECK("depth_terms_finalize");
  return NASSEG_OK;
}

template <bool kRows>
int terms_bwd(const char* who, const act_t* pred, const float* target, RowTable<kRows> rt, const float* resid,
              const float* berhu, const float* terms, const float* gscale, int B, int h, int w, int H, int W,
              float valid_min, float valid_max, float pred_min, float silog_lambda, int scales, float berhu_weight,
              float silog_weight, float grad_weight, act_t* dpred, void* stream) {
  MaskedGeom g;
  NASSEG_REQUIRE(masked_geom(B, h, w, H, W, valid_min, valid_max, &g), "%s: bad shape", who);
  NASSEG_REQUIRE(pred && target && resid && berhu && terms && dpred, "%s: null pointer", who);
  ROWS_CHECK(who);
  TERMS_CHECK(who);
  const int64_t n = (int64_t)B * h * w;
  hipLaunchKernelGGL(depth_terms_bwd_kernel<kRows>, dim3(red_grid(n) * 2), dim3(256), 0, (hipStream_t)stream, pred,
                     target, rt, resid, berhu, terms, gscale, n, g, pred_min, silog_lambda, scales, berhu_weight,
                     silog_weight, grad_weight, dpred);
  NASSEG_LAUNCH_CHECK("depth_terms_bwd");
  return NASSEG_OK;
}

const RowTable<false> kNoRows = {};

}  // namespace

extern "C" {

#if NASSEG_FP32_ONLY
int64_t nasseg_berhu_masked_workspace(void) { return 3 * kMaxGrid; }
#endif

// pred: dense [B][h][w] (one channel), target: fp32 [B][H][W].  out[0] = loss, out[1] = c, out[2] = n_valid.
// ws: nasseg_berhu_masked_workspace() floats.
int NASSEG_FN(berhu_masked_fwd)(const act_t* pred, const float* target, int B, int h, int w, int H, int W,
                                float valid_min, float valid_max, float* out, float* ws, void* stream) {
  return masked_fwd<false>("berhu_masked_fwd", pred, target, kNoRows, B, h, w, H, W, valid_min, valid_max, out, ws,
                           stream);
}

// stats = out of nasseg_berhu_masked_fwd; gscale = device scalar upstream gradient (null = 1)
int NASSEG_FN(berhu_masked_bwd)(const act_t* pred, const float* target, const float* stats, const float* gscale,
                                int B, int h, int w, int H, int W, float valid_min, float valid_max, act_t* dpred,
                                void* stream) {
  return masked_bwd<false>("berhu_masked_bwd", pred, target, kNoRows, stats, gscale, B, h, w, H, W, valid_min,
                           valid_max, dpred, stream);
}

// The row-indexed twins: target is the whole cache [n_rows][H][W], rows a device array of B cache rows; image b of the
// prediction meets target[clamp(rows[b], 0, n_rows - 1)].  Everything else - and every bit - as above on target[rows].
int NASSEG_FN(berhu_masked_rows_fwd)(const act_t* pred, const float* target, const int64_t* rows, int64_t n_rows,
                                     int B, int h, int w, int H, int W, float valid_min, float valid_max, float* out,
                                     float* ws, void* stream) {
  const RowTable<true> rt = {rows, n_rows};
  return masked_fwd<true>("berhu_masked_rows_fwd", pred, target, rt, B, h, w, H, W, valid_min, valid_max, out, ws,
                          stream);
}

int NASSEG_FN(berhu_masked_rows_bwd)(const act_t* pred, const float* target, const int64_t* rows, int64_t n_rows,
                                     const float* stats, const float* gscale, int B, int h, int w, int H, int W,
                                     float valid_min, float valid_max, act_t* dpred, void* stream) {
  const RowTable<true> rt = {rows, n_rows};
  return masked_bwd<true>("berhu_masked_rows_bwd", pred, target, rt, stats, gscale, B, h, w, H, W, valid_min,
                          valid_max, dpred, stream);
}

#if NASSEG_FP32_ONLY
// floats: [1024] maxima | [1024] counts | [1024] sums, whatever the sizes - a function of the grid alone
int64_t nasseg_berhu_up_workspace(int B, int h, int w, int H, int W) {
  UpGeom g;
  return up_geom(B, h, w, H, W, 0.f, 0.f, &g) ? 3 * kMaxGrid : 0;
}
#endif

// pred: dense [B][h][w] (one channel), target: fp32 [B][H][W].  out[0] = loss, out[1] = c, out[2] = n_valid.
// ws: nasseg_berhu_up_workspace floats.
int NASSEG_FN(berhu_up_fwd)(const act_t* pred, const float* target, int B, int h, int w, int H, int W,
                            float valid_min, float valid_max, float* out, float* ws, void* stream) {
  return up_fwd<false>("berhu_up_fwd", pred, target, kNoRows, B, h, w, H, W, valid_min, valid_max, out, ws, stream);
}

// stats = out of nasseg_berhu_up_fwd; gscale = device scalar upstream gradient (null = 1); group: lanes per
// prediction pixel - 0: chosen from the shapes (up_bwd_group), else 1, 4, 16, 64 or 256 (measurements and tests)
int NASSEG_FN(berhu_up_bwd)(const act_t* pred, const float* target, const float* stats, const float* gscale, int B,
                            int h, int w, int H, int W, float valid_min, float valid_max, int group, act_t* dpred,
                            void* stream) {
  return up_bwd<false>("berhu_up_bwd", pred, target, kNoRows, stats, gscale, B, h, w, H, W, valid_min, valid_max,
                       group, dpred, stream);
}

// row-indexed twins (see nasseg_berhu_masked_rows_fwd): the limits B*H*W < 2^32, B*h*w < 2^31 are the BATCH's, the
// cache may be larger
int NASSEG_FN(berhu_up_rows_fwd)(const act_t* pred, const float* target, const int64_t* rows, int64_t n_rows, int B,
                                 int h, int w, int H, int W, float valid_min, float valid_max, float* out, float* ws,
                                 void* stream) {
  const RowTable<true> rt = {rows, n_rows};
  return up_fwd<true>("berhu_up_rows_fwd", pred, target, rt, B, h, w, H, W, valid_min, valid_max, out, ws, stream);
}

int NASSEG_FN(berhu_up_rows_bwd)(const act_t* pred, const float* target, const int64_t* rows, int64_t n_rows,
                                 const float* stats, const float* gscale, int B, int h, int w, int H, int W,
                                 float valid_min, float valid_max, int group, act_t* dpred, void* stream) {
  const RowTable<true> rt = {rows, n_rows};
  return up_bwd<true>("berhu_up_rows_bwd", pred, target, rt, stats, gscale, B, h, w, H, W, valid_min, valid_max,
                      group, dpred, stream);
}

#if NASSEG_FP32_ONLY
// floats: [3 + 2 * 8][1024] workgroup partials, whatever the sizes
int64_t nasseg_depth_terms_workspace(void) { return (int64_t)kTermParts * kMaxGrid; }
#endif

// Scale-invariant log + gradient-matching terms (definition: include/nasseg.h, "Depth terms").  berhu: out of
// nasseg_berhu_masked_fwd on the same arguments (null: the total has no berHu); resid: fp32 [B][h][w], written;
// out: 16 floats = total | D | L_gm | n | m | M_0..M_7 | 3 unused; ws: nasseg_depth_terms_workspace() floats.
int NASSEG_FN(depth_terms_fwd)(const act_t* pred, const float* target, int B, int h, int w, int H, int W,
                               float valid_min, float valid_max, float pred_min, float silog_lambda, int scales,
                               const float* berhu, float berhu_weight, float silog_weight, float grad_weight,
                               float* resid, float* out, float* ws, void* stream) {
  return terms_fwd<false>("depth_terms_fwd", pred, target, kNoRows, B, h, w, H, W, valid_min, valid_max, pred_min,
                          silog_lambda, scales, berhu, berhu_weight, silog_weight, grad_weight, resid, out, ws,
                          stream);
}

// resid, terms: resid and out of nasseg_depth_terms_fwd; berhu: out of nasseg_berhu_masked_fwd; gscale: device scalar
// upstream gradient of the total (null = 1).  dpred: the gradient of all three terms, written once.
int NASSEG_FN(depth_terms_bwd)(const act_t* pred, const float* target, const float* resid, const float* berhu,
                               const float* terms, const float* gscale, int B, int h, int w, int H, int W,
                               float valid_min, float valid_max, float pred_min, float silog_lambda, int scales,
                               float berhu_weight, float silog_weight, float grad_weight, act_t* dpred,
                               void* stream) {
  return terms_bwd<false>("depth_terms_bwd", pred, target, kNoRows, resid, berhu, terms, gscale, B, h, w, H, W,
                          valid_min, valid_max, pred_min, silog_lambda, scales, berhu_weight, silog_weight,
                          grad_weight, dpred, stream);
}

// row-indexed twins (see nasseg_berhu_masked_rows_fwd): target is the cache [n_rows][H][W], read in place
int NASSEG_FN(depth_terms_rows_fwd)(const act_t* pred, const float* target, const int64_t* rows, int64_t n_rows,
                                    int B, int h, int w, int H, int W, float valid_min, float valid_max,
                                    float pred_min, float silog_lambda, int scales, const float* berhu,
                                    float berhu_weight, float silog_weight, float grad_weight, float* resid,
                                    float* out, float* ws, void* stream) {
  const RowTable<true> rt = {rows, n_rows};
  return terms_fwd<true>("depth_terms_rows_fwd", pred, target, rt, B, h, w, H, W, valid_min, valid_max, pred_min,
                         silog_lambda, scales, berhu, berhu_weight, silog_weight, grad_weight, resid, out, ws, stream);
}

int NASSEG_FN(depth_terms_rows_bwd)(const act_t* pred, const float* target, const int64_t* rows, int64_t n_rows,
                                    const float* resid, const float* berhu, const float* terms, const float* gscale,
                                    int B, int h, int w, int H, int W, float valid_min, float valid_max,
                                    float pred_min, float silog_lambda, int scales, float berhu_weight,
                                    float silog_weight, float grad_weight, act_t* dpred, void* stream) {
  const RowTable<true> rt = {rows, n_rows};
  return terms_bwd<true>("depth_terms_rows_bwd", pred, target, rt, resid, berhu, terms, gscale, B, h, w, H, W,
                         valid_min, valid_max, pred_min, silog_lambda, scales, berhu_weight, silog_weight,
                         grad_weight, dpred, stream);
}

}  // extern "C"
