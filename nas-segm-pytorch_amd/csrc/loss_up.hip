// Cross-entropy of low-resolution logits against FULL-SIZE labels, the bilinear up-sampling fused in (definition:
// include/nasseg.h, "full-size cross-entropy"; INTEGRATION.md, "Losses").
//
// Reference: src/engine/trainer.py:141-146,236-250 resize the labels DOWN to the logits (nearest) before the loss,
// while validate() (src/engine/inference.py:55-66) scores the logits resized UP to the labels.  The remedy of DeepLab /
// torchvision / mmseg - up-sample the logits, take the loss at the labels' size - composed from nasseg_bilinear_fwd +
// nasseg_ce_sel_fwd writes, keeps and reads back a [B][H][W][C] tensor in each direction.  Here the interpolated row of
// a label pixel lives in registers only:
//   forward   one lane per label pixel: the four neighbour rows of the logits through L1 / L2 (lanes next to each other
//             share them), v_c = the row nasseg_argmax_cm takes its argmax of, bit for bit; pixel_loss and lse are the
//             only per-pixel outputs.  Selection: nasseg_ohem_threshold over pixel_loss.  Then the sum pass and the
//             fp64 finalize of nasseg_ce_sel_fwd (csrc/loss_common.h: the same kernels).
//   backward  a gather (as nasseg_bilinear_bwd): a workgroup owns a tile of kUpTile x kUpTile logits pixels and a chunk
//             of <= kUpChunk channels, stages tile + halo of the logits in LDS (row stride cn | 1 floats: odd), and every
//             thread walks the label pixels of ITS (pixel, channel) in a fixed order: re-interpolates its channel,
//             exp(v - lse) - onehot, times the pixel's factor and Wy Wx.  dlogits is written once; no atomics.
// Every pass exists once, as a template on an optional ROW TABLE (nasseg_ce_up_rows_*; `Rows... lr`: LabelRows,
// csrc/loss_common.h): image b of the logits then meets image rows[b] of a label cache - the task0 cache - instead of
// image b of the labels; only the address of an image's labels differs, so both forms give the same bits and the
// batch's labels are never gathered into a copy.
// The region-overlap term at the labels' size (nasseg_ce_up_region_*): after the forward above, a pass that adds the
// class sums of q = expf(v - lse) into per-workgroup fp64 rows, the finalize of nasseg_ce_region_fwd
// (csrc/loss_common.h) on them, one more pass for gdot[p] = sum_c G_pc q_pc, and the backward gather above with the
// region part inside its per-visit expression (a compile-time flag: without it, the kernel nasseg_ce_up_bwd launches).
#include <math.h>

#include <type_traits>

#include "loss_common.h"
#include "resize_index.h"

namespace {

constexpr int kUpTile = 8;        // backward: logits pixels per tile side
constexpr int kUpPatch = kUpTile + 2;
constexpr int kUpChunk = 64;      // backward: channels per workgroup

template <typename TL, typename... Rows>
__global__ __launch_bounds__(256) void ce_up_fwd_kernel(const act_t* __restrict__ logits, const TL* __restrict__ target,
                                                        int B, int h, int w, int C, int H, int W, float sh, float sw,
                                                        int ignore, float* __restrict__ pixel_loss,
                                                        float* __restrict__ lse_out, Rows... lr) {
  const int64_t P = (int64_t)B * H * W;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    int X, Y, b;
    int64_t t;
    if constexpr (sizeof...(Rows) != 0) {  // (the label's address needs b: decoded first - in 32 bits, p < 2^32)
      const uint32_t off = label_decode((uint32_t)p, b, lr...);
      Y = (int)(off / (uint32_t)W);
      X = (int)(off - (uint32_t)Y * (uint32_t)W);
      t = (int64_t)label_image(target, (int64_t)b, lr...)[off];
    } else {
      t = (int64_t)target[p];
    }
    if (NASSEG_LABEL_SKIPPED(t, C, ignore)) {
      pixel_loss[p] = -1.f;
      lse_out[p] = 0.f;
      continue;
    }
    if constexpr (sizeof...(Rows) == 0) {
      X = (int)(p % W);
      const int64_t q = p / W;
      Y = (int)(q % H);
      b = (int)(q / H);
    }
    const Lin ly = lin_coeff(Y, sh, h, H);
    const Lin lx = lin_coeff(X, sw, w, W);
    const act_t* lb = logits + (int64_t)b * h * w * C;
    const act_t* p00 = lb + ((int64_t)ly.i0 * w + lx.i0) * C;
    const act_t* p01 = lb + ((int64_t)ly.i0 * w + lx.i1) * C;
    const act_t* p10 = lb + ((int64_t)ly.i1 * w + lx.i0) * C;
    const act_t* p11 = lb + ((int64_t)ly.i1 * w + lx.i1) * C;
    float m = up_interp(lda1(p00), lda1(p01), lda1(p10), lda1(p11), ly, lx);
    for (int c = 1; c < C; ++c)
      m = fmaxf(m, up_interp(lda1(p00 + c), lda1(p01 + c), lda1(p10 + c), lda1(p11 + c), ly, lx));
    float s = 0.f;
    for (int c = 0; c < C; ++c)
      s += expf(up_interp(lda1(p00 + c), lda1(p01 + c), lda1(p10 + c), lda1(p11 + c), ly, lx) - m);
    const float lse = m + logf(s);
    pixel_loss[p] = lse - up_interp(lda1(p00 + t), lda1(p01 + t), lda1(p10 + t), lda1(p11 + t), ly, lx);
    lse_out[p] = lse;
  }
}

// ---------------------------------------------------------------------------
// The region-overlap term at the labels' size (nasseg_ce_up_region_*; definition: include/nasseg.h).
// ---------------------------------------------------------------------------
// Label pixel p of the batch -> its label (returned), image and coordinates: the decoding of ce_up_fwd_kernel.
template <typename TL, typename... Rows>
__device__ __forceinline__ int64_t up_label(const TL* __restrict__ target, int64_t p, int H, int W, int& b, int& Y,
                                            int& X, Rows... lr) {
  if constexpr (sizeof...(Rows) != 0) {
    const uint32_t off = label_decode((uint32_t)p, b, lr...);
    Y = (int)(off / (uint32_t)W);
    X = (int)(off - (uint32_t)Y * (uint32_t)W);
    return (int64_t)label_image(target, (int64_t)b, lr...)[off];
  } else {
    X = (int)(p % W);
    const int64_t q = p / W;
    Y = (int)(q % H);
    b = (int)(q / H);
    return (int64_t)target[p];
  }
}

// The four neighbour rows of a label pixel and its two coefficient pairs.
struct UpRow {
  const act_t *p00, *p01, *p10, *p11;
  Lin ly, lx;
  __device__ __forceinline__ float at(int64_t c) const {
    return up_interp(lda1(p00 + c), lda1(p01 + c), lda1(p10 + c), lda1(p11 + c), ly, lx);
  }
};
__device__ __forceinline__ UpRow up_row(const act_t* __restrict__ logits, int b, int Y, int X, int h, int w, int C,
                                        int H, int W, float sh, float sw) {
  UpRow r;
  r.ly = lin_coeff(Y, sh, h, H);
  r.lx = lin_coeff(X, sw, w, W);
  const act_t* lb = logits + (int64_t)b * h * w * C;
  r.p00 = lb + ((int64_t)r.ly.i0 * w + r.lx.i0) * C;
  r.p01 = lb + ((int64_t)r.ly.i0 * w + r.lx.i1) * C;
  r.p10 = lb + ((int64_t)r.ly.i1 * w + r.lx.i0) * C;
  r.p11 = lb + ((int64_t)r.ly.i1 * w + r.lx.i1) * C;
  return r;
}

// After ce_up_fwd_kernel (which stays the one writer of pixel_loss and lse: their bits are nasseg_ce_up_fwd's because
// the kernel is): the class sums of q_pc = expf(v_pc - lse_p) over the valid pixels (pixel_loss >= 0), the row
// interpolated once more, by the route of region_fwd_kernel (csrc/loss.hip): per class a butterfly over the wave (fp32
// within the tile of 256 label pixels), the four waves' sums through 3 KB of LDS in chunks of 64 classes, and the
// workgroup's row of part[3][C][kRegionRows] accumulated in place in fp64, each element by the one thread that owns
// it, in tile order.  Every workgroup of ce_grid(P) owns at least one tile, so every row below the grid's size is
// written.
template <typename TL, typename... Rows>
__global__ __launch_bounds__(256) void ce_up_region_sums_kernel(const act_t* __restrict__ logits,
                                                                const TL* __restrict__ target, int B, int h, int w,
                                                                int C, int H, int W, float sh, float sw,
                                                                const float* __restrict__ pixel_loss,
                                                                const float* __restrict__ lse_in,
                                                                double* __restrict__ part, Rows... lr) {
  __shared__ float red[4][3][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t P = (int64_t)B * H * W;
  const int64_t ntiles = (P + 255) / 256;
  bool first = true;
  for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const int64_t p = tl * 256 + tid;
    int64_t t = -1;
    bool valid = false;
    float lse = 0.f;
    UpRow r = {};
    if (p < P && pixel_loss[p] >= 0.f) {
      int X, Y, b;
      t = up_label(target, p, H, W, b, Y, X, lr...);  // (valid: in [0, C))
      valid = true;
      r = up_row(logits, b, Y, X, h, w, C, H, W, sh, sw);
      lse = lse_in[p];
    }
    for (int c0 = 0; c0 < C; c0 += 64) {
      const int nc = C - c0 < 64 ? C - c0 : 64;
      for (int j = 0; j < nc; ++j) {
        const int c = c0 + j;
        const float q = valid ? expf(r.at(c) - lse) : 0.f;
        const bool hit = valid && t == (int64_t)c;
        const float vS = wave_allsum(q);
        const float vI = wave_allsum(hit ? q : 0.f);
        const float vN = (float)__popcll(__ballot(hit));
        if (lane == 0) {
          red[wave][0][j] = vI;
          red[wave][1][j] = vS;
          red[wave][2][j] = vN;
        }
      }
      __syncthreads();
      if (tid < 3 * nc) {
        const int k = tid / nc, j = tid - k * nc;
        const float v = ((red[0][k][j] + red[1][k][j]) + red[2][k][j]) + red[3][k][j];
        double* dst = part + ((int64_t)k * C + c0 + j) * kRegionRows + blockIdx.x;
        *dst = first ? (double)v : *dst + (double)v;
      }
      __syncthreads();
    }
    first = false;
  }
}

// After the finalize: gdot[p] = sum_c G_pc q_pc with G_pc = coef[C + c] + [t_p == c] coef[c] and q the forward's
// (expf(v - lse), the row interpolated once more), 0 on pixels that are not valid (pixel_loss < 0).  One lane per label
// pixel; the sum runs over c ascending, the label's own term last.
template <typename TL, typename... Rows>
__global__ __launch_bounds__(256) void ce_up_gdot_kernel(const act_t* __restrict__ logits,
                                                         const TL* __restrict__ target, int B, int h, int w, int C,
                                                         int H, int W, float sh, float sw,
                                                         const float* __restrict__ pixel_loss,
                                                         const float* __restrict__ lse, const float* __restrict__ coef,
                                                         float* __restrict__ gdot, Rows... lr) {
  const int64_t P = (int64_t)B * H * W;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    if (pixel_loss[p] < 0.f) {
      gdot[p] = 0.f;
      continue;
    }
    int X, Y, b;
    const int64_t t = up_label(target, p, H, W, b, Y, X, lr...);  // (valid: in [0, C))
    const UpRow r = up_row(logits, b, Y, X, h, w, C, H, W, sh, sw);
    const float l = lse[p];
    float dot = 0.f;
    for (int c = 0; c < C; ++c) dot = fmaf(coef[C + c], expf(r.at(c) - l), dot);
    gdot[p] = fmaf(coef[t], expf(r.at(t) - l), dot);
  }
}

// (up_interp, up_dst_range, up_weight: csrc/resize_index.h)
// grid: (channel chunk, tile x, tile y, image), flattened, chunk fastest.  VEC: the patch is staged with 16-byte
// (bf16: 8-byte) loads - one chunk (C <= kUpChunk) and 16-byte aligned logits; else element by element.
// LDS: patch[kUpPatch][kUpPatch][cn | 1] floats.
// RG = NoRegion: the cross-entropy alone (nasseg_ce_up_bwd: the `else` branches below are its code).  RG = RegionBwd
// (nasseg_ce_up_region_bwd): every VALID label pixel is visited and adds region_weight * q (G - gdot) to the
// cross-entropy part, which only a kept pixel has; the thread's channel is fixed, so its two coefficients are
// registers.
struct NoRegion {};
struct RegionBwd {
  const float* coef;  // [2C]: region_finalize_kernel's
  const float* gdot;  // [B][H][W]: sum_c G_pc q_pc (ce_up_gdot_kernel)
  float rweight;
  int with_ce;
};

template <typename TL, bool VEC, typename RG, typename... Rows>
__global__ __launch_bounds__(256) void ce_up_bwd_kernel(const act_t* __restrict__ logits, const TL* __restrict__ target,
                                                        const float* __restrict__ weight,
                                                        const float* __restrict__ pixel_loss,
                                                        const float* __restrict__ lse, const float* __restrict__ stats,
                                                        const float* __restrict__ gscale, int B, int h, int w, int C,
                                                        int H, int W, float sh, float sw, int tiles_y, int tiles_x,
                                                        int nchunk, act_t* __restrict__ dlogits, RG rg, Rows... lr) {
  constexpr bool kRows = sizeof...(Rows) != 0;
  constexpr bool kRegion = std::is_same<RG, RegionBwd>::value;
  extern __shared__ float patch[];
  const int tid = threadIdx.x;
  int wi = blockIdx.x;
  const int ch = wi % nchunk;
  wi /= nchunk;
  const int tx = wi % tiles_x;
  wi /= tiles_x;
  const int ty = wi % tiles_y;
  const int b = wi / tiles_y;
  const int c0 = ch * kUpChunk;
  const int cn = C - c0 < kUpChunk ? C - c0 : kUpChunk;
  const int CS = cn | 1;
  const int y0 = ty * kUpTile, x0 = tx * kUpTile;
  const int ny = h - y0 < kUpTile ? h - y0 : kUpTile;  // the tile's own pixels
  const int nx = w - x0 < kUpTile ? w - x0 : kUpTile;
  const int oy = y0 > 0 ? y0 - 1 : 0, ox = x0 > 0 ? x0 - 1 : 0;  // origin of the patch: one pixel of halo, inside the map
  const int py = (y0 + ny < h ? y0 + ny : h - 1) - oy + 1;         // its rows (<= kUpPatch)
  const int px = (x0 + nx < w ? x0 + nx : w - 1) - ox + 1;         // its pixels per row (<= kUpPatch)
  if (VEC) {  // (cn == C) a patch row is px * C contiguous elements: whole aligned vectors around it, inside the buffer
    const int64_t total4 = ((int64_t)B * h * w * C) & ~(int64_t)3;
    const int n = px * C;
    const int nvmax = (n + 3) / 4 + 1;
    for (int j = tid; j < py * nvmax; j += 256) {
      const int r = j / nvmax, i = j - r * nvmax;
      const int64_t g0 = (((int64_t)b * h + oy + r) * w + ox) * C;
      const int64_t a = (g0 & ~(int64_t)3) + 4 * (int64_t)i;
      if (a >= g0 + n) continue;
      float* prow = patch + r * kUpPatch * CS;
      const int rel = (int)(a - g0);  // (-3 .. n - 1)
      if (a + 4 <= total4) {
        const float4 v = lda4(logits + a);
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int q = rel + k;
          if (q >= 0 && q < n) {
            const int xx = q / C;
            prow[xx * CS + (q - xx * C)] = e[k];
          }
        }
      } else {  // (the last, incomplete vector of the buffer)
        for (int k = 0; k < 4; ++k) {
          const int q = rel + k;
          if (q >= 0 && q < n) {
            const int xx = q / C;
            prow[xx * CS + (q - xx * C)] = lda1(logits + a + k);
          }
        }
      }
    }
  } else {
    const int n = px * cn;
    for (int j = tid; j < py * n; j += 256) {
      const int r = j / n, q = j - r * n;
      const int xx = q / cn, c = q - xx * cn;
      patch[(r * kUpPatch + xx) * CS + c] = lda1(logits + (((int64_t)b * h + oy + r) * w + ox + xx) * C + c0 + c);
    }
  }
  __syncthreads();
  const float g = gscale ? gscale[0] : 1.f;
  float sumw, tau, gr = 0.f;
  bool with_ce = true;
  if constexpr (kRegion) {  // (the term alone: stats may be null)
    with_ce = rg.with_ce != 0;
    sumw = with_ce ? stats[0] : 1.f;
    tau = with_ce ? stats[1] : 0.f;
    gr = g * rg.rweight;
  } else {
    sumw = stats[0];
    tau = stats[1];
  }
  // (with a table: pixel p of the batch has its label (rows[b] - b) images further on in the cache - one scalar load
  //  of the table per workgroup, and every visit reads the address it read without one, from another base)
  const TL* tbase = target;
  if constexpr (kRows) tbase = label_base(target, (int64_t)b, lr...);
  for (int item = tid; item < ny * nx * cn; item += 256) {
    const int pix = item / cn, c = item - pix * cn;
    const int iy = pix / nx, jx = pix - iy * nx;
    const int i = y0 + iy, j = x0 + jx;
    int ylo, yhi, xlo, xhi;
    up_dst_range(i, sh, h, H, ylo, yhi);
    up_dst_range(j, sw, w, W, xlo, xhi);
    float acc = 0.f;
    float ca = 0.f, cb = 0.f;
    if constexpr (kRegion) {
      ca = rg.coef[c0 + c];
      cb = rg.coef[C + c0 + c];
    }
    for (int Y = ylo; Y <= yhi; ++Y) {
      const Lin ly = lin_coeff(Y, sh, h, H);
      const float wy = up_weight(ly, i);
      if (wy == 0.f) continue;  // (so ly.i0, ly.i1 lie in [i - 1, i + 1]: inside the patch)
      const float* r0 = patch + (ly.i0 - oy) * kUpPatch * CS + c;
      const float* r1 = patch + (ly.i1 - oy) * kUpPatch * CS + c;
      const int64_t prow = ((int64_t)b * H + Y) * W;
      for (int X = xlo; X <= xhi; ++X) {
        const Lin lx = lin_coeff(X, sw, w, W);
        const float wx = up_weight(lx, j);
        if (wx == 0.f) continue;
        const int64_t p = prow + X;
        if constexpr (kRegion) {
          const float pl = pixel_loss[p];
          if (pl < 0.f) continue;  // (-1 on pixels that are not valid)
          const bool kept = with_ce && sel_kept(pl, tau);
          const int64_t t = (int64_t)tbase[p];
          const bool y = (int64_t)(c0 + c) == t;
          const int a0 = (lx.i0 - ox) * CS, a1 = (lx.i1 - ox) * CS;
          const float v = up_interp(r0[a0], r0[a1], r1[a0], r1[a1], ly, lx);
          const float q = expf(v - lse[p]);
          float ce = 0.f;
          if (kept) ce = ((g * (weight ? weight[t] : 1.f)) / sumw) * (q - (y ? 1.f : 0.f));  // (the line below)
          const float G = cb + (y ? ca : 0.f);
          acc = fmaf(wy * wx, fmaf(gr, q * (G - rg.gdot[p]), ce), acc);
        } else {
          if (!sel_kept(pixel_loss[p], tau)) continue;  // (-1 on pixels that are not valid)
          const int64_t t = (int64_t)tbase[p];
          const float gp = (g * (weight ? weight[t] : 1.f)) / sumw;
          const int a0 = (lx.i0 - ox) * CS, a1 = (lx.i1 - ox) * CS;
          const float v = up_interp(r0[a0], r0[a1], r1[a0], r1[a1], ly, lx);
          const float d = gp * (expf(v - lse[p]) - ((int64_t)(c0 + c) == t ? 1.f : 0.f));
          acc = fmaf(wy * wx, d, acc);
        }
      }
    }
    sta1(dlogits + (((int64_t)b * h + i) * w + j) * C + c0 + c, acc);
  }
}

inline bool up_shape_ok(int B, int h, int w, int C, int H, int W) {
  if (B <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || C < 2) return false;
  if ((int64_t)B * H * W >= ((int64_t)1 << 32)) return false;
  if ((int64_t)B * h * w * C >= ((int64_t)1 << 31)) return false;
  // the backward's grid: one workgroup of 256 threads per (tile, channel chunk), and a grid holds fewer than 2^32 threads
  if ((int64_t)B * cdiv(h, kUpTile) * cdiv(w, kUpTile) * cdiv(C, kUpChunk) >= ((int64_t)1 << 24)) return false;
  return true;
}

#define UP_SHAPE_CHECK(who)                          \
  NASSEG_REQUIRE(up_shape_ok(B, h, w, C, H, W),      \
                 "%s: bad shape (C >= 2, B*H*W < 2^32, B*h*w*C < 2^31, fewer than 2^24 backward tiles)", who)

// Launches: one body per entry-point pair.  lr empty: target is the batch's own [B][H][W] labels; one LabelRows: the
// cache [n_rows][H][W] and the device table of B rows.  Same geometry, same order of sums, same finalize.
inline bool rows_ok() { return true; }
inline bool rows_ok(const LabelRows& lr) { return lr.rows && lr.n_rows > 0; }
#define ROWS_CHECK(who) \
  NASSEG_REQUIRE(rows_ok(lr...), "%s: a row table of B entries and n_rows > 0 are expected", who)
// (H*W < 2^32: up_shape_ok, which every launch body checks first)
inline LabelRows label_rows(const int64_t* rows, int64_t n_rows, int H, int W) {
  return {rows, n_rows, (uint32_t)((int64_t)H * W)};
}

template <typename... Rows>
int up_fwd(const char* who, const act_t* logits, const void* target, int elem_size, const float* weight, int B, int h,
           int w, int C, int H, int W, int ignore, int select, float t_loss, int64_t min_kept, double keep_fraction,
           float* loss, float* stats, int64_t* counts, float* pixel_loss, float* lse, float* ws, void* stream,
           Rows... lr) {
  static_assert(sizeof...(Rows) <= 1, "no table, or one LabelRows");
  UP_SHAPE_CHECK(who);
  NASSEG_TRY(check_elem_size(who, elem_size));
  NASSEG_REQUIRE(logits && target && loss && stats && counts && pixel_loss && lse && ws, "%s: null pointer", who);
  ROWS_CHECK(who);
  NASSEG_TRY(check_selection(who, select, min_kept, keep_fraction));
  hipStream_t s = (hipStream_t)stream;
  const int64_t P = (int64_t)B * H * W;
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  with_labels(target, elem_size, [&](auto labels) {
    hipLaunchKernelGGL((ce_up_fwd_kernel<label_of<decltype(labels)>, Rows...>), dim3(ce_grid(P)), dim3(256), 0, s,
                       logits, labels, B, h, w, C, H, W, sh, sw, ignore, pixel_loss, lse, lr...);
  });
  NASSEG_LAUNCH_CHECK("ce_up_fwd");
  const auto selection = [&](float* tau, int64_t* cnt) {  // (the stand-alone one: include/nasseg.h)
    return nasseg_ohem_threshold(pixel_loss, P, t_loss, min_kept, keep_fraction, tau, cnt, ws + 3 * kCeGridCap, stream);
  };
  return ce_sel_reduce("ce_up_sum", "ce_up_finalize", selection, pixel_loss, target, elem_size, weight, P, select, loss,
                       stats, counts, ws, s, lr...);
}

// rg: NoRegion (the cross-entropy alone) or RegionBwd.
template <typename RG, typename... Rows>
int up_bwd(const char* who, const act_t* logits, const void* target, int elem_size, const float* weight,
           const float* pixel_loss, const float* lse, const float* stats, const float* gscale, int B, int h, int w,
           int C, int H, int W, act_t* dlogits, void* stream, RG rg, Rows... lr) {
  static_assert(sizeof...(Rows) <= 1, "no table, or one LabelRows");
  UP_SHAPE_CHECK(who);
  NASSEG_TRY(check_elem_size(who, elem_size));
  NASSEG_REQUIRE(logits && target && pixel_loss && lse && dlogits, "%s: null pointer", who);
  if constexpr (std::is_same<RG, RegionBwd>::value)
    NASSEG_REQUIRE(rg.coef && rg.gdot && (!rg.with_ce || stats), "%s: null pointer", who);
  else
    NASSEG_REQUIRE(stats, "%s: null pointer", who);
  ROWS_CHECK(who);
  hipStream_t s = (hipStream_t)stream;
  const int tiles_y = cdiv(h, kUpTile), tiles_x = cdiv(w, kUpTile), nchunk = cdiv(C, kUpChunk);
  const int64_t nwg = (int64_t)B * tiles_y * tiles_x * nchunk;  // (< 2^24: up_shape_ok)
  const int cmax = C < kUpChunk ? C : kUpChunk;
  const size_t lds = (size_t)kUpPatch * kUpPatch * (cmax | 1) * sizeof(float);
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  const bool vec = nchunk == 1 && ((uintptr_t)logits & 15) == 0;
  with_labels(target, elem_size, [&](auto labels) {
    using TL = label_of<decltype(labels)>;
    const auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)nwg), dim3(256), lds, s, logits, labels, weight, pixel_loss, lse, stats,
                         gscale, B, h, w, C, H, W, sh, sw, tiles_y, tiles_x, nchunk, dlogits, rg, lr...);
    };
    if (vec)
      launch(ce_up_bwd_kernel<TL, true, RG, Rows...>);
    else
      launch(ce_up_bwd_kernel<TL, false, RG, Rows...>);
  });
  NASSEG_LAUNCH_CHECK("ce_up_bwd");
  return NASSEG_OK;
}

// The backward with the region term.  region_weight == 0 beside the cross-entropy: the term adds nothing, and the launch
// is nasseg_ce_up_bwd's own - the kernel without the region part - so that the gradient has its bits.  (The region
// instantiation computes the same cross-entropy expression, but the compiler fuses the multiply-adds of the
// interpolation differently in the two instantiations, so their last bits differ.)
template <typename... Rows>
int up_region_bwd(const char* who, const act_t* logits, const void* target, int elem_size, const float* weight,
                  const float* pixel_loss, const float* lse, const float* stats, const float* coef, const float* gdot,
                  const float* gscale, int with_ce, double region_weight, int B, int h, int w, int C, int H, int W,
                  act_t* dlogits, void* stream, Rows... lr) {
  const float rw = (float)region_weight;
  if (with_ce && rw == 0.f)
    return up_bwd(who, logits, target, elem_size, weight, pixel_loss, lse, stats, gscale, B, h, w, C, H, W, dlogits,
                  stream, NoRegion{}, lr...);
  return up_bwd(who, logits, target, elem_size, weight, pixel_loss, lse, stats, gscale, B, h, w, C, H, W, dlogits,
                stream, RegionBwd{coef, gdot, rw, with_ce}, lr...);
}

// floats of the workspace before its fp64 part: the sum pass's partials | the selection's words, to an even count
inline int64_t up_region_head() { return (3 * kCeGridCap + nasseg_ohem_workspace() + 1) & ~(int64_t)1; }

struct RegionFwd {
  int with_ce;
  double alpha, beta, smooth;
  int all_classes;
  double rweight;
  float *loss_ce, *loss_region, *coef, *sums;
  int64_t* ncls;
  float* gdot;
};

// ce_up_fwd_kernel, ce_up_region_sums_kernel, [the selection and the sum pass of up_fwd,] region_finalize_kernel on
// this path's rows, ce_up_gdot_kernel.  ws: partials | selection | fp64 part[3][C][kRegionRows] | fp64 tot[3][C].
template <typename... Rows>
int up_region_fwd(const char* who, const act_t* logits, const void* target, int elem_size, const float* weight, int B,
                  int h, int w, int C, int H, int W, int ignore, int select, float t_loss, int64_t min_kept,
                  double keep_fraction, const RegionFwd& rf, float* loss, float* stats, int64_t* counts,
                  float* pixel_loss, float* lse, float* ws, void* stream, Rows... lr) {
  static_assert(sizeof...(Rows) <= 1, "no table, or one LabelRows");
  UP_SHAPE_CHECK(who);
  NASSEG_TRY(check_elem_size(who, elem_size));
  NASSEG_REQUIRE(logits && target && loss && rf.loss_ce && rf.loss_region && rf.coef && rf.sums && rf.ncls &&
                     rf.gdot && pixel_loss && lse && ws,
                 "%s: null pointer", who);
  NASSEG_REQUIRE(!rf.with_ce || (stats && counts), "%s: null pointer", who);
  ROWS_CHECK(who);
  NASSEG_REQUIRE(rf.with_ce || !select, "%s: selection without the cross-entropy", who);
  NASSEG_TRY(check_selection(who, select, min_kept, keep_fraction));
  NASSEG_REQUIRE(rf.alpha >= 0.0 && rf.beta >= 0.0 && rf.alpha + rf.beta > 0.0 && rf.smooth >= 0.0,
                 "%s: alpha, beta, smooth >= 0 and alpha + beta > 0 expected", who);
  NASSEG_REQUIRE(!rf.all_classes || rf.smooth > 0.0, "%s: all classes need smooth > 0", who);
  NASSEG_REQUIRE(((uintptr_t)ws & 7) == 0, "%s: the workspace must be 8-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const int64_t P = (int64_t)B * H * W;
  const int grid = ce_grid(P);  // (<= kRegionRows)
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  double* part = (double*)(ws + up_region_head());
  double* tot = part + (int64_t)3 * C * kRegionRows;
  with_labels(target, elem_size, [&](auto labels) {
    using TL = label_of<decltype(labels)>;
    hipLaunchKernelGGL((ce_up_fwd_kernel<TL, Rows...>), dim3(grid), dim3(256), 0, s, logits, labels, B, h, w, C, H, W,
                       sh, sw, ignore, pixel_loss, lse, lr...);
    hipLaunchKernelGGL((ce_up_region_sums_kernel<TL, Rows...>), dim3(grid), dim3(256), 0, s, logits, labels, B, h, w, C,
                       H, W, sh, sw, pixel_loss, lse, part, lr...);
  });
  NASSEG_LAUNCH_CHECK("ce_up_region_fwd");
  if (rf.with_ce) {  // (the finalizer below reads the partials)
    const auto selection = [&](float* tau, int64_t* cnt) {
      return nasseg_ohem_threshold(pixel_loss, P, t_loss, min_kept, keep_fraction, tau, cnt, ws + 3 * kCeGridCap,
                                   stream);
    };
    NASSEG_TRY(ce_sel_reduce("ce_up_region_sum", nullptr, selection, pixel_loss, target, elem_size, weight, P, select,
                             nullptr, stats, counts, ws, s, lr...));
  }
  hipLaunchKernelGGL(region_finalize_kernel, dim3(1), dim3(1024), 0, s, ws, part, grid, C, rf.with_ce, select,
                     rf.alpha, rf.beta, rf.smooth, rf.all_classes, rf.rweight, loss, rf.loss_ce, rf.loss_region, stats,
                     counts, rf.coef, rf.sums, rf.ncls, tot);
  NASSEG_LAUNCH_CHECK("ce_up_region_finalize");
  // (nothing is summed here, so no cap of 1024 workgroups: a workgroup per 256 label pixels, fewer than 2^24 - with four
  //  waves per SIMD the pass waits on its loads, measured: DESIGN.md 3.6)
  const unsigned gdot_grid = (unsigned)((P + 255) / 256);
  with_labels(target, elem_size, [&](auto labels) {
    hipLaunchKernelGGL((ce_up_gdot_kernel<label_of<decltype(labels)>, Rows...>), dim3(gdot_grid), dim3(256), 0, s,
                       logits, labels, B, h, w, C, H, W, sh, sw, pixel_loss, lse, rf.coef, rf.gdot, lr...);
  });
  NASSEG_LAUNCH_CHECK("ce_up_gdot");
  return NASSEG_OK;
}

}  // namespace

extern "C" {

#if NASSEG_FP32_ONLY
// floats: [kCeGridCap][3] partials | the selection's words.  A function of the grid alone.
int64_t nasseg_ce_up_workspace(int B, int h, int w, int C, int H, int W) {
  if (!up_shape_ok(B, h, w, C, H, W)) return 0;
  return 3 * kCeGridCap + nasseg_ohem_workspace();
}
#endif

int NASSEG_FN(ce_up_fwd)(const act_t* logits, const void* target, int elem_size, const float* weight, int B, int h,
                         int w, int C, int H, int W, int ignore, int select, float t_loss, int64_t min_kept,
                         double keep_fraction, float* loss, float* stats, int64_t* counts, float* pixel_loss,
                         float* lse, float* ws, void* stream) {
  return up_fwd("ce_up_fwd", logits, target, elem_size, weight, B, h, w, C, H, W, ignore, select, t_loss, min_kept,
                keep_fraction, loss, stats, counts, pixel_loss, lse, ws, stream);
}

int NASSEG_FN(ce_up_bwd)(const act_t* logits, const void* target, int elem_size, const float* weight,
                         const float* pixel_loss, const float* lse, const float* stats, const float* gscale, int B,
                         int h, int w, int C, int H, int W, int ignore, act_t* dlogits, void* stream) {
  (void)ignore;  // (validity is pixel_loss >= 0: the forward decided it)
  return up_bwd("ce_up_bwd", logits, target, elem_size, weight, pixel_loss, lse, stats, gscale, B, h, w, C, H, W,
                dlogits, stream, NoRegion{});
}

// The row-indexed twins: target is the whole label cache [n_rows][H][W], rows a device array of B cache rows; image b
// of the logits meets target[clamp(rows[b], 0, n_rows - 1)].  Everything else - and every bit - as above on
// target[rows]; the limits of up_shape_ok are the BATCH's, the cache may be larger.
int NASSEG_FN(ce_up_rows_fwd)(const act_t* logits, const void* target, int elem_size, const int64_t* rows,
                              int64_t n_rows, const float* weight, int B, int h, int w, int C, int H, int W,
                              int ignore, int select, float t_loss, int64_t min_kept, double keep_fraction,
                              float* loss, float* stats, int64_t* counts, float* pixel_loss, float* lse, float* ws,
                              void* stream) {
  return up_fwd("ce_up_rows_fwd", logits, target, elem_size, weight, B, h, w, C, H, W, ignore, select, t_loss,
                min_kept, keep_fraction, loss, stats, counts, pixel_loss, lse, ws, stream,
                label_rows(rows, n_rows, H, W));
}

int NASSEG_FN(ce_up_rows_bwd)(const act_t* logits, const void* target, int elem_size, const int64_t* rows,
                              int64_t n_rows, const float* weight, const float* pixel_loss, const float* lse,
                              const float* stats, const float* gscale, int B, int h, int w, int C, int H, int W,
                              int ignore, act_t* dlogits, void* stream) {
  (void)ignore;
  return up_bwd("ce_up_rows_bwd", logits, target, elem_size, weight, pixel_loss, lse, stats, gscale, B, h, w, C, H, W,
                dlogits, stream, NoRegion{}, label_rows(rows, n_rows, H, W));
}

#if NASSEG_FP32_ONLY
// floats: nasseg_ce_up_workspace's (to an even count) | fp64 part[3][C][kRegionRows] | fp64 tot[3][C]
int64_t nasseg_ce_up_region_workspace(int B, int h, int w, int C, int H, int W) {
  if (!up_shape_ok(B, h, w, C, H, W)) return 0;
  return up_region_head() + 2 * ((int64_t)3 * C * kRegionRows + (int64_t)3 * C);
}
#endif

// The cross-entropy above plus the region-overlap term over the label pixels (include/nasseg.h).
int NASSEG_FN(ce_up_region_fwd)(const act_t* logits, const void* target, int elem_size, const float* weight, int B,
                                int h, int w, int C, int H, int W, int ignore, int with_ce, int select, float t_loss,
                                int64_t min_kept, double keep_fraction, double alpha, double beta, double smooth,
                                int all_classes, double region_weight, float* loss, float* loss_ce, float* loss_region,
                                float* stats, int64_t* counts, float* pixel_loss, float* lse, float* coef, float* sums,
                                int64_t* ncls, float* gdot, float* ws, void* stream) {
  const RegionFwd rf = {with_ce, alpha, beta, smooth, all_classes, region_weight, loss_ce, loss_region, coef, sums,
                        ncls,    gdot};
  return up_region_fwd("ce_up_region_fwd", logits, target, elem_size, weight, B, h, w, C, H, W, ignore, select, t_loss,
                       min_kept, keep_fraction, rf, loss, stats, counts, pixel_loss, lse, ws, stream);
}

int NASSEG_FN(ce_up_region_bwd)(const act_t* logits, const void* target, int elem_size, const float* weight,
                                const float* pixel_loss, const float* lse, const float* stats, const float* coef,
                                const float* gdot, const float* gscale, int with_ce, double region_weight, int B, int h,
                                int w, int C, int H, int W, int ignore, act_t* dlogits, void* stream) {
  (void)ignore;
  return up_region_bwd("ce_up_region_bwd", logits, target, elem_size, weight, pixel_loss, lse, stats, coef, gdot, gscale,
                       with_ce, region_weight, B, h, w, C, H, W, dlogits, stream);
}

int NASSEG_FN(ce_up_region_rows_fwd)(const act_t* logits, const void* target, int elem_size, const int64_t* rows,
                                     int64_t n_rows, const float* weight, int B, int h, int w, int C, int H, int W,
                                     int ignore, int with_ce, int select, float t_loss, int64_t min_kept,
                                     double keep_fraction, double alpha, double beta, double smooth, int all_classes,
                                     double region_weight, float* loss, float* loss_ce, float* loss_region,
                                     float* stats, int64_t* counts, float* pixel_loss, float* lse, float* coef,
                                     float* sums, int64_t* ncls, float* gdot, float* ws, void* stream) {
  const RegionFwd rf = {with_ce, alpha, beta, smooth, all_classes, region_weight, loss_ce, loss_region, coef, sums,
                        ncls,    gdot};
  return up_region_fwd("ce_up_region_rows_fwd", logits, target, elem_size, weight, B, h, w, C, H, W, ignore, select,
                       t_loss, min_kept, keep_fraction, rf, loss, stats, counts, pixel_loss, lse, ws, stream,
                       label_rows(rows, n_rows, H, W));
}

int NASSEG_FN(ce_up_region_rows_bwd)(const act_t* logits, const void* target, int elem_size, const int64_t* rows,
                                     int64_t n_rows, const float* weight, const float* pixel_loss, const float* lse,
                                     const float* stats, const float* coef, const float* gdot, const float* gscale,
                                     int with_ce, double region_weight, int B, int h, int w, int C, int H, int W,
                                     int ignore, act_t* dlogits, void* stream) {
  (void)ignore;
  return up_region_bwd("ce_up_region_rows_bwd", logits, target, elem_size, weight, pixel_loss, lse, stats, coef, gdot,
                       gscale, with_ce, region_weight, B, h, w, C, H, W, dlogits, stream,
                       label_rows(rows, n_rows, H, W));
}

}  // extern "C"
