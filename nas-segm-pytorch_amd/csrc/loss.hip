// Per-pixel log-softmax + NLL loss with ignore index, fp32 NHWC logits, gfx950.
//
// Reference: nn.LogSoftmax() (implicit dim=1) followed by
// nn.NLLLoss2d(ignore_index=255) (src/main_search.py:435,
// src/engine/trainer.py:144-146,156-158,239-241,248-250):
//   loss = mean over pixels with target != ignore of -log_softmax(logits)[target]
// (an all-ignored batch gives 0/0 = NaN, as in torch).
// In NHWC the C class scores of one pixel are contiguous, so one lane owns one
// pixel; the forward also emits the gradient wrt the logits for a unit upstream
// gradient, so backward is a single scale.
#include <math.h>

#include "loss_common.h"

namespace {

// The selection's histograms (3 x 2048 words, see sel_hist_kernel) back to zero, by whatever grid runs this: the
// forward kernels of nasseg_ce_sel_fwd do it on their way, the selection's launches follow them.
constexpr int kSelBins = 2048;
constexpr int kSelHistWords = 3 * kSelBins;
__device__ __forceinline__ void sel_clear(uint32_t* __restrict__ hist) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < kSelHistWords; i += gridDim.x * blockDim.x) hist[i] = 0u;
}

// KD (nasseg_ce_mse_fwd): each thread also adds (x - t)^2 over its pixels' rows - ignored pixels included, as
// nn.MSELoss knows no ignore index - and the workgroup's sum goes to sqpart[blockIdx.x].
// SEL (nasseg_ce_sel_fwd): the same per-pixel arithmetic, but l_p goes to pixel_loss[p] (-1 for a pixel that is
// not valid) and nothing is reduced here.
template <typename TL, bool KD = false, bool SEL = false>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const act_t* __restrict__ logits,
                                                     const TL* __restrict__ target, int64_t P,
                                                     int C, int ignore, float* __restrict__ partial,
                                                     const float* __restrict__ teacher = nullptr,
                                                     float* __restrict__ sqpart = nullptr,
                                                     float* __restrict__ pixel_loss = nullptr,
                                                     uint32_t* __restrict__ sel_hist = nullptr) {
  if (SEL && sel_hist) sel_clear(sel_hist);
  __shared__ float red_l[256];
  __shared__ float red_n[256];
  __shared__ float red_s[KD ? 256 : 1];
  float loss = 0.f, cnt = 0.f, sq = 0.f;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    const int64_t t = (int64_t)target[p];
    const act_t* lp = logits + p * C;
    if (KD)
      for (int c = 0; c < C; ++c) {
        const float d = lda1(lp + c) - teacher[p * C + c];
        sq += d * d;
      }
    if (NASSEG_LABEL_SKIPPED(t, C, ignore)) {
      if (SEL) pixel_loss[p] = -1.f;
      continue;
    }
    float m = lda1(lp);
    for (int c = 1; c < C; ++c) m = fmaxf(m, lda1(lp + c));
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(lda1(lp + c) - m);
    const float lse = m + logf(s);
    if (SEL) {
      pixel_loss[p] = lse - lda1(lp + t);
      continue;
    }
    loss += lse - lda1(lp + t);
    cnt += 1.f;
  }
  if (SEL) return;
  red_l[threadIdx.x] = loss;
  red_n[threadIdx.x] = cnt;
  if (KD) red_s[threadIdx.x] = sq;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red_l[threadIdx.x] += red_l[threadIdx.x + s];
      red_n[threadIdx.x] += red_n[threadIdx.x + s];
      if (KD) red_s[threadIdx.x] += red_s[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[blockIdx.x * 2] = red_l[0];
    partial[blockIdx.x * 2 + 1] = red_n[0];
    if (KD) sqpart[blockIdx.x] = red_s[0];
  }
}

// out[0] = loss (mean), out[1] = number of valid pixels.  One workgroup of 256 threads: thread t
// adds the partials of blocks t, t+256, ... in fp64, then a fixed-order tree through LDS.
// KD: also ce[0] = out[0] and mse[0] = (sum of the sqpart partials, same order) / n_el.
template <bool KD = false>
__global__ __launch_bounds__(256) void ce_finalize_kernel(const float* __restrict__ partial, int nblk,
                                                          float* __restrict__ out,
                                                          const float* __restrict__ sqpart = nullptr,
                                                          double n_el = 0.0, float* __restrict__ ce = nullptr,
                                                          float* __restrict__ mse = nullptr) {
  __shared__ double red_l[256];
  __shared__ double red_n[256];
  __shared__ double red_s[KD ? 256 : 1];
  double l = 0.0, n = 0.0, q = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) {
    l += (double)partial[b * 2];
    n += (double)partial[b * 2 + 1];
    if (KD) q += (double)sqpart[b];
  }
  red_l[threadIdx.x] = l;
  red_n[threadIdx.x] = n;
  if (KD) red_s[threadIdx.x] = q;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red_l[threadIdx.x] += red_l[threadIdx.x + s];
      red_n[threadIdx.x] += red_n[threadIdx.x + s];
      if (KD) red_s[threadIdx.x] += red_s[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)(red_l[0] / red_n[0]);
    out[1] = (float)red_n[0];
    if (KD) {
      ce[0] = out[0];
      mse[0] = (float)(red_s[0] / n_el);
    }
  }
}

// The same two computations for C <= 63 with the scores staged through LDS: a workgroup's 256
// pixels are 256*C CONTIGUOUS floats, loaded (and, backward, stored) with fully coalesced
// accesses; each lane then works on its pixel's row in LDS (row stride C|1 is odd: no bank
// conflicts).  One lane per pixel straight from HBM touches 64 rows 4*C bytes apart per load.
// Pixel -> (workgroup, thread) assignment, per-pixel arithmetic and reduction order are those
// of ce_fwd_kernel / ce_bwd_kernel: bit-identical results.
// KD (nasseg_ce_mse_fwd / _bwd): the teacher's fp32 tile [np][C] is read with the same coalesced float4 loops -
// forward, by the staging loop (sum of (x - t)^2 over every element, ignored pixels included -> sqpart[blockIdx.x]);
// backward, by the store loop, which adds gmse * 2 (x - t) / (P*C) to the cross-entropy gradient.  Pixel mapping,
// per-pixel arithmetic and the reduction order of the cross-entropy part are those of the plain kernel, so the NLL
// and (with gmse = 0) its gradient are bit-identical to nasseg_ce_fwd / nasseg_ce_bwd.
// SEL (nasseg_ce_sel_fwd / _bwd): forward, l_p goes to pixel_loss[p] (-1 where the pixel is not valid) instead of
// into the workgroup's sums; backward, stats = {sum of the kept pixels' weights, tau}: a pixel is skipped (zeros)
// unless it is valid and sel_kept(pixel_loss[p], tau), and its factor is gscale * weight[t] / stats[0] - with unit
// weights the very division of the plain kernel.
template <typename TL, bool BWD, bool KD = false, bool SEL = false>
__global__ __launch_bounds__(256) void ce_tile_kernel(const act_t* __restrict__ logits,
                                                      const TL* __restrict__ target, int64_t P, int C,
                                                      int ignore, float* __restrict__ partial,
                                                      const float* __restrict__ stats,
                                                      const float* __restrict__ gscale,
                                                      act_t* __restrict__ dlogits,
                                                      const float* __restrict__ teacher = nullptr,
                                                      const float* __restrict__ gmse = nullptr,
                                                      float* __restrict__ sqpart = nullptr,
                                                      const float* __restrict__ weight = nullptr,
                                                      float* __restrict__ pixel_loss = nullptr,
                                                      uint32_t* __restrict__ sel_hist = nullptr) {
  if (!BWD && SEL && sel_hist) sel_clear(sel_hist);
  extern __shared__ float tile[];  // [256][C | 1]
  __shared__ float red_l[256];
  __shared__ float red_n[256];
  __shared__ float red_s[KD && !BWD ? 256 : 1];
  const int CS = C | 1;
  const int tid = threadIdx.x;
  const int64_t ntiles = (P + 255) / 256;
  float loss = 0.f, cnt = 0.f, sq = 0.f;
  float g = 0.f, gm = 0.f;
  if (BWD) g = SEL ? (gscale ? gscale[0] : 1.f) : (gscale ? gscale[0] : 1.f) / stats[1];
  const float sumw = BWD && SEL ? stats[0] : 1.f, tau = BWD && SEL ? stats[1] : 0.f;
  if (BWD && KD) gm = (float)(2.0 * (double)(gmse ? gmse[0] : 1.f) / ((double)P * (double)C));
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t p0 = t * 256;
    const int np = (int)((P - p0) < 256 ? (P - p0) : 256);
    const int nel = np * C;
    const act_t* src = logits + p0 * C;
    const float* tsrc = KD ? teacher + p0 * C : nullptr;
    const int nel4 = nel >> 2;  // (p0*C is a multiple of 4: vector accesses are aligned)
    float pl = -1.f;  // (SEL backward: asked for before the tile is staged, needed after it)
    if (BWD && SEL && tid < np) pl = pixel_loss[p0 + tid];
    for (int i = tid; i < nel4; i += 256) {
      const float4 v = lda4(src + 4 * i);
      if (KD && !BWD) {
        const float4 tv = ld4(tsrc + 4 * i);
        const float d0 = v.x - tv.x, d1 = v.y - tv.y, d2 = v.z - tv.z, d3 = v.w - tv.w;
        sq += d0 * d0;
        sq += d1 * d1;
        sq += d2 * d2;
        sq += d3 * d3;
      }
      int pix = (4 * i) / C;
      int c = 4 * i - pix * C;
      const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        tile[pix * CS + c] = e[r];
        if (++c == C) {
          c = 0;
          ++pix;
        }
      }
    }
    for (int i = 4 * nel4 + tid; i < nel; i += 256) {
      const int pix = i / C;
      const float x = lda1(src + i);
      tile[pix * CS + (i - pix * C)] = x;
      if (KD && !BWD) {
        const float d = x - tsrc[i];
        sq += d * d;
      }
    }
    __syncthreads();
    if (tid < np) {
      float* row = tile + tid * CS;
      const int64_t tg = (int64_t)target[p0 + tid];
      bool skip = NASSEG_LABEL_SKIPPED(tg, C, ignore);
      float gp = g;
      if (BWD && SEL && !skip) {
        skip = !sel_kept(pl, tau);
        gp = (g * (weight ? weight[tg] : 1.f)) / sumw;
      }
      if (!BWD && SEL && skip) pixel_loss[p0 + tid] = -1.f;
      if (BWD && skip) {
        for (int c = 0; c < C; ++c) row[c] = 0.f;
      } else if (!skip) {
        float m = row[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, row[c]);
        float sum = 0.f;
        for (int c = 0; c < C; ++c) {
          const float e = expf(row[c] - m);
          if (BWD) row[c] = e;  // (kept: the softmax needs it again)
          sum += e;
        }
        if (BWD) {
          const float inv = 1.f / sum;
          for (int c = 0; c < C; ++c) row[c] = gp * (row[c] * inv - ((int64_t)c == tg ? 1.f : 0.f));
        } else if (SEL) {
          pixel_loss[p0 + tid] = (m + logf(sum)) - row[tg];
        } else {
          loss += (m + logf(sum)) - row[tg];
          cnt += 1.f;
        }
      }
    }
    __syncthreads();
    if (BWD) {
      act_t* dst = dlogits + p0 * C;
      for (int i = tid; i < nel4; i += 256) {
        int pix = (4 * i) / C;
        int c = 4 * i - pix * C;
        float e[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          e[r] = tile[pix * CS + c];
          if (++c == C) {
            c = 0;
            ++pix;
          }
        }
        if (KD) {  // (the staged logits were overwritten by the softmax: read again, L2-resident)
          const float4 v = lda4(src + 4 * i);
          const float4 tv = ld4(tsrc + 4 * i);
          e[0] = fmaf(gm, v.x - tv.x, e[0]);
          e[1] = fmaf(gm, v.y - tv.y, e[1]);
          e[2] = fmaf(gm, v.z - tv.z, e[2]);
          e[3] = fmaf(gm, v.w - tv.w, e[3]);
        }
        sta4(dst + 4 * i, make_float4(e[0], e[1], e[2], e[3]));
      }
      for (int i = 4 * nel4 + tid; i < nel; i += 256) {
        const int pix = i / C;
        float e = tile[pix * CS + (i - pix * C)];
        if (KD) e = fmaf(gm, lda1(src + i) - tsrc[i], e);
        sta1(dst + i, e);
      }
      __syncthreads();
    }
  }
  if (!BWD && !SEL) {
    red_l[tid] = loss;
    red_n[tid] = cnt;
    if (KD) red_s[tid] = sq;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) {
        red_l[tid] += red_l[tid + s];
        red_n[tid] += red_n[tid + s];
        if (KD) red_s[tid] += red_s[tid + s];
      }
      __syncthreads();
    }
    if (tid == 0) {
      partial[blockIdx.x * 2] = red_l[0];
      partial[blockIdx.x * 2 + 1] = red_n[0];
      if (KD) sqpart[blockIdx.x] = red_s[0];
    }
  }
}

// dlogits[p][c] = gscale[0] * (softmax(p)[c] - [c == target]) / nvalid   (0 for ignored pixels)
// KD (nasseg_ce_mse_bwd): + gmse[0] * 2 (x - teacher) / (P*C) on every element, ignored pixels included.
// SEL (nasseg_ce_sel_bwd): as in ce_tile_kernel.
template <typename TL, bool KD = false, bool SEL = false>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const act_t* __restrict__ logits,
                                                     const TL* __restrict__ target,
                                                     const float* __restrict__ stats,
                                                     const float* __restrict__ gscale, int64_t P,
                                                     int C, int ignore, act_t* __restrict__ dlogits,
                                                     const float* __restrict__ teacher = nullptr,
                                                     const float* __restrict__ gmse = nullptr,
                                                     const float* __restrict__ weight = nullptr,
                                                     const float* __restrict__ pixel_loss = nullptr) {
  const float g = SEL ? (gscale ? gscale[0] : 1.f) : (gscale ? gscale[0] : 1.f) / stats[1];
  const float sumw = SEL ? stats[0] : 1.f, tau = SEL ? stats[1] : 0.f;
  const float gm = KD ? (float)(2.0 * (double)(gmse ? gmse[0] : 1.f) / ((double)P * (double)C)) : 0.f;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    const int64_t t = (int64_t)target[p];
    const act_t* lp = logits + p * C;
    act_t* dp = dlogits + p * C;
    const float* tp = KD ? teacher + p * C : nullptr;
    bool skip = NASSEG_LABEL_SKIPPED(t, C, ignore);
    float gp = g;
    if (SEL && !skip) {
      skip = !sel_kept(pixel_loss[p], tau);
      gp = (g * (weight ? weight[t] : 1.f)) / sumw;
    }
    if (skip) {
      for (int c = 0; c < C; ++c) sta1(dp + c, KD ? gm * (lda1(lp + c) - tp[c]) : 0.f);
      continue;
    }
    float m = lda1(lp);
    for (int c = 1; c < C; ++c) m = fmaxf(m, lda1(lp + c));
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(lda1(lp + c) - m);
    const float inv = 1.f / s;
    for (int c = 0; c < C; ++c) {
      float sm = expf(lda1(lp + c) - m) * inv;
      float d = gp * (sm - ((int64_t)c == t ? 1.f : 0.f));
      if (KD) d = fmaf(gm, lda1(lp + c) - tp[c], d);
      sta1(dp + c, d);
    }
  }
}

// ---------------------------------------------------------------------------
// Hard-example selection (nasseg_ohem_threshold, nasseg_ce_sel_fwd): the exact k-th largest of the per-pixel
// losses that take part (entries >= 0), by a radix select on their bit patterns - for non-negative floats the
// unsigned order of the patterns is the order of the values.  Three digits of 11 + 11 + 10 bits, most significant
// first; per digit one histogram pass over the array (the values that match the digits found so far; LDS
// histogram per workgroup, flushed with INTEGER atomics - sums of integers do not depend on arrival order) and
// one single-workgroup scan that walks the bins from the top until k is reached.  k itself is computed on the
// device from the number of entries that take part (the total of the first histogram).  No host synchronisation,
// no allocation, no float atomics.
// Workspace (4-byte words): hist[3][2048] | SelState.
// ---------------------------------------------------------------------------
struct SelState {
  int64_t krem;     // rank still to find among the entries that match `prefix`
  uint32_t prefix;  // the digits found so far, right-aligned
  uint32_t pad;
};
constexpr int kSelWsWords = kSelHistWords + (int)(sizeof(SelState) / 4);

__global__ __launch_bounds__(256) void sel_zero_kernel(uint32_t* __restrict__ hist) { sel_clear(hist); }

template <int PASS>
__global__ __launch_bounds__(256) void sel_hist_kernel(const float* __restrict__ v, int64_t P,
                                                       const SelState* __restrict__ st,
                                                       uint32_t* __restrict__ hist) {
  __shared__ uint32_t bins[kSelBins];
  constexpr int NB = PASS == 2 ? 1024 : 2048;
  for (int i = threadIdx.x; i < NB; i += 256) bins[i] = 0u;
  __syncthreads();
  const uint32_t prefix = PASS ? st->prefix : 0u;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    const float x = v[p];
    if (x < 0.f) continue;
    const uint32_t key = __float_as_uint(x) & 0x7fffffffu;  // (-0 takes part as +0)
    if (PASS == 0) {
      atomicAdd(&bins[key >> 21], 1u);
    } else if (PASS == 1) {
      if ((key >> 21) == prefix) atomicAdd(&bins[(key >> 10) & 0x7ffu], 1u);
    } else {
      if ((key >> 10) == prefix) atomicAdd(&bins[key & 0x3ffu], 1u);
    }
  }
  __syncthreads();
  uint32_t* out = hist + PASS * kSelBins;
  for (int i = threadIdx.x; i < NB; i += 256)
    if (bins[i]) atomicAdd(&out[i], bins[i]);
}

// One workgroup of 256 threads, 8 (4 in the last pass) consecutive bins each.  PASS 0 also computes
// k = min(n, max(min_kept, ceil(keep_fraction * n))) from n = the histogram's total; PASS 2 ends the selection:
// tau = min(t_loss, L_(k)), counts = {k, n, 0} (n == 0: L_(k) = +inf).
template <int PASS>
__global__ __launch_bounds__(256) void sel_scan_kernel(const uint32_t* __restrict__ hist, SelState* __restrict__ st,
                                                       float t_loss, int64_t min_kept, double keep_fraction,
                                                       float* __restrict__ tau, int64_t* __restrict__ counts) {
  constexpr int PER = PASS == 2 ? 4 : 8;
  __shared__ int64_t sums[256];
  __shared__ int64_t s_krem;
  const uint32_t* h = hist + PASS * kSelBins;
  const int tid = threadIdx.x;
  uint32_t c[PER];
  int64_t mine = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    c[i] = h[tid * PER + i];
    mine += (int64_t)c[i];
  }
  sums[tid] = mine;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {  // suffix sums: sums[t] = the entries in the bins of threads t .. 255
    const int64_t add = tid + off < 256 ? sums[tid + off] : 0;
    __syncthreads();
    sums[tid] += add;
    __syncthreads();
  }
  if (tid == 0) {
    if (PASS == 0) {
      const int64_t n = sums[0];
      int64_t k = (int64_t)ceil(keep_fraction * (double)n);
      if (k < min_kept) k = min_kept;
      if (k > n) k = n;
      s_krem = k;
      counts[0] = k;
      counts[1] = n;
      counts[2] = 0;
    } else {
      s_krem = st->krem;
    }
  }
  __syncthreads();
  const int64_t krem = s_krem;
  if (PASS == 0 && krem == 0) {  // nothing takes part
    if (tid == 0) {
      st->krem = 0;
      st->prefix = 0u;
    }
    return;
  }
  int64_t above = sums[tid] - mine;  // entries in the bins of the threads after this one
  if (above < krem && krem <= above + mine) {  // exactly one thread: the k-th largest lies in its bins
#pragma unroll
    for (int i = PER - 1; i >= 0; --i) {
      if (krem <= above + (int64_t)c[i]) {
        const uint32_t digit = (uint32_t)(tid * PER + i);
        const uint32_t prefix = PASS == 0 ? digit : ((st->prefix << (PASS == 1 ? 11 : 10)) | digit);
        st->prefix = prefix;
        st->krem = krem - above;
        break;
      }
      above += (int64_t)c[i];
    }
  }
  if (PASS == 2) {
    __syncthreads();
    if (tid == 0) {
      const bool none = counts[1] == 0;
      const float lk = none ? __builtin_inff() : __uint_as_float(st->prefix);
      // min(t_loss, L_(k)): L_(k) >= 0, so a t_loss that is not positive is the smaller one
      const bool t_smaller = !(t_loss > 0.f) || __float_as_uint(t_loss) < __float_as_uint(lk);
      tau[0] = t_smaller ? t_loss : lk;
    }
  }
}

// counts[2] += entries kept at tau (integer atomics; sel_scan_kernel<2> left 0 there)
__global__ __launch_bounds__(256) void sel_count_kernel(const float* __restrict__ v, int64_t P,
                                                        const float* __restrict__ tau,
                                                        int64_t* __restrict__ counts) {
  __shared__ unsigned int red[256];
  const float t = tau[0];
  unsigned int n = 0;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256)
    n += sel_kept(v[p], t) ? 1u : 0u;
  red[threadIdx.x] = n;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0 && red[0])
    atomicAdd(reinterpret_cast<unsigned long long*>(counts + 2), (unsigned long long)red[0]);
}

// ---------------------------------------------------------------------------
// Region-overlap term (soft Jaccard / Dice / Tversky; nasseg_ce_region_fwd / _bwd, definition: include/nasseg.h)
// computed in the two passes over the logits the cross-entropy makes anyway.  Over the valid pixels, with
// q = softmax(x): I_c = sum q_pc [t_p == c], S_c = sum q_pc, N_c = sum [t_p == c].
// Forward: a workgroup adds the three rows of its pixels - fp32 within a tile of 256 pixels, fp64 across its tiles -
// and writes them as row blockIdx.x of part[3][C][kRegionRows] (fp64); region_finalize_kernel adds the rows in fp64 in
// a fixed order.  No atomics anywhere: deterministic, capturable.
// Kernels of their own (not further flags of ce_tile_kernel / ce_fwd_kernel / ce_bwd_kernel), so that what the
// existing entry points compute cannot move; pixel -> (workgroup, thread) mapping, the per-pixel max / exp / sum
// arithmetic and the cross-entropy gradient expression are copied from them, so that pixel_loss and, at
// region_weight = 0, dlogits are bit-identical to nasseg_ce_sel_fwd's / _bwd's.
// ---------------------------------------------------------------------------
// (kRegionRows, wave_allsum, region_finalize_kernel: csrc/loss_common.h - nasseg_ce_up_region_* shares them)

// One [np][C] tile of logits into LDS rows of stride CS: the staging loops of ce_tile_kernel.
__device__ __forceinline__ void region_stage(const act_t* __restrict__ src, float* __restrict__ tile, int nel, int C,
                                             int CS, int tid) {
  const int nel4 = nel >> 2;
  for (int i = tid; i < nel4; i += 256) {
    const float4 v = lda4(src + 4 * i);
    int pix = (4 * i) / C;
    int c = 4 * i - pix * C;
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      tile[pix * CS + c] = e[r];
      if (++c == C) {
        c = 0;
        ++pix;
      }
    }
  }
  for (int i = 4 * nel4 + tid; i < nel; i += 256) {
    const int pix = i / C;
    tile[pix * CS + (i - pix * C)] = lda1(src + i);
  }
}

// C <= 63, aligned logits.  LDS: the [256][C | 1] tile of ce_tile_kernel and nothing else (C = 19: 19,456 bytes).
// Each lane turns its pixel's row into q in place (zeros for a pixel that is not valid) and marks the label's entry
// with the sign bit (q >= 0, and -0 keeps the mark): the class sums are then column sums of the tile - thread
// (seg, col) adds the rows of segment seg (256 / C segments) in order, the segments' sums pass through the head of
// the tile (free by then) and thread c < C adds them in order.
// (amdgpu_waves_per_eu: 8 workgroups per CU, as many as the LDS tile allows at C = 19 and as ce_tile_kernel runs.)
template <typename TL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void region_tile_fwd_kernel(
    const act_t* __restrict__ logits, const TL* __restrict__ target, int64_t P, int C, int ignore,
    float* __restrict__ pixel_loss, uint32_t* __restrict__ sel_hist, double* __restrict__ part) {
  if (sel_hist) sel_clear(sel_hist);
  extern __shared__ float tile[];  // [256][C | 1]
  const int CS = C | 1;
  const int tid = threadIdx.x;
  const int NS = 256 / C;              // row segments (>= 4)
  const int RS = (256 + NS - 1) / NS;  // rows per segment
  const int seg = tid / C, col = tid - seg * C;
  const int64_t ntiles = (P + 255) / 256;
  double accI = 0.0, accS = 0.0, accN = 0.0;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t p0 = t * 256;
    const int np = (int)((P - p0) < 256 ? (P - p0) : 256);
    region_stage(logits + p0 * C, tile, np * C, C, CS, tid);
    __syncthreads();
    {
      float* row = tile + tid * CS;
      int64_t tg = -1;
      bool valid = false;
      if (tid < np) {
        tg = (int64_t)target[p0 + tid];
        valid = !NASSEG_LABEL_SKIPPED(tg, C, ignore);
      }
      if (valid) {
        float m = row[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, row[c]);
        const float xt = row[tg];
        float sum = 0.f;
        for (int c = 0; c < C; ++c) {
          const float e = expf(row[c] - m);
          row[c] = e;
          sum += e;
        }
        if (pixel_loss) pixel_loss[p0 + tid] = (m + logf(sum)) - xt;
        const float inv = 1.f / sum;
        for (int c = 0; c < C; ++c) row[c] *= inv;
        row[tg] = -row[tg];
      } else {
        if (tid < np && pixel_loss) pixel_loss[p0 + tid] = -1.f;
        for (int c = 0; c < C; ++c) row[c] = 0.f;  // (rows past the end of a ragged tile too)
      }
    }
    __syncthreads();
    float sI = 0.f, sS = 0.f, sN = 0.f;
    if (seg < NS) {
      const int r1 = (seg + 1) * RS < 256 ? (seg + 1) * RS : 256;
      for (int r = seg * RS; r < r1; ++r) {
        const float v = tile[r * CS + col];
        const float a = fabsf(v);
        const bool hit = (__float_as_uint(v) >> 31) != 0u;
        sS += a;
        sI += hit ? a : 0.f;
        sN += hit ? 1.f : 0.f;
      }
    }
    __syncthreads();
    if (seg < NS) {
      tile[(seg * 3 + 0) * C + col] = sI;
      tile[(seg * 3 + 1) * C + col] = sS;
      tile[(seg * 3 + 2) * C + col] = sN;
    }
    __syncthreads();
    if (tid < C) {
      float tI = 0.f, tS = 0.f, tN = 0.f;
      for (int s = 0; s < NS; ++s) {
        tI += tile[(s * 3 + 0) * C + tid];
        tS += tile[(s * 3 + 1) * C + tid];
        tN += tile[(s * 3 + 2) * C + tid];
      }
      accI += (double)tI;
      accS += (double)tS;
      accN += (double)tN;
    }
    __syncthreads();
  }
  if (tid < C) {
    part[((int64_t)0 * C + tid) * kRegionRows + blockIdx.x] = accI;
    part[((int64_t)1 * C + tid) * kRegionRows + blockIdx.x] = accS;
    part[((int64_t)2 * C + tid) * kRegionRows + blockIdx.x] = accN;
  }
}

// Any C, any alignment: one lane per pixel straight from memory, as ce_fwd_kernel (same pixel mapping and per-pixel
// arithmetic).  The class sums by another route: per class a butterfly over the wave, the four waves' sums through
// 3 KB of LDS in chunks of 64 classes, and the workgroup's row of `part` is accumulated in place (each element by
// the one thread that owns it, in tile order).
template <typename TL>
__global__ __launch_bounds__(256) void region_fwd_kernel(const act_t* __restrict__ logits,
                                                         const TL* __restrict__ target, int64_t P, int C, int ignore,
                                                         float* __restrict__ pixel_loss,
                                                         uint32_t* __restrict__ sel_hist, double* __restrict__ part) {
  if (sel_hist) sel_clear(sel_hist);
  __shared__ float red[4][3][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t ntiles = (P + 255) / 256;
  bool first = true;
  for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const int64_t p = tl * 256 + tid;
    const act_t* lp = logits + (p < P ? p : 0) * C;
    int64_t t = -1;
    bool valid = false;
    float m = 0.f, inv = 0.f;
    if (p < P) {
      t = (int64_t)target[p];
      valid = !NASSEG_LABEL_SKIPPED(t, C, ignore);
      if (valid) {
        m = lda1(lp);
        for (int c = 1; c < C; ++c) m = fmaxf(m, lda1(lp + c));
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += expf(lda1(lp + c) - m);
        const float lse = m + logf(s);
        if (pixel_loss) pixel_loss[p] = lse - lda1(lp + t);
        inv = 1.f / s;
      } else if (pixel_loss) {
        pixel_loss[p] = -1.f;
      }
    }
    for (int c0 = 0; c0 < C; c0 += 64) {
      const int nc = C - c0 < 64 ? C - c0 : 64;
      for (int j = 0; j < nc; ++j) {
        const int c = c0 + j;
        const float q = valid ? expf(lda1(lp + c) - m) * inv : 0.f;
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

// dlogits = gscale * [cross-entropy part of nasseg_ce_sel_bwd (kept pixels) + rweight * q (G - sum_c G_c q_c)] with
// G_c = coef[C + c] + [c == t] coef[c] (G up to a constant, which cancels), on every valid pixel; exact zeros on the
// others; written once.  Tiled form:
// staging, softmax and the coalesced store of ce_tile_kernel<BWD, SEL>.
template <typename TL>
__global__ __launch_bounds__(256) void region_tile_bwd_kernel(const act_t* __restrict__ logits,
                                                              const TL* __restrict__ target, int64_t P, int C,
                                                              int ignore, const float* __restrict__ weight,
                                                              const float* __restrict__ pixel_loss,
                                                              const float* __restrict__ stats,
                                                              const float* __restrict__ coef,
                                                              const float* __restrict__ gscale, int with_ce,
                                                              float rweight, act_t* __restrict__ dlogits) {
  extern __shared__ float tile[];  // [256][C | 1]
  const int CS = C | 1;
  const int tid = threadIdx.x;
  const int64_t ntiles = (P + 255) / 256;
  const float g = gscale ? gscale[0] : 1.f;
  const float gr = g * rweight;
  const float sumw = with_ce ? stats[0] : 1.f, tau = with_ce ? stats[1] : 0.f;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t p0 = t * 256;
    const int np = (int)((P - p0) < 256 ? (P - p0) : 256);
    const int nel = np * C;
    const int nel4 = nel >> 2;
    float pl = -1.f;
    if (with_ce && tid < np) pl = pixel_loss[p0 + tid];
    region_stage(logits + p0 * C, tile, nel, C, CS, tid);
    __syncthreads();
    if (tid < np) {
      float* row = tile + tid * CS;
      const int64_t tg = (int64_t)target[p0 + tid];
      if (NASSEG_LABEL_SKIPPED(tg, C, ignore)) {
        for (int c = 0; c < C; ++c) row[c] = 0.f;
      } else {
        const bool kept = with_ce && sel_kept(pl, tau);
        const float gp = kept ? (g * (weight ? weight[tg] : 1.f)) / sumw : 0.f;
        float m = row[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, row[c]);
        float sum = 0.f, dot = 0.f;
        for (int c = 0; c < C; ++c) {
          const float e = expf(row[c] - m);
          row[c] = e;
          sum += e;
          dot = fmaf(coef[C + c], e, dot);
        }
        const float inv = 1.f / sum;
        dot = fmaf(coef[tg], row[tg], dot) * inv;
        for (int c = 0; c < C; ++c) {
          const bool y = (int64_t)c == tg;
          // (fmaf: the contraction the compiler makes of ce_tile_kernel's `row[c] * inv - onehot`)
          const float ce = kept ? gp * fmaf(row[c], inv, y ? -1.f : -0.f) : 0.f;
          const float G = coef[C + c] + (y ? coef[c] : 0.f);
          row[c] = fmaf(gr, (row[c] * inv) * (G - dot), ce);
        }
      }
    }
    __syncthreads();
    act_t* dst = dlogits + p0 * C;
    for (int i = tid; i < nel4; i += 256) {
      int pix = (4 * i) / C;
      int c = 4 * i - pix * C;
      float e[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        e[r] = tile[pix * CS + c];
        if (++c == C) {
          c = 0;
          ++pix;
        }
      }
      sta4(dst + 4 * i, make_float4(e[0], e[1], e[2], e[3]));
    }
    for (int i = 4 * nel4 + tid; i < nel; i += 256) {
      const int pix = i / C;
      sta1(dst + i, tile[pix * CS + (i - pix * C)]);
    }
    __syncthreads();
  }
}

// ... and one lane per pixel, as ce_bwd_kernel<SEL>.
template <typename TL>
__global__ __launch_bounds__(256) void region_bwd_kernel(const act_t* __restrict__ logits,
                                                         const TL* __restrict__ target, int64_t P, int C, int ignore,
                                                         const float* __restrict__ weight,
                                                         const float* __restrict__ pixel_loss,
                                                         const float* __restrict__ stats,
                                                         const float* __restrict__ coef,
                                                         const float* __restrict__ gscale, int with_ce, float rweight,
                                                         act_t* __restrict__ dlogits) {
  const float g = gscale ? gscale[0] : 1.f;
  const float gr = g * rweight;
  const float sumw = with_ce ? stats[0] : 1.f, tau = with_ce ? stats[1] : 0.f;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    const int64_t t = (int64_t)target[p];
    const act_t* lp = logits + p * C;
    act_t* dp = dlogits + p * C;
    if (NASSEG_LABEL_SKIPPED(t, C, ignore)) {
      for (int c = 0; c < C; ++c) sta1(dp + c, 0.f);
      continue;
    }
    const bool kept = with_ce && sel_kept(pixel_loss[p], tau);
    const float gp = kept ? (g * (weight ? weight[t] : 1.f)) / sumw : 0.f;
    float m = lda1(lp);
    for (int c = 1; c < C; ++c) m = fmaxf(m, lda1(lp + c));
    float s = 0.f, dot = 0.f;
    for (int c = 0; c < C; ++c) {
      const float e = expf(lda1(lp + c) - m);
      s += e;
      dot = fmaf(coef[C + c], e, dot);
    }
    const float inv = 1.f / s;
    dot = fmaf(coef[t], expf(lda1(lp + t) - m), dot) * inv;
    for (int c = 0; c < C; ++c) {
      const bool y = (int64_t)c == t;
      const float e = expf(lda1(lp + c) - m);
      const float sm = e * inv;
      const float ce = kept ? gp * fmaf(e, inv, y ? -1.f : -0.f) : 0.f;  // (as above, for ce_bwd_kernel)
      const float G = coef[C + c] + (y ? coef[c] : 0.f);
      sta1(dp + c, fmaf(gr, sm * (G - dot), ce));
    }
  }
}

// ---------------------------------------------------------------------------
// berHu (reverse Huber) loss for the depth head (BASELINE config 5).  Not present in
// the reference ("parity unpinned"): Laina et al. 2016, eq. 2 -
//   B(d) = |d| if |d| <= c else (d^2 + c^2) / (2c),  c = 0.2 * max|d| over the batch,
// mean over all elements; c is treated as a constant in the backward pass.
// Three tiny passes: block maxima -> c, block sums -> mean.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void berhu_max_kernel(const act_t* __restrict__ pred,
                                                        const act_t* __restrict__ target, int64_t n,
                                                        float* __restrict__ partial) {
  __shared__ float red[256];
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    m = fmaxf(m, fabsf(lda1(pred + i) - lda1(target + i)));
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void berhu_sum_kernel(const act_t* __restrict__ pred,
                                                        const act_t* __restrict__ target, int64_t n,
                                                        const float* __restrict__ maxpart, int nblk,
                                                        float* __restrict__ partial,
                                                        float* __restrict__ out) {
  __shared__ float red[256];
  __shared__ float cs;
  if (threadIdx.x == 0) {
    float m = 0.f;
    for (int b = 0; b < nblk; ++b) m = fmaxf(m, maxpart[b]);
    cs = 0.2f * m;
    if (blockIdx.x == 0) out[1] = cs;
  }
  __syncthreads();
  const float c = cs;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float d = fabsf(lda1(pred + i) - lda1(target + i));
    acc += (d <= c) ? d : (d * d + c * c) / (2.f * c);
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ void berhu_finalize_kernel(const float* __restrict__ partial, int nblk, double n,
                                      float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += (double)partial[b];
  out[0] = (float)(s / n);
}

// dpred = g/n * (sign(diff) if |diff| <= c else diff / c)
__global__ __launch_bounds__(256) void berhu_bwd_kernel(const act_t* __restrict__ pred,
                                                        const act_t* __restrict__ target,
                                                        const float* __restrict__ stats,
                                                        const float* __restrict__ gscale, int64_t n,
                                                        act_t* __restrict__ dpred) {
  const float c = stats[1];
  const float g = (gscale ? gscale[0] : 1.f) / (float)n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float d = lda1(pred + i) - lda1(target + i);
    const float ad = fabsf(d);
    const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    sta1(dpred + i, g * ((ad <= c) ? sgn : d / c));
  }
}

// the selection's launches: [zero the histograms, unless an earlier launch did,] 3 x (histogram, scan); tau[0] and
// counts[0..2] = {k, n, 0} after
int sel_launch(const float* v, int64_t P, float t_loss, int64_t min_kept, double keep_fraction, float* tau,
               int64_t* counts, void* ws, bool zeroed, hipStream_t s) {
  uint32_t* hist = (uint32_t*)ws;
  SelState* st = (SelState*)(hist + kSelHistWords);
  const int grid = ce_grid(P);
  if (!zeroed) {
    hipLaunchKernelGGL(sel_zero_kernel, dim3(6), dim3(256), 0, s, hist);
    NASSEG_LAUNCH_CHECK("sel_zero");
  }
  hipLaunchKernelGGL(sel_hist_kernel<0>, dim3(grid), dim3(256), 0, s, v, P, st, hist);
  hipLaunchKernelGGL(sel_scan_kernel<0>, dim3(1), dim3(256), 0, s, hist, st, t_loss, min_kept, keep_fraction, tau,
                     counts);
  NASSEG_LAUNCH_CHECK("sel_pass0");
  hipLaunchKernelGGL(sel_hist_kernel<1>, dim3(grid), dim3(256), 0, s, v, P, st, hist);
  hipLaunchKernelGGL(sel_scan_kernel<1>, dim3(1), dim3(256), 0, s, hist, st, t_loss, min_kept, keep_fraction, tau,
                     counts);
  NASSEG_LAUNCH_CHECK("sel_pass1");
  hipLaunchKernelGGL(sel_hist_kernel<2>, dim3(grid), dim3(256), 0, s, v, P, st, hist);
  hipLaunchKernelGGL(sel_scan_kernel<2>, dim3(1), dim3(256), 0, s, hist, st, t_loss, min_kept, keep_fraction, tau,
                     counts);
  NASSEG_LAUNCH_CHECK("sel_pass2");
  return NASSEG_OK;
}

// ... as ce_sel_reduce's `selection`, behind a forward kernel that cleared the histograms on its way
auto sel_after_clear(const float* v, int64_t P, float t_loss, int64_t min_kept, double keep_fraction, void* ws,
                     hipStream_t s) {
  return [=](float* tau, int64_t* counts) {
    return sel_launch(v, P, t_loss, min_kept, keep_fraction, tau, counts, ws, true, s);
  };
}

}  // namespace

extern "C" {

#if NASSEG_FP32_ONLY
int64_t nasseg_ce_workspace(void) { return 2 * kCeGridCap; }
int64_t nasseg_ce_mse_workspace(void) { return 3 * kCeGridCap; }
int64_t nasseg_ohem_workspace(void) { return kSelWsWords; }
int64_t nasseg_ce_sel_workspace(void) { return 3 * kCeGridCap + kSelWsWords; }

// tau = min(t_loss, k-th largest of the entries of pixel_loss that are >= 0), k = min(n, max(min_kept,
// ceil(keep_fraction * n))) with n = the number of such entries; counts = {k, n, entries >= tau among them}.
// ws: nasseg_ohem_workspace() 4-byte words.
int nasseg_ohem_threshold(const float* pixel_loss, int64_t P, float t_loss, int64_t min_kept, double keep_fraction,
                          float* tau, int64_t* counts, void* ws, void* stream) {
  NASSEG_REQUIRE(P > 0 && P < ((int64_t)1 << 32), "ohem_threshold: bad size");
  NASSEG_REQUIRE(min_kept >= 1 && keep_fraction >= 0.0 && keep_fraction <= 1.0,
                 "ohem_threshold: min_kept >= 1 and 0 <= keep_fraction <= 1 expected");
  NASSEG_REQUIRE(pixel_loss && tau && counts && ws, "ohem_threshold: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int rc = sel_launch(pixel_loss, P, t_loss, min_kept, keep_fraction, tau, counts, ws, false, s);
  if (rc != NASSEG_OK) return rc;
  hipLaunchKernelGGL(sel_count_kernel, dim3(ce_grid(P)), dim3(256), 0, s, pixel_loss, P, tau, counts);
  NASSEG_LAUNCH_CHECK("sel_count");
  return NASSEG_OK;
}
#endif

// Class-weighted cross-entropy with hard-example selection (include/nasseg.h).  One pass over the logits writes
// pixel_loss; the selection and the sum pass read pixel_loss (and the labels) only.
// ws: nasseg_ce_sel_workspace() floats = [1024][3] partials | the selection's words.
int NASSEG_FN(ce_sel_fwd)(const act_t* logits, const void* target, int elem_size, const float* weight, int64_t P,
                          int C, int ignore, int select, float t_loss, int64_t min_kept, double keep_fraction,
                          float* loss, float* stats, int64_t* counts, float* pixel_loss, float* ws, void* stream) {
  NASSEG_TRY(check_shape("ce_sel_fwd", P, C, true));
  NASSEG_TRY(check_elem_size("ce_sel_fwd", elem_size));
  NASSEG_REQUIRE(logits && target && loss && stats && counts && pixel_loss && ws, "ce_sel_fwd: null pointer");
  NASSEG_TRY(check_selection("ce_sel_fwd", select, min_kept, keep_fraction));
  hipStream_t s = (hipStream_t)stream;
  const CeGeom g = ce_geom(P, C, {logits});
  float* sel_ws = ws + 3 * kCeGridCap;
  uint32_t* hist = select ? (uint32_t*)sel_ws : nullptr;  // (cleared by the forward kernel on its way)
  with_labels(target, elem_size, [&](auto labels) {
    using TL = label_of<decltype(labels)>;
    if (g.tiled)
      hipLaunchKernelGGL((ce_tile_kernel<TL, false, false, true>), dim3(g.fwd), dim3(256), g.lds, s, logits, labels, P,
                         C, ignore, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, pixel_loss,
                         hist);
    else
      hipLaunchKernelGGL((ce_fwd_kernel<TL, false, true>), dim3(g.fwd), dim3(256), 0, s, logits, labels, P, C, ignore,
                         nullptr, nullptr, nullptr, pixel_loss, hist);
  });
  NASSEG_LAUNCH_CHECK("ce_sel_fwd");
  return ce_sel_reduce("ce_sel_sum", "ce_sel_finalize", sel_after_clear(pixel_loss, P, t_loss, min_kept, keep_fraction,
                                                                        sel_ws, s),
                       pixel_loss, target, elem_size, weight, P, select, loss, stats, counts, ws, s);
}

// dlogits = gscale * weight[t] * (softmax - onehot) / stats[0] for the pixels kept at stats[1] (pixel_loss, stats:
// from nasseg_ce_sel_fwd), exact zeros elsewhere; written once.
int NASSEG_FN(ce_sel_bwd)(const act_t* logits, const void* target, int elem_size, const float* weight,
                          const float* pixel_loss, const float* stats, const float* gscale, int64_t P, int C,
                          int ignore, act_t* dlogits, void* stream) {
  NASSEG_TRY(check_shape("ce_sel_bwd", P, C, false));
  NASSEG_TRY(check_elem_size("ce_sel_bwd", elem_size));
  NASSEG_REQUIRE(logits && target && pixel_loss && stats && dlogits, "ce_sel_bwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const CeGeom g = ce_geom(P, C, {logits, dlogits});
  float* pl = const_cast<float*>(pixel_loss);  // (the tiled kernel's one parameter for both directions; backward reads)
  with_labels(target, elem_size, [&](auto labels) {
    using TL = label_of<decltype(labels)>;
    if (g.tiled)
      hipLaunchKernelGGL((ce_tile_kernel<TL, true, false, true>), dim3(g.tiles), dim3(256), g.lds, s, logits, labels, P,
                         C, ignore, nullptr, stats, gscale, dlogits, nullptr, nullptr, nullptr, weight, pl);
    else
      hipLaunchKernelGGL((ce_bwd_kernel<TL, false, true>), dim3(g.bwd), dim3(256), 0, s, logits, labels, stats, gscale,
                         P, C, ignore, dlogits, nullptr, nullptr, weight, pixel_loss);
  });
  NASSEG_LAUNCH_CHECK("ce_sel_bwd");
  return NASSEG_OK;
}

// Cross-entropy of nasseg_ce_sel_fwd plus the region-overlap term (include/nasseg.h), the logits read once.
// ws: nasseg_ce_region_workspace(C) floats = nasseg_ce_sel_workspace()'s | fp64 part[3][C][1024] | fp64 tot[3][C].
#if NASSEG_FP32_ONLY
int64_t nasseg_ce_region_workspace(int C) {
  if (C < 1) return 0;
  return 3 * kCeGridCap + kSelWsWords + 2 * ((int64_t)3 * C * kRegionRows + (int64_t)3 * C);
}
#endif

int NASSEG_FN(ce_region_fwd)(const act_t* logits, const void* target, int elem_size, const float* weight, int64_t P,
                             int C, int ignore, int with_ce, int select, float t_loss, int64_t min_kept,
                             double keep_fraction, double alpha, double beta, double smooth, int all_classes,
                             double region_weight, float* loss, float* loss_ce, float* loss_region, float* stats,
                             int64_t* counts, float* pixel_loss, float* coef, float* sums, int64_t* ncls, float* ws,
                             void* stream) {
  NASSEG_TRY(check_shape("ce_region_fwd", P, C, true));
  NASSEG_TRY(check_elem_size("ce_region_fwd", elem_size));
  NASSEG_REQUIRE(logits && target && loss && loss_ce && loss_region && coef && sums && ncls && ws,
                 "ce_region_fwd: null pointer");
  NASSEG_REQUIRE(!with_ce || (stats && counts && pixel_loss), "ce_region_fwd: null pointer");
  NASSEG_REQUIRE(with_ce || !select, "ce_region_fwd: selection without the cross-entropy");
  NASSEG_TRY(check_selection("ce_region_fwd", select, min_kept, keep_fraction));
  NASSEG_REQUIRE(alpha >= 0.0 && beta >= 0.0 && alpha + beta > 0.0 && smooth >= 0.0,
                 "ce_region_fwd: alpha, beta, smooth >= 0 and alpha + beta > 0 expected");
  NASSEG_REQUIRE(!all_classes || smooth > 0.0, "ce_region_fwd: all classes need smooth > 0");
  static_assert((3 * kCeGridCap + kSelWsWords) % 2 == 0, "the fp64 part of the workspace is 8-byte aligned");
  NASSEG_REQUIRE(((uintptr_t)ws & 7) == 0, "ce_region_fwd: the workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const CeGeom g = ce_geom(P, C, {logits});  // (g.fwd <= kRegionRows)
  float* sel_ws = ws + 3 * kCeGridCap;
  uint32_t* hist = select ? (uint32_t*)sel_ws : nullptr;  // (cleared by the forward kernel on its way)
  double* part = (double*)(sel_ws + kSelWsWords);
  double* tot = part + (int64_t)3 * C * kRegionRows;
  float* pl = with_ce ? pixel_loss : nullptr;
  with_labels(target, elem_size, [&](auto labels) {
    using TL = label_of<decltype(labels)>;
    if (g.tiled)
      hipLaunchKernelGGL(region_tile_fwd_kernel<TL>, dim3(g.fwd), dim3(256), g.lds, s, logits, labels, P, C, ignore, pl,
                         hist, part);
    else
      hipLaunchKernelGGL(region_fwd_kernel<TL>, dim3(g.fwd), dim3(256), 0, s, logits, labels, P, C, ignore, pl, hist,
                         part);
  });
  NASSEG_LAUNCH_CHECK("ce_region_fwd");
  if (with_ce)  // (the finalizer below reads the partials)
    NASSEG_TRY(ce_sel_reduce("ce_region_sum", nullptr, sel_after_clear(pixel_loss, P, t_loss, min_kept, keep_fraction,
                                                                       sel_ws, s),
                             pixel_loss, target, elem_size, weight, P, select, nullptr, stats, counts, ws, s));
  hipLaunchKernelGGL(region_finalize_kernel, dim3(1), dim3(1024), 0, s, ws, part, g.fwd, C, with_ce, select, alpha,
                     beta, smooth, all_classes, region_weight, loss, loss_ce, loss_region, stats, counts, coef, sums,
                     ncls, tot);
  NASSEG_LAUNCH_CHECK("ce_region_finalize");
  return NASSEG_OK;
}

int NASSEG_FN(ce_region_bwd)(const act_t* logits, const void* target, int elem_size, const float* weight,
                             const float* pixel_loss, const float* stats, const float* coef, const float* gscale,
                             int with_ce, double region_weight, int64_t P, int C, int ignore, act_t* dlogits,
                             void* stream) {
  NASSEG_TRY(check_shape("ce_region_bwd", P, C, false));
  NASSEG_TRY(check_elem_size("ce_region_bwd", elem_size));
  NASSEG_REQUIRE(logits && target && coef && dlogits, "ce_region_bwd: null pointer");
  NASSEG_REQUIRE(!with_ce || (pixel_loss && stats), "ce_region_bwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const CeGeom g = ce_geom(P, C, {logits, dlogits});
  const float rw = (float)region_weight;
  with_labels(target, elem_size, [&](auto labels) {
    using TL = label_of<decltype(labels)>;
    if (g.tiled)
      hipLaunchKernelGGL(region_tile_bwd_kernel<TL>, dim3(g.tiles), dim3(256), g.lds, s, logits, labels, P, C, ignore,
                         weight, pixel_loss, stats, coef, gscale, with_ce, rw, dlogits);
    else
      hipLaunchKernelGGL(region_bwd_kernel<TL>, dim3(g.bwd), dim3(256), 0, s, logits, labels, P, C, ignore, weight,
                         pixel_loss, stats, coef, gscale, with_ce, rw, dlogits);
  });
  NASSEG_LAUNCH_CHECK("ce_region_bwd");
  return NASSEG_OK;
}

// logits [P][C] dense NHWC, target [P] (elem_size 1 = uint8, 8 = int64).
// out[0] = mean NLL over valid pixels, out[1] = valid count. ws: nasseg_ce_workspace() floats.
int NASSEG_FN(ce_fwd)(const act_t* logits, const void* target, int elem_size, int64_t P, int C,
                  int ignore, float* out, float* ws, void* stream) {
  NASSEG_TRY(check_shape("ce_fwd", P, C, false));
  NASSEG_TRY(check_elem_size("ce_fwd", elem_size));
  hipStream_t s = (hipStream_t)stream;
  const CeGeom g = ce_geom(P, C, {logits});
  with_labels(target, elem_size, [&](auto labels) {
    using TL = label_of<decltype(labels)>;
    if (g.tiled)
      hipLaunchKernelGGL((ce_tile_kernel<TL, false>), dim3(g.fwd), dim3(256), g.lds, s, logits, labels, P, C, ignore,
                         ws, nullptr, nullptr, nullptr);
    else
      hipLaunchKernelGGL((ce_fwd_kernel<TL>), dim3(g.fwd), dim3(256), 0, s, logits, labels, P, C, ignore, ws);
  });
  NASSEG_LAUNCH_CHECK("ce_fwd");
  hipLaunchKernelGGL(ce_finalize_kernel<false>, dim3(1), dim3(256), 0, s, ws, g.fwd, out, nullptr, 0.0, nullptr,
                     nullptr);
  NASSEG_LAUNCH_CHECK("ce_finalize");
  return NASSEG_OK;
}

// stats = out of nasseg_ce_fwd; gscale = device scalar upstream gradient (null = 1)
int NASSEG_FN(ce_bwd)(const act_t* logits, const void* target, int elem_size, const float* stats,
                  const float* gscale, int64_t P, int C, int ignore, act_t* dlogits, void* stream) {
  NASSEG_TRY(check_shape("ce_bwd", P, C, false));
  NASSEG_TRY(check_elem_size("ce_bwd", elem_size));
  hipStream_t s = (hipStream_t)stream;
  const CeGeom g = ce_geom(P, C, {logits, dlogits});
  with_labels(target, elem_size, [&](auto labels) {
    using TL = label_of<decltype(labels)>;
    if (g.tiled)
      hipLaunchKernelGGL((ce_tile_kernel<TL, true>), dim3(g.tiles), dim3(256), g.lds, s, logits, labels, P, C, ignore,
                         nullptr, stats, gscale, dlogits);
    else
      hipLaunchKernelGGL((ce_bwd_kernel<TL>), dim3(g.bwd), dim3(256), 0, s, logits, labels, stats, gscale, P, C,
                         ignore, dlogits);
  });
  NASSEG_LAUNCH_CHECK("ce_bwd");
  return NASSEG_OK;
}

// Softmax-NLL and the distillation term nn.MSELoss()(logits, teacher) of one decoder-only step
// (src/engine/trainer.py:144-149) from one pass over the logits: ce[0] = the NLL exactly as nasseg_ce_fwd computes
// it, mse[0] = sum((x - t)^2) / (P*C) over ALL elements (ignored pixels too), stats = nasseg_ce_fwd's out.
// teacher: fp32 [P][C] (the task0 cache's kd_y, whatever the logits' storage).  ws: nasseg_ce_mse_workspace() floats.
int NASSEG_FN(ce_mse_fwd)(const act_t* logits, const void* target, int elem_size, const float* teacher, int64_t P,
                          int C, int ignore, float* ce, float* mse, float* stats, float* ws, void* stream) {
  NASSEG_TRY(check_shape("ce_mse_fwd", P, C, false));
  NASSEG_TRY(check_elem_size("ce_mse_fwd", elem_size));
  NASSEG_REQUIRE(logits && target && teacher && ce && mse && stats && ws, "ce_mse_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const CeGeom g = ce_geom(P, C, {logits, teacher});
  float* sqpart = ws + 2 * kCeGridCap;  // (ws = [1024][2] NLL partials | [1024] squared-difference partials)
  with_labels(target, elem_size, [&](auto labels) {
    using TL = label_of<decltype(labels)>;
    if (g.tiled)
      hipLaunchKernelGGL((ce_tile_kernel<TL, false, true>), dim3(g.fwd), dim3(256), g.lds, s, logits, labels, P, C,
                         ignore, ws, nullptr, nullptr, nullptr, teacher, nullptr, sqpart);
    else
      hipLaunchKernelGGL((ce_fwd_kernel<TL, true>), dim3(g.fwd), dim3(256), 0, s, logits, labels, P, C, ignore, ws,
                         teacher, sqpart);
  });
  NASSEG_LAUNCH_CHECK("ce_mse_fwd");
  hipLaunchKernelGGL(ce_finalize_kernel<true>, dim3(1), dim3(256), 0, s, ws, g.fwd, stats, sqpart,
                     (double)P * (double)C, ce, mse);
  NASSEG_LAUNCH_CHECK("ce_mse_finalize");
  return NASSEG_OK;
}

// dlogits = g_ce[0] * dNLL + g_mse[0] * 2 (x - teacher) / (P*C), written once (stats: from nasseg_ce_mse_fwd;
// g_ce / g_mse: device scalars, null = 1).  With g_mse = 0 it equals nasseg_ce_bwd's result.
int NASSEG_FN(ce_mse_bwd)(const act_t* logits, const void* target, int elem_size, const float* teacher,
                          const float* stats, const float* g_ce, const float* g_mse, int64_t P, int C, int ignore,
                          act_t* dlogits, void* stream) {
  NASSEG_TRY(check_shape("ce_mse_bwd", P, C, false));
  NASSEG_TRY(check_elem_size("ce_mse_bwd", elem_size));
  NASSEG_REQUIRE(logits && target && teacher && stats && dlogits, "ce_mse_bwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const CeGeom g = ce_geom(P, C, {logits, dlogits, teacher});
  with_labels(target, elem_size, [&](auto labels) {
    using TL = label_of<decltype(labels)>;
    if (g.tiled)
      hipLaunchKernelGGL((ce_tile_kernel<TL, true, true>), dim3(g.tiles), dim3(256), g.lds, s, logits, labels, P, C,
                         ignore, nullptr, stats, g_ce, dlogits, teacher, g_mse, nullptr);
    else
      hipLaunchKernelGGL((ce_bwd_kernel<TL, true>), dim3(g.bwd), dim3(256), 0, s, logits, labels, stats, g_ce, P, C,
                         ignore, dlogits, teacher, g_mse);
  });
  NASSEG_LAUNCH_CHECK("ce_mse_bwd");
  return NASSEG_OK;
}

// berHu loss (depth head): out[0] = mean loss, out[1] = c = 0.2 * max|pred - target|.
// pred / target: n fp32 elements, any layout (elementwise).  ws: nasseg_ce_workspace() floats.
int NASSEG_FN(berhu_fwd)(const act_t* pred, const act_t* target, int64_t n, float* out, float* ws,
                     void* stream) {
  NASSEG_REQUIRE(n > 0, "berhu_fwd: empty input");
  hipStream_t s = (hipStream_t)stream;
  const int grid = ce_grid(n);
  hipLaunchKernelGGL(berhu_max_kernel, dim3(grid), dim3(256), 0, s, pred, target, n, ws);
  NASSEG_LAUNCH_CHECK("berhu_max");
  hipLaunchKernelGGL(berhu_sum_kernel, dim3(grid), dim3(256), 0, s, pred, target, n, ws, grid,
                     ws + 1024, out);
  NASSEG_LAUNCH_CHECK("berhu_sum");
  hipLaunchKernelGGL(berhu_finalize_kernel, dim3(1), dim3(64), 0, s, ws + 1024, grid, (double)n, out);
  NASSEG_LAUNCH_CHECK("berhu_finalize");
  return NASSEG_OK;
}

int NASSEG_FN(berhu_bwd)(const act_t* pred, const act_t* target, const float* stats,
                     const float* gscale, int64_t n, act_t* dpred, void* stream) {
  NASSEG_REQUIRE(n > 0, "berhu_bwd: empty input");
  hipLaunchKernelGGL(berhu_bwd_kernel, dim3(ce_grid(n) * 2), dim3(256), 0, (hipStream_t)stream, pred,
                     target, stats, gscale, n, dpred);
  NASSEG_LAUNCH_CHECK("berhu_bwd");
  return NASSEG_OK;
}

}  // extern "C"
