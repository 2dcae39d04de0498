// What the segmentation losses share (csrc/loss.hip, csrc/loss_up.hip, csrc/lovasz.hip): the predicates every kernel
// must agree on, the sum pass and the finalizer over per-pixel losses, and the host side of a launch - dispatch over
// the label type, launch geometry, argument checks.  Like the .hip files, compiled for both activation storages.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "common.h"

namespace {

// Is a per-pixel loss that takes part (l >= 0; -1 marks the others) kept at threshold tau?  l >= tau on the fp32
// values, compared through their bit patterns (for non-negative floats the order of the patterns is the order of
// the values) so that the answer is the same integer comparison the radix selection (csrc/loss.hip) made, denormals
// included.
__device__ __forceinline__ bool sel_kept(float l, float tau) {
  if (l < 0.f) return false;
  return !(tau > 0.f) || __float_as_uint(l) >= __float_as_uint(tau);
}

// Does the pixel with label t (int64_t) stay out of the loss?  Out-of-range labels are skipped, never read.
// A macro for the kernels that had the expression in their bodies: through a function the compiler orders the
// operands of one scalar `and` the other way round, and these kernels' instruction streams are pinned.
#define NASSEG_LABEL_SKIPPED(t, C, ignore) ((t) == (ignore) || (t) < 0 || (t) >= (C))
__device__ __forceinline__ bool label_valid(int64_t t, int C, int ignore) {
  return !NASSEG_LABEL_SKIPPED(t, C, ignore);
}

// A ROW TABLE over the labels (nasseg_ce_up_rows_*; as RowTable of csrc/depth.hip): the labels are a cache
// [n_rows][hw] and image b of the batch is its row rows[b], clamped to the cache as nasseg_gather_rows clamps it (a
// memory-safety net: the host checks).  The kernels that read labels take it as a trailing parameter pack `Rows... lr`
// that is empty or one LabelRows: empty, image b of the labels is image b and the kernel - the one the un-indexed
// entry points launch - has neither an argument nor an instruction for it.
struct LabelRows {
  const int64_t* rows;
  int64_t n_rows;
  uint32_t hw;  // label pixels per image (the batch holds fewer than 2^32)
};

template <typename TL>
__device__ __forceinline__ const TL* label_image(const TL* __restrict__ target, int64_t b, const LabelRows& lr) {
  int64_t r = lr.rows[b];
  r = r < 0 ? 0 : (r >= lr.n_rows ? lr.n_rows - 1 : r);
  return target + r * (int64_t)lr.hw;  // (64-bit: the cache may hold more than 2^32 pixels)
}

// the base from which pixel p of the BATCH (its flat index, image b's among them) has its label at base[p]: the cache
// image's start less b images.  Formed as an integer - the base itself may lie outside the cache, base[p] never does.
template <typename TL>
__device__ __forceinline__ const TL* label_base(const TL* __restrict__ target, int64_t b, const LabelRows& lr) {
  const uintptr_t image = reinterpret_cast<uintptr_t>(label_image(target, b, lr));
  return reinterpret_cast<const TL*>(image - (uintptr_t)(b * (int64_t)lr.hw) * sizeof(TL));
}

// pixel p of the batch (p < 2^32 with a table) -> its image b, and returned its offset within the image
__device__ __forceinline__ uint32_t label_decode(uint32_t p, int& b, const LabelRows& lr) {
  const uint32_t i = p / lr.hw;
  b = (int)i;
  return p - i * lr.hw;
}

// label of pixel p of the batch: the batch's own, or - with a table - that of the cache image its image selects
template <typename TL>
__device__ __forceinline__ int64_t label_at(const TL* __restrict__ target, int64_t p) {
  return (int64_t)target[p];
}
template <typename TL>
__device__ __forceinline__ int64_t label_at(const TL* __restrict__ target, int64_t p, const LabelRows& lr) {
  int b;
  const uint32_t off = label_decode((uint32_t)p, b, lr);
  return (int64_t)label_image(target, (int64_t)b, lr)[off];
}

constexpr int kCeGridCap = 1024;  // workgroups of a pass over the pixels = rows of its partials
constexpr int kCeTileMaxC = 63;   // classes up to which a tile of 256 pixels is staged through LDS

#ifndef NASSEG_LOSS_NO_SUM_PASS  // (a source that sums no per-pixel losses keeps the kernels out of its code object)
// Sum pass over pixel_loss + labels: partial[b] = {sum w l, sum w, count} over the kept pixels of workgroup b, with
// the pixel -> (workgroup, thread) mapping, the accumulation order and the tree of ce_fwd_kernel: with unit weights
// and everything kept, the very sums of nasseg_ce_fwd.  tau == nullptr: no selection, every valid pixel is kept.
// lr: the labels behind a row table (P < 2^32) - only the address of a pixel's label differs.
template <typename TL, typename... Rows>
__global__ __launch_bounds__(256) void ce_sel_sum_kernel(const float* __restrict__ pixel_loss,
                                                         const TL* __restrict__ target,
                                                         const float* __restrict__ weight, int64_t P,
                                                         const float* __restrict__ tau,
                                                         float* __restrict__ partial, Rows... lr) {
  __shared__ float red_l[256];
  __shared__ float red_w[256];
  __shared__ float red_n[256];
  const float t = tau ? tau[0] : 0.f;
  float loss = 0.f, sw = 0.f, cnt = 0.f;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    const float l = pixel_loss[p];
    if (!sel_kept(l, t)) continue;
    const float w = weight ? weight[label_at(target, p, lr...)] : 1.f;  // (l >= 0: the label is in [0, C))
    loss += w * l;
    sw += w;
    cnt += 1.f;
  }
  red_l[threadIdx.x] = loss;
  red_w[threadIdx.x] = sw;
  red_n[threadIdx.x] = cnt;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red_l[threadIdx.x] += red_l[threadIdx.x + s];
      red_w[threadIdx.x] += red_w[threadIdx.x + s];
      red_n[threadIdx.x] += red_n[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[blockIdx.x * 3] = red_l[0];
    partial[blockIdx.x * 3 + 1] = red_w[0];
    partial[blockIdx.x * 3 + 2] = red_n[0];
  }
}

// loss = sum w l / sum w, stats = {sum w, tau}, counts[2] = kept pixels (selected: counts[0..1] and stats[1] are
// the selection's; else k = n = kept and tau = -inf); fp64, the order of ce_finalize_kernel.
__global__ __launch_bounds__(256) void ce_sel_finalize_kernel(const float* __restrict__ partial, int nblk,
                                                              int selected, float* __restrict__ loss,
                                                              float* __restrict__ stats,
                                                              int64_t* __restrict__ counts) {
  __shared__ double red_l[256];
  __shared__ double red_w[256];
  __shared__ double red_n[256];
  double l = 0.0, w = 0.0, n = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) {
    l += (double)partial[b * 3];
    w += (double)partial[b * 3 + 1];
    n += (double)partial[b * 3 + 2];
  }
  red_l[threadIdx.x] = l;
  red_w[threadIdx.x] = w;
  red_n[threadIdx.x] = n;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red_l[threadIdx.x] += red_l[threadIdx.x + s];
      red_w[threadIdx.x] += red_w[threadIdx.x + s];
      red_n[threadIdx.x] += red_n[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    loss[0] = (float)(red_l[0] / red_w[0]);
    stats[0] = (float)red_w[0];
    counts[2] = (int64_t)red_n[0];
    if (!selected) {
      stats[1] = -__builtin_inff();
      counts[0] = counts[1] = (int64_t)red_n[0];
    }
  }
}

// The region-overlap term (nasseg_ce_region_*: csrc/loss.hip; nasseg_ce_up_region_*: csrc/loss_up.hip): the forward
// kernels of both write per-workgroup fp64 rows part[3][C][kRegionRows] = I | S | N, and one finalize adds them.
constexpr int kRegionRows = kCeGridCap;  // (a row per workgroup of the forward)

__device__ __forceinline__ float wave_allsum(float v) {  // (a fixed butterfly: the same pairing every time)
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ double wave_allsum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// One workgroup of 1024 threads.  1. with_ce: the statements of ce_sel_finalize_kernel, by the first 256 threads, on
// the sum pass's partials (lce, stats, counts: bit-identical to nasseg_ce_sel_fwd's).  2. wave w of 16 adds rows
// 0 .. nblk-1 of part for the elements w, w + 16, ...: each lane its <= 16 rows, all loads in flight at once, added
// in row order, then the butterfly -> tot[3][C].  3. per class T_c and the members of K; sum T and |K| by a tree;
// lreg = 1 - sum T / |K| (0 when K is empty), loss = [lce +] rweight * lreg, and for backward
// coef = {-a_c / |K|} | {-b_c / |K| - their mean over the C classes} (outside K: a_c = b_c = 0).  All in fp64.
__global__ __launch_bounds__(1024) void region_finalize_kernel(const float* __restrict__ partial,
                                                               const double* __restrict__ part, int nblk, int C,
                                                               int with_ce, int selected, double alpha, double beta,
                                                               double smooth, int all_classes, double rweight,
                                                               float* __restrict__ loss, float* __restrict__ lce,
                                                               float* __restrict__ lreg, float* __restrict__ stats,
                                                               int64_t* __restrict__ counts, float* __restrict__ coef,
                                                               float* __restrict__ sums, int64_t* __restrict__ ncls,
                                                               double* tot) {
  __shared__ double red_l[256];
  __shared__ double red_w[256];
  __shared__ double red_n[256];
  const int tid = threadIdx.x;
  const bool head = tid < 256;
  if (with_ce) {
    if (head) {
      double l = 0.0, w = 0.0, n = 0.0;
      for (int b = tid; b < nblk; b += 256) {
        l += (double)partial[b * 3];
        w += (double)partial[b * 3 + 1];
        n += (double)partial[b * 3 + 2];
      }
      red_l[tid] = l;
      red_w[tid] = w;
      red_n[tid] = n;
    }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) {
        red_l[tid] += red_l[tid + s];
        red_w[tid] += red_w[tid + s];
        red_n[tid] += red_n[tid + s];
      }
      __syncthreads();
    }
    if (tid == 0) {
      lce[0] = (float)(red_l[0] / red_w[0]);
      stats[0] = (float)red_w[0];
      counts[2] = (int64_t)red_n[0];
      if (!selected) {
        stats[1] = -__builtin_inff();
        counts[0] = counts[1] = (int64_t)red_n[0];
      }
    }
    __syncthreads();
  } else if (tid == 0) {
    lce[0] = 0.f;
  }
  const int lane = tid & 63, wave = tid >> 6;
  for (int e = wave; e < 3 * C; e += 16) {
    const double* src = part + (int64_t)e * kRegionRows;
    double r[kRegionRows / 64];
#pragma unroll
    for (int i = 0; i < kRegionRows / 64; ++i) r[i] = lane + 64 * i < nblk ? src[lane + 64 * i] : 0.0;
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < kRegionRows / 64; ++i) v += r[i];
    v = wave_allsum(v);
    if (lane == 0) tot[e] = v;
  }
  __syncthreads();
  const double gamma = 1.0 - alpha - beta;
  double tsum = 0.0, bsum = 0.0, kcnt = 0.0;
  if (head) {
    for (int c = tid; c < C; c += 256) {
      const double I = tot[c], S = tot[C + c], N = tot[2 * C + c];
      if (all_classes || N > 0.0) {
        const double D = gamma * I + alpha * S + beta * N + smooth;
        tsum += (I + smooth) / D;
        bsum += (I + smooth) * alpha / (D * D);
        kcnt += 1.0;
      }
    }
    red_l[tid] = tsum;
    red_w[tid] = bsum;
    red_n[tid] = kcnt;
  }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      red_l[tid] += red_l[tid + s];
      red_w[tid] += red_w[tid + s];
      red_n[tid] += red_n[tid + s];
    }
    __syncthreads();
  }
  const double K = red_n[0];
  // The gradient q_j (G_j - sum_c G_c q_c) does not change when a constant is added to every G_c (sum_c q_c = 1):
  // the -b_c / |K| are stored minus their mean over the C classes, so that fp32 does not have to cancel it.
  const double bmean = K > 0.0 ? red_w[0] / K / (double)C : 0.0;
  if (head) {
    for (int c = tid; c < C; c += 256) {
      const double I = tot[c], S = tot[C + c], N = tot[2 * C + c];
      float ca = 0.f;
      double cb = 0.0;
      if (all_classes || N > 0.0) {
        const double D = gamma * I + alpha * S + beta * N + smooth;
        ca = (float)(-((D - (I + smooth) * gamma) / (D * D)) / K);
        cb = ((I + smooth) * alpha / (D * D)) / K;
      }
      coef[c] = ca;
      coef[C + c] = (float)(cb - bmean);
      sums[c] = (float)I;
      sums[C + c] = (float)S;
      ncls[c] = (int64_t)N;
    }
  }
  if (tid == 0) {
    const float lr = K > 0.0 ? (float)(1.0 - red_l[0] / K) : 0.f;
    lreg[0] = lr;
    ncls[C] = (int64_t)K;
    loss[0] = (float)((with_ce ? (double)lce[0] : 0.0) + rweight * (double)lr);
  }
}

#endif  // NASSEG_LOSS_NO_SUM_PASS

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
#define NASSEG_TRY(call)              \
  do {                                \
    const int rc_ = (call);           \
    if (rc_ != NASSEG_OK) return rc_; \
  } while (0)

// f(labels) with the labels as const int64_t* or const uint8_t*: a generic lambda names its kernel's template
// arguments and its arguments once, label_of<decltype(labels)> being the kernel's label type.
template <typename F>
inline void with_labels(const void* target, int elem_size, F&& f) {
  if (elem_size == 8)
    f((const int64_t*)target);
  else
    f((const uint8_t*)target);
}
template <typename Ptr>
using label_of = std::remove_const_t<std::remove_pointer_t<Ptr>>;

inline int ce_grid(int64_t P) {
  int64_t b = (P + 255) / 256;
  if (b > kCeGridCap) b = kCeGridCap;
  if (b < 1) b = 1;
  return (int)b;
}

// Launch geometry of the cross-entropy kernels over [P][C] logits, 256 threads each.  tiled (ce_tile_kernel and its
// kin: C <= kCeTileMaxC and every pointer of `vec`, which they touch with 16-byte accesses, so aligned): `fwd`
// workgroups forward, `tiles` backward, `lds` bytes of [256][C | 1] floats.  Else (one lane per pixel): `fwd`
// workgroups forward, `bwd` backward, no LDS.
struct CeGeom {
  int fwd, bwd;
  unsigned tiles;
  size_t lds;
  bool tiled;
};
inline CeGeom ce_geom(int64_t P, int C, std::initializer_list<const void*> vec) {
  uintptr_t bits = 0;
  for (const void* p : vec) bits |= (uintptr_t)p;
  int64_t tiles = (P + 255) / 256;
  if (tiles > 4096) tiles = 4096;
  CeGeom g;
  g.fwd = ce_grid(P);
  g.bwd = g.fwd * 2;
  g.tiles = (unsigned)tiles;
  g.lds = (size_t)256 * (C | 1) * sizeof(float);
  g.tiled = C <= kCeTileMaxC && (bits & 15) == 0;
  return g;
}

// The argument checks the entry points share.  p32: P also indexes 32-bit counters.
inline int check_shape(const char* who, int64_t P, int C, bool p32) {
  if (P > 0 && (!p32 || P < ((int64_t)1 << 32)) && C > 0) return NASSEG_OK;
  return nasseg_fail(NASSEG_ERR_ARG, "%s: bad shape", who);
}
inline int check_elem_size(const char* who, int elem_size) {
  if (elem_size == 8 || elem_size == 1) return NASSEG_OK;
  return nasseg_fail(NASSEG_ERR_ARG, "%s: elem_size %d not supported", who, elem_size);
}
inline int check_selection(const char* who, int select, int64_t min_kept, double keep_fraction) {
  if (!select || (min_kept >= 1 && keep_fraction >= 0.0 && keep_fraction <= 1.0)) return NASSEG_OK;
  return nasseg_fail(NASSEG_ERR_ARG, "%s: selection needs min_kept >= 1 and 0 <= keep_fraction <= 1", who);
}

#ifndef NASSEG_LOSS_NO_SUM_PASS
// What follows the pass that wrote pixel_loss: the selection (`selection(tau, counts)`, when `select`), the sum pass
// into ws = [kCeGridCap][3] partials and - unless the caller's own finalizer reads them (fin_name == nullptr) - the
// fp64 finalize.  lr: the row table the labels are read through (none: `target` is the batch's own labels).
template <typename Sel, typename... Rows>
inline int ce_sel_reduce(const char* sum_name, const char* fin_name, Sel&& selection, const float* pixel_loss,
                         const void* target, int elem_size, const float* weight, int64_t P, int select,
                         float* loss, float* stats, int64_t* counts, float* ws, hipStream_t s, Rows... lr) {
  static_assert(sizeof...(Rows) <= 1, "no table, or one LabelRows");
  const int grid = ce_grid(P);
  if (select) NASSEG_TRY(selection(stats + 1, counts));
  const float* tau = select ? stats + 1 : nullptr;
  with_labels(target, elem_size, [&](auto labels) {
    hipLaunchKernelGGL((ce_sel_sum_kernel<label_of<decltype(labels)>, Rows...>), dim3(grid), dim3(256), 0, s,
                       pixel_loss, labels, weight, P, tau, ws, lr...);
  });
  NASSEG_LAUNCH_CHECK(sum_name);
  if (fin_name) {
    hipLaunchKernelGGL(ce_sel_finalize_kernel, dim3(1), dim3(256), 0, s, ws, grid, select, loss, stats, counts);
    NASSEG_LAUNCH_CHECK(fin_name);
  }
  return NASSEG_OK;
}
#endif  // NASSEG_LOSS_NO_SUM_PASS

}  // namespace
