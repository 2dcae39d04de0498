// Depth metrics on the device: the depth counterpart of nasseg_argmax_cm (miou.hip), gfx950.
//
// Not present in the reference (its depth networks are inference only; "parity unpinned"): the usual scores of a
// depth network (Eigen et al. 2014) from ONE pass over the ground truth.  Channel 0 of the NHWC prediction
// [B][h][w][ldp] is up-sampled bilinearly (align_corners=False; lin_coeff and the explicitly rounded fp32 products
// and sums of argmax_cm_kernel, so the value is the fp32 up-sampling torch performs) to the ground truth's (H, W);
// pixels whose gt is finite and in (min_depth, max_depth] are kept, the prediction is clamped to
// [min_depth, max_depth] (min_depth > 0: every logarithm is defined), and from the fp32 p and g, in double:
//   acc[0] += n                 acc[1] += sum |p-g|            acc[2] += sum (p-g)^2
//   acc[3] += sum |p-g|/g       acc[4] += sum (p-g)^2/g        acc[5] += sum |log10 p - log10 g|
//   acc[6] += sum (ln p - ln g) acc[7] += sum (ln p - ln g)^2
//   acc[8..10] += #{max(p/g, g/p) < 1.25, 1.25^2, 1.25^3}      acc[11]: reserved, untouched
// Every workgroup writes one row of partial sums; ONE workgroup then adds the rows in a fixed order and adds the
// result to acc: the same inputs give the same 12 doubles on every run (no atomics).
#include <math.h>

#include "common.h"
#include "resize_index.h"

namespace {

constexpr int kSlots = 11;   // sums written per row
constexpr int kRow = 12;     // doubles per row / in acc
constexpr int kMaxRows = 2048;

__device__ __forceinline__ bool gt_valid(float g, float dmin, float dmax) {
  const bool finite = (__float_as_uint(g) & 0x7f800000u) != 0x7f800000u;
  return finite && g > dmin && g <= dmax;
}

__global__ __launch_bounds__(256) void depth_metrics_kernel(const act_t* __restrict__ pred, int64_t ldp, int B,
                                                            int h, int w, const float* __restrict__ gt, int H,
                                                            int W, float sh, float sw, float dmin, float dmax,
                                                            double* __restrict__ rows) {
  __shared__ double red[256];
  double a[kSlots];
#pragma unroll
  for (int k = 0; k < kSlots; ++k) a[k] = 0.0;
  const int64_t P = (int64_t)B * H * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256) {
    const float gf = gt[i];
    if (!gt_valid(gf, dmin, dmax)) continue;
    const int ox = (int)(i % W);
    const int64_t t = i / W;
    const int oy = (int)(t % H);
    const int64_t b = t / H;
    const Lin ly = lin_coeff(oy, sh, h, H);
    const Lin lx = lin_coeff(ox, sw, w, W);
    const act_t* pb = pred + b * h * w * ldp;
    const float p00 = lda1(pb + ((int64_t)ly.i0 * w + lx.i0) * ldp);
    const float p01 = lda1(pb + ((int64_t)ly.i0 * w + lx.i1) * ldp);
    const float p10 = lda1(pb + ((int64_t)ly.i1 * w + lx.i0) * ldp);
    const float p11 = lda1(pb + ((int64_t)ly.i1 * w + lx.i1) * ldp);
    // explicit rounding of every product / sum (no fma contraction): the fp32 up-sampling of argmax_cm_kernel
    const float top = __fadd_rn(__fmul_rn(lx.l0, p00), __fmul_rn(lx.l1, p01));
    const float bot = __fadd_rn(__fmul_rn(lx.l0, p10), __fmul_rn(lx.l1, p11));
    const float pf = fminf(fmaxf(__fadd_rn(__fmul_rn(ly.l0, top), __fmul_rn(ly.l1, bot)), dmin), dmax);
    // fp64 from here on; one division and one logarithm per pixel: |p-g|/g and (p-g)^2/g through 1/g,
    // ln p - ln g as ln(p/g) (both within a few 1e-16 relative of the separate forms), and the three threshold
    // tests as products - p < t g and g < t p are exact in double for fp32 p, g and these t, hence exactly
    // max(p/g, g/p) < t
    const double p = (double)pf, g = (double)gf;
    const double inv = 1.0 / g;
    const double d = p - g, ad = fabs(d), d2 = d * d;
    const double l = log(p * inv);
    a[0] += 1.0;
    a[1] += ad;
    a[2] += d2;
    a[3] += ad * inv;
    a[4] += d2 * inv;
    a[5] += fabs(l) * 0.43429448190325182765;  // |log10 p - log10 g| = |ln p - ln g| / ln 10
    a[6] += l;
    a[7] += l * l;
    a[8] += (p < 1.25 * g && g < 1.25 * p) ? 1.0 : 0.0;
    a[9] += (p < 1.5625 * g && g < 1.5625 * p) ? 1.0 : 0.0;
    a[10] += (p < 1.953125 * g && g < 1.953125 * p) ? 1.0 : 0.0;
  }
  // one fixed-order tree per sum
#pragma unroll
  for (int k = 0; k < kSlots; ++k) {
    red[threadIdx.x] = a[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) rows[(int64_t)blockIdx.x * kRow + k] = red[0];
    __syncthreads();
  }
}

// acc[k] += sum over the rows, k < 11: thread t adds rows t, t+256, ..., then a fixed-order tree through LDS
__global__ __launch_bounds__(256) void depth_metrics_finalize_kernel(const double* __restrict__ rows, int nrows,
                                                                     double* __restrict__ acc) {
  __shared__ double red[256];
  for (int k = 0; k < kSlots; ++k) {
    double s = 0.0;
    for (int r = threadIdx.x; r < nrows; r += 256) s += rows[(int64_t)r * kRow + k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int j = 128; j > 0; j >>= 1) {
      if ((int)threadIdx.x < j) red[threadIdx.x] += red[threadIdx.x + j];
      __syncthreads();
    }
    if (threadIdx.x == 0) acc[k] += red[0];
    __syncthreads();
  }
}

inline int dm_grid(int64_t P) {
  int64_t b = (P + 256 * 4 - 1) / (256 * 4);
  if (b > kMaxRows) b = kMaxRows;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

extern "C" {

#if NASSEG_FP32_ONLY
// doubles of workspace for one nasseg_depth_metrics call on a [B][H][W] ground truth
int64_t nasseg_depth_metrics_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (int64_t)dm_grid((int64_t)B * H * W) * kRow;
}
#endif

// pred: channel 0 of an NHWC map [B][h][w] with pixel stride ldp elements; gt: fp32 [B][H][W];
// acc: 12 doubles on the device, ACCUMULATED into (zero them first for fresh sums).
int NASSEG_FN(depth_metrics)(const act_t* pred, int64_t ldp, int B, int h, int w, const float* gt, int H, int W,
                             float min_depth, float max_depth, double* acc, double* ws, void* stream) {
  NASSEG_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && ldp >= 1, "depth_metrics: bad shape");
  NASSEG_REQUIRE(min_depth > 0.f && max_depth > min_depth,
                 "depth_metrics: need 0 < min_depth < max_depth (got %g, %g)", (double)min_depth,
                 (double)max_depth);
  NASSEG_REQUIRE(pred && gt && acc && ws, "depth_metrics: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int grid = dm_grid((int64_t)B * H * W);
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  hipLaunchKernelGGL(depth_metrics_kernel, dim3(grid), dim3(256), 0, s, pred, ldp, B, h, w, gt, H, W, sh, sw,
                     min_depth, max_depth, ws);
  NASSEG_LAUNCH_CHECK("depth_metrics");
  hipLaunchKernelGGL(depth_metrics_finalize_kernel, dim3(1), dim3(256), 0, s, ws, grid, acc);
  NASSEG_LAUNCH_CHECK("depth_metrics_finalize");
  return NASSEG_OK;
}

}  // extern "C"
