// Test-time ensemble over scales and mirroring (engine/predict.py, engine/inference.py).
//
// view_image: the network's input of one view - the normalised image resized bilinearly (align_corners=False, the
// arithmetic of bilinear_fwd_scalar_kernel in resize.hip) with its columns reversed for a mirrored view.
//
// fuse_views: V small logit maps -> labels / mean probabilities / confusion matrix / mean map at the image's size
// without a full-resolution tensor per view.  Per output pixel and view the resampled logits are the host tables'
// taps (4 per axis: predict.hip's cubic_at; 2: bilinear) applied as a horizontal pass over the source rows and a
// vertical pass, each summed in tap order from zero without FMA contraction.  The horizontal sum of a source row does
// not depend on the output row, so a workgroup owns a 32 x 16 output tile and, per view, computes the horizontal pass
// ONCE for every source row its 16 output rows touch - [rows][32 columns][C] in LDS - and every thread (one output
// pixel) runs the vertical pass from LDS: T loads from L1 / L2 per LDS value (the tile's column taps staged in LDS
// as well) instead of T * T per output value.  Each value is the same sequence of fp32 operations as cubic_at's
// (only who computes the row sum changed), so the result is bit-identical to it.  The softmax of the view and the C
// partial sums of P stay in registers.
// A view whose rows do not fit the LDS buffer (a strong reduction, many classes) is staged in bands of output rows
// with a slot per (output row, tap) instead: same arithmetic, same bits.
#include "common.h"
#include "resize_index.h"

namespace {

#define FV_MAX_VIEWS 16
#define FV_MAX_CLASSES 64
#define FV_TW 32             // tile width = one 32-lane half of a wave: the lanes of an LDS access share their source row
#define FV_TH 16             // tile height
#define FV_THREADS (FV_TW * FV_TH)
#define FV_HS_FLOATS 11904   // horizontal sums; with the 4096 confusion-matrix bins: 64 KiB of LDS, two workgroups per CU
#define FV_CM_BINS 4096

template <typename T>
struct FuseViews {
  const T* x[FV_MAX_VIEWS];
  int h[FV_MAX_VIEWS], w[FV_MAX_VIEWS], off[FV_MAX_VIEWS];
};

struct FuseOut {
  const uint8_t* gt;
  uint8_t* labels;
  float* probs;
  unsigned long long* cm;
  float* mean;
  int n;
};

// MODE 0: softmax outputs (labels, probs, cm); 1: the mean map; 2: both.  CMAX: C rounded up to a compiled size (the
// per-thread arrays are registers only when every index is a compile-time constant).
template <int T, int CMAX, int MODE>
__global__ __launch_bounds__(FV_THREADS, CMAX <= 24 ? 4 : 2) void fuse_views_kernel(const FuseViews<act_t> views, int V,
                                                                const int* __restrict__ taps,
                                                                const float* __restrict__ coef, int C, int H, int W,
                                                                const FuseOut out) {
#pragma clang fp contract(off)
  constexpr bool SOFT = MODE != 1, MEAN = MODE != 0;
  __shared__ float hs[FV_HS_FLOATS];
  __shared__ int bins[SOFT ? FV_CM_BINS : 1];
  __shared__ int s_rows[2][2];  // (per view parity: wave 0 may be a view ahead of the others)
  __shared__ int s_xo[4 * FV_TW];  // the tile's column taps (clamped, times C) and weights of the current view
  __shared__ float s_cx[4 * FV_TW];
  const int tid = threadIdx.x;
  const int tx = tid % FV_TW, ty = tid / FV_TW;
  const int ox0 = blockIdx.x * FV_TW, oy0 = blockIdx.y * FV_TH, b = blockIdx.z;
  const int ox = ox0 + tx, oy = oy0 + ty;
  const bool live = ox < W && oy < H;
  const int tile_h = min(FV_TH, H - oy0), tile_w = min(FV_TW, W - ox0);
  const int Cp = C | 1;  // pixel stride in LDS: odd, so that the 32 pixels of an access fall on 32 banks
  const uint64_t inv_row = (((uint64_t)1 << 32) + tile_w * C - 1) / (tile_w * C);
  const unsigned inv_c = ((1u << 20) + C - 1) / C;
  const int nn = out.n * out.n;
  const bool use_bins = SOFT && out.cm && nn <= FV_CM_BINS;
  if (use_bins)
    for (int i = tid; i < nn; i += FV_THREADS) bins[i] = 0;  // (visible after the first barrier of the view loop)

  float P[CMAX], M[MEAN ? CMAX : 1];
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    if (SOFT) P[c] = 0.f;
    if (MEAN) M[c] = 0.f;
  }

  for (int v = 0; v < V; ++v) {
    const int h = views.h[v], w = views.w[v];
    const int* trow = taps + views.off[v];
    const float* crow = coef + views.off[v];
    const int* tcol = trow + T * H;
    const float* ccol = crow + T * H;
    const act_t* xb = views.x[v] + (int64_t)b * h * w * C;
    const int64_t ld = (int64_t)w * C;

    // the source rows of this tile (indices clamped: every load stays in bounds whatever the tables hold)
    if (tid < 64) {
      int lo = h, hi = -1;
      if (tid < T * tile_h) {
        lo = hi = min(max(trow[T * oy0 + tid], 0), h - 1);
      }
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {
        lo = min(lo, __shfl_xor(lo, s));
        hi = max(hi, __shfl_xor(hi, s));
      }
      if (tid == 0) {
        s_rows[v & 1][0] = lo;
        s_rows[v & 1][1] = hi - lo + 1;
      }
    }
    // (waves 1 and 2; the previous view's horizontal passes ended before the barrier these waves have passed)
    if (tid >= 64 && tid < 64 + T * tile_w) {
      s_xo[tid - 64] = min(max(tcol[T * ox0 + tid - 64], 0), w - 1) * C;
      s_cx[tid - 64] = ccol[T * ox0 + tid - 64];
    }
    __syncthreads();  // (also: every thread is done with the previous view's horizontal sums)
    const int row0 = s_rows[v & 1][0], nrows = s_rows[v & 1][1];
    // shared: the tile's source rows row0 .. row0 + nrows - 1 fit the buffer, one band of FV_TH output rows.  Else
    // (a strong reduction, many classes): bands of `band` output rows, a slot per (output row, tap) - nothing shared
    // between output rows, the same arithmetic
    const bool shared = nrows * FV_TW * Cp <= FV_HS_FLOATS;
    const int band = shared ? FV_TH : max(1, FV_HS_FLOATS / (T * FV_TW * Cp));

    int slot[T];
    float cy[T];
    if (live) {
#pragma unroll
      for (int k = 0; k < T; ++k) {
        slot[k] = shared ? min(max(trow[T * oy + k], 0), h - 1) - row0 : (ty % band) * T + k;
        cy[k] = crow[T * oy + k];
      }
    }
    for (int y0 = 0; y0 < tile_h; y0 += band) {
      if (y0 > 0) __syncthreads();
      // horizontal pass: item = (slot, tile column, channel), channel fastest - a wave reads runs of C consecutive
      // values and writes consecutive LDS words
      const int nslots = shared ? nrows : min(band, tile_h - y0) * T;
      const int per_row = tile_w * C;
      const int items = nslots * per_row;  // (< 2^14: the buffer's size)
      for (int i = tid; i < items; i += FV_THREADS) {
        // i / per_row and rem / C by multiplication: exact for i < 2^14, per_row <= 2^11, C <= 2^6
        const int rr = (int)(((uint64_t)i * inv_row) >> 32);
        const int rem = i - rr * per_row;
        const int px = (int)(((unsigned)rem * inv_c) >> 20), c = rem - px * C;
        const int sr = shared ? row0 + rr : min(max(trow[T * (oy0 + y0) + rr], 0), h - 1);
        const act_t* row = xb + (int64_t)sr * ld + c;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < T; ++j) s = s + lda1(row + s_xo[T * px + j]) * s_cx[T * px + j];
        hs[(rr * FV_TW + px) * Cp + c] = s;
      }
      __syncthreads();
      if (live && ty >= y0 && ty < y0 + band) {
        // vertical pass: the 32 lanes of an access read one slot, pixel stride Cp (odd): 32 banks
        const float* col = hs + tx * Cp;
        float r[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
          if (c < C) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < T; ++k) acc = acc + col[slot[k] * FV_TW * Cp + c] * cy[k];
            r[c] = acc;
          }
        }
        if (MEAN) {
#pragma unroll
          for (int c = 0; c < CMAX; ++c)
            if (c < C) M[c] = M[c] + r[c];
        }
        if (SOFT) {
          float m = r[0];
#pragma unroll
          for (int c = 1; c < CMAX; ++c)
            if (c < C) m = fmaxf(m, r[c]);
          float sum = 0.f;
#pragma unroll
          for (int c = 0; c < CMAX; ++c) {
            if (c < C) {
              r[c] = expf(r[c] - m);
              sum = sum + r[c];
            }
          }
          const float inv = 1.f / sum;
#pragma unroll
          for (int c = 0; c < CMAX; ++c)
            if (c < C) P[c] = P[c] + r[c] * inv;
        }
      }
    }
  }

  if (live) {
    const int64_t p = ((int64_t)b * H + oy) * W + ox;
    const float fv = (float)V;
    if (MEAN) {
#pragma unroll
      for (int c = 0; c < CMAX; ++c)
        if (c < C) out.mean[p * C + c] = M[c] / fv;
    }
    if (SOFT) {
      if (out.probs) {
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
          if (c < C) out.probs[p * C + c] = P[c] / fv;
      }
      if (out.labels || out.cm) {
        float best = P[0];
        int arg = 0;
#pragma unroll
        for (int c = 1; c < CMAX; ++c) {
          if (c < C) {
            const float q = P[c];
            if (q > best || (q != q && best == best)) {
              best = q;
              arg = c;
            }
          }
        }
        if (out.labels) out.labels[p] = (uint8_t)arg;
        if (out.cm) {
          const int a = out.gt[p];
          if (a < out.n && arg < out.n) {
            if (use_bins)
              atomicAdd(&bins[a * out.n + arg], 1);
            else
              atomicAdd(&out.cm[a * out.n + arg], 1ULL);
          }
        }
      }
    }
  }
  if (use_bins) {
    __syncthreads();
    for (int i = tid; i < nn; i += FV_THREADS)
      if (bins[i]) atomicAdd(&out.cm[i], (unsigned long long)bins[i]);
  }
}

template <int T, int CMAX>
void fuse_launch(int mode, dim3 grid, hipStream_t stream, const FuseViews<act_t>& views, int V, const int* taps,
                 const float* coef, int C, int H, int W, const FuseOut& out) {
  if (mode == 0)
    hipLaunchKernelGGL((fuse_views_kernel<T, CMAX, 0>), grid, dim3(FV_THREADS), 0, stream, views, V, taps, coef, C, H,
                       W, out);
  else if (mode == 1)
    hipLaunchKernelGGL((fuse_views_kernel<T, CMAX, 1>), grid, dim3(FV_THREADS), 0, stream, views, V, taps, coef, C, H,
                       W, out);
  else
    hipLaunchKernelGGL((fuse_views_kernel<T, CMAX, 2>), grid, dim3(FV_THREADS), 0, stream, views, V, taps, coef, C, H,
                       W, out);
}

template <int T>
void fuse_launch_c(int mode, dim3 grid, hipStream_t stream, const FuseViews<act_t>& views, int V, const int* taps,
                   const float* coef, int C, int H, int W, const FuseOut& out) {
  if (C <= 4)
    fuse_launch<T, 4>(mode, grid, stream, views, V, taps, coef, C, H, W, out);
  else if (C <= 12)
    fuse_launch<T, 12>(mode, grid, stream, views, V, taps, coef, C, H, W, out);
  else if (C <= 24)
    fuse_launch<T, 24>(mode, grid, stream, views, V, taps, coef, C, H, W, out);
  else if (C <= 40)
    fuse_launch<T, 40>(mode, grid, stream, views, V, taps, coef, C, H, W, out);
  else
    fuse_launch<T, FV_MAX_CLASSES>(mode, grid, stream, views, V, taps, coef, C, H, W, out);
}

// one thread per output value: consecutive channels of consecutive pixels, whatever C is
__global__ __launch_bounds__(256) void view_image_kernel(const act_t* __restrict__ x, act_t* __restrict__ y, int B,
                                                         int Hi, int Wi, int C, int Ho, int Wo, float sh, float sw,
                                                         int mirror) {
  const int64_t total = (int64_t)B * Ho * Wo * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int64_t p = i / C;
    const int ox = (int)(p % Wo);
    const int64_t prow = p / Wo;
    const int oy = (int)(prow % Ho);
    const int b = (int)(prow / Ho);
    const Lin ly = lin_coeff(oy, sh, Hi, Ho);
    const Lin lx = lin_coeff(mirror ? Wo - 1 - ox : ox, sw, Wi, Wo);
    const act_t* xb = x + (int64_t)b * Hi * Wi * C + c;
    const float v00 = lda1(xb + ((int64_t)ly.i0 * Wi + lx.i0) * C);
    const float v01 = lda1(xb + ((int64_t)ly.i0 * Wi + lx.i1) * C);
    const float v10 = lda1(xb + ((int64_t)ly.i1 * Wi + lx.i0) * C);
    const float v11 = lda1(xb + ((int64_t)ly.i1 * Wi + lx.i1) * C);
    sta1(y + i, bilerp(v00, v01, v10, v11, ly, lx));
  }
}

}  // namespace

extern "C" {

int NASSEG_FN(view_image)(const act_t* x, act_t* y, int B, int Hi, int Wi, int C, int Ho, int Wo, int mirror,
                          void* stream) {
  NASSEG_REQUIRE(B > 0 && Hi > 0 && Wi > 0 && C > 0 && Ho > 0 && Wo > 0, "view_image: bad shape");
  NASSEG_REQUIRE(x && y, "view_image: null pointer");
  const int64_t total = (int64_t)B * Ho * Wo * C;
  const int64_t blocks = cdiv64(total, 256);
  const float sh = (float)Hi / (float)Ho, sw = (float)Wi / (float)Wo;
  hipLaunchKernelGGL(view_image_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0,
                     (hipStream_t)stream, x, y, B, Hi, Wi, C, Ho, Wo, sh, sw, mirror);
  NASSEG_LAUNCH_CHECK("view_image");
  return NASSEG_OK;
}

int NASSEG_FN(fuse_views)(int n_views, const act_t* const* views, const int* dims, const int* taps, const float* coef,
                          int n_taps, int B, int C, int H, int W, const uint8_t* gt, int n, uint8_t* labels,
                          float* probs, int64_t* cm, float* mean, void* stream) {
  NASSEG_REQUIRE(n_views >= 1 && n_views <= FV_MAX_VIEWS, "fuse_views: n_views=%d: between 1 and %d views", n_views,
                 FV_MAX_VIEWS);
  NASSEG_REQUIRE(n_taps == 2 || n_taps == 4, "fuse_views: n_taps=%d: 2 (bilinear) or 4 (cubic)", n_taps);
  NASSEG_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "fuse_views: bad shape");
  NASSEG_REQUIRE(B <= 65535 && H <= 65535 * FV_TH, "fuse_views: B=%d, H=%d: too large", B, H);
  NASSEG_REQUIRE((int64_t)n_views * n_taps * ((int64_t)H + W) < ((int64_t)1 << 31), "fuse_views: tables too large");
  NASSEG_REQUIRE(views && dims && taps && coef, "fuse_views: null pointer");
  const bool soft = labels || probs || cm;
  NASSEG_REQUIRE(soft || mean, "fuse_views: no output");
  NASSEG_REQUIRE(C <= FV_MAX_CLASSES, "fuse_views: C=%d: at most %d classes (channels)", C, FV_MAX_CLASSES);
  NASSEG_REQUIRE(!cm || (gt && n > 0 && n <= 256), "fuse_views: n=%d: a confusion matrix needs gt and 1 <= n <= 256",
                 n);
  FuseViews<act_t> fv;
  for (int v = 0; v < FV_MAX_VIEWS; ++v) {
    const int s = v < n_views ? v : 0;
    NASSEG_REQUIRE(views[s] && dims[3 * s] > 0 && dims[3 * s + 1] > 0 && dims[3 * s + 2] >= 0,
                   "fuse_views: view %d: null map or bad dims", s);
    NASSEG_REQUIRE((int64_t)dims[3 * s] * dims[3 * s + 1] * C < ((int64_t)1 << 31), "fuse_views: view %d too large", s);
    fv.x[v] = views[s];
    fv.h[v] = dims[3 * s];
    fv.w[v] = dims[3 * s + 1];
    fv.off[v] = dims[3 * s + 2];
  }
  FuseOut out;
  out.gt = gt;
  out.labels = labels;
  out.probs = probs;
  out.cm = (unsigned long long*)cm;
  out.mean = mean;
  out.n = cm ? n : 0;
  const int mode = !soft ? 1 : (mean ? 2 : 0);
  const dim3 grid((unsigned)cdiv(W, FV_TW), (unsigned)cdiv(H, FV_TH), (unsigned)B);
  if (n_taps == 4)
    fuse_launch_c<4>(mode, grid, (hipStream_t)stream, fv, n_views, taps, coef, C, H, W, out);
  else
    fuse_launch_c<2>(mode, grid, (hipStream_t)stream, fv, n_views, taps, coef, C, H, W, out);
  NASSEG_LAUNCH_CHECK("fuse_views");
  return NASSEG_OK;
}

}  // extern "C"
