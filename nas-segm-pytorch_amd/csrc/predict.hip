// Post-processing of a prediction: the resize the reference's inference notebooks do on the host -
// cv2.resize(logits, dsize, interpolation=INTER_CUBIC), float branch - then, for segmentation, the argmax over the
// classes.  The host hands over per-axis tables built by data/datasets._cubic_taps (four clipped source indices and
// four float32 Keys weights, A = -0.75, per output row and column), so the kernels do no coordinate arithmetic: each
// output value is the host restatement's sequence of fp32 operations - a horizontal pass over the four source rows,
// then a vertical pass, each summed in tap order 0..3 from zero, every product and sum rounded on its own (no FMA
// contraction) - and equals it bit for bit.  At the identity size the weights are (0, 1, 0, 0): the input comes back.
#include "common.h"

namespace {

// one output value at column taps (xo, cx) from the rows of taps (ty, cy): x points at channel c of the sample,
// pixel stride C
__device__ __forceinline__ float cubic_at(const act_t* __restrict__ x, int64_t row_ld, const int64_t ro[4],
                                          const float cy[4], const int xo[4], const float cx[4]) {
  // (hipcc contracts a * b + c into an FMA by default, __fmul_rn / __fadd_rn included: numpy rounds twice)
#pragma clang fp contract(off)
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const act_t* row = x + ro[k] * row_ld;
    float hs = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) hs = hs + lda1(row + xo[j]) * cx[j];
    acc = acc + hs * cy[k];
  }
  return acc;
}

// one thread per output VALUE (pixel, channel) of one output row (blockIdx.y) of one sample (blockIdx.z): a wave
// reads and writes consecutive channels of consecutive pixels - contiguous NHWC, whatever C is
__global__ __launch_bounds__(256) void resize_cubic_kernel(const act_t* __restrict__ x, int h, int w, int C,
                                                           const int* __restrict__ taps,
                                                           const float* __restrict__ coef, float* __restrict__ y,
                                                           int H, int W) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= W * C) return;
  const int oy = blockIdx.y, b = blockIdx.z;
  const int ox = i / C, c = i - ox * C;
  int64_t ro[4];
  float cy[4], cx[4];
  int xo[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // (indices clamped again: every load stays in bounds whatever the tables hold)
    ro[k] = min(max(taps[4 * oy + k], 0), h - 1);
    cy[k] = coef[4 * oy + k];
    xo[k] = min(max(taps[4 * H + 4 * ox + k], 0), w - 1) * C;
    cx[k] = coef[4 * H + 4 * ox + k];
  }
  const act_t* xb = x + (int64_t)b * h * w * C + c;
  y[((int64_t)b * H + oy) * W * C + i] = cubic_at(xb, (int64_t)w * C, ro, cy, xo, cx);
}

// one thread per output pixel of one output row (blockIdx.y) of one sample (blockIdx.z); the resized values of the
// C channels are compared as they are made and never stored.  The lowest index wins ties (numpy's argmax,
// argmax_cm_kernel); so does the first NaN, as in numpy.
__global__ __launch_bounds__(256) void resize_cubic_argmax_kernel(const act_t* __restrict__ x, int h, int w, int C,
                                                                  const int* __restrict__ taps,
                                                                  const float* __restrict__ coef,
                                                                  uint8_t* __restrict__ labels, int H, int W) {
  const int ox = blockIdx.x * 256 + threadIdx.x;
  if (ox >= W) return;
  const int oy = blockIdx.y, b = blockIdx.z;
  int64_t ro[4];
  float cy[4], cx[4];
  int xo[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ro[k] = min(max(taps[4 * oy + k], 0), h - 1);
    cy[k] = coef[4 * oy + k];
    xo[k] = min(max(taps[4 * H + 4 * ox + k], 0), w - 1) * C;
    cx[k] = coef[4 * H + 4 * ox + k];
  }
  const act_t* xb = x + (int64_t)b * h * w * C;
  const int64_t ld = (int64_t)w * C;
  float best = cubic_at(xb, ld, ro, cy, xo, cx);
  int arg = 0;
  for (int c = 1; c < C; ++c) {
    const float v = cubic_at(xb + c, ld, ro, cy, xo, cx);
    if (v > best || (v != v && best == best)) {
      best = v;
      arg = c;
    }
  }
  labels[((int64_t)b * H + oy) * W + ox] = (uint8_t)arg;
}

int check_shape(const char* name, int B, int h, int w, int C, int H, int W) {
  NASSEG_REQUIRE(B > 0 && h > 0 && w > 0 && C > 0 && H > 0 && W > 0, "%s: bad shape", name);
  NASSEG_REQUIRE(B <= 65535 && H <= 65535, "%s: B=%d, H=%d: at most 65535 of each", name, B, H);
  NASSEG_REQUIRE((int64_t)W * C < ((int64_t)1 << 31) && (int64_t)4 * (H + W) < ((int64_t)1 << 31),
                 "%s: output too large", name);
  return NASSEG_OK;
}

}  // namespace

extern "C" {

int NASSEG_FN(resize_cubic)(const act_t* x, int B, int h, int w, int C, const int* taps, const float* coef, float* y,
                            int H, int W, void* stream) {
  const int rc = check_shape("resize_cubic", B, h, w, C, H, W);
  if (rc != NASSEG_OK) return rc;
  NASSEG_REQUIRE(x && taps && coef && y, "resize_cubic: null pointer");
  hipLaunchKernelGGL(resize_cubic_kernel, dim3((unsigned)cdiv64((int64_t)W * C, 256), H, B), dim3(256), 0,
                     (hipStream_t)stream, x, h, w, C, taps, coef, y, H, W);
  NASSEG_LAUNCH_CHECK("resize_cubic");
  return NASSEG_OK;
}

int NASSEG_FN(resize_cubic_argmax)(const act_t* x, int B, int h, int w, int C, const int* taps, const float* coef,
                                   uint8_t* labels, int H, int W, void* stream) {
  const int rc = check_shape("resize_cubic_argmax", B, h, w, C, H, W);
  if (rc != NASSEG_OK) return rc;
  NASSEG_REQUIRE(C <= 256, "resize_cubic_argmax: C=%d does not fit uint8 labels", C);
  NASSEG_REQUIRE(x && taps && coef && labels, "resize_cubic_argmax: null pointer");
  hipLaunchKernelGGL(resize_cubic_argmax_kernel, dim3((unsigned)cdiv(W, 256), H, B), dim3(256), 0,
                     (hipStream_t)stream, x, h, w, C, taps, coef, labels, H, W);
  NASSEG_LAUNCH_CHECK("resize_cubic_argmax");
  return NASSEG_OK;
}

}  // extern "C"
