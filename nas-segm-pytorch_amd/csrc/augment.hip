// Sample augmentation of the data pipeline (data/datasets.py, planned by data/device.py): OpenCV's fixed-point
// INTER_CUBIC resize, crops, mirror and constant borders, Normalise and the cast of the engine's image, in one
// gather per batch.  The host hands over per-axis tables - four source indices and four 11-bit coefficients per
// output row / column (index -1: a fill pixel), a nearest index per row / column for the mask - already rebased to
// the uploaded source window, so the kernel only adds integers: the result is exact by construction, whatever the
// summation order.  The uint8 result v of channel c becomes lut[c][v] (Normalise evaluated by the host in float64
// and cast to act_t there).
//
// augment_depth_kernel is the same launch for a metric depth target instead of a label map: the image half is the
// one function both kernels call (augment_image); the target windows hold little-endian 16-bit counts and the output
// is fp32 metres, count * depth_scale / zoom[b], each operation rounded once as numpy's float32 product and quotient
// are (__fmul_rn, __fdiv_rn: no contraction, no reciprocal), or the sample's fill, written as it is.  A packed target
// window may start at any byte (an image of odd 3 h w bytes precedes it), so a count is read as TWO BYTE LOADS and
// put together in a register: the target half issues no 16-bit load, aligned or not, and the host packs without
// padding.
//
// The colour launches (nasseg_augment_colour, nasseg_augment_depth_colour: data/datasets.py's ColourJitter) are the
// same two kernels with augment_image's compile-time switch on: a live pixel's resampled uint8 triple v goes through
// the sample's 12-bit colour matrix, m[c] = clip((sum_k q[c][k] v[k] + 2048) >> 12, 0, 255) (arithmetic shift, skipped
// unless the sample's word 9 is set), then through the sample's byte table ctab[c][m[c]], then through lut as before.
// A fill pixel goes from the descriptor's fill straight to lut: the host has jittered that fill where its pipeline does.
// The sum is int32: each coefficient is clamped to |q| <= 2^15 as it is read (the planner refuses larger ones), so
// |sum| <= 3 * 2^15 * 255 + 2^11 < 2^25 whatever `colour` holds, and every table index is a value clipped to 0..255.
// The sample's 12 words are uniform per workgroup (blockIdx.y); its 768 table bytes sit in LDS beside lut.
#include "common.h"

namespace {

// per-sample descriptor: int64 [AUG_DESC]
enum { AUG_IMG_OFF, AUG_MSK_OFF, AUG_H, AUG_W, AUG_IMG_LD, AUG_MSK_LD, AUG_IMG_FILL, AUG_MSK_FILL, AUG_DESC };

// The image half of one output pixel (oy, ox) of a sample (its image window: the descriptor's img_off, h, w, img_ld
// and img_fill; its tables t): OpenCV's fixed-point bicubic of the four by four taps (or the fill), through the table
// in LDS, to the pixel's three values at o.  Every kernel of this file calls it.  COLOUR: the live pixel's colour
// matrix cq (the sample's 12 words, wave-uniform) and byte table stab (LDS, [3][256]) in between; without it
// neither is touched.
template <bool COLOUR>
__device__ __forceinline__ void augment_image(const uint8_t* __restrict__ src, int64_t src_bytes, int64_t img_off,
                                              int h, int w, int64_t img_ld, int img_fill, const int* __restrict__ t,
                                              const act_t* slut, act_t* __restrict__ o, int oy, int ox, int Ho,
                                              const int32_t* __restrict__ cq, const uint8_t* stab) {
  // a window that does not lie inside the buffer is read as fill (the host checks before it launches; this
  // keeps every load in bounds whatever it is handed)
  const bool img_ok = h > 0 && w > 0 && img_off >= 0 && img_ld >= 3 * (int64_t)w &&
                      img_off + (h - 1) * img_ld + 3 * (int64_t)w <= src_bytes;

  const int* ty = t + oy * 8;
  const int* tx = t + Ho * 8 + ox * 8;

  int v[3];
  if (ty[0] < 0 || tx[0] < 0 || !img_ok) {
    v[0] = img_fill & 255;
    v[1] = (img_fill >> 8) & 255;
    v[2] = (img_fill >> 16) & 255;
  } else {
    int xo[4], ax[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      xo[j] = 3 * min(max(tx[j], 0), w - 1);
      ax[j] = tx[4 + j];
    }
    // horizontal sums: |sum| <= 255 * sum|ax| (< 2^13 * 255), int32; vertical products and sum in int64 (up to
    // ~255 * 2816^2 = 2.0e9 for Keys' A = -0.75, within 7 % of 2^31: exact in int64 for any coefficients)
    int64_t acc[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint8_t* row = src + img_off + (int64_t)min(max(ty[k], 0), h - 1) * img_ld;
      int hs[3] = {0, 0, 0};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int c = 0; c < 3; ++c) hs[c] += ax[j] * (int)row[xo[j] + c];
      }
      const int64_t ay = ty[4 + k];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += ay * hs[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t r = (acc[c] + (1 << 21)) >> 22;  // arithmetic shift, as numpy's >> on int64
      v[c] = (int)(r < 0 ? 0 : (r > 255 ? 255 : r));
    }
    if (COLOUR) {
      if (cq[9] != 0) {
        int m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          int sum = 1 << 11;
#pragma unroll
          for (int k = 0; k < 3; ++k) sum += min(max(cq[3 * c + k], -(1 << 15)), 1 << 15) * v[k];
          m[c] = min(max(sum >> 12, 0), 255);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = m[c];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = stab[256 * c + v[c]];
    }
  }
  o[0] = slut[v[0]];
  o[1] = slut[256 + v[1]];
  o[2] = slut[512 + v[2]];
}

// one thread per output pixel of one sample (blockIdx.y), the pixels of a sample in row-major order: a wave writes
// 64 consecutive pixels (768 contiguous bytes of fp32 image, 64 of mask), and the few output rows a workgroup
// covers read the same four source rows, which stay in L1 / L2 between the lanes that share them.
// COLOUR: colour int32 [B][12] and ctab uint8 [B][3][256] (4-byte aligned: copied as 192 words) are read, else ignored.
template <bool COLOUR>
__global__ __launch_bounds__(256) void augment_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                      const int64_t* __restrict__ desc,
                                                      const int* __restrict__ taps,
                                                      const int32_t* __restrict__ colour,
                                                      const uint8_t* __restrict__ ctab,
                                                      const act_t* __restrict__ lut, act_t* __restrict__ image,
                                                      uint8_t* __restrict__ mask, int Ho, int Wo) {
  const int b = blockIdx.y;
  __shared__ act_t slut[3 * 256];
  __shared__ uint32_t stab[COLOUR ? 3 * 64 : 1];
  for (int i = threadIdx.x; i < 3 * 256; i += 256) slut[i] = lut[i];
  if (COLOUR && threadIdx.x < 3 * 64) stab[threadIdx.x] = ((const uint32_t*)ctab)[(int64_t)b * (3 * 64) + threadIdx.x];
  __syncthreads();

  const int64_t npix = (int64_t)Ho * Wo;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  const int oy = (int)(p / Wo), ox = (int)(p - (int64_t)oy * Wo);

  const int64_t* d = desc + (int64_t)b * AUG_DESC;
  const int64_t img_off = d[AUG_IMG_OFF], msk_off = d[AUG_MSK_OFF];
  const int h = (int)d[AUG_H], w = (int)d[AUG_W];
  const int64_t img_ld = d[AUG_IMG_LD], msk_ld = d[AUG_MSK_LD];
  const int img_fill = (int)d[AUG_IMG_FILL], msk_fill = (int)d[AUG_MSK_FILL];
  const bool msk_ok = h > 0 && w > 0 && msk_off >= 0 && msk_ld >= w &&
                      msk_off + (h - 1) * msk_ld + w <= src_bytes;

  // tables of the sample: rows [Ho][8], columns [Wo][8] (4 indices, 4 coefficients), mask rows [Ho], columns [Wo]
  const int* t = taps + (int64_t)b * (9 * (Ho + Wo));
  const int my = t[8 * (Ho + Wo) + oy], mx = t[8 * (Ho + Wo) + Ho + ox];

  augment_image<COLOUR>(src, src_bytes, img_off, h, w, img_ld, img_fill, t, slut, image + ((int64_t)b * npix + p) * 3,
                        oy, ox, Ho, COLOUR ? colour + (int64_t)b * 12 : nullptr, (const uint8_t*)stab);

  if (!mask) return;  // (an image without a mask: F.prepare_image)
  int m = msk_fill & 255;
  if (my >= 0 && mx >= 0 && msk_ok) m = src[msk_off + (int64_t)min(my, h - 1) * msk_ld + min(mx, w - 1)];
  mask[(int64_t)b * npix + p] = (uint8_t)m;
}

// The same launch for a depth target (see the head of the file): the target window of sample b holds h rows of w
// little-endian 16-bit counts, msk_ld BYTES apart (>= 2 w); params [B][2] = {zoom, fill} in fp32.  A wave writes 64
// consecutive floats of the target (256 contiguous bytes) next to its 768 bytes of fp32 image.  The descriptor's
// mask fill is not read.  COLOUR: as augment_kernel's.
template <bool COLOUR>
__global__ __launch_bounds__(256) void augment_depth_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                            const int64_t* __restrict__ desc,
                                                            const int* __restrict__ taps,
                                                            const int32_t* __restrict__ colour,
                                                            const uint8_t* __restrict__ ctab,
                                                            const act_t* __restrict__ lut,
                                                            const float* __restrict__ params, float depth_scale,
                                                            act_t* __restrict__ image, float* __restrict__ target,
                                                            int Ho, int Wo) {
  const int b = blockIdx.y;
  __shared__ act_t slut[3 * 256];
  __shared__ uint32_t stab[COLOUR ? 3 * 64 : 1];
  for (int i = threadIdx.x; i < 3 * 256; i += 256) slut[i] = lut[i];
  if (COLOUR && threadIdx.x < 3 * 64) stab[threadIdx.x] = ((const uint32_t*)ctab)[(int64_t)b * (3 * 64) + threadIdx.x];
  __syncthreads();

  const int64_t npix = (int64_t)Ho * Wo;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  const int oy = (int)(p / Wo), ox = (int)(p - (int64_t)oy * Wo);

  const int64_t* d = desc + (int64_t)b * AUG_DESC;
  const int64_t img_off = d[AUG_IMG_OFF], msk_off = d[AUG_MSK_OFF];
  const int h = (int)d[AUG_H], w = (int)d[AUG_W];
  const int64_t img_ld = d[AUG_IMG_LD], msk_ld = d[AUG_MSK_LD];
  const int img_fill = (int)d[AUG_IMG_FILL];
  // (the last byte read is the high byte of the last count of the last row)
  const bool msk_ok = h > 0 && w > 0 && msk_off >= 0 && msk_off <= src_bytes && msk_ld >= 2 * (int64_t)w &&
                      msk_ld <= src_bytes && msk_off + (h - 1) * msk_ld + 2 * (int64_t)w <= src_bytes;
  const int* t = taps + (int64_t)b * (9 * (Ho + Wo));
  const int my = t[8 * (Ho + Wo) + oy], mx = t[8 * (Ho + Wo) + Ho + ox];

  augment_image<COLOUR>(src, src_bytes, img_off, h, w, img_ld, img_fill, t, slut, image + ((int64_t)b * npix + p) * 3,
                        oy, ox, Ho, COLOUR ? colour + (int64_t)b * 12 : nullptr, (const uint8_t*)stab);

  float v = params[2 * b + 1];  // the fill: a pad comes after the resize on the host, so it is not divided
  if (my >= 0 && mx >= 0 && msk_ok) {
    const uint8_t* c = src + msk_off + (int64_t)min(my, h - 1) * msk_ld + 2 * (int64_t)min(mx, w - 1);
    // two byte loads that stay two: the compiler fuses adjacent byte loads into one 16-bit load (here at an address
    // that may be odd) when it can see that they are adjacent, so the high byte's offset passes through an empty asm
    int hi_at = 1;
    asm volatile("" : "+v"(hi_at));
    const int count = (int)c[0] | ((int)c[hi_at] << 8);
    v = __fdiv_rn(__fmul_rn((float)count, depth_scale), params[2 * b]);
  }
  target[(int64_t)b * npix + p] = v;
}

// the launches of the four entry points: one check, one grid (one thread per output pixel, blockIdx.y = sample)
template <bool COLOUR>
int launch_augment(const char* what, const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps,
                   const int32_t* colour, const uint8_t* ctab, const act_t* lut, act_t* image, uint8_t* mask, int B,
                   int Ho, int Wo, void* stream) {
  NASSEG_REQUIRE(B > 0 && B <= 65535 && Ho > 0 && Wo > 0 && src_bytes > 0, "%s: bad shape", what);
  NASSEG_REQUIRE(!COLOUR || (colour != nullptr && ctab != nullptr && ((uintptr_t)ctab & 3) == 0),
                 "%s: colour and a 4-byte aligned ctab are required", what);
  NASSEG_REQUIRE((int64_t)9 * (Ho + Wo) < ((int64_t)1 << 31), "%s: output too large", what);
  const int64_t npix = (int64_t)Ho * Wo;
  NASSEG_REQUIRE(cdiv64(npix, 256) < ((int64_t)1 << 31), "%s: output too large", what);
  hipLaunchKernelGGL(augment_kernel<COLOUR>, dim3((unsigned)cdiv64(npix, 256), B), dim3(256), 0, (hipStream_t)stream,
                     src, src_bytes, desc, taps, colour, ctab, lut, image, mask, Ho, Wo);
  NASSEG_LAUNCH_CHECK(what);
  return NASSEG_OK;
}

template <bool COLOUR>
int launch_augment_depth(const char* what, const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps,
                         const int32_t* colour, const uint8_t* ctab, const act_t* lut, const float* params,
                         float depth_scale, act_t* image, float* target, int B, int Ho, int Wo, void* stream) {
  NASSEG_REQUIRE(B > 0 && B <= 65535 && Ho > 0 && Wo > 0 && src_bytes > 0, "%s: bad shape", what);
  NASSEG_REQUIRE(params != nullptr && target != nullptr, "%s: params and target are required", what);
  NASSEG_REQUIRE(!COLOUR || (colour != nullptr && ctab != nullptr && ((uintptr_t)ctab & 3) == 0),
                 "%s: colour and a 4-byte aligned ctab are required", what);
  NASSEG_REQUIRE((int64_t)9 * (Ho + Wo) < ((int64_t)1 << 31), "%s: output too large", what);
  const int64_t npix = (int64_t)Ho * Wo;
  NASSEG_REQUIRE(cdiv64(npix, 256) < ((int64_t)1 << 31), "%s: output too large", what);
  hipLaunchKernelGGL(augment_depth_kernel<COLOUR>, dim3((unsigned)cdiv64(npix, 256), B), dim3(256), 0,
                     (hipStream_t)stream, src, src_bytes, desc, taps, colour, ctab, lut, params, depth_scale, image,
                     target, Ho, Wo);
  NASSEG_LAUNCH_CHECK(what);
  return NASSEG_OK;
}

}  // namespace

extern "C" {

int NASSEG_FN(augment)(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps,
                       const act_t* lut, act_t* image, uint8_t* mask, int B, int Ho, int Wo, void* stream) {
  return launch_augment<false>("augment", src, src_bytes, desc, taps, nullptr, nullptr, lut, image, mask, B, Ho, Wo,
                               stream);
}

int NASSEG_FN(augment_colour)(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps,
                              const int32_t* colour, const uint8_t* ctab, const act_t* lut, act_t* image,
                              uint8_t* mask, int B, int Ho, int Wo, void* stream) {
  return launch_augment<true>("augment_colour", src, src_bytes, desc, taps, colour, ctab, lut, image, mask, B, Ho, Wo,
                              stream);
}

int NASSEG_FN(augment_depth)(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps,
                             const act_t* lut, const float* params, float depth_scale, act_t* image, float* target,
                             int B, int Ho, int Wo, void* stream) {
  return launch_augment_depth<false>("augment_depth", src, src_bytes, desc, taps, nullptr, nullptr, lut, params,
                                     depth_scale, image, target, B, Ho, Wo, stream);
}

int NASSEG_FN(augment_depth_colour)(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps,
                                    const int32_t* colour, const uint8_t* ctab, const act_t* lut, const float* params,
                                    float depth_scale, act_t* image, float* target, int B, int Ho, int Wo,
                                    void* stream) {
  return launch_augment_depth<true>("augment_depth_colour", src, src_bytes, desc, taps, colour, ctab, lut, params,
                                    depth_scale, image, target, B, Ho, Wo, stream);
}

}  // extern "C"
