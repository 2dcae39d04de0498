// Sample augmentation of the data pipeline (data/datasets.py, planned by data/device.py): OpenCV's fixed-point
// INTER_CUBIC resize, crops, mirror and constant borders, Normalise and the cast of the engine's image, in one
// gather per batch.  The host hands over per-axis tables - four source indices and four 11-bit coefficients per
// output row / column (index -1: a fill pixel), a nearest index per row / column for the target - already rebased to
// the uploaded source window, so the kernel only adds integers: the result is exact by construction, whatever the
// summation order.  The uint8 result v of channel c becomes lut[c][v] (Normalise evaluated by the host in float64
// and cast to act_t there).
//
// One kernel, augment_kernel<COLOUR, Target>, with two targets.  LabelTarget: the target windows hold a byte per
// pixel and the output is that byte, or the descriptor's mask fill.  DepthTarget: the windows hold little-endian 16-bit
// counts and the output is fp32 metres, count * depth_scale / zoom[b], each operation rounded once as numpy's float32
// product and quotient are (__fmul_rn, __fdiv_rn: no contraction, no reciprocal), or the sample's fill, written as it
// is.  A packed target window may start at any byte (an image of odd 3 h w bytes precedes it), so a count is read as
// TWO BYTE LOADS and put together in a register: the target half issues no 16-bit load, aligned or not, and the host
// packs without padding.
//
// COLOUR (nasseg_augment_colour, nasseg_augment_depth_colour: data/datasets.py's ColourJitter) is augment_image's
// compile-time switch: a live pixel's resampled uint8 triple v goes through the sample's 12-bit colour matrix,
// m[c] = clip((sum_k q[c][k] v[k] + 2048) >> 12, 0, 255) (arithmetic shift, skipped
// unless the sample's word 9 is set), then through the sample's byte table ctab[c][m[c]], then through lut as before.
// A fill pixel goes from the descriptor's fill straight to lut: the host has jittered that fill where its pipeline does.
// The sum is int32: each coefficient is clamped to |q| <= 2^15 as it is read (the planner refuses larger ones), so
// |sum| <= 3 * 2^15 * 255 + 2^11 < 2^25 whatever `colour` holds, and every table index is a value clipped to 0..255.
// The sample's 12 words are uniform per workgroup (blockIdx.y); its 768 table bytes sit in LDS beside lut.
#include "common.h"

namespace {

// per-sample descriptor: int64 [AUG_DESC]
enum { AUG_IMG_OFF, AUG_MSK_OFF, AUG_H, AUG_W, AUG_IMG_LD, AUG_MSK_LD, AUG_IMG_FILL, AUG_MSK_FILL, AUG_DESC };

// Does the window of h rows of w elements of `elem` bytes, ld bytes apart from byte `off`, lie inside src?  One that
// does not is read as fill (the host checks before it launches; this keeps every load in bounds whatever the kernel
// is handed).  elem: 3 for the image, 1 for a label map, 2 for depth counts.
__device__ __forceinline__ bool window_ok(int64_t off, int64_t ld, int h, int w, int elem, int64_t src_bytes) {
  return h > 0 && w > 0 && off >= 0 && off <= src_bytes && ld >= elem * (int64_t)w && ld <= src_bytes &&
         off + (h - 1) * ld + elem * (int64_t)w <= src_bytes;
}

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
  const bool img_ok = window_ok(img_off, img_ld, h, w, 3, src_bytes);

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

// The target half of a pixel, passed to the kernel by value: the bytes of an element of the packed window, what the
// half needs of sample b (descriptor d; `of`, read before the kernel stores anything, so that the loads stay scalar:
// a pointer inside a struct is no __restrict__ kernel argument), what a fill pixel and a live pixel (c: its element in
// src) become, and where they go.
struct LabelTarget {
  typedef uint8_t out_t;
  typedef int sample_t;  // the descriptor's mask fill
  static constexpr int ELEM = 1;
  uint8_t* out;  // [B][Ho][Wo]; null: no mask is written (an image alone: F.prepare_image)
  __device__ bool skip() const { return out == nullptr; }
  __device__ sample_t of(const int64_t* d, int b) const { return (int)d[AUG_MSK_FILL]; }
  __device__ out_t fill(sample_t s) const { return (out_t)s; }
  __device__ out_t live(const uint8_t* c, sample_t s) const { return c[0]; }
};

struct DepthTarget {
  typedef float out_t;
  typedef float2 sample_t;  // params[b] = {zoom, fill}; the descriptor's mask fill is not read
  static constexpr int ELEM = 2;
  float* out;           // [B][Ho][Wo], always written
  const float* params;  // [B][2]
  float depth_scale;
  __device__ bool skip() const { return false; }
  __device__ sample_t of(const int64_t* d, int b) const { return make_float2(params[2 * b], params[2 * b + 1]); }
  // a pad comes after the resize on the host, so the fill is not divided
  __device__ out_t fill(sample_t s) const { return s.y; }
  __device__ out_t live(const uint8_t* c, sample_t s) const {
    // two byte loads that stay two: the compiler fuses adjacent byte loads into one 16-bit load (here at an address
    // that may be odd) when it can see that they are adjacent, so the high byte's offset passes through an empty asm
    int hi_at = 1;
    asm volatile("" : "+v"(hi_at));
    const int count = (int)c[0] | ((int)c[hi_at] << 8);
    return __fdiv_rn(__fmul_rn((float)count, depth_scale), s.x);
  }
};

// one thread per output pixel of one sample (blockIdx.y), the pixels of a sample in row-major order: a wave writes
// 64 consecutive pixels (768 contiguous bytes of fp32 image, 64 of mask or 256 of depth target), and the few output
// rows a workgroup covers read the same four source rows, which stay in L1 / L2 between the lanes that share them.
// The target window of sample b holds h rows of w elements, msk_ld BYTES apart (>= Target::ELEM * w).
// COLOUR: colour int32 [B][12] and ctab uint8 [B][3][256] (4-byte aligned: copied as 192 words) are read, else ignored.
template <bool COLOUR, typename Target>
__global__ __launch_bounds__(256) void augment_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                      const int64_t* __restrict__ desc,
                                                      const int* __restrict__ taps,
                                                      const int32_t* __restrict__ colour,
                                                      const uint8_t* __restrict__ ctab,
                                                      const act_t* __restrict__ lut, act_t* __restrict__ image,
                                                      Target target, int Ho, int Wo) {
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
  const typename Target::sample_t of_sample = target.of(d, b);
  // (for counts, the last byte read is the high byte of the last count of the last row)
  const bool msk_ok = window_ok(msk_off, msk_ld, h, w, Target::ELEM, src_bytes);

  // tables of the sample: rows [Ho][8], columns [Wo][8] (4 indices, 4 coefficients), target rows [Ho], columns [Wo]
  const int* t = taps + (int64_t)b * (9 * (Ho + Wo));
  const int my = t[8 * (Ho + Wo) + oy], mx = t[8 * (Ho + Wo) + Ho + ox];

  augment_image<COLOUR>(src, src_bytes, img_off, h, w, img_ld, img_fill, t, slut, image + ((int64_t)b * npix + p) * 3,
                        oy, ox, Ho, COLOUR ? colour + (int64_t)b * 12 : nullptr, (const uint8_t*)stab);

  if (target.skip()) return;
  typename Target::out_t v = target.fill(of_sample);
  if (my >= 0 && mx >= 0 && msk_ok)
    v = target.live(src + msk_off + (int64_t)min(my, h - 1) * msk_ld + Target::ELEM * (int64_t)min(mx, w - 1),
                    of_sample);
  target.out[(int64_t)b * npix + p] = v;
}

// the launch of the four entry points: one check, one grid (one thread per output pixel, blockIdx.y = sample)
template <bool COLOUR, typename Target>
int launch_augment(const char* what, const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps,
                   const int32_t* colour, const uint8_t* ctab, const act_t* lut, act_t* image, Target target, int B,
                   int Ho, int Wo, void* stream) {
  NASSEG_REQUIRE(B > 0 && B <= 65535 && Ho > 0 && Wo > 0 && src_bytes > 0, "%s: bad shape", what);
  NASSEG_REQUIRE(!COLOUR || (colour != nullptr && ctab != nullptr && ((uintptr_t)ctab & 3) == 0),
                 "%s: colour and a 4-byte aligned ctab are required", what);
  NASSEG_REQUIRE((int64_t)9 * (Ho + Wo) < ((int64_t)1 << 31), "%s: output too large", what);
  const int64_t npix = (int64_t)Ho * Wo;
  NASSEG_REQUIRE(cdiv64(npix, 256) < ((int64_t)1 << 31), "%s: output too large", what);
  hipLaunchKernelGGL((augment_kernel<COLOUR, Target>), dim3((unsigned)cdiv64(npix, 256), B), dim3(256), 0,
                     (hipStream_t)stream, src, src_bytes, desc, taps, colour, ctab, lut, image, target, Ho, Wo);
  NASSEG_LAUNCH_CHECK(what);
  return NASSEG_OK;
}

// the depth entry points: a label launch may go without its mask, a depth launch not without its target
template <bool COLOUR>
int launch_augment_depth(const char* what, const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps,
                         const int32_t* colour, const uint8_t* ctab, const act_t* lut, const float* params,
                         float depth_scale, act_t* image, float* target, int B, int Ho, int Wo, void* stream) {
  NASSEG_REQUIRE(params != nullptr && target != nullptr, "%s: params and target are required", what);
  return launch_augment<COLOUR>(what, src, src_bytes, desc, taps, colour, ctab, lut, image,
                                DepthTarget{target, params, depth_scale}, B, Ho, Wo, stream);
}

}  // namespace

extern "C" {

int NASSEG_FN(augment)(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps,
                       const act_t* lut, act_t* image, uint8_t* mask, int B, int Ho, int Wo, void* stream) {
  return launch_augment<false>("augment", src, src_bytes, desc, taps, nullptr, nullptr, lut, image, LabelTarget{mask},
                               B, Ho, Wo, stream);
}

int NASSEG_FN(augment_colour)(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int* taps,
                              const int32_t* colour, const uint8_t* ctab, const act_t* lut, act_t* image,
                              uint8_t* mask, int B, int Ho, int Wo, void* stream) {
  return launch_augment<true>("augment_colour", src, src_bytes, desc, taps, colour, ctab, lut, image,
                              LabelTarget{mask}, B, Ho, Wo, stream);
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
