// Lovasz-Softmax term of the segmentation criterion (Berman, Triggs, Blaschko, CVPR 2018; definition:
// include/nasseg.h), gfx950: per class a stable segmented radix sort of the errors on the device, an integer scan of
// the foreground counts over the sorted order, and the Lovasz gradient in fp64 from those integers.
//
// The sort: least-significant-digit radix sort, 4 passes of 8 bits, classes as grid rows (blockIdx.y = class, absent
// classes return at once unless every class takes part), tiles of kLovTile = 4096 keys per workgroup.
//   key     = bit pattern of e, complemented below the sign bit (descending e = ascending key); 0xffffffff on a pixel
//             that is not valid, which therefore sorts behind every valid one
//   payload = flat pixel index p (< 2^30) | foreground flag [t_p == c] << 31, made by the first pass
// A pass is three launches: per-tile digit histograms (LDS integer atomics: counts have no order), an exclusive scan
// of every row hist[class][digit][.] over the tiles with the row totals (one wave per row; the scatter scans the 256
// totals of its class itself), and the scatter.  The scatter is STABLE - equal digits keep
// their order, which after four passes is ascending p among equal errors: a tile is cut into four contiguous
// quarters, one per wave; a wave walks its quarter 64 keys at a time, finds the lanes holding its digit with eight
// 64-bit ballots, ranks a key by the popcount of the lower lanes plus the wave's running count of that digit (a table
// only this wave touches), and the four waves' totals are put in wave order by the thread that owns the digit.  No
// atomic takes part in any rank.  The tile is brought into digit order in LDS before it is stored, so that the stores
// are runs of consecutive addresses.
// Everything is launched with a geometry that depends on (P, C) alone: capturable; no allocation, no float atomics.
#include <math.h>

#define NASSEG_LOSS_NO_SUM_PASS  // (nothing here sums per-pixel losses)
#include "loss_common.h"

namespace {

constexpr int kLovItems = 16;
constexpr int kLovTile = 256 * kLovItems;
constexpr int kLovCntLds = 1024;  // classes counted through LDS (more: global integer atomics)
constexpr uint32_t kLovInvalid = 0xffffffffu;
constexpr uint32_t kLovIndex = 0x7fffffffu;

__device__ __forceinline__ uint32_t lov_key(float e) { return (__float_as_uint(e) & 0x7fffffffu) ^ 0x7fffffffu; }
__device__ __forceinline__ float lov_error(uint32_t key) { return __uint_as_float(key ^ 0x7fffffffu); }

__device__ __forceinline__ int64_t lov_label(const void* target, int elem_size, int64_t p) {
  return elem_size == 8 ? ((const int64_t*)target)[p] : (int64_t)((const uint8_t*)target)[p];
}

// cnt = {N_c} (C words) | n | |K|
__global__ __launch_bounds__(256) void lov_zero_kernel(uint32_t* __restrict__ cnt, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) cnt[i] = 0u;
}

// One [np][C] tile between memory and LDS rows of stride CS = C | 1 (odd: a lane per row meets no bank conflict):
// consecutive lanes touch consecutive elements, whatever the alignment.
template <typename T>
__device__ __forceinline__ void lov_stage(const T* __restrict__ src, float* __restrict__ tile, int nel, int C, int CS,
                                          int tid) {
  for (int i = tid; i < nel; i += 256) {
    const int pix = i / C;
    tile[pix * CS + (i - pix * C)] = lda1(src + i);
  }
}

// errors[p][c] = |y_pc - q_pc| (-1 on a pixel that is not valid); q = exp(x - max) * (1 / sum), the very operations
// of the region term and of nasseg_ce_fwd, the product and the difference rounded separately (no contraction): a
// function of the pixel's own row.  `row` (stride 1) holds x and receives the errors.
__device__ __forceinline__ void lov_err_row(float* __restrict__ row, int64_t t, int C, int ignore) {
  if (!label_valid(t, C, ignore)) {
    for (int c = 0; c < C; ++c) row[c] = -1.f;
    return;
  }
  float m = row[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, row[c]);
  float s = 0.f;
  for (int c = 0; c < C; ++c) {
    const float e = expf(row[c] - m);
    row[c] = e;
    s += e;
  }
  const float inv = 1.f / s;
  for (int c = 0; c < C; ++c) {
    const float q = __fmul_rn(row[c], inv);
    row[c] = fabsf(__fsub_rn((int64_t)c == t ? 1.f : 0.f, q));
  }
}

// C <= 63: a workgroup's 256 pixels are 256 * C contiguous values, staged through LDS so that loads and stores are
// coalesced; each lane works on its pixel's row in LDS.
template <typename TL>
__global__ __launch_bounds__(256) void lov_err_tile_kernel(const act_t* __restrict__ logits,
                                                           const TL* __restrict__ target, int64_t P, int C,
                                                           int ignore, float* __restrict__ errors) {
  extern __shared__ float tile[];  // [256][C | 1]
  const int CS = C | 1, tid = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * 256;
  const int np = (int)((P - p0) < 256 ? (P - p0) : 256);
  lov_stage(logits + p0 * C, tile, np * C, C, CS, tid);
  __syncthreads();
  if (tid < np) lov_err_row(tile + tid * CS, (int64_t)target[p0 + tid], C, ignore);
  __syncthreads();
  float* dst = errors + p0 * C;
  for (int i = tid; i < np * C; i += 256) {
    const int pix = i / C;
    dst[i] = tile[pix * CS + (i - pix * C)];
  }
}

// Any C: one lane per pixel straight from memory, the same arithmetic (the row passes through the errors' own row).
template <typename TL>
__global__ __launch_bounds__(256) void lov_err_kernel(const act_t* __restrict__ logits,
                                                      const TL* __restrict__ target, int64_t P, int C, int ignore,
                                                      float* __restrict__ errors) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const act_t* lp = logits + p * C;
  float* ep = errors + p * C;
  for (int c = 0; c < C; ++c) ep[c] = lda1(lp + c);
  lov_err_row(ep, (int64_t)target[p], C, ignore);
}

// keys[c][p] from errors[p][c] (one lane per pixel: its row is read once, the stores are coalesced per class), and
// the counts N_c and n.
__global__ __launch_bounds__(256) void lov_keys_kernel(const float* __restrict__ errors, const void* __restrict__ target,
                                                       int elem_size, int64_t P, int C, int ignore,
                                                       uint32_t* __restrict__ keys, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t lc[kLovCntLds + 1];
  const int tid = threadIdx.x;
  const bool in_lds = C <= kLovCntLds;
  if (in_lds) {
    for (int i = tid; i <= C; i += 256) lc[i] = 0u;
    __syncthreads();
  }
  const int64_t p = (int64_t)blockIdx.x * 256 + tid;
  bool valid = false;
  int64_t t = -1;
  if (p < P) {
    t = lov_label(target, elem_size, p);
    valid = label_valid(t, C, ignore);
  }
  const int nv = __popcll(__ballot(valid));
  if (in_lds) {
    if (valid) atomicAdd(&lc[t], 1u);
    if ((tid & 63) == 0 && nv) atomicAdd(&lc[C], (uint32_t)nv);
  } else {
    if (valid) atomicAdd(&cnt[t], 1u);
    if ((tid & 63) == 0 && nv) atomicAdd(&cnt[C], (uint32_t)nv);
  }
  if (p < P) {
    const float* ep = errors + p * C;
    for (int c = 0; c < C; ++c) keys[(int64_t)c * P + p] = valid ? lov_key(ep[c]) : kLovInvalid;
  }
  if (in_lds) {
    __syncthreads();
    for (int i = tid; i <= C; i += 256)
      if (lc[i]) atomicAdd(&cnt[i], lc[i]);
  }
}

// ncls = {N_c} | |K| as int64; cnt[C + 1] = |K|
__global__ __launch_bounds__(256) void lov_meta_kernel(uint32_t* __restrict__ cnt, int C, int all,
                                                       int64_t* __restrict__ ncls) {
  __shared__ uint32_t red[256];
  uint32_t k = 0;
  for (int c = threadIdx.x; c < C; c += 256) {
    const uint32_t v = cnt[c];
    ncls[c] = (int64_t)v;
    k += v > 0u ? 1u : 0u;
  }
  red[threadIdx.x] = k;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const uint32_t K = all ? (uint32_t)C : red[0];
    cnt[C + 1] = K;
    ncls[C] = (int64_t)K;
  }
}

__device__ __forceinline__ bool lov_skip(const uint32_t* __restrict__ cnt, int c, int all) {
  return !all && cnt[c] == 0u;  // (uniform over the workgroup)
}

// hist[c][digit][tile] = keys of the tile with that digit
__global__ __launch_bounds__(256) void lov_hist_kernel(const uint32_t* __restrict__ keys, int64_t P, int nb, int shift,
                                                       int all, const uint32_t* __restrict__ cnt,
                                                       uint32_t* __restrict__ hist) {
  const int c = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
  if (lov_skip(cnt, c, all)) return;
  __shared__ uint32_t lh[256];
  lh[tid] = 0u;
  __syncthreads();
  const uint32_t* k = keys + (int64_t)c * P;
  const int64_t base = (int64_t)b * kLovTile;
#pragma unroll
  for (int i = 0; i < kLovItems; ++i) {
    const int64_t pos = base + i * 256 + tid;
    if (pos < P) atomicAdd(&lh[(k[pos] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[((int64_t)c * 256 + tid) * nb + b] = lh[tid];
}

// In place, one wave per row of nb words: row -> its exclusive prefix sums, the row's total -> tot[row] (tot may be
// null).  Row r = blockIdx.y * gridDim.x + blockIdx.x belongs to class blockIdx.y.  For the histograms a row is one
// (class, digit): hist[c][d][0 .. nb) becomes the keys with digit d in the tiles before, tot[c][d] all keys with digit
// d - the scatter adds the digits below d by itself.
__global__ __launch_bounds__(64) void lov_rowscan_kernel(uint32_t* __restrict__ v, int nb, uint32_t* __restrict__ tot,
                                                         int all, const uint32_t* __restrict__ cnt) {
  const int c = blockIdx.y, lane = threadIdx.x;
  if (lov_skip(cnt, c, all)) return;
  const int64_t r = (int64_t)c * gridDim.x + blockIdx.x;
  uint32_t* row = v + r * nb;
  uint32_t carry = 0u;
  for (int j0 = 0; j0 < nb; j0 += 64) {
    const int j = j0 + lane;
    const uint32_t x = j < nb ? row[j] : 0u;
    uint32_t incl = x;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = __shfl_up(incl, off);
      if (lane >= off) incl += o;
    }
    if (j < nb) row[j] = carry + incl - x;
    carry += __shfl(incl, 63);
  }
  if (tot && lane == 0) tot[r] = carry;
}

// One stable scatter pass (see the head of this file).  FIRST: the payload is made here (p | foreground << 31).
template <bool FIRST>
__global__ __launch_bounds__(256) void lov_scatter_kernel(const uint32_t* __restrict__ kin,
                                                          const uint32_t* __restrict__ vin,
                                                          uint32_t* __restrict__ kout, uint32_t* __restrict__ vout,
                                                          const uint32_t* __restrict__ hist,
                                                          const uint32_t* __restrict__ tot, int64_t P, int nb,
                                                          int shift, int all, const uint32_t* __restrict__ cnt,
                                                          const void* __restrict__ target, int elem_size) {
  const int c = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (lov_skip(cnt, c, all)) return;
  __shared__ uint32_t wcnt[4][256];
#pragma unroll
  for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0u;
  __syncthreads();
  const int64_t row = (int64_t)c * P;
  const int64_t base = (int64_t)b * kLovTile + wave * (64 * kLovItems) + lane;
  const uint64_t lower = ((uint64_t)1 << lane) - 1;
  uint32_t key[kLovItems], rk[kLovItems];
#pragma unroll
  for (int i = 0; i < kLovItems; ++i) {
    const int64_t pos = base + i * 64;
    const bool in = pos < P;
    key[i] = in ? kin[row + pos] : kLovInvalid;
    const uint32_t d = (key[i] >> shift) & 255u;
    uint64_t peers = __ballot(in);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool one = (d >> bit) & 1u;
      const uint64_t m = __ballot(one);
      peers &= one ? m : ~m;
    }
    const int leader = in ? __ffsll((unsigned long long)peers) - 1 : lane;
    uint32_t pre = 0u;
    if (in && lane == leader) {
      pre = wcnt[wave][d];
      wcnt[wave][d] = pre + (uint32_t)__popcll(peers);
    }
    pre = __shfl(pre, leader);
    rk[i] = pre + (uint32_t)__popcll(peers & lower);
    __syncthreads();
  }
  // Thread d: G = the keys with a digit below d in the whole row (a scan of tot over the 256 digits) plus those with
  // digit d in the tiles before (hist, scanned); ls = the keys of this tile with a digit below d.  The tile is put in
  // digit order in LDS first (position ls + the waves before + the rank in the wave), so that the stores to memory run
  // through consecutive addresses per digit: element j of the ordered tile goes to G[d] + (j - ls[d]).
  __shared__ uint32_t skey[kLovTile], sval[kLovTile];
  __shared__ uint32_t gofs[256];
  __shared__ uint32_t dsum[4], lsum[4];
  {
    const uint32_t c0 = wcnt[0][tid], c1 = wcnt[1][tid], c2 = wcnt[2][tid], c3 = wcnt[3][tid];
    const uint32_t td = tot[(int64_t)c * 256 + tid], tl = c0 + c1 + c2 + c3;
    uint32_t incl = td, lincl = tl;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = __shfl_up(incl, off), lo = __shfl_up(lincl, off);
      if (lane >= off) {
        incl += o;
        lincl += lo;
      }
    }
    if (lane == 63) {
      dsum[wave] = incl;
      lsum[wave] = lincl;
    }
    __syncthreads();
    uint32_t g = hist[((int64_t)c * 256 + tid) * nb + b] + (incl - td);
    uint32_t ls = lincl - tl;
    for (int w = 0; w < wave; ++w) {
      g += dsum[w];
      ls += lsum[w];
    }
    wcnt[0][tid] = ls;
    wcnt[1][tid] = ls + c0;
    wcnt[2][tid] = ls + c0 + c1;
    wcnt[3][tid] = ls + c0 + c1 + c2;
    gofs[tid] = g - ls;  // (modulo 2^32, undone by the addition below)
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kLovItems; ++i) {
    const int64_t pos = base + i * 64;
    if (pos >= P) continue;
    const uint32_t d = (key[i] >> shift) & 255u;
    const uint32_t lp = wcnt[wave][d] + rk[i];
    if (lp >= (uint32_t)kLovTile) continue;  // (cannot happen; never write outside the tile)
    skey[lp] = key[i];
    if (FIRST)
      sval[lp] = (uint32_t)pos | (lov_label(target, elem_size, pos) == (int64_t)c ? 0x80000000u : 0u);
    else
      sval[lp] = vin[row + pos];
  }
  __syncthreads();
  const int64_t left = P - (int64_t)b * kLovTile;
  const int ntile = left < kLovTile ? (int)left : kLovTile;
#pragma unroll
  for (int i = 0; i < kLovItems; ++i) {
    const int j = i * 256 + tid;
    if (j >= ntile) continue;
    const uint32_t k = skey[j];
    const int64_t dst = (int64_t)(uint32_t)(gofs[(k >> shift) & 255u] + (uint32_t)j);
    if (dst >= P) continue;  // (cannot happen with a consistent histogram; never write outside the row)
    kout[row + dst] = k;
    vout[row + dst] = sval[j];
  }
}

// fgc[c][tile] = foreground pixels among the tile's valid positions of the sorted order (positions < n)
__global__ __launch_bounds__(256) void lov_fgcount_kernel(const uint32_t* __restrict__ vals, int64_t P, int C, int nb,
                                                          int all, const uint32_t* __restrict__ cnt,
                                                          uint32_t* __restrict__ fgc) {
  const int c = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
  if (lov_skip(cnt, c, all)) return;
  __shared__ uint32_t red[4];
  const int64_t n = (int64_t)cnt[C];
  const uint32_t* v = vals + (int64_t)c * P;
  const int64_t base = (int64_t)b * kLovTile;
  uint32_t f = 0u;
#pragma unroll
  for (int i = 0; i < kLovItems; ++i) {
    const int64_t pos = base + i * 256 + tid;
    if (pos < n) f += v[pos] >> 31;
  }
  for (int off = 32; off > 0; off >>= 1) f += __shfl_xor(f, off);
  if ((tid & 63) == 0) red[tid >> 6] = f;
  __syncthreads();
  if (tid == 0) fgc[(int64_t)c * nb + b] = red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ double lov_wave_allsum(double v) {  // (a fixed butterfly: the same pairing every time)
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Over the sorted order of class c: F_i by ballots within the tile on top of the scanned tile counts, the Lovasz
// gradient g_i in fp64 from the integers, coef[p][c] = -+ g_i / |K|, rank[p][c] = i - 1, and the tile's share of
// sum_i e_(i) g_i -> part[c][tile] (each lane its keys in order, a butterfly, the four waves in order).
// A class outside K: zeros and -1, its tile of pixels taken in place.
__global__ __launch_bounds__(256) void lov_grad_kernel(const uint32_t* __restrict__ keys,
                                                       const uint32_t* __restrict__ vals,
                                                       const uint32_t* __restrict__ fgx,
                                                       const uint32_t* __restrict__ cnt, int64_t P, int C, int nb,
                                                       int all, float* __restrict__ coef, int* __restrict__ rank,
                                                       double* __restrict__ part) {
  const int c = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (lov_skip(cnt, c, all)) {
    const int64_t base = (int64_t)b * kLovTile;
    for (int i = 0; i < kLovItems; ++i) {
      const int64_t p = base + i * 256 + tid;
      if (p < P) {
        coef[p * C + c] = 0.f;
        if (rank) rank[p * C + c] = -1;
      }
    }
    if (tid == 0) part[(int64_t)c * nb + b] = 0.0;
    return;
  }
  __shared__ uint32_t wtot[4];
  __shared__ double red[4];
  const int64_t n = (int64_t)cnt[C];
  const int64_t Nc = (int64_t)cnt[c];
  const double invK = 1.0 / (double)cnt[C + 1];
  const int64_t row = (int64_t)c * P;
  const int64_t base = (int64_t)b * kLovTile + wave * (64 * kLovItems) + lane;
  const uint64_t upto = (((uint64_t)1 << lane) - 1) | ((uint64_t)1 << lane);
  uint32_t v[kLovItems], incl[kLovItems];
  uint32_t run = 0u;
#pragma unroll
  for (int i = 0; i < kLovItems; ++i) {
    const int64_t pos = base + i * 64;
    v[i] = pos < P ? vals[row + pos] : 0u;
    const uint64_t m = __ballot(pos < n && (v[i] >> 31) != 0u);
    incl[i] = run + (uint32_t)__popcll(m & upto);
    run += (uint32_t)__popcll(m);
  }
  if (lane == 0) wtot[wave] = run;
  __syncthreads();
  uint32_t off = fgx[(int64_t)c * nb + b];
  for (int w = 0; w < wave; ++w) off += wtot[w];
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < kLovItems; ++i) {
    const int64_t pos = base + i * 64;
    if (pos >= P) continue;
    const int64_t o = (int64_t)(v[i] & kLovIndex) * C + c;
    if (pos < n) {
      const bool fg = (v[i] >> 31) != 0u;
      const int64_t F = (int64_t)off + incl[i];
      const int64_t U = Nc + (pos + 1 - F);
      double g;
      if (fg)
        g = 1.0 / (double)U;
      else
        g = U - 1 > 0 ? (double)(Nc - F) / ((double)(U - 1) * (double)U) : 1.0;
      acc += (double)lov_error(keys[row + pos]) * g;
      coef[o] = (float)((fg ? -g : g) * invK);
      if (rank) rank[o] = (int)pos;
    } else {
      coef[o] = 0.f;
      if (rank) rank[o] = -1;
    }
  }
  acc = lov_wave_allsum(acc);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (tid == 0) part[(int64_t)c * nb + b] = ((red[0] + red[1]) + red[2]) + red[3];
}

// loss_c = the tiles' shares added in tile order; L = sum_{c in K} loss_c / |K| in class order (0 when K is empty);
// loss = [base +] lweight * L.  All in fp64.
__global__ __launch_bounds__(256) void lov_final_kernel(const double* __restrict__ part,
                                                        const uint32_t* __restrict__ cnt, int C, int nb, int all,
                                                        double lweight, const float* __restrict__ base,
                                                        float* __restrict__ loss, float* __restrict__ llov,
                                                        double* __restrict__ lossc) {
  for (int c = threadIdx.x; c < C; c += 256) {
    double s = 0.0;
    if (!lov_skip(cnt, c, all)) {
      const double* r = part + (int64_t)c * nb;
      for (int b = 0; b < nb; ++b) s += r[b];
    }
    lossc[c] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t K = cnt[C + 1];
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += lossc[c];
    const float L = K > 0u ? (float)(s / (double)K) : 0.f;
    if (llov) llov[0] = L;
    loss[0] = (float)((base ? (double)base[0] : 0.0) + lweight * (double)L);
  }
}

// d = gscale * lweight * q_j (G_j - sum_c G_c q_c) on valid pixels, exact zeros elsewhere; accumulate: added onto what
// dlogits holds (the cross-entropy's gradient, written just before by nasseg_ce_sel_bwd / nasseg_ce_region_bwd).
// Evaluated as q_j ((G_j - G_a) - sum_c (G_c - G_a) q_c) with a = the row's arg max: the same number (sum_c q_c = 1),
// but no term of the sum carries q_a, which may be 1 - 1e-4 while the result hangs on the 1e-4: the small q_c keep
// their relative accuracy, 1 - q_a formed from a rounded q_a would not (an absent class under all_classes puts a G of
// 1 / |K| on exactly such a pixel).
// x: the row's logits, G: its coefficients (stride 1 both); x receives the gradient.
__device__ __forceinline__ void lov_bwd_row(float* __restrict__ x, const float* __restrict__ G, int C, float gl) {
  float m = x[0];
  int a = 0;
  for (int c = 1; c < C; ++c) {
    if (x[c] > m) {
      m = x[c];
      a = c;
    }
  }
  const float ga = G[a];
  float s = 0.f, dot = 0.f;
  for (int c = 0; c < C; ++c) {
    const float e = expf(x[c] - m);
    x[c] = e;
    s += e;
    dot = fmaf(G[c] - ga, e, dot);
  }
  const float inv = 1.f / s;
  dot *= inv;
  for (int c = 0; c < C; ++c) x[c] = gl * ((x[c] * inv) * ((G[c] - ga) - dot));
}

// C <= 31: logits and coefficients staged through two LDS tiles, the gradient stored (or added) coalesced.
template <typename TL>
__global__ __launch_bounds__(256) void lov_bwd_tile_kernel(const act_t* __restrict__ logits,
                                                           const TL* __restrict__ target,
                                                           const float* __restrict__ coef,
                                                           const float* __restrict__ gscale, float lweight,
                                                           int accumulate, int64_t P, int C, int ignore,
                                                           act_t* __restrict__ dlogits) {
  extern __shared__ float tile[];  // x [256][C | 1] | G [256][C | 1]
  const int CS = C | 1, tid = threadIdx.x;
  float* gt = tile + 256 * CS;
  const float gl = (gscale ? gscale[0] : 1.f) * lweight;
  const int64_t p0 = (int64_t)blockIdx.x * 256;
  const int np = (int)((P - p0) < 256 ? (P - p0) : 256);
  lov_stage(logits + p0 * C, tile, np * C, C, CS, tid);
  lov_stage(coef + p0 * C, gt, np * C, C, CS, tid);
  __syncthreads();
  if (tid < np) {
    float* row = tile + tid * CS;
    if (label_valid((int64_t)target[p0 + tid], C, ignore))
      lov_bwd_row(row, gt + tid * CS, C, gl);
    else
      for (int c = 0; c < C; ++c) row[c] = 0.f;
  }
  __syncthreads();
  act_t* dst = dlogits + p0 * C;
  for (int i = tid; i < np * C; i += 256) {
    const int pix = i / C;
    const float d = tile[pix * CS + (i - pix * C)];
    sta1(dst + i, accumulate ? lda1(dst + i) + d : d);
  }
}

// Any C: one lane per pixel straight from memory (the exponentials are taken twice instead of kept).
template <typename TL>
__global__ __launch_bounds__(256) void lov_bwd_kernel(const act_t* __restrict__ logits, const TL* __restrict__ target,
                                                      const float* __restrict__ coef,
                                                      const float* __restrict__ gscale, float lweight,
                                                      int accumulate, int64_t P, int C, int ignore,
                                                      act_t* __restrict__ dlogits) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const float gl = (gscale ? gscale[0] : 1.f) * lweight;
  const int64_t t = (int64_t)target[p];
  const act_t* lp = logits + p * C;
  const float* gp = coef + p * C;
  act_t* dp = dlogits + p * C;
  if (!label_valid(t, C, ignore)) {
    if (!accumulate)
      for (int c = 0; c < C; ++c) sta1(dp + c, 0.f);
    return;
  }
  float m = lda1(lp);
  int a = 0;
  for (int c = 1; c < C; ++c) {
    const float x = lda1(lp + c);
    if (x > m) {
      m = x;
      a = c;
    }
  }
  const float ga = gp[a];
  float s = 0.f, dot = 0.f;
  for (int c = 0; c < C; ++c) {
    const float e = expf(lda1(lp + c) - m);
    s += e;
    dot = fmaf(gp[c] - ga, e, dot);
  }
  const float inv = 1.f / s;
  dot *= inv;
  for (int c = 0; c < C; ++c) {
    const float d = gl * ((expf(lda1(lp + c) - m) * inv) * ((gp[c] - ga) - dot));
    sta1(dp + c, accumulate ? lda1(dp + c) + d : d);
  }
}

// Workspace, in 4-byte words: cnt (C + 2, padded to even) | lossc fp64 [C] | part fp64 [C][nb] | fgc [C][nb] |
// tot [C][256] | hist [C][256][nb] | keys A, keys B, payload A, payload B ([C][P] each);  nb = ceil(P / 4096).
struct LovWs {
  uint32_t* cnt;
  double* lossc;
  double* part;
  uint32_t* fgc;
  uint32_t* tot;
  uint32_t* hist;
  uint32_t* key[2];
  uint32_t* val[2];
  int64_t words;
};
LovWs lov_ws(void* ws, int64_t P, int C) {
  const int64_t nb = cdiv64(P, kLovTile);
  LovWs w;
  uint32_t* p = (uint32_t*)ws;
  int64_t o = 0;
  w.cnt = p + o;
  o += (C + 2 + 1) & ~(int64_t)1;
  w.lossc = (double*)(p + o);
  o += 2 * (int64_t)C;
  w.part = (double*)(p + o);
  o += 2 * (int64_t)C * nb;
  w.fgc = p + o;
  o += (int64_t)C * nb;
  w.tot = p + o;
  o += (int64_t)C * 256;
  w.hist = p + o;
  o += (int64_t)C * 256 * nb;
  for (int i = 0; i < 2; ++i) {
    w.key[i] = p + o;
    o += (int64_t)C * P;
    w.val[i] = p + o;
    o += (int64_t)C * P;
  }
  w.words = o;
  return w;
}

// the sort-and-scan half: everything behind the errors
int lov_launch(const float* errors, const void* target, int elem_size, int64_t P, int C, int ignore, int all,
               double lweight, const float* base, float* loss, float* llov, float* coef, int* rank, int64_t* ncls,
               void* ws, hipStream_t s) {
  const LovWs w = lov_ws(ws, P, C);
  const int nb = (int)cdiv64(P, kLovTile);
  const dim3 tiles((unsigned)nb, (unsigned)C);
  hipLaunchKernelGGL(lov_zero_kernel, dim3(cdiv(C + 2, 256)), dim3(256), 0, s, w.cnt, C + 2);
  hipLaunchKernelGGL(lov_keys_kernel, dim3((unsigned)cdiv64(P, 256)), dim3(256), 0, s, errors, target, elem_size, P,
                     C, ignore, w.key[0], w.cnt);
  hipLaunchKernelGGL(lov_meta_kernel, dim3(1), dim3(256), 0, s, w.cnt, C, all, ncls);
  NASSEG_LAUNCH_CHECK("lovasz_keys");
  for (int pass = 0; pass < 4; ++pass) {
    const int in = pass & 1, out = in ^ 1, shift = 8 * pass;
    hipLaunchKernelGGL(lov_hist_kernel, tiles, dim3(256), 0, s, w.key[in], P, nb, shift, all, w.cnt, w.hist);
    hipLaunchKernelGGL(lov_rowscan_kernel, dim3(256, C), dim3(64), 0, s, w.hist, nb, w.tot, all, w.cnt);
    if (pass == 0)
      hipLaunchKernelGGL(lov_scatter_kernel<true>, tiles, dim3(256), 0, s, w.key[in], w.val[in], w.key[out],
                         w.val[out], w.hist, w.tot, P, nb, shift, all, w.cnt, target, elem_size);
    else
      hipLaunchKernelGGL(lov_scatter_kernel<false>, tiles, dim3(256), 0, s, w.key[in], w.val[in], w.key[out],
                         w.val[out], w.hist, w.tot, P, nb, shift, all, w.cnt, target, elem_size);
    NASSEG_LAUNCH_CHECK("lovasz_sort_pass");
  }
  // (four passes: the sorted order is back in buffer 0)
  hipLaunchKernelGGL(lov_fgcount_kernel, tiles, dim3(256), 0, s, w.val[0], P, C, nb, all, w.cnt, w.fgc);
  hipLaunchKernelGGL(lov_rowscan_kernel, dim3(1, C), dim3(64), 0, s, w.fgc, nb, (uint32_t*)nullptr, all, w.cnt);
  hipLaunchKernelGGL(lov_grad_kernel, tiles, dim3(256), 0, s, w.key[0], w.val[0], w.fgc, w.cnt, P, C, nb, all, coef,
                     rank, w.part);
  hipLaunchKernelGGL(lov_final_kernel, dim3(1), dim3(256), 0, s, w.part, w.cnt, C, nb, all, lweight, base, loss, llov,
                     w.lossc);
  NASSEG_LAUNCH_CHECK("lovasz_coef");
  return NASSEG_OK;
}

int lov_check(const char* who, int64_t P, int C, int elem_size) {
  NASSEG_REQUIRE(P > 0 && C >= 2 && C <= 65535, "%s: P > 0 and 2 <= C <= 65535 expected (got P = %lld, C = %d)", who,
                 (long long)P, C);
  NASSEG_REQUIRE(P * (int64_t)C < ((int64_t)1 << 31), "%s: P * C must stay below 2^31 (got %lld x %d)", who,
                 (long long)P, C);
  return check_elem_size(who, elem_size);
}

}  // namespace

extern "C" {

#if NASSEG_FP32_ONLY
int64_t nasseg_lovasz_workspace(int64_t P, int C) {
  if (P < 1 || C < 2 || C > 65535 || P * (int64_t)C >= ((int64_t)1 << 31)) return 0;
  return lov_ws(nullptr, P, C).words;
}

int nasseg_lovasz_coef(const float* errors, const void* target, int elem_size, int64_t P, int C, int ignore,
                       int all_classes, float* loss, float* coef, int* rank, int64_t* ncls, float* ws, void* stream) {
  NASSEG_TRY(lov_check("lovasz_coef", P, C, elem_size));
  NASSEG_REQUIRE(errors && target && loss && coef && ncls && ws, "lovasz_coef: null pointer");
  NASSEG_REQUIRE(((uintptr_t)ws & 7) == 0, "lovasz_coef: the workspace must be 8-byte aligned");
  return lov_launch(errors, target, elem_size, P, C, ignore, all_classes != 0, 1.0, nullptr, loss, nullptr,
                               coef, rank, ncls, ws, (hipStream_t)stream);
}
#endif

int NASSEG_FN(lovasz_fwd)(const act_t* logits, const void* target, int elem_size, int64_t P, int C, int ignore,
                          int all_classes, double lovasz_weight, const float* base_loss, float* loss,
                          float* loss_lovasz, float* errors, float* coef, int* rank, int64_t* ncls, float* ws,
                          void* stream) {
  NASSEG_TRY(lov_check("lovasz_fwd", P, C, elem_size));
  NASSEG_REQUIRE(logits && target && loss && errors && coef && ncls && ws, "lovasz_fwd: null pointer");
  NASSEG_REQUIRE(((uintptr_t)ws & 7) == 0, "lovasz_fwd: the workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)cdiv64(P, 256);
  const size_t lds = (size_t)256 * (C | 1) * sizeof(float);
  with_labels(target, elem_size, [&](auto labels) {
    using TL = label_of<decltype(labels)>;
    if (C <= 63)
      hipLaunchKernelGGL(lov_err_tile_kernel<TL>, dim3(grid), dim3(256), lds, s, logits, labels, P, C, ignore, errors);
    else
      hipLaunchKernelGGL(lov_err_kernel<TL>, dim3(grid), dim3(256), 0, s, logits, labels, P, C, ignore, errors);
  });
  NASSEG_LAUNCH_CHECK("lovasz_errors");
  return lov_launch(errors, target, elem_size, P, C, ignore, all_classes != 0, lovasz_weight, base_loss,
                               loss, loss_lovasz, coef, rank, ncls, ws, s);
}

int NASSEG_FN(lovasz_bwd)(const act_t* logits, const void* target, int elem_size, const float* coef,
                          const float* gscale, double lovasz_weight, int accumulate, int64_t P, int C, int ignore,
                          act_t* dlogits, void* stream) {
  NASSEG_TRY(lov_check("lovasz_bwd", P, C, elem_size));
  NASSEG_REQUIRE(logits && target && coef && dlogits, "lovasz_bwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)cdiv64(P, 256);
  const float lw = (float)lovasz_weight;
  const size_t lds = (size_t)2 * 256 * (C | 1) * sizeof(float);
  with_labels(target, elem_size, [&](auto labels) {
    using TL = label_of<decltype(labels)>;
    if (C <= 31)
      hipLaunchKernelGGL(lov_bwd_tile_kernel<TL>, dim3(grid), dim3(256), lds, s, logits, labels, coef, gscale, lw,
                         accumulate, P, C, ignore, dlogits);
    else
      hipLaunchKernelGGL(lov_bwd_kernel<TL>, dim3(grid), dim3(256), 0, s, logits, labels, coef, gscale, lw, accumulate,
                         P, C, ignore, dlogits);
  });
  NASSEG_LAUNCH_CHECK("lovasz_bwd");
  return NASSEG_OK;
}

}  // extern "C"
