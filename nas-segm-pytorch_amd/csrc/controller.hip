// The search controller on the device: the stacked-LSTM policy of src/rl/micro_controllers.py (MicroController
// :148-265, TemplateController :442-571), its backward through time and the PPO surrogate of
// src/rl/gradient_estimators.py:147-198.
//
// In both controllers the LSTM's next input is its own previous output (`inputs = output`; enc_op is never
// used), so the distribution of every step is independent of the sampled actions: evaluating B action rows is ONE
// T-step rollout plus B*T gathers, sampling n candidates is one rollout plus n*T inverse-CDF look-ups.
//
// The controller is described by a step table int32 [T][3] = {head (-1: a warm-up step without a head), choices,
// position of the step's action in an action row (-1: none)} and a table of parameter addresses in torch's own
// layouts: [0] g_emb, [1 + 4k ..] weight_ih_l{k} (4H, H), weight_hh_l{k} (4H, H), bias_ih_l{k}, bias_hh_l{k} (gate
// order i, f, g, o), [1 + 4L + 2j ..] head j's weight (n_j, H) and bias.  Nothing is re-packed.
//
// The dependent chain (T steps x L layers) runs in ONE workgroup of 1024 threads: 4H gate rows of 2H columns per
// layer do not fit the LDS at H = 100 and are streamed from L2 every step, a wave per row (coalesced), rows four at a
// time.  There is no grid-wide barrier, no cooperative launch and no float atomic in this file; every sum has a fixed
// order, so results repeat bit for bit, host-launched or replayed from a hipGraph.
#include "common.h"

#if NASSEG_FP32_ONLY

#define CT_THREADS 1024
#define CT_WAVES 16
#define CT_MAX_H 256
#define CT_MAX_L 4
#define CT_MAX_T 128
#define CT_MAX_N 64
#define CT_MAX_B 1024
#define CT_MAX_HEADS 64

struct CtrlDims {
  int T, H, L, NH, A, maxn;
};

// saved by the rollout for the backward (floats): activated gates [T][L][4H], cell states [T][L][H], layer outputs
// [T][L][H], per step [T][64] each: probabilities, log-probabilities and the logits centred on their mean under p
// (l_i - sum_j p_j l_j = log p_i + H_t without the cancellation of two numbers of size log n: the entropy's gradient)
static inline __host__ __device__ int64_t ct_off_cs(int T, int H, int L) { return (int64_t)T * L * 4 * H; }
static inline __host__ __device__ int64_t ct_off_hs(int T, int H, int L) { return ct_off_cs(T, H, L) + (int64_t)T * L * H; }
static inline __host__ __device__ int64_t ct_off_p(int T, int H, int L) { return ct_off_hs(T, H, L) + (int64_t)T * L * H; }
static inline __host__ __device__ int64_t ct_off_lp(int T, int H, int L) { return ct_off_p(T, H, L) + (int64_t)T * CT_MAX_N; }
static inline __host__ __device__ int64_t ct_off_cen(int T, int H, int L) { return ct_off_lp(T, H, L) + (int64_t)T * CT_MAX_N; }
static inline __host__ __device__ int64_t ct_saved(int T, int H, int L) { return ct_off_cen(T, H, L) + (int64_t)T * CT_MAX_N; }
// backward workspace (floats): gate gradients [T][L][4H], logit gradients [T][64]
static inline __host__ __device__ int64_t ct_off_dlog(int T, int H, int L) { return (int64_t)T * L * 4 * H; }
static inline __host__ __device__ int64_t ct_work(int T, int H, int L) { return ct_off_dlog(T, H, L) + (int64_t)T * CT_MAX_N; }

__device__ __forceinline__ const float* ct_param(const int64_t* params, int i) {
  return reinterpret_cast<const float*>(static_cast<uintptr_t>(params[i]));
}

struct CtrlStep {
  int head, n, pos;
};
// a step as the kernels use it: whatever the table holds, head < NH, 1 <= n <= maxn <= 64 and pos < A, so no index
// derived from it leaves a buffer
__device__ __forceinline__ CtrlStep ct_step(const int* __restrict__ steps, int t, const CtrlDims& d) {
  CtrlStep s;
  s.head = steps[3 * t];
  s.n = steps[3 * t + 1];
  s.pos = steps[3 * t + 2];
  if (s.head < 0 || s.head >= d.NH || s.n < 1) {
    s.head = -1;
    s.n = 0;
  }
  s.n = min(s.n, d.maxn);
  if (s.pos < 0 || s.pos >= d.A || s.head < 0) s.pos = -1;
  return s;
}
__device__ __forceinline__ int ct_action(const int* __restrict__ actions, const int* __restrict__ rows, int n_rows,
                                         int b, int A, int pos, int n) {
  int row = rows ? rows[b] : b;
  row = min(max(row, 0), n_rows - 1);
  return min(max(actions[(int64_t)row * A + pos], 0), n - 1);
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float ct_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// ---------------------------------------------------------------------------------------------------------------------
// rollout: grid 1 x 1024 threads
// ---------------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(CT_THREADS) void ctrl_rollout_kernel(
    const int64_t* __restrict__ params, const int* __restrict__ steps, CtrlDims d, const int* __restrict__ actions,
    const int* __restrict__ rows, int n_rows, int B, const float* __restrict__ u, int ns, int* __restrict__ sampled,
    float* __restrict__ sampled_lp, float* __restrict__ saved, float* __restrict__ entropy,
    float* __restrict__ log_prob) {
  __shared__ float s_x[CT_MAX_H];
  __shared__ float s_h[CT_MAX_L][CT_MAX_H];
  __shared__ float s_c[CT_MAX_L][CT_MAX_H];
  __shared__ float s_g[4 * CT_MAX_H];
  __shared__ float s_logit[CT_MAX_N];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = d.T, H = d.H, L = d.L, H4 = 4 * d.H;
  float* gates = saved;
  float* cs = saved + ct_off_cs(T, H, L);
  float* hs = saved + ct_off_hs(T, H, L);
  float* probs = saved + ct_off_p(T, H, L);
  float* logps = saved + ct_off_lp(T, H, L);
  float* cent = saved + ct_off_cen(T, H, L);

  if (tid < H) {
    s_x[tid] = ct_param(params, 0)[tid];
    for (int k = 0; k < L; ++k) {
      s_h[k][tid] = 0.f;
      s_c[k][tid] = 0.f;
    }
  }
  float ent_total = 0.f;  // (wave 0)
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    for (int k = 0; k < L; ++k) {
      // layer 0 reads the top layer's output of the step before (g_emb at t = 0), layer k > 0 layer k-1's of this step
      const float* in = k > 0 ? s_h[k - 1] : (t == 0 ? s_x : s_h[L - 1]);
      const float* wih = ct_param(params, 1 + 4 * k);
      const float* whh = ct_param(params, 2 + 4 * k);
      const float* bih = ct_param(params, 3 + 4 * k);
      const float* bhh = ct_param(params, 4 + 4 * k);
      float xr[4], hr[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int c = lane + 64 * m;
        xr[m] = c < H ? in[c] : 0.f;
        hr[m] = c < H ? s_h[k][c] : 0.f;
      }
      for (int r0 = wave; r0 < H4; r0 += 4 * CT_WAVES) {
        float acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[j] = 0.f;
          const int r = r0 + CT_WAVES * j;
          if (r < H4) {
            const float* wi = wih + (int64_t)r * H;
            const float* wh = whh + (int64_t)r * H;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
              const int c = lane + 64 * m;
              if (c < H) acc[j] = fmaf(wh[c], hr[m], fmaf(wi[c], xr[m], acc[j]));
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = r0 + CT_WAVES * j;
          const float v = wave_sum(acc[j]);
          if (lane == 0 && r < H4) s_g[r] = v + bih[r] + bhh[r];
        }
      }
      __syncthreads();
      if (tid < H) {
        const float gi = ct_sigmoid(s_g[tid]);
        const float gf = ct_sigmoid(s_g[H + tid]);
        const float gg = tanhf(s_g[2 * H + tid]);
        const float go = ct_sigmoid(s_g[3 * H + tid]);
        const float c = fmaf(gf, s_c[k][tid], gi * gg);
        const float h = go * tanhf(c);
        float* gsave = gates + ((int64_t)t * L + k) * H4;
        gsave[tid] = gi;
        gsave[H + tid] = gf;
        gsave[2 * H + tid] = gg;
        gsave[3 * H + tid] = go;
        cs[((int64_t)t * L + k) * H + tid] = c;
        hs[((int64_t)t * L + k) * H + tid] = h;
        s_c[k][tid] = c;
        s_h[k][tid] = h;
      }
      __syncthreads();
    }
    const CtrlStep st = ct_step(steps, t, d);
    if (st.head >= 0) {
      const float* hw = ct_param(params, 1 + 4 * L + 2 * st.head);
      const float* hb = ct_param(params, 2 + 4 * L + 2 * st.head);
      for (int i = wave; i < st.n; i += CT_WAVES) {
        float acc = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int c = lane + 64 * m;
          if (c < H) acc = fmaf(hw[(int64_t)i * H + c], s_h[L - 1][c], acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) s_logit[i] = acc + hb[i];
      }
    }
    __syncthreads();
    if (wave == 0) {
      float p = 0.f, lp = 0.f, ent = 0.f, cen = 0.f;
      if (st.head >= 0) {
        const bool on = lane < st.n;
        const float l = on ? s_logit[lane] : -__builtin_inff();
        const float mx = wave_max(l);
        const float e = on ? expf(l - mx) : 0.f;
        const float sum = wave_sum(e);
        lp = on ? (l - mx) - logf(sum) : 0.f;
        p = on ? e / sum : 0.f;
        ent = -wave_sum(p * lp);
        const float lm = on ? l - mx : 0.f;
        const float mean = wave_sum(p * lm);
        cen = on ? lm - mean : 0.f;
      }
      probs[(int64_t)t * CT_MAX_N + lane] = p;
      logps[(int64_t)t * CT_MAX_N + lane] = lp;
      cent[(int64_t)t * CT_MAX_N + lane] = cen;
      ent_total += ent;
    }
    // (s_logit is next written after the 2L barriers of step t+1; s_h[L-1] after at least one)
  }
  if (tid == 0) *entropy = ent_total;
  __threadfence_block();
  __syncthreads();

  // log-probabilities of the given action rows: steps in ascending order
  for (int b = tid; b < B; b += CT_THREADS) {
    float lp = 0.f;
    for (int t = 0; t < T; ++t) {
      const CtrlStep st = ct_step(steps, t, d);
      if (st.pos < 0) continue;
      lp += logps[(int64_t)t * CT_MAX_N + ct_action(actions, rows, n_rows, b, d.A, st.pos, st.n)];
    }
    log_prob[b] = lp;
  }
  // sampling by inverse CDF: the CDF accumulated in ascending index order, the first index with u < cdf, the last
  // index catches the rest
  for (int s = tid; s < ns; s += CT_THREADS) {
    float lp = 0.f;
    for (int a = 0; a < d.A; ++a) sampled[(int64_t)s * d.A + a] = 0;  // (positions without a step: CVPR's dummy)
    for (int t = 0; t < T; ++t) {
      const CtrlStep st = ct_step(steps, t, d);
      if (st.pos < 0) continue;
      const float uu = u[(int64_t)s * T + t];
      float cdf = 0.f;
      int idx = st.n - 1;
      for (int i = 0; i < st.n; ++i) {
        cdf += probs[(int64_t)t * CT_MAX_N + i];
        if (uu < cdf) {
          idx = i;
          break;
        }
      }
      sampled[(int64_t)s * d.A + st.pos] = idx;
      lp += logps[(int64_t)t * CT_MAX_N + idx];
    }
    sampled_lp[s] = lp;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward through time: grid 1 x 1024 threads.  Writes the gate gradients [T][L][4H] and the logit gradients [T][64]
// for the parameter-gradient launch, and g_emb's gradient.
// ---------------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(CT_THREADS) void ctrl_bptt_kernel(
    const int64_t* __restrict__ params, const int* __restrict__ steps, CtrlDims d, const int* __restrict__ actions,
    const int* __restrict__ rows, int n_rows, int B, const float* __restrict__ d_lp, const float* __restrict__ d_ent,
    const float* __restrict__ saved, float* __restrict__ work, const int* __restrict__ gtab,
    float* __restrict__ grads) {
  __shared__ float s_dhrec[CT_MAX_L][CT_MAX_H];
  __shared__ float s_dcrec[CT_MAX_L][CT_MAX_H];
  __shared__ float s_dg[4 * CT_MAX_H];
  __shared__ float s_dx[CT_MAX_H];  // layer 0's input gradient of the step after: part of this step's top gradient
  __shared__ float s_up[CT_MAX_H];  // the gradient arriving at a layer's output from above
  __shared__ float s_part[2][CT_WAVES][CT_MAX_H];
  const int tid = threadIdx.x;
  const int T = d.T, H = d.H, L = d.L, H4 = 4 * d.H;
  const float* gates = saved;
  const float* cs = saved + ct_off_cs(T, H, L);
  const float* probs = saved + ct_off_p(T, H, L);
  const float* cent = saved + ct_off_cen(T, H, L);
  float* dgates = work;
  float* dlog = work + ct_off_dlog(T, H, L);

  // dlogits[t][i] = sum_b d_lp[b] (onehot(a[b,t]) - p) + d_ent (-p (logp + H_t)); b ascending; logp + H_t is the
  // centred logit the rollout saved
  const float de = d_ent ? *d_ent : 0.f;
  for (int item = tid; item < T * CT_MAX_N; item += CT_THREADS) {
    const int t = item / CT_MAX_N, i = item % CT_MAX_N;
    const CtrlStep st = ct_step(steps, t, d);
    float v = 0.f;
    if (st.head >= 0 && i < st.n) {
      float hit = 0.f, tot = 0.f;
      if (st.pos >= 0 && d_lp) {
        for (int b = 0; b < B; ++b) {
          const float g = d_lp[b];
          tot += g;
          if (ct_action(actions, rows, n_rows, b, d.A, st.pos, st.n) == i) hit += g;
        }
      }
      const float p = probs[item];
      v = (hit - p * tot) + de * (-p * cent[item]);
    }
    dlog[item] = v;
  }
  if (tid < H) {
    for (int k = 0; k < L; ++k) {
      s_dhrec[k][tid] = 0.f;
      s_dcrec[k][tid] = 0.f;
    }
    s_dx[tid] = 0.f;
  }
  __threadfence_block();
  __syncthreads();

  // the column sums W^T dgates: HP columns x G row groups, group g adds rows g, g + G, ...; the groups are then
  // added in ascending order
  const int HP = (H + 63) & ~63;
  const int G = CT_THREADS / HP;
  const int grp = tid / HP, col = tid % HP;

  for (int t = T - 1; t >= 0; --t) {
    const CtrlStep st = ct_step(steps, t, d);
    if (tid < H) {
      float acc = s_dx[tid];
      if (st.head >= 0) {
        const float* hw = ct_param(params, 1 + 4 * L + 2 * st.head);
        for (int i = 0; i < st.n; ++i) acc = fmaf(hw[(int64_t)i * H + tid], dlog[(int64_t)t * CT_MAX_N + i], acc);
      }
      s_up[tid] = acc;
    }
    __syncthreads();
    for (int k = L - 1; k >= 0; --k) {
      if (tid < H) {
        const float* gs = gates + ((int64_t)t * L + k) * H4;
        const float gi = gs[tid], gf = gs[H + tid], gg = gs[2 * H + tid], go = gs[3 * H + tid];
        const float c = cs[((int64_t)t * L + k) * H + tid];
        const float cprev = t > 0 ? cs[((int64_t)(t - 1) * L + k) * H + tid] : 0.f;
        const float tc = tanhf(c);
        const float dh = s_dhrec[k][tid] + s_up[tid];
        const float dc = s_dcrec[k][tid] + dh * go * (1.f - tc * tc);
        s_dcrec[k][tid] = dc * gf;
        const float dgi = dc * gg * gi * (1.f - gi);
        const float dgf = dc * cprev * gf * (1.f - gf);
        const float dgg = dc * gi * (1.f - gg * gg);
        const float dgo = dh * tc * go * (1.f - go);
        float* dgs = dgates + ((int64_t)t * L + k) * H4;
        s_dg[tid] = dgs[tid] = dgi;
        s_dg[H + tid] = dgs[H + tid] = dgf;
        s_dg[2 * H + tid] = dgs[2 * H + tid] = dgg;
        s_dg[3 * H + tid] = dgs[3 * H + tid] = dgo;
      }
      __syncthreads();
      if (grp < G && col < H) {
        const float* wih = ct_param(params, 1 + 4 * k);
        const float* whh = ct_param(params, 2 + 4 * k);
        float a0 = 0.f, a1 = 0.f;
#pragma unroll 4
        for (int r = grp; r < H4; r += G) {
          const float g = s_dg[r];
          a0 = fmaf(wih[(int64_t)r * H + col], g, a0);
          a1 = fmaf(whh[(int64_t)r * H + col], g, a1);
        }
        s_part[0][grp][col] = a0;
        s_part[1][grp][col] = a1;
      }
      __syncthreads();
      if (tid < H) {
        float dx = 0.f, dh = 0.f;
        for (int g = 0; g < G; ++g) {
          dx += s_part[0][g][tid];
          dh += s_part[1][g][tid];
        }
        s_dhrec[k][tid] = dh;
        if (k == 0)
          s_dx[tid] = dx;
        else
          s_up[tid] = dx;
      }
      __syncthreads();
    }
  }
  if (tid < H) grads[gtab[0] + tid] = s_dx[tid];  // g_emb: layer 0's input gradient at t = 0
}

// ---------------------------------------------------------------------------------------------------------------------
// parameter gradients: one thread per element, t ascending; blockIdx.y + 1 = entry of the parameter table.
// gtab int32 [1 + 4L + 2NH][2] = {offset of the entry's gradient in `grads`, rows}
// ---------------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void ctrl_wgrad_kernel(const int64_t* __restrict__ params,
                                                         const int* __restrict__ steps, CtrlDims d,
                                                         const float* __restrict__ saved,
                                                         const float* __restrict__ work,
                                                         const int* __restrict__ gtab, float* __restrict__ grads) {
  const int T = d.T, H = d.H, L = d.L, H4 = 4 * d.H;
  const int e = blockIdx.y + 1;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const float* hs = saved + ct_off_hs(T, H, L);
  const float* dgates = work;
  const float* dlog = work + ct_off_dlog(T, H, L);
  float* out = grads + gtab[2 * e];
  float acc = 0.f;
  if (e <= 4 * L) {
    const int k = (e - 1) / 4, kind = (e - 1) % 4;
    if (kind < 2) {
      if (idx >= H4 * H) return;
      const int r = idx / H, c = idx % H;
      for (int t = kind; t < T; ++t) {
        float x;
        if (kind == 1)
          x = hs[((int64_t)(t - 1) * L + k) * H + c];
        else if (k > 0)
          x = hs[((int64_t)t * L + k - 1) * H + c];
        else
          x = t == 0 ? ct_param(params, 0)[c] : hs[((int64_t)(t - 1) * L + L - 1) * H + c];
        acc = fmaf(dgates[((int64_t)t * L + k) * H4 + r], x, acc);
      }
    } else {  // bias_ih and bias_hh: the same sum
      if (idx >= H4) return;
      for (int t = 0; t < T; ++t) acc += dgates[((int64_t)t * L + k) * H4 + idx];
    }
  } else {
    const int j = (e - 1 - 4 * L) / 2, is_bias = (e - 1 - 4 * L) % 2;
    const int n = min(max(gtab[2 * e + 1], 0), d.maxn);
    if (idx >= (is_bias ? n : n * H)) return;
    const int i = is_bias ? idx : idx / H, c = is_bias ? 0 : idx % H;
    for (int t = 0; t < T; ++t) {
      const CtrlStep st = ct_step(steps, t, d);
      if (st.head != j || i >= st.n) continue;
      const float g = dlog[(int64_t)t * CT_MAX_N + i];
      acc = is_bias ? acc + g : fmaf(g, hs[((int64_t)t * L + L - 1) * H + c], acc);
    }
  }
  out[idx] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// PPO seed (src/rl/gradient_estimators.py:170-187): grid 1 x 1024 threads.  The reference subtracts a (B, 1) array of
// old log-probabilities from the (B,) new ones, so ratio, both surrogates and the mean run over B x B pairs
// (i: old / advantage row, j: new log-probability); B = 1, the search's setting, is the usual formula.
// ---------------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(CT_THREADS) void ctrl_ppo_seed_kernel(const float* __restrict__ lp,
                                                                   const float* __restrict__ entropy,
                                                                   const float* __restrict__ old_lp,
                                                                   const float* __restrict__ adv,
                                                                   const int* __restrict__ rows, int n_rows, int B,
                                                                   float lo, float hi, float ent_coef,
                                                                   float* __restrict__ acc, float* __restrict__ d_lp,
                                                                   float* __restrict__ d_ent) {
  __shared__ float s_sum[CT_THREADS];
  const int j = threadIdx.x;
  float part = 0.f, dj = 0.f;
  if (j < B) {
    const float l = lp[j];
    for (int i = 0; i < B; ++i) {
      int row = rows ? rows[i] : i;
      row = min(max(row, 0), n_rows - 1);
      const float a = adv[row];
      const float r = expf(l - old_lp[row]);
      const float rc = fminf(fmaxf(r, lo), hi);
      const float s1 = r * a, s2 = rc * a;
      part += fminf(s1, s2);
      // torch's minimum: the smaller operand takes the gradient, a tie splits it; clamp passes it on [lo, hi]
      const float w1 = s1 < s2 ? 1.f : (s1 == s2 ? 0.5f : 0.f);
      const float w2 = s2 < s1 ? 1.f : (s1 == s2 ? 0.5f : 0.f);
      const float inside = (r >= lo && r <= hi) ? 1.f : 0.f;
      dj += (w1 * a + w2 * a * inside) * r;
    }
    const float inv = 1.f / ((float)B * (float)B);
    d_lp[j] = -dj * inv;
  }
  s_sum[j] = part;
  __syncthreads();
  for (int off = CT_THREADS / 2; off > 0; off >>= 1) {
    if (j < off) s_sum[j] += s_sum[j + off];
    __syncthreads();
  }
  if (j == 0) {
    acc[0] += -s_sum[0] / ((float)B * (float)B);
    acc[1] += *entropy;
    *d_ent = -ent_coef;
  }
}

static int ct_check(const char* who, const void* params, const void* steps, int T, int H, int L, int n_heads,
                    int max_choices, int B, int n_rows, int A) {
  NASSEG_REQUIRE(params && steps, "%s: null parameter or step table", who);
  NASSEG_REQUIRE(H >= 1 && H <= CT_MAX_H, "%s: hidden size %d (1..%d)", who, H, CT_MAX_H);
  NASSEG_REQUIRE(L >= 1 && L <= CT_MAX_L, "%s: %d LSTM layers (1..%d)", who, L, CT_MAX_L);
  NASSEG_REQUIRE(T >= 1 && T <= CT_MAX_T, "%s: %d steps (1..%d)", who, T, CT_MAX_T);
  NASSEG_REQUIRE(n_heads >= 1 && n_heads <= CT_MAX_HEADS, "%s: %d heads (1..%d)", who, n_heads, CT_MAX_HEADS);
  NASSEG_REQUIRE(max_choices >= 1 && max_choices <= CT_MAX_N, "%s: %d choices per head (1..%d)", who, max_choices,
                 CT_MAX_N);
  NASSEG_REQUIRE(B >= 0 && B <= CT_MAX_B, "%s: %d action rows (0..%d)", who, B, CT_MAX_B);
  NASSEG_REQUIRE(A >= 1 && (B == 0 || n_rows >= 1), "%s: action rows of %d entries, %d rows", who, A, n_rows);
  return NASSEG_OK;
}

extern "C" {

int64_t nasseg_ctrl_saved_floats(int T, int H, int L) {
  if (T < 1 || H < 1 || L < 1) return 0;
  return ct_saved(T, H, L);
}

int64_t nasseg_ctrl_work_floats(int T, int H, int L) {
  if (T < 1 || H < 1 || L < 1) return 0;
  return ct_work(T, H, L);
}

int nasseg_ctrl_rollout(const int64_t* params, const int* steps, int T, int H, int L, int n_heads, int max_choices,
                        const int* actions, const int* rows, int n_rows, int B, int A, const float* u, int n_samples,
                        int* sampled, float* sampled_lp, float* saved, float* entropy, float* log_prob,
                        void* stream) {
  const int rc = ct_check("ctrl_rollout", params, steps, T, H, L, n_heads, max_choices, B, n_rows, A);
  if (rc != NASSEG_OK) return rc;
  NASSEG_REQUIRE(saved && entropy, "ctrl_rollout: null output");
  NASSEG_REQUIRE(B == 0 || (actions && log_prob), "ctrl_rollout: %d action rows without actions / log_prob", B);
  NASSEG_REQUIRE(n_samples >= 0 && n_samples <= CT_MAX_B, "ctrl_rollout: %d samples (0..%d)", n_samples, CT_MAX_B);
  NASSEG_REQUIRE(n_samples == 0 || (u && sampled && sampled_lp), "ctrl_rollout: %d samples without u / outputs",
                 n_samples);
  const CtrlDims d = {T, H, L, n_heads, A, max_choices};
  hipLaunchKernelGGL(ctrl_rollout_kernel, dim3(1), dim3(CT_THREADS), 0, (hipStream_t)stream, params, steps, d,
                     actions, rows, n_rows, B, u, n_samples, sampled, sampled_lp, saved, entropy, log_prob);
  NASSEG_LAUNCH_CHECK("ctrl_rollout");
  return NASSEG_OK;
}

int nasseg_ctrl_backward(const int64_t* params, const int* steps, int T, int H, int L, int n_heads, int max_choices,
                         const int* actions, const int* rows, int n_rows, int B, int A, const float* d_log_prob,
                         const float* d_entropy, const float* saved, float* work, const int* gtab, float* grads,
                         void* stream) {
  const int rc = ct_check("ctrl_backward", params, steps, T, H, L, n_heads, max_choices, B, n_rows, A);
  if (rc != NASSEG_OK) return rc;
  NASSEG_REQUIRE(saved && work && gtab && grads, "ctrl_backward: null buffer");
  NASSEG_REQUIRE(B == 0 || !d_log_prob || actions, "ctrl_backward: %d action rows without actions", B);
  const CtrlDims d = {T, H, L, n_heads, A, max_choices};
  hipLaunchKernelGGL(ctrl_bptt_kernel, dim3(1), dim3(CT_THREADS), 0, (hipStream_t)stream, params, steps, d, actions,
                     rows, n_rows, B, d_log_prob, d_entropy, saved, work, gtab, grads);
  NASSEG_LAUNCH_CHECK("ctrl_backward (chain)");
  // (the widest entry: an LSTM weight, 4H x H, or - small H, many choices - a head's weight, up to max_choices x H)
  const int widest = 4 * H * H > max_choices * H ? 4 * H * H : max_choices * H;
  hipLaunchKernelGGL(ctrl_wgrad_kernel, dim3(cdiv(widest, 256), 4 * L + 2 * n_heads), dim3(256), 0,
                     (hipStream_t)stream, params, steps, d, saved, (const float*)work, gtab, grads);
  NASSEG_LAUNCH_CHECK("ctrl_backward (parameters)");
  return NASSEG_OK;
}

int nasseg_ctrl_ppo_seed(const float* log_prob, const float* entropy, const float* old_log_prob, const float* adv,
                         const int* rows, int n_rows, int B, float clip_lo, float clip_hi, float entropy_coef,
                         float* acc, float* d_log_prob, float* d_entropy, void* stream) {
  NASSEG_REQUIRE(log_prob && entropy && old_log_prob && adv && acc && d_log_prob && d_entropy,
                 "ctrl_ppo_seed: null buffer");
  NASSEG_REQUIRE(B >= 1 && B <= CT_MAX_B && n_rows >= 1, "ctrl_ppo_seed: %d action rows (1..%d) of %d", B, CT_MAX_B,
                 n_rows);
  NASSEG_REQUIRE(clip_lo <= clip_hi, "ctrl_ppo_seed: clip range [%g, %g]", (double)clip_lo, (double)clip_hi);
  hipLaunchKernelGGL(ctrl_ppo_seed_kernel, dim3(1), dim3(CT_THREADS), 0, (hipStream_t)stream, log_prob, entropy,
                     old_log_prob, adv, rows, n_rows, B, clip_lo, clip_hi, entropy_coef, acc, d_log_prob, d_entropy);
  NASSEG_LAUNCH_CHECK("ctrl_ppo_seed");
  return NASSEG_OK;
}

}  // extern "C"

#endif  // NASSEG_FP32_ONLY
