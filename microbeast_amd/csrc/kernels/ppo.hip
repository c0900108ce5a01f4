// PPO objective (Schulman et al. 2017): GAE(lambda) advantages + the clipped surrogate and
// clipped value losses with their gradients, beside the V-trace path (vtrace.hip).
//
// Reference: libs/utils.py:104-163 (get_deltas / get_advantages: dead code there) and the name
// of its learn step (PPO_learn, which is V-trace). Two launchers, called once per rollout and
// once per epoch:
//
//   mbk_gae       v_old [T+1,B], reward, done [T,B] -> adv, ret [T,B], stats[2]
//     delta_t = r_t + gamma nd_t v_old[t+1] - v_old[t],  A_t = delta_t + gamma lambda nd_t A_{t+1}
//     (A_T = 0),  R_t = A_t + v_old[t];  stats = (mean A, 1 / (std A + 1e-8)) over the T*B
//     elements (population std), or (0, 1) with normalisation off.
//   mbk_vtrace_adv  mbk_gae for rollouts acted by an older policy mu (--ppo_adv vtrace):
//     + logp_pi, logp_mu [T,B] -> adv, ret, stats as above, is_stats[3]
//     w = exp(logp_pi - logp_mu), rho = min(rho_bar, w), c = lambda min(c_bar, w)
//     adv_t = delta_t + gamma nd_t lambda d_{t+1},  d_t = rho_t delta_t + gamma nd_t c_t d_{t+1}
//     (d_T = 0),  ret_t = v_old[t] + d_t;  is_stats = mean w, share w > rho_bar, share w > c_bar.
//     w == 1 and both bars >= 1: mbk_gae's adv and ret.
//   mbk_ppo_loss  logp_new, logp_old, v, v_old, adv, ret, entropy, stats -> g_logp [T,B],
//     g_value [T+1,B] (row T = 0), losses[7]
//     A^ = (A - mean) rstd, ratio = exp(logp_new - logp_old), M = T*B
//     pg    = -mean(min(ratio A^, clamp(ratio, 1-eps, 1+eps) A^))
//     value = bc mean(max((v-R)^2, (v_c-R)^2)),  v_c = v_old + clamp(v - v_old, -eps_v, eps_v)
//             (eps_v = 0: the plain (v-R)^2)
//     dL/dlogp = -A^ ratio / M, or 0 where (A^ > 0, ratio > 1+eps) or (A^ < 0, ratio < 1-eps)
//     dL/dv    = 2 bc (v-R)/M where (v-R)^2 >= (v_c-R)^2; else 2 bc (v_c-R)/M where
//                |v - v_old| <= eps_v; else 0
//     dL/dH    = -entropy_cost / M (constant: the caller's seed)
//     losses   = pg, value, entropy, total, mean ratio, approx_kl = mean((ratio-1) - log ratio),
//                clip_frac = mean(|ratio-1| > eps)
//
// Row-block minibatches (K optimiser steps per epoch, step = Tm = T/K consecutive rows, all B):
//   mbk_adv_stats_rows  adv [T,B] -> stats [K][2]: each block's own (mean, 1 / (std + 1e-8))
//   mbk_ppo_loss_rows   the same element pass on the step's own [Tm,B] arrays (logp_new, values,
//     entropy, g_logp, g_value: no bootstrap row) and rows t0.. of the rollout-wide logp_old,
//     v_old, adv, ret; M = Tm*B. Its finalize also keeps the ordered running mean of the
//     epoch's per-step losses (epoch_mean[7]).
//
// Every reduction is two-pass and ordered (per-block partials, one finalize wave): no float
// atomics, bit-reproducible between runs. The advantage statistics merge per-block
// (n, mean, M2) triples (Chan et al.), not a global sum of squares.
//
// Each step exists once: push / block_merge / write_stats below serve the three kernels that
// keep moments and their finalizes, block_sums<K> (common.h) is the first pass of every plain
// sum (shared with vtrace.hip), ppo_finalize_kernel serves both loss launchers (epoch_mean
// null: none kept), and launch_ppo_loss holds the vector / scalar choice and both launches.
#include "../include/mbk_api.h"
#include "common.h"

using namespace mbk;

namespace {

// (n, mean, M2) of a set; merge of two disjoint sets (Chan, Golub, LeVeque 1979)
struct Moments {
  float n, mean, m2;
};
__device__ __forceinline__ Moments merge(Moments a, Moments b) {
  const float n = a.n + b.n;
  if (n == 0.f) return a;
  const float d = b.mean - a.mean, f = b.n / n;
  return {n, a.mean + d * f, a.m2 + b.m2 + d * d * a.n * f};
}
// lane 0 ends with the wave's merge, in a fixed order
__device__ __forceinline__ Moments wave_merge(Moments m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Moments r;
    r.n = __shfl_down(m.n, o, 64);
    r.mean = __shfl_down(m.mean, o, 64);
    r.m2 = __shfl_down(m.m2, o, 64);
    m = merge(m, r);
  }
  return m;
}
// Welford update of a lane's own running value
__device__ __forceinline__ void push(Moments& m, float x) {
  m.n += 1.f;
  const float d = x - m.mean;
  m.mean += d / m.n;
  m.m2 += d * (x - m.mean);
}
// A 256-lane block's merge -> its partial triple out[3]: wave_merge, LDS, thread 0 merges the
// waves in order. All lanes call it.
__device__ __forceinline__ void block_merge(Moments mo, float* __restrict__ out) {
  __shared__ Moments red[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  mo = wave_merge(mo);
  if (lane == 0) red[wave] = mo;
  __syncthreads();
  if (threadIdx.x == 0) {
    Moments s = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) s = merge(s, red[w]);
    out[0] = s.n;
    out[1] = s.mean;
    out[2] = s.m2;
  }
}
// stats[0..1] = mean, 1 / (std + 1e-8) (population std); (0, 1) with normalisation off
__device__ __forceinline__ void write_stats(Moments s, int norm, float* __restrict__ stats) {
  const float sd = sqrtf(fmaxf(s.m2, 0.f) / fmaxf(s.n, 1.f));
  stats[0] = norm ? s.mean : 0.f;
  stats[1] = norm ? 1.f / (sd + 1e-8f) : 1.f;
}

__global__ __launch_bounds__(256) void gae_kernel(
    const float* __restrict__ v_old, const float* __restrict__ reward,
    const uint8_t* __restrict__ done, int T, int B, float gamma, float lambda, float reward_clip,
    float* __restrict__ adv_out, float* __restrict__ ret_out,
    float* __restrict__ partials /* [gridDim.x][3] */) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  Moments mo = {0.f, 0.f, 0.f};
  if (b < B) {
    float v_next = v_old[(size_t)T * B + b];
    float acc = 0.f;
    for (int t = T - 1; t >= 0; --t) {
      const size_t i = (size_t)t * B + b;
      float r = reward[i];
      if (reward_clip > 0.f) r = fmaxf(-reward_clip, fminf(reward_clip, r));
      const float disc = done[i] ? 0.f : gamma;
      const float v = v_old[i];
      const float delta = r + disc * v_next - v;
      acc = delta + disc * lambda * acc;
      adv_out[i] = acc;
      ret_out[i] = acc + v;
      push(mo, acc);
      v_next = v;
    }
  }
  block_merge(mo, partials + blockIdx.x * 3);
}

__global__ __launch_bounds__(64) void gae_finalize_kernel(const float* __restrict__ partials,
                                                          int nblocks, int norm,
                                                          float* __restrict__ stats) {
  const int lane = threadIdx.x;
  Moments s = {0.f, 0.f, 0.f};
  for (int i = lane; i < nblocks; i += 64)
    s = merge(s, Moments{partials[i * 3], partials[i * 3 + 1], partials[i * 3 + 2]});
  s = wave_merge(s);
  if (lane == 0) write_stats(s, norm, stats);
}

// V-trace(lambda) advantages for lagged rollouts: gae_kernel with the importance weights
// w = exp(logp_pi - logp_mu) of the learner's first pass against the behaviour policy.
// d = vs - v is the carried value; with w == 1 and both bars >= 1 every step is gae_kernel's.
// partials [gridDim.x][kVtParts] = the block's (n, mean, M2) of adv, then its sums of w,
// (w > rho_bar) and (w > c_bar).
constexpr int kVtParts = 6;

__global__ __launch_bounds__(256) void vtrace_adv_kernel(
    const float* __restrict__ logp_pi, const float* __restrict__ logp_mu,
    const float* __restrict__ v_old, const float* __restrict__ reward,
    const uint8_t* __restrict__ done, int T, int B, float gamma, float lambda, float rho_bar,
    float c_bar, float reward_clip, float* __restrict__ adv_out, float* __restrict__ ret_out,
    float* __restrict__ partials) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  Moments mo = {0.f, 0.f, 0.f};
  float is[3] = {0.f, 0.f, 0.f};
  if (b < B) {
    float v_next = v_old[(size_t)T * B + b];
    float acc = 0.f;  // d_{t+1}
    for (int t = T - 1; t >= 0; --t) {
      const size_t i = (size_t)t * B + b;
      const float w = __expf(logp_pi[i] - logp_mu[i]);
      float r = reward[i];
      if (reward_clip > 0.f) r = fmaxf(-reward_clip, fminf(reward_clip, r));
      const float disc = done[i] ? 0.f : gamma;
      const float v = v_old[i];
      const float delta = r + disc * v_next - v;
      const float a = delta + disc * lambda * acc;
      acc = fminf(rho_bar, w) * delta + disc * (lambda * fminf(c_bar, w)) * acc;
      adv_out[i] = a;
      ret_out[i] = acc + v;
      push(mo, a);
      is[0] += w;
      is[1] += w > rho_bar ? 1.f : 0.f;
      is[2] += w > c_bar ? 1.f : 0.f;
      v_next = v;
    }
  }
  float* out = partials + (size_t)blockIdx.x * kVtParts;
  block_merge(mo, out);
  block_sums<3>(is, out + 3);
}

// gae_finalize_kernel's stats, and is_stats[0..2] = mean w, share of w > rho_bar, share of
// w > c_bar over the M = T*B elements
__global__ __launch_bounds__(64) void vtrace_adv_finalize_kernel(
    const float* __restrict__ partials, int nblocks, int norm, float invM,
    float* __restrict__ stats, float* __restrict__ is_stats) {
  const int lane = threadIdx.x;
  Moments s = {0.f, 0.f, 0.f};
  float t[3] = {0.f, 0.f, 0.f};
  for (int i = lane; i < nblocks; i += 64) {
    const float* p = partials + (size_t)i * kVtParts;
    s = merge(s, Moments{p[0], p[1], p[2]});
    for (int k = 0; k < 3; ++k) t[k] += p[3 + k];
  }
  s = wave_merge(s);
  for (int k = 0; k < 3; ++k) t[k] = wave_sum(t[k]);
  if (lane == 0) {
    write_stats(s, norm, stats);
    for (int k = 0; k < 3; ++k) is_stats[k] = t[k] * invM;
  }
}

constexpr int kSums = 6;  // surrogate, value, entropy, ratio, kl, clipped count

struct PpoParams {
  float mean, rstd, lo, hi, clip, vclip, bc2_invM, invM;
};

// one element: gradients out, sums accumulated
__device__ __forceinline__ void ppo_element(float lpn, float lpo, float v, float vo, float adv,
                                            float ret, float ent, const PpoParams& p,
                                            float& g_logp, float& g_value, float s[kSums]) {
  const float lr = lpn - lpo;
  const float ratio = __expf(lr);
  const float a = (adv - p.mean) * p.rstd;
  const float s1 = ratio * a;
  const float s2 = fminf(fmaxf(ratio, p.lo), p.hi) * a;
  const bool out = (a > 0.f && ratio > p.hi) || (a < 0.f && ratio < p.lo);
  g_logp = out ? 0.f : -s1 * p.invM;
  const float e = v - ret, e1 = e * e;
  float vterm = e1, gv = e;
  // inside the clip range v_c = v: the first case. Outside it v_c = v_old +- eps_v is constant
  // in v, so where its error is the larger one the gradient is 0
  const float d = v - vo;
  if (p.vclip > 0.f && fabsf(d) > p.vclip) {
    const float ec = vo + copysignf(p.vclip, d) - ret, e2 = ec * ec;
    if (e1 < e2) {
      vterm = e2;
      gv = 0.f;
    }
  }
  g_value = p.bc2_invM * gv;
  s[0] += fminf(s1, s2);
  s[1] += vterm;
  s[2] += ent;
  s[3] += ratio;
  s[4] += (ratio - 1.f) - lr;
  s[5] += fabsf(ratio - 1.f) > p.clip ? 1.f : 0.f;
}

// VEC = 4: 128-bit loads / stores (B % 4 == 0 and 16-byte aligned arrays); VEC = 1: scalar.
// Items [0, M / VEC) are the T*B elements; items up to (M + B) / VEC zero g_value's row T.
template <int VEC>
__global__ __launch_bounds__(256) void ppo_loss_kernel(
    const float* __restrict__ logp_new, const float* __restrict__ logp_old,
    const float* __restrict__ values, const float* __restrict__ v_old,
    const float* __restrict__ adv, const float* __restrict__ ret,
    const float* __restrict__ entropy, const float* __restrict__ stats, size_t M, size_t MB,
    float lo, float hi, float clip, float vclip, float baseline_cost,
    float* __restrict__ g_logp, float* __restrict__ g_value,
    float* __restrict__ partials /* [gridDim.x][kSums] */) {
  const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  float s[kSums] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (i < M) {
    PpoParams p;
    p.mean = stats[0];
    p.rstd = stats[1];
    p.lo = lo;
    p.hi = hi;
    p.clip = clip;
    p.vclip = vclip;
    p.invM = 1.f / (float)M;
    p.bc2_invM = 2.f * baseline_cost * p.invM;
    if constexpr (VEC == 4) {
      const float4 a = *(const float4*)(logp_new + i), b = *(const float4*)(logp_old + i);
      const float4 c = *(const float4*)(values + i), d = *(const float4*)(v_old + i);
      const float4 e = *(const float4*)(adv + i), f = *(const float4*)(ret + i);
      float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
      if (entropy) h = *(const float4*)(entropy + i);
      float4 gl, gv;
      ppo_element(a.x, b.x, c.x, d.x, e.x, f.x, h.x, p, gl.x, gv.x, s);
      ppo_element(a.y, b.y, c.y, d.y, e.y, f.y, h.y, p, gl.y, gv.y, s);
      ppo_element(a.z, b.z, c.z, d.z, e.z, f.z, h.z, p, gl.z, gv.z, s);
      ppo_element(a.w, b.w, c.w, d.w, e.w, f.w, h.w, p, gl.w, gv.w, s);
      *(float4*)(g_logp + i) = gl;
      *(float4*)(g_value + i) = gv;
    } else {
      float gl, gv;
      ppo_element(logp_new[i], logp_old[i], values[i], v_old[i], adv[i], ret[i],
                  entropy ? entropy[i] : 0.f, p, gl, gv, s);
      g_logp[i] = gl;
      g_value[i] = gv;
    }
  } else if (i < MB) {  // the bootstrap row has no gradient
    if constexpr (VEC == 4) {
      *(float4*)(g_value + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      g_value[i] = 0.f;
    }
  }
  block_sums<kSums>(s, partials + (size_t)blockIdx.x * kSums);
}

// losses[0..6] = pg, value, entropy, total, mean ratio, approx_kl, clip_frac. epoch_mean (null:
// none kept): the ordered running mean of the per-step losses of a row-block epoch so far
// (step 0 restarts it)
__global__ __launch_bounds__(64) void ppo_finalize_kernel(
    const float* __restrict__ partials, int nblocks, size_t M, float baseline_cost,
    float entropy_cost, int step, float* __restrict__ losses, float* __restrict__ epoch_mean) {
  const int lane = threadIdx.x;
  float s[kSums] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = lane; i < nblocks; i += 64)
    for (int k = 0; k < kSums; ++k) s[k] += partials[(size_t)i * kSums + k];
  for (int k = 0; k < kSums; ++k) s[k] = wave_sum(s[k]);
  if (lane == 0) {
    const float invM = 1.f / (float)M;
    const float pg = -s[0] * invM, vl = baseline_cost * s[1] * invM, ent = s[2] * invM;
    const float l[7] = {pg, vl, ent, pg + vl - entropy_cost * ent, s[3] * invM, s[4] * invM,
                        s[5] * invM};
    const float inv = 1.f / (float)(step + 1);
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      losses[k] = l[k];
      if (epoch_mean)
        epoch_mean[k] = step == 0 ? l[k] : epoch_mean[k] + (l[k] - epoch_mean[k]) * inv;
    }
  }
}

// ---- row-block minibatches: per-block advantage statistics ----

// Block k = rows [k Tm, (k+1) Tm) of adv: n = Tm*B contiguous elements. gridDim = (nb, K);
// thread j of the nb*256 of a block takes elements j, j + nb*256, ... (a fixed assignment, so
// the moments do not depend on the run). partials [K][nb][3].
__global__ __launch_bounds__(256) void adv_stats_rows_kernel(const float* __restrict__ adv,
                                                             size_t n,
                                                             float* __restrict__ partials) {
  const float* a = adv + (size_t)blockIdx.y * n;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  Moments mo = {0.f, 0.f, 0.f};
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    push(mo, a[i]);
  block_merge(mo, partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3);
}

// one wave per block k: stats[k] = mean, 1 / (std + 1e-8); (0, 1) with normalisation off
__global__ __launch_bounds__(64) void adv_stats_rows_finalize_kernel(
    const float* __restrict__ partials, int nb, int norm, float* __restrict__ stats) {
  const int lane = threadIdx.x;
  const float* p = partials + (size_t)blockIdx.x * nb * 3;
  Moments s = {0.f, 0.f, 0.f};
  for (int i = lane; i < nb; i += 64) s = merge(s, Moments{p[i * 3], p[i * 3 + 1], p[i * 3 + 2]});
  s = wave_merge(s);
  if (lane == 0) write_stats(s, norm, stats + blockIdx.x * 2);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// ppo_loss_kernel on M elements (items M.. up to MB: g_value's rows to zero) and its finalize;
// the vector kernel where B % 4 == 0 and every array is 16-byte aligned. epoch_mean may be null.
int launch_ppo_loss(const float* logp_new, const float* logp_old, const float* values,
                    const float* v_old, const float* adv, const float* ret, const float* entropy,
                    const float* stats, size_t M, size_t MB, int B, float clip_lo, float clip_hi,
                    float clip, float value_clip, float baseline_cost, float entropy_cost,
                    int step, float* g_logp, float* g_value, float* partials, float* losses,
                    float* epoch_mean, hipStream_t stream) {
  const bool vec = B % 4 == 0 && aligned16(logp_new) && aligned16(logp_old) &&
                   aligned16(values) && aligned16(v_old) && aligned16(adv) && aligned16(ret) &&
                   (!entropy || aligned16(entropy)) && aligned16(g_logp) && aligned16(g_value);
  const size_t items = vec ? MB / 4 : MB;
  const size_t nb = (items + 255) / 256;
  if (nb > 0x7fffffffull) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(vec ? ppo_loss_kernel<4> : ppo_loss_kernel<1>, dim3((unsigned)nb), dim3(256),
                     0, stream, logp_new, logp_old, values, v_old, adv, ret, entropy, stats, M,
                     MB, clip_lo, clip_hi, clip, value_clip, baseline_cost, g_logp, g_value,
                     partials);
  hipLaunchKernelGGL(ppo_finalize_kernel, dim3(1), dim3(64), 0, stream, partials, (int)nb, M,
                     baseline_cost, entropy_cost, step, losses, epoch_mean);
  return (int)hipGetLastError();
}

// blocks of 256 lanes per row block in adv_stats_rows_kernel
inline int stats_rows_blocks(size_t n) {
  const size_t nb = (n + 255) / 256;
  return (int)(nb < 256 ? nb : 256);
}

}  // namespace

// partials: 3 * K * min(256, ceil(T / K * B / 256)) floats; stats [K][2]
extern "C" int mbk_adv_stats_rows(const float* adv, int T, int B, int K, int norm_adv,
                                  float* partials, float* stats, hipStream_t stream) {
  if (T < 1 || B < 1 || K < 1 || K > 65535 || T % K != 0) return (int)hipErrorInvalidValue;
  const size_t n = (size_t)(T / K) * B;
  const int nb = stats_rows_blocks(n);
  hipLaunchKernelGGL(adv_stats_rows_kernel, dim3(nb, K), dim3(256), 0, stream, adv, n, partials);
  hipLaunchKernelGGL(adv_stats_rows_finalize_kernel, dim3(K), dim3(64), 0, stream, partials, nb,
                     norm_adv, stats);
  return (int)hipGetLastError();
}

// partials: 6 * ceil(Tm * B / 256) floats
extern "C" int mbk_ppo_loss_rows(const float* logp_new, const float* logp_old,
                                 const float* values, const float* v_old, const float* adv,
                                 const float* ret, const float* entropy, const float* stats,
                                 int t0, int Tm, int B, float clip_lo, float clip_hi, float clip,
                                 float value_clip, float baseline_cost, float entropy_cost,
                                 int step, float* g_logp, float* g_value, float* partials,
                                 float* losses, float* epoch_mean, hipStream_t stream) {
  if (t0 < 0 || Tm < 1 || B < 1 || step < 0) return (int)hipErrorInvalidValue;
  const size_t M = (size_t)Tm * B, off = (size_t)t0 * B;
  // (MB = M: the step's arrays have no bootstrap row to zero)
  return launch_ppo_loss(logp_new, logp_old + off, values, v_old + off, adv + off, ret + off,
                         entropy, stats, M, M, B, clip_lo, clip_hi, clip, value_clip,
                         baseline_cost, entropy_cost, step, g_logp, g_value, partials, losses,
                         epoch_mean, stream);
}

extern "C" int mbk_gae(const float* v_old, const float* reward, const uint8_t* done, int T, int B,
                       float gamma, float lambda, float reward_clip, int norm_adv, float* adv,
                       float* ret, float* partials, float* stats, hipStream_t stream) {
  if (T < 1 || B < 1) return (int)hipErrorInvalidValue;
  const int nb = (B + 255) / 256;
  hipLaunchKernelGGL(gae_kernel, dim3(nb), dim3(256), 0, stream, v_old, reward, done, T, B, gamma,
                     lambda, reward_clip, adv, ret, partials);
  hipLaunchKernelGGL(gae_finalize_kernel, dim3(1), dim3(64), 0, stream, partials, nb, norm_adv,
                     stats);
  return (int)hipGetLastError();
}

// partials: 6 * ceil(B / 256) floats; stats[2]; is_stats[3]
extern "C" int mbk_vtrace_adv(const float* logp_pi, const float* logp_mu, const float* v,
                              const float* reward, const uint8_t* done, int T, int B, float gamma,
                              float lambda, float rho_bar, float c_bar, float reward_clip,
                              int norm_adv, float* adv, float* ret, float* partials, float* stats,
                              float* is_stats, hipStream_t stream) {
  if (T < 1 || B < 1 || !(rho_bar > 0.f) || !(c_bar > 0.f)) return (int)hipErrorInvalidValue;
  const int nb = (B + 255) / 256;
  hipLaunchKernelGGL(vtrace_adv_kernel, dim3(nb), dim3(256), 0, stream, logp_pi, logp_mu, v,
                     reward, done, T, B, gamma, lambda, rho_bar, c_bar, reward_clip, adv, ret,
                     partials);
  hipLaunchKernelGGL(vtrace_adv_finalize_kernel, dim3(1), dim3(64), 0, stream, partials, nb,
                     norm_adv, 1.f / ((float)T * (float)B), stats, is_stats);
  return (int)hipGetLastError();
}

// partials: 6 * ceil((T+1) * B / 256) floats (the scalar kernel's blocks; the vector kernel
// uses a quarter of them)
extern "C" int mbk_ppo_loss(const float* logp_new, const float* logp_old, const float* values,
                            const float* v_old, const float* adv, const float* ret,
                            const float* entropy, const float* stats, int T, int B,
                            float clip_lo, float clip_hi, float clip, float value_clip,
                            float baseline_cost, float entropy_cost, float* g_logp,
                            float* g_value, float* partials, float* losses, hipStream_t stream) {
  if (T < 1 || B < 1) return (int)hipErrorInvalidValue;
  const size_t M = (size_t)T * B;
  return launch_ppo_loss(logp_new, logp_old, values, v_old, adv, ret, entropy, stats, M,
                         M + (size_t)B, B, clip_lo, clip_hi, clip, value_clip, baseline_cost,
                         entropy_cost, 0, g_logp, g_value, partials, losses, nullptr, stream);
}
