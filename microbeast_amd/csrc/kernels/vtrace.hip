// Fused V-trace (Espeholt et al. 2018, from_importance_weights) + IMPALA
// losses + their gradients, one lane per trajectory column.
//
// Reference: libs/utils.py:277-329 (PPO_learn): a Python reverse loop over T
// with torch ops per step, then three means. Here the reverse scan runs in
// registers and the kernel writes the gradients the backward needs directly:
//   pg_loss    = -mean(logp * pg_adv)           (sign fixed)
//   value_loss = baseline_cost * mean((vs - V)^2)   (reference: 0.5*mean)
//   ent_loss   = mean(H);  total = pg + value - entropy_cost * ent
//   dL/dlogp_t = -pg_adv_t / M,  dL/dV_t = 2*bc*(V_t - vs_t)/M,
//   dL/dH_t = -entropy_cost / M,  M = T*B (the reference means over T*B).
// Inputs are time-major [T(+1), B]; values[T] is the bootstrap (no gradient).
#include "../include/mbk_api.h"
#include "common.h"

using namespace mbk;

namespace {

__global__ __launch_bounds__(256) void vtrace_kernel(
    const float* __restrict__ logp_new, const float* __restrict__ logp_old,
    const float* __restrict__ values, const float* __restrict__ reward,
    const uint8_t* __restrict__ done, const float* __restrict__ entropy, int T, int B,
    float gamma, float rho_bar, float c_bar, float pg_rho_bar, float baseline_cost,
    float entropy_cost, float reward_clip, float* __restrict__ vs_out,
    float* __restrict__ adv_out, float* __restrict__ g_logp, float* __restrict__ g_value,
    float* __restrict__ partials /* [gridDim.x][4] */) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const float invM = 1.f / ((float)T * (float)B);
  float s_pg = 0.f, s_v = 0.f, s_ent = 0.f, s_rho = 0.f;
  if (b < B) {
    const float boot = values[(size_t)T * B + b];
    float acc = 0.f;
    float vs_next = boot;  // vs_{t+1}, with vs_T = V(x_T)
    float v_next = boot;   // V_{t+1}
    g_value[(size_t)T * B + b] = 0.f;
    for (int t = T - 1; t >= 0; --t) {
      const size_t i = (size_t)t * B + b;
      const float lpn = logp_new[i];
      const float ratio = __expf(lpn - logp_old[i]);
      const float rho = fminf(rho_bar, ratio), c = fminf(c_bar, ratio);
      float r = reward[i];
      if (reward_clip > 0.f) r = fmaxf(-reward_clip, fminf(reward_clip, r));
      const float disc = done[i] ? 0.f : gamma;
      const float v = values[i];
      const float delta = rho * (r + disc * v_next - v);
      acc = delta + disc * c * acc;
      const float vs = acc + v;
      const float adv = fminf(pg_rho_bar, ratio) * (r + disc * vs_next - v);
      if (vs_out) vs_out[i] = vs;
      if (adv_out) adv_out[i] = adv;
      g_logp[i] = -adv * invM;
      g_value[i] = 2.f * baseline_cost * (v - vs) * invM;
      s_pg -= lpn * adv;
      s_v += (vs - v) * (vs - v);
      if (entropy) s_ent += entropy[i];
      s_rho += rho;
      vs_next = vs;
      v_next = v;
    }
  }
  const float s[4] = {s_pg, s_v, s_ent, s_rho};
  block_sums<4>(s, partials + blockIdx.x * 4);
}

// vtrace_kernel with V-trace(lambda) value targets and the UPGO policy term (Vinyals et al.
// 2019): the trace is cut by lambda * min(c_bar, w), and a second policy-gradient term follows
// the sampled return only while it does at least as well as the value estimate,
//   q_t = r_t + g_t V_{t+1},  G_t = r_t + g_t (q_{t+1} >= V_{t+1} ? G_{t+1} : V_{t+1}),
//   G_{T-1} = q_{T-1},  upgo_adv_t = min(upgo_rho_bar, w_t) (G_t - V_t),
//   dL/dlogp_t = -(adv_t + upgo_cost upgo_adv_t) / M.
// G_{t+1}, q_{t+1} and V_{t+1} are the previous iteration's registers: no load is added. All
// three start at the bootstrap, whose tie (q == V) hands the first step G = q_{T-1}.
// lambda = 1 and upgo_cost = 0 are vtrace_kernel's numbers bit for bit: the compiler's contraction
// is off here and in the finalize, and every multiply-add that vtrace_kernel's code object fuses
// is written as fmaf (the others stay apart), so the rounding does not move with the code around
// it. (One scan body, template <bool UPGO> with contraction off in both instances, computes
// vtrace_kernel's arithmetic sequence but measured 3.4 us slower on the default path: not merged.)
// Both scans end in block_sums<K> (common.h) and share vtrace_finalize_kernel<UPGO>.
__global__ __launch_bounds__(256) void vtrace_upgo_kernel(
    const float* __restrict__ logp_new, const float* __restrict__ logp_old,
    const float* __restrict__ values, const float* __restrict__ reward,
    const uint8_t* __restrict__ done, const float* __restrict__ entropy, int T, int B,
    float gamma, float lambda, float rho_bar, float c_bar, float pg_rho_bar, float upgo_rho_bar,
    float baseline_cost, float upgo_cost, float reward_clip, float* __restrict__ vs_out,
    float* __restrict__ adv_out, float* __restrict__ upgo_out, float* __restrict__ g_logp,
    float* __restrict__ g_value, float* __restrict__ partials /* [gridDim.x][5] */) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const float invM = 1.f / ((float)T * (float)B);
  float s_pg = 0.f, s_v = 0.f, s_ent = 0.f, s_rho = 0.f, s_up = 0.f;
  if (b < B) {
    const float boot = values[(size_t)T * B + b];
    float acc = 0.f;
    float vs_next = boot;  // vs_{t+1}, with vs_T = V(x_T)
    float v_next = boot;   // V_{t+1}
    float q_next = boot;   // q_{t+1}
    float G_next = boot;   // G_{t+1}
    g_value[(size_t)T * B + b] = 0.f;
    for (int t = T - 1; t >= 0; --t) {
      const size_t i = (size_t)t * B + b;
      const float lpn = logp_new[i];
      const float ratio = __expf(lpn - logp_old[i]);
      const float rho = fminf(rho_bar, ratio), c = lambda * fminf(c_bar, ratio);
      float r = reward[i];
      if (reward_clip > 0.f) r = fmaxf(-reward_clip, fminf(reward_clip, r));
      const float disc = done[i] ? 0.f : gamma;
      const float v = values[i];
      const float q = fmaf(disc, v_next, r);
      const float delta = rho * (q - v);
      acc = fmaf(disc * c, acc, delta);
      const float vs = acc + v;
      const float adv = fminf(pg_rho_bar, ratio) * (fmaf(disc, vs_next, r) - v);
      const float G = fmaf(disc, q_next >= v_next ? G_next : v_next, r);
      const float uadv = fminf(upgo_rho_bar, ratio) * (G - v);
      if (vs_out) vs_out[i] = vs;
      if (adv_out) adv_out[i] = adv;
      if (upgo_out) upgo_out[i] = G;
      g_logp[i] = -(adv + upgo_cost * uadv) * invM;
      g_value[i] = 2.f * baseline_cost * (v - vs) * invM;
      s_pg = fmaf(-lpn, adv, s_pg);
      s_up = fmaf(-lpn, uadv, s_up);
      s_v = fmaf(vs - v, vs - v, s_v);
      if (entropy) s_ent += entropy[i];
      s_rho += rho;
      vs_next = vs;
      v_next = v;
      q_next = q;
      G_next = G;
    }
  }
  const float s[5] = {s_pg, s_v, s_ent, s_rho, s_up};
  block_sums<5>(s, partials + blockIdx.x * 5);
}

// losses[0..4] = pg, value, entropy, total, mean_rho; UPGO: [5] = upgo (pg: the V-trace term
// alone; upgo unweighted; total = pg + upgo_cost * upgo + value - entropy_cost * entropy)
template <bool UPGO>
__global__ __launch_bounds__(64) void vtrace_finalize_kernel(
    const float* __restrict__ partials, int nblocks, int T, int B, float baseline_cost,
    float entropy_cost, float upgo_cost, float* __restrict__ losses) {
#pragma clang fp contract(off)
  constexpr int K = UPGO ? 5 : 4;
  const int lane = threadIdx.x;
  float s[K] = {};
  for (int i = lane; i < nblocks; i += 64)
    for (int k = 0; k < K; ++k) s[k] += partials[i * K + k];
  for (int k = 0; k < K; ++k) s[k] = wave_sum(s[k]);
  if (lane == 0) {
    const float invM = 1.f / ((float)T * (float)B);
    const float pg = s[0] * invM, vl = baseline_cost * s[1] * invM, ent = s[2] * invM;
    float total = pg;
    if constexpr (UPGO) {
      const float up = s[K - 1] * invM;
      total = pg + upgo_cost * up;
      losses[5] = up;
    }
    losses[0] = pg;
    losses[1] = vl;
    losses[2] = ent;
    losses[3] = total + vl - entropy_cost * ent;
    losses[4] = s[3] * invM;
  }
}

}  // namespace

extern "C" int mbk_vtrace_upgo(const float* logp_new, const float* logp_old, const float* values,
                               const float* reward, const uint8_t* done, const float* entropy,
                               int T, int B, float gamma, float lambda, float rho_bar,
                               float c_bar, float pg_rho_bar, float upgo_rho_bar,
                               float baseline_cost, float entropy_cost, float upgo_cost,
                               float reward_clip, float* vs_out, float* adv_out, float* upgo_out,
                               float* g_logp, float* g_value,
                               float* partials /* >= 5*ceil(B/256) */, float* losses /* 6 */,
                               hipStream_t stream) {
  // (negated comparisons: a NaN is refused too)
  if (T < 1 || B < 1 || !(lambda >= 0.f && lambda <= 1.f) || !(upgo_cost >= 0.f) ||
      !(upgo_rho_bar > 0.f))
    return (int)hipErrorInvalidValue;
  const int nb = (B + 255) / 256;
  hipLaunchKernelGGL(vtrace_upgo_kernel, dim3(nb), dim3(256), 0, stream, logp_new, logp_old,
                     values, reward, done, entropy, T, B, gamma, lambda, rho_bar, c_bar,
                     pg_rho_bar, upgo_rho_bar, baseline_cost, upgo_cost, reward_clip, vs_out,
                     adv_out, upgo_out, g_logp, g_value, partials);
  hipLaunchKernelGGL(vtrace_finalize_kernel<true>, dim3(1), dim3(64), 0, stream, partials, nb, T,
                     B, baseline_cost, entropy_cost, upgo_cost, losses);
  return (int)hipGetLastError();
}

extern "C" int mbk_vtrace(const float* logp_new, const float* logp_old, const float* values,
                          const float* reward, const uint8_t* done, const float* entropy, int T,
                          int B, float gamma, float rho_bar, float c_bar, float pg_rho_bar,
                          float baseline_cost, float entropy_cost, float reward_clip,
                          float* vs_out, float* adv_out, float* g_logp, float* g_value,
                          float* partials /* >= 4*ceil(B/256) */, float* losses /* 5 */,
                          hipStream_t stream) {
  const int nb = (B + 255) / 256;
  hipLaunchKernelGGL(vtrace_kernel, dim3(nb), dim3(256), 0, stream, logp_new, logp_old, values,
                     reward, done, entropy, T, B, gamma, rho_bar, c_bar, pg_rho_bar, baseline_cost,
                     entropy_cost, reward_clip, vs_out, adv_out, g_logp, g_value, partials);
  hipLaunchKernelGGL(vtrace_finalize_kernel<false>, dim3(1), dim3(64), 0, stream, partials, nb, T,
                     B, baseline_cost, entropy_cost, 0.f, losses);
  return (int)hipGetLastError();
}
