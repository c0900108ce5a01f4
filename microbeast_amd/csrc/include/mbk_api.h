// C ABI of the microbeast_amd HIP kernel library (libmbk_kernels.so).
// Every launcher enqueues on the given HIP stream, never synchronises and never
// allocates, so callers can capture sequences of them into hipGraphs.
// Return value: hipError_t of the launch (0 = success).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBK_MAX_COPY_SEGS 16
typedef struct {
  const void* src;
  void* dst;
  uint64_t bytes;
} MbkCopySeg;

// Many independent D2D copies in ONE launch (rollout scatter).
int mbk_multi_copy(const MbkCopySeg* segs, int n, hipStream_t stream);

typedef struct {
  const float* w;  // fp32 [cout][cin_real][3][3]
  void* fwd;       // bf16 packed fwd weights
  void* bwd;       // bf16 packed dgrad weights (nullable)
  int cin, cin_real, cout;
} MbkPackJob;

int mbk_conv_pack(const MbkPackJob* jobs, int n, hipStream_t stream);

typedef struct {
  const float* w;  // fp32 [cout][cin_real][3][3]
  void* q;         // e4m3 packed fwd weights [cout][nch][32]
  float* scale;    // [cout] dequant multipliers
  int cin, cin_real, cout;
} MbkPackJob8;

int mbk_conv_pack_fp8(const MbkPackJob8* jobs, int n, hipStream_t stream);

// ---- fused acting step (act.hip-level API; kernels in trunk.hip + head.hip) ----------------
// One policy step of the flat IMPALA agent on a 16x16 map in TWO launches:
//   A (trunk.hip act_trunk_kernel): per 16-env tile, 16-bit codes -> obs bit planes + 78-bit
//     masks (written straight into the rollout row), per-cell buckets of active pairs, stage-0
//     conv with the max-pool in registers, the 14 trunk convs in LDS, network.5 + critic;
//   B (head.hip head_act_kernel): sparse head GEMM + masked sampling per 16-pair unit, per-env
//     completion counters: the wave that finishes an env's last active cell sums its log-prob
//     and writes its packed 16-bit actions; the last workgroup resets the buckets and advances
//     the sampler's step counter.
// Model / workspace pointers are fixed per policy lane; step pointers change every step.
typedef struct {
  const void* w0;          // stage-0 conv packed fwd weights [16][9][32] bf16
  const float* b0;         // [16]
  const void* w[14];       // trunk layers 1..14 packed fwd weights (bf16)
  const float* b[14];
  const void* w5;          // network.5 [256][H2*W2*32] bf16, NHWC column order
  const float* b5;         // [256]
  const float* wc;         // critic [256]
  const float* bc;         // [1]
  const void* Wp;          // sparse head [S][80][256] bf16
  const float* bp;         // [S][80]
  uint64_t* rng;           // Philox (seed, step): the step is MbkActStep.step; [1] is set
                           // to step + 1 after the step (the graph path's counter)
  void* feat;              // workspace: network.5 output [E][256] bf16
  int* bucket_cnt;         // [2][S]: step t counts in half t & 1; launch A of step t zeroes
                           // the other half (step t-1's, read by its launch B)
  int* bucket;             // [S][E]
  uint64_t* cellx;         // [E][S] per active cell (rank k): {log-prob, cell | action << 16}
  int* pending;            // [2E]: active cells not yet sampled, then each env's total
  int E, H, W;
} MbkActModel;

typedef struct {
  // input: dense codes + resources, or (code_list != null) the sparse rows of list_stride
  // uint32 per env: word 0 = n | resources << 16, then n entries cell | code << 16 (occupied
  // cells only: empty cells are code 0)
  const uint16_t* codes;   // [E][S] (device or pinned host)
  const int32_t* res;      // [E]
  const uint32_t* code_list;
  uint32_t* obs;           // rollout row [E][S]
  uint32_t* mask;          // [E][S][3]
  uint32_t* obs2;          // optional second destination (previous slot's bootstrap row)
  uint32_t* mask2;
  uint8_t* action;         // [E][S][7]
  float* logp;             // [E]
  float* value;            // [E]
  // output actions: dense packed codes [E][S] (device or pinned host), or (act_list != null)
  // sparse rows: word 0 = n, then n entries cell | code << 16 for the non-noop cells
  uint16_t* act16;
  uint32_t* act_list;
  int list_stride;
  const float* reward_src; // optional reward / done of the previous env step -> dst
  const uint8_t* done_src;
  float* reward_dst;
  uint8_t* done_dst;
  uint64_t step;           // Philox step of this policy step (the lane's step count)
  uint32_t* abits;         // optional [E][S/32] active-cell bitmap of the row (bit c & 31 of
  uint32_t* abits2;        // word c >> 5: the cell's mask is non-zero), + the obs2 copy; the
                           // learner's head compaction then never reads the masks in full
  int32_t greedy;          // 0: sample the actions (Philox); 1: arg-max actions (per segment the
                           // lowest legal index at the legal maximum), no random numbers drawn
} MbkActStep;

int mbk_act_step(const MbkActModel* m, const MbkActStep* s, hipStream_t stream);
// sparse-row I/O of the captured-graph policy step (copy.hip): pinned occupied-cell rows ->
// dense device codes + resources, and dense packed actions -> pinned non-noop action rows
int mbk_rows_to_codes(const uint32_t* rows, int stride, int E, int S, void* codes, int32_t* res,
                      hipStream_t stream);
int mbk_codes_to_rows(const void* act16, int E, int S, uint32_t* rows, int stride,
                      hipStream_t stream);
// the two launches separately (mbk_act_step = A then B)
int mbk_act_trunk(const MbkActModel* m, const MbkActStep* s, hipStream_t stream);
int mbk_act_head(const MbkActModel* m, const MbkActStep* s, hipStream_t stream);

// ---- PPO objective (ppo.hip) ----------------------------------------------------------------
// Time-major fp32 [T, B] arrays (v_old / values / g_value: [T+1, B], row T = the bootstrap).
// GAE(lambda) from one value snapshot: adv, ret [T, B] and stats = (mean, 1 / (std + 1e-8)) of
// adv over its T*B elements, (0, 1) when norm_adv == 0. partials: 3 * ceil(B / 256) floats.
int mbk_gae(const float* v_old, const float* reward, const uint8_t* done, int T, int B,
            float gamma, float lambda, float reward_clip, int norm_adv, float* adv, float* ret,
            float* partials, float* stats, hipStream_t stream);
// mbk_gae corrected for a rollout acted by an older policy (V-trace(lambda)): logp_pi [T, B] are
// the log-probs of the pass that gave v, logp_mu the behaviour ones, w = exp(logp_pi - logp_mu).
//   adv_t = td_t + gamma nd_t lambda d_{t+1},  d_t = min(rho_bar, w_t) td_t
//           + gamma nd_t lambda min(c_bar, w_t) d_{t+1}  (d_T = 0),  ret_t = v[t] + d_t
// is_stats[3] = mean w, share of w > rho_bar, share of w > c_bar. Both bars > 0.
// partials: 6 * ceil(B / 256) floats. Ordered, no atomics.
int mbk_vtrace_adv(const float* logp_pi, const float* logp_mu, const float* v,
                   const float* reward, const uint8_t* done, int T, int B, float gamma,
                   float lambda, float rho_bar, float c_bar, float reward_clip, int norm_adv,
                   float* adv, float* ret, float* partials, float* stats, float* is_stats,
                   hipStream_t stream);
// Clipped surrogate + clipped value loss and their gradients g_logp [T, B], g_value [T+1, B]
// (row T zeroed); losses[7] = pg, value, entropy, total, mean ratio, approx_kl, clip_frac.
// clip_lo / clip_hi = 1 -/+ clip as the caller rounds them; value_clip 0 = unclipped value
// loss; entropy may be null. partials: 6 * ceil((T+1) * B / 256) floats.
int mbk_ppo_loss(const float* logp_new, const float* logp_old, const float* values,
                 const float* v_old, const float* adv, const float* ret, const float* entropy,
                 const float* stats, int T, int B, float clip_lo, float clip_hi, float clip,
                 float value_clip, float baseline_cost, float entropy_cost, float* g_logp,
                 float* g_value, float* partials, float* losses, hipStream_t stream);
// Row-block minibatches: block k = rows [k T/K, (k+1) T/K) of the rollout, all B columns.
// stats[K][2] = each block's own (mean, 1 / (std + 1e-8)) of adv, (0, 1) when norm_adv == 0;
// T % K == 0. partials: 3 * K * min(256, ceil(T/K * B / 256)) floats. Ordered, no atomics.
int mbk_adv_stats_rows(const float* adv, int T, int B, int K, int norm_adv, float* partials,
                       float* stats, hipStream_t stream);
// mbk_ppo_loss on one block: logp_new, values, entropy, g_logp, g_value are the step's own
// [Tm, B] arrays (no bootstrap row); logp_old, v_old, adv, ret are the rollout-wide arrays, read
// from row t0; stats is the block's pair; M = Tm * B. losses[7] is the step's; epoch_mean[7] is
// the running mean over the epoch's steps (step = the step's index in its epoch; 0 restarts
// it). partials: 6 * ceil(Tm * B / 256) floats.
int mbk_ppo_loss_rows(const float* logp_new, const float* logp_old, const float* values,
                      const float* v_old, const float* adv, const float* ret,
                      const float* entropy, const float* stats, int t0, int Tm, int B,
                      float clip_lo, float clip_hi, float clip, float value_clip,
                      float baseline_cost, float entropy_cost, int step, float* g_logp,
                      float* g_value, float* partials, float* losses, float* epoch_mean,
                      hipStream_t stream);

// ---- IMPALA objective with V-trace(lambda) targets and the UPGO term (vtrace.hip) -----------
// mbk_vtrace's arrays (time-major fp32 [T, B]; values / g_value [T+1, B], row T the bootstrap,
// its gradient zeroed; entropy may be null) with the trace cut by lambda * min(c_bar, w) and a
// second policy-gradient term on the upgoing return
//   G_t = r_t + g_t (q_{t+1} >= V_{t+1} ? G_{t+1} : V_{t+1}),  q_t = r_t + g_t V_{t+1},
//   G_{T-1} = q_{T-1},  upgo_adv_t = min(upgo_rho_bar, w_t) (G_t - V_t),
//   g_logp_t = -(adv_t + upgo_cost upgo_adv_t) / (T B).
// vs_out, adv_out, upgo_out (G) [T, B] may each be null. losses[6] = pg (V-trace term alone),
// value, entropy, total (= pg + upgo_cost upgo + value - entropy_cost entropy), mean rho, upgo
// (unweighted). partials: 5 * ceil(B / 256) floats. Ordered, no atomics. Refused with
// hipErrorInvalidValue, nothing launched: T < 1, B < 1, lambda outside [0, 1], upgo_cost < 0,
// upgo_rho_bar <= 0.
int mbk_vtrace_upgo(const float* logp_new, const float* logp_old, const float* values,
                    const float* reward, const uint8_t* done, const float* entropy, int T, int B,
                    float gamma, float lambda, float rho_bar, float c_bar, float pg_rho_bar,
                    float upgo_rho_bar, float baseline_cost, float entropy_cost, float upgo_cost,
                    float reward_clip, float* vs_out, float* adv_out, float* upgo_out,
                    float* g_logp, float* g_value, float* partials, float* losses,
                    hipStream_t stream);

#ifdef __cplusplus
}
#endif
