// w2a_actor_critic.hip.h -- shared-trunk actor-critic (PPO-clip + value regression + entropy) along GIVEN schedules:
// one MLP whose output layer keeps two rows, row 0 the policy logit z and row 1 the state value V
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_ACTOR_CRITIC_HIP_H
#define W2A_ACTOR_CRITIC_HIP_H

// ----------------------------------------------------------------------------------------
// one trunk, two output rows (w2a_actor_critic_mlp, estimator in w2a.h)
// ----------------------------------------------------------------------------------------
// The env is forced along its schedule exactly as in w2a_surrogate.hip.h (the same bitmap, the same attempted-versus-
// issued rule, the same rows, the same scored days m_s: a day require_budget forces or the gate closes is attempted as 0
// and has no policy score) and pays its rewards exactly as in w2a_gae.hip.h. The parameter block is the two-head layout
// of w2a_qlearn.hip.h; mlp_heads2 evaluates the hidden layers once and gives both rows, each bit for bit what mlp_logit
// returns for the one-output net of the same hidden layers and that row. Per env-day BOTH rows receive a coefficient:
//     c_pi,s = w_e (live_s rho_s A_s delta_s + beta dH_s/dz)   on dz_s/dtheta  (k_sg_pass1's c_s; 0 on a forced day)
//     c_v,s  = w_e vf_coef (T_s - V_s)                          on dV_s/dtheta  (every stepped day)
//   k_ac_pass1<.., EPOCH = false>  COLLECT: k_gae_pass1's day loop with mlp_heads2_groups in place of mlp_logit_groups and
//                       k_sg_pass1's scored-day rule. Leaves day = (f32(delta_s), V_s) (the TD residual of row 1, as
//                       k_gae_pass1), z_s in one more f32 column [n_steps][n], and the alert byte with two more bits
//                       (bit 1 the schedule's a_s, bit 2 m_s) that k_ac_finish takes out again.
//   k_ac_finish         collect only: k_gae_finish's backward sweep -- A_s = delta_s + gamma lambda A_{s+1} in fp64, written
//                       with T_s = A_s + V_s and lp_s at the env's id by the statements k_gae_finish and sg_day use (so
//                       the three arrays are the bits value_gradient() and surrogate_gradient(log_prob=True) give for
//                       the one-head nets) -- then both coefficients with rho = 1 and T_s - V_s = A_s, and the record
//                       overwritten in place with day = (f32(c_pi), f32(c_v)) and the plain alert byte.
//   k_ac_pass1<.., EPOCH = true>   advantages, targets and old log-probabilities are given: no reward is formed, both
//                       coefficients are complete on the day itself (fp64, as k_sg_pass1 and the TARGET form of
//                       k_gae_pass1), day = (f32(c_pi), f32(c_v)); no finish kernel runs.
//   k_ac_pass2          the text of k_pgm_pass2 (w2a_policy_gradient_mlp_pass2.inc.h) with HEADS = 2 and PGM_PASS2_BOTH:
//                       one row rebuild, one forward and one backward pass serve both losses. k_pgm_count, k_pgm_scan and
//                       k_pgm_reduce run unchanged (ga.total is neither written nor read).
// No floating-point atomics: identical calls give identical bits.
struct AcArgs {
  SurrogateArgs sg;           // schedule, w_e, lo / hi / beta, the per-env sums; EPOCH: advantage and old_log_prob (both
                              // non-NULL); COLLECT: log_prob = the "log_prob" rows (never NULL), advantage = NULL
  const float *value_target;  // EPOCH: [>= n_steps][n] T_s by call-day and ENV ID
  double vf_coef;
  double gamma, gl;           // COLLECT: discount, gamma * lambda
  int32_t bootstrap;          // COLLECT: 1: Vn of a truncated env's last call-day is row 1 on the row it then holds
  float *advantage_out;       // COLLECT: [n_steps][n] A_s by call-day and ENV ID; zero-filled before the launch
  float *value_target_out;    // COLLECT: [n_steps][n] T_s, same layout
  float *value_loss;          // [n] sum_s 1/2 (T_s - V_s)^2
  float *ret;                 // [n] sum_s r_s (COLLECT)
  float *day_z;               // COLLECT: [n_steps][n] z_s of the lane at visiting position `slot` (workspace)
};

struct AcMlpArgs {
  MlpGradArgs g;  // as w2a_q_gradient_mlp builds it (m.stride = the two-head stride; baseline and total unused)
  AcArgs ac;
};

#define AC_BYTE_LABEL 2u   // the schedule's bit a_s
#define AC_BYTE_SCORED 4u  // m_s

// sg_day's statements with the advantage and the old log-probability as arguments (COLLECT has A_s in fp64 and
// rho = 1: has_old = false). Returns c_pi,s and adds the day's terms to the per-env sums; lp is the day's log pi.
__device__ __forceinline__ double ac_day(const SurrogateArgs &sg, double w_e, double z, float delta, uint32_t a, double A,
                                         bool has_old, double old_lp, SgSums &sum, double &lp_out) {
  const double lp = im_log_pi(z, a);
  const double e = exp(-fabs(z));
  const double r = 1.0 / (1.0 + e);
  const double p = z >= 0.0 ? r : e * r, q = z >= 0.0 ? e * r : r;
  const double lp_other = a ? lp - z : lp + z;
  double rho = 1.0, d = 0.0;
  if (has_old) {
    d = lp - old_lp;
    rho = exp(d);
  }
  const bool live = !((A > 0.0 && rho > sg.hi) || (A < 0.0 && rho < sg.lo));
  const double rA = rho * A;
  sum.L += fmin(rA, fmin(fmax(rho, sg.lo), sg.hi) * A);
  sum.kl += (rho - 1.0) - d;
  sum.H -= a ? p * lp + q * lp_other : q * lp + p * lp_other;
  sum.clipped += live ? 0 : 1;
  sum.scored += 1;
  lp_out = lp;
  double c = live ? (w_e * (double)delta) * rA : 0.0;
  if (sg.beta != 0.0) c += w_e * (sg.beta * (-z * p * q));  // beta dH/dz
  return c;
}

// ------------------------------------------------------------------------------------------------ pass 1
// Registers: as k_gae_pass1 (wb[32], we[32] and xv[32] next to the network's fragments; EPOCH drops both reward rows).
template <int WIDTH, int LAYERS, bool GATE, bool EPOCH>
__global__ __launch_bounds__(BLOCK, 2) void k_ac_pass1(const AcMlpArgs xa) {
  __shared__ __attribute__((aligned(16))) float s_x[MLP_WAVES][64 * MLP_XS];
  const MlpGradArgs &ga = xa.g;
  const MlpRolloutArgs &ma = ga.m;
  const RolloutArgs &a = ma.r;
  const SurrogateArgs &sg = xa.ac.sg;
  const int64_t slot64 = (int64_t)logical_block(blockIdx.x, gridDim.x >> 3) * BLOCK + threadIdx.x;
  if (slot64 - (threadIdx.x & 63) >= a.n) return;  // whole wave past the end
  const bool valid = slot64 < a.n;
  const uint32_t slot = (uint32_t)(valid ? slot64 : (a.n - 1));
  uint32_t e = a.order ? a.order[slot] : slot;  // the env this lane serves
  e = e < (uint32_t)a.n ? e : (uint32_t)(a.n - 1);
  float *xs = s_x[threadIdx.x >> 6];
  float *xrow = xs + (threadIdx.x & 63) * MLP_XS;
  uint4 c2, hot;
  load_step_state(a.st, e, c2, hot);
  const uint4 cold = load_cold(a.st, e);
  uint32_t t = D0_T(hot.x), used = D0_USED(hot.x), streak = D0_STREAK(hot.x), hist = D1_HIST(hot.y);
  const uint32_t ndays = D1_NDAYS(hot.y);
  const int32_t budget = (int32_t)hot.w;
  const uint32_t rows_per_day = (uint32_t)(a.tb.S_w * a.tb.Y);
  float wb[32], we[32];
  if (!EPOCH) {
    const uint32_t wrow = W_COL(cold.y) * (uint32_t)a.tb.n_samples + W_SAMPLE(cold.y);
    const float4 *wq = a.tb.W + (size_t)wrow * (2 * ROWF / 4);
#pragma unroll
    for (int q = 0; q < ROWF / 4; ++q) {
      const float4 b = wq[q], f = wq[ROWF / 4 + q];
      wb[4 * q] = b.x; wb[4 * q + 1] = b.y; wb[4 * q + 2] = b.z; wb[4 * q + 3] = b.w;
      we[4 * q] = f.x; we[4 * q + 1] = f.y; we[4 * q + 2] = f.z; we[4 * q + 3] = f.w;
    }
  }
  const int32_t g = pgm_group(ma, e);
  const uint32_t obs0 = e * (uint32_t)ma.n_obs;
  const size_t n = (size_t)a.n;
  const double w_e = sg.env_weight ? (double)sg.env_weight[e] : 1.0;
  uint32_t lab_word = 0, lab_idx = 0xFFFFFFFFu;
  uint32_t gate_word = 0, gate_idx = 0xFFFFFFFFu;
  SgSums sum = {0.0, 0.0, 0.0, 0, 0};
  double ret = 0.0, vl = 0.0;
  int32_t n_valid = 0;
  bool active = D1_FIN(hot.y) == 0 && valid;
#pragma unroll
  for (int k = 0; k < ROWF; ++k)
    xrow[k] = (k < RO64_SLOTS && ma.slot_obs[k] >= 0 && active) ? ma.obs[obs0 + ma.slot_obs[k]] : 0.0f;
  mlp_wave_lds_sync();
  float z, v;  // z_s and V_s: both rows on the row the env holds
  mlp_heads2_groups<WIDTH, LAYERS>(ma, ma.params, g, xs, z, v);
  for (int s = 0; s < a.n_steps; ++s) {
    if (!__any(active)) break;
    const uint32_t lab = active ? im_label_bits(sg.alert_mask, sg.mask_words, e, t, lab_word, lab_idx) : 0u;
    const float p = sigmoid_f32(z);
    int32_t act = (int32_t)lab;
    const float delta = (float)act - p;
    bool scores = true;
    if (a.pol.require_budget && budget - (int32_t)used <= 0) { act = 0; scores = false; }  // m_s = 0: forced
    if (GATE && active && !gate_allows(ma.gate, ma.gate_words, e, t, gate_word, gate_idx)) { act = 0; scores = false; }
    const uint32_t atb_s = ((int32_t)used == budget) ? 1u : 0u;
    const uint32_t actual = (act == 1 && atb_s) ? 0u : (uint32_t)act;
    const uint32_t used2 = used + actual;
    const uint32_t hist2 = ((hist << 1) | actual) & 0x3FFFu;
    const uint32_t day_row = t * rows_per_day + cold.x;
    float xv[32];
    {
      const float4 *xp = a.tb.X + (size_t)day_row * (ROWF / 4);
#pragma unroll
      for (int q = 0; q < ROWF / 4; ++q) {
        if (q == RT_QUAD) continue;  // slots 24..27 are run-time fields
        const float4 x4 = xp[q];
        xv[4 * q] = x4.x; xv[4 * q + 1] = x4.y; xv[4 * q + 2] = x4.z; xv[4 * q + 3] = x4.w;
      }
    }
    xv[4 * RT_QUAD] = (t > 0) ? (float)actual : 0.0f;
    xv[4 * RT_QUAD + 1] = (float)streak;
    xv[4 * RT_QUAD + 2] = (float)(budget - (int32_t)used2);
    xv[4 * RT_QUAD + 3] = (float)__popc(hist2);
    float r = 0.0f;
    if (!EPOCH) {
      double zb = 0.0, ze = 0.0;
#pragma unroll
      for (int k = 0; k < RO64_SLOTS; ++k) {
        asm volatile("" : "+v"(wb[k]), "+v"(we[k]));  // keep the coefficients f32 (see k_rollout64)
        const double xk = (double)xv[k];
        zb = fma(xk, (double)wb[k], zb);
        ze = fma(xk, (double)we[k], ze);
      }
      if (!(xv[30] > 0.5f)) ze = -__builtin_inf();
      r = reward_from_logits(zb, ze, actual);
    }
    // tomorrow's network input: the observation columns of xv[] (zeros elsewhere and for lanes with no live env)
    mlp_wave_lds_sync();  // every lane's reads of the previous input are done
#pragma unroll
    for (int q = 0; q < ROWF / 4; ++q) {
      float4 x4;
      x4.x = (active && ((ma.obs_mask >> (4 * q)) & 1u)) ? xv[4 * q] : 0.0f;
      x4.y = (active && ((ma.obs_mask >> (4 * q + 1)) & 1u)) ? xv[4 * q + 1] : 0.0f;
      x4.z = (active && ((ma.obs_mask >> (4 * q + 2)) & 1u)) ? xv[4 * q + 2] : 0.0f;
      x4.w = (active && ((ma.obs_mask >> (4 * q + 3)) & 1u)) ? xv[4 * q + 3] : 0.0f;
      reinterpret_cast<float4 *>(xrow)[q] = x4;
    }
    const bool stepped = active;
    // wave-uniform: a row after this day is looked at -- inside the call, or past it when a collect call bootstraps
    const bool look = s + 1 < a.n_steps || (!EPOCH && xa.ac.bootstrap);
    bool more = false;  // the env holds a row after this day whose value enters: Vn_s is row 1 on it
    if (active) {
      const bool done = (t + 1 >= ndays);
      more = !done && look;
      used = used2; hist = hist2;
      if (!done) { streak = actual ? streak + 1 : 0; t = t + 1; }
      else active = false;
    }
    float zn = 0.0f, vn = 0.0f;
    if (look) {  // both rows on the row each env now holds, for tomorrow (or for the bootstrap)
      mlp_wave_lds_sync();
      mlp_heads2_groups<WIDTH, LAYERS>(ma, ma.params, g, xs, zn, vn);
    }
    if (stepped) {  // day s's record
      const size_t d = (size_t)s * n + slot;
      const size_t day_env = (size_t)s * n + e;
      if (EPOCH) {
        double lp;
        const double c_pi = scores ? ac_day(sg, w_e, (double)z, delta, lab, (double)sg.advantage[day_env], true,
                                            (double)sg.old_log_prob[day_env], sum, lp)
                                   : 0.0;
        const double dv = (double)xa.ac.value_target[day_env] - (double)v;  // T_s - V_s
        vl = fma(0.5 * dv, dv, vl);
        ga.day[d] = make_float2((float)c_pi, (float)(w_e * (xa.ac.vf_coef * dv)));
        ga.day_alert[d] = (uint8_t)actual;
      } else {
        const float dl = (float)(((double)r + xa.ac.gamma * (more ? (double)vn : 0.0)) - (double)v);
        ga.day[d] = make_float2(dl, v);  // k_ac_finish turns it into (c_pi, c_v)
        xa.ac.day_z[d] = z;
        ga.day_alert[d] = (uint8_t)(actual | (lab ? AC_BYTE_LABEL : 0u) | (scores ? AC_BYTE_SCORED : 0u));
        ret += (double)r;
      }
      n_valid = s + 1;
    }
    z = zn;
    v = vn;
  }
  if (valid) {
    ga.n_valid[slot] = n_valid;
    if (EPOCH) {
      sg.surrogate[e] = (float)sum.L;
      sg.clipped[e] = sum.clipped;
      sg.approx_kl[e] = (float)sum.kl;
      sg.entropy[e] = (float)sum.H;
      sg.days[e] = sum.scored;
      xa.ac.value_loss[e] = (float)vl;
    } else {
      xa.ac.ret[e] = (float)ret;
    }
  }
}

// collect: per visiting position, from the env's last day back. The loads and stores of `day`, `day_z` and the alert
// byte are lane-consecutive; the rows go to the env's own column, lane-consecutive in identity order.
__global__ __launch_bounds__(256) void k_ac_finish(const AcMlpArgs xa) {
  const MlpGradArgs &ga = xa.g;
  const RolloutArgs &a = ga.m.r;
  const SurrogateArgs &sg = xa.ac.sg;
  const int64_t slot64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot64 >= a.n) return;
  const uint32_t slot = (uint32_t)slot64;
  uint32_t e = a.order ? a.order[slot] : slot;
  e = e < (uint32_t)a.n ? e : (uint32_t)(a.n - 1);
  const size_t n = (size_t)a.n;
  const int32_t nv = ga.n_valid[slot];
  const double w_e = sg.env_weight ? (double)sg.env_weight[e] : 1.0;
  float *adv = xa.ac.advantage_out + e;
  float *vt = xa.ac.value_target_out + e;
  float *lpo = sg.log_prob + e;
  SgSums sum = {0.0, 0.0, 0.0, 0, 0};
  double A = 0.0, vl = 0.0;
  for (int s = nv - 1; s >= 0; --s) {
    const size_t d = (size_t)s * n + slot;
    const float2 rec = ga.day[d];  // (f32(delta_s), V_s)
    const uint32_t byte = ga.day_alert[d];
    A = fma(xa.ac.gl, A, (double)rec.x);
    adv[(size_t)s * n] = (float)A;
    vt[(size_t)s * n] = (float)(A + (double)rec.y);
    double c_pi = 0.0;
    if (byte & AC_BYTE_SCORED) {
      const float z = xa.ac.day_z[d];
      const uint32_t lab = (byte & AC_BYTE_LABEL) ? 1u : 0u;
      const float delta = (float)(int32_t)lab - sigmoid_f32(z);
      double lp;
      c_pi = ac_day(sg, w_e, (double)z, delta, lab, A, false, 0.0, sum, lp);
      lpo[(size_t)s * n] = (float)lp;
    }
    vl = fma(0.5 * A, A, vl);  // T_s - V_s = A_s
    ga.day[d] = make_float2((float)c_pi, (float)(w_e * (xa.ac.vf_coef * A)));
    ga.day_alert[d] = (uint8_t)(byte & 1u);
  }
  sg.surrogate[e] = (float)sum.L;
  sg.clipped[e] = sum.clipped;
  sg.approx_kl[e] = (float)sum.kl;
  sg.entropy[e] = (float)sum.H;
  sg.days[e] = sum.scored;
  xa.ac.value_loss[e] = (float)vl;
}

// ------------------------------------------------------------------------------------------------ pass 2
// k_qg_pass2's registers without the per-day row select; one more f32 per lane (c_v) and one more row fragment in the
// backward pass's first step. The compiler's figures: DESIGN.md.
#define PGM_PASS2_KERNEL k_ac_pass2
#define PGM_PASS2_HEADS 2
#define PGM_PASS2_BOTH 1
#include "w2a_policy_gradient_mlp_pass2.inc.h"
#undef PGM_PASS2_KERNEL
#undef PGM_PASS2_HEADS
#undef PGM_PASS2_BOTH

// gradient = false (collect only): the first pass and the sweep alone -- the three [n_steps][n] arrays and the per-env sums
template <int WIDTH, int LAYERS>
static void launch_ac(const AcMlpArgs &xa, bool epoch, bool gradient, unsigned grid1, hipStream_t s) {
  const MlpGradArgs &ga = xa.g;
  if (epoch) {
    if (ga.m.gate) hipLaunchKernelGGL((k_ac_pass1<WIDTH, LAYERS, true, true>), dim3(grid1), dim3(BLOCK), 0, s, xa);
    else hipLaunchKernelGGL((k_ac_pass1<WIDTH, LAYERS, false, true>), dim3(grid1), dim3(BLOCK), 0, s, xa);
  } else {
    if (ga.m.gate) hipLaunchKernelGGL((k_ac_pass1<WIDTH, LAYERS, true, false>), dim3(grid1), dim3(BLOCK), 0, s, xa);
    else hipLaunchKernelGGL((k_ac_pass1<WIDTH, LAYERS, false, false>), dim3(grid1), dim3(BLOCK), 0, s, xa);
    hipLaunchKernelGGL(k_ac_finish, dim3((unsigned)((ga.m.r.n + 255) / 256)), dim3(256), 0, s, xa);
  }
  if (!gradient) return;
  hipLaunchKernelGGL(k_pgm_count, dim3(ga.n_chunks), dim3(64), 0, s, ga);
  hipLaunchKernelGGL(k_pgm_scan, dim3(1), dim3(1024), 0, s, ga);
  hipLaunchKernelGGL((k_ac_pass2<WIDTH, LAYERS>), dim3(ga.n_chunks), dim3(64), 0, s, ga);
  hipLaunchKernelGGL(k_pgm_reduce, dim3(ga.m.n_groups, (ga.m.stride + 255) / 256), dim3(256), 0, s, ga);
}

#endif  // W2A_ACTOR_CRITIC_HIP_H
