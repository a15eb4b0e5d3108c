// w2a_qlearn.hip.h -- DQN / double-DQN temporal-difference semi-gradient of a two-head MLP Q-net along GIVEN schedules
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_QLEARN_HIP_H
#define W2A_QLEARN_HIP_H

// ----------------------------------------------------------------------------------------
// Q-learning along a schedule (w2a_q_gradient_mlp, estimator in w2a.h)
// ----------------------------------------------------------------------------------------
// The env is forced along its schedule and pays its rewards exactly as in w2a_value.hip.h. The network has TWO output
// rows, Q(o, 0) and Q(o, 1), in the two-head block layout of w2a.h (the w2a_mlp_policy block with the tail
// wo0[w], wo1[w], bo0, bo1, 2 pad; stride W2A_MLP_HEADS_STRIDE = W2A_MLP_STRIDE + w, rows stay 16-B aligned). Per day
//     y_s = r_s + gamma N_s,   N_s = max_a' Qt(o_{s+1}, a')  (double: Qt(o_{s+1}, argmax_a' Q(o_{s+1}, a'))),
//     delta_s = y_s - Q(o_s, a_s),   c_s = delta_s (squared) or clamp(delta_s, +-huber_delta) (Huber)
// with a_s the alert ISSUED, N_s = 0 on the episode's last day and on the call's last day unless `bootstrap`, and the
// max / argmax restricted to a' = 0 when require_budget is set and no budget is left after day s.
//   mlp_heads2          mlp_logit's forward pass with the hidden layers computed once and two output chains, each in
//                       mlp_logit's order (bias first, the same fmaf order, the same two __shfl_xor folds): head a is,
//                       bit for bit, what mlp_logit returns for the one-output net of the same hidden layers and row a.
//   k_qg_pass1          k_vg_pass1's day loop. Every row is evaluated under the online block and, unless the target
//                       block IS the online one (wave-uniform), under the target block. The four values of row s + 1
//                       close day s: c_s is complete then, so no finish kernel runs. With `bootstrap` one more
//                       wave-uniform evaluation follows the call's last day (as k_gae_pass1). The day record is the one
//                       k_sg_pass1 leaves: day = (f32(w_e c_s), 0), total = 1, and the alert byte -- which pass 2 now
//                       also reads as the head a_s whose output row the backward pass starts from.
//   k_qg_pass2          the text of k_pgm_pass2 (w2a_policy_gradient_mlp_pass2.inc.h) with HEADS = 2: dh_last =
//                       c_s w_out[a_s], dw_out and db_out accumulated per head. k_pgm_count, k_pgm_scan and k_pgm_reduce
//                       run unchanged (the reduce kernel is stride-generic).
// y_s, delta_s and c_s are formed in fp64 from the f32 head values and the f32 reward and stored as f32. No
// floating-point atomics: identical calls give identical bits.
struct QgMlpArgs {
  MlpGradArgs g;         // as w2a_value_gradient_mlp builds it, m.stride = the two-head stride; m.r.pol.require_budget
  ValueArgs v;           // the schedule and w_e; sq_error = loss [n], advantage = td_error [n_steps][n] (nullable)
  const float *tparams;  // [n_groups][stride] the target net's blocks (== g.m.params: the online net is its own target)
  float *td_target;      // [n_steps][n] y_s by call-day and ENV ID (nullable); zero-filled before the launch
  double gamma;
  double huber_delta;    // <= 0: squared loss
  int32_t double_q;      // 1: the online net picks a', the target net values it
  int32_t bootstrap;     // 1: N of a truncated env's last call-day is taken on the row it then holds
};

// both heads of every lane's env under group block p (two-head layout); xs holds the wave's 64 input rows
template <int WIDTH, int LAYERS>
__device__ __forceinline__ void mlp_heads2(const float *__restrict__ p, const float *xs, int activation, float &q0,
                                           float &q1) {
  constexpr int NT = WIDTH / 16;  // hidden tiles
  constexpr int NB = 4 / NT;      // blocks of 16 envs per pass: NT * NB = 4 accumulator tiles
  const int l = threadIdx.x & 63, lo = l & 15, hi = l >> 4;
  const float *W1 = p, *b1 = p + ROWF * WIDTH;
  const float *W2 = b1 + WIDTH, *b2 = W2 + WIDTH * WIDTH;
  const float *wo0 = LAYERS == 2 ? b2 + WIDTH : W2;
  const float *wo1 = wo0 + WIDTH;
  const float bo0 = wo1[WIDTH], bo1 = wo1[WIDTH + 1];
  float z0 = 0.0f, z1 = 0.0f;
#pragma unroll
  for (int b0 = 0; b0 < 4; b0 += NB) {
    mlp_f4 h[NB][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const mlp_f4 bias = *reinterpret_cast<const mlp_f4 *>(b1 + 16 * t + 4 * hi);  // bias first
#pragma unroll
      for (int j = 0; j < NB; ++j) h[j][t] = bias;
    }
#pragma unroll
    for (int ks = 0; ks < ROWF / 4; ++ks) {
      float xb[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) xb[j] = xs[(16 * (b0 + j) + lo) * MLP_XS + 4 * ks + hi];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float a = W1[(4 * ks + hi) * WIDTH + 16 * t + lo];
#pragma unroll
        for (int j = 0; j < NB; ++j) h[j][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xb[j], h[j][t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) h[j][t][i] = mlp_act(h[j][t][i], activation);
    if (LAYERS == 2) {
      mlp_f4 h2[NB][NT];
#pragma unroll
      for (int o = 0; o < NT; ++o) {
        const mlp_f4 bias = *reinterpret_cast<const mlp_f4 *>(b2 + 16 * o + 4 * hi);
#pragma unroll
        for (int j = 0; j < NB; ++j) h2[j][o] = bias;
      }
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int o = 0; o < NT; ++o) {
            const float a = W2[(16 * t + 4 * hi + i) * WIDTH + 16 * o + lo];
#pragma unroll
            for (int j = 0; j < NB; ++j) h2[j][o] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, h[j][t][i], h2[j][o], 0, 0, 0);
          }
#pragma unroll
      for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int o = 0; o < NT; ++o)
#pragma unroll
          for (int i = 0; i < 4; ++i) h[j][o][i] = mlp_act(h2[j][o][i], activation);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      float s0 = hi == 0 ? bo0 : 0.0f, s1 = hi == 0 ? bo1 : 0.0f;  // b_out first
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const mlp_f4 w0 = *reinterpret_cast<const mlp_f4 *>(wo0 + 16 * t + 4 * hi);
        const mlp_f4 w1 = *reinterpret_cast<const mlp_f4 *>(wo1 + 16 * t + 4 * hi);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          s0 = fmaf(w0[i], h[j][t][i], s0);
          s1 = fmaf(w1[i], h[j][t][i], s1);
        }
      }
      s0 += __shfl_xor(s0, 16);  // (l, l^16) then (l^32, l^48), as mlp_logit
      s0 += __shfl_xor(s0, 32);
      s1 += __shfl_xor(s1, 16);
      s1 += __shfl_xor(s1, 32);
      if (hi == b0 + j) { z0 = s0; z1 = s1; }
    }
  }
  q0 = z0;
  q1 = z1;
}

// every lane's two head values for the input rows in xs under the blocks at `params` (the online or the target net's),
// over the distinct groups of the wave (wave-uniform loop, as mlp_logit_groups)
template <int WIDTH, int LAYERS>
__device__ __forceinline__ void mlp_heads2_groups(const MlpRolloutArgs &ma, const float *params, int32_t g,
                                                  const float *xs, float &q0, float &q1) {
  q0 = 0.0f;
  q1 = 0.0f;
  uint64_t todo = __ballot(1);
  while (todo) {
    const int32_t gw = __builtin_amdgcn_readfirstlane(__shfl(g, __ffsll((unsigned long long)todo) - 1));
    float a0, a1;
    mlp_heads2<WIDTH, LAYERS>(params + (size_t)gw * ma.stride, xs, ma.activation, a0, a1);
    if (g == gw) { q0 = a0; q1 = a1; }
    todo &= ~__ballot(g == gw);
  }
}

// ------------------------------------------------------------------------------------------------ pass 1
// Registers: as k_vg_pass1 (wb[32], we[32] and xv[32] next to the network's fragments); the record of the day at hand
// (r, Q(o_s, .), the alert, the mask flag) lives across the two evaluations of the next row.
template <int WIDTH, int LAYERS>
__global__ __launch_bounds__(BLOCK, 2) void k_qg_pass1(const QgMlpArgs qa) {
  __shared__ __attribute__((aligned(16))) float s_x[MLP_WAVES][64 * MLP_XS];
  const MlpGradArgs &ga = qa.g;
  const MlpRolloutArgs &ma = ga.m;
  const RolloutArgs &a = ma.r;
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
  const uint32_t wrow = W_COL(cold.y) * (uint32_t)a.tb.n_samples + W_SAMPLE(cold.y);
  float wb[32], we[32];
  {
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
  const float w_e = qa.v.env_weight ? qa.v.env_weight[e] : 1.0f;
  const bool own = qa.tparams == ma.params;  // wave-uniform: the online net is its own target
  const bool huber = qa.huber_delta > 0.0;
  uint32_t lab_word = 0, lab_idx = 0xFFFFFFFFu;
  double loss = 0.0, ret = 0.0;
  int32_t n_valid = 0;
  bool active = D1_FIN(hot.y) == 0 && valid;
#pragma unroll
  for (int k = 0; k < ROWF; ++k)
    xrow[k] = (k < RO64_SLOTS && ma.slot_obs[k] >= 0 && active) ? ma.obs[obs0 + ma.slot_obs[k]] : 0.0f;
  mlp_wave_lds_sync();
  float q0, q1;  // Q(o_s, .) under the online net: the row the env holds
  mlp_heads2_groups<WIDTH, LAYERS>(ma, ma.params, g, xs, q0, q1);
  for (int s = 0; s < a.n_steps; ++s) {
    if (!__any(active)) break;
    const int32_t act = active ? (int32_t)im_label_bits(qa.v.alert_mask, qa.v.mask_words, e, t, lab_word, lab_idx) : 0;
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
        const float4 v = xp[q];
        xv[4 * q] = v.x; xv[4 * q + 1] = v.y; xv[4 * q + 2] = v.z; xv[4 * q + 3] = v.w;
      }
    }
    xv[4 * RT_QUAD] = (t > 0) ? (float)actual : 0.0f;
    xv[4 * RT_QUAD + 1] = (float)streak;
    xv[4 * RT_QUAD + 2] = (float)(budget - (int32_t)used2);
    xv[4 * RT_QUAD + 3] = (float)__popc(hist2);
    double zb = 0.0, ze = 0.0;
#pragma unroll
    for (int k = 0; k < RO64_SLOTS; ++k) {
      asm volatile("" : "+v"(wb[k]), "+v"(we[k]));  // keep the coefficients f32 (see k_rollout64)
      const double xk = (double)xv[k];
      zb = fma(xk, (double)wb[k], zb);
      ze = fma(xk, (double)we[k], ze);
    }
    if (!(xv[30] > 0.5f)) ze = -__builtin_inf();
    const float r = reward_from_logits(zb, ze, actual);
    // tomorrow's network input: the observation columns of xv[] (zeros elsewhere and for lanes with no live env)
    mlp_wave_lds_sync();  // every lane's reads of the previous input are done
#pragma unroll
    for (int q = 0; q < ROWF / 4; ++q) {
      float4 v;
      v.x = (active && ((ma.obs_mask >> (4 * q)) & 1u)) ? xv[4 * q] : 0.0f;
      v.y = (active && ((ma.obs_mask >> (4 * q + 1)) & 1u)) ? xv[4 * q + 1] : 0.0f;
      v.z = (active && ((ma.obs_mask >> (4 * q + 2)) & 1u)) ? xv[4 * q + 2] : 0.0f;
      v.w = (active && ((ma.obs_mask >> (4 * q + 3)) & 1u)) ? xv[4 * q + 3] : 0.0f;
      reinterpret_cast<float4 *>(xrow)[q] = v;
    }
    const bool stepped = active;
    // wave-uniform: a row after this day is looked at -- inside the call, or past it when the caller bootstraps
    const bool look = s + 1 < a.n_steps || qa.bootstrap;
    bool more = false;    // the env holds a row after this day whose values enter: N_s is taken on it
    bool masked = false;  // no budget is left after this day: an alert on the next row is a no-op
    if (active) {
      const bool done = (t + 1 >= ndays);
      more = !done && look;
      masked = a.pol.require_budget && budget - (int32_t)used2 <= 0;
      used = used2; hist = hist2;
      if (!done) { streak = actual ? streak + 1 : 0; t = t + 1; }
      else active = false;
    }
    float n0 = 0.0f, n1 = 0.0f, t0 = 0.0f, t1 = 0.0f;  // Q(o_{s+1}, .) and Qt(o_{s+1}, .)
    if (look) {  // the row each env now holds, for tomorrow (or for the bootstrap)
      mlp_wave_lds_sync();
      mlp_heads2_groups<WIDTH, LAYERS>(ma, ma.params, g, xs, n0, n1);
      if (own) { t0 = n0; t1 = n1; }
      else mlp_heads2_groups<WIDTH, LAYERS>(ma, qa.tparams, g, xs, t0, t1);
    }
    if (stepped) {  // day s's record, now that the next row's four values are known
      const float qsa = actual ? q1 : q0;
      float nv = 0.0f;
      if (more) {
        if (masked) nv = t0;
        else if (qa.double_q) nv = n1 > n0 ? t1 : t0;
        else nv = fmaxf(t0, t1);
      }
      const double y = (double)r + qa.gamma * (double)nv;
      const double dl = y - (double)qsa;
      double c = dl, l = 0.5 * dl * dl;
      if (huber && fabs(dl) > qa.huber_delta) {
        c = dl > 0.0 ? qa.huber_delta : -qa.huber_delta;
        l = qa.huber_delta * (fabs(dl) - 0.5 * qa.huber_delta);
      }
      const size_t d = (size_t)s * n + slot;
      ga.day[d] = make_float2((float)((double)w_e * c), 0.0f);  // pass 2: c_s = day.x (1 - 0)
      ga.day_alert[d] = (uint8_t)actual;
      if (qa.v.advantage) qa.v.advantage[(size_t)s * n + e] = (float)dl;
      if (qa.td_target) qa.td_target[(size_t)s * n + e] = (float)y;
      loss += l;
      ret += (double)r;
      n_valid = s + 1;
    }
    q0 = n0;
    q1 = n1;
  }
  if (valid) {
    ga.total[slot] = 1.0;
    ga.n_valid[slot] = n_valid;
    qa.v.sq_error[e] = (float)loss;
    qa.v.days[e] = n_valid;
    qa.v.ret[e] = (float)ret;
  }
}

// ------------------------------------------------------------------------------------------------ pass 2
// k_pgm_pass2's text with the output row selected per env-day. The second head adds NT mlp_f4 accumulators and one
// float to the registers of the HEADS = 1 kernel (<64, 2>: 121 + 17). The compiler's figures: DESIGN.md.
#define PGM_PASS2_KERNEL k_qg_pass2
#define PGM_PASS2_HEADS 2
#include "w2a_policy_gradient_mlp_pass2.inc.h"
#undef PGM_PASS2_KERNEL
#undef PGM_PASS2_HEADS

template <int WIDTH, int LAYERS>
static void launch_qg(const QgMlpArgs &qa, unsigned grid1, hipStream_t s) {
  const MlpGradArgs &ga = qa.g;
  hipLaunchKernelGGL((k_qg_pass1<WIDTH, LAYERS>), dim3(grid1), dim3(BLOCK), 0, s, qa);
  hipLaunchKernelGGL(k_pgm_count, dim3(ga.n_chunks), dim3(64), 0, s, ga);
  hipLaunchKernelGGL(k_pgm_scan, dim3(1), dim3(1024), 0, s, ga);
  hipLaunchKernelGGL((k_qg_pass2<WIDTH, LAYERS>), dim3(ga.n_chunks), dim3(64), 0, s, ga);
  hipLaunchKernelGGL(k_pgm_reduce, dim3(ga.m.n_groups, (ga.m.stride + 255) / 256), dim3(256), 0, s, ga);
}

#endif  // W2A_QLEARN_HIP_H
