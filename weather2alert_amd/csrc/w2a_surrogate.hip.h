// w2a_surrogate.hip.h -- gradient of the PPO-clip surrogate along a GIVEN alert schedule, linear and MLP policies
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_SURROGATE_HIP_H
#define W2A_SURROGATE_HIP_H

// ----------------------------------------------------------------------------------------
// K epochs on the same episodes (w2a_surrogate_gradient_linear / _mlp, estimator in w2a.h)
// ----------------------------------------------------------------------------------------
// The env is forced along its schedule exactly as in w2a_imitation.hip.h: the same bitmap, the same
// attempted-versus-issued rule, the same rows, the same m_s. What changes is the coefficient of dz_s/dtheta:
//   c_s = w_e (live_s rho_s A_s delta_s + beta dH_s/dz),   rho_s = exp(lp_s - old_log_prob[s, e]),
//   live_s = !((A_s > 0 && rho_s > 1 + clip) || (A_s < 0 && rho_s < 1 - clip))
// -- the gradient of min(rho A, clamp(rho, 1 - clip, 1 + clip) A) plus an entropy bonus. With old_log_prob = NULL (rho = 1)
// and beta = 0 this is the weighted imitation coefficient w_e delta_s A_s.
//   k_surrogate_linear  k_imitation_linear's shape: one pass, lane = env, no scratch, 31 fp64 accumulators
//   k_sg_pass1          k_im_pass1's day loop; leaves day = (f32(c_s), 0), the alert issued, total = 1 and n_valid, so
//                       the count, scan, pass 2 and reduce kernels of w2a_policy_gradient_mlp.hip.h run unchanged
// Every per-day scalar past delta_s (lp, rho, the clip test, the entropy and its derivative, the sums) is fp64.
// No floating-point atomics: identical calls give identical bits.
struct SurrogateArgs {
  const uint32_t *alert_mask;  // [n][mask_words] the schedule, as ImitationArgs
  int32_t mask_words;
  const float *env_weight;     // [n] w_e (nullable = 1)
  const float *advantage;      // [>= n_steps][n] A_s by call-day and ENV ID
  const float *old_log_prob;   // [>= n_steps][n] log pi_old(a_s | o_s), same layout (nullable: rho = 1)
  double lo, hi;               // 1 - clip, 1 + clip
  double beta;                 // entropy coefficient
  float *log_prob;             // [n_steps][n] lp_s on scored days (nullable; zero-filled by the entry point)
  float *surrogate;            // [n] L_e
  int32_t *clipped;            // [n] scored days with live_s = 0
  float *approx_kl;            // [n] sum_s (rho_s - 1) - log rho_s
  float *entropy;              // [n] sum_s H_s
  int32_t *days;               // [n] sum_s m_s
};

struct SgLinearArgs {
  LinearRolloutArgs l;   // as w2a_rollout_linear builds it (r.pol: require_budget only); l.obs is only read
  SurrogateArgs sg;
  float *grad;           // [n_obs + 1][n] per-env gradient, column-major as ImLinearArgs
};

struct SgMlpArgs {
  MlpGradArgs g;         // as w2a_policy_gradient_mlp builds it (baseline unused)
  SurrogateArgs sg;
};

// the per-env sums of a call
struct SgSums {
  double L, kl, H;
  int32_t clipped, scored;
};

// One scored day: returns c_s and adds the day's terms to the per-env sums. z is the logit as the kernel holds it (the
// fp64 chain, or the f32 network's widened), delta = a - sigmoid_f32(z) as the imitation kernels form it.
__device__ __forceinline__ double sg_day(const SurrogateArgs &sg, double w_e, double z, float delta, uint32_t a,
                                         size_t day_env, SgSums &sum) {
  const double lp = im_log_pi(z, a);
  // p and 1 - p without cancellation, from the exponential im_log_pi takes: e = exp(-|z|)
  const double e = exp(-fabs(z));
  const double r = 1.0 / (1.0 + e);
  const double p = z >= 0.0 ? r : e * r, q = z >= 0.0 ? e * r : r;
  const double lp_other = a ? lp - z : lp + z;  // log pi of the action not taken: log sigmoid(z) - log sigmoid(-z) = z
  const double A = (double)sg.advantage[day_env];
  double rho = 1.0, d = 0.0;
  if (sg.old_log_prob) {
    d = lp - (double)sg.old_log_prob[day_env];
    rho = exp(d);
  }
  const bool live = !((A > 0.0 && rho > sg.hi) || (A < 0.0 && rho < sg.lo));
  const double rA = rho * A;
  sum.L += fmin(rA, fmin(fmax(rho, sg.lo), sg.hi) * A);
  sum.kl += (rho - 1.0) - d;
  sum.H -= a ? p * lp + q * lp_other : q * lp + p * lp_other;
  sum.clipped += live ? 0 : 1;
  sum.scored += 1;
  if (sg.log_prob) sg.log_prob[day_env] = (float)lp;
  double c = live ? (w_e * (double)delta) * rA : 0.0;
  if (sg.beta != 0.0) c += w_e * (sg.beta * (-z * p * q));  // beta dH/dz
  return c;
}

// Registers: as k_imitation_linear (the policy row, xv[] and 31 fp64 accumulators) plus the three fp64 sums and the
// temporaries of the fp64 exponentials; at two waves per SIMD it spills (DESIGN.md has the figures).
// GATE (w2a_surrogate_gradient_linear_gated): sa.l.gate restricts the attempts, as in k_imitation_linear<GATE>: a
// disallowed day is attempted as 0 and adds nothing to any sum. GATE = false compiles from the statements it had before.
template <bool GATE>
__global__ __launch_bounds__(BLOCK, 2) void k_surrogate_linear(const SgLinearArgs sa) {
  const LinearRolloutArgs &la = sa.l;
  const RolloutArgs &a = la.r;
  const int64_t slot64 = (int64_t)logical_block(blockIdx.x, gridDim.x >> 3) * BLOCK + threadIdx.x;
  if (slot64 >= a.n) return;
  const uint32_t slot = (uint32_t)slot64;
  const uint32_t e = a.order ? a.order[slot] : slot;  // the env this lane serves
  uint4 c2, hot;
  load_step_state(a.st, e, c2, hot);
  const uint4 cold = load_cold(a.st, e);
  uint32_t t = D0_T(hot.x), used = D0_USED(hot.x), streak = D0_STREAK(hot.x), hist = D1_HIST(hot.y);
  const uint32_t ndays = D1_NDAYS(hot.y);
  const int32_t budget = (int32_t)hot.w;
  const uint32_t rows_per_day = (uint32_t)(a.tb.S_w * a.tb.Y);
  const uint32_t obs0 = e * (uint32_t)la.n_obs;
  const size_t n = (size_t)a.n;
  float wp[32];
  {
    int32_t g = la.group ? la.group[e] : 0;
    g = g < 0 ? 0 : (g >= la.n_groups ? la.n_groups - 1 : g);
    const float4 *pq = la.weight + (size_t)g * (ROWF / 4);
#pragma unroll
    for (int q = 0; q < ROWF / 4; ++q) {
      const float4 p = pq[q];
      wp[4 * q] = p.x; wp[4 * q + 1] = p.y; wp[4 * q + 2] = p.z; wp[4 * q + 3] = p.w;
    }
#pragma unroll
    for (int k = 0; k < 32; ++k) wp[k] = ((la.obs_mask >> k) & 1u) ? wp[k] : 0.0f;
    wp[31] = la.bias[g];  // the bias rides in slot 31, as in k_rollout_linear
  }
  const double w_e = sa.sg.env_weight ? (double)sa.sg.env_weight[e] : 1.0;
  uint32_t lab_word = 0, lab_idx = 0xFFFFFFFFu;
  uint32_t gate_word = 0, gate_idx = 0xFFFFFFFFu;
  double g[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) g[k] = 0.0;  // slot k's column; the bias rides in slot 31, as in the policy row
  SgSums sum = {0.0, 0.0, 0.0, 0, 0};
  bool active = D1_FIN(hot.y) == 0;
  // decision 0: the logit of the observation row the agent holds, and its term of the gradient
  uint32_t lab = 0;      // a_s of the decision at hand
  bool scores = false;   // m_s of the decision at hand
  if (active) {
    double z = (double)wp[31];
#pragma unroll
    for (int k = 0; k < RO64_SLOTS; ++k)
      if (la.slot_obs[k] >= 0) z = fma((double)la.obs[obs0 + la.slot_obs[k]], (double)wp[k], z);
    lab = im_label_bits(sa.sg.alert_mask, sa.sg.mask_words, e, t, lab_word, lab_idx);
    scores = !(a.pol.require_budget && budget - (int32_t)used <= 0);
    if (GATE && !gate_allows(la.gate, la.gate_words, e, t, gate_word, gate_idx)) scores = false;
    if (scores) {
      const float delta = (float)lab - sigmoid_f32((float)z);
      const double c = sg_day(sa.sg, w_e, z, delta, lab, e, sum);
#pragma unroll
      for (int k = 0; k < RO64_SLOTS; ++k)
        if (la.slot_obs[k] >= 0) g[k] = c * (double)la.obs[obs0 + la.slot_obs[k]];
      g[31] = c;
    }
  }
  for (int s = 0; s < a.n_steps; ++s) {
    if (!__any(active)) break;
    // ---- the schedule's action; require_budget forces it to 0 with no budget left (m_s = 0, scored above as such)
    const int32_t act = scores ? (int32_t)lab : 0;
    // ---- env.py:242-250
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
    double zp = (double)wp[31];
#pragma unroll
    for (int k = 0; k < RO64_SLOTS; ++k) zp = fma((double)xv[k], (double)wp[k], zp);
    if (active) {
      const bool done = (t + 1 >= ndays);
      used = used2; hist = hist2;
      if (!done) { streak = actual ? streak + 1 : 0; t = t + 1; }
      else active = false;
      // decision s + 1, on the row the lane holds right now
      if (active && s + 1 < a.n_steps) {
        lab = im_label_bits(sa.sg.alert_mask, sa.sg.mask_words, e, t, lab_word, lab_idx);
        scores = !(a.pol.require_budget && budget - (int32_t)used <= 0);
        if (GATE && !gate_allows(la.gate, la.gate_words, e, t, gate_word, gate_idx)) scores = false;
        if (scores) {
          const float delta = (float)lab - sigmoid_f32((float)zp);
          const double c = sg_day(sa.sg, w_e, zp, delta, lab, (size_t)(s + 1) * n + e, sum);
#pragma unroll
          for (int k = 0; k < RO64_SLOTS; ++k)
            if (la.slot_obs[k] >= 0) g[k] = fma(c, (double)xv[k], g[k]);
          g[31] += c;
        }
      }
    }
  }
  // column-major, as k_policy_gradient_linear: a column's envs are contiguous
  float *out = sa.grad + e;
#pragma unroll
  for (int k = 0; k < RO64_SLOTS; ++k)
    if (la.slot_obs[k] >= 0) out[(size_t)la.slot_obs[k] * n] = (float)g[k];
  out[(size_t)la.n_obs * n] = (float)g[31];
  sa.sg.surrogate[e] = (float)sum.L;
  sa.sg.clipped[e] = sum.clipped;
  sa.sg.approx_kl[e] = (float)sum.kl;
  sa.sg.entropy[e] = (float)sum.H;
  sa.sg.days[e] = sum.scored;
}

// ------------------------------------------------------------------------------------------------ MLP: pass 1
// GATE (w2a_surrogate_gradient_mlp_gated): as k_surrogate_linear<GATE>; GATE = false compiles from the statements it
// had before the gate existed
template <int WIDTH, int LAYERS, bool GATE>
__global__ __launch_bounds__(BLOCK, 2) void k_sg_pass1(const SgMlpArgs sa) {
  __shared__ __attribute__((aligned(16))) float s_x[MLP_WAVES][64 * MLP_XS];
  const MlpGradArgs &ga = sa.g;
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
  const int32_t g = pgm_group(ma, e);
  const uint32_t obs0 = e * (uint32_t)ma.n_obs;
  const size_t n = (size_t)a.n;
  const double w_e = sa.sg.env_weight ? (double)sa.sg.env_weight[e] : 1.0;
  uint32_t lab_word = 0, lab_idx = 0xFFFFFFFFu;
  uint32_t gate_word = 0, gate_idx = 0xFFFFFFFFu;
  SgSums sum = {0.0, 0.0, 0.0, 0, 0};
  int32_t n_valid = 0;
  bool active = D1_FIN(hot.y) == 0 && valid;
#pragma unroll
  for (int k = 0; k < ROWF; ++k)
    xrow[k] = (k < RO64_SLOTS && ma.slot_obs[k] >= 0 && active) ? ma.obs[obs0 + ma.slot_obs[k]] : 0.0f;
  mlp_wave_lds_sync();
  float z = mlp_logit_groups<WIDTH, LAYERS>(ma, g, xs);
  for (int s = 0; s < a.n_steps; ++s) {
    if (!__any(active)) break;
    const uint32_t lab = active ? im_label_bits(sa.sg.alert_mask, sa.sg.mask_words, e, t, lab_word, lab_idx) : 0u;
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
        const float4 v = xp[q];
        xv[4 * q] = v.x; xv[4 * q + 1] = v.y; xv[4 * q + 2] = v.z; xv[4 * q + 3] = v.w;
      }
    }
    xv[4 * RT_QUAD] = (t > 0) ? (float)actual : 0.0f;
    xv[4 * RT_QUAD + 1] = (float)streak;
    xv[4 * RT_QUAD + 2] = (float)(budget - (int32_t)used2);
    xv[4 * RT_QUAD + 3] = (float)__popc(hist2);
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
    if (active) {
      const bool done = (t + 1 >= ndays);
      const size_t d = (size_t)s * n + slot;
      const double c = scores ? sg_day(sa.sg, w_e, (double)z, delta, lab, (size_t)s * n + e, sum) : 0.0;
      ga.day[d] = make_float2((float)c, 0.0f);  // pass 2: c_s = day.x (1 - 0)
      ga.day_alert[d] = (uint8_t)actual;
      n_valid = s + 1;
      used = used2; hist = hist2;
      if (!done) { streak = actual ? streak + 1 : 0; t = t + 1; }
      else active = false;
    }
    if (s + 1 < a.n_steps) {  // wave-uniform: the logit of the row each env now holds, for tomorrow
      mlp_wave_lds_sync();
      z = mlp_logit_groups<WIDTH, LAYERS>(ma, g, xs);
    }
  }
  if (valid) {
    ga.total[slot] = 1.0;
    ga.n_valid[slot] = n_valid;
    sa.sg.surrogate[e] = (float)sum.L;
    sa.sg.clipped[e] = sum.clipped;
    sa.sg.approx_kl[e] = (float)sum.kl;
    sa.sg.entropy[e] = (float)sum.H;
    sa.sg.days[e] = sum.scored;
  }
}

template <int WIDTH, int LAYERS>
static void launch_sg(const SgMlpArgs &sa, unsigned grid1, hipStream_t s) {
  const MlpGradArgs &ga = sa.g;
  if (ga.m.gate) hipLaunchKernelGGL((k_sg_pass1<WIDTH, LAYERS, true>), dim3(grid1), dim3(BLOCK), 0, s, sa);
  else hipLaunchKernelGGL((k_sg_pass1<WIDTH, LAYERS, false>), dim3(grid1), dim3(BLOCK), 0, s, sa);
  hipLaunchKernelGGL(k_pgm_count, dim3(ga.n_chunks), dim3(64), 0, s, ga);
  hipLaunchKernelGGL(k_pgm_scan, dim3(1), dim3(1024), 0, s, ga);
  hipLaunchKernelGGL((k_pgm_pass2<WIDTH, LAYERS>), dim3(ga.n_chunks), dim3(64), 0, s, ga);
  hipLaunchKernelGGL(k_pgm_reduce, dim3(ga.m.n_groups, (ga.m.stride + 255) / 256), dim3(256), 0, s, ga);
}

#endif  // W2A_SURROGATE_HIP_H
