// w2a_imitation.hip.h -- log-likelihood gradient of a GIVEN alert schedule (teacher forcing), linear and MLP policies
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_IMITATION_HIP_H
#define W2A_IMITATION_HIP_H

// ----------------------------------------------------------------------------------------
// supervised counterpart of the policy gradient (w2a_imitation_gradient_linear / _mlp, estimator in w2a.h)
// ----------------------------------------------------------------------------------------
// The env is forced along a per-env schedule (a bitmap by day of the episode) and the policy is evaluated on the rows
// it would have held. The estimator is REINFORCE's with two substitutions: the policy's draw a_s becomes the schedule's
// bit, and the reward-to-go Q_s becomes the env's constant weight w_e. So there are no reward chains, no coefficient
// rows and no no-alert fork; the kernels read the state, the tables, the schedule and the observation rows and write
// none of them.
//   k_imitation_linear  one pass, lane = env, no scratch: the logit of decision s + 1 is formed while the lane holds
//                       xv[] = o_{s+1} in registers (k_rollout_linear's third FMA chain, statement for statement), so
//                       c_{s+1} = w_e m (a* - sigmoid(z)) is known on the spot and g += c (o_{s+1}, 1) in fp64.
//   k_im_pass1          k_pgm_pass1's day loop with the action taken from the bitmap and the reward work removed. It
//                       leaves day = (f32(w_e delta_s), 0), the alert issued, total = 1 and n_valid, so that
//                       k_pgm_pass2's c_s = day.x (total - prefix) is exactly w_e delta_s (prefix sums day.y = 0): the
//                       count, scan, pass 2 and reduce kernels of w2a_policy_gradient_mlp.hip.h run unchanged.
// An optional weight per (call-day, env id) multiplies c_s (w2a_imitation_gradient_*_weighted: an advantage along a
// sampled rollout's schedule makes this the score-function gradient with a learned baseline); NULL is the unweighted
// computation bit for bit.
// No floating-point atomics: identical calls give identical bits.
struct ImitationArgs {
  const uint32_t *alert_mask;  // [n][mask_words] the schedule: bit (t & 31) of word t >> 5 = attempt an alert on day t
  int32_t mask_words;
  const float *env_weight;     // [n] w_e (nullable = 1)
  const float *day_weight;     // [n_steps][n] d_{s,e} by call-day and ENV ID (nullable = 1): c_s = w_e delta_s d_{s,e}
  float *loglik;               // [n] sum_s m_s log pi(a*_s | o_s)
  int32_t *days;               // [n] sum_s m_s
  const uint32_t *labels;      // [n][mask_words] the LABELS forms only (w2a_relabel_imitation_*): a*_s, while alert_mask
                               // still forces the env (DAgger: the learner's states, the expert's actions)
};

struct ImLinearArgs {
  LinearRolloutArgs l;   // as w2a_rollout_linear builds it (r.pol: require_budget only); l.obs is only read
  ImitationArgs im;
  float *grad;           // [n_obs + 1][n] per-env gradient: observation column j of env e at j * n + e, bias last;
                         // LOOK: [n_obs + 1 + D][n], lookahead input k at row n_obs + k (k = 1..D, after the bias)
};

struct ImMlpArgs {
  MlpGradArgs g;         // as w2a_policy_gradient_mlp builds it (baseline unused)
  ImitationArgs im;
};

// the schedule's bit of day t; the word is loaded once per 32 days
__device__ __forceinline__ uint32_t im_label_bits(const uint32_t *alert_mask, int32_t mask_words, uint32_t e, uint32_t t,
                                                  uint32_t &word, uint32_t &idx) {
  const uint32_t wi = t >> 5;
  if (wi != idx) {
    idx = wi;
    word = wi < (uint32_t)mask_words ? alert_mask[(size_t)e * mask_words + wi] : 0u;
  }
  return (word >> (t & 31)) & 1u;
}

__device__ __forceinline__ uint32_t im_label(const ImitationArgs &im, uint32_t e, uint32_t t, uint32_t &word,
                                             uint32_t &idx) {
  return im_label_bits(im.alert_mask, im.mask_words, e, t, word, idx);
}

// a*_s of the decision of day t: the schedule's own bit `lab`, or with LABELS the bit of im.labels (its word cached apart)
template <bool LABELS>
__device__ __forceinline__ uint32_t im_target(const ImitationArgs &im, uint32_t e, uint32_t t, uint32_t lab,
                                              uint32_t &word, uint32_t &idx) {
  if constexpr (LABELS) return im_label_bits(im.labels, im.mask_words, e, t, word, idx);
  else return lab;
}

// c_s = w_e delta_s, times the day's weight where the caller gave one (the products are fp64)
__device__ __forceinline__ double im_coef(const ImitationArgs &im, double w_e, float delta, size_t day_env) {
  const double c = w_e * (double)delta;
  return im.day_weight ? c * (double)im.day_weight[day_env] : c;
}

// log pi(a | z) of the Bernoulli policy pi(1) = sigmoid(z): -softplus(-z) for a = 1, -softplus(z) for a = 0, stable
__device__ __forceinline__ double im_log_pi(double z, uint32_t a) {
  const double x = a ? -z : z;
  return -(fmax(x, 0.0) + log1p(exp(-fabs(x))));
}

// Registers: the policy row (32 f32), xv[] and 31 fp64 accumulators; two waves per SIMD leave 256 VGPRs.
// GATE (w2a_imitation_gradient_linear_gated): ia.l.gate restricts the attempts; an alert the schedule asks for on a
// disallowed day is attempted as 0 and the day is not scored. GATE = false compiles from the statements it had before.
// LOOK (w2a_lookahead_imitation_gradient_linear; GATE when its nullable allowed_days is given): the logit chain goes on over the lookahead inputs of
// the held row's day, as k_rollout_linear<.., LOOK>, and D more fp64 accumulators take c f_k. LOOK = false compiles
// from the statements it had before.
// LABELS (w2a_relabel_imitation_linear): the schedule still forces the env and decides m_s; delta_s and the
// log-likelihood take a*_s from ia.im.labels. LABELS = false scores the schedule's own bit, as before.
// NOISE (w2a_forecast_imitation_gradient_linear; needs LOOK, no LABELS form): the inputs carry the forecast error of
// la.look.mae, as k_rollout_linear<.., NOISE> forms them.
template <bool GATE, bool LOOK = false, bool LABELS = false, bool NOISE = false>
__global__ __launch_bounds__(BLOCK, 2) void k_imitation_linear(const ImLinearArgs ia) {
  const LinearRolloutArgs &la = ia.l;
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
  float lw[W2A_LOOK_MAX], lf[W2A_LOOK_MAX];
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
    if constexpr (LOOK) look_weights(la.look, g, lw);
  }
  const float *lser = nullptr;
  if constexpr (LOOK) lser = look_series(la.look, cold.x);
  uint64_t estream = 0;
  if constexpr (NOISE) estream = look_noise_stream(la.look, (uint64_t)(a.gid0 + e), cold.w);
  double gl[W2A_LOOK_MAX];  // LOOK: the lookahead inputs' columns
#pragma unroll
  for (int k = 0; k < W2A_LOOK_MAX; ++k) gl[k] = 0.0;
  const double w_e = ia.im.env_weight ? (double)ia.im.env_weight[e] : 1.0;
  uint32_t lab_word = 0, lab_idx = 0xFFFFFFFFu;
  uint32_t tgt_word = 0, tgt_idx = 0xFFFFFFFFu;
  uint32_t gate_word = 0, gate_idx = 0xFFFFFFFFu;
  double g[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) g[k] = 0.0;  // slot k's column; the bias rides in slot 31, as in the policy row
  double ll = 0.0;
  int32_t scored = 0;
  bool active = D1_FIN(hot.y) == 0;
  // decision 0: the logit of the observation row the agent holds, and its term of the gradient
  uint32_t lab = 0;      // a*_s of the decision at hand
  bool scores = false;   // m_s of the decision at hand
  if (active) {
    double z = (double)wp[31];
#pragma unroll
    for (int k = 0; k < RO64_SLOTS; ++k)
      if (la.slot_obs[k] >= 0) z = fma((double)la.obs[obs0 + la.slot_obs[k]], (double)wp[k], z);
    if constexpr (LOOK) {
      look_inputs<NOISE>(la.look, look_series_of<NOISE>(la.look, lser, cold.x), t > 0 ? t - 1 : 0u, ndays, lf, estream);
      z = look_logit(la.look, lf, lw, z);
    }
    lab = im_label(ia.im, e, t, lab_word, lab_idx);
    scores = !(a.pol.require_budget && budget - (int32_t)used <= 0);
    if (GATE && !gate_allows(la.gate, la.gate_words, e, t, gate_word, gate_idx)) scores = false;
    if (scores) {
      const uint32_t tgt = im_target<LABELS>(ia.im, e, t, lab, tgt_word, tgt_idx);
      const float delta = (float)tgt - sigmoid_f32((float)z);
      const double c = im_coef(ia.im, w_e, delta, e);
#pragma unroll
      for (int k = 0; k < RO64_SLOTS; ++k)
        if (la.slot_obs[k] >= 0) g[k] = c * (double)la.obs[obs0 + la.slot_obs[k]];
      g[31] = c;
      if constexpr (LOOK) {
#pragma unroll
        for (int k = 0; k < W2A_LOOK_MAX; ++k) gl[k] = c * (double)lf[k];
      }
      ll = im_log_pi(z, tgt);
      scored = 1;
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
    for (int k = 0; k < RO64_SLOTS; ++k) {
      asm volatile("" : "+v"(wp[k]));  // keep the coefficients f32 (see k_rollout64)
      zp = fma((double)xv[k], (double)wp[k], zp);
    }
    if constexpr (LOOK) {  // xv[] is day t's row
      look_inputs<NOISE>(la.look, look_series_of<NOISE>(la.look, lser, cold.x), t, ndays, lf, estream);
      zp = look_logit(la.look, lf, lw, zp);
    }
    if (active) {
      const bool done = (t + 1 >= ndays);
      used = used2; hist = hist2;
      if (!done) { streak = actual ? streak + 1 : 0; t = t + 1; }
      else active = false;
      // decision s + 1, on the row the lane holds right now
      if (active && s + 1 < a.n_steps) {
        lab = im_label(ia.im, e, t, lab_word, lab_idx);
        scores = !(a.pol.require_budget && budget - (int32_t)used <= 0);
        if (GATE && !gate_allows(la.gate, la.gate_words, e, t, gate_word, gate_idx)) scores = false;
        if (scores) {
          const uint32_t tgt = im_target<LABELS>(ia.im, e, t, lab, tgt_word, tgt_idx);
          const float delta = (float)tgt - sigmoid_f32((float)zp);
          const double c = im_coef(ia.im, w_e, delta, (size_t)(s + 1) * n + e);
#pragma unroll
          for (int k = 0; k < RO64_SLOTS; ++k)
            if (la.slot_obs[k] >= 0) g[k] = fma(c, (double)xv[k], g[k]);
          g[31] += c;
          if constexpr (LOOK) {
#pragma unroll
            for (int k = 0; k < W2A_LOOK_MAX; ++k) gl[k] = fma(c, (double)lf[k], gl[k]);
          }
          ll += im_log_pi(zp, tgt);
          scored += 1;
        }
      }
    }
  }
  // column-major, as k_policy_gradient_linear: a column's envs are contiguous
  float *out = ia.grad + e;
#pragma unroll
  for (int k = 0; k < RO64_SLOTS; ++k)
    if (la.slot_obs[k] >= 0) out[(size_t)la.slot_obs[k] * n] = (float)g[k];
  out[(size_t)la.n_obs * n] = (float)g[31];
  if constexpr (LOOK) {
#pragma unroll
    for (int k = 0; k < W2A_LOOK_MAX; ++k)
      if (k < la.look.days) out[(size_t)(la.n_obs + 1 + k) * n] = (float)gl[k];
  }
  ia.im.loglik[e] = (float)ll;
  ia.im.days[e] = scored;
}

// ------------------------------------------------------------------------------------------------ MLP: pass 1
// GATE (w2a_imitation_gradient_mlp_gated): as k_imitation_linear<GATE>; GATE = false compiles from the statements it
// had before the gate existed. LABELS (w2a_relabel_imitation_mlp): as k_imitation_linear<.., LABELS>
template <int WIDTH, int LAYERS, bool GATE, bool LABELS = false>
__global__ __launch_bounds__(BLOCK, 2) void k_im_pass1(const ImMlpArgs ia) {
  __shared__ __attribute__((aligned(16))) float s_x[MLP_WAVES][64 * MLP_XS];
  const MlpGradArgs &ga = ia.g;
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
  const double w_e = ia.im.env_weight ? (double)ia.im.env_weight[e] : 1.0;
  uint32_t lab_word = 0, lab_idx = 0xFFFFFFFFu;
  uint32_t tgt_word = 0, tgt_idx = 0xFFFFFFFFu;
  double ll = 0.0;
  int32_t scored = 0, n_valid = 0;
  uint32_t gate_word = 0, gate_idx = 0xFFFFFFFFu;
  bool active = D1_FIN(hot.y) == 0 && valid;
#pragma unroll
  for (int k = 0; k < ROWF; ++k)
    xrow[k] = (k < RO64_SLOTS && ma.slot_obs[k] >= 0 && active) ? ma.obs[obs0 + ma.slot_obs[k]] : 0.0f;
  mlp_wave_lds_sync();
  float z = mlp_logit_groups<WIDTH, LAYERS>(ma, g, xs);
  for (int s = 0; s < a.n_steps; ++s) {
    if (!__any(active)) break;
    const uint32_t lab = active ? im_label(ia.im, e, t, lab_word, lab_idx) : 0u;  // a*_s: the schedule's bit
    const float p = sigmoid_f32(z);
    int32_t act = (int32_t)lab;
    const uint32_t tgt = active ? im_target<LABELS>(ia.im, e, t, lab, tgt_word, tgt_idx) : 0u;  // a*_s
    float delta = (float)(LABELS ? (int32_t)tgt : act) - p;
    bool scores = true;
    if (a.pol.require_budget && budget - (int32_t)used <= 0) { act = 0; delta = 0.0f; scores = false; }  // m_s = 0: forced
    if (GATE && active && !gate_allows(ma.gate, ma.gate_words, e, t, gate_word, gate_idx)) { act = 0; delta = 0.0f; scores = false; }
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
      ga.day[d] = make_float2((float)im_coef(ia.im, w_e, delta, (size_t)s * n + e), 0.0f);  // pass 2: c_s = day.x (1 - 0)
      ga.day_alert[d] = (uint8_t)actual;
      if (scores) { ll += im_log_pi((double)z, tgt); scored += 1; }
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
    ia.im.loglik[e] = (float)ll;
    ia.im.days[e] = scored;
  }
}

template <int WIDTH, int LAYERS>
static void launch_im(const ImMlpArgs &ia, unsigned grid1, hipStream_t s) {
  const MlpGradArgs &ga = ia.g;
  if (ia.im.labels && ga.m.gate) hipLaunchKernelGGL((k_im_pass1<WIDTH, LAYERS, true, true>), dim3(grid1), dim3(BLOCK), 0, s, ia);
  else if (ia.im.labels) hipLaunchKernelGGL((k_im_pass1<WIDTH, LAYERS, false, true>), dim3(grid1), dim3(BLOCK), 0, s, ia);
  else if (ga.m.gate) hipLaunchKernelGGL((k_im_pass1<WIDTH, LAYERS, true>), dim3(grid1), dim3(BLOCK), 0, s, ia);
  else hipLaunchKernelGGL((k_im_pass1<WIDTH, LAYERS, false>), dim3(grid1), dim3(BLOCK), 0, s, ia);
  hipLaunchKernelGGL(k_pgm_count, dim3(ga.n_chunks), dim3(64), 0, s, ga);
  hipLaunchKernelGGL(k_pgm_scan, dim3(1), dim3(1024), 0, s, ga);
  hipLaunchKernelGGL((k_pgm_pass2<WIDTH, LAYERS>), dim3(ga.n_chunks), dim3(64), 0, s, ga);
  hipLaunchKernelGGL(k_pgm_reduce, dim3(ga.m.n_groups, (ga.m.stride + 255) / 256), dim3(256), 0, s, ga);
}

#endif  // W2A_IMITATION_HIP_H
