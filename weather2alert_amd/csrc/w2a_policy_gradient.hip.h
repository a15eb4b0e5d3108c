// w2a_policy_gradient.hip.h -- k_policy_gradient_linear: score-function gradient of a sampled linear policy's rollout
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_POLICY_GRADIENT_HIP_H
#define W2A_POLICY_GRADIENT_HIP_H

// ----------------------------------------------------------------------------------------
// reward-to-go REINFORCE gradient of w2a_rollout_linear(sample = 1) (w2a_policy_gradient_linear, estimator in w2a.h)
// ----------------------------------------------------------------------------------------
// The kernel runs BEFORE the rollout it differentiates, on the state and the observation rows that rollout will start
// from, and modifies neither: lane = env, the day loop of k_rollout_linear<SAMPLE> statement for statement (the same
// uniform, the same fp64 FMA chains -- bias first, slots 0..29 in slot order --, the same f32 sigmoids and
// reward_from_logits), so every u, z_s and r_s is the value the rollout then uses. It keeps no observation row:
//   pass 1  the rollout's days, plus the no-alert fork of the reward (it differs from the played day in slots 24..27
//           only: the baseline chain branches off the played one after slot 23), and per (call-day, lane) 9 B of scratch:
//           delta_s = m_s (a_s - sigmoid(z_s)), A_s = r_s - beta_s (both f32) and the alert issued; sum A in fp64.
//   pass 2  the env's days once more WITHOUT the three coefficient rows: o_s is the entry row (s = 0) or the table row of
//           the day before with its four run-time fields, rebuilt from the start state and the stored alerts; with the
//           total known Q_s = sum A - sum_{s' < s} A_s', and g += delta_s Q_s (o_s, 1) in fp64, one accumulator per slot.
// Registers: pass 1 lives on k_rollout_linear's budget (three coefficient rows + xv[]), pass 2 on 31 fp64 accumulators +
// xv[]; neither holds both, which a one-pass form (trace_s = sum delta_t o_t next to g) would have to.
struct PolicyGradArgs {
  LinearRolloutArgs l;   // as w2a_rollout_linear builds it (r.pol: require_budget and seed); l.obs is only read
  int32_t baseline;      // W2A_PG_BASELINE_*
  float2 *day;           // [n_steps][n] (delta_s, A_s) of the lane at visiting position `slot`
  uint8_t *day_alert;    // [n_steps][n] the alert issued on that call-day
  float *grad;           // [n_obs + 1][n] per-env gradient: observation column j of env e at j * n + e, bias last;
                         // LOOK: [n_obs + 1 + D][n], lookahead input k at row n_obs + k (k = 1..D, after the bias)
};

// GATE (w2a_policy_gradient_linear_gated): ga.l.gate restricts the attempts, as in k_rollout_linear<.., GATE>; a
// disallowed day is a forced choice, m_s = 0. GATE = false compiles from the statements it had before the gate existed.
// LOOK (w2a_lookahead_policy_gradient_linear; GATE when its nullable allowed_days is given): pass 1 continues the logit chain over the lookahead
// inputs as k_rollout_linear<.., LOOK> does; pass 2 rebuilds them for o_s from the series and keeps D more fp64
// accumulators. LOOK = false compiles from the statements it had before.
// NOISE (w2a_forecast_policy_gradient_linear; needs LOOK): both passes form the inputs with the forecast error of
// la.look.mae from the env's one stream, so pass 2 sees the inputs pass 1 and the rollout act on.
template <bool GATE, bool LOOK = false, bool NOISE = false>
__global__ __launch_bounds__(BLOCK, 2) void k_policy_gradient_linear(const PolicyGradArgs ga) {
  const LinearRolloutArgs &la = ga.l;
  const RolloutArgs &a = la.r;
  const int64_t slot64 = (int64_t)logical_block(blockIdx.x, gridDim.x >> 3) * BLOCK + threadIdx.x;
  if (slot64 >= a.n) return;
  const uint32_t slot = (uint32_t)slot64;
  const uint32_t e = a.order ? a.order[slot] : slot;  // the env this lane serves
  uint4 c2, hot;
  load_step_state(a.st, e, c2, hot);
  const uint4 cold = load_cold(a.st, e);
  const uint32_t t0 = D0_T(hot.x), used0 = D0_USED(hot.x), streak0 = D0_STREAK(hot.x), hist0 = D1_HIST(hot.y);
  const uint32_t ndays = D1_NDAYS(hot.y);
  const int32_t budget = (int32_t)hot.w;
  const uint32_t rows_per_day = (uint32_t)(a.tb.S_w * a.tb.Y);
  const uint32_t obs0 = e * (uint32_t)la.n_obs;
  const size_t n = (size_t)a.n;
  double total = 0.0;   // sum of A_s over the env's days of this call
  int32_t n_valid = 0;  // days the env steps in this call
  const float *lser = nullptr;
  if constexpr (LOOK) lser = look_series(la.look, cold.x);
  uint64_t estream = 0;
  if constexpr (NOISE) estream = look_noise_stream(la.look, (uint64_t)(a.gid0 + e), cold.w);
  // ---------------------------------------------------------------- pass 1: k_rollout_linear's days
  {
    const uint32_t wrow = W_COL(cold.y) * (uint32_t)a.tb.n_samples + W_SAMPLE(cold.y);
    float wb[32], we[32], wp[32];
    float lw[W2A_LOOK_MAX], lf[W2A_LOOK_MAX];
    {
      const float4 *wq = a.tb.W + (size_t)wrow * (2 * ROWF / 4);
      int32_t g = la.group ? la.group[e] : 0;
      g = g < 0 ? 0 : (g >= la.n_groups ? la.n_groups - 1 : g);
      const float4 *pq = la.weight + (size_t)g * (ROWF / 4);
#pragma unroll
      for (int q = 0; q < ROWF / 4; ++q) {
        const float4 b = wq[q], f = wq[ROWF / 4 + q], p = pq[q];
        wb[4 * q] = b.x; wb[4 * q + 1] = b.y; wb[4 * q + 2] = b.z; wb[4 * q + 3] = b.w;
        we[4 * q] = f.x; we[4 * q + 1] = f.y; we[4 * q + 2] = f.z; we[4 * q + 3] = f.w;
        wp[4 * q] = p.x; wp[4 * q + 1] = p.y; wp[4 * q + 2] = p.z; wp[4 * q + 3] = p.w;
      }
#pragma unroll
      for (int k = 0; k < 32; ++k) wp[k] = ((la.obs_mask >> k) & 1u) ? wp[k] : 0.0f;
      wp[31] = la.bias[g];
      if constexpr (LOOK) look_weights(la.look, g, lw);
    }
    const uint64_t pstream = rng_stream(a.pol.seed ^ 0xA5A5A5A55A5A5A5Aull, (uint64_t)(a.gid0 + e), cold.w);
    uint32_t t = t0, used = used0, streak = streak0, hist = hist0;
    // the no-alert fork: no alert from the call's first day on, so the budget stays at its start value, the streak is
    // the start state's on the first day and 0 after it, and the 14-day window only decays
    uint32_t streak_f = streak0, hist_f = hist0;
    bool active = D1_FIN(hot.y) == 0;
    uint32_t gate_word = 0, gate_idx = 0xFFFFFFFFu;
    double z = (double)wp[31];
    if (active) {
#pragma unroll
      for (int k = 0; k < RO64_SLOTS; ++k)
        if (la.slot_obs[k] >= 0) z = fma((double)la.obs[obs0 + la.slot_obs[k]], (double)wp[k], z);
      if constexpr (LOOK) {
        look_inputs<NOISE>(la.look, look_series_of<NOISE>(la.look, lser, cold.x), t > 0 ? t - 1 : 0u, ndays, lf, estream);
        z = look_logit(la.look, lf, lw, z);
      }
    }
    for (int s = 0; s < a.n_steps; ++s) {
      if (!__any(active)) break;
      const uint32_t u = (uint32_t)(w2a_mix64(pstream + (uint64_t)(t + 1) * 0x9E3779B97F4A7C15ull) >> 32);
      const float p = sigmoid_f32((float)z);
      int32_t act = ((float)u * 2.3283064365386963e-10f < p) ? 1 : 0;  // a_s: the policy's own draw
      float delta = (float)act - p;
      if (a.pol.require_budget && budget - (int32_t)used <= 0) { act = 0; delta = 0.0f; }  // m_s = 0: forced, off-policy
      if (GATE && active && !gate_allows(la.gate, la.gate_words, e, t, gate_word, gate_idx)) { act = 0; delta = 0.0f; }
      const uint32_t atb_s = ((int32_t)used == budget) ? 1u : 0u;
      const uint32_t actual = (act == 1 && atb_s) ? 0u : (uint32_t)act;
      const uint32_t used2 = used + actual;
      const uint32_t hist2 = ((hist << 1) | actual) & 0x3FFFu;
      const uint32_t hist_f2 = (hist_f << 1) & 0x3FFFu;
      const uint32_t day_row = t * rows_per_day + cold.x;
      float xv[32];
      {
        const float4 *xp = a.tb.X + (size_t)day_row * (ROWF / 4);
#pragma unroll
        for (int q = 0; q < ROWF / 4; ++q) {
          if (q == RT_QUAD) continue;
          const float4 v = xp[q];
          xv[4 * q] = v.x; xv[4 * q + 1] = v.y; xv[4 * q + 2] = v.z; xv[4 * q + 3] = v.w;
        }
      }
      xv[4 * RT_QUAD] = (t > 0) ? (float)actual : 0.0f;
      xv[4 * RT_QUAD + 1] = (float)streak;
      xv[4 * RT_QUAD + 2] = (float)(budget - (int32_t)used2);
      xv[4 * RT_QUAD + 3] = (float)__popc(hist2);
      const float xf[4] = {0.0f, (float)streak_f, (float)(budget - (int32_t)used0), (float)__popc(hist_f2)};
      double zb = 0.0, ze = 0.0, zp = (double)wp[31], zf = 0.0;
#pragma unroll
      for (int k = 0; k < RO64_SLOTS; ++k) {
        asm volatile("" : "+v"(wb[k]), "+v"(we[k]), "+v"(wp[k]));  // keep the coefficients f32 (see k_rollout64)
        if (k == 4 * RT_QUAD) zf = zb;  // the fork shares the prefix over slots 0..23
        const double xk = (double)xv[k];
        if (k >= 4 * RT_QUAD) zf = fma((k < 4 * RT_QUAD + 4) ? (double)xf[k - 4 * RT_QUAD] : xk, (double)wb[k], zf);
        zb = fma(xk, (double)wb[k], zb);
        ze = fma(xk, (double)we[k], ze);
        zp = fma(xk, (double)wp[k], zp);
      }
      if constexpr (LOOK) {
        look_inputs<NOISE>(la.look, look_series_of<NOISE>(la.look, lser, cold.x), t, ndays, lf, estream);
        zp = look_logit(la.look, lf, lw, zp);
      }
      if (!(xv[30] > 0.5f)) ze = -__builtin_inf();
      const float r = reward_from_logits(zb, ze, actual);
      // no alert issued: the effectiveness term is multiplied by 0, whatever its logit
      const float beta = ga.baseline == W2A_PG_BASELINE_NO_ALERT ? reward_from_logits(zf, -__builtin_inf(), 0u) : 0.0f;
      if (active) {
        const bool done = (t + 1 >= ndays);
        const float adv = r - beta;
        const size_t d = (size_t)s * n + slot;
        ga.day[d] = make_float2(delta, adv);
        ga.day_alert[d] = (uint8_t)actual;
        total += (double)adv;
        n_valid = s + 1;
        used = used2; hist = hist2; hist_f = hist_f2;
        if (!done) { streak = actual ? streak + 1 : 0; streak_f = 0; t = t + 1; }
        else active = false;
        z = zp;
      }
    }
  }
  // ---------------------------------------------------------------- pass 2: g = sum_s delta_s Q_s (o_s, 1)
  double g[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) g[k] = 0.0;  // slot k's column; the bias rides in slot 31, as in the policy row
  double prefix = 0.0;
  double gl[W2A_LOOK_MAX];  // LOOK: the lookahead inputs' columns
#pragma unroll
  for (int k = 0; k < W2A_LOOK_MAX; ++k) gl[k] = 0.0;
  if (n_valid > 0) {  // s = 0: the row the env holds on entry
    const float2 da = ga.day[slot];
    const double c = (double)da.x * total;
#pragma unroll
    for (int k = 0; k < RO64_SLOTS; ++k)
      if (la.slot_obs[k] >= 0) g[k] = c * (double)la.obs[obs0 + la.slot_obs[k]];
    g[31] = c;
    if constexpr (LOOK) {
      float lf[W2A_LOOK_MAX];
      look_inputs<NOISE>(la.look, look_series_of<NOISE>(la.look, lser, cold.x), t0 > 0 ? t0 - 1 : 0u, ndays, lf, estream);
#pragma unroll
      for (int k = 0; k < W2A_LOOK_MAX; ++k) gl[k] = c * (double)lf[k];
    }
    prefix = (double)da.y;
  }
  {
    uint32_t t = t0, used = used0, streak = streak0, hist = hist0;
    for (int s = 1; s < a.n_steps; ++s) {  // o_s = the vector of call-day s - 1
      const bool live = s < n_valid;
      if (!__any(live)) break;
      if (!live) continue;
      const size_t d = (size_t)s * n + slot;
      const float2 da = ga.day[d];
      const uint32_t actual = ga.day_alert[d - n];
      const double c = (double)da.x * (total - prefix);
      prefix += (double)da.y;
      used += actual;
      hist = ((hist << 1) | actual) & 0x3FFFu;
      const float4 *xp = a.tb.X + (size_t)(t * rows_per_day + cold.x) * (ROWF / 4);
#pragma unroll
      for (int q = 0; q < ROWF / 4; ++q) {
        if (q == RT_QUAD) continue;
        const float4 v = xp[q];
        g[4 * q] = fma(c, (double)v.x, g[4 * q]);
        g[4 * q + 1] = fma(c, (double)v.y, g[4 * q + 1]);
        if (q < GATE_QUAD) {  // slots 30 and 31 are no observation columns
          g[4 * q + 2] = fma(c, (double)v.z, g[4 * q + 2]);
          g[4 * q + 3] = fma(c, (double)v.w, g[4 * q + 3]);
        }
      }
      g[4 * RT_QUAD] = fma(c, (t > 0) ? (double)actual : 0.0, g[4 * RT_QUAD]);
      g[4 * RT_QUAD + 1] = fma(c, (double)streak, g[4 * RT_QUAD + 1]);
      g[4 * RT_QUAD + 2] = fma(c, (double)(budget - (int32_t)used), g[4 * RT_QUAD + 2]);
      g[4 * RT_QUAD + 3] = fma(c, (double)__popc(hist), g[4 * RT_QUAD + 3]);
      g[31] += c;
      if constexpr (LOOK) {  // o_s is day t's row
        float lf[W2A_LOOK_MAX];
        look_inputs<NOISE>(la.look, look_series_of<NOISE>(la.look, lser, cold.x), t, ndays, lf, estream);
#pragma unroll
        for (int k = 0; k < W2A_LOOK_MAX; ++k) gl[k] = fma(c, (double)lf[k], gl[k]);
      }
      streak = actual ? streak + 1 : 0;  // call-day s - 1 was not terminal: the env stepped again on call-day s
      t = t + 1;
    }
  }
  // column-major: a column's envs are contiguous (lane-consecutive stores in identity order, and the per-group
  // reduction that follows scans each column along memory)
  float *out = ga.grad + e;
#pragma unroll
  for (int k = 0; k < RO64_SLOTS; ++k)
    if (la.slot_obs[k] >= 0) out[(size_t)la.slot_obs[k] * n] = (float)g[k];
  out[(size_t)la.n_obs * n] = (float)g[31];
  if constexpr (LOOK) {
#pragma unroll
    for (int k = 0; k < W2A_LOOK_MAX; ++k)
      if (k < la.look.days) out[(size_t)(la.n_obs + 1 + k) * n] = (float)gl[k];
  }
}

#endif  // W2A_POLICY_GRADIENT_HIP_H
