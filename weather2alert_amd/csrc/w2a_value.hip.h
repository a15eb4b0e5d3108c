// w2a_value.hip.h -- gradient of a state-value regression along GIVEN alert schedules (critic fit), linear and MLP
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_VALUE_HIP_H
#define W2A_VALUE_HIP_H

// ----------------------------------------------------------------------------------------
// least-squares fit of V_theta(o) = z(o) to the reward-to-go (w2a_value_gradient_linear / _mlp, estimator in w2a.h)
// ----------------------------------------------------------------------------------------
// The env is forced along a per-env schedule as in w2a_imitation.hip.h (im_label), the day's reward is formed by the
// statements of the rollout kernels, and the network's raw logit is read as the value of the row it was formed on. The
// per-day coefficient of the gradient is the residual Q_s - V_s, which telescopes over the one-step residuals
//     y_s = r_s + V_{s+1} - V_s   (V := 0 past the env's last stepped day of the call),
//     sum_{s' >= s} y_s' = Q_s - V_s,   so with total = sum_s y_s:   Q_s - V_s = total - sum_{s' < s} y_s'
// -- the form c_s = day.x (total - prefix of day.y) that the second passes of the policy-gradient kernels already take.
//   k_value_gradient_linear  k_policy_gradient_linear's two passes: pass 1 is k_rollout_linear's day loop with the action
//                       taken from the bitmap (three fp64 chains: both reward logits and the value of the row the env
//                       will hold tomorrow); per (call-day, lane) 8 B of scratch, y_s in fp64 (nothing is rounded before
//                       the residual is), and 1 B, the alert issued. Pass 2 walks the days again without the coefficient
//                       rows and adds w_e (total - prefix) (o_s, 1) into 31 fp64 accumulators; it knows Q_s - V_s on
//                       every day, so the squared error and the optional advantage rows are written there.
//   k_vg_pass1          k_pgm_pass1's day loop with the action from the bitmap, the reward chains kept and the no-alert
//                       fork removed. V_{s+1} is the logit the loop forms at the end of iteration s for tomorrow's
//                       decision anyway, so day s's record is written after it: day = (f32(w_e), f32(y_s)), the alert
//                       issued, total = the fp64 sum of the ROUNDED y_s (so that total - prefix is exactly the sum of the
//                       stored residuals of the days still to come) and n_valid. The count, scan, pass 2 and reduce
//                       kernels of w2a_policy_gradient_mlp.hip.h run unchanged.
//   k_vg_finish         lane = visiting position: one more walk over the lane's column of day.y for sum (Q_s - V_s)^2
//                       and, when asked for, the advantage rows f32(total - prefix) at [call-day][env id].
// No floating-point atomics: identical calls give identical bits.
struct ValueArgs {
  const uint32_t *alert_mask;  // [n][mask_words] the schedule, as ImitationArgs
  int32_t mask_words;
  const float *env_weight;     // [n] w_e (nullable = 1)
  float *sq_error;             // [n] sum_s (Q_s - V_s)^2
  int32_t *days;               // [n] S_e: days stepped in this call
  float *ret;                  // [n] Q_0 = sum_s r_s
  float *advantage;            // [n_steps][n] Q_s - V_s by call-day and ENV ID (nullable); zero-filled before the launch
};

struct VgLinearArgs {
  LinearRolloutArgs l;   // as w2a_rollout_linear builds it; l.obs is only read
  ValueArgs v;
  double *day_y;         // [n_steps][n] y_s of the lane at visiting position `slot`
  uint8_t *day_alert;    // [n_steps][n] the alert issued on that call-day
  float *grad;           // [n_obs + 1][n] per-env gradient: observation column j of env e at j * n + e, bias last
};

struct VgMlpArgs {
  MlpGradArgs g;         // as w2a_policy_gradient_mlp builds it (baseline unused)
  ValueArgs v;
};

// Registers: pass 1 holds three coefficient rows and xv[] (k_policy_gradient_linear's pass 1 less the fork), pass 2
// xv[]-free table quads and 31 fp64 accumulators. The one-pass form (g += y_s * running sum of (o_s', 1)) would hold 62
// fp64 accumulators next to the three rows: 124 + 96 + 32 registers before any address or state, over the 256 that two
// waves per SIMD leave. The compiler's figures: DESIGN.md.
__global__ __launch_bounds__(BLOCK, 2) void k_value_gradient_linear(const VgLinearArgs va) {
  const LinearRolloutArgs &la = va.l;
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
  double total = 0.0;   // sum of y_s over the env's days of this call = Q_0 - V_0
  double ret = 0.0;     // sum of r_s = Q_0
  int32_t n_valid = 0;  // days the env steps in this call
  // ---------------------------------------------------------------- pass 1: the schedule's days, rewards and values
  {
    const uint32_t wrow = W_COL(cold.y) * (uint32_t)a.tb.n_samples + W_SAMPLE(cold.y);
    float wb[32], we[32], wp[32];
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
    }
    uint32_t t = t0, used = used0, streak = streak0, hist = hist0;
    uint32_t lab_word = 0, lab_idx = 0xFFFFFFFFu;
    bool active = D1_FIN(hot.y) == 0;
    double z = (double)wp[31];  // V_s: the value of the row the env holds
    if (active) {
#pragma unroll
      for (int k = 0; k < RO64_SLOTS; ++k)
        if (la.slot_obs[k] >= 0) z = fma((double)la.obs[obs0 + la.slot_obs[k]], (double)wp[k], z);
    }
    for (int s = 0; s < a.n_steps; ++s) {
      if (!__any(active)) break;
      const int32_t act = active ? (int32_t)im_label_bits(va.v.alert_mask, va.v.mask_words, e, t, lab_word, lab_idx) : 0;
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
          if (q == RT_QUAD) continue;
          const float4 v = xp[q];
          xv[4 * q] = v.x; xv[4 * q + 1] = v.y; xv[4 * q + 2] = v.z; xv[4 * q + 3] = v.w;
        }
      }
      xv[4 * RT_QUAD] = (t > 0) ? (float)actual : 0.0f;
      xv[4 * RT_QUAD + 1] = (float)streak;
      xv[4 * RT_QUAD + 2] = (float)(budget - (int32_t)used2);
      xv[4 * RT_QUAD + 3] = (float)__popc(hist2);
      double zb = 0.0, ze = 0.0, zp = (double)wp[31];
#pragma unroll
      for (int k = 0; k < RO64_SLOTS; ++k) {
        asm volatile("" : "+v"(wb[k]), "+v"(we[k]), "+v"(wp[k]));  // keep the coefficients f32 (see k_rollout64)
        const double xk = (double)xv[k];
        zb = fma(xk, (double)wb[k], zb);
        ze = fma(xk, (double)we[k], ze);
        zp = fma(xk, (double)wp[k], zp);
      }
      if (!(xv[30] > 0.5f)) ze = -__builtin_inf();
      const float r = reward_from_logits(zb, ze, actual);
      if (active) {
        const bool done = (t + 1 >= ndays);
        const double vn = (!done && s + 1 < a.n_steps) ? zp : 0.0;  // V_{s+1}: 0 past the env's last day of the call
        const double y = ((double)r + vn) - z;
        const size_t d = (size_t)s * n + slot;
        va.day_y[d] = y;
        va.day_alert[d] = (uint8_t)actual;
        total += y;
        ret += (double)r;
        n_valid = s + 1;
        used = used2; hist = hist2;
        if (!done) { streak = actual ? streak + 1 : 0; t = t + 1; }
        else active = false;
        z = zp;
      }
    }
  }
  // ---------------------------------------------------------------- pass 2: g = w_e sum_s (Q_s - V_s) (o_s, 1)
  const double w_e = va.v.env_weight ? (double)va.v.env_weight[e] : 1.0;
  float *adv = va.v.advantage ? va.v.advantage + e : nullptr;
  double g[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) g[k] = 0.0;  // slot k's column; the bias rides in slot 31, as in the policy row
  double prefix = 0.0, sq = 0.0;
  if (n_valid > 0) {  // s = 0: the row the env holds on entry
    const double c = w_e * total;
#pragma unroll
    for (int k = 0; k < RO64_SLOTS; ++k)
      if (la.slot_obs[k] >= 0) g[k] = c * (double)la.obs[obs0 + la.slot_obs[k]];
    g[31] = c;
    sq = total * total;
    if (adv) adv[0] = (float)total;
    prefix = va.day_y[slot];
  }
  {
    uint32_t t = t0, used = used0, streak = streak0, hist = hist0;
    for (int s = 1; s < a.n_steps; ++s) {  // o_s = the vector of call-day s - 1
      const bool live = s < n_valid;
      if (!__any(live)) break;
      if (!live) continue;
      const size_t d = (size_t)s * n + slot;
      const uint32_t actual = va.day_alert[d - n];
      const double res = total - prefix;  // Q_s - V_s
      const double c = w_e * res;
      prefix += va.day_y[d];
      sq = fma(res, res, sq);
      if (adv) adv[(size_t)s * n] = (float)res;
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
      streak = actual ? streak + 1 : 0;  // call-day s - 1 was not terminal: the env stepped again on call-day s
      t = t + 1;
    }
  }
  // column-major, as k_policy_gradient_linear: a column's envs are contiguous
  float *out = va.grad + e;
#pragma unroll
  for (int k = 0; k < RO64_SLOTS; ++k)
    if (la.slot_obs[k] >= 0) out[(size_t)la.slot_obs[k] * n] = (float)g[k];
  out[(size_t)la.n_obs * n] = (float)g[31];
  va.v.sq_error[e] = (float)sq;
  va.v.days[e] = n_valid;
  va.v.ret[e] = (float)ret;
}

// ------------------------------------------------------------------------------------------------ MLP: pass 1
// Registers: wb[32], we[32] and xv[32] next to the network's fragments, as k_pgm_pass1 at the same launch bounds; the
// fork's state and chain are gone, the record of the day at hand (r, V_s, the alert, two flags) lives across the
// logit call in their place.
template <int WIDTH, int LAYERS>
__global__ __launch_bounds__(BLOCK, 2) void k_vg_pass1(const VgMlpArgs va) {
  __shared__ __attribute__((aligned(16))) float s_x[MLP_WAVES][64 * MLP_XS];
  const MlpGradArgs &ga = va.g;
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
  const float w_e = va.v.env_weight ? va.v.env_weight[e] : 1.0f;
  uint32_t lab_word = 0, lab_idx = 0xFFFFFFFFu;
  double total = 0.0, ret = 0.0;
  int32_t n_valid = 0;
  bool active = D1_FIN(hot.y) == 0 && valid;
#pragma unroll
  for (int k = 0; k < ROWF; ++k)
    xrow[k] = (k < RO64_SLOTS && ma.slot_obs[k] >= 0 && active) ? ma.obs[obs0 + ma.slot_obs[k]] : 0.0f;
  mlp_wave_lds_sync();
  float z = mlp_logit_groups<WIDTH, LAYERS>(ma, g, xs);  // V_s: the value of the row the env holds
  for (int s = 0; s < a.n_steps; ++s) {
    if (!__any(active)) break;
    const int32_t act = active ? (int32_t)im_label_bits(va.v.alert_mask, va.v.mask_words, e, t, lab_word, lab_idx) : 0;
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
    bool more = false;  // the env holds a row after this day, inside the call: V_{s+1} is its logit
    if (active) {
      const bool done = (t + 1 >= ndays);
      more = !done && s + 1 < a.n_steps;
      used = used2; hist = hist2;
      if (!done) { streak = actual ? streak + 1 : 0; t = t + 1; }
      else active = false;
    }
    float zn = 0.0f;
    if (s + 1 < a.n_steps) {  // wave-uniform: the logit of the row each env now holds, for tomorrow
      mlp_wave_lds_sync();
      zn = mlp_logit_groups<WIDTH, LAYERS>(ma, g, xs);
    }
    if (stepped) {  // day s's record, now that V_{s+1} is known
      const float y = (float)(((double)r + (more ? (double)zn : 0.0)) - (double)z);
      const size_t d = (size_t)s * n + slot;
      ga.day[d] = make_float2(w_e, y);  // pass 2: c_s = w_e (total - prefix) = w_e (Q_s - V_s)
      ga.day_alert[d] = (uint8_t)actual;
      total += (double)y;
      ret += (double)r;
      n_valid = s + 1;
    }
    z = zn;
  }
  if (valid) {
    ga.total[slot] = total;
    ga.n_valid[slot] = n_valid;
    va.v.days[e] = n_valid;
    va.v.ret[e] = (float)ret;
  }
}

// per visiting position: sum_s (total - prefix_s)^2 and, when asked for, the advantage rows. The loads of day.y are
// lane-consecutive; the stores go to the env's own column, lane-consecutive in identity order.
__global__ __launch_bounds__(256) void k_vg_finish(const VgMlpArgs va) {
  const MlpGradArgs &ga = va.g;
  const RolloutArgs &a = ga.m.r;
  const int64_t slot64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot64 >= a.n) return;
  const uint32_t slot = (uint32_t)slot64;
  uint32_t e = a.order ? a.order[slot] : slot;
  e = e < (uint32_t)a.n ? e : (uint32_t)(a.n - 1);
  const size_t n = (size_t)a.n;
  const double total = ga.total[slot];
  const int32_t nv = ga.n_valid[slot];
  float *adv = va.v.advantage ? va.v.advantage + e : nullptr;
  double prefix = 0.0, sq = 0.0;
  for (int s = 0; s < nv; ++s) {
    const double res = total - prefix;  // Q_s - V_s
    prefix += (double)ga.day[(size_t)s * n + slot].y;
    sq = fma(res, res, sq);
    if (adv) adv[(size_t)s * n] = (float)res;
  }
  va.v.sq_error[e] = (float)sq;
}

template <int WIDTH, int LAYERS>
static void launch_vg(const VgMlpArgs &va, unsigned grid1, hipStream_t s) {
  const MlpGradArgs &ga = va.g;
  hipLaunchKernelGGL((k_vg_pass1<WIDTH, LAYERS>), dim3(grid1), dim3(BLOCK), 0, s, va);
  hipLaunchKernelGGL(k_vg_finish, dim3((unsigned)((ga.m.r.n + 255) / 256)), dim3(256), 0, s, va);
  hipLaunchKernelGGL(k_pgm_count, dim3(ga.n_chunks), dim3(64), 0, s, ga);
  hipLaunchKernelGGL(k_pgm_scan, dim3(1), dim3(1024), 0, s, ga);
  hipLaunchKernelGGL((k_pgm_pass2<WIDTH, LAYERS>), dim3(ga.n_chunks), dim3(64), 0, s, ga);
  hipLaunchKernelGGL(k_pgm_reduce, dim3(ga.m.n_groups, (ga.m.stride + 255) / 256), dim3(256), 0, s, ga);
}

#endif  // W2A_VALUE_HIP_H
