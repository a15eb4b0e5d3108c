// w2a_gae.hip.h -- value regression along GIVEN alert schedules with GAE(lambda), discounting, a bootstrap past the call
// and targets fixed by an earlier call, linear and MLP
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_GAE_HIP_H
#define W2A_GAE_HIP_H

// ----------------------------------------------------------------------------------------
// lambda-returns along a schedule (w2a_value_gradient_linear_gae / _mlp_gae, estimator in w2a.h)
// ----------------------------------------------------------------------------------------
// The env is forced along its schedule and pays its rewards exactly as in w2a_value.hip.h. What changes is the per-day
// coefficient of dV_s/dtheta:
//     delta_s = r_s + gamma Vn_s - V_s,   A_s = delta_s + gamma lambda A_{s+1}  (A := 0 past the env's last day),
//     c_s = A_s,   or   c_s = target[s, e] - V_s   with targets given (no reward is formed then)
// Vn_s is the value of the row after day s: 0 on the episode's last day, and on the call's last day unless `bootstrap`.
// A_s does not telescope into total - prefix once gamma lambda < 1: the weights (gamma lambda)^(s' - s) would have to be
// carried as (gamma lambda)^s' / (gamma lambda)^s, which under- and overflows f32 (and loses fp64's digits) over 153
// days. So a backward sweep forms c_s per day and REWRITES the day record with it:
//   k_value_gradient_linear_gae  k_value_gradient_linear with the sweep between its passes, in the lane that wrote the
//                       column (no synchronisation): pass 1 stores delta_s and V_s in fp64 and the alert byte (17 B per
//                       env-day), the sweep walks the column from the env's last day back, replaces delta_s by c_s, writes
//                       the optional rows and sq_error; pass 2 is the forward walk with c = w_e c_s read from scratch.
//                       TARGET: pass 1 keeps the value row alone and stores c_s at once, the sweep is skipped.
//   k_gae_pass1         k_vg_pass1's day loop with day = (f32(delta_s), V_s), gamma on Vn_s and, with `bootstrap`, one
//                       more wave-uniform logit call after the call's last day. With targets the reward chains and the
//                       coefficient rows are skipped by a wave-uniform branch.
//   k_gae_finish        lane = visiting position: walks the lane's column backwards from n_valid - 1, forms A_s in fp64
//                       from the stored f32 delta_s, writes advantage / value_target at the env's id, sums c_s^2, and
//                       overwrites the record in place with day = (f32(w_e c_s), 0); total = 1 -- what k_sg_pass1
//                       leaves, so the count, scan, pass 2 and reduce kernels of w2a_policy_gradient_mlp.hip.h run unchanged.
// No floating-point atomics: identical calls give identical bits.
struct GaeArgs {
  double gamma;         // discount
  double gl;            // gamma * lambda
  int32_t bootstrap;    // 1: Vn of a truncated env's last call-day is the value of the row it then holds
  float *value_target;  // [n_steps][n] R_s = A_s + V_s by call-day and ENV ID (nullable); zero-filled before the launch
  const float *target;  // [>= n_steps][n] fixed targets, same layout (nullable)
};

struct GaeLinearArgs {
  VgLinearArgs v;   // as w2a_value_gradient_linear builds it; v.day_y holds delta_s, then c_s
  GaeArgs g;
  double *day_v;    // [n_steps][n] V_s of the lane at visiting position `slot`
};

struct GaeMlpArgs {
  VgMlpArgs v;      // as w2a_value_gradient_mlp builds it
  GaeArgs g;
};

// Registers: as k_value_gradient_linear (three coefficient rows and xv[] in pass 1, 31 fp64 accumulators in pass 2); the
// sweep between them holds four fp64 scalars. TARGET drops two of the three rows and both reward chains.
template <bool TARGET>
__global__ __launch_bounds__(BLOCK, 2) void k_value_gradient_linear_gae(const GaeLinearArgs xa) {
  const VgLinearArgs &va = xa.v;
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
  double ret = 0.0;     // sum of r_s (undiscounted)
  double sq = 0.0;      // sum of c_s^2
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
        const float4 p = pq[q];
        wp[4 * q] = p.x; wp[4 * q + 1] = p.y; wp[4 * q + 2] = p.z; wp[4 * q + 3] = p.w;
        if (!TARGET) {
          const float4 b = wq[q], f = wq[ROWF / 4 + q];
          wb[4 * q] = b.x; wb[4 * q + 1] = b.y; wb[4 * q + 2] = b.z; wb[4 * q + 3] = b.w;
          we[4 * q] = f.x; we[4 * q + 1] = f.y; we[4 * q + 2] = f.z; we[4 * q + 3] = f.w;
        }
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
      float r = 0.0f;
      if (TARGET) {
#pragma unroll
        for (int k = 0; k < RO64_SLOTS; ++k) zp = fma((double)xv[k], (double)wp[k], zp);
      } else {
#pragma unroll
        for (int k = 0; k < RO64_SLOTS; ++k) {
          asm volatile("" : "+v"(wb[k]), "+v"(we[k]), "+v"(wp[k]));  // keep the coefficients f32 (see k_rollout64)
          const double xk = (double)xv[k];
          zb = fma(xk, (double)wb[k], zb);
          ze = fma(xk, (double)we[k], ze);
          zp = fma(xk, (double)wp[k], zp);
        }
        if (!(xv[30] > 0.5f)) ze = -__builtin_inf();
        r = reward_from_logits(zb, ze, actual);
      }
      if (active) {
        const bool done = (t + 1 >= ndays);
        const size_t d = (size_t)s * n + slot;
        if (TARGET) {
          const double c = (double)xa.g.target[(size_t)s * n + e] - z;
          va.day_y[d] = c;
          sq = fma(c, c, sq);
        } else {
          // Vn_s: 0 on the episode's last day, and on the call's last day unless the caller bootstraps
          const double vn = (!done && (s + 1 < a.n_steps || xa.g.bootstrap)) ? zp : 0.0;
          va.day_y[d] = ((double)r + xa.g.gamma * vn) - z;
          xa.day_v[d] = z;
          ret += (double)r;
        }
        va.day_alert[d] = (uint8_t)actual;
        n_valid = s + 1;
        used = used2; hist = hist2;
        if (!done) { streak = actual ? streak + 1 : 0; t = t + 1; }
        else active = false;
        z = zp;
      }
    }
  }
  // ---------------------------------------------------------------- the sweep: A_s from the env's last day back
  if (!TARGET) {
    float *adv = va.v.advantage ? va.v.advantage + e : nullptr;
    float *vt = xa.g.value_target ? xa.g.value_target + e : nullptr;
    double A = 0.0;
    for (int s = n_valid - 1; s >= 0; --s) {
      const size_t d = (size_t)s * n + slot;
      A = fma(xa.g.gl, A, va.day_y[d]);
      va.day_y[d] = A;  // c_s
      sq = fma(A, A, sq);
      if (adv) adv[(size_t)s * n] = (float)A;
      if (vt) vt[(size_t)s * n] = (float)(A + xa.day_v[d]);
    }
  }
  // ---------------------------------------------------------------- pass 2: g = w_e sum_s c_s (o_s, 1)
  const double w_e = va.v.env_weight ? (double)va.v.env_weight[e] : 1.0;
  double g[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) g[k] = 0.0;  // slot k's column; the bias rides in slot 31, as in the policy row
  if (n_valid > 0) {  // s = 0: the row the env holds on entry
    const double c = w_e * va.day_y[slot];
#pragma unroll
    for (int k = 0; k < RO64_SLOTS; ++k)
      if (la.slot_obs[k] >= 0) g[k] = c * (double)la.obs[obs0 + la.slot_obs[k]];
    g[31] = c;
  }
  {
    uint32_t t = t0, used = used0, streak = streak0, hist = hist0;
    for (int s = 1; s < a.n_steps; ++s) {  // o_s = the vector of call-day s - 1
      const bool live = s < n_valid;
      if (!__any(live)) break;
      if (!live) continue;
      const size_t d = (size_t)s * n + slot;
      const uint32_t actual = va.day_alert[d - n];
      const double c = w_e * va.day_y[d];
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
// Registers: as k_vg_pass1 (wb[32], we[32] and xv[32] next to the network's fragments); w_e and the running total are
// gone, gamma and the bootstrap flag are wave-uniform arguments.
template <int WIDTH, int LAYERS>
__global__ __launch_bounds__(BLOCK, 2) void k_gae_pass1(const GaeMlpArgs xa) {
  __shared__ __attribute__((aligned(16))) float s_x[MLP_WAVES][64 * MLP_XS];
  const VgMlpArgs &va = xa.v;
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
  const bool given = xa.g.target != nullptr;  // wave-uniform: the targets are given, no reward is formed
  float wb[32], we[32];
  if (!given) {
    const uint32_t wrow = W_COL(cold.y) * (uint32_t)a.tb.n_samples + W_SAMPLE(cold.y);
    const float4 *wq = a.tb.W + (size_t)wrow * (2 * ROWF / 4);
#pragma unroll
    for (int q = 0; q < ROWF / 4; ++q) {
      const float4 b = wq[q], f = wq[ROWF / 4 + q];
      wb[4 * q] = b.x; wb[4 * q + 1] = b.y; wb[4 * q + 2] = b.z; wb[4 * q + 3] = b.w;
      we[4 * q] = f.x; we[4 * q + 1] = f.y; we[4 * q + 2] = f.z; we[4 * q + 3] = f.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 32; ++k) wb[k] = we[k] = 0.0f;
  }
  const int32_t g = pgm_group(ma, e);
  const uint32_t obs0 = e * (uint32_t)ma.n_obs;
  const size_t n = (size_t)a.n;
  uint32_t lab_word = 0, lab_idx = 0xFFFFFFFFu;
  double ret = 0.0;
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
    float r = 0.0f;
    if (!given) {
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
      float4 v;
      v.x = (active && ((ma.obs_mask >> (4 * q)) & 1u)) ? xv[4 * q] : 0.0f;
      v.y = (active && ((ma.obs_mask >> (4 * q + 1)) & 1u)) ? xv[4 * q + 1] : 0.0f;
      v.z = (active && ((ma.obs_mask >> (4 * q + 2)) & 1u)) ? xv[4 * q + 2] : 0.0f;
      v.w = (active && ((ma.obs_mask >> (4 * q + 3)) & 1u)) ? xv[4 * q + 3] : 0.0f;
      reinterpret_cast<float4 *>(xrow)[q] = v;
    }
    const bool stepped = active;
    // wave-uniform: a row after this day is looked at -- inside the call, or past it when the caller bootstraps
    const bool look = s + 1 < a.n_steps || (xa.g.bootstrap && !given);
    bool more = false;  // the env holds a row after this day whose value enters: Vn_s is its logit
    if (active) {
      const bool done = (t + 1 >= ndays);
      more = !done && look;
      used = used2; hist = hist2;
      if (!done) { streak = actual ? streak + 1 : 0; t = t + 1; }
      else active = false;
    }
    float zn = 0.0f;
    if (look) {  // the logit of the row each env now holds, for tomorrow (or for the bootstrap)
      mlp_wave_lds_sync();
      zn = mlp_logit_groups<WIDTH, LAYERS>(ma, g, xs);
    }
    if (stepped) {  // day s's record, now that Vn_s is known
      const float dl = (float)(((double)r + xa.g.gamma * (more ? (double)zn : 0.0)) - (double)z);
      const size_t d = (size_t)s * n + slot;
      ga.day[d] = make_float2(dl, z);  // k_gae_finish turns it into (w_e c_s, 0)
      ga.day_alert[d] = (uint8_t)actual;
      ret += (double)r;
      n_valid = s + 1;
    }
    z = zn;
  }
  if (valid) {
    ga.n_valid[slot] = n_valid;
    va.v.days[e] = n_valid;
    va.v.ret[e] = (float)ret;
  }
}

// per visiting position, from the env's last day back: A_s, the optional rows, sum_s c_s^2 and the record pass 2 reads.
// The loads and stores of `day` are lane-consecutive; the rows go to the env's own column, lane-consecutive in identity
// order.
__global__ __launch_bounds__(256) void k_gae_finish(const GaeMlpArgs xa) {
  const VgMlpArgs &va = xa.v;
  const MlpGradArgs &ga = va.g;
  const RolloutArgs &a = ga.m.r;
  const int64_t slot64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot64 >= a.n) return;
  const uint32_t slot = (uint32_t)slot64;
  uint32_t e = a.order ? a.order[slot] : slot;
  e = e < (uint32_t)a.n ? e : (uint32_t)(a.n - 1);
  const size_t n = (size_t)a.n;
  const int32_t nv = ga.n_valid[slot];
  const double w_e = va.v.env_weight ? (double)va.v.env_weight[e] : 1.0;
  float *adv = va.v.advantage ? va.v.advantage + e : nullptr;
  float *vt = xa.g.value_target ? xa.g.value_target + e : nullptr;
  const float *tg = xa.g.target ? xa.g.target + e : nullptr;
  double A = 0.0, sq = 0.0;
  for (int s = nv - 1; s >= 0; --s) {
    const size_t d = (size_t)s * n + slot;
    const float2 rec = ga.day[d];  // (f32(delta_s), V_s)
    double c;
    if (tg) {
      c = (double)tg[(size_t)s * n] - (double)rec.y;
    } else {
      A = fma(xa.g.gl, A, (double)rec.x);
      c = A;
      if (adv) adv[(size_t)s * n] = (float)A;
      if (vt) vt[(size_t)s * n] = (float)(A + (double)rec.y);
    }
    sq = fma(c, c, sq);
    ga.day[d] = make_float2((float)(w_e * c), 0.0f);  // pass 2: c_s = day.x (1 - 0)
  }
  ga.total[slot] = 1.0;
  va.v.sq_error[e] = (float)sq;
}

template <int WIDTH, int LAYERS>
static void launch_gae(const GaeMlpArgs &xa, unsigned grid1, hipStream_t s) {
  const MlpGradArgs &ga = xa.v.g;
  hipLaunchKernelGGL((k_gae_pass1<WIDTH, LAYERS>), dim3(grid1), dim3(BLOCK), 0, s, xa);
  hipLaunchKernelGGL(k_gae_finish, dim3((unsigned)((ga.m.r.n + 255) / 256)), dim3(256), 0, s, xa);
  hipLaunchKernelGGL(k_pgm_count, dim3(ga.n_chunks), dim3(64), 0, s, ga);
  hipLaunchKernelGGL(k_pgm_scan, dim3(1), dim3(1024), 0, s, ga);
  hipLaunchKernelGGL((k_pgm_pass2<WIDTH, LAYERS>), dim3(ga.n_chunks), dim3(64), 0, s, ga);
  hipLaunchKernelGGL(k_pgm_reduce, dim3(ga.m.n_groups, (ga.m.stride + 255) / 256), dim3(256), 0, s, ga);
}

#endif  // W2A_GAE_HIP_H
