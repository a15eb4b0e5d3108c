// w2a_rollout_linear.hip.h -- k_rollout_linear: on-device rollout of a linear policy with one parameter row per group
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_ROLLOUT_LINEAR_HIP_H
#define W2A_ROLLOUT_LINEAR_HIP_H

// ----------------------------------------------------------------------------------------
// linear-logistic policy inside k_rollout64's day loop (w2a_rollout_linear)
// ----------------------------------------------------------------------------------------
// Env i acts on logit = W[g[i]] . obs_i + b[g[i]], where obs_i is exactly the row w2a_step would have returned to the
// agent before that decision (faithful semantics: the lagging observation, Q6). That row is the 32-slot vector xv[] the
// reward of the PREVIOUS day is computed on (k_step64 scatters the same vector into the observation rows): so tomorrow's
// logit is a third fp64 FMA chain over today's xv[], next to the two reward chains, and one fp64 scalar is carried into
// the next day. The first day's logit comes from the observation row the caller holds (the state alone cannot rebuild
// it: the observed streak is the pre-update one). Every env writes the row it holds when the call ends back into that
// buffer, once: on the last day of the call, or on the day before its terminal day (the terminal step leaves the stale
// observation, env.py:257-262), so consecutive calls and mixed w2a_step / w2a_rollout_linear sequences chain.
//   Logit order: bias first, then slots 0..29 in slot order -- the same sequence of fp64 FMAs on the first day (from the
//   observation row, through slot_obs) as on every later day (from xv[]); slots that are not observation columns carry a
//   zero coefficient (masked on load), so their products add exactly 0.
struct LinearRolloutArgs {
  RolloutArgs r;           // tables, state, outputs, visiting order, n_steps (r.pol: require_budget and seed only)
  const float4 *weight;    // [n_groups][8] policy rows in slot order
  const float *bias;       // [n_groups]
  const int32_t *group;    // [n] group of every env (nullable = group 0); clamped into [0, n_groups) -- never read outside
  int32_t n_groups;
  int32_t n_obs;
  uint32_t obs_mask;       // bit k: slot k is an observation column (others get a zero coefficient)
  float *obs;              // [n][n_obs] in: the row every env holds; out: the row it holds when the call ends
  int8_t slot_obs[RO64_SLOTS];  // slot -> observation column, -1 = none (kernel argument: scalar loads, no table)
  const uint32_t *gate;    // [n][gate_words] allowed days (policy["allowed_days"]): bit (t & 31) of word t >> 5, the layout
                           // of alert_mask. Read by the GATE = true instantiations only (the *_gated entry points)
  int32_t gate_words;
  LookArgs look;           // policy["lookahead"] (w2a_lookahead.hip.h): read by the LOOK = true instantiations only (the
                           // w2a_lookahead_* entry points); zero otherwise
};

// the gate's bit of day t: on a day whose bit is clear the attempted action is forced to 0 before the budget test, and
// the day carries no score (as a day on which require_budget forces the action). One plain 32-bit load per env per 32
// days; a day past the bitmap is not allowed (the host checks that gate_words covers T)
__device__ __forceinline__ bool gate_allows(const uint32_t *gate, int32_t gate_words, uint32_t e, uint32_t t,
                                            uint32_t &word, uint32_t &idx) {
  const uint32_t wi = t >> 5;
  if (wi != idx) {
    idx = wi;
    word = wi < (uint32_t)gate_words ? gate[(size_t)e * gate_words + wi] : 0u;
  }
  return ((word >> (t & 31)) & 1u) != 0u;
}

// RECORD (w2a_rollout_linear_record / w2a_rollout_mlp_record): every active day also stores the trajectory entry of
// (call-day s, env e) -- action, logit, reward, flags and the observation row the env holds after the step -- with
// plain per-lane stores at env-id addresses (w2a.h: w2a_trajectory). Addresses are formed where they are used: 64-bit
// slab offsets ((s + 1) * n * n_obs passes 2^32 at 1 M envs), one pointer per row, nothing held across the day loop.
__device__ __forceinline__ float *traj_obs_row(const w2a_trajectory &tr, int32_t slab, int64_t n, uint32_t e,
                                               int32_t n_obs) {
  uint64_t o = ((uint64_t)slab * (uint64_t)n + e) * (uint64_t)n_obs;
  asm volatile("" : "+v"(o));  // one offset register pair: the 29 row addresses are not hoisted out of the day loop
  return tr.obs + o;
}

// one whole observation row of the caller's buffer into trajectory slab `slab` (slab 0 on entry, slab n_steps at
// the end, and the repeated row after a terminal step)
template <class Args>
__device__ __forceinline__ void traj_copy_row(const Args &pa, const w2a_trajectory &tr, int32_t slab, uint32_t e,
                                              uint32_t obs0) {
  float *dst = traj_obs_row(tr, slab, pa.r.n, e, pa.n_obs);
  uint32_t o = obs0;
  asm volatile("" : "+v"(o));
#pragma unroll
  for (int k = 0; k < RO64_SLOTS; ++k)
    if (pa.slot_obs[k] >= 0) dst[pa.slot_obs[k]] = pa.obs[o + pa.slot_obs[k]];
}

// Two store designs for the observation rows (profiles/r09/store_design_ab.log):
//   staged  (identity visiting order: a wave serves 64 consecutive envs, whose rows of slab s + 1 are one contiguous
//           64 * n_obs-float block): each lane puts its row into the wave's LDS tile [64][n_obs], then the wave stores
//           the block with lane-consecutive dwords (every store instruction covers 256 contiguous bytes);
//   direct  (any other order): each lane stores its own row, n_obs scattered dwords.
// The host passes no visiting order to a recorded call where it can (w2a_kernels.hip), so the staged form is the usual one.
#define TRAJ_TILE (64 * RO64_SLOTS)  // floats of a wave's staging tile (n_obs <= RO64_SLOTS)

__device__ __forceinline__ void traj_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the trajectory entry of an active env's call-day s; xv[] is the row it holds after a non-terminal step. stage: the
// wave's LDS tile (staged design) or nullptr (direct design)
template <class Args>
__device__ __forceinline__ void traj_record_day(const Args &pa, const w2a_trajectory &tr, int32_t s, uint32_t e,
                                                uint32_t obs0, const float (&xv)[32], int32_t act, float logit,
                                                float r, bool done, uint32_t actual, float *stage) {
  const size_t d = (size_t)s * (size_t)pa.r.n + e;
  tr.action[d] = (uint8_t)act;
  tr.logit[d] = logit;
  tr.reward[d] = r;
  tr.flags[d] = (uint8_t)(W2A_TRAJ_VALID | (done ? W2A_TRAJ_TERMINATED : 0) | (actual ? W2A_TRAJ_ALERT : 0));
  if (s + 1 < pa.r.n_steps) {  // slab n_steps: after the day loop, for every env
    uint32_t o = obs0;
    asm volatile("" : "+v"(o));
    float *dst = stage ? stage + (threadIdx.x & 63) * pa.n_obs : traj_obs_row(tr, s + 1, pa.r.n, e, pa.n_obs);
    if (done) {  // the terminal step leaves the previous row, still in the buffer
#pragma unroll
      for (int k = 0; k < RO64_SLOTS; ++k)
        if (pa.slot_obs[k] >= 0) dst[pa.slot_obs[k]] = pa.obs[o + pa.slot_obs[k]];
    } else {
#pragma unroll
      for (int k = 0; k < RO64_SLOTS; ++k)
        if (pa.slot_obs[k] >= 0) dst[pa.slot_obs[k]] = xv[k];
    }
  }
}

// staged design, wave-uniform, after every lane's traj_record_day of call-day s: the wave's tile to slab s + 1. Rows of
// lanes with no live env carry stale values into entries the contract leaves unspecified; nothing is stored past env
// n - 1 (e0: the wave's first env)
template <class Args>
__device__ __forceinline__ void traj_store_tile(const Args &pa, const w2a_trajectory &tr, int32_t s, uint32_t e0,
                                                const float *stage) {
  if (s + 1 >= pa.r.n_steps) return;
  traj_wave_lds_sync();
  const int64_t left = pa.r.n - (int64_t)e0;
  const uint32_t lim = (uint32_t)(left < 64 ? left : 64) * (uint32_t)pa.n_obs;
  float *blk = traj_obs_row(tr, s + 1, pa.r.n, e0, pa.n_obs);
  for (uint32_t f = threadIdx.x & 63; f < lim; f += 64) blk[f] = stage[f];
  traj_wave_lds_sync();  // the tile is read before the next day's rows go in
}

// Registers: the third coefficient row costs 30 VGPRs over k_rollout64's 121-124. Left to itself the compiler takes
// 169-189 (2 waves/SIMD, no spill); held to 3 waves/SIMD (168) it spills 14-89 B per lane to scratch and runs faster:
// 1.50 ms against 1.71 ms per 1 M-env episode (profiles/r07/kernel_trace_linear.txt).
// RECORD = false compiles to the kernel without a trajectory (same registers, scratch and LDS).
// GATE (w2a_rollout_linear_gated / _record_gated): la.gate restricts the attempts; GATE = false compiles from the
// statements it had before the gate existed.
// LOOK (w2a_lookahead_rollout_linear and its _gated form): the logit chain goes on over la.look.days lookahead inputs of
// the held row's day (w2a_lookahead.hip.h): on entry from the state and the series, then every day next to zp. LOOK =
// false compiles from the statements it had before; there is no RECORD form.
// NOISE (w2a_forecast_rollout_linear; needs LOOK): the lookahead inputs carry the forecast error of la.look.mae
// (w2a_lookahead.hip.h), drawn from a stream of the env's own that is derived once, before the day loop.
template <bool MASKS, bool SAMPLE, bool RECORD, bool GATE, bool LOOK = false, bool NOISE = false>
__global__ __launch_bounds__(BLOCK, 3) void k_rollout_linear(const LinearRolloutArgs la, const w2a_trajectory tr) {
  const RolloutArgs &a = la.r;
  const int64_t slot64 = (int64_t)logical_block(blockIdx.x, gridDim.x >> 3) * BLOCK + threadIdx.x;
  if (slot64 - (threadIdx.x & 63) >= a.n) return;  // whole wave past the end
  const bool valid = slot64 < a.n;
  const uint32_t slot = (uint32_t)(valid ? slot64 : (a.n - 1));
  const uint32_t e = a.order ? a.order[slot] : slot;  // the env this lane serves
  uint4 c2, hot;
  load_step_state(a.st, e, c2, hot);
  const uint4 cold = load_cold(a.st, e);
  uint32_t t = D0_T(hot.x), used = D0_USED(hot.x), streak = D0_STREAK(hot.x), last = D0_LAST(hot.x);
  uint32_t atb = D0_ATB(hot.x), hist = D1_HIST(hot.y);
  const uint32_t ndays = D1_NDAYS(hot.y);
  const int32_t budget = (int32_t)hot.w;
  bool fin = D1_FIN(hot.y) != 0;
  float ret_total = __uint_as_float(hot.z);
  const uint32_t rows_per_day = (uint32_t)(a.tb.S_w * a.tb.Y);
  const uint32_t wrow = W_COL(cold.y) * (uint32_t)a.tb.n_samples + W_SAMPLE(cold.y);
  // the env's two coefficient rows and its policy row, once per launch
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
    wp[31] = la.bias[g];  // slot 31 holds no observation column and no reward input: the bias rides there
  }
  float lw[W2A_LOOK_MAX], lf[W2A_LOOK_MAX];
  const float *lser = nullptr;
  if constexpr (LOOK) {
    int32_t g = la.group ? la.group[e] : 0;
    g = g < 0 ? 0 : (g >= la.n_groups ? la.n_groups - 1 : g);
    look_weights(la.look, g, lw);
    lser = look_series(la.look, cold.x);
  }
  uint64_t estream = 0;
  if constexpr (NOISE) estream = look_noise_stream(la.look, (uint64_t)(a.gid0 + e), cold.w);
  const uint64_t pstream = SAMPLE ? rng_stream(a.pol.seed ^ 0xA5A5A5A55A5A5A5Aull, (uint64_t)(a.gid0 + e), cold.w) : 0ull;
  const uint32_t obs0 = e * (uint32_t)la.n_obs;  // first element of the env's observation row (host: n * n_obs < 2^31)
  if (RECORD && valid) traj_copy_row(la, tr, 0, e, obs0);  // slab 0: the row every env holds on entry
  float *stage = nullptr;  // staged store design: identity order (wave-uniform)
  if constexpr (RECORD) {
    __shared__ float s_traj[BLOCK / 64][TRAJ_TILE];
    if (!a.order) stage = s_traj[threadIdx.x >> 6];
  }
  float ret = 0.0f;
  int32_t alerts = 0, over = 0;
  uint32_t mask_word = 0, mask_idx = 0xFFFFFFFFu;
  uint32_t att_word = 0, att_idx = 0xFFFFFFFFu;
  float snap = 0.0f;
  bool snapped = false;
  bool active = !fin && valid;
  uint32_t gate_word = 0, gate_idx = 0xFFFFFFFFu;
  // first day: the logit of the observation row the agent holds
  double z = (double)wp[31];
  if (active) {
#pragma unroll
    for (int k = 0; k < RO64_SLOTS; ++k)
      if (la.slot_obs[k] >= 0) z = fma((double)la.obs[obs0 + la.slot_obs[k]], (double)wp[k], z);
    if constexpr (LOOK) {  // the held row is day max(t - 1, 0)'s: its lookahead inputs are rebuilt, never carried
      look_inputs<NOISE>(la.look, look_series_of<NOISE>(la.look, lser, cold.x), t > 0 ? t - 1 : 0u, ndays, lf, estream);
      z = look_logit(la.look, lf, lw, z);
    }
  }
  for (int s = 0; s < a.n_steps; ++s) {
    if (!__any(active)) break;
    // ---- policy: alert iff logit > 0, or u < sigmoid(logit) with the Bernoulli policy's uniform of (env, episode, day)
    int32_t act;
    if (SAMPLE) {
      // sigmoid in f32 (v_exp_f32 / v_rcp_f32, as the reward's): within ~1e-7 of the fp64 value
      const uint32_t u = (uint32_t)(w2a_mix64(pstream + (uint64_t)(t + 1) * 0x9E3779B97F4A7C15ull) >> 32);
      act = ((float)u * 2.3283064365386963e-10f < sigmoid_f32((float)z)) ? 1 : 0;
    } else {
      act = z > 0.0 ? 1 : 0;
    }
    if (a.pol.require_budget && budget - (int32_t)used <= 0) act = 0;
    if (GATE && active && !gate_allows(la.gate, la.gate_words, e, t, gate_word, gate_idx)) act = 0;  // not attempted
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
    // the run-time fields of the faithful observation (env.py:190-193): lag = today's alert, the pre-update streak
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
    if constexpr (LOOK) {  // xv[] is day t's row: tomorrow's decision looks ahead from day t
      look_inputs<NOISE>(la.look, look_series_of<NOISE>(la.look, lser, cold.x), t, ndays, lf, estream);
      zp = look_logit(la.look, lf, lw, zp);
    }
    if (!(xv[30] > 0.5f)) ze = -__builtin_inf();
    const float r = reward_from_logits(zb, ze, actual);
    if (active) {
      const bool done = (t + 1 >= ndays);
      ret += r;
      ret_total += r;
      alerts += (int32_t)actual;
      over += (act == 1 && atb_s) ? 1 : 0;
      if (MASKS && a.alert_mask && actual) {
        const uint32_t wi = t >> 5;
        if (wi != mask_idx) {
          if (mask_idx != 0xFFFFFFFFu && mask_idx < (uint32_t)a.mask_words)
            a.alert_mask[(size_t)e * a.mask_words + mask_idx] |= mask_word;
          mask_idx = wi;
          mask_word = 0;
        }
        mask_word |= 1u << (t & 31);
      }
      if (MASKS && a.attempt_mask && act == 1) {
        const uint32_t wi = t >> 5;
        if (wi != att_idx) {
          if (att_idx != 0xFFFFFFFFu && att_idx < (uint32_t)a.mask_words)
            a.attempt_mask[(size_t)e * a.mask_words + att_idx] |= att_word;
          att_idx = wi;
          att_word = 0;
        }
        att_word |= 1u << (t & 31);
      }
      if (MASKS && (done ? t : t + 1) + 2 == ndays) { snap = ret_total; snapped = true; }
      if (RECORD) traj_record_day(la, tr, s, e, obs0, xv, act, (float)z, r, done, actual, stage);
      // the row the agent now holds is xv[] (a terminal step leaves the previous one): written back once, when it is
      // the last row of this call -- its last day, or the day before the terminal one
      if (!done && (s + 1 == a.n_steps || t + 2 >= ndays)) {
        // the addresses are formed here, from one offset register: hoisted out of the day loop, the 29 of them would
        // hold 58 VGPRs for the whole launch
        uint32_t o = obs0;
        asm volatile("" : "+v"(o));
#pragma unroll
        for (int k = 0; k < RO64_SLOTS; ++k)
          if (la.slot_obs[k] >= 0) la.obs[o + la.slot_obs[k]] = xv[k];
      }
      used = used2; hist = hist2; last = actual; atb = atb_s;
      if (!done) { streak = actual ? streak + 1 : 0; t = t + 1; }
      else { fin = true; active = false; }
      z = zp;
    }
    if (RECORD && stage) traj_store_tile(la, tr, s, (uint32_t)(slot64 - (threadIdx.x & 63)), stage);
  }
  if (RECORD && valid) traj_copy_row(la, tr, a.n_steps, e, obs0);  // slab n_steps: the buffer as the call leaves it
  if (valid) {
    store_hot(a.st, e, make_uint4(pack_d0(t, used, streak, last, atb), pack_d1(hist, ndays, fin ? 1u : 0u),
                                  __float_as_uint(ret_total), (uint32_t)budget));
    if (a.ret_out) a.ret_out[e] = ret;
    if (a.alerts_out) a.alerts_out[e] = alerts;
    if (a.attempts_over_budget) a.attempts_over_budget[e] = over;
    if (MASKS && a.alert_mask && mask_idx != 0xFFFFFFFFu && mask_idx < (uint32_t)a.mask_words)
      a.alert_mask[(size_t)e * a.mask_words + mask_idx] |= mask_word;
    if (MASKS && a.attempt_mask && att_idx != 0xFFFFFFFFu && att_idx < (uint32_t)a.mask_words)
      a.attempt_mask[(size_t)e * a.mask_words + att_idx] |= att_word;
    if (MASKS && a.ret_snapshot && snapped) a.ret_snapshot[e] = snap;
    if (fin && a.last_return && !D1_FIN(hot.y)) a.last_return[e] = ret_total;
  }
}

#endif  // W2A_ROLLOUT_LINEAR_HIP_H
