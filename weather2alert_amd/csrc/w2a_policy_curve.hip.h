// w2a_policy_curve.hip.h -- k_policy_curve_linear: a linear policy's rollout for EVERY remaining budget 0 .. B in one sweep
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_POLICY_CURVE_HIP_H
#define W2A_POLICY_CURVE_HIP_H

// ----------------------------------------------------------------------------------------
// policy budget curve (w2a_policy_curve_linear)
// ----------------------------------------------------------------------------------------
// Column b of env e is k_rollout_linear on the twin whose budget is used + b. The reward and the policy read the budget
// through the run-time slots 24..27 only (alert_lag1, the pre-update streak, the remaining budget, the agent's 14-day
// count), and the three fp64 chains of k_rollout_linear run in slot order: so their values after slot 23 -- from 0 for
// the two reward chains, from the bias for the policy chain -- are the same bits for every budget, and so is the
// Bernoulli uniform of a day (keyed by seed, env id, episode and day). One gather and one 72-FMA prefix per env-day
// serve all budgets; per budget only slots 24..27 from that budget's counters, then 28 and 29, then the decision, the
// reward and the counter update of k_rollout_linear, statement for statement.
//   Mapping: one 64-lane workgroup (one wave) serves E envs x C budgets, C = the budgets of one chunk (<= 64, the same
//   for every chunk of a call), E = 64 / C envs, in blocks of D = 64 / E call-days:
//     prefix phase  lane l = (env l / D, call-day l % D): gathers that day's row once, runs the three chains over slots
//                   0..23 and leaves them in LDS with x28, x29, the day's uniform and its two flags (heat gate, alert gate);
//     tail phase    lane l = (env l / C, budget l % C): walks the D days with ITS budget's counters, logit, return, counts
//                   and schedule word in registers, reading each day's prefixes from LDS (all lanes of an env read one
//                   address: a broadcast).
//   Budgets beyond 64 go in chunks of equal size (ceil((B + 1) / ceil((B + 1) / 64))); each chunk is a workgroup of its
//   own that redoes the prefix. No per-budget state lives in LDS or scratch; LDS holds 64 day entries of 40 B.
//   First day: the logit of the row the agent holds, from the caller's observation buffer with (float) b in place of
//   its remaining_budget column at that column's place in the chain -- or, with obs = NULL (a start no buffer belongs
//   to: every live env at t = 0 with nothing used), from day 0's table row with lag 0, streak 0 and count 0, the row a
//   reset writes. One lane per (env, budget) runs that whole chain once.
//   No atomics; identical calls give identical bits; nothing is written but the outputs. The start is a w2a_state_view
//   (the caller's arrays): the handle's state, observation buffer and bookkeeping are not touched.
#define PC_BLOCK 64
#define PC_MAX_BUDGET 1023

struct PcArgs {
  DevTables tb;
  w2a_state_view st;       // start state (device i32 arrays); budget and used are not read
  int64_t n, gid0;
  int32_t n_steps, B;
  int32_t C, n_chunks;     // budgets per chunk, chunks
  int32_t E, D;            // envs per workgroup, call-days per phase
  const float4 *weight;    // [n_groups][8] policy rows in slot order
  const float *bias;       // [n_groups]
  const int32_t *group;    // nullable, clamped as in k_rollout_linear
  int32_t n_groups, n_obs;
  uint32_t obs_mask;
  const float *obs;        // [n][n_obs] the rows the agents hold, or NULL (rebuilt from day 0's table row)
  int8_t slot_obs[RO64_SLOTS];
  int32_t require_budget;
  uint64_t seed;
  const uint32_t *gate;    // [n][gate_words], GATE = true only
  int32_t gate_words;
  float *ret;              // [n][B + 1]
  int32_t *alerts, *over;  // [n][B + 1]
  uint32_t *mask;          // SCHED = true only: [n][B + 1][mask_words]
  int32_t mask_words;
};

struct PcEnv {  // one env's start, decoded and range-checked
  uint32_t t0, streak, hist, ndays, ep_row, wrow, episode;
  int32_t g;
  bool bad;
  uint32_t H;  // call-days the env steps
};
__device__ __forceinline__ PcEnv pc_env(const PcArgs &a, uint32_t e) {
  const w2a_state_view &v = a.st;
  PcEnv h;
  h.t0 = (uint32_t)v.t[e]; h.streak = (uint32_t)v.streak[e]; h.hist = (uint32_t)v.hist14[e] & 0x3FFFu;
  h.ndays = (uint32_t)v.n_days[e]; h.episode = (uint32_t)v.episode_no[e];
  const uint32_t cw = (uint32_t)v.county_w[e], yi = (uint32_t)v.year_i[e], col = (uint32_t)v.coef_col[e];
  const uint32_t smp = (uint32_t)v.sample[e];
  // a start state no reset can produce would index outside the tables: NaN marks the env, nothing is read
  h.bad = cw >= (uint32_t)a.tb.S_w || yi >= (uint32_t)a.tb.Y || col >= (uint32_t)a.tb.S ||
          smp >= (uint32_t)a.tb.n_samples || h.ndays > (uint32_t)a.tb.T;
  h.ep_row = cw * (uint32_t)a.tb.Y + yi;
  h.wrow = col * (uint32_t)a.tb.n_samples + smp;
  int32_t g = a.group ? a.group[e] : 0;
  h.g = g < 0 ? 0 : (g >= a.n_groups ? a.n_groups - 1 : g);
  const bool active = !h.bad && v.finished[e] == 0 && h.t0 < h.ndays;
  h.H = active ? min((uint32_t)a.n_steps, h.ndays - h.t0) : 0u;
  return h;
}

#define PC_FLAG_HEAT 1u  // xv[30] > 0.5f: the effectiveness enters the reward
#define PC_FLAG_OPEN 2u  // the alert gate allows the day

// SAMPLE: the Bernoulli policy (u < sigmoid(logit)); GATE: a.gate restricts the attempts; SCHED: a.mask takes the
// schedules. Grid: ceil(n / E) * n_chunks workgroups of PC_BLOCK lanes; workgroup w serves envs (w / n_chunks) * E ..
// and budgets (w % n_chunks) * C ..
template <bool SAMPLE, bool GATE, bool SCHED>
__global__ __launch_bounds__(PC_BLOCK) void k_policy_curve_linear(const PcArgs a) {
  __shared__ double s_pb[PC_BLOCK], s_pe[PC_BLOCK], s_pp[PC_BLOCK];  // the chains after slot 23: baseline, effectiveness, policy
  __shared__ float4 s_tl[PC_BLOCK];                                  // x28, x29, the day's uniform, the flags
  const uint32_t lane = threadIdx.x;
  const uint32_t tile = blockIdx.x / (uint32_t)a.n_chunks, chunk = blockIdx.x % (uint32_t)a.n_chunks;
  const uint32_t E = (uint32_t)a.E, D = (uint32_t)a.D, C = (uint32_t)a.C, B = (uint32_t)a.B;
  const uint64_t e_first = (uint64_t)tile * E;
  const uint32_t rows_per_day = (uint32_t)(a.tb.S_w * a.tb.Y);

  // ---- this lane's two roles
  const uint32_t pi = lane / D, pd = lane % D;  // prefix: env pi of the tile, call-day pd of the block
  const bool p_ok = pi < E && e_first + pi < (uint64_t)a.n;
  const uint32_t pe_id = (uint32_t)(p_ok ? e_first + pi : 0);
  PcEnv hp;
  hp.H = 0;
  if (p_ok) hp = pc_env(a, pe_id);
  const uint32_t ti = lane / C, tc = lane % C;  // tail: env ti of the tile, budget tc of the chunk
  const uint32_t b = chunk * C + tc;
  const bool t_ok = ti < E && e_first + ti < (uint64_t)a.n && b <= B;
  const uint32_t e = (uint32_t)(t_ok ? e_first + ti : 0);
  PcEnv h;
  h.H = 0; h.bad = false;
  if (t_ok) h = pc_env(a, e);

  // ---- the tail role's coefficients of slots 24..29 (f32 as stored; the policy row masked as in k_rollout_linear)
  float wb[6], we[6], wp[6];
  double z = 0.0;  // the logit of the next decision
  if (h.H > 0) {
    const float4 *wq = a.tb.W + (size_t)h.wrow * (2 * ROWF / 4);
    const float4 *pq = a.weight + (size_t)h.g * (ROWF / 4);
    const float4 b6 = wq[RT_QUAD], b7 = wq[GATE_QUAD], f6 = wq[ROWF / 4 + RT_QUAD], f7 = wq[ROWF / 4 + GATE_QUAD];
    const float4 p6 = pq[RT_QUAD], p7 = pq[GATE_QUAD];
    wb[0] = b6.x; wb[1] = b6.y; wb[2] = b6.z; wb[3] = b6.w; wb[4] = b7.x; wb[5] = b7.y;
    we[0] = f6.x; we[1] = f6.y; we[2] = f6.z; we[3] = f6.w; we[4] = f7.x; we[5] = f7.y;
    wp[0] = p6.x; wp[1] = p6.y; wp[2] = p6.z; wp[3] = p6.w; wp[4] = p7.x; wp[5] = p7.y;
#pragma unroll
    for (int k = 0; k < 6; ++k) wp[k] = ((a.obs_mask >> (4 * RT_QUAD + k)) & 1u) ? wp[k] : 0.0f;
    // first day: the logit of the row the agent holds -- bias first, then the observation columns in slot order, with
    // (float) b where the row has its remaining budget
    z = (double)a.bias[h.g];
    const float *prow = reinterpret_cast<const float *>(pq);
    const float *held = a.obs ? a.obs + (size_t)e * (size_t)a.n_obs : nullptr;
    const float *day0 = reinterpret_cast<const float *>(a.tb.X + (size_t)h.ep_row * (ROWF / 4));
    for (int k = 0; k < RO64_SLOTS; ++k) {
      if (a.slot_obs[k] < 0) continue;
      float x;
      if (k == 4 * RT_QUAD + 2) x = (float)b;
      else if (held) x = held[a.slot_obs[k]];
      else x = (k >= 4 * RT_QUAD && k < 4 * RT_QUAD + 4) ? 0.0f : day0[k];
      z = fma((double)x, (double)prow[k], z);
    }
  }

  // ---- the tail role's counters of budget b
  int32_t rem = (int32_t)b;  // budget - used of the twin
  uint32_t streak = h.streak, hist = h.hist;
  float ret = 0.0f;
  int32_t alerts = 0, over = 0;
  const uint32_t nw = SCHED ? (uint32_t)a.mask_words : 0u;
  const size_t row = (size_t)e * (B + 1u) + b;
  uint32_t w = 0, word = 0;
  // ---- the prefix role's stream of uniforms
  const uint64_t pstream =
      SAMPLE && hp.H > 0 ? rng_stream(a.seed ^ 0xA5A5A5A55A5A5A5Aull, (uint64_t)(a.gid0 + pe_id), hp.episode) : 0ull;

  for (uint32_t s0 = 0; __any(s0 < h.H); s0 += D) {
    // ---- prefix phase: call-day s0 + pd of env pi
    if (s0 + pd < hp.H) {
      const uint32_t t = hp.t0 + s0 + pd;
      const float4 *xp = a.tb.X + (size_t)(t * rows_per_day + hp.ep_row) * (ROWF / 4);
      const float4 *wq = a.tb.W + (size_t)hp.wrow * (2 * ROWF / 4);
      const float4 *pq = a.weight + (size_t)hp.g * (ROWF / 4);
      double zb = 0.0, ze = 0.0, zp = (double)a.bias[hp.g];
#pragma unroll
      for (int q = 0; q < RT_QUAD; ++q) {  // slots 0..23 in slot order
        const float4 x = xp[q], bq = wq[q], fq = wq[ROWF / 4 + q];
        float4 p = pq[q];
        p.x = ((a.obs_mask >> (4 * q)) & 1u) ? p.x : 0.0f;
        p.y = ((a.obs_mask >> (4 * q + 1)) & 1u) ? p.y : 0.0f;
        p.z = ((a.obs_mask >> (4 * q + 2)) & 1u) ? p.z : 0.0f;
        p.w = ((a.obs_mask >> (4 * q + 3)) & 1u) ? p.w : 0.0f;
        zb = fma((double)x.x, (double)bq.x, zb); ze = fma((double)x.x, (double)fq.x, ze); zp = fma((double)x.x, (double)p.x, zp);
        zb = fma((double)x.y, (double)bq.y, zb); ze = fma((double)x.y, (double)fq.y, ze); zp = fma((double)x.y, (double)p.y, zp);
        zb = fma((double)x.z, (double)bq.z, zb); ze = fma((double)x.z, (double)fq.z, ze); zp = fma((double)x.z, (double)p.z, zp);
        zb = fma((double)x.w, (double)bq.w, zb); ze = fma((double)x.w, (double)fq.w, ze); zp = fma((double)x.w, (double)p.w, zp);
      }
      const float4 x7 = xp[GATE_QUAD];
      float uf = 0.0f;
      if (SAMPLE) {
        const uint32_t u = (uint32_t)(w2a_mix64(pstream + (uint64_t)(t + 1) * 0x9E3779B97F4A7C15ull) >> 32);
        uf = (float)u * 2.3283064365386963e-10f;
      }
      uint32_t flags = x7.z > 0.5f ? PC_FLAG_HEAT : 0u;
      if (GATE) {  // a day past the bitmap is not allowed (gate_allows)
        const uint32_t wi = t >> 5;
        const uint32_t gw = wi < (uint32_t)a.gate_words ? a.gate[(size_t)pe_id * a.gate_words + wi] : 0u;
        flags |= ((gw >> (t & 31)) & 1u) ? PC_FLAG_OPEN : 0u;
      }
      s_pb[lane] = zb; s_pe[lane] = ze; s_pp[lane] = zp;  // lane == pi * D + pd
      s_tl[lane] = make_float4(x7.x, x7.y, uf, __uint_as_float(flags));
    }
    __syncthreads();
    // ---- tail phase: budget b of env ti through the block's days
    for (uint32_t dd = 0; dd < D && s0 + dd < h.H; ++dd) {
      const uint32_t t = h.t0 + s0 + dd;
      const uint32_t entry = ti * D + dd;
      const float4 tq = s_tl[entry];
      const uint32_t flags = __float_as_uint(tq.w);
      // ---- policy: alert iff logit > 0, or u < sigmoid(logit)
      int32_t act;
      if (SAMPLE) act = (tq.z < sigmoid_f32((float)z)) ? 1 : 0;
      else act = z > 0.0 ? 1 : 0;
      if (a.require_budget && rem <= 0) act = 0;
      if (GATE && !(flags & PC_FLAG_OPEN)) act = 0;  // not attempted
      // ---- env.py:242-250
      const uint32_t atb_s = rem == 0 ? 1u : 0u;
      const uint32_t actual = (act == 1 && atb_s) ? 0u : (uint32_t)act;
      const int32_t rem2 = rem - (int32_t)actual;
      const uint32_t hist2 = ((hist << 1) | actual) & 0x3FFFu;
      float xr[6];
      xr[0] = (t > 0) ? (float)actual : 0.0f;
      xr[1] = (float)streak;
      xr[2] = (float)rem2;
      xr[3] = (float)__popc(hist2);
      xr[4] = tq.x;
      xr[5] = tq.y;
      double zb = s_pb[entry], ze = s_pe[entry], zp = s_pp[entry];
#pragma unroll
      for (int k = 0; k < 6; ++k) {  // slots 24..29
        const double xk = (double)xr[k];
        zb = fma(xk, (double)wb[k], zb);
        ze = fma(xk, (double)we[k], ze);
        zp = fma(xk, (double)wp[k], zp);
      }
      if (!(flags & PC_FLAG_HEAT)) ze = -__builtin_inf();
      float r = reward_from_logits(zb, ze, actual);
      asm volatile("" : "+v"(r));  // the reward is rounded to f32 before it is added, as in the rollout kernels (no fma)
      ret += r;
      alerts += (int32_t)actual;
      over += (act == 1 && atb_s) ? 1 : 0;
      if (SCHED) {
        for (; w < nw && w < (t >> 5); ++w) {  // the words before the day's are complete
          a.mask[row * nw + w] = word;
          word = 0;
        }
        if (actual) word |= 1u << (t & 31u);
      }
      rem = rem2; hist = hist2;
      if (t + 1 < h.ndays) streak = actual ? streak + 1 : 0;
      z = zp;
    }
    __syncthreads();  // the block's entries are read before the next block's go in
  }
  if (t_ok) {
    if (SCHED)
      for (; w < nw; ++w) {  // every word of the row is written exactly once
        a.mask[row * nw + w] = word;
        word = 0;
      }
    a.ret[row] = h.bad ? __builtin_nanf("") : ret;
    a.alerts[row] = alerts;
    a.over[row] = over;
  }
}

#endif  // W2A_POLICY_CURVE_HIP_H
