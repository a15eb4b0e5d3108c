// w2a_hindsight_posterior.hip.h -- k_hs_pm_dp: every env's best alert schedule in hindsight when the weather is known
// and the env's posterior draw is NOT: the exact DP of k_hs_dp on the reward averaged over all draws of the env's column;
// k_hs_pm_along: the same DP's values and decisions in the states a given schedule reaches
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_HINDSIGHT_POSTERIOR_HIP_H
#define W2A_HINDSIGHT_POSTERIOR_HIP_H

// ----------------------------------------------------------------------------------------
// hindsight optimum of the posterior mean (w2a_hindsight_posterior)
// ----------------------------------------------------------------------------------------
// The state space, the transitions, the day pruning and the strict comparison are k_hs_dp's (w2a_hindsight.hip.h):
// states (j, k) by hs_ns / hs_nc / hs_row, (j, k) -> (j, 0) and (j, k) -> (j + 1, k + 1), the alert only while
// j < budget - used on an open day, taken only if q1 > q0. Only the reward a state weighs changes. With K = n_samples
// and r_a^(i) = hs_reward with the prefixes and coefficients of draw i of the env's column (row coef_col * K + i of W)
// -- bit for bit the f32 reward an env holding draw i pays in that state -- the DP weighs
//     m_a = ( sum over i = 0 .. K - 1 of (double) r_a^(i) ) / (double) K,
// the sum in fp64, sequential in i from 0 (one lane adds all draws of its state: no cross-lane combination, no atomics,
// identical calls give identical bits). The return is the fp64 sum in day order of the chosen m_a along the backtracked
// path, rounded once to f32. `sample` is read only by hs_env's range check. With K = 1, m_a = (double) r_a exactly and
// every comparison is k_hs_dp's: the schedule and the count are bit-identical, the return agrees to f32 rounding.
//   Mapping: one 64-lane workgroup per env, binned by U with k_hs_plan / k_hs_scatter as they are. LDS per env: 16 B per
//   day (x28, x29, the heat gate: k_hs_dp's tail; its 16 B per day of prefixes have no place here, they depend on the
//   draw), per draw the run-time coefficients (HsCoef, 80 B, filled once) and ONE day's two fp64 prefixes over slots
//   0..23 (16 B), then V and the decision words as in k_hs_dp (GLOBAL: in the caller's pool).
//   Per day of the backward sweep, lanes over draws (lane, lane + 64, ...) form that day's prefixes of every draw with
//   hs_prefix, the FMA chain of k_hs_dp's statics; one barrier; then k_hs_dp's state loop with the two hs_reward calls inside
//   a loop over draws whose prefixes and coefficients are wave-uniform LDS reads. The coefficient rows of slots 0..23
//   (192 B per draw) are re-read from L2 every day rather than kept in registers: draws per lane are a run-time number,
//   two draws would take 96 VGPRs, and the reads (19 KB per env-day at K = 100) are two orders below the state loop's
//   arithmetic.
//   The backtrack walks the path with lanes over draws: each lane re-forms its draws' prefixes of the path's day and the
//   chosen reward, leaves (double) r^(i) in LDS, and after a barrier every lane adds them in draw order -- the same sum
//   and the same bits as the sweep's m_a.
__host__ __device__ __forceinline__ size_t hs_pm_fixed_bytes(uint32_t hb, uint32_t K) { return 16ull * hb + 96ull * K; }

// hs_state on the draw-mean reward: state idx = (j, k) on a day whose per-draw prefixes are pp[0 .. K) (coefficients
// cf[0 .. K), both wave-uniform LDS reads) and whose tail is tq, V_{d+1} in vn. The sums run over the draws in draw
// order in fp64: k_hs_pm_dp and k_hs_pm_along weigh the same bits by construction.
__device__ __forceinline__ HsState hs_pm_state(const HsCoef *cf, const double2 *pp, uint32_t K, double dK, const HsEnv &h,
                                               int32_t rem0, bool open, float4 tq, bool gate, bool day0, const double *vn,
                                               uint32_t idx) {
  const uint32_t j = hs_row(idx), k = idx - j * (j + 3u) / 2u;
  const float s = (float)(k == j + 1u ? h.s0 + j : k);
  const int32_t rem = h.budget - (int32_t)(h.used + j);
  HsState r;
  r.allowed = (int32_t)j < rem0 && open;
  double s0 = 0.0, s1 = 0.0;
  for (uint32_t i = 0; i < K; ++i) {  // draws in order: the sums' one order
    const HsCoef c = cf[i];
    const double2 p = pp[i];
    s0 += (double)hs_reward(c, p.x, p.y, tq.x, tq.y, gate, day0, s, rem, 0u);
    if (r.allowed) s1 += (double)hs_reward(c, p.x, p.y, tq.x, tq.y, gate, day0, s, rem - 1, 1u);
  }
  r.q0 = s0 / dK + vn[j * (j + 3u) / 2u];
  r.best = r.q0; r.q1 = r.q0;
  r.alert = false;
  if (r.allowed) {
    r.q1 = s1 / dK + vn[(j + 1u) * (j + 4u) / 2u + k + 1u];
    r.alert = r.q1 > r.q0;
    r.best = r.alert ? r.q1 : r.q0;
  }
  return r;
}

// one env per 64-lane workgroup; list, U, GLOBAL, GATE, pool as k_hs_dp
template <bool GLOBAL, bool GATE>
__global__ __launch_bounds__(HS_BLOCK) void k_hs_pm_dp(const HsArgs a, const uint32_t *list, uint32_t U, char *pool,
                                                       size_t pool_stride) {
  extern __shared__ __attribute__((aligned(16))) char hs_lds[];
  const uint32_t lane = threadIdx.x;
  const uint32_t e = list[blockIdx.x];
  const HsEnv h = hs_env(a, e);
  const uint32_t H = h.H, hb = (uint32_t)a.hb, K = (uint32_t)a.tb.n_samples;
  const uint32_t NCU = hs_nc(U);
  float4 *tl = reinterpret_cast<float4 *>(hs_lds);                                   // [hb] x28, x29, gate, -
  HsCoef *cf = reinterpret_cast<HsCoef *>(hs_lds + 16 * (size_t)hb);                 // [K] run-time coefficients
  double2 *pp = reinterpret_cast<double2 *>(hs_lds + 16 * (size_t)hb + 80 * (size_t)K);  // [K] one day's prefixes (b, e)
  double *rr = reinterpret_cast<double *>(pp);                                       // [K] the backtrack's rewards
  char *dp = GLOBAL ? pool + (size_t)blockIdx.x * pool_stride : hs_lds + hs_pm_fixed_bytes(hb, K);
  double *V0 = reinterpret_cast<double *>(dp);
  double *V1 = V0 + hs_ns(U);
  uint64_t *dec = reinterpret_cast<uint64_t *>(V1 + hs_ns(U));     // [hb][NCU]

  // the coefficient rows of draw 0 of the env's column (wave-uniform), f32 as stored; draw i is 2 * ROWF / 4 quads on
  const float4 *w0 = a.tb.W + (size_t)((uint32_t)a.st.coef_col[e] * K) * (2 * ROWF / 4);
  const uint32_t rows_per_day = (uint32_t)(a.tb.S_w * a.tb.Y);
  // ---- day tails: lanes over days; run-time coefficients: lanes over draws
  for (uint32_t d = lane; d < H; d += HS_BLOCK)
    tl[d] = hs_day_tail(a.tb.X[(size_t)((h.t0 + d) * rows_per_day + h.ep_row) * (ROWF / 4) + GATE_QUAD]);
  for (uint32_t i = lane; i < K; i += HS_BLOCK) cf[i] = hs_load_coef(w0 + (size_t)i * (2 * ROWF / 4));
  const int32_t rem0 = h.budget - (int32_t)h.used;  // remaining budget at the start; an alert needs j < rem0
  const double dK = (double)K;
  for (uint32_t i = lane; i < hs_ns(U); i += HS_BLOCK) V1[i] = 0.0;  // V_H = 0
  __syncthreads();

  // ---- backward DP: V_{d+1} in vn, V_d into vc
  double *vn = V1, *vc = V0;
  uint32_t gate_word = 0, gate_idx = 0xFFFFFFFFu;
  for (int32_t d = (int32_t)H - 1; d >= 0; --d) {
    const float4 *xp = a.tb.X + (size_t)((h.t0 + (uint32_t)d) * rows_per_day + h.ep_row) * (ROWF / 4);
    for (uint32_t i = lane; i < K; i += HS_BLOCK) pp[i] = hs_prefix(xp, w0 + (size_t)i * (2 * ROWF / 4));
    __syncthreads();
    const bool open = !GATE || gate_allows(a.gate, a.gate_words, e, h.t0 + (uint32_t)d, gate_word, gate_idx);
    const uint32_t J = min((uint32_t)d, U);
    const uint32_t nsd = hs_ns(J);
    const float4 tq = tl[d];
    const bool day0 = (h.t0 + (uint32_t)d) == 0u, gate = tq.z != 0.0f;
    for (uint32_t c0 = 0; c0 < nsd; c0 += HS_BLOCK) {
      const uint32_t idx = c0 + lane;
      const bool valid = idx < nsd;
      bool alert = false;
      if (valid) {
        const HsState st = hs_pm_state(cf, pp, K, dK, h, rem0, open, tq, gate, day0, vn, idx);
        alert = st.alert;
        vc[idx] = st.best;
      }
      const uint64_t bits = __ballot(alert);
      if (lane == 0) dec[(size_t)d * NCU + c0 / HS_BLOCK] = bits;
    }
    __syncthreads();  // the day's prefixes have been read, V_d and its decisions are written
    double *tmp = vn; vn = vc; vc = tmp;
  }

  // ---- backtrack from (0, s0): lanes over draws re-form the chosen rewards, every lane adds them in draw order and
  // the days' means in fp64 in day order (every lane the same path)
  uint32_t j = 0, k = h.s0 > 0 ? 1u : 0u, n_alerts = 0, word = 0;
  double ret = 0.0;
  for (uint32_t d = 0; d < H; ++d) {
    const uint32_t idx = j * (j + 3u) / 2u + k;
    const uint32_t act = (uint32_t)(dec[(size_t)d * NCU + (idx >> 6)] >> (idx & 63u)) & 1u;
    const float4 tq = tl[d];
    const uint32_t tt = h.t0 + d;
    const float s = (float)(k == j + 1u ? h.s0 + j : k);
    const int32_t rem = h.budget - (int32_t)(h.used + j + act);
    const float4 *xp = a.tb.X + (size_t)(tt * rows_per_day + h.ep_row) * (ROWF / 4);
    for (uint32_t i = lane; i < K; i += HS_BLOCK) {
      const double2 p = hs_prefix(xp, w0 + (size_t)i * (2 * ROWF / 4));
      rr[i] = (double)hs_reward(cf[i], p.x, p.y, tq.x, tq.y, tq.z != 0.0f, tt == 0u, s, rem, act);
    }
    __syncthreads();
    double sum = 0.0;
    for (uint32_t i = 0; i < K; ++i) sum += rr[i];
    ret += sum / dK;
    __syncthreads();  // rr is free for the next day
    if (act && lane == (tt >> 5)) word |= 1u << (tt & 31u);
    n_alerts += act;
    j += act;
    k = act ? k + 1u : 0u;
  }
  hs_store_mask_row(a, e, lane, word);
  if (lane == 0) {
    a.ret[e] = (float)ret;
    a.alerts[e] = (int32_t)n_alerts;
  }
}

// ----------------------------------------------------------------------------------------
// draw-blind hindsight values along a GIVEN schedule (w2a_hindsight_posterior_along)
// ----------------------------------------------------------------------------------------
// k_hs_along's job on k_hs_pm_dp's reward: the sweep above (hs_pm_state: the same sums, the same fp64 values, the same
// strict comparison) keeping, per day, the values of the ONE state a caller's schedule reaches.
//   Forward first, as k_hs_along: every lane walks the schedule (attempts; closed days and attempts without budget are
//   no-ops) and lane 0 leaves the day's state index and the alert issued in the fourth float of tl[d], which k_hs_pm_dp
//   does not use (HS_PATH_ALERT, HS_PATH_EXPERT, HS_PATH_IDX as there).
//   In the sweep the lane whose idx is the path's writes the day's outputs, sets HS_PATH_EXPERT and puts the fp64 loss
//   where the day's x28 and x29 were (tl[d].x, tl[d].y: 8 bytes, and day d's tail is in every lane's registers before
//   the state loop and not read again -- one wave per workgroup, so no lane reads it after the store). LDS, the pool and
//   the largest n_samples are therefore k_hs_pm_dp's (hs_pm_fixed_bytes; the decision words' room is simply not used).
//   Afterwards every lane assembles the expert bitmap and lane 0 adds the losses in fp64 in day order: the regret is
//   their sum, there is no backtrack and no second pass over the draws. No atomics: identical calls give identical bits.
template <bool GLOBAL, bool GATE>
__global__ __launch_bounds__(HS_BLOCK) void k_hs_pm_along(const HsAlongArgs aa, const uint32_t *list, uint32_t U, char *pool,
                                                          size_t pool_stride) {
  extern __shared__ __attribute__((aligned(16))) char hs_lds[];
  const HsArgs &a = aa.h;
  const uint32_t lane = threadIdx.x;
  const uint32_t e = list[blockIdx.x];
  const HsEnv h = hs_env(a, e);
  const uint32_t H = h.H, hb = (uint32_t)a.hb, K = (uint32_t)a.tb.n_samples;
  float4 *tl = reinterpret_cast<float4 *>(hs_lds);                                   // [hb] x28, x29 (then: the loss),
                                                                                     // gate, the path's word
  HsCoef *cf = reinterpret_cast<HsCoef *>(hs_lds + 16 * (size_t)hb);                 // [K] run-time coefficients
  double2 *pp = reinterpret_cast<double2 *>(hs_lds + 16 * (size_t)hb + 80 * (size_t)K);  // [K] one day's prefixes (b, e)
  char *dp = GLOBAL ? pool + (size_t)blockIdx.x * pool_stride : hs_lds + hs_pm_fixed_bytes(hb, K);
  double *V0 = reinterpret_cast<double *>(dp);
  double *V1 = V0 + hs_ns(U);

  // the coefficient rows of draw 0 of the env's column (wave-uniform), f32 as stored; draw i is 2 * ROWF / 4 quads on
  const float4 *w0 = a.tb.W + (size_t)((uint32_t)a.st.coef_col[e] * K) * (2 * ROWF / 4);
  const uint32_t rows_per_day = (uint32_t)(a.tb.S_w * a.tb.Y);
  // ---- day tails: lanes over days; run-time coefficients: lanes over draws
  for (uint32_t d = lane; d < H; d += HS_BLOCK)
    tl[d] = hs_day_tail(a.tb.X[(size_t)((h.t0 + d) * rows_per_day + h.ep_row) * (ROWF / 4) + GATE_QUAD]);
  for (uint32_t i = lane; i < K; i += HS_BLOCK) cf[i] = hs_load_coef(w0 + (size_t)i * (2 * ROWF / 4));
  const int32_t rem0 = h.budget - (int32_t)h.used;  // remaining budget at the start; an alert needs j < rem0
  const double dK = (double)K;
  for (uint32_t i = lane; i < hs_ns(U); i += HS_BLOCK) V1[i] = 0.0;  // V_H = 0
  __syncthreads();

  // ---- forward along the schedule from (0, s0): the state of every day (every lane the same path)
  {
    uint32_t j = 0, k = h.s0 > 0 ? 1u : 0u;
    uint32_t sch_word = 0, sch_idx = 0xFFFFFFFFu, gate_word = 0, gate_idx = 0xFFFFFFFFu;
    for (uint32_t d = 0; d < H; ++d) {
      const uint32_t tt = h.t0 + d;
      uint32_t act = im_label_bits(aa.sched, a.mask_words, e, tt, sch_word, sch_idx);
      if (GATE && !gate_allows(a.gate, a.gate_words, e, tt, gate_word, gate_idx)) act = 0u;  // before the budget test
      if ((int32_t)j >= rem0) act = 0u;  // an attempt with no budget left issues nothing
      if (lane == 0) tl[d].w = __uint_as_float((j * (j + 3u) / 2u + k) | (act ? HS_PATH_ALERT : 0u));
      j += act;
      k = act ? k + 1u : 0u;
    }
  }
  __syncthreads();

  // ---- backward DP (k_hs_pm_dp's: hs_pm_state): V_{d+1} in vn, V_d into vc
  double *vn = V1, *vc = V0;
  uint32_t gate_word = 0, gate_idx = 0xFFFFFFFFu;
  const size_t n = (size_t)a.n;
  for (int32_t d = (int32_t)H - 1; d >= 0; --d) {
    const float4 *xp = a.tb.X + (size_t)((h.t0 + (uint32_t)d) * rows_per_day + h.ep_row) * (ROWF / 4);
    for (uint32_t i = lane; i < K; i += HS_BLOCK) pp[i] = hs_prefix(xp, w0 + (size_t)i * (2 * ROWF / 4));
    __syncthreads();
    const bool open = !GATE || gate_allows(a.gate, a.gate_words, e, h.t0 + (uint32_t)d, gate_word, gate_idx);
    const uint32_t J = min((uint32_t)d, U);
    const uint32_t nsd = hs_ns(J);
    const float4 tq = tl[d];
    const uint32_t path = __float_as_uint(tq.w);
    const bool day0 = (h.t0 + (uint32_t)d) == 0u, gate = tq.z != 0.0f;
    bool mine = false, mine_alert = false;  // this lane holds the path's state of day d
    double mine_loss = 0.0;
    for (uint32_t c0 = 0; c0 < nsd; c0 += HS_BLOCK) {
      const uint32_t idx = c0 + lane;
      if (idx < nsd) {
        const HsState st = hs_pm_state(cf, pp, K, dK, h, rem0, open, tq, gate, day0, vn, idx);
        vc[idx] = st.best;
        if (idx == (path & HS_PATH_IDX)) {
          const size_t o = (size_t)d * n + e;
          mine = true;
          mine_alert = st.alert;
          mine_loss = st.best - ((path & HS_PATH_ALERT) ? st.q1 : st.q0);  // an issued alert was allowed: q1 is its value
          aa.gain[o] = st.allowed ? (float)(st.q1 - st.q0) : __builtin_nanf("");
          if (aa.value) aa.value[o] = (float)st.best;
          if (aa.loss) aa.loss[o] = (float)mine_loss;
        }
      }
    }
    if (mine) {  // day d's tail is in every lane's registers: x28 and x29 make room for the day's loss
      tl[d].x = __int_as_float(__double2loint(mine_loss));
      tl[d].y = __int_as_float(__double2hiint(mine_loss));
      tl[d].w = __uint_as_float(path | (mine_alert ? HS_PATH_EXPERT : 0u));
    }
    __syncthreads();  // the day's prefixes have been read, V_d and the day's results are written
    double *tmp = vn; vn = vc; vc = tmp;
  }

  // ---- the expert's bits along the path (every lane the same days), the regret in fp64 in day order
  uint32_t word = 0;
  for (uint32_t d = 0; d < H; ++d) {
    const uint32_t tt = h.t0 + d;
    if ((__float_as_uint(tl[d].w) & HS_PATH_EXPERT) && lane == (tt >> 5)) word |= 1u << (tt & 31u);
  }
  hs_store_mask_row(a, e, lane, word);
  if (lane == 0) {
    double regret = 0.0;
    for (uint32_t d = 0; d < H; ++d) regret += __hiloint2double(__float_as_int(tl[d].y), __float_as_int(tl[d].x));
    a.ret[e] = (float)regret;
  }
  for (uint32_t s = H + lane; s < hb; s += HS_BLOCK) {  // call-days the env does not step
    const size_t o = (size_t)s * n + e;
    aa.gain[o] = __builtin_nanf("");
    if (aa.value) aa.value[o] = 0.0f;
    if (aa.loss) aa.loss[o] = 0.0f;
  }
}

#endif  // W2A_HINDSIGHT_POSTERIOR_HIP_H
