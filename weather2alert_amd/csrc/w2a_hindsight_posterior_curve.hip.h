// w2a_hindsight_posterior_curve.hip.h -- k_hs_pm_curve: every env's hindsight optimum WITH THE DRAW UNKNOWN for EVERY
// remaining budget 0 .. B in one sweep: k_hs_curve's sweep and backtrack on k_hs_pm_dp's reward
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_HINDSIGHT_POSTERIOR_CURVE_HIP_H
#define W2A_HINDSIGHT_POSTERIOR_CURVE_HIP_H

// ----------------------------------------------------------------------------------------
// draw-blind hindsight budget curve (w2a_hindsight_posterior_curve)
// ----------------------------------------------------------------------------------------
// The state space, the index, the transitions, the day pruning and the strict comparison are k_hs_curve's
// (w2a_hindsight_curve.hip.h): (B + 1)(B + 2) states over (r = alerts remaining, family, m) by hc_off / hc_ns / hc_nc /
// hc_group, m-major, groups m <= min(d, B) on day d, an alert only if q1 > q0. Only the reward a state weighs changes,
// and it is k_hs_pm_dp's (w2a_hindsight_posterior.hip.h): with K = n_samples,
//     m_a = ( sum over i = 0 .. K - 1 of (double) hs_reward(draw i's coefficients and prefixes, rem) ) / (double) K,
// rem = r without an alert and r - 1 with one -- the integers k_hs_pm_dp passes for the twin whose remaining budget is
// that value -- the sum in fp64, sequential in i from 0, in one lane (no cross-lane combination, no atomics). So
// V_d(r, s) is the twin's value bit for bit (hc_pm_state below is hs_pm_state with k_hs_curve's index).
//   Mapping: one 64-lane workgroup per env, one launch for the batch (B is uniform), as k_hs_curve. Per day of the
//   sweep, lanes over draws re-form that day's prefixes behind one barrier, exactly as k_hs_pm_dp does; then lanes over
//   the day's states in chunks of 64.
//   Backtrack: lanes over BUDGETS (lane l walks budget b0 + l through the decision words; B + 1 > 64 loops). Per day the
//   prefixes of every draw are re-formed once for the workgroup (lanes over draws, hs_prefix: the sweep's bits) and each
//   lane adds its own path's K rewards in draw order in fp64, divides by (double) K and adds the day's mean to its
//   fp64 return: the sum k_hs_pm_dp's backtrack forms from its LDS staging, in the same order, so return[e][b] is
//   k_hs_pm_dp's for budget = used + b bit for bit, rounded once to f32. All 64 lanes take every barrier; lanes beyond
//   B only help re-form the prefixes.
//   Memory: dynamic LDS holds k_hs_pm_dp's fixed part (hs_pm_fixed_bytes: 16 B per day of tails, per draw 80 B of
//   run-time coefficients and 16 B of one day's prefixes), then V and the decision words (hc_dp_bytes); beyond
//   HS_LDS_CAP, GLOBAL = true keeps V and the words in the caller's pool through the same code. B >= 63 is always
//   GLOBAL (16 * hc_ns(63) > 64 KB); the largest n_samples is k_hs_pm_dp's (657 at 153 days).
//   No atomics; identical calls give identical bits; nothing is written but the outputs and the workspace.
//   Resources (gfx950, -O3, the compiler's report): 117 VGPRs, no AGPRs, 106 SGPRs and 0 bytes of scratch in all four
//   <GLOBAL, GATE> instantiations (k_hs_curve 124 VGPRs, k_hs_pm_dp 162); no static LDS, dynamic LDS as above.

struct HcPmState {
  bool alert;   // the DP takes the alert
  double best;  // V_d of the state
};

// hs_pm_state on k_hs_curve's index: state idx = (m, f, i) on a day whose per-draw prefixes are pp[0 .. K)
// (coefficients cf[0 .. K), both wave-uniform LDS reads) and whose tail is tq, V_{d+1} in vn. The loop over the draws
// is hs_pm_state's statement for statement, with rem = r = B - m - i in the place of the twin's budget - used - j.
__device__ __forceinline__ HcPmState hc_pm_state(const HsCoef *cf, const double2 *pp, uint32_t K, double dK, const HsEnv &h,
                                                 uint32_t B, bool open, float4 tq, bool gate, bool day0, const double *vn,
                                                 uint32_t idx) {
  const uint32_t m = hc_group(idx, B), wd = B - m + 1u, pos = idx - hc_off(m, B);
  const uint32_t f = pos >= wd ? 1u : 0u, i0 = pos - f * wd;
  const float s = (float)(f ? h.s0 + m : m);
  const int32_t rem = (int32_t)(B - m - i0);
  HcPmState r;
  const bool allowed = rem > 0 && open;
  double s0 = 0.0, s1 = 0.0;
  for (uint32_t i = 0; i < K; ++i) {  // draws in order: the sums' one order
    const HsCoef c = cf[i];
    const double2 p = pp[i];
    s0 += (double)hs_reward(c, p.x, p.y, tq.x, tq.y, gate, day0, s, rem, 0u);
    if (allowed) s1 += (double)hs_reward(c, p.x, p.y, tq.x, tq.y, gate, day0, s, rem - 1, 1u);
  }
  const double q0 = s0 / dK + vn[m + i0];
  r.best = q0;
  r.alert = false;
  if (allowed) {
    const double q1 = s1 / dK + vn[hc_off(m + 1u, B) + f * (B - m) + i0];
    r.alert = q1 > q0;
    r.best = r.alert ? q1 : q0;
  }
  return r;
}

// one env per 64-lane workgroup: env e0 + blockIdx.x; GLOBAL, GATE, pool as k_hs_curve
template <bool GLOBAL, bool GATE>
__global__ __launch_bounds__(HS_BLOCK) void k_hs_pm_curve(const HcArgs ca, uint32_t e0, char *pool, size_t pool_stride) {
  extern __shared__ __attribute__((aligned(16))) char hs_lds[];
  const HsArgs &a = ca.h;
  const uint32_t lane = threadIdx.x;
  const uint32_t e = e0 + blockIdx.x;
  const uint32_t B = (uint32_t)ca.B;
  const HsEnv h = hs_env(a, e);
  const uint32_t H = h.H, hb = (uint32_t)a.hb, K = (uint32_t)a.tb.n_samples;
  const uint32_t nw = a.mask ? (uint32_t)a.mask_words : 0u;
  if (h.bad || H == 0) {  // no DP: rows of 0 (NaN: a start outside the tables), no alerts, empty schedules
    const float fill = h.bad ? __builtin_nanf("") : 0.0f;
    for (uint32_t b = lane; b <= B; b += HS_BLOCK) {
      const size_t row = (size_t)e * (B + 1u) + b;
      a.ret[row] = fill;
      a.alerts[row] = 0;
    }
    for (size_t w = lane; w < (size_t)(B + 1u) * nw; w += HS_BLOCK) a.mask[(size_t)e * (B + 1u) * nw + w] = 0u;
    return;
  }
  const uint32_t NS = hc_ns(B), NC = hc_nc(B);
  float4 *tl = reinterpret_cast<float4 *>(hs_lds);                                   // [hb] x28, x29, gate, -
  HsCoef *cf = reinterpret_cast<HsCoef *>(hs_lds + 16 * (size_t)hb);                 // [K] run-time coefficients
  double2 *pp = reinterpret_cast<double2 *>(hs_lds + 16 * (size_t)hb + 80 * (size_t)K);  // [K] one day's prefixes (b, e)
  char *dp = GLOBAL ? pool + (size_t)blockIdx.x * pool_stride : hs_lds + hs_pm_fixed_bytes(hb, K);
  double *V0 = reinterpret_cast<double *>(dp);
  double *V1 = V0 + NS;
  uint64_t *dec = reinterpret_cast<uint64_t *>(V1 + NS);           // [hb][NC]

  // the coefficient rows of draw 0 of the env's column (wave-uniform), f32 as stored; draw i is 2 * ROWF / 4 quads on
  const float4 *w0 = a.tb.W + (size_t)((uint32_t)a.st.coef_col[e] * K) * (2 * ROWF / 4);
  const uint32_t rows_per_day = (uint32_t)(a.tb.S_w * a.tb.Y);
  // ---- day tails: lanes over days; run-time coefficients: lanes over draws
  for (uint32_t d = lane; d < H; d += HS_BLOCK)
    tl[d] = hs_day_tail(a.tb.X[(size_t)((h.t0 + d) * rows_per_day + h.ep_row) * (ROWF / 4) + GATE_QUAD]);
  for (uint32_t i = lane; i < K; i += HS_BLOCK) cf[i] = hs_load_coef(w0 + (size_t)i * (2 * ROWF / 4));
  const double dK = (double)K;
  for (uint32_t i = lane; i < NS; i += HS_BLOCK) V1[i] = 0.0;  // V_H = 0
  __syncthreads();

  // ---- backward DP: V_{d+1} in vn, V_d into vc
  double *vn = V1, *vc = V0;
  uint32_t gate_word = 0, gate_idx = 0xFFFFFFFFu;
  for (int32_t d = (int32_t)H - 1; d >= 0; --d) {
    const float4 *xp = a.tb.X + (size_t)((h.t0 + (uint32_t)d) * rows_per_day + h.ep_row) * (ROWF / 4);
    for (uint32_t i = lane; i < K; i += HS_BLOCK) pp[i] = hs_prefix(xp, w0 + (size_t)i * (2 * ROWF / 4));
    __syncthreads();
    const bool open = !GATE || gate_allows(a.gate, a.gate_words, e, h.t0 + (uint32_t)d, gate_word, gate_idx);
    const uint32_t nsd = hc_off(min((uint32_t)d, B) + 1u, B);  // groups m <= d: what some budget reaches on day d
    const float4 tq = tl[d];
    const bool day0 = (h.t0 + (uint32_t)d) == 0u, gate = tq.z != 0.0f;
    for (uint32_t c0 = 0; c0 < nsd; c0 += HS_BLOCK) {
      const uint32_t idx = c0 + lane;
      const bool valid = idx < nsd;
      bool alert = false;
      if (valid) {
        const HcPmState st = hc_pm_state(cf, pp, K, dK, h, B, open, tq, gate, day0, vn, idx);
        alert = st.alert;
        vc[idx] = st.best;
      }
      const uint64_t bits = __ballot(alert);
      if (lane == 0) dec[(size_t)d * NC + c0 / HS_BLOCK] = bits;
    }
    __syncthreads();  // the day's prefixes have been read, V_d and its decisions are written
    double *tmp = vn; vn = vc; vc = tmp;
  }

  // ---- backtrack, lanes over budgets: lane l walks budget b0 + l from (b, s0). Per day the workgroup re-forms the
  // prefixes of every draw, then each lane adds its path's rewards in draw order and the day's mean in fp64 in day
  // order; its schedule leaves word by word (every word of the row is written exactly once)
  for (uint32_t b0 = 0; b0 <= B; b0 += HS_BLOCK) {
    const uint32_t b = b0 + lane;
    const bool walk = b <= B;  // the others take the barriers and help with the prefixes
    const size_t row = (size_t)e * (B + 1u) + (walk ? b : 0u);
    uint32_t m = 0, f = 1u, i0 = walk ? B - b : 0u, n_alerts = 0, w = 0, word = 0;
    double ret = 0.0;
    for (uint32_t d = 0; d < H; ++d) {
      const uint32_t tt = h.t0 + d;
      const float4 *xp = a.tb.X + (size_t)(tt * rows_per_day + h.ep_row) * (ROWF / 4);
      for (uint32_t i = lane; i < K; i += HS_BLOCK) pp[i] = hs_prefix(xp, w0 + (size_t)i * (2 * ROWF / 4));
      __syncthreads();
      if (walk) {
        for (; w < nw && w < (tt >> 5); ++w) {  // the words before the day's are complete
          a.mask[row * nw + w] = word;
          word = 0;
        }
        const uint32_t idx = hc_off(m, B) + f * (B - m + 1u) + i0;
        const uint32_t act = (uint32_t)(dec[(size_t)d * NC + (idx >> 6)] >> (idx & 63u)) & 1u;
        const float4 tq = tl[d];
        const float s = (float)(f ? h.s0 + m : m);
        const int32_t rem = (int32_t)(B - m - i0) - (int32_t)act;
        double sum = 0.0;
        for (uint32_t i = 0; i < K; ++i) {  // draws in order, as the sweep
          const double2 p = pp[i];
          sum += (double)hs_reward(cf[i], p.x, p.y, tq.x, tq.y, tq.z != 0.0f, tt == 0u, s, rem, act);
        }
        ret += sum / dK;
        if (act) word |= 1u << (tt & 31u);
        n_alerts += act;
        if (act) {
          m += 1u;
        } else {
          i0 += m; m = 0; f = 0;
        }
      }
      __syncthreads();  // pp is free for the next day
    }
    if (walk) {
      for (; w < nw; ++w) {
        a.mask[row * nw + w] = word;
        word = 0;
      }
      a.ret[row] = (float)ret;
      a.alerts[row] = (int32_t)n_alerts;
    }
  }
}

#endif  // W2A_HINDSIGHT_POSTERIOR_CURVE_HIP_H
