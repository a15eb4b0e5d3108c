// w2a_hindsight_curve.hip.h -- k_hs_curve: every env's hindsight optimum for EVERY remaining budget 0 .. B in one sweep
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_HINDSIGHT_CURVE_HIP_H
#define W2A_HINDSIGHT_CURVE_HIP_H

// ----------------------------------------------------------------------------------------
// hindsight budget curve (w2a_hindsight_curve)
// ----------------------------------------------------------------------------------------
// The reward of a day reads the agent through alert_lag1, the pre-update streak and the REMAINING budget
// (w2a_hindsight.hip.h), so over (r = alerts remaining, s = streak) one value table is exact for every starting budget:
//   V_d(r, s) = max( r0 + V_{d+1}(r, 0),  r1 + V_{d+1}(r - 1, s + 1) ),  the second only while r > 0 (and the gate is
// open), and column b of the answer is V_0(b, s0). k_hs_dp cannot serve: its state is "alerts issued j" against ONE
// budget, its row j holds the streaks k <= j and the one slot s0 + j, and rows j > d are never formed -- "as if B - b
// alerts were already issued, streak s0" is not among its states.
//   States. At r remaining, an optimum of SOME budget b <= B has issued b - r <= B - r alerts, so its streak is either
//   one begun inside the horizon, m = 0 .. B - r (family 0), or the start streak still unbroken, s0 + m with
//   m = 0 .. B - r (family 1; at s0 = 0 the two hold the same values). 2 (B - r + 1) states per r, (B + 1)(B + 2) in
//   all: about twice hs_ns(B).
//   Index: m-major, so that the states some budget can reach on day d (m <= d) are a prefix. Group m starts at
//   off(m) = m (2 B + 3 - m) and holds, for each family, the B - m + 1 states i = 0 .. B - m with r = B - m - i:
//     idx(m, f, i) = off(m) + f (B - m + 1) + i;   no alert -> (0, 0, m + i) = m + i;   alert -> (m + 1, f, i)
//   (an alert needs r >= 1, i.e. i <= B - m - 1, which is group m + 1's width). The start of budget b is (0, 1, B - b).
//   On day d only groups m <= min(d, B) are formed (a speed matter: the values of the others are never read).
//   Mapping: one 64-lane workgroup per env, lanes over the day's states in chunks of 64 in the sweep and over BUDGETS in
//   the backtrack (lane l walks budget c0 + l through the decision words; B + 1 > 64 loops). B is the same for every
//   env of a call, so there is no binning by U and one launch serves the batch; an env with nothing to choose
//   (finished, t >= n_days) or a start outside the tables writes its rows of 0 / NaN itself and leaves.
//   Memory: dynamic LDS holds the day statics (32 B per day, always), the double-buffered V (16 B per state) and one
//   ballot word per 64-state chunk and day, which stay until the last budget chunk is walked; when that exceeds
//   HS_LDS_CAP, GLOBAL = true keeps V and the words in the caller's workspace through the same code.
//   Numerics: the sweep is k_hs_dp's statement for statement -- hs_reward with rem = r (no alert) and r - 1 (alert),
//   the integers k_hs_dp passes for the twin whose remaining budget is that value, q = (double)reward + V, alert only
//   if q1 > q0 -- so V_d(r, s) is the twin's value bit for bit, and the backtrack re-adds the chosen rewards in f32 in
//   day order behind the same barrier: return[e][b] is bit-identical to k_hs_dp's return for budget = used + b.
//   No atomics; identical calls give identical bits; nothing is written but the outputs and the workspace.
#define HC_MAX_BUDGET (HS_BINS - 1)

__host__ __device__ __forceinline__ uint32_t hc_off(uint32_t m, uint32_t B) { return m * (2u * B + 3u - m); }
__host__ __device__ __forceinline__ uint32_t hc_ns(uint32_t B) { return (B + 1u) * (B + 2u); }
__host__ __device__ __forceinline__ uint32_t hc_nc(uint32_t B) { return (hc_ns(B) + 63u) / 64u; }
// bytes of V + decision words of one env at B over hb days (LDS or workspace)
__host__ __device__ __forceinline__ size_t hc_dp_bytes(uint32_t B, uint32_t hb) {
  return 16ull * hc_ns(B) + 8ull * hb * hc_nc(B);
}

struct HcArgs {
  HsArgs h;   // ret, alerts: [n][B + 1]; mask: NULL or [n][B + 1][mask_words]; the binning fields are not used
  int32_t B;  // max_budget
};

__device__ __forceinline__ uint32_t hc_group(uint32_t idx, uint32_t B) {  // m of state idx: off(m) <= idx < off(m + 1)
  const float a = (float)(2u * B + 3u);
  uint32_t m = (uint32_t)((a - __builtin_sqrtf(a * a - 4.0f * (float)idx)) * 0.5f);
  m = min(m, B);
  while (m > 0 && hc_off(m, B) > idx) --m;
  while (m < B && hc_off(m + 1u, B) <= idx) ++m;
  return m;
}

// one env per 64-lane workgroup: env e0 + blockIdx.x. GLOBAL: V and the decision words live in `pool` (pool_stride
// bytes per workgroup) instead of LDS. GATE: the alert transition exists only on the days a.gate allows.
template <bool GLOBAL, bool GATE>
__global__ __launch_bounds__(HS_BLOCK) void k_hs_curve(const HcArgs ca, uint32_t e0, char *pool, size_t pool_stride) {
  extern __shared__ __attribute__((aligned(16))) char hs_lds[];
  const HsArgs &a = ca.h;
  const uint32_t lane = threadIdx.x;
  const uint32_t e = e0 + blockIdx.x;
  const uint32_t B = (uint32_t)ca.B;
  const HsEnv h = hs_env(a, e);
  const uint32_t H = h.H, hb = (uint32_t)a.hb;
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
  double2 *pz = reinterpret_cast<double2 *>(hs_lds);                  // [hb] prefixes over slots 0..23 (b, e)
  float4 *tl = reinterpret_cast<float4 *>(hs_lds + 16 * (size_t)hb);  // [hb] x28, x29, gate, -
  char *dp = GLOBAL ? pool + (size_t)blockIdx.x * pool_stride : hs_lds + hs_day_bytes(hb);
  double *V0 = reinterpret_cast<double *>(dp);
  double *V1 = V0 + NS;
  uint64_t *dec = reinterpret_cast<uint64_t *>(V1 + NS);              // [hb][NC]

  // the env's own coefficient rows (wave-uniform), f32 as stored
  const float4 *wq = a.tb.W + (size_t)h.wrow * (2 * ROWF / 4);
  hs_day_statics(a, h, wq, lane, pz, tl);
  const HsCoef c = hs_load_coef(wq);
  for (uint32_t i = lane; i < NS; i += HS_BLOCK) V1[i] = 0.0;  // V_H = 0
  __syncthreads();

  // ---- backward DP: V_{d+1} in vn, V_d into vc
  double *vn = V1, *vc = V0;
  uint32_t gate_word = 0, gate_idx = 0xFFFFFFFFu;
  for (int32_t d = (int32_t)H - 1; d >= 0; --d) {
    const bool open = !GATE || gate_allows(a.gate, a.gate_words, e, h.t0 + (uint32_t)d, gate_word, gate_idx);
    const uint32_t nsd = hc_off(min((uint32_t)d, B) + 1u, B);  // groups m <= d: what some budget reaches on day d
    const double2 p = pz[d];
    const float4 tq = tl[d];
    const bool day0 = (h.t0 + (uint32_t)d) == 0u, gate = tq.z != 0.0f;
    for (uint32_t c0 = 0; c0 < nsd; c0 += HS_BLOCK) {
      const uint32_t idx = c0 + lane;
      const bool valid = idx < nsd;
      bool alert = false;
      if (valid) {
        const uint32_t m = hc_group(idx, B), wd = B - m + 1u, pos = idx - hc_off(m, B);
        const uint32_t f = pos >= wd ? 1u : 0u, i = pos - f * wd;
        const float s = (float)(f ? h.s0 + m : m);
        const int32_t rem = (int32_t)(B - m - i);
        const bool allowed = rem > 0 && open;
        const float r0 = hs_reward(c, p.x, p.y, tq.x, tq.y, gate, day0, s, rem, 0u);
        const double q0 = (double)r0 + vn[m + i];
        double best = q0;
        if (allowed) {
          const float r1 = hs_reward(c, p.x, p.y, tq.x, tq.y, gate, day0, s, rem - 1, 1u);
          const double q1 = (double)r1 + vn[hc_off(m + 1u, B) + f * (B - m) + i];
          alert = q1 > q0;
          best = alert ? q1 : q0;
        }
        vc[idx] = best;
      }
      const uint64_t bits = __ballot(alert);
      if (lane == 0) dec[(size_t)d * NC + c0 / HS_BLOCK] = bits;
    }
    __syncthreads();
    double *tmp = vn; vn = vc; vc = tmp;
  }

  // ---- backtrack, lanes over budgets: lane l walks budget b0 + l from (b, s0), re-adding the chosen rewards in f32 in
  // day order; its schedule leaves word by word (every word of the row is written exactly once)
  for (uint32_t b0 = 0; b0 <= B; b0 += HS_BLOCK) {
    const uint32_t b = b0 + lane;
    if (b > B) continue;
    const size_t row = (size_t)e * (B + 1u) + b;
    uint32_t m = 0, f = 1u, i = B - b, n_alerts = 0, w = 0, word = 0;
    float ret = 0.0f;
    for (uint32_t d = 0; d < H; ++d) {
      const uint32_t tt = h.t0 + d;
      for (; w < nw && w < (tt >> 5); ++w) {  // the words before the day's are complete
        a.mask[row * nw + w] = word;
        word = 0;
      }
      const uint32_t idx = hc_off(m, B) + f * (B - m + 1u) + i;
      const uint32_t act = (uint32_t)(dec[(size_t)d * NC + (idx >> 6)] >> (idx & 63u)) & 1u;
      const double2 p = pz[d];
      const float4 tq = tl[d];
      const float s = (float)(f ? h.s0 + m : m);
      float r = hs_reward(c, p.x, p.y, tq.x, tq.y, tq.z != 0.0f, tt == 0u, s, (int32_t)(B - m - i) - (int32_t)act, act);
      asm volatile("" : "+v"(r));  // the reward is rounded to f32 before it is added, as in the rollout kernels (no fma)
      ret += r;
      if (act) word |= 1u << (tt & 31u);
      n_alerts += act;
      if (act) {
        m += 1u;
      } else {
        i += m; m = 0; f = 0;
      }
    }
    for (; w < nw; ++w) {
      a.mask[row * nw + w] = word;
      word = 0;
    }
    a.ret[row] = ret;
    a.alerts[row] = (int32_t)n_alerts;
  }
}

#endif  // W2A_HINDSIGHT_CURVE_HIP_H
