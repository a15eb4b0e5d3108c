// w2a_hindsight.hip.h -- k_hs_plan / k_hs_scatter / k_hs_dp: every env's best alert schedule in hindsight, by exact DP;
// k_hs_along: the same DP's values and decisions in the states a given schedule reaches
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_HINDSIGHT_HIP_H
#define W2A_HINDSIGHT_HIP_H

// ----------------------------------------------------------------------------------------
// hindsight optimum (w2a_hindsight_optimum)
// ----------------------------------------------------------------------------------------
// Under the faithful semantics the reward of day d reads four run-time slots and nothing else that depends on the
// agent (w2a_posterior_returns.hip.h): 24 alert_lag1 (today's alert, 0 on day 0), 25 the pre-update streak, 26 the
// remaining budget after today's alert, 27 the agent's 14-day count -- whose coefficient is zero (quirk Q1: the
// reference's key is the historical alerts_2wks; the entry refuses tables where it is not). So with j = alerts issued
// inside the horizon and s = the current streak, (j, s) is an exact DP state:
//   V_d(j, s) = max( r0 + V_{d+1}(j, 0),  r1 + V_{d+1}(j + 1, s + 1) ),  the second only while used + j < budget,
// fp64 sums of the f32 rewards, alert only if STRICTLY greater (ties do not alert).
//   State index. Streaks that started inside the horizon are <= j; the one streak that did not (the start streak s0,
//   unbroken since) is s0 + j at j = d. Slot k = 0 .. j + 1 of row j holds streak k (k <= j) or s0 + j (k = j + 1):
//   idx(j, k) = j (j + 3) / 2 + k, NS(U) = (U + 1)(U + 4) / 2 states for j <= U, and both transitions are
//   (j, k) -> (j, 0) and (j, k) -> (j + 1, k + 1). At day d only rows j <= min(d, U) are reachable and computed.
//   Mapping: one 64-lane workgroup (one wave) per env, lanes over the day's states in chunks of 64. Envs are binned by
//   U (k_hs_plan / k_hs_scatter: a counting sort) and each bin is one launch whose dynamic LDS holds exactly its need:
//   per day the static logit prefixes (slots 0..23, fp64, 16 B) and slots 28..30 (16 B), the double-buffered V
//   (2 x 8 B x NS) and one ballot word of decision bits per 64-state chunk and day. Bins whose need exceeds
//   HS_LDS_CAP keep V and the decision words in the caller's workspace instead (the same code through global pointers;
//   large budgets: correct, not fast).
//   Numerics: the prefix over slots 0..23 is the FMA chain of the step / rollout kernels up to slot 23; per state the
//   chain continues over slots 24, 25, 26, 28, 29 in slot order (slot 27's term is +-0 and is left out: the logit can
//   differ from the env's only in the sign of a zero, which no sigmoid sees), then the heat gate and
//   reward_from_logits: every reward the DP weighs is the one the env would pay in that state, bit for bit. The
//   backtrack recomputes the chosen rewards with the same code and adds them in f32 in day order, as the env does.
#define HS_BLOCK 64
#define HS_LDS_CAP (64 * 1024)
#define HS_BINS 1024  // U <= H <= T <= 1023

__host__ __device__ __forceinline__ uint32_t hs_ns(uint32_t U) { return (U + 1u) * (U + 4u) / 2u; }
__host__ __device__ __forceinline__ uint32_t hs_nc(uint32_t U) { return (hs_ns(U) + 63u) / 64u; }
// bytes of V + decision words of one env at U over hb days (LDS or workspace)
__host__ __device__ __forceinline__ size_t hs_dp_bytes(uint32_t U, uint32_t hb) {
  return 16ull * hs_ns(U) + 8ull * hb * hs_nc(U);
}
// bytes of the per-day statics (always LDS)
__host__ __device__ __forceinline__ size_t hs_day_bytes(uint32_t hb) { return 32ull * hb; }

struct HsArgs {
  DevTables tb;
  w2a_state_view st;       // start state (device i32 arrays, w2a_get_state's decoding)
  int32_t n_steps;
  int32_t hb;              // min(n_steps, T): bound of every env's horizon (stride of the decision words)
  int32_t mask_words;
  int64_t n;
  float *ret;              // [n]
  uint32_t *mask;          // [n][mask_words]
  int32_t *alerts;         // [n]
  uint32_t *u_env;         // [n] workspace: U, or HS_NONE / HS_BAD (no DP: k_hs_scatter writes the outputs)
  uint32_t *hist;          // [HS_BINS] workspace: envs per U
  uint32_t *cursor;        // [HS_BINS] workspace: first position of every bin in `order`, advanced by k_hs_scatter
  uint32_t *order;         // [n] workspace: env ids by U
  const uint32_t *gate;    // [n][gate_words] allowed days, the layout of `mask` (w2a_hindsight_optimum_gated; read by the
                           // GATE = true instantiations only): the DP may alert only on a day whose bit is set
  int32_t gate_words;
};
#define HS_NONE 0xFFFFFFFFu  // nothing to choose (finished, or t >= n_days): return 0
#define HS_BAD 0xFFFFFFFEu   // a start outside the tables: return NaN

struct HsEnv {  // one env's start, decoded and range-checked
  uint32_t t0, used, s0, ndays, ep_row, wrow;
  int32_t budget;
  bool bad;
  uint32_t H, U;
};
__device__ __forceinline__ HsEnv hs_env(const HsArgs &a, uint32_t e) {
  const w2a_state_view &v = a.st;
  HsEnv h;
  h.t0 = (uint32_t)v.t[e]; h.used = (uint32_t)v.used[e]; h.s0 = (uint32_t)v.streak[e];
  h.budget = v.budget[e]; h.ndays = (uint32_t)v.n_days[e];
  const uint32_t cw = (uint32_t)v.county_w[e], yi = (uint32_t)v.year_i[e], col = (uint32_t)v.coef_col[e];
  const uint32_t smp = (uint32_t)v.sample[e];
  // a start state no reset can produce would index outside the tables: NaN marks the env, nothing is read
  h.bad = cw >= (uint32_t)a.tb.S_w || yi >= (uint32_t)a.tb.Y || col >= (uint32_t)a.tb.S ||
          smp >= (uint32_t)a.tb.n_samples || h.ndays > (uint32_t)a.tb.T;
  h.ep_row = cw * (uint32_t)a.tb.Y + yi;
  h.wrow = col * (uint32_t)a.tb.n_samples + smp;
  const bool active = v.finished[e] == 0 && h.t0 < h.ndays;
  h.H = active ? min((uint32_t)a.n_steps, h.ndays - h.t0) : 0u;
  const int32_t rem = h.budget - (int32_t)h.used;
  h.U = rem <= 0 ? 0u : min((uint32_t)rem, h.H);
  return h;
}

// per env: horizon and U (envs without a DP are marked); histogram of U. Writes no output: the host checks the
// workspace against the histogram before anything the caller sees is written.
__global__ __launch_bounds__(256) void k_hs_plan(const HsArgs a) {
  __shared__ uint32_t cnt[HS_BINS];
  const uint32_t nb = (uint32_t)a.hb + 1u;
  for (uint32_t b = threadIdx.x; b < nb; b += 256) cnt[b] = 0;
  __syncthreads();
  const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (e < (uint64_t)a.n) {
    const HsEnv h = hs_env(a, (uint32_t)e);
    if (h.bad || h.H == 0) {
      a.u_env[e] = h.bad ? HS_BAD : HS_NONE;
    } else {
      a.u_env[e] = h.U;
      atomicAdd(&cnt[h.U], 1u);
    }
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nb; b += 256)
    if (cnt[b]) atomicAdd(&a.hist[b], cnt[b]);
}

// counting sort by U: a block reserves one range per bin, its envs take consecutive places in it; an env without a DP
// gets its outputs from fill(e, bad) (bad: a start outside the tables)
template <class Fill>
__device__ __forceinline__ void hs_scatter(const HsArgs &a, Fill fill) {
  __shared__ uint32_t cnt[HS_BINS];
  const uint32_t nb = (uint32_t)a.hb + 1u;
  for (uint32_t b = threadIdx.x; b < nb; b += 256) cnt[b] = 0;
  __syncthreads();
  const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  uint32_t U = e < (uint64_t)a.n ? a.u_env[e] : HS_NONE;
  if (U == HS_NONE || U == HS_BAD) {
    if (e < (uint64_t)a.n) fill(e, U == HS_BAD);
    U = HS_NONE;
  }
  const uint32_t rank = U != HS_NONE ? atomicAdd(&cnt[U], 1u) : 0u;
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nb; b += 256)
    if (cnt[b]) cnt[b] = atomicAdd(&a.cursor[b], cnt[b]);
  __syncthreads();
  if (U != HS_NONE) a.order[cnt[U] + rank] = (uint32_t)e;
}

// hs_scatter for w2a_hindsight_optimum and w2a_hindsight_posterior: 0 or NaN, an empty bitmap, no alerts
__global__ __launch_bounds__(256) void k_hs_scatter(const HsArgs a) {
  hs_scatter(a, [&](uint64_t e, bool bad) {
    a.ret[e] = bad ? __builtin_nanf("") : 0.0f;
    a.alerts[e] = 0;
    for (int w = 0; w < a.mask_words; ++w) a.mask[e * (uint32_t)a.mask_words + w] = 0u;
  });
}

struct HsCoef {  // the coefficients of the run-time part of both chains (slots 24, 25, 26, 28, 29), fp64
  double b24, b25, b26, b28, b29, e24, e25, e26, e28, e29;
};
// the reward the env pays on a day with static prefixes (pb, pe) and tail (x28, x29, gate), in state (j, streak),
// for action `act` (1 only where the budget allows it): the chain of the rollout kernels from slot 24 on
__device__ __forceinline__ float hs_reward(const HsCoef &c, double pb, double pe, float x28, float x29, bool gate,
                                           bool day0, float streak, int32_t rem, uint32_t act) {
  const double x24 = (double)((!day0) ? (float)act : 0.0f);
  const double x25 = (double)streak, x26 = (double)(float)rem, d28 = (double)x28, d29 = (double)x29;
  double zb = fma(x24, c.b24, pb);
  zb = fma(x25, c.b25, zb);
  zb = fma(x26, c.b26, zb);
  zb = fma(d28, c.b28, zb);
  zb = fma(d29, c.b29, zb);
  double ze = -__builtin_inf();  // with no alert the effectiveness does not enter the reward (eff * 0)
  if (act && gate) {
    ze = fma(x24, c.e24, pe);
    ze = fma(x25, c.e25, ze);
    ze = fma(x26, c.e26, ze);
    ze = fma(d28, c.e28, ze);
    ze = fma(d29, c.e29, ze);
  }
  return reward_from_logits(zb, ze, act);
}

__device__ __forceinline__ uint32_t hs_row(uint32_t idx) {  // j of state idx: j (j + 3) / 2 <= idx < (j + 1)(j + 4) / 2
  uint32_t j = (uint32_t)((__builtin_sqrtf(8.0f * (float)idx + 9.0f) - 3.0f) * 0.5f);
  while (j > 0 && j * (j + 3u) / 2u > idx) --j;
  while ((j + 1u) * (j + 4u) / 2u <= idx) ++j;
  return j;
}

// ---- the statements every kernel of the family shares (k_hs_dp, k_hs_along, k_hs_curve, k_hs_pm_dp): written once, so
// that "the same statements, the same bits" holds by construction

// the two fp64 prefixes (b, e) over slots 0..23 of one day (row xp) under one coefficient row pair (wq)
__device__ __forceinline__ double2 hs_prefix(const float4 *xp, const float4 *wq) {
  double zb = 0.0, ze = 0.0;
#pragma unroll
  for (int q = 0; q < RT_QUAD; ++q) {  // slots 0..23 in slot order
    const float4 x = xp[q], b = wq[q], f = wq[ROWF / 4 + q];
    zb = fma((double)x.x, (double)b.x, zb); ze = fma((double)x.x, (double)f.x, ze);
    zb = fma((double)x.y, (double)b.y, zb); ze = fma((double)x.y, (double)f.y, ze);
    zb = fma((double)x.z, (double)b.z, zb); ze = fma((double)x.z, (double)f.z, ze);
    zb = fma((double)x.w, (double)b.w, zb); ze = fma((double)x.w, (double)f.w, ze);
  }
  return make_double2(zb, ze);
}

// a day's tail from quad 7 of its row: x28, x29, the heat gate, -
__device__ __forceinline__ float4 hs_day_tail(const float4 x7) {
  return make_float4(x7.x, x7.y, x7.z > 0.5f ? 1.0f : 0.0f, 0.0f);
}

// day statics under the coefficient rows wq, lanes over days: pz[d] and tl[d] for d = lane .. H
__device__ __forceinline__ void hs_day_statics(const HsArgs &a, const HsEnv &h, const float4 *wq, uint32_t lane,
                                               double2 *pz, float4 *tl) {
  const uint32_t rows_per_day = (uint32_t)(a.tb.S_w * a.tb.Y);
  for (uint32_t d = lane; d < h.H; d += HS_BLOCK) {
    const float4 *xp = a.tb.X + (size_t)((h.t0 + d) * rows_per_day + h.ep_row) * (ROWF / 4);
    const double2 p = hs_prefix(xp, wq);
    const float4 x7 = xp[GATE_QUAD];
    pz[d] = p;
    tl[d] = hs_day_tail(x7);
  }
}

__device__ __forceinline__ HsCoef hs_load_coef(const float4 *wq) {
  const float4 b6 = wq[RT_QUAD], b7 = wq[GATE_QUAD], f6 = wq[ROWF / 4 + RT_QUAD], f7 = wq[ROWF / 4 + GATE_QUAD];
  HsCoef c;
  c.b24 = b6.x; c.b25 = b6.y; c.b26 = b6.z; c.b28 = b7.x; c.b29 = b7.y;
  c.e24 = f6.x; c.e25 = f6.y; c.e26 = f6.z; c.e28 = f7.x; c.e29 = f7.y;
  return c;
}

// env e's bitmap row: lane l holds word l (every lane walked the same path); words past the 64th are empty
__device__ __forceinline__ void hs_store_mask_row(const HsArgs &a, uint32_t e, uint32_t lane, uint32_t word) {
  for (uint32_t w = lane; w < (uint32_t)a.mask_words; w += HS_BLOCK)
    a.mask[(size_t)e * (uint32_t)a.mask_words + w] = w < HS_BLOCK && w == lane ? word : 0u;
}

// state idx = (j, k) of the (alerts, streak) DP on a day with prefixes p and tail tq, V_{d+1} in vn: both Q values, the
// strict comparison and V_d. k_hs_dp keeps `best` and `alert`; k_hs_along also q0, q1 and `allowed` in the path's state.
struct HsState {
  bool allowed, alert;  // the alert transition exists (budget left, day open); the DP takes it
  double q0, q1, best;  // q1 = q0 where no alert is allowed
};
__device__ __forceinline__ HsState hs_state(const HsCoef &c, const HsEnv &h, int32_t rem0, bool open, double2 p, float4 tq,
                                            bool gate, bool day0, const double *vn, uint32_t idx) {
  const uint32_t j = hs_row(idx), k = idx - j * (j + 3u) / 2u;
  const float s = (float)(k == j + 1u ? h.s0 + j : k);
  const int32_t rem = h.budget - (int32_t)(h.used + j);
  HsState r;
  r.allowed = (int32_t)j < rem0 && open;
  const float r0 = hs_reward(c, p.x, p.y, tq.x, tq.y, gate, day0, s, rem, 0u);
  r.q0 = (double)r0 + vn[j * (j + 3u) / 2u];
  r.best = r.q0; r.q1 = r.q0;
  r.alert = false;
  if (r.allowed) {
    const float r1 = hs_reward(c, p.x, p.y, tq.x, tq.y, gate, day0, s, rem - 1, 1u);
    r.q1 = (double)r1 + vn[(j + 1u) * (j + 4u) / 2u + k + 1u];
    r.alert = r.q1 > r.q0;
    r.best = r.alert ? r.q1 : r.q0;
  }
  return r;
}

// one env per 64-lane workgroup; envs list[0 .. gridDim.x) all have this U. GLOBAL: V and the decision words live in
// `pool` (pool_stride bytes per workgroup) instead of LDS.
// GATE: the alert transition exists only on the days a.gate allows (the best schedule UNDER the restriction); the word
// of a day is wave-uniform and loaded once per 32 days. GATE = false compiles from the statements it had before.
template <bool GLOBAL, bool GATE>
__global__ __launch_bounds__(HS_BLOCK) void k_hs_dp(const HsArgs a, const uint32_t *list, uint32_t U, char *pool,
                                                    size_t pool_stride) {
  extern __shared__ __attribute__((aligned(16))) char hs_lds[];
  const uint32_t lane = threadIdx.x;
  const uint32_t e = list[blockIdx.x];
  const HsEnv h = hs_env(a, e);
  const uint32_t H = h.H, hb = (uint32_t)a.hb;
  const uint32_t NCU = hs_nc(U);
  double2 *pz = reinterpret_cast<double2 *>(hs_lds);               // [hb] prefixes over slots 0..23 (b, e)
  float4 *tl = reinterpret_cast<float4 *>(hs_lds + 16 * (size_t)hb);  // [hb] x28, x29, gate, -
  char *dp = GLOBAL ? pool + (size_t)blockIdx.x * pool_stride : hs_lds + hs_day_bytes(hb);
  double *V0 = reinterpret_cast<double *>(dp);
  double *V1 = V0 + hs_ns(U);
  uint64_t *dec = reinterpret_cast<uint64_t *>(V1 + hs_ns(U));     // [hb][NCU]

  // the env's own coefficient rows (wave-uniform), f32 as stored
  const float4 *wq = a.tb.W + (size_t)h.wrow * (2 * ROWF / 4);
  hs_day_statics(a, h, wq, lane, pz, tl);
  const HsCoef c = hs_load_coef(wq);
  const int32_t rem0 = h.budget - (int32_t)h.used;  // remaining budget at the start; an alert needs j < rem0
  for (uint32_t i = lane; i < hs_ns(U); i += HS_BLOCK) V1[i] = 0.0;  // V_H = 0
  __syncthreads();

  // ---- backward DP: V_{d+1} in vn, V_d into vc
  double *vn = V1, *vc = V0;
  uint32_t gate_word = 0, gate_idx = 0xFFFFFFFFu;
  for (int32_t d = (int32_t)H - 1; d >= 0; --d) {
    const bool open = !GATE || gate_allows(a.gate, a.gate_words, e, h.t0 + (uint32_t)d, gate_word, gate_idx);
    const uint32_t J = min((uint32_t)d, U);
    const uint32_t nsd = hs_ns(J);
    const double2 p = pz[d];
    const float4 tq = tl[d];
    const bool day0 = (h.t0 + (uint32_t)d) == 0u, gate = tq.z != 0.0f;
    for (uint32_t c0 = 0; c0 < nsd; c0 += HS_BLOCK) {
      const uint32_t idx = c0 + lane;
      bool alert = false;
      if (idx < nsd) {
        const HsState st = hs_state(c, h, rem0, open, p, tq, gate, day0, vn, idx);
        alert = st.alert;
        vc[idx] = st.best;
      }
      const uint64_t bits = __ballot(alert);
      if (lane == 0) dec[(size_t)d * NCU + c0 / HS_BLOCK] = bits;
    }
    __syncthreads();
    double *tmp = vn; vn = vc; vc = tmp;
  }

  // ---- backtrack from (0, s0), re-adding the chosen rewards in f32 in day order (every lane the same path)
  uint32_t j = 0, k = h.s0 > 0 ? 1u : 0u, n_alerts = 0, word = 0;
  float ret = 0.0f;
  for (uint32_t d = 0; d < H; ++d) {
    const uint32_t idx = j * (j + 3u) / 2u + k;
    const uint32_t act = (uint32_t)(dec[(size_t)d * NCU + (idx >> 6)] >> (idx & 63u)) & 1u;
    const double2 p = pz[d];
    const float4 tq = tl[d];
    const uint32_t tt = h.t0 + d;
    const float s = (float)(k == j + 1u ? h.s0 + j : k);
    float r = hs_reward(c, p.x, p.y, tq.x, tq.y, tq.z != 0.0f, tt == 0u, s,
                        h.budget - (int32_t)(h.used + j + act), act);
    asm volatile("" : "+v"(r));  // the reward is rounded to f32 before it is added, as in the rollout kernels (no fma)
    ret += r;
    if (act && lane == (tt >> 5)) word |= 1u << (tt & 31u);
    n_alerts += act;
    j += act;
    k = act ? k + 1u : 0u;
  }
  hs_store_mask_row(a, e, lane, word);
  if (lane == 0) {
    a.ret[e] = ret;
    a.alerts[e] = (int32_t)n_alerts;
  }
}

// ----------------------------------------------------------------------------------------
// hindsight values along a GIVEN schedule (w2a_hindsight_along)
// ----------------------------------------------------------------------------------------
// The backward sweep above forms Q_d(state, no alert) and Q_d(state, alert) of every reachable state and keeps only
// what the optimum's own path needs. k_hs_along runs the same sweep (hs_state: the same rewards, the same fp64 values,
// the same strict comparison) and keeps, per day, the values of the ONE state a caller's schedule reaches: the labels
// DAgger fits to and the per-day share of the regret.
//   Forward first: every lane walks the schedule (attempts; closed days and attempts without budget are no-ops) and
//   lane 0 leaves the day's state index and the alert issued in the fourth float of tl[d] (bit 31 the alert, bits
//   0..29 the index), so LDS and workspace are those of k_hs_dp (the decision words' room is simply not used).
//   In the sweep the lane whose idx is the path's holds q0, q1 and best: it writes the day's outputs, sets bit 30 of
//   the word (the DP's decision in that state) and puts the fp64 loss where the day's prefix pz[d].x was (day d's
//   statics are not read again). Afterwards every lane assembles the expert bitmap as the backtrack assembles its own,
//   and lane 0 adds the losses in fp64 in day order. No atomics: identical calls give identical bits.
struct HsAlongArgs {
  HsArgs h;               // ret = regret_out, mask = expert_mask, alerts unused (NULL); gate NULL: GATE = false
  const uint32_t *sched;  // [n][mask_words] the schedule: attempts by day of the episode
  float *gain;            // [hb][n] by call-day and env id
  float *value;           // [hb][n], nullable
  float *loss;            // [hb][n], nullable
};

// hs_scatter for w2a_hindsight_along: envs without a DP get 0 (NaN: a start outside the tables) in every float output,
// NaN in every gain and an empty bitmap
__global__ __launch_bounds__(256) void k_hs_along_scatter(const HsAlongArgs aa) {
  const HsArgs &a = aa.h;
  hs_scatter(a, [&](uint64_t e, bool bad) {
    const float nan = __builtin_nanf(""), fill = bad ? nan : 0.0f;
    a.ret[e] = fill;
    for (int w = 0; w < a.mask_words; ++w) a.mask[e * (uint32_t)a.mask_words + w] = 0u;
    for (uint32_t s = 0; s < (uint32_t)a.hb; ++s) {
      const size_t o = (size_t)s * (size_t)a.n + e;
      aa.gain[o] = nan;
      if (aa.value) aa.value[o] = fill;
      if (aa.loss) aa.loss[o] = fill;
    }
  });
}

#define HS_PATH_ALERT 0x80000000u   // the alert the schedule issues that day
#define HS_PATH_EXPERT 0x40000000u  // the DP's decision in the state the schedule reaches
#define HS_PATH_IDX 0x3FFFFFFFu

// one env per 64-lane workgroup, as k_hs_dp (GLOBAL, GATE, list, U, pool as there)
template <bool GLOBAL, bool GATE>
__global__ __launch_bounds__(HS_BLOCK) void k_hs_along(const HsAlongArgs aa, const uint32_t *list, uint32_t U, char *pool,
                                                       size_t pool_stride) {
  extern __shared__ __attribute__((aligned(16))) char hs_lds[];
  const HsArgs &a = aa.h;
  const uint32_t lane = threadIdx.x;
  const uint32_t e = list[blockIdx.x];
  const HsEnv h = hs_env(a, e);
  const uint32_t H = h.H, hb = (uint32_t)a.hb;
  double2 *pz = reinterpret_cast<double2 *>(hs_lds);               // [hb] prefixes over slots 0..23 (b, e); .x: the loss
  float4 *tl = reinterpret_cast<float4 *>(hs_lds + 16 * (size_t)hb);  // [hb] x28, x29, gate, the path's word
  char *dp = GLOBAL ? pool + (size_t)blockIdx.x * pool_stride : hs_lds + hs_day_bytes(hb);
  double *V0 = reinterpret_cast<double *>(dp);
  double *V1 = V0 + hs_ns(U);

  // the env's own coefficient rows (wave-uniform), f32 as stored
  const float4 *wq = a.tb.W + (size_t)h.wrow * (2 * ROWF / 4);
  hs_day_statics(a, h, wq, lane, pz, tl);
  const HsCoef c = hs_load_coef(wq);
  const int32_t rem0 = h.budget - (int32_t)h.used;  // remaining budget at the start; an alert needs j < rem0
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
      if (lane == 0) reinterpret_cast<uint32_t *>(tl + d)[3] = (j * (j + 3u) / 2u + k) | (act ? HS_PATH_ALERT : 0u);
      j += act;
      k = act ? k + 1u : 0u;
    }
  }
  __syncthreads();

  // ---- backward DP (k_hs_dp's: hs_state): V_{d+1} in vn, V_d into vc
  double *vn = V1, *vc = V0;
  uint32_t gate_word = 0, gate_idx = 0xFFFFFFFFu;
  const size_t n = (size_t)a.n;
  for (int32_t d = (int32_t)H - 1; d >= 0; --d) {
    const bool open = !GATE || gate_allows(a.gate, a.gate_words, e, h.t0 + (uint32_t)d, gate_word, gate_idx);
    const uint32_t J = min((uint32_t)d, U);
    const uint32_t nsd = hs_ns(J);
    const double2 p = pz[d];
    const float4 tq = tl[d];
    const uint32_t path = __float_as_uint(tq.w);
    const bool day0 = (h.t0 + (uint32_t)d) == 0u, gate = tq.z != 0.0f;
    bool mine = false, mine_alert = false;  // this lane holds the path's state of day d
    double mine_loss = 0.0;
    for (uint32_t c0 = 0; c0 < nsd; c0 += HS_BLOCK) {
      const uint32_t idx = c0 + lane;
      if (idx < nsd) {
        const HsState st = hs_state(c, h, rem0, open, p, tq, gate, day0, vn, idx);
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
    if (mine) {  // day d's statics have been read by every lane: their room takes the day's results
      pz[d].x = mine_loss;
      reinterpret_cast<uint32_t *>(tl + d)[3] = path | (mine_alert ? HS_PATH_EXPERT : 0u);
    }
    __syncthreads();
    double *tmp = vn; vn = vc; vc = tmp;
  }

  // ---- the expert's bits along the path (every lane the same days), the regret in fp64 in day order
  uint32_t word = 0;
  for (uint32_t d = 0; d < H; ++d) {
    const uint32_t tt = h.t0 + d;
    const uint32_t path = reinterpret_cast<const uint32_t *>(tl + d)[3];
    if ((path & HS_PATH_EXPERT) && lane == (tt >> 5)) word |= 1u << (tt & 31u);
  }
  hs_store_mask_row(a, e, lane, word);
  if (lane == 0) {
    double regret = 0.0;
    for (uint32_t d = 0; d < H; ++d) regret += pz[d].x;
    a.ret[e] = (float)regret;
  }
  for (uint32_t s = H + lane; s < hb; s += HS_BLOCK) {  // call-days the env does not step
    const size_t o = (size_t)s * n + e;
    aa.gain[o] = __builtin_nanf("");
    if (aa.value) aa.value[o] = 0.0f;
    if (aa.loss) aa.loss[o] = 0.0f;
  }
}

// some coefficient row has a nonzero slot-27 term (the agent's 14-day count): the DP state would not be exact
__global__ void k_hs_scan_slot27(const float4 *W, int64_t rows, int32_t *flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  if (W[i * (ROWF / 4) + RT_QUAD].w != 0.0f) atomicOr(flag, 1);
}

#endif  // W2A_HINDSIGHT_HIP_H
