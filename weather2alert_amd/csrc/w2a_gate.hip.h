// w2a_gate.hip.h -- k_alert_gate: the days on which a table-sourced observation column reaches a threshold, per env
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_GATE_HIP_H
#define W2A_GATE_HIP_H

// ----------------------------------------------------------------------------------------
// alert gate (w2a_alert_gate)
// ----------------------------------------------------------------------------------------
// The older reference env restricts alerts to hot days: an alert attempted while observation[heat_qi] < HI_restriction
// becomes "no alert" before the attempt is recorded and before the budget test (_deprecated/env.py, step()). The column
// is table-sourced, so whether day t is allowed depends on (county, year, t) only, never on what the agent did: a
// bitmap over the days of the episode, in the layout of alert_mask (bit t & 31 of word t >> 5). This kernel builds it;
// the *_gated entry points read it (k_rollout_linear<.., GATE> and its kin).
//   Row: the agent chooses day t's action on the row step() returned for day t - 1 -- under the faithful semantics the
//   table row of day max(t - 1, 0) (the lagging observation, Q6: days 0 and 1 both see row 0), with W2A_FIX_OBS the row of
//   day t itself. The row is read from the tables with the env's (county, year), as the rollout kernels read it; the
//   observation buffer is not read.
//   Days: from the env's current day over the days it would still step (n_steps of them, or to its terminal day). Days
//   before, days after and finished envs are 0. One lane per env; every word of the env's row of `out` is written once,
//   with a plain store, by that lane: no atomics, and nothing else is written.
//   Access pattern: a call per batch of episodes, not a hot path, and written for clarity. Lane e stores its `words`
//   words at a stride of 4 * words bytes from lane e + 1 (uncoalesced: 64 lanes touch 64 separate 20-B runs at T = 153),
//   and reads one f32 per day at a stride of rows_per_day * 128 B along the days, the same row-per-day walk the rollout
//   kernels make (neighbouring lanes share lines only where neighbouring envs share a (county, year)).
struct GateArgs {
  DevTables tb;
  StateArrays st;
  int64_t n;
  int32_t slot;            // feature-row slot of the column (host: an observation column outside slots 24..27)
  int32_t lag;             // 1: row of day max(t - 1, 0) (faithful); 0: row of day t (W2A_FIX_OBS)
  int32_t n_steps;
  int32_t words;           // words per env of `out` (host: words * 32 >= T)
  float threshold;         // used when thresholds is NULL
  const float *thresholds; // [n] per-env threshold (nullable)
  uint32_t *out;           // [n][words]
};

__global__ __launch_bounds__(BLOCK) void k_alert_gate(const GateArgs a) {
  const int64_t e64 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e64 >= a.n) return;
  const uint32_t e = (uint32_t)e64;
  uint4 c2, hot;
  load_step_state(a.st, e, c2, hot);
  const uint4 cold = load_cold(a.st, e);
  const uint32_t t0 = D0_T(hot.x), ndays = min(D1_NDAYS(hot.y), (uint32_t)a.tb.T);
  const bool fin = D1_FIN(hot.y) != 0;
  const uint32_t rows_per_day = (uint32_t)(a.tb.S_w * a.tb.Y);
  // a (county, year) row outside the tables (no reset produces one) reads nothing: the env gets an empty bitmap
  const bool ok = !fin && cold.x < rows_per_day && t0 < ndays;
  const uint32_t t1 = ok ? (uint32_t)min((uint64_t)t0 + (uint64_t)a.n_steps, (uint64_t)ndays) : 0u;  // one past the last day
  const float tau = a.thresholds ? a.thresholds[e] : a.threshold;
  const float *Xf = reinterpret_cast<const float *>(a.tb.X);
  uint32_t *row = a.out + (size_t)e * a.words;
  for (uint32_t w = 0; w < (uint32_t)a.words; ++w) {
    uint32_t word = 0;
    const uint32_t lo = max(32u * w, ok ? t0 : 0xFFFFFFFFu), hi = min(32u * w + 32u, t1);
    for (uint32_t t = lo; t < hi; ++t) {
      const uint32_t src = (a.lag && t > 0) ? t - 1 : t;  // src <= t < ndays <= T
      const float v = Xf[((size_t)src * rows_per_day + cold.x) * ROWF + a.slot];
      word |= (v >= tau ? 1u : 0u) << (t & 31);
    }
    row[w] = word;
  }
}

#endif  // W2A_GATE_HIP_H
