// w2a_lookahead.hip.h -- the lookahead inputs of a learned policy: the coming days' weather, seen from the held row
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_LOOKAHEAD_HIP_H
#define W2A_LOOKAHEAD_HIP_H

// ----------------------------------------------------------------------------------------
// policy["lookahead"] = {"feature": .., "days": D}  (the older reference env's incorp_forecasts, zero forecast error)
// ----------------------------------------------------------------------------------------
// The row an agent holds is the table row of day r = max(t - 1, 0) (the lagging observation, Q6). A lookahead policy
// gets D more inputs next to it,
//     f_k = h(r + k) - h(r),  k = 1..D,      f_k = 0 where r + k >= n_days of the env,
// h(d) the f32 table value of one table-sourced feature on day d of the env's episode. The difference is one f32
// subtraction. h comes from the series table (HeatAlertVecEnv.lookahead_table: f32 [S_w * Y][stride >= T], one episode's
// days contiguous), so a day costs D + 1 consecutive floats of one series, not D + 1 strided feature rows.
//   Past the end: the load is redirected to h(r) itself, and h(r) - h(r) is +0 for every finite h.
//   Bounds: every index is below lim = min(n_days, stride), and r is clamped below lim too (r <= t < n_days for every
//   state the library writes), so nothing is read outside the env's own series.
#define W2A_LOOK_MAX W2A_LOOKAHEAD_MAX_DAYS  // D <= 10 (the older reference env's "D10")
#define W2A_LOOK_PAD W2A_LOOKAHEAD_PAD       // floats per weight row / per MLP input row: whole k-steps of 4

struct LookArgs {
  const float *series;  // [S_w * Y][stride]
  int32_t stride;       // floats per series, >= T
  int32_t days;         // D in 1..W2A_LOOK_MAX (wave-uniform: the loops below branch on it with scalar compares)
  const float *weight;  // linear kind: [n_groups][W2A_LOOK_PAD], k = 1 first (the MLP kind keeps its rows in the block)
};

// the series of feature row `row` (cold.x = county_w * Y + year_i)
__device__ __forceinline__ const float *look_series(const LookArgs &lk, uint32_t row) {
  return lk.series + (size_t)row * (size_t)lk.stride;
}

// f[k - 1] = f_k for k <= D; entries past D are 0
__device__ __forceinline__ void look_inputs(const LookArgs &lk, const float *series, uint32_t r, uint32_t ndays,
                                            float (&f)[W2A_LOOK_MAX]) {
  const uint32_t lim = ndays < (uint32_t)lk.stride ? ndays : (uint32_t)lk.stride;
  r = r < lim ? r : lim - 1u;
  const float h0 = series[r];
#pragma unroll
  for (int k = 0; k < W2A_LOOK_MAX; ++k) {
    f[k] = 0.0f;
    if (k < lk.days) {
      const uint32_t d = r + 1u + (uint32_t)k;
      f[k] = series[d < lim ? d : r] - h0;
    }
  }
}

// the fp64 logit chain continued over the lookahead inputs, in order of k
__device__ __forceinline__ double look_logit(const LookArgs &lk, const float (&f)[W2A_LOOK_MAX],
                                             const float (&lw)[W2A_LOOK_MAX], double z) {
#pragma unroll
  for (int k = 0; k < W2A_LOOK_MAX; ++k)
    if (k < lk.days) z = fma((double)f[k], (double)lw[k], z);
  return z;
}

// the group's lookahead weights (linear kind)
__device__ __forceinline__ void look_weights(const LookArgs &lk, int32_t g, float (&lw)[W2A_LOOK_MAX]) {
#pragma unroll
  for (int k = 0; k < W2A_LOOK_MAX; ++k) lw[k] = k < lk.days ? lk.weight[(size_t)g * W2A_LOOK_PAD + k] : 0.0f;
}

#endif  // W2A_LOOKAHEAD_HIP_H
