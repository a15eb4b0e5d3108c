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
  // forecast error (policy["lookahead"]["error"], the w2a_forecast_* entry points): read by the NOISE = true
  // instantiations only; zero otherwise. Kernel arguments, so the row is wave-uniform (scalar loads, no table)
  uint64_t err_seed;        // error_seed
  float mae[W2A_LOOK_PAD];  // e_k at [k - 1], zero past D
};

// the series of feature row `row` (cold.x = county_w * Y + year_i)
__device__ __forceinline__ const float *look_series(const LookArgs &lk, uint32_t row) {
  return lk.series + (size_t)row * (size_t)lk.stride;
}

// ----------------------------------------------------------------------------------------
// forecast error: {"error": e_1..e_D, "error_seed": s}  (the older reference env's forecast_error > 0 branch)
// ----------------------------------------------------------------------------------------
//     f_k = fmaf(U(r, k), e_k, h(r + k)) - h(r)     one f32 fma, one f32 subtraction; h(r) itself is exact
//     f_k = +0 where r + k >= n_days (no noise), and h(r + k) is taken as it is where e_k == 0 (the fma would turn a
//     -0 into +0), so a zero row gives the bits of the form without noise for every finite h
// U(r, k) = (float)(word >> 8) * 2^-23 - 1 in [-1, 1 - 2^-23], word 32 bits of
//     x = w2a_mix64(stream + (8 * r + ((k - 1) >> 1) + 1) * 0x9E3779B97F4A7C15),
// the high half for odd k, the low half for even k (one hash serves two leads), with
//     stream = rng_stream(error_seed ^ W2A_LOOK_NOISE_C, global env id, episode number):
// a function of (error_seed, global env id, episode, held day, lead) and of nothing else. W2A_LOOK_NOISE_C differs from
// the constant of the Bernoulli policies' stream, so equal seeds still give independent draws. (include/w2a.h)
#define W2A_LOOK_NOISE_C 0xC3C3C3C33C3C3C3Cull

// the env's error stream: once per env, outside the day loop
__device__ __forceinline__ uint64_t look_noise_stream(const LookArgs &lk, uint64_t gid, uint32_t episode) {
  return rng_stream(lk.err_seed ^ W2A_LOOK_NOISE_C, gid, episode);
}

// the series pointer at a use inside the day loop. NOISE: formed again from the feature row, from one register that
// is live anyway, so the pointer is not held across the loop -- the stream takes its two registers
template <bool NOISE>
__device__ __forceinline__ const float *look_series_of(const LookArgs &lk, const float *held, uint32_t row) {
  if constexpr (NOISE) {
    asm volatile("" : "+v"(row));
    return look_series(lk, row);
  } else {
    return held;
  }
}

// f[k - 1] = f_k for k <= D; entries past D are 0. NOISE: with the forecast error of the env's stream `estream`
template <bool NOISE = false>
__device__ __forceinline__ void look_inputs(const LookArgs &lk, const float *series, uint32_t r, uint32_t ndays,
                                            float (&f)[W2A_LOOK_MAX], uint64_t estream = 0) {
  const uint32_t lim = ndays < (uint32_t)lk.stride ? ndays : (uint32_t)lk.stride;
  r = r < lim ? r : lim - 1u;
  const float h0 = series[r];
  uint64_t x = 0;
#pragma unroll
  for (int k = 0; k < W2A_LOOK_MAX; ++k) {
    f[k] = 0.0f;
    if (k < lk.days) {
      const uint32_t d = r + 1u + (uint32_t)k;
      if constexpr (NOISE) {
        if ((k & 1) == 0) x = w2a_mix64(estream + (uint64_t)(8u * r + (uint32_t)(k >> 1) + 1u) * 0x9E3779B97F4A7C15ull);
        const uint32_t word = (k & 1) ? (uint32_t)x : (uint32_t)(x >> 32);
        const float u = (float)(word >> 8) * 1.1920928955078125e-07f - 1.0f;
        const float e = lk.mae[k];  // wave-uniform
        const float h = series[d < lim ? d : r];
        const float hk = e != 0.0f ? fmaf(u, e, h) : h;
        f[k] = d < lim ? hk - h0 : 0.0f;
      } else {
        f[k] = series[d < lim ? d : r] - h0;
      }
    }
  }
}

// w2a_forecast_features: the noisy inputs of the rows the envs hold now, f32 [n][D], through look_inputs<true> itself
// (what HeatAlertVecEnv.lookahead_features() returns for a spec with "error"; one lane per env, nothing is written
// past out[n * D])
struct LookFeaturesArgs {
  StateArrays st;
  int64_t n;
  int64_t gid0;
  LookArgs look;
  float *out;
};

__global__ __launch_bounds__(BLOCK) void k_lookahead_features(const LookFeaturesArgs fa) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= fa.n) return;
  const uint32_t e = (uint32_t)i;
  uint4 c2, hot;
  load_step_state(fa.st, e, c2, hot);
  const uint4 cold = load_cold(fa.st, e);
  const uint32_t t = D0_T(hot.x), ndays = D1_NDAYS(hot.y);
  const uint64_t estream = look_noise_stream(fa.look, (uint64_t)(fa.gid0 + e), cold.w);
  float lf[W2A_LOOK_MAX];
  look_inputs<true>(fa.look, look_series(fa.look, cold.x), t > 0 ? t - 1 : 0u, ndays, lf, estream);
  float *row = fa.out + (size_t)e * (size_t)fa.look.days;
#pragma unroll
  for (int k = 0; k < W2A_LOOK_MAX; ++k)
    if (k < fa.look.days) row[k] = lf[k];
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
