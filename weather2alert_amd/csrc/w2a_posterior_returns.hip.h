// w2a_posterior_returns.hip.h -- k_posterior_returns: an env's return under every posterior draw of its coefficient column
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_POSTERIOR_RETURNS_HIP_H
#define W2A_POSTERIOR_RETURNS_HIP_H

// ----------------------------------------------------------------------------------------
// returns under every posterior draw (w2a_posterior_returns)
// ----------------------------------------------------------------------------------------
// The trajectory does not depend on the draw: the state update (env.py:238-262) reads only the actions and the alert
// buffers, and the draw enters only the reward (env.py:197-226, coef_index at :209,216). So the start-of-call state and
// the bitmap of the alerts actually issued fix every day's 32-slot input vector, and the return under draw k of the
// env's column c is the f32 day-ordered sum of reward(x_t, a_t; W[c * n_samples + k]).
//   Mapping: one lane per (env, draw) pair, p = e * n_samples + k, dense over the batch (no padding of n_samples to the
//   wave: at n_samples = 100 a wave serves parts of two envs). A lane's work is a VALU instruction stream whatever its
//   operands' uniformity, so the dense form issues n * n_samples / 64 waves where one-env-per-wave would issue
//   n * ceil(n_samples / 64). Lanes of one env read the same feature-row lines (broadcast in the vector L1) and
//   consecutive coefficient rows; the output store is lane-consecutive.
//   Numerics: each day rebuilds xv[] exactly as k_rollout_linear / k_rollout64 do (table row, faithful run-time quad)
//   and runs the same two fp64 FMA chains over slots 0..29, the same heat gate and reward_from_logits, then adds the
//   reward to an f32 sum in day order -- for the env's own draw the very operations of those kernels' `return`.
struct PostRetArgs {
  DevTables tb;
  w2a_state_view st;         // start-of-call state (device i32 arrays, w2a_get_state's decoding)
  const uint32_t *alert_mask;  // [n][mask_words] bit d: alert issued on day d
  int32_t mask_words;
  int32_t n_steps;
  int64_t n;
  float *out;                // [n][n_samples]
};

__global__ __launch_bounds__(256) void k_posterior_returns(const PostRetArgs a) {
  const uint32_t ns = (uint32_t)a.tb.n_samples;
  const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (p >= (uint64_t)a.n * ns) return;
  const uint32_t e = (uint32_t)(p / ns);
  const uint32_t k = (uint32_t)(p - (uint64_t)e * ns);
  const w2a_state_view &v = a.st;
  uint32_t t = (uint32_t)v.t[e], used = (uint32_t)v.used[e], streak = (uint32_t)v.streak[e];
  uint32_t hist = (uint32_t)v.hist14[e] & 0x3FFFu;
  const int32_t budget = v.budget[e];
  const uint32_t ndays = (uint32_t)v.n_days[e];
  const uint32_t cw = (uint32_t)v.county_w[e], yi = (uint32_t)v.year_i[e], col = (uint32_t)v.coef_col[e];
  // a start state no reset can produce would index outside the tables: NaN marks the row, nothing is read
  if (cw >= (uint32_t)a.tb.S_w || yi >= (uint32_t)a.tb.Y || col >= (uint32_t)a.tb.S || ndays > (uint32_t)a.tb.T) {
    a.out[p] = __builtin_nanf("");
    return;
  }
  const uint32_t ep_row = cw * (uint32_t)a.tb.Y + yi;
  const uint32_t rows_per_day = (uint32_t)(a.tb.S_w * a.tb.Y);
  const uint32_t *mask = a.alert_mask + (size_t)e * (uint32_t)a.mask_words;
  // this lane's two coefficient rows, once, widened to fp64 (exact): the day loop is 60 FMAs with no converts of W
  double wb[RO64_SLOTS], we[RO64_SLOTS];
  {
    const float4 *wq = a.tb.W + ((size_t)col * ns + k) * (2 * ROWF / 4);
    float fb[32], fe[32];
#pragma unroll
    for (int q = 0; q < ROWF / 4; ++q) {
      const float4 b = wq[q], f = wq[ROWF / 4 + q];
      fb[4 * q] = b.x; fb[4 * q + 1] = b.y; fb[4 * q + 2] = b.z; fb[4 * q + 3] = b.w;
      fe[4 * q] = f.x; fe[4 * q + 1] = f.y; fe[4 * q + 2] = f.z; fe[4 * q + 3] = f.w;
    }
#pragma unroll
    for (int s = 0; s < RO64_SLOTS; ++s) { wb[s] = (double)fb[s]; we[s] = (double)fe[s]; }
  }
  float ret = 0.0f;
  bool active = v.finished[e] == 0 && t < ndays;
  for (int s = 0; s < a.n_steps && active; ++s) {
    // ---- env.py:242-250 with the action the rollout actually issued
    const uint32_t actual = (mask[t >> 5] >> (t & 31)) & 1u;
    const uint32_t used2 = used + actual;
    const uint32_t hist2 = ((hist << 1) | actual) & 0x3FFFu;
    const uint32_t day_row = t * rows_per_day + ep_row;
    float xv[32];
    {
      const float4 *xp = a.tb.X + (size_t)day_row * (ROWF / 4);
#pragma unroll
      for (int q = 0; q < ROWF / 4; ++q) {
        if (q == RT_QUAD) continue;  // slots 24..27 are run-time fields
        const float4 x = xp[q];
        xv[4 * q] = x.x; xv[4 * q + 1] = x.y; xv[4 * q + 2] = x.z; xv[4 * q + 3] = x.w;
      }
    }
    // the run-time fields of the faithful observation (env.py:190-193): lag = today's alert, the pre-update streak
    xv[4 * RT_QUAD] = (t > 0) ? (float)actual : 0.0f;
    xv[4 * RT_QUAD + 1] = (float)streak;
    xv[4 * RT_QUAD + 2] = (float)(budget - (int32_t)used2);
    xv[4 * RT_QUAD + 3] = (float)__popc(hist2);
    double zb = 0.0, ze = 0.0;
#pragma unroll
    for (int q = 0; q < RO64_SLOTS; ++q) {
      const double xk = (double)xv[q];
      zb = fma(xk, wb[q], zb);
      ze = fma(xk, we[q], ze);
    }
    if (!(xv[30] > 0.5f)) ze = -__builtin_inf();
    float r = reward_from_logits(zb, ze, actual);
    asm volatile("" : "+v"(r));  // the reward is rounded to f32 before it is added, as in the rollout kernels (no fma)
    ret += r;
    used = used2; hist = hist2;
    if (t + 1 >= ndays) active = false;  // the terminal day
    else { streak = actual ? streak + 1 : 0; t = t + 1; }
  }
  a.out[p] = ret;
}

#endif  // W2A_POSTERIOR_RETURNS_HIP_H
