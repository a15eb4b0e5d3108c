// w2a_rollout_mlp.hip.h -- k_rollout_mlp: on-device rollout of a small MLP policy with one parameter block per group
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_ROLLOUT_MLP_HIP_H
#define W2A_ROLLOUT_MLP_HIP_H

// ----------------------------------------------------------------------------------------
// MLP policy inside k_rollout_linear's day loop (w2a_rollout_mlp)
// ----------------------------------------------------------------------------------------
// The day loop, the faithful observation, the first day read from the observation row, the single write-back of the
// final row, the masks and the snapshots are k_rollout_linear's (w2a_rollout_linear.hip.h). Its third fp64 chain is
// replaced by a 1- or 2-hidden-layer f32 network on the 32-slot vector xv[], computed on the matrix cores with
// v_mfma_f32_16x16x4_f32 (exact f32: bit for bit a k-ordered fmaf chain).
//   Orientation: H^T = W^T . X^T, hidden units on M (16 per tile), the 16 envs of a block on N (lane & 15).
//   Input: the wave's 64 xv[] rows go through LDS (xs: [64 envs][36 floats], conflict-free for the B-operand reads)
//     into the B operand of the first layer: lane l of k-step ks holds slot 4ks + (l >> 4) of env 16 blk + (l & 15).
//   Layer to layer: register i of hidden tile t holds unit 16t + 4(l >> 4) + i of env l & 15 -- exactly a B operand
//     whose k index l >> 4 is that unit, so it feeds the next layer with no lane movement; the A operand is permuted
//     to match on load: lane l of k-step (t, i) gets W2[16t + 4(l >> 4) + i][16o + (l & 15)].
//   Output: each lane's fmaf chain over its 4 * (width / 16) units with w_out (b_out first, on lanes 0..15), then
//     a sum over lanes l, l ^ 16, l ^ 32, l ^ 48; lane e takes the value of block e >> 4.
//   Blocks: 4 / (width / 16) blocks of 16 envs go through the network together, so every layer has 4 independent
//     accumulator tiles in flight (the f32 MFMA's dependent latency is 40 cycles against a 32-cycle issue).
//   Groups: a wave visits the distinct group ids of its lanes one after the other (wave-uniform loop, usually one
//     pass with the group-major visiting order policy.py passes); every lane keeps the logit of its own group. An
//     env's logit is therefore the same bits whichever envs share its wave and in whichever order the envs are visited.
//   Parameters: read as A fragments from the group's block (global memory, L1/L2-resident: 25 KB for [64, 64]) where
//     they are used, so no register holds a parameter across the day loop.
// Every MFMA runs in wave-uniform control flow; lanes with no live env feed zeros.
struct MlpRolloutArgs {
  RolloutArgs r;           // tables, state, outputs, visiting order, n_steps (r.pol: require_budget and seed only)
  const float *params;     // [n_groups][stride] (w2a.h: w2a_mlp_policy)
  const int32_t *group;    // [n] group of every env (nullable = group 0); clamped into [0, n_groups) -- never read outside
  int32_t n_groups;
  int32_t stride;          // floats per group block
  int32_t activation;      // W2A_MLP_TANH / W2A_MLP_RELU
  int32_t n_obs;
  uint32_t obs_mask;       // bit k: slot k is an observation column (the others feed zeros)
  float *obs;              // [n][n_obs] in: the row every env holds; out: the row it holds when the call ends
  int8_t slot_obs[RO64_SLOTS];  // slot -> observation column, -1 = none
  const uint32_t *gate;    // [n][gate_words] allowed days, as LinearRolloutArgs::gate: read by the GATE = true
                           // instantiations only (the *_gated entry points); NULL selects GATE = false on the host
  int32_t gate_words;
  LookArgs look;           // policy["lookahead"] (w2a_lookahead.hip.h; look.weight unused: the rows W1f[12][width] sit at
                           // the tail of every block, w2a.h: W2A_MLP_LOOKAHEAD_STRIDE): read by the LOOK = true
                           // instantiations only (the w2a_lookahead_* entry points); zero otherwise
};

#define MLP_XS 36  // LDS row of one env's input vector, in floats: 16-B aligned rows, conflict-free B-operand reads
#define MLP_WAVES (BLOCK / 64)

// the wave's lanes exchange their input rows through LDS: order every lane's LDS accesses before the next ones (no
// workgroup barrier -- the waves of a block leave the day loop at different days)
__device__ __forceinline__ void mlp_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

typedef float mlp_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float mlp_act(float x, int activation) {
  return activation == W2A_MLP_RELU ? fmaxf(x, 0.0f) : tanhf(x);  // tanhf: ocml, <= 2 ulp
}

// the logit of every lane's env under group block p; xs holds the wave's 64 input rows
// LOOK: after the 8 k-steps over the slots the first layer runs ceil(look_days / 4) more over the wave's lookahead
// rows xl ([64 envs][W2A_LOOK_PAD floats], zero past look_days) against W1f[W2A_LOOK_PAD][WIDTH] at the block's tail
template <int WIDTH, int LAYERS, bool LOOK = false>
__device__ __forceinline__ float mlp_logit(const float *__restrict__ p, const float *xs, int activation,
                                           const float *xl = nullptr, int look_days = 0) {
  constexpr int NT = WIDTH / 16;  // hidden tiles
  constexpr int NB = 4 / NT;      // blocks of 16 envs per pass: NT * NB = 4 accumulator tiles
  const int l = threadIdx.x & 63, lo = l & 15, hi = l >> 4;
  const float *W1 = p, *b1 = p + ROWF * WIDTH;
  const float *W2 = b1 + WIDTH, *b2 = W2 + WIDTH * WIDTH;
  const float *wo = LAYERS == 2 ? b2 + WIDTH : W2;
  const float bo = wo[WIDTH];
  float z = 0.0f;
#pragma unroll
  for (int b0 = 0; b0 < 4; b0 += NB) {
    mlp_f4 h[NB][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const mlp_f4 bias = *reinterpret_cast<const mlp_f4 *>(b1 + 16 * t + 4 * hi);  // bias first
#pragma unroll
      for (int j = 0; j < NB; ++j) h[j][t] = bias;
    }
#pragma unroll
    for (int ks = 0; ks < ROWF / 4; ++ks) {
      float xb[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) xb[j] = xs[(16 * (b0 + j) + lo) * MLP_XS + 4 * ks + hi];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float a = W1[(4 * ks + hi) * WIDTH + 16 * t + lo];
#pragma unroll
        for (int j = 0; j < NB; ++j) h[j][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xb[j], h[j][t], 0, 0, 0);
      }
    }
    if constexpr (LOOK) {
      const float *W1f = p + W2A_MLP_STRIDE(WIDTH, LAYERS);
#pragma unroll
      for (int ks = 0; ks < W2A_LOOK_PAD / 4; ++ks) {
        if (4 * ks < look_days) {  // wave-uniform
          float xb[NB];
#pragma unroll
          for (int j = 0; j < NB; ++j) xb[j] = xl[(16 * (b0 + j) + lo) * W2A_LOOK_PAD + 4 * ks + hi];
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const float a = W1f[(4 * ks + hi) * WIDTH + 16 * t + lo];
#pragma unroll
            for (int j = 0; j < NB; ++j) h[j][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xb[j], h[j][t], 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) h[j][t][i] = mlp_act(h[j][t][i], activation);
    if (LAYERS == 2) {
      mlp_f4 h2[NB][NT];
#pragma unroll
      for (int o = 0; o < NT; ++o) {
        const mlp_f4 bias = *reinterpret_cast<const mlp_f4 *>(b2 + 16 * o + 4 * hi);
#pragma unroll
        for (int j = 0; j < NB; ++j) h2[j][o] = bias;
      }
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int o = 0; o < NT; ++o) {
            const float a = W2[(16 * t + 4 * hi + i) * WIDTH + 16 * o + lo];
#pragma unroll
            for (int j = 0; j < NB; ++j) h2[j][o] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, h[j][t][i], h2[j][o], 0, 0, 0);
          }
#pragma unroll
      for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int o = 0; o < NT; ++o)
#pragma unroll
          for (int i = 0; i < 4; ++i) h[j][o][i] = mlp_act(h2[j][o][i], activation);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      float s = hi == 0 ? bo : 0.0f;  // b_out first
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const mlp_f4 w = *reinterpret_cast<const mlp_f4 *>(wo + 16 * t + 4 * hi);
#pragma unroll
        for (int i = 0; i < 4; ++i) s = fmaf(w[i], h[j][t][i], s);
      }
      s += __shfl_xor(s, 16);  // (l, l^16) then (l^32, l^48): the same f32 value on all four lanes
      s += __shfl_xor(s, 32);
      if (hi == b0 + j) z = s;
    }
  }
  return z;
}

// every lane's logit for the input rows in xs, over the distinct groups of the wave (wave-uniform loop)
template <int WIDTH, int LAYERS, bool LOOK = false>
__device__ __forceinline__ float mlp_logit_groups(const MlpRolloutArgs &ma, int32_t g, const float *xs,
                                                  const float *xl = nullptr) {
  float z = 0.0f;
  uint64_t todo = __ballot(1);
  while (todo) {
    const int32_t gw = __builtin_amdgcn_readfirstlane(__shfl(g, __ffsll((unsigned long long)todo) - 1));
    const float zg = mlp_logit<WIDTH, LAYERS, LOOK>(ma.params + (size_t)gw * ma.stride, xs, ma.activation, xl,
                                                    LOOK ? ma.look.days : 0);
    if (g == gw) z = zg;
    todo &= ~__ballot(g == gw);
  }
  return z;
}

// Registers: see DESIGN.md (k_rollout_mlp); held to 2 waves/SIMD like the other large day loops
// RECORD: the trajectory of w2a_rollout_mlp_record (k_rollout_linear's traj_record_day); RECORD = false compiles to the
// kernel without one
// GATE (w2a_rollout_mlp_gated): ma.gate restricts the attempts, as in k_rollout_linear; GATE = false compiles from the
// statements it had before the gate existed
// LOOK (w2a_lookahead_rollout_mlp and its _gated form): every lane also puts the lookahead inputs of the row it holds
// (w2a_lookahead.hip.h) into a second LDS region next to xs, and the first layer runs on over them. LOOK = false
// compiles from the statements it had before; there is no RECORD form.
// NOISE (w2a_forecast_rollout_mlp; needs LOOK): the lookahead inputs carry the forecast error of ma.look.mae, as in
// k_rollout_linear.
template <int WIDTH, int LAYERS, bool MASKS, bool RECORD, bool GATE, bool LOOK = false, bool NOISE = false>
__global__ __launch_bounds__(BLOCK, 2) void k_rollout_mlp(const MlpRolloutArgs ma, const int32_t sample,
                                                          const w2a_trajectory tr) {
  __shared__ __attribute__((aligned(16))) float s_x[MLP_WAVES][64 * MLP_XS];
  const RolloutArgs &a = ma.r;
  const int64_t slot64 = (int64_t)logical_block(blockIdx.x, gridDim.x >> 3) * BLOCK + threadIdx.x;
  if (slot64 - (threadIdx.x & 63) >= a.n) return;  // whole wave past the end
  const bool valid = slot64 < a.n;
  const uint32_t slot = (uint32_t)(valid ? slot64 : (a.n - 1));
  uint32_t e = a.order ? a.order[slot] : slot;  // the env this lane serves
  e = e < (uint32_t)a.n ? e : (uint32_t)(a.n - 1);
  float *xs = s_x[threadIdx.x >> 6];
  float *xrow = xs + (threadIdx.x & 63) * MLP_XS;
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
  // the env's two coefficient rows, once per launch
  float wb[32], we[32];
  {
    const float4 *wq = a.tb.W + (size_t)wrow * (2 * ROWF / 4);
#pragma unroll
    for (int q = 0; q < ROWF / 4; ++q) {
      const float4 b = wq[q], f = wq[ROWF / 4 + q];
      wb[4 * q] = b.x; wb[4 * q + 1] = b.y; wb[4 * q + 2] = b.z; wb[4 * q + 3] = b.w;
      we[4 * q] = f.x; we[4 * q + 1] = f.y; we[4 * q + 2] = f.z; we[4 * q + 3] = f.w;
    }
  }
  int32_t g = ma.group ? ma.group[e] : 0;
  g = g < 0 ? 0 : (g >= ma.n_groups ? ma.n_groups - 1 : g);
  const uint64_t pstream = sample ? rng_stream(a.pol.seed ^ 0xA5A5A5A55A5A5A5Aull, (uint64_t)(a.gid0 + e), cold.w) : 0ull;
  const uint32_t obs0 = e * (uint32_t)ma.n_obs;  // first element of the env's observation row (host: n * n_obs < 2^31)
  if (RECORD && valid) traj_copy_row(ma, tr, 0, e, obs0);  // slab 0: the row every env holds on entry
  float *stage = nullptr;  // staged store design: identity order (wave-uniform)
  if constexpr (RECORD) {
    __shared__ float s_traj[MLP_WAVES][TRAJ_TILE];
    if (!a.order) stage = s_traj[threadIdx.x >> 6];
  }
  float ret = 0.0f;
  int32_t alerts = 0, over = 0;
  uint32_t mask_word = 0, mask_idx = 0xFFFFFFFFu;
  uint32_t att_word = 0, att_idx = 0xFFFFFFFFu;
  float snap = 0.0f;
  bool snapped = false;
  uint32_t gate_word = 0, gate_idx = 0xFFFFFFFFu;
  bool active = !fin && valid;
  float *xl = nullptr, *xlrow = nullptr;  // the wave's lookahead rows and this lane's
  const float *lser = nullptr;
  if constexpr (LOOK) {
    __shared__ __attribute__((aligned(16))) float s_xl[MLP_WAVES][64 * W2A_LOOK_PAD];
    xl = s_xl[threadIdx.x >> 6];
    xlrow = xl + (threadIdx.x & 63) * W2A_LOOK_PAD;
    lser = look_series(ma.look, cold.x);
  }
  uint64_t estream = 0;
  if constexpr (NOISE) estream = look_noise_stream(ma.look, (uint64_t)(a.gid0 + e), cold.w);
  // first day: the logit of the observation row the agent holds (zeros for lanes with no live env)
#pragma unroll
  for (int k = 0; k < ROWF; ++k)
    xrow[k] = (k < RO64_SLOTS && ma.slot_obs[k] >= 0 && active) ? ma.obs[obs0 + ma.slot_obs[k]] : 0.0f;
  if constexpr (LOOK) {  // the held row is day max(t - 1, 0)'s: its lookahead inputs are rebuilt, never carried
    float lf[W2A_LOOK_MAX];
    look_inputs<NOISE>(ma.look, look_series_of<NOISE>(ma.look, lser, cold.x), t > 0 ? t - 1 : 0u, ndays, lf, estream);
#pragma unroll
    for (int k = 0; k < W2A_LOOK_PAD; ++k) xlrow[k] = (k < W2A_LOOK_MAX && active) ? lf[k < W2A_LOOK_MAX ? k : 0] : 0.0f;
  }
  mlp_wave_lds_sync();
  float z = mlp_logit_groups<WIDTH, LAYERS, LOOK>(ma, g, xs, xl);
  for (int s = 0; s < a.n_steps; ++s) {
    if (!__any(active)) break;
    // ---- policy: alert iff logit > 0, or u < sigmoid(logit) with the Bernoulli policy's uniform of (env, episode, day)
    int32_t act;
    if (sample) {
      const uint32_t u = (uint32_t)(w2a_mix64(pstream + (uint64_t)(t + 1) * 0x9E3779B97F4A7C15ull) >> 32);
      act = ((float)u * 2.3283064365386963e-10f < sigmoid_f32(z)) ? 1 : 0;
    } else {
      act = z > 0.0f ? 1 : 0;
    }
    if (a.pol.require_budget && budget - (int32_t)used <= 0) act = 0;
    if (GATE && active && !gate_allows(ma.gate, ma.gate_words, e, t, gate_word, gate_idx)) act = 0;  // not attempted
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
    double zb = 0.0, ze = 0.0;
#pragma unroll
    for (int k = 0; k < RO64_SLOTS; ++k) {
      asm volatile("" : "+v"(wb[k]), "+v"(we[k]));  // keep the coefficients f32 (see k_rollout64)
      const double xk = (double)xv[k];
      zb = fma(xk, (double)wb[k], zb);
      ze = fma(xk, (double)we[k], ze);
    }
    if (!(xv[30] > 0.5f)) ze = -__builtin_inf();
    const float r = reward_from_logits(zb, ze, actual);
    // tomorrow's network input: the observation columns of xv[] (zeros elsewhere and for lanes with no live env)
    mlp_wave_lds_sync();  // every lane's reads of the previous input are done
#pragma unroll
    for (int q = 0; q < ROWF / 4; ++q) {
      float4 v;
      v.x = (active && ((ma.obs_mask >> (4 * q)) & 1u)) ? xv[4 * q] : 0.0f;
      v.y = (active && ((ma.obs_mask >> (4 * q + 1)) & 1u)) ? xv[4 * q + 1] : 0.0f;
      v.z = (active && ((ma.obs_mask >> (4 * q + 2)) & 1u)) ? xv[4 * q + 2] : 0.0f;
      v.w = (active && ((ma.obs_mask >> (4 * q + 3)) & 1u)) ? xv[4 * q + 3] : 0.0f;
      reinterpret_cast<float4 *>(xrow)[q] = v;
    }
    if constexpr (LOOK) {  // xv[] is day t's row: tomorrow's decision looks ahead from day t
      float lf[W2A_LOOK_MAX];
      look_inputs<NOISE>(ma.look, look_series_of<NOISE>(ma.look, lser, cold.x), t, ndays, lf, estream);
#pragma unroll
      for (int k = 0; k < W2A_LOOK_PAD; ++k) xlrow[k] = (k < W2A_LOOK_MAX && active) ? lf[k < W2A_LOOK_MAX ? k : 0] : 0.0f;
    }
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
      if (RECORD) traj_record_day(ma, tr, s, e, obs0, xv, act, z, r, done, actual, stage);
      // the row the agent now holds is xv[] (a terminal step leaves the previous one): written back once, when it is
      // the last row of this call -- its last day, or the day before the terminal one
      if (!done && (s + 1 == a.n_steps || t + 2 >= ndays)) {
        uint32_t o = obs0;
        asm volatile("" : "+v"(o));
#pragma unroll
        for (int k = 0; k < RO64_SLOTS; ++k)
          if (ma.slot_obs[k] >= 0) ma.obs[o + ma.slot_obs[k]] = xv[k];
      }
      used = used2; hist = hist2; last = actual; atb = atb_s;
      if (!done) { streak = actual ? streak + 1 : 0; t = t + 1; }
      else { fin = true; active = false; }
    }
    if (RECORD && stage) traj_store_tile(ma, tr, s, (uint32_t)(slot64 - (threadIdx.x & 63)), stage);
    if (s + 1 < a.n_steps) {  // wave-uniform: the logit of the row each env now holds, for tomorrow
      mlp_wave_lds_sync();
      z = mlp_logit_groups<WIDTH, LAYERS, LOOK>(ma, g, xs, xl);
    }
  }
  if (RECORD && valid) traj_copy_row(ma, tr, a.n_steps, e, obs0);  // slab n_steps: the buffer as the call leaves it
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

// the host side's launch of one of the 24 instantiations (w2a_rollout_mlp, w2a_rollout_mlp_record: traj non-NULL)
template <int WIDTH, int LAYERS>
static void launch_rollout_mlp(const MlpRolloutArgs &ma, bool masks, int32_t sample, const w2a_trajectory *traj,
                               unsigned grid, hipStream_t s) {
  w2a_trajectory tr;
  memset(&tr, 0, sizeof(tr));
  if (traj) tr = *traj;
#define W2A_LAUNCH_MLP(M, R)                                                                                             \
  do {                                                                                                                   \
    if (ma.gate) hipLaunchKernelGGL((k_rollout_mlp<WIDTH, LAYERS, M, R, true>), dim3(grid), dim3(BLOCK), 0, s, ma, sample, tr); \
    else hipLaunchKernelGGL((k_rollout_mlp<WIDTH, LAYERS, M, R, false>), dim3(grid), dim3(BLOCK), 0, s, ma, sample, tr);   \
  } while (0)
  if (traj && masks) W2A_LAUNCH_MLP(true, true);
  else if (traj) W2A_LAUNCH_MLP(false, true);
  else if (masks) W2A_LAUNCH_MLP(true, false);
  else W2A_LAUNCH_MLP(false, false);
#undef W2A_LAUNCH_MLP
}

// the 24 LOOK instantiations (w2a_lookahead_rollout_mlp and its gated form): no trajectory
template <int WIDTH, int LAYERS>
static void launch_rollout_mlp_lookahead(const MlpRolloutArgs &ma, bool masks, int32_t sample, unsigned grid, hipStream_t s) {
  w2a_trajectory tr;
  memset(&tr, 0, sizeof(tr));
  if (ma.gate && masks) hipLaunchKernelGGL((k_rollout_mlp<WIDTH, LAYERS, true, false, true, true>), dim3(grid), dim3(BLOCK), 0, s, ma, sample, tr);
  else if (ma.gate) hipLaunchKernelGGL((k_rollout_mlp<WIDTH, LAYERS, false, false, true, true>), dim3(grid), dim3(BLOCK), 0, s, ma, sample, tr);
  else if (masks) hipLaunchKernelGGL((k_rollout_mlp<WIDTH, LAYERS, true, false, false, true>), dim3(grid), dim3(BLOCK), 0, s, ma, sample, tr);
  else hipLaunchKernelGGL((k_rollout_mlp<WIDTH, LAYERS, false, false, false, true>), dim3(grid), dim3(BLOCK), 0, s, ma, sample, tr);
}

// the 24 NOISE instantiations (w2a_forecast_rollout_mlp, allowed_days nullable): no trajectory
template <int WIDTH, int LAYERS>
static void launch_rollout_mlp_forecast(const MlpRolloutArgs &ma, bool masks, int32_t sample, unsigned grid, hipStream_t s) {
  w2a_trajectory tr;
  memset(&tr, 0, sizeof(tr));
  if (ma.gate && masks) hipLaunchKernelGGL((k_rollout_mlp<WIDTH, LAYERS, true, false, true, true, true>), dim3(grid), dim3(BLOCK), 0, s, ma, sample, tr);
  else if (ma.gate) hipLaunchKernelGGL((k_rollout_mlp<WIDTH, LAYERS, false, false, true, true, true>), dim3(grid), dim3(BLOCK), 0, s, ma, sample, tr);
  else if (masks) hipLaunchKernelGGL((k_rollout_mlp<WIDTH, LAYERS, true, false, false, true, true>), dim3(grid), dim3(BLOCK), 0, s, ma, sample, tr);
  else hipLaunchKernelGGL((k_rollout_mlp<WIDTH, LAYERS, false, false, false, true, true>), dim3(grid), dim3(BLOCK), 0, s, ma, sample, tr);
}

#endif  // W2A_ROLLOUT_MLP_HIP_H
