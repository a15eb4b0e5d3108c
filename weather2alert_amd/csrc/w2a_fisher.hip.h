// w2a_fisher.hip.h -- Fisher-vector products of a linear or MLP policy along a GIVEN alert schedule (natural gradient, TRPO)
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_FISHER_HIP_H
#define W2A_FISHER_HIP_H

// ----------------------------------------------------------------------------------------
// F v over the episodes at hand (w2a_fisher_vector_product_linear / _mlp, estimator in w2a.h)
// ----------------------------------------------------------------------------------------
// The env is forced along its schedule exactly as in w2a_surrogate.hip.h: the same bitmap, the same attempted-versus-issued
// rule, the same rows, the same m_s. The Fisher information of one Bernoulli decision with logit z_s is
// p_s (1 - p_s) J_s^T J_s, J_s = dz_s/dtheta, so F v is the backward pass the other gradients run with the coefficient
//   c_s = w_e p_s (1 - p_s) u_s,   u_s = J_s . v_g
// and the only new device work is u_s: a second dot product (linear), a forward-mode tangent pass next to the logit (MLP).
//   k_fisher_linear  k_surrogate_linear's shape: one pass, lane = env, no scratch; a second masked row wv[] and a second
//                    fp64 FMA chain
//   mlp_logit_jvp    mlp_logit with the tangent accumulators next to the primal ones; z is mlp_logit's, bit for bit
//   k_fv_pass1       k_sg_pass1's day loop; leaves day = (f32(c_s), 0), the alert issued, total = 1 and n_valid, so the
//                    count, scan, pass 2 and reduce kernels of w2a_policy_gradient_mlp.hip.h run unchanged
// Every per-day scalar past u_s (p, 1 - p, c, the sum of q_e) is fp64. No floating-point atomics: identical calls give
// identical bits.
struct FisherArgs {
  const uint32_t *alert_mask;  // [n][mask_words] the schedule, as ImitationArgs
  int32_t mask_words;
  const float *env_weight;     // [n] w_e (nullable = 1)
  float *quadratic;            // [n] q_e = sum_s m_s p_s (1 - p_s) u_s^2 (unweighted)
  int32_t *days;               // [n] sum_s m_s
};

struct FvLinearArgs {
  LinearRolloutArgs l;     // as w2a_rollout_linear builds it (r.pol: require_budget only); l.obs is only read
  FisherArgs fv;
  const float4 *vec_weight;  // [n_groups][32] the vector's weight block, slot order as l.weight
  const float *vec_bias;     // [n_groups]
  float *grad;               // [n_obs + 1][n] per-env product, column-major as SgLinearArgs
};

struct FvMlpArgs {
  MlpGradArgs g;           // as w2a_policy_gradient_mlp builds it (baseline unused)
  FisherArgs fv;
  const float *vec;        // [n_groups][stride] the vector, in the policy's packed layout and stride
};

// One scored day: returns c_s = w_e p q u and adds p q u^2 to the env's sum. p and q = 1 - p without cancellation, from
// e = exp(-|z|), as sg_day forms them.
__device__ __forceinline__ double fv_day(double w_e, double z, double u, double &quad) {
  const double e = exp(-fabs(z));
  const double r = 1.0 / (1.0 + e);
  const double p = z >= 0.0 ? r : e * r, q = z >= 0.0 ? e * r : r;
  const double pqu = (p * q) * u;
  quad = fma(pqu, u, quad);
  return w_e * pqu;
}

// Registers: as k_surrogate_linear plus the vector's row; at two waves per SIMD it spills (DESIGN.md has the figures).
// GATE: fa.l.gate restricts the scored days, as in k_surrogate_linear<GATE>; a NULL gate selects GATE = false on the host.
template <bool GATE>
__global__ __launch_bounds__(BLOCK, 2) void k_fisher_linear(const FvLinearArgs fa) {
  const LinearRolloutArgs &la = fa.l;
  const RolloutArgs &a = la.r;
  const int64_t slot64 = (int64_t)logical_block(blockIdx.x, gridDim.x >> 3) * BLOCK + threadIdx.x;
  if (slot64 >= a.n) return;
  const uint32_t slot = (uint32_t)slot64;
  const uint32_t e = a.order ? a.order[slot] : slot;  // the env this lane serves
  uint4 c2, hot;
  load_step_state(a.st, e, c2, hot);
  const uint4 cold = load_cold(a.st, e);
  uint32_t t = D0_T(hot.x), used = D0_USED(hot.x), streak = D0_STREAK(hot.x), hist = D1_HIST(hot.y);
  const uint32_t ndays = D1_NDAYS(hot.y);
  const int32_t budget = (int32_t)hot.w;
  const uint32_t rows_per_day = (uint32_t)(a.tb.S_w * a.tb.Y);
  const uint32_t obs0 = e * (uint32_t)la.n_obs;
  const size_t n = (size_t)a.n;
  float wp[32], wv[32];
  {
    int32_t g = la.group ? la.group[e] : 0;
    g = g < 0 ? 0 : (g >= la.n_groups ? la.n_groups - 1 : g);  // the vector is read with the same clamped id
    const float4 *pq = la.weight + (size_t)g * (ROWF / 4);
    const float4 *vq = fa.vec_weight + (size_t)g * (ROWF / 4);
#pragma unroll
    for (int q = 0; q < ROWF / 4; ++q) {
      const float4 p = pq[q], v = vq[q];
      wp[4 * q] = p.x; wp[4 * q + 1] = p.y; wp[4 * q + 2] = p.z; wp[4 * q + 3] = p.w;
      wv[4 * q] = v.x; wv[4 * q + 1] = v.y; wv[4 * q + 2] = v.z; wv[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      wp[k] = ((la.obs_mask >> k) & 1u) ? wp[k] : 0.0f;
      wv[k] = ((la.obs_mask >> k) & 1u) ? wv[k] : 0.0f;
    }
    wp[31] = la.bias[g];  // the biases ride in slot 31, as in k_rollout_linear
    wv[31] = fa.vec_bias[g];
  }
  const double w_e = fa.fv.env_weight ? (double)fa.fv.env_weight[e] : 1.0;
  uint32_t lab_word = 0, lab_idx = 0xFFFFFFFFu;
  uint32_t gate_word = 0, gate_idx = 0xFFFFFFFFu;
  double g[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) g[k] = 0.0;  // slot k's column; the bias rides in slot 31, as in the policy row
  double quad = 0.0;
  int32_t scored = 0;
  bool active = D1_FIN(hot.y) == 0;
  // decision 0: the logit and the tangent of the observation row the agent holds, and its term of the product
  uint32_t lab = 0;      // a_s of the decision at hand
  bool scores = false;   // m_s of the decision at hand
  if (active) {
    double z = (double)wp[31], u = (double)wv[31];
#pragma unroll
    for (int k = 0; k < RO64_SLOTS; ++k)
      if (la.slot_obs[k] >= 0) {
        const double xk = (double)la.obs[obs0 + la.slot_obs[k]];
        z = fma(xk, (double)wp[k], z);
        u = fma(xk, (double)wv[k], u);
      }
    lab = im_label_bits(fa.fv.alert_mask, fa.fv.mask_words, e, t, lab_word, lab_idx);
    scores = !(a.pol.require_budget && budget - (int32_t)used <= 0);
    if (GATE && !gate_allows(la.gate, la.gate_words, e, t, gate_word, gate_idx)) scores = false;
    if (scores) {
      const double c = fv_day(w_e, z, u, quad);
      scored = 1;
#pragma unroll
      for (int k = 0; k < RO64_SLOTS; ++k)
        if (la.slot_obs[k] >= 0) g[k] = c * (double)la.obs[obs0 + la.slot_obs[k]];
      g[31] = c;
    }
  }
  for (int s = 0; s < a.n_steps; ++s) {
    if (!__any(active)) break;
    // ---- the schedule's action; a day that is not scored is attempted as 0
    const int32_t act = scores ? (int32_t)lab : 0;
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
    xv[4 * RT_QUAD] = (t > 0) ? (float)actual : 0.0f;
    xv[4 * RT_QUAD + 1] = (float)streak;
    xv[4 * RT_QUAD + 2] = (float)(budget - (int32_t)used2);
    xv[4 * RT_QUAD + 3] = (float)__popc(hist2);
    double zp = (double)wp[31], up = (double)wv[31];
#pragma unroll
    for (int k = 0; k < RO64_SLOTS; ++k) {
      zp = fma((double)xv[k], (double)wp[k], zp);
      up = fma((double)xv[k], (double)wv[k], up);
    }
    if (active) {
      const bool done = (t + 1 >= ndays);
      used = used2; hist = hist2;
      if (!done) { streak = actual ? streak + 1 : 0; t = t + 1; }
      else active = false;
      // decision s + 1, on the row the lane holds right now
      if (active && s + 1 < a.n_steps) {
        lab = im_label_bits(fa.fv.alert_mask, fa.fv.mask_words, e, t, lab_word, lab_idx);
        scores = !(a.pol.require_budget && budget - (int32_t)used <= 0);
        if (GATE && !gate_allows(la.gate, la.gate_words, e, t, gate_word, gate_idx)) scores = false;
        if (scores) {
          const double c = fv_day(w_e, zp, up, quad);
          scored += 1;
#pragma unroll
          for (int k = 0; k < RO64_SLOTS; ++k)
            if (la.slot_obs[k] >= 0) g[k] = fma(c, (double)xv[k], g[k]);
          g[31] += c;
        }
      }
    }
  }
  // column-major, as k_policy_gradient_linear: a column's envs are contiguous
  float *out = fa.grad + e;
#pragma unroll
  for (int k = 0; k < RO64_SLOTS; ++k)
    if (la.slot_obs[k] >= 0) out[(size_t)la.slot_obs[k] * n] = (float)g[k];
  out[(size_t)la.n_obs * n] = (float)g[31];
  fa.fv.quadratic[e] = (float)quad;
  fa.fv.days[e] = scored;
}

// ------------------------------------------------------------------------------------------------ MLP: the tangent pass
// The logit of every lane's env under group block p and its directional derivative along the block v (same layout):
//   layer 1  a1 = W1 x + b1,  adot1 = V1 x + vb1,  h1 = act(a1),  hdot1 = act'(h1) adot1
//   layer 2  a2 = W2 h1 + b2, adot2 = W2 hdot1 + V2 h1 + vb2,  h2 = act(a2),  hdot2 = act'(h2) adot2
//   output   z = w_o . h + b_o,  u = w_o . hdot + v_o . h + vb_o
// Orientation, the LDS input tile, the layer-to-layer register reuse and the blocks are mlp_logit's: a tangent tile has
// its primal tile's layout, so hdot feeds the next layer's B operand as h does. The primal chain is mlp_logit's statement
// for statement (the same operands in the same order), so z is the same bits; nothing of it is reassociated to share work
// with the tangent. act' is taken from the activation's value by pgm_dact, the convention of the backward pass.
// Every MFMA runs in wave-uniform control flow; lanes with no live env feed zeros.
template <int WIDTH, int LAYERS>
__device__ __forceinline__ float mlp_logit_jvp(const float *__restrict__ p, const float *__restrict__ v, const float *xs,
                                               int activation, float &u_out) {
  constexpr int NT = WIDTH / 16;  // hidden tiles
  constexpr int NB = 4 / NT;      // blocks of 16 envs per pass: NT * NB = 4 primal and 4 tangent accumulator tiles
  const int l = threadIdx.x & 63, lo = l & 15, hi = l >> 4;
  const float *W1 = p, *b1 = p + ROWF * WIDTH;
  const float *W2 = b1 + WIDTH, *b2 = W2 + WIDTH * WIDTH;
  const float *wo = LAYERS == 2 ? b2 + WIDTH : W2;
  const float bo = wo[WIDTH];
  const float *V1 = v, *vb1 = v + ROWF * WIDTH;
  const float *V2 = vb1 + WIDTH, *vb2 = V2 + WIDTH * WIDTH;
  const float *vo = LAYERS == 2 ? vb2 + WIDTH : V2;
  const float vbo = vo[WIDTH];
  float z = 0.0f, u = 0.0f;
#pragma unroll
  for (int b0 = 0; b0 < 4; b0 += NB) {
    mlp_f4 h[NB][NT], hd[NB][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const mlp_f4 bias = *reinterpret_cast<const mlp_f4 *>(b1 + 16 * t + 4 * hi);  // bias first
      const mlp_f4 vbias = *reinterpret_cast<const mlp_f4 *>(vb1 + 16 * t + 4 * hi);
#pragma unroll
      for (int j = 0; j < NB; ++j) { h[j][t] = bias; hd[j][t] = vbias; }
    }
#pragma unroll
    for (int ks = 0; ks < ROWF / 4; ++ks) {
      float xb[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) xb[j] = xs[(16 * (b0 + j) + lo) * MLP_XS + 4 * ks + hi];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float a = W1[(4 * ks + hi) * WIDTH + 16 * t + lo];
        const float av = V1[(4 * ks + hi) * WIDTH + 16 * t + lo];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          h[j][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xb[j], h[j][t], 0, 0, 0);
          hd[j][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xb[j], hd[j][t], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          h[j][t][i] = mlp_act(h[j][t][i], activation);
          hd[j][t][i] = pgm_dact(h[j][t][i], activation) * hd[j][t][i];
        }
    if (LAYERS == 2) {
      mlp_f4 h2[NB][NT], hd2[NB][NT];
#pragma unroll
      for (int o = 0; o < NT; ++o) {
        const mlp_f4 bias = *reinterpret_cast<const mlp_f4 *>(b2 + 16 * o + 4 * hi);
        const mlp_f4 vbias = *reinterpret_cast<const mlp_f4 *>(vb2 + 16 * o + 4 * hi);
#pragma unroll
        for (int j = 0; j < NB; ++j) { h2[j][o] = bias; hd2[j][o] = vbias; }
      }
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int o = 0; o < NT; ++o) {
            const float a = W2[(16 * t + 4 * hi + i) * WIDTH + 16 * o + lo];
            const float av = V2[(16 * t + 4 * hi + i) * WIDTH + 16 * o + lo];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
              h2[j][o] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, h[j][t][i], h2[j][o], 0, 0, 0);
              hd2[j][o] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, hd[j][t][i], hd2[j][o], 0, 0, 0);
              hd2[j][o] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, h[j][t][i], hd2[j][o], 0, 0, 0);
            }
          }
#pragma unroll
      for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int o = 0; o < NT; ++o)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            h[j][o][i] = mlp_act(h2[j][o][i], activation);
            hd[j][o][i] = pgm_dact(h[j][o][i], activation) * hd2[j][o][i];
          }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      float s = hi == 0 ? bo : 0.0f;  // b_out first
      float sd = hi == 0 ? vbo : 0.0f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const mlp_f4 w = *reinterpret_cast<const mlp_f4 *>(wo + 16 * t + 4 * hi);
        const mlp_f4 wd = *reinterpret_cast<const mlp_f4 *>(vo + 16 * t + 4 * hi);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          s = fmaf(w[i], h[j][t][i], s);
          sd = fmaf(w[i], hd[j][t][i], sd);
          sd = fmaf(wd[i], h[j][t][i], sd);
        }
      }
      s += __shfl_xor(s, 16);  // (l, l^16) then (l^32, l^48): the same f32 value on all four lanes
      s += __shfl_xor(s, 32);
      sd += __shfl_xor(sd, 16);
      sd += __shfl_xor(sd, 32);
      if (hi == b0 + j) { z = s; u = sd; }
    }
  }
  u_out = u;
  return z;
}

// every lane's logit and tangent for the input rows in xs, over the distinct groups of the wave (wave-uniform loop); the
// vector's block is read at the policy's stride with the same clamped group id
template <int WIDTH, int LAYERS>
__device__ __forceinline__ float mlp_logit_jvp_groups(const MlpRolloutArgs &ma, const float *vec, int32_t g,
                                                      const float *xs, float &u_out) {
  float z = 0.0f, u = 0.0f;
  uint64_t todo = __ballot(1);
  while (todo) {
    const int32_t gw = __builtin_amdgcn_readfirstlane(__shfl(g, __ffsll((unsigned long long)todo) - 1));
    float ug;
    const float zg = mlp_logit_jvp<WIDTH, LAYERS>(ma.params + (size_t)gw * ma.stride, vec + (size_t)gw * ma.stride, xs,
                                                  ma.activation, ug);
    if (g == gw) { z = zg; u = ug; }
    todo &= ~__ballot(g == gw);
  }
  u_out = u;
  return z;
}

// ------------------------------------------------------------------------------------------------ MLP: pass 1
// GATE: as k_fisher_linear<GATE>
template <int WIDTH, int LAYERS, bool GATE>
__global__ __launch_bounds__(BLOCK, 2) void k_fv_pass1(const FvMlpArgs fa) {
  __shared__ __attribute__((aligned(16))) float s_x[MLP_WAVES][64 * MLP_XS];
  const MlpGradArgs &ga = fa.g;
  const MlpRolloutArgs &ma = ga.m;
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
  uint32_t t = D0_T(hot.x), used = D0_USED(hot.x), streak = D0_STREAK(hot.x), hist = D1_HIST(hot.y);
  const uint32_t ndays = D1_NDAYS(hot.y);
  const int32_t budget = (int32_t)hot.w;
  const uint32_t rows_per_day = (uint32_t)(a.tb.S_w * a.tb.Y);
  const int32_t g = pgm_group(ma, e);
  const uint32_t obs0 = e * (uint32_t)ma.n_obs;
  const size_t n = (size_t)a.n;
  const double w_e = fa.fv.env_weight ? (double)fa.fv.env_weight[e] : 1.0;
  uint32_t lab_word = 0, lab_idx = 0xFFFFFFFFu;
  uint32_t gate_word = 0, gate_idx = 0xFFFFFFFFu;
  double quad = 0.0;
  int32_t scored = 0, n_valid = 0;
  bool active = D1_FIN(hot.y) == 0 && valid;
#pragma unroll
  for (int k = 0; k < ROWF; ++k)
    xrow[k] = (k < RO64_SLOTS && ma.slot_obs[k] >= 0 && active) ? ma.obs[obs0 + ma.slot_obs[k]] : 0.0f;
  mlp_wave_lds_sync();
  float u;
  float z = mlp_logit_jvp_groups<WIDTH, LAYERS>(ma, fa.vec, g, xs, u);
  for (int s = 0; s < a.n_steps; ++s) {
    if (!__any(active)) break;
    const uint32_t lab = active ? im_label_bits(fa.fv.alert_mask, fa.fv.mask_words, e, t, lab_word, lab_idx) : 0u;
    int32_t act = (int32_t)lab;
    bool scores = true;
    if (a.pol.require_budget && budget - (int32_t)used <= 0) { act = 0; scores = false; }  // m_s = 0: forced
    if (GATE && active && !gate_allows(ma.gate, ma.gate_words, e, t, gate_word, gate_idx)) { act = 0; scores = false; }
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
    xv[4 * RT_QUAD] = (t > 0) ? (float)actual : 0.0f;
    xv[4 * RT_QUAD + 1] = (float)streak;
    xv[4 * RT_QUAD + 2] = (float)(budget - (int32_t)used2);
    xv[4 * RT_QUAD + 3] = (float)__popc(hist2);
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
    if (active) {
      const bool done = (t + 1 >= ndays);
      const size_t d = (size_t)s * n + slot;
      double c = 0.0;
      if (scores) { c = fv_day(w_e, (double)z, (double)u, quad); scored += 1; }
      ga.day[d] = make_float2((float)c, 0.0f);  // pass 2: c_s = day.x (1 - 0)
      ga.day_alert[d] = (uint8_t)actual;
      n_valid = s + 1;
      used = used2; hist = hist2;
      if (!done) { streak = actual ? streak + 1 : 0; t = t + 1; }
      else active = false;
    }
    if (s + 1 < a.n_steps) {  // wave-uniform: the logit and tangent of the row each env now holds, for tomorrow
      mlp_wave_lds_sync();
      z = mlp_logit_jvp_groups<WIDTH, LAYERS>(ma, fa.vec, g, xs, u);
    }
  }
  if (valid) {
    ga.total[slot] = 1.0;
    ga.n_valid[slot] = n_valid;
    fa.fv.quadratic[e] = (float)quad;
    fa.fv.days[e] = scored;
  }
}

template <int WIDTH, int LAYERS>
static void launch_fv(const FvMlpArgs &fa, unsigned grid1, hipStream_t s) {
  const MlpGradArgs &ga = fa.g;
  if (ga.m.gate) hipLaunchKernelGGL((k_fv_pass1<WIDTH, LAYERS, true>), dim3(grid1), dim3(BLOCK), 0, s, fa);
  else hipLaunchKernelGGL((k_fv_pass1<WIDTH, LAYERS, false>), dim3(grid1), dim3(BLOCK), 0, s, fa);
  hipLaunchKernelGGL(k_pgm_count, dim3(ga.n_chunks), dim3(64), 0, s, ga);
  hipLaunchKernelGGL(k_pgm_scan, dim3(1), dim3(1024), 0, s, ga);
  hipLaunchKernelGGL((k_pgm_pass2<WIDTH, LAYERS>), dim3(ga.n_chunks), dim3(64), 0, s, ga);
  hipLaunchKernelGGL(k_pgm_reduce, dim3(ga.m.n_groups, (ga.m.stride + 255) / 256), dim3(256), 0, s, ga);
}

#endif  // W2A_FISHER_HIP_H
