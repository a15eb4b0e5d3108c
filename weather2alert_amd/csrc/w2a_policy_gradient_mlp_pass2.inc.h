// w2a_policy_gradient_mlp_pass2.inc.h -- the text of the MLP gradient's second pass. NOT a header: it is included once per
// kernel it defines, with PGM_PASS2_KERNEL (the kernel's name) and PGM_PASS2_HEADS (output rows of the parameter block)
// defined -- by w2a_policy_gradient_mlp.hip.h (k_pgm_pass2, HEADS = 1) and w2a_qlearn.hip.h (k_qg_pass2, HEADS = 2). The
// description of the pass, the matrix-core mapping and the bank argument are in w2a_policy_gradient_mlp.hip.h.
// HEADS = 2: the block ends in wo0[w], wo1[w], bo0, bo1, 2 pad (w2a.h: the two-head layout). day_alert[d] -- the alert
// issued on call-day s, which is the action a_s the coefficient belongs to -- selects the row the backward pass starts
// from, and dw_out / db_out are accumulated per head (a head's env-days feed 0 into the other head's chain). Nothing new
// goes through LDS: the bank argument and the fragment layouts hold as they are. Every HEADS == 2 branch is a
// compile-time constant, so HEADS = 1 compiles to the statements the kernel had before the parameter existed.
// PGM_PASS2_BOTH (defined by w2a_actor_critic.hip.h for k_ac_pass2, with HEADS = 2): BOTH output rows receive a
// coefficient on every env-day. The day record is read as the two coefficients themselves, day = (c_pi, c_v): no
// total - prefix, ga.total is not read, and the alert byte is only the alert issued. dh_last = (c_pi w_out0 + c_v w_out1)
// act', dw_out0 += c_pi h, dw_out1 += c_v h, db_out0 += c_pi, db_out1 += c_v. Every BOTH branch is a compile-time
// constant as well: without the macro the kernels compile from the statements they had before it existed.
template <int WIDTH, int LAYERS>
__global__ __launch_bounds__(64, 1) void PGM_PASS2_KERNEL(const MlpGradArgs ga) {
  constexpr int HEADS = PGM_PASS2_HEADS;
#ifdef PGM_PASS2_BOTH
  constexpr bool BOTH = true;
  static_assert(HEADS == 2, "PGM_PASS2_BOTH needs the two-head block");
#else
  constexpr bool BOTH = false;
#endif
  constexpr int NT = WIDTH / 16;           // hidden tiles
  constexpr int NB = 4 / NT;               // blocks of 16 envs per pass
  constexpr int ND = WIDTH == 16 ? 2 : 1;  // copies of every weight-gradient tile (even / odd k-steps)
  constexpr int P = PgmPitch<WIDTH>::P;
  constexpr int TB = NB * 16 * P;          // floats of one transposed buffer
  __shared__ __attribute__((aligned(16))) float s_xs[64 * MLP_XS];
  __shared__ __attribute__((aligned(16))) float s_xt[64 * PGM_XT];
  __shared__ __attribute__((aligned(16))) float s_t[(LAYERS == 2 ? 3 : 1) * TB];  // one hidden layer: dh1T only
  const MlpRolloutArgs &ma = ga.m;
  const RolloutArgs &a = ma.r;
  const int l = threadIdx.x, lo = l & 15, hi = l >> 4;
  const uint32_t w = blockIdx.x;
  const size_t n = (size_t)a.n;
  const int activation = ma.activation;
  const uint32_t rows_per_day = (uint32_t)(a.tb.S_w * a.tb.Y);
  float *dh1T = s_t, *h1T = s_t + (LAYERS == 2 ? TB : 0), *dh2T = s_t + (LAYERS == 2 ? 2 * TB : 0);
  int32_t cur = -1;
  uint32_t pslot = ga.chunk_base[w], pcnt = 0;
  bool fresh = true;
  for (int tile = 0; tile < ga.tiles; ++tile) {
    const int64_t first = ((int64_t)w * ga.tiles + tile) * 64;
    if (first >= a.n) break;
    const bool valid = first + l < a.n;
    const uint32_t slot = (uint32_t)(valid ? first + l : a.n - 1);
    uint32_t e = a.order ? a.order[slot] : slot;
    e = e < (uint32_t)a.n ? e : (uint32_t)(a.n - 1);
    uint4 c2, hot;
    load_step_state(a.st, e, c2, hot);
    const uint4 cold = load_cold(a.st, e);
    const uint32_t t0 = D0_T(hot.x), used0 = D0_USED(hot.x), streak0 = D0_STREAK(hot.x), hist0 = D1_HIST(hot.y);
    const int32_t budget = (int32_t)hot.w;
    const uint32_t obs0 = e * (uint32_t)ma.n_obs;
    const int32_t g = valid ? pgm_group(ma, e) : -1;
    const double total = (!BOTH && valid) ? ga.total[slot] : 0.0;
    const int32_t nv_all = valid ? ga.n_valid[slot] : 0;
    uint64_t todo = __ballot(valid);
    while (todo) {
      const int32_t gw = __builtin_amdgcn_readfirstlane(__shfl(g, __ffsll((unsigned long long)todo) - 1));
      const bool mine = g == gw;
      todo &= ~__ballot(mine);
      if (gw != cur) {
        if (cur != -1) {
          if (l == 0 && pslot < ga.capacity) { ga.tag[pslot] = cur; ga.pcount[pslot] = pcnt; }
          ++pslot;
          fresh = true;
        }
        cur = gw;
        pcnt = 0;
      }
      pcnt += (uint32_t)__popcll((unsigned long long)__ballot(mine));
      const float *pg = ma.params + (size_t)gw * ma.stride;
      // ---- the accumulators of this (tile, group) pass
      mlp_f4 dW1[ND][2][NT], dW2[ND][NT][NT], dwo[NT];
      float db1[NT], db2[NT], dbo = 0.0f;
      mlp_f4 dwo_b[HEADS == 2 ? NT : 1];  // HEADS = 2: the second output row's accumulators
      float dbo_b = 0.0f;
      const mlp_f4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          dW1[d][0][t] = zero4; dW1[d][1][t] = zero4;
#pragma unroll
          for (int k = 0; k < NT; ++k) dW2[d][k][t] = zero4;
        }
#pragma unroll
      for (int t = 0; t < NT; ++t) { dwo[t] = zero4; db1[t] = 0.0f; db2[t] = 0.0f; }
      if (HEADS == 2) {
#pragma unroll
        for (int t = 0; t < NT; ++t) dwo_b[t] = zero4;
      }
      // ---- the days of the lanes of group gw
      const int32_t nv = mine ? nv_all : 0;
      uint32_t t = t0, used = used0, streak = streak0, hist = hist0;
      double prefix = 0.0;
      for (int s = 0; s < a.n_steps; ++s) {
        const bool live = s < nv;
        if (!__any(live)) break;
        // the parameters are read as fragments where they are used, every day anew (L1/L2-resident): the pointer is
        // opaque per day, so that no register holds a parameter across the day loop
        const float *p = pg;
        asm volatile("" : "+s"(p));
        const float *W1 = p, *b1 = p + ROWF * WIDTH;
        const float *W2 = b1 + WIDTH, *b2 = W2 + WIDTH * WIDTH;
        const float *wo = LAYERS == 2 ? b2 + WIDTH : W2;
        float xv[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) xv[k] = 0.0f;
        float c = 0.0f;
        float cv = 0.0f;  // BOTH: the second output row's coefficient
        int head = 0;  // HEADS = 2: the output row of the action taken on call-day s
        if (live) {
          const size_t d = (size_t)s * n + slot;
          const float2 da = ga.day[d];
          if (HEADS == 2 && !BOTH) head = ga.day_alert[d];
          if (s == 0) {  // the row the env holds on entry
#pragma unroll
            for (int k = 0; k < RO64_SLOTS; ++k)
              if (ma.slot_obs[k] >= 0) xv[k] = ma.obs[obs0 + ma.slot_obs[k]];
          } else {       // the vector of call-day s - 1
            const uint32_t actual = ga.day_alert[d - n];
            used += actual;
            hist = ((hist << 1) | actual) & 0x3FFFu;
            const float4 *xp = a.tb.X + (size_t)(t * rows_per_day + cold.x) * (ROWF / 4);
#pragma unroll
            for (int q = 0; q < ROWF / 4; ++q) {
              if (q == RT_QUAD) continue;
              const float4 v = xp[q];
              xv[4 * q] = v.x; xv[4 * q + 1] = v.y; xv[4 * q + 2] = v.z; xv[4 * q + 3] = v.w;
            }
            xv[4 * RT_QUAD] = (t > 0) ? (float)actual : 0.0f;
            xv[4 * RT_QUAD + 1] = (float)streak;
            xv[4 * RT_QUAD + 2] = (float)(budget - (int32_t)used);
            xv[4 * RT_QUAD + 3] = (float)__popc(hist);
#pragma unroll
            for (int k = 0; k < 32; ++k) xv[k] = ((ma.obs_mask >> k) & 1u) ? xv[k] : 0.0f;
            streak = actual ? streak + 1 : 0;  // call-day s - 1 was not terminal: the env stepped again on call-day s
            t = t + 1;
          }
          if (BOTH) {
            c = da.x;
            cv = da.y;
          } else {
            c = (float)((double)da.x * (total - prefix));  // delta_s Q_s
            prefix += (double)da.y;
          }
        }
        if (BOTH) {
          dbo += c;
          dbo_b += cv;
        } else if (HEADS == 2) {
          dbo += head ? 0.0f : c;
          dbo_b += head ? c : 0.0f;
        } else {
          dbo += c;
        }
        mlp_wave_lds_sync();  // every lane's reads of the previous day are done
#pragma unroll
        for (int q = 0; q < ROWF / 4; ++q) {
          const float4 v = make_float4(xv[4 * q], xv[4 * q + 1], xv[4 * q + 2], xv[4 * q + 3]);
          reinterpret_cast<float4 *>(s_xs + l * MLP_XS)[q] = v;
          reinterpret_cast<float4 *>(s_xt + l * PGM_XT)[q] = v;
        }
        mlp_wave_lds_sync();
#pragma unroll
        for (int b0 = 0; b0 < 4; b0 += NB) {
          // ---- forward, as mlp_logit, keeping the activations
          mlp_f4 h1[NB][NT], h2[NB][NT];
#pragma unroll
          for (int tt = 0; tt < NT; ++tt) {
            const mlp_f4 bias = *reinterpret_cast<const mlp_f4 *>(b1 + 16 * tt + 4 * hi);
#pragma unroll
            for (int j = 0; j < NB; ++j) h1[j][tt] = bias;
          }
#pragma unroll
          for (int ks = 0; ks < ROWF / 4; ++ks) {
            float xb[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) xb[j] = s_xs[(16 * (b0 + j) + lo) * MLP_XS + 4 * ks + hi];
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) {
              const float av = W1[(4 * ks + hi) * WIDTH + 16 * tt + lo];
#pragma unroll
              for (int j = 0; j < NB; ++j) h1[j][tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xb[j], h1[j][tt], 0, 0, 0);
            }
          }
#pragma unroll
          for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int tt = 0; tt < NT; ++tt)
#pragma unroll
              for (int i = 0; i < 4; ++i) h1[j][tt][i] = mlp_act(h1[j][tt][i], activation);
          if (LAYERS == 2) {
#pragma unroll
            for (int o = 0; o < NT; ++o) {
              const mlp_f4 bias = *reinterpret_cast<const mlp_f4 *>(b2 + 16 * o + 4 * hi);
#pragma unroll
              for (int j = 0; j < NB; ++j) h2[j][o] = bias;
            }
#pragma unroll
            for (int tt = 0; tt < NT; ++tt)
#pragma unroll
              for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int o = 0; o < NT; ++o) {
                  const float av = W2[(16 * tt + 4 * hi + i) * WIDTH + 16 * o + lo];
#pragma unroll
                  for (int j = 0; j < NB; ++j)
                    h2[j][o] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, h1[j][tt][i], h2[j][o], 0, 0, 0);
                }
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
              for (int o = 0; o < NT; ++o)
#pragma unroll
                for (int i = 0; i < 4; ++i) h2[j][o][i] = mlp_act(h2[j][o][i], activation);
          }
          // ---- backward: dz/dh_last = w_out, scaled by this env's c
          mlp_f4 dh1[NB][NT];
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            const float cb = __shfl(c, 16 * (b0 + j) + lo);
            const float cvb = BOTH ? __shfl(cv, 16 * (b0 + j) + lo) : 0.0f;
            const int hb = (HEADS == 2 && !BOTH) ? __shfl(head, 16 * (b0 + j) + lo) : 0;
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) {
              mlp_f4 wv = *reinterpret_cast<const mlp_f4 *>(wo + 16 * tt + 4 * hi);
              mlp_f4 wv_2 = wv;  // BOTH: the second output row
              if (HEADS == 2) {
                const mlp_f4 wv_b = *reinterpret_cast<const mlp_f4 *>(wo + WIDTH + 16 * tt + 4 * hi);
                if (BOTH) wv_2 = wv_b;
                else wv = hb ? wv_b : wv;
              }
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const float hl = LAYERS == 2 ? h2[j][tt][i] : h1[j][tt][i];
                if (BOTH) {
                  dwo[tt][i] = fmaf(cb, hl, dwo[tt][i]);
                  dwo_b[tt][i] = fmaf(cvb, hl, dwo_b[tt][i]);
                } else if (HEADS == 2) {
                  dwo[tt][i] = fmaf(hb ? 0.0f : cb, hl, dwo[tt][i]);
                  dwo_b[tt][i] = fmaf(hb ? cb : 0.0f, hl, dwo_b[tt][i]);
                } else {
                  dwo[tt][i] = fmaf(cb, hl, dwo[tt][i]);
                }
                const float dv = BOTH ? fmaf(cvb, wv_2[i], cb * wv[i]) * pgm_dact(hl, activation)
                                      : cb * wv[i] * pgm_dact(hl, activation);
                if (LAYERS == 2) h2[j][tt][i] = dv;  // h2 now holds dh2
                else dh1[j][tt][i] = dv;
              }
            }
          }
          if (LAYERS == 2) {
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
              for (int tt = 0; tt < NT; ++tt) {
                *reinterpret_cast<mlp_f4 *>(h1T + (16 * j + lo) * P + 16 * tt + 4 * hi) = h1[j][tt];
                *reinterpret_cast<mlp_f4 *>(dh2T + (16 * j + lo) * P + 16 * tt + 4 * hi) = h2[j][tt];
                dh1[j][tt] = zero4;
              }
            // dh1^T = W2 . dh2^T (A = W2[input unit on lo][output unit on k], B = dh2 in C layout)
#pragma unroll
            for (int tt = 0; tt < NT; ++tt)
#pragma unroll
              for (int kt = 0; kt < NT; ++kt) {
                const mlp_f4 a4 = *reinterpret_cast<const mlp_f4 *>(W2 + (16 * kt + lo) * WIDTH + 16 * tt + 4 * hi);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                  for (int j = 0; j < NB; ++j)
                    dh1[j][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[i], h2[j][tt][i], dh1[j][kt], 0, 0, 0);
              }
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
              for (int tt = 0; tt < NT; ++tt)
#pragma unroll
                for (int i = 0; i < 4; ++i) dh1[j][tt][i] *= pgm_dact(h1[j][tt][i], activation);
          }
#pragma unroll
          for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int tt = 0; tt < NT; ++tt)
              *reinterpret_cast<mlp_f4 *>(dh1T + (16 * j + lo) * P + 16 * tt + 4 * hi) = dh1[j][tt];
          mlp_wave_lds_sync();
          // ---- weight gradients: GEMMs over the pass's envs, 4 per k-step
#pragma unroll
          for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              constexpr int dmask = ND - 1;
              const int d = (4 * j + q) & dmask;
              const int row = (16 * j + 4 * q + hi) * P + lo;
              float bd1[NT], ax[2];
#pragma unroll
              for (int ut = 0; ut < NT; ++ut) {
                bd1[ut] = dh1T[row + 16 * ut];
                db1[ut] += bd1[ut];
              }
#pragma unroll
              for (int mt = 0; mt < 2; ++mt) ax[mt] = s_xt[(16 * (b0 + j) + 4 * q + hi) * PGM_XT + 16 * mt + lo];
#pragma unroll
              for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int ut = 0; ut < NT; ++ut)
                  dW1[d][mt][ut] = __builtin_amdgcn_mfma_f32_16x16x4f32(ax[mt], bd1[ut], dW1[d][mt][ut], 0, 0, 0);
              if (LAYERS == 2) {
                float a1[NT], bd2[NT];
#pragma unroll
                for (int ut = 0; ut < NT; ++ut) {
                  a1[ut] = h1T[row + 16 * ut];
                  bd2[ut] = dh2T[row + 16 * ut];
                  db2[ut] += bd2[ut];
                }
#pragma unroll
                for (int kt = 0; kt < NT; ++kt)
#pragma unroll
                  for (int ut = 0; ut < NT; ++ut)
                    dW2[d][kt][ut] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[kt], bd2[ut], dW2[d][kt][ut], 0, 0, 0);
              }
            }
          if (b0 + NB < 4) mlp_wave_lds_sync();  // the transposed buffers are free for the next pass
        }
      }
      // ---- the pass's registers into the wave's current partial block (fp64, wave-private, fixed order)
      // folds: biases over hi (the envs = hi mod 4), dw_out over lo (the envs of a block), db_out over the wave
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        db1[tt] += __shfl_xor(db1[tt], 16); db1[tt] += __shfl_xor(db1[tt], 32);
        db2[tt] += __shfl_xor(db2[tt], 16); db2[tt] += __shfl_xor(db2[tt], 32);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int m = 1; m < 16; m <<= 1) dwo[tt][i] += __shfl_xor(dwo[tt][i], m);
      }
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) dbo += __shfl_xor(dbo, m);
      if (HEADS == 2) {
#pragma unroll
        for (int tt = 0; tt < NT; ++tt)
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) dwo_b[tt][i] += __shfl_xor(dwo_b[tt][i], m);
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) dbo_b += __shfl_xor(dbo_b, m);
      }
      if (pslot < ga.capacity) {
        double *part = ga.partial + (size_t)pslot * ma.stride;
        const int oW2 = ROWF * WIDTH + WIDTH;
        const int oWo = LAYERS == 2 ? oW2 + WIDTH * WIDTH + WIDTH : oW2;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int ut = 0; ut < NT; ++ut)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              float v = dW1[0][mt][ut][i];
              if (ND == 2) v += dW1[ND - 1][mt][ut][i];
              pgm_put(part, fresh, (16 * mt + 4 * hi + i) * WIDTH + 16 * ut + lo, v);
            }
        if (LAYERS == 2) {
#pragma unroll
          for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int ut = 0; ut < NT; ++ut)
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                float v = dW2[0][kt][ut][i];
                if (ND == 2) v += dW2[ND - 1][kt][ut][i];
                pgm_put(part, fresh, oW2 + (16 * kt + 4 * hi + i) * WIDTH + 16 * ut + lo, v);
              }
        }
        if (hi == 0) {
#pragma unroll
          for (int tt = 0; tt < NT; ++tt) {
            pgm_put(part, fresh, ROWF * WIDTH + 16 * tt + lo, db1[tt]);
            if (LAYERS == 2) pgm_put(part, fresh, oW2 + WIDTH * WIDTH + 16 * tt + lo, db2[tt]);
          }
        }
        if (lo == 0) {
#pragma unroll
          for (int tt = 0; tt < NT; ++tt)
#pragma unroll
            for (int i = 0; i < 4; ++i) pgm_put(part, fresh, oWo + 16 * tt + 4 * hi + i, dwo[tt][i]);
        }
        if (HEADS == 2) {  // wo0[w] (above), wo1[w], bo0, bo1 and the block's two padding floats
          if (lo == 0) {
#pragma unroll
            for (int tt = 0; tt < NT; ++tt)
#pragma unroll
              for (int i = 0; i < 4; ++i) pgm_put(part, fresh, oWo + WIDTH + 16 * tt + 4 * hi + i, dwo_b[tt][i]);
          }
          if (l == 0) pgm_put(part, fresh, oWo + 2 * WIDTH, dbo);
          if (l == 1) pgm_put(part, fresh, oWo + 2 * WIDTH + 1, dbo_b);
          if (l >= 2 && l < 4 && fresh) part[oWo + 2 * WIDTH + l] = 0.0;
        } else {
          if (l == 0) pgm_put(part, fresh, oWo + WIDTH, dbo);
          if (l >= 1 && l < 4 && fresh) part[oWo + WIDTH + l] = 0.0;  // the block's three padding floats
        }
      }
      fresh = false;
    }
  }
  if (cur != -1 && l == 0 && pslot < ga.capacity) { ga.tag[pslot] = cur; ga.pcount[pslot] = pcnt; }
}
