// w2a_policy_gradient_mlp.hip.h -- score-function gradient of a sampled MLP policy's rollout, reduced per group
// Part of libw2a.so; included only by w2a_kernels.hip (one translation unit, see the file comment there).
#ifndef W2A_POLICY_GRADIENT_MLP_HIP_H
#define W2A_POLICY_GRADIENT_MLP_HIP_H

// ----------------------------------------------------------------------------------------
// reward-to-go REINFORCE gradient of w2a_rollout_mlp(sample = 1) (w2a_policy_gradient_mlp, estimator in w2a.h)
// ----------------------------------------------------------------------------------------
// As k_policy_gradient_linear (w2a_policy_gradient.hip.h) the kernels run BEFORE the rollout they differentiate, on the
// state and the observation rows it will start from, and write neither. The parameter gradient of a [64, 64] block is
// 6 404 floats, so nothing is written per env: the gradient leaves the kernels already summed over envs.
//   k_pgm_pass1   k_rollout_mlp's day loop with sample = 1, statement for statement (same uniform, same
//                 mlp_logit_groups call on the same LDS rows, same two fp64 reward chains), plus the no-alert fork of
//                 k_policy_gradient_linear (the baseline chain branches off the played one after slot 23). Per
//                 (call-day, lane) 9 B of scratch: delta_s = m_s (a_s - sigmoid(z_s)), A_s = r_s - beta_s (f32) and the
//                 alert issued; per lane sum A (fp64) and the number of days stepped.
//   k_pgm_count / k_pgm_scan   how many partial blocks every wave of pass 2 will write, and where its first one goes
//                 (an exclusive scan): the partial index of a block depends on the visiting order only, never on timing.
//   k_pgm_pass2   one wave per workgroup covers `tiles` consecutive 64-env tiles of the visiting order. Per tile and per
//                 distinct group of its lanes (wave-uniform loop, as mlp_logit_groups; one pass with the group-major
//                 order the host passes) it walks the days again as the linear kernel's pass 2 does -- o_s is the entry
//                 row (s = 0) or the table row of the day before with its four run-time fields rebuilt from the start
//                 state and the stored alerts -- and per day: the wave's 64 rows to LDS, the forward pass keeping the
//                 hidden activations, c_s = delta_s Q_s (Q_s = sum A - sum_{s' < s} A_s' in fp64; 0 and a zero row for
//                 lanes that are not live or of another group), the backward pass, and the weight-gradient products.
//   k_pgm_reduce  per group and parameter: the partial blocks tagged with the group, summed in partial-index order in
//                 fp64, divided by the group's env count (the sum of the blocks' counts: 0 / 0 = NaN for a group without
//                 envs), rounded to f32 once. No floating-point atomics anywhere: identical calls give identical bits.
// Matrix-core mapping of pass 2 (v_mfma_f32_16x16x4_f32; A: lane l holds A[m = l & 15][k = l >> 4], B: B[k = l >> 4]
// [n = l & 15], C: register i holds C[m = 4 (l >> 4) + i][n = l & 15]; lo = l & 15, hi = l >> 4):
//   forward     mlp_logit's: units on M, the 16 envs of a block on N, NB = 4 / (width / 16) blocks together.
//   backward    dh1^T = W2 . dh2^T: input units on M, output units on K, envs on N. dh2 comes out of the elementwise
//               step in C layout, which is a B operand as it stands (k-step (t, i): unit 16 t + 4 hi + i), and the A
//               fragment W2[16 kt + lo][16 t + 4 hi .. + 3] is one 16-B load for the four k-steps i.
//   gradients   dW1 += x (x) dh1 and dW2 += h1 (x) dh2 are GEMMs over envs: K = 4 envs per instruction, both operands
//               want unit (or slot) on lo and env on hi, the transpose of the C layout. They go through LDS: each C tile
//               is stored as [env][unit] rows of pitch P floats, one 16-B store per lane and tile (row lo, units
//               16 t + 4 hi ..), and read back as dword [(4 q + hi) P + 16 t + lo] for k-step q.
//               Bank argument: a ds_read_b32 is served in two groups of 32 lanes, {0..31} and {32..63}, over 32 banks
//               of 4 B. Within a group hi takes two values h, h + 1 and lo all 16: the dword addresses are
//               c + h P + lo and c + (h + 1) P + lo, so with P = 16 (mod 32) the 32 lanes hit 32 different banks --
//               conflict-free. P = 16 / 48 / 80 for width 16 / 32 / 64, and the second copy of the input rows (xT,
//               the A operand of dW1) has P = 48. (The first copy keeps mlp_logit's pitch of 36 for the forward's
//               B-operand reads.)
//               Accumulator tiles in flight per k-step: 2 NT (dW1) + NT^2 (dW2), NT = width / 16; width 16 keeps two
//               copies of each (even / odd k-steps), so no instantiation has fewer than four independent chains.
//   biases      db = the sum of the transposed B operand itself (per lane over the envs = hi mod 4, hi folded at the
//               flush), dw_out += c h in C layout (lo folded at the flush), db_out += c per env lane.
// Numerics: every product and sum inside a tile's day loop is f32 (the MFMA's accumulator); after each (tile, group)
// pass the wave adds its registers into its current partial block in fp64 (wave-private read-modify-write, in program
// order), so an f32 chain is never longer than 16 MFMAs x the days of one tile.
struct MlpGradArgs {
  MlpRolloutArgs m;      // as w2a_rollout_mlp builds it (r.pol: require_budget and seed); m.obs is only read
  int32_t baseline;      // W2A_PG_BASELINE_*
  float2 *day;           // [n_steps][n] (delta_s, A_s) of the lane at visiting position `slot`
  uint8_t *day_alert;    // [n_steps][n] the alert issued on that call-day
  double *total;         // [n] sum of A_s over the days of the lane at `slot`
  int32_t *n_valid;      // [n] days it steps in this call
  int32_t tiles;         // 64-env tiles per wave of pass 2
  uint32_t n_chunks;     // waves of pass 2
  uint32_t *chunk_count; // [n_chunks] partial blocks the wave writes
  uint32_t *chunk_base;  // [n_chunks + 1] exclusive scan; [n_chunks] = all
  uint32_t capacity;     // partial blocks the workspace holds
  int32_t *tag;          // [capacity] group of the partial block
  uint32_t *pcount;      // [capacity] envs whose gradient it sums
  double *partial;       // [capacity][stride]
  float *grad;           // [n_groups][stride]
};

__device__ __forceinline__ int32_t pgm_group(const MlpRolloutArgs &ma, uint32_t e) {
  int32_t g = ma.group ? ma.group[e] : 0;
  return g < 0 ? 0 : (g >= ma.n_groups ? ma.n_groups - 1 : g);
}

// ------------------------------------------------------------------------------------------------ pass 1
// GATE (w2a_policy_gradient_mlp_gated): a day ga.m.gate closes is a forced choice, m_s = 0: it reaches pass 2 as a zero
// coefficient. GATE = false compiles from the statements it had before the gate existed
template <int WIDTH, int LAYERS, bool GATE>
__global__ __launch_bounds__(BLOCK, 2) void k_pgm_pass1(const MlpGradArgs ga) {
  __shared__ __attribute__((aligned(16))) float s_x[MLP_WAVES][64 * MLP_XS];
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
  const uint32_t used0 = used;
  const uint32_t ndays = D1_NDAYS(hot.y);
  const int32_t budget = (int32_t)hot.w;
  const uint32_t rows_per_day = (uint32_t)(a.tb.S_w * a.tb.Y);
  const uint32_t wrow = W_COL(cold.y) * (uint32_t)a.tb.n_samples + W_SAMPLE(cold.y);
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
  const int32_t g = pgm_group(ma, e);
  const uint64_t pstream = rng_stream(a.pol.seed ^ 0xA5A5A5A55A5A5A5Aull, (uint64_t)(a.gid0 + e), cold.w);
  const uint32_t obs0 = e * (uint32_t)ma.n_obs;
  // the no-alert fork (k_policy_gradient_linear): the budget stays at its start value, the streak is the start state's
  // on the first day and 0 after it, the 14-day window only decays
  uint32_t streak_f = streak, hist_f = hist;
  const size_t n = (size_t)a.n;
  double total = 0.0;
  int32_t n_valid = 0;
  uint32_t gate_word = 0, gate_idx = 0xFFFFFFFFu;
  bool active = D1_FIN(hot.y) == 0 && valid;
#pragma unroll
  for (int k = 0; k < ROWF; ++k)
    xrow[k] = (k < RO64_SLOTS && ma.slot_obs[k] >= 0 && active) ? ma.obs[obs0 + ma.slot_obs[k]] : 0.0f;
  mlp_wave_lds_sync();
  float z = mlp_logit_groups<WIDTH, LAYERS>(ma, g, xs);
  for (int s = 0; s < a.n_steps; ++s) {
    if (!__any(active)) break;
    const uint32_t u = (uint32_t)(w2a_mix64(pstream + (uint64_t)(t + 1) * 0x9E3779B97F4A7C15ull) >> 32);
    const float p = sigmoid_f32(z);
    int32_t act = ((float)u * 2.3283064365386963e-10f < p) ? 1 : 0;  // a_s: the policy's own draw
    float delta = (float)act - p;
    if (a.pol.require_budget && budget - (int32_t)used <= 0) { act = 0; delta = 0.0f; }  // m_s = 0: forced, off-policy
    if (GATE && active && !gate_allows(ma.gate, ma.gate_words, e, t, gate_word, gate_idx)) { act = 0; delta = 0.0f; }
    const uint32_t atb_s = ((int32_t)used == budget) ? 1u : 0u;
    const uint32_t actual = (act == 1 && atb_s) ? 0u : (uint32_t)act;
    const uint32_t used2 = used + actual;
    const uint32_t hist2 = ((hist << 1) | actual) & 0x3FFFu;
    const uint32_t hist_f2 = (hist_f << 1) & 0x3FFFu;
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
    const float xf[4] = {0.0f, (float)streak_f, (float)(budget - (int32_t)used0), (float)__popc(hist_f2)};
    double zb = 0.0, ze = 0.0, zf = 0.0;
#pragma unroll
    for (int k = 0; k < RO64_SLOTS; ++k) {
      asm volatile("" : "+v"(wb[k]), "+v"(we[k]));  // keep the coefficients f32 (see k_rollout64)
      if (k == 4 * RT_QUAD) zf = zb;  // the fork shares the prefix over slots 0..23
      const double xk = (double)xv[k];
      if (k >= 4 * RT_QUAD) zf = fma((k < 4 * RT_QUAD + 4) ? (double)xf[k - 4 * RT_QUAD] : xk, (double)wb[k], zf);
      zb = fma(xk, (double)wb[k], zb);
      ze = fma(xk, (double)we[k], ze);
    }
    if (!(xv[30] > 0.5f)) ze = -__builtin_inf();
    const float r = reward_from_logits(zb, ze, actual);
    const float beta = ga.baseline == W2A_PG_BASELINE_NO_ALERT ? reward_from_logits(zf, -__builtin_inf(), 0u) : 0.0f;
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
      const float adv = r - beta;
      const size_t d = (size_t)s * n + slot;
      ga.day[d] = make_float2(delta, adv);
      ga.day_alert[d] = (uint8_t)actual;
      total += (double)adv;
      n_valid = s + 1;
      used = used2; hist = hist2; hist_f = hist_f2;
      if (!done) { streak = actual ? streak + 1 : 0; streak_f = 0; t = t + 1; }
      else active = false;
    }
    if (s + 1 < a.n_steps) {  // wave-uniform: the logit of the row each env now holds, for tomorrow
      mlp_wave_lds_sync();
      z = mlp_logit_groups<WIDTH, LAYERS>(ma, g, xs);
    }
  }
  if (valid) {
    ga.total[slot] = total;
    ga.n_valid[slot] = n_valid;
  }
}

// ------------------------------------------------------------------------------------------------ partial-block layout
// One wave per chunk of ga.tiles tiles walks the (tile, distinct group) pairs in the order k_pgm_pass2 does and counts
// the partial blocks: a new one whenever the group differs from the pair before.
__global__ __launch_bounds__(64) void k_pgm_count(const MlpGradArgs ga) {
  const MlpRolloutArgs &ma = ga.m;
  const RolloutArgs &a = ma.r;
  const uint32_t w = blockIdx.x, l = threadIdx.x;
  int32_t cur = -1;
  uint32_t count = 0;
  for (int tile = 0; tile < ga.tiles; ++tile) {
    const int64_t first = ((int64_t)w * ga.tiles + tile) * 64;
    if (first >= a.n) break;
    const bool valid = first + l < a.n;
    uint32_t e = 0;
    if (valid) {
      e = a.order ? a.order[first + l] : (uint32_t)(first + l);
      e = e < (uint32_t)a.n ? e : (uint32_t)(a.n - 1);
    }
    const int32_t g = valid ? pgm_group(ma, e) : -1;
    uint64_t todo = __ballot(valid);
    while (todo) {
      const int32_t gw = __builtin_amdgcn_readfirstlane(__shfl(g, __ffsll((unsigned long long)todo) - 1));
      if (gw != cur) { ++count; cur = gw; }
      todo &= ~__ballot(g == gw);
    }
  }
  if (l == 0) ga.chunk_count[w] = count;
}

__global__ __launch_bounds__(1024) void k_pgm_scan(const MlpGradArgs ga) {
  __shared__ uint32_t s_sum[1024];
  const uint32_t nc = ga.n_chunks, seg = (nc + 1023) / 1024;
  const uint32_t lo = threadIdx.x * seg, hi = lo + seg < nc ? lo + seg : nc;
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; ++i) sum += ga.chunk_count[i];
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int i = 0; i < 1024; ++i) { const uint32_t v = s_sum[i]; s_sum[i] = run; run += v; }
    ga.chunk_base[nc] = run;
  }
  __syncthreads();
  uint32_t run = s_sum[threadIdx.x];
  for (uint32_t i = lo; i < hi; ++i) { ga.chunk_base[i] = run; run += ga.chunk_count[i]; }
}

// ------------------------------------------------------------------------------------------------ pass 2
#define PGM_XT 48  // pitch of the second copy of the input rows (16 mod 32: see the bank argument above)

template <int WIDTH>
struct PgmPitch { static constexpr int P = WIDTH == 16 ? 16 : WIDTH + 16; };

__device__ __forceinline__ float pgm_dact(float h, int activation) {
  // from the activation's value: tanh' = 1 - h^2; ReLU' = 1 where the pre-activation is positive (0 at exactly 0)
  return activation == W2A_MLP_RELU ? (h > 0.0f ? 1.0f : 0.0f) : fmaf(-h, h, 1.0f);
}

// adds `v` (this lane's element at `off` of the parameter layout) into the wave's current partial block
__device__ __forceinline__ void pgm_put(double *part, bool fresh, int off, float v) {
  part[off] = fresh ? (double)v : part[off] + (double)v;
}

// Launch bounds: one wave per workgroup, and one wave per SIMD -- the accumulators ([64, 64]: 121 registers) live next to
// the hidden tiles, the fragments in flight and the day loop's state, and VGPRs and AGPRs share one budget of 512 per
// lane at that occupancy. The compiler's figures per instantiation: DESIGN.md.
// The kernel's text is w2a_policy_gradient_mlp_pass2.inc.h, stamped out twice: here as k_pgm_pass2 with HEADS = 1, and in
// w2a_qlearn.hip.h as k_qg_pass2 with HEADS = 2 (a parameter block that ends in two output rows, the row selected per
// env-day). It is included as text and not called as a function template: an inlined call changed the register
// allocation of <32, 2> and larger, and HEADS = 1 has to stay the code it was (profiles/r23/device_code_identity.txt).
#define PGM_PASS2_KERNEL k_pgm_pass2
#define PGM_PASS2_HEADS 1
#include "w2a_policy_gradient_mlp_pass2.inc.h"
#undef PGM_PASS2_KERNEL
#undef PGM_PASS2_HEADS

// ------------------------------------------------------------------------------------------------ reduction
__global__ __launch_bounds__(256) void k_pgm_reduce(const MlpGradArgs ga) {
  __shared__ uint32_t s_first, s_last;
  const int32_t g = blockIdx.x, stride = ga.m.stride;
  const int32_t i = blockIdx.y * 256 + threadIdx.x;
  const uint32_t all = ga.chunk_base[ga.n_chunks];
  const bool fits = all <= ga.capacity;
  // the range of partial indices that holds the group's blocks (contiguous in a group-major order): every thread looks
  // at all / 256 tags once, integer min / max through LDS
  if (threadIdx.x == 0) { s_first = 0xFFFFFFFFu; s_last = 0; }
  __syncthreads();
  if (fits) {
    uint32_t first = 0xFFFFFFFFu, last = 0;
    for (uint32_t p = threadIdx.x; p < all; p += 256)
      if (ga.tag[p] == g) { first = first < p ? first : p; last = p + 1; }
    if (last) { atomicMin(&s_first, first); atomicMax(&s_last, last); }
  }
  __syncthreads();
  if (i >= stride) return;
  float out = __builtin_nanf("");  // more partial blocks than the workspace holds (no group-major order): no gradient
  if (fits) {
    double sum = 0.0;
    uint64_t cnt = 0;
    for (uint32_t p = s_first; p < s_last; ++p)
      if (ga.tag[p] == g) {
        sum += ga.partial[(size_t)p * stride + i];
        cnt += ga.pcount[p];
      }
    out = (float)(sum / (double)cnt);  // a group without envs: 0 / 0
  }
  ga.grad[(size_t)g * stride + i] = out;
}

template <int WIDTH, int LAYERS>
static void launch_pgm(const MlpGradArgs &ga, unsigned grid1, hipStream_t s) {
  if (ga.m.gate) hipLaunchKernelGGL((k_pgm_pass1<WIDTH, LAYERS, true>), dim3(grid1), dim3(BLOCK), 0, s, ga);
  else hipLaunchKernelGGL((k_pgm_pass1<WIDTH, LAYERS, false>), dim3(grid1), dim3(BLOCK), 0, s, ga);
  hipLaunchKernelGGL(k_pgm_count, dim3(ga.n_chunks), dim3(64), 0, s, ga);
  hipLaunchKernelGGL(k_pgm_scan, dim3(1), dim3(1024), 0, s, ga);
  hipLaunchKernelGGL((k_pgm_pass2<WIDTH, LAYERS>), dim3(ga.n_chunks), dim3(64), 0, s, ga);
  hipLaunchKernelGGL(k_pgm_reduce, dim3(ga.m.n_groups, (ga.m.stride + 255) / 256), dim3(256), 0, s, ga);
}

#endif  // W2A_POLICY_GRADIENT_MLP_HIP_H
