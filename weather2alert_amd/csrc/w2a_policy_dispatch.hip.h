// w2a_policy_dispatch.hip.h -- host side of the learned-policy entry points: w2a_rollout_linear / _mlp, the policy,
// imitation, surrogate and value gradients and GAE, with their _record, _gated and _weighted forms. Part of libw2a.so;
// included only by w2a_kernels.hip inside its extern "C" block. No device code lives here.
//
// Twelve bodies serve those exports, two more the Fisher-vector products (w2a_fisher_vector_product_linear / _mlp,
// which take their nullable gate directly) one w2a_q_gradient_mlp (a second, nullable parameter struct: the target net) and one w2a_actor_critic_mlp (the two-row
// net of a shared trunk; nullable gate, nullable epoch inputs). What they share is written once, in the helpers of the first half of this file:
//   check_linear_policy_struct / check_mlp_policy_struct   the checks of the policy struct (and n_steps): need no handle
//   check_handle_common      NULL handle, the schedule's word count, corrected-semantics flags, 2^31 observation offsets
//   check_mlp_stride / check_mlp_workspace                 2^31 floats of parameters; the PgmLayout workspace's size
//   check_gate, refuse_while_capturing                     the allowed-days bitmap; a stream that records a hipGraph
//   fill_rollout_common -> fill_linear / fill_mlp          the slot map and what every kernel reads of RolloutArgs
//   bind_pgm_workspace, dispatch_mlp_shape                 the MLP gradient workspace; width x layers -> instantiation
// What differs between the bodies stays written out in each: the ORDER of the helper calls (a caller sees which of two
// bad arguments is reported: tests/test_policy_entry_refusals_cpu.py), a.order, pol.seed, pol.require_budget, the
// trajectory rules, the bookkeeping call, the memsets and the launch. DESIGN.md ("Host side of the learned-policy
// entry points") has the table.
#ifndef W2A_POLICY_DISPATCH_HIP_H
#define W2A_POLICY_DISPATCH_HIP_H

#define W2A_CHECK(expr)                \
  do {                                 \
    const int rc_ = (expr);            \
    if (rc_ != W2A_OK) return rc_;     \
  } while (0)

// what W2A_Q_LAST_ROLLOUT_KERNEL reports after w2a_rollout_linear / w2a_rollout_mlp (the built-in kernels' values come
// from w2a_bookkeeping.h: bk_rollout_kernel)
#define W2A_ROLLOUT_KERNEL_LINEAR 3
#define W2A_ROLLOUT_KERNEL_MLP 4

// ---- checks that need no handle (so that they are made on any machine) ----------------------------------------------
// how an entry point reads policy->sample: a rollout, an imitation or a surrogate call takes 0 or 1; a policy gradient
// needs a stochastic policy; a value network has neither sample nor require_budget (both ignored) and is called "value"
enum SampleRule { SAMPLE_0_OR_1, SAMPLE_MUST_BE_1, SAMPLE_IGNORED };

static int check_sample_rule(const char *fn, int32_t sample, int32_t require_budget, SampleRule rule) {
  if (rule == SAMPLE_IGNORED) return W2A_OK;
  if (rule == SAMPLE_MUST_BE_1 && sample != 1)
    return fail(W2A_ERR_ARG, "%s: sample must be 1 (a deterministic policy has no score function)", fn);
  if (sample != 0 && sample != 1) return fail(W2A_ERR_ARG, "%s: sample must be 0 or 1", fn);
  if (require_budget != 0 && require_budget != 1) return fail(W2A_ERR_ARG, "%s: require_budget must be 0 or 1", fn);
  return W2A_OK;
}

static int check_linear_policy_struct(const char *fn, const w2a_linear_policy *p, int32_t n_steps, SampleRule rule) {
  if (!p) return fail(W2A_ERR_ARG, rule == SAMPLE_IGNORED ? "%s: NULL value" : "%s: NULL policy", fn);
  if (n_steps <= 0) return fail(W2A_ERR_ARG, "%s: n_steps must be positive", fn);
  if (!p->weight || !p->bias) return fail(W2A_ERR_ARG, "%s: NULL weight or bias", fn);
  if (p->n_groups <= 0) return fail(W2A_ERR_ARG, "%s: n_groups must be positive", fn);
  W2A_CHECK(check_sample_rule(fn, p->sample, p->require_budget, rule));
  if ((uintptr_t)p->weight & 15) return fail(W2A_ERR_ARG, "%s: weight must be 16-B aligned", fn);
  return W2A_OK;
}

static int check_mlp_policy_struct(const char *fn, const w2a_mlp_policy *p, int32_t n_steps, SampleRule rule) {
  if (!p) return fail(W2A_ERR_ARG, rule == SAMPLE_IGNORED ? "%s: NULL value" : "%s: NULL policy", fn);
  if (n_steps <= 0) return fail(W2A_ERR_ARG, "%s: n_steps must be positive", fn);
  if (!p->params) return fail(W2A_ERR_ARG, "%s: NULL params", fn);
  if (p->n_groups <= 0) return fail(W2A_ERR_ARG, "%s: n_groups must be positive", fn);
  if (p->n_layers != 1 && p->n_layers != 2) return fail(W2A_ERR_ARG, "%s: n_layers must be 1 or 2", fn);
  if (p->width != 16 && p->width != 32 && p->width != 64) return fail(W2A_ERR_ARG, "%s: width must be 16, 32 or 64", fn);
  if (p->activation != W2A_MLP_TANH && p->activation != W2A_MLP_RELU)
    return fail(W2A_ERR_ARG, "%s: activation must be W2A_MLP_TANH or W2A_MLP_RELU", fn);
  W2A_CHECK(check_sample_rule(fn, p->sample, p->require_budget, rule));
  if ((uintptr_t)p->params & 15) return fail(W2A_ERR_ARG, "%s: params must be 16-B aligned", fn);
  return W2A_OK;
}

static int check_obs(const char *fn, const float *obs) {
  if (!obs) return fail(W2A_ERR_ARG, "%s: NULL obs (the rows the agent holds are the first day's input)", fn);
  return W2A_OK;
}

static int check_workspace_pointer(const char *fn, const void *workspace) {
  if (!workspace) return fail(W2A_ERR_ARG, "%s: NULL workspace", fn);
  if ((uintptr_t)workspace & 255) return fail(W2A_ERR_ARG, "%s: workspace must be 256-B aligned", fn);
  return W2A_OK;
}

// the host-side checks of a trajectory (w2a_rollout_linear_record, w2a_rollout_mlp_record): before anything else
static int check_trajectory(const w2a_trajectory *traj, const char *fn) {
  if (!traj) return fail(W2A_ERR_ARG, "%s: NULL trajectory", fn);
  if (!traj->obs || !traj->logit || !traj->reward || !traj->action || !traj->flags)
    return fail(W2A_ERR_ARG, "%s: NULL trajectory array", fn);
  return W2A_OK;
}

// the checks w2a_imitation_gradient_linear and _mlp share once the policy's own have passed (same order in both)
static int check_imitation(const char *fn, const uint32_t *alert_mask, const float *obs, const void *grad,
                           const float *loglik, const int32_t *days) {
  if (!alert_mask) return fail(W2A_ERR_ARG, "%s: NULL alert_mask (the schedule to score)", fn);
  W2A_CHECK(check_obs(fn, obs));
  if (!grad || !loglik || !days) return fail(W2A_ERR_ARG, "%s: NULL grad, loglik or days", fn);
  return W2A_OK;
}

static int check_day_weight(const char *fn, const float *day_weight, int32_t day_weight_days, int32_t n_steps) {
  if (day_weight && day_weight_days < n_steps)
    return fail(W2A_ERR_ARG, "%s: day_weight holds fewer call-days than n_steps", fn);
  return W2A_OK;
}

// the checks w2a_surrogate_gradient_linear and _mlp share once the policy's own have passed (same order in both)
static int check_surrogate_outputs(const char *fn, const uint32_t *alert_mask, const float *obs, const void *grad,
                                   const float *surrogate, const int32_t *clipped_days, const float *approx_kl,
                                   const float *entropy, const int32_t *days) {
  if (!alert_mask) return fail(W2A_ERR_ARG, "%s: NULL alert_mask (the schedule to score)", fn);
  W2A_CHECK(check_obs(fn, obs));
  if (!grad || !surrogate || !clipped_days || !approx_kl || !entropy || !days)
    return fail(W2A_ERR_ARG, "%s: NULL grad, surrogate, clipped_days, approx_kl, entropy or days", fn);
  return W2A_OK;
}

// ... and what the surrogate adds to the weighted imitation calls' checks, where they check day_weight_days
static int check_surrogate_inputs(const char *fn, const float *advantage, int32_t advantage_days,
                                  const float *old_log_prob, int32_t old_log_prob_days, double clip,
                                  double entropy_coef, int32_t n_steps) {
  if (!advantage) return fail(W2A_ERR_ARG, "%s: NULL advantage", fn);
  if (advantage_days < n_steps) return fail(W2A_ERR_ARG, "%s: advantage holds fewer call-days than n_steps", fn);
  if (old_log_prob && old_log_prob_days < n_steps)
    return fail(W2A_ERR_ARG, "%s: old_log_prob holds fewer call-days than n_steps", fn);
  if (!isfinite(clip) || clip < 0.0) return fail(W2A_ERR_ARG, "%s: clip must be finite and not negative", fn);
  if (!isfinite(entropy_coef)) return fail(W2A_ERR_ARG, "%s: entropy_coef must be finite", fn);
  return W2A_OK;
}

// the checks the four value calls share once the network's own have passed (same order in all)
static int check_value(const char *fn, const uint32_t *alert_mask, const float *obs, const void *grad,
                       const float *sq_error, const int32_t *days, const float *ret) {
  if (!alert_mask) return fail(W2A_ERR_ARG, "%s: NULL alert_mask (the schedule to follow)", fn);
  W2A_CHECK(check_obs(fn, obs));
  if (!grad || !sq_error || !days || !ret) return fail(W2A_ERR_ARG, "%s: NULL grad, sq_error, days or ret", fn);
  return W2A_OK;
}

// what w2a_value_gradient_linear_gae and _mlp_gae check beyond check_value (same order in both)
static int check_gae(const char *fn, double gamma, double lambda, int32_t bootstrap, const float *advantage,
                     const float *value_target, const float *target, int32_t target_days, int32_t n_steps) {
  if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(W2A_ERR_ARG, "%s: gamma must lie in [0, 1]", fn);
  if (!(lambda >= 0.0 && lambda <= 1.0)) return fail(W2A_ERR_ARG, "%s: lambda must lie in [0, 1]", fn);
  if (bootstrap != 0 && bootstrap != 1) return fail(W2A_ERR_ARG, "%s: bootstrap must be 0 or 1", fn);
  if (target) {
    if (target_days < n_steps) return fail(W2A_ERR_ARG, "%s: target holds fewer call-days than n_steps", fn);
    if (advantage || value_target)
      return fail(W2A_ERR_ARG, "%s: advantage and value_target are not formed when target is given", fn);
    if (gamma != 1.0 || lambda != 1.0 || bootstrap)
      return fail(W2A_ERR_ARG, "%s: gamma, lambda and bootstrap have no meaning when target is given", fn);
  }
  return W2A_OK;
}

// ---- checks that read the handle -------------------------------------------------------------------------------------
// which bitmaps of ceil(T/32) words per env the call takes: none (the policy gradients), the schedule to follow, or the
// two a rollout writes (checked when either is wanted)
enum MaskRule { MASK_NONE, MASK_SCHEDULE, MASK_ROLLOUT };
// what the corrected-semantics flags would change for the call: the value calls also form returns from the rewards
enum FixesChange { FIXES_CHANGE_OBS, FIXES_CHANGE_OBS_AND_REWARD };

// every body's first look at the handle, in the one order all twelve had: NULL, the bitmap's width, the flags, the
// offsets. mask_words is widened before the product (the two rollout bodies used to multiply in 32 bits, which agrees
// for every mask_words below 2^26).
static int check_handle_common(const char *fn, const w2a_env *env, FixesChange what_changes, MaskRule masks,
                               int32_t mask_words) {
  if (!env) return fail(W2A_ERR_ARG, "%s: NULL handle", fn);
  if (masks != MASK_NONE && (int64_t)mask_words * 32 < env->tb.T)
    return fail(W2A_ERR_ARG, masks == MASK_ROLLOUT ? "%s: alert_mask / attempt_mask need ceil(T/32) words per env"
                                                   : "%s: alert_mask needs ceil(T/32) words per env", fn);
  if (env->tb.fixes)
    return fail(W2A_ERR_ARG, what_changes == FIXES_CHANGE_OBS
                                 ? "%s: not available with corrected-semantics flags (they change what the observation is)"
                                 : "%s: not available with corrected-semantics flags (they change what the observation "
                                   "and the reward are)", fn);
  if (env->n * (int64_t)env->tb.n_obs >= (1ll << 31))
    return fail(W2A_ERR_ARG, "%s: num_envs * n_obs must stay below 2^31 (32-bit observation offsets)", fn);
  return W2A_OK;
}

static int check_mlp_stride(const char *fn, const w2a_mlp_policy *p) {
  if ((int64_t)p->n_groups * W2A_MLP_STRIDE((int64_t)p->width, p->n_layers) >= (1ll << 31))
    return fail(W2A_ERR_ARG, "%s: n_groups * block size must stay below 2^31 floats", fn);
  return W2A_OK;
}

// the allowed-days bitmap of the *_gated entry points: checked where the schedule's bitmap is. In the bodies below,
// gated: the call came through a _gated export (the gate is then checked, after the workspace's size, and the GATE
// instantiations run); every other export passes a NULL gate of 0 words.
static int check_gate(const char *fn, const w2a_env *env, const uint32_t *gate, int32_t gate_words) {
  if (!gate) return fail(W2A_ERR_ARG, "%s: NULL allowed_days (the entry point without _gated takes no gate)", fn);
  if ((int64_t)gate_words * 32 < env->tb.T) return fail(W2A_ERR_ARG, "%s: allowed_days needs ceil(T/32) words per env", fn);
  return W2A_OK;
}

// the lookahead block of the w2a_lookahead_* entry points: checked after the gate. needs_weight: the linear kind's rows
// (the MLP kind keeps its lookahead rows at the tail of every parameter block)
static int check_lookahead(const char *fn, const w2a_env *env, const w2a_lookahead *look, bool needs_weight) {
  if (!look || !look->series) return fail(W2A_ERR_ARG, "%s: NULL lookahead or series", fn);
  if (look->days < 1 || look->days > W2A_LOOKAHEAD_MAX_DAYS)
    return fail(W2A_ERR_ARG, "%s: lookahead days must lie in 1..W2A_LOOKAHEAD_MAX_DAYS", fn);
  if (look->stride < env->tb.T) return fail(W2A_ERR_ARG, "%s: lookahead stride must be at least T", fn);
  if (needs_weight && !look->weight) return fail(W2A_ERR_ARG, "%s: NULL lookahead weight", fn);
  return W2A_OK;
}

static void fill_lookahead(const w2a_lookahead *look, LookArgs &lk) {
  lk.series = look->series; lk.stride = look->stride; lk.days = look->days; lk.weight = look->weight;
}

// the forecast-error block of the w2a_forecast_* entry points: checked after the lookahead block
static int check_forecast_error(const char *fn, const w2a_lookahead *look, const w2a_forecast_error *err) {
  if (!err) return fail(W2A_ERR_ARG, "%s: NULL forecast error", fn);
  for (int k = 0; k < look->days; ++k)
    if (!isfinite(err->mae[k]) || err->mae[k] < 0.0f)
      return fail(W2A_ERR_ARG, "%s: forecast error mae must be finite and non-negative", fn);
  return W2A_OK;
}

// entries past `days` are never read by the kernels; they are passed as zeros
static void fill_forecast_error(const w2a_lookahead *look, const w2a_forecast_error *err, LookArgs &lk) {
  lk.err_seed = err->seed;
  for (int k = 0; k < W2A_LOOK_PAD; ++k) lk.mae[k] = k < look->days ? err->mae[k] : 0.0f;
}

// REFUSE_WHILE_CAPTURING with the name at run time: every body's last refusal
static int refuse_while_capturing(const char *fn, void *stream) {
  if (stream_is_capturing((hipStream_t)stream))
    return fail(W2A_ERR_STATE, "%s: the stream is recording a hipGraph; only w2a_step can be recorded (episode "
                               "boundaries inside a graph: W2A_STEP_AUTORESET)", fn);
  return W2A_OK;
}

// ---- kernel arguments ------------------------------------------------------------------------------------------------
// The slot map, and the fields of RolloutArgs every kernel of this file reads. Every observation column must sit on a
// slot the day loop multiplies (0..RO64_SLOTS-1): then slot 31, which carries the bias, is provably none of them.
// The caller has zeroed the struct; a.order, a.pol and the outputs of a rollout are the caller's to set.
static int fill_rollout_common(const char *fn, const w2a_env *env, int32_t n_steps, RolloutArgs &a, int8_t *slot_obs,
                               uint32_t &obs_mask) {
  obs_mask = 0;
  for (int k = 0; k < RO64_SLOTS; ++k) slot_obs[k] = -1;
  for (int j = 0; j < env->tb.n_obs; ++j) {
    const int sl = env->obs_slot_host[j];
    if (sl < 0 || sl >= RO64_SLOTS)
      return fail(W2A_ERR_SCHEMA, "%s: an observation column sits on slot 30 or 31 of the feature row", fn);
    obs_mask |= 1u << sl;
    slot_obs[sl] = (int8_t)j;
  }
  a.tb = env->tb; a.st = env->st; a.status = env->status; a.n = env->n; a.gid0 = env->gid0;
  a.n_steps = n_steps;
  return W2A_OK;
}

// obs: only the two rollouts write it
static int fill_linear(const char *fn, const w2a_env *env, const w2a_linear_policy *p, int32_t n_steps, const float *obs,
                       const uint32_t *gate, int32_t gate_words, LinearRolloutArgs &la) {
  W2A_CHECK(fill_rollout_common(fn, env, n_steps, la.r, la.slot_obs, la.obs_mask));
  la.gate = gate;
  la.gate_words = gate_words;
  la.weight = reinterpret_cast<const float4 *>(p->weight);
  la.bias = p->bias;
  la.group = p->group;
  la.n_groups = p->n_groups;
  la.n_obs = env->tb.n_obs;
  la.obs = const_cast<float *>(obs);
  return W2A_OK;
}

static int fill_mlp(const char *fn, const w2a_env *env, const w2a_mlp_policy *p, int32_t n_steps, const float *obs,
                    const uint32_t *gate, int32_t gate_words, MlpRolloutArgs &ma) {
  W2A_CHECK(fill_rollout_common(fn, env, n_steps, ma.r, ma.slot_obs, ma.obs_mask));
  ma.gate = gate;
  ma.gate_words = gate_words;
  ma.params = p->params;
  ma.group = p->group;
  ma.n_groups = p->n_groups;
  ma.stride = (int32_t)W2A_MLP_STRIDE((int64_t)p->width, p->n_layers);  // below 2^31: check_mlp_stride
  ma.activation = p->activation;
  ma.n_obs = env->tb.n_obs;
  ma.obs = const_cast<float *>(obs);
  return W2A_OK;
}

// the visiting order of the MLP gradient kernels: they write no state, so it is their own -- the policy's (group-major,
// so that the partial blocks fit the workspace) or identity, never the handle's feature-row order
static const uint32_t *mlp_own_order(const w2a_mlp_policy *p) { return reinterpret_cast<const uint32_t *>(p->order); }

static void fill_imitation(ImitationArgs &im, const uint32_t *alert_mask, int32_t mask_words, const float *env_weight,
                           const float *day_weight, float *loglik, int32_t *days) {
  im.alert_mask = alert_mask; im.mask_words = mask_words; im.env_weight = env_weight;
  im.day_weight = day_weight;
  im.loglik = loglik; im.days = days;
}

static void fill_surrogate(SurrogateArgs &sg, const uint32_t *alert_mask, int32_t mask_words, const float *env_weight,
                           const float *advantage, const float *old_log_prob, double clip, double entropy_coef,
                           float *log_prob, float *surrogate, int32_t *clipped_days, float *approx_kl, float *entropy,
                           int32_t *days) {
  sg.alert_mask = alert_mask; sg.mask_words = mask_words; sg.env_weight = env_weight;
  sg.advantage = advantage; sg.old_log_prob = old_log_prob;
  sg.lo = 1.0 - clip; sg.hi = 1.0 + clip; sg.beta = entropy_coef;
  sg.log_prob = log_prob; sg.surrogate = surrogate; sg.clipped = clipped_days; sg.approx_kl = approx_kl;
  sg.entropy = entropy; sg.days = days;
}

static void fill_value(ValueArgs &v, const uint32_t *alert_mask, int32_t mask_words, const float *env_weight,
                       float *sq_error, int32_t *days, float *ret, float *advantage) {
  v.alert_mask = alert_mask; v.mask_words = mask_words; v.env_weight = env_weight;
  v.sq_error = sq_error; v.days = days; v.ret = ret; v.advantage = advantage;
}

static void fill_gae(GaeArgs &g, double gamma, double lambda, int32_t bootstrap, float *value_target, const float *target) {
  g.gamma = gamma; g.gl = gamma * lambda; g.bootstrap = bootstrap;
  g.value_target = value_target; g.target = target;
}

// 64 envs per wave, whole groups of 8 workgroups (one per XCD)
static unsigned grid64(const w2a_env *env) { return (unsigned)((((env->n + BLOCK - 1) / BLOCK) + 7) / 8 * 8); }

// zeroes the flags of every (call-day, env) the kernel writes: entries of envs that take no step keep 0
static int clear_trajectory_flags(const w2a_env *env, int32_t n_steps, const w2a_trajectory *traj, hipStream_t s) {
  HIP_TRY(hipMemsetAsync(traj->flags, 0, (size_t)n_steps * (size_t)env->n, s));
  return W2A_OK;
}

// zeroes a [n_steps][n] f32 output whose rows of days not stepped stay 0 (nullable)
static int clear_day_rows(const w2a_env *env, int32_t n_steps, float *rows, hipStream_t s) {
  if (rows) HIP_TRY(hipMemsetAsync(rows, 0, sizeof(float) * (size_t)env->n * (size_t)n_steps, s));
  return W2A_OK;
}

// ---- the workspace of the MLP gradient calls -------------------------------------------------------------------------
// pass 1's scratch (9 B per env-day, 12 B per env) and the partial blocks (fp64 [stride] each) of pass 2's waves: laid
// out for w2a_policy_gradient_mlp; the imitation, surrogate, value and GAE calls run the same second pass on it
struct PgmLayout {
  int32_t tiles;      // 64-env tiles per wave of pass 2
  uint32_t n_chunks;  // its waves
  uint32_t capacity;  // partial blocks: one per wave and one per group boundary of a group-major order
  size_t day, day_alert, total, n_valid, chunk_count, chunk_base, tag, pcount, partial, bytes;
};
#define PGM_TARGET_WAVES 1024  // one wave per SIMD of the device
#define PGM_MAX_TILES 16

// heads: 1, or 2 for the two-head blocks of w2a_q_gradient_mlp (the partial blocks then have that layout's stride)
static PgmLayout pgm_layout(int64_t n, int32_t n_steps, int32_t n_groups, int32_t width, int32_t n_layers,
                            int32_t heads = 1) {
  PgmLayout L;
  const int64_t n_tiles = (n + 63) / 64;
  int64_t tiles = (n_tiles + PGM_TARGET_WAVES - 1) / PGM_TARGET_WAVES;
  tiles = tiles < 1 ? 1 : (tiles > PGM_MAX_TILES ? PGM_MAX_TILES : tiles);
  L.tiles = (int32_t)tiles;
  L.n_chunks = (uint32_t)((n_tiles + tiles - 1) / tiles);
  const int64_t groups = (int64_t)n_groups < n ? (int64_t)n_groups : n;
  L.capacity = (uint32_t)(L.n_chunks + groups);
  const size_t days = (size_t)n * (size_t)n_steps;
  const size_t stride = heads == 2 ? (size_t)W2A_MLP_HEADS_STRIDE((int64_t)width, n_layers)
                                   : (size_t)W2A_MLP_STRIDE((int64_t)width, n_layers);
  size_t off = 0;
  L.day = off; off += align256(sizeof(float2) * days);
  L.day_alert = off; off += align256(days);
  L.total = off; off += align256(sizeof(double) * (size_t)n);
  L.n_valid = off; off += align256(sizeof(int32_t) * (size_t)n);
  L.chunk_count = off; off += align256(sizeof(uint32_t) * L.n_chunks);
  L.chunk_base = off; off += align256(sizeof(uint32_t) * ((size_t)L.n_chunks + 1));
  L.tag = off; off += align256(sizeof(int32_t) * (size_t)L.capacity);
  L.pcount = off; off += align256(sizeof(uint32_t) * (size_t)L.capacity);
  L.partial = off; off += align256(sizeof(double) * (size_t)L.capacity * stride);
  L.bytes = off;
  return L;
}

// after the handle's own checks: the parameter block's size, then the workspace's (too_small: the call's own text)
static int check_mlp_workspace(const char *fn, const w2a_env *env, const w2a_mlp_policy *p, int32_t n_steps,
                               size_t workspace_bytes, const char *too_small, PgmLayout &L) {
  W2A_CHECK(check_mlp_stride(fn, p));
  L = pgm_layout(env->n, n_steps, p->n_groups, p->width, p->n_layers);
  if (workspace_bytes < L.bytes) return fail(W2A_ERR_ARG, too_small, fn);
  return W2A_OK;
}

static void bind_pgm_workspace(MlpGradArgs &ga, const PgmLayout &L, void *workspace, float *grad) {
  char *ws = reinterpret_cast<char *>(workspace);
  ga.day = reinterpret_cast<float2 *>(ws + L.day);
  ga.day_alert = reinterpret_cast<uint8_t *>(ws + L.day_alert);
  ga.total = reinterpret_cast<double *>(ws + L.total);
  ga.n_valid = reinterpret_cast<int32_t *>(ws + L.n_valid);
  ga.tiles = L.tiles;
  ga.n_chunks = L.n_chunks;
  ga.chunk_count = reinterpret_cast<uint32_t *>(ws + L.chunk_count);
  ga.chunk_base = reinterpret_cast<uint32_t *>(ws + L.chunk_base);
  ga.capacity = L.capacity;
  ga.tag = reinterpret_cast<int32_t *>(ws + L.tag);
  ga.pcount = reinterpret_cast<uint32_t *>(ws + L.pcount);
  ga.partial = reinterpret_cast<double *>(ws + L.partial);
  ga.grad = grad;
}

// f(width, layers) with both as std::integral_constant<int, ..>: the one place that turns a checked (width, n_layers)
// into template arguments. check_mlp_policy_struct has passed, so the default is 64 x 2.
extern "C++" {
template <class F>
static void dispatch_mlp_shape(int32_t width, int32_t n_layers, F &&f) {
  using std::integral_constant;
  switch (width * 4 + n_layers) {
    case 16 * 4 + 1: f(integral_constant<int, 16>{}, integral_constant<int, 1>{}); break;
    case 16 * 4 + 2: f(integral_constant<int, 16>{}, integral_constant<int, 2>{}); break;
    case 32 * 4 + 1: f(integral_constant<int, 32>{}, integral_constant<int, 1>{}); break;
    case 32 * 4 + 2: f(integral_constant<int, 32>{}, integral_constant<int, 2>{}); break;
    case 64 * 4 + 1: f(integral_constant<int, 64>{}, integral_constant<int, 1>{}); break;
    default: f(integral_constant<int, 64>{}, integral_constant<int, 2>{}); break;
  }
}
}  // extern "C++"

// ---- workspace sizes (exported) --------------------------------------------------------------------------------------
// scratch of w2a_policy_gradient_linear: (delta_s, A_s) and the alert issued, per (call-day, env)
size_t w2a_policy_gradient_workspace_bytes(int64_t num_envs, int32_t n_steps) {
  if (num_envs <= 0 || n_steps <= 0) return 0;
  const size_t days = (size_t)num_envs * (size_t)n_steps;
  return align256(sizeof(float2) * days) + align256(days);
}

size_t w2a_policy_gradient_mlp_workspace_bytes(int64_t num_envs, int32_t n_steps, int32_t n_groups, int32_t width,
                                               int32_t n_layers) {
  if (num_envs <= 0 || n_steps <= 0 || n_groups <= 0) return 0;
  if ((width != 16 && width != 32 && width != 64) || (n_layers != 1 && n_layers != 2)) return 0;
  return pgm_layout(num_envs, n_steps, n_groups, width, n_layers).bytes;
}

// the workspace of w2a_policy_gradient_mlp: the same scratch and partial blocks serve the same second pass
size_t w2a_imitation_gradient_mlp_workspace_bytes(int64_t num_envs, int32_t n_steps, int32_t n_groups, int32_t width,
                                                  int32_t n_layers) {
  return w2a_policy_gradient_mlp_workspace_bytes(num_envs, n_steps, n_groups, width, n_layers);
}
size_t w2a_surrogate_gradient_mlp_workspace_bytes(int64_t num_envs, int32_t n_steps, int32_t n_groups, int32_t width,
                                                  int32_t n_layers) {
  return w2a_imitation_gradient_mlp_workspace_bytes(num_envs, n_steps, n_groups, width, n_layers);
}
size_t w2a_value_gradient_mlp_workspace_bytes(int64_t num_envs, int32_t n_steps, int32_t n_groups, int32_t width,
                                              int32_t n_layers) {
  return w2a_policy_gradient_mlp_workspace_bytes(num_envs, n_steps, n_groups, width, n_layers);
}
size_t w2a_value_gradient_mlp_gae_workspace_bytes(int64_t num_envs, int32_t n_steps, int32_t n_groups, int32_t width,
                                                  int32_t n_layers) {
  return w2a_policy_gradient_mlp_workspace_bytes(num_envs, n_steps, n_groups, width, n_layers);
}

// w2a_q_gradient_mlp: the layout of w2a_value_gradient_mlp with the partial blocks at the two-head stride
size_t w2a_q_gradient_mlp_workspace_bytes(int64_t num_envs, int32_t n_steps, int32_t n_groups, int32_t width,
                                          int32_t n_layers) {
  if (num_envs <= 0 || n_steps <= 0 || n_groups <= 0) return 0;
  if ((width != 16 && width != 32 && width != 64) || (n_layers != 1 && n_layers != 2)) return 0;
  return pgm_layout(num_envs, n_steps, n_groups, width, n_layers, 2).bytes;
}

// scratch of w2a_value_gradient_linear: y_s (fp64) and the alert issued, per (call-day, env) -- 9 B, as the policy gradient's
size_t w2a_value_gradient_linear_workspace_bytes(int64_t num_envs, int32_t n_steps) {
  return w2a_policy_gradient_workspace_bytes(num_envs, n_steps);
}

// scratch of w2a_value_gradient_linear_gae: delta_s / c_s and V_s (fp64) and the alert issued, per (call-day, env) -- 17 B
size_t w2a_value_gradient_linear_gae_workspace_bytes(int64_t num_envs, int32_t n_steps) {
  if (num_envs <= 0 || n_steps <= 0) return 0;
  const size_t days = (size_t)num_envs * (size_t)n_steps;
  return 2 * align256(sizeof(double) * days) + align256(days);
}

// ---- rollouts --------------------------------------------------------------------------------------------------------
static void set_rollout_outputs(RolloutArgs &a, float *ret_out, int32_t *alerts_out, int32_t *attempts_over_budget,
                                uint32_t *alert_mask, uint32_t *attempt_mask, int32_t mask_words, float *last_return,
                                float *ret_snapshot) {
  a.ret_out = ret_out; a.alerts_out = alerts_out; a.attempts_over_budget = attempts_over_budget;
  a.alert_mask = alert_mask; a.attempt_mask = attempt_mask; a.mask_words = mask_words; a.last_return = last_return;
  a.ret_snapshot = ret_snapshot;
}

// the lock-step bookkeeping of w2a_rollout, what W2A_Q_LAST_ROLLOUT_KERNEL then reports, and the two bitmaps zeroed
static int begin_policy_rollout(w2a_env *env, int32_t n_steps, int kernel, uint32_t *alert_mask, uint32_t *attempt_mask,
                                int32_t mask_words, hipStream_t s) {
  HipDev dv{env, s};
  (void)bk_rollout_begin(env->bk, dv, n_steps);
  env->bk.last_rollout_kernel = kernel;
  if (alert_mask) HIP_TRY(hipMemsetAsync(alert_mask, 0, (size_t)env->n * mask_words * sizeof(uint32_t), s));
  if (attempt_mask) HIP_TRY(hipMemsetAsync(attempt_mask, 0, (size_t)env->n * mask_words * sizeof(uint32_t), s));
  return W2A_OK;
}

static int rollout_linear(const char *fn, w2a_env *env, const w2a_linear_policy *policy, int32_t n_steps, float *obs, float *ret_out,
                          int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask,
                          uint32_t *attempt_mask, int32_t mask_words, float *last_return, float *ret_snapshot,
                          void *stream, const w2a_trajectory *traj, bool gated = false, const uint32_t *gate = nullptr,
                          int32_t gate_words = 0, bool looking = false, const w2a_lookahead *look = nullptr,
                          bool noisy = false, const w2a_forecast_error *ferr = nullptr) {
  W2A_CHECK(check_linear_policy_struct(fn, policy, n_steps, SAMPLE_0_OR_1));
  W2A_CHECK(check_obs(fn, obs));
  W2A_CHECK(check_handle_common(fn, env, FIXES_CHANGE_OBS, (alert_mask || attempt_mask) ? MASK_ROLLOUT : MASK_NONE, mask_words));
  if (gated) W2A_CHECK(check_gate(fn, env, gate, gate_words));
  if (looking) W2A_CHECK(check_lookahead(fn, env, look, true));
  if (noisy) W2A_CHECK(check_forecast_error(fn, look, ferr));
  W2A_CHECK(refuse_while_capturing(fn, stream));
  LinearRolloutArgs la;
  memset(&la, 0, sizeof(la));
  W2A_CHECK(fill_linear(fn, env, policy, n_steps, obs, gate, gate_words, la));
  if (looking) fill_lookahead(look, la.look);
  if (noisy) fill_forecast_error(look, ferr, la.look);
  la.r.pol.require_budget = policy->require_budget;
  la.r.pol.seed = policy->seed;
  la.r.order = env->order;
  set_rollout_outputs(la.r, ret_out, alerts_out, attempts_over_budget, alert_mask, attempt_mask, mask_words, last_return, ret_snapshot);
  hipStream_t s = (hipStream_t)stream;
  W2A_CHECK(begin_policy_rollout(env, n_steps, W2A_ROLLOUT_KERNEL_LINEAR, alert_mask, attempt_mask, mask_words, s));
  const unsigned g64 = grid64(env);
  const bool masks = alert_mask || attempt_mask || ret_snapshot;
  w2a_trajectory tr;
  memset(&tr, 0, sizeof(tr));
  if (traj) {
    tr = *traj;
    la.r.order = nullptr;  // identity order: the kernel's staged store design (every env's result is order-independent)
    W2A_CHECK(clear_trajectory_flags(env, n_steps, traj, s));
  }
#define W2A_LAUNCH_LINEAR(M, S, R)                                                                        \
  do {                                                                                                    \
    if (gated) hipLaunchKernelGGL((k_rollout_linear<M, S, R, true>), dim3(g64), dim3(BLOCK), 0, s, la, tr); \
    else hipLaunchKernelGGL((k_rollout_linear<M, S, R, false>), dim3(g64), dim3(BLOCK), 0, s, la, tr);      \
  } while (0)
#define W2A_LAUNCH_LINEAR_LOOK(M, S)                                                                                \
  do {                                                                                                              \
    if (gated) hipLaunchKernelGGL((k_rollout_linear<M, S, false, true, true>), dim3(g64), dim3(BLOCK), 0, s, la, tr); \
    else hipLaunchKernelGGL((k_rollout_linear<M, S, false, false, true>), dim3(g64), dim3(BLOCK), 0, s, la, tr);      \
  } while (0)
#define W2A_LAUNCH_LINEAR_NOISE(M, S)                                                                                     \
  do {                                                                                                                    \
    if (gated) hipLaunchKernelGGL((k_rollout_linear<M, S, false, true, true, true>), dim3(g64), dim3(BLOCK), 0, s, la, tr); \
    else hipLaunchKernelGGL((k_rollout_linear<M, S, false, false, true, true>), dim3(g64), dim3(BLOCK), 0, s, la, tr);      \
  } while (0)
  if (noisy) {  // w2a_forecast_rollout_linear
    if (masks && policy->sample) W2A_LAUNCH_LINEAR_NOISE(true, true);
    else if (masks) W2A_LAUNCH_LINEAR_NOISE(true, false);
    else if (policy->sample) W2A_LAUNCH_LINEAR_NOISE(false, true);
    else W2A_LAUNCH_LINEAR_NOISE(false, false);
  } else if (looking) {  // no trajectory: the w2a_lookahead_* exports take none
    if (masks && policy->sample) W2A_LAUNCH_LINEAR_LOOK(true, true);
    else if (masks) W2A_LAUNCH_LINEAR_LOOK(true, false);
    else if (policy->sample) W2A_LAUNCH_LINEAR_LOOK(false, true);
    else W2A_LAUNCH_LINEAR_LOOK(false, false);
  } else if (traj) {
    if (masks && policy->sample) W2A_LAUNCH_LINEAR(true, true, true);
    else if (masks) W2A_LAUNCH_LINEAR(true, false, true);
    else if (policy->sample) W2A_LAUNCH_LINEAR(false, true, true);
    else W2A_LAUNCH_LINEAR(false, false, true);
  } else {
    if (masks && policy->sample) W2A_LAUNCH_LINEAR(true, true, false);
    else if (masks) W2A_LAUNCH_LINEAR(true, false, false);
    else if (policy->sample) W2A_LAUNCH_LINEAR(false, true, false);
    else W2A_LAUNCH_LINEAR(false, false, false);
  }
#undef W2A_LAUNCH_LINEAR
#undef W2A_LAUNCH_LINEAR_LOOK
#undef W2A_LAUNCH_LINEAR_NOISE
  HIP_TRY(hipGetLastError());
  end_call(env, s);
  return W2A_OK;
}

int w2a_rollout_linear(w2a_env *env, const w2a_linear_policy *policy, int32_t n_steps, float *obs, float *ret_out,
                       int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask, uint32_t *attempt_mask,
                       int32_t mask_words, float *last_return, float *ret_snapshot, void *stream) {
  return rollout_linear("w2a_rollout_linear", env, policy, n_steps, obs, ret_out, alerts_out, attempts_over_budget, alert_mask, attempt_mask,
                        mask_words, last_return, ret_snapshot, stream, nullptr);
}

int w2a_rollout_linear_record(w2a_env *env, const w2a_linear_policy *policy, int32_t n_steps, float *obs,
                              float *ret_out, int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask,
                              uint32_t *attempt_mask, int32_t mask_words, float *last_return, float *ret_snapshot,
                              void *stream, const w2a_trajectory *traj) {
  W2A_CHECK(check_trajectory(traj, "w2a_rollout_linear_record"));
  return rollout_linear("w2a_rollout_linear_record", env, policy, n_steps, obs, ret_out, alerts_out, attempts_over_budget, alert_mask, attempt_mask,
                        mask_words, last_return, ret_snapshot, stream, traj);
}

int w2a_rollout_linear_gated(w2a_env *env, const w2a_linear_policy *policy, int32_t n_steps, float *obs, float *ret_out,
                             int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask,
                             uint32_t *attempt_mask, int32_t mask_words, float *last_return, float *ret_snapshot,
                             void *stream, const w2a_trajectory *traj, const uint32_t *allowed_days,
                             int32_t allowed_words) {
  if (traj) W2A_CHECK(check_trajectory(traj, "w2a_rollout_linear_gated"));
  return rollout_linear("w2a_rollout_linear_gated", env, policy, n_steps, obs, ret_out, alerts_out, attempts_over_budget, alert_mask, attempt_mask,
                        mask_words, last_return, ret_snapshot, stream, traj, true, allowed_days, allowed_words);
}

int w2a_lookahead_rollout_linear(w2a_env *env, const w2a_linear_policy *policy, int32_t n_steps, float *obs,
                                 float *ret_out, int32_t *alerts_out, int32_t *attempts_over_budget,
                                 uint32_t *alert_mask, uint32_t *attempt_mask, int32_t mask_words, float *last_return,
                                 float *ret_snapshot, void *stream, const w2a_lookahead *lookahead) {
  return rollout_linear("w2a_lookahead_rollout_linear", env, policy, n_steps, obs, ret_out, alerts_out, attempts_over_budget, alert_mask,
                        attempt_mask, mask_words, last_return, ret_snapshot, stream, nullptr, false, nullptr, 0, true, lookahead);
}

int w2a_lookahead_rollout_linear_gated(w2a_env *env, const w2a_linear_policy *policy, int32_t n_steps, float *obs,
                                       float *ret_out, int32_t *alerts_out, int32_t *attempts_over_budget,
                                       uint32_t *alert_mask, uint32_t *attempt_mask, int32_t mask_words,
                                       float *last_return, float *ret_snapshot, void *stream,
                                       const w2a_lookahead *lookahead, const uint32_t *allowed_days,
                                       int32_t allowed_words) {
  return rollout_linear("w2a_lookahead_rollout_linear_gated", env, policy, n_steps, obs, ret_out, alerts_out, attempts_over_budget, alert_mask,
                        attempt_mask, mask_words, last_return, ret_snapshot, stream, nullptr, true, allowed_days, allowed_words, true,
                        lookahead);
}

// allowed_days nullable: NULL runs the ungated NOISE forms
int w2a_forecast_rollout_linear(w2a_env *env, const w2a_linear_policy *policy, int32_t n_steps, float *obs,
                                float *ret_out, int32_t *alerts_out, int32_t *attempts_over_budget,
                                uint32_t *alert_mask, uint32_t *attempt_mask, int32_t mask_words, float *last_return,
                                float *ret_snapshot, void *stream, const w2a_lookahead *lookahead,
                                const uint32_t *allowed_days, int32_t allowed_words, const w2a_forecast_error *error) {
  return rollout_linear("w2a_forecast_rollout_linear", env, policy, n_steps, obs, ret_out, alerts_out, attempts_over_budget, alert_mask,
                        attempt_mask, mask_words, last_return, ret_snapshot, stream, nullptr, allowed_days != nullptr, allowed_days,
                        allowed_words, true, lookahead, true, error);
}

static int rollout_mlp(const char *fn, w2a_env *env, const w2a_mlp_policy *policy, int32_t n_steps, float *obs, float *ret_out,
                       int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask, uint32_t *attempt_mask,
                       int32_t mask_words, float *last_return, float *ret_snapshot, void *stream,
                       const w2a_trajectory *traj, bool gated = false, const uint32_t *gate = nullptr,
                       int32_t gate_words = 0, bool looking = false, const w2a_lookahead *look = nullptr,
                       bool noisy = false, const w2a_forecast_error *ferr = nullptr) {
  W2A_CHECK(check_mlp_policy_struct(fn, policy, n_steps, SAMPLE_0_OR_1));
  W2A_CHECK(check_obs(fn, obs));
  W2A_CHECK(check_handle_common(fn, env, FIXES_CHANGE_OBS, (alert_mask || attempt_mask) ? MASK_ROLLOUT : MASK_NONE, mask_words));
  W2A_CHECK(check_mlp_stride(fn, policy));
  if (gated) W2A_CHECK(check_gate(fn, env, gate, gate_words));
  if (looking) {
    W2A_CHECK(check_lookahead(fn, env, look, false));
    if ((int64_t)policy->n_groups * W2A_MLP_LOOKAHEAD_STRIDE((int64_t)policy->width, policy->n_layers) >= (1ll << 31))
      return fail(W2A_ERR_ARG, "%s: n_groups * block size must stay below 2^31 floats", fn);
  }
  if (noisy) W2A_CHECK(check_forecast_error(fn, look, ferr));
  W2A_CHECK(refuse_while_capturing(fn, stream));
  MlpRolloutArgs ma;
  memset(&ma, 0, sizeof(ma));
  W2A_CHECK(fill_mlp(fn, env, policy, n_steps, obs, gate, gate_words, ma));
  if (looking) {  // the blocks carry W1f[12][width] at their tail
    fill_lookahead(look, ma.look);
    ma.stride = (int32_t)W2A_MLP_LOOKAHEAD_STRIDE((int64_t)policy->width, policy->n_layers);
  }
  if (noisy) fill_forecast_error(look, ferr, ma.look);
  ma.r.pol.require_budget = policy->require_budget;
  ma.r.pol.seed = policy->seed;
  ma.r.order = policy->order ? mlp_own_order(policy) : env->order;  // the rollout writes state: the handle's order serves too
  set_rollout_outputs(ma.r, ret_out, alerts_out, attempts_over_budget, alert_mask, attempt_mask, mask_words, last_return, ret_snapshot);
  hipStream_t s = (hipStream_t)stream;
  W2A_CHECK(begin_policy_rollout(env, n_steps, W2A_ROLLOUT_KERNEL_MLP, alert_mask, attempt_mask, mask_words, s));
  const unsigned g64 = grid64(env);
  const bool masks = alert_mask || attempt_mask || ret_snapshot;
  const int32_t smp = policy->sample;
  if (traj) {
    W2A_CHECK(clear_trajectory_flags(env, n_steps, traj, s));
    // one group: identity order, the kernel's staged store design (results are order-independent); with groups the
    // group-major order keeps the kernel's group loop short and the rows are stored directly
    if (policy->n_groups == 1) ma.r.order = nullptr;
  }
  if (noisy)
    dispatch_mlp_shape(policy->width, policy->n_layers,
                       [&](auto W, auto L) { launch_rollout_mlp_forecast<W(), L()>(ma, masks, smp, g64, s); });
  else if (looking)
    dispatch_mlp_shape(policy->width, policy->n_layers,
                       [&](auto W, auto L) { launch_rollout_mlp_lookahead<W(), L()>(ma, masks, smp, g64, s); });
  else
    dispatch_mlp_shape(policy->width, policy->n_layers,
                       [&](auto W, auto L) { launch_rollout_mlp<W(), L()>(ma, masks, smp, traj, g64, s); });
  HIP_TRY(hipGetLastError());
  end_call(env, s);
  return W2A_OK;
}

int w2a_rollout_mlp(w2a_env *env, const w2a_mlp_policy *policy, int32_t n_steps, float *obs, float *ret_out,
                    int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask, uint32_t *attempt_mask,
                    int32_t mask_words, float *last_return, float *ret_snapshot, void *stream) {
  return rollout_mlp("w2a_rollout_mlp", env, policy, n_steps, obs, ret_out, alerts_out, attempts_over_budget, alert_mask, attempt_mask,
                     mask_words, last_return, ret_snapshot, stream, nullptr);
}

int w2a_rollout_mlp_record(w2a_env *env, const w2a_mlp_policy *policy, int32_t n_steps, float *obs, float *ret_out,
                           int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask,
                           uint32_t *attempt_mask, int32_t mask_words, float *last_return, float *ret_snapshot,
                           void *stream, const w2a_trajectory *traj) {
  W2A_CHECK(check_trajectory(traj, "w2a_rollout_mlp_record"));
  return rollout_mlp("w2a_rollout_mlp_record", env, policy, n_steps, obs, ret_out, alerts_out, attempts_over_budget, alert_mask, attempt_mask,
                     mask_words, last_return, ret_snapshot, stream, traj);
}

int w2a_rollout_mlp_gated(w2a_env *env, const w2a_mlp_policy *policy, int32_t n_steps, float *obs, float *ret_out,
                          int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask,
                          uint32_t *attempt_mask, int32_t mask_words, float *last_return, float *ret_snapshot,
                          void *stream, const w2a_trajectory *traj, const uint32_t *allowed_days, int32_t allowed_words) {
  if (traj) W2A_CHECK(check_trajectory(traj, "w2a_rollout_mlp_gated"));
  return rollout_mlp("w2a_rollout_mlp_gated", env, policy, n_steps, obs, ret_out, alerts_out, attempts_over_budget, alert_mask, attempt_mask,
                     mask_words, last_return, ret_snapshot, stream, traj, true, allowed_days, allowed_words);
}

int w2a_lookahead_rollout_mlp(w2a_env *env, const w2a_mlp_policy *policy, int32_t n_steps, float *obs, float *ret_out,
                              int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask,
                              uint32_t *attempt_mask, int32_t mask_words, float *last_return, float *ret_snapshot,
                              void *stream, const w2a_lookahead *lookahead) {
  return rollout_mlp("w2a_lookahead_rollout_mlp", env, policy, n_steps, obs, ret_out, alerts_out, attempts_over_budget, alert_mask,
                     attempt_mask, mask_words, last_return, ret_snapshot, stream, nullptr, false, nullptr, 0, true, lookahead);
}

int w2a_lookahead_rollout_mlp_gated(w2a_env *env, const w2a_mlp_policy *policy, int32_t n_steps, float *obs,
                                    float *ret_out, int32_t *alerts_out, int32_t *attempts_over_budget,
                                    uint32_t *alert_mask, uint32_t *attempt_mask, int32_t mask_words,
                                    float *last_return, float *ret_snapshot, void *stream,
                                    const w2a_lookahead *lookahead, const uint32_t *allowed_days,
                                    int32_t allowed_words) {
  return rollout_mlp("w2a_lookahead_rollout_mlp_gated", env, policy, n_steps, obs, ret_out, alerts_out, attempts_over_budget, alert_mask,
                     attempt_mask, mask_words, last_return, ret_snapshot, stream, nullptr, true, allowed_days, allowed_words, true,
                     lookahead);
}

// allowed_days nullable: NULL runs the ungated NOISE forms
int w2a_forecast_rollout_mlp(w2a_env *env, const w2a_mlp_policy *policy, int32_t n_steps, float *obs, float *ret_out,
                             int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask,
                             uint32_t *attempt_mask, int32_t mask_words, float *last_return, float *ret_snapshot,
                             void *stream, const w2a_lookahead *lookahead, const uint32_t *allowed_days,
                             int32_t allowed_words, const w2a_forecast_error *error) {
  return rollout_mlp("w2a_forecast_rollout_mlp", env, policy, n_steps, obs, ret_out, alerts_out, attempts_over_budget, alert_mask,
                     attempt_mask, mask_words, last_return, ret_snapshot, stream, nullptr, allowed_days != nullptr, allowed_days,
                     allowed_words, true, lookahead, true, error);
}

// ---- policy gradients ------------------------------------------------------------------------------------------------
// As found: these two bodies read the canonical state words (the rollout that follows would make them current itself),
// change nothing else, and -- unlike the ten others -- do not call end_call.
static int check_policy_gradient(const char *fn, int32_t baseline, const float *obs, const void *grad, const void *workspace) {
  if (baseline != W2A_PG_BASELINE_NONE && baseline != W2A_PG_BASELINE_NO_ALERT)
    return fail(W2A_ERR_ARG, "%s: baseline must be W2A_PG_BASELINE_NONE or W2A_PG_BASELINE_NO_ALERT", fn);
  W2A_CHECK(check_obs(fn, obs));
  if (!grad || !workspace) return fail(W2A_ERR_ARG, "%s: NULL grad or workspace", fn);
  if ((uintptr_t)workspace & 255) return fail(W2A_ERR_ARG, "%s: workspace must be 256-B aligned", fn);
  return W2A_OK;
}

static int policy_gradient_linear(const char *fn, w2a_env *env, const w2a_linear_policy *policy, int32_t baseline, int32_t n_steps,
                                  const float *obs, float *grad, void *workspace, size_t workspace_bytes, void *stream,
                                  bool gated, const uint32_t *gate, int32_t gate_words, bool looking = false,
                                  const w2a_lookahead *look = nullptr, bool noisy = false,
                                  const w2a_forecast_error *ferr = nullptr) {
  W2A_CHECK(check_linear_policy_struct(fn, policy, n_steps, SAMPLE_MUST_BE_1));
  W2A_CHECK(check_policy_gradient(fn, baseline, obs, grad, workspace));
  W2A_CHECK(check_handle_common(fn, env, FIXES_CHANGE_OBS, MASK_NONE, 0));
  if (workspace_bytes < w2a_policy_gradient_workspace_bytes(env->n, n_steps))
    return fail(W2A_ERR_ARG, "%s: workspace smaller than w2a_policy_gradient_workspace_bytes", fn);
  if (gated) W2A_CHECK(check_gate(fn, env, gate, gate_words));
  if (looking) W2A_CHECK(check_lookahead(fn, env, look, true));
  if (noisy) W2A_CHECK(check_forecast_error(fn, look, ferr));
  W2A_CHECK(refuse_while_capturing(fn, stream));
  PolicyGradArgs ga;
  memset(&ga, 0, sizeof(ga));
  W2A_CHECK(fill_linear(fn, env, policy, n_steps, obs, gate, gate_words, ga.l));
  if (looking) fill_lookahead(look, ga.l.look);
  if (noisy) fill_forecast_error(look, ferr, ga.l.look);
  ga.l.r.pol.require_budget = policy->require_budget;
  ga.l.r.pol.seed = policy->seed;
  ga.l.r.order = env->order;
  ga.baseline = baseline;
  ga.day = reinterpret_cast<float2 *>(workspace);
  ga.day_alert = reinterpret_cast<uint8_t *>(workspace) + align256(sizeof(float2) * (size_t)env->n * (size_t)n_steps);
  ga.grad = grad;
  hipStream_t s = (hipStream_t)stream;
  if (!ensure_canonical(env, s, fn)) return W2A_ERR_STATE;
  const unsigned g64 = grid64(env);
  if (noisy && gated) hipLaunchKernelGGL((k_policy_gradient_linear<true, true, true>), dim3(g64), dim3(BLOCK), 0, s, ga);
  else if (noisy) hipLaunchKernelGGL((k_policy_gradient_linear<false, true, true>), dim3(g64), dim3(BLOCK), 0, s, ga);
  else if (looking && gated) hipLaunchKernelGGL((k_policy_gradient_linear<true, true>), dim3(g64), dim3(BLOCK), 0, s, ga);
  else if (looking) hipLaunchKernelGGL((k_policy_gradient_linear<false, true>), dim3(g64), dim3(BLOCK), 0, s, ga);
  else if (gated) hipLaunchKernelGGL(k_policy_gradient_linear<true>, dim3(g64), dim3(BLOCK), 0, s, ga);
  else hipLaunchKernelGGL(k_policy_gradient_linear<false>, dim3(g64), dim3(BLOCK), 0, s, ga);
  HIP_TRY(hipGetLastError());
  return W2A_OK;
}

int w2a_policy_gradient_linear(w2a_env *env, const w2a_linear_policy *policy, int32_t baseline, int32_t n_steps,
                               const float *obs, float *grad, void *workspace, size_t workspace_bytes, void *stream) {
  return policy_gradient_linear("w2a_policy_gradient_linear", env, policy, baseline, n_steps, obs, grad, workspace, workspace_bytes, stream, false,
                                nullptr, 0);
}

int w2a_policy_gradient_linear_gated(w2a_env *env, const w2a_linear_policy *policy, int32_t baseline, int32_t n_steps,
                                     const float *obs, float *grad, void *workspace, size_t workspace_bytes,
                                     void *stream, const uint32_t *allowed_days, int32_t allowed_words) {
  return policy_gradient_linear("w2a_policy_gradient_linear_gated", env, policy, baseline, n_steps, obs, grad, workspace, workspace_bytes, stream, true,
                                allowed_days, allowed_words);
}

// allowed_days nullable: NULL runs the ungated LOOK form
int w2a_lookahead_policy_gradient_linear(w2a_env *env, const w2a_linear_policy *policy, int32_t baseline,
                                         int32_t n_steps, const float *obs, float *grad, void *workspace,
                                         size_t workspace_bytes, void *stream, const w2a_lookahead *lookahead,
                                         const uint32_t *allowed_days, int32_t allowed_words) {
  return policy_gradient_linear("w2a_lookahead_policy_gradient_linear", env, policy, baseline, n_steps, obs, grad, workspace, workspace_bytes, stream,
                                allowed_days != nullptr, allowed_days, allowed_words, true, lookahead);
}

// allowed_days nullable: NULL runs the ungated NOISE form
int w2a_forecast_policy_gradient_linear(w2a_env *env, const w2a_linear_policy *policy, int32_t baseline,
                                        int32_t n_steps, const float *obs, float *grad, void *workspace,
                                        size_t workspace_bytes, void *stream, const w2a_lookahead *lookahead,
                                        const uint32_t *allowed_days, int32_t allowed_words,
                                        const w2a_forecast_error *error) {
  return policy_gradient_linear("w2a_forecast_policy_gradient_linear", env, policy, baseline, n_steps, obs, grad, workspace, workspace_bytes, stream,
                                allowed_days != nullptr, allowed_days, allowed_words, true, lookahead, true, error);
}

static int policy_gradient_mlp(const char *fn, w2a_env *env, const w2a_mlp_policy *policy, int32_t baseline, int32_t n_steps,
                               const float *obs, float *grad, void *workspace, size_t workspace_bytes, void *stream,
                               bool gated, const uint32_t *gate, int32_t gate_words) {
  W2A_CHECK(check_mlp_policy_struct(fn, policy, n_steps, SAMPLE_MUST_BE_1));
  W2A_CHECK(check_policy_gradient(fn, baseline, obs, grad, workspace));
  W2A_CHECK(check_handle_common(fn, env, FIXES_CHANGE_OBS, MASK_NONE, 0));
  PgmLayout L;
  W2A_CHECK(check_mlp_workspace(fn, env, policy, n_steps, workspace_bytes,
                                "%s: workspace smaller than w2a_policy_gradient_mlp_workspace_bytes", L));
  if (gated) W2A_CHECK(check_gate(fn, env, gate, gate_words));
  W2A_CHECK(refuse_while_capturing(fn, stream));
  MlpGradArgs ga;
  memset(&ga, 0, sizeof(ga));
  W2A_CHECK(fill_mlp(fn, env, policy, n_steps, obs, gate, gate_words, ga.m));
  ga.m.r.pol.require_budget = policy->require_budget;
  ga.m.r.pol.seed = policy->seed;
  ga.m.r.order = mlp_own_order(policy);
  ga.baseline = baseline;
  bind_pgm_workspace(ga, L, workspace, grad);
  hipStream_t s = (hipStream_t)stream;
  if (!ensure_canonical(env, s, fn)) return W2A_ERR_STATE;
  const unsigned g64 = grid64(env);
  dispatch_mlp_shape(policy->width, policy->n_layers, [&](auto W, auto L_) { launch_pgm<W(), L_()>(ga, g64, s); });
  HIP_TRY(hipGetLastError());
  return W2A_OK;
}

int w2a_policy_gradient_mlp(w2a_env *env, const w2a_mlp_policy *policy, int32_t baseline, int32_t n_steps,
                            const float *obs, float *grad, void *workspace, size_t workspace_bytes, void *stream) {
  return policy_gradient_mlp("w2a_policy_gradient_mlp", env, policy, baseline, n_steps, obs, grad, workspace, workspace_bytes, stream, false,
                             nullptr, 0);
}

int w2a_policy_gradient_mlp_gated(w2a_env *env, const w2a_mlp_policy *policy, int32_t baseline, int32_t n_steps,
                                  const float *obs, float *grad, void *workspace, size_t workspace_bytes, void *stream,
                                  const uint32_t *allowed_days, int32_t allowed_words) {
  return policy_gradient_mlp("w2a_policy_gradient_mlp_gated", env, policy, baseline, n_steps, obs, grad, workspace, workspace_bytes, stream, true,
                             allowed_days, allowed_words);
}

// ---- imitation gradients: read the canonical state words, change nothing else ---------------------------------------
static int imitation_gradient_linear(const char *fn, w2a_env *env, const w2a_linear_policy *policy,
                                     const uint32_t *alert_mask, int32_t mask_words, const float *env_weight,
                                     const float *day_weight, int32_t day_weight_days, int32_t n_steps, const float *obs,
                                     float *grad, float *loglik, int32_t *days, void *stream, bool gated = false,
                                     const uint32_t *gate = nullptr, int32_t gate_words = 0, bool looking = false,
                                     const w2a_lookahead *look = nullptr, bool relabel = false,
                                     const uint32_t *labels = nullptr, bool noisy = false,
                                     const w2a_forecast_error *ferr = nullptr) {
  W2A_CHECK(check_linear_policy_struct(fn, policy, n_steps, SAMPLE_0_OR_1));
  W2A_CHECK(check_imitation(fn, alert_mask, obs, grad, loglik, days));
  W2A_CHECK(check_day_weight(fn, day_weight, day_weight_days, n_steps));
  W2A_CHECK(check_handle_common(fn, env, FIXES_CHANGE_OBS, MASK_SCHEDULE, mask_words));
  if (gated) W2A_CHECK(check_gate(fn, env, gate, gate_words));
  if (looking) W2A_CHECK(check_lookahead(fn, env, look, true));
  if (noisy) W2A_CHECK(check_forecast_error(fn, look, ferr));
  W2A_CHECK(refuse_while_capturing(fn, stream));
  if (relabel && !labels) return fail(W2A_ERR_ARG, "%s: NULL labels (the actions to score along the schedule)", fn);
  ImLinearArgs ia;
  memset(&ia, 0, sizeof(ia));
  W2A_CHECK(fill_linear(fn, env, policy, n_steps, obs, gate, gate_words, ia.l));
  if (looking) fill_lookahead(look, ia.l.look);
  if (noisy) fill_forecast_error(look, ferr, ia.l.look);
  ia.l.r.pol.require_budget = policy->require_budget;
  ia.l.r.order = env->order;
  fill_imitation(ia.im, alert_mask, mask_words, env_weight, day_weight, loglik, days);
  ia.im.labels = labels;
  ia.grad = grad;
  hipStream_t s = (hipStream_t)stream;
  if (!ensure_canonical(env, s, fn)) return W2A_ERR_STATE;
  const unsigned g64 = grid64(env);
  if (relabel && gated) hipLaunchKernelGGL((k_imitation_linear<true, false, true>), dim3(g64), dim3(BLOCK), 0, s, ia);
  else if (relabel) hipLaunchKernelGGL((k_imitation_linear<false, false, true>), dim3(g64), dim3(BLOCK), 0, s, ia);
  else if (noisy && gated) hipLaunchKernelGGL((k_imitation_linear<true, true, false, true>), dim3(g64), dim3(BLOCK), 0, s, ia);
  else if (noisy) hipLaunchKernelGGL((k_imitation_linear<false, true, false, true>), dim3(g64), dim3(BLOCK), 0, s, ia);
  else if (looking && gated) hipLaunchKernelGGL((k_imitation_linear<true, true>), dim3(g64), dim3(BLOCK), 0, s, ia);
  else if (looking) hipLaunchKernelGGL((k_imitation_linear<false, true>), dim3(g64), dim3(BLOCK), 0, s, ia);
  else if (gated) hipLaunchKernelGGL(k_imitation_linear<true>, dim3(g64), dim3(BLOCK), 0, s, ia);
  else hipLaunchKernelGGL(k_imitation_linear<false>, dim3(g64), dim3(BLOCK), 0, s, ia);
  HIP_TRY(hipGetLastError());
  end_call(env, s);
  return W2A_OK;
}

int w2a_imitation_gradient_linear(w2a_env *env, const w2a_linear_policy *policy, const uint32_t *alert_mask,
                                  int32_t mask_words, const float *env_weight, int32_t n_steps, const float *obs,
                                  float *grad, float *loglik, int32_t *days, void *stream) {
  return imitation_gradient_linear("w2a_imitation_gradient_linear", env, policy, alert_mask, mask_words, env_weight,
                                   nullptr, 0, n_steps, obs, grad, loglik, days, stream);
}

int w2a_imitation_gradient_linear_weighted(w2a_env *env, const w2a_linear_policy *policy, const uint32_t *alert_mask,
                                           int32_t mask_words, const float *env_weight, const float *day_weight,
                                           int32_t day_weight_days, int32_t n_steps, const float *obs, float *grad,
                                           float *loglik, int32_t *days, void *stream) {
  return imitation_gradient_linear("w2a_imitation_gradient_linear_weighted", env, policy, alert_mask, mask_words,
                                   env_weight, day_weight, day_weight_days, n_steps, obs, grad, loglik, days, stream);
}

// day_weight nullable (= 1), as w2a_imitation_gradient_linear
int w2a_imitation_gradient_linear_gated(w2a_env *env, const w2a_linear_policy *policy, const uint32_t *alert_mask,
                                        int32_t mask_words, const float *env_weight, const float *day_weight,
                                        int32_t day_weight_days, int32_t n_steps, const float *obs, float *grad,
                                        float *loglik, int32_t *days, void *stream, const uint32_t *allowed_days,
                                        int32_t allowed_words) {
  return imitation_gradient_linear("w2a_imitation_gradient_linear_gated", env, policy, alert_mask, mask_words,
                                   env_weight, day_weight, day_weight_days, n_steps, obs, grad, loglik, days, stream,
                                   true, allowed_days, allowed_words);
}

// day_weight and allowed_days nullable (= 1, = no gate)
int w2a_lookahead_imitation_gradient_linear(w2a_env *env, const w2a_linear_policy *policy, const uint32_t *alert_mask,
                                            int32_t mask_words, const float *env_weight, const float *day_weight,
                                            int32_t day_weight_days, int32_t n_steps, const float *obs, float *grad,
                                            float *loglik, int32_t *days, void *stream,
                                            const w2a_lookahead *lookahead, const uint32_t *allowed_days,
                                            int32_t allowed_words) {
  return imitation_gradient_linear("w2a_lookahead_imitation_gradient_linear", env, policy, alert_mask, mask_words,
                                   env_weight, day_weight, day_weight_days, n_steps, obs, grad, loglik, days, stream,
                                   allowed_days != nullptr, allowed_days, allowed_words, true, lookahead);
}

// day_weight and allowed_days nullable (= 1, = no gate)
int w2a_forecast_imitation_gradient_linear(w2a_env *env, const w2a_linear_policy *policy, const uint32_t *alert_mask,
                                           int32_t mask_words, const float *env_weight, const float *day_weight,
                                           int32_t day_weight_days, int32_t n_steps, const float *obs, float *grad,
                                           float *loglik, int32_t *days, void *stream,
                                           const w2a_lookahead *lookahead, const uint32_t *allowed_days,
                                           int32_t allowed_words, const w2a_forecast_error *error) {
  return imitation_gradient_linear("w2a_forecast_imitation_gradient_linear", env, policy, alert_mask, mask_words,
                                   env_weight, day_weight, day_weight_days, n_steps, obs, grad, loglik, days, stream,
                                   allowed_days != nullptr, allowed_days, allowed_words, true, lookahead, false, nullptr,
                                   true, error);
}

// the inputs of the rows the envs hold now, through look_inputs<true> (k_lookahead_features): reads the canonical state
// words, changes nothing
int w2a_forecast_features(w2a_env *env, const w2a_lookahead *lookahead, const w2a_forecast_error *error, float *out,
                          void *stream) {
  const char *fn = "w2a_forecast_features";
  if (!env) return fail(W2A_ERR_ARG, "%s: NULL handle", fn);
  if (!out) return fail(W2A_ERR_ARG, "%s: NULL out", fn);
  W2A_CHECK(check_lookahead(fn, env, lookahead, false));
  W2A_CHECK(check_forecast_error(fn, lookahead, error));
  W2A_CHECK(refuse_while_capturing(fn, stream));
  LookFeaturesArgs fa;
  memset(&fa, 0, sizeof(fa));
  fa.st = env->st; fa.n = env->n; fa.gid0 = env->gid0; fa.out = out;
  fill_lookahead(lookahead, fa.look);
  fill_forecast_error(lookahead, error, fa.look);
  hipStream_t s = (hipStream_t)stream;
  if (!ensure_canonical(env, s, fn)) return W2A_ERR_STATE;
  hipLaunchKernelGGL(k_lookahead_features, dim3((unsigned)((env->n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, fa);
  HIP_TRY(hipGetLastError());
  end_call(env, s);
  return W2A_OK;
}

// labels scored along the schedule that forces the env (DAgger); day_weight and allowed_days nullable (= 1, = no gate)
int w2a_relabel_imitation_linear(w2a_env *env, const w2a_linear_policy *policy, const uint32_t *alert_mask,
                                 int32_t mask_words, const uint32_t *labels, const float *env_weight,
                                 const float *day_weight, int32_t day_weight_days, int32_t n_steps, const float *obs,
                                 float *grad, float *loglik, int32_t *days, void *stream, const uint32_t *allowed_days,
                                 int32_t allowed_words) {
  return imitation_gradient_linear("w2a_relabel_imitation_linear", env, policy, alert_mask, mask_words, env_weight,
                                   day_weight, day_weight_days, n_steps, obs, grad, loglik, days, stream,
                                   allowed_days != nullptr, allowed_days, allowed_words, false, nullptr, true, labels);
}

static int imitation_gradient_mlp(const char *fn, w2a_env *env, const w2a_mlp_policy *policy,
                                  const uint32_t *alert_mask, int32_t mask_words, const float *env_weight,
                                  const float *day_weight, int32_t day_weight_days, int32_t n_steps, const float *obs,
                                  float *grad, float *loglik, int32_t *days, void *workspace, size_t workspace_bytes,
                                  void *stream, bool gated = false, const uint32_t *gate = nullptr,
                                  int32_t gate_words = 0, bool relabel = false, const uint32_t *labels = nullptr) {
  W2A_CHECK(check_mlp_policy_struct(fn, policy, n_steps, SAMPLE_0_OR_1));
  W2A_CHECK(check_imitation(fn, alert_mask, obs, grad, loglik, days));
  W2A_CHECK(check_workspace_pointer(fn, workspace));
  W2A_CHECK(check_day_weight(fn, day_weight, day_weight_days, n_steps));
  W2A_CHECK(check_handle_common(fn, env, FIXES_CHANGE_OBS, MASK_SCHEDULE, mask_words));
  PgmLayout L;
  W2A_CHECK(check_mlp_workspace(fn, env, policy, n_steps, workspace_bytes,
                                "%s: workspace smaller than w2a_imitation_gradient_mlp_workspace_bytes", L));
  if (gated) W2A_CHECK(check_gate(fn, env, gate, gate_words));
  W2A_CHECK(refuse_while_capturing(fn, stream));
  if (relabel && !labels) return fail(W2A_ERR_ARG, "%s: NULL labels (the actions to score along the schedule)", fn);
  ImMlpArgs ia;
  memset(&ia, 0, sizeof(ia));
  W2A_CHECK(fill_mlp(fn, env, policy, n_steps, obs, gate, gate_words, ia.g.m));
  ia.g.m.r.pol.require_budget = policy->require_budget;
  ia.g.m.r.order = mlp_own_order(policy);
  bind_pgm_workspace(ia.g, L, workspace, grad);
  fill_imitation(ia.im, alert_mask, mask_words, env_weight, day_weight, loglik, days);
  ia.im.labels = labels;
  hipStream_t s = (hipStream_t)stream;
  if (!ensure_canonical(env, s, fn)) return W2A_ERR_STATE;
  const unsigned g64 = grid64(env);
  dispatch_mlp_shape(policy->width, policy->n_layers, [&](auto W, auto L_) { launch_im<W(), L_()>(ia, g64, s); });
  HIP_TRY(hipGetLastError());
  end_call(env, s);
  return W2A_OK;
}

int w2a_imitation_gradient_mlp(w2a_env *env, const w2a_mlp_policy *policy, const uint32_t *alert_mask,
                               int32_t mask_words, const float *env_weight, int32_t n_steps, const float *obs,
                               float *grad, float *loglik, int32_t *days, void *workspace, size_t workspace_bytes,
                               void *stream) {
  return imitation_gradient_mlp("w2a_imitation_gradient_mlp", env, policy, alert_mask, mask_words, env_weight, nullptr,
                                0, n_steps, obs, grad, loglik, days, workspace, workspace_bytes, stream);
}

int w2a_imitation_gradient_mlp_weighted(w2a_env *env, const w2a_mlp_policy *policy, const uint32_t *alert_mask,
                                        int32_t mask_words, const float *env_weight, const float *day_weight,
                                        int32_t day_weight_days, int32_t n_steps, const float *obs, float *grad,
                                        float *loglik, int32_t *days, void *workspace, size_t workspace_bytes,
                                        void *stream) {
  return imitation_gradient_mlp("w2a_imitation_gradient_mlp_weighted", env, policy, alert_mask, mask_words, env_weight,
                                day_weight, day_weight_days, n_steps, obs, grad, loglik, days, workspace,
                                workspace_bytes, stream);
}

// day_weight nullable (= 1), as w2a_imitation_gradient_mlp
int w2a_imitation_gradient_mlp_gated(w2a_env *env, const w2a_mlp_policy *policy, const uint32_t *alert_mask,
                                     int32_t mask_words, const float *env_weight, const float *day_weight,
                                     int32_t day_weight_days, int32_t n_steps, const float *obs, float *grad,
                                     float *loglik, int32_t *days, void *workspace, size_t workspace_bytes,
                                     void *stream, const uint32_t *allowed_days, int32_t allowed_words) {
  return imitation_gradient_mlp("w2a_imitation_gradient_mlp_gated", env, policy, alert_mask, mask_words, env_weight,
                                day_weight, day_weight_days, n_steps, obs, grad, loglik, days, workspace,
                                workspace_bytes, stream, true, allowed_days, allowed_words);
}

int w2a_relabel_imitation_mlp(w2a_env *env, const w2a_mlp_policy *policy, const uint32_t *alert_mask,
                              int32_t mask_words, const uint32_t *labels, const float *env_weight,
                              const float *day_weight, int32_t day_weight_days, int32_t n_steps, const float *obs,
                              float *grad, float *loglik, int32_t *days, void *workspace, size_t workspace_bytes,
                              void *stream, const uint32_t *allowed_days, int32_t allowed_words) {
  return imitation_gradient_mlp("w2a_relabel_imitation_mlp", env, policy, alert_mask, mask_words, env_weight,
                                day_weight, day_weight_days, n_steps, obs, grad, loglik, days, workspace,
                                workspace_bytes, stream, allowed_days != nullptr, allowed_days, allowed_words, true,
                                labels);
}

// ---- surrogate gradients: read the canonical state words, change nothing else ---------------------------------------
static int surrogate_gradient_linear(const char *fn, w2a_env *env, const w2a_linear_policy *policy,
                                     const uint32_t *alert_mask, int32_t mask_words, const float *env_weight,
                                     const float *advantage, int32_t advantage_days, const float *old_log_prob,
                                     int32_t old_log_prob_days, double clip, double entropy_coef, int32_t n_steps,
                                     const float *obs, float *grad, float *surrogate, int32_t *clipped_days,
                                     float *approx_kl, float *entropy, int32_t *days, float *log_prob, void *stream,
                                     bool gated, const uint32_t *gate, int32_t gate_words) {
  W2A_CHECK(check_linear_policy_struct(fn, policy, n_steps, SAMPLE_0_OR_1));
  W2A_CHECK(check_surrogate_outputs(fn, alert_mask, obs, grad, surrogate, clipped_days, approx_kl, entropy, days));
  W2A_CHECK(check_surrogate_inputs(fn, advantage, advantage_days, old_log_prob, old_log_prob_days, clip, entropy_coef, n_steps));
  W2A_CHECK(check_handle_common(fn, env, FIXES_CHANGE_OBS, MASK_SCHEDULE, mask_words));
  if (gated) W2A_CHECK(check_gate(fn, env, gate, gate_words));
  W2A_CHECK(refuse_while_capturing(fn, stream));
  SgLinearArgs sa;
  memset(&sa, 0, sizeof(sa));
  W2A_CHECK(fill_linear(fn, env, policy, n_steps, obs, gate, gate_words, sa.l));
  sa.l.r.pol.require_budget = policy->require_budget;
  sa.l.r.order = env->order;
  fill_surrogate(sa.sg, alert_mask, mask_words, env_weight, advantage, old_log_prob, clip, entropy_coef, log_prob, surrogate,
                 clipped_days, approx_kl, entropy, days);
  sa.grad = grad;
  hipStream_t s = (hipStream_t)stream;
  if (!ensure_canonical(env, s, fn)) return W2A_ERR_STATE;
  W2A_CHECK(clear_day_rows(env, n_steps, log_prob, s));
  const unsigned g64 = grid64(env);
  if (gated) hipLaunchKernelGGL(k_surrogate_linear<true>, dim3(g64), dim3(BLOCK), 0, s, sa);
  else hipLaunchKernelGGL(k_surrogate_linear<false>, dim3(g64), dim3(BLOCK), 0, s, sa);
  HIP_TRY(hipGetLastError());
  end_call(env, s);
  return W2A_OK;
}

int w2a_surrogate_gradient_linear(w2a_env *env, const w2a_linear_policy *policy, const uint32_t *alert_mask,
                                  int32_t mask_words, const float *env_weight, const float *advantage,
                                  int32_t advantage_days, const float *old_log_prob, int32_t old_log_prob_days,
                                  double clip, double entropy_coef, int32_t n_steps, const float *obs, float *grad,
                                  float *surrogate, int32_t *clipped_days, float *approx_kl, float *entropy,
                                  int32_t *days, float *log_prob, void *stream) {
  return surrogate_gradient_linear("w2a_surrogate_gradient_linear", env, policy, alert_mask, mask_words, env_weight,
                                   advantage, advantage_days, old_log_prob, old_log_prob_days, clip, entropy_coef,
                                   n_steps, obs, grad, surrogate, clipped_days, approx_kl, entropy, days, log_prob,
                                   stream, false, nullptr, 0);
}

int w2a_surrogate_gradient_linear_gated(w2a_env *env, const w2a_linear_policy *policy, const uint32_t *alert_mask,
                                        int32_t mask_words, const float *env_weight, const float *advantage,
                                        int32_t advantage_days, const float *old_log_prob, int32_t old_log_prob_days,
                                        double clip, double entropy_coef, int32_t n_steps, const float *obs,
                                        float *grad, float *surrogate, int32_t *clipped_days, float *approx_kl,
                                        float *entropy, int32_t *days, float *log_prob, void *stream,
                                        const uint32_t *allowed_days, int32_t allowed_words) {
  return surrogate_gradient_linear("w2a_surrogate_gradient_linear_gated", env, policy, alert_mask, mask_words,
                                   env_weight, advantage, advantage_days, old_log_prob, old_log_prob_days, clip,
                                   entropy_coef, n_steps, obs, grad, surrogate, clipped_days, approx_kl, entropy, days,
                                   log_prob, stream, true, allowed_days, allowed_words);
}

static int surrogate_gradient_mlp(const char *fn, w2a_env *env, const w2a_mlp_policy *policy,
                                  const uint32_t *alert_mask, int32_t mask_words, const float *env_weight,
                                  const float *advantage, int32_t advantage_days, const float *old_log_prob,
                                  int32_t old_log_prob_days, double clip, double entropy_coef, int32_t n_steps,
                                  const float *obs, float *grad, float *surrogate, int32_t *clipped_days,
                                  float *approx_kl, float *entropy, int32_t *days, float *log_prob, void *workspace,
                                  size_t workspace_bytes, void *stream, bool gated, const uint32_t *gate,
                                  int32_t gate_words) {
  W2A_CHECK(check_mlp_policy_struct(fn, policy, n_steps, SAMPLE_0_OR_1));
  W2A_CHECK(check_surrogate_outputs(fn, alert_mask, obs, grad, surrogate, clipped_days, approx_kl, entropy, days));
  W2A_CHECK(check_workspace_pointer(fn, workspace));
  W2A_CHECK(check_surrogate_inputs(fn, advantage, advantage_days, old_log_prob, old_log_prob_days, clip, entropy_coef, n_steps));
  W2A_CHECK(check_handle_common(fn, env, FIXES_CHANGE_OBS, MASK_SCHEDULE, mask_words));
  PgmLayout L;
  W2A_CHECK(check_mlp_workspace(fn, env, policy, n_steps, workspace_bytes,
                                "%s: workspace smaller than w2a_surrogate_gradient_mlp_workspace_bytes", L));
  if (gated) W2A_CHECK(check_gate(fn, env, gate, gate_words));
  W2A_CHECK(refuse_while_capturing(fn, stream));
  SgMlpArgs sa;
  memset(&sa, 0, sizeof(sa));
  W2A_CHECK(fill_mlp(fn, env, policy, n_steps, obs, gate, gate_words, sa.g.m));
  sa.g.m.r.pol.require_budget = policy->require_budget;
  sa.g.m.r.order = mlp_own_order(policy);
  bind_pgm_workspace(sa.g, L, workspace, grad);
  fill_surrogate(sa.sg, alert_mask, mask_words, env_weight, advantage, old_log_prob, clip, entropy_coef, log_prob, surrogate,
                 clipped_days, approx_kl, entropy, days);
  hipStream_t s = (hipStream_t)stream;
  if (!ensure_canonical(env, s, fn)) return W2A_ERR_STATE;
  W2A_CHECK(clear_day_rows(env, n_steps, log_prob, s));
  const unsigned g64 = grid64(env);
  dispatch_mlp_shape(policy->width, policy->n_layers, [&](auto W, auto L_) { launch_sg<W(), L_()>(sa, g64, s); });
  HIP_TRY(hipGetLastError());
  end_call(env, s);
  return W2A_OK;
}

int w2a_surrogate_gradient_mlp(w2a_env *env, const w2a_mlp_policy *policy, const uint32_t *alert_mask,
                               int32_t mask_words, const float *env_weight, const float *advantage,
                               int32_t advantage_days, const float *old_log_prob, int32_t old_log_prob_days,
                               double clip, double entropy_coef, int32_t n_steps, const float *obs, float *grad,
                               float *surrogate, int32_t *clipped_days, float *approx_kl, float *entropy,
                               int32_t *days, float *log_prob, void *workspace, size_t workspace_bytes, void *stream) {
  return surrogate_gradient_mlp("w2a_surrogate_gradient_mlp", env, policy, alert_mask, mask_words, env_weight,
                                advantage, advantage_days, old_log_prob, old_log_prob_days, clip, entropy_coef, n_steps,
                                obs, grad, surrogate, clipped_days, approx_kl, entropy, days, log_prob, workspace,
                                workspace_bytes, stream, false, nullptr, 0);
}

int w2a_surrogate_gradient_mlp_gated(w2a_env *env, const w2a_mlp_policy *policy, const uint32_t *alert_mask,
                                     int32_t mask_words, const float *env_weight, const float *advantage,
                                     int32_t advantage_days, const float *old_log_prob, int32_t old_log_prob_days,
                                     double clip, double entropy_coef, int32_t n_steps, const float *obs, float *grad,
                                     float *surrogate, int32_t *clipped_days, float *approx_kl, float *entropy,
                                     int32_t *days, float *log_prob, void *workspace, size_t workspace_bytes,
                                     void *stream, const uint32_t *allowed_days, int32_t allowed_words) {
  return surrogate_gradient_mlp("w2a_surrogate_gradient_mlp_gated", env, policy, alert_mask, mask_words, env_weight,
                                advantage, advantage_days, old_log_prob, old_log_prob_days, clip, entropy_coef, n_steps,
                                obs, grad, surrogate, clipped_days, approx_kl, entropy, days, log_prob, workspace,
                                workspace_bytes, stream, true, allowed_days, allowed_words);
}

// ---- Fisher-vector products: read the canonical state words, change nothing else -------------------------------------
// New exports take the nullable gate directly (NULL: no gate, allowed_words is not read), so there are no _gated twins.
static int check_fisher_outputs(const char *fn, const uint32_t *alert_mask, const float *obs, const void *fv,
                                const float *quadratic, const int32_t *days) {
  if (!alert_mask) return fail(W2A_ERR_ARG, "%s: NULL alert_mask (the schedule to follow)", fn);
  W2A_CHECK(check_obs(fn, obs));
  if (!fv || !quadratic || !days) return fail(W2A_ERR_ARG, "%s: NULL fv, quadratic or days", fn);
  return W2A_OK;
}

static void fill_fisher(FisherArgs &f, const uint32_t *alert_mask, int32_t mask_words, const float *env_weight,
                        float *quadratic, int32_t *days) {
  f.alert_mask = alert_mask; f.mask_words = mask_words; f.env_weight = env_weight;
  f.quadratic = quadratic; f.days = days;
}

size_t w2a_fisher_vector_product_mlp_workspace_bytes(int64_t num_envs, int32_t n_steps, int32_t n_groups, int32_t width,
                                                     int32_t n_layers) {
  return w2a_policy_gradient_mlp_workspace_bytes(num_envs, n_steps, n_groups, width, n_layers);
}

int w2a_fisher_vector_product_linear(w2a_env *env, const w2a_linear_policy *policy, const float *vec_weight,
                                     const float *vec_bias, const uint32_t *alert_mask, int32_t mask_words,
                                     const float *env_weight, int32_t n_steps, const float *obs, float *fv,
                                     float *quadratic, int32_t *days, void *stream, const uint32_t *allowed_days,
                                     int32_t allowed_words) {
  const char *fn = "w2a_fisher_vector_product_linear";
  W2A_CHECK(check_linear_policy_struct(fn, policy, n_steps, SAMPLE_0_OR_1));
  if (!vec_weight || !vec_bias) return fail(W2A_ERR_ARG, "%s: NULL vec_weight or vec_bias", fn);
  if ((uintptr_t)vec_weight & 15) return fail(W2A_ERR_ARG, "%s: vec_weight must be 16-B aligned", fn);
  W2A_CHECK(check_fisher_outputs(fn, alert_mask, obs, fv, quadratic, days));
  W2A_CHECK(check_handle_common(fn, env, FIXES_CHANGE_OBS, MASK_SCHEDULE, mask_words));
  if (allowed_days) W2A_CHECK(check_gate(fn, env, allowed_days, allowed_words));
  W2A_CHECK(refuse_while_capturing(fn, stream));
  FvLinearArgs fa;
  memset(&fa, 0, sizeof(fa));
  W2A_CHECK(fill_linear(fn, env, policy, n_steps, obs, allowed_days, allowed_days ? allowed_words : 0, fa.l));
  fa.l.r.pol.require_budget = policy->require_budget;
  fa.l.r.order = env->order;
  fill_fisher(fa.fv, alert_mask, mask_words, env_weight, quadratic, days);
  fa.vec_weight = reinterpret_cast<const float4 *>(vec_weight);
  fa.vec_bias = vec_bias;
  fa.grad = fv;
  hipStream_t s = (hipStream_t)stream;
  if (!ensure_canonical(env, s, fn)) return W2A_ERR_STATE;
  const unsigned g64 = grid64(env);
  if (allowed_days) hipLaunchKernelGGL(k_fisher_linear<true>, dim3(g64), dim3(BLOCK), 0, s, fa);
  else hipLaunchKernelGGL(k_fisher_linear<false>, dim3(g64), dim3(BLOCK), 0, s, fa);
  HIP_TRY(hipGetLastError());
  end_call(env, s);
  return W2A_OK;
}

int w2a_fisher_vector_product_mlp(w2a_env *env, const w2a_mlp_policy *policy, const float *vector,
                                  const uint32_t *alert_mask, int32_t mask_words, const float *env_weight,
                                  int32_t n_steps, const float *obs, float *fv, float *quadratic, int32_t *days,
                                  void *workspace, size_t workspace_bytes, void *stream, const uint32_t *allowed_days,
                                  int32_t allowed_words) {
  const char *fn = "w2a_fisher_vector_product_mlp";
  W2A_CHECK(check_mlp_policy_struct(fn, policy, n_steps, SAMPLE_0_OR_1));
  if (!vector) return fail(W2A_ERR_ARG, "%s: NULL vector", fn);
  if ((uintptr_t)vector & 15) return fail(W2A_ERR_ARG, "%s: vector must be 16-B aligned", fn);
  W2A_CHECK(check_fisher_outputs(fn, alert_mask, obs, fv, quadratic, days));
  W2A_CHECK(check_workspace_pointer(fn, workspace));
  W2A_CHECK(check_handle_common(fn, env, FIXES_CHANGE_OBS, MASK_SCHEDULE, mask_words));
  PgmLayout L;
  W2A_CHECK(check_mlp_workspace(fn, env, policy, n_steps, workspace_bytes,
                                "%s: workspace smaller than w2a_fisher_vector_product_mlp_workspace_bytes", L));
  if (allowed_days) W2A_CHECK(check_gate(fn, env, allowed_days, allowed_words));
  W2A_CHECK(refuse_while_capturing(fn, stream));
  FvMlpArgs fa;
  memset(&fa, 0, sizeof(fa));
  W2A_CHECK(fill_mlp(fn, env, policy, n_steps, obs, allowed_days, allowed_days ? allowed_words : 0, fa.g.m));
  fa.g.m.r.pol.require_budget = policy->require_budget;
  fa.g.m.r.order = mlp_own_order(policy);
  bind_pgm_workspace(fa.g, L, workspace, fv);
  fill_fisher(fa.fv, alert_mask, mask_words, env_weight, quadratic, days);
  fa.vec = vector;
  hipStream_t s = (hipStream_t)stream;
  if (!ensure_canonical(env, s, fn)) return W2A_ERR_STATE;
  const unsigned g64 = grid64(env);
  dispatch_mlp_shape(policy->width, policy->n_layers, [&](auto W, auto L_) { launch_fv<W(), L_()>(fa, g64, s); });
  HIP_TRY(hipGetLastError());
  end_call(env, s);
  return W2A_OK;
}

// ---- value gradients and GAE: read the canonical state words, change nothing else; no gate, no pol fields ------------
int w2a_value_gradient_linear(w2a_env *env, const w2a_linear_policy *value, const uint32_t *alert_mask,
                              int32_t mask_words, const float *env_weight, int32_t n_steps, const float *obs,
                              float *grad, float *sq_error, int32_t *days, float *ret, float *advantage,
                              void *workspace, size_t workspace_bytes, void *stream) {
  const char *fn = "w2a_value_gradient_linear";
  W2A_CHECK(check_linear_policy_struct(fn, value, n_steps, SAMPLE_IGNORED));
  W2A_CHECK(check_value(fn, alert_mask, obs, grad, sq_error, days, ret));
  W2A_CHECK(check_workspace_pointer(fn, workspace));
  W2A_CHECK(check_handle_common(fn, env, FIXES_CHANGE_OBS_AND_REWARD, MASK_SCHEDULE, mask_words));
  if (workspace_bytes < w2a_value_gradient_linear_workspace_bytes(env->n, n_steps))
    return fail(W2A_ERR_ARG, "%s: workspace smaller than w2a_value_gradient_linear_workspace_bytes", fn);
  W2A_CHECK(refuse_while_capturing(fn, stream));
  VgLinearArgs va;
  memset(&va, 0, sizeof(va));
  W2A_CHECK(fill_linear(fn, env, value, n_steps, obs, nullptr, 0, va.l));
  va.l.r.order = env->order;
  fill_value(va.v, alert_mask, mask_words, env_weight, sq_error, days, ret, advantage);
  va.day_y = reinterpret_cast<double *>(workspace);
  va.day_alert = reinterpret_cast<uint8_t *>(workspace) + align256(sizeof(double) * (size_t)env->n * (size_t)n_steps);
  va.grad = grad;
  hipStream_t s = (hipStream_t)stream;
  if (!ensure_canonical(env, s, fn)) return W2A_ERR_STATE;
  W2A_CHECK(clear_day_rows(env, n_steps, advantage, s));
  hipLaunchKernelGGL(k_value_gradient_linear, dim3(grid64(env)), dim3(BLOCK), 0, s, va);
  HIP_TRY(hipGetLastError());
  end_call(env, s);
  return W2A_OK;
}

int w2a_value_gradient_mlp(w2a_env *env, const w2a_mlp_policy *value, const uint32_t *alert_mask, int32_t mask_words,
                           const float *env_weight, int32_t n_steps, const float *obs, float *grad, float *sq_error,
                           int32_t *days, float *ret, float *advantage, void *workspace, size_t workspace_bytes,
                           void *stream) {
  const char *fn = "w2a_value_gradient_mlp";
  W2A_CHECK(check_mlp_policy_struct(fn, value, n_steps, SAMPLE_IGNORED));
  W2A_CHECK(check_value(fn, alert_mask, obs, grad, sq_error, days, ret));
  W2A_CHECK(check_workspace_pointer(fn, workspace));
  W2A_CHECK(check_handle_common(fn, env, FIXES_CHANGE_OBS_AND_REWARD, MASK_SCHEDULE, mask_words));
  PgmLayout L;
  W2A_CHECK(check_mlp_workspace(fn, env, value, n_steps, workspace_bytes,
                                "%s: workspace smaller than w2a_value_gradient_mlp_workspace_bytes", L));
  W2A_CHECK(refuse_while_capturing(fn, stream));
  VgMlpArgs va;
  memset(&va, 0, sizeof(va));
  W2A_CHECK(fill_mlp(fn, env, value, n_steps, obs, nullptr, 0, va.g.m));
  va.g.m.r.order = mlp_own_order(value);
  bind_pgm_workspace(va.g, L, workspace, grad);
  fill_value(va.v, alert_mask, mask_words, env_weight, sq_error, days, ret, advantage);
  hipStream_t s = (hipStream_t)stream;
  if (!ensure_canonical(env, s, fn)) return W2A_ERR_STATE;
  W2A_CHECK(clear_day_rows(env, n_steps, advantage, s));
  const unsigned g64 = grid64(env);
  dispatch_mlp_shape(value->width, value->n_layers, [&](auto W, auto L_) { launch_vg<W(), L_()>(va, g64, s); });
  HIP_TRY(hipGetLastError());
  end_call(env, s);
  return W2A_OK;
}

int w2a_value_gradient_linear_gae(w2a_env *env, const w2a_linear_policy *value, const uint32_t *alert_mask,
                                  int32_t mask_words, const float *env_weight, int32_t n_steps, const float *obs,
                                  float *grad, float *sq_error, int32_t *days, float *ret, float *advantage,
                                  double gamma, double lambda, int32_t bootstrap, float *value_target,
                                  const float *target, int32_t target_days, void *workspace, size_t workspace_bytes,
                                  void *stream) {
  const char *fn = "w2a_value_gradient_linear_gae";
  W2A_CHECK(check_linear_policy_struct(fn, value, n_steps, SAMPLE_IGNORED));
  W2A_CHECK(check_value(fn, alert_mask, obs, grad, sq_error, days, ret));
  W2A_CHECK(check_gae(fn, gamma, lambda, bootstrap, advantage, value_target, target, target_days, n_steps));
  W2A_CHECK(check_workspace_pointer(fn, workspace));
  W2A_CHECK(check_handle_common(fn, env, FIXES_CHANGE_OBS_AND_REWARD, MASK_SCHEDULE, mask_words));
  if (workspace_bytes < w2a_value_gradient_linear_gae_workspace_bytes(env->n, n_steps))
    return fail(W2A_ERR_ARG, "%s: workspace smaller than w2a_value_gradient_linear_gae_workspace_bytes", fn);
  W2A_CHECK(refuse_while_capturing(fn, stream));
  GaeLinearArgs xa;
  memset(&xa, 0, sizeof(xa));
  VgLinearArgs &va = xa.v;
  W2A_CHECK(fill_linear(fn, env, value, n_steps, obs, nullptr, 0, va.l));
  va.l.r.order = env->order;
  fill_value(va.v, alert_mask, mask_words, env_weight, sq_error, days, ret, advantage);
  const size_t col = align256(sizeof(double) * (size_t)env->n * (size_t)n_steps);
  va.day_y = reinterpret_cast<double *>(workspace);
  xa.day_v = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + col);
  va.day_alert = reinterpret_cast<uint8_t *>(workspace) + 2 * col;
  va.grad = grad;
  fill_gae(xa.g, gamma, lambda, bootstrap, value_target, target);
  hipStream_t s = (hipStream_t)stream;
  if (!ensure_canonical(env, s, fn)) return W2A_ERR_STATE;
  W2A_CHECK(clear_day_rows(env, n_steps, advantage, s));
  W2A_CHECK(clear_day_rows(env, n_steps, value_target, s));
  const unsigned g64 = grid64(env);
  if (target) hipLaunchKernelGGL(k_value_gradient_linear_gae<true>, dim3(g64), dim3(BLOCK), 0, s, xa);
  else hipLaunchKernelGGL(k_value_gradient_linear_gae<false>, dim3(g64), dim3(BLOCK), 0, s, xa);
  HIP_TRY(hipGetLastError());
  end_call(env, s);
  return W2A_OK;
}

int w2a_value_gradient_mlp_gae(w2a_env *env, const w2a_mlp_policy *value, const uint32_t *alert_mask,
                               int32_t mask_words, const float *env_weight, int32_t n_steps, const float *obs,
                               float *grad, float *sq_error, int32_t *days, float *ret, float *advantage, double gamma,
                               double lambda, int32_t bootstrap, float *value_target, const float *target,
                               int32_t target_days, void *workspace, size_t workspace_bytes, void *stream) {
  const char *fn = "w2a_value_gradient_mlp_gae";
  W2A_CHECK(check_mlp_policy_struct(fn, value, n_steps, SAMPLE_IGNORED));
  W2A_CHECK(check_value(fn, alert_mask, obs, grad, sq_error, days, ret));
  W2A_CHECK(check_gae(fn, gamma, lambda, bootstrap, advantage, value_target, target, target_days, n_steps));
  W2A_CHECK(check_workspace_pointer(fn, workspace));
  W2A_CHECK(check_handle_common(fn, env, FIXES_CHANGE_OBS_AND_REWARD, MASK_SCHEDULE, mask_words));
  PgmLayout L;
  W2A_CHECK(check_mlp_workspace(fn, env, value, n_steps, workspace_bytes,
                                "%s: workspace smaller than w2a_value_gradient_mlp_gae_workspace_bytes", L));
  W2A_CHECK(refuse_while_capturing(fn, stream));
  GaeMlpArgs xa;
  memset(&xa, 0, sizeof(xa));
  VgMlpArgs &va = xa.v;
  W2A_CHECK(fill_mlp(fn, env, value, n_steps, obs, nullptr, 0, va.g.m));
  va.g.m.r.order = mlp_own_order(value);
  bind_pgm_workspace(va.g, L, workspace, grad);
  fill_value(va.v, alert_mask, mask_words, env_weight, sq_error, days, ret, advantage);
  fill_gae(xa.g, gamma, lambda, bootstrap, value_target, target);
  hipStream_t s = (hipStream_t)stream;
  if (!ensure_canonical(env, s, fn)) return W2A_ERR_STATE;
  W2A_CHECK(clear_day_rows(env, n_steps, advantage, s));
  W2A_CHECK(clear_day_rows(env, n_steps, value_target, s));
  const unsigned g64 = grid64(env);
  dispatch_mlp_shape(value->width, value->n_layers, [&](auto W, auto L_) { launch_gae<W(), L_()>(xa, g64, s); });
  HIP_TRY(hipGetLastError());
  end_call(env, s);
  return W2A_OK;
}

// ---- Q-learning ------------------------------------------------------------------------------------------------------
// what w2a_q_gradient_mlp checks beyond check_value: the target net against the online one, and the estimator's scalars
static int check_q_args(const char *fn, const w2a_mlp_policy *q, const w2a_mlp_policy *target_net, double gamma,
                        int32_t double_q, int32_t loss, double huber_delta, int32_t bootstrap) {
  if (q->require_budget != 0 && q->require_budget != 1) return fail(W2A_ERR_ARG, "%s: require_budget must be 0 or 1", fn);
  if (target_net) {
    if (!target_net->params) return fail(W2A_ERR_ARG, "%s: NULL params of the target net", fn);
    if ((uintptr_t)target_net->params & 15) return fail(W2A_ERR_ARG, "%s: the target net's params must be 16-B aligned", fn);
    if (target_net->width != q->width || target_net->n_layers != q->n_layers ||
        target_net->activation != q->activation || target_net->n_groups != q->n_groups)
      return fail(W2A_ERR_ARG, "%s: the target net must have the online net's width, n_layers, activation and n_groups", fn);
  }
  if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(W2A_ERR_ARG, "%s: gamma must lie in [0, 1]", fn);
  if (double_q != 0 && double_q != 1) return fail(W2A_ERR_ARG, "%s: double_q must be 0 or 1", fn);
  if (loss != W2A_Q_LOSS_SQUARED && loss != W2A_Q_LOSS_HUBER)
    return fail(W2A_ERR_ARG, "%s: loss must be W2A_Q_LOSS_SQUARED or W2A_Q_LOSS_HUBER", fn);
  if (loss == W2A_Q_LOSS_HUBER && !(isfinite(huber_delta) && huber_delta > 0.0))
    return fail(W2A_ERR_ARG, "%s: huber_delta must be finite and positive", fn);
  if (bootstrap != 0 && bootstrap != 1) return fail(W2A_ERR_ARG, "%s: bootstrap must be 0 or 1", fn);
  return W2A_OK;
}

int w2a_q_gradient_mlp(w2a_env *env, const w2a_mlp_policy *q, const w2a_mlp_policy *target_net,
                       const uint32_t *alert_mask, int32_t mask_words, const float *env_weight, int32_t n_steps,
                       const float *obs, float *grad, float *loss_out, int32_t *days, float *ret, double gamma,
                       int32_t double_q, int32_t loss, double huber_delta, int32_t bootstrap, float *td_error,
                       float *td_target, void *workspace, size_t workspace_bytes, void *stream) {
  const char *fn = "w2a_q_gradient_mlp";
  if (!q) return fail(W2A_ERR_ARG, "%s: NULL q (the online Q-net)", fn);  // not the value calls' "NULL value"
  W2A_CHECK(check_mlp_policy_struct(fn, q, n_steps, SAMPLE_IGNORED));
  if (!alert_mask) return fail(W2A_ERR_ARG, "%s: NULL alert_mask (the schedule to follow)", fn);
  W2A_CHECK(check_obs(fn, obs));
  if (!grad || !loss_out || !days || !ret) return fail(W2A_ERR_ARG, "%s: NULL grad, loss, days or ret", fn);
  W2A_CHECK(check_q_args(fn, q, target_net, gamma, double_q, loss, huber_delta, bootstrap));
  W2A_CHECK(check_workspace_pointer(fn, workspace));
  W2A_CHECK(check_handle_common(fn, env, FIXES_CHANGE_OBS_AND_REWARD, MASK_SCHEDULE, mask_words));
  if ((int64_t)q->n_groups * W2A_MLP_HEADS_STRIDE((int64_t)q->width, q->n_layers) >= (1ll << 31))
    return fail(W2A_ERR_ARG, "%s: n_groups * block size must stay below 2^31 floats", fn);
  const PgmLayout L = pgm_layout(env->n, n_steps, q->n_groups, q->width, q->n_layers, 2);
  if (workspace_bytes < L.bytes)
    return fail(W2A_ERR_ARG, "%s: workspace smaller than w2a_q_gradient_mlp_workspace_bytes", fn);
  W2A_CHECK(refuse_while_capturing(fn, stream));
  QgMlpArgs qa;
  memset(&qa, 0, sizeof(qa));
  W2A_CHECK(fill_mlp(fn, env, q, n_steps, obs, nullptr, 0, qa.g.m));
  qa.g.m.stride = (int32_t)W2A_MLP_HEADS_STRIDE((int64_t)q->width, q->n_layers);  // below 2^31: checked above
  qa.g.m.r.order = mlp_own_order(q);
  qa.g.m.r.pol.require_budget = q->require_budget;  // masks the next row's max / argmax when no budget is left
  bind_pgm_workspace(qa.g, L, workspace, grad);
  fill_value(qa.v, alert_mask, mask_words, env_weight, loss_out, days, ret, td_error);
  qa.tparams = target_net ? target_net->params : q->params;
  qa.td_target = td_target;
  qa.gamma = gamma;
  qa.huber_delta = loss == W2A_Q_LOSS_HUBER ? huber_delta : 0.0;
  qa.double_q = double_q;
  qa.bootstrap = bootstrap;
  hipStream_t s = (hipStream_t)stream;
  if (!ensure_canonical(env, s, fn)) return W2A_ERR_STATE;
  W2A_CHECK(clear_day_rows(env, n_steps, td_error, s));
  W2A_CHECK(clear_day_rows(env, n_steps, td_target, s));
  const unsigned g64 = grid64(env);
  dispatch_mlp_shape(q->width, q->n_layers, [&](auto W, auto L_) { launch_qg<W(), L_()>(qa, g64, s); });
  HIP_TRY(hipGetLastError());
  end_call(env, s);
  return W2A_OK;
}

// ---- shared-trunk actor-critic ---------------------------------------------------------------------------------------
// w2a_q_gradient_mlp's layout (the partial blocks at the two-head stride), then the collect call's z_s column
static PgmLayout ac_layout(int64_t n, int32_t n_steps, int32_t n_groups, int32_t width, int32_t n_layers, size_t &day_z) {
  PgmLayout L = pgm_layout(n, n_steps, n_groups, width, n_layers, 2);
  day_z = L.bytes;
  L.bytes += align256(sizeof(float) * (size_t)n * (size_t)n_steps);
  return L;
}

size_t w2a_actor_critic_mlp_workspace_bytes(int64_t num_envs, int32_t n_steps, int32_t n_groups, int32_t width,
                                            int32_t n_layers) {
  if (num_envs <= 0 || n_steps <= 0 || n_groups <= 0) return 0;
  if ((width != 16 && width != 32 && width != 64) || (n_layers != 1 && n_layers != 2)) return 0;
  size_t day_z;
  return ac_layout(num_envs, n_steps, n_groups, width, n_layers, day_z).bytes;
}

// The handle first (a new export: its name is the first thing a caller learns), then w2a_surrogate_gradient_mlp_gated's
// checks in its order -- the struct, the schedule, obs and the outputs, the workspace pointer, the inputs and scalars, the
// handle's own, the workspace's size, the gate (only when one is given: allowed_days = NULL is the ungated call), the
// stream.
int w2a_actor_critic_mlp(w2a_env *env, const w2a_mlp_policy *net, const uint32_t *alert_mask, int32_t mask_words,
                         const float *env_weight, const float *advantage, int32_t advantage_days,
                         const float *value_target, int32_t value_target_days, const float *old_log_prob,
                         int32_t old_log_prob_days, double clip, double vf_coef, double entropy_coef, double gamma,
                         double lambda, int32_t bootstrap, int32_t n_steps, const float *obs, float *grad,
                         float *surrogate, float *value_loss, int32_t *clipped_days, float *approx_kl, float *entropy,
                         int32_t *days, float *ret, float *advantage_out, float *value_target_out, float *log_prob_out,
                         void *workspace, size_t workspace_bytes, void *stream, const uint32_t *allowed_days,
                         int32_t allowed_words) {
  const char *fn = "w2a_actor_critic_mlp";
  if (!env) return fail(W2A_ERR_ARG, "%s: NULL handle", fn);
  if (!net) return fail(W2A_ERR_ARG, "%s: NULL net (the two-row actor-critic network)", fn);
  W2A_CHECK(check_mlp_policy_struct(fn, net, n_steps, SAMPLE_0_OR_1));
  if (!alert_mask) return fail(W2A_ERR_ARG, "%s: NULL alert_mask (the schedule to follow)", fn);
  W2A_CHECK(check_obs(fn, obs));
  if (!surrogate || !value_loss || !clipped_days || !approx_kl || !entropy || !days)
    return fail(W2A_ERR_ARG, "%s: NULL surrogate, value_loss, clipped_days, approx_kl, entropy or days", fn);
  W2A_CHECK(check_workspace_pointer(fn, workspace));
  const bool epoch = advantage || value_target || old_log_prob;
  if (epoch) {
    if (!advantage || !value_target || !old_log_prob)
      return fail(W2A_ERR_ARG, "%s: advantage, value_target and old_log_prob come together (an epoch) or not at all", fn);
    if (advantage_days < n_steps) return fail(W2A_ERR_ARG, "%s: advantage holds fewer call-days than n_steps", fn);
    if (value_target_days < n_steps) return fail(W2A_ERR_ARG, "%s: value_target holds fewer call-days than n_steps", fn);
    if (old_log_prob_days < n_steps) return fail(W2A_ERR_ARG, "%s: old_log_prob holds fewer call-days than n_steps", fn);
    if (advantage_out || value_target_out || log_prob_out || ret)
      return fail(W2A_ERR_ARG, "%s: advantage_out, value_target_out, log_prob_out and ret are not formed in an epoch", fn);
    if (gamma != 1.0 || lambda != 1.0 || bootstrap)
      return fail(W2A_ERR_ARG, "%s: gamma, lambda and bootstrap have no meaning in an epoch", fn);
    if (!grad) return fail(W2A_ERR_ARG, "%s: NULL grad (only a collect call may leave the gradient out)", fn);
  } else {
    if (!advantage_out || !value_target_out || !log_prob_out || !ret)
      return fail(W2A_ERR_ARG, "%s: NULL advantage_out, value_target_out, log_prob_out or ret (a collect call)", fn);
    if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(W2A_ERR_ARG, "%s: gamma must lie in [0, 1]", fn);
    if (!(lambda >= 0.0 && lambda <= 1.0)) return fail(W2A_ERR_ARG, "%s: lambda must lie in [0, 1]", fn);
    if (bootstrap != 0 && bootstrap != 1) return fail(W2A_ERR_ARG, "%s: bootstrap must be 0 or 1", fn);
  }
  if (!isfinite(clip) || clip < 0.0) return fail(W2A_ERR_ARG, "%s: clip must be finite and not negative", fn);
  if (!isfinite(entropy_coef)) return fail(W2A_ERR_ARG, "%s: entropy_coef must be finite", fn);
  if (!isfinite(vf_coef) || vf_coef < 0.0) return fail(W2A_ERR_ARG, "%s: vf_coef must be finite and not negative", fn);
  W2A_CHECK(check_handle_common(fn, env, epoch ? FIXES_CHANGE_OBS : FIXES_CHANGE_OBS_AND_REWARD, MASK_SCHEDULE, mask_words));
  if ((int64_t)net->n_groups * W2A_MLP_HEADS_STRIDE((int64_t)net->width, net->n_layers) >= (1ll << 31))
    return fail(W2A_ERR_ARG, "%s: n_groups * block size must stay below 2^31 floats", fn);
  size_t day_z;
  const PgmLayout L = ac_layout(env->n, n_steps, net->n_groups, net->width, net->n_layers, day_z);
  if (workspace_bytes < L.bytes)
    return fail(W2A_ERR_ARG, "%s: workspace smaller than w2a_actor_critic_mlp_workspace_bytes", fn);
  if (allowed_days) W2A_CHECK(check_gate(fn, env, allowed_days, allowed_words));
  W2A_CHECK(refuse_while_capturing(fn, stream));
  AcMlpArgs xa;
  memset(&xa, 0, sizeof(xa));
  W2A_CHECK(fill_mlp(fn, env, net, n_steps, obs, allowed_days, allowed_days ? allowed_words : 0, xa.g.m));
  xa.g.m.stride = (int32_t)W2A_MLP_HEADS_STRIDE((int64_t)net->width, net->n_layers);  // below 2^31: checked above
  xa.g.m.r.pol.require_budget = net->require_budget;
  xa.g.m.r.order = mlp_own_order(net);
  bind_pgm_workspace(xa.g, L, workspace, grad);
  fill_surrogate(xa.ac.sg, alert_mask, mask_words, env_weight, advantage, old_log_prob, clip, entropy_coef, log_prob_out,
                 surrogate, clipped_days, approx_kl, entropy, days);
  xa.ac.value_target = value_target;
  xa.ac.vf_coef = vf_coef;
  xa.ac.gamma = gamma;
  xa.ac.gl = gamma * lambda;
  xa.ac.bootstrap = bootstrap;
  xa.ac.advantage_out = advantage_out;
  xa.ac.value_target_out = value_target_out;
  xa.ac.value_loss = value_loss;
  xa.ac.ret = ret;
  xa.ac.day_z = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + day_z);
  hipStream_t s = (hipStream_t)stream;
  if (!ensure_canonical(env, s, fn)) return W2A_ERR_STATE;
  W2A_CHECK(clear_day_rows(env, n_steps, advantage_out, s));
  W2A_CHECK(clear_day_rows(env, n_steps, value_target_out, s));
  W2A_CHECK(clear_day_rows(env, n_steps, log_prob_out, s));
  const unsigned g64 = grid64(env);
  dispatch_mlp_shape(net->width, net->n_layers,
                     [&](auto W, auto L_) { launch_ac<W(), L_()>(xa, epoch, grad != nullptr, g64, s); });
  HIP_TRY(hipGetLastError());
  end_call(env, s);
  return W2A_OK;
}

#undef W2A_CHECK
#endif  // W2A_POLICY_DISPATCH_HIP_H
