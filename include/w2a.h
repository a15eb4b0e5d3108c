/* w2a.h -- C ABI of the MI355X-native vectorised HeatAlertEnv hot path (libw2a.so).
 *
 * The reference (NSAPH-Projects/weather2alert) is pure Python and exposes no FFI; its
 * boundary for this path is the Gymnasium Env API of src/weather2alert/env.py. Each entry
 * point below names the reference lines it replaces. The Python host class
 * (weather2alert_amd/env.py) keeps the reference's ctor/reset/step surface and calls these
 * through ctypes with torch-ROCm tensor data_ptr()s; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer owned by the caller (PyTorch) unless marked host.
 *     The library allocates nothing on the device and frees nothing but the handle.
 *   - All calls are asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream). Three calls wait for the device: w2a_create (once per handle: it uploads the slot map and
 *     scans the tables on the NULL stream, then hipDeviceSynchronize), w2a_read_status (waits for `stream`
 *     only, to read the status word back) and w2a_hindsight_optimum (waits for `stream`: a slot-27 flag and a
 *     histogram of the budgets come to the host). Nothing else synchronises or allocates. What may be RECORDED into a
 *     hipGraph is w2a_step (w2a_state_bytes below says what a recording implies) and, while they need no
 *     conversion of the state's form, w2a_posterior_mean_reward / w2a_policy_actions / w2a_get_state; every
 *     other entry point that launches work fails with W2A_ERR_STATE while `stream` is capturing -- a replay
 *     would run it without the handle's bookkeeping (episode boundaries inside a graph: W2A_STEP_AUTORESET).
 *   - Return value: 0 = W2A_OK, negative = error (w2a_last_error() gives the text). Nothing
 *     throws across the ABI. Arguments are validated on the host before any launch; values
 *     that live in device arrays (episode tuples, actions) are range-checked inside the
 *     kernels, which clamp them and set a bit in the device status word instead of faulting.
 *   - A handle is not thread-safe; one handle per (process, device).
 */
#ifndef W2A_H
#define W2A_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define W2A_ABI_VERSION 18
#define W2A_ROW_FLOATS 32 /* floats per feature / weight row: one 128-B line */

enum {
  W2A_OK = 0,
  W2A_ERR_ARG = -1,      /* NULL pointer, non-positive size, bad enum */
  W2A_ERR_SCHEMA = -2,   /* table dims / slot layout the kernels cannot serve */
  W2A_ERR_HIP = -3,      /* a HIP runtime call failed */
  W2A_ERR_STATE = -4     /* state buffer too small / misaligned */
};

/* bits of the device status word (w2a_read_status) */
enum {
  W2A_ST_BAD_EPISODE = 1, /* reset tuple out of range (reference: KeyError env.py:127 / ValueError :121) */
  W2A_ST_BAD_ACTION = 2,  /* action not in {0,1} (reference action_space = Discrete(2), env.py:95) */
  W2A_ST_STEP_AFTER_DONE = 4, /* step() on a finished episode without autoreset */
  W2A_ST_STALE_GRAPH = 8  /* a replayed hipGraph holds a w2a_step on the packed lock-step form of the state, and that form
                             could not be kept current (the batch left lock step: a masked reset, a restored
                             checkpoint): the replayed step did NOTHING -- see w2a_state_bytes */
};

/* action buffer element types accepted by w2a_step */
enum { W2A_ACT_I32 = 0, W2A_ACT_I64 = 1, W2A_ACT_U8 = 2 };

/* w2a_step flags */
enum {
  W2A_STEP_AUTORESET = 1, /* same-step autoreset with the device RNG (needs w2a_set_autoreset): envs whose terminal step
                             has just run draw their next episode inside the step kernel and return its first
                             observation -- for batches that are not in lock step, and for loops recorded into a
                             hipGraph, where no reset can be launched between two steps (both step kernels serve it; a
                             batch that IS in lock step restarts together and stays on the packed form) */
  W2A_STEP_NO_OBS = 2,    /* reward-only: skip the observation write */
  W2A_STEP_CLASSIC = 8,   /* force the 4-lanes-per-env kernel where the 64-envs-per-wave one would be chosen (same
                             results up to the order of the fp64 additions; for A/B measurements and tests) */
  W2A_STEP_WIDE = 32,     /* force the 64-envs-per-wave kernel for small batches too (by default it serves batches of
                             >= 131 072 envs, the 4-lanes-per-env kernel smaller ones: the faster one on MI355X) */
  W2A_STEP_UNPACKED = 128, /* do not use the lock-step mirror of the per-env state (below; same results; for A/B
                             measurements and tests) */
  W2A_STEP_NEXT_STEP = 256, /* with W2A_STEP_AUTORESET: the restart happens on the call AFTER the terminal step (Gymnasium's
                             AutoresetMode.NEXT_STEP): the terminal step leaves the env finished with its stale
                             observation; the next call ignores that env's action, draws its next episode and returns
                             the episode's first observation with reward 0 and done 0 */
  W2A_STEP_NO_CAPTURE = 512, /* the caller drives episode boundaries from the host (it counts days and launches a reset
                             after the terminal step): such a loop cannot be recorded into a hipGraph -- a replay would
                             reset at a fixed position of the graph, or never -- so the call fails with W2A_ERR_STATE
                             while `stream` is capturing instead of recording a step (no cost otherwise: the capture
                             status is queried anyway) */
  W2A_STEP_SKIP_FINISHED = 64, /* with W2A_STEP_REWARD_GIVEN: envs whose episode is over are left untouched (reward
                             written as 0, done 1, state / return / observation unchanged, no status bit): policy
                             loops over batches that are not in lock step */
  W2A_STEP_REWARD_GIVEN = 16 /* `reward` is an INPUT: it already holds today's reward of every env
                             (w2a_posterior_mean_reward on the same state and actions); the step does everything
                             else of env.py:238-262 and accumulates that reward into the episode return */
};

/* budget sampling of reset(sample_budget=..., sample_budget_type=...), env.py:172-177 */
enum { W2A_BUDGET_FIXED = 0, W2A_BUDGET_LESS_THAN = 1, W2A_BUDGET_CENTERED = 2 };

/* Dense tables, compiled on the host by weather2alert_amd/tables.py.
 *
 * Replaces what HeatAlertEnv.__init__ builds (env.py:49-85): the merged (fips, year, date)
 * feature frame and the posterior coefficient tensors.
 *
 * Internal slot layout of a 32-float row (how lanes split a row is a kernel detail, not part of the ABI):
 *   slots  0..23  table-sourced columns (reward features first, in merged-column order)
 *   slots 24..27  run-time fields: alert_lag1, alert_streak, remaining_budget, alert_2wks(agent)
 *   slot   28     25th table-sourced column if the schema has one (else 0)
 *   slot   29     bias input (the table stores 1.0)
 *   slot   30     0/1 flag "heat_qi > 0.5" (the effectiveness gate of env.py:218, decided by the table
 *                 compiler on the file's float64 value), zero coefficient; kernels test it with > 0.5f
 *   slot   31     zero
 * W rows use the same slots (zero where a slot has no coefficient), so a reward logit is a
 * plain 32-wide dot product. obs_slot[j] maps observation column j (reference order,
 * env.py:186-195: the 28 episode columns then 'alert_2wks') to its slot.
 */
typedef struct w2a_tables {
  const float *X;                 /* [T][S_w*Y][32]  day-major feature rows            */
  const int32_t *n_days;          /* [S_w*Y]  episode length, 0 = (county, year) absent */
  const int32_t *B0;              /* [S_w*Y]  default budget = remaining_budget at day 0 (env.py:169) */
  const float *W;                 /* [S*n_samples][2][32]  head 0 baseline, 1 effectiveness */
  const int32_t *fips_to_weather; /* [S]  weight column -> county row of X, -1 = no weather */
  const int32_t *sim_cnt;         /* [S]  |similar(county) ∩ fips_list|  (env.py:115-117)  */
  int32_t T, S_w, Y, S, n_samples;
  int32_t n_obs;                  /* observation width (29 with the reference schema)    */
  int32_t obs_slot[W2A_ROW_FLOATS]; /* obs column -> slot, first n_obs entries valid       */
  int32_t slot_heat_qi;           /* slot of the 'heat_qi' feature (informational; the gate reads slot 30) */
  /* optional, for the corrected-semantics flags (w2a_set_semantics): */
  const int32_t *sim_ptr;         /* [S+1] CSR of similar(county) ∩ fips_list, confounders order (W2A_FIX_AUGMENT)     */
  const int32_t *sim_idx;         /* weight-column index of each similar county                                       */
  int32_t slot_alerts_2wks;       /* slot of the historical 'alerts_2wks' column, -1 = absent (W2A_FIX_ALERTS_2WKS)    */
  /* optional (NULL = off): the gate flags of slot 30 as a bitmap, [T][gate_words] uint32, bit (row & 31) of word
   * row >> 5 for row = county_w * Y + year_i. Lets the 64-envs-per-wave step kernel know in its first phase whether
   * the effectiveness row is needed at all (alert today AND heat_qi > 0.5, env.py:218-221) before any row is gathered */
  const uint32_t *gate_bits;
  int32_t gate_words;             /* words per day = ceil(S_w * Y / 32)                                               */
} w2a_tables;

typedef struct w2a_env w2a_env; /* opaque handle: pointers + dims only */

/* Decoded per-env state, for tests / checkpointing: every field is an int32 [num_envs]
 * device array supplied by the caller (NULL = skip). */
typedef struct w2a_state_view {
  int32_t *t, *used, *streak, *hist14, *last_actual, *at_budget, *budget, *n_days;
  int32_t *county_w, *year_i, *coef_col, *sample, *sticky_budget, *episode_no;
  int32_t *finished;     /* 1 once the terminal step of the current episode has run (done was returned) */
  float *episode_return; /* running return of the current episode */
} w2a_state_view;

int w2a_abi_version(void);
const char *w2a_last_error(void);

/* Bytes of caller-owned device memory one handle needs for `num_envs` envs (256-B aligned): 40 B per env of
 * canonical state (episode record, read-only step constants, counters + return) and a 16-B lock-step mirror (+ one day
 * word per 64 envs). While the handle knows the batch to be in lock step -- every env reset together by an unmasked
 * reset, one episode length for every (county, year), plain steps and rollouts since -- the day and the episode length
 * are the same for every env; the 64-envs-per-wave step kernel then streams 8 + 8 B of packed state per env in and 8 B
 * out instead of 12 + 12 and 12, with the day in the mirror's per-tile day word (needs T <= 255, S < 65536, n_samples
 * <= 1024, S_w * Y < 2^22 -- table properties; budgets may be anything: those the mirror's 16-bit field cannot hold are
 * read from the canonical words inside the kernel; other tables use the canonical arrays). The library converts between
 * the two forms by itself whenever an entry point needs the other one; a caller that rewrites the state buffer behind
 * the library's back (checkpoint restore) must call w2a_invalidate.
 * Stream capture. Every step kernel reads the day from device memory, so a w2a_step recorded into a hipGraph steps
 * correctly on every replay. What a recording fixes is the FORM of the state its kernel steps (no conversion between the
 * forms is ever recorded: w2a_step fails with W2A_ERR_STATE if the form its kernel needs is not current -- step once
 * eagerly, or call w2a_get_state, before capturing). From then on the handle keeps that form current at the end of
 * every call, so that a replay may come at any time:
 *   - recorded on the packed form (a lock-step batch of >= 131 072 envs, or W2A_STEP_WIDE, after one eager step): the
 *     mirror stays the primary form; calls that work on the canonical words (resets, rollouts, state reads) convert
 *     back before they return. Where the batch can no longer be packed (a masked reset, w2a_invalidate) the mirror is
 *     marked stale on the device and a replay of the recorded step does nothing but raise W2A_ST_STALE_GRAPH -- until
 *     the next whole-batch reset (of any kind: device RNG or the caller's tuples, with or without budgets) makes it
 *     packable again.
 *   - recorded on the canonical form: the handle never uses the packed form again.
 *   Replays advance days behind the host's back: a handle with a recorded step answers W2A_Q_LOCKSTEP_DAY with -1 (it
 *   still knows WHETHER the batch is in lock step, which is all the packed step and the matrix-core rollout need).
 *   Lock step survives a recorded W2A_STEP_AUTORESET step too (envs that are on one day finish, and restart, together:
 *   W2A_Q_LOCKSTEP stays 1 and the batch stays on the packed form); what such a handle never again reports valid is
 *   what belongs to particular EPISODES, which replays re-draw behind the host's back: the day, the column grouping
 *   (w2a_posterior_mean_reward), the tile list (w2a_rollout_mfma_prepare), the row counts of the visiting order.
 * The decisions are plain C++ in csrc/w2a_bookkeeping.h (run on the CPU under sanitizers, randomly and exhaustively, by
 * tests/test_bookkeeping_cpu.py). */
size_t w2a_state_bytes(int64_t num_envs);

/* Replaces HeatAlertEnv.__init__ (env.py:20-105) for `num_envs` envs whose global ids are
 * env_gid0 .. env_gid0+num_envs-1 (the device RNG is keyed by global id, so results do not
 * depend on how envs are sharded over GPUs). `tables` (host struct of device pointers) is
 * copied; `state` must stay alive until w2a_destroy. `status` is a caller-owned int32. */
int w2a_create(const w2a_tables *tables, int64_t num_envs, int64_t env_gid0, void *state, size_t state_bytes,
               int32_t *status, w2a_env **out);
void w2a_destroy(w2a_env *env);

/* Replaces reset() (env.py:133-184) with the episode tuples chosen by the caller (the host
 * replays NumPy's draws for seed parity, or injects them): per env the weather county row,
 * year index, coefficient column (env.py:117/121), posterior sample (env.py:160) and budget
 * (env.py:167-178). mask (uint8, nullable) selects which envs reset. Writes the first
 * observation rows into obs [num_envs][n_obs] (nullable). */
int w2a_reset(w2a_env *env, const int32_t *county_w, const int32_t *year_i, const int32_t *coef_col,
              const int32_t *sample, const int32_t *budget, const uint8_t *mask, float *obs, void *stream);

/* reset() with every draw of env.py:145-177 made on the device from a counter-based RNG keyed
 * by (seed, global env id, per-env episode number). location < 0 draws the county
 * (env.py:151-152), otherwise it is the weight-column index of the requested county.
 * budget_kw < 0 means "budget=None". Budget stickiness (env.py:167-170) is kept per env
 * unless `sticky` is 0. restart_episodes != 0: the (selected) envs' episode counters restart at 0, so a
 * reset with an explicit seed reproduces the same episodes every time (env.py:143-145 re-creates the
 * Generator from the seed); 0: the counters advance, which is what an autoreset does. */
int w2a_reset_device_rng(w2a_env *env, uint64_t seed, int32_t location, int augment, int32_t budget_kw,
                         int sample_budget_mode, int sticky, int restart_episodes, const uint8_t *mask, float *obs,
                         void *stream);

/* Parameters the same-step autoreset of w2a_step uses (same meaning as above). They travel to the step kernels as
 * arguments: a w2a_step recorded into a hipGraph keeps the parameters it was recorded with. */
int w2a_set_autoreset(w2a_env *env, uint64_t seed, int32_t location, int augment, int32_t budget_kw,
                      int sample_budget_mode, int sticky);

/* Replaces step() (env.py:238-262) for all envs: budget gate, history update, feature-row
 * gather, the two 28-term logits against the env's posterior draw, reward, termination, and
 * the next observation. actions: [num_envs] of `action_dtype`. obs [num_envs][n_obs] f32,
 * reward [num_envs] f32, done [num_envs] uint8. On a terminal step without autoreset the
 * obs rows are left untouched (the reference returns the stale observation, env.py:257-262);
 * with autoreset they hold the new episode's first observation and last_return (nullable,
 * f32 [num_envs]) receives the finished episode's return. */
int w2a_step(w2a_env *env, const void *actions, int action_dtype, float *obs, float *reward, uint8_t *done,
             float *last_return, int flags, void *stream);

/* episode_order="sorted" (no reference counterpart; opt-in): after a reset, relabel the envs so that env
 * indices follow the coefficient row (column, draw); envs of one row keep their order (a stable sort). The
 * multiset of episodes is unchanged -- only which env index holds which episode -- but neighbouring envs now
 * share table lines, which the step kernel's gathers turn into L2 hits. The whole per-env record moves
 * (episode tuple, budget, sticky budget, episode number).
 * workspace: caller-owned, w2a_sort_workspace_bytes(num_envs) bytes, 256-B aligned. */
size_t w2a_sort_workspace_bytes(int64_t num_envs);
int w2a_sort_episodes(w2a_env *env, void *workspace, size_t workspace_bytes, void *stream);
/* The same relabelling fused into the whole-batch device-RNG reset that precedes it (what episode_order="sorted" does once
 * per episode): w2a_reset_device_rng + w2a_sort_episodes + w2a_observe in three launches and no moved record. Pass 1 draws
 * every env's next episode and keeps only its sort key -- the coefficient row (column, draw) -- with the env's sticky
 * budget and episode number; a stable radix sort of (key, env index); pass 2 is k_reset with "index e receives the
 * episode env src[e] draws" (same global id, sticky budget and episode number as that env's own draw: the result is bit
 * for bit that of the three calls above) and writes state and first observations (obs nullable) in place.
 * Arguments as w2a_reset_device_rng without a mask; workspace as w2a_sort_episodes. Returns 1 (nothing done) when the key
 * does not fit 32 bits (S * n_samples > 2^32): the caller runs the three calls instead. */
int w2a_reset_device_rng_sorted(w2a_env *env, uint64_t seed, int32_t location, int augment, int32_t budget_kw,
                                int sample_budget_mode, int sticky, int restart_episodes, float *obs, void *workspace,
                                size_t workspace_bytes, void *stream);

/* reward_mode = "posterior_mean" (the legacy env's eval mode, _deprecated/env.py:332-342: `posterior_indices =
 * np.arange(n_posterior_samples) if eval_mode`, `np.mean([_get_reward(i, ...)])`, on today's reward form
 * env.py:197-226): the reward of every env is the mean over ALL posterior draws of its coefficient column
 * instead of the one draw of the episode. One grouped fp64 contraction per step: per column
 * [envs x 32 slots] * [32 slots x 2 heads x n_samples draws], sigmoid / gate / mean epilogue.
 *   w2a_group_by_column        after EVERY reset -- and after anything else that changes which episode an env index
 *                              holds: w2a_sort_episodes, a w2a_step with W2A_STEP_AUTORESET (both mark the grouping
 *                              stale, and w2a_posterior_mean_reward then refuses to run) --: sorts the env ids by coefficient column into `workspace`
 *                              (caller-owned, w2a_group_workspace_bytes(num_envs, S, n_samples), 256-B aligned, must
 *                              stay alive while w2a_posterior_mean_reward is used) and writes a pre-scaled fp64 copy
 *                              of W there. W rows that give slot 28, 30 or 31 a coefficient are honoured (w2a_create
 *                              scans for them once) at the price of a wider contraction;
 *   w2a_posterior_mean_reward  before w2a_step(..., W2A_STEP_REWARD_GIVEN) with the SAME actions: writes
 *                              reward [num_envs] f32 from the pre-step state. Same budget gate as the step
 *                              (env.py:242-246): an alert attempted at budget counts as no alert. */
/*   w2a_set_posterior_kernel   which kernel computes the contraction (same results to ~1e-7; speed differs):
 *                              W2A_PM_VECTOR (default) fp64 FMAs on the vector ALU with DPP-broadcast coefficients,
 *                              W2A_PM_MATRIX_F64 the fp64 matrix-core form (v_mfma_f64_16x16x4_f64; on MI355X the fp64
 *                              matrix rate equals the fp64 vector rate, so it is the slower of the two),
 *                              W2A_PM_MATRIX_I8 the int8 matrix-core form (v_mfma_i32_16x16x64_i8 on exact fixed-point
 *                              digits of both operands, int32 accumulation; logits within ~2e-6 by an a-priori bound,
 *                              columns outside the fixed-point range take an exact fp64 path inside the kernel).
 *                              The choice also decides whether w2a_rollout_posterior_mean's one-launch kernel applies
 *                              (it is built on the vector form). */
enum { W2A_PM_VECTOR = 0, W2A_PM_MATRIX_F64 = 1, W2A_PM_MATRIX_I8 = 2 };
int w2a_set_posterior_kernel(w2a_env *env, int kernel);
size_t w2a_group_workspace_bytes(int64_t num_envs, int32_t S, int32_t n_samples);
int w2a_group_by_column(w2a_env *env, void *workspace, size_t workspace_bytes, void *stream);
int w2a_posterior_mean_reward(w2a_env *env, const void *actions, int action_dtype, float *reward, void *stream);

/* First observation (env.py:181) of every env from its packed state; valid right after a reset
 * (t == 0 for every env, else W2A_ST_STEP_AFTER_DONE is raised). Used after w2a_sort_episodes. */
int w2a_observe(w2a_env *env, float *obs, void *stream);

/* Opt-in corrections of reference quirks. Default 0 = faithful to env.py, which is
 * what every parity claim refers to; each bit is independent:
 *   ALERTS_2WKS (Q1) the agent's 14-day alert count replaces the historical 'alerts_2wks' column (env.py:191
 *                    writes it to a new key instead), so it reaches the reward through that coefficient
 *   LAG         (Q3) alert_lag1 is yesterday's actual action (env.py:190 reads the buffer after today's append)
 *   PENALTY     (Q5) an alert attempted at budget costs reward -1 (env.py:223-224 is dead code)
 *   OBS         (Q6) step() returns the row of the next day with the updated state (env.py:257-259 returns the
 *                    current day's row and a stale row on the terminal step)
 *   AUGMENT     (Q8) similar_climate_counties uses the drawn county's weather and its true coefficient column
 *                    (env.py:116-127 indexes the filtered list and keeps the requested county's weather);
 *                    applies to device-RNG resets, host-tuple resets pass what they want
 *   (Q9, per-episode budgets, is the `sticky = 0` argument of the reset entry points.) */
enum { W2A_FIX_ALERTS_2WKS = 1, W2A_FIX_LAG = 2, W2A_FIX_PENALTY = 4, W2A_FIX_OBS = 8, W2A_FIX_AUGMENT = 16,
       W2A_FIX_ALL = 31 };
int w2a_set_semantics(w2a_env *env, uint32_t fixes);

/* On-device policy rollout (replaces a Python loop of `action = policy(obs); env.step(action)`
 * such as env.py:265-277): every env runs up to n_steps days, or to the end of its episode, inside one launch
 * with its coefficient rows held in registers. The policy sees what the reference's agent would see before
 * acting on day t: the lagging observation (row of day t-1), the remaining budget and the day. */
enum { W2A_POLICY_NEVER = 0, W2A_POLICY_ALWAYS = 1, W2A_POLICY_BERNOULLI = 2, W2A_POLICY_THRESHOLD = 3,
       W2A_POLICY_TABLE = 4 };
typedef struct w2a_policy {
  int32_t kind;
  float p;                /* BERNOULLI: P(alert); drawn from the counter RNG keyed (seed, env id, episode, day) */
  int32_t obs_col;        /* THRESHOLD: observation column (reference order) of a table-sourced feature ...      */
  float threshold;        /* ... alert iff obs[obs_col] > threshold                                              */
  int32_t obs_lag;        /* THRESHOLD: 1 = the agent sees yesterday's row (faithful, Q6); 0 = today's row        */
  int32_t require_budget; /* 1: never attempt an alert with remaining_budget <= 0                                */
  const uint8_t *table;   /* TABLE: device uint8 [T][table_R], action = table[day][min(remaining_budget, R-1)]   */
  int32_t table_R;
  uint64_t seed;
} w2a_policy;
/* Outputs (device, nullable): ret_out f32 [n] rewards summed over the days run by this call, alerts_out i32 [n]
 * alerts issued, attempts_over_budget i32 [n] alerts attempted at budget (silently dropped, Q5), alert_mask /
 * attempt_mask u32 [n][mask_words] bit d = alert issued / attempted on day d (the reference's actual_ and
 * attempted_alert_buffer, env.py:239,248), last_return f32 [n] episode return of envs that finished,
 * ret_snapshot f32 [n] the running episode return after the step that leaves t == n_days - 2, the moment the
 * reference's logging callbacks read the env (callbacks.py:47-48,128-132; untouched if that step is not in this call). */
int w2a_rollout(w2a_env *env, const w2a_policy *policy, int32_t n_steps, float *ret_out, int32_t *alerts_out,
                int32_t *attempts_over_budget, uint32_t *alert_mask, uint32_t *attempt_mask, int32_t mask_words,
                float *last_return, float *ret_snapshot, void *stream);
/* w2a_rollout with a linear-logistic policy that has one parameter row per group of envs (policy search: many candidate
 * parameter vectors, each scored on the envs of its group). Env i acts on
 *     logit = weight[g] . obs_i + bias[g],   g = group[i],
 * where obs_i is exactly the row w2a_step would have returned to the agent before that decision: the lagging
 * observation with the faithful run-time columns (alert_lag1, the pre-update alert_streak,
 * remaining_budget, alert_2wks). The logit is accumulated in fp64 over the f32 inputs and parameters: bias first, then
 * the observation columns in slot order. sample = 0: alert iff logit > 0; sample = 1: alert iff u < sigmoid(logit),
 * u the BERNOULLI policy's uniform of (seed, global env id, episode number, day). require_budget as in w2a_policy.
 *   weight  device f32 [n_groups][32], 16-B aligned, in SLOT order: observation column j's coefficient at
 *           slot obs_slot[j] of w2a_tables; the other slots are ignored
 *   bias    device f32 [n_groups]
 *   group   device i32 [num_envs] in [0, n_groups) (NULL = group 0 for every env); the caller checks the range --
 *           the kernel clamps ids into it and never reads outside weight / bias
 * obs (device f32 [num_envs][n_obs], in/out) is the observation buffer of w2a_reset / w2a_step: on entry it must hold
 * the row every env's agent holds (the first day's input -- the state alone cannot rebuild it); on return it holds the
 * row each env holds after this call (a terminal day leaves the previous row, like w2a_step), so calls chain with each
 * other and with w2a_step. n_steps, outputs and lock-step bookkeeping are those of w2a_rollout (no in-call autoreset).
 * Refused (W2A_ERR_ARG) on a handle with corrected-semantics flags (they change what the observation is). */
typedef struct w2a_linear_policy {
  const float *weight;
  const float *bias;
  const int32_t *group;
  int32_t n_groups;
  int32_t sample;         /* 0 or 1 */
  int32_t require_budget; /* 0 or 1 */
  uint64_t seed;          /* sample = 1 only */
} w2a_linear_policy;
int w2a_rollout_linear(w2a_env *env, const w2a_linear_policy *policy, int32_t n_steps, float *obs, float *ret_out,
                       int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask, uint32_t *attempt_mask,
                       int32_t mask_words, float *last_return, float *ret_snapshot, void *stream);
/* w2a_rollout_linear with a small multilayer perceptron instead of the linear logit, one parameter block per group:
 *     h1 = act(W1 . obs_i + b1),  [h2 = act(W2 . h1 + b2),]  logit = w_out . h_last + b_out,   g = group[i],
 * on the same faithful observation row obs_i, with the same decisions (sample = 0: alert iff logit > 0; sample = 1:
 * alert iff u < sigmoid(logit), the same uniform u), require_budget, obs buffer, outputs and bookkeeping.
 * Numerics: parameters and activations are f32; every layer's pre-activation is an f32 sum of f32 products, bias
 * first; tanh (within ~2e-7 absolute of the exact value over all f32) and ReLU in f32; the logit is f32. A decision
 * can therefore differ from an fp64 evaluation of the same network only at a near-tie: |logit| <= 1e-4 (|b_out| +
 * sum_h |w_out,h h_h|), or with sample = 1, |sigmoid(logit) - u| <= 1e-5. An env's result does not depend on which
 * other envs share its wave, on the group layout or on the visiting order (bit for bit).
 *   params  device f32, 16-B aligned: n_groups blocks of W2A_MLP_STRIDE(width, n_layers) floats, each
 *             W1[32][width]     row obs_slot[j] (w2a_tables) holds observation column j; rows of other slots are zero
 *             b1[width]
 *             W2[width][width]  b2[width]   (n_layers == 2 only; W2[k][u]: input unit k, output unit u)
 *             w_out[width]
 *             b_out, 0, 0, 0
 *           every part zero-padded to width (units past a layer's real width have zero weights and bias); a two-row
 *           output (SB3's two action values) is folded by the caller into w_out = row1 - row0, b_out = b1 - b0
 *   group   device i32 [num_envs] in [0, n_groups) (NULL = group 0 for every env); the kernel clamps, never reads
 *           outside params
 *   order   device i32 [num_envs], a permutation of the env ids: the visiting order (NULL = the handle's rollout
 *           order, or identity). Speed only: a stable sort by group puts each group's envs in whole waves.
 *   width   padded hidden width of every hidden layer: 16, 32 or 64;  n_layers: 1 or 2 hidden layers
 *   activation  W2A_MLP_TANH or W2A_MLP_RELU, after every hidden layer (none after the output)
 * Refused (W2A_ERR_ARG) where w2a_rollout_linear is, and for a bad width, n_layers, activation, sample or alignment. */
enum { W2A_MLP_TANH = 0, W2A_MLP_RELU = 1 };
#define W2A_MLP_STRIDE(width, n_layers) \
  (W2A_ROW_FLOATS * (width) + (width) + ((n_layers) == 2 ? (width) * (width) + (width) : 0) + (width) + 4)
/* The two-head layout of the same block, read by w2a_q_gradient_mlp alone (a Q-net with one output row per action;
 * every other entry point takes the layout above): everything up to and including b2 (b1 with one hidden layer) is
 * unchanged, and the tail  w_out[width], b_out, 0, 0, 0  becomes
 *             w_out0[width]     Q(o, 0): no alert
 *             w_out1[width]     Q(o, 1): alert
 *             b_out0, b_out1, 0, 0
 * W2A_MLP_HEADS_STRIDE = W2A_MLP_STRIDE + width floats per block: rows stay 16-B aligned. The struct is the same
 * w2a_mlp_policy; which layout `params` holds is decided by the entry point it is passed to. */
#define W2A_MLP_HEADS_STRIDE(width, n_layers) (W2A_MLP_STRIDE(width, n_layers) + (width))
typedef struct w2a_mlp_policy {
  const float *params;
  const int32_t *group;
  const int32_t *order;
  int32_t n_groups;
  int32_t n_layers;       /* 1 or 2 */
  int32_t width;          /* 16, 32 or 64 */
  int32_t activation;     /* W2A_MLP_TANH 0 or W2A_MLP_RELU 1 */
  int32_t sample;         /* 0 or 1 */
  int32_t require_budget; /* 0 or 1 */
  uint64_t seed;          /* sample = 1 only */
} w2a_mlp_policy;
int w2a_rollout_mlp(w2a_env *env, const w2a_mlp_policy *policy, int32_t n_steps, float *obs, float *ret_out,
                    int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask, uint32_t *attempt_mask,
                    int32_t mask_words, float *last_return, float *ret_snapshot, void *stream);
/* w2a_rollout_linear / w2a_rollout_mlp that also record the per-day trajectory (on-policy training data). Arguments,
 * results and refusals are those of the plain forms, which the recording changes in no bit; in addition
 * W2A_ERR_ARG for a NULL traj or a NULL member pointer (checked on the host, before the handle). Every array is
 * device memory indexed [call-day s][env id] (n = num_envs, n_obs of w2a_tables), s = 0 .. n_steps - 1:
 *   obs     f32 [n_steps + 1][n][n_obs], 4-B aligned: slab s is the row the agent held before decision s (exactly what
 *           w2a_step would have returned); slab 0 is the obs buffer on entry, for every env; slab s + 1 after a
 *           terminal step repeats slab s (the terminal step leaves the previous row); slab n_steps is, for every env,
 *           the obs buffer when the call returns -- the bootstrap row of a truncated chunk. Rows past an env's
 *           terminal day, other than slab n_steps, are unspecified.
 *   logit   f32 [n_steps][n]: the logit decision s was taken on (linear: the fp64 logit rounded to f32; mlp: the f32
 *           logit, row1 - row0 for a two-row output)
 *   reward  f32 [n_steps][n]: the reward w2a_step returns for that day
 *   action  u8  [n_steps][n]: the action passed to the env (the policy's decision after require_budget)
 *   flags   u8  [n_steps][n]: W2A_TRAJ_VALID (the env took a step on call-day s) | W2A_TRAJ_TERMINATED (that step ended
 *           its episode) | W2A_TRAJ_ALERT (an alert was issued: an attempt with no budget left is none). The library
 *           zeroes flags on the stream first, so entries the env did not step hold 0; their logit, reward, action are
 *           left unwritten. A recorded call visits the envs in identity order where it can (speed only).
 * Bytes per env-day: 4 n_obs + 10 (126 on the default schema). */
enum { W2A_TRAJ_VALID = 1, W2A_TRAJ_TERMINATED = 2, W2A_TRAJ_ALERT = 4 };
typedef struct w2a_trajectory {
  float *obs;      /* [n_steps + 1][n][n_obs] */
  float *logit;    /* [n_steps][n] */
  float *reward;   /* [n_steps][n] */
  uint8_t *action; /* [n_steps][n] */
  uint8_t *flags;  /* [n_steps][n] */
} w2a_trajectory;
int w2a_rollout_linear_record(w2a_env *env, const w2a_linear_policy *policy, int32_t n_steps, float *obs,
                              float *ret_out, int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask,
                              uint32_t *attempt_mask, int32_t mask_words, float *last_return, float *ret_snapshot,
                              void *stream, const w2a_trajectory *traj);
int w2a_rollout_mlp_record(w2a_env *env, const w2a_mlp_policy *policy, int32_t n_steps, float *obs, float *ret_out,
                           int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask,
                           uint32_t *attempt_mask, int32_t mask_words, float *last_return, float *ret_snapshot,
                           void *stream, const w2a_trajectory *traj);
/* The returns of a stretch of days under EVERY posterior draw of each env's coefficient column. The trajectory does not
 * depend on the draw (the state update reads only the actions and the alert buffers; the draw enters only the reward,
 * env.py:197-226), so the state at the start of the stretch and the bitmap of the alerts issued in it fix every day's
 * input vector, and
 *     out[e][k] = sum over the days env e ran of reward(x_t, a_t; W[coef_col[e] * n_samples + k]),  k < n_samples,
 * summed in f32 in day order. Draw k is a joint posterior sample over all counties: the mean over a set of envs of
 * out[.][k] is one posterior sample of the mean return.
 *   start       device i32 arrays of the state BEFORE the stretch, as w2a_get_state decodes it; read: t, used, streak,
 *               hist14, budget, n_days, county_w, year_i, coef_col, finished (the others may be NULL)
 *   alert_mask  device u32 [num_envs][mask_words], bit d = an alert was issued on day d (the alert_mask output of the
 *               rollout that ran the stretch, the reference's actual_alert_buffer); mask_words * 32 >= T
 *   n_steps     days of the stretch: each env runs from its start day t for at most n_steps days, stopping after its
 *               terminal day; envs finished on entry get a row of zeros
 *   out         device f32 [num_envs][n_samples]
 * Numerics contract: every day rebuilds the 32-slot vector exactly as the rollout kernels do (the table row of day t,
 * the faithful run-time fields: alert_lag1, the pre-update alert_streak, remaining_budget, alert_2wks from the bitmap)
 * and evaluates both logits as fp64 FMA chains over slots 0..29 in slot order, the heat gate, the f32 sigmoids and the
 * reward of w2a_step. Hence column sample_e (the env's own draw) is BIT-IDENTICAL to the ret_out of the rollout that
 * produced the bitmap for the fp64-chain kernels (k_rollout64, k_rollout_linear, k_rollout_mlp: w2a_rollout with a
 * visiting order and no matrix-core prepare, w2a_rollout_linear, w2a_rollout_mlp), and within 2e-6 relative of it for
 * k_rollout_mfma (int8 digits of the table-sourced terms); every column is within the reward bars (1e-5 per day) of an
 * fp64 restatement. A start state outside the tables (no reset produces one) gives NaN rows.
 * Reads the tables and the caller's arrays only: the handle's state and bookkeeping are untouched. W2A_ERR_ARG for NULL
 * pointers, n_steps <= 0, mask_words <= 0 (checked on the host, before the handle), mask_words * 32 < T, and on a handle
 * with corrected-semantics flags (the reward then depends on attempts and on other table rows); W2A_ERR_STATE while
 * `stream` is recording a hipGraph. */
int w2a_posterior_returns(w2a_env *env, const w2a_state_view *start, const uint32_t *alert_mask, int32_t mask_words,
                          int32_t n_steps, float *out, void *stream);
/* The hindsight optimum: every env's best alert schedule for a stretch of days, knowing the whole stretch's weather,
 * its own posterior draw and its remaining budget -- the upper bound against which a policy's return reads as regret.
 * Under the faithful semantics the reward of a day depends on the agent only through four run-time slots: 24
 * alert_lag1 (today's alert, 0 on day 0), 25 the streak before today's update, 26 budget - used after today's alert, 27
 * the agent's 14-day count, whose coefficient is zero (the reference's weights key the historical alerts_2wks). So
 * with j = alerts issued in the stretch and s = the current streak, a finite-horizon DP over (j, s) is exact:
 *     V_d(j, s) = max( r0 + V_{d+1}(j, 0),  r1 + V_{d+1}(j + 1, s + 1) ),  V_H = 0,
 * the alert allowed only while used + j < budget (an attempt at the budget is a no-op), values fp64 sums of the f32
 * rewards, an alert taken only if STRICTLY better (ties do not alert); the schedule is backtracked from (0, streak).
 * Each env runs from its start day t for H = min(n_steps, n_days - t) days, stopping after its terminal day (the
 * convention of w2a_posterior_returns); U = min(budget - used, H) bounds j, (U + 1)(U + 4) / 2 states per day.
 *   start       device i32 arrays of the state at the start, as w2a_get_state decodes it; read: t, used, streak, budget,
 *               n_days, county_w, year_i, coef_col, sample, finished (the others may be NULL)
 *   n_steps     days of the stretch (> 0)
 *   ret_out     device f32 [num_envs]: the return of the schedule
 *   alert_mask  device u32 [num_envs][mask_words], bit d = alert on day d of the episode (as w2a_rollout's alert_mask;
 *               only days t .. t + H - 1 can be set); mask_words * 32 >= T
 *   alerts_out  device i32 [num_envs]: alerts in the schedule (<= budget - used)
 *   workspace   device memory of workspace_bytes >= w2a_hindsight_workspace_bytes(env, n_steps, max_remaining, 1)
 *               bytes, 256-B aligned, max_remaining >= max(budget - used) over the envs of `start`: 8 B per env of
 *               scratch, and a pool only if that budget's DP does not fit in LDS (budgets far beyond the tables'
 *               defaults; about U^2 x 10 B per env at a remaining budget U); `big_envs` sizes the pool for that many
 *               such envs per launch (speed only)
 * Envs finished on entry (or with t >= n_days) get 0, an empty bitmap and 0 alerts; a start state outside the tables
 * (no reset produces one) gives NaN, an empty bitmap and 0.
 * Numerics contract: every reward the DP weighs is bit-identical to the one the env pays on that day in that state (the
 * fp64 FMA chain of the step and rollout kernels over slots 0..23 once per env-day, continued per state over slots 24,
 * 25, 26, 28, 29 in slot order, the heat gate, reward_from_logits), and ret_out re-adds the chosen rewards in f32 in day
 * order: it is BIT-IDENTICAL to column `sample` of w2a_posterior_returns(start, alert_mask) and so to what a
 * fp64-chain rollout replaying the schedule returns.
 * Synchronises `stream` (one histogram of U comes to the host to size and bin the launches) and returns after the
 * work is done. Reads the tables and the caller's arrays only: the handle's state and bookkeeping are untouched.
 * W2A_ERR_ARG for NULL pointers, n_steps <= 0, mask_words <= 0 (checked on the host, before the handle), mask_words * 32
 * < T, a handle with corrected-semantics flags, tables where some coefficient row has a nonzero slot-27 term (one
 * scan of W per call), and a workspace too small for the batch; every refusal comes before any output is written.
 * W2A_ERR_STATE while `stream` is recording a hipGraph. */
size_t w2a_hindsight_workspace_bytes(const w2a_env *env, int32_t n_steps, int32_t max_remaining, int32_t big_envs);
int w2a_hindsight_optimum(w2a_env *env, const w2a_state_view *start, int32_t n_steps, float *ret_out,
                          uint32_t *alert_mask, int32_t mask_words, int32_t *alerts_out, void *workspace,
                          size_t workspace_bytes, void *stream);
/* The score-function (REINFORCE) gradient, with reward-to-go, of the rollout that w2a_rollout_linear(env, policy,
 * n_steps, obs, ...) with sample = 1 would run from the handle's CURRENT state and observation rows: call it right
 * before that rollout, with the same policy, n_steps and obs. It reads the state, the tables and obs and modifies none of
 * them, nor the handle's bookkeeping beyond making the canonical state words current (which the rollout does anyway).
 * The estimator, for env e of group g over the call-days s = 0 .. S_e - 1 on which the env takes a step:
 *   o_s      the observation row the agent holds before decision s (slab s of w2a_rollout_linear_record)
 *   z_s      = weight[g] . o_s + bias[g], the fp64 logit of that decision;  p_s = sigmoid(z_s) in f32, as the rollout's
 *   a_s      the policy's own draw, u < p_s
 *   m_s      0 on a day where require_budget forced the action to 0 because no budget was left (the action is off the
 *            policy's distribution there), else 1; without require_budget an attempt at the budget counts (m_s = 1)
 *   delta_s  = m_s (a_s - p_s): d log pi(a_s | o_s) / d z_s
 *   A_s      = r_s - beta_s, r_s the reward w2a_step returns for that day; beta_s = 0 (W2A_PG_BASELINE_NONE) or
 *            (W2A_PG_BASELINE_NO_ALERT) the reward the same env would have been paid on that day had no alert been
 *            issued from the call's first day on, starting from the call's start state: alert_lag1 = 0, the streak of
 *            the start state on the first day and 0 after it, the 14-day window decaying, the remaining budget frozen
 *            at its start value. It depends on nothing the policy does inside the call, so it is a valid baseline for
 *            every earlier score. ("Today's reward without today's alert" would not be: today's state depends on
 *            earlier actions.)
 *   Q_s      = sum over s' >= s of A_s': undiscounted reward-to-go over the env's days of THIS call -- a chunk that
 *            ends before the episode does is truncated, nothing is bootstrapped past its last day
 *   g_e      = sum_s delta_s Q_s (o_s, 1);  envs finished on entry get a row of zeros
 * grad (device f32 [n_obs + 1][num_envs], column-major: component j of env e at j * num_envs + e) receives g_e: the
 * weight columns in OBSERVATION order, the bias last. The mean of g_e over a group's envs estimates the gradient of that
 * group's mean return with respect to its parameter row.
 * Numerics contract: u, z_s, p_s and r_s are computed by the statements of k_rollout_linear (same uniform, same fp64 FMA
 * chains: bias first, slots 0..29 in slot order; same f32 sigmoids; reward_from_logits), so they are the values the
 * rollout then uses; beta_s continues the baseline chain of the played day after slot 23 over the fork's slots 24..29
 * and goes through reward_from_logits; delta_s and A_s are f32, Q_s and the sums over s fp64, g_e rounded to f32 once.
 * An env's g_e does not depend on the other envs, the group layout or the visiting order (bit for bit): reduce them
 * over groups in any fixed order for a deterministic gradient.
 *   baseline    W2A_PG_BASELINE_NONE or W2A_PG_BASELINE_NO_ALERT
 *   workspace   device memory of w2a_policy_gradient_workspace_bytes(num_envs, n_steps) bytes, 256-B aligned: 9 B per
 *               env-day (delta_s, A_s and the alert issued); no observation row is written or read per day
 * W2A_ERR_ARG where w2a_rollout_linear refuses (checked in the same order), for sample != 1, an unknown baseline, a NULL
 * grad or workspace and a workspace too small or misaligned; W2A_ERR_STATE while `stream` is recording a hipGraph. */
enum { W2A_PG_BASELINE_NONE = 0, W2A_PG_BASELINE_NO_ALERT = 1 };
size_t w2a_policy_gradient_workspace_bytes(int64_t num_envs, int32_t n_steps);
int w2a_policy_gradient_linear(w2a_env *env, const w2a_linear_policy *policy, int32_t baseline, int32_t n_steps,
                               const float *obs, float *grad, void *workspace, size_t workspace_bytes, void *stream);
/* The same estimator for w2a_rollout_mlp(env, policy, n_steps, obs, ...) with sample = 1, already reduced per group:
 * z_s is the f32 logit k_rollout_mlp computes for o_s (the same bits: pass 1 is that kernel's day loop), dz_s/dtheta the
 * backward pass of the f32 network (the ReLU derivative is 0 at a pre-activation of exactly 0), delta_s, A_s, Q_s and the
 * baselines as above, and
 *     grad[g] = (1 / N_g) sum over the envs e of group g of  sum_s delta_s Q_s dz_s/dtheta(theta_g),
 * N_g the number of envs of group g (envs finished on entry contribute zero and count; a group without envs gives a
 * block of NaN). Call it right before that rollout, with the same policy, n_steps and obs; it reads the state, the tables
 * and obs and modifies none of them, nor the handle's bookkeeping beyond making the canonical state words current.
 *   grad        device f32 [n_groups][W2A_MLP_STRIDE(width, n_layers)]: every block in the layout of `params` (rows of
 *               W1 on non-observation slots, padding units and the three trailing floats are zero)
 *   policy->order  the visiting order of THESE kernels (they write no state, so it need not be the rollout's): pass the
 *               env ids stably sorted by group (NULL = identity order: right for n_groups == 1). The workspace holds one
 *               partial block per wave and one per group boundary of a group-major order; an order that changes group
 *               more often than that runs out of blocks, and grad is then filled with NaN.
 *   workspace   device memory of w2a_policy_gradient_mlp_workspace_bytes(...) bytes, 256-B aligned: 9 B per env-day and
 *               12 B per env of scratch, and the partial blocks (fp64 [stride] each)
 * Numerics contract: u, z_s, p_s, r_s and beta_s are computed by the statements of k_rollout_mlp and of
 * w2a_policy_gradient_linear's fork; delta_s and A_s are f32, Q_s fp64, c_s = delta_s Q_s rounded to f32; the forward
 * recomputation, the backward pass and the sums over the days of one 64-env tile are f32 (matrix-core accumulators);
 * the tiles' sums are added in fp64 in a fixed order and the mean is rounded to f32 once. No atomics: two identical
 * calls give identical bits. The partial sums (not the estimator) depend on the visiting order.
 * W2A_ERR_ARG where w2a_rollout_mlp refuses (checked in the same order), for sample != 1, an unknown baseline, a NULL
 * grad or workspace and a workspace too small or misaligned; W2A_ERR_STATE while `stream` is recording a hipGraph. */
size_t w2a_policy_gradient_mlp_workspace_bytes(int64_t num_envs, int32_t n_steps, int32_t n_groups, int32_t width,
                                               int32_t n_layers);
int w2a_policy_gradient_mlp(w2a_env *env, const w2a_mlp_policy *policy, int32_t baseline, int32_t n_steps,
                            const float *obs, float *grad, void *workspace, size_t workspace_bytes, void *stream);
/* The gradient of the log-likelihood of a GIVEN alert schedule under a linear policy (teacher forcing): the supervised
 * counterpart of w2a_policy_gradient_linear. Every env is forced along its own schedule from the handle's CURRENT state
 * and observation rows, and the policy is evaluated on the rows it would have held. It reads the state, the tables, the
 * schedule and obs and modifies none of them, nor the RNG, nor the handle's bookkeeping beyond making the canonical state
 * words current: epochs over the same episodes need no reset in between.
 * The estimator, for env e of group g over the call-days s = 0 .. S_e - 1 on which the env takes a step (at most n_steps,
 * and none after its terminal day):
 *   a*_s     bit (t & 31) of alert_mask[e][t >> 5], t the env's day of the episode: the action ATTEMPTED. The alert
 *            issued is a*_s unless used == budget, then 0 (an attempt over budget, as w2a_step treats it); the state
 *            fields advance as in the step and rollout kernels
 *   o_s      the observation row the agent holds before decision s: row e of obs for s = 0, after that the table row of
 *            the day before with its four run-time fields -- the row w2a_step(a*_{s-1}) would have returned
 *   z_s      = weight[g] . o_s + bias[g], the fp64 logit;  p_s = sigmoid(z_s) in f32, as the rollout's
 *   m_s      0 on a day where require_budget is set and no budget is left (the policy's action is forced there and
 *            carries no likelihood; the action taken is 0), else 1
 *   delta_s  = m_s (a*_s - p_s): d log pi(a*_s | o_s) / d z_s
 *   ll_e     = sum_s m_s log pi(a*_s | o_s), each term -softplus(-z_s) (a* = 1) or -softplus(z_s) (a* = 0)
 *   g_e      = w_e sum_s delta_s (o_s, 1), w_e = env_weight[e] (NULL: 1); envs finished on entry get zeros
 * grad (device f32 [n_obs + 1][num_envs], column-major: component j of env e at j * num_envs + e) receives g_e: the
 * weight columns in OBSERVATION order, the bias last. loglik (f32 [num_envs]) receives ll_e (unweighted), days (i32
 * [num_envs]) sum_s m_s. The mean of g_e over a group's envs is the gradient of that group's mean w_e ll_e, so
 * theta += lr * mean is an ascent step on the likelihood.
 * Numerics contract: z_s is computed by the statements of k_rollout_linear (the same fp64 FMA chain: bias first, slots
 * 0..29 in slot order) and p_s by its f32 sigmoid; delta_s is f32; the products with w_e and o_s and the sums over s are
 * fp64, g_e is rounded to f32 once. Every term of ll_e is computed stably in fp64 from z_s, the sum is fp64 and rounded to
 * f32 once. An env's outputs do not depend on the other envs, the group layout or the visiting order (bit for bit).
 * policy->sample and policy->seed are ignored (nothing is drawn). No scratch memory.
 *   alert_mask  device u32 [num_envs][mask_words], mask_words * 32 >= T (the format w2a_rollout and w2a_hindsight_optimum
 *               write); bits of days outside the stretch are ignored
 * W2A_ERR_ARG where w2a_rollout_linear refuses (checked in the same order), for a NULL alert_mask, obs, grad, loglik or
 * days and for mask_words * 32 < T; W2A_ERR_STATE while `stream` is recording a hipGraph. */
int w2a_imitation_gradient_linear(w2a_env *env, const w2a_linear_policy *policy, const uint32_t *alert_mask,
                                  int32_t mask_words, const float *env_weight, int32_t n_steps, const float *obs,
                                  float *grad, float *loglik, int32_t *days, void *stream);
/* The same estimator for an MLP policy, already reduced per group: z_s is the f32 logit k_rollout_mlp computes for o_s
 * (the same mlp_logit_groups call on the same rows), dz_s/dtheta the backward pass of the f32 network as in
 * w2a_policy_gradient_mlp, and
 *     grad[g] = (1 / N_g) sum over the envs e of group g of  w_e sum_s delta_s dz_s/dtheta(theta_g)
 * (envs finished on entry contribute zero and count; a group without envs gives a block of NaN). grad, policy->order,
 * the workspace and the partial-block rule are those of w2a_policy_gradient_mlp; the workspace size is
 * w2a_imitation_gradient_mlp_workspace_bytes(...), equal to w2a_policy_gradient_mlp_workspace_bytes(...). loglik and days
 * as above, per env.
 * Numerics contract: c_s = w_e delta_s is formed in fp64 and rounded to f32 once; from there on the second pass, the
 * fp64 sums over tiles and the reduction are the kernels of w2a_policy_gradient_mlp, run unchanged (its c_s = delta_s Q_s
 * is fed Q_s = 1). The terms of ll_e are computed in fp64 from the f32 logit. No atomics: two identical calls give
 * identical bits.
 * W2A_ERR_ARG where w2a_rollout_mlp refuses (checked in the same order), for a NULL alert_mask, obs, grad, loglik, days
 * or workspace, mask_words * 32 < T and a workspace too small or misaligned; W2A_ERR_STATE while `stream` is recording a
 * hipGraph. */
size_t w2a_imitation_gradient_mlp_workspace_bytes(int64_t num_envs, int32_t n_steps, int32_t n_groups, int32_t width,
                                                  int32_t n_layers);
int w2a_imitation_gradient_mlp(w2a_env *env, const w2a_mlp_policy *policy, const uint32_t *alert_mask,
                               int32_t mask_words, const float *env_weight, int32_t n_steps, const float *obs,
                               float *grad, float *loglik, int32_t *days, void *workspace, size_t workspace_bytes,
                               void *stream);
/* w2a_imitation_gradient_linear / _mlp with a weight per call-day: the estimator becomes
 *     g_e = w_e sum_s d_{s,e} delta_s dz_s/dtheta,   d_{s,e} = day_weight[s * num_envs + e]
 * (device f32 [day_weight_days][num_envs], indexed by CALL-DAY and ENV ID -- the layout of w2a_value_gradient_*'s
 * advantage; entries of days the env does not step are not read). ll_e and days are unchanged. day_weight = NULL is the
 * unweighted call, bit for bit (the two entry points above forward NULL). The product w_e delta_s d_{s,e} is formed in
 * fp64 in that order; the MLP form rounds it to f32 once, as before.
 * With the schedule a sampled rollout ISSUED (w2a_rollout_*'s alert bitmap) and day_weight an advantage, this is the
 * score-function gradient of that rollout with the advantage in place of the reward-to-go -- exactly so only under
 * require_budget = 1, where attempts and issued alerts agree on every scored day; without it the policy gradient scores
 * an attempt at the budget as a_s = 1 while the bitmap of issued alerts holds 0 there.
 * day_weight is read as given: a NaN or infinite weight on a scored day goes into the gradient (the Python binding
 * refuses non-finite weights).
 * W2A_ERR_ARG as the unweighted entry points (same order), and for day_weight != NULL with day_weight_days < n_steps
 * (after every NULL and alignment check, the workspace's included, before the handle is looked at). */
int w2a_imitation_gradient_linear_weighted(w2a_env *env, const w2a_linear_policy *policy, const uint32_t *alert_mask,
                                           int32_t mask_words, const float *env_weight, const float *day_weight,
                                           int32_t day_weight_days, int32_t n_steps, const float *obs, float *grad,
                                           float *loglik, int32_t *days, void *stream);
int w2a_imitation_gradient_mlp_weighted(w2a_env *env, const w2a_mlp_policy *policy, const uint32_t *alert_mask,
                                        int32_t mask_words, const float *env_weight, const float *day_weight,
                                        int32_t day_weight_days, int32_t n_steps, const float *obs, float *grad,
                                        float *loglik, int32_t *days, void *workspace, size_t workspace_bytes,
                                        void *stream);
/* The gradient of the PPO-clip surrogate along a GIVEN alert schedule under a linear policy: what K epochs on the same
 * episodes need, the clipped importance ratio formed inside the kernel. Every env is forced along its own schedule from
 * the handle's CURRENT state and observation rows exactly as in w2a_imitation_gradient_linear: the same alert_mask, the
 * same attempted-versus-issued rule, the same o_s and the same require_budget rule for m_s. It reads the state, the
 * tables, the schedule, obs, advantage and old_log_prob and modifies none of them, nor the RNG, nor the handle's
 * bookkeeping beyond making the canonical state words current: epochs over the same episodes need no reset in between.
 * The estimator, for env e of group g on every scored call-day s (m_s = 1):
 *   z_s      the policy's logit on o_s;  a_s the schedule's bit (the action ATTEMPTED);  p_s = sigmoid(z_s)
 *   delta_s  = a_s - p_s
 *   lp_s     = log pi(a_s | z_s): -softplus(-z_s) (a_s = 1) or -softplus(z_s) (a_s = 0)
 *   rho_s    = exp(lp_s - old_log_prob[s * num_envs + e]); exactly 1 when old_log_prob is NULL
 *   A_s      = advantage[s * num_envs + e]
 *   lo, hi   = 1 - clip, 1 + clip
 *   live_s   = !((A_s > 0 && rho_s > hi) || (A_s < 0 && rho_s < lo)): the gradient of min(rho A, clamp(rho, lo, hi) A)
 *   H_s      = -p_s log p_s - (1 - p_s) log(1 - p_s), the Bernoulli entropy;  dH_s/dz = -z_s p_s (1 - p_s)
 *   L_e      = sum_s min(rho_s A_s, clamp(rho_s, lo, hi) A_s)
 *   g_e      = w_e sum_s [ live_s rho_s A_s delta_s + beta dH_s/dz ] (o_s, 1),  beta = entropy_coef,
 *              w_e = env_weight[e] (NULL: 1); envs finished on entry get zeros
 * The mean of g_e over a group's envs is the gradient of that group's mean w_e (L_e + beta sum_s H_s), so
 * theta += lr * mean is an ascent step on the clipped surrogate with an entropy bonus. With old_log_prob = NULL and
 * entropy_coef = 0 the estimator is w2a_imitation_gradient_linear_weighted's with day_weight = advantage.
 *   advantage      device f32 [advantage_days >= n_steps][num_envs] by CALL-DAY and ENV ID (the layout of
 *                  w2a_value_gradient_*'s advantage and of day_weight); entries of days that are not scored are not read.
 *                  Read as given: a NaN or infinite entry on a scored day goes into the outputs
 *   old_log_prob   nullable; device f32 [old_log_prob_days >= n_steps][num_envs], same layout: lp_s under the policy that
 *                  collected the schedule -- the log_prob output of an earlier call
 *   grad           device f32 [n_obs + 1][num_envs], column-major as w2a_imitation_gradient_linear: g_e
 *   surrogate      f32 [num_envs]: L_e (unweighted)
 *   clipped_days   i32 [num_envs]: the scored days with live_s = 0
 *   approx_kl      f32 [num_envs]: sum_s ((rho_s - 1) - log rho_s), summed and not averaged
 *   entropy        f32 [num_envs]: sum_s H_s
 *   days           i32 [num_envs]: sum_s m_s, as w2a_imitation_gradient_linear
 *   log_prob       nullable; device f32 [n_steps][num_envs] by call-day and env id: lp_s on scored days, 0 elsewhere (the
 *                  library zero-fills it on `stream` first). This is how the first epoch obtains old_log_prob
 * Numerics contract: z_s by the statements of k_rollout_linear (the fp64 FMA chain), delta_s in f32 from its f32 sigmoid,
 * as w2a_imitation_gradient_linear; lp_s, rho_s, the clip test, p_s and 1 - p_s of the entropy, the coefficient
 * (w_e delta_s) (rho_s A_s) + w_e beta dH_s/dz, its products with o_s and every sum over s are fp64; g_e, surrogate,
 * approx_kl, entropy and log_prob are rounded to f32 once. An env's outputs do not depend on the other envs, the group
 * layout or the visiting order (bit for bit). No scratch memory, no atomics: identical calls give identical bits.
 * W2A_ERR_ARG where w2a_imitation_gradient_linear_weighted refuses (checked in the same order; a NULL surrogate,
 * clipped_days, approx_kl or entropy counts as a NULL output), and -- where that call checks day_weight_days -- for a
 * NULL advantage, advantage_days < n_steps, old_log_prob != NULL with old_log_prob_days < n_steps, clip < 0 and a clip
 * or entropy_coef that is not finite; W2A_ERR_STATE while `stream` is recording a hipGraph. */
int w2a_surrogate_gradient_linear(w2a_env *env, const w2a_linear_policy *policy, const uint32_t *alert_mask,
                                  int32_t mask_words, const float *env_weight, const float *advantage,
                                  int32_t advantage_days, const float *old_log_prob, int32_t old_log_prob_days,
                                  double clip, double entropy_coef, int32_t n_steps, const float *obs, float *grad,
                                  float *surrogate, int32_t *clipped_days, float *approx_kl, float *entropy,
                                  int32_t *days, float *log_prob, void *stream);
/* The same estimator for an MLP policy, already reduced per group: z_s is the f32 logit k_rollout_mlp computes for o_s,
 * (o_s, 1) becomes dz_s/dtheta, the backward pass of the f32 network as in w2a_policy_gradient_mlp, and
 *     grad[g] = (1 / N_g) sum over the envs e of group g of  w_e sum_s [ live_s rho_s A_s delta_s + beta dH_s/dz ] dz_s/dtheta
 * (envs finished on entry contribute zero and count; a group without envs gives a block of NaN). grad, policy->order, the
 * workspace and the partial-block rule are those of w2a_policy_gradient_mlp; the workspace size is
 * w2a_surrogate_gradient_mlp_workspace_bytes(...), equal to w2a_imitation_gradient_mlp_workspace_bytes(...). The other
 * outputs as above, per env.
 * Numerics contract: delta_s in f32 as w2a_imitation_gradient_mlp; lp_s, rho_s, the clip test, the entropy terms and the
 * coefficient c_s are formed in fp64 from the f32 logit and c_s is rounded to f32 once; from there on the second pass,
 * the fp64 sums over tiles and the reduction are the kernels of w2a_policy_gradient_mlp, run unchanged (day = (c_s, 0),
 * total = 1). No atomics: two identical calls give identical bits.
 * W2A_ERR_ARG where w2a_imitation_gradient_mlp_weighted refuses (same order) and for the arguments listed above;
 * W2A_ERR_STATE while `stream` is recording a hipGraph. */
size_t w2a_surrogate_gradient_mlp_workspace_bytes(int64_t num_envs, int32_t n_steps, int32_t n_groups, int32_t width,
                                                  int32_t n_layers);
int w2a_surrogate_gradient_mlp(w2a_env *env, const w2a_mlp_policy *policy, const uint32_t *alert_mask,
                               int32_t mask_words, const float *env_weight, const float *advantage,
                               int32_t advantage_days, const float *old_log_prob, int32_t old_log_prob_days,
                               double clip, double entropy_coef, int32_t n_steps, const float *obs, float *grad,
                               float *surrogate, int32_t *clipped_days, float *approx_kl, float *entropy,
                               int32_t *days, float *log_prob, void *workspace, size_t workspace_bytes, void *stream);
/* The gradient of a least-squares fit of a state-value function to the reward-to-go along a GIVEN alert schedule: the
 * critic's counterpart of w2a_imitation_gradient_linear. `value` is a linear policy struct whose logit is read as a
 * value, V(o) = weight[g] . o + bias[g]: no sigmoid, nothing drawn; value->sample, ->seed and ->require_budget are
 * ignored. Every env is forced along its own schedule from the handle's CURRENT state and observation rows, with
 * alert_mask, a*_s, the alert issued and o_s exactly as w2a_imitation_gradient_linear defines them. It reads the state,
 * the tables, the schedule and obs and modifies none of them, nor the RNG, nor the handle's bookkeeping beyond making
 * the canonical state words current.
 * The estimator, for env e of group g over the call-days s = 0 .. S_e - 1 on which the env takes a step:
 *   r_s      the reward w2a_step pays for that day under the env's own posterior draw
 *   Q_s      = sum over s' >= s of r_s': undiscounted, truncated at the call's last day, nothing is bootstrapped
 *              (discounting, GAE(lambda), a bootstrap and fixed targets: w2a_value_gradient_linear_gae below)
 *   V_s      = V(o_s)
 *   g_e      = w_e sum_s (Q_s - V_s) (o_s, 1), w_e = env_weight[e] (NULL: 1); envs finished on entry get zeros
 * grad (device f32 [n_obs + 1][num_envs], column-major, as w2a_policy_gradient_linear) receives g_e; the mean of g_e
 * over a group's envs is MINUS the gradient of 1/2 mean_e w_e sum_s (V_s - Q_s)^2, so theta += lr * mean descends it.
 *   sq_error    f32 [num_envs]: sum_s (Q_s - V_s)^2 (unweighted)
 *   days        i32 [num_envs]: S_e
 *   ret         f32 [num_envs]: Q_0
 *   advantage   nullable; device f32 [n_steps][num_envs] by call-day and ENV ID: Q_s - V_s on stepped days, 0 elsewhere
 *               (the library zero-fills it on `stream` first)
 *   workspace   w2a_value_gradient_linear_workspace_bytes(num_envs, n_steps) bytes, 256-B aligned: 9 B per env-day
 * Numerics contract: r_s is computed by the statements of k_rollout_linear (the two fp64 chains, reward_from_logits,
 * f32), V_s by its fp64 logit chain (bias first, slots 0..29 in slot order). The one-step residual
 * y_s = r_s + V_{s+1} - V_s (V := 0 past the env's last stepped day of the call) is formed and kept in fp64,
 * Q_s - V_s = sum_s y - sum_{s' < s} y_s' in fp64, the products with w_e and o_s and the sums over s in fp64; g_e,
 * sq_error, ret and advantage are rounded to f32 once. An env's outputs do not depend on the other envs, the group
 * layout or the visiting order (bit for bit). No atomics: two identical calls give identical bits.
 * W2A_ERR_ARG where w2a_imitation_gradient_linear refuses (same order; sample and require_budget are not looked at),
 * for a NULL sq_error, days, ret or workspace and a workspace too small or misaligned; W2A_ERR_STATE while `stream`
 * is recording a hipGraph. */
size_t w2a_value_gradient_linear_workspace_bytes(int64_t num_envs, int32_t n_steps);
int w2a_value_gradient_linear(w2a_env *env, const w2a_linear_policy *value, const uint32_t *alert_mask,
                              int32_t mask_words, const float *env_weight, int32_t n_steps, const float *obs,
                              float *grad, float *sq_error, int32_t *days, float *ret, float *advantage,
                              void *workspace, size_t workspace_bytes, void *stream);
/* The same estimator for an MLP, already reduced per group: V_s is the f32 logit k_rollout_mlp computes for o_s (the same
 * mlp_logit_groups call on the same rows), (o_s, 1) becomes dV_s/dtheta, the backward pass of the f32 network as in
 * w2a_policy_gradient_mlp, and
 *     grad[g] = (1 / N_g) sum over the envs e of group g of  w_e sum_s (Q_s - V_s) dV_s/dtheta(theta_g)
 * (envs finished on entry contribute zero and count; a group without envs gives a block of NaN). grad, value->order, the
 * workspace and the partial-block rule are those of w2a_policy_gradient_mlp; the workspace size is
 * w2a_value_gradient_mlp_workspace_bytes(...), equal to w2a_policy_gradient_mlp_workspace_bytes(...). sq_error, days, ret
 * and advantage as above, per env.
 * Numerics contract: r_s by the statements of k_rollout_mlp; y_s = r_s + V_{s+1} - V_s is formed in fp64 from the f32
 * values and rounded to f32 once (the scratch holds f32); total = the fp64 sum of the rounded y_s, so Q_s - V_s is taken
 * as total - sum_{s' < s} y_s', exactly the sum of the stored residuals of the days still to come: it differs from the
 * unrounded residual by at most 2^-24 sum_{s' >= s} |y_s'|. c_s = w_e (Q_s - V_s) is formed in fp64 and rounded to
 * f32 once; from there on the second pass, the fp64 sums over tiles and the reduction are the kernels of
 * w2a_policy_gradient_mlp, run unchanged (day = (w_e, y_s)). sq_error and advantage come from the same fp64
 * differences. No atomics: two identical calls give identical bits.
 * W2A_ERR_ARG where w2a_imitation_gradient_mlp refuses (same order; sample and require_budget are not looked at), for a
 * NULL sq_error, days or ret; W2A_ERR_STATE while `stream` is recording a hipGraph. */
size_t w2a_value_gradient_mlp_workspace_bytes(int64_t num_envs, int32_t n_steps, int32_t n_groups, int32_t width,
                                              int32_t n_layers);
int w2a_value_gradient_mlp(w2a_env *env, const w2a_mlp_policy *value, const uint32_t *alert_mask, int32_t mask_words,
                           const float *env_weight, int32_t n_steps, const float *obs, float *grad, float *sq_error,
                           int32_t *days, float *ret, float *advantage, void *workspace, size_t workspace_bytes,
                           void *stream);
/* w2a_value_gradient_linear with GAE(lambda), discounting, a bootstrap past the call, and targets fixed by an earlier
 * call. The env is forced along its schedule exactly as in w2a_value_gradient_linear (the same bitmap, the same
 * attempted-versus-issued rule, the same rows o_s, the same reward statements). The estimator, for env e over the
 * call-days s = 0 .. S_e - 1 on which it takes a step:
 *   V_s      = V(o_s)
 *   Vn_s     the value of the row after day s: V(o_{s+1}) when the env holds a row after day s inside the call; 0 when
 *            day s is the episode's last day; on the call's last day (s + 1 == n_steps) with the episode not finished,
 *            V(o_{s+1}) when bootstrap = 1 and 0 when bootstrap = 0 (w2a_value_gradient_linear's convention)
 *   delta_s  = r_s + gamma Vn_s - V_s
 *   A_s      = delta_s + gamma lambda A_{s+1},  A_{S_e} = 0
 *   R_s      = A_s + V_s  (the lambda-return)
 *   c_s      = A_s (the semi-gradient: the target R_s is held fixed);  with target given, c_s = target[s][e] - V_s
 *   g_e      = w_e sum_s c_s (o_s, 1)
 * gamma = lambda = 1 with bootstrap = 0 is the estimator of w2a_value_gradient_linear.
 *   sq_error      sum_s c_s^2
 *   ret           the UNDISCOUNTED sum_s r_s (zeros when target is given: no reward is formed then)
 *   advantage     nullable; A_s at [call-day][env id], 0 elsewhere (zero-filled on `stream` first)
 *   value_target  nullable; R_s in the same layout (zero-filled on `stream` first)
 *   target        nullable; device f32 [target_days >= n_steps][num_envs], the layout of value_target; entries of days
 *                 an env does not step are not read. With target given no reward enters.
 *   workspace     w2a_value_gradient_linear_gae_workspace_bytes(num_envs, n_steps) bytes, 256-B aligned: 17 B per env-day
 * Numerics contract: r_s and V_s as w2a_value_gradient_linear; delta_s is formed and kept in fp64; the recursion, c_s,
 * the products with w_e and o_s and the sums over s are fp64; g_e, sq_error, ret, advantage and value_target are rounded
 * to f32 once. An env's outputs do not depend on the other envs, the group layout or the visiting order (bit for bit).
 * No atomics: two identical calls give identical bits.
 * W2A_ERR_ARG where w2a_value_gradient_linear refuses (same order), and, after its NULL-output check: gamma or lambda
 * outside [0, 1] (NaN included), bootstrap other than 0 or 1, target_days < n_steps, and target combined with advantage,
 * value_target, a gamma or lambda other than 1, or bootstrap. W2A_ERR_STATE while `stream` is recording a hipGraph. */
size_t w2a_value_gradient_linear_gae_workspace_bytes(int64_t num_envs, int32_t n_steps);
int w2a_value_gradient_linear_gae(w2a_env *env, const w2a_linear_policy *value, const uint32_t *alert_mask,
                                  int32_t mask_words, const float *env_weight, int32_t n_steps, const float *obs,
                                  float *grad, float *sq_error, int32_t *days, float *ret, float *advantage,
                                  double gamma, double lambda, int32_t bootstrap, float *value_target,
                                  const float *target, int32_t target_days, void *workspace, size_t workspace_bytes,
                                  void *stream);
/* The same estimator for an MLP, reduced per group as w2a_value_gradient_mlp: (o_s, 1) becomes dV_s/dtheta. The
 * workspace is that of w2a_value_gradient_mlp (w2a_value_gradient_mlp_gae_workspace_bytes(...) returns the same size).
 * Numerics contract: V_s and Vn_s are the f32 logits; delta_s is formed in fp64 from them and the f32 reward and rounded
 * to f32 once (the scratch holds (f32(delta_s), V_s)); the recursion runs in fp64 over the stored delta_s, backwards from
 * the env's last day, so A_s differs from the recursion on unrounded residuals by at most
 * 2^-24 sum_{s' >= s} (gamma lambda)^(s' - s) |delta_s'|. w_e c_s is formed in fp64 and rounded to f32 once; it replaces
 * the day's record (day = (f32(w_e c_s), 0), total = 1), and from there on the second pass, the fp64 sums over tiles and
 * the reduction are the kernels of w2a_policy_gradient_mlp, run unchanged. sq_error, advantage and value_target come from
 * the same fp64 values, each rounded to f32 once. No atomics: two identical calls give identical bits.
 * W2A_ERR_ARG where w2a_value_gradient_mlp refuses (same order) and for the arguments listed above. */
size_t w2a_value_gradient_mlp_gae_workspace_bytes(int64_t num_envs, int32_t n_steps, int32_t n_groups, int32_t width,
                                                  int32_t n_layers);
int w2a_value_gradient_mlp_gae(w2a_env *env, const w2a_mlp_policy *value, const uint32_t *alert_mask,
                               int32_t mask_words, const float *env_weight, int32_t n_steps, const float *obs,
                               float *grad, float *sq_error, int32_t *days, float *ret, float *advantage, double gamma,
                               double lambda, int32_t bootstrap, float *value_target, const float *target,
                               int32_t target_days, void *workspace, size_t workspace_bytes, void *stream);
/* Optional, speed only: let w2a_rollout visit the envs in the order of their feature rows (envs that share a
 * (county, year) sit in the same wave and read the same table lines every day). Results are those of any other
 * order -- per-env outputs, RNG streams and state stay indexed by env id. Call after a reset (the order of an
 * earlier episode stays valid as a permutation, it is just no longer sorted). workspace: caller-owned,
 * w2a_rollout_order_workspace_bytes(num_envs, S_w * Y) bytes, 256-B aligned, must stay alive while w2a_rollout is
 * used -- and, once attached, until w2a_destroy.
 *   w2a_rollout_order_attach  (host only) hands the workspace over ahead of time: from then on every whole-batch reset
 *                             also counts the envs of each feature row and ranks every env inside its row there (the
 *                             first pass of the counting sort, hidden behind the reset's observation stores), and
 *                             w2a_rollout_order is left with a scan and an atomic-free placement. w2a_rollout_order
 *                             attaches its workspace itself on first use. */
size_t w2a_rollout_order_workspace_bytes(int64_t num_envs, int64_t table_rows);
int w2a_rollout_order_attach(w2a_env *env, void *workspace, size_t workspace_bytes);
int w2a_rollout_order(w2a_env *env, void *workspace, size_t workspace_bytes, void *stream);

/* Optional, speed only: let w2a_rollout compute the table-sourced part of both logits -- 27 of their 30 terms, which do
 * not depend on the agent's actions -- for all envs of a (county, year) and 16 days at a time on the int8 matrix cores
 * (exact fixed-point digits, int32 accumulation; csrc/w2a_rollout_mfma.hip.h), leaving 3 + 3 fp64 FMAs per env-day on
 * the vector ALU instead of 30 + 30. Call after w2a_rollout_order of the episode (it lists the tiles of envs sharing a
 * feature row from that order and, once per table, builds a digit table of W in the workspace). Used by w2a_rollout
 * while the handle knows the batch to be in lock step and no corrected-semantics flag is set; results agree with the
 * other rollout kernels to the accuracy of the fixed point (returns within ~1e-6 relative), integers identical.
 * workspace: caller-owned, w2a_rollout_mfma_workspace_bytes(...) bytes, 256-B aligned, alive while w2a_rollout is used. */
size_t w2a_rollout_mfma_workspace_bytes(int64_t num_envs, int64_t table_rows, int32_t S, int32_t n_samples);
int w2a_rollout_mfma_prepare(w2a_env *env, void *workspace, size_t workspace_bytes, void *stream);

/* w2a_rollout with the posterior-mean reward (w2a_posterior_mean_reward's value every day), whole episode in one launch:
 * same arguments and outputs as w2a_rollout; needs w2a_group_by_column after the last reset. Built on the kernel selected
 * by w2a_set_posterior_kernel: W2A_PM_MATRIX_I8 (k_pm_rollout_i8) or W2A_PM_VECTOR (k_pm_rollout). Returns 1 (nothing
 * done) when no one-launch kernel applies -- more posterior draws than one LDS staging pass holds (112), the vector form
 * with coefficients on slots 28/30/31, W2A_PM_MATRIX_F64 -- and the caller runs the per-day sequence w2a_policy_actions,
 * w2a_posterior_mean_reward, w2a_step. */
int w2a_rollout_posterior_mean(w2a_env *env, const w2a_policy *policy, int32_t n_steps, float *ret_out,
                               int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask,
                               uint32_t *attempt_mask, int32_t mask_words, float *last_return, float *ret_snapshot,
                               void *stream);

/* One day of a built-in policy: actions i32 [n] of every env from its pre-step state -- the same policy evaluation,
 * lagging observation and budget gate as w2a_rollout (finished envs get action 0) -- for policy loops whose step is
 * w2a_step, e.g. with w2a_posterior_mean_reward. Nullable accumulators, updated for today: alerts i32 [n] += alert
 * issued, attempts_over_budget i32 [n] += alert attempted at budget, alert_mask / attempt_mask u32 [n][mask_words]
 * |= bit (day) -- the caller zeroes them before the first day. */
int w2a_policy_actions(w2a_env *env, const w2a_policy *policy, int32_t *actions, int32_t *alerts,
                       int32_t *attempts_over_budget, uint32_t *alert_mask, uint32_t *attempt_mask, int32_t mask_words,
                       void *stream);

/* Decode the packed state into the caller's arrays (see w2a_state_view). */
int w2a_get_state(w2a_env *env, const w2a_state_view *view, void *stream);

/* What the handle knows (host-side bookkeeping, no device work): the day every env is on if the batch is known to be in
 * lock step AND the host can know the day (-1 otherwise: not in lock step, past the terminal step, or a step of this
 * handle was recorded into a hipGraph); whether the tables allow the lock-step mirror at all; which of the two
 * forms of the step state is current; whether the batch is known to be in lock step. */
enum { W2A_Q_LOCKSTEP = 6,           /* 1: every env is known to be on the same day of an episode of the one length there is */
       W2A_Q_LOCKSTEP_DAY = 0, W2A_Q_PACKED_ELIGIBLE = 1, W2A_Q_PACKED_CURRENT = 2, W2A_Q_CANONICAL_CURRENT = 3,
       W2A_Q_LAST_ROLLOUT_KERNEL = 4 /* what the last w2a_rollout launched: -1 none yet, 0 k_rollout (4 lanes per env),
                                        1 k_rollout64 (lane = env), 2 k_rollout_mfma (int8 matrix cores); 3 after
                                        w2a_rollout_linear: k_rollout_linear (lane = env); 4 after
                                        w2a_rollout_mlp: k_rollout_mlp (lane = env, f32 matrix cores) */,
       W2A_Q_LAST_STEP_KERNEL = 5    /* what the last w2a_step launched: -1 none yet, 0 k_step (4 lanes per env),
                                        1 k_step64 on the canonical state words, 2 k_step64 on the lock-step mirror */,
       W2A_Q_EPISODE_WORD_BYTES = 7  /* bytes per env of the lock-step mirror's per-episode word: 4 (narrow) or 8 */ };
int w2a_query(w2a_env *env, int what);

/* Debug / A-B switch, results never depend on it. The lock-step mirror keeps one word per env that is constant while an
 * episode runs. w2a_create picks its form from the table dims: where the coefficient-row index (S * n_samples values)
 * and the day-row index (S_w * Y values) fit 32 bits together, a 4-byte word of the two indices (the budget then
 * travels as the remaining budget in the mirror's state word: 145 B per env-step), else the 8-byte word of budget,
 * column, row and draw (149 B). force_wide != 0 makes the handle use the 8-byte word whatever the dims, 0 goes back to
 * the rule. To be called before the handle first steps on the packed form: W2A_ERR_STATE while the mirror is current
 * or a packed step has been recorded into a hipGraph. */
int w2a_set_episode_word(w2a_env *env, int force_wide);

/* The caller has overwritten the state buffer (e.g. restored a checkpoint of its canonical part) on `stream`: forget
 * every derived form (lock-step mirror, column grouping, row counts, what is known about days). Host-side bookkeeping
 * only -- plus, on a handle with a recorded packed step, one small launch on `stream` that marks the mirror stale --:
 * no wait, nothing read back. (Until ABI 17 the call scanned the restored buffer for its largest budget and waited for
 * the stream, and w2a_set_budget_bound let a caller state one: the packed form held budgets in 16 bits and the handle had
 * to bound them from the host side. The packed kernel now serves any budget; both are gone.)
 * Fails with W2A_ERR_STATE while `stream` is recording a hipGraph. */
int w2a_invalidate(w2a_env *env, void *stream);

/* Synchronise `stream`, read and clear the device status word (host int out). */
int w2a_read_status(w2a_env *env, int32_t *status_out, void *stream);

/* ----------------------------------------------------------------------------------------------------------------------
 * Alert gates: learned policies restricted to allowed days (the older reference env's restrict_alerts / HI_restriction).
 *
 * allowed_days is a per-env bitmap over the days of the episode in the layout of alert_mask: uint32 [num_envs]
 * [allowed_words], bit (t & 31) of word t >> 5, allowed_words * 32 >= T. On a day whose bit is clear the attempted
 * action is forced to 0 BEFORE the attempt is recorded and before the budget test: such a day never counts as an
 * over-budget attempt, and it is a forced choice like a day on which require_budget forces the action -- it carries no
 * score, no log-likelihood, no ratio, no entropy, and the `days` outputs do not count it. The Bernoulli uniform of a day
 * is a function of (env, episode, day): a gated day moves no other day's draw. A NULL allowed_days is refused (the entry
 * points without _gated take no gate); an all-ones bitmap gives the bits of the ungated call. The gate is an argument of
 * the call and is not kept on the handle; w2a_step and the built-in policy kinds know nothing of it.
 *
 * w2a_alert_gate builds the bitmap the reference's restriction stands for: bit t of env e is set iff the value of
 * observation column obs_col in the row the agent holds when it chooses day t's action is >= the threshold
 * (thresholds[e] when thresholds is not NULL, else threshold; >= as in the reference, not the > of the threshold policy
 * kind). That row is the one w2a_step would have returned: the table row of day max(t - 1, 0) under the faithful
 * semantics (the lagging observation), the row of day t with W2A_FIX_OBS. It covers the days the env would still step
 * from its current state (n_steps of them, or to its terminal day); days before, days after and finished envs are 0.
 * obs_col must be table-sourced (slots 24..27, and the 'alerts_2wks' column under W2A_FIX_ALERTS_2WKS, hold the agent's
 * own history: W2A_ERR_ARG). Reads the tables and the state, writes allowed_days only; asynchronous on `stream`.
 *
 * The *_gated entry points take the arguments of the entry point they are named after, then allowed_days and
 * allowed_words. w2a_rollout_linear_gated takes w2a_rollout_linear_record's arguments with traj nullable (NULL: no
 * trajectory; recorded `action` is 0 on a gated day, `logit` is still the policy's). w2a_imitation_gradient_linear_gated
 * takes w2a_imitation_gradient_linear_weighted's with day_weight nullable: an alert the schedule asks for on a
 * disallowed day is attempted as 0. w2a_hindsight_optimum_gated: the DP may alert only on allowed days, so the result is
 * the best schedule under the restriction, its return the bits the env pays for that schedule. */
int w2a_alert_gate(w2a_env *env, int32_t obs_col, float threshold, const float *thresholds, int32_t n_steps,
                   uint32_t *allowed_days, int32_t allowed_words, void *stream);
int w2a_rollout_linear_gated(w2a_env *env, const w2a_linear_policy *policy, int32_t n_steps, float *obs, float *ret_out,
                             int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask,
                             uint32_t *attempt_mask, int32_t mask_words, float *last_return, float *ret_snapshot,
                             void *stream, const w2a_trajectory *traj, const uint32_t *allowed_days,
                             int32_t allowed_words);
int w2a_policy_gradient_linear_gated(w2a_env *env, const w2a_linear_policy *policy, int32_t baseline, int32_t n_steps,
                                     const float *obs, float *grad, void *workspace, size_t workspace_bytes,
                                     void *stream, const uint32_t *allowed_days, int32_t allowed_words);
int w2a_imitation_gradient_linear_gated(w2a_env *env, const w2a_linear_policy *policy, const uint32_t *alert_mask,
                                        int32_t mask_words, const float *env_weight, const float *day_weight,
                                        int32_t day_weight_days, int32_t n_steps, const float *obs, float *grad,
                                        float *loglik, int32_t *days, void *stream, const uint32_t *allowed_days,
                                        int32_t allowed_words);
int w2a_surrogate_gradient_linear_gated(w2a_env *env, const w2a_linear_policy *policy, const uint32_t *alert_mask,
                                        int32_t mask_words, const float *env_weight, const float *advantage,
                                        int32_t advantage_days, const float *old_log_prob, int32_t old_log_prob_days,
                                        double clip, double entropy_coef, int32_t n_steps, const float *obs,
                                        float *grad, float *surrogate, int32_t *clipped_days, float *approx_kl,
                                        float *entropy, int32_t *days, float *log_prob, void *stream,
                                        const uint32_t *allowed_days, int32_t allowed_words);
/* the MLP kind: w2a_rollout_mlp_record's arguments with traj nullable, w2a_policy_gradient_mlp's,
 * w2a_imitation_gradient_mlp_weighted's with day_weight nullable, w2a_surrogate_gradient_mlp's -- then the bitmap. The
 * workspaces are those of the ungated calls. */
int w2a_rollout_mlp_gated(w2a_env *env, const w2a_mlp_policy *policy, int32_t n_steps, float *obs, float *ret_out,
                          int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask,
                          uint32_t *attempt_mask, int32_t mask_words, float *last_return, float *ret_snapshot,
                          void *stream, const w2a_trajectory *traj, const uint32_t *allowed_days, int32_t allowed_words);
int w2a_policy_gradient_mlp_gated(w2a_env *env, const w2a_mlp_policy *policy, int32_t baseline, int32_t n_steps,
                                  const float *obs, float *grad, void *workspace, size_t workspace_bytes, void *stream,
                                  const uint32_t *allowed_days, int32_t allowed_words);
int w2a_imitation_gradient_mlp_gated(w2a_env *env, const w2a_mlp_policy *policy, const uint32_t *alert_mask,
                                     int32_t mask_words, const float *env_weight, const float *day_weight,
                                     int32_t day_weight_days, int32_t n_steps, const float *obs, float *grad,
                                     float *loglik, int32_t *days, void *workspace, size_t workspace_bytes,
                                     void *stream, const uint32_t *allowed_days, int32_t allowed_words);
int w2a_surrogate_gradient_mlp_gated(w2a_env *env, const w2a_mlp_policy *policy, const uint32_t *alert_mask,
                                     int32_t mask_words, const float *env_weight, const float *advantage,
                                     int32_t advantage_days, const float *old_log_prob, int32_t old_log_prob_days,
                                     double clip, double entropy_coef, int32_t n_steps, const float *obs, float *grad,
                                     float *surrogate, int32_t *clipped_days, float *approx_kl, float *entropy,
                                     int32_t *days, float *log_prob, void *workspace, size_t workspace_bytes,
                                     void *stream, const uint32_t *allowed_days, int32_t allowed_words);
int w2a_hindsight_optimum_gated(w2a_env *env, const w2a_state_view *start, int32_t n_steps, float *ret_out,
                                uint32_t *alert_mask, int32_t mask_words, int32_t *alerts_out, void *workspace,
                                size_t workspace_bytes, void *stream, const uint32_t *allowed_days,
                                int32_t allowed_words);

/* Fisher-vector products of a policy along a GIVEN alert schedule: the primitive of the natural policy gradient and of
 * TRPO's conjugate-gradient step, over the episodes at hand and with no observation row recorded. Every env is forced
 * along its own schedule from the handle's CURRENT state and observation rows exactly as in
 * w2a_surrogate_gradient_linear: the same alert_mask, the same attempted-versus-issued rule, the same o_s and the same
 * m_s (a day on which require_budget forces the action, or which allowed_days closes, is not scored). The state, the
 * tables, the schedule, obs and the vector are only read, as there.
 * The Fisher information of one Bernoulli decision with logit z_s and p_s = sigmoid(z_s) is p_s (1 - p_s) J_s^T J_s,
 * J_s = dz_s/dtheta. For env e of group g, with v_g that group's block of the vector:
 *   u_s   = J_s . v_g                                   (linear: vec_weight[g] . o_s + vec_bias[g])
 *   Fv_e  = w_e sum_s m_s p_s (1 - p_s) u_s J_s^T        (linear: J_s = (o_s, 1)); w_e = env_weight[e] (NULL: 1)
 *   q_e   = sum_s m_s p_s (1 - p_s) u_s^2                (unweighted)
 * The mean of Fv_e over a group's envs is F_g v_g, and the mean of w_e q_e is <v_g, F_g v_g>: 1/2 eps^2 of it is the
 * second-order term of the group's mean w_e sum_s KL(pi_theta || pi_{theta + eps v}). The schedule's labels enter only
 * through the states visited.
 *   vec_weight, vec_bias   device f32 [n_groups][32] (16-B aligned, slot order as policy->weight) and [n_groups]: read
 *                          with the policy's clamped group id, never outside these bounds
 *   fv          device f32 [n_obs + 1][num_envs], column-major as w2a_surrogate_gradient_linear's grad: Fv_e
 *   quadratic   f32 [num_envs]: q_e;   days  i32 [num_envs]: sum_s m_s, as w2a_surrogate_gradient_linear
 *   allowed_days, allowed_words   nullable gate, as the *_gated entry points take it (NULL: every day is allowed and
 *                          allowed_words is not read)
 * Numerics contract: z_s and u_s are two fp64 FMA chains in the slot order of k_rollout_linear; p_s and 1 - p_s are
 * formed in fp64 from exp(-|z_s|) without cancellation; the coefficient, its products with o_s and every sum over s are
 * fp64; Fv_e and q_e are rounded to f32 once. No scratch memory, no atomics: identical calls give identical bits.
 * W2A_ERR_ARG where w2a_surrogate_gradient_linear refuses its policy, then for a NULL or misaligned vector, a NULL
 * alert_mask, obs or output, then as that call for the handle and the gate; W2A_ERR_STATE while `stream` is recording a
 * hipGraph. */
int w2a_fisher_vector_product_linear(w2a_env *env, const w2a_linear_policy *policy, const float *vec_weight,
                                     const float *vec_bias, const uint32_t *alert_mask, int32_t mask_words,
                                     const float *env_weight, int32_t n_steps, const float *obs, float *fv,
                                     float *quadratic, int32_t *days, void *stream, const uint32_t *allowed_days,
                                     int32_t allowed_words);
/* The same product for an MLP policy, already reduced per group: fv[g] = (1 / N_g) sum over the envs of group g of Fv_e,
 * a block in the layout of policy->params (a group without envs gives a block of NaN; envs finished on entry contribute
 * zero and count). `vector` is device f32 [n_groups][W2A_MLP_STRIDE(width, n_layers)], 16-B aligned, in the packed
 * layout and stride of policy->params, padding zero. u_s is the forward-mode tangent of the f32 network along v_g,
 * computed on the matrix cores next to the logit: adot_1 = V1 x + vb1, hdot_1 = act'(h_1) adot_1,
 * adot_2 = W2 hdot_1 + V2 h_1 + vb2, u = w_o . hdot + v_o . h + vb_o, with act' taken from the activation's value as in the
 * backward pass (tanh: 1 - h^2; ReLU: 1 where h > 0, 0 at exactly 0).
 * Numerics contract: z_s is the f32 logit of k_rollout_mlp, bit for bit; u_s is f32 (k-ordered fmaf chains, the bias
 * first); p_s, 1 - p_s, c_s = w_e p_s (1 - p_s) u_s and q_e are fp64 and c_s is rounded to f32 once; from there on the
 * second pass, the fp64 sums over tiles and the reduction are the kernels of w2a_policy_gradient_mlp, run unchanged
 * (day = (c_s, 0), total = 1). No atomics: two identical calls give identical bits. The workspace is that of
 * w2a_policy_gradient_mlp. */
size_t w2a_fisher_vector_product_mlp_workspace_bytes(int64_t num_envs, int32_t n_steps, int32_t n_groups, int32_t width,
                                                     int32_t n_layers);
int w2a_fisher_vector_product_mlp(w2a_env *env, const w2a_mlp_policy *policy, const float *vector,
                                  const uint32_t *alert_mask, int32_t mask_words, const float *env_weight,
                                  int32_t n_steps, const float *obs, float *fv, float *quadratic, int32_t *days,
                                  void *workspace, size_t workspace_bytes, void *stream, const uint32_t *allowed_days,
                                  int32_t allowed_words);
/* DQN / double-DQN temporal-difference semi-gradient of a two-head MLP Q-net along a GIVEN alert schedule, reduced per
 * group. The env is forced along its schedule exactly as in w2a_value_gradient_mlp (the same bitmap, the same
 * attempted-versus-issued rule, the same rows o_s, the same reward statements); an off-policy replay buffer is therefore
 * a list of (reset seed, schedule bitmap) pairs and no observation row is stored. `q` and `target_net` point to blocks
 * in the TWO-HEAD layout above (W2A_MLP_HEADS_STRIDE floats each); target_net = NULL: the online net is its own target
 * (the second evaluation of every row is then skipped). Of target_net only params, width, n_layers, activation and
 * n_groups are read, and the last four must equal q's; group and order are q's. For env e over the call-days
 * s = 0 .. S_e - 1 on which it takes a step, with a_s the alert ISSUED on day s (after the budget test):
 *   N_s      0 when day s is the episode's last day, and on the call's last day (s + 1 == n_steps) unless bootstrap = 1;
 *            else max_a' Qt(o_{s+1}, a'), or with double_q = 1 Qt(o_{s+1}, a*), a* = 1 iff Q(o_{s+1}, 1) > Q(o_{s+1}, 0)
 *            under the ONLINE net. With q->require_budget = 1 the max / argmax is restricted to a' = 0 when no budget is
 *            left after day s (an alert there would be a no-op).
 *   y_s      = r_s + gamma N_s
 *   delta_s  = y_s - Q(o_s, a_s)
 *   c_s      = delta_s (W2A_Q_LOSS_SQUARED, l = delta^2 / 2) or clamp(delta_s, +-huber_delta) (W2A_Q_LOSS_HUBER,
 *              l = delta^2 / 2 inside, huber_delta (|delta| - huber_delta / 2) outside: smooth_l1 at huber_delta = 1)
 *   grad[g]  = (1 / N_g) sum over the envs e of group g of  w_e sum_s c_s dQ(o_s, a_s)/dtheta(theta_g)
 * the semi-gradient (y_s is held fixed), pointing in the ASCENT direction of -loss as every other gradient here. Envs
 * finished on entry contribute zero and count; a group without envs gives a block of NaN.
 *   grad        device f32 [n_groups][W2A_MLP_HEADS_STRIDE(width, n_layers)] in the two-head layout
 *   loss        f32 [num_envs]: sum_s l(delta_s), unweighted;   days  i32 [num_envs]: S_e;   ret  f32 [num_envs]: sum_s r_s
 *   td_error, td_target   nullable f32 [n_steps][num_envs] by call-day and ENV ID: delta_s and y_s on stepped days, 0
 *               elsewhere (the library zero-fills them on `stream` first)
 *   workspace   w2a_q_gradient_mlp_workspace_bytes(...) bytes, 256-B aligned: the layout of w2a_value_gradient_mlp with
 *               the partial blocks at the two-head stride. A smaller one is refused; nothing is written past it.
 * Numerics contract: head a of a row is, bit for bit, the f32 logit k_rollout_mlp forms for the one-output net made of
 * the same hidden layers and output row a. y_s, delta_s and c_s are formed in fp64 from the f32 head values and the f32
 * reward; w_e c_s is rounded to f32 once, and from there on the second pass is that of w2a_policy_gradient_mlp with the
 * output row selected per env-day; the fp64 sums over tiles and the reduction run unchanged. An env's outputs do not
 * depend on the other envs, the group layout or the visiting order. No atomics: identical calls give identical bits.
 * W2A_ERR_ARG where w2a_value_gradient_mlp refuses (same order; sample is not looked at), then for a target net that
 * differs in shape, a gamma outside [0, 1], a double_q, loss or bootstrap that is no listed value and a huber_delta
 * that is not finite and positive; W2A_ERR_STATE while `stream` is recording a hipGraph. */
enum { W2A_Q_LOSS_SQUARED = 0, W2A_Q_LOSS_HUBER = 1 };
size_t w2a_q_gradient_mlp_workspace_bytes(int64_t num_envs, int32_t n_steps, int32_t n_groups, int32_t width,
                                          int32_t n_layers);
int w2a_q_gradient_mlp(w2a_env *env, const w2a_mlp_policy *q, const w2a_mlp_policy *target_net,
                       const uint32_t *alert_mask, int32_t mask_words, const float *env_weight, int32_t n_steps,
                       const float *obs, float *grad, float *loss_out, int32_t *days, float *ret, double gamma,
                       int32_t double_q, int32_t loss, double huber_delta, int32_t bootstrap, float *td_error,
                       float *td_target, void *workspace, size_t workspace_bytes, void *stream);
/* Shared-trunk actor-critic: the ascent direction of PPO's objective for ONE network whose output layer keeps two rows,
 * row 0 the policy logit z and row 1 the state value V, along a GIVEN alert schedule, reduced per group (additions to
 * ABI 18). `net` points to blocks in the TWO-HEAD layout above. The env is forced along its schedule exactly as in
 * w2a_surrogate_gradient_mlp_gated (the same bitmap, the same attempted-versus-issued rule, the same rows o_s, the same
 * scored days m_s: a day net->require_budget forces, or allowed_days closes, is attempted as 0 and has no policy
 * score; the value term still applies there). allowed_days = NULL: no gate, allowed_words is not read. Per group
 *   J_g     = (1 / N_g) sum_e w_e sum_s [ m_s (L^clip_s + entropy_coef H_s) - (vf_coef / 2) (T_s - V_s)^2 ]
 *   grad[g] = dJ_g/dtheta_g = (1 / N_g) sum_e sum_s ( c_pi,s dz_s/dtheta + c_v,s dV_s/dtheta ),
 *   c_pi,s  = w2a_surrogate_gradient_mlp's coefficient, statement for statement (0 where m_s = 0)
 *   c_v,s   = w_e vf_coef (T_s - V_s)
 * The value loss carries the factor 1/2: stable-baselines3 takes vf_coef * mean (T - V)^2, whose gradient is twice this
 * one's, so its vf_coef = 0.5 is vf_coef = 1.0 here.
 * COLLECT (advantage, value_target and old_log_prob all NULL): the rewards are formed by w2a_value_gradient_mlp_gae's
 * statements, delta_s = r_s + gamma Vn_s - V_s and A_s = delta_s + gamma lambda A_{s+1} come from the net's own row 1
 * (Vn_s and bootstrap as there), T_s = A_s + V_s, rho_s = 1, nothing is clipped and T_s - V_s = A_s.
 *   advantage_out, value_target_out, log_prob_out   f32 [n_steps][num_envs] by call-day and ENV ID, required: A_s and
 *               T_s on stepped days, log pi(a_s | z_s) on scored days, 0 elsewhere (zero-filled on `stream` first).
 *               Bit for bit w2a_value_gradient_mlp_gae's advantage / value_target for the one-output net (hidden layers
 *               and row 1) and w2a_surrogate_gradient_mlp's log_prob for (hidden layers and row 0).
 *   ret         f32 [num_envs], required: sum_s r_s (undiscounted)
 *   grad        NULL: the first pass and the backward sweep alone (the arrays above and the per-env sums)
 * EPOCH (all three given, f32 [>= n_steps][num_envs] by call-day and env id, *_days rows each): advantages and targets
 * are fixed, rho_s = exp(lp_s - old_log_prob[s, e]) and the clip test are formed in the kernel, no reward is formed.
 * advantage_out, value_target_out, log_prob_out and ret must be NULL, gamma = lambda = 1 and bootstrap = 0.
 * Both modes:
 *   grad        device f32 [n_groups][W2A_MLP_HEADS_STRIDE(width, n_layers)] in the two-head layout; a group without
 *               envs gives a block of NaN; envs finished on entry contribute zero and count
 *   surrogate, approx_kl, entropy f32 [num_envs], clipped_days, days i32 [num_envs]: as w2a_surrogate_gradient_mlp
 *   value_loss  f32 [num_envs]: sum_s 1/2 (T_s - V_s)^2, unweighted by vf_coef
 *   workspace   w2a_actor_critic_mlp_workspace_bytes(...) bytes, 256-B aligned: the layout of w2a_q_gradient_mlp (the
 *               partial blocks at the two-head stride) followed by one f32 column [n_steps][num_envs], rounded up to
 *               256 B, that holds z_s between a collect call's kernels. A smaller one is refused; nothing is written
 *               past it.
 * Numerics contract: both rows of a day come from ONE evaluation of the hidden layers and are, bit for bit, the f32
 * logits k_rollout_mlp forms for the two one-output nets. delta_s is stored as f32; A_s, lp_s, rho_s, the clip test, the
 * entropy and both coefficients are fp64; c_pi,s and c_v,s are rounded to f32 once and the second pass (one row
 * rebuild, one forward, one backward: dh_last = (c_pi w_out0 + c_v w_out1) act') is w2a_policy_gradient_mlp's with both
 * output rows fed; the fp64 sums over tiles and the reduction run unchanged. No atomics: identical calls give
 * identical bits. Nothing is written but the outputs and the workspace.
 * W2A_ERR_ARG for a NULL handle first, then where w2a_surrogate_gradient_mlp_gated refuses, in its order (the inputs'
 * checks include: one or two of the three epoch arrays, outputs that the mode does not form, gamma or lambda outside
 * [0, 1], a vf_coef that is negative or not finite); W2A_ERR_STATE while `stream` is recording a hipGraph. */
size_t w2a_actor_critic_mlp_workspace_bytes(int64_t num_envs, int32_t n_steps, int32_t n_groups, int32_t width,
                                            int32_t n_layers);
int w2a_actor_critic_mlp(w2a_env *env, const w2a_mlp_policy *net, const uint32_t *alert_mask, int32_t mask_words,
                         const float *env_weight, const float *advantage, int32_t advantage_days,
                         const float *value_target, int32_t value_target_days, const float *old_log_prob,
                         int32_t old_log_prob_days, double clip, double vf_coef, double entropy_coef, double gamma,
                         double lambda, int32_t bootstrap, int32_t n_steps, const float *obs, float *grad,
                         float *surrogate, float *value_loss, int32_t *clipped_days, float *approx_kl, float *entropy,
                         int32_t *days, float *ret, float *advantage_out, float *value_target_out, float *log_prob_out,
                         void *workspace, size_t workspace_bytes, void *stream, const uint32_t *allowed_days,
                         int32_t allowed_words);

/* Lookahead: learned policies that see the coming days' weather (the older reference env's incorp_forecasts / "D3" /
 * "D10" inputs with zero forecast error; additions to ABI 18, nothing above changes). The row an agent holds on env day
 * t is the table row of day r = max(t - 1, 0) (Q6). The w2a_lookahead_* entry points give its decision `days` more inputs
 *     f_k = h(r + k) - h(r),   k = 1 .. days,       f_k = 0 where r + k >= n_days of that env,
 * h(d) the f32 value of one table-sourced feature on day d of the env's episode, the difference one f32 subtraction.
 *   series  device f32 [S_w * Y][stride]: h of every feature row (county_w * Y + year_i), one episode's days
 *           contiguous (the feature's column of X, transposed); stride >= T floats
 *   days    1 .. W2A_LOOKAHEAD_MAX_DAYS
 *   weight  linear kind: device f32 [n_groups][W2A_LOOKAHEAD_PAD], k = 1 first, entries past `days` ignored. The logit
 *           is w2a_rollout_linear's fp64 chain (bias, slots 0..29) continued by `days` more fp64 FMAs in order of k.
 *           mlp kind: NULL; every block of `params` has W2A_MLP_LOOKAHEAD_STRIDE floats, the block above with
 *           W1f[W2A_LOOKAHEAD_PAD][width] appended (row k - 1: input f_k, zero past `days` and past the real width),
 *           and nothing before the tail moves. The first layer runs its 8 k-steps over the slots and then
 *           ceil(days / 4) more over the lookahead inputs, in that order.
 * The first decision's inputs are rebuilt from the state and `series` on entry, so calls of k and S - k days equal one
 * of S days; with all lookahead weights zero every output, the state and obs are the bits of the call without them.
 * w2a_lookahead_rollout_linear / w2a_lookahead_rollout_mlp take w2a_rollout_linear's / w2a_rollout_mlp's arguments
 * and the block; the _gated forms also the gate of w2a_rollout_*_gated. No trajectory is recorded.
 * w2a_lookahead_policy_gradient_linear and w2a_lookahead_imitation_gradient_linear take the arguments of
 * w2a_policy_gradient_linear_gated / w2a_imitation_gradient_linear_gated with allowed_days nullable (NULL: no gate);
 * grad is f32 [n_obs + 1 + days][num_envs], the lookahead inputs' rows after the bias row, k = 1 first.
 * W2A_ERR_ARG where the entry point without lookahead refuses, then for a NULL block or series, days outside the
 * range, stride < T and (linear) a NULL weight. */
#define W2A_LOOKAHEAD_MAX_DAYS 10
#define W2A_LOOKAHEAD_PAD 12
#define W2A_MLP_LOOKAHEAD_STRIDE(width, n_layers) (W2A_MLP_STRIDE(width, n_layers) + W2A_LOOKAHEAD_PAD * (width))
typedef struct w2a_lookahead {
  const float *series;
  int32_t stride;
  int32_t days;
  const float *weight;
} w2a_lookahead;
int w2a_lookahead_rollout_linear(w2a_env *env, const w2a_linear_policy *policy, int32_t n_steps, float *obs,
                                 float *ret_out, int32_t *alerts_out, int32_t *attempts_over_budget,
                                 uint32_t *alert_mask, uint32_t *attempt_mask, int32_t mask_words, float *last_return,
                                 float *ret_snapshot, void *stream, const w2a_lookahead *lookahead);
int w2a_lookahead_rollout_linear_gated(w2a_env *env, const w2a_linear_policy *policy, int32_t n_steps, float *obs,
                                       float *ret_out, int32_t *alerts_out, int32_t *attempts_over_budget,
                                       uint32_t *alert_mask, uint32_t *attempt_mask, int32_t mask_words,
                                       float *last_return, float *ret_snapshot, void *stream,
                                       const w2a_lookahead *lookahead, const uint32_t *allowed_days,
                                       int32_t allowed_words);
int w2a_lookahead_rollout_mlp(w2a_env *env, const w2a_mlp_policy *policy, int32_t n_steps, float *obs, float *ret_out,
                              int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask,
                              uint32_t *attempt_mask, int32_t mask_words, float *last_return, float *ret_snapshot,
                              void *stream, const w2a_lookahead *lookahead);
int w2a_lookahead_rollout_mlp_gated(w2a_env *env, const w2a_mlp_policy *policy, int32_t n_steps, float *obs,
                                    float *ret_out, int32_t *alerts_out, int32_t *attempts_over_budget,
                                    uint32_t *alert_mask, uint32_t *attempt_mask, int32_t mask_words,
                                    float *last_return, float *ret_snapshot, void *stream,
                                    const w2a_lookahead *lookahead, const uint32_t *allowed_days,
                                    int32_t allowed_words);
int w2a_lookahead_policy_gradient_linear(w2a_env *env, const w2a_linear_policy *policy, int32_t baseline,
                                         int32_t n_steps, const float *obs, float *grad, void *workspace,
                                         size_t workspace_bytes, void *stream, const w2a_lookahead *lookahead,
                                         const uint32_t *allowed_days, int32_t allowed_words);
int w2a_lookahead_imitation_gradient_linear(w2a_env *env, const w2a_linear_policy *policy, const uint32_t *alert_mask,
                                            int32_t mask_words, const float *env_weight, const float *day_weight,
                                            int32_t day_weight_days, int32_t n_steps, const float *obs, float *grad,
                                            float *loglik, int32_t *days, void *stream,
                                            const w2a_lookahead *lookahead, const uint32_t *allowed_days,
                                            int32_t allowed_words);

/* Forecast error: lookahead inputs as the older reference env forms them with forecast_error > 0 (its default; additions
 * to ABI 18, nothing above changes). The w2a_forecast_* entry points take a w2a_lookahead block and a w2a_forecast_error
 * block (host memory, read during the call). For the held row's day r and lead k = 1 .. days,
 *     f_k = fmaf(U(r, k), mae[k - 1], h(r + k)) - h(r)     one f32 fma, then one f32 subtraction; h(r) itself is exact
 *     f_k = +0 where r + k >= n_days of that env (no noise)
 * and where mae[k - 1] == 0 the term is skipped, h(r + k) is taken as it is (the fma would turn a -0 into +0): with
 * every entry zero the inputs, and so every output, are the bits of the w2a_lookahead_* call, for every finite h.
 *     U(r, k) = (float)(word >> 8) * 2^-23 - 1.0f       24 bits, exact in f32, in [-1, 1 - 2^-23]
 *     x       = w2a_mix64(stream + (uint64_t)(8 * r + ((k - 1) >> 1) + 1) * 0x9E3779B97F4A7C15)
 *     word    = x >> 32 for odd k, (uint32_t)x for even k          (one hash serves the two leads 2j + 1, 2j + 2)
 *     stream  = rng_stream(seed ^ 0xC3C3C3C33C3C3C3C, env_gid0 + env id, episode number)
 * with w2a_mix64 / rng_stream the pair of the device reset and of the Bernoulli policies, whose stream uses another
 * constant: equal seeds still give independent draws. A draw depends on (seed, global env id, episode number, held
 * day, lead) and on nothing else -- not on the schedule, the call boundaries, the visiting order or the shard. So calls
 * of k and S - k days equal one of S days, the gradient kernels' passes see the rollout's inputs, and handles that
 * cover the same global ids draw the same noise.
 *   mae   mean absolute error per lead in the feature's own units, >= 0 and finite for the first `days` entries (the
 *         reference's profile for a feature in degrees: 2.5, 3.0, .., 7.0); later entries are not read
 *   seed  any value
 * w2a_forecast_rollout_linear / w2a_forecast_rollout_mlp: the arguments of w2a_lookahead_rollout_*_gated with
 * allowed_days nullable (NULL: no gate) and the block. w2a_forecast_policy_gradient_linear /
 * w2a_forecast_imitation_gradient_linear: the arguments of their w2a_lookahead_* forms and the block.
 * w2a_forecast_features writes out = device f32 [num_envs][days], the inputs of the rows the envs hold now (weight is
 * not read); it changes no state.
 * W2A_ERR_ARG where the w2a_lookahead_* form refuses (same order), then for a NULL block, then for a negative or
 * non-finite mae among the first `days`. */
typedef struct w2a_forecast_error {
  float mae[W2A_LOOKAHEAD_PAD];
  uint64_t seed;
} w2a_forecast_error;
int w2a_forecast_rollout_linear(w2a_env *env, const w2a_linear_policy *policy, int32_t n_steps, float *obs,
                                float *ret_out, int32_t *alerts_out, int32_t *attempts_over_budget,
                                uint32_t *alert_mask, uint32_t *attempt_mask, int32_t mask_words, float *last_return,
                                float *ret_snapshot, void *stream, const w2a_lookahead *lookahead,
                                const uint32_t *allowed_days, int32_t allowed_words, const w2a_forecast_error *error);
int w2a_forecast_rollout_mlp(w2a_env *env, const w2a_mlp_policy *policy, int32_t n_steps, float *obs, float *ret_out,
                             int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_mask,
                             uint32_t *attempt_mask, int32_t mask_words, float *last_return, float *ret_snapshot,
                             void *stream, const w2a_lookahead *lookahead, const uint32_t *allowed_days,
                             int32_t allowed_words, const w2a_forecast_error *error);
int w2a_forecast_policy_gradient_linear(w2a_env *env, const w2a_linear_policy *policy, int32_t baseline,
                                        int32_t n_steps, const float *obs, float *grad, void *workspace,
                                        size_t workspace_bytes, void *stream, const w2a_lookahead *lookahead,
                                        const uint32_t *allowed_days, int32_t allowed_words,
                                        const w2a_forecast_error *error);
int w2a_forecast_imitation_gradient_linear(w2a_env *env, const w2a_linear_policy *policy, const uint32_t *alert_mask,
                                           int32_t mask_words, const float *env_weight, const float *day_weight,
                                           int32_t day_weight_days, int32_t n_steps, const float *obs, float *grad,
                                           float *loglik, int32_t *days, void *stream,
                                           const w2a_lookahead *lookahead, const uint32_t *allowed_days,
                                           int32_t allowed_words, const w2a_forecast_error *error);
int w2a_forecast_features(w2a_env *env, const w2a_lookahead *lookahead, const w2a_forecast_error *error, float *out,
                          void *stream);

/* Hindsight values along a GIVEN schedule (additions to ABI 18, nothing above changes): what the DP of
 * w2a_hindsight_optimum says in the states a caller's schedule reaches, not only on the optimum's own path -- the
 * expert labels of DAgger / hindsight relabelling and the share of every day's decision in the regret.
 * The env is walked from `start` along alert_mask for H = min(n_steps, n_days - t) days. The bits are ATTEMPTS: with
 * allowed_days an attempt on a closed day is 0 before the budget test, and an attempt with used + j == budget issues
 * nothing, as everywhere else. Let (j_s, streak_s) be the state on call-day s. With the recurrence, the fp64 values,
 * the bit-identical f32 rewards and the strict comparison of w2a_hindsight_optimum (under the same gate),
 *     Q0 = r0 + V_{d+1}(j, 0),    Q1 = r1 + V_{d+1}(j + 1, streak + 1)   (Q1 only while used + j < budget on an allowed day)
 *   start, n_steps   as w2a_hindsight_optimum
 *   alert_mask   device u32 [num_envs][mask_words], the schedule (w2a_rollout's or w2a_hindsight_optimum's format)
 *   allowed_days, allowed_words   nullable gate (NULL: every day is allowed and allowed_words is not read)
 *   gain_out     device f32 [min(n_steps, T)][num_envs] by call-day and ENV ID: (float)(Q1 - Q0), the difference in
 *                fp64; NaN where no alert is possible that day (budget spent, day closed) and on call-days s >= H
 *   expert_mask  device u32 [num_envs][mask_words]: bit t + s is set iff Q1 > Q0 in fp64 -- the DP's own decision in
 *                that state; 0 where no alert is possible
 *   regret_out   device f32 [num_envs]: the fp64 sum, in day order, of V_d(state) - Q_{a_s}, a_s the alert ISSUED on
 *                call-day s, rounded once: V_0(start) less what the schedule earns
 *   value_out    nullable f32 [min(n_steps, T)][num_envs]: (float)V_d(state) = max(Q0, Q1); 0 for s >= H
 *   loss_out     nullable f32 [min(n_steps, T)][num_envs]: (float)(V_d(state) - Q_{a_s}) >= 0, exactly +0 where the
 *                alert issued is the expert's bit; 0 for s >= H
 *   workspace    as w2a_hindsight_optimum: w2a_hindsight_workspace_bytes(env, n_steps, max_remaining, 1) bytes
 * Envs finished on entry (or with t >= n_days) get 0, NaN gains and an empty bitmap; a start state outside the tables
 * gives NaN in every float output and an empty bitmap.
 * Numerics contract: the backward sweep is w2a_hindsight_optimum's, statement for statement, so along that call's own
 * schedule expert_mask is the schedule, every loss is +0 and the regret is 0; the values of a state do not depend on
 * the start the DP was run from, so rows s >= k equal the rows of a call from the state reached after k days, bit for
 * bit. One lane writes each output, the regret is added by one lane in day order, and there are no atomics on outputs:
 * identical calls give identical bits.
 * Synchronises `stream` and refuses as w2a_hindsight_optimum (every refusal before any output is written); reads the
 * tables and the caller's arrays only. */
int w2a_hindsight_along(w2a_env *env, const w2a_state_view *start, int32_t n_steps, const uint32_t *alert_mask,
                        int32_t mask_words, const uint32_t *allowed_days, int32_t allowed_words, float *gain_out,
                        uint32_t *expert_mask, float *regret_out, float *value_out, float *loss_out, void *workspace,
                        size_t workspace_bytes, void *stream);
/* Imitation with the labels apart from the schedule (DAgger): the arguments of w2a_imitation_gradient_linear_gated /
 * w2a_imitation_gradient_mlp_gated with `labels`, a second bitmap in alert_mask's format, after mask_words, and
 * allowed_days nullable (NULL: no gate). The env is still forced along alert_mask -- rows, budget, streak, gate and
 * require_budget exactly as there, and the same days are scored -- while delta_s = labels_s - sigmoid(z_s) and the
 * log-likelihood term take labels_s. With labels == alert_mask every output is the sibling's, bit for bit.
 * The checks of the sibling in the same order, then W2A_ERR_ARG for NULL labels. */
int w2a_relabel_imitation_linear(w2a_env *env, const w2a_linear_policy *policy, const uint32_t *alert_mask,
                                 int32_t mask_words, const uint32_t *labels, const float *env_weight,
                                 const float *day_weight, int32_t day_weight_days, int32_t n_steps, const float *obs,
                                 float *grad, float *loglik, int32_t *days, void *stream, const uint32_t *allowed_days,
                                 int32_t allowed_words);
int w2a_relabel_imitation_mlp(w2a_env *env, const w2a_mlp_policy *policy, const uint32_t *alert_mask,
                              int32_t mask_words, const uint32_t *labels, const float *env_weight,
                              const float *day_weight, int32_t day_weight_days, int32_t n_steps, const float *obs,
                              float *grad, float *loglik, int32_t *days, void *workspace, size_t workspace_bytes,
                              void *stream, const uint32_t *allowed_days, int32_t allowed_words);

/* The hindsight budget curve (additions to ABI 18, nothing above changes): w2a_hindsight_optimum for EVERY remaining
 * budget b = 0 .. max_budget at once -- what one more alert would have been worth to each env, and where alerts stop
 * paying. The reward of a day reads the agent through alert_lag1, the streak and the REMAINING budget only, so with
 * r = alerts remaining and s = the streak one table
 *     V_d(r, s) = max( r0 + V_{d+1}(r, 0),  r1 + V_{d+1}(r - 1, s + 1) ),  V_H = 0,  the alert only while r > 0,
 * is exact for every starting budget, and column b is V_0(b, streak): the optimum over H = min(n_steps, n_days - t)
 * days from the env's start day, streak and draw HAD ITS REMAINING BUDGET AT THE START BEEN b -- w2a_hindsight_optimum
 * of the twin whose budget is used + b. The env's own budget and used are not read; budget - used selects the env's
 * own column when it is <= max_budget. (max_budget + 1)(max_budget + 2) states per day.
 *   start, n_steps  as w2a_hindsight_optimum
 *   max_budget      0 .. 1023, the same for every env of the call
 *   ret_out         device f32 [num_envs][max_budget + 1]: the return of budget b's schedule. NOT monotone in b in
 *                   general: the remaining budget enters the reward of days without an alert too
 *   alerts_out      device i32 [num_envs][max_budget + 1]: alerts in that schedule (<= b)
 *   alert_masks     NULL (mask_words is then not read), or device u32 [num_envs][max_budget + 1][mask_words]: the
 *                   schedules, in w2a_hindsight_optimum's format; mask_words * 32 >= T
 *   workspace       device memory of workspace_bytes >= w2a_hindsight_curve_workspace_bytes(env, n_steps, max_budget,
 *                   1) bytes, 256-B aligned: 256 B, and a pool only if 32 B per day + 16 B per state + 8 B per day and
 *                   64 states exceed 64 KiB of LDS (max_budget above 40 at 153 days); `big_envs` sizes the pool for that
 *                   many envs per launch (speed only)
 *   allowed_days, allowed_words  (w2a_hindsight_curve_gated) the gate of w2a_hindsight_optimum_gated: every column is
 *                   the best schedule UNDER the restriction
 * Envs finished on entry (or with t >= n_days) get rows of 0, 0 alerts and empty bitmaps; a start state outside the
 * tables gives a row of NaN, 0 alerts and empty bitmaps.
 * Numerics contract: the backward sweep is w2a_hindsight_optimum's, statement for statement, on the same reward bits
 * (rem = r without an alert, r - 1 with one: the integers that call passes for the twin), and each budget's
 * schedule is backtracked and its rewards re-added in f32 in day order as there: ret_out[e][b], alerts_out[e][b] and
 * alert_masks[e][b] are BIT-IDENTICAL to w2a_hindsight_optimum's outputs for the twin with budget = used + b (under
 * the same gate), and so to w2a_posterior_returns of that schedule. No atomics: identical calls give identical bits.
 * Synchronises `stream` once (the slot-27 flag comes to the host before anything is written), then queues its launches
 * and returns without waiting for them: max_budget is uniform, so nothing is binned on the host. Reads the tables and
 * the caller's arrays only: the handle's state and bookkeeping are untouched.
 * Refuses where w2a_hindsight_optimum refuses, in its order and before any output is written: W2A_ERR_ARG for NULL
 * pointers, n_steps <= 0, mask_words <= 0 with alert_masks, max_budget outside 0..1023 (checked on the host, before the
 * handle), mask_words * 32 < T with alert_masks, a handle with corrected-semantics flags, a workspace smaller than
 * w2a_hindsight_curve_workspace_bytes(env, n_steps, max_budget, 1), tables where some coefficient row has a nonzero
 * slot-27 term; W2A_ERR_STATE while `stream` is recording a hipGraph. w2a_hindsight_curve_workspace_bytes returns 0 for
 * a NULL handle and for arguments the entry refuses. */
size_t w2a_hindsight_curve_workspace_bytes(const w2a_env *env, int32_t n_steps, int32_t max_budget, int32_t big_envs);
int w2a_hindsight_curve(w2a_env *env, const w2a_state_view *start, int32_t n_steps, int32_t max_budget, float *ret_out,
                        int32_t *alerts_out, uint32_t *alert_masks, int32_t mask_words, void *workspace,
                        size_t workspace_bytes, void *stream);
int w2a_hindsight_curve_gated(w2a_env *env, const w2a_state_view *start, int32_t n_steps, int32_t max_budget,
                              float *ret_out, int32_t *alerts_out, uint32_t *alert_masks, int32_t mask_words,
                              void *workspace, size_t workspace_bytes, void *stream, const uint32_t *allowed_days,
                              int32_t allowed_words);

/* The hindsight optimum of the posterior mean (additions to ABI 18, nothing above changes): every env's best alert
 * schedule for a stretch of days, knowing the whole stretch's weather and its remaining budget but NOT its posterior
 * draw -- the schedule that maximises the return averaged over all n_samples draws of the env's coefficient column.
 * No policy observes the draw, so this is the bound a policy can reach, an expert whose labels are functions of what a
 * policy sees, and the yardstick of an env that pays the posterior mean.
 * The states (j, s), the transitions, the day pruning and the strict comparison are w2a_hindsight_optimum's; only the
 * reward a state weighs changes. With r_a^(i) the f32 reward an env holding draw i of the column (row coef_col *
 * n_samples + i of W) pays in that state, bit for bit, the DP weighs
 *     m_a = ( sum over i = 0 .. n_samples - 1 of (double) r_a^(i) ) / (double) n_samples,
 * the sum in fp64, sequential in i from 0, by one lane per state (no cross-lane combination, no atomics: identical
 * calls give identical bits). ret_out is the fp64 sum in day order of the chosen m_a along the backtracked path,
 * rounded once to f32. With n_samples = 1, alert_mask and alerts_out are bit-identical to w2a_hindsight_optimum's and
 * ret_out agrees to f32 rounding (that call adds in f32).
 *   start, n_steps, ret_out, alert_mask, mask_words, alerts_out, stream   as w2a_hindsight_optimum; `sample` is only
 *               range-checked (a start outside the tables gives NaN), the outputs do not depend on it
 *   workspace   device memory of workspace_bytes >= w2a_hindsight_posterior_workspace_bytes(num_envs, T, n_samples,
 *               n_steps, max_remaining, 1) bytes, 256-B aligned: w2a_hindsight_optimum's 8 B per env, and the pool
 *               from the remaining budget at which 16 B per day + 96 B per draw + 16 B per state + 8 B per day and 64
 *               states exceed 64 KiB of LDS. That function reads no handle (num_envs, T and n_samples are the
 *               handle's), is non-decreasing in n_steps and max_remaining, and returns 0 for arguments the entry
 *               refuses
 *   allowed_days, allowed_words  (w2a_hindsight_posterior_gated) the gate of w2a_hindsight_optimum_gated
 * Envs finished on entry, envs without a DP, the binning by U and the split between LDS and the pool are
 * w2a_hindsight_optimum's (the same plan and scatter kernels). Synchronises `stream` and returns after the work is
 * done. Reads the tables and the caller's arrays only: the handle's state and bookkeeping are untouched.
 * Refuses where w2a_hindsight_optimum refuses, in its order and before any output is written, and W2A_ERR_ARG for
 * tables whose n_samples is too large for the per-draw arrays (16 B per day + 96 B per draw above 64 KiB: more than
 * 657 draws at 153 days). Sampled and posterior-mean handles alike: the reward mode is not read. */
size_t w2a_hindsight_posterior_workspace_bytes(int64_t num_envs, int32_t T, int32_t n_samples, int32_t n_steps,
                                               int32_t max_remaining, int32_t big_envs);
int w2a_hindsight_posterior(w2a_env *env, const w2a_state_view *start, int32_t n_steps, float *ret_out,
                            uint32_t *alert_mask, int32_t mask_words, int32_t *alerts_out, void *workspace,
                            size_t workspace_bytes, void *stream);
int w2a_hindsight_posterior_gated(w2a_env *env, const w2a_state_view *start, int32_t n_steps, float *ret_out,
                                  uint32_t *alert_mask, int32_t mask_words, int32_t *alerts_out, void *workspace,
                                  size_t workspace_bytes, void *stream, const uint32_t *allowed_days,
                                  int32_t allowed_words);

/* Draw-blind hindsight values along a GIVEN schedule (additions to ABI 18, nothing above changes): what the DP of
 * w2a_hindsight_posterior says in the states a caller's schedule reaches, not only on its own optimal path -- DAgger
 * labels that are functions of what a policy sees, and every day's share of the regret against the bound a policy can
 * reach. w2a_hindsight_along's job on w2a_hindsight_posterior's reward: the walk, the attempts (an attempt on a closed
 * day is 0 before the budget test; an attempt with used + j == budget issues nothing), the outputs, their shapes and
 * their fills are w2a_hindsight_along's, with
 *     Q0 = m_0 + V_{d+1}(j, 0),    Q1 = m_1 + V_{d+1}(j + 1, streak + 1)   (Q1 only while used + j < budget on an allowed day)
 * and m_a the draw-mean of w2a_hindsight_posterior: the fp64 sum of the f32 rewards over the draws in draw order,
 * divided by (double) n_samples.
 *   start, n_steps, alert_mask, mask_words, allowed_days, allowed_words   as w2a_hindsight_along; `sample` is only
 *                range-checked, the outputs do not depend on it
 *   gain_out     device f32 [min(n_steps, T)][num_envs] by call-day and ENV ID: (float)(Q1 - Q0); NaN where no alert is
 *                possible that day and on call-days s >= H
 *   expert_mask  device u32 [num_envs][mask_words]: bit t + s is set iff Q1 > Q0 in fp64
 *   regret_out   device f32 [num_envs]: the fp64 sum, in day order, of V_d(state) - Q_{a_s}, a_s the alert ISSUED on
 *                call-day s, rounded once: w2a_hindsight_posterior's optimum from `start` less the schedule's
 *                posterior-mean return
 *   value_out    nullable f32 [min(n_steps, T)][num_envs]: (float)V_d(state) = max(Q0, Q1); 0 for s >= H
 *   loss_out     nullable f32 [min(n_steps, T)][num_envs]: (float)(V_d(state) - Q_{a_s}) >= 0, exactly +0 where the
 *                alert issued is the expert's bit; 0 for s >= H
 *   workspace    as w2a_hindsight_posterior: w2a_hindsight_posterior_workspace_bytes(num_envs, T, n_samples, n_steps,
 *                max_remaining, 1) bytes. The day's fp64 loss takes the room of the day's slots 28 and 29 once they
 *                have been read, so LDS, the split between LDS and the pool and the largest n_samples are that call's
 * Envs finished on entry (or with t >= n_days) get 0, NaN gains and an empty bitmap; a start state outside the tables
 * gives NaN in every float output and an empty bitmap.
 * Numerics contract: the backward sweep is w2a_hindsight_posterior's, statement for statement (one device function),
 * so along that call's own schedule expert_mask is the schedule, every loss is +0 and the regret is +0; with
 * n_samples = 1 every output is w2a_hindsight_along's bit for bit (0.0 + (double) r and x / 1.0 are exact); the
 * values of a state do not depend on the start the DP was run from, so rows s >= k equal the rows of a call from the
 * state reached after k days, bit for bit. One lane writes each output, the regret is added by one lane in day order,
 * and there are no atomics: identical calls give identical bits.
 * Synchronises `stream` and refuses as w2a_hindsight_posterior, in its order (NULL alert_mask, gain_out, expert_mask or
 * regret_out among the NULL arguments; every refusal before any output is written); reads the tables and the caller's
 * arrays only. Sampled and posterior-mean handles alike. */
int w2a_hindsight_posterior_along(w2a_env *env, const w2a_state_view *start, int32_t n_steps, const uint32_t *alert_mask,
                                  int32_t mask_words, const uint32_t *allowed_days, int32_t allowed_words,
                                  float *gain_out, uint32_t *expert_mask, float *regret_out, float *value_out,
                                  float *loss_out, void *workspace, size_t workspace_bytes, void *stream);

/* The draw-blind hindsight budget curve (additions to ABI 18, nothing above changes): w2a_hindsight_posterior for EVERY
 * remaining budget b = 0 .. max_budget at once -- the return-versus-budget curves of a decision that is taken before
 * anyone knows which posterior draw an episode will get. w2a_hindsight_curve's job on w2a_hindsight_posterior's
 * reward: the states (r = alerts remaining, s = the streak), the recurrence
 *     V_d(r, s) = max( m_0 + V_{d+1}(r, 0),  m_1 + V_{d+1}(r - 1, s + 1) ),  V_H = 0,  the alert only while r > 0,
 * the (max_budget + 1)(max_budget + 2) states per day and the strict comparison are w2a_hindsight_curve's, and m_a is
 * the draw-mean of w2a_hindsight_posterior: the fp64 sum over the draws i = 0 .. n_samples - 1, in draw order, of the
 * f32 reward an env holding draw i of the column pays in that state (rem = r without an alert, r - 1 with one),
 * divided by (double) n_samples, by one lane per state.
 *   start, n_steps, max_budget, ret_out, alerts_out, alert_masks, mask_words, stream   as w2a_hindsight_curve; `sample`
 *                   is only range-checked (a start outside the tables gives a row of NaN), the outputs do not depend
 *                   on it, and the env's own budget and used are not read
 *   workspace       device memory of workspace_bytes >= w2a_hindsight_posterior_curve_workspace_bytes(env, n_steps,
 *                   max_budget, 1) bytes, 256-B aligned: 256 B, and a pool only if 16 B per day + 96 B per draw + 16 B
 *                   per state + 8 B per day and 64 states exceed 64 KiB of LDS (always from max_budget 63);
 *                   `big_envs` sizes the pool for that many envs per launch (speed only)
 *   allowed_days, allowed_words  (w2a_hindsight_posterior_curve_gated) the gate of w2a_hindsight_optimum_gated: every
 *                   column is the best schedule UNDER the restriction
 * Envs finished on entry (or with t >= n_days) get rows of 0, 0 alerts and empty bitmaps; a start state outside the
 * tables gives a row of NaN, 0 alerts and empty bitmaps.
 * Numerics contract: the backward sweep weighs w2a_hindsight_posterior's sums statement for statement, and each
 * budget's schedule is backtracked by one lane that adds its path's rewards in draw order and the days' means in fp64
 * in day order, rounded once to f32: ret_out[e][b], alerts_out[e][b] and alert_masks[e][b] are BIT-IDENTICAL to
 * w2a_hindsight_posterior's outputs for the twin with budget = used + b (under the same gate). With n_samples = 1 the
 * alerts and the schedules are w2a_hindsight_curve's bit for bit and ret_out agrees to f32 rounding. No atomics:
 * identical calls give identical bits.
 * Synchronises `stream` once (the slot-27 flag comes to the host before anything is written), then queues its launches
 * and returns without waiting for them. Reads the tables and the caller's arrays only: the handle's state and
 * bookkeeping are untouched. Sampled and posterior-mean handles alike: the reward mode is not read.
 * Refuses where w2a_hindsight_curve refuses, in its order and before any output is written, and after the handle's
 * checks W2A_ERR_ARG for tables whose n_samples is too large for the per-draw arrays (16 B per day + 96 B per draw above
 * 64 KiB: more than 657 draws at 153 days). w2a_hindsight_posterior_curve_workspace_bytes returns 0 for a NULL handle
 * and for arguments or tables the entry refuses. */
size_t w2a_hindsight_posterior_curve_workspace_bytes(const w2a_env *env, int32_t n_steps, int32_t max_budget,
                                                     int32_t big_envs);
int w2a_hindsight_posterior_curve(w2a_env *env, const w2a_state_view *start, int32_t n_steps, int32_t max_budget,
                                  float *ret_out, int32_t *alerts_out, uint32_t *alert_masks, int32_t mask_words,
                                  void *workspace, size_t workspace_bytes, void *stream);
int w2a_hindsight_posterior_curve_gated(w2a_env *env, const w2a_state_view *start, int32_t n_steps, int32_t max_budget,
                                        float *ret_out, int32_t *alerts_out, uint32_t *alert_masks, int32_t mask_words,
                                        void *workspace, size_t workspace_bytes, void *stream,
                                        const uint32_t *allowed_days, int32_t allowed_words);

/* The policy budget curve (additions to ABI 18, nothing above changes): w2a_rollout_linear for EVERY remaining budget
 * b = 0 .. max_budget at once -- what the policy that will actually run earns with b alerts, the row of the
 * budget-curve table whose upper bounds are w2a_hindsight_curve and w2a_hindsight_posterior_curve. Column b of env e is
 * w2a_rollout_linear of the twin whose budget is used + b: the same weather, draw, counters and Bernoulli uniforms
 * (keyed by seed, env id, episode and day), require_budget and the gate as there.
 * The reward and the policy read the budget through the run-time slots 24..27 only, and the fp64 chains run in slot
 * order: per env-day the row is gathered once and the three chains run once over slots 0..23; per budget only slots
 * 24..27 from that budget's counters, then 28 and 29, the decision, the reward and the counter update.
 *   policy          as w2a_rollout_linear (weight, bias, group, n_groups, sample, require_budget, seed)
 *   start           the start state; t, streak, hist14, n_days, county_w, year_i, coef_col, sample, episode_no and
 *                   finished are read. budget and used are NOT read: the remaining budget of column b is b
 *   n_steps         days to run from every env's start day (an env stops at its episode's end)
 *   max_budget      0 .. 1023, the same for every env of the call
 *   obs             device f32 [num_envs][n_obs]: the row every env's agent holds in `start` (the first decision's
 *                   input; column b reads (float) b in place of its remaining_budget column, at that column's place in
 *                   the chain). Read only. NULL: the rows are rebuilt as a reset writes them -- day 0's table row with
 *                   lag, streak and 14-day count 0 -- which is the held row only where every live env of `start` is at
 *                   t = 0 with nothing used
 *   ret_out         device f32 [num_envs][max_budget + 1]: the rewards summed over the days run
 *   alerts_out      device i32 [num_envs][max_budget + 1]: alerts issued
 *   attempts_over_budget  device i32 [num_envs][max_budget + 1]: attempts made with no budget left
 *   alert_masks     NULL (mask_words is then not read), or device u32 [num_envs][max_budget + 1][mask_words]: the
 *                   alerts issued by day of the episode, in w2a_rollout_linear's alert_mask format; every word is
 *                   written; mask_words * 32 >= T
 *   workspace       device memory of workspace_bytes >= w2a_policy_curve_workspace_bytes(env, n_steps, max_budget)
 *                   bytes, 256-B aligned: 256 reserved bytes (the per-budget state lives in registers, the day
 *                   prefixes in LDS)
 *   allowed_days, allowed_words  (w2a_policy_curve_linear_gated) the gate of w2a_rollout_linear_gated
 * Envs finished on entry (or with t >= n_days) get rows of 0 and empty bitmaps; a start state outside the tables gives
 * a row of NaN, zero counts and empty bitmaps.
 * Numerics contract: the statements of w2a_rollout_linear in its order -- logit with the bias first and slots in slot
 * order, require_budget, the gate, the budget test, the gate flag of slot 30, the f32 sigmoids, the f32 sum of the
 * rewards in day order: ret_out[e][b], alerts_out[e][b], attempts_over_budget[e][b] and alert_masks[e][b] are
 * BIT-IDENTICAL to that call's outputs on the twin. No atomics: identical calls give identical bits.
 * Queues one launch and returns without waiting. Reads the tables and the caller's arrays only: the handle's state,
 * observation buffer and bookkeeping are untouched.
 * Refuses before anything is written: W2A_ERR_ARG for what w2a_rollout_linear refuses of the policy struct and n_steps,
 * NULL start, outputs or start-state arrays, mask_words <= 0 with alert_masks, max_budget outside 0..1023, a NULL or
 * misaligned workspace (all checked before the handle), a NULL handle, mask_words * 32 < T with alert_masks, a handle
 * with corrected-semantics flags, num_envs * n_obs >= 2^31, a workspace smaller than
 * w2a_policy_curve_workspace_bytes(env, n_steps, max_budget), a bad gate; W2A_ERR_STATE while `stream` is recording a
 * hipGraph; W2A_ERR_SCHEMA as w2a_rollout_linear. w2a_policy_curve_workspace_bytes returns 0 for a NULL handle and for
 * arguments the entry refuses. */
size_t w2a_policy_curve_workspace_bytes(const w2a_env *env, int32_t n_steps, int32_t max_budget);
int w2a_policy_curve_linear(w2a_env *env, const w2a_linear_policy *policy, const w2a_state_view *start, int32_t n_steps,
                            int32_t max_budget, const float *obs, float *ret_out, int32_t *alerts_out,
                            int32_t *attempts_over_budget, uint32_t *alert_masks, int32_t mask_words, void *workspace,
                            size_t workspace_bytes, void *stream);
int w2a_policy_curve_linear_gated(w2a_env *env, const w2a_linear_policy *policy, const w2a_state_view *start,
                                  int32_t n_steps, int32_t max_budget, const float *obs, float *ret_out,
                                  int32_t *alerts_out, int32_t *attempts_over_budget, uint32_t *alert_masks,
                                  int32_t mask_words, void *workspace, size_t workspace_bytes, void *stream,
                                  const uint32_t *allowed_days, int32_t allowed_words);

#ifdef __cplusplus
}
#endif
#endif /* W2A_H */
