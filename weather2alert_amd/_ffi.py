"""ctypes binding of include/w2a.h (libw2a.so). No fallback: a missing library is an error."""
from __future__ import annotations

import ctypes as C
import os

from . import build as _build

ROW_FLOATS = 32

OK = 0
ST_BAD_EPISODE, ST_BAD_ACTION, ST_STEP_AFTER_DONE, ST_STALE_GRAPH = 1, 2, 4, 8
ACT_I32, ACT_I64, ACT_U8 = 0, 1, 2
STEP_AUTORESET, STEP_NO_OBS, STEP_CLASSIC, STEP_REWARD_GIVEN, STEP_WIDE, STEP_SKIP_FINISHED, STEP_UNPACKED, STEP_NEXT_STEP, STEP_NO_CAPTURE = 1, 2, 8, 16, 32, 64, 128, 256, 512
S64_MIN_ENVS = 131072  # w2a_step picks the 64-envs-per-wave kernel from this batch size on (csrc/w2a_step64.hip.h)
ABI_VERSION = 18
FIX_BITS = {"alert_2wks": 1, "lag": 2, "penalty": 4, "obs": 8, "augment": 16}  # + "budget" (sticky = 0)
BUDGET_FIXED, BUDGET_LESS_THAN, BUDGET_CENTERED = 0, 1, 2

# every symbol include/w2a.h declares (checked by tests/test_abi.py against the header text)
SYMBOLS = [
    "w2a_abi_version", "w2a_last_error", "w2a_state_bytes", "w2a_create", "w2a_destroy", "w2a_reset",
    "w2a_reset_device_rng", "w2a_set_autoreset", "w2a_step", "w2a_get_state", "w2a_read_status",
    "w2a_sort_workspace_bytes", "w2a_sort_episodes", "w2a_reset_device_rng_sorted", "w2a_observe", "w2a_rollout", "w2a_rollout_order_workspace_bytes", "w2a_rollout_order_attach", "w2a_rollout_order", "w2a_rollout_posterior_mean", "w2a_policy_actions", "w2a_set_semantics",
    "w2a_group_workspace_bytes", "w2a_group_by_column", "w2a_posterior_mean_reward", "w2a_set_posterior_kernel", "w2a_set_episode_word", "w2a_invalidate", "w2a_query", "w2a_rollout_mfma_workspace_bytes", "w2a_rollout_mfma_prepare",
    "w2a_rollout_linear", "w2a_rollout_mlp", "w2a_rollout_linear_record", "w2a_rollout_mlp_record",
    "w2a_posterior_returns", "w2a_hindsight_workspace_bytes", "w2a_hindsight_optimum",
    "w2a_policy_gradient_workspace_bytes", "w2a_policy_gradient_linear",
    "w2a_policy_gradient_mlp_workspace_bytes", "w2a_policy_gradient_mlp",
    "w2a_imitation_gradient_linear", "w2a_imitation_gradient_mlp_workspace_bytes", "w2a_imitation_gradient_mlp",
    "w2a_imitation_gradient_linear_weighted", "w2a_imitation_gradient_mlp_weighted",
    "w2a_value_gradient_linear_workspace_bytes", "w2a_value_gradient_linear",
    "w2a_value_gradient_mlp_workspace_bytes", "w2a_value_gradient_mlp",
    "w2a_value_gradient_linear_gae_workspace_bytes", "w2a_value_gradient_linear_gae",
    "w2a_value_gradient_mlp_gae_workspace_bytes", "w2a_value_gradient_mlp_gae",
    "w2a_surrogate_gradient_linear", "w2a_surrogate_gradient_mlp_workspace_bytes", "w2a_surrogate_gradient_mlp",
    "w2a_alert_gate", "w2a_rollout_linear_gated", "w2a_policy_gradient_linear_gated",
    "w2a_imitation_gradient_linear_gated", "w2a_surrogate_gradient_linear_gated", "w2a_hindsight_optimum_gated",
    "w2a_rollout_mlp_gated", "w2a_policy_gradient_mlp_gated", "w2a_imitation_gradient_mlp_gated",
    "w2a_surrogate_gradient_mlp_gated",
    "w2a_fisher_vector_product_linear", "w2a_fisher_vector_product_mlp_workspace_bytes",
    "w2a_fisher_vector_product_mlp",
    "w2a_q_gradient_mlp_workspace_bytes", "w2a_q_gradient_mlp",
    "w2a_actor_critic_mlp_workspace_bytes", "w2a_actor_critic_mlp",
    "w2a_lookahead_rollout_linear", "w2a_lookahead_rollout_linear_gated", "w2a_lookahead_rollout_mlp",
    "w2a_lookahead_rollout_mlp_gated", "w2a_lookahead_policy_gradient_linear",
    "w2a_lookahead_imitation_gradient_linear",
    "w2a_forecast_rollout_linear", "w2a_forecast_rollout_mlp", "w2a_forecast_policy_gradient_linear",
    "w2a_forecast_imitation_gradient_linear", "w2a_forecast_features",
    "w2a_hindsight_along", "w2a_relabel_imitation_linear", "w2a_relabel_imitation_mlp",
    "w2a_hindsight_curve_workspace_bytes", "w2a_hindsight_curve", "w2a_hindsight_curve_gated",
    "w2a_hindsight_posterior_workspace_bytes", "w2a_hindsight_posterior", "w2a_hindsight_posterior_gated",
    "w2a_hindsight_posterior_along",
    "w2a_hindsight_posterior_curve_workspace_bytes", "w2a_hindsight_posterior_curve",
    "w2a_hindsight_posterior_curve_gated",
    "w2a_policy_curve_workspace_bytes", "w2a_policy_curve_linear", "w2a_policy_curve_linear_gated",
]
Q_LOCKSTEP_DAY, Q_PACKED_ELIGIBLE, Q_PACKED_CURRENT, Q_CANONICAL_CURRENT, Q_LAST_ROLLOUT_KERNEL, Q_LAST_STEP_KERNEL, Q_LOCKSTEP = 0, 1, 2, 3, 4, 5, 6
Q_EPISODE_WORD_BYTES = 7
ROLLOUT_KERNELS = {0: "k_rollout", 1: "k_rollout64", 2: "k_rollout_mfma", 3: "k_rollout_linear", 4: "k_rollout_mlp"}  # W2A_Q_LAST_ROLLOUT_KERNEL
PM_KERNELS = {"vector": 0, "matrix": 1, "matrix_i8": 2}  # W2A_PM_VECTOR, W2A_PM_MATRIX_F64, W2A_PM_MATRIX_I8
POLICY_KINDS = {"never": 0, "always": 1, "bernoulli": 2, "threshold": 3, "table": 4}


class Policy(C.Structure):
    _fields_ = [("kind", C.c_int32), ("p", C.c_float), ("obs_col", C.c_int32), ("threshold", C.c_float),
                ("obs_lag", C.c_int32), ("require_budget", C.c_int32), ("table", C.c_void_p),
                ("table_R", C.c_int32), ("seed", C.c_uint64)]


class LinearPolicy(C.Structure):
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("group", C.c_void_p), ("n_groups", C.c_int32),
                ("sample", C.c_int32), ("require_budget", C.c_int32), ("seed", C.c_uint64)]


class MlpPolicy(C.Structure):
    _fields_ = [("params", C.c_void_p), ("group", C.c_void_p), ("order", C.c_void_p), ("n_groups", C.c_int32),
                ("n_layers", C.c_int32), ("width", C.c_int32), ("activation", C.c_int32), ("sample", C.c_int32),
                ("require_budget", C.c_int32), ("seed", C.c_uint64)]


class Lookahead(C.Structure):
    """w2a_lookahead: the series table, its stride, D and (linear kind) the lookahead weights [G][12]."""
    _fields_ = [("series", C.c_void_p), ("stride", C.c_int32), ("days", C.c_int32), ("weight", C.c_void_p)]


class ForecastError(C.Structure):
    """w2a_forecast_error: the MAE of every lead (k = 1 first, the first D entries are read) and the error seed."""
    _fields_ = [("mae", C.c_float * 12), ("seed", C.c_uint64)]


MLP_ACTIVATIONS = {"tanh": 0, "relu": 1}  # W2A_MLP_TANH, W2A_MLP_RELU


class Trajectory(C.Structure):
    """w2a_trajectory: device arrays [call-day][env] of w2a_rollout_*_record (include/w2a.h)."""
    _fields_ = [("obs", C.c_void_p), ("logit", C.c_void_p), ("reward", C.c_void_p), ("action", C.c_void_p),
                ("flags", C.c_void_p)]


TRAJ_VALID, TRAJ_TERMINATED, TRAJ_ALERT = 1, 2, 4  # W2A_TRAJ_* flag bits
Q_LOSSES = {"squared": 0, "huber": 1}  # W2A_Q_LOSS_SQUARED, W2A_Q_LOSS_HUBER
PG_BASELINES = {"none": 0, "no_alert": 1}  # W2A_PG_BASELINE_NONE, W2A_PG_BASELINE_NO_ALERT


class Tables(C.Structure):
    _fields_ = [
        ("X", C.c_void_p), ("n_days", C.c_void_p), ("B0", C.c_void_p), ("W", C.c_void_p),
        ("fips_to_weather", C.c_void_p), ("sim_cnt", C.c_void_p),
        ("T", C.c_int32), ("S_w", C.c_int32), ("Y", C.c_int32), ("S", C.c_int32), ("n_samples", C.c_int32),
        ("n_obs", C.c_int32), ("obs_slot", C.c_int32 * ROW_FLOATS), ("slot_heat_qi", C.c_int32),
        ("sim_ptr", C.c_void_p), ("sim_idx", C.c_void_p), ("slot_alerts_2wks", C.c_int32),
        ("gate_bits", C.c_void_p), ("gate_words", C.c_int32),
    ]


STATE_FIELDS = ["t", "used", "streak", "hist14", "last_actual", "at_budget", "budget", "n_days", "county_w",
                "year_i", "coef_col", "sample", "sticky_budget", "episode_no", "finished", "episode_return"]


class StateView(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in STATE_FIELDS]


class W2AError(RuntimeError):
    pass


_lib = None


def lib_path() -> str:
    # W2A_LIB: load another build of the library instead of the in-tree one (tools/mutation_fuzz.py: deliberately broken
    # builds that the call-sequence fuzz has to catch). Never set in normal use.
    return os.environ.get("W2A_LIB") or _build.LIB


def load(build_if_missing: bool = True):
    """Load libw2a.so (building it with hipcc first when the sources are newer)."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if build_if_missing and not os.environ.get("W2A_LIB") and _build.needs_build():
        try:
            _build.build_lib()
        except Exception as e:  # noqa: BLE001
            # never fall back to an older library when its sources have changed: the ABI version check below would
            # accept a stale .so whose kernels differ from the sources in the tree
            raise W2AError(f"libw2a.so is out of date (or missing) and could not be rebuilt: {e}") from e
    if not os.path.exists(path):
        raise W2AError(f"{path} not found: run `python -m weather2alert_amd.build` (there is no CPU fallback)")
    lib = C.CDLL(path)
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    lib.w2a_abi_version.restype = C.c_int
    lib.w2a_abi_version.argtypes = []
    lib.w2a_last_error.restype = C.c_char_p
    lib.w2a_last_error.argtypes = []
    lib.w2a_state_bytes.restype = C.c_size_t
    lib.w2a_state_bytes.argtypes = [i64]
    lib.w2a_create.restype = C.c_int
    lib.w2a_create.argtypes = [C.POINTER(Tables), i64, i64, vp, C.c_size_t, vp, C.POINTER(vp)]
    lib.w2a_destroy.restype = None
    lib.w2a_destroy.argtypes = [vp]
    lib.w2a_reset.restype = C.c_int
    lib.w2a_reset.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.w2a_reset_device_rng.restype = C.c_int
    lib.w2a_reset_device_rng.argtypes = [vp, u64, i32, C.c_int, i32, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    lib.w2a_set_autoreset.restype = C.c_int
    lib.w2a_set_autoreset.argtypes = [vp, u64, i32, C.c_int, i32, C.c_int, C.c_int]
    lib.w2a_step.restype = C.c_int
    lib.w2a_step.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp]
    lib.w2a_get_state.restype = C.c_int
    lib.w2a_get_state.argtypes = [vp, C.POINTER(StateView), vp]
    lib.w2a_read_status.restype = C.c_int
    lib.w2a_read_status.argtypes = [vp, C.POINTER(i32), vp]
    lib.w2a_sort_workspace_bytes.restype = C.c_size_t
    lib.w2a_sort_workspace_bytes.argtypes = [i64]
    lib.w2a_sort_episodes.restype = C.c_int
    lib.w2a_sort_episodes.argtypes = [vp, vp, C.c_size_t, vp]
    lib.w2a_reset_device_rng_sorted.restype = C.c_int
    lib.w2a_reset_device_rng_sorted.argtypes = [vp, u64, i32, C.c_int, i32, C.c_int, C.c_int, C.c_int, vp, vp, C.c_size_t, vp]
    lib.w2a_group_workspace_bytes.restype = C.c_size_t
    lib.w2a_group_workspace_bytes.argtypes = [i64, C.c_int32, C.c_int32]
    lib.w2a_group_by_column.restype = C.c_int
    lib.w2a_group_by_column.argtypes = [vp, vp, C.c_size_t, vp]
    lib.w2a_posterior_mean_reward.restype = C.c_int
    lib.w2a_posterior_mean_reward.argtypes = [vp, vp, C.c_int, vp, vp]
    lib.w2a_set_posterior_kernel.restype = C.c_int
    lib.w2a_set_posterior_kernel.argtypes = [vp, C.c_int]
    lib.w2a_set_episode_word.restype = C.c_int
    lib.w2a_set_episode_word.argtypes = [vp, C.c_int]
    lib.w2a_rollout_mfma_workspace_bytes.restype = C.c_size_t
    lib.w2a_rollout_mfma_workspace_bytes.argtypes = [i64, i64, i32, i32]
    lib.w2a_rollout_mfma_prepare.restype = C.c_int
    lib.w2a_rollout_mfma_prepare.argtypes = [vp, vp, C.c_size_t, vp]
    lib.w2a_query.restype = C.c_int
    lib.w2a_query.argtypes = [vp, C.c_int]
    lib.w2a_invalidate.restype = C.c_int
    lib.w2a_invalidate.argtypes = [vp, vp]
    lib.w2a_observe.restype = C.c_int
    lib.w2a_observe.argtypes = [vp, vp, vp]
    lib.w2a_set_semantics.restype = C.c_int
    lib.w2a_set_semantics.argtypes = [vp, C.c_uint32]
    lib.w2a_rollout.restype = C.c_int
    lib.w2a_rollout.argtypes = [vp, C.POINTER(Policy), i32, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    lib.w2a_rollout_order_workspace_bytes.restype = C.c_size_t
    lib.w2a_rollout_order_workspace_bytes.argtypes = [i64, i64]
    lib.w2a_rollout_order.restype = C.c_int
    lib.w2a_rollout_order.argtypes = [vp, vp, C.c_size_t, vp]
    lib.w2a_rollout_order_attach.restype = C.c_int
    lib.w2a_rollout_order_attach.argtypes = [vp, vp, C.c_size_t]
    lib.w2a_rollout_posterior_mean.restype = C.c_int
    lib.w2a_rollout_posterior_mean.argtypes = [vp, C.POINTER(Policy), i32, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    lib.w2a_rollout_linear.restype = C.c_int
    lib.w2a_rollout_linear.argtypes = [vp, C.POINTER(LinearPolicy), i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    lib.w2a_rollout_mlp.restype = C.c_int
    lib.w2a_rollout_mlp.argtypes = [vp, C.POINTER(MlpPolicy), i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    lib.w2a_rollout_linear_record.restype = C.c_int
    lib.w2a_rollout_linear_record.argtypes = lib.w2a_rollout_linear.argtypes + [C.POINTER(Trajectory)]
    lib.w2a_rollout_mlp_record.restype = C.c_int
    lib.w2a_rollout_mlp_record.argtypes = lib.w2a_rollout_mlp.argtypes + [C.POINTER(Trajectory)]
    lib.w2a_posterior_returns.restype = C.c_int
    lib.w2a_posterior_returns.argtypes = [vp, C.POINTER(StateView), vp, i32, i32, vp, vp]
    lib.w2a_hindsight_workspace_bytes.restype = C.c_size_t
    lib.w2a_hindsight_workspace_bytes.argtypes = [vp, i32, i32, i32]
    lib.w2a_hindsight_optimum.restype = C.c_int
    lib.w2a_hindsight_optimum.argtypes = [vp, C.POINTER(StateView), i32, vp, vp, i32, vp, vp, C.c_size_t, vp]
    lib.w2a_policy_gradient_workspace_bytes.restype = C.c_size_t
    lib.w2a_policy_gradient_workspace_bytes.argtypes = [i64, i32]
    lib.w2a_policy_gradient_linear.restype = C.c_int
    lib.w2a_policy_gradient_linear.argtypes = [vp, C.POINTER(LinearPolicy), i32, i32, vp, vp, vp, C.c_size_t, vp]
    lib.w2a_policy_gradient_mlp_workspace_bytes.restype = C.c_size_t
    lib.w2a_policy_gradient_mlp_workspace_bytes.argtypes = [i64, i32, i32, i32, i32]
    lib.w2a_policy_gradient_mlp.restype = C.c_int
    lib.w2a_policy_gradient_mlp.argtypes = [vp, C.POINTER(MlpPolicy), i32, i32, vp, vp, vp, C.c_size_t, vp]
    lib.w2a_imitation_gradient_linear.restype = C.c_int
    lib.w2a_imitation_gradient_linear.argtypes = [vp, C.POINTER(LinearPolicy), vp, i32, vp, i32, vp, vp, vp, vp, vp]
    lib.w2a_imitation_gradient_mlp_workspace_bytes.restype = C.c_size_t
    lib.w2a_imitation_gradient_mlp_workspace_bytes.argtypes = [i64, i32, i32, i32, i32]
    lib.w2a_imitation_gradient_mlp.restype = C.c_int
    lib.w2a_imitation_gradient_mlp.argtypes = [vp, C.POINTER(MlpPolicy), vp, i32, vp, i32, vp, vp, vp, vp, vp, C.c_size_t, vp]
    lib.w2a_imitation_gradient_linear_weighted.restype = C.c_int
    lib.w2a_imitation_gradient_linear_weighted.argtypes = [vp, C.POINTER(LinearPolicy), vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    lib.w2a_imitation_gradient_mlp_weighted.restype = C.c_int
    lib.w2a_imitation_gradient_mlp_weighted.argtypes = [vp, C.POINTER(MlpPolicy), vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, C.c_size_t, vp]
    lib.w2a_value_gradient_linear_workspace_bytes.restype = C.c_size_t
    lib.w2a_value_gradient_linear_workspace_bytes.argtypes = [i64, i32]
    lib.w2a_value_gradient_linear.restype = C.c_int
    lib.w2a_value_gradient_linear.argtypes = [vp, C.POINTER(LinearPolicy), vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    lib.w2a_value_gradient_mlp_workspace_bytes.restype = C.c_size_t
    lib.w2a_value_gradient_mlp_workspace_bytes.argtypes = [i64, i32, i32, i32, i32]
    lib.w2a_value_gradient_mlp.restype = C.c_int
    lib.w2a_value_gradient_mlp.argtypes = [vp, C.POINTER(MlpPolicy), vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    gae = [C.c_double, C.c_double, i32, vp, vp, i32]  # gamma, lambda, bootstrap, value_target, target, target_days
    lib.w2a_value_gradient_linear_gae_workspace_bytes.restype = C.c_size_t
    lib.w2a_value_gradient_linear_gae_workspace_bytes.argtypes = [i64, i32]
    lib.w2a_value_gradient_linear_gae.restype = C.c_int
    lib.w2a_value_gradient_linear_gae.argtypes = [vp, C.POINTER(LinearPolicy), vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, *gae, vp, C.c_size_t, vp]
    lib.w2a_value_gradient_mlp_gae_workspace_bytes.restype = C.c_size_t
    lib.w2a_value_gradient_mlp_gae_workspace_bytes.argtypes = [i64, i32, i32, i32, i32]
    lib.w2a_value_gradient_mlp_gae.restype = C.c_int
    lib.w2a_value_gradient_mlp_gae.argtypes = [vp, C.POINTER(MlpPolicy), vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, *gae, vp, C.c_size_t, vp]
    lib.w2a_surrogate_gradient_linear.restype = C.c_int
    lib.w2a_surrogate_gradient_linear.argtypes = [vp, C.POINTER(LinearPolicy), vp, i32, vp, vp, i32, vp, i32, C.c_double,
                                                  C.c_double, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.w2a_surrogate_gradient_mlp_workspace_bytes.restype = C.c_size_t
    lib.w2a_surrogate_gradient_mlp_workspace_bytes.argtypes = [i64, i32, i32, i32, i32]
    lib.w2a_surrogate_gradient_mlp.restype = C.c_int
    lib.w2a_surrogate_gradient_mlp.argtypes = [vp, C.POINTER(MlpPolicy), vp, i32, vp, vp, i32, vp, i32, C.c_double,
                                               C.c_double, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    # alert gates: the arguments of the entry point each is named after, then the allowed-days bitmap and its word count
    gate = [vp, i32]
    lib.w2a_alert_gate.restype = C.c_int
    lib.w2a_alert_gate.argtypes = [vp, i32, C.c_float, vp, i32, vp, i32, vp]
    lib.w2a_rollout_linear_gated.restype = C.c_int
    lib.w2a_rollout_linear_gated.argtypes = lib.w2a_rollout_linear.argtypes + [C.POINTER(Trajectory)] + gate
    lib.w2a_policy_gradient_linear_gated.restype = C.c_int
    lib.w2a_policy_gradient_linear_gated.argtypes = lib.w2a_policy_gradient_linear.argtypes + gate
    lib.w2a_imitation_gradient_linear_gated.restype = C.c_int
    lib.w2a_imitation_gradient_linear_gated.argtypes = lib.w2a_imitation_gradient_linear_weighted.argtypes + gate
    lib.w2a_surrogate_gradient_linear_gated.restype = C.c_int
    lib.w2a_surrogate_gradient_linear_gated.argtypes = lib.w2a_surrogate_gradient_linear.argtypes + gate
    lib.w2a_rollout_mlp_gated.restype = C.c_int
    lib.w2a_rollout_mlp_gated.argtypes = lib.w2a_rollout_mlp.argtypes + [C.POINTER(Trajectory)] + gate
    lib.w2a_policy_gradient_mlp_gated.restype = C.c_int
    lib.w2a_policy_gradient_mlp_gated.argtypes = lib.w2a_policy_gradient_mlp.argtypes + gate
    lib.w2a_imitation_gradient_mlp_gated.restype = C.c_int
    lib.w2a_imitation_gradient_mlp_gated.argtypes = lib.w2a_imitation_gradient_mlp_weighted.argtypes + gate
    lib.w2a_surrogate_gradient_mlp_gated.restype = C.c_int
    lib.w2a_surrogate_gradient_mlp_gated.argtypes = lib.w2a_surrogate_gradient_mlp.argtypes + gate
    lib.w2a_hindsight_optimum_gated.restype = C.c_int
    lib.w2a_hindsight_optimum_gated.argtypes = lib.w2a_hindsight_optimum.argtypes + gate
    # Fisher-vector products: the policy, the vector, the schedule, env_weight, n_steps, obs, the outputs, [the
    # workspace,] the stream and the nullable gate
    lib.w2a_fisher_vector_product_linear.restype = C.c_int
    lib.w2a_fisher_vector_product_linear.argtypes = [vp, C.POINTER(LinearPolicy), vp, vp, vp, i32, vp, i32, vp, vp, vp,
                                                     vp, vp] + gate
    lib.w2a_fisher_vector_product_mlp_workspace_bytes.restype = C.c_size_t
    lib.w2a_fisher_vector_product_mlp_workspace_bytes.argtypes = [i64, i32, i32, i32, i32]
    lib.w2a_fisher_vector_product_mlp.restype = C.c_int
    lib.w2a_fisher_vector_product_mlp.argtypes = [vp, C.POINTER(MlpPolicy), vp, vp, i32, vp, i32, vp, vp, vp, vp, vp,
                                                  C.c_size_t, vp] + gate
    # Q-learning: the online net, the nullable target net, the schedule, env_weight, n_steps, obs, grad, loss, days,
    # ret, gamma, double_q, loss kind, huber_delta, bootstrap, td_error, td_target, the workspace and the stream
    lib.w2a_q_gradient_mlp_workspace_bytes.restype = C.c_size_t
    lib.w2a_q_gradient_mlp_workspace_bytes.argtypes = [i64, i32, i32, i32, i32]
    lib.w2a_q_gradient_mlp.restype = C.c_int
    lib.w2a_q_gradient_mlp.argtypes = [vp, C.POINTER(MlpPolicy), C.POINTER(MlpPolicy), vp, i32, vp, i32, vp, vp, vp, vp,
                                       vp, C.c_double, i32, i32, C.c_double, i32, vp, vp, vp, C.c_size_t, vp]
    # shared-trunk actor-critic: the net, the schedule, env_weight, the three epoch inputs with their day counts, clip,
    # vf_coef, entropy_coef, gamma, lambda, bootstrap, n_steps, obs, grad, the six per-env sums, ret, the three collect
    # outputs, the workspace, the stream and the nullable gate
    lib.w2a_actor_critic_mlp_workspace_bytes.restype = C.c_size_t
    lib.w2a_actor_critic_mlp_workspace_bytes.argtypes = [i64, i32, i32, i32, i32]
    lib.w2a_actor_critic_mlp.restype = C.c_int
    lib.w2a_actor_critic_mlp.argtypes = [vp, C.POINTER(MlpPolicy), vp, i32, vp, vp, i32, vp, i32, vp, i32] + \
        [C.c_double] * 5 + [i32, i32, vp, vp] + [vp] * 6 + [vp] * 4 + [vp, C.c_size_t, vp] + gate
    lib.w2a_policy_actions.restype = C.c_int
    lib.w2a_policy_actions.argtypes = [vp, C.POINTER(Policy), vp, vp, vp, vp, vp, i32, vp]
    look = [C.POINTER(Lookahead)]
    lib.w2a_lookahead_rollout_linear.restype = C.c_int
    lib.w2a_lookahead_rollout_linear.argtypes = lib.w2a_rollout_linear.argtypes + look
    lib.w2a_lookahead_rollout_linear_gated.restype = C.c_int
    lib.w2a_lookahead_rollout_linear_gated.argtypes = lib.w2a_rollout_linear.argtypes + look + [vp, i32]
    lib.w2a_lookahead_rollout_mlp.restype = C.c_int
    lib.w2a_lookahead_rollout_mlp.argtypes = lib.w2a_rollout_mlp.argtypes + look
    lib.w2a_lookahead_rollout_mlp_gated.restype = C.c_int
    lib.w2a_lookahead_rollout_mlp_gated.argtypes = lib.w2a_rollout_mlp.argtypes + look + [vp, i32]
    lib.w2a_lookahead_policy_gradient_linear.restype = C.c_int
    lib.w2a_lookahead_policy_gradient_linear.argtypes = lib.w2a_policy_gradient_linear.argtypes + look + [vp, i32]
    lib.w2a_lookahead_imitation_gradient_linear.restype = C.c_int
    lib.w2a_lookahead_imitation_gradient_linear.argtypes = lib.w2a_imitation_gradient_linear_weighted.argtypes + look + [vp, i32]
    ferr = [C.POINTER(ForecastError)]
    lib.w2a_forecast_rollout_linear.restype = C.c_int
    lib.w2a_forecast_rollout_linear.argtypes = lib.w2a_lookahead_rollout_linear_gated.argtypes + ferr
    lib.w2a_forecast_rollout_mlp.restype = C.c_int
    lib.w2a_forecast_rollout_mlp.argtypes = lib.w2a_lookahead_rollout_mlp_gated.argtypes + ferr
    lib.w2a_forecast_policy_gradient_linear.restype = C.c_int
    lib.w2a_forecast_policy_gradient_linear.argtypes = lib.w2a_lookahead_policy_gradient_linear.argtypes + ferr
    lib.w2a_forecast_imitation_gradient_linear.restype = C.c_int
    lib.w2a_forecast_imitation_gradient_linear.argtypes = lib.w2a_lookahead_imitation_gradient_linear.argtypes + ferr
    lib.w2a_forecast_features.restype = C.c_int
    lib.w2a_forecast_features.argtypes = [vp] + look + ferr + [vp, vp]
    # hindsight values along a schedule: start, n_steps, the schedule, the nullable gate, gain, expert bitmap, regret,
    # the nullable value and loss, the workspace and the stream
    lib.w2a_hindsight_along.restype = C.c_int
    lib.w2a_hindsight_along.argtypes = [vp, C.POINTER(StateView), i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp,
                                        C.c_size_t, vp]
    # the gated imitation calls with the labels after mask_words
    lib.w2a_relabel_imitation_linear.restype = C.c_int
    lib.w2a_relabel_imitation_linear.argtypes = [vp, C.POINTER(LinearPolicy), vp, i32, vp, vp, vp, i32, i32, vp, vp, vp,
                                                 vp, vp] + gate
    lib.w2a_relabel_imitation_mlp.restype = C.c_int
    lib.w2a_relabel_imitation_mlp.argtypes = [vp, C.POINTER(MlpPolicy), vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp,
                                              vp, C.c_size_t, vp] + gate
    # the hindsight budget curve: start, n_steps, max_budget, returns, alerts, the nullable schedules and their words, the
    # workspace and the stream
    lib.w2a_hindsight_curve_workspace_bytes.restype = C.c_size_t
    lib.w2a_hindsight_curve_workspace_bytes.argtypes = [vp, i32, i32, i32]
    lib.w2a_hindsight_curve.restype = C.c_int
    lib.w2a_hindsight_curve.argtypes = [vp, C.POINTER(StateView), i32, i32, vp, vp, vp, i32, vp, C.c_size_t, vp]
    lib.w2a_hindsight_curve_gated.restype = C.c_int
    lib.w2a_hindsight_curve_gated.argtypes = lib.w2a_hindsight_curve.argtypes + gate
    # the hindsight optimum of the posterior mean: w2a_hindsight_optimum's arguments; the workspace size reads no handle
    # (num_envs, T, n_samples, n_steps, max_remaining, big_envs)
    lib.w2a_hindsight_posterior_workspace_bytes.restype = C.c_size_t
    lib.w2a_hindsight_posterior_workspace_bytes.argtypes = [i64, i32, i32, i32, i32, i32]
    lib.w2a_hindsight_posterior.restype = C.c_int
    lib.w2a_hindsight_posterior.argtypes = lib.w2a_hindsight_optimum.argtypes
    lib.w2a_hindsight_posterior_gated.restype = C.c_int
    lib.w2a_hindsight_posterior_gated.argtypes = lib.w2a_hindsight_optimum.argtypes + gate
    # its values along a schedule: w2a_hindsight_along's arguments, w2a_hindsight_posterior's workspace
    lib.w2a_hindsight_posterior_along.restype = C.c_int
    lib.w2a_hindsight_posterior_along.argtypes = lib.w2a_hindsight_along.argtypes
    # the draw-blind budget curve: w2a_hindsight_curve's arguments throughout
    lib.w2a_hindsight_posterior_curve_workspace_bytes.restype = C.c_size_t
    lib.w2a_hindsight_posterior_curve_workspace_bytes.argtypes = lib.w2a_hindsight_curve_workspace_bytes.argtypes
    lib.w2a_hindsight_posterior_curve.restype = C.c_int
    lib.w2a_hindsight_posterior_curve.argtypes = lib.w2a_hindsight_curve.argtypes
    lib.w2a_hindsight_posterior_curve_gated.restype = C.c_int
    lib.w2a_hindsight_posterior_curve_gated.argtypes = lib.w2a_hindsight_curve_gated.argtypes
    # the policy budget curve: the policy, start, n_steps, max_budget, the held rows (nullable), returns, alerts,
    # attempts over budget, the nullable schedules and their words, the workspace and the stream
    lib.w2a_policy_curve_workspace_bytes.restype = C.c_size_t
    lib.w2a_policy_curve_workspace_bytes.argtypes = [vp, i32, i32]
    lib.w2a_policy_curve_linear.restype = C.c_int
    lib.w2a_policy_curve_linear.argtypes = [vp, C.POINTER(LinearPolicy), C.POINTER(StateView), i32, i32, vp, vp, vp, vp,
                                            vp, i32, vp, C.c_size_t, vp]
    lib.w2a_policy_curve_linear_gated.restype = C.c_int
    lib.w2a_policy_curve_linear_gated.argtypes = lib.w2a_policy_curve_linear.argtypes + gate
    if lib.w2a_abi_version() != ABI_VERSION:
        raise W2AError(f"libw2a.so ABI {lib.w2a_abi_version()} != {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != OK:
        msg = load().w2a_last_error().decode("utf-8", "replace")
        raise W2AError(f"{what} failed ({rc}): {msg}")
