"""Linear-logistic and MLP policies for ``HeatAlertVecEnv.rollout({"kind": "linear" | "mlp", ...})``
(csrc/w2a_rollout_linear.hip.h, csrc/w2a_rollout_mlp.hip.h). The MLP kind's host side (checks, packing into the w2a.h
layout, the group-major visiting order, ``mlp_from_module``) follows the linear kind's, below it.

The host side of w2a_rollout_linear: argument checks, the permutation of the parameters from observation order (the
columns of ``env.feature_names``) into the kernels' 32-slot feature-row order (``CompiledTables.obs_slot``), and the
per-group reduction of the returns. Nothing here launches a kernel, so all of it runs on the CPU as well.

    {"kind": "linear",
     "weight": W,             # float [G, n_obs], columns in observation order
     "bias": b,               # float [G]
     "group": g,              # int [num_envs] in [0, G); may be omitted when G == 1
     "sample": False,         # False: alert iff logit > 0; True: alert iff u < sigmoid(logit)
     "seed": 0,               # sample=True only: keys the Bernoulli policy's counter-RNG uniform u
     "require_budget": False, # never attempt an alert with no budget left
     "allowed_days": None}    # optional bool [num_envs, T] by day of the episode (HeatAlertVecEnv.alert_gate(), or any
                              # other mask): on a day whose bit is clear the attempted action is 0, before the budget test
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

ROW_FLOATS = 32
LOGIT_SLOTS = 30  # slots the day loop multiplies (0..29); an observation column elsewhere cannot be served
KEYS = {"kind", "weight", "bias", "group", "sample", "seed", "require_budget", "allowed_days", "lookahead"}
GATE_KINDS = ("linear", "mlp")  # the kinds whose kernels take "allowed_days"
LOOKAHEAD_MAX_DAYS = 10  # w2a.h: W2A_LOOKAHEAD_MAX_DAYS (the older reference env's "D10")
LOOKAHEAD_PAD = 12       # w2a.h: W2A_LOOKAHEAD_PAD, floats per lookahead weight row


@dataclass
class LinearPolicyArgs:
    """A checked linear policy, on the env's device: what w2a_linear_policy points to, plus the group ids for the
    per-group mean of the returns."""
    weight_slots: torch.Tensor   # f32 [G, 32] slot order, contiguous
    bias: torch.Tensor           # f32 [G]
    group: torch.Tensor | None   # int32 [num_envs], None = every env in group 0
    n_groups: int
    sample: bool
    seed: int
    require_budget: bool
    look_feature: str | None = None          # "lookahead": the feature's name, None without the key
    look_days: int = 0                       # D
    look_weight: torch.Tensor | None = None  # f32 [G, LOOKAHEAD_PAD], k = 1 first, zero past D
    look_error: tuple | None = None          # "error": the MAE row e_1..e_D as f32 values, None without the key
    look_error_seed: int = 0                 # "error_seed"


def check_lookahead(policy: dict, who: str, feature_names=None, obs_slot=None, n_obs: int | None = None, fixes=(),
                    slot_alerts_2wks: int = -1):
    """The ``"lookahead"`` key of a linear or mlp policy dict: None when it is absent or None, else (feature, D) from
    ``{"feature": name, "days": D}``. The decision then gets D more inputs f_k = h(r + k) - h(r), k = 1..D, after the
    observation columns: h the f32 table value of `feature` along the env's episode, r the day of the row the agent
    holds, 0 past the env's last day. ValueError for another structure, a D that is not an int in 1..10, a feature that
    is no observation column and -- the rule of alert_gate() -- one that is not table-sourced (run-time slots 24..27, and
    alerts_2wks under the "alert_2wks" fix). The name is checked when `feature_names` is given.

    Two optional keys add forecast error (the older reference env's ``forecast_error > 0``; check_forecast_error
    returns them, this function's result does not change): ``"error"``, one finite non-negative MAE for every lead or
    a sequence of exactly D of them e_1..e_D in the feature's own units, and ``"error_seed"``, an int in 0..2**63 - 1
    (default 0; ValueError without "error"). Then, for the held row's day r,
    f_k = fmaf(U(r, k), e_k, h(r + k)) - h(r) in f32, with h(r) exact, +0 past the env's last day, h(r + k) taken as it
    is where e_k == 0, and U uniform in [-1, 1) from a counter-based stream of (error_seed, global env id, episode
    number, held day, lead) alone (include/w2a.h: w2a_forecast_error). ValueError for a bool, str or None value, a
    negative, NaN or inf entry and a sequence of another length; every other key stays refused."""
    if not isinstance(policy, dict) or policy.get("lookahead") is None:
        return None
    la = policy["lookahead"]
    if not isinstance(la, dict) or not {"feature", "days"} <= set(la) <= {"feature", "days", "error", "error_seed"}:
        raise ValueError(f"{who}: 'lookahead' must be {{'feature': name, 'days': D}} with the optional keys 'error' and "
                         f"'error_seed', got {la!r}")
    feature, D = la["feature"], la["days"]
    if not isinstance(feature, str):
        raise ValueError(f"{who}: lookahead feature must be a column name, got {feature!r}")
    if isinstance(D, (bool, np.bool_)) or not isinstance(D, (int, np.integer)):
        raise ValueError(f"{who}: lookahead days must be an int in 1..{LOOKAHEAD_MAX_DAYS}, got {D!r}")
    if not 1 <= int(D) <= LOOKAHEAD_MAX_DAYS:
        raise ValueError(f"{who}: lookahead days must lie in 1..{LOOKAHEAD_MAX_DAYS}, got {D}")
    if feature_names is not None:
        if feature not in list(feature_names):
            raise ValueError(f"{who}: lookahead feature {feature!r} is no observation column")
        if obs_slot is not None and n_obs is not None:
            slot = int(slot_map(obs_slot, n_obs)[list(feature_names).index(feature)])
            if 24 <= slot <= 27 or ("alert_2wks" in set(fixes) and slot == slot_alerts_2wks):
                raise ValueError(f"{who}: lookahead feature {feature!r} is not table-sourced (lookahead reads "
                                 "table-sourced columns only)")
    _forecast_error(la, int(D), who)
    return feature, int(D)


def _forecast_error(la: dict, D: int, who: str):
    """None, or (the MAE row as D Python floats holding f32 values, the seed) of a checked-so-far lookahead dict."""
    if "error" not in la:
        if "error_seed" in la:
            raise ValueError(f"{who}: lookahead 'error_seed' needs 'error'")
        return None
    err = la["error"]
    if err is None or isinstance(err, (bool, np.bool_, str, bytes, dict)):
        raise ValueError(f"{who}: lookahead error must be a number or a sequence of D numbers, got {err!r}")
    if isinstance(err, (int, float, np.integer, np.floating)):
        row = [err] * D
    else:
        try:
            row = list(err.tolist() if hasattr(err, "tolist") else err)
        except TypeError:
            raise ValueError(f"{who}: lookahead error must be a number or a sequence of D numbers, got {err!r}") from None
        if len(row) != D:
            raise ValueError(f"{who}: lookahead error must have exactly days={D} entries, got {len(row)}")
    out = []
    for v in row:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{who}: lookahead error entries must be numbers, got {v!r}")
        with np.errstate(over="ignore"):
            try:
                f = float(np.float32(v))
            except OverflowError:
                f = float("inf")
        if not np.isfinite(f) or f < 0:  # the kernels compute on the f32 values
            raise ValueError(f"{who}: lookahead error entries must be finite and non-negative (as float32), got {v!r}")
        out.append(f)
    seed = la.get("error_seed", 0)
    if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2**63:
        raise ValueError(f"{who}: lookahead error_seed must be an int in 0..2**63 - 1, got {seed!r}")
    return tuple(out), int(seed)


def check_forecast_error(policy: dict, who: str):
    """None for a policy without ``"lookahead"`` or without its ``"error"`` key, else (e_1..e_D as f32 values, seed):
    what check_lookahead checks of the two optional keys, returned."""
    look = check_lookahead(policy, who)
    if look is None:
        return None
    return _forecast_error(policy["lookahead"], look[1], who)


def slot_map(obs_slot, n_obs: int) -> np.ndarray:
    """int64 [n_obs]: the feature-row slot of every observation column, checked to be an injective map into the slots the
    kernels' logits cover (so slots 30 and 31 are never observation columns)."""
    s = np.asarray(list(obs_slot)[:n_obs], dtype=np.int64)
    if s.shape != (n_obs,):
        raise ValueError(f"obs_slot has {s.size} entries for {n_obs} observation columns")
    if ((s < 0) | (s >= LOGIT_SLOTS)).any() or len(np.unique(s)) != n_obs:
        raise ValueError(f"obs_slot must map the observation columns one-to-one into slots 0..{LOGIT_SLOTS - 1}")
    return s


def to_slot_order(weight: torch.Tensor, obs_slot, n_obs: int) -> torch.Tensor:
    """[G, n_obs] in observation order -> f32 [G, 32] in slot order (zero where a slot is no observation column): a dot
    product with an observation row equals the same dot product with the env's 32-slot feature row."""
    s = torch.as_tensor(slot_map(obs_slot, n_obs), device=weight.device)
    out = torch.zeros((weight.shape[0], ROW_FLOATS), dtype=torch.float32, device=weight.device)
    out[:, s] = weight.to(torch.float32)
    return out


def _tensor(x, name: str, device) -> torch.Tensor:
    if x is None:
        raise ValueError(f"linear policy: {name!r} is required")
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    return t.to(device)


def check_linear_policy(policy: dict, n_obs: int, num_envs: int, obs_slot, device, feature_names=None, fixes=(),
                        slot_alerts_2wks: int = -1) -> LinearPolicyArgs:
    """Validate a {"kind": "linear", ...} policy (ValueError on anything the kernel could not run as asked) and bring its
    parameters into the kernel's form on `device`. One host reduction: the range of the group ids. With "lookahead"
    (check_lookahead; `feature_names`, `fixes` and `slot_alerts_2wks` serve its feature check) the weight is
    [G, n_obs + D]: the D lookahead columns last, k = 1 first."""
    unknown = set(policy) - KEYS
    if unknown:
        raise ValueError(f"linear policy: unknown key(s) {sorted(unknown)}; choose from {sorted(KEYS)}")
    look = check_lookahead(policy, "linear policy", feature_names, obs_slot, n_obs, fixes, slot_alerts_2wks)
    D = 0 if look is None else look[1]
    w = _tensor(policy.get("weight"), "weight", device)
    if w.is_complex() or not (w.is_floating_point() or w.dtype in (torch.int32, torch.int64)):
        raise ValueError(f"linear policy: weight must be real numbers, got {w.dtype}")
    if D and (w.dim() != 2 or w.shape[1] != n_obs + D or w.shape[0] < 1):
        raise ValueError(f"linear policy: with lookahead days={D} weight must be [G, n_obs + D = {n_obs + D}] (the "
                         f"lookahead columns last), got {tuple(w.shape)}")
    if w.dim() != 2 or w.shape[1] != n_obs + D or w.shape[0] < 1:
        raise ValueError(f"linear policy: weight must be [G, n_obs={n_obs}], got {tuple(w.shape)}")
    G = int(w.shape[0])
    w = w.to(torch.float32)
    b = _tensor(policy.get("bias"), "bias", device)
    if b.dim() > 1 or b.numel() != G or not (b.is_floating_point() or b.dtype in (torch.int32, torch.int64)):
        raise ValueError(f"linear policy: bias must be a float [G={G}], got {tuple(b.shape)} {b.dtype}")
    b = b.reshape(G).to(torch.float32).contiguous()
    # the kernels compute on the f32 values: a parameter that is not finite there is refused
    if not bool(torch.isfinite(w).all()) or not bool(torch.isfinite(b).all()):
        raise ValueError("linear policy: weight and bias must be finite (as float32)")
    g = policy.get("group")
    if g is None:
        if G != 1:
            raise ValueError(f"linear policy: 'group' [num_envs] is required with G={G} parameter rows")
    else:
        g = _tensor(g, "group", device)
        if g.dtype not in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64):
            raise ValueError(f"linear policy: group must be integer, got {g.dtype}")
        if g.dim() != 1 or g.numel() != num_envs:
            raise ValueError(f"linear policy: group must be [num_envs={num_envs}], got {tuple(g.shape)}")
        lo, hi = (int(v) for v in torch.stack([g.min(), g.max()]).to(torch.int64).tolist())
        if lo < 0 or hi >= G:
            raise ValueError(f"linear policy: group ids must lie in [0, {G}), got [{lo}, {hi}]")
        g = g.to(torch.int32).contiguous()
    sample = policy.get("sample", False)
    rb = policy.get("require_budget", False)
    if not isinstance(sample, (bool, np.bool_)) or not isinstance(rb, (bool, np.bool_)):
        raise ValueError("linear policy: 'sample' and 'require_budget' must be bools")
    seed = policy.get("seed", 0)
    if not isinstance(seed, (int, np.integer)) or isinstance(seed, bool):
        raise ValueError("linear policy: 'seed' must be an int")
    args = LinearPolicyArgs(to_slot_order(w[:, :n_obs], obs_slot, n_obs).contiguous(), b, g, G, bool(sample),
                            int(seed) & (2**64 - 1), bool(rb))
    if look is not None:
        args.look_feature, args.look_days = look
        args.look_weight = torch.nn.functional.pad(w[:, n_obs:], (0, LOOKAHEAD_PAD - D)).contiguous()
        fe = _forecast_error(policy["lookahead"], D, "linear policy")
        if fe is not None:
            args.look_error, args.look_error_seed = fe
    return args


PG_BASELINES = ("none", "no_alert")


def check_policy_gradient(policy_gradient, kind, sample, reward_mode="sampled", fixes=(), record=False,
                          kinds=("linear",)):
    """The ``policy_gradient`` keyword of ``rollout()``: None when it is off (False), else the baseline's name ("none" or
    "no_alert"; True means "no_alert"). ValueError for everything the gradient kernels do not serve: a kind outside
    `kinds` (rollout() passes ("linear", "mlp")), sample=False (a deterministic policy has no score function),
    reward_mode="posterior_mean", fixes other than "budget", record=True (take one or the other per call) and an unknown
    baseline."""
    if policy_gradient is False or policy_gradient is None:
        return None
    if policy_gradient is True:
        policy_gradient = "no_alert"
    if not isinstance(policy_gradient, str) or policy_gradient not in PG_BASELINES:
        raise ValueError(f"rollout(policy_gradient=...) must be False, True or one of {PG_BASELINES}, "
                         f"got {policy_gradient!r}")
    if kind not in kinds:
        raise ValueError(f"rollout(policy_gradient=...) needs kind {' or '.join(repr(k) for k in kinds)}, got {kind!r}")
    if not isinstance(sample, (bool, np.bool_)) or not sample:
        raise ValueError("rollout(policy_gradient=...) needs a sampled policy (sample=True): a deterministic policy "
                         "has no score function")
    if reward_mode != "sampled":
        raise ValueError("rollout(policy_gradient=...) needs reward_mode='sampled'")
    extra = set(fixes) - {"budget"}
    if extra:
        raise ValueError(f"rollout(policy_gradient=...) needs faithful observations; fixes {sorted(extra)} change what "
                         "the observation is")
    if record:
        raise ValueError("rollout(policy_gradient=...) and record=True are not combined: a recorded trajectory already "
                         "holds everything a learner needs")
    return policy_gradient


IMITATION_KINDS = ("linear", "mlp")


def check_day_bitmap(days, name: str, num_envs: int, T: int, who: str) -> torch.Tensor:
    """A bool [num_envs, T] array by day of the episode (``alert_days``, ``allowed_days``) as a torch tensor; ValueError
    for another dtype or shape."""
    ad = days if torch.is_tensor(days) else torch.as_tensor(np.asarray(days))
    if ad.dtype != torch.bool:
        raise ValueError(f"{who}: {name} must be bool, got {ad.dtype}")
    if ad.dim() != 2 or tuple(ad.shape) != (num_envs, T):
        raise ValueError(f"{who}: {name} must be bool [{num_envs}, {T}] (by day of the episode), "
                         f"got {tuple(ad.shape)}")
    return ad


def check_allowed_days(policy, num_envs: int, T: int, device, who: str):
    """The ``"allowed_days"`` key of a policy dict (or the ``allowed_days=`` of hindsight_optimum(), passed as
    ``{"kind": "linear", "allowed_days": mask}``): None when it is absent or None, else the gate packed like a
    schedule, int32 [num_envs, ceil(T / 32)] on `device`. ValueError for a kind that takes no gate (every built-in kind:
    their kernels are not gated), a dtype other than bool and a shape other than [num_envs, T]. A mask that is already
    packed -- int32 [num_envs, ceil(T / 32)], alert_gate(packed=True) -- is taken as it is: a loop over epochs then packs
    nothing per call. The shape decides before the dtype is looked at: an int32 [N, 1] array at T <= 32 is read as packed
    words, never refused as "not bool" (of no consequence at the tables' T)."""
    if not isinstance(policy, dict) or policy.get("allowed_days") is None:
        return None
    kind = policy.get("kind")
    if kind not in GATE_KINDS:
        raise ValueError(f"{who}: 'allowed_days' is taken by kind {' or '.join(repr(k) for k in GATE_KINDS)} only, "
                         f"got {kind!r}")
    words = (T + 31) // 32
    ad = policy["allowed_days"]
    if torch.is_tensor(ad) and ad.dtype == torch.int32 and tuple(ad.shape) == (num_envs, words):
        return ad.to(device).contiguous()
    ad = check_day_bitmap(ad, "allowed_days", num_envs, T, who)
    return pack_alert_days(ad.to(device), words)


def unpack_alert_days(words: torch.Tensor, T: int) -> torch.Tensor:
    """The inverse of pack_alert_days: int32 [N, W] -> bool [N, T]."""
    bits = torch.arange(32, device=words.device, dtype=torch.int32)
    return (((words.unsqueeze(-1) >> bits) & 1).reshape(words.shape[0], words.shape[1] * 32)[:, :T]).bool()


def pack_alert_days(alert_days: torch.Tensor, words: int) -> torch.Tensor:
    """bool [N, T <= 32 * words] by day of the episode -> int32 [N, words], bit (t & 31) of word t >> 5: the bitmap the
    rollout kernels write and w2a_posterior_returns / w2a_imitation_gradient_* read."""
    n = alert_days.shape[0]
    a32 = torch.nn.functional.pad(alert_days.to(torch.int32), (0, words * 32 - alert_days.shape[1])).view(n, words, 32)
    # bits of one word are distinct powers of two: their int32 sum is the word (bit 31 as -2^31, no overflow)
    shifts = torch.arange(32, dtype=torch.int32, device=alert_days.device)
    return (a32 << shifts).sum(-1, dtype=torch.int32).contiguous()


def check_schedule(days, name: str, num_envs: int, T: int, device, who: str) -> torch.Tensor:
    """A schedule by day of the episode (hindsight_values()'s ``alert_days``, imitation_gradient()'s ``labels``) as the
    packed bitmap int32 [num_envs, ceil(T / 32)] on `device`: a bool [num_envs, T] array is packed, words that are already
    packed (a torch int32 tensor of that shape) are taken as they are, as check_allowed_days does. ValueError for None,
    another dtype or another shape."""
    if days is None:
        raise ValueError(f"{who}: {name} is required")
    words = (T + 31) // 32
    if torch.is_tensor(days) and days.dtype == torch.int32 and tuple(days.shape) == (num_envs, words):
        return days.to(device).contiguous()
    return pack_alert_days(check_day_bitmap(days, name, num_envs, T, who).to(device), words)


def check_imitation_args(kind, alert_days, env_weight, n_steps, num_envs: int, T: int, device, fixes=(),
                         who: str = "imitation_gradient()"):
    """The arguments of ``imitation_gradient()`` that are not the policy itself: ValueError for a kind other than linear
    or mlp, fixes other than "budget" (they change what the observation is), an alert_days that is not bool
    [num_envs, T], an env_weight that is not a finite float [num_envs], and n_steps <= 0. Returns (packed schedule int32
    [num_envs, ceil(T / 32)], env_weight f32 [num_envs] or None, days to run) on `device`. `who` names the caller in the
    messages (value_gradient() takes the same arguments)."""
    if kind not in IMITATION_KINDS:
        raise ValueError(f"{who} needs kind {' or '.join(repr(k) for k in IMITATION_KINDS)}, got {kind!r}")
    extra = set(fixes) - {"budget"}
    if extra:
        raise ValueError(f"{who} needs faithful observations; fixes {sorted(extra)} change what the "
                         "observation is")
    if n_steps is not None:
        if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)):
            raise ValueError(f"{who}: n_steps must be an int, got {n_steps!r}")
        if n_steps <= 0:
            raise ValueError(f"{who}: n_steps must be positive")
    if alert_days is None:
        raise ValueError(f"{who}: alert_days is required")
    ad = check_day_bitmap(alert_days, "alert_days", num_envs, T, who)
    w = None
    if env_weight is not None:
        w = env_weight if torch.is_tensor(env_weight) else torch.as_tensor(np.asarray(env_weight))
        if not w.is_floating_point():
            raise ValueError(f"{who}: env_weight must be float, got {w.dtype}")
        if tuple(w.shape) != (num_envs,):
            raise ValueError(f"{who}: env_weight must be [{num_envs}], got {tuple(w.shape)}")
        w = w.detach().to(device=device, dtype=torch.float32).contiguous()
        if not bool(torch.isfinite(w).all()):
            raise ValueError(f"{who}: env_weight must be finite (as float32)")
    words = (T + 31) // 32
    return pack_alert_days(ad.to(device), words), w, (int(n_steps) if n_steps is not None else T)


def check_day_weight(day_weight, n_steps: int, num_envs: int, device, who: str = "imitation_gradient()",
                     name: str = "day_weight"):
    """``imitation_gradient(day_weight=...)``: None, or a float [S >= n_steps, num_envs] by call-day and env id (the
    layout of value_gradient()'s "advantage"), finite, returned as contiguous f32 on `device`. ValueError otherwise
    (every entry is checked, those of days an env does not step included: "advantage" holds zeros there). `who` and
    `name` name the caller and the argument in the messages (surrogate_gradient() checks its two [S, N] arrays here)."""
    if day_weight is None:
        return None
    d = day_weight if torch.is_tensor(day_weight) else torch.as_tensor(np.asarray(day_weight))
    if not d.is_floating_point():
        raise ValueError(f"{who}: {name} must be float, got {d.dtype}")
    if d.dim() != 2 or d.shape[1] != num_envs:
        raise ValueError(f"{who}: {name} must be [S, {num_envs}] (call-day, env id), got {tuple(d.shape)}")
    if d.shape[0] < n_steps:
        raise ValueError(f"{who}: {name} holds {d.shape[0]} call-days, the call runs {n_steps}")
    d = d.detach().to(device=device, dtype=torch.float32).contiguous()
    if not bool(torch.isfinite(d).all()):  # one pass over the weights and a sync, as for env_weight
        raise ValueError(f"{who}: {name} must be finite (as float32)")
    return d


def check_surrogate_args(advantage, old_log_prob, clip, entropy_coef, n_steps: int, num_envs: int, device):
    """The arguments of ``surrogate_gradient()`` beyond those of imitation_gradient(): advantage (required) and
    old_log_prob (optional), both through check_day_weight, a log-probability above zero, a clip that is negative or not
    finite and an entropy_coef that is not finite: ValueError. Returns (advantage, old_log_prob or None, clip,
    entropy_coef), the arrays contiguous f32 [S, num_envs] on `device`."""
    who = "surrogate_gradient()"
    if advantage is None:
        raise ValueError(f"{who}: advantage is required")
    adv = check_day_weight(advantage, n_steps, num_envs, device, who=who, name="advantage")
    old = check_day_weight(old_log_prob, n_steps, num_envs, device, who=who, name="old_log_prob")
    if old is not None and bool((old > 0).any()):
        raise ValueError(f"{who}: old_log_prob holds a log-probability above zero")
    for nm, v in (("clip", clip), ("entropy_coef", entropy_coef)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError(f"{who}: {nm} must be a finite number, got {v!r}")
    if clip < 0:
        raise ValueError(f"{who}: clip must not be negative, got {clip!r}")
    return adv, old, float(clip), float(entropy_coef)


def check_value_args(kind, alert_days, env_weight, n_steps, num_envs: int, T: int, device, reward_mode="sampled",
                     fixes=()):
    """The arguments of ``value_gradient()`` that are not the network itself: those of imitation_gradient(), and -- because
    rewards enter -- what rollout(policy_gradient=...) refuses: reward_mode other than "sampled"."""
    out = check_imitation_args(kind, alert_days, env_weight, n_steps, num_envs, T, device, fixes, who="value_gradient()")
    if reward_mode != "sampled":
        raise ValueError("value_gradient() needs reward_mode='sampled'")
    return out


def check_gae_args(gamma, gae_lambda, bootstrap, value_target, advantage, target, n_steps: int, num_envs: int, device):
    """The arguments of ``value_gradient()`` beyond those of check_value_args: gamma and gae_lambda finite numbers in
    [0, 1], bootstrap and value_target plain bools, target None or an [S >= n_steps, num_envs] float array
    (through check_day_weight) that is combined with none of advantage=True, value_target=True, bootstrap=True or a
    gamma / gae_lambda other than 1: ValueError otherwise. Returns (gamma, gae_lambda, target or None, new) with `new`
    true when any of them leaves its default (the call then takes the *_gae entry points)."""
    who = "value_gradient()"
    for nm, v in (("gamma", gamma), ("gae_lambda", gae_lambda)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError(f"{who}: {nm} must be a finite number in [0, 1], got {v!r}")
        if not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"{who}: {nm} must lie in [0, 1], got {v!r}")
    for nm, v in (("bootstrap", bootstrap), ("value_target", value_target)):
        if not isinstance(v, bool):
            raise ValueError(f"{who}: {nm} must be a bool, got {v!r}")
    tg = check_day_weight(target, n_steps, num_envs, device, who=who, name="target")
    gamma, gae_lambda = float(gamma), float(gae_lambda)
    if tg is not None:
        if advantage or value_target:
            raise ValueError(f"{who}: advantage and value_target are not formed when target is given")
        if gamma != 1.0 or gae_lambda != 1.0 or bootstrap:
            raise ValueError(f"{who}: gamma, gae_lambda and bootstrap have no meaning when target is given")
    new = tg is not None or gamma != 1.0 or gae_lambda != 1.0 or bootstrap or value_target
    return gamma, gae_lambda, tg, new


def group_mean(values: torch.Tensor, group: torch.Tensor | None, n_groups: int) -> torch.Tensor:
    """f32 [n_groups] (values [N]) or [n_groups, K] (values [N, K], e.g. returns under K posterior draws): the mean of
    `values` over each group's envs, per column (NaN for a group without envs), on the device of `values`: the groups'
    segments of the rows sorted by group, summed as differences of one fp64 prefix sum down the rows. (An index_add into
    n_groups fp64 cells measured 7.7 ms at 1 048 576 envs and G = 1024 -- four times the rollout it follows -- every
    env's atomic contending with a thousand others for its cell; this is a sort and a scan.)"""
    if group is None:
        if values.dim() == 1:
            return values.to(torch.float32).mean().reshape(1)
        return values.to(torch.float64).mean(0, keepdim=True).to(torch.float32)
    sg, perm = torch.sort(group.to(torch.int32))
    csum = torch.cumsum(values.to(torch.float64)[perm], dim=0)
    csum = torch.cat([torch.zeros((1,) + tuple(csum.shape[1:]), dtype=torch.float64, device=values.device), csum])
    ids = torch.arange(n_groups, dtype=torch.int32, device=values.device)
    lo = torch.searchsorted(sg, ids, right=False)
    hi = torch.searchsorted(sg, ids, right=True)
    cnt = (hi - lo).to(torch.float64).reshape((n_groups,) + (1,) * (values.dim() - 1))
    return ((csum[hi] - csum[lo]) / cnt).to(torch.float32)


def group_mean_columns(values_t: torch.Tensor, group: torch.Tensor | None, n_groups: int) -> torch.Tensor:
    """group_mean for K values per env stored column-major: values_t [K, N] -> f32 [n_groups, K]. The same sort and fp64
    prefix sum, but the scan runs along memory (one row of N per column); down the rows of an [N, K] array it measured
    410 ms at 1 048 576 envs, K = 30 and G = 1024. A fixed summation order: identical inputs give identical bits."""
    if group is None:
        return values_t.to(torch.float64).mean(1)[None, :].to(torch.float32)
    sg, perm = torch.sort(group.to(torch.int32), stable=True)
    csum = torch.cumsum(values_t.to(torch.float64)[:, perm], dim=1)
    csum = torch.cat([torch.zeros((values_t.shape[0], 1), dtype=torch.float64, device=values_t.device), csum], dim=1)
    ids = torch.arange(n_groups, dtype=torch.int32, device=values_t.device)
    lo = torch.searchsorted(sg, ids, right=False)
    hi = torch.searchsorted(sg, ids, right=True)
    return ((csum[:, hi] - csum[:, lo]) / (hi - lo).to(torch.float64)[None, :]).T.contiguous().to(torch.float32)


# ----------------------------------------------------------------------------------------------------------------------
# MLP policies: rollout({"kind": "mlp", ...}) (csrc/w2a_rollout_mlp.hip.h)
# ----------------------------------------------------------------------------------------------------------------------
#     {"kind": "mlp",
#      "layers": [(W1, b1), (W2, b2), (Wo, bo)],  # torch Linear convention: W [out, in] or [G, out, in], b [out] / [G, out]
#      "activation": "tanh",   # or "relu": after every hidden layer, none after the output
#      "group": g,             # int [num_envs] in [0, G); may be omitted when G == 1
#      "order": None,          # optional int [num_envs] visiting permutation (default: the envs stably sorted by group)
#      "sample": False, "seed": 0, "require_budget": False}   # as for kind="linear"
# One or two hidden layers of width 1..64; the first takes the n_obs observation columns in observation order; the
# output has one row (the logit) or two (SB3's two action values: logit = row1 - row0, folded here in fp64).

MLP_KEYS = {"kind", "layers", "activation", "group", "order", "sample", "seed", "require_budget", "allowed_days",
            "lookahead"}
MLP_WIDTHS = (16, 32, 64)  # the kernel's padded hidden widths
MLP_MAX_HIDDEN = 2
MLP_ACTIVATIONS = ("tanh", "relu")


def mlp_stride(width: int, n_layers: int) -> int:
    """Floats per group block of the packed parameters (w2a.h: W2A_MLP_STRIDE)."""
    return ROW_FLOATS * width + width + (width * width + width if n_layers == 2 else 0) + width + 4


def mlp_lookahead_stride(width: int, n_layers: int) -> int:
    """Floats per group block of a lookahead policy (w2a.h: W2A_MLP_LOOKAHEAD_STRIDE): the block of mlp_stride with
    W1f[LOOKAHEAD_PAD][width], the first layer's rows of the lookahead inputs, appended."""
    return mlp_stride(width, n_layers) + LOOKAHEAD_PAD * width


def mlp_width(hidden) -> int:
    """The padded width the kernel runs for these hidden widths."""
    m = max(hidden)
    return next(w for w in MLP_WIDTHS if w >= m)


@dataclass
class MlpPolicyArgs:
    """A checked MLP policy, on the env's device: what w2a_mlp_policy points to, plus the group ids for the per-group
    mean of the returns."""
    params: torch.Tensor         # f32 [G, mlp_stride(width, n_layers)], contiguous (the w2a.h layout)
    group: torch.Tensor | None   # int32 [num_envs], None = every env in group 0
    order: torch.Tensor | None   # int32 [num_envs] visiting permutation, None = the env's own order
    n_groups: int
    n_layers: int                # hidden layers
    width: int                   # padded hidden width: 16, 32 or 64
    activation: str
    sample: bool
    seed: int
    require_budget: bool
    hidden: tuple = ()           # the real (unpadded) hidden widths
    n_out: int = 1               # rows of the output layer as given (2: folded into row1 - row0)
    group_major: bool = False    # `order` is group_order(group), built here (no "order" key in the policy)
    look_feature: str | None = None  # "lookahead": the feature's name, None without the key
    look_days: int = 0               # D: params then has mlp_lookahead_stride floats per block
    look_error: tuple | None = None  # "error": the MAE row e_1..e_D as f32 values, None without the key
    look_error_seed: int = 0         # "error_seed"


def _real(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.is_complex() or not (t.is_floating_point() or t.dtype in (torch.int32, torch.int64)):
        raise ValueError(f"mlp policy: {what} must be real numbers, got {t.dtype}")
    return t.to(torch.float64)


def _mlp_layers(layers, n_obs: int, look_days: int = 0):
    """The layers as fp64 [G or 1, out, in] / [G or 1, out] tensors, checked, and G. look_days = D > 0: the first layer
    takes n_obs + D inputs, the D lookahead columns last."""
    if not isinstance(layers, (list, tuple)) or not 2 <= len(layers) <= MLP_MAX_HIDDEN + 1:
        raise ValueError(f"mlp policy: 'layers' must be a list of 2..{MLP_MAX_HIDDEN + 1} (weight, bias) pairs "
                         f"(1..{MLP_MAX_HIDDEN} hidden layers and the output layer)")
    out, G, fan_in = [], None, n_obs + look_days
    for i, layer in enumerate(layers):
        if not isinstance(layer, (list, tuple)) or len(layer) != 2:
            raise ValueError(f"mlp policy: layer {i} must be a (weight, bias) pair")
        W, b = (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x)) for x in layer)
        W, b = _real(W.detach().cpu(), f"layer {i} weight"), _real(b.detach().cpu(), f"layer {i} bias")
        if W.dim() == 2:
            W = W.unsqueeze(0)
        if W.dim() != 3 or W.shape[2] != fan_in or W.shape[1] < 1 or W.shape[0] < 1:
            raise ValueError(f"mlp policy: layer {i} weight must be [out, {fan_in}] or [G, out, {fan_in}], "
                             f"got {tuple(layer[0].shape) if hasattr(layer[0], 'shape') else '?'}")
        rows = int(W.shape[1])
        if b.dim() == 1:
            b = b.unsqueeze(0)
        if b.dim() != 2 or b.shape[1] != rows or b.shape[0] not in (1, W.shape[0]):
            raise ValueError(f"mlp policy: layer {i} bias must be [{rows}] or [G, {rows}], got {tuple(b.shape)}")
        for n_g in (W.shape[0], b.shape[0]):
            if n_g != 1:
                if G is not None and n_g != G:
                    raise ValueError(f"mlp policy: layers disagree on the number of groups ({G} vs {n_g})")
                G = int(n_g)
        last = i == len(layers) - 1
        if last and rows not in (1, 2):
            raise ValueError(f"mlp policy: the output layer must have 1 or 2 rows, got {rows}")
        if not last and rows > MLP_WIDTHS[-1]:
            raise ValueError(f"mlp policy: hidden layer {i} is {rows} wide; at most {MLP_WIDTHS[-1]}")
        out.append((W, b))
        fan_in = rows
    # the kernels compute on the f32 values: a parameter that is not finite there is refused
    if not all(bool(torch.isfinite(x.to(torch.float32)).all()) for wb in out for x in wb):
        raise ValueError("mlp policy: weights and biases must be finite (as float32)")
    return out, (G or 1)


def pack_mlp(layers, obs_slot, n_obs: int, look_days: int = 0):
    """Pack checked or raw layers into the kernel's layout (w2a.h: w2a_mlp_policy): f32 [G, stride] on the CPU, with
    (width, n_layers, G). A two-row output is folded into logit = row1 - row0 in fp64 before rounding to f32.
    look_days = D > 0 (policy["lookahead"]): the first layer's weight is [out, n_obs + D]; its last D columns go, k = 1
    first, into W1f[LOOKAHEAD_PAD][width] at the block's tail (mlp_lookahead_stride; nothing before the tail moves)."""
    L, G = _mlp_layers(layers, n_obs, look_days)
    hidden = [int(W.shape[1]) for W, _ in L[:-1]]
    nl, w = len(hidden), mlp_width(hidden)
    s = torch.as_tensor(slot_map(obs_slot, n_obs))
    P = torch.zeros((G, mlp_lookahead_stride(w, nl) if look_days else mlp_stride(w, nl)), dtype=torch.float64)
    off = 0

    def put(dst_shape, src):
        nonlocal off
        n = int(np.prod(dst_shape))
        P[:, off:off + n].view(G, *dst_shape).copy_(src)
        off += n

    W1, b1 = (x.expand(G, *x.shape[1:]) for x in L[0])
    W1s = torch.zeros((G, ROW_FLOATS, w), dtype=torch.float64)
    W1s[:, s, :hidden[0]] = W1[:, :, :n_obs].transpose(1, 2)
    put((ROW_FLOATS, w), W1s)
    put((w,), torch.nn.functional.pad(b1, (0, w - hidden[0])))
    if nl == 2:
        W2, b2 = (x.expand(G, *x.shape[1:]) for x in L[1])
        W2p = torch.zeros((G, w, w), dtype=torch.float64)
        W2p[:, :hidden[0], :hidden[1]] = W2.transpose(1, 2)  # [input unit][output unit]
        put((w, w), W2p)
        put((w,), torch.nn.functional.pad(b2, (0, w - hidden[1])))
    Wo, bo = (x.expand(G, *x.shape[1:]) for x in L[-1])
    if Wo.shape[1] == 2:  # SB3's two action values: argmax / softmax over {0, 1} is the sign / sigmoid of row1 - row0
        Wo, bo = Wo[:, 1:] - Wo[:, :1], bo[:, 1:] - bo[:, :1]
    put((w,), torch.nn.functional.pad(Wo[:, 0], (0, w - hidden[-1])))
    P[:, off] = bo[:, 0]
    if look_days:
        tail = mlp_stride(w, nl)
        P[:, tail:].view(G, LOOKAHEAD_PAD, w)[:, :look_days, :hidden[0]] = W1[:, :, n_obs:].transpose(1, 2)
    P = P.to(torch.float32)
    if not bool(torch.isfinite(P).all()):
        raise ValueError("mlp policy: the folded output row (row1 - row0) is not finite as float32")
    return P, w, nl, G


def unpack_mlp_grad(P, obs_slot, n_obs: int, hidden, n_out: int = 1, look_days: int = 0):
    """A gradient in the kernel's block layout (f32 or f64 [G, mlp_stride(width, n_layers)], as w2a_policy_gradient_mlp
    writes it) -> layers [(dW [G, out, in], db [G, out]), ...] in torch's Linear convention with the real widths
    `hidden` and `n_out` output rows: the adjoint of pack_mlp's placement, <pack(L), P> = <L, unpack(P)>. Padding units
    and non-observation slots are dropped; a two-row output gets +g on row 1 and -g on row 0 (the adjoint of the fold
    logit = row1 - row0). look_days = D > 0: P has mlp_lookahead_stride floats per block and the first layer's dW is
    [G, out, n_obs + D], the lookahead columns (from the tail W1f) last."""
    hidden = [int(h) for h in hidden]
    nl, w = len(hidden), mlp_width(hidden)
    want = mlp_lookahead_stride(w, nl) if look_days else mlp_stride(w, nl)
    if P.dim() != 2 or P.shape[1] != want:
        raise ValueError(f"unpack_mlp_grad: expected [G, {want}] for hidden widths {hidden}, got {tuple(P.shape)}")
    if n_out not in (1, 2):
        raise ValueError(f"unpack_mlp_grad: n_out must be 1 or 2, got {n_out}")
    G = int(P.shape[0])
    s = torch.as_tensor(slot_map(obs_slot, n_obs), device=P.device)
    off = 0

    def take(shape):
        nonlocal off
        n = int(np.prod(shape))
        v = P[:, off:off + n].reshape(G, *shape)
        off += n
        return v

    W1s = take((ROW_FLOATS, w))
    dW1 = W1s[:, s, :hidden[0]].transpose(1, 2)
    if look_days:
        W1f = P[:, mlp_stride(w, nl):].reshape(G, LOOKAHEAD_PAD, w)
        dW1 = torch.cat([dW1, W1f[:, :look_days, :hidden[0]].transpose(1, 2)], dim=2)
    layers = [(dW1.contiguous(), take((w,))[:, :hidden[0]].contiguous())]
    if nl == 2:
        W2p = take((w, w))
        layers.append((W2p[:, :hidden[0], :hidden[1]].transpose(1, 2).contiguous(), take((w,))[:, :hidden[1]].contiguous()))
    go, gb = take((w,))[:, None, :hidden[-1]], P[:, off:off + 1]
    if n_out == 2:
        go, gb = torch.cat([-go, go], dim=1), torch.cat([-gb, gb], dim=1)
    layers.append((go.contiguous(), gb.contiguous()))
    return layers


# ----------------------------------------------------------------------------------------------------------------------
# Two-head Q-nets: q_gradient() (csrc/w2a_qlearn.hip.h). The output layer keeps its two rows, Q(o, 0) and Q(o, 1).
# ----------------------------------------------------------------------------------------------------------------------
def mlp_heads_stride(width: int, n_layers: int) -> int:
    """Floats per group block of the two-head layout (w2a.h: W2A_MLP_HEADS_STRIDE): the block of mlp_stride with the tail
    wo[w], bo, 3 pad replaced by wo0[w], wo1[w], bo0, bo1, 2 pad."""
    return mlp_stride(width, n_layers) + width


def pack_mlp_heads(layers, obs_slot, n_obs: int):
    """Pack layers whose output layer has exactly two rows into the two-head layout: f32 [G, mlp_heads_stride] on the
    CPU, with (width, n_layers, G). Nothing is folded: row a of the output layer is Q(o, a). Up to and including the
    first output row the block is pack_mlp's of the one-output net made of the same hidden layers and row 0."""
    L, G = _mlp_layers(layers, n_obs)
    Wo, bo = L[-1]
    if Wo.shape[1] != 2:
        raise ValueError(f"mlp q-net: the output layer must have exactly 2 rows (one action value each), got {Wo.shape[1]}")
    P0, w, nl, _ = pack_mlp(L[:-1] + [(Wo[:, :1], bo[:, :1])], obs_slot, n_obs)
    P1 = pack_mlp(L[:-1] + [(Wo[:, 1:], bo[:, 1:])], obs_slot, n_obs)[0]
    st = mlp_stride(w, nl)
    P = torch.zeros((G, st + w), dtype=torch.float32)
    P[:, :st - 4] = P0[:, :st - 4]
    P[:, st - 4:st - 4 + w] = P1[:, st - 4 - w:st - 4]
    P[:, st - 4 + w] = P0[:, st - 4]
    P[:, st - 3 + w] = P1[:, st - 4]
    return P, w, nl, G


def unpack_mlp_heads_grad(P, obs_slot, n_obs: int, hidden):
    """A gradient in the two-head block layout (f32 or f64 [G, mlp_heads_stride(width, n_layers)], as w2a_q_gradient_mlp
    writes it) -> layers [(dW [G, out, in], db [G, out]), ...] in torch's Linear convention with the real widths
    `hidden` and a two-row output layer: the adjoint of pack_mlp_heads' placement, <pack(L), P> = <L, unpack(P)>."""
    hidden = [int(h) for h in hidden]
    nl, w = len(hidden), mlp_width(hidden)
    st = mlp_stride(w, nl)
    if P.dim() != 2 or P.shape[1] != st + w:
        raise ValueError(f"unpack_mlp_heads_grad: expected [G, {st + w}] for hidden widths {hidden}, got {tuple(P.shape)}")
    pad = torch.zeros((P.shape[0], 3), dtype=P.dtype, device=P.device)
    row0 = torch.cat([P[:, :st - 4], P[:, st - 4 + w:st - 3 + w], pad], dim=1)
    row1 = torch.cat([P[:, :st - 4 - w], P[:, st - 4:st - 4 + w], P[:, st - 3 + w:st - 2 + w], pad], dim=1)
    L0 = unpack_mlp_grad(row0, obs_slot, n_obs, hidden, 1)
    L1 = unpack_mlp_grad(row1, obs_slot, n_obs, hidden, 1)
    return L0[:-1] + [(torch.cat([L0[-1][0], L1[-1][0]], dim=1).contiguous(),
                       torch.cat([L0[-1][1], L1[-1][1]], dim=1).contiguous())]


def mlp_heads_grad_to_module(module: torch.nn.Module, grad: dict, group: int = 0, ascent: bool = True) -> None:
    """Write ``q_gradient()["q_gradient"]`` of group `group` into the ``.grad`` of the Linears of an SB3-shaped q_net
    (``model.q_net.q_net``: Linear, act, [Linear, act,] Linear with two output units), as mlp_grad_to_module does for a
    policy: ascent=True writes the NEGATED gradient, so that a torch optimizer's ``step()`` descends the TD loss."""
    out = grad["layers"][-1][0]
    if out.shape[-2] != 2:
        raise ValueError(f"mlp_heads_grad_to_module: the gradient's output layer has {out.shape[-2]} rows, not 2")
    mlp_grad_to_module(module, grad, group, ascent)


Q_LOSSES = ("huber", "squared")


def check_q_net(q, target_net, n_obs: int, num_envs: int, obs_slot, device, who: str = "q_gradient()"):
    """The two nets of ``q_gradient()``: `q` a kind="mlp" dict as rollout() takes it whose output layer has exactly two
    rows, `target_net` None or a second one with the same hidden widths, activation and number of groups (its "group",
    "order" and "require_budget" are not read: the online net's hold). ValueError for a one-row output, for
    "allowed_days" and "sample" (gates and sampling have no meaning here) and for an "order" that is not group-major.
    Returns (MlpPolicyArgs of q with `params` in the two-head layout, the target's f32 [G, stride] blocks or None)."""
    if not isinstance(q, dict) or q.get("kind") != "mlp":
        raise ValueError(f"{who} needs kind 'mlp', got {q.get('kind') if isinstance(q, dict) else type(q).__name__!r}")
    if q.get("allowed_days") is not None:
        raise ValueError(f"{who}: 'allowed_days' is not taken (gates are out of scope for Q-learning here)")
    if q.get("sample"):
        raise ValueError(f"{who}: 'sample' is not taken (the schedule holds the actions; collect with rollout())")
    pol = check_mlp_policy(q, n_obs, num_envs, obs_slot, device)
    if pol.n_out != 2:
        raise ValueError(f"{who}: the output layer must have exactly 2 rows (one action value each), got {pol.n_out}")
    if q.get("order") is not None and pol.group is not None and not torch.equal(pol.order, group_order(pol.group)):
        raise ValueError(f"{who}: 'order' must be group-major (leave it out: the envs are visited sorted by group)")
    pol.params = pack_mlp_heads(q["layers"], obs_slot, n_obs)[0].to(device).contiguous()
    tparams = None
    if target_net is not None:
        if not isinstance(target_net, dict) or target_net.get("kind") != "mlp":
            raise ValueError(f"{who}: target_net must be None or a kind='mlp' dict")
        unknown = set(target_net) - MLP_KEYS
        if unknown:
            raise ValueError(f"{who}: target_net: unknown key(s) {sorted(unknown)}")
        if "layers" not in target_net:
            raise ValueError(f"{who}: target_net: 'layers' is required")
        if target_net.get("activation", "tanh") != pol.activation:
            raise ValueError(f"{who}: target_net's activation differs from the online net's ({pol.activation!r})")
        tl, tG = _mlp_layers(target_net["layers"], n_obs)
        t_hidden = tuple(int(W.shape[1]) for W, _ in tl[:-1])
        if t_hidden != tuple(pol.hidden) or tG != pol.n_groups:
            raise ValueError(f"{who}: target_net must have the online net's hidden widths {tuple(pol.hidden)} and "
                             f"{pol.n_groups} group(s), got {t_hidden} and {tG}")
        tparams = pack_mlp_heads(target_net["layers"], obs_slot, n_obs)[0].to(device).contiguous()
    return pol, tparams


def check_q_args(gamma, double, loss, huber_delta, bootstrap, td_error, td_target, who: str = "q_gradient()"):
    """The scalars of ``q_gradient()``: gamma a finite number in [0, 1], loss "huber" or "squared", huber_delta finite and
    positive, double / bootstrap / td_error / td_target plain bools: ValueError otherwise. Returns (gamma, huber_delta)."""
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float, np.integer, np.floating)) or not np.isfinite(gamma) \
            or not 0.0 <= float(gamma) <= 1.0:
        raise ValueError(f"{who}: gamma must be a finite number in [0, 1], got {gamma!r}")
    if loss not in Q_LOSSES:
        raise ValueError(f"{who}: loss must be one of {Q_LOSSES}, got {loss!r}")
    if isinstance(huber_delta, bool) or not isinstance(huber_delta, (int, float, np.integer, np.floating)) \
            or not np.isfinite(huber_delta) or not huber_delta > 0:
        raise ValueError(f"{who}: huber_delta must be a finite positive number, got {huber_delta!r}")
    for nm, v in (("double", double), ("bootstrap", bootstrap), ("td_error", td_error), ("td_target", td_target)):
        if not isinstance(v, bool):
            raise ValueError(f"{who}: {nm} must be a bool, got {v!r}")
    return float(gamma), float(huber_delta)


# ----------------------------------------------------------------------------------------------------------------------
# Shared-trunk actor-critic: actor_critic_gradient() (csrc/w2a_actor_critic.hip.h). Row 0 of the output layer is the
# policy logit, row 1 the state value; the block is the two-head layout above.
# ----------------------------------------------------------------------------------------------------------------------
def check_actor_critic_net(net, n_obs: int, num_envs: int, obs_slot, device, who: str = "actor_critic_gradient()"):
    """The network of ``actor_critic_gradient()``: a kind="mlp" dict as surrogate_gradient() takes it (hidden shapes,
    activation, "group", "require_budget", "allowed_days") whose output layer has exactly two rows -- ValueError for a
    linear kind and for another number of output rows. Returns MlpPolicyArgs with `params` in the two-head layout
    (pack_mlp_heads) and `order` group-major whatever "order" says (the gradient kernels' partial blocks are sized for
    it, as in surrogate_gradient())."""
    kind = net.get("kind") if isinstance(net, dict) else None
    if kind != "mlp":
        raise ValueError(f"{who} needs kind 'mlp' (one trunk with a policy row and a value row), got {kind!r}")
    pol = check_mlp_policy(net, n_obs, num_envs, obs_slot, device)
    if pol.n_out != 2:
        raise ValueError(f"{who}: the output layer must have exactly 2 rows (row 0 the policy logit, row 1 the state "
                         f"value), got {pol.n_out}")
    pol.params = pack_mlp_heads(net["layers"], obs_slot, n_obs)[0].to(device).contiguous()
    if pol.group is not None and not pol.group_major:
        pol.order, pol.group_major = group_order(pol.group), True
    return pol


def check_actor_critic_args(advantage, value_target, old_log_prob, clip, vf_coef, entropy_coef, gamma, gae_lambda,
                            bootstrap, gradient, n_steps: int, num_envs: int, device,
                            who: str = "actor_critic_gradient()"):
    """The arguments of ``actor_critic_gradient()`` beyond the net and the schedule, with the checks of
    check_surrogate_args and check_gae_args: advantage, value_target and old_log_prob all None (collect) or all given
    (epoch; each through check_day_weight, a log-probability above zero refused); clip and vf_coef finite and not
    negative, entropy_coef finite; gamma and gae_lambda finite in [0, 1]; bootstrap and gradient plain bools. In an epoch
    gamma, gae_lambda and bootstrap must stay at their defaults (they have no meaning there, as value_gradient(target=))
    and gradient must be True. ValueError otherwise. Returns (advantage, value_target, old_log_prob -- contiguous f32
    [S, num_envs] on `device` or None --, clip, vf_coef, entropy_coef, gamma, gae_lambda)."""
    given = [x is not None for x in (advantage, value_target, old_log_prob)]
    if any(given) and not all(given):
        raise ValueError(f"{who}: advantage, value_target and old_log_prob come together (an epoch on a collect call's "
                         "outputs) or not at all (collect)")
    for nm, v in (("clip", clip), ("vf_coef", vf_coef), ("entropy_coef", entropy_coef)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError(f"{who}: {nm} must be a finite number, got {v!r}")
    if clip < 0:
        raise ValueError(f"{who}: clip must not be negative, got {clip!r}")
    if vf_coef < 0:
        raise ValueError(f"{who}: vf_coef must not be negative, got {vf_coef!r}")
    for nm, v in (("gamma", gamma), ("gae_lambda", gae_lambda)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError(f"{who}: {nm} must be a finite number in [0, 1], got {v!r}")
        if not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"{who}: {nm} must lie in [0, 1], got {v!r}")
    for nm, v in (("bootstrap", bootstrap), ("gradient", gradient)):
        if not isinstance(v, bool):
            raise ValueError(f"{who}: {nm} must be a bool, got {v!r}")
    adv = vt = old = None
    if all(given):
        if float(gamma) != 1.0 or float(gae_lambda) != 1.0 or bootstrap:
            raise ValueError(f"{who}: gamma, gae_lambda and bootstrap have no meaning in an epoch (the advantages and "
                             "targets are given)")
        if not gradient:
            raise ValueError(f"{who}: gradient=False is a collect call's option (an epoch forms nothing else)")
        adv = check_day_weight(advantage, n_steps, num_envs, device, who=who, name="advantage")
        vt = check_day_weight(value_target, n_steps, num_envs, device, who=who, name="value_target")
        old = check_day_weight(old_log_prob, n_steps, num_envs, device, who=who, name="old_log_prob")
        if bool((old > 0).any()):
            raise ValueError(f"{who}: old_log_prob holds a log-probability above zero")
    return adv, vt, old, float(clip), float(vf_coef), float(entropy_coef), float(gamma), float(gae_lambda)


def check_fisher_args(kind, vector, pol, n_obs: int, obs_slot, device):
    """The ``vector`` of ``fisher_vector_product()``, which has the shape of the "policy_gradient" the gradient calls
    return for the checked policy `pol` (LinearPolicyArgs or MlpPolicyArgs): linear {"weight": [G, n_obs], "bias": [G]},
    mlp {"layers": [(V, vb), ...]} in the policy's own shapes (a leading G where the policy has G > 1 blocks; a two-row
    output as two rows). ValueError for another structure, a shape that differs in any layer, another G, and an entry
    that is not finite (as float32). Returns the vector in the kernel's form on `device`, packed by what the policy
    itself goes through -- linear: (f32 [G, 32] in slot order, f32 [G]); mlp: f32 [G, stride] -- both linear maps, so the
    two-row fold and the padding come out right and the padding stays zero."""
    who = "fisher_vector_product()"
    if not isinstance(vector, dict):
        raise ValueError(f"{who}: vector must be a dict in the shape of \"policy_gradient\", got {type(vector).__name__}")
    G = pol.n_groups
    if kind == "linear":
        if set(vector) != {"weight", "bias"}:
            raise ValueError(f"{who}: a linear policy's vector is {{'weight': [G, n_obs], 'bias': [G]}}, "
                             f"got keys {sorted(vector)}")
        vw, vb = (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x)) for x in (vector["weight"], vector["bias"]))
        if not vw.is_floating_point() or not vb.is_floating_point():
            raise ValueError(f"{who}: vector must be float, got {vw.dtype} and {vb.dtype}")
        if tuple(vw.shape) != (G, n_obs):
            raise ValueError(f"{who}: vector['weight'] must be [G={G}, n_obs={n_obs}], got {tuple(vw.shape)}")
        if vb.numel() != G or vb.dim() > 1:
            raise ValueError(f"{who}: vector['bias'] must be [G={G}], got {tuple(vb.shape)}")
        vw = vw.detach().to(device=device, dtype=torch.float32)
        vb = vb.detach().reshape(G).to(device=device, dtype=torch.float32).contiguous()
        if not bool(torch.isfinite(vw).all()) or not bool(torch.isfinite(vb).all()):
            raise ValueError(f"{who}: vector must be finite (as float32)")
        return to_slot_order(vw, obs_slot, n_obs).contiguous(), vb
    if set(vector) != {"layers"}:
        raise ValueError(f"{who}: an mlp policy's vector is {{'layers': [(V, vb), ...]}}, got keys {sorted(vector)}")
    layers = vector["layers"]
    if not isinstance(layers, (list, tuple)) or len(layers) != pol.n_layers + 1:
        raise ValueError(f"{who}: vector['layers'] must hold {pol.n_layers + 1} (V, vb) pairs, as the policy's layers")
    fan_in, out_rows = [n_obs] + list(pol.hidden), list(pol.hidden) + [pol.n_out]
    full = []
    for i, layer in enumerate(layers):
        if not isinstance(layer, (list, tuple)) or len(layer) != 2:
            raise ValueError(f"{who}: vector layer {i} must be a (V, vb) pair")
        V, vb = (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x)) for x in layer)
        if not V.is_floating_point() or not vb.is_floating_point():
            raise ValueError(f"{who}: vector layer {i} must be float, got {V.dtype} and {vb.dtype}")
        V, vb = V.detach().cpu(), vb.detach().cpu()
        if G == 1 and V.dim() == 2:
            V = V.unsqueeze(0)
        if G == 1 and vb.dim() == 1:
            vb = vb.unsqueeze(0)
        if tuple(V.shape) != (G, out_rows[i], fan_in[i]) or tuple(vb.shape) != (G, out_rows[i]):
            raise ValueError(f"{who}: vector layer {i} must be [G={G}, {out_rows[i]}, {fan_in[i]}] and "
                             f"[G={G}, {out_rows[i]}], the policy's own shapes, got {tuple(np.shape(layer[0]))} and "
                             f"{tuple(np.shape(layer[1]))}")
        if not bool(torch.isfinite(V.to(torch.float32)).all()) or not bool(torch.isfinite(vb.to(torch.float32)).all()):
            raise ValueError(f"{who}: vector must be finite (as float32)")
        full.append((V, vb))
    try:
        P, width, nl, G_v = pack_mlp(full, obs_slot, n_obs)
    except ValueError as e:  # the folded output row overflowing f32
        raise ValueError(f"{who}: {e}") from None
    assert (width, nl, G_v) == (pol.width, pol.n_layers, G)
    return P.to(device).contiguous()


def mlp_grad_to_module(module: torch.nn.Module, grad: dict, group: int = 0, ascent: bool = True) -> None:
    """Write ``rollout(mlp, policy_gradient=...)["policy_gradient"]`` of group `group` into the ``.grad`` of the Linears
    of the Sequential mlp_from_module accepts (in order). ascent=True writes the NEGATED gradient, so that a torch
    optimizer's ``step()`` (which descends) ascends the return; ascent=False writes it as it is."""
    def flat(m):
        if isinstance(m, torch.nn.Sequential):
            for c in m:
                yield from flat(c)
        else:
            yield m

    lins = [m for m in flat(module) if isinstance(m, torch.nn.Linear)]
    layers = grad["layers"]
    if len(lins) != len(layers):
        raise ValueError(f"mlp_grad_to_module: the module has {len(lins)} Linear layers, the gradient {len(layers)}")
    sign = -1.0 if ascent else 1.0
    for m, (dW, db) in zip(lins, layers):
        dW, db = dW[group], db[group]
        if tuple(dW.shape) != tuple(m.weight.shape):
            raise ValueError(f"mlp_grad_to_module: gradient {tuple(dW.shape)} for a weight {tuple(m.weight.shape)}")
        m.weight.grad = (sign * dW).to(device=m.weight.device, dtype=m.weight.dtype)
        if m.bias is not None:
            m.bias.grad = (sign * db).to(device=m.bias.device, dtype=m.bias.dtype)


def group_order(group: torch.Tensor) -> torch.Tensor:
    """int32 [num_envs]: the env ids stably sorted by group, so each group's envs fill whole waves."""
    return torch.sort(group, stable=True).indices.to(torch.int32).contiguous()


def check_mlp_policy(policy: dict, n_obs: int, num_envs: int, obs_slot, device, feature_names=None, fixes=(),
                     slot_alerts_2wks: int = -1) -> MlpPolicyArgs:
    """Validate a {"kind": "mlp", ...} policy (ValueError on anything the kernel could not run as asked) and bring its
    parameters into the kernel's layout on `device`. With "lookahead" (check_lookahead; `feature_names`, `fixes` and
    `slot_alerts_2wks` serve its feature check) the first layer takes n_obs + D inputs."""
    unknown = set(policy) - MLP_KEYS
    if unknown:
        raise ValueError(f"mlp policy: unknown key(s) {sorted(unknown)}; choose from {sorted(MLP_KEYS)}")
    look = check_lookahead(policy, "mlp policy", feature_names, obs_slot, n_obs, fixes, slot_alerts_2wks)
    D = 0 if look is None else look[1]
    act = policy.get("activation", "tanh")
    if act not in MLP_ACTIVATIONS:
        raise ValueError(f"mlp policy: activation must be one of {MLP_ACTIVATIONS}, got {act!r}")
    if "layers" not in policy:
        raise ValueError("mlp policy: 'layers' is required")
    P, width, nl, G = pack_mlp(policy["layers"], obs_slot, n_obs, D)
    g = policy.get("group")
    if g is None:
        if G != 1:
            raise ValueError(f"mlp policy: 'group' [num_envs] is required with G={G} parameter blocks")
    else:
        g = _tensor(g, "group", device)
        if g.dtype not in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64):
            raise ValueError(f"mlp policy: group must be integer, got {g.dtype}")
        if g.dim() != 1 or g.numel() != num_envs:
            raise ValueError(f"mlp policy: group must be [num_envs={num_envs}], got {tuple(g.shape)}")
        lo, hi = (int(v) for v in torch.stack([g.min(), g.max()]).to(torch.int64).tolist())
        if lo < 0 or hi >= G:
            raise ValueError(f"mlp policy: group ids must lie in [0, {G}), got [{lo}, {hi}]")
        g = g.to(torch.int32).contiguous()
    order = policy.get("order")
    if order is not None:
        order = _tensor(order, "order", device)
        if order.dtype not in (torch.int16, torch.int32, torch.int64) or order.dim() != 1 or order.numel() != num_envs:
            raise ValueError(f"mlp policy: order must be an integer [num_envs={num_envs}] permutation")
        if not torch.equal(torch.sort(order.to(torch.int64)).values,
                           torch.arange(num_envs, dtype=torch.int64, device=order.device)):
            raise ValueError("mlp policy: order must be a permutation of the env ids")
        order = order.to(torch.int32).contiguous()
    elif g is not None:
        order = group_order(g)
    group_major = policy.get("order") is None and g is not None
    sample = policy.get("sample", False)
    rb = policy.get("require_budget", False)
    if not isinstance(sample, (bool, np.bool_)) or not isinstance(rb, (bool, np.bool_)):
        raise ValueError("mlp policy: 'sample' and 'require_budget' must be bools")
    seed = policy.get("seed", 0)
    if not isinstance(seed, (int, np.integer)) or isinstance(seed, bool):
        raise ValueError("mlp policy: 'seed' must be an int")
    shapes = [tuple(np.shape(W)) for W, _ in policy["layers"]]
    fe = None if look is None else _forecast_error(policy["lookahead"], D, "mlp policy")
    return MlpPolicyArgs(P.to(device).contiguous(), g, order, G, nl, width, act, bool(sample), int(seed) & (2**64 - 1),
                         bool(rb), tuple(int(sh[-2]) for sh in shapes[:-1]), int(shapes[-1][-2]), group_major,
                         None if look is None else look[0], D, None if fe is None else fe[0],
                         0 if fe is None else fe[1])


def mlp_from_module(module: torch.nn.Module, group=None) -> dict:
    """A {"kind": "mlp", ...} policy from a torch.nn.Sequential of Linear / Tanh / ReLU: Linear, act, [Linear, act,]
    Linear, with one activation type and an output of 1 or 2 units. Nested Sequentials are flattened, so an SB3 actor is
    ``mlp_from_module(nn.Sequential(*model.policy.mlp_extractor.policy_net, model.policy.action_net))`` and a DQN
    Q-net ``mlp_from_module(model.q_net.q_net)``. The parameters are copied (detached) as they are now."""
    def flat(m):
        if isinstance(m, torch.nn.Sequential):
            for c in m:
                yield from flat(c)
        else:
            yield m

    if not isinstance(module, torch.nn.Sequential):
        raise ValueError(f"mlp_from_module: expected a torch.nn.Sequential, got {type(module).__name__}")
    mods = [m for m in flat(module) if not isinstance(m, (torch.nn.Identity, torch.nn.Flatten))]
    acts = {torch.nn.Tanh: "tanh", torch.nn.ReLU: "relu"}
    for m in mods:
        if not isinstance(m, torch.nn.Linear) and type(m) not in acts:
            raise ValueError(f"mlp_from_module: unsupported module {type(m).__name__} (Linear, Tanh and ReLU only)")
    kinds = {acts[type(m)] for m in mods if type(m) in acts}
    if len(kinds) > 1:
        raise ValueError("mlp_from_module: one activation type only (Tanh or ReLU), got both")
    pattern = ["L" if isinstance(m, torch.nn.Linear) else "A" for m in mods]
    if pattern not in (["L", "A", "L"], ["L", "A", "L", "A", "L"]):
        raise ValueError(f"mlp_from_module: expected Linear, act, [Linear, act,] Linear; got "
                         f"{[type(m).__name__ for m in mods]} (1 or 2 hidden layers)")
    layers = []
    for m in mods:
        if isinstance(m, torch.nn.Linear):
            W = m.weight.detach().clone()
            b = m.bias.detach().clone() if m.bias is not None else torch.zeros(m.out_features, dtype=W.dtype)
            layers.append((W, b))
    if layers[-1][0].shape[0] not in (1, 2):
        raise ValueError(f"mlp_from_module: the output layer has {layers[-1][0].shape[0]} units; 1 or 2 supported")
    pol = {"kind": "mlp", "layers": layers, "activation": kinds.pop()}
    if group is not None:
        pol["group"] = group
    return pol


def action_log_prob(logit, action):
    """log P(action | logit) of the Bernoulli policy pi(alert) = sigmoid(logit): the decision rule of ``sample=True``
    (alert iff u < sigmoid(logit)) and SB3's two-way categorical on its two action values (logit = row1 - row0).
    Computed stably, elementwise and differentiably: -softplus(-logit) for action 1, -softplus(logit) for action 0.
    ``logit`` is a float tensor (as recorded in ``rollout(..., record=True)["trajectory"]["logit"]`` or recomputed by
    the learner), ``action`` anything that broadcasts with it (0 / 1, bool or u8).
    With ``require_budget=True`` the kernel forces the action to 0 when no budget is left, whatever the draw: such
    actions are off the policy's distribution, and their log-probability here is that of the policy, not of the
    forced choice -- mask them (or do not use require_budget) when computing on-policy ratios."""
    logit = logit if torch.is_tensor(logit) else torch.as_tensor(logit)
    a = torch.as_tensor(action, device=logit.device).to(torch.bool)
    return -torch.nn.functional.softplus(torch.where(a, -logit, logit))
