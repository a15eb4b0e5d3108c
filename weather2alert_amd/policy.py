"""Linear-logistic policies for ``HeatAlertVecEnv.rollout({"kind": "linear", ...})`` (csrc/w2a_rollout_linear.hip.h).

The host side of w2a_rollout_linear: argument checks, the permutation of the parameters from observation order (the
columns of ``env.feature_names``) into the kernels' 32-slot feature-row order (``CompiledTables.obs_slot``), and the
per-group reduction of the returns. Nothing here launches a kernel, so all of it runs on the CPU as well.

    {"kind": "linear",
     "weight": W,             # float [G, n_obs], columns in observation order
     "bias": b,               # float [G]
     "group": g,              # int [num_envs] in [0, G); may be omitted when G == 1
     "sample": False,         # False: alert iff logit > 0; True: alert iff u < sigmoid(logit)
     "seed": 0,               # sample=True only: keys the Bernoulli policy's counter-RNG uniform u
     "require_budget": False} # never attempt an alert with no budget left
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

ROW_FLOATS = 32
LOGIT_SLOTS = 30  # slots the day loop multiplies (0..29); an observation column elsewhere cannot be served
KEYS = {"kind", "weight", "bias", "group", "sample", "seed", "require_budget"}


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


def check_linear_policy(policy: dict, n_obs: int, num_envs: int, obs_slot, device) -> LinearPolicyArgs:
    """Validate a {"kind": "linear", ...} policy (ValueError on anything the kernel could not run as asked) and bring its
    parameters into the kernel's form on `device`. One host reduction: the range of the group ids."""
    unknown = set(policy) - KEYS
    if unknown:
        raise ValueError(f"linear policy: unknown key(s) {sorted(unknown)}; choose from {sorted(KEYS)}")
    w = _tensor(policy.get("weight"), "weight", device)
    if w.is_complex() or not (w.is_floating_point() or w.dtype in (torch.int32, torch.int64)):
        raise ValueError(f"linear policy: weight must be real numbers, got {w.dtype}")
    if w.dim() != 2 or w.shape[1] != n_obs or w.shape[0] < 1:
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
    return LinearPolicyArgs(to_slot_order(w, obs_slot, n_obs).contiguous(), b, g, G, bool(sample),
                            int(seed) & (2**64 - 1), bool(rb))


def group_mean(values: torch.Tensor, group: torch.Tensor | None, n_groups: int) -> torch.Tensor:
    """f32 [n_groups]: the mean of `values` over each group's envs (NaN for a group without envs), on the device of
    `values`: the groups' segments of the values sorted by group, summed as differences of one fp64 prefix sum. (An
    index_add into n_groups fp64 cells measured 7.7 ms at 1 048 576 envs and G = 1024 -- four times the rollout it
    follows -- every env's atomic contending with a thousand others for its cell; this is a sort and a scan.)"""
    if group is None:
        return values.to(torch.float32).mean().reshape(1)
    sg, perm = torch.sort(group.to(torch.int32))
    csum = torch.cat([torch.zeros(1, dtype=torch.float64, device=values.device),
                      torch.cumsum(values.to(torch.float64)[perm], dim=0)])
    ids = torch.arange(n_groups, dtype=torch.int32, device=values.device)
    lo = torch.searchsorted(sg, ids, right=False)
    hi = torch.searchsorted(sg, ids, right=True)
    return ((csum[hi] - csum[lo]) / (hi - lo).to(torch.float64)).to(torch.float32)
