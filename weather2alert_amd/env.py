"""Vectorised, MI355X-resident HeatAlertEnv with the reference's reset()/step() surface.

``HeatAlertVecEnv`` steps ``num_envs`` independent copies of the reference's
``weather2alert.env.HeatAlertEnv`` (``/root/reference/src/weather2alert/env.py``) inside
hand-written gfx950 kernels (``csrc/*.hip.h``, ``csrc/w2a_kernels.hip`` through the C ABI of
``include/w2a.h``). ``HeatAlertEnv`` is the ``num_envs=1`` drop-in with the reference's
exact constructor / ``reset`` / ``step`` signatures and NumPy-seed parity.

All reference quirks listed in SURVEY.md §3.3 (Q1-Q12) are reproduced; there is no CPU
fallback -- constructing an env without a ROCm device or without libw2a.so raises.
"""
from __future__ import annotations

import ctypes as C
import types
from typing import Literal

import numpy as np
import torch

from . import _ffi, policy as _policy, stats as _stats
from .info import _LazyInfo
from .options import KernelOptions
from .rng import numpy_parity_episode
from .spaces import Box, Discrete
from .tables import CompiledTables, DeviceTables, compile_from_files

_ACT_CODES = {torch.int32: _ffi.ACT_I32, torch.int64: _ffi.ACT_I64, torch.uint8: _ffi.ACT_U8,
              torch.bool: _ffi.ACT_U8}
_BUDGET_MODES = {"less_than": _ffi.BUDGET_LESS_THAN, "centered": _ffi.BUDGET_CENTERED}
_cur_device = getattr(torch._C, "_cuda_getDevice", torch.cuda.current_device)

try:  # a real Gymnasium VectorEnv when the package is importable; the same duck-typed surface otherwise
    from gymnasium.vector import VectorEnv as _VectorEnvBase
except ImportError:  # gymnasium is not a dependency of the reference's numerical path
    _VectorEnvBase = object
try:  # gymnasium >= 1.0 names the autoreset behaviour of a vector env with this enum (metadata["autoreset_mode"])
    from gymnasium.vector import AutoresetMode as _AutoresetMode
except ImportError:
    _AutoresetMode = None


def _check_learned(env, policy: dict):
    """check_linear_policy / check_mlp_policy with what the "lookahead" key's feature check needs from the env (module
    level, as _refuse_lookahead: the entry points read nothing of the env but its tables and settings before they refuse)."""
    ct = env.ct
    check = _policy.check_linear_policy if policy.get("kind") == "linear" else _policy.check_mlp_policy
    return check(policy, ct.n_obs, env.num_envs, ct.obs_slot, env.device, ct.feature_names, env.fixes,
                 ct.slot_of.get("alerts_2wks", -1))


def _refuse_lookahead(policy, who: str):
    """The learners whose kernels do not read the lookahead inputs yet."""
    if isinstance(policy, dict) and policy.get("lookahead") is not None:
        raise ValueError(f"{who} does not take a 'lookahead' policy yet: its kernels do not read the lookahead "
                         "inputs (rollout(), rollout(linear, policy_gradient=...) and imitation_gradient(linear) do)")


def _autoreset_metadata(mode: str):
    """metadata["autoreset_mode"]: gymnasium's AutoresetMode member when the package has one, else the plain string."""
    if _AutoresetMode is None:
        return mode
    return {"same_step": _AutoresetMode.SAME_STEP, "next_step": _AutoresetMode.NEXT_STEP,
            "disabled": _AutoresetMode.DISABLED}[mode]


class HeatAlertVecEnv(_VectorEnvBase):
    """``num_envs`` heat-alert environments stepped in lock step on one MI355X.

    Constructor keeps the reference's keyword arguments (env.py:20-29) and adds:

    num_envs, device     batch size and ROCm device
    seed_mode            "device": every draw of reset() comes from the counter-based device RNG
                         keyed by (seed, global env id, episode number) -- same distributions as
                         the reference, not the same stream; "numpy_parity": the host replays
                         NumPy's Generator call sequence of env.py:145-177 per env (env i is
                         seeded with seed+i), bit-identical episode tuples to the reference.
    autoreset            "same_step" (finished envs restart inside the same step() call and the
                         returned observation is the new episode's first one; the finished
                         episode's return is in info["final_return"]) or "disabled". same_step is what SB3's
                         DummyVecEnv does around the reference env and Gymnasium's AutoresetMode.SAME_STEP
                         (``metadata["autoreset_mode"]``). No ``final_obs`` is returned: the reference's terminal
                         step hands back the PREVIOUS step's observation unchanged (env.py:257-262, Q6), i.e. a row
                         the caller already holds, and episodes end by termination only (no truncation to
                         bootstrap from). "next_step" is Gymnasium's AutoresetMode.NEXT_STEP (what
                         SyncVectorEnv does by default around the reference env): the terminal step returns done =
                         True with the stale observation; on the NEXT call a finished env ignores its action, starts
                         its next episode and returns that episode's first observation with reward 0 and done =
                         False. Per env the sequence of episodes is the same as with "same_step" (device seed mode
                         only).
    episode_order        "iid" (default): env i keeps its own independent draws, like N reference envs;
                         "sorted": after every (lock-step) reset the envs are relabelled so that env indices
                         follow the coefficient row. The batch holds exactly the same multiset of
                         episodes, only which index holds which episode changes (env identity is not preserved
                         across episodes); neighbouring envs then share table lines and the step kernel's
                         gathers become L2 hits. Needs seed_mode="device" and a uniform episode length.
    lockstep             how same-step autoreset is driven in device seed mode. True: every episode has the same
                         length and the whole batch resets together, so the host counts steps and launches the
                         reset kernel after the terminal step (the step kernel then runs its leaner, full-occupancy
                         variant). False: each env restarts inside the step kernel whenever it finishes (needed
                         after partial resets, and what a loop recorded into a hipGraph needs: no reset can be
                         launched between two recorded steps; a batch that is in lock step anyway keeps the packed
                         16-B state there too). None (default): True when the tables allow it; falls back to
                         False by itself after a masked reset.
                         hipGraphs: step() neither synchronises nor allocates and reads the day from device memory;
                         step once eagerly, then capture (torch.cuda.graph, or record_steps() below, which also reads the
                         status word behind every replay). Needs lockstep=False or autoreset="disabled": a loop whose
                         episode boundaries the host drives (the default in lock step: it counts days and launches the
                         reset) cannot be recorded, and step() raises instead of recording it. The library keeps the form
                         of the state the recorded steps work on current from then on (include/w2a.h, w2a_state_bytes).
    faithful / fixes     faithful=True (default) reproduces every reference quirk -- all parity
                         claims refer to this mode. ``fixes`` opts into individual corrections (faithful=False =
                         all of them): "alert_2wks" (Q1: the agent's 14-day count feeds the reward), "lag" (Q3:
                         alert_lag1 is yesterday's action), "penalty" (Q5: -1 for an alert attempted at budget),
                         "obs" (Q6: step() returns the next day's row), "augment" (Q8: the drawn similar county
                         supplies weather and coefficients), "budget" (Q9: per-episode budgets, no stickiness).
    reward_mode          "sampled" (default, the reference: one posterior draw per episode, env.py:160,209,216) or
                         "posterior_mean": every step's reward is the mean over ALL posterior draws of the env's
                         coefficient column -- the legacy env's eval mode (_deprecated/env.py:332-342) on today's
                         reward form -- one grouped contraction per step (csrc/w2a_posterior.hip.h).
                         Needs lock-step / disabled autoreset and faithful semantics.
    kernel               KernelOptions (weather2alert_amd/options.py): the switches that select HOW a step, a rollout
                         or the posterior-mean reward is computed -- step_kernel, write_obs, rollout_order, rollout_mfma,
                         pm_kernel, reward_path -- never what; each may also be passed by name (step_kernel="wide", ...).
                         Every combination gives the same results up to the order of the fp64 additions (~1e-7 for
                         the posterior-mean kernels); the defaults are the fastest choice on MI355X.
    pm_sync_group        pm_kernel="auto" only: a torch.distributed process group (True = the default group) whose ranks
                         must all use the kernel its first rank measured fastest -- the choice is then BROADCAST inside the
                         first reset() (a collective: every rank of the group must get there). Default None: no
                         communication, each process keeps its own choice; for one kernel on every rank without a
                         collective pass pm_kernel=<name> (the default "matrix_i8" is such a name).
    tables               pre-compiled CompiledTables (skips file loading)
    env_gid0             global id of env 0 (multi-GPU sharding keeps results shard-invariant)
    """

    metadata = {"autoreset_mode": _autoreset_metadata("same_step")}  # the default; instances carry their own mode
    spec = None
    render_mode = None
    closed = False

    def __init__(
        self,
        num_envs: int = 1,
        weights: str = "nn_full_medicare_all",
        years: list | None = None,
        fips_list: list | None = None,  # ignored, like the reference (overwritten at env.py:75)
        similar_climate_counties: bool = False,
        budget: int | None = None,
        data_dir: str | None = None,
        split: str = "65k",
        device: str | torch.device = "cuda:0",
        seed_mode: Literal["device", "numpy_parity"] = "device",
        autoreset: Literal["same_step", "next_step", "disabled"] = "same_step",
        tables: CompiledTables | DeviceTables | None = None,
        env_gid0: int = 0,
        episode_order: Literal["iid", "sorted"] = "iid",
        lockstep: bool | None = None,
        faithful: bool = True,
        fixes: set | list | None = None,
        reward_mode: Literal["sampled", "posterior_mean"] = "sampled",
        kernel: KernelOptions | None = None,
        pm_sync_group=None,
        **kernel_overrides,  # any field of KernelOptions by name (step_kernel=..., pm_kernel=..., write_obs=..., ...)
    ):
        # HOW things are computed (never what): one record, weather2alert_amd/options.py
        self.kernel = (kernel or KernelOptions()).with_overrides(**kernel_overrides)
        write_obs, step_kernel, pm_kernel = self.kernel.write_obs, self.kernel.step_kernel, self.kernel.pm_kernel
        rollout_order, rollout_mfma = self.kernel.rollout_order, self.kernel.rollout_mfma
        self._lib = _ffi.load()
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("HeatAlertVecEnv needs a ROCm GPU (device='cuda:N'); there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if num_envs <= 0:
            raise ValueError("num_envs must be positive")
        if seed_mode not in ("device", "numpy_parity"):
            raise ValueError(f"seed_mode {seed_mode!r}")
        if autoreset not in ("same_step", "next_step", "disabled"):
            raise ValueError(f"autoreset {autoreset!r}")
        if autoreset == "next_step" and seed_mode != "device":
            raise ValueError("autoreset='next_step' needs seed_mode='device'")
        self.num_envs = int(num_envs)
        self.similar_climate_counties = bool(similar_climate_counties)
        self.seed_mode = seed_mode
        self.autoreset = autoreset
        self.metadata = {**type(self).metadata, "autoreset_mode": _autoreset_metadata(autoreset)}
        self.env_gid0 = int(env_gid0)
        self.write_obs = bool(write_obs)
        self._ctor_budget = budget
        if isinstance(tables, DeviceTables):
            if tables.device != self.device:
                raise ValueError(f"tables live on {tables.device}, the env on {self.device}")
            self.dtables = tables
        else:
            ct = tables if tables is not None else compile_from_files(data_dir, weights, split, years)
            self.dtables = DeviceTables(ct, self.device)
        reward_path = "gather"
        allf = set(_ffi.FIX_BITS) | {"budget"}
        self.fixes = set(allf) if (not faithful and fixes is None) else set(fixes or ())
        if self.fixes - allf:
            raise ValueError(f"unknown fixes {sorted(self.fixes - allf)}; choose from {sorted(allf)}")
        self.reward_path = reward_path
        self.step_kernel = step_kernel
        if reward_mode not in ("sampled", "posterior_mean"):
            raise ValueError(f"reward_mode {reward_mode!r}")
        if reward_mode == "posterior_mean" and (self.fixes or step_kernel == "classic"):
            raise ValueError("reward_mode='posterior_mean' needs faithful semantics and the 64-envs-per-wave step kernel")
        self.reward_mode = reward_mode
        self.pm_kernel = pm_kernel
        self.pm_kernel_choice = None if pm_kernel == "auto" else pm_kernel  # decided after the first reset
        self.pm_kernel_timing_us: dict = {}
        self.pm_sync_group = pm_sync_group
        self.rollout_order = bool(rollout_order)  # rollout() visits the envs in feature-row order (speed only; A/B)
        # rollout(): the table-sourced part of the logits on the int8 matrix cores (needs the visiting order, a batch in
        # lock step and faithful semantics; speed only; A/B)
        self.rollout_mfma = bool(rollout_mfma)
        self._mfma_ws = None
        self.pm_rollout_kernel = True  # posterior_mean rollouts in one launch when possible (False: per-day launches)
        # which path the last posterior_mean rollout() took: "k_pm_rollout" / "k_pm_rollout_i8" (one launch), "per_day"
        # (policy kernel + reward kernel + step kernel per day), None before the first one or when no env had a day left
        self.last_pm_rollout: str | None = None
        self._order_stale = True
        if episode_order not in ("iid", "sorted"):
            raise ValueError(f"episode_order {episode_order!r}")
        if episode_order == "sorted" and seed_mode != "device":
            raise ValueError("episode_order='sorted' needs seed_mode='device'")
        self.episode_order = episode_order
        ct = self.ct = self.dtables.ct
        self.fips_list = ct.fips_list
        self.valid_years = ct.years
        self.n_samples = ct.n_samples
        self.feature_names = ct.feature_names
        self._fips_pos = {f: i for i, f in enumerate(ct.fips_list)}
        # Q12: the true observation width (the reference declares len(columns)+2 = 33, env.py:88)
        self.single_observation_space = Box(-np.inf, np.inf, (ct.n_obs,), np.float32)
        self.single_action_space = Discrete(2)  # env.py:95
        self.observation_space = Box(-np.inf, np.inf, (self.num_envs, ct.n_obs), np.float32)
        self.action_space = self.single_action_space

        n, dev = self.num_envs, self.device
        with torch.cuda.device(dev):
            nbytes = self._lib.w2a_state_bytes(n)
            self._state = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
            self._status = torch.zeros(1, dtype=torch.int32, device=dev)
            self._obs = torch.zeros((n, ct.n_obs), dtype=torch.float32, device=dev)
            self._reward = torch.zeros(n, dtype=torch.float32, device=dev)
            self._done = torch.zeros(n, dtype=torch.uint8, device=dev)
            self._final_return = torch.zeros(n, dtype=torch.float32, device=dev)
            self._truncated = torch.zeros(n, dtype=torch.bool, device=dev)
            h = C.c_void_p()
            _ffi.check(self._lib.w2a_create(C.byref(self.dtables.struct), n, self.env_gid0, self._state.data_ptr(),
                                            nbytes, self._status.data_ptr(), C.byref(h)), "w2a_create")
        self._h = h
        bits = sum(_ffi.FIX_BITS[k] for k in self.fixes if k in _ffi.FIX_BITS)
        if bits:
            _ffi.check(self._lib.w2a_set_semantics(h, bits), "w2a_set_semantics")
        if reward_mode == "posterior_mean" and self.pm_kernel_choice is not None:
            _ffi.check(self._lib.w2a_set_posterior_kernel(h, _ffi.PM_KERNELS[self.pm_kernel_choice]),
                       "w2a_set_posterior_kernel")
        if self.kernel.force_wide_episode_word:
            _ffi.check(self._lib.w2a_set_episode_word(h, 1), "w2a_set_episode_word")
        # hot-path constants (step() is called millions of times: no per-call attribute chains)
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._obs_ptr = self._obs.data_ptr() if self.write_obs else None
        self._rew_ptr, self._done_ptr = self._reward.data_ptr(), self._done.data_ptr()
        self._fr_ptr = self._final_return.data_ptr()
        self._done_bool = self._done.view(torch.bool)
        self._sort_ws = None
        self._order_ws = None
        self._look_tables = {}  # feature -> f32 [S_w * Y, T] series table (lookahead_table(); built on first use)
        self._group_ws = None
        if reward_mode == "posterior_mean":
            with torch.cuda.device(dev):
                self._group_ws = torch.empty(self._lib.w2a_group_workspace_bytes(n, ct.S, ct.n_samples), dtype=torch.uint8,
                                             device=dev)
        nd = np.unique(ct.n_days)
        uniform = len(nd) == 1 and nd[0] > 0
        if episode_order == "sorted":
            if not uniform:
                raise ValueError("episode_order='sorted' needs one episode length for every (county, year)")
            if lockstep is False:
                raise ValueError("episode_order='sorted' implies lockstep")
            with torch.cuda.device(dev):
                self._sort_ws = torch.empty(self._lib.w2a_sort_workspace_bytes(n), dtype=torch.uint8, device=dev)
        if lockstep and not uniform:
            raise ValueError("lockstep=True needs one episode length for every (county, year)")
        self._episode_len = int(nd[0]) if uniform else 0
        self._lockstep = bool(uniform and self.seed_mode == "device" and lockstep is not False)
        self._steps_in_episode = 0
        self._pending_reset = False  # next_step autoreset in lock step: the terminal step has run, the next call restarts
        self._reset_cfg = None
        self._set_step_mode()
        self._w2a_step = self._lib.w2a_step
        self._raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        self._sticky = [budget] * n  # host mirror of self.budget per env (numpy_parity mode, Q9)
        self._needs_reset = True
        # the observation buffer holds the row every env's agent holds (rollout(kind="linear") reads it on its first day):
        # after reset(), step() and linear rollouts that wrote it; not after built-in rollouts (they write no rows)
        self._obs_current = False
        self._last_opts: dict = {}
        self._np_random = None
        self._np_random_seed = None

    # ------------------------------------------------------------------ Gymnasium VectorEnv attributes
    @property
    def unwrapped(self):
        return self

    @property
    def np_random(self) -> np.random.Generator:
        """Host Generator seeded by the last explicit reset(seed=...) (Gymnasium convention). Episode draws come
        from the device RNG (seed_mode="device") or from per-env Generators (seed_mode="numpy_parity"), not from
        this one; it serves wrappers and samplers that expect the attribute."""
        if self._np_random is None:
            self._np_random_seed = int(np.random.SeedSequence().entropy % (2**63))
            self._np_random = np.random.default_rng(self._np_random_seed)
        return self._np_random

    @np_random.setter
    def np_random(self, value: np.random.Generator):
        self._np_random, self._np_random_seed = value, -1

    @property
    def np_random_seed(self):
        self.np_random  # noqa: B018  (initialises on first use)
        return self._np_random_seed

    # ------------------------------------------------------------------ plumbing
    def _set_step_mode(self):
        """in-kernel autoreset only when the batch is not in lock step (device seed mode)."""
        auto = self.autoreset in ("same_step", "next_step") and self.seed_mode == "device"
        self._dev_auto = auto and not self._lockstep
        # lock step: the host counts days and launches the reset kernel right after the terminal step (same_step) or at
        # the start of the following call (next_step: _pending_reset)
        self._host_auto = auto and self._lockstep and self.autoreset == "same_step"
        self._host_next = auto and self._lockstep and self.autoreset == "next_step"
        if not self._host_next:
            self._pending_reset = False  # envs left finished by a terminal step restart inside the kernel from here on
        if self.reward_mode == "posterior_mean" and self._dev_auto:
            raise ValueError("reward_mode='posterior_mean' cannot run with the in-kernel autoreset (batches that left "
                             "lock step); use autoreset='disabled' or whole-batch resets")
        self._pm = self.reward_mode == "posterior_mean"
        # episode boundaries driven from this class (a counted reset launch, a pending restart, NumPy draws on the host): such
        # a loop cannot be recorded into a hipGraph -- w2a_step then refuses to record instead of baking a reset into a
        # fixed position of the graph, or none at all (W2A_STEP_NO_CAPTURE; the query costs nothing extra)
        host_driven = self._host_auto or self._host_next or (self.autoreset == "same_step" and not self._dev_auto)
        self._step_flags = ((0 if self.write_obs else _ffi.STEP_NO_OBS) |
                            (_ffi.STEP_NO_CAPTURE if host_driven else 0) |
                            (_ffi.STEP_REWARD_GIVEN if self._pm else 0) |
                            (_ffi.STEP_CLASSIC if self.step_kernel == "classic" else 0) |
                            (_ffi.STEP_WIDE if self.step_kernel in ("wide", "wide_unpacked") else 0) |
                            (_ffi.STEP_UNPACKED if self.step_kernel in ("unpacked", "wide_unpacked") else 0) |
                            (_ffi.STEP_AUTORESET if self._dev_auto else 0) |
                            (_ffi.STEP_NEXT_STEP if self._dev_auto and self.autoreset == "next_step" else 0))

    @property
    def step_kernel_name(self) -> str:
        """The step kernel w2a_step launches for this env right now (mirrors the dispatch in csrc/w2a_kernels.hip)."""
        wide = self._pm or self.step_kernel in ("wide", "wide_unpacked") or (self.step_kernel in ("auto", "unpacked") and
                                                          self.num_envs >= _ffi.S64_MIN_ENVS)
        return "k_step64" if (wide and self.step_kernel != "classic") else "k_step"

    @property
    def last_step_kernel(self) -> str | None:
        """Which kernel the last step() launched, from the library's own record: "k_step" (4 lanes per env), "k_step64"
        (64 envs per wave, canonical state words), "k_step64<packed>" (the lock-step mirror) or None before the first."""
        return {0: "k_step", 1: "k_step64", 2: "k_step64<packed>"}.get(
            self._lib.w2a_query(self._h, _ffi.Q_LAST_STEP_KERNEL))

    @property
    def packed_state(self) -> bool:
        """The library currently holds the step state in its packed lock-step form (the last step ran the packed
        variant of the 64-envs-per-wave kernel)."""
        return bool(self._lib.w2a_query(self._h, _ffi.Q_PACKED_CURRENT)) and not bool(
            self._lib.w2a_query(self._h, _ffi.Q_CANONICAL_CURRENT))

    @property
    def episode_word_bytes(self) -> int:
        """Bytes per env of the lock-step mirror's per-episode word on this handle: 4 (both row indices in one word, the
        library's choice wherever the table dims allow it) or 8 (csrc/w2a_episode_word.h)."""
        return int(self._lib.w2a_query(self._h, _ffi.Q_EPISODE_WORD_BYTES))

    @property
    def last_rollout_kernel(self) -> str | None:
        """Which kernel the last sampled-reward rollout() launched: "k_rollout_mfma" (int8 matrix cores), "k_rollout64"
        (lane = env, vector ALU), "k_rollout" (4 lanes per env), "k_rollout_linear" (kind="linear"), "k_rollout_mlp"
        (kind="mlp") or None before the first one."""
        return _ffi.ROLLOUT_KERNELS.get(self._lib.w2a_query(self._h, _ffi.Q_LAST_ROLLOUT_KERNEL))

    def _stream(self):
        if self._raw_stream is not None:
            return self._raw_stream(self._dev_index)
        return torch.cuda.current_stream(self.device).cuda_stream

    def close(self, **kwargs):
        if getattr(self, "_h", None):
            torch.cuda.synchronize(self.device)
            self._lib.w2a_destroy(self._h)
            self._h = None
        self._look_tables = {}  # the series tables of lookahead_table()
        self.closed = True

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def check_status(self) -> int:
        """Synchronise and raise if a kernel flagged bad inputs since the last call."""
        out = C.c_int32(0)
        with torch.cuda.device(self.device):
            _ffi.check(self._lib.w2a_read_status(self._h, C.byref(out), self._stream()), "w2a_read_status")
        return self._raise_for_status(out.value)

    @property
    def status_word(self) -> torch.Tensor:
        """The device status word (int32 [1], W2A_ST_* bits, sticky until check_status() clears it): what a loop that
        must not synchronise -- a replayed hipGraph -- copies out or asserts on."""
        return self._status

    @staticmethod
    def _raise_for_status(bits: int) -> int:
        if bits & _ffi.ST_BAD_EPISODE:
            raise KeyError("reset: an episode tuple is out of range or has no data "
                           "(reference: KeyError at env.py:127 / ValueError at env.py:121)")
        if bits & _ffi.ST_BAD_ACTION:
            raise ValueError("step: actions must be 0 or 1 (action_space = Discrete(2))")
        if bits & _ffi.ST_STALE_GRAPH:
            raise RuntimeError("a replayed hipGraph holds step() calls on the packed lock-step form of this env's state, "
                               "which could not be kept current (a masked reset or a restored checkpoint since the "
                               "capture took the batch out of lock step): those replayed steps did nothing. Reset the "
                               "whole batch (or capture again) before replaying (include/w2a.h, w2a_state_bytes)")
        return bits

    def state(self) -> dict[str, torch.Tensor]:
        """Decoded per-env integer state (device tensors)."""
        return self._state_packed()[1]

    def _state_packed(self, fields=None):
        """(one int32 [n_fields, N] buffer, dict of per-field views into it): a single D2H copy fetches all.
        fields: decode only these (w2a_state_view: a NULL array is skipped)."""
        v = _ffi.StateView()
        names = _ffi.STATE_FIELDS if fields is None else [k for k in _ffi.STATE_FIELDS if k in fields]
        buf = torch.empty((len(names), self.num_envs), dtype=torch.int32, device=self.device)
        out = {}
        for i, k in enumerate(names):
            out[k] = buf[i].view(torch.float32) if k == "episode_return" else buf[i]
            setattr(v, k, buf[i].data_ptr())
        with torch.cuda.device(self.device):
            _ffi.check(self._lib.w2a_get_state(self._h, C.byref(v), self._stream()), "w2a_get_state")
        return buf, out

    # ------------------------------------------------------------------ checkpoint / resume
    def state_dict(self) -> dict:
        """Everything needed to resume this batch bit-exactly: the packed per-env state (episode tuples,
        counters, returns, sticky budgets, episode numbers), the last observations and the host-side mirrors.
        (The reference env has no save/restore)"""
        self.state()  # brings the canonical arrays up to date (the library may hold the packed lock-step form)
        return {
            "state": self._state.clone(), "obs": self._obs.clone(), "final_return": self._final_return.clone(),
            "reward": self._reward.clone(), "done": self._done.clone(),
            "host": {"sticky": list(self._sticky), "steps_in_episode": self._steps_in_episode,
                     "lockstep": self._lockstep, "reset_cfg": self._reset_cfg, "last_opts": dict(self._last_opts),
                     "needs_reset": self._needs_reset, "pending_reset": self._pending_reset, "info_location": list(getattr(self, "_info_location", [])),
                     "num_envs": self.num_envs, "env_gid0": self.env_gid0,
                     # format of "state": w2a_state_bytes grew with ABI 17 (the mirror's day words); the canonical part
                     # at its front (header, cold, hot3, stepc) is what a restore needs
                     "abi_version": _ffi.ABI_VERSION, "state_bytes": int(self._state.numel()),
                     # pm_kernel="auto" measures; a resumed run must compute rewards with the same kernel to stay
                     # bit-exact with the run it continues (the kernels agree to ~1e-7, not to the last bit)
                     "pm_kernel_choice": self.pm_kernel_choice},
        }

    def load_state_dict(self, sd: dict) -> None:
        h = sd["host"]
        if h["num_envs"] != self.num_envs or h["env_gid0"] != self.env_gid0:
            raise ValueError("state_dict belongs to a different env batch (num_envs / env_gid0 differ)")
        hdr = self._state[:256].clone()  # slot map written by w2a_create for THIS handle
        src = sd["state"]
        if src.numel() == self._state.numel():
            self._state.copy_(src)
        else:
            # a checkpoint of another build of the library (the lock-step mirror behind the canonical words changed size):
            # the canonical part -- header, cold 16 B, hot3 12 B, stepc 12 B per env, each array on a 256-B boundary -- has
            # had the same layout in every ABI version; w2a_invalidate rebuilds everything derived from it
            a256 = lambda x: (x + 255) & ~255  # noqa: E731
            canon = 256 + a256(16 * self.num_envs) + 2 * a256(12 * self.num_envs)
            if src.numel() < canon or self._state.numel() < canon:
                raise ValueError(f"state_dict['state'] holds {src.numel()} bytes (written by ABI {h.get('abi_version', '<= 17')}); "
                                 f"this build (ABI {_ffi.ABI_VERSION}) needs at least the {canon} canonical bytes of "
                                 f"{self.num_envs} envs: not a checkpoint of this env batch")
            self._state[:canon].copy_(src[:canon])
        self._state[:256].copy_(hdr)
        self._obs_current = False  # which row each agent held is not part of the checkpoint's guarantees
        # the state buffer changed behind the library: it forgets what it derived and scans the restored buffer for its
        # largest budget, sticky ones included (waits for this stream -- the one the copy above ran on -- and no other)
        with torch.cuda.device(self.device):
            _ffi.check(self._lib.w2a_invalidate(self._h, self._stream()), "w2a_invalidate")
        self._obs.copy_(sd["obs"])
        self._final_return.copy_(sd["final_return"])
        self._reward.copy_(sd["reward"])
        self._done.copy_(sd["done"])
        self._sticky = list(h["sticky"])
        self._steps_in_episode, self._lockstep = h["steps_in_episode"], h["lockstep"]
        self._reset_cfg, self._last_opts, self._needs_reset = h["reset_cfg"], dict(h["last_opts"]), h["needs_reset"]
        if h["info_location"]:
            self._info_location = list(h["info_location"])
        self._set_step_mode()
        self._pending_reset = bool(h.get("pending_reset", False)) and self._host_next
        if self._reset_cfg is not None:
            with torch.cuda.device(self.device):
                _ffi.check(self._lib.w2a_set_autoreset(self._h, *self._reset_cfg), "w2a_set_autoreset")
        if self._pm and h.get("pm_kernel_choice") in _ffi.PM_KERNELS:  # continue on the kernel the checkpointed run used
            self.pm_kernel_choice = h["pm_kernel_choice"]
            _ffi.check(self._lib.w2a_set_posterior_kernel(self._h, _ffi.PM_KERNELS[self.pm_kernel_choice]),
                       "w2a_set_posterior_kernel")
        self._regroup()  # posterior_mean: the restored episode tuples need their own column grouping

    # ------------------------------------------------------------------ reset
    def _opt(self, options, key, default):
        v = None if options is None else options.get(key)
        return default if v is None else v

    def reset(self, seed: int | list | None = None, options: dict | None = None):
        """Gymnasium VectorEnv.reset. ``options`` carries the reference's reset kwargs
        (env.py:133-141): location, similar_climate_counties, budget, sample_budget,
        sample_budget_type -- scalars, or per-env sequences in numpy_parity mode -- plus
        "episodes": dict of int arrays (county_w, year_i, coef_col, sample, budget) to inject
        episode tuples directly, and "mask": bool[num_envs] to reset a subset."""
        options = dict(options or {})
        if seed is not None and not isinstance(seed, (list, tuple, np.ndarray)):
            self._np_random, self._np_random_seed = np.random.default_rng(int(seed)), int(seed)
        mask = options.get("mask")
        mask_t = None
        if mask is not None:
            mask_t = torch.as_tensor(np.asarray(mask), dtype=torch.uint8, device=self.device)
        obs_ptr = self._obs.data_ptr() if self.write_obs else None
        self._last_opts = {k: v for k, v in options.items() if k not in ("mask", "episodes")}
        if self._lockstep and (mask is not None or "episodes" in options):
            if self.episode_order == "sorted":
                raise ValueError("episode_order='sorted' resets the whole batch with the device RNG only")
            self._lockstep = False  # partial / injected resets: envs finish at different times from now on
            self._set_step_mode()
        if "episodes" in options:
            self._reset_tuples(options["episodes"], mask_t, obs_ptr)
            if self.seed_mode == "device" and self.autoreset in ("same_step", "next_step"):
                # later episodes of these envs come from the device RNG (in-kernel autoreset)
                self._reset_cfg = self._device_cfg(seed, self._last_opts)
                with torch.cuda.device(self.device):
                    _ffi.check(self._lib.w2a_set_autoreset(self._h, *self._reset_cfg), "w2a_set_autoreset")
        elif self.seed_mode == "numpy_parity":
            self._reset_numpy_parity(seed, options, mask, mask_t, obs_ptr)
        else:
            self._reset_device(seed, options, mask_t, obs_ptr)
        self._needs_reset = False
        if mask is None:  # a masked reset leaves the other envs' rows as they were
            self._obs_current = self.write_obs
        return self._obs, self._info()

    def _reset_tuples(self, ep: dict, mask_t, obs_ptr):
        ct, n = self.ct, self.num_envs
        arrs = {}
        for k in ("county_w", "year_i", "coef_col", "sample"):
            a = np.broadcast_to(np.asarray(ep[k], dtype=np.int64), (n,))
            arrs[k] = a
        lim = {"county_w": ct.S_w, "year_i": ct.Y, "coef_col": ct.S, "sample": ct.n_samples}
        sel = np.ones(n, bool) if mask_t is None else mask_t.cpu().numpy().astype(bool)
        for k, a in arrs.items():
            if ((a[sel] < 0) | (a[sel] >= lim[k])).any():
                raise KeyError(f"reset: {k} outside [0, {lim[k]})")
        rows = arrs["county_w"] * ct.Y + arrs["year_i"]
        if (ct.n_days[rows[sel]] <= 0).any():
            raise KeyError("reset: (county, year) has no data (reference: KeyError at env.py:127)")
        if ep.get("budget") is None:
            bud = ct.B0[rows].astype(np.int64)
        else:
            bud = np.broadcast_to(np.asarray(ep["budget"], dtype=np.int64), (n,))
        dev = self.device
        t = {k: torch.from_numpy(np.array(a, dtype=np.int32)).to(dev) for k, a in arrs.items()}
        tb = torch.from_numpy(np.array(bud, dtype=np.int32)).to(dev)
        with torch.cuda.device(dev):
            _ffi.check(self._lib.w2a_reset(self._h, t["county_w"].data_ptr(), t["year_i"].data_ptr(),
                                           t["coef_col"].data_ptr(), t["sample"].data_ptr(), tb.data_ptr(),
                                           None if mask_t is None else mask_t.data_ptr(), obs_ptr, self._stream()),
                       "w2a_reset")
        self._keep = (t, tb, mask_t)  # keep inputs alive until the async launch has consumed them
        self._regroup()

    def _per_env(self, v, i):
        if isinstance(v, (list, tuple, np.ndarray)):
            return v[i]
        return v

    def _reset_numpy_parity(self, seed, options, mask, mask_t, obs_ptr):
        """Host replay of env.py:143-178 per env with NumPy's own Generator."""
        ct, n = self.ct, self.num_envs
        loc_o = options.get("location")
        aug_o = self._opt(options, "similar_climate_counties", self.similar_climate_counties)
        bud_o = options.get("budget")
        sb_o = self._opt(options, "sample_budget", False)
        sbt_o = self._opt(options, "sample_budget_type", "less_than")
        cw, yi, cc, sm, bd = (np.zeros(n, np.int64) for _ in range(5))
        self._info_location = getattr(self, "_info_location", [None] * n)
        sel = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
        for i in range(n):
            if not sel[i]:
                continue
            if seed is None:
                s = np.random.randint(0, 10000)  # env.py:143-144
            elif isinstance(seed, (list, tuple, np.ndarray)):
                s = int(seed[i])
            else:
                s = int(seed) + i
            aug = bool(self._per_env(aug_o, i))
            w, y_i, li, ci, b, self._info_location[i] = numpy_parity_episode(
                ct, s, self._per_env(loc_o, i), aug, self._sticky[i], self._per_env(bud_o, i),
                bool(self._per_env(sb_o, i)), self._per_env(sbt_o, i), "augment" in self.fixes)
            self._sticky[i] = self._ctor_budget if "budget" in self.fixes else b
            cw[i], yi[i], cc[i], sm[i], bd[i] = w, y_i, li, ci, b
        self._reset_tuples(dict(county_w=cw, year_i=yi, coef_col=cc, sample=sm, budget=bd), mask_t, obs_ptr)

    def _device_cfg(self, seed, options):
        loc = options.get("location")
        if loc is None:
            loc_i = -1
        else:
            if loc not in self._fips_pos:
                raise ValueError(f"{loc!r} is not in list")
            loc_i = self._fips_pos[loc]
            if self.ct.fips_to_weather[loc_i] < 0:
                raise KeyError(loc)
        aug = bool(self._opt(options, "similar_climate_counties", self.similar_climate_counties))
        if aug and loc_i >= 0 and self.ct.sim_cnt[loc_i] <= 0:
            raise KeyError(loc)  # county absent from the confounders: confounders.loc[fips] (datautils.py:123)
        bk = self._ctor_budget if self._ctor_budget is not None else options.get("budget")
        mode = _ffi.BUDGET_FIXED
        if self._opt(options, "sample_budget", False):
            typ = self._opt(options, "sample_budget_type", "less_than")
            if typ not in _BUDGET_MODES:
                raise ValueError(f"sample_budget_type {typ!r}")
            mode = _BUDGET_MODES[typ]
        if seed is None:
            seed = int(np.random.randint(0, 2**31 - 1))
        return int(seed) & (2**64 - 1), loc_i, int(aug), -1 if bk is None else int(bk), mode, int("budget" not in self.fixes)

    def _reset_device(self, seed, options, mask_t, obs_ptr):
        ct = self.ct
        if (ct.fips_to_weather < 0).any() or (ct.n_days <= 0).any():
            raise KeyError("seed_mode='device' needs state tables for every fips_list county and year "
                           "(the reference raises KeyError at env.py:127 when it draws a missing pair)")
        cfg = self._device_cfg(seed, options)
        if cfg[2] and (ct.sim_cnt <= 0).any() and cfg[1] < 0:
            raise KeyError("a fips_list county is missing from the confounders table (datautils.py:123)")
        if self.episode_order == "sorted" and mask_t is not None:
            raise ValueError("episode_order='sorted' resets the whole batch; masks are not supported")
        self._reset_cfg = cfg
        # reset() re-seeds (explicit seed, or a fresh one for seed=None like env.py:143-145), so the per-env episode
        # counters restart: equal seeds give equal episodes. Autoresets advance the counters instead.
        self._launch_device_reset(mask_t, obs_ptr, restart=True)
        with torch.cuda.device(self.device):
            _ffi.check(self._lib.w2a_set_autoreset(self._h, *cfg), "w2a_set_autoreset")
        self._keep = (mask_t,)

    def _launch_device_reset(self, mask_t, obs_ptr, restart=False):
        """Device-RNG reset of the batch (restart: episode number 0 for a re-seeding reset(); else the next episode
        number per env, i.e. an autoreset); in sorted mode followed by the relabelling sort and the observation
        pass. Asynchronous, no host sync."""
        lib, st = self._lib, self._stream()
        srt = self.episode_order == "sorted"
        with torch.cuda.device(self.device):
            if srt and self.kernel.sorted_reset == "fused":
                # draw keys -> stable radix sort -> k_reset with "index e receives the episode env src[e] draws": the
                # relabelling without moving a record (1 = the key does not fit 32 bits: the three calls below)
                rc = lib.w2a_reset_device_rng_sorted(self._h, *self._reset_cfg, int(restart), obs_ptr, self._sort_ws.data_ptr(),
                                                     self._sort_ws.numel(), st)
                if rc not in (0, 1):
                    _ffi.check(rc, "w2a_reset_device_rng_sorted")
                srt = rc == 1
                done = rc == 0
            else:
                done = False
            if not done:
                _ffi.check(lib.w2a_reset_device_rng(self._h, *self._reset_cfg, int(restart), None if mask_t is None else
                                                    mask_t.data_ptr(), None if srt else obs_ptr, st),
                           "w2a_reset_device_rng")
            if srt and not done:
                _ffi.check(lib.w2a_sort_episodes(self._h, self._sort_ws.data_ptr(), self._sort_ws.numel(), st),
                           "w2a_sort_episodes")
                if obs_ptr is not None:
                    _ffi.check(lib.w2a_observe(self._h, obs_ptr, st), "w2a_observe")
        self._steps_in_episode = 0
        self._pending_reset = False
        if mask_t is None:
            self._obs_current = obs_ptr is not None
        self._regroup()

    def _regroup(self):
        """posterior_mean: env ids sorted by coefficient column for the grouped GEMM; after EVERY reset."""
        self._order_stale = True  # rollout(): the visiting order by feature row belongs to the previous episode
        if self._group_ws is not None:
            if max(int(self.ct.B0.max()), int(self._ctor_budget or 0), int(self._last_opts.get("budget") or 0)) > 65535:
                raise ValueError("reward_mode='posterior_mean' packs remaining_budget into 16 bits: budgets <= 65535")
            with torch.cuda.device(self.device):
                _ffi.check(self._lib.w2a_group_by_column(self._h, self._group_ws.data_ptr(), self._group_ws.numel(),
                                                         self._stream()), "w2a_group_by_column")
            if self.pm_kernel_choice is None:
                self._pick_pm_kernel()

    def _pick_pm_kernel(self, reps: int = 3):
        """pm_kernel="auto": time w2a_posterior_mean_reward with each kernel on this env's own grouped batch (HIP
        events on the launch stream, best of `reps`; the call only writes the reward buffer and its scratch) and keep
        the faster one. Runs once per env, right after the first grouping."""
        act = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        best = {}
        with torch.cuda.device(self.device):
            for name, code in _ffi.PM_KERNELS.items():
                _ffi.check(self._lib.w2a_set_posterior_kernel(self._h, code), "w2a_set_posterior_kernel")
                times = []
                for _ in range(reps + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    _ffi.check(self._lib.w2a_posterior_mean_reward(self._h, act.data_ptr(), _ffi.ACT_I32, self._rew_ptr,
                                                                   self._stream()), "w2a_posterior_mean_reward")
                    e1.record()
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1) * 1e3)
                best[name] = min(times[1:])
            self.pm_kernel_timing_us = best
            self.pm_kernel_choice = min(best, key=best.get)
            # The kernels differ in the last bits, and the device RNG's shard invariance (env_gid0) would be worth little
            # if the same global env id got other reward bits on another rank: with pm_sync_group= every rank of that
            # group takes the group's first rank's choice. A COLLECTIVE -- so only when the caller asked for it (every
            # rank of the group must then build such an env and reach its first reset()); without it "auto" is a
            # per-process choice (say pm_kernel=<name> for a fixed one).
            if self.pm_sync_group is not None:
                import torch.distributed as td

                names = list(_ffi.PM_KERNELS)
                pick = torch.tensor([names.index(self.pm_kernel_choice)], dtype=torch.int32, device=self.device)
                group = None if self.pm_sync_group is True else self.pm_sync_group
                td.broadcast(pick, src=td.get_global_rank(group, 0) if group is not None else 0, group=group)
                self.pm_kernel_choice = names[int(pick.item())]
            _ffi.check(self._lib.w2a_set_posterior_kernel(self._h, _ffi.PM_KERNELS[self.pm_kernel_choice]),
                       "w2a_set_posterior_kernel")
            self.check_status()  # zero actions on a fresh episode raise no status bit; clear what a mid-episode call may

    # ------------------------------------------------------------------ step
    def step(self, actions):
        """Gymnasium VectorEnv.step: (obs, reward, terminated, truncated, info), all device
        tensors that are reused by the next call (clone them to keep a copy)."""
        if self._needs_reset:
            raise RuntimeError("call reset() before step()")
        if (type(actions) is not torch.Tensor or actions.device != self.device or actions.dtype not in _ACT_CODES
                or actions.numel() != self.num_envs or not actions.is_contiguous()):
            actions = self._coerce_actions(actions)
        if _cur_device() != self._dev_index:  # kernels launch on the current device: it must be this env's
            with torch.cuda.device(self.device):
                return self.step(actions)
        if self._pending_reset:
            # autoreset="next_step" in lock step: the previous call was the terminal step of every env, so this call is
            # their restart -- actions ignored, first observations of the next episodes, reward 0, nobody done
            self._launch_device_reset(None, self._obs_ptr)
            self._reward.zero_()
            self._done.zero_()
            self._keep_act = actions
            return self._obs, self._reward, self._done_bool, self._truncated, _LazyInfo(self)
        if self._pm:  # today's reward of every env as the mean over all posterior draws, from the pre-step state
            rc = self._lib.w2a_posterior_mean_reward(self._h, actions.data_ptr(), _ACT_CODES[actions.dtype],
                                                     self._rew_ptr, self._stream())
            if rc != 0:
                _ffi.check(rc, "w2a_posterior_mean_reward")
        rc = self._w2a_step(self._h, actions.data_ptr(), _ACT_CODES[actions.dtype], self._obs_ptr, self._rew_ptr,
                            self._done_ptr, self._fr_ptr, self._step_flags, self._stream())
        if rc != 0:
            _ffi.check(rc, "w2a_step")
        self._keep_act = actions
        self._obs_current = self.write_obs
        done = self._done_bool
        if self._host_auto:  # lock step: the host counts days and launches the reset after the terminal step
            self._steps_in_episode += 1
            if self._steps_in_episode == self._episode_len:
                self._launch_device_reset(None, self._obs_ptr)
        elif self._host_next:  # ... or leaves it to the next call
            self._steps_in_episode += 1
            if self._steps_in_episode == self._episode_len:
                self._pending_reset = True
        elif self.autoreset == "same_step" and not self._dev_auto:
            d = done.cpu().numpy()
            if d.any():  # host-side autoreset (numpy_parity): fresh global-RNG seeds like reset(seed=None)
                self._reset_numpy_parity(None, self._last_opts, d, torch.as_tensor(d.astype(np.uint8),
                                         device=self.device), self._obs_ptr)
        return self._obs, self._reward, done, self._truncated, _LazyInfo(self)

    def record_steps(self, one_day, days: int, warmup: bool = True):
        """Record `days` calls of one_day() -- a policy on device tensors + self.step(actions) -- into a hipGraph and
        return a weather2alert_amd.graph.RecordedSteps: .replay() launches the block and reads the device status word
        BEHIND every replay (asynchronously: replay k checks what replay k-1 left), so a block that could not run -- the
        mirror of a packed lock-step batch marked stale by a masked reset or a restored checkpoint, W2A_ST_STALE_GRAPH --
        or bad actions raise at the next replay instead of training on frozen observations."""
        from .graph import RecordedSteps

        return RecordedSteps(self, one_day, days, warmup)

    # ------------------------------------------------------------------ rollout
    def rollout(self, policy: dict, n_steps: int | None = None, alert_mask: bool = False, record: bool = False,
                posterior_returns: bool = False, hindsight: bool = False,
                policy_gradient: bool | str = False) -> dict:
        """Run a built-in policy inside the kernel for ``n_steps`` days (default: to the end of the episode)
        without returning to Python between days (replaces loops like env.py:265-277). With
        reward_mode="posterior_mean" the whole rollout is one launch of k_pm_rollout (vector kernel, <= 112 posterior
        draws, reference schema); otherwise a host loop of policy kernel + reward kernels + step kernel per day (same
        policies, same outputs): the legacy eval mode's evaluation sweep.

        policy: {"kind": "never" | "always"} |
                {"kind": "bernoulli", "p": 0.1, "seed": 0} |
                {"kind": "threshold", "feature": "heat_qi", "threshold": 0.9, "lag": 1} |
                {"kind": "table", "table": uint8 [T, R]}   (action = table[day][min(remaining_budget, R-1)]) |
                {"kind": "linear", "weight": f32 [G, n_obs], "bias": f32 [G], "group": int [num_envs] (may be
                 omitted when G == 1), "sample": False, "seed": 0}   (weather2alert_amd/policy.py) |
                {"kind": "mlp", "layers": [(W1, b1), [(W2, b2),] (Wo, bo)] (torch Linear convention, optionally with
                 a leading G dim), "activation": "tanh" | "relu", "group", "order", "sample", "seed"}
                plus optional "require_budget": True (never attempt an alert with no budget left), and for the linear
                and mlp kinds optional "allowed_days": bool [num_envs, T] by day of the episode (alert_gate(), or any
                other mask; or the packed int32 [num_envs, ceil(T / 32)] of alert_gate(packed=True)): on a day whose bit is clear the attempted action is 0 -- before the attempt is recorded and
                before the budget test, so it never counts as an over-budget attempt -- and the day is a forced choice:
                no score under policy_gradient (m_s = 0, as for require_budget), a recorded "action" of 0 next to the
                policy's own "logit", and under hindsight=True the optimum is the best schedule on allowed days. The
                uniform u of a day does not depend on the gate. ValueError for a wrong dtype or shape and for a kind
                that takes no gate. An all-ones mask gives the bits of the call without the key.
        The linear policy acts on logit = weight[g] . obs + bias[g] (fp64 over the f32 values) for the env's group g,
        where obs is exactly the row step() would have returned before that decision -- so rollout(linear, k) is
        indistinguishable from k iterations of `a = policy(obs); obs = env.step(a)`, observation buffer included.
        sample=False alerts iff logit > 0, sample=True iff u < sigmoid(logit) with the bernoulli policy's uniform u.
        It reads the observation buffer on its first day and writes the final rows back (k_rollout_linear), so it needs
        that buffer current: after reset(), step() or a linear rollout with write_obs=True -- not after a built-in
        rollout that did not end in a whole-batch reset, nor after load_state_dict (RuntimeError). Faithful semantics
        only (fixes other than "budget" change what the observation is) and reward_mode="sampled" (ValueError). Its
        result also holds "group_mean_return" f32 [G]: the mean "return" of each group's envs.
        The mlp policy is the same with an f32 network of 1-2 hidden layers (width <= 64) in place of the linear logit
        (k_rollout_mlp, f32 matrix cores; a two-row output is SB3's two action values, logit = row1 - row0); its
        decisions can differ from an fp64 evaluation only at near-ties (include/w2a.h). policy.mlp_from_module turns a
        torch Sequential into such a dict.
        The threshold policy sees the lagging observation the reference's agent would see (Q6; lag=0 reads
        today's row instead). Returns device tensors: "return" (rewards summed over the days run), "alerts",
        "attempts_over_budget", "final_return" (episode return of envs that finished), "done", and with
        alert_mask=True "alert_days" bool [N, T]. In lock-step same_step-autoreset mode a finished batch is
        reset, so consecutive calls evaluate consecutive episodes.
        record=True (linear and mlp kinds only; ValueError otherwise) also returns the per-day trajectory for
        on-policy training, "trajectory": a dict of device tensors indexed [call-day s, env id] (S = the days the call
        was asked to run, N = num_envs), written by the same kernel launch (w2a_rollout_*_record, include/w2a.h):
          "obs"        f32 [S+1, N, n_obs]  obs[s]: the row the agent held before decision s (what step() returned);
                                            obs[S]: the observation buffer as the call leaves it, before any lock-step
                                            autoreset it triggers -- the bootstrap row of a truncated chunk
          "action"     u8   [S, N]  the action passed to the env (after require_budget)
          "logit"      f32  [S, N]  the logit of that decision (linear: the fp64 logit rounded to f32)
          "reward"     f32  [S, N]  the reward step() returns for that day
          "valid"      bool [S, N]  the env took a step on call-day s
          "terminated" bool [S, N]  that step ended its episode
          "alert"      bool [S, N]  the alert actually issued
        Entries where valid is False are unspecified, except that valid, terminated and alert are False there.
        Recording changes nothing else the call returns or leaves behind, bit for bit; two calls of k and S - k days
        record what one call of S days does. policy.action_log_prob(logit, action) gives the log-probability of a
        recorded action. The tensors are allocated per call (torch's caching allocator): 4 n_obs + 10 bytes per
        env-day plus one obs slab -- 126 B on the default schema, about 20 GB for 1 M envs x 153 days.
        posterior_returns=True (every kind, with or without record, both reward modes) also returns
        "posterior_returns" f32 [N, n_samples]: each env's return over the days this call ran under EVERY posterior draw
        of its coefficient column (w2a_posterior_returns, include/w2a.h: the trajectory does not depend on the draw, so
        the call's alert bitmap and start state fix every day's input). Column "sample" of an env is its own draw: bit
        for bit "return" for the fp64-chain rollout kernels, within 2e-6 relative for k_rollout_mfma. The linear and mlp
        kinds also return "group_posterior_returns" f32 [G, n_samples], the mean over each group's envs per draw (one
        posterior sample of the group's value per column; stats.posterior_summary, stats.prob_better). Nothing else the
        call returns or leaves behind changes. Faithful semantics only (fixes other than "budget": ValueError).
        hindsight=True (every kind, combinable with record and posterior_returns) also returns "hindsight_return" f32
        [N]: the return of each env's best alert schedule over the same days from the same start state
        (hindsight_optimum(), the yardstick that turns "return" into regret); the linear and mlp kinds also return
        "group_hindsight_return" f32 [G]. Nothing else the call returns or leaves behind changes. Sampled reward and
        faithful semantics only (ValueError otherwise, and for tables with a nonzero slot-27 coefficient).
        policy_gradient="none" | "no_alert" | True (= "no_alert"); kind="linear" or "mlp" with sample=True only -- ValueError for
        sample=False, every other kind, reward_mode="posterior_mean", fixes other than "budget", an unknown string, and
        together with record=True (a recorded trajectory already holds everything a learner needs); combinable with
        alert_mask, posterior_returns and hindsight. Also returns "policy_gradient": {"weight": f32 [G, n_obs] (columns
        in observation order, like policy["weight"]), "bias": f32 [G]}, the reward-to-go score-function (REINFORCE)
        estimate of the gradient of each group's mean "return", so ``W += lr * out["policy_gradient"]["weight"]`` is an
        ascent step (NaN rows for a group without envs). Per env e, over the call-days s on which it took a step:
          g_e = sum_s delta_s Q_s (o_s, 1),   delta_s = m_s (a_s - sigmoid(z_s)),   Q_s = sum_{s' >= s} (r_s' - beta_s')
        with o_s the row held before decision s, z_s its fp64 logit, a_s the policy's own draw, m_s = 0 on a day where
        require_budget forced the action to 0 with no budget left (off the policy's distribution; without require_budget
        an attempt at the budget counts), r_s the day's reward; beta_s = 0 ("none") or ("no_alert") the reward the same
        env would have been paid that day had no alert been issued from the call's first day on, from the call's start
        state (alert_lag1 0, the start streak on the first day then 0, the 14-day window decaying, the budget frozen):
        independent of everything the policy does in the call, so a valid baseline for every earlier score, and it
        removes the large action-independent part of the reward. Undiscounted; Q_s stops at the call's last day -- a
        chunk shorter than the episode is truncated, nothing is bootstrapped. The group's gradient is the mean of g_e
        over its envs; envs finished on entry contribute zero and count. w2a_policy_gradient_linear (include/w2a.h)
        runs right before the rollout on the same state and rows, with the rollout's own statements for u, z_s and
        r_s; no observation row goes to memory per day (9 B of scratch per env-day). Deterministic: two identical calls
        return bit-identical gradients. Nothing else the call returns or leaves behind changes, bit for bit.
        For kind="mlp" the same estimator with z_s the f32 logit k_rollout_mlp acts on and (o_s, 1) replaced by
        dz_s/dtheta, the backward pass of the f32 network (ReLU' = 0 at a pre-activation of exactly 0):
        "policy_gradient": {"layers": [(dW, db), ...]} in the shapes and torch Linear convention of policy["layers"]
        with a leading G ([G, out, in] / [G, out], f32; for a two-row output row 1 gets +g and row 0 -g, the adjoint of
        logit = row1 - row0). w2a_policy_gradient_mlp: the forward pass is recomputed and backpropagated on the matrix
        cores inside the kernel, the parameter gradients are summed over envs in registers and reduced per group in
        fp64 in a fixed order (no atomics; a few tens of MB of partial blocks at 1 M envs). policy.mlp_grad_to_module
        writes a group's gradient into the .grad of the torch module the policy came from."""
        pg = _policy.check_policy_gradient(policy_gradient, policy.get("kind"), policy.get("sample", False),
                                           self.reward_mode, self.fixes, record, kinds=("linear", "mlp"))
        if self._needs_reset:
            raise RuntimeError("call reset() before rollout()")
        ct = self.ct
        kind = policy.get("kind")
        lin = None
        gate = _policy.check_allowed_days(policy, self.num_envs, ct.T, self.device, "rollout()")
        if record and kind not in ("linear", "mlp"):
            raise ValueError(f"rollout(record=True) needs kind 'linear' or 'mlp', got {kind!r}")
        if posterior_returns and self.fixes - {"budget"}:
            raise ValueError(f"rollout(posterior_returns=True) needs faithful semantics; fixes "
                             f"{sorted(self.fixes - {'budget'})} make the reward depend on attempts and other rows")
        if hindsight:
            self._check_hindsight("rollout(hindsight=True)")
        if kind in ("linear", "mlp"):  # every argument is checked before anything runs
            if self._pm:
                raise ValueError(f"rollout(kind={kind!r}) needs reward_mode='sampled'")
            if self.fixes - {"budget"}:
                raise ValueError(f"rollout(kind={kind!r}) needs faithful observations; fixes {sorted(self.fixes - {'budget'})} "
                                 "change what the observation is")
            if policy.get("lookahead") is not None:
                if record:
                    raise ValueError("rollout(record=True) does not take a 'lookahead' policy: the recorded rows would "
                                     "lack the lookahead inputs (a later addition)")
                if pg is not None and kind == "mlp":
                    raise ValueError("rollout(policy_gradient=...) takes 'lookahead' with kind 'linear' only; the mlp "
                                     "kind's gradient kernels do not read the lookahead inputs yet")
            lin = _check_learned(self, policy)
        elif kind not in _ffi.POLICY_KINDS:
            raise ValueError(f"policy kind {kind!r}")
        if self._pending_reset:  # next_step autoreset in lock step: the finished batch restarts before anything runs
            self._launch_device_reset(None, self._obs_ptr)
        if lin is not None and not self._obs_current:
            raise RuntimeError(f"rollout(kind={kind!r}) reads the observation buffer, which does not hold the agents' "
                               "current rows (write_obs=False, a built-in rollout or load_state_dict since the last "
                               "step()/reset()): call step() or reset() first")
        pr, hs = bool(posterior_returns), bool(hindsight)
        if kind == "mlp":
            return self._rollout_mlp(lin, n_steps, alert_mask, bool(record), pr, hs, pg, gate)
        if lin is not None:
            return self._rollout_linear(lin, n_steps, alert_mask, bool(record), pr, hs, pg, gate)
        p = _ffi.Policy()
        p.kind = _ffi.POLICY_KINDS[kind]
        p.p = float(policy.get("p", 0.0))
        p.require_budget = int(bool(policy.get("require_budget", False)))
        p.seed = int(policy.get("seed", 0)) & (2**64 - 1)
        p.obs_lag = int(policy.get("lag", 1))
        keep = None
        if kind == "threshold":
            feat = policy["feature"]
            if feat not in ct.feature_names:
                raise KeyError(feat)
            p.obs_col, p.threshold = ct.feature_names.index(feat), float(policy["threshold"])
        if kind == "table":
            keep = torch.as_tensor(policy["table"], device=self.device).to(torch.uint8).contiguous()
            if keep.dim() != 2 or keep.shape[0] < ct.T:
                raise ValueError(f"policy table must be [T >= {ct.T}, R]")
            p.table, p.table_R = keep.data_ptr(), int(keep.shape[1])
        return self._rollout_run(p, None, n_steps, alert_mask, keep, posterior_returns=pr, hindsight=hs)

    def lookahead_table(self, feature: str = "heat_qi") -> torch.Tensor:
        """f32 [S_w * Y, T] on the device: the value of the table-sourced observation column `feature` on every day of
        every (county, year) episode -- that column of the feature table X, transposed so that one episode's days are
        contiguous (a lookahead decision reads D + 1 consecutive floats of one series). Built once per feature and
        kept on the env until close(); it does not depend on the env's state. ValueError, as every other lookahead
        check, for a name that is no observation column and for a column that is not table-sourced (the rule of
        alert_gate())."""
        ct = self.ct
        cache = self._look_tables
        if feature in cache:
            return cache[feature]
        if feature not in ct.feature_names:
            raise ValueError(f"lookahead_table(feature={feature!r}): no observation column of that name")
        slot = int(_policy.slot_map(ct.obs_slot, ct.n_obs)[ct.feature_names.index(feature)])
        if 24 <= slot <= 27 or ("alert_2wks" in self.fixes and slot == ct.slot_of.get("alerts_2wks", -1)):
            raise ValueError(f"lookahead_table(feature={feature!r}): lookahead reads table-sourced columns only")
        cache[feature] = self.dtables.X[:, :, slot].t().contiguous()  # [T, R] -> [R, T]
        return cache[feature]

    def lookahead_features(self, spec: dict) -> torch.Tensor:
        """f32 [N, D]: the lookahead inputs of the rows the envs hold right now, for ``spec = {"feature": name,
        "days": D}`` (a policy's "lookahead" value): f_k = h(r + k) - h(r), k = 1..D, with h the series of
        lookahead_table(feature) for the env's (county, year), r = max(t - 1, 0) the day of the row step() returned last
        (Q6), and 0 where r + k >= n_days of the env. What the kernels of a lookahead policy form themselves: a torch
        policy driven through step() acts on ``cat(obs, env.lookahead_features(spec))``. A spec with ``"error"``
        (policy.check_lookahead) gives the noisy inputs, formed by the device function the rollout kernels use
        (w2a_forecast_features): the same values whenever and however often it is asked."""
        if self._needs_reset:
            raise RuntimeError("call reset() before lookahead_features()")
        feature, D = _policy.check_lookahead({"lookahead": spec}, "lookahead_features()", self.ct.feature_names,
                                             self.ct.obs_slot, self.ct.n_obs, self.fixes,
                                             self.ct.slot_of.get("alerts_2wks", -1))
        tab = self.lookahead_table(feature)
        fe = _policy.check_forecast_error({"lookahead": spec}, "lookahead_features()")
        if fe is not None:
            pol = types.SimpleNamespace(look_feature=feature, look_days=D, look_error=fe[0], look_error_seed=fe[1])
            look, ferr = self._lookahead_struct(pol), self._forecast_error_struct(pol)
            out = torch.empty((self.num_envs, D), dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                _ffi.check(self._lib.w2a_forecast_features(self._h, C.byref(look), C.byref(ferr), out.data_ptr(),
                                                           self._stream()), "w2a_forecast_features")
            return out
        st = self._state_packed(("t", "n_days", "county_w", "year_i"))[1]
        row = (st["county_w"].long() * self.ct.Y + st["year_i"].long())[:, None]
        r = (st["t"].long() - 1).clamp_(min=0)[:, None]
        d = r + torch.arange(1, D + 1, device=self.device)[None, :]
        ok = d < st["n_days"].long()[:, None]
        h = tab[row, torch.where(ok, d, r)]
        return torch.where(ok, h - tab[row, r], torch.zeros((), dtype=torch.float32, device=self.device))

    def _lookahead_struct(self, pol):
        """The w2a_lookahead block of a checked lookahead policy (linear: with its weight rows), and what it points to."""
        tab = self.lookahead_table(pol.look_feature)
        lk = _ffi.Lookahead()
        lk.series, lk.stride, lk.days = tab.data_ptr(), int(tab.shape[1]), pol.look_days
        lk.weight = pol.look_weight.data_ptr() if getattr(pol, "look_weight", None) is not None else None
        return lk

    @staticmethod
    def _forecast_error_struct(pol):
        """The w2a_forecast_error block of a checked lookahead policy with "error", None without the key."""
        if getattr(pol, "look_error", None) is None:
            return None
        fe = _ffi.ForecastError()
        for k, v in enumerate(pol.look_error):
            fe.mae[k] = v
        fe.seed = pol.look_error_seed
        return fe

    def _rollout_linear(self, lin, n_steps, alert_mask, record=False, posterior_returns=False, hindsight=False,
                        policy_gradient=None, gate=None) -> dict:
        """rollout(kind="linear"): w2a_rollout_linear on the checked policy (weather2alert_amd/policy.py)."""
        lp = _ffi.LinearPolicy()
        lp.weight, lp.bias = lin.weight_slots.data_ptr(), lin.bias.data_ptr()
        lp.group = None if lin.group is None else lin.group.data_ptr()
        lp.n_groups, lp.sample, lp.require_budget, lp.seed = lin.n_groups, int(lin.sample), int(lin.require_budget), lin.seed
        out = self._rollout_run(None, lp, n_steps, alert_mask, lin, record, posterior_returns, hindsight, policy_gradient,
                                gate)
        out["group_mean_return"] = _policy.group_mean(out["return"], lin.group, lin.n_groups)
        if posterior_returns:
            out["group_posterior_returns"] = _policy.group_mean(out["posterior_returns"], lin.group, lin.n_groups)
        if hindsight:
            out["group_hindsight_return"] = _policy.group_mean(out["hindsight_return"], lin.group, lin.n_groups)
        if policy_gradient is not None:
            # per-env gradients -> per-group mean, in a fixed order (a sort and an fp64 scan along each column)
            g = _policy.group_mean_columns(out.pop("_policy_gradient_env"), lin.group, lin.n_groups)
            no = self.ct.n_obs  # rows: the observation columns, the bias, then the lookahead inputs
            out["policy_gradient"] = {"weight": torch.cat([g[:, :no], g[:, no + 1:]], dim=1).contiguous(),
                                      "bias": g[:, no].contiguous()}
        return out

    def _rollout_mlp(self, mlp, n_steps, alert_mask, record=False, posterior_returns=False, hindsight=False,
                     policy_gradient=None, gate=None) -> dict:
        """rollout(kind="mlp"): w2a_rollout_mlp on the checked, packed policy (weather2alert_amd/policy.py)."""
        mp = _ffi.MlpPolicy()
        mp.params = mlp.params.data_ptr()
        mp.group = None if mlp.group is None else mlp.group.data_ptr()
        mp.order = None if mlp.order is None else mlp.order.data_ptr()
        mp.n_groups, mp.n_layers, mp.width = mlp.n_groups, mlp.n_layers, mlp.width
        mp.activation = _ffi.MLP_ACTIVATIONS[mlp.activation]
        mp.sample, mp.require_budget, mp.seed = int(mlp.sample), int(mlp.require_budget), mlp.seed
        out = self._rollout_run(None, mp, n_steps, alert_mask, mlp, record, posterior_returns, hindsight, policy_gradient,
                                gate)
        if policy_gradient is not None:
            out["policy_gradient"] = {"layers": _policy.unpack_mlp_grad(
                out.pop("_policy_gradient_blocks"), self.ct.obs_slot, self.ct.n_obs, mlp.hidden, mlp.n_out)}
        out["group_mean_return"] = _policy.group_mean(out["return"], mlp.group, mlp.n_groups)
        if posterior_returns:
            out["group_posterior_returns"] = _policy.group_mean(out["posterior_returns"], mlp.group, mlp.n_groups)
        if hindsight:
            out["group_hindsight_return"] = _policy.group_mean(out["hindsight_return"], mlp.group, mlp.n_groups)
        return out

    def _rollout_run(self, p, lp, n_steps, alert_mask, keep, record=False, posterior_returns=False,
                     hindsight=False, policy_gradient=None, gate=None) -> dict:
        """The launch and the outputs shared by every policy kind: built-in (p, w2a_rollout / the posterior-mean path) or
        linear / mlp (lp, w2a_rollout_linear / w2a_rollout_mlp, or their *_record forms with record=True).
        posterior_returns: the alert bitmap is taken in any case (the rollout kernels' results do not depend on it) and
        w2a_posterior_returns runs on it and the start state right after the rollout. hindsight: w2a_hindsight_optimum on
        the same start state and days. policy_gradient ("none" / "no_alert"): w2a_policy_gradient_linear /
        w2a_policy_gradient_mlp right before the rollout, on the state and the rows the rollout starts from; the linear
        kind's per-env rows come back as "_policy_gradient_env" f32 [n_obs + 1, N], the mlp kind's per-group blocks as
        "_policy_gradient_blocks" f32 [G, stride] (the layout of the packed parameters). gate: the packed
        "allowed_days" of a linear or mlp policy (int32 [N, words]); the gradient, the rollout and the hindsight optimum then
        take their *_gated entry points."""
        ct = self.ct
        n, dev = self.num_envs, self.device
        steps = int(n_steps) if n_steps is not None else ct.T
        # a lookahead policy (rollout() has refused record=True): the w2a_lookahead_* entry points
        look = self._lookahead_struct(keep) if getattr(keep, "look_days", 0) else None
        ferr = self._forecast_error_struct(keep)  # with "error": the w2a_forecast_* entry points
        out = {"return": torch.empty(n, dtype=torch.float32, device=dev),
               "alerts": torch.empty(n, dtype=torch.int32, device=dev),
               "attempts_over_budget": torch.empty(n, dtype=torch.int32, device=dev)}
        words = (ct.T + 31) // 32
        mask = torch.empty((n, words), dtype=torch.int32, device=dev) if (alert_mask or posterior_returns) else None
        amask = torch.empty((n, words), dtype=torch.int32, device=dev) if alert_mask else None
        snap = torch.full((n,), float("nan"), dtype=torch.float32, device=dev) if alert_mask else None
        st0 = self.state() if (alert_mask or self._pm or posterior_returns or hindsight) else None
        traj = tr = None
        if record:  # lp is not None: rollout() refuses record=True for the other kinds
            traj = {"obs": torch.empty((steps + 1, n, ct.n_obs), dtype=torch.float32, device=dev),
                    "logit": torch.empty((steps, n), dtype=torch.float32, device=dev),
                    "reward": torch.empty((steps, n), dtype=torch.float32, device=dev),
                    "action": torch.empty((steps, n), dtype=torch.uint8, device=dev),
                    "flags": torch.empty((steps, n), dtype=torch.uint8, device=dev)}  # zeroed by the library
            tr = _ffi.Trajectory(*(traj[k].data_ptr() for k in ("obs", "logit", "reward", "action", "flags")))
        with torch.cuda.device(dev):
            if not self._pm and getattr(self, "_order_stale", True) and self.rollout_order:
                if self._order_ws is None:
                    # attached from here on: every later whole-batch reset leaves the feature-row counts and per-env ranks
                    # in it (the first pass of the counting sort, inside k_reset), w2a_rollout_order only scans and places
                    self._order_ws = torch.empty(self._lib.w2a_rollout_order_workspace_bytes(n, ct.S_w * ct.Y), dtype=torch.uint8, device=dev)
                    _ffi.check(self._lib.w2a_rollout_order_attach(self._h, self._order_ws.data_ptr(), self._order_ws.numel()),
                               "w2a_rollout_order_attach")
                _ffi.check(self._lib.w2a_rollout_order(self._h, self._order_ws.data_ptr(), self._order_ws.numel(),
                                                       self._stream()), "w2a_rollout_order")
                self._order_stale = False
                if self.rollout_mfma and not (self.fixes - {"budget"}):
                    if self._mfma_ws is None:
                        self._mfma_ws = torch.empty(self._lib.w2a_rollout_mfma_workspace_bytes(
                            n, ct.S_w * ct.Y, ct.S, ct.n_samples), dtype=torch.uint8, device=dev)
                    _ffi.check(self._lib.w2a_rollout_mfma_prepare(self._h, self._mfma_ws.data_ptr(), self._mfma_ws.numel(),
                                                                  self._stream()), "w2a_rollout_mfma_prepare")
            if policy_gradient is not None and isinstance(lp, _ffi.MlpPolicy):
                # the gradient kernels write no state, so their visiting order is their own: always group-major (the
                # partial blocks of w2a_policy_gradient_mlp are sized for it), whatever "order" the rollout itself uses
                gp = _ffi.MlpPolicy.from_buffer_copy(lp)
                gorder = None if keep.group is None else (keep.order if keep.group_major else _policy.group_order(keep.group))
                gp.order = None if gorder is None else gorder.data_ptr()
                out["_policy_gradient_blocks"] = torch.empty(
                    (keep.n_groups, _policy.mlp_stride(keep.width, keep.n_layers)), dtype=torch.float32, device=dev)
                ws = torch.empty(self._lib.w2a_policy_gradient_mlp_workspace_bytes(
                    n, steps, keep.n_groups, keep.width, keep.n_layers), dtype=torch.uint8, device=dev)
                pgm_args = (self._h, C.byref(gp), _ffi.PG_BASELINES[policy_gradient], steps, self._obs.data_ptr(),
                            out["_policy_gradient_blocks"].data_ptr(), ws.data_ptr(), ws.numel(), self._stream())
                if gate is None:
                    _ffi.check(self._lib.w2a_policy_gradient_mlp(*pgm_args), "w2a_policy_gradient_mlp")
                else:
                    _ffi.check(self._lib.w2a_policy_gradient_mlp_gated(*pgm_args, gate.data_ptr(), int(gate.shape[1])),
                               "w2a_policy_gradient_mlp_gated")
            elif policy_gradient is not None:
                out["_policy_gradient_env"] = torch.empty((ct.n_obs + 1 + keep.look_days, n), dtype=torch.float32,
                                                          device=dev)
                ws = torch.empty(self._lib.w2a_policy_gradient_workspace_bytes(n, steps), dtype=torch.uint8, device=dev)
                pg_args = (self._h, C.byref(lp), _ffi.PG_BASELINES[policy_gradient], steps, self._obs.data_ptr(),
                           out["_policy_gradient_env"].data_ptr(), ws.data_ptr(), ws.numel(), self._stream())
                if look is not None:
                    fn = "w2a_lookahead_policy_gradient_linear" if ferr is None else "w2a_forecast_policy_gradient_linear"
                    _ffi.check(getattr(self._lib, fn)(
                        *pg_args, C.byref(look), None if gate is None else gate.data_ptr(),
                        0 if gate is None else int(gate.shape[1]), *(() if ferr is None else (C.byref(ferr),))), fn)
                elif gate is None:
                    _ffi.check(self._lib.w2a_policy_gradient_linear(*pg_args), "w2a_policy_gradient_linear")
                else:
                    _ffi.check(self._lib.w2a_policy_gradient_linear_gated(*pg_args, gate.data_ptr(), int(gate.shape[1])),
                               "w2a_policy_gradient_linear_gated")
            if ferr is not None:
                fn = "w2a_forecast_rollout_mlp" if isinstance(lp, _ffi.MlpPolicy) else "w2a_forecast_rollout_linear"
                _ffi.check(getattr(self._lib, fn)(
                    self._h, C.byref(lp), steps, self._obs.data_ptr(), out["return"].data_ptr(),
                    out["alerts"].data_ptr(), out["attempts_over_budget"].data_ptr(),
                    None if mask is None else mask.data_ptr(), None if amask is None else amask.data_ptr(), words,
                    self._fr_ptr, None if snap is None else snap.data_ptr(), self._stream(), C.byref(look),
                    None if gate is None else gate.data_ptr(), 0 if gate is None else int(gate.shape[1]),
                    C.byref(ferr)), fn)
            elif look is not None:
                fn = "w2a_lookahead_rollout_mlp" if isinstance(lp, _ffi.MlpPolicy) else "w2a_lookahead_rollout_linear"
                args = (self._h, C.byref(lp), steps, self._obs.data_ptr(), out["return"].data_ptr(),
                        out["alerts"].data_ptr(), out["attempts_over_budget"].data_ptr(),
                        None if mask is None else mask.data_ptr(), None if amask is None else amask.data_ptr(), words,
                        self._fr_ptr, None if snap is None else snap.data_ptr(), self._stream(), C.byref(look))
                if gate is not None:
                    fn += "_gated"
                    args += (gate.data_ptr(), int(gate.shape[1]))
                _ffi.check(getattr(self._lib, fn)(*args), fn)
            elif lp is not None and gate is not None:
                fn = "w2a_rollout_mlp_gated" if isinstance(lp, _ffi.MlpPolicy) else "w2a_rollout_linear_gated"
                _ffi.check(getattr(self._lib, fn)(
                    self._h, C.byref(lp), steps, self._obs.data_ptr(), out["return"].data_ptr(),
                    out["alerts"].data_ptr(), out["attempts_over_budget"].data_ptr(),
                    None if mask is None else mask.data_ptr(), None if amask is None else amask.data_ptr(), words,
                    self._fr_ptr, None if snap is None else snap.data_ptr(), self._stream(),
                    None if tr is None else C.byref(tr), gate.data_ptr(), int(gate.shape[1])), fn)
            elif lp is not None:
                fn = "w2a_rollout_mlp" if isinstance(lp, _ffi.MlpPolicy) else "w2a_rollout_linear"
                args = (self._h, C.byref(lp), steps, self._obs.data_ptr(), out["return"].data_ptr(),
                        out["alerts"].data_ptr(), out["attempts_over_budget"].data_ptr(),
                        None if mask is None else mask.data_ptr(), None if amask is None else amask.data_ptr(), words,
                        self._fr_ptr, None if snap is None else snap.data_ptr(), self._stream())
                if tr is not None:
                    fn += "_record"
                    args += (C.byref(tr),)
                _ffi.check(getattr(self._lib, fn)(*args), fn)
            elif self._pm:
                steps = self._rollout_posterior_mean(p, steps, out, mask, amask, words, snap, st0)
            else:
                _ffi.check(self._lib.w2a_rollout(self._h, C.byref(p), steps, out["return"].data_ptr(),
                                                 out["alerts"].data_ptr(), out["attempts_over_budget"].data_ptr(),
                                                 None if mask is None else mask.data_ptr(),
                                                 None if amask is None else amask.data_ptr(), words, self._fr_ptr,
                                                 None if snap is None else snap.data_ptr(), self._stream()), "w2a_rollout")
            if posterior_returns:
                out["posterior_returns"] = self._posterior_returns_packed(st0, mask, words, steps)
            if hindsight:
                out["hindsight_return"] = self._hindsight_packed(st0, steps, gate)[0]
        self._keep_pol = (keep, gate)
        self._obs_current = lp is not None  # built-in policies write no observation rows (a reset below may)
        # only what this call returns is decoded (sixteen arrays of N int32 otherwise: 64 MB of writes at 1 M envs)
        st = self.state() if alert_mask else self._state_packed(("finished",))[1]
        out["done"] = st["finished"].bool()  # the terminal step has run (t stops at n_days-1 before AND after it)
        out["final_return"] = self._final_return.clone()  # meaningful where out["done"]
        if traj is not None:
            flags = traj.pop("flags")
            traj["valid"] = (flags & _ffi.TRAJ_VALID) != 0
            traj["terminated"] = (flags & _ffi.TRAJ_TERMINATED) != 0
            traj["alert"] = (flags & _ffi.TRAJ_ALERT) != 0
            out["trajectory"] = traj
        if alert_mask:
            bits = torch.arange(32, device=dev, dtype=torch.int32)
            unpack = lambda m: (((m.unsqueeze(-1) >> bits) & 1).reshape(n, words * 32)[:, : ct.T]).bool()  # noqa: E731
            out["alert_days"] = unpack(mask)      # the reference's actual_alert_buffer (env.py:248), per day
            out["attempt_days"] = unpack(amask)   # its attempted_alert_buffer (env.py:239)
            out["return_snapshot"] = snap         # running return when the callbacks read the env (t == n_days - 2)
            out["n_days"], out["budget"] = st["n_days"], st["budget"]
            out["first_day"] = st0["t"]           # day index this call started from (0 for whole episodes)
            out["year"] = torch.as_tensor(ct.years, dtype=torch.int32, device=dev)[st["year_i"].long()]
        if self._host_auto or self._host_next:
            self._steps_in_episode = min(self._steps_in_episode + steps, self._episode_len)
            if self._steps_in_episode >= self._episode_len:
                if self._host_auto:
                    self._launch_device_reset(None, self._obs_ptr)
                else:
                    self._pending_reset = True
        return out

    # ------------------------------------------------------------------ returns under every posterior draw
    def posterior_returns(self, start_state: dict, alert_days, n_steps: int | None = None) -> torch.Tensor:
        """f32 [N, n_samples]: each env's return over a stretch of days under every posterior draw of its coefficient
        column -- what rollout(..., posterior_returns=True) returns, for any way the days were run (a torch policy
        driven through step(), say). start_state: a state() dict taken before the stretch; alert_days: bool [N, T], the
        alerts issued (day d of the episode; rollout(alert_mask=True)'s "alert_days", or built from the actions and the
        budget); n_steps: the stretch's length in days (default: to the end of every episode). Envs finished in
        start_state give zeros. w2a_posterior_returns (include/w2a.h): the same vector and the same fp64 FMA chains as
        the step and rollout kernels. Faithful semantics only (fixes other than "budget": ValueError)."""
        if self.fixes - {"budget"}:
            raise ValueError(f"posterior_returns() needs faithful semantics; fixes {sorted(self.fixes - {'budget'})} "
                             "make the reward depend on attempts and other rows")
        ct, n, dev = self.ct, self.num_envs, self.device
        words = (ct.T + 31) // 32
        ad = torch.as_tensor(alert_days, device=dev)
        if ad.dim() != 2 or ad.shape[0] != n or ad.shape[1] > words * 32:
            raise ValueError(f"alert_days must be bool [{n}, T <= {words * 32}], got {tuple(ad.shape)}")
        a32 = torch.nn.functional.pad(ad.to(torch.int32), (0, words * 32 - ad.shape[1])).view(n, words, 32)
        # bits of one word are distinct powers of two: their int32 sum is the word (bit 31 as -2^31, no overflow)
        mask = (a32 << torch.arange(32, dtype=torch.int32, device=dev)).sum(-1, dtype=torch.int32)
        st = {}
        for k in _PR_FIELDS:
            if k not in start_state:
                raise KeyError(f"start_state lacks {k!r} (pass a state() dict)")
            st[k] = torch.as_tensor(start_state[k], device=dev).to(torch.int32).contiguous()
            if st[k].shape != (n,):
                raise ValueError(f"start_state[{k!r}] must have shape ({n},)")
        steps = int(n_steps) if n_steps is not None else ct.T
        with torch.cuda.device(dev):
            return self._posterior_returns_packed(st, mask.contiguous(), words, steps)

    def _posterior_returns_packed(self, st0: dict, mask: torch.Tensor, words: int, steps: int) -> torch.Tensor:
        """w2a_posterior_returns on device int32 state arrays and a packed [N, words] alert bitmap."""
        out = torch.zeros((self.num_envs, self.ct.n_samples), dtype=torch.float32, device=self.device)
        if steps <= 0:
            return out
        v = _ffi.StateView()
        for k in _PR_FIELDS:
            setattr(v, k, st0[k].data_ptr())
        _ffi.check(self._lib.w2a_posterior_returns(self._h, C.byref(v), mask.data_ptr(), words, steps, out.data_ptr(),
                                                   self._stream()), "w2a_posterior_returns")
        return out

    # ------------------------------------------------------------------ imitation: likelihood of a given schedule
    def imitation_gradient(self, policy: dict, alert_days, env_weight=None, n_steps: int | None = None,
                           day_weight=None, labels=None) -> dict:
        """The gradient of the log-likelihood of a GIVEN alert schedule under a linear or MLP policy: the supervised
        counterpart of rollout(policy_gradient=...). Every env is forced along its own schedule from its current state
        and the policy is evaluated on the rows it would have held (teacher forcing), all inside the kernel: behaviour
        cloning of hindsight_optimum()["alert_days"], and with env_weight fitting to the elite envs of a population or
        reward- / advantage-weighted regression.
          policy      a kind="linear" or kind="mlp" dict, as rollout() takes it (group, order, require_budget and the
                      two-row MLP output included; sample and seed are ignored: nothing is drawn). With
                      "allowed_days" an alert the schedule asks for on a disallowed day is attempted as 0
                      and the day is not scored: no gradient, no log-likelihood, and "days" does not count it
          alert_days  bool [N, T] by day of the episode: the actions ATTEMPTED (hindsight_optimum()["alert_days"],
                      rollout(alert_mask=True)["alert_days"]); an attempt with used == budget issues no alert, as in step()
          env_weight  optional float [N], finite (default 1)
          n_steps     days from every env's current day (default: to the end of every episode; an env stops after its
                      terminal day, as in rollout())
          day_weight  optional device float [S >= n_steps, N], finite (ValueError), by call-day and ENV ID, the layout of
                      value_gradient()'s "advantage": the estimator becomes
                      g_e = w_e sum_s d_{s,e} delta_s dz_s/dtheta ("log_likelihood" and "days" are unchanged; None is
                      today's result bit for bit). With the schedule a sampled
                      rollout(alert_mask=True) issued and day_weight an advantage this is the score-function gradient
                      of that rollout with a learned baseline -- exactly so only under require_budget=True, where
                      attempts and issued alerts agree on every scored day; without it rollout(policy_gradient=...)
                      scores an attempt at the budget as a_s = 1 while "alert_days" holds 0 there
          labels      optional second schedule, bool [N, T] or its packed int32 words (ValueError otherwise): the
                      actions to SCORE, while alert_days still forces the env -- rows, budget, streak, gate and
                      require_budget exactly as without it, and the same days are scored. delta_s = labels_s -
                      sigmoid(z_s) and the log-likelihood takes labels_s: DAgger / hindsight relabelling with
                      alert_days the learner's own rollout and labels hindsight_values(alert_days)["expert_alert_days"].
                      labels equal to alert_days is the call without it, bit for bit. Not with "lookahead" (ValueError)
        Returns
          "policy_gradient"       linear: {"weight" f32 [G, n_obs], "bias" f32 [G]}; mlp: {"layers": [(dW, db), ...]}: the
                                  gradient of "group_log_likelihood" (shapes, column order and NaN for a group without
                                  envs as rollout(policy_gradient=...)), so ``theta += lr * grad`` ascends the likelihood
          "log_likelihood"        f32 [N]  sum over the env's scored days of log pi(a*_s | o_s) (unweighted)
          "days"                  i32 [N]  scored days: the days stepped, less those on which require_budget forced the
                                  action because no budget was left (they carry no likelihood)
          "group_log_likelihood"  f32 [G]  mean over the group's envs of env_weight * log_likelihood
        Envs finished on entry contribute zero and count. No side effects: the state, the tables, the observation buffer
        and the RNG are only read, so ``reset -> hindsight_optimum -> K x (imitation_gradient, optimizer step)`` works
        on the same episodes. Needs the observation buffer current (RuntimeError as rollout(kind="linear")) and
        faithful observations (fixes other than "budget": ValueError); reward_mode and the tables' slot-27 coefficients
        do not matter, rewards never enter. w2a_imitation_gradient_linear / _mlp (include/w2a.h)."""
        kind = policy.get("kind") if isinstance(policy, dict) else None
        ct, n, dev = self.ct, self.num_envs, self.device
        mask, w, steps = _policy.check_imitation_args(kind, alert_days, env_weight, n_steps, n, ct.T, dev, self.fixes)
        if kind == "mlp" and policy.get("lookahead") is not None:
            raise ValueError("imitation_gradient() takes 'lookahead' with kind 'linear' only; the mlp kind's gradient "
                             "kernels do not read the lookahead inputs yet")
        if labels is not None and policy.get("lookahead") is not None:
            raise ValueError("imitation_gradient(labels=...) does not take a 'lookahead' policy: the kernels that score "
                             "labels apart from the schedule do not read the lookahead inputs")
        pol = _check_learned(self, policy)  # every argument is checked before anything runs
        dw = _policy.check_day_weight(day_weight, min(steps, 2**31 - 1), n, dev)
        gate = _policy.check_allowed_days(policy, n, ct.T, dev, "imitation_gradient()")
        lab = None if labels is None else _policy.check_schedule(labels, "labels", n, ct.T, dev, "imitation_gradient()")
        if self._needs_reset:
            raise RuntimeError("call reset() before imitation_gradient()")
        if not self._obs_current:
            raise RuntimeError(f"imitation_gradient(kind={kind!r}) reads the observation buffer, which does not hold the "
                               "agents' current rows (write_obs=False, a built-in rollout or load_state_dict since the "
                               "last step()/reset()): call step() or reset() first")
        words = mask.shape[1]
        out = {"log_likelihood": torch.empty(n, dtype=torch.float32, device=dev),
               "days": torch.empty(n, dtype=torch.int32, device=dev)}
        wp = None if w is None else w.data_ptr()
        with torch.cuda.device(dev):
            if kind == "linear":
                lp = _ffi.LinearPolicy()
                lp.weight, lp.bias = pol.weight_slots.data_ptr(), pol.bias.data_ptr()
                lp.group = None if pol.group is None else pol.group.data_ptr()
                lp.n_groups, lp.sample, lp.require_budget, lp.seed = pol.n_groups, 0, int(pol.require_budget), 0
                rows = torch.empty((ct.n_obs + 1 + pol.look_days, n), dtype=torch.float32, device=dev)
                if lab is not None:
                    _ffi.check(self._lib.w2a_relabel_imitation_linear(
                        self._h, C.byref(lp), mask.data_ptr(), words, lab.data_ptr(), wp,
                        None if dw is None else dw.data_ptr(), 0 if dw is None else int(dw.shape[0]), steps,
                        self._obs.data_ptr(), rows.data_ptr(), out["log_likelihood"].data_ptr(), out["days"].data_ptr(),
                        self._stream(), None if gate is None else gate.data_ptr(),
                        0 if gate is None else int(gate.shape[1])), "w2a_relabel_imitation_linear")
                elif pol.look_days:
                    look, ferr = self._lookahead_struct(pol), self._forecast_error_struct(pol)
                    fn = "w2a_lookahead_imitation_gradient_linear" if ferr is None else \
                        "w2a_forecast_imitation_gradient_linear"
                    _ffi.check(getattr(self._lib, fn)(
                        self._h, C.byref(lp), mask.data_ptr(), words, wp, None if dw is None else dw.data_ptr(),
                        0 if dw is None else int(dw.shape[0]), steps, self._obs.data_ptr(), rows.data_ptr(),
                        out["log_likelihood"].data_ptr(), out["days"].data_ptr(), self._stream(), C.byref(look),
                        None if gate is None else gate.data_ptr(), 0 if gate is None else int(gate.shape[1]),
                        *(() if ferr is None else (C.byref(ferr),))), fn)
                elif gate is not None:
                    _ffi.check(self._lib.w2a_imitation_gradient_linear_gated(
                        self._h, C.byref(lp), mask.data_ptr(), words, wp, None if dw is None else dw.data_ptr(),
                        0 if dw is None else int(dw.shape[0]), steps, self._obs.data_ptr(), rows.data_ptr(),
                        out["log_likelihood"].data_ptr(), out["days"].data_ptr(), self._stream(), gate.data_ptr(),
                        int(gate.shape[1])), "w2a_imitation_gradient_linear_gated")
                elif dw is None:
                    _ffi.check(self._lib.w2a_imitation_gradient_linear(
                        self._h, C.byref(lp), mask.data_ptr(), words, wp, steps, self._obs.data_ptr(), rows.data_ptr(),
                        out["log_likelihood"].data_ptr(), out["days"].data_ptr(), self._stream()),
                        "w2a_imitation_gradient_linear")
                else:
                    _ffi.check(self._lib.w2a_imitation_gradient_linear_weighted(
                        self._h, C.byref(lp), mask.data_ptr(), words, wp, dw.data_ptr(), int(dw.shape[0]), steps,
                        self._obs.data_ptr(), rows.data_ptr(), out["log_likelihood"].data_ptr(), out["days"].data_ptr(),
                        self._stream()), "w2a_imitation_gradient_linear_weighted")
                # per-env gradients -> per-group mean, in a fixed order (a sort and an fp64 scan along each column)
                g = _policy.group_mean_columns(rows, pol.group, pol.n_groups)
                # rows: the observation columns, the bias, then the lookahead inputs
                out["policy_gradient"] = {"weight": torch.cat([g[:, :ct.n_obs], g[:, ct.n_obs + 1:]], dim=1).contiguous(),
                                          "bias": g[:, ct.n_obs].contiguous()}
            else:
                mp = _ffi.MlpPolicy()
                mp.params = pol.params.data_ptr()
                mp.group = None if pol.group is None else pol.group.data_ptr()
                # always group-major (the partial blocks are sized for it), whatever "order" a rollout would use
                gorder = None if pol.group is None else (pol.order if pol.group_major else _policy.group_order(pol.group))
                mp.order = None if gorder is None else gorder.data_ptr()
                mp.n_groups, mp.n_layers, mp.width = pol.n_groups, pol.n_layers, pol.width
                mp.activation = _ffi.MLP_ACTIVATIONS[pol.activation]
                mp.sample, mp.require_budget, mp.seed = 0, int(pol.require_budget), 0
                blocks = torch.empty((pol.n_groups, _policy.mlp_stride(pol.width, pol.n_layers)), dtype=torch.float32,
                                     device=dev)
                ws = torch.empty(self._lib.w2a_imitation_gradient_mlp_workspace_bytes(
                    n, steps, pol.n_groups, pol.width, pol.n_layers), dtype=torch.uint8, device=dev)
                if lab is not None:
                    _ffi.check(self._lib.w2a_relabel_imitation_mlp(
                        self._h, C.byref(mp), mask.data_ptr(), words, lab.data_ptr(), wp,
                        None if dw is None else dw.data_ptr(), 0 if dw is None else int(dw.shape[0]), steps,
                        self._obs.data_ptr(), blocks.data_ptr(), out["log_likelihood"].data_ptr(),
                        out["days"].data_ptr(), ws.data_ptr(), ws.numel(), self._stream(),
                        None if gate is None else gate.data_ptr(), 0 if gate is None else int(gate.shape[1])),
                        "w2a_relabel_imitation_mlp")
                elif gate is not None:
                    _ffi.check(self._lib.w2a_imitation_gradient_mlp_gated(
                        self._h, C.byref(mp), mask.data_ptr(), words, wp, None if dw is None else dw.data_ptr(),
                        0 if dw is None else int(dw.shape[0]), steps, self._obs.data_ptr(), blocks.data_ptr(),
                        out["log_likelihood"].data_ptr(), out["days"].data_ptr(), ws.data_ptr(), ws.numel(),
                        self._stream(), gate.data_ptr(), int(gate.shape[1])), "w2a_imitation_gradient_mlp_gated")
                elif dw is None:
                    _ffi.check(self._lib.w2a_imitation_gradient_mlp(
                        self._h, C.byref(mp), mask.data_ptr(), words, wp, steps, self._obs.data_ptr(), blocks.data_ptr(),
                        out["log_likelihood"].data_ptr(), out["days"].data_ptr(), ws.data_ptr(), ws.numel(),
                        self._stream()), "w2a_imitation_gradient_mlp")
                else:
                    _ffi.check(self._lib.w2a_imitation_gradient_mlp_weighted(
                        self._h, C.byref(mp), mask.data_ptr(), words, wp, dw.data_ptr(), int(dw.shape[0]), steps,
                        self._obs.data_ptr(), blocks.data_ptr(), out["log_likelihood"].data_ptr(),
                        out["days"].data_ptr(), ws.data_ptr(), ws.numel(), self._stream()),
                        "w2a_imitation_gradient_mlp_weighted")
                out["policy_gradient"] = {"layers": _policy.unpack_mlp_grad(blocks, ct.obs_slot, ct.n_obs, pol.hidden,
                                                                            pol.n_out)}
            wll = out["log_likelihood"].double() if w is None else (w.double() * out["log_likelihood"].double())
            if pol.group is None:  # one group: the fp64 mean, rounded once
                out["group_log_likelihood"] = wll.mean().to(torch.float32).reshape(1)
            else:
                out["group_log_likelihood"] = _policy.group_mean(wll, pol.group, pol.n_groups)
        return out

    # ------------------------------------------------------------------ PPO-clip: K epochs along a given schedule
    def surrogate_gradient(self, policy: dict, alert_days, advantage, old_log_prob=None, clip: float = 0.2,
                           entropy_coef: float = 0.0, env_weight=None, n_steps: int | None = None,
                           log_prob: bool = False) -> dict:
        """The gradient of the PPO-clip surrogate along a GIVEN alert schedule under a linear or MLP policy: what K
        epochs on the same episodes need, with the clipped importance ratio formed inside the kernel and no observation
        row recorded. Every env is forced along its own schedule exactly as in imitation_gradient() (alert_days holds
        the actions ATTEMPTED; the same rows o_s, the same require_budget rule for the scored days). On every scored
        call-day s of env e, with z_s the logit, a_s the schedule's bit and p_s = sigmoid(z_s):
          lp_s   = log pi(a_s | z_s);   rho_s = exp(lp_s - old_log_prob[s, e])  (exactly 1 for old_log_prob=None)
          live_s = not ((A_s > 0 and rho_s > 1 + clip) or (A_s < 0 and rho_s < 1 - clip)),   A_s = advantage[s, e]
          L_e    = sum_s min(rho_s A_s, clamp(rho_s, 1 - clip, 1 + clip) A_s)
          g_e    = w_e sum_s [live_s rho_s A_s (a_s - p_s) + entropy_coef dH_s/dz] dz_s/dtheta,  H_s the Bernoulli entropy
        and per group the mean of g_e over its envs, so ``theta += lr * grad`` ascends
        mean_e w_e (L_e + entropy_coef sum_s H_s).
          policy        a kind="linear" or kind="mlp" dict, as imitation_gradient() takes it ("allowed_days" included:
                        a disallowed day is attempted as 0 and adds no ratio, entropy, approx_kl or clipped day; "days"
                        does not count it and "log_prob" is 0 there)
          alert_days    bool [N, T] by day of the episode (rollout(alert_mask=True)["alert_days"])
          advantage     float [S >= n_steps, N], finite (ValueError), by call-day and ENV ID: value_gradient()'s
                        "advantage", or any other (GAE, discounting and normalisation are the caller's)
          old_log_prob  optional float [S >= n_steps, N], same layout, <= 0 (ValueError): the "log_prob" of an earlier
                        call under the policy that collected the schedule
          clip          >= 0, finite; entropy_coef finite (ValueError)
          env_weight, n_steps  as imitation_gradient()
          log_prob      True: also return lp_s -- how the first epoch obtains old_log_prob without a recorded rollout
        Returns
          "policy_gradient"  as imitation_gradient() (NaN for a group without envs)
          "surrogate"        f32 [N]  L_e (unweighted)
          "clipped_days"     i32 [N]  scored days with live_s = 0
          "approx_kl"        f32 [N]  sum_s ((rho_s - 1) - log rho_s): SB3's estimator, summed and not averaged
          "entropy"          f32 [N]  sum_s H_s
          "days"             i32 [N]  scored days, as imitation_gradient()
          "group_surrogate"  f32 [G]  mean over the group's envs of env_weight * surrogate
          "log_prob"         (log_prob=True) f32 [S, N] by call-day and env id: lp_s on scored days, 0 elsewhere
        With old_log_prob=None and entropy_coef=0 this is imitation_gradient(day_weight=advantage). No side effects: the
        state, the tables, the observation buffer and the RNG are only read. No floating-point atomics: two identical
        calls give identical bits. Needs the observation buffer current (RuntimeError as imitation_gradient()) and
        faithful observations. Value-loss clipping and minibatches inside a call are not offered.
        w2a_surrogate_gradient_linear / _mlp (include/w2a.h)."""
        _refuse_lookahead(policy, "surrogate_gradient()")
        kind = policy.get("kind") if isinstance(policy, dict) else None
        ct, n, dev = self.ct, self.num_envs, self.device
        mask, w, steps = _policy.check_imitation_args(kind, alert_days, env_weight, n_steps, n, ct.T, dev, self.fixes,
                                                      who="surrogate_gradient()")
        check = _policy.check_linear_policy if kind == "linear" else _policy.check_mlp_policy
        pol = check(policy, ct.n_obs, n, ct.obs_slot, dev)  # every argument is checked before anything runs
        adv, old, clip, beta = _policy.check_surrogate_args(advantage, old_log_prob, clip, entropy_coef,
                                                            min(steps, 2**31 - 1), n, dev)
        gate = _policy.check_allowed_days(policy, n, ct.T, dev, "surrogate_gradient()")
        if self._needs_reset:
            raise RuntimeError("call reset() before surrogate_gradient()")
        if not self._obs_current:
            raise RuntimeError(f"surrogate_gradient(kind={kind!r}) reads the observation buffer, which does not hold the "
                               "agents' current rows (write_obs=False, a built-in rollout or load_state_dict since the "
                               "last step()/reset()): call step() or reset() first")
        words = mask.shape[1]
        out = {"surrogate": torch.empty(n, dtype=torch.float32, device=dev),
               "clipped_days": torch.empty(n, dtype=torch.int32, device=dev),
               "approx_kl": torch.empty(n, dtype=torch.float32, device=dev),
               "entropy": torch.empty(n, dtype=torch.float32, device=dev),
               "days": torch.empty(n, dtype=torch.int32, device=dev)}
        if log_prob:
            out["log_prob"] = torch.empty((steps, n), dtype=torch.float32, device=dev)  # zero-filled by the library
        lpp = out["log_prob"].data_ptr() if log_prob else None
        wp = None if w is None else w.data_ptr()
        oldp, old_days = (None, 0) if old is None else (old.data_ptr(), int(min(old.shape[0], 2**31 - 1)))
        front = (mask.data_ptr(), words, wp, adv.data_ptr(), int(min(adv.shape[0], 2**31 - 1)), oldp, old_days, clip, beta,
                 steps, self._obs.data_ptr())
        outs = (out["surrogate"].data_ptr(), out["clipped_days"].data_ptr(), out["approx_kl"].data_ptr(),
                out["entropy"].data_ptr(), out["days"].data_ptr(), lpp)
        with torch.cuda.device(dev):
            if kind == "linear":
                lp = _ffi.LinearPolicy()
                lp.weight, lp.bias = pol.weight_slots.data_ptr(), pol.bias.data_ptr()
                lp.group = None if pol.group is None else pol.group.data_ptr()
                lp.n_groups, lp.sample, lp.require_budget, lp.seed = pol.n_groups, 0, int(pol.require_budget), 0
                rows = torch.empty((ct.n_obs + 1, n), dtype=torch.float32, device=dev)
                if gate is None:
                    _ffi.check(self._lib.w2a_surrogate_gradient_linear(
                        self._h, C.byref(lp), *front, rows.data_ptr(), *outs, self._stream()),
                        "w2a_surrogate_gradient_linear")
                else:
                    _ffi.check(self._lib.w2a_surrogate_gradient_linear_gated(
                        self._h, C.byref(lp), *front, rows.data_ptr(), *outs, self._stream(), gate.data_ptr(),
                        int(gate.shape[1])), "w2a_surrogate_gradient_linear_gated")
                # per-env gradients -> per-group mean, in a fixed order (a sort and an fp64 scan along each column)
                g = _policy.group_mean_columns(rows, pol.group, pol.n_groups)
                out["policy_gradient"] = {"weight": g[:, :-1].contiguous(), "bias": g[:, -1].contiguous()}
            else:
                mp = _ffi.MlpPolicy()
                mp.params = pol.params.data_ptr()
                mp.group = None if pol.group is None else pol.group.data_ptr()
                # always group-major (the partial blocks are sized for it), whatever "order" a rollout would use
                gorder = None if pol.group is None else (pol.order if pol.group_major else _policy.group_order(pol.group))
                mp.order = None if gorder is None else gorder.data_ptr()
                mp.n_groups, mp.n_layers, mp.width = pol.n_groups, pol.n_layers, pol.width
                mp.activation = _ffi.MLP_ACTIVATIONS[pol.activation]
                mp.sample, mp.require_budget, mp.seed = 0, int(pol.require_budget), 0
                blocks = torch.empty((pol.n_groups, _policy.mlp_stride(pol.width, pol.n_layers)), dtype=torch.float32,
                                     device=dev)
                ws = torch.empty(self._lib.w2a_surrogate_gradient_mlp_workspace_bytes(
                    n, steps, pol.n_groups, pol.width, pol.n_layers), dtype=torch.uint8, device=dev)
                sgm_args = (self._h, C.byref(mp), *front, blocks.data_ptr(), *outs, ws.data_ptr(), ws.numel(),
                            self._stream())
                if gate is None:
                    _ffi.check(self._lib.w2a_surrogate_gradient_mlp(*sgm_args), "w2a_surrogate_gradient_mlp")
                else:
                    _ffi.check(self._lib.w2a_surrogate_gradient_mlp_gated(*sgm_args, gate.data_ptr(),
                                                                          int(gate.shape[1])),
                               "w2a_surrogate_gradient_mlp_gated")
                out["policy_gradient"] = {"layers": _policy.unpack_mlp_grad(blocks, ct.obs_slot, ct.n_obs, pol.hidden,
                                                                            pol.n_out)}
            ws_ = out["surrogate"].double() if w is None else (w.double() * out["surrogate"].double())
            if pol.group is None:  # one group: the fp64 mean, rounded once
                out["group_surrogate"] = ws_.mean().to(torch.float32).reshape(1)
            else:
                out["group_surrogate"] = _policy.group_mean(ws_, pol.group, pol.n_groups)
        return out

    # ------------------------------------------------------------------ natural gradient / TRPO: Fisher-vector products
    def fisher_vector_product(self, policy: dict, alert_days, vector, env_weight=None,
                              n_steps: int | None = None) -> dict:
        """The Fisher-vector product F v of a linear or MLP policy over the episodes at hand, along a GIVEN alert
        schedule: what the natural policy gradient and TRPO's conjugate-gradient step need, formed inside the kernel with
        no observation row recorded. Every env is forced along its own schedule exactly as in surrogate_gradient() (the
        same rows o_s, the same scored days: a day on which require_budget forces the action, or which "allowed_days"
        closes, is not scored). With z_s the logit, p_s = sigmoid(z_s), J_s = dz_s/dtheta and v_g the block of `vector`
        of the env's group:
          u_s  = J_s . v_g
          Fv_e = w_e sum_s p_s (1 - p_s) u_s J_s^T        q_e = sum_s p_s (1 - p_s) u_s^2  (unweighted)
        and per group the mean of Fv_e over its envs, F_g v_g. The labels of the schedule enter only through the states
        visited. 1/2 eps^2 "group_quadratic" is the second-order term of the mean over envs of
        w_e sum_s KL(pi_theta || pi_{theta + eps v}), so TRPO's step length is sqrt(2 delta / group_quadratic) without
        another pass (examples/trpo_on_device.py).
          policy      a kind="linear" or kind="mlp" dict, as surrogate_gradient() takes it ("allowed_days", group,
                      require_budget and the two-row MLP output included; sample and seed are ignored)
          alert_days  bool [N, T] by day of the episode: the actions ATTEMPTED, as surrogate_gradient()
          vector      in the shape of the "policy_gradient" the other calls return -- linear: {"weight": [G, n_obs],
                      "bias": [G]}; mlp: {"layers": [(V, vb), ...]} in the policy's own shapes -- finite (ValueError)
          env_weight, n_steps  as surrogate_gradient()
        Returns
          "fisher_vector_product"  same structure as "policy_gradient" (NaN for a group without envs)
          "quadratic"              f32 [N]  q_e
          "days"                   i32 [N]  scored days, as surrogate_gradient()
          "group_quadratic"        f32 [G]  mean over the group's envs of env_weight * quadratic = <v_g, F_g v_g>
        Envs finished on entry contribute zero and count. No side effects: the state, the tables, the observation buffer
        and the RNG are only read. No floating-point atomics: two identical calls give identical bits. Needs the
        observation buffer current (RuntimeError as surrogate_gradient()) and faithful observations.
        w2a_fisher_vector_product_linear / _mlp (include/w2a.h)."""
        _refuse_lookahead(policy, "fisher_vector_product()")
        kind = policy.get("kind") if isinstance(policy, dict) else None
        ct, n, dev = self.ct, self.num_envs, self.device
        mask, w, steps = _policy.check_imitation_args(kind, alert_days, env_weight, n_steps, n, ct.T, dev, self.fixes,
                                                      who="fisher_vector_product()")
        check = _policy.check_linear_policy if kind == "linear" else _policy.check_mlp_policy
        pol = check(policy, ct.n_obs, n, ct.obs_slot, dev)  # every argument is checked before anything runs
        vec = _policy.check_fisher_args(kind, vector, pol, ct.n_obs, ct.obs_slot, dev)
        gate = _policy.check_allowed_days(policy, n, ct.T, dev, "fisher_vector_product()")
        if self._needs_reset:
            raise RuntimeError("call reset() before fisher_vector_product()")
        if not self._obs_current:
            raise RuntimeError(f"fisher_vector_product(kind={kind!r}) reads the observation buffer, which does not hold "
                               "the agents' current rows (write_obs=False, a built-in rollout or load_state_dict since "
                               "the last step()/reset()): call step() or reset() first")
        words = mask.shape[1]
        out = {"quadratic": torch.empty(n, dtype=torch.float32, device=dev),
               "days": torch.empty(n, dtype=torch.int32, device=dev)}
        wp = None if w is None else w.data_ptr()
        front = (mask.data_ptr(), words, wp, steps, self._obs.data_ptr())
        outs = (out["quadratic"].data_ptr(), out["days"].data_ptr())
        gate_args = (None, 0) if gate is None else (gate.data_ptr(), int(gate.shape[1]))
        with torch.cuda.device(dev):
            if kind == "linear":
                lp = _ffi.LinearPolicy()
                lp.weight, lp.bias = pol.weight_slots.data_ptr(), pol.bias.data_ptr()
                lp.group = None if pol.group is None else pol.group.data_ptr()
                lp.n_groups, lp.sample, lp.require_budget, lp.seed = pol.n_groups, 0, int(pol.require_budget), 0
                rows = torch.empty((ct.n_obs + 1, n), dtype=torch.float32, device=dev)
                _ffi.check(self._lib.w2a_fisher_vector_product_linear(
                    self._h, C.byref(lp), vec[0].data_ptr(), vec[1].data_ptr(), *front, rows.data_ptr(), *outs,
                    self._stream(), *gate_args), "w2a_fisher_vector_product_linear")
                # per-env products -> per-group mean, in a fixed order (a sort and an fp64 scan along each column)
                g = _policy.group_mean_columns(rows, pol.group, pol.n_groups)
                out["fisher_vector_product"] = {"weight": g[:, :-1].contiguous(), "bias": g[:, -1].contiguous()}
            else:
                mp = _ffi.MlpPolicy()
                mp.params = pol.params.data_ptr()
                mp.group = None if pol.group is None else pol.group.data_ptr()
                # always group-major (the partial blocks are sized for it), whatever "order" a rollout would use
                gorder = None if pol.group is None else (pol.order if pol.group_major else _policy.group_order(pol.group))
                mp.order = None if gorder is None else gorder.data_ptr()
                mp.n_groups, mp.n_layers, mp.width = pol.n_groups, pol.n_layers, pol.width
                mp.activation = _ffi.MLP_ACTIVATIONS[pol.activation]
                mp.sample, mp.require_budget, mp.seed = 0, int(pol.require_budget), 0
                blocks = torch.empty((pol.n_groups, _policy.mlp_stride(pol.width, pol.n_layers)), dtype=torch.float32,
                                     device=dev)
                ws = torch.empty(self._lib.w2a_fisher_vector_product_mlp_workspace_bytes(
                    n, steps, pol.n_groups, pol.width, pol.n_layers), dtype=torch.uint8, device=dev)
                _ffi.check(self._lib.w2a_fisher_vector_product_mlp(
                    self._h, C.byref(mp), vec.data_ptr(), *front, blocks.data_ptr(), *outs, ws.data_ptr(), ws.numel(),
                    self._stream(), *gate_args), "w2a_fisher_vector_product_mlp")
                out["fisher_vector_product"] = {"layers": _policy.unpack_mlp_grad(blocks, ct.obs_slot, ct.n_obs,
                                                                                  pol.hidden, pol.n_out)}
            wq = out["quadratic"].double() if w is None else (w.double() * out["quadratic"].double())
            if pol.group is None:  # one group: the fp64 mean, rounded once
                out["group_quadratic"] = wq.mean().to(torch.float32).reshape(1)
            else:
                out["group_quadratic"] = _policy.group_mean(wq, pol.group, pol.n_groups)
        return out

    # ------------------------------------------------------------------ critic: value regression along a schedule
    def value_gradient(self, value: dict, alert_days, env_weight=None, n_steps: int | None = None,
                       advantage: bool = False, gamma: float = 1.0, gae_lambda: float = 1.0, bootstrap: bool = False,
                       value_target: bool = False, target=None) -> dict:
        """The gradient of a least-squares fit of a learned state-value function to the reward-to-go along a GIVEN
        alert schedule, and the advantages it leaves -- the critic of an on-device actor-critic loop, with no
        observation row recorded. `value` is a kind="linear" or kind="mlp" dict as rollout() takes it (groups, padding,
        the two-row output and policy.mlp_from_module included) whose logit is read as a state value,
        V_theta(o) = z(o): no sigmoid, nothing sampled; "sample", "seed" and "require_budget" are ignored.
        Every env is forced along its own schedule from its current state and observation rows exactly as in
        imitation_gradient(): alert_days bool [N, T] by day of the episode holds the actions ATTEMPTED, an attempt
        with used == budget issues no alert, o_s is the row step() would have returned. env_weight and n_steps as there.
        Per env e over the call-days s = 0 .. S_e - 1 it steps:
          r_s  the reward step() pays for that day under the env's own posterior draw
          Q_s  = sum_{s' >= s} r_s'  (undiscounted, truncated at the end of the call: nothing is bootstrapped)
          V_s  = z(o_s)  (mlp: the f32 logit k_rollout_mlp forms on that row; linear: k_rollout_linear's fp64 chain)
          g_e  = w_e sum_s (Q_s - V_s) dV_s/dtheta
        and per group the mean of g_e over its envs (envs finished on entry give zero and count; NaN for a group
        without envs), so ``theta += lr * grad`` DESCENDS 1/2 mean_e w_e sum_s (V_s - Q_s)^2. Returns
          "value_gradient"  in the shapes of rollout()'s "policy_gradient": linear {"weight" f32 [G, n_obs], "bias" f32
                            [G]}; mlp {"layers": [(dW, db), ...]}, usable with policy.mlp_grad_to_module
          "sq_error"        f32 [N]  sum_s (Q_s - V_s)^2
          "days"            i32 [N]  S_e
          "return"          f32 [N]  Q_0
          "group_loss"      f32 [G]  mean over the group's envs of 1/2 env_weight * sq_error
          "advantage"       (advantage=True) f32 [S, N] by call-day and ENV ID: Q_s - V_s on stepped days, 0 elsewhere
                            -- the day_weight of imitation_gradient(), which along a sampled rollout's schedule gives
                            the policy gradient with this critic as baseline
        No side effects: the state, the tables, the schedule, the observation buffer and the RNG are only read. No
        floating-point atomics: two identical calls give identical bits. Needs the observation buffer current
        (RuntimeError as rollout(kind="linear")), reward_mode="sampled" and faithful semantics (ValueError for what
        rollout(policy_gradient=...) refuses: rewards enter here). w2a_value_gradient_linear / _mlp (include/w2a.h).

        GAE(lambda), discounting, a bootstrap past the call and fixed targets. With every argument below at its
        default the call is the one above, bit for bit. Otherwise, with Vn_s the value of the row after day s --
        z(o_{s+1}) while the env holds one inside the call, 0 on the episode's last day, and on the call's last day
        (s + 1 == n_steps) of an unfinished episode z(o_{s+1}) if `bootstrap` else 0:
          delta_s = r_s + gamma Vn_s - V_s;   A_s = delta_s + gamma gae_lambda A_{s+1}, A_{S_e} = 0;   R_s = A_s + V_s
          g_e     = w_e sum_s c_s dV_s/dtheta,  c_s = A_s (the semi-gradient: the target R_s is held fixed, as SB3 does)
          gamma, gae_lambda  finite, in [0, 1] (ValueError); 1, 1 with bootstrap=False is the estimator above, computed
                             by the GAE kernels whenever any of these arguments is not at its default
          bootstrap          plain bool: what makes n_steps < T usable for training on truncated chunks
          value_target       plain bool; True adds "value_target" f32 [S, N]: R_s in the layout of "advantage"
          target             float [S >= n_steps, N] by call-day and ENV ID, finite (checked as surrogate_gradient()'s
                             advantage): c_s = target[s, e] - V_s, PPO's critic epochs on targets fixed at collection
                             time (the "value_target" of the first call). No reward is needed then, so the call also
                             works with reward_mode="posterior_mean", and "return" is left out. Combined with
                             advantage=True, value_target=True, bootstrap=True or a gamma / gae_lambda other than 1:
                             ValueError.
        "sq_error" is sum_s c_s^2, "advantage" holds A_s, "return" stays the UNDISCOUNTED sum_s r_s, "days" and
        "group_loss" as above. Advantage normalisation and a clipped value loss stay with the caller (clipped ratios:
        surrogate_gradient()). w2a_value_gradient_linear_gae / _mlp_gae (include/w2a.h)."""
        _refuse_lookahead(value, "value_gradient()")
        kind = value.get("kind") if isinstance(value, dict) else None
        ct, n, dev = self.ct, self.num_envs, self.device
        # with targets given no reward enters: the reward mode does not matter then (as for imitation_gradient())
        mask, w, steps = _policy.check_value_args(kind, alert_days, env_weight, n_steps, n, ct.T, dev,
                                                  "sampled" if target is not None else self.reward_mode, self.fixes)
        check = _policy.check_linear_policy if kind == "linear" else _policy.check_mlp_policy
        pol = check(value, ct.n_obs, n, ct.obs_slot, dev)  # every argument is checked before anything runs
        gamma, lam, tg, gae = _policy.check_gae_args(gamma, gae_lambda, bootstrap, value_target, advantage, target,
                                                     min(steps, 2**31 - 1), n, dev)
        if self._needs_reset:
            raise RuntimeError("call reset() before value_gradient()")
        if not self._obs_current:
            raise RuntimeError(f"value_gradient(kind={kind!r}) reads the observation buffer, which does not hold the "
                               "agents' current rows (write_obs=False, a built-in rollout or load_state_dict since the "
                               "last step()/reset()): call step() or reset() first")
        words = mask.shape[1]
        out = {"sq_error": torch.empty(n, dtype=torch.float32, device=dev),
               "days": torch.empty(n, dtype=torch.int32, device=dev),
               "return": torch.empty(n, dtype=torch.float32, device=dev)}
        if advantage:
            out["advantage"] = torch.empty((steps, n), dtype=torch.float32, device=dev)  # zero-filled by the library
        if value_target:
            out["value_target"] = torch.empty((steps, n), dtype=torch.float32, device=dev)  # zero-filled by the library
        ap = out["advantage"].data_ptr() if advantage else None
        wp = None if w is None else w.data_ptr()
        # what the *_gae entry points take after `advantage`
        tail = (gamma, lam, int(bootstrap), out["value_target"].data_ptr() if value_target else None,
                None if tg is None else tg.data_ptr(), 0 if tg is None else int(min(tg.shape[0], 2**31 - 1)))
        with torch.cuda.device(dev):
            if kind == "linear":
                lp = _ffi.LinearPolicy()
                lp.weight, lp.bias = pol.weight_slots.data_ptr(), pol.bias.data_ptr()
                lp.group = None if pol.group is None else pol.group.data_ptr()
                lp.n_groups, lp.sample, lp.require_budget, lp.seed = pol.n_groups, 0, 0, 0
                rows = torch.empty((ct.n_obs + 1, n), dtype=torch.float32, device=dev)
                if gae:
                    ws = torch.empty(self._lib.w2a_value_gradient_linear_gae_workspace_bytes(n, steps),
                                     dtype=torch.uint8, device=dev)
                    _ffi.check(self._lib.w2a_value_gradient_linear_gae(
                        self._h, C.byref(lp), mask.data_ptr(), words, wp, steps, self._obs.data_ptr(), rows.data_ptr(),
                        out["sq_error"].data_ptr(), out["days"].data_ptr(), out["return"].data_ptr(), ap, *tail,
                        ws.data_ptr(), ws.numel(), self._stream()), "w2a_value_gradient_linear_gae")
                else:
                    ws = torch.empty(self._lib.w2a_value_gradient_linear_workspace_bytes(n, steps), dtype=torch.uint8,
                                     device=dev)
                    _ffi.check(self._lib.w2a_value_gradient_linear(
                        self._h, C.byref(lp), mask.data_ptr(), words, wp, steps, self._obs.data_ptr(), rows.data_ptr(),
                        out["sq_error"].data_ptr(), out["days"].data_ptr(), out["return"].data_ptr(), ap, ws.data_ptr(),
                        ws.numel(), self._stream()), "w2a_value_gradient_linear")
                # per-env gradients -> per-group mean, in a fixed order (a sort and an fp64 scan along each column)
                g = _policy.group_mean_columns(rows, pol.group, pol.n_groups)
                out["value_gradient"] = {"weight": g[:, :-1].contiguous(), "bias": g[:, -1].contiguous()}
            else:
                mp = _ffi.MlpPolicy()
                mp.params = pol.params.data_ptr()
                mp.group = None if pol.group is None else pol.group.data_ptr()
                # always group-major (the partial blocks are sized for it), whatever "order" a rollout would use
                gorder = None if pol.group is None else (pol.order if pol.group_major else _policy.group_order(pol.group))
                mp.order = None if gorder is None else gorder.data_ptr()
                mp.n_groups, mp.n_layers, mp.width = pol.n_groups, pol.n_layers, pol.width
                mp.activation = _ffi.MLP_ACTIVATIONS[pol.activation]
                mp.sample, mp.require_budget, mp.seed = 0, 0, 0
                blocks = torch.empty((pol.n_groups, _policy.mlp_stride(pol.width, pol.n_layers)), dtype=torch.float32,
                                     device=dev)
                ws = torch.empty(self._lib.w2a_value_gradient_mlp_workspace_bytes(
                    n, steps, pol.n_groups, pol.width, pol.n_layers), dtype=torch.uint8, device=dev)  # both routes
                if gae:
                    _ffi.check(self._lib.w2a_value_gradient_mlp_gae(
                        self._h, C.byref(mp), mask.data_ptr(), words, wp, steps, self._obs.data_ptr(), blocks.data_ptr(),
                        out["sq_error"].data_ptr(), out["days"].data_ptr(), out["return"].data_ptr(), ap, *tail,
                        ws.data_ptr(), ws.numel(), self._stream()), "w2a_value_gradient_mlp_gae")
                else:
                    _ffi.check(self._lib.w2a_value_gradient_mlp(
                        self._h, C.byref(mp), mask.data_ptr(), words, wp, steps, self._obs.data_ptr(), blocks.data_ptr(),
                        out["sq_error"].data_ptr(), out["days"].data_ptr(), out["return"].data_ptr(), ap, ws.data_ptr(),
                        ws.numel(), self._stream()), "w2a_value_gradient_mlp")
                out["value_gradient"] = {"layers": _policy.unpack_mlp_grad(blocks, ct.obs_slot, ct.n_obs, pol.hidden,
                                                                           pol.n_out)}
            half = 0.5 * (out["sq_error"].double() if w is None else (w.double() * out["sq_error"].double()))
            if pol.group is None:  # one group: the fp64 mean, rounded once
                out["group_loss"] = half.mean().to(torch.float32).reshape(1)
            else:
                out["group_loss"] = _policy.group_mean(half, pol.group, pol.n_groups)
        if tg is not None:
            del out["return"]  # no reward was formed
        return out

    # ------------------------------------------------------------------ Q-learning along a schedule
    def q_gradient(self, q: dict, alert_days, target_net: dict | None = None, gamma: float = 0.99, double: bool = False,
                   loss: str = "huber", huber_delta: float = 1.0, env_weight=None, n_steps: int | None = None,
                   bootstrap: bool = False, td_error: bool = False, td_target: bool = False) -> dict:
        """The DQN / double-DQN temporal-difference semi-gradient of a two-head MLP Q-net along a GIVEN alert schedule,
        with no observation row recorded: an episode is regenerated from its seed (reset(seed=) on a twin) and forced
        along its schedule, so a replay buffer is a list of (seed, alert_days) pairs, 1 bit per env-day.
          q           a kind="mlp" dict as rollout() takes it (groups, padded widths, tanh or ReLU,
                      policy.mlp_from_module(model.q_net.q_net)) whose output layer has exactly TWO rows: row a is
                      Q(o, a). A one-row output, "allowed_days", "sample" and an "order" that is not group-major:
                      ValueError. "require_budget": True masks the next row's max / argmax, see below.
          target_net  None (the online net is its own target) or a second dict with the same hidden widths, activation
                      and number of groups (ValueError otherwise)
          alert_days, env_weight, n_steps, bootstrap   as value_gradient()
        Every env is forced along its own schedule exactly as in value_gradient() (the same rows o_s, the same rewards).
        Per env e over the call-days s it steps, with a_s the alert actually ISSUED (after the budget test):
          N_s     = 0 on the episode's last day, and on the call's last day unless bootstrap=True; otherwise
                    max_a' Qt(o_{s+1}, a'), or with double=True Qt(o_{s+1}, a*), a* = 1 iff Q(o_{s+1}, 1) > Q(o_{s+1}, 0)
                    under the ONLINE net. With "require_budget" the max / argmax is restricted to a' = 0 when no budget
                    is left after day s: an alert there is a no-op (action masking).
          y_s     = r_s + gamma N_s;   delta_s = y_s - Q(o_s, a_s)
          c_s     = delta_s for loss="squared" (l = delta^2 / 2); clamp(delta_s, +-huber_delta) for "huber" (l = delta^2 / 2
                    inside, huber_delta (|delta| - huber_delta / 2) outside: SB3's smooth_l1_loss at huber_delta = 1)
          g_e     = w_e sum_s c_s dQ(o_s, a_s)/dtheta   (the semi-gradient: nothing flows through y_s)
        and per group the mean of g_e over its envs, so ``theta += lr * grad`` DESCENDS the TD loss ("Adam descends":
        policy.mlp_heads_grad_to_module writes the negated gradient into an SB3-shaped q_net). Returns
          "q_gradient"   {"layers": [(dW, db), ...]} in the net's own shapes, the output layer with its two rows; the
                         mean over each group's envs (envs finished on entry give zero and count; NaN for a group
                         without envs)
          "loss"         f32 [N]  sum_s l(delta_s), unweighted
          "days"         i32 [N]  days scored (every stepped day is)
          "return"       f32 [N]  sum_s r_s along the schedule (undiscounted)
          "group_loss"   f32 [G]  mean over the group's envs of env_weight * loss
          "td_error"     (td_error=True) f32 [S, N] by call-day and ENV ID: delta_s on stepped days, 0 elsewhere -- what
                         prioritised replay needs
          "td_target"    (td_target=True) f32 [S, N]: y_s
        No side effects: the state, the tables, the schedule, the observation buffer and the RNG are only read. No
        floating-point atomics: two identical calls give identical bits. Needs the observation buffer current
        (RuntimeError as value_gradient()), reward_mode="sampled" and faithful semantics (ValueError where
        value_gradient() refuses: rewards enter here). w2a_q_gradient_mlp (include/w2a.h)."""
        who = "q_gradient()"
        ct, n, dev = self.ct, self.num_envs, self.device
        _refuse_lookahead(q, who)
        _refuse_lookahead(target_net, who)
        if not isinstance(q, dict) or q.get("kind") != "mlp":
            raise ValueError(f"{who} needs kind 'mlp', got {q.get('kind') if isinstance(q, dict) else q!r}")
        mask, w, steps = _policy.check_imitation_args("mlp", alert_days, env_weight, n_steps, n, ct.T, dev, self.fixes,
                                                      who=who)
        if self.reward_mode != "sampled":
            raise ValueError(f"{who} needs reward_mode='sampled'")
        pol, tparams = _policy.check_q_net(q, target_net, ct.n_obs, n, ct.obs_slot, dev, who)
        gamma, huber_delta = _policy.check_q_args(gamma, double, loss, huber_delta, bootstrap, td_error, td_target, who)
        if self._needs_reset:
            raise RuntimeError("call reset() before q_gradient()")
        if not self._obs_current:
            raise RuntimeError("q_gradient() reads the observation buffer, which does not hold the agents' current rows "
                               "(write_obs=False, a built-in rollout or load_state_dict since the last step()/reset()): "
                               "call step() or reset() first")
        words = mask.shape[1]
        out = {"loss": torch.empty(n, dtype=torch.float32, device=dev),
               "days": torch.empty(n, dtype=torch.int32, device=dev),
               "return": torch.empty(n, dtype=torch.float32, device=dev)}
        for key, wanted in (("td_error", td_error), ("td_target", td_target)):
            if wanted:
                out[key] = torch.empty((steps, n), dtype=torch.float32, device=dev)  # zero-filled by the library
        with torch.cuda.device(dev):
            mp = _ffi.MlpPolicy()
            mp.params = pol.params.data_ptr()
            mp.group = None if pol.group is None else pol.group.data_ptr()
            mp.order = None if pol.group is None else pol.order.data_ptr()  # group-major: check_q_net
            mp.n_groups, mp.n_layers, mp.width = pol.n_groups, pol.n_layers, pol.width
            mp.activation = _ffi.MLP_ACTIVATIONS[pol.activation]
            mp.sample, mp.require_budget, mp.seed = 0, int(pol.require_budget), 0
            tp = None
            if tparams is not None:
                tp = _ffi.MlpPolicy()
                tp.params, tp.group, tp.order = tparams.data_ptr(), None, None
                tp.n_groups, tp.n_layers, tp.width, tp.activation = mp.n_groups, mp.n_layers, mp.width, mp.activation
                tp.sample, tp.require_budget, tp.seed = 0, 0, 0
            blocks = torch.empty((pol.n_groups, _policy.mlp_heads_stride(pol.width, pol.n_layers)), dtype=torch.float32,
                                 device=dev)
            ws = torch.empty(self._lib.w2a_q_gradient_mlp_workspace_bytes(n, steps, pol.n_groups, pol.width, pol.n_layers),
                             dtype=torch.uint8, device=dev)
            _ffi.check(self._lib.w2a_q_gradient_mlp(
                self._h, C.byref(mp), None if tp is None else C.byref(tp), mask.data_ptr(), words,
                None if w is None else w.data_ptr(), steps, self._obs.data_ptr(), blocks.data_ptr(),
                out["loss"].data_ptr(), out["days"].data_ptr(), out["return"].data_ptr(), gamma, int(double),
                _ffi.Q_LOSSES[loss], huber_delta, int(bootstrap), out["td_error"].data_ptr() if td_error else None,
                out["td_target"].data_ptr() if td_target else None, ws.data_ptr(), ws.numel(), self._stream()),
                "w2a_q_gradient_mlp")
            out["q_gradient"] = {"layers": _policy.unpack_mlp_heads_grad(blocks, ct.obs_slot, ct.n_obs, pol.hidden)}
            wl = out["loss"].double() if w is None else (w.double() * out["loss"].double())
            if pol.group is None:  # one group: the fp64 mean, rounded once
                out["group_loss"] = wl.mean().to(torch.float32).reshape(1)
            else:
                out["group_loss"] = _policy.group_mean(wl, pol.group, pol.n_groups)
        return out

    # ------------------------------------------------------------------ shared-trunk actor-critic (PPO)
    def actor_critic_gradient(self, net: dict, alert_days, advantage=None, value_target=None, old_log_prob=None,
                              clip: float = 0.2, vf_coef: float = 0.5, entropy_coef: float = 0.0, gamma: float = 1.0,
                              gae_lambda: float = 1.0, bootstrap: bool = False, env_weight=None,
                              n_steps: int | None = None, gradient: bool = True) -> dict:
        """PPO for ONE network with a shared trunk: the ascent direction of the clipped surrogate, the entropy bonus and
        the value loss together, along a GIVEN alert schedule, with one row rebuild, one forward and one backward pass
        per env-day where value_gradient() plus surrogate_gradient() on two networks take two of each.
          net         a kind="mlp" dict as surrogate_gradient() takes it (hidden shapes, tanh or ReLU, "group",
                      "require_budget", "allowed_days") whose output layer has exactly TWO rows: row 0 is the policy
                      logit z, row 1 the state value V. A linear kind, another number of rows, "lookahead": ValueError.
          alert_days, env_weight, n_steps   as surrogate_gradient()
        Every env is forced along its own schedule exactly as in surrogate_gradient() / value_gradient(): the same rows
        o_s, the same scored days (a day "require_budget" forces or "allowed_days" closes is attempted as 0 and has no
        policy score; the value term still applies there). Per group the call returns the ASCENT direction of
          J_g = (1/n_g) sum_e w_e sum_s [ L^clip_s + entropy_coef H_s - (vf_coef / 2) (T_s - V_s)^2 ]
        with the per-day coefficients c_pi,s = surrogate_gradient()'s on dz_s/dtheta and c_v,s = w_e vf_coef (T_s - V_s)
        on dV_s/dtheta. The value loss carries the factor 1/2: stable-baselines3's vf_coef multiplies mean (T - V)^2, whose
        gradient is twice this one's, so SB3's vf_coef = 0.5 is vf_coef = 1.0 here.
        COLLECT (advantage, value_target and old_log_prob all None): the rewards are those step() pays; with V the net's
        own row 1, delta_s = r_s + gamma Vn_s - V_s, A_s = delta_s + gamma gae_lambda A_{s+1} (GAE(lambda); Vn_s and
        bootstrap as in value_gradient()), T_s = A_s + V_s; rho = 1, nothing is clipped, T_s - V_s = A_s. Always returns
          "advantage", "value_target", "log_prob"  f32 [S, N] by call-day and ENV ID (0 where the env does not step / is
                      not scored): bit for bit value_gradient()'s and surrogate_gradient(log_prob=True)'s for the two
                      one-output nets made of the trunk and row 1 / row 0
          "return"    f32 [N]  sum_s r_s (undiscounted)
        gradient=False skips the second pass and returns no "gradient" and no "group_objective" (the first pass is the
        cheap part). reward_mode="posterior_mean": ValueError, as value_gradient().
        EPOCH (all three given, float [S >= n_steps, N]; one or two: ValueError): advantages and targets are fixed (the
        caller may normalise the advantages in between), the clipped ratio is formed in the kernel from old_log_prob, no
        reward is formed -- reward_mode="posterior_mean" is accepted, as value_gradient(target=). gamma, gae_lambda and
        bootstrap must stay at their defaults.
        Both modes return
          "gradient"         {"layers": [(dW, db), ...]} in the net's own shapes, the output layer with its two rows
                             (policy.mlp_heads_grad_to_module writes it into a module); NaN for a group without envs
          "surrogate", "entropy", "approx_kl", "clipped_days", "days"   per env, as surrogate_gradient()
          "value_loss"       f32 [N]  sum_s 1/2 (T_s - V_s)^2, unweighted by vf_coef
          "group_objective"  f32 [G]  mean over the group's envs of w_e (surrogate + entropy_coef entropy - vf_coef value_loss)
        No side effects: the state, the tables, the observation buffer and the RNG are only read. No floating-point
        atomics: two identical calls give identical bits. Needs the observation buffer current (RuntimeError as
        surrogate_gradient()) and faithful observations. w2a_actor_critic_mlp (include/w2a.h)."""
        who = "actor_critic_gradient()"
        _refuse_lookahead(net, who)
        ct, n, dev = self.ct, self.num_envs, self.device
        pol = _policy.check_actor_critic_net(net, ct.n_obs, n, ct.obs_slot, dev, who)
        mask, w, steps = _policy.check_imitation_args("mlp", alert_days, env_weight, n_steps, n, ct.T, dev, self.fixes,
                                                      who=who)
        adv, vt, old, clip, vf_coef, beta, gamma, lam = _policy.check_actor_critic_args(
            advantage, value_target, old_log_prob, clip, vf_coef, entropy_coef, gamma, gae_lambda, bootstrap, gradient,
            min(steps, 2**31 - 1), n, dev, who)
        epoch = adv is not None
        if not epoch and self.reward_mode != "sampled":
            raise ValueError(f"{who} needs reward_mode='sampled' to collect (rewards enter; an epoch on given "
                             "advantages and targets does not)")
        gate = _policy.check_allowed_days(net, n, ct.T, dev, who)
        if self._needs_reset:
            raise RuntimeError("call reset() before actor_critic_gradient()")
        if not self._obs_current:
            raise RuntimeError("actor_critic_gradient() reads the observation buffer, which does not hold the agents' "
                               "current rows (write_obs=False, a built-in rollout or load_state_dict since the last "
                               "step()/reset()): call step() or reset() first")
        words = mask.shape[1]
        f32 = dict(dtype=torch.float32, device=dev)
        out = {"surrogate": torch.empty(n, **f32), "value_loss": torch.empty(n, **f32),
               "clipped_days": torch.empty(n, dtype=torch.int32, device=dev), "approx_kl": torch.empty(n, **f32),
               "entropy": torch.empty(n, **f32), "days": torch.empty(n, dtype=torch.int32, device=dev)}
        if not epoch:
            out["return"] = torch.empty(n, **f32)
            for key in ("advantage", "value_target", "log_prob"):
                out[key] = torch.empty((steps, n), **f32)  # zero-filled by the library
        ptr = lambda key: out[key].data_ptr() if key in out else None  # noqa: E731
        rows = lambda t: (None, 0) if t is None else (t.data_ptr(), int(min(t.shape[0], 2**31 - 1)))  # noqa: E731
        with torch.cuda.device(dev):
            mp = _ffi.MlpPolicy()
            mp.params = pol.params.data_ptr()
            mp.group = None if pol.group is None else pol.group.data_ptr()
            mp.order = None if pol.group is None else pol.order.data_ptr()  # group-major: check_actor_critic_net
            mp.n_groups, mp.n_layers, mp.width = pol.n_groups, pol.n_layers, pol.width
            mp.activation = _ffi.MLP_ACTIVATIONS[pol.activation]
            mp.sample, mp.require_budget, mp.seed = 0, int(pol.require_budget), 0
            blocks = None
            if gradient:
                blocks = torch.empty((pol.n_groups, _policy.mlp_heads_stride(pol.width, pol.n_layers)), **f32)
            ws = torch.empty(self._lib.w2a_actor_critic_mlp_workspace_bytes(n, steps, pol.n_groups, pol.width,
                                                                            pol.n_layers), dtype=torch.uint8, device=dev)
            _ffi.check(self._lib.w2a_actor_critic_mlp(
                self._h, C.byref(mp), mask.data_ptr(), words, None if w is None else w.data_ptr(), *rows(adv), *rows(vt),
                *rows(old), clip, vf_coef, beta, gamma, lam, int(bootstrap), steps, self._obs.data_ptr(),
                None if blocks is None else blocks.data_ptr(), ptr("surrogate"), ptr("value_loss"), ptr("clipped_days"),
                ptr("approx_kl"), ptr("entropy"), ptr("days"), ptr("return"), ptr("advantage"), ptr("value_target"),
                ptr("log_prob"), ws.data_ptr(), ws.numel(), self._stream(),
                None if gate is None else gate.data_ptr(), 0 if gate is None else int(gate.shape[1])),
                "w2a_actor_critic_mlp")
            if gradient:
                out["gradient"] = {"layers": _policy.unpack_mlp_heads_grad(blocks, ct.obs_slot, ct.n_obs, pol.hidden)}
                obj = out["surrogate"].double() + beta * out["entropy"].double() - vf_coef * out["value_loss"].double()
                if w is not None:
                    obj = w.double() * obj
                if pol.group is None:  # one group: the fp64 mean, rounded once
                    out["group_objective"] = obj.mean().to(torch.float32).reshape(1)
                else:
                    out["group_objective"] = _policy.group_mean(obj, pol.group, pol.n_groups)
        return out

    # ------------------------------------------------------------------ hindsight optimum
    def hindsight_optimum(self, start_state: dict | None = None, n_steps: int | None = None,
                          allowed_days=None) -> dict:
        """Every env's best alert schedule in hindsight: knowing the weather of the whole stretch, the env's own
        posterior draw and its remaining budget, the schedule of at most budget - used alerts with the highest return
        over the days from start_state (a state() dict; default: the current state) for n_steps days (default: to the
        end of every episode; each env stops after its terminal day, as in rollout()). The upper bound a policy's return
        reads against as regret, and an expert schedule for imitation. Returns
            "return":     f32 [N]     the schedule's return: bit for bit what the env pays when stepped with it
                                      (posterior_returns(start_state, alert_days)[:, sample])
            "alert_days": bool [N, T] the schedule (day of the episode; only the stretch's days can be set)
            "alerts":     i32 [N]     alerts in it
        Envs finished in start_state give 0 and an empty schedule. An exact DP over (alerts issued, current streak)
        (w2a_hindsight_optimum, include/w2a.h); ties do not alert. Reads start_state and the tables only: the env's
        state, observation buffer and bookkeeping are untouched. Sampled reward and faithful semantics only; tables
        whose slot-27 (alert_2wks of the agent) coefficient is nonzero are refused (ValueError).
        allowed_days: optional bool [N, T] by day of the episode (alert_gate(), or any other mask; ValueError for
        another dtype or shape): the DP may alert only on allowed days, so the result is the best schedule UNDER the
        restriction -- the regret yardstick and the imitation expert of a policy with the same "allowed_days". Its
        return is still bit for bit what the env pays for that schedule."""
        who = "hindsight_optimum()"
        self._check_hindsight(who)
        ct, n, dev = self.ct, self.num_envs, self.device
        gate = _policy.check_allowed_days({"kind": "linear", "allowed_days": allowed_days}, n, ct.T, dev, who)
        st = self._hs_start_state(start_state)
        steps = self._hs_steps(n_steps, who, strict=False)
        with torch.cuda.device(dev):
            ret, mask, alerts = self._hindsight_packed(st, steps, gate)
        return {"return": ret, "alert_days": _policy.unpack_alert_days(mask, ct.T), "alerts": alerts}

    def hindsight_posterior_optimum(self, start_state: dict | None = None, n_steps: int | None = None,
                                    allowed_days=None, share: bool = True, posterior_returns: bool = False) -> dict:
        """Every env's best alert schedule in hindsight WITH THE DRAW UNKNOWN: knowing the weather of the whole stretch
        and the remaining budget, but not the env's posterior draw, the schedule of at most budget - used alerts with
        the highest return AVERAGED OVER ALL n_samples DRAWS of the env's coefficient column. No policy observes the
        draw, so this -- not hindsight_optimum() -- is the bound a policy can reach, an imitation expert whose labels
        are functions of what a policy sees, and the yardstick of a reward_mode="posterior_mean" env (which pays that
        average). start_state, n_steps and allowed_days as hindsight_optimum(). Returns
            "return":     f32 [N]     the schedule's posterior-mean return: the fp64 sum over its days of the mean
                                      over draws of the f32 rewards, rounded once (the draw-mean of
                                      posterior_returns(start_state, alert_days) up to f32 rounding)
            "alert_days": bool [N, T] the schedule (day of the episode; only the stretch's days can be set)
            "alerts":     i32 [N]     alerts in it
            "posterior_returns" (posterior_returns=True): f32 [N, n_samples], posterior_returns(start_state, alert_days)
                                      on the schedule: column `sample` is what a sampled env pays for it, and the
                                      rows feed stats.posterior_summary
        Envs finished in start_state give 0 and an empty schedule, a start outside the tables NaN; ties do not alert.
        hindsight_optimum()'s exact DP over (alerts issued, current streak) with the reward of every state averaged over
        the draws in fp64, in draw order (w2a_hindsight_posterior, include/w2a.h); with n_samples = 1 the schedule is
        hindsight_optimum()'s bit for bit. The result does not depend on `sample`: with share=True (the default) envs
        that agree on t, used, streak, budget, n_days, county_w, year_i, coef_col and finished are found on the host
        (torch.unique), one of each runs and the outputs are gathered back -- bit for bit what share=False, which runs
        every env, returns. With allowed_days every env has its own gate row and nothing is shared.
        Sampled and posterior_mean envs alike; faithful semantics only, and tables whose slot-27 coefficient is nonzero
        or whose n_samples is beyond the kernel's per-draw arrays (657 draws at 153 days) are refused before anything
        is written. Reads start_state and the tables only: the env's state, observation buffer and bookkeeping are
        untouched."""
        who = "hindsight_posterior_optimum()"
        self._check_hindsight_fixes(who)
        self._check_hindsight_slot27(who)
        ct, n, dev = self.ct, self.num_envs, self.device
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise _ffi.W2AError(f"{who}: the stream is recording a hipGraph; the call finds the distinct problems and "
                                "sizes its launches on the host")
        gate = _policy.check_allowed_days({"kind": "linear", "allowed_days": allowed_days}, n, ct.T, dev, who)
        st = self._hs_start_state(start_state)
        steps = self._hs_steps(n_steps, who, strict=False)
        with torch.cuda.device(dev):
            if share and gate is None and n:
                rep, inv, _, m = self._hs_posterior_share(st)
                ret, mask, alerts = (x[:m][inv] for x in self._hindsight_packed(rep, steps, None, posterior=True))
                self.last_hindsight_posterior_keys = int(m)
            else:
                ret, mask, alerts = self._hindsight_packed(st, steps, gate, posterior=True)
                self.last_hindsight_posterior_keys = n
        out = {"return": ret, "alert_days": _policy.unpack_alert_days(mask, ct.T), "alerts": alerts}
        if posterior_returns:
            pr_state = dict(start_state) if start_state is not None else self.state()
            out["posterior_returns"] = self.posterior_returns(pr_state, out["alert_days"], n_steps=n_steps)
        return out

    def hindsight_values(self, alert_days, start_state: dict | None = None, n_steps: int | None = None,
                         allowed_days=None, value: bool = False, loss: bool = False) -> dict:
        """What hindsight_optimum()'s DP says in the states a GIVEN schedule reaches: the expert's action on every day
        of a learner's own rollout (the labels of DAgger / hindsight relabelling, see imitation_gradient(labels=...))
        and each day's share of the regret. The env is walked from start_state (a state() dict; default: the current
        state) along alert_days for n_steps days (default: to the end of every episode), H_e = min(n_steps, n_days - t)
        days per env.
          alert_days    bool [N, T] by day of the episode or its packed int32 words (hindsight_optimum()["alert_days"],
                        rollout(alert_mask=True)["alert_days"]): the actions ATTEMPTED; an attempt with no budget left
                        is a no-op, as in step()
          allowed_days  as hindsight_optimum(): an attempt on a closed day is 0 before the budget test, and the DP
                        may alert only on allowed days
        In the state of call-day s, with the recurrence, the fp64 values, the bit-identical rewards and the strict
        comparison of hindsight_optimum(): Q0 = r0 + V(no alert), Q1 = r1 + V(alert), the latter only while budget is
        left on an allowed day. Returns device tensors, [S, N] by call-day and env id as value_gradient()'s "advantage":
            "alert_gain"         f32 [S, N]  Q1 - Q0 (the difference in fp64); NaN where no alert is possible (budget
                                             spent, day closed, s >= H_e)
            "expert_alert_days"  bool [N, T] day t0 + s is set iff Q1 > Q0: the DP's own decision in that state
            "regret"             f32 [N]     the fp64 sum over the env's days of V(state) - Q(issued alert): the
                                             optimum's value from start_state less what the schedule earns
            "value"  (value=True) f32 [S, N] V(state) = max(Q0, Q1); 0 for s >= H_e
            "loss"   (loss=True)  f32 [S, N] V(state) - Q(issued alert) >= 0, exactly 0 where the alert issued is the
                                             expert's; 0 for s >= H_e
        Along hindsight_optimum()'s own schedule the expert bits are the schedule and every loss and the regret are 0.
        Envs finished in start_state give 0, NaN gains and no bits; a start state outside the tables gives NaN. Refuses
        what hindsight_optimum() refuses, before anything is written; reads start_state, the tables and the schedule
        only: the env's state, observation buffer and bookkeeping are untouched. w2a_hindsight_along (include/w2a.h)."""
        who = "hindsight_values()"
        self._check_hindsight(who)
        ct, n, dev = self.ct, self.num_envs, self.device
        mask = _policy.check_schedule(alert_days, "alert_days", n, ct.T, dev, who)
        gate = _policy.check_allowed_days({"kind": "linear", "allowed_days": allowed_days}, n, ct.T, dev, who)
        st = self._hs_start_state(start_state)
        steps = self._hs_steps(n_steps, who, strict=True)
        words = mask.shape[1]

        def rows(fill):  # the library writes the first min(steps, T) call-days
            if steps > ct.T:
                return torch.full((steps, n), fill, dtype=torch.float32, device=dev)
            return torch.empty((steps, n), dtype=torch.float32, device=dev)

        gain = rows(float("nan"))
        val = rows(0.0) if value else None
        los = rows(0.0) if loss else None
        expert = torch.empty((n, words), dtype=torch.int32, device=dev)
        regret = torch.empty(n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ws_bytes = self._lib.w2a_hindsight_workspace_bytes(self._h, steps, self._hs_max_remaining(st), _HS_BIG_ENVS)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            v = self._hs_state_view(st)
            _ffi.check(self._lib.w2a_hindsight_along(
                self._h, C.byref(v), steps, mask.data_ptr(), words, None if gate is None else gate.data_ptr(),
                0 if gate is None else int(gate.shape[1]), gain.data_ptr(), expert.data_ptr(), regret.data_ptr(),
                None if val is None else val.data_ptr(), None if los is None else los.data_ptr(), ws.data_ptr(),
                ws_bytes, self._stream()), "w2a_hindsight_along")
        out = {"alert_gain": gain, "expert_alert_days": _policy.unpack_alert_days(expert, ct.T), "regret": regret}
        if value:
            out["value"] = val
        if loss:
            out["loss"] = los
        return out

    def hindsight_posterior_values(self, alert_days, start_state: dict | None = None, n_steps: int | None = None,
                                   allowed_days=None, value: bool = False, loss: bool = False,
                                   share: bool = True) -> dict:
        """hindsight_values() with THE DRAW UNKNOWN: what hindsight_posterior_optimum()'s DP says in the states a GIVEN
        schedule reaches. The draw-blind expert's action on every day of a learner's own rollout -- DAgger labels that
        are functions of what a policy sees (imitation_gradient(labels=...), examples/dagger_draw_blind.py) -- and each
        day's share of the regret against the bound a policy can reach. alert_days, start_state, n_steps (an int),
        allowed_days, value and loss as hindsight_values(); the keys, the [S, N] shapes by call-day and the fills (NaN
        gains and 0 for s >= H_e and beyond T, 0 / NaN gains / no bits for finished envs, NaN for a start outside the
        tables) are that call's too, with Q0 = m0 + V(no alert), Q1 = m1 + V(alert) and m the reward averaged over all
        n_samples draws of the env's coefficient column in fp64, in draw order:
            "alert_gain"         f32 [S, N]  Q1 - Q0; NaN where no alert is possible
            "expert_alert_days"  bool [N, T] day t0 + s is set iff Q1 > Q0
            "regret"             f32 [N]     the fp64 sum over the env's days of V(state) - Q(issued alert):
                                             hindsight_posterior_optimum()'s return from start_state less the
                                             schedule's posterior-mean return
            "value"  (value=True) f32 [S, N] V(state) = max(Q0, Q1)
            "loss"   (loss=True)  f32 [S, N] V(state) - Q(issued alert) >= 0, exactly 0 where the alert issued is the
                                             expert's
        Along hindsight_posterior_optimum()'s own schedule the expert bits are the schedule and every loss and the
        regret are 0; with n_samples = 1 every output is hindsight_values()'s bit for bit. The result does not depend on
        `sample`. share=True (the default) runs one env of each set that agrees on the problem (the fields
        hindsight_posterior_optimum() shares on) AND on the packed schedule words, and gathers the columns back -- bit
        for bit what share=False returns; last_hindsight_posterior_keys is the number run. A sampled learner's
        schedules differ from env to env, so it shares next to nothing; a deterministic learner's schedule is a function
        of the problem and shares as the optimum does. With allowed_days nothing is shared.
        Sampled and posterior_mean envs alike; refuses what hindsight_posterior_optimum() refuses (corrected-semantics
        fixes, slot-27 tables, a stream capture, an n_samples beyond the kernel's per-draw arrays) before anything is
        written. Reads start_state, the tables and the schedule only: the env's state, observation buffer and
        bookkeeping are untouched. w2a_hindsight_posterior_along (include/w2a.h)."""
        who = "hindsight_posterior_values()"
        self._check_hindsight_fixes(who)
        self._check_hindsight_slot27(who)
        ct, n, dev = self.ct, self.num_envs, self.device
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise _ffi.W2AError(f"{who}: the stream is recording a hipGraph; the call finds the distinct problems and "
                                "sizes its launches on the host")
        mask = _policy.check_schedule(alert_days, "alert_days", n, ct.T, dev, who)
        gate = _policy.check_allowed_days({"kind": "linear", "allowed_days": allowed_days}, n, ct.T, dev, who)
        st = self._hs_start_state(start_state)
        steps = self._hs_steps(n_steps, who, strict=True)
        words = mask.shape[1]
        inv = None
        if share and gate is None and n:
            # the representatives first with their own schedules, the rest marked finished (no DP)
            st, inv, first, m = self._hs_posterior_share(st, mask)
            sched = torch.zeros_like(mask)
            sched[:m] = mask[first]
            mask = sched

        def rows(fill):  # the library writes the first min(steps, T) call-days
            if steps > ct.T:
                return torch.full((steps, n), fill, dtype=torch.float32, device=dev)
            return torch.empty((steps, n), dtype=torch.float32, device=dev)

        gain = rows(float("nan"))
        val = rows(0.0) if value else None
        los = rows(0.0) if loss else None
        expert = torch.empty((n, words), dtype=torch.int32, device=dev)
        regret = torch.empty(n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ws_bytes = self._lib.w2a_hindsight_posterior_workspace_bytes(n, ct.T, ct.n_samples, steps,
                                                                         self._hs_max_remaining(st), _HS_BIG_ENVS)
            # (0 bytes: tables the entry refuses, with its message)
            ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
            v = self._hs_state_view(st)
            _ffi.check(self._lib.w2a_hindsight_posterior_along(
                self._h, C.byref(v), steps, mask.data_ptr(), words, None if gate is None else gate.data_ptr(),
                0 if gate is None else int(gate.shape[1]), gain.data_ptr(), expert.data_ptr(), regret.data_ptr(),
                None if val is None else val.data_ptr(), None if los is None else los.data_ptr(), ws.data_ptr(),
                ws_bytes, self._stream()), "w2a_hindsight_posterior_along")
        self.last_hindsight_posterior_keys = n if inv is None else int(m)
        if inv is not None:  # rows beyond T keep their fill in every column
            gain, expert, regret = gain[:, :m][:, inv], expert[:m][inv], regret[:m][inv]
            val = None if val is None else val[:, :m][:, inv]
            los = None if los is None else los[:, :m][:, inv]
        out = {"alert_gain": gain, "expert_alert_days": _policy.unpack_alert_days(expert, ct.T), "regret": regret}
        if value:
            out["value"] = val
        if loss:
            out["loss"] = los
        return out

    def _hs_posterior_share(self, st: dict, sched=None, unread=()):
        """The distinct problems of the draw-blind DP, found on the host: envs that agree on every _HS_FIELDS array
        but `sample` (a draw outside the tables keeps its own key: its answer is NaN) and, with sched (int32
        [N, words]), on their packed schedule words. unread: further fields the caller's kernel does not read (the
        budget curve's `budget` and `used`). Returns (rep, inv, first, m): rep the state arrays the library
        runs -- num_envs entries, the m representatives (the lowest env id of each key, `first`) in front and the rest
        marked finished (no DP) -- and inv the key of every env, so that x[:m][inv] gathers a per-env output back."""
        n, dev = st["t"].shape[0], st["t"].device
        cols = [st[k] for k in _HS_FIELDS if k != "sample" and k not in unread] + \
               [((st["sample"] < 0) | (st["sample"] >= self.ct.n_samples)).to(torch.int32)]
        key = torch.stack(cols, dim=1)
        if sched is not None:
            key = torch.cat([key, sched.to(torch.int32)], dim=1)
        uniq, inv = torch.unique(key, dim=0, return_inverse=True)
        m = uniq.shape[0]
        first = torch.full((m,), n, dtype=torch.int64, device=dev)
        first.scatter_reduce_(0, inv, torch.arange(n, device=dev), reduce="amin")  # the lowest env id per key
        rep = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in _HS_FIELDS}
        rep["finished"].fill_(1)
        for k in _HS_FIELDS:
            rep[k][:m] = st[k][first]
        return rep, inv, first, m

    def hindsight_budget_curve(self, max_budget: int, start_state: dict | None = None, n_steps: int | None = None,
                               allowed_days=None, schedules: bool = False, packed: bool = False) -> dict:
        """hindsight_optimum() for EVERY remaining budget 0 .. max_budget in one sweep: what one more alert would have
        been worth to each env, and where alerts stop paying -- the return-versus-budget curves that splitting a fixed
        number of alerts over counties needs (stats.budget_curve_by_group, stats.allocate_budget), and the regret of a
        rollout under a sampled budget without a second DP. Column b of env e is the optimum over the env's stretch
        (start_state, n_steps and allowed_days as hindsight_optimum()) from its start day, streak and draw HAD ITS
        REMAINING BUDGET AT THE START BEEN b: hindsight_optimum() of the twin with budget = used + b, bit for bit
        (return, alerts and schedule). The env's own budget is not read. Returns, with B = max_budget,
            "return":     f32 [N, B + 1]  NOT monotone in b in general: the remaining budget enters the reward of
                                          days without an alert too
            "alerts":     i32 [N, B + 1]  alerts in budget b's schedule (<= b)
            "own_budget": i32 [N]         budget - used of start_state: the env's own column where it is in 0 .. B
            "alert_days": (schedules=True) bool [N, B + 1, T] by day of the episode, or with packed=True the kernel's
                                          int32 [N, B + 1, ceil(T / 32)] words
        Envs finished in start_state give rows of 0 and empty schedules; a start outside the tables gives a row of NaN.
        One exact DP over (alerts remaining, streak) per env serves all budgets (w2a_hindsight_curve, include/w2a.h),
        about twice the states of one hindsight_optimum() at budget B and no pruning by day. ValueError for a max_budget
        that is not an int in 0 .. 1023, for schedules of more than 4 GiB (packed words plus, unless packed=True, the
        bool array: ask for fewer envs or budgets per call), and for what hindsight_optimum() refuses. Reads
        start_state and the tables only: the env's state, observation buffer and bookkeeping are untouched."""
        who = "hindsight_budget_curve()"
        self._check_hindsight(who)
        B = self._curve_check(who, max_budget, schedules, packed)
        ct, n, dev = self.ct, self.num_envs, self.device
        gate = _policy.check_allowed_days({"kind": "linear", "allowed_days": allowed_days}, n, ct.T, dev, who)
        st = self._hs_start_state(start_state)
        steps = self._hs_steps(n_steps, who, strict=True)
        with torch.cuda.device(dev):
            ret, alerts, masks = self._curve_packed(st, steps, B, gate, schedules)
        return self._curve_out(ret, alerts, masks, st, schedules, packed)

    def hindsight_posterior_budget_curve(self, max_budget: int, start_state: dict | None = None,
                                         n_steps: int | None = None, allowed_days=None, schedules: bool = False,
                                         packed: bool = False, share: bool = True) -> dict:
        """hindsight_budget_curve() WITH THE DRAW UNKNOWN: hindsight_posterior_optimum() for EVERY remaining budget
        0 .. max_budget in one sweep. Splitting a fixed number of alerts over counties (stats.budget_curve_by_group,
        stats.allocate_budget) is decided before anyone knows which posterior draw a county's episode will get; curves
        under each env's own draw make the allocation chase draw noise and report regret against a bound no policy can
        reach. Column b of env e is hindsight_posterior_optimum() of the twin with budget = used + b, bit for bit
        (return, alerts and schedule), also under allowed_days and a truncated n_steps. The env's own budget is not
        read. Keys, shapes, dtypes and fills are hindsight_budget_curve()'s, with B = max_budget:
            "return":     f32 [N, B + 1]  the posterior-mean return of budget b's schedule (the fp64 sum over its days
                                          of the mean over draws of the f32 rewards, rounded once)
            "alerts":     i32 [N, B + 1]  alerts in budget b's schedule (<= b)
            "own_budget": i32 [N]         budget - used of start_state: the env's own column where it is in 0 .. B
            "alert_days": (schedules=True) bool [N, B + 1, T] by day of the episode, or with packed=True the kernel's
                                          int32 [N, B + 1, ceil(T / 32)] words
        Envs finished in start_state give rows of 0 and empty schedules; a start outside the tables gives a row of NaN.
        hindsight_budget_curve()'s DP over (alerts remaining, streak) with the reward of every state averaged over the
        n_samples draws of the env's coefficient column in fp64, in draw order (w2a_hindsight_posterior_curve,
        include/w2a.h); with n_samples = 1 alerts and schedules are hindsight_budget_curve()'s bit for bit. The result
        depends on neither `sample` nor the env's budget and used: with share=True (the default) envs that agree on t,
        streak, n_days, county_w, year_i, coef_col and finished are found on the host (torch.unique), one of each runs
        and the rows are gathered back -- bit for bit what share=False returns; last_hindsight_posterior_keys is the
        number run. With allowed_days every env has its own gate row and nothing is shared.
        Sampled and posterior_mean envs alike. max_budget, n_steps (an int) and the 4 GiB schedule cap as
        hindsight_budget_curve(); refuses what hindsight_posterior_optimum() refuses (corrected-semantics fixes,
        slot-27 tables, a stream capture, an n_samples beyond the kernel's per-draw arrays: 657 draws at 153 days)
        before anything is written. Reads start_state and the tables only: the env's state, observation buffer and
        bookkeeping are untouched."""
        who = "hindsight_posterior_budget_curve()"
        self._check_hindsight_fixes(who)
        self._check_hindsight_slot27(who)
        B = self._curve_check(who, max_budget, schedules, packed)
        ct, n, dev = self.ct, self.num_envs, self.device
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise _ffi.W2AError(f"{who}: the stream is recording a hipGraph; the call finds the distinct problems and "
                                "sizes its launches on the host")
        gate = _policy.check_allowed_days({"kind": "linear", "allowed_days": allowed_days}, n, ct.T, dev, who)
        st = self._hs_start_state(start_state)
        steps = self._hs_steps(n_steps, who, strict=True)
        with torch.cuda.device(dev):
            if share and gate is None and n:
                # k_hs_pm_curve reads neither budget nor used (rem is B - m - i), so they are not part of the problem
                rep, inv, _, m = self._hs_posterior_share(st, unread=("budget", "used"))
                ret, alerts, masks = self._curve_packed(rep, steps, B, None, schedules, posterior=True)
                ret, alerts = ret[:m][inv], alerts[:m][inv]
                masks = None if masks is None else masks[:m][inv]
                self.last_hindsight_posterior_keys = int(m)
            else:
                ret, alerts, masks = self._curve_packed(st, steps, B, gate, schedules, posterior=True)
                self.last_hindsight_posterior_keys = n
        return self._curve_out(ret, alerts, masks, st, schedules, packed)

    def policy_budget_curve(self, policy: dict, max_budget: int, start_state: dict | None = None,
                            n_steps: int | None = None, schedules: bool = False, packed: bool = False) -> dict:
        """rollout(linear) for EVERY remaining budget 0 .. max_budget in one sweep: what the policy that will actually
        run earns with b alerts -- the policy's row of the budget-curve table whose upper bounds are
        hindsight_budget_curve() (weather and draw known) and hindsight_posterior_budget_curve() (weather known), so
        that stats.budget_curve_by_group / stats.allocate_budget split alerts over counties on what is attainable and
        ``curve_policy / curve_hindsight`` is the regret per budget. Column b of env e is rollout() of the twin env whose
        budget is used + b, bit for bit in return, counts and schedule: the same weather, draw and counters, the same
        Bernoulli uniforms (keyed by seed, env id, episode and day: all budgets share them), require_budget and the gate.
        policy: a ``"kind": "linear"`` dict as rollout() takes it -- weight, bias, group, sample, seed, require_budget
        and "allowed_days" (bool [N, T] or packed words). Returns, with B = max_budget, the keys of
        hindsight_budget_curve() (same names, shapes, dtypes and fills) and one more:
            "return":     f32 [N, B + 1]  rewards summed over the days run
            "alerts":     i32 [N, B + 1]  alerts issued (<= b)
            "attempts_over_budget": i32 [N, B + 1]  attempts with no budget left, as rollout() counts them
            "own_budget": i32 [N]         budget - used of the start state: the env's own column where it is in 0 .. B
            "alert_days": (schedules=True) bool [N, B + 1, T] by day of the episode, or with packed=True the kernel's
                                          int32 [N, B + 1, ceil(T / 32)] words (the 4 GiB cap of hindsight_budget_curve())
        Envs finished in the start state give rows of 0 and empty schedules.
        The reward and the policy read the budget through four run-time slots only, and the fp64 chains run in slot
        order: per env-day the table row is gathered once and the three chains run once over slots 0..23; per budget
        only the tail runs (w2a_policy_curve_linear, include/w2a.h) -- against B + 1 reset(budget=b) + rollout() calls.
        start_state (default: the env's own state) is taken with the checks of hindsight_budget_curve() and goes to
        the kernel the same way, as decoded int32 arrays: the env's packed state is not read. The first decision needs
        the row the agent holds. For the env's own state (start_state None, or a state() dict equal to the current
        state) it is read from the observation buffer, which must be current (RuntimeError as rollout(linear)); column
        b puts float(b) in place of that row's remaining_budget column. For any other start_state the buffer does not
        belong to it, and the call is refused (ValueError) unless every live env of it is at t == 0 with used == 0,
        streak == 0 and an empty 14-day window: there the held row is day 0's table row with lag 0 and streak 0, which
        the kernel rebuilds.
        The call changes nothing: state, observation buffer, statistics and status word stay as they were, and a
        following rollout() sees the same episodes. ValueError, before anything touches a device, for kind "mlp" (a
        later addition: its first layer shares the same way, in a kernel of its own), a "lookahead" key,
        reward_mode="posterior_mean", fixes other than "budget", a max_budget that is not an int in 0..1023,
        n_steps < 1, an env that needs a reset, and whatever rollout(linear) refuses of the policy."""
        who = "policy_budget_curve()"
        kind = policy.get("kind") if isinstance(policy, dict) else None
        if kind == "mlp":
            raise ValueError(f"{who} takes kind 'linear' only; the mlp kind is a later addition (its first layer's "
                             "table-sourced k-steps share the same way, in a kernel of its own)")
        if kind != "linear":
            raise ValueError(f"{who} takes a policy dict of kind 'linear', got {kind!r}")
        if policy.get("lookahead") is not None:
            raise ValueError(f"{who} does not take a 'lookahead' policy: its kernel does not read the lookahead inputs")
        if self._pm:
            raise ValueError(f"{who} needs reward_mode='sampled', not 'posterior_mean'")
        if self.fixes - {"budget"}:
            raise ValueError(f"{who} needs faithful observations; fixes {sorted(self.fixes - {'budget'})} change what "
                             "the observation is")
        B = self._curve_check(who, max_budget, schedules, packed)
        steps = self._hs_steps(n_steps, who, strict=True)
        if self._needs_reset:
            raise ValueError(f"{who}: the env needs a reset(): there is no state to start from")
        ct, n, dev = self.ct, self.num_envs, self.device
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise _ffi.W2AError(f"{who}: the stream is recording a hipGraph; the call compares the start state with "
                                "the env's own on the host")
        gate = _policy.check_allowed_days(policy, n, ct.T, dev, who)
        lin = _check_learned(self, policy)
        own = start_state is None
        if own:
            st = self._state_packed(_PC_FIELDS)[1]
        else:
            st = self._hs_start_state(start_state, _PC_FIELDS)
            cur = self._state_packed(_PC_FIELDS)[1]
            own = all(torch.equal(st[k], cur[k]) for k in _PC_FIELDS)
            if not own:
                live = (st["finished"] == 0) & (st["t"] < st["n_days"])
                fresh = (st["t"] == 0) & (st["used"] == 0) & (st["streak"] == 0) & (st["hist14"] == 0)
                if bool((live & ~fresh).any()):
                    raise ValueError(f"{who}: start_state is not the env's current state, so the observation buffer does "
                                     "not hold its agents' rows; such a start is taken only where every live env is at "
                                     "t == 0 with used == 0 (the held row is then rebuilt from day 0's table row)")
        if own and not self._obs_current:
            raise RuntimeError(f"{who} reads the observation buffer, which does not hold the agents' current rows "
                               "(write_obs=False, a built-in rollout or load_state_dict since the last step()/reset()): "
                               "call step() or reset() first")
        lp = _ffi.LinearPolicy()
        lp.weight, lp.bias = lin.weight_slots.data_ptr(), lin.bias.data_ptr()
        lp.group = None if lin.group is None else lin.group.data_ptr()
        lp.n_groups, lp.sample, lp.require_budget, lp.seed = lin.n_groups, int(lin.sample), int(lin.require_budget), lin.seed
        words = (ct.T + 31) // 32
        ret = torch.empty((n, B + 1), dtype=torch.float32, device=dev)
        alerts = torch.empty((n, B + 1), dtype=torch.int32, device=dev)
        over = torch.empty((n, B + 1), dtype=torch.int32, device=dev)
        masks = torch.empty((n, B + 1, words), dtype=torch.int32, device=dev) if schedules else None
        with torch.cuda.device(dev):
            ws_bytes = self._lib.w2a_policy_curve_workspace_bytes(self._h, steps, B)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            v = _ffi.StateView()
            for k in _PC_FIELDS:
                setattr(v, k, st[k].data_ptr())
            args = (self._h, C.byref(lp), C.byref(v), steps, B, self._obs.data_ptr() if own else None, ret.data_ptr(),
                    alerts.data_ptr(), over.data_ptr(), None if masks is None else masks.data_ptr(), words,
                    ws.data_ptr(), ws_bytes, self._stream())
            if gate is None:
                _ffi.check(self._lib.w2a_policy_curve_linear(*args), "w2a_policy_curve_linear")
            else:
                _ffi.check(self._lib.w2a_policy_curve_linear_gated(*args, gate.data_ptr(), int(gate.shape[1])),
                           "w2a_policy_curve_linear_gated")
        self._keep_curve = (st, gate, ws, lin)  # the launch is asynchronous
        out = self._curve_out(ret, alerts, masks, st, schedules, packed)
        out["attempts_over_budget"] = over
        return out

    def _curve_check(self, who: str, max_budget, schedules: bool, packed: bool) -> int:
        """max_budget as an int in 0 .. 1023 and the byte cap of the schedules"""
        if isinstance(max_budget, bool) or not isinstance(max_budget, (int, np.integer)) or \
                not 0 <= max_budget <= _CURVE_MAX_BUDGET:
            raise ValueError(f"{who}: max_budget must be an int in 0..{_CURVE_MAX_BUDGET}, got {max_budget!r}")
        ct, n = self.ct, self.num_envs
        B = int(max_budget)
        words = (ct.T + 31) // 32
        if schedules:
            need = n * (B + 1) * (4 * words + (0 if packed else ct.T))
            if need > _CURVE_SCHEDULE_BYTES:
                raise ValueError(f"{who}: the schedules of {n} envs x {B + 1} budgets need {need} bytes, more than "
                                 f"{_CURVE_SCHEDULE_BYTES}; ask for fewer envs or budgets per call"
                                 + ("" if packed else ", or packed=True"))
        return B

    def _curve_packed(self, st: dict, steps: int, B: int, gate, schedules: bool, posterior: bool = False):
        """w2a_hindsight_curve (posterior: w2a_hindsight_posterior_curve) on device int32 state arrays: (return f32
        [N, B + 1], alerts i32 [N, B + 1], packed schedules i32 [N, B + 1, words] or None). gate: packed allowed days
        (the _gated entry)."""
        ct, n, dev = self.ct, self.num_envs, self.device
        words = (ct.T + 31) // 32
        ret = torch.empty((n, B + 1), dtype=torch.float32, device=dev)
        alerts = torch.empty((n, B + 1), dtype=torch.int32, device=dev)
        masks = torch.empty((n, B + 1, words), dtype=torch.int32, device=dev) if schedules else None
        name = "w2a_hindsight_posterior_curve" if posterior else "w2a_hindsight_curve"
        ws_bytes = getattr(self._lib, name + "_workspace_bytes")(self._h, steps, B, _HS_BIG_ENVS)
        # (0 bytes, the posterior's answer for tables it cannot take: the entry refuses, with its message)
        ws = torch.empty(max(ws_bytes, 256) if posterior else ws_bytes, dtype=torch.uint8, device=dev)
        v = self._hs_state_view(st)
        args = (self._h, C.byref(v), steps, B, ret.data_ptr(), alerts.data_ptr(),
                None if masks is None else masks.data_ptr(), words, ws.data_ptr(), ws_bytes, self._stream())
        if gate is None:
            _ffi.check(getattr(self._lib, name)(*args), name)
        else:
            _ffi.check(getattr(self._lib, name + "_gated")(*args, gate.data_ptr(), int(gate.shape[1])), name + "_gated")
        self._keep_curve = (st, gate, ws)  # the launches are asynchronous
        return ret, alerts, masks

    def _curve_out(self, ret, alerts, masks, st: dict, schedules: bool, packed: bool) -> dict:
        """the curve calls' dict; own_budget from the caller's (unshared) start state"""
        ct, n = self.ct, self.num_envs
        B, words = ret.shape[1] - 1, (ct.T + 31) // 32
        out = {"return": ret, "alerts": alerts, "own_budget": st["budget"] - st["used"]}
        if schedules:
            out["alert_days"] = masks if packed else \
                _policy.unpack_alert_days(masks.reshape(n * (B + 1), words), ct.T).view(n, B + 1, ct.T)
        return out

    def _check_hindsight(self, who: str):
        self._check_hindsight_fixes(who)
        if self._pm:
            raise ValueError(f"{who} needs reward_mode='sampled', not 'posterior_mean': that env pays the mean over "
                             "draws, so an optimum under the env's own draw is not its yardstick")
        self._check_hindsight_slot27(who)

    def _check_hindsight_fixes(self, who: str):
        if self.fixes - {"budget"}:
            raise ValueError(f"{who} needs faithful semantics; fixes {sorted(self.fixes - {'budget'})} make the reward "
                             "depend on attempts and on the 14-day window")

    def _check_hindsight_slot27(self, who: str):
        dt = self.dtables
        if getattr(dt, "_slot27_zero", None) is None:  # once per table
            dt._slot27_zero = not bool(np.any(np.asarray(self.ct.W).reshape(-1, 2, 32)[:, :, 27] != 0))
        if not dt._slot27_zero:
            raise ValueError(f"{who}: some coefficient row has a nonzero slot-27 (alert_2wks of the agent) term; the "
                             "(alerts, streak) DP is exact only without it")

    def _hs_start_state(self, start_state: dict | None, fields=None) -> dict:
        """start_state (a state() dict; None: the current state) as the int32 [N] device arrays of `fields` (default:
        _HS_FIELDS)"""
        fields = _HS_FIELDS if fields is None else fields
        if start_state is None:
            return self._state_packed(fields)[1]
        n, st = self.num_envs, {}
        for k in fields:
            if k not in start_state:
                raise KeyError(f"start_state lacks {k!r} (pass a state() dict)")
            st[k] = torch.as_tensor(start_state[k], device=self.device).to(torch.int32).contiguous()
            if st[k].shape != (n,):
                raise ValueError(f"start_state[{k!r}] must have shape ({n},)")
        return st

    def _hs_steps(self, n_steps, who: str, strict: bool) -> int:
        """n_steps (None: to the end of every episode) as a positive int; strict refuses what is not an integer
        (hindsight_optimum() and hindsight_posterior_optimum() take what int() takes)"""
        if strict and n_steps is not None and (isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer))):
            raise ValueError(f"{who}: n_steps must be an int, got {n_steps!r}")
        steps = int(n_steps) if n_steps is not None else self.ct.T
        if steps <= 0:
            raise ValueError(f"{who}: n_steps must be positive")
        return steps

    def _hs_max_remaining(self, st: dict) -> int:
        """the largest remaining budget of a live env, as the *_workspace_bytes functions take it: one host reduction
        that sizes the pool of the DPs beyond LDS (none at the tables' default budgets). 0 under a stream capture, which
        the library itself refuses (hindsight_posterior_optimum() has refused it before it gets here)"""
        if not self.num_envs or torch.cuda.is_current_stream_capturing():
            return 0
        live = (st["finished"] == 0) & (st["t"] < st["n_days"])
        return max(0, min(int(torch.where(live, st["budget"] - st["used"], 0).max().item()), 1 << 30))

    @staticmethod
    def _hs_state_view(st: dict):
        v = _ffi.StateView()
        for k in _HS_FIELDS:
            setattr(v, k, st[k].data_ptr())
        return v

    def _hindsight_packed(self, st0: dict, steps: int, gate=None, posterior: bool = False):
        """w2a_hindsight_optimum (posterior: w2a_hindsight_posterior) on device int32 state arrays: (return f32 [N],
        packed bitmap i32 [N, words], alerts i32 [N]). gate: packed allowed days, int32 [N, words] (the _gated entry)."""
        n, dev, ct = self.num_envs, self.device, self.ct
        words = (ct.T + 31) // 32
        ret = torch.empty(n, dtype=torch.float32, device=dev)
        mask = torch.empty((n, words), dtype=torch.int32, device=dev)
        alerts = torch.empty(n, dtype=torch.int32, device=dev)
        rem = self._hs_max_remaining(st0)
        if posterior:
            ws_bytes = self._lib.w2a_hindsight_posterior_workspace_bytes(n, ct.T, ct.n_samples, steps, rem, _HS_BIG_ENVS)
        else:
            ws_bytes = self._lib.w2a_hindsight_workspace_bytes(self._h, steps, rem, _HS_BIG_ENVS)
        # (0 bytes, the posterior's answer for tables it cannot take: the entry refuses, with its message)
        ws = torch.empty(max(ws_bytes, 256) if posterior else ws_bytes, dtype=torch.uint8, device=dev)
        v = self._hs_state_view(st0)
        name = ("w2a_hindsight_posterior" if posterior else "w2a_hindsight_optimum") + ("" if gate is None else "_gated")
        tail = () if gate is None else (gate.data_ptr(), int(gate.shape[1]))
        _ffi.check(getattr(self._lib, name)(self._h, C.byref(v), steps, ret.data_ptr(), mask.data_ptr(), words,
                                            alerts.data_ptr(), ws.data_ptr(), ws_bytes, self._stream(), *tail), name)
        return ret, mask, alerts

    # ------------------------------------------------------------------ alert gate
    def alert_gate(self, feature: str = "heat_qi", threshold=0.8, n_steps: int | None = None,
                   packed: bool = False) -> torch.Tensor:
        """bool [N, T] by day of the episode: the days on which the older reference env's alert restriction
        (``restrict_alerts`` / ``HI_restriction``: an alert attempted while observation[heat_qi] < HI_restriction becomes
        "no alert") lets an alert through -- the "allowed_days" of a kind="linear" or kind="mlp" policy dict and of
        hindsight_optimum(). Bit t of env e is set iff the value of `feature` in the observation row the agent HOLDS
        when it chooses day t's action is >= threshold (>=, as in the reference; the built-in "threshold" kind tests >).
        That row is the one step() would have returned: the table row of day max(t - 1, 0) under the faithful semantics
        (the lagging observation, Q6: days 0 and 1 both see row 0), the row of day t itself with the "obs" fix.
          feature    a table-sourced observation column (KeyError for an unknown name; ValueError for the state-sourced
                     alert_lag1, alerts_streak, remaining_budget and the agent's alert_2wks, with the threshold kind's message)
          threshold  a float, or a float [N] tensor: tau_county[county_of_env] for per-county thresholds, tau_group[group]
                     for a sweep (ValueError for another shape, a non-float tensor or NaN)
          n_steps    days from every env's current day (default: to the end of every episode)
          packed     True: return the kernel's own int32 [N, ceil(T / 32)] words (bit t & 31 of word t >> 5), which
                     "allowed_days" and allowed_days= also take -- nothing is unpacked here or packed again per call
        Covers the days each env would still step from its current state; days before, days past the stretch and
        finished envs are False. Reads the tables with each env's (county, year) and the state; writes nothing but its
        result (w2a_alert_gate, include/w2a.h). Nothing is kept on the env: the mask is an argument of the calls that
        take it, and any other bool [N, T] mask (weekends off, a month window) is as good."""
        if self._needs_reset:
            raise RuntimeError("call reset() before alert_gate()")
        ct, n, dev = self.ct, self.num_envs, self.device
        if feature not in ct.feature_names:
            raise KeyError(feature)
        col = ct.feature_names.index(feature)
        slot = int(_policy.slot_map(ct.obs_slot, ct.n_obs)[col])
        if 24 <= slot <= 27 or ("alert_2wks" in self.fixes and slot == ct.slot_of.get("alerts_2wks", -1)):
            raise ValueError(f"alert_gate(feature={feature!r}): threshold policies read table-sourced columns only")
        if n_steps is not None:
            if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or n_steps <= 0:
                raise ValueError(f"alert_gate(): n_steps must be a positive int, got {n_steps!r}")
        steps = int(n_steps) if n_steps is not None else ct.T
        tau, tau_t = 0.0, None
        if torch.is_tensor(threshold) or isinstance(threshold, np.ndarray):
            tau_t = threshold if torch.is_tensor(threshold) else torch.as_tensor(threshold)
            if not tau_t.is_floating_point() or tuple(tau_t.shape) != (n,):
                raise ValueError(f"alert_gate(): threshold must be a float or a float [{n}] tensor, got "
                                 f"{tuple(tau_t.shape)} {tau_t.dtype}")
            tau_t = tau_t.detach().to(device=dev, dtype=torch.float32).contiguous()
            if bool(torch.isnan(tau_t).any()):
                raise ValueError("alert_gate(): threshold holds NaN")
        else:
            if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) \
                    or np.isnan(threshold):
                raise ValueError(f"alert_gate(): threshold must be a float or a float [{n}] tensor, got {threshold!r}")
            tau = float(threshold)
        words = (ct.T + 31) // 32
        out = torch.empty((n, words), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _ffi.check(self._lib.w2a_alert_gate(self._h, col, tau, None if tau_t is None else tau_t.data_ptr(), steps,
                                                out.data_ptr(), words, self._stream()), "w2a_alert_gate")
        self._keep_gate = tau_t  # the launch is asynchronous
        return out if packed else _policy.unpack_alert_days(out, ct.T)

    def _rollout_posterior_mean(self, p, steps, out, mask, amask, words, snap, st0) -> int:
        """rollout() with reward_mode="posterior_mean": one launch of k_pm_rollout when it applies, else per day
        w2a_policy_actions (the policy and counters of k_rollout), w2a_posterior_mean_reward, w2a_step(REWARD_GIVEN |
        SKIP_FINISHED). Every env is handled on its own day and its own episode length (batches that left lock step
        under autoreset="disabled", ragged episode lengths): envs whose episode is over take no part. Returns the
        number of days run = the most any env had left, capped by `steps`."""
        for k in ("return", "alerts", "attempts_over_budget"):
            out[k].zero_()
        for m in (mask, amask):
            if m is not None:
                m.zero_()
        left = torch.where(st0["finished"].bool(), torch.zeros_like(st0["t"]), st0["n_days"] - st0["t"])
        steps = min(steps, int(left.max()))
        lib, h, stream = self._lib, self._h, self._stream()
        self.last_pm_rollout = "per_day" if steps else None
        if steps and self.pm_rollout_kernel:  # the whole rollout in one launch, when the kernel applies
            rc = lib.w2a_rollout_posterior_mean(h, C.byref(p), steps, out["return"].data_ptr(), out["alerts"].data_ptr(),
                                                out["attempts_over_budget"].data_ptr(),
                                                None if mask is None else mask.data_ptr(),
                                                None if amask is None else amask.data_ptr(), words, self._fr_ptr,
                                                None if snap is None else snap.data_ptr(), stream)
            if rc == 0:
                self.last_pm_rollout = "k_pm_rollout_i8" if self.pm_kernel_choice == "matrix_i8" else "k_pm_rollout"
                return steps
            if rc != 1:
                _ffi.check(rc, "w2a_rollout_posterior_mean")
        act = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        flags = self._step_flags | _ffi.STEP_NO_OBS | _ffi.STEP_SKIP_FINISHED
        nd2 = st0["n_days"] - 2
        for _ in range(steps):
            _ffi.check(lib.w2a_policy_actions(h, C.byref(p), act.data_ptr(), out["alerts"].data_ptr(),
                                              out["attempts_over_budget"].data_ptr(),
                                              None if mask is None else mask.data_ptr(),
                                              None if amask is None else amask.data_ptr(), words, stream),
                       "w2a_policy_actions")
            _ffi.check(lib.w2a_posterior_mean_reward(h, act.data_ptr(), _ffi.ACT_I32, self._rew_ptr, stream),
                       "w2a_posterior_mean_reward")
            # like k_rollout, no observation rows are written (the next step() or reset() brings them up to date);
            # finished envs are skipped: their reward comes back as 0 and their state stays
            _ffi.check(self._w2a_step(h, act.data_ptr(), _ffi.ACT_I32, None, self._rew_ptr, self._done_ptr,
                                      self._fr_ptr, flags, stream), "w2a_step")
            out["return"] += self._reward
            if snap is not None:  # per env: the moment the reference's callbacks read it (t == n_days - 2 after a step)
                st = self.state()
                hit = (st["t"] == nd2) & (st["finished"] == 0) & torch.isnan(snap)
                torch.where(hit, st["episode_return"], snap, out=snap)
        self._keep_act = act
        return steps

    # ------------------------------------------------------------------ statistics (weather2alert_amd/stats.py)
    episode_stats = staticmethod(_stats.episode_stats)
    callback_stats = staticmethod(_stats.callback_stats)
    episode_rows = staticmethod(_stats.episode_rows)
    write_episode_csv = staticmethod(_stats.write_episode_csv)
    CSV_FIELDS = _stats.CSV_FIELDS

    def _coerce_actions(self, actions):
        if not torch.is_tensor(actions):
            actions = torch.as_tensor(np.asarray(actions), device=self.device)
        elif actions.device != self.device:
            actions = actions.to(self.device)
        if actions.dtype not in _ACT_CODES:
            actions = actions.to(torch.int32)
        if actions.numel() != self.num_envs:
            raise ValueError(f"expected {self.num_envs} actions, got {actions.numel()}")
        return actions.contiguous()

    def _info(self):
        return _LazyInfo(self)


# the start-state fields w2a_posterior_returns reads
_PR_FIELDS = ("t", "used", "streak", "hist14", "budget", "n_days", "county_w", "year_i", "coef_col", "finished")
# the start-state fields w2a_hindsight_optimum reads, and how many envs beyond the LDS budget one launch serves
_HS_FIELDS = ("t", "used", "streak", "budget", "n_days", "county_w", "year_i", "coef_col", "sample", "finished")
_HS_BIG_ENVS = 64
# what policy_budget_curve() takes of a start state: the hindsight fields, the 14-day window, the episode number
_PC_FIELDS = _HS_FIELDS + ("hist14", "episode_no")
# hindsight_budget_curve(): the largest max_budget w2a_hindsight_curve takes, and the bytes of schedules one call returns
_CURVE_MAX_BUDGET = 1023
_CURVE_SCHEDULE_BYTES = 4 << 30


def __getattr__(name):  # weather2alert_amd.env.HeatAlertEnv: the drop-in lives in dropin.py (it builds on this module)
    if name == "HeatAlertEnv":
        from .dropin import HeatAlertEnv

        return HeatAlertEnv
    raise AttributeError(name)
