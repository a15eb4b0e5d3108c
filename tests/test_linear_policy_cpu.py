"""CPU checks of rollout(kind="linear"): the C ABI of w2a_rollout_linear (struct layout, host-side refusals without a
GPU) and weather2alert_amd/policy.py (argument checks, the observation -> slot permutation, the per-group mean)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from weather2alert_amd import _ffi, build, policy, synth, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.load()


@pytest.fixture(scope="module")
def ct():
    return tables.compile_from_synth(synth.make_synth("linear", n_fips=8, years=[2006, 2007], n_samples=3, seed=2))


def test_linear_policy_struct_matches_header():
    text = open(os.path.join(ROOT, "include", "w2a.h")).read()
    body = re.search(r"typedef struct w2a_linear_policy \{(.*?)\} w2a_linear_policy;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(\w+);", body)
    assert fields == [f for f, _ in _ffi.LinearPolicy._fields_]
    # 3 pointers, 3 int32 (+4 pad before the uint64), 1 uint64
    assert C.sizeof(_ffi.LinearPolicy) == 3 * 8 + 3 * 4 + 4 + 8
    assert _ffi.LinearPolicy.seed.offset == 40
    assert "w2a_rollout_linear" in _ffi.SYMBOLS
    assert _ffi.ROLLOUT_KERNELS[3] == "k_rollout_linear"
    assert re.search(r"3 after\s+\*?\s*w2a_rollout_linear: k_rollout_linear", text)


def test_rollout_linear_refuses_bad_arguments_without_gpu(lib):
    w = (C.c_float * 32)()
    b = (C.c_float * 1)()
    obs = (C.c_float * 29)()

    def call(p, n_steps=10, ob=obs):
        return lib.w2a_rollout_linear(None, None if p is None else C.byref(p), n_steps, C.cast(ob, C.c_void_p) if ob is not None else None,
                                      None, None, None, None, None, 0, None, None, None)

    def pol(**kw):
        p = _ffi.LinearPolicy()
        p.weight, p.bias, p.group, p.n_groups, p.sample, p.require_budget, p.seed = (
            C.cast(w, C.c_void_p), C.cast(b, C.c_void_p), None, 1, 0, 0, 0)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    for p, n, ob, msg in ((None, 10, obs, b"NULL policy"), (pol(), 0, obs, b"n_steps"), (pol(weight=None), 10, obs, b"NULL weight"),
                          (pol(bias=None), 10, obs, b"NULL weight or bias"), (pol(n_groups=0), 10, obs, b"n_groups"),
                          (pol(sample=2), 10, obs, b"sample"), (pol(require_budget=-1), 10, obs, b"require_budget"),
                          (pol(), 10, None, b"NULL obs"), (pol(), 10, obs, b"NULL handle")):
        assert call(p, n, ob) == -1
        assert msg in lib.w2a_last_error(), (msg, lib.w2a_last_error())


def test_slot_permutation_preserves_dot_products(ct):
    """A dot product with the observation row (observation order) equals the dot product of the permuted row with the
    env's 32-slot feature row, on synthetic tables, for every group."""
    rng = np.random.default_rng(0)
    n_obs = ct.n_obs
    s = policy.slot_map(ct.obs_slot, n_obs)
    assert sorted(s.tolist()) == sorted(ct.obs_slot[:n_obs]) and s.max() < policy.LOGIT_SLOTS
    W = rng.standard_normal((7, n_obs)).astype(np.float32)
    Ws = policy.to_slot_order(torch.as_tensor(W), ct.obs_slot, n_obs).numpy()
    assert Ws.shape == (7, 32) and Ws.dtype == np.float32
    others = np.setdiff1d(np.arange(32), s)
    assert (Ws[:, others] == 0).all() and 30 in others and 31 in others
    for _ in range(20):
        obs = rng.standard_normal(n_obs).astype(np.float32)
        row = rng.standard_normal(32).astype(np.float32)  # the feature row: slots outside the observation hold anything
        row[s] = obs
        np.testing.assert_allclose(W.astype(np.float64) @ obs, Ws.astype(np.float64) @ row, rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError):
        policy.slot_map([0, 1, 1], 3)  # not injective
    with pytest.raises(ValueError):
        policy.slot_map([0, 31], 2)  # slot 31 carries the bias


def _ok(n_obs, n, G=3):
    return dict(kind="linear", weight=np.zeros((G, n_obs), np.float32), bias=np.zeros(G, np.float32),
                group=np.arange(n) % G)


def test_linear_policy_argument_checks(ct):
    n_obs, n = ct.n_obs, 10
    a = policy.check_linear_policy(_ok(n_obs, n), n_obs, n, ct.obs_slot, "cpu")
    assert a.n_groups == 3 and a.weight_slots.shape == (3, 32) and a.group.dtype == torch.int32
    assert a.sample is False and a.require_budget is False and a.seed == 0
    a1 = policy.check_linear_policy(dict(kind="linear", weight=np.ones((1, n_obs)), bias=[0.5]), n_obs, n, ct.obs_slot, "cpu")
    assert a1.group is None and a1.bias.dtype == torch.float32
    bad = [
        dict(weight=np.zeros((3, n_obs + 1), np.float32)),          # wrong width
        dict(weight=np.zeros(n_obs, np.float32)),                    # not [G, n_obs]
        dict(bias=np.zeros(2, np.float32)),                          # bias not [G]
        dict(group=np.arange(n + 1) % 3),                            # group not [num_envs]
        dict(group=np.full(n, 3)),                                   # out of range
        dict(group=np.full(n, -1)),                                  # out of range
        dict(group=np.zeros(n, np.float32)),                         # not integer
        dict(group=None),                                            # G > 1 needs groups
        dict(weight=np.full((3, n_obs), np.nan, np.float32)),        # non-finite
        dict(bias=np.array([0, np.inf, 0], np.float32)),             # non-finite
        dict(weight=np.full((3, n_obs), 1e300)),                     # not finite as float32
        dict(sample=1),                                              # not a bool
        dict(seed=1.5),                                              # not an int
        dict(lag=1),                                                 # unknown key
        dict(weight=None),                                           # missing
    ]
    for kw in bad:
        p = {**_ok(n_obs, n), **kw}
        if "group" in kw and kw["group"] is None:
            del p["group"]
        with pytest.raises(ValueError):
            policy.check_linear_policy(p, n_obs, n, ct.obs_slot, "cpu")


def test_group_mean():
    ret = torch.tensor([1.0, 2.0, 3.0, 4.0, 10.0])
    g = torch.tensor([0, 1, 0, 1, 3], dtype=torch.int32)
    m = policy.group_mean(ret, g, 4)
    assert m.dtype == torch.float32 and m.shape == (4,)
    np.testing.assert_allclose(m[[0, 1, 3]].numpy(), [2.0, 3.0, 10.0])
    assert torch.isnan(m[2])  # a group without envs
    np.testing.assert_allclose(policy.group_mean(ret, None, 1).numpy(), [4.0])
    rng = np.random.default_rng(0)
    v, gg = rng.standard_normal(10000).astype(np.float32), rng.integers(0, 37, 10000)
    m = policy.group_mean(torch.as_tensor(v), torch.as_tensor(gg), 40).numpy()
    np.testing.assert_allclose(m[:37], [v[gg == k].astype(np.float64).mean() for k in range(37)], rtol=1e-6, atol=1e-7)
    assert np.isnan(m[37:]).all()
