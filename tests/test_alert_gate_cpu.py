"""Alert gates without a GPU: the validation and packing of "allowed_days", and the restatement
(tests/alert_gate_restatement.py) on the inputs the GPU tests use -- so the references are known to stay inside the
conditions the GPU tests rely on (allowed share, lag, word boundaries, gated attempts with budget left)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alert_gate_restatement as G  # noqa: E402

from weather2alert_amd import policy  # noqa: E402

CPU = torch.device("cpu")


def test_allowed_days_validation():
    n, T = 5, 70
    ok = torch.ones((n, T), dtype=torch.bool)
    assert policy.check_allowed_days({"kind": "linear"}, n, T, CPU, "rollout()") is None
    assert policy.check_allowed_days({"kind": "linear", "allowed_days": None}, n, T, CPU, "rollout()") is None
    assert policy.check_allowed_days({"kind": "linear", "allowed_days": ok}, n, T, CPU, "rollout()").shape == (n, 3)
    assert policy.check_allowed_days({"kind": "linear", "allowed_days": ok.numpy()}, n, T, CPU, "x").dtype == torch.int32
    for bad in (ok.to(torch.uint8), ok.float(), ok.to(torch.int32)):
        with pytest.raises(ValueError, match="allowed_days must be bool"):
            policy.check_allowed_days({"kind": "linear", "allowed_days": bad}, n, T, CPU, "rollout()")
    for bad in (ok[:, :-1], ok[:-1], ok[0], ok.T, torch.ones((n, 96), dtype=torch.bool)):
        with pytest.raises(ValueError, match="allowed_days must be bool \\[5, 70\\]"):
            policy.check_allowed_days({"kind": "linear", "allowed_days": bad}, n, T, CPU, "rollout()")
    for kind in ("never", "always", "bernoulli", "threshold", "table", None):
        with pytest.raises(ValueError, match="'allowed_days' is taken by kind"):
            policy.check_allowed_days({"kind": kind, "allowed_days": ok}, n, T, CPU, "rollout()")
    assert policy.check_allowed_days({"kind": "never", "allowed_days": None}, n, T, CPU, "rollout()") is None  # absent
    assert policy.check_allowed_days({"kind": "mlp", "allowed_days": ok}, n, T, CPU, "rollout()").shape == (n, 3)
    packed = policy.pack_alert_days(ok, 3)  # already packed: taken as it is
    assert policy.check_allowed_days({"kind": "mlp", "allowed_days": packed}, n, T, CPU, "x") is packed
    with pytest.raises(ValueError, match="allowed_days must be bool"):
        policy.check_allowed_days({"kind": "linear", "allowed_days": packed[:, :2]}, n, T, CPU, "x")
    # the key passes both kinds' own checks
    W, b = np.zeros((1, 4), np.float32), np.zeros(1, np.float32)
    policy.check_linear_policy(dict(kind="linear", weight=W, bias=b, allowed_days=ok), 4, n, [0, 1, 2, 3], CPU)
    policy.check_mlp_policy(dict(kind="mlp", layers=[(np.zeros((3, 4)), np.zeros(3)), (np.zeros((1, 3)), np.zeros(1))],
                                 allowed_days=ok), 4, n, [0, 1, 2, 3], CPU)


@pytest.mark.parametrize("T", [1, 31, 32, 33, 64, 153])
def test_packing_round_trip(T):
    rng = np.random.default_rng(T)
    days = rng.random((7, T)) < 0.5
    days[0] = True   # bit 31 of every whole word set: the int32 word is negative
    days[1] = False
    if T >= 32:
        days[2] = False
        days[2, 31] = True  # bit 31 alone: -2^31
    words = policy.pack_alert_days(torch.as_tensor(days), (T + 31) // 32)
    assert words.dtype == torch.int32 and words.shape == (7, (T + 31) // 32)
    np.testing.assert_array_equal(words.numpy().view(np.uint32), G.pack_words(days))
    if T >= 32:
        assert int(words[2, 0]) == -2**31
    assert torch.equal(policy.unpack_alert_days(words, T), torch.as_tensor(days))
    np.testing.assert_array_equal(G.unpack_words(words.numpy(), T), days)
    gate = policy.check_allowed_days({"kind": "linear", "allowed_days": torch.as_tensor(days)}, 7, T, CPU, "x")
    assert torch.equal(gate, words)


@pytest.mark.parametrize("name", ["synth", "ragged"])
def test_restatement_on_the_gpu_tests_inputs(name):
    ct = G.make_tables(name)
    case = G.make_case(ct)
    assert len(case["tau"]) == G.N_ENVS == 257 and set(case["group"]) == {0, 2}
    allowed = G.check_case(ct, case)
    st = case["start"]
    # n_steps < T, a mid-episode start and finished envs
    mid = dict(st, t=np.minimum(st["t"] + 40, st["n_days"] - 1), finished=(np.arange(G.N_ENVS) % 5 == 0).astype(np.int64))
    part = G.gate_fp32(ct.X, ct.Y, case["slot"], mid, case["tau"], n_steps=30)
    assert not part[mid["finished"] != 0].any()
    cols = np.arange(ct.T)[None, :]
    inside = (cols >= mid["t"][:, None]) & (cols < np.minimum(mid["t"] + 30, mid["n_days"])[:, None]) & (mid["finished"] == 0)[:, None]
    np.testing.assert_array_equal(part, allowed & inside)
    # the "obs" fix: day t sees row t, so the faithful gate is this one shifted by a day (day 0 apart)
    fixed = G.gate_fp32(ct.X, ct.Y, case["slot"], st, case["tau"], lag=False)
    live = cols < st["n_days"][:, None]
    np.testing.assert_array_equal(allowed[:, 1:], fixed[:, :-1] & live[:, 1:])
    np.testing.assert_array_equal(allowed[:, 0], fixed[:, 0])
    # an all-ones gate forces nothing but what require_budget forces; an all-zero gate issues nothing
    ones, zeros = np.ones_like(allowed), np.zeros_like(allowed)
    a = G.gated_walk(case["sched"], ones, st["t"], st["used"], st["budget"], st["n_days"], st["finished"], ct.T)
    assert not a["forced"].any() and a["over"].any()
    z = G.gated_walk(case["sched"], zeros, st["t"], st["used"], st["budget"], st["n_days"], st["finished"], ct.T)
    assert not z["attempt"].any() and not z["over"].any() and (z["forced"] == z["valid"]).all()
