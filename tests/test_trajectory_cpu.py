"""CPU checks of rollout(record=True): the C ABI of w2a_rollout_linear_record / w2a_rollout_mlp_record (header and
binding, struct layout, a strict-C caller, host-side refusals without a GPU) and policy.action_log_prob."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from weather2alert_amd import _ffi, build, policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "w2a.h")
ERR_ARG = -1  # W2A_ERR_ARG (checked against the header below)


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.load()


def _header():
    return open(HEADER).read()


def test_record_symbols_and_flags_match_header(lib):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for sym in ("w2a_rollout_linear_record", "w2a_rollout_mlp_record"):
        assert re.search(r"\b" + sym + r"\s*\(", text), sym
        assert sym in _ffi.SYMBOLS and hasattr(lib, sym)
        assert re.fullmatch(r"w2a_[a-z_]+", sym)
    for name, val in (("W2A_TRAJ_VALID", _ffi.TRAJ_VALID), ("W2A_TRAJ_TERMINATED", _ffi.TRAJ_TERMINATED),
                      ("W2A_TRAJ_ALERT", _ffi.TRAJ_ALERT)):
        m = re.search(r"\b" + name + r"\s*=\s*(\d+)", text)
        assert m and int(m.group(1)) == val, name
    assert {_ffi.TRAJ_VALID, _ffi.TRAJ_TERMINATED, _ffi.TRAJ_ALERT} == {1, 2, 4}
    # the record forms take the plain form's arguments plus the trajectory
    assert lib.w2a_rollout_linear_record.argtypes[:-1] == lib.w2a_rollout_linear.argtypes
    assert lib.w2a_rollout_mlp_record.argtypes[:-1] == lib.w2a_rollout_mlp.argtypes
    assert re.search(r"#define W2A_ABI_VERSION 18\b", _header())
    assert int(re.search(r"\bW2A_ERR_ARG\s*=\s*(-?\d+)", text).group(1)) == ERR_ARG


def test_trajectory_struct_matches_header():
    body = re.search(r"typedef struct w2a_trajectory \{(.*?)\} w2a_trajectory;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+);", body) == [f for f, _ in _ffi.Trajectory._fields_]
    assert C.sizeof(_ffi.Trajectory) == 5 * C.sizeof(C.c_void_p)
    assert [getattr(_ffi.Trajectory, f).offset for f, _ in _ffi.Trajectory._fields_] == [0, 8, 16, 24, 32]


C_PROGRAM = r"""
#include <stdio.h>
#include <stdint.h>
#include "w2a.h"

int main(void) {
  float obs[2 * 29], logit[1], reward[1], params[4];
  uint8_t action[1], flags[1];
  float weight[32] = {0}, bias[1] = {0};
  w2a_trajectory tr;
  w2a_linear_policy lp;
  w2a_mlp_policy mp;
  int rc_lin, rc_mlp, rc_null;
  tr.obs = obs; tr.logit = logit; tr.reward = reward; tr.action = action; tr.flags = flags;
  lp.weight = weight; lp.bias = bias; lp.group = 0; lp.n_groups = 1; lp.sample = 0; lp.require_budget = 0; lp.seed = 0;
  mp.params = params; mp.group = 0; mp.order = 0; mp.n_groups = 1; mp.n_layers = 1; mp.width = 16;
  mp.activation = W2A_MLP_TANH; mp.sample = 0; mp.require_budget = 0; mp.seed = 0;
  /* no handle: refused on the host, nothing is launched */
  rc_lin = w2a_rollout_linear_record(0, &lp, 1, obs, 0, 0, 0, 0, 0, 0, 0, 0, 0, &tr);
  rc_mlp = w2a_rollout_mlp_record(0, &mp, 1, obs, 0, 0, 0, 0, 0, 0, 0, 0, 0, &tr);
  rc_null = w2a_rollout_linear_record(0, &lp, 1, obs, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);
  printf("sizeof(w2a_trajectory)=%u rc=%d,%d,%d flags=%d,%d,%d\n", (unsigned)sizeof(w2a_trajectory), rc_lin, rc_mlp,
         rc_null, W2A_TRAJ_VALID, W2A_TRAJ_TERMINATED, W2A_TRAJ_ALERT);
  return (rc_lin == W2A_ERR_ARG && rc_mlp == W2A_ERR_ARG && rc_null == W2A_ERR_ARG) ? 0 : 1;
}
"""


def test_strict_c_program_calls_record_entry_points(lib, tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "traj_abi.c"
    src.write_text(C_PROGRAM)
    exe = tmp_path / "traj_abi"
    libdir = os.path.dirname(_ffi.lib_path())
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-L", libdir, "-lw2a", f"-Wl,-rpath,{libdir}", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert f"sizeof(w2a_trajectory)={C.sizeof(_ffi.Trajectory)}" in r.stdout
    assert "flags=1,2,4" in r.stdout


def _aligned(n):
    buf = (C.c_float * (n + 4))()
    return buf, (C.addressof(buf) + 15) // 16 * 16


@pytest.mark.parametrize("kind", ["linear", "mlp"])
def test_record_refusals_without_gpu(lib, kind):
    keep, aligned = _aligned(policy.mlp_stride(16, 1))
    obs = (C.c_float * (2 * 29))()
    small = (C.c_float * 4)()
    bytes_ = (C.c_uint8 * 4)()
    if kind == "linear":
        p = _ffi.LinearPolicy()
        p.weight, p.bias, p.group, p.n_groups, p.sample, p.require_budget, p.seed = aligned, C.addressof(small), None, 1, 0, 0, 0
        fn = lib.w2a_rollout_linear_record
    else:
        p = _ffi.MlpPolicy()
        p.params, p.group, p.order, p.n_groups, p.n_layers, p.width, p.activation = aligned, None, None, 1, 1, 16, 0
        p.sample, p.require_budget, p.seed = 0, 0, 0
        fn = lib.w2a_rollout_mlp_record

    def traj(**kw):
        t = _ffi.Trajectory(C.addressof(obs), C.addressof(small), C.addressof(small), C.addressof(bytes_),
                            C.addressof(bytes_))
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def call(pp, t, n_steps=1):
        return fn(None, None if pp is None else C.byref(pp), n_steps, C.addressof(obs), None, None, None, None, None, 0,
                  None, None, None, None if t is None else C.byref(t))

    assert call(p, traj()) == ERR_ARG  # NULL handle
    assert b"NULL handle" in lib.w2a_last_error()
    assert call(p, None) == ERR_ARG  # NULL trajectory
    assert b"NULL trajectory" in lib.w2a_last_error()
    for field, _ in _ffi.Trajectory._fields_:
        assert call(p, traj(**{field: None})) == ERR_ARG, field
        assert b"NULL trajectory array" in lib.w2a_last_error()
    # where the plain form refuses, so does the record form
    assert call(None, traj()) == ERR_ARG
    assert call(p, traj(), n_steps=0) == ERR_ARG
    assert b"n_steps must be positive" in lib.w2a_last_error()
    p.sample = 2
    assert call(p, traj()) == ERR_ARG
    assert b"sample must be 0 or 1" in lib.w2a_last_error()


def test_action_log_prob_matches_fp64():
    z = np.array([-100.0, -30.0, -5.0, -1.0, -1e-3, 0.0, 1e-3, 0.5, 2.0, 17.0, 100.0], np.float64)
    for a in (0, 1):
        act = np.full(z.shape, a)
        ref = np.where(act == 1, -np.logaddexp(0.0, -z), -np.logaddexp(0.0, z))
        got = policy.action_log_prob(torch.tensor(z, dtype=torch.float32), torch.tensor(act, dtype=torch.uint8))
        assert got.dtype == torch.float32 and torch.isfinite(got).all()
        np.testing.assert_allclose(got.double().numpy(), ref, rtol=1e-6, atol=1e-7)
        got64 = policy.action_log_prob(torch.tensor(z), torch.tensor(act, dtype=torch.bool))
        np.testing.assert_allclose(got64.numpy(), ref, rtol=1e-12, atol=1e-300)
    # |logit| = 100: exact tails, no overflow to -inf or nan
    lp = policy.action_log_prob(torch.tensor([100.0, -100.0]), torch.tensor([0, 1]))
    assert torch.allclose(lp, torch.tensor([-100.0, -100.0]))
    # probabilities of the two actions sum to 1, and it is differentiable
    zt = torch.linspace(-8, 8, 33, dtype=torch.float64, requires_grad=True)
    p1, p0 = policy.action_log_prob(zt, 1).exp(), policy.action_log_prob(zt, 0).exp()
    assert torch.allclose(p1 + p0, torch.ones_like(p1))
    assert torch.allclose(p1, torch.sigmoid(zt))
    policy.action_log_prob(zt, torch.ones(33)).sum().backward()
    assert torch.allclose(zt.grad, 1 - torch.sigmoid(zt.detach()))


def test_action_log_prob_is_sb3_two_way_categorical():
    g = torch.Generator().manual_seed(0)
    rows = torch.randn(64, 2, generator=g, dtype=torch.float64) * 4
    a = torch.randint(0, 2, (64,), generator=g)
    ref = torch.distributions.Categorical(logits=rows).log_prob(a)
    got = policy.action_log_prob(rows[:, 1] - rows[:, 0], a)
    assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)
