"""CPU checks of the returns under every posterior draw: the fp64 restatement against the reference's per-draw rewards
(tests/golden/posterior_draws.npz), the C ABI of w2a_posterior_returns (header, binding, a strict-C caller, host-side
refusals without a GPU), policy.group_mean over K columns, stats.posterior_summary and stats.prob_better."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from weather2alert_amd import _ffi, build, policy, stats, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "w2a.h")
ERR_ARG = -1
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from posterior_restatement import posterior_returns_fp64  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.load()


def fixture_batches():
    """(compiled tables, start-state dict, alert_days [E, T], fixture rows) per data set of posterior_draws.npz."""
    d = dict(np.load(os.path.join(GOLDEN, "posterior_draws.npz")))
    meta = json.loads(str(d["meta_json"]))
    out = []
    for data in ("mini", "mini64"):
        idx = [i for i, e in enumerate(meta["episodes"]) if e["data"] == data]
        ct = tables.CompiledTables.load_npz(os.path.join(GOLDEN, f"{data}_compiled.npz"))
        eps = [meta["episodes"][i]["episode_index"].split("_") for i in idx]
        E = len(idx)
        start = dict(t=np.zeros(E, np.int32), used=np.zeros(E, np.int32), streak=np.zeros(E, np.int32),
                     hist14=np.zeros(E, np.int32), budget=d["budget"][idx], n_days=d["n_days"][idx],
                     county_w=np.asarray([ct.fips_weather.index(f) for f, _ in eps], np.int32),
                     year_i=np.asarray([ct.years.index(int(y)) for _, y in eps], np.int32),
                     coef_col=d["location_index"][idx], finished=np.zeros(E, np.int32))
        out.append((data, ct, start, d["actual"][idx].astype(bool), {k: d[k][idx] for k in d if k != "meta_json"}))
    return out


def test_fixture_covers_the_issue():
    d = dict(np.load(os.path.join(GOLDEN, "posterior_draws.npz")))
    meta = json.loads(str(d["meta_json"]))
    data = [e["data"] for e in meta["episodes"]]
    assert data.count("mini") >= 8 and data.count("mini64") >= 2
    assert os.path.getsize(os.path.join(GOLDEN, "posterior_draws.npz")) < 1 << 20
    resets = [e["reset"] for e in meta["episodes"]]
    assert {r.get("budget") for r in resets} >= {0, 1, 5, None}
    assert any(r.get("similar_climate_counties") or e["ctor"].get("similar_climate_counties")
               for r, e in zip(resets, meta["episodes"]))
    acts = d["actions"]
    assert (acts.sum(1) == 0).any() and (acts.sum(1) == acts.shape[1]).any()
    # some episode hits its budget: attempts beyond it are dropped
    assert ((d["actual"].sum(1) == d["budget"]) & (acts.sum(1) > d["budget"])).any()
    assert set(d["n_samples"][[i for i, x in enumerate(data) if x == "mini"]]) == {8}
    assert set(d["n_samples"][[i for i, x in enumerate(data) if x == "mini64"]]) == {6}


def test_restatement_equals_reference_per_draw_rewards():
    """The fp64 restatement (rows rebuilt from the compiled tables, the start state and the alert bitmap; env.py:197-226
    per draw) equals the unmodified reference with coef_index overwritten, day by day and draw by draw: to 1e-12 on
    tables that are float32-representable (mini). mini64's inputs are float64 values the compiled tables hold as float32
    (CompiledTables.f32_exact is False), so there the bar is the rounding of the inputs: 1e-6 per day."""
    worst = {}
    for data, ct, start, alert_days, d in fixture_batches():
        K = ct.n_samples
        ret, days = posterior_returns_fp64(ct.X, ct.W, K, len(ct.years), start, alert_days, ct.T, per_day=True)
        ref = d["reward"][:, :, :K]
        live = ~np.isnan(ref[:, :, 0])
        assert (live.sum(1) == d["n_days"]).all()
        np.testing.assert_array_equal(np.isnan(days), np.isnan(ref))
        bar = 1e-12 if ct.f32_exact else 1e-6
        assert ct.f32_exact == (data == "mini")
        np.testing.assert_allclose(days[live], ref[live], rtol=0, atol=bar)
        np.testing.assert_allclose(ret, np.nansum(ref, axis=1), rtol=bar, atol=bar * ct.T)
        worst[data] = float(np.nanmax(np.abs(days - ref)))
        # the draws really differ, and the bitmap is the reference's actual_alert_buffer (budget-capped attempts)
        assert (ret.max(1) - ret.min(1) > 1.0).all()
        used = np.cumsum(d["actual"], 1)
        assert (used[:, -1] <= d["budget"]).all()
    print(f"max |restatement - reference| per day and draw: {worst}")


def test_restatement_partial_stretches_add_up():
    """Two stretches (the second from the state the first leaves) sum to the whole episode (fp64 restatement)."""
    data, ct, start, alert_days, d = fixture_batches()[0]
    K, Y = ct.n_samples, len(ct.years)
    whole = posterior_returns_fp64(ct.X, ct.W, K, Y, start, alert_days, ct.T)
    k = 57
    first = posterior_returns_fp64(ct.X, ct.W, K, Y, start, alert_days, k)
    a = alert_days[:, :k].astype(np.int64)
    streak = np.zeros(len(a), np.int64)
    for t in range(k - 1):  # the streak after day t is carried into day t + 1
        streak = np.where(a[:, t] == 1, streak + 1, 0)
    hist = np.zeros(len(a), np.int64)
    for t in range(k):
        hist = ((hist << 1) | a[:, t]) & 0x3FFF
    mid = dict(start, t=np.full(len(a), k, np.int32), used=a.sum(1).astype(np.int32), streak=streak.astype(np.int32),
               hist14=hist.astype(np.int32))
    second = posterior_returns_fp64(ct.X, ct.W, K, Y, mid, alert_days, ct.T)
    np.testing.assert_allclose(first + second, whole, rtol=1e-12, atol=1e-9)
    fin = dict(start, finished=np.ones(len(a), np.int32))
    assert (posterior_returns_fp64(ct.X, ct.W, K, Y, fin, alert_days, ct.T) == 0).all()


# ------------------------------------------------------------------ C ABI
def test_entry_point_declared_exported_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint w2a_posterior_returns\s*\(w2a_env \*env, const w2a_state_view \*start, const uint32_t "
                     r"\*alert_mask,\s*int32_t mask_words,\s*int32_t n_steps, float \*out, void \*stream\);", text)
    assert "w2a_posterior_returns" in _ffi.SYMBOLS and hasattr(lib, "w2a_posterior_returns")
    assert lib.w2a_posterior_returns.restype is C.c_int
    assert len(lib.w2a_posterior_returns.argtypes) == 7
    assert re.search(r"#define W2A_ABI_VERSION 18\b", open(HEADER).read())
    assert lib.w2a_abi_version() == 18


def _view(**null):
    bufs = {k: (C.c_int32 * 4)() for k in _ffi.STATE_FIELDS}
    v = _ffi.StateView()
    for k in _ffi.STATE_FIELDS:
        setattr(v, k, None if k in null else C.addressof(bufs[k]))
    return v, bufs


def test_host_side_refusals_without_gpu(lib):
    v, keep = _view()
    mask = (C.c_uint32 * 32)()
    out = (C.c_float * 32)()

    def call(view=v, m=C.addressof(mask), words=5, steps=3, o=C.addressof(out)):
        return lib.w2a_posterior_returns(None, None if view is None else C.byref(view), m, words, steps, o, None)

    assert call() == ERR_ARG
    assert b"NULL handle" in lib.w2a_last_error()
    assert call(view=None) == ERR_ARG and b"NULL argument" in lib.w2a_last_error()
    assert call(m=None) == ERR_ARG and b"NULL argument" in lib.w2a_last_error()
    assert call(o=None) == ERR_ARG and b"NULL argument" in lib.w2a_last_error()
    for k in ("t", "used", "streak", "hist14", "budget", "n_days", "county_w", "year_i", "coef_col", "finished"):
        vv, kk = _view(**{k: 1})
        assert call(view=vv) == ERR_ARG, k
        assert b"NULL start-state array" in lib.w2a_last_error()
    for k in ("last_actual", "at_budget", "sample", "sticky_budget", "episode_no", "episode_return"):
        vv, kk = _view(**{k: 1})  # not read: past the array checks, refused for the handle
        assert call(view=vv) == ERR_ARG and b"NULL handle" in lib.w2a_last_error(), k
    assert call(steps=0) == ERR_ARG and b"n_steps must be positive" in lib.w2a_last_error()
    assert call(steps=-4) == ERR_ARG and b"n_steps must be positive" in lib.w2a_last_error()
    assert call(words=0) == ERR_ARG and b"mask_words must be positive" in lib.w2a_last_error()


C_PROGRAM = r"""
#include <stdio.h>
#include <stdint.h>
#include "w2a.h"

int main(void) {
  int32_t a[10][1] = {{0}};
  uint32_t mask[5] = {0};
  float out[8];
  w2a_state_view v;
  int rc_handle, rc_steps, rc_null;
  v.t = a[0]; v.used = a[1]; v.streak = a[2]; v.hist14 = a[3]; v.budget = a[4]; v.n_days = a[5];
  v.county_w = a[6]; v.year_i = a[7]; v.coef_col = a[8]; v.finished = a[9];
  v.last_actual = 0; v.at_budget = 0; v.sample = 0; v.sticky_budget = 0; v.episode_no = 0; v.episode_return = 0;
  /* no handle: refused on the host, nothing is launched */
  rc_handle = w2a_posterior_returns(0, &v, mask, 5, 153, out, 0);
  rc_steps = w2a_posterior_returns(0, &v, mask, 5, 0, out, 0);
  rc_null = w2a_posterior_returns(0, 0, mask, 5, 153, out, 0);
  printf("rc=%d,%d,%d\n", rc_handle, rc_steps, rc_null);
  return (rc_handle == W2A_ERR_ARG && rc_steps == W2A_ERR_ARG && rc_null == W2A_ERR_ARG) ? 0 : 1;
}
"""


def test_strict_c_program_calls_entry_point(lib, tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "pr_abi.c"
    src.write_text(C_PROGRAM)
    exe = tmp_path / "pr_abi"
    libdir = os.path.dirname(_ffi.lib_path())
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-L", libdir, "-lw2a", f"-Wl,-rpath,{libdir}", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "rc=-1,-1,-1" in r.stdout


# ------------------------------------------------------------------ group means over K columns, statistics
def test_group_mean_over_k_columns():
    g = torch.Generator().manual_seed(3)
    N, K, G = 1000, 7, 13
    vals = torch.randn(N, K, generator=g, dtype=torch.float64).to(torch.float32) * 100
    grp = torch.randint(0, G - 1, (N,), generator=g)  # group G - 1 has no envs
    got = policy.group_mean(vals, grp, G)
    assert got.shape == (G, K) and got.dtype == torch.float32
    v64 = vals.double().numpy()
    for j in range(G - 1):
        np.testing.assert_allclose(got[j].double().numpy(), v64[grp.numpy() == j].mean(0), rtol=1e-6)
    assert torch.isnan(got[G - 1]).all()
    # column j of the K-column form is the one-column form of column j
    for j in range(K):
        np.testing.assert_array_equal(got[:, j].numpy(), policy.group_mean(vals[:, j].contiguous(), grp, G).numpy())
    one = policy.group_mean(vals, None, 1)
    assert one.shape == (1, K)
    np.testing.assert_allclose(one[0].double().numpy(), v64.mean(0), rtol=1e-6)


def test_posterior_summary_hand_values():
    R = torch.tensor([3.0, 1.0, 2.0, 4.0, 5.0])
    s = stats.posterior_summary(R, probs=(0.0, 0.25, 0.5, 1.0), cvar_alpha=0.3)
    assert float(s["mean"]) == 3.0
    assert abs(float(s["std"]) - np.sqrt(2.0)) < 1e-15
    np.testing.assert_allclose(s["quantiles"].numpy(), [1.0, 2.0, 3.0, 5.0])
    # alpha K = 1.5: the lowest draw fully, the second lowest with weight 0.5 -> (1 + 0.5 * 2) / 1.5
    assert abs(float(s["cvar"]) - 2.0 / 1.5) < 1e-15
    assert abs(float(stats.posterior_summary(R, cvar_alpha=0.4)["cvar"]) - 1.5) < 1e-15  # alpha K = 2 exactly
    assert abs(float(stats.posterior_summary(R, cvar_alpha=1.0)["cvar"]) - 3.0) < 1e-15
    assert abs(float(stats.posterior_summary(R, cvar_alpha=0.1)["cvar"]) - 1.0) < 1e-15  # alpha K = 0.5 < 1
    # draws in the last dimension, leading dims kept; 90 % interval from the 5 / 95 % quantiles
    RR = torch.stack([R, R * 2])
    s2 = stats.posterior_summary(RR)
    assert s2["mean"].shape == (2,) and s2["quantiles"].shape == (3, 2)
    np.testing.assert_allclose(s2["quantiles"][:, 1].numpy(), 2 * np.quantile(R.numpy(), [0.05, 0.5, 0.95]))
    with pytest.raises(ValueError):
        stats.posterior_summary(R, cvar_alpha=0.0)


def test_prob_better_hand_values():
    a = torch.tensor([1.0, 2.0, 3.0, 4.0])
    b = torch.tensor([0.0, 2.0, 5.0, 1.0])
    assert float(stats.prob_better(a, b)) == (1 + 0.5 + 0 + 1) / 4
    assert float(stats.prob_better(b, a)) == (0 + 0.5 + 1 + 0) / 4
    assert float(stats.prob_better(a, a)) == 0.5
    both = stats.prob_better(torch.stack([a, b]), torch.stack([b, b]))
    np.testing.assert_array_equal(both.numpy(), [0.625, 0.5])
    with pytest.raises(ValueError):
        stats.prob_better(a, b[:3])
