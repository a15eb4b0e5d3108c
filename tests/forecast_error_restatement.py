"""The forecast error of policy["lookahead"] = {..., "error": e, "error_seed": s}, restated on the host in NumPy from
include/w2a.h (w2a_forecast_error) alone: the counter-based draws with the oracle's uint64 mix, the one f32 fma done
exactly, and the loops of tests/lookahead_restatement.py run on the noisy inputs (tests/test_forecast_error_cpu.py,
tests/test_forecast_error_gpu.py). Nothing here calls HeatAlertVecEnv.lookahead_features().

    f_k = fmaf(U(r, k), e_k, h(r + k)) - h(r),  k = 1..D,  r = max(t - 1, 0);  +0 where r + k >= n_days;
    h(r + k) as it is where e_k == 0
    U(r, k) = (float)(word >> 8) * 2^-23 - 1,  x = mix64(stream + (8 r + ((k - 1) >> 1) + 1) * GOLD),
    word = x >> 32 for odd k, the low half for even k,  stream = rng_stream(seed ^ NOISE_C, global env id, episode)"""
from unittest import mock

import numpy as np

import lookahead_restatement as LR
from oracle.heatalert_oracle import _mix64_np

NOISE_C = 0xC3C3C3C33C3C3C3C
GOLD = np.uint64(0x9E3779B97F4A7C15)
REFERENCE_MAE = (np.arange(1, 11) * 0.5 + 2).astype(np.float32)  # the reference's profile, for a feature in degrees


def error_row(error, D):
    """f32 [D] from the key's value: one MAE for every lead, or D of them"""
    e = np.asarray(error, np.float32)
    return np.full(D, e, np.float32) if e.ndim == 0 else e.reshape(D)


def stream(seed, gid, episode):
    """uint64 [N]: rng_stream(seed ^ NOISE_C, gid, episode)"""
    with np.errstate(over="ignore"):
        gid, ep = np.asarray(gid, np.uint64), np.asarray(episode, np.uint64)
        h = _mix64_np(np.uint64((seed ^ NOISE_C) & (2**64 - 1)) + GOLD * (gid + np.uint64(1)))
        return _mix64_np(h ^ (ep * np.uint64(0xBF58476D1CE4E5B9) + np.uint64(0x94D049BB133111EB)))


def uniform(st, r, k):
    """f32 U(r, k) in [-1, 1) on the streams st; st, r and k (1-based) broadcast"""
    with np.errstate(over="ignore"):
        r, k = np.asarray(r, np.uint64), np.asarray(k, np.uint64)
        x = _mix64_np(st + (np.uint64(8) * r + ((k - np.uint64(1)) >> np.uint64(1)) + np.uint64(1)) * GOLD)
    word = np.where(k & np.uint64(1), x >> np.uint64(32), x & np.uint64(0xFFFFFFFF))
    return (word >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1)


def fma32(a, b, c):
    """round_f32(a * b + c) with ONE rounding, for f32 arrays: the product is exact in f64, TwoSum gives the f64 sum's
    error, and the f64 -> f32 rounding is corrected where the f64 sum sits exactly halfway between two f32 values while
    the exact sum does not (the only way two roundings can differ from one)"""
    p, c = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64), \
        np.asarray(c, np.float32).astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # p + c == s + err exactly
    r = s.astype(np.float32)
    d = s - r.astype(np.float64)  # exact
    nb = np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    halfway = (d != 0) & (d == nb.astype(np.float64) - s)
    return np.where(halfway & (err != 0) & (np.sign(err) == np.sign(d)), nb, r).astype(np.float32)


def inputs(ct, spec, st, gid0):
    """f32 [N, D] from a host state dict (t, n_days, county_w, year_i and, when it has run episodes before, episode_no)
    of the envs with global ids gid0 .. gid0 + N - 1"""
    D = spec["days"]
    h = LR.series(ct, spec["feature"])
    e = error_row(spec["error"], D)
    row = np.asarray(st["county_w"], np.int64) * ct.Y + np.asarray(st["year_i"], np.int64)
    r = LR.held_day(st["t"])
    nd = np.asarray(st["n_days"], np.int64)
    n = len(r)
    s = stream(spec.get("error_seed", 0), gid0 + np.arange(n), st.get("episode_no", np.zeros(n, np.int64)))
    f = np.zeros((n, D), np.float32)
    for k in range(1, D + 1):
        ok = r + k < nd
        hk = h[row[ok], r[ok] + k]
        if e[k - 1] != 0:
            hk = fma32(uniform(s[ok], r[ok], k), e[k - 1], hk)
        f[ok, k - 1] = hk - h[row[ok], r[ok]]  # f32 - f32, one rounding
    return f


def clean(spec):
    return {k: v for k, v in spec.items() if k in ("feature", "days")}


def _noisy(spec, gid0):
    """lookahead_restatement's loops form their inputs through its module-level inputs(): the same loops, statement for
    statement, on the noisy inputs"""
    return mock.patch.object(LR, "inputs", lambda ct, feature, D, st: inputs(ct, spec, st, gid0))


def twin_loop(env, ct, spec, gid0, logit_fn, n_steps, kind, **kw):
    """lookahead_restatement.twin_loop with a = policy(cat(obs, noisy f))"""
    with _noisy(spec, gid0):
        return LR.twin_loop(env, ct, clean(spec), logit_fn, n_steps, kind, **kw)


def host_walk(V, ct, tup, spec, gid0, logit_fn, n_steps, kind, **kw):
    """lookahead_restatement.host_walk on the noisy inputs (episode 0 of every env)"""
    with _noisy(spec, gid0):
        return LR.host_walk(V, ct, tup, clean(spec), logit_fn, n_steps, kind, **kw)
