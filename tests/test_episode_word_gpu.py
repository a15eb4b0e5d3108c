"""The lock-step mirror's narrow episode word (csrc/w2a_episode_word.h, w2a_common.hip.h StateArrays): where both row
indices of an episode fit 32 bits together, the packed form of k_step64 streams ONE u32 per env -- coefficient-row index |
day-row index << kw -- instead of the 8-byte word, and the budget travels as the REMAINING budget in the mirror's state
word (8 bits, 255 = escape to the canonical words). 145 B per env-step instead of 149; results must not move.

Every case runs the forced 64-envs-per-wave kernel (step_kernel="wide": small batches reach the packed form) and is
compared two ways:
  * day by day against the float64 oracle: rewards within 1e-5, done flags, integer state and observation rows exact;
  * BIT FOR BIT against the same env on the canonical state words -- step_kernel="wide_unpacked", i.e. what
    step_kernel="unpacked" runs at batch sizes from 131 072 envs (below that "unpacked" is the 4-lanes-per-env kernel, whose
    fp64 additions run in another order): reward, done, obs, state() and final_return.
The host-side rule that picks the form is checked without a GPU (last test: the header compiled on the CPU)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import heatalert_oracle as O
from weather2alert_amd import synth, tables

REWARD_TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "weather2alert_amd", "csrc")
N_DAYS = 5
# the clamp lanes of a ragged wave, whole waves, one env into the next wave / workgroup, and the dense 4-byte array's tails
SIZES = (63, 64, 65, 255, 256, 257, 1023)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world():
    sd = synth.make_synth("linear", n_fips=20, years=[2006, 2007, 2008], n_samples=9, n_days=N_DAYS, seed=53,
                          extra_confounder_fips=3)
    ct = tables.compile_from_synth(sd)
    assert ct.T == N_DAYS
    return sd, ct


def _oracle(sd):
    return O.VectorOracle(O.RefData.from_synth(sd), sd.fips_weather, sd.years)


def _np_state(env):
    return {k: v.cpu().numpy() for k, v in env.state().items()}


def _twin(dev, ct, n, narrow_kw=None, **kw):
    """(the env on the mirror, its twin on the canonical words), both on k_step64"""
    from weather2alert_amd import HeatAlertVecEnv

    A = HeatAlertVecEnv(n, tables=ct, device=dev, step_kernel="wide", **dict(kw, **(narrow_kw or {})))
    B = HeatAlertVecEnv(n, tables=ct, device=dev, step_kernel="wide_unpacked", **kw)
    assert A.step_kernel_name == "k_step64" and B.step_kernel_name == "k_step64"
    return A, B


def _same_state(A, B, what):
    sa, sb = A.state(), B.state()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (k, what)
    return sa


def _ints_equal_oracle(st, V):
    np.testing.assert_array_equal(st["t"], V.t)
    np.testing.assert_array_equal(st["used"], V.used)
    np.testing.assert_array_equal(st["budget"], V.budget)
    np.testing.assert_array_equal(st["streak"], V.streak)
    np.testing.assert_array_equal(st["hist14"], (V.hist * (1 << np.arange(13, -1, -1))).sum(axis=1))


def _step_both(A, B, V, a, what, obs_exact=True, packed="k_step64<packed>"):
    """one day on both envs and the oracle; returns A's outputs and the oracle's reward"""
    at = torch.as_tensor(np.asarray(a, np.int32), device=A.device)
    oa, ra, da, _, ia = A.step(at)
    ob, rb, db, _, ib = B.step(at)
    assert A.last_step_kernel == packed and B.last_step_kernel == "k_step64", what
    assert torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(oa, ob), what
    assert torch.equal(A._final_return, B._final_return), what
    obs_o, r_o, done_o, _ = V.step(np.asarray(a, np.int64))
    err = float(np.abs(ra.cpu().numpy().astype(np.float64) - r_o).max())
    assert err <= REWARD_TOL, (what, err)
    np.testing.assert_array_equal(da.cpu().numpy(), done_o)
    if obs_exact:
        np.testing.assert_array_equal(oa.cpu().numpy(), obs_o.astype(np.float32))
    return oa, ra, da, ia, r_o


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_batch_edges_two_episodes(dev, world, n):
    """Two whole episodes, terminal days included, with the host's reset between them: the re-pack of the new episode's
    words, and -- ten consecutive launches -- both walk directions on every day of an episode."""
    sd, ct = world
    A, B = _twin(dev, ct, n, similar_climate_counties=True, env_gid0=3)
    assert A.episode_word_bytes == 4
    oa, _ = A.reset(seed=5)
    ob, _ = B.reset(seed=5)
    assert torch.equal(oa, ob)
    rng = np.random.default_rng(n)
    V = _oracle(sd)
    for episode in range(2):
        st = _np_state(A)
        assert (st["t"] == 0).all() and (st["episode_no"] == episode).all()
        obs_o = V.reset(st["county_w"], st["year_i"], st["coef_col"], st["sample"], st["budget"])
        np.testing.assert_array_equal(oa.cpu().numpy(), obs_o.astype(np.float32))
        ret = np.zeros(n)
        for t in range(N_DAYS):
            a = (rng.random(n) < 0.5).astype(np.int32)
            # (the terminal step of a lock-step batch returns the next episode's first row: checked above)
            oa, ra, da, ia, r_o = _step_both(A, B, V, a, (n, episode, t), obs_exact=t < N_DAYS - 1)
            ret += r_o
        assert bool(da.all())
        np.testing.assert_allclose(ia["final_return"].cpu().numpy(), ret, rtol=2e-6, atol=2e-5)
    _same_state(A, B, n)
    assert A.check_status() == 0 and B.check_status() == 0
    A.close()
    B.close()


def _budget_episode(dev, sd, ct, n, budgets, T, reset_kw=None):
    """all-ones actions for a whole episode on envs holding `budgets`; remaining_budget and at_budget checked every day"""
    A, B = _twin(dev, ct, n, autoreset="disabled")
    i_rem = ct.feature_names.index("remaining_budget")
    if budgets is not None:
        rng = np.random.default_rng(17)
        county = rng.integers(0, ct.S, n)
        ep = dict(county_w=np.asarray(ct.fips_to_weather)[county], year_i=rng.integers(0, ct.Y, n), coef_col=county,
                  sample=rng.integers(0, ct.n_samples, n), budget=np.asarray(budgets, np.int64)[np.arange(n) % len(budgets)])
        A.reset(seed=1, options={"episodes": ep})
        B.reset(seed=1, options={"episodes": ep})
    else:
        A.reset(**reset_kw)
        B.reset(**reset_kw)
    st = _np_state(A)
    if budgets is not None:
        np.testing.assert_array_equal(st["budget"], ep["budget"])
    V = _oracle(sd)
    V.reset(st["county_w"], st["year_i"], st["coef_col"], st["sample"], st["budget"])
    ones = np.ones(n, np.int32)
    for t in range(T):
        oa, ra, da, ia, _ = _step_both(A, B, V, ones, ("budget", t), obs_exact=t < T - 1)
        if t < T - 1:
            np.testing.assert_array_equal(oa.cpu().numpy()[:, i_rem], (V.budget - V.used).astype(np.float32))
        # info reads the state back (mirror -> canonical words), the next step packs it again
        np.testing.assert_array_equal(ia["at_budget"].cpu().numpy(), V.at_budget)
        np.testing.assert_array_equal(ia["remaining_budget"].cpu().numpy(), V.budget - V.used)
    st = _np_state(A)
    _ints_equal_oracle(st, V)
    np.testing.assert_array_equal(st["used"], np.minimum(st["budget"], T))  # every attempt within budget is granted (Q5)
    _same_state(A, B, "budget")
    assert A.check_status() == 0 and B.check_status() == 0
    A.close()
    B.close()
    return st


@pytest.mark.gpu
def test_budgets_on_both_sides_of_the_escape(dev):
    """Budgets 0, 1, 5 run out under an alert every day; 153 (an always-alert budget) and 254 stay in the 8-bit field for
    the whole episode, 255 and 256 enter through the escape and -- 153 alert days -- leave it on the way down, 1000 never
    does. The episode has the benchmark's 153 days so that 255 and 256 really cross the border."""
    sd = synth.make_synth("linear", n_fips=12, years=[2006, 2007], n_samples=5, n_days=153, seed=59, extra_confounder_fips=2)
    ct = tables.compile_from_synth(sd)
    st = _budget_episode(dev, sd, ct, 257, [0, 1, 5, 153, 254, 255, 256, 1000], 153)
    assert set(np.unique(st["budget"])) == {0, 1, 5, 153, 254, 255, 256, 1000}


@pytest.mark.gpu
def test_sampled_sticky_budget_chain(dev, world):
    """sample_budget with the sticky chain (env.py:167-178, Q9): three episodes, each re-sampling around the last value,
    the large keyword budget putting most envs on the escape."""
    from weather2alert_amd import HeatAlertVecEnv

    sd, ct = world
    n = 257
    kw = dict(tables=ct, device=dev, autoreset="same_step", lockstep=False)
    A = HeatAlertVecEnv(n, step_kernel="wide", **kw)
    B = HeatAlertVecEnv(n, step_kernel="wide_unpacked", **kw)
    opts = {"budget": 250, "sample_budget": True, "sample_budget_type": "centered"}
    oa, _ = A.reset(seed=4, options=opts)
    ob, _ = B.reset(seed=4, options=opts)
    assert torch.equal(oa, ob)
    V = _oracle(sd)
    seen = []
    ones = np.ones(n, np.int32)
    for episode in range(3):
        st = _np_state(A)
        assert (st["t"] == 0).all() and (st["episode_no"] == episode).all()
        seen.append(st["budget"].copy())
        obs_o = V.reset(st["county_w"], st["year_i"], st["coef_col"], st["sample"], st["budget"])
        np.testing.assert_array_equal(oa.cpu().numpy(), obs_o.astype(np.float32))
        for t in range(N_DAYS):
            oa, ra, da, ia, _ = _step_both(A, B, V, ones, ("sticky", episode, t), obs_exact=t < N_DAYS - 1)
            if t == N_DAYS - 2:
                _ints_equal_oracle(_np_state(A), V)
    allb = np.concatenate(seen)
    assert (allb >= 255).any() and (allb < 255).any()  # both sides of the escape were drawn
    assert not np.array_equal(seen[0], seen[1])        # the chain moved
    _same_state(A, B, "sticky")
    assert A.check_status() == 0 and B.check_status() == 0
    A.close()
    B.close()


@pytest.mark.gpu
def test_forced_wide_word_is_bit_identical_to_narrow(dev, world):
    """The 8-byte word is otherwise chosen only for tables too large for a quick test: KernelOptions'
    force_wide_episode_word keeps it on a small table. Narrow, forced wide and the canonical words, side by side."""
    from weather2alert_amd import HeatAlertVecEnv

    sd, ct = world
    n = 257
    A, B = _twin(dev, ct, n, similar_climate_counties=True)
    W = HeatAlertVecEnv(n, tables=ct, device=dev, step_kernel="wide", similar_climate_counties=True, force_wide_episode_word=True)
    assert A.episode_word_bytes == 4 and W.episode_word_bytes == 8
    oa, _ = A.reset(seed=8, options={"budget": 300})
    B.reset(seed=8, options={"budget": 300})
    ow, _ = W.reset(seed=8, options={"budget": 300})
    assert torch.equal(oa, ow)
    st = _np_state(A)
    V = _oracle(sd)
    V.reset(st["county_w"], st["year_i"], st["coef_col"], st["sample"], st["budget"])
    rng = np.random.default_rng(2)
    for t in range(N_DAYS - 1):
        a = (rng.random(n) < 0.5).astype(np.int32)
        oa, ra, da, ia, _ = _step_both(A, B, V, a, ("forced wide", t))
        ow, rw, dw, _, _ = W.step(torch.as_tensor(a, device=dev))
        assert W.last_step_kernel == "k_step64<packed>"
        assert torch.equal(oa, ow) and torch.equal(ra, rw) and torch.equal(da, dw), t
    _same_state(A, W, "forced wide")
    _same_state(A, B, "forced wide")
    for e in (A, B, W):
        assert e.check_status() == 0
        e.close()


@pytest.mark.gpu
def test_bit_boundary_kw_plus_kx_is_32(dev):
    """128 coefficient columns x 1024 draws = 2^17 coefficient rows (kw = 17, the largest index all ones), 128 x 129
    (county, year) pairs = 16 512 day rows (kw + kx = 32 exactly): the last env holds the largest index of both."""
    years = list(range(1900, 2029))
    sd = synth.make_synth("linear", n_fips=128, years=years, n_samples=1024, n_days=3, seed=61)
    ct = tables.compile_from_synth(sd)
    assert ct.S * ct.n_samples == 1 << 17 and 1 << 14 < ct.S_w * ct.Y <= 1 << 15
    n, T = 257, 3
    A, B = _twin(dev, ct, n, autoreset="disabled")
    assert A.episode_word_bytes == 4
    rng = np.random.default_rng(23)
    county = rng.integers(0, ct.S, n)
    f2w = np.asarray(ct.fips_to_weather)
    county[-1] = int(np.flatnonzero(f2w == ct.S_w - 1)[0])
    ep = dict(county_w=f2w[county], year_i=rng.integers(0, ct.Y, n), coef_col=county.copy(),
              sample=rng.integers(0, ct.n_samples, n), budget=rng.integers(0, 4, n))
    ep["year_i"][-1], ep["coef_col"][-1], ep["sample"][-1] = ct.Y - 1, ct.S - 1, ct.n_samples - 1
    assert ep["county_w"][-1] * ct.Y + ep["year_i"][-1] == ct.S_w * ct.Y - 1
    assert ep["coef_col"][-1] * ct.n_samples + ep["sample"][-1] == (1 << 17) - 1
    A.reset(seed=1, options={"episodes": ep})
    B.reset(seed=1, options={"episodes": ep})
    V = _oracle(sd)
    V.reset(ep["county_w"], ep["year_i"], ep["coef_col"], ep["sample"], ep["budget"])
    for t in range(T):
        a = (rng.random(n) < 0.6).astype(np.int32)
        _step_both(A, B, V, a, ("boundary", t), obs_exact=t < T - 1)
    st = _same_state(A, B, "boundary")
    _ints_equal_oracle({k: v.cpu().numpy() for k, v in st.items()}, V)
    assert A.check_status() == 0 and B.check_status() == 0
    A.close()
    B.close()


@pytest.mark.gpu
def test_mid_episode_round_trip(dev, world):
    """state() in the middle of an episode reads the mirror back into the canonical words, the next step packs them again:
    nothing may differ from an env that never left the mirror."""
    from weather2alert_amd import HeatAlertVecEnv

    sd, ct = world
    n = 257
    A, B = _twin(dev, ct, n)
    C_ = HeatAlertVecEnv(n, tables=ct, device=dev, step_kernel="wide")  # never unpacked until the end
    for e in (A, B, C_):
        e.reset(seed=6, options={"budget": 256})  # on the escape at the start of the episode
    st = _np_state(A)
    V = _oracle(sd)
    V.reset(st["county_w"], st["year_i"], st["coef_col"], st["sample"], st["budget"])
    rng = np.random.default_rng(4)
    for t in range(N_DAYS - 1):
        a = (rng.random(n) < 0.7).astype(np.int32)
        oa, ra, da, _, _ = _step_both(A, B, V, a, ("round trip", t))
        oc, rc, dc, _, _ = C_.step(torch.as_tensor(a, device=dev))
        assert torch.equal(oa, oc) and torch.equal(ra, rc) and torch.equal(da, dc), t
        assert A.packed_state and C_.packed_state
        _ints_equal_oracle(_np_state(A), V)  # the unpack
        assert not A.packed_state
    _same_state(A, C_, "round trip")
    _same_state(A, B, "round trip")
    for e in (A, B, C_):
        assert e.check_status() == 0
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("budget", [3, 300])
def test_in_kernel_autoreset_writes_the_narrow_words(dev, world, budget):
    """lockstep=False: the packed kernel's own epilogue draws the next episode and writes its narrow word and its remaining
    budget (300: through the escape). Three episodes without any conversion in between."""
    from weather2alert_amd import HeatAlertVecEnv

    sd, ct = world
    n = 1023
    kw = dict(tables=ct, device=dev, autoreset="same_step", lockstep=False, similar_climate_counties=True)
    A = HeatAlertVecEnv(n, step_kernel="wide", **kw)
    B = HeatAlertVecEnv(n, step_kernel="wide_unpacked", **kw)
    assert A._dev_auto and A.episode_word_bytes == 4
    opts = {"budget": budget, "sample_budget": True}
    A.reset(seed=12, options=opts)
    B.reset(seed=12, options=opts)
    g = torch.Generator(device=dev).manual_seed(budget)
    for k in range(3 * N_DAYS):
        a = (torch.rand(n, device=dev, generator=g) < 0.6).to(torch.int32)
        oa, ra, da, _, _ = A.step(a)
        ob, rb, db, _, _ = B.step(a)
        assert A.last_step_kernel == "k_step64<packed>" and A.packed_state, k
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), k
        assert torch.equal(A._final_return, B._final_return), k
    # the third episode's last-but-one... the batch restarted three times inside the kernel; day by day against the oracle
    st = _np_state(A)
    assert (st["episode_no"] == 3).all() and (st["t"] == 0).all()
    V = _oracle(sd)
    obs_o = V.reset(st["county_w"], st["year_i"], st["coef_col"], st["sample"], st["budget"])
    np.testing.assert_array_equal(oa.cpu().numpy(), obs_o.astype(np.float32))
    rng = np.random.default_rng(budget)
    for t in range(N_DAYS - 1):
        _step_both(A, B, V, (rng.random(n) < 0.6).astype(np.int32), ("autoreset", t))
    _ints_equal_oracle(_np_state(A), V)
    _same_state(A, B, "autoreset")
    assert A.check_status() == 0 and B.check_status() == 0
    A.close()
    B.close()


@pytest.mark.gpu
def test_recorded_block_replayed_twice(dev, world):
    """One hipGraph block of three packed steps, replayed twice (an episode boundary inside), equals six eager steps."""
    from weather2alert_amd import HeatAlertVecEnv

    _, ct = world
    n = 1023
    kw = dict(tables=ct, device=dev, similar_climate_counties=True, lockstep=False, step_kernel="wide")
    A, B = HeatAlertVecEnv(n, **kw), HeatAlertVecEnv(n, **kw)
    oa, _ = A.reset(seed=3, options={"budget": 300, "sample_budget": True})
    ob, _ = B.reset(seed=3, options={"budget": 300, "sample_budget": True})
    assert torch.equal(oa, ob) and A.episode_word_bytes == 4
    g = torch.Generator(device=dev).manual_seed(11)
    acts = [(torch.rand(n, device=dev, generator=g) < 0.6).to(torch.int32) for _ in range(3)]
    A.step(acts[0]); B.step(acts[0])  # (loads the kernels and packs the mirror before the capture)
    assert A.last_step_kernel == "k_step64<packed>"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for a in acts:
            A.step(a)
    for rep in range(2):
        graph.replay()
        for a in acts:
            o, r, d, _, _ = B.step(a)
        torch.cuda.synchronize()
        assert torch.equal(A._obs, o) and torch.equal(A._reward, r) and torch.equal(A._done_bool, d), rep
        assert torch.equal(A._final_return, B._final_return), rep
    sa = _same_state(A, B, "graph")
    assert int(sa["episode_no"].min()) >= 1 and A.check_status() == 0 and B.check_status() == 0
    A.close()
    B.close()


@pytest.mark.gpu
def test_posterior_mean_step_on_a_narrow_handle(dev, world):
    """reward_mode="posterior_mean" reads the canonical words (k_pm_prep) and steps with the reward given: on a handle
    whose mirror is narrow, after sampled-reward days on the mirror of a twin, it must see the same state."""
    from weather2alert_amd import HeatAlertVecEnv

    sd, ct = world
    n = 257
    P = HeatAlertVecEnv(n, tables=ct, device=dev, reward_mode="posterior_mean", pm_kernel="vector", autoreset="disabled")
    assert P.episode_word_bytes == 4
    P.reset(seed=2)
    st = _np_state(P)
    V = O.VectorOracle(O.RefData.from_synth(sd), sd.fips_weather, sd.years, reward_mode="posterior_mean")
    V.reset(st["county_w"], st["year_i"], st["coef_col"], st["sample"], st["budget"])
    a = (np.random.default_rng(1).random(n) < 0.5).astype(np.int32)
    o, r, d, _, _ = P.step(torch.as_tensor(a, device=dev))
    obs_o, r_o, done_o, _ = V.step(a.astype(np.int64))
    assert float(np.abs(r.cpu().numpy().astype(np.float64) - r_o).max()) <= REWARD_TOL
    np.testing.assert_array_equal(o.cpu().numpy(), obs_o.astype(np.float32))
    np.testing.assert_array_equal(d.cpu().numpy(), done_o)
    _ints_equal_oracle(_np_state(P), V)
    assert P.check_status() == 0
    P.close()


RULE_SRC = r"""
#include <stdio.h>
#include "w2a_episode_word.h"
int main() {
  const int dims[][4] = {{746, 100, 746, 11}, {720, 100, 720, 11}, {128, 1024, 128, 129}, {65535, 1024, 63, 1},
                         {65535, 1024, 64, 1}, {65535, 1024, 65, 1}, {1, 1, 1, 1}};
  for (const auto &d : dims) {
    const EpisodeWord w = ew_choose(d[0], d[1], d[2], d[3], false), f = ew_choose(d[0], d[1], d[2], d[3], true);
    printf("%d %d %d %d\n", w.kw, w.kx, w.narrow, f.narrow);
  }
  return 0;
}
"""


def test_eligibility_rule_on_the_host(tmp_path):
    """ew_choose (the header libw2a.so compiles) on the CPU: narrow for the table sizes of configs[2] (746 columns x 100
    draws, 746 x 11 day rows) and configs[3] (720), narrow at kw + kx = 32 exactly, wide at 33, never narrow when forced."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "rule.cpp"
    src.write_text(RULE_SRC)
    exe = str(tmp_path / "rule")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = [tuple(int(x) for x in ln.split()) for ln in subprocess.run([exe], capture_output=True, text=True).stdout.splitlines()]
    assert out[0] == (17, 14, 1, 0)   # configs[2]: 74 600 coefficient rows, 8 206 day rows
    assert out[1] == (17, 13, 1, 0)   # configs[3] / [4]: 72 000, 7 920
    assert out[2] == (17, 15, 1, 0)   # the bit-boundary test's table: 32 bits exactly
    assert out[3] == (26, 6, 1, 0)    # 32 again, the other way round
    assert out[4] == (26, 6, 1, 0)    # 64 day rows still need 6 bits
    assert out[5] == (26, 7, 0, 0)    # 33: the 8-byte word
    assert out[6] == (0, 0, 1, 0)     # one row of each: no bits at all
