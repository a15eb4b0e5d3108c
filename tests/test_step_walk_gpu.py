"""k_step64's serpentine walk: consecutive launches of a handle walk every XCD's share of the env tiles in opposite
directions (w2a_step64.hip.h, StepArgs::walk_rev). The direction may change speed only. Here: the forced 64-envs-per-wave
kernel at batch sizes around its workgroup and grid boundaries, stepped for two short episodes so that both directions
run four times each, against the float64 oracle and against the 4-lanes-per-env kernel (which has no direction), and a
recorded block of an odd number of steps whose replays start on the other parity than the eager twin's steps.

Bars (tests/test_env_gpu.py): integer state, done flags and observations bit-exact, rewards within 1e-5 of the oracle and
1e-6 of the other kernel (the order of the fp64 additions), final returns within the suite's return tolerance."""
import numpy as np
import pytest
import torch

from oracle import heatalert_oracle as O
from weather2alert_amd import synth, tables

pytestmark = pytest.mark.gpu

REWARD_TOL = 1e-5
KERNEL_TOL = 1e-6
RETURN_RTOL, RETURN_ATOL = 2e-6, 2e-5
N_DAYS = 4    # days per episode: 8 consecutive steps = two episodes, each direction four times, two terminal days
EPISODES = 2
# 37: a single ragged wave; 2 049: one env past 8 workgroups of 256 envs, so the grid of 16 has padding workgroups;
# 2 111: the same grid with a ragged last wave; 16 385: several workgroups per XCD and a ragged tail
SIZES = (37, 2049, 2111, 16385)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world():
    sd = synth.make_synth("linear", n_fips=20, years=[2006, 2007, 2008], n_samples=9, n_days=N_DAYS, seed=47,
                          extra_confounder_fips=3)
    ct = tables.compile_from_synth(sd)
    assert ct.T == N_DAYS
    return sd, ct


def _ints_equal_oracle(env, V):
    st = {k: v.cpu().numpy() for k, v in env.state().items()}
    np.testing.assert_array_equal(st["t"], V.t)
    np.testing.assert_array_equal(st["used"], V.used)
    np.testing.assert_array_equal(st["streak"], V.streak)
    np.testing.assert_array_equal(st["hist14"], (V.hist * (1 << np.arange(13, -1, -1))).sum(axis=1))
    np.testing.assert_array_equal(st["budget"], V.budget)


def _walk_both_ways(dev, world, n, write_obs, lockstep):
    from weather2alert_amd import HeatAlertVecEnv

    sd, ct = world
    V = O.VectorOracle(O.RefData.from_synth(sd), sd.fips_weather, sd.years)
    kw = dict(tables=ct, device=dev, write_obs=write_obs, similar_climate_counties=True, env_gid0=5, lockstep=lockstep)
    wide, classic = HeatAlertVecEnv(n, step_kernel="wide", **kw), HeatAlertVecEnv(n, step_kernel="classic", **kw)
    assert wide.step_kernel_name == "k_step64" and classic.step_kernel_name == "k_step"
    assert wide._dev_auto == (lockstep is False) and wide._host_auto == (lockstep is not False)
    o1, _ = wide.reset(seed=9)
    o2, _ = classic.reset(seed=9)
    assert torch.equal(o1, o2)
    rng = np.random.default_rng(n)
    worst = 0.0
    for episode in range(EPISODES):
        # the episodes the batch is on (first the reset's, then the ones the autoreset drew) seed the oracle
        st = {k: v.cpu().numpy() for k, v in wide.state().items()}
        assert (st["t"] == 0).all() and (st["episode_no"] == episode).all()
        obs_o = V.reset(st["county_w"], st["year_i"], st["coef_col"], st["sample"], st["budget"])
        if write_obs:  # the row the reset (or the terminal step's autoreset) returned
            np.testing.assert_array_equal(o1.cpu().numpy(), obs_o.astype(np.float32))
        ret = np.zeros(n)
        for t in range(N_DAYS):
            a = (rng.random(n) < 0.4).astype(np.int32)
            at = torch.as_tensor(a, device=dev)
            o1, r1, d1, _, i1 = wide.step(at)
            o2, r2, d2, _, i2 = classic.step(at)
            obs_o, r_o, done_o, _ = V.step(a)
            assert wide.last_step_kernel.startswith("k_step64") and classic.last_step_kernel == "k_step"
            err = float(np.abs(r1.cpu().numpy().astype(np.float64) - r_o).max())
            worst = max(worst, err)
            assert err <= REWARD_TOL, (episode, t, err)
            assert torch.allclose(r1, r2, rtol=0, atol=KERNEL_TOL), (episode, t)
            np.testing.assert_array_equal(d1.cpu().numpy(), done_o)
            assert torch.equal(d1, d2), (episode, t)
            if write_obs:
                assert torch.equal(o1, o2), (episode, t)
                if t < N_DAYS - 1:  # (the terminal step returns the next episode's first row: checked above)
                    np.testing.assert_array_equal(o1.cpu().numpy(), obs_o.astype(np.float32))
            ret += r_o
            if t == N_DAYS - 2:  # integer state once per episode; every other step follows its predecessor directly
                _ints_equal_oracle(wide, V)
                s1, s2 = wide.state(), classic.state()
                for k in s1:
                    if k != "episode_return":
                        assert torch.equal(s1[k], s2[k]), (k, episode, t)
        assert bool(d1.all())
        np.testing.assert_allclose(i1["final_return"].cpu().numpy(), ret, rtol=RETURN_RTOL, atol=RETURN_ATOL)
        np.testing.assert_allclose(i2["final_return"].cpu().numpy(), ret, rtol=RETURN_RTOL, atol=RETURN_ATOL)
    s1, s2 = wide.state(), classic.state()
    for k in s1:
        if k != "episode_return":
            assert torch.equal(s1[k], s2[k]), k
    assert int(s1["episode_no"].min()) == EPISODES and wide.check_status() == 0 and classic.check_status() == 0
    print(f"n={n} write_obs={write_obs} lockstep={lockstep}: max |reward - oracle| = {worst:.3e}")
    wide.close()
    classic.close()


@pytest.mark.parametrize("write_obs", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_walk_directions_across_the_terminal_day_with_the_host_reset(dev, world, n, write_obs):
    """A lock-step batch: the host launches k_reset behind the terminal step, the next step walks the other way."""
    _walk_both_ways(dev, world, n, write_obs, None)


@pytest.mark.parametrize("write_obs", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_walk_directions_with_the_autoreset_inside_the_kernel(dev, world, n, write_obs):
    """lockstep=False: the envs restart in k_step64's epilogue, in whichever direction the terminal step walks."""
    _walk_both_ways(dev, world, n, write_obs, False)


def test_recorded_steps_replay_on_either_parity(dev, world):
    """The direction is a kernel argument, so a recorded launch keeps the one it was recorded with. A block of three steps
    (an odd count) replayed twice walks fwd-rev-fwd twice where six eager steps alternate throughout: every step from the
    fourth on runs in the other direction than its eager twin. Everything must be equal bit for bit."""
    from weather2alert_amd import HeatAlertVecEnv

    _, ct = world
    n = 2111
    kw = dict(tables=ct, device=dev, similar_climate_counties=True, lockstep=False, step_kernel="wide")
    A, B = HeatAlertVecEnv(n, **kw), HeatAlertVecEnv(n, **kw)
    oa, _ = A.reset(seed=3)
    ob, _ = B.reset(seed=3)
    assert torch.equal(oa, ob)
    g = torch.Generator(device=dev).manual_seed(11)
    acts = [(torch.rand(n, device=dev, generator=g) < 0.4).to(torch.int32) for _ in range(3)]
    A.step(acts[0]); B.step(acts[0])  # (loads the kernels before the capture)
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
    sa, sb = A.state(), B.state()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert int(sa["episode_no"].min()) >= 1 and A.check_status() == 0 and B.check_status() == 0
    A.close()
    B.close()
