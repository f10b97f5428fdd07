"""The fused multi-agent steps under snap_start="previous", start_kernel="fast":
pgw_coord_step_prev / _f32 (the agents' kernel, then k_coord_pf_od_prev) on the
coordinated 5-building scenario, and pgw_ma_step's agents followed by
pgw_pf_solve_prev on the heterogeneous one.  Needs an MI355X.

Against the generic path (the agents stepped one by one, pgw_agent_reduce,
pgw_pf_solve_prev, the host's reward transform) every output is demanded bit
for bit; against the chained reference (tests/_pf_prev_common.py) within the
project's bounds for a solve against the oracle.  Cases, seeds and draw order:
tests/_pf_prev_common.py; tests/test_cpu_pf_prev.py asserts their coverage.

A fused step without the history ring writes the coordinated bus only, and --
unlike every history-free route -- cannot restate the other nodes afterwards
(the env's start was overwritten by its own solve): env.voltages of another
node raises there, and the tests that compare every node record the history.
"""
import numpy as np
import pytest
import torch

from tests import _pf_prev_common as C
from tests.test_gpu_configs import close
from tests.test_gpu_f32 import F32_ULP, assert_f32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COMPS = (("building", 0, 6), ("pv", 6, 7), ("storage", 7, 8))
T64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)
BUS = "675.3"


def _env(case, n, fused, max_iter=None, start_kernel="fast", **kw):
    from powergridworld_amd.scenarios.coordinated import CoordinatedMultiBuildingControlEnv
    env = CoordinatedMultiBuildingControlEnv(**C.env_config(case, max_iter, start_kernel), num_envs=n, device=DEV,
                                             fused=fused, **kw)
    ps = env.pf_solver
    assert ps.snap_start == "previous" and ps.warm_start and not ps.od_table
    assert ps._prev_fast == (start_kernel == "fast") and ps.general == (start_kernel == "general")
    if fused and start_kernel == "fast":
        f32 = kw.get("dtype") == torch.float32
        assert env._fused is not None and env._ma is None
        assert env._fused["kernel"] == ("pgw_coord_step_prev_f32" if f32 else "pgw_coord_step_prev")
        assert not env._one_launch_ok() and not env._fused.get("od_on")
    else:
        assert env._fused is None and env._ma is None
    return env


def _start(env, soc):
    env.reset()
    for ai, agent in enumerate(env.agents):
        agent.env_dict["storage"].reset(init_storage=soc[ai])
    env.load_component_state()


def _dict_action(env, a):
    return {ag.name: {c: a[i, :, lo:hi] for c, lo, hi in COMPS} for i, ag in enumerate(env.agents)}


def _generic_obs(env, obs):
    return torch.stack([torch.cat([obs[ag.name][c] for c, _, _ in COMPS], 1) for ag in env.agents])


def _bus(env):
    return env.voltages[BUS]


def _assert_same_step(fused, generic, rf, df, mf, og, rg, dg, mg, tag, nodes):
    """Every per-env output of a fused step against the generic path's, bit for bit."""
    assert torch.equal(fused.packed_obs(), _generic_obs(generic, og)), tag
    for af, ag in zip(fused.agents, generic.agents):
        assert torch.equal(rf[af.name], rg[ag.name]), tag
        assert torch.equal(af.real_power, ag.real_power), tag
    assert torch.equal(mf["voltage_violation"], mg["voltage_violation"]), tag
    assert torch.equal(fused.pf_solver.iterations, generic.pf_solver.iterations), tag
    assert torch.equal(_bus(fused), _bus(generic)), tag
    if nodes:
        for x in generic.pf_solver.feeder.node_names:
            assert torch.equal(fused.voltages[x], generic.voltages[x]), (tag, x)
        for x, y in zip(fused.pf_solver.voltage_extrema(), generic.pf_solver.voltage_extrema()):
            assert torch.equal(x, y), tag
    assert df == dg, tag


# ------------------------------------------------------------------ 1. fused == generic
@pytest.mark.parametrize("hist", [False, True])
@pytest.mark.parametrize("case,n,max_iter", [("std", 1, None), ("std", 65, None), ("std", 257, None),
                                             ("wide", 1, None), ("wide", 65, None), ("wide", 257, None),
                                             ("wide", 257, 3)])
def test_fused_equals_generic_bit_for_bit(case, n, max_iter, hist):
    """MultiAgentEnv(fused=True) against fused=False, both start_kernel="fast",
    12 steps from reset: observations, rewards, voltage_violation, agent powers,
    iteration counts, the coordinated bus, dones -- and, with the history ring
    (the kernel's all-rows path), every node and the extrema.  n = 1 (one lane),
    65 (a wave and a lane), 257 (a block and a lane); wide under max_iter = 3
    has envs the cap stops (negative counts).  On the parent commit the
    constructor refuses the keyword."""
    steps = 12
    soc, act = C.draws(case, n, steps)
    fused = _env(case, n, True, max_iter, record_history=hist)
    generic = _env(case, n, False, max_iter, record_history=hist)
    assert len(fused.pf_solver.output_names) == (fused.pf_solver.feeder.n if hist else 1)
    for env in (fused, generic):
        _start(env, T64(soc))
    counts = set()
    for t in range(steps):
        a = T64(act[t])
        _, rf, df, mf = fused.step(a)
        og, rg, dg, mg = generic.step(_dict_action(generic, a))
        _assert_same_step(fused, generic, rf, df, mf, og, rg, dg, mg, (case, n, t), hist)
        counts |= set(fused.pf_solver.iterations.tolist())
    if max_iter == 3:
        assert counts == {2, 3, -3}
    elif case == "wide" and n == 257:
        assert len(counts) >= 4 and 2 in counts
    if hist:
        vf, pf_, nf = fused.voltage_history()
        vg, pg, ng = generic.voltage_history()
        assert nf == ng and vf.shape == (steps, len(ng), n)
        assert torch.equal(vf, vg) and torch.equal(pf_, pg)


def test_other_nodes_without_the_history_ring_raise():
    """No second solver can restate a step of this route: asking a fused env
    without history for a node it did not write is an error that says so."""
    n = 65
    soc, act = C.draws("std", n, 1)
    env = _env("std", n, True)
    _start(env, T64(soc))
    env.step(T64(act[0]))
    assert env.voltages[BUS].shape == (n,)
    with pytest.raises(RuntimeError, match="record_history=True"):
        env.voltages["650.1"]


# ------------------------------------------------------------------ 2. against the chained reference
@pytest.mark.parametrize("run", ["wide", "wide3", "wide2", "std"])
def test_fused_against_the_chained_reference(run):
    """The fused step against CoordinatedOracle with the chained snap solve
    (PrevPF; the reset solve is a link of the chain on both sides): signed
    iteration counts equal in every env; the coordinated bus voltage within 1e-9
    rel; observations and agent powers under test_gpu_configs.close (1e-12).
    Rewards: reward = raw - vv * VV_UNIT_PENALTY / n_agents with the raw reward
    under close's 1e-12 and vv = max(0, lo - v, v - hi) carrying the voltage's
    error unchanged, |dvv| <= 1e-9 |v|: the bound is
    1e-12 + 1e-12 |reward| + (VV_UNIT_PENALTY / n_agents) 1e-9 |v|."""
    case, n, steps, cap = C.REF_RUNS[run]
    soc, act = C.draws(case, n, steps)
    ref = C.reference(run)
    env = _env(case, n, True, None if cap == 15 else cap)
    _start(env, T64(soc))
    k = env.VV_UNIT_PENALTY / len(env.agents)
    for t in range(steps):
        _, rew, _, meta = env.step(T64(act[t]))
        w = ref[t]
        np.testing.assert_array_equal(env.pf_solver.iterations.cpu().numpy(), w["it"])
        v = _bus(env).cpu().numpy()
        np.testing.assert_allclose(v, w["v"], rtol=1e-9, atol=0)
        close(env.packed_obs(), w["obs"])
        close(torch.stack([a.real_power for a in env.agents]), w["power"])
        r = torch.stack([rew[a.name] for a in env.agents]).cpu().numpy()
        bound = 1e-12 + 1e-12 * np.abs(w["rew"]) + k * 1e-9 * np.abs(w["v"])[None]
        err = np.abs(r - w["rew"])
        assert (err <= bound).all(), (t, float((err / bound).max()))
        np.testing.assert_allclose(meta["voltage_violation"].cpu().numpy(), w["vv"], rtol=0,
                                   atol=1e-9 * float(np.abs(w["v"]).max()))


def test_every_node_against_the_chained_reference():
    """With the history ring the fused step writes every node: each within 1e-9
    rel of the reference's."""
    case, n, steps, cap = C.REF_RUNS["wide"]
    soc, act = C.draws(case, n, steps)
    env = _env(case, n, True, record_history=True)
    _start(env, T64(soc))
    names = env.pf_solver.feeder.node_names
    for t in range(steps):
        env.step(T64(act[t]))
        pu = torch.stack([env.voltages[x] for x in names], 1).cpu().numpy()
        np.testing.assert_allclose(pu, C.reference("wide")[t]["pu"], rtol=1e-9, atol=0)


# ------------------------------------------------------------------ 3. the chain and the episode
def test_chain_continues_across_reset_as_on_the_default_route():
    """reset() does not restart the chain (the reference compiles one circuit,
    once): two episodes' first steps on the fused fast route equal the generic
    path on the default route (start_kernel="general") in counts and within
    1e-11 rel at the bus (a restart on one side alone moves the bus by ~1e-8) --
    and the second episode's bits differ from the first's, which started from
    the direct solution."""
    n, steps = 65, 4
    soc, act = C.draws("wide", n, steps)
    f, g = _env("wide", n, True), _env("wide", n, False, start_kernel="general")
    first = []
    for episode in range(2):
        for env in (f, g):
            _start(env, T64(soc))
        for t in range(steps):
            a = T64(act[t])
            f.step(a)
            g.step(_dict_action(g, a))
            assert torch.equal(f.pf_solver.iterations, g.pf_solver.iterations), (episode, t)
            vf, vg = _bus(f).cpu().numpy(), _bus(g).cpu().numpy()
            np.testing.assert_allclose(vf, vg, rtol=1e-11, atol=0)
            if episode == 0:
                first.append(vf.copy())
            elif t == 0:
                # (a chain restarted at reset() would repeat the first episode's bits)
                assert not np.array_equal(vf, first[0])


# ------------------------------------------------------------------ 4. fp32 storage
@pytest.mark.parametrize("case,n", [("std", 130), ("wide", 130), ("wide", 129)])
def test_f32_storage(case, n):
    """dtype=float32 (n = 129 is odd: no env pairs), 12 steps.  Teacher-forced as
    tests/test_gpu_f32.py: with the fp32 state copied into an fp64 fused env
    before each step, every agent output is the fp64 step's rounded once.  The
    fp32 step's solve reads the stored (rounded) agent powers, so it is held to
    the fp64 stand-alone entry on those powers, 0 + p0 + p1 ..., run on a copy
    of the env's state buffer taken before the step: equal counts, the stored
    voltage and violation that solve's rounded once, the extrema buffers and the
    state buffer after the step the fp64 values themselves.  Rewards as
    tests/test_gpu_coord_h1.py::test_f32_storage bounds them:
    |r32 - r64| <= 2^-23 (|r64| + share64) + k |v - v_teacher|."""
    from powergridworld_amd import _lib
    steps = 12
    soc, act = C.draws(case, n, steps)
    e32, e64 = _env(case, n, True, dtype=torch.float32), _env(case, n, True)
    soc32 = T64(soc).float().double()
    _start(e32, soc32)
    _start(e64, soc32)
    F32, F64 = e32._fused, e64._fused
    lo, hi = e32.VOLTAGE_LIMITS
    s32 = e32.pf_solver
    v64 = torch.zeros((1, n), dtype=torch.float64, device=DEV)
    it64 = torch.zeros(n, dtype=torch.int32, device=DEV)
    for t in range(steps):
        F64["x"].copy_(F32["x"])
        F64["soc"].copy_(F32["soc"])
        e64.pf_solver._prev_U.copy_(s32._prev_U)             # (the two chains differ by the powers' rounding)
        U = s32._prev_U.clone()
        a = T64(act[t]).float()
        _, r32, d32, m32 = e32.step(a)
        _, r64, d64, m64 = e64.step(a.double())
        assert_f32(e32.packed_obs(), e64.packed_obs(), ulps=0)
        assert_f32(F32["x"], F64["x"], ulps=0)
        assert_f32(F32["soc"], F64["soc"], ulps=0)
        assert_f32(F32["agent_power"], F64["agent_power"], ulps=0)
        P = torch.zeros(n, dtype=torch.float64, device=DEV)
        for ai in range(len(e32.agents)):
            P = P + F32["agent_power"][ai].double()
        vmin, vmax = s32._vmin.clone(), s32._vmax.clone()
        pfp, pft = s32.step_params(e32.time), s32.step_tables(e32.time)
        _lib.check(_lib.lib().pgw_pf_solve_prev(pfp, pft, U.data_ptr(), n, P.data_ptr(), None, v64.data_ptr(),
                                                it64.data_ptr(), _lib.stream_ptr(s32.device)))
        torch.cuda.synchronize()
        assert torch.equal(F32["iters"], it64), t
        assert torch.equal(F32["v_out"][0], v64[0].float()) and torch.equal(U, s32._prev_U)
        vv64 = torch.maximum(torch.maximum(torch.zeros_like(v64[0]), lo - v64[0]), v64[0] - hi)
        assert torch.equal(m32["voltage_violation"], vv64.float())
        assert vmin.dtype == torch.float64 and torch.equal(vmin, v64[0]) and torch.equal(vmax, v64[0])
        k = e32.VV_UNIT_PENALTY / len(e32.agents)
        dshare = k * (v64[0] - F64["v_out"][0]).abs() * (1 + 1e-9) + 1e-12
        for ag in e32.agents:
            r = r64[ag.name]
            tol = F32_ULP * (r.abs() + k * m64["voltage_violation"]) + dshare
            err = (r32[ag.name].double() - r).abs()
            assert r32[ag.name].dtype == torch.float32 and bool((err <= tol).all()), (t, float((err / tol).max()))
        assert d32 == d64


# ------------------------------------------------------------------ 5. graph, checkpoint
def test_capture_step_equals_eager_across_an_episode_boundary():
    """capture_step(actions, steps=4) on wide, n = 65: replayed before and
    after a reset, against eager stepping, bit for bit -- the captured launches
    read and write the state buffer as the eager ones do."""
    n = 65
    soc, act = C.draws("wide", n, 8)
    ea, eg = _env("wide", n, True), _env("wide", n, True)
    bufs = [torch.empty((5, n, 8), dtype=torch.float64, device=DEV) for _ in range(4)]
    g = eg.capture_step(bufs, steps=4)
    for episode in range(2):
        for env in (ea, eg):
            _start(env, T64(soc))
        for call in range(2):
            for i in range(4):
                a = T64(act[4 * call + i])
                bufs[i].copy_(a)
                o, r, d, m = ea.step(a)
            og, rg, dg, mg = g()
            assert torch.equal(ea.packed_obs(), eg.packed_obs())
            for x, y in zip(ea.agents, eg.agents):
                assert torch.equal(r[x.name], rg[y.name]) and torch.equal(x.real_power, y.real_power)
            assert torch.equal(m["voltage_violation"], mg["voltage_violation"])
            assert torch.equal(ea.pf_solver.iterations, eg.pf_solver.iterations)
            assert torch.equal(_bus(ea), _bus(eg))
            assert torch.equal(ea.pf_solver._prev_U, eg.pf_solver._prev_U)
            assert d == dg and ea.episode_step == eg.episode_step == 4 * (call + 1)
    g.release()


def test_checkpoint_round_trip_restores_the_state_buffer():
    """state_dict() / load_state_dict() on the fused route, wide, n = 65: saved
    after 280 steps, then 20 more (the episode ends and the env resets among
    them) three times -- on the env itself, on it again after a rewind, and on a
    fresh env loaded from the checkpoint (whose own chain is at the direct
    solution until the load) -- every output bit for bit, which needs U."""
    n = 65
    soc, act = C.draws("wide", n, 12)

    def step(env, t):
        _, rew, d, meta = env.step(T64(act[t % 12]))
        out = [env.packed_obs().clone(), torch.stack([rew[a.name] for a in env.agents]),
               torch.stack([a.real_power for a in env.agents]), meta["voltage_violation"].clone(),
               env.pf_solver.iterations.clone(), _bus(env).clone(), env.pf_solver._prev_U.clone(),
               torch.tensor(float(d["__all__"]))]
        if d["__all__"]:
            env.reset()
        return out

    env = _env("wide", n, True)
    _start(env, T64(soc))
    for t in range(280):
        step(env, t)
    assert env.episode_step == 280
    sd = env.state_dict()
    assert any(k.endswith("_prev_U") for k in sd)
    ref = [step(env, t) for t in range(280, 300)]
    assert any(bool(x[-1]) for x in ref)                 # the episode boundary lies in the replayed steps
    env.load_state_dict(sd)
    again = [step(env, t) for t in range(280, 300)]
    fresh = _env("wide", n, True)
    fresh.reset()
    assert not torch.equal(fresh.pf_solver._prev_U, sd[[k for k in sd if k.endswith("_prev_U")][0]])
    fresh.load_state_dict(sd)
    other = [step(fresh, t) for t in range(280, 300)]
    for t, (x, y, z) in enumerate(zip(ref, again, other)):
        for i, (u, v, w) in enumerate(zip(x, y, z)):
            assert torch.equal(u, v), "rewound env, step %d output %d" % (t, i)
            assert torch.equal(u, w), "fresh env, step %d output %d" % (t, i)


# ------------------------------------------------------------------ 6. the heterogeneous scenario
def _het_cfg(**pf):
    from powergridworld_amd.scenarios.heterogeneous import make_env_config
    cfg = make_env_config()
    cfg["pf_config"]["config"].update(dict(snap_start="previous"), **pf)
    return cfg


def _het_act(a):
    return {"building": {"building": a[:, :6], "pv": a[:, 6:7], "storage": a[:, 7:8]},
            "pv": a[:, 8:9], "ev-charging": a[:, 9:10]}


def _flat(o):
    return torch.cat([o["building"]["building"], o["building"]["pv"], o["building"]["storage"],
                      o["pv"], o["ev-charging"]], 1)


@pytest.mark.parametrize("hist", [False, True])
def test_het_fused_equals_generic(hist):
    """The heterogeneous scenario with start_kernel="fast", 256 envs, 12 steps
    from reset: the fused multi-agent step (pgw_ma_step's agents, then
    pgw_pf_solve_prev on the bus loads) equals the generic path bit for bit --
    observations (the PV farm's holds the previous solve's minimum voltage),
    rewards, extrema, iteration counts, and with the history ring every node."""
    from powergridworld_amd import _lib
    from powergridworld_amd.multiagent_env import MultiAgentEnv
    n, steps = 256, 12
    envs = [MultiAgentEnv(**_het_cfg(start_kernel="fast"), num_envs=n, device=DEV, fused=f, record_history=hist)
            for f in (True, False)]
    assert envs[0]._ma is not None and envs[0]._fused is None and envs[1]._ma is None
    assert envs[0]._ma["prev"] is _lib.lib().pgw_pf_solve_prev and envs[0]._ma["h1"] is None
    for env in envs:
        ps = env.pf_solver
        assert ps._prev_fast and not ps.general and list(ps._ctrl_names) == ["675c"]
    rng = np.random.default_rng(9)
    soc0 = torch.tensor(rng.uniform(5.0, 240.0, size=n), device=DEV)
    for env in envs:
        env.reset()
        env.agent_dict["building"].env_dict["storage"].reset(init_storage=soc0)
    nodes = envs[0].pf_solver.feeder.node_names
    counts = set()
    for k in range(steps):
        a = torch.tensor(rng.uniform(-1.1, 1.1, (n, 10)), device=DEV)
        (o0, r0, d0, _), (o1, r1, d1, _) = [env.step(_het_act(a)) for env in envs]
        assert torch.equal(_flat(o0), _flat(o1)), k
        for nm in ("building", "pv", "ev-charging"):
            assert torch.equal(r0[nm], r1[nm]), (k, nm)
        assert d0 == d1
        e0, e1 = envs[0].pf_solver.voltage_extrema(), envs[1].pf_solver.voltage_extrema()
        assert torch.equal(e0[0], e1[0]) and torch.equal(e0[1], e1[1]), k
        assert torch.equal(envs[0].pf_solver.iterations, envs[1].pf_solver.iterations), k
        assert torch.equal(envs[0].pf_solver._prev_U, envs[1].pf_solver._prev_U), k
        if hist:
            for x in nodes:
                assert torch.equal(envs[0].voltages[x], envs[1].voltages[x]), (k, x)
        counts |= set(envs[0].pf_solver.iterations.tolist())
    assert min(counts) >= 2 and max(counts) <= 15


# ------------------------------------------------------------------ 7. route selection
def test_default_start_kernel_keeps_the_refusals_and_the_generic_path():
    """start_kernel="general" (the default): both fused paths refuse with the
    texts they had, the solver runs the general kernel, the generic path steps;
    RegControls and yprim="step" are not this route's."""
    from powergridworld_amd.multiagent_env import MultiAgentEnv
    from powergridworld_amd.scenarios.coordinated import CoordinatedMultiBuildingControlEnv
    text = "snap_start='previous' (each env's solve starts from its own previous solution)"
    cfg = C.env_config("std")
    cfg["pf_config"]["config"].pop("start_kernel")
    env = CoordinatedMultiBuildingControlEnv(**cfg, num_envs=64, device=DEV)
    ps = env.pf_solver
    assert env._fused is None and env._ma is None and env._fusable() == text and env._ma_fusable() == text
    assert ps.general and ps.warm_start and not ps.od_table and not ps._prev_fast and ps.start_kernel == "general"
    with pytest.raises(Exception, match="snap_start='previous'"):
        CoordinatedMultiBuildingControlEnv(**cfg, num_envs=64, device=DEV, fused=True)
    het = MultiAgentEnv(**_het_cfg(), num_envs=64, device=DEV)
    assert het._ma is None and het._ma_fusable() == text
    fast = _env("std", 64, True)
    assert fast._fusable() is None
    # the keyword is ignored unless snap_start="previous"
    cfg = C.env_config("std")
    cfg["pf_config"]["config"]["snap_start"] = "direct"
    d = CoordinatedMultiBuildingControlEnv(**cfg, num_envs=64, device=DEV, fused=True)
    assert d._fused["kernel"] == "pgw_coord_step" and not d.pf_solver._prev_fast and d.pf_solver.od_table
    # agents on two buses: the fused step refuses, the solver falls back to the general kernel
    cfg = _het_cfg(start_kernel="fast")
    cfg["agents"][0]["bus"] = "684c"
    two = MultiAgentEnv(**cfg, num_envs=64, device=DEV)
    assert two._ma is None and two._fused is None and two._ma_fusable() == text
    two.reset()
    two.step(_het_act(torch.zeros((64, 10), dtype=torch.float64, device=DEV)))
    assert two.pf_solver.general and not two.pf_solver._prev_fast
    assert bool(((two.pf_solver.iterations >= 2) & (two.pf_solver.iterations <= 15)).all())
