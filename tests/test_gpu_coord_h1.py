"""The fused C4 step under yprim="step" (H1): pgw_coord_step_h1 / _f32 -- the
agents' kernel, then k_coord_pf_od_h1 (k_pf_solve_od_h1's solve between the
coordinated prologue and epilogue).  Needs an MI355X.

Against the generic path (five agents stepped one by one, pgw_agent_reduce,
pgw_pf_solve_h1, the host's reward transform) every output is demanded bit
for bit; against the H1 reference (tests/_coord_h1_common.py) within the
project's bounds for a solve against the oracle.  Cases, seeds and draw order:
tests/_coord_h1_common.py; tests/test_cpu_coord_h1.py asserts their coverage.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import _coord_h1_common as C
from tests.test_gpu_configs import close
from tests.test_gpu_f32 import F32_ULP, assert_f32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COMPS = (("building", 0, 6), ("pv", 6, 7), ("storage", 7, 8))
T64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64, device=DEV)


def _env(case, n, fused, max_iter=None, **kw):
    from powergridworld_amd.scenarios.coordinated import CoordinatedMultiBuildingControlEnv
    env = CoordinatedMultiBuildingControlEnv(**C.env_config(case, max_iter), num_envs=n, device=DEV, fused=fused, **kw)
    assert env.pf_solver.yprim == "step" and env.pf_solver._h1_fast and not env.pf_solver.general
    if fused:
        f32 = kw.get("dtype") == torch.float32
        assert env._fused is not None and env._ma is None
        assert env._fused["kernel"] == ("pgw_coord_step_h1_f32" if f32 else "pgw_coord_step_h1")
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


def _all_nodes(env):
    v = env.pf_solver.get_bus_voltages()
    return torch.stack([v[x] for x in env.pf_solver.feeder.node_names])


def _assert_same_step(fused, generic, of, rf, df, mf, og, rg, dg, mg, tag):
    """Every per-env output of a fused step against the generic path's, bit for bit."""
    assert torch.equal(fused.packed_obs(), _generic_obs(generic, og)), tag
    for af, ag in zip(fused.agents, generic.agents):
        assert torch.equal(rf[af.name], rg[ag.name]), tag
        assert torch.equal(af.real_power, ag.real_power), tag
    assert torch.equal(mf["voltage_violation"], mg["voltage_violation"]), tag
    assert torch.equal(fused.pf_solver.iterations, generic.pf_solver.iterations), tag
    assert torch.equal(_all_nodes(fused), _all_nodes(generic)), tag
    for x, y in zip(fused.pf_solver.voltage_extrema(), generic.pf_solver.voltage_extrema()):
        assert torch.equal(x, y), tag
    assert df == dg, tag


# ------------------------------------------------------------------ 1. fused == generic
@pytest.mark.parametrize("case,n,max_iter", [("std", 1, None), ("std", 65, None), ("std", 257, None),
                                             ("wide", 1, None), ("wide", 65, None), ("wide", 257, None),
                                             ("wide", 257, 3)])
def test_fused_equals_generic_bit_for_bit(case, n, max_iter):
    """MultiAgentEnv(fused=True) against fused=False, both step_kernel="fast", 12
    steps from reset: observations, rewards, voltage_violation, agent powers,
    iteration counts, extrema, every node, dones.  n = 1 (one lane), 65 (a wave
    and a lane), 257 (a block and a lane); wide under max_iter = 3 has envs the
    cap stops (negative counts).  On the parent commit fused=True raises."""
    steps = 12
    soc, act = C.draws(case, n, steps)
    fused, generic = _env(case, n, True, max_iter), _env(case, n, False, max_iter)
    for env in (fused, generic):
        _start(env, T64(soc))
    counts = set()
    for t in range(steps):
        a = T64(act[t])
        of, rf, df, mf = fused.step(a)
        og, rg, dg, mg = generic.step(_dict_action(generic, a))
        _assert_same_step(fused, generic, of, rf, df, mf, og, rg, dg, mg, (case, n, t))
        counts |= set(fused.pf_solver.iterations.tolist())
    if max_iter == 3:
        assert counts == {3, -3}
    elif case == "wide" and n == 257:
        assert len(counts) >= 3 and min(counts) > 0


# ------------------------------------------------------------------ 2. against the H1 reference
@pytest.mark.parametrize("run", ["wide", "wide3", "std"])
def test_fused_against_the_h1_reference(run):
    """The fused step against CoordinatedOracle with the H1 snap solve: signed
    iteration counts equal in every env (every decision is >= 1e-8 pu from the
    threshold, test_cpu_coord_h1.py); the coordinated bus voltage within 1e-9
    rel, the project's figure for a solve against the oracle; observations and
    agent powers under test_gpu_configs.close (1e-12).
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
        v = env.pf_solver.get_bus_voltage_by_name("675c").cpu().numpy()
        np.testing.assert_allclose(v, w["v"], rtol=1e-9, atol=0)
        close(env.packed_obs(), w["obs"])
        close(torch.stack([a.real_power for a in env.agents]), w["power"])
        r = torch.stack([rew[a.name] for a in env.agents]).cpu().numpy()
        bound = 1e-12 + 1e-12 * np.abs(w["rew"]) + k * 1e-9 * np.abs(w["v"])[None]
        err = np.abs(r - w["rew"])
        assert (err <= bound).all(), (t, float((err / bound).max()))
        np.testing.assert_allclose(meta["voltage_violation"].cpu().numpy(), w["vv"], rtol=0,
                                   atol=1e-9 * float(np.abs(w["v"]).max()))


# ------------------------------------------------------------------ 3. H1 is not H2
def test_h1_is_not_h2():
    """The coordinated bus under yprim="step" differs from the yprim="dss_file"
    fused step without its table by more than 1e-7 pu somewhere: a route that
    ran k_coord_pf_od would pass the bit-for-bit test against nothing."""
    from powergridworld_amd.scenarios.coordinated import CoordinatedMultiBuildingControlEnv
    n, steps = 65, 4
    soc, act = C.draws("wide", n, steps)
    h1 = _env("wide", n, True)
    cfg = C.env_config("wide")
    cfg["pf_config"]["config"].update(yprim="dss_file", od_table=False)
    cfg["pf_config"]["config"].pop("step_kernel")
    h2 = CoordinatedMultiBuildingControlEnv(**cfg, num_envs=n, device=DEV, fused=True)
    assert h2._fused["kernel"] == "pgw_coord_step"
    worst = 0.0
    for env in (h1, h2):
        _start(env, T64(soc))
    for t in range(steps):
        for env in (h1, h2):
            env.step(T64(act[t]))
        d = (h1.pf_solver.get_bus_voltage_by_name("675c") - h2.pf_solver.get_bus_voltage_by_name("675c")).abs()
        worst = max(worst, float(d.max()))
        assert torch.equal(torch.stack([a.real_power for a in h1.agents]),
                           torch.stack([a.real_power for a in h2.agents]))
    assert worst > 1e-7, worst


# ------------------------------------------------------------------ 4. history
def test_history_ring_and_lazy_voltages():
    """record_history=True at n = 65, wide: every node of every ring slot (the
    kernel's rows_lds path writes them all) equals the generic path's ring bit
    for bit, and so do the lazy env.voltages of a fused env without history."""
    n, steps = 65, 6
    soc, act = C.draws("wide", n, steps)
    fh = _env("wide", n, True, record_history=True)
    gh = _env("wide", n, False, record_history=True)
    lazy = _env("wide", n, True)
    assert len(fh.pf_solver.output_names) == fh.pf_solver.feeder.n and len(lazy.pf_solver.output_names) == 1
    for env in (fh, gh, lazy):
        _start(env, T64(soc))
    for t in range(steps):
        a = T64(act[t])
        fh.step(a)
        lazy.step(a)
        gh.step(_dict_action(gh, a))
        names = gh.pf_solver.feeder.node_names
        assert list(lazy.voltages) == list(names)
        for x in names:
            assert torch.equal(lazy.voltages[x], gh.voltages[x]), (t, x)
            assert torch.equal(fh.voltages[x], gh.voltages[x]), (t, x)
        assert torch.equal(fh.pf_solver.iterations, gh.pf_solver.iterations)
    vf, pf_, nf = fh.voltage_history()
    vg, pg, ng = gh.voltage_history()
    assert nf == ng and vf.shape == (steps, len(ng), n)
    assert torch.equal(vf, vg) and torch.equal(pf_, pg)


# ------------------------------------------------------------------ 5. fp32 storage
@pytest.mark.parametrize("case,n", [("std", 130), ("wide", 130), ("std", 129), ("wide", 129)])
def test_f32_storage(case, n):
    """dtype=float32 (n = 129 is odd: no env pairs), 12 steps.  Teacher-forced as
    tests/test_gpu_f32.py: with the fp32 state copied into an fp64 fused H1 env
    before each step, every agent output is the fp64 step's rounded once.  The
    fp32 step's solve reads the stored (rounded) agent powers, so its outputs
    are held to the fp64 solve OF THOSE POWERS, pgw_pf_solve_h1 on 0 + p0 + p1
    ... (the env's own on-demand solve of every node): equal iteration counts,
    the stored voltage and violation that solve's rounded once, and the
    solver's extrema buffers the fp64 value itself.
    Rewards against the teacher-forced fp64 env: r32 = RN32(RN32(raw) +
    RN32(-share)) with raw the fp64 env's raw reward and share = k vv, k =
    VV_UNIT_PENALTY / n_agents, of the solve of the STORED powers, while the
    fp64 env's share comes from its unrounded powers.  Three roundings of at
    most 2^-24 relative on |raw| <= |r| + share, share and |r|, plus the two
    shares' difference, at most k |v - v_teacher| (vv is 1-Lipschitz in v):
    |r32 - r64| <= 2^-23 (|r64| + share64) + k |v - v_teacher|, both voltages
    fp64 solves the test reads (at 1200 kW per battery the powers' fp32
    rounding moves the bus load by ~1e-4 kW and the share by ~5e-6)."""
    steps = 12
    soc, act = C.draws(case, n, steps)
    e32, e64 = _env(case, n, True, dtype=torch.float32), _env(case, n, True)
    soc32 = T64(soc).float().double()
    _start(e32, soc32)
    _start(e64, soc32)
    F32, F64 = e32._fused, e64._fused
    lo, hi = e32.VOLTAGE_LIMITS
    for t in range(steps):
        F64["x"].copy_(F32["x"])
        F64["soc"].copy_(F32["soc"])
        a = T64(act[t]).float()
        _, r32, d32, m32 = e32.step(a)
        _, r64, d64, m64 = e64.step(a.double())
        assert_f32(e32.packed_obs(), e64.packed_obs(), ulps=0)
        assert_f32(F32["x"], F64["x"], ulps=0)
        assert_f32(F32["soc"], F64["soc"], ulps=0)
        assert_f32(F32["agent_power"], F64["agent_power"], ulps=0)
        # the fp64 H1 solve of the stored powers
        full = e32._full_voltages(e32._fused_steps)
        solver = e32._pf_full
        v64 = solver.v_out[solver.output_names.index("675.3")]
        assert torch.equal(F32["iters"], solver.iterations), t
        assert torch.equal(F32["iters"], F64["iters"]), t            # and the teacher-forced fp64 step's
        assert torch.equal(F32["v_out"][0], v64.float()) and torch.equal(full["675.3"], v64.float())
        vv64 = torch.maximum(torch.maximum(torch.zeros_like(v64), lo - v64), v64 - hi)
        assert torch.equal(m32["voltage_violation"], vv64.float())
        assert e32.pf_solver._vmin.dtype == torch.float64
        assert torch.equal(e32.pf_solver._vmin, v64) and torch.equal(e32.pf_solver._vmax, v64)
        k = e32.VV_UNIT_PENALTY / len(e32.agents)
        dshare = k * (v64 - F64["v_out"][0]).abs() * (1 + 1e-9) + 1e-12
        for ag in e32.agents:
            r = r64[ag.name]
            tol = F32_ULP * (r.abs() + k * m64["voltage_violation"]) + dshare
            err = (r32[ag.name].double() - r).abs()
            assert r32[ag.name].dtype == torch.float32 and bool((err <= tol).all()), (t, float((err / tol).max()))
        assert d32 == d64


# ------------------------------------------------------------------ 6. graph
def test_capture_step_equals_eager_across_an_episode_boundary():
    """capture_step(actions, steps=4) on wide, n = 65: replayed before and
    after a reset, against eager stepping, bit for bit."""
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
            assert torch.equal(_all_nodes(ea), _all_nodes(eg))
            assert d == dg and ea.episode_step == eg.episode_step == 4 * (call + 1)
    g.release()


def test_checkpoint_round_trip_across_an_episode_boundary():
    """state_dict() / load_state_dict() on the H1 fused route, wide, n = 65:
    saved after 280 steps, then 20 more (the episode ends and the env resets
    among them) three times -- on the env itself, on it again after a rewind,
    and on a fresh env loaded from the checkpoint -- every output bit for bit."""
    n = 65
    soc, act = C.draws("wide", n, 12)

    def step(env, t):
        _, rew, d, meta = env.step(T64(act[t % 12]))
        out = [env.packed_obs().clone(), torch.stack([rew[a.name] for a in env.agents]),
               torch.stack([a.real_power for a in env.agents]), meta["voltage_violation"].clone(),
               env.pf_solver.iterations.clone(), _all_nodes(env), torch.tensor(float(d["__all__"]))]
        if d["__all__"]:
            env.reset()
        return out

    env = _env("wide", n, True)
    _start(env, T64(soc))
    for t in range(280):
        step(env, t)
    assert env.episode_step == 280
    sd = env.state_dict()
    ref = [step(env, t) for t in range(280, 300)]
    assert any(bool(x[-1]) for x in ref)                 # the episode boundary lies in the replayed steps
    env.load_state_dict(sd)
    again = [step(env, t) for t in range(280, 300)]
    fresh = _env("wide", n, True)
    fresh.reset()
    fresh.load_state_dict(sd)
    other = [step(fresh, t) for t in range(280, 300)]
    for t, (x, y, z) in enumerate(zip(ref, again, other)):
        for i, (u, v, w) in enumerate(zip(x, y, z)):
            assert torch.equal(u, v), "rewound env, step %d output %d" % (t, i)
            assert torch.equal(u, w), "fresh env, step %d output %d" % (t, i)


# ------------------------------------------------------------------ 7. the C ABI directly
GUARD = 64
SENT = -12345.5


class _Guarded:
    """A sentinel-filled device buffer of `size` elements with GUARD sentinel
    elements on either side."""

    def __init__(self, size, dtype=torch.float64):
        self.size = size
        self.sent = -77 if dtype == torch.int32 else SENT
        self.t = torch.full((size + 2 * GUARD,), self.sent, dtype=dtype, device=DEV)
        self.ptr = self.t.data_ptr() + GUARD * self.t.element_size()

    @property
    def inner(self):
        return self.t[GUARD:GUARD + self.size]

    def guards_intact(self):
        return bool((self.t[:GUARD] == self.sent).all() and (self.t[GUARD + self.size:] == self.sent).all())

    def untouched(self):
        return bool((self.t == self.sent).all())


def _direct_setup(n, dtype=torch.float64):
    """A started std env, its first step's constants and a copy of its launch
    buffers whose five outputs are guarded buffers (of the env's storage type)."""
    from powergridworld_amd import _lib
    soc, act = C.draws("std", n, 1)
    f32 = dtype == torch.float32
    env = _env("std", n, True, **(dict(dtype=dtype) if f32 else {}))
    _start(env, T64(soc).to(dtype))
    F = env._fused
    a = T64(act[0]).to(dtype)
    bld, pv = F["bld0"], F["pv0"]
    info, pfp, pft, _ = env._step_entry((bld.time_index, pv.index, env._time_at(1), env.pf_solver.tables_version))
    b = type(F["bufs"]).from_buffer_copy(F["bufs"])
    assert isinstance(b, _lib.CoordBuffersF32 if f32 else _lib.CoordBuffers)
    b.action = F["Mat"](a.data_ptr(), a.stride(1), a.stride(2))
    b.act_stride_agent = a.stride(0)
    na, no = len(env.agents), pfp.n_out
    g = dict(v_out=_Guarded(no * n, dtype), vv=_Guarded(n, dtype), iters=_Guarded(n, torch.int32),
             reward=_Guarded(na * n, dtype), agent_power=_Guarded(na * n, dtype))
    for k, x in g.items():
        setattr(b, k, x.ptr)
    return env, a, info, pfp, pft, b, g


def _solve_h1(env, pfp, pft, P):
    """pgw_pf_solve_h1 on the bus loads P: (the coordinated bus [n], iters [n])."""
    from powergridworld_amd import _lib
    n = P.numel()
    v = torch.zeros((pfp.n_out, n), dtype=torch.float64, device=DEV)
    it = torch.zeros(n, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().pgw_pf_solve_h1(pfp, pft, pft._h1, n, _lib.dptr(P), None, _lib.dptr(v), _lib.dptr(it),
                                          _lib.stream_ptr(env.device)))
    return v[0], it


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("variant", ["coordinated", "uncoordinated", "agent_off"])
def test_c_abi_direct(n, variant):
    """pgw_coord_step_h1 called directly with sentinel guards around v_out, vv,
    iters, reward and agent_power: nothing is written outside n, every element
    inside is.  The voltage and the counts are pgw_pf_solve_h1's on 0 + p0 + p1
    ... of the agents in the bus load (agent_ctrl = -1 leaves one out);
    coordinated = 0 leaves the rewards as the agents' kernel wrote them and
    writes no vv; coordinated = 1 stores raw + (-(vv penalty / n_agents))."""
    from powergridworld_amd import _lib
    env, a, info, pfp, pft, b, g = _direct_setup(n)
    F = env._fused
    na = len(env.agents)
    p = _lib.CoordParams.from_buffer_copy(F["params"])
    p.coordinated = 0
    if variant == "agent_off":
        p.agent_ctrl[na - 1] = -1
    st = _lib.stream_ptr(env.device)
    x0, s0 = F["x"].clone(), F["soc"].clone()
    assert _lib.lib().pgw_coord_step_h1(p, pfp, pft, pft._h1, info, n, b, st) == 0
    torch.cuda.synchronize()
    assert all(x.guards_intact() for x in g.values())
    assert g["vv"].untouched()                                   # coordinated = 0 writes no vv
    for k in ("v_out", "iters", "reward", "agent_power"):
        assert not bool((g[k].inner == g[k].sent).any()), k
    raw = g["reward"].inner.view(na, n).clone()
    power = g["agent_power"].inner.view(na, n)
    P = torch.zeros(n, dtype=torch.float64, device=DEV)
    for ai in range(na - 1 if variant == "agent_off" else na):
        P = P + power[ai]
    v, it = _solve_h1(env, pfp, pft, P)
    assert torch.equal(g["v_out"].inner, v) and torch.equal(g["iters"].inner, it)
    if variant == "agent_off":
        v_all, _ = _solve_h1(env, pfp, pft, P + power[na - 1])
        assert not torch.equal(v, v_all)
    if variant != "coordinated":
        return
    # the same step again from the same state, coordinated
    F["x"].copy_(x0)
    F["soc"].copy_(s0)
    p.coordinated = 1
    g2 = {k: _Guarded(x.size, x.t.dtype) for k, x in g.items()}
    for k, x in g2.items():
        setattr(b, k, x.ptr)
    assert _lib.lib().pgw_coord_step_h1(p, pfp, pft, pft._h1, info, n, b, st) == 0
    torch.cuda.synchronize()
    assert all(x.guards_intact() for x in g2.values())
    for k, x in g2.items():
        assert not bool((x.inner == x.sent).any()), k
    assert torch.equal(g2["v_out"].inner, v) and torch.equal(g2["iters"].inner, it)
    assert torch.equal(g2["agent_power"].inner, g["agent_power"].inner)
    vv = torch.maximum(torch.maximum(torch.zeros_like(v), p.vv_lo - v), v - p.vv_hi)
    assert torch.equal(g2["vv"].inner, vv)
    share = (vv * p.vv_penalty) / torch.tensor(float(na), dtype=torch.float64, device=DEV)
    assert torch.equal(g2["reward"].inner.view(na, n), raw + (-share))


def test_c_abi_refusals_touch_nothing():
    """Every refusal of pgw_coord_step_h1 returns PGW_ERR_ARG before any
    launch: the guarded outputs, the observations and the state stay as they were."""
    from powergridworld_amd import _lib
    n = 65
    env, a, info, pfp, pft, b, g = _direct_setup(n)
    F = env._fused
    lib, st = _lib.lib(), _lib.stream_ptr(env.device)
    od0 = pft._keep[0]
    dummy = torch.zeros(4096, dtype=torch.float64, device=DEV)
    c = pft._h1.elem
    other = (c + 1) % pfp.m
    before = [F["obs"].clone(), F["x"].clone(), F["soc"].clone()]

    def call(P=None, pf=None, t=None, od=None, h=pft._h1, bufs=None, s=info):
        t = _lib.PFTables.from_buffer_copy(pft) if t is None else t
        if od is not None:
            t.od = ctypes.addressof(od) if od != "null" else None
        rc = lib.pgw_coord_step_h1(F["params"] if P is None else P, pfp if pf is None else pf, t, h, s, n,
                                   b if bufs is None else bufs, st)
        torch.cuda.synchronize()
        return rc

    def params(**kw):
        q = _lib.PFParams.from_buffer_copy(pfp)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def od(**kw):
        q = _lib.PFOD.from_buffer_copy(od0)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def tables(**kw):
        q = _lib.PFTables.from_buffer_copy(pft)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    two_bands = params()
    two_bands.vmin[3] = 0.9
    two_on_slot = params()
    two_on_slot.elem_ctrl[other] = 0
    wrong_elem = _lib.PFH1.from_buffer_copy(pft._h1)
    wrong_elem.elem = other
    no_agents = _lib.CoordParams.from_buffer_copy(F["params"])
    no_agents.n_agents = 0
    bad_row = _lib.CoordParams.from_buffer_copy(F["params"])
    bad_row.vv_row = pfp.n_out
    no_reward = _lib.CoordBuffers.from_buffer_copy(b)
    no_reward.reward = None
    cases = {
        "od NULL": dict(od="null"),
        "m = 16": dict(pf=params(m=16)),
        "two voltage bands": dict(pf=two_bands),
        "n_ctrl = 2": dict(pf=params(n_ctrl=2)),
        "two elements on slot 0": dict(pf=two_on_slot),
        "h->elem another element": dict(h=wrong_elem),
        "h NULL": dict(h=None),
        "U_init": dict(t=tables(U_init=dummy.data_ptr())),
        "load_scale": dict(t=tables(load_scale=dummy.data_ptr())),
        "od resp": dict(od=od(resp=dummy.data_ptr())),
        "od resp_v": dict(od=od(resp_v=dummy.data_ptr())),
        "od resp_q": dict(od=od(resp_q=dummy.data_ptr())),
        "od start": dict(od=od(start=dummy.data_ptr())),
        "max_iter = 0": dict(pf=params(max_iter=0)),
        "n_agents = 0": dict(P=no_agents),
        "vv_row = n_out": dict(P=bad_row),
        "reward NULL": dict(bufs=no_reward),
        "step info NULL": dict(s=None),
    }
    for name, kw in cases.items():
        assert call(**kw) == -1, name                              # PGW_ERR_ARG
        assert _lib.lib().pgw_last_error(), name
        assert all(x.untouched() for x in g.values()), name
        for x, y in zip(before, (F["obs"], F["x"], F["soc"])):
            assert torch.equal(x, y), name
    assert call() == 0                                             # the unchanged arguments run
    torch.cuda.synchronize()
    assert not any(x.untouched() for x in g.values())


def test_c_abi_f32_direct_and_refusals():
    """pgw_coord_step_h1_f32 called directly, n = 65 (odd: the one-env agents'
    kernel): its refusals -- the fp64 entry's, and any agent layout but the
    standard one, which fp32 storage has no agents' kernel for -- return
    PGW_ERR_ARG with nothing touched; the unchanged arguments write every
    element inside the guards and none outside, the counts those of
    pgw_pf_solve_h1 on the stored powers summed in agent order and the stored
    voltage that solve's rounded once."""
    from powergridworld_amd import _lib
    n = 65
    env, a, info, pfp, pft, b, g = _direct_setup(n, torch.float32)
    F = env._fused
    lib, st = _lib.lib(), _lib.stream_ptr(env.device)
    na = len(env.agents)
    before = [F["obs"].clone(), F["x"].clone(), F["soc"].clone()]
    swapped = _lib.CoordParams.from_buffer_copy(F["params"])
    swapped.comp_order[1], swapped.comp_order[2] = 2, 1            # a valid layout, not the standard one
    two_ctrl = _lib.PFParams.from_buffer_copy(pfp)
    two_ctrl.n_ctrl = 2
    no_od = _lib.PFTables.from_buffer_copy(pft)
    no_od.od = None
    start = _lib.PFOD.from_buffer_copy(pft._keep[0])
    start.start = F["obs"].data_ptr()
    with_start = _lib.PFTables.from_buffer_copy(pft)
    with_start.od = ctypes.addressof(start)
    no_power = type(b).from_buffer_copy(b)
    no_power.agent_power = None
    cases = {
        "non-standard layout": (swapped, pfp, pft, pft._h1, b),
        "n_ctrl = 2": (F["params"], two_ctrl, pft, pft._h1, b),
        "od NULL": (F["params"], pfp, no_od, pft._h1, b),
        "od start": (F["params"], pfp, with_start, pft._h1, b),
        "h NULL": (F["params"], pfp, pft, None, b),
        "agent_power NULL": (F["params"], pfp, pft, pft._h1, no_power),
    }
    for name, (P, pf, t, h, bufs) in cases.items():
        assert lib.pgw_coord_step_h1_f32(P, pf, t, h, info, n, bufs, st) == -1, name     # PGW_ERR_ARG
        torch.cuda.synchronize()
        assert lib.pgw_last_error(), name
        assert all(x.untouched() for x in g.values()), name
        for x, y in zip(before, (F["obs"], F["x"], F["soc"])):
            assert torch.equal(x, y), name
    # the fp64 entry takes the swapped layout (k_coord_agents): the refusal is fp32's own
    assert lib.pgw_coord_step_h1_f32(F["params"], pfp, pft, pft._h1, info, n, b, st) == 0
    torch.cuda.synchronize()
    assert all(x.guards_intact() for x in g.values())
    for k, x in g.items():
        assert not bool((x.inner == x.sent).any()), k
    P = torch.zeros(n, dtype=torch.float64, device=DEV)
    for ai in range(na):
        P = P + g["agent_power"].inner.view(na, n)[ai].double()
    v, it = _solve_h1(env, pfp, pft, P)
    assert torch.equal(g["iters"].inner, it) and torch.equal(g["v_out"].inner, v.float())


# ------------------------------------------------------------------ 8. route selection
@pytest.mark.parametrize("change,text", [
    (dict(bus="671"), "yprim='step' (every solve's Y holds its own loads' admittances)"),
    (dict(step_kernel="general"), "yprim='step' (every solve's Y holds its own loads' admittances)"),
    (dict(snap_start="previous"), "snap_start='previous' (each env's solve starts from its own previous solution)"),
])
def test_route_selection_keeps_its_refusals(change, text):
    """Agents on 671 (a three-phase delta load), step_kernel="general" and
    snap_start="previous" keep their refusal texts -- fused=True raises them --
    and step on the generic path.  (The coordinated transform needs a one-phase
    bus, so the agents on 671 run under the base MultiAgentEnv.)"""
    from powergridworld_amd.multiagent_env import MultiAgentEnv
    from powergridworld_amd.scenarios.coordinated import CoordinatedMultiBuildingControlEnv
    cls = MultiAgentEnv if "bus" in change else CoordinatedMultiBuildingControlEnv
    n = 16

    def config():
        cfg = C.env_config("std")
        pf = cfg["pf_config"]["config"]
        if "bus" in change:
            for ag in cfg["agents"]:
                ag["bus"] = change["bus"]
        elif "snap_start" in change:                      # (yprim="step" needs the direct start)
            pf.update(yprim="dss_file", snap_start="previous")
            pf.pop("step_kernel")
        else:
            pf.update(change)
        return cfg

    with pytest.raises(ValueError) as err:
        cls(**config(), num_envs=n, device=DEV, fused=True)
    assert text in str(err.value)
    env = cls(**config(), num_envs=n, device=DEV)
    assert env._fused is None and env._ma is None
    assert env._fusable() == text
    soc, act = C.draws("std", n, 2)
    _start(env, T64(soc))
    for t in range(2):
        _, rew, _, meta = env.step(_dict_action(env, T64(act[t])))
        assert all(bool(torch.isfinite(r).all()) for r in rew.values())
    it = env.pf_solver.iterations
    assert bool(((it >= 2) & (it <= 15)).all())
