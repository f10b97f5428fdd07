"""OpenDSS's snap solve with every solve's own Yeq in Y (yprim="step", H1) on
the fast one-lane-per-env kernel (OpenDSSSolver(step_kernel="fast");
csrc/pgw_pf.hip k_pf_solve_od_h1, pgw_pf_solve_h1): the hour's reduction in the
packed block, the env's rank-1 Yeq correction K formed in the kernel, no
response table.  Needs an MI355X.

The reference is the oracle's restatement of OpenDSS's snap solve with
yprim_kw = None (oracle/pf_oracle.py Feeder.snap_opendss) on the cases of
tests/_pf_h1_common.py -- equal iteration counts with the sign, every node
within 1e-9 rel, the project's standing figure for a solve against the oracle
-- and the general kernel (step_kernel="general") on the same inputs: equal
counts, 1e-11 rel, the figure the multi-slot tests use between the fast and the
general kernel.  tests/test_cpu_pf_h1.py asserts, from the oracle alone, that
every stopping decision of these cases is at least 1e-8 from the threshold, so
equal counts are a fair demand.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _pf_h1_common as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = -1                                         # PGW_ERR_ARG (include/pgw.h)


def _solver(K, case=None, **kw):
    from powergridworld_amd.distribution_system.opendss import OpenDSSSolver
    if case is not None and C.CASES[case]["max_iter"]:
        kw["max_iter"] = C.CASES[case]["max_iter"]
    kw.setdefault("yprim", "step")
    if kw["yprim"] == "step":
        kw.setdefault("step_kernel", "fast")
    return OpenDSSSolver(C.IEEE13, C.SHAPE, device=DEV, system_load_rescale_factor=C.RESCALE, convergence="opendss",
                         num_envs=K, **kw)


def _T(a, K):
    return torch.tensor(np.ascontiguousarray(a[:K]), dtype=torch.float64, device=DEV)


def _solve(s, load, loads, K):
    """[T, nodes, K] pu and [T, K] iterations of s over TIMES with the load's
    powers `loads` (per time (P, Q) [>= K]; load None: no controllable load)."""
    v, it = [], []
    for t, (P, Q) in zip(C.TIMES, loads):
        if load is None:
            s.calculate_power_flow(current_time=t)
        else:
            s.calculate_power_flow({load: _T(P, K)}, {load: _T(Q, K)}, current_time=t)
        bv = s.get_bus_voltages()
        v.append(torch.stack([bv[nm] for nm in s.feeder.node_names]).clone())
        it.append(s.iterations.clone())
    torch.cuda.synchronize()
    return torch.stack(v), torch.stack(it)


@functools.lru_cache(maxsize=None)
def _fast(case, K=C.K):
    """The fast H1 solve of a case (shared, left unchanged)."""
    s = _solver(K, case)
    out = _solve(s, C.CASES[case]["load"], C.loads(case), K)
    assert s._h1_fast and s._od_fast and not s.general
    return out


def _rel(a, b):
    return ((a - b).abs() / b.abs()).max().item()


# ------------------------------------------------------------------ selection
def test_step_kernel_selects_the_route():
    """step_kernel="fast" keeps general False on IEEE-13 with no controllable
    load and with one of one phase element; the delta load 671 (three elements)
    and two loads fall back to the general kernel; the default is the general
    kernel; and the tables it hands out evaluate every check row and carry no
    response table."""
    s = _solver(8)
    assert s.step_kernel == "fast" and s._h1_fast and not s.general and not s.od_table
    s.set_controllable_loads(["675c"])
    assert s._h1_fast and not s.general and s.params.n_ctrl == 1
    tb = s.step_tables(C.TIMES[0])
    od = tb._keep[0]
    assert od.n_rep == od.n_rows > 0 and not od.resp and not od.resp_v and not od.resp_q and not od.start
    assert tb._h1.elem == C.elem_of("675c")
    assert s.step_tables(C.TIMES[0]) is tb                       # cached per (hour, configuration)
    for names in (["671"], ["675a", "675c"]):
        g = _solver(8)
        g.set_controllable_loads(names)
        assert g.general and not g._h1_fast and not g._od_fast, names
    d = _solver(8, step_kernel="general")
    assert d.general and not d._h1_fast


# ------------------------------------------------------------------ oracle, general kernel
@pytest.mark.parametrize("case,K", [(c, k) for c in "RST" for k in C.BATCHES] + [("T3", C.K)])
def test_h1_vs_oracle_and_general_kernel(case, K):
    """Through the solver: iterations equal the oracle's with the sign, every
    node within 1e-9 rel; and the general kernel on the same inputs gives equal
    counts and voltages within 1e-11 rel."""
    load, loads = C.CASES[case]["load"], C.loads(case)
    v, it = _fast(case, K)
    g = _solver(K, case, step_kernel="general")
    vg, itg = _solve(g, load, loads, K)
    assert g.general and not g._h1_fast
    worst_o, worst_og = 0.0, 0.0
    for i, ref in enumerate(C.oracle(case)):
        want = torch.tensor(ref["pu"][:K].T.copy(), device=DEV)
        worst_o = max(worst_o, _rel(v[i], want))
        worst_og = max(worst_og, _rel(vg[i], want))
    print("case %s K %d: fast vs oracle %.3e, general vs oracle %.3e, fast vs general %.3e"
          % (case, K, worst_o, worst_og, _rel(v, vg)))
    for i, ref in enumerate(C.oracle(case)):
        np.testing.assert_array_equal(it[i].cpu().numpy(), C.signed_iterations(ref)[:K])
        np.testing.assert_allclose(v[i].cpu().numpy().T, ref["pu"][:K], rtol=1e-9, atol=0)
    assert torch.equal(it, itg)
    torch.testing.assert_close(v, vg, rtol=1e-11, atol=0)
    if case == "T3":
        assert (it == -3).any() and (it > 0).any()
    if case == "T" and K == C.K:
        assert (it == -15).any()


def test_h1_is_measurably_not_h2():
    """The same inputs under yprim="dss_file" (H2, every env solved): more than
    1e-7 pu apart."""
    v, _ = _fast("S")
    h2 = _solver(C.K, "S", yprim="dss_file", od_table=False)
    v2, _ = _solve(h2, "675c", C.loads("S"), C.K)
    assert not h2.general and (v - v2).abs().max().item() > 1e-7


def test_h1_no_controllable_load_and_zero_powers():
    """No controllable load gives the oracle's base solve (with and without a
    controllable slot configured); envs at P = 0, Q = 0 or both agree with the
    oracle like any other."""
    K = 4
    for names in ([], ["675c"]):
        s = _solver(K)
        s.set_controllable_loads(names)
        v, it = _solve(s, None, [(None, None)] * len(C.TIMES), K)
        assert s._h1_fast and not s.general
        for i, (pu0, it0) in enumerate(C.oracle_base()):
            assert (it[i] == it0).all()
            np.testing.assert_allclose(v[i].cpu().numpy().T, np.tile(pu0, (K, 1)), rtol=1e-9, atol=0)
    s = _solver(K)
    v, it = _solve(s, "675c", [(C.EDGE_P, C.EDGE_Q)] * len(C.TIMES), K)
    g = _solver(K, step_kernel="general")
    vg, itg = _solve(g, "675c", [(C.EDGE_P, C.EDGE_Q)] * len(C.TIMES), K)
    for i, (pue, ite) in enumerate(C.oracle_edge()):
        np.testing.assert_array_equal(it[i].cpu().numpy(), ite)
        np.testing.assert_allclose(v[i].cpu().numpy().T, pue, rtol=1e-9, atol=0)
    assert torch.equal(it, itg)
    torch.testing.assert_close(v, vg, rtol=1e-11, atol=0)
    # P = Q = 0 on the slot is the solve without a controllable load
    base = _solve(_solver(K), None, [(None, None)] * len(C.TIMES), K)
    assert torch.equal(v[:, :, 0], base[0][:, :, 0]) and torch.equal(it[:, 0], base[1][:, 0])


def test_h1_sparse_and_dense_row_tests_agree():
    """The check rows as every lane's row groups (sparse_envs = -1) and one env
    at a time (64): equal to the default, bit for bit, counts included."""
    ref = _fast("T")
    s = _solver(C.K, "T")
    for sp in (-1, 64):
        s._od_proto.sparse_envs = sp
        s._h1f_cache.clear()
        got = _solve(s, "675c", C.loads("T"), C.K)
        assert torch.equal(got[1], ref[1]) and torch.equal(got[0], ref[0]), sp


# ------------------------------------------------------------------ the C ABI directly
def _abi_inputs(case, K, ti=1):
    s = _solver(K, case)
    s.set_controllable_loads([C.CASES[case]["load"]])
    t = C.TIMES[ti]
    P, Q = C.loads(case)[ti]
    return s, s.step_params(t), s.solve_tables(t, True), _T(P, K).reshape(1, K), _T(Q, K).reshape(1, K), ti


def test_abi_refusals():
    """PGW_ERR_ARG before any launch: od NULL; a shape other than the fast one
    (two bands; m = 8); n_ctrl > 1; more or fewer than one element on slot 0,
    or pgw_pf_h1.elem not that element; U_init; load_scale; resp, resp_v,
    resp_q.  The plain call is OK."""
    from powergridworld_amd import _lib
    K = 65
    s, prm, tb, Pd, Qd, _ = _abi_inputs("S", K)
    lib, st = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    v = torch.empty((prm.n_out, K), dtype=torch.float64, device=DEV)
    it = torch.empty(K, dtype=torch.int32, device=DEV)
    dummy = torch.zeros(4096, dtype=torch.float64, device=DEV)

    def call(p=prm, tabs=tb, h=None, fn=lib.pgw_pf_solve_h1):
        return fn(p, tabs, tb._h1 if h is None else h, K, _lib.dptr(Pd), _lib.dptr(Qd), _lib.dptr(v), _lib.dptr(it), st)
    assert call() == 0
    t2 = _lib.PFTables.from_buffer_copy(tb)
    t2.od = None
    assert call(tabs=t2) == ERR_ARG
    p2 = _lib.PFParams.from_buffer_copy(prm)
    p2.vmin[3] = 0.9
    assert call(p=p2) == ERR_ARG
    p2 = _lib.PFParams.from_buffer_copy(prm)
    p2.m = 8
    assert call(p=p2) == ERR_ARG
    p2 = _lib.PFParams.from_buffer_copy(prm)
    p2.n_ctrl = 2
    assert call(p=p2) == ERR_ARG
    c = C.elem_of("675c")
    p2 = _lib.PFParams.from_buffer_copy(prm)                 # two elements on slot 0
    p2.elem_ctrl[(c + 1) % 14] = 0
    assert call(p=p2) == ERR_ARG
    p2 = _lib.PFParams.from_buffer_copy(prm)                 # none
    p2.elem_ctrl[c] = -1
    assert call(p=p2) == ERR_ARG
    for bad in (c + 1, -1, 14):                              # elem is not the slot's element
        h2 = _lib.PFH1.from_buffer_copy(tb._h1)
        h2.elem = bad
        assert call(h=h2) == ERR_ARG, bad
    for field in ("load_scale", "U_init"):
        t2 = _lib.PFTables.from_buffer_copy(tb)
        setattr(t2, field, dummy.data_ptr())
        assert call(tabs=t2) == ERR_ARG, field
    for field in ("resp", "resp_v", "resp_q"):
        od = _lib.PFOD.from_buffer_copy(tb._keep[0])
        setattr(od, field, dummy.data_ptr())
        t2 = _lib.PFTables.from_buffer_copy(tb)
        t2.od = ctypes.addressof(od)
        assert call(tabs=t2) == ERR_ARG, field
        assert call(tabs=t2, fn=lib.pgw_pf_solve_h1_f32) == ERR_ARG, field
    torch.cuda.synchronize()


@pytest.mark.parametrize("case,K", [("S", 1), ("S", 65), ("T", 65)])
def test_abi_outputs_agree_and_stay_in_bounds(case, K):
    """pgw_pf_solve_h1 called directly: v_min_out / v_max_out are the extrema of
    v_out's rows in row order, the extrema-only call (v_out NULL) gives the same
    bit for bit, and sentinels around v_out, iters and the extrema are intact:
    nothing is written past n."""
    from powergridworld_amd import _lib
    s, prm, tb, Pd, Qd, ti = _abi_inputs(case, K)
    n_out, G = prm.n_out, 64
    lib, st = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    SENT = -7.25
    vbuf = torch.full((n_out * K + 2 * G,), SENT, dtype=torch.float64, device=DEV)
    ibuf = torch.full((K + 2 * G,), -77, dtype=torch.int32, device=DEV)
    vmn, vmx, vmn2, vmx2 = (torch.full((K + 2 * G,), SENT, dtype=torch.float64, device=DEV) for _ in range(4))
    t2 = _lib.PFTables.from_buffer_copy(tb)
    t2.v_min_out, t2.v_max_out = vmn[G:].data_ptr(), vmx[G:].data_ptr()
    _lib.check(lib.pgw_pf_solve_h1(prm, t2, tb._h1, K, _lib.dptr(Pd), _lib.dptr(Qd),
                                   ctypes.c_void_p(vbuf[G:].data_ptr()), ctypes.c_void_p(ibuf[G:].data_ptr()), st))
    t3 = _lib.PFTables.from_buffer_copy(tb)            # extrema only
    t3.v_min_out, t3.v_max_out = vmn2[G:].data_ptr(), vmx2[G:].data_ptr()
    _lib.check(lib.pgw_pf_solve_h1(prm, t3, tb._h1, K, _lib.dptr(Pd), _lib.dptr(Qd), None, None, st))
    torch.cuda.synchronize()
    for buf, size in ((vbuf, n_out * K), (vmn, K), (vmx, K), (vmn2, K), (vmx2, K)):
        assert (buf[:G] == SENT).all() and (buf[G + size:] == SENT).all()
        assert (buf[G:G + size] != SENT).all()
    assert (ibuf[:G] == -77).all() and (ibuf[G + K:] == -77).all()
    v = vbuf[G:G + n_out * K].view(n_out, K)
    ref = C.oracle(case)[ti]
    np.testing.assert_array_equal(ibuf[G:G + K].cpu().numpy(), C.signed_iterations(ref)[:K])
    rows = [s.feeder.node_index[nm] for nm in s.output_names]
    np.testing.assert_allclose(v.cpu().numpy().T, ref["pu"][:K][:, rows], rtol=1e-9, atol=0)
    assert torch.equal(vmn[G:G + K], v.min(0).values) and torch.equal(vmx[G:G + K], v.max(0).values)
    assert torch.equal(vmn2[G:G + K], vmn[G:G + K]) and torch.equal(vmx2[G:G + K], vmx[G:G + K])


@pytest.mark.parametrize("case", ["S", "T"])
def test_h1_f32_equals_fp64_solve(case):
    """pgw_pf_solve_h1_f32 (test_pf_solve_f32_equals_fp64_solve's contract): from
    fp32-representable powers, every voltage is the fp64 entry's rounded once,
    every iteration count equal."""
    from powergridworld_amd import _lib
    K = C.K
    s, prm, tb, _, _, _ = _abi_inputs(case, K)
    lib, st = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    n_out = prm.n_out
    for ti, t in enumerate(C.TIMES):
        prm, tb = s.step_params(t), s.solve_tables(t, True)
        P, Q = C.loads(case)[ti]
        p32 = torch.tensor(np.ascontiguousarray(P), dtype=torch.float32, device=DEV).reshape(1, K)
        q32 = torch.tensor(np.ascontiguousarray(Q), dtype=torch.float32, device=DEV).reshape(1, K)
        p64, q64 = p32.double(), q32.double()
        v64 = torch.empty((n_out, K), dtype=torch.float64, device=DEV)
        v32 = torch.empty((n_out, K), dtype=torch.float32, device=DEV)
        i64 = torch.empty(K, dtype=torch.int32, device=DEV)
        i32 = torch.empty(K, dtype=torch.int32, device=DEV)
        _lib.check(lib.pgw_pf_solve_h1(prm, tb, tb._h1, K, _lib.dptr(p64), _lib.dptr(q64), _lib.dptr(v64),
                                       _lib.dptr(i64), st))
        _lib.check(lib.pgw_pf_solve_h1_f32(prm, tb, tb._h1, K, _lib.dptr(p32), _lib.dptr(q32), _lib.dptr(v32),
                                           _lib.dptr(i32), st))
        torch.cuda.synchronize()
        assert torch.equal(i64, i32), t
        assert torch.equal(v64.float(), v32), t
        assert (i64 != 0).all() and torch.isfinite(v64).all()


# ------------------------------------------------------------------ the fused multi-agent step
def _het_cfg(**pf):
    from powergridworld_amd.scenarios.heterogeneous import make_env_config
    cfg = make_env_config()
    cfg["pf_config"]["config"].update(dict(yprim="step", step_kernel="fast"), **pf)
    return cfg


def _het_act(a):
    return {"building": {"building": a[:, :6], "pv": a[:, 6:7], "storage": a[:, 7:8]},
            "pv": a[:, 8:9], "ev-charging": a[:, 9:10]}


def _flat(o):
    return torch.cat([o["building"]["building"], o["building"]["pv"], o["building"]["storage"],
                      o["pv"], o["ev-charging"]], 1)


def test_het_h1_fused_equals_generic():
    """The heterogeneous scenario with yprim="step", step_kernel="fast", 256 envs,
    12 steps from reset: the fused multi-agent step (pgw_ma_step's agents, then
    pgw_pf_solve_h1 on the bus loads) equals the generic path bit for bit --
    observations, rewards, extrema, every node voltage, iteration counts."""
    from powergridworld_amd import _lib
    from powergridworld_amd.multiagent_env import MultiAgentEnv
    n, steps = 256, 12
    envs = [MultiAgentEnv(**_het_cfg(), num_envs=n, device=DEV, fused=f) for f in (True, False)]
    assert envs[0]._ma is not None and envs[0]._fused is None and envs[1]._ma is None
    assert envs[0]._ma["h1"] is _lib.lib().pgw_pf_solve_h1
    for env in envs:
        ps = env.pf_solver
        assert ps._h1_fast and not ps.general and list(ps._ctrl_names) == ["675c"]
    rng = np.random.default_rng(9)
    soc0 = torch.tensor(rng.uniform(5.0, 240.0, size=n), device=DEV)
    for env in envs:
        env.reset()
        env.agent_dict["building"].env_dict["storage"].reset(init_storage=soc0)
    nodes = envs[0].pf_solver.feeder.node_names
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
        v0, v1 = envs[0].pf_solver.get_bus_voltages(), envs[1].pf_solver.get_bus_voltages()
        for x in nodes:
            assert torch.equal(v0[x], v1[x]), (k, x)
    it = envs[0].pf_solver.iterations
    assert bool(((it >= 2) & (it <= 15)).all())


def test_het_h1_f32_agents_against_the_component_entries():
    """dtype=float32 on the same configuration (pgw_ma_step_f32, then the fp64
    pgw_pf_solve_h1), 256 envs, 12 steps, as tests/test_gpu_f32_ma.py compares:
    fp32 twins of the agents stepped through their own fp32 entries give the
    same observations, powers and rewards bit for bit, the bus load is the fp64
    sum of the stored agent powers, and the step's power flow is the stand-alone
    fp64 H1 solve of that bus load (extrema and iteration counts)."""
    from powergridworld_amd import _lib
    from powergridworld_amd.base import MultiComponentEnv
    from powergridworld_amd.agents.vehicles import EVChargingEnv
    from powergridworld_amd.distribution_system.opendss import OpenDSSSolver
    from powergridworld_amd.multiagent_env import MultiAgentEnv
    from powergridworld_amd.scenarios.heterogeneous import ThisPVEnv
    F32 = torch.float32
    n, steps = 256, 12
    cfg = _het_cfg()
    env = MultiAgentEnv(**cfg, num_envs=n, device=DEV, dtype=F32)
    assert env._ma is not None and env._ma["fn"] is _lib.lib().pgw_ma_step_f32
    assert env._ma["h1"] is _lib.lib().pgw_pf_solve_h1 and env.pf_solver._h1_fast
    by = {a["name"]: a for a in cfg["agents"]}
    cc = cfg["common_config"]
    mc = MultiComponentEnv(name="building", num_envs=n, device=DEV, dtype=F32, **by["building"]["config"], **cc)
    pv = ThisPVEnv(name="pv", num_envs=n, device=DEV, dtype=F32, **by["pv"]["config"], **cc)
    ev = EVChargingEnv(name="ev-charging", num_envs=n, device=DEV, dtype=F32, **by["ev-charging"]["config"], **cc)
    pf = OpenDSSSolver(**cfg["pf_config"]["config"], num_envs=n, device=DEV)
    pf.set_controllable_loads(["675c"])
    assert pf._h1_fast and not pf.general
    rng = np.random.default_rng(10)
    soc0 = torch.tensor(rng.uniform(5.0, 240.0, size=n), device=DEV).float()
    env.reset()
    env.agent_dict["building"].env_dict["storage"].reset(init_storage=soc0)
    pf.calculate_power_flow(current_time=env.time)
    v_prev = env.pf_solver.voltage_extrema()[0].clone()
    assert torch.equal(v_prev, pf.voltage_extrema()[0])
    mc.reset()
    mc.env_dict["storage"].reset(init_storage=soc0)
    pv.reset(min_voltage=v_prev)
    ev.reset()
    A = env.agent_dict
    z = torch.zeros(n, dtype=torch.float64, device=DEV)
    for k in range(steps):
        a = torch.tensor(rng.uniform(-1.1, 1.1, (n, 10)), device=DEV).float()
        obs, rew, done, _ = env.step(_het_act(a))
        o_mc, r_mc, _, _ = mc.step(_het_act(a)["building"])
        o_pv, r_pv, _, _ = pv.step(a[:, 8:9], min_voltage=v_prev)
        o_ev, r_ev, _, _ = ev.step(a[:, 9:10])
        for c in ("building", "pv", "storage"):
            assert torch.equal(obs["building"][c], o_mc[c]), (k, c)
        assert torch.equal(obs["pv"], o_pv) and torch.equal(obs["ev-charging"], o_ev), k
        assert torch.equal(rew["building"], r_mc) and torch.equal(rew["pv"], r_pv), k
        assert torch.equal(rew["ev-charging"], r_ev), k
        for f, t in ((A["building"], mc), (A["pv"], pv), (A["ev-charging"], ev)):
            assert f.real_power.dtype == F32 and torch.equal(f.real_power, t.real_power), (k, f.name)
        bus = ((z + A["building"].real_power.double()) + A["pv"].real_power.double()) + \
            A["ev-charging"].real_power.double()
        assert env._ma["bus_p"].dtype == torch.float64 and torch.equal(env._ma["bus_p"][0], bus), k
        pf.calculate_power_flow(current_time=env.time, p_controllable_consumed={"675c": bus})
        e_f, e_s = env.pf_solver.voltage_extrema(), pf.voltage_extrema()
        assert e_f[0].dtype == torch.float64
        assert torch.equal(e_f[0], e_s[0]) and torch.equal(e_f[1], e_s[1]), k
        assert torch.equal(env.pf_solver.iterations, pf.iterations), k
        v_prev = e_f[0].clone()
    assert (env.pf_solver.iterations > 0).all()


def test_het_h1_layout_on_671_falls_back():
    """The agents on the delta load 671 (three phase elements): the solver runs
    the general kernel and the fused step refuses, as under step_kernel =
    "general"; the generic path steps."""
    from powergridworld_amd.multiagent_env import MultiAgentEnv
    cfg = _het_cfg()
    for a in cfg["agents"]:
        a["bus"] = "671"
    env = MultiAgentEnv(**cfg, num_envs=64, device=DEV)
    assert env._ma is None and env._fused is None
    env.reset()
    a = torch.tensor(np.random.default_rng(3).uniform(-1, 1, (64, 10)), device=DEV)
    _, r, _, _ = env.step(_het_act(a))
    ps = env.pf_solver
    assert ps.general and not ps._h1_fast and ps.yprim == "step"
    assert bool(((ps.iterations >= 2) & (ps.iterations <= 15)).all())
    assert all(bool(torch.isfinite(x).all()) for x in r.values())
