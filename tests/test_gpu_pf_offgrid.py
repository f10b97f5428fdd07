"""OpenDSS's snap solve off the response table's kW grid, on every path that
restates it (csrc/pgw_pf.hip od_solve, od_wave_solve, the general kernel):
iteration counts up to the cap of 15 and envs stopped by it (-15), loads in the
constant-impedance bands on both sides of [vminpu, vmaxpu], V675.3 below
Vlowpu, node voltages 0.39 .. 1.6 pu -- where od_decide's bounded rows are no
longer a few percent apart.  The inputs are tests/_offgrid_common.py's
(tests/test_cpu_pf_offgrid.py shows on the oracle that they reach all of this
and that no env is a knife edge); the reference is the oracle's restatement of
the snap solve (oracle/pf_oracle.py Feeder.snap_opendss), which evaluates every
node every iteration.  Every tolerance is one the suite already pins in the
table's operating region (1e-9 rel against the oracle, 1e-11 between kernels
and for the table's fit, 1e-12 for row records, bit identity between paths
that run the same solve).  Solver level first, then the fused C4 step; the
list form of the step (PGW_STEP_LIST=1, read at library load) runs in a child
process (tests/_step_list_child.py).  Needs an MI355X."""
import functools
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

from tests import _offgrid_common as C
from tests.test_gpu_pf_od import _served
from tests.test_gpu_step_overlap import NAMES, _bad, _outputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ solver level
def _new_solver(rescale, num_envs=C.K, **kw):
    from powergridworld_amd.distribution_system.opendss import OpenDSSSolver
    return OpenDSSSolver(C.IEEE13, C.SHAPE, device=DEV, system_load_rescale_factor=rescale, num_envs=num_envs,
                         convergence="opendss", **kw)


@functools.lru_cache(maxsize=None)
def _solvers(rescale):
    """(a) the fast kernel with the table, (b) without it, (c) the general
    kernel -- one of each per rescale factor (one table build)."""
    return {"table": _new_solver(rescale), "solve": _new_solver(rescale, od_table=False),
            "general": _new_solver(rescale, general=True)}


def _dev(x):
    return None if x is None else torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=DEV)


def _solve(s, ti, P, Q):
    """([nodes, K] pu in the feeder's node order, [K] iterations) of one
    calculate_power_flow at TIMES[ti]."""
    s.calculate_power_flow({"675c": _dev(P)}, None if Q is None else {"675c": _dev(Q)},
                           current_time=pd.Timestamp(C.TIMES[ti][0]))
    bv = s.get_bus_voltages()
    v = torch.stack([bv[nm] for nm in s.feeder.node_names]).clone()
    it = s.iterations.clone()
    torch.cuda.synchronize()
    return v, it


def _rel(x, y):
    return ((x - y).abs() / y.abs()).max().item()


def _oracle_nodes(s, ti, which):
    """The oracle's ladder result in the solver's node order: ([nodes, K] pu,
    iterations, last_converged)."""
    _, pu, it, conv = C.oracle_ladder(ti, which)
    names = C.feeder(ti).node_names
    order = [names.index(nm) for nm in s.feeder.node_names]
    return pu[:, order].T, it, conv


@pytest.mark.parametrize("ti", range(len(C.TIMES)))
def test_offgrid_ladder_every_entry_vs_oracle(ti):
    """Both passes of the ladder through (a) the fast kernel with the table,
    (b) without it, (c) the general kernel, (d) pgw_pf_solve_f32 and (e) the
    oracle.  (a) = (b) in every iteration count, bit for bit in every node of
    an env the table does not serve (both run od_solve), within 1e-11 rel where
    it serves; (a) = (c) in iterations, nodes within 1e-11 rel; each of (a),
    (b), (c) against the oracle: |iterations| equal, negative exactly where the
    oracle's last iteration failed the test, unconverged() that number, every
    node within 1e-9 rel -- capped envs included: no wider bound for them was
    needed (measured on an MI355X: every entry within 2.8e-11 rel of the
    oracle over the six ladders, the worst env a capped one; fast vs general
    5.6e-14; the figures are printed); (d) equals the fp64 entry on the widened
    inputs rounded once.  In the Q pass the two envs at P = +-0 have Q = 0 and
    are served."""
    from powergridworld_amd import _lib
    t, rescale = C.TIMES[ti]
    S = _solvers(rescale)
    P = C.ladder()
    lib, st = _lib.lib(), _lib.stream_ptr(torch.device(DEV))
    for which in C.PASSES:
        Q = C.ladder_q(P, which)
        res = {k: _solve(s, ti, P, Q) for k, s in S.items()}
        unc = {k: s.unconverged() for k, s in S.items()}
        (va, ia), (vb, ib), (vc, ic) = res["table"], res["solve"], res["general"]
        tab = S["table"]
        # the table serves Q = 0 only: in the Q pass the two envs at P = +-0
        served = _served(tab, tab.hour_of(pd.Timestamp(t)), P) & (True if Q is None else Q == 0.0)
        inside = C.in_grid(P)
        assert not served[~inside].any()
        if which == "q0":
            assert served[inside].sum() >= 0.9 * inside.sum(), (int(served.sum()), int(inside.sum()))
        else:
            assert served.sum() <= 2, int(served.sum())
        sv = torch.tensor(served, device=DEV)
        # (a) vs (b)
        assert torch.equal(ia, ib), "%s: table vs solve: %d iteration counts differ" % (which, int((ia != ib).sum()))
        bad = (va[:, ~sv] != vb[:, ~sv]).any(0)
        assert not bad.any(), "%s: %d unserved envs differ between table and solve" % (which, int(bad.sum()))
        if served.any():
            r = _rel(va[:, sv], vb[:, sv])
            print("%s %s: table vs solve on %d served envs %.3e" % (t, which, int(served.sum()), r))
            assert r < 1e-11, r
        # (a) vs (c)
        assert torch.equal(ia, ic), "%s: fast vs general: %d iteration counts differ" % (which, int((ia != ic).sum()))
        r = _rel(va, vc)
        print("%s %s: fast vs general %.3e" % (t, which, r))
        assert r < 1e-11, r
        # (a), (b), (c) vs (e)
        want, oit, conv = _oracle_nodes(tab, ti, which)
        capped = oit == 15
        for k, (v, it) in res.items():
            it_h, v_h = it.cpu().numpy(), v.cpu().numpy()
            err = np.abs(v_h - want) / want
            print("%s %s %s vs oracle: all %.3e, capped %.3e (%d envs, %d unconverged)"
                  % (t, which, k, err.max(), err[:, capped].max(), int(capped.sum()), int((~conv).sum())))
            np.testing.assert_array_equal(np.abs(it_h), oit, err_msg="%s %s" % (which, k))
            np.testing.assert_array_equal(it_h < 0, ~conv, err_msg="%s %s" % (which, k))
            assert unc[k] == int((~conv).sum()) > 0, (k, unc[k])
            np.testing.assert_allclose(v_h, want, rtol=1e-9, atol=0, err_msg="%s %s" % (which, k))
        # (d) the fp32 entry on both fast solvers
        ts = pd.Timestamp(t)
        for k in ("table", "solve"):
            s = S[k]
            prm, tb = s.step_params(ts), s.solve_tables(ts, True)
            p32 = torch.tensor(P, dtype=torch.float32, device=DEV)[None].contiguous()
            q32 = None if Q is None else torch.tensor(Q, dtype=torch.float32, device=DEV)[None].contiguous()
            p64, q64 = p32.double(), None if q32 is None else q32.double()
            n_out = prm.n_out
            v64 = torch.empty((n_out, C.K), dtype=torch.float64, device=DEV)
            v32 = torch.empty((n_out, C.K), dtype=torch.float32, device=DEV)
            i64 = torch.empty(C.K, dtype=torch.int32, device=DEV)
            i32 = torch.empty(C.K, dtype=torch.int32, device=DEV)
            _lib.check(lib.pgw_pf_solve(prm, tb, C.K, _lib.dptr(p64), _lib.dptr(q64), _lib.dptr(v64),
                                        _lib.dptr(i64), st))
            _lib.check(lib.pgw_pf_solve_f32(prm, tb, C.K, _lib.dptr(p32), _lib.dptr(q32), _lib.dptr(v32),
                                            _lib.dptr(i32), st))
            torch.cuda.synchronize()
            assert torch.equal(i64, i32), (which, k)
            assert torch.equal(v64.float(), v32), (which, k)
            assert (i64 != 0).all() and (i64 < 0).any() and torch.isfinite(v64).all()


@pytest.mark.parametrize("rescale", sorted({r for _, r in C.TIMES}))
def test_offgrid_bounded_rows_equal_every_row_and_rerun(rescale):
    """tests/test_gpu_pf_od.py's bounded-rows loop on the ladder, every env
    solved (od_table=False): the fast kernel equals the same solve with every
    row evaluated (n_rep = n_rows), with bounds that never decide (gsrc = 1e9)
    and with the rows evaluated as row groups or one env at a time
    (sparse_envs -1 / 64) -- iterations and every node bit for bit, where the
    node voltages are tens of percent apart.  On the ladder no env is decided
    by a bounded row, so a third batch holds the envs that are (found on the
    oracle, decider_envs) and their neighbourhoods: at their centres the
    kernel's count is the oracle's over every node, one above the count of the
    evaluated nodes alone -- a build in which od_decide's bound always decides
    gives the latter (checked once, with such a build)."""
    tis = [i for i, (_, r) in enumerate(C.TIMES) if r == rescale]
    P = C.ladder()
    loads = [(ti, P, C.ladder_q(P, w)) for ti in tis for w in C.PASSES]
    # and the envs a bounded row decides (tests/_offgrid_common.py decider_envs:
    # the evaluated nodes pass the test an iteration before every node does),
    # with their neighbourhoods, tiled over the batch
    for ti in tis:
        Pd = C.decider_ladder(ti)
        assert 0 < len(Pd) <= C.K
        loads.append((ti, np.resize(Pd, C.K), None))
    base = _solvers(rescale)["solve"]
    od, f = base._od_proto, base.feeder
    elem = {f.node_names[f.elem_p[k]] for k in range(f.m) if f.elem_q[k] < 0}
    assert elem | set(base._od_rows[:od.n_rep]) == set(C.EVALUATED), "the evaluated rows changed: update EVALUATED"
    ref = [_solve(base, *ld) for ld in loads]
    assert any((it < 0).any() for _, it in ref) and any((it == 15).any() for _, it in ref)
    for (ti, Pl, _), (_, it) in zip(loads[-len(tis):], ref[-len(tis):]):
        # the solve is on the every-node side of those envs: the oracle's count
        # at the centres of the intervals
        centre, _ = C.decider_envs(ti)
        mid = np.arange(len(centre)) * C.DECIDER_POINTS + C.DECIDER_POINTS // 2
        assert np.array_equal(Pl[mid], centre)
        want, sub = C.counts_by_rows(ti, centre)
        got = np.abs(it.cpu().numpy()[mid])
        print("%s decider envs: kernel %s, every node %s, evaluated nodes alone %s" % (C.TIMES[ti][0], got, want, sub))
        np.testing.assert_array_equal(got, want)
    for change in (dict(n_rep=None), dict(gsrc=1e9), dict(sparse_envs=-1), dict(sparse_envs=64),
                   dict(sparse_envs=64, gsrc=1e9), dict(sparse_envs=-1, gsrc=1e9)):
        s = _new_solver(rescale, od_table=False)
        assert 0 < s._od_proto.n_rep < s._od_proto.n_rows
        if change.get("n_rep", 0) is None:
            s._od_proto.n_rep = s._od_proto.n_rows
        if "gsrc" in change:
            s._od_proto.gsrc = change["gsrc"]
        if "sparse_envs" in change:
            s._od_proto.sparse_envs = change["sparse_envs"]
        s._tables_cache.clear()
        for ld, (v0, i0) in zip(loads, ref):
            v, it = _solve(s, *ld)
            assert torch.equal(it, i0), (change, C.TIMES[ld[0]][0], int((it != i0).sum()))
            assert torch.equal(v, v0), (change, C.TIMES[ld[0]][0], int((v != v0).any(0).sum()))


def _extrema_only(s, ts, P):
    """The solve at `ts` with v_out = NULL: (min, max, iterations, the tables'
    od struct) -- as tests/test_gpu_parity.py makes the call."""
    from powergridworld_amd import _lib
    n = len(P)
    prm, tb = s.step_params(ts), s.step_tables(ts)
    t = type(tb).from_buffer_copy(tb)
    t._od_ref = tb._od_ref
    mn = torch.full((n,), -1.0, dtype=torch.float64, device=DEV)
    mx = torch.full((n,), -1.0, dtype=torch.float64, device=DEV)
    it = torch.zeros(n, dtype=torch.int32, device=DEV)
    t.v_min_out, t.v_max_out = mn.data_ptr(), mx.data_ptr()
    cp = _dev(P)[None].contiguous()
    _lib.check(_lib.lib().pgw_pf_solve(prm, t, n, cp.data_ptr(), None, None, _lib.dptr(it),
                                       _lib.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    return mn, mx, it, tb._od_ref


def _served_block(s, ts, count):
    """`count` kW values inside the grid that the hour's table serves (chosen
    from the table's own records on the host)."""
    x0, h, n = C.grid()
    pool = np.random.default_rng(5).uniform(x0 + 1.0, x0 + (n - 1) * h - 1.0, 4 * count)
    ok = pool[_served(s, s.hour_of(ts), pool)]
    assert len(ok) >= count, len(ok)
    return ok[:count]


def test_offgrid_extrema_rows_and_row_records():
    """The heterogeneous scenario's settings and output rows (every node):
    voltage_extrema() equals Python's min / max over the rows in order; the
    extrema-only solve (v_out = NULL) gives the same bits -- on the ladder,
    whose blocks all mix served and off-grid envs, and on the ladder with its
    first 256 envs replaced by served ones (a block the row records serve
    alone, blk_fast, beside mixed ones), with the row records in use (resp_q
    and resp_rows set: the qfast launch); and the same with the rows from the
    currents (od_row_records=False), equal within 1e-12 rel."""
    ti = C.HET
    ts = pd.Timestamp(C.TIMES[ti][0])
    rescale = C.TIMES[ti][1]
    s, cur = _solvers(rescale)["table"], _new_solver(rescale)
    cur.od_row_records = False
    _solve(s, ti, np.zeros(C.K), None)                       # the hour's tables
    P0 = C.ladder()
    P1 = P0.copy()
    P1[:256] = _served_block(s, ts, 256)
    for P in (P0, P1):
        v, it = _solve(s, ti, P, None)
        rows = [v[i].cpu().numpy() for i in [s.feeder.node_names.index(nm) for nm in s.output_names]]
        vmn, vmx = rows[0].copy(), rows[0].copy()
        for r in rows[1:]:
            vmn = np.where(r < vmn, r, vmn)
            vmx = np.where(r > vmx, r, vmx)
        lo, hi = s.voltage_extrema()
        assert np.array_equal(lo.cpu().numpy(), vmn) and np.array_equal(hi.cpu().numpy(), vmx)
        mn, mx, it_x, od = _extrema_only(s, ts, P)
        assert od.resp_q and od.resp_rows != 0 and od.resp_q_rows != 0, "row records not in use: no qfast launch"
        assert torch.equal(it_x, it)
        assert torch.equal(mn, lo) and torch.equal(mx, hi)
        assert (it < 0).any() and float(lo.min()) < 0.5 and float(hi.max()) > 1.25
        _solve(cur, ti, P, None)
        mn_c, mx_c, it_c, od_c = _extrema_only(cur, ts, P)
        assert not od_c.resp_q
        assert torch.equal(it_c, it)
        assert _rel(mn, mn_c) < 1e-12 and _rel(mx, mx_c) < 1e-12, (_rel(mn, mn_c), _rel(mx, mx_c))


def test_offgrid_stale_row_set_after_node_records_off():
    """The row-record row set against the node-record flag: the tables built
    with node records, od_node_records switched off and only the tables cache
    cleared.  The row set then cached left out the node record's row (675.3),
    which no longer has a record to read: the extrema-only solve of served
    blocks must not take it as 0 V.  vmin equals the solve with the rows from
    the currents within 1e-12 rel and stays above 0.3 pu."""
    ti, n = C.HET, 130
    ts = pd.Timestamp(C.TIMES[ti][0])
    rescale = C.TIMES[ti][1]
    s, cur = _new_solver(rescale, num_envs=n), _new_solver(rescale, num_envs=n)
    cur.od_row_records = False
    for x in (s, cur):
        _solve(x, ti, np.zeros(n), None)                     # the hour's tables
    P = _served_block(s, ts, n)
    _, _, _, od = _extrema_only(s, ts, P)
    assert od.resp_q and od.resp_v and od.resp_v_row > 0
    s.od_node_records = False
    s._tables_cache.clear()
    mn, mx, it, od = _extrema_only(s, ts, P)
    assert not od.resp_v and od.resp_v_row == -1
    mn_c, mx_c, it_c, _ = _extrema_only(cur, ts, P)
    assert torch.equal(it, it_c)
    assert float(mn.min()) > 0.3, float(mn.min())
    assert _rel(mn, mn_c) < 1e-12 and _rel(mx, mx_c) < 1e-12, (_rel(mn, mn_c), _rel(mx, mx_c))


# ------------------------------------------------------------------ step level
# The outputs that read V675.3, name: (rtol, atol).  An env the table serves
# takes it from its node record, fitted to the solve within 1e-11 rel (the
# table's bound, tests/test_gpu_pf_od.py), so against the step without a table
# (every env solved) these outputs are bit-identical for the envs the table
# leaves and, for the ones it serves (V < 1.1 pu there, asserted): V within
# 1e-11 rel; the violation max(0, 0.95 - v, v - 1.05) within |dv| <= 1.1e-11;
# a reward within VV_UNIT_PENALTY = 1e4 times that over the agents (divided
# where used), plus its own rounding.
_FROM_V = {"V675c": (1e-11, 0.0), "voltage_violation": (0.0, 1.1e-11), "rewards": (1e-14, 1.1e-7)}


def _step_envs(n, agents, max_power, kinds):
    """Fused C4 envs on the step scenario: "one" the one-launch step, "two"
    the two-kernel step, "solve" the two-kernel step without a table,
    "generic" the component kernels (fused=False)."""
    from powergridworld_amd.scenarios.coordinated import CoordinatedMultiBuildingControlEnv
    envs = []
    for kind in kinds:
        env = CoordinatedMultiBuildingControlEnv(**C.step_env_config(agents, max_power), num_envs=n, device=DEV,
                                                 fused=kind != "generic")
        if kind == "generic":
            assert env._fused is None
        else:
            assert env._fused is not None and env._fused["kernel"] == "pgw_coord_step" and env.pf_solver._od_fast
            env.set_pf_list(kind == "one")
            if kind == "one":
                assert env._one_launch_ok()
            if kind == "solve":
                env.pf_solver.od_table = False
        envs.append(env)
    return envs


def _step_reset(envs):
    n = envs[0].num_envs
    soc = torch.full((n,), C.STEP_SOC, dtype=torch.float64, device=DEV)
    for env in envs:
        env.reset()
        for agent in env.agents:
            agent.env_dict["storage"].reset(init_storage=soc)
        env.load_component_state()


def _bus_load(agent_power):
    """The kernels' bus load: 0 + p0 + p1 + ... in agent order."""
    ap = agent_power.cpu().numpy()
    load = np.zeros(ap.shape[1])
    for a in range(ap.shape[0]):
        load = load + ap[a]
    return load


def _dict_action(env, a):
    return {ag.name: {"building": a[i, :, :6], "pv": a[i, :, 6:7], "storage": a[i, :, 7:8]}
            for i, ag in enumerate(env.agents)}


def _run_steps(envs, kinds, acts, ref=None, generic_steps=0):
    """Step every env on the same actions.  After each step: the fused envs
    bit-identical in every output and the state; the one-launch env's od_count
    equal to the envs its table does not serve; some env stopped by the cap;
    against the oracle's step `ref[t]` when given.  Returns the out-of-bounds
    actions expected."""
    fused = [e for e, k in zip(envs, kinds) if k != "generic"]
    generic = [e for e, k in zip(envs, kinds) if k == "generic"]
    one = envs[kinds.index("one")]
    n, want = one.num_envs, 0
    for t, act in enumerate(acts):
        a = torch.tensor(act, device=DEV)
        want += int(_bad(a[:, :, :6]).any(2).sum() + _bad(a[:, :, 6]).sum() + _bad(a[:, :, 7]).sum())
        outs = []
        for env in fused:
            _, r, _, m = env.step(a)
            outs.append(_outputs(env, r, m))
        torch.cuda.synchronize()
        F = one._fused
        par = F["bufs"].od_parity & 1
        cnt = [int(c) for c in F["od_count"][:2]]
        load = _bus_load(outs[0][5])
        solver = one.pf_solver
        unserved = ~_served(solver, solver.hour_of(one.time), load)
        assert unserved[~C.in_grid(load)].all()
        un = torch.tensor(unserved, device=DEV)
        assert float(outs[0][3][~un].max()) < 1.1            # (_FROM_V's bound on a served env's V)
        for k, o in zip([kd for kd in kinds if kd != "generic"][1:], outs[1:]):
            for nm, x, y in zip(NAMES, outs[0], o):
                if k == "solve" and nm in _FROM_V:
                    # without a table every env is solved: the envs the table serves
                    # differ from their records by the table's fit (_FROM_V)
                    bad = (x != y)[..., un]
                    assert not bad.any(), "one vs solve: step %d, %s (%d unserved differ)" % (t, nm, int(bad.sum()))
                    rtol, atol = _FROM_V[nm]
                    atol = atol / len(one.agents) if nm == "rewards" else atol
                    torch.testing.assert_close(x[..., ~un], y[..., ~un], rtol=rtol, atol=atol,
                                               msg=lambda m: "one vs solve: step %d, %s, served envs: %s" % (t, nm, m))
                else:
                    assert torch.equal(x, y), "%s vs %s: step %d, %s (%d differ)" % (
                        kinds[0], k, t, nm, int((x != y).sum()))
        assert cnt[par] == int(unserved.sum()) and cnt[par ^ 1] == 0, (t, cnt, par, int(unserved.sum()))
        assert 0 < cnt[par] < n, (t, cnt)
        its = outs[0][4].cpu().numpy()
        assert (its < 0).any(), "step %d: no env stopped by the cap" % t
        if t < generic_steps:
            for env in generic:
                og, rg, _, mg = env.step(_dict_action(env, a))
                obs_g = torch.stack([torch.cat([og[ag.name][c] for c in ("building", "pv", "storage")], 1)
                                     for ag in env.agents])
                assert torch.equal(obs_g, outs[0][0]), "generic vs fused: step %d, obs" % t
                assert torch.equal(torch.stack([rg[ag.name] for ag in env.agents]), outs[0][1]), \
                    "generic vs fused: step %d, rewards" % t
                assert torch.equal(mg["voltage_violation"], outs[0][2]), "generic vs fused: step %d, violation" % t
                assert torch.equal(env.pf_solver.iterations, outs[0][4]), "generic vs fused: step %d, iterations" % t
        if ref is not None:
            w = ref[t]
            np.testing.assert_allclose(load, w["load"], rtol=1e-12, atol=1e-9, err_msg="step %d bus load" % t)
            np.testing.assert_array_equal(np.abs(its), w["iterations"], err_msg="step %d" % t)
            np.testing.assert_array_equal(its < 0, ~w["last_converged"], err_msg="step %d" % t)
            np.testing.assert_allclose(outs[0][0].cpu().numpy(), w["obs"], rtol=1e-10, atol=1e-10,
                                       err_msg="step %d obs" % t)
            np.testing.assert_allclose(outs[0][1].cpu().numpy(), w["rewards"], rtol=1e-7, atol=1e-7,
                                       err_msg="step %d rewards" % t)
            np.testing.assert_allclose(outs[0][3].cpu().numpy(), w["v"], rtol=1e-10, atol=0,
                                       err_msg="step %d V675c" % t)
            np.testing.assert_allclose(outs[0][2].cpu().numpy(), w["voltage_violation"], rtol=1e-8, atol=1e-11,
                                       err_msg="step %d violation" % t)
    return want


def _check_oob(envs, want):
    got = [int(env.oob_actions().item()) for env in envs]
    assert want > 0 and got == [want] * len(envs), (got, want)


@pytest.mark.parametrize("n,agents,max_power", C.STEP_SHAPES)
def test_offgrid_step_every_path_vs_oracle(n, agents, max_power):
    """The fused C4 step with bus loads of -7.4 .. 6.2 MW, six steps: the
    one-launch step (the lookup wave's od_wave_solve for ~85 % of the envs,
    beside served lanes) and the two-kernel step agree bit for bit in every
    output, the state and the out-of-bounds count; so does the two-kernel step
    without a table, but for the outputs that read V675.3 of an env the table
    serves, which are within the table's fit (_FROM_V: a served env's record
    is no bit copy of its solve); od_count is the number of envs the table
    does not serve; some env
    stops at the cap every step; observations, rewards, V675.3, the violation
    and the signed iteration counts match the C4 oracle with the same battery.
    At n = 193 the generic path (fused=False) joins for three steps, bit for
    bit in observations, rewards, violation and iterations."""
    kinds = ["one", "two", "solve"] + (["generic"] if n == 193 else [])
    envs = _step_envs(n, agents, max_power, kinds)
    _step_reset(envs)
    want = _run_steps(envs, kinds, C.step_actions(n, agents), ref=C.step_reference(n, agents, max_power),
                      generic_steps=3)
    _check_oob(envs[:3], want)


def test_offgrid_step_across_reset():
    """Three steps, reset(), three more (the action stream going on): x_k and
    the SoC equal after the reset, every output after every step."""
    n, agents, max_power = C.STEP_SHAPES[0]
    kinds = ["one", "two"]
    envs = _step_envs(n, agents, max_power, kinds)
    _step_reset(envs)
    want = _run_steps(envs, kinds, C.step_actions(n, agents, 3), ref=C.step_reference(n, agents, max_power))
    _step_reset(envs)
    F = [env._fused for env in envs]
    assert torch.equal(F[0]["x"], F[1]["x"]) and torch.equal(F[0]["soc"], F[1]["soc"])
    more = _run_steps(envs, kinds, C.step_actions(n, agents, 3, skip=3))
    _check_oob(envs, want + more)


# ------------------------------------------------------------------ the list form
def test_offgrid_step_list_form_in_child_process():
    """PGW_STEP_LIST=1 (k_coord_step_od<.., false> + k_coord_pf_od_list) is read
    when the library loads: a fresh process runs tests/_step_list_child.py --
    the n = 193 comparison on the step scenario and on make_c4_config() with a
    third of the records unfit, the default fused step against the two-kernel
    step, the list and its count checked against the unserved envs."""
    p = subprocess.run([sys.executable, "-m", "tests._step_list_child"], env={**os.environ, "PGW_STEP_LIST": "1"},
                       cwd=REPO, timeout=240, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, "tests._step_list_child exited %d:\n%s" % (p.returncode, p.stdout[-4000:])
    assert "list form ok" in p.stdout, p.stdout[-4000:]
