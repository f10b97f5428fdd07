"""The inputs of tests/test_gpu_pf_offgrid.py, checked on the oracle alone
(oracle/pf_oracle.py Feeder.snap_opendss, no GPU): the ladder and the step
scenario of tests/_offgrid_common.py really leave the operating region of the
rest of the suite -- iteration counts up to the cap of 15, envs stopped by the
cap, loads above vmaxpu and below vminpu, V675.3 below Vlowpu -- and no env is a
knife edge: moving every kW by +-1e-7 changes no iteration count and no
convergence flag, so a kernel that differs from the oracle by rounding cannot
land on the other side of a decision, and the GPU tests exclude no env."""
import numpy as np
import pytest

from tests import _offgrid_common as C

C4_TIMES = [i for i, (_, rescale) in enumerate(C.TIMES) if rescale == 1.2]


def test_ladder_shape_and_grid_edges():
    x0, h, n = C.grid()
    end = x0 + (n - 1) * h
    P = C.ladder()
    assert P.shape == (C.K,) and C.K % 256 not in (0, 1) and C.K > 3 * 256
    assert P.min() == C.LADDER_LO and P.max() == C.LADDER_HI
    for v in (x0, np.nextafter(x0, -np.inf), np.nextafter(x0, 0.0), end, np.nextafter(end, 0.0),
              np.nextafter(end, np.inf)):
        assert (P == v).sum() == 1, v
    assert (P == 0.0).sum() == 2 and np.signbit(P[P == 0.0]).sum() == 1       # 0.0 and -0.0
    # the kernels' grid test at the edges: x0 inside, the end and beyond outside
    # (the last value below the end rounds onto it in (P - x0) / h: either side
    # is right there, the GPU tests take the kernels' own formula)
    assert C.in_grid([x0, np.nextafter(x0, 0.0), 0.0, -0.0]).all()
    assert not C.in_grid([np.nextafter(x0, -np.inf), end, np.nextafter(end, np.inf)]).any()
    # every 64-lane wave of the launch mixes lanes inside and outside the grid
    inside = C.in_grid(P)
    for w in range(0, C.K, 64):
        s = inside[w:w + 64]
        assert 0 < s.sum() < len(s), (w, int(s.sum()))


@pytest.mark.parametrize("ti", C4_TIMES)
def test_ladder_reaches_cap_and_every_load_band(ti):
    """Q = 0 pass at rescale 1.2: every count 4..15, a quarter of the envs at
    the cap, envs stopped unconverged and an env converged exactly at the cap's
    neighbourhood, loads above vmaxpu and below vminpu, and at hour 0 V675.3
    below Vlowpu."""
    f = C.feeder(ti)
    V, pu, it, conv = C.oracle_ladder(ti, "q0")
    assert np.isfinite(pu).all()
    assert set(range(4, 16)) <= set(np.unique(it).tolist()), np.bincount(it)
    assert (it == 15).mean() >= 0.25
    assert (~conv).any() and (~conv <= (it == 15)).all()      # unconverged only at the cap
    assert conv[it < 15].all()
    load_nodes = sorted({int(i) for i in f.elem_p})
    assert (pu[:, load_nodes] > 1.05).any()
    U = np.abs(V @ f.Cinc.T) / f.elem_vbase                     # the loads' own voltages, pu
    vmin, vmax, vlow = (np.array(a)[f.elem_load] for a in (f.load_vmin, f.load_vmax, f.load_vlow))
    assert (U > vmax).any() and ((U <= vmin) & (U > vlow)).any()
    if ti == 0:
        assert (pu[:, f.idx["675.3"]] < 0.5).any()
        assert (U <= vlow).any()                                # the m2 <= lo2 branch


@pytest.mark.parametrize("ti", range(len(C.TIMES)))
@pytest.mark.parametrize("which", C.PASSES)
def test_ladder_has_no_knife_edge(ti, which):
    P = C.ladder()
    _, pu, it, conv = C.oracle_ladder(ti, which)
    assert (~conv).any() and (it < 15).any()
    worst = 0.0
    for d in (C.EDGE, -C.EDGE):
        _, pu_d, it_d, conv_d = C.oracle_solve(ti, P + d, C.ladder_q(P, which))
        np.testing.assert_array_equal(it_d, it)
        np.testing.assert_array_equal(conv_d, conv)
        worst = max(worst, float((np.abs(pu_d - pu) / pu).max() / C.EDGE))
    print("largest relative node change per kW: %.3e" % worst)
    assert worst <= 1e-2, worst


@pytest.mark.parametrize("n,agents,max_power", C.STEP_SHAPES)
def test_step_scenario_mix_and_no_knife_edge(n, agents, max_power):
    """The six bus-load vectors of each step shape: envs inside and outside
    the grid, envs at the cap and stopped by it, everything finite, and no
    count or flag moved by +-1e-7 kW."""
    ref = C.step_reference(n, agents, max_power)
    assert len(ref) == C.STEPS
    for t, r in enumerate(ref):
        load = r["load"]
        inside = C.in_grid(load)
        assert 0 < inside.sum() < n, (t, int(inside.sum()))
        assert (r["iterations"] == 15).any() and (~r["last_converged"]).any(), t
        assert all(np.isfinite(r[k]).all() for k in ("obs", "rewards", "voltage_violation", "v")), t
        assert load.min() < -5000.0 and load.max() > 5000.0, (t, load.min(), load.max())
        ti = 0 if r["time"].hour == 0 else None
        assert ti is not None, r["time"]
        _, pu, it, conv = C.oracle_solve(ti, load)
        np.testing.assert_array_equal(it, r["iterations"])
        np.testing.assert_array_equal(conv, r["last_converged"])
        for d in (C.EDGE, -C.EDGE):
            _, pu_d, it_d, conv_d = C.oracle_solve(ti, load + d)
            np.testing.assert_array_equal(it_d, it, err_msg="step %d" % t)
            np.testing.assert_array_equal(conv_d, conv, err_msg="step %d" % t)
            assert float((np.abs(pu_d - pu) / pu).max() / C.EDGE) <= 1e-2
    if n == 193:
        assert any((r["v"] < 0.5).any() for r in ref)


@pytest.mark.parametrize("ti", range(len(C.TIMES)))
def test_decider_envs_are_decided_by_a_bounded_row(ti):
    """The envs of the bounded-rows test that od_decide's bounds must not get
    wrong: at each centre the evaluated nodes alone pass the test one
    iteration (or more) before every node does, also 1e-7 kW to either side;
    the ladder around them has envs on both sides of each interval.  On the
    random ladders no env is like this (the bounded rows exceed the evaluated
    ones by at most 5e-7 of tol), so without these envs a bound that always
    decided would go unnoticed."""
    centre, width = C.decider_envs(ti)
    assert len(centre) >= 3 and (width >= C.DECIDER_MIN_WIDTH).all(), (centre, width)
    for d in (0.0, C.EDGE, -C.EDGE):
        it, sub = C.counts_by_rows(ti, centre + d)
        assert (sub < it).all(), (d, it, sub)
    P = C.decider_ladder(ti)
    assert P.shape == (len(centre) * C.DECIDER_POINTS,)
    it, sub = C.counts_by_rows(ti, P)
    per = (sub < it).reshape(len(centre), C.DECIDER_POINTS)
    assert (per.sum(1) >= C.DECIDER_POINTS // 6).all() and not per[:, 0].any() and not per[:, -1].any(), per.sum(1)
    it, sub = C.counts_by_rows(ti, C.ladder())
    assert (sub == it).all()


def test_oracle_last_converged_matches_a_longer_solve():
    """last_converged tells the two kinds of 15 apart: an env is flagged
    unconverged exactly when a solve allowed 16 iterations goes past 15."""
    import pandas as pd
    P = C.ladder()
    _, _, it, conv = C.oracle_ladder(0, "q0")
    t, rescale = C.TIMES[0]
    from oracle.pf_oracle import BatchedPF
    o = BatchedPF(system_load_rescale_factor=rescale, semantics="opendss")
    f = o.feeder
    kw, kvar = o.loads(pd.Timestamp(t), {"675c": P}, None, K=len(P))
    _, it16 = f.snap_opendss(kw, kvar, f.base_kw, f.base_kvar, max_iter=16)
    np.testing.assert_array_equal(it16 > 15, ~conv)
    np.testing.assert_array_equal(np.minimum(it16, 15), it)
    assert ((it == 15) & conv).any()                            # converged exactly at the cap
    assert o.last_converged is None
    o.calculate(t, {"675c": P}, K=len(P))
    np.testing.assert_array_equal(o.last_converged, conv)
    np.testing.assert_array_equal(o.last_iters, it)
