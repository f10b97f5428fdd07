"""The restated Home-Steward house of tests/_hs_direct_common.py against the
reference's recorded runs, and the coverage of the direct GPU test's cases.
No GPU.

    golden replay   hs_scenario, hs_order and every hs_edges_* golden through
                    house_ref in the reference's own order ("set"): every
                    field within rtol / atol 1e-12 (the tolerance of the
                    end-to-end HS golden tests), the vehicle lists equal to
                    the recorded ones element for element; prints the
                    bit-equal count per field
    order effect    the same replays in the library's order ("ascending"):
                    still within 1e-12; prints the worst difference in ulps
                    and the share of env-steps that differ at all
    coverage        every counter of COUNTERS non-zero over the golden
                    replays and, separately, over the GPU test's case lists
    no raising      none of the GPU test's cases meets the reference's
                    ZeroDivisionError, except the named exhaustion case
"""
import numpy as np
import pytest

from tests import _hs_direct_common as H

TOL = 1e-12

def _ulps(a, b):
    """|a - b| in units of the spacing at b (0 where both are NaN or equal)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(a - b) / np.spacing(np.maximum(np.abs(b), np.finfo(np.float64).tiny))
    return np.where((a == b) | (np.isnan(a) & np.isnan(b)), 0.0, d)


@pytest.fixture(scope="module")
def replays():
    out = {}
    for name in H.golden_names():
        cov = {}
        out[name] = (H.replay(name, "set", cov), H.replay(name, "ascending"), cov)
    return out


def test_golden_names():
    names = H.golden_names()
    assert names[:2] == ["hs_scenario", "hs_order"] and len(names) >= 6, names


def test_golden_replay_reference_order(replays):
    for name, (r, _, _) in replays.items():
        assert r.raises == 0, name
        for k, (mine, gold) in r.fields.items():
            eq, size = H.count_bit_equal(mine, gold)
            print("hs-ref %s %s bit-equal %d / %d" % (name, k, eq, size))
            np.testing.assert_allclose(mine, gold, rtol=TOL, atol=TOL, equal_nan=True, err_msg="%s %s" % (name, k))
        g = r.golden
        if "charging" in g:
            for t, e, chg, dep in r.lists:
                assert chg == [int(i) for i in g["charging"][t, e] if i >= 0], (name, t, e)
                assert dep == [int(i) for i in g["departed"][t, e] if i >= 0], (name, t, e)


def test_order_effect(replays):
    """The library's order against the reference's run: the vehicle sums, the
    mean deficit and unserved ** 2 (see _hs_direct_common).  Printed, and held
    to the goldens' 1e-12."""
    worst, differ, steps, unsorted_lists, lists = 0.0, 0, 0, 0, 0
    for name, (r_set, r_asc, _) in replays.items():
        g = r_asc.golden
        A = g["actions"]
        per = A.shape[0] // int(g["episodes"])
        stepped = [i for i in range((per + 1) * int(g["episodes"])) if i % (per + 1)]     # obs rows of steps
        w_name, rows = 0.0, np.zeros(A.shape[:2], dtype=bool)
        for k, (mine, gold) in r_asc.fields.items():
            np.testing.assert_allclose(mine, gold, rtol=TOL, atol=TOL, equal_nan=True, err_msg="%s %s" % (name, k))
            u = _ulps(mine, r_set.fields[k][0])
            w_name = max(w_name, float(u.max()))
            u = u if u.shape[0] == A.shape[0] else u[stepped]
            rows |= (u.reshape(u.shape[0], u.shape[1], -1) > 0).any(axis=2)
        d = int(rows.sum())
        for _, _, chg, dep in r_set.lists:
            lists += 1
            unsorted_lists += chg != sorted(chg) or dep != sorted(dep)
        print("hs-ref order-effect %s worst %.2f ulp, %d of %d env-steps differ" % (name, w_name, d, r_asc.steps))
        worst, differ, steps = max(worst, w_name), differ + d, steps + r_asc.steps
    print("hs-ref order-effect all worst %.2f ulp, %d of %d env-steps differ (%.2f%%); %d of %d recorded vehicle "
          "lists are not ascending" % (worst, differ, steps, 100.0 * differ / steps, unsorted_lists, lists))
    assert steps > 0


def test_coverage_goldens(replays):
    total = {}
    for name, (_, _, cov) in replays.items():
        H.merge_cov(total, cov)
        print("hs-ref coverage %s %s" % (name, {k: cov.get(k, 0) for k in H.COUNTERS}))
    missing = [k for k in H.COUNTERS if not total.get(k, 0)]
    assert not missing, missing
    edges = {}
    for name in H.golden_names()[2:]:
        H.merge_cov(edges, replays[name][2])
    low = replays["hs_edges_a"][2]
    assert low.get("nact_ge2", 0) and not low.get("veh_ge32", 0)       # the config whose active rows are all < 8
    assert edges.get("veh_ge32", 0) and edges.get("veh63", 0)


@pytest.fixture(scope="module")
def gpu_cases():
    """The GPU test's case lists at n = 65 (fp64 storage), references only."""
    return {c.id: H.episode(c.id, 65, "f64", True) for c in H.CASES + [H.EXHAUSTION]}


def test_coverage_gpu_cases(gpu_cases):
    total = {}
    for cid, (P, c, recs, cov) in gpu_cases.items():
        if cid != H.EXHAUSTION.id:
            H.merge_cov(total, cov)
    print("hs-ref coverage gpu-cases %s" % {k: total.get(k, 0) for k in H.COUNTERS})
    missing = [k for k in H.COUNTERS if not total.get(k, 0)]
    assert not missing, missing
    assert {c.id for c in H.REDUCED} <= set(gpu_cases) and len(H.REDUCED) >= 3
    # shapes, chains and nullable buffers the issue names
    veh = {c.kw["n_veh"] for c in H.CASES if H.EV in c.chain}
    dev = {c.kw["n_dev"] for c in H.CASES if H.DEVICES in c.chain}
    assert {0, 1, 2, 33, 64} <= veh and {1, 3, 4} <= dev, (veh, dev)
    chains = {c.chain for c in H.CASES}
    assert len([ch for ch in chains if len(ch) == 4]) == 6 and len([ch for ch in chains if len(ch) < 4]) == 14
    for null in ("meta_out", "step_meta", "pv_power_last"):
        assert any(null in c.nulls for c in H.CASES) and any(null not in c.nulls for c in H.CASES)
    assert {tuple(c.rescale) for c in H.CASES if len(c.chain) == 4} >= {(1, 1, 1, 1), (0, 0, 0, 0), (1, 0, 1, 0)}
    assert {c.kw.get("grid_aware", 0) for c in H.CASES} == {0, 1}
    # windows with bits 31, 32 and 63 set at once
    P, c, recs, _ = gpu_cases["chain-PSED"]
    assert any((r.s.ev_window >> 31) & (r.s.ev_window >> 32) & (r.s.ev_window >> 63) & 1 for r in recs)


def test_no_raising_cases(gpu_cases):
    flagged = total = 0
    for cid, (P, c, recs, _) in gpu_cases.items():
        if cid == H.EXHAUSTION.id:
            continue
        for r in recs:
            flagged += int(r.ref.raises.sum())
            total += r.ref.raises.size
    print("hs-ref raising share of the GPU cases: %d of %d" % (flagged, total))
    assert flagged == 0 and total > 0
    P, c, recs, _ = gpu_cases[H.EXHAUSTION.id]
    mixed = 0
    for r in recs:
        bad = r.ref.raises
        assert np.isnan(r.ref.dev_cost[bad] + r.ref.soc_cost[bad]).all()
        mixed += 0 < int(bad.sum()) < 65
    assert mixed > 0                          # launches in which some envs raise and the others do not


def test_window_bits_reach_the_struct():
    """1 << v for v = 31, 32, 63 (HSEVChargingEnv.window builds the mask with
    Python ints) survives the assignment to pgw_hs_step_info.ev_window."""
    from powergridworld_amd import _lib
    P = H.synth_house(0, (H.PV, H.EV), (1, 1), n_veh=64, high=(31, 32, 63))
    s = H.info_at(P, 1, 10.0, 15.0)
    want = (1 << 31) | (1 << 32) | (1 << 63)
    assert s.ev_window & want == want
    i = H.hs_info(s)
    assert int(i.ev_window) == s.ev_window and int(i.ev_window) >> 63 == 1
    assert _lib.HSStepInfo.ev_window.size == 8
