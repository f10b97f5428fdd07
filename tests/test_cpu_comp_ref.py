"""The evidence that the references of tests/_comp_direct_common.py are right,
without a GPU: they replay the reference's own recordings (tests/golden)
within the tolerances tests/test_gpu_parity.py uses for them, equal the
oracle (oracle/pgw_oracle.py) bit for bit on the synthetic cases, and reach
every edge the case lists are built for (the coverage conditions), so that
tests/test_gpu_comp_direct.py cannot pass by never getting there."""
import datetime
import json

import numpy as np
import pytest

from oracle import pgw_oracle as O
from tests import _comp_direct_common as K
from tests.conftest import golden_path


def load(name):
    with np.load(golden_path(name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _report(what, pairs):
    eq = sum(K.count_bit_equal(a, b)[0] for a, b in pairs)
    tot = sum(K.count_bit_equal(a, b)[1] for a, b in pairs)
    print("comp-ref %s bit-equal %d/%d" % (what, eq, tot))
    return eq, tot


# ---------------------------------------------------------------- golden replay
@pytest.mark.parametrize("case", ["default", "norescale", "big"])
def test_battery_golden(case):
    g = load("battery_" + case)
    cfg = json.loads(str(g["config"]))
    lo, hi = cfg.get("storage_range", (3.0, 50.0))
    B = K.Battery(lo, hi, cfg.get("charge_efficiency", 0.95), cfg.get("discharge_efficiency", 0.9),
                  cfg.get("max_power", 15.0), 300 / 3600.0, int(cfg.get("rescale_spaces", True)))
    r = K.battery_reset_ref(B, g["init_storage"])
    np.testing.assert_allclose(r.obs, g["obs"][0], 1e-12, 1e-12)
    pairs = [(r.obs, g["obs"][0]), (r.soc, g["soc"][0])]
    for t in range(g["actions"].shape[0]):
        r = K.battery_step_ref(B, r.soc, g["actions"][t])
        np.testing.assert_allclose(r.obs, g["obs"][t + 1], 1e-12, 1e-12)
        np.testing.assert_allclose(r.rp, g["real_power"][t], 1e-12, 1e-12)
        np.testing.assert_allclose(r.soc, g["soc"][t + 1], 1e-12, 1e-12)
        assert (g["done"][t] == (t + 2 == 288)).all() and (g["reward"][t] == 0.0).all()
        pairs += [(r.obs, g["obs"][t + 1]), (r.rp, g["real_power"][t]), (r.soc, g["soc"][t + 1])]
    _report("golden battery_" + case, pairs)


@pytest.mark.parametrize("case", ["default", "norescale", "offpeak_short"])
def test_pv_golden(case):
    g = load("pv_" + case)
    cfg = json.loads(str(g["config"]))
    data = O.load_pv_profile(cfg["profile_csv"]) * cfg.get("scaling_factor", 1.0)
    length = min(cfg.get("max_episode_steps", len(data)), len(data))
    P = K.PV(-np.max(data), int(cfg.get("rescale_spaces", True)))
    n, pairs = g["actions"].shape[1], []
    for t in range(g["actions"].shape[0]):
        r = K.pv_ref(P, n, data[t], g["actions"][t])
        np.testing.assert_allclose(r.obs, g["obs"][t], 1e-12, 1e-12)
        np.testing.assert_allclose(r.rp, g["real_power"][t], 1e-12, 1e-12)
        assert (g["done"][t] == (t + 1 == length - 1)).all() and (g["reward"][t] == 0.0).all()
        pairs += [(r.obs, g["obs"][t]), (r.rp, g["real_power"][t])]
    _report("golden pv_" + case, pairs)


def _golden_rows(cfg, max_steps):
    """The exogenous rows start_time .. end_time of the recorded frame."""
    with np.load(golden_path("exogenous_synthetic"), allow_pickle=False) as z:
        index, cols, vals = z["index_ns"], [str(c) for c in z["columns"]], z["values"]
    ns = lambda s: int(datetime.datetime.strptime(s, "%m-%d-%Y %H:%M:%S").replace(
        tzinfo=datetime.timezone.utc).timestamp()) * 10 ** 9
    keep = (index >= ns(cfg["start_time"])) & (index <= ns(cfg["end_time"]))
    vals = vals[keep]
    pick = lambda pre: vals[:, [i for i, c in enumerate(cols) if c.startswith(pre)]]
    assert max_steps == len(vals) - 3                                    # five_zone_rom_env.py:97
    return [K.Exo(pick("T_oa")[t, 0], pick("Q_solar")[t], pick("Q_int")[t], pick("Q_cool_")[t], 22.0, 28.0,
                  1.0 * t / max_steps) for t in range(len(vals))]


@pytest.mark.parametrize("case", ["default", "tests_obs", "allobs"])
def test_building_golden_two_episodes(case):
    g0 = load("building_%s_ep0" % case)
    cfg = json.loads(str(g0["config"]))
    max_steps = int(g0["max_episode_steps"])
    rows = _golden_rows(cfg, max_steps)
    M = K.shipped_building(cfg.get("obs_config"), int(cfg.get("rescale_spaces", True)))
    n = g0["actions"].shape[1]
    x = np.tile(K.shipped_x0()[:, None], (1, n))
    pairs_x, pairs_rp = [], []
    for ep in range(2):                              # the second episode: x_k carries over the reset
        g = load("building_%s_ep%d" % (case, ep))
        r = K.building_reset_ref(M, rows[0], x)
        np.testing.assert_allclose(r.obs, g["obs"][0], 1e-10, 1e-10)
        np.testing.assert_allclose(r.x.T, g["x_k"][0], 1e-10, 1e-10)
        for t in range(g["actions"].shape[0]):
            r = K.building_step_ref(M, rows[t], rows[t + 1], r.x, g["actions"][t], r.rstate, 1)
            np.testing.assert_allclose(r.obs, g["obs"][t + 1], 1e-10, 1e-10)
            np.testing.assert_allclose(r.rout, g["reward"][t], 1e-10, 1e-10)
            np.testing.assert_allclose(r.pc, g["real_power"][t], 1e-10, 1e-10)
            np.testing.assert_allclose(r.x.T, g["x_k"][t + 1], 1e-10, 1e-10)
            assert (g["done"][t] == (t + 1 == max_steps - 1)).all()
            pairs_x.append((r.x.T, g["x_k"][t + 1]))
            pairs_rp.append((r.pc, g["real_power"][t]))
        x = r.x
    _report("golden building_%s x_k" % case, pairs_x)
    eq, tot = _report("golden building_%s real_power" % case, pairs_rp)
    # real_power depends on the actions alone: with the exact cube, every value has the recording's bits
    assert eq == tot


# ---------------------------------------------------------------- oracle agreement
def _no_nan(a):
    return np.where(np.isnan(a), 0.3, a)


@pytest.mark.parametrize("c", K.BATTERY_CASES, ids=[c.id for c in K.BATTERY_CASES])
def test_battery_equals_the_oracle(c):
    import pandas as pd
    B = K.Battery(**c.cfg)
    init, act = K.battery_inputs(c, 65)
    o = O.BatteryOracle(65, storage_range=(B.soc_min, B.soc_max), charge_efficiency=B.eta_c,
                        discharge_efficiency=B.eta_d, max_power=B.max_power, rescale_spaces=bool(B.rescale),
                        control_timedelta=pd.Timedelta(round(B.dt_h * 3600), "s"))
    assert o.dt == B.dt_h
    with np.errstate(all="ignore"):
        r = K.battery_reset_ref(B, init)
        K.same_bits(r.obs, o.reset(init), "reset obs")
        K.same_bits(r.soc, o.soc, "reset soc")
        for t in range(c.steps):
            r = K.battery_step_ref(B, r.soc, act[t])
            obs = o.step(act[t][:, None])[0]
            K.same_bits(r.obs, obs, ("obs", t))
            K.same_bits(r.soc, o.soc, ("soc", t))
            K.same_bits(r.rp, o.real_power, ("real power", t))


@pytest.mark.parametrize("c", K.PV_CASES, ids=[c.id for c in K.PV_CASES])
def test_pv_equals_the_oracle(c):
    act, vmin = K.pv_inputs(c, 65)
    profile = np.array(K.PV_PMAX)
    o = O.PVOracle(65, None, profile=profile, rescale_spaces=bool(c.rescale), grid_aware=bool(c.grid_aware))
    P = K.PV(-np.max(profile), c.rescale, c.grid_aware)
    assert P.obs_low == o.obs_low[0]
    with np.errstate(all="ignore"):
        for t, pmax in enumerate(K.PV_PMAX):
            r = K.pv_ref(P, 65, pmax, act[t], vmin)
            obs = o.step(act[t][:, None], vmin)[0]
            K.same_bits(r.obs, obs, ("obs", t))
            K.same_bits(r.rp, o.real_power, ("real power", t))


class ExactCubeOracle(O.BuildingOracle):
    def p_consumed(self, a, t):
        s = (((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]) + a[:, 4]
        return (0.0076 * K.cube(s) + 4.8865) + np.maximum(0., s * (self.T_oa[t] - a[:, 5]))


SHIPPED = [c for c in K.BLD_CASES if c.kind in ("std", "shipped") and c.config]


@pytest.mark.parametrize("c", SHIPPED, ids=[c.id for c in SHIPPED])
def test_building_equals_the_oracle(c, exo_frame):
    """The shipped-model cases (NaN actions replaced: the oracle's np.maximum
    propagates a NaN that Python's max(0, nan), the original's, does not)."""
    n = 65
    M = K.building_of(c)
    rows = K.exo_rows(c.seed, c.steps)
    x0, act, ext_all = K.building_inputs(M, c.seed, n, c.steps)
    ext = {k: v for k, v in ext_all.items() if k in c.ext}
    kw = {{"bus": "bus_voltage", "vmin": "min_voltage", "vmax": "max_voltage", "pset": "p_setpoint"}[k]: v
          for k, v in ext.items()}
    oracles = []
    for cls in (ExactCubeOracle, O.BuildingOracle):
        o = cls(n, exo_frame, obs_config=dict(c.config), rescale_spaces=bool(c.rescale))
        o.T_oa = np.array([r.T_oa for r in rows])
        o.q_solar, o.q_int = np.array([r.q_solar for r in rows]), np.array([r.q_int for r in rows])
        o.q_cool = np.array([r.q_cool for r in rows])
        o.cb = np.array([[r.lb, r.ub] for r in rows])
        o.max_episode_steps = c.steps
        o.x = x0.T.copy()
        oracles.append(o)
    exact, plain = oracles
    free = [j for j, v in enumerate(M.obs_var) if v < 15]             # no p_consumed in them
    with np.errstate(all="ignore"):
        x, rstate = x0, np.zeros(n)
        for _ in range(2):
            r = K.building_reset_ref(M, rows[0], x, ext)
            for o in oracles:
                # (the oracle's reset takes no obs inputs: its obs are formed by get_obs)
                o.reset()
                K.same_bits(r.x.T, o.x, "reset x")
                K.same_bits(r.obs, o.get_obs(**kw), "reset obs")
                K.same_bits(r.rstate, o.step_reward(), "reset reward")
            x, rstate = r.x, r.rstate
        for t in range(c.steps):
            a = _no_nan(act[t])
            r = K.building_step_ref(M, rows[t], rows[t + 1], x, a, rstate, c.lagged, ext)
            obs, rew = exact.step(a, lagged_reward=bool(c.lagged), **kw)[:2]
            K.same_bits(r.obs, obs, ("obs", t))
            K.same_bits(r.rout, rew, ("reward", t))
            K.same_bits(r.pc, exact.real_power, ("p_consumed", t))
            K.same_bits(r.x.T, exact.x, ("x", t))
            obs = plain.step(a, lagged_reward=bool(c.lagged), **kw)[0]
            K.same_bits(r.x.T, plain.x, ("x, NumPy cube", t))
            K.same_bits(M.C * r.x.T + M.mean, plain.T, ("zone temperatures", t))
            K.same_bits(r.obs[:, free], obs[:, free], ("temperature and violation obs, NumPy cube", t))
            x, rstate = r.x, r.rstate


# ---------------------------------------------------------------- coverage conditions
@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_battery_cases_reach_every_edge(storage):
    cov, outside = {}, {0: 0, 1: 0}
    for c in K.BATTERY_CASES:
        for sampled in (0, 1):
            ep = K.battery_episode(c.id, 65, storage, sampled)
            B, init, _, r = ep[0]
            out = (init < B.soc_min) | (init > B.soc_max)
            assert out.any()
            if sampled:
                assert (r.soc[out] == init[out]).all()
            else:
                assert ((r.soc[out] == B.soc_min) | (r.soc[out] == B.soc_max)).all()
            outside[sampled] += int(out.sum())
            for _, _, _, r in ep[1:]:
                K.merge_cov(cov, r.cov)
    print("comp-ref coverage battery %s %s" % (storage, sorted(cov.items())))
    for key in ("dis_clamp", "chg_clamp", "dis_at_bound", "chg_at_bound", "zero_power", "free_dis", "free_chg",
                "nan"):
        assert cov.get(key, 0) > 0, key
    assert outside[0] > 0 and outside[1] > 0


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_pv_cases_reach_every_edge(storage):
    nd = K.ND[storage]
    assert 0.0 in K.PV_PMAX and K.PV_MAX in K.PV_PMAX and any(0.0 < p < 1e-200 for p in K.PV_PMAX)
    for c in K.PV_CASES:
        act, vmin = K.pv_inputs(c, 65, storage)
        for v in K.PINNED + K.BEYOND:
            assert (act == nd(v)).any(), (c.id, v)
        assert np.isnan(act).any()
        assert (vmin < 0.9).any() and (vmin > 1.1).any() and ((vmin > 0.9) & (vmin < 1.1)).any()
    assert {(c.rescale, c.grid_aware) for c in K.PV_CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # beyond the bound by one ulp counts, the bound itself does not (float64 actions)
    P = K.PV(-K.PV_MAX, 1)
    r = K.pv_ref(P, 6, 1.0, np.array(K.PINNED + K.BEYOND))
    assert r.oob == 2


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_building_cases_reach_every_edge(storage):
    cov = {}
    for c in K.BLD_CASES:
        for rec in K.building_episode(c.id, 65, storage)[3]:
            K.merge_cov(cov, rec.ref.cov)
    print("comp-ref coverage building %s %s" % (storage, sorted(cov.items())))
    need = ["%s_%s" % (cls, tag) for cls in ("temp", "upper", "lower", "pcons", "pset")
            for tag in ("below", "above", "inside")]
    need += ["chiller_zero", "chiller_pos", "comfort_negzero", "viol_upper", "viol_lower", "one_nan",
             "reset_reward_negzero"] + ["pinned%d" % k for k in range(4)]
    for key in need:
        assert cov.get(key, 0) > 0, key
    # every u_pos index is selected by one of the synthetic models
    for c in K.BLD_CASES:
        if c.kind == "synth":
            M = K.building_of(c)
            assert set(M.sel.ravel()) == set(range(8)) and not K.bld_is_std_ref(M)
            assert not np.array_equal(M.nbr, K.STD_NBR)
    assert {len(K.building_of(c).obs_var) for c in K.BLD_GEN_CASES} >= {0, 1, 24}


def test_exactly_zero_chiller_term():
    """T_oa = 16.0 and the highest discharge temperature: s * (16 - 16) is an exact zero."""
    M = K.shipped_building(rescale=1)
    a = np.array([[0.1, 0.2, 0.3, 0.4, 0.5, 1.0]])
    with np.errstate(all="ignore"):
        pc, term = K._p_consumed(K.to_raw(a, M.act_low, M.act_high), 16.0)
    assert term[0] == 0.0 and pc[0] > 4.8865


# ---------------------------------------------------------------- helpers
def test_semantics_helpers():
    nan = np.nan
    x = np.array([-2.0, -0.0, 0.0, 0.5, 2.0, nan])
    with np.errstate(all="ignore"):
        K.same_bits(K.clip(x, 0.0, 1.0), np.array([0.0, -0.0, 0.0, 0.5, 1.0, nan]))
        nz = x[[0, 3, 4, 5]]
        K.same_bits(K.clip(nz, 0.0, 1.0), np.clip(nz, 0.0, 1.0))
        for a, b in ((1.0, 2.0), (2.0, 1.0), (0.0, -0.0), (-0.0, 0.0), (nan, 1.0), (1.0, nan)):
            for ours, py in ((K.pymax, max), (K.pymin, min)):
                K.same_bits(ours(np.array([a]), np.array([b])), np.array([py(a, b)]), (py.__name__, a, b))
    assert not K.oob_bad(np.array(K.PINNED)).any() and K.oob_bad(np.array(K.BEYOND + (nan,))).all()


def test_cube_is_correctly_rounded_where_pow_is_not():
    rng = np.random.default_rng(1)
    s = rng.uniform(0.5, 12.0, 20000)
    exact = K.cube(s)
    assert (np.abs(exact - s ** 3) <= np.spacing(exact)).all()
    assert (exact != s * s * s).any()        # the two-rounding product misses some


def test_derived_quantities_and_exact_division():
    """make_bld_derived as restated, and exact_div from them == the IEEE quotient."""
    for cfg in (K.DEFAULT_OBS, {k: K.TIGHT_OBS[k] for k in K.DEFAULT_OBS}):
        M = K.shipped_building(cfg)
        d = K.bld_derived_ref(M)
        np.testing.assert_array_equal(d.act_rng, M.act_high - M.act_low)
        np.testing.assert_array_equal(d.act_sum, M.act_high + M.act_low)
        np.testing.assert_array_equal(d.obs_rng, M.obs_high - M.obs_low)
        np.testing.assert_array_equal(d.obs_sum, M.obs_low + M.obs_high)
        np.testing.assert_array_equal(d.obs_rcp, 1.0 / (M.obs_high - M.obs_low))
        rng = np.random.default_rng(2)
        a = rng.uniform(-1.0, 1.0, (50, 6))
        np.testing.assert_array_equal((a * d.act_rng + d.act_sum) * 0.5, K.to_raw(a, M.act_low, M.act_high))
        for j in range(15):
            for v in list(rng.uniform(M.obs_low[j], M.obs_high[j], 20)) + [M.obs_low[j], M.obs_high[j], -0.0]:
                c = float(K.clip(np.array(v), M.obs_low[j], M.obs_high[j]))
                num = 2.0 * c - d.obs_sum[j]
                got = K.exact_div_ref(num, float(d.obs_rng[j]), float(d.obs_rcp[j]))
                K.same_bits(np.array(got), np.array(num / d.obs_rng[j]), (j, v))
    pc = np.random.default_rng(3).uniform(0.0, 400.0, 200)
    for v in pc:
        K.same_bits(np.array(K.exact_div_ref(-v, 12.0, 1.0 / 12.0)), np.array(-v / 12.0))


def test_standard_layout_detection():
    M = K.shipped_building()
    assert K.bld_is_std_ref(M)
    assert K.bld_is_std_ref(K.shipped_building(rescale=0))
    for c in K.BLD_STD_CASES:
        assert K.bld_is_std_ref(K.building_of(c))
    for c in K.BLD_GEN_CASES:
        assert not K.bld_is_std_ref(K.building_of(c)), c.id

    def perturbed(f):
        P = K.shipped_building()
        f(P)
        return P
    plus = perturbed(lambda P: (P.obs_var.append(K.BV_BUS_VOLTAGE), setattr(P, "obs_low", np.append(P.obs_low, .9)),
                                setattr(P, "obs_high", np.append(P.obs_high, 1.1))))
    assert len(plus.obs_var) == 16 and not K.bld_is_std_ref(plus)
    assert not K.bld_is_std_ref(perturbed(lambda P: P.sel.__setitem__((2, 2), 6)))
    assert not K.bld_is_std_ref(perturbed(lambda P: P.nbr.__setitem__((4, 3), 2)))
    assert not K.bld_is_std_ref(perturbed(lambda P: P.obs_var.__setitem__(3, 0)))
    assert not K.bld_is_std_ref(perturbed(lambda P: P.obs_var.pop()))


def test_reduce_reference_order_matters():
    for n_comp in (1, 3, K.MAX_COMP):
        cols = K.reduce_columns(65, n_comp, 0)
        w, r = K.reduce_ref(list(cols), list(cols[::-1]), 65)
        assert not np.signbit(w[0]) and w[0] == 0.0                     # -0.0 only: 0.0 + -0.0 = +0.0
        if n_comp >= 3:
            assert w[1] == 1.0 and r[1] != 1.0                           # the reversed order loses the 1.0
            assert (w != np.sum(cols, axis=0)).any() or (w != r).any()
    w, r = K.reduce_ref([], [], 5)
    assert (w == 0.0).all() and not np.signbit(w).any()
