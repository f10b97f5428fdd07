"""The EV station kernels against tests/_ev_direct_common.ev_step_ref at the
word, chunk and wave edges: every env at every step of an episode, from the
same pre-step state.  The new requirements, the charging words and the
vehicle count (obs column 1) bit for bit; the other outputs within the
derived bound B of _ev_direct_common's docstring (fp32 storage: inside
[RN32(ref - B), RN32(ref + B)]); the out-of-bounds counter equal to the
reference's count.

    walk      pgw_ev_step / pgw_ev_step_f32 through EVChargingEnv (k_ev_step:
              kEvTable in whole waves, kEvDivide in the partial one, kEvPerEnv
              for randomize), 1 .. 16 words, 1 .. 128 chunks
    partial   a partial wave's env (kEvDivide) == a whole wave's (kEvTable)
              given the same actions, and tl_rcp = NULL in whole waves too
    lanes     pgw_ev_step_lanes through the ABI at its 7 (LPE, W) x 3 modes,
              197 envs (no envs-per-wave value divides it)
    mc        pgw_mc_agent_step(_f32), the walk in one lane and split over 8
              waves (pgw_mc_ev_split_mode 0 / 1), and a 4-step clocked graph
    ma        k_ma_step: the heterogeneous scenario with 129 vehicles

Each test prints `ev-direct <entry> <largest error / B>`.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _ev_direct_common as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TD = {"f64": torch.float64, "f32": torch.float32}
ND = {"f64": np.float64, "f32": np.float32}


def _record(entry, worst):
    print("ev-direct %s %.4f" % (entry, worst))
    assert worst <= 1.0, (entry, worst)


def _csv(c, tmp_path):
    return None if c.table == "shipped" else E.write_csv(E.table_of(c.table), tmp_path / (c.table + ".csv"))


def _make_env(c, storage, tmp_path):
    from powergridworld_amd.agents import EVChargingEnv
    env = EVChargingEnv(num_envs=c.n, device=DEV, dtype=TD[storage], randomize=c.randomize,
                        vehicle_csv=_csv(c, tmp_path), **c.cfg)
    _same_params(env.params, E.station_of(c))
    return env


def _same_params(p, P):
    """The host's pgw_ev_params against the Station's, field by field."""
    assert (p.rate, p.hours_per_step, p.mult, p.u_pen, p.p_pen, p.thr, p.reward_scale) == \
        (P.rate, P.hours, P.mult, P.u_pen, P.p_pen, P.thr, P.scale)
    assert list(p.obs_low) == list(P.obs_low) and list(p.obs_high) == list(P.obs_high)
    assert (p.n_vehicles, p.rescale) == (P.V, int(P.rescale))


def _host(ev):
    """An EVChargingEnv's state and outputs as host arrays, env-major."""
    torch.cuda.synchronize()
    V, W = ev.num_vehicles, (ev.num_vehicles + 63) // 64
    return dict(req=ev.req[:V].t().contiguous().cpu().numpy(),
                words=ev.charging[:W].t().contiguous().cpu().numpy().view(np.uint64),
                obs=ev._obs.contiguous().cpu().numpy(), rp=ev._real_power.cpu().numpy(),
                rew=ev._reward.cpu().numpy())


def _compare(got, r, storage, tag):
    """Exact parts exactly, the rest within B; returns the largest error / B."""
    nd = ND[storage]
    assert got["req"].dtype == nd and got["obs"].dtype == nd
    np.testing.assert_array_equal(got["req"], r.req, err_msg="requirements, %s" % (tag,))
    np.testing.assert_array_equal(got["words"], r.words, err_msg="charging words, %s" % (tag,))
    np.testing.assert_array_equal(got["obs"][:, 1], r.obs1.astype(nd), err_msg="vehicle count, %s" % (tag,))
    cols = [0, 2, 3, 4, 5]
    worst = 0.0
    for name, out, ref, B in (("obs", got["obs"][:, cols], r.obs[:, cols], r.B_obs[:, cols]),
                              ("real power", got["rp"], r.rp, r.B_rp), ("reward", got["rew"], r.rew, r.B_rew)):
        q = E.ratio(out, ref, B, storage)
        assert E.within(out, ref, B, storage), "%s, %s: error / B = %g" % (name, tag, q)
        worst = max(worst, q)
    return worst


def _act(a, storage):
    return torch.tensor(np.ascontiguousarray(a.reshape(-1, 1)), dtype=TD[storage], device=DEV)


# ---------------------------------------------------------------- the standalone walk
@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("c", E.WALK_CASES, ids=[c.id for c in E.WALK_CASES])
def test_walk_against_the_reference(c, storage, tmp_path):
    P = E.station_of(c)
    env = _make_env(c, storage, tmp_path)
    acts, ids = E.case_actions(c, P), E.case_ids(c, P)
    worst, oob, most = 0.0, 0, 0
    for ti, step, _, a, r in E.episode_ref(P, acts, storage, ids):
        if ti == 0:
            env.reset(vehicle_ids=ids) if c.randomize else env.reset()
        else:
            env.step(_act(a, storage))
        worst = max(worst, _compare(_host(env), r, storage, (c.id, storage, ti)))
        oob += r.oob
        most = max(most, E.chunks(step.scan))
    assert env.is_terminal() and ti == P.n_steps()
    assert int(env.oob_count) == oob
    if c.table == "dense":
        assert most == 128
    _record("walk %s %s" % (storage, c.id), worst)


def test_walk_with_no_vehicles_writes_an_empty_station():
    """V = 0, one step through the ABI: the outputs are an empty station's and
    the rows around req and charging stay untouched."""
    from powergridworld_amd import _lib
    lib, n = _lib.lib(), 65
    P = E.Station(E.shipped_table(), num_vehicles=0, **dict(E.C3, rescale_spaces=False))
    p, keep = _abi_params(P)
    step = P.step_at(3)
    s, keep2 = _abi_step_info(P, step, "divide", n)
    guard = 3.25
    req = torch.full((3, n), guard, dtype=torch.float64, device=DEV)
    chg = torch.full((3, n), 0x5A5A5A5A, dtype=torch.int64, device=DEV)
    obs = torch.full((6, n), guard, dtype=torch.float64, device=DEV).t()
    rp, rew = (torch.full((n,), guard, dtype=torch.float64, device=DEV) for _ in range(2))
    endp = torch.zeros(1, dtype=torch.float64, device=DEV)
    a = _act(np.full(n, 0.5), "f64")
    _lib.check(lib.pgw_ev_step(p, s, n, _lib.mat(a), _lib.dptr(endp), _lib.dptr(req[1:]), _lib.dptr(chg[1:]),
                               _lib.mat(obs), _lib.dptr(rp), _lib.dptr(rew), _lib.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    r = E.ev_step_ref(P, step, (np.zeros((n, 0)), np.zeros((n, 0), dtype=bool)), np.full(n, 0.5))
    assert bool((req == guard).all()) and bool((chg == 0x5A5A5A5A).all())
    np.testing.assert_array_equal(obs.cpu().numpy(), r.obs.astype(np.float64))
    np.testing.assert_array_equal(obs.cpu().numpy(), np.tile([step.next_time, 0, 0, 0, 0, 0], (n, 1)))
    assert bool((rp == 0).all()) and bool((rew == 0).all())
    assert int(keep[0]) == 0


# ---------------------------------------------------------------- the host's packing at 16 words
@pytest.mark.parametrize("table", ["dense", "sparse"])
def test_step_info_words_at_16_words(table, tmp_path):
    c = E.case(table, 1024, 1)
    P, env = E.station_of(c), _make_env(c, "f64", tmp_path)
    prev = None
    for ti in range(P.n_steps() + 1):
        s, win = env._step_info_at(ti, prev)
        step = P.step_at(ti)
        # independently of words(): bit v of word v // 64, from the table
        want_w, want_s = [0] * 16, [0] * 16
        for v in range(1024):
            t = step.time
            now = P.start[v] <= t <= np.floor(P.endp[v])
            before = ti > 0 and P.start[v] <= P.times[ti - 1] <= np.floor(P.endp[v])
            want_w[v // 64] |= int(now) << (v % 64)
            want_s[v // 64] |= int(now or before) << (v % 64)
        assert s.n_words == 16 and list(s.window) == want_w and list(s.scan) == want_s, ti
        assert [int(x) for x in E.words(step.window)] == want_w and [int(x) for x in E.words(step.scan)] == want_s
        assert (s.time, s.next_time, s.action_default) == (step.time, step.next_time, step.action_default)
        tl = env._tl_rcp[ti].cpu().numpy()
        np.testing.assert_array_equal(tl[:, 0], (P.endp - step.time) / 60.0)
        prev = win


# ---------------------------------------------------------------- a partial wave == a whole wave
@pytest.mark.parametrize("table,V", [("dense", 1024), ("shipped", 129)])
def test_partial_wave_divides_to_the_table_waves_bits(table, V, tmp_path):
    """n = 65: env 64 is alone in the second wave (kEvDivide, IEEE division in
    the kernel), env 0 in a whole one (kEvTable, exact_div from the host's
    reciprocals).  Given the same actions every output is the same bits; and
    the whole batch stepped with tl_rcp = NULL (kEvDivide in a whole wave too)
    returns the bits of the env's own step."""
    from powergridworld_amd import _lib
    lib = _lib.lib()
    c = E.case(table, V, 65, seed=40)
    P, env = E.station_of(c), _make_env(c, "f64", tmp_path)
    acts = E.case_actions(c, P)
    acts[:, 64] = acts[:, 0]
    p2 = type(env.params).from_buffer_copy(env.params)
    p2.oob = None
    env.reset()
    st = _lib.stream_ptr(torch.device(DEV))
    for t in range(P.n_steps()):
        s = env._step_info_at(env.time_index, env._prev_window)[0]
        assert s.tl_rcp and not s.env_start
        s2 = type(s).from_buffer_copy(s)
        s2.tl_rcp = None
        a = _act(acts[t], "f64")
        req2, chg2, obs2 = env.req.clone(), env.charging.clone(), env._new_obs(6)
        rp2, rew2 = torch.zeros_like(env._real_power), torch.zeros_like(env._reward)
        _lib.check(lib.pgw_ev_step(p2, s2, c.n, env._mat(a), _lib.dptr(env._endp_dev), _lib.dptr(req2),
                                   _lib.dptr(chg2), env._mat(obs2), _lib.dptr(rp2), _lib.dptr(rew2), st))
        env.step(a)
        torch.cuda.synchronize()
        for x in (env.req, env.charging):
            assert torch.equal(x[:, 64], x[:, 0]), t
        assert torch.equal(env._obs[64], env._obs[0]) and torch.equal(env._real_power[64], env._real_power[0]), t
        assert torch.equal(env._reward[64], env._reward[0]), t
        for x, y in ((req2, env.req), (chg2, env.charging), (obs2, env._obs), (rp2, env._real_power),
                     (rew2, env._reward)):
            assert torch.equal(x, y), t
    assert env.is_terminal()


# ---------------------------------------------------------------- lanes over vehicles, through the ABI
def _abi_params(P):
    from powergridworld_amd import _lib
    p = _lib.EVParams()
    p.rate, p.hours_per_step, p.mult = P.rate, P.hours, P.mult
    p.u_pen, p.p_pen, p.thr, p.reward_scale = P.u_pen, P.p_pen, P.thr, P.scale
    for j in range(6):
        p.obs_low[j], p.obs_high[j] = P.obs_low[j], P.obs_high[j]
    p.n_vehicles, p.rescale = P.V, int(P.rescale)
    oob = torch.zeros(1, dtype=torch.int64, device=DEV)
    p.oob = oob.data_ptr()
    return p, oob


def _abi_step_info(P, step, mode, n, tables=None):
    """pgw_ev_step_info of a Station step.  mode "table": tl_rcp as pgw.h
    states it, (end_park - time) / 60 and its reciprocal (0 where the time left
    is 0: never divided by); "divide": tl_rcp = NULL; "perenv": `tables`,
    device (env_start, env_endp) in the kernel's layout."""
    from powergridworld_amd import _lib
    s, keep = _lib.EVStepInfo(), None
    s.time, s.next_time, s.action_default, s.n_words = step.time, step.next_time, step.action_default, P.W
    if mode == "perenv":
        s.env_start, s.env_endp = tables[0].data_ptr(), tables[1].data_ptr()
    else:
        for w, x in enumerate(E.words(step.window)):
            s.window[w] = int(x)
        if mode == "table" and P.V:
            tl = (P.endp - step.time) / 60.0
            rc = np.divide(1.0, tl, out=np.zeros_like(tl), where=tl != 0.0)
            keep = torch.tensor(np.ascontiguousarray(np.stack([tl, rc], -1)), device=DEV)
            s.tl_rcp = keep.data_ptr()
    for w, x in enumerate(E.words(step.scan)):
        s.scan[w] = int(x)
    return s, keep


LANES = [(10, 16, 1), (25, 32, 1), (64, 64, 1), (65, 64, 2), (200, 64, 4), (300, 64, 8), (1024, 64, 16)]
LANES_CASES = ([(V, m, 197) for V, _, _ in LANES for m in ("table", "divide")]
               + [(V, "perenv", 197) for V, _, _ in LANES] + [(25, "table", 1), (300, "perenv", 1)]
               + [(1024, "dense-" + m, 197) for m in ("table", "divide", "perenv")])
PAD = -7.5                                  # what the rows' padding columns hold
GUARD, MAX_W = 0x5A5A5A5A5A5A, E.MAX_WORDS   # rows behind the charging words, and what they hold


@pytest.mark.parametrize("V,mode,n", LANES_CASES,
                         ids=["L%dW%d-V%d-%s-n%d" % ([(l, w) for v, l, w in LANES if v == x[0]][0] + x)
                              for x in LANES_CASES])
def test_lanes_against_the_reference(V, mode, n):
    """k_ev_lanes<LPE, W, MODE>: V = 10, 25, 64, 65, 200, 300, 1024 are its 7
    (LPE, W) pairs, table / divide / perenv its 3 modes; the 1024-vehicle dense
    table adds the full scan."""
    from powergridworld_amd import _lib
    lib = _lib.lib()
    table, mode = ("dense", mode[6:]) if mode.startswith("dense-") else ("shipped", mode)
    c = E.case(table, V, n, randomize=mode == "perenv", seed=60 + V % 7)
    P = E.station_of(c)
    row = int(lib.pgw_ev_row(V))
    lpe, W = [(l, w) for v, l, w in LANES if v == V][0]
    assert row == E.ev_row(V) == lpe * W
    p, oob_dev = _abi_params(P)
    acts, ids = E.case_actions(c, P), E.case_ids(c, P)
    dev = lambda x, dt=torch.float64: torch.tensor(np.ascontiguousarray(x), dtype=dt, device=DEV)
    tables = None
    if c.randomize:
        es, ee, _ = P.tables_of(ids)
        tables = (E.rows(dev(es.T), row), E.rows(dev(ee.T), row))
    endp = dev(P.endp)
    st = _lib.stream_ptr(torch.device(DEV))
    worst, oob = 0.0, 0
    for ti, step, (req0, chg0), a, r in E.episode_ref(P, acts, "f64", ids):
        s, keep = _abi_step_info(P, step, mode, n, tables)
        req = E.rows(dev(req0.T), row)
        req[:, V:] = PAD
        # the charging words are n_words rows (not the row's W): guard rows behind them
        chg_all = torch.full((P.W + MAX_W, n), GUARD, dtype=torch.int64, device=DEV)
        chg = chg_all[:P.W]
        chg.copy_(dev(E.words(chg0).view(np.int64).T, torch.int64))
        obs = torch.zeros((6, n), dtype=torch.float64, device=DEV).t()
        rp, rew = torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV)
        am = _lib.mat(_act(a, "f64")) if a is not None else _lib.mat(None)
        _lib.check(lib.pgw_ev_step_lanes(p, s, n, am, _lib.dptr(endp), _lib.dptr(req), _lib.dptr(chg), _lib.mat(obs),
                                         _lib.dptr(rp), _lib.dptr(rew), st))
        torch.cuda.synchronize()
        assert bool((req[:, V:] == PAD).all()), ti
        assert bool((chg_all[P.W:] == GUARD).all()), ti
        got = dict(req=req[:, :V].contiguous().cpu().numpy(),
                   words=chg.t().contiguous().cpu().numpy().view(np.uint64), obs=obs.contiguous().cpu().numpy(),
                   rp=rp.cpu().numpy(), rew=rew.cpu().numpy())
        worst = max(worst, _compare(got, r, "f64", (V, mode, n, ti)))
        oob += r.oob
    assert int(oob_dev[0]) == oob
    _record("lanes<%d,%d> %s %s n%d" % (lpe, W, mode, table, n), worst)


# ---------------------------------------------------------------- the fused agent step
def _mc_env(c, storage, tmp_path):
    from powergridworld_amd import MultiComponentEnv
    from powergridworld_amd.agents import EnergyStorageEnv, EVChargingEnv
    comps = [{"name": "storage", "cls": EnergyStorageEnv, "config": {}},
             {"name": "ev", "cls": EVChargingEnv, "config": dict(c.cfg, vehicle_csv=_csv(c, tmp_path))}]
    env = MultiComponentEnv(name="mc", components=comps, num_envs=c.n, device=DEV, dtype=TD[storage])
    assert env._mc_fusable()
    env.reset(init_storage=torch.linspace(5.0, 45.0, c.n, dtype=TD[storage], device=DEV))
    return env


def _split(mode):
    from powergridworld_amd import _lib
    prev = ctypes.c_int32(0)
    _lib.check(_lib.lib().pgw_mc_ev_split_mode(mode, ctypes.byref(prev)))
    return prev.value


MC_TABLES = [("shipped", 129), ("dense", 1024), ("sparse", 1024)]


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("n", [65, 197])
@pytest.mark.parametrize("split", [0, 1], ids=["unsplit", "split"])
@pytest.mark.parametrize("table,V", MC_TABLES, ids=["%s-V%d" % x for x in MC_TABLES])
def test_mc_agent_step_against_the_reference(table, V, split, n, storage, tmp_path):
    c = E.case(table, V, n, seed=80 + n % 7)
    P = E.station_of(c)
    acts = E.case_actions(c, P)
    gen = torch.Generator(DEV).manual_seed(n)
    before = _split(split)
    try:
        env = _mc_env(c, storage, tmp_path)
        ev, sto = env.env_dict["ev"], env.env_dict["storage"]
        _same_params(ev.params, P)
        worst, oob = 0.0, 0
        for ti, step, _, a, r in E.episode_ref(P, acts, storage):
            if ti:
                sa = torch.rand((n, 1), dtype=torch.float64, device=DEV, generator=gen).to(TD[storage]) * 2 - 1
                env.step({"storage": sa, "ev": _act(a, storage)})
                torch.cuda.synchronize()
                # the agent's power: the components' in order from 0 (base.py:125-156), rounded once
                want = ((0.0 + sto.real_power.double()) + ev.real_power.double()).to(TD[storage])
                assert torch.equal(env.real_power, want), ti
            worst = max(worst, _compare(_host(ev), r, storage, (c.id, split, storage, ti)))
            oob += r.oob
        assert int(env.oob_count) == oob
    finally:
        _split(before)
    _record("mc %s %s %s" % ("split" if split else "unsplit", storage, c.id), worst)


def test_mc_clocked_graph_equals_the_eager_step():
    """capture_step(..., steps=4), device-clocked, at 129 vehicles and 65 envs
    (a partial wave in the second block): every buffer equal to the eager
    fused step's after every replay."""
    c = E.case("shipped", 129, 65, seed=90)
    P = E.station_of(c)
    acts = E.case_actions(c, P)
    ea, eb = _mc_env(c, "f64", None), _mc_env(c, "f64", None)
    gen = torch.Generator(DEV).manual_seed(9)
    bufs = [{"storage": torch.zeros((c.n, 1), dtype=torch.float64, device=DEV),
             "ev": torch.zeros((c.n, 1), dtype=torch.float64, device=DEV)} for _ in range(4)]
    g4 = eb.capture_step(bufs, steps=4, clocked=True)
    assert g4._clocked

    def snap(env):
        ev, sto = env.env_dict["ev"], env.env_dict["storage"]
        return [t.clone() for t in (env._reward, env._real_power, ev.req, ev.charging, ev._obs, ev._real_power,
                                    ev._reward, sto._obs, sto._real_power, sto.soc)]
    for rnd in range(P.n_steps() // 4):
        for k in range(4):
            bufs[k]["storage"].uniform_(-1, 1, generator=gen)
            bufs[k]["ev"].copy_(_act(acts[4 * rnd + k], "f64"))
            ea.step(bufs[k])
        g4()
        torch.cuda.synchronize()
        for i, (x, y) in enumerate(zip(snap(ea), snap(eb))):
            assert torch.equal(x, y), (rnd, i)
    assert int(ea.oob_count) == int(eb.oob_count)


# ---------------------------------------------------------------- the fused multi-agent step
def test_ma_step_ev_agent_against_the_reference():
    """k_ma_step: the heterogeneous scenario with the EV agent at 129 vehicles
    (3 words, up to 14 chunks), 65 envs, one episode."""
    from powergridworld_amd.multiagent_env import MultiAgentEnv
    from powergridworld_amd.scenarios.heterogeneous import make_env_config
    n = 65
    cfg = make_env_config()
    ev_cfg = [a for a in cfg["agents"] if a["name"] == "ev-charging"][0]["config"]
    ev_cfg["num_vehicles"] = 129
    env = MultiAgentEnv(**cfg, num_envs=n, device=DEV)
    assert env._ma is not None, "the scenario left the fused multi-agent path at 129 vehicles"
    ev = env.agent_dict["ev-charging"]
    P = E.Station(E.shipped_table(), **ev_cfg)
    _same_params(ev.params, P)
    acts = E.actions(95, P.n_steps(), n)
    gen = torch.Generator(DEV).manual_seed(5)
    worst, done, steps = 0.0, False, 0
    for ti, step, _, a, r in E.episode_ref(P, acts, "f64"):
        if done:
            break
        if ti == 0:
            env.reset()
        else:
            o = torch.rand((n, 9), dtype=torch.float64, device=DEV, generator=gen) * 2 - 1
            obs, _, d, _ = env.step({"building": {"building": o[:, :6], "pv": o[:, 6:7], "storage": o[:, 7:8]},
                                     "pv": o[:, 8:9], "ev-charging": _act(a, "f64")})
            done = bool(d["__all__"])
            torch.cuda.synchronize()
            assert torch.equal(obs["ev-charging"], ev._obs)
        worst = max(worst, _compare(_host(ev), r, "f64", ("ma", ti)))
        steps += 1
    assert done and steps > 250, (done, steps)
    _record("ma f64 shipped-V129-n65", worst)
