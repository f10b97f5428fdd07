"""The fp32-storage Home-Steward house (HSMultiComponentEnv(dtype=torch.float32):
pgw_hs_reset_f32 / pgw_hs_step_f32).  Needs an MI355X.

The contract: every per-env value is widened to fp64 on load, the chain runs
the fp64 house's arithmetic, every store rounds once.  So ONE step (or reset)
of the fp32 house from a given state equals RN32 of the fp64 house's step from
the same (widened) state, value for value, with no tolerance -- tested by
teacher forcing, as test_battery_f32_one_step_and_episode does.  Free-running,
the storage roundings accumulate and branches may flip; there the bound is the
north star's for fp32 (rtol 1e-3 + atol 1e-3) against the reference's own run.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests.conftest import golden_path

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64

NEVER = 1 << 40
_cache = {}


def golden(name):
    if name not in _cache:
        with np.load(golden_path(name), allow_pickle=False) as z:
            _cache[name] = {k: z[k] for k in z.files}
    return _cache[name]


def config(name):
    """(house config, component names) of a golden: hs_scenario = the shipped
    JSON scenario; hs_order = [PV grid-aware, EV, devices, storage]."""
    from powergridworld_amd.scenarios.heterogeneous_hs import make_env_config
    names = [str(x) for x in golden(name)["names"]]
    cfg = make_env_config()
    by = {c["name"]: c for c in cfg["components"]}
    cfg["components"] = [by[n] for n in names]
    if name == "hs_order":
        by["pv"]["config"]["grid_aware"] = True
    return cfg, names


def house(cfg, n, dtype=None, **kw):
    from powergridworld_amd.base_hs import HSMultiComponentEnv
    return HSMultiComponentEnv(**copy.deepcopy(cfg), num_envs=n, device=DEV, dtype=dtype, **kw)


def state_bufs(e):
    """Every per-env state buffer the kernel reads at the next reset / step."""
    st = e.env_dict["storage"]
    return {"soc": st.soc, "soc_cost": st.cost, "ev_req": e._ev_req, "ev_cost": e._ev_cost,
            "dev_cost": e._dev_cost, "es_power_last": e._es_last, "pv_power_last": e._pv_last}


def out_bufs(e):
    return {"obs": e._obs_buf, "reward": e._reward, "real_power": e._real_power, "meta": e._meta,
            "step_meta": e._rec_buf}


def force(e32, e64):
    """Teacher forcing: the fp32 house's whole state, widened, into the fp64 house."""
    for (k, a), b in zip(state_bufs(e32).items(), state_bufs(e64).values()):
        assert a.dtype == F32 and b.dtype == F64 and a.shape == b.shape, k
        b.copy_(a)
    e64._ev_chg.copy_(e32._ev_chg)


class Mismatch:
    """Marks, on the device, the elements where an fp32 buffer is not exactly
    RN32 of its fp64 twin (same bits, or both NaN), and the first step at which
    each did; the buffers of one call are compared as one flat vector, the
    host reads the marks once per episode."""

    def __init__(self):
        self.names = self.first = None

    def check(self, bufs32, bufs64, t):
        """bufs32 / bufs64: {name: tensor}, the same names and shapes; t: step (device scalar)."""
        assert all(a.dtype == F32 and b.dtype == F64 and a.shape == b.shape
                   for a, b in zip(bufs32.values(), bufs64.values()))
        x = torch.cat([a.reshape(-1) for a in bufs32.values()])
        r = torch.cat([b.reshape(-1) for b in bufs64.values()]).to(F32)
        ok = (x.view(torch.int32) == r.view(torch.int32)) | (x.isnan() & r.isnan())
        if self.first is None:
            self.names = [(k, a.numel()) for k, a in bufs32.items()]
            self.first = torch.full(x.shape, NEVER, dtype=torch.int64, device=DEV)
        self.first = torch.minimum(self.first, torch.where(ok, NEVER, t))

    def assert_none(self, where):
        first = self.first.cpu().numpy()
        bad, o = {}, 0
        for k, sz in self.names:
            f = first[o:o + sz]
            o += sz
            if (f != NEVER).any():
                bad[k] = (int((f != NEVER).sum()), int(f.min()))
        assert not bad, "%s: fp32 != RN32(fp64), {buffer: (elements, first step)} = %s" % (where, bad)


def perturbed_actions(g, n, seed):
    """The golden's action stream rounded to fp32 and tiled to n envs, plus
    seeded fp32 noise per env; the exact 0.0 and -1.0 entries (the chain's
    power == 0 / a == 0 branches and the box edge) are left alone."""
    A = g["actions"].astype(np.float32)                          # [T, K, n_comp]
    K = A.shape[1]
    assert n % K == 0
    A = np.tile(A, (1, n // K, 1))
    rng = np.random.default_rng(seed)
    noise = (0.05 * rng.standard_normal(A.shape)).astype(np.float32)
    keep = (A == 0.0) | (A == -1.0)
    out = np.where(keep, A, (A + noise).astype(np.float32)).astype(np.float32)
    assert keep.any() and (out[keep] == A[keep]).all() and (out[~keep] != A[~keep]).any()
    return torch.tensor(out, device=DEV)


def one_step_contract(name, n, seed):
    from powergridworld_amd.base_hs import HS_COMMON_FIELDS
    g = golden(name)
    cfg, names = config(name)
    e32, e64 = house(cfg, n, F32), house(cfg, n)
    assert e32.dtype == F32 and type(e32._bufs).__name__ == "HSBuffersF32" and e64.dtype == F64
    assert all(e.dtype == F32 for e in e32.envs)
    A32 = perturbed_actions(g, n, seed)
    A64 = A32.to(F64)
    grid_aware = bool(e32.params.pv_grid_aware)
    assert grid_aware == (name == "hs_order")
    if grid_aware:
        # a per-env fp64 min_voltage (not fp32-representable), at every reset and step
        rng = np.random.default_rng(seed + 1)
        MV = np.tile(g["min_voltage"], (1, n // g["min_voltage"].shape[1]))
        MV = torch.tensor(MV + 1e-3 * rng.standard_normal(MV.shape), dtype=F64, device=DEV)
        assert not torch.equal(MV.to(F32).to(F64), MV)
    lo, hi = e32.env_dict["storage"].storage_range
    # initial SoC: fp32 values, some outside storage_range (the reset's clip)
    init32 = torch.linspace(lo - 1.0, hi + 1.0, n, dtype=F32, device=DEV)
    mm_reset, mm, chg_bad = Mismatch(), Mismatch(), torch.zeros((), dtype=torch.int64, device=DEV)
    tt = torch.zeros((), dtype=torch.int64, device=DEV)
    t_obs = t_act = 0
    for ep in range(int(g["episodes"])):
        kw = {"min_voltage": MV[t_obs]} if grid_aware else {}
        force(e32, e64)
        o32 = e32.reset(init_storage=init32, **kw)
        o64 = e64.reset(init_storage=init32.to(F64), **kw)
        assert all(o32[k].dtype == F32 and o64[k].dtype == F64 for k in names)
        tt.fill_(ep)
        mm_reset.check({"obs": e32._obs_buf, **state_bufs(e32)}, {"obs": e64._obs_buf, **state_bufs(e64)}, tt)
        chg_bad += (e32._ev_chg != e64._ev_chg).sum()
        t_obs += 1
        while True:
            kw = {"min_voltage": MV[t_obs]} if grid_aware else {}
            force(e32, e64)
            tt.fill_(t_act)
            if t_act % 2:       # packed and dict actions in turn
                r32 = e32.step(A32[t_act], **kw)
                r64 = e64.step(A64[t_act], **kw)
            else:
                r32 = e32.step({k: A32[t_act][:, i:i + 1] for i, k in enumerate(names)}, **kw)
                r64 = e64.step({k: A64[t_act][:, i:i + 1] for i, k in enumerate(names)}, **kw)
            mm.check({**out_bufs(e32), **state_bufs(e32)}, {**out_bufs(e64), **state_bufs(e64)}, tt)
            chg_bad += (e32._ev_chg != e64._ev_chg).sum()
            assert r32[2] == r64[2] == bool(g["done"][t_act, 0])
            if t_act in (0, 100):                               # what the API hands out
                o, r, d, m = r32
                assert all(o[k].dtype == F32 and o[k].shape[0] == n for k in names) and r.dtype == F32
                assert e32.real_power.dtype == F32 and e32.env_dict["storage"].current_storage.dtype == F32
                assert all(m[k].dtype == F32 for k in ("pv_power", "es_power", "grid_power"))
                for rec, rec64 in zip(m["step_meta"], r64[3]["step_meta"]):
                    assert list(rec["device_custom_info"]) == list(rec64["device_custom_info"])
                    vals = [rec[f] for f in HS_COMMON_FIELDS] + list(rec["device_custom_info"].values())
                    assert all(v.dtype == F32 and v.shape == (n,) for v in vals)
            t_obs += 1
            t_act += 1
            if r32[2]:
                break
        mm_reset.assert_none("%s reset %d" % (name, ep))
        mm.assert_none("%s episode %d" % (name, ep))
        assert int(chg_bad) == 0, "ev_charging differs"
        # out-of-bounds actions (the golden's stream leaves [-1, 1]) counted alike
        c32, c64 = int(e32.oob_actions()), int(e64.oob_actions())
        assert c32 == c64 and c32 > 0
    assert t_act == g["actions"].shape[0]


def test_hs_f32_one_step_contract_shipped_scenario():
    """N = 260 = one full 256-lane block plus a 4-lane tail; both episodes
    (crossing the reset), every output and state buffer == RN32(fp64), 0 ulps."""
    import os
    import re
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "powergridworld_amd", "csrc", "pgw_common.h")) as f:
        src = f.read()
    assert int(re.search(r"constexpr int kBlock = (\d+);", src).group(1)) == 256
    one_step_contract("hs_scenario", 260, 11)


def test_hs_f32_one_step_contract_reordered_grid_aware():
    """[PV grid-aware, EV, devices, storage] with a per-env fp64 min_voltage at
    every reset and step (the path that reads pv_power_last and min_voltage);
    N = 261 is odd."""
    one_step_contract("hs_order", 261, 23)


@pytest.mark.parametrize("name", ["hs_scenario", "hs_order"])
def test_hs_f32_free_running_within_north_star_of_reference(name):
    """The fp32 house on its own state against the reference's own run (the
    goldens' batch, actions cast to fp32, both episodes): every observation,
    reward, real power, meta and SoC within rtol 1e-3 + atol 1e-3 at every step."""
    g = golden(name)
    cfg, names = config(name)
    A, O = g["actions"], g["obs"]
    K = A.shape[1]
    env = house(cfg, K, F32, step_meta=False)
    MV = g.get("min_voltage")
    mv = lambda t: {} if MV is None else {"min_voltage": torch.tensor(MV[t], dtype=F64, device=DEV)}
    A32 = torch.tensor(A.astype(np.float32), device=DEV)
    got = {k: [] for k in ("obs", "reward", "real_power", "meta", "soc")}
    soc = env.env_dict["storage"].current_storage
    flat = lambda o: torch.cat([o[n] for n in names], 1)
    rows, t_obs, t_act = [], 0, 0
    for ep in range(int(g["episodes"])):
        o = env.reset(**mv(t_obs))
        reset_obs, reset_soc = flat(o).clone(), soc.clone()
        np.testing.assert_allclose(reset_obs.cpu().numpy(), O[t_obs], 1e-3, 1e-3)
        np.testing.assert_allclose(reset_soc.cpu().numpy(), g["soc"][t_obs], 1e-3, 1e-3)
        t_obs += 1
        while True:
            o, r, d, m = env.step({n: A32[t_act][:, i:i + 1] for i, n in enumerate(names)}, **mv(t_obs))
            got["obs"].append(flat(o).clone())
            got["reward"].append(r.clone())
            got["real_power"].append(env.real_power.clone())
            got["meta"].append(torch.stack([m["pv_power"], m["es_power"], m["grid_power"]], 1))
            got["soc"].append(soc.clone())
            rows.append(t_obs)
            assert d == bool(g["done"][t_act, 0])
            t_obs += 1
            t_act += 1
            if d:
                break
    assert t_act == A.shape[0] == len(rows)
    want = {"obs": O[rows], "reward": g["reward"], "real_power": g["real_power"], "meta": g["meta"][rows],
            "soc": g["soc"][rows]}
    for k, v in got.items():
        x = torch.stack(v).cpu().numpy()
        assert x.dtype == np.float32 and x.shape == want[k].shape, k
        err = np.abs(x.astype(np.float64) - want[k]) / (1e-3 + 1e-3 * np.abs(want[k]))
        print("%s %s: worst error %.4f of the bound (step %d)" % (name, k, np.nanmax(err),
                                                                 np.unravel_index(np.nanargmax(err), err.shape)[0]))
        np.testing.assert_allclose(x, want[k], 1e-3, 1e-3, err_msg=k)


def test_hs_f32_graph_matches_eager_across_reset():
    """8-step graphs of the fp32 house == its eager steps, every output and
    state buffer bit for bit, over more than an episode and a reset, mixed with
    eager steps (as test_hs_graph_matches_eager_across_reset, fp64)."""
    n, steps = 260, 8
    cfg, _ = config("hs_scenario")
    ea, eb = house(cfg, n, F32), house(cfg, n, F32)
    gen = torch.Generator(DEV).manual_seed(12)
    acts = [torch.empty((n, len(ea.envs)), dtype=F32, device=DEV).uniform_(-1, 1, generator=gen)
            for _ in range(steps)]
    init = torch.linspace(0.2, 0.9, n, dtype=F32, device=DEV)
    for e in (ea, eb):
        e.reset(init_storage=init)
    with pytest.raises(ValueError, match="float32"):          # packed actions of the house's dtype
        eb.capture_step([a.to(F64) for a in acts], steps=steps)
    g = eb.capture_step(acts, steps=steps)

    def state(e):
        bufs = list(out_bufs(e).values()) + list(state_bufs(e).values()) + [e._ev_chg]
        assert all(t.dtype == F32 for t in bufs[:-1])
        return [t.detach().cpu().numpy().copy() for t in bufs]

    for ep in range(2):
        calls = 0
        while True:
            da = False
            for a in acts:
                da = ea.step(a)[2] or da
            if calls % 5 == 3:
                db = False
                for a in acts:
                    db = eb.step(a)[2] or db
            else:
                db = g()[2]
            assert da == db
            calls += 1
            if calls % 7 == 0 or da:
                for x, y in zip(state(ea), state(eb)):
                    np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), "ep %d call %d" % (ep, calls))
            if da or eb._hs_step_k() + steps > g._n_dyn:
                break
        for e in (ea, eb):
            e.reset(init_storage=init)
    assert len(g._pos_graphs) > 1


def test_hs_f32_checkpoint_across_reset():
    """Save, run on, restore, replay: the fp32 trajectory comes back bit for bit
    in the same house and in a fresh one; an fp64 house's state is refused."""
    n = 260
    cfg, names = config("hs_scenario")
    make = lambda dtype=F32: house(cfg, n, dtype)
    rng = np.random.default_rng(4)
    acts = [torch.tensor(rng.uniform(-1.1, 1.1, (n, len(names))).astype(np.float32), device=DEV)
            for _ in range(300)]

    def step(env, a):
        o, r, d, m = env.step(a)
        if d:
            env.reset()
        out = [o[k] for k in names] + [r, env.real_power, m["pv_power"], m["es_power"], m["grid_power"]]
        assert all(t.dtype == F32 for t in out)
        return [t.clone() for t in out] + list(state_bufs(env).values()) + [env._ev_chg.clone(), torch.tensor(d)]

    def replay(env, aa):
        return [[t.clone() for t in step(env, a)] for a in aa]

    env = make()
    env.reset()
    for a in acts[:283]:
        step(env, a)
    sd = env.state_dict()
    ref = replay(env, acts[283:])                # crosses the episode's end (step 288)
    env.load_state_dict(sd)
    again = replay(env, acts[283:])
    fresh = make()
    fresh.reset()
    fresh.load_state_dict(sd)
    other = replay(fresh, acts[283:])
    for t, (x, y, z) in enumerate(zip(ref, again, other)):
        for i, (u, v, w) in enumerate(zip(x, y, z)):
            # (bit patterns: the carried pv_power may be NaN)
            bits = lambda q: q.view(torch.int32) if q.dtype == F32 else q
            assert torch.equal(bits(u), bits(v)), "rewound house, step %d output %d" % (t, i)
            assert torch.equal(bits(u), bits(w)), "fresh house, step %d output %d" % (t, i)
    # packed actions are read in place: a restore must leave the caller's tensors alone
    rng = np.random.default_rng(4)
    for a in acts:
        assert torch.equal(a, torch.tensor(rng.uniform(-1.1, 1.1, a.shape).astype(np.float32), device=DEV))
    e64 = make(F64)
    e64.reset()
    with pytest.raises(ValueError, match="expected .* torch.float32"):
        env.load_state_dict(e64.state_dict())


def test_hs_f32_c_abi_checks_and_dtype_mismatch():
    from powergridworld_amd import _lib
    cfg, names = config("hs_scenario")
    n = 8
    env = house(cfg, n, F32)
    env.reset()
    lib, info, st = _lib.lib(), env._info_at(0), env._stream()
    act = torch.zeros((n, len(names)), dtype=F32, device=DEV)
    b = _lib.HSBuffersF32.from_buffer_copy(env._bufs)
    b.action = _lib.Matf(None, 0, 0)
    assert lib.pgw_hs_step_f32(env.params, info, n, b, st) != 0
    assert b"null" in lib.pgw_last_error()
    b.action = _lib.matf(act)
    assert lib.pgw_hs_reset_f32(env.params, info, n, None, b, st) != 0
    assert b"init_soc" in lib.pgw_last_error()
    b.obs = _lib.Matf(None, 0, 0)
    assert lib.pgw_hs_step_f32(env.params, info, n, b, st) != 0 and b"null" in lib.pgw_last_error()
    # n == 0: nothing launched, PGW_OK
    b = _lib.HSBuffersF32.from_buffer_copy(env._bufs)
    b.action = _lib.matf(act)
    assert lib.pgw_hs_step_f32(env.params, info, 0, b, st) == 0
    assert lib.pgw_hs_reset_f32(env.params, info, 0, C.c_void_p(env._init_soc.data_ptr()), b, st) == 0
    before = [t.clone() for t in list(out_bufs(env).values()) + list(state_bufs(env).values())]
    torch.cuda.synchronize()
    for x, y in zip(before, list(out_bufs(env).values()) + list(state_bufs(env).values())):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # a component of another dtype than the house
    for house_dt, comp_dt in ((F32, F64), (None, F32)):
        bad = copy.deepcopy(cfg)
        bad["components"][1]["config"]["dtype"] = comp_dt
        with pytest.raises(NotImplementedError, match="component"):
            house(bad, n, house_dt)
