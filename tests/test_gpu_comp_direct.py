"""The battery, PV, building and reduce kernels (csrc/pgw_components.hip, the
device functions of csrc/pgw_common.h) called through the C ABI and compared
BIT FOR BIT with the restated references of tests/_comp_direct_common.py:
every env at every step, each step from the reference's own pre-step state,
fp64 and fp32 storage, at the sizes where one-thread-per-env indexing and the
`e >= n` guard can go wrong, in three pgw_mat layouts, with every output
buffer inside a sentinel-filled allocation that must stay intact around the
n x dim window.

    battery    pgw_battery_reset / _step (+ _f32)
    pv         pgw_pv_obs / _step (+ _f32)
    building   pgw_building_reset / _step (+ _f32): the standard layout
               (bld_std_step), standard == generic with a 16th slot, the
               generic path (n_obs 0 / 1 / 24, synthetic sel / nbr, ext arrays)
    wave       pgw_mc_agent_step (+ _f32) through MultiComponentEnv: the fused
               agent wave (bld_stage_wave) against the references
    reduce     pgw_agent_reduce
    args       every refusal of the entries: PGW_ERR_ARG, nothing launched

Each test prints `comp-direct <entry> <cases> <envs x steps compared>`.
Needs an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _comp_direct_common as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TD = {"f64": torch.float64, "f32": torch.float32}
STORAGES = ["f64", "f32"]
LAYOUTS = ("major", "minor", "window")
PAD = 32                                    # guard envs before and after (n + 64 allocated)
# no result can equal these: the outputs are NaN, infinite or far smaller
SENT = {"f64": -1.2345678901234567e300, "f32": -1.2345678e30}


def _lib():
    from powergridworld_amd import _lib
    return _lib


def _fn(name, storage):
    return getattr(_lib().lib(), name + ("_f32" if storage == "f32" else ""))


def _stream():
    return _lib().stream_ptr(torch.device(DEV))


def _record(entry, cases, compared):
    print("comp-direct %s %d %d" % (entry, cases, compared))
    assert compared > 0


class G:
    """Window elements `idx` (any shape) of a sentinel-filled device buffer."""

    def __init__(self, idx, size, storage, values=None, s_env=0, s_dim=0):
        self.idx, self.size, self.storage = np.asarray(idx, dtype=np.int64), size, storage
        self.s_env, self.s_dim = s_env, s_dim
        self.off = int(self.idx.ravel()[0]) if self.idx.size else PAD
        self.t = torch.empty(size, dtype=TD[storage], device=DEV)
        self.set(values)

    def set(self, values=None):
        host = np.full(self.size, SENT[self.storage], dtype=K.ND[self.storage])
        if values is not None:
            host[self.idx] = np.asarray(values, dtype=K.ND[self.storage])
        self.t.copy_(torch.from_numpy(host))
        return self

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + self.off * self.t.element_size())

    def mat(self):
        L = _lib()
        return (L.Matf if self.storage == "f32" else L.Mat)(self.ptr.value, self.s_env, self.s_dim)

    def check(self, ref, what):
        """The guards still hold the sentinel; the window holds ref's bits (ref
        None: the window too is untouched)."""
        host = self.t.cpu().numpy()
        u = K.UINT[self.storage]
        outside = np.ones(self.size, dtype=bool)
        if ref is not None:
            outside[self.idx.ravel()] = False
        sent = np.array([SENT[self.storage]], dtype=K.ND[self.storage]).view(u)[0]
        bad = np.flatnonzero(host.view(u)[outside] != sent)
        assert bad.size == 0, "%s: %d elements outside the window were written" % (what, bad.size)
        if ref is not None:
            K.same_bits(host[self.idx], np.asarray(ref, dtype=K.ND[self.storage]).reshape(self.idx.shape), what)


def vec(n, storage, values=None):
    return G(PAD + np.arange(n), n + 2 * PAD, storage, values)


def state_x(n, storage, values=None):
    """x: 5 x n zone-major with its true n, guards before and after."""
    return G(PAD + np.arange(5 * n).reshape(5, n), 5 * n + 2 * PAD, storage, values)


def matrix(n, dim, layout, storage, values=None):
    """An [n, dim] pgw_mat window: env-major contiguous, env-minor, or a column
    window of a wider env-major matrix; n + 64 envs allocated, guard columns."""
    N = n + 2 * PAD
    if layout == "major":
        s_env, s_dim, off, size = dim, 1, PAD * dim, N * dim
    elif layout == "minor":
        s_env, s_dim, off, size = 1, N, N + PAD, (dim + 2) * N
    else:
        D = dim + 3
        s_env, s_dim, off, size = D, 1, PAD * D + 2, N * D
    idx = off + np.arange(n)[:, None] * s_env + np.arange(dim)[None, :] * s_dim
    g = G(idx, max(size, 2 * PAD), storage, values, s_env, s_dim)
    g.off = off if size else PAD
    return g


def f64_dev(a):
    """A float64 input array on the device (PAD spare elements behind it)."""
    if a is None:
        return None
    return torch.tensor(np.concatenate([np.asarray(a, dtype=np.float64), np.zeros(PAD)]), dtype=torch.float64,
                        device=DEV)


def counter():
    return torch.zeros(1, dtype=torch.int64, device=DEV)


def ok(rc):
    _lib().check(rc)


# ---------------------------------------------------------------- battery
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("c", K.BATTERY_CASES, ids=[c.id for c in K.BATTERY_CASES])
def test_battery(c, storage):
    reset, step = _fn("pgw_battery_reset", storage), _fn("pgw_battery_step", storage)
    compared = 0
    for n in K.SIZES:
        for sampled in (0, 1):
            ep = K.battery_episode(c.id, n, storage, sampled)
            for li, layout in enumerate(LAYOUTS):
                cnt = counter() if li == 0 else None      # oob = NULL changes nothing else
                want = 0
                for t, (B, pre, act, r) in enumerate(ep):
                    tag = (c.id, storage, n, sampled, layout, t)
                    p = K.battery_params(B, cnt.data_ptr() if cnt is not None else None)
                    obs = matrix(n, 1, layout, storage)
                    if act is None:
                        init, soc = vec(n, storage, pre), vec(n, storage)
                        ok(reset(p, n, init.ptr, soc.ptr, obs.mat(), _stream()))
                        init.check(pre, ("init", tag))
                    else:
                        a, soc, rp = matrix(n, 1, layout, storage, act[:, None]), vec(n, storage, pre), vec(n, storage)
                        ok(step(p, n, a.mat(), soc.ptr, obs.mat(), rp.ptr, _stream()))
                        a.check(act[:, None], ("action", tag))
                        rp.check(r.rp, ("real power", tag))
                        want += r.oob
                    soc.check(r.soc, ("soc", tag))
                    obs.check(r.obs, ("obs", tag))
                    compared += n
                if cnt is not None:
                    assert int(cnt) == want, (c.id, n, sampled)
    _record("battery %s %s" % (storage, c.id), len(K.SIZES) * 2 * len(LAYOUTS), compared)


# ---------------------------------------------------------------- PV
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("c", K.PV_CASES, ids=[c.id for c in K.PV_CASES])
def test_pv(c, storage):
    obs_fn, step = _fn("pgw_pv_obs", storage), _fn("pgw_pv_step", storage)
    P = K.PV(-K.PV_MAX, c.rescale, c.grid_aware)
    dim, compared = 1 + c.grid_aware, 0
    for n in K.SIZES:
        act, vmin = K.pv_inputs(c, n, storage)
        vmin_d = f64_dev(vmin) if c.grid_aware else None
        for li, layout in enumerate(LAYOUTS):
            cnt = counter() if li == 0 else None
            want = 0
            p = K.pv_params(P, cnt.data_ptr() if cnt is not None else None)
            for t, pmax in enumerate(K.PV_PMAX):
                tag = (c.id, storage, n, layout, pmax)
                r = K.pv_ref(P, n, pmax, act[t], vmin, storage)
                a, obs, rp = matrix(n, 1, layout, storage, act[t][:, None]), matrix(n, dim, layout, storage), \
                    vec(n, storage)
                ok(step(p, n, pmax, a.mat(), _lib().dptr(vmin_d), obs.mat(), rp.ptr, _stream()))
                obs.check(r.obs, ("obs", tag))
                rp.check(r.rp, ("real power", tag))
                a.check(act[t][:, None], ("action", tag))
                want += r.oob
                # the obs entry (no action, no real power): the same observation, no count
                obs2 = matrix(n, dim, layout, storage)
                ok(obs_fn(p, n, pmax, _lib().dptr(vmin_d), obs2.mat(), _stream()))
                obs2.check(K.pv_ref(P, n, pmax, None, vmin, storage).obs, ("obs entry", tag))
                compared += 2 * n
            if cnt is not None:
                assert int(cnt) == want, (c.id, n)
    _record("pv %s %s" % (storage, c.id), len(K.SIZES) * len(LAYOUTS) * len(K.PV_PMAX), compared)


# ---------------------------------------------------------------- building
def _ext_dev(ext):
    keep = {k: f64_dev(v) for k, v in ext.items()}
    return K.building_ext({k: v.data_ptr() for k, v in keep.items()}), keep


def _building_launch(M, rec, n, storage, layout, lagged, ext, oob=None, no_rout=False, no_rstate=False,
                     n_obs=None):
    """One record's launch from its pre-state; returns the output buffers."""
    dim = len(M.obs_var)
    p = K.building_params(M, oob, n_obs)
    ext_s, keep = _ext_dev(ext)
    x, pc, obs = state_x(n, storage, rec.x), vec(n, storage), matrix(n, dim, layout, storage)
    rstate = None if no_rstate else vec(n, storage, rec.rstate)
    out = K.NS(x=x, pc=pc, obs=obs, rstate=rstate, rout=None, act=None)
    if rec.kind == "reset":
        ok(_fn("pgw_building_reset", storage)(p, K.building_exo(rec.ex), n, x.ptr, pc.ptr,
                                              rstate.ptr if rstate else None, ext_s, obs.mat(), _stream()))
    else:
        out.act = matrix(n, 6, layout, storage, rec.action)
        out.rout = None if no_rout else vec(n, storage)
        ok(_fn("pgw_building_step", storage)(p, K.building_exo(rec.ex), K.building_exo(rec.exn), n, out.act.mat(),
                                             x.ptr, pc.ptr, out.rout.ptr if out.rout else None,
                                             rstate.ptr if rstate else None, lagged, ext_s, obs.mat(), _stream()))
    torch.cuda.synchronize()
    del keep
    return out


def _building_check(out, rec, tag):
    r = rec.ref
    out.x.check(r.x, ("x", tag))
    out.pc.check(r.pc, ("p_consumed", tag))
    out.obs.check(r.obs if r.obs.shape[1] else None, ("obs", tag))
    if out.rstate is not None:
        out.rstate.check(r.rstate, ("reward_state", tag))
    if out.rout is not None:
        out.rout.check(r.rout, ("reward_out", tag))
    if out.act is not None:
        out.act.check(rec.action, ("action", tag))


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("c", K.BLD_CASES, ids=[c.id for c in K.BLD_CASES])
def test_building(c, storage):
    """Two consecutive resets (x_k persists) and the steps of a case.  lagged = 0
    cases pass reward_out = NULL in the env-minor layout and reward_state =
    NULL in the window layout; the counter is bound in the first layout only."""
    compared = 0
    for n in K.BLD_SIZES:
        M, rows, ext, recs = K.building_episode(c.id, n, storage)
        assert K.bld_is_std_ref(M) == (c.kind == "std")
        for li, layout in enumerate(LAYOUTS):
            cnt = counter() if li == 0 else None
            want = 0
            for t, rec in enumerate(recs):
                tag = (c.id, storage, n, layout, t, rec.kind)
                out = _building_launch(M, rec, n, storage, layout, c.lagged, ext,
                                       cnt.data_ptr() if cnt is not None else None,
                                       no_rout=(not c.lagged and li == 1), no_rstate=(not c.lagged and li == 2))
                _building_check(out, rec, tag)
                want += getattr(rec.ref, "oob", 0)
                compared += n
            if cnt is not None:
                assert int(cnt) == want, (c.id, n)
    _record("building %s %s" % (storage, c.id), len(K.BLD_SIZES) * len(LAYOUTS), compared)


def _plus_bus_slot(M):
    P = K.Building(M.A, M.B, M.K, M.C, M.mean, M.sel, M.nbr, M.obs_var + [K.BV_BUS_VOLTAGE],
                   np.append(M.obs_low, 0.9), np.append(M.obs_high, 1.1), M.rescale, M.T_init)
    assert K.bld_is_std_ref(M) and not K.bld_is_std_ref(P)
    return P


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("degenerate", [False, True], ids=["shipped-bounds", "low-equals-high"])
@pytest.mark.parametrize("rescale", [1, 0])
def test_building_standard_equals_generic(rescale, degenerate, storage):
    """bld_std_step == the generic functions, op for op: the same model with a
    16th slot (bus voltage) takes the generic kernel, and its first 15 columns,
    x, p_consumed, both rewards and the count equal the standard kernel's.
    Both are given the same ext arrays; the standard kernel ignores them and
    nothing compared depends on them.  low-equals-high: obs_low == obs_high on
    two slots; the generic to_scaled divides 0 by 0 there, and exact_div of a
    zero numerator by a zero range with an infinite reciprocal is 0 * inf: a
    NaN on both paths (and in the reference)."""
    compared = 0
    cid = "std-r%d-l0" % rescale
    for n in K.BLD_SIZES:
        M, rows, _, recs = K.building_episode(cid, n, storage)
        if degenerate:
            M = K.Building(M.A, M.B, M.K, M.C, M.mean, M.sel, M.nbr, M.obs_var, M.obs_low, M.obs_high, M.rescale,
                           M.T_init)
            M.obs_low[3], M.obs_low[13] = M.obs_high[3], M.obs_high[13]
        M16 = _plus_bus_slot(M)
        ext = {"bus": K.building_inputs(M, 77, n, 1)[2]["bus"]}
        for rec in recs[2:]:
            ref = K.building_step_ref(M, rec.ex, rec.exn, rec.x, rec.action, rec.rstate, 0, None, storage)
            if degenerate and rescale:
                assert np.isnan(ref.obs[:, [3, 13]]).all()
            c_std, c_gen = counter(), counter()
            std = _building_launch(M, rec, n, storage, "major", 0, ext, c_std.data_ptr())
            gen = _building_launch(M16, rec, n, storage, "window", 0, ext, c_gen.data_ptr())
            tag = (cid, degenerate, storage, n)
            for name in ("x", "pc", "rstate", "rout"):
                a, b = getattr(std, name), getattr(gen, name)
                K.same_bits(a.t.cpu().numpy()[a.idx], b.t.cpu().numpy()[b.idx], (name, tag))
                a.check(getattr(ref, name), (name, "standard", tag))
            o_std, o_gen = std.obs.t.cpu().numpy()[std.obs.idx], gen.obs.t.cpu().numpy()[gen.obs.idx]
            K.same_bits(o_std, o_gen[:, :15], ("obs", tag))
            std.obs.check(ref.obs, ("obs", "standard", tag))
            ref16 = K.building_step_ref(M16, rec.ex, rec.exn, rec.x, rec.action, rec.rstate, 0, ext, storage)
            gen.obs.check(ref16.obs, ("obs", "generic", tag))
            assert int(c_std) == int(c_gen) == ref.oob
            compared += n
    _record("building std==generic %s r%d %s" % (storage, rescale, degenerate), len(K.BLD_SIZES), compared)


# ---------------------------------------------------------------- the fused agent wave
def _same_struct(a, b, skip=("oob",)):
    for name, _ in a._fields_:
        if name in skip:
            continue
        va, vb = getattr(a, name), getattr(b, name)
        if hasattr(va, "_length_"):
            va, vb = np.ctypeslib.as_array(va).tolist(), np.ctypeslib.as_array(vb).tolist()
        assert va == vb, name


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("with_pv_storage", [False, True], ids=["building", "building-pv-storage"])
@pytest.mark.parametrize("n", K.WAVE_SIZES)
def test_fused_agent_wave(n, with_pv_storage, storage):
    """pgw_mc_agent_step(_f32) through MultiComponentEnv on the shipped model:
    bld_stage_wave (every lane of the building wave copies parameters, e < n or
    not; the last block is partial) against building_step_ref with lagged = 0,
    the PV and battery waves against theirs, and the agent's sums."""
    from powergridworld_amd import MultiComponentEnv
    from powergridworld_amd.agents import EnergyStorageEnv, FiveZoneROMThermalEnergyEnv, PVEnv
    comps = [{"name": "building", "cls": FiveZoneROMThermalEnergyEnv, "config": {}}]
    if with_pv_storage:
        comps += [{"name": "pv", "cls": PVEnv, "config": {"profile_csv": "pv_profile.csv", "scaling_factor": 40.}},
                  {"name": "storage", "cls": EnergyStorageEnv, "config": {}}]
    env = MultiComponentEnv(name="mc", components=comps, num_envs=n, device=DEV, dtype=TD[storage])
    assert env._mc_fusable()
    env.reset(init_storage=np.full(n, 30.0))
    bld = env.env_dict["building"]
    steps, nd, td = 6, K.ND[storage], TD[storage]
    M = K.shipped_building(rescale=1)
    _same_struct(bld.params, K.building_params(M))
    x, act_b, _ = K.building_inputs(M, 40 + n, n, steps, storage)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=td, device=DEV)
    host = lambda t: t.contiguous().cpu().numpy()
    if with_pv_storage:
        pv, bat = env.env_dict["pv"], env.env_dict["storage"]
        pv.index = 130                                   # midday rows of the profile
        P, B = K.PV(-float(np.max(pv.data)), 1, 0), K.Battery()
        _same_struct(pv.params, K.pv_params(P))
        _same_struct(bat.params, K.battery_params(B))
        cb = next(c for c in K.BATTERY_CASES if c.id == "default-r1")
        soc, act_s = K.battery_inputs(K.NS(cfg=cb.cfg, seed=n, steps=steps), n, storage)
        soc = K.battery_reset_ref(B, soc, storage).soc
        act_p = K.pv_inputs(K.NS(seed=n), max(n, 2), storage)[0]
        act_p = np.resize(act_p, (steps, n))
    want_oob = 0
    for t in range(steps):
        tag = (n, with_pv_storage, storage, t)
        ex, exn = K.exo_of_struct(bld._exo[t]), K.exo_of_struct(bld._exo[t + 1])
        r = K.building_step_ref(M, ex, exn, x, act_b[t], None, 0, None, storage)
        bld.x.copy_(dev(x))
        action = {"building": dev(act_b[t])}
        want_oob += r.oob
        total_rp, total_rew = 0.0 + r.pc.astype(np.float64), 0.0 + r.rstate.astype(np.float64)
        if with_pv_storage:
            pmax = float(pv.data[pv.index])
            assert pmax > 0.0
            rp_ = K.pv_ref(P, n, pmax, act_p[t], None, storage)
            rb = K.battery_step_ref(B, soc, act_s[t], storage)
            bat.soc.copy_(dev(soc))
            action["pv"], action["storage"] = dev(act_p[t][:, None]), dev(act_s[t][:, None])
            want_oob += rp_.oob + rb.oob
            with np.errstate(all="ignore"):
                total_rp = (total_rp + rp_.rp.astype(np.float64)) + rb.rp.astype(np.float64)
                total_rew = (total_rew + 0.0) + 0.0
        env.step(action)
        torch.cuda.synchronize()
        K.same_bits(host(bld._obs), r.obs, ("building obs", tag))
        K.same_bits(host(bld.x), r.x, ("x", tag))
        K.same_bits(host(bld.p_consumed), r.pc, ("p_consumed", tag))
        K.same_bits(host(bld._reward_state), r.rstate, ("fresh reward", tag))
        if with_pv_storage:
            K.same_bits(host(pv._obs), rp_.obs, ("pv obs", tag))
            K.same_bits(host(pv._real_power), rp_.rp, ("pv real power", tag))
            K.same_bits(host(bat._obs), rb.obs, ("battery obs", tag))
            K.same_bits(host(bat.soc), rb.soc, ("soc", tag))
            K.same_bits(host(bat._real_power), rb.rp, ("battery real power", tag))
            soc = rb.soc
        K.same_bits(host(env._real_power), total_rp.astype(nd), ("agent real power", tag))
        K.same_bits(host(env._reward), total_rew.astype(nd), ("agent reward", tag))
        x = r.x
    assert int(env.oob_count) == want_oob
    _record("wave %s %s" % (storage, "building-pv-storage" if with_pv_storage else "building"), 1, n * steps)


# ---------------------------------------------------------------- reduce
@pytest.mark.parametrize("n_comp", [0, 1, K.MAX_COMP])
def test_agent_reduce(n_comp):
    L = _lib()
    fn, compared = L.lib().pgw_agent_reduce, 0
    nulls = [(), (0,), (n_comp // 2,), (n_comp - 1,), (0, n_comp // 2, n_comp - 1)] if n_comp else [()]
    for n in K.SIZES:
        for k, null in enumerate(nulls):
            rp_cols, rw_cols = K.reduce_columns(n, n_comp, k), K.reduce_columns(n, n_comp, 50 + k)
            rp_dev, rw_dev = [f64_dev(c) for c in rp_cols], [f64_dev(c) for c in rw_cols]
            a = L.ReduceArgs()
            a.n_comp = n_comp
            for i in range(n_comp):
                a.real_power[i] = None if i in null else rp_dev[i].data_ptr()
                a.reward[i] = None if (n_comp - 1 - i) in null else rw_dev[i].data_ptr()
            w, r = K.reduce_ref([None if i in null else c for i, c in enumerate(rp_cols)],
                                [None if (n_comp - 1 - i) in null else c for i, c in enumerate(rw_cols)], n)
            for out_rp, out_rw in ((True, True), (False, True), (True, False)):
                g_rp, g_rw = vec(n, "f64"), vec(n, "f64")
                ok(fn(a, n, g_rp.ptr if out_rp else None, g_rw.ptr if out_rw else None, _stream()))
                g_rp.check(w if out_rp else None, ("real power", n_comp, n, null))
                g_rw.check(r if out_rw else None, ("reward", n_comp, n, null))
                compared += n
            if n_comp and not null:
                assert w[0] == 0.0 and not np.signbit(w[0])          # the -0.0-only column sums to +0.0
    _record("reduce n_comp=%d" % n_comp, len(K.SIZES) * len(nulls) * 3, compared)


# ---------------------------------------------------------------- argument checks
def _refused(entry, storage, call, buffers):
    name = entry + ("_f32" if storage == "f32" else "")
    L = _lib()
    rc = call(getattr(L.lib(), name))
    torch.cuda.synchronize()
    assert rc == -1, (name, rc)                                   # PGW_ERR_ARG
    assert L.lib().pgw_last_error().decode().startswith(name + ":"), (name, L.lib().pgw_last_error())
    for b in buffers:
        b.check(None, (name, "refused"))


@pytest.mark.parametrize("storage", STORAGES)
def test_argument_checks(storage):
    L = _lib()
    n, s = 65, _stream()
    nomat = (L.Matf if storage == "f32" else L.Mat)(None, 0, 0)
    cases = 0
    # battery
    B = K.battery_params(K.Battery())
    init, soc, obs, rp, act = vec(n, storage), vec(n, storage), matrix(n, 1, "major", storage), vec(n, storage), \
        matrix(n, 1, "major", storage)
    outs = [soc, obs, rp]
    for call in (lambda f: f(None, n, init.ptr, soc.ptr, obs.mat(), s), lambda f: f(B, n, None, soc.ptr, obs.mat(), s),
                 lambda f: f(B, n, init.ptr, None, obs.mat(), s), lambda f: f(B, n, init.ptr, soc.ptr, nomat, s),
                 lambda f: f(B, -1, init.ptr, soc.ptr, obs.mat(), s)):
        _refused("pgw_battery_reset", storage, call, outs)
        cases += 1
    for call in (lambda f: f(None, n, act.mat(), soc.ptr, obs.mat(), rp.ptr, s),
                 lambda f: f(B, n, nomat, soc.ptr, obs.mat(), rp.ptr, s),
                 lambda f: f(B, n, act.mat(), None, obs.mat(), rp.ptr, s),
                 lambda f: f(B, n, act.mat(), soc.ptr, nomat, rp.ptr, s),
                 lambda f: f(B, n, act.mat(), soc.ptr, obs.mat(), None, s),
                 lambda f: f(B, -1, act.mat(), soc.ptr, obs.mat(), rp.ptr, s)):
        _refused("pgw_battery_step", storage, call, outs)
        cases += 1
    # PV
    P, Pg = K.pv_params(K.PV(-K.PV_MAX)), K.pv_params(K.PV(-K.PV_MAX, 1, 1))
    obs2 = matrix(n, 2, "major", storage)
    vmin = f64_dev(np.ones(n))
    outs = [obs2, rp]
    for call in (lambda f: f(None, n, 1.0, None, obs2.mat(), s), lambda f: f(P, n, 1.0, None, nomat, s),
                 lambda f: f(P, -1, 1.0, None, obs2.mat(), s), lambda f: f(Pg, n, 1.0, None, obs2.mat(), s)):
        _refused("pgw_pv_obs", storage, call, outs)
        cases += 1
    for call in (lambda f: f(None, n, 1.0, act.mat(), None, obs2.mat(), rp.ptr, s),
                 lambda f: f(P, n, 1.0, nomat, None, obs2.mat(), rp.ptr, s),
                 lambda f: f(P, n, 1.0, act.mat(), None, nomat, rp.ptr, s),
                 lambda f: f(P, n, 1.0, act.mat(), None, obs2.mat(), None, s),
                 lambda f: f(P, -1, 1.0, act.mat(), None, obs2.mat(), rp.ptr, s),
                 lambda f: f(Pg, n, 1.0, act.mat(), None, obs2.mat(), rp.ptr, s)):
        _refused("pgw_pv_step", storage, call, outs)
        cases += 1
    # building
    M = K.shipped_building()
    p, ex = K.building_params(M), K.building_exo(K.exo_rows(0, 1)[0])
    x, pc, rout, rstate = state_x(n, storage), vec(n, storage), vec(n, storage), vec(n, storage)
    obs15, act6 = matrix(n, 15, "major", storage), matrix(n, 6, "major", storage)
    ext = K.building_ext({})
    outs = [x, pc, rout, rstate, obs15]
    resets = [lambda f: f(None, ex, n, x.ptr, pc.ptr, rstate.ptr, ext, obs15.mat(), s),
              lambda f: f(p, None, n, x.ptr, pc.ptr, rstate.ptr, ext, obs15.mat(), s),
              lambda f: f(p, ex, n, None, pc.ptr, rstate.ptr, ext, obs15.mat(), s),
              lambda f: f(p, ex, n, x.ptr, None, rstate.ptr, ext, obs15.mat(), s),
              lambda f: f(p, ex, n, x.ptr, pc.ptr, rstate.ptr, ext, nomat, s),
              lambda f: f(p, ex, -1, x.ptr, pc.ptr, rstate.ptr, ext, obs15.mat(), s)]
    steps = [lambda f: f(None, ex, ex, n, act6.mat(), x.ptr, pc.ptr, rout.ptr, rstate.ptr, 1, ext, obs15.mat(), s),
             lambda f: f(p, None, ex, n, act6.mat(), x.ptr, pc.ptr, rout.ptr, rstate.ptr, 1, ext, obs15.mat(), s),
             lambda f: f(p, ex, None, n, act6.mat(), x.ptr, pc.ptr, rout.ptr, rstate.ptr, 1, ext, obs15.mat(), s),
             lambda f: f(p, ex, ex, n, nomat, x.ptr, pc.ptr, rout.ptr, rstate.ptr, 1, ext, obs15.mat(), s),
             lambda f: f(p, ex, ex, n, act6.mat(), None, pc.ptr, rout.ptr, rstate.ptr, 1, ext, obs15.mat(), s),
             lambda f: f(p, ex, ex, n, act6.mat(), x.ptr, None, rout.ptr, rstate.ptr, 1, ext, obs15.mat(), s),
             lambda f: f(p, ex, ex, n, act6.mat(), x.ptr, pc.ptr, rout.ptr, rstate.ptr, 1, ext, nomat, s),
             lambda f: f(p, ex, ex, -1, act6.mat(), x.ptr, pc.ptr, rout.ptr, rstate.ptr, 1, ext, obs15.mat(), s),
             lambda f: f(p, ex, ex, n, act6.mat(), x.ptr, pc.ptr, rout.ptr, None, 1, ext, obs15.mat(), s)]
    for bad in (-1, 25):
        q = K.building_params(M, n_obs=bad)
        resets.append(lambda f, q=q: f(q, ex, n, x.ptr, pc.ptr, rstate.ptr, ext, obs15.mat(), s))
        steps.append(lambda f, q=q: f(q, ex, ex, n, act6.mat(), x.ptr, pc.ptr, rout.ptr, rstate.ptr, 1, ext,
                                      obs15.mat(), s))
    for call in resets:
        _refused("pgw_building_reset", storage, call, outs)
        cases += 1
    for call in steps:
        _refused("pgw_building_step", storage, call, outs)
        cases += 1
    # n = 0: PGW_OK, nothing touched
    assert _fn("pgw_battery_reset", storage)(B, 0, init.ptr, soc.ptr, obs.mat(), s) == 0
    assert _fn("pgw_battery_step", storage)(B, 0, act.mat(), soc.ptr, obs.mat(), rp.ptr, s) == 0
    assert _fn("pgw_pv_obs", storage)(P, 0, 1.0, None, obs2.mat(), s) == 0
    assert _fn("pgw_pv_step", storage)(P, 0, 1.0, act.mat(), None, obs2.mat(), rp.ptr, s) == 0
    assert _fn("pgw_building_reset", storage)(p, ex, 0, x.ptr, pc.ptr, rstate.ptr, ext, obs15.mat(), s) == 0
    assert _fn("pgw_building_step", storage)(p, ex, ex, 0, act6.mat(), x.ptr, pc.ptr, rout.ptr, rstate.ptr, 1, ext,
                                             obs15.mat(), s) == 0
    torch.cuda.synchronize()
    for b in [soc, obs, rp, obs2, x, pc, rout, rstate, obs15, init, act, act6]:
        b.check(None, "n = 0")
    if storage == "f64":
        a = L.ReduceArgs()
        g = vec(n, "f64")
        assert L.lib().pgw_agent_reduce(None, n, g.ptr, g.ptr, s) != 0
        assert L.lib().pgw_agent_reduce(a, 0, g.ptr, g.ptr, s) == 0
        torch.cuda.synchronize()
        g.check(None, "pgw_agent_reduce refused / n = 0")
    _record("args %s" % storage, cases, cases)
