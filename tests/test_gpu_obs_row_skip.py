"""pgw_coord_step_rows: the one-launch C4 step told which env-uniform
observation rows (slots 10, 11, 12, 14, 15) the buffer already holds, and
MultiAgentEnv's bookkeeping of what its buffer holds.  Needs an MI355X.

Everything is demanded bit for bit (torch.equal): a row left in place must be
what pgw_coord_step would have stored, and nothing else may change.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = (10, 11, 12, 14, 15)
ALL = sum(1 << j for j in ROWS)
OBS = 17
GUARD = 64
PAD = 3                  # columns between an observation row's n envs and the next row
SENT = -12345.5          # finite; no observation, state or reward takes this value
PGW_ERR_ARG = -1


def _c4_env(n, na=5, comfort_bounds=None, **kw):
    from powergridworld_amd.scenarios.coordinated import CoordinatedMultiBuildingControlEnv, make_c4_config
    cfg = make_c4_config(num_buildings=na)
    if comfort_bounds is not None:      # (one component list shared by every agent)
        cfg["agents"][0]["config"]["components"][0]["config"]["comfort_bounds"] = comfort_bounds
    env = CoordinatedMultiBuildingControlEnv(**cfg, num_envs=n, device=DEV, fused=True, **kw)
    F = env._fused
    assert F is not None and F["kernel"] == "pgw_coord_step" and F["rows"] and F.get("od_on")
    for ai, agent in enumerate(env.agents):
        agent.env_dict["storage"].seed(100 + ai)
    return env


# ------------------------------------------------------------------ 1. the C ABI directly
class _Guarded:
    """A sentinel-filled device buffer of `size` elements with GUARD sentinel
    elements on either side."""

    def __init__(self, size, dtype=torch.float64, init=None):
        self.size = size
        self.sent = -77 if dtype == torch.int32 else SENT
        self.t = torch.full((size + 2 * GUARD,), self.sent, dtype=dtype, device=DEV)
        if init is not None:
            self.inner.copy_(init.reshape(-1))
        self.ptr = self.t.data_ptr() + GUARD * self.t.element_size()

    @property
    def inner(self):
        return self.t[GUARD:GUARD + self.size]

    def guards_intact(self):
        return bool((self.t[:GUARD] == self.sent).all() and (self.t[GUARD + self.size:] == self.sent).all())


class _Direct:
    """One post-reset state of an n-env, na-agent C4 env, and launch buffers of
    its own for every copy of it: each buffer guarded, the observation rows
    n + PAD apart and filled with the sentinel."""

    def __init__(self, n, na):
        from powergridworld_amd import _lib
        self.n, self.na = n, na
        env = self.env = _c4_env(n, na)
        env.reset()
        F = env._fused
        g = torch.Generator(device=DEV).manual_seed(7 * n + na)
        self.act = torch.rand((na, 8, n), dtype=torch.float64, device=DEV, generator=g) * 2.0 - 1.0
        self.x0, self.soc0 = F["x"].clone(), F["soc"].clone()
        bld, pv = F["bld0"], F["pv0"]
        self.info, self.pfp, self.pft, _ = env._step_entry(
            (bld.time_index, pv.index, env._time_at(1), env.pf_solver.tables_version))
        self.st = _lib.stream_ptr(env.device)
        self.lib = _lib.lib()
        self.ref = self.copy()
        assert self.lib.pgw_coord_step(F["params"], self.pfp, self.pft, self.info, n, self.ref["b"], self.st) == 0
        torch.cuda.synchronize()

    def copy(self):
        from powergridworld_amd import _lib
        n, na, F = self.n, self.na, self.env._fused
        g = dict(obs=_Guarded(na * OBS * (n + PAD)), x=_Guarded(na * 5 * n, init=self.x0),
                 soc=_Guarded(na * n, init=self.soc0), reward=_Guarded(na * n), agent_power=_Guarded(na * n),
                 v_out=_Guarded(n), vv=_Guarded(n), iters=_Guarded(n, torch.int32),
                 od_list=_Guarded(n, torch.int32), od_count=_Guarded(2, torch.int32))
        g["od_count"].inner.zero_()
        b = _lib.CoordBuffers.from_buffer_copy(F["bufs"])
        b.action = _lib.Mat(self.act.data_ptr(), 1, self.act.stride(1))
        b.act_stride_agent = self.act.stride(0)
        b.obs = _lib.Mat(g["obs"].ptr, 1, n + PAD)
        b.obs_stride_agent = OBS * (n + PAD)
        for k in ("x", "soc", "reward", "agent_power", "v_out", "vv", "iters", "od_list", "od_count"):
            setattr(b, k, g[k].ptr)
        b.od_parity = 1
        return dict(b=b, g=g)

    def obs(self, c):
        return c["g"]["obs"].inner.view(self.na, OBS, self.n + PAD)


_direct_cache = {}


@pytest.fixture(params=[(193, 5), (65, 1), (65, 8)], ids=lambda s: "n%d_a%d" % s)
def direct(request):
    """(three full blocks and a one-env block; one agent; PGW_MAX_AGENTS agents)"""
    if request.param not in _direct_cache:
        _direct_cache[request.param] = _Direct(*request.param)
    return _direct_cache[request.param]


def test_reference_copy_stores_every_row(direct):
    """pgw_coord_step itself: every row's n envs written, nothing past n."""
    o = direct.obs(direct.ref)
    assert not bool((o[:, :, :direct.n] == SENT).any())
    assert bool((o[:, :, direct.n:] == SENT).all())
    assert all(x.guards_intact() for x in direct.ref["g"].values())


@pytest.mark.parametrize("mask", [1 << j for j in ROWS] + [ALL], ids=lambda m: "mask_%#x" % m)
def test_held_rows_are_left_and_nothing_else_changes(direct, mask):
    d, n = direct, direct.n
    B = d.copy()
    rc = d.lib.pgw_coord_step_rows(d.env._fused["params"], d.pfp, d.pft, d.info, n, B["b"], d.st, mask)
    assert rc == 0
    torch.cuda.synchronize()
    oa, ob = d.obs(d.ref), d.obs(B)
    for j in range(OBS):
        if mask >> j & 1:       # every element of a held row of every agent: still the sentinel
            assert bool((ob[:, j] == SENT).all()), j
        else:
            assert torch.equal(oa[:, j], ob[:, j]), j
            assert not bool((ob[:, j, :n] == SENT).any()), j
    assert bool((ob[:, :, n:] == SENT).all())           # nothing past n in any row
    for k, x in B["g"].items():
        assert x.guards_intact(), k
        if k not in ("obs", "od_list"):
            assert torch.equal(x.inner, d.ref["g"][k].inner), k
    cnt = int(B["g"]["od_count"].inner[1])
    assert torch.equal(B["g"]["od_list"].inner[:cnt].sort().values, d.ref["g"]["od_list"].inner[:cnt].sort().values)


@pytest.mark.parametrize("mask", [1 << 0, 1 << 13, 1 << 16, ALL | 1 << 13], ids=lambda m: "mask_%#x" % m)
def test_other_bits_are_refused_before_any_launch(direct, mask):
    d = direct
    B = d.copy()
    before = {k: x.t.clone() for k, x in B["g"].items()}
    rc = d.lib.pgw_coord_step_rows(d.env._fused["params"], d.pfp, d.pft, d.info, d.n, B["b"], d.st, mask)
    torch.cuda.synchronize()
    assert rc == PGW_ERR_ARG
    for k, x in B["g"].items():
        assert torch.equal(x.t, before[k]), k


def test_held_rows_need_the_standard_layout(direct):
    """Another agent layout: a held row is refused before any launch."""
    from powergridworld_amd import _lib
    d = direct
    p = _lib.CoordParams.from_buffer_copy(d.env._fused["params"])
    p.bld.obs_var[3] = 5                                # not the default building observations
    B = d.copy()
    before = {k: x.t.clone() for k, x in B["g"].items()}
    rc = d.lib.pgw_coord_step_rows(p, d.pfp, d.pft, d.info, d.n, B["b"], d.st, 1 << 10)
    torch.cuda.synchronize()
    assert rc == PGW_ERR_ARG
    for k, x in B["g"].items():
        assert torch.equal(x.t, before[k]), k


# ------------------------------------------------------------------ 2. env against env
def _bits(x):
    return np.asarray([x], dtype=np.float64).view(np.int64)[0]


def _host_key(env):
    """The five source scalars of the step about to run, from the components'
    exogenous arrays (not from the env's step cache)."""
    F = env._fused
    bld, pv = F["bld0"], F["pv0"]
    t = bld.time_index + 1
    return tuple(_bits(v) for v in (bld._cb[t, 0], bld._cb[t, 1], bld._T_oa[t], 1. * t / bld.max_episode_steps,
                                    float(pv.data[pv.index])))


def _outputs(env, rew, meta):
    F = env._fused
    return [env.packed_obs(), torch.stack([rew[a.name] for a in env.agents]), F["x"], F["soc"], F["agent_power"],
            F["v_out"], meta["voltage_violation"], env.pf_solver.iterations]


def _bounds():
    """Comfort bounds per exogenous row: the default, another pair where the
    steps 5 .. 8 read it (ex_next of step k is row k), the default again from step 9."""
    from powergridworld_amd.agents.buildings import DEFAULT_COMFORT_BOUNDS
    cb = np.tile(np.asarray(DEFAULT_COMFORT_BOUNDS, dtype=np.float64), (1024, 1))
    cb[5:9] += np.array([-0.5, 0.75])
    return cb




def test_env_with_row_skip_equals_env_without():
    """Two 130-env C4 envs with the same seeds and actions, one with
    obs_row_skip=False: one whole episode (night -> day -> night), its reset
    and 20 more steps, every output equal after every step, and the rows
    skipped equal to the count the exogenous arrays give."""
    n = 130
    on, off = _c4_env(n, comfort_bounds=_bounds()), _c4_env(n, comfort_bounds=_bounds(), obs_row_skip=False)
    assert on.obs_row_skip and not off.obs_row_skip
    g = torch.Generator(device=DEV).manual_seed(11)
    acts = torch.rand((306, 5, n, 8), dtype=torch.float64, device=DEV, generator=g) * 2.0 - 1.0
    state = dict(expect=0, held=None, k=0, lb=set())

    def start():
        for env in (on, off):
            env.reset()
        state["held"] = None
        assert torch.equal(on.packed_obs(), off.packed_obs())

    def step():
        key = _host_key(on)
        state["lb"].add(key[0])
        if state["held"] is not None:
            state["expect"] += sum(int(a == b) for a, b in zip(state["held"], key))
        state["held"] = key
        a = acts[state["k"]]
        state["k"] += 1
        _, r1, d1, m1 = on.step(a)
        _, r0, d0, m0 = off.step(a)
        for i, (u, v) in enumerate(zip(_outputs(on, r1, m1), _outputs(off, r0, m0))):
            assert torch.equal(u, v), "step %d output %d" % (state["k"], i)
        assert d1 == d0
        assert on.obs_rows_skipped == state["expect"], state["k"]
        return d1["__all__"]

    start()
    while not step():
        assert state["k"] < 286
    assert state["k"] == 286
    start()
    for _ in range(20):
        assert not step()
    assert len(state["lb"]) == 2                  # the bounds did change, and back
    assert off.obs_rows_skipped == 0
    # slots 10 and 11 repeat on every step but each episode's first, the change
    # and the change back; the other rows add to that (the PV row at night)
    assert on.obs_rows_skipped == state["expect"] >= 2 * (306 - 2 - 2)


# ------------------------------------------------------------------ 3. invalidation
def _poison(env):
    env._fused["obs"][:, list(ROWS)] = SENT


def _clean(env):
    return not bool((env._fused["obs"] == SENT).any())


def test_next_step_stores_all_rows_after_reset_restore_and_graph():
    """Poison the five rows, take one step: no sentinel may survive right after
    reset(), right after load_state_dict() to an earlier step and right after
    a captured two-step graph call; and the run equals, bit for bit, a twin's
    that was never interrupted."""
    n = 130
    env, twin = _c4_env(n), _c4_env(n)
    g = torch.Generator(device=DEV).manual_seed(5)
    acts = torch.rand((16, 5, n, 8), dtype=torch.float64, device=DEV, generator=g) * 2.0 - 1.0

    def run(e, lo, hi):
        out = []
        for t in range(lo, hi):
            _, rew, _, meta = e.step(acts[t])
            out.append([x.clone() for x in _outputs(e, rew, meta)])
        return out

    def same(x, y, tag):
        for t, (p, q) in enumerate(zip(x, y)):
            for i, (u, v) in enumerate(zip(p, q)):
                assert torch.equal(u, v), "%s, step %d output %d" % (tag, t, i)

    for e in (env, twin):
        e.reset()
    # (the test can see a skip: a row the env holds does survive a poisoning)
    run(env, 0, 2), run(twin, 0, 2)
    _poison(env)
    skipped = env.obs_rows_skipped
    run(env, 2, 3), run(twin, 2, 3)
    assert env.obs_rows_skipped > skipped and not _clean(env)
    # 1. right after reset()
    for e in (env, twin):
        e.reset()
    _poison(env)
    first = run(env, 0, 1)
    assert _clean(env)
    same(first + run(env, 1, 4), run(twin, 0, 4), "after reset")
    # 2. right after a load_state_dict() to an earlier step
    sd = env.state_dict()
    uninterrupted = run(twin, 4, 8)
    same(run(env, 4, 8), uninterrupted, "before the restore")
    env.load_state_dict(sd)
    _poison(env)
    again = run(env, 4, 5)
    assert _clean(env)
    same(again + run(env, 5, 8), uninterrupted, "restored run")
    # 3. right after a capture_step(steps=2) graph call
    graph = env.capture_step([acts[8], acts[9]], steps=2)
    graph()
    run(twin, 8, 10)
    _poison(env)
    after = run(env, 10, 11)
    assert _clean(env)
    same(after, run(twin, 10, 11), "after the graph call")
    graph.release()
