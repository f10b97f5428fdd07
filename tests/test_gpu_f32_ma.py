"""fp32 storage for the fused multi-agent step (pgw_ma_step_f32): the
heterogeneous scenario with every agent buffer fp32, fp64 arithmetic, each
stored value rounded once, the power flow the fp64 one.  Needs an MI355X.

* bit level: the fused step against fp32 twins of its agents stepped through
  their own fp32 entries (pgw_mc_agent_step_f32, pgw_pv_step_f32,
  pgw_ev_step_f32), the sums and bus loads formed in torch, and a standalone
  fp64 power flow on the fused step's bus loads;
* a free-running episode against the fp64 fused step within the north-star
  fp32 bound (tests/test_gpu_f32.py's bounds);
* checkpoint round trip and the history ring.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32


def _het_act(a):
    return {"building": {"building": a[:, :6], "pv": a[:, 6:7], "storage": a[:, 7:8]},
            "pv": a[:, 8:9], "ev-charging": a[:, 9:10]}


def _make(n, dtype=F32, **kw):
    from powergridworld_amd.multiagent_env import MultiAgentEnv
    from powergridworld_amd.scenarios.heterogeneous import make_env_config
    return MultiAgentEnv(**make_env_config(), num_envs=n, device=DEV, dtype=dtype, **kw)


def _actions(n, steps, seed):
    """Seeded uniform actions in [-1.1, 1.1] (some past the box: the kernels clip), fp32."""
    gen = torch.Generator(DEV).manual_seed(seed)
    return [(torch.rand((n, 10), dtype=torch.float64, device=DEV, generator=gen) * 2.2 - 1.1).float()
            for _ in range(steps)]


def _soc0(n, seed):
    gen = torch.Generator(DEV).manual_seed(seed)
    return (torch.rand(n, dtype=torch.float64, device=DEV, generator=gen) * 235.0 + 5.0).float()


def _band(v):
    """ThisPVEnv.step_reward in fp64 (k_band_penalty's operations)."""
    zero = torch.zeros_like(v)
    lo, up = v - 0.95, 1.05 - v
    viol = torch.where(lo < 0, lo, zero) + torch.where(up < 0, up, zero)
    y = 1000.0 * viol
    return -(y * y)


@pytest.mark.parametrize("n,max_steps", [(200, None), (1, 20)])
def test_het_f32_fused_equals_component_entries(n, max_steps):
    """pgw_ma_step_f32 against the fp32 component entries, bit for bit: n = 200
    (three full 64-env blocks + 8 lanes) over a whole episode, n = 1 over 20
    steps.  The twins get the fused env's own previous min_voltage extrema."""
    from powergridworld_amd import _lib
    from powergridworld_amd.base import MultiComponentEnv
    from powergridworld_amd.agents.vehicles import EVChargingEnv
    from powergridworld_amd.distribution_system.opendss import OpenDSSSolver
    from powergridworld_amd.scenarios.heterogeneous import ThisPVEnv, make_env_config
    cfg = make_env_config()
    env = _make(n)
    assert env._ma is not None and env._ma["fn"] is _lib.lib().pgw_ma_step_f32
    by = {a["name"]: a for a in cfg["agents"]}
    cc = cfg["common_config"]
    mc = MultiComponentEnv(name="building", num_envs=n, device=DEV, dtype=F32, **by["building"]["config"], **cc)
    pv = ThisPVEnv(name="pv", num_envs=n, device=DEV, dtype=F32, **by["pv"]["config"], **cc)
    ev = EVChargingEnv(name="ev-charging", num_envs=n, device=DEV, dtype=F32, **by["ev-charging"]["config"], **cc)
    assert pv.grid_aware and pv.dtype == F32 and all(e.dtype == F32 for e in mc.envs)
    pf = OpenDSSSolver(**cfg["pf_config"]["config"], num_envs=n, device=DEV)
    pf.set_controllable_loads(["675c"])

    soc0 = _soc0(n, 21)
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
    fb, fp, fs = (A["building"].env_dict[c] for c in ("building", "pv", "storage"))
    tb, tp, ts = (mc.env_dict[c] for c in ("building", "pv", "storage"))
    o = env.get_obs()
    for c in ("building", "pv", "storage"):
        assert o["building"][c].dtype == F32 and torch.equal(o["building"][c], mc.env_dict[c]._obs), c
    assert torch.equal(o["pv"], pv._obs) and torch.equal(o["ev-charging"], ev._obs)

    acts = _actions(n, 300, 22)
    steps = 0
    while True:
        a = acts[steps]
        obs, rew, done, _ = env.step(_het_act(a))
        o_mc, r_mc, d_mc, _ = mc.step(_het_act(a)["building"])
        o_pv, r_pv, d_pv, _ = pv.step(a[:, 8:9], min_voltage=v_prev)
        o_ev, r_ev, d_ev, _ = ev.step(a[:, 9:10])
        # every component: obs, state, real power, reward
        for c in ("building", "pv", "storage"):
            assert torch.equal(obs["building"][c], o_mc[c]), (steps, c)
        assert torch.equal(obs["pv"], o_pv) and torch.equal(obs["ev-charging"], o_ev), steps
        assert torch.equal(fb.x, tb.x) and torch.equal(fs.soc, ts.soc), steps
        assert torch.equal(A["ev-charging"].req, ev.req) and torch.equal(A["ev-charging"].charging, ev.charging), steps
        for f, t in ((fb, tb), (fp, tp), (fs, ts), (A["pv"], pv), (A["ev-charging"], ev)):
            assert f.real_power.dtype == F32 and torch.equal(f.real_power, t.real_power), (steps, f.name)
        assert torch.equal(fb._reward_state, tb._reward_state), steps
        assert torch.equal(rew["ev-charging"], r_ev) and torch.equal(rew["pv"], r_pv), steps
        assert torch.equal(rew["building"], r_mc) and torch.equal(A["building"].real_power, mc.real_power), steps
        # band reward: RN32 of the fp64 expression on the fp64 min_voltage
        assert rew["pv"].dtype == F32 and torch.equal(rew["pv"], _band(v_prev).float()), steps
        # MultiComponentEnv sums: RN32(((0 + c0) + c1) + c2) over the stored values, widened
        z = torch.zeros(n, dtype=torch.float64, device=DEV)
        want_p = ((z + fb.real_power.double()) + fp.real_power.double()) + fs.real_power.double()
        want_r = ((z + fb._reward_state.double()) + 0.0) + 0.0
        assert torch.equal(A["building"].real_power, want_p.float()), steps
        assert torch.equal(rew["building"], want_r.float()), steps
        # the bus load: ((0 + a0) + a1) + a2 in fp64 over the stored agent powers
        bus = ((z + A["building"].real_power.double()) + A["pv"].real_power.double()) + \
            A["ev-charging"].real_power.double()
        assert env._ma["bus_p"].dtype == torch.float64 and torch.equal(env._ma["bus_p"][0], bus), steps
        # the power flow: the standalone fp64 solve of that bus load
        pf.calculate_power_flow(current_time=env.time, p_controllable_consumed={"675c": bus})
        e_f, e_s = env.pf_solver.voltage_extrema(), pf.voltage_extrema()
        assert e_f[0].dtype == torch.float64
        assert torch.equal(e_f[0], e_s[0]) and torch.equal(e_f[1], e_s[1]), steps
        assert torch.equal(env.pf_solver.iterations, pf.iterations), steps
        v_prev = e_f[0].clone()
        steps += 1
        if done["__all__"] or steps == max_steps:
            break
    assert steps == max_steps or steps > 250          # (n = 200: the whole day)
    assert (env.pf_solver.iterations > 0).all()


def test_het_f32_episode_within_bound():
    """A free-running episode at n = 2048 against the fp64 fused step, the same
    actions (fp32-representable): observations and state within rtol 1e-3 /
    atol 1e-3 (EV requirements atol 1e-2), rewards within the same bound on all
    but a 1e-4 fraction (the battery clamp and the band kink are
    discontinuous).

    Measured (MI355X, 286 steps): worst observation error 0.0022 of the bound,
    worst state error 0.0068, worst reward error 0.06 of it; 0 of 1 757 184
    rewards outside, so the cap is not used."""
    n = 2048
    e32, e64 = _make(n), _make(n, torch.float64)
    assert e32._ma is not None and e64._ma is not None
    soc0 = _soc0(n, 31)
    for e in (e32, e64):
        e.reset()
        e.agent_dict["building"].env_dict["storage"].reset(init_storage=soc0.to(e.dtype))
    acts = _actions(n, 300, 32)
    names = ("building", "pv", "ev-charging")

    def flat(o):
        return torch.cat([o["building"]["building"], o["building"]["pv"], o["building"]["storage"],
                          o["pv"], o["ev-charging"]], 1)

    def worst(g, w, atol):
        return float(((g.double() - w).abs() / (1e-3 * w.abs() + atol)).max())

    bad_r = tot_r = steps = 0
    w_obs = w_state = w_rew = 0.0
    while True:
        a = acts[steps]
        o32, r32, d32, _ = e32.step(_het_act(a))
        o64, r64, d64, _ = e64.step(_het_act(a.double()))
        steps += 1
        w_obs = max(w_obs, worst(flat(o32), flat(o64), 1e-3))
        b32, b64 = e32.agent_dict["building"], e64.agent_dict["building"]
        w_state = max(w_state, worst(b32.env_dict["building"].x, b64.env_dict["building"].x, 1e-3),
                      worst(b32.env_dict["storage"].soc, b64.env_dict["storage"].soc, 1e-3),
                      worst(e32.agent_dict["ev-charging"].req, e64.agent_dict["ev-charging"].req, 1e-2))
        for nm in names:
            g, w = r32[nm].double(), r64[nm]
            err = (g - w).abs()
            out = err > 1e-3 * w.abs() + 1e-3
            bad_r += int(out.sum())
            tot_r += n
            w_rew = max(w_rew, float((err / (1e-3 * w.abs() + 1e-3)).max()))
        assert d32["__all__"] == d64["__all__"]
        if d64["__all__"]:
            break
    print("het f32 episode: steps %d, worst obs %.3g, state %.3g, reward %.3g of the bound; "
          "rewards outside %d of %d" % (steps, w_obs, w_state, w_rew, bad_r, tot_r))
    assert steps > 250
    assert w_obs <= 1.0, w_obs
    assert w_state <= 1.0, w_state
    assert bad_r <= 1e-4 * tot_r, (bad_r, tot_r)


def test_het_f32_checkpoint_roundtrip():
    """state_dict() / load_state_dict() of the fp32 HET env: save, 10 steps,
    restore, replay -- the same trajectory bit for bit."""
    n = 200
    env = _make(n)
    env.reset()
    env.agent_dict["building"].env_dict["storage"].reset(init_storage=_soc0(n, 41))
    acts = _actions(n, 15, 42)

    def run(a):
        o, r, d, _ = env.step(_het_act(a))
        flat = [o["building"][c] for c in ("building", "pv", "storage")] + [o["pv"], o["ev-charging"]] + \
            [r[k] for k in ("building", "pv", "ev-charging")] + list(env.pf_solver.voltage_extrema()) + \
            [env.pf_solver.iterations, env._ma["bus_p"]]
        return [t.clone() for t in flat], d["__all__"]

    for a in acts[:5]:
        run(a)
    sd = env.state_dict()
    ref = [run(a) for a in acts[5:]]
    env.load_state_dict(sd)
    again = [run(a) for a in acts[5:]]
    for t, ((x, dx), (y, dy)) in enumerate(zip(ref, again)):
        assert dx == dy
        for i, (u, w) in enumerate(zip(x, y)):
            assert u.dtype == w.dtype and torch.equal(u, w), (t, i)
    assert ref[0][0][0].dtype == F32


def test_het_f32_history_ring():
    """record_history=True on the fp32 multi-agent path: the ring is fp64 (the
    voltages are the fp64 power flow's; the stored fp32 agent powers widened)."""
    n = 70
    e_h, e_p = _make(n, record_history=True), _make(n)
    soc0 = _soc0(n, 51)
    for e in (e_h, e_p):
        e.reset()
        e.agent_dict["building"].env_dict["storage"].reset(init_storage=soc0)
    acts = _actions(n, 4, 52)
    want_v, want_p = [], []
    for a in acts:
        o_h, r_h, _, _ = e_h.step(_het_act(a))
        o_p, r_p, _, _ = e_p.step(_het_act(a))
        for nm in ("building", "pv", "ev-charging"):
            assert torch.equal(r_h[nm], r_p[nm])
        v = e_p.pf_solver.get_bus_voltages()
        want_v.append(torch.stack([v[x].clone() for x in e_p.pf_solver.feeder.node_names]))
        want_p.append(torch.stack([ag.real_power.double() for ag in e_p.agents]))
    v, p, names = e_h.voltage_history()
    assert v.dtype == torch.float64 and p.dtype == torch.float64
    assert names == list(e_p.pf_solver.feeder.node_names)
    assert torch.equal(v, torch.stack(want_v)) and torch.equal(p, torch.stack(want_p))


def test_f32_needs_a_fused_path():
    """fp32 storage has no generic path: fused=False, or a configuration neither
    fused step implements, raises."""
    from powergridworld_amd.multiagent_env import MultiAgentEnv
    from powergridworld_amd.scenarios.heterogeneous import make_env_config
    with pytest.raises(ValueError):
        MultiAgentEnv(**make_env_config(), num_envs=4, device=DEV, dtype=F32, fused=False)

    class OwnObs(MultiAgentEnv):
        def get_obs(self):
            return super().get_obs()
    with pytest.raises(ValueError):
        OwnObs(**make_env_config(), num_envs=4, device=DEV, dtype=F32)
