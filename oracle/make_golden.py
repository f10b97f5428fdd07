"""Golden-vector generator: runs the REFERENCE (``/root/reference``) in this build
container and writes small ``.npz`` fixtures under ``tests/golden/``.

Test infrastructure only -- never shipped, never run on the GPU box (the
reference does not exist there).  The committed fixtures are data: seeded
inputs and the reference's outputs.

How the reference is made importable:
  * ``gym`` -> ``oracle/_stubs/gym`` (first on sys.path);
  * ``ray`` absent -> the reference's own fallback (``multiagent_env.py:13-17``);
  * ``five_zone_rom_env.load_data`` is monkeypatched: the exogenous CSV is a
    missing blob, and the state-space pickle is NOT unpickled -- the model is
    rebuilt from ``powergridworld_amd/data/state_space_model.json`` (decoded
    from the pickle's opcodes by ``tools/import_reference_data.py``);
  * OpenDSS is absent: multi-agent fixtures use ``OraclePowerFlowSolver``
    (``oracle/pf_oracle.py``) behind the reference's ``PowerFlowSolver`` ABC,
    so every non-PF output is pinned by the reference and the voltages fed
    in are recorded in the fixture.
  * the battery's ``print`` on every obs (``energy_storage_env.py:172``) is
    sent to /dev/null.

Usage:  python oracle/make_golden.py [--only NAME]
"""
import argparse
import contextlib
import copy
import io
import json
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "_stubs"))
sys.path.insert(1, "/root/reference")
sys.path.insert(2, REPO)

from oracle.exogenous import synthetic_exogenous_frame  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
EXO = synthetic_exogenous_frame()


def _ss_models():
    with open(os.path.join(REPO, "powergridworld_amd", "data",
                           "state_space_model.json")) as f:
        zones = json.load(f)["zones"]
    models = []
    for z in zones:
        models.append({
            "ss_A": np.array([z["ss_A"]], dtype=np.float64),
            "ss_B": np.array([z["ss_B"]], dtype=np.float64),
            "ss_C": np.array([z["ss_C"]], dtype=np.int64),
            "ss_D": np.array([z["ss_D"]], dtype=np.int64),
            "ss_K": np.array([z["ss_K"]], dtype=np.float64),
            "input_sel_list": np.array([z["input_sel_list"]], dtype=np.int64),
            "mean_inputs": np.array([z["mean_inputs"]], dtype=np.int64),
            "mean_output": np.array([z["mean_output"]], dtype=np.float64),
            "neighbors": list(z["neighbors"]),
            "x_k": np.array([z["x_k"]], dtype=np.float64),
        })
    return models


def _patched_load_data(start_time=None, end_time=None):
    """Stand-in for five_zone_rom_env.load_data (five_zone_rom_env.py:30-52)
    with the synthetic frame and the opcode-decoded state-space model."""
    df = EXO
    start_time = pd.Timestamp(start_time) if start_time else df.index[0]
    end_time = pd.Timestamp(end_time) if end_time else df.index[-1]
    _df = df.loc[start_time:end_time]
    if _df is None or len(_df) == 0:
        raise ValueError("empty exogenous range")
    return _df, _ss_models()


import gridworld  # noqa: E402
from gridworld import MultiComponentEnv, MultiAgentEnv  # noqa: E402
from gridworld.agents.buildings import five_zone_rom_env  # noqa: E402
five_zone_rom_env.load_data = _patched_load_data
from gridworld.agents.buildings import FiveZoneROMThermalEnergyEnv  # noqa: E402
from gridworld.agents.pv import PVEnv  # noqa: E402
from gridworld.agents.energy_storage import EnergyStorageEnv  # noqa: E402
from gridworld.agents.vehicles import EVChargingEnv  # noqa: E402
import logging  # noqa: E402
logging.getLogger("default").setLevel(logging.ERROR)


@contextlib.contextmanager
def quiet():
    with contextlib.redirect_stdout(io.StringIO()):
        yield


def _save(name, **arrays):
    os.makedirs(GOLDEN, exist_ok=True)
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, {k: np.shape(v) for k, v in arrays.items()})


def _actions(rng, T, K, dim, lo=-1.0, hi=1.0, overshoot=0.0):
    """Seeded actions; a few entries pushed past the box to exercise to_raw's clip."""
    a = rng.uniform(lo, hi, size=(T, K, dim))
    if overshoot > 0:
        mask = rng.random((T, K, dim)) < 0.05
        a[mask] *= (1.0 + overshoot)
    return a


# --------------------------------------------------------------------------
# Battery (energy_storage_env.py)
# --------------------------------------------------------------------------
def gen_battery():
    rng = np.random.default_rng(101)
    cases = {
        "default": dict(),
        "norescale": dict(rescale_spaces=False),
        "big": dict(storage_range=(3.0, 250.0), max_power=20.0,
                    charge_efficiency=0.9, discharge_efficiency=0.85),
    }
    for cname, cfg in cases.items():
        K, T = 8, 300
        init = np.concatenate([[3.0, 50.0, 1.0, 400.0],
                               rng.uniform(3.0, 50.0, K - 4)])
        acts = _actions(rng, T, K, 1, overshoot=0.3)
        if not cfg.get("rescale_spaces", True):
            acts = np.clip(acts, -1, 1)
        acts[:20, 0, 0] = 1.0     # drive env 0 to the discharge clamp
        acts[:20, 1, 0] = -1.0    # env 1 to the charge clamp
        obs = np.zeros((T + 1, K, 1)); rp = np.zeros((T, K)); rew = np.zeros((T, K))
        done = np.zeros((T, K), bool); soc = np.zeros((T + 1, K))
        envs = [EnergyStorageEnv(name="storage", **cfg) for _ in range(K)]
        with quiet():
            for k, e in enumerate(envs):
                o, _ = e.reset(init_storage=init[k])
                obs[0, k] = o; soc[0, k] = e.current_storage
            for t in range(T):
                for k, e in enumerate(envs):
                    o, r, d, _ = e.step(acts[t, k])
                    obs[t + 1, k] = o; rp[t, k] = e.real_power; rew[t, k] = r
                    done[t, k] = d; soc[t + 1, k] = e.current_storage
        _save("battery_" + cname, config=json.dumps(cfg), init_storage=init,
              actions=acts, obs=obs, real_power=rp, reward=rew, done=done, soc=soc)


# --------------------------------------------------------------------------
# PV (pv_profile_env.py)
# --------------------------------------------------------------------------
def gen_pv():
    rng = np.random.default_rng(202)
    cases = {
        "default": dict(profile_csv="pv_profile.csv", scaling_factor=40.0),
        "norescale": dict(profile_csv="pv_profile.csv", scaling_factor=10.0,
                          rescale_spaces=False),
        "offpeak_short": dict(profile_csv="off-peak.csv", scaling_factor=40.0,
                              max_episode_steps=100),
    }
    for cname, cfg in cases.items():
        K, T = 4, 286 if "max_episode_steps" not in cfg else 99
        acts = _actions(rng, T, K, 1, overshoot=0.2)
        if not cfg.get("rescale_spaces", True):
            acts = rng.uniform(0, 1, size=(T, K, 1))
        envs = [PVEnv(name="pv", **cfg) for _ in range(K)]
        obs = np.zeros((T, K, 1)); rp = np.zeros((T, K)); done = np.zeros((T, K), bool)
        rew = np.zeros((T, K))
        for e in envs:
            assert e.reset() is None
        for t in range(T):
            for k, e in enumerate(envs):
                o, r, d, _ = e.step(acts[t, k])
                obs[t, k] = o; rp[t, k] = e.real_power; done[t, k] = d; rew[t, k] = r
        _save("pv_" + cname, config=json.dumps(cfg), actions=acts, obs=obs,
              real_power=rp, reward=rew, done=done)


# --------------------------------------------------------------------------
# Building (five_zone_rom_env.py) -- standalone, lagged reward
# --------------------------------------------------------------------------
def gen_building():
    rng = np.random.default_rng(303)
    cases = {
        "default": dict(start_time="08-12-2020 00:00:00", end_time="08-13-2020 00:00:00"),
        "tests_obs": dict(start_time="08-12-2020 00:00:00", end_time="08-13-2020 00:00:00",
                          rescale_spaces=False,
                          obs_config={"zone_temp": (18, 34), "p_consumed": (-100, 100)}),
        "allobs": dict(start_time="08-12-2020 06:00:00", end_time="08-12-2020 12:00:00",
                       obs_config={"zone_temp": (16., 40.), "zone_upper_viol": (-10., 10.),
                                   "zone_lower_viol": (-10., 10.), "comfort_lower": (20., 23.),
                                   "comfort_upper": (23., 29.), "outdoor_temp": (0., 56.),
                                   "p_setpoint": (0., 200.), "p_consumed": (0., 200.),
                                   "time_of_day": (0., 1.), "bus_voltage": (0.9, 1.1),
                                   "min_voltage": (0.9, 1.1), "max_voltage": (0.9, 1.1)}),
    }
    for cname, cfg in cases.items():
        K = 4
        envs = [FiveZoneROMThermalEnergyEnv(name="building", **cfg) for _ in range(K)]
        T1 = envs[0].max_episode_steps - 1     # steps until done
        T2 = 20                                # second episode (x_k carry-over)
        odim = envs[0].observation_space.shape[0]
        for ep, T in enumerate([T1, T2]):
            acts = _actions(rng, T, K, 6, overshoot=0.2)
            if not cfg.get("rescale_spaces", True):
                lo, hi = envs[0]._action_space.low, envs[0]._action_space.high
                acts = rng.uniform(lo, hi, size=(T, K, 6))
            obs = np.zeros((T + 1, K, odim)); rew = np.zeros((T, K)); rp = np.zeros((T, K))
            done = np.zeros((T, K), bool); xk = np.zeros((T + 1, K, 5))
            for k, e in enumerate(envs):
                obs[0, k] = e.reset()
                xk[0, k] = [float(np.squeeze(m["x_k"])) for m in e.models]
            for t in range(T):
                for k, e in enumerate(envs):
                    o, r, d, _ = e.step(acts[t, k])
                    obs[t + 1, k] = o; rew[t, k] = r; rp[t, k] = e.real_power
                    done[t, k] = d
                    xk[t + 1, k] = [float(np.squeeze(m["x_k"])) for m in e.models]
            _save("building_%s_ep%d" % (cname, ep), config=json.dumps(cfg),
                  actions=acts, obs=obs, reward=rew, real_power=rp, done=done,
                  x_k=xk, max_episode_steps=envs[0].max_episode_steps)


# --------------------------------------------------------------------------
# EV charging (ev_charging_env.py)
# --------------------------------------------------------------------------
EV_NB_CONFIG = dict(num_vehicles=100, minutes_per_step=5, max_charge_rate_kw=7.,
                    peak_threshold=250., vehicle_multiplier=5., rescale_spaces=False)


def gen_ev():
    rng = np.random.default_rng(404)
    cases = {
        "notebook": dict(EV_NB_CONFIG),
        "rescaled": dict(EV_NB_CONFIG, rescale_spaces=True),
        "hetero25": dict(num_vehicles=25, minutes_per_step=5, max_charge_rate_kw=7.,
                         peak_threshold=200., vehicle_multiplier=40., rescale_spaces=True),
    }
    for cname, cfg in cases.items():
        K = 4
        envs = [EVChargingEnv(**cfg) for _ in range(K)]
        T = int(envs[0].max_episode_steps) - 2
        if cfg["rescale_spaces"]:
            acts = _actions(rng, T, K, 1, overshoot=0.2)
        else:
            acts = rng.uniform(0, 1, size=(T, K, 1))
            acts[:, 0, 0] = 1.0   # the notebook's "high" policy in env 0
            acts[:, 1, 0] = 0.0   # "low" in env 1
        obs = np.zeros((T + 1, K, 6)); rew = np.zeros((T, K)); rp = np.zeros((T, K))
        done = np.zeros((T, K), bool)
        for k, e in enumerate(envs):
            obs[0, k], _ = e.reset()
        for t in range(T):
            for k, e in enumerate(envs):
                o, r, d, _ = e.step(acts[t, k])
                obs[t + 1, k] = o; rew[t, k] = r; rp[t, k] = e.real_power; done[t, k] = d
        assert done[-1].all() and not done[:-1].any()
        _save("ev_" + cname, config=json.dumps(cfg), actions=acts, obs=obs,
              reward=rew, real_power=rp, done=done)


def gen_ev_random():
    """randomize=True (ev_charging_env.py:154-156): each env's DataFrame.sample
    draws its own vehicles from NumPy's global state.  Two episodes per env; the
    sampled row ids (the 'index' column reset_index() keeps) are recorded so
    the engine can inject the same subsets."""
    rng = np.random.default_rng(606)
    np.random.seed(606)
    cases = {
        "hetero25": dict(num_vehicles=25, minutes_per_step=5, max_charge_rate_kw=7.,
                         peak_threshold=200., vehicle_multiplier=40., rescale_spaces=True,
                         randomize=True),
        "v100": dict(EV_NB_CONFIG, rescale_spaces=True, randomize=True),
    }
    for cname, cfg in cases.items():
        K, EP = 4, 2
        envs = [EVChargingEnv(**cfg) for _ in range(K)]
        V = cfg["num_vehicles"]
        T = int(envs[0].max_episode_steps) - 2
        acts = _actions(rng, EP * T, K, 1, overshoot=0.2).reshape(EP, T, K, 1)
        obs = np.zeros((EP, T + 1, K, 6)); rew = np.zeros((EP, T, K)); rp = np.zeros((EP, T, K))
        ids = np.zeros((EP, K, V), np.int64)
        for ep in range(EP):
            for k, e in enumerate(envs):
                obs[ep, 0, k], _ = e.reset()
                ids[ep, k] = e.df["index"].values
            for t in range(T):
                for k, e in enumerate(envs):
                    o, r, d, _ = e.step(acts[ep, t, k])
                    obs[ep, t + 1, k] = o; rew[ep, t, k] = r; rp[ep, t, k] = e.real_power
        _save("ev_random_" + cname, config=json.dumps(cfg), vehicle_ids=ids, actions=acts, obs=obs,
              reward=rew, real_power=rp)


# --------------------------------------------------------------------------
# MultiComponentEnv C3: building + PV + battery + EV (base.py:74-182)
# --------------------------------------------------------------------------
def c3_components():
    return [
        {"name": "building", "cls": FiveZoneROMThermalEnergyEnv, "config": {}},
        {"name": "pv", "cls": PVEnv,
         "config": {"profile_csv": "pv_profile.csv", "scaling_factor": 40.}},
        {"name": "storage", "cls": EnergyStorageEnv, "config": {}},
        {"name": "ev", "cls": EVChargingEnv,
         "config": dict(EV_NB_CONFIG, rescale_spaces=True)},
    ]


def gen_mc():
    rng = np.random.default_rng(505)
    K = 3
    envs = [MultiComponentEnv(name="mc", components=c3_components()) for _ in range(K)]
    names = [e.name for e in envs[0].envs]
    dims = {e.name: e.observation_space.shape[0] for e in envs[0].envs}
    adims = {e.name: e.action_space.shape[0] for e in envs[0].envs}
    T = 285
    init = np.zeros(K)
    acts = {n: _actions(rng, T, K, adims[n], overshoot=0.1) for n in names}
    obs = {n: np.zeros((T + 1, K, dims[n])) for n in names}
    rew = np.zeros((T, K)); rp = np.zeros((T, K)); done = np.zeros((T, K), bool)
    with quiet():
        for k, e in enumerate(envs):
            # MC.reset forwards kwargs to every component and the EV step_reward
            # rejects them (base.py:110, ev_charging_env.py:163,259), so the SoC
            # drawn by the reference's global RNG is recorded and injected instead.
            o, _ = e.reset()
            init[k] = e.env_dict["storage"].current_storage
            for n in names:
                obs[n][0, k] = o[n]
        for t in range(T):
            for k, e in enumerate(envs):
                o, r, d, _ = e.step({n: acts[n][t, k] for n in names})
                for n in names:
                    obs[n][t + 1, k] = o[n]
                rew[t, k] = r; rp[t, k] = e.real_power; done[t, k] = d
    arrays = dict(init_storage=init, reward=rew, real_power=rp, done=done,
                  names=np.array(names))
    for n in names:
        arrays["act_" + n] = acts[n]
        arrays["obs_" + n] = obs[n]
    _save("mc_c3", **arrays)


# --------------------------------------------------------------------------
# C4: 5 coordinated buildings + power flow (multiagent_env.py + train.py:37-88)
# --------------------------------------------------------------------------
from gridworld.distribution_system.powerflow import PowerFlowSolver  # noqa: E402
from gridworld.scenarios.buildings import make_env_config  # noqa: E402
from oracle.pf_oracle import BatchedPF  # noqa: E402


class OraclePowerFlowSolver(PowerFlowSolver):
    """The oracle PF behind the reference's PowerFlowSolver ABC (OpenDSS is absent).
    semantics: "exact" (the fixed point) or "opendss" (OpenDSS's stopped snap
    iterate, Feeder.snap_opendss -- the rule the reference's OpenDSSSolver runs,
    opendss.py:131-135)."""

    def __init__(self, system_load_rescale_factor=1.0, semantics="exact", **kwargs):
        self.pf = BatchedPF(system_load_rescale_factor=system_load_rescale_factor, semantics=semantics)
        self.bus_voltages = {}
        self.trace = []

    def calculate_power_flow(self, p_controllable_consumed=None, q_controllable_consumed=None,
                             current_time=None):
        pu = self.pf.calculate(current_time, p_controllable_consumed, q_controllable_consumed, K=1)[0]
        self.bus_voltages = dict(zip(self.pf.feeder.node_names, pu))
        self.trace.append(pu.copy())

    def get_bus_voltages(self):
        return self.bus_voltages

    def get_bus_voltage_by_name(self, bus_name):
        PHASE_MAP = {'a': '.1', 'b': '.2', 'c': '.3'}
        if bus_name[-1] in PHASE_MAP.keys():
            return self.bus_voltages[bus_name.replace(bus_name[-1], PHASE_MAP[bus_name[-1]])]
        return [self.bus_voltages[x] for x in [bus_name + p for p in PHASE_MAP.values()]]


class CoordinatedEnv(MultiAgentEnv):
    """Restates CoordinatedMultiBuildingControlEnv (examples/marl/openai/train.py:37-88),
    whose module cannot be imported here (tensorflow/maddpg)."""
    VOLTAGE_LIMITS = [0.95, 1.05]
    VV_UNIT_PENALTY = 1e4

    def reward_transform(self, rew_dict):
        vv = self.get_voltage_violation()
        for key in rew_dict.keys():
            rew_dict[key] -= (vv * self.VV_UNIT_PENALTY / len(rew_dict))
        return rew_dict

    def meta_transform(self, meta):
        meta.update({'voltage_violation': self.get_voltage_violation()})
        return meta

    def get_voltage_violation(self):
        bus_id = list(set(self.agent_name_bus_map.values()))[0]
        v = self.pf_solver.get_bus_voltage_by_name(bus_id)
        return max([0.0, self.VOLTAGE_LIMITS[0] - v, v - self.VOLTAGE_LIMITS[1]])


def gen_c4(semantics="exact"):
    rng = np.random.default_rng(606)
    K, NA = 2, 5
    T = 286
    cfg = make_env_config(building_config={},
                          pv_config={"profile_csv": "pv_profile.csv", "scaling_factor": 40.},
                          storage_config={"max_power": 15., "storage_range": (3., 50.)},
                          system_load_rescale_factor=1.2, num_buildings=NA)
    cfg["pf_config"] = {"cls": OraclePowerFlowSolver,
                        "config": {"system_load_rescale_factor": 1.2, "semantics": semantics}}
    acts = rng.uniform(-1, 1, size=(T, NA, K, 8))
    mask = rng.random(acts.shape) < 0.03
    acts[mask] *= 1.2
    obs = np.zeros((T + 1, NA, K, 17)); rew = np.zeros((T, NA, K)); vv = np.zeros((T, K))
    done = np.zeros((T, K), bool); soc0 = np.zeros((NA, K)); v675 = np.zeros((T + 1, K))
    for k in range(K):
        env = CoordinatedEnv(**copy.deepcopy(cfg))
        names = [a.name for a in env.agents]
        with quiet():
            o = env.reset()
        for a, nm in enumerate(names):
            soc0[a, k] = env.agent_dict[nm].env_dict["storage"].current_storage
            obs[0, a, k] = np.concatenate([o[nm]["building"], o[nm]["pv"], o[nm]["storage"]])
        v675[0, k] = env.pf_solver.get_bus_voltage_by_name("675c")
        for t in range(T):
            action = {nm: {"building": acts[t, a, k, :6], "pv": acts[t, a, k, 6:7],
                           "storage": acts[t, a, k, 7:8]} for a, nm in enumerate(names)}
            with quiet():
                o, r, d, m = env.step(action)
            for a, nm in enumerate(names):
                obs[t + 1, a, k] = np.concatenate([o[nm]["building"], o[nm]["pv"], o[nm]["storage"]])
                rew[t, a, k] = r[nm]
            vv[t, k] = m["voltage_violation"]
            done[t, k] = d["__all__"]
            v675[t + 1, k] = env.pf_solver.get_bus_voltage_by_name("675c")
    assert done[-1].all() and not done[:-1].any()
    _save("c4_coordinated" + _SUFFIX[semantics], actions=acts, obs=obs, reward=rew, voltage_violation=vv,
          done=done, init_storage=soc0, v675=v675)


_SUFFIX = {"exact": "", "opendss": "_od"}


def _c4_cfg(semantics="exact"):
    cfg = make_env_config(building_config={},
                          pv_config={"profile_csv": "pv_profile.csv", "scaling_factor": 40.},
                          storage_config={"max_power": 15., "storage_range": (3., 50.)},
                          system_load_rescale_factor=1.2, num_buildings=5)
    cfg["pf_config"] = {"cls": OraclePowerFlowSolver,
                        "config": {"system_load_rescale_factor": 1.2, "semantics": semantics}}
    return cfg


def gen_c4_episodes(semantics="exact"):
    """C4 across the episode boundary: two full episodes per env, with the SoC
    the reference draws at each reset (energy_storage_env.py:80-95) and every
    building's x_k (persists across reset, five_zone_rom_env.py:147-176;
    MultiAgentEnv.reset, multiagent_env.py:125-140) recorded after the resets
    and after every step."""
    rng = np.random.default_rng(616)
    K, NA, E, T = 2, 5, 2, 286
    acts = rng.uniform(-1, 1, size=(E, T, NA, K, 8))
    acts[rng.random(acts.shape) < 0.03] *= 1.2
    obs = np.zeros((E, T + 1, NA, K, 17)); rew = np.zeros((E, T, NA, K)); vv = np.zeros((E, T, K))
    done = np.zeros((E, T, K), bool); soc0 = np.zeros((E, NA, K)); v675 = np.zeros((E, T + 1, K))
    xk = np.zeros((E, T + 1, NA, K, 5))
    for k in range(K):
        env = CoordinatedEnv(**copy.deepcopy(_c4_cfg(semantics)))
        names = [a.name for a in env.agents]

        def snap(e, t):
            for a, nm in enumerate(names):
                ag = env.agent_dict[nm]
                xk[e, t, a, k] = [float(np.ravel(m["x_k"])[0])
                                  for m in ag.env_dict["building"].models]
            v675[e, t, k] = env.pf_solver.get_bus_voltage_by_name("675c")

        for e in range(E):
            with quiet():
                o = env.reset()
            for a, nm in enumerate(names):
                soc0[e, a, k] = env.agent_dict[nm].env_dict["storage"].current_storage
                obs[e, 0, a, k] = np.concatenate([o[nm]["building"], o[nm]["pv"], o[nm]["storage"]])
            snap(e, 0)
            for t in range(T):
                action = {nm: {"building": acts[e, t, a, k, :6], "pv": acts[e, t, a, k, 6:7],
                               "storage": acts[e, t, a, k, 7:8]} for a, nm in enumerate(names)}
                with quiet():
                    o, r, d, m = env.step(action)
                for a, nm in enumerate(names):
                    obs[e, t + 1, a, k] = np.concatenate([o[nm]["building"], o[nm]["pv"],
                                                          o[nm]["storage"]])
                    rew[e, t, a, k] = r[nm]
                vv[e, t, k] = m["voltage_violation"]
                done[e, t, k] = d["__all__"]
                snap(e, t + 1)
    assert done[:, -1].all() and not done[:, :-1].any()
    _save("c4_two_episodes" + _SUFFIX[semantics], actions=acts, obs=obs, reward=rew, voltage_violation=vv,
          done=done, init_storage=soc0, v675=v675, x_k=xk)


# --------------------------------------------------------------------------
# Heterogeneous 3-agent scenario (gridworld/scenarios/heterogeneous.py:13-112):
# MC building (alpha 0) + grid-aware PV farm rewarded on min_voltage + EV 25x40
# --------------------------------------------------------------------------
from gridworld.scenarios.heterogeneous import make_env_config as make_het_config  # noqa: E402


def gen_het(semantics="exact"):
    rng = np.random.default_rng(707)
    K = 2
    cfg = make_het_config()
    cfg["pf_config"] = {"cls": OraclePowerFlowSolver,
                        "config": {"system_load_rescale_factor": 0.65, "semantics": semantics}}
    rows = []
    for k in range(K):
        env = MultiAgentEnv(**copy.deepcopy(cfg))
        with quiet():
            o = env.reset()
        soc0 = env.agent_dict["building"].env_dict["storage"].current_storage
        rec = dict(soc0=soc0, obs=[o], rew=[], done=[], volt=[env.pf_solver.trace[-1]], acts=[])
        while True:
            a = {"building": {"building": rng.uniform(-1, 1, 6), "pv": rng.uniform(-1, 1, 1),
                              "storage": rng.uniform(-1, 1, 1)},
                 "pv": rng.uniform(-1, 1, 1), "ev-charging": rng.uniform(-1, 1, 1)}
            with quiet():
                o, r, d, _ = env.step(a)
            rec["acts"].append(a)
            rec["obs"].append(o)
            rec["rew"].append(r)
            rec["done"].append(d["__all__"])
            rec["volt"].append(env.pf_solver.trace[-1])
            if d["__all__"]:
                break
        rows.append(rec)
    T = len(rows[0]["rew"])
    assert all(len(r["rew"]) == T for r in rows)
    flat_obs = lambda o: np.concatenate([o["building"]["building"], o["building"]["pv"],
                                         o["building"]["storage"], o["pv"], o["ev-charging"]])
    flat_act = lambda a: np.concatenate([a["building"]["building"], a["building"]["pv"],
                                         a["building"]["storage"], a["pv"], a["ev-charging"]])
    agents = ["building", "pv", "ev-charging"]
    _save("het_scenario" + _SUFFIX[semantics],
          init_storage=np.array([r["soc0"] for r in rows]),
          actions=np.stack([[flat_act(r["acts"][t]) for r in rows] for t in range(T)]),
          obs=np.stack([[flat_obs(r["obs"][t]) for r in rows] for t in range(T + 1)]),
          reward=np.stack([[[r["rew"][t][a] for a in agents] for r in rows] for t in range(T)]),
          done=np.array([[r["done"][t] for r in rows] for t in range(T)]),
          voltages=np.stack([[r["volt"][t] for r in rows] for t in range(T + 1)]),
          node_names=np.array(BatchedPF().feeder.node_names))


# --------------------------------------------------------------------------
# Home-Steward path: HSMultiComponentEnv of [HSPVEnv,
# HSEnergyStorageEnv, HSEVChargingEnv, HSDevicesEnv] with the shipped JSON
# scenario (gridworld/base_hs.py, scenarios/heterogeneous_hs.py); two
# episodes per env so the state that survives reset is exercised.
# --------------------------------------------------------------------------
def gen_hs():
    from gridworld import HSMultiComponentEnv
    from gridworld.scenarios.heterogeneous_hs import make_env_config as make_hs_config
    rng = np.random.default_rng(808)
    K, EPISODES = 4, 2
    cfg = make_hs_config()
    names = [c["name"] for c in cfg["components"]]
    runs = []
    for k in range(K):
        env = HSMultiComponentEnv(**copy.deepcopy(cfg))
        rec = dict(obs=[], act=[], rew=[], rp=[], done=[], meta=[], soc=[], smeta=[], sts=[])
        for ep in range(EPISODES):
            with quiet():
                o = env.reset()
            rec["obs"].append(np.concatenate([np.ravel(o[n]) for n in names]))
            rec["meta"].append([np.nan] * 3)
            rec["soc"].append(env.env_dict["storage"].current_storage)
            while True:
                # actions slightly beyond [-1, 1] exercise the clips; a few exact
                # zeros and ends exercise the zero-power branches
                a = rng.uniform(-1.1, 1.1, len(names))
                a[rng.random(len(names)) < 0.05] = 0.0
                a[rng.random(len(names)) < 0.03] = -1.0
                with quiet():
                    o, r, d, m = env.step({n: a[i:i + 1].copy() for i, n in enumerate(names)})
                rec["act"].append(a)
                rec["obs"].append(np.concatenate([np.ravel(o[n]) for n in names]))
                rec["rew"].append(float(r))
                rec["rp"].append(float(env.real_power))
                rec["done"].append(bool(d))
                rec["meta"].append([m["pv_power"], m["es_power"], m["grid_power"]])
                # the per-device step_meta records (base_hs.py:133-164), numeric fields
                # in the reference's key order, custom-info keys recorded once
                sm = np.full((len(names), HS_META_FIELDS), np.nan)
                assert [r["device_id"] for r in m["step_meta"]] == names
                for c, r in enumerate(m["step_meta"]):
                    assert r["timestamp"] == m["timestamp"]
                    vals = [r["cost"], r["reward"], r["action"][0], r["solar_power_consumed"],
                            r["es_power_consumed"], r["grid_power_consumed"]]
                    vals += list(r["device_custom_info"].values())
                    sm[c, :len(vals)] = vals
                    HS_CUSTOM_KEYS[c] = list(r["device_custom_info"].keys())
                rec["smeta"].append(sm)
                rec["sts"].append(str(m["timestamp"]))
                rec["soc"].append(env.env_dict["storage"].current_storage)
                if d:
                    break
        runs.append(rec)
    T = len(runs[0]["rew"])
    assert all(len(r["rew"]) == T for r in runs)
    stack = lambda key: np.stack([np.asarray(r[key], dtype=np.float64) for r in runs], 1)
    assert all(r["sts"] == runs[0]["sts"] for r in runs)
    _save("hs_scenario", names=np.array(names), actions=stack("act"), obs=stack("obs"),
          reward=stack("rew"), real_power=stack("rp"), done=stack("done").astype(bool),
          meta=stack("meta"), soc=stack("soc"), episodes=np.array(EPISODES),
          step_meta=stack("smeta"), step_meta_timestamp=np.array(runs[0]["sts"]),
          step_meta_custom_keys=np.array([",".join(HS_CUSTOM_KEYS[c]) for c in range(len(names))]))


HS_META_FIELDS = 13
HS_CUSTOM_KEYS = {}


# The same house with the chain in another order -- [PV (grid-aware), EV,
# devices, storage] -- and a per-step min_voltage keyword: the devices draw on
# the resources before the storage does, the storage's reward sees what the EV
# and the devices left.  (A component ahead of the PV is not a configuration the
# reference runs: its meta_state pv_power is None until the PV's first step,
# and the EV's reset step and every component's step_meta subtract from it.)
def gen_hs_order():
    from gridworld import HSMultiComponentEnv
    from gridworld.scenarios.heterogeneous_hs import make_env_config as make_hs_config
    rng = np.random.default_rng(909)
    K, EPISODES = 3, 2
    cfg = make_hs_config()
    by = {c["name"]: c for c in cfg["components"]}
    cfg["components"] = [by["pv"], by["ev-charging"], by["other-devices"], by["storage"]]
    by["pv"]["config"]["grid_aware"] = True
    names = [c["name"] for c in cfg["components"]]
    runs = []
    for k in range(K):
        env = HSMultiComponentEnv(**copy.deepcopy(cfg))
        rec = dict(obs=[], act=[], rew=[], rp=[], done=[], meta=[], soc=[], mv=[])
        for ep in range(EPISODES):
            mv = float(rng.uniform(0.88, 1.12))
            rec["mv"].append(mv)
            with quiet():
                o = env.reset(min_voltage=mv)
            rec["obs"].append(np.concatenate([np.ravel(o[n]) for n in names]))
            rec["meta"].append([np.nan] * 3)
            rec["soc"].append(env.env_dict["storage"].current_storage)
            while True:
                a = rng.uniform(-1.1, 1.1, len(names))
                a[rng.random(len(names)) < 0.05] = 0.0
                mv = float(rng.uniform(0.88, 1.12))
                with quiet():
                    o, r, d, m = env.step({n: a[i:i + 1].copy() for i, n in enumerate(names)}, min_voltage=mv)
                rec["act"].append(a)
                rec["mv"].append(mv)
                rec["obs"].append(np.concatenate([np.ravel(o[n]) for n in names]))
                rec["rew"].append(float(r))
                rec["rp"].append(float(env.real_power))
                rec["done"].append(bool(d))
                rec["meta"].append([m["pv_power"], m["es_power"], m["grid_power"]])
                rec["soc"].append(env.env_dict["storage"].current_storage)
                if d:
                    break
        runs.append(rec)
    stack = lambda key: np.stack([np.asarray(r[key], dtype=np.float64) for r in runs], 1)
    _save("hs_order", names=np.array(names), actions=stack("act"), obs=stack("obs"), reward=stack("rew"),
          real_power=stack("rp"), done=stack("done").astype(bool), meta=stack("meta"), soc=stack("soc"),
          min_voltage=stack("mv"), episodes=np.array(EPISODES))


# The house off the shipped scenario (tests/_hs_direct_common.py replays these):
# synthetic configs that reach what hs_scenario / hs_order never do -- several
# vehicles charging at once, indices >= 32 and vehicle 63, vehicles departing
# unserved, a grid cap that binds, grid costs <= 0, device rows that are exact
# zeros or sit at round(x, 3)'s 0.0005 edge, a storage range narrow enough for
# both SoC limits, rescale_spaces off, 1 / 2 / 3 / 4 device columns, the chain
# [pv, devices, storage, ev].  Each fixture holds the whole config as JSON
# (settings only), so a test rebuilds pgw_hs_params / pgw_hs_step_info from it,
# and the charging / departed vehicle lists in the reference's own iteration
# order (CPython's set order, ev_charging_env_hs.py:201-206).
HS_EDGE_NAMES = {"pv": "HSPVEnv", "storage": "HSEnergyStorageEnv", "ev-charging": "HSEVChargingEnv",
                 "other-devices": "HSDevicesEnv"}
HS_EDGE_ACT = {"pv": (0.98, 1.0), "storage": (-1.0, 1.0), "ev-charging": (0.0, 1.0), "other-devices": (0.99, 1.0)}
HS_EDGE_STEPS = 60


def _hs_edge_vehicles(rng, n, active, lo_park, hi_park, pinned=()):
    """A vehicle table of n rows: the rows in `active` park inside the
    episode (overlapping windows, parks of lo_park..hi_park minutes: some too
    short for their energy), the others long after it.  `pinned` rows share
    one window with at least two others, so they charge together."""
    T = HS_EDGE_STEPS * 5
    rows = []
    for v in range(n):
        if v in active:
            start = float(rng.integers(0, T - 40)) + float(rng.choice([0.0, 0.0, 2.5, 4.0]))
            park = float(rng.integers(lo_park, hi_park))
            need = float(np.round(rng.uniform(0.3, 6.0), 3))
        else:
            start, park, need = 5000.0 + 5 * v, 30.0, 4.0
        rows.append([start, start + park, need])
    for k, v in enumerate(pinned):
        rows[v][0], rows[v][1] = 60.0 + 5.0 * (k % 2), 60.0 + 45.0 + 5.0 * (k % 3)
    return {"columns": ["start_time_min", "end_time_park_min", "energy_required_kwh"],
            "index": list(range(n)), "data": rows}


def _hs_edge_configs():
    rng = np.random.default_rng(4242)
    T = HS_EDGE_STEPS
    costs = lambda: [float(c) for c in rng.choice([-0.21, -0.05, 0.0, 0.0, 0.25847, 0.46, 0.57098], T)]
    stamps = [str(t) for t in pd.date_range("2022-06-29 06:00:00", periods=T, freq="5min")]

    def pv_data():
        d = rng.uniform(0.0, 9.0, T)
        d[rng.random(T) < 0.3] = 0.0
        return [float(x) for x in d]

    def devices(ncol, edge=False):
        d = {}
        for c in range(ncol):
            col = rng.uniform(0.0, 0.4, T + 1)
            col[rng.random(T + 1) < 0.25] = 0.0
            col[rng.random(T + 1) < 0.2] = rng.uniform(0.0, 0.001 / ncol)     # sums on both sides of 0.0005
            d["dev%d" % c] = col
        if edge:
            # rows whose sum is exactly the edge of round(x, 3) == 0.0 and its two
            # neighbours (one column holds it, the others exact zeros), and all zeros
            edges = [0.0005, float(np.nextafter(0.0005, 0.0)), float(np.nextafter(0.0005, 1.0)), 0.0, 0.0004, 0.0006]
            for k, x in enumerate(edges * 2):
                row = 3 + 4 * k
                for c in range(ncol):
                    d["dev%d" % c][row] = x if c == k % ncol else 0.0
        return {k: [float(x) for x in v] for k, v in d.items()}

    def comp(name, **config):
        return {"name": name, "cls": HS_EDGE_NAMES[name], "config": dict(config, minutes_per_step=5)}

    def house(tag, order, max_grid_power, parts):
        return {"tag": tag, "name": "house", "max_grid_power": max_grid_power, "max_episode_steps": T,
                "grid_cost": costs(), "timestamps": stamps, "components": [parts[k] for k in order]}

    out = []
    # a: the shipped order; 33 vehicles of which only rows < 8 ever park; one device column
    out.append(house("a", ["pv", "storage", "ev-charging", "other-devices"], 48, {
        "pv": comp("pv", profile_csv="", profile_data=pv_data(), rescale_spaces=True),
        "storage": comp("storage", max_power=6, storage_range=[3.0, 4.5], charge_efficiency=0.95,
                        discharge_efficiency=0.9, rescale_spaces=True, initial_storage_cost=0.25847,
                        max_storage_cost=0.57098),
        "ev-charging": comp("ev-charging", num_vehicles=8, max_charge_rate_kw=7.0, rescale_spaces=True,
                            max_charge_cost=0.57098, unserved_penalty=1.0,
                            profile_data=_hs_edge_vehicles(rng, 33, set(range(8)), 10, 45, pinned=(1, 4, 6))),
        "other-devices": comp("other-devices", profile_csv="", profile_data=devices(1), rescale_spaces=True)}))
    # b: hs_order's chain with a grid-aware PV; 64 vehicles, rows up to 63 park; three device
    # columns; the EV and the storage take raw actions
    out.append(house("b", ["pv", "ev-charging", "other-devices", "storage"], 400, {
        "pv": comp("pv", profile_csv="", profile_data=pv_data(), rescale_spaces=True, grid_aware=True),
        "storage": comp("storage", max_power=15.0, storage_range=[3.0, 50.0], charge_efficiency=0.93,
                        discharge_efficiency=0.87, rescale_spaces=False, initial_storage_cost=0.1,
                        max_storage_cost=0.55),
        "ev-charging": comp("ev-charging", num_vehicles=64, max_charge_rate_kw=7.0, rescale_spaces=False,
                            max_charge_cost=0.55, unserved_penalty=0.5, vehicle_multiplier=2,
                            profile_data=_hs_edge_vehicles(rng, 64, set(range(64)), 10, 60,
                                                           pinned=(31, 32, 63, 40, 57, 35, 9))),
        "other-devices": comp("other-devices", profile_csv="", profile_data=devices(3), rescale_spaces=True)}))
    # c: [pv, devices, storage, ev]; a 3 kW grid cap that the storage and the EV exhaust (the EV
    # last: its cost is guarded by `sum > 0`); four device columns with the round(x, 3) edges and
    # a raw device action; a raw PV action; a narrow storage range
    out.append(house("c", ["pv", "other-devices", "storage", "ev-charging"], 3, {
        "pv": comp("pv", profile_csv="", profile_data=pv_data(), rescale_spaces=False),
        "storage": comp("storage", max_power=15.0, storage_range=[3.0, 5.0], charge_efficiency=0.95,
                        discharge_efficiency=0.95, rescale_spaces=True, initial_storage_cost=0.0,
                        max_storage_cost=0.55),
        "ev-charging": comp("ev-charging", num_vehicles=16, max_charge_rate_kw=11.0, rescale_spaces=True,
                            max_charge_cost=0.55, unserved_penalty=1.0,
                            profile_data=_hs_edge_vehicles(rng, 64, set(range(0, 64, 2)) | {31, 63}, 10, 40,
                                                           pinned=(31, 32, 63, 62, 8))),
        "other-devices": comp("other-devices", profile_csv="", profile_data=devices(4, edge=True),
                              rescale_spaces=False)}))
    # d: the shipped order, nothing rescaled; 33 vehicles, every row parks; two device columns
    out.append(house("d", ["pv", "storage", "ev-charging", "other-devices"], 400, {
        "pv": comp("pv", profile_csv="", profile_data=pv_data(), rescale_spaces=False, grid_aware=True),
        "storage": comp("storage", max_power=6.0, storage_range=[0.5, 2.0], charge_efficiency=0.95,
                        discharge_efficiency=0.95, rescale_spaces=False, initial_storage_cost=0.3,
                        max_storage_cost=0.57098),
        "ev-charging": comp("ev-charging", num_vehicles=33, max_charge_rate_kw=7.0, rescale_spaces=False,
                            max_charge_cost=0.57098, unserved_penalty=2.0,
                            profile_data=_hs_edge_vehicles(rng, 33, set(range(33)), 10, 50, pinned=(32, 8, 16, 24))),
        "other-devices": comp("other-devices", profile_csv="", profile_data=devices(2, edge=True),
                              rescale_spaces=False)}))
    return out


def gen_hs_edges():
    import gridworld.agents.devices as rdev
    import gridworld.agents.energy_storage as rsto
    import gridworld.agents.pv as rpv
    import gridworld.agents.vehicles as rveh
    from gridworld import HSMultiComponentEnv
    classes = {"HSPVEnv": rpv.HSPVEnv, "HSEnergyStorageEnv": rsto.HSEnergyStorageEnv,
               "HSEVChargingEnv": rveh.HSEVChargingEnv, "HSDevicesEnv": rdev.HSDevicesEnv}
    K, EPISODES = 3, 2
    for ci, cfg in enumerate(_hs_edge_configs()):
        rng = np.random.default_rng(5150 + ci)
        text = json.dumps(cfg)                      # what the fixture holds: rebuilt from it below
        names = [c["name"] for c in cfg["components"]]
        rescale = [bool(c["config"]["rescale_spaces"]) for c in cfg["components"]]
        aware = any(c["config"].get("grid_aware") for c in cfg["components"])
        n_veh = len(cfg["components"][names.index("ev-charging")]["config"]["profile_data"]["data"])
        dev_slot = names.index("other-devices")
        runs = []
        for k in range(K):
            live = json.loads(text)
            live.pop("tag")
            for c in live["components"]:
                c["cls"] = classes[c["cls"]]
            env = HSMultiComponentEnv(**live)
            ev, sto, dev = env.env_dict["ev-charging"], env.env_dict["storage"], env.env_dict["other-devices"]
            rec = dict(obs=[], act=[], rew=[], rp=[], done=[], meta=[], soc=[], smeta=[], sts=[], mv=[], init=[],
                       chg=[], dep=[], req=[], costs=[])

            def state():
                pad = lambda l: [int(i) for i in l] + [-1] * (n_veh - len(l))
                rec["chg"].append(pad(ev.charging_vehicles))
                rec["dep"].append(pad(ev.departed_vehicles))
                rec["req"].append(np.array(ev.df["energy_required_kwh"], dtype=np.float64, copy=True))
                rec["costs"].append([float(sto.current_cost), float(getattr(ev, "current_cost", 0.0)),
                                     float(getattr(dev, "current_cost", 0.0))])
                rec["soc"].append(float(sto.current_storage))

            for ep in range(EPISODES):
                lo, hi = sto.storage_range
                init = float(rng.uniform(lo - 0.3, hi + 0.3))
                mv = float(rng.uniform(0.88, 1.12))
                rec["init"].append(init)
                rec["mv"].append(mv)
                with quiet():
                    o = env.reset(init_storage=init, **({"min_voltage": mv} if aware else {}))
                rec["obs"].append(np.concatenate([np.ravel(o[n]) for n in names]))
                rec["meta"].append([np.nan] * 3)
                state()
                while True:
                    a = rng.uniform(-1.1, 1.1, len(names))
                    a[rng.random(len(names)) < 0.05] = 0.0
                    a[rng.random(len(names)) < 0.04] = -1.0
                    a[rng.random(len(names)) < 0.04] = 1.0
                    for i, n in enumerate(names):
                        if not rescale[i]:          # a raw action, inside the component's own box
                            l, h = HS_EDGE_ACT[n]
                            a[i] = l + (np.clip(a[i], -1.0, 1.0) + 1.0) / 2.0 * (h - l)
                    if not rescale[dev_slot] and k < 2:
                        a[dev_slot] = 1.0           # exactly the row's sum: the 0.0005 edge rows
                    mv = float(rng.uniform(0.88, 1.12))
                    with quiet():
                        o, r, d, m = env.step({n: a[i:i + 1].copy() for i, n in enumerate(names)},
                                              **({"min_voltage": mv} if aware else {}))
                    rec["act"].append(a)
                    rec["mv"].append(mv)
                    rec["obs"].append(np.concatenate([np.ravel(o[n]) for n in names]))
                    rec["rew"].append(float(r))
                    rec["rp"].append(float(env.real_power))
                    rec["done"].append(bool(d))
                    rec["meta"].append([m["pv_power"], m["es_power"], m["grid_power"]])
                    sm = np.full((len(names), HS_META_FIELDS), np.nan)
                    assert [q["device_id"] for q in m["step_meta"]] == names
                    keys = []
                    for c, q in enumerate(m["step_meta"]):
                        vals = [q["cost"], q["reward"], q["action"][0], q["solar_power_consumed"],
                                q["es_power_consumed"], q["grid_power_consumed"]]
                        vals += list(q["device_custom_info"].values())
                        sm[c, :len(vals)] = vals
                        keys.append(",".join(q["device_custom_info"].keys()))
                    rec["smeta"].append(sm)
                    rec["sts"].append(str(m["timestamp"]))
                    state()
                    if d:
                        break
            runs.append(rec)
        stack = lambda key: np.stack([np.asarray(r[key], dtype=np.float64) for r in runs], 1)
        istack = lambda key: np.stack([np.asarray(r[key], dtype=np.int64) for r in runs], 1)
        T = len(runs[0]["rew"])
        assert T == EPISODES * HS_EDGE_STEPS and all(len(r["rew"]) == T for r in runs)
        # the reference alone completed, and nowhere did it divide 0 by 0 into a NaN
        for key in ("obs", "rew", "rp", "soc", "costs", "req"):
            assert np.isfinite(stack(key)).all(), (cfg["tag"], key)
        assert np.isfinite(stack("meta")[[t for t in range(T + EPISODES) if t % (HS_EDGE_STEPS + 1)]]).all()
        _save("hs_edges_" + cfg["tag"], names=np.array(names), config_json=np.array(text), actions=stack("act"),
              obs=stack("obs"), reward=stack("rew"), real_power=stack("rp"), done=stack("done").astype(bool),
              meta=stack("meta"), soc=stack("soc"), episodes=np.array(EPISODES), step_meta=stack("smeta"),
              step_meta_timestamp=np.array(runs[0]["sts"]), step_meta_custom_keys=np.array(keys),
              init_storage=stack("init"), min_voltage=stack("mv"), charging=istack("chg"), departed=istack("dep"),
              ev_req=stack("req"), costs=stack("costs"))


GENERATORS = {"battery": gen_battery, "pv": gen_pv, "building": gen_building,
              "ev": gen_ev, "evrand": gen_ev_random, "mc": gen_mc, "c4": gen_c4, "c4ep": gen_c4_episodes,
              "het": gen_het, "hs": gen_hs, "hs_order": gen_hs_order, "hs_edges": gen_hs_edges,
              # the reference's own power-flow rule (OpenDSS's snap solve, opendss.py:131-135)
              # through the reference's MultiAgentEnv: the same seeded action streams
              "c4_od": lambda: gen_c4("opendss"), "c4ep_od": lambda: gen_c4_episodes("opendss"),
              "het_od": lambda: gen_het("opendss")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    np.savez_compressed(os.path.join(GOLDEN, "exogenous_synthetic.npz"),
                        index_ns=EXO.index.values.astype("datetime64[ns]").astype(np.int64),
                        columns=np.array(list(EXO.columns)), values=EXO.values)
    for name, fn in GENERATORS.items():
        if args.only and name != args.only:
            continue
        # each generator draws from the reference's global NumPy RNG (the
        # battery's truncnorm SoC, energy_storage_env.py:83): seed it per
        # generator, so a full run and `--only NAME` give the same fixtures
        np.random.seed(0)
        fn()


if __name__ == "__main__":
    main()
