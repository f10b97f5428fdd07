"""Throughput of the BASELINE configs other than the headline C4 (BASELINE.md
section 4): C2 = EnergyStorageEnv defaults at batch 4096, C3 = the
MultiComponentEnv building + PV + storage + EV(100 vehicles) at batch 16384,
and HET = the reference's 3-agent heterogeneous scenario (scenarios/
heterogeneous.py) and HS = the Home-Steward house (base_hs.py) at 65536.  Each step goes through the public API
with actions resident in HBM (a pool of pre-generated batches); episodes reset
inside the timed region.  One JSON line per config.

Usage: python tools/bench_configs.py [--configs C2,C3,HET,HETG,HS,...] [--steps K] [--warmup W]
(HET: OpenDSS's snap-solve rule, the default, with its response table; HETS:
every env solved; HETX: the exact fixed point; HETG: the heterogeneous scenario
on the generic path, fused=False; HETF: HET with fp32 storage
(pgw_ma_step_f32); HETMG / HETMF: the heterogeneous agents on three buses
(675c, 634a, 684c), the power flow on the general kernel (multi_bus="general",
the default route) / on the fast kernel's multi-slot instantiation
(multi_bus="fast"); HETYG / HETYF: the heterogeneous scenario under
yprim="step" (every solve's Y holds its own loads' Yeq), the generic agents and
the general kernel (step_kernel="general", the default) / the fused multi-agent
step and the fast kernel (step_kernel="fast", pgw_pf_solve_h1); C4YG / C4YF:
the coordinated 5-building scenario (C4) at 65 536 envs under yprim="step",
step_kernel="fast", on the generic path (fused=False) / on the fused step
(pgw_coord_step_h1); HETPG / HETPF and C4PG / C4PF: the heterogeneous scenario
and C4 at 65 536 envs under snap_start="previous" (every env's solve continues
from its previous solution), start_kernel="general" (the default: the general
kernel, the generic paths) / "fast" (the fused steps with pgw_pf_solve_prev /
pgw_coord_step_prev); C3F / C3G8F:
C3 with fp32 storage (pgw_mc_agent_step_f32); C3L: C3 at
65 536 envs; C2Gk / C3Gk: the step replayed from captured hipGraphs of k steps,
C3 through the device clocks; C3Pk / HSPk: captured once per episode position,
powergridworld_amd/graph.py; HS32 / HS32P8: HS / HSP8 with fp32 storage
(pgw_hs_step_f32))
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# algorithmic HBM bytes per agent-env-step
BYTES = {"C2": 48, "C3": 1990}
# HETMG / HETMF: the heterogeneous agents' buses (building, PV farm, EV station)
MULTI_BUSES = ("675c", "634a", "684c")


def timed_loop(env, step, reset, steps, warmup):
    reset()
    for _ in range(warmup):
        if step():
            reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        if step():
            reset()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def graph_steps(env, acts, per, reset, clocked=False):
    """Captured steps (powergridworld_amd/graph.py) over the action pool: one
    graph per pool entry (per = 1: as if the policy wrote into one of the pool's
    buffers), or graphs of `per` consecutive pool entries (open-loop rollout).
    Returns step() -> done, advancing `per` env steps per call."""
    pool = len(acts)
    kw = {"clocked": True} if clocked else {}
    graphs = [env.capture_step(acts[i] if per == 1 else [acts[(i + j) % pool] for j in range(per)], steps=per, **kw)
              for i in range(0, pool, per)]
    reset()
    k = [0]

    def step():
        done = graphs[k[0] % len(graphs)]()[2]
        k[0] += 1
        return done
    return step


def bench_c2(dev, steps, warmup, n=4096, pool=64, graph=0):
    from powergridworld_amd.agents import EnergyStorageEnv
    env = EnergyStorageEnv(num_envs=n, device=dev)
    gen = torch.Generator(dev).manual_seed(0)
    acts = torch.empty((pool, n, 1), dtype=torch.float64, device=dev).uniform_(-1, 1, generator=gen)
    init = torch.empty(n, dtype=torch.float64, device=dev).uniform_(3.0, 50.0, generator=gen)
    k = [0]

    def step():
        _, _, done, _ = env.step(acts[k[0] % pool])
        k[0] += 1
        return done

    reset = lambda: env.reset(init_storage=init)
    if graph:
        step = graph_steps(env, list(acts), graph, reset)
        steps, warmup = steps // graph, warmup // graph
    dt = timed_loop(env, step, reset, steps, warmup)
    steps *= max(graph, 1)
    return dict(config="C2" + ("G%d" % graph if graph else ""),
                workload="EnergyStorageEnv defaults" + (", %d-step captured graphs" % graph if graph else ""),
                batch=n, agents=1, steps=steps, seconds=dt)


def c3_env(dev, n, pool=16, dtype=torch.float64):
    """The C3 agent and a pool of pre-generated action dicts (HBM resident)."""
    from powergridworld_amd import MultiComponentEnv
    from powergridworld_amd.agents import EnergyStorageEnv, EVChargingEnv, FiveZoneROMThermalEnergyEnv, PVEnv
    comps = [
        {"name": "building", "cls": FiveZoneROMThermalEnergyEnv, "config": {}},
        {"name": "pv", "cls": PVEnv, "config": {"profile_csv": "pv_profile.csv", "scaling_factor": 40.}},
        {"name": "storage", "cls": EnergyStorageEnv, "config": {}},
        {"name": "ev", "cls": EVChargingEnv,
         "config": dict(num_vehicles=100, minutes_per_step=5, max_charge_rate_kw=7.,
                        peak_threshold=250., vehicle_multiplier=5., rescale_spaces=True)},
    ]
    env = MultiComponentEnv(name="mc", components=comps, num_envs=n, device=dev, dtype=dtype)
    gen = torch.Generator(dev).manual_seed(0)
    dims = {"building": 6, "pv": 1, "storage": 1, "ev": 1}
    acts = [{c: torch.empty((n, d), dtype=dtype, device=dev).uniform_(-1, 1, generator=gen)
             for c, d in dims.items()} for _ in range(pool)]
    return env, acts


def bench_c3(dev, steps, warmup, n=16384, pool=16, graph=0, clocked=True, dtype=torch.float64):
    env, acts = c3_env(dev, n, pool, dtype)
    gen = torch.Generator(dev).manual_seed(1)
    init = torch.empty(n, dtype=dtype, device=dev).uniform_(3.0, 50.0, generator=gen)
    k = [0]

    def step():
        _, _, done, _ = env.step(acts[k[0] % pool])
        k[0] += 1
        return done

    reset = lambda: env.reset(init_storage=init)
    if graph:
        # (the episode's 287 steps are not a multiple of `graph`: before a call
        # that would pass the end, the env resets, as done would make it)
        reset()
        gstep = graph_steps(env, acts, graph, reset, clocked)

        def step():
            if env._ep_step + graph > 287:
                reset()
            return gstep()
        steps, warmup = steps // graph, warmup // graph
        if not clocked:
            # every (graph, position) pair is captured on first use: warm up
            # until the pool's graphs have met every position (the pool cycles
            # with period len(graphs) calls, an episode is 287 // graph calls)
            warmup = max(warmup, (pool // graph) * (287 // graph + 1))
    dt = timed_loop(env, step, reset, steps, warmup)
    steps *= max(graph, 1)
    return dict(config="C3" + ("L" if n != 16384 else "") + (("G%d" if clocked else "P%d") % graph if graph else "")
                + ("F" if dtype == torch.float32 else ""),
                workload="MC building+PV+storage+EV(100 vehicles)" + (
                    ", %d-step captured graphs%s" % (graph, "" if clocked else " per episode position")
                    if graph else ""),
                batch=n, agents=1, steps=steps, seconds=dt)


def bench_het(dev, steps, warmup, n=65536, pool=16, fused="auto", conv="opendss", table=True, vrec=True, qrec=True,
              rrows=True, dtype=torch.float64, multi_bus=None, step_kernel=None, start_kernel=None):
    from powergridworld_amd.scenarios.heterogeneous import make_env_config
    from powergridworld_amd.multiagent_env import MultiAgentEnv
    cfg = make_env_config(pf_convergence=conv)
    if multi_bus:                  # one bus per agent; several controllable slots take no response table
        for a, bus in zip(cfg["agents"], MULTI_BUSES):
            a["bus"] = bus
        cfg["pf_config"]["config"]["multi_bus"] = multi_bus
        table = False
    if step_kernel:                # yprim="step": no response table, every env is solved
        cfg["pf_config"]["config"].update(yprim="step", step_kernel=step_kernel)
        table = False
    if start_kernel:               # snap_start="previous": the result depends on history, no table
        cfg["pf_config"]["config"].update(snap_start="previous", start_kernel=start_kernel)
        table = False
    env = MultiAgentEnv(**cfg, num_envs=n, device=dev, fused=fused, dtype=dtype)
    env.pf_solver.od_table = table
    if hasattr(env.pf_solver, "od_node_records"):
        env.pf_solver.od_node_records = vrec
        env.pf_solver.od_row_records = qrec
        env.pf_solver.od_record_rows = rrows
        env.pf_solver._tables_cache.clear()
        env.pf_solver._od_qinfo.clear()
    gen = torch.Generator(dev).manual_seed(0)
    acts = []
    for _ in range(pool):
        acts.append({a.name: ({c.name: torch.empty((n, c.action_space.shape[0]), dtype=dtype,
                                                    device=dev).uniform_(-1, 1, generator=gen)
                               for c in a.envs} if hasattr(a, "envs") else
                              torch.empty((n, a.action_space.shape[0]), dtype=dtype,
                                          device=dev).uniform_(-1, 1, generator=gen))
                     for a in env.agents})
    k = [0]

    def step():
        _, _, dones, _ = env.step(acts[k[0] % pool])
        k[0] += 1
        return dones["__all__"]

    dt = timed_loop(env, step, env.reset, steps, warmup)
    name = ("HET" if fused else "HETG") + ("X" if conv == "exact" else "") + ("" if table else "S") \
        + ("" if vrec else "V") + ("" if qrec else "Q") + ("" if rrows else "R") \
        + ("F" if dtype == torch.float32 else "")
    if multi_bus:
        name = "HETM" + multi_bus[0].upper()
    if step_kernel:
        name = "HETY" + step_kernel[0].upper()
    if start_kernel:
        name = "HETP" + start_kernel[0].upper()
    return dict(config=name,
                workload="3-agent heterogeneous (MC building, grid-aware PV farm, EV 25x40)"
                         + (" on buses %s" % ", ".join(MULTI_BUSES) if multi_bus else "") + " + IEEE-13 PF, "
                         + ("fused multi-agent step (pgw_ma_step%s)" % ("_f32" if dtype == torch.float32 else "")
                            if env._ma is not None else "generic path"),
                pf_convergence=conv, pf_response_table=bool(table and conv == "opendss"),
                pf_kernel="general" if env.pf_solver.general else "fast",
                pf_yprim=getattr(env.pf_solver, "yprim", "dss_file"),
                batch=n, agents=3, steps=steps, seconds=dt)


def bench_c4y(dev, steps, warmup, n=65536, pool=16, fused=True):
    """C4 under yprim="step" on the fast kernel: the generic path (five agents
    stepped one by one, pgw_agent_reduce, pgw_pf_solve_h1, the host's reward
    transform) or the fused step (pgw_coord_step_h1); packed actions on the
    fused path, the same draws as dicts on the generic one."""
    from powergridworld_amd.scenarios.coordinated import CoordinatedMultiBuildingControlEnv, make_c4_config
    cfg = make_c4_config()
    cfg["pf_config"]["config"].update(yprim="step", step_kernel="fast")
    env = CoordinatedMultiBuildingControlEnv(**cfg, num_envs=n, device=dev, fused=fused)
    assert (env._fused is not None) == bool(fused) and env.pf_solver._h1_fast
    gen = torch.Generator(dev).manual_seed(0)
    na, dims = len(env.agents), [c.action_space.shape[0] for c in env.agents[0].envs]
    packed = [torch.empty((na, n, sum(dims)), dtype=torch.float64, device=dev).uniform_(-1, 1, generator=gen)
              for _ in range(pool)]
    if fused:
        acts = packed
    else:
        offs = [sum(dims[:i]) for i in range(len(dims))]
        acts = [{a.name: {c.name: p[ai, :, o:o + d] for c, o, d in zip(a.envs, offs, dims)}
                 for ai, a in enumerate(env.agents)} for p in packed]
    k = [0]

    def step():
        _, _, dones, _ = env.step(acts[k[0] % pool])
        k[0] += 1
        return dones["__all__"]

    dt = timed_loop(env, step, env.reset, steps, warmup)
    return dict(config="C4YF" if fused else "C4YG",
                workload="coordinated 5-building (C4) + IEEE-13 PF under yprim='step', "
                         + ("fused step (%s)" % env._fused["kernel"] if fused else "generic path"),
                pf_kernel="general" if env.pf_solver.general else "fast", pf_yprim=env.pf_solver.yprim,
                batch=n, agents=na, steps=steps, seconds=dt)


def bench_c4p(dev, steps, warmup, n=65536, pool=16, start_kernel="fast"):
    """C4 under snap_start="previous": start_kernel="general" runs the generic
    path on the general kernel (both fused steps refuse the route), "fast" the
    fused step (pgw_coord_step_prev); packed actions on the fused path, the same
    draws as dicts on the generic one."""
    from powergridworld_amd.scenarios.coordinated import CoordinatedMultiBuildingControlEnv, make_c4_config
    cfg = make_c4_config()
    cfg["pf_config"]["config"].update(snap_start="previous", start_kernel=start_kernel)
    env = CoordinatedMultiBuildingControlEnv(**cfg, num_envs=n, device=dev)
    fused = start_kernel == "fast"
    assert (env._fused is not None) == fused and env.pf_solver._prev_fast == fused
    gen = torch.Generator(dev).manual_seed(0)
    na, dims = len(env.agents), [c.action_space.shape[0] for c in env.agents[0].envs]
    packed = [torch.empty((na, n, sum(dims)), dtype=torch.float64, device=dev).uniform_(-1, 1, generator=gen)
              for _ in range(pool)]
    if fused:
        acts = packed
    else:
        offs = [sum(dims[:i]) for i in range(len(dims))]
        acts = [{a.name: {c.name: p[ai, :, o:o + d] for c, o, d in zip(a.envs, offs, dims)}
                 for ai, a in enumerate(env.agents)} for p in packed]
    k = [0]

    def step():
        _, _, dones, _ = env.step(acts[k[0] % pool])
        k[0] += 1
        return dones["__all__"]

    dt = timed_loop(env, step, env.reset, steps, warmup)
    return dict(config="C4PF" if fused else "C4PG",
                workload="coordinated 5-building (C4) + IEEE-13 PF under snap_start='previous', "
                         + ("fused step (%s)" % env._fused["kernel"] if fused else "generic path"),
                pf_kernel="general" if env.pf_solver.general else "fast", pf_snap_start=env.pf_solver.snap_start,
                batch=n, agents=na, steps=steps, seconds=dt)


def bench_hs(dev, steps, warmup, n=65536, pool=16, graph=0, dtype=torch.float64):
    from powergridworld_amd.base_hs import HSMultiComponentEnv
    from powergridworld_amd.scenarios.heterogeneous_hs import make_env_config
    env = HSMultiComponentEnv(**make_env_config(), num_envs=n, device=dev, dtype=dtype)
    gen = torch.Generator(dev).manual_seed(0)
    acts = torch.empty((pool, n, len(env.envs)), dtype=torch.float64, device=dev).uniform_(-1, 1, generator=gen)
    acts = acts.to(dtype)          # (the same draws for both storage dtypes)
    k = [0]

    def step():
        _, _, done, _ = env.step(acts[k[0] % pool])
        k[0] += 1
        return done

    if graph:
        # per-position graphs of `graph` steps over the pool (as C3's); before
        # a call that would pass the data's end the house resets
        env.reset()
        gstep = graph_steps(env, list(acts), graph, env.reset)
        L = env._hs_steps()

        def step():
            if env._hs_step_k() + graph > L:
                env.reset()
            return gstep()
        steps, warmup = steps // graph, max(warmup // graph, (pool // graph) * (L // graph + 1))
    dt = timed_loop(env, step, env.reset, steps, warmup)
    steps *= max(graph, 1)
    f32 = dtype == torch.float32
    return dict(config="HS" + ("32" if f32 else "") + ("P%d" % graph if graph else ""),
                workload="Home-Steward house (PV, battery, EV, devices; shipped JSON scenario)" + (
                    ", fp32 storage (pgw_hs_step_f32)" if f32 else "") + (
                    ", %d-step captured graphs per episode position" % graph if graph else ""),
                batch=n, agents=1, steps=steps, seconds=dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3,HET,HS")
    ap.add_argument("--steps", type=int, default=572)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    fns = {"C2": bench_c2, "C3": bench_c3, "HET": bench_het, "HS": bench_hs,
           "HETG": lambda *a: bench_het(*a, fused=False),
           "HETX": lambda *a: bench_het(*a, conv="exact"),
           "HETS": lambda *a: bench_het(*a, table=False),
           "HETV": lambda *a: bench_het(*a, vrec=False),
           "HETQ": lambda *a: bench_het(*a, qrec=False),
           "HETR": lambda *a: bench_het(*a, rrows=False),
           "HETF": lambda *a: bench_het(*a, dtype=torch.float32),
           "HETMG": lambda *a: bench_het(*a, multi_bus="general"),
           "HETMF": lambda *a: bench_het(*a, multi_bus="fast"),
           "HETYG": lambda *a: bench_het(*a, step_kernel="general"),
           "HETYF": lambda *a: bench_het(*a, step_kernel="fast"),
           "C4YG": lambda *a: bench_c4y(*a, fused=False), "C4YF": lambda *a: bench_c4y(*a, fused=True),
           "HETPG": lambda *a: bench_het(*a, start_kernel="general"),
           "HETPF": lambda *a: bench_het(*a, start_kernel="fast"),
           "C4PG": lambda *a: bench_c4p(*a, start_kernel="general"),
           "C4PF": lambda *a: bench_c4p(*a, start_kernel="fast"),
           "C2G1": lambda *a: bench_c2(*a, graph=1), "C2G8": lambda *a: bench_c2(*a, graph=8),
           "C3G1": lambda *a: bench_c3(*a, graph=1), "C3G8": lambda *a: bench_c3(*a, graph=8),
           "C3P1": lambda *a: bench_c3(*a, graph=1, clocked=False),
           "C3P8": lambda *a: bench_c3(*a, graph=8, clocked=False),
           "C3L": lambda *a: bench_c3(*a, n=65536),
           "C3F": lambda *a: bench_c3(*a, dtype=torch.float32),
           "C3G8F": lambda *a: bench_c3(*a, graph=8, dtype=torch.float32),
           "HSP8": lambda *a: bench_hs(*a, graph=8),
           "HS32": lambda *a: bench_hs(*a, dtype=torch.float32),
           "HS32P8": lambda *a: bench_hs(*a, graph=8, dtype=torch.float32)}
    for name in args.configs.split(","):
        r = fns[name](dev, args.steps, args.warmup)
        units = r["batch"] * r["agents"] * r["steps"]
        r["value"] = units / r["seconds"]
        r["unit"] = "agent-env-steps/s"
        r["us_per_step"] = r["seconds"] / r["steps"] * 1e6
        if name[:2] in BYTES:
            r["step_level_hbm_gbs"] = BYTES[name[:2]] * units / r["seconds"] / 1e9
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
