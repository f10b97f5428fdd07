"""Same-box A/B of OpenDSSSolver(snap_start="previous", start_kernel="general" |
"fast") at 65,536 envs, one process, the two alternated in every round:
  * the stand-alone power flow on 675c with every node written, chained over a
    pool of 8 load draws (a repeated draw would take 2 iterations in every env:
    the chain starts where it stopped), `reps` solves between two device
    events, after a check that both routes give equal iteration counts and
    voltages within 1e-11 rel over the same chain;
  * the heterogeneous scenario's step (tools/bench_configs.py HETPG / HETPF: the
    generic agents and the general kernel against the fused multi-agent step
    and pgw_pf_solve_prev), host clock around synchronised regions;
  * the C4 scenario's step (C4PG / C4PF: the generic path on the general kernel,
    the only route start_kernel="general" has, against the fused
    pgw_coord_step_prev), with the iteration histogram the chained start takes
    on the C4 loads beside the direct start's.
Usage: python tools/gpu/ab_prev.py [rounds] [reps] [steps]
       python tools/gpu/ab_prev.py --trace [steps]
           the program for `rocprofv3 --kernel-trace --stats -- python ...`:
           `steps` fused C4 steps, each followed by the stand-alone
           pgw_pf_solve_prev on the same bus loads from a copy of the step's
           start, so the trace holds k_coord_agents_std, k_coord_pf_od_prev and
           k_pf_solve_od_prev side by side."""
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

TOOLS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(TOOLS))      # the repository root: powergridworld_amd
from powergridworld_amd import _lib   # noqa: E402
from powergridworld_amd.distribution_system.opendss import OpenDSSSolver   # noqa: E402
from powergridworld_amd.multiagent_env import MultiAgentEnv   # noqa: E402
from powergridworld_amd.scenarios.coordinated import CoordinatedMultiBuildingControlEnv, make_c4_config   # noqa: E402
from powergridworld_amd.scenarios.heterogeneous import make_env_config   # noqa: E402

dev = torch.device("cuda", 0)
n, pool = 65536, 16
trace = len(sys.argv) > 1 and sys.argv[1] == "--trace"
args = sys.argv[2:] if trace else sys.argv[1:]
MODES = ("general", "fast")


def make_c4(mode, **pf):
    cfg = make_c4_config()
    cfg["pf_config"]["config"].update(dict(snap_start="previous", start_kernel=mode), **pf)
    env = CoordinatedMultiBuildingControlEnv(**cfg, num_envs=n, device=dev)
    assert env.pf_solver.general == (mode == "general") and (env._fused is not None) == (mode == "fast")
    return env


gen = torch.Generator(dev).manual_seed(0)
packed = [torch.empty((5, n, 8), dtype=torch.float64, device=dev).uniform_(-1, 1, generator=gen) for _ in range(pool)]

if trace:
    steps = int(args[0]) if args else 100
    env = make_c4("fast")
    F, solver = env._fused, env.pf_solver
    assert F["kernel"] == "pgw_coord_step_prev" and solver.params.n_out == 1
    v = torch.zeros((1, n), dtype=torch.float64, device=dev)
    it = torch.zeros(n, dtype=torch.int32, device=dev)
    U = torch.zeros_like(solver._prev_U)
    env.reset()
    same = True
    for k in range(steps):
        U.copy_(solver._prev_U)
        env.step(packed[k % pool])
        P = torch.zeros(n, dtype=torch.float64, device=dev)
        for ai in range(len(env.agents)):
            P = P + F["agent_power"][ai]
        pfp, pft = solver.step_params(env.time), solver.step_tables(env.time)
        _lib.check(_lib.lib().pgw_pf_solve_prev(pfp, pft, U.data_ptr(), n, _lib.dptr(P), None, _lib.dptr(v),
                                                _lib.dptr(it), _lib.stream_ptr(dev)))
        same = same and bool(torch.equal(v[0], F["v_out"][0])) and bool(torch.equal(it, F["iters"])) \
            and bool(torch.equal(U, solver._prev_U))
    torch.cuda.synchronize()
    print("trace: %d fused steps + stand-alone solves, outputs equal %s, iteration histogram %s"
          % (steps, same, torch.bincount(it.clamp(min=0)).tolist()), flush=True)
    sys.exit(0 if same else 1)

rounds = int(args[0]) if args else 4
reps = int(args[1]) if len(args) > 1 else 200
steps = int(args[2]) if len(args) > 2 else 286
T = pd.Timestamp("08-12-2021 11:10:00")

# ---------------------------------------------------------------- stand-alone power flow, every node
rng = np.random.default_rng(1)
draws = []
for _ in range(8):
    P = rng.uniform(-400.0, 900.0, n)
    draws.append(({"675c": torch.tensor(P, device=dev)},
                  {"675c": torch.tensor(rng.uniform(-0.3, 0.5, n) * np.abs(P), device=dev)}))
runs = {}
for mode in MODES:
    s = OpenDSSSolver("ieee_13_dss/IEEE13Nodeckt.dss", "ieee_13_dss/annual_hourly_load_profile.csv", device=dev,
                      system_load_rescale_factor=1.2, convergence="opendss", num_envs=n, snap_start="previous",
                      start_kernel=mode)
    s.set_controllable_loads(["675c"])
    assert s.general == (mode == "general") and s._prev_fast == (mode == "fast")
    assert len(s.output_names) == s.feeder.n
    k = [0]

    def call(s=s, k=k):
        p, q = draws[k[0] % len(draws)]
        k[0] += 1
        s.calculate_power_flow(p, q, current_time=T)
    hist = torch.zeros(16, dtype=torch.long, device=dev)
    for _ in range(24):
        call()
        hist += torch.bincount(s.iterations.clamp(min=0), minlength=16)[:16]
    torch.cuda.synchronize()
    runs[mode] = (s, call, hist)
vg, vf = runs["general"][0].v_out, runs["fast"][0].v_out
ig, if_ = runs["general"][0].iterations, runs["fast"][0].iterations
print("PF: after 24 chained solves iterations equal %s, fast vs general %.3e rel, iteration histogram of the 24 "
      "solves %s (general %s)" % (bool(torch.equal(ig, if_)), ((vf - vg).abs() / vg.abs()).max().item(),
                                  runs["fast"][2].tolist(), runs["general"][2].tolist()), flush=True)
for r in range(rounds):
    out = []
    for mode in MODES:
        call = runs[mode][1]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    print("PF round %d: general %.2f us/solve  fast %.2f us/solve  ratio %.3f" % (r, out[0], out[1], out[0] / out[1]),
          flush=True)
del runs


# ---------------------------------------------------------------- env steps
def actions(env, count=8):
    g = torch.Generator(dev).manual_seed(0)
    draw = lambda d: torch.empty((n, d), dtype=torch.float64, device=dev).uniform_(-1, 1, generator=g)
    return [{ag.name: ({c.name: draw(c.action_space.shape[0]) for c in ag.envs} if hasattr(ag, "envs")
                       else draw(ag.action_space.shape[0])) for ag in env.agents} for _ in range(count)]


def ab(label, envs, acts, m):
    ks = [0, 0]
    hist = [torch.zeros(17, dtype=torch.long, device=dev) for _ in envs]

    def run(i, count, tally=False):
        e = envs[i]
        for _ in range(count):
            _, _, d, _ = e.step(acts[i][ks[i] % len(acts[i])])
            ks[i] += 1
            if tally:          # (counts by magnitude; slot 16: envs the cap stopped)
                it = e.pf_solver.iterations
                hist[i] += torch.bincount(torch.where(it < 0, torch.full_like(it, 16), it), minlength=17)[:17]
            if d["__all__"]:
                e.reset()
    # per-env counts over the first 16 steps from reset (two env instances share
    # their agents' trajectories only that long: the components' own random
    # draws differ between instances later in the episode), then each route's
    # histogram over the first 100 steps
    for i in range(2):
        envs[i].reset()
    same = bool(torch.equal(envs[0].pf_solver.iterations, envs[1].pf_solver.iterations))
    for _ in range(16):
        for i in range(2):
            run(i, 1, tally=True)
        same = same and bool(torch.equal(envs[0].pf_solver.iterations, envs[1].pf_solver.iterations))
    for i in range(2):
        run(i, min(m, 100) - 16, tally=True)
    torch.cuda.synchronize()
    print("%s: iterations equal in every env over the first 16 steps %s; histogram of the first %d steps general %s "
          "fast %s" % (label, same, min(m, 100), hist[0].tolist(), hist[1].tolist()), flush=True)
    for r in range(rounds):
        out = []
        for i in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(i, m)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / m * 1e6)
        print("%s round %d: general %.2f us/step  fast %.2f us/step  ratio %.3f"
              % (label, r, out[0], out[1], out[0] / out[1]), flush=True)


envs = []
for mode in MODES:
    cfg = make_env_config()
    cfg["pf_config"]["config"].update(snap_start="previous", start_kernel=mode)
    envs.append(MultiAgentEnv(**cfg, num_envs=n, device=dev))
    assert envs[-1].pf_solver.general == (mode == "general") and (envs[-1]._ma is not None) == (mode == "fast")
a = actions(envs[0])
ab("HET step", envs, [a, a], steps)
del envs, a

envs = [make_c4(mode) for mode in MODES]
offs = ((0, 6), (6, 7), (7, 8))
dicts = [{ag.name: {c.name: p[ai, :, lo:hi] for c, (lo, hi) in zip(ag.envs, offs)}
          for ai, ag in enumerate(envs[0].agents)} for p in packed]
print("C4 fused kernel:", envs[1]._fused["kernel"], flush=True)
ab("C4 step", envs, [dicts, packed], steps)
del envs

# what the reading costs or saves: the direct start's counts on the same C4 loads
cfg = make_c4_config()
cfg["pf_config"]["config"].update(od_table=False)
d = CoordinatedMultiBuildingControlEnv(**cfg, num_envs=n, device=dev)
d.reset()
hist = torch.zeros(17, dtype=torch.long, device=dev)
for k in range(100):
    _, _, done, _ = d.step(packed[k % pool])
    it = d.pf_solver.iterations
    hist += torch.bincount(torch.where(it < 0, torch.full_like(it, 16), it), minlength=17)[:17]
    if done["__all__"]:
        d.reset()
torch.cuda.synchronize()
print("C4 step, snap_start='direct' (no table): iteration histogram of the first 100 steps %s" % hist.tolist(),
      flush=True)
