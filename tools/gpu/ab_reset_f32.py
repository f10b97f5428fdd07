"""Same-box A/B of env.reset() on the fp32-storage C4 env: the parent commit's
tree against this one, every run a process of its own, the two alternated.

The workload is bench.py's episode loop on MultiAgentEnv(dtype=torch.float32)
at 65 536 envs: first reset, one cold episode, reset, W warmup steps, then K
timed steps (572 = two episodes, so the region holds two resets), host clock
around the synchronised region.

  python tools/gpu/ab_reset_f32.py --child [--tree DIR] [--steps 572] [--warmup 30] [--batch 65536]
      one measurement in this process of the package under DIR (default: this
      repository); prints one JSON line.  Also the program to put after
      `rocprofv3 --kernel-trace --output-format csv -d OUT --` (a trace of its
      own, no counters); tools/gpu/reset_gap.py reads the CSV.
  python tools/gpu/ab_reset_f32.py --parent-tree DIR [--pairs 5] [--bench-pairs 3] [--limit 240]
      `--pairs` alternated pairs of --child runs (parent/new, new/parent, ...),
      then `--bench-pairs` alternated pairs of `python bench.py` (the fp64
      headline, each in its own tree).  Every GPU run is a child under its own
      `timeout -k 10 LIMIT`; the script stops at the first non-zero exit status
      and returns it.  DIR holds the parent commit's powergridworld_amd/ (with
      its built libpgw.so), include/, oracle/ and bench.py.
"""
import argparse
import gc
import json
import os
import statistics as st
import subprocess
import sys
import time

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))


def child(a):
    tree = os.path.abspath(a.tree or ROOT)
    sys.path.insert(0, tree)
    import torch
    import powergridworld_amd
    from powergridworld_amd.scenarios.coordinated import CoordinatedMultiBuildingControlEnv, make_c4_config
    assert os.path.dirname(os.path.dirname(os.path.abspath(powergridworld_amd.__file__))) == tree, \
        "powergridworld_amd was not imported from %s" % tree
    dev = torch.device("cuda", 0)
    n, P = a.batch, 64
    env = CoordinatedMultiBuildingControlEnv(**make_c4_config(), num_envs=n, device=dev, dtype=torch.float32)
    assert env._fused is not None and env._fused["kernel"] == "pgw_coord_step_f32"
    for i, agent in enumerate(env.agents):
        agent.env_dict["storage"].seed(i)
    gen = torch.Generator(dev).manual_seed(0)
    pool = torch.empty((P, 5, 8, n), dtype=torch.float32, device=dev)
    pool.uniform_(-1.0, 1.0, generator=gen)
    packed = pool.transpose(2, 3)
    k, host, resets = [0], [], []

    def run(m):
        for _ in range(m):
            h0 = time.perf_counter()
            _, _, dones, _ = env.step(packed[k[0] % P])
            k[0] += 1
            if dones["__all__"]:
                env.reset()
                resets.append(len(host))
            host.append(time.perf_counter() - h0)

    env.reset()
    while not resets:                  # the cold episode and the reset that ends it
        run(1)
    cold = k[0]
    gc.collect()
    gc.freeze()
    run(a.warmup)
    torch.cuda.synchronize()
    del host[:], resets[:]
    t0 = time.perf_counter()
    run(a.steps)
    t_issued = time.perf_counter()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    srt = sorted(host)
    print(json.dumps({"tree": tree, "us_per_step": dt / a.steps * 1e6, "steps": a.steps, "warmup": a.warmup,
                      "batch": n, "cold_episode_steps": cold, "resets_in_region": len(resets),
                      "reset_step_host_us": [host[i] * 1e6 for i in resets],
                      "host_step_median_us": srt[len(srt) // 2] * 1e6,
                      "issue_us": (t_issued - t0) * 1e6,
                      "fused_resets": getattr(env, "fused_resets", None)}), flush=True)


def gpu_run(cmd, cwd, limit):
    """One GPU process under its own time limit; the last JSON line it printed.
    The script ends with the child's status if that is not 0."""
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=cwd, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    if r.returncode != 0:
        sys.stderr.write(r.stderr.decode(errors="replace")[-4000:])
        print("stopped: exit status %d of %s in %s" % (r.returncode, " ".join(cmd), cwd), flush=True)
        sys.exit(r.returncode)
    lines = [x for x in r.stdout.decode().splitlines() if x.startswith("{")]
    return json.loads(lines[-1])


def pairs(label, count, parent_run, new_run, fmt):
    par, new = [], []
    for i in range(count):
        order = ("parent", "new") if i % 2 == 0 else ("new", "parent")
        res = {}
        for which in order:
            res[which] = (parent_run if which == "parent" else new_run)()
        par.append(res["parent"])
        new.append(res["new"])
        print("%s pair %d  %-11s  parent %s  new %s  parent - new %.2f"
              % (label, i + 1, "/".join(order), fmt(res["parent"]), fmt(res["new"]),
                 res["parent"]["us"] - res["new"]["us"]), flush=True)
    p, q = [x["us"] for x in par], [x["us"] for x in new]
    diff = [x - y for x, y in zip(p, q)]
    print("%s: parent %.2f-%.2f  new %.2f-%.2f us per step; new lower in %d of %d pairs; median difference %.2f us; "
          "the parent's own spread %.2f us; ranges overlap: %s"
          % (label, min(p), max(p), min(q), max(q), sum(d > 0 for d in diff), count, st.median(diff),
             max(p) - min(p), max(min(p), min(q)) <= min(max(p), max(q))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree")
    ap.add_argument("--parent-tree")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--bench-pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=572)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--limit", type=int, default=240, help="time limit of each GPU run, seconds")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_tree:
        ap.error("--child or --parent-tree DIR")
    parent = os.path.abspath(a.parent_tree)
    shape = ["--steps", str(a.steps), "--warmup", str(a.warmup), "--batch", str(a.batch)]

    def f32(tree):
        def go():
            r = gpu_run([sys.executable, HERE, "--child", "--tree", tree] + shape, tree, a.limit)
            r["us"] = r["us_per_step"]
            return r
        return go

    def bench(tree):
        def go():
            r = gpu_run([sys.executable, "bench.py", "--gpus", "1"] + shape, tree, a.limit)
            r["us"] = r["ms_per_step"] * 1e3
            return r
        return go

    if a.pairs:
        print("fp32 C4 env, %d envs, --steps %d --warmup %d, us per step" % (a.batch, a.steps, a.warmup), flush=True)
        pairs("f32", a.pairs, f32(parent), f32(ROOT),
              lambda r: "%.2f (reset steps' host %s us, fused resets %s)"
              % (r["us"], "/".join("%.0f" % x for x in r["reset_step_host_us"]), r["fused_resets"]))
    if a.bench_pairs:
        print("fp64 headline, python bench.py --gpus 1 with the same shape, us per step", flush=True)
        pairs("bench.py", a.bench_pairs, bench(parent), bench(ROOT), lambda r: "%.2f" % r["us"])


if __name__ == "__main__":
    main()
