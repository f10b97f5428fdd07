"""The GPU side of env.reset() inside bench.py's timed region, from a rocprofv3
--kernel-trace CSV (kernel_trace.csv) of a plain `bench.py --steps K --warmup W`
run (a kernel trace only, no counters).

bench.py's step sequence is: first reset, one cold episode, reset, W warmup
steps, K timed steps, with a reset after every step that ends an episode.  The
step kernel is k_coord_step_od; a reset is a gap between two consecutive step
launches that holds a reset kernel (k_building_reset or k_coord_reset).  For
every reset between two TIMED steps this prints
  - the wall gap on the GPU from the end of the episode's last step kernel to
    the start of the next episode's first one,
  - the number of kernels (and copies, when a memory_copy_trace.csv is given
    too) dispatched in that gap,
  - the sum of their durations,
and k_coord_reset's own duration where the gap holds one.  A trace of the
fp32 loop (tools/gpu/ab_reset_f32.py --child, the same step sequence) reads
the same way: the names match k_coord_step_od_f32 and k_coord_reset_f32 too.

usage: python tools/gpu/reset_gap.py kernel_trace.csv [memory_copy_trace.csv]
                                     [--steps 572] [--warmup 30] [--names]
"""
import argparse
import csv
import statistics as st

STEP, RESETS = "k_coord_step_od", ("k_building_reset", "k_coord_reset")


def short(name):
    return name.split("(")[0].replace("void ", "").replace("pgw::", "")[:60]


def load(path, name_key):
    out = []
    for r in csv.DictReader(open(path)):
        out.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get(name_key) or "copy"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kernel_trace")
    ap.add_argument("copy_trace", nargs="?")
    ap.add_argument("--steps", type=int, default=572)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--names", action="store_true", help="list the kernels of each gap by name")
    a = ap.parse_args()

    ev = load(a.kernel_trace, "Kernel_Name")
    if a.copy_trace:
        ev += load(a.copy_trace, "Direction")
    ev.sort()
    steps = [i for i, e in enumerate(ev) if STEP in e[2]]
    if not steps:
        raise SystemExit("no %s launch in the trace" % STEP)

    def is_reset(k):          # the gap after step launch k holds a reset kernel
        return any(any(r in e[2] for r in RESETS) for e in ev[steps[k] + 1:steps[k + 1]])

    cold = next((k + 1 for k in range(len(steps) - 1) if is_reset(k)), None)
    if cold is None:
        raise SystemExit("no reset between two step launches")
    first, last = cold + a.warmup, cold + a.warmup + a.steps - 1
    if last >= len(steps):
        raise SystemExit("the trace holds %d step launches, the timed region needs %d" % (len(steps), last + 1))
    t0, t1 = ev[steps[first]][0], ev[steps[last]][1]
    durs = [(ev[i][1] - ev[i][0]) / 1e3 for i in steps[first:last + 1]]
    print("cold episode %d steps, warmup %d, timed %d: step launches %d..%d" % (cold, a.warmup, a.steps, first, last))
    print("timed region on the GPU: %.1f us = %.3f us per step; step kernel mean %.2f median %.2f us"
          % ((t1 - t0) / 1e3, (t1 - t0) / 1e3 / a.steps, st.mean(durs), st.median(durs)))
    plain = [(ev[steps[k + 1]][0] - ev[steps[k]][1]) / 1e3 for k in range(first, last) if not is_reset(k)]
    if plain:
        print("gap between two steps of one episode: median %.2f us" % st.median(plain))
    print("%-12s %10s %8s %10s %10s %14s" % ("reset after", "gap us", "events", "busy us", "idle us", "k_coord_reset"))
    gaps = []
    for k in range(first, last):
        if not is_reset(k):
            continue
        inside = ev[steps[k] + 1:steps[k + 1]]
        gap = (ev[steps[k + 1]][0] - ev[steps[k]][1]) / 1e3
        busy = sum(e[1] - e[0] for e in inside) / 1e3
        own = [(e[1] - e[0]) / 1e3 for e in inside if "k_coord_reset" in e[2]]
        gaps.append(gap)
        print("%-12s %10.1f %8d %10.1f %10.1f %14s"
              % ("step %d" % k, gap, len(inside), busy, gap - busy, " ".join("%.2f" % d for d in own) or "-"))
        if a.names:
            by = {}
            for e in inside:
                by.setdefault(short(e[2]), []).append((e[1] - e[0]) / 1e3)
            for name, d in sorted(by.items(), key=lambda kv: -sum(kv[1])):
                print("    %4d x %-60s mean %7.2f us  sum %8.1f us" % (len(d), name, st.mean(d), sum(d)))
    if gaps:
        print("resets in the timed region: %d, gap sum %.1f us = %.3f us per timed step"
              % (len(gaps), sum(gaps), sum(gaps) / a.steps))


if __name__ == "__main__":
    main()
