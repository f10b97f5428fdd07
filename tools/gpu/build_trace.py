"""Launch count and GPU-busy time of the first reset's table build, from a
rocprofv3 --kernel-trace CSV of a plain bench run.  The build window runs from
the first k_pf_od_probe launch to the last launch before the first step
kernel; the certificate's part of it is what follows the last probe (the fit
check's) -- torch launches on the Python path, k_pf_od_certify on the native.
Usage: python tools/gpu/build_trace.py <kernel_trace.csv>"""
import csv
import sys


def main(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    step = next((i for i, r in enumerate(rows) if "k_coord_step" in r[2]), len(rows))
    first = rows[:step]
    probes = [i for i, r in enumerate(first) if "k_pf_od_probe" in r[2]]
    if not probes:
        print("no k_pf_od_probe launch before the first step")
        return
    build = first[probes[0]:]
    # the certificate follows the last probe that is itself followed by the
    # fit/check kernels: the probe launches after it belong to the first reset's tail
    fits = [i for i, r in enumerate(first) if "k_pf_od_resp_check" in r[2]]
    c0 = fits[-1] + 1 if fits else probes[-1] + 1
    cert = first[c0:]

    def show(name, part):
        if not part:
            print("%s: no launches" % name)
            return
        busy = sum(e - s for s, e, _ in part)
        wall = part[-1][1] - part[0][0]
        print("%s: %d launches, kernel time %.3f ms, first to last %.3f ms (GPU busy %.1f %%)"
              % (name, len(part), busy / 1e6, wall / 1e6, 100.0 * busy / max(wall, 1)))

    show("before the first step", first)
    show("table build (first probe .. first step)", build)
    show("after the last fit check (certificate, row masks, reset tail)", cert)
    n_cert = sum(1 for r in cert if "k_pf_od_certify" in r[2])
    print("k_pf_od_certify launches: %d" % n_cert)
    names = {}
    for s, e, n in cert:
        k = n.split("(")[0][:90]
        c = names.setdefault(k, [0, 0])
        c[0] += 1
        c[1] += e - s
    for k, (c, t) in sorted(names.items(), key=lambda kv: -kv[1][0])[:12]:
        print("  %6d  %9.3f ms  %s" % (c, t / 1e6, k))


if __name__ == "__main__":
    main(sys.argv[1])
