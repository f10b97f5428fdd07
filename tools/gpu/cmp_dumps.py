"""Compare two `bench.py --dump-outputs DIR` folders array by array, bit for bit.
usage: python tools/gpu/cmp_dumps.py DIR_A DIR_B      (exit status 1 on any difference)"""
import os
import sys

import numpy as np

a, b = sys.argv[1:3]
names = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
other = sorted(f for f in os.listdir(b) if f.endswith(".npy"))
bad = names != other
if bad:
    print("different array sets:", sorted(set(names) ^ set(other)))
for f in names:
    if f not in other:
        continue
    x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
    same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
    print("%-28s %-18s %s" % (f, x.shape, "bit-equal" if same else "DIFFERENT"))
    bad = bad or not same
print("all arrays bit-equal" if not bad else "NOT equal")
sys.exit(1 if bad else 0)
