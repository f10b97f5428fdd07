"""Shared inputs and reference of tests/test_cpu_pf_multibus.py and
tests/test_gpu_pf_multibus.py: OpenDSS's snap solve on IEEE-13 with 2 .. 8
controllable loads (OpenDSSSolver(multi_bus="fast"): k_pf_solve_od_ms).  Cases,
seeds, the draw order and the oracle's results (computed once per process and
left unchanged) live here; nothing in this file touches a GPU.

IEEE-13 at rescale 1.2 over the four TIMES of tests/test_gpu_pf_od.py.  Its
twelve constant-PQ loads give m = 14 load phase elements (`671` is one
three-phase delta load: three elements that share a slot).

Draw order of a case (seed s, K envs): rng = default_rng(s); for every time in
TIMES, for every slot in the case's order: P = U(lo, hi) [K], then
Q = U(-0.3, 0.5) [K] * |P|.  A smaller batch takes the first envs of the K = 321
draw, so every batch shares one reference.
"""
import functools

import numpy as np
import pandas as pd

IEEE13 = "ieee_13_dss/IEEE13Nodeckt.dss"
SHAPE = "ieee_13_dss/annual_hourly_load_profile.csv"
RESCALE = 1.2
TIMES = [pd.Timestamp("08-12-2021 %02d:10:00" % h) for h in (3, 11, 17, 20)]
NAMES = ("671", "634a", "634b", "634c", "645", "675a", "675b", "675c", "670a", "670b", "670c", "684c")
M = 14
K = 321                          # one block of 256, one full wave and one lane
K_SMALL = (1, 65)                # case A also at these
TOL, VLOW, VMIN, VMAX = 1e-4, 0.5, 0.95, 1.05

# slots, kW range, max_iter (None: OpenDSS's 15, the solver's default), seed
CASES = {
    "A": dict(slots=("675a", "675c"), lo=-400.0, hi=900.0, max_iter=None, seed=11),
    "B": dict(slots=("671", "675c", "684c"), lo=-400.0, hi=900.0, max_iter=None, seed=12),
    "C": dict(slots=NAMES[:8], lo=-300.0, hi=600.0, max_iter=None, seed=13),
    "D": dict(slots=NAMES[:8], lo=-1500.0, hi=3000.0, max_iter=6, seed=14),
}


def max_iter_of(case):
    return CASES[case]["max_iter"] or 15


@functools.lru_cache(maxsize=None)
def loads(case):
    """Per time of TIMES: (P [C, K] kW, Q [C, K] kvar), slot-major in the
    case's slot order (read-only)."""
    c = CASES[case]
    rng = np.random.default_rng(c["seed"])
    out = []
    for _ in TIMES:
        P, Q = [], []
        for _ in c["slots"]:
            p = rng.uniform(c["lo"], c["hi"], K)
            q = rng.uniform(-0.3, 0.5, K) * np.abs(p)
            P.append(p)
            Q.append(q)
        P, Q = np.stack(P), np.stack(Q)
        P.setflags(write=False)
        Q.setflags(write=False)
        out.append((P, Q))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pf():
    from oracle.pf_oracle import BatchedPF
    return BatchedPF(system_load_rescale_factor=RESCALE, semantics="opendss")


def feeder():
    return pf().feeder


def oracle_solve(t, slots, P, Q, max_iter=15, trace=None):
    """The oracle's snap solve at time t with slot powers P, Q [C, K]: (V [K,
    nodes] complex volts, iterations [K], last_converged [K])."""
    o = pf()
    f = o.feeder
    n = np.asarray(P).shape[1]
    kw, kvar = o.loads(t, {nm: P[s] for s, nm in enumerate(slots)}, {nm: Q[s] for s, nm in enumerate(slots)}, K=n)
    V, it = f.snap_opendss(kw, kvar, f.base_kw, f.base_kvar, max_iter=max_iter, trace=trace)
    return V, it.copy(), f.last_converged.copy()


def elem_pu(V):
    """Element voltages u = C V / vb [K, m] complex of node voltages V."""
    f = feeder()
    return (V @ f.Cinc.T) / f.elem_vbase


@functools.lru_cache(maxsize=None)
def oracle(case):
    """Per time of TIMES a dict of the oracle's snap solve of the case (read
    only): V, pu [K, nodes], it, conv [K], u_last [K, m] (the stopped iterate's
    element voltages, pu), and what the conditions of test_cpu_pf_multibus.py
    read --
      err    [k_max + 1, K]: iteration k's tested quantity, the largest change
             of any node's magnitude (pu), NaN where the env no longer iterates
             (and for k < 1);
      umag   [k_max + 1, K, m]: |u| (pu) at which iteration k evaluates the load
             law -- the element voltages of the iterate before it, the direct
             solution for k = 1 --, NaN where the env no longer iterates."""
    c = CASES[case]
    cap = max_iter_of(case)
    f = feeder()
    out = []
    for t, (P, Q) in zip(TIMES, loads(case)):
        trace = []
        V, it, conv = oracle_solve(t, c["slots"], P, Q, cap, trace)
        kmax = int(it.max())
        err = np.full((kmax + 1, K), np.nan)
        umag = np.full((kmax + 1, K, M), np.nan)
        for k in range(1, kmax + 1):
            on = it >= k                                     # the envs that run iteration k
            err[k, on] = trace[k - 1].max(1)[on]
            # the iterate before iteration k: the solve stopped after k - 1
            # iterations (envs that stopped earlier keep theirs and are masked)
            Vp, _, _ = oracle_solve(t, c["slots"], P, Q, k - 1)
            umag[k, on] = np.abs(elem_pu(Vp))[on]
        d = dict(V=V, pu=f.pu(V), it=it, conv=conv, u_last=elem_pu(V), err=err, umag=umag)
        for a in d.values():
            a.setflags(write=False)
        out.append(d)
    return tuple(out)


def signed_iterations(ref):
    """The kernels' count: -iterations where the cap stopped the env."""
    return np.where(ref["conv"], ref["it"], -ref["it"])


# ---------------------------------------------------------------- the start table's inputs
@functools.lru_cache(maxsize=None)
def reduced():
    """The snap iteration's element-space operands from the oracle's feeder,
    in pu of the element bases: W'' [m, m] (of Y + the DSS file's load Yeq), u0
    [m] (the direct solution), y0 [m] (the Yeq powers per phase, W - j var)."""
    from oracle.pf_oracle import _accurate_inverse
    f = feeder()
    C, vb = f.Cinc, f.elem_vbase
    ykw = f.base_kw[f.elem_load] * 1000.0 / f.elem_nph
    ykv = f.base_kvar[f.elem_load] * 1000.0 / f.elem_nph
    y0 = ykw - 1j * ykv
    Z1 = _accurate_inverse(f.Y + C.T @ np.diag(y0 / (vb * vb)) @ C)
    W2 = (-C @ Z1 @ C.T) / (vb[:, None] * vb[None, :])
    u0 = (C @ (Z1 @ f.I_src)) / vb
    return W2, u0, y0


def start_u1(table, P, Q):
    """u_1 [K, m] complex (pu) of a start table (pgw_pf_od.start, include/pgw.h)
    for slot powers P, Q [C, K] (kW, kvar): u1b + sum_s (P_s u1P_s + Q_s u1Q_s),
    read at the header's offsets -- slot 0's maps at m and 2 m (complex), slot
    s >= 1's at 6 m + 4 m (s - 1) and one m further."""
    t = np.asarray(table).view(np.complex128)
    P, Q = np.atleast_2d(P), np.atleast_2d(Q)
    u = np.tile(t[:M], (P.shape[1], 1))
    for s in range(P.shape[0]):
        b = M if s == 0 else 6 * M + (s - 1) * 4 * M
        u = u + P[s][:, None] * t[b:b + M] + Q[s][:, None] * t[b + M:b + 2 * M]
    return u


def elem_ctrl(slots):
    """Slot of every element (-1: not controllable)."""
    f = feeder()
    names = [f.load_names[li] for li in f.elem_load]
    return np.array([slots.index(nm) if nm in slots else -1 for nm in names])


def elem_base(t):
    """The hour's base loads per element (kW, kvar of the whole load)."""
    o = pf()
    kw, kvar = o.base_loads(t)
    return kw[o.feeder.elem_load], kvar[o.feeder.elem_load]
