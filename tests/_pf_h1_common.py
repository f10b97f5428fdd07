"""Shared inputs and reference of tests/test_cpu_pf_h1.py and
tests/test_gpu_pf_h1.py: OpenDSS's snap solve in the reading where every
solve's Y holds its own loads' Yeq (OpenDSSSolver(yprim="step"), H1) on the fast
one-lane-per-env kernel (step_kernel="fast": pgw_pf_solve_h1).  Cases, seeds,
the draw order and the oracle's results (computed once per process and left
unchanged) live here; nothing in this file touches a GPU.

IEEE-13 at rescale 1.2 over the four TIMES of tests/test_gpu_pf_od.py; one
controllable load of one phase element.  Draw order of a case (seed s): rng =
default_rng(s); for every time in TIMES: P = U(lo, hi) [K], then Q = U(-0.3,
0.5) [K] * |P|.  A smaller batch takes the first envs of the K = 321 draw, so
every batch shares one reference.

  R   684c, the range of test_opendss_yprim_step_vs_oracle: a second element index
  S   675c, a range where the stopping rule decides between 2, 3 and 4 iterations
  T   675c, a wider one: 2 .. 6 iterations and one env per time at the cap of 15
  T3  case T's draw under max_iter = 3: tens of envs stopped by the cap
"""
import functools

import numpy as np

from tests._pf_multibus_common import IEEE13, SHAPE, RESCALE, TIMES, M, TOL, VLOW, VMIN, VMAX, pf, feeder, elem_pu  # noqa: F401

K = 321                          # one block of 256, one full wave and one lane
BATCHES = (1, 65, 321)

CASES = {
    "R": dict(load="684c", lo=-400.0, hi=900.0, max_iter=None, seed=22),
    "S": dict(load="675c", lo=-1500.0, hi=3000.0, max_iter=None, seed=24),
    "T": dict(load="675c", lo=-3000.0, hi=6000.0, max_iter=None, seed=26),
    "T3": dict(load="675c", lo=-3000.0, hi=6000.0, max_iter=3, seed=26),
}


def max_iter_of(case):
    return CASES[case]["max_iter"] or 15


@functools.lru_cache(maxsize=None)
def loads(case):
    """Per time of TIMES: (P [K] kW, Q [K] kvar) of the case's load (read-only)."""
    c = CASES[case]
    rng = np.random.default_rng(c["seed"])
    out = []
    for _ in TIMES:
        p = rng.uniform(c["lo"], c["hi"], K)
        q = rng.uniform(-0.3, 0.5, K) * np.abs(p)
        p.setflags(write=False)
        q.setflags(write=False)
        out.append((p, q))
    return tuple(out)


def oracle_solve(t, load, P, Q, max_iter=15, trace=None):
    """The oracle's H1 snap solve (yprim_kw = None: every env's own Yeq in Y) at
    time t with the load's powers P, Q [K] (None: no controllable load, one
    env): (V [K, nodes] complex volts, iterations [K], last_converged [K])."""
    o = pf()
    f = o.feeder
    if P is None:
        kw, kvar = o.loads(t, K=1)
    else:
        kw, kvar = o.loads(t, {load: np.asarray(P)}, {load: np.asarray(Q)}, K=len(P))
    V, it = f.snap_opendss(kw, kvar, max_iter=max_iter, trace=trace)
    return V, it.copy(), f.last_converged.copy()


@functools.lru_cache(maxsize=None)
def oracle(case):
    """Per time of TIMES a dict of the oracle's solve of the case (read only):
    V, pu [K, nodes], it, conv [K], and err [k_max + 1, K]: iteration k's tested
    quantity, the largest change of any node's magnitude (pu), NaN where the env
    no longer iterates (and for k < 1)."""
    c = CASES[case]
    cap = max_iter_of(case)
    f = feeder()
    out = []
    for t, (P, Q) in zip(TIMES, loads(case)):
        trace = []
        V, it, conv = oracle_solve(t, c["load"], P, Q, cap, trace)
        kmax = int(it.max())
        err = np.full((kmax + 1, K), np.nan)
        for k in range(1, kmax + 1):
            on = it >= k                                     # the envs that run iteration k
            err[k, on] = trace[k - 1].max(1)[on]
        d = dict(V=V, pu=f.pu(V), it=it, conv=conv, err=err)
        for a in d.values():
            a.setflags(write=False)
        out.append(d)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_umag(case):
    """Per time of TIMES, umag [k_max + 1, K, m]: |u| (pu) at which iteration k
    evaluates the load law -- the element voltages of the iterate before it, the
    direct solution at the env's own Y for k = 1 --, NaN where the env no
    longer iterates.  (The oracle keeps no iterates: iteration k's input is its
    solve stopped after k - 1 iterations, of the envs that run iteration k.)"""
    c = CASES[case]
    out = []
    for t, (P, Q), ref in zip(TIMES, loads(case), oracle(case)):
        it = ref["it"]
        kmax = int(it.max())
        umag = np.full((kmax + 1, K, M), np.nan)
        for k in range(1, kmax + 1):
            on = it >= k
            Vp, _, _ = oracle_solve(t, c["load"], P[on], Q[on], k - 1)
            umag[k, on] = np.abs(elem_pu(Vp))
        umag.setflags(write=False)
        out.append(umag)
    return tuple(out)


def signed_iterations(ref):
    """The kernels' count: -iterations where the cap stopped the env."""
    return np.where(ref["conv"], ref["it"], -ref["it"])


@functools.lru_cache(maxsize=None)
def oracle_base():
    """Per time: (pu [nodes], signed iterations) of the solve with no
    controllable load."""
    f = feeder()
    out = []
    for t in TIMES:
        V, it, conv = oracle_solve(t, None, None, None)
        out.append((f.pu(V)[0], int(np.where(conv, it, -it)[0])))
    return tuple(out)


# P = 0 and Q = 0 envs (on 675c): both zero, Q alone, P alone
EDGE_P = np.array([0.0, 700.0, 0.0, -350.0])
EDGE_Q = np.array([0.0, 0.0, 120.0, 0.0])


@functools.lru_cache(maxsize=None)
def oracle_edge():
    """Per time: (pu [4, nodes], signed iterations [4]) at EDGE_P / EDGE_Q."""
    f = feeder()
    out = []
    for t in TIMES:
        V, it, conv = oracle_solve(t, "675c", EDGE_P, EDGE_Q)
        out.append((f.pu(V), np.where(conv, it, -it)))
    return tuple(out)


# ---------------------------------------------------------------- the hour tables' inputs
@functools.lru_cache(maxsize=None)
def file_model():
    """The file model's operands from the oracle's feeder, in pu (element bases
    for u and the scaled currents, node bases for the rows): W'' [m, m], u0 [m],
    y0 [m] (the DSS file's Yeq powers per phase, W - j var), and every node's
    row G [n, m], V0 [n] (V = V0 + G J')."""
    from oracle.pf_oracle import _accurate_inverse
    f = feeder()
    C, vb = f.Cinc, f.elem_vbase
    vbn = f.kv_ln * 1000.0
    y0 = f.base_kw[f.elem_load] * 1000.0 / f.elem_nph - 1j * (f.base_kvar[f.elem_load] * 1000.0 / f.elem_nph)
    Z1 = _accurate_inverse(f.Y + C.T @ np.diag(y0 / (vb * vb)) @ C)
    W2 = (-C @ Z1 @ C.T) / (vb[:, None] * vb[None, :])
    u0 = (C @ (Z1 @ f.I_src)) / vb
    G = (-(Z1 @ C.T) / vb[None, :]) / vbn[:, None]
    V0 = (Z1 @ f.I_src) / vbn
    return W2, u0, y0, G, V0


def elem_of(load):
    """The one load phase element of `load`."""
    f = feeder()
    k = [i for i, li in enumerate(f.elem_load) if f.load_names[li] == load]
    assert len(k) == 1, (load, k)
    return k[0]


def elem_base(t):
    """The hour's base loads per element (kW, kvar of the whole load)."""
    o = pf()
    kw, kvar = o.base_loads(t)
    return kw[o.feeder.elem_load], kvar[o.feeder.elem_load]
