"""Shared by tests/test_gpu_reg_kernels.py, tests/test_cpu_regloop_ref.py and
tests/test_gpu_pf_regloop_direct.py: the synthetic RegControl models, the
extended-precision factor K(t) = (I + D S)^-1 D, and -- for
pgw_pf_solve_regulated (include/pgw.h, "The snap solve with controls in one
launch") -- synthetic regulated problems with an np.longdouble restatement of
the whole loop: solve, sample the controls, execute the nearest actions,
re-factor, repeat.  Nothing here needs a GPU unless a device is asked for.

A case is a _pfg_direct_common.Problem (m elements, n_reg correction columns,
r_reg regulator nodes) plus a pgw_reg_params over the same r_reg:
_synthetic_model(r_reg)'s regulated phases and S, rho from the Problem, and
control records tuned to the problem (`Case._controls`).  In this synthetic
setting the node voltages at R are V = rho x - S c = (I + S D(t))^-1 (rho x)
with |S D| of order 10 per tap step, so a monitored |V| falls by an order of
magnitude within a few steps of the DSS tap: vreg, band, vbase and the LDC
impedance of every control are therefore set on the scale of that control's
own monitored |V| over the batch at the starting taps (rounded to three
digits, so that they do not depend on the last bits of a library solve).
Across the controls: max_tap_change 1 / 4 / 16, pick PHASE / MAX / MIN over
1 - 3 monitored phases, LDC on and off, Vlimit on one control (with and
without a Vlimit node), inverse time on one, delays 15 / 30 / 45 s.

The reference loop (`reference`) follows pgw.h's text alone; its solves are
_pfg_direct_common.Ref's, its K is a longdouble Gauss-Jordan elimination
memoised by the tuple of taps, the taps themselves move in float64 (a tap is
data: tap + steps * incr, clamped, as the header states it).  Error bounds:
Ref's propagated ones, with K known to 4 kappa_2(I + D S) 2^-52 max |K| (the
figure test_gpu_reg_kernels.py holds pgw_reg_factor to) carried through c = K
(rho x), and every EXACT re-solve seeded with the previous pass's bound on U.
An env is excluded (undecidable at the reference's own accuracy) when in any
of its passes a decision sits within KNIFE of its threshold: Ref's own flags,
|dv| against band / 2, the local voltage against vlimit, |need| / incr against
an integer 1 .. max_tap_change, two monitored magnitudes (the MAX / MIN pick),
two acting controls' delays that are not identical.
"""
import functools

import numpy as np

from tests import _pfg_direct_common as C

LD, CLD = C.LD, C.CLD
DEV = "cuda:0"
EPS = 2.0 ** -52
STEP = 0.00625                  # the feeders' tap step, (1.1 - 0.9) / 32
PICK_PHASE, PICK_MAX, PICK_MIN = 0, 1, 2
KNIFE = C.KNIFE


# ---------------------------------------------------------------- the models
class Model:
    """What one pgw_reg_params describes, host side (phases: dicts of a, b,
    ctrl, tap_winding, A, B, C, tap1, tap2; S: r x r complex; taps0: the
    controls' DSS taps) and device side (rp, whose S / rho point into `keep`)."""

    def __init__(self, r, phases, taps0, S, rp, keep, reg=None):
        self.r, self.phases, self.taps0, self.S, self.rp, self.keep, self.reg = r, phases, taps0, S, rp, keep, reg
        self.n_ctrl = len(taps0)
        self.n_tri = r * (r + 1) // 2


def _dev_S_rho(S, rho, device=DEV):
    import torch
    return (torch.tensor(np.ascontiguousarray(S).view(np.float64).ravel(), device=device),
            torch.tensor(np.asarray(rho, float), dtype=torch.float64, device=device))


def _synthetic_model(r, device=DEV):
    """r regulator nodes, min(r // 2, 12) regulated phases over random node
    pairs a != b (nodes may be shared between phases), tap windings mixed 1
    and 2, about three phases per control; A, B, C of the feeders' magnitude
    (|y| 800 .. 2100 S at -45 degrees there) with a turns ratio near 1; S
    exactly complex symmetric with a positive-definite real part, entries of
    the feeders' S's magnitude (|S_jj| 0.9 .. 1.9 ohm there).  device=None:
    the host side alone (rp.S / rp.rho stay NULL).

    The scale of S matters to the bound the factor is held to.  pgw.h's D(t) =
    Y(t) - Y(DSS taps) cancels: one tap step (0.00625) off the DSS tap,
    |D| = |A| / 80, so rounding A / t^2 alone leaves D with a relative error of
    ~100 x 2^-52 in any float64 evaluation of that formula.  K = (I + D S)^-1 D
    damps it by |(I + S D)^-1| ~ 1 / (1 + |D S|): to a few 2^-52 where
    |D S| >> 1, as on the feeders (|A| |S| / 80 ~ 10 .. 50 per step), and not
    for a weakly coupled model -- with S halved the two-node model (kappa ~ 5)
    needed 6 kappa 2^-52 in a float64 NumPy transcription of the kernel, with
    this S 2.9.  Hence S of the feeders' size, not smaller."""
    from powergridworld_amd import _lib
    rng = np.random.default_rng(1000 + r)
    nq = min(r // 2, _lib.REG_MAX_PHASES)
    nc = max(1, nq // 3)
    taps0 = 1.0 + STEP * rng.integers(-3, 4, size=nc)
    phases = []
    for q in range(nq):
        a, b = (int(x) for x in rng.choice(r, 2, replace=False))
        g = q % nc
        tw = int(rng.integers(1, 3))
        y = rng.uniform(800.0, 2100.0) * np.exp(-1j * np.deg2rad(rng.uniform(40.0, 80.0)))
        nr = rng.uniform(0.9, 1.1)
        other = 1.0 + STEP * int(rng.integers(-3, 4))
        phases.append(dict(a=a, b=b, ctrl=g, tap_winding=tw, A=complex(y), B=complex(-y * nr),
                           C=complex(y * nr * nr), tap1=float(taps0[g]) if tw == 1 else other,
                           tap2=float(taps0[g]) if tw == 2 else other))
    G = rng.normal(size=(r, r))
    H = rng.normal(size=(r, r))
    re = G @ G.T / r + 0.05 * np.eye(r)
    re = 0.5 * (re + re.T)                       # x + y == y + x: exactly symmetric
    im = 0.5 * (H + H.T)
    S = re + 1j * im
    assert (S == S.T).all() and np.linalg.eigvalsh(S.real).min() > 0.0
    keep = _dev_S_rho(S, np.ones(r), device) if device is not None else None
    rp = _lib.RegParams()
    rp.n_reg, rp.r_reg, rp.n_phase, rp.n_ctrl = -(-r // 8) * 8, r, nq, nc
    for q, ph in enumerate(phases):
        d = rp.phase[q]
        d.a, d.b, d.ctrl, d.tap_winding = ph["a"], ph["b"], ph["ctrl"], ph["tap_winding"]
        d.A[0], d.A[1] = ph["A"].real, ph["A"].imag
        d.B[0], d.B[1] = ph["B"].real, ph["B"].imag
        d.C[0], d.C[1] = ph["C"].real, ph["C"].imag
        d.tap1, d.tap2 = ph["tap1"], ph["tap2"]
    for g in range(nc):                           # control records that pass the argument check
        d = rp.ctrl[g]
        q0 = g                                    # (phase g follows control g)
        d.n_mon, d.pick, d.winding, d.max_tap_change, d.vlim_node = 1, _lib.REG_PICK_PHASE, 2, 16, -1
        d.mon_node[0], d.mon_phase[0] = phases[q0]["b"], q0
        d.vreg, d.band, d.ptratio, d.ctprim, d.vbase = 120.0, 2.0, 20.0, 300.0, 120.0
        d.incr, d.min_tap, d.max_tap, d.delay = STEP, 0.9, 1.1, 15.0
    if keep is not None:
        rp.S, rp.rho = keep[0].data_ptr(), keep[1].data_ptr()
    return Model(r, phases, taps0, S, rp, keep)


# ------------------------------------------------------------- the factor
def _tri(r):
    """(i, l) of the packed upper triangle, in pgw_pfg_tables.Kreg's order."""
    i, l = np.triu_indices(r)
    assert all(int(i[k]) * r - int(i[k]) * (int(i[k]) - 1) // 2 + int(l[k]) - int(i[k]) == k for k in range(len(i)))
    return i, l


def _ref_K(m, taps):
    """One env's K = (I + D S)^-1 D from pgw.h's formulas in 50-digit mpmath
    arithmetic (every input taken at its float64 value): Gauss-Jordan with
    partial pivoting on [I + D S | D].  Returns (K as complex128, what that
    rounding left, kappa_2(I + D S)), or None where I + D S is singular."""
    import mpmath as mp
    with mp.workdps(50):
        r = m.r
        zero = mp.mpc(0)
        D = [[zero] * r for _ in range(r)]
        for ph in m.phases:
            t = mp.mpf(float(taps[ph["ctrl"]]))
            tap1, tap2 = mp.mpf(ph["tap1"]), mp.mpf(ph["tap2"])
            t1 = t if ph["tap_winding"] == 1 else tap1
            t2 = t if ph["tap_winding"] == 2 else tap2
            A, B, C = mp.mpc(ph["A"]), mp.mpc(ph["B"]), mp.mpc(ph["C"])
            a, b = ph["a"], ph["b"]
            dab = B / (t1 * t2) - B / (tap1 * tap2)
            D[a][a] += A / (t1 * t1) - A / (tap1 * tap1)
            D[a][b] += dab
            D[b][a] += dab
            D[b][b] += C / (t2 * t2) - C / (tap2 * tap2)
        S = [[mp.mpc(complex(x)) for x in row] for row in m.S]
        M = []
        for i in range(r):
            nz = [(k, D[i][k]) for k in range(r) if D[i][k] != 0]
            M.append([(1 if i == j else 0) + sum((d * S[k][j] for k, d in nz), zero) for j in range(r)])
        M64 = np.array([[complex(x) for x in row] for row in M])
        A_ = [M[i] + D[i] for i in range(r)]
        for c in range(r):
            p = max(range(c, r), key=lambda i: abs(A_[i][c]))
            if A_[p][c] == 0:
                return None
            A_[c], A_[p] = A_[p], A_[c]
            inv = 1 / A_[c][c]
            rowc = [x * inv for x in A_[c][c:]]
            A_[c][c:] = rowc
            for i in range(r):
                f = A_[i][c]
                if i != c and f != 0:
                    A_[i][c:] = [x - f * y for x, y in zip(A_[i][c:], rowc)]
        ii, ll = _tri(r)
        K = [A_[i][r + l] for i, l in zip(ii, ll)]
        hi = np.array([complex(x) for x in K])
        lo = np.array([complex(x - mp.mpc(h)) for x, h in zip(K, hi)])
        return hi, lo, float(np.linalg.cond(M64))


def _ld_D(phases, r, taps):
    """D(t) [r, r] in longdouble from pgw.h's formulas (inputs at their float64 values)."""
    D = np.zeros((r, r), CLD)
    for ph in phases:
        t = LD(float(taps[ph["ctrl"]]))
        tap1, tap2 = LD(ph["tap1"]), LD(ph["tap2"])
        t1 = t if ph["tap_winding"] == 1 else tap1
        t2 = t if ph["tap_winding"] == 2 else tap2
        A, B, Cc = CLD(ph["A"]), CLD(ph["B"]), CLD(ph["C"])
        a, b = ph["a"], ph["b"]
        dab = B / (t1 * t2) - B / (tap1 * tap2)
        D[a, a] += A / (t1 * t1) - A / (tap1 * tap1)
        D[a, b] += dab
        D[b, a] += dab
        D[b, b] += Cc / (t2 * t2) - Cc / (tap2 * tap2)
    return D


def ld_K(phases, S, taps):
    """K(t) = (I + D S)^-1 D in longdouble (Gauss-Jordan with partial pivoting
    on [I + D S | D]), mirrored from its upper triangle as the kernels read
    it: (K [r, r] clongdouble, kappa_2(I + D S)).  Its own error, of order
    kappa 2^-63, is 2^-11 of the bound K is used with.  A singular I + D S
    raises."""
    r = S.shape[0]
    D = _ld_D(phases, r, taps)
    M = np.eye(r, dtype=CLD) + D @ S.astype(CLD)
    kappa = float(np.linalg.cond(M.astype(complex)))
    A = np.concatenate([M, D], 1)
    for c in range(r):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if A[p, c] == 0:
            raise ZeroDivisionError("I + D S is singular at taps %r" % (tuple(taps),))
        if p != c:
            A[[c, p]] = A[[p, c]]
        A[c] = A[c] / A[c, c]
        f = A[:, c].copy()
        f[c] = 0
        A -= f[:, None] * A[c][None, :]
    K = A[:, r:]
    K = np.triu(K) + np.triu(K, 1).T
    return K, kappa


# ---------------------------------------------------------------- the cases
class Reading:
    """A deliberately wrong reading of the loop, for the sensitivity test."""

    def __init__(self, stale_K=False, exact_from_direct=False, no_last_control=False, all_act=False,
                 block_active=False):
        self.stale_K, self.exact_from_direct, self.no_last_control = stale_K, exact_from_direct, no_last_control
        self.all_act, self.block_active = all_act, block_active


READINGS = {
    "K not refreshed after a move": Reading(stale_K=True),
    "EXACT re-solve from the direct solution": Reading(exact_from_direct=True),
    "no control after the last allowed solve": Reading(no_last_control=True),
    "all controls act, not the nearest delay only": Reading(all_act=True),
    "next pass solves every env of a block that moved": Reading(block_active=True),
}


def _round3(x):
    return float("%.3g" % x)


class Case:
    """One regulated problem: the Problem, the regulator model (phases, S,
    taps0, ctrls: dicts of pgw_reg_ctrl's fields), the starting taps
    [N_REF, n_ctrl] and the solve's settings."""

    def __init__(self, m, n_out, n_chk, n_reg, r_reg, mode, kind="syn"):
        assert C.pad8(r_reg) <= n_reg
        self.m, self.n_out, self.n_chk, self.n_reg, self.r_reg, self.mode = m, n_out, n_chk, n_reg, r_reg, mode
        self.kind = kind
        self.prob = C.problem(m, n_out, max(n_chk, 8), n_reg, r_reg, scale=SCALE)
        if kind == "small":
            # test_gpu_reg_kernels._small_model: one regulated phase over nodes (0, 1), A = 1, B = -1,
            # C = 1, DSS taps 1 / 1, the tap on winding 2, S = [[3, 1], [1, 0]] -- at SINGULAR_TAP = 0.5,
            # D = [[0, -1], [-1, 3]] exactly and I + D S is the zero matrix
            assert r_reg == 2
            self.phases = [dict(a=0, b=1, ctrl=0, tap_winding=2, A=1 + 0j, B=-1 + 0j, C=1 + 0j, tap1=1.0, tap2=1.0)]
            self.S, self.taps0 = np.array([[3.0, 1.0], [1.0, 0.0]], complex), np.array([1.0])
        else:
            syn = _synthetic_model(r_reg, device=None)
            self.phases, self.S, self.taps0 = syn.phases, syn.S, syn.taps0
        self.n_ctrl = len(self.taps0)
        self.rho = self.prob.rho
        self.cp, self.cq = C.ctrl_powers()
        self.U_init = C.placement(m) if mode == C.PF_EXACT else None
        if mode == C.PF_EXACT:
            self.tol, self.min_iter, self.max_iter = EXACT_TOL, 1, C.EXACT_MAX_ITER
        else:
            self.tol, self.min_iter, self.max_iter = C.OD_TOL, C.OD_MIN_ITER, C.OD_MAX_ITER
        rng = np.random.default_rng(11 + r_reg)
        self.taps = self.taps0[None, :] + STEP * rng.integers(-6, 7, size=(C.N_REF, self.n_ctrl))
        self.taps.setflags(write=False)
        self._memo = {}
        self.ctrls = self._controls()

    def id(self):
        return "m%d+%d-r%d%s-CE%d-%s" % (self.m, self.n_reg, self.r_reg, "small" if self.kind == "small" else "",
                                          C.ce_of(self.m + self.n_reg),
                                          "CN%d" % C.cn_of(self.n_chk) if self.mode else "exact")

    # -- K(t), memoised by the tuple of taps (a 33-value grid per control)
    def K_of(self, taps):
        """([n, r, r] clongdouble, dK [n]: the bound the device's K is known to)."""
        Ks, dKs = [], []
        for row in taps:
            key = tuple(float(t) for t in row)
            if key not in self._memo:
                K, kappa = ld_K(self.phases, self.S, row)
                self._memo[key] = (K, 4.0 * kappa * EPS * float(np.abs(K).max()) * (1.0 + 2.0 ** -8))
            Ks.append(self._memo[key][0])
            dKs.append(self._memo[key][1])
        return np.stack(Ks), np.array(dKs)

    def node_v(self, x, c):
        """V at the regulator nodes [n, r] = rho x - S c (pgw_reg.h / pgw.h "RegControl")."""
        r = self.r_reg
        return self.rho.astype(LD) * x[:, :r] - c[:, :r] @ self.S.astype(CLD).T

    # -- the control records
    def _controls(self):
        """See the module docstring.  The scale of control g is the median over
        the batch of its picked monitored |V| at the starting taps with the
        no-load x (float64; only three digits of it are kept)."""
        r, nc = self.r_reg, self.n_ctrl
        p = self.prob
        VREG_F, BAND_F, VBASE_F, VLIM_F = TUNING.get("small" if self.kind == "small" else r, TUNING_DEFAULT)
        V = np.zeros((C.N_REF, r), complex)
        for e in range(C.N_REF):
            D = _ld_D(self.phases, r, self.taps[e]).astype(complex)
            V[e] = np.linalg.solve(np.eye(r) + self.S @ D, p.rho * p.V0reg[:r])
        out = []
        for g in range(nc):
            qs = [q for q, ph in enumerate(self.phases) if ph["ctrl"] == g]
            idx = g + r
            pick = (PICK_PHASE, PICK_MAX, PICK_MIN)[idx % 3] if len(qs) > 1 else PICK_PHASE
            n_mon = 1 if pick == PICK_PHASE else min(len(qs), 2 + idx % 2)
            winding = self.phases[qs[0]]["tap_winding"]
            node = lambda q: self.phases[q]["a" if winding == 1 else "b"]
            c = dict(n_mon=n_mon, pick=pick, winding=winding, mon_phase=qs[:n_mon],
                     mon_node=[node(q) for q in qs[:n_mon]], max_tap_change=(1, 4, 16)[idx % 3], ldc=idx % 2,
                     vlim_node=-1, inverse_time=0, ptratio=20.0, ctprim=300.0, r_ldc=0.0, x_ldc=0.0,
                     incr=STEP, min_tap=0.9, max_tap=1.1, delay=(15.0, 30.0)[g % 2], vlimit=0.0)
            mags = np.abs(V[:, c["mon_node"]])
            v = mags[:, 0] if pick == PICK_PHASE else mags.max(1) if pick == PICK_MAX else mags.min(1)
            scale = float(np.median(v)) / c["ptratio"]
            c["vreg"] = _round3(VREG_F * scale)
            c["band"] = _round3(BAND_F * c["vreg"])
            c["vbase"] = _round3(VBASE_F * c["band"] / (2.0 * STEP))
            if c["ldc"]:
                # (R + jX) I / ctprim of a tenth of the control voltage at the median current
                ph = self.phases[c["mon_phase"][0]]
                i_in = np.abs(ph["C" if winding == 2 else "A"]) * float(np.median(v))
                z = 0.1 * scale * c["ctprim"] / i_in
                c["r_ldc"], c["x_ldc"] = _round3(z), _round3(2.0 * z)
            first = g == 0
            last = g == nc - 1
            if (first and nc > 1) or (nc == 1 and r % 2 == 1):
                c["vlimit"] = _round3(VLIM_F * c["vreg"])
                if r % 3 == 0:                        # Vlimit read at a node of its own (Bus=)
                    c["vlim_node"] = self.phases[qs[-1]]["b" if winding == 1 else "a"]
            if (last and nc > 1) or (nc == 1 and r % 2 == 0):
                c["inverse_time"], c["delay"] = 1, 45.0
            out.append(c)
        return out

    def reg_params(self, S_ptr, rho_ptr):
        """The pgw_reg_params (ctypes) of this case over device copies of S / rho."""
        from powergridworld_amd import _lib
        reg = dict(nodes=list(range(self.r_reg)), phases=self.phases, ctrls=self.ctrls)
        rp = _lib.reg_params(reg, S_ptr, rho_ptr)
        assert rp.n_reg == C.pad8(self.r_reg)
        return rp


# W scaled to a contraction (Ref's propagated bound grows without limit over an env's passes otherwise);
# the exact rule stops at 1e-7: at 1e-10 the bound on U -- up to 2e-11 with K known to 4 kappa 2^-52 max |K|
# -- leaves the stopping test of a quarter of the envs undecidable
SCALE = C.CONV_SCALE
EXACT_TOL = 1e-7
# vreg / the median monitored |V|, band / vreg, vbase / (band / (2 incr)), vlimit / vreg: chosen, on the
# reference alone, so that every env of every compared case comes to rest within 15 passes (a |V| that
# falls off steeply on both sides of the DSS tap makes narrow bands cycle); r_reg = 2 takes a band placed
# higher, under which its envs move up as well as down; the weakly coupled two-node model a narrow one
TUNING = {2: (2.0, 1.4, 1.0, 1.6), "small": (1.0, 0.05, 1.0, 1.02)}
TUNING_DEFAULT = (1.0, 1.6, 1.5, 1.15)
SINGULAR_TAP = 0.5


@functools.lru_cache(maxsize=None)
def case(m, n_out, n_chk, n_reg, r_reg, mode, kind="syn"):
    return Case(m, n_out, n_chk, n_reg, r_reg, mode, kind)


# ---------------------------------------------------------------- the control pass
def control_pass(ctrls, phases, V, taps, all_act=False):
    """RegControl.Sample + DoPendingAction + the nearest delay (pgw.h,
    pgw_reg_control) for n envs at once: V [n, r] clongdouble node voltages,
    taps [n, n_ctrl] float64.  Returns (new taps, moved [n], knife [n])."""
    n, nc = taps.shape
    want = taps.copy()
    dl = np.full((n, nc), np.inf, LD)
    knife = np.zeros(n, bool)
    ar = np.arange(n)
    for g, c in enumerate(ctrls):
        tap = taps[:, g]
        nodes = np.array(c["mon_node"][:c["n_mon"]])
        mags = np.abs(V[:, nodes])                                       # [n, n_mon]
        k = np.zeros(n, int)
        mk = mags[:, 0].copy()
        for i in range(1, c["n_mon"]):
            better = mags[:, i] > mk if c["pick"] == PICK_MAX else mags[:, i] < mk
            k, mk = np.where(better, i, k), np.where(better, mags[:, i], mk)
            for i2 in range(i):            # a near tie of the pick (the same node twice ties exactly: the first)
                if nodes[i] != nodes[i2]:
                    knife |= np.abs(mags[:, i] / mags[:, i2] - 1) < KNIFE
        pt = LD(c["ptratio"])
        vc = V[ar, nodes[k]] / pt
        vlocal = np.zeros(n, LD)
        if c["vlimit"] > 0.0:
            vlocal = np.abs(V[:, c["vlim_node"]] / pt) if c["vlim_node"] >= 0 else np.abs(vc)
        if c["ldc"]:
            i_in = np.zeros(n, CLD)
            for i in range(c["n_mon"]):                                  # the picked phase's current
                ph = phases[c["mon_phase"][i]]
                t = tap.astype(LD)
                t1 = t if ph["tap_winding"] == 1 else LD(ph["tap1"]) + 0 * t
                t2 = t if ph["tap_winding"] == 2 else LD(ph["tap2"]) + 0 * t
                yaa, yab, ybb = CLD(ph["A"]) / (t1 * t1), CLD(ph["B"]) / (t1 * t2), CLD(ph["C"]) / (t2 * t2)
                va, vb = V[:, ph["a"]], V[:, ph["b"]]
                cur = yab * va + ybb * vb if c["winding"] == 2 else yaa * va + yab * vb
                i_in = np.where(k == i, cur, i_in)
            vc = vc - CLD(complex(c["r_ldc"], c["x_ldc"])) * (-i_in / LD(c["ctprim"]))
        dv = LD(c["vreg"]) - np.abs(vc)
        half = LD(c["band"]) / 2
        over = (vlocal > LD(c["vlimit"])) if c["vlimit"] > 0.0 else np.zeros(n, bool)
        trig = (np.abs(dv) > half) | over
        knife |= np.abs(np.abs(dv) / half - 1) < KNIFE
        if c["vlimit"] > 0.0:
            knife |= np.abs(vlocal / LD(c["vlimit"]) - 1) < KNIFE
        need = np.where(over, LD(c["vlimit"]) - vlocal, dv) / LD(c["vbase"])
        q = np.abs(need) / LD(c["incr"])
        whole = np.rint(q)
        knife |= trig & (whole >= 1) & (whole <= c["max_tap_change"]) & (np.abs(q - whole) < KNIFE)
        steps = np.minimum(np.maximum(np.trunc(q), 1), c["max_tap_change"]).astype(np.float64)
        nt = tap + np.where(need > 0, steps, -steps) * np.float64(c["incr"])          # float64: the tap is data
        nt = np.minimum(np.maximum(nt, c["min_tap"]), c["max_tap"])
        acts = trig & (nt != tap)
        want[:, g] = np.where(acts, nt, tap)
        if c["inverse_time"]:
            f = np.minimum(LD(10), 2 * np.abs(dv) / LD(c["band"]))
            with np.errstate(divide="ignore"):
                d = np.where(f > 0, LD(c["delay"]) / np.where(f > 0, f, 1), np.inf)
        else:
            d = np.full(n, LD(c["delay"]))
        dl[:, g] = np.where(acts, d, np.inf)
    dmin = dl.min(1)
    acting = want != taps
    if not all_act:
        fin = np.isfinite(dl) & np.isfinite(dmin)[:, None]
        ratio = np.where(fin, dl, 1) / np.where(fin, dmin[:, None], 2)
        near = acting & (dl != dmin[:, None]) & (np.abs(ratio - 1) < KNIFE)
        knife |= near.any(1)
        acting &= dl == dmin[:, None]
    new = np.where(acting, want, taps)
    return new, acting.any(1), knife


# ---------------------------------------------------------------- the reference loop
def run_loop(cs, max_passes, reading=None, taps=None, n=C.N_REF):
    """pgw.h's loop for the first n envs of the case, each env on its own.
    Returns a dict: taps [n, n_ctrl], passes, iters, u / e_u, V / e_v (output
    rows), x / e_x, c / e_c of each env's last solve, excluded, finished (the
    env's last control pass moved nothing), pass_moved (per pass, the envs that
    moved) ."""
    rd = reading or Reading()
    p = cs.prob
    ref = C.Ref(p, cs.mode)
    taps = np.array(cs.taps[:n] if taps is None else taps[:n], float)
    K, dK = cs.K_of(taps)
    active = np.ones(n, bool)
    passes = np.zeros(n, int)
    excluded = np.zeros(n, bool)
    finished = np.zeros(n, bool)
    res = {}
    e_u = None
    blocks = np.arange(n) // 64
    for ps in range(1, max_passes + 1):
        idx = np.nonzero(active)[0]
        U_init = e_init = None
        if cs.mode == C.PF_EXACT:
            if ps == 1:
                U_init = None if cs.U_init is None else cs.U_init[idx]
            elif not rd.exact_from_direct:
                U_init, e_init = res["u"][idx], res["e_u"][idx]
        sol = ref.solve(len(idx), cs.cp[:, idx], cs.cq[:, idx], cs.tol, cs.min_iter, cs.max_iter, U_init=U_init,
                        K=K[idx], e_init=e_init, dK=dK[idx])
        for key in ("u", "e_u", "V", "e_v", "iters", "x", "c", "e_x", "e_c"):
            if key not in res:
                res[key] = np.zeros((n,) + sol[key].shape[1:], sol[key].dtype)
            res[key][idx] = sol[key]
        excluded[idx] |= sol["excluded"]
        passes[idx] += 1
        if rd.no_last_control and ps == max_passes:
            break
        Vn = cs.node_v(res["x"][idx], res["c"][idx])
        new, moved, knife = control_pass(cs.ctrls, cs.phases, Vn, taps[idx], all_act=rd.all_act)
        excluded[idx] |= knife
        taps[idx] = new
        finished[idx] = ~moved
        mv = idx[moved]
        if len(mv) and not rd.stale_K:
            K[mv], dK[mv] = cs.K_of(taps[mv])
        active = np.zeros(n, bool)
        active[mv] = True
        if rd.block_active:
            active = np.isin(blocks, np.unique(blocks[mv]))
        if not active.any():
            break
    res.update(taps=taps, passes=passes, excluded=excluded, finished=finished)
    return res


@functools.lru_cache(maxsize=None)
def reference(m, n_out, n_chk, n_reg, r_reg, mode, max_passes=15):
    """The reference loop of a case over N_REF envs (computed once, shared, read-only)."""
    r = run_loop(case(m, n_out, n_chk, n_reg, r_reg, mode), max_passes)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


# ---------------------------------------------------------------- the GPU file's cases
MAX_PASSES = 15
# (b) against the reference: (m, n_out, n_chk, n_reg, r_reg, mode) -- each CE x {EXACT, one CN >= 2}
REF_CASES = (
    (8, 7, 0, 8, 5, C.PF_EXACT), (8, 9, 40, 24, 17, C.PF_OPENDSS),
    (40, 11, 0, 24, 17, C.PF_EXACT), (40, 13, 72, 8, 2, C.PF_OPENDSS),
    (104, 8, 0, 24, 17, C.PF_EXACT), (72, 10, 136, 8, 5, C.PF_OPENDSS),
)
# the cap cases: (case, max_passes)
CAP_CASES = ((REF_CASES[0], 1), (REF_CASES[0], 2), (REF_CASES[5], 1), (REF_CASES[5], 2))
# the other edges (rest beside work, a repeated call, a singular env, passes = NULL): one CE 1 and one CE 4 shape
EDGE_CASES = (REF_CASES[0], (104, 8, 72, 24, 17, C.PF_OPENDSS))
# a singular env in a running block: the two-node model (kind "small"), three envs started at SINGULAR_TAP
SINGULAR_CASES = ((8, 7, 0, 8, 2, C.PF_EXACT, "small"), (72, 9, 40, 8, 2, C.PF_OPENDSS, "small"))
SINGULAR_ENVS = (5, 100, 129)
# (a) bit for bit against the host loop: (m, n_out, n_chk, n_reg, r_reg, mode, n, max_iter or None) -- the
# smallest shapes that select each instantiation k_pf_regulated<CE, CN> with both factor shapes (two envs
# per 64 lanes for r_reg <= 16, one above); every other case stops its solves at 3 (OPENDSS: 2) iterations, so that
# converged and unconverged solves (iters of either sign) alternate within an env's passes
X, O = C.PF_EXACT, C.PF_OPENDSS
SHAPES = (
    (8, 7, 0, 8, 5, X, 130, None), (8, 9, 0, 24, 17, X, 1, 3), (8, 8, 8, 24, 24, O, 130, None),
    (8, 11, 40, 8, 2, O, 65, 2), (8, 13, 72, 24, 17, O, 65, None), (8, 7, 136, 8, 5, O, 1, 2),
    (8, 10, 136, 24, 24, O, 130, None),
    (40, 7, 0, 16, 12, X, 130, 3), (40, 9, 8, 24, 17, O, 65, None), (40, 12, 40, 16, 16, O, 1, 2),
    (40, 13, 72, 24, 24, O, 130, None), (40, 8, 136, 16, 12, O, 65, 2), (40, 10, 0, 24, 17, X, 1, None),
    (72, 7, 0, 8, 5, X, 130, 3), (104, 13, 8, 24, 24, O, 130, None), (72, 9, 40, 8, 2, O, 1, 2),
    (104, 11, 72, 24, 17, O, 65, None), (72, 12, 136, 8, 5, O, 65, 2), (104, 8, 136, 24, 17, O, 130, None),
    (104, 10, 0, 24, 24, X, 1, 3),
)


def shape_id(s):
    m, n_out, n_chk, n_reg, r, mode, n, mi = s
    return "m%d+%d-r%d-CE%d-%s-n%d%s" % (m, n_reg, r, C.ce_of(m + n_reg), "CN%d" % C.cn_of(n_chk) if mode else "exact",
                                          n, "-it%d" % mi if mi else "")


def check_shapes():
    """SHAPES reaches all 15 instantiations, every CE with both factor shapes,
    with one env and with three blocks; the other lists keep what they promise."""
    inst = {(C.ce_of(s[0] + s[3]), C.cn_of(s[2]) if s[5] else 0) for s in SHAPES}
    assert inst == {(ce, cn) for ce in (1, 2, 4) for cn in (0, 1, 2, 4, 8)}, sorted(inst)
    for ce in (1, 2, 4):
        mine = [s for s in SHAPES if C.ce_of(s[0] + s[3]) == ce]
        assert any(s[4] <= 16 for s in mine) and any(s[4] > 16 for s in mine), ce
        assert any(s[6] == 1 for s in mine) and any(s[6] == 130 for s in mine), ce
        assert any(s[7] for s in mine) and any(not s[7] for s in mine), ce
    assert {s[6] for s in SHAPES} == {1, 65, 130}
    assert {(s[0], s[3]) for s in SHAPES} == {(8, 8), (8, 24), (40, 16), (40, 24), (72, 8), (104, 24)}
    assert {s[2] for s in SHAPES} == {0, 8, 40, 72, 136} and {s[4] for s in SHAPES} == {2, 5, 12, 16, 17, 24}
    assert all(7 <= s[1] <= 13 and C.pad8(s[4]) == s[3] or s[3] == 24 for s in SHAPES)
    ref = {(C.ce_of(c[0] + c[3]), "exact" if c[5] == X else "od") for c in REF_CASES}
    assert len(REF_CASES) == 6 and ref == {(ce, k) for ce in (1, 2, 4) for k in ("exact", "od")}
    assert all(C.cn_of(c[2]) >= 2 for c in REF_CASES if c[5] == O)
    assert [C.ce_of(c[0] + c[3]) for c in EDGE_CASES] == [1, 4]
    assert [C.ce_of(c[0] + c[3]) for c in SINGULAR_CASES] == [1, 4]
    assert {C.ce_of(c[0] + c[3]) for c, _ in CAP_CASES} == {1, 4} and {k for _, k in CAP_CASES} == {1, 2}
