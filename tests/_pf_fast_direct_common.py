"""Shared inputs and reference of tests/test_cpu_pf_fast_ref.py and
tests/test_gpu_pf_fast_direct.py: synthetic problems for the C ABI of
pgw_pf_solve / pgw_pf_solve_f32 without `od` (include/pgw.h, "Distribution power
flow"; k_pf_solve and k_coord_pf in csrc/pgw_pf.hip), voltages placed in every
band of every element, and the map u <- u0 + W'' I'(u) restated from the
header's text and PFSolver's comments in np.longdouble (63-bit mantissa; a test
that finds a shorter one skips).  Nothing in this file touches a GPU; it calls
the host function pgw_pf_pack, and the reference reads W'', u0, the squared
bands and row 0 from the block it wrote -- exactly what the device receives
(test_cpu_pf_fast_ref.py holds pgw_pf_pack itself to longdouble).

Problems (everything seeded): M = padded element count (8, 14, 16), m_true
real elements, per-element base voltage, nph in 1..3, signed base_kw /
base_kvar of `power_scale` W per phase, a dense exactly symmetric complex W''
with a dominant diagonal scaled so that W'' I' is of order 0.05 pu, n_out
output rows G / V0 (pu), n_ctrl controllable slots (slot 0 holds two elements,
every other slot one, while elements last).  Elements >= m_true are
OpenDSSSolver._base_params' padding: vbase 1, band 0.5 / 0.95 / 1.05, nph 1,
ctrl -1, zero load, zero rows and columns.

Which kernel instantiation a problem runs (PGW_PF_DISPATCH) is restated in
`inst_of`: <8,F,T,T>, <14,T,F,F> (one band over all 14 elements, n_ctrl <= 1,
no load_scale, n_out <= 1), <14,T,F,T> (the same, n_out > 1), <14,F,T,T>,
<16,F,T,T>.

Error bound of one pass (derived, u = 2^-53, per component; -ffp-contract=off,
so every product and sum below is one rounding unless written as fma).

Powers.  GC variants form s = ((kw * scale + p) * 1000) / nph: four roundings,
the first relative to |kw scale| alone, so |ds| <= 4u Sa with the amplitude
Sa = (|kw scale| + |p|) 1000 / nph (no cancellation credit).  The other
variants form s = fma(f, pc, s0) with s0 = (kw 1000) / nph (two roundings on
the host), f = 1000 / nph (one) and the fma's own: <= 4u Sa as well.  Allowed:
5u Sa per part.

Law.  m2 = fma(ui, ui, ur * ur): relative 2u (both terms positive).  The clamp
to [vmin^2, vmax^2] is continuous, so a comparison decided the other way moves
mc by no more than m2's own error; the switch at vlow is not, and an env within
KNIFE of it is left out.  g = fast_rcp(mc), v_rcp_f64 and two Newton steps
whose last fma rounds once from a residual already at 2^-48: allowed 2u.  So g
is within 4u, g ur within 5u, and ir = fma(s_r, g ur, -(s_i g ui)) within
(5 + 5 + 1 + 1) u = 12u of the amplitude Ar = g (Sa_r |ur| + Sa_i |ui|);
likewise ii against Ai = g (Sa_r |ui| + Sa_i |ur|).  is = ir + ii: 13u (Ar + Ai).

Matvec, 3-multiplication form: A = u0re + sum Wr ir, B = sum Wi ii, C = u0sum +
sum Ws is (M fmas each; u0sum and Ws = Wr + Wi carry the packer's rounding),
re = A - B, im = (C - A) - B.  With
    Pre_i = |u0re_i| + sum_k (|Wr_ik| Ar_k + |Wi_ik| Ai_k)
    Pim_i = |u0re_i| + |u0im_i| + sum_k (|Wr_ik| + |Wi_ik|) (Ar_k + Ai_k)
the chains cost (M + 1)u, the subtraction 1u, the currents 12u:
    e_re_i = (M + 14) u Pre_i.
The imaginary part is a difference of three sums that each reach Pim: C costs
(M + 1)u for its chain, 2u for the packer's two roundings and 13u for `is`; A
and B (M + 1 + 12)u each against parts of Pim; the two subtractions 2u against
at most 2 Pim.  Summed against Pim: (M + 16) + (M + 13) + 4 = 2M + 33,
    e_im_i = (2M + 33) u Pim_i
-- over (|Wr| + |Wi|)(|Ir| + |Ii|), not |W||I|.

Output rows.  vr = V0r + sum (Gr ir - Gi ii), vi alike: 2M fmas per chain,
    e_vr = u ((2M + 1)|V0r| + (2M + 13) sum (|Gr| Ar + |Gi| Ai)),
e_vi with Ar, Ai exchanged; |V| = sqrt(fma(vi, vi, vr vr)) adds 2u |V|, and
| |a| - |b| | <= |a - b| <= hypot(e_vr, e_vi).

k passes.  Above vlow and inside the band I' = conj(S) / conj(u), so inputs off
by d = |du| (modulus, hypot of the two component bounds) move the current by
|S| d / (|u| |u'|); on the clamped sides and below vlow I' = conj(S) g u moves by
|S| g d; the clamp is continuous, so |dI'_k| <= |S_k| g_k d_k everywhere but
across vlow ((1 + 1e-6) covers the second order).  The next iterate's modulus,
hence each of its components, then moves by at most sum_k |W''_ik| |dI'_k|, a row
by sum_k |G_ok| |dI'_k|, added to that pass's own bound.
"""
import collections
import ctypes
import functools

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
U53 = 2.0 ** -53
SQRT2 = float(np.sqrt(2.0))
N_REF = 520                      # two 256-lane blocks and 8 lanes; a batch of n takes the first n
EDGE = 1e-6                      # relative distance of the threshold probes
KNIFE = 1e-9                     # an env this close (rel) to a discontinuous threshold is undecidable
KNIFE_TOL = 1e-6                 # ... or with its stopping error this close (rel) to tol
PAD_BAND = (0.5, 0.95, 1.05)     # vlow, vmin, vmax of _base_params' padding
MOVED_BAND = (0.62, 0.93, 1.07)  # one band for every true element, not the padding's
VBASES = (2401.78, 277.13, 120.0)
W_SCALE = 0.05
K_ROWS_LDS = 4096                # kRowsLds (csrc/pgw_pf.hip)
CONV_TOL, CONV_MAX_ITER = 1e-10, 30


def have_longdouble():
    return np.finfo(np.longdouble).nmant >= 63


def padded_m(m):
    return 8 if m <= 8 else 14 if m <= 14 else 16


def row_pairs(M):
    return (2 * M + 2 + 15) // 16


def last_lds_rows(M):
    """The largest n_out whose rows pf_rows_stage keeps in LDS."""
    return K_ROWS_LDS // (16 * row_pairs(M))


def inst_of(M, uniform_all, n_ctrl, n_out, load_scale):
    """PGW_PF_DISPATCH restated: uniform_all = one band over all M (padded) elements."""
    if M != 14:
        return "m%d-FTT" % M
    if uniform_all and n_ctrl <= 1 and not load_scale:
        return "m14-TFF" if n_out <= 1 else "m14-TFT"
    return "m14-FTT"


# the problem shape that selects each instantiation: (M, band, n_ctrl, n_out)
INST = collections.OrderedDict([
    ("m8-FTT", (8, "each", 2, 5)),
    ("m14-TFF", (14, "pad", 1, 1)),
    ("m14-TFT", (14, "pad", 1, 5)),
    ("m14-FTT", (14, "each", 2, 5)),
    ("m16-FTT", (16, "each", 2, 5)),
])


# ---------------------------------------------------------------- the problems
class Problem:
    """One synthetic pgw_pf_params / pgw_pf_tables, host side (float64 /
    complex128).  band: "pad" (every element the padding's band), "moved"
    (every true element MOVED_BAND), "each" (vlow, vmin, vmax all differ)."""

    def __init__(self, M, m_true, n_out, n_ctrl, band="each", power_scale=1.0, seed=0):
        assert M == padded_m(M) and 1 <= m_true <= M and 0 <= n_ctrl <= 8
        self.M, self.m_true, self.n_out, self.n_ctrl = M, m_true, n_out, n_ctrl
        self.band, self.power_scale, self.seed = band, power_scale, seed
        real = np.arange(M) < m_true
        rng = np.random.default_rng(7000 + 31 * M + seed)          # the elements depend on M alone (placement())
        self.vbase = np.where(real, np.array(VBASES)[rng.integers(0, 3, M)], 1.0)
        self.nph = np.where(real, rng.integers(1, 4, M).astype(float), 1.0)
        sign = np.where(rng.random(M) < 0.25, -1.0, 1.0)
        self.base_kw = np.where(real, sign * rng.uniform(0.3, 1.0, M) * 1e-3 * power_scale * self.nph, 0.0)
        self.base_kvar = np.where(real, rng.uniform(-0.5, 0.5, M) * 1e-3 * power_scale * self.nph, 0.0)
        each = (rng.uniform(0.4, 0.8, M), rng.uniform(0.85, 0.97, M), rng.uniform(1.02, 1.12, M))
        one = {"pad": PAD_BAND, "moved": MOVED_BAND}.get(band)
        self.vlow, self.vmin, self.vmax = (np.where(real, each[j] if one is None else one[j], PAD_BAND[j])
                                           for j in range(3))
        rng = np.random.default_rng(8000 + 31 * M + 7 * m_true + n_ctrl + seed)
        self.elem_ctrl = np.full(M, -1)
        order = list(rng.permutation(m_true))
        for s in range(n_ctrl):
            for _ in range(2 if s == 0 else 1):
                if order:
                    self.elem_ctrl[order.pop()] = s
        rng = np.random.default_rng(5000 + 131 * M + 17 * n_out + m_true + seed)

        def dense(rows):
            mag = rng.uniform(0.02, 0.3, (rows, M))
            return mag * np.exp(2j * np.pi * rng.random((rows, M)))

        def unit(rows):
            return rng.uniform(0.97, 1.03, rows) * np.exp(2j * np.pi * rng.random(rows))

        A = dense(M)
        A[np.arange(M), np.arange(M)] = np.exp(2j * np.pi * rng.random(M))     # dominant diagonal
        A = np.triu(A) + np.triu(A, 1).T                                       # exactly symmetric
        keep = np.outer(real, real)
        self.Wpu = np.where(keep, A * (W_SCALE / power_scale), 0.0)
        # volts, as opendss.py hands them to pgw_pf_pack (vb_i vb_k commutes: still exactly symmetric)
        self.W = self.Wpu * np.outer(self.vbase, self.vbase)
        self.U0 = np.where(real, unit(M) * self.vbase, 0.0)
        self.G = np.where(real[None, :], dense(n_out) * (W_SCALE / power_scale), 0.0)
        self.V0 = unit(n_out)
        self._block = None
        self._freeze()

    def _freeze(self):
        for a in vars(self).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)

    def copy(self, **arrays):
        """A copy with some arrays replaced (repacked on demand)."""
        q = Problem.__new__(Problem)
        q.__dict__.update(self.__dict__)
        for k, v in arrays.items():
            setattr(q, k, np.array(v))
        q.n_out = len(q.V0)
        q._block = None
        q._freeze()
        return q

    def dup_rows(self, positions):
        """A copy whose listed rows repeat row 0's G and V0 bit for bit."""
        G, V0 = self.G.copy(), self.V0.copy()
        for o in positions:
            G[o], V0[o] = G[0], V0[0]
        return self.copy(G=G, V0=V0)

    def with_band(self, k, vlow, vmin, vmax):
        """A copy with element k's band moved."""
        b = [self.vlow.copy(), self.vmin.copy(), self.vmax.copy()]
        b[0][k], b[1][k], b[2][k] = vlow, vmin, vmax
        return self.copy(vlow=b[0], vmin=b[1], vmax=b[2])

    @property
    def uniform_all(self):
        return all((a == a[0]).all() for a in (self.vlow, self.vmin, self.vmax))

    def inst(self, load_scale=False):
        return inst_of(self.M, self.uniform_all, self.n_ctrl, self.n_out, load_scale)

    def params(self, tol=0.0, max_iter=1):
        from powergridworld_amd import _lib
        p = _lib.PFParams()
        for k in range(self.M):
            p.vbase[k], p.vmin[k], p.vmax[k], p.vlow[k] = self.vbase[k], self.vmin[k], self.vmax[k], self.vlow[k]
            p.nph[k], p.base_kw[k], p.base_kvar[k] = self.nph[k], self.base_kw[k], self.base_kvar[k]
            p.elem_ctrl[k] = int(self.elem_ctrl[k])
        p.tol, p.m, p.n_ctrl, p.n_out, p.max_iter = tol, self.M, self.n_ctrl, self.n_out, max_iter
        return p

    def g_flat(self):
        """[n_out x M] complex row-major as doubles (pgw_pf_tables.G)."""
        return np.ascontiguousarray(self.G).view(np.float64).ravel()

    def v0_flat(self):
        return np.ascontiguousarray(self.V0).view(np.float64).ravel()

    def block(self):
        """What pgw_pf_pack writes for this problem (host call; cached, read-only)."""
        if self._block is None:
            self._block = pack(self.params(), self.W, self.U0, self.G[0] if self.n_out else None,
                               self.V0[:1] if self.n_out else None)
        return self._block


def _dptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def pack(prm, W, U0, G0, V0_0, expect_ok=True):
    """pgw_pf_pack on host arrays: the block (read-only), or (rc, message)."""
    from powergridworld_amd import _lib
    lib = _lib.lib()
    M = prm.m
    w = np.ascontiguousarray(W, complex).view(np.float64).ravel()
    u = np.ascontiguousarray(U0, complex).view(np.float64).ravel()
    g = None if G0 is None else np.ascontiguousarray(G0, complex).view(np.float64).ravel()
    v = None if V0_0 is None else np.ascontiguousarray(V0_0, complex).view(np.float64).ravel()
    size = lib.pgw_pf_pack_size(M) if 1 <= M <= 16 else 1024
    out = np.full(size + 16, np.nan)                      # (guard: nothing past pgw_pf_pack_size)
    rc = lib.pgw_pf_pack(prm, _dptr(w), _dptr(u), _dptr(g), _dptr(v), _dptr(out))
    if not expect_ok:
        return rc, lib.pgw_last_error().decode()
    assert rc == 0, lib.pgw_last_error().decode()
    assert np.isnan(out[size:]).all() and np.isfinite(out[:size]).all()
    blk = out[:size].copy()
    blk.setflags(write=False)
    return blk


def block_layout(M):
    """Offsets of the packed block (PFBlock<M>, csrc/pgw_pf.hip)."""
    T = M * (M + 1) // 2
    u0 = 3 * T
    return dict(T=T, u0re=u0, u0im=u0 + M, u0sum=u0 + 2 * M, lo2=u0 + 3 * M, mn2=u0 + 4 * M, mx2=u0 + 5 * M,
                g0re=u0 + 6 * M, g0im=u0 + 7 * M, v0re=u0 + 8 * M, v0im=u0 + 8 * M + 1, size=u0 + 8 * M + 2)


@functools.lru_cache(maxsize=None)
def problem(M, m_true, n_out, n_ctrl, band="each", power_scale=1.0, seed=0):
    return Problem(M, m_true, n_out, n_ctrl, band, power_scale, seed)


def inst_problem(inst, n_out=None, n_ctrl=None, power_scale=1.0):
    M, band, nc, no = INST[inst]
    return problem(M, M, no if n_out is None else n_out, nc if n_ctrl is None else n_ctrl, band, power_scale)


@functools.lru_cache(maxsize=None)
def placement(M, band="each", seed=0):
    """U_init [N_REF, M] complex: per (env, element) a magnitude from a ladder
    over 0.3 .. 1.6 pu, or (half of the samples) a value a relative EDGE on
    either side of the element's own vlow, vmin, vmax; random phase.  The bands
    are those of every Problem of this (M, band) with m_true = M."""
    p = problem(M, M, 1, 1, band)
    rng = np.random.default_rng(777 + M + seed)
    ladder = np.linspace(0.3013, 1.6013, 261)             # (off the round limits 0.5, 0.62, 0.95, 1.05 ...)
    mag = ladder[rng.integers(0, len(ladder), (N_REF, M))]
    thr = np.stack([p.vlow, p.vmin, p.vmax])                                 # [3, M]
    e, k = np.meshgrid(np.arange(N_REF), np.arange(M), indexing="ij")
    slot = (e * 5 + k * 3) % 12
    probe = thr[(slot % 6) // 2, k] * np.where(slot % 2 == 0, 1.0 - EDGE, 1.0 + EDGE)
    mag = np.where(slot < 6, probe, mag)
    u = mag * np.exp(2j * np.pi * rng.random((N_REF, M)))
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def ctrl_powers(power_scale=1.0, seed=0):
    """(ctrl_p, ctrl_q) [8, N_REF] kW / kvar; a problem takes its first n_ctrl rows."""
    rng = np.random.default_rng(4242 + seed)
    p = rng.uniform(-1.0, 1.5, (8, N_REF)) * 1e-3 * power_scale
    q = rng.uniform(-0.5, 0.5, (8, N_REF)) * 1e-3 * power_scale
    for a in (p, q):
        a.setflags(write=False)
    return p, q


@functools.lru_cache(maxsize=None)
def load_scale(seed=0):
    a = np.random.default_rng(99 + seed).uniform(0.6, 1.4, N_REF)
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------- the reference
class Variant:
    """A deliberately wrong reading, for the sensitivity test."""

    def __init__(self, roll=False, shift=None, swap=False, no_clamp=False, drop_slot=None, no_nph=False,
                 rows_from_final=False):
        self.roll, self.shift, self.swap, self.no_clamp = roll, shift, swap, no_clamp
        self.drop_slot, self.no_nph, self.rows_from_final = drop_slot, no_nph, rows_from_final


class Ref:
    """The longdouble restatement for one Problem, on the operands of its packed block."""

    def __init__(self, prob, variant=None, W=None):
        self.p, self.var = prob, variant or Variant()
        M, L, blk = prob.M, block_layout(prob.M), prob.block()
        iu = np.triu_indices(M)                           # row-major upper triangle: the block's order

        def full(part):
            A = np.zeros((M, M))
            A[iu] = blk[part * L["T"]:(part + 1) * L["T"]]
            return A + np.triu(A, 1).T

        self.Wr, self.Wi = full(0), full(1)
        if W is not None:                                 # (sensitivity: a non-symmetric matrix)
            self.Wr, self.Wi = np.array(W.real), np.array(W.imag)
        self.W = self.Wr.astype(LD) + 1j * self.Wi.astype(LD)
        self.u0r, self.u0i = blk[L["u0re"]:L["u0re"] + M], blk[L["u0im"]:L["u0im"] + M]
        self.u0 = self.u0r.astype(LD) + 1j * self.u0i.astype(LD)
        band = [blk[L[k]:L[k] + M].astype(LD) for k in ("lo2", "mn2", "mx2")]
        if self.var.roll:
            band = [np.roll(a, -1) for a in band]
        if self.var.shift:
            j = ("vlow", "vmin", "vmax").index(self.var.shift[0])
            band[j] = band[j] * LD(self.var.shift[1]) ** 2
        if self.var.swap:
            band[1], band[2] = band[2], band[1]
        self.lo2, self.mn2, self.mx2 = band
        self.G = prob.G.astype(CLD)
        self.V0 = prob.V0.astype(CLD)
        if prob.n_out:                                    # row 0: the block's copy
            self.G[0] = blk[L["g0re"]:L["g0re"] + M].astype(LD) + 1j * blk[L["g0im"]:L["g0im"] + M].astype(LD)
            self.V0[0] = LD(blk[L["v0re"]]) + 1j * LD(blk[L["v0im"]])
        self.aWr, self.aWi = np.abs(self.Wr), np.abs(self.Wi)
        self.aGr, self.aGi = np.abs(prob.G.real), np.abs(prob.G.imag)
        self.aW, self.aG = np.hypot(self.Wr, self.Wi), np.abs(prob.G)

    # -- S_k per env: pgw.h "Element k draws S_k = ((base_kw[k] + ctrl_p[elem_ctrl[k]]) * 1000 / nph[k])
    # + j(...kvar)", base_kw / base_kvar times load_scale; returns conj(S) = (cr, ci) and the amplitudes
    def powers(self, n, ctrl_p=None, ctrl_q=None, ls=None):
        p = self.p
        s = np.ones(n, LD) if ls is None else ls[:n].astype(LD)
        kw = s[:, None] * p.base_kw.astype(LD)[None, :]
        kvar = s[:, None] * p.base_kvar.astype(LD)[None, :]
        akw, akvar = np.abs(kw).astype(float), np.abs(kvar).astype(float)
        for k in np.nonzero((p.elem_ctrl >= 0) & (p.elem_ctrl < p.n_ctrl))[0]:
            c = p.elem_ctrl[k]
            if c == self.var.drop_slot:
                continue
            if ctrl_p is not None:
                kw[:, k] += ctrl_p[c, :n].astype(LD)
                akw[:, k] += np.abs(ctrl_p[c, :n])
            if ctrl_q is not None:
                kvar[:, k] += ctrl_q[c, :n].astype(LD)
                akvar[:, k] += np.abs(ctrl_q[c, :n])
        nph = np.ones(p.M, LD) if self.var.no_nph else p.nph.astype(LD)
        f = 1000 / nph
        return kw * f, -(kvar * f), akw * f.astype(float), akvar * f.astype(float)

    def gain(self, m2, force_low=None):
        low = m2 <= self.lo2
        if force_low is not None:                         # (decided by the caller: |u|^2 == vlow^2 in float64)
            low = np.where(force_low[0], force_low[1], low)
        mc = m2 if self.var.no_clamp else np.minimum(np.maximum(m2, self.mn2), self.mx2)
        return np.where(low, LD(1), mc), low

    def one_pass(self, u, S, er=None, ei=None, force_low=None):
        """One pass from voltages u [n, M] known to (er, ei) per component
        (None: exact inputs), S = powers(...).  Bounds: the module's docstring.
        force_low = (mask [n, M], value): the band decision at vlow of the
        masked entries is `value`, not the longdouble comparison's."""
        cr, ci, sar, sai = S
        M = self.p.M
        ur, ui = u.real, u.imag
        aur, aui = np.abs(ur).astype(float), np.abs(ui).astype(float)
        mc, low = self.gain(ur * ur + ui * ui, force_low)
        g = 1 / mc
        I = (cr + 1j * ci) * u * g
        gf = g.astype(float)
        Ar, Ai = gf * (sar * aur + sai * aui), gf * (sar * aui + sai * aur)
        if er is None:
            dI = np.zeros_like(Ar)
        else:
            dI = np.hypot(cr, ci).astype(float) * gf * np.hypot(er, ei) * (1 + 1e-6)
        Pre = np.abs(self.u0r) + Ar @ self.aWr.T + Ai @ self.aWi.T
        Pim = np.abs(self.u0r) + np.abs(self.u0i) + (Ar + Ai) @ (self.aWr + self.aWi).T
        prop = dI @ self.aW.T
        return dict(u=self.u0 + I @ self.W.T, I=I, Ar=Ar, Ai=Ai, dI=dI,
                    er=(M + 14) * U53 * Pre + prop, ei=(2 * M + 33) * U53 * Pim + prop)

    def rows(self, ps):
        """(V complex [n, n_out], bound of |V|) from a pass's currents."""
        M = self.p.M
        V = self.V0 + ps["I"] @ self.G.T
        Ar, Ai = ps["Ar"], ps["Ai"]
        evr = U53 * ((2 * M + 1) * np.abs(self.p.V0.real) + (2 * M + 13) * (Ar @ self.aGr.T + Ai @ self.aGi.T))
        evi = U53 * ((2 * M + 1) * np.abs(self.p.V0.imag) + (2 * M + 13) * (Ai @ self.aGr.T + Ar @ self.aGi.T))
        return V, np.hypot(evr, evi) + ps["dI"] @ self.aG.T + 2 * U53 * np.abs(V).astype(float)

    def knife(self, u, skip=None):
        """[n]: some element (but those of `skip` [n, M]) within KNIFE (rel, of |u|) of vlow."""
        m2 = (u.real * u.real + u.imag * u.imag).astype(float)
        near = np.abs(m2 / self.lo2.astype(float) - 1.0) < 2 * KNIFE
        return (near if skip is None else near & ~skip).any(1)

    def signature(self, u):
        """(sig [n] int32 as pgw_pf_tables.sig_out, near [n]: some element's
        |u| within KNIFE of one of its three limits)."""
        m2 = u.real * u.real + u.imag * u.imag
        b = (m2 > self.lo2).astype(np.int64) + (m2 > self.mn2) + (m2 > self.mx2)
        sig = (b << (2 * np.arange(self.p.M))).sum(1)
        near = np.zeros(len(u), bool)
        for t in (self.lo2, self.mn2, self.mx2):
            near |= (np.abs(m2.astype(float) / t.astype(float) - 1.0) < 2 * KNIFE).any(1)
        return sig.astype(np.uint32).view(np.int32), near

    def solve(self, n, ctrl_p=None, ctrl_q=None, ls=None, tol=0.0, max_iter=1, U_init=None, e_init=None,
              force_low=None):
        """The header's iteration, every env on its own (a stopped env keeps
        its state).  Returns u, er, ei, V, ev, vmin / vmax (over the rows in
        order), iters (-count where the cap stopped an env that never passed
        the test), sig, excluded [n] (knife edges; sig_near: for sig_out alone).
        force_low: see one_pass (the first pass only; those entries are no knife edges)."""
        p = self.p
        S = self.powers(n, ctrl_p, ctrl_q, ls)
        if U_init is None:
            u = np.tile(self.u0, (n, 1))
        else:
            u = U_init[:n].astype(CLD)
        er = np.zeros((n, p.M)) if e_init is None else np.array(e_init[0][:n], float)
        ei = np.zeros((n, p.M)) if e_init is None else np.array(e_init[1][:n], float)
        excluded = np.zeros(n, bool)
        active = np.ones(n, bool)
        iters = np.zeros(n, int)
        conv_ok = np.zeros(n, bool)
        last = None
        for it in range(1, max_iter + 1):
            fl = force_low if it == 1 else None
            ps = self.one_pass(u, S, er, ei, fl)
            excluded |= active & self.knife(u, None if fl is None else fl[0])
            err = np.abs(ps["u"] - u).max(1)
            conv = err < tol                              # max_k |du_k|^2 < tol^2, strict
            if tol > 0:
                # undecidable: within KNIFE_TOL of tol, or within the two iterates' own error of it
                slack = 2 * SQRT2 * (np.maximum(ps["er"], ps["ei"]).max(1) + np.maximum(er, ei).max(1))
                e = err.astype(float)
                excluded |= active & ((np.abs(e / tol - 1.0) < KNIFE_TOL) | (np.abs(e - tol) <= slack))
            if last is None:
                last = {k: v.copy() for k, v in ps.items()}
            else:
                for k, v in ps.items():
                    last[k][active] = v[active]
            a2 = active[:, None]
            u = np.where(a2, ps["u"], u)
            er, ei = np.where(a2, ps["er"], er), np.where(a2, ps["ei"], ei)
            iters[active] = it
            conv_ok |= active & conv
            active &= ~conv
            if not active.any():
                break
        if self.var.rows_from_final:                      # (wrong on purpose: currents of the final voltages)
            last = self.one_pass(u, S, er, ei)
        V, ev = self.rows(last)
        sig, near = self.signature(u)
        out = dict(u=u, er=er, ei=ei, V=V, ev=ev, iters=np.where(conv_ok, iters, -iters), excluded=excluded,
                   sig=sig, sig_near=near, I=last["I"])
        mag = np.abs(V)
        if p.n_out:
            out["vmin"], out["vmax"] = mag.min(1), mag.max(1)
        return out


# ---------------------------------------------------------------- the GPU test's cases
NS = (1, 63, 64, 65, 255, 256, 257, 520)

Case = collections.namedtuple("Case", "M m_true n_out n_ctrl band power_scale start tol max_iter use_p use_q use_ls")


def case(inst=None, **kw):
    M, band, n_ctrl, n_out = INST[inst] if inst else (None, "each", 2, 5)
    d = dict(M=M, m_true=None, n_out=n_out, n_ctrl=n_ctrl, band=band, power_scale=1.0, start="placement",
             tol=0.0, max_iter=1, use_p=True, use_q=True, use_ls=False)
    d.update(kw)
    if d["m_true"] is None:
        d["m_true"] = d["M"]
    return Case(**d)


def case_problem(c):
    return problem(c.M, c.m_true, c.n_out, c.n_ctrl, c.band, c.power_scale)


def case_inst(c):
    return case_problem(c).inst(c.use_ls)


def case_inputs(c):
    """(ctrl_p, ctrl_q, load_scale, U_init) over N_REF envs; None where the call passes NULL."""
    cp, cq = ctrl_powers(c.power_scale)
    band = c.band if c.m_true == c.M else "each"          # (a placement exists per (M, band) of full problems)
    return (cp[:c.n_ctrl] if c.use_p and c.n_ctrl else None, cq[:c.n_ctrl] if c.use_q and c.n_ctrl else None,
            load_scale() if c.use_ls else None, placement(c.M, band) if c.start == "placement" else None)


@functools.lru_cache(maxsize=None)
def median_iters(c):
    """The reference's median count of the run to CONV_TOL of this case's problem."""
    r = reference(c._replace(start="u0", tol=CONV_TOL, max_iter=CONV_MAX_ITER))
    assert (r["iters"] > 0).all()
    return int(np.median(r["iters"]))


@functools.lru_cache(maxsize=None)
def reference(c):
    """The reference of a case over N_REF envs (shared, read-only).
    max_iter "median": median_iters(c)."""
    if c.max_iter == "median":
        c = c._replace(max_iter=median_iters(c))
    cp, cq, ls, U = case_inputs(c)
    r = Ref(case_problem(c)).solve(N_REF, cp, cq, ls, c.tol, c.max_iter, U_init=U)
    r["max_iter"] = c.max_iter
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


ONE_PASS = [(inst, n) for inst in INST for n in NS]

# k passes and convergence: (inst, mode, n)
K_MODES = ("k2", "k3", "conv", "median")


def k_case(inst, mode):
    if mode in ("k2", "k3"):
        return case(inst, max_iter=int(mode[1]))
    return case(inst, start="u0", tol=CONV_TOL, max_iter=CONV_MAX_ITER if mode == "conv" else "median")


K_PASS = [(inst, mode, n) for inst in INST for mode in K_MODES for n in (520, 65)]

# sizes and padding: (M, m_true, band); M = 14 with n_ctrl = 1, so that the
# padding's band runs <14,T,F,T> and a moved one <14,F,T,T>
SIZES = [(M, mt, band) for M, mts in ((8, (1, 5, 8)), (14, (9, 13, 14)), (16, (15, 16))) for mt in mts
         for band in (("pad", "moved") if mt < M else ("each",))]


def size_case(M, m_true, band, mode):
    c = case(M=M, m_true=m_true, band=band, n_ctrl=1 if M == 14 else 2, n_out=5)
    return c if mode == "one" else c._replace(start="u0", tol=CONV_TOL, max_iter=CONV_MAX_ITER)


# slots and scale: (M, n_ctrl, which of ctrl_p / ctrl_q are passed, load_scale passed)
# (M = 8 with 8 slots: slot 0 takes two of the 8 elements, slots 1 .. 6 one each, slot 7 none -- its
# ctrl_p / ctrl_q rows are read and must change nothing)
SLOTS = [(M, nc, pq, ls) for M in (8, 14, 16) for nc in (0, 1, 2, 8)
         for pq in (("pq", "p", "q") if nc else ("none",)) for ls in (False, True)]


def slot_case(M, n_ctrl, pq, ls):
    return case(M=M, band="pad" if M == 14 else "each", n_ctrl=n_ctrl, n_out=5, use_p="p" in pq, use_q="q" in pq,
                use_ls=ls)


def n_outs(M):
    e = last_lds_rows(M)
    return (0, 1, 2, 3, 4, 5, 6, 9, e, e + 1)


# output rows: (inst family, n_out); "m14-T" is <14,T,F,F> up to one row and <14,T,F,T> beyond
ROW_FAMILIES = collections.OrderedDict([("m8-FTT", "m8-FTT"), ("m14-T", "m14-TFT"), ("m14-FTT", "m14-FTT"),
                                        ("m16-FTT", "m16-FTT")])
ROWS = [(fam, no) for fam in ROW_FAMILIES for no in n_outs(INST[ROW_FAMILIES[fam]][0])]


def row_case(fam, n_out):
    return case(ROW_FAMILIES[fam], n_out=n_out, start="u0", tol=CONV_TOL, max_iter=3)


def dup_positions(n_out):
    return sorted({1, 2, 3, 4, 5, n_out - 1})


def all_cases():
    """Every (label, Case, n) whose reference a GPU test compares against."""
    out = [("one-pass %s" % inst, case(inst), n) for inst, n in ONE_PASS]
    out += [("%s %s" % (mode, inst), k_case(inst, mode), n) for inst, mode, n in K_PASS]
    out += [("size M%d m%d %s %s" % (M, mt, band, mode), size_case(M, mt, band, mode), 257)
            for M, mt, band in SIZES for mode in ("one", "conv")]
    out += [("slots M%d c%d %s ls%d" % s, slot_case(*s), 257) for s in SLOTS]
    out += [("rows %s nout%d" % r, row_case(*r), 257) for r in ROWS]
    out += [("f32 %s" % inst, k_case(inst, "median"), 257) for inst in INST]
    return out


# ---------------------------------------------------------------- the predictor
PRED_P = (3, 4, 9)
PRED_TABLES = 3


@functools.lru_cache(maxsize=None)
def pred_grid(M, P, seed=0):
    """U_grid [PRED_TABLES, P, M] complex: smooth in the grid index plus noise."""
    rng = np.random.default_rng(600 + 17 * M + P + seed)
    j = np.arange(P)[None, :, None]
    a, b, c = (rng.uniform(0.9, 1.1, (PRED_TABLES, 1, M)) * np.exp(2j * np.pi * rng.random((PRED_TABLES, 1, M)))
               for _ in range(3))
    U = a + 0.01 * b * j + 0.001 * c * j * j + 1e-4 * rng.normal(size=(PRED_TABLES, P, M))
    U.setflags(write=False)
    return U


def pred_records_numpy(U):
    """pgw_pf_pred_pack restated in NumPy for one table U [P, M]: (u fp64 [P, M]
    complex, d1, d2 fp32 [P, M, 2]).  Centred differences about cj = clamp(j, 1,
    P - 2); a record at an end re-centres: d1 = (up - um) + s 2 (up - 2 u0 + um),
    s = j - cj, so that u_j + t d1/2 + t^2 d2/2 is the quadratic of cj at t + s.
    float64 arithmetic in the kernel's order, then one rounding to fp32."""
    P, M = U.shape
    d1 = np.zeros((P, M, 2), np.float32)
    d2 = np.zeros((P, M, 2), np.float32)
    for j in range(P):
        cj = min(max(j, 1), P - 2)
        s = float(j - cj)
        for c, part in enumerate((U.real, U.imag)):
            um, u0, up = part[cj - 1], part[cj], part[cj + 1]
            sec = (up - 2.0 * u0) + um
            d1[j, :, c] = ((up - um) + (s * 2.0) * sec).astype(np.float32)
            d2[j, :, c] = sec.astype(np.float32)
    return U.copy(), d1, d2


def pred_unpack(rec, P, M):
    """Records (bytes of pgw_pf_pred_pack's output for one table) -> (u, d1, d2)."""
    raw = np.frombuffer(rec, np.uint8).reshape(P, 32 * M)
    u = raw[:, :16 * M].copy().view(np.complex128).reshape(P, M)
    d1 = raw[:, 16 * M:24 * M].copy().view(np.float32).reshape(P, M, 2)
    d2 = raw[:, 24 * M:].copy().view(np.float32).reshape(P, M, 2)
    return u, d1, d2


def pred_quadratic(u, d1, d2, c, g):
    """The record's quadratic at grid coordinate g [n] in longdouble: u_c + t
    (d1/2 + t d2/2), t = g - c; and a componentwise bound of the kernel's
    evaluation of it (t one rounding, h2 = 0.5 t t one, two fmas: 4u of the
    terms' magnitudes; g itself is passed in as the kernel's own double)."""
    t = g.astype(LD) - c
    D1 = d1[c].astype(LD)
    D2 = d2[c].astype(LD)
    uc = u[c]
    re = uc.real.astype(LD) + t[:, None] * (D1[..., 0] / 2 + t[:, None] * D2[..., 0] / 2)
    im = uc.imag.astype(LD) + t[:, None] * (D1[..., 1] / 2 + t[:, None] * D2[..., 1] / 2)
    at = np.abs(t).astype(float)[:, None]
    er = 4 * U53 * (np.abs(uc.real) + at * np.abs(d1[c][..., 0]) / 2 + at * at * np.abs(d2[c][..., 0]) / 2)
    ei = 4 * U53 * (np.abs(uc.imag) + at * np.abs(d1[c][..., 1]) / 2 + at * at * np.abs(d2[c][..., 1]) / 2)
    return re + 1j * im, er, ei


def meta_reference(P, M, U, S, vlow, vmin, vmax):
    """pgw_pf_pred_meta restated from the comment above k_pf_pred_meta for one
    table (U [P, M] complex, S [P] signatures): list of (left, right, tstar)
    per segment, tstar by a longdouble Newton (the kernel's 8 steps) on the same quadratic."""
    def same(a, sg):
        return a >= 0 and a + 2 <= P - 1 and S[a] == sg and S[a + 1] == sg and S[a + 2] == sg

    out = []
    for j in range(P - 1):
        left, right, ts = max(0, min(j - 1, P - 3)), max(0, min(j, P - 3)), LD(0.5)
        s0, s1 = int(S[j]), int(S[j + 1])
        if s0 == s1:
            # both sides: the nearest 3-point stencil of that signature around the segment
            for q in (j + 1, j - 2, j, j - 1):            # (later wins: j - 1 is preferred for the left)
                if same(q, s0):
                    left = q
            for q in (j - 2, j + 1, j - 1, j):
                if same(q, s0):
                    right = q
        else:
            have_left = False
            for q in (j - 2, j - 3):
                if same(q, s0):
                    left, have_left = q, True
                    break
            for q in (j + 1, j + 2):
                if same(q, s1):
                    right = q
                    break
            for k in range(M):
                b0, b1 = (s0 >> (2 * k)) & 3, (s1 >> (2 * k)) & 3
                if b0 == b1:
                    continue
                lim = (vlow, vmin, vmax)[min(b0, b1)][k]
                thr = LD(lim) * LD(lim)
                m0, m1 = (LD(U[j + i, k].real) ** 2 + LD(U[j + i, k].imag) ** 2 for i in (0, 1))
                ts = min(max((thr - m0) / (m1 - m0), LD(0)), LD(1)) if m1 != m0 else LD(0.5)
                c = (left if have_left else right) + 1
                um, u0, up = (U[c + i, k] for i in (-1, 0, 1))
                d1 = (CLD(up) - CLD(um)) / 2
                d2 = (CLD(up) - 2 * CLD(u0) + CLD(um)) / 2
                for _ in range(8):
                    tau = LD(j - c) + ts
                    uu = CLD(u0) + tau * (d1 + tau * d2)
                    du = d1 + 2 * tau * d2
                    f = uu.real ** 2 + uu.imag ** 2 - thr
                    fp = 2 * (uu.real * du.real + uu.imag * du.imag)
                    if fp == 0:
                        break
                    ts = ts - f / fp
                ts = min(max(ts, LD(0)), LD(1))
                break
        out.append((left + 1, right + 1, ts))
    return out


# ---------------------------------------------------------------- the predictor's solve cases
PRED_M, PRED_POINTS, PRED_N = 14, 9, 257
PRED_X0, PRED_H = -0.9e-3, 0.3e-3


def sig_of(U, p):
    """Band signatures (pgw_pf_tables.sig_out's layout) of grid voltages U [..., M] in float64."""
    m2 = U.real ** 2 + U.imag ** 2
    b = (m2 > p.vlow ** 2).astype(np.int64) + (m2 > p.vmin ** 2) + (m2 > p.vmax ** 2)
    return (b << (2 * np.arange(p.M))).sum(-1).astype(np.uint32).view(np.int32)


def meta_tables(M, P=PRED_POINTS):
    """Hand-made grids [3, P, M] for pgw_pf_pred_meta (band 0.5 / 0.95 / 1.05):
    table 0 -- element 0 crosses vmin between points 3 and 4: a switch with a
    left and a right stencil, equal-signature segments whose stencil starts at
    j - 1 (left) / j (right), at j (the first segment) and at j - 1 for both
    (the last); table 1 -- element 1 crosses vmax between points 1 and 2: a
    switch without a left stencil (Newton on the right one); table 2 -- element
    0 crosses vlow, vmin and vmax in three consecutive segments and back: no
    matching stencil on either side (the plain ones)."""
    rng = np.random.default_rng(12 + M)
    j = np.arange(P)
    U = np.tile(1.0 * np.exp(2j * np.pi * rng.random(M))[None, None, :], (3, P, 1)).astype(complex)
    ph = np.exp(0.02j * j)
    U[0, :, 0] = (0.9065 + 0.0101 * j + 0.0003 * j * j) * ph
    U[1, :, 1] = (1.0213 + 0.0187 * j - 0.0004 * j * j) * ph
    mags = np.array([0.43, 0.47, 0.71, 0.97, 1.09, 1.01, 0.93, 0.47, 0.45])
    U[2, :, 0] = mags[:P] * ph
    return U


def pred_problem(n_out):
    """<14,T,F,F> (n_out = 1) and <14,T,F,T> (2) on the same block."""
    p1 = problem(PRED_M, PRED_M, 1, 1, "pad")
    if n_out == 1:
        return p1
    extra = problem(PRED_M, PRED_M, 2, 1, "pad")
    return p1.copy(G=np.vstack([p1.G, extra.G[1:]]), V0=np.concatenate([p1.V0, extra.V0[1:]]))


def pred_case(with_meta, records, tstar, lr):
    """The predictor's solve case on meta_tables' table 0 (its switch segment
    has a tstar off 1/2): envs at record centres, segment ends, either side
    of tstar and of 1/2, and outside the grid.  records = (u, d1, d2) of the
    packed table, tstar [P - 1], lr [P - 1, 2] its meta (the device's on the
    GPU; pred_records_numpy's and meta_reference's without one).  Returns
    ctrl_p [1, n], ctrl_q [1, n], the record c [n] the kernel must pick, and
    the start with its bounds (pred_quadratic)."""
    P, n = PRED_POINTS, PRED_N
    g = []
    for jj in range(P - 1):
        for t in (0.0, 1e-9, tstar[jj] - 1e-9, tstar[jj] + 1e-9, 0.5 - 1e-9, 0.5 + 1e-9, 1.0 - 1e-9, 0.3, 0.8):
            g.append(jj + t)
    g += [float(P - 1), -0.4, -1.7, P - 1 + 0.6, P + 1.2]
    rng = np.random.default_rng(3)
    g = np.array(g + list(rng.uniform(-1.0, P, n - len(g))))[:n]
    pc = PRED_X0 + g * PRED_H
    cq = ctrl_powers()[1][:1, :n]
    # the kernel's own grid coordinate and stencil choice, in the same double arithmetic
    gk = (pc - PRED_X0) * (1.0 / PRED_H)
    if with_meta:
        js = np.clip(np.floor(gk), 0, P - 2).astype(int)
        c = np.where(gk - js < tstar[js], lr[js, 0], lr[js, 1])
        # (a choice is decidable: no env within 1e-12 of its segment's tstar)
        assert (np.abs((gk - js) - tstar[js]) > 1e-12).all()
    else:
        c = np.clip(np.rint(gk), 1, P - 2).astype(int)
        assert (np.abs(np.abs(gk - np.floor(gk)) - 0.5) > 1e-12).all()
    start, er, ei = pred_quadratic(records[0], records[1], records[2], c, gk)
    return pc[None, :], cq, c, start, er, ei


def pred_host_meta():
    """(records, tstar, lr) of table 0 from the host restatements alone."""
    p = pred_problem(1)
    U = meta_tables(PRED_M)[0]
    want = meta_reference(PRED_POINTS, PRED_M, U, sig_of(U, p), p.vlow, p.vmin, p.vmax)
    return (pred_records_numpy(U), np.array([float(w[2]) for w in want]),
            np.array([[w[0], w[1]] for w in want], np.int32))


def pred_reference(with_meta, records, tstar, lr):
    cp, cq, c, start, er, ei = pred_case(with_meta, records, tstar, lr)
    r = Ref(pred_problem(1)).solve(PRED_N, cp, cq, None, 0.0, 1, U_init=start, e_init=(er, ei))
    return cp, cq, c, r


# ---------------------------------------------------------------- |u|^2 == vlow^2 exactly
def equality_case(inst):
    """The placement of `inst` with, in env e, element e % M at u = (vlow, 0):
    fma(0, 0, vlow * vlow) is the packed vlow^2 bit for bit, so the kernel's
    `m2 <= vlo2` holds there and `m2 < vlo2` would not -- decidable on the
    device, not by the longdouble comparison (vlow^2 rounds differently in 64
    bits), so the reference is told (force_low).  Returns (Case, U_init, mask)."""
    c = case(inst)
    U = np.array(case_inputs(c)[3])
    p = case_problem(c)
    e = np.arange(N_REF)
    mask = np.zeros((N_REF, c.M), bool)
    mask[e, e % c.M] = True
    U[mask] = p.vlow[e % c.M] + 0j
    return c, U, mask


def equality_reference(inst, low=True):
    """low = False: the strict reading `<` (for the sensitivity test)."""
    c, U, mask = equality_case(inst)
    cp, cq, ls, _ = case_inputs(c)
    return Ref(case_problem(c)).solve(N_REF, cp, cq, ls, 0.0, 1, U_init=U,
                                      force_low=(mask, np.full(mask.shape, low)))


# ---------------------------------------------------------------- references built outside Case
def one_slot_moved():
    """test_one_slot_as_s0_plus_f_pc_and_per_lane's second problem: slot_case(14, 1) with
    element 13's band moved, so that it runs <14,F,T,T>."""
    c = slot_case(14, 1, "pq", False)
    q = case_problem(c).with_band(13, 0.61, 0.94, 1.06)
    cp, cq, _, U = case_inputs(c)
    return c, q, Ref(q).solve(N_REF, cp, cq, None, 0.0, 1, U_init=U)


def extra_references():
    """(label, reference, n) of the GPU file's comparisons that are no Case,
    with the host restatements standing in for the device's predictor tables."""
    rec, tstar, lr = pred_host_meta()
    out = [("one slot, band moved", one_slot_moved()[2], 257),
           ("n_ctrl = 2 ignores U_pred", reference(case("m14-FTT", start="u0")), PRED_N)]
    out += [("predictor %s" % ("meta" if m else "nearest"), pred_reference(m, rec, tstar, lr)[3], PRED_N)
            for m in (False, True)]
    out += [("vlow itself %s" % inst, equality_reference(inst), 257) for inst in INST]
    return out
