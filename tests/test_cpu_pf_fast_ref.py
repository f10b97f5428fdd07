"""The inputs and the reference of tests/test_gpu_pf_fast_direct.py do what
they claim (tests/_pf_fast_direct_common.py; no GPU, libpgw's host functions
only): the placed voltages reach all four bands and both sides of every
element's own limits; a band read from the neighbouring element, a limit one
probe off, the strict comparison at |u|^2 == vlow^2 itself, vmin / vmax exchanged, no clamp, a dropped slot, nph ignored, rows
from the final voltages or W'' transposed each move some component by more
than 1e4 times the bound the kernel is held to; a float64 evaluation of the
same pass stays inside that bound; every case the GPU file runs loses at most
1 % of its envs to knife edges; pgw_pf_pack is held to longdouble entry by
entry; pgw_pf_padded_m; and pgw_pf_solve / _f32 refuse bad shapes before any
launch (n = 0).
"""
import ctypes

import numpy as np
import pytest

from tests import _pf_fast_direct_common as C

pytestmark = pytest.mark.skipif(not C.have_longdouble(), reason="np.longdouble has no 63-bit mantissa here")
SIZES = (8, 14, 16)


def _setup(M, band="each", variant=None, n_ctrl=2, W=None):
    p = C.problem(M, M, 5, n_ctrl, band)
    ref = C.Ref(p, variant, W=W)
    cp, cq = C.ctrl_powers()
    return p, ref, cp[:n_ctrl], cq[:n_ctrl], C.placement(M, band)


# ---------------------------------------------------------------- placement
@pytest.mark.parametrize("band", ["each", "pad"])
@pytest.mark.parametrize("M", SIZES)
def test_placement_reaches_every_band_and_both_sides_of_every_limit(M, band):
    p, ref, _, _, U = _setup(M, band)
    sig, near = ref.signature(U.astype(C.CLD))
    assert not near.any()
    b = (sig.view(np.uint32)[:, None] >> (2 * np.arange(M))[None, :]) & 3
    for k in range(M):
        for lvl in range(4):
            assert (b[:, k] == lvl).mean() >= 0.02, (M, k, lvl)
        v2 = np.abs(U[:, k]) ** 2
        for t in (p.vlow[k], p.vmin[k], p.vmax[k]):
            r = v2 / t ** 2 - 1.0
            assert ((r > 0) & (r < 3 * C.EDGE)).any() and ((r < 0) & (r > -3 * C.EDGE)).any(), (M, k, t)
    if band == "each":
        for a in (p.vlow, p.vmin, p.vmax, ):
            assert len(np.unique(a)) == M
        assert len(np.unique(p.vbase)) > 1 and len(np.unique(p.nph)) > 1
        assert (p.base_kw < 0).any() and (p.base_kw > 0).any()
    assert sorted(np.bincount(p.elem_ctrl[p.elem_ctrl >= 0]).tolist()) == [1, 2]


# ---------------------------------------------------------------- sensitivity
WRONG = {
    "band of element k + 1": dict(variant=C.Variant(roll=True)),
    "vlow one probe up": dict(variant=C.Variant(shift=("vlow", 1.0 + 2 * C.EDGE))),
    "vlow one probe down": dict(variant=C.Variant(shift=("vlow", 1.0 - 2 * C.EDGE))),
    "vmin and vmax exchanged": dict(variant=C.Variant(swap=True)),
    "g not clamped": dict(variant=C.Variant(no_clamp=True)),
    "slot 0 dropped": dict(variant=C.Variant(drop_slot=0)),
    "slot 1 dropped": dict(variant=C.Variant(drop_slot=1)),
    "nph ignored": dict(variant=C.Variant(no_nph=True)),
    "rows from the final voltages": dict(variant=C.Variant(rows_from_final=True), rows=True),
}


@pytest.mark.parametrize("name", list(WRONG))
@pytest.mark.parametrize("M", SIZES)
def test_a_wrong_reading_exceeds_the_bound_by_1e4(M, name):
    w = WRONG[name]
    p, ref, cp, cq, U = _setup(M)
    _, bad, _, _, _ = _setup(M, variant=w["variant"])
    k = 2 if w.get("rows") else 1                 # (one pass: the rows' currents are the starting ones either way)
    a = ref.solve(C.N_REF, cp, cq, None, 0.0, k, U_init=U)
    b = bad.solve(C.N_REF, cp, cq, None, 0.0, k, U_init=U)
    d = a["u"] - b["u"]
    ratio = max(float((np.abs(d.real) / a["er"]).max()), float((np.abs(d.imag) / a["ei"]).max()),
                float((np.abs(np.abs(a["V"]) - np.abs(b["V"])) / a["ev"]).max()))
    assert ratio >= 1e4, (M, name, ratio)


@pytest.mark.parametrize("inst", list(C.INST))
def test_the_strict_reading_at_vlow_exceeds_the_bound_by_1e4(inst):
    """`<=` against `<` at vlow differs only at |u|^2 == vlow^2 exactly, which
    the knife-edge rule leaves out of every other case (and which longdouble
    cannot decide: vlow^2 rounds differently in 64 bits).  C.equality_case
    puts one element per env at u = (vlow, 0), where the float64 the kernel
    forms is the packed vlow^2 bit for bit; the reference is told the decision,
    and the strict one moves U_out far beyond the bound."""
    c, U, mask = C.equality_case(inst)
    p = C.case_problem(c)
    assert mask[:257].any(0).all() and (mask.sum(1) == 1).all()
    k = np.arange(C.N_REF) % c.M
    m2 = U[mask].imag * U[mask].imag + U[mask].real * U[mask].real     # (fma(0, 0, x) = x)
    L = C.block_layout(c.M)
    np.testing.assert_array_equal(m2, p.block()[L["lo2"] + k])
    a, b = C.equality_reference(inst), C.equality_reference(inst, low=False)
    d = a["u"] - b["u"]
    worst = np.maximum(np.abs(d.real) / a["er"], np.abs(d.imag) / a["ei"]).max(1)
    assert (worst >= 1e4).all(), (inst, float(worst.min()))


@pytest.mark.parametrize("M", SIZES)
def test_a_transposed_matrix_exceeds_the_bound_by_1e4(M):
    """On a W'' made non-symmetric (upper triangle x 1.5): the reference's
    u_i = u0_i + sum_k W''_ik I'_k against sum_k W''_ki I'_k."""
    p = C.problem(M, M, 5, 2)
    base = C.Ref(p)
    W = (base.Wr + 1j * base.Wi) * np.where(np.triu(np.ones((M, M)), 1) > 0, 1.5, 1.0)
    _, ref, cp, cq, U = _setup(M, W=W)
    _, bad, _, _, _ = _setup(M, W=W.T)
    a = ref.solve(C.N_REF, cp, cq, None, 0.0, 1, U_init=U)
    b = bad.solve(C.N_REF, cp, cq, None, 0.0, 1, U_init=U)
    d = a["u"] - b["u"]
    assert max(float((np.abs(d.real) / a["er"]).max()), float((np.abs(d.imag) / a["ei"]).max())) >= 1e4


# ---------------------------------------------------------------- the bound against a float64 evaluation
def _pass_f64(ref, u, S):
    """One pass in float64 in the kernel's form (3 multiplications; NumPy has
    no fma, so a few more roundings than the kernel's)."""
    cr, ci = S[0].astype(float), S[1].astype(float)
    ur, ui = u.real.copy(), u.imag.copy()
    m2 = ui * ui + ur * ur
    lo2, mn2, mx2 = (a.astype(float) for a in (ref.lo2, ref.mn2, ref.mx2))
    mc = np.where(m2 <= lo2, 1.0, np.minimum(np.maximum(m2, mn2), mx2))
    g = 1.0 / mc
    gr, gi = g * ur, g * ui
    ir, ii = cr * gr - ci * gi, cr * gi + ci * gr
    A = ref.u0r[None, :].repeat(len(u), 0)
    B = np.zeros_like(A)
    Cc = (ref.u0r + ref.u0i)[None, :].repeat(len(u), 0)
    Ws = ref.Wr + ref.Wi
    for k in range(ref.p.M):
        A = A + ref.Wr[:, k][None, :] * ir[:, k:k + 1]
        B = B + ref.Wi[:, k][None, :] * ii[:, k:k + 1]
        Cc = Cc + Ws[:, k][None, :] * (ir + ii)[:, k:k + 1]
    return (A - B) + 1j * ((Cc - A) - B), ir + 1j * ii


@pytest.mark.parametrize("band", ["each", "pad"])
@pytest.mark.parametrize("M", SIZES)
def test_a_float64_evaluation_stays_inside_the_bound(M, band):
    """Three passes from the placement in float64 against the propagated
    bound (knife edges left out): the derivation is not too tight for plain
    double arithmetic of the same form."""
    p, ref, cp, cq, U = _setup(M, band)
    S = ref.powers(C.N_REF, cp, cq, C.load_scale())
    r = ref.solve(C.N_REF, cp, cq, C.load_scale(), 0.0, 3, U_init=U)
    u = np.array(U)
    for _ in range(3):
        u, I = _pass_f64(ref, u, S)
    keep = ~r["excluded"]
    d = u.astype(C.CLD) - r["u"]
    worst = max(float((np.abs(d.real) / r["er"])[keep].max()), float((np.abs(d.imag) / r["ei"])[keep].max()))
    V = ref.p.V0[None, :] + I @ ref.p.G.T
    worst_v = float((np.abs(np.abs(V).astype(C.LD) - np.abs(r["V"])) / r["ev"])[keep].max())
    print("M %d %s: float64 error / bound: U %.3g, rows %.3g" % (M, band, worst, worst_v))
    assert 0 < worst <= 1.0 and 0 < worst_v <= 1.0


# ---------------------------------------------------------------- knife edges
def test_every_gpu_case_keeps_99_percent_of_its_envs():
    """On the reference alone, for every case and batch size of the GPU file:
    at most 1 % of the envs (none of a batch of fewer than 100) are knife edges,
    sig_out's own near-limit envs included."""
    seen = set()
    for label, c, n in C.all_cases():
        if (c, n) in seen:
            continue
        seen.add((c, n))
        r = C.reference(c)
        out = (r["excluded"] | r["sig_near"])[:n].sum()
        assert out <= 0.01 * n, (label, n, out)
    assert len(seen) >= 150
    # the comparisons that are no Case (the predictor's tables from the host restatements)
    extra = C.extra_references()
    assert len(extra) == 4 + len(C.INST)
    for label, r, n in extra:
        out = (r["excluded"] | r["sig_near"])[:n].sum()
        assert out <= 0.01 * n, (label, n, out)


def test_convergence_cases_mix_counts_and_the_cap_inside_a_wave():
    earlier = 0
    for inst in C.INST:
        r = C.reference(C.k_case(inst, "conv"))
        assert (r["iters"] > 0).all() and r["iters"].max() < C.CONV_MAX_ITER
        assert len(np.unique(r["iters"][:64])) >= 2, inst
        m = C.reference(C.k_case(inst, "median"))
        k = m["max_iter"]
        first = m["iters"][:64]
        # the cap and convergence in the same iteration (+k), earlier stops, and the cap alone (-k)
        assert (first == k).any() and (first == -k).any(), (inst, k)
        earlier += int(((first > 0) & (first < k)).any())
        np.testing.assert_array_equal(m["iters"] == k, r["iters"] == k)
        np.testing.assert_array_equal(m["iters"] == -k, r["iters"] > k)
    assert earlier >= 3


def test_every_instantiation_is_selected():
    for inst in C.INST:
        assert C.case_inst(C.case(inst)) == inst
    got = {C.case_inst(c) for _, c, _ in C.all_cases()}
    assert got == set(C.INST)
    # a moved band below the padding's runs the per-element read
    assert C.problem(14, 9, 5, 1, "moved").inst() == "m14-FTT" and C.problem(14, 9, 5, 1, "pad").inst() == "m14-TFT"
    assert C.problem(14, 14, 5, 1, "pad").inst(load_scale=True) == "m14-FTT"
    assert [C.last_lds_rows(M) for M in SIZES] == [128, 128, 85]


# ---------------------------------------------------------------- pgw_pf_pack
@pytest.mark.parametrize("band", ["each", "pad"])
@pytest.mark.parametrize("M", SIZES)
def test_pack_against_longdouble(M, band):
    from powergridworld_amd import _lib
    p = C.problem(M, M, 3, 2, band)
    blk, L = p.block(), C.block_layout(M)
    T = L["T"]
    assert _lib.lib().pgw_pf_pack_size(M) == len(blk) == L["size"] == 3 * M * (M + 1) // 2 + 8 * M + 2
    vb = p.vbase.astype(C.LD)
    # the triangle: every (i, k) of the full matrix reads entry i M - i (i - 1) / 2 + (k - i), i <= k
    # (every entry of W is distinct: a wrong index cannot pass)
    assert len(np.unique(p.W[np.triu_indices(M)])) == T
    for i in range(M):
        for k in range(M):
            a, b = min(i, k), max(i, k)
            e = a * M - a * (a - 1) // 2 + (b - a)
            want = p.W[i, k].astype(C.CLD) / (vb[i] * vb[k])
            wr, wi, ws = blk[e], blk[T + e], blk[2 * T + e]
            # 1 / (vb_i vb_k) (two roundings), then the product: 3 u, and a margin of 1
            assert abs(wr - want.real) <= 4 * C.U53 * abs(want.real), (i, k)
            assert abs(wi - want.imag) <= 4 * C.U53 * abs(want.imag), (i, k)
            assert ws == wr + wi, (i, k)                   # the 3-multiplication form's third part: one rounding
    u0 = p.U0.astype(C.CLD) / vb
    ur, ui, us = (blk[L[k]:L[k] + M] for k in ("u0re", "u0im", "u0sum"))
    assert (np.abs(ur - u0.real) <= C.U53 * np.abs(u0.real)).all()          # one division
    assert (np.abs(ui - u0.imag) <= C.U53 * np.abs(u0.imag)).all()
    np.testing.assert_array_equal(us, ur + ui)
    for name, v in (("lo2", p.vlow), ("mn2", p.vmin), ("mx2", p.vmax)):
        got = blk[L[name]:L[name] + M]
        np.testing.assert_array_equal(got, v * v)
        assert (np.abs(got - v.astype(C.LD) ** 2) <= C.U53 * got).all()
    np.testing.assert_array_equal(blk[L["g0re"]:L["g0re"] + M], p.G[0].real)      # row 0 verbatim
    np.testing.assert_array_equal(blk[L["g0im"]:L["g0im"] + M], p.G[0].imag)
    assert blk[L["v0re"]] == p.V0[0].real and blk[L["v0im"]] == p.V0[0].imag


def test_pack_without_rows_writes_a_zero_row():
    full = C.problem(8, 8, 3, 1)
    p = full.copy(G=np.zeros((0, 8), complex), V0=np.zeros(0, complex))
    blk, L = p.block(), C.block_layout(8)
    assert p.n_out == 0 and (blk[L["g0re"]:] == 0).all()
    np.testing.assert_array_equal(blk[:L["g0re"]], full.block()[:L["g0re"]])


def test_pack_refusals():
    p = C.problem(8, 8, 2, 1)

    def rc(prm=None, W=None, G0=p.G[0], V0=p.V0[:1]):
        return C.pack(prm or p.params(), p.W if W is None else W, p.U0, G0, V0, expect_ok=False)

    assert rc()[0] == 0
    W = p.W.copy()
    W[2, 5] *= 1.0 + 1e-9
    r, msg = rc(W=W)
    assert r != 0 and "not symmetric" in msg
    W = p.W.copy()
    W[2, 5] *= 1.0 + 1e-14                                # (rounding-level asymmetry is averaged, not refused)
    assert rc(W=W)[0] == 0
    for bad in (0.0, -120.0):
        prm = p.params()
        prm.vbase[3] = bad
        r, msg = rc(prm)
        assert r != 0 and "vbase[3]" in msg
    for m in (0, 7, 9, 13, 15, 17):
        prm = p.params()
        prm.m = m
        r, msg = rc(prm)
        assert r != 0 and "not padded" in msg, m
    r, msg = rc(G0=None)
    assert r != 0 and "row missing" in msg


def test_padded_m():
    from powergridworld_amd import _lib
    got = [_lib.lib().pgw_pf_padded_m(m) for m in range(1, 17)]
    assert got == [8] * 8 + [14] * 6 + [16] * 2 == [C.padded_m(m) for m in range(1, 17)]


# ---------------------------------------------------------------- pgw_pf_solve's refusals
@pytest.mark.parametrize("entry", ["pgw_pf_solve", "pgw_pf_solve_f32"])
def test_solve_refuses_bad_shapes_before_any_launch(entry):
    """n = 0: the checks run, nothing launches (no GPU needed), as
    test_cpu_host.py does for pgw_ma_step."""
    from powergridworld_amd import _lib
    lib = _lib.lib()
    fn = getattr(lib, entry)
    dummy = 256                                           # never dereferenced

    def call(block=dummy, G=dummy, V0=dummy, v_out=dummy, vmin=None, **kw):
        prm = C.problem(8, 8, 1, 1).params(1e-6, 5)
        for k, v in kw.items():
            setattr(prm, k, v)
        t = _lib.PFTables(block=block, G=G, V0=V0, v_min_out=vmin)
        r = fn(ctypes.byref(prm), ctypes.byref(t), 0, None, None, v_out, None, None)
        return r, lib.pgw_last_error().decode()

    assert call()[0] == 0
    assert call(v_out=None, vmin=dummy)[0] == 0           # extrema only
    assert call(n_out=0, G=None, V0=None, v_out=None)[0] == 0
    bad = [dict(m=m) for m in (0, 9, 15, 17)] + [dict(n_ctrl=c) for c in (-1, 9)] + \
          [dict(G=None), dict(V0=None), dict(v_out=None), dict(max_iter=0), dict(block=None)]
    for kw in bad:
        r, msg = call(**kw)
        assert r != 0 and msg.startswith("pgw_pf_solve"), (kw, r, msg)
    assert fn(None, None, 0, None, None, None, None, None) != 0
