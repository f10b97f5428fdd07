"""pgw_pf_solve_general called through the C ABI (csrc/pgw_pf_general.hip;
include/pgw.h, "General batched power flow") on synthetic problems, against
the np.longdouble restatement of u <- U0 + W I(u) in
tests/_pfg_direct_common.py.  Needs an MI355X.

Every (model, branch) cell of the load laws, per-element bands that all
differ, every instance of the kernel (CE 1 / 2 / 4 by m + n_reg, CN 1 / 2 / 4 /
8 by n_chk, REG on / off: the test ids name them), n_out 1 .. 41 (ld =
pad8(n_out) and the ragged last chunk) and batches of 1 .. 130 envs.
tests/test_cpu_pf_general_ref.py shows on the reference alone that a wrong
branch, threshold or element record would miss the bound by more than 1e4.

The bound B is derived in _pfg_direct_common (one pass: (2 mtot + 24) 2^-53
(|U0_i| + sum_k |W_ik| A_k) per component; k passes: propagated with the
currents' Lipschitz factors through |W|).  Largest error / B seen on the
MI355X over every env, row and component of a group's cases: one pass 0.178,
k passes 0.090, run to convergence 0.159, regulator columns 0.063 (each test's
docstring names its worst case); pow() of model 4 needed no allowance.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import _pfg_direct_common as C

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not C.have_longdouble(), reason="np.longdouble has no 63-bit mantissa here")]
DEV = "cuda:0"
SENTINEL = -1.2345e300           # what the outputs hold where the kernel must not store
ISENT = -777


def _dev(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _elems(p):
    from powergridworld_amd import _lib
    arr = (_lib.PFGElem * p.m)()
    for k in range(p.m):
        e = arr[k]
        e.base_kw, e.base_kvar, e.nph = p.base_kw[k], p.base_kvar[k], p.nph[k]
        e.y0r, e.y0i = p.y0r[k], p.y0i[k]
        e.vlo2, e.vmn2, e.vmx2, e.vcut2 = p.vlo2[k], p.vmn2[k], p.vmx2[k], p.vcut2[k]
        e.ctrl, e.model = int(p.ctrl[k]), int(p.model[k])
        e.exp_p, e.exp_q = p.exp_p[k], p.exp_q[k]
        for i in range(6):
            e.zip[i] = p.zip[k, i]
    return torch.tensor(np.frombuffer(bytes(arr), np.uint8).copy(), device=DEV)


def _launch(p, mode, n, tol, min_iter, max_iter, U_init=None, ctrl=None, active=None, reg=False):
    """One call on sentinel-filled outputs.  Every buffer's numel is held to
    the size pgw.h gives before the launch.  Returns a dict of host arrays."""
    from powergridworld_amd import _lib
    od = mode == C.PF_OPENDSS
    size = p.sizes(n)
    buf = {k: _dev(v) for k, v in p.tables().items()}
    if not od:
        buf.pop("Gc"), buf.pop("V0c")
    if U_init is not None:
        buf["U_init"] = _dev(np.ascontiguousarray(U_init[:n]).view(np.float64).ravel())
    if ctrl is not None:
        buf["ctrl_p"], buf["ctrl_q"] = _dev(ctrl[0][:, :n].ravel()), _dev(ctrl[1][:, :n].ravel())
    if active is not None:
        buf["env_active"] = _dev(active[:n], torch.int32)
    if reg:
        buf["Kreg"] = _dev(p.kreg(n).view(np.float64).ravel())
        for k in ("reg_x", "reg_c"):
            buf[k] = torch.full((size[k],), SENTINEL, dtype=torch.float64, device=DEV)
    for k in ("U_out", "v_min_out", "v_max_out", "v_out"):
        buf[k] = torch.full((size[k],), SENTINEL, dtype=torch.float64, device=DEV)
    buf["iters"] = torch.full((n,), ISENT, dtype=torch.int32, device=DEV)
    for k, t in buf.items():
        assert t.numel() == size[k] and t.is_contiguous(), (k, t.numel(), size[k])
    elem = _elems(p)
    assert elem.numel() == p.m * ctypes.sizeof(_lib.PFGElem)
    prm = _lib.PFGParams()
    prm.m, prm.n_chk, prm.n_out, prm.n_ctrl = p.m, p.n_chk if od else 0, p.n_out, p.n_ctrl
    prm.mode, prm.min_iter, prm.max_iter, prm.tol = mode, min_iter, max_iter, tol
    prm.coef, prm.rescale = p.coef, p.rescale
    if reg:
        prm.n_reg, prm.r_reg = p.n_reg, p.r_reg
    tb = _lib.PFGTables()
    tb.elem = elem.data_ptr()
    for k in ("W", "U0", "Gc", "V0c", "G", "V0", "U_init", "U_out", "v_min_out", "v_max_out", "Greg", "V0reg",
              "Kreg", "reg_x", "reg_c", "env_active", "reg_rho"):
        if k in buf:
            setattr(tb, k, buf[k].data_ptr())
    cp = buf["ctrl_p"].data_ptr() if ctrl is not None else None
    cq = buf["ctrl_q"].data_ptr() if ctrl is not None else None
    rc = _lib.lib().pgw_pf_solve_general(prm, tb, n, cp, cq, buf["v_out"].data_ptr(), buf["iters"].data_ptr(),
                                         _lib.stream_ptr(torch.device(DEV)))
    _lib.check(rc)
    torch.cuda.synchronize()
    out = {k: buf[k].cpu().numpy() for k in ("U_out", "v_min_out", "v_max_out", "v_out", "iters")}
    out["U_out"] = out["U_out"].view(np.complex128).reshape(n, p.m)
    out["v_out"] = out["v_out"].reshape(p.n_out, n)
    if reg:
        for k in ("reg_x", "reg_c"):
            out[k] = buf[k].cpu().numpy().view(np.complex128).reshape(p.r_reg, n)
    return out


def _ratio(err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(err == 0, 0.0, np.asarray(err, float) / bound)


def _compare(out, p, r, n, what, reg=False):
    """Every output of the n envs against the reference r (over N_REF envs),
    knife-edge envs left out; returns the largest error / bound.  U_out, reg_x
    and reg_c are held componentwise; v_out is held to the same figure of its
    row through | |a| - |b| | <= |a - b| (stricter than the sqrt2 the
    componentwise bound would allow a modulus)."""
    keep = ~r["excluded"][:n]
    assert keep.sum() >= 0.99 * n
    np.testing.assert_array_equal(out["iters"][keep], r["iters"][:n][keep], err_msg=what)
    for k in ("U_out", "v_out", "v_min_out", "v_max_out"):
        assert np.isfinite(out[k].view(np.float64)).all(), (what, k)
    d = out["U_out"].astype(C.CLD) - r["u"][:n]
    ru = np.maximum(_ratio(np.abs(d.real), r["e_u"][:n]), _ratio(np.abs(d.imag), r["e_u"][:n]))[keep]
    vr = np.abs(r["V"][:n])                                              # [n, n_out] longdouble
    rv = _ratio(np.abs(out["v_out"].T.astype(C.LD) - vr), r["e_v"][:n])[keep]
    # the extrema are the kernel's own rows' (bit for bit), so within the rows' bounds
    np.testing.assert_array_equal(out["v_min_out"], out["v_out"].min(0), err_msg=what)
    np.testing.assert_array_equal(out["v_max_out"], out["v_out"].max(0), err_msg=what)
    worst = [ru.max(), rv.max()]
    if reg:
        for k, ref, e in (("reg_x", r["x"], r["e_x"]), ("reg_c", r["c"], r["e_c"])):
            rr = p.r_reg
            d = out[k].T.astype(C.CLD) - ref[:n, :rr]
            worst.append(np.maximum(_ratio(np.abs(d.real), e[:n, :rr]), _ratio(np.abs(d.imag), e[:n, :rr]))[keep].max())
    print("%s: worst error / bound: U_out %.3g, v_out %.3g%s (%d envs, %d left out)"
          % (what, worst[0], worst[1], (", reg_x %.3g, reg_c %.3g" % tuple(worst[2:])) if reg else "",
             n, n - keep.sum()))
    assert max(worst) <= 1.0, (what, worst)
    return max(worst)


# ---------------------------------------------------------------- one pass
@pytest.mark.parametrize("case", C.ONE_PASS, ids=lambda c: C.case_id(*c))
def test_one_pass_vs_longdouble(case):
    """max_iter = min_iter = 1, tol = 0, U_init placed in every cell, ctrl_p /
    ctrl_q set: U_out, v_out and the extrema within B, iters == -1.  The
    controllable powers, and coef / rescale on model 1 alone, are the
    reference's (pgw.h's formula).  Largest error / B on the MI355X over the
    27 cases: 0.178 (m16-CE1-CN8-nout13-n63, U_out); at m = 128, 0.064."""
    m, mode, n_chk, n_out, n = case
    p, r = C.one_pass_reference(m, mode, n_chk, n_out)
    assert not r["excluded"].any() and (r["iters"] == -1).all()
    out = _launch(p, mode, n, 0.0, 1, 1, U_init=C.placement(m), ctrl=C.ctrl_powers())
    assert (out["iters"] == -1).all()
    _compare(out, p, r, n, C.case_id(*case))


# ---------------------------------------------------------------- k passes
@pytest.mark.parametrize("case", C.K_PASS, ids=lambda c: C.case_id(*c[:5]) + "-k%d" % c[5])
def test_k_passes_vs_longdouble(case):
    """max_iter = 2 or 3 from the same placement, the bound propagated pass by
    pass (Ref.one_pass: sum_k |W_ik| L_k sqrt2 e_k on top of that pass's B).
    Largest error / bound on the MI355X: 0.090 (m16, k = 2); 0.006 at m = 128, k = 3."""
    m, mode, n_chk, n_out, n, k = case
    p, r = C.k_pass_reference(m, mode, n_chk, n_out, k)
    out = _launch(p, mode, n, 0.0, 1, k, U_init=C.placement(m), ctrl=C.ctrl_powers())
    _compare(out, p, r, n, C.case_id(*case[:5]) + "-k%d" % k)


# ---------------------------------------------------------------- run to convergence
def _converge(case, active=None):
    m, mode, n_chk, n_out, n, size = case
    p, r = C.converge_reference(*case)
    U, cp, cq = C.conv_inputs(m, mode, size)
    if mode == C.PF_EXACT:
        out = _launch(p, mode, n, C.EXACT_TOL, 1, C.EXACT_MAX_ITER, U_init=U, ctrl=(cp, cq), active=active)
    else:
        out = _launch(p, mode, n, C.OD_TOL, C.OD_MIN_ITER, C.OD_MAX_ITER, ctrl=(cp, cq), active=active)
    return p, r, out


@pytest.mark.parametrize("case", C.CONVERGE, ids=lambda c: C.case_id(*c[:5]))
def test_run_to_convergence_vs_longdouble(case):
    """A contraction run to its stopping rule (EXACT tol 1e-10, at most 12;
    OPENDSS tol 1e-4, min 2, max 15), the controllable power sized per env so
    that the envs of a block stop at different iterations and some at the cap:
    iters equals the reference's count of the env run alone, negative exactly
    where unconverged, and the voltages are within the propagated bound -- a
    stopped env keeps its state while its block runs on.  Largest error /
    bound on the MI355X: 0.159 (m16-CE1-CN2, v_out); 0.119 EXACT (m32);
    no env left out."""
    p, r, out = _converge(case)
    _compare(out, p, r, case[4], C.case_id(*case[:5]))


# ---------------------------------------------------------------- env_active
@pytest.mark.parametrize("case", [C.CONVERGE[1], C.CONVERGE[4]], ids=lambda c: C.case_id(*c[:5]))
def test_env_active_leaves_masked_envs_untouched(case):
    """Masks that empty a whole block (envs 64 .. 127), leave a single lane
    of a block, and a random one: a masked env's outputs keep the sentinel bit
    for bit, an active env's are bit for bit those of the unmasked call."""
    n = case[4]
    p, r, full = _converge(case)
    rng = np.random.default_rng(5)
    masks = {"block-empty": np.where((np.arange(n) >= 64) & (np.arange(n) < 128), 0, 1),
             "single-lane": np.where(np.arange(n) == 70, 1, np.where(np.arange(n) < 128, 0, 1)),
             "random": (rng.random(n) < 0.5).astype(int)}
    for name, mask in masks.items():
        _, _, out = _converge(case, active=mask)
        on = mask != 0
        assert on.any() and (~on).any()
        for k in ("U_out", "v_out", "v_min_out", "v_max_out", "iters"):
            a, b = out[k], full[k]
            if k == "U_out":
                a, b = a.view(np.float64).reshape(n, -1).T, b.view(np.float64).reshape(n, -1).T
            a, b = np.atleast_2d(a), np.atleast_2d(b)                   # [rows, n]
            np.testing.assert_array_equal(a[:, on], b[:, on], err_msg="%s %s" % (name, k))
            sent = ISENT if k == "iters" else SENTINEL
            assert (a[:, ~on] == sent).all(), (name, k)


# ---------------------------------------------------------------- REG at full width
REG_M, REG_N = 104, 24                                      # m + n_reg = 128: CE = 4 with REG
REG_CASES = [(r_reg, form, n) for r_reg, n in ((1, 65), (23, 130), (24, 64))
             for form in ("uinit-exact", "direct-exact", "direct-CN4")]


@pytest.mark.parametrize("case", REG_CASES, ids=lambda c: "m104-CE4-REG1-r%d-%s-n%d" % c)
def test_regulator_columns_at_full_width_vs_longdouble(case):
    """m + n_reg = 128 with n_reg = 24 (the instance whose static LDS is just
    under the limit), r_reg = 1 / 23 / 24, a random symmetric K per env and
    reg_rho: x = V0reg + Greg J, c = K (rho x), every row over m + n_reg
    columns.  One pass from U_init (EXACT), and the direct-start form (no
    U_init: a first pass with J = 0) in both modes; reg_x / reg_c compared too.
    Largest error / bound on the MI355X: 0.063 (r23 from U_init, reg_x); U_out 0.059."""
    r_reg, form, n = case
    mode = C.PF_OPENDSS if form.endswith("CN4") else C.PF_EXACT
    direct = form.startswith("direct")
    n_chk = 72 if mode else 0
    p, r = C.one_pass_reference(REG_M, mode, n_chk, 13, REG_N, r_reg, direct)
    assert p.mtot == 128 and C.ce_of(p.mtot) == 4
    out = _launch(p, mode, n, 0.0, 1, 1, U_init=None if direct else C.placement(REG_M), ctrl=C.ctrl_powers(),
                  reg=True)
    assert (out["iters"] == -1).all()
    _compare(out, p, r, n, "REG r%d %s" % (r_reg, form), reg=True)


# ---------------------------------------------------------------- argument checks
def _bad_call(mutate):
    """A valid tiny call's arguments, mutated, on buffers large enough for any
    of the mutations (nothing may launch): (rc, message)."""
    from powergridworld_amd import _lib
    big = torch.zeros(1 << 18, dtype=torch.float64, device=DEV)
    prm = _lib.PFGParams()
    prm.m, prm.n_chk, prm.n_out, prm.n_ctrl = 8, 8, 1, 0
    prm.mode, prm.min_iter, prm.max_iter, prm.tol = C.PF_OPENDSS, 1, 1, 0.0
    prm.coef = prm.rescale = 1.0
    tb = _lib.PFGTables()
    for k in ("elem", "W", "U0", "Gc", "V0c", "G", "V0", "U_out", "Greg", "V0reg", "Kreg", "reg_x", "reg_c",
              "reg_rho"):
        setattr(tb, k, big.data_ptr())
    n = mutate(prm, tb, big)
    n = 1 if n is None else n
    before = big.clone()
    rc = _lib.lib().pgw_pf_solve_general(prm, tb, n, None, None, None, None, _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    msg = _lib.lib().pgw_last_error().decode()
    assert torch.equal(big, before)
    return rc, msg


def _set(**kw):
    def f(prm, tb, big):
        for k, v in kw.items():
            if k == "n":
                continue
            obj = prm if hasattr(prm, k) and k in dict(prm._fields_) else tb
            setattr(obj, k, big.data_ptr() if v == "ptr" else v)
        return kw.get("n")
    return f


BAD = {
    "m % 8": (_set(m=12), "m=12"),
    "m > 128": (_set(m=136), "m=136"),
    "n_chk % 8": (_set(n_chk=12), "n_chk"),
    "OPENDSS without Gc": (_set(Gc=None), "Gc"),
    "m + n_reg > 128": (_set(m=112, n_reg=24, r_reg=24, mode=C.PF_EXACT), "n_reg 24"),
    "r_reg > n_reg": (_set(n_reg=8, r_reg=9, mode=C.PF_EXACT), "r_reg 9"),
    "OPENDSS + U_init + regulators": (_set(n_reg=8, r_reg=2, U_init="ptr"), "U_init"),
    "n_out > 0 without G": (_set(G=None), "G / V0"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_argument_checks_return_an_error_that_names_the_argument(name):
    mutate, word = BAD[name]
    rc, msg = _bad_call(mutate)
    assert rc != 0, name
    assert "pgw_pf_solve_general" in msg and word in msg, (name, msg)


def test_zero_envs_is_ok_and_launches_nothing():
    rc, _ = _bad_call(_set(n=0))
    assert rc == 0
