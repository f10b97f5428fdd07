"""pgw_pf_solve_regulated called through the C ABI (k_pf_regulated<CE, CN> in
csrc/pgw_pf_general.hip; include/pgw.h, "The snap solve with controls in one
launch") on the synthetic regulated problems of
tests/_regloop_direct_common.py, the buffers the tests' own.  Needs an MI355X.

Two references.  (a) The host loop of the three stand-alone entries, written
here as OpenDSSSolver._solve_regulated composes them (pgw_pf_solve_general
over env_active, pgw_reg_control, pgw_reg_factor on the control's mask): bit
for bit, at every one of the 15 instantiations and with both factor shapes
(two envs per 64 lanes for r_reg <= 16, one above) per CE, n = 1, 65 and 130.
(b) The np.longdouble restatement of the loop from pgw.h's text: taps, passes
and iters equal, U_out, v_out, reg_x and reg_c within the propagated bound, on
six cases (each CE under either stopping rule) and four capped ones.
tests/test_cpu_regloop_ref.py shows on the reference alone that the cases
make the loop work and that a wrong reading of it would show.  (c) The loop's
edges against the host loop.

Every output buffer is sentinel-filled and exactly as long as pgw.h says, with
a guard tail that must come back untouched.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import _pfg_direct_common as C
from tests import _regloop_direct_common as R
from tests.test_gpu_pf_general_direct import _dev, _elems, _ratio

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not C.have_longdouble(), reason="np.longdouble has no 63-bit mantissa here")]
DEV = "cuda:0"
SENTINEL = -1.2345e300
ISENT = -777
GUARD = 64
F64_OUT = ("U_out", "v_min_out", "v_max_out", "v_out", "reg_x", "reg_c", "taps", "Kreg")
I32_OUT = ("iters", "passes")
BITS = F64_OUT + ("iters",)


class Ctx:
    """The device-side constants of one case at n envs: tables, parameters,
    the regulator record, the inputs (powers, U_init, starting taps [n_ctrl,
    n]) and the starting K of those taps (pgw_reg_factor)."""

    def __init__(self, case, n, max_iter=None, taps=None):
        from powergridworld_amd import _lib
        p = case.prob
        self.case, self.p, self.n = case, p, n
        od = case.mode == C.PF_OPENDSS
        self.size = size = dict(p.sizes(n), taps=case.n_ctrl * n, passes=n)
        self.const = {k: _dev(v) for k, v in p.tables().items()}
        if not od:
            self.const.pop("Gc"), self.const.pop("V0c")
        self.const["ctrl_p"], self.const["ctrl_q"] = _dev(case.cp[:, :n].ravel()), _dev(case.cq[:, :n].ravel())
        if case.U_init is not None:
            self.const["U_init"] = _dev(np.ascontiguousarray(case.U_init[:n]).view(np.float64).ravel())
        for k, t in self.const.items():
            assert t.numel() == size[k] and t.is_contiguous(), (k, t.numel(), size[k])
        self.elem = _elems(p)
        assert self.elem.numel() == p.m * ctypes.sizeof(_lib.PFGElem)
        self.S_rho = R._dev_S_rho(case.S, case.rho)
        assert self.S_rho[0].numel() == 2 * case.r_reg ** 2 and self.S_rho[1].numel() == case.r_reg
        self.rp = case.reg_params(self.S_rho[0].data_ptr(), self.S_rho[1].data_ptr())
        prm = _lib.PFGParams()
        prm.m, prm.n_chk, prm.n_out, prm.n_ctrl = p.m, p.n_chk if od else 0, p.n_out, p.n_ctrl
        prm.mode, prm.min_iter, prm.tol = case.mode, case.min_iter, case.tol
        prm.max_iter = max_iter or case.max_iter
        prm.coef, prm.rescale, prm.n_reg, prm.r_reg = p.coef, p.rescale, p.n_reg, p.r_reg
        self.prm = prm
        self.st = _lib.stream_ptr(torch.device(DEV))
        self.lib = _lib.lib()
        self.check = _lib.check
        taps = case.taps[:n].T if taps is None else taps
        self.taps0 = np.ascontiguousarray(taps, np.float64)                     # [n_ctrl, n]
        assert self.taps0.shape == (case.n_ctrl, n)
        K = torch.full((size["Kreg"],), SENTINEL, dtype=torch.float64, device=DEV)
        self.check(self.lib.pgw_reg_factor(self.rp, n, _dev(self.taps0).data_ptr(), None, K.data_ptr(), self.st))
        torch.cuda.synchronize()
        self.K0 = K.cpu().numpy()

    def outputs(self, taps=None, K=None):
        """Fresh sentinel-filled outputs with their guard tails; taps and Kreg
        hold the starting values."""
        out = {k: torch.full((self.size[k] + GUARD,), SENTINEL, dtype=torch.float64, device=DEV) for k in F64_OUT}
        for k in I32_OUT:
            out[k] = torch.full((self.size[k] + GUARD,), ISENT, dtype=torch.int32, device=DEV)
        out["taps"][:self.size["taps"]] = _dev((self.taps0 if taps is None else taps).ravel())
        out["Kreg"][:self.size["Kreg"]] = _dev(self.K0 if K is None else K)
        return out

    def tables(self, out, U_init="given"):
        from powergridworld_amd import _lib
        tb = _lib.PFGTables()
        tb.elem = self.elem.data_ptr()
        for k in ("W", "U0", "Gc", "V0c", "G", "V0", "Greg", "V0reg", "reg_rho"):
            if k in self.const:
                setattr(tb, k, self.const[k].data_ptr())
        for k in ("U_out", "v_min_out", "v_max_out", "Kreg", "reg_x", "reg_c"):
            setattr(tb, k, out[k].data_ptr())
        if U_init == "given" and "U_init" in self.const:
            tb.U_init = self.const["U_init"].data_ptr()
        return tb

    def harvest(self, out):
        """Host copies; the guard tails must hold the sentinel still."""
        torch.cuda.synchronize()
        res = {}
        for k, t in out.items():
            a = t.cpu().numpy()
            sent = ISENT if k in I32_OUT else SENTINEL
            assert (a[self.size[k]:] == sent).all(), "the guard tail of %s was written" % k
            res[k] = a[:self.size[k]].copy()
        return res


@pytest.fixture(scope="module")
def ctx_cache():
    cache = {}

    def get(cs, n=C.N_REF, max_iter=None):
        key = (cs, n, max_iter)
        if key not in cache:
            cache[key] = Ctx(R.case(*cs), n, max_iter)
        return cache[key]
    return get


def _device(ctx, max_passes, taps=None, K=None, want_passes=True):
    out = ctx.outputs(taps, K)
    tb = ctx.tables(out)
    ctx.check(ctx.lib.pgw_pf_solve_regulated(
        ctx.prm, tb, ctx.rp, ctx.n, ctx.const["ctrl_p"].data_ptr(), ctx.const["ctrl_q"].data_ptr(),
        out["taps"].data_ptr(), out["Kreg"].data_ptr(), max_passes, out["v_out"].data_ptr(),
        out["iters"].data_ptr(), out["passes"].data_ptr() if want_passes else None, ctx.st))
    return ctx.harvest(out)


def _host(ctx, max_passes, taps=None, K=None):
    """OpenDSSSolver._solve_regulated's host loop from the three stand-alone
    entries on buffers of its own; `passes` is each env's count of solves, read
    off the masks the solves ran under."""
    n = ctx.n
    out = ctx.outputs(taps, K)
    tb = ctx.tables(out)
    active = torch.full((n,), ISENT, dtype=torch.int32, device=DEV)
    nchg = torch.zeros(1, dtype=torch.int32, device=DEV)
    solves = np.zeros(n, np.int32)
    mask = np.ones(n, np.int32)
    for it in range(1, max_passes + 1):
        if ctx.case.mode == C.PF_EXACT and it == 2:
            tb.U_init = out["U_out"].data_ptr()                 # from the env's previous pass
        tb.env_active = None if it == 1 else active.data_ptr()
        ctx.check(ctx.lib.pgw_pf_solve_general(ctx.prm, tb, n, ctx.const["ctrl_p"].data_ptr(),
                                               ctx.const["ctrl_q"].data_ptr(), out["v_out"].data_ptr(),
                                               out["iters"].data_ptr(), ctx.st))
        solves += (mask != 0)
        nchg.zero_()
        ctx.check(ctx.lib.pgw_reg_control(ctx.rp, n, out["reg_x"].data_ptr(), out["reg_c"].data_ptr(),
                                          out["taps"].data_ptr(), active.data_ptr(), nchg.data_ptr(), ctx.st))
        ctx.check(ctx.lib.pgw_reg_factor(ctx.rp, n, out["taps"].data_ptr(), active.data_ptr(),
                                         out["Kreg"].data_ptr(), ctx.st))
        mask = active.cpu().numpy()
        assert int(nchg.item()) == int((mask != 0).sum())
        if not mask.any():
            break
    out["passes"][:n] = torch.tensor(solves, device=DEV)
    res = ctx.harvest(out)
    res["last_mask"] = mask
    return res


def _env_view(res, k, n):
    """[rows, n] integer view of output k (bit patterns), one column per env."""
    a = res[k]
    if k == "U_out":
        a = a.reshape(n, -1).T
    elif k in ("reg_x", "reg_c", "Kreg"):
        a = a.reshape(-1, n, 2).transpose(0, 2, 1).reshape(-1, n)
    else:
        a = a.reshape(-1, n)
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _assert_bits(dev, host, what, envs=None):
    """Every output bit for bit (NaN included), all envs or the given ones."""
    n = len(dev["passes"])
    sel = np.ones(n, bool) if envs is None else envs
    for k in BITS + ("passes",):
        a, b = _env_view(dev, k, n)[:, sel], _env_view(host, k, n)[:, sel]
        bad = np.nonzero((a != b).any(0))[0]
        assert len(bad) == 0, "%s: %s differs in %d envs, first %s" % (what, k, len(bad), np.nonzero(sel)[0][bad[:5]])


# ------------------------------------------------ (a) every instantiation against the host loop
def test_shape_list_covers_every_instantiation():
    R.check_shapes()


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_every_instantiation_equals_the_host_loop(shape):
    """taps, Kreg, v_out, iters, v_min / v_max, U_out, reg_x and reg_c bit for
    bit those of the host loop of the three entries, and passes each env's
    count of solves there; nothing is stored past n (the guard tails).  The
    batch does work: unless n = 1, some env moves a tap."""
    cs, n, max_iter = shape[:6], shape[6], shape[7]
    ctx = Ctx(R.case(*cs), n, max_iter)
    dev, host = _device(ctx, R.MAX_PASSES), _host(ctx, R.MAX_PASSES)
    _assert_bits(dev, host, R.shape_id(shape))
    ps = dev["passes"]
    assert ps.min() >= 1 and ps.max() <= R.MAX_PASSES and (dev["iters"] != 0).all()
    for k in F64_OUT:
        assert not (dev[k] == SENTINEL).any(), k
    print("%s: passes %s, iters %s" % (R.shape_id(shape), np.bincount(ps).tolist(), np.unique(dev["iters"]).tolist()))
    if n > 1:
        assert ps.max() >= 3 and (dev["taps"] != ctx.taps0.ravel()).any()


# ------------------------------------------------ (b) against the longdouble loop
def _compare(dev, ctx, r, what):
    """The non-excluded envs against the reference loop: taps, passes and iters
    equal, U_out / reg_x / reg_c componentwise and v_out (through | |a| - |b| |
    <= |a - b|) within the propagated bound.  Returns the largest error / bound."""
    n, p = ctx.n, ctx.p
    keep = ~r["excluded"][:n]
    assert keep.sum() >= 0.99 * n
    taps = dev["taps"].reshape(-1, n).T
    np.testing.assert_array_equal(taps[keep], r["taps"][:n][keep], err_msg=what)
    np.testing.assert_array_equal(dev["passes"][keep], r["passes"][:n][keep], err_msg=what)
    np.testing.assert_array_equal(dev["iters"][keep], r["iters"][:n][keep], err_msg=what)
    for k in ("U_out", "v_out", "v_min_out", "v_max_out", "reg_x", "reg_c", "Kreg"):
        assert np.isfinite(dev[k]).all(), (what, k)
    U = dev["U_out"].view(np.complex128).reshape(n, p.m)
    d = U.astype(C.CLD) - r["u"][:n]
    worst = {"U_out": np.maximum(_ratio(np.abs(d.real), r["e_u"][:n]), _ratio(np.abs(d.imag), r["e_u"][:n]))[keep].max()}
    v = dev["v_out"].reshape(p.n_out, n)
    worst["v_out"] = _ratio(np.abs(v.T.astype(C.LD) - np.abs(r["V"][:n])), r["e_v"][:n])[keep].max()
    np.testing.assert_array_equal(dev["v_min_out"], v.min(0), err_msg=what)
    np.testing.assert_array_equal(dev["v_max_out"], v.max(0), err_msg=what)
    rr = p.r_reg
    for k, ref, e in (("reg_x", r["x"], r["e_x"]), ("reg_c", r["c"], r["e_c"])):
        g = dev[k].view(np.complex128).reshape(rr, n).T
        d = g.astype(C.CLD) - ref[:n, :rr]
        worst[k] = np.maximum(_ratio(np.abs(d.real), e[:n, :rr]), _ratio(np.abs(d.imag), e[:n, :rr]))[keep].max()
    print("%s: worst error / bound: %s (%d envs, %d left out; passes up to %d)"
          % (what, ", ".join("%s %.3g" % kv for kv in worst.items()), n, n - keep.sum(), dev["passes"].max()))
    assert max(worst.values()) <= 1.0, (what, worst)
    return max(worst.values())


@pytest.mark.parametrize("cs", R.REF_CASES, ids=[R.case(*c).id() for c in R.REF_CASES])
def test_loop_vs_longdouble(cs, ctx_cache):
    """130 envs, up to 15 passes: for the envs the reference can decide, the
    same taps, passes and iters, and U_out, v_out, reg_x and reg_c of each
    env's last solve within the bound propagated through all its passes (Ref's
    bound, K known to 4 kappa 2^-52 max |K|, every EXACT re-solve seeded with
    the previous pass's bound).  Largest error / bound on the MI355X: 0.138
    (m40+8-r2-CE2-CN4, v_out; U_out 0.095); the other cases 0.093 (m8+8-r5
    exact, reg_x), 0.016, 0.0045, 0.0016 (the r_reg = 17 cases, whose bound
    carries kappa up to 1e4) and 0.046 (m72+8-r5-CE4-CN8); no env left out."""
    ctx = ctx_cache(cs)
    dev = _device(ctx, R.MAX_PASSES)
    _compare(dev, ctx, R.reference(*cs), R.case(*cs).id())


@pytest.mark.parametrize("cs, cap", R.CAP_CASES, ids=["%s-cap%d" % (R.case(*c).id(), k) for c, k in R.CAP_CASES])
def test_pass_cap_vs_longdouble_and_host(cs, cap, ctx_cache):
    """max_passes = 1 and 2, where the cap binds (shown on the reference by
    test_cpu_regloop_ref.py): control and factor still follow the last allowed
    solve -- the reference's taps after `cap` control passes, K refreshed
    exactly where a tap moved (bit for bit the stand-alone factor's, through
    the host loop), the others' K untouched -- and no env counts more than
    `cap` solves; at max_passes = 1 passes is 1 everywhere.  Largest error /
    bound on the MI355X: 0.093, 0.093 (CE 1, caps 1 and 2), 0.054, 0.074 (CE 4)."""
    ctx = ctx_cache(cs)
    n = ctx.n
    dev, host = _device(ctx, cap), _host(ctx, cap)
    _assert_bits(dev, host, "cap %d" % cap)
    r = R.reference(*cs, max_passes=cap)
    _compare(dev, ctx, r, "%s cap %d" % (R.case(*cs).id(), cap))
    assert dev["passes"].max() == cap and (cap > 1 or (dev["passes"] == 1).all())
    assert host["last_mask"].any()                                   # envs cut short by the cap
    if cap == 1:
        moved = (dev["taps"].reshape(-1, n) != ctx.taps0).any(0)
        K, K0 = dev["Kreg"].reshape(-1, n, 2), ctx.K0.reshape(-1, n, 2)
        assert moved.any() and (~moved).any()
        assert (K[:, ~moved] == K0[:, ~moved]).all() and (K[:, moved] != K0[:, moved]).any(0).any(1).all()


# ------------------------------------------------ (c) the other edges
EDGE_IDS = [R.case(*c).id() for c in R.EDGE_CASES]


@pytest.mark.parametrize("cs", R.EDGE_CASES, ids=EDGE_IDS)
def test_block_at_rest_beside_blocks_at_work(cs, ctx_cache):
    """Block 0 entirely at rest (its taps and K those a finished call left),
    block 1 from the case's starting taps (several passes), block 2 one of
    each: block 0's envs get passes = 1 and keep taps and K bit for bit, the
    others run as they did, and all of it equals the host loop."""
    ctx = ctx_cache(cs)
    n = ctx.n
    first = _host(ctx, R.MAX_PASSES)
    assert not first["last_mask"].any()                              # every env came to rest
    rest = np.arange(n) < 64
    rest[128] = True
    taps = np.where(rest, first["taps"].reshape(-1, n), ctx.taps0)
    K = np.where(np.repeat(rest, 2), first["Kreg"].reshape(-1, 2 * n), ctx.K0.reshape(-1, 2 * n)).ravel()
    dev, host = _device(ctx, R.MAX_PASSES, taps, K), _host(ctx, R.MAX_PASSES, taps, K)
    _assert_bits(dev, host, "rest / work")
    assert (dev["passes"][rest] == 1).all()
    for k, start in (("taps", taps.ravel()), ("Kreg", K)):
        a, b = _env_view(dev, k, n), _env_view({k: start}, k, n)
        assert (a[:, rest] == b[:, rest]).all(), k
    assert dev["passes"][64:128].max() >= 3 and dev["passes"][129] == first["passes"][129]
    np.testing.assert_array_equal(dev["passes"][~rest], first["passes"][~rest])
    np.testing.assert_array_equal(dev["taps"].reshape(-1, n)[:, ~rest], first["taps"].reshape(-1, n)[:, ~rest])


@pytest.mark.parametrize("cs", R.EDGE_CASES, ids=EDGE_IDS)
def test_call_repeated_on_its_own_outputs(cs, ctx_cache):
    """The call again with the taps and K it left: every env that ended below
    the cap gets passes = 1 and keeps its taps and K bit for bit."""
    ctx = ctx_cache(cs)
    n = ctx.n
    one = _device(ctx, R.MAX_PASSES)
    two = _device(ctx, R.MAX_PASSES, one["taps"].reshape(-1, n), one["Kreg"])
    done = one["passes"] < R.MAX_PASSES
    assert done.sum() >= 0.9 * n and (one["passes"] >= 3).any()
    assert (two["passes"][done] == 1).all()
    for k in ("taps", "Kreg"):
        a, b = _env_view(one, k, n), _env_view(two, k, n)
        assert (a[:, done] == b[:, done]).all(), k


def _poisoned(ctx, tap):
    """The case with SINGULAR_ENVS (one per block) started at `tap`: (the run
    without them, the poisoned Ctx -- its K0 is pgw_reg_factor's at those taps
    -- its run on the device, the mask of the other envs)."""
    n = ctx.n
    clean = _device(ctx, R.MAX_PASSES)
    bad = np.array(R.SINGULAR_ENVS)
    taps = ctx.taps0.copy()
    taps[0, bad] = tap
    pctx = Ctx(ctx.case, n, taps=taps)
    K0 = pctx.K0.reshape(-1, n, 2)
    assert np.isnan(K0[:, bad]).all() and np.isfinite(np.delete(K0, bad, 1)).all()
    dev = _device(pctx, R.MAX_PASSES)
    other = np.ones(n, bool)
    other[bad] = False
    _assert_bits(dev, clean, "beside a singular env", other)
    assert (clean["passes"] >= 3).any()
    assert np.isnan(dev["Kreg"].reshape(-1, n, 2)[:, bad]).all()
    assert (dev["iters"][bad] == -ctx.prm.max_iter).all()
    a, b = _env_view(dev, "taps", n), _env_view({"taps": taps.ravel()}, "taps", n)
    assert (a[:, bad] == b[:, bad]).all()                               # its taps did not move
    _assert_bits(dev, _host(pctx, R.MAX_PASSES), "singular envs: host loop")
    return dev, bad


@pytest.mark.parametrize("cs", R.SINGULAR_CASES, ids=[R.case(*c).id() for c in R.SINGULAR_CASES])
def test_singular_env_stays_its_own(cs, ctx_cache):
    """One env per block whose I + D S is singular at its starting tap (the
    two-node model of test_reg_factor_singular_env_is_nan at tap 0.5: I + D S
    is the zero matrix, so pgw_reg_factor leaves NaN in its K; pgw.h: "its next
    solve reports unconverged"): it ends with NaN K, passes = 1, iters =
    -max_iter and its taps unmoved, while every other env -- its block runs up
    to nine passes -- is bit for bit what it is in the run without it, and
    the whole equals the host loop.  NaN is data here, not a fault."""
    dev, bad = _poisoned(ctx_cache(cs), R.SINGULAR_TAP)
    assert (dev["passes"][bad] == 1).all()


@pytest.mark.parametrize("cs", R.EDGE_CASES, ids=EDGE_IDS)
def test_nan_tap_poisons_its_own_env_only(cs, ctx_cache):
    """A NaN starting tap (test_reg_factor_nan_tap_poisons_its_own_env_only's
    input) on one env per block: NaN K, iters = -max_iter, the tap still NaN,
    every other env bit for bit as without it, and the device loop equal to the
    host loop -- in which such an env counts as moved in every pass
    (pgw_reg_control compares the wanted tap with the present one, and NaN !=
    NaN), so it is solved max_passes times in both."""
    dev, bad = _poisoned(ctx_cache(cs), np.nan)
    assert (dev["passes"][bad] == R.MAX_PASSES).all()


@pytest.mark.parametrize("cs", R.EDGE_CASES, ids=EDGE_IDS)
def test_passes_may_be_null(cs, ctx_cache):
    ctx = ctx_cache(cs)
    a, b = _device(ctx, R.MAX_PASSES), _device(ctx, R.MAX_PASSES, want_passes=False)
    assert (b["passes"] == ISENT).all()
    b["passes"] = a["passes"]
    _assert_bits(a, b, "passes = NULL")
