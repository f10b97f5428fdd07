"""OpenDSS's snap solve with 2 .. 8 controllable loads on the fast kernel
(OpenDSSSolver(multi_bus="fast"), k_pf_solve_od_ms): what can be checked
without a GPU -- the option's validation, the unchanged ABI, the multi-slot
first-iteration table (a pure NumPy builder) against the oracle's first
iteration, and the conditions tests/test_gpu_pf_multibus.py relies on, asserted
from the oracle alone (tests/_pf_multibus_common.py).

Oracle figures for the seeds and the draw order of _pf_multibus_common
(IEEE-13, rescale 1.2): the smallest distance of a tested stopping decision
from the 1e-4 threshold is 2.3e-7 (case A; 4.0e-7 in B and D, 2.4e-7 in C);
iteration counts 2 .. 6 in A, 2 .. 8 in B, 3 .. 6 in C; case D per hour 314 .. 318
of 321 envs stopped by the cap of 6, 115 .. 181 load-law evaluations at or
below vlow, 18 400 .. 19 800 in (vlow, vmin] and 1 400 .. 2 200 above vmax, none
within 1.9e-5 pu of vlow.  The first-iteration table's u_1 is within 1e-15 rel
of the oracle's.
"""
import ctypes

import numpy as np
import pytest

# the multi-slot path's host side: without it (before the feature) nothing in
# this module has a subject, and the module does not import
from powergridworld_amd.distribution_system.opendss import od_start_affine, od_start_table
from tests import _pf_multibus_common as C


# ------------------------------------------------------------------ arguments, ABI
def test_multi_bus_validated_before_the_device():
    """A bad multi_bus raises ValueError before the device is looked at (the
    device named here does not exist); the default is "general"."""
    import inspect
    from powergridworld_amd.distribution_system.opendss import OpenDSSSolver
    with pytest.raises(ValueError, match="multi_bus"):
        OpenDSSSolver(C.IEEE13, C.SHAPE, device="no-such-device:0", multi_bus="quick")
    assert inspect.signature(OpenDSSSolver.__init__).parameters["multi_bus"].default == "general"


def test_abi_and_struct_sizes_unchanged():
    """ABI 33; pgw_pf_params, pgw_pf_tables and pgw_pf_od keep the sizes of
    the commit before the multi-slot path (1008, 96 and 536 bytes), and the
    multi-slot table's extent is the header's (4 + 8 C) m doubles."""
    from powergridworld_amd import _lib
    assert _lib.ABI_VERSION == 33
    assert (ctypes.sizeof(_lib.PFParams), ctypes.sizeof(_lib.PFTables), ctypes.sizeof(_lib.PFOD)) == (1008, 96, 536)
    assert int(_lib.lib().pgw_abi_version()) == 33
    assert _lib.PF_MAX_CTRL == 8
    W2, u0, y0 = C.reduced()
    f = C.feeder()
    kw, kvar = C.elem_base(C.TIMES[0])
    for n in range(1, 9):
        aff = od_start_affine(W2, u0, f.elem_nph, C.elem_ctrl(C.NAMES[:n]), n, (0.25, 0.9025, 1.1025))
        assert od_start_table(W2, u0, y0, kw, kvar, f.elem_nph, aff).shape == ((4 + 8 * n) * C.M,)


# ------------------------------------------------------------------ the start table
def _table(slots, t):
    W2, u0, y0 = C.reduced()
    f = C.feeder()
    kw, kvar = C.elem_base(t)
    aff = od_start_affine(W2, u0, f.elem_nph, C.elem_ctrl(tuple(slots)), max(len(slots), 1),
                          (C.VLOW ** 2, C.VMIN ** 2, C.VMAX ** 2))
    return od_start_table(W2, u0, y0, kw, kvar, f.elem_nph, aff)


@pytest.mark.parametrize("case", ["A", "B", "C", "D"])
def test_start_table_u1_equals_the_oracles_first_iteration(case):
    """u_1 = u1b + sum_s (P_s u1P_s + Q_s u1Q_s) of the multi-slot table equals
    the element voltages of Feeder.snap_opendss(..., max_iter=1) to 1e-12 rel
    (of the largest element voltage, ~1 pu), for the case's random (P_s, Q_s)."""
    slots = C.CASES[case]["slots"]
    for t, (P, Q) in zip(C.TIMES, C.loads(case)):
        tab = _table(slots, t)
        assert tab.shape == ((4 + 8 * len(slots)) * C.M,)
        u1 = C.start_u1(tab, P, Q)
        V, it, _ = C.oracle_solve(t, slots, P, Q, max_iter=1)
        assert (it == 1).all()
        want = C.elem_pu(V)
        err = np.abs(u1 - want).max() / np.abs(want).max()
        print("case %s %s: u_1 max rel err %.3e" % (case, t, err))
        assert err <= 1e-12


def test_start_table_one_slot_is_todays_table():
    """With one slot (and with none) the builder's table is the one-slot table
    bit for bit, in its layout: u1b, u1P, u1Q, J1b, J1P, J1Q -- the expressions
    of OpenDSSSolver._od_starts before the multi-slot path, restated here."""
    W2, u0, y0 = C.reduced()
    f = C.feeder()
    nph = np.array(f.elem_nph, float)
    for slots in (("675c",), ("671",), ()):
        ctrl0 = C.elem_ctrl(slots) == 0
        fr = np.where(ctrl0, 1000.0 / nph, 0.0)
        fi = np.where(ctrl0, -1000.0 / nph, 0.0)
        m2 = np.abs(u0) ** 2
        g = 1.0 / np.where(m2 <= C.VLOW ** 2, 1.0, np.clip(m2, C.VMIN ** 2, C.VMAX ** 2))
        jP, jQ = fr * g * u0, 1j * fi * g * u0
        u1P, u1Q = W2 @ jP, W2 @ jQ
        for t in C.TIMES:
            kw, kvar = C.elem_base(t)
            s0 = (np.array(kw) * 1000.0) / nph - 1j * ((np.array(kvar) * 1000.0) / nph)
            J0 = (s0 * g - y0) * u0
            want = np.concatenate([u0 + W2 @ J0, u1P, u1Q, J0, jP, jQ]).view(np.float64)
            got = _table(slots, t)
            assert got.shape == (12 * C.M,) and got.tobytes() == want.tobytes()
    # and the first 12 m doubles of a multi-slot table are slot 0's one-slot table
    two = _table(("675c", "675a"), C.TIMES[1])
    assert two[:12 * C.M].tobytes() == _table(("675c",), C.TIMES[1]).tobytes()


# ------------------------------------------------------------------ what the GPU tests rely on
def _decisions(ref):
    """The tested quantity of every stopping decision: iterations >= 2 of the
    envs still iterating."""
    e = ref["err"][2:]
    return e[np.isfinite(e)]


@pytest.mark.parametrize("case", ["A", "B", "C", "D"])
def test_stopping_decisions_are_clear_of_the_threshold(case):
    """Every tested stopping decision is at least 1e-9 pu away from 1e-4: a
    kernel within 1e-9 of the oracle takes the same decisions, so equal
    iteration counts are a fair demand."""
    worst = min(np.abs(_decisions(r) - C.TOL).min() for r in C.oracle(case))
    print("case %s: smallest threshold margin %.3e" % (case, worst))
    assert worst >= 1e-9


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_cases_abc_converge_with_several_counts(case):
    for r in C.oracle(case):
        assert r["conv"].all() and (r["it"] >= 2).all() and (r["it"] < 15).all()
    counts = np.unique(np.concatenate([r["it"] for r in C.oracle(case)]))
    print("case %s: iteration counts %s" % (case, counts))
    assert len(counts) >= 3


def test_case_d_reaches_the_cap_and_every_load_band():
    """Case D (cap 6): envs stopped by the cap and envs that converge; the load
    law evaluated at or below vlow, in (vlow, vmin] and above vmax; no evaluated
    |u| within 1e-6 pu of vlow, the law's only discontinuity."""
    for t, r in zip(C.TIMES, C.oracle("D")):
        capped = int((~r["conv"]).sum())
        u = r["umag"][np.isfinite(r["umag"])]
        low, under, over = int((u <= C.VLOW).sum()), int(((u > C.VLOW) & (u <= C.VMIN)).sum()), int((u > C.VMAX).sum())
        dist = np.abs(u - C.VLOW).min()
        print("case D %s: %d of %d capped, |u| <= vlow %d, (vlow, vmin] %d, > vmax %d, nearest to vlow %.3e"
              % (t, capped, C.K, low, under, over, dist))
        assert 0 < capped < C.K and (r["it"][~r["conv"]] == 6).all() and (r["it"] <= 6).all()
        assert low > 0 and under > 0 and over > 0
        assert dist >= 1e-6
