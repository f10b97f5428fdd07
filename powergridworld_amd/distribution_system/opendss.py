"""Batched drop-in for OpenDSSSolver (reference:
gridworld/distribution_system/opendss.py:15-186).

Same constructor (feeder_file, loadshape_file, system_load_rescale_factor)
and the same call sequence -- calculate_power_flow(p, q, current_time),
get_bus_voltages(), get_bus_voltage_by_name(name) -- but every value is a
[N] tensor (one power flow per env copy) and the snap solve runs in the
pgw_pf_solve kernel on the GPU instead of the OpenDSS engine.
"""
import os
from datetime import datetime
from typing import List, Union

import numpy as np
import pandas as pd
import torch

from powergridworld_amd import _lib
from powergridworld_amd.base import as_env_tensor
from powergridworld_amd.distribution_system.feeder import DATA_DIR, Feeder, load_feeder_spec
from powergridworld_amd.distribution_system.powerflow import PowerFlowSolver

PHASE_MAP = {'a': '.1', 'b': '.2', 'c': '.3'}


def bus_name_to_nodes(bus_name: str) -> List[str]:
    """opendss.py:177-186 -- note str.replace replaces EVERY occurrence of the last
    character, exactly as the reference does."""
    if bus_name[-1] in PHASE_MAP.keys():
        return [bus_name.replace(bus_name[-1], PHASE_MAP[bus_name[-1]])]
    return [bus_name + p for p in PHASE_MAP.values()]


def load_loadshape(loadshape_file):
    base = os.path.basename(str(loadshape_file)).lower()
    if base == "annual_hourly_load_profile.csv" and not os.path.exists(str(loadshape_file)):
        return np.load(os.path.join(DATA_DIR, "loadshape_8760.npy"))
    if os.path.exists(str(loadshape_file)):
        return np.genfromtxt(loadshape_file)
    if base == "annual_hourly_load_profile.csv":
        return np.load(os.path.join(DATA_DIR, "loadshape_8760.npy"))
    raise FileNotFoundError("loadshape file %r not found" % (loadshape_file,))


def get_hour_of_year(dt):
    """opendss.py:98-103"""
    beginning_of_year = datetime(dt.year, 1, 1)
    return int((dt - beginning_of_year).total_seconds() // 3600)


def _extrema_bounds(A, B, C, tl, th, samples=9, delta=1e-9):
    """Per piece and row, bounds (lo, hi) [pieces, rows] of |V_r(t)|^2 over t
    in [tl, th] (V_r(t) = A + t (B + t C)): `samples` equally spaced values
    plus a Lipschitz margin (|d|V|^2/dt| <= 2 |V| |V'|) plus `delta`."""
    S = samples
    ts = (tl[:, None] + (th - tl)[:, None] * torch.linspace(0.0, 1.0, S, dtype=torch.float64,
                                                              device=A.device)[None, :])[:, :, None]
    V = A[:, None, :] + ts * (B[:, None, :] + ts * C[:, None, :])            # [P, S, rows]
    m2 = V.real * V.real + V.imag * V.imag
    T = torch.maximum(tl.abs(), th.abs())[:, None]
    L = 2.0 * (A.abs() + B.abs() * T + C.abs() * T * T) * (B.abs() + 2.0 * C.abs() * T)
    marg = L * ((th - tl)[:, None] / (S - 1)) * 0.5 + delta
    return m2.min(1).values - marg, m2.max(1).values + marg


def extrema_candidates(A, B, C, tl, th, samples=9, delta=1e-9):
    """Rows that can hold the minimum or the maximum |V| over t in [tl, th] of
    some piece: A, B, C [pieces, rows] complex (V_r(t) = A + t (B + t C)), tl /
    th [pieces].  Per piece, |V_r|^2 is bounded as _extrema_bounds does; a
    row is a candidate when its lower bound reaches every row's upper bound or
    its upper bound every row's lower bound.  Returns a bool array [rows], or
    None when a bound is not finite (then every row is kept)."""
    lo, hi = _extrema_bounds(A, B, C, tl, th, samples, delta)
    if not (torch.isfinite(lo).all() and torch.isfinite(hi).all()):
        return None
    cand = ((lo <= hi.min(1, keepdim=True).values) | (hi >= lo.max(1, keepdim=True).values)).any(0)
    return cand.cpu().numpy()


def extrema_candidates_per_piece(A, B, C, tl, th, samples=9, delta=1e-9):
    """extrema_candidates for each piece on its own: [pieces, rows] bool, the
    rows that can hold that piece's minimum or maximum |V| (every row of a
    piece whose bounds are not finite).  Comparing fewer rows only adds
    candidates, so a row set that holds every row the extremum can come from
    (the table's candidates) is enough."""
    lo, hi = _extrema_bounds(A, B, C, tl, th, samples, delta)
    fin = torch.isfinite(lo).all(1) & torch.isfinite(hi).all(1)
    cand = (lo <= hi.min(1, keepdim=True).values) | (hi >= lo.max(1, keepdim=True).values)
    cand[~fin] = True
    return cand


def od_start_affine(W2, u0, nph, elem_ctrl, n_slots, band2):
    """The hour-independent part of the first-iteration table (pgw_pf_od.start):
    from the direct solution u0 the compensation currents are affine in every
    controllable slot's (P, Q) -- g(|u0|^2) is the same for every env --, so per
    slot s the maps jP_s, jQ_s (the currents' change per kW / kvar: nonzero on
    the slot's elements) and u1P_s = W'' jP_s, u1Q_s = W'' jQ_s.  Pure NumPy.
    W2 [M, M], u0 [M] complex (pu); nph, elem_ctrl [M]; band2 = (vlow^2,
    vmin^2, vmax^2).  Returns (g [M], [(u1P, u1Q, jP, jQ)] per slot)."""
    lo2, mn2, mx2 = band2
    nph = np.asarray(nph, float)
    ctrl = np.asarray(elem_ctrl)
    m2 = np.abs(u0) ** 2
    g = 1.0 / np.where(m2 <= lo2, 1.0, np.clip(m2, mn2, mx2))
    slots = []
    for s in range(n_slots):
        on = ctrl == s
        fr = np.where(on, 1000.0 / nph, 0.0)
        fi = np.where(on, -1000.0 / nph, 0.0)
        jP, jQ = fr * g * u0, 1j * fi * g * u0
        slots.append((W2 @ jP, W2 @ jQ, jP, jQ))
    return g, slots


def od_start_table(W2, u0, y0, base_kw, base_kvar, nph, affine):
    """pgw_pf_od.start of one hour for C = len(slots) controllable slots, (4 +
    8 C) M doubles: u1b, u1P_0, u1Q_0, J1b, J1P_0, J1Q_0 -- the one-slot table
    and layout, 12 M -- then u1P_s, u1Q_s, J1P_s, J1Q_s per further slot (M
    complex each), so that
        u_1 = u1b + sum_s (P_s u1P_s + Q_s u1Q_s),  J_1 = J1b + sum_s (P_s J1P_s + Q_s J1Q_s).
    base_kw / base_kvar [M]: the hour's base loads per element; y0 [M] complex:
    the loads' Yeq powers; affine: od_start_affine's result.  Pure NumPy."""
    g, slots = affine
    nph = np.asarray(nph, float)
    s0 = (np.asarray(base_kw, float) * 1000.0) / nph - 1j * ((np.asarray(base_kvar, float) * 1000.0) / nph)
    J0 = (s0 * g - y0) * u0
    u1P, u1Q, jP, jQ = slots[0]
    parts = [u0 + W2 @ J0, u1P, u1Q, J0, jP, jQ]
    for sl in slots[1:]:
        parts.extend(sl)
    return np.concatenate(parts).view(np.float64)


def h1_yeq_change(base_kw, base_kvar, nph, y0):
    """yprim="step": the hour's base-load Yeq change dD [M] against the DSS
    file's (per element, W - j var per phase): the kernel's own per-phase power
    of the hour (base_kw / base_kvar [M]: the hour's loads per element) less
    y0 [M] complex, the Yeq powers in the file model's Y.  Pure NumPy."""
    nph = np.asarray(nph, float)
    s = (np.asarray(base_kw, float) * 1000.0) / nph - 1j * ((np.asarray(base_kvar, float) * 1000.0) / nph)
    return s - np.asarray(y0, complex)


def h1_hour_reduction(W2, u0, dD):
    """The hour's reduction from the file model's (W2 [M, M], u0 [M], pu): u =
    u0 + W J with J = J' + dD u gives W_h = (I - W dD)^-1 W (complex symmetric,
    symmetrised against rounding) and u0_h = (I - W dD)^-1 u0.  Pure NumPy."""
    A = np.eye(len(u0)) - W2 * dD[None, :]
    Wh = np.linalg.solve(A, W2)
    return 0.5 * (Wh + Wh.T), np.linalg.solve(A, u0)


def h1_hour_rows(G, V0, dD, Wh, u0h):
    """Rows V0 + G J of the file model (G [R, M], V0 [R]) as the hour's V0_h +
    G_h J': G_h = G (I + dD W_h), V0_h = V0 + G dD u0_h.  Pure NumPy.
    The two products are summed term by term in index order on real and
    imaginary parts, so a row's bits do not depend on which other rows are
    asked for: BLAS rounds a row by the product's shape, and a solver that
    outputs one node (the fused C4 step) owes that node the bits of a solver
    that outputs them all (the generic path, the on-demand env.voltages)."""
    B = np.concatenate([Wh, u0h[:, None]], axis=1)           # [M, M + 1]: G dD W_h and G dD u0_h at once
    ar = G.real * dD.real[None, :] - G.imag * dD.imag[None, :]
    ai = G.real * dD.imag[None, :] + G.imag * dD.real[None, :]
    br, bi = B.real, B.imag
    re, im = np.zeros((G.shape[0], B.shape[1])), np.zeros((G.shape[0], B.shape[1]))
    for k in range(B.shape[0]):
        re += ar[:, k, None] * br[None, k] - ai[:, k, None] * bi[None, k]
        im += ar[:, k, None] * bi[None, k] + ai[:, k, None] * br[None, k]
    P = re + 1j * im
    return G + P[:, :-1], V0 + P[:, -1]


def h1_hour_tables(W2, u0, y0, base_kw, base_kvar, nph, G_out, V0_out, G_chk, V0_chk, elem):
    """Everything pgw_pf_solve_h1 reads of one hour (include/pgw.h, pgw_pf_h1):
    dict(W, u0: the block's operands; G, V0: the output rows; Gc, V0c: the check
    rows; wc: W_h[:, elem] [M] complex, zeros with elem < 0).  Pure NumPy."""
    dD = h1_yeq_change(base_kw, base_kvar, nph, y0)
    Wh, u0h = h1_hour_reduction(W2, u0, dD)
    G, V0 = h1_hour_rows(G_out, V0_out, dD, Wh, u0h)
    Gc, V0c = h1_hour_rows(G_chk, V0_chk, dD, Wh, u0h)
    wc = Wh[:, elem].copy() if elem >= 0 else np.zeros(len(u0), complex)
    return dict(W=Wh, u0=u0h, G=G, V0=V0, Gc=Gc, V0c=V0c, wc=wc)


class OpenDSSSolver(PowerFlowSolver):

    # Per-hour predictor grid (single controllable load): the batched solve
    # starts each env from the quadratic through 3 grid solutions near its
    # controllable kW (chosen so that they share its load-band signature).  Envs
    # outside the grid extrapolate (more iterations, same result).
    PREDICTOR_X0, PREDICTOR_H, PREDICTOR_N = -500.0, 0.625, 3201
    PREDICTOR_TOL = 1e-12
    PREDICTOR_MAX_TABLES = 64      # hours kept on the device (~180 KB each)
    PREDICTOR_LOOKAHEAD = 24       # hours solved per table launch

    # OpenDSS's snap-solve defaults (Solution.pas: ConvergenceTolerance,
    # MinIterations, MaxIterations)
    OPENDSS_TOL, OPENDSS_MIN_ITER, OPENDSS_MAX_ITER = 1e-4, 2, 15

    def __init__(self, feeder_file: str, loadshape_file: str, system_load_rescale_factor: float = 1.0,
                 num_envs: int = 1, device=None, tol: float = None, max_iter: int = None,
                 output_nodes=None, predictor: bool = True, warm_start: bool = False,
                 convergence: str = "opendss", general: bool = None, od_table: bool = True,
                 snap_start: str = "direct", yprim: str = "dss_file", control_loop: str = "host",
                 multi_bus: str = "general", step_kernel: str = "general", start_kernel: str = "general",
                 **kwargs):
        """convergence: "opendss" (the default) -- OpenDSS's own snap solve as
        the reference runs it (opendss.py:134):
        loads' nominal admittances in Y, start from the direct solution, stop at
        the first iteration >= 2 whose largest node-voltage magnitude change is
        <= tol = 1e-4 pu, at most 15; "exact" (opt-in) -- every env's solve
        iterates to the fixed point (max |dU| < tol = 1e-10 pu), history-free
        and reproducible (DESIGN.md section 2 measures the difference).
        Feeders with more than 16 load phase elements, other load models or
        RegControls run the general kernel (pgw_pf_solve_general); general=True
        forces it (tests, measurements).  od_table: the fast OpenDSS-rule
        kernels read the hour's response table (pgw_pf_od.resp) and solve only
        the envs it does not cover; False solves every env.
        snap_start (OpenDSS rule): "direct" (the default) -- every snap solve
        starts from the direct solution, as `Solve mode=snap` re-initialises
        the solution; "previous" -- each env's solve
        starts from its previous solution (the other reading of
        opendss.py:134, which this build cannot confirm without OpenDSS): the
        general kernel with U_init / U_out over a per-env buffer (the first
        solve starts from the direct solution); no response table, the
        generic multi-agent path.
        yprim (OpenDSS rule): "dss_file" (the default, H2) -- Y keeps every
        load's Yeq of the DSS file, as the Loads.kW / kvar setters leave Yprim
        valid; "step" (H1) -- each solve's Y holds its own
        loads' Yeq (the hour's base loads and each env's controllable power):
        the general kernel with the hour's reduction and the controllable
        elements' per-env Yeq change as correction columns
        (PGW_PF_OPENDSS_STEP); no response table, the generic multi-agent path.
        control_loop (feeders with RegControls; nothing changes without them):
        "host" (the default) -- the snap solve with controls as a host loop of
        pgw_pf_solve_general / pgw_reg_control / pgw_reg_factor launches, one
        host synchronisation per control pass; "device" -- the whole loop in
        one launch (pgw_pf_solve_regulated: each block of 64 envs runs its own
        passes), no synchronisation, the same per-env arithmetic and results
        bit for bit; control_passes then holds each env's solves, and the
        fused multi-agent step (pgw_ma_step) serves the feeder.  Not with
        snap_start="previous" on such a feeder (ValueError).
        multi_bus (OpenDSS rule, 2 .. 8 controllable loads on a feeder of the
        fast shape; nothing changes otherwise): "general" (the default) -- the
        general kernel, as every other feeder; "fast" -- the fast kernel's
        multi-slot instantiation (k_pf_solve_od_ms: per-lane element powers,
        the closed-form first iteration over every slot, no response table --
        od_table is ignored there, every env is solved), which the fused
        multi-agent step then runs too; `general` / `_od_fast` tell which.
        step_kernel (yprim="step"; nothing changes otherwise): "general" (the
        default) -- the general kernel as described above; "fast" -- on a
        feeder of the fast shape with at most one controllable load of one
        phase element, the fast one-lane-per-env kernel (pgw_pf_solve_h1,
        k_pf_solve_od_h1): the hour's reduction packed per hour and cached on
        the device, the env's correction K formed in the kernel -- no per-step
        torch arithmetic --, and the fused multi-agent step runs it too.
        Anything else (a delta load such as 671, several controllable loads,
        other feeders) falls back to the general kernel; `general` tells which
        route runs.
        start_kernel (snap_start="previous"; ignored otherwise): "general" (the
        default) -- the general kernel with U_init / U_out as described above;
        "fast" -- on a feeder of the fast shape with at most one controllable
        load (of any number of phase elements), the fast one-lane-per-env
        kernel (pgw_pf_solve_prev, k_pf_solve_od_prev): each env's element
        voltages live in a [2 M][N] fp64 state buffer that the kernel reads
        and overwrites in place; the chain restarts from the direct solution
        (pgw_pf_prev_reset) at construction and whenever the outputs or the
        controllable loads change, not at an env's reset(); no response table;
        the fused multi-agent steps run it too (pgw_coord_step_prev, or
        pgw_ma_step's agents followed by pgw_pf_solve_prev).  Anything else
        (several controllable loads, other feeders, RegControls) falls back to
        the general kernel; `general` tells which route runs."""
        super().__init__(**kwargs)
        if start_kernel not in ("general", "fast"):
            raise ValueError("start_kernel must be 'general' or 'fast', got %r" % (start_kernel,))
        self.start_kernel = start_kernel
        if step_kernel not in ("general", "fast"):
            raise ValueError("step_kernel must be 'general' or 'fast', got %r" % (step_kernel,))
        self.step_kernel = step_kernel
        if multi_bus not in ("general", "fast"):
            raise ValueError("multi_bus must be 'general' or 'fast', got %r" % (multi_bus,))
        self.multi_bus = multi_bus
        if control_loop not in ("host", "device"):
            raise ValueError("control_loop must be 'host' or 'device', got %r" % (control_loop,))
        self.control_loop = control_loop
        if convergence not in ("exact", "opendss"):
            raise ValueError("convergence must be 'exact' or 'opendss', got %r" % (convergence,))
        if snap_start not in ("direct", "previous"):
            raise ValueError("snap_start must be 'direct' or 'previous', got %r" % (snap_start,))
        if snap_start == "previous" and convergence != "opendss":
            raise ValueError("snap_start='previous' is a reading of OpenDSS's snap solve (convergence='opendss'); "
                             "the exact fixed point has warm_start=True")
        self.snap_start = snap_start
        if snap_start == "previous":
            od_table = False
            if start_kernel != "fast":
                general = True
        if yprim not in ("dss_file", "step"):
            raise ValueError("yprim must be 'dss_file' or 'step', got %r" % (yprim,))
        if yprim == "step" and (convergence != "opendss" or snap_start != "direct"):
            raise ValueError("yprim='step' is a reading of OpenDSS's snap solve from the direct solution "
                             "(convergence='opendss', snap_start='direct')")
        self.yprim = yprim
        if yprim == "step":
            od_table = False
            if step_kernel != "fast":
                general = True
        self.convergence = convergence
        self.od_table = bool(od_table)
        self.num_envs = int(num_envs)
        self.device = _lib.require_device(device)
        spec = load_feeder_spec(feeder_file)
        self.feeder = Feeder(spec)
        # the fast kernels hold up to PF_MAX_M constant-PQ elements; larger feeders,
        # other load models and OpenDSS's stopping rule run the general kernel
        self.regulators = None
        f = self.feeder
        regctl = bool(spec.get("regcontrols") and spec.get("controlmode", "static") != "off")
        model1 = not bool((f.elem_model != 1).any())
        # OpenDSS's rule on the fast kernels (pgw_pf_tables.od): the C4 shape --
        # 14 constant-PQ elements in one voltage band, no RegControl; at most one
        # controllable load, or with multi_bus="fast" up to 8
        # (set_controllable_loads falls back to the general kernel beyond that)
        self._od_fast = (convergence == "opendss" and not general and not regctl and model1 and
                         self.OPENDSS_MIN_ITER >= 2 and
                         f.m <= _lib.PF_MAX_M and int(_lib.lib().pgw_pf_padded_m(f.m)) == 14 and
                         len({(a, b, c) for a, b, c in zip(f.elem_vmin, f.elem_vmax, f.elem_vlow)}) == 1)
        self.general = (bool(general) or (convergence == "opendss" and not self._od_fast)
                        or f.m > _lib.PF_MAX_M or not model1 or regctl)
        # yprim="step" on the fast kernel (step_kernel="fast"; pgw_pf_solve_h1)
        self._h1_fast = yprim == "step" and self._od_fast
        self._h1f_cache = {}
        # snap_start="previous" on the fast kernel (start_kernel="fast"; pgw_pf_solve_prev)
        self._prev_fast = snap_start == "previous" and self._od_fast
        self._prev_U, self._prev_keepalive = None, None
        if self.feeder.m > _lib.PFG_MAX_M:
            raise ValueError("feeder has %d load phase elements (max %d)" % (self.feeder.m, _lib.PFG_MAX_M))
        if convergence == "opendss":
            if warm_start and snap_start != "previous":
                raise ValueError("convergence='opendss' starts every solve from the direct solution; "
                                 "snap_start='previous' starts it from the env's previous solution")
            warm_start = snap_start == "previous"
            self._fd_iter = Feeder(spec, load_yprim=True)      # OpenDSS's Y (+ loads' Yeq)
            tol = self.OPENDSS_TOL if tol is None else tol
            max_iter = self.OPENDSS_MAX_ITER if max_iter is None else max_iter
        else:
            self._fd_iter = self.feeder
            tol = 1e-10 if tol is None else tol
            max_iter = 100 if max_iter is None else max_iter
        # RegControl (automatic regulator taps, STATIC control mode): per-env taps,
        # the control loop in calculate_power_flow (pgw_reg_control / pgw_reg_factor)
        self.regulators = self.feeder.regulators(Z=self._fd_iter.Z)
        if self.regulators is not None and yprim == "step":
            raise ValueError("yprim='step' with RegControls is not supported")
        if self.regulators is not None and control_loop == "device" and snap_start == "previous":
            # the kernel re-arms the direct-solution pass after every tap move, and
            # both entries refuse the OpenDSS rule with U_init and RegControls
            raise ValueError("control_loop='device' with snap_start='previous' and RegControls is not "
                             "supported: a re-solve after a tap move starts from the direct solution")
        if self.regulators is not None:
            self._init_regulators()
        self._h1, self._h1_cache = None, {}
        self.system_load_rescale_factor = system_load_rescale_factor
        self.annual_hourly_load_profile = load_loadshape(loadshape_file)
        if len(self.annual_hourly_load_profile) != 8760:
            print("Warning: The provided load shape file is not annual hourly ",
                  "profile. Error might occur later")
        # the PQ (model-1) loads the reference manipulates, in circuit order
        # (opendss.py:54-77); other loads stay at their base values
        self.load_bus_name = [nm for nm, ld in zip(self.feeder.load_names, self.feeder.spec["loads"])
                              if ld.get("model", 1) == 1]
        self.base_load = np.stack([self.feeder.base_kw, self.feeder.base_kvar], 1)
        self.tol, self.max_iter = float(tol), int(max_iter)
        self.min_iter = self.OPENDSS_MIN_ITER if convergence == "opendss" else 1
        self.bus_voltages = {}
        self.iterations = None       # [N] int32 per env; -max_iter = stopped unconverged
        self._extrema = None
        self._hour_memo = {}
        self._ctrl_names = []
        self.use_predictor = bool(predictor)
        # warm_start: without a predictor table (several controllable loads),
        # each env's solve starts from its previous solution, as OpenDSS's snap
        # solve starts from the last one (opendss.py:134): the same fixed point
        # to tol, in fewer iterations than from the no-load voltages -- but the
        # last bits then depend on the env's history (off by default: results
        # reproducible per step, and the fused multi-bus step, which always
        # starts cold, stays bit-identical to the generic one).
        self.warm_start = bool(warm_start)
        self._U_prev = None
        self._warm = None
        self.set_output_nodes(output_nodes)

    # ------------------------------------------------------------ configuration
    def set_output_nodes(self, nodes=None):
        """Which node voltages the solve writes (default: every node, as
        AllBusMagPu does).  The fused multi-agent step asks only for what it uses."""
        f = self.feeder
        names = f.node_names if nodes is None else [n.lower() for n in nodes]
        self.output_names = names
        self._names_ver = getattr(self, "_names_ver", 0) + 1
        idx = [f.node_index[n] for n in names]
        self._out_idx = idx
        if self.general:
            return self._set_general_tables(idx)
        # OpenDSS rule: the reduction of its iteration matrix (Y + the loads' Yeq;
        # U0 = the direct solution)
        M, W, U0, G, V0o = (self._fd_iter if self._od_fast else f).reduce(idx)
        self.M = M
        self._base_params()
        dev = self.device
        as_dev = lambda c: torch.tensor(np.ascontiguousarray(c).view(np.float64).ravel(),
                                        dtype=torch.float64, device=dev)
        block = np.zeros(int(_lib.lib().pgw_pf_pack_size(M)))
        # output rows in pu against the scaled currents I'_k = I_k vb_k
        vb_elem = np.array([self.params.vbase[k] for k in range(M)])
        inv_vb_out = 1.0 / (f.kv_ln[idx] * 1000.0)
        Gs = (G / vb_elem[None, :]) * inv_vb_out[:, None]
        V0s = V0o * inv_vb_out
        Wf = np.ascontiguousarray(W).view(np.float64).ravel()
        U0f = np.ascontiguousarray(U0).view(np.float64).ravel()
        G0 = np.ascontiguousarray(Gs[0]).view(np.float64).ravel()
        V00 = np.ascontiguousarray(V0s[:1]).view(np.float64).ravel()
        cp = lambda a: a.ctypes.data_as(_lib.C.c_void_p)
        _lib.check(_lib.lib().pgw_pf_pack(self.params, cp(Wf), cp(U0f), cp(G0), cp(V00), cp(block)))
        self._block = torch.tensor(block, dtype=torch.float64, device=dev)
        self._G, self._V0 = as_dev(Gs), as_dev(V0s)
        # per-env min / max over the output rows, written by the solve's epilogue
        # (multiagent_env.py:107-113 reads them when an agent observes them)
        self._vmin = torch.zeros(self.num_envs, dtype=torch.float64, device=dev)
        self._vmax = torch.zeros(self.num_envs, dtype=torch.float64, device=dev)
        self._all_nodes = len(names) == f.n
        self.tables = _lib.PFTables(block=self._block.data_ptr(), G=self._G.data_ptr(),
                                    V0=self._V0.data_ptr(), v_min_out=self._vmin.data_ptr(),
                                    v_max_out=self._vmax.data_ptr())
        self.v_out = torch.zeros((max(len(names), 1), self.num_envs), dtype=torch.float64, device=dev)
        self._own_v_out = self.v_out
        self._bv_cache = {}
        self._iters = torch.zeros(self.num_envs, dtype=torch.int32, device=dev)
        n_pred = self.PREDICTOR_N
        self._pred_x = torch.tensor([[self.PREDICTOR_X0 + j * self.PREDICTOR_H for j in range(n_pred)]],
                                    dtype=torch.float64, device=dev)
        # preallocated: cached PFTables hold raw pointers into these.  Records
        # (pgw_pf_pred_pack) are 32 M bytes = 4 M doubles per grid point.
        self._pred_table = torch.zeros((self.PREDICTOR_MAX_TABLES, n_pred, 4 * M), dtype=torch.float64,
                                       device=dev)
        self._pred_grid = None                         # scratch: grid solutions of one batch
        self._pred_sig = torch.zeros((self.PREDICTOR_MAX_TABLES, n_pred), dtype=torch.int32, device=dev)
        # pgw_pred_meta per grid segment: (tstar f64, left i32, right i32) = 2 x 8 bytes
        self._pred_meta = torch.zeros((self.PREDICTOR_MAX_TABLES, n_pred - 1, 2), dtype=torch.float64,
                                      device=dev)
        self._pred_index = {}
        if self._od_fast:
            self._set_od_tables(W, U0, vb_elem)
        if self._prev_fast:
            self._prev_restart()

    # ------------------------------------------------------------ OpenDSS rule, fast kernels
    OD_MAX_TABLES = 64            # hours of first-iteration tables kept on the device

    def _set_od_tables(self, W, U0, vb_elem):
        """pgw_pf_od (include/pgw.h): the loads' Yeq powers y0', the element-node
        scales, the check rows -- every node that is not an element's terminal:
        evaluated rows first, then members (electrically next to an evaluated
        row or an element node) and source-side nodes, both bounded -- and the
        bound constants.  OpenDSS's test runs over every node (Solution.pas
        Converged); the bounds only decide which rows the kernel must evaluate."""
        f, fi, M = self.feeder, self._fd_iter, self.M
        m, n = f.m, f.n
        vbn = f.kv_ln * 1000.0
        _, _, Gall, V0all = fi.reduce_rows(list(range(n)))
        Gs = np.zeros((n, M), complex)
        Gs[:, :m] = (Gall / f.elem_vbase[None, :]) / vbn[:, None]
        V0s = V0all / vbn
        od = _lib.PFOD()
        od.tol, od.min_iter = self.tol, self.min_iter
        elem_nodes = []
        for k in range(m):
            li = f.elem_load[k]
            od.y0r[k] = f.base_kw[li] * 1000.0 / f.elem_nph[k]
            od.y0i[k] = -(f.base_kvar[li] * 1000.0 / f.elem_nph[k])
            if f.elem_q[k] < 0:                      # phase node -> ground: the node itself
                od.elem_scale[k] = f.elem_vbase[k] / vbn[f.elem_p[k]]
                elem_nodes.append(int(f.elem_p[k]))
        rowmax = np.abs(Gs).max(1)
        others = [i for i in range(n) if i not in elem_nodes]
        src = [i for i in others if rowmax[i] <= 1e-2 * rowmax.max()]
        reps, members = [], []
        for j in others:
            if j in src:
                continue
            best = None
            for r in elem_nodes + reps:
                g = np.abs(Gs[j] - Gs[r]).max()
                if g <= 1e-5 * rowmax[r] and abs(V0s[j] - V0s[r]) <= 1e-5 and (best is None or g < best[0]):
                    best = (g, r)
            if best is None:
                reps.append(j)
            else:
                members.append((j, best[1]))
        rows = reps + [j for j, _ in members] + src
        if len(rows) > _lib.PF_OD_MAX_ROWS:
            raise ValueError("%d check rows (max %d)" % (len(rows), _lib.PF_OD_MAX_ROWS))
        od.n_rep, od.n_rows = len(reps), len(rows)
        od.gamma = max([float(np.abs(Gs[j] - Gs[r]).max()) for j, r in members], default=0.0)
        od.eps = max([float(abs(V0s[j] - V0s[r])) for j, r in members], default=0.0)
        od.gmax = float(rowmax[elem_nodes + reps].max())
        od.gsrc = float(rowmax[src].max()) if src else 0.0
        dev = self.device
        cdev = lambda a: torch.tensor(np.ascontiguousarray(a).view(np.float64).ravel(), dtype=torch.float64,
                                      device=dev)
        self._od_Gall, self._od_V0all = Gs, V0s          # every node's row (the node records)
        self._od_row_idx = rows
        self._od_rows_V0 = cdev(V0s[rows] if rows else np.zeros(1, complex))
        self._od_rows_G = cdev(Gs[rows] if rows else np.zeros((1, M), complex))
        od.rows_V0, od.rows_G = self._od_rows_V0.data_ptr(), self._od_rows_G.data_ptr()
        self._od_proto = od
        self._od_rows = [f.node_names[i] for i in rows]
        self._od_W2 = W / (vb_elem[:, None] * vb_elem[None, :])
        self._od_u0 = U0 / vb_elem
        self._od_start = torch.zeros((self.OD_MAX_TABLES, 12 * M), dtype=torch.float64, device=dev)
        self._od_resp = None                 # response tables (allocated on the first build)
        self._od_vresp = None                # their node records (pgw_pf_od.resp_v)
        self._od_rowmask = {}                # pgw_pf_od.resp_rows per (table row, configuration)
        self.od_node_records = True          # False: every solve reads the node's row from the currents
        self.od_row_masks = True             # pgw_pf_od.resp_rows (False: every row, for A/Bs and tests)
        self.od_record_rows = True           # row records' per-record candidate slots (False: every slot)
        self.od_certify = True               # certify every piece (od_certify; False: probes only, for A/Bs)
        self.od_certify_native = True        # the certificate in k_pf_od_certify (False: the torch program, for A/Bs)
        self.od_row_records = True           # pgw_pf_od.resp_q (False: the rows from the currents, for A/Bs)
        self._od_qrec = None                 # row records [table row, record, OD_QSTRIDE]
        self._od_qinfo = {}                  # (table row, configuration) -> (row bits, k) or None
        self._od_qflags = {}                 # ... -> (od_node_records, od_record_rows) it was built with
        self.od_resp_stats, self.od_resp_brackets = {}, {}
        self._od_index = {}
        self._od_keep = {}

    def _od_starts(self, hour):
        """First-iteration tables (pgw_pf_od.start) of `hour` and the following
        hours that have none: from the direct solution u0 the currents are affine
        in the controllable (P, Q), so they and u_1 are tabulated as affine maps."""
        hours, keys = [], []
        for h in range(hour, min(hour + self.PREDICTOR_LOOKAHEAD, len(self.annual_hourly_load_profile))):
            k = self._hour_key(h)
            if k not in self._od_index and k not in keys:
                hours.append(h)
                keys.append(k)
        if len(self._od_index) + len(keys) > self.OD_MAX_TABLES:
            self._od_index, self._tables_cache, self._od_keep = {}, {}, {}
            self.tables_version += 1
        idx0 = len(self._od_index)
        M, od = self.M, self._od_proto
        W2, u0 = self._od_W2, self._od_u0
        p0 = self.params
        nph = np.array(p0.nph[:M])
        y0 = np.array(od.y0r[:M]) + 1j * np.array(od.y0i[:M])
        # one table per slot set: (4 + 8 C) M doubles, 12 M with one slot (or none)
        n_slots = max(len(self._ctrl_names), 1)
        width = (4 + 8 * n_slots) * M
        if self._od_start.shape[1] != width:     # (the slots changed: _base_params emptied the index)
            self._od_start = torch.zeros((self.OD_MAX_TABLES, width), dtype=torch.float64, device=self.device)
        affine = od_start_affine(W2, u0, nph, np.array(p0.elem_ctrl[:M]), n_slots,
                                 (p0.vlow[0] ** 2, p0.vmin[0] ** 2, p0.vmax[0] ** 2))
        recs = np.zeros((len(hours), width))
        for q, h in enumerate(hours):
            p = self._params_for_hour(h)
            recs[q] = od_start_table(W2, u0, y0, np.array(p.base_kw[:M]), np.array(p.base_kvar[:M]), nph, affine)
        for j, k in enumerate(keys):
            self._od_index[k] = idx0 + j
        if hours:
            self._od_start[idx0:idx0 + len(hours)].copy_(torch.from_numpy(recs), non_blocking=False)
            if self.od_table and n_slots == 1:   # (several slots: no response table, every env is solved)
                self._od_response(hours, idx0)

    # ------------------------------------------------------------ OpenDSS rule: response tables
    # pgw_pf_od.resp (include/pgw.h): per hour, the snap solve's accepted
    # currents J' and iteration count as piecewise quadratics of the env's kW
    # (one controllable slot, Q = 0), built with pgw_pf_od_probe -- the same snap
    # solve -- on the predictor grid: every segment's ends and midpoint; segments
    # whose three signatures (iteration count + every iterate's load bands) differ
    # sampled at OD_RESP_SUB points and every signature change bisected to a
    # bracket of ~1e-10 kW; three fit points per piece; two check points per
    # piece bound the fit error (OD_RESP_TOL, relative, else the piece is left to
    # the solve); then a certificate per piece (od_certify: Taylor models of the
    # whole iteration over the interval) proves every band and stopping decision
    # constant over what the record serves, cutting the piece to its longest
    # certified run.  Envs in a bracket or a cut-off guard zone, outside the grid
    # or with Q != 0 run the solve.
    OD_RESP_EXTRA = 1024          # records per hour beyond the grid's (further pieces of a segment)
    OD_RESP_SUB = 64              # sample points across a segment with a breakpoint
    OD_RESP_BISECT = 26           # rounds per bracket: h / 64 / 2^26 ~ 1.5e-10 kW
    OD_RESP_PASSES = 6            # bracket passes (a further breakpoint inside a bracket)
    OD_RESP_MIN_WIDTH = 1e-9      # kW: narrower pieces are left to the solve
    OD_RESP_TOL = 2e-11           # fit error bound at the check points (max |dJ| / max |J|)

    @staticmethod
    def _od_meta_word(it, nxt):
        """Record word [4] (PGW_OD_REC): int32 k* in the low half, int32 next in
        the high half, as an int64."""
        return int(np.array([(it & 0xffffffff) | ((nxt & 0xffffffff) << 32)], np.uint64).view(np.int64)[0])

    def _od_probe(self, hours, idx0, pts):
        """pgw_pf_od_probe over the batch's hours (rows idx0.. of the start
        tables): pts[q] = the kW points of hour q.  Returns (J [n, M, 2] device,
        signatures [n] uint64, iterations [n] int32, per-hour lane offsets)."""
        M, H, dev = self.M, len(hours), self.device
        lph = max(256, -(-max(len(p) for p in pts) // 256) * 256)
        n = H * lph
        P = np.full(n, self.PREDICTOR_X0)
        for q, p in enumerate(pts):
            P[q * lph:q * lph + len(p)] = p
        Pd = torch.from_numpy(P).to(dev)
        J = torch.empty((n, M, 2), dtype=torch.float64, device=dev)
        sig = torch.empty(n, dtype=torch.int64, device=dev)
        it = torch.empty(n, dtype=torch.int32, device=dev)
        lib = _lib.lib()
        args = torch.empty(int(lib.pgw_pf_od_probe_args_size(H)), dtype=torch.uint8, device=dev)
        ph = (_lib.PFParams * H)(*[self._params_for_hour(hr) for hr in hours])
        od = _lib.PFOD.from_buffer_copy(self._od_proto)
        od.start = self._od_start[idx0].data_ptr()
        t = _lib.PFTables.from_buffer_copy(self.tables)
        t.od = _lib.C.addressof(od)
        _lib.check(lib.pgw_pf_od_probe(ph, H, t, self._od_start[idx0].data_ptr(), lph, n, Pd.data_ptr(),
                                       J.data_ptr(), sig.data_ptr(), it.data_ptr(), args.data_ptr(),
                                       _lib.stream_ptr(dev)))
        return J, sig.cpu().numpy().view(np.uint64), it.cpu().numpy(), np.arange(H) * lph

    def _od_vnode(self):
        """The node whose voltage the node records carry: the controllable
        load's, when it is one phase-to-ground element (C4, HET: 675c ->
        675.3); None otherwise (no node records)."""
        f = self.feeder
        if len(self._ctrl_names) != 1:
            return None
        li = f.load_names.index(self._ctrl_names[0])
        ks = [k for k in range(f.m) if f.elem_load[k] == li]
        if len(ks) != 1 or f.elem_q[ks[0]] >= 0:
            return None
        return int(f.elem_p[ks[0]])

    def _od_vcoef(self, recs):
        """Node-record coefficients [.., 3] complex (v0, v1, v2) of response
        records recs [.., R]: V_node = V0 + G J'(t), composed."""
        node, M = self._od_vnode(), self.M
        c = torch.view_as_complex(recs[..., 6:6 + 6 * M].reshape(*recs.shape[:-1], 3, M, 2).contiguous())
        G = torch.from_numpy(np.ascontiguousarray(self._od_Gall[node, :M])).to(recs.device)
        v = (c * G).sum(-1)
        v[..., 0] = v[..., 0] + complex(self._od_V0all[node])
        return v

    def _od_row_mask(self, idx):
        """pgw_pf_od.resp_rows of table row idx for the present output rows (0 =
        every row): the rows r >= 1 that can hold the minimum or the maximum
        |V| of an env the table serves.  Every served record's rows are
        V_r(t) = A_r + t (B_r + t C_r) (V0 + G J'(t) composed); |V_r|^2 over the
        piece's t range is bounded by 9 samples plus a Lipschitz margin plus
        1e-9 (far above the kernels' rounding and the node records' fit), and a
        row is kept when its lower bound reaches every row's upper bound (a
        minimum candidate) or its upper bound every row's lower bound (a maximum
        candidate) in some piece.  Cached per (row, configuration)."""
        key = (idx, self._cfg_version)
        if key in self._od_rowmask:
            return self._od_rowmask[key]
        names = list(self.output_names)
        mask = 0
        if self._od_resp is not None and 2 <= len(names) <= 64:
            f, M, dev = self.feeder, self.M, self.device
            recs = self._od_resp[idx]
            meta = recs.view(torch.int64)[:, 4]
            rr = recs[((meta & 0xffffffff) != 0) & (recs[:, 0] <= recs[:, 1])]
            if rr.shape[0]:
                rows = [f.node_index[nm] for nm in names]
                G = torch.from_numpy(np.ascontiguousarray(self._od_Gall[rows][:, :M])).to(dev)
                V0 = torch.from_numpy(np.ascontiguousarray(self._od_V0all[rows])).to(dev)
                c = torch.view_as_complex(rr[:, 6:6 + 6 * M].reshape(-1, 3, M, 2).contiguous())
                abc = torch.einsum("pqm,rm->pqr", c, G)                          # [P, 3, rows]
                tl, th = (rr[:, 0] - rr[:, 2]) * rr[:, 3], (rr[:, 1] - rr[:, 2]) * rr[:, 3]
                cand = extrema_candidates(abc[:, 0] + V0, abc[:, 1], abc[:, 2], tl, th)
                mask = sum(1 << r for r in range(1, len(names)) if cand[r]) if cand is not None else 0
        self._od_rowmask[key] = mask
        return mask

    OD_QROWS = 12                 # row records: listed output rows per record at most
    OD_QSTRIDE = 6 + 5 * 12       # doubles per row record (PGW_OD_REC_HEAD + 5 per row)

    def _od_qrows(self, idx):
        """pgw_pf_od.resp_q of table row idx for the present output rows: the
        rows that can hold a served env's extremum (_od_row_mask's candidates)
        and row 0, the node records' row excepted, each as |V_r(t)|^2 = a0 + t
        (a1 + t (a2 + t (a3 + t a4))) per record -- V_r(t) = A + t (B + t C),
        V0 + G J'(t) composed (the node records' composition), expanded in
        fp64.  Written into the row's slice of the row-record buffer with the
        response records' headers copied bitwise.  Returns (row bits, k) or None
        (no mask, more than OD_QROWS rows, no response table).  Cached per
        (row, configuration) and rebuilt when od_node_records or od_record_rows
        changed since: the listed rows leave out the node records' row only
        while that row has a node record to read."""
        key = (idx, self._cfg_version)
        flags = (bool(self.od_node_records), bool(self.od_record_rows))
        if key in self._od_qinfo and self._od_qflags.get(key) == flags:
            return self._od_qinfo[key]
        if key in self._od_qinfo:
            # the row's records are rewritten in place: tables handed out with
            # the old row set must not be used again
            self._tables_cache.clear()
            self._od_keep.clear()
            self.tables_version += 1
        self._od_qflags[key] = flags
        info = None
        mask = self._od_row_mask(idx)
        names = list(self.output_names)
        if mask and self._od_resp is not None:
            vnode = self._od_vnode()
            vrow = -1
            if self._od_vresp is not None and vnode is not None and self.od_node_records:
                nm = self.feeder.node_names[vnode]
                vrow = names.index(nm) if nm in names else -1
            rows = [r for r in [0] + [r for r in range(1, min(len(names), 64)) if (mask >> r) & 1] if r != vrow]
            if 0 < len(rows) <= self.OD_QROWS:
                f, M, dev = self.feeder, self.M, self.device
                R = _lib.od_rec(M)
                recs = self._od_resp[idx]                                              # [rec_n, R]
                if self._od_qrec is None:
                    self._od_qrec = torch.zeros((self.OD_MAX_TABLES, recs.shape[0], self.OD_QSTRIDE),
                                                dtype=torch.float64, device=dev)
                nodes = [f.node_index[names[r]] for r in rows]
                G = torch.from_numpy(np.ascontiguousarray(self._od_Gall[nodes][:, :M])).to(dev)
                V0 = torch.from_numpy(np.ascontiguousarray(self._od_V0all[nodes])).to(dev)
                c = torch.view_as_complex(recs[:, 6:6 + 6 * M].reshape(-1, 3, M, 2).contiguous())
                abc = torch.einsum("pqm,rm->pqr", c, G)                                 # [rec_n, 3, rows]
                A, B, C = abc[:, 0] + V0, abc[:, 1], abc[:, 2]
                re = lambda x, y: x.real * y.real + x.imag * y.imag                    # Re(x conj(y))
                q = torch.stack([re(A, A), 2.0 * re(A, B), re(B, B) + 2.0 * re(A, C), 2.0 * re(B, C), re(C, C)],
                                -1)                                                     # [rec_n, rows, 5]
                out = self._od_qrec[idx]
                out.zero_()
                out.view(torch.int64)[:, :6] = recs.view(torch.int64)[:, :6]
                out[:, 6:6 + 5 * len(rows)] = q.reshape(recs.shape[0], -1)
                # header word 5 (unused by the response records): per record, the
                # slots that can hold its own served envs' extremum -- the rows
                # compared are the listed ones and the node records' row
                if self.od_record_rows:
                    if vrow > 0:
                        gv = f.node_index[names[vrow]]
                        Gv = torch.from_numpy(np.ascontiguousarray(self._od_Gall[[gv]][:, :M])).to(dev)
                        V0v = torch.from_numpy(np.ascontiguousarray(self._od_V0all[[gv]])).to(dev)
                        av = torch.einsum("pqm,rm->pqr", c, Gv)
                        A, B, C = torch.cat([A, av[:, 0] + V0v], 1), torch.cat([B, av[:, 1]], 1), \
                            torch.cat([C, av[:, 2]], 1)
                    tl, th = (recs[:, 0] - recs[:, 2]) * recs[:, 3], (recs[:, 1] - recs[:, 2]) * recs[:, 3]
                    cand = extrema_candidates_per_piece(A, B, C, tl, th)[:, :len(rows)]
                    bits = (cand.to(torch.int64) << torch.arange(len(rows), device=dev)[None, :]).sum(1)
                    out.view(torch.int64)[:, 5] = bits
                    st_ = self.od_resp_stats
                    st_["record_rows_listed"] = st_.get("record_rows_listed", 0) + int(cand.shape[0]) * len(rows)
                    st_["record_rows_candidates"] = st_.get("record_rows_candidates", 0) + int(cand.sum())
                info = (sum(1 << r for r in rows), len(rows))
        self._od_qinfo[key] = info
        return info

    def _od_response(self, hours, idx0):
        """Build and upload the response tables of `hours` (rows idx0.. of the
        start tables).  Control flow and bookkeeping here; every solve, fit and
        fit check runs on the device."""
        import time as _time
        t_start = _time.perf_counter()
        M, H, dev = self.M, len(hours), self.device
        x0, h, nseg = self.PREDICTOR_X0, self.PREDICTOR_H, self.PREDICTOR_N - 1
        R = _lib.od_rec(M)
        rec_n = nseg + self.OD_RESP_EXTRA
        if self._od_resp is None:
            self._od_resp = torch.empty((self.OD_MAX_TABLES, rec_n, R), dtype=torch.float64, device=dev)
        lib, st = _lib.lib(), _lib.stream_ptr(dev)
        blk = self._od_resp[idx0:idx0 + H]
        blk[:, :, 0] = float("inf")                        # lo > hi: no piece
        blk[:, :, 1] = -float("inf")
        # (k*, next) as two int32 in one double: written through an int64 view
        # (the pattern of next = -1 is a NaN, which float paths may canonicalise)
        blk.view(torch.int64)[:, :, 4] = self._od_meta_word(0, -1)
        x = x0 + h * np.arange(nseg + 1)
        # ---- 1. every segment's ends and midpoint
        pts = x0 + 0.5 * h * np.arange(2 * nseg + 1)
        Jg, sg, itg, og = self._od_probe(hours, idx0, [pts] * H)
        lanes = og[:, None] + np.arange(2 * nseg + 1)[None, :]
        S_ = sg[lanes]                                      # [H, 2 nseg + 1]
        clean = (S_[:, 0:-1:2] == S_[:, 1::2]) & (S_[:, 1::2] == S_[:, 2::2])
        # ---- 2. segments with a breakpoint: sample, then bracket every change
        dq, dj = np.nonzero(~clean)
        sub = np.arange(self.OD_RESP_SUB + 1) / self.OD_RESP_SUB
        per = [[] for _ in range(H)]
        for i, (q, j) in enumerate(zip(dq, dj)):
            per[q].append(i)
        brk = []                                            # (i = dirty index, lo, hi, s_lo, s_hi)
        if len(dq):
            Jd, sd, _, od_ = self._od_probe(hours, idx0, [np.concatenate([x[dj[i]] + h * sub for i in per[q]])
                                                           if per[q] else np.zeros(0) for q in range(H)])
            ns = len(sub)
            for q in range(H):
                for r, i in enumerate(per[q]):
                    s = sd[od_[q] + r * ns: od_[q] + (r + 1) * ns]
                    for k in np.nonzero(s[1:] != s[:-1])[0]:
                        brk.append((i, x[dj[i]] + h * sub[k], x[dj[i]] + h * sub[k + 1], s[k], s[k + 1]))
            del Jd
        done, gaps, passes = [], [], 0
        work = brk
        while work and passes < self.OD_RESP_PASSES:
            passes += 1
            I = np.array([w[0] for w in work])
            lo = np.array([w[1] for w in work])
            hi = np.array([w[2] for w in work])
            slo = np.array([w[3] for w in work], np.uint64)
            shi = np.array([w[4] for w in work], np.uint64)
            hi0, tgt = hi.copy(), shi.copy()
            qs = dq[I]
            for _ in range(self.OD_RESP_BISECT):
                mid = 0.5 * (lo + hi)
                order = [np.nonzero(qs == q)[0] for q in range(H)]
                _, sm, _, om = self._od_probe(hours, idx0, [mid[o] for o in order])
                smid = np.empty(len(mid), np.uint64)
                for q, o in enumerate(order):
                    smid[o] = sm[om[q]: om[q] + len(o)]
                left = smid == slo
                lo = np.where(left, mid, lo)
                hi = np.where(left, hi, mid)
                shi = np.where(left, shi, smid)
            nxt = []
            for k in range(len(work)):
                done.append((I[k], lo[k], hi[k], slo[k], shi[k]))
                if shi[k] != tgt[k]:                        # a further breakpoint in (hi, hi0]
                    nxt.append((I[k], hi[k], hi0[k], shi[k], tgt[k]))
            work = nxt
        for w in work:                                      # unresolved: left to the solve
            gaps.append(w)
        # ---- 3. pieces: clean segments one each, the others between brackets
        pieces = []          # (q, j, a, b, sig, it, lane triple or None)
        cq, cj = np.nonzero(clean)
        n_clean = len(cq)
        by_seg = {}
        for (i, lo_, hi_, s0, s1) in done:
            by_seg.setdefault(i, []).append((lo_, hi_, s0, s1))
        for (i, lo_, hi_, s0, s1) in gaps:
            by_seg.setdefault(i, []).append((lo_, hi_, None, None))
        dirty_pieces = []    # (q, j, a, b, sig)
        for i, (q, j) in enumerate(zip(dq, dj)):
            a, sa = x[j], S_[q, 2 * j]
            for lo_, hi_, s0, s1 in sorted(by_seg.get(i, []), key=lambda z: z[0]):
                if s0 is not None and lo_ - a >= self.OD_RESP_MIN_WIDTH and s0 == sa:
                    dirty_pieces.append((q, j, a, lo_, sa))
                a, sa = hi_, s1
            if sa is not None and x[j + 1] - a >= self.OD_RESP_MIN_WIDTH and sa == S_[q, 2 * j + 2]:
                dirty_pieces.append((q, j, a, x[j + 1], sa))
        # fit points of the pieces between brackets
        nd = len(dirty_pieces)
        if nd:
            fq = np.array([p[0] for p in dirty_pieces])
            fa = np.array([p[2] for p in dirty_pieces])
            fb = np.array([p[3] for p in dirty_pieces])
            fs = np.array([p[4] for p in dirty_pieces], np.uint64)
            order = [np.nonzero(fq == q)[0] for q in range(H)]
            Jf, sf, itf, of_ = self._od_probe(hours, idx0, [np.stack([fa[o], 0.5 * (fa[o] + fb[o]), fb[o]], 1).ravel()
                                                             for o in order])
            f_lanes = np.empty((nd, 3), np.int64)
            for q, o in enumerate(order):
                f_lanes[o] = of_[q] + np.arange(3 * len(o)).reshape(-1, 3)
            f_ok = (sf[f_lanes] == fs[:, None]).all(1)
            f_it = itf[f_lanes[:, 1]]
        # ---- 4. records: segment j's first piece at record j, more in the extra slots
        extra = np.zeros(H, np.int64)
        rec_first = {}
        d_rec = np.empty(nd, np.int64)
        d_next = np.full(nd, -1, np.int64)
        prev = {}
        for k, (q, j, a, b, sg_) in enumerate(dirty_pieces):
            if (q, j) not in rec_first:
                rec_first[(q, j)] = k
                d_rec[k] = j
            elif extra[q] < self.OD_RESP_EXTRA:
                d_rec[k] = nseg + extra[q]
                extra[q] += 1
                d_next[prev[(q, j)]] = d_rec[k]
            else:
                d_rec[k] = -1                              # no room: left to the solve
                continue
            prev[(q, j)] = k
        row = (idx0 + np.arange(H)).astype(np.int64)

        T = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).to(dev)

        def fit(Jbuf, lanes3, a, b, it_, nxt, recs_global):
            n_ = len(a)
            if n_ == 0:
                return
            meta = np.stack([a, b, 0.5 * (a + b), 2.0 / (b - a)], 1)
            inext = np.stack([it_, nxt], 1).astype(np.int32)
            # (held by name until the kernel has run: a temporary's block could be
            # handed to the next allocation before the launch reads it)
            d3, dm, dn, dr = T(lanes3, np.int32), T(meta, np.float64), T(inext, np.int32), T(recs_global, np.int32)
            _lib.check(lib.pgw_pf_od_resp_fit(M, n_, Jbuf.data_ptr(), d3.data_ptr(), dm.data_ptr(), dn.data_ptr(),
                                              dr.data_ptr(), self._od_resp.data_ptr(), st))
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)

        c_lanes = og[cq][:, None] + 2 * cj[:, None] + np.arange(3)[None, :]
        c_rec = row[cq] * rec_n + cj
        fit(Jg, c_lanes, x[cj], x[cj + 1], itg[c_lanes[:, 0]], np.full(n_clean, -1), c_rec)
        if nd:
            keep = d_rec >= 0
            d_it = np.where(f_ok, f_it, 0)
            fit(Jf, f_lanes[keep], fa[keep], fb[keep], d_it[keep], d_next[keep], row[fq[keep]] * rec_n + d_rec[keep])
        # ---- 5. check points t = +-1/2 of every fitted piece
        pa = np.concatenate([x[cj], fa[keep] if nd else np.zeros(0)])
        pb = np.concatenate([x[cj + 1], fb[keep] if nd else np.zeros(0)])
        pq_ = np.concatenate([cq, fq[keep] if nd else np.zeros(0, np.int64)])
        psig = np.concatenate([S_[cq, 2 * cj], fs[keep] if nd else np.zeros(0, np.uint64)])
        prec = np.concatenate([c_rec, (row[fq[keep]] * rec_n + d_rec[keep]) if nd else np.zeros(0, np.int64)])
        pit = np.concatenate([itg[c_lanes[:, 0]], d_it[keep] if nd else np.zeros(0, np.int32)])
        pnext = np.concatenate([np.full(n_clean, -1), d_next[keep] if nd else np.zeros(0, np.int64)])
        w = pb - pa
        chk = np.stack([pa + 0.25 * w, pa + 0.75 * w], 1)
        order = [np.nonzero(pq_ == q)[0] for q in range(H)]
        Jc, sc, _, oc = self._od_probe(hours, idx0, [chk[o].ravel() for o in order])
        c_l = np.empty((len(pa), 2), np.int64)
        for q, o in enumerate(order):
            c_l[o] = oc[q] + np.arange(2 * len(o)).reshape(-1, 2)
        err = torch.empty(2 * len(pa), dtype=torch.float64, device=dev)
        dr, dp, dq_ = T(np.repeat(prec, 2), np.int32), T(chk.ravel(), np.float64), T(c_l.ravel(), np.int32)
        _lib.check(lib.pgw_pf_od_resp_check(M, 2 * len(pa), self._od_resp.data_ptr(), dr.data_ptr(), dp.data_ptr(),
                                            Jc.data_ptr(), dq_.data_ptr(), err.data_ptr(), st))
        e_ = err.cpu().numpy().reshape(-1, 2).max(1)
        del dr, dp, dq_
        vnode = self._od_vnode()
        if vnode is not None and len(pa):
            # the node records' voltage at the same check points against the
            # probed currents composed exactly (relative error, as the currents')
            rr = self._od_resp.view(-1, R)[torch.from_numpy(prec).to(dev)]          # [P, R]
            vc = self._od_vcoef(rr)                                                 # [P, 3]
            tt = (torch.from_numpy(chk).to(dev) - rr[:, 2:3]) * rr[:, 3:4]          # [P, 2]
            vfit = vc[:, :1] + tt * (vc[:, 1:2] + tt * vc[:, 2:3])
            Jl = torch.view_as_complex(Jc.reshape(-1, M, 2)[torch.from_numpy(c_l.ravel()).to(dev)].contiguous())
            G = torch.from_numpy(np.ascontiguousarray(self._od_Gall[vnode, :M])).to(dev)
            vtrue = ((Jl * G).sum(-1) + complex(self._od_V0all[vnode])).reshape(-1, 2)
            ev = ((vfit - vtrue).abs() / vtrue.abs()).max(1).values.cpu().numpy()
            e_ = np.maximum(e_, np.where(np.isfinite(ev), ev, np.inf))
        bad = (pit != 0) & ((e_ > self.OD_RESP_TOL) | (sc[c_l] != psig[:, None]).any(1) | ~np.isfinite(e_))
        # ---- 6. certificates (od_certify): every band and stopping decision of
        # the snap solve proven constant over the served interval; a piece is cut
        # to its longest certified run, or left to the solve
        cand = np.nonzero((pit != 0) & ~bad)[0]
        n_cut, kw_cut, t_cert = 0, 0.0, _time.perf_counter()
        if self.od_certify and len(cand):
            from powergridworld_amd.distribution_system.od_certify import SnapModel, certify_pieces
            model = SnapModel.from_solver(self, list(range(idx0, idx0 + H)), hours)
            model.native = bool(self.od_certify_native)
            c_lo, c_hi, c_kw = certify_pieces(model, pq_[cand], pa[cand], pb[cand], pit[cand], psig[cand],
                                              min_width=self.OD_RESP_MIN_WIDTH)
            none = c_lo > c_hi
            bad[cand[none]] = True
            cut = ~none & ((c_lo > pa[cand]) | (c_hi < pb[cand]))
            n_cut = int(cut.sum())
            kw_cut = float(((pb - pa)[cand] - np.where(none, 0.0, c_hi - c_lo)).sum())
            if n_cut:
                hdr = torch.from_numpy(np.stack([c_lo[cut], c_hi[cut]], 1)).to(dev)
                self._od_resp.view(-1, R)[torch.from_numpy(prec[cand[cut]]).to(dev), 0:2] = hdr
        t_cert = _time.perf_counter() - t_cert
        if bad.any():                                       # left to the solve
            words = np.array([self._od_meta_word(0, int(nx)) for nx in pnext[bad]], np.int64)
            self._od_resp.view(-1, R).view(torch.int64)[torch.from_numpy(prec[bad]).to(dev), 4] = \
                torch.from_numpy(words).to(dev)
        ok = (pit != 0) & ~bad
        if vnode is not None:                               # node records: headers copied bitwise
            if self._od_vresp is None:
                self._od_vresp = torch.zeros((self.OD_MAX_TABLES, rec_n, _lib.OD_VREC), dtype=torch.float64,
                                             device=dev)
            vb = self._od_vresp[idx0:idx0 + H]
            vb.view(torch.int64)[:, :, :6] = blk.view(torch.int64)[:, :, :6]
            vb[:, :, 6:12] = torch.view_as_real(self._od_vcoef(blk)).reshape(H, rec_n, 6)
        # the extrema rows of the rebuilt table rows (computed here, with the
        # build, not at the first step of each hour)
        for q in range(H):
            for k in [k for k in self._od_rowmask if k[0] == idx0 + q]:
                del self._od_rowmask[k]
            for k in [k for k in self._od_qinfo if k[0] == idx0 + q]:
                del self._od_qinfo[k]
            self._od_row_mask(idx0 + q)
            self._od_qrows(idx0 + q)
        # the brackets per table row (kW intervals the tables leave to the solve;
        # an hour's row: _od_index[_hour_key(hour)]), for tests and diagnostics
        for q, hr in enumerate(hours):
            self.od_resp_brackets[idx0 + q] = np.array(sorted((lo_, hi_) for (i, lo_, hi_, _, _) in done + gaps
                                                        if dq[i] == q)).reshape(-1, 2)
        st_ = self.od_resp_stats
        st_["hours"] = st_.get("hours", 0) + H
        st_["segments_with_breakpoints"] = st_.get("segments_with_breakpoints", 0) + len(dq)
        st_["brackets"] = st_.get("brackets", 0) + len(done)
        st_["unresolved_brackets"] = st_.get("unresolved_brackets", 0) + len(gaps)
        st_["pieces"] = st_.get("pieces", 0) + int(ok.sum())
        st_["pieces_left_to_solve"] = st_.get("pieces_left_to_solve", 0) + int((~ok).sum())
        st_["max_fit_err"] = max(st_.get("max_fit_err", 0.0), float(e_[ok].max()) if ok.any() else 0.0)
        st_["certified"] = bool(self.od_certify)
        st_["certified_pieces"] = st_.get("certified_pieces", 0) + (int(ok.sum()) if self.od_certify else 0)
        st_["pieces_cut_by_certificate"] = st_.get("pieces_cut_by_certificate", 0) + n_cut
        st_["uncertified_kw"] = st_.get("uncertified_kw", 0.0) + kw_cut
        st_["certify_s"] = st_.get("certify_s", 0.0) + t_cert
        st_["build_s"] = st_.get("build_s", 0.0) + (_time.perf_counter() - t_start)

    def _od_tables(self, hour):
        key = (hour, self._cfg_version)
        t = self._tables_cache.get(key)
        if t is not None:
            return t
        idx = self._od_index.get(self._hour_key(hour))
        if idx is None:
            self._od_starts(hour)
            idx = self._od_index[self._hour_key(hour)]
        od = _lib.PFOD.from_buffer_copy(self._od_proto)
        od.start = self._od_start[idx].data_ptr()
        od.resp_v_row = -1
        if self.od_table and self._od_resp is not None and len(self._ctrl_names) <= 1:
            od.resp = self._od_resp[idx].data_ptr()
            od.resp_x0, od.resp_h, od.resp_nseg = self.PREDICTOR_X0, self.PREDICTOR_H, self.PREDICTOR_N - 1
            od.resp_rows = self._od_row_mask(idx) if self.od_row_masks else 0
            vnode = self._od_vnode()
            if self._od_vresp is not None and vnode is not None and self.od_node_records:
                name = self.feeder.node_names[vnode]
                if name in self.output_names:
                    od.resp_v = self._od_vresp[idx].data_ptr()
                    od.resp_v_row = self.output_names.index(name)
            qi = self._od_qrows(idx) if self.od_row_records else None
            if qi is not None:
                od.resp_q, od.resp_q_rows, od.resp_q_k = self._od_qrec[idx].data_ptr(), qi[0], qi[1]
                od.resp_q_stride = self.OD_QSTRIDE
        t = _lib.PFTables.from_buffer_copy(self.tables)
        t.od = _lib.C.addressof(od)
        t._od_ref = od                     # the struct lives as long as these tables
        if len(self._tables_cache) > 4096:
            self._tables_cache.clear()
            self._od_keep.clear()
        self._tables_cache[key] = t
        self._od_keep[key] = od            # the tables hold its address
        return t

    # ------------------------------------------------------------ general kernel
    def _set_general_tables(self, idx):
        """Device tables of pgw_pf_solve_general (include/pgw.h): the iteration
        model's reduction (W, u0; check rows = every node for "opendss") and the
        output rows, in per unit (element / node bases), element-major, rows
        padded to chunks of 8 with inert zero-power elements."""
        f, fi, dev = self.feeder, self._fd_iter, self.device
        m = f.m
        mp = -(-m // 8) * 8
        self.M = mp
        no = len(idx)
        allidx = list(range(f.n))
        W, U0, G, V0o = fi.reduce_rows(idx)
        vb = f.elem_vbase
        vbn = f.kv_ln * 1000.0

        def emaj(rows_cm, ld):         # [rows, m] complex -> [mp][ld] complex, zero padded
            out = np.zeros((mp, ld), complex)
            out[:rows_cm.shape[1], :rows_cm.shape[0]] = rows_cm.T
            return out

        def dev_c(a):
            return torch.tensor(np.ascontiguousarray(a).view(np.float64).ravel(), dtype=torch.float64,
                                device=dev)
        Ws = W / (vb[:, None] * vb[None, :])
        u0 = np.zeros(mp, complex)
        u0[:m] = U0 / vb
        ldo = max(-(-no // 8) * 8, 8)
        Gs = (G / vb[None, :]) / vbn[idx][:, None]
        V0s = np.zeros(ldo, complex)
        V0s[:no] = V0o / vbn[idx]
        # RegControl: n_reg extra columns -- each row's response to the correction
        # currents c (amps) at the regulator nodes R: -(Z U)[row, R] in the row's pu
        reg = self.regulators
        nreg = 0
        if reg is not None:
            R, r = reg["nodes"], len(reg["nodes"])
            nreg = -(-r // 8) * 8
            ZR = fi.Z[:, R]                                        # [n, r]
            CZ = np.zeros((m, r), complex)
            for k in range(m):
                CZ[k] = ZR[f.elem_p[k]] - (ZR[f.elem_q[k]] if f.elem_q[k] >= 0 else 0.0)
            pad = lambda a: np.pad(a, ((0, 0), (0, nreg - r)))
            Ws_aug = np.hstack([np.pad(Ws, ((0, 0), (0, mp - m))), pad(-CZ / vb[:, None])])   # [m, mp + nreg]
            Gs_aug = np.hstack([np.pad(Gs, ((0, 0), (0, mp - m))), pad(-ZR[idx] / vbn[idx][:, None])])
            _, _, GR, V0R = fi.reduce_rows(list(R))
            rho = reg["rho"]
            V0rs = np.zeros(nreg, complex)
            V0rs[:r] = V0R / rho
            self._g_Greg = dev_c(emaj((GR / vb[None, :]) / rho[:, None], nreg))
            self._g_V0reg = dev_c(V0rs)

            def emaj_aug(rows_cm, ld):     # [rows, mp + nreg] -> [mp + nreg][ld]
                out = np.zeros((mp + nreg, ld), complex)
                out[:, :rows_cm.shape[0]] = rows_cm.T
                return out
            self._g_W = dev_c(emaj_aug(np.pad(Ws_aug, ((0, mp - m), (0, 0))), mp))
            self._g_G = dev_c(emaj_aug(Gs_aug, ldo))
        else:
            self._g_W = dev_c(emaj(Ws.T, mp))           # column k = W''[:, k]
            self._g_G = dev_c(emaj(Gs, ldo))
        if self.yprim == "step":
            # H1: the file model's reduction, kept for the hours' tables
            # (_h1_hour); the correction columns are the controllable elements'
            self._h1 = dict(Ws=Ws, u0=U0 / vb, Gs=Gs, V0o=V0o / vbn[idx], ldo=ldo, no=no, m=m, mp=mp,
                            emaj=emaj, dev_c=dev_c)
        self._g_nreg = nreg
        self._g_U0 = dev_c(u0)
        self._g_V0 = dev_c(V0s)
        n_chk = 0
        self._g_Gc = self._g_V0c = None
        if self.convergence == "opendss":
            _, _, Gc, V0c = fi.reduce_rows(allidx)
            n_chk = -(-f.n // 8) * 8
            if n_chk > _lib.PFG_MAX_CHK:
                raise ValueError("feeder has %d nodes (max %d for convergence='opendss')"
                                 % (f.n, _lib.PFG_MAX_CHK))
            V0cs = np.zeros(n_chk, complex)
            V0cs[:f.n] = V0c / vbn
            Gcs = (Gc / vb[None, :]) / vbn[:, None]
            if self._h1 is not None:
                self._h1.update(Gcs=Gcs, V0c=V0c / vbn, n_chk=n_chk)
            if reg is not None:
                Gcs = np.hstack([np.pad(Gcs, ((0, 0), (0, mp - m))), pad(-ZR / vbn[:, None])])
                self._g_Gc = dev_c(emaj_aug(Gcs, n_chk))
            else:
                self._g_Gc = dev_c(emaj(Gcs, n_chk))
            self._g_V0c = dev_c(V0cs)
        self._g_n_chk = n_chk
        self._vmin = torch.zeros(self.num_envs, dtype=torch.float64, device=dev)
        self._vmax = torch.zeros(self.num_envs, dtype=torch.float64, device=dev)
        self._all_nodes = len(idx) == f.n
        self.v_out = torch.zeros((max(no, 1), self.num_envs), dtype=torch.float64, device=dev)
        self._own_v_out = self.v_out
        self._bv_cache = {}
        self._iters = torch.zeros(self.num_envs, dtype=torch.int32, device=dev)
        self._base_params()

    def _h1_hour(self, hour):
        """yprim='step': the hour's reduction with every load's Yeq at the hour's
        powers (the controllable loads' base part included), from the file
        model's by the Yeq change dD: u = U0 + W J' with J' = (conj(S) g - D) u
        gives W_h = (I - W dD)^-1 W, U0_h = (I - W dD)^-1 U0, and any row read
        out as V = V0 + G J' becomes V0 + G dD U0_h + G (I + dD W_h) J'.  The
        controllable elements' columns (W_h, G_h, Gc_h) follow as the
        correction columns, their rows of W_h / U0_h as the correction's x.
        Cached per (hour, configuration) on the device."""
        key = (hour, self._cfg_version)
        c = self._h1_cache.get(key)
        if c is not None:
            return c
        H, f = self._h1, self.feeder
        m, mp, ldo, no, n_chk = H["m"], H["mp"], H["ldo"], H["no"], H["n_chk"]
        emaj, dev_c = H["emaj"], H["dev_c"]
        coef, resc = float(self.annual_hourly_load_profile[hour]), float(self.system_load_rescale_factor)
        dD = np.zeros(m, complex)
        for k in range(m):
            if f.elem_model[k] == 1:               # the kernel's (coef * base) * rescale; other models fixed
                li = f.elem_load[k]
                dP = (coef * f.base_kw[li]) * resc - f.base_kw[li]
                dQ = (coef * f.base_kvar[li]) * resc - f.base_kvar[li]
                dD[k] = complex(dP * 1000.0 / f.elem_nph[k], -(dQ * 1000.0 / f.elem_nph[k]))
        Ws, u0 = H["Ws"], H["u0"]
        A = np.eye(m) - Ws * dD[None, :]
        Wh = np.linalg.solve(A, Ws)
        U0h = np.linalg.solve(A, u0)
        rows = lambda G, V0: (G + (G * dD[None, :]) @ Wh, V0 + (G * dD[None, :]) @ U0h)
        Gh, V0h = rows(H["Gs"], H["V0o"])
        Gch, V0ch = rows(H["Gcs"], H["V0c"])
        C = self._h1_ctrl
        r, nreg = len(C), (8 if self._h1_ctrl else 0)
        pad_c = lambda M: np.pad(M[:, C], ((0, 0), (0, nreg - r))) if nreg else np.zeros((M.shape[0], 0), complex)

        def emaj_aug(rows_cm, ld):                 # [rows, mp + nreg] -> [mp + nreg][ld]
            out = np.zeros((mp + nreg, ld), complex)
            out[:, :rows_cm.shape[0]] = rows_cm.T
            return out
        W_aug = np.hstack([np.pad(Wh, ((0, 0), (0, mp - m))), pad_c(Wh)])          # [m, mp + nreg]
        G_aug = np.hstack([np.pad(Gh, ((0, 0), (0, mp - m))), pad_c(Gh)])
        Gc_aug = np.hstack([np.pad(Gch, ((0, 0), (0, mp - m))), pad_c(Gch)])
        u0p = np.zeros(mp, complex)
        u0p[:m] = U0h
        V0p = np.zeros(ldo, complex)
        V0p[:no] = V0h
        V0cp = np.zeros(n_chk, complex)
        V0cp[:len(V0ch)] = V0ch
        c = dict(W=dev_c(emaj_aug(np.pad(W_aug, ((0, mp - m), (0, 0))), mp)), U0=dev_c(u0p),
                 G=dev_c(emaj_aug(G_aug, ldo)), V0=dev_c(V0p), Gc=dev_c(emaj_aug(Gc_aug, n_chk)), V0c=dev_c(V0cp))
        if nreg:
            V0r = np.zeros(nreg, complex)
            V0r[:r] = U0h[C]
            c.update(Greg=dev_c(emaj(Wh[C, :], nreg)), V0reg=dev_c(V0r),
                     Wcc=torch.tensor(Wh[np.ix_(C, C)], dtype=torch.complex128, device=self.device),
                     nph=torch.tensor([float(f.elem_nph[k]) for k in C], dtype=torch.float64, device=self.device),
                     slot=[self._ctrl_names.index(f.load_names[f.elem_load[k]]) for k in C])
        if len(self._h1_cache) > 64:
            self._h1_cache.clear()
        self._h1_cache[key] = c
        return c

    def _h1_tables(self, hour, cp, cq):
        """yprim='step': PFGTables of this solve -- the hour's reduction and the
        per-env correction K = (I - D W_cc)^-1 D of the controllable elements'
        Yeq change D (diag, the env's controllable conj(S) per phase: the
        kernel's own y0' change), its upper triangle in Kreg."""
        c = self._h1_hour(hour)
        t = _lib.PFGTables.from_buffer_copy(self.tables)
        t.W, t.U0, t.G, t.V0 = c["W"].data_ptr(), c["U0"].data_ptr(), c["G"].data_ptr(), c["V0"].data_ptr()
        t.Gc, t.V0c = c["Gc"].data_ptr(), c["V0c"].data_ptr()
        keep = [c]
        if "Greg" in c:
            n, dev, r = self.num_envs, self.device, len(self._h1_ctrl)
            z = torch.zeros(n, dtype=torch.float64, device=dev)
            pk = torch.stack([cp[s] if cp is not None else z for s in c["slot"]])          # [r, n] kW
            qk = torch.stack([cq[s] if cq is not None else z for s in c["slot"]])
            d = torch.complex((pk * 1000.0) / c["nph"][:, None], -((qk * 1000.0) / c["nph"][:, None])).t()  # [n, r]
            if r == 1:
                K = (d[:, 0] / (1.0 - d[:, 0] * c["Wcc"][0, 0]))[None]                          # [1, n]
            else:
                Mx = torch.eye(r, dtype=torch.complex128, device=dev)[None] - d[:, :, None] * c["Wcc"][None]
                Kf = torch.linalg.solve(Mx, torch.diag_embed(d))                                 # [n, r, r]
                iu = torch.triu_indices(r, r, device=dev)
                K = Kf[:, iu[0], iu[1]].t()                                                      # [r(r+1)/2, n]
            Kreg = torch.view_as_real(K.contiguous()).contiguous()                               # [r(r+1)/2, n, 2]
            if getattr(self, "_h1_scratch", None) is None or self._h1_scratch[0].shape[1] != n:
                self._h1_scratch = (torch.zeros((8, n, 2), dtype=torch.float64, device=dev),
                                    torch.zeros((8, n, 2), dtype=torch.float64, device=dev),
                                    torch.ones(8, dtype=torch.float64, device=dev))
            rx, rc, rho = self._h1_scratch
            t.Greg, t.V0reg, t.Kreg = c["Greg"].data_ptr(), c["V0reg"].data_ptr(), Kreg.data_ptr()
            t.reg_x, t.reg_c, t.reg_rho = rx.data_ptr(), rc.data_ptr(), rho.data_ptr()
            keep.append(Kreg)
        t._keep = keep                             # (the tensors live as long as these tables)
        return t

    def _general_elems(self):
        """pgw_pfg_elem per (padded) element: the load's base kW / kvar, its
        phases, the Yeq power in OpenDSS's Y ("opendss"), the voltage band and
        the controllable slot."""
        f, mp = self.feeder, self.M
        arr = (_lib.PFGElem * mp)()
        for k in range(mp):
            e = arr[k]
            if k < f.m:
                li = f.elem_load[k]
                ld = f.spec["loads"][li]
                e.base_kw, e.base_kvar, e.nph = f.base_kw[li], f.base_kvar[li], f.elem_nph[k]
                if self.convergence == "opendss":
                    e.y0r = f.base_kw[li] * 1000.0 / f.elem_nph[k]
                    e.y0i = -(f.base_kvar[li] * 1000.0 / f.elem_nph[k])
                e.vlo2, e.vmn2, e.vmx2 = f.elem_vlow[k] ** 2, f.elem_vmin[k] ** 2, f.elem_vmax[k] ** 2
                e.model = int(f.elem_model[k])
                e.exp_p, e.exp_q = float(ld.get("cvrwatts", 1.0)), float(ld.get("cvrvars", 2.0))
                if e.model == 8:
                    z = ld.get("zipv") or [1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
                    if len(z) != 7:
                        raise ValueError("load %s: ZIPV needs 7 values, got %d" % (ld["name"], len(z)))
                    for i in range(6):
                        e.zip[i] = float(z[i])
                    e.vcut2 = float(z[6]) ** 2
                ln = f.load_names[li]
                e.ctrl = self._ctrl_names.index(ln) if ln in self._ctrl_names else -1
            else:
                e.nph, e.vlo2, e.vmn2, e.vmx2, e.ctrl, e.model = 1.0, 0.25, 0.9025, 1.1025, -1, 1
        return arr

    def set_controllable_loads(self, names):
        """Load names that receive per-env controllable P/Q (<= 8)."""
        names = [n for n in names if n in self.load_bus_name]
        if len(names) > _lib.PF_MAX_CTRL:
            raise ValueError("at most %d controllable loads" % _lib.PF_MAX_CTRL)
        if names != self._ctrl_names:
            self._ctrl_names = names
            self._seen_keys = None
            if self._prev_fast and not self.prev_fast_serves(names):
                # snap_start="previous": the fast kernel takes one controllable
                # load; anything else runs the general kernel (U_init / U_out)
                self._od_fast, self.general, self._prev_fast = False, True, False
                self.set_output_nodes(self.output_names)
            elif self._h1_fast and not self.h1_fast_serves(names):
                # yprim="step": the fast kernel takes one controllable load of
                # one phase element; anything else runs the general kernel
                self._od_fast, self.general, self._h1_fast = False, True, False
                self.set_output_nodes(self.output_names)
            elif self._od_fast and not self._h1_fast and len(names) > 1 and self.multi_bus != "fast":
                # several controllable slots run the general kernel unless
                # multi_bus="fast" asks for the fast kernel's multi-slot
                # instantiation (k_pf_solve_od_ms: no response table)
                self._od_fast, self.general = False, True
                self.set_output_nodes(self.output_names)
            else:
                self._base_params()
                if self._prev_fast:
                    self._prev_restart()

    def prev_fast_serves(self, names):
        """snap_start="previous", start_kernel="fast": whether the fast kernel
        serves these controllable loads -- none, or one load (of any number of
        phase elements: Y is the DSS file's, there is no per-env correction)."""
        names = [n for n in names if n in self.load_bus_name]
        return self._prev_fast and len(names) <= 1

    def _prev_restart(self):
        """snap_start="previous" on the fast kernel: the chain starts over --
        every env's column of the state buffer takes the direct solution
        (pgw_pf_prev_reset), where the general route drops its warm tables."""
        if self._prev_U is None or tuple(self._prev_U.shape) != (2 * self.M, self.num_envs):
            self._prev_U = torch.zeros((2 * self.M, self.num_envs), dtype=torch.float64, device=self.device)
        _lib.check(_lib.lib().pgw_pf_prev_reset(self.params, self.tables, self._prev_U.data_ptr(), self.num_envs,
                                                _lib.stream_ptr(self.device)))

    def _prev_tables(self):
        """snap_start="previous" on the fast kernel: the one PFTables of the
        configuration -- the DSS file's block and rows, od without a
        first-iteration or response table (the hour enters through step_params
        only)."""
        t = self._prev_keepalive
        if t is None or t._cfg != self._cfg_version:
            od = _lib.PFOD.from_buffer_copy(self._od_proto)
            od.start = od.resp = od.resp_v = od.resp_q = None
            od.resp_v_row = -1
            t = _lib.PFTables.from_buffer_copy(self.tables)
            t.od = _lib.C.addressof(od)
            t._od_ref, t._cfg = od, self._cfg_version     # (the struct lives as long as these tables)
            self._prev_keepalive = t
        return t

    def h1_fast_serves(self, names):
        """yprim="step", step_kernel="fast": whether the fast kernel serves these
        controllable loads -- none, or one load of one phase element."""
        f = self.feeder
        names = [n for n in names if n in self.load_bus_name]
        elems = [k for k in range(f.m) if f.load_names[f.elem_load[k]] in names]
        return self._h1_fast and len(names) <= 1 and len(elems) == len(names)

    def _h1f_tables(self, hour):
        """yprim="step" on the fast kernel: the hour's PFTables -- the packed
        block of (W_h, u0_h) with output row 0, the output rows, every check row
        (n_rep = n_rows: the bound constants hold for the file model's rows, not
        the hour's) -- with pgw_pf_h1 (the controllable element, W_h[:, c]) as
        its `_h1`.  One upload per (hour, configuration), cached on the device."""
        key = (hour, self._cfg_version)
        t = self._h1f_cache.get(key)
        if t is not None:
            return t
        M, od0, p = self.M, self._od_proto, self._params_for_hour(hour)
        ctrl = [k for k in range(M) if p.elem_ctrl[k] == 0]
        elem = ctrl[0] if len(ctrl) == 1 and p.n_ctrl == 1 else -1
        rows = self._od_row_idx
        y0 = np.array(od0.y0r[:M]) + 1j * np.array(od0.y0i[:M])
        c = h1_hour_tables(self._od_W2, self._od_u0, y0, np.array(p.base_kw[:M]), np.array(p.base_kvar[:M]),
                           np.array(p.nph[:M]), self._od_Gall[self._out_idx], self._od_V0all[self._out_idx],
                           self._od_Gall[rows] if rows else np.zeros((1, M), complex),
                           self._od_V0all[rows] if rows else np.zeros(1, complex), elem)
        vb = np.array(p.vbase[:M])
        flat = lambda a: np.ascontiguousarray(a, dtype=complex).view(np.float64).ravel()
        block = np.zeros(int(_lib.lib().pgw_pf_pack_size(M)))
        cp = lambda a: a.ctypes.data_as(_lib.C.c_void_p)
        no = len(self._out_idx)
        G0 = flat(c["G"][0]) if no else np.zeros(2 * M)
        V00 = flat(c["V0"][:1]) if no else np.zeros(2)
        # (pgw_pf_pack divides by the element bases: hand it volts)
        Wv, U0v = flat(c["W"] * (vb[:, None] * vb[None, :])), flat(c["u0"] * vb)
        _lib.check(_lib.lib().pgw_pf_pack(p, cp(Wv), cp(U0v), cp(G0), cp(V00), cp(block)))
        parts = [block, flat(c["G"]) if no else np.zeros(2 * M), flat(c["V0"]) if no else np.zeros(2),
                 flat(c["V0c"]), flat(c["Gc"])]
        offs = np.cumsum([0] + [len(a) for a in parts])
        buf = torch.tensor(np.concatenate(parts), dtype=torch.float64, device=self.device)
        at = lambda i: buf.data_ptr() + 8 * int(offs[i])
        od = _lib.PFOD.from_buffer_copy(od0)
        od.rows_V0, od.rows_G, od.start = at(3), at(4), None
        od.n_rep = od.n_rows                       # every check row evaluated
        od.resp = od.resp_v = od.resp_q = None
        od.resp_v_row = -1
        t = _lib.PFTables.from_buffer_copy(self.tables)
        t.block, t.G, t.V0 = at(0), at(1), at(2)
        t.od = _lib.C.addressof(od)
        h = _lib.PFH1()
        h.elem = elem
        wc = flat(c["wc"])
        for i in range(2 * M):
            h.wc[i] = wc[i]
        t._h1, t._keep = h, (od, buf)              # (they live as long as these tables)
        if len(self._h1f_cache) > 64:
            self._h1f_cache.clear()
            self.tables_version += 1
        self._h1f_cache[key] = t
        return t

    def _base_params(self):
        if self.general:
            return self._base_params_general()
        f, M = self.feeder, self.M
        p = _lib.PFParams()
        for k in range(M):
            real = k < f.m
            p.vbase[k] = f.elem_vbase[k] if real else 1.0
            p.vmin[k] = f.elem_vmin[k] if real else 0.95
            p.vmax[k] = f.elem_vmax[k] if real else 1.05
            p.vlow[k] = f.elem_vlow[k] if real else 0.50
            p.nph[k] = f.elem_nph[k] if real else 1.0
            ln = f.load_names[f.elem_load[k]] if real else None
            p.elem_ctrl[k] = self._ctrl_names.index(ln) if ln in self._ctrl_names else -1
        p.tol, p.m, p.n_ctrl = self.tol, M, len(self._ctrl_names)
        p.n_out, p.max_iter = len(self.output_names), self.max_iter
        p.pred_x0, p.pred_h, p.pred_n = self.PREDICTOR_X0, self.PREDICTOR_H, self.PREDICTOR_N
        self.params = p
        self._cfg_version = getattr(self, "_cfg_version", 0) + 1
        # bumped whenever a PFTables handed out earlier may no longer be valid
        self.tables_version = getattr(self, "tables_version", 0) + 1
        self._step_cache = {}
        self._tables_cache = {}
        self._pred_index = {}
        self._od_index, self._od_keep = {}, {}     # (first-iteration tables depend on the slots)
        self._warm = None              # (cold, warm) PFTables over the previous solutions

    def _base_params_general(self):
        p = _lib.PFGParams()
        p.m, p.n_chk, p.n_out, p.n_ctrl = self.M, self._g_n_chk, len(self.output_names), len(self._ctrl_names)
        p.mode = _lib.PF_OPENDSS if self.convergence == "opendss" else _lib.PF_EXACT
        p.min_iter, p.max_iter, p.tol = self.min_iter, self.max_iter, self.tol
        p.coef, p.rescale = 1.0, float(self.system_load_rescale_factor)
        reg = self.regulators
        if reg is not None:
            p.n_reg, p.r_reg = self._g_nreg, len(reg["nodes"])
        if self.yprim == "step":
            f = self.feeder
            ctrl = [k for k in range(f.m) if f.load_names[f.elem_load[k]] in self._ctrl_names]
            if len(ctrl) > 8:
                raise ValueError("yprim='step': at most 8 controllable load phase elements, got %d" % len(ctrl))
            self._h1_ctrl = ctrl
            p.mode = _lib.PF_OPENDSS_STEP
            p.n_reg, p.r_reg = (8, len(ctrl)) if ctrl else (0, 0)
            self._h1_cache = {}
        self.params = p
        elems = self._general_elems()
        self._g_elem = torch.tensor(np.frombuffer(bytes(elems), np.uint8), device=self.device)
        self.tables = _lib.PFGTables(elem=self._g_elem.data_ptr(), W=self._g_W.data_ptr(),
                                     U0=self._g_U0.data_ptr(), G=self._g_G.data_ptr(),
                                     V0=self._g_V0.data_ptr(),
                                     Gc=self._g_Gc.data_ptr() if self._g_Gc is not None else None,
                                     V0c=self._g_V0c.data_ptr() if self._g_V0c is not None else None,
                                     v_min_out=self._vmin.data_ptr(), v_max_out=self._vmax.data_ptr())
        if reg is not None:
            t = self.tables
            t.Greg, t.V0reg = self._g_Greg.data_ptr(), self._g_V0reg.data_ptr()
            t.Kreg, t.reg_x, t.reg_c = self._Kreg.data_ptr(), self._reg_x.data_ptr(), self._reg_c.data_ptr()
            t.reg_rho = self._reg_rho.data_ptr()
        self._cfg_version = getattr(self, "_cfg_version", 0) + 1
        self.tables_version = getattr(self, "tables_version", 0) + 1
        self._step_cache = {}
        self._tables_cache = {}
        self._pred_index = {}
        self._warm = None

    def hour_of(self, current_time):
        """Hour of year of a step time (opendss.py:98-103), memoized per time."""
        h = self._hour_memo.get(current_time)
        if h is None:
            if len(self._hour_memo) > 1 << 16:
                self._hour_memo.clear()
            h = self._hour_memo[current_time] = get_hour_of_year(pd.Timestamp(current_time))
        return h

    def step_params(self, current_time):
        """PFParams with this step's base loads: loadshape[hour] * base * rescale
        (opendss.py:96-108).  Cached per (hour, configuration): the base loads
        only change hourly."""
        return self._params_for_hour(self.hour_of(current_time))

    def _params_for_hour(self, hour):
        key = (hour, self._cfg_version)
        p = self._step_cache.get(key)
        if p is not None:
            return p
        if self.general:      # the kernel forms (coef * base) * rescale per element
            p = _lib.PFGParams.from_buffer_copy(self.params)
            p.coef = float(self.annual_hourly_load_profile[hour])
            if len(self._step_cache) > 4096:
                self._step_cache.clear()
            self._step_cache[key] = p
            return p
        coef = self.annual_hourly_load_profile[hour]
        step_load = coef * self.base_load * self.system_load_rescale_factor
        f = self.feeder
        p = _lib.PFParams.from_buffer_copy(self.params)
        for k in range(self.M):
            real = k < f.m
            p.base_kw[k] = step_load[f.elem_load[k], 0] if real else 0.0
            p.base_kvar[k] = step_load[f.elem_load[k], 1] if real else 0.0
        if len(self._step_cache) > 4096:
            self._step_cache.clear()
        self._step_cache[key] = p
        return p

    def step_tables(self, current_time):
        """PFTables for this step: with a single controllable load, the per-hour
        predictor table is attached (PREDICTOR_N solutions on the kW grid).  A
        missing hour is solved on the device together with the next
        PREDICTOR_LOOKAHEAD - 1 hours in ONE launch (the hours differ only by
        the loadshape coefficient, passed as a per-env load scale), so an
        episode pays for about one table solve.  Otherwise the cold-start tables."""
        if self._h1_fast:
            return self._h1f_tables(self.hour_of(current_time))
        if self._prev_fast:
            return self._prev_tables()
        if self._od_fast:
            return self._od_tables(self.hour_of(current_time))
        if self.general or not (self.use_predictor and len(self._ctrl_names) == 1):
            return self.tables
        hour = self.hour_of(current_time)
        key = (hour, self._cfg_version)
        t = self._tables_cache.get(key)
        if t is not None:
            return t
        idx = self._pred_index.get(self._hour_key(hour))
        if idx is None:
            self._solve_tables(hour)
            idx = self._pred_index[self._hour_key(hour)]
        t = _lib.PFTables.from_buffer_copy(self.tables)
        t.U_pred = self._pred_table[idx].data_ptr()
        t.U_pred_meta = self._pred_meta[idx].data_ptr()
        if len(self._tables_cache) > 4096:
            self._tables_cache.clear()
        self._tables_cache[key] = t
        return t

    def _hour_key(self, hour):
        p = self._params_for_hour(hour)
        return (tuple(p.base_kw), tuple(p.base_kvar))

    def _solve_tables(self, hour):
        """Predictor tables for `hour` and the following hours of the year that
        have none yet (one k_pf_solve over n_hours x PREDICTOR_N grid points)."""
        hours, keys = [], []
        for h in range(hour, min(hour + self.PREDICTOR_LOOKAHEAD, len(self.annual_hourly_load_profile))):
            k = self._hour_key(h)
            if k not in self._pred_index and k not in keys:
                hours.append(h)
                keys.append(k)
        if len(self._pred_index) + len(keys) > self.PREDICTOR_MAX_TABLES:
            self._pred_index, self._tables_cache = {}, {}
            self.tables_version += 1
        idx0 = len(self._pred_index)
        for j, k in enumerate(keys):
            self._pred_index[k] = idx0 + j
        P, H = self.PREDICTOR_N, len(hours)
        # base loads at coefficient 1, per-env scale = loadshape[hour] (the same
        # product as step_params up to rounding; the table only seeds the solve)
        sp = _lib.PFParams.from_buffer_copy(self.params)
        base = self.base_load * self.system_load_rescale_factor
        f = self.feeder
        for k in range(self.M):
            real = k < f.m
            sp.base_kw[k] = base[f.elem_load[k], 0] if real else 0.0
            sp.base_kvar[k] = base[f.elem_load[k], 1] if real else 0.0
        sp.tol = min(self.tol, self.PREDICTOR_TOL)
        sp.max_iter = max(self.max_iter, 200)
        sp.n_out = 0
        dev = self.device
        scale = torch.tensor(np.repeat(self.annual_hourly_load_profile[hours], P), dtype=torch.float64,
                             device=dev)
        cp = self._pred_x.repeat(1, H)
        cq = torch.zeros_like(cp)
        if self._pred_grid is None or self._pred_grid.shape[0] < H * P:
            self._pred_grid = torch.empty((self.PREDICTOR_LOOKAHEAD * P, self.M, 2), dtype=torch.float64,
                                          device=dev)
        grid = self._pred_grid
        tb = _lib.PFTables.from_buffer_copy(self.tables)
        tb.U_pred = None
        tb.U_out = grid.data_ptr()
        tb.sig_out = self._pred_sig[idx0].data_ptr()
        tb.load_scale = scale.data_ptr()
        tb.v_min_out = tb.v_max_out = None         # (grid solves: H * P lanes, no output rows)
        st = _lib.stream_ptr(dev)
        lib = _lib.lib()
        _lib.check(lib.pgw_pf_solve(sp, tb, H * P, _lib.dptr(cp), _lib.dptr(cq), None, None, st))
        _lib.check(lib.pgw_pf_pred_meta(sp, H, P, grid.data_ptr(), self._pred_sig[idx0].data_ptr(),
                                        self._pred_meta[idx0].data_ptr(), st))
        _lib.check(lib.pgw_pf_pred_pack(sp, H, P, grid.data_ptr(), self._pred_table[idx0].data_ptr(), st))
        self._pred_keepalive = (scale, cp, cq)     # until the stream has consumed them

    # ------------------------------------------------------------ reference API
    def calculate_power_flow(self, p_controllable_consumed: dict = None,
                             q_controllable_consumed: dict = None, current_time: str = None) -> None:
        n = self.num_envs
        if p_controllable_consumed is not None:
            kt = (tuple(p_controllable_consumed), tuple(q_controllable_consumed or ()))
            if kt != self.__dict__.get("_seen_keys"):     # (checked once per key set)
                keys = [k for k in self.load_bus_name
                        if k in p_controllable_consumed or k in (q_controllable_consumed or {})]
                if not set(keys) <= set(self._ctrl_names):     # the controllable set only grows
                    grown = set(keys) | set(self._ctrl_names)
                    self.set_controllable_loads([k for k in self.load_bus_name if k in grown])
                self._seen_keys = kt
        p = self.step_params(current_time)
        cp = cq = None
        if self._ctrl_names and p_controllable_consumed is not None:
            zeros = None
            get = lambda d, k: as_env_tensor(d[k], n, self.device, k) if (d and k in d) else None
            ps = [get(p_controllable_consumed, k) for k in self._ctrl_names]
            qs = [get(q_controllable_consumed, k) for k in self._ctrl_names]
            if len(ps) == 1:                       # one load: a [1, N] view, no copy
                cp = ps[0].reshape(1, n) if ps[0] is not None else None
                cq = qs[0].reshape(1, n) if qs[0] is not None else None
                if cp is None:
                    cp = torch.zeros((1, n), dtype=torch.float64, device=self.device)
            else:
                zeros = torch.zeros(n, dtype=torch.float64, device=self.device)
                cp = torch.stack([x if x is not None else zeros for x in ps])
                cq = torch.stack([x if x is not None else zeros for x in qs])
        tables = self.solve_tables(current_time, cp is not None)
        if self.yprim == "step" and not self._h1_fast:
            tables = self._h1_tables(self.hour_of(current_time), cp, cq)
        fn = _lib.lib().pgw_pf_solve_general if self.general else _lib.lib().pgw_pf_solve
        if self.regulators is not None:
            self._solve_regulated(fn, p, tables, cp, cq)
        elif self._h1_fast:
            _lib.check(_lib.lib().pgw_pf_solve_h1(p, tables, tables._h1, n, _lib.dptr(cp), _lib.dptr(cq),
                                                  _lib.dptr(self.v_out), _lib.dptr(self._iters),
                                                  _lib.stream_ptr(self.device)))
        elif self._prev_fast:
            _lib.check(_lib.lib().pgw_pf_solve_prev(p, tables, self._prev_U.data_ptr(), n, _lib.dptr(cp),
                                                    _lib.dptr(cq), _lib.dptr(self.v_out), _lib.dptr(self._iters),
                                                    _lib.stream_ptr(self.device)))
        else:
            _lib.check(fn(p, tables, n, _lib.dptr(cp), _lib.dptr(cq), _lib.dptr(self.v_out),
                          _lib.dptr(self._iters), _lib.stream_ptr(self.device)))
        self.solved(tables)
        self.iterations = self._iters
        self._prepare_bus_voltages()
        if self._all_nodes:                        # the epilogue's min / max over every node
            self._extrema = (self._vmin, self._vmax)

    # ------------------------------------------------------------ RegControl
    # OpenDSS's snap solve with controls (SolveSnap): solve, sample every
    # control, execute the pending actions (STATIC: the nearest delay first),
    # repeat until no control acts or MaxControlIterations.  Taps persist
    # across solves and episodes, as the regulator objects do in the
    # reference's one OpenDSS circuit (opendss.py:36-39 compiles it once).
    OPENDSS_MAX_CONTROL_ITER = 15

    def _init_regulators(self):
        reg, n, dev = self.regulators, self.num_envs, self.device
        r = len(reg["nodes"])
        self.reg_taps = torch.tensor(np.repeat(reg["taps0"][:, None], n, 1), dtype=torch.float64, device=dev)
        # K per env, its upper triangle (pgw_pfg_tables.Kreg); DSS taps: K = 0
        self._Kreg = torch.zeros((r * (r + 1) // 2, n, 2), dtype=torch.float64, device=dev)
        self._reg_x = torch.zeros((r, n, 2), dtype=torch.float64, device=dev)
        self._reg_c = torch.zeros((r, n, 2), dtype=torch.float64, device=dev)
        self._reg_active = torch.ones(n, dtype=torch.int32, device=dev)
        self._reg_nchg = torch.zeros(1, dtype=torch.int32, device=dev)
        self._reg_S = torch.tensor(np.ascontiguousarray(reg["S"]).view(np.float64).ravel(), device=dev)
        self._reg_rho = torch.tensor(reg["rho"], dtype=torch.float64, device=dev)
        self._reg_params = _lib.reg_params(reg, self._reg_S.data_ptr(), self._reg_rho.data_ptr())
        # control_loop="device": the solves each env got in the last power flow
        # ([N] int32, written by the kernel: an output like iterations).  A
        # checkpoint saves and restores it like every tensor of the solver, in
        # place and together with _control_iterations (None = "ask the
        # device"), so control_iterations describes the restored step.
        self.control_passes = (torch.zeros(n, dtype=torch.int32, device=dev)
                               if self.control_loop == "device" else None)
        self.control_iterations = 0

    @property
    def control_iterations(self):
        """Control passes of the last power flow (the most any env took).  With
        control_loop="device" it is read from the device on request only
        (control_passes.max(): a synchronisation)."""
        it = self.__dict__.get("_control_iterations", 0)
        if it is None:
            it = self._control_iterations = int(self.control_passes.max())
        return it

    @control_iterations.setter
    def control_iterations(self, v):
        self._control_iterations = v

    def set_regulator_taps(self, taps):
        """Set every env's RegControl taps ([n_ctrl] or [n_ctrl, N], pu) and
        refactor the Woodbury correction for them."""
        t = torch.as_tensor(taps, dtype=torch.float64, device=self.device)
        self.reg_taps.copy_(t.reshape(len(self.regulators["ctrls"]), -1).expand_as(self.reg_taps))
        _lib.check(_lib.lib().pgw_reg_factor(self._reg_params, self.num_envs, self.reg_taps.data_ptr(), None,
                                             self._Kreg.data_ptr(), _lib.stream_ptr(self.device)))

    def _solve_regulated(self, fn, p, tables, cp, cq, v_out=None, iters=None):
        """The control loop (v_out / iters: the solver's own buffers unless given).  Exact mode: a re-solve after a tap move starts from
        the env's solution of the previous pass (U_init = U_out of the same
        per-env buffer) -- the fixed point to tol in a few iterations instead of
        ~11 from the direct solution; the result depends only on this call's
        inputs and the taps it started from.  (OpenDSS mode keeps its
        direct-solution start)"""
        n, st, lib = self.num_envs, _lib.stream_ptr(self.device), _lib.lib()
        v_out = self.v_out if v_out is None else v_out
        iters = self._iters if iters is None else iters
        t = type(tables).from_buffer_copy(tables)
        t.Kreg, t.reg_x, t.reg_c = self._Kreg.data_ptr(), self._reg_x.data_ptr(), self._reg_c.data_ptr()
        t.reg_rho = self._reg_rho.data_ptr()
        t.env_active = None
        warm = self.convergence == "exact"
        if warm:
            if getattr(self, "_reg_U", None) is None or self._reg_U.shape[1] != self.M:
                self._reg_U = torch.zeros((n, self.M, 2), dtype=torch.float64, device=self.device)
                self._reg_U_valid = False
            t.U_out = self._reg_U.data_ptr()
            if self.warm_start and self._reg_U_valid:
                # warm_start=True: the first pass too starts from the env's last
                # solution, as OpenDSS's snap solve does (history-dependent last bits)
                t.U_init = self._reg_U.data_ptr()
            self._reg_U_valid = True
        if self.control_loop == "device":
            # the same loop per block of 64 envs in one launch, no host sync
            _lib.check(lib.pgw_pf_solve_regulated(p, t, self._reg_params, n, _lib.dptr(cp), _lib.dptr(cq),
                                                  self.reg_taps.data_ptr(), self._Kreg.data_ptr(),
                                                  int(self.OPENDSS_MAX_CONTROL_ITER), _lib.dptr(v_out),
                                                  _lib.dptr(iters), self.control_passes.data_ptr(), st))
            self.control_iterations = None        # (control_passes.max() when asked for)
            return
        active = None
        for it in range(1, self.OPENDSS_MAX_CONTROL_ITER + 1):
            if warm and it == 2:
                t.U_init = self._reg_U.data_ptr()
            t.env_active = active
            _lib.check(fn(p, t, n, _lib.dptr(cp), _lib.dptr(cq), _lib.dptr(v_out), _lib.dptr(iters), st))
            self._reg_nchg.zero_()
            _lib.check(lib.pgw_reg_control(self._reg_params, n, self._reg_x.data_ptr(), self._reg_c.data_ptr(),
                                           self.reg_taps.data_ptr(), self._reg_active.data_ptr(),
                                           self._reg_nchg.data_ptr(), st))
            _lib.check(lib.pgw_reg_factor(self._reg_params, n, self.reg_taps.data_ptr(),
                                          self._reg_active.data_ptr(), self._Kreg.data_ptr(), st))
            self.control_iterations = it
            if int(self._reg_nchg.item()) == 0:          # (one host sync per control pass)
                break
            active = self._reg_active.data_ptr()

    def solve_tables(self, current_time, controllable=True):
        """The PFTables a solve at `current_time` uses: the hour's predictor tables
        (one controllable load), else the cold-start tables -- or, with
        warm_start, the ones over each env's previous solution."""
        tables = self.step_tables(current_time) if (controllable or self._od_fast) else self.tables
        if (controllable or self.snap_start == "previous") and self.warm_start and tables is self.tables:
            tables = self._warm_tables()
        return tables

    def solved(self, tables):
        """Call after a solve launched with solve_tables(): the warm-start buffer
        now holds a solution."""
        if self._warm is not None and tables is self._warm[0]:
            self._warm_valid = True

    def _warm_tables(self):
        """PFTables writing each env's converged element voltages into a per-env
        buffer (U_out) and, once it holds a solution, starting from it (U_init)."""
        if self._warm is None:
            if self._U_prev is None or self._U_prev.shape[1] != self.M:
                self._U_prev = torch.zeros((self.num_envs, self.M, 2), dtype=torch.float64, device=self.device)
            T = type(self.tables)
            cold = T.from_buffer_copy(self.tables)
            cold.U_out = self._U_prev.data_ptr()
            warm = T.from_buffer_copy(cold)
            warm.U_init = self._U_prev.data_ptr()
            self._warm, self._warm_valid = (cold, warm), False
        return self._warm[1] if self._warm_valid else self._warm[0]

    @property
    def iterations(self):
        """[N] int32 iteration count of the last solve per env (-max_iter =
        stopped unconverged)."""
        return self._iterations

    @iterations.setter
    def iterations(self, v):
        self._iterations = v

    def unconverged(self) -> int:
        """Envs whose last solve stopped at max_iter without meeting tol (the
        kernels report their count as -iterations).  Synchronises; never
        called on the step path."""
        return 0 if self.iterations is None else int((self.iterations < 0).sum())

    def bind_output(self, v_out=None):
        """Write the next solves' node voltages into `v_out` ([n_out, N] fp64, e.g.
        a slot of MultiAgentEnv's on-device voltage history) instead of the
        solver's own buffer; None restores the own buffer."""
        if v_out is None:
            v_out = self._own_v_out
        elif (v_out.dtype != torch.float64 or v_out.device != self._own_v_out.device or
              tuple(v_out.shape) != tuple(self._own_v_out.shape) or not v_out.is_contiguous()):
            raise ValueError("bind_output: need a contiguous fp64 [%d, %d] tensor on %s"
                             % (tuple(self._own_v_out.shape) + (self._own_v_out.device,)))
        self.v_out = v_out

    def _prepare_bus_voltages(self):
        """{node: [N] view of its v_out row}; the views stay valid across solves
        (one dict per output buffer, cached)."""
        key = (self.v_out.data_ptr(), self._names_ver)
        if getattr(self, "_bv_key", None) != key:
            cache = self.__dict__.setdefault("_bv_cache", {})
            bv = cache.get(key)
            if bv is None:
                if len(cache) > 8192:
                    cache.clear()
                bv = cache[key] = {name: self.v_out[i] for i, name in enumerate(self.output_names)}
            self._bv = bv
            self._bv_key = key
        # (a fused MultiAgentEnv step replaces bus_voltages with its own mapping)
        self.bus_voltages = self._bv
        self._extrema = None

    def voltage_extrema(self):
        """(min, max) over all output nodes per env, once per solve (multiagent_env.py:107-113)."""
        if self._extrema is None:
            if self._all_nodes and self.bus_voltages is self._bv:
                v = self.v_out[:len(self.output_names)]
            else:     # a subset of rows, or a fused step's mapping (every node, on demand)
                v = torch.stack(list(self.bus_voltages.values()))
            self._extrema = (v.min(0).values, v.max(0).values)
        return self._extrema

    def get_bus_voltages(self) -> dict:
        return self.bus_voltages

    def get_bus_voltage_by_name(self, bus_name: str) -> Union[torch.Tensor, List[torch.Tensor]]:
        nodes = bus_name_to_nodes(bus_name)
        if len(nodes) == 1:
            return self.bus_voltages[nodes[0]]
        return [self.bus_voltages[x] for x in nodes]
