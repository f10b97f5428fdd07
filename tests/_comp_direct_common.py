"""Shared by tests/test_cpu_comp_ref.py and tests/test_gpu_comp_direct.py: plain
host-side descriptions of a battery, a PV plant, a five-zone building and an
exogenous row, the functions that fill the ABI structs from them, NumPy float64
restatements of the component kernels (include/pgw.h: "Energy storage", "PV
curtailment", "Five-zone reduced-order building", "MultiComponentEnv
reduction"; the device functions of csrc/pgw_common.h) and the case lists both
test files run.  Nothing here needs a GPU.

What is compared, and why bit equality is the contract.  The kernels are
elementwise: one thread per env, no sum whose order depends on the launch, no
transcendental.  libpgw is built with -ffp-contract=off, every division is the
IEEE quotient (the standard building path divides by host reciprocals through
exact_div, which returns the IEEE quotient), and the only fused operations
are the ones of cube_rn, which forms the correctly rounded s^3.  Every output
therefore has ONE correct bit pattern, the one np.float64 arithmetic produces
when it does the same operations in the same order:

    clip(x, lo, hi)  = (y > hi ? hi : y), y = (x < lo ? lo : x)       (np.clip)
    pymax(a, b)      = b > a ? b : a       pymin(a, b) = b < a ? b : a
    to_raw(y, lo, hi)    = (clip(y, -1, 1) * (hi - lo) + (hi + lo)) / 2
    to_scaled(x, lo, hi) = (2 clip(x, lo, hi) - (lo + hi)) / (hi - lo)
    bu = ((B0 u0 + B1 u1) + B2 u2) + B3 u3,   x' = A x + bu
    s  = (((a0 + a1) + a2) + a3) + a4
    pc = (0.0076 RN(s^3) + 4.8865) + pymax(0, s (T_oa - a5))
    reward = alpha (-pc / 12) 0.5 + (1 - alpha) c,   c = -(sum of m_z^2 from 0.0)

RN(s^3) is formed exactly here (float(Fraction(s) ** 3)); NumPy's `**` is
glibc's pow, which is not correctly rounded.  The halving in to_raw and the
`* 0.5` of the standard path are exact either way.  fp32 storage (the _f32
entries): the state and the actions are float32 values widened exactly, the
arithmetic is the float64 one above, and every stored output is
np.float32(ref64), rounded once.

One thing IEEE 754 leaves open: the sign and payload of a NaN that an
operation produces (x86 and gfx950 differ).  `same_bits` therefore asks for
equal bits everywhere except where the reference is NaN, and there for a NaN.
The sign of a zero is compared.

No operation of these kernels needed a bound: the tolerance is zero.

Case lists: fixed recipes over seeded np.random.default_rng; the coverage
conditions they are built to meet are asserted by tests/test_cpu_comp_ref.py
on the references alone.
"""
import functools
import json
import os
import types
from fractions import Fraction

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(REPO, "powergridworld_amd", "data")
OOB_EPS = 1e-4                                     # PGW_OOB_EPS (pgw.h)
PINNED = (1.0, -1.0, 1.0 + 1e-4, -(1.0 + 1e-4))
BEYOND = (float(np.nextafter(1.0 + 1e-4, 2.0)), float(np.nextafter(-(1.0 + 1e-4), -2.0)))
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)        # one thread per env, kBlock = 256
BLD_SIZES = (1, 65, 257, 513)
WAVE_SIZES = (1, 63, 65, 129)                      # the fused agent wave: 64 envs per block
MAX_COMP = 8                                       # PGW_MAX_COMP
ND = {"f64": np.float64, "f32": np.float32}
UINT = {"f64": np.uint64, "f32": np.uint32}
NS = types.SimpleNamespace

# PGW_BV_* (pgw.h): the reference's state-dict order
BV_ZONE_TEMP, BV_UPPER_VIOL, BV_LOWER_VIOL = 0, 5, 10
BV_COMFORT_LOWER, BV_COMFORT_UPPER, BV_OUTDOOR_TEMP, BV_P_CONSUMED, BV_TIME_OF_DAY = 15, 16, 17, 18, 19
BV_BUS_VOLTAGE, BV_MIN_VOLTAGE, BV_MAX_VOLTAGE, BV_P_SETPOINT = 20, 21, 22, 23
# five_zone_rom_env.py:230-262 (values) and obs_space.py:9-48 (bounds): (key, zones)
STATE_KEYS = (("zone_temp", 5), ("zone_upper_viol", 5), ("zone_lower_viol", 5), ("comfort_lower", 1),
              ("comfort_upper", 1), ("outdoor_temp", 1), ("p_consumed", 1), ("time_of_day", 1),
              ("bus_voltage", 1), ("min_voltage", 1), ("max_voltage", 1), ("p_setpoint", 1))
SPACE_KEYS = ("zone_temp", "zone_upper_viol", "zone_lower_viol", "comfort_lower", "comfort_upper",
              "outdoor_temp", "p_setpoint", "p_consumed", "time_of_day", "bus_voltage", "min_voltage",
              "max_voltage")
DEFAULT_OBS = {"zone_upper_viol": (-10., 10.), "zone_lower_viol": (-10., 10.), "comfort_lower": (20., 25.),
               "comfort_upper": (25., 30.), "outdoor_temp": (0., 56.), "p_consumed": (0., 100.),
               "time_of_day": (0., 1.)}                                        # defaults.py:2-10
ALL_OBS = {"zone_temp": (16., 40.), "zone_upper_viol": (-10., 10.), "zone_lower_viol": (-10., 10.),
           "comfort_lower": (20., 23.), "comfort_upper": (23., 29.), "outdoor_temp": (0., 56.),
           "p_setpoint": (0., 200.), "p_consumed": (0., 200.), "time_of_day": (0., 1.),
           "bus_voltage": (0.9, 1.1), "min_voltage": (0.9, 1.1), "max_voltage": (0.9, 1.1)}
# every slot its own bounds, tight enough that each clips both ways
TIGHT_OBS = {"zone_temp": (21., 29.), "zone_upper_viol": (-4., 3.), "zone_lower_viol": (-3., 5.),
             "comfort_lower": (20.5, 22.5), "comfort_upper": (24., 27.), "outdoor_temp": (12., 31.),
             "p_setpoint": (10., 150.), "p_consumed": (20., 60.), "time_of_day": (0.125, 0.75),
             "bus_voltage": (0.95, 1.05), "min_voltage": (0.94, 1.0), "max_voltage": (1.0, 1.06)}
ACT_LOW = (.22, .22, .22, .22, .32, 10.0)                                      # five_zone_rom_env.py:22-26
ACT_HIGH = (2.2, 2.2, 2.2, 2.2, 3.2, 16.0)
STD_SEL = ((0, 7, 6, 1), (0, 7, 6, 1), (0, 7, 5, 1), (0, 7, 5, 1), (0, 7, 5, 1))
STD_NBR = ((1, 2, 3, 4), (0, 2, 3, 4), (0, 1, 3, 4), (0, 1, 2, 4), (0, 1, 2, 3))


# ---------------------------------------------------------------- comparing
def same_bits(got, ref, what=""):
    """got == ref bit for bit (the sign of a zero included); where ref is NaN,
    got must be a NaN (its sign and payload are not IEEE's to fix)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    u = {8: np.uint64, 4: np.uint32}[ref.dtype.itemsize]
    g, r = np.ascontiguousarray(got).view(u).copy(), np.ascontiguousarray(ref).view(u).copy()
    both = np.isnan(got) & np.isnan(ref)
    g[both] = 0
    r[both] = 0
    np.testing.assert_array_equal(g, r, err_msg=str(what))


def count_bit_equal(got, ref):
    got, ref = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
    return int((got.view(np.uint64) == ref.view(np.uint64)).sum()), got.size


def _quiet(f):
    @functools.wraps(f)
    def g(*a, **k):
        with np.errstate(all="ignore"):
            return f(*a, **k)
    return g


def _widen(x):
    return np.asarray(x).astype(np.float64)


def _store(x, storage):
    """A stored output: the float64 value, or np.float32 of it (rounded once)."""
    return np.asarray(x, dtype=np.float64).astype(ND[storage])


# ---------------------------------------------------------------- numpy semantics (pgw_common.h)
def clip(x, lo, hi):
    y = np.where(x < lo, lo, x)
    return np.where(y > hi, hi, y)


def pymax(a, b):
    return np.where(b > a, b, a)


def pymin(a, b):
    return np.where(b < a, b, a)


def to_scaled(x, lo, hi):
    x = clip(x, lo, hi)
    return (2.0 * x - (lo + hi)) / (hi - lo)


def to_raw(y, lo, hi):
    y = clip(y, -1.0, 1.0)
    return (y * (hi - lo) + (hi + lo)) / 2.0


def oob_bad(y):
    return ~((y >= -1.0 - OOB_EPS) & (y <= 1.0 + OOB_EPS))


@functools.lru_cache(maxsize=1 << 18)
def _cube1(s):
    if s != s or s in (np.inf, -np.inf):
        return s * s * s
    return float(Fraction(s) ** 3)


def cube(s):
    """s^3 correctly rounded (what cube_rn computes), elementwise."""
    s = np.asarray(s, dtype=np.float64)
    return np.array([_cube1(float(v)) for v in s.ravel()], dtype=np.float64).reshape(s.shape)


def fma(a, b, c):
    """One correctly rounded a * b + c of finite Python floats."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def exact_div_ref(x, d, r):
    """pgw_common.h exact_div, restated with the exact fma above."""
    q0 = x * r
    q1 = fma(fma(-d, q0, x), r, q0)
    q2 = fma(fma(-d, q1, x), r, q1)
    return q0 if x == 0.0 else q2


# ---------------------------------------------------------------- descriptions
def Battery(soc_min=3.0, soc_max=50.0, eta_c=0.95, eta_d=0.9, max_power=15.0, dt_h=300 / 3600.0, rescale=1,
            sampled_init=0):
    return NS(soc_min=float(soc_min), soc_max=float(soc_max), eta_c=float(eta_c), eta_d=float(eta_d),
              max_power=float(max_power), dt_h=float(dt_h), rescale=int(rescale), sampled_init=int(sampled_init))


def PV(obs_low, rescale=1, grid_aware=0, obs_high=0.0, vmin_low=0.9, vmin_high=1.1):
    return NS(obs_low=float(obs_low), obs_high=float(obs_high), vmin_low=float(vmin_low),
              vmin_high=float(vmin_high), rescale=int(rescale), grid_aware=int(grid_aware))


def Exo(T_oa, q_solar, q_int, q_cool, lb, ub, tod):
    f = lambda v: np.asarray(v, dtype=np.float64).copy()
    return NS(T_oa=float(T_oa), q_solar=f(q_solar), q_int=f(q_int), q_cool=f(q_cool), lb=float(lb), ub=float(ub),
              tod=float(tod))


def obs_layout(config):
    """(obs_var, obs_low, obs_high) of an obs config: values in state-dict
    order, bounds in make_obs_space order (five_zone_rom_env.py:265-270 zips
    them exactly so)."""
    var, k = [], 0
    for key, nz in STATE_KEYS:
        if key in config:
            var += list(range(k, k + nz))
        k += nz
    lo, hi = [], []
    for key in SPACE_KEYS:
        if key in config:
            nz = dict(STATE_KEYS)[key]
            lo += [float(config[key][0])] * nz
            hi += [float(config[key][1])] * nz
    return var, lo, hi


def Building(A, B, K, C, mean, sel, nbr, obs_var, obs_low, obs_high, rescale=1, T_init=None, alpha=0.2,
             act_low=ACT_LOW, act_high=ACT_HIGH):
    f = lambda v: np.asarray(v, dtype=np.float64).copy()
    assert len(obs_var) == len(obs_low) == len(obs_high)
    return NS(A=f(A), B=f(B), K=f(K), C=f(C), mean=f(mean), sel=np.asarray(sel, dtype=np.int64).copy(),
              nbr=np.asarray(nbr, dtype=np.int64).copy(), obs_var=[int(v) for v in obs_var], obs_low=f(obs_low),
              obs_high=f(obs_high), rescale=int(rescale), T_init=f(np.full(5, 27.0) if T_init is None else T_init),
              alpha=float(alpha), act_low=f(act_low), act_high=f(act_high))


@functools.lru_cache(maxsize=None)
def _zones():
    with open(os.path.join(DATA, "state_space_model.json")) as f:
        return json.load(f)["zones"]


def shipped_x0():
    return np.array([float(np.ravel(z["x_k"])[0]) for z in _zones()])


def shipped_building(config=None, rescale=1, T_init=None, layout=None):
    """The shipped state-space model (ss_B rounded to float32, dynamics.py:51)."""
    z = _zones()
    one = lambda k: [float(np.ravel(m[k])[0]) for m in z]
    B = np.array([np.ravel(m["ss_B"]) for m in z], dtype=np.float64).astype(np.float32).astype(np.float64)
    sel = [[int(v) - 1 for v in np.ravel(m["input_sel_list"])] for m in z]
    nbr = [[int(v) for v in m["neighbors"]] for m in z]
    var, lo, hi = layout if layout is not None else obs_layout(DEFAULT_OBS if config is None else config)
    return Building(one("ss_A"), B, one("ss_K"), one("ss_C"), one("mean_output"), sel, nbr, var, lo, hi, rescale,
                    T_init)


def synthetic_building(seed, config, rescale=1):
    """A model that is not the shipped one: `sel` uses every u_pos index 0..7
    across the zones (q_int, the reset's q_cool and every neighbour slot), the
    neighbour rows are permutations of other zones with repeats."""
    rng = np.random.default_rng(7000 + seed)
    A = rng.uniform(0.90, 0.99, 5)
    B = rng.uniform(-0.02, 0.02, (5, 4)).astype(np.float32).astype(np.float64)
    K = rng.uniform(0.05, 0.6, 5)
    C = rng.uniform(0.8, 1.3, 5)
    mean = rng.uniform(22.0, 26.0, 5)
    sel = [[0, 7, 2, 1], [3, 4, 5, 6], [7, 2, 6, 0], [1, 3, 7, 5], [4, 0, 2, 7]]
    if seed % 2:
        sel = [[2, 3, 7, 4], [0, 1, 7, 5], [6, 7, 1, 2], [5, 0, 4, 3], [7, 6, 3, 1]]
    assert {s for row in sel for s in row} == set(range(8))
    nbr = [[4, 3, 2, 1], [4, 4, 0, 2], [1, 0, 4, 3], [2, 2, 1, 0], [3, 1, 0, 0]]
    if seed % 2:
        nbr = [[2, 4, 1, 3], [3, 0, 4, 2], [3, 3, 0, 1], [1, 4, 0, 2], [2, 0, 3, 3]]
    var, lo, hi = obs_layout(config)
    return Building(A, B, K, C, mean, sel, nbr, var, lo, hi, rescale, rng.uniform(20.0, 30.0, 5))


def bld_is_std_ref(M):
    """pgw_common.h bld_is_std."""
    return (len(M.obs_var) == 15 and np.array_equal(M.sel, STD_SEL) and np.array_equal(M.nbr, STD_NBR)
            and list(M.obs_var) == [5 + j for j in range(15)])


def bld_derived_ref(M):
    """pgw_common.h make_bld_derived (the first 15 slots)."""
    lo, hi = M.obs_low[:15], M.obs_high[:15]
    with np.errstate(all="ignore"):
        return NS(act_rng=M.act_high - M.act_low, act_sum=M.act_high + M.act_low, obs_sum=lo + hi,
                  obs_rng=hi - lo, obs_rcp=1.0 / (hi - lo))


# ---------------------------------------------------------------- ABI structs
def battery_params(B, oob=None):
    from powergridworld_amd import _lib
    return _lib.BatteryParams(soc_min=B.soc_min, soc_max=B.soc_max, eta_c=B.eta_c, eta_d=B.eta_d,
                              max_power=B.max_power, dt_h=B.dt_h, rescale=B.rescale,
                              sampled_init=B.sampled_init, oob=oob)


def pv_params(P, oob=None):
    from powergridworld_amd import _lib
    return _lib.PVParams(obs_low=P.obs_low, obs_high=P.obs_high, vmin_low=P.vmin_low, vmin_high=P.vmin_high,
                         rescale=P.rescale, grid_aware=P.grid_aware, oob=oob)


def building_params(M, oob=None, n_obs=None):
    from powergridworld_amd import _lib
    p = _lib.BuildingParams()
    for z in range(5):
        p.A[z], p.K[z], p.C[z], p.mean[z], p.T_init[z] = M.A[z], M.K[z], M.C[z], M.mean[z], M.T_init[z]
        for j in range(4):
            p.B[z][j], p.sel[z][j], p.nbr[z][j] = M.B[z, j], int(M.sel[z, j]), int(M.nbr[z, j])
    for j in range(6):
        p.act_low[j], p.act_high[j] = M.act_low[j], M.act_high[j]
    for j, v in enumerate(M.obs_var):
        p.obs_var[j], p.obs_low[j], p.obs_high[j] = v, M.obs_low[j], M.obs_high[j]
    p.n_obs = len(M.obs_var) if n_obs is None else n_obs
    p.alpha, p.rescale, p.oob = M.alpha, M.rescale, oob
    return p


def building_exo(ex):
    from powergridworld_amd import _lib
    s = _lib.BuildingExo()
    s.T_oa, s.comfort_lb, s.comfort_ub, s.time_of_day = ex.T_oa, ex.lb, ex.ub, ex.tod
    for z in range(5):
        s.q_solar[z], s.q_int[z], s.q_cool[z] = ex.q_solar[z], ex.q_int[z], ex.q_cool[z]
    return s


def exo_of_struct(s):
    return Exo(s.T_oa, list(s.q_solar), list(s.q_int), list(s.q_cool), s.comfort_lb, s.comfort_ub, s.time_of_day)


def building_ext(ptrs):
    """pgw_building_ext from {"bus" | "vmin" | "vmax" | "pset": device pointer}."""
    from powergridworld_amd import _lib
    return _lib.BuildingExt(bus_voltage=ptrs.get("bus"), min_voltage=ptrs.get("vmin"),
                            max_voltage=ptrs.get("vmax"), p_setpoint=ptrs.get("pset"))


# ---------------------------------------------------------------- battery (energy_storage_env.py:72-157)
def battery_obs(B, s):
    return to_scaled(s, B.soc_min, B.soc_max) if B.rescale else s


@_quiet
def battery_reset_ref(B, init, storage="f64"):
    i = _widen(init)
    s = i if B.sampled_init else clip(i, B.soc_min, B.soc_max)
    return NS(soc=_store(s, storage), obs=_store(battery_obs(B, s), storage)[:, None])


@_quiet
def battery_step_ref(B, soc, action, storage="f64"):
    soc, a = _widen(soc), _widen(action).reshape(-1)
    oob = 0
    if B.rescale:
        oob = int(oob_bad(a).sum())
        a = to_raw(a, -1.0, 1.0)
    p0 = a * B.max_power
    power = p0
    # validate_power :112-126: `if power > 0 ... elif power < 0`, on the unclamped power
    dis = (p0 > 0.0) & (soc - (p0 * B.dt_h) / B.eta_d < B.soc_min)
    power = np.where(dis, pymax(soc - B.soc_min, 0.0) / B.dt_h, power)
    chg = (p0 < 0.0) & (soc - (B.eta_c * p0) * B.dt_h > B.soc_max)
    power = np.where(chg, -(pymax(B.soc_max - soc, 0.0) / B.dt_h), power)
    s_c = pymin(soc - (B.eta_c * power) * B.dt_h, B.soc_max)
    s_d = pymax(soc - (power * B.dt_h) / B.eta_d, B.soc_min)
    new = np.where(power < 0.0, s_c, np.where(power > 0.0, s_d, soc))
    cov = {"dis_clamp": int((dis & (power > 0.0)).sum()), "chg_clamp": int((chg & (power < 0.0)).sum()),
           "dis_at_bound": int((dis & (power == 0.0)).sum()), "chg_at_bound": int((chg & (power == 0.0)).sum()),
           "zero_power": int((p0 == 0.0).sum()), "free_dis": int(((p0 > 0.0) & ~dis).sum()),
           "free_chg": int(((p0 < 0.0) & ~chg).sum()), "nan": int(np.isnan(p0).sum())}
    return NS(soc=_store(new, storage), obs=_store(battery_obs(B, new), storage)[:, None],
              rp=_store(-power, storage), oob=oob, cov=cov)


# ---------------------------------------------------------------- PV (pv_profile_env.py:102-148)
@_quiet
def pv_ref(P, n, pmax, action=None, vmin=None, storage="f64"):
    """obs (and, with an action, real power) of pgw_pv_obs / pgw_pv_step."""
    raw = np.full(n, -float(pmax))
    cols = [to_scaled(raw, P.obs_low, P.obs_high) if P.rescale else raw]
    if P.grid_aware:
        v = np.asarray(vmin, dtype=np.float64)
        cols.append(to_scaled(v, P.vmin_low, P.vmin_high) if P.rescale else v)
    out = NS(obs=_store(np.stack(cols, 1), storage), rp=None, oob=0)
    if action is not None:
        a = _widen(action).reshape(-1)
        if P.rescale:
            out.oob = int(oob_bad(a).sum())
            a = to_raw(a, 0.0, 1.0)
        out.rp = _store(a * (-float(pmax)), storage)
    return out


# ---------------------------------------------------------------- building
def _ext_values(ext, n):
    """five_zone_rom_env.py:256-262: bus 1.0; min / max = the bus value when a
    bus array is given, else 1.0; p_setpoint +inf."""
    ext = ext or {}
    bus = np.asarray(ext["bus"], dtype=np.float64) if ext.get("bus") is not None else np.full(n, 1.0)
    dflt = bus if ext.get("bus") is not None else np.full(n, 1.0)
    vmin = np.asarray(ext["vmin"], dtype=np.float64) if ext.get("vmin") is not None else dflt
    vmax = np.asarray(ext["vmax"], dtype=np.float64) if ext.get("vmax") is not None else dflt
    pset = np.asarray(ext["pset"], dtype=np.float64) if ext.get("pset") is not None else np.full(n, np.inf)
    return bus, vmin, vmax, pset


def _state_update(M, ex, T, act, x):
    """dynamics.py:12-55 for all zones; act None: the reset form (u_pos[7] = q_cool)."""
    n = T.shape[0]
    new = np.empty_like(x)
    for z in range(5):
        upos = [ex.T_oa - T[:, z], np.full(n, ex.q_solar[z]), np.full(n, ex.q_int[z])]
        upos += [T[:, M.nbr[z, i]] - T[:, z] for i in range(4)]
        upos.append(np.full(n, ex.q_cool[z]) if act is None else act[:, z] * (act[:, 5] - T[:, z]))
        u = [upos[M.sel[z, j]] for j in range(4)]
        bu = M.B[z, 0] * u[0]
        bu = bu + M.B[z, 1] * u[1]
        bu = bu + M.B[z, 2] * u[2]
        bu = bu + M.B[z, 3] * u[3]
        new[:, z] = M.A[z] * x[:, z] + bu
    return new


def _p_consumed(a, T_oa):
    s = (((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]) + a[:, 4]
    fan = 0.0076 * cube(s) + 4.8865
    term = s * (T_oa - a[:, 5])
    return fan + pymax(0.0, term), term


def _reward(M, T, lb, ub, pc):
    c = np.zeros(T.shape[0])
    for z in range(5):
        m = pymax(pymax(T[:, z] - ub, lb - T[:, z]), 0.0)
        c = c + m * m
    c = -c
    return M.alpha * (-pc / 12.0) * 0.5 + (1.0 - M.alpha) * c, c


def _obs(M, T, ex, pc, ext, n):
    bus, vmin, vmax, pset = _ext_values(ext, n)
    src = {BV_COMFORT_LOWER: np.full(n, ex.lb), BV_COMFORT_UPPER: np.full(n, ex.ub),
           BV_OUTDOOR_TEMP: np.full(n, ex.T_oa), BV_P_CONSUMED: pc, BV_TIME_OF_DAY: np.full(n, ex.tod),
           BV_BUS_VOLTAGE: bus, BV_MIN_VOLTAGE: vmin, BV_MAX_VOLTAGE: vmax, BV_P_SETPOINT: pset}
    raw = np.empty((n, len(M.obs_var)))
    out = np.empty((n, len(M.obs_var)))
    for j, var in enumerate(M.obs_var):
        v = T[:, var] if var < 5 else T[:, var - 5] - ex.ub if var < 10 else ex.lb - T[:, var - 10] if var < 15 \
            else src[var]
        raw[:, j] = v
        v = clip(v, M.obs_low[j], M.obs_high[j])
        out[:, j] = to_scaled(v, M.obs_low[j], M.obs_high[j]) if M.rescale else v
    return raw, out


def _obs_cov(M, raw):
    """Per class of slot that can clip: env-steps below / above / inside its bounds."""
    cov = {}
    for j, var in enumerate(M.obs_var):
        cls = "temp" if var < 5 else "upper" if var < 10 else "lower" if var < 15 else \
            {BV_P_CONSUMED: "pcons", BV_P_SETPOINT: "pset"}.get(var)
        if cls is None:
            continue
        v = raw[:, j]
        for tag, m in (("below", v < M.obs_low[j]), ("above", v > M.obs_high[j]),
                       ("inside", (v >= M.obs_low[j]) & (v <= M.obs_high[j]))):
            cov[cls + "_" + tag] = cov.get(cls + "_" + tag, 0) + int(m.sum())
    return cov


@_quiet
def building_reset_ref(M, ex0, x, ext=None, storage="f64"):
    """pgw_building_reset: x is the [5, n] zone-major state (persists)."""
    xs = _widen(x).T.copy()
    n = xs.shape[0]
    T = np.tile(M.T_init, (n, 1))
    for _ in range(2):                                   # five_zone_rom_env.py:160-173
        xs = _state_update(M, ex0, T, None, xs)
        yhat = M.C * xs
        yact = T - M.mean
        xs = xs + M.K * (yact - yhat)
    T = M.C * xs + M.mean
    pc = np.zeros(n)
    raw, obs = _obs(M, T, ex0, pc, ext, n)
    rew, c = _reward(M, T, ex0.lb, ex0.ub, pc)
    cov = _obs_cov(M, raw)
    cov["reset_reward_negzero"] = int((np.signbit(rew) & (rew == 0.0)).sum())
    return NS(x=_store(xs.T, storage), pc=_store(pc, storage), rstate=_store(rew, storage),
              obs=_store(obs, storage), cov=cov)


@_quiet
def building_step_ref(M, ex, exn, x, action, rstate=None, lagged=0, ext=None, storage="f64"):
    """pgw_building_step: rout = the previous rstate when lagged, else the fresh reward."""
    xs, v = _widen(x).T.copy(), _widen(action)
    n = xs.shape[0]
    bad = oob_bad(v).any(axis=1)
    a = to_raw(v, M.act_low, M.act_high) if M.rescale else v
    T = M.C * xs + M.mean
    xs = _state_update(M, ex, T, a, xs)
    T = M.C * xs + M.mean
    pc, term = _p_consumed(a, ex.T_oa)
    fresh, c = _reward(M, T, exn.lb, exn.ub, pc)
    raw, obs = _obs(M, T, exn, pc, ext, n)
    fresh_s = _store(fresh, storage)
    cov = _obs_cov(M, raw)
    up, lo = (T - exn.ub > 0.0).any(axis=1), (exn.lb - T > 0.0).any(axis=1)
    cov.update(chiller_zero=int((term <= 0.0).sum()), chiller_pos=int((term > 0.0).sum()),
               comfort_negzero=int((np.signbit(c) & (c == 0.0)).sum()), viol_upper=int(up.sum()),
               viol_lower=int(lo.sum()), one_nan=int((np.isnan(v).sum(axis=1) == 1).sum()))
    for k, pin in enumerate(PINNED):
        cov["pinned%d" % k] = int((v == ND[storage](pin)).sum())
    return NS(x=_store(xs.T, storage), pc=_store(pc, storage), rstate=fresh_s,
              rout=np.asarray(rstate).astype(ND[storage]).copy() if lagged else fresh_s,
              obs=_store(obs, storage), oob=int(bad.sum()) if M.rescale else 0, cov=cov)


# ---------------------------------------------------------------- reduce (base.py:125-156)
@_quiet
def reduce_ref(real_power, reward, n):
    """Left to right from 0.0 in component order; a None entry contributes 0.0."""
    w, r = np.zeros(n), np.zeros(n)
    for rp, rw in zip(real_power, reward):
        r = r + (np.asarray(rw, dtype=np.float64) if rw is not None else 0.0)
        w = w + (np.asarray(rp, dtype=np.float64) if rp is not None else 0.0)
    return w, r


def reduce_columns(n, n_comp, seed):
    """Component columns whose left-to-right sum from 0.0 has bits no other
    order gives: magnitudes from 1e-9 to 1e16 with both signs (so most
    reorderings round differently), env 0 all -0.0 (sum +0.0: it starts from
    +0.0), env 1 a cancellation that only left-to-right resolves to 1.0."""
    rng = np.random.default_rng(9000 + 17 * n_comp + seed)
    cols = rng.standard_normal((n_comp, n)) * 10.0 ** rng.integers(-9, 17, (n_comp, n))
    if n_comp:
        cols[:, 0] = -0.0
    if n_comp >= 3 and n > 1:
        cols[:, 1] = 0.0
        cols[0, 1], cols[1, 1], cols[2, 1] = 1e16, -1e16, 1.0     # (1e16 - 1e16) + 1 = 1; 1e16 + (1 - 1e16) = 0
    return cols


# ---------------------------------------------------------------- cases: battery
BATTERY_SETS = {"default": dict(), "big": dict(soc_min=3.0, soc_max=250.0, max_power=20.0, eta_c=0.9, eta_d=0.85),
                "odd": dict(soc_min=2.5, soc_max=41.3, max_power=11.7, eta_c=0.93, eta_d=0.87, dt_h=7 / 60.0)}
# (the goldens' three sets are default, default at rescale = 0 and big)
BATTERY_CASES = [NS(id="%s-r%d" % (k, r), cfg=dict(v, rescale=r), seed=i * 2 + r, steps=8)
                 for i, (k, v) in enumerate(BATTERY_SETS.items()) for r in (1, 0)]


def battery_inputs(c, n, storage="f64"):
    """(init [n], actions [steps, n]) of a case, as stored values.  Env e follows
    pattern (e + seed) % 12: the clamps, the clamp at the bound, zero power,
    free charge and discharge, inits outside the range, PINNED, BEYOND, NaN."""
    B = Battery(**c.cfg)
    rng = np.random.default_rng(100 + c.seed)
    step_kwh = B.max_power * B.dt_h
    mid = 0.5 * (B.soc_min + B.soc_max)
    init = rng.uniform(B.soc_min - 3.0, B.soc_max + 3.0, n)
    act = rng.uniform(-1.3, 1.3, (c.steps, n))
    special = list(PINNED) + list(BEYOND) + [np.nan, 0.0]
    for e in range(n):
        k = (e + c.seed) % 12
        if k == 0:
            init[e], act[:, e] = B.soc_min + 0.3 * step_kwh, 1.0
        elif k == 1:
            init[e], act[:, e] = B.soc_max - 0.3 * step_kwh, -1.0
        elif k == 2:
            init[e], act[:, e] = mid, 0.0
        elif k == 3:
            init[e], act[:, e] = mid, rng.uniform(-0.3, 0.3, c.steps)
        elif k == 4:
            init[e], act[:, e] = mid, [special[(t + e) % len(special)] for t in range(c.steps)]
        elif k == 5:
            init[e], act[:, e] = B.soc_min - 2.0, 0.5
        elif k == 6:
            init[e], act[:, e] = B.soc_max + 2.0, -0.5
    return init.astype(ND[storage]), act.astype(ND[storage])


@functools.lru_cache(maxsize=None)
def battery_episode(cid, n, storage, sampled_init):
    """[(B, pre-step soc, action, reference)] with the reset first (action None)."""
    c = next(c for c in BATTERY_CASES if c.id == cid)
    B = Battery(sampled_init=sampled_init, **c.cfg)
    init, act = battery_inputs(c, n, storage)
    r = battery_reset_ref(B, init, storage)
    out = [(B, init, None, r)]
    for t in range(c.steps):
        soc = r.soc
        r = battery_step_ref(B, soc, act[t], storage)
        out.append((B, soc, act[t], r))
    return out


# ---------------------------------------------------------------- cases: PV
PV_MAX = 37.25                                                   # max(data) of the synthetic profile
PV_PMAX = (0.0, 1e-300, PV_MAX, 12.3)                            # 0, tiny, max(data), an ordinary row
PV_CASES = [NS(id="r%d-g%d" % (r, g), rescale=r, grid_aware=g, seed=2 * r + g) for r in (1, 0) for g in (0, 1)]


def pv_inputs(c, n, storage="f64"):
    """(actions [len(PV_PMAX), n], vmin [n] float64): PINNED, BEYOND, NaN and
    draws; min_voltage below, inside and above (vmin_low, vmin_high)."""
    rng = np.random.default_rng(300 + c.seed)
    act = rng.uniform(-1.3, 1.3, (len(PV_PMAX), n))
    special = list(PINNED) + list(BEYOND) + [np.nan, 0.0, -0.0]
    for e in range(0, n, 2):
        for t in range(len(PV_PMAX)):
            act[t, e] = special[(e // 2 + t + c.seed) % len(special)]
    vmin = np.array([(0.85, 0.97, 1.15, 0.9, 1.1, 1.0312)[(e + c.seed) % 6] for e in range(n)])
    return act.astype(ND[storage]), vmin


# ---------------------------------------------------------------- cases: building
def exo_rows(seed, steps):
    """steps + 1 synthetic exogenous rows.  T_oa from below every discharge
    temperature (chiller term 0) through exactly 16.0 (the term is an exact 0
    at the highest discharge temperature) to a hot 41; comfort bounds that
    move, so upper and lower violations and rows without any occur."""
    rng = np.random.default_rng(500 + seed)
    T_oa = [8.5, 16.0, 24.75, 41.0, 33.1, 9.0, 28.3, 19.9, 36.6, 13.0, 30.0, 22.2, 27.7]
    lbs = [22.0, 21.0, 26.5, 10.0, 22.0, 23.5, 5.0, 22.0, 24.0, 22.0, 20.0, 12.0, 22.0]
    ubs = [28.0, 27.0, 29.0, 45.0, 24.0, 28.0, 50.0, 23.0, 28.0, 26.0, 25.0, 44.0, 28.0]
    rows = []
    for t in range(steps + 1):
        k = (t + seed) % len(T_oa)
        rows.append(Exo(T_oa[k], rng.uniform(0.0, 3.1, 5), rng.uniform(1.0, 1.5, 5), rng.uniform(-3.0, -2.0, 5),
                        lbs[k], ubs[k], t / float(steps)))
    return rows


def building_inputs(M, seed, n, steps, storage="f64"):
    """(x0 [5, n], actions [steps, n, 6], ext arrays) as stored values.  x0 puts
    the zone temperatures from about 8 to 48 degrees (below, inside and above every
    temperature and violation bound); actions are draws around [-1, 1]
    (rescale) or around the raw ranges, with PINNED values, BEYOND and one NaN
    per row in some envs."""
    rng = np.random.default_rng(600 + seed)
    T0 = rng.uniform(8.0, 48.0, (5, n))
    T0[:, ::3] = rng.uniform(22.5, 27.5, (5, len(range(0, n, 3))))          # a third start comfortable
    x0 = (T0 - M.mean[:, None]) / M.C[:, None]
    if M.rescale:
        act = rng.uniform(-1.25, 1.25, (steps, n, 6))
    else:
        act = rng.uniform(M.act_low - 0.6, M.act_high + 0.6, (steps, n, 6))
    special = list(PINNED) + list(BEYOND)
    for e in range(n):
        k = (e + seed) % 7
        if k == 0:                                   # a PINNED / BEYOND value in every element
            for t in range(steps):
                act[t, e, :] = special[(t + e // 7) % len(special)]
        elif k == 1:                                 # exactly one NaN, the element moving with the step
            for t in range(steps):
                act[t, e, (t + e // 7) % 6] = np.nan
        elif k == 2:                                 # the highest discharge temperature, exactly
            act[:, e, 5] = 1.0 if M.rescale else M.act_high[5]
        elif k == 3 and not M.rescale:               # raw flows far below their range: p_consumed < 0
            act[:, e, :5] = rng.uniform(-2.6, -1.2, (steps, 5))
    ext = {"bus": rng.uniform(0.88, 1.12, n), "vmin": rng.uniform(0.88, 1.12, n),
           "vmax": rng.uniform(0.88, 1.12, n), "pset": rng.uniform(-20.0, 260.0, n)}
    # (with all 24 variables the p_setpoint slot is zipped with the max_voltage bounds)
    ext["pset"][1::3] = rng.uniform(0.96, 1.04, len(range(1, n, 3)))
    return x0.astype(ND[storage]), act.astype(ND[storage]), ext


def _pick_ext(ext, which):
    return {k: v for k, v in ext.items() if k in which}


ONE_OBS = {"p_setpoint": (0., 200.)}                  # p_setpoint alone: the default +inf clipped to 200
BLD_STD_CASES = [NS(id="std-r%d-l%d" % (r, l), kind="std", config=DEFAULT_OBS, rescale=r, lagged=l, seed=10 + 2 * r + l, steps=6,
                    ext=()) for r in (1, 0) for l in (1, 0)]
BLD_GEN_CASES = [
    NS(id="gen-nobs0", kind="shipped", config={}, rescale=1, lagged=1, seed=20, steps=6, ext=()),
    NS(id="gen-nobs1-pset-inf", kind="shipped", config=ONE_OBS, rescale=1, lagged=0, seed=21, steps=6, ext=()),
    NS(id="gen-nobs1-pset", kind="shipped", config=ONE_OBS, rescale=0, lagged=1, seed=25, steps=6, ext=("pset",)),
    NS(id="gen-all24-none", kind="shipped", config=ALL_OBS, rescale=1, lagged=1, seed=22, steps=6,
       ext=()),
    NS(id="gen-all24-bus", kind="shipped", config=ALL_OBS, rescale=0, lagged=0, seed=23, steps=6,
       ext=("bus",)),
    NS(id="gen-tight24-all4", kind="shipped", config=TIGHT_OBS, rescale=1, lagged=1, seed=24, steps=6,
       ext=("bus", "vmin", "vmax", "pset")),
    NS(id="gen-synth0-r1", kind="synth", config=TIGHT_OBS, rescale=1, lagged=0, seed=30, steps=6,
       ext=("bus", "vmin", "vmax", "pset")),
    NS(id="gen-synth1-r0", kind="synth", config=ALL_OBS, rescale=0, lagged=1, seed=31, steps=6,
       ext=("bus", "pset")),
]
BLD_CASES = BLD_STD_CASES + BLD_GEN_CASES


def building_of(c):
    if c.kind in ("std", "shipped"):
        return shipped_building(c.config, c.rescale)
    return synthetic_building(c.seed, c.config, c.rescale)


@functools.lru_cache(maxsize=None)
def building_episode(cid, n, storage):
    """(M, rows, ext, [records]): the first two records are two consecutive
    resets (x_k persists), the rest the steps; a record is
    NS(kind, x, rstate, action, ex, exn, ref) with x / rstate the state before it."""
    c = next(c for c in BLD_CASES if c.id == cid)
    M = building_of(c)
    rows = exo_rows(c.seed, c.steps)
    x0, act, ext_all = building_inputs(M, c.seed, n, c.steps, storage)
    ext = _pick_ext(ext_all, c.ext)
    recs, x = [], x0
    rstate = np.zeros(n, dtype=ND[storage])
    for _ in range(2):
        r = building_reset_ref(M, rows[0], x, ext, storage)
        recs.append(NS(kind="reset", x=x, rstate=rstate, action=None, ex=rows[0], exn=None, ref=r))
        x, rstate = r.x, r.rstate
    for t in range(c.steps):
        r = building_step_ref(M, rows[t], rows[t + 1], x, act[t], rstate, c.lagged, ext, storage)
        recs.append(NS(kind="step", x=x, rstate=rstate, action=act[t], ex=rows[t], exn=rows[t + 1], ref=r))
        x, rstate = r.x, r.rstate
    return M, rows, ext, recs


def merge_cov(total, cov):
    for k, v in cov.items():
        total[k] = total.get(k, 0) + v
    return total
