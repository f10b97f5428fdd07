"""The Home-Steward house kernel k_hs (csrc/pgw_hs.hip) called through the C
ABI -- pgw_hs_reset, pgw_hs_step and their _f32 twins -- and compared BIT FOR
BIT with the restated reference of tests/_hs_direct_common.py in the library's
vehicle order: every env at every launch, each launch from the reference's own
pre-launch state uploaded fresh, fp64 and fp32 storage, at the wave and block
edges of a one-thread-per-env kernel (kBlock = 256), in three pgw_mat layouts
for `action` and `obs`, with every output buffer inside a sentinel-filled
allocation whose guards (32 envs on each side) must stay intact.

    full       every case of CASES at n = 65 and 257: every order of {storage,
               EV, devices} after the PV, every subset of one to three
               components, rescale flags mixed per slot, grid-aware PV on and
               off, n_veh 0 / 1 / 2 / 33 / 64 with bits 31, 32 and 63 set,
               n_dev 1 / 2 / 3 / 4, meta_out / step_meta / pv_power_last NULL
               and not, the oob counter bound and NULL
    reduced    the REDUCED cases at n = 1, 63, 64, 255, 256, 513
    exhaustion the named case in which some envs meet the reference's
               ZeroDivisionError: their divided cost is NaN (0 / 0), every
               other env of the same launch stays bit-exact
    args       every refusal of hs_check / hs_reset / hs_step: PGW_ERR_ARG and
               nothing launched; n = 0: PGW_OK and nothing written

Besides the values: step_meta fields a kind does not write keep the sentinel,
ev_req rows >= n_veh are untouched, a reset writes neither reward, real_power,
meta_out, es_power_last, pv_power_last nor step_meta, the inputs are unchanged.

Each test prints `hs-direct <entry> <cases> <envs x launches compared>`.
Needs an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _hs_direct_common as H
from tests.test_gpu_comp_direct import DEV, LAYOUTS, PAD, G, counter, f64_dev, matrix, vec

pytestmark = pytest.mark.gpu
STORAGES = ["f64", "f32"]
FULL_SIZES = (65, 257)
REDUCED_SIZES = tuple(n for n in H.SIZES if n not in FULL_SIZES)
MASK_SENT = 0x5A5A5A5A5A5A5A5A                  # no mask of a case: bits 1, 3, 4, 6 of every byte


def _lib():
    from powergridworld_amd import _lib
    return _lib


def _fn(name, storage):
    return getattr(_lib().lib(), name + ("_f32" if storage == "f32" else ""))


def _stream():
    return _lib().stream_ptr(torch.device(DEV))


def _record(entry, cases, compared):
    print("hs-direct %s %d %d" % (entry, cases, compared))
    assert compared > 0


class Masks:
    """ev_charging: n uint64 words inside a sentinel-filled allocation."""

    def __init__(self, n, values=None):
        self.n = n
        host = np.full(n + 2 * PAD, MASK_SENT, dtype=np.uint64)
        if values is not None:
            host[PAD:PAD + n] = values
        self.t = torch.from_numpy(host.view(np.int64)).to(DEV)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + PAD * 8)

    def check(self, ref, what):
        host = self.t.cpu().numpy().view(np.uint64)
        want = np.full(self.n + 2 * PAD, MASK_SENT, dtype=np.uint64)
        if ref is not None:
            want[PAD:PAD + self.n] = ref
        np.testing.assert_array_equal(host, want, err_msg=str(what))


def block(rows, n, storage, values=None, keep=None, total=None):
    """A rows x n buffer (row-major, its true n) with guards; `keep`: the rows
    of the window (the others must stay untouched); `total`: rows allocated."""
    total = rows if total is None else total
    keep = np.arange(rows) if keep is None else np.asarray(keep, dtype=np.int64)
    idx = PAD + keep[:, None] * n + np.arange(n)[None, :]
    return G(idx, total * n + 2 * PAD, storage, values)


def _launch(P, rec, n, storage, layout, nulls, oob):
    """One record's launch from its pre-state; returns the buffers and the rc."""
    L = _lib()
    pre, reset = rec.pre, rec.act is None
    has_ev = H.EV in P.kind
    b = (L.HSBuffersF32 if storage == "f32" else L.HSBuffers)()
    o = H.NS()
    o.obs = matrix(n, P.obs_dim, layout, storage)
    o.act = None if reset else matrix(n, P.n_comp, layout, storage, rec.act)
    o.soc, o.soc_cost = vec(n, storage, pre.soc), vec(n, storage, pre.soc_cost)
    o.ev_cost, o.dev_cost = vec(n, storage, pre.ev_cost), vec(n, storage, pre.dev_cost)
    o.es_last = vec(n, storage, pre.es_last)
    o.pv_last = None if "pv_power_last" in nulls else vec(n, storage, pre.pv_last)
    o.ev_req = block(P.n_veh, n, storage, pre.ev_req[:P.n_veh], total=H.MAX_VEH)
    o.ev_chg = Masks(n, pre.ev_charging)
    o.reward, o.real_power = vec(n, storage), vec(n, storage)
    o.meta = None if "meta_out" in nulls else block(3, n, storage)
    o.step_meta = None
    if "step_meta" not in nulls:
        keep = [c * H.META_FIELDS + f for c in range(P.n_comp) for f in range(H.WRITTEN[P.kind[c]])]
        o.step_meta = block(len(keep), n, storage, keep=keep, total=P.n_comp * H.META_FIELDS)
    o.init = vec(n, storage, pre.init_soc) if reset else None
    vmin = f64_dev(pre.vmin) if P.pv_grid_aware else None
    b.obs = o.obs.mat()
    if o.act is not None:
        b.action = o.act.mat()
    b.soc, b.soc_cost, b.ev_cost, b.dev_cost = o.soc.ptr, o.soc_cost.ptr, o.ev_cost.ptr, o.dev_cost.ptr
    b.es_power_last = o.es_last.ptr
    b.pv_power_last = o.pv_last.ptr if o.pv_last is not None else None
    if has_ev:
        b.ev_req, b.ev_charging = o.ev_req.ptr, o.ev_chg.ptr
    b.reward, b.real_power = o.reward.ptr, o.real_power.ptr
    b.meta_out = o.meta.ptr if o.meta is not None else None
    b.step_meta = o.step_meta.ptr if o.step_meta is not None else None
    b.min_voltage = L.dptr(vmin)
    p, s = H.hs_params(P, oob), H.hs_info(rec.s)
    if reset:
        rc = _fn("pgw_hs_reset", storage)(p, s, n, o.init.ptr, b, _stream())
    else:
        rc = _fn("pgw_hs_step", storage)(p, s, n, b, _stream())
    torch.cuda.synchronize()
    del vmin
    return o, rc


def _check(P, o, rec, tag):
    r, pre, reset = rec.ref, rec.pre, rec.act is None
    o.obs.check(r.obs if P.obs_dim else None, ("obs", tag))
    o.soc.check(r.soc, ("soc", tag))
    o.soc_cost.check(r.soc_cost, ("soc_cost", tag))
    o.ev_cost.check(r.ev_cost, ("ev_cost", tag))
    o.dev_cost.check(r.dev_cost, ("dev_cost", tag))
    o.ev_req.check(r.ev_req[:P.n_veh], ("ev_req", tag))
    o.ev_chg.check(r.ev_charging, ("ev_charging", tag))
    o.es_last.check(r.es_last, ("es_power_last", tag))           # (a reset: the uploaded values)
    if o.pv_last is not None:
        o.pv_last.check(r.pv_last, ("pv_power_last", tag))
    o.reward.check(None if reset else r.reward, ("reward", tag))
    o.real_power.check(None if reset else r.real_power, ("real_power", tag))
    if o.meta is not None:
        o.meta.check(None if reset else r.meta, ("meta_out", tag))
    if o.step_meta is not None:
        o.step_meta.check(None if reset else r.step_meta[r.written], ("step_meta", tag))
    if o.act is not None:
        o.act.check(rec.act, ("action", tag))
    if o.init is not None:
        o.init.check(pre.init_soc, ("init_soc", tag))


def _run_case(c, n, storage, first_layout=0):
    """Every record of a case at n envs; the layout moves with the record, the
    counter is NULL at every third one.  Returns the envs x launches compared."""
    P, c, recs, _ = H.episode(c.id, n, storage)
    cnt, want = counter(), 0
    for t, rec in enumerate(recs):
        layout = LAYOUTS[(t + first_layout) % len(LAYOUTS)]
        bound = t % 3 != 2
        o, rc = _launch(P, rec, n, storage, layout, c.nulls, cnt.data_ptr() if bound else None)
        _lib().check(rc)
        _check(P, o, rec, (c.id, storage, n, layout, t))
        want += rec.ref.oob if bound else 0
    assert int(cnt) == want, (c.id, storage, n, int(cnt), want)
    return n * len(recs), recs


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("c", H.CASES, ids=[c.id for c in H.CASES])
def test_full(c, storage):
    compared = 0
    for k, n in enumerate(FULL_SIZES):
        compared += _run_case(c, n, storage, k)[0]
    _record("full %s %s" % (storage, c.id), len(FULL_SIZES), compared)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("n", REDUCED_SIZES)
def test_reduced(n, storage):
    compared = 0
    for k, c in enumerate(H.REDUCED):
        compared += _run_case(c, n, storage, k)[0]
    _record("reduced %s n=%d" % (storage, n), len(H.REDUCED), compared)


@pytest.mark.parametrize("storage", STORAGES)
def test_exhaustion(storage):
    """Where the reference raises ZeroDivisionError the kernel stores NaN: the
    flagged envs' divided cost (dev_cost, or delta_cost through soc_cost) is
    0 / 0; every other env of the launch is bit-exact (checked by _run_case for
    all of them, a NaN for a NaN)."""
    n = 65
    compared, recs = _run_case(H.EXHAUSTION, n, storage)
    flagged = mixed = 0
    for rec in recs:
        bad = rec.ref.raises
        assert np.isnan(rec.ref.dev_cost[bad].astype(np.float64) + rec.ref.soc_cost[bad].astype(np.float64)).all()
        flagged += int(bad.sum())
        mixed += 0 < int(bad.sum()) < n
    assert flagged > 0 and mixed > 0
    _record("exhaustion %s flagged=%d" % (storage, flagged), 1, compared)


@pytest.mark.parametrize("storage", STORAGES)
def test_argument_checks(storage):
    L = _lib()
    n = 65
    P, c, recs, _ = H.episode(H.CASES[0].id, n, storage)
    Pg = H.synth_house(1, (H.PV, H.EV), (1, 1), grid_aware=1)           # grid-aware, no storage
    nomat = (L.Matf if storage == "f32" else L.Mat)(None, 0, 0)
    reset, step = _fn("pgw_hs_reset", storage), _fn("pgw_hs_step", storage)

    def attempt(entry, edit_p=None, edit_b=None, null_p=False, null_s=False, null_init=False, n_=n, want=-1,
                params=P):
        """One call with sentinel-only buffers: nothing may be written."""
        b = (L.HSBuffersF32 if storage == "f32" else L.HSBuffers)()
        bufs = {k: vec(n, storage) for k in ("soc", "soc_cost", "ev_cost", "dev_cost", "es_power_last", "reward",
                                             "real_power", "pv_power_last")}
        bufs["ev_req"] = block(H.MAX_VEH, n, storage)
        bufs["meta_out"] = block(3, n, storage)
        bufs["step_meta"] = block(4 * H.META_FIELDS, n, storage)
        obs, act, init, chg = matrix(n, P.obs_dim, "major", storage), matrix(n, 4, "major", storage), \
            vec(n, storage), Masks(n)
        vmin = f64_dev(np.ones(n))
        for k, g in bufs.items():
            setattr(b, k, g.ptr)
        b.obs, b.action, b.ev_charging, b.min_voltage = obs.mat(), act.mat(), chg.ptr, L.dptr(vmin)
        p, s = H.hs_params(params), H.hs_info(recs[1].s)
        if edit_p:
            edit_p(p)
        if edit_b:
            edit_b(b)
        pa, sa = (None if null_p else p), (None if null_s else s)
        if entry == "reset":
            rc = reset(pa, sa, n_, None if null_init else init.ptr, b, _stream())
        else:
            rc = step(pa, sa, n_, b, _stream())
        torch.cuda.synchronize()
        assert rc == want, (entry, rc, L.lib().pgw_last_error())
        if want:
            assert L.lib().pgw_last_error().decode().startswith("pgw_hs"), L.lib().pgw_last_error()
        for k, g in list(bufs.items()) + [("obs", obs), ("action", act), ("init", init), ("ev_charging", chg)]:
            g.check(None, (entry, k, "refused" if want else "n = 0"))

    def setp(**kw):
        def f(p):
            for k, v in kw.items():
                if isinstance(v, (list, tuple)):
                    for i, x in enumerate(v):
                        getattr(p, k)[i] = x
                else:
                    setattr(p, k, v)
        return f

    def setb(**kw):
        def f(b):
            for k, v in kw.items():
                setattr(b, k, v)
        return f

    cases = 0
    for entry in ("reset", "step"):
        both = [dict(null_p=True), dict(null_s=True), dict(n_=-1),
                dict(edit_p=setp(n_comp=0)), dict(edit_p=setp(n_comp=5)),
                dict(edit_p=setp(n_veh=-1)), dict(edit_p=setp(n_veh=H.MAX_VEH + 1)),
                dict(edit_p=setp(n_dev=-1)), dict(edit_p=setp(n_dev=H.MAX_DEV + 1)),
                dict(edit_p=setp(kind=[0, 1, 2, 4])), dict(edit_p=setp(kind=[-1, 1, 2, 3])),
                dict(edit_p=setp(kind=[0, 1, 1, 3])),
                dict(edit_b=setb(obs=nomat))]
        both += [dict(edit_b=setb(**{k: None})) for k in ("soc", "soc_cost", "ev_cost", "dev_cost", "es_power_last")]
        both += [dict(edit_b=setb(ev_req=None)), dict(edit_b=setb(ev_charging=None)),
                 dict(edit_b=setb(min_voltage=None), params=Pg),                      # grid-aware: no min_voltage
                 dict(edit_p=setp(pv_grid_aware=1, kind=[1, 2, 3, 0], n_comp=3))]    # grid-aware: no PV in the chain
        if entry == "reset":
            both.append(dict(null_init=True))
        else:
            both += [dict(edit_b=setb(action=nomat)), dict(edit_b=setb(reward=None)),
                     dict(edit_b=setb(real_power=None))]
        for kw in both:
            attempt(entry, **kw)
            cases += 1
        attempt(entry, n_=0, want=0)                                                 # PGW_OK, nothing written
        cases += 1
    _record("args %s" % storage, cases, cases)
