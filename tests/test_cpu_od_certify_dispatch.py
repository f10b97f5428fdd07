"""od_certify.certify's dispatch: CPU tensors take the torch program (the
results tests/test_cpu_od_response.py pins), GPU tensors the native entry
unless the model opts out, and OpenDSSSolver.od_certify_native reaches the
model the builder certifies with."""
import types

import numpy as np
import pytest
import torch

from tests.test_cpu_od_response import HOURS, _toy_model, cpu_solver  # noqa: F401  (fixture)


def test_cpu_tensors_take_the_torch_path(monkeypatch):
    from powergridworld_amd.distribution_system import od_certify as C

    def never(*a, **k):
        raise AssertionError("native entry called for CPU tensors")

    monkeypatch.setattr(C, "_certify_native", never)
    a, b = -0.3125, 0.3125
    m = _toy_model(0.96 ** 2 + 1e-6 * 0.02 ** 2)
    assert m.native and m.u0.device.type == "cpu"
    it_p, sig_p = m.solve_points([0], [a])
    ok, ret, sig = C.certify(m, [0], [a], [b])
    assert ok.dtype == bool and ret.dtype == np.int64 and sig.dtype == np.uint64
    assert not ok[0]                                       # the excursion at 0.1 kW
    lo, hi, kw = C.certify_pieces(m, [0], [a], [b], [int(it_p[0])], [sig_p[0]])
    assert lo[0] == a and 0.08 - 1e-3 < hi[0] <= 0.08 and kw[0] > (hi[0] - lo[0]) + 0.18
    m2 = _toy_model(0.96 ** 2 - 1e-6)
    ok2, ret2, sig2 = C.certify(m2, [0], [a], [b])
    it2, sg2 = m2.solve_points([0], [0.0])
    assert ok2[0] and ret2[0] == int(it2[0]) == 2 and sig2[0] == sg2[0]


def test_gpu_tensors_take_the_native_entry_unless_opted_out(monkeypatch):
    from powergridworld_amd.distribution_system import od_certify as C
    calls = []
    monkeypatch.setattr(C, "_certify_native", lambda model, h, lo, hi, db, ds: calls.append((db, ds)) or "native")
    on_gpu = types.SimpleNamespace(native=True, u0=types.SimpleNamespace(device=torch.device("cuda:0")))
    assert C.certify(on_gpu, [0], [0.0], [1.0], delta_band=2e-12) == "native" and calls == [(2e-12, 1e-12)]
    on_gpu.native = False
    # the torch program, which this stub cannot serve (nor a machine without a GPU)
    with pytest.raises((AttributeError, RuntimeError)):
        C.certify(on_gpu, [0], [0.0], [1.0])
    assert len(calls) == 1


def test_solver_flag_reaches_the_model(cpu_solver, monkeypatch):
    from powergridworld_amd.distribution_system import od_certify as C
    s, _ = cpu_solver
    assert s.od_certify_native is True
    seen = []
    real = C.certify_pieces

    def spy(model, *a, **k):
        seen.append(model.native)
        return real(model, *a, **k)

    monkeypatch.setattr(C, "certify_pieces", spy)
    s.od_certify_native = False
    s._od_tables(HOURS[0])
    assert seen == [False]
    st = s.od_resp_stats
    assert st["certified"] and st["certified_pieces"] == st["pieces"] > 6000 and st["pieces_left_to_solve"] == 0
