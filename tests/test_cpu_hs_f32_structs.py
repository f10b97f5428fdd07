"""pgw_hs_buffers_f32 mirrors pgw_hs_buffers field by field, and the fp32 house's
two entries are bound (pure ctypes: no library load, no GPU).  The struct is
deliberately not in _lib.STRUCTS / pgw_struct_sizes (the ABI version stays):
libpgw static_asserts its layout against pgw_hs_buffers, whose size the
binding checks at load."""
import ctypes as C

from powergridworld_amd import _lib


def _offsets(st):
    return {nm: getattr(st, nm).offset for nm, _ in st._fields_}


def test_hs_buffers_f32_layout():
    a, b = _lib.HSBuffers, _lib.HSBuffersF32
    assert [nm for nm, _ in b._fields_] == [nm for nm, _ in a._fields_]
    assert _offsets(b) == _offsets(a)
    assert C.sizeof(b) == C.sizeof(a)
    types = dict(b._fields_)
    assert types["action"] is _lib.Matf and types["obs"] is _lib.Matf
    assert [nm for nm, tp in a._fields_ if tp is _lib.Mat] == ["action", "obs"]
    # every other field is the same pointer type as the fp64 struct's
    assert all(tp is dict(a._fields_)[nm] for nm, tp in b._fields_ if nm not in ("action", "obs"))


def test_hs_f32_entries_bound_and_abi_unchanged():
    for sym in ("pgw_hs_reset_f32", "pgw_hs_step_f32"):
        assert sym in _lib.EXPORTED
    res, args = _lib._SIGS["pgw_hs_reset_f32"]
    assert res is _lib.i32 and args[4] is _lib.HSBuffersF32 and len(args) == len(_lib._SIGS["pgw_hs_reset"][1])
    res, args = _lib._SIGS["pgw_hs_step_f32"]
    assert res is _lib.i32 and args[3] is _lib.HSBuffersF32 and len(args) == len(_lib._SIGS["pgw_hs_step"][1])
    assert _lib.ABI_VERSION == 33
    assert _lib.STRUCTS[-1] is _lib.MAStepArgsF32 and _lib.HSBuffersF32 not in _lib.STRUCTS
