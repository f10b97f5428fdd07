"""The fp32 twins of the fused steps' argument structs mirror their fp64
structs field by field (pure ctypes: no library load, no GPU)."""
import ctypes as C

from powergridworld_amd import _lib


def _offsets(st):
    return {nm: getattr(st, nm).offset for nm, _ in st._fields_}


def test_ma_step_args_f32_layout():
    a, b = _lib.MAStepArgs, _lib.MAStepArgsF32
    assert C.sizeof(b) == C.sizeof(a)
    assert [nm for nm, _ in b._fields_] == [nm for nm, _ in a._fields_]
    assert _offsets(b) == _offsets(a)
    # the component records too (kind, action, obs, real_power)
    assert C.sizeof(_lib.MCComponentF32) == C.sizeof(_lib.MCComponent)
    assert _offsets(_lib.MCComponentF32) == _offsets(_lib.MCComponent)
    assert b in _lib.STRUCTS and _lib.STRUCTS.index(b) == len(_lib.STRUCTS) - 1
    assert "pgw_ma_step_f32" in _lib.EXPORTED


def test_coord_buffers_f32_has_the_list_scratch():
    """od_list / od_count / od_parity follow iters in pgw_coord_buffers_f32 as
    they do in pgw_coord_buffers (the one-launch step's scratch)."""
    a, b = _offsets(_lib.CoordBuffers), _offsets(_lib.CoordBuffersF32)
    for nm in ("od_list", "od_count", "od_parity", "pad_"):
        assert b[nm] - b["iters"] == a[nm] - a["iters"], nm
    assert [nm for nm, _ in _lib.CoordBuffersF32._fields_] == [nm for nm, _ in _lib.CoordBuffers._fields_]
    assert C.sizeof(_lib.CoordBuffersF32) == C.sizeof(_lib.CoordBuffers)
    assert _lib.ABI_VERSION == 33
