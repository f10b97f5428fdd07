"""pgw_coord_step_rows and the host's held-row bookkeeping: what can be checked
without a GPU -- the entry in the built library and the header, the ABI
version, and the key comparison MultiAgentEnv uses to decide which env-uniform
observation rows its buffer already holds (by bit pattern, never by ==)."""
import ctypes
import math
import os
import re
import struct

from powergridworld_amd import _lib
from powergridworld_amd.multiagent_env import OBS_ROWS_UNIFORM, obs_rows_held, obs_rows_key

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = sum(1 << j for j in OBS_ROWS_UNIFORM)


def test_entry_resolves_and_abi_is_33():
    lib = _lib.lib()
    assert "pgw_coord_step_rows" in _lib.EXPORTED
    fn = lib.pgw_coord_step_rows
    assert fn.restype is ctypes.c_int32
    args = list(fn.argtypes)
    assert args[:-1] == list(lib.pgw_coord_step.argtypes) and args[-1] is ctypes.c_uint32
    assert _lib.ABI_VERSION == 33 and int(lib.pgw_abi_version()) == 33


def test_header_declares_the_entry():
    with open(os.path.join(REPO, "include", "pgw.h")) as f:
        text = f.read()
    assert re.search(r"#define\s+PGW_ABI_VERSION\s+33\b", text)
    m = re.search(r"int32_t\s+pgw_coord_step_rows\(([^;]*)\);", text)
    assert m
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    base = re.search(r"int32_t\s+pgw_coord_step\(([^;]*)\);", text)
    assert args[:-1] == [a.strip() for a in base.group(1).replace("\n", " ").split(",")]
    assert args[-1] == "uint32_t obs_rows_held"


def test_uniform_slots():
    assert OBS_ROWS_UNIFORM == (10, 11, 12, 14, 15)


def test_nothing_held_without_a_key():
    k = obs_rows_key(20.0, 26.0, 30.0, 0.5, 0.0)
    assert obs_rows_held(None, k) == 0
    assert obs_rows_held(k, k) == ALL
    assert obs_rows_held(k, obs_rows_key(20.0, 26.0, 30.0, 0.5, 0.0)) == ALL


def test_one_scalar_changes_one_bit():
    base = [20.0, 26.0, 30.0, 0.5, 0.0]
    k = obs_rows_key(*base)
    for i, j in enumerate(OBS_ROWS_UNIFORM):
        other = list(base)
        other[i] = math.nextafter(base[i], math.inf)      # one ulp is a change
        assert obs_rows_held(k, obs_rows_key(*other)) == ALL & ~(1 << j)


def test_negative_zero_is_not_zero():
    a, b = obs_rows_key(20.0, 26.0, 30.0, 0.5, 0.0), obs_rows_key(20.0, 26.0, 30.0, 0.5, -0.0)
    assert 0.0 == -0.0 and a != b
    assert obs_rows_held(a, b) == ALL & ~(1 << 15)
    assert obs_rows_held(b, b) == ALL


def test_nan_equals_itself_only_bit_for_bit():
    nan = float("nan")
    other_nan = struct.unpack("<d", struct.pack("<q", struct.unpack("<q", struct.pack("<d", nan))[0] ^ 1))[0]
    assert math.isnan(other_nan) and nan != nan
    a = obs_rows_key(20.0, 26.0, nan, 0.5, 0.0)
    assert obs_rows_held(a, obs_rows_key(20.0, 26.0, nan, 0.5, 0.0)) == ALL
    assert obs_rows_held(a, obs_rows_key(20.0, 26.0, other_nan, 0.5, 0.0)) == ALL & ~(1 << 12)


def test_a_change_and_a_change_back():
    """The held key is always the LAST writer's: a one-step change costs two
    stores of the row (the changed value, then the old one again)."""
    seq = [(20.0, 26.0), (20.0, 26.0), (19.0, 26.0), (20.0, 26.0), (20.0, 26.0)]
    held, masks = None, []
    for lb, ub in seq:
        k = obs_rows_key(lb, ub, 30.0, 0.5, 0.0)
        masks.append(obs_rows_held(held, k))
        held = k
    assert masks == [0, ALL, ALL & ~(1 << 10), ALL & ~(1 << 10), ALL]
