"""pgw_coord_reset and MultiAgentEnv's one-launch reset: what can be checked
without a GPU -- the entry in the built library and the header, the ABI
version, the binding's struct, and the predicate that decides whether the
agents' resets are the ones the kernel restates (on stand-ins: it reads
classes and plain attributes only)."""
import ctypes
import os
import re
import types

from powergridworld_amd import _lib
from powergridworld_amd.agents.buildings import FiveZoneROMEnv, FiveZoneROMThermalEnergyEnv
from powergridworld_amd.agents.energy_storage import EnergyStorageEnv
from powergridworld_amd.agents.pv import PVEnv
from powergridworld_amd.base import MultiComponentEnv
from powergridworld_amd.multiagent_env import fused_reset_why

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_resolves_and_abi_is_33():
    lib = _lib.lib()
    assert "pgw_coord_reset" in _lib.EXPORTED
    fn = lib.pgw_coord_reset
    assert fn.restype is ctypes.c_int32
    P = ctypes.POINTER
    assert list(fn.argtypes) == [P(_lib.CoordParams), P(_lib.BuildingExo), ctypes.c_double, ctypes.c_int64,
                                 _lib.CoordBuffers, P(_lib.CoordResetArgs), ctypes.c_void_p]
    assert _lib.ABI_VERSION == 33 and int(lib.pgw_abi_version()) == 33


def test_header_declares_the_entry_and_its_struct():
    with open(os.path.join(REPO, "include", "pgw.h")) as f:
        text = f.read()
    assert re.search(r"#define\s+PGW_ABI_VERSION\s+33\b", text)
    m = re.search(r"int32_t\s+pgw_coord_reset\(([^;]*)\);", text)
    assert m
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["const pgw_coord_params* p", "const pgw_building_exo* ex0", "double pv_pmax0", "int64_t n",
                    "pgw_coord_buffers b", "const pgw_coord_reset_args* r", "void* stream"]
    s = re.search(r"typedef struct pgw_coord_reset_args \{(.*?)\} pgw_coord_reset_args;", text, re.S)
    assert s
    fields = re.findall(r"(\w+)(?:\[PGW_MAX_AGENTS\])?\s*[;,]", s.group(1))
    assert fields == [nm for nm, _ in _lib.CoordResetArgs._fields_]


def test_reset_args_layout():
    """The struct is not in _lib.STRUCTS / pgw_struct_sizes (the ABI version
    stays); libpgw static_asserts the size the binding has."""
    st = _lib.CoordResetArgs
    assert st not in _lib.STRUCTS
    assert ctypes.sizeof(st) == 24 + 3 * 8 * _lib.MAX_AGENTS
    off = {nm: getattr(st, nm).offset for nm, _ in st._fields_}
    assert off == {"init": 0, "init_stride_agent": 8, "sampled_init": 16, "pad_": 20, "p_consumed": 24,
                   "reward_state": 24 + 8 * _lib.MAX_AGENTS, "storage_power": 24 + 16 * _lib.MAX_AGENTS}


# ------------------------------------------------------------------ the predicate
def _exo(T_oa=30.0):
    ex = _lib.BuildingExo()
    ex.T_oa, ex.comfort_lb, ex.comfort_ub = T_oa, 22.0, 28.0
    return ex


def _stand_in(cls, **attrs):
    """An instance of a component class without its constructor (no device)."""
    o = cls.__new__(cls)
    o.__dict__.update(attrs)
    return o


def _agent(name, bld=FiveZoneROMThermalEnergyEnv, pv=PVEnv, bat=EnergyStorageEnv, agent=MultiComponentEnv,
           mean=30.0, std=5.0, T_oa=30.0):
    a = _stand_in(agent, name=name)
    a.envs = [_stand_in(bld, _exo=[_exo(T_oa), _exo(99.0)]), _stand_in(pv),
              _stand_in(bat, initial_storage_mean=mean, initial_storage_std=std)]
    return a


def test_plain_agents_are_eligible():
    assert fused_reset_why([_agent("a")]) is None
    assert fused_reset_why([_agent("a"), _agent("b"), _agent("c")]) is None
    # the base building class's reset is the one restated too
    assert fused_reset_why([_agent("a", bld=FiveZoneROMEnv)]) is None


def test_an_overridden_hook_falls_back():
    class Bat(EnergyStorageEnv):
        def _sample_initial_storage(self):
            return None

    class BatObs(EnergyStorageEnv):
        def get_obs(self, **kw):
            return None

    class Bld(FiveZoneROMThermalEnergyEnv):
        def reset(self, **kw):
            return None

    class Pv(PVEnv):
        def get_obs(self, **kw):
            return None

    class PvReset(PVEnv):
        def reset(self, **kw):
            return None

    class Agent(MultiComponentEnv):
        def reset(self, **kw):
            return None

    class Plain(EnergyStorageEnv):       # a subclass that overrides nothing of it stays eligible
        extra = 1

    for kw in (dict(bat=Bat), dict(bat=BatObs), dict(bld=Bld), dict(pv=Pv), dict(pv=PvReset), dict(agent=Agent)):
        assert fused_reset_why([_agent("a"), _agent("b", **kw)]) is not None, kw
        assert fused_reset_why([_agent("a", **kw)]) is not None, kw
    assert fused_reset_why([_agent("a"), _agent("b", bat=Plain)]) is None


def test_components_must_be_building_pv_storage():
    a = _agent("a")
    a.envs = a.envs[:2]
    assert fused_reset_why([a]) is not None
    b = _agent("b")
    b.envs = [b.envs[0], b.envs[2], b.envs[1]]
    assert fused_reset_why([b]) is not None


def test_storages_share_one_distribution():
    assert fused_reset_why([_agent("a"), _agent("b", mean=31.0)]) is not None
    assert fused_reset_why([_agent("a"), _agent("b", std=4.0)]) is not None
    assert fused_reset_why([_agent("a", mean=12.5, std=0.0), _agent("b", mean=12.5, std=0.0)]) is None
    # 30 == 30.0, but the drawn values' arithmetic is stated for one operand type
    assert fused_reset_why([_agent("a", mean=30), _agent("b", mean=30.0)]) is not None
    # anything but a plain number (a tensor, an array) is left to the component's own code
    assert fused_reset_why([_agent("a", std=types.SimpleNamespace())]) is not None


def test_first_exogenous_rows_are_compared_bytewise():
    assert fused_reset_why([_agent("a"), _agent("b", T_oa=30.5)]) is not None
    assert fused_reset_why([_agent("a", T_oa=0.0), _agent("b", T_oa=-0.0)]) is not None
    assert fused_reset_why([_agent("a", T_oa=-0.0), _agent("b", T_oa=-0.0)]) is None
