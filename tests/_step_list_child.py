"""The list form of the fused C4 step -- k_coord_step_od<.., false> lists the
envs the response table does not serve, k_coord_pf_od_list solves them in a
second launch -- which the library selects with PGW_STEP_LIST=1, read once when
it loads.  Run as a program in a fresh process with that variable set
(tests/test_gpu_pf_offgrid.py starts it; not collected by pytest):

    PGW_STEP_LIST=1 python -m tests._step_list_child

At n = 193 (three full 64-env blocks and a single-env block), six steps each:
the step scenario of tests/_offgrid_common.py (most envs off the grid, many
stopped by the cap), and make_c4_config() with every third record unfit.  The
default fused step against the two-kernel step (k_coord_agents_std +
k_coord_pf_od): every output and the state bit for bit; od_count is the number
of envs the table does not serve, the list holds exactly their ids and the
list's unused tail is still zero -- so the list kernels really ran.  Exits
non-zero on any mismatch.  Needs an MI355X."""
import os
import sys

import numpy as np
import torch

DEV = "cuda:0"
N, STEPS = 193, 6


def _compare(envs, actions, want_capped):
    from tests.test_gpu_pf_od import _served
    from tests.test_gpu_pf_offgrid import _bus_load
    from tests.test_gpu_step_overlap import NAMES, _outputs
    lst, two = envs
    F = lst._fused
    assert F.get("od_on") and lst._one_launch_ok() and "od_list" in F, "the default step is not the list step"
    assert not two._fused.get("od_on")
    assert not F["od_list"].any() and not F["od_count"].any()
    top, listed, capped = 0, 0, 0
    for t, a in enumerate(actions):
        outs = []
        for env in envs:
            _, r, _, m = env.step(a)
            outs.append(_outputs(env, r, m))
        torch.cuda.synchronize()
        for nm, x, y in zip(NAMES, outs[0], outs[1]):
            assert torch.equal(x, y), "list form vs two kernels: step %d, %s (%d differ)" % (
                t, nm, int((x != y).sum()))
        par = F["bufs"].od_parity & 1
        cnt = [int(c) for c in F["od_count"][:2]]
        solver = lst.pf_solver
        unserved = np.nonzero(~_served(solver, solver.hour_of(lst.time), _bus_load(outs[0][5])))[0]
        assert cnt[par] == len(unserved) and cnt[par ^ 1] == 0, (t, cnt, par, len(unserved))
        assert 0 < cnt[par] < N, (t, cnt)
        ids = F["od_list"].cpu().numpy()
        assert np.array_equal(np.sort(ids[:cnt[par]]), unserved), "step %d: the list is not the unserved envs" % t
        top = max(top, cnt[par])
        assert not ids[top:].any(), "step %d: list slots past the largest count were written" % t
        listed += cnt[par]
        capped += int((outs[0][4] < 0).sum())
    assert (capped > 0) == want_capped, capped
    return listed


def main():
    if os.environ.get("PGW_STEP_LIST") != "1":
        print("tests._step_list_child: run with PGW_STEP_LIST=1")
        return 2
    from powergridworld_amd.scenarios.coordinated import CoordinatedMultiBuildingControlEnv, make_c4_config
    from tests import _offgrid_common as C
    from tests.test_gpu_pf_od import _unfit
    from tests.test_gpu_pf_offgrid import _step_reset
    from tests.test_gpu_step_overlap import _reset
    # 1. the step scenario: bus loads of -7.4 .. 6.2 MW
    n, agents, max_power = C.STEP_SHAPES[0]
    assert n == N
    envs = [CoordinatedMultiBuildingControlEnv(**C.step_env_config(agents, max_power), num_envs=N, device=DEV,
                                               fused=True) for _ in range(2)]
    envs[1].set_pf_list(False)
    _step_reset(envs)
    acts = [torch.tensor(a, device=DEV) for a in C.step_actions(N, agents, STEPS)]
    listed = _compare(envs, acts, True)
    print("step scenario: %d envs listed over %d steps" % (listed, STEPS))
    del envs
    # 2. make_c4_config(), every third record unfit
    envs = [CoordinatedMultiBuildingControlEnv(**make_c4_config(), num_envs=N, device=DEV, fused=True)
            for _ in range(2)]
    envs[1].set_pf_list(False)
    _reset(envs, 17)
    for env in envs:
        _unfit(env.pf_solver, 3)
    g = torch.Generator(DEV).manual_seed(3)
    acts = [torch.rand((5, N, 8), dtype=torch.float64, device=DEV, generator=g) * 2.2 - 1.1 for _ in range(STEPS)]
    listed = _compare(envs, acts, False)
    print("make_c4_config, every third record unfit: %d envs listed over %d steps" % (listed, STEPS))
    print("list form ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
