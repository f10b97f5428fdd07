"""The one-launch C4 step (csrc/pgw_pf.hip k_coord_step_od) with the lookup on
a wave of its own: a block is one wave per agent and the lookup wave, the two
kinds run separate code that meets at the block's two barriers, and the lookup
wave alone reads the node records, solves the envs the table leaves and writes
V675.3, the violation and the iteration count.  As tests/test_gpu_step_overlap.py
(its pair of envs and comparisons): every output, the state left behind, the
out-of-bounds action count and the count of solved envs after every step,
bit for bit against the two-kernel step (k_coord_agents_std + k_coord_pf_od),
at the shapes the new block shape adds: several full blocks and a single-env
block with solved and served lanes mixed in one lookup wave, the 576-thread
block with the wave solve, the two-wave block, and the record base changing
between steps (a reset, then an hour boundary of the table).  Needs an MI355X."""
import pytest
import torch

from tests.test_gpu_step_overlap import NAMES, _bad, _oob, _outputs, _pair, _reset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(envs, g, steps, k, n):
    """`steps` steps of both envs on the same seeded actions in [-1.1, 1.1]
    (some out of range): every output and the state equal after each, this
    step's count of solved envs within [0, n] and the next step's count left
    zero; returns the counts step by step and the warnings expected."""
    solved, want = [], 0
    for t in range(steps):
        a = torch.rand((k, n, 8), dtype=torch.float64, device=DEV, generator=g) * 2.2 - 1.1
        want += int(_bad(a[:, :, :6]).any(2).sum() + _bad(a[:, :, 6]).sum() + _bad(a[:, :, 7]).sum())
        outs = []
        for env in envs:
            _, r, _, m = env.step(a)
            outs.append(_outputs(env, r, m))
        F = envs[0]._fused
        par = F["bufs"].od_parity & 1
        cnt = [int(c) for c in F["od_count"][:2]]
        assert 0 <= cnt[par] <= n and cnt[par ^ 1] == 0, "step %d: od_count %s, parity %d" % (t, cnt, par)
        solved.append(cnt[par])
        for nm, x, y in zip(NAMES, outs[0], outs[1]):
            assert torch.equal(x, y), "one launch vs two kernels: step %d, %s" % (t, nm)
    assert (envs[0].pf_solver.iterations > 0).all()
    return solved, want


def test_lookup_wave_mixed_blocks():
    """n = 193, 5 agents, every 2nd record unfit: three full blocks and a
    single-env block, solved and served lanes mixed in one lookup wave."""
    n, steps = 193, 6
    envs = _pair(n, 5, 2)
    solved, want = _run(envs, torch.Generator(DEV).manual_seed(11), steps, 5, n)
    _oob(envs, want)
    assert all(0 < c < n for c in solved), solved


def test_lookup_wave_max_agents_inline_solve():
    """n = 65, PGW_MAX_AGENTS = 8 agents, every 3rd record unfit: the
    576-thread block (nine waves) with the lookup wave's inline solve."""
    n, steps = 65, 6
    envs = _pair(n, 8, 3)
    solved, want = _run(envs, torch.Generator(DEV).manual_seed(12), steps, 8, n)
    _oob(envs, want)
    assert all(0 < c < n for c in solved), solved


def test_lookup_wave_one_agent():
    """n = 65, one agent, the table as built: a two-wave block (the agent's
    wave and the lookup wave)."""
    n, steps = 65, 6
    envs = _pair(n, 1, 0)
    _, want = _run(envs, torch.Generator(DEV).manual_seed(13), steps, 1, n)
    _oob(envs, want)


def test_lookup_wave_reset_then_hour_boundary():
    """n = 130, 5 agents: 3 steps, env.reset(), then 14 steps from midnight at
    12 steps an hour, so the last steps read the next hour's records (another
    record base than the steps before them)."""
    n = 130
    envs = _pair(n, 5, 0)
    g = torch.Generator(DEV).manual_seed(14)
    _, want = _run(envs, g, 3, 5, n)
    _reset(envs, 19)
    F = [env._fused for env in envs]
    assert torch.equal(F[0]["x"], F[1]["x"]) and torch.equal(F[0]["soc"], F[1]["soc"])
    solver = envs[0].pf_solver
    first = solver.step_tables(envs[0].time)._od_ref.resp_v
    _, more = _run(envs, g, 14, 5, n)
    assert envs[0].time.hour == 1 and envs[1].time.hour == 1, (envs[0].time, envs[1].time)
    last = solver.step_tables(envs[0].time)._od_ref.resp_v
    assert first and last and first != last, "the steps stayed within one hour's node records"
    _oob(envs, want + more)
