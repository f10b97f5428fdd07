"""The one-launch C4 step on fp32 buffers (k_coord_step_od_f32: an env pair per
lane, 128 envs a block) against the fp32 two-kernel step
(k_coord_agents_std_x2 + k_coord_pf_od<.., pgw_coord_buffers_f32>), bit for
bit.  Needs an MI355X.

The pair kernel reads env-minor packed actions (env.action_buffer()'s layout,
the benchmark's); the tests pass [5, N, 8] views of [5, 8, N] tensors.  With
any other layout, or an odd batch, the library stays on the two kernels."""
import pytest
import torch

from tests.test_gpu_pf_od import _unfit

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32


def _envs(n, every, kinds=("one", "two", "no_table")):
    from powergridworld_amd.scenarios.coordinated import CoordinatedMultiBuildingControlEnv, make_c4_config
    envs = []
    for kind in kinds:
        env = CoordinatedMultiBuildingControlEnv(**make_c4_config(), num_envs=n, device=DEV, dtype=F32)
        assert env._fused is not None and env._fused["kernel"] == "pgw_coord_step_f32"
        env.set_pf_list(kind == "one")
        if kind == "no_table":
            env.pf_solver.od_table = False
        envs.append(env)
    gen = torch.Generator(DEV).manual_seed(17)
    init = (torch.rand((5, n), dtype=torch.float64, device=DEV, generator=gen) * 40.0 + 5.0).float().double()
    for env in envs:
        env.reset()
        for ai, agent in enumerate(env.agents):
            agent.env_dict["storage"].reset(init_storage=init[ai])
        env.load_component_state()
        if every and env.pf_solver.od_table:
            _unfit(env.pf_solver, every)
    return envs


def _action(n, gen, env_minor=True):
    """rand * 2.2 - 1.1 cast to fp32, as the packed [5, N, 8] tensor."""
    if env_minor:
        return (torch.rand((5, 8, n), dtype=torch.float64, device=DEV, generator=gen) * 2.2 - 1.1).float().transpose(1, 2)
    return (torch.rand((5, n, 8), dtype=torch.float64, device=DEV, generator=gen) * 2.2 - 1.1).float()


def _outputs(env, r, m):
    """Every per-env output: obs, x, soc, agent_power, reward, v_out, vv, iters."""
    F = env._fused
    return [env.packed_obs().clone(), F["x"].clone(), F["soc"].clone(), F["agent_power"].clone(),
            torch.stack([r[a.name] for a in env.agents]).clone(), F["v_out"].clone(),
            m["voltage_violation"].clone(), F["iters"].clone()]


@pytest.mark.parametrize("n,every,env_minor", [(4134, 0, True), (4134, 3, True), (4134, 1, True), (126, 1, True),
                                               (2, 1, True), (4133, 3, True), (4134, 3, False)])
def test_f32_one_launch_equals_two_kernels(n, every, env_minor):
    """set_pf_list(True) against set_pf_list(False) on fp32 buffers, every
    output torch.equal over 12-20 steps: 4134 = 32 * 128 + 38 (a partial last
    block with 19 live lanes), 126 (one partial block), 2 (one live lane); with
    the table serving (every = 0), a third of its records unfit, and all of
    them (then also equal to the step without a table, and od_count = every
    env of every step).  od_count counts the envs left to the wave solve, so on
    the two-kernel fallback -- an odd batch (4133), or env-major actions (the
    last case, added here) -- nothing is counted: there the outputs are still
    identical, od_on stays set and od_count is 0 at every step."""
    steps = {0: 20, 3: 16, 1: 12}[every]
    envs = _envs(n, every)
    assert envs[0]._fused["od_on"] is True and envs[0]._one_launch_ok()
    assert not envs[1]._fused.get("od_on")
    fallback = n % 2 == 1 or not env_minor
    gen = torch.Generator(DEV).manual_seed(3)
    F = envs[0]._fused
    listed = 0
    for t in range(steps):
        a = _action(n, gen, env_minor)
        outs = []
        for env in envs:
            o, r, d, m = env.step(a)
            outs.append(_outputs(env, r, m))
        listed += int(F["od_count"][F["bufs"].od_parity & 1])
        assert int(F["od_count"][(F["bufs"].od_parity & 1) ^ 1]) == 0       # the next step's slot
        for i, (x, y) in enumerate(zip(outs[0], outs[1])):
            assert x.dtype == y.dtype and torch.equal(x, y), "one launch vs two kernels: step %d output %d" % (t, i)
        if every == 1:
            for i, (x, y) in enumerate(zip(outs[0], outs[2])):
                assert torch.equal(x, y), "all unfit vs no table: step %d output %d" % (t, i)
    if fallback:
        assert listed == 0, listed
    elif every == 1:
        assert listed == n * steps, listed
    elif every == 3:
        assert 0 < listed < n * steps, listed
    assert (envs[0].pf_solver.iterations > 0).all()


def test_f32_capture_step_equals_eager():
    """capture_step(actions, steps=4) on the fp32 env, two calls = 8 steps,
    against eager steps, bit for bit, at n = 4134 with a third of the records
    unfit: both list parities occur inside a graph."""
    n = 4134
    ea, eg = _envs(n, 3, kinds=("one", "one"))
    assert ea._fused["od_on"] is True and eg._fused["od_on"] is True
    gen = torch.Generator(DEV).manual_seed(5)
    acts = [_action(n, gen) for _ in range(8)]
    bufs = [torch.empty((5, 8, n), dtype=F32, device=DEV).transpose(1, 2) for _ in range(4)]
    g = eg.capture_step(bufs, steps=4)
    listed_a = listed_g = 0
    for call in range(2):
        for i in range(4):
            bufs[i].copy_(acts[4 * call + i])
            o, r, d, m = ea.step(acts[4 * call + i])
        want = _outputs(ea, r, m)
        o, r, d, m = g()
        got = _outputs(eg, r, m)
        for i, (x, y) in enumerate(zip(want, got)):
            assert torch.equal(x, y), "graph vs eager: call %d output %d" % (call, i)
        for e in (ea, eg):
            assert e._fused["bufs"].od_parity == ea._fused["bufs"].od_parity
        listed_a += int(ea._fused["od_count"][ea._fused["bufs"].od_parity & 1])
        listed_g += int(eg._fused["od_count"][eg._fused["bufs"].od_parity & 1])
    assert listed_a == listed_g and 0 < listed_a < 2 * n
    assert ea.episode_step == eg.episode_step == 8
