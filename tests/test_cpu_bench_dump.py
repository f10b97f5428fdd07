"""bench.py --dump-outputs: the snapshot of a step's returned dicts and its
files (host tensors stand in for the device's; no GPU)."""
import os

import numpy as np
import torch

import bench


def _step_out(n):
    g = torch.Generator().manual_seed(3)
    obs = {"a0": {"building": torch.rand(n, 3, generator=g, dtype=torch.float64),
                  "pv": torch.rand(2, n, generator=g, dtype=torch.float64).t()},
           "a1": {"building": torch.rand(n, 3, generator=g, dtype=torch.float64)}}
    rew = {"a0": torch.rand(n, generator=g, dtype=torch.float32), "a1": torch.rand(n, generator=g)}
    meta = {"a0": {}, "a1": {}, "voltage_violation": torch.rand(n, generator=g, dtype=torch.float64),
            "oob_actions": torch.tensor([7], dtype=torch.int64)}
    dones = {"a0": False, "a1": False, "__all__": False}
    return obs, rew, dones, meta


def test_snapshot_is_a_copy_of_every_returned_tensor():
    out = _step_out(11)
    kept = bench.snapshot_outputs(out)
    assert sorted(kept) == ["meta.oob_actions", "meta.voltage_violation", "obs.a0.building", "obs.a0.pv",
                            "obs.a1.building", "reward.a0", "reward.a1"]
    want = out[0]["a0"]["pv"].clone()
    out[0]["a0"]["pv"].zero_()                     # the next step overwrites the buffer
    assert torch.equal(kept["obs.a0.pv"], want)


def test_dump_whole_and_sampled(tmp_path, monkeypatch):
    n = 1000
    out = _step_out(n)
    kept = bench.snapshot_outputs(out)
    whole = str(tmp_path / "whole")
    bench.dump_outputs(whole, kept, n)
    assert sorted(os.listdir(whole)) == sorted(k + ".npy" for k in kept)
    for k, t in kept.items():
        a = np.load(os.path.join(whole, k + ".npy"))
        assert a.dtype == np.float64 and a.shape == tuple(t.shape)
        np.testing.assert_array_equal(a, t.double().numpy())
    # above the limit: the same seeded env sample from every array with an env
    # axis, the same files from run to run, within the limit in all
    limit = 40000
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", limit)
    dirs = [str(tmp_path / "s0"), str(tmp_path / "s1")]
    for d in dirs:
        bench.dump_outputs(d, kept, n)
    idx = np.load(os.path.join(dirs[0], "sample_env_index.npy"))
    assert idx.dtype == np.float64 and 0 < len(idx) < n and np.all(np.diff(idx) > 0)
    ii = idx.astype(np.int64)
    total = 0
    for f in sorted(os.listdir(dirs[0])):
        a = np.load(os.path.join(dirs[0], f))
        np.testing.assert_array_equal(a, np.load(os.path.join(dirs[1], f)))
        total += a.nbytes
        if f in ("sample_env_index.npy", "meta.oob_actions.npy"):
            continue
        full = kept[f[:-4]].double().numpy()
        np.testing.assert_array_equal(a, np.take(full, ii, axis=full.shape.index(n)))
    assert total <= limit
