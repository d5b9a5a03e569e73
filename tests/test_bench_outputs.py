"""bench.py --full / --dump-outputs: the plain line, the dumped outputs and their repeatability."""
import json

import numpy as np
import pytest
import torch


def test_parse_full_and_dump_default_off():
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.full is False and a.dump_outputs is None and a.steps == 20 and a.warmup == 5
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import bench
    e = 40
    obs = torch.arange(e * 3 * 5, dtype=torch.float32).reshape(e, 3, 5)
    term = (torch.arange(e * 3).reshape(e, 3) % 2).bool()
    done = torch.arange(e, dtype=torch.uint8)
    named = [("obs", obs), ("terminated", term), ("env_done", done), ("global_state", None)]
    bench.dump_outputs(tmp_path / "all", named, e, 0, 1)
    assert sorted(p.name for p in (tmp_path / "all").iterdir()) == \
        ["env_done.npy", "env_index.npy", "obs.npy", "terminated.npy"]
    assert np.array_equal(np.load(tmp_path / "all" / "env_index.npy"), np.arange(e))
    got = np.load(tmp_path / "all" / "obs.npy")
    assert got.dtype == np.float32 and np.array_equal(got, obs.numpy())
    got = np.load(tmp_path / "all" / "terminated.npy")
    assert got.dtype == np.float32 and np.array_equal(got, term.numpy().astype(np.float32))
    # over the budget: the same seeded, sorted sample of the envs for every tensor, twice the same
    per_env = (15 + 3 + 1) * 4 + 8
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10 * per_env)
    bench.dump_outputs(tmp_path / "s1", named, e, 0, 1)
    bench.dump_outputs(tmp_path / "s2", named, e, 1, 2)
    idx = np.load(tmp_path / "s1" / "env_index.npy")
    assert idx.dtype == np.float64 and len(idx) == 10 and np.all(np.diff(idx) > 0) and idx[-1] < e
    assert np.array_equal(idx, np.load(tmp_path / "s2" / "env_index.rank1.npy"))
    sel = idx.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "s1" / "obs.npy"), obs.numpy()[sel])
    assert np.array_equal(np.load(tmp_path / "s1" / "env_done.npy"), done.numpy()[sel].astype(np.float32))
    total = sum(p.stat().st_size for p in (tmp_path / "s1").iterdir())
    assert total <= 10 * per_env + 4 * 128  # the arrays + four .npy headers


@pytest.mark.gpu
def test_bench_plain_line_and_dump_repeat(tmp_path, capsys):
    """A plain run prints the headline fields without the --full legs; --dump-outputs writes the
    last timed step's outputs, equal from run to run and equal to W + K steps of a fresh batch
    with the bench's seeds (the clock-counted device warm-up leaves no trace in them)."""
    import bench
    from swarm_marl_amd import VecSwarm
    e, n, w, k_steps = 96, 64, 3, 6
    recs = []
    for name in ("a", "b"):
        bench.main(["--gpus", "1", "--envs", str(e), "--steps", str(k_steps), "--warmup", str(w),
                    "--device-warmup-ms", "3", "--rehearse", "1", "--dump-outputs", str(tmp_path / name)])
        recs.append(json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1]))
    rec = recs[0]
    assert rec["steps"] == k_steps and rec["warmup"] == w and rec["full"] is False
    assert rec["unit"] == "agent-steps/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(e * n * k_steps / (rec["ms_per_step"] * 1e-3 * k_steps))
    for key in ("cpu_baseline", "cpu_baseline_variants", "ms_per_step_eager"):
        assert key not in rec
    assert "kernel_ms_per_launch" not in rec["roofline"] and rec["roofline"]["kernel_ms_mean"] > 0
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["env_done.npy", "env_index.npy", "obs.npy", "reward.npy", "terminated.npy", "truncated.npy"]
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    for f in files:
        assert got[f[:-4]].dtype in (np.float32, np.float64)
        assert np.array_equal(got[f[:-4]], np.load(tmp_path / "b" / f)), f
    dev = torch.device("cuda", 0)
    vec = VecSwarm(e, {"num_drones": n}, device=dev, auto_reset=True, seed=0)
    vec.reset()
    gen = torch.Generator(device=dev).manual_seed(1000)
    ring = [torch.rand((e, n, 3), device=dev, generator=gen) * 2 - 1 for _ in range(8)]
    for k in [*range(w), *range(k_steps)]:
        vec.step(ring[k % 8])
    torch.cuda.synchronize()
    assert np.array_equal(got["env_index"], np.arange(e))
    for name in ("obs", "reward", "terminated", "truncated", "env_done"):
        assert np.array_equal(got[name], getattr(vec, name).float().cpu().numpy()), name
