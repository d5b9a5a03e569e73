#!/usr/bin/env python3
"""Timing of the on-device actor training path against the torch learner.

One JSON line per measurement, all on one GPU in one process, device events, a warm-up, the sides
alternated for --pairs rounds (>= 5), median [min, max]:

  actor    forward + backward (+ push) of the actor on one minibatch of 262,144 rows (4,096 env-rows x
           64) and of 12,288 rows, D = 37, A = 3.  Sides: `hip` (ActorTrainer: the inference kernel,
           swarm_policy_backward, the device packer), `torch_f32` (the default backend's float32 torch
           MLP, autograd), `torch_bf16` (the same under torch.autocast(bfloat16)).  Achieved FLOP/s from
           the network's 3 x forward FLOPs per row; the hip side's bytes/s from the bytes its launches
           move per row (obs three times, grad_logits, logits, the workspace tensors written and read
           once); `bound_by` names the larger of the two floors at 2.5 PFLOP/s and 8 TB/s.
  update   one `PPOLearner.update()` of a collected 32 x 8,192 x 64 fragment, backend torch and hip.
  loop     --iters iterations of `learner.update(col.collect())`, backend torch and hip, alternated
           iteration by iteration.

--quick runs small shapes (a rehearsal of the tool, not a measurement).  Needs a GPU.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "multi-agent-rl-for-autonomous-drone-swarms_amd", ROOT, ROOT / "tools"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from critic_time import alternate  # noqa: E402

D, A, H = 37, 3, 256
PEAK_FLOPS, HBM_BYTES_PER_S = 2.5e15, 8e12


def actor_arrays(seed: int):
    rng = np.random.default_rng(seed)
    shapes = ((H, D), (H,), (H, H), (H,), (2 * A, H), (2 * A,))
    return [rng.uniform(-1, 1, s).astype(np.float32) / np.float32(np.sqrt(s[-1])) for s in shapes]


def actor_case(dev, rows: int, pairs: int) -> dict:
    from swarm_marl_amd import ActorTrainer
    from swarm_marl_amd.policy import PolicyMLP
    from swarm_marl_amd.ppo import _mlp
    w = actor_arrays(1)
    pol = PolicyMLP.from_arrays(*w, device=dev, precision="bf16")
    trainer = ActorTrainer(pol)
    net = _mlp(pol.layers, dev)
    gen = torch.Generator(device=dev).manual_seed(rows)
    obs = (torch.rand((rows, D), device=dev, generator=gen) * 6 - 3).contiguous()
    g = (torch.randn((rows, 2 * A), device=dev, generator=gen) / rows).contiguous()

    def hip():
        trainer.logits(obs)
        trainer.backward(obs, g)
        trainer.push()

    def torch_f32():
        net.zero_grad(set_to_none=True)
        (net(obs) * g).sum().backward()

    def torch_bf16():
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = net(obs)
        (out.float() * g).sum().backward()

    res = alternate({"hip": hip, "torch_f32": torch_f32, "torch_bf16": torch_bf16}, pairs)
    flops = 3 * 2.0 * rows * ((D + 1) * H + H * H + H * 2 * A)
    nbytes = rows * (3 * 4 * D + 2 * 4 * 2 * A + 2 * 2 * (64 + 32 + 5 * H))
    t = res["hip"]["median_ms"] * 1e-3
    floors = dict(flops=flops / PEAK_FLOPS, bytes=nbytes / HBM_BYTES_PER_S)
    return dict(case="actor", rows=rows, pairs=pairs, **res, flops=flops, bytes=nbytes,
                hip_tflops=flops / t / 1e12, hip_tbytes_per_s=nbytes / t / 1e12,
                torch_f32_tflops=flops / (res["torch_f32"]["median_ms"] * 1e9),
                torch_bf16_tflops=flops / (res["torch_bf16"]["median_ms"] * 1e9),
                floor_ms={k: v * 1e3 for k, v in floors.items()}, bound_by=max(floors, key=floors.get),
                speedup_vs_torch_f32=res["torch_f32"]["median_ms"] / res["hip"]["median_ms"],
                speedup_vs_torch_bf16=res["torch_bf16"]["median_ms"] / res["hip"]["median_ms"])


def make_loop(dev, backend: str, e: int, n: int, t: int, mb: int, epochs: int):
    from swarm_marl_amd import CriticMLP, PPOLearner, RolloutCollector, VecSwarm
    from swarm_marl_amd.policy import PolicyMLP
    from critic_time import mlp_layers
    vec = VecSwarm(e, dict(num_drones=n), device=dev, auto_reset=True, seed=11, with_global_state=True)
    vec.reset()
    pol = PolicyMLP.from_arrays(*actor_arrays(1), device=dev, precision="bf16")
    critic = CriticMLP([(w.numpy(), b.numpy()) for w, b in mlp_layers(6 * n + 3, n)], device=dev, precision="bf16")
    col = RolloutCollector(vec, pol, critic, horizon=t, seed=3)
    learner = PPOLearner(pol, critic, minibatch_env_rows=mb, num_epochs=epochs, backend=backend)
    return col, learner


def timed(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v) -> dict:
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), samples=len(v))


def update_and_loop(dev, e: int, n: int, t: int, mb: int, epochs: int, pairs: int, iters: int, parts) -> None:
    loops = {b: make_loop(dev, b, e, n, t, mb, epochs) for b in ("torch", "hip")}
    shape = dict(envs=e, num_drones=n, horizon=t, agent_rows=e * n * t, minibatch_env_rows=mb, num_epochs=epochs)
    if "update" in parts:
        batches = {b: {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in col.collect().items()}
                   for b, (col, _) in loops.items()}
        for b, (_, learner) in loops.items():
            learner.update(batches[b])  # warm-up: buffers, the workspace, hipBLASLt's choices
        samples = {b: [] for b in loops}
        for _ in range(pairs):
            for b, (_, learner) in loops.items():
                samples[b].append(timed(lambda: learner.update(batches[b])))
        res = {b: stats(v) for b, v in samples.items()}
        print(json.dumps(dict(case="update", **shape, pairs=pairs, **res,
                              speedup_hip=res["torch"]["median_ms"] / res["hip"]["median_ms"])), flush=True)
        del batches
    if "loop" in parts:
        for col, learner in loops.values():
            learner.update(col.collect())  # warm-up
        samples = {b: [] for b in loops}
        kl = {b: [] for b in loops}
        for _ in range(iters):
            for b, (col, learner) in loops.items():
                info = {}
                samples[b].append(timed(lambda: info.update(learner.update(col.collect()))))
                kl[b].append(info["kl"])
        res = {b: dict(stats(v), total_ms=sum(v)) for b, v in samples.items()}
        print(json.dumps(dict(case="loop", **shape, iters=iters, **res, last_epoch_kl=kl,
                              speedup_hip=res["torch"]["total_ms"] / res["hip"]["total_ms"])), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--parts", default="actor,update,loop")
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal of the tool, not a measurement)")
    args = ap.parse_args()
    if args.pairs < 5 and not args.quick:
        ap.error("--pairs must be >= 5")
    if not torch.cuda.is_available():
        print("train_time.py needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    parts = set(args.parts.split(","))
    if "actor" in parts:
        for rows in ((4096, 1024) if args.quick else (262_144, 12_288)):
            print(json.dumps(actor_case(dev, rows, args.pairs)), flush=True)
    if parts & {"update", "loop"}:
        e, n, t, mb = (64, 8, 8, 128) if args.quick else (8192, 64, 32, 4096)
        update_and_loop(dev, e, n, t, mb, args.epochs, args.pairs, args.iters, parts)
    return 0


if __name__ == "__main__":
    sys.exit(main())
