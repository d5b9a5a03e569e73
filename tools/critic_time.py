#!/usr/bin/env python3
"""Timing of the centralized critic and of RolloutCollector.collect().

One JSON line per case:
  * critic, bf16 and f32, at N = 64 (G = 387) and N = 256 (G = 1539), rows 8,192 and 32 x 8,192,
    against torch's own chain on the same f32 tensor in the same process: F.linear + relu in bf16
    for the bf16 path (timed with the f32 -> bf16 cast the tensor needs, and again on an input cast
    beforehand), in f32 for the f32 path;
  * collect() at N = 64 x E = 8,192 x T = 32 with the bf16 actor and the bf16 critic.
Method: a warm-up of every shape, then ours / torch alternated for --pairs pairs; every sample is a
device-event window over enough calls to last ~0.1 s.  Each side reports its median and its
spread (min, max).  Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "multi-agent-rl-for-autonomous-drone-swarms_amd", ROOT):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def window(fn, iters: int) -> float:
    """ms per call over one device-event window of `iters` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def calibrate(fn, target_ms: float = 100.0) -> int:
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    one = max(window(fn, 3), 1e-3)
    return int(min(max(target_ms / one, 3), 2000))


def alternate(sides: dict, pairs: int) -> dict:
    iters = {k: calibrate(fn) for k, fn in sides.items()}
    samples = {k: [] for k in sides}
    for _ in range(pairs):
        for k, fn in sides.items():
            samples[k].append(window(fn, iters[k]))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), calls_per_window=iters[k])
            for k, v in samples.items()}


def mlp_layers(in_dim: int, seed: int, out: int = 1):
    torch.manual_seed(seed)
    lins = [torch.nn.Linear(in_dim, 256), torch.nn.Linear(256, 256), torch.nn.Linear(256, out)]
    return [(lin.weight.detach(), lin.bias.detach()) for lin in lins]


def critic_case(dev, n: int, rows: int, precision: str, pairs: int) -> dict:
    from swarm_marl_amd import CriticMLP
    g = 6 * n + 3
    layers = mlp_layers(g, n)
    critic = CriticMLP([(w.numpy(), b.numpy()) for w, b in layers], device=dev, precision=precision)
    gen = torch.Generator(device=dev).manual_seed(rows)
    gs = (torch.rand((rows, g), device=dev, generator=gen) * 20 - 10).contiguous()
    out = torch.empty(rows, dtype=torch.float32, device=dev)
    dt = torch.bfloat16 if precision == "bf16" else torch.float32
    wd = [(w.to(dev, dt), b.to(dev, dt)) for w, b in layers]

    def chain(x):
        x = F.relu(F.linear(x, *wd[0]))
        x = F.relu(F.linear(x, *wd[1]))
        return F.linear(x, *wd[2])

    sides = {"ours": lambda: critic.value(gs, out=out), "torch": lambda: chain(gs.to(dt))}
    if precision == "bf16":
        pre = gs.to(dt)
        sides["torch_precast"] = lambda: chain(pre)
    res = alternate(sides, pairs)
    ref = chain(gs.to(dt)).float()[:, 0]
    flops = 2.0 * rows * ((g + 1) * 256 + 256 * 256 + 256)
    return dict(case="critic", precision=precision, num_drones=n, in_dim=g, rows=rows, pairs=pairs, **res,
                ours_tflops=flops / (res["ours"]["median_ms"] * 1e9),
                speedup_vs_torch=res["torch"]["median_ms"] / res["ours"]["median_ms"],
                max_abs_diff_vs_torch=float((critic.value(gs) - ref).abs().max()))


def collect_case(dev, n: int, e: int, t: int, pairs: int) -> dict:
    from swarm_marl_amd import CriticMLP, RolloutCollector, VecSwarm
    from swarm_marl_amd.policy import PolicyMLP
    vec = VecSwarm(e, {"num_drones": n}, device=dev, auto_reset=True, seed=1, with_global_state=True)
    vec.reset()
    pol = PolicyMLP.from_arrays(*[a.numpy() for wb in mlp_layers(vec.obs_dim, 1, out=6) for a in wb], device=dev,
                                precision="bf16")
    critic = CriticMLP([(w.numpy(), b.numpy()) for w, b in mlp_layers(6 * n + 3, n)], device=dev, precision="bf16")
    col = RolloutCollector(vec, pol, critic, horizon=t)

    def tail():  # the part after the step loop: critic, log-prob, GAE
        from swarm_marl_amd import gae, gaussian_logp
        critic.value(col.global_state, out=col.value)
        gaussian_logp(col.logits, col.actions, out=col.logp)
        gae(col.reward, col.value, col.terminated, col.truncated, col.env_done, col.valid, gamma=col.gamma,
            lam=col.lam, advantage=col.advantage, value_target=col.value_target)

    def bare():  # policy + step only, nothing recorded
        for i in range(t):
            pol.forward(vec.obs, actions=col.actions[0], sample=True, seed=0, counter=i)
            vec.step(col.actions[0])

    res = alternate({"collect": col.collect, "tail_only": tail, "policy_and_step_only": bare}, pairs)
    ms = res["collect"]["median_ms"]
    return dict(case="collect", num_drones=n, envs=e, horizon=t, pairs=pairs, **res,
                agent_steps_per_s=e * n * t / (ms * 1e-3), ms_per_step=ms / t)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--skip-collect", action="store_true")
    args = ap.parse_args()
    if args.pairs < 3:
        ap.error("--pairs must be >= 3")
    if not torch.cuda.is_available():
        print("critic_time.py needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    rows = (256, 1024) if args.quick else (8192, 32 * 8192)
    for precision in ("bf16", "f32"):
        for n in (64, 256):
            for r in rows:
                print(json.dumps(critic_case(dev, n, r, precision, args.pairs)), flush=True)
    if not args.skip_collect:
        e, t = (64, 4) if args.quick else (8192, 32)
        print(json.dumps(collect_case(dev, 64, e, t, args.pairs)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
