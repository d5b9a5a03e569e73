#!/usr/bin/env python3
"""Timing of the per-agent critic and of RolloutCollector.collect() with it.

One JSON line per case:
  * value: three kernels on the same D = 37 x 524,288 observation rows (64 x 8,192 agents) in one
    process: (a) AgentValueMLP bf16 (swarm_value_forward), (b) CriticMLP(in_dim=37, "bf16").value,
    the streaming centralized-critic kernel run at this width, (c) PolicyMLP bf16 logits only (the
    actor kernel: the same two hidden layers plus 16 layer-3 MFMAs per tile and a 6-wide output);
    and the f32 path of (a) for the record (parity only);
  * collect: collect() at N = 64 x E = 8,192 x T = 32 with the bf16 actor, once with the per-agent
    bf16 value tower and once with the centralized bf16 critic, and the tails alone (value launch,
    log-prob, GAE).
Method: a warm-up of every shape, then the sides alternated for --pairs pairs; every sample is a
device-event window over enough calls to last ~0.1 s.  Each side reports its median and its
spread (min, max).  Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "multi-agent-rl-for-autonomous-drone-swarms_amd", ROOT, ROOT / "tools"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import torch  # noqa: E402

from critic_time import alternate, mlp_layers  # noqa: E402


def _np(layers):
    return [(w.numpy(), b.numpy()) for w, b in layers]


def value_case(dev, d: int, rows: int, pairs: int) -> dict:
    from swarm_marl_amd import AgentValueMLP, CriticMLP
    from swarm_marl_amd.policy import PolicyMLP
    layers = _np(mlp_layers(d, 7))
    tower = AgentValueMLP(layers, device=dev, precision="bf16")
    tower32 = AgentValueMLP(layers, device=dev, precision="f32")
    stream = CriticMLP(layers, device=dev, precision="bf16")
    actor = PolicyMLP.from_arrays(*[a for wb in _np(mlp_layers(d, 1, out=6)) for a in wb], device=dev, precision="bf16")
    gen = torch.Generator(device=dev).manual_seed(rows)
    obs = (torch.rand((rows, d), device=dev, generator=gen) * 20 - 10).contiguous()
    out = torch.empty(rows, dtype=torch.float32, device=dev)
    out_b = torch.empty(rows, dtype=torch.float32, device=dev)
    logits = torch.empty((rows, 6), dtype=torch.float32, device=dev)
    sides = {"value_bf16": lambda: tower.value(obs, out=out), "critic_bf16_streaming": lambda: stream.value(obs, out=out_b),
             "policy_bf16_logits": lambda: actor.forward(obs, logits=logits)}
    res = alternate(sides, pairs)
    res.update(alternate({"value_f32": lambda: tower32.value(obs, out=out_b)}, pairs))
    a, b, c = (res[k] for k in ("value_bf16", "critic_bf16_streaming", "policy_bf16_logits"))
    flops = 2.0 * rows * ((d + 1) * 256 + 256 * 256 + 256)
    return dict(case="value", in_dim=d, rows=rows, pairs=pairs, **res,
                value_bf16_tflops=flops / (a["median_ms"] * 1e9),
                speedup_vs_streaming_critic=b["median_ms"] / a["median_ms"],
                beats_streaming_critic_beyond_spread=a["max_ms"] < b["min_ms"],
                ratio_to_policy_logits=a["median_ms"] / c["median_ms"],
                # the two bf16 kernels round the same operands: they differ by f32 summation order
                max_abs_diff_vs_streaming_critic=float((tower.value(obs) - stream.value(obs)).abs().max()))


def collect_case(dev, n: int, e: int, t: int, pairs: int) -> dict:
    from swarm_marl_amd import AgentValueMLP, CriticMLP, RolloutCollector, VecSwarm, gae, gae_agent, gaussian_logp
    from swarm_marl_amd.policy import PolicyMLP

    def make(per_agent: bool):
        vec = VecSwarm(e, {"num_drones": n}, device=dev, auto_reset=True, seed=1, with_global_state=not per_agent)
        vec.reset()
        pol = PolicyMLP.from_arrays(*[a for wb in _np(mlp_layers(vec.obs_dim, 1, out=6)) for a in wb], device=dev,
                                    precision="bf16")
        critic = (AgentValueMLP(_np(mlp_layers(vec.obs_dim, 7)), device=dev, precision="bf16") if per_agent else
                  CriticMLP(_np(mlp_layers(6 * n + 3, n)), device=dev, precision="bf16"))
        return RolloutCollector(vec, pol, critic, horizon=t)

    agent, central = make(True), make(False)

    def tail_agent():  # the part after the step loop: value launch over the block, log-prob, GAE
        agent.critic.value(agent.obs_block, out=agent.value)
        gaussian_logp(agent.logits, agent.actions, out=agent.logp)
        gae_agent(agent.reward, agent.value, agent.terminated, agent.truncated, agent.env_done, agent.valid,
                  gamma=agent.gamma, lam=agent.lam, advantage=agent.advantage, value_target=agent.value_target)

    def tail_central():
        central.critic.value(central.global_state, out=central.value)
        gaussian_logp(central.logits, central.actions, out=central.logp)
        gae(central.reward, central.value, central.terminated, central.truncated, central.env_done, central.valid,
            gamma=central.gamma, lam=central.lam, advantage=central.advantage, value_target=central.value_target)

    res = alternate({"collect_per_agent": agent.collect, "collect_centralized": central.collect,
                     "tail_per_agent": tail_agent, "tail_centralized": tail_central}, pairs)
    return dict(case="collect", num_drones=n, envs=e, horizon=t, pairs=pairs, value_rows=(t + 1) * e * n, **res,
                per_agent_minus_centralized_ms=res["collect_per_agent"]["median_ms"] - res["collect_centralized"]["median_ms"])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--skip-collect", action="store_true")
    args = ap.parse_args()
    if args.pairs < 3:
        ap.error("--pairs must be >= 3")
    if not torch.cuda.is_available():
        print("value_time.py needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    print(json.dumps(value_case(dev, 37, 1024 if args.quick else 64 * 8192, args.pairs)), flush=True)
    if not args.skip_collect:
        e, t = (64, 4) if args.quick else (8192, 32)
        print(json.dumps(collect_case(dev, 64, e, t, args.pairs)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
