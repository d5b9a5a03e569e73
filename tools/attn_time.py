#!/usr/bin/env python3
"""Timing of the attention actor's bf16 kernel.

One JSON line: swarm_attn_policy_forward (bf16, logits + deterministic actions) over 524,288
observation rows (N = 64 x E = 8,192, K = 3, Ms = 4), against, on the same rows in the same process,
  * `PolicyMLP` bf16 (swarm_policy_forward: the trunk alone, a 48-wide first layer), and
  * the torch `AttentionActor` forward in eager mode, f32 and bf16 (the module cast to bf16, timed
    with the f32 -> bf16 cast of the observations it needs).
Also a K sweep of the attention kernel (K = 1, 3, 8, 16): the front end's share grows with K.
Method (tools/critic_time.py): a warm-up of every side, then the sides alternated for --pairs pairs;
every sample is a device-event window over enough calls to last ~0.1 s.  Each side reports its
median and its spread (min, max).  Needs a GPU: there is no fallback.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from critic_time import alternate  # noqa: E402


def make_policy(dev, k: int, ms: int, out: int = 6):
    from swarm_marl_amd import AttentionActor, AttentionPolicy
    torch.manual_seed(100 * k + ms)
    actor = AttentionActor(k, ms, out)
    with torch.no_grad():
        for name, p in actor.named_parameters():
            if name.endswith("bias"):
                p.uniform_(-0.1, 0.1)  # torch zero-initialises the attention biases
    params, layers = actor.split_state()
    return AttentionPolicy(params, layers, neighbor_k=k, sensed_obstacles=ms, device=dev, precision="bf16"), actor


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal of the tool, not a measurement)")
    args = ap.parse_args()
    if args.pairs < 3:
        ap.error("--pairs must be >= 3")
    if not torch.cuda.is_available():
        print("attn_time.py needs a GPU", file=sys.stderr)
        return 2
    from swarm_marl_amd.policy import PolicyMLP
    dev = torch.device("cuda", 0)
    rows = 64 * (64 if args.quick else 8192)
    k, ms = 3, 4
    pol, actor = make_policy(dev, k, ms)
    d = pol.in_dim
    gen = torch.Generator(device=dev).manual_seed(rows)
    obs = (torch.rand((rows, d), device=dev, generator=gen) * 6 - 3).contiguous()
    logits = torch.empty((rows, 6), dtype=torch.float32, device=dev)
    actions = torch.empty((rows, 3), dtype=torch.float32, device=dev)
    rng = np.random.default_rng(0)
    mlp = PolicyMLP.from_arrays(*[rng.uniform(-1, 1, s).astype(np.float32) / np.float32(np.sqrt(s[-1]))
                                  for s in ((256, d), (256,), (256, 256), (256,), (6, 256), (6,))], device=dev)
    a32 = actor.to(dev).eval()
    a16 = make_policy(dev, k, ms)[1].to(dev).to(torch.bfloat16).eval()

    from torch.nn.attention import SDPBackend, sdpa_kernel

    def eager(m, dt):
        # bf16: the math backend — torch's fused attention kernels put the batch on a grid axis and
        # reject 524,288 one-query batches ("invalid argument"); f32 takes torch's own choice
        with torch.no_grad():
            if dt == torch.bfloat16:
                with sdpa_kernel(SDPBackend.MATH):
                    return m(obs.to(dt))
            return m(obs.to(dt))

    sides = {"attn_bf16": lambda: pol.forward(obs, logits=logits, actions=actions),
             "policy_mlp_bf16": lambda: mlp.forward(obs, logits=logits, actions=actions),
             "torch_eager_f32": lambda: eager(a32, torch.float32),
             "torch_eager_bf16": lambda: eager(a16, torch.bfloat16)}
    res = alternate(sides, args.pairs)
    ours = res["attn_bf16"]["median_ms"]
    pol.forward(obs, logits=logits)
    diff = float((logits - eager(a32, torch.float32)).abs().max())
    print(json.dumps(dict(case="attn_forward", rows=rows, neighbor_k=k, sensed_obstacles=ms, pairs=args.pairs, **res,
                          ns_per_row=ours * 1e6 / rows,
                          ratio_vs_policy_mlp=ours / res["policy_mlp_bf16"]["median_ms"],
                          speedup_vs_torch_f32=res["torch_eager_f32"]["median_ms"] / ours,
                          speedup_vs_torch_bf16=res["torch_eager_bf16"]["median_ms"] / ours,
                          max_abs_diff_vs_torch_f32=diff)), flush=True)
    sweep = {}
    for kk in (1, 3, 8, 16):
        p2, _ = make_policy(dev, kk, ms)
        o2 = (torch.rand((rows, p2.in_dim), device=dev, generator=gen) * 6 - 3).contiguous()
        sweep[f"K={kk}"] = (lambda p=p2, o=o2: p.forward(o, logits=logits, actions=actions))
    res = alternate(sweep, args.pairs)
    print(json.dumps(dict(case="attn_k_sweep", rows=rows, sensed_obstacles=ms, pairs=args.pairs, **res)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
