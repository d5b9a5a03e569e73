#!/usr/bin/env python3
"""Timing of the fused PPO loss head against the same loss in eager torch.

One JSON line per shape: R = 2,048 x 64 and R = 32 x 8,192 x 64 agent rows (N = 64, A = 3), every
row valid (the most traffic the head can have).  Sides, on the same tensors in the same process:
  * fused:     `ppo_loss` forward + torch.autograd.grad w.r.t. logits and value (the head's launch,
               its finalising launch, and the backward's scaling of the stored gradients);
  * head_only: the `ppo_loss` forward alone — the launch already holds both gradients;
  * eager:     RLlib's loss written with torch f32 ops (masked means) + torch.autograd.grad.
Method: a warm-up of every side, then the sides alternated for --pairs rounds; every sample is a
device-event window over enough calls to last ~0.1 s.  Each side reports its median and its
spread (min, max).  `floor_fraction` is the bytes-only floor over the head_only median: the
kernel's bytes per row (read 8A + 8A + 4A + 4 + 4 + 4 + 1, written 8A, plus 8 / N for the value
and its gradient = 97.125 at A = 3, N = 64) at 8 TB/s.  Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "multi-agent-rl-for-autonomous-drone-swarms_amd", ROOT, ROOT / "tools"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import torch  # noqa: E402

from critic_time import alternate  # noqa: E402

COEF = dict(clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.01, kl_coeff=0.2)
HBM_BYTES_PER_S = 8e12


def eager_loss(logits, value, b, n, mean, inv_std):
    """PPOTorchPolicy.loss, f32 torch ops; `b` the batch dict."""
    a = b["actions"].shape[1]
    mu, ls = logits[:, :a], logits[:, a:]
    mu0, ls0 = b["behaviour_logits"][:, :a], b["behaviour_logits"][:, a:]
    mask = b["valid"].to(torch.float32)
    count = mask.sum()
    z = (b["actions"] - mu) * torch.exp(-ls)
    lp = (-0.5 * z * z - ls).sum(-1) - 0.5 * a * math.log(2 * math.pi)
    ratio = torch.exp(lp - b["logp"])
    adv = (b["advantage"] - mean) * inv_std
    surr = torch.minimum(adv * ratio, adv * torch.clamp(ratio, 1 - COEF["clip_param"], 1 + COEF["clip_param"]))
    v = value.reshape(-1, 1).expand(-1, n).reshape(-1)
    vf = torch.clamp((v - b["value_target"]) ** 2, max=COEF["vf_clip_param"])
    ent = ls.sum(-1) + 0.5 * a * math.log(2 * math.pi * math.e)
    kl = (ls - ls0 + (torch.exp(2 * ls0) + (mu0 - mu) ** 2) / (2 * torch.exp(2 * ls)) - 0.5).sum(-1)
    row = -surr + COEF["vf_loss_coeff"] * vf - COEF["entropy_coeff"] * ent + COEF["kl_coeff"] * kl
    return (row * mask).sum() / count


def case(dev, env_rows: int, n: int, pairs: int) -> dict:
    from swarm_marl_amd import masked_moments, ppo_loss
    a, rows = 3, env_rows * n
    gen = torch.Generator(device=dev).manual_seed(env_rows)
    rnd = lambda *s: torch.randn(s, device=dev, generator=gen)  # noqa: E731
    uni = lambda *s: torch.rand(s, device=dev, generator=gen)  # noqa: E731
    behaviour = torch.cat([uni(rows, a) * 2 - 1, uni(rows, a) * 2.5 - 2], 1).contiguous()
    actions = behaviour[:, :a] + torch.exp(behaviour[:, a:]) * rnd(rows, a)
    z = (actions - behaviour[:, :a]) * torch.exp(-behaviour[:, a:])
    value = rnd(env_rows).requires_grad_(True)
    b = dict(behaviour_logits=behaviour, actions=actions.contiguous(),
             logp=(-0.5 * z * z - behaviour[:, a:]).sum(-1) - 0.5 * a * math.log(2 * math.pi),
             advantage=rnd(rows) * 2 + 0.3,
             value_target=(value.detach().repeat_interleave(n) + rnd(rows) * 3).contiguous(),
             valid=torch.ones(rows, dtype=torch.bool, device=dev))
    logits = (behaviour + 0.15 * rnd(rows, 2 * a)).requires_grad_(True)
    mom = masked_moments(b["advantage"], b["valid"])
    mean, inv_std = (float(x) for x in mom[[1, 3]].cpu())

    def head():
        return ppo_loss(logits, value, adv_moments=mom, valid_moments=mom, **b, **COEF)[0]

    def fused():
        return torch.autograd.grad(head(), (logits, value))

    def eager():
        return torch.autograd.grad(eager_loss(logits, value, b, n, mean, inv_std), (logits, value))

    gf, ge = fused(), eager()
    res = alternate({"fused": fused, "head_only": head, "eager": eager}, pairs)
    floor_ms = rows * (8 * a * 3 + 4 * a + 13 + 8.0 / n) / HBM_BYTES_PER_S * 1e3
    return dict(case="ppo_loss", rows=rows, env_rows=env_rows, num_agents=n, act_dim=a, pairs=pairs, **res,
                speedup_vs_eager=res["eager"]["median_ms"] / res["fused"]["median_ms"],
                floor_ms=floor_ms, floor_fraction=floor_ms / res["head_only"]["median_ms"],
                max_rel_grad_diff_vs_eager=float((gf[0] - ge[0]).abs().max() / ge[0].abs().max()))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal of the tool, not a measurement)")
    args = ap.parse_args()
    if args.pairs < 3:
        ap.error("--pairs must be >= 3")
    if not torch.cuda.is_available():
        print("ppo_time.py needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    for env_rows in ((64, 512) if args.quick else (2048, 32 * 8192)):
        print(json.dumps(case(dev, env_rows, 64, args.pairs)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
