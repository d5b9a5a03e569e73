#!/usr/bin/env python3
"""Timing of the perturbation layer: swarm_sense, swarm_actuate and a perturbed fragment.

One JSON line per case:
  * kernels: on 524,288 rows of D = 37 (N = 64 x E = 8,192) with the reference's full spec,
    (a) Perturbation.sense(out=buf) against the buf.copy_(vec.obs) it replaces in the collector,
    (b) Perturbation.actuate(actions) (no unperturbed counterpart: the step reads the actions in
    place), both with the bytes they move and the rate that makes;
  * collect: a 32-step fragment of N = 64 x E = 8,192 with the bf16 actor, once with perturb= (the
    full spec) and once without, on two batches of the same seed.
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

# the reference's configs/domain_randomization_v1.yaml, actuation and sensing groups
FULL_SPEC = dict(delay_values=[0, 1, 2], delay_probs=[0.7, 0.2, 0.1], thrust_noise_std=0.03, position_noise_std=0.02,
                 velocity_noise_std=0.02, obstacle_distance_noise_std=0.03)


def kernels_case(dev, n: int, e: int, pairs: int) -> dict:
    from swarm_marl_amd import Perturbation, VecSwarm
    vec = VecSwarm(e, {"num_drones": n}, device=dev, auto_reset=True, seed=1)
    vec.reset()
    per = Perturbation(vec, FULL_SPEC, seed=3)
    buf = torch.empty_like(vec.obs)
    gen = torch.Generator(device=dev).manual_seed(e)
    actions = torch.rand((e, n, 3), device=dev, generator=gen) * 3 - 1.5
    res = alternate({"sense": lambda: per.sense(out=buf), "copy": lambda: buf.copy_(vec.obs),
                     "actuate": lambda: per.actuate(actions)}, pairs)
    rows, d = e * n, vec.obs_dim
    sense_bytes = rows * (2 * 4 * d + 1)  # obs in, out, the active byte
    act_bytes = rows * 12 * 4             # actions in, ring write, ring read, eff out
    return dict(case="kernels", num_drones=n, envs=e, rows=rows, obs_dim=d, pairs=pairs, **res,
                sense_over_copy=res["sense"]["median_ms"] / res["copy"]["median_ms"],
                sense_slower_than_twice_the_copy=res["sense"]["median_ms"] > 2 * res["copy"]["median_ms"],
                sense_gb_s=sense_bytes / (res["sense"]["median_ms"] * 1e6),
                copy_gb_s=rows * 8 * d / (res["copy"]["median_ms"] * 1e6),
                actuate_gb_s=act_bytes / (res["actuate"]["median_ms"] * 1e6))


def collect_case(dev, n: int, e: int, t: int, pairs: int) -> dict:
    from swarm_marl_amd import Perturbation, RolloutCollector, VecSwarm
    from swarm_marl_amd.policy import PolicyMLP

    def make(perturbed: bool):
        vec = VecSwarm(e, {"num_drones": n}, device=dev, auto_reset=True, seed=1)
        vec.reset()
        pol = PolicyMLP.from_arrays(*[a.numpy() for wb in mlp_layers(vec.obs_dim, 1, out=6) for a in wb], device=dev,
                                    precision="bf16")
        per = Perturbation(vec, FULL_SPEC, seed=3) if perturbed else None
        return RolloutCollector(vec, pol, None, horizon=t, perturb=per)

    with_p, plain = make(True), make(False)
    res = alternate({"collect_perturbed": with_p.collect, "collect_plain": plain.collect}, pairs)
    a, b = res["collect_perturbed"], res["collect_plain"]
    return dict(case="collect", num_drones=n, envs=e, horizon=t, pairs=pairs, **res,
                perturbed_over_plain=a["median_ms"] / b["median_ms"],
                perturbed_minus_plain_ms_per_step=(a["median_ms"] - b["median_ms"]) / t,
                differs_beyond_spread=a["min_ms"] > b["max_ms"])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--skip-collect", action="store_true")
    args = ap.parse_args()
    if args.pairs < 3:
        ap.error("--pairs must be >= 3")
    if not torch.cuda.is_available():
        print("perturb_time.py needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    e, t = (64, 4) if args.quick else (8192, 32)
    print(json.dumps(kernels_case(dev, 64, e, args.pairs)), flush=True)
    if not args.skip_collect:
        print(json.dumps(collect_case(dev, 64, e, t, args.pairs)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
