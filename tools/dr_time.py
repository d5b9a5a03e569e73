#!/usr/bin/env python3
"""Timing of the keyed domain randomiser inside rollout fragments.

One JSON line per case:
  * collect: a 32-step fragment with the bf16 actor and the bf16 centralized critic at
    N x E = 3 x 1,024, 8 x 8,192 and 64 x 8,192, in one process, from seven collectors of one seed:
      eager                 (a) eager, no randomiser (the specialised step kernel where there is one)
      eager_generator       (b) eager, DomainRandomizer in generator mode
      eager_keyed           (c) eager, DomainRandomizer(keyed=True)
      graph                 (d) graph, no randomiser
      graph_keyed           (e) graph, DomainRandomizer(keyed=True)
      eager_records / graph_records   as (a) / (d) with uniform per-env records: any randomiser moves
                            the step to the generic kernel, and these two show that share of (b) - (a)
                            and (e) - (d) on its own
    with `keyed_bitwise_equal` (two fragments of (c) and (e), every tensor and both record buffers);
  * launch: swarm_env_cfg_randomize alone at E = 8,192: every env written (mask NULL), and
    `after_step()` on the mask the last step left (the envs it reset).
Method (tools/rollout_graph_time.py's): a warm-up of every side (the graph sides have captured by
then), then the sides alternated for --rounds rounds; every sample is one window over enough calls to
last ~0.1 s (at least 3), timed by device events around the calls and by the host clock to the end of a
final synchronisation.  Each side reports the median and the spread (min, max) of both; rounds x calls
is at least 21 fragments per side.  Needs a GPU: there is no fallback.
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
import yaml  # noqa: E402

from critic_time import mlp_layers  # noqa: E402
from rollout_graph_time import alternate  # noqa: E402

SHAPES = ((3, 1024), (8, 8192), (64, 8192))
DR_PATH = ROOT / "tests" / "golden" / "domain_randomization_v1.yaml"
SIDES = (("eager", False, None), ("eager_generator", False, "generator"), ("eager_keyed", False, "keyed"),
         ("graph", True, None), ("graph_keyed", True, "keyed"), ("eager_records", False, "records"),
         ("graph_records", True, "records"))


def make(dev, dr_cfg, n: int, e: int, t: int, graph: bool, randomiser):
    from swarm_marl_amd import CriticMLP, RolloutCollector, VecSwarm
    from swarm_marl_amd.domain_randomization import DomainRandomizer
    from swarm_marl_amd.policy import PolicyMLP
    vec = VecSwarm(e, {"num_drones": n}, device=dev, auto_reset=True, seed=1, with_global_state=True)
    dr = None
    if randomiser == "records":
        vec.set_env_config()
        vec.set_env_config(next_episode=True)
        vec.reset()
    elif randomiser is not None:
        dr = DomainRandomizer(vec, dr_cfg, seed=3, force=True, keyed=randomiser == "keyed")
        dr.begin()
    else:
        vec.reset()
    pol = PolicyMLP.from_arrays(*[a.numpy() for wb in mlp_layers(vec.obs_dim, 1, out=6) for a in wb], device=dev,
                                precision="bf16")
    critic = CriticMLP([(w.numpy(), b.numpy()) for w, b in mlp_layers(6 * n + 3, n)], device=dev, precision="bf16")
    return RolloutCollector(vec, pol, critic, horizon=t, randomizer=dr, graph=graph)


def collect_case(dev, dr_cfg, n: int, e: int, t: int, rounds: int) -> dict:
    cols = {name: make(dev, dr_cfg, n, e, t, graph, rnd) for name, graph, rnd in SIDES}
    ea, gr = cols["eager_keyed"], cols["graph_keyed"]
    same = True
    for _ in range(2):
        a, b = ea.collect(), gr.collect()
        same = same and all(torch.equal(v, b[k]) for k, v in a.items() if v is not None)
    same = same and all(torch.equal(v, gr.vec.state_dict()[k]) for k, v in ea.vec.state_dict().items())
    same = same and torch.equal(ea.vec.env_cfg, gr.vec.env_cfg) and torch.equal(ea.vec.env_cfg_next, gr.vec.env_cfg_next)
    res = alternate({name: col.collect for name, col in cols.items()}, rounds)
    med = {k: v["median_ms"] for k, v in res.items()}
    wall = {k: v["wall_median_ms"] for k, v in res.items()}

    def beyond(x, y):  # x slower than y beyond both spreads
        return res[x]["min_ms"] > res[y]["max_ms"]

    return dict(case="collect", num_drones=n, envs=e, horizon=t, rounds=rounds, **res,
                kernel={k: c.vec.kernel_name() for k, c in cols.items()}, keyed_bitwise_equal=bool(same),
                generator_cost_ms=med["eager_generator"] - med["eager"], keyed_eager_cost_ms=med["eager_keyed"] - med["eager"],
                keyed_graph_cost_ms=med["graph_keyed"] - med["graph"],
                keyed_graph_cost_over_generator_cost=(med["graph_keyed"] - med["graph"]) / (med["eager_generator"] - med["eager"]),
                keyed_graph_cost_beyond_records_ms=med["graph_keyed"] - med["graph_records"],
                keyed_eager_cost_beyond_records_ms=med["eager_keyed"] - med["eager_records"],
                generator_cost_beyond_records_ms=med["eager_generator"] - med["eager_records"],
                generator_cost_wall_ms=wall["eager_generator"] - wall["eager"],
                keyed_eager_cost_wall_ms=wall["eager_keyed"] - wall["eager"],
                keyed_graph_cost_wall_ms=wall["graph_keyed"] - wall["graph"],
                keyed_over_generator=med["eager_keyed"] / med["eager_generator"],
                keyed_over_generator_wall=wall["eager_keyed"] / wall["eager_generator"],
                keyed_slower_than_generator_beyond_spread=beyond("eager_keyed", "eager_generator"))


def launch_case(dev, dr_cfg, e: int, rounds: int) -> dict:
    from swarm_marl_amd import VecSwarm
    from swarm_marl_amd.domain_randomization import DomainRandomizer
    vec = VecSwarm(e, {"num_drones": 3, "max_steps": 8}, device=dev, auto_reset=True, seed=1)
    dr = DomainRandomizer(vec, dr_cfg, seed=3, force=True, keyed=True)
    dr.begin()
    gen = torch.Generator(device=dev).manual_seed(2)
    for _ in range(8):  # the eighth step truncates and resets every env
        vec.step(torch.rand((e, 3, 3), device=dev, generator=gen) * 2 - 1)
        dr.after_step()
    reset = int(((vec.env_done & 4) != 0).sum())
    res = alternate({"all_envs": lambda: dr._launch(vec.env_cfg_next, 1, None, 0xFF), "after_step": dr.after_step}, rounds)
    return dict(case="launch", envs=e, envs_reset_by_last_step=reset, rounds=rounds, **res,
                all_envs_us=res["all_envs"]["median_ms"] * 1e3, after_step_us=res["after_step"]["median_ms"] * 1e3)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--only", choices=["collect", "launch"], default=None)
    ap.add_argument("--shape", type=int, default=None, help="index into the collect shapes (default: all)")
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("--rounds must be >= 7 (at least 21 fragments per side)")
    if not torch.cuda.is_available():
        print("dr_time.py needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    dr_cfg = yaml.safe_load(DR_PATH.read_text())
    shapes, t, big = (((3, 16), (8, 16)), 4, 64) if args.quick else (SHAPES, 32, 8192)
    if args.only in (None, "launch"):
        print(json.dumps(launch_case(dev, dr_cfg, big, args.rounds)), flush=True)
    if args.only in (None, "collect"):
        for i, (n, e) in enumerate(shapes):
            if args.shape is None or args.shape == i:
                print(json.dumps(collect_case(dev, dr_cfg, n, e, t, args.rounds)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
