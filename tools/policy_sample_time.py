#!/usr/bin/env python3
"""Timing of the sampled epilogue of the f32x3 and f32 actor kernels.

One JSON line per case:
  * policy, f32x3 and f32: PolicyMLP.forward writing logits and actions for D = 37 x 524,288 rows
    (64 x 8,192 agents), mean mode and sampled mode alternated in one process.  With --parent-lib
    the same mean-mode launch of a library built from the parent commit joins the alternation: it
    is called through the C-ABI with this build's handle (the blob formats did not change), so
    "mean mode did not move" is read off two sides of one run on one box.
  * collect: collect() at N = 64 x E = 8,192 x T = 32 with the bf16 critic, once with the sampling
    f32x3 actor and once with the bf16 actor (tools/critic_time.py's shape).
Method: a warm-up of every side, then the sides alternated for --pairs rounds; every sample is a
device-event window over enough calls to last ~0.1 s.  Each side reports its median and its
spread (min, max).  Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "multi-agent-rl-for-autonomous-drone-swarms_amd", ROOT, ROOT / "tools"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import torch  # noqa: E402

from critic_time import alternate, mlp_layers  # noqa: E402


def _arrays(d: int, seed: int, out: int):
    return [a.numpy() for wb in mlp_layers(d, seed, out=out) for a in wb]


def parent_forward(path: str):
    """swarm_policy_forward of another build of the library (or of its policy unit alone)."""
    from swarm_marl_amd import _native as nat
    lib = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    lib.swarm_policy_forward.restype = ctypes.c_int
    lib.swarm_policy_forward.argtypes = [ctypes.POINTER(nat.SwarmPolicy), vp, ctypes.c_longlong, vp, vp, ctypes.c_int,
                                         ctypes.c_ulonglong, ctypes.c_ulonglong, vp]
    return lib.swarm_policy_forward


def policy_case(dev, precision: str, rows: int, pairs: int, parent) -> dict:
    from swarm_marl_amd.policy import PolicyMLP
    d = 37
    pol = PolicyMLP.from_arrays(*_arrays(d, 1, 6), device=dev, precision=precision)
    gen = torch.Generator(device=dev).manual_seed(rows)
    obs = (torch.rand((rows, d), device=dev, generator=gen) * 20 - 10).contiguous()
    logits = torch.empty((rows, 6), dtype=torch.float32, device=dev)
    actions = torch.empty((rows, 3), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    sides = {"mean": lambda: pol.forward(obs, logits=logits, actions=actions),
             "sampled": lambda: pol.forward(obs, logits=logits, actions=actions, sample=True, seed=1, counter=3)}
    if parent is not None:
        def parent_mean():
            rc = parent(ctypes.byref(pol._c), obs.data_ptr(), rows, logits.data_ptr(), actions.data_ptr(), 0, 0, 0, stream)
            if rc != 0:
                raise RuntimeError(f"the parent build's swarm_policy_forward returned {rc}")
        sides["parent_mean"] = parent_mean
    res = alternate(sides, pairs)
    out = dict(case="policy", precision=precision, in_dim=d, rows=rows, pairs=pairs, **res,
               sampled_over_mean=res["sampled"]["median_ms"] / res["mean"]["median_ms"])
    if parent is not None:
        m, q = res["mean"], res["parent_mean"]
        out["mean_over_parent_mean"] = m["median_ms"] / q["median_ms"]
        out["mean_moved_beyond_spread"] = m["min_ms"] > q["max_ms"] or m["max_ms"] < q["min_ms"]
        parent_mean()
        ref = logits.clone()
        pol.forward(obs, logits=logits, actions=actions)
        out["mean_logits_bitwise_equal_parent"] = bool(torch.equal(ref.view(torch.int32), logits.view(torch.int32)))
    return out


def collect_case(dev, n: int, e: int, t: int, pairs: int) -> dict:
    from swarm_marl_amd import CriticMLP, RolloutCollector, VecSwarm
    from swarm_marl_amd.policy import PolicyMLP

    def make(precision: str):
        vec = VecSwarm(e, {"num_drones": n}, device=dev, auto_reset=True, seed=1, with_global_state=True)
        vec.reset()
        pol = PolicyMLP.from_arrays(*_arrays(vec.obs_dim, 1, 6), device=dev, precision=precision)
        critic = CriticMLP([(w.numpy(), b.numpy()) for w, b in mlp_layers(6 * n + 3, n)], device=dev, precision="bf16")
        return RolloutCollector(vec, pol, critic, horizon=t)

    x3, b16 = make("f32x3"), make("bf16")
    res = alternate({"collect_f32x3_actor": x3.collect, "collect_bf16_actor": b16.collect}, pairs)
    ms = res["collect_f32x3_actor"]["median_ms"]
    return dict(case="collect", num_drones=n, envs=e, horizon=t, pairs=pairs, **res,
                f32x3_agent_steps_per_s=e * n * t / (ms * 1e-3), f32x3_ms_per_step=ms / t)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library to time mean mode against")
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--skip-collect", action="store_true")
    args = ap.parse_args()
    if args.pairs < 3:
        ap.error("--pairs must be >= 3")
    if not torch.cuda.is_available():
        print("policy_sample_time.py needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    parent = parent_forward(args.parent_lib) if args.parent_lib else None
    for precision in ("f32x3", "f32"):
        print(json.dumps(policy_case(dev, precision, 1024 if args.quick else 64 * 8192, args.pairs, parent)), flush=True)
    if not args.skip_collect:
        e, t = (64, 4) if args.quick else (8192, 32)
        print(json.dumps(collect_case(dev, 64, e, t, args.pairs)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
