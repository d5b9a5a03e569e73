"""Reference for the PPO loss head (include/swarm_mi355x.h, "PPO loss head").

`loss` is RLlib's PPOTorchPolicy.loss written with torch ops (torch.minimum, torch.clamp, a masked
mean, the env-row value expanded to its agents) in whatever dtype and on whatever device its
inputs have: float64 on the CPU with autograd is the reference of the kernel tests, float32 on the
GPU the eager chain the autograd test and tools/ppo_time.py compare with.  `closed_form_grads`
evaluates the gradient formulas the kernel is held to (NumPy float64); `moments` is RLlib's
standardized() statistics in NumPy float64.  `make_case` draws the inputs of a kernel test.
"""
from __future__ import annotations

import math

import numpy as np
import torch

COEF = dict(clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2)
STATS = ("count", "total_loss", "policy_loss", "vf_loss", "entropy", "kl", "clip_frac")


def moments(x, valid):
    """(count, mean, population std, 1 / max(std, 1e-4)) over valid rows; mean 0 / 1e4 with none."""
    sel = np.asarray(x, np.float64).reshape(-1)[np.asarray(valid).reshape(-1) != 0]
    if sel.size == 0:
        return np.array([0.0, 0.0, 0.0, 1e4])
    sd = sel.std()
    return np.array([float(sel.size), sel.mean(), sd, 1.0 / max(sd, 1e-4)])


def loss(logits, value, behaviour_logits, actions, logp, advantage, value_target, valid, adv_mean, adv_inv_std, *,
         clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff):
    """(total, stats dict of tensors, per-row ratio, per-row squared value error).  logits [R,2A],
    value [R/N]; rows with valid == 0 are replaced by benign numbers before any arithmetic and
    masked out of every mean."""
    r_, a2 = logits.shape
    a = a2 // 2
    n = r_ // value.numel()
    m = valid.reshape(-1) != 0
    mf = m.to(logits.dtype)
    count = mf.sum()

    def clean(x, fill=0.0):
        mask = m.reshape((-1,) + (1,) * (x.dim() - 1))
        return torch.where(mask, x, torch.full_like(x, fill))

    logits, behaviour_logits, actions = clean(logits), clean(behaviour_logits), clean(actions)
    logp, advantage, value_target = clean(logp), clean(advantage), clean(value_target)
    mu, ls = logits[:, :a], logits[:, a:]
    mu0, ls0 = behaviour_logits[:, :a], behaviour_logits[:, a:]
    new = torch.distributions.Normal(mu, torch.exp(ls))
    old = torch.distributions.Normal(mu0, torch.exp(ls0))
    lp = new.log_prob(actions).sum(-1)
    ratio = torch.exp(lp - logp)
    adv = (advantage - adv_mean) * adv_inv_std
    s1 = adv * ratio
    s2 = adv * torch.clamp(ratio, 1.0 - clip_param, 1.0 + clip_param)
    surr = torch.minimum(s1, s2)
    v_agent = value.reshape(-1, 1).expand(-1, n).reshape(-1)
    err2 = (v_agent - value_target) ** 2
    vf = torch.clamp(err2, max=vf_clip_param)
    ent = new.entropy().sum(-1)
    kl = torch.distributions.kl_divergence(old, new).sum(-1)

    def mean_valid(x):
        return (x * mf).sum() / count

    stats = dict(count=count, policy_loss=mean_valid(-surr), vf_loss=mean_valid(vf), entropy=mean_valid(ent),
                 kl=mean_valid(kl), clip_frac=mean_valid((s2 < s1).to(logits.dtype)))
    total = mean_valid(-surr + vf_loss_coeff * vf - entropy_coeff * ent + kl_coeff * kl)
    stats["total_loss"] = total
    return total, stats, ratio, err2


def closed_form_grads(logits, value, behaviour_logits, actions, logp, advantage, value_target, valid, adv_mean,
                      adv_inv_std, *, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff):
    """(grad_logits [R,2A], grad_value [R/N]) of the mean loss by the formulas of the issue, NumPy f64."""
    f = lambda x: np.asarray(x, np.float64)  # noqa: E731
    logits, b, act = f(logits), f(behaviour_logits), f(actions)
    a = act.shape[1]
    n = logits.shape[0] // np.asarray(value).size
    m = np.asarray(valid).reshape(-1) != 0
    inv = 1.0 / m.sum()
    g = np.zeros_like(logits)
    gv = np.zeros(np.asarray(value).size)
    for i in np.nonzero(m)[0]:
        mu, s, mu0, s0 = logits[i, :a], logits[i, a:], b[i, :a], b[i, a:]
        z = (act[i] - mu) * np.exp(-s)
        lp = np.sum(-0.5 * z * z - s) - 0.5 * a * math.log(2 * math.pi)
        r = math.exp(lp - float(logp[i]))
        adv = (float(advantage[i]) - adv_mean) * adv_inv_std
        blocked = (adv > 0 and r > 1 + clip_param) or (adv < 0 and r < 1 - clip_param)
        w = 0.0 if blocked else -adv * r
        u = np.exp(2 * s0) + (mu0 - mu) ** 2
        g[i, :a] = inv * (w * z * np.exp(-s) + kl_coeff * (mu - mu0) * np.exp(-2 * s))
        g[i, a:] = inv * (w * (z * z - 1) - entropy_coeff + kl_coeff * (1 - u * np.exp(-2 * s)))
        d = float(value[i // n]) - float(value_target[i])
        if d * d < vf_clip_param:
            gv[i // n] += inv * vf_loss_coeff * 2 * d
    return g, gv


def make_case(env_rows: int, n: int, a: int, seed: int, coef=None, *, target_spread: float = 3.0):
    """float32 NumPy inputs of a head test: log-std in [-2, 0.5], new logits = behaviour + N(0, 0.15),
    ~20 % of the rows invalid (a tenth of the env-rows wholly), targets `target_spread` around the
    values so that some rows reach vf_clip_param.  A row whose ratio falls within 2e-3 of a clip
    boundary 1 +- clip_param, or whose squared value error within 2e-3 of vf_clip_param, is moved off
    it (behaviour logp + 0.02, target + 0.05 away from the value): a float32 kernel and a float64
    reference may not take different branches there, and no seed keeps 16,640 rows clear of both."""
    coef = coef or COEF
    rng = np.random.default_rng(seed)
    r = env_rows * n
    mu0 = rng.uniform(-1, 1, (r, a))
    ls0 = rng.uniform(-2, 0.5, (r, a))
    behaviour = np.concatenate([mu0, ls0], 1).astype(np.float32)
    logits = (behaviour + rng.normal(0, 0.15, (r, 2 * a))).astype(np.float32)
    actions = (mu0 + np.exp(ls0) * rng.normal(0, 1, (r, a))).astype(np.float32)
    b64 = behaviour.astype(np.float64)
    z = (actions - b64[:, :a]) * np.exp(-b64[:, a:])
    logp = (np.sum(-0.5 * z * z - b64[:, a:], 1) - 0.5 * a * math.log(2 * math.pi)).astype(np.float32)
    advantage = rng.normal(0.3, 2.0, r).astype(np.float32)
    value = rng.normal(0, 1, env_rows).astype(np.float32)
    value_target = (np.repeat(value, n) + rng.normal(0, target_spread, r)).astype(np.float32)
    valid = rng.random(r) < 0.85
    dead = rng.random(env_rows) < 0.1
    dead[0] = False
    if env_rows > 1:
        dead[env_rows // 2] = True
    valid &= ~np.repeat(dead, n)
    valid[0] = True  # never an empty batch
    l64 = logits.astype(np.float64)
    zn = (actions - l64[:, :a]) * np.exp(-l64[:, a:])
    lp_new = np.sum(-0.5 * zn * zn - l64[:, a:], 1) - 0.5 * a * math.log(2 * math.pi)
    ratio = np.exp(lp_new - logp)
    near = np.minimum(np.abs(ratio - (1 + coef["clip_param"])), np.abs(ratio - (1 - coef["clip_param"]))) < 2e-3
    logp = np.where(near, logp + np.float32(0.02), logp).astype(np.float32)
    d = np.repeat(value, n).astype(np.float64) - value_target
    near = np.abs(d * d - coef["vf_clip_param"]) < 2e-3
    value_target = np.where(near, value_target - np.sign(d).astype(np.float32) * np.float32(0.05), value_target).astype(np.float32)
    return dict(logits=logits, value=value, behaviour_logits=behaviour, actions=actions, logp=logp,
                advantage=advantage, value_target=value_target, valid=valid)


def reference(case, coef):
    """float64 CPU reference of a make_case() dict: dict(total, stats, grad_logits, grad_value, ratio, err2,
    adv_moments)."""
    t = {k: torch.from_numpy(np.asarray(v, np.float64 if v.dtype != bool else bool)) for k, v in case.items()}
    mom = moments(case["advantage"], case["valid"])
    lg = t["logits"].clone().requires_grad_(True)
    val = t["value"].clone().requires_grad_(True)
    total, stats, ratio, err2 = loss(lg, val, t["behaviour_logits"], t["actions"], t["logp"], t["advantage"],
                                     t["value_target"], t["valid"], float(mom[1]), float(mom[3]), **coef)
    total.backward()
    return dict(total=float(total.detach()), stats={k: float(v.detach()) for k, v in stats.items()}, grad_logits=lg.grad.numpy(),
                grad_value=val.grad.numpy(), ratio=ratio.detach().numpy(), err2=err2.detach().numpy(), adv_moments=mom)
