"""PPO on collected fragments: the fused loss head and a learner.

`ppo_loss` is RLlib's PPOTorchPolicy.loss (clipped surrogate, clipped value loss, entropy bonus, KL
penalty against the behaviour policy, the mean over valid rows) and its gradient in one kernel pass
over the agent rows (swarm_ppo_loss, csrc/swarm_ppo.hip; the arithmetic is written out in
include/swarm_mi355x.h).  It is a torch.autograd.Function: the forward launches the head and keeps
d loss / d logits and d loss / d value, the backward hands them to autograd, so the actor's and the
critic's MLPs (torch, hipBLASLt) train through it.  `masked_moments` is RLlib's standardized()
statistics (swarm_masked_moments).  `PPOLearner` runs the update of a RolloutCollector fragment:

    col = RolloutCollector(vec, policy, critic, horizon=32)
    learner = PPOLearner(policy, critic, minibatch_env_rows=4096)
    info = learner.update(col.collect())       # policy / critic now hold the new weights

Rows are grouped by env-row — one (t, e) with its N agents, the collector's [T, E, N, ...] flatten —
and values are per env-row.  With an `AgentValueMLP` as the critic the value net runs
on the minibatch's obs rows and the head is called with one value per agent row (num_agents = 1).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native as nat
from .actor_train import ActorTrainer
from .attention import AttentionActor, AttentionPolicy
from .critic import CriticMLP
from .policy import PolicyMLP
from .rollout import _F32, _U8, _check, _stream
from .value import AgentValueMLP

STATS = ("count", "total_loss", "policy_loss", "vf_loss", "entropy", "kl", "clip_frac")
_F64 = (torch.float64,)


def _workspace(device) -> torch.Tensor:
    return torch.empty(nat.PPO_WORKSPACE_BYTES // 8, dtype=torch.float64, device=device)


def masked_moments(x: torch.Tensor, valid: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """float64 [4] on the device: (count, mean, population std, 1 / max(std, 1e-4)) of x over the
    elements with valid != 0; mean 0 and inverse std 1e4 when there is none.  Two launches, async on
    the current stream, bitwise repeatable."""
    if not isinstance(x, torch.Tensor):
        raise ValueError("x must be a tensor")
    _check("x", x, x.shape, _F32)
    _check("valid", valid, x.shape, _U8, x.device)
    if out is None:
        out = torch.empty(nat.PPO_MOMENTS, dtype=torch.float64, device=x.device)
    else:
        _check("out", out, (nat.PPO_MOMENTS,), _F64, x.device)
    if x.numel() == 0:
        out.copy_(torch.tensor([0.0, 0.0, 0.0, 1e4], dtype=torch.float64))
        return out
    lib = nat.load_library()
    nat.check(lib.swarm_masked_moments(x.data_ptr(), valid.data_ptr(), x.numel(), _workspace(x.device).data_ptr(),
                                       out.data_ptr(), _stream(x.device)), lib, which="ppo")
    return out


def _flat(t, *shape):
    """t viewed as `shape` when its element count fits; anything else is left for `_check` to name."""
    return t.reshape(shape) if isinstance(t, torch.Tensor) and t.numel() == int(np.prod(shape)) else t


class _PPOLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, value, behaviour_logits, actions, logp, advantage, value_target, valid, adv_moments,
                valid_moments, num_agents, coef):
        dev = logits.device
        rows, adim = actions.shape
        grad_logits = torch.empty_like(logits)
        grad_value = torch.empty_like(value)
        stats = torch.empty(nat.PPO_STATS, dtype=torch.float64, device=dev)
        work = _workspace(dev)
        args = nat.SwarmPpoArgs(logits.data_ptr(), behaviour_logits.data_ptr(), actions.data_ptr(), logp.data_ptr(),
                                advantage.data_ptr(), value_target.data_ptr(), value.data_ptr(), valid.data_ptr(),
                                adv_moments.data_ptr(), valid_moments.data_ptr(), grad_logits.data_ptr(),
                                grad_value.data_ptr(), stats.data_ptr(), work.data_ptr(), rows, num_agents, adim, *coef)
        lib = nat.load_library()
        nat.check(lib.swarm_ppo_loss(ctypes.byref(args), _stream(dev)), lib, which="ppo")
        ctx.save_for_backward(grad_logits, grad_value)
        ctx.mark_non_differentiable(stats)
        return stats[1].to(torch.float32), stats

    @staticmethod
    def backward(ctx, grad_loss, _grad_stats):
        grad_logits, grad_value = ctx.saved_tensors
        return (grad_logits * grad_loss, grad_value * grad_loss) + (None,) * 10


def ppo_loss(logits: torch.Tensor, value: torch.Tensor, *, behaviour_logits: torch.Tensor, actions: torch.Tensor,
             logp: torch.Tensor, advantage: torch.Tensor, value_target: torch.Tensor, valid: torch.Tensor,
             adv_moments: torch.Tensor, valid_moments: torch.Tensor | None = None, clip_param: float = 0.3,
             vf_clip_param: float = 10.0, vf_loss_coeff: float = 1.0, entropy_coeff: float = 0.0,
             kl_coeff: float = 0.2):
    """(loss, stats): the 0-dim float32 PPO loss of R = env_rows x N agent rows, differentiable in
    `logits` [R, 2A] and `value` [env_rows], and the float64 `STATS` vector (not differentiable).

    behaviour_logits [R, 2A], actions [R, A], logp / advantage / value_target / valid [R] are the
    collector's tensors (leading dims flattened or not: only the element counts and the last dim
    of logits and actions matter).  adv_moments: `masked_moments` of the advantages to standardise
    with (the whole fragment's, RLlib-style); valid_moments: `masked_moments` over exactly these
    rows (its count is the M of the mean), computed here when None.  The defaults are RLlib's.
    One fused launch plus a one-wave finalising launch, async on the current stream."""
    if not isinstance(actions, torch.Tensor) or actions.dim() < 1 or not actions.is_cuda:
        raise ValueError("actions must be a GPU tensor [..., A]")
    dev = actions.device
    adim = int(actions.shape[-1])
    rows = actions.numel() // max(adim, 1)
    if not 1 <= adim <= nat.PPO_MAX_ACT:
        raise ValueError(f"actions are {adim} wide, the head takes 1..{nat.PPO_MAX_ACT} action dims")
    if not isinstance(value, torch.Tensor) or value.numel() < 1 or rows % value.numel():
        raise ValueError(f"value must hold one element per env-row: {rows} rows do not divide into "
                         f"{value.numel() if isinstance(value, torch.Tensor) else 0} env-rows")
    env_rows = value.numel()
    n = rows // env_rows
    if not 1 <= n <= nat.PPO_MAX_AGENTS:
        raise ValueError(f"{n} agents per env-row, the head takes 1..{nat.PPO_MAX_AGENTS}")
    logits, behaviour_logits = _flat(logits, rows, 2 * adim), _flat(behaviour_logits, rows, 2 * adim)
    actions, value = _flat(actions, rows, adim), _flat(value, env_rows)
    logp, advantage, value_target, valid = (_flat(t, rows) for t in (logp, advantage, value_target, valid))
    _check("logits", logits, (rows, 2 * adim), _F32, dev)
    _check("behaviour_logits", behaviour_logits, (rows, 2 * adim), _F32, dev)
    _check("actions", actions, (rows, adim), _F32, dev)
    _check("value", value, (env_rows,), _F32, dev)
    for name, t in (("logp", logp), ("advantage", advantage), ("value_target", value_target)):
        _check(name, t, (rows,), _F32, dev)
    _check("valid", valid, (rows,), _U8, dev)
    _check("adv_moments", adv_moments, (nat.PPO_MOMENTS,), _F64, dev)
    if valid_moments is None:
        valid_moments = masked_moments(advantage, valid)
    _check("valid_moments", valid_moments, (nat.PPO_MOMENTS,), _F64, dev)
    coef = tuple(float(c) for c in (clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff))
    return _PPOLoss.apply(logits, value, behaviour_logits, actions, logp, advantage, value_target, valid,
                          adv_moments, valid_moments, n, coef)


def _mlp(layers, device) -> torch.nn.Sequential:
    """A float32 torch MLP (relu between the dense layers) holding the given [(w [out,in], b [out])]."""
    mods = []
    for i, (w, b) in enumerate(layers):
        lin = torch.nn.Linear(int(w.shape[1]), int(w.shape[0]))
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(np.asarray(w, np.float32)))
            lin.bias.copy_(torch.from_numpy(np.asarray(b, np.float32).reshape(-1)))
        mods.append(lin)
        if i + 1 < len(layers):
            mods.append(torch.nn.ReLU())
    return torch.nn.Sequential(*mods).to(device)


def _layers_of(mlp: torch.nn.Sequential):
    return [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in mlp
            if isinstance(m, torch.nn.Linear)]


class PPOLearner:
    """PPO updates of a `PolicyMLP` / `CriticMLP` pair from RolloutCollector fragments.

    The trainable copies are float32 torch MLPs (`actor`: D -> 256 -> 256 -> 2A, `value_net`:
    G -> 256 -> 256 -> 1, relu) initialised from `policy.layers` / `critic.layers`, under one
    torch.optim.Adam.  With an `AttentionPolicy` the actor is an `AttentionActor` (the reference's
    module on nn.MultiheadAttention, initialised from `policy.params` / `policy.layers`) under the same
    Adam, written back with `load_params`.  `update(batch)`: the advantage moments once over the whole fragment; per
    epoch a seeded permutation of the env-rows; per minibatch of `minibatch_env_rows` env-rows an
    index_select gather into preallocated buffers, the valid count, both forwards, `ppo_loss`,
    backward and an Adam step; then RLlib's adaptive KL coefficient from the last epoch's mean KL
    (x 1.5 above 2 x kl_target, x 0.5 below 0.5 x kl_target; the update's one read of a device
    result) and the new weights pushed into `policy` / `critic` in place (`load_layers`: the packers
    are host code, so the weights pass through host memory once per update).

    With an `AgentValueMLP` as `critic` (the per-agent value tower of the reference's multi-agent and
    single-agent PPO set-ups) `value_net` is D -> 256 -> 256 -> 1 on the minibatch's obs rows, `ppo_loss`
    gets one value per agent row, and a fragment without `global_state` is accepted.

    backend="hip" (needs a `PolicyMLP` of precision "bf16") trains the actor on the
    device instead: the parameters under Adam are an `ActorTrainer`'s float32 masters, a minibatch's
    logits come from the inference kernel itself as a leaf tensor, `loss.backward()` stops there and at
    the value net, `trainer.backward` turns d loss / d logits into the masters' gradients, and after the
    Adam step `trainer.push()` repacks the blob on the device — in place, so a captured collector keeps
    its graph.  A bf16 collector is then exactly on-policy.  `policy.layers` is refreshed by one
    device-to-host copy at the end of `update`.  The value net stays torch in either backend.
    """

    def __init__(self, policy: PolicyMLP, critic: CriticMLP | AgentValueMLP, *, lr: float = 3e-4, num_epochs: int = 10,
                 minibatch_env_rows: int, kl_target: float = 0.01, seed: int = 0, backend: str = "torch", **loss_kw):
        if not isinstance(policy, (PolicyMLP, AttentionPolicy)) or not isinstance(critic, (CriticMLP, AgentValueMLP)):
            raise ValueError("PPOLearner needs a PolicyMLP and a CriticMLP")
        if backend not in ("torch", "hip"):
            raise ValueError(f"backend must be 'torch' or 'hip', got {backend!r}")
        if backend == "hip" and not (isinstance(policy, PolicyMLP) and policy.precision == "bf16"):
            raise ValueError("backend='hip' trains a PolicyMLP of precision 'bf16' (not an AttentionPolicy, not f32 / f32x3)")
        self.backend = backend
        self.per_agent = isinstance(critic, AgentValueMLP)
        if self.per_agent and critic.in_dim != policy.in_dim:
            raise ValueError(f"the per-agent critic takes {critic.in_dim} inputs, the policy's observations are "
                             f"{policy.in_dim} wide")
        if policy.device != critic.device:
            raise ValueError(f"policy is on {policy.device}, critic on {critic.device}")
        if policy.out_dim % 2 or not 1 <= policy.out_dim // 2 <= nat.PPO_MAX_ACT:
            raise ValueError(f"policy has {policy.out_dim} outputs, expected [mean | log_std] of 1..{nat.PPO_MAX_ACT} dims")
        if int(num_epochs) < 1 or int(minibatch_env_rows) < 1:
            raise ValueError("num_epochs and minibatch_env_rows must be >= 1")
        unknown = set(loss_kw) - {"clip_param", "vf_clip_param", "vf_loss_coeff", "entropy_coeff", "kl_coeff"}
        if unknown:
            raise ValueError(f"unknown loss parameters {sorted(unknown)}")
        self.policy, self.critic, self.device = policy, critic, policy.device
        self.num_epochs, self.minibatch_env_rows = int(num_epochs), int(minibatch_env_rows)
        self.kl_target = float(kl_target)
        self.kl_coeff = float(loss_kw.pop("kl_coeff", 0.2))
        self.loss_kw = loss_kw
        self.trainer = ActorTrainer(policy) if backend == "hip" else None
        self.actor = (None if self.trainer else AttentionActor.from_policy(policy).to(self.device)
                      if isinstance(policy, AttentionPolicy) else _mlp(policy.layers, self.device))
        self.value_net = _mlp(critic.layers, self.device)
        actor_params = self.trainer.parameters() if self.trainer else list(self.actor.parameters())
        self.optimizer = torch.optim.Adam(actor_params + list(self.value_net.parameters()), lr=lr)
        self.generator = torch.Generator(device=self.device).manual_seed(int(seed))
        self._adv_moments = torch.empty(nat.PPO_MOMENTS, dtype=torch.float64, device=self.device)
        self._valid_moments = torch.empty(nat.PPO_MOMENTS, dtype=torch.float64, device=self.device)
        self._buf = None

    def _buffers(self, n: int, d: int, a: int, g: int):
        m = self.minibatch_env_rows
        key = (m, n, d, a, g)
        if self._buf is None or self._buf[0] != key:
            kw = dict(device=self.device)
            f32 = torch.float32
            self._buf = (key, dict(
                obs=torch.empty((m, n, d), dtype=f32, **kw), behaviour_logits=torch.empty((m, n, 2 * a), dtype=f32, **kw),
                actions=torch.empty((m, n, a), dtype=f32, **kw), logp=torch.empty((m, n), dtype=f32, **kw),
                advantage=torch.empty((m, n), dtype=f32, **kw), value_target=torch.empty((m, n), dtype=f32, **kw),
                valid=torch.empty((m, n), dtype=torch.bool, **kw), global_state=torch.empty((m, g), dtype=f32, **kw)))
        return self._buf[1]

    def update(self, batch: dict) -> dict:
        """One PPO update from a `RolloutCollector.collect()` dict.  Returns the last epoch's mean
        stats (`STATS` keys, floats), `epoch_total_loss` (the mean total loss of every epoch) and
        the new `kl_coeff`.  Minibatches stay grouped by env-row in either critic mode: a minibatch is
        `minibatch_env_rows` whole (t, e) rows with all their N agents, also when the value is per agent."""
        valid = batch["valid"]
        if self.per_agent:
            return self._update(batch, 0)
        if batch.get("global_state") is None:
            raise ValueError("the fragment has no global_state: collect with VecSwarm(..., with_global_state=True)")
        return self._update(batch, int(batch["global_state"].shape[-1]))

    def _update(self, batch: dict, g: int) -> dict:
        """`update` for a fragment whose global_state is g wide; g = 0: the per-agent critic, which
        reads no global_state."""
        valid = batch["valid"]
        t, e, n = (int(s) for s in valid.shape)
        d, a = int(batch["obs"].shape[-1]), int(batch["actions"].shape[-1])
        if d != self.policy.in_dim or 2 * a != self.policy.out_dim or (g if g else d) != self.critic.in_dim:
            raise ValueError(f"fragment is obs {d} / actions {a} / global_state {g} wide, the learner's networks take "
                             f"{self.policy.in_dim} / {self.policy.out_dim // 2} / {self.critic.in_dim}")
        te = t * e
        src = dict(obs=batch["obs"].reshape(te, n, d), behaviour_logits=batch["logits"].reshape(te, n, 2 * a),
                   actions=batch["actions"].reshape(te, n, a), logp=batch["logp"].reshape(te, n),
                   advantage=batch["advantage"].reshape(te, n), value_target=batch["value_target"].reshape(te, n),
                   valid=valid.reshape(te, n))
        if g:
            src["global_state"] = batch["global_state"][:t].reshape(te, g)
        buf = self._buffers(n, d, a, g)
        masked_moments(batch["advantage"], valid, out=self._adv_moments)
        mb = self.minibatch_env_rows
        epochs = torch.zeros((self.num_epochs, nat.PPO_STATS), dtype=torch.float64, device=self.device)
        nmb = (te + mb - 1) // mb
        for ep in range(self.num_epochs):
            perm = torch.randperm(te, device=self.device, generator=self.generator)
            for i in range(nmb):
                idx = perm[i * mb:(i + 1) * mb]
                m = int(idx.numel())
                cur = {k: buf[k][:m] for k in src}
                for k in cur:
                    torch.index_select(src[k], 0, idx, out=cur[k])
                masked_moments(cur["advantage"], cur["valid"], out=self._valid_moments)
                obs_mb = cur["obs"].view(m * n, d)
                logits = self.trainer.logits(obs_mb).requires_grad_(True) if self.trainer else self.actor(obs_mb)
                value = (self.value_net(cur["global_state"]).view(m) if g else
                         self.value_net(cur["obs"].view(m * n, d)).view(m * n))
                loss, stats = ppo_loss(logits, value, behaviour_logits=cur["behaviour_logits"], actions=cur["actions"],
                                       logp=cur["logp"], advantage=cur["advantage"], value_target=cur["value_target"],
                                       valid=cur["valid"], adv_moments=self._adv_moments,
                                       valid_moments=self._valid_moments, kl_coeff=self.kl_coeff, **self.loss_kw)
                self.optimizer.zero_grad(set_to_none=True)
                loss.backward()
                if self.trainer:
                    self.trainer.backward(obs_mb, logits.grad)
                self.optimizer.step()
                if self.trainer:
                    self.trainer.push()
                epochs[ep] += stats
        epochs /= nmb
        host = epochs.cpu().numpy()  # the update's one read of a device result
        info = {k: float(v) for k, v in zip(STATS, host[-1])}
        if info["kl"] > 2.0 * self.kl_target:
            self.kl_coeff *= 1.5
        elif info["kl"] < 0.5 * self.kl_target:
            self.kl_coeff *= 0.5
        info["kl_coeff"] = self.kl_coeff
        info["epoch_total_loss"] = [float(v) for v in host[:, 1]]
        if self.trainer:
            self.trainer.sync_policy()
        elif isinstance(self.policy, AttentionPolicy):
            self.policy.load_params(*self.actor.split_state())
        else:
            self.policy.load_layers(_layers_of(self.actor))
        self.critic.load_layers(_layers_of(self.value_net))
        return info
