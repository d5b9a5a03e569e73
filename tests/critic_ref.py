"""Host references shared by the critic / rollout tests (CPU and GPU), independent of the kernels:

* `make_critic(in_dim, seed)`: torch's default nn.Linear init, and `truth64`, its float64 forward;
* `global_state_like`: inputs laid out like a global state (positions, goal in +-10, velocities +-2);
* `emulate_bf16_blob`: the bf16 kernel's arithmetic in NumPy read back from the packed blob through
  the MFMA fragment maps (operands rounded to bf16, float64 sums, activations re-rounded);
* `direct_bf16`: the same arithmetic from the dense weights, no blob;
* `gae_loop`: the header's GAE loop in any float dtype; `logp64`: the Gaussian log-density.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

# in_dim + 1 on / just over / just under a multiple of 16; N = 64; N = 256 (nc1 = ceil((in + 1) / 32) W1
# chunks: 1, 1, 1, 13, 49, all odd); then the minimum, in + 1 on / just over / just under 32 and 64, in
# on 64 and 128 (the f32 kernel's 64-term blocks), N = 8 and N = 16: nc1 = 1, 1, 2, 2, 2, 3, 4, 5 (with
# an even nc1 the first W2 chunk and a tile's last chunk sit in the other LDS buffer)
IN_DIMS = (15, 16, 21, 387, 1539, 1, 31, 32, 51, 63, 64, 99, 128)
H = 256


def make_critic(in_dim: int, seed: int = 0):
    """[(w, b)] x 3 float32 arrays of a torch nn.Linear stack in -> 256 -> 256 -> 1 (default init)."""
    state = torch.random.get_rng_state()
    torch.manual_seed(1000 + seed)
    try:
        lins = [torch.nn.Linear(in_dim, H), torch.nn.Linear(H, H), torch.nn.Linear(H, 1)]
    finally:
        torch.random.set_rng_state(state)
    return [(lin.weight.detach().numpy().copy(), lin.bias.detach().numpy().copy()) for lin in lins]


def truth64(layers, x: np.ndarray) -> np.ndarray:
    """torch on the CPU in float64: an nn.Linear stack with the given weights."""
    mods = []
    for i, (w, b) in enumerate(layers):
        lin = torch.nn.Linear(w.shape[1], w.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w).double())
            lin.bias.copy_(torch.from_numpy(b).double())
        mods.append(lin)
        if i < 2:
            mods.append(torch.nn.ReLU())
    with torch.no_grad():
        return torch.nn.Sequential(*mods)(torch.from_numpy(x).double()).numpy()[:, 0]


def global_state_like(rows: int, in_dim: int, seed: int = 0) -> np.ndarray:
    """concat(pos 3N, vel 3N, goal 3) for the largest N that fits, the rest position-like."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-10, 10, (rows, in_dim)).astype(np.float32)
    n = max((in_dim - 3) // 6, 0)
    x[:, 3 * n:6 * n] = rng.uniform(-2, 2, (rows, 3 * n)).astype(np.float32)
    return x


def pack(lib, layers, precision: int) -> np.ndarray:
    (w1, b1), (w2, b2), (w3, b3) = layers
    in_dim = w1.shape[1]
    nb = lib.swarm_critic_packed_bytes(in_dim, precision)
    assert nb > 0
    buf = np.zeros(nb, np.uint8)
    keep = [np.ascontiguousarray(a, np.float32) for a in (w1, b1, w2, b2, w3, b3)]
    rc = lib.swarm_critic_pack(in_dim, precision, *[a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) for a in keep],
                               buf.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return buf


def from_bf16(u16: np.ndarray) -> np.ndarray:
    return (u16.astype(np.uint32) << 16).view(np.float32)


def to_bf16(x: np.ndarray) -> np.ndarray:
    """float32 values rounded to bf16 (nearest even), as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return from_bf16(u.astype(np.uint16)).reshape(np.shape(x))


# v_mfma_f32_32x32x16_bf16 maps: A[row m][k = 8h + j] on lane 32h + m; B[k = 8h + j][col n] on lane
# 32h + n; C[row (i & 3) + 8 (i >> 2) + 4h][col n] in register i of lane 32h + n.  A layer's
# accumulators chained as the next B operand: element j of lane half h in k-step 2 ob + s is
# register 8 s + j of out block ob.
_REG_ROW = np.array([[(i & 3) + 8 * (i >> 2) + 4 * h for i in range(16)] for h in range(2)])
_CHAIN = np.array([[[(ks >> 1) * 32 + _REG_ROW[h, 8 * (ks & 1) + j] for j in range(8)] for h in range(2)]
                   for ks in range(16)])  # [ks, h, j] -> hidden unit


def emulate_bf16_blob(buf: np.ndarray, x: np.ndarray) -> np.ndarray:
    """blob layout: nc1 = ceil((in + 1) / 32) W1 chunks [2 k-steps][8 out blocks][64 lanes][8] bf16,
    W2 [8 out blocks][16 k-steps][64 lanes][8] bf16, b2 256 f32, w3 256 f32 (bf16 values), b3."""
    rows, d = x.shape
    nc1 = (d + 1 + 31) // 32
    off = nc1 * 16384
    w1f = from_bf16(buf[:off].view(np.uint16)).reshape(nc1, 2, 8, 2, 32, 8)       # c, ks, ob, h, m, j
    w2f = from_bf16(buf[off:off + 8 * 16384].view(np.uint16)).reshape(8, 16, 2, 32, 8)  # ob, ks, h, m, j
    off += 8 * 16384
    b2 = buf[off:off + 1024].view(np.float32)
    w3 = buf[off + 1024:off + 2048].view(np.float32)
    b3 = buf[off + 2048:off + 2052].view(np.float32)[0]
    assert len(buf) == off + 2048 + 16
    xp = np.zeros((rows, nc1 * 32), np.float32)
    xp[:, :d] = x
    xp[:, d] = 1.0  # the bias column
    xb = to_bf16(xp).reshape(rows, nc1, 2, 2, 8).astype(np.float64)               # n, c, ks, h, j
    c1 = np.einsum("csohmj,ncshj->nom", w1f.astype(np.float64), xb).reshape(rows, H)
    h1 = to_bf16(np.maximum(c1, 0).astype(np.float32)).astype(np.float64)
    h1f = h1[:, _CHAIN]                                                           # n, ks, h, j
    c2 = np.einsum("okhmj,nkhj->nom", w2f.astype(np.float64), h1f).reshape(rows, H) + b2
    h2 = to_bf16(np.maximum(c2, 0).astype(np.float32)).astype(np.float64)
    return h2 @ w3.astype(np.float64) + np.float64(b3)


def direct_bf16(layers, x: np.ndarray) -> np.ndarray:
    (w1, b1), (w2, b2), (w3, b3) = layers
    f64 = np.float64
    w1b = to_bf16(np.concatenate([w1, b1[:, None]], axis=1)).astype(f64)
    xb = to_bf16(np.concatenate([x, np.ones((len(x), 1), np.float32)], axis=1)).astype(f64)
    h1 = to_bf16(np.maximum(xb @ w1b.T, 0).astype(np.float32)).astype(f64)
    h2 = to_bf16(np.maximum(h1 @ to_bf16(w2).astype(f64).T + b2, 0).astype(np.float32)).astype(f64)
    return h2 @ to_bf16(w3[0]).astype(f64) + f64(b3[0])


ENV_TERMINATED, ENV_TRUNCATED, ENV_RESET = 1, 2, 4


def gae_loop(reward, value, terminated, truncated, env_done, valid, gamma, lam, dtype=np.float32):
    """The loop of include/swarm_mi355x.h, vectorised over (e, n), every operation in `dtype`."""
    f = dtype
    t_n, e_n, n_n = reward.shape
    reward, value = reward.astype(f), value.astype(f)
    gamma, lam = f(gamma), f(lam)
    gl = f(gamma * lam)
    adv = np.zeros((t_n, e_n, n_n), f)
    tgt = np.zeros((t_n, e_n, n_n), f)
    carry = np.zeros((e_n, n_n), f)
    zero = f(0)
    for t in range(t_n - 1, -1, -1):
        ok = valid[t].astype(bool)
        done = (terminated[t].astype(bool) | truncated[t].astype(bool)
                | ((env_done[t] & (ENV_TERMINATED | ENV_TRUNCATED)) != 0)[:, None])
        v = value[t][:, None]
        nv = np.where(done, zero, value[t + 1][:, None]).astype(f)
        prev = np.where(done, zero, carry).astype(f)
        delta = ((reward[t] + (gamma * nv).astype(f)).astype(f) - v).astype(f)
        c = (delta + (gl * prev).astype(f)).astype(f)
        carry = np.where(ok, c, zero).astype(f)
        adv[t] = carry
        tgt[t] = np.where(ok, (c + v).astype(f), zero)
    return adv, tgt


def random_gae_inputs(t_n, e_n, n_n, seed=0):
    """Rewards, values and flags with valid == 0 runs, per-agent ends and env_done bits with and
    without RESET."""
    rng = np.random.default_rng(seed)
    reward = rng.normal(0, 1, (t_n, e_n, n_n)).astype(np.float32)
    value = rng.normal(0, 2, (t_n + 1, e_n)).astype(np.float32)
    terminated = rng.random((t_n, e_n, n_n)) < 0.1
    truncated = (rng.random((t_n, e_n, n_n)) < 0.05) & ~terminated
    valid = rng.random((t_n, e_n, n_n)) > 0.2
    bits = np.array([0, 0, 0, 0, ENV_RESET, ENV_TERMINATED, ENV_TERMINATED | ENV_RESET, ENV_TRUNCATED,
                     ENV_TRUNCATED | ENV_RESET], np.uint8)
    env_done = bits[rng.integers(0, len(bits), (t_n, e_n))]
    return reward, value, terminated, truncated, env_done, valid


def logp64(logits: np.ndarray, actions: np.ndarray) -> np.ndarray:
    lg, a = logits.astype(np.float64), actions.astype(np.float64)
    ad = a.shape[-1]
    mean, ls = lg[..., :ad], lg[..., ad:]
    z = (a - mean) * np.exp(-ls)
    return (-0.5 * z * z - ls).sum(-1) - 0.5 * ad * np.log(2 * np.pi)
