"""Host references shared by the per-agent critic tests (CPU and GPU), independent of the kernels:

* `make_value(in_dim, seed)`: torch's default nn.Linear init (tests/critic_ref.py `make_critic`), and
  `truth64`, its float64 forward;
* `obs_like`: inputs laid out like an observation row (position, velocity, goal, then groups of a
  relative vector and its distance): positions and goal in +-10, velocities +-4, relative vectors
  +-20, distances 0 .. 35;
* `emulate_bf16_blob`: the bf16 kernel's arithmetic in NumPy read back from the packed blob through
  the MFMA fragment maps (operands rounded to bf16, float64 sums, activations re-rounded);
* `direct_bf16`: the same arithmetic from the dense weights, no blob;
* `gae_agent_loop`: the header's per-agent GAE loop in any float dtype;
* `consistent_flags`: episode-consistent fragment flags (a valid step that is not done is followed by
  a valid step; an agent that is done inside a running env stays invalid until the env ends), and
  `random_gae_agent_inputs`, rewards and per-agent values with them.
"""
from __future__ import annotations

import ctypes

import numpy as np

from tests import critic_ref as cr

IN_DIMS = (1, 15, 16, 25, 31, 37, 47)  # in + 1 on a k-step edge (15, 31, 47), one past (16), D = 25, the default 37
ROWS = (1, 31, 33, 63, 65, 257)
H = 256
BLOB_BYTES = (8 * 3 + 8 * 16) * 1024 + 1024 + 1024 + 16

make_value = cr.make_critic
truth64 = cr.truth64
to_bf16, from_bf16 = cr.to_bf16, cr.from_bf16
ENV_TERMINATED, ENV_TRUNCATED, ENV_RESET = cr.ENV_TERMINATED, cr.ENV_TRUNCATED, cr.ENV_RESET


def obs_like(rows: int, in_dim: int, seed: int = 0) -> np.ndarray:
    """[pos 3 | vel 3 | goal 3 | (relative vector 3, distance 1) ...] cut to in_dim columns."""
    rng = np.random.default_rng(seed)
    width = max(in_dim, 9) + 4
    x = rng.uniform(-20, 20, (rows, width))
    x[:, 0:3] = rng.uniform(-10, 10, (rows, 3))
    x[:, 3:6] = rng.uniform(-4, 4, (rows, 3))
    x[:, 6:9] = rng.uniform(-10, 10, (rows, 3))
    for c in range(12, width, 4):
        x[:, c] = rng.uniform(0, 35, rows)
    return np.ascontiguousarray(x[:, :in_dim], np.float32)


def pack(lib, layers, precision: int) -> np.ndarray:
    (w1, b1), (w2, b2), (w3, b3) = layers
    in_dim = w1.shape[1]
    nb = lib.swarm_value_packed_bytes(in_dim, precision)
    assert nb > 0
    buf = np.zeros(nb, np.uint8)
    keep = [np.ascontiguousarray(a, np.float32) for a in (w1, b1, w2, b2, w3, b3)]
    rc = lib.swarm_value_pack(in_dim, precision, *[a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) for a in keep],
                              buf.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return buf


# v_mfma_f32_32x32x16_bf16 maps (tests/critic_ref.py): A[row m][k = 8h + j] on lane 32h + m; B[k = 8h + j]
# [col n] on lane 32h + n; C[row (i & 3) + 8 (i >> 2) + 4h][col n] in register i of lane 32h + n; chained
# as the next B operand, element j of lane half h in k-step 2 ob + s is register 8 s + j of out block ob.
_REG_ROW = np.array([[(i & 3) + 8 * (i >> 2) + 4 * h for i in range(16)] for h in range(2)])
_CHAIN = np.array([[[(ks >> 1) * 32 + _REG_ROW[h, 8 * (ks & 1) + j] for j in range(8)] for h in range(2)]
                   for ks in range(16)])  # [ks, h, j] -> hidden unit


def emulate_bf16_blob(buf: np.ndarray, x: np.ndarray) -> np.ndarray:
    """blob layout: W1 [8 out blocks][3 k-steps][64 lanes][8] bf16 (k = 16 ks + 8 h + j, the bias in
    column k = in), W2 [8 out blocks][16 k-steps][64 lanes][8] bf16, b2 256 f32, w3 256 f32 (bf16
    values), b3."""
    rows, d = x.shape
    assert len(buf) == BLOB_BYTES and 1 <= d <= 47
    o1, o2 = 24 * 1024, 152 * 1024
    w1f = from_bf16(buf[:o1].view(np.uint16)).reshape(8, 3, 2, 32, 8)        # ob, ks, h, m, j
    w2f = from_bf16(buf[o1:o2].view(np.uint16)).reshape(8, 16, 2, 32, 8)     # ob, ks, h, m, j
    b2 = buf[o2:o2 + 1024].view(np.float32)
    w3 = buf[o2 + 1024:o2 + 2048].view(np.float32)
    b3 = buf[o2 + 2048:o2 + 2052].view(np.float32)[0]
    xp = np.zeros((rows, 48), np.float32)
    xp[:, :d] = x
    xp[:, d] = 1.0  # the bias column
    xb = to_bf16(xp).reshape(rows, 3, 2, 8).astype(np.float64)                # n, ks, h, j
    c1 = np.einsum("oshmj,nshj->nom", w1f.astype(np.float64), xb).reshape(rows, H)
    h1 = to_bf16(np.maximum(c1, 0).astype(np.float32)).astype(np.float64)
    h1f = h1[:, _CHAIN]                                                       # n, ks, h, j
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


def gae_agent_loop(reward, value, terminated, truncated, env_done, valid, gamma, lam, dtype=np.float32):
    """The swarm_gae_agent loop of include/swarm_mi355x.h, vectorised over (e, n), every operation in
    `dtype`; value [T+1, E, N].  Values that the loop does not read (an invalid step's, the next value
    of an invalid or done step) are masked out before any arithmetic, so they may be NaN."""
    f = dtype
    t_n, e_n, n_n = reward.shape
    assert value.shape == (t_n + 1, e_n, n_n)
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
        v = np.where(ok, value[t], zero).astype(f)
        r = np.where(ok, reward[t], zero).astype(f)
        nv = np.where(done | ~ok, zero, value[t + 1]).astype(f)
        prev = np.where(done, zero, carry).astype(f)
        delta = ((r + (gamma * nv).astype(f)).astype(f) - v).astype(f)
        c = (delta + (gl * prev).astype(f)).astype(f)
        carry = np.where(ok, c, zero).astype(f)
        adv[t] = carry
        tgt[t] = np.where(ok, (c + v).astype(f), zero)
    return adv, tgt


def consistent_flags(t_n, e_n, n_n, seed=0):
    """(terminated, truncated [T,E,N] bool, env_done [T,E] u8, valid [T,E,N] bool) of simulated
    episodes: valid[t] is the active mask before step t; an active agent terminates with p = 0.12;
    an env ends TERMINATED when its last agent does and TRUNCATED (every still-active agent
    truncated) with p = 0.1; three ended envs in four reset (RESET bit: every agent active again),
    the fourth stays inactive for the rest of the fragment.  Envs start part-way through an episode
    (some agents already inactive)."""
    rng = np.random.default_rng(seed)
    terminated = np.zeros((t_n, e_n, n_n), bool)
    truncated = np.zeros((t_n, e_n, n_n), bool)
    valid = np.zeros((t_n, e_n, n_n), bool)
    env_done = np.zeros((t_n, e_n), np.uint8)
    active = rng.random((e_n, n_n)) < 0.8
    active[np.arange(e_n), rng.integers(0, n_n, e_n)] = True  # a running env has an active agent
    for t in range(t_n):
        valid[t] = active
        term = active & (rng.random((e_n, n_n)) < 0.12)
        left = active & ~term
        running = active.any(1)
        env_term = running & ~left.any(1)
        env_trunc = running & ~env_term & (rng.random(e_n) < 0.1)
        trunc = left & env_trunc[:, None]
        ended = env_term | env_trunc
        reset = ended & (rng.random(e_n) < 0.75)
        terminated[t], truncated[t] = term, trunc
        env_done[t] = (env_term * ENV_TERMINATED + env_trunc * ENV_TRUNCATED + reset * ENV_RESET).astype(np.uint8)
        active = np.where(ended[:, None], reset[:, None] & np.ones((1, n_n), bool), left)
    return terminated, truncated, env_done, valid


def check_consistent(terminated, truncated, env_done, valid) -> None:
    """The two properties the generator promises, asserted from the flags alone."""
    t_n = valid.shape[0]
    ended = (env_done & (ENV_TERMINATED | ENV_TRUNCATED)) != 0
    done = terminated | truncated | ended[:, :, None]
    assert not (terminated & ~valid).any() and not (truncated & ~valid).any()
    for t in range(t_n - 1):
        assert valid[t + 1][valid[t] & ~done[t]].all(), t                       # valid and not done -> next valid
        inside = valid[t] & done[t] & ~ended[t][:, None]                        # done inside a running env
        assert not valid[t + 1][inside].any(), t
        assert not valid[t + 1][~valid[t] & ~ended[t][:, None]].any(), t        # stays invalid until the env ends


def random_gae_agent_inputs(t_n, e_n, n_n, seed=0):
    """(reward, value [T+1,E,N], terminated, truncated, env_done, valid) with `consistent_flags`."""
    rng = np.random.default_rng(seed + 1000)
    reward = rng.normal(0, 1, (t_n, e_n, n_n)).astype(np.float32)
    value = rng.normal(0, 2, (t_n + 1, e_n, n_n)).astype(np.float32)
    return (reward, value) + consistent_flags(t_n, e_n, n_n, seed)


def poison_unread_values(value, terminated, truncated, env_done, valid):
    """A copy of value [T+1,E,N] with NaN wherever the loop must not read: value[t] of an invalid
    step, and value[T] where step T-1 is invalid or done.  (With consistent flags value[t+1] behind an
    invalid or done step t < T-1 is either the value of an invalid step, poisoned, or that of the
    first step after an env end, which step t + 1 itself reads.)"""
    t_n = valid.shape[0]
    out = value.copy()
    out[:t_n][~valid] = np.nan
    done = terminated[-1] | truncated[-1] | ((env_done[-1] & (ENV_TERMINATED | ENV_TRUNCATED)) != 0)[:, None]
    out[t_n][~valid[-1] | done] = np.nan
    return out
