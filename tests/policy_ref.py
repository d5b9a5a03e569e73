"""Host references shared by the actor tests off the default dims (CPU and GPU), independent of the
kernels:

* `make_actor(in_dim, out_dim)`: uniform(-1, 1) / sqrt(fan_in) weights, seeded per shape (the
  `_actor` of tests/test_gpu_rollout.py at any width); `forward64`, its float64 forward;
* `obs_set(in_dim)`: 257 rows of uniform(-3, 3) observations, seeded per width;
* `sample_noise64`: the standard normals swarm_policy_forward draws in SWARM_POLICY_ACT_SAMPLE mode,
  from their definition in csrc/swarm_policy.hip, evaluated in float64.
"""
from __future__ import annotations

import numpy as np

H = 256
ROWS = 257
# (in_dim, out_dim): both minima; neighbor_k = sensed_obstacles = 0; in + 1 on a 16-wide k-step
# boundary and one past it; the single-drone D; in + 1 = 32; the default less one input; the default
# input width with the widest output; both maxima (in + 1 = 48 fills the padded K); in + 1 a multiple
# of 4 (the f32 path's kq1)
SHAPES = ((1, 2), (9, 6), (15, 2), (16, 4), (25, 6), (31, 12), (36, 6), (37, 12), (47, 12), (3, 6))


def make_actor(in_dim: int, out_dim: int, log_std_scale: float | None = None):
    """[(w, b, relu)] x 3 float32 layers in -> 256 -> 256 -> out.  With `log_std_scale` the log_std
    half of the last layer is scaled down and centred on -0.75, which keeps log_std inside
    [-2, 0.5] on `obs_set` (asserted by the caller on the logits it uses)."""
    rng = np.random.default_rng(1000 * in_dim + out_dim)
    w = [rng.uniform(-1, 1, s).astype(np.float32) / np.float32(np.sqrt(s[-1]))
         for s in ((H, in_dim), (H,), (H, H), (H,), (out_dim, H), (out_dim,))]
    if log_std_scale is not None:
        ad = out_dim // 2
        w[4][ad:] *= np.float32(log_std_scale)
        w[5][ad:] = rng.uniform(-1.0, -0.5, out_dim - ad).astype(np.float32)
    return [(w[0], w[1], True), (w[2], w[3], True), (w[4], w[5], False)]


def obs_set(in_dim: int, rows: int = ROWS) -> np.ndarray:
    return np.random.default_rng(77 + in_dim).uniform(-3, 3, (rows, in_dim)).astype(np.float32)


def forward64(layers, x: np.ndarray) -> np.ndarray:
    x = x.astype(np.float64)
    for w, b, relu in layers:
        x = x @ w.T.astype(np.float64) + b.astype(np.float64)
        if relu:
            x = np.maximum(x, 0)
    return x


TWO_PI_F32 = np.float32(6.28318530717958647692)  # the kernel's constant, rounded to f32 as hipcc does


def sample_noise64(rows: int, adim: int, seed: int, counter: int) -> np.ndarray:
    """z [rows, adim] (adim <= 6) in float64.  Per row r: Philox4x32-10 with key (seed_lo, seed_hi)
    on the counter words (r_lo, r_hi, counter_lo, counter_hi) gives x0..x3, a second block on
    (r_lo, r_hi ^ 0x80000000, counter_lo, counter_hi) gives x4..x7 (used by normals 4 and 5 only).
    Pair p: u1 = ((x[2p] >> 8) + 0.5) * 2^-24 and u2 = (x[2p+1] >> 8) * 2^-24, both formed in f32 as
    the kernel forms them (n + 0.5 is not representable for n >= 2^23 and rounds to even: that
    rounding is part of the definition), then z[2p] = sqrt(-2 ln u1) cos(2 pi u2) and z[2p+1] =
    sqrt(-2 ln u1) sin(2 pi u2) in float64, with the kernel's f32 2 pi."""
    from oracle.swarm_oracle import philox4x32_10
    r = np.arange(rows, dtype=np.uint64)
    lo32 = np.uint64(0xFFFFFFFF)
    seed, counter = int(seed) & (2**64 - 1), int(counter) & (2**64 - 1)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    c2, c3 = np.full(rows, counter & 0xFFFFFFFF, np.uint64), np.full(rows, counter >> 32, np.uint64)
    r_lo, r_hi = r & lo32, r >> np.uint64(32)
    x = philox4x32_10(r_lo, r_hi, c2, c3, k0, k1) + philox4x32_10(r_lo, r_hi ^ np.uint64(0x80000000), c2, c3, k0, k1)
    z = np.zeros((rows, 6), np.float64)
    for p in range(3):
        n1 = (x[2 * p] >> np.uint32(8)).astype(np.float32)
        n2 = (x[2 * p + 1] >> np.uint32(8)).astype(np.float32)
        u1 = ((n1 + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float64)
        u2 = (n2 * np.float32(2.0 ** -24)).astype(np.float64)
        rad = np.sqrt(-2.0 * np.log(u1))
        ang = np.float64(TWO_PI_F32) * u2
        z[:, 2 * p] = rad * np.cos(ang)
        z[:, 2 * p + 1] = rad * np.sin(ang)
    return z[:, :adim]
