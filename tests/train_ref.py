"""Host references for the bf16 actor's backward (csrc/swarm_train.hip), independent of the kernels.

* `bf16`: round to nearest even onto the bf16 grid, from float64, in float64; `bits`: the bf16 bit
  patterns of values already on that grid.
* The stages of include/swarm_mi355x.h's swarm_policy_backward one by one, every sum in float64:
  `stage_h1`, `stage_h2`, `stage_dz2`, `stage_dz1` return (pre, out, mag): the value before its bf16
  rounding (after the relu or the mask), the rounded value, and sum_k |a_k b_k| of the sum behind it;
  `weight_grads` returns the six gradients and the six sum|terms|.  Fed the kernel's own upstream
  stage outputs they give per-stage references whose errors do not compound.
* `emulate`: the stages chained (rounding=False: no rounding anywhere, which must equal `plain_backward`).
* `plain_backward`: the float64 gradient of the unrounded network for a given d loss / d logits.
* `int_fixture`: small-integer weights, observations and logit gradients for which every value of
  the backward is an integer that bf16 and f32 hold exactly.
"""
from __future__ import annotations

import numpy as np

H = 256
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")


def bf16(x) -> np.ndarray:
    """x (float64) rounded to nearest even onto the bf16 grid, as float64 (normal range)."""
    x = np.ascontiguousarray(x, np.float64)
    u = x.view(np.uint64)
    drop = np.uint64(45)  # 52 - 7 mantissa bits
    lsb = (u >> drop) & np.uint64(1)
    r = (u + (np.uint64((1 << 44) - 1) + lsb)) >> drop << drop
    return r.view(np.float64).reshape(x.shape)


def bits(x) -> np.ndarray:
    """bf16 bit patterns (uint16) of values on the bf16 grid; -0 is written as +0."""
    f = (np.asarray(x, np.float64) + 0.0).astype(np.float32)
    assert np.array_equal(f.astype(np.float64), np.asarray(x, np.float64) + 0.0)
    u = np.ascontiguousarray(f).view(np.uint32)
    assert not (u & np.uint32(0xFFFF)).any(), "not on the bf16 grid"
    return (u >> np.uint32(16)).astype(np.uint16)


def from_bits(b) -> np.ndarray:
    """float64 values of bf16 bit patterns (any integer dtype holding 16 bits)."""
    u = (np.asarray(b).astype(np.int64) & 0xFFFF).astype(np.uint32) << np.uint32(16)
    return u.view(np.float32).astype(np.float64)


def _r(x, rounding):
    return bf16(x) if rounding else np.asarray(x, np.float64)


def widen(x, rounding=True):
    """x~: the obs rows with the 1 in column D, rounded."""
    x = np.asarray(x, np.float64)
    return _r(np.concatenate([x, np.ones((x.shape[0], 1))], axis=1), rounding)


def _affine(a, w, bias=None):
    """(a w^T + bias, |a| |w|^T + |bias|) in float64."""
    s, m = a @ w.T, np.abs(a) @ np.abs(w).T
    if bias is not None:
        s, m = s + bias, m + np.abs(bias)
    return s, m


def stage_h1(w1, b1, x, rounding=True):
    w = _r(np.concatenate([np.asarray(w1, np.float64), np.asarray(b1, np.float64).reshape(-1, 1)], axis=1), rounding)
    s, m = _affine(widen(x, rounding), w)
    return np.maximum(s, 0), np.maximum(_r(s, rounding), 0), m


def stage_h2(w2, b2, h1, rounding=True):
    s, m = _affine(h1, _r(np.asarray(w2, np.float64), rounding), np.asarray(b2, np.float64))  # b2 stays f32
    return np.maximum(s, 0), np.maximum(_r(s, rounding), 0), m


def stage_dz2(w3, g, h2, rounding=True):
    s, m = _affine(_r(np.asarray(g, np.float64), rounding), _r(np.asarray(w3, np.float64), rounding).T)
    mask = h2 > 0
    return np.where(mask, s, 0), np.where(mask, _r(s, rounding), 0), m


def stage_dz1(w2, dz2, h1, rounding=True):
    s, m = _affine(dz2, _r(np.asarray(w2, np.float64), rounding).T)
    mask = h1 > 0
    return np.where(mask, s, 0), np.where(mask, _r(s, rounding), 0), m


def weight_grads(x, g, h1, h2, dz2, dz1, rounding=True):
    """({name: gradient}, {name: sum over rows of |term|}) from the rounded stage values."""
    xw = widen(x, rounding)
    gb = _r(np.asarray(g, np.float64), rounding)
    d = xw.shape[1] - 1
    out, mag = {}, {}
    for name, a, b in (("w1", dz1, xw[:, :d]), ("w2", dz2, h1), ("w3", gb, h2)):
        out[name], mag[name] = a.T @ b, np.abs(a).T @ np.abs(b)
    for name, a in (("b1", dz1), ("b2", dz2), ("b3", gb)):
        out[name], mag[name] = a.sum(axis=0), np.abs(a).sum(axis=0)
    return out, mag


def emulate(layers, x, g, rounding=True):
    """Every stage and gradient of swarm_policy_backward with the documented roundings (or none)."""
    (w1, b1), (w2, b2), (w3, b3) = [(l[0], l[1]) for l in layers]
    _, h1, _ = stage_h1(w1, b1, x, rounding)
    _, h2, _ = stage_h2(w2, b2, h1, rounding)
    _, dz2, _ = stage_dz2(w3, g, h2, rounding)
    _, dz1, _ = stage_dz1(w2, dz2, h1, rounding)
    grads, _ = weight_grads(x, g, h1, h2, dz2, dz1, rounding)
    return dict(h1=h1, h2=h2, dz2=dz2, dz1=dz1), grads


def plain_backward(layers, x, g):
    """{name: float64 gradient} of sum(logits * g) for the unrounded network, written out by hand."""
    (w1, b1), (w2, b2), (w3, b3) = [(np.asarray(l[0], np.float64), np.asarray(l[1], np.float64).reshape(-1)) for l in layers]
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    z1 = x @ w1.T + b1
    h1 = np.maximum(z1, 0)
    z2 = h1 @ w2.T + b2
    h2 = np.maximum(z2, 0)
    dz2 = (g @ w3) * (z2 > 0)
    dz1 = (dz2 @ w2) * (z1 > 0)
    return dict(w1=dz1.T @ x, b1=dz1.sum(0), w2=dz2.T @ h1, b2=dz2.sum(0), w3=g.T @ h2, b3=g.sum(0))


def int_fixture(in_dim: int, out_dim: int, rows: int, seed: int = 0):
    """(layers [(w, b, relu)] x 3, x [rows, in_dim], g [rows, out_dim]), all float32 small integers:
    x, g in {-2..2}; W1 in {-1, 0, 1} with at most 3 nonzeros per row, b1 in {-1, 0, 1} (|z1| <= 7);
    W2[o][i] = +-1 only for i in {o, o + 7, o + 31} mod 256 (3 nonzeros per row and per column), b2 in
    {-1, 0, 1} (|z2| <= 22); W3 in {-1, 0, 1}, b3 in {-2..2} (|dz2| <= 24, |dz1| <= 72).  Every
    activation, dz and product is an integer below 256 and every row sum stays below 2^24 up to 87,000
    rows (192 per row at most), so bf16 and f32 hold all of it exactly."""
    assert rows * 192 < 2 ** 24
    rng = np.random.default_rng(9000 + 100 * in_dim + out_dim + seed)
    w1 = np.zeros((H, in_dim), np.float32)
    for o in range(H):
        cols = rng.choice(in_dim, size=min(3, in_dim), replace=False)
        w1[o, cols] = rng.choice([-1.0, 1.0], size=cols.size)
    w2 = np.zeros((H, H), np.float32)
    for o in range(H):
        for k in (0, 7, 31):
            w2[o, (o + k) % H] = rng.choice([-1.0, 1.0])
    w3 = rng.integers(-1, 2, (out_dim, H)).astype(np.float32)
    b1, b2 = (rng.integers(-1, 2, H).astype(np.float32) for _ in range(2))
    b3 = rng.integers(-2, 3, out_dim).astype(np.float32)
    x = rng.integers(-2, 3, (rows, in_dim)).astype(np.float32)
    g = rng.integers(-2, 3, (rows, out_dim)).astype(np.float32)
    g[rng.random(rows) < 0.2] = 0  # rows that must add exactly nothing
    return [(w1, b1, True), (w2, b2, True), (w3, b3, False)], x, g
