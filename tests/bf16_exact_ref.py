"""Fixtures on which the bf16 actor, value and critic kernels have no freedom at all, and their
reference (NumPy only; independent of the kernels, of the packers and of every blob).

The arithmetic, from include/swarm_mi355x.h (bf = round to nearest even onto the bf16 grid):
    x~ = bf(x | 1)                       the observation row widened with the bias column
    h1 = relu(bf(bf([W1 | b1]) x~))      b1 is rounded along with W1
    h2 = relu(bf(bf(W2) h1 + b2))        b2 stays f32
    out = bf(W3) h2 + b3                 b3 stays f32; for the towers W3 is the one bf16-rounded row w3
every product of two bf16 values (exact in f32), every sum an f32 accumulation in an order the
header leaves to the kernel: MFMA k-steps, chained accumulators, the towers' VALU layer-3 sum.

The budget rule.  The fixtures hold small integers (and values that ROUND to small integers), so
after the operand roundings every term a_k b_k of every sum is an integer.  If
    sum_k |a_k b_k| + |bias| < 2^24
every partial sum in any order is an integer below 2^24, which f32 holds exactly: the f32 sum equals
the exact sum whatever its order (`budget` returns the three maxima; tests/test_bf16_exact_cpu.py
asserts them and accumulates in three orders).  The bf16 rounding of an exact integer is a pure
function, so h1, h2 and the outputs are fully determined: kernel and reference must agree bit for bit
although activations reach 2^16 and round constantly, exact ties included (257 -> 256, 259 -> 260).

`fixture(kind, in_dim, out_dim, rows, seed)`:
    W1, b1, x   integers in -3..3 (-1..1 from in_dim 387 on); eight units' b1 from +-257..263
    x[:, -1]    six rows in ten from {257, 259, -261, -263, 2, 0, -1}, the others integers in
                -264..264 (so that a one-column input still has a hundred distinct rows)
    W2 in -2..2, W3 in -1..1, b2 from {-3, -1, 0, 2, 257, -1025}, b3 from {-2, 0, 1, 259, -1027}
and one entry in ten of x, W1, b1, W2 and W3 whose integer is +-1, +-2 or +-3 is replaced by a
neighbour that bf16 does not hold and that rounds back to the integer: half a bf16 step below it (a
tie that goes up, to the even neighbour), half a step above (a tie that goes down), a quarter step
below or above (no tie).  So the ROUNDED operands are the recipe's integers and the budget is the
recipe's, while truncation, round-half-up or a missing rounding each give another operand.  b2 and
b3 hold 257, 259, -1025 and -1027, which bf16 does not hold: a kernel or packer that rounds them is
off by one or more (b3[0] is always one of 259 and -1027, and with it b3[-1] the other).  Four
"quiet" hidden units have six +-1 in their W2 row and a small b2, so their h2 stays small, and W3
holds one of 257, 259, -261, -263 in each of their columns: integer weights that tie in both
directions, within the layer-3 budget; in the backward they take dz2 and dz1 past 256, where those
round.  `wide=False` leaves out the +-264 column and the +-257..263 biases (`train_fixture`: the
weight gradients sum over rows and have a budget of their own, `grad_budget`).

`forward(layers, x, fault=None)` evaluates the formulas above in float64 (exact here) and returns
dict(z1, h1, z2, h2, out); with `fault` the same arithmetic broken one way (FAULTS), in the style of
tests/exact_ref.py: a fault that no output bit notices means the fixture is too weak.
`classes(pre)` counts the four rounding classes among values about to be rounded.
"""
from __future__ import annotations

import numpy as np

H = 256
ROWS = 257
LIMIT = 2.0 ** 24
f64 = np.float64

# the shapes of tests/test_gpu_bf16_exact.py (and of tests/test_bf16_exact_cpu.py)
ACTOR_SHAPES = ((37, 6), (37, 4), (36, 6), (1, 2), (15, 12), (16, 2), (31, 8), (32, 10), (47, 12), (47, 2))
ACTOR_PREFIXES = (1, 31, 32, 33, 255, 256, 257)
VALUE_IN_DIMS = (37, 36, 1, 15, 16, 31, 32, 47)
CRITIC_IN_DIMS = (1, 30, 31, 32, 63, 64, 387, 1539)
CRITIC_ROWS = (1, 127, 128, 129, 257)
TRAIN_SHAPES = ((37, 6), (47, 12), (1, 2))
TRAIN_ROWS = (33, 257)

SPECIAL = (257, 259, -261, -263, 2, 0, -1)
B1_WIDE = (257, 259, -261, -263)
B2_SET = (-3, -1, 0, 2, 257, -1025)
B3_SET = (-2, 0, 1, 259, -1027)

SITES = ("x", "w1", "w2", "w3", "h1", "h2")
# (kind, argument).  trunc / half_up: that rounding in place of round-to-nearest-even at one site
# (half_up: ties away from zero); b2_bf16 / b3_bf16: the bias rounded to bf16; b2_swap: b2 of unit u
# taken from u ^ 4 (the accumulator's lane-half swap); w2_halfswap: in chained k-step ks (the 16 units
# 16 ks .. 16 ks + 15) W2's operand carries the other lane half's columns, u ^ 4; bias_col: the 1 of the
# bias column at k = in - 1 (over the last input) or k = in + 1 (where W1~ is zero); w3_leak (actor):
# row `out` of the layer-3 fragment is not masked and its sum lands one past the row's logits, on
# logit 0 of the next row; w3_unrounded (towers): w3 taken as f32.
FAULTS = (tuple(("trunc", s) for s in SITES) + tuple(("half_up", s) for s in SITES)
          + (("b2_bf16", 0), ("b3_bf16", 0), ("b2_swap", 0), ("w2_halfswap", 0), ("w2_halfswap", 9),
             ("bias_col", -1), ("bias_col", 1), ("w3_leak", 0), ("w3_unrounded", 0)))


def faults_of(kind: str):
    skip = "w3_unrounded" if kind == "actor" else "w3_leak"
    return tuple(f for f in FAULTS if f[0] != skip)


# ---------------------------------------------------------------- rounding
def round_bf16(x, mode: str = "rne") -> np.ndarray:
    """float64 -> the bf16 grid (normal range), as float64.  rne: nearest, ties to the even
    neighbour; trunc: towards zero; half_up: nearest, ties away from zero."""
    x = np.ascontiguousarray(x, f64)
    u = x.view(np.uint64)
    drop = np.uint64(45)  # 52 - 7 mantissa bits
    if mode == "rne":
        u = u + (np.uint64((1 << 44) - 1) + ((u >> drop) & np.uint64(1)))
    elif mode == "half_up":
        u = u + np.uint64(1 << 44)
    elif mode != "trunc":
        raise ValueError(mode)
    return (u >> drop << drop).view(f64).reshape(x.shape)


def classes(pre) -> dict:
    """Of the values `pre` that bf16 does not hold: how many are ties that round-to-nearest-even
    takes down (towards zero), ties it takes up (away from zero), non-ties that go up, non-ties that
    go down."""
    a = np.abs(np.asarray(pre, f64)).ravel()
    lo = round_bf16(a, "trunc")
    rne = round_bf16(a)
    _, e = np.frexp(a)                                  # a = m 2^e, m in [0.5, 1): the bf16 step is 2^(e - 8)
    d, half = a - lo, np.ldexp(0.5, e - 8)
    off = d > 0
    tie = off & (d == half)
    return dict(tie_down=int((tie & (rne == lo)).sum()), tie_up=int((tie & (rne > lo)).sum()),
                up=int((off & ~tie & (d > half)).sum()), down=int((off & ~tie & (d < half)).sum()))


def off_grid(a) -> np.ndarray:
    """Mask of the values bf16 does not hold."""
    a = np.asarray(a, f64)
    return round_bf16(a, "trunc") != a


# ---------------------------------------------------------------- the fixtures
# bf16 steps below and above the integers 1, 2, 3 (the grid's step doubles at 1, 2 and 4)
_STEP = {1: (2.0 ** -8, 2.0 ** -7), 2: (2.0 ** -7, 2.0 ** -6), 3: (2.0 ** -6, 2.0 ** -6)}


def _sprinkle(a: np.ndarray, rng, share: float = 0.1) -> np.ndarray:
    """A float32 copy of the integer array `a` in which `share` of the entries +-1, +-2, +-3 sit half
    or a quarter of a bf16 step off their integer (and round back to it)."""
    out = a.astype(f64)
    flat, src = out.reshape(-1), a.reshape(-1)
    for v, (below, above) in _STEP.items():
        idx = np.flatnonzero(np.abs(src) == v)
        idx = idx[rng.random(idx.size) < share]
        delta = np.array([-below / 2, above / 2, -below / 4, above / 4])[np.arange(idx.size) % 4]
        flat[idx] = np.sign(src[idx]) * (v + delta)
    out32 = out.astype(np.float32)
    assert np.array_equal(out32.astype(f64), out) and np.array_equal(round_bf16(out), round_bf16(a.astype(f64)))
    return out32


def fixture(kind: str, in_dim: int, out_dim: int = 1, rows: int = ROWS, seed: int = 0, wide: bool = True):
    """(layers, x [rows, in_dim]) float32.  kind "actor": layers [(w, b, relu)] x 3 as PolicyMLP takes
    them; kind "tower": [(w, b)] x 3 with w3 [1, 256] as CriticMLP / AgentValueMLP take them."""
    if kind not in ("actor", "tower") or (kind == "tower" and out_dim != 1):
        raise ValueError((kind, out_dim))
    rng = np.random.default_rng([31337, int(kind == "tower"), in_dim, out_dim, seed])
    m = 3 if in_dim < 387 else 1
    w1 = rng.integers(-m, m + 1, (H, in_dim))
    b1 = rng.integers(-m, m + 1, H)
    x = rng.integers(-m, m + 1, (rows, in_dim))
    w2 = rng.integers(-2, 3, (H, H))
    w3 = rng.integers(-1, 2, (out_dim, H))
    b2 = rng.choice(B2_SET, H).astype(np.float32)
    b3 = rng.choice(B3_SET, out_dim).astype(np.float32)
    b3[[0, -1]] = rng.permutation(B3_SET[-2:])   # out_dim 1: one of the two
    col = np.where(rng.random(rows) < 0.6, rng.choice(SPECIAL, rows), rng.integers(-264, 265, rows))
    units, big_b1 = rng.choice(H, 8, replace=False), rng.choice(B1_WIDE, 8)
    if wide:
        x[:, -1], b1[units] = col, big_b1
    # four quiet units: six +-1 in their W2 row and a small b2 keep their h2 small, so W3 may hold a
    # +-257..263 in their column
    quiet = rng.choice(H, 4, replace=False)
    w2[quiet] = 0
    for u in quiet:
        w2[u, rng.choice(H, 6, replace=False)] = rng.choice([-1, 1], 6)
    b2[quiet] = rng.choice(B2_SET[:4], 4)
    w3[rng.integers(0, out_dim, 4), quiet] = rng.permutation(B1_WIDE)
    x, w1, b1, w2, w3 = (_sprinkle(a, rng) for a in (x, w1, b1, w2, w3))
    if kind == "actor":
        return [(w1, b1, True), (w2, b2, True), (w3, b3, False)], x
    return [(w1, b1), (w2, b2), (w3, b3)], x


def _wb(layers):
    return [(np.asarray(l[0], f64), np.asarray(l[1], f64).reshape(-1)) for l in layers]


def forward(layers, x, fault=None) -> dict:
    """dict(z1, h1, z2, h2, out) in float64: z the sums before their rounding, out [rows, out_dim]
    (a tower: [rows])."""
    if fault is not None and fault not in FAULTS:
        raise ValueError(fault)
    kind, arg = fault if fault is not None else (None, None)

    def rd(site, v):
        return round_bf16(v, kind if kind in ("trunc", "half_up") and arg == site else "rne")

    (w1, b1), (w2, b2), (w3, b3) = _wb(layers)
    x = np.asarray(x, f64)
    rows, d = x.shape
    xa = np.concatenate([x, np.ones((rows, 1)), np.zeros((rows, 1))], axis=1)   # columns d (bias) and d + 1 (pad)
    wa = np.concatenate([w1, b1[:, None], np.zeros((H, 1))], axis=1)
    if kind == "bias_col":
        xa[:, d] = 0.0
        xa[:, d + arg] = 1.0
    z1 = rd("x", xa) @ rd("w1", wa).T
    h1 = np.maximum(rd("h1", z1), 0)
    w2t = rd("w2", w2)
    if kind == "w2_halfswap":
        blk = 16 * arg + np.arange(16)
        w2t[:, blk] = w2t[:, blk ^ 4]
    if kind == "b2_bf16":
        b2 = round_bf16(b2)
    elif kind == "b2_swap":
        b2 = b2[np.arange(H) ^ 4]
    z2 = h1 @ w2t.T + b2
    h2 = np.maximum(rd("h2", z2), 0)
    w3t = w3 if kind == "w3_unrounded" else rd("w3", w3)
    if kind == "b3_bf16":
        b3 = round_bf16(b3)
    out = h2 @ w3t.T + b3
    if kind == "w3_leak":
        n = out.shape[1]
        leak = h2 @ w3t[0][np.arange(H) ^ 4]   # what an unmasked fragment row carries: another slot's weights, no bias
        flat = np.concatenate([out.ravel(), np.zeros(n)])
        flat[np.arange(rows) * n + n] = leak
        out = flat[:rows * n].reshape(rows, n)
    if len(layers[0]) == 2:
        out = out[:, 0]
    return dict(z1=z1, h1=h1, z2=z2, h2=h2, out=out)


def budget(layers, x) -> tuple:
    """The maxima over rows and units of sum_k |a_k b_k| + |bias| of layers 1, 2 and 3, operands
    rounded as the kernels round them (the layer-1 bias is the term b1 * 1)."""
    (w1, b1), (w2, b2), (w3, b3) = _wb(layers)
    x = np.asarray(x, f64)
    r = forward(layers, x)
    xa = np.abs(round_bf16(np.concatenate([x, np.ones((len(x), 1))], axis=1)))
    m1 = xa @ np.abs(round_bf16(np.concatenate([w1, b1[:, None]], axis=1))).T
    m2 = r["h1"] @ np.abs(round_bf16(w2)).T + np.abs(b2)
    m3 = r["h2"] @ np.abs(round_bf16(w3)).T + np.abs(b3)
    return float(m1.max()), float(m2.max()), float(m3.max())


# ---------------------------------------------------------------- training
def train_fixture(in_dim: int, out_dim: int, rows: int, seed: int = 0):
    """(layers, x, g, wide): the actor fixture and integer logit gradients g in -2..2 (one row in five
    all zero).  Through W3's +-257..263 entries dz2 and dz1 reach past 256 and round, ties included.
    The weight gradients are sums over rows, so they have a budget of their own (`grad_budget`); where
    the +-264 input column breaks it, the fixture without that column and without the +-257..263
    biases is returned (wide = False)."""
    g = np.random.default_rng([4242, in_dim, out_dim, rows, seed]).integers(-2, 3, (rows, out_dim)).astype(np.float32)
    g[::5] = 0
    for wide in (True, False):
        layers, x = fixture("actor", in_dim, out_dim, rows, seed, wide=wide)
        if max(grad_budget(layers, x, g).values()) < LIMIT:
            break
    return layers, x, g, wide


def grad_budget(layers, x, g) -> dict:
    """{name: max sum over rows of |term|} of the six gradients, and of the two dz sums ("dz2",
    "dz1"), from tests/train_ref.py's stage functions."""
    from tests import train_ref as tr
    (w1, b1), (w2, b2), (w3, b3) = _wb(layers)
    _, h1, _ = tr.stage_h1(w1, b1, x)
    _, h2, _ = tr.stage_h2(w2, b2, h1)
    _, dz2, m2 = tr.stage_dz2(w3, g, h2)
    _, dz1, m1 = tr.stage_dz1(w2, dz2, h1)
    _, mag = tr.weight_grads(x, g, h1, h2, dz2, dz1)
    out = {k: float(v.max()) for k, v in mag.items()}
    out.update(dz2=float(m2.max()), dz1=float(m1.max()))
    return out
