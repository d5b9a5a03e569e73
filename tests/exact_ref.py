"""Host references that hold the f32 and f32x3 actor kernels (csrc/swarm_policy.hip) to bounds taken
from their arithmetic (CPU and GPU tests), written from the kernels' definitions and independent of
them:

* `scale64(layers, x)`: the float64 magnitude S [rows, out] that a logit's rounding errors scale
  with: a1 = |W1||x| + |b1|, a2 = |W2| a1 + |b2|, S = |W3| a2 + |b3| (no relu);
* `forward_f32acc(layers, x, order)`: the f32 graph as one f32 MFMA chain computes it: every
  product-and-add fused (the f32 x f32 product is exact in float64; product + accumulator is rounded
  to f32), layer 1 from zero with the bias as the product b1 * 1.0 at position k = in (the kernel's
  bias column), layers 2 and 3 from the bias, k ascending or descending;
* `x3_f32acc(buf, x, out, order, fault)`: the f32x3 arithmetic from the packed blob (hi blob, lo
  blob): exact f16 x f16 products, the hi*hi chain and the cross-term chain (hi*lo and lo*hi, scaled
  by 2^11) each accumulated in f32 in the given k order, layer output c + x * 2^-11 in f32, relu,
  split again.  `fault` breaks it in one of the ways of FAULTS;
* `tower_f32acc(layers, x, order)` / `tower_bound`: the same construction for the f32 value towers
  (critic_mlp_f32: unfused products, a layer's bias added last);
* `case(shape, regime)`: weights and 257 input rows of the regimes R0..R4;
* `f32_bound` / `x3_bound`: for a case, u = 2^-24, c = max over elements and both orders of
  |model_f32acc - model64| / (u S) and the bound 4 c u S on |kernel - model64|, model64 the float64
  forward (f32) or tests/test_policy_cpu.py emulate_x3_kernel (f32x3, float64 sums).  Nothing in it
  comes from a kernel.  The factor 4 covers what no model here knows: the order of the sum inside
  one MFMA k-step (16 deep for f16, 4 for f32) and the interleaving of the chains; the correct
  models use at most 0.25 of the bound by construction.

(product + accumulator is formed in float64 and then rounded to f32: two roundings, which differ
from the fused one only when the float64 sum lands within 2^-53 of an f32 tie.)
"""
from __future__ import annotations

import numpy as np

from tests import policy_ref as pr
from tests import value_ref as vr

U = 2.0 ** -24
ORDERS = ("ascending", "descending")
SHAPES = ((37, 6), (47, 12), (16, 4))
REGIMES = ("R0", "R1", "R2", "R3", "R4")
PREFIXES = (1, 33, 257)
FACTOR = 4.0
# (kind, argument): lo of W dropped in layer i; lo of the layer input dropped in layer i; lo dropped
# in one 32-unit out block of W2; lo stored unscaled (f16(v - hi), cross terms added unscaled); the
# 2^-11 factor doubled in layer i
FAULTS = (tuple(("w_lo", i) for i in (1, 2, 3)) + tuple(("x_lo", i) for i in (1, 2, 3))
          + (("w2_lo_block", 0), ("w2_lo_block", 5), ("unscaled", 0)) + tuple(("scale_x2", i) for i in (1, 2, 3)))

f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------- the cases
def case(shape, regime: str):
    """(layers, x [257, in]) of a regime, all inside the f32x3 domain:
    R0  make_actor / obs_set (policy_ref);
    R1  observation-like inputs (value_ref.obs_like: positions +-10, velocities +-4, relative vectors
        +-20, distances to 35);
    R2  W1 * 2^-10 and obs * 2^10, b1 as it is (the bias column carries 1.0): the same function, the
        float64 logits equal R0's bit for bit; W1 sits at the bottom of the f16 normal range (its
        smaller entries are f16 subnormals), |obs| reaches 3072;
    R3  W3 and b3 * 64: logits to about +-45;
    R4  obs * 2^-12: the layer-1 input's lo pieces are f16 subnormals even scaled by 2^11."""
    layers = pr.make_actor(*shape)
    x = pr.obs_set(shape[0])
    (w1, b1, _), l2, (w3, b3, _) = layers
    if regime == "R1":
        x = vr.obs_like(pr.ROWS, shape[0], seed=shape[0])
    elif regime == "R2":
        layers = [(w1 * f32(2.0 ** -10), b1, True), l2, (w3, b3, False)]
        x = x * f32(2.0 ** 10)
    elif regime == "R3":
        layers = [(w1, b1, True), l2, (w3 * f32(64), b3 * f32(64), False)]
    elif regime == "R4":
        x = x * f32(2.0 ** -12)
    elif regime != "R0":
        raise ValueError(regime)
    return layers, np.ascontiguousarray(x, f32)


def scale64(layers, x: np.ndarray) -> np.ndarray:
    a = np.abs(x.astype(f64))
    for w, b, _ in layers:
        a = a @ np.abs(w.astype(f64)).T + np.abs(b.astype(f64))
    return a


# ---------------------------------------------------------------- f32 chains
def _fma(acc: np.ndarray, prod: np.ndarray) -> np.ndarray:
    return (prod + acc.astype(f64)).astype(f32)


def _ks(n: int, order: str):
    if order not in ORDERS:
        raise ValueError(order)
    return range(n) if order == "ascending" else range(n - 1, -1, -1)


def forward_f32acc(layers, x: np.ndarray, order: str) -> np.ndarray:
    (w1, b1, _), (w2, b2, _), (w3, b3, _) = layers
    rows, d = x.shape
    xa = np.concatenate([x.astype(f32), np.ones((rows, 1), f32)], axis=1).astype(f64)   # the bias column
    wa = np.concatenate([w1, b1[:, None]], axis=1).astype(f64)
    acc = np.zeros((rows, w1.shape[0]), f32)
    for k in _ks(d + 1, order):
        acc = _fma(acc, np.multiply.outer(xa[:, k], wa[:, k]))
    for w, b, relu in ((w2, b2, True), (w3, b3, False)):
        h = np.maximum(acc, f32(0)).astype(f64)
        w = w.astype(f64)
        acc = np.broadcast_to(b.astype(f32), (rows, w.shape[0]))
        for k in _ks(h.shape[1], order):
            acc = _fma(acc, np.multiply.outer(h[:, k], w[:, k]))
    return acc


def tower_f32acc(layers, x: np.ndarray, order: str) -> np.ndarray:
    """The f32 value towers (csrc/swarm_critic.hip critic_mlp_f32, compiled with fp contract off; the
    per-agent tower launches the same kernel): every product rounded to f32, then added to the f32
    accumulator; a layer's sum starts at zero and its bias is added last.  `layers` = [(w, b)] x 3 of an
    in -> 256 -> 256 -> 1 tower; [rows] f32."""
    act = x.astype(f32)
    for i, (w, b) in enumerate(layers):
        w = w.astype(f32)
        acc = np.zeros((act.shape[0], w.shape[0]), f32)
        for k in _ks(act.shape[1], order):
            acc = acc + np.multiply.outer(act[:, k], w[:, k])  # f32 product, f32 sum: two roundings
        acc = acc + np.reshape(b, -1).astype(f32)
        act = np.maximum(acc, f32(0)) if i < 2 else acc
    assert act.dtype == f32
    return act[:, 0]


def tower_bound(layers, x: np.ndarray) -> dict:
    from tests import critic_ref as cr
    s = scale64([(w, np.reshape(b, -1), None) for w, b in layers], x)[:, 0]
    return _bound(cr.truth64(layers, x), [tower_f32acc(layers, x, o) for o in ORDERS], s)


# ---------------------------------------------------------------- the f32x3 model
# v_mfma_f32_32x32x16 maps (tests/test_policy_cpu.py): C[row (i & 3) + 8 (i >> 2) + 4 h] in register i of
# lane half h; chained as the next B operand, element j of half h in k-step ks is register 8 (ks & 1) + j
# of out block ks >> 1.  _CHAIN[k], k = (ks, h, j) flattened, is the hidden unit at position k.
_REG_ROW = np.array([[(i & 3) + 8 * (i >> 2) + 4 * h for i in range(16)] for h in range(2)])
_CHAIN = np.array([(ks >> 1) * 32 + _REG_ROW[h, 8 * (ks & 1) + j]
                   for ks in range(16) for h in range(2) for j in range(8)])
LO_SCALE = f32(2048)


def _blob(buf: np.ndarray, out: int):
    """Per part (hi, lo): W1 [48, 256], W2 [256, 256], W3 [256, out] as float64, first index the k
    position (ks, h, j) of the fragment order; b2, b3 (f32, hi part only)."""
    total = len(buf) // 2
    parts = []
    for part in range(2):
        b = buf[part * total:(part + 1) * total]
        o1, o2 = 8 * 3 * 1024, 8 * 19 * 1024
        o3 = o2 + 16 * 2 * out * 16
        w1 = b[:o1].view(np.float16).astype(f64).reshape(8, 3, 2, 32, 8)        # ob, ks, h, m, j
        w2 = b[o1:o2].view(np.float16).astype(f64).reshape(8, 16, 2, 32, 8)
        w3 = b[o2:o3].view(np.float16).astype(f64).reshape(16, 2, out, 8)       # ks, h, m, j
        parts.append((w1.transpose(1, 2, 4, 0, 3).reshape(48, 256), w2.transpose(1, 2, 4, 0, 3).reshape(256, 256),
                      w3.transpose(0, 1, 3, 2).reshape(256, out)))
        if part == 0:
            b2, b3 = b[o3:o3 + 1024].view(f32).copy(), b[o3 + 1024:o3 + 1024 + 4 * out].view(f32).copy()
    return parts[0], parts[1], b2, b3


def _split(v: np.ndarray, scaled: bool = True):
    """f32 -> (hi, lo) as the kernel splits its operands: hi = f16(v), lo = f16((v - hi) * 2^11), both
    round to nearest even, v - hi exact in f32; `scaled=False` is the fault f16(v - hi)."""
    v = np.asarray(v, f32)
    hi = v.astype(np.float16)
    rest = v - hi.astype(f32)
    lo = (rest * LO_SCALE if scaled else rest).astype(np.float16)
    return hi.astype(f64), lo.astype(f64)


def _x3_layer(wh, wl, xh, xl, bias, order: str, lo_inv) -> np.ndarray:
    """[rows, units] f32.  wh / wl [K, units], xh / xl [rows, K]; the hi*hi chain starts from the
    bias, the cross chain from zero; per 16-deep k-step the cross chain takes the step's hi*lo
    products and then its lo*hi products (descending: the whole sequence reversed)."""
    rows, k_n = xh.shape
    c = np.broadcast_to(f32(0) if bias is None else bias.astype(f32), (rows, wh.shape[1])).astype(f32)
    for k in _ks(k_n, order):
        c = _fma(c, np.multiply.outer(xh[:, k], wh[k]))
    seq = [(a, k) for s in range(0, k_n, 16) for a in (0, 1) for k in range(s, s + 16)]
    x = np.zeros_like(c)
    for a, k in (seq if order == "ascending" else seq[::-1]):
        x = _fma(x, np.multiply.outer(xl[:, k], wh[k]) if a == 0 else np.multiply.outer(xh[:, k], wl[k]))
    return (c.astype(f64) + (x * f32(lo_inv)).astype(f64)).astype(f32)


def x3_f32acc(buf: np.ndarray, x: np.ndarray, out: int, order: str, fault=None) -> np.ndarray:
    kind, arg = fault if fault is not None else (None, 0)
    if fault is not None and fault not in FAULTS:
        raise ValueError(fault)
    whs, wls, b2, b3 = _blob(buf, out)
    wls = [w.copy() for w in wls]
    scaled = kind != "unscaled"
    inv = [1.0 if not scaled else 2.0 ** -11] * 3
    if kind == "w_lo":
        wls[arg - 1][:] = 0
    elif kind == "w2_lo_block":
        wls[1][:, 32 * arg:32 * arg + 32] = 0
    elif kind == "unscaled":  # from the blob's scaled lo: f16(lo * 2^-11), the bits an unscaled store keeps
        wls = [(w * 2.0 ** -11).astype(np.float16).astype(f64) for w in wls]
    elif kind == "scale_x2":
        inv[arg - 1] *= 2
    rows, d = x.shape
    act = np.zeros((rows, 48), f32)
    act[:, :d] = x
    act[:, d] = 1.0
    for i, bias in enumerate((None, b2, b3)):
        ah, al = _split(act, scaled)
        if kind == "x_lo" and arg == i + 1:
            al[:] = 0
        act = _x3_layer(whs[i], wls[i], ah, al, bias, order, inv[i])
        if i < 2:
            act = np.maximum(act, f32(0))[:, _CHAIN]
    return act


# ---------------------------------------------------------------- the bound
def _bound(model64: np.ndarray, models, s: np.ndarray) -> dict:
    c = max(float(np.max(np.abs(m.astype(f64) - model64) / (U * s))) for m in models)
    return dict(model64=model64, S=s, c=c, bound=FACTOR * c * U * s, models=list(models))


def f32_bound(layers, x: np.ndarray) -> dict:
    return _bound(pr.forward64(layers, x), [forward_f32acc(layers, x, o) for o in ORDERS], scale64(layers, x))


def x3_bound(buf: np.ndarray, layers, x: np.ndarray) -> dict:
    from tests.test_policy_cpu import emulate_x3_kernel
    out = layers[2][0].shape[0]
    return _bound(emulate_x3_kernel(buf, x, out), [x3_f32acc(buf, x, out, o) for o in ORDERS], scale64(layers, x))


def share(got: np.ndarray, b: dict) -> float:
    """The largest share of the bound that `got` uses."""
    return float(np.max(np.abs(got.astype(f64) - b["model64"]) / b["bound"]))


def old_share(got: np.ndarray, l64: np.ndarray) -> float:
    """The largest share of the suite's f32 logit bound, 1e-4 + 1e-5 |float64 forward|."""
    return float(np.max(np.abs(got.astype(f64) - l64) / (1e-4 + 1e-5 * np.abs(l64))))
