"""Host references for the attention actor (CPU and GPU tests), independent of the kernels and of
torch: a NumPy float64 forward written from the formulas in include/swarm_mi355x.h (unfolded), the
float64 folds, and the bf16 path's emulation — the folded forward with bf16 round-to-nearest-even
at the rounding points DESIGN.md §3.3 lists.

* `make_attn(k, ms, out)`: uniform(-1, 1) / sqrt(fan_in) weights as in tests/policy_ref.py, seeded
  per (k, ms, out); small non-zero biases everywhere (bk, bv and bout included);
* `obs_set(k, ms)`: 257 rows of uniform(-3, 3) observations, seeded per (k, ms).
"""
from __future__ import annotations

import numpy as np

H = 256
EM = 32
ROWS = 257
# (K, Ms, out): the default; one neighbour (softmax over one slot); no obstacles and the narrowest
# logits; every maximum (the 64-wide layer-1 K is full to column 61); a small odd-ish mix
SHAPES = ((3, 4, 6), (1, 4, 6), (6, 0, 2), (16, 5, 12), (2, 1, 6))
# the logits widths SHAPES leaves out (out = 4, 8, 10: ad = 2, 4, 5; at ad = 4 the log-std half sits
# wholly in the other lane half, at ad = 5 it straddles it) with sensed_obstacles = 2 and 3.  Kept
# apart so that SHAPES and the measured table of DESIGN.md §5.4 keep their meaning.
MORE_SHAPES = ((5, 2, 4), (8, 3, 8), (11, 5, 10))
ROW_COUNTS = (1, 33, 257)  # a lone row, one past a 32-row tile, one past a 256-row workgroup

NAMES = ("neighbor_embed.0.weight", "neighbor_embed.0.bias", "own_embed.0.weight", "own_embed.0.bias",
         "attn_block.attn.in_proj_weight", "attn_block.attn.in_proj_bias",
         "attn_block.attn.out_proj.weight", "attn_block.attn.out_proj.bias")
_SHAPES = ((EM, 4), (EM,), (EM, 9), (EM,), (3 * EM, EM), (3 * EM,), (EM, EM), (EM,))


def make_attn(k: int, ms: int, out: int, *, log_std_scale: float | None = None, in_proj_scale: float = 1.0,
              seed_offset: int = 0, q_scale: float = 1.0):
    """(params, layers): params maps the reference's names to float32 arrays, layers = [(w, b)] x 3 of
    the trunk (41 + 4 ms -> 256 -> 256 -> out).  Weights uniform(-1, 1) / sqrt(fan_in); biases
    uniform(-1, 1) / sqrt(fan_in) of their layer (small, non-zero).  `log_std_scale` as in
    tests/policy_ref.py make_actor; `in_proj_scale` multiplies in_proj_weight (the peaked fixture);
    `q_scale` multiplies the query third of in_proj_weight and in_proj_bias only (rows [:32]): the
    scores grow, Wv and with it the folded F = W1c Wout Wv keep their size (the saturated fixture)."""
    rng = np.random.default_rng(100000 * k + 1000 * ms + out + 7919 * seed_offset)
    params = {}
    for (wn, ws), (bn, bs) in zip(zip(NAMES[0::2], _SHAPES[0::2]), zip(NAMES[1::2], _SHAPES[1::2])):
        fan = np.float32(np.sqrt(ws[-1]))
        params[wn] = rng.uniform(-1, 1, ws).astype(np.float32) / fan
        params[bn] = rng.uniform(-1, 1, bs).astype(np.float32) / fan
    params["attn_block.attn.in_proj_weight"] = (params["attn_block.attn.in_proj_weight"]
                                                * np.float32(in_proj_scale)).astype(np.float32)
    if q_scale != 1.0:
        params["attn_block.attn.in_proj_weight"][:EM] *= np.float32(q_scale)
        params["attn_block.attn.in_proj_bias"][:EM] *= np.float32(q_scale)
    in1 = 9 + EM + 4 * ms
    layers = []
    for shape in ((H, in1), (H, H), (out, H)):
        fan = np.float32(np.sqrt(shape[-1]))
        layers.append((rng.uniform(-1, 1, shape).astype(np.float32) / fan,
                       rng.uniform(-1, 1, shape[:1]).astype(np.float32) / fan))
    if log_std_scale is not None:
        ad = out // 2
        w3, b3 = layers[2]
        w3[ad:] *= np.float32(log_std_scale)
        b3[ad:] = rng.uniform(-1.0, -0.5, out - ad).astype(np.float32)
    return params, layers


def obs_set(k: int, ms: int, rows: int = ROWS) -> np.ndarray:
    d = 9 + 4 * k + 4 * ms
    return np.random.default_rng(4242 + 100 * k + ms).uniform(-3, 3, (rows, d)).astype(np.float32)


def _f64(params):
    p = {n: params[n].astype(np.float64) for n in NAMES}
    wi, bi = p["attn_block.attn.in_proj_weight"], p["attn_block.attn.in_proj_bias"]
    return dict(wnb=p[NAMES[0]], bnb=p[NAMES[1]], wown=p[NAMES[2]], bown=p[NAMES[3]],
                wq=wi[:EM], wk=wi[EM:2 * EM], wv=wi[2 * EM:], bq=bi[:EM], bk=bi[EM:2 * EM], bv=bi[2 * EM:],
                wout=p[NAMES[6]], bout=p[NAMES[7]])


def _split(x: np.ndarray, k: int):
    x = x.astype(np.float64)
    return x[:, :9], x[:, 9:9 + 4 * k].reshape(len(x), k, 4), x[:, 9 + 4 * k:]


def forward64(params, layers, k: int, x: np.ndarray, *, details: bool = False):
    """logits [rows, out] in float64, the unfolded formulas.  details=True also returns the raw scores
    q . k_j / sqrt(32) [rows, k] and the attention weights [rows, k]."""
    p = _f64(params)
    own, nb, obst = _split(x, k)
    o = np.maximum(own @ p["wown"].T + p["bown"], 0)                      # [R, 32]
    e = np.maximum(nb @ p["wnb"].T + p["bnb"], 0)                         # [R, K, 32]
    q = o @ p["wq"].T + p["bq"]
    kk = e @ p["wk"].T + p["bk"]
    v = e @ p["wv"].T + p["bv"]
    score = np.einsum("ri,rji->rj", q, kk) / np.sqrt(float(EM))
    a = np.exp(score - score.max(axis=1, keepdims=True))
    a /= a.sum(axis=1, keepdims=True)
    c = np.einsum("rj,rji->ri", a, v) @ p["wout"].T + p["bout"]
    h = np.concatenate([own, c, obst], axis=1)
    for i, (w, b) in enumerate(layers):
        h = h @ w.T.astype(np.float64) + b.astype(np.float64)
        if i < 2:
            h = np.maximum(h, 0)
    return (h, score, a) if details else h


def folds64(params, layers):
    """The two folds in float64: A [32,32], c0 [32] (score_j = (A o + c0) . e_j + j-constant terms) and
    F [256,32], d [256] (W1[:, 9:41] c = F s + d with s = sum_j a_j e_j)."""
    p = _f64(params)
    scale = 1.0 / np.sqrt(float(EM))
    w1c = layers[0][0][:, 9:9 + EM].astype(np.float64)
    return dict(A=p["wk"].T @ p["wq"] * scale, c0=p["wk"].T @ p["bq"] * scale,
                F=w1c @ p["wout"] @ p["wv"], d=w1c @ (p["wout"] @ p["bv"] + p["bout"]))


def bf16(x: np.ndarray) -> np.ndarray:
    """float64 -> float32 -> bf16 (round to nearest even) -> float64."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16) << np.uint64(16)
    return u.astype(np.uint32).view(np.float32).astype(np.float64).reshape(np.shape(x))


def f32(x: np.ndarray) -> np.ndarray:
    return np.asarray(x, np.float32).astype(np.float64)


def s_of_col(kcol: int) -> int:
    """The s component carried by column kcol < 32 of the bf16 blob's layer-1 fragments."""
    return 16 * ((kcol >> 3) & 1) + 8 * (kcol >> 4) + (kcol & 7)


def folded_w1(params, layers, ms: int) -> np.ndarray:
    """[256, 64] float64, unrounded: the folded first layer in the blob's column order
    [F (columns permuted by s_of_col) | W1 own | W1 obst | b1 + d | 0]."""
    f = folds64(params, layers)
    w1, b1 = layers[0][0].astype(np.float64), layers[0][1].astype(np.float64)
    out = np.zeros((H, 64))
    out[:, :32] = f["F"][:, [s_of_col(c) for c in range(32)]]
    out[:, 32:41] = w1[:, :9]
    out[:, 41:41 + 4 * ms] = w1[:, 9 + EM:]
    out[:, 41 + 4 * ms] = b1 + f["d"]
    return out


def forward_bf16_emu(params, layers, k: int, ms: int, x: np.ndarray) -> np.ndarray:
    """The bf16 path in float64 arithmetic with its roundings: the front end on the
    folded scores with A, c0 rounded to f32; then bf16 at s, own, obst, the folded layer-1 weights
    (F, the own / obstacle columns, b1 + d), h1, W2, h2, W3; b2, b3 stay f32."""
    p = _f64(params)
    f = folds64(params, layers)
    own, nb, obst = _split(x, k)
    o = np.maximum(own @ p["wown"].T + p["bown"], 0)
    e = np.maximum(nb @ p["wnb"].T + p["bnb"], 0)
    t = o @ f32(f["A"]).T + f32(f["c0"])
    score = np.einsum("ri,rji->rj", t, e)
    a = np.exp(score - score.max(axis=1, keepdims=True))
    s = np.einsum("rj,rji->ri", a, e) / a.sum(axis=1, keepdims=True)
    w1 = bf16(folded_w1(params, layers, ms))
    xin = np.zeros((len(x), 64))
    xin[:, :32] = bf16(s)[:, [s_of_col(c) for c in range(32)]]
    xin[:, 32:41] = bf16(own)
    xin[:, 41:41 + 4 * ms] = bf16(obst)
    xin[:, 41 + 4 * ms] = 1.0
    h1 = bf16(np.maximum(xin @ w1.T, 0))
    h2 = bf16(np.maximum(h1 @ bf16(layers[1][0]).T + layers[1][1].astype(np.float64), 0))
    return h2 @ bf16(layers[2][0]).T + layers[2][1].astype(np.float64)


# ---------------------------------------------------------------- the saturated softmax fixture
SAT_SHAPE = (16, 5, 12)
SAT_Q_SCALE = 144.0
SAT_ROWS = 97          # one full 64-row group and a 33-row group
SAT_SPAN = 104.0       # max score - min score: f32 exp(-104) is 0
SAT_GAP = 30.0         # top score - second score: every other weight is below exp(-30) < 1e-13


def make_saturated():
    """(params, layers) of the saturated fixture: SAT_SHAPE, seed_offset 1, the query scaled by 144."""
    return make_attn(*SAT_SHAPE, seed_offset=1, q_scale=SAT_Q_SCALE)


def saturated_rows(params, layers, pool: int = 8192):
    """(x, score): the first SAT_ROWS rows of obs_set(K, Ms, rows=pool) whose float64 scores span more
    than SAT_SPAN with the top one more than SAT_GAP above the second, and those scores.  Fewer than
    SAT_ROWS rows come back when the pool holds fewer (the caller asserts the count)."""
    k, ms, _ = SAT_SHAPE
    x = obs_set(k, ms, rows=pool)
    _, score, _ = forward64(params, layers, k, x, details=True)
    srt = np.sort(score, axis=1)
    keep = (srt[:, -1] - srt[:, 0] > SAT_SPAN) & (srt[:, -1] - srt[:, -2] > SAT_GAP)
    return x[keep][:SAT_ROWS], score[keep][:SAT_ROWS]


def reorder_slots(x: np.ndarray, k: int, order: np.ndarray) -> np.ndarray:
    """x with row r's neighbour slot j replaced by its slot order[r, j]; own and obstacle columns stay."""
    out = x.copy()
    nb = x[:, 9:9 + 4 * k].reshape(len(x), k, 4)
    out[:, 9:9 + 4 * k] = np.take_along_axis(nb, order[:, :, None], axis=1).reshape(len(x), 4 * k)
    return out


def saturated_variants(params, layers, pool: int = 8192):
    """{"drawn", "ascending", "descending"} -> observations [<= SAT_ROWS, D]: the selected rows as drawn,
    and with the slots of every row permuted into ascending / descending float64 score."""
    x, score = saturated_rows(params, layers, pool)
    asc = np.argsort(score, axis=1, kind="stable")
    return {"drawn": x, "ascending": reorder_slots(x, SAT_SHAPE[0], asc),
            "descending": reorder_slots(x, SAT_SHAPE[0], asc[:, ::-1])}
