"""CPU: the exact bf16 fixtures of tests/bf16_exact_ref.py are what they claim to be, the host packers
and the blob-reading emulations reproduce their reference bit for bit, and every modelled fault shows.

1. Fixture conditions, asserted at every shape tests/test_gpu_bf16_exact.py runs: every budget
   sum|terms| + |bias| below 2^24; each layer accumulated in f32 three ways (ascending from the bias,
   descending onto it, 16-term blocks) equals the float64 sum bit for bit; at least 100 elements of
   z2 in each rounding class (ties down and up, non-ties up and down; counted where z > 0, the rest is
   relu'd away), and of z1 where W1 and x reach +-3 (with +-1 inputs layer 1 stays below 512 but for a
   handful of elements, where only ties exist: there the two tie classes); 40 .. 60 % of h1 and of h2
   zero; at least 100 distinct outputs; off-grid values where the format has a rule to break.
2. swarm_policy_pack + emulate_bf16_kernel, swarm_value_pack / swarm_critic_pack + their
   emulate_bf16_blob, and direct_bf16 all equal `forward`: the blob-reading emulations that every
   Gaussian GPU test leans on are tied to a statement of the format made from the layers.
3. Every fault of bf16_exact_ref.FAULTS changes at least one output bit at every shape of its kind.
4. The training fixtures: the gradient budgets, tests/train_ref.py's stages against `forward`, and
   both tie directions in dz1.
"""
from __future__ import annotations

import numpy as np
import pytest

from tests import bf16_exact_ref as br
from tests import train_ref as tr

f32, f64 = np.float32, np.float64

CASES = ([("actor", i, o) for i, o in br.ACTOR_SHAPES]
         + [("tower", i, 1) for i in sorted(set(br.VALUE_IN_DIMS + br.CRITIC_IN_DIMS))])
IDS = [f"{k}-{i}to{o}" for k, i, o in CASES]

_FIX = {}


def fix(case):
    """Per case, computed once: layers, the 257 rows, the reference."""
    if case not in _FIX:
        layers, x = br.fixture(*case)
        _FIX[case] = dict(layers=layers, x=x, ref=br.forward(layers, x))
    return _FIX[case]


# ---------------------------------------------------------------- the reference's own parts
def test_rounding_modes_on_known_values():
    v = np.array([257.0, 259.0, -261.0, -263.0, 258.0, 513.0, 515.0, 1.0 - 2.0 ** -9, 1.0 + 2.0 ** -8, -1025.0, 0.0])
    assert np.array_equal(br.round_bf16(v), [256, 260, -260, -264, 258, 512, 516, 1, 1, -1024, 0])
    assert np.array_equal(br.round_bf16(v, "trunc"), [256, 258, -260, -262, 258, 512, 512, 1.0 - 2.0 ** -8, 1, -1024, 0])
    assert np.array_equal(br.round_bf16(v, "half_up"), [258, 260, -262, -264, 258, 512, 516, 1, 1.0 + 2.0 ** -7, -1024, 0])
    rng = np.random.default_rng(0)
    w = np.concatenate([rng.normal(0, 100, 4096), rng.integers(-70000, 70000, 4096).astype(f64)])
    assert np.array_equal(br.round_bf16(w), tr.bf16(w))  # train_ref's, written independently
    assert br.classes(v) == dict(tie_down=3, tie_up=3, up=1, down=2)  # 257 -261 1+2^-8 | 259 -263 1-2^-9 | 515 | 513 -1025
    assert np.array_equal(br.off_grid(v), [1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0])


# ---------------------------------------------------------------- 1. fixture conditions
def _f32_orders(a, w, bias):
    """[rows, units] f32 x 3: sum_k a[r, k] w[u, k] + bias[u] accumulated in f32, term by term, from
    the bias upwards in k; from the last k downwards, the bias last; and in 16-term blocks (each
    summed ascending, then the blocks' sums ascending, then the bias)."""
    rows, k_n = a.shape
    pad = -k_n % 16
    bias = np.zeros(len(w)) if bias is None else bias
    outs = [np.empty((rows, len(w)), f32) for _ in range(3)]
    for r0 in range(0, rows, 16):
        t64 = a[r0:r0 + 16, None, :] * w[None, :, :]
        t = t64.astype(f32)
        assert np.array_equal(t.astype(f64), t64)  # products of two bf16 values are exact in f32
        b = np.broadcast_to(bias.astype(f32)[None, :, None], t.shape[:2] + (1,))
        seq = np.concatenate([b, t], axis=2)
        outs[0][r0:r0 + 16] = np.cumsum(seq, axis=2, dtype=f32)[..., -1]
        outs[1][r0:r0 + 16] = np.cumsum(seq[..., ::-1], axis=2, dtype=f32)[..., -1]
        blk = np.concatenate([t, np.zeros(t.shape[:2] + (pad,), f32)], axis=2).reshape(t.shape[:2] + (-1, 16))
        sums = np.cumsum(blk, axis=3, dtype=f32)[..., -1]
        outs[2][r0:r0 + 16] = np.cumsum(np.concatenate([sums, b], axis=2), axis=2, dtype=f32)[..., -1]
    return outs


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture_conditions(case):
    kind, d, out = case
    c = fix(case)
    layers, x, r = c["layers"], c["x"], c["ref"]
    (w1, b1), (w2, b2), (w3, b3) = br._wb(layers)
    b = br.budget(layers, x)
    z1c, z2c = br.classes(np.maximum(r["z1"], 0)), br.classes(np.maximum(r["z2"], 0))
    zero = [float((r[k] == 0).mean()) for k in ("h1", "h2")]
    distinct = len(np.unique(r["out"]))
    print(f"{kind} {d}->{out}: log2 budgets {[round(float(np.log2(v)), 2) for v in b]}  z1 {z1c}  z2 {z2c}  "
          f"zero h1 {zero[0]:.3f} h2 {zero[1]:.3f}  {distinct} distinct outputs")
    assert max(b) < br.LIMIT, b
    # order independence, from the rounded operands
    xa = br.round_bf16(np.concatenate([x.astype(f64), np.ones((len(x), 1))], axis=1))
    wa = br.round_bf16(np.concatenate([w1, b1[:, None]], axis=1))
    outv = r["out"].reshape(len(x), -1)
    for a, w, bias, want in ((xa, wa, None, r["z1"]), (r["h1"], br.round_bf16(w2), b2, r["z2"]),
                             (r["h2"], br.round_bf16(w3), b3, outv)):
        for got in _f32_orders(a, w, bias):
            assert np.array_equal(got.astype(f64), want)
    # rounding classes, sparsity, variety
    assert min(z2c.values()) >= 100, z2c
    if d < 387:
        assert min(z1c.values()) >= 100, z1c
    else:
        assert min(z1c["tie_down"], z1c["tie_up"]) >= 100, z1c
    assert all(0.4 <= z <= 0.6 for z in zero), zero
    assert distinct >= 100, distinct
    # values bf16 does not hold: the inputs, [W1 | b1], W2, W3 (both tie directions, and non-ties), b2, b3
    assert br.off_grid(x[:, -1]).sum() >= 50 and (d == 1 or br.off_grid(x[:, :-1]).sum() >= 50)
    for name, w in (("w1", np.concatenate([w1, b1[:, None]], axis=1)), ("w2", w2), ("w3", w3)):
        wc = br.classes(w)
        assert min(wc.values()) >= (3 if name != "w3" or out > 1 else 1), (name, wc)
    assert br.off_grid(b1).any() and br.off_grid(b2).sum() >= 20 and br.off_grid(b3).any()
    # and all of it is float32
    assert all(a.dtype == f32 for l in layers for a in l[:2]) and x.dtype == f32


# ---------------------------------------------------------------- 2. packers and blob emulations
@pytest.fixture(scope="module")
def lib():
    from swarm_marl_amd import _native as nat
    return nat.load_library()


def _same(got, want, tag):
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{tag}: {len(bad)} elements differ, first at {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


@pytest.mark.parametrize("shape", br.ACTOR_SHAPES, ids=[f"{i}to{o}" for i, o in br.ACTOR_SHAPES])
def test_policy_pack_and_blob_emulation_equal_the_reference(lib, shape):
    from swarm_marl_amd import _native as nat
    from tests.test_policy_cpu import _pack, emulate_bf16_kernel
    c = fix(("actor",) + shape)
    buf = _pack(lib, c["layers"], nat.POLICY_BF16)
    _same(emulate_bf16_kernel(buf, c["x"], shape[1]), c["ref"]["out"], f"actor {shape}")


@pytest.mark.parametrize("d", br.VALUE_IN_DIMS)
def test_value_pack_blob_emulation_and_direct_equal_the_reference(lib, d):
    from swarm_marl_amd import _native as nat
    from tests import value_ref as vr
    c = fix(("tower", d, 1))
    buf = vr.pack(lib, c["layers"], nat.POLICY_BF16)
    _same(vr.emulate_bf16_blob(buf, c["x"]), c["ref"]["out"], f"value {d} blob")
    _same(vr.direct_bf16(c["layers"], c["x"]), c["ref"]["out"], f"value {d} direct")


@pytest.mark.parametrize("d", br.CRITIC_IN_DIMS)
def test_critic_pack_blob_emulation_and_direct_equal_the_reference(lib, d):
    from swarm_marl_amd import _native as nat
    from tests import critic_ref as cr
    c = fix(("tower", d, 1))
    buf = cr.pack(lib, c["layers"], nat.POLICY_BF16)
    _same(cr.emulate_bf16_blob(buf, c["x"]), c["ref"]["out"], f"critic {d} blob")
    _same(cr.direct_bf16(c["layers"], c["x"]), c["ref"]["out"], f"critic {d} direct")


# ---------------------------------------------------------------- 3. faults
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_fault_changes_an_output_bit(case):
    c = fix(case)
    want = c["ref"]["out"]
    faults = br.faults_of(case[0])
    assert len(faults) == len(br.FAULTS) - 1
    for fault in faults:
        got = br.forward(c["layers"], c["x"], fault)["out"]
        assert got.shape == want.shape
        n = int((got != want).sum())
        assert n > 0, f"{case}: fault {fault} changes nothing"
    with pytest.raises(ValueError):
        br.forward(c["layers"], c["x"], ("trunc", "b2"))


# ---------------------------------------------------------------- 4. the training fixtures
@pytest.mark.parametrize("rows", br.TRAIN_ROWS)
@pytest.mark.parametrize("shape", br.TRAIN_SHAPES, ids=[f"{i}to{o}" for i, o in br.TRAIN_SHAPES])
def test_training_fixture_budgets_and_stages(shape, rows):
    layers, x, g, wide = br.train_fixture(*shape, rows)
    gb = br.grad_budget(layers, x, g)
    print(f"train {shape} rows={rows} wide={wide}: log2 budgets { {k: round(float(np.log2(max(v, 1))), 2) for k, v in gb.items()} }")
    assert max(br.budget(layers, x)) < br.LIMIT and max(gb.values()) < br.LIMIT, gb
    r = br.forward(layers, x)
    stages, grads = tr.emulate(layers, x, g)
    assert np.array_equal(stages["h1"], r["h1"]) and np.array_equal(stages["h2"], r["h2"])
    for name in tr.NAMES:  # integers below 2^24: f32 holds every gradient
        assert np.array_equal(grads[name].astype(f32).astype(f64), grads[name]), name
        assert np.any(grads[name] != 0), name
    (w1, b1), (w2, b2), (w3, b3) = br._wb(layers)
    pre2, _, _ = tr.stage_dz2(w3, g, stages["h2"])
    pre1, _, _ = tr.stage_dz1(w2, stages["dz2"], stages["h1"])
    for name, dc in (("dz2", br.classes(pre2)), ("dz1", br.classes(pre1))):  # both round, ties in both directions
        print(f"  {name} {dc}")
        assert min(dc["tie_down"], dc["tie_up"]) >= (20 if rows == 257 else 1), (name, dc)
    assert not (g[::5] != 0).any() and (g != 0).any()
