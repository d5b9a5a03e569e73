"""GPU: the per-agent critic (csrc/swarm_value.hip) through AgentValueMLP.

Reference: torch on the CPU in float64, an nn.Linear stack with torch's default init
(tests/value_ref.py), on observation-like inputs (positions and goal in +-10, velocities +-4,
relative vectors +-20, distances 0 .. 35).  One input set of 257 rows per in_dim; the smaller row
counts are its prefixes.  in_dim 15, 31 and 47 put in + 1 on a k-step edge, 16 one past it, 25 is
the single-drone observation, 37 the default width (the compile-time-width kernel instance).
Tolerances:
  f32   |v - v64| <= 1e-5 + 1e-5 |v64|  (the project's bound for the f32 critic).
  bf16  against the host emulation of the same bf16 arithmetic read back from the packed blob
        (bf16 operands, float64 sums, activations re-rounded): f32 accumulation order and rare bf16
        double-rounding flips only.  Measured maximum over the cases of
        test_bf16_value_vs_emulation_and_float64 on an MI355X: 6.612e-4 (in_dim 25, in one of rows
        1 .. 30: the size of one flipped bf16 activation, as in tests/test_gpu_critic.py; 1.3e-4 at
        in_dim 15, 1.5e-5 at in_dim 31, 1.3e-6 at in_dim 37); bound 4x that, 2.645e-3.  The second-grid-pass cases repeat their in_dim's figure
        bit for bit; the collector fragments of tests/test_gpu_value_rollout.py (env observations,
        other weights) measured 8.125e-4 and 1.542e-3 against the same bound.
  bf16  against the float64 truth: max|v - v64| <= 2 m, m the emulation's own maximum error
        against float64 over the in_dim's input set (computed here from the references, never
        from the kernel).
The second-grid-pass case mirrors the grid of swarm_value_forward (GRID below).
The bit-exact layer of the bf16 path (rounding rules, format, no tolerance) is tests/test_gpu_bf16_exact.py.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from tests import value_ref as vr

pytestmark = pytest.mark.gpu

BF16_EMU_MEASURED = 6.612e-4  # the figure the bound is set from
BF16_EMU_BOUND = 4 * BF16_EMU_MEASURED


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


_REF = {}


def ref(in_dim):
    """Per in_dim, computed once: weights, inputs, float64 truth."""
    if in_dim not in _REF:
        layers = vr.make_value(in_dim)
        x = vr.obs_like(max(vr.ROWS), in_dim, seed=in_dim)
        _REF[in_dim] = dict(layers=layers, x=x, v64=vr.truth64(layers, x))
    return _REF[in_dim]


_TOWERS = {}


def tower(dev, in_dim, precision):
    from swarm_marl_amd import AgentValueMLP
    key = (in_dim, precision)
    if key not in _TOWERS:
        _TOWERS[key] = AgentValueMLP(ref(in_dim)["layers"], device=dev, precision=precision)
    return _TOWERS[key]


def emu(r, c):
    if "emu" not in r:
        r["emu"] = vr.emulate_bf16_blob(c.packed_host, r["x"])
        r["m"] = np.abs(r["emu"] - r["v64"]).max()
    return r["emu"], r["m"]


def run_guarded(c, x: np.ndarray, dev) -> np.ndarray:
    """value() into the head of a longer buffer: nothing is written past `rows`."""
    rows = len(x)
    buf = torch.full((rows + 300,), -777.0, dtype=torch.float32, device=dev)
    out = c.value(torch.from_numpy(x).to(dev), out=buf[:rows])
    assert out.data_ptr() == buf.data_ptr()
    got = buf.cpu().numpy()
    assert np.all(got[rows:] == -777.0)
    return got[:rows]


@pytest.mark.parametrize("rows", vr.ROWS)
@pytest.mark.parametrize("in_dim", vr.IN_DIMS)
def test_f32_value_vs_float64(dev, in_dim, rows):
    r = ref(in_dim)
    got = run_guarded(tower(dev, in_dim, "f32"), r["x"][:rows], dev)
    v64 = r["v64"][:rows]
    err = np.abs(got - v64)
    print(f"f32 in={in_dim} rows={rows} max err {err.max():.3e} (bound use {np.max(err / (1e-5 + 1e-5 * np.abs(v64))):.3f})")
    assert np.all(err <= 1e-5 + 1e-5 * np.abs(v64)), err.max()


@pytest.mark.parametrize("rows", vr.ROWS)
@pytest.mark.parametrize("in_dim", vr.IN_DIMS)
def test_bf16_value_vs_emulation_and_float64(dev, in_dim, rows):
    r = ref(in_dim)
    c = tower(dev, in_dim, "bf16")
    e, m = emu(r, c)
    got = run_guarded(c, r["x"][:rows], dev)
    e_emu = np.abs(got - e[:rows]).max()
    e_64 = np.abs(got - r["v64"][:rows]).max()
    print(f"bf16 in={in_dim} rows={rows} vs emulation {e_emu:.3e}  vs float64 {e_64:.3e}  m {m:.3e}")
    assert e_emu <= BF16_EMU_BOUND, e_emu
    assert e_64 <= 2 * m, (e_64, m)


# rows of one workgroup's pass (8 waves x one 32-row tile) and workgroups per CU of a launch: the
# constants of swarm_value_forward's grid_for call (csrc/swarm_value.hip), mirrored here
GRID = (8 * 32, 1)


@pytest.mark.parametrize("in_dim", [37, 25])  # the compile-time-width instance and the runtime-width one
def test_second_grid_pass(dev, in_dim):
    """1.5 x the rows one pass of the grid holds, + 77: half of the waves run their tile loop twice,
    the last tile is ragged.  The input is the in_dim's 257-row set repeated on the device: 257 is
    coprime with the tile size, so every row of the set lands in every lane position.  Row r is held
    to the reference of row r mod 257 at the usual bounds, and is bitwise the value of row r mod 257
    in a 257-row launch: a value depends on its own row alone and not on its place in the tile or in
    the grid — an MFMA output column is a function of its own B column, the relu / pack and the
    layer-3 products and sums are per lane in a fixed order, and the two lane halves meet in one
    shuffle."""
    tile, per_cu = GRID
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    rows = cus * per_cu * tile * 3 // 2 + 77
    r = ref(in_dim)
    c = tower(dev, in_dim, "bf16")
    e, m = emu(r, c)
    small = run_guarded(c, r["x"], dev)
    x = torch.from_numpy(r["x"]).to(dev).repeat((rows + 256) // 257, 1)[:rows]
    assert x.is_contiguous() and x.shape == (rows, in_dim)
    buf = torch.full((rows + 300,), -777.0, dtype=torch.float32, device=dev)
    c.value(x, out=buf[:rows])
    got = buf.cpu().numpy()
    assert np.all(got[rows:] == -777.0)
    got = got[:rows]
    idx = np.arange(rows) % 257
    e_emu, e_64 = np.abs(got - e[idx]).max(), np.abs(got - r["v64"][idx]).max()
    print(f"bf16 in={in_dim} rows={rows} vs emulation {e_emu:.3e}  vs float64 {e_64:.3e}  m {m:.3e}")
    assert e_emu <= BF16_EMU_BOUND, e_emu
    assert e_64 <= 2 * m, (e_64, m)
    same = got.view(np.uint32) == small.view(np.uint32)[idx]
    assert same.all(), (int((~same).sum()), int(np.flatnonzero(~same)[0]))


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_rows_zero_is_a_noop(dev, precision):
    from swarm_marl_amd import _native as nat
    c = tower(dev, 25, precision)
    out = c.value(torch.empty((0, 25), dtype=torch.float32, device=dev))
    assert tuple(out.shape) == (0,)
    keep = torch.full((8,), 3.0, dtype=torch.float32, device=dev)
    obs = torch.zeros((8, 25), dtype=torch.float32, device=dev)
    assert c.lib.swarm_value_forward(ctypes.byref(c._c), obs.data_ptr(), 0, keep.data_ptr(), None) == nat.SWARM_OK
    torch.cuda.synchronize()
    assert torch.all(keep == 3.0)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_block_view_equals_flat_rows_and_repeats_bitwise(dev, precision):
    in_dim, t1, e, n = 37, 4, 13, 5  # 260 rows: nine bf16 row tiles, the last ragged
    r = ref(in_dim)
    c = tower(dev, in_dim, precision)
    x = torch.from_numpy(np.concatenate([r["x"], r["x"][:3]])).to(dev)
    flat = c.value(x)
    block = c.value(x.view(t1, e, n, in_dim))
    assert tuple(block.shape) == (t1, e, n)
    again = c.value(x)
    assert torch.equal(block.reshape(-1), flat) and torch.equal(again, flat)
    assert np.array_equal(flat.cpu().numpy()[:257], run_guarded(c, r["x"], dev))


def test_value_validates_its_arguments(dev):
    from swarm_marl_amd import AgentValueMLP
    c = tower(dev, 25, "f32")
    good = torch.zeros((4, 25), dtype=torch.float32, device=dev)
    for bad in (good.cpu(), good.double(), torch.zeros((4, 26), dtype=torch.float32, device=dev), good.t().contiguous().t()):
        with pytest.raises(ValueError):
            c.value(bad)
    with pytest.raises(ValueError):
        c.value(good, out=torch.zeros(5, dtype=torch.float32, device=dev))
    with pytest.raises(ValueError):
        AgentValueMLP(vr.make_value(48), device=dev)
    with pytest.raises(ValueError):
        AgentValueMLP(vr.make_value(25), device=dev, precision="f32x3")


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_load_layers_changes_the_values_in_place(dev, precision):
    from swarm_marl_amd import AgentValueMLP
    in_dim = 25
    r = ref(in_dim)
    c = AgentValueMLP(r["layers"], device=dev, precision=precision)
    x = torch.from_numpy(r["x"]).to(dev)
    before, ptr = c.value(x).clone(), c.weights.data_ptr()
    other = vr.make_value(in_dim, seed=9)
    c.load_layers(other)
    after = c.value(x)
    assert c.weights.data_ptr() == ptr
    assert (after - before).abs().max().item() > 1e-2
    fresh = AgentValueMLP(other, device=dev, precision=precision)
    assert torch.equal(after, fresh.value(x))
    c.load_layers(r["layers"])
    assert torch.equal(c.value(x), before)
    with pytest.raises(ValueError):
        c.load_layers(vr.make_value(in_dim + 1))
