"""GPU: the centralized critic (csrc/swarm_critic.hip) through CriticMLP.

Reference: torch on the CPU in float64, an nn.Linear stack with torch's default init
(tests/critic_ref.py), on inputs laid out like a global state (positions and goal in +-10,
velocities in +-2).  One input set of 257 rows per in_dim; the smaller row counts are its prefixes.
Tolerances:
  f32   |v - v64| <= 1e-5 + 1e-5 |v64|  (torch's own f32 forward uses at most 0.07 of it here).
  bf16  against the host emulation of the same bf16 arithmetic read back from the packed blob
        (bf16 operands, float64 sums, activations re-rounded): f32 accumulation order and rare bf16
        double-rounding flips only.  Measured maximum over the first five in_dims on an MI355X:
        2.413e-4 (one flipped bf16 activation at rows = 257; 1.3e-7 where none flips); bound 4x that,
        9.652e-4, kept as it was when the in_dims 1 .. 128 and the second-grid-pass cases were
        added: over every case below the maximum is now 3.406e-4 (in_dim 99, rows = 257).
  bf16  against the float64 truth: max|v - v64| <= 2 m, m the emulation's own maximum error
        against float64 over the in_dim's input set (computed here from the references, never
        from the kernel; 0.004-0.009 on |v| up to 2).
The second-grid-pass cases mirror the per-CU grid caps of swarm_critic_forward (GRID below).
The bit-exact layer of the bf16 path (rounding rules, format, no tolerance) is tests/test_gpu_bf16_exact.py.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from tests import critic_ref as cr

pytestmark = pytest.mark.gpu

ROWS = (1, 31, 33, 257)
BF16_EMU_MEASURED = 2.413e-4  # the figure the bound was set from (3.406e-4 over every in_dim since)
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
        layers = cr.make_critic(in_dim)
        x = cr.global_state_like(max(ROWS), in_dim, seed=in_dim)
        _REF[in_dim] = dict(layers=layers, x=x, v64=cr.truth64(layers, x))
    return _REF[in_dim]


_CRITICS = {}


def critic(dev, in_dim, precision):
    from swarm_marl_amd import CriticMLP
    key = (in_dim, precision)
    if key not in _CRITICS:
        _CRITICS[key] = CriticMLP(ref(in_dim)["layers"], device=dev, precision=precision)
    return _CRITICS[key]


def run_guarded(c, x: np.ndarray, dev) -> np.ndarray:
    """value() into the head of a longer buffer: nothing is written past `rows`."""
    rows = len(x)
    buf = torch.full((rows + 300,), -777.0, dtype=torch.float32, device=dev)
    out = c.value(torch.from_numpy(x).to(dev), out=buf[:rows])
    assert out.data_ptr() == buf.data_ptr()
    got = buf.cpu().numpy()
    assert np.all(got[rows:] == -777.0)
    return got[:rows]


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("in_dim", cr.IN_DIMS)
def test_f32_value_vs_float64(dev, in_dim, rows):
    r = ref(in_dim)
    got = run_guarded(critic(dev, in_dim, "f32"), r["x"][:rows], dev)
    v64 = r["v64"][:rows]
    err = np.abs(got - v64)
    print(f"f32 in={in_dim} rows={rows} max err {err.max():.3e} (bound use {np.max(err / (1e-5 + 1e-5 * np.abs(v64))):.3f})")
    assert np.all(err <= 1e-5 + 1e-5 * np.abs(v64)), err.max()


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("in_dim", cr.IN_DIMS)
def test_bf16_value_vs_emulation_and_float64(dev, in_dim, rows):
    r = ref(in_dim)
    c = critic(dev, in_dim, "bf16")
    if "emu" not in r:
        r["emu"] = cr.emulate_bf16_blob(c.packed_host, r["x"])
        r["m"] = np.abs(r["emu"] - r["v64"]).max()
    got = run_guarded(c, r["x"][:rows], dev)
    e_emu = np.abs(got - r["emu"][:rows]).max()
    e_64 = np.abs(got - r["v64"][:rows]).max()
    print(f"bf16 in={in_dim} rows={rows} vs emulation {e_emu:.3e}  vs float64 {e_64:.3e}  m {r['m']:.3e}")
    assert e_emu <= BF16_EMU_BOUND, e_emu
    assert e_64 <= 2 * r["m"], (e_64, r["m"])


# rows of one workgroup's tile and workgroups per CU of a launch: the constants of swarm_critic_forward's
# two grid_for calls (csrc/swarm_critic.hip), mirrored here
GRID = {"bf16": (128, 16), "f32": (32, 32)}


@pytest.mark.parametrize("in_dim", [21, 51])  # nc1 = 1 and 2: the tile's last chunk in either LDS buffer
@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_second_grid_pass(dev, precision, in_dim):
    """1.5 x the rows one pass of the capped grid holds, + 77: half of the workgroups run their
    tile loop twice (in the bf16 kernel the second pass stages chunk 0 into LDS buffer 0 right after
    the previous tile's last barrier), the last tile is ragged.  The input is the in_dim's 257-row
    set repeated on the device: 257 is coprime with both tile sizes, so every row of the set lands
    in every lane position.  Row r is held to the reference of row r mod 257 at the usual bounds,
    and is bitwise the value of row r mod 257 in a 257-row launch: a value depends on its own row
    alone and not on its place in the tile — in the f32 kernel every thread runs one operation
    sequence for each of its 32 rows (f32_block, the layer-3 sum of 32 units and three shuffles); in
    the bf16 kernel an MFMA output column is a function of its own B column, the relu / pack and the
    layer-3 products and sums are per lane in a fixed order, and the two lane halves meet in one
    shuffle."""
    tile, per_cu = GRID[precision]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    first_pass = cus * per_cu * tile
    rows = first_pass * 3 // 2 + 77
    r = ref(in_dim)
    c = critic(dev, in_dim, precision)
    small = run_guarded(c, r["x"], dev)
    x = torch.from_numpy(r["x"]).to(dev).repeat((rows + 256) // 257, 1)[:rows]
    assert x.is_contiguous() and x.shape == (rows, in_dim)
    buf = torch.full((rows + 300,), -777.0, dtype=torch.float32, device=dev)
    c.value(x, out=buf[:rows])
    got = buf.cpu().numpy()
    assert np.all(got[rows:] == -777.0)
    got = got[:rows]
    idx = np.arange(rows) % 257
    v64 = r["v64"][idx]
    if precision == "f32":
        err = np.abs(got - v64)
        print(f"f32 in={in_dim} rows={rows} max err {err.max():.3e}")
        assert np.all(err <= 1e-5 + 1e-5 * np.abs(v64)), err.max()
    else:
        if "emu" not in r:
            r["emu"] = cr.emulate_bf16_blob(c.packed_host, r["x"])
            r["m"] = np.abs(r["emu"] - r["v64"]).max()
        e_emu, e_64 = np.abs(got - r["emu"][idx]).max(), np.abs(got - v64).max()
        print(f"bf16 in={in_dim} rows={rows} vs emulation {e_emu:.3e}  vs float64 {e_64:.3e}  m {r['m']:.3e}")
        assert e_emu <= BF16_EMU_BOUND, e_emu
        assert e_64 <= 2 * r["m"], (e_64, r["m"])
    same = got.view(np.uint32) == small.view(np.uint32)[idx]
    assert same.all(), (int((~same).sum()), int(np.flatnonzero(~same)[0]))


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_rows_zero_is_a_noop(dev, precision):
    from swarm_marl_amd import _native as nat
    c = critic(dev, 21, precision)
    out = c.value(torch.empty((0, 21), dtype=torch.float32, device=dev))
    assert tuple(out.shape) == (0,)
    keep = torch.full((8,), 3.0, dtype=torch.float32, device=dev)
    gs = torch.zeros((8, 21), dtype=torch.float32, device=dev)
    assert c.lib.swarm_critic_forward(ctypes.byref(c._c), gs.data_ptr(), 0, keep.data_ptr(), None) == nat.SWARM_OK
    torch.cuda.synchronize()
    assert torch.all(keep == 3.0)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_block_view_equals_flat_rows_and_repeats_bitwise(dev, precision):
    in_dim, t1, e = 387, 4, 65  # 260 rows: three bf16 row tiles, the last ragged
    r = ref(in_dim)
    c = critic(dev, in_dim, precision)
    x = torch.from_numpy(np.concatenate([r["x"], r["x"][:3]])).to(dev)
    flat = c.value(x)
    block = c.value(x.view(t1, e, in_dim))
    assert tuple(block.shape) == (t1, e)
    again = c.value(x)
    assert torch.equal(block.reshape(-1), flat) and torch.equal(again, flat)
    assert np.array_equal(flat.cpu().numpy()[:257], run_guarded(c, r["x"], dev))


def test_value_validates_its_arguments(dev):
    c = critic(dev, 21, "f32")
    good = torch.zeros((4, 21), dtype=torch.float32, device=dev)
    for bad in (good.cpu(), good.double(), torch.zeros((4, 22), dtype=torch.float32, device=dev), good.t().contiguous().t()):
        with pytest.raises(ValueError):
            c.value(bad)
    with pytest.raises(ValueError):
        c.value(good, out=torch.zeros(5, dtype=torch.float32, device=dev))
