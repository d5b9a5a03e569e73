"""GPU: the actor kernels (csrc/swarm_policy.hip) off the default 37 -> 6 dims.

swarm_policy_forward takes in_dim 1..47 and even out_dim 2..12; for (37, 6) the bf16 path launches
compile-time-dims instances, every other shape the runtime-dims ones: the pad / bias-column selects
(k < in, k == in), the layer-3 row masks (m < out, w3lane, w3idx), F32Layout.kq1, ad = out / 2 in the
action epilogue and the second Philox block (ad > 2) only run here.

Weights uniform(-1, 1) / sqrt(fan_in) seeded per shape, observations uniform(-3, 3), 257 rows per
shape and its prefixes 1, 33, 65 (tests/policy_ref.py).  References and bounds:
  f32, f32x3  float64 NumPy forward, |err| <= 1e-4 + 1e-5 |ref| (the project's f32 logit bound).
  bf16        the host emulation of the kernel's bf16 arithmetic from the packed blob
              (tests/test_policy_cpu.py emulate_bf16_kernel, generic in d and out), <= 1e-3; and the
              float64 forward, max|err| <= 2 m, m the emulation's own maximum error against float64
              on the shape's inputs (from the two references, never from the kernel).
Logits and actions are written into the heads of sentinel-filled buffers: nothing past rows * out
or rows * out / 2 changes; in mean mode the actions are logits[:, :out/2] bit for bit.

Sampling (bf16, out_dim 2, 4, 6, 12 and the default shape's compile-time instance): the kernel's
standard normals are recovered from its own outputs, z = (a - mean) exp(-log_std), and compared
with policy_ref.sample_noise64 (Philox4x32-10 + Box-Muller from the kernel's definition, float64).
Error budget of |z - z_ref|: the angle 2 pi u2 is rounded to f32 (<= 2.4e-7 absolute on an angle
below 6.29) and multiplies a radius <= sqrt(-2 ln 2^-25) = 5.9: <= 1.5e-6; a few ulps in logf, sqrtf,
cosf, sinf add about the same again; recovering z through a = mean + exp(log_std) z costs a's f32
rounding, 2^-24 |a| exp(-log_std), and expf's ulps on z.  Bound:
  |z - z_ref| <= 1e-5 (1 + |z_ref|) + 2^-22 |a| exp(-log_std),   log_std in [-2, 0.5] (asserted).
Measured maximum of |z - z_ref| on an MI355X over every case below: 8.298e-7 (MEASURED_Z_ERR; at
most 0.052 of the bound).  Measured bf16 logits against the emulation: at most 1.078e-4 ((31, 12),
one flipped bf16 activation at rows = 257; 1e-7 where none flips).
The bit-exact layer of the bf16 path (rounding rules, format, no tolerance) is tests/test_gpu_bf16_exact.py.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import policy_ref as pr

pytestmark = pytest.mark.gpu

PREFIXES = (1, 33, 65, 257)
BIG_ROWS = 70_001  # > 256 CUs x 8 waves x 32 rows (bf16, f32x3) and > 512 blocks x 4 waves x 16 rows (f32)
BIG_SHAPE = (25, 6)
MEASURED_Z_ERR = 8.298e-7  # a record, not a bound: see the docstring


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _ids(shapes):
    return [f"{i}to{o}" for i, o in shapes]


_REF = {}


def ref(shape):
    """Per shape, computed once: layers, the 257 observations, the float64 logits."""
    if shape not in _REF:
        layers = pr.make_actor(*shape)
        x = pr.obs_set(shape[0])
        _REF[shape] = dict(layers=layers, x=x, l64=pr.forward64(layers, x))
    return _REF[shape]


_POL = {}


def policy(dev, shape, precision):
    from swarm_marl_amd.policy import PolicyMLP
    key = (shape, precision)
    if key not in _POL:
        _POL[key] = PolicyMLP(ref(shape)["layers"], device=dev, precision=precision)
    return _POL[key]


def bf16_refs(pol, shape):
    """The blob emulation on the shape's inputs and m, its own maximum error against float64."""
    from tests.test_policy_cpu import emulate_bf16_kernel
    r = ref(shape)
    if "emu" not in r:
        r["emu"] = emulate_bf16_kernel(pol.packed_host, r["x"], shape[1])
        r["m"] = np.abs(r["emu"] - r["l64"]).max()
    return r["emu"], r["m"]


def run_guarded(pol, obs: torch.Tensor, **kw):
    """forward() into the heads of longer sentinel-filled buffers: (logits, actions) on the host,
    nothing written past rows * out or rows * out / 2."""
    rows, out, ad = obs.shape[0], pol.out_dim, pol.out_dim // 2
    lbuf = torch.full((rows * out + 300,), -777.0, dtype=torch.float32, device=obs.device)
    abuf = torch.full((rows * ad + 300,), -555.0, dtype=torch.float32, device=obs.device)
    pol.forward(obs, logits=lbuf[:rows * out].view(rows, out), actions=abuf[:rows * ad].view(rows, ad), **kw)
    lg, ac = lbuf.cpu().numpy(), abuf.cpu().numpy()
    assert np.all(lg[rows * out:] == -777.0) and np.all(ac[rows * ad:] == -555.0)
    return lg[:rows * out].reshape(rows, out), ac[:rows * ad].reshape(rows, ad)


def check_f32(got, want, tag):
    err = np.abs(got - want)
    print(f"{tag} max err {err.max():.3e} (bound use {np.max(err / (1e-4 + 1e-5 * np.abs(want))):.3f})")
    assert np.all(err <= 1e-4 + 1e-5 * np.abs(want)), (tag, err.max())


def check_bf16(got, emu, l64, m, tag):
    e_emu, e_64 = np.abs(got - emu).max(), np.abs(got - l64).max()
    print(f"{tag} vs emulation {e_emu:.3e}  vs float64 {e_64:.3e}  m {m:.3e}")
    assert e_emu <= 1e-3, (tag, e_emu)
    assert e_64 <= 2 * m, (tag, e_64, m)


@pytest.mark.parametrize("precision", ["f32", "f32x3"])
@pytest.mark.parametrize("shape", pr.SHAPES, ids=_ids(pr.SHAPES))
def test_f32_logits_vs_float64(dev, shape, precision):
    r = ref(shape)
    pol = policy(dev, shape, precision)
    x = torch.from_numpy(r["x"]).to(dev)
    for rows in PREFIXES:
        lg, ac = run_guarded(pol, x[:rows])
        assert np.array_equal(ac.view(np.uint32), lg[:, :shape[1] // 2].view(np.uint32)), rows
        check_f32(lg, r["l64"][:rows], f"{precision} {shape} rows={rows}")


@pytest.mark.parametrize("shape", pr.SHAPES, ids=_ids(pr.SHAPES))
def test_bf16_logits_vs_emulation_and_float64(dev, shape):
    r = ref(shape)
    pol = policy(dev, shape, "bf16")
    emu, m = bf16_refs(pol, shape)
    x = torch.from_numpy(r["x"]).to(dev)
    for rows in PREFIXES:
        lg, ac = run_guarded(pol, x[:rows])
        assert np.array_equal(ac.view(np.uint32), lg[:, :shape[1] // 2].view(np.uint32)), rows
        check_bf16(lg, emu[:rows], r["l64"][:rows], m, f"bf16 {shape} rows={rows}")


@pytest.mark.parametrize("precision", ["bf16", "f32", "f32x3"])
def test_more_row_tiles_than_one_grid_pass(dev, precision):
    """70,001 rows of a runtime-dims shape: the 257-row set repeated on the device, so row r is
    checked against the 257-row reference of row r mod 257 (the wave's second tile, the ragged last
    tile and every lane position of a tile: 257 is coprime with 16 and 32)."""
    shape = BIG_SHAPE
    r = ref(shape)
    pol = policy(dev, shape, precision)
    x = torch.from_numpy(r["x"]).to(dev).repeat((BIG_ROWS + pr.ROWS - 1) // pr.ROWS, 1)[:BIG_ROWS]
    assert x.is_contiguous() and x.shape == (BIG_ROWS, shape[0])
    lg, ac = run_guarded(pol, x)
    assert np.array_equal(ac.view(np.uint32), lg[:, :shape[1] // 2].view(np.uint32))
    idx = np.arange(BIG_ROWS) % pr.ROWS
    if precision == "bf16":
        emu, m = bf16_refs(pol, shape)
        check_bf16(lg, emu[idx], r["l64"][idx], m, f"bf16 {shape} rows={BIG_ROWS}")
    else:
        check_f32(lg, r["l64"][idx], f"{precision} {shape} rows={BIG_ROWS}")


# ---------------------------------------------------------------- sampling
SAMPLE_SHAPES = ((15, 2), (16, 4), (25, 6), (47, 12), (37, 6))  # ad = 1, 2, 3, 6; the compile-time instance
SEEDS = ((5, 7), (0x9E3779B97F4A7C15, (1 << 32) + 3))  # the second: all four key / counter words non-zero


def _recovered_z(pol, x, seed, counter):
    lg, a = run_guarded(pol, x, sample=True, seed=seed, counter=counter)
    ad = pol.out_dim // 2
    mean, ls = lg[:, :ad].astype(np.float64), lg[:, ad:].astype(np.float64)
    assert ls.min() >= -2.0 and ls.max() <= 0.5, (ls.min(), ls.max())
    return (a.astype(np.float64) - mean) * np.exp(-ls), a.astype(np.float64), ls, lg


@pytest.mark.parametrize("seed,counter", SEEDS, ids=["low_words", "all_words"])
@pytest.mark.parametrize("shape", SAMPLE_SHAPES, ids=_ids(SAMPLE_SHAPES))
def test_sampled_noise_is_the_defined_philox_box_muller(dev, shape, seed, counter):
    from swarm_marl_amd.policy import PolicyMLP
    ad = shape[1] // 2
    pol = PolicyMLP(pr.make_actor(*shape, log_std_scale=0.25), device=dev, precision="bf16")
    x = torch.from_numpy(pr.obs_set(shape[0])).to(dev)
    z, a, ls, lg = _recovered_z(pol, x, seed, counter)
    mean_lg, _ = run_guarded(pol, x)
    assert np.array_equal(lg.view(np.uint32), mean_lg.view(np.uint32))  # sampling leaves the logits alone
    z_ref = pr.sample_noise64(pr.ROWS, ad, seed, counter)
    err = np.abs(z - z_ref)
    bound = 1e-5 * (1 + np.abs(z_ref)) + 2.0 ** -22 * np.abs(a) * np.exp(-ls)
    print(f"sample {shape} seed={seed:#x} counter={counter:#x}: max |z - z_ref| {err.max():.3e} "
          f"(bound use {np.max(err / bound):.3f}, max |z| {np.abs(z_ref).max():.2f})")
    assert np.all(err <= bound), (err.max(), np.max(err / bound))
    # rows get their own draws, and so do consecutive counters
    for i, j in ((0, 1), (0, 32), (1, 32)):
        assert np.abs(z[i] - z[j]).max() > 1e-3, (i, j)
    z2, _, _, _ = _recovered_z(pol, x, seed, counter + 1)
    assert np.abs(z2 - z).max(axis=1).min() > 1e-6 and np.abs(z2 - z).max() > 0.1
    z3, _, _, _ = _recovered_z(pol, x, seed, counter)
    assert np.array_equal(z3, z)
    # prefixes: a row's draw depends on its index, not on the launch's row count
    for rows in (1, 33):
        zp, _, _, _ = _recovered_z(pol, x[:rows], seed, counter)
        assert np.array_equal(zp, z[:rows]), rows


# ---------------------------------------------------------------- limits
@pytest.mark.parametrize("in_dim,out_dim", [(48, 6), (37, 14), (37, 5)])
def test_dims_out_of_range_raise_with_the_policy_error_string(dev, in_dim, out_dim):
    from swarm_marl_amd import _native as nat
    from swarm_marl_amd.policy import PolicyMLP
    lib = nat.load_library()
    # leave another message in every other component's error string
    assert lib.swarm_critic_packed_bytes(0, 0) < 0 and b"critic" in lib.swarm_critic_last_error()
    assert lib.swarm_policy_packed_bytes(37, 6, 7) < 0 and b"precision" in lib.swarm_policy_last_error()
    with pytest.raises(ValueError, match="policy dims out of range"):
        PolicyMLP(pr.make_actor(in_dim, out_dim), device=dev)
    assert lib.swarm_policy_last_error() == b"policy dims out of range"


def test_collector_rejects_an_env_wider_than_the_actor_supports(dev):
    """obs_dim = 9 + 4 * 6 + 4 * 10 = 73 > 47: no PolicyMLP of that width exists, and the collector
    refuses any other before it allocates or launches anything."""
    from swarm_marl_amd import RolloutCollector, VecSwarm
    vec = VecSwarm(4, dict(num_drones=8, neighbor_k=6, sensed_obstacles=10, num_obstacles=10), device=dev, seed=1)
    assert vec.obs_dim == 73
    with pytest.raises(ValueError, match="policy dims out of range"):
        policy(dev, (vec.obs_dim, 6), "bf16")
    obs_before = vec.obs.clone()
    with pytest.raises(ValueError, match="73"):
        RolloutCollector(vec, policy(dev, (37, 6), "bf16"), horizon=4)
    assert torch.equal(vec.obs, obs_before)
