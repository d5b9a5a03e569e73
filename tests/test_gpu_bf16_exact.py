"""GPU: the bf16 actor, per-agent value, centralized critic and training kernels, bit for bit.

On the fixtures of tests/bf16_exact_ref.py every sum the kernels form is a sum of integers whose
absolute values add up to less than 2^24 (asserted on the CPU by tests/test_bf16_exact_cpu.py), so
every f32 accumulation is exact in any order and every bf16 rounding, ties included, is a pure
function of an exact integer: the outputs are fully determined by include/swarm_mi355x.h's formulas.
Every comparison here is on bits, against `bf16_exact_ref.forward` (float64 NumPy, written from the
formulas, never reading a blob); no tolerance, no excluded element.  A mismatch reports the shape,
the first differing element and both bit patterns.  Outputs are written into the heads of
sentinel-filled buffers.

  actor     PolicyMLP(precision="bf16"): (37, 6) the compile-time instance, (37, 4) and (36, 6) its
            neighbours on the runtime instance, in + 1 on and past the 16-wide k-steps, both minima and
            maxima; rows the prefixes 1, 31, 32, 33, 255, 256, 257 of one set; mean-mode actions are
            logits[:, :out/2]; a sampled launch leaves the logits alone; a second grid pass at (37, 6)
            and (36, 6).
  value     AgentValueMLP: in_dim 37 (compile-time) and 36, 1, 15, 16, 31, 32, 47; the same prefixes;
            a second grid pass.
  critic    CriticMLP: in_dim 1, 30, 31 / 63 (the bias column last in a 32-column chunk), 32 / 64 (alone
            in a chunk of its own), 387, 1539 (49 chunks); rows 1, 127, 128, 129, 257; a second grid pass
            at in_dim 63.
  training  ActorTrainer on the dense fixtures with integer grad_logits in -2..2: its logits, the
            stages h1, h2, dz2, dz1 (dz2 and dz1 round, ties included) and the six gradients against
            tests/train_ref.py's stage functions; after push() the blob is the host pack and the logits
            do not move.
The Gaussian tests of these kernels (test_gpu_policy.py, test_gpu_policy_dims.py, test_gpu_value.py,
test_gpu_critic.py, test_gpu_train.py) stay as they are: they cover realistic magnitudes, this file
the rounding rules and the layout.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import bf16_exact_ref as br
from tests import train_ref as tr

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


_FIX = {}


def fix(case):
    """Per (kind, in_dim, out_dim), computed once: layers, the 257 rows, the reference outputs as f32."""
    if case not in _FIX:
        layers, x = br.fixture(*case)
        want = br.forward(layers, x)["out"]
        want32 = want.astype(f32)
        assert np.array_equal(want32.astype(f64), want)  # integers below 2^24
        _FIX[case] = dict(layers=layers, x=x, want=want32)
    return _FIX[case]


def assert_bits(got: np.ndarray, want: np.ndarray, tag: str) -> int:
    """got == want bit for bit (both f32, or both bf16 patterns); returns the elements compared."""
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape)
    view = np.uint32 if got.dtype == f32 else np.uint16
    g, w = np.ascontiguousarray(got).view(view), np.ascontiguousarray(want).view(view)
    bad = np.argwhere(g != w)
    if bad.size:
        at = tuple(int(i) for i in bad[0])
        raise AssertionError(f"{tag}: {len(bad)} of {g.size} elements differ, first at {at}: "
                             f"kernel {int(g[at]):#x} ({got[at]}), reference {int(w[at]):#x} ({want[at]})")
    return g.size


def guarded_logits(pol, obs: torch.Tensor, **kw):
    """forward() into the heads of longer sentinel-filled buffers: nothing past rows * out or
    rows * out / 2 is written."""
    rows, out, ad = obs.shape[0], pol.out_dim, pol.out_dim // 2
    lbuf = torch.full((rows * out + 300,), -777.0, dtype=torch.float32, device=obs.device)
    abuf = torch.full((rows * ad + 300,), -555.0, dtype=torch.float32, device=obs.device)
    pol.forward(obs, logits=lbuf[:rows * out].view(rows, out), actions=abuf[:rows * ad].view(rows, ad), **kw)
    lg, ac = lbuf.cpu().numpy(), abuf.cpu().numpy()
    assert np.all(lg[rows * out:] == -777.0) and np.all(ac[rows * ad:] == -555.0)
    return lg[:rows * out].reshape(rows, out), ac[:rows * ad].reshape(rows, ad)


def guarded_value(net, x: torch.Tensor) -> np.ndarray:
    rows = x.shape[0]
    buf = torch.full((rows + 300,), -777.0, dtype=torch.float32, device=x.device)
    net.value(x, out=buf[:rows])
    got = buf.cpu().numpy()
    assert np.all(got[rows:] == -777.0)
    return got[:rows]


def repeated(x257: torch.Tensor, rows: int) -> torch.Tensor:
    """The 257-row set repeated on the device to `rows` rows: row r is row r mod 257 (257 is coprime
    with every tile size, so every row of the set lands in every lane position)."""
    x = x257.repeat((rows + br.ROWS - 1) // br.ROWS, 1)[:rows]
    assert x.is_contiguous() and x.shape == (rows, x257.shape[1])
    return x


# ---------------------------------------------------------------- actor
def _actor(dev, shape):
    from swarm_marl_amd.policy import PolicyMLP
    c = fix(("actor",) + shape)
    if "pol" not in c:
        c["pol"] = PolicyMLP(c["layers"], device=dev, precision="bf16")
        c["xd"] = torch.from_numpy(c["x"]).to(dev)
    return c


@pytest.mark.parametrize("shape", br.ACTOR_SHAPES, ids=[f"{i}to{o}" for i, o in br.ACTOR_SHAPES])
def test_actor_logits_bitwise(dev, shape):
    c = _actor(dev, shape)
    ad, n = shape[1] // 2, 0
    for rows in br.ACTOR_PREFIXES:
        lg, ac = guarded_logits(c["pol"], c["xd"][:rows])
        n += assert_bits(lg, c["want"][:rows], f"actor {shape} rows={rows}")
        assert_bits(ac, np.ascontiguousarray(lg[:, :ad]), f"actor {shape} rows={rows} mean actions")
    lg, _ = guarded_logits(c["pol"], c["xd"], sample=True, seed=5, counter=7)
    n += assert_bits(lg, c["want"], f"actor {shape} sampled launch")
    print(f"actor {shape}: {len(br.ACTOR_PREFIXES) + 1} launches, {n} logits compared")


@pytest.mark.parametrize("shape", [(37, 6), (36, 6)], ids=["37to6", "36to6"])
def test_actor_second_grid_pass(dev, shape):
    c = _actor(dev, shape)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    rows = cus * 8 * 32 * 3 // 2 + 77
    lg, ac = guarded_logits(c["pol"], repeated(c["xd"], rows))
    n = assert_bits(lg, c["want"][np.arange(rows) % br.ROWS], f"actor {shape} rows={rows}")
    assert_bits(ac, np.ascontiguousarray(lg[:, :shape[1] // 2]), f"actor {shape} rows={rows} mean actions")
    print(f"actor {shape} rows={rows}: {n} logits compared")


# ---------------------------------------------------------------- per-agent value
def _tower(dev, cls_name, d):
    import swarm_marl_amd
    c = fix(("tower", d, 1))
    if cls_name not in c:
        c[cls_name] = getattr(swarm_marl_amd, cls_name)(c["layers"], device=dev, precision="bf16")
        c["xd"] = torch.from_numpy(c["x"]).to(dev)
    return c, c[cls_name]


@pytest.mark.parametrize("d", br.VALUE_IN_DIMS)
def test_value_bitwise(dev, d):
    c, net = _tower(dev, "AgentValueMLP", d)
    n = sum(assert_bits(guarded_value(net, c["xd"][:rows]), c["want"][:rows], f"value in={d} rows={rows}")
            for rows in br.ACTOR_PREFIXES)
    print(f"value in={d}: {len(br.ACTOR_PREFIXES)} launches, {n} values compared")


def test_value_second_grid_pass(dev):
    from tests.test_gpu_value import GRID
    d = 37
    c, net = _tower(dev, "AgentValueMLP", d)
    tile, per_cu = GRID
    rows = torch.cuda.get_device_properties(dev).multi_processor_count * per_cu * tile * 3 // 2 + 77
    n = assert_bits(guarded_value(net, repeated(c["xd"], rows)), c["want"][np.arange(rows) % br.ROWS],
                    f"value in={d} rows={rows}")
    print(f"value in={d} rows={rows}: {n} values compared")


# ---------------------------------------------------------------- centralized critic
@pytest.mark.parametrize("d", br.CRITIC_IN_DIMS)
def test_critic_bitwise(dev, d):
    c, net = _tower(dev, "CriticMLP", d)
    n = sum(assert_bits(guarded_value(net, c["xd"][:rows]), c["want"][:rows], f"critic in={d} rows={rows}")
            for rows in br.CRITIC_ROWS)
    print(f"critic in={d}: {len(br.CRITIC_ROWS)} launches, {n} values compared")


def test_critic_second_grid_pass(dev):
    from tests.test_gpu_critic import GRID
    d = 63
    c, net = _tower(dev, "CriticMLP", d)
    tile, per_cu = GRID["bf16"]
    rows = torch.cuda.get_device_properties(dev).multi_processor_count * per_cu * tile * 3 // 2 + 77
    n = assert_bits(guarded_value(net, repeated(c["xd"], rows)), c["want"][np.arange(rows) % br.ROWS],
                    f"critic in={d} rows={rows}")
    print(f"critic in={d} rows={rows}: {n} values compared")


# ---------------------------------------------------------------- training
@pytest.mark.parametrize("rows", br.TRAIN_ROWS)
@pytest.mark.parametrize("shape", br.TRAIN_SHAPES, ids=[f"{i}to{o}" for i, o in br.TRAIN_SHAPES])
def test_training_stages_and_gradients_bitwise(dev, shape, rows):
    from swarm_marl_amd import ActorTrainer
    from swarm_marl_amd.policy import PolicyMLP
    layers, x, g, wide = br.train_fixture(*shape, rows)
    assert max(br.grad_budget(layers, x, g).values()) < br.LIMIT  # the gradients' own budget
    want = br.forward(layers, x)
    want_s, want_g = tr.emulate(layers, x, g)
    assert np.array_equal(want_s["h1"], want["h1"]) and np.array_equal(want_s["h2"], want["h2"])
    pol = PolicyMLP(layers, device=dev, precision="bf16")
    trainer = ActorTrainer(pol)
    xd, gd = torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev)
    tag = f"train {shape} rows={rows} wide={wide}"
    logits = trainer.logits(xd).cpu().numpy()
    n = assert_bits(logits, want["out"].astype(f32), f"{tag} logits")
    assert_bits(guarded_logits(pol, xd)[0], logits, f"{tag} the actor's logits")
    st = trainer.backward(xd, gd, stages=True)
    for k in ("h1", "h2", "dz2", "dz1"):
        n += assert_bits(st[k].cpu().numpy().view(np.uint16), tr.bits(want_s[k]), f"{tag} stage {k}")
    for name, p in zip(tr.NAMES, trainer.masters):
        w32 = want_g[name].astype(f32)
        assert np.array_equal(w32.astype(f64), want_g[name])
        n += assert_bits(p.grad.cpu().numpy(), w32 + f32(0), f"{tag} d{name}")  # + 0: an exact zero sum is +0
    # push() of these masters: the host packer's bytes, and the logits stay
    pol.weights.fill_(0xAB)
    trainer.push()
    assert torch.equal(pol.weights.cpu(), torch.from_numpy(pol.packed_host))
    assert_bits(trainer.logits(xd).cpu().numpy(), logits, f"{tag} logits after push")
    print(f"{tag}: {n} elements compared")
