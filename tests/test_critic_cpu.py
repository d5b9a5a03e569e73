"""CPU: the centralized critic's host side (swarm_critic_packed_bytes / swarm_critic_pack through the
loaded library, CriticMLP.from_state_dict) and the arithmetic the GPU tests hold the kernels to.

* The packed bf16 blob, decoded through the MFMA fragment maps the kernel assumes and evaluated in
  NumPy (tests/critic_ref.py: bf16 operands, float64 sums, activations re-rounded), reproduces a
  direct bf16-rounded evaluation of the same weights: the chunk order, the fragment permutation
  and the accumulator-chaining permutation of W2 agree.  The GPU tests check the maps against the
  hardware.
* The f32 GAE loop of include/swarm_mi355x.h stays within 1e-5 * max(1, max|ref|) of a float64 loop.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from tests import critic_ref as cr


@pytest.fixture(scope="module")
def nat():
    from swarm_marl_amd import _native
    return _native


@pytest.fixture(scope="module")
def lib(nat):
    return nat.load_library()


def test_packed_bytes(nat, lib):
    for d in cr.IN_DIMS + (1,):
        nc1 = (d + 1 + 31) // 32
        assert lib.swarm_critic_packed_bytes(d, nat.POLICY_BF16) == (nc1 + 8) * 16384 + 2048 + 16
        assert lib.swarm_critic_packed_bytes(d, nat.POLICY_F32) == 4 * (d * 256 + 256 + 65536 + 256 + 256 + 4)
    assert nat.CRITIC_MAX_IN == 1539


@pytest.mark.parametrize("args,code", [((0, 0), "ELIMIT"), ((-3, 1), "ELIMIT"), ((1540, 0), "ELIMIT"),
                                       ((387, 2), "ELIMIT"), ((387, 7), "EINVAL")])
def test_bad_dims_return_a_code_and_a_message(nat, lib, args, code):
    want = getattr(nat, "SWARM_" + code)
    assert lib.swarm_critic_packed_bytes(*args) == want
    assert lib.swarm_critic_last_error()
    a = np.zeros(4, np.float32)
    fp = a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.swarm_critic_pack(*args, fp, fp, fp, fp, fp, fp, a.ctypes.data) == want  # rejected before any read
    with pytest.raises(ValueError):
        nat.check(want, lib, which="critic")


def test_null_arguments_and_empty_batches(nat, lib):
    assert lib.swarm_critic_pack(15, 0, None, None, None, None, None, None, None) == nat.SWARM_ENULL
    assert b"null" in lib.swarm_critic_last_error().lower()
    c = nat.SwarmCritic(387, nat.POLICY_BF16, None)
    assert lib.swarm_critic_forward(None, None, 4, None, None) == nat.SWARM_ENULL
    assert lib.swarm_critic_forward(ctypes.byref(c), None, 4, None, None) == nat.SWARM_ENULL
    c.weights = 4096
    assert lib.swarm_critic_forward(ctypes.byref(c), None, -1, None, None) == nat.SWARM_EINVAL
    assert lib.swarm_critic_forward(ctypes.byref(c), None, 0, None, None) == 0      # rows == 0: no-op
    assert lib.swarm_critic_forward(ctypes.byref(c), None, 4, None, None) == nat.SWARM_ENULL
    c.precision = nat.POLICY_F32X3
    assert lib.swarm_critic_forward(ctypes.byref(c), 16, 4, 16, None) == nat.SWARM_ELIMIT
    assert lib.swarm_gaussian_logp(None, None, 0, 3, None, None) == 0
    assert lib.swarm_gaussian_logp(None, None, 5, 3, None, None) == nat.SWARM_ENULL
    assert lib.swarm_gaussian_logp(16, 16, 5, 0, 16, None) == nat.SWARM_EINVAL
    assert lib.swarm_gae(None, None, None, None, None, None, 0, 4, 4, 0.99, 0.95, None, None, None) == 0
    assert lib.swarm_gae(None, None, None, None, None, None, 2, 4, 4, 0.99, 0.95, None, None, None) == nat.SWARM_ENULL
    assert lib.swarm_gae(None, None, None, None, None, None, -1, 4, 4, 0.99, 0.95, None, None, None) == nat.SWARM_EINVAL


@pytest.mark.parametrize("in_dim", cr.IN_DIMS)
def test_bf16_blob_emulation_reproduces_direct_bf16(nat, lib, in_dim):
    layers = cr.make_critic(in_dim)
    buf = cr.pack(lib, layers, nat.POLICY_BF16)
    x = cr.global_state_like(37, in_dim, seed=in_dim)
    got = cr.emulate_bf16_blob(buf, x)
    ref = cr.direct_bf16(layers, x)
    # the same rounded operands summed in float64 in another order: only a sum within ~1e-15 of a
    # bf16 rounding tie could differ
    assert np.abs(got - ref).max() <= 1e-9, np.abs(got - ref).max()
    # and it is the critic: within bf16's error of the float64 truth
    v64 = cr.truth64(layers, x)
    assert np.abs(got - v64).max() < 0.05 * max(1.0, np.abs(v64).max())
    # the permutations matter: W2 read without the chaining permutation is another function
    nc1 = (in_dim + 1 + 31) // 32
    w2 = buf[nc1 * 16384:(nc1 + 8) * 16384].view(np.uint16).reshape(8, 16, 2, 32, 8)
    dense = np.zeros((256, 256), np.uint16)
    for ks in range(16):
        for h in range(2):
            for j in range(8):
                dense[:, 16 * ks + 8 * h + j] = w2[:, ks, h, :, j].reshape(256)
    assert not np.array_equal(cr.from_bf16(dense), cr.to_bf16(layers[1][0]))


def test_f32_blob_is_the_transposed_weights(nat, lib):
    layers = cr.make_critic(21)
    (w1, b1), (w2, b2), (w3, b3) = layers
    f = cr.pack(lib, layers, nat.POLICY_F32).view(np.float32)
    assert np.array_equal(f[:21 * 256].reshape(21, 256), w1.T)
    off = 21 * 256
    assert np.array_equal(f[off:off + 256], b1)
    assert np.array_equal(f[off + 256:off + 256 + 65536].reshape(256, 256), w2.T)
    off += 256 + 65536
    assert np.array_equal(f[off:off + 256], b2) and np.array_equal(f[off + 256:off + 512], w3[0])
    assert f[off + 512] == b3[0]


def _rllib_state_dict(layers, prefix="value_model."):
    names = ["_hidden_layers.0._model.0", "_hidden_layers.1._model.0", "_logits._model.0"]
    sd = {}
    for name, (w, b) in zip(names, layers):
        sd[prefix + name + ".weight"] = torch.from_numpy(w)
        sd[prefix + name + ".bias"] = torch.from_numpy(b)
    return sd


def test_from_state_dict():
    from swarm_marl_amd import CriticMLP
    layers = cr.make_critic(387)
    sd = _rllib_state_dict(layers)
    # the actor's layers, TorchFC's unused value head and a 1-D entry are all ignored
    sd.update(_rllib_state_dict(cr.make_critic(37, seed=1), prefix="action_model."))
    sd["value_model._value_branch._model.0.weight"] = torch.zeros(1, 256)
    sd["value_model._value_branch._model.0.bias"] = torch.zeros(1)
    sd["log_std"] = torch.zeros(3)
    c = CriticMLP.from_state_dict(sd, device="cpu")
    assert c.in_dim == 387 and c.precision == "bf16"
    for (w, b), (w0, b0) in zip(c.layers, layers):
        assert np.array_equal(w, w0) and np.array_equal(b, b0)
    ref = CriticMLP.from_arrays(*[a for wb in layers for a in wb], device="cpu")
    assert np.array_equal(c.packed_host, ref.packed_host)
    # names are not relied on: the same chain under other names, in another order
    odd = {"vf.c.weight": sd["value_model._logits._model.0.weight"], "vf.c.bias": sd["value_model._logits._model.0.bias"],
           "vf.a.weight": sd["value_model._hidden_layers.0._model.0.weight"],
           "vf.a.bias": sd["value_model._hidden_layers.0._model.0.bias"],
           "vf.b.weight": sd["value_model._hidden_layers.1._model.0.weight"],
           "vf.b.bias": sd["value_model._hidden_layers.1._model.0.bias"]}
    c2 = CriticMLP.from_state_dict(odd, prefix="vf.", device="cpu", precision="f32")
    assert np.array_equal(c2.layers[0][0], layers[0][0]) and np.array_equal(c2.layers[2][0], layers[2][0])
    # wrong shapes: a clear error
    bad = dict(sd)
    bad["value_model._hidden_layers.1._model.0.weight"] = torch.zeros(128, 256)
    bad["value_model._hidden_layers.1._model.0.bias"] = torch.zeros(128)
    with pytest.raises(ValueError, match="256 -> 256 -> 1"):
        CriticMLP.from_state_dict(bad, device="cpu")
    with pytest.raises(ValueError, match="256 -> 256 -> 1"):
        CriticMLP.from_state_dict(sd, prefix="nothing.", device="cpu")
    with pytest.raises(ValueError):
        CriticMLP.from_arrays(np.zeros((256, 1540), np.float32), *[a for wb in layers for a in wb][1:], device="cpu")
    with pytest.raises(ValueError):
        CriticMLP.from_arrays(*[a for wb in layers for a in wb], device="cpu", precision="f32x3")


@pytest.mark.parametrize("shape", [(1, 1, 1), (7, 33, 4), (16, 5, 64), (64, 3, 8)])
def test_f32_gae_loop_tracks_float64(shape):
    args = cr.random_gae_inputs(*shape, seed=sum(shape))
    a32, t32 = cr.gae_loop(*args, 0.99, 0.95, dtype=np.float32)
    a64, t64 = cr.gae_loop(*args, 0.99, 0.95, dtype=np.float64)
    assert a32.dtype == np.float32
    for got, ref in ((a32, a64), (t32, t64)):
        assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
    valid = args[5]
    assert np.all(a32[~valid] == 0) and np.all(t32[~valid] == 0)


def test_gae_loop_semantics():
    """One agent, hand-checked: an episode end stops the bootstrap and the carry; an invalid step
    zeroes both and the carry; only the fragment end bootstraps."""
    r = np.array([1.0, 2.0, 3.0, 4.0], np.float32).reshape(4, 1, 1)
    v = np.array([0.5, 0.25, 1.0, 2.0, 8.0], np.float32).reshape(5, 1)
    z = np.zeros((4, 1, 1), bool)
    ok = np.ones((4, 1, 1), bool)
    trunc = z.copy()
    trunc[1] = True  # the agent's own truncation at t = 1: not bootstrapped
    adv, tgt = cr.gae_loop(r, v, z, trunc, np.zeros((4, 1), np.uint8), ok, 0.5, 1.0, dtype=np.float64)
    a3 = 4 + 0.5 * 8 - 2
    a2 = 3 + 0.5 * 2 - 1 + 0.5 * a3
    a1 = 2 - 0.25
    a0 = 1 + 0.5 * 0.25 - 0.5 + 0.5 * a1
    assert np.allclose(adv[:, 0, 0], [a0, a1, a2, a3]) and np.allclose(tgt[:, 0, 0], adv[:, 0, 0] + v[:4, 0])
    env = np.zeros((4, 1), np.uint8)
    env[2] = cr.ENV_TERMINATED | cr.ENV_RESET  # the env's __all__ at t = 2
    ok2 = ok.copy()
    ok2[1] = False
    adv, _ = cr.gae_loop(r, v, z, z, env, ok2, 0.5, 1.0, dtype=np.float64)
    assert np.allclose(adv[:, 0, 0], [1 + 0.5 * 0.25 - 0.5, 0.0, 3 - 1.0, a3])
