"""CPU: the per-agent critic's host side (swarm_value_packed_bytes / swarm_value_pack through the
loaded library, AgentValueMLP.from_state_dict) and the arithmetic the GPU tests hold the kernels to.

* The packed bf16 blob, decoded through the MFMA fragment maps the kernel assumes and evaluated in
  NumPy (tests/value_ref.py: bf16 operands, float64 sums, activations re-rounded), reproduces a
  direct bf16-rounded evaluation of the same weights at every tested in_dim: the fragment
  permutation, the bias column and the accumulator-chaining permutation of W2 agree.  The GPU tests
  check the maps against the hardware.
* The f32 blob is swarm_critic_pack's.
* The f32 per-agent GAE loop of include/swarm_mi355x.h stays within 1e-5 * max(1, max|ref|) of a
  float64 loop, and with value[t, e, n] = v[t, e] it is tests/critic_ref.py's gae_loop bit for bit.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from tests import critic_ref as cr
from tests import value_ref as vr


@pytest.fixture(scope="module")
def nat():
    from swarm_marl_amd import _native
    return _native


@pytest.fixture(scope="module")
def lib(nat):
    return nat.load_library()


def test_packed_bytes(nat, lib):
    for d in vr.IN_DIMS:
        assert lib.swarm_value_packed_bytes(d, nat.POLICY_BF16) == vr.BLOB_BYTES == 157712
        assert lib.swarm_value_packed_bytes(d, nat.POLICY_F32) == lib.swarm_critic_packed_bytes(d, nat.POLICY_F32)
    assert vr.BLOB_BYTES <= 160 * 1024  # one CU's LDS
    assert nat.ABI_VERSION == lib.swarm_abi_version() == 5


@pytest.mark.parametrize("args,code", [((0, 0), "ELIMIT"), ((48, 0), "ELIMIT"), ((0, 1), "ELIMIT"), ((48, 1), "ELIMIT"),
                                       ((-3, 0), "ELIMIT"), ((37, 2), "ELIMIT"), ((37, 7), "EINVAL")])
def test_bad_dims_return_a_code_and_a_message(nat, lib, args, code):
    want = getattr(nat, "SWARM_" + code)
    assert lib.swarm_value_packed_bytes(*args) == want
    assert lib.swarm_value_last_error()
    a = np.zeros(4, np.float32)
    fp = a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.swarm_value_pack(*args, fp, fp, fp, fp, fp, fp, a.ctypes.data) == want  # rejected before any read
    v = nat.SwarmValue(args[0], args[1], 4096)
    assert lib.swarm_value_forward(ctypes.byref(v), 16, 4, 16, None) == want  # and before any launch
    with pytest.raises(ValueError):
        nat.check(want, lib, which="value")


def test_null_arguments_and_empty_batches(nat, lib):
    for prec in (nat.POLICY_BF16, nat.POLICY_F32):
        assert lib.swarm_value_pack(15, prec, None, None, None, None, None, None, None) == nat.SWARM_ENULL
        assert b"null" in lib.swarm_value_last_error().lower()
        v = nat.SwarmValue(37, prec, None)
        assert lib.swarm_value_forward(None, None, 4, None, None) == nat.SWARM_ENULL
        assert lib.swarm_value_forward(ctypes.byref(v), None, 4, None, None) == nat.SWARM_ENULL
        v.weights = 4096
        assert lib.swarm_value_forward(ctypes.byref(v), None, -1, None, None) == nat.SWARM_EINVAL
        assert lib.swarm_value_forward(ctypes.byref(v), None, 0, None, None) == 0      # rows == 0: no-op
        assert lib.swarm_value_forward(ctypes.byref(v), None, 4, None, None) == nat.SWARM_ENULL
        assert lib.swarm_value_forward(ctypes.byref(v), 16, 4, None, None) == nat.SWARM_ENULL
        v.weights = 4100
        assert lib.swarm_value_forward(ctypes.byref(v), 16, 4, 16, None) == nat.SWARM_EINVAL  # 16-B alignment
    assert lib.swarm_gae_agent(None, None, None, None, None, None, 0, 4, 4, 0.99, 0.95, None, None, None) == 0
    assert lib.swarm_gae_agent(None, None, None, None, None, None, -1, 4, 4, 0.99, 0.95, None, None, None) == nat.SWARM_EINVAL
    assert lib.swarm_gae_agent(None, None, None, None, None, None, 2, 4, 4, 0.99, 0.95, None, None, None) == nat.SWARM_ENULL
    with pytest.raises(ValueError, match="NULL"):
        nat.check(nat.SWARM_ENULL, lib, which="value")


@pytest.mark.parametrize("in_dim", vr.IN_DIMS)
def test_bf16_blob_emulation_reproduces_direct_bf16(nat, lib, in_dim):
    layers = vr.make_value(in_dim)
    buf = vr.pack(lib, layers, nat.POLICY_BF16)
    x = vr.obs_like(37, in_dim, seed=in_dim)
    got = vr.emulate_bf16_blob(buf, x)
    ref = vr.direct_bf16(layers, x)
    # the same rounded operands summed in float64 in another order: only a sum within ~1e-15 of a
    # bf16 rounding tie could differ
    assert np.abs(got - ref).max() <= 1e-9, np.abs(got - ref).max()
    # and it is the value tower: within bf16's error of the float64 truth
    v64 = vr.truth64(layers, x)
    assert np.abs(got - v64).max() < 0.05 * max(1.0, np.abs(v64).max())
    # the pad columns past the bias column are zero, and the bias column holds b1
    w1 = vr.from_bf16(buf[:24 * 1024].view(np.uint16)).reshape(8, 3, 2, 32, 8)
    dense = np.zeros((256, 48), np.float32)
    for ks in range(3):
        for h in range(2):
            for j in range(8):
                dense[:, 16 * ks + 8 * h + j] = w1[:, ks, h, :, j].reshape(256)
    assert np.all(dense[:, in_dim + 1:] == 0)
    assert np.array_equal(dense[:, in_dim], vr.to_bf16(layers[0][1]))
    assert np.array_equal(dense[:, :in_dim], vr.to_bf16(layers[0][0]))
    # the permutations matter: W2 read without the chaining permutation is another function
    w2 = buf[24 * 1024:152 * 1024].view(np.uint16).reshape(8, 16, 2, 32, 8)
    plain = np.zeros((256, 256), np.uint16)
    for ks in range(16):
        for h in range(2):
            for j in range(8):
                plain[:, 16 * ks + 8 * h + j] = w2[:, ks, h, :, j].reshape(256)
    assert not np.array_equal(vr.from_bf16(plain), vr.to_bf16(layers[1][0]))


def test_f32_blob_is_the_critics(nat, lib):
    layers = vr.make_value(25)
    assert np.array_equal(vr.pack(lib, layers, nat.POLICY_F32), cr.pack(lib, layers, nat.POLICY_F32))


def _rllib_state_dict(d, prefix, seed):
    """RLlib TorchFC(vf_share_layers=False) parameter names: the actor's layers and the value tower."""
    actor = cr.make_critic(d, seed=seed + 1)
    tower = vr.make_value(d, seed=seed)
    rng = np.random.default_rng(seed)
    names = {"_hidden_layers.0._model.0": actor[0], "_hidden_layers.1._model.0": actor[1],
             "_logits._model.0": (rng.normal(0, 0.1, (6, 256)).astype(np.float32), np.zeros(6, np.float32)),
             "_value_branch_separate.0._model.0": tower[0], "_value_branch_separate.1._model.0": tower[1],
             "_value_branch._model.0": tower[2]}
    sd = {}
    for name, (w, b) in names.items():
        sd[prefix + name + ".weight"] = torch.from_numpy(w)
        sd[prefix + name + ".bias"] = torch.from_numpy(b)
    return sd, tower


@pytest.mark.parametrize("prefix", ["", "policy.model."])
def test_from_state_dict(prefix):
    from swarm_marl_amd import AgentValueMLP
    sd, tower = _rllib_state_dict(37, prefix, seed=3)
    v = AgentValueMLP.from_state_dict(sd, prefix=prefix, device="cpu")
    ref = AgentValueMLP.from_arrays(*[a for wb in tower for a in wb], device="cpu")
    assert v.in_dim == 37 and np.array_equal(v.packed_host, ref.packed_host)
    for (w, b), (rw, rb) in zip(v.layers, tower):
        assert np.array_equal(w, rw) and np.array_equal(b, rb)
    assert v.weights.data_ptr() % 16 == 0 and v.weights.numel() == vr.BLOB_BYTES
    # the tower's two hidden layers listed in the other order are still chained by shape
    rev = dict(reversed(list(sd.items())))
    assert np.array_equal(AgentValueMLP.from_state_dict(rev, prefix=prefix, device="cpu", precision="f32").layers[0][0],
                          tower[0][0])
    # the wrong prefix, a dict without the tower (vf_share_layers=True), an unsupported precision or width
    with pytest.raises(ValueError):
        AgentValueMLP.from_state_dict(sd, prefix="nothing.", device="cpu")
    shared = {k: t for k, t in sd.items() if "_value_branch_separate" not in k}
    with pytest.raises(ValueError):
        AgentValueMLP.from_state_dict(shared, prefix=prefix, device="cpu")
    with pytest.raises(ValueError):
        AgentValueMLP.from_arrays(*[a for wb in tower for a in wb], device="cpu", precision="f32x3")
    with pytest.raises(ValueError):
        AgentValueMLP.from_arrays(np.zeros((256, 48), np.float32), *[a for wb in tower for a in wb][1:], device="cpu")


def test_load_layers_repacks_in_place():
    from swarm_marl_amd import AgentValueMLP
    a, b = vr.make_value(25, seed=1), vr.make_value(25, seed=2)
    v = AgentValueMLP(a, device="cpu")
    ptr, before = v.weights.data_ptr(), v.packed_host.copy()
    v.load_layers(b)
    assert v.weights.data_ptr() == ptr and not np.array_equal(v.packed_host, before)
    assert np.array_equal(v.packed_host, AgentValueMLP(b, device="cpu").packed_host)
    assert np.array_equal(v.weights.numpy(), v.packed_host)
    with pytest.raises(ValueError):
        v.load_layers(vr.make_value(26))


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 3, 5), (16, 9, 7)])
def test_flag_generator_is_episode_consistent(shape):
    flags = vr.consistent_flags(*shape, seed=sum(shape))
    vr.check_consistent(*flags)
    if shape == (16, 9, 7):
        terminated, truncated, env_done, valid = flags
        assert (~valid).any() and terminated.any() and truncated.any()
        assert (env_done & vr.ENV_RESET).any() and ((env_done & 3) != 0).any()


@pytest.mark.parametrize("shape", [(5, 3, 5), (32, 9, 7)])
def test_f32_gae_agent_loop_tracks_float64(shape):
    args = vr.random_gae_agent_inputs(*shape, seed=sum(shape))
    a32, t32 = vr.gae_agent_loop(*args, 0.99, 0.95, dtype=np.float32)
    a64, t64 = vr.gae_agent_loop(*args, 0.99, 0.95, dtype=np.float64)
    assert a32.dtype == np.float32 and a64.dtype == np.float64
    tol = 1e-5 * max(1.0, np.abs(a64).max(), np.abs(t64).max())
    assert np.abs(a32 - a64).max() <= tol and np.abs(t32 - t64).max() <= tol
    valid = args[5]
    assert np.all(a32[~valid] == 0) and np.all(t32[~valid] == 0)
    # values the loop must not read may be NaN: the same bits come out
    poisoned = vr.poison_unread_values(args[1], *args[2:])
    assert np.isnan(poisoned).any()
    ap, tp = vr.gae_agent_loop(args[0], poisoned, *args[2:], 0.99, 0.95, dtype=np.float32)
    assert np.array_equal(ap.view(np.uint32), a32.view(np.uint32)) and np.array_equal(tp.view(np.uint32), t32.view(np.uint32))


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (0.9, 0.0)])
def test_gae_agent_loop_on_broadcast_values_is_the_env_loop(gamma, lam):
    reward, value, terminated, truncated, env_done, valid = cr.random_gae_inputs(9, 6, 5, seed=8)
    wide = np.ascontiguousarray(np.broadcast_to(value[:, :, None], (10, 6, 5)))
    a_ref, t_ref = cr.gae_loop(reward, value, terminated, truncated, env_done, valid, gamma, lam, dtype=np.float32)
    a, t = vr.gae_agent_loop(reward, wide, terminated, truncated, env_done, valid, gamma, lam, dtype=np.float32)
    assert np.array_equal(a.view(np.uint32), a_ref.view(np.uint32)) and np.array_equal(t.view(np.uint32), t_ref.view(np.uint32))
