"""CPU: the attention actor's references, packer, torch module and argument validation.  No kernel is
launched: the packer is host code, and every rejected call returns before touching the GPU.

* tests/attn_ref.py forward64 against a torch float64 module of the reference's structure
  (nn.MultiheadAttention(32, 1, batch_first=True)) built here, and against AttentionActor.double():
  <= 1e-12 (both measured <= 5e-16);
* the packer's folded matrices, read back from the bf16 blob, against the float64 folds rounded the
  way the header says (A, c0 to f32; the folded first layer to f32 then bf16): exact;
* state_dict names, validation errors, the struct layouts against the header;
* the premises of the GPU tests' fixtures: the saturated softmax fixture (its row count, score span
  and gap, monotone slot orders, order-independent reference), `q_scale`, the log-std range of the
  sampling fixtures at attn_ref.MORE_SHAPES.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import attn_ref as ar

ROOT = Path(__file__).resolve().parents[1]

REFERENCE_NAMES = ar.NAMES + tuple(f"action_model.{layer}._model.0.{part}"
                                   for layer in ("_hidden_layers.0", "_hidden_layers.1", "_logits")
                                   for part in ("weight", "bias"))


def _state_dict(params, layers):
    sd = {n: torch.from_numpy(params[n]) for n in ar.NAMES}
    for key, a in zip(REFERENCE_NAMES[len(ar.NAMES):], (a for wb in layers for a in wb)):
        sd[key] = torch.from_numpy(a)
    return sd


class _TorchReference(torch.nn.Module):
    """The reference's actor written out on torch modules (float64 in the tests)."""

    def __init__(self, params, layers, k):
        super().__init__()
        self.k = k
        self.nb = torch.nn.Linear(4, 32)
        self.own = torch.nn.Linear(9, 32)
        self.attn = torch.nn.MultiheadAttention(32, 1, batch_first=True)
        self.fc = torch.nn.ModuleList([torch.nn.Linear(w.shape[1], w.shape[0]) for w, _ in layers])
        with torch.no_grad():
            for dst, name in ((self.nb.weight, ar.NAMES[0]), (self.nb.bias, ar.NAMES[1]), (self.own.weight, ar.NAMES[2]),
                              (self.own.bias, ar.NAMES[3]), (self.attn.in_proj_weight, ar.NAMES[4]),
                              (self.attn.in_proj_bias, ar.NAMES[5]), (self.attn.out_proj.weight, ar.NAMES[6]),
                              (self.attn.out_proj.bias, ar.NAMES[7])):
                dst.copy_(torch.from_numpy(params[name]))
            for lin, (w, b) in zip(self.fc, layers):
                lin.weight.copy_(torch.from_numpy(w))
                lin.bias.copy_(torch.from_numpy(b))
        self.eval()

    def forward(self, obs):
        k = self.k
        own = obs[:, :9]
        e = torch.relu(self.nb(obs[:, 9:9 + 4 * k].reshape(-1, k, 4)))
        o = torch.relu(self.own(own)).unsqueeze(1)
        ctx, _ = self.attn(o, e, e)
        h = torch.cat([own, ctx.squeeze(1), obs[:, 9 + 4 * k:]], dim=1)
        return self.fc[2](torch.relu(self.fc[1](torch.relu(self.fc[0](h)))))


@pytest.mark.parametrize("k,ms,out", ar.SHAPES + ar.MORE_SHAPES)
def test_reference_matches_torch_float64(k, ms, out):
    from swarm_marl_amd import AttentionActor
    params, layers = ar.make_attn(k, ms, out)
    for name in ("attn_block.attn.in_proj_bias", "attn_block.attn.out_proj.bias"):
        assert np.abs(params[name]).min() > 0  # bk, bv, bout are exercised
    x = ar.obs_set(k, ms)
    ref = ar.forward64(params, layers, k, x)
    xt = torch.from_numpy(x).double()
    with torch.no_grad():
        want = _TorchReference(params, layers, k).double()(xt).numpy()
        actor = AttentionActor(k, ms, out)
        actor.load_state_dict(_state_dict(params, layers))
        got = actor.double()(xt).numpy()
    print(f"K={k} Ms={ms} out={out}: ref - torch {np.abs(ref - want).max():.2e}, actor - ref {np.abs(got - ref).max():.2e}")
    assert np.abs(ref - want).max() <= 1e-12
    assert np.abs(got - ref).max() <= 1e-12


def test_folds_are_exact_identities():
    """The folded forward (no rounding) is the unfolded one: scores up to a per-row constant, the
    first layer's pre-activation exactly."""
    k, ms, out = 3, 4, 6
    params, layers = ar.make_attn(k, ms, out)
    x = ar.obs_set(k, ms)
    p, f = ar._f64(params), ar.folds64(params, layers)
    own, nb, obst = ar._split(x, k)
    o = np.maximum(own @ p["wown"].T + p["bown"], 0)
    e = np.maximum(nb @ p["wnb"].T + p["bnb"], 0)
    _, score, a = ar.forward64(params, layers, k, x, details=True)
    folded = np.einsum("ri,rji->rj", o @ f["A"].T + f["c0"], e)
    diff = score - folded
    assert np.abs(diff - diff[:, :1]).max() <= 1e-12  # equal up to a j-constant
    s = np.einsum("rj,rji->ri", a, e)
    c = np.einsum("rj,rji->ri", a, e @ p["wv"].T + p["bv"]) @ p["wout"].T + p["bout"]
    w1c = layers[0][0][:, 9:41].astype(np.float64)
    assert np.abs(c @ w1c.T - (s @ f["F"].T + f["d"])).max() <= 1e-12


@pytest.mark.parametrize("k,ms,out", ar.SHAPES + ar.MORE_SHAPES)
def test_packer_folds_match_float64(k, ms, out):
    from swarm_marl_amd.attention import AttentionPolicy, unpack_bf16_blob
    params, layers = ar.make_attn(k, ms, out)
    pol = AttentionPolicy(params, layers, neighbor_k=k, sensed_obstacles=ms, device="cpu")
    got = unpack_bf16_blob(pol.packed_host, out)
    f = ar.folds64(params, layers)
    assert np.array_equal(got["A"], f["A"].astype(np.float32))
    assert np.array_equal(got["c0"], f["c0"].astype(np.float32))
    assert np.array_equal(got["own_w"], params["own_embed.0.weight"])
    assert np.array_equal(got["own_b"], params["own_embed.0.bias"])
    assert np.array_equal(got["neighbor_w"], params["neighbor_embed.0.weight"])
    assert np.array_equal(got["neighbor_b"], params["neighbor_embed.0.bias"])
    want = ar.bf16(ar.folded_w1(params, layers, ms))
    # a float64 sum in another order may land on the far side of a rounding tie: allow one bf16 ulp
    # on at most a handful of the 16384 entries, none elsewhere
    diff = np.abs(got["w1"].astype(np.float64) - want)
    ulp = np.maximum(np.abs(want), 2.0 ** -126) * 2.0 ** -7
    assert (diff <= ulp).all()
    assert (diff > 0).sum() <= 8, (diff > 0).sum()
    # the trunk's other layers: the bf16 blob holds bf16(W2), bf16(W3) in fragment order, b2 / b3 as f32
    b2_off = 131072 + 512 * out
    assert np.array_equal(pol.packed_host[b2_off:b2_off + 1024].view(np.float32), layers[1][1])
    assert np.array_equal(pol.packed_host[b2_off + 1024:b2_off + 1024 + 4 * out].view(np.float32), layers[2][1])


def test_q_scale_touches_the_query_third_only():
    k, ms, out = ar.SAT_SHAPE
    p0, l0 = ar.make_attn(k, ms, out, seed_offset=1)
    p1, l1 = ar.make_saturated()
    for name in ar.NAMES[4:6]:
        assert np.array_equal(p1[name][:32], p0[name][:32] * np.float32(ar.SAT_Q_SCALE))
        assert np.array_equal(p1[name][32:], p0[name][32:])  # Wk, Wv, bk, bv as they were
    for name in ar.NAMES[:4] + ar.NAMES[6:]:
        assert np.array_equal(p1[name], p0[name])
    for (w1, b1), (w0, b0) in zip(l1, l0):
        assert np.array_equal(w1, w0) and np.array_equal(b1, b0)
    f0, f1 = ar.folds64(p0, l0), ar.folds64(p1, l1)
    assert np.array_equal(f1["F"], f0["F"]) and np.array_equal(f1["d"], f0["d"])  # the folded first layer keeps its size
    # the score matrix grows 144-fold (Wq x 144 is rounded to f32: 2^-24 per product, against the largest entry)
    assert np.abs(f1["A"] - ar.SAT_Q_SCALE * f0["A"]).max() <= 1e-6 * np.abs(f1["A"]).max()


def test_saturated_fixture_premises():
    """What tests/test_gpu_attn_shapes.py::test_saturated_softmax_in_score_order relies on."""
    k, ms, out = ar.SAT_SHAPE
    params, layers = ar.make_saturated()
    x, score = ar.saturated_rows(params, layers)
    assert len(x) >= ar.SAT_ROWS == 97
    assert len(ar.saturated_rows(params, layers, pool=4096)[0]) == 71  # 8192 is the smallest power of two that serves
    srt = np.sort(score, axis=1)
    assert (srt[:, -1] - srt[:, 0]).min() > 104 and (srt[:, -1] - srt[:, -2]).min() > 30
    assert np.exp(np.float32(-104.0)) == 0  # f32: the lowest slot's weight underflows
    var = ar.saturated_variants(params, layers)
    refs = {}
    for name, xv in var.items():
        assert xv.shape == (97, 93) and xv.dtype == np.float32
        refs[name], sc, a = ar.forward64(params, layers, k, xv, details=True)
        assert np.array_equal(np.sort(sc, axis=1), srt)  # a slot's score does not depend on its position
        assert a.max(axis=1).min() > 1 - 1e-12
        if name == "ascending":
            assert np.all(np.diff(sc, axis=1) > 0)
        if name == "descending":
            assert np.all(np.diff(sc, axis=1) < 0)
        assert np.array_equal(xv[:, :9], x[:, :9]) and np.array_equal(xv[:, 9 + 4 * k:], x[:, 9 + 4 * k:])
    assert np.array_equal(var["drawn"], x)
    assert not np.array_equal(var["ascending"], x) and not np.array_equal(var["descending"], x)
    assert np.array_equal(var["ascending"][:, 9:9 + 4 * k].reshape(97, k, 4)[:, ::-1],
                          var["descending"][:, 9:9 + 4 * k].reshape(97, k, 4))
    spread = max(np.abs(refs[n] - refs["drawn"]).max() for n in ("ascending", "descending"))
    print(f"saturated: scores up to {score.max():.1f}, span up to {(srt[:, -1] - srt[:, 0]).max():.1f}, "
          f"variants' ref64 within {spread:.1e} (bound 1e-12)")
    assert spread <= 1e-12


@pytest.mark.parametrize("k,ms,out", [(3, 4, 6), (16, 5, 12)] + list(ar.MORE_SHAPES))
def test_sampling_fixtures_keep_log_std_in_range(k, ms, out):
    """The premise of test_sampling_with_real_weights (-2 <= log_std <= 0.5), on both references."""
    params, layers = ar.make_attn(k, ms, out, log_std_scale=0.25)
    x = ar.obs_set(k, ms)
    for lg in (ar.forward64(params, layers, k, x), ar.forward_bf16_emu(params, layers, k, ms, x)):
        ls = lg[:, out // 2:]
        assert -2.0 + 0.1 <= ls.min() and ls.max() <= 0.5 - 0.1, (ls.min(), ls.max())


def test_state_dict_names_and_round_trip():
    from swarm_marl_amd import AttentionActor, AttentionPolicy
    from swarm_marl_amd.attention import STATE_DICT_KEYS
    k, ms, out = 3, 4, 6
    actor = AttentionActor(k, ms, out)
    assert tuple(actor.state_dict().keys()) == REFERENCE_NAMES == STATE_DICT_KEYS
    params, layers = ar.make_attn(k, ms, out)
    sd = _state_dict(params, layers)
    sd["value_model._logits._model.0.weight"] = torch.zeros(1, 256)  # the critic's entries are ignored
    pol = AttentionPolicy.from_state_dict(sd, neighbor_k=k, sensed_obstacles=ms, device="cpu", precision="f32")
    assert (pol.in_dim, pol.out_dim, pol.precision, pol.device) == (37, 6, "f32", torch.device("cpu"))
    for n in ar.NAMES:
        assert pol.params[n].dtype == np.float32 and np.array_equal(pol.params[n], params[n])
    for (w, b), (w0, b0) in zip(pol.layers, layers):
        assert np.array_equal(w, w0) and np.array_equal(b, b0)
    back = AttentionActor.from_policy(pol).state_dict()
    for key in REFERENCE_NAMES:
        assert torch.equal(back[key], sd[key]), key
    with pytest.raises(ValueError, match="lacks"):
        AttentionPolicy.from_state_dict({n: sd[n] for n in ar.NAMES}, neighbor_k=k, sensed_obstacles=ms, device="cpu")


def test_load_params_repacks_in_place():
    from swarm_marl_amd import AttentionPolicy
    k, ms, out = 2, 1, 6
    params, layers = ar.make_attn(k, ms, out)
    pol = AttentionPolicy(params, layers, neighbor_k=k, sensed_obstacles=ms, device="cpu")
    before, ptr = pol.packed_host.copy(), pol.weights.data_ptr()
    p2, l2 = ar.make_attn(k, ms, out, seed_offset=3)
    pol.load_params(p2, l2)
    fresh = AttentionPolicy(p2, l2, neighbor_k=k, sensed_obstacles=ms, device="cpu")
    assert not np.array_equal(pol.packed_host, before)
    assert np.array_equal(pol.packed_host, fresh.packed_host)
    assert np.array_equal(pol.weights.numpy(), fresh.packed_host) and pol.weights.data_ptr() == ptr
    with pytest.raises(ValueError):
        pol.load_params(p2, ar.make_attn(k, ms + 1, out)[1])  # another trunk width
    assert np.array_equal(pol.params[ar.NAMES[0]], p2[ar.NAMES[0]])  # a rejected load leaves the policy as it was


@pytest.mark.parametrize("k,ms,out,word", [(0, 4, 6, "neighbor_k"), (17, 4, 6, "neighbor_k"),
                                           (3, 6, 6, "sensed_obstacles"), (3, -1, 6, "sensed_obstacles"),
                                           (3, 4, 5, "out_dim"), (3, 4, 14, "out_dim"), (3, 4, 0, "out_dim")])
def test_limits_are_named(k, ms, out, word):
    from swarm_marl_amd import AttentionPolicy
    from swarm_marl_amd import _native as nat
    lib = nat.load_library()
    for prec in (nat.POLICY_BF16, nat.POLICY_F32):
        assert lib.swarm_attn_policy_packed_bytes(k, ms, out, prec) == nat.SWARM_ELIMIT
        assert word.encode() in lib.swarm_attn_policy_last_error()
    c = nat.SwarmAttnPolicy(k, ms, out, nat.POLICY_BF16, 256)
    assert lib.swarm_attn_policy_forward(ctypes.byref(c), 256, 4, 256, None, 0, 0, 0, None) == nat.SWARM_ELIMIT
    if out > 0 and ms >= 0:
        params, layers = ar.make_attn(max(k, 1), min(ms, 5), max(out, 2))
        layers[2] = (np.zeros((out, 256), np.float32), np.zeros(out, np.float32))
        with pytest.raises(ValueError, match=word):
            AttentionPolicy(params, layers, neighbor_k=k, sensed_obstacles=ms, device="cpu")


def test_other_validation_errors():
    from swarm_marl_amd import AttentionPolicy
    from swarm_marl_amd import _native as nat
    lib = nat.load_library()
    assert lib.swarm_attn_policy_packed_bytes(3, 4, 6, nat.POLICY_F32X3) == nat.SWARM_ELIMIT
    assert b"f32x3" in lib.swarm_attn_policy_last_error()
    assert lib.swarm_attn_policy_packed_bytes(3, 4, 6, 9) == nat.SWARM_EINVAL
    assert lib.swarm_attn_policy_packed_bytes(3, 4, 6, nat.POLICY_BF16) == 131072 + 512 * 6 + 1024 + 128 + 32768 + 6144
    host = np.zeros(200000, np.uint8)
    assert lib.swarm_attn_policy_pack(3, 4, 6, nat.POLICY_BF16, None, host.ctypes.data_as(ctypes.c_void_p)) == nat.SWARM_ENULL
    w = nat.SwarmAttnWeights()  # every pointer NULL
    assert lib.swarm_attn_policy_pack(3, 4, 6, nat.POLICY_BF16, ctypes.byref(w),
                                      host.ctypes.data_as(ctypes.c_void_p)) == nat.SWARM_ENULL
    # forward: rejected before any launch; rows == 0 is a no-op
    c = nat.SwarmAttnPolicy(3, 4, 6, nat.POLICY_BF16, 256)
    fwd = lib.swarm_attn_policy_forward
    assert fwd(None, 256, 4, 256, None, 0, 0, 0, None) == nat.SWARM_ENULL
    assert fwd(ctypes.byref(nat.SwarmAttnPolicy(3, 4, 6, nat.POLICY_BF16, None)), 256, 4, 256, None, 0, 0, 0, None) == nat.SWARM_ENULL
    assert fwd(ctypes.byref(c), 256, -1, 256, None, 0, 0, 0, None) == nat.SWARM_EINVAL
    assert fwd(ctypes.byref(c), None, 0, None, None, 0, 0, 0, None) == nat.SWARM_OK
    assert fwd(ctypes.byref(c), None, 4, 256, None, 0, 0, 0, None) == nat.SWARM_ENULL
    assert fwd(ctypes.byref(c), 256, 4, None, None, 0, 0, 0, None) == nat.SWARM_ENULL
    assert fwd(ctypes.byref(c), 256, 4, 256, None, 7, 0, 0, None) == nat.SWARM_EINVAL
    assert fwd(ctypes.byref(nat.SwarmAttnPolicy(3, 4, 6, nat.POLICY_BF16, 264)), 256, 4, 256, None, 0, 0, 0, None) == nat.SWARM_EINVAL
    assert fwd(ctypes.byref(nat.SwarmAttnPolicy(3, 4, 6, nat.POLICY_F32X3, 256)), 256, 4, 256, None, 0, 0, 0, None) == nat.SWARM_ELIMIT
    with pytest.raises(ValueError):
        nat.check(nat.SWARM_ELIMIT, lib, which="attn")
    # python: shapes and precision
    params, layers = ar.make_attn(3, 4, 6)
    kw = dict(neighbor_k=3, sensed_obstacles=4, device="cpu")
    with pytest.raises(ValueError, match="precision"):
        AttentionPolicy(params, layers, precision="f32x3", **kw)
    with pytest.raises(ValueError, match="missing"):
        AttentionPolicy({n: params[n] for n in ar.NAMES[1:]}, layers, **kw)
    bad = dict(params)
    bad[ar.NAMES[4]] = params[ar.NAMES[4]][:64]
    with pytest.raises(ValueError, match="in_proj_weight"):
        AttentionPolicy(bad, layers, **kw)
    with pytest.raises(ValueError, match="trunk"):
        AttentionPolicy(params, layers[:2], **kw)
    with pytest.raises(ValueError, match="trunk"):
        AttentionPolicy(params, ar.make_attn(3, 3, 6)[1], **kw)  # W1 of another Ms
    pol = AttentionPolicy(params, layers, **kw)
    with pytest.raises(ValueError):
        pol.logits(torch.zeros(4, 36))  # wrong width


def test_learner_rejects_other_policies():
    from swarm_marl_amd import PPOLearner
    with pytest.raises(ValueError, match="PPOLearner needs a PolicyMLP and a CriticMLP"):
        PPOLearner(object(), object(), minibatch_env_rows=4)


@pytest.mark.parametrize("ctype,cname", [("SwarmAttnPolicy", "swarm_attn_policy_t"),
                                         ("SwarmAttnWeights", "swarm_attn_weights_t")])
def test_attn_struct_layouts_match_header(tmp_path, ctype, cname):
    from swarm_marl_amd import _native as nat
    cls = getattr(nat, ctype)
    fields = [f for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "swarm_mi355x.h"', "int main(void) {",
             f'printf("%zu\\n", sizeof({cname}));']
    lines += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f in fields]
    lines += ['printf("%d %d %d\\n", SWARM_ATTN_EMBED, SWARM_ATTN_MAX_K, SWARM_ATTN_MAX_MS);', "return 0; }"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(cls)
    assert out[1:-3] == [getattr(cls, f).offset for f in fields]
    assert out[-3:] == [nat.ATTN_EMBED, nat.ATTN_MAX_K, nat.ATTN_MAX_MS]


def test_symbol_groups_keep_their_names():
    from swarm_marl_amd import _native as nat
    assert nat.ROLLOUT_SYMBOLS == ("swarm_critic_packed_bytes", "swarm_critic_pack", "swarm_critic_forward",
                                   "swarm_critic_last_error", "swarm_gaussian_logp", "swarm_gae")
    assert nat.PPO_SYMBOLS == ("swarm_masked_moments", "swarm_ppo_loss", "swarm_ppo_last_error")
    assert nat.ATTN_SYMBOLS == ("swarm_attn_policy_packed_bytes", "swarm_attn_policy_pack",
                                "swarm_attn_policy_forward", "swarm_attn_policy_last_error")
    assert nat.ABI_VERSION == 5
