"""GPU: the attention actor's kernels (csrc/swarm_attn.hip) on the code tests/test_gpu_attn.py never
executes.  References, helpers and bounds are that module's (check_f32, check_bf16, _guarded, _case);
no tolerance is new.

* more than one workgroup and more than one trip through the grid-stride loop: the 257-row fixture
  repeated on the device (row r is fixture row r mod 257; 257 is prime, so every 64-row group sees it
  at another phase).  MID = 1633 rows: four bf16 workgroups, the last with a full group, a 32 + 1 row
  group and six idle waves.  BIG_BF16 = 512 CUs + 97 and BIG_F32 = 32 CUs + 13 rows: one past the rows
  of one pass of either kernel's grid, so the second trip holds a full group and a 33-row one (bf16)
  or one 8-row block and a 5-row one (f32).  The sampled launch's recovered normals against
  sample_noise64 over all rows are what sees a row index lost between trips;
* the one-pass softmax (bf16) with the slots of every row in ascending and in descending score on a
  saturated fixture (attn_ref.saturated_variants: K = 16, span > 104, top - second > 30);
* rows do not leak: NaN / +inf / -inf rows leave every other row bitwise as in the clean launch;
* obs, logits and actions as views one float off their storage; a launch on a side stream;
* RolloutCollector on the bf16 sampling actor.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import attn_ref as ar
from tests import policy_ref as pr
from tests.test_gpu_attn import (E, GUARD, N, SENTINEL, _case, _guarded, _policy, _rollout, check_bf16,
                                 check_f32)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guards_hold(buf, n, tag):
    assert torch.all(buf[n:] == SENTINEL), tag   # nothing past the output
    assert torch.all(buf[:n] != SENTINEL), tag   # every element written


def _check(precision, got, emu, ref, tag):
    if precision == "f32":
        check_f32(got, ref, tag)
    else:
        check_bf16(got, emu, ref, tag)


def _recovered_normals(lg, ac, ad):
    lgn, acn = lg.cpu().numpy().astype(np.float64), ac.cpu().numpy().astype(np.float64)
    mean, ls = lgn[:, :ad], lgn[:, ad:]
    assert ls.min() >= -2.0 and ls.max() <= 0.5, (ls.min(), ls.max())
    return (acn - mean) / np.exp(ls)


# ---------------------------------------------------------------- workgroups and grid passes
MID = 8 * 64 * 3 + 64 + 33  # 1633: 4 bf16 workgroups (26 groups of 64), 205 f32 workgroups


def _rows(dev, which):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count  # what the kernels size their grids from
    return {"mid": MID, "big_f32": cus * 32 + 13, "big_bf16": cus * 512 + 97}[which], cus


@pytest.mark.parametrize("which", ["mid", "big_f32", "big_bf16"])
@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("k,ms,out", [(16, 5, 12), (3, 4, 6)])
def test_more_than_one_workgroup_and_grid_pass(dev, precision, k, ms, out, which):
    rows, cus = _rows(dev, which)
    if which == "mid":
        assert 3 * 512 < rows <= 4 * 512 < cus * 512 and (rows - 3 * 512) == 64 + 32 + 1
    elif which == "big_" + precision:  # the premise: one pass of this kernel's grid does not reach the last rows
        assert rows > cus * (512 if precision == "bf16" else 32)
    params, layers, x, ref, emu = _case(k, ms, out, log_std_scale=0.25)
    pol = _policy(dev, params, layers, k, ms, precision)
    ad = out // 2
    big = torch.tensor(x).to(dev)[torch.arange(rows, device=dev) % ar.ROWS]
    assert big.is_contiguous() and big.shape == (rows, pol.in_dim)
    idx = np.arange(rows) % ar.ROWS
    tag = f"{which} K={k} Ms={ms} out={out} rows={rows} ({cus} CUs)"

    lbuf, lg = _guarded(dev, rows, out)
    abuf, ac = _guarded(dev, rows, ad)
    pol.forward(big, logits=lg, actions=ac)
    _guards_hold(lbuf, rows * out, tag)
    _guards_hold(abuf, rows * ad, tag)
    _check(precision, lg.cpu().numpy(), emu[idx], ref[idx], tag)
    assert torch.equal(_bits(ac), _bits(lg[:, :ad])), tag

    lbuf2, lg2 = _guarded(dev, rows, out)
    abuf2, ac2 = _guarded(dev, rows, ad)
    pol.forward(big, logits=lg2, actions=ac2)
    assert torch.equal(lbuf2.view(torch.int32), lbuf.view(torch.int32)), tag
    assert torch.equal(abuf2.view(torch.int32), abuf.view(torch.int32)), tag

    lbuf3, lg3 = _guarded(dev, rows, out)
    abuf3, ac3 = _guarded(dev, rows, ad)
    pol.forward(big, logits=lg3, actions=ac3, sample=True, seed=99, counter=17)
    _guards_hold(lbuf3, rows * out, tag)
    _guards_hold(abuf3, rows * ad, tag)
    assert torch.equal(lbuf3.view(torch.int32), lbuf.view(torch.int32)), tag  # sampling leaves the logits alone
    z = _recovered_normals(lg3, ac3, ad)
    err = np.abs(z - pr.sample_noise64(rows, ad, 99, 17)).max(axis=1)
    print(f"sample {precision} {tag}: max |z - z_ref| {err.max():.3e} (bound 1e-5)")
    assert err.max() <= 1e-5, (tag, int(np.argmax(err > 1e-5)))


# ---------------------------------------------------------------- slot order on a saturated softmax
def test_saturated_softmax_in_score_order(dev):
    """Every neighbour raises the running maximum and exp(old - new) underflows to 0 (ascending), or
    every later p underflows (descending): K = 16, scores up to 171, span up to 243.  The top slot
    is > 30 above the second, so s is the top slot's embedding to f32 precision in any order."""
    k, ms, out = ar.SAT_SHAPE
    params, layers, _, _, _ = _case(k, ms, out, seed_offset=1, q_scale=ar.SAT_Q_SCALE)
    var = ar.saturated_variants(params, layers)
    refs, emus = {}, {}
    for name, x in var.items():
        assert len(x) == ar.SAT_ROWS == 97, (name, len(x))  # short: enlarge the pool, the thresholds stay
        refs[name], score, _ = ar.forward64(params, layers, k, x, details=True)
        emus[name] = ar.forward_bf16_emu(params, layers, k, ms, x)
        srt = np.sort(score, axis=1)
        assert (srt[:, -1] - srt[:, 0]).min() > 104 and (srt[:, -1] - srt[:, -2]).min() > 30
        if name == "ascending":
            assert np.all(np.diff(score, axis=1) > 0)
        if name == "descending":
            assert np.all(np.diff(score, axis=1) < 0)
    spread = max(np.abs(refs[n] - refs["drawn"]).max() for n in var)
    print(f"saturated: the variants' ref64 within {spread:.1e} of each other (bound 1e-12)")
    assert spread <= 1e-12
    for precision in ("f32", "bf16"):
        pol = _policy(dev, params, layers, k, ms, precision)
        got = {}
        for name, x in var.items():
            got[name] = pol.logits(torch.tensor(x).to(dev)).cpu().numpy()
            _check(precision, got[name], emus[name], refs[name], f"saturated {name}")
        if precision == "bf16":  # a slot's score does not depend on its position: only the rescales' order differs
            for a, b in (("drawn", "ascending"), ("drawn", "descending"), ("ascending", "descending")):
                d = np.abs(got[a].astype(np.float64) - got[b]).max()
                print(f"saturated bf16 {a} vs {b}: max diff {d:.3e} (bound 1e-3)")
                assert d <= 1e-3, (a, b, d)


# ---------------------------------------------------------------- rows are independent
POISONED = {33: (0, 31, 32), 257: (0, 31, 32, 63, 64, 256)}  # tile and group edges; the last row, which tail lanes repeat


@pytest.mark.parametrize("rows", [33, 257])
@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("k,ms,out", [(16, 5, 12), (6, 0, 2)])
def test_rows_do_not_leak(dev, precision, k, ms, out, rows):
    params, layers, x0, _, _ = _case(k, ms, out, log_std_scale=0.25)
    pol = _policy(dev, params, layers, k, ms, precision)
    ad = out // 2
    x = x0[:rows].copy()
    for i, r in enumerate(POISONED[rows]):
        x[r] = (np.nan, np.inf, -np.inf)[i % 3]
    assert POISONED[rows][-1] == rows - 1
    keep = torch.tensor(np.setdiff1d(np.arange(rows), POISONED[rows]), device=dev)

    def run(obs, sample):
        lbuf, lg = _guarded(dev, rows, out)
        abuf, ac = _guarded(dev, rows, ad)
        pol.forward(torch.tensor(obs).to(dev), logits=lg, actions=ac, sample=sample, seed=21, counter=4)
        _guards_hold(lbuf, rows * out, (precision, rows, sample))
        _guards_hold(abuf, rows * ad, (precision, rows, sample))
        return lg, ac

    for sample in (False, True):
        lg0, ac0 = run(x0[:rows], sample)
        assert torch.isfinite(lg0).all() and torch.isfinite(ac0).all()
        lg1, ac1 = run(x, sample)
        assert torch.equal(_bits(lg1[keep]), _bits(lg0[keep])), (precision, rows, sample)
        assert torch.equal(_bits(ac1[keep]), _bits(ac0[keep])), (precision, rows, sample)
        if sample:
            assert not torch.equal(_bits(ac0), _bits(lg0[:, :ad]))


# ---------------------------------------------------------------- offsets and streams
@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("k,ms,out", [(16, 5, 12), (3, 4, 6)])  # D = 93, 37: rows are 4-byte aligned at best anyway
def test_views_one_float_off_their_storage(dev, precision, k, ms, out):
    params, layers, x, _, _ = _case(k, ms, out, log_std_scale=0.25)
    pol = _policy(dev, params, layers, k, ms, precision)
    ad, rows, d = out // 2, ar.ROWS, pol.in_dim
    xt = torch.tensor(x).to(dev)
    obuf = torch.zeros(rows * d + 1, device=dev)
    xv = obuf[1:].view(rows, d)
    xv.copy_(xt)

    def off_by_one(width):  # [GUARD + 1 sentinels | rows x width | GUARD sentinels]
        buf = torch.full((GUARD + 1 + rows * width + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        return buf, buf[GUARD + 1:GUARD + 1 + rows * width].view(rows, width)

    for sample in (False, True):
        kw = dict(sample=sample, seed=8, counter=2)
        lg0 = torch.empty((rows, out), device=dev)
        ac0 = torch.empty((rows, ad), device=dev)
        pol.forward(xt, logits=lg0, actions=ac0, **kw)
        lbuf, lg = off_by_one(out)
        abuf, ac = off_by_one(ad)
        for t in (xv, lg, ac):
            assert t.is_contiguous() and t.data_ptr() % 8 == 4  # 4-byte aligned only
        assert lg0.data_ptr() % 16 == 0 and ac0.data_ptr() % 16 == 0 and xt.data_ptr() % 16 == 0
        pol.forward(xv, logits=lg, actions=ac, **kw)
        for buf, n in ((lbuf, rows * out), (abuf, rows * ad)):
            assert torch.all(buf[:GUARD + 1] == SENTINEL) and torch.all(buf[GUARD + 1 + n:] == SENTINEL), (precision, sample)
            assert torch.all(buf[GUARD + 1:GUARD + 1 + n] != SENTINEL)
        assert torch.equal(_bits(lg), _bits(lg0)), (precision, sample)
        assert torch.equal(_bits(ac), _bits(ac0)), (precision, sample)


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_side_stream(dev, precision):
    k, ms, out = 16, 5, 12
    params, layers, x, _, _ = _case(k, ms, out, log_std_scale=0.25)
    pol = _policy(dev, params, layers, k, ms, precision)
    ad, rows = out // 2, ar.ROWS
    xt = torch.tensor(x).to(dev)
    for sample in (False, True):
        kw = dict(sample=sample, seed=8, counter=2)
        lbuf0, lg0 = _guarded(dev, rows, out)
        abuf0, ac0 = _guarded(dev, rows, ad)
        pol.forward(xt, logits=lg0, actions=ac0, **kw)
        lbuf, lg = _guarded(dev, rows, out)
        abuf, ac = _guarded(dev, rows, ad)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))  # the inputs were produced on the current stream
        with torch.cuda.stream(side):
            assert torch.cuda.current_stream(dev) == side
            pol.forward(xt, logits=lg, actions=ac, **kw)
        side.synchronize()
        assert torch.equal(lbuf.view(torch.int32), lbuf0.view(torch.int32)), (precision, sample)
        assert torch.equal(abuf.view(torch.int32), abuf0.view(torch.int32)), (precision, sample)
        _guards_hold(lbuf, rows * out, (precision, sample))
        _guards_hold(abuf, rows * ad, (precision, sample))


# ---------------------------------------------------------------- the collector on the bf16 sampling actor
def test_collector_with_bf16_attention_policy(dev):
    """The path the project means to run: bf16, sampling, from RolloutCollector (E = 8, N = 4, horizon 3)."""
    col, policy, _, params, layers = _rollout(dev, 3, precision="bf16")
    assert policy.precision == "bf16"
    batch = col.collect()
    assert batch["obs"].shape == (3, E, N, 37) and batch["logits"].shape == (3, E, N, 6)
    for t in range(3):
        assert torch.equal(_bits(batch["logits"][t]), _bits(policy.logits(batch["obs"][t])))
    obs = batch["obs"].cpu().numpy().reshape(-1, 37)
    ref = ar.forward64(params, layers, 3, obs)
    emu = ar.forward_bf16_emu(params, layers, 3, 4, obs)
    lg = batch["logits"].cpu().numpy().reshape(-1, 6)
    check_bf16(lg, emu, ref, "bf16 collector logits")
    lg = lg.astype(np.float64)
    act = batch["actions"].cpu().numpy().reshape(-1, 3).astype(np.float64)
    assert np.abs(act - lg[:, :3]).max() > 1e-2  # sampled, not the mean
    z1 = _recovered_normals(batch["logits"][1].reshape(-1, 6), batch["actions"][1].reshape(-1, 3), 3)
    err = np.abs(z1 - pr.sample_noise64(E * N, 3, 3, 1)).max()  # step 1: seed 3, counter 1
    print(f"bf16 collector step 1: max |z - z_ref| {err:.3e} (bound 1e-5)")
    assert err <= 1e-5
    # the log-prob kernel sees the collected logits, not the float64 ones: the density under those
    mean, ls = lg[:, :3], lg[:, 3:]
    zz = (act - mean) * np.exp(-ls)
    logp = np.sum(-0.5 * zz * zz - ls, axis=1) - 0.5 * 3 * np.log(2 * np.pi)
    got = batch["logp"].cpu().numpy().reshape(-1).astype(np.float64)
    err = np.abs(got - logp)
    print(f"bf16 collector logp: max err {err.max():.3e} (bound use {np.max(err / (1e-4 + 1e-5 * np.abs(logp))):.4f})")
    assert np.isfinite(got).all()
    assert np.all(err <= 1e-4 + 1e-5 * np.abs(logp))
