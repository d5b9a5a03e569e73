"""CPU: the keyed domain-randomisation draw on the host (`keyed_values`) against its independent NumPy
statement (tests/dr_ref.py), what the draw must satisfy as a distribution and as a key layout, and the
argument checks of `swarm_env_cfg_randomize` (no launch: every call returns before touching the GPU).

Every comparison of values is bitwise: both sides are float64 without fused multiply-add.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest
import yaml

from tests import dr_ref
from tests import perturb_ref

ROOT = Path(__file__).resolve().parents[1]
DR_PATH = ROOT / "tests" / "golden" / "domain_randomization_v1.yaml"
SEEDS = (0, 1, 0x9E3779B97F4A7C15, 2**64 - 1)
# env indices below and above 2^16 and at the top of the 32-bit range; episodes at both ends of theirs
ENVS = np.concatenate([np.arange(0, 40), [65535, 65536, 65537, 70000, 70063, 2**31 - 1, 2**31, 2**32 - 2, 2**32 - 1]])
EPISODES = np.concatenate([np.arange(0, 12), [255, 65536, 2**31 - 1, 2**31, 2**32 - 2, 2**32 - 1]])


@pytest.fixture(scope="module")
def ranges():
    from swarm_marl_amd.domain_randomization import scale_ranges
    r, _ = scale_ranges(yaml.safe_load(DR_PATH.read_text()))
    assert set(r) == set(dr_ref.PARAMS)
    return r


@pytest.fixture(scope="module")
def base():
    from swarm_marl_amd.envs.common import DroneEnvConfig
    c = DroneEnvConfig()
    return {p: float(getattr(c, p)) for p in dr_ref.PARAMS}


@pytest.fixture(scope="module")
def nat():
    from swarm_marl_amd import _native
    return _native


@pytest.fixture(scope="module")
def lib(nat):
    return nat.load_library()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------- the host draw
def test_keyed_values_equal_the_reference_bitwise(ranges, base):
    from swarm_marl_amd.domain_randomization import keyed_values
    g, ep = ENVS[:, None], EPISODES[None, :]
    total = 0
    for seed in SEEDS:
        got, want = keyed_values(seed, g, ep, ranges, base), dr_ref.values(seed, g, ep, ranges, base)
        assert set(got) == set(dr_ref.PARAMS)
        for p in dr_ref.PARAMS:
            assert got[p].dtype == np.float64 and got[p].shape == (len(ENVS), len(EPISODES))
            assert np.array_equal(_bits(got[p]), _bits(want[p])), (seed, p)
        total += got["dt"].size
    assert total >= 3000
    # the key is (seed, env, episode) modulo 2^32 each way: an episode counter that wraps draws episode 0's values
    a = keyed_values(5, ENVS, 2**32 - 1 + 1, ranges, base)
    b = keyed_values(5, ENVS, 0, ranges, base)
    c = keyed_values(5, ENVS, 2**32 - 1, ranges, base)
    for p in dr_ref.PARAMS:
        assert np.array_equal(_bits(a[p]), _bits(b[p])) and not np.array_equal(_bits(b[p]), _bits(c[p]))
    # int32 views of the device counters (negative numbers) are the same episodes
    d = keyed_values(5, ENVS, np.int32(-1), ranges, base)
    assert all(np.array_equal(_bits(c[p]), _bits(d[p])) for p in dr_ref.PARAMS)


def test_a_parameter_without_a_range_is_its_base_value(ranges, base):
    from swarm_marl_amd.domain_randomization import keyed_values
    some = {k: v for k, v in ranges.items() if k in ("max_speed", "obstacle_radius")}
    got, want = keyed_values(9, ENVS, 3, some, base), dr_ref.values(9, ENVS, 3, some, base)
    full = keyed_values(9, ENVS, 3, ranges, base)
    for p in dr_ref.PARAMS:
        assert np.array_equal(_bits(got[p]), _bits(want[p]))
        if p in some:  # the other parameters' switches do not move a parameter's word
            assert np.array_equal(_bits(got[p]), _bits(full[p]))
        else:
            assert np.all(got[p] == base[p])
    none = keyed_values(9, ENVS, 3, {}, base)
    assert all(np.all(none[p] == base[p]) for p in dr_ref.PARAMS)


def test_every_scale_is_strictly_inside_its_range(ranges):
    g, ep = ENVS[:, None], EPISODES[None, :]
    for seed in SEEDS:
        sc = dr_ref.scales(seed, g, ep, ranges)
        for p, (lo, hi) in ranges.items():
            assert np.all(sc[p] > lo) and np.all(sc[p] < hi), (seed, p)
    # the extreme words: u = 2^-25 and 1 - 2^-25 stay inside after the roundings
    for p, (lo, hi) in ranges.items():
        for n24 in (0, 2**24 - 1):
            u = (np.float64(n24) + 0.5) * 2.0 ** -24
            s = np.float64(lo) + (np.float64(hi) - np.float64(lo)) * u
            assert lo < s < hi, (p, n24)


# picked here, on the CPU, before any kernel ran: the reference's own means at this seed
MEAN_SEED = 1


def test_mean_scale_over_4096_envs(ranges):
    e = 4096
    for episode in (0, 7):
        sc = dr_ref.scales(MEAN_SEED, np.arange(e), episode, ranges)
        for p, (lo, hi) in ranges.items():
            bound = 4 * (hi - lo) / np.sqrt(12 * e)
            assert abs(sc[p].mean() - (lo + hi) / 2) <= bound, (p, episode, sc[p].mean(), bound)


def test_parameters_and_episodes_never_share_a_word(ranges):
    # structurally: parameter i owns word i & 3 of block i >> 2, five different (block, word) slots
    slots = {(i >> 2, i & 3) for i in range(len(dr_ref.PARAMS))}
    assert len(slots) == len(dr_ref.PARAMS)
    # the counter of a block holds (g, block and stream, episode, 0): two episodes of an env, and the
    # perturbation layer's streams 0..2 with the same seed, are other blocks
    assert dr_ref.STREAM_DR not in (perturb_ref.STREAM_ACT, perturb_ref.STREAM_SENSE, perturb_ref.STREAM_DELAY)
    g = ENVS[:, None]
    ep = np.arange(64)[None, :]
    seed = SEEDS[2]
    words = np.stack([dr_ref.word(seed, g, ep, i) for i in range(5)])  # [5, G, 64]
    for i in range(5):
        for j in range(i + 1, 5):
            assert np.mean(words[i] == words[j]) < 1e-3, (i, j)  # other words, not one word read twice
    for k in (1, 2, 63):  # episode ep against episode ep + k of the same env
        assert np.mean(words[:, :, k:] == words[:, :, :-k]) < 1e-3, k
    blk = [np.stack(perturb_ref._words(seed, g, 0, b, dr_ref.STREAM_DR, ep, 0)) for b in (0, 1)]
    assert np.array_equal(words[:4], blk[0]) and np.array_equal(words[4], blk[1][0])
    for stream in (0, 1, 2):
        for b in (0, 1):
            other = np.stack(perturb_ref._words(seed, g, 0, b, stream, ep, 0))
            assert np.mean(other == blk[b]) < 1e-3, (stream, b)
    # and two envs of one episode
    assert np.mean(words[:, 1:] == words[:, :-1]) < 1e-3


# ---------------------------------------------------------------- the ABI
def _params(nat, lib, **kw):
    p = nat.SwarmParams()
    lib.swarm_params_default(ctypes.byref(p))
    p.num_envs = 4
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _table(nat, ranges, **over):
    t = nat.SwarmDrTable()
    for i, name in enumerate(nat.DR_PARAMS):
        if name in ranges:
            t.lo[i], t.hi[i] = ranges[name]
            t.enabled[i] = 1
    for name, (lo, hi, on) in over.items():
        i = nat.DR_PARAMS.index(name)
        t.lo[i], t.hi[i], t.enabled[i] = lo, hi, on
    return t


def _call(lib, p, t, episode=16, cfg=64, mask=None):
    return lib.swarm_env_cfg_randomize(None if p is None else ctypes.byref(p), None if t is None else ctypes.byref(t),
                                       7, episode, 1, mask, 0xFF, cfg, None)


def _fails(nat, lib, rc, code, text=None):
    assert rc == getattr(nat, "SWARM_" + code), rc
    assert lib.swarm_dr_last_error()
    if text is not None:
        assert text in lib.swarm_dr_last_error()
    with pytest.raises(ValueError, match="swarm_mi355x error"):
        nat.check(rc, lib, which="dr")


def test_binding(nat, lib):
    assert nat.DR_PARAMS == dr_ref.PARAMS
    assert nat.LAST_ERROR["dr"] == "swarm_dr_last_error"
    for name in nat.DR_SYMBOLS:
        assert name in nat.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert nat.ABI_VERSION == 5  # additions only


def test_table_layout_matches_header(nat, tmp_path):
    fields = [f for f, _ in nat.SwarmDrTable._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "swarm_mi355x.h"', "int main(void) {",
             'printf("%zu %d\\n", sizeof(swarm_dr_table_t), SWARM_DR_PARAMS);']
    lines += [f'printf("%zu\\n", offsetof(swarm_dr_table_t, {f}));' for f in fields]
    lines += ["return 0; }"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(nat.SwarmDrTable) and out[1] == len(nat.DR_PARAMS) == 5
    assert out[2:] == [getattr(nat.SwarmDrTable, f).offset for f in fields]


def test_randomize_null_arguments(nat, lib, ranges):
    p, t = _params(nat, lib), _table(nat, ranges)
    _fails(nat, lib, _call(lib, None, t), "ENULL")
    _fails(nat, lib, _call(lib, p, None), "ENULL")
    _fails(nat, lib, _call(lib, p, t, episode=None), "ENULL", b"episode")
    _fails(nat, lib, _call(lib, p, t, cfg=None), "ENULL", b"env_cfg")


@pytest.mark.parametrize("name", dr_ref.PARAMS)
@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-0.5, 1.0), (1.2, 1.1), (float("nan"), 1.0), (0.9, float("nan")),
                                   (0.9, float("inf"))])
def test_randomize_range_errors(nat, lib, ranges, name, lo, hi):
    p = _params(nat, lib)
    _fails(nat, lib, _call(lib, p, _table(nat, ranges, **{name: (lo, hi, 1)})), "EINVAL", b"lo")
    # also for an empty batch, as swarm_actuate reports its table
    _fails(nat, lib, _call(lib, _params(nat, lib, num_envs=0), _table(nat, ranges, **{name: (lo, hi, 1)})), "EINVAL")


def test_randomize_param_errors_and_physics_dt(nat, lib, ranges):
    t = _table(nat, ranges)
    _fails(nat, lib, _call(lib, _params(nat, lib, num_envs=-1), t), "EINVAL")
    _fails(nat, lib, _call(lib, _params(nat, lib, abi_version=1), t), "EINVAL")
    _fails(nat, lib, _call(lib, _params(nat, lib, dynamics=7), t), "EINVAL")
    phys = dict(dynamics=nat.DYN_POINTMASS_PHYSICS, reward_mode=nat.REW_PHYSICS)
    _fails(nat, lib, _call(lib, _params(nat, lib, **phys), t), "EINVAL", b"dt")
    _fails(nat, lib, _call(lib, _params(nat, lib, num_envs=0, **phys), t), "EINVAL", b"dt")


def test_randomize_empty_batch_is_a_no_op(nat, lib, ranges):
    p0 = _params(nat, lib, num_envs=0)
    assert _call(lib, p0, _table(nat, ranges), episode=None, cfg=None) == 0
    # a disabled parameter's range is not read: physics with dt off, and a bad range that is off
    phys = _params(nat, lib, num_envs=0, dynamics=nat.DYN_POINTMASS_PHYSICS, reward_mode=nat.REW_PHYSICS)
    assert _call(lib, phys, _table(nat, ranges, dt=(0.95, 1.05, 0)), episode=None, cfg=None) == 0
    assert _call(lib, p0, _table(nat, ranges, max_accel=(-1.0, -2.0, 0)), episode=None, cfg=None) == 0
    assert _call(lib, p0, _table(nat, {}), episode=None, cfg=None) == 0


def test_generator_mode_signature_is_unchanged():
    import inspect

    from swarm_marl_amd.domain_randomization import DomainRandomizer
    sig = inspect.signature(DomainRandomizer.__init__)
    assert sig.parameters["keyed"].default is False
    assert [k for k in sig.parameters][:3] == ["self", "vec", "dr_cfg"]
