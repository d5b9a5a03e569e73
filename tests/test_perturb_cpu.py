"""CPU: the perturbation layer's config mapping, the argument checks of its two C entry points (no
launch: every call returns before touching the GPU) and the reference's delay draw; then what
tests/test_gpu_perturb_shapes.py rests on: the reference's eight-entry table with zero-probability
entries, its delay line at ring sizes 3 and 8 against a literally indexed history, and a None sigma.

tests/golden/domain_randomization_v1.yaml is the reference's configs/domain_randomization_v1.yaml.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest
import yaml

from tests import perturb_ref as ref

ROOT = Path(__file__).resolve().parents[1]
DR_PATH = ROOT / "tests" / "golden" / "domain_randomization_v1.yaml"


@pytest.fixture(scope="module")
def cfg():
    return yaml.safe_load(DR_PATH.read_text())


@pytest.fixture(scope="module")
def nat():
    from swarm_marl_amd import _native
    return _native


@pytest.fixture(scope="module")
def lib(nat):
    return nat.load_library()


def test_noise_spec_train_and_ood(cfg):
    from swarm_marl_amd.perturbation import noise_spec
    spec, unsupported = noise_spec(cfg)
    assert spec == dict(delay_values=[0, 1, 2], delay_probs=[0.7, 0.2, 0.1], thrust_noise_std=0.03,
                        position_noise_std=0.02, velocity_noise_std=0.02, obstacle_distance_noise_std=0.03)
    assert unsupported == []
    ood, unsupported = noise_spec(cfg, "ood")
    assert ood["delay_values"] == [0, 1, 2, 3] and ood["delay_probs"] == [0.5, 0.25, 0.15, 0.10]
    assert {k: v for k, v in ood.items() if k.endswith("_std")} == {k: v for k, v in spec.items() if k.endswith("_std")}
    assert unsupported == []
    with pytest.raises(ValueError):
        noise_spec(cfg, "bogus")
    # groups that are absent perturb nothing; entries without a counterpart are reported
    empty, _ = noise_spec({"randomization": {}})
    assert empty["delay_values"] == [0] and empty["delay_probs"] == [1.0] and empty["thrust_noise_std"] == 0.0
    odd = {"randomization": {"actuation": {"thrust_noise_std": {"distribution": "uniform", "min": 0, "max": 1},
                                           "motor_lag": {"distribution": "normal", "std": 1.0}},
                             "sensing": {"position_noise_std": {"distribution": "normal", "mean": 0.5, "std": 0.1}}}}
    spec, unsupported = noise_spec(odd)
    assert spec["thrust_noise_std"] == 0.0 and spec["position_noise_std"] == 0.0
    assert set(unsupported) == {"actuation.thrust_noise_std", "actuation.motor_lag", "sensing.position_noise_std"}


@pytest.mark.parametrize("group,name,entry", [
    ("actuation", "thrust_noise_std", {"distribution": "normal", "std": -0.1}),
    ("sensing", "obstacle_distance_noise_std", {"distribution": "normal", "std": -1e-9}),
    ("actuation", "control_delay_steps", {"distribution": "discrete", "values": [0, 8], "probs": [0.5, 0.5]}),
    ("actuation", "control_delay_steps", {"distribution": "discrete", "values": [0, -1], "probs": [0.5, 0.5]}),
    ("actuation", "control_delay_steps", {"distribution": "discrete", "values": [0, 1], "probs": []}),
    ("actuation", "control_delay_steps", {"distribution": "discrete", "values": [], "probs": []}),
    ("actuation", "control_delay_steps", {"distribution": "discrete", "values": [0, 1], "probs": [1.2, -0.2]}),
    ("actuation", "control_delay_steps", {"distribution": "discrete", "values": [0, 1], "probs": [0.5, 0.49999]}),
    ("actuation", "control_delay_steps", {"distribution": "discrete", "values": [0, 1], "probs": [0.5, 0.50001]}),
    ("actuation", "control_delay_steps", {"distribution": "discrete", "values": [0, 1, 2], "probs": [0.5, 0.5]}),
], ids=["neg_std", "neg_std_tiny", "delay_8", "delay_neg", "no_probs", "empty", "neg_prob", "sum_low", "sum_high", "lengths"])
def test_noise_spec_errors(group, name, entry):
    from swarm_marl_amd.perturbation import noise_spec
    with pytest.raises(ValueError):
        noise_spec({"randomization": {group: {name: entry}}})


def test_noise_spec_accepts_a_sum_within_1e_6():
    from swarm_marl_amd.perturbation import noise_spec
    spec, _ = noise_spec({"randomization": {"actuation": {"control_delay_steps": {
        "distribution": "discrete", "values": [0, 7], "probs": [0.5, 0.5000005]}}}})
    assert spec["delay_values"] == [0, 7]


def test_scale_ranges_is_unchanged(cfg):
    """What tests/test_env_cfg_cpu.py test_dr_scale_ranges pins, on the reference file: the noise
    entries stay in scale_ranges' `unsupported` (they are Perturbation's, not DomainRandomizer's)."""
    from swarm_marl_amd.domain_randomization import scale_ranges
    ranges, unsupported = scale_ranges(cfg)
    assert ranges == {"max_accel": (0.9, 1.1), "max_speed": (0.9, 1.1), "dt": (0.95, 1.05),
                      "obstacle_radius": (0.9, 1.1), "world_size": (0.95, 1.05)}
    assert set(unsupported) == {"dynamics.mass_scale", "actuation.control_delay_steps", "actuation.thrust_noise_std",
                                "sensing.position_noise_std", "sensing.velocity_noise_std",
                                "sensing.obstacle_distance_noise_std"}


def test_delay_cum_matches_the_reference(cfg):
    from swarm_marl_amd.perturbation import delay_cum
    for probs in ([0.7, 0.2, 0.1], [0.5, 0.25, 0.15, 0.10], [1.0], [0.1] * 8):
        got, want = delay_cum(probs), ref.delay_cum(probs)
        assert got.dtype == np.float32 and np.array_equal(got, want) and got[-1] == 1.0
    assert np.array_equal(ref.delay_cum([0.7, 0.2, 0.1]), np.array([0.7, 0.7 + 0.2, 1.0]).astype(np.float32))


@pytest.mark.parametrize("ctype,cname", [("SwarmDelayTable", "swarm_delay_table_t"),
                                         ("SwarmActuateArgs", "swarm_actuate_args_t"),
                                         ("SwarmSenseArgs", "swarm_sense_args_t")])
def test_struct_layouts_match_header(nat, tmp_path, ctype, cname):
    cls = getattr(nat, ctype)
    fields = [f for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "swarm_mi355x.h"', "int main(void) {",
             f'printf("%zu\\n", sizeof({cname}));']
    lines += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f in fields]
    lines += ['printf("%d\\n", SWARM_PERTURB_MAX_DELAY);', "return 0; }"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(cls)
    assert out[1:-1] == [getattr(cls, f).offset for f in fields]
    assert out[-1] == nat.PERTURB_MAX_DELAY == ref.MAX_DELAY == 7
    assert nat.ABI_VERSION == 5  # additions only


def _act_args(nat, **kw):
    a = nat.SwarmActuateArgs()
    for name in ("actions", "ring", "step_count", "episode", "eff"):
        setattr(a, name, 16)  # never dereferenced: every call below returns before a launch
    a.delays.count = 1
    a.delays.cum[0] = 1.0
    a.ring_slots, a.num_envs, a.num_drones = 1, 4, 3
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _sense_args(nat, **kw):
    s = nat.SwarmSenseArgs()
    s.obs, s.active, s.step_count, s.episode, s.out = 16, 32, 48, 64, 80
    s.num_envs, s.num_drones, s.neighbor_k, s.sensed_obstacles = 4, 3, 3, 4
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _fails(nat, lib, rc, code):
    assert rc == getattr(nat, "SWARM_" + code), rc
    assert lib.swarm_perturb_last_error()
    with pytest.raises(ValueError, match="swarm_mi355x error"):
        nat.check(rc, lib, which="perturb")


@pytest.mark.parametrize("kw,code", [
    ({"actions": None}, "ENULL"), ({"ring": None}, "ENULL"), ({"eff": None}, "ENULL"),
    ({"step_count": None}, "ENULL"), ({"episode": None}, "ENULL"),
    ({"actions": None, "ring": None, "eff": None}, "ENULL"),  # the delay query without delay_out
    ({"num_envs": -1}, "EINVAL"), ({"num_drones": 0}, "ELIMIT"), ({"num_drones": 257}, "ELIMIT"),
    ({"ring_slots": 0}, "ELIMIT"), ({"ring_slots": 9}, "ELIMIT"),
])
def test_actuate_argument_errors(nat, lib, kw, code):
    _fails(nat, lib, lib.swarm_actuate(ctypes.byref(_act_args(nat, **kw)), None), code)


def test_actuate_delay_table_errors(nat, lib):
    assert lib.swarm_actuate(None, None) == nat.SWARM_ENULL
    a = _act_args(nat, ring_slots=8)
    a.delays.count = 0
    _fails(nat, lib, lib.swarm_actuate(ctypes.byref(a), None), "EINVAL")
    a.delays.count = 9
    _fails(nat, lib, lib.swarm_actuate(ctypes.byref(a), None), "EINVAL")
    a.delays.count = 2
    a.delays.values[0], a.delays.values[1] = 0, 8
    a.delays.cum[0], a.delays.cum[1] = 0.5, 1.0
    _fails(nat, lib, lib.swarm_actuate(ctypes.byref(a), None), "ELIMIT")  # delay above 7
    assert b"SWARM_PERTURB_MAX_DELAY" in lib.swarm_perturb_last_error()
    a.delays.values[1] = -1
    _fails(nat, lib, lib.swarm_actuate(ctypes.byref(a), None), "EINVAL")
    a.delays.values[1] = 3
    a.ring_slots = 3
    _fails(nat, lib, lib.swarm_actuate(ctypes.byref(a), None), "EINVAL")  # the ring is too short for it
    a.ring_slots = 4
    a.delays.cum[1] = 0.9
    _fails(nat, lib, lib.swarm_actuate(ctypes.byref(a), None), "EINVAL")  # cum does not end at 1
    a.delays.cum[0], a.delays.cum[1] = 1.0, 0.5
    _fails(nat, lib, lib.swarm_actuate(ctypes.byref(a), None), "EINVAL")  # cum falls
    # an empty batch is a valid no-op whatever the pointers
    assert lib.swarm_actuate(ctypes.byref(_act_args(nat, num_envs=0, actions=None, ring=None)), None) == 0


@pytest.mark.parametrize("kw,code", [
    ({"obs": None}, "ENULL"), ({"active": None}, "ENULL"), ({"step_count": None}, "ENULL"),
    ({"episode": None}, "ENULL"), ({"out": None}, "ENULL"), ({"out": 16}, "EINVAL"),
    ({"num_envs": -1}, "EINVAL"), ({"num_drones": 0}, "ELIMIT"), ({"num_drones": 257}, "ELIMIT"),
    ({"neighbor_k": -1}, "EINVAL"), ({"neighbor_k": 17}, "ELIMIT"), ({"sensed_obstacles": -1}, "EINVAL"),
    ({"sensed_obstacles": 6}, "ELIMIT"), ({"num_envs": 2**31 - 1, "num_drones": 256}, "ELIMIT"),
])
def test_sense_argument_errors(nat, lib, kw, code):
    _fails(nat, lib, lib.swarm_sense(ctypes.byref(_sense_args(nat, **kw)), None), code)


def test_sense_null_args_and_empty_batch(nat, lib):
    assert lib.swarm_sense(None, None) == nat.SWARM_ENULL
    assert lib.swarm_sense(ctypes.byref(_sense_args(nat, num_envs=0, obs=None, out=None)), None) == 0


# picked here, on the CPU, before any kernel ran: the reference's own frequencies at this seed
FREQ_SEED = 1


@pytest.mark.parametrize("profile", ["train", "ood"])
def test_reference_delay_frequencies(cfg, profile):
    from swarm_marl_amd.perturbation import noise_spec
    spec, _ = noise_spec(cfg, profile)
    e = 4096
    values, probs = spec["delay_values"], spec["delay_probs"]
    d = ref.draw_delays(FREQ_SEED, values, probs, np.arange(e), np.zeros(e, np.int64))
    assert set(np.unique(d)) <= set(values)
    for v, p in zip(values, probs):
        sigma = np.sqrt(e * p * (1 - p))
        assert abs(int((d == v).sum()) - e * p) <= 5 * sigma, (v, int((d == v).sum()), e * p, sigma)
    # an episode later every env draws again; an override wins where it is >= 0
    d1 = ref.draw_delays(FREQ_SEED, values, probs, np.arange(e), np.ones(e, np.int64))
    assert 0.2 < np.mean(d1 != d) < 0.8
    ov = np.full(e, -1, np.int32)
    ov[:10] = 2
    d2 = ref.draw_delays(FREQ_SEED, values, probs, np.arange(e), np.zeros(e, np.int64), ov)
    assert np.all(d2[:10] == 2) and np.array_equal(d2[10:], d[10:])


def test_reference_normals_are_standard():
    z = ref.normals(5, np.arange(20000), 3, 2, ref.STREAM_SENSE, 7, 11)
    assert z.shape == (4, 20000)
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    assert abs(np.corrcoef(z[0], z[1])[0, 1]) < 0.03 and abs(np.corrcoef(z[0], z[2])[0, 1]) < 0.03
    # every counter field matters
    base = ref.normals(5, 1, 3, 2, ref.STREAM_SENSE, 7, 11)
    for other in (ref.normals(6, 1, 3, 2, 1, 7, 11), ref.normals(5, 2, 3, 2, 1, 7, 11), ref.normals(5, 1, 4, 2, 1, 7, 11),
                  ref.normals(5, 1, 3, 3, 1, 7, 11), ref.normals(5, 1, 3, 2, 0, 7, 11), ref.normals(5, 1, 3, 2, 1, 8, 11),
                  ref.normals(5, 1, 3, 2, 1, 7, 12)):
        assert not np.array_equal(base, other)


# ---------------------------------------------------------------- what tests/test_gpu_perturb_shapes.py rests on
FULL_VALUES = [5, 2, 7, 0, 3, 6, 1, 4]
FULL_PROBS = [0, 0.2, 0, 0.3, 0.1, 0, 0.4, 0]


def test_reference_eight_entry_table_with_zero_probabilities():
    """cum has equal consecutive entries where a prob is 0; `first i with u < cum[i]` never lands on
    one of those, whatever the order of the values."""
    from swarm_marl_amd.perturbation import delay_cum
    cum = ref.delay_cum(FULL_PROBS)
    assert np.array_equal(cum, np.array([0, .2, .2, .5, .6, .6, 1, 1], np.float32))
    assert np.array_equal(delay_cum(FULL_PROBS), cum)
    e = 4096
    g, ep = 77 + np.arange(e), np.arange(e)[::-1].copy()
    d = ref.draw_delays(FREQ_SEED, FULL_VALUES, FULL_PROBS, g, ep)
    # literally: the uniform of the header against cum, entry by entry
    x0 = ref._words(FREQ_SEED, g, 0, 0, ref.STREAM_DELAY, ep, 0)[0]
    u = (x0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    for i in range(e):
        first = next(j for j in range(8) if u[i] < cum[j])
        assert d[i] == FULL_VALUES[first] and FULL_PROBS[first] > 0
    for v, p in zip(FULL_VALUES, FULL_PROBS):
        count = int((d == v).sum())
        assert (count == 0) if p == 0 else abs(count - e * p) <= 5 * np.sqrt(e * p * (1 - p)), (v, count)
    assert np.all(ref.draw_delays(FREQ_SEED, [5], [1.0], g, ep) == 5)  # a single entry draws nothing


@pytest.mark.parametrize("r", [3, 8])
def test_reference_delay_line_against_a_literal_history(r):
    """DelayLine with ring_slots 3 and 8: eff is the clipped command of d steps ago in the same
    episode, zero before the episode's step d, with restarts, a start far from 0 and overrides above
    R - 1 (clamped to R - 1)."""
    e, n, steps = 5, 2, 3 * r + 2
    values = [r - 1, 0, 1]
    line = ref.DelayLine(e, n, values, [0.3, 0.3, 0.4], FREQ_SEED, env_offset=3, ring_slots=r)
    assert line.ring.shape == (r, e, n, 3)
    override = np.array([r - 1, -1, 7 + r, -1, 0], np.int32)
    rng = np.random.default_rng(r)
    sc = np.array([0, 2**31 - 40, 0, 1, 2], np.int64)
    ep = rng.integers(0, 2**32, e).astype(np.uint32)
    hist, zeroed, seen = [], 0, set()
    for t in range(steps):
        a = rng.uniform(-1.5, 1.5, (e, n, 3)).astype(np.float32)
        delayed, want, bound, d = line.actuate(a, sc, ep, None, override)
        assert d[0] == r - 1 and d[2] == r - 1 and d[4] == 0 and set(d.tolist()) <= set(values)
        assert not bound.any() and np.array_equal(want, delayed.astype(np.float64))
        hist.append((ep.copy(), sc.copy(), np.clip(a, np.float32(-1), np.float32(1))))
        for i in range(e):
            if d[i] <= sc[i] and t - d[i] >= 0:
                p_ep, p_sc, p_c = hist[t - d[i]]
                assert p_ep[i] == ep[i] and p_sc[i] == sc[i] - d[i]
                assert np.array_equal(delayed[i], p_c[i]), (t, i)
            elif d[i] > sc[i]:
                zeroed += 1
                assert not delayed[i].any()
        seen |= set(d.tolist())
        sc += 1
        for i in (3, 4):
            if sc[i] >= r + 1 + i:
                sc[i], ep[i] = 0, rng.integers(0, 2**32)
    assert zeroed > 0 and len(seen) >= 2


def test_reference_sense_none_sigma_is_a_zero_sigma():
    e, n, k, ms = 4, 3, 2, 1
    rng = np.random.default_rng(0)
    obs = rng.uniform(-3, 3, (e, n, 9 + 4 * k + 4 * ms)).astype(np.float32)
    active = np.ones((e, n), np.uint8)
    sig = [np.full(e, s, np.float32) for s in (0.1, 0.2, 0.3)]
    sc, ep = np.arange(e), np.arange(e) + 5
    full = ref.sense(obs, active, *sig, sc, ep, 9, 2, k, ms)
    for null in ((0,), (1,), (2,), (0, 1, 2)):
        none = ref.sense(obs, active, *[None if i in null else s for i, s in enumerate(sig)], sc, ep, 9, 2, k, ms)
        zeros = [np.zeros(e, np.float32) if i in null else s for i, s in enumerate(sig)]
        zero = ref.sense(obs, active, *zeros, sc, ep, 9, 2, k, ms)
        for a, b in zip(none, zero):
            assert np.array_equal(a, b)
        assert none[2].sum() < full[2].sum()
    assert not none[2].any() and np.array_equal(none[0], obs.astype(np.float64))
