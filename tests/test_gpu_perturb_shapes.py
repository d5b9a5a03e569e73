"""GPU: swarm_sense and swarm_actuate (csrc/swarm_perturb.hip) called directly through ctypes on
synthetic state, off the shapes tests/test_gpu_perturb.py reaches through `Perturbation`, against
tests/perturb_ref.py under that file's bounds (derived in its docstring; nothing new here):
    a noisy element   sigma 1e-5 (1 + |z_ref|) + 2^-22 |ref|   (a recomputed distance: the sum of its
                      three components' bounds plus 2^-22 |ref|)
    everything the definition leaves alone, every delay and the ring: bit for bit.

swarm_sense, S = 1 + K + Ms lanes per row.  SENSE_CASES: both maxima (S = 22, a ragged fourth
workgroup), full N = 256 (agent numbers up to 255 in the counter word), K = 0 with obstacles (block
numbers without a neighbour offset), N = 1 with S = 1 (every lane an own lane) and two S that do not
divide 64; in all but S = 1 rows straddle wave boundaries (asserted on the sizes).  obs and out are
views into guard-filled arenas that start 4 bytes past a 16-byte boundary; episode uses its high bit,
step_count is any non-negative int32, env_offset + e crosses 2^32 in one case.  Crafted into every
case before either side sees it: padding slots (four zeros) in front of live ones, slots with one
non-zero float at each of the four positions, a slot of four -0.0 (padding by `== 0`), a slot with a
NaN (not padding), and NaN payloads (a signalling one too), infinities, -0.0 and denormals in
inactive rows, in the groups of zero-sigma envs and in the obstacle vectors, all compared as uint32.
An obstacle slot's NaN sits in its vector: fmaxf(NaN, 0) is 0 by the header while NumPy's maximum
gives NaN, so a NaN distance is left out.  A reference NaN (the neighbour slot with one) must be a
NaN in the output.  The NULL sigma pointers are passed one at a time and all at once.

swarm_actuate, stepped on a step_count / episode / ring the test owns and advances itself (envs
restart at 0 with a new episode number at different times): ring sizes 1, 3, 5, 6, 7, 8 with
unsorted tables at (E, N) = (3, 256), (37, 7), (5, 1), the longest delay R - 1 fixed on env 0, for
2 R + 5 steps; a step_count of 2^31 - 12 counting up; two eight-entry tables with zero-probability
entries over 4,099 envs through the query path; overrides above R - 1 (the kernel's clamp), also
through `Perturbation.set(delay=<device tensor>)`; delay_override, thrust_noise_std and delay_out
NULL.  eff, delay_out and the ring live in guard-filled arenas.

Each case asserts on the reference or the sizes that what it exists for occurs.  The largest share
of the bound used is printed per case; measured on an MI355X over every case of this file: 0.227 on
sense (full N with K = 16), 0.116 on actuate (R = 8, 37 x 7), MEASURED below (tests/test_gpu_perturb.py:
0.231 on sense, 0.102 on actuate).
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from tests import perturb_ref as ref

pytestmark = pytest.mark.gpu

# records, not bounds: the largest share of the bound used over the cases of this file
MEASURED = dict(sense=0.2267, actuate=0.1161)

SEED = 0x12345678_9ABCDEF1
GUARD = 0x5A5A5A5A
PAD = 64  # guard floats on either side of an arena's payload (plus one in front: the 4-byte offset)
# bit patterns that arithmetic would not leave alone: quiet NaNs with payloads (one negative), a
# signalling NaN, +-inf, -0.0, the smallest denormal and the largest negative one
SPECIALS = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF],
                    np.uint32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib():
    from swarm_marl_amd import _native as nat
    return nat.load_library()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _np(t):
    return t.cpu().numpy().copy()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class Arena:
    """`count` 4-byte elements between guards, the payload 4 bytes past a 16-byte boundary."""

    def __init__(self, dev, count, init=None, dtype=torch.float32):
        self.raw = torch.full((PAD + 1 + count + PAD,), GUARD, dtype=torch.int32, device=dev)
        assert self.raw.data_ptr() % 16 == 0
        self.count = count
        self.view = self.raw[PAD + 1:PAD + 1 + count].view(dtype)
        assert self.view.data_ptr() % 16 == 4
        if init is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1)).to(dev))
        self.before = self.raw.clone()

    def ptr(self):
        return self.view.data_ptr()

    def guards_intact(self):
        return bool((self.raw[:PAD + 1] == GUARD).all()) and bool((self.raw[PAD + 1 + self.count:] == GUARD).all())

    def unchanged(self):
        return torch.equal(self.raw, self.before)

    def host(self, shape, dtype=np.float32):
        return _np(self.view.view(torch.int32)).view(dtype).reshape(shape)


def _dev_i32(dev, a):
    """A device int32 tensor with the bits of the 4-byte host array `a`."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(dev)


# ---------------------------------------------------------------- swarm_sense
# (E, N, K, Ms, env_offset)
SENSE_CASES = {
    "both_maxima": (5, 7, 16, 5, 2**32 - 2),     # g = env_offset + e wraps the low word
    "full_n": (2, 256, 16, 0, 11),
    "no_neighbour_slots": (9, 3, 0, 5, 1000),
    "own_block_only": (300, 1, 0, 0, 7),
    "s3": (3, 64, 1, 1, 2**31 - 1),
    "s7": (4, 5, 5, 1, 5),
}
RECIPES = ("pad", "single0", "single1", "single2", "single3", "negzero", "nan")


def _sense_sigmas(e):
    """Per-env stds, each group zero on other envs (E = 2 has a zero and a non-zero of each); env 1
    has so = 5, which drives distances to the clamp at 0."""
    i = np.arange(e)
    sp = np.where(i % 3 == 1, 0.0, 0.02 + 0.1 * (i % 4)).astype(np.float32)
    sv = np.where(i % 2 == 0, 0.0, 0.02 * (1 + i % 3)).astype(np.float32)
    so = np.where(i % 4 == 0, 0.0, 0.03).astype(np.float32)
    so[1] = 5.0
    return sp, sv, so


def _slot_value(recipe, kind):
    if recipe == "pad":
        return np.zeros(4, np.float32)
    if recipe == "negzero":
        return np.full(4, -0.0, np.float32)
    if recipe == "nan":  # an obstacle's distance stays finite (the module docstring)
        return np.array([np.nan, 1, -2, 3] if kind == "nbr" else [1, np.nan, -2, 3], np.float32)
    v = np.zeros(4, np.float32)
    v[int(recipe[-1])] = 2.5
    return v


def _synthetic(e, n, k, ms, sig, seed):
    """(obs [E,N,D] f32, active [E,N] u8, step_count [E] i32, episode [E] u32), the edge cases
    crafted in; `crafted`: {kind: {recipe: (env, agent, slot)}}."""
    rng = np.random.default_rng(seed)
    sp, sv, so = sig
    d = 9 + 4 * k + 4 * ms
    obs = np.zeros((e, n, d), np.float32)
    obs[..., 0:3] = rng.uniform(-10, 10, (e, n, 3))
    obs[..., 3:6] = rng.uniform(-2, 2, (e, n, 3))
    obs[..., 6:9] = rng.uniform(-20, 20, (e, n, 3))
    for j in range(k + ms):
        o = 9 + 4 * j
        rel = rng.uniform(-8, 8, (e, n, 3)).astype(np.float32)
        dist = np.sqrt((rel.astype(np.float64) ** 2).sum(-1))
        obs[..., o:o + 3] = rel
        obs[..., o + 3] = dist if j < k else np.maximum(dist - 0.5, 0.0)  # to an obstacle's surface
    active = (rng.uniform(size=(e, n)) < 0.8).astype(np.uint8)
    step_count = rng.integers(0, 2**31, e).astype(np.int32)
    episode = rng.integers(0, 2**32, e).astype(np.uint32)
    episode[0] |= np.uint32(0x80000000)
    act = active.astype(bool)
    bits = obs.view(np.uint32)

    def specials(count, shift):
        return SPECIALS[(np.arange(count) + shift) % len(SPECIALS)]

    # what is copied whatever it holds: inactive rows, the groups of zero-sigma envs (every other
    # active row), the vector of an obstacle slot
    for i, a in zip(*np.nonzero(~act)):
        bits[i, a] = specials(d, i + a)
    for i in range(e):
        for a in np.flatnonzero(act[i])[::2]:
            if sp[i] == 0:
                bits[i, a, 0:3], bits[i, a, 6:9] = specials(3, a), specials(3, a + 3)
                if k:
                    bits[i, a, 9:13] = specials(4, a + 1)
            if sv[i] == 0:
                bits[i, a, 3:6] = specials(3, a + 5)
            if ms and so[i] == 0:
                bits[i, a, 9 + 4 * k:13 + 4 * k] = specials(4, a + 2)
            if ms and so[i] != 0:
                o = 9 + 4 * (k + ms - 1)
                bits[i, a, o:o + 3] = specials(3, a + 6)
    # the slot classes, each in an active row of an env whose sigma would otherwise touch the slot
    crafted = {}
    for kind, count, first, s in (("nbr", k, 0, sp), ("obst", ms, k, so)):
        if not count:
            continue
        rows = np.flatnonzero((act & (s != 0)[:, None]).reshape(-1))
        assert len(rows) >= len(RECIPES), (kind, len(rows))
        rows = rows[np.linspace(0, len(rows) - 1, len(RECIPES)).astype(int)]
        assert len(set(rows.tolist())) == len(RECIPES)
        crafted[kind] = {}
        for r, (recipe, row) in enumerate(zip(RECIPES, rows)):
            i, a = divmod(int(row), n)
            slot = 0 if recipe == "pad" else r % count  # the padding in front of live slots
            o = 9 + 4 * (first + slot)
            obs[i, a, o:o + 4] = _slot_value(recipe, kind)
            if recipe == "pad" and count > 1:  # followed by a live slot
                obs[i, a, o + 4:o + 8] = np.array([1.5, -2.5, 0.5, 3.0], np.float32)
            crafted[kind][recipe] = (i, a, first + slot)
    return obs, active, step_count, episode, crafted


def _classes_occur(obs, active, sig, touched, k, ms, crafted):
    """On the inputs and the reference alone: every class the case exists for is there."""
    act = active.astype(bool)
    for s in sig[:2] + ((sig[2],) if ms else ()):
        assert (s == 0).any() and (s != 0).any()
    groups = [slice(0, 3), slice(3, 6), slice(6, 9)]
    if k:
        groups.append(slice(9, 9 + 4 * k))
    if ms:
        groups.append(slice(12 + 4 * k, 9 + 4 * (k + ms), 4))  # the obstacle distances
        vectors = np.ones(4 * ms, bool)
        vectors[3::4] = False
        assert not touched[..., 9 + 4 * k:][..., vectors].any()  # an obstacle's vector stays
    for g in groups:
        assert touched[..., g].any() and not touched[..., g].all(), g
    assert not touched[~act].any() and (~act).any() and act.any()
    special = np.isin(_bits(obs), SPECIALS[:5]) | np.isin(_bits(obs), SPECIALS[5:])
    assert special[~act].any() and special[act].any() and not (special & touched).any()
    for kind, made in crafted.items():
        s = sig[0] if kind == "nbr" else sig[2]
        for recipe, (i, a, slot) in made.items():
            o = 9 + 4 * slot
            v, t = obs[i, a, o:o + 4], touched[i, a, o:o + 4]
            assert act[i, a] and s[i] != 0
            if recipe in ("pad", "negzero"):
                assert not (v != 0).any() and not t.any(), (kind, recipe)
                assert (_bits(v) == (0x80000000 if recipe == "negzero" else 0)).all()
            else:
                assert (np.isnan(v).sum() == 1) if recipe == "nan" else ((v != 0).sum() == 1 and v[int(recipe[-1])] != 0)
                assert t[3] and t[:3].all() == (kind == "nbr"), (kind, recipe)
        i, a, slot = made["pad"]
        last = k if kind == "nbr" else k + ms
        if slot + 1 < last:
            assert obs[i, a, 13 + 4 * slot:17 + 4 * slot].all()  # not a trailing padding


def _sense(dev, lib, obs_arena, out_arena, active, sig_dev, step_count, episode, e, n, k, ms, env_offset):
    from swarm_marl_amd import _native as nat
    s = nat.SwarmSenseArgs()
    s.obs, s.out, s.active = obs_arena.ptr(), out_arena.ptr(), active.data_ptr()
    s.position_noise_std, s.velocity_noise_std, s.obstacle_noise_std = (None if t is None else t.data_ptr() for t in sig_dev)
    s.step_count, s.episode = step_count.data_ptr(), episode.data_ptr()
    s.seed, s.env_offset = SEED, env_offset
    s.num_envs, s.num_drones, s.neighbor_k, s.sensed_obstacles = e, n, k, ms
    nat.check(lib.swarm_sense(ctypes.byref(s), _stream(dev)), lib, which="perturb")
    torch.cuda.synchronize(dev)


def _compare_sense(got, obs, want, bound, touched, tag):
    """Untouched elements bit for bit, a reference NaN a NaN, the rest under the bound; the share used."""
    assert np.array_equal(_bits(got)[~touched], _bits(obs)[~touched]), tag
    nan = touched & np.isnan(want)
    assert np.isnan(got[nan]).all(), tag
    ok = touched & ~nan
    if not ok.any():
        return 0.0
    assert np.isfinite(bound[ok]).all() and (bound[ok] > 0).all()
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - want)
    share = float(np.max(err[ok] / bound[ok]))
    assert np.all(err[ok] <= bound[ok]), (tag, share)
    return share


class SenseCase:
    def __init__(self, dev, e, n, k, ms, env_offset, seed, sig=None):
        self.shape = (e, n, k, ms, env_offset)
        self.sig = _sense_sigmas(e) if sig is None else sig
        self.obs, self.active, self.step_count, self.episode, self.crafted = _synthetic(e, n, k, ms, self.sig, seed)
        self.dev = dev
        self.obs_arena = Arena(dev, self.obs.size, self.obs)
        self.d_active = torch.from_numpy(self.active).to(dev)
        self.d_sig = [torch.from_numpy(s).to(dev) for s in self.sig]
        self.d_step, self.d_episode = _dev_i32(dev, self.step_count), _dev_i32(dev, self.episode)

    def run(self, lib, null=()):
        """(got, out arena, (want, bound, touched)) with the sigma pointers named in `null` NULL."""
        e, n, k, ms, env_offset = self.shape
        out = Arena(self.dev, self.obs.size)
        sig_dev = [None if i in null else t for i, t in enumerate(self.d_sig)]
        _sense(self.dev, lib, self.obs_arena, out, self.d_active, sig_dev, self.d_step, self.d_episode, e, n, k, ms, env_offset)
        sig = [None if i in null else s for i, s in enumerate(self.sig)]
        with np.errstate(invalid="ignore"):  # the crafted NaNs
            want = ref.sense(self.obs, self.active, *sig, self.step_count, self.episode, SEED, env_offset, k, ms)
        return out.host(self.obs.shape), out, want


def _max_agents():
    from swarm_marl_amd import _native as nat
    return nat.PERTURB_MAX_AGENTS


@pytest.mark.parametrize("name", list(SENSE_CASES))
def test_sense_at_untested_shapes(dev, lib, name):
    e, n, k, ms, env_offset = SENSE_CASES[name]
    s = 1 + k + ms
    lanes = e * n * s
    if name == "both_maxima":
        assert s == 22 and lanes == 770 and lanes % 256 != 0 and -(-lanes // 256) == 4
    if name == "full_n":
        assert n == _max_agents() and lanes > 256
    if s > 1:  # rows straddle wave boundaries (and so workgroup boundaries: 256 = 4 x 64)
        assert 64 % s != 0 and lanes > 64
    else:
        assert n == 1 and lanes == e > 256
    case = SenseCase(dev, e, n, k, ms, env_offset, seed=len(name) + 100 * e)
    got, out, (want, bound, touched) = case.run(lib)
    _classes_occur(case.obs, case.active, case.sig, touched, k, ms, case.crafted)
    assert out.guards_intact() and case.obs_arena.unchanged()
    share = _compare_sense(got, case.obs, want, bound, touched, name)
    if ms and e > 1:  # env 1 (so = 5): the clamp at 0 is hit, exactly
        o = slice(12 + 4 * k, 9 + 4 * (k + ms), 4)
        hit = touched[1][..., o] & (want[1][..., o] == 0)
        assert hit.any() and not got[1][..., o][hit].any() and not (got[1][..., o][touched[1][..., o]] < 0).any()
    print(f"sense {name} E={e} N={n} K={k} Ms={ms} S={s} lanes={lanes}: largest share of the bound used {share:.4f}")


def test_sense_null_sigma_pointers(dev, lib):
    """Each sigma pointer NULL in turn equals that sigma zero; all three NULL copy obs bit for bit."""
    e, n, k, ms = 6, 5, 2, 2
    sig = tuple(np.where(s == 0, np.float32(0.05), s) for s in _sense_sigmas(e))  # every group on, so a NULL matters
    case = SenseCase(dev, e, n, k, ms, 3, seed=77, sig=sig)
    _, _, (_, _, full) = case.run(lib)
    shares = []
    for null in ((0,), (1,), (2,), (0, 1, 2)):
        got, out, (want, bound, touched) = case.run(lib, null)
        assert touched.sum() < full.sum() and not (touched & ~full).any()  # the group is off on the reference
        assert out.guards_intact() and case.obs_arena.unchanged()
        shares.append(_compare_sense(got, case.obs, want, bound, touched, f"null {null}"))
        if len(null) == 3:
            assert not touched.any() and np.array_equal(_bits(got), _bits(case.obs))
        else:
            assert touched.any()
    print(f"sense NULL sigmas: largest share of the bound used {max(shares):.4f}")


# ---------------------------------------------------------------- swarm_actuate
def _table(a, values, probs):
    a.delays.count = len(values)
    for i, (v, c) in enumerate(zip(values, ref.delay_cum(probs))):
        a.delays.values[i], a.delays.cum[i] = int(v), float(c)


class Actuator:
    """swarm_actuate on state the test owns: step_count, episode, ring, eff and delay_out on the
    device (the last three between guards), with the reference's DelayLine next to them."""

    def __init__(self, dev, lib, e, n, r, values, probs, *, env_offset=0, override=None, sigma=None, want_delays=True):
        from swarm_marl_amd import _native as nat
        self.dev, self.lib, self.nat, self.e, self.n, self.r = dev, lib, nat, e, n, r
        self.ring = Arena(dev, r * e * n * 3, np.zeros(r * e * n * 3, np.float32))
        self.eff = Arena(dev, e * n * 3)
        self.delay_out = Arena(dev, e, dtype=torch.int32)
        self.step_count = torch.zeros(e, dtype=torch.int32, device=dev)
        self.episode = torch.zeros(e, dtype=torch.int32, device=dev)
        self.actions = torch.zeros((e, n, 3), dtype=torch.float32, device=dev)
        self.override = None if override is None else torch.from_numpy(np.asarray(override, np.int32)).to(dev)
        self.sigma = None if sigma is None else torch.from_numpy(np.asarray(sigma, np.float32)).to(dev)
        a = nat.SwarmActuateArgs()
        a.actions, a.ring, a.eff = self.actions.data_ptr(), self.ring.ptr(), self.eff.ptr()
        a.delay_override = None if override is None else self.override.data_ptr()
        a.thrust_noise_std = None if sigma is None else self.sigma.data_ptr()
        a.step_count, a.episode = self.step_count.data_ptr(), self.episode.data_ptr()
        a.delay_out = self.delay_out.ptr() if want_delays else None
        _table(a, values, probs)
        a.ring_slots, a.num_envs, a.num_drones = r, e, n
        a.seed, a.env_offset = SEED, env_offset
        self.args = a
        self.line = ref.DelayLine(e, n, values, probs, SEED, env_offset, ring_slots=r)

    def step(self, actions, step_count, episode):
        """(eff [E,N,3], delay_out [E], ring [R,E,N,3]) after one launch at the given host state."""
        self.actions.copy_(torch.from_numpy(actions).to(self.dev))
        self.step_count.copy_(_dev_i32(self.dev, step_count))
        self.episode.copy_(_dev_i32(self.dev, episode))
        self.nat.check(self.lib.swarm_actuate(ctypes.byref(self.args), _stream(self.dev)), self.lib, which="perturb")
        torch.cuda.synchronize(self.dev)
        assert self.ring.guards_intact() and self.eff.guards_intact() and self.delay_out.guards_intact()
        e, n, r = self.e, self.n, self.r
        return self.eff.host((e, n, 3)), self.delay_out.host((e,), np.int32), self.ring.host((r, e, n, 3))


def _actions(rng, e, n):
    return rng.uniform(-1.5, 1.5, (e, n, 3)).astype(np.float32)


def _unsorted_table(rng, r):
    """(values, probs): up to five distinct delays from [0, R), not in rising order."""
    count = min(r, 5)
    values = rng.permutation(r)[:count]
    while count > 1 and np.all(np.diff(values) > 0):
        values = rng.permutation(r)[:count]
    return [int(v) for v in values], rng.dirichlet(np.ones(count)).tolist()


def _thrust_sigmas(e):
    i = np.arange(e)
    return np.where(i % 2 == 0, 0.0, 0.03 * (1 + i % 5)).astype(np.float32)


def _stepped(dev, lib, e, n, r, steps, *, start, lengths, seed, env_offset, tag):
    """`steps` launches against DelayLine: eff (quiet envs bit for bit, also against a literally
    indexed history; the others under the bound), delay_out and the ring exact.  Env i starts at
    step_count start[i] and restarts at 0 with a new episode number after step lengths[i] - 1.
    Returns what occurred."""
    rng = np.random.default_rng(seed)
    values, probs = _unsorted_table(rng, r)
    override = np.full(e, -1, np.int32)
    override[0] = r - 1  # the longest delay the ring holds, on a quiet env that never restarts
    if e > 2:
        override[2] = 0
    sigma = _thrust_sigmas(e)
    act = Actuator(dev, lib, e, n, r, values, probs, env_offset=env_offset, override=override, sigma=sigma)
    sc = np.asarray(start, np.int64).copy()
    ep = rng.integers(0, 2**32, e).astype(np.uint32)
    ep[0] |= np.uint32(0x80000000)
    quiet = sigma == 0
    hist, seen = [], dict(delays=set(), zeroed=0, delayed=0, slots=set(), reread=set(), restarts=0, share=0.0, clip=False)
    written = {}  # (env, slot) -> the step it was last written at, this episode
    for t in range(steps):
        a = _actions(rng, e, n)
        delayed, want, bound, d = act.line.actuate(a, sc, ep, sigma, override)
        eff, d_got, ring = act.step(a, sc.astype(np.int32), ep)
        assert np.array_equal(d_got, d), (tag, t)
        assert np.array_equal(_bits(ring), _bits(act.line.ring)), (tag, t)
        assert np.array_equal(_bits(eff[quiet]), _bits(delayed[quiet])), (tag, t)
        err = np.abs(eff.astype(np.float64) - want)
        if (~quiet).any():
            seen["share"] = max(seen["share"], float(np.max(err[~quiet] / bound[~quiet])))
            assert np.all(err[~quiet] <= bound[~quiet]), (tag, t, seen["share"])
            assert np.abs(eff - delayed)[~quiet].max() > 1e-3
        clipped = np.clip(a, np.float32(-1), np.float32(1))
        seen["clip"] |= bool((np.abs(clipped) == 1).any())
        hist.append((ep.copy(), sc.copy(), clipped))
        for i in range(e):
            slot = int(sc[i] % r)
            if written.get((i, slot)) is not None:
                seen["slots"].add((i, slot, "rewritten"))
            written[i, slot] = t
            if 0 < d[i] <= sc[i]:
                seen["delayed"] += 1
                if sc[i] >= r:
                    seen["reread"].add((i, int((sc[i] - d[i]) % r)))  # read after the ring wrapped
            if not quiet[i]:
                continue
            if d[i] <= sc[i] and t - d[i] >= 0:  # the clipped command of d steps ago, whatever ring there is
                p_ep, p_sc, p_c = hist[t - d[i]]
                assert p_ep[i] == ep[i] and p_sc[i] == sc[i] - d[i]
                assert np.array_equal(_bits(eff[i]), _bits(p_c[i])), (tag, t, i)
            elif d[i] > sc[i]:
                seen["zeroed"] += 1
                assert not _bits(eff[i]).any(), (tag, t, i)
        seen["delays"] |= set(d.tolist())
        sc += 1
        for i in np.flatnonzero(sc >= np.asarray(lengths)):
            sc[i], ep[i] = 0, rng.integers(0, 2**32)
            seen["restarts"] += 1
            for slot in range(r):
                written.pop((int(i), slot), None)
    assert seen["clip"]
    return seen, values


@pytest.mark.parametrize("e,n", [(3, 256), (37, 7), (5, 1)], ids=["3x256", "37x7", "5x1"])
@pytest.mark.parametrize("r", [1, 3, 5, 6, 7, 8])
def test_actuate_ring_sizes(dev, lib, r, e, n):
    lanes = e * n
    assert (lanes, lanes % 256) in ((768, 0), (259, 3), (5, 5))  # whole workgroups, a ragged second one, one wave's corner
    steps = 2 * r + 5
    assert steps >= 2 * r + 3
    i = np.arange(e)
    start = i % 3  # the envs are at different steps
    lengths = np.where(i == 0, 10**9, r + 2 + i % 4)  # and restart at different times; env 0 never does
    seen, values = _stepped(dev, lib, e, n, r, steps, start=start, lengths=lengths, seed=1000 * r + lanes, env_offset=2**32 - 2,
                            tag=f"R={r} E={e} N={n}")
    assert sorted(values) != values or r == 1
    assert seen["restarts"] >= e - 1
    # env 0 holds the longest delay and never restarts: every slot of its ring is written again
    # after a wrap and read again after it
    assert {(0, s, "rewritten") for s in range(r)} <= seen["slots"]
    if r > 1:
        assert {(0, s) for s in range(r)} <= seen["reread"] and r - 1 in seen["delays"] and seen["zeroed"] > 0
        assert seen["delayed"] > 0 and len(seen["delays"]) >= 2
    else:
        assert seen["delays"] == {0}
    print(f"actuate R={r} E={e} N={n}: largest share of the bound used {seen['share']:.4f}")


@pytest.mark.parametrize("r", [3, 7])
def test_actuate_ring_index_far_from_zero(dev, lib, r):
    """Env 1 (noisy) and env 0 (quiet, delay R - 1) count up from 2^31 - 12 to 2^31 - 1: s % R and
    (s - d) % R for an R that is no power of two, where s & (R - 1) differs."""
    e, n, steps = 4, 2, 12
    first = 2**31 - 12
    assert first + steps - 1 == 2**31 - 1 and any((first + t) % r != (first + t) & (r - 1) for t in range(steps))
    start = np.array([first, first, 0, 1], np.int64)
    lengths = np.array([2**40, 2**40, r + 2, r + 3])
    seen, _ = _stepped(dev, lib, e, n, r, steps, start=start, lengths=lengths, seed=r, env_offset=9, tag=f"far R={r}")
    assert {(0, s) for s in range(r)} <= seen["reread"]
    print(f"actuate far from zero R={r}: largest share of the bound used {seen['share']:.4f}")


def _query(dev, lib, e, r, values, probs, episode, env_offset, override=None):
    """delay_out [E] of the actions == NULL path."""
    from swarm_marl_amd import _native as nat
    out = Arena(dev, e, dtype=torch.int32)
    step_count = torch.zeros(e, dtype=torch.int32, device=dev)
    d_episode = _dev_i32(dev, episode)
    d_override = None if override is None else torch.from_numpy(np.asarray(override, np.int32)).to(dev)
    a = nat.SwarmActuateArgs()
    a.step_count, a.episode, a.delay_out = step_count.data_ptr(), d_episode.data_ptr(), out.ptr()
    a.delay_override = None if override is None else d_override.data_ptr()
    _table(a, values, probs)
    a.ring_slots, a.num_envs, a.num_drones = r, e, 3
    a.seed, a.env_offset = SEED, env_offset
    nat.check(lib.swarm_actuate(ctypes.byref(a), _stream(dev)), lib, which="perturb")
    torch.cuda.synchronize(dev)
    assert out.guards_intact()
    return out.host((e,), np.int32)


# the eight-entry tables: the one with cum = [0, .2, .2, .5, .6, .6, 1, 1], whose first and last entries
# are never drawn, and one whose first and last entries are the likely ones
TABLES = {"inner": [0, 0.2, 0, 0.3, 0.1, 0, 0.4, 0], "ends": [0.4, 0, 0.3, 0.1, 0, 0, 0, 0.2]}


@pytest.mark.parametrize("name", list(TABLES))
def test_delay_table_with_eight_entries_and_zero_probabilities(dev, lib, name):
    e, env_offset = 4099, 2**32 - 2000
    values = [5, 2, 7, 0, 3, 6, 1, 4]
    probs = TABLES[name]
    assert sorted(values) == list(range(8)) and values != sorted(values)
    cum = ref.delay_cum(probs)
    if name == "inner":
        assert np.array_equal(cum, np.array([0, .2, .2, .5, .6, .6, 1, 1], np.float32))
    assert (np.diff(cum, prepend=np.float32(0)) == 0).sum() == 4 and cum[-1] == 1  # four entries are never drawn
    episode = np.random.default_rng(8).integers(0, 2**32, e).astype(np.uint32)
    want = ref.draw_delays(SEED, values, probs, env_offset + np.arange(e), episode)
    drawn = {v for v, p in zip(values, probs) if p > 0}
    assert set(want.tolist()) == drawn and len(drawn) == 4  # every positive entry, no zero-probability one
    got = _query(dev, lib, e, 8, values, probs, episode, env_offset)
    assert np.array_equal(got, want)
    # overrides win where they are >= 0, the rest still draw
    override = np.where(np.arange(e) % 3 == 0, np.arange(e) % 8, -1).astype(np.int32)
    want_o = ref.draw_delays(SEED, values, probs, env_offset + np.arange(e), episode, override)
    assert np.array_equal(_query(dev, lib, e, 8, values, probs, episode, env_offset, override), want_o)
    assert (want_o != want).any()
    # a single-entry table draws nothing
    one = _query(dev, lib, e, 8, [5], [1.0], episode, env_offset)
    assert np.array_equal(one, ref.draw_delays(SEED, [5], [1.0], env_offset + np.arange(e), episode)) and (one == 5).all()


def test_override_above_the_ring_is_clamped(dev, lib):
    """delay_override above ring_slots - 1, as a device-side set() may leave it: the delay is R - 1."""
    e, n, r, steps = 6, 3, 3, 8
    override = np.array([7, -1, 3, 2**31 - 1, 2, 0], np.int32)
    assert (override > r - 1).sum() == 3
    act = Actuator(dev, lib, e, n, r, [1, 0], [0.5, 0.5], override=override, sigma=np.zeros(e, np.float32))
    rng = np.random.default_rng(3)
    ep = rng.integers(0, 2**32, e).astype(np.uint32)
    hist = []
    for t in range(steps):
        sc = np.full(e, t, np.int64)
        a = _actions(rng, e, n)
        delayed, _, _, d = act.line.actuate(a, sc, ep, None, override)
        eff, d_got, ring = act.step(a, sc.astype(np.int32), ep)
        hist.append(np.clip(a, np.float32(-1), np.float32(1)))
        assert np.array_equal(d_got, d) and (d_got[override > r - 1] == r - 1).all() and d_got[4] == 2 and d_got[5] == 0
        assert np.array_equal(_bits(eff), _bits(delayed)) and np.array_equal(_bits(ring), _bits(act.line.ring))
        for i in np.flatnonzero(override > r - 1):  # the command of R - 1 steps ago
            past = hist[t - (r - 1)][i] if t >= r - 1 else np.zeros((n, 3), np.float32)
            assert np.array_equal(_bits(eff[i]), _bits(past)), (t, i)


def test_set_delay_from_a_device_tensor_is_clamped(dev):
    """`Perturbation.set(delay=<device tensor>)` is not range-checked on the host; the docstring
    promises the kernel's clamp."""
    from swarm_marl_amd import Perturbation, VecSwarm
    e, n = 4, 3
    vec = VecSwarm(e, dict(num_drones=n, max_steps=50), device=dev, auto_reset=True, seed=5)
    per = Perturbation(vec, dict(delay_values=[0, 1, 2], delay_probs=[0.5, 0.3, 0.2]), seed=SEED)
    assert per.max_delay == 2
    asked = [7, 2, 100, 1]
    per.set(delay=torch.tensor(asked, dtype=torch.int32, device=dev))
    vec.reset()
    assert _np(per.delays()).tolist() == [2, 2, 2, 1]
    rng = np.random.default_rng(2)
    hist, delayed = [], 0
    for t in range(6):
        sc, ep = _np(vec.step_count), _np(vec.episode)
        a = _actions(rng, e, n)
        hist.append((ep, sc, np.clip(a, np.float32(-1), np.float32(1))))
        per.step(torch.from_numpy(a).to(dev))
        eff = _np(per.eff)
        for i, d in enumerate([2, 2, 2, 1]):
            if d <= sc[i]:  # the command of d steps ago in the same episode
                p_ep, p_sc, p_c = hist[t - d]
                assert p_ep[i] == ep[i] and p_sc[i] == sc[i] - d
                assert np.array_equal(_bits(eff[i]), _bits(p_c[i])), (t, i)
                delayed += 1
            else:
                assert not _bits(eff[i]).any(), (t, i)
    assert delayed >= 8


def test_actuate_null_pointers(dev, lib):
    """delay_override NULL draws everywhere (an override of -1); thrust_noise_std NULL adds nothing
    (all zeros): eff is the delayed command; delay_out NULL changes nothing else."""
    e, n, r, steps = 9, 5, 4, 7
    values, probs = [2, 0, 3, 1], [0.25, 0.25, 0.25, 0.25]
    sigma = np.full(e, 0.05, np.float32)
    runs = dict(
        full=Actuator(dev, lib, e, n, r, values, probs, override=np.full(e, -1, np.int32), sigma=sigma),
        no_override=Actuator(dev, lib, e, n, r, values, probs, override=None, sigma=sigma),
        no_sigma=Actuator(dev, lib, e, n, r, values, probs, override=None, sigma=None),
        zero_sigma=Actuator(dev, lib, e, n, r, values, probs, override=None, sigma=np.zeros(e, np.float32)),
        no_delay_out=Actuator(dev, lib, e, n, r, values, probs, override=None, sigma=sigma, want_delays=False),
    )
    rng = np.random.default_rng(6)
    ep = rng.integers(0, 2**32, e).astype(np.uint32)
    seen, share = set(), 0.0
    for t in range(steps):
        sc = np.full(e, t, np.int64)
        a = _actions(rng, e, n)
        delayed, want, bound, d = runs["full"].line.actuate(a, sc, ep, sigma, None)
        out = {k: v.step(a, sc.astype(np.int32), ep) for k, v in runs.items()}
        eff, d_got, ring = out["full"]
        assert np.array_equal(d_got, d) and np.array_equal(_bits(ring), _bits(runs["full"].line.ring))
        err = np.abs(eff.astype(np.float64) - want)
        share = max(share, float(np.max(err / bound)))
        assert np.all(err <= bound), (t, share)
        for k in ("no_override", "no_delay_out"):
            assert np.array_equal(_bits(out[k][0]), _bits(eff)) and np.array_equal(_bits(out[k][2]), _bits(ring)), (k, t)
        assert np.array_equal(out["no_override"][1], d)
        assert runs["no_delay_out"].delay_out.unchanged()  # nothing written, the guards' pattern throughout
        for k in ("no_sigma", "zero_sigma"):
            assert np.array_equal(_bits(out[k][0]), _bits(delayed)) and np.array_equal(out[k][1], d), (k, t)
        assert not np.array_equal(eff, delayed)
        seen |= set(d.tolist())
    assert len(seen) >= 3  # the delays were drawn, not fixed
    print(f"actuate NULL pointers: largest share of the bound used {share:.4f}")
