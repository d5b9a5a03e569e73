"""NumPy definition of the actuation and sensing perturbations (the arithmetic in
include/swarm_mi355x.h), the yardstick of tests/test_perturb_cpu.py, tests/test_gpu_perturb.py and
tests/test_gpu_perturb_shapes.py.

Noise: Philox4x32-10 (oracle.swarm_oracle.philox4x32_10) with key (seed lo, seed hi) on the counter
(g, n | block << 16 | stream << 30, episode, step), g the low 32 bits of env_offset + e.  Normals are
formed as tests/policy_ref.py sample_noise64 forms them: the uniforms in f32 as the kernel forms
them (part of the definition), radius, angle (the kernel's f32 2 pi), cos and sin in float64.
Everything noisy is returned in float64 with its error bound; everything that must be untouched is
marked so, and is compared bit for bit.
"""
from __future__ import annotations

import numpy as np

from oracle.swarm_oracle import philox4x32_10
from tests.policy_ref import TWO_PI_F32

MAX_DELAY = 7
STREAM_ACT, STREAM_SENSE, STREAM_DELAY = 0, 1, 2
Z_BOUND = 1e-5      # |z - z_ref| <= Z_BOUND (1 + |z_ref|): the project's normal bound (tests/test_gpu_policy_dims.py)
ROUND = 2.0 ** -22  # a few f32 roundings of the result


def _words(seed, g, n, block, stream, episode, step):
    seed = int(seed) & (2**64 - 1)
    g, n, block, episode, step = np.broadcast_arrays(*(np.asarray(x, np.uint64) for x in (g, n, block, episode, step)))
    m32 = np.uint64(0xFFFFFFFF)
    w1 = n | (block << np.uint64(16)) | (np.uint64(stream) << np.uint64(30))
    return philox4x32_10(g & m32, w1 & m32, episode & m32, step & m32, seed & 0xFFFFFFFF, seed >> 32)


def normals(seed, g, n, block, stream, episode, step) -> np.ndarray:
    """z [4, ...] float64 of one Philox block: words (x0, x1) give z0, z1, words (x2, x3) z2, z3."""
    x = _words(seed, g, n, block, stream, episode, step)
    z = np.zeros((4,) + x[0].shape, np.float64)
    for p in range(2):
        n1 = (x[2 * p] >> np.uint32(8)).astype(np.float32)
        n2 = (x[2 * p + 1] >> np.uint32(8)).astype(np.float32)
        u1 = ((n1 + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float64)
        u2 = (n2 * np.float32(2.0 ** -24)).astype(np.float64)
        rad = np.sqrt(-2.0 * np.log(u1))
        ang = np.float64(TWO_PI_F32) * u2
        z[2 * p] = rad * np.cos(ang)
        z[2 * p + 1] = rad * np.sin(ang)
    return z


def delay_cum(probs) -> np.ndarray:
    """The float32 rounding of the float64 running sum of the probs, the last entry forced to 1."""
    cum = np.zeros(len(probs), np.float32)
    run = np.float64(0.0)
    for i, p in enumerate(probs):
        run = run + np.float64(p)
        cum[i] = np.float32(run)
    cum[-1] = np.float32(1.0)
    return cum


def draw_delays(seed, values, probs, g, episode, override=None) -> np.ndarray:
    """d [E] int32: values[i] for the first i with u < cum[i], u = (x0 >> 8) 2^-24 of the block
    (g, stream 2, episode, 0); override[e] >= 0 wins."""
    x0 = _words(seed, g, 0, 0, STREAM_DELAY, episode, 0)[0]
    u = (x0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    cum = delay_cum(probs)
    d = np.zeros(u.shape, np.int32)
    for e in range(u.size):
        d[e] = values[int(np.argmax(u[e] < cum))]  # the first True; cum[-1] = 1 > u
    if override is not None:
        override = np.asarray(override, np.int32)
        d = np.where(override >= 0, override, d).astype(np.int32)
    return d


class DelayLine:
    """The delay line and thrust noise of a batch, restated literally: a ring [R, E, N, 3] f32."""

    def __init__(self, e, n, values, probs, seed, env_offset=0, ring_slots=None):
        self.values, self.probs, self.seed, self.env_offset = list(values), list(probs), seed, env_offset
        self.r = max(values) + 1 if ring_slots is None else ring_slots
        self.ring = np.zeros((self.r, e, n, 3), np.float32)
        self.e, self.n = e, n

    def actuate(self, actions, step_count, episode, sigma_t=None, override=None):
        """(delayed [E,N,3] f32 exact, eff_ref [E,N,3] float64, bound [E,N,3], d [E])."""
        e, n = self.e, self.n
        g = self.env_offset + np.arange(e)
        ep = np.asarray(episode).astype(np.int64) & 0xFFFFFFFF
        s = np.asarray(step_count, np.int64)
        d = np.minimum(draw_delays(self.seed, self.values, self.probs, g, ep, override), self.r - 1)
        c = np.clip(np.asarray(actions, np.float32), np.float32(-1), np.float32(1))
        delayed = np.zeros((e, n, 3), np.float32)
        for i in range(e):
            self.ring[s[i] % self.r, i] = c[i]
            if d[i] <= s[i]:
                delayed[i] = self.ring[(s[i] - d[i]) % self.r, i]
        sig = np.zeros(e, np.float32) if sigma_t is None else np.asarray(sigma_t, np.float32)
        z = normals(self.seed, g[:, None], np.arange(n)[None, :], 0, STREAM_ACT, ep[:, None], s[:, None])[:3]
        z = np.moveaxis(z, 0, -1)  # [E, N, 3]
        sg = sig.astype(np.float64)[:, None, None]
        ref = delayed.astype(np.float64) + sg * z
        bound = np.where(sg != 0, sg * Z_BOUND * (1 + np.abs(z)) + ROUND * np.abs(ref), 0.0)
        return delayed, ref, bound, d


def sense(obs, active, sigma_p, sigma_v, sigma_o, step_count, episode, seed, env_offset, k, ms):
    """(ref [E,N,D] float64, bound [E,N,D] float64, touched [E,N,D] bool) for obs [E,N,D] f32.
    Where touched is False the output is obs bit for bit (bound 0).  A sigma may be None: the NULL
    pointer of the ABI, no noise in that group, as a zero sigma."""
    sigma_p, sigma_v, sigma_o = (0.0 if x is None else x for x in (sigma_p, sigma_v, sigma_o))
    obs = np.asarray(obs, np.float32)
    e, n, dim = obs.shape
    assert dim == 9 + 4 * k + 4 * ms
    ref = obs.astype(np.float64)
    bound = np.zeros_like(ref)
    touched = np.zeros(obs.shape, bool)
    g = (env_offset + np.arange(e))[:, None]
    ag = np.arange(n)[None, :]
    ep = (np.asarray(episode).astype(np.int64) & 0xFFFFFFFF)[:, None]
    st = (np.asarray(step_count).astype(np.int64) & 0xFFFFFFFF)[:, None]
    act = np.asarray(active).astype(bool)
    sp, sv, so = (np.broadcast_to(np.asarray(x, np.float32), (e,)).astype(np.float64)[:, None] for x in
                  (sigma_p, sigma_v, sigma_o))

    def zb(sig, z):
        return sig * Z_BOUND * (1 + np.abs(z))

    def put(col, val, bnd, mask):
        ref[..., col] = np.where(mask, val, ref[..., col])
        bound[..., col] = np.where(mask, bnd + ROUND * np.abs(val), 0.0)
        touched[..., col] = mask

    z0 = normals(seed, g, ag, 0, STREAM_SENSE, ep, st)
    z1 = normals(seed, g, ag, 1, STREAM_SENSE, ep, st)
    for c in range(3):
        m = act & (sp != 0)
        put(c, ref[..., c] + sp * z0[c], zb(sp, z0[c]), m)
        put(6 + c, ref[..., 6 + c] - sp * z0[c], zb(sp, z0[c]), m)
        put(3 + c, ref[..., 3 + c] + sv * z1[c], zb(sv, z1[c]), act & (sv != 0))
    for j in range(k):
        o = 9 + 4 * j
        z = normals(seed, g, ag, 2 + j, STREAM_SENSE, ep, st)
        m = act & (sp != 0) & (obs[..., o:o + 4] != 0).any(-1)
        comp = np.zeros((e, n))
        for c in range(3):
            put(o + c, ref[..., o + c] + sp * z[c], zb(sp, z[c]), m)
            comp = comp + bound[..., o + c]
        dist = np.sqrt(ref[..., o] ** 2 + ref[..., o + 1] ** 2 + ref[..., o + 2] ** 2)
        put(o + 3, dist, comp, m)
    for j in range(ms):
        o = 9 + 4 * k + 4 * j
        z = normals(seed, g, ag, 2 + k + j, STREAM_SENSE, ep, st)
        m = act & (so != 0) & (obs[..., o:o + 4] != 0).any(-1)
        put(o + 3, np.maximum(ref[..., o + 3] + so * z[0], 0.0), zb(so, z[0]), m)
    return ref, bound, touched
