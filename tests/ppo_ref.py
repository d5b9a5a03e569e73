"""Reference for the PPO loss head (include/swarm_mi355x.h, "PPO loss head").

`loss` is RLlib's PPOTorchPolicy.loss written with torch ops (torch.minimum, torch.clamp, a masked
mean, the env-row value expanded to its agents) in whatever dtype and on whatever device its
inputs have: float64 on the CPU with autograd is the reference of the kernel tests, float32 on the
GPU the eager chain the autograd test and tools/ppo_time.py compare with.  `closed_form_grads`
evaluates the gradient formulas the kernel is held to (NumPy float64); `moments` is RLlib's
standardized() statistics in NumPy float64.  `make_case` draws the inputs of a kernel test.

`check_head` is the comparison of every GPU head test with its bounds, here so that the CPU tests
can show that it rejects a wrong kernel: `head_model` is the header's formulas on all rows at once
(NumPy float64), optionally with one of `FAULTS` built in.  `shape_cases` / `SECOND_PASS` list the
width, tile-edge and coefficient sweep of tests/test_gpu_ppo_shapes.py.  `exact_case` draws inputs
on which every number the head forms is exactly representable; `check_exact` compares bits.
"""
from __future__ import annotations

import math

import numpy as np
import torch

COEF = dict(clip_param=0.3, vf_clip_param=10.0, vf_loss_coeff=1.0, entropy_coeff=0.0, kl_coeff=0.2)
STATS = ("count", "total_loss", "policy_loss", "vf_loss", "entropy", "kl", "clip_frac")


def moments(x, valid):
    """(count, mean, population std, 1 / max(std, 1e-4)) over valid rows; mean 0 / 1e4 with none."""
    sel = np.asarray(x, np.float64).reshape(-1)[np.asarray(valid).reshape(-1) != 0]
    if sel.size == 0:
        return np.array([0.0, 0.0, 0.0, 1e4])
    sd = sel.std()
    return np.array([float(sel.size), sel.mean(), sd, 1.0 / max(sd, 1e-4)])


ILL_CONDITIONED = ((1e4, 1e-2, 70_002), (-3e5, 0.5, 70_003))  # (mean, std, rows): |mean| >= 6e5 std


def moments_data(mean, sd, rows):
    """(x float32 [rows], valid [rows], ~80 % set) drawn from N(mean, sd): the moments tests' ill-conditioned data."""
    rng = np.random.default_rng(rows)
    return rng.normal(mean, sd, rows).astype(np.float32), rng.random(rows) < 0.8


def loss(logits, value, behaviour_logits, actions, logp, advantage, value_target, valid, adv_mean, adv_inv_std, *,
         clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff):
    """(total, stats dict of tensors, per-row ratio, per-row squared value error).  logits [R,2A],
    value [R/N]; rows with valid == 0 are replaced by benign numbers before any arithmetic and
    masked out of every mean."""
    r_, a2 = logits.shape
    a = a2 // 2
    n = r_ // value.numel()
    m = valid.reshape(-1) != 0
    mf = m.to(logits.dtype)
    count = mf.sum()

    def clean(x, fill=0.0):
        mask = m.reshape((-1,) + (1,) * (x.dim() - 1))
        return torch.where(mask, x, torch.full_like(x, fill))

    logits, behaviour_logits, actions = clean(logits), clean(behaviour_logits), clean(actions)
    logp, advantage, value_target = clean(logp), clean(advantage), clean(value_target)
    mu, ls = logits[:, :a], logits[:, a:]
    mu0, ls0 = behaviour_logits[:, :a], behaviour_logits[:, a:]
    new = torch.distributions.Normal(mu, torch.exp(ls))
    old = torch.distributions.Normal(mu0, torch.exp(ls0))
    lp = new.log_prob(actions).sum(-1)
    ratio = torch.exp(lp - logp)
    adv = (advantage - adv_mean) * adv_inv_std
    s1 = adv * ratio
    s2 = adv * torch.clamp(ratio, 1.0 - clip_param, 1.0 + clip_param)
    surr = torch.minimum(s1, s2)
    v_agent = value.reshape(-1, 1).expand(-1, n).reshape(-1)
    err2 = (v_agent - value_target) ** 2
    vf = torch.clamp(err2, max=vf_clip_param)
    ent = new.entropy().sum(-1)
    kl = torch.distributions.kl_divergence(old, new).sum(-1)

    def mean_valid(x):
        return (x * mf).sum() / count

    stats = dict(count=count, policy_loss=mean_valid(-surr), vf_loss=mean_valid(vf), entropy=mean_valid(ent),
                 kl=mean_valid(kl), clip_frac=mean_valid((s2 < s1).to(logits.dtype)))
    total = mean_valid(-surr + vf_loss_coeff * vf - entropy_coeff * ent + kl_coeff * kl)
    stats["total_loss"] = total
    return total, stats, ratio, err2


def closed_form_grads(logits, value, behaviour_logits, actions, logp, advantage, value_target, valid, adv_mean,
                      adv_inv_std, *, clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff):
    """(grad_logits [R,2A], grad_value [R/N]) of the mean loss by the formulas of the issue, NumPy f64."""
    f = lambda x: np.asarray(x, np.float64)  # noqa: E731
    logits, b, act = f(logits), f(behaviour_logits), f(actions)
    a = act.shape[1]
    n = logits.shape[0] // np.asarray(value).size
    m = np.asarray(valid).reshape(-1) != 0
    inv = 1.0 / m.sum()
    g = np.zeros_like(logits)
    gv = np.zeros(np.asarray(value).size)
    for i in np.nonzero(m)[0]:
        mu, s, mu0, s0 = logits[i, :a], logits[i, a:], b[i, :a], b[i, a:]
        z = (act[i] - mu) * np.exp(-s)
        lp = np.sum(-0.5 * z * z - s) - 0.5 * a * math.log(2 * math.pi)
        r = math.exp(lp - float(logp[i]))
        adv = (float(advantage[i]) - adv_mean) * adv_inv_std
        blocked = (adv > 0 and r > 1 + clip_param) or (adv < 0 and r < 1 - clip_param)
        w = 0.0 if blocked else -adv * r
        u = np.exp(2 * s0) + (mu0 - mu) ** 2
        g[i, :a] = inv * (w * z * np.exp(-s) + kl_coeff * (mu - mu0) * np.exp(-2 * s))
        g[i, a:] = inv * (w * (z * z - 1) - entropy_coeff + kl_coeff * (1 - u * np.exp(-2 * s)))
        d = float(value[i // n]) - float(value_target[i])
        if d * d < vf_clip_param:
            gv[i // n] += inv * vf_loss_coeff * 2 * d
    return g, gv


def make_case(env_rows: int, n: int, a: int, seed: int, coef=None, *, target_spread: float = 3.0):
    """float32 NumPy inputs of a head test: log-std in [-2, 0.5], new logits = behaviour + N(0, 0.15),
    ~20 % of the rows invalid (a tenth of the env-rows wholly), targets `target_spread` around the
    values so that some rows reach vf_clip_param.  A row whose ratio falls within 2e-3 of a clip
    boundary 1 +- clip_param, or whose squared value error within 2e-3 of vf_clip_param, is moved off
    it (behaviour logp + 0.02, target + 0.05 away from the value): a float32 kernel and a float64
    reference may not take different branches there, and no seed keeps 16,640 rows clear of both."""
    coef = coef or COEF
    rng = np.random.default_rng(seed)
    r = env_rows * n
    mu0 = rng.uniform(-1, 1, (r, a))
    ls0 = rng.uniform(-2, 0.5, (r, a))
    behaviour = np.concatenate([mu0, ls0], 1).astype(np.float32)
    logits = (behaviour + rng.normal(0, 0.15, (r, 2 * a))).astype(np.float32)
    actions = (mu0 + np.exp(ls0) * rng.normal(0, 1, (r, a))).astype(np.float32)
    b64 = behaviour.astype(np.float64)
    z = (actions - b64[:, :a]) * np.exp(-b64[:, a:])
    logp = (np.sum(-0.5 * z * z - b64[:, a:], 1) - 0.5 * a * math.log(2 * math.pi)).astype(np.float32)
    advantage = rng.normal(0.3, 2.0, r).astype(np.float32)
    value = rng.normal(0, 1, env_rows).astype(np.float32)
    value_target = (np.repeat(value, n) + rng.normal(0, target_spread, r)).astype(np.float32)
    valid = rng.random(r) < 0.85
    dead = rng.random(env_rows) < 0.1
    dead[0] = False
    if env_rows > 1:
        dead[env_rows // 2] = True
    valid &= ~np.repeat(dead, n)
    valid[0] = True  # never an empty batch
    l64 = logits.astype(np.float64)
    zn = (actions - l64[:, :a]) * np.exp(-l64[:, a:])
    lp_new = np.sum(-0.5 * zn * zn - l64[:, a:], 1) - 0.5 * a * math.log(2 * math.pi)
    ratio = np.exp(lp_new - logp)
    near = np.minimum(np.abs(ratio - (1 + coef["clip_param"])), np.abs(ratio - (1 - coef["clip_param"]))) < 2e-3
    logp = np.where(near, logp + np.float32(0.02), logp).astype(np.float32)
    d = np.repeat(value, n).astype(np.float64) - value_target
    near = np.abs(d * d - coef["vf_clip_param"]) < 2e-3
    value_target = np.where(near, value_target - np.sign(d).astype(np.float32) * np.float32(0.05), value_target).astype(np.float32)
    return dict(logits=logits, value=value, behaviour_logits=behaviour, actions=actions, logp=logp,
                advantage=advantage, value_target=value_target, valid=valid)


def reference(case, coef):
    """float64 CPU reference of a make_case() dict: dict(total, stats, grad_logits, grad_value, ratio, err2,
    adv_moments).  The advantages are standardised with the moments of the case's own valid rows;
    without a valid row (mean 0, inverse 1e4) the means are 0 / 0: use `head_model` there."""
    t = {k: torch.from_numpy(np.asarray(v, np.float64 if v.dtype != bool else bool)) for k, v in case.items()}
    mom = moments(case["advantage"], case["valid"])
    lg = t["logits"].clone().requires_grad_(True)
    val = t["value"].clone().requires_grad_(True)
    total, stats, ratio, err2 = loss(lg, val, t["behaviour_logits"], t["actions"], t["logp"], t["advantage"],
                                     t["value_target"], t["valid"], float(mom[1]), float(mom[3]), **coef)
    total.backward()
    return dict(total=float(total.detach()), stats={k: float(v.detach()) for k, v in stats.items()}, grad_logits=lg.grad.numpy(),
                grad_value=val.grad.numpy(), ratio=ratio.detach().numpy(), err2=err2.detach().numpy(), adv_moments=mom)


# ---------------------------------------------------------------- the comparison of the GPU tests
GRAD_BOUND, STATS_BOUND, BAND = 2e-5, 1e-5, 1e-3


def check_head(case, coef, ref, stats, gl, gv, *, require_dead=True, label=""):
    """The comparison every head test makes (tests/test_gpu_ppo.py's docstring derives the bounds):
    `stats` [7] f64, `gl` [R,2A] and `gv` [env_rows] of a launch against a `reference` / `head_model`
    dict.  Asserts the 1e-3 band conditions on the reference, the exact valid and clipped counts,
    gradients within 2e-5 (|ref| + max|ref|), stats within 1e-5 max(1, |ref|), exact zeros on invalid
    rows and on env-rows without a valid agent.  Returns the three maximum errors."""
    v, c = np.asarray(case["valid"]).reshape(-1) != 0, coef["clip_param"]
    env_rows = np.asarray(case["value"]).size
    n = v.size // env_rows
    a = gl.shape[1] // 2
    r, e2 = ref["ratio"][v], ref["err2"][v]
    assert np.minimum(np.abs(r - (1 + c)), np.abs(r - (1 - c))).min() >= BAND
    assert np.abs(e2 - coef["vf_clip_param"]).min() >= BAND
    rs = ref["stats"]
    want = np.array([rs[k] for k in STATS])
    gl_err = np.abs(gl - ref["grad_logits"]) / (np.abs(ref["grad_logits"]) + np.abs(ref["grad_logits"]).max())
    gv_den = np.abs(ref["grad_value"]) + np.abs(ref["grad_value"]).max()
    gv_err = np.abs(gv - ref["grad_value"]) / np.where(gv_den > 0, gv_den, 1.0)
    st_err = np.abs(stats - want) / np.maximum(1.0, np.abs(want))
    print(f"head{label} A={a} N={n} env_rows={env_rows}: grad_logits {gl_err.max():.2e} grad_value {gv_err.max():.2e} "
          f"(bound 2e-5) stats {st_err.max():.2e} (bound 1e-5) clipped {rs['clip_frac'] * rs['count']:.0f}/{rs['count']:.0f}")
    assert stats[0] == v.sum() == rs["count"]
    clipped = stats[6] * stats[0]
    assert abs(clipped - round(clipped)) < 1e-6 and round(clipped) == round(rs["clip_frac"] * rs["count"])
    assert gl_err.max() <= GRAD_BOUND and gv_err.max() <= GRAD_BOUND
    assert st_err.max() <= STATS_BOUND
    assert np.all(gl[~v] == 0)
    dead = ~v.reshape(env_rows, n).any(1)
    assert np.all(gv[dead] == 0) and (dead.any() or env_rows == 1 or not require_dead)
    return dict(grad_logits=float(gl_err.max()), grad_value=float(gv_err.max()), stats=float(st_err.max()))


def check_empty(stats, loss, gl, gv):
    """The header's "with M == 0 every gradient and stats [1..6] are 0" (and the count is 0)."""
    assert np.array_equal(stats, np.zeros(len(STATS))), stats
    assert np.isfinite(loss) and loss == 0.0, loss
    assert np.array_equal(gl, np.zeros_like(gl)) and np.array_equal(gv, np.zeros_like(gv))


# ---------------------------------------------------------------- the head's formulas, vectorised, with faults
C2 = dict(clip_param=0.2, vf_clip_param=4.0, vf_loss_coeff=0.5, entropy_coeff=0.02, kl_coeff=0.0)
C3 = dict(clip_param=0.1, vf_clip_param=1.0, vf_loss_coeff=2.0, entropy_coeff=0.0, kl_coeff=1.0)
MAX_BLOCKS = 1024  # SWARM_PPO_MAX_BLOCKS: tiles past it are a workgroup's second pass
THREADS = 256      # rows of a tile: G = max(1, THREADS // N) whole env-rows
GROUP = 16         # agents of one group sum of the value gradient

FAULTS = (
    "vf_grad_ignores_coeff",      # vf_loss_coeff dropped from g_row
    "vf_total_ignores_coeff",     # vf_loss_coeff dropped from stats[1]
    "clip_fixed_at_0.3",          # the clip band hard-coded
    "no_entropy_grad",            # the entropy term dropped from the log-std gradient
    "no_kl_logstd_grad",          # the KL term dropped from the log-std gradient
    "vf_clip_le",                 # <= instead of < at the value clip
    "group_last_agent_lost",      # agent 16 j + 15 of every group left out of grad_value
    "last_agent_lost",            # agent N - 1 left out of grad_value when N is no multiple of 16
    "tile_last_env_row_lost",     # the last env-row of every tile not worked on when 256 % N != 0 (G > 1)
    "partial_last_tile_skipped",  # a last tile with fewer than G env-rows not worked on
    "second_pass_skipped",        # tiles 1,024 and up not worked on
    "inv_from_row_count",         # inv = 1 / R instead of 1 / M
    "empty_batch_nan",            # M == 0: inv = 0 / 0
)


def tiles_of(env_rows: int, n: int):
    """(G, tile index of every env-row): a workgroup's tile is G = max(1, 256 // N) whole env-rows."""
    g = max(1, THREADS // n)
    return g, np.arange(env_rows) // g


def head_model(case, coef, adv_mean, adv_inv_std, *, fault=None):
    """The header's formulas ("PPO loss head") on every row at once in NumPy float64, each expression
    associated as the header writes it: the same dict as `reference` (stats, grad_logits,
    grad_value, ratio, err2, total) plus `stats_vec`.  Unlike the autograd reference it takes the
    header's side at a tie (strict `<` at vf_clip_param: torch.clamp's gradient is non-strict) and
    is defined without a valid row.  `fault`: one of FAULTS, the outputs a kernel with that defect
    would write; rows it does not work on get zeros and leave every sum."""
    assert fault is None or fault in FAULTS, fault
    f = lambda k: np.asarray(case[k], np.float64)  # noqa: E731
    m = np.asarray(case["valid"]).reshape(-1) != 0
    rows = m.size
    value = f("value").reshape(-1)
    env_rows = value.size
    n = rows // env_rows
    a = np.asarray(case["actions"]).shape[-1]

    def clean(k):
        x = f(k).reshape(rows, -1)
        return np.where(m[:, None], x, 0.0)

    lg, b, act = clean("logits"), clean("behaviour_logits"), clean("actions")
    logp, advantage, target = clean("logp")[:, 0], clean("advantage")[:, 0], clean("value_target")[:, 0]
    count = float(m.sum())
    if fault == "empty_batch_nan" and count == 0:
        nan = np.full(len(STATS), np.nan)
        nan[0] = 0.0
        return dict(total=np.nan, stats=dict(zip(STATS, nan)), stats_vec=nan, grad_logits=np.full((rows, 2 * a), np.nan),
                    grad_value=np.full(env_rows, np.nan), ratio=np.ones(rows), err2=np.zeros(rows))
    inv = 1.0 / (rows if fault == "inv_from_row_count" else count) if count > 0 else 0.0
    g_tile, tile_of_env = tiles_of(env_rows, n)
    env = np.arange(rows) // n
    done = m.copy()  # the rows the kernel works on
    if fault == "tile_last_env_row_lost" and THREADS % n and g_tile > 1:
        done &= env % g_tile != g_tile - 1
    if fault == "partial_last_tile_skipped" and env_rows % g_tile:
        done &= tile_of_env[env] != tile_of_env[-1]
    if fault == "second_pass_skipped":
        done &= tile_of_env[env] < MAX_BLOCKS
    c = 0.3 if fault == "clip_fixed_at_0.3" else coef["clip_param"]
    vf_clip, c_v, c_e, c_kl = coef["vf_clip_param"], coef["vf_loss_coeff"], coef["entropy_coeff"], coef["kl_coeff"]
    mu, s, mu0, s0 = lg[:, :a], lg[:, a:], b[:, :a], b[:, a:]
    e = np.exp(-s)
    z = (act - mu) * e
    lp = np.sum(-0.5 * z * z - s, 1) - 0.5 * a * math.log(2 * math.pi)
    r = np.exp(lp - logp)
    adv = (advantage - adv_mean) * adv_inv_std
    surr = np.minimum(adv * r, adv * np.clip(r, 1 - c, 1 + c))
    clipped = ((adv > 0) & (r > 1 + c)) | ((adv < 0) & (r < 1 - c))
    d = np.where(m, np.repeat(value, n), 0.0) - target
    d2 = d * d
    inside = d2 <= vf_clip if fault == "vf_clip_le" else d2 < vf_clip
    g_row = np.where(done & inside, inv * (1.0 if fault == "vf_grad_ignores_coeff" else c_v) * 2.0 * d, 0.0)
    k = np.arange(rows) % n
    if fault == "group_last_agent_lost":
        g_row[k % GROUP == GROUP - 1] = 0.0
    if fault == "last_agent_lost" and n % GROUP:
        g_row[k == n - 1] = 0.0
    gv = g_row.reshape(env_rows, n).sum(1)
    w = np.where(clipped, 0.0, -(adv * r))[:, None]
    ee = e * e
    u = np.exp(2 * s0) + (mu0 - mu) ** 2
    g_mu = inv * (w * z * e + c_kl * (mu - mu0) * ee)
    ent_term = 0.0 if fault == "no_entropy_grad" else c_e
    kl_term = 0.0 if fault == "no_kl_logstd_grad" else c_kl * (1.0 - u * ee)
    g_ls = inv * ((w * (z * z - 1.0) - ent_term) + kl_term)
    gl = np.where(done[:, None], np.concatenate([g_mu, g_ls], 1), 0.0)
    ent = s.sum(1) + 0.5 * a * (math.log(2 * math.pi) + 1.0)
    kl = np.sum(((s - s0) + 0.5 * u * ee) - 0.5, 1)
    mean = lambda x: inv * float(np.sum(x[done]))  # noqa: E731
    pol, vf, h, klm = mean(-surr), mean(np.minimum(d2, vf_clip)), mean(ent), mean(kl)
    total = ((pol + (1.0 if fault == "vf_total_ignores_coeff" else c_v) * vf) - c_e * h) + c_kl * klm
    vec = np.array([float(done.sum()), total, pol, vf, h, klm, mean(clipped.astype(np.float64))])
    return dict(total=total, stats=dict(zip(STATS, vec)), stats_vec=vec, grad_logits=gl, grad_value=gv, ratio=r, err2=d2)


def shape_cases():
    """[(a, n, env_rows, coef name)] of the width / tile-edge / coefficient sweep: A in {2, 4, 5} (the
    instantiations the first tests never launched) x N at the edges of the 16-agent groups, of G
    (128 -> 129: 2 -> 1, 85 -> 86: 3 -> 2) and of the idle lanes (255: one, 86: 84) x env_rows in
    {1, G, G + 1, 65}; C2 and C3 alternate over N and env_rows so that every A and every N meets both."""
    out = []
    for a in (2, 4, 5):
        for i_n, n in enumerate((15, 16, 17, 31, 32, 33, 85, 86, 128, 129, 255)):
            g = max(1, THREADS // n)
            seen = set()
            for ie, env_rows in enumerate((1, g, g + 1, 65)):
                if env_rows not in seen:
                    seen.add(env_rows)
                    out.append((a, n, env_rows, "C2" if (i_n + ie) % 2 else "C3"))
    return out


# (a, n, env_rows, coef name): the smallest launches whose tiles outnumber the 1,024 workgroups
SECOND_PASS = ((2, 64, 4 * 1024 + 3, "C2"),     # G = 4: 1,025 tiles, the last one partial (3 of 4 env-rows)
               (4, 3, 85 * 1024 + 7, "C2"),     # G = 85, one idle lane
               (5, 1, 256 * 1024 + 300, "C3"))  # G = 256: the per-agent critic's mode, two tiles past the grid


def seed_of(a, n, env_rows):
    return 1000 * a + 10 * n + env_rows


# ---------------------------------------------------------------- the exact fixture
EXACT_COEF = dict(clip_param=0.25, vf_clip_param=4.0, vf_loss_coeff=0.5, entropy_coeff=0.125, kl_coeff=0.25)
EXACT_MOMENTS = (0.5, 0.5, 2.0)  # mean, std, inverse std handed to the head: adv = 2 (advantage - 0.5)
EXACT_SHAPES = ((1, 6), (3, 2), (17, 5), (64, 4), (86, 3), (255, 1))  # (N, A), at env_rows G + 1 and 65
EXACT_SECOND_PASS = (4 * 1024 + 3, 64, 2)  # (env_rows, N, A)


def logp_f32(logits, actions):
    """swarm_gaussian_logp's expression (the head's `lp`) operation by operation in NumPy float32."""
    lg, act = np.asarray(logits, np.float32), np.asarray(actions, np.float32)
    a = act.shape[1]
    s = np.zeros(act.shape[0], np.float32)
    for k in range(a):
        ls = lg[:, a + k]
        z = (act[:, k] - lg[:, k]) * np.exp(-ls)
        s = s + (np.float32(-0.5) * z * z - ls)
    return s - np.float32(0.5) * np.float32(a) * np.float32(1.8378770664093453)


def exact_case(env_rows: int, n: int, a: int, seed: int):
    """A head input on which every number the kernel forms is exactly representable in float32 (and
    every sum in float64), so its outputs are compared bit for bit and no summation order matters.

    Log-stds 0 (e = 1); means multiples of 1/8 in [-2, 2], behaviour means off by multiples of 1/8 in
    [-1/2, 1/2], actions the mean plus a multiple of 1/8 in [-2, 2]; advantages multiples of 1/4 with
    the moments handed in as (0.5, 0.5, 2) so that adv = 2 (advantage - 0.5); values multiples of 1/4
    in [-2, 2], targets off by multiples of 1/4 in [-3, 3]: with vf_clip_param 4 many rows sit exactly
    at d^2 == vf_clip_param, where the header's strict `<` decides.  About 80 % of the rows are valid,
    trimmed to a power of two (inv exact), with one env-row wholly invalid.  Half the rows are
    on-policy: their behaviour log-prob is the library's own gaussian_logp of (logits, actions), so
    lp - logp == 0 and r == 1.  The others get that log-prob -1 with adv > 0 or +1 with adv < 0:
    r ~ e or 1/e, clipped, w = 0 and surr = adv (1 +- 0.25).

    Returns (case, extra): `case` like make_case's, its logp the float32 emulation (`logp_f32`) plus
    `extra["logp_offset"]` — a GPU test replaces it by the device's; extra["logp_exact"] is the
    float64 log-prob plus the offset, for the reference."""
    rng = np.random.default_rng(seed)
    r = env_rows * n
    step = lambda lo, hi, shape, q: rng.integers(lo, hi + 1, shape) / q  # noqa: E731
    mu = step(-16, 16, (r, a), 8.0)
    mu0 = mu + step(-4, 4, (r, a), 8.0)
    actions = mu + step(-16, 16, (r, a), 8.0)
    zeros = np.zeros((r, a))
    value = step(-8, 8, env_rows, 4.0)
    target = np.repeat(value, n) + step(-12, 12, r, 4.0)
    advantage = step(-12, 12, r, 4.0)
    valid = rng.random(r) < 0.8
    if env_rows > 1:
        valid.reshape(env_rows, n)[env_rows // 2] = False
    valid[0] = True
    idx = np.nonzero(valid)[0]
    keep = 1 << (idx.size.bit_length() - 1)
    valid[rng.choice(idx, idx.size - keep, replace=False)] = False
    idx = np.nonzero(valid)[0]
    offset = np.where(rng.random(r) < 0.5, 0.0, np.where(rng.random(r) < 0.5, -1.0, 1.0))
    if idx.size >= 4:  # every kind of row at every shape
        offset[idx[:3]] = (0.0, -1.0, 1.0)
        target[idx[0]] = value[idx[0] // n] - 2.0   # d^2 == vf_clip_param
        target[idx[1]] = value[idx[1] // n] + 2.25  # above it
        target[idx[3]] = value[idx[3] // n] + 0.5   # below it
    dist = np.abs(advantage - 0.5)
    dist = np.where(dist == 0, 0.25, dist)
    advantage = np.where(offset < 0, 0.5 + dist, np.where(offset > 0, 0.5 - dist, advantage))  # clipped: adv > 0 / < 0
    f32 = lambda x: np.asarray(x, np.float64).astype(np.float32)  # noqa: E731
    logits, behaviour = f32(np.concatenate([mu, zeros], 1)), f32(np.concatenate([mu0, zeros], 1))
    z = actions - mu
    exact = np.sum(-0.5 * z * z, 1) - 0.5 * a * math.log(2 * math.pi)
    case = dict(logits=logits, value=f32(value), behaviour_logits=behaviour, actions=f32(actions),
                logp=logp_f32(logits, f32(actions)) + f32(offset), advantage=f32(advantage), value_target=f32(target),
                valid=valid)
    for k, v in (("logits", np.concatenate([mu, zeros], 1)), ("actions", actions), ("advantage", advantage),
                 ("value_target", target), ("value", value)):
        assert np.array_equal(case[k], v), k  # nothing was rounded
    return case, dict(logp_offset=f32(offset), logp_exact=exact + offset, adv_moments=np.array([float(keep), *EXACT_MOMENTS]))


def exact_reference(case, extra, coef=None, *, fault=None):
    """`head_model` of an exact_case with the float64 log-prob, plus the row counts the fixture promises
    (on-policy, clipped, exactly at vf_clip_param, above it; valid rows only)."""
    coef = coef or EXACT_COEF
    ref = head_model(dict(case, logp=extra["logp_exact"]), coef, EXACT_MOMENTS[0], EXACT_MOMENTS[2], fault=fault)
    v = case["valid"]
    adv = (case["advantage"].astype(np.float64) - 0.5) * 2.0
    r, c = ref["ratio"], coef["clip_param"]
    blocked = ((adv > 0) & (r > 1 + c)) | ((adv < 0) & (r < 1 - c))
    ref["rows"] = dict(on_policy=int((v & (r == 1.0)).sum()), clipped=int((v & blocked).sum()),
                       unblocked_off_policy=int((v & (r != 1.0) & ~blocked).sum()),
                       at_clip=int((v & (ref["err2"] == coef["vf_clip_param"])).sum()),
                       above_clip=int((v & (ref["err2"] > coef["vf_clip_param"])).sum()))
    return ref


def check_exact(ref, coef, stats, gl, gv):
    """grad_logits, grad_value and stats 0, 2, 3, 5, 6 bit for bit; stats 4 and 1 carry the kernel's
    float32 log(2 pi e): within 1e-6 max(1, |ref|), and with entropy_coeff == 0 stats 1 bit for bit."""
    bits32 = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)  # noqa: E731
    bits64 = lambda x: np.ascontiguousarray(x, np.float64).view(np.uint64)  # noqa: E731
    assert np.array_equal(ref["grad_logits"], ref["grad_logits"].astype(np.float32)), "the fixture is not exact"
    assert np.array_equal(ref["grad_value"], ref["grad_value"].astype(np.float32)), "the fixture is not exact"
    bad = bits32(gl) != bits32(ref["grad_logits"])
    assert not bad.any(), f"grad_logits: {bad.sum()} of {bad.size} differ, first row {np.nonzero(bad.any(1))[0][0]}"
    bad = bits32(gv) != bits32(ref["grad_value"])
    assert not bad.any(), f"grad_value: {bad.sum()} of {bad.size} differ, first env-row {np.nonzero(bad)[0][0]}"
    want = ref["stats_vec"]
    same = bits64(stats) == bits64(want)
    exact = [0, 2, 3, 5, 6] + ([1] if coef["entropy_coeff"] == 0 else [])
    assert same[exact].all(), (stats, want)
    err = np.abs(stats - want) / np.maximum(1.0, np.abs(want))
    assert err[[1, 4]].max() <= 1e-6, (stats, want)
