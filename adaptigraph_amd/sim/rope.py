"""The reference's episodes come from a closed CUDA particle solver stepped by src/sim/sim_env/flex_env.py:258-402; that solver does not run
on this hardware, so the model here is the project's own: position-based dynamics of a chain of particles (distance constraints, bending
stiffness by straight-segment shape matching over windows of `w` particles), a cylindrical pusher, a flat table with Coulomb friction.

`rope_push_host` IS the specification: float32 numpy, only + - * / sqrt, every product rounded on its own, every sum in a stated order.
`rope_push(..., device=)` runs the same arithmetic as one HIP launch (csrc/ag_sim.hip: one workgroup per episode, one particle per thread)
and returns the same bits.

One push (xs, zs) -> (xe, ze) of an episode takes n_push = int(|e - s| / speed) + 1 steps of `substeps` substeps each, then `settle`
steps without the pusher.  Substep k (1-based over the n_push * substeps substeps of the push), h = dt / substeps:
  a  predict    v.y -= g h;  p = x + h v
  b  stretch    pairs (i, i + 1), all even i, then all odd i: d = p_j - p_i, len = sqrt((dx dx + dy dy) + dz dz); if len > 0:
                c = (len - l0) / (len 2), p_i += c d, p_j -= c d
  c  stiffness  (skipped when w < 3 or w > n; Jacobi: every cluster reads the p of b)  cluster j = particles j .. j + w - 1, j = 0 .. n - w:
                centroid (cx, cz) = (sum_k p_x / w, sum_k p_z / w), k ascending from the first term; rest coordinate q_k = float(k - (w - 1) / 2) l0;
                a = sum_k q_k (p_kx - cx), b = sum_k q_k (p_kz - cz); nn = sqrt(a a + b b); u = (a / nn, b / nn), or (1, 0) when nn == 0;
                goal of member k: (cx + q_k ux, cz + q_k uz).  A particle sums the goals of the clusters that hold it, ascending in the
                cluster index j from the first term, divides by their count and moves by kappa (mean goal - p) in x and z.
  d  pusher     (push steps) c = s + (e - s) (float(k) inv), inv = float32(1 / (n_push substeps)) computed in float64; a particle with
                0 < d = sqrt(dx dx + dz dz) < R + r, (dx, dz) = p - c, gets (x, z) = c + (dx, dz) ((R + r) / d)
  e  ground     on = p.y <= r;  p.y = max(p.y, r)
  f  velocity   v = (p - x) / h; sp = sqrt(vx vx + vz vz); on: v_x, v_z scaled by 1 - (mu g) h / sp when sp > (mu g) h, by 0 otherwise;  x = p
After push step st (0-based) with st % record_every == 0 frame st / record_every holds x and the pusher point (c.x, r, c.z); after the settle
one more frame holds x and (xe, r + lift, ze).
"""
import dataclasses
import math

import numpy as np

from ._common import DEFAULT, F32, DeviceCall, _as_push, _check_frames, _f_max, _ordered_sum, _xv_ok, push_steps

MAX_PARTICLES = 256      # AG_SIM_ROPE_MAX_PARTICLES

def stiffness_mapping(stiffness):
    """The physics parameter `stiffness` in [0, 1] -> (cluster width w, cluster gain kappa)."""
    s = float(stiffness)
    return 3 + int(s * 13), F32(0.1 + 0.5 * s)


@dataclasses.dataclass
class RopeScene:
    """Per-episode state of E ropes, host arrays: n (E) int32 particles, l0 (E) rest spacing, w (E) int32 cluster width, kappa (E) cluster gain,
    x and v (E, n_max, 3) float32 (rows >= n are zero), stiffness (E) the physics parameter the clusters were mapped from (or None)."""
    n: np.ndarray
    l0: np.ndarray
    w: np.ndarray
    kappa: np.ndarray
    x: np.ndarray
    v: np.ndarray
    stiffness: np.ndarray = None

    @property
    def E(self):
        return len(self.n)

    @classmethod
    def from_ropes(cls, ropes, stiffness=None, w=None, kappa=None, n_max=None):
        """ropes: list of (n_e, 3) positions in rope order; l0 = the mean segment length; clusters from `stiffness` (E) or from w, kappa (E) given."""
        E = len(ropes)
        n = np.array([len(p) for p in ropes], np.int32)
        n_max = int(n.max()) if n_max is None else n_max
        x = np.zeros((E, n_max, 3), F32)
        l0 = np.zeros(E, F32)
        for e, p in enumerate(ropes):
            p = np.asarray(p, F32)
            x[e, :len(p)] = p
            if len(p) > 1:
                l0[e] = F32(np.linalg.norm(np.diff(p.astype(np.float64), axis=0), axis=1).mean())
        if stiffness is not None:
            stiffness = np.asarray(stiffness, np.float64)
            w, kappa = zip(*(stiffness_mapping(s) for s in stiffness))
        return cls(n, l0, np.asarray(w, np.int32), np.asarray(kappa, F32), x, np.zeros_like(x), stiffness)


def _check(scene, push, f_max, params):
    push = _as_push(push)
    if len(push) != scene.E or not _xv_ok(scene):
        raise ValueError("rope_push: one push (xs, zs, xe, ze) per episode and x, v of shape (E, n_max, 3)")
    n_push, inv = push_steps(push, params)
    return push, n_push, inv, _f_max(n_push, f_max, params)


def _validate(scene, n_push, F, params):
    """What rope_push_host and rope_push refuse, alike: a rope of fewer than 2 or more than min(n_max, 256) particles, too few frames."""
    n, n_max = np.asarray(scene.n, np.int64), scene.x.shape[1]
    if n.min() < 2 or n.max() > min(n_max, MAX_PARTICLES):
        raise ValueError(f"rope_push: n outside 2 .. {min(n_max, MAX_PARTICLES)}")
    _check_frames("rope_push", "push", n_push, F, params)


def rope_push_host(scene, push, params=DEFAULT, f_max=None):
    """One push of every episode of `scene` (see the module text).  push (E, 4) float32.  -> obj (E, F, n_max, 3) float32, eef (E, F, 3) float32,
    n_frames (E) int32, x, v (E, n_max, 3) float32 after the settle; F = f_max or the frames of the longest push; frames behind an episode's
    n_frames and rows behind its n are zero.  `scene` is not modified."""
    push, n_push, inv, F = _check(scene, push, f_max, params)
    E, n_max = scene.x.shape[:2]
    _validate(scene, n_push, F, params)
    n = np.asarray(scene.n, np.int64)
    S, rec = int(params.substeps), int(params.record_every)
    h, g, r, mu = params.h, F32(params.g), F32(params.r), F32(params.mu)
    gh, reach, mgh = g * h, F32(params.R) + r, (mu * g) * h
    l0 = np.asarray(scene.l0, F32)[:, None]
    kappa = np.asarray(scene.kappa, F32)[:, None]
    w_all = np.asarray(scene.w, np.int64)
    idx = np.arange(n_max)
    live = idx[None, :] < n[:, None]
    pair = [(idx[par:n_max - 1:2][None, :] + 1 < n[:, None]) for par in (0, 1)]        # pair (i, i + 1) exists
    sx, sz, ex, ez = (push[:, c:c + 1] for c in range(4))
    # clusters: the episodes of one width share the index tables
    groups = []
    for w in np.unique(w_all):
        sel = np.nonzero((w_all == w) & (w >= 3) & (w <= n))[0]
        if len(sel) == 0:
            continue
        w = int(w)
        J = n_max - w + 1
        q = ((2 * np.arange(w) - (w - 1)).astype(F32) * F32(0.5))[None, :] * l0[sel]            # (G, w)
        win = idx[:J, None] + np.arange(w)[None, :]                                            # (J, w): member k of cluster j
        jj = idx[:, None] - (w - 1) + np.arange(w)[None, :]                                    # (n_max, w): slot m -> cluster j, ascending
        kk = (w - 1) - np.arange(w)                                                            # member index of the particle in that cluster
        valid = (jj[None] >= 0) & (jj[None] <= (n[sel] - w)[:, None, None])                    # (G, n_max, w)
        groups.append((sel, w, q, win, np.clip(jj, 0, J - 1), kk, valid, valid.sum(-1).astype(F32), kappa[sel]))

    x = np.array(scene.x, F32)
    v = np.array(scene.v, F32)
    obj = np.zeros((E, F, n_max, 3), F32)
    eef = np.zeros((E, F, 3), F32)
    total = n_push + int(params.settle)
    rows = np.arange(E)
    with np.errstate(all="ignore"):
        for st in range(int(total.max())):
            run = st < total                           # episodes still stepping
            pushing = (st < n_push)[:, None]
            act = live & run[:, None]
            for s in range(S):
                # a. predict
                vy = v[:, :, 1] - gh
                px, py, pz = x[:, :, 0] + h * v[:, :, 0], x[:, :, 1] + h * vy, x[:, :, 2] + h * v[:, :, 2]
                # b. stretch
                for par in (0, 1):
                    a_, b_ = slice(par, n_max - 1, 2), slice(par + 1, n_max, 2)
                    dx, dy, dz = px[:, b_] - px[:, a_], py[:, b_] - py[:, a_], pz[:, b_] - pz[:, a_]
                    ln = np.sqrt((dx * dx + dy * dy) + dz * dz)
                    c = (ln - l0) / (ln * F32(2))
                    m = pair[par] & (ln > 0)
                    for p_, d_ in ((px, dx), (py, dy), (pz, dz)):
                        cd = c * d_
                        p_[:, a_], p_[:, b_] = np.where(m, p_[:, a_] + cd, p_[:, a_]), np.where(m, p_[:, b_] - cd, p_[:, b_])
                # c. straight-segment shape matching
                for sel, w, q, win, jj, kk, valid, cnt, kap in groups:
                    gx_, gz_ = px[sel], pz[sel]
                    wx, wz = gx_[:, win], gz_[:, win]                                          # (G, J, w)
                    cx, cz = _ordered_sum(wx) / F32(w), _ordered_sum(wz) / F32(w)
                    fa = _ordered_sum(q[:, None, :] * (wx - cx[:, :, None]))
                    fb = _ordered_sum(q[:, None, :] * (wz - cz[:, :, None]))
                    nn = np.sqrt(fa * fa + fb * fb)
                    zero = nn == 0
                    ux, uz = np.where(zero, F32(1), fa / nn), np.where(zero, F32(0), fb / nn)
                    qk = q[:, kk][:, None, :]                                                  # (G, 1, w)
                    # slots of clusters that do not exist hold -0.0, the identity of float addition (-0 + t = t, s + -0 = s for every t, s):
                    # the ordered sum over all w slots is the sum over the existing clusters that starts with its first term
                    goal_x = np.where(valid, cx[:, jj] + qk * ux[:, jj], F32(-0.0))
                    goal_z = np.where(valid, cz[:, jj] + qk * uz[:, jj], F32(-0.0))
                    sum_x, sum_z = _ordered_sum(goal_x), _ordered_sum(goal_z)
                    lv = live[sel]
                    px[sel] = np.where(lv, gx_ + kap * (sum_x / cnt - gx_), gx_)
                    pz[sel] = np.where(lv, gz_ + kap * (sum_z / cnt - gz_), gz_)
                # d. pusher
                t = np.full((E, 1), st * S + s + 1, F32) * inv[:, None]
                cpx, cpz = sx + (ex - sx) * t, sz + (ez - sz) * t
                dx, dz = px - cpx, pz - cpz
                d = np.sqrt(dx * dx + dz * dz)
                hit = pushing & (d > 0) & (d < reach)
                k = reach / d
                px, pz = np.where(hit, cpx + dx * k, px), np.where(hit, cpz + dz * k, pz)
                # e. ground
                on = py <= r
                py = np.maximum(py, r)
                # f. velocity and friction
                vx, vy, vz = (px - x[:, :, 0]) / h, (py - x[:, :, 1]) / h, (pz - x[:, :, 2]) / h
                sp = np.sqrt(vx * vx + vz * vz)
                f = np.where(on, np.where(sp > mgh, F32(1) - mgh / sp, F32(0)), F32(1))
                vx, vz = np.where(on, vx * f, vx), np.where(on, vz * f, vz)
                x = np.where(act[:, :, None], np.stack([px, py, pz], 2), x)
                v = np.where(act[:, :, None], np.stack([vx, vy, vz], 2), v)
            if st % rec == 0 and st < int(n_push.max()):
                e_rec = rows[st < n_push]
                obj[e_rec, st // rec] = x[e_rec]
                eef[e_rec, st // rec, 0], eef[e_rec, st // rec, 1], eef[e_rec, st // rec, 2] = cpx[e_rec, 0], r, cpz[e_rec, 0]
    last = (n_push - 1) // rec + 1
    obj[rows, last] = x
    eef[rows, last, 0], eef[rows, last, 1], eef[rows, last, 2] = push[:, 2], r + F32(params.lift), push[:, 3]
    return obj, eef, (last + 1).astype(np.int32), x, v


def rope_push_scalar(x, v, l0, w, kappa, push, params=DEFAULT):
    """The model of the module text for ONE episode, particle by particle in float32 scalars, with no vectorisation: slow, and meant to be read.
    x, v (n, 3); push (xs, zs, xe, ze).  -> obj (F, n, 3), eef (F, 3), x, v as rope_push_host returns them for that episode
    (tests/test_sim_rope_cpu.py holds the vectorised code to it bit for bit)."""
    f = F32
    n = len(x)
    x, v = [[f(c) for c in p] for p in x], [[f(c) for c in p] for p in v]
    l0, kappa = f(l0), f(kappa)
    xs, zs, xe, ze = (f(c) for c in push)
    steps, inv = push_steps(np.array([[xs, zs, xe, ze]], F32), params)
    n_push, inv = int(steps[0]), inv[0]
    S, rec = int(params.substeps), int(params.record_every)
    h, g, r, mu = params.h, f(params.g), f(params.r), f(params.mu)
    gh, reach, mgh = g * h, f(params.R) + r, (mu * g) * h
    q = [(f(2 * k - (w - 1)) * f(0.5)) * l0 for k in range(max(w, 0))]
    obj, eef = [], []
    with np.errstate(all="ignore"):
        for st in range(n_push + int(params.settle)):
            for s in range(S):
                # a. predict
                for i in range(n):
                    v[i][1] = v[i][1] - gh
                p = [[x[i][c] + h * v[i][c] for c in range(3)] for i in range(n)]
                # b. stretch
                for parity in (0, 1):
                    for i in range(parity, n - 1, 2):
                        d = [p[i + 1][c] - p[i][c] for c in range(3)]
                        ln = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                        if ln > 0:
                            c_ = (ln - l0) / (ln * f(2))
                            for c in range(3):
                                p[i][c], p[i + 1][c] = p[i][c] + c_ * d[c], p[i + 1][c] - c_ * d[c]
                # c. straight-segment shape matching
                if 3 <= w <= n:
                    fits = []
                    for j in range(n - w + 1):
                        cx, cz = p[j][0], p[j][2]
                        for k in range(1, w):
                            cx, cz = cx + p[j + k][0], cz + p[j + k][2]
                        cx, cz = cx / f(w), cz / f(w)
                        a, b = q[0] * (p[j][0] - cx), q[0] * (p[j][2] - cz)
                        for k in range(1, w):
                            a, b = a + q[k] * (p[j + k][0] - cx), b + q[k] * (p[j + k][2] - cz)
                        nn = np.sqrt(a * a + b * b)
                        fits.append((cx, cz, f(1), f(0)) if nn == 0 else (cx, cz, a / nn, b / nn))
                    moved = []
                    for i in range(n):
                        mine = range(max(0, i - w + 1), min(i, n - w) + 1)      # the clusters that hold particle i
                        gx = gz = None
                        for j in mine:
                            cx, cz, ux, uz = fits[j]
                            tx, tz = cx + q[i - j] * ux, cz + q[i - j] * uz
                            gx, gz = (tx, tz) if gx is None else (gx + tx, gz + tz)
                        cnt = f(len(mine))
                        moved.append((p[i][0] + kappa * (gx / cnt - p[i][0]), p[i][2] + kappa * (gz / cnt - p[i][2])))
                    for i in range(n):
                        p[i][0], p[i][2] = moved[i]
                # d. pusher
                if st < n_push:
                    t = f(st * S + s + 1) * inv
                    cx, cz = xs + (xe - xs) * t, zs + (ze - zs) * t
                    for i in range(n):
                        dx, dz = p[i][0] - cx, p[i][2] - cz
                        d = np.sqrt(dx * dx + dz * dz)
                        if 0 < d < reach:
                            p[i][0], p[i][2] = cx + dx * (reach / d), cz + dz * (reach / d)
                for i in range(n):
                    # e. ground
                    on = p[i][1] <= r
                    p[i][1] = max(p[i][1], r)
                    # f. velocity and friction
                    v[i] = [(p[i][c] - x[i][c]) / h for c in range(3)]
                    if on:
                        sp = np.sqrt(v[i][0] * v[i][0] + v[i][2] * v[i][2])
                        scale = f(1) - mgh / sp if sp > mgh else f(0)
                        v[i][0], v[i][2] = v[i][0] * scale, v[i][2] * scale
                    x[i] = list(p[i])
            if st < n_push and st % rec == 0:
                obj.append(np.array(x, F32))
                eef.append(np.array([cx, r, cz], F32))
    obj.append(np.array(x, F32))
    eef.append(np.array([xe, r + f(params.lift), ze], F32))
    return np.stack(obj), np.stack(eef), np.array(x, F32), np.array(v, F32)


# ---------------------------------------------------------------------------------------------------------------------
# The device path
# ---------------------------------------------------------------------------------------------------------------------
class DevicePush(DeviceCall):
    """The arguments of one ag_sim_rope_push call (see DeviceCall): x, v in place; an episode whose n lies outside 2 .. n_max gets n_frames = 0."""
    entry = "ag_sim_rope_push"
    pointers = ("n", "l0", "w", "kappa", "inv", "n_push", "push", "x", "v", "obj", "eef", "n_frames")
    results = ("obj", "eef", "n_frames", "x", "v")
    _validate = staticmethod(_validate)

    def __init__(self, scene, push, params=DEFAULT, f_max=None, device="cuda:0"):
        push, n_push, inv, F = _check(scene, push, f_max, params)
        self.steps = n_push      # (host copy)
        super().__init__(scene, params, device, n_push, F, scene.x.shape[1], dict(n=scene.n, w=scene.w, n_push=n_push),
                         dict(l0=scene.l0, kappa=scene.kappa, inv=inv, push=push),
                         (params.h, params.g, params.r, params.R, params.mu, params.lift))


def rope_push(scene, push, params=DEFAULT, f_max=None, device="cuda:0"):
    """rope_push_host on the GPU: the same arguments, the same five results bit for bit, as tensors on `device`.  scene.x and scene.v may be
    host arrays or tensors (copied: `scene` is not modified).  Raises what rope_push_host raises."""
    return DevicePush(scene, push, params, f_max, device).validate().launch()


# ---------------------------------------------------------------------------------------------------------------------
# Scenes and pushes (host, numpy's generator)
# ---------------------------------------------------------------------------------------------------------------------
def initial_rope(rng, n=128, r=DEFAULT.r):
    """A rope of length 2.5 .. 3.0 (src/sim/sim_env/scenes.py:19) lying on the ground along a gently curved line (an arc of up to 0.6 rad),
    rotated about the vertical by a random angle, centred at the origin.  -> (n, 3) float32 in rope order."""
    length = rng.uniform(2.5, 3.0)
    bend = rng.uniform(-0.6, 0.6)
    angle = rng.uniform(0.0, 2.0 * math.pi)
    s = (np.arange(n) / (n - 1) - 0.5) * length
    if abs(bend) < 1e-6:
        px, pz = s, np.zeros(n)
    else:
        rad = length / bend
        px, pz = rad * np.sin(s / rad), rad * (1.0 - np.cos(s / rad))
    pz = pz - pz.mean()
    c, sn = math.cos(angle), math.sin(angle)
    return np.stack([c * px - sn * pz, np.full(n, float(r)), sn * px + c * pz], 1).astype(F32)


def sample_push(x, rng, params=DEFAULT, tries=100):
    """A push for the rope x (n, 3): a straight segment 0.8 .. 1.6 long through the neighbourhood (within 0.1) of a random particle, in a random
    direction, whose start is clear of every particle by more than R + r (with a margin of r).  -> (4,) float32 xs, zs, xe, ze."""
    x = np.asarray(x, np.float64)
    clear = float(params.R) + 2.0 * float(params.r)
    for _ in range(tries):
        i = int(rng.integers(len(x)))
        through = x[i, [0, 2]] + rng.uniform(-0.1, 0.1, 2)
        a = rng.uniform(0.0, 2.0 * math.pi)
        length = rng.uniform(0.8, 1.6)
        frac = rng.uniform(0.3, 0.7)
        u = np.array([math.cos(a), math.sin(a)])
        s, e = through - frac * length * u, through + (1.0 - frac) * length * u
        if np.sqrt(((x[:, [0, 2]] - s) ** 2).sum(1)).min() > clear:
            return np.array([s[0], s[1], e[0], e[1]], F32)
    raise RuntimeError("sample_push: no push starts clear of the rope")
