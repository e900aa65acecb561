"""Batched particle simulators, a rope on a table, a pile of discs pushed by a board, a cloth dragged by a gripper and a rigid box with a hidden centre
of mass: the data side of the workflow.

The reference's episodes come from a closed CUDA particle solver stepped by src/sim/sim_env/flex_env.py:258-402; that solver does not run
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

The granular model (`pile_push_host` IS its specification, `pile_push(..., device=)` is csrc/ag_sim_pile.hip: one workgroup per
episode, four grains per thread, a neighbour grid in LDS): one layer of n <= 1024 discs of radius rho in the x-z plane on the table, pushed by a flat
board of half width W and half thickness T.  float32, only + - * / sqrt, rint, min and max, every product rounded on its own; y is carried and
never read.  Steps, settle and recording as above.  Substep k (1-based over the push), h = dt / substeps:
  a  predict    p = x + h v                                                      (x and z)
  b  contacts   `iters` Jacobi iterations, every grain reading the p of the iteration before: over every j != i with 0 < d < 2 rho,
                (dx, dz) = p_i - p_j, d = sqrt(dx dx + dz dz):  c = (2 rho - d) / (d 2);  sx += int32(rint((c dx) 2^22)), sz += int32(rint((c dz) 2^22)),
                cnt += 1 -- integer sums, exact in any order: the set "all j within 2 rho" is the whole statement, with no grid and no order in it.
                Where cnt > 0:  p_i += (float(sx) 2^-22) / float(cnt), likewise z.  (|c dx| <= rho <= 0.25, so 1023 terms stay inside int32.)
  c  board      (push steps) centre c = s + (e - s) (float(k) inv); lateral unit vector u = (ux, uz), the push direction turned by a quarter turn
                ((-dz, dx) / |e - s|, float64 on the host, rounded to float32; (0, 1) for a push of no length); r = p - c;
                a = min(max(rx ux + rz uz, -W), W); foot q = c + a u; (fx, fz) = p - q, d = sqrt(fx fx + fz fz); a grain with 0 < d < rho + T
                gets p = q + (fx, fz) (((rho + T) + slack) / d): slack (2^-19) is a few roundings of a coordinate of size 2, so that the grain
                lands outside rho + T in exact arithmetic too, not merely up to the rounding of q and of p
  d  velocity   v = (p - x) / h; sp = sqrt(vx vx + vz vz); v scaled by 1 - (mu g) h / sp when sp > (mu g) h, by 0 otherwise (every grain lies
                on the table);  x = p
A frame holds x and the board's five key points c + (W o_k) u, o = (1, -1, 0, 1/2, -1/2), at height tool_y; the frame after the settle has them at
the push end e, raised by lift.

The cloth model (`cloth_push_host` IS its specification, `cloth_push(..., device=)` is csrc/ag_sim_cloth.hip: one workgroup of
1 024 threads per episode, four particles per thread, the predicted positions in LDS).  It is the project's own: NOT FleX and not fitted to it,
with NO self-collision (the sampled drags pull an edge outward, away from the cloth); it follows the reference only in the shape of the
stiffness mapping (scenes.py:139-175), of the gripper's way points and pick (flex_env.py:258-402) and of the sampled grasps (flex_env.py:472-525).
A cloth is a grid of nx x nz particles, i = iz nx + ix, 2 <= nx, nz <= 64, at rest spacing l0, lying on the table at height r, held together by
distance constraints: stretch (ix, ix + 1), (iz, iz + 1) at l0 with gain ks; shear, both diagonals of every cell, at float32(l0 sqrt 2) (the product
in float64 on the host) with gain kh; bend (ix, ix + 2), (iz, iz + 2) at l0 2 with gain kb.  float32, only + - * / sqrt, min and max, every product
rounded on its own.  One SWEEP is twelve phases in this order, a coloured Gauss-Seidel pass in place; within a phase no particle is in two pairs,
so the order of the pairs of a phase does not matter:
   0, 1   stretch x   (ix, iz)-(ix + 1, iz)          ix even, then ix odd
   2, 3   stretch z   (ix, iz)-(ix, iz + 1)          iz even, then iz odd
   4, 5   diagonal    (ix, iz)-(ix + 1, iz + 1)      the cell's ix even, then odd
   6, 7   diagonal    (ix + 1, iz)-(ix, iz + 1)      the cell's ix even, then odd
   8, 9   bend x      (ix, iz)-(ix + 2, iz)          ix >> 1 even, then odd
  10, 11  bend z      (ix, iz)-(ix, iz + 2)          iz >> 1 even, then odd
A pair (i, j) of rest length L and gain k, with inverse masses w in {0, 1} (0: pinned): d = p_j - p_i, len = sqrt((dx dx + dy dy) + dz dz); skipped
when len == 0 or w_i + w_j == 0; c = (k (len - L)) / (len (w_i + w_j)); p_i = p_i + w_i (c d), p_j = p_j - w_j (c d).
The action (xs, zs, xe, ze) moves a gripper along two segments, heights being offsets above the grasp height: from (xs, 0, zs) to (xe, lift, ze) in
n1 = int(len3 / speed) + 1 steps (len3 the 3-D length), then down to (xe, 0, ze) in n2 = int(lift / speed) + 1 steps; then it lets go and `settle`
steps follow.  inv1 = float32(1 / (n1 substeps)), inv2 likewise, computed in float64.  At substep k (1-based within its segment), t = float(k) inv:
segment 1: c = (xs + (xe - xs) t, lift t, zs + (ze - zs) t); segment 2: c = (xe, max(lift - lift t, 0), ze).
The pick, on the state x the call starts from: d2_i = dx dx + dz dz with (dx, dz) = (x_i.x - xs, x_i.z - zs); the up to 5 particles of smallest
(d2, i) -- the 64-bit key (bits of d2) << 32 | i, so equal d2 is decided by the lower index -- are grasped if the smallest d2 <= grasp grasp, and
nothing is otherwise (the cloth is then simulated free).  A grasped particle keeps off = (x.x - xs, x.y, x.z - zs).
Substep, h = dt / substeps:
  a  predict    v.y = v.y - g h;  v = v damp (damp = float32(1 - drag h), float64 on the host);  p = x + h v
  b  pins       (both segments) a grasped particle: p = c + off, w = 0;  every other particle, and every particle after the release: w = 1
  c  sweeps     `iters` of them
  d  ground     on = p.y <= r;  p.y = max(p.y, r)
  e  velocity   v = (p - x) / h; sp = sqrt(vx vx + vz vz); on and w == 1: v_x, v_z scaled by 1 - (mu g) h / sp when sp > (mu g) h, by 0 otherwise;  x = p
After step st (0-based over the n1 + n2 steps of both segments) with st % record_every == 0 frame st / record_every holds x and the two finger
points (c.x +- finger u.x, tool_y + c.y, c.z +- finger u.z), u the lateral unit vector of `board_lateral`; after the settle one more frame holds x
and the finger points at (xe, lift, ze).

The box model (`box_push_host` IS its specification, `box_push(..., device=)` is csrc/ag_sim_box.hip: one workgroup of 256 threads
per episode, up to four particles per thread).  It is the project's own: NOT pymunk and not fitted to it, one box, no walls, a FRICTIONLESS pusher;
it follows the reference (src/sim/data_gen/data_gen_box.py, config/data_gen/box.yaml) in the ranges of the sides, the friction 0.5, the hidden
centre of mass and the shape of the sampled pushes.  One unit is 100 px of box.yaml.  A box is a rigid rectangle a x b; its centre of mass lies at
the fractions (fx, fz) of the sides from the geometric centre.  It is sampled by nx x nz particles, i = iz nx + ix, at the centres of the nx x nz
cells of the rectangle (nx = int(a / (2 r)), so the spacing a / nx is 2 r or a little more), lying at height r, with masses m_i = wx[ix] wz[iz],
w ~ exp(lam c): a density tilted exponentially along each axis, the tilt found by bisection so that the discrete centre of mass IS the requested
one (`box_masses`, float64, outside the bit-exact path).  The simulation reads: q_i the rest coordinates relative to the centre of mass, m_i
(sum 1), the footprint x_lo, x_hi, z_lo, z_hi relative to the centre of mass, I = sum m |q|^2 and rho_max >= max |q|; it computes none of these.
State: the pose (X, Z, co, si) of the centre of mass, (co, si) a unit vector (a body vector (x, z) lies at (co x - si z, si x + co z)), and the
velocity (VX, VZ, Omega).  float32, only + - * / sqrt, rint, min and max, every product rounded on its own.  Steps, settle, recording and the
pusher's centre c of substep k are the rope's; the pusher is a cylinder of radius R.  TURN(co, si, t), the rotation of Cayley parameter t:
unchanged when t == 0 (so a box at rest is a fixed point), otherwise (cr, sr) = ((1 - t t) / (1 + t t), (t + t) / (1 + t t)),
(c2, s2) = (co cr - si sr, si cr + co sr), nn = sqrt(c2 c2 + s2 s2), (co, si) = (c2 / nn, s2 / nn).  Substep, h = dt / substeps:
  a  predict    X = X + h VX, Z likewise;  TURN by (Omega h) / 2
  b  pusher     (push steps, `iters` times) d = c - (X, Z); in the body frame l = (co dx + si dz, co dz - si dx); the closest point of the footprint
                kp = (min(max(lx, x_lo), x_hi), likewise z); g = l - kp, dist = sqrt(gx gx + gz gz).
                dist == 0 (the centre is inside): the distances to the faces d0 = lx - x_lo, d1 = x_hi - lx, d2 = lz - z_lo, d3 = z_hi - lz, dmin their
                minimum; the FIRST face with d == dmin decides: normal nb = (1, 0), (-1, 0), (0, 1), (0, -1), contact pc = (x_lo, lz), (x_hi, lz),
                (lx, z_lo), (lx, z_hi); pen = dmin + R.   0 < dist < R: nb = -(g / dist), pc = kp, pen = R - dist.   Otherwise nothing.
                cr = pc.x nb.z - pc.z nb.x; w = 1 + (cr cr) / I  (the generalised inverse mass of a unit mass and inertia I);
                nw = (co nb.x - si nb.z, si nb.x + co nb.z).  A correction by lam: (X, Z) += lam nw; TURN by ((cr lam) / I) / 2 -- the contact point
                moves by lam w along the normal.  If pen > cap, cap = float32(depen speed / substeps): first a correction by lam = (pen - cap) / w
                applied to the pose AND to the pose the substep started from (so step c sees no velocity in it: a pusher that starts in or
                against the box moves it out of the way without throwing it; a push in progress never gets there, its pen is about one
                advance of the pusher).  Then, always, a correction by lam = min(pen, cap) / w with the nw computed above.
  c  velocity   V = ((X, Z) - (X, Z)_start) / h;  crel = co co_start + si si_start, srel = si co_start - co si_start, trel = srel / (1 + crel),
                Omega = (trel + trel) / h  (the inverse of a)
  d  friction   every particle on the table, implicitly: rho_i = (co qx - si qz, si qx + co qz), u_i = (VX - Omega rho_z, VZ + Omega rho_x),
                k_i = (m_i (mu g)) / max(sqrt(ux ux + uz uz), eps): Coulomb's m mu g against the motion, viscous below the speed eps.
                Four sums over the particles, S0 of k, Sx of k rho_x, Sz of k rho_z, S2 of k (rho_x rho_x + rho_z rho_z), each the INTEGER sum of
                int64(rint(term 2^22)), exact in any order, brought back as float32(float64(sum)) 2^-22.  (k <= (mu g) / eps <= 8192 = 2^13 as m <= 1,
                |rho| <= rho_max <= 8: a scaled term stays under 2^13 2^6 2^22 = 2^41 and 1024 of them under 2^51, inside int64 and inside the
                53 bits of float64; _box_validate and the kernel refuse anything beyond these bounds.)
                (M + h A) v' = M v with M = diag(1, 1, I), A = [[S0, 0, -Sz], [0, S0, Sx], [-Sz, Sx, S2]], in closed form: a = 1 + h S0,
                b = -(h Sz), c = h Sx, d = I + h S2;  Omega' = (I Omega - (b VX + c VZ) / a) / (d - (b b + c c) / a);  VX' = (VX - b Omega') / a,
                VZ' = (VZ - c Omega') / a.  A is positive semi-definite: friction brakes and never reverses.
                If sqrt(VX' VX' + VZ' VZ') + max(Omega', -Omega') rho_max < v_rest the velocity becomes exactly zero.
A frame holds the particles (X + ((co qx) - (si qz)), r, Z + ((si qx) + (co qz))), the pusher point (c.x, r, c.z) and the pose; the frame after the
settle has the pusher point (xe, r + lift, ze).  theta = atan2(si, co) is taken on the host afterwards, for the records only.
"""
import dataclasses
import math

import numpy as np

MAX_PARTICLES = 256      # AG_SIM_ROPE_MAX_PARTICLES
F32 = np.float32


@dataclasses.dataclass(frozen=True)
class SimParams:
    dt: float = 1.0 / 60.0
    substeps: int = 8
    g: float = 9.8
    r: float = 0.03            # particle radius
    R: float = 0.05            # pusher radius
    mu: float = 0.1            # the reference scene's dynamicFriction (scenes.py:33)
    speed: float = 0.01        # pusher advance per step
    record_every: int = 10
    settle: int = 120
    lift: float = 0.2

    @property
    def h(self):
        return F32(self.dt / self.substeps)


DEFAULT = SimParams()


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


def push_steps(push, params=DEFAULT):
    """push (E, 4) float32 xs, zs, xe, ze -> (n_push (E) int32, inv (E) float32): the steps of every push and 1 / its substeps."""
    p = np.asarray(push, F32).astype(np.float64).reshape(-1, 4)
    length = np.sqrt((p[:, 2] - p[:, 0]) ** 2 + (p[:, 3] - p[:, 1]) ** 2)
    n_push = (length / float(params.speed)).astype(np.int64) + 1
    return n_push.astype(np.int32), (1.0 / (n_push * params.substeps)).astype(F32)


def frames_of(n_push, params=DEFAULT):
    """Frames a push of n_push steps records: steps 0, record_every, ... < n_push and the frame after the settle."""
    return (np.asarray(n_push) - 1) // params.record_every + 2


def _check(scene, push, f_max, params):
    push = np.ascontiguousarray(push, F32).reshape(-1, 4)
    if len(push) != scene.E or scene.x.shape != scene.v.shape or scene.x.shape[0] != scene.E or scene.x.shape[2] != 3:
        raise ValueError("rope_push: one push (xs, zs, xe, ze) per episode and x, v of shape (E, n_max, 3)")
    n_push, inv = push_steps(push, params)
    need = int(frames_of(n_push, params).max())
    return push, n_push, inv, need if f_max is None else int(f_max)


def _validate(scene, n_push, F, params):
    """What rope_push_host and rope_push refuse, alike: a rope of fewer than 2 or more than min(n_max, 256) particles, too few frames."""
    n, n_max = np.asarray(scene.n, np.int64), scene.x.shape[1]
    if n.min() < 2 or n.max() > min(n_max, MAX_PARTICLES):
        raise ValueError(f"rope_push: n outside 2 .. {min(n_max, MAX_PARTICLES)}")
    if F < int(frames_of(n_push, params).max()):
        raise ValueError(f"rope_push: f_max = {F} frames, the longest push writes {int(frames_of(n_push, params).max())}")


def _ordered_sum(a):
    """Sum over the last axis in index order, starting with the first term (np.sum adds pairwise; a running sum does not)."""
    return np.cumsum(a, axis=-1)[..., -1]


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
class DevicePush:
    """The arguments of one ag_sim_rope_push call as device tensors: `launch()` enqueues the kernel on the current stream (no synchronisation,
    no allocation: it captures into a HIP graph), reading and writing x, v in place and writing obj, eef, n_frames.  The arguments go to the
    library as given: what it refuses comes back as its argument error (RuntimeError), and an episode whose n lies outside 2 .. n_max gets
    n_frames = 0 with nothing else written.  `rope_push` checks the scene first, as the host path does."""

    def __init__(self, scene, push, params=DEFAULT, f_max=None, device="cuda:0"):
        import torch
        self.device = torch.device(device)
        push, n_push, inv, F = _check(scene, push, f_max, params)
        E, n_max = scene.x.shape[:2]
        self.steps = n_push      # (host copy)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.device)
        self.n, self.w, self.n_push = up(scene.n, np.int32), up(scene.w, np.int32), up(n_push, np.int32)
        self.l0, self.kappa, self.inv, self.push = up(scene.l0, F32), up(scene.kappa, F32), up(inv, F32), up(push, F32)
        self.x, self.v = (t.to(self.device).contiguous().clone() if isinstance(t, torch.Tensor) else up(t, F32) for t in (scene.x, scene.v))
        self.obj = torch.zeros((E, F, n_max, 3), dtype=torch.float32, device=self.device)
        self.eef = torch.zeros((E, F, 3), dtype=torch.float32, device=self.device)
        self.n_frames = torch.zeros(E, dtype=torch.int32, device=self.device)
        self.dims = (E, n_max, F, int(n_push.max()), int(params.substeps), int(params.record_every), int(params.settle))
        self.floats = tuple(float(F32(c)) for c in (params.h, params.g, params.r, params.R, params.mu, params.lift))

    def launch(self):
        from . import _lib
        _lib.call("ag_sim_rope_push", self.device, self.n, self.l0, self.w, self.kappa, self.inv, self.n_push, self.push, self.x, self.v, self.obj,
                  self.eef, self.n_frames, *self.dims, *self.floats)
        return self.obj, self.eef, self.n_frames, self.x, self.v


def rope_push(scene, push, params=DEFAULT, f_max=None, device="cuda:0"):
    """rope_push_host on the GPU: the same arguments, the same five results bit for bit, as tensors on `device`.  scene.x and scene.v may be
    host arrays or tensors (copied: `scene` is not modified).  Raises what rope_push_host raises."""
    call = DevicePush(scene, push, params, f_max, device)
    _validate(scene, call.steps, call.dims[2], params)
    return call.launch()


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


# ---------------------------------------------------------------------------------------------------------------------
# The granular model: a pile of discs pushed by a board (the module text)
# ---------------------------------------------------------------------------------------------------------------------
PILE_MAX_PARTICLES = 1024      # AG_SIM_PILE_MAX_PARTICLES
PILE_RHO_MAX = 0.25            # the bound that keeps 1023 contact terms of at most rho 2^22 inside int32
PILE_KEY_OFFSETS = (1.0, -1.0, 0.0, 0.5, -0.5)      # times W: lateral offsets 0.5, -0.5, 0, 0.25, -0.25 (config/dynamics/granular.yaml:18-25)
_Q22, _IQ22 = F32(4194304.0), F32(1.0 / 4194304.0)


@dataclasses.dataclass(frozen=True)
class PileParams:
    dt: float = 1.0 / 60.0
    substeps: int = 8
    iters: int = 4             # Jacobi contact iterations per substep
    g: float = 9.8
    mu: float = 1.0            # the reference scene's dynamic_friction (scenes.py:118)
    W: float = 0.5             # board half width
    T: float = 0.02            # board half thickness
    slack: float = 2.0 ** -19  # how far beyond rho + T the board puts a grain (the module text)
    tool_y: float = 0.1        # height of the board's key points
    speed: float = 0.01
    record_every: int = 10
    settle: int = 120
    lift: float = 0.2

    @property
    def h(self):
        return F32(self.dt / self.substeps)


PILE_DEFAULT = PileParams()


@dataclasses.dataclass
class PileScene:
    """Per-episode state of E piles, host arrays: n (E) int32 grains, rho (E) float32 disc radius, x and v (E, n_max, 3) float32 (rows >= n zero)."""
    n: np.ndarray
    rho: np.ndarray
    x: np.ndarray
    v: np.ndarray

    @property
    def E(self):
        return len(self.n)

    @classmethod
    def from_piles(cls, piles, rho, n_max=None):
        """piles: list of (n_e, 3) grain positions; rho (E) their radii."""
        n = np.array([len(p) for p in piles], np.int32)
        n_max = int(n.max()) if n_max is None else n_max
        x = np.zeros((len(piles), n_max, 3), F32)
        for e, p in enumerate(piles):
            x[e, :len(p)] = np.asarray(p, F32)
        return cls(n, np.asarray(rho, F32).reshape(-1), x, np.zeros_like(x))


def board_lateral(push):
    """push (E, 4) float32 -> (E, 2) float32: the unit vector along the board, the push direction turned by a quarter turn (float64, rounded once)."""
    p = np.asarray(push, F32).astype(np.float64).reshape(-1, 4)
    dx, dz = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    length = np.sqrt(dx * dx + dz * dz)
    ok = length > 0
    safe = np.where(ok, length, 1.0)
    return np.stack([np.where(ok, -dz / safe, 0.0), np.where(ok, dx / safe, 1.0)], 1).astype(F32)


def _pile_check(scene, push, f_max, params):
    push = np.ascontiguousarray(push, F32).reshape(-1, 4)
    if len(push) != scene.E or scene.x.shape != scene.v.shape or scene.x.shape[0] != scene.E or scene.x.shape[2] != 3 or len(scene.rho) != scene.E:
        raise ValueError("pile_push: one push (xs, zs, xe, ze) and one rho per episode and x, v of shape (E, n_max, 3)")
    n_push, inv = push_steps(push, params)
    need = int(frames_of(n_push, params).max())
    return push, n_push, inv, board_lateral(push), need if f_max is None else int(f_max)


def _pile_validate(scene, n_push, F, params):
    """What pile_push_host and pile_push refuse, alike."""
    n, n_max = np.asarray(scene.n, np.int64), scene.x.shape[1]
    if n.min() < 1 or n.max() > min(n_max, PILE_MAX_PARTICLES):
        raise ValueError(f"pile_push: n outside 1 .. {min(n_max, PILE_MAX_PARTICLES)}")
    rho = np.asarray(scene.rho, F32)
    if not (rho > 0).all() or rho.max() > F32(PILE_RHO_MAX):
        raise ValueError(f"pile_push: rho outside (0, {PILE_RHO_MAX}]")
    if int(params.iters) < 1:
        raise ValueError("pile_push: iters < 1")
    if F < int(frames_of(n_push, params).max()):
        raise ValueError(f"pile_push: f_max = {F} frames, the longest push writes {int(frames_of(n_push, params).max())}")


class _PairList:
    """Candidate contact pairs of a batch of piles, complete by construction: every ordered pair (i, j), i != j, of one episode whose centres
    were nearer than 2 rho + skin (skin = rho) when the list was made, rebuilt (brute force, float64) as soon as any grain has moved more than
    0.45 skin since.  Two grains nearer than 2 rho in float32 (a relative error of a few 2^-24) are then at most 2 rho (1 + 1e-6) + 0.9 skin
    apart at the time of the build: in the list.  Which pairs the list holds beyond those never matters: the d < 2 rho test decides."""

    def __init__(self, n, rho):
        self.n, self.rho = n, np.asarray(rho, np.float64)
        self.ref = None

    def pairs(self, px, pz):
        """-> (I, J) flat indices e n_max + i of the candidate pairs for the positions px, pz (E, n_max)."""
        qx, qz = px.astype(np.float64), pz.astype(np.float64)
        if self.ref is not None:
            moved = (qx - self.ref[0]) ** 2 + (qz - self.ref[1]) ** 2
            if all((moved[e, :k] <= (0.45 * self.rho[e]) ** 2).all() for e, k in enumerate(self.n)):
                return self.I, self.J
        n_max = px.shape[1]
        I, J = [], []
        for e, k in enumerate(self.n):
            ax, az = qx[e, :k], qz[e, :k]
            near = (ax[:, None] - ax[None, :]) ** 2 + (az[:, None] - az[None, :]) ** 2 < (3.0 * self.rho[e]) ** 2
            np.fill_diagonal(near, False)
            i, j = np.nonzero(near)
            I.append(i + e * n_max)
            J.append(j + e * n_max)
        self.I, self.J, self.ref = np.concatenate(I), np.concatenate(J), (qx, qz)
        return self.I, self.J


def pile_push_host(scene, push, params=PILE_DEFAULT, f_max=None, trace=None):
    """One board push of every episode of `scene` (the granular model of the module text).  push (E, 4) float32.  -> obj (E, F, n_max, 3) float32,
    eef (E, F, 5, 3) float32, n_frames (E) int32, x, v (E, n_max, 3) float32 after the settle; frames behind an episode's n_frames and rows
    behind its n are zero.  `scene` is not modified.  trace, if given, is called as trace(st, s, px, pz, cx, cz) at the end of every substep
    (px, pz (E, n_max) the positions, cx, cz (E, 1) the board's centre)."""
    push, n_push, inv, lat, F = _pile_check(scene, push, f_max, params)
    E, n_max = scene.x.shape[:2]
    _pile_validate(scene, n_push, F, params)
    n = np.asarray(scene.n, np.int64)
    S, rec, iters = int(params.substeps), int(params.record_every), int(params.iters)
    h, W = params.h, F32(params.W)
    mgh = (F32(params.mu) * F32(params.g)) * h
    rho = np.asarray(scene.rho, F32)[:, None]
    two_rho, reach = rho * F32(2), rho + F32(params.T)
    out = reach + F32(params.slack)
    live = np.arange(n_max)[None, :] < n[:, None]
    sx, sz, ex, ez = (push[:, c:c + 1] for c in range(4))
    ux, uz = lat[:, 0:1], lat[:, 1:2]
    x = np.array(scene.x, F32)
    v = np.array(scene.v, F32)
    obj = np.zeros((E, F, n_max, 3), F32)
    eef = np.zeros((E, F, 5, 3), F32)
    off = np.array(PILE_KEY_OFFSETS, F32)[None, :] * W                      # (1, 5)
    total = n_push + int(params.settle)
    rows = np.arange(E)
    near = _PairList(n, rho[:, 0])
    flat_two_rho = np.broadcast_to(two_rho, (E, n_max)).reshape(-1)
    with np.errstate(all="ignore"):
        for st in range(int(total.max())):
            run = st < total
            pushing = (st < n_push)[:, None]
            act = live & run[:, None]
            for s in range(S):
                # a. predict
                px, pz = x[:, :, 0] + h * v[:, :, 0], x[:, :, 2] + h * v[:, :, 2]
                # b. contacts
                for _ in range(iters):
                    I, J = near.pairs(px, pz)
                    fx, fz = px.reshape(-1), pz.reshape(-1)
                    dx, dz = fx[I] - fx[J], fz[I] - fz[J]
                    d = np.sqrt(dx * dx + dz * dz)
                    tr = flat_two_rho[I]
                    hit = (d > 0) & (d < tr)
                    c = (tr - d) / (d * F32(2))
                    tx = np.where(hit, np.rint((c * dx) * _Q22), F32(0)).astype(np.float64)      # integers: float64 sums of them are exact
                    tz = np.where(hit, np.rint((c * dz) * _Q22), F32(0)).astype(np.float64)
                    cnt = np.bincount(I, hit, E * n_max).reshape(E, n_max)
                    sum_x = np.bincount(I, tx, E * n_max).reshape(E, n_max).astype(np.int32)
                    sum_z = np.bincount(I, tz, E * n_max).reshape(E, n_max).astype(np.int32)
                    fc = cnt.astype(F32)
                    px = np.where(cnt > 0, px + (sum_x.astype(F32) * _IQ22) / fc, px)
                    pz = np.where(cnt > 0, pz + (sum_z.astype(F32) * _IQ22) / fc, pz)
                # c. board
                t = np.full((E, 1), st * S + s + 1, F32) * inv[:, None]
                cpx, cpz = sx + (ex - sx) * t, sz + (ez - sz) * t
                rx, rz = px - cpx, pz - cpz
                a = np.minimum(np.maximum(rx * ux + rz * uz, -W), W)
                qx, qz = cpx + a * ux, cpz + a * uz
                gx, gz = px - qx, pz - qz
                d = np.sqrt(gx * gx + gz * gz)
                hit = pushing & (d > 0) & (d < reach)
                k = out / d
                px, pz = np.where(hit, qx + gx * k, px), np.where(hit, qz + gz * k, pz)
                # d. velocity and friction
                vx, vz = (px - x[:, :, 0]) / h, (pz - x[:, :, 2]) / h
                sp = np.sqrt(vx * vx + vz * vz)
                f = np.where(sp > mgh, F32(1) - mgh / sp, F32(0))
                vx, vz = vx * f, vz * f
                x = np.where(act[:, :, None], np.stack([px, x[:, :, 1], pz], 2), x)
                v = np.where(act[:, :, None], np.stack([vx, v[:, :, 1], vz], 2), v)
                if trace is not None:
                    trace(st, s, x[:, :, 0], x[:, :, 2], cpx, cpz)
            if st % rec == 0 and st < int(n_push.max()):
                e_rec = rows[st < n_push]
                obj[e_rec, st // rec] = x[e_rec]
                eef[e_rec, st // rec, :, 0] = (cpx + off * ux)[e_rec]
                eef[e_rec, st // rec, :, 1] = F32(params.tool_y)
                eef[e_rec, st // rec, :, 2] = (cpz + off * uz)[e_rec]
    last = (n_push - 1) // rec + 1
    obj[rows, last] = x
    eef[rows, last, :, 0] = ex + off * ux
    eef[rows, last, :, 1] = F32(params.tool_y) + F32(params.lift)
    eef[rows, last, :, 2] = ez + off * uz
    return obj, eef, (last + 1).astype(np.int32), x, v


def pile_push_scalar(x, v, rho, push, params=PILE_DEFAULT):
    """The granular model for ONE episode, grain by grain in float32 scalars, with brute-force neighbours: slow, and meant to be read.
    x, v (n, 3); push (xs, zs, xe, ze).  -> obj (F, n, 3), eef (F, 5, 3), x, v as pile_push_host returns them for that episode
    (tests/test_sim_pile_cpu.py holds the vectorised code to it bit for bit)."""
    f = F32
    n = len(x)
    x, v = [[f(c) for c in p] for p in x], [[f(c) for c in p] for p in v]
    rho = f(rho)
    xs, zs, xe, ze = (f(c) for c in push)
    steps, inv = push_steps(np.array([[xs, zs, xe, ze]], F32), params)
    n_push, inv = int(steps[0]), inv[0]
    ux, uz = board_lateral(np.array([[xs, zs, xe, ze]], F32))[0]
    S, rec = int(params.substeps), int(params.record_every)
    h, W = params.h, f(params.W)
    mgh, two_rho, reach = (f(params.mu) * f(params.g)) * h, rho * f(2), rho + f(params.T)
    out = reach + f(params.slack)
    off = [f(o) * W for o in PILE_KEY_OFFSETS]
    obj, eef = [], []
    with np.errstate(all="ignore"):
        for st in range(n_push + int(params.settle)):
            for s in range(S):
                # a. predict
                p = [[x[i][0] + h * v[i][0], x[i][2] + h * v[i][2]] for i in range(n)]
                # b. contacts
                for _ in range(int(params.iters)):
                    nxt = []
                    for i in range(n):
                        sum_x = sum_z = cnt = 0
                        for j in range(n):
                            dx, dz = p[i][0] - p[j][0], p[i][1] - p[j][1]
                            d = np.sqrt(dx * dx + dz * dz)
                            if j != i and 0 < d < two_rho:
                                c = (two_rho - d) / (d * f(2))
                                sum_x, sum_z, cnt = sum_x + int(np.rint((c * dx) * _Q22)), sum_z + int(np.rint((c * dz) * _Q22)), cnt + 1
                        nxt.append([p[i][0] + (f(sum_x) * _IQ22) / f(cnt), p[i][1] + (f(sum_z) * _IQ22) / f(cnt)] if cnt else list(p[i]))
                    p = nxt
                # c. board
                if st < n_push:
                    t = f(st * S + s + 1) * inv
                    cx, cz = xs + (xe - xs) * t, zs + (ze - zs) * t
                    for i in range(n):
                        rx, rz = p[i][0] - cx, p[i][1] - cz
                        a = min(max(rx * ux + rz * uz, -W), W)
                        qx, qz = cx + a * ux, cz + a * uz
                        gx, gz = p[i][0] - qx, p[i][1] - qz
                        d = np.sqrt(gx * gx + gz * gz)
                        if 0 < d < reach:
                            p[i] = [qx + gx * (out / d), qz + gz * (out / d)]
                # d. velocity and friction
                for i in range(n):
                    vx, vz = (p[i][0] - x[i][0]) / h, (p[i][1] - x[i][2]) / h
                    sp = np.sqrt(vx * vx + vz * vz)
                    scale = f(1) - mgh / sp if sp > mgh else f(0)
                    v[i][0], v[i][2] = vx * scale, vz * scale
                    x[i][0], x[i][2] = p[i][0], p[i][1]
            if st < n_push and st % rec == 0:
                obj.append(np.array(x, F32))
                eef.append(np.array([[cx + o * ux, f(params.tool_y), cz + o * uz] for o in off], F32))
    obj.append(np.array(x, F32))
    eef.append(np.array([[xe + o * ux, f(params.tool_y) + f(params.lift), ze + o * uz] for o in off], F32))
    return np.stack(obj), np.stack(eef), np.array(x, F32), np.array(v, F32)


class DevicePilePush:
    """The arguments of one ag_sim_pile_push call as device tensors, as DevicePush holds those of the rope: `launch()` enqueues the kernel on the
    current stream (no synchronisation, no allocation: it captures into a HIP graph), reading and writing x, v in place and writing obj, eef,
    n_frames.  The arguments go to the library as given; `rho_max`, the host's bound on the device-side radii, defaults to the largest of the
    scene.  An episode whose n, n_push or rho lies outside the bounds gets n_frames = 0 with nothing else written."""

    def __init__(self, scene, push, params=PILE_DEFAULT, f_max=None, device="cuda:0", rho_max=None):
        import torch
        self.device = torch.device(device)
        push, n_push, inv, lat, F = _pile_check(scene, push, f_max, params)
        E, n_max = scene.x.shape[:2]
        self.steps = n_push      # (host copy)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.device)
        self.n, self.n_push = up(scene.n, np.int32), up(n_push, np.int32)
        self.rho, self.inv, self.push, self.lat = up(scene.rho, F32), up(inv, F32), up(push, F32), up(lat, F32)
        self.x, self.v = (t.to(self.device).contiguous().clone() if isinstance(t, torch.Tensor) else up(t, F32) for t in (scene.x, scene.v))
        self.obj = torch.zeros((E, F, n_max, 3), dtype=torch.float32, device=self.device)
        self.eef = torch.zeros((E, F, 5, 3), dtype=torch.float32, device=self.device)
        self.n_frames = torch.zeros(E, dtype=torch.int32, device=self.device)
        self.dims = (E, n_max, F, int(n_push.max()), int(params.substeps), int(params.iters), int(params.record_every), int(params.settle))
        rho_max = float(np.asarray(scene.rho, F32).max()) if rho_max is None else rho_max
        self.floats = tuple(float(F32(c)) for c in (params.h, params.g, params.mu, params.W, params.T, params.slack, params.tool_y, params.lift, rho_max))

    def launch(self):
        from . import _lib
        _lib.call("ag_sim_pile_push", self.device, self.n, self.rho, self.inv, self.n_push, self.push, self.lat, self.x, self.v, self.obj,
                  self.eef, self.n_frames, *self.dims, *self.floats)
        return self.obj, self.eef, self.n_frames, self.x, self.v


def pile_push(scene, push, params=PILE_DEFAULT, f_max=None, device="cuda:0"):
    """pile_push_host on the GPU: the same arguments, the same five results bit for bit, as tensors on `device`.  scene.x and scene.v may be
    host arrays or tensors (copied: `scene` is not modified).  Raises what pile_push_host raises."""
    call = DevicePilePush(scene, push, params, f_max, device)
    _pile_validate(scene, call.steps, call.dims[2], params)
    return call.launch()


def initial_pile(rng, area_range=(1.0, 9.0)):
    """One layer of granules as src/sim/sim_env/scenes.py:86-109 lays them out: granular_scale U(0.1, 0.3), area U(*area_range), xz_ratio U(0.8, 1.2),
    spacing scale + U(0.1, 0.2) scale, int((extent - scale) / spacing + 1) grains per axis, centred at the origin, each jittered by up to a
    quarter of the gap.  -> (pile (n, 3) float32 at height rho, granular_scale): 9 .. about 700 grains of radius rho = granular_scale / 2."""
    scale = rng.uniform(0.1, 0.3)
    area = rng.uniform(*area_range)
    ratio = rng.uniform(0.8, 1.2)
    gap = rng.uniform(0.1, 0.2) * scale
    ext_x, ext_z = math.sqrt(area * ratio), math.sqrt(area / ratio)
    nx, nz = int((ext_x - scale) / (gap + scale) + 1), int((ext_z - scale) / (gap + scale) + 1)
    gx, gz = np.meshgrid((np.arange(nx) - (nx - 1) / 2) * (gap + scale), (np.arange(nz) - (nz - 1) / 2) * (gap + scale), indexing="ij")
    xz = np.stack([gx.ravel(), gz.ravel()], 1) + rng.uniform(-0.25 * gap, 0.25 * gap, (nx * nz, 2))
    return np.stack([xz[:, 0], np.full(nx * nz, scale / 2), xz[:, 1]], 1).astype(F32), float(scale)


def board_clearance(x, rho, push, params=PILE_DEFAULT):
    """The smallest distance (float64) from a grain centre of x (n, 3) to the board's segment at the START of `push`, minus rho + T."""
    x = np.asarray(x, np.float64)
    s = np.asarray(push, F32).astype(np.float64)[:2]
    u = board_lateral(np.asarray(push, F32)[None])[0].astype(np.float64)
    r = x[:, [0, 2]] - s
    a = np.clip(r @ u, -float(params.W), float(params.W))
    return np.sqrt(((r - a[:, None] * u) ** 2).sum(1)).min() - (float(rho) + float(params.T))


def sample_board_push(x, rho, rng, params=PILE_DEFAULT, tries=200):
    """A push for the pile x (n, 3) of radius rho: a straight segment 0.8 .. 1.6 long through the neighbourhood (within 0.1) of a random grain, in
    a random direction, at whose start the whole board is clear of every grain by more than rho + T, with a margin of rho.  The start is
    moved back along the push direction, in steps of rho, until it is.  -> (4,) float32 xs, zs, xe, ze."""
    x = np.asarray(x, np.float64)
    for _ in range(tries):
        i = int(rng.integers(len(x)))
        through = x[i, [0, 2]] + rng.uniform(-0.1, 0.1, 2)
        a = rng.uniform(0.0, 2.0 * math.pi)
        length = rng.uniform(0.8, 1.6)
        frac = rng.uniform(0.3, 0.7)
        u = np.array([math.cos(a), math.sin(a)])
        for back in range(64):
            s = through - (frac * length + back * float(rho)) * u
            push = np.concatenate([s, s + length * u]).astype(F32)
            if board_clearance(x, rho, push, params) > float(rho):
                if back * float(rho) < (1.0 - frac) * length:      # the board still reaches the point it was aimed through
                    return push
                break
    raise RuntimeError("sample_board_push: no push starts clear of the pile")


# ---------------------------------------------------------------------------------------------------------------------
# The cloth model: a mass-spring grid grasped and dragged by a gripper (the module text)
# ---------------------------------------------------------------------------------------------------------------------
CLOTH_MAX_PARTICLES = 4096     # AG_SIM_CLOTH_MAX_PARTICLES
CLOTH_MAX_SIDE = 64
CLOTH_PICK_K = 5               # AG_SIM_CLOTH_PICK_K (flex_env.py:331)
_NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


@dataclasses.dataclass(frozen=True)
class ClothParams:
    dt: float = 1.0 / 60.0
    substeps: int = 4
    iters: int = 4             # constraint sweeps per substep
    g: float = 9.8
    r: float = 0.03            # particle radius (scenes.py:140): the height of a particle lying on the table
    drag: float = 1.0          # linear drag, 1 / s: v is scaled by 1 - drag h every substep
    speed: float = 0.02        # gripper advance per step
    lift: float = 0.5          # height of the drag's end above the grasp height (flex_env.py:280)
    grasp: float = 0.1         # the nearest particle must be this near the action's start (flex_env.py:312)
    finger: float = 0.2        # half distance of the two finger points
    tool_y: float = 0.03       # height of the finger points at the grasp
    record_every: int = 5
    settle: int = 120          # as for the rope and the pile

    @property
    def h(self):
        return F32(self.dt / self.substeps)

    @property
    def damp(self):
        return F32(1.0 - float(self.drag) * (self.dt / self.substeps))


CLOTH_DEFAULT = ClothParams()


def cloth_stiffness_mapping(sf):
    """The physics parameter `sf` in [0, 1] -> (k_stretch, k_shear, k_bend, mu), float32, in the shape of scenes.py:149-153: with
    f = 0.1 + 1.4 sf, k_stretch = min(max(f, 1), 1.5) / 1.5 (the reference clips its stretch stiffness to 1 .. 1.5: 2/3 up to sf = 0.643, then
    rising to 1), k_shear = min(f, 1), k_bend = min(f, 1) / 2 (both grow with f and are capped), mu = 1 - 0.9 sf (the table's friction)."""
    s = float(sf)
    f = 0.1 + 1.4 * s
    return F32(min(max(f, 1.0), 1.5) / 1.5), F32(min(f, 1.0)), F32(0.5 * min(f, 1.0)), F32(1.0 - 0.9 * s)


@dataclasses.dataclass
class ClothScene:
    """Per-episode state of E cloths, host arrays: nx, nz (E) int32 grid size, l0 (E) rest spacing, ks, kh, kb (E) the gains of the stretch, shear
    and bend constraints, mu (E) the table's friction, x and v (E, n_max, 3) float32 (particle i = iz nx + ix; rows >= nx nz are zero), sf (E) the
    physics parameter the gains were mapped from (or None)."""
    nx: np.ndarray
    nz: np.ndarray
    l0: np.ndarray
    ks: np.ndarray
    kh: np.ndarray
    kb: np.ndarray
    mu: np.ndarray
    x: np.ndarray
    v: np.ndarray
    sf: np.ndarray = None

    @property
    def E(self):
        return len(self.nx)

    @property
    def n(self):
        return (np.asarray(self.nx, np.int64) * np.asarray(self.nz, np.int64)).astype(np.int32)

    @classmethod
    def from_cloths(cls, cloths, sf=None, gains=None, n_max=None, l0=None):
        """cloths: list of (nz_e, nx_e, 3) particle positions; l0 (E) given, or the mean length of the grid's stretch edges; the gains from
        `sf` (E) through cloth_stiffness_mapping, or gains = (ks, kh, kb, mu), (E) each."""
        E = len(cloths)
        nz = np.array([np.shape(c)[0] for c in cloths], np.int32)
        nx = np.array([np.shape(c)[1] for c in cloths], np.int32)
        n = nx.astype(np.int64) * nz
        n_max = int(n.max()) if n_max is None else n_max
        x = np.zeros((E, n_max, 3), F32)
        rest = np.zeros(E, F32)
        for e, c in enumerate(cloths):
            c = np.asarray(c, F32)
            x[e, :n[e]] = c.reshape(-1, 3)
            q = c.astype(np.float64)
            edges = np.concatenate([np.linalg.norm(np.diff(q, axis=0), axis=2).ravel(), np.linalg.norm(np.diff(q, axis=1), axis=2).ravel()])
            rest[e] = F32(edges.mean()) if len(edges) else F32(0)
        if l0 is not None:
            rest = np.asarray(l0, F32).reshape(-1)
        if sf is not None:
            sf = np.asarray(sf, np.float64).reshape(-1)
            gains = tuple(np.array(g, F32) for g in zip(*(cloth_stiffness_mapping(s) for s in sf)))
        ks, kh, kb, mu = (np.asarray(g, F32).reshape(-1) for g in gains)
        return cls(nx, nz, rest, ks, kh, kb, mu, x, np.zeros_like(x), sf)


def cloth_phases(nx, nz):
    """The twelve phases of one sweep over an nx x nz grid, in the module text's order: a list of (I, J) index arrays, pair q of a phase joining
    particles I[q] and J[q].  Within a phase no particle occurs twice."""
    ix, iz = np.meshgrid(np.arange(nx), np.arange(nz))           # (nz, nx)
    idx = iz * nx + ix
    cell = (ix + 1 < nx) & (iz + 1 < nz)
    out = []
    for p in (0, 1):
        out.append((idx[(ix % 2 == p) & (ix + 1 < nx)], 1))
    for p in (0, 1):
        out.append((idx[(iz % 2 == p) & (iz + 1 < nz)], nx))
    for p in (0, 1):
        out.append((idx[cell & (ix % 2 == p)], nx + 1))
    for p in (0, 1):
        out.append((idx[cell & (ix % 2 == p)] + 1, nx - 1))
    for p in (0, 1):
        out.append((idx[((ix >> 1) % 2 == p) & (ix + 2 < nx)], 2))
    for p in (0, 1):
        out.append((idx[((iz >> 1) % 2 == p) & (iz + 2 < nz)], 2 * nx))
    return [(i.astype(np.int64), i.astype(np.int64) + d) for i, d in out]


def grasp_steps(action, params=CLOTH_DEFAULT):
    """action (E, 4) float32 xs, zs, xe, ze -> (steps (E, 2) int32, inv (E, 2) float32): the steps n1, n2 of the drag's two segments and
    1 / (n substeps) of each, in float64 rounded once, as push_steps has them."""
    a = np.asarray(action, F32).astype(np.float64).reshape(-1, 4)
    lift = float(F32(params.lift))
    len3 = np.sqrt((a[:, 2] - a[:, 0]) ** 2 + lift ** 2 + (a[:, 3] - a[:, 1]) ** 2)
    n1 = (len3 / float(params.speed)).astype(np.int64) + 1
    n2 = np.full(len(a), int(lift / float(params.speed)) + 1, np.int64)
    steps = np.stack([n1, n2], 1)
    return steps.astype(np.int32), (1.0 / (steps * int(params.substeps))).astype(F32)


def cloth_pick(x, n, xs, zs, grasp2):
    """The pick of the module text for one episode: x (n_max, 3) float32, its first n rows live.  -> (CLOTH_PICK_K,) int32, -1 where none."""
    dx, dz = x[:n, 0] - F32(xs), x[:n, 2] - F32(zs)
    d2 = dx * dx + dz * dz
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    order = np.argsort(key, kind="stable")[:CLOTH_PICK_K]
    out = np.full(CLOTH_PICK_K, -1, np.int32)
    if len(order) and d2[order[0]] <= grasp2:
        out[:len(order)] = order
    return out


def _cloth_check(scene, action, f_max, params):
    action = np.ascontiguousarray(action, F32).reshape(-1, 4)
    E = scene.E
    if (len(action) != E or scene.x.shape != scene.v.shape or scene.x.shape[0] != E or scene.x.shape[2] != 3
            or any(len(np.reshape(a, -1)) != E for a in (scene.nz, scene.l0, scene.ks, scene.kh, scene.kb, scene.mu))):
        raise ValueError("cloth_push: one action (xs, zs, xe, ze), grid size, l0 and gains per episode and x, v of shape (E, n_max, 3)")
    steps, inv = grasp_steps(action, params)
    need = int(frames_of(steps.sum(1), params).max())
    return action, steps, inv, board_lateral(action), need if f_max is None else int(f_max)


def _cloth_validate(scene, steps, F, params):
    """What cloth_push_host and cloth_push refuse, alike."""
    nx, nz, n_max = np.asarray(scene.nx, np.int64), np.asarray(scene.nz, np.int64), scene.x.shape[1]
    if n_max < 4 or n_max > CLOTH_MAX_PARTICLES:
        raise ValueError(f"cloth_push: n_max = {n_max} outside 4 .. {CLOTH_MAX_PARTICLES}")
    if min(nx.min(), nz.min()) < 2 or max(nx.max(), nz.max()) > CLOTH_MAX_SIDE or (nx * nz).max() > n_max:
        raise ValueError(f"cloth_push: nx, nz outside 2 .. {CLOTH_MAX_SIDE} or nx nz > n_max = {n_max}")
    if int(params.substeps) < 1 or int(params.iters) < 1 or int(params.record_every) < 1:
        raise ValueError("cloth_push: substeps, iters or record_every < 1")
    need = int(frames_of(steps.sum(1), params).max())
    if F < need:
        raise ValueError(f"cloth_push: f_max = {F} frames, the longest drag writes {need}")


def cloth_push_host(scene, action, params=CLOTH_DEFAULT, f_max=None):
    """One grasp-and-drag of every episode of `scene` (the cloth model of the module text).  action (E, 4) float32.  -> obj (E, F, n_max, 3) float32,
    eef (E, F, 2, 3) float32, n_frames (E) int32, picked (E, 5) int32 (-1 where none), x, v (E, n_max, 3) float32 after the settle; frames behind
    an episode's n_frames and rows behind its nx nz are zero.  `scene` is not modified."""
    action, steps, inv, lat, F = _cloth_check(scene, action, f_max, params)
    E, n_max = scene.x.shape[:2]
    _cloth_validate(scene, steps, F, params)
    nx, nz = np.asarray(scene.nx, np.int64), np.asarray(scene.nz, np.int64)
    n = nx * nz
    S, rec, iters = int(params.substeps), int(params.record_every), int(params.iters)
    h, r, damp, lift = params.h, F32(params.r), params.damp, F32(params.lift)
    gh = F32(params.g) * h
    mgh = ((np.asarray(scene.mu, F32) * F32(params.g)) * h)[:, None]
    fing, tool_y = F32(params.finger), F32(params.tool_y)
    grasp2 = F32(params.grasp) * F32(params.grasp)
    l0 = np.asarray(scene.l0, F32)
    lsh = (l0.astype(np.float64) * math.sqrt(2.0)).astype(F32)
    rests = (l0, lsh, l0 * F32(2))
    gains = tuple(np.asarray(g, F32) for g in (scene.ks, scene.kh, scene.kb))
    # the pairs of every phase, all episodes in one flat list each
    per = [cloth_phases(int(nx[e]), int(nz[e])) for e in range(E)]
    phases = []
    for ph in range(12):
        fam = (0, 0, 1, 1, 2, 2)[ph // 2]
        I = np.concatenate([per[e][ph][0] + e * n_max for e in range(E)])
        J = np.concatenate([per[e][ph][1] + e * n_max for e in range(E)])
        cnt = [len(per[e][ph][0]) for e in range(E)]
        phases.append((I, J, np.repeat(rests[fam], cnt), np.repeat(gains[fam], cnt)))
    live = np.arange(n_max)[None, :] < n[:, None]
    sx, sz, ex, ez = (action[:, c:c + 1] for c in range(4))
    ux, uz = lat[:, 0:1], lat[:, 1:2]
    n1, n_push = steps[:, 0].astype(np.int64), steps.sum(1).astype(np.int64)
    inv1, inv2 = inv[:, 0:1], inv[:, 1:2]
    x = np.array(scene.x, F32)
    v = np.array(scene.v, F32)
    # the pick, on the state the call starts from
    picked = np.stack([cloth_pick(x[e], int(n[e]), action[e, 0], action[e, 1], grasp2) for e in range(E)])
    pe, pk = np.nonzero(picked >= 0)
    pi = picked[pe, pk].astype(np.int64)
    offx, offy, offz = x[pe, pi, 0] - action[pe, 0], x[pe, pi, 1], x[pe, pi, 2] - action[pe, 1]
    obj = np.zeros((E, F, n_max, 3), F32)
    eef = np.zeros((E, F, 2, 3), F32)
    total = n_push + int(params.settle)
    rows = np.arange(E)
    one = np.ones((E, n_max), F32)

    def tool_points(f, e_sel, cx, cy, cz):
        fx, fz = fing * ux, fing * uz
        eef[e_sel, f, 0, 0], eef[e_sel, f, 1, 0] = (cx + fx)[e_sel, 0], (cx - fx)[e_sel, 0]
        eef[e_sel, f, 0, 1] = eef[e_sel, f, 1, 1] = (tool_y + cy)[e_sel, 0]
        eef[e_sel, f, 0, 2], eef[e_sel, f, 1, 2] = (cz + fz)[e_sel, 0], (cz - fz)[e_sel, 0]

    with np.errstate(all="ignore"):
        for st in range(int(total.max())):
            run = st < total
            seg1 = (st < n1)[:, None]
            hold = (st < n_push)[pe]                  # the pins still held at this step
            act = live & run[:, None]
            w = one.copy()
            w[pe[hold], pi[hold]] = F32(0)
            wf = w.reshape(-1)
            free = w == F32(1)
            for s in range(S):
                # a. predict
                vy = v[:, :, 1] - gh
                vx, vy, vz = v[:, :, 0] * damp, vy * damp, v[:, :, 2] * damp
                px, py, pz = x[:, :, 0] + h * vx, x[:, :, 1] + h * vy, x[:, :, 2] + h * vz
                # b. the gripper and its pins
                t1 = (np.full((E, 1), st * S + s + 1, np.int64)).astype(F32) * inv1
                t2 = ((st - n1[:, None]) * S + s + 1).astype(F32) * inv2
                cx = np.where(seg1, sx + (ex - sx) * t1, ex)
                cy = np.where(seg1, lift * t1, np.maximum(lift - lift * t2, F32(0)))
                cz = np.where(seg1, sz + (ez - sz) * t1, ez)
                px[pe[hold], pi[hold]] = (cx[pe, 0] + offx)[hold]
                py[pe[hold], pi[hold]] = (cy[pe, 0] + offy)[hold]
                pz[pe[hold], pi[hold]] = (cz[pe, 0] + offz)[hold]
                # c. sweeps
                fx, fy, fz = px.reshape(-1), py.reshape(-1), pz.reshape(-1)          # views: px, py, pz are contiguous
                for _ in range(iters):
                    for I, J, rest, k in phases:
                        dx, dy, dz = fx[J] - fx[I], fy[J] - fy[I], fz[J] - fz[I]
                        ln = np.sqrt((dx * dx + dy * dy) + dz * dz)
                        wi, wj = wf[I], wf[J]
                        ws = wi + wj
                        c = (k * (ln - rest)) / (ln * ws)
                        m = ~(ln == 0) & ~(ws == 0)
                        for f_, d_ in ((fx, dx), (fy, dy), (fz, dz)):
                            cd = c * d_
                            f_[I], f_[J] = np.where(m, f_[I] + wi * cd, f_[I]), np.where(m, f_[J] - wj * cd, f_[J])
                # d. ground
                on = py <= r
                py = np.maximum(py, r)
                # e. velocity and friction
                vx, vy, vz = (px - x[:, :, 0]) / h, (py - x[:, :, 1]) / h, (pz - x[:, :, 2]) / h
                sp = np.sqrt(vx * vx + vz * vz)
                rub = on & free
                f = np.where(sp > mgh, F32(1) - mgh / sp, F32(0))
                vx, vz = np.where(rub, vx * f, vx), np.where(rub, vz * f, vz)
                x = np.where(act[:, :, None], np.stack([px, py, pz], 2), x)
                v = np.where(act[:, :, None], np.stack([vx, vy, vz], 2), v)
            if st % rec == 0 and st < int(n_push.max()):
                e_rec = rows[st < n_push]
                obj[e_rec, st // rec] = x[e_rec]
                tool_points(st // rec, e_rec, cx, cy, cz)
    last = (n_push - 1) // rec + 1
    obj[rows, last] = x
    tool_points(last, rows, ex, np.full((E, 1), lift, F32), ez)
    return obj, eef, (last + 1).astype(np.int32), picked, x, v


def cloth_push_scalar(x, v, nx, nz, l0, gains, action, params=CLOTH_DEFAULT):
    """The cloth model for ONE episode, pair by pair in float32 scalars: slow, and meant to be read.  Within a phase it visits the pairs from the
    LAST to the first, the reverse of cloth_push_host: equal bits show that the colouring is free of conflicts.  x, v (nx nz, 3); gains
    (ks, kh, kb, mu); action (xs, zs, xe, ze).  -> obj (F, n, 3), eef (F, 2, 3), picked (5,), x, v as cloth_push_host returns them for that episode."""
    f = F32
    n = nx * nz
    x, v = [[f(c) for c in p] for p in x], [[f(c) for c in p] for p in v]
    l0 = f(l0)
    ks, kh, kb, mu = (f(c) for c in gains)
    xs, zs, xe, ze = (f(c) for c in action)
    act = np.array([[xs, zs, xe, ze]], F32)
    steps, inv = grasp_steps(act, params)
    n1, n2, inv1, inv2 = int(steps[0, 0]), int(steps[0, 1]), inv[0, 0], inv[0, 1]
    ux, uz = board_lateral(act)[0]
    S, rec = int(params.substeps), int(params.record_every)
    h, r, damp, lift = params.h, f(params.r), params.damp, f(params.lift)
    gh, mgh = f(params.g) * h, (mu * f(params.g)) * h
    fing, tool_y = f(params.finger), f(params.tool_y)
    lsh = f(float(l0) * math.sqrt(2.0))
    at = lambda ix, iz: iz * nx + ix
    # the pairs, phase by phase, each phase listed backwards
    stretch = [[(at(ix, iz), at(ix + 1, iz)) for iz in range(nz) for ix in range(p, nx - 1, 2)] for p in (0, 1)]
    stretch += [[(at(ix, iz), at(ix, iz + 1)) for iz in range(p, nz - 1, 2) for ix in range(nx)] for p in (0, 1)]
    shear = [[(at(ix, iz), at(ix + 1, iz + 1)) for iz in range(nz - 1) for ix in range(p, nx - 1, 2)] for p in (0, 1)]
    shear += [[(at(ix + 1, iz), at(ix, iz + 1)) for iz in range(nz - 1) for ix in range(p, nx - 1, 2)] for p in (0, 1)]
    bend = [[(at(ix, iz), at(ix + 2, iz)) for iz in range(nz) for ix in range(nx - 2) if (ix >> 1) % 2 == p] for p in (0, 1)]
    bend += [[(at(ix, iz), at(ix, iz + 2)) for iz in range(nz - 2) if (iz >> 1) % 2 == p for ix in range(nx)] for p in (0, 1)]
    phases = [(ph[::-1], l0, ks) for ph in stretch] + [(ph[::-1], lsh, kh) for ph in shear] + [(ph[::-1], l0 * f(2), kb) for ph in bend]
    # the pick
    keys = []
    for i in range(n):
        dx, dz = x[i][0] - xs, x[i][2] - zs
        keys.append((int(np.array(dx * dx + dz * dz, F32).view(np.uint32)), i))
    best = sorted(keys)[:CLOTH_PICK_K]
    d2min = np.array(best[0][0], np.uint32).view(F32)
    pins = [i for _, i in best] if d2min <= f(params.grasp) * f(params.grasp) else []
    picked = np.array(pins + [-1] * (CLOTH_PICK_K - len(pins)), np.int32)
    off = {i: (x[i][0] - xs, x[i][1], x[i][2] - zs) for i in pins}
    obj, eef = [], []
    fingers = lambda cx, cy, cz: np.array([[cx + fing * ux, tool_y + cy, cz + fing * uz], [cx - fing * ux, tool_y + cy, cz - fing * uz]], F32)
    with np.errstate(all="ignore"):
        for st in range(n1 + n2 + int(params.settle)):
            held = off if st < n1 + n2 else {}
            w = [f(0) if i in held else f(1) for i in range(n)]
            for s in range(S):
                # a. predict
                p = []
                for i in range(n):
                    vy = v[i][1] - gh
                    p.append([x[i][0] + h * (v[i][0] * damp), x[i][1] + h * (vy * damp), x[i][2] + h * (v[i][2] * damp)])
                # b. the gripper and its pins
                if st < n1:
                    t = f(st * S + s + 1) * inv1
                    cx, cy, cz = xs + (xe - xs) * t, lift * t, zs + (ze - zs) * t
                elif st < n1 + n2:
                    t = f((st - n1) * S + s + 1) * inv2
                    cx, cy, cz = xe, max(lift - lift * t, f(0)), ze
                for i, (ox, oy, oz) in held.items():
                    p[i] = [cx + ox, cy + oy, cz + oz]
                # c. sweeps
                for _ in range(int(params.iters)):
                    for pairs, rest, k in phases:
                        for i, j in pairs:
                            d = [p[j][c] - p[i][c] for c in range(3)]
                            ln = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                            ws = w[i] + w[j]
                            if ln == 0 or ws == 0:
                                continue
                            c_ = (k * (ln - rest)) / (ln * ws)
                            for c in range(3):
                                p[i][c], p[j][c] = p[i][c] + w[i] * (c_ * d[c]), p[j][c] - w[j] * (c_ * d[c])
                for i in range(n):
                    # d. ground
                    on = p[i][1] <= r
                    p[i][1] = max(p[i][1], r)
                    # e. velocity and friction
                    v[i] = [(p[i][c] - x[i][c]) / h for c in range(3)]
                    if on and w[i] == 1:
                        sp = np.sqrt(v[i][0] * v[i][0] + v[i][2] * v[i][2])
                        scale = f(1) - mgh / sp if sp > mgh else f(0)
                        v[i][0], v[i][2] = v[i][0] * scale, v[i][2] * scale
                    x[i] = list(p[i])
            if st < n1 + n2 and st % rec == 0:
                obj.append(np.array(x, F32))
                eef.append(fingers(cx, cy, cz))
    obj.append(np.array(x, F32))
    eef.append(fingers(xe, lift, ze))
    return np.stack(obj), np.stack(eef), picked, np.array(x, F32), np.array(v, F32)


class DeviceClothPush:
    """The arguments of one ag_sim_cloth_push call as device tensors, as DevicePilePush holds those of the pile: `launch()` enqueues the kernel on
    the current stream (no synchronisation, no allocation: it captures into a HIP graph), reading and writing x, v in place and writing obj, eef,
    n_frames, picked.  The arguments go to the library as given: what it refuses comes back as its argument error (RuntimeError), and an episode
    whose nx, nz or step counts lie outside the bounds gets n_frames = 0 with nothing else written."""

    def __init__(self, scene, action, params=CLOTH_DEFAULT, f_max=None, device="cuda:0"):
        import torch
        self.device = torch.device(device)
        action, steps, inv, lat, F = _cloth_check(scene, action, f_max, params)
        E, n_max = scene.x.shape[:2]
        self.host_steps = steps
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.device)
        l0 = np.asarray(scene.l0, F32).reshape(-1)
        rest = np.stack([l0, (l0.astype(np.float64) * math.sqrt(2.0)).astype(F32)], 1)
        self.nx, self.nz, self.steps = up(scene.nx, np.int32), up(scene.nz, np.int32), up(steps, np.int32)
        self.rest, self.inv, self.action, self.lat = up(rest, F32), up(inv, F32), up(action, F32), up(lat, F32)
        self.gains = up(np.stack([np.asarray(g, F32).reshape(-1) for g in (scene.ks, scene.kh, scene.kb, scene.mu)], 1), F32)
        self.x, self.v = (t.to(self.device).contiguous().clone() if isinstance(t, torch.Tensor) else up(t, F32) for t in (scene.x, scene.v))
        self.obj = torch.zeros((E, F, n_max, 3), dtype=torch.float32, device=self.device)
        self.eef = torch.zeros((E, F, 2, 3), dtype=torch.float32, device=self.device)
        self.n_frames = torch.zeros(E, dtype=torch.int32, device=self.device)
        self.picked = torch.full((E, CLOTH_PICK_K), -1, dtype=torch.int32, device=self.device)
        self.dims = (E, n_max, F, int(steps.sum(1).max()), int(params.substeps), int(params.iters), int(params.record_every), int(params.settle))
        grasp2 = F32(params.grasp) * F32(params.grasp)
        self.floats = tuple(float(F32(c)) for c in (params.h, params.g, params.r, params.damp, params.lift, grasp2, params.finger, params.tool_y))

    def launch(self):
        from . import _lib
        _lib.call("ag_sim_cloth_push", self.device, self.nx, self.nz, self.rest, self.gains, self.steps, self.inv, self.action, self.lat, self.x,
                  self.v, self.obj, self.eef, self.n_frames, self.picked, *self.dims, *self.floats)
        return self.obj, self.eef, self.n_frames, self.picked, self.x, self.v


def cloth_push(scene, action, params=CLOTH_DEFAULT, f_max=None, device="cuda:0"):
    """cloth_push_host on the GPU: the same arguments, the same six results bit for bit, as tensors on `device`.  scene.x and scene.v may be
    host arrays or tensors (copied: `scene` is not modified).  Raises what cloth_push_host raises."""
    call = DeviceClothPush(scene, action, params, f_max, device)
    _cloth_validate(scene, call.host_steps, call.dims[2], params)
    return call.launch()


def initial_cloth(rng, nx=None, nz=None, side_range=(2.0, 3.0), rotate=True, r=CLOTH_DEFAULT.r):
    """A flat cloth lying on the table: an nx x nz grid (each drawn from 24 .. 32 when not given) whose longer side is U(*side_range) long -- 2 to 3
    units, the extent that `fps_radius_range` 0.25 covers with `max_nobj` 100 key points --, centred at the origin, turned about the vertical by
    a random angle when `rotate`.  -> (cloth (nz, nx, 3) float32 at height r, l0)."""
    nx = int(rng.integers(24, 33)) if nx is None else int(nx)
    nz = int(rng.integers(24, 33)) if nz is None else int(nz)
    side = rng.uniform(*side_range)
    angle = rng.uniform(0.0, 2.0 * math.pi) if rotate else 0.0
    l0 = side / (max(nx, nz) - 1)
    gx, gz = np.meshgrid((np.arange(nx) - (nx - 1) / 2) * l0, (np.arange(nz) - (nz - 1) / 2) * l0)      # (nz, nx)
    c, sn = math.cos(angle), math.sin(angle)
    return np.stack([c * gx - sn * gz, np.full_like(gx, float(r)), sn * gx + c * gz], 2).astype(F32), float(l0)


def cloth_border(nx, nz):
    """The border particles of an nx x nz grid and the side each lies on, recorded once from the initial layout as flex_env.py:480-495 does (a
    corner belongs to the first side that claims it): -> (idx (B,) int, side (B,) int: 1 ix = nx - 1, 2 ix = 0, 3 iz = nz - 1, 4 iz = 0)."""
    ix, iz = np.meshgrid(np.arange(nx), np.arange(nz))
    ix, iz = ix.ravel(), iz.ravel()
    side = np.where(ix == nx - 1, 1, np.where(ix == 0, 2, np.where(iz == nz - 1, 3, np.where(iz == 0, 4, 0))))
    idx = np.nonzero(side)[0]
    return idx, side[idx]


def sample_grasp(x, border, rng, params=CLOTH_DEFAULT, tries=1000, nx=None):
    """A grasp-and-drag for the cloth x (n, 3) after flex_env.py:472-525: it starts at a random particle of `border` = cloth_border(nx, nz) and ends
    1.0 .. 1.5 away along the outward axis of that particle's side: the grid's own +-ix or +-iz direction as it lies now (taken from the border
    particle to its inner neighbour, so a rotated cloth is pulled along its own axes), accepted when |xe| < 3.5 and |ze| < 2.5.
    nx: the grid's width (default: inferred from the border).  -> (4,) float32 xs, zs, xe, ze."""
    x = np.asarray(x, np.float64)
    idx, side = border
    nx = int(idx[side == 1][0]) + 1 if nx is None else int(nx)
    inward = {1: -1, 2: 1, 3: -nx, 4: nx}
    for _ in range(tries):
        b = int(rng.integers(len(idx)))
        i = int(idx[b])
        dist = rng.uniform(1.0, 1.5)
        out = x[i, [0, 2]] - x[i + inward[int(side[b])], [0, 2]]
        norm = float(np.hypot(*out))
        out = out / norm if norm > 0 else np.array([1.0, 0.0])
        s = x[i, [0, 2]]
        e = s + dist * out
        if abs(e[0]) < 3.5 and abs(e[1]) < 2.5:
            return np.array([s[0], s[1], e[0], e[1]], F32)
    raise RuntimeError("sample_grasp: no drag ends inside the workspace")


# ---------------------------------------------------------------------------------------------------------------------
# The box model: a rigid rectangle with a hidden centre of mass, pushed by a cylinder (the module text)
# ---------------------------------------------------------------------------------------------------------------------
BOX_MAX_PARTICLES = 1024       # AG_SIM_BOX_MAX_PARTICLES
BOX_SIDE_MAX = 4.0             # the largest side from_boxes accepts (box.yaml draws up to 3.0)
BOX_RHO_MAX = 8.0              # bound on |q|: the far corner of a 4 x 4 box seen from a centre of mass at (0.4, 0.4) lies 5.1 away
BOX_K_MAX = 8192.0             # bound on (mu g) / eps: with BOX_RHO_MAX it keeps the integer sums of step d inside 2^51 (the module text)
BOX_COM_MAX = 0.4              # |fx|, |fz| of initial_box (the reference draws up to 0.5: data_gen_box.py:33)


@dataclasses.dataclass(frozen=True)
class BoxParams:
    dt: float = 1.0 / 60.0
    substeps: int = 8
    iters: int = 2             # pusher corrections per substep
    g: float = 9.8
    mu: float = 0.5            # data_gen_box.py:34
    r: float = 0.04            # particle radius: a 3.0 x 2.0 box holds int(3.0 / 0.08) int(2.0 / 0.08) = 37 x 25 = 925 <= 1024 particles
    R: float = 0.1             # pusher radius
    eps: float = 1.0e-3        # the speed under which a particle's friction becomes viscous
    v_rest: float = 1.0e-3     # |V| + |Omega| rho_max under which the box is at rest
    depen: float = 2.0         # a correction deeper than depen pusher advances per substep moves the box without giving it velocity (step b)
    speed: float = 0.01        # pusher advance per step
    record_every: int = 10
    settle: int = 30           # a box released at the pusher's 0.6 / s stops under mu g = 4.9 / s^2 within 8 steps
    lift: float = 0.2

    @property
    def h(self):
        return F32(self.dt / self.substeps)

    @property
    def cap(self):
        return F32(float(self.depen) * float(self.speed) / self.substeps)


BOX_DEFAULT = BoxParams()


def box_masses(k, f, what="x"):
    """Positive weights w (k,) float64, sum 1, of k cells at the centres c_j = (j + 1/2) / k - 1/2 of a unit side whose mean sum_j w_j c_j is f:
    w_j ~ exp(lam c_j), the tilt lam found by bisection (the mean grows with lam from the first centre to the last)."""
    c = (np.arange(k) + 0.5) / k - 0.5
    if not abs(f) < c[-1]:
        raise ValueError(f"from_boxes: a centre of mass at {f} of the side along {what} needs more than {k} cells (|f| < {c[-1]:.4f})")

    def tilt(lam):
        w = np.exp(lam * (c - (c[-1] if lam > 0 else c[0])))
        return w / w.sum()

    lo, hi = -1.0, 1.0
    while (tilt(lo) * c).sum() > f:
        lo *= 2.0
    while (tilt(hi) * c).sum() < f:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if (tilt(mid) * c).sum() < f else (lo, mid)
    return tilt(0.5 * (lo + hi)) if f != 0 else np.full(k, 1.0 / k)


def box_particles(pose, q, n, r):
    """The particles of E boxes at `pose` (E, 4) = X, Z, co, si: (X + ((co qx) - (si qz)), r, Z + ((si qx) + (co qz))), float32, rows >= n zero."""
    pose, q = np.asarray(pose, F32), np.asarray(q, F32)
    X, Z, co, si = (pose[:, c:c + 1] for c in range(4))
    qx, qz = q[:, :, 0], q[:, :, 1]
    live = np.arange(q.shape[1])[None, :] < np.asarray(n, np.int64)[:, None]
    out = np.stack([X + (co * qx - si * qz), np.broadcast_to(F32(r), qx.shape), Z + (si * qx + co * qz)], 2)
    return np.where(live[:, :, None], out, F32(0)).astype(F32)


@dataclasses.dataclass
class BoxScene:
    """Per-episode state of E boxes, host arrays: n (E) int32 particles; q (E, n_max, 2) float32 their rest coordinates relative to the centre of
    mass; m (E, n_max) float32 their masses (sum 1); rect (E, 4) float32 the footprint x_lo, x_hi, z_lo, z_hi relative to the centre of mass;
    inertia (E) = sum m |q|^2; rho_max (E) = max |q| (rounded up); pose (E, 4) = X, Z, co, si of the centre of mass; vel (E, 3) = VX, VZ, Omega;
    x (E, n_max, 3) the particles at `pose` (what SimEnv renders); size (E, 2) the sides a, b; com (E, 2) the centre of mass as a fraction of
    the sides from the geometric centre; grid (E, 2) int32 nx, nz; r the particle radius.  Rows >= n are zero."""
    n: np.ndarray
    q: np.ndarray
    m: np.ndarray
    rect: np.ndarray
    inertia: np.ndarray
    rho_max: np.ndarray
    pose: np.ndarray
    vel: np.ndarray
    x: np.ndarray
    size: np.ndarray
    com: np.ndarray
    grid: np.ndarray
    r: float

    @property
    def E(self):
        return len(self.n)

    @property
    def v(self):
        return self.vel

    @property
    def theta(self):
        p = np.asarray(self.pose, np.float64)
        return np.arctan2(p[:, 3], p[:, 2])

    def row(self, e):
        """Episode e as a scene of its own (views)."""
        return BoxScene(*(getattr(self, f.name)[e:e + 1] for f in dataclasses.fields(self)[:-1]), self.r)

    @classmethod
    def from_boxes(cls, sizes, coms, angles=None, centres=None, grids=None, r=BOX_DEFAULT.r, n_max=None):
        """sizes (E, 2) the sides a, b; coms (E, 2) the fractions fx, fz; angles (E) about the vertical and centres (E, 2) of the GEOMETRIC
        centre (default 0); grids (E, 2) nx, nz (default int(a / (2 r)), int(b / (2 r)), at least 2: the cells are no smaller than a particle).
        Particle i = iz nx + ix sits at the centre of cell (ix, iz) of the nx x nz cells of the rectangle and carries the mass wx[ix] wz[iz]
        of `box_masses`.  All of this in float64, rounded once."""
        sizes, coms = np.asarray(sizes, np.float64).reshape(-1, 2), np.asarray(coms, np.float64).reshape(-1, 2)
        E = len(sizes)
        if sizes.min() <= 0 or sizes.max() > BOX_SIDE_MAX:
            raise ValueError(f"from_boxes: a side outside (0, {BOX_SIDE_MAX}]")
        angles = np.zeros(E) if angles is None else np.asarray(angles, np.float64).reshape(E)
        centres = np.zeros((E, 2)) if centres is None else np.asarray(centres, np.float64).reshape(E, 2)
        if grids is None:
            grids = np.maximum((sizes / (2.0 * float(r))).astype(np.int64), 2)
        grids = np.asarray(grids, np.int64).reshape(E, 2)
        n = grids[:, 0] * grids[:, 1]
        n_max = int(n.max()) if n_max is None else int(n_max)
        q, m = np.zeros((E, max(n_max, int(n.max())), 2), F32), np.zeros((E, max(n_max, int(n.max()))), F32)
        rect, inertia, rho_max, pose = np.zeros((E, 4), F32), np.zeros(E, F32), np.zeros(E, F32), np.zeros((E, 4), F32)
        for e in range(E):
            (a, b), (fx, fz), (nx, nz) = sizes[e], coms[e], grids[e]
            wx, wz = box_masses(int(nx), fx, "x"), box_masses(int(nz), fz, "z")
            cx, cz = ((np.arange(nx) + 0.5) / nx - 0.5 - fx) * a, ((np.arange(nz) + 0.5) / nz - 0.5 - fz) * b
            qe = np.stack(np.meshgrid(cx, cz), 2).reshape(-1, 2)                  # (nz nx, 2): i = iz nx + ix
            me = (wz[:, None] * wx[None, :]).reshape(-1)
            q[e, :n[e]], m[e, :n[e]] = qe, me
            rect[e] = (-0.5 - fx) * a, (0.5 - fx) * a, (-0.5 - fz) * b, (0.5 - fz) * b
            inertia[e] = (me * (qe ** 2).sum(1)).sum()
            rho_max[e] = np.nextafter(F32(np.sqrt((qe ** 2).sum(1).max())), F32(np.inf))
            co, si = math.cos(angles[e]), math.sin(angles[e])
            pose[e] = centres[e, 0] + co * fx * a - si * fz * b, centres[e, 1] + si * fx * a + co * fz * b, co, si
        n = n.astype(np.int32)
        return cls(n, q, m, rect, inertia, rho_max, pose, np.zeros((E, 3), F32), box_particles(pose, q, n, r), sizes.astype(F32),
                   coms.astype(F32), grids.astype(np.int32), float(r))


def _box_check(scene, push, f_max, params):
    push = np.ascontiguousarray(push, F32).reshape(-1, 4)
    E = scene.E
    q, m = np.shape(scene.q), np.shape(scene.m)
    if (len(push) != E or len(q) != 3 or q[0] != E or q[2] != 2 or m != q[:2] or np.shape(scene.pose) != (E, 4) or np.shape(scene.vel) != (E, 3)
            or np.shape(scene.rect) != (E, 4) or any(len(np.reshape(a, -1)) != E for a in (scene.inertia, scene.rho_max))):
        raise ValueError("box_push: one push (xs, zs, xe, ze), rect, inertia, rho_max, pose (4) and vel (3) per episode and q (E, n_max, 2), m (E, n_max)")
    if int(params.substeps) < 1 or int(params.iters) < 1 or int(params.record_every) < 1:
        raise ValueError("box_push: substeps, iters or record_every < 1")
    n_push, inv = push_steps(push, params)
    need = int(frames_of(n_push, params).max())
    return push, n_push, inv, need if f_max is None else int(f_max)


def _box_validate(scene, n_push, F, params):
    """What box_push_host and box_push refuse, alike."""
    n, n_max = np.asarray(scene.n, np.int64), np.shape(scene.q)[1]
    if n_max < 4 or n_max > BOX_MAX_PARTICLES:
        raise ValueError(f"box_push: n_max = {n_max} outside 4 .. {BOX_MAX_PARTICLES}")
    if n.min() < 4 or n.max() > n_max:
        raise ValueError(f"box_push: n outside 4 .. {n_max}")
    inertia, rho_max = np.asarray(scene.inertia, F32), np.asarray(scene.rho_max, F32)
    if not (inertia > 0).all() or not (rho_max > 0).all() or rho_max.max() > F32(BOX_RHO_MAX):
        raise ValueError(f"box_push: inertia <= 0 or rho_max outside (0, {BOX_RHO_MAX}]")
    m, q = np.asarray(scene.m, F32), np.asarray(scene.q, F32)
    if m.min() < 0 or m.max() > 1 or (np.sqrt((q.astype(np.float64) ** 2).sum(2)).max(1) > rho_max).any():
        raise ValueError("box_push: a mass outside 0 .. 1 or a rest coordinate beyond rho_max")
    if not F32(params.eps) > 0 or (F32(params.mu) * F32(params.g)) / F32(params.eps) > F32(BOX_K_MAX):
        raise ValueError(f"box_push: (mu g) / eps outside (0, {BOX_K_MAX}]")
    if F < int(frames_of(n_push, params).max()):
        raise ValueError(f"box_push: f_max = {F} frames, the longest push writes {int(frames_of(n_push, params).max())}")


def _cayley(co, si, t):
    """(co, si) turned by the rotation of Cayley parameter t (the angle 2 atan t) and renormalised; left as it is where t == 0."""
    tt = t * t
    den = F32(1) + tt
    cr, sr = (F32(1) - tt) / den, (t + t) / den
    c2, s2 = co * cr - si * sr, si * cr + co * sr
    nn = np.sqrt(c2 * c2 + s2 * s2)
    still = t == 0
    return np.where(still, co, c2 / nn), np.where(still, si, s2 / nn)


def _exact(total):
    """An integer sum of terms scaled by 2^22 (|total| < 2^53) -> float32: through float64 (exact), rounded once, times 2^-22 (exact)."""
    return np.asarray(total, np.int64).astype(np.float64).astype(F32) * _IQ22


def box_push_host(scene, push, params=BOX_DEFAULT, f_max=None):
    """One push of every episode of `scene` (the box model of the module text).  push (E, 4) float32.  -> obj (E, F, n_max, 3) float32, eef (E, F, 3)
    float32, pose (E, F, 4) float32 the recorded X, Z, co, si, n_frames (E) int32, and the pose (E, 4) and velocity (E, 3) after the settle; frames
    behind an episode's n_frames and rows behind its n are zero.  `scene` is not modified."""
    push, n_push, inv, F = _box_check(scene, push, f_max, params)
    E, n_max = np.shape(scene.q)[:2]
    _box_validate(scene, n_push, F, params)
    n = np.asarray(scene.n, np.int64)
    S, rec, iters = int(params.substeps), int(params.record_every), int(params.iters)
    h, r, R, eps, v_rest, cap = params.h, F32(params.r), F32(params.R), F32(params.eps), F32(params.v_rest), params.cap
    mug = F32(params.mu) * F32(params.g)
    qx, qz, m = np.asarray(scene.q, F32)[:, :, 0], np.asarray(scene.q, F32)[:, :, 1], np.asarray(scene.m, F32)
    xlo, xhi, zlo, zhi = (np.asarray(scene.rect, F32)[:, c] for c in range(4))
    I, rho_max = np.asarray(scene.inertia, F32).reshape(-1), np.asarray(scene.rho_max, F32).reshape(-1)
    live = np.arange(n_max)[None, :] < n[:, None]
    sx, sz, ex, ez = (push[:, c] for c in range(4))
    X, Z, co, si = (np.array(scene.pose, F32)[:, c] for c in range(4))
    VX, VZ, Om = (np.array(scene.vel, F32)[:, c] for c in range(3))
    obj, eef, posef = np.zeros((E, F, n_max, 3), F32), np.zeros((E, F, 3), F32), np.zeros((E, F, 4), F32)
    total = n_push + int(params.settle)
    rows = np.arange(E)
    one, half, zero = F32(1), F32(0.5), F32(0)
    with np.errstate(all="ignore"):
        for st in range(int(total.max())):
            run = st < total
            pushing = st < n_push
            for s in range(S):
                X0, Z0, co0, si0 = X, Z, co, si
                # a. predict
                pX, pZ = X + h * VX, Z + h * VZ
                pc, ps = _cayley(co, si, (Om * h) * half)
                # b. pusher
                t = np.full(E, st * S + s + 1, F32) * inv
                cpx, cpz = sx + (ex - sx) * t, sz + (ez - sz) * t
                for _ in range(iters):
                    dx, dz = cpx - pX, cpz - pZ
                    lx, lz = pc * dx + ps * dz, pc * dz - ps * dx
                    kx, kz = np.minimum(np.maximum(lx, xlo), xhi), np.minimum(np.maximum(lz, zlo), zhi)
                    gx, gz = lx - kx, lz - kz
                    dist = np.sqrt(gx * gx + gz * gz)
                    inside = dist == 0
                    d0, d1, d2, d3 = lx - xlo, xhi - lx, lz - zlo, zhi - lz
                    dmin = np.minimum(np.minimum(d0, d1), np.minimum(d2, d3))
                    f0, f1, f2 = d0 == dmin, d1 == dmin, d2 == dmin
                    nbx = np.where(inside, np.where(f0, one, np.where(f1, -one, zero)), -(gx / dist))
                    nbz = np.where(inside, np.where(f0 | f1, zero, np.where(f2, one, -one)), -(gz / dist))
                    pcx = np.where(inside, np.where(f0, xlo, np.where(f1, xhi, lx)), kx)
                    pcz = np.where(inside, np.where(f0 | f1, lz, np.where(f2, zlo, zhi)), kz)
                    pen = np.where(inside, dmin + R, R - dist)
                    hit = pushing & (inside | (dist < R))
                    cr = pcx * nbz - pcz * nbx
                    w = one + (cr * cr) / I
                    nwx, nwz = pc * nbx - ps * nbz, ps * nbx + pc * nbz
                    # the part of the penetration beyond cap: the box AND the substep's start move alike, so no velocity comes of it
                    tele = hit & (pen > cap)
                    lam = (pen - cap) / w
                    t1 = ((cr * lam) / I) * half
                    pX, pZ, X0, Z0 = (np.where(tele, c_ + lam * n_, c_) for c_, n_ in ((pX, nwx), (pZ, nwz), (X0, nwx), (Z0, nwz)))
                    (tc, ts), (t0c, t0s) = _cayley(pc, ps, t1), _cayley(co0, si0, t1)
                    pc, ps, co0, si0 = np.where(tele, tc, pc), np.where(tele, ts, ps), np.where(tele, t0c, co0), np.where(tele, t0s, si0)
                    # the part up to cap
                    lam = np.minimum(pen, cap) / w
                    tc, ts = _cayley(pc, ps, ((cr * lam) / I) * half)
                    pX, pZ = np.where(hit, pX + lam * nwx, pX), np.where(hit, pZ + lam * nwz, pZ)
                    pc, ps = np.where(hit, tc, pc), np.where(hit, ts, ps)
                # c. velocity
                wx, wz = (pX - X0) / h, (pZ - Z0) / h
                crel, srel = pc * co0 + ps * si0, ps * co0 - pc * si0
                trel = srel / (one + crel)
                wo = (trel + trel) / h
                # d. support friction
                rx, rz = pc[:, None] * qx - ps[:, None] * qz, ps[:, None] * qx + pc[:, None] * qz
                ux, uz = wx[:, None] - wo[:, None] * rz, wz[:, None] + wo[:, None] * rx
                k = (m * mug) / np.maximum(np.sqrt(ux * ux + uz * uz), eps)
                S0, Sx, Sz, S2 = (_exact(np.where(live, np.rint(term * _Q22), zero).astype(np.int64).sum(1))
                                  for term in (k, k * rx, k * rz, k * (rx * rx + rz * rz)))
                a, b, c, d = one + h * S0, -(h * Sz), h * Sx, I + h * S2
                r3 = I * wo
                wo = (r3 - (b * wx + c * wz) / a) / (d - (b * b + c * c) / a)
                wx, wz = (wx - b * wo) / a, (wz - c * wo) / a
                rest = np.sqrt(wx * wx + wz * wz) + np.maximum(wo, -wo) * rho_max < v_rest
                wx, wz, wo = np.where(rest, zero, wx), np.where(rest, zero, wz), np.where(rest, zero, wo)
                X, Z, co, si = np.where(run, pX, X), np.where(run, pZ, Z), np.where(run, pc, co), np.where(run, ps, si)
                VX, VZ, Om = np.where(run, wx, VX), np.where(run, wz, VZ), np.where(run, wo, Om)
            if st % rec == 0 and st < int(n_push.max()):
                e_rec = rows[st < n_push]
                pose = np.stack([X, Z, co, si], 1)
                obj[e_rec, st // rec] = box_particles(pose, scene.q, n, r)[e_rec]
                eef[e_rec, st // rec, 0], eef[e_rec, st // rec, 1], eef[e_rec, st // rec, 2] = cpx[e_rec], r, cpz[e_rec]
                posef[e_rec, st // rec] = pose[e_rec]
    last = (n_push - 1) // rec + 1
    pose = np.stack([X, Z, co, si], 1).astype(F32)
    obj[rows, last] = box_particles(pose, scene.q, n, r)
    eef[rows, last, 0], eef[rows, last, 1], eef[rows, last, 2] = push[:, 2], r + F32(params.lift), push[:, 3]
    posef[rows, last] = pose
    return obj, eef, posef, (last + 1).astype(np.int32), pose, np.stack([VX, VZ, Om], 1).astype(F32)


def box_push_scalar(q, m, rect, inertia, rho_max, pose, vel, push, params=BOX_DEFAULT):
    """The box model for ONE episode in float32 scalars, particle by particle, the four sums of step d as Python integers: slow, and meant to be
    read.  q (n, 2), m (n), rect (4), pose (4), vel (3); push (xs, zs, xe, ze).  -> obj (F, n, 3), eef (F, 3), pose (F, 4), and the pose and velocity
    after the settle, as box_push_host returns them for that episode (tests/test_sim_box_cpu.py holds the vectorised code to it bit for bit)."""
    f = F32
    n = len(q)
    q, m = [[f(c) for c in p] for p in q], [f(c) for c in m]
    xlo, xhi, zlo, zhi = (f(c) for c in rect)
    I, rho_max = f(inertia), f(rho_max)
    X, Z, co, si = (f(c) for c in pose)
    VX, VZ, Om = (f(c) for c in vel)
    xs, zs, xe, ze = (f(c) for c in push)
    steps, inv = push_steps(np.array([[xs, zs, xe, ze]], F32), params)
    n_push, inv = int(steps[0]), inv[0]
    S, rec = int(params.substeps), int(params.record_every)
    h, r, R, eps, v_rest, cap = params.h, f(params.r), f(params.R), f(params.eps), f(params.v_rest), params.cap
    mug = f(params.mu) * f(params.g)
    one, half, zero = f(1), f(0.5), f(0)

    def turn(co, si, t):
        if t == 0:
            return co, si
        tt = t * t
        den = one + tt
        cr, sr = (one - tt) / den, (t + t) / den
        c2, s2 = co * cr - si * sr, si * cr + co * sr
        nn = np.sqrt(c2 * c2 + s2 * s2)
        return c2 / nn, s2 / nn

    def to_f32(total):
        return f(float(total)) * _IQ22            # |total| < 2^53: float() is exact, f() rounds once

    def frame():
        return np.array([[X + (co * qx - si * qz), r, Z + (si * qx + co * qz)] for qx, qz in q], F32), np.array([X, Z, co, si], F32)

    obj, eef, posef = [], [], []
    with np.errstate(all="ignore"):
        for st in range(n_push + int(params.settle)):
            for s in range(S):
                X0, Z0, co0, si0 = X, Z, co, si
                # a. predict
                X, Z = X + h * VX, Z + h * VZ
                co, si = turn(co, si, (Om * h) * half)
                # b. pusher
                if st < n_push:
                    t = f(st * S + s + 1) * inv
                    cx, cz = xs + (xe - xs) * t, zs + (ze - zs) * t
                    for _ in range(int(params.iters)):
                        dx, dz = cx - X, cz - Z
                        lx, lz = co * dx + si * dz, co * dz - si * dx
                        kx, kz = min(max(lx, xlo), xhi), min(max(lz, zlo), zhi)
                        gx, gz = lx - kx, lz - kz
                        dist = np.sqrt(gx * gx + gz * gz)
                        if dist == 0:                                    # inside: out through the nearest face, the first of x_lo, x_hi, z_lo, z_hi
                            faces = [(lx - xlo, one, zero, xlo, lz), (xhi - lx, -one, zero, xhi, lz), (lz - zlo, zero, one, lx, zlo),
                                     (zhi - lz, zero, -one, lx, zhi)]
                            dmin = min(min(faces[0][0], faces[1][0]), min(faces[2][0], faces[3][0]))
                            _, nbx, nbz, pcx, pcz = next(fc for fc in faces if fc[0] == dmin)
                            pen = dmin + R
                        elif dist < R:
                            nbx, nbz, pcx, pcz, pen = -(gx / dist), -(gz / dist), kx, kz, R - dist
                        else:
                            continue
                        cr = pcx * nbz - pcz * nbx
                        w = one + (cr * cr) / I
                        nwx, nwz = co * nbx - si * nbz, si * nbx + co * nbz
                        if pen > cap:                                    # beyond cap: the box and the substep's start alike
                            lam = (pen - cap) / w
                            t1 = ((cr * lam) / I) * half
                            X, Z, X0, Z0 = X + lam * nwx, Z + lam * nwz, X0 + lam * nwx, Z0 + lam * nwz
                            (co, si), (co0, si0) = turn(co, si, t1), turn(co0, si0, t1)
                        lam = min(pen, cap) / w
                        X, Z = X + lam * nwx, Z + lam * nwz
                        co, si = turn(co, si, ((cr * lam) / I) * half)
                # c. velocity
                wx, wz = (X - X0) / h, (Z - Z0) / h
                crel, srel = co * co0 + si * si0, si * co0 - co * si0
                trel = srel / (one + crel)
                wo = (trel + trel) / h
                # d. support friction
                t0 = tx = tz = t2 = 0
                for i in range(n):
                    rx, rz = co * q[i][0] - si * q[i][1], si * q[i][0] + co * q[i][1]
                    ux, uz = wx - wo * rz, wz + wo * rx
                    k = (m[i] * mug) / max(np.sqrt(ux * ux + uz * uz), eps)
                    t0, tx, tz = t0 + int(np.rint(k * _Q22)), tx + int(np.rint((k * rx) * _Q22)), tz + int(np.rint((k * rz) * _Q22))
                    t2 += int(np.rint((k * (rx * rx + rz * rz)) * _Q22))
                S0, Sx, Sz, S2 = to_f32(t0), to_f32(tx), to_f32(tz), to_f32(t2)
                a, b, c, d = one + h * S0, -(h * Sz), h * Sx, I + h * S2
                r3 = I * wo
                wo = (r3 - (b * wx + c * wz) / a) / (d - (b * b + c * c) / a)
                wx, wz = (wx - b * wo) / a, (wz - c * wo) / a
                if np.sqrt(wx * wx + wz * wz) + max(wo, -wo) * rho_max < v_rest:
                    wx = wz = wo = zero
                VX, VZ, Om = wx, wz, wo
            if st < n_push and st % rec == 0:
                o, p = frame()
                obj.append(o), eef.append(np.array([cx, r, cz], F32)), posef.append(p)
    o, p = frame()
    obj.append(o), eef.append(np.array([xe, r + f(params.lift), ze], F32)), posef.append(p)
    return np.stack(obj), np.stack(eef), np.stack(posef), p, np.array([VX, VZ, Om], F32)


class DeviceBoxPush:
    """The arguments of one ag_sim_box_push call as device tensors, as DeviceClothPush holds those of the cloth: `launch()` enqueues the kernel on
    the current stream (no synchronisation, no allocation: it captures into a HIP graph), reading and writing pose, vel in place and writing obj,
    eef, pose_frames, n_frames.  The arguments go to the library as given: what it refuses comes back as its argument error (RuntimeError), and
    an episode whose n, n_push, inertia or rho_max lies outside the bounds gets n_frames = 0 with nothing else written."""

    def __init__(self, scene, push, params=BOX_DEFAULT, f_max=None, device="cuda:0"):
        import torch
        self.device = torch.device(device)
        push, n_push, inv, F = _box_check(scene, push, f_max, params)
        E, n_max = np.shape(scene.q)[:2]
        self.steps = n_push      # (host copy)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.device)
        body = np.concatenate([np.asarray(scene.rect, F32), np.asarray(scene.inertia, F32).reshape(-1, 1),
                               np.asarray(scene.rho_max, F32).reshape(-1, 1)], 1)                      # (E, 6)
        self.n, self.n_push = up(scene.n, np.int32), up(n_push, np.int32)
        self.q, self.m, self.body, self.inv, self.push = up(scene.q, F32), up(scene.m, F32), up(body, F32), up(inv, F32), up(push, F32)
        self.pose, self.vel = (t.to(self.device).contiguous().clone() if isinstance(t, torch.Tensor) else up(t, F32) for t in (scene.pose, scene.vel))
        self.obj = torch.zeros((E, F, n_max, 3), dtype=torch.float32, device=self.device)
        self.eef = torch.zeros((E, F, 3), dtype=torch.float32, device=self.device)
        self.pose_frames = torch.zeros((E, F, 4), dtype=torch.float32, device=self.device)
        self.n_frames = torch.zeros(E, dtype=torch.int32, device=self.device)
        self.dims = (E, n_max, F, int(n_push.max()), int(params.substeps), int(params.iters), int(params.record_every), int(params.settle))
        self.floats = tuple(float(F32(c)) for c in (params.h, params.g, params.mu, params.r, params.R, params.eps, params.v_rest, params.cap, params.lift))

    def launch(self):
        from . import _lib
        _lib.call("ag_sim_box_push", self.device, self.n, self.q, self.m, self.body, self.inv, self.n_push, self.push, self.pose, self.vel,
                  self.obj, self.eef, self.pose_frames, self.n_frames, *self.dims, *self.floats)
        return self.obj, self.eef, self.pose_frames, self.n_frames, self.pose, self.vel


def box_push(scene, push, params=BOX_DEFAULT, f_max=None, device="cuda:0"):
    """box_push_host on the GPU: the same arguments, the same six results bit for bit, as tensors on `device`.  scene.pose and scene.vel may be
    host arrays or tensors (copied: `scene` is not modified).  Raises what box_push_host raises."""
    call = DeviceBoxPush(scene, push, params, f_max, device)
    _box_validate(scene, call.steps, call.dims[2], params)
    return call.launch()


def initial_box(rng):
    """A box as data_gen_box.py:26-33 draws it, in units of 100 px: sides a U(1.5, 3.0), b U(0.5, 2.0) (box.yaml:14-15), the centre of mass a
    fraction U(-0.4, 0.4) of each side from the geometric centre (the reference draws +-0.5; the edge is left out so that the masses stay
    bounded), turned about the vertical by a random angle, the geometric centre at the origin.  -> (size (2,), com (2,), angle)."""
    size = np.array([rng.uniform(1.5, 3.0), rng.uniform(0.5, 2.0)])
    com = rng.uniform(-BOX_COM_MAX, BOX_COM_MAX, 2)
    return size, com, float(rng.uniform(0.0, 2.0 * math.pi))


def sample_box_push(scene_row, rng, length=5.0):
    """A push for the box `scene_row` (a BoxScene of one episode: `scene.row(e)`) after data_gen_box.py:42-56: one of the four sides, a start
    1.0 .. 2.0 outside it at a lateral position drawn uniformly along it, straight across over `length` (50 frames of 0.1), all in the box's
    current frame, so that a turned box is still pushed squarely.  -> (4,) float32 xs, zs, xe, ze."""
    a, b = (float(c) for c in scene_row.size[0])
    fx, fz = (float(c) for c in scene_row.com[0])
    X, Z, co, si = (float(c) for c in np.asarray(scene_row.pose, np.float64)[0])
    side = int(rng.integers(4))
    if side == 0:        # from +z to -z
        s, d = (rng.uniform(-a / 2, a / 2), b / 2 + rng.uniform(1.0, 2.0)), (0.0, -1.0)
    elif side == 1:      # from -z to +z
        s, d = (rng.uniform(-a / 2, a / 2), -b / 2 - rng.uniform(1.0, 2.0)), (0.0, 1.0)
    elif side == 2:      # from -x to +x
        s, d = (-a / 2 - rng.uniform(1.0, 2.0), rng.uniform(-b / 2, b / 2)), (1.0, 0.0)
    else:                # from +x to -x
        s, d = (a / 2 + rng.uniform(1.0, 2.0), rng.uniform(-b / 2, b / 2)), (-1.0, 0.0)
    e = (s[0] + length * d[0], s[1] + length * d[1])
    out = []
    for px, pz in (s, e):                                # geometric-centre frame -> centre-of-mass frame -> world
        lx, lz = px - fx * a, pz - fz * b
        out += [X + co * lx - si * lz, Z + si * lx + co * lz]
    return np.array(out, F32)
