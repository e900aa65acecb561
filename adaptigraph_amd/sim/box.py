"""The box model (`box_push_host` IS its specification, `box_push(..., device=)` is csrc/ag_sim_box.hip: one workgroup of 256 threads
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

from ._common import _IQ22, _Q22, F32, DeviceCall, _as_push, _check_frames, _f_max, push_steps

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
    push = _as_push(push)
    E = scene.E
    q, m = np.shape(scene.q), np.shape(scene.m)
    if (len(push) != E or len(q) != 3 or q[0] != E or q[2] != 2 or m != q[:2] or np.shape(scene.pose) != (E, 4) or np.shape(scene.vel) != (E, 3)
            or np.shape(scene.rect) != (E, 4) or any(len(np.reshape(a, -1)) != E for a in (scene.inertia, scene.rho_max))):
        raise ValueError("box_push: one push (xs, zs, xe, ze), rect, inertia, rho_max, pose (4) and vel (3) per episode and q (E, n_max, 2), m (E, n_max)")
    if int(params.substeps) < 1 or int(params.iters) < 1 or int(params.record_every) < 1:
        raise ValueError("box_push: substeps, iters or record_every < 1")
    n_push, inv = push_steps(push, params)
    return push, n_push, inv, _f_max(n_push, f_max, params)


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
    _check_frames("box_push", "push", n_push, F, params)


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


class DeviceBoxPush(DeviceCall):
    """The arguments of one ag_sim_box_push call (see DeviceCall): pose, vel in place, and `pose_frames` (E, F, 4) written beside obj, eef and
    n_frames.  An episode whose n, n_push, inertia or rho_max lies outside the bounds gets n_frames = 0 with nothing else written."""
    entry = "ag_sim_box_push"
    pointers = ("n", "q", "m", "body", "inv", "n_push", "push", "pose", "vel", "obj", "eef", "pose_frames", "n_frames")
    results = ("obj", "eef", "pose_frames", "n_frames", "pose", "vel")
    state = ("pose", "vel")
    _validate = staticmethod(_box_validate)

    def __init__(self, scene, push, params=BOX_DEFAULT, f_max=None, device="cuda:0"):
        import torch
        push, n_push, inv, F = _box_check(scene, push, f_max, params)
        self.steps = n_push      # (host copy)
        body = np.concatenate([np.asarray(scene.rect, F32), np.asarray(scene.inertia, F32).reshape(-1, 1),
                               np.asarray(scene.rho_max, F32).reshape(-1, 1)], 1)                      # (E, 6)
        super().__init__(scene, params, device, n_push, F, np.shape(scene.q)[1], dict(n=scene.n, n_push=n_push),
                         dict(q=scene.q, m=scene.m, body=body, inv=inv, push=push),
                         (params.h, params.g, params.mu, params.r, params.R, params.eps, params.v_rest, params.cap, params.lift))
        self.pose_frames = torch.zeros((scene.E, F, 4), dtype=torch.float32, device=self.device)


def box_push(scene, push, params=BOX_DEFAULT, f_max=None, device="cuda:0"):
    """box_push_host on the GPU: the same arguments, the same six results bit for bit, as tensors on `device`.  scene.pose and scene.vel may be
    host arrays or tensors (copied: `scene` is not modified).  Raises what box_push_host raises."""
    return DeviceBoxPush(scene, push, params, f_max, device).validate().launch()


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
