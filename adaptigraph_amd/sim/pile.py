"""The granular model (`pile_push_host` IS its specification, `pile_push(..., device=)` is csrc/ag_sim_pile.hip: one workgroup per
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
"""
import dataclasses
import math

import numpy as np

from ._common import _IQ22, _Q22, F32, DeviceCall, _as_push, _check_frames, _f_max, _xv_ok, board_lateral, push_steps

PILE_MAX_PARTICLES = 1024      # AG_SIM_PILE_MAX_PARTICLES
PILE_RHO_MAX = 0.25            # the bound that keeps 1023 contact terms of at most rho 2^22 inside int32
PILE_KEY_OFFSETS = (1.0, -1.0, 0.0, 0.5, -0.5)      # times W: lateral offsets 0.5, -0.5, 0, 0.25, -0.25 (config/dynamics/granular.yaml:18-25)


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



def _pile_check(scene, push, f_max, params):
    push = _as_push(push)
    if len(push) != scene.E or not _xv_ok(scene) or len(scene.rho) != scene.E:
        raise ValueError("pile_push: one push (xs, zs, xe, ze) and one rho per episode and x, v of shape (E, n_max, 3)")
    n_push, inv = push_steps(push, params)
    return push, n_push, inv, board_lateral(push), _f_max(n_push, f_max, params)


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
    _check_frames("pile_push", "push", n_push, F, params)


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


class DevicePilePush(DeviceCall):
    """The arguments of one ag_sim_pile_push call (see DeviceCall): x, v in place.  `rho_max`, the host's bound on the device-side radii, defaults
    to the largest of the scene.  An episode whose n, n_push or rho lies outside the bounds gets n_frames = 0 with nothing else written."""
    entry = "ag_sim_pile_push"
    pointers = ("n", "rho", "inv", "n_push", "push", "lat", "x", "v", "obj", "eef", "n_frames")
    results = ("obj", "eef", "n_frames", "x", "v")
    tool_shape = (5, 3)
    _validate = staticmethod(_pile_validate)

    def __init__(self, scene, push, params=PILE_DEFAULT, f_max=None, device="cuda:0", rho_max=None):
        push, n_push, inv, lat, F = _pile_check(scene, push, f_max, params)
        self.steps = n_push      # (host copy)
        rho_max = float(np.asarray(scene.rho, F32).max()) if rho_max is None else rho_max
        super().__init__(scene, params, device, n_push, F, scene.x.shape[1], dict(n=scene.n, n_push=n_push),
                         dict(rho=scene.rho, inv=inv, push=push, lat=lat),
                         (params.h, params.g, params.mu, params.W, params.T, params.slack, params.tool_y, params.lift, rho_max))


def pile_push(scene, push, params=PILE_DEFAULT, f_max=None, device="cuda:0"):
    """pile_push_host on the GPU: the same arguments, the same five results bit for bit, as tensors on `device`.  scene.x and scene.v may be
    host arrays or tensors (copied: `scene` is not modified).  Raises what pile_push_host raises."""
    return DevicePilePush(scene, push, params, f_max, device).validate().launch()


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
