"""The cloth model (`cloth_push_host` IS its specification, `cloth_push(..., device=)` is csrc/ag_sim_cloth.hip: one workgroup of
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
"""
import dataclasses
import math

import numpy as np

from ._common import F32, DeviceCall, _as_push, _check_frames, _f_max, _xv_ok, board_lateral

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
    action = _as_push(action)
    E = scene.E
    if (len(action) != E or not _xv_ok(scene)
            or any(len(np.reshape(a, -1)) != E for a in (scene.nz, scene.l0, scene.ks, scene.kh, scene.kb, scene.mu))):
        raise ValueError("cloth_push: one action (xs, zs, xe, ze), grid size, l0 and gains per episode and x, v of shape (E, n_max, 3)")
    steps, inv = grasp_steps(action, params)
    return action, steps, inv, board_lateral(action), _f_max(steps.sum(1), f_max, params)


def _cloth_validate(scene, total, F, params):
    """What cloth_push_host and cloth_push refuse, alike."""
    nx, nz, n_max = np.asarray(scene.nx, np.int64), np.asarray(scene.nz, np.int64), scene.x.shape[1]
    if n_max < 4 or n_max > CLOTH_MAX_PARTICLES:
        raise ValueError(f"cloth_push: n_max = {n_max} outside 4 .. {CLOTH_MAX_PARTICLES}")
    if min(nx.min(), nz.min()) < 2 or max(nx.max(), nz.max()) > CLOTH_MAX_SIDE or (nx * nz).max() > n_max:
        raise ValueError(f"cloth_push: nx, nz outside 2 .. {CLOTH_MAX_SIDE} or nx nz > n_max = {n_max}")
    if int(params.substeps) < 1 or int(params.iters) < 1 or int(params.record_every) < 1:
        raise ValueError("cloth_push: substeps, iters or record_every < 1")
    _check_frames("cloth_push", "drag", total, F, params)


def cloth_push_host(scene, action, params=CLOTH_DEFAULT, f_max=None):
    """One grasp-and-drag of every episode of `scene` (the cloth model of the module text).  action (E, 4) float32.  -> obj (E, F, n_max, 3) float32,
    eef (E, F, 2, 3) float32, n_frames (E) int32, picked (E, 5) int32 (-1 where none), x, v (E, n_max, 3) float32 after the settle; frames behind
    an episode's n_frames and rows behind its nx nz are zero.  `scene` is not modified."""
    action, steps, inv, lat, F = _cloth_check(scene, action, f_max, params)
    E, n_max = scene.x.shape[:2]
    _cloth_validate(scene, steps.sum(1), F, params)
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


class DeviceClothPush(DeviceCall):
    """The arguments of one ag_sim_cloth_push call (see DeviceCall): x, v in place, and `picked` (E, 5) written beside obj, eef and n_frames;
    `steps` (E, 2) is the kernel's argument, a device tensor.  An episode whose nx, nz or step counts lie outside the bounds gets n_frames = 0
    with nothing else written."""
    entry = "ag_sim_cloth_push"
    pointers = ("nx", "nz", "rest", "gains", "steps", "inv", "action", "lat", "x", "v", "obj", "eef", "n_frames", "picked")
    results = ("obj", "eef", "n_frames", "picked", "x", "v")
    tool_shape = (2, 3)
    _validate = staticmethod(_cloth_validate)

    def __init__(self, scene, action, params=CLOTH_DEFAULT, f_max=None, device="cuda:0"):
        import torch
        action, steps, inv, lat, F = _cloth_check(scene, action, f_max, params)
        l0 = np.asarray(scene.l0, F32).reshape(-1)
        rest = np.stack([l0, (l0.astype(np.float64) * math.sqrt(2.0)).astype(F32)], 1)
        gains = np.stack([np.asarray(g, F32).reshape(-1) for g in (scene.ks, scene.kh, scene.kb, scene.mu)], 1)
        grasp2 = F32(params.grasp) * F32(params.grasp)
        super().__init__(scene, params, device, steps.sum(1), F, scene.x.shape[1], dict(nx=scene.nx, nz=scene.nz, steps=steps),
                         dict(rest=rest, gains=gains, inv=inv, action=action, lat=lat),
                         (params.h, params.g, params.r, params.damp, params.lift, grasp2, params.finger, params.tool_y))
        self.picked = torch.full((scene.E, CLOTH_PICK_K), -1, dtype=torch.int32, device=self.device)


def cloth_push(scene, action, params=CLOTH_DEFAULT, f_max=None, device="cuda:0"):
    """cloth_push_host on the GPU: the same arguments, the same six results bit for bit, as tensors on `device`.  scene.x and scene.v may be
    host arrays or tensors (copied: `scene` is not modified).  Raises what cloth_push_host raises."""
    return DeviceClothPush(scene, action, params, f_max, device).validate().launch()


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
