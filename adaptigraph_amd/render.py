"""Simulated depth cameras: depth and id images of a particle scene from calibrated pinhole cameras, every particle a sphere, the table a plane
(DESIGN.md §8.14).  It is what the reference takes from its simulator's renderer (`pyflex.render(render_depth=True)`, flex_env.py:151-189,
:404-409), for the project's own simulators (sim/): a sphere splat of their particles, NOT FleX's renderer, with no tool and no sensor
noise; colour images are viz.py's, from the id image.

Two paths, one result.  `render_depth_host` is the statement of the arithmetic, in numpy; `render_depth(..., device=)` is one launch of
csrc/ag_render.hip and returns the same bits.  All of it is float64 on float32 inputs, every product and sum rounded on its own in the written
order, only + - * / sqrt:
  camera c     Kinv = inv(K) (numpy, on the host), R, t with p_world = R p_cam + t: the convention of perception.depth_to_points
  sphere i     d_k = float64(p_k) - t_k; c_r = (R[0,r] d_0 + R[1,r] d_1) + R[2,r] d_2 (R^T (p - t)); rr = float64(radius)
  cull         the sphere takes part iff c_2 - rr > near (part of the statement: a sphere nearer than that can still hit pixels)
  pixel (u, v) qx = (Kinv[0,0] u + Kinv[0,1] v) + Kinv[0,2], qy likewise from row 1; A = (qx qx + qy qy) + 1; B = (qx c_0 + qy c_1) + c_2;
               Cc = ((c_0 c_0 + c_1 c_1) + c_2 c_2) - rr rr; disc = B B - A Cc; a hit iff disc >= 0, at d = (B - sqrt(disc)) / A, counted iff
               near < d < far.  d is the depth along the camera's axis: the hit point is d (qx, qy, 1).
  plane        (nx, ny, nz, o), the points with nx x + ny y + nz z = o in the world frame: w_r = (R[r,0] qx + R[r,1] qy) + R[r,2];
               den = (nx w_0 + ny w_1) + nz w_2; num = o - ((nx t_0 + ny t_1) + nz t_2); if den != 0, dp = num / den, counted iff near < dp < far
  winner       the smallest double: spheres in ascending index with strict <, so the lower index keeps a tie; the plane only if strictly smaller
               than every sphere hit
  written      depth = float32(winner), id = the particle index, -1 for the plane; depth = 0 and id = -2 where nothing counts (0 is the "no
               data" value that depth_to_points drops with lo = 0)
The statement has no pixel box in it.  `accelerate=True` and the kernel visit only a box of pixels per sphere that is a superset of its hits:
the sphere lies inside [c_0 +- rr] x [c_1 +- rr] x [c_2 +- rr], whose z is positive after the cull, so x / z over it is extreme at the corners:
u from floor(fx min((c_0 - rr) / z) + cx) - 1 to ceil(fx max((c_0 + rr) / z) + cx) + 1 over z in {c_2 - rr, c_2 + rr}, likewise in v.  That needs
a pinhole (zero skew, last row 0 0 1, fx, fy > 0), which both paths insist on.
"""
import math

import numpy as np

from .perception import _camera_rows

TILE = 32                  # AG_RENDER_TILE: pixels along a tile's edge, one workgroup per tile
CHUNK = 256                # AG_RENDER_CHUNK: particles staged through LDS at a time
MAX_SIDE = 4096            # AG_RENDER_MAX_SIDE
MAX_PARTICLES = 4096       # AG_RENDER_MAX_PARTICLES
ID_PLANE, ID_NONE = -1, -2


def camera_rows(R_list, t_list, intr_list):
    """(C, 25) float64: Kinv, R, t as perception._camera_rows lays them out, then fx, fy, cx, cy.  Raises ValueError unless every K is a pinhole."""
    for K in intr_list:
        K = np.asarray(K, np.float64)
        if K.shape != (3, 3) or K[0, 1] != 0 or K[1, 0] != 0 or K[2, 0] != 0 or K[2, 1] != 0 or K[2, 2] != 1 or not (K[0, 0] > 0 and K[1, 1] > 0):
            raise ValueError("render_depth: intrinsics must be a pinhole [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] with fx, fy > 0")
    if not (len(R_list) == len(t_list) == len(intr_list) >= 1):
        raise ValueError("render_depth: one R, t and K per camera, at least one camera")
    tail = np.stack([[K[0][0], K[1][1], K[0][2], K[1][2]] for K in (np.asarray(K, np.float64) for K in intr_list)])
    return np.concatenate([_camera_rows(R_list, t_list, intr_list), tail], 1)


def _scene(pts, n, radius):
    pts = pts if type(pts).__module__.startswith("torch") else np.ascontiguousarray(pts, np.float32)
    if pts.ndim != 3 or pts.shape[2] != 3 or pts.shape[0] < 1:
        raise ValueError(f"render_depth: pts is (E, n_max, 3); got {tuple(pts.shape)}")
    E, n_max = int(pts.shape[0]), int(pts.shape[1])
    if not 1 <= n_max <= MAX_PARTICLES:
        raise ValueError(f"render_depth: n_max = {n_max} outside 1 .. {MAX_PARTICLES}")
    if tuple(np.shape(n)) != (E,) or tuple(np.shape(radius)) != (E,):
        raise ValueError("render_depth: one n and one radius per episode")
    return pts, E, n_max


def _limits(H, W, near, far):
    if not (1 <= int(H) <= MAX_SIDE and 1 <= int(W) <= MAX_SIDE):
        raise ValueError(f"render_depth: H, W outside 1 .. {MAX_SIDE}")
    if not 0.0 <= float(near) < float(far):
        raise ValueError("render_depth: 0 <= near < far")
    return np.array([float(near), float(far)], np.float64)


def _plane(plane):
    if plane is None:
        return None
    p = np.asarray(plane, np.float64).reshape(-1)
    if p.shape != (4,):
        raise ValueError("render_depth: plane is (nx, ny, nz, o)")
    return p


def _pixel_range(lo, hi, size):
    """The pixels lo .. hi (floats, inclusive) clipped to 0 .. size - 1 as a slice; bounds that are not finite give the whole axis."""
    a = 0 if not math.isfinite(lo) else int(min(max(lo, 0.0), float(size)))
    b = size if not math.isfinite(hi) else int(min(max(hi + 1.0, 0.0), float(size)))
    return slice(a, max(a, b))


def render_depth_host(pts, n, radius, R_list, t_list, intr_list, H, W, plane=None, near=0.05, far=4.0, accelerate=True):
    """The statement (module text).  pts (E, n_max, 3) float32, n (E) int, radius (E) float32.  -> depth (E, C, H, W) float32, id (E, C, H, W) int32.
    `accelerate=True` visits only each sphere's pixel box, False every pixel for every sphere: the same arrays.  An n outside 0 .. n_max renders
    as 0; rows >= n are not read."""
    pts, E, n_max = _scene(pts, n, radius)
    cams = camera_rows(R_list, t_list, intr_list)
    near, far = _limits(H, W, near, far)
    plane = _plane(plane)
    H, W, C = int(H), int(W), len(cams)
    depth = np.zeros((E, C, H, W), np.float32)
    ids = np.full((E, C, H, W), ID_NONE, np.int32)
    u = np.arange(W, dtype=np.float64)[None, :]
    v = np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        for c in range(C):
            Kinv, R, t = cams[c, :9].reshape(3, 3), cams[c, 9:18].reshape(3, 3), cams[c, 18:21]
            fx, fy, cx, cy = cams[c, 21:]
            qx = (Kinv[0, 0] * u + Kinv[0, 1] * v) + Kinv[0, 2]
            qy = (Kinv[1, 0] * u + Kinv[1, 1] * v) + Kinv[1, 2]
            A = (qx * qx + qy * qy) + 1.0
            for e in range(E):
                ne = int(n[e])
                ne = ne if 0 <= ne <= n_max else 0
                rr = np.float64(np.float32(radius[e]))
                best = np.full((H, W), np.inf)
                bid = np.full((H, W), ID_NONE, np.int32)
                d = pts[e, :ne].astype(np.float64) - t[None, :]
                cen = [(R[0, r] * d[:, 0] + R[1, r] * d[:, 1]) + R[2, r] * d[:, 2] for r in range(3)]
                for i in range(ne):
                    c0, c1, c2 = cen[0][i], cen[1][i], cen[2][i]
                    z1 = c2 - rr
                    if not z1 > near:
                        continue
                    rows = cols = slice(None)
                    if accelerate and z1 > 0.0:
                        i1, i2 = 1.0 / z1, 1.0 / (c2 + rr)
                        xl, xh, yl, yh = c0 - rr, c0 + rr, c1 - rr, c1 + rr
                        cols = _pixel_range(np.floor(fx * min(xl * i1, xl * i2) + cx) - 1.0, np.ceil(fx * max(xh * i1, xh * i2) + cx) + 1.0, W)
                        rows = _pixel_range(np.floor(fy * min(yl * i1, yl * i2) + cy) - 1.0, np.ceil(fy * max(yh * i1, yh * i2) + cy) + 1.0, H)
                    sx, sy, sA = qx[rows, cols], qy[rows, cols], A[rows, cols]
                    B = (sx * c0 + sy * c1) + c2
                    Cc = ((c0 * c0 + c1 * c1) + c2 * c2) - rr * rr
                    disc = B * B - sA * Cc
                    dd = (B - np.sqrt(disc)) / sA
                    win = (disc >= 0.0) & (dd > near) & (dd < far) & (dd < best[rows, cols])
                    best[rows, cols] = np.where(win, dd, best[rows, cols])
                    bid[rows, cols] = np.where(win, np.int32(i), bid[rows, cols])
                if plane is not None:
                    w = [(R[r, 0] * qx + R[r, 1] * qy) + R[r, 2] for r in range(3)]
                    den = (plane[0] * w[0] + plane[1] * w[1]) + plane[2] * w[2]
                    num = plane[3] - ((plane[0] * t[0] + plane[1] * t[1]) + plane[2] * t[2])
                    dp = num / den
                    win = (den != 0.0) & (dp > near) & (dp < far) & (dp < best)
                    best = np.where(win, dp, best)
                    bid = np.where(win, np.int32(ID_PLANE), bid)
                depth[e, c] = np.where(bid == ID_NONE, 0.0, best).astype(np.float32)
                ids[e, c] = bid
    return depth, ids


class DeviceRenderer:
    """The cameras, the plane and the limits of ag_render_depth as device tensors, and the output images: `launch(pts, n, radius)` enqueues the one
    kernel on the current stream (no synchronisation, no allocation: it captures into a HIP graph) and returns `depth`, `id`, (E, C, H, W) fp32 /
    int32, which the next launch overwrites.  pts (E, n_max, 3) fp32, n (E) int32, radius (E) fp32: contiguous tensors on the device."""

    def __init__(self, R_list, t_list, intr_list, H, W, plane=None, near=0.05, far=4.0, E=1, device="cuda:0"):
        import torch
        self.device = torch.device(device)
        cams = camera_rows(R_list, t_list, intr_list)
        limits = _limits(H, W, near, far)
        plane = _plane(plane)
        self.E, self.C, self.H, self.W = int(E), len(cams), int(H), int(W)
        self.cams = torch.from_numpy(cams).to(self.device)
        self.limits = torch.from_numpy(limits).to(self.device)
        self.plane = None if plane is None else torch.from_numpy(plane).to(self.device)
        self.depth = torch.empty((self.E, self.C, self.H, self.W), dtype=torch.float32, device=self.device)
        self.id = torch.empty((self.E, self.C, self.H, self.W), dtype=torch.int32, device=self.device)

    def launch(self, pts, n, radius):
        import torch
        from . import _lib
        for name, x, dt, shape in (("pts", pts, torch.float32, (self.E, pts.shape[1] if pts.dim() == 3 else -1, 3)), ("n", n, torch.int32, (self.E,)),
                                   ("radius", radius, torch.float32, (self.E,))):
            if x.device != self.device or x.dtype != dt or tuple(x.shape) != shape or not x.is_contiguous():
                raise ValueError(f"DeviceRenderer: {name} must be a contiguous {dt} tensor of shape {shape} on {self.device}")
        _lib.call("ag_render_depth", self.device, pts, n, radius, self.cams, self.plane, self.limits, self.E, int(pts.shape[1]), self.C, self.H,
                  self.W, self.depth, self.id)
        return self.depth, self.id


def render_depth(pts, n, radius, R_list, t_list, intr_list, H, W, plane=None, near=0.05, far=4.0, device=None):
    """render_depth_host on the GPU: the same arguments (pts may be a tensor), the same two arrays bit for bit, as tensors on `device`.
    device=None runs the host statement and returns numpy."""
    if device is None:
        return render_depth_host(pts, n, radius, R_list, t_list, intr_list, H, W, plane, near, far)
    import torch
    pts, E, n_max = _scene(pts, n, radius)
    r = DeviceRenderer(R_list, t_list, intr_list, H, W, plane, near, far, E, device)
    up = lambda a, np_dt, dt: (a.to(device=r.device, dtype=dt) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, np_dt)).to(r.device)).contiguous()
    return r.launch(up(pts, np.float32, torch.float32), up(n, np.int32, torch.int32), up(radius, np.float32, torch.float32))


# ---------------------------------------------------------------------------------------------------------------------
# cameras
# ---------------------------------------------------------------------------------------------------------------------
def look_at_cameras(positions, target, H, W, fov_deg, up=(0.0, 0.0, 1.0)):
    """Pinhole cameras at `positions` (C, 3) looking at `target` (3,), image H x W, vertical field of view `fov_deg`, square pixels, the principal
    point at the image centre.  -> R_list, t_list, intr_list with p_world = R p_cam + t; the camera's z looks at the target, x is to the right
    and y down in the image, `up` the world's up direction."""
    target, up = np.asarray(target, np.float64), np.asarray(up, np.float64)
    f = 0.5 * float(H) / math.tan(math.radians(float(fov_deg)) / 2.0)
    K = np.array([[f, 0.0, 0.5 * float(W)], [0.0, f, 0.5 * float(H)], [0.0, 0.0, 1.0]])
    R_list, t_list, intr_list = [], [], []
    for pos in np.asarray(positions, np.float64).reshape(-1, 3):
        z = target - pos
        z = z / np.linalg.norm(z)
        x = np.cross(z, up)
        if np.linalg.norm(x) < 1e-12:
            raise ValueError("look_at_cameras: a camera looks along `up`")
        x = x / np.linalg.norm(x)
        y = np.cross(z, x)
        R_list.append(np.stack([x, y, z], 1))
        t_list.append(pos.copy())
        intr_list.append(K.copy())
    return R_list, t_list, intr_list


DEFAULT_FOV_DEG = 30.0


def default_cameras(sim_real_ratio, H=720, W=1280):
    """The reference's four views (src/sim/sim_env/cameras.py:10-15): distance 6 and height 10 in simulator units at 45, 135, 225 and 315
    degrees, expressed in the board frame (simulator (x, y, z) -> board (x, z, -y) / sim_real_ratio) and aimed at the table origin.  The
    reference takes its field of view from FleX's projection matrix, which is not available here: the 30 degrees (vertical) are OURS, chosen
    so that the simulators' 7 x 5 unit work area fills most of a 16:9 image from that distance."""
    s = 1.0 / float(sim_real_ratio)
    pos = [(6.0 * sx * s, 6.0 * sz * s, -10.0 * s) for sx, sz in ((1, 1), (1, -1), (-1, -1), (-1, 1))]
    return look_at_cameras(pos, (0.0, 0.0, 0.0), H, W, DEFAULT_FOV_DEG, up=(0.0, 0.0, -1.0))
