"""Rollout and planning records drawn as images: what the reference draws with cv2 at every stage -- `visualize_graph`
(src/dynamics/rollout/graph.py:44-230: key points, tool, edges, motion trails, pred | gt side by side) and `visualize_img`
(src/planning/plan_utils.py:104-300: start state and edges, action arrows, predicted state and target as a half-transparent overlay) -- for the
project's own records.  What it is NOT: our coverage rule is not cv2's Bresenham lines or its anti-aliasing; there is no text (JPEG files and
videos of the frames: jpeg.py); particles are spheres (the background is render.py's sphere splat); the overlay is a fixed-point blend.

Two paths, one result.  `draw_host` is the statement of the arithmetic, in numpy; `draw(..., device=)` / `DeviceCanvas.launch` is one call of
csrc/ag_draw.hip (two launches) and returns the same bits.  A frame is drawn from a DISPLAY LIST, primitives in paint order over a background:
  pts    (n_pts, 3) float32   points in the cameras' world (board) frame
  prims  (n_prim, 4) int32    point a, point b (b == a for a disc), style, 0
  styles (n_style, 4) int32   kind (0 disc about a, 1 segment a -> b), size (disc radius / segment width in pixels, 0 .. 64), layer (0 opaque,
                              1 overlay), colour 0xRRGGBB
  frames (F, 4) int32         camera, first primitive, primitive count, background index
  cams   (C, 25) float64      render.camera_rows
  background, one mode per call: 0 the colour color0; 1 `bg` = (n_bg, H, W, 4) uint8 images (alpha ignored); 2 `bg` = (n_bg, H, W) int32 id
                              images as ag_render_depth writes them and `palette` (n_pal,) int32: palette[id % n_pal] for id >= 0, color0 for
                              -1 (the table), color1 otherwise (nothing).  A background index outside 0 .. n_bg - 1 gives color0.
  out    (F, H, W, 4) uint8   R, G, B and the alpha byte 255
Projection of point p in camera c, float64 on float32 inputs, every product and sum rounded on its own in the written order:
  d = float64(p) - t; c_r = (R[0,r] d_0 + R[1,r] d_1) + R[2,r] d_2; the point is valid iff c_2 > near
  x = trunc(fx (c_0 / c_2) + cx), y = trunc(fy (c_1 / c_2) + cy)  (toward zero, the reference's int(...)); invalid if either is not finite
  or exceeds 16 383 in magnitude.
A primitive is DROPPED if a point or style index is out of range (it is never dereferenced), if its kind, size or layer is none of the above,
or if an endpoint it uses is invalid (a disc uses a alone; segments are not clipped against the near plane).  A frame's primitive range is
clipped to 0 .. n_prim and is empty for a camera outside 0 .. C - 1.
Coverage of pixel p = (u, v), all int64:
  disc     (u - a_x)^2 + (v - a_y)^2 <= size^2
  segment  d = b - a, L2 = d.d, q = p - a, s = q.d, X = q_x d_y - q_y d_x:
           L2 == 0 or s < 0: 4 |p - a|^2 <= size^2;  s > L2: 4 |p - b|^2 <= size^2 (round caps);  otherwise 4 X^2 <= size^2 L2
  (a == b is the disc of diameter size).  With |coordinates| <= 16 383, pixels in 0 .. 4 095 and size <= 64: |q| <= 20 478 and |d| <= 32 766 per
  component, so |s|, |X| <= 2 * 20 478 * 32 766 < 1.35e9 and 4 X^2 < 7.3e18 < 2^63; size^2 L2 < 8.9e12.  tests/test_viz_cpu.py holds the int64
  test to Python's unbounded integers at those corners.
Paint, per pixel: base = background; every covering layer-0 primitive in ascending index sets base to its colour (the last one wins); top = base;
every covering layer-1 primitive in ascending index sets top; per channel out = (top alpha + base (256 - alpha) + 128) >> 8 with alpha in
0 .. 256, one value per call.  A pixel no overlay primitive covers comes out as base exactly ((256 c + 128) >> 8 = c).
The statement has no pixel box in it.  `accelerate=True` and the kernel visit only a box per primitive, the endpoints +- size clipped to the
image: a superset of the covered pixels, since coverage implies a distance of at most size from a or b or the segment between them.
"""
import binascii
import struct
import zlib

import numpy as np

from . import render

MAX_SIZE = 64              # AG_DRAW_MAX_SIZE
MAX_COORD = 16383          # AG_DRAW_MAX_COORD
DISC, SEGMENT = 0, 1
OPAQUE, OVERLAY = 0, 1

# the reference's colours, restated by value.  rgb_colormap(repeat=100) (src/dynamics/utils.py:139-145): point k is blue, green, red by k // 100
COLORMAP = (0x0000FF, 0x00FF00, 0xFF0000)
RED, GREEN = 0xFF0000, 0x00FF00
# visualize_img's four colours, read as RGB
COLOR_START, COLOR_ACTION, COLOR_PRED, COLOR_TARGET = ((202 << 16) | (63 << 8) | 41, (27 << 16) | (74 << 8) | 242, (237 << 16) | (158 << 8) | 49,
                                                       (26 << 16) | (130 << 8) | 81)
# OURS: the sphere splat's colours (the reference shows its simulator's rendering there)
PALETTE = (0xD8C39A, 0xC9B287, 0xE3D0AB, 0xBDA578)
TABLE_COLOR, VOID_COLOR = 0x6E6E73, 0x000000
FRAME_BUDGET = 64 * 720 * 1280 * 8      # bytes of images per launch: 64 frames of 720 x 1 280, 4 bytes out and (depth and id shared by a pair) 4 more each


def frames_per_launch(H, W, budget=FRAME_BUDGET):
    """How many frames of H x W one launch draws under the byte budget: an even number (a pred and a gt frame share a background), at least 2."""
    return max(2, int(budget) // (int(H) * int(W) * 8) // 2 * 2)


# ---------------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------------
def project_host(pts, cam, near):
    """pts (n, 3) float32, cam one row of render.camera_rows -> x, y (n,) int64 and valid (n,) bool (module text)."""
    R, t = cam[9:18].reshape(3, 3), cam[18:21]
    fx, fy, cx, cy = cam[21:]
    with np.errstate(all="ignore"):
        d = np.asarray(pts, np.float32).astype(np.float64) - t[None, :]
        c = [(R[0, r] * d[:, 0] + R[1, r] * d[:, 1]) + R[2, r] * d[:, 2] for r in range(3)]
        x = np.trunc(fx * (c[0] / c[2]) + cx)
        y = np.trunc(fy * (c[1] / c[2]) + cy)
        valid = (c[2] > near) & (np.abs(x) <= MAX_COORD) & (np.abs(y) <= MAX_COORD)      # (a NaN or an infinity fails the comparison)
    return np.where(valid, x, 0).astype(np.int64), np.where(valid, y, 0).astype(np.int64), valid


def coverage(kind, size, ax, ay, bx, by, u, v):
    """The pixels (u, v) (int64 arrays) a primitive covers (module text) -> bool array."""
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    ax, ay, bx, by, ww = np.int64(ax), np.int64(ay), np.int64(bx), np.int64(by), np.int64(size) * np.int64(size)
    qx, qy = u - ax, v - ay
    if kind == DISC:
        return qx * qx + qy * qy <= ww
    dx, dy = bx - ax, by - ay
    L2 = dx * dx + dy * dy
    s = qx * dx + qy * dy
    X = qx * dy - qy * dx
    rx, ry = u - bx, v - by
    cap_a = np.int64(4) * (qx * qx + qy * qy) <= ww
    cap_b = np.int64(4) * (rx * rx + ry * ry) <= ww
    body = np.int64(4) * (X * X) <= ww * L2
    return np.where((L2 == 0) | (s < 0), cap_a, np.where(s > L2, cap_b, body))


def _colour_planes(bg_mode, bg, palette, color0, color1, index, H, W):
    """The background of one frame as (H, W) int32 0xRRGGBB."""
    flat = np.full((H, W), np.int32(int(color0) & 0xFFFFFF), np.int32)
    if bg_mode == 0 or not 0 <= index < len(bg):
        return flat
    if bg_mode == 1:
        img = np.asarray(bg[index]).astype(np.int32)
        return (img[..., 0] << 16) | (img[..., 1] << 8) | img[..., 2]
    ids = np.asarray(bg[index], np.int32)
    pal = np.asarray(palette, np.int32)
    return np.where(ids >= 0, pal[ids % len(pal)], np.where(ids == -1, np.int32(int(color0)), np.int32(int(color1)))) & 0xFFFFFF


def _check_tables(pts, prims, styles, frames, cams, H, W, alpha, bg_mode, bg, palette):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    prims, styles, frames = (np.ascontiguousarray(a, np.int32).reshape(-1, 4) for a in (prims, styles, frames))
    cams = np.ascontiguousarray(cams, np.float64)
    if cams.ndim != 2 or cams.shape[1] != 25 or len(cams) < 1 or len(frames) < 1:
        raise ValueError("draw: cams is (C, 25) = render.camera_rows with C >= 1, frames (F, 4) with F >= 1")
    if not (1 <= int(H) <= render.MAX_SIDE and 1 <= int(W) <= render.MAX_SIDE):
        raise ValueError(f"draw: H, W outside 1 .. {render.MAX_SIDE}")
    if not 0 <= int(alpha) <= 256:
        raise ValueError("draw: alpha outside 0 .. 256")
    if bg_mode not in (0, 1, 2):
        raise ValueError("draw: background mode outside 0 .. 2")
    if bg_mode != 0:
        want = (int(H), int(W), 4) if bg_mode == 1 else (int(H), int(W))
        if bg is None or len(bg) < 1 or tuple(bg.shape[1:]) != want:
            raise ValueError(f"draw: background mode {bg_mode} needs images of shape (n_bg >= 1, {', '.join(map(str, want))})")
        if bg_mode == 2 and (palette is None or len(palette) < 1):
            raise ValueError("draw: background mode 2 needs a palette")
    return pts, prims, styles, frames, cams


def draw_host(pts, prims, styles, frames, cams, H, W, alpha=256, bg_mode=0, bg=None, palette=None, color0=0, color1=0, near=0.05,
              accelerate=True):
    """The statement (module text) -> out (F, H, W, 4) uint8.  `accelerate=True` visits only each primitive's pixel box, False every pixel for
    every primitive: the same array."""
    pts, prims, styles, frames, cams = _check_tables(pts, prims, styles, frames, cams, H, W, alpha, bg_mode, bg, palette)
    H, W, alpha, near = int(H), int(W), int(alpha), float(near)
    n_pts, n_prim, n_style, C = len(pts), len(prims), len(styles), len(cams)
    out = np.empty((len(frames), H, W, 4), np.uint8)
    proj = {}
    for f, (cam, first, count, index) in enumerate(frames.tolist()):
        base = _colour_planes(bg_mode, bg, palette, color0, color1, index, H, W).copy()
        lo, hi = max(first, 0), min(first + count, n_prim)
        if not 0 <= cam < C or count < 0:
            hi = lo
        if hi > lo and cam not in proj:
            proj[cam] = project_host(pts, cams[cam], near)
        listed = ([], [])      # per layer: (box, kind, size, a, b, colour) in ascending index
        for i in range(lo, hi):
            pa, pb, st = (int(z) for z in prims[i, :3])
            if not (0 <= pa < n_pts and 0 <= pb < n_pts and 0 <= st < n_style):
                continue
            kind, size, layer, colour = (int(z) for z in styles[st])
            if kind not in (DISC, SEGMENT) or not 0 <= size <= MAX_SIZE or layer not in (OPAQUE, OVERLAY):
                continue
            x, y, valid = proj[cam]
            if kind == DISC:
                pb = pa
            if not (valid[pa] and valid[pb]):
                continue
            listed[layer].append((kind, size, int(x[pa]), int(y[pa]), int(x[pb]), int(y[pb]), colour & 0xFFFFFF))
        top = None
        for layer in (OPAQUE, OVERLAY):
            if layer == OVERLAY:
                top = base.copy()
            plane = base if layer == OPAQUE else top
            for kind, size, ax, ay, bx, by, colour in listed[layer]:
                u0, u1, v0, v1 = 0, W, 0, H
                if accelerate:
                    u0, u1 = min(max(min(ax, bx) - size, 0), W), min(max(max(ax, bx) + size + 1, 0), W)
                    v0, v1 = min(max(min(ay, by) - size, 0), H), min(max(max(ay, by) + size + 1, 0), H)
                    if u1 <= u0 or v1 <= v0:
                        continue
                hit = coverage(kind, size, ax, ay, bx, by, np.arange(u0, u1, dtype=np.int64)[None, :], np.arange(v0, v1, dtype=np.int64)[:, None])
                plane[v0:v1, u0:u1] = np.where(hit, np.int32(colour), plane[v0:v1, u0:u1])
        for ch, shift in enumerate((16, 8, 0)):
            out[f, :, :, ch] = ((((top >> shift) & 0xFF) * alpha + ((base >> shift) & 0xFF) * (256 - alpha) + 128) >> 8).astype(np.uint8)
        out[f, :, :, 3] = 255
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the device path
# ---------------------------------------------------------------------------------------------------------------------
class DeviceCanvas:
    """The cameras of ag_draw as a device tensor, and the output images and the projection scratch preallocated for up to F frames and max_pts
    points: `launch(...)` enqueues the two kernels on the current stream (no synchronisation, no allocation: it captures into a HIP graph) and
    returns out[:F'] (F', H, W, 4) uint8, which the next launch overwrites.  The tables are contiguous device tensors of the statement's types."""

    def __init__(self, cams, H, W, F=1, max_pts=4096, near=0.05, device="cuda:0"):
        import ctypes

        import torch
        from . import _lib
        self.device = torch.device(device)
        cams = np.ascontiguousarray(cams, np.float64)
        if cams.ndim != 2 or cams.shape[1] != 25 or len(cams) < 1:
            raise ValueError("DeviceCanvas: cams is (C, 25) = render.camera_rows, C >= 1")
        if not (1 <= int(H) <= render.MAX_SIDE and 1 <= int(W) <= render.MAX_SIDE) or int(F) < 1:
            raise ValueError(f"DeviceCanvas: H, W outside 1 .. {render.MAX_SIDE} or F < 1")
        self.C, self.H, self.W, self.F, self.max_pts = len(cams), int(H), int(W), int(F), max(int(max_pts), 1)
        self.cams = torch.from_numpy(cams).to(self.device)
        self.near = ctypes.c_double(float(near))
        self.scratch_bytes = int(_lib.lib().ag_draw_scratch_bytes(self.max_pts, self.C))
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=self.device)
        self.out = torch.empty((self.F, self.H, self.W, 4), dtype=torch.uint8, device=self.device)
        self._none_f = torch.zeros(4, dtype=torch.float32, device=self.device)      # stands in for an empty table: a non-null pointer
        self._none_i = torch.zeros(4, dtype=torch.int32, device=self.device)

    def launch(self, pts, prims, styles, frames, alpha=256, bg_mode=0, bg=None, palette=None, color0=0, color1=0):
        import ctypes

        import torch
        from . import _lib
        for name, x, dt, last in (("pts", pts, torch.float32, 3), ("prims", prims, torch.int32, 4), ("styles", styles, torch.int32, 4),
                                  ("frames", frames, torch.int32, 4)):
            if x.device != self.device or x.dtype != dt or x.dim() != 2 or x.shape[1] != last or not x.is_contiguous():
                raise ValueError(f"DeviceCanvas: {name} must be a contiguous {dt} tensor of shape (n, {last}) on {self.device}")
        F = int(frames.shape[0])
        if not 1 <= F <= self.F or int(pts.shape[0]) > self.max_pts:
            raise ValueError(f"DeviceCanvas: {F} frames, {int(pts.shape[0])} points; built for 1 .. {self.F} frames and {self.max_pts} points")
        n_bg = n_pal = 0
        if bg_mode in (1, 2):
            want = (self.H, self.W, 4) if bg_mode == 1 else (self.H, self.W)
            dt = torch.uint8 if bg_mode == 1 else torch.int32
            if bg is None or bg.device != self.device or bg.dtype != dt or tuple(bg.shape[1:]) != want or not bg.is_contiguous() or bg.shape[0] < 1:
                raise ValueError(f"DeviceCanvas: background mode {bg_mode} needs a contiguous {dt} tensor (n_bg >= 1, {want}) on {self.device}")
            n_bg = int(bg.shape[0])
            if bg_mode == 2:
                if palette is None or palette.device != self.device or palette.dtype != torch.int32 or palette.dim() != 1 or not palette.is_contiguous():
                    raise ValueError("DeviceCanvas: background mode 2 needs a contiguous int32 palette on the device")
                n_pal = int(palette.shape[0])
        some = lambda x, none: x if x.numel() else none
        _lib.call("ag_draw", self.device, some(pts, self._none_f), int(pts.shape[0]), some(prims, self._none_i), int(prims.shape[0]),
                  some(styles, self._none_i), int(styles.shape[0]), frames, F, self.cams, self.C, ctypes.byref(self.near), self.H, self.W, int(alpha),
                  int(bg_mode), bg if bg_mode else None, n_bg, palette if bg_mode == 2 else None, n_pal, int(color0) & 0xFFFFFF,
                  int(color1) & 0xFFFFFF, self.scratch, self.scratch_bytes, self.out)
        return self.out[:F]


def draw(pts, prims, styles, frames, cams, H, W, alpha=256, bg_mode=0, bg=None, palette=None, color0=0, color1=0, near=0.05, device=None):
    """draw_host on the GPU: the same arguments (arrays or tensors), the same array bit for bit, as a tensor on `device`.  device=None runs the
    host statement and returns numpy."""
    if device is None:
        host = lambda a: a.detach().cpu().numpy() if type(a).__module__.startswith("torch") else a
        return draw_host(host(pts), host(prims), host(styles), host(frames), host(cams), H, W, alpha, bg_mode, None if bg is None else host(bg),
                         None if palette is None else host(palette), color0, color1, near)
    import torch
    device = torch.device(device)

    def up(a, np_dt, dt, last=None):
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(a, np_dt))
        a = a.to(device=device, dtype=dt)
        return (a.reshape(-1, last) if last else a).contiguous()

    cams = cams.detach().cpu().numpy() if isinstance(cams, torch.Tensor) else cams
    pts, prims, styles, frames = up(pts, np.float32, torch.float32, 3), up(prims, np.int32, torch.int32, 4), up(styles, np.int32, torch.int32, 4), up(
        frames, np.int32, torch.int32, 4)
    canvas = DeviceCanvas(cams, H, W, max(int(frames.shape[0]), 1), int(pts.shape[0]), near, device)
    if bg_mode == 1:
        bg = up(bg, np.uint8, torch.uint8)
    elif bg_mode == 2:
        bg, palette = up(bg, np.int32, torch.int32), up(palette, np.int32, torch.int32)
    return canvas.launch(pts, prims, styles, frames, alpha, bg_mode, bg, palette, color0, color1)


# ---------------------------------------------------------------------------------------------------------------------
# display lists
# ---------------------------------------------------------------------------------------------------------------------
class DrawList:
    """A display list under construction: numpy arrays with device=None, tensors on `device` otherwise (what is given is moved there).  Every
    method is array indexing -- no Python loop over particles or edges -- and none reads a device value on the host: the numbers of points and
    primitives are shapes.  `tables()` -> pts, prims, styles, frames for draw / draw_host / DeviceCanvas.launch."""

    def __init__(self, device=None):
        self.device = device
        if device is not None:
            import torch
            self.device = torch.device(device)
        self._pts, self._prims, self.styles, self.frames = [], [], [], []
        self.n_pts = self.n_prim = 0
        self._open = None

    # ---- array helpers: one spelling for numpy and torch
    def _f32(self, a):
        if self.device is None:
            a = a.detach().cpu().numpy() if type(a).__module__.startswith("torch") else a
            return np.asarray(a, np.float32).reshape(-1, 3)
        import torch
        a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, np.float32))
        return a.to(device=self.device, dtype=torch.float32).reshape(-1, 3)

    def _i32(self, a, n=None):
        """An index array (or one integer, repeated n times) as int32 of this list's kind."""
        if self.device is None:
            a = a.detach().cpu().numpy() if type(a).__module__.startswith("torch") else a
            a = np.asarray(a, np.int32).reshape(-1)
            return np.full(n, a[0], np.int32) if n is not None and a.size == 1 and n != 1 else a
        import torch
        a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a).reshape(-1), np.int32))
        a = a.to(device=self.device, dtype=torch.int32).reshape(-1)
        return a.expand(n).contiguous() if n is not None and a.numel() == 1 and n != 1 else a

    def _arange(self, n):
        if self.device is None:
            return np.arange(n, dtype=np.int32)
        import torch
        return torch.arange(n, dtype=torch.int32, device=self.device)

    def _stack(self, cols):
        if self.device is None:
            return np.stack(cols, 1).astype(np.int32)
        import torch
        return torch.stack(cols, 1).to(torch.int32)

    # ---- the tables
    def style(self, kind, size, layer, colour):
        """The index of the style (kind, size, layer, colour), added if new."""
        row = (int(kind), int(size), int(layer), int(colour) & 0xFFFFFF)
        if row not in self.styles:
            self.styles.append(row)
        return self.styles.index(row)

    def add_points(self, points):
        """points (..., 3) in the cameras' world frame -> the index of the first."""
        p = self._f32(points)
        first = self.n_pts
        self._pts.append(p)
        self.n_pts += int(p.shape[0])
        return first

    def add_prims(self, a, b, style):
        """Primitives a[k] -> b[k] (global point indices) of style[k] (or one style for all)."""
        a, b = self._i32(a), self._i32(b)
        n = int(a.shape[0])
        self._prims.append(self._stack([a, b, self._i32(style, n), self._arange(n) * 0]))
        self.n_prim += n

    def begin_frame(self, camera=0, background=0):
        """What is added from here on belongs to a new frame (the one before is closed)."""
        self.end_frame()
        self._open = (int(camera), self.n_prim, int(background))

    def end_frame(self):
        if self._open is not None:
            cam, first, bgi = self._open
            self.frames.append((cam, first, self.n_prim - first, bgi))
            self._open = None

    def add_discs(self, points, style):
        """One disc per point; `style` one index or one per point."""
        first = self.add_points(points)
        idx = self._arange(self.n_pts - first) + first
        self.add_prims(idx, idx, style)
        return first

    def add_segments(self, points_a, points_b, style):
        """One segment per pair of points."""
        fa = self.add_points(points_a)
        n = self.n_pts - fa
        fb = self.add_points(points_b)
        if self.n_pts - fb != n:
            raise ValueError("DrawList.add_segments: as many starts as ends")
        self.add_prims(self._arange(n) + fa, self._arange(n) + fb, style)
        return fa

    def add_edges(self, point_offset, recv, send, style, tool_style=None, max_nobj=None, *, tool_offset=None, sample=None):
        """One segment per edge between the points point_offset + recv[k] and point_offset + send[k] (local node indices; the nodes' points were
        added before, node i at point_offset + i, or -- with `tool_offset` -- node i >= max_nobj at tool_offset + i - max_nobj).  With
        `tool_style` an edge with an end >= max_nobj takes that style (graph.py:136-154).
        `recv` may be a graph.CSREdges and `send` None: the edges of its sample `sample`, taken WITHOUT a host read -- e_cap // B primitives,
        those past the sample's count with point index -1, which draw drops."""
        if send is None:
            import torch
            csr, b = recv, int(sample)
            cap = csr.e_cap // max(csr.B, 1)
            rp = csr.row_ptr.long()
            e = rp[b * csr.N] + torch.arange(cap, device=rp.device)
            ok = e < rp[(b + 1) * csr.N]
            e = e.clamp(max=max(int(csr.edge_recv.shape[0]) - 1, 0))
            recv = torch.where(ok, csr.edge_recv[e].long() - b * csr.N, torch.full_like(e, -1))
            send = torch.where(ok, csr.edge_send[e].long() - b * csr.N, torch.full_like(e, -1))
        recv, send = self._i32(recv), self._i32(send)
        n = int(recv.shape[0])
        st = self._i32(style, n)
        as_i32 = (lambda m: m.astype(np.int32)) if self.device is None else (lambda m: m.to(st.dtype))
        if tool_style is not None:
            st = st + as_i32((recv >= int(max_nobj)) | (send >= int(max_nobj))) * (int(tool_style) - int(style))
        neg = (recv < 0) | (send < 0)
        off = int(point_offset)
        jump = 0 if tool_offset is None else int(tool_offset) - int(max_nobj) - off      # what a tool node's point lies past off + i
        a, b2 = recv + off + as_i32(recv >= int(max_nobj or 0)) * jump, send + off + as_i32(send >= int(max_nobj or 0)) * jump
        if self.device is None:
            a, b2 = np.where(neg, -1, a), np.where(neg, -1, b2)
        else:
            import torch
            a, b2 = torch.where(neg, torch.full_like(a, -1), a), torch.where(neg, torch.full_like(b2, -1), b2)
        self.add_prims(a, b2, st)

    def add_arrows(self, start, end, style, tip=0.5, normal=(0.0, 0.0, 1.0)):
        """One arrow per (start, end) pair of world points: the shaft start -> end and two head strokes from `end`, the reversed shaft turned by
        +-45 degrees about `normal` (the board's normal) and scaled to tip |arrow|, computed in world space in float32 (Rodrigues' formula for
        a unit normal perpendicular or not: v cos + (n x v) sin + n (n.v)(1 - cos))."""
        s, e = self._f32(start), self._f32(end)
        n = np.asarray(normal, np.float64)
        n = (n / np.linalg.norm(n)).astype(np.float32)
        cs = np.float32(np.sqrt(0.5))
        back = (s - e) * np.float32(tip) if self.device is None else (s - e) * float(np.float32(tip))
        if self.device is None:
            nv = np.broadcast_to(n, back.shape)
            cross = np.cross(nv, back).astype(np.float32)
            along = nv * (back @ n)[:, None] * np.float32(1.0 - cs)
        else:
            import torch
            nt = torch.from_numpy(n).to(self.device)
            nv = nt.expand_as(back)
            cross = torch.cross(nv, back, dim=1)
            along = nv * (back @ nt)[:, None] * float(np.float32(1.0 - cs))
        heads = [e + (back * float(cs) + cross * float(sign * cs) + along) for sign in (1.0, -1.0)]
        self.add_segments(s, e, style)
        self.add_segments(e, heads[0], style)
        self.add_segments(e, heads[1], style)

    def tables(self):
        """-> pts (n_pts, 3) float32, prims (n_prim, 4) int32, styles (n_style, 4) int32, frames (F, 4) int32."""
        self.end_frame()
        styles = np.asarray(self.styles, np.int32).reshape(-1, 4)
        frames = np.asarray(self.frames, np.int32).reshape(-1, 4)
        if self.device is None:
            pts = np.concatenate(self._pts, 0) if self._pts else np.zeros((0, 3), np.float32)
            prims = np.concatenate(self._prims, 0) if self._prims else np.zeros((0, 4), np.int32)
            return pts, prims, styles, frames
        import torch
        pts = torch.cat(self._pts, 0) if self._pts else torch.zeros((0, 3), dtype=torch.float32, device=self.device)
        prims = torch.cat(self._prims, 0) if self._prims else torch.zeros((0, 4), dtype=torch.int32, device=self.device)
        return pts.contiguous(), prims.contiguous(), torch.from_numpy(styles).to(self.device), torch.from_numpy(frames).to(self.device)


def _board(points, sim_real_ratio):
    from .sim_env import to_board_frame
    return points if sim_real_ratio is None else to_board_frame(points, sim_real_ratio)


def rollout_frames(pred, gt, eef, edges, n_kp, max_nobj, sim_real_ratio=None, *, camera=0, backgrounds=None, lengths=None, t_line=5,
                   point_size=4, edge_size=1, line_size=2, device=None):
    """The display lists of `visualize_graph` (graph.py:44-230) for every step of every rollout of a batch -> DrawList with frames in the order
    (b, t, pred), (b, t, gt); draw them with alpha = 128 (line_alpha 0.5).
    pred, gt (B, T, max_nobj, 3): the model's and the recorded key points that frame t shows, eef (B, T, n_eef, 3) the tool in it, edges[b][t]
    its graph: the caller keeps them at ONE time (the evaluation rollout: the state step t's forward reads, all at the step's start frame); arrays or tensors, in simulator units when `sim_real_ratio` is given (they go through sim_env.to_board_frame), otherwise already in the
    cameras' frame.  edges[b][t]: (recv, send) local node indices of step t's graph (tool nodes from max_nobj on), or (a graph.CSREdges, its sample).
    n_kp (B,) ints: the rollout's key points; lengths (B,): its steps (default T); backgrounds (B, T) ints: the frame's background index.
    A pred frame: key point k a disc of radius 4 in COLORMAP[k // 100], tool points red discs of radius 3, object edges green and tool edges
    red of width 1, and as the overlay the motion of the last t_line steps, key point k from step t' - 1 to t', t' = max(1, t - t_line + 1)
    .. t, width 2.  A gt frame: the same with the recorded key points (tool radius 4).  The loops are over rollouts and steps only.
    `dl.spans[b]` is the range of points rollout b uses, so that a batch of frames can be drawn with its own rollouts' points alone."""
    dl = DrawList(device)
    dl.spans = []
    B, T = int(pred.shape[0]), int(pred.shape[1])
    kp_styles = [dl.style(DISC, point_size, OPAQUE, c) for c in COLORMAP]
    trail_styles = [dl.style(SEGMENT, line_size, OVERLAY, c) for c in COLORMAP]
    tool_pred, tool_gt = dl.style(DISC, 3, OPAQUE, RED), dl.style(DISC, point_size, OPAQUE, RED)
    edge_obj, edge_tool = dl.style(SEGMENT, edge_size, OPAQUE, GREEN), dl.style(SEGMENT, edge_size, OPAQUE, RED)
    n_eef = int(eef.shape[2])
    for b in range(B):
        steps = T if lengths is None else int(lengths[b])
        k = int(n_kp[b])
        which = np.minimum(np.arange(k) // 100, len(COLORMAP) - 1)
        kp_st, tr_st = np.asarray(kp_styles, np.int32)[which], np.asarray(trail_styles, np.int32)[which]
        first = {"pred": dl.add_points(_board(pred[b, :steps], sim_real_ratio)), "gt": dl.add_points(_board(gt[b, :steps], sim_real_ratio))}
        tool0 = dl.add_points(_board(eef[b, :steps], sim_real_ratio))
        dl.spans.append((first["pred"], dl.n_pts))
        ks = np.arange(k, dtype=np.int32)
        for t in range(steps):
            for name in ("pred", "gt"):
                dl.begin_frame(camera, 0 if backgrounds is None else int(backgrounds[b][t]))
                here = first[name] + t * max_nobj
                dl.add_prims(ks + here, ks + here, kp_st)
                tools = dl._arange(n_eef) + (tool0 + t * n_eef)
                dl.add_prims(tools, tools, tool_pred if name == "pred" else tool_gt)
                if edges is not None and edges[b][t] is not None:
                    r, s = edges[b][t]
                    csr = hasattr(r, "row_ptr")
                    dl.add_edges(here, r, None if csr else s, edge_obj, edge_tool, max_nobj, tool_offset=tool0 + t * n_eef, sample=s if csr else None)
                t0 = max(1, t - t_line + 1)
                if t >= t0 and k:
                    tt = np.repeat(np.arange(t0, t + 1, dtype=np.int32), k)
                    kk = np.tile(ks, t + 1 - t0)
                    dl.add_prims(first[name] + tt * max_nobj + kk, first[name] + (tt - 1) * max_nobj + kk, np.tile(tr_st, t + 1 - t0))
    return dl


def planning_frame(state_init, state_pred, action, repeat, edges_init, edges_pred, sim_real_ratio, *, target_state=None, target_box=None,
                   state_after=None, edges_after=None, camera=0, background=0, device=None):
    """The display list of `visualize_img` (plan_utils.py:104-300) -> DrawList with one frame; draw it with alpha = 128.
    state_init (n, 3), state_pred (n, 3), target_state (m, 3): simulator units; action the decoded (x_start, z_start, x_end, z_end) of one
    repeat, `repeat` how many; edges_*: (recv, send) of the state's graph, or (a graph.CSREdges, its sample); target_box ((x_min, x_max), (z_min, z_max)).
    Opaque: the start state (state_after with its edges instead, for the `_1` image) as discs of radius 5 and its edges of width 2 in
    COLOR_START, one arrow of width 2 per repeat in COLOR_ACTION at the start state's mean height.  Overlay: the target cloud as discs (or the
    target box as an outline of width 2: ours, the reference fills four thin rectangles) in COLOR_TARGET, then the predicted state and its
    edges in COLOR_PRED."""
    dl = DrawList(device)
    dl.begin_frame(camera, background)
    start, start_edges = (state_init, edges_init) if state_after is None else (state_after, edges_after)
    p_start, e_start = dl.style(DISC, 5, OPAQUE, COLOR_START), dl.style(SEGMENT, 2, OPAQUE, COLOR_START)
    arrow = dl.style(SEGMENT, 2, OPAQUE, COLOR_ACTION)
    p_target, e_target = dl.style(DISC, 5, OVERLAY, COLOR_TARGET), dl.style(SEGMENT, 2, OVERLAY, COLOR_TARGET)
    p_pred, e_pred = dl.style(DISC, 5, OVERLAY, COLOR_PRED), dl.style(SEGMENT, 2, OVERLAY, COLOR_PRED)
    def add_edges(first, edges, style):      # (recv, send), or (a graph.CSREdges, its sample)
        if edges is not None:
            csr = hasattr(edges[0], "row_ptr")
            dl.add_edges(first, edges[0], None if csr else edges[1], style, sample=edges[1] if csr else None)

    first = dl.add_discs(_board(_host(start), sim_real_ratio), p_start)
    add_edges(first, start_edges, e_start)
    xs, zs, xe, ze = (float(a) for a in np.asarray(_host(action), np.float64).reshape(-1)[:4])
    y = float(np.asarray(_host(state_init), np.float32)[:, 1].mean())
    i = np.arange(int(repeat), dtype=np.float64)
    a0 = np.stack([xs + i * (xe - xs), np.full_like(i, y), zs + i * (ze - zs)], 1).astype(np.float32)
    a1 = np.stack([xe + i * (xe - xs), np.full_like(i, y), ze + i * (ze - zs)], 1).astype(np.float32)
    if int(repeat) > 0:
        dl.add_arrows(_board(a0, sim_real_ratio), _board(a1, sim_real_ratio), arrow)
    if target_state is not None:
        dl.add_discs(_board(_host(target_state), sim_real_ratio), p_target)
    if target_box is not None:
        (x0, x1), (z0, z1) = np.asarray(_host(target_box), np.float64).reshape(2, 2)
        corners = np.array([[x0, 0, z0], [x1, 0, z0], [x1, 0, z1], [x0, 0, z1]], np.float32)
        dl.add_segments(_board(corners, sim_real_ratio), _board(np.roll(corners, -1, 0), sim_real_ratio), e_target)
    add_edges(dl.add_discs(_board(_host(state_pred), sim_real_ratio), p_pred), edges_pred, e_pred)
    return dl


def radius_edges_host(state, adj_thresh, topk):
    """The object-object edges of graph.py:38-89 for points without a tool, in numpy, for a picture: receiver i, sender j iff |x_i - x_j|^2 <
    adj_thresh^2 and j is among the topk nearest of i (self-edges included, as there; ties by index).  -> recv, send int32."""
    x = np.asarray(state, np.float32)
    dis = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    near = np.zeros_like(dis, bool)
    k = min(int(topk), len(x))
    if k:
        np.put_along_axis(near, np.argsort(dis, 1, kind="stable")[:, :k], True, 1)
    recv, send = np.nonzero((dis < np.float32(adj_thresh) ** 2) & near)
    return recv.astype(np.int32), send.astype(np.int32)


def planning_image(env, state_init, state_pred, action, *, target_state=None, target_box=None, state_after=None, camera=0):
    """One image of the closed loop (plan_utils.py:104-300 as plan.py:262-283 calls it) -> (H, W, 4) uint8, numpy or a tensor on the
    environment's device (a view of the environment's canvas, which the next image overwrites): planning_frame over the environment's own
    render (the id image of camera `camera` from its last observation, `env.last_ids`, else `env.render()`; background mode 2) at alpha = 128.  `action` is the planner's (x_start, z_start, theta, repeat); the edges are those of the task's adj_thresh and topk: ag_build_edges
    on the device, read from its CSR without a host read, radius_edges_host otherwise."""
    task = env.task_config
    act = np.asarray(_host(action), np.float64).reshape(-1)
    step = (act[0], act[1], act[0] - task["push_length"] * np.cos(act[2]), act[1] - task["push_length"] * np.sin(act[2]))
    device = getattr(env, "device", None)

    def edges_of(state):
        if state is None:
            return None
        if device is None:
            return radius_edges_host(_host(state), task["adj_thresh"], task["topk"])
        import torch
        from .graph import build_edges
        x = (state if isinstance(state, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(state, np.float32))).to(device).float()[None]
        n = x.shape[1]
        return build_edges(x, task["adj_thresh"], torch.ones((1, n), dtype=torch.bool, device=device),
                           torch.zeros((1, n), dtype=torch.bool, device=device), task["topk"], task.get("connect_tools_all", False), "single",
                           max_tools=1), 0

    dl = planning_frame(state_init, state_pred, step, int(act[3]), edges_of(state_init), edges_of(state_pred), env.ratio, target_state=target_state,
                        target_box=target_box, state_after=state_after, edges_after=edges_of(state_after), camera=camera, background=camera,
                        device=device)
    ids = getattr(env, "last_ids", None)      # the observation the loop has just made, where the environment keeps it (SimEnv does)
    if ids is None:
        ids = env.render()[1]
    tables = dl.tables()
    if device is None:
        return draw_host(*tables, render.camera_rows(env.R_list, env.t_list, env.intr_list), env.H, env.W, 128, 2, ids, PALETTE, TABLE_COLOR,
                         VOID_COLOR, env.near)[0]
    import torch
    kept = getattr(env, "_plan_canvas", None)      # one canvas and one palette per environment, grown only if a list outgrows it
    if kept is None or kept[0].max_pts < dl.n_pts:
        kept = (DeviceCanvas(render.camera_rows(env.R_list, env.t_list, env.intr_list), env.H, env.W, 1, max(dl.n_pts, 4096), env.near, device),
                torch.tensor(PALETTE, dtype=torch.int32, device=device))
        env._plan_canvas = kept
    return kept[0].launch(*tables, 128, 2, ids.contiguous(), kept[1], TABLE_COLOR, VOID_COLOR)[0]


def write_rollout_record(dirs, schedules, pred, gt, eef, edges, n_kp, max_nobj, particles, material, device=None, radius=None, H=720, W=1280,
                         camera=0, batch=None, video=False, fmt="png"):
    """Every step of every rollout of a batch as {start:06}_{end:06}_{pred,gt,both}.png in dirs[b] (graph.py:163-225's names with png for jpg;
    `both` is pred | gt side by side).  fmt="jpg": the reference's own names, baseline JPEG files (jpeg.py) -- on the device encoded from the
    drawn frames where they are (`both` from the device-side concatenation), so that only the compressed bytes are copied to the host.
    `video`: every directory drawn into also gets pred.avi, gt.avi and both.avi, Motion-JPEG at 10 fps of its frames in file-name order
    (rollout.py:197-203); the encoded frames are kept in host memory until the last chunk is drawn.
    schedules[b] = [(start, end)] per step; pred, gt (B, T, max_nobj, 3), eef (B, T, n_eef, 3) and edges as rollout_frames takes them, all at frame `start`; edges[t] a graph.CSREdges of the whole batch at step t; particles[b][t] (n, 3): the
    recorded particles of frame `start`, the background (a sphere splat from camera `camera` of render.default_cameras, the reference's
    cam = 0, where the reference shows the recorded camera image).  Everything is in simulator units and goes to the board frame with the
    task's sim_real_ratio; `radius` is the particles' (default: the material's simulator default `r`; the pile's is per scene, 0.1 here).
    Frames are rendered and drawn `batch` at a time (default: frames_per_launch(H, W), the byte budget) -- one ag_render_depth and one
    ag_draw call, one copy to the host -- never one per launch; a launch gets the points and primitives of its own rollouts alone.
    device=None: the host statements.  -> the paths written."""
    import os

    from . import configs, jpeg, sim_env
    if fmt not in ("png", "jpg"):
        raise ValueError('write_rollout_record: fmt is "png" or "jpg"')
    coded, reels = video or fmt == "jpg", {}
    ratio = float(configs.task_config(material)["sim_real_ratio"])
    if radius is None:
        radius = getattr(sim_env.SIMULATORS[material][0], "r", 0.1)
    lengths = [len(s) for s in schedules]
    steps = [(b, t) for b, n in enumerate(lengths) for t in range(n)]
    order = {bt: j for j, bt in enumerate(steps)}
    B, T = len(schedules), max(lengths)
    dl = rollout_frames(pred, gt, eef, None if edges is None else [[(edges[t], b) for t in range(lengths[b])] for b in range(B)], n_kp, max_nobj,
                        ratio, camera=0, backgrounds=[[order.get((b, t), 0) for t in range(T)] for b in range(B)], lengths=lengths, device=device)
    pts, prims, styles, _ = dl.tables()
    cam = [[x[camera]] for x in render.default_cameras(ratio, H, W)]
    cams = render.camera_rows(*cam)
    per = max(int(frames_per_launch(H, W) if batch is None else batch) // 2, 1)      # steps per launch: a pred and a gt frame each
    per = min(per, len(steps))
    n_max = max(max(len(p) for row in particles for p in row), 1)
    rr = np.full(per, np.float32(radius) * np.float32(1.0 / ratio), np.float32)
    chunks = [steps[j0:j0 + per] for j0 in range(0, len(steps), per)]
    spans = [(dl.spans[c[0][0]][0], dl.spans[c[-1][0]][1]) for c in chunks]      # the points of the rollouts a chunk touches
    if device is not None:
        import torch
        renderer = render.DeviceRenderer(*cam, H, W, (0.0, 0.0, 1.0, 0.0), E=per, device=device)
        canvas = DeviceCanvas(cams, H, W, 2 * per, max(hi - lo for lo, hi in spans), device=device)
        palette, rr_dev = torch.tensor(PALETTE, dtype=torch.int32, device=device), torch.from_numpy(rr).to(device)
        if coded:
            encoders = (jpeg.DeviceEncoder(H, W, min(2 * per, jpeg.frames_per_launch(H, W)), device=device),
                        jpeg.DeviceEncoder(H, 2 * W, min(per, jpeg.frames_per_launch(H, 2 * W)), device=device))
    written = []
    for k, chunk in enumerate(chunks):
        j0, (lo, hi) = k * per, spans[k]
        scene, n = np.zeros((per, n_max, 3), np.float32), np.zeros(per, np.int32)
        for e, (b, t) in enumerate(chunk):
            n[e] = len(particles[b][t])
            scene[e, :n[e]] = sim_env.to_board_frame(np.asarray(particles[b][t], np.float32), ratio)
        # the chunk's frames over its own slice of the tables: primitives p0 .. p1, points lo .. hi (an index of -1 stays negative: still dropped)
        mine = dl.frames[2 * j0:2 * (j0 + len(chunk))]
        p0, p1 = mine[0][1], mine[-1][1] + mine[-1][2]
        fr = np.array([[c, first - p0, count, bg - j0] for c, first, count, bg in mine], np.int32)
        shift = np.array([lo, lo, 0, 0], np.int32)
        if device is None:
            ids = render.render_depth_host(scene, n, rr, *cam, H, W, (0.0, 0.0, 1.0, 0.0))[1][:, 0]
            images = draw_host(pts[lo:hi], prims[p0:p1] - shift, styles, fr, cams, H, W, 128, 2, ids, PALETTE, TABLE_COLOR, VOID_COLOR)
            if coded:
                both = np.concatenate([images[0::2], images[1::2]], 2)
                files = jpeg.encode_jpeg(images), jpeg.encode_jpeg(both)
        else:
            ids = renderer.launch(torch.from_numpy(scene).to(device), torch.from_numpy(n).to(device), rr_dev)[1][:, 0]
            images = canvas.launch(pts[lo:hi].contiguous(), (prims[p0:p1] - torch.from_numpy(shift).to(device)).contiguous(), styles,
                                   torch.from_numpy(fr).to(device), 128, 2, ids.contiguous(), palette, TABLE_COLOR, VOID_COLOR)
            if coded:      # where the frames are: pred and gt as drawn, `both` their concatenation on the device
                files = encoders[0].encode(images), encoders[1].encode(torch.cat([images[0::2], images[1::2]], 2).contiguous())
            if fmt == "png":
                images = images.cpu().numpy()
        for e, (b, t) in enumerate(chunk):
            start, end = schedules[b][t]
            stem = os.path.join(dirs[b], f"{int(start):06}_{int(end):06}")
            for name in ("pred", "gt", "both"):
                data = None if not coded else files[1][e] if name == "both" else files[0][2 * e + (name == "gt")]
                if fmt == "png":
                    write_png(f"{stem}_{name}.png", np.concatenate([images[2 * e], images[2 * e + 1]], 1) if name == "both" else
                              images[2 * e + (name == "gt")])
                else:
                    with open(f"{stem}_{name}.jpg", "wb") as fh:
                        fh.write(data)
                written.append(f"{stem}_{name}.{fmt}")
                if video:
                    reels.setdefault((dirs[b], name), []).append((os.path.basename(stem), data))
    for (d, name), frames in reels.items():      # a directory's frames in file-name order, whichever rollouts they came from
        with jpeg.VideoWriter(os.path.join(d, f"{name}.avi"), H, 2 * W if name == "both" else W, 10) as out:
            out.add([data for _, data in sorted(frames, key=lambda x: x[0])])
        written.append(os.path.join(d, f"{name}.avi"))
    return written


def _host(a):
    return a.detach().cpu().numpy() if type(a).__module__.startswith("torch") else np.asarray(a)


# ---------------------------------------------------------------------------------------------------------------------
# PNG files: 8-bit RGB, filter 0, from the standard library alone.  (JPEG files and Motion-JPEG videos: jpeg.py.)
# ---------------------------------------------------------------------------------------------------------------------
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", binascii.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path, image, level=6):
    """image (H, W, 3) or (H, W, 4) uint8 (array or tensor; an alpha channel is not written) -> an 8-bit RGB PNG, every row with filter 0."""
    img = np.ascontiguousarray(_host(image))
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] not in (3, 4) or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("write_png: an (H, W, 3) or (H, W, 4) uint8 image")
    H, W = img.shape[:2]
    rows = np.zeros((H, 1 + 3 * W), np.uint8)
    rows[:, 1:] = img[:, :, :3].reshape(H, 3 * W)
    with open(path, "wb") as fh:
        fh.write(_PNG_MAGIC + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level))
                 + _chunk(b"IEND", b""))


def read_png(path):
    """A file of write_png -> (H, W, 3) uint8.  Reads 8-bit RGB, no interlace, filter 0 on every row; anything else raises."""
    data = open(path, "rb").read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError("read_png: not a PNG file")
    at, idat, head = 8, b"", None
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        if struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] != binascii.crc32(kind + body) & 0xFFFFFFFF:
            raise ValueError("read_png: checksum")
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        at += 12 + n
    if head is None or head[2:] != (8, 2, 0, 0, 0):
        raise ValueError("read_png: only 8-bit RGB without interlace")
    W, H = head[:2]
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 3 * W)
    if rows[:, 0].any():
        raise ValueError("read_png: only filter 0")
    return rows[:, 1:].reshape(H, W, 3).copy()
