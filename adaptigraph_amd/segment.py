"""Object masks from colour images: the stage between a camera's colour image and the `keep_masks` argument of perception.state_from_depth.

The reference gets instance masks from GroundingDINO and SAM and then does something small and classical with them
(src/planning/perception.py:176-209): it joins the masks labelled "table" / "sheet" and the masks of the objects, forms mask_table & ~mask_obj and
keeps every pixel that is NOT table.  This module builds that last stage without a learned model: pixels are classified by colour keys in integer
HSV, the binary mask is cleaned (square morphology, small-blob removal, hole filling), its connected components are labelled, and the
reference's keep rule is formed.  Not here: a learned model, text prompts, a mapping from instances to p_instance, watershed / grab-cut, the tool
in view (the robot retracts before it observes), sensor noise.

The numpy functions `*_host` are the statement of the arithmetic -- integers only, so "equal" means np.array_equal -- and csrc/ag_segment.hip
repeats it on the device (`DeviceSegmenter`, or the thin functions with `device="cuda:0"`).  Images are (C, H, W, 3 | 4) uint8 (the alpha byte is
ignored), masks (C, H, W) bool / uint8 (non-zero = set), labels (C, H, W) int32; a single (H, W[, ch]) image is taken as C = 1 and returned so.

Conventions, each the one of scipy.ndimage (tests/test_segment_cpu.py holds them to it where scipy imports):
  morphology   the (2r + 1) x (2r + 1) square, pixels outside the image are background for every operation (binary_erosion / _dilation / _opening /
               _closing with border_value=0), r = 0 the identity;
  labels       0 the background, the components of one image numbered 1 .. count in ascending order of their lowest row-major pixel index
               (ndimage.label for both connectivities), restarting in every image;
  holes        the background components, under the dual connectivity, that do not touch the image border (binary_fill_holes for connectivity 8).
"""
import dataclasses

import numpy as np

TILE_H, TILE_W = 16, 64      # the labelling kernel's tile (AG_SEGMENT_TILE_H, _W): the tests size their images from these
MAX_RADIUS = 8               # AG_SEGMENT_MAX_RADIUS
MAX_KEYS = 8                 # AG_SEGMENT_MAX_KEYS
MAX_KEEP = 8                 # AG_SEGMENT_MAX_KEEP
OPS = {"erode": 0, "dilate": 1, "opening": 2, "closing": 3}      # AG_SEGMENT_ERODE .. _CLOSE


# ---------------------------------------------------------------------------------------------------------------------
# argument checks shared by both paths
# ---------------------------------------------------------------------------------------------------------------------
def _is_tensor(a):
    return type(a).__module__.startswith("torch")


def _check_images(images):
    if _is_tensor(images):
        import torch
        ok = images.dtype == torch.uint8
    else:
        images = np.asarray(images)
        ok = images.dtype == np.uint8
    if not ok or images.ndim not in (3, 4) or images.shape[-1] not in (3, 4) or 0 in images.shape:
        raise ValueError("segment: images must be (C, H, W, 3 | 4) or (H, W, 3 | 4) uint8")
    return images


def _check_mask(mask):
    if _is_tensor(mask):
        import torch
        ok = mask.dtype in (torch.bool, torch.uint8)
    else:
        mask = np.asarray(mask)
        ok = mask.dtype in (np.bool_, np.uint8)
    if not ok or mask.ndim not in (2, 3) or 0 in mask.shape:
        raise ValueError("segment: a mask must be (C, H, W) or (H, W) bool / uint8")
    return mask


def _check_radius(r):
    if int(r) != r or not 0 <= int(r) <= MAX_RADIUS:
        raise ValueError(f"segment: radius {r!r} outside 0 .. {MAX_RADIUS} (MAX_RADIUS)")
    return int(r)


def _check_connectivity(connectivity):
    if connectivity not in (4, 8):
        raise ValueError(f"segment: connectivity must be 4 or 8; got {connectivity!r}")
    return int(connectivity)


def _check_select(min_area, keep_largest):
    if keep_largest is not None and (int(keep_largest) != keep_largest or not 1 <= int(keep_largest) <= MAX_KEEP):
        raise ValueError(f"segment: keep_largest {keep_largest!r} outside 1 .. {MAX_KEEP}")
    return int(min_area), (0 if keep_largest is None else int(keep_largest))


def _check_keys(keys):
    keys = [keys] if isinstance(keys, ColorKey) else list(keys)
    if len(keys) > MAX_KEYS or not all(isinstance(k, ColorKey) for k in keys):
        raise ValueError(f"segment: at most {MAX_KEYS} ColorKey per mask")
    return keys


# ---------------------------------------------------------------------------------------------------------------------
# a. colour keys
# ---------------------------------------------------------------------------------------------------------------------
def hsv_host(rgb):
    """(..., 3 | 4) integers 0 .. 255 -> (..., 3) int32 H 0 .. 359, S 0 .. 255, V 0 .. 255, integers only.  With mx, mn the channel maximum and
    minimum and d = mx - mn: V = mx; S = 0 if mx == 0 else (255 d + mx // 2) // mx; H = 0 if d == 0, else by the maximum channel, r before g
    before b: (60 (g - b) + d // 2) // d mod 360, (60 (b - r) + d // 2) // d + 120 mod 360, (60 (r - g) + d // 2) // d + 240 mod 360.  `//` floors
    (toward minus infinity), which matters: (60 (20 - 200) + 95) // 190 is -57 and C's truncation gives -56."""
    c = np.asarray(rgb).astype(np.int32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    d = mx - mn
    s = np.where(mx == 0, 0, (255 * d + mx // 2) // np.maximum(mx, 1))
    dd = np.maximum(d, 1)
    h = np.where(mx == r, ((60 * (g - b) + d // 2) // dd) % 360,
                 np.where(mx == g, ((60 * (b - r) + d // 2) // dd + 120) % 360, ((60 * (r - g) + d // 2) // dd + 240) % 360))
    h = np.where(d == 0, 0, h)
    return np.stack([h, s, mx], -1).astype(np.int32)


@dataclasses.dataclass(frozen=True)
class ColorKey:
    """An inclusive box in hsv_host's space.  h_lo > h_hi: the hue interval wraps through 359 -> 0."""
    h_lo: int = 0
    h_hi: int = 359
    s_lo: int = 0
    s_hi: int = 255
    v_lo: int = 0
    v_hi: int = 255

    @classmethod
    def exact(cls, rgb_int):
        """The degenerate box of one colour 0xRRGGBB (or an (r, g, b) triple)."""
        rgb = ((rgb_int >> 16) & 255, (rgb_int >> 8) & 255, rgb_int & 255) if isinstance(rgb_int, (int, np.integer)) else tuple(rgb_int)
        h, s, v = (int(z) for z in hsv_host(np.array(rgb, np.int32)))
        return cls(h, h, s, s, v, v)

    def row(self):
        return [int(self.h_lo), int(self.h_hi), int(self.s_lo), int(self.s_hi), int(self.v_lo), int(self.v_hi)]


def color_mask_host(images, keys):
    """images (C, H, W, 3 | 4) uint8, up to MAX_KEYS keys -> (C, H, W) bool: the pixel lies in any key's box."""
    images, keys = np.asarray(_check_images(images)), _check_keys(keys)
    hsv = hsv_host(images)
    h, s, v = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    out = np.zeros(images.shape[:-1], bool)
    for k in keys:
        hue = ((h >= k.h_lo) & (h <= k.h_hi)) if k.h_lo <= k.h_hi else ((h >= k.h_lo) | (h <= k.h_hi))
        out |= hue & (s >= k.s_lo) & (s <= k.s_hi) & (v >= k.v_lo) & (v <= k.v_hi)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# b. morphology
# ---------------------------------------------------------------------------------------------------------------------
def _pass(m, r, axis, dilate):
    """One pass of the separable square along `axis` of (C, H, W) bool: OR (dilate) or AND (erode) of the 2r + 1 shifts, outside = False."""
    n = m.shape[axis]
    pad = [(0, 0)] * 3
    pad[axis] = (r, r)
    p = np.pad(m, pad)
    out = np.zeros_like(m) if dilate else np.ones_like(m)
    for k in range(2 * r + 1):
        piece = np.take(p, np.arange(k, k + n), axis)
        out = (out | piece) if dilate else (out & piece)
    return out


def _as3(mask):
    m = np.asarray(_check_mask(mask)) != 0
    return (m[None], True) if m.ndim == 2 else (m, False)


def _morph_host(mask, r, steps):
    m, single = _as3(mask)
    r = _check_radius(r)
    for dilate in steps:
        m = _pass(_pass(m, r, 2, dilate), r, 1, dilate)
    return m[0] if single else m


def erode_host(mask, r):
    return _morph_host(mask, r, (False,))


def dilate_host(mask, r):
    return _morph_host(mask, r, (True,))


def opening_host(mask, r):
    return _morph_host(mask, r, (False, True))


def closing_host(mask, r):
    return _morph_host(mask, r, (True, False))


# ---------------------------------------------------------------------------------------------------------------------
# c. labelling
# ---------------------------------------------------------------------------------------------------------------------
def _label_one(m, conn8):
    """(H, W) bool -> labels (H, W) int32, count.  Row runs in raster order, a union-find over the runs (the lower run number is the root), the
    runs of neighbouring rows joined where they touch: columns overlap, or for 8-connectivity differ by one.  A run's number orders it by its
    first pixel, so a component's root is the run that holds its lowest pixel index and the roots, in order, are 1 .. count."""
    H, W = m.shape
    d = np.diff(np.pad(m.astype(np.int8), ((0, 0), (1, 1))), axis=1)
    ys, starts = np.nonzero(d == 1)
    ends = np.nonzero(d == -1)[1]      # one past the run's last pixel
    n = len(ys)
    labels = np.zeros((H, W), np.int32)
    if n == 0:
        return labels, 0
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    first = np.searchsorted(ys, np.arange(H + 1))      # the runs of row y are first[y] .. first[y + 1]
    reach = 1 if conn8 else 0
    S, E = starts.tolist(), ends.tolist()
    for y in range(1, H):
        i, i_end, j, j_end = first[y - 1], first[y], first[y], first[y + 1]
        while i < i_end and j < j_end:
            if S[i] < E[j] + reach and S[j] < E[i] + reach:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
            if E[i] < E[j]:
                i += 1
            else:
                j += 1
    number, count = np.zeros(n, np.int32), 0
    for k in range(n):
        root = find(k)
        if root == k:
            count += 1
            number[k] = count
        else:
            number[k] = number[root]
    labels[m] = np.repeat(number, ends - starts)
    return labels, count


def label_host(mask, connectivity=8):
    """mask (C, H, W) -> labels (C, H, W) int32, count (C,) int32."""
    m, single = _as3(mask)
    conn8 = _check_connectivity(connectivity) == 8
    out = [_label_one(x, conn8) for x in m]
    labels, count = np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32)
    return (labels[0], count) if single else (labels, count)


# ---------------------------------------------------------------------------------------------------------------------
# d. the component table
# ---------------------------------------------------------------------------------------------------------------------
def components_host(labels, count, max_labels):
    """labels (C, H, W) int32, count (C,) -> table (C, max_labels, 8) int64 rows [area, x_min, y_min, x_max, y_max, sum_x, sum_y, touches_border]
    of labels 1 .. min(count, max_labels), the other rows zero; and count, unchanged, so that a caller sees a truncation."""
    labels = np.asarray(labels)
    single = labels.ndim == 2
    lab = labels[None] if single else labels
    count = np.asarray(count, np.int32).reshape(-1)
    if lab.ndim != 3 or lab.dtype != np.int32 or len(count) != len(lab) or int(max_labels) < 1:
        raise ValueError("segment: labels (C, H, W) int32, count (C,), max_labels >= 1")
    C, H, W = lab.shape
    table = np.zeros((C, int(max_labels), 8), np.int64)
    for c in range(C):
        n = min(int(count[c]), int(max_labels))
        ys, xs = np.nonzero((lab[c] >= 1) & (lab[c] <= n))
        k = lab[c][ys, xs].astype(np.int64) - 1
        t = table[c]
        t[:n, 1], t[:n, 2] = np.iinfo(np.int64).max, np.iinfo(np.int64).max
        np.add.at(t[:, 0], k, 1)
        np.minimum.at(t[:, 1], k, xs)
        np.minimum.at(t[:, 2], k, ys)
        np.maximum.at(t[:, 3], k, xs)
        np.maximum.at(t[:, 4], k, ys)
        np.add.at(t[:, 5], k, xs)
        np.add.at(t[:, 6], k, ys)
        np.maximum.at(t[:, 7], k, ((ys == 0) | (ys == H - 1) | (xs == 0) | (xs == W - 1)).astype(np.int64))
    return (table[0] if single else table), count.copy()


# ---------------------------------------------------------------------------------------------------------------------
# e. selection and holes
# ---------------------------------------------------------------------------------------------------------------------
def select_host(mask, min_area=0, keep_largest=None, connectivity=8):
    """Keeps the components with at least min_area pixels; with keep_largest = k (1 .. MAX_KEEP) of those only the k largest, equal areas ordered
    by the lower label.  Any number of components."""
    m, single = _as3(mask)
    min_area, k = _check_select(min_area, keep_largest)
    labels, count = label_host(m, connectivity)
    out = np.zeros_like(m)
    for c in range(len(m)):
        area = np.bincount(labels[c].ravel(), minlength=int(count[c]) + 1)
        ok = area >= min_area
        ok[0] = False
        if k:
            order = sorted(np.nonzero(ok)[0].tolist(), key=lambda l: (-int(area[l]), l))
            ok[:] = False
            ok[order[:k]] = True
        out[c] = ok[labels[c]]
    return out[0] if single else out


def fill_holes_host(mask, connectivity=8):
    """Adds every background component that does not touch the image border; the background under the dual connectivity (4 for 8, 8 for 4)."""
    m, single = _as3(mask)
    dual = 4 if _check_connectivity(connectivity) == 8 else 8
    labels, count = label_host(~m, dual)
    out = m.copy()
    for c in range(len(m)):
        L = labels[c]
        edge = np.concatenate([L[0], L[-1], L[:, 0], L[:, -1]])
        hole = np.ones(int(count[c]) + 1, bool)
        hole[edge] = False
        hole[0] = False
        out[c] |= hole[L]
    return out[0] if single else out


# ---------------------------------------------------------------------------------------------------------------------
# f. the keep rule
# ---------------------------------------------------------------------------------------------------------------------
def _chain_host(images, keys, open_radius, close_radius, min_area, keep_largest, connectivity):
    m = color_mask_host(images, keys)
    if open_radius:
        m = opening_host(m, open_radius)
    if close_radius:
        m = closing_host(m, close_radius)
    if min_area > 0 or keep_largest is not None:
        m = select_host(m, min_area, keep_largest, connectivity)
    return m


def _check_keep(open_radius, close_radius, min_area, keep_largest, connectivity):
    _check_radius(open_radius), _check_radius(close_radius), _check_select(min_area, keep_largest), _check_connectivity(connectivity)


def keep_mask_host(images, table_keys, object_keys=None, *, open_radius=0, close_radius=0, min_area=0, keep_largest=None, fill=False,
                   connectivity=8):
    """perception.py:203-209 over colour keys: table = color_mask(images, table_keys), opened, closed, selected; objects = the same chain for
    object_keys, plus fill_holes if `fill` (all False without object_keys); -> ~(table & ~objects), (C, H, W) bool."""
    images = np.asarray(_check_images(images))
    _check_keep(open_radius, close_radius, min_area, keep_largest, connectivity)
    single = images.ndim == 3
    img = images[None] if single else images
    table = _chain_host(img, table_keys, open_radius, close_radius, min_area, keep_largest, connectivity)
    objects = np.zeros_like(table)
    if object_keys is not None:
        objects = _chain_host(img, object_keys, open_radius, close_radius, min_area, keep_largest, connectivity)
        if fill:
            objects = fill_holes_host(objects, connectivity)
    out = ~(table & ~objects)
    return out[0] if single else out


# ---------------------------------------------------------------------------------------------------------------------
# the device path
# ---------------------------------------------------------------------------------------------------------------------
class DeviceSegmenter:
    """The ag_segment_* calls with their scratch and their mask buffers preallocated for up to C images of up to H x W pixels (as DeviceRenderer,
    DeviceCanvas and DeviceEncoder do).  Every method enqueues on the current stream -- no synchronisation, no allocation beyond the returned
    tensors of `label` / `components`, nothing read back -- and takes contiguous tensors on the segmenter's device, smaller images included.
    `keep_mask` writes into the segmenter's own buffers and returns a view that the next call overwrites: it captures into a HIP graph."""

    def __init__(self, C, H, W, device="cuda:0"):
        import ctypes
        import torch
        from . import _lib
        self.device = torch.empty(0, device=device).device      # ("cuda" -> cuda:0: what the tensors of that device report)
        self.C, self.H, self.W = int(C), int(H), int(W)
        L = _lib.lib()
        th, tw = ctypes.c_int(), ctypes.c_int()
        L.ag_segment_tile_sizes(ctypes.byref(th), ctypes.byref(tw))
        if (th.value, tw.value) != (TILE_H, TILE_W):
            raise RuntimeError(f"segment: the library's tile is {th.value} x {tw.value}, this module says {TILE_H} x {TILE_W} (stale build?)")
        self.scratch_bytes = int(L.ag_segment_scratch_bytes(self.C, self.H, self.W))
        if self.C < 1 or self.H < 1 or self.W < 1 or self.scratch_bytes == 0:
            raise ValueError(f"DeviceSegmenter: {self.C} images of {self.H} x {self.W} are outside what one call takes")
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=self.device)
        self._masks = torch.empty((3, self.C * self.H * self.W), dtype=torch.uint8, device=self.device)

    # ---- checks
    def _shape(self, t, trailing=0):
        import torch
        if not isinstance(t, torch.Tensor) or t.device != self.device or not t.is_contiguous() or t.dim() != 3 + trailing:
            raise ValueError(f"DeviceSegmenter: a contiguous tensor of {3 + trailing} dimensions on {self.device} is needed")
        C, H, W = (int(z) for z in t.shape[:3])
        if not (1 <= C <= self.C and 1 <= H and 1 <= W and H * W <= self.H * self.W):
            raise ValueError(f"DeviceSegmenter: built for {self.C} x {self.H} x {self.W}; got {tuple(t.shape)}")
        return C, H, W

    def _mask(self, mask):
        import torch
        from . import _lib
        if not isinstance(mask, torch.Tensor):
            raise ValueError(f"DeviceSegmenter: a tensor on {self.device} is needed")
        return _lib._u8(_check_mask(mask))

    def _buf(self, i, C, H, W):
        return self._masks[i, :C * H * W].view(C, H, W)

    def _out(self, out, like):
        import torch
        return torch.empty(like.shape, dtype=torch.uint8, device=self.device) if out is None else out

    # ---- the stages
    def color_mask(self, images, keys, out=None):
        import ctypes
        from . import _lib
        images, keys = _check_images(images), _check_keys(keys)
        C, H, W = self._shape(images, 1)
        out = self._out(out, images[..., 0])
        rows = (ctypes.c_int32 * (6 * max(len(keys), 1)))(*[v for k in keys for v in k.row()])
        _lib.call("ag_segment_color_mask", self.device, images, C, H, W, int(images.shape[3]), rows, len(keys), out)
        return out

    def morph(self, op, mask, r, out=None):
        from . import _lib
        mask, r = self._mask(mask), _check_radius(r)
        C, H, W = self._shape(mask)
        out = self._out(out, mask)
        _lib.call("ag_segment_morph", self.device, mask, C, H, W, OPS[op], r, self.scratch, self.scratch_bytes, out)
        return out

    def label(self, mask, connectivity=8):
        import torch
        from . import _lib
        mask, connectivity = self._mask(mask), _check_connectivity(connectivity)
        C, H, W = self._shape(mask)
        labels = torch.empty((C, H, W), dtype=torch.int32, device=self.device)
        count = torch.empty(C, dtype=torch.int32, device=self.device)
        _lib.call("ag_segment_label", self.device, mask, C, H, W, connectivity, self.scratch, self.scratch_bytes, labels, count)
        return labels, count

    def components(self, labels, count, max_labels):
        import torch
        from . import _lib
        C, H, W = self._shape(labels)
        if labels.dtype != torch.int32 or count.dtype != torch.int32 or tuple(count.shape) != (C,) or count.device != self.device or int(max_labels) < 1:
            raise ValueError("DeviceSegmenter: labels (C, H, W) int32, count (C,) int32 on the device, max_labels >= 1")
        table = torch.empty((C, int(max_labels), 8), dtype=torch.int64, device=self.device)
        _lib.call("ag_segment_components", self.device, labels, count.contiguous(), C, H, W, int(max_labels), table)
        return table, count

    def select(self, mask, min_area=0, keep_largest=None, connectivity=8, out=None):
        from . import _lib
        mask, connectivity = self._mask(mask), _check_connectivity(connectivity)
        min_area, k = _check_select(min_area, keep_largest)
        C, H, W = self._shape(mask)
        out = self._out(out, mask)
        _lib.call("ag_segment_select", self.device, mask, C, H, W, connectivity, min_area, k, self.scratch, self.scratch_bytes, out)
        return out

    def fill_holes(self, mask, connectivity=8, out=None):
        from . import _lib
        mask, connectivity = self._mask(mask), _check_connectivity(connectivity)
        C, H, W = self._shape(mask)
        out = self._out(out, mask)
        _lib.call("ag_segment_fill_holes", self.device, mask, C, H, W, connectivity, self.scratch, self.scratch_bytes, out)
        return out

    def _chain(self, images, keys, buf, open_radius, close_radius, min_area, keep_largest, connectivity):
        """keep_mask_host's chain in `buf`: every stage after the colour keys runs in place (a call writes its output in its last launch, and
        that launch reads the input at the pixel's own index at most)."""
        m = self.color_mask(images, keys, out=buf)
        if open_radius:
            self.morph("opening", m, open_radius, out=m)
        if close_radius:
            self.morph("closing", m, close_radius, out=m)
        if min_area > 0 or keep_largest is not None:
            self.select(m, min_area, keep_largest, connectivity, out=m)
        return m

    def keep_mask(self, images, table_keys, object_keys=None, *, open_radius=0, close_radius=0, min_area=0, keep_largest=None, fill=False,
                  connectivity=8):
        """keep_mask_host on the device -> (C, H, W) bool, a view of the segmenter's buffer."""
        import torch
        from . import _lib
        images = _check_images(images)
        _check_keep(open_radius, close_radius, min_area, keep_largest, connectivity)
        C, H, W = self._shape(images, 1)
        table, objects, out = (self._buf(i, C, H, W) for i in range(3))
        self._chain(images, table_keys, table, open_radius, close_radius, min_area, keep_largest, connectivity)
        if object_keys is not None:
            self._chain(images, object_keys, objects, open_radius, close_radius, min_area, keep_largest, connectivity)
            if fill:
                self.fill_holes(objects, connectivity, out=objects)
        _lib.call("ag_segment_keep", self.device, table, objects if object_keys is not None else None, C, H, W, out)
        return out.view(torch.bool)


# ---------------------------------------------------------------------------------------------------------------------
# thin functions: device=None is the statement, otherwise one DeviceSegmenter built for the argument
# ---------------------------------------------------------------------------------------------------------------------
def _to_device(a, device, check):
    """-> the (C, ...) uint8 / bool tensor on `device`, and whether a leading axis was added."""
    import torch
    a = check(a)
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    single = t.dim() == (3 if check is _check_images else 2)
    t = t[None] if single else t
    return t.to(device).contiguous(), single


def _segmenter(t, device):
    return DeviceSegmenter(t.shape[0], t.shape[1], t.shape[2], device)


def color_mask(images, keys, device=None):
    if device is None:
        return color_mask_host(images, keys)
    import torch
    t, single = _to_device(images, device, _check_images)
    out = _segmenter(t, device).color_mask(t, keys).view(torch.bool)
    return out[0] if single else out


def _morph(op, host, mask, r, device):
    if device is None:
        return host(mask, r)
    import torch
    t, single = _to_device(mask, device, _check_mask)
    out = _segmenter(t, device).morph(op, t, r).view(torch.bool)
    return out[0] if single else out


def erode(mask, r, device=None):
    return _morph("erode", erode_host, mask, r, device)


def dilate(mask, r, device=None):
    return _morph("dilate", dilate_host, mask, r, device)


def opening(mask, r, device=None):
    return _morph("opening", opening_host, mask, r, device)


def closing(mask, r, device=None):
    return _morph("closing", closing_host, mask, r, device)


def label(mask, connectivity=8, device=None):
    """-> labels, count; on the device path both stay on the device."""
    if device is None:
        return label_host(mask, connectivity)
    t, single = _to_device(mask, device, _check_mask)
    labels, count = _segmenter(t, device).label(t, connectivity)
    return (labels[0], count) if single else (labels, count)


def components(labels, count, max_labels, device=None):
    """-> table (C, max_labels, 8) int64, count."""
    if device is None:
        return components_host(labels, count, max_labels)
    import torch
    lab = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(labels))
    single = lab.dim() == 2
    lab = (lab[None] if single else lab).to(device).contiguous()
    cnt = (count if isinstance(count, torch.Tensor) else torch.from_numpy(np.asarray(count, np.int32).reshape(-1))).to(device).reshape(-1)
    table, cnt = _segmenter(lab, device).components(lab, cnt, max_labels)
    return (table[0] if single else table), cnt


def select(mask, min_area=0, keep_largest=None, connectivity=8, device=None):
    if device is None:
        return select_host(mask, min_area, keep_largest, connectivity)
    import torch
    t, single = _to_device(mask, device, _check_mask)
    out = _segmenter(t, device).select(t, min_area, keep_largest, connectivity).view(torch.bool)
    return out[0] if single else out


def fill_holes(mask, connectivity=8, device=None):
    if device is None:
        return fill_holes_host(mask, connectivity)
    import torch
    t, single = _to_device(mask, device, _check_mask)
    out = _segmenter(t, device).fill_holes(t, connectivity).view(torch.bool)
    return out[0] if single else out


def keep_mask(images, table_keys, object_keys=None, *, open_radius=0, close_radius=0, min_area=0, keep_largest=None, fill=False, connectivity=8,
              device=None):
    """The keep rule on the path it is given -> (C, H, W) bool, ready for state_from_depth(..., keep_masks=list(mask))."""
    kw = dict(open_radius=open_radius, close_radius=close_radius, min_area=min_area, keep_largest=keep_largest, fill=fill, connectivity=connectivity)
    if device is None:
        return keep_mask_host(images, table_keys, object_keys, **kw)
    t, single = _to_device(images, device, _check_images)
    out = _segmenter(t, device).keep_mask(t, table_keys, object_keys, **kw).clone()
    return out[0] if single else out
