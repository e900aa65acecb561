"""The geometry between the cameras and `state_cur`: depth images -> tabletop cloud -> key points (src/planning/perception.py:151-256
`get_tabletop_points`, :318-349 `get_state_cur`), without the vision models: GroundingDINO and SAM only contribute a boolean keep-mask per
camera, and that mask is an input here.  What the reference does with the models' masks (:176-209, ~(mask_table & ~mask_obj)) is
`segment.keep_mask`, which makes the mask from a colour image by colour keys, morphology and connected components instead of a learned model;
`SimEnv(masks="color")` feeds it to this module.  Colours are not carried into the cloud (the reference uses them for drawing only).

The reference does this stage with numpy and open3d (`crop`, `voxel_down_sample`, `remove_statistical_outlier`).  open3d is not vendored and
was not available when this was written, so, as `sampling.py` does for DGL's sampler, the algorithm is RESTATED below as host code in numpy
float64, and parity is pinned to that statement, not to library outputs.  The following open3d details were written down from memory and
could NOT be checked against the library; someone with open3d at hand should check them:
  * `remove_statistical_outlier`: the query point counts among its own `nb_neighbors` neighbours; the deviation divides by `n - 1`; a point is
    kept iff `avg < threshold` (strict); points with `avg <= 0` are neither kept nor counted in the mean and the deviation (`> 0` tests),
    while the mean still divides by `n`;
  * `crop` with an axis-aligned box is inclusive on both sides;
  * `voxel_down_sample` puts the grid origin at `min_bound - 0.5 * voxel_size` and averages the members of a voxel.
  * open3d leaves the ORDER of the voxel output unspecified; here it is ascending lowest member index, because the farthest-point sampler that
    follows draws a start INDEX.

Two paths, one result.  numpy input (and `device=None`) runs the host code, which is the statement of the arithmetic.  With `device=` (or a
`DeviceCloud`) the HIP kernels of csrc/ag_tabletop.hip run; the cloud then stays on the device as a `(cap, 3)` fp32 tensor plus a device count
(`DeviceCloud`).  tests/test_tabletop_cloud.py holds the device path to the host path: the same kept pixels, the same voxels bit for bit, the
same neighbour means to 1e-14, the same keep decisions and iteration counts, the same key points under one `np.random.seed`.

The arithmetic, stage by stage (all of it float64 on float32 inputs, every product and sum rounded separately):
  depth_to_points   d = float32(depth[v, u]) at rows / columns 0, stride, ...; kept iff lo < d < hi (as doubles), the mask allows it and the
                    board-frame point lies in the box (inclusive); a = u d, b = v d; p_cam_r = (Kinv[r,0] a + Kinv[r,1] b) + Kinv[r,2] d;
                    p_r = ((R[r,0] p_cam_0 + R[r,1] p_cam_1) + R[r,2] p_cam_2) + t_r; stored as float32; camera-major, then row-major.
  voxel_down_sample origin = min - 0.5 voxel per axis; key = floor((p - origin) / voxel) (a division); one point per occupied voxel = the sum
                    of its members in ascending index / their number, as float32; ordered by lowest member index.
  statistical_outlier_mask  k = min(nb_neighbors, n) nearest under the total order (d2, j), self included, d2 = (dx dx + dy dy) + dz dz;
                    avg_i = (sum of sqrt(d2) in ascending neighbour order) / k; mean = (sum of the avg_i > 0) / n; std = sqrt((sum over
                    avg_i > 0 of (avg_i - mean)^2) / (n - 1)); threshold = mean + std_ratio std; keep_i = 0 < avg_i < threshold; n <= 1 keeps
                    nothing.  The cloud-wide sums run in a fixed order on either path (numpy's pairwise sum on the host, a fixed tree on the
                    device): the same bits on every call; the two trees differ in the last bits of the threshold, not in a decision that is
                    not an exact tie.
  denoise           iteration r uses std_ratio = 1.5 + 0.5 r; stops after the first iteration that removes nothing, or on an empty cloud.
  height_filter     k_filter >= 1: unchanged; else the points with z < sorted(z)[int(k_filter n)], in order.
"""
import numpy as np

VOXEL_SIZE = 0.0005                 # perception.py:230
MAX_POINTS = 1 << 20                # AG_TABLETOP_MAX_POINTS: the device path refuses larger clouds
MAX_NEIGHBORS = 20                  # AG_TABLETOP_MAX_NEIGHBORS: the neighbour kernels keep this many candidates per point in registers
VOXEL_KEY_LIMIT = 1 << 21           # AG_TABLETOP_VOXEL_KEY_LIMIT: voxel keys per axis the 64-bit sort key holds


# ---------------------------------------------------------------------------------------------------------------------
# host path: the statement of the arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def _f32_cloud(points):
    p = np.asarray(points)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"a cloud is (n, 3); got {p.shape}")
    return np.ascontiguousarray(p, np.float32)


def _box(bbox):
    b = np.asarray(bbox, np.float64)
    if b.shape != (3, 2):
        raise ValueError(f"bbox is (3, 2): [min, max] per axis (perception.py:227); got {b.shape}")
    return b


def _camera_rows(R_list, t_list, intr_list):
    """(C, 21) float64: Kinv (row-major), R (row-major), t per camera; Kinv = np.linalg.inv(intr), computed here on the host."""
    rows = []
    for R, t, K in zip(R_list, t_list, intr_list):
        Kinv = np.linalg.inv(np.asarray(K, np.float64).reshape(3, 3))
        rows.append(np.concatenate([Kinv.reshape(9), np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)]))
    return np.stack(rows) if rows else np.zeros((0, 21))


def depth_to_points_host(depth_list, R_list, t_list, intr_list, bbox, keep_masks=None, stride=4, depth_threshold=(0, 2), return_pixels=False):
    """-> (n, 3) float32 [, (n, 3) int64 (camera, v, u) of every kept pixel]."""
    box = _box(bbox)
    lo, hi = float(depth_threshold[0]), float(depth_threshold[1])
    cams = _camera_rows(R_list, t_list, intr_list)
    out, pix = [np.zeros((0, 3), np.float32)], [np.zeros((0, 3), np.int64)]
    for c, depth in enumerate(depth_list):
        d32 = np.asarray(depth).astype(np.float32)[::stride, ::stride]
        d = d32.astype(np.float64)
        v = (np.arange(d.shape[0], dtype=np.float64) * stride)[:, None]
        u = (np.arange(d.shape[1], dtype=np.float64) * stride)[None, :]
        Kinv, R, t = cams[c, :9].reshape(3, 3), cams[c, 9:18].reshape(3, 3), cams[c, 18:]
        with np.errstate(invalid="ignore", over="ignore"):
            a, b = u * d, v * d
            pc = [(Kinv[r, 0] * a + Kinv[r, 1] * b) + Kinv[r, 2] * d for r in range(3)]
            p = [((R[r, 0] * pc[0] + R[r, 1] * pc[1]) + R[r, 2] * pc[2]) + t[r] for r in range(3)]
            keep = (d > lo) & (d < hi)
            if keep_masks is not None:
                keep &= np.asarray(keep_masks[c]).astype(bool)[::stride, ::stride]
            for r in range(3):
                keep &= (p[r] >= box[r, 0]) & (p[r] <= box[r, 1])
            vi, ui = np.nonzero(keep)                       # row-major
            out.append(np.stack([p[r][vi, ui] for r in range(3)], 1).astype(np.float32))
        pix.append(np.stack([np.full(len(vi), c, np.int64), vi * stride, ui * stride], 1))
    pts = np.concatenate(out, 0)
    return (pts, np.concatenate(pix, 0)) if return_pixels else pts


def voxel_keys_host(points, voxel_size):
    """(n, 3) int64 voxel keys of a float32 cloud: floor((p - origin) / voxel), origin = min - 0.5 voxel, in float64."""
    p = _f32_cloud(points).astype(np.float64)
    voxel = float(voxel_size)
    origin = p.min(0) - 0.5 * voxel
    return np.floor((p - origin) / voxel).astype(np.int64)


def voxel_down_sample_host(points, voxel_size):
    p32 = _f32_cloud(points)
    if len(p32) == 0:
        return p32
    keys = voxel_keys_host(p32, voxel_size)
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(first, kind="stable")                # voxels by lowest member index
    rank = np.empty(len(first), np.int64)
    rank[order] = np.arange(len(first))
    slot = rank[inverse]
    sums = np.zeros((len(first), 3))
    np.add.at(sums, slot, p32.astype(np.float64))           # unbuffered: members are added in ascending input index
    return (sums / np.bincount(slot, minlength=len(first))[:, None]).astype(np.float32)


def _d2_rows(q, p):
    dx, dy, dz = q[:, None, 0] - p[None, :, 0], q[:, None, 1] - p[None, :, 1], q[:, None, 2] - p[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def _avg_of_sorted(d2_sorted, k):
    r = np.sqrt(d2_sorted[:, :k])
    a = np.zeros(len(r))
    for c in range(k):                                      # ascending neighbour order
        a = a + r[:, c]
    return a / k


def _knn_mean_brute(p, rows, k):
    n = len(p)
    avg = np.empty(len(rows))
    chunk = max(1, (1 << 22) // max(n, 1))
    for s in range(0, len(rows), chunk):
        d2 = _d2_rows(p[rows[s:s + chunk]], p)
        d2.sort(axis=1, kind="stable")                      # the values of the k smallest do not depend on how ties are ordered
        avg[s:s + chunk] = _avg_of_sorted(d2, k)
    return avg


def knn_mean_host(points, nb_neighbors=20, accelerate=True):
    """avg_i of the contract, float64 (n,).  The statement is the O(n^2) scan (`accelerate=False`).  Above 4 096 points, and when scipy
    imports, a k-d tree proposes k + 4 candidates per point; their distances are recomputed by the contract, and every point whose k-th
    distance is not clearly below the last candidate's is redone by the scan, so the values are those of the scan."""
    p = _f32_cloud(points).astype(np.float64)
    n = len(p)
    if n == 0:
        return np.zeros(0)
    k = min(int(nb_neighbors), n)
    if k < 1:
        raise ValueError("nb_neighbors must be >= 1")
    tree = None
    if accelerate and n > 4096:
        try:
            from scipy.spatial import cKDTree
            tree = cKDTree(p)
        except ImportError:
            tree = None
    if tree is None:
        return _knn_mean_brute(p, np.arange(n), k)
    kq = min(n, k + 4)
    dist, idx = tree.query(p, k=kq)
    d = p[:, None, :] - p[idx]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    d2s = np.sort(d2, axis=1, kind="stable")
    avg = _avg_of_sorted(d2s, k)
    unsure = np.nonzero(~(d2s[:, k - 1] < dist[:, -1] ** 2 * (1 - 1e-12)))[0] if kq < n else np.zeros(0, np.int64)
    if len(unsure):
        avg[unsure] = _knn_mean_brute(p, unsure, k)
    return avg


def outlier_threshold_host(avg, n, std_ratio):
    """(mean, std, threshold) of the contract from the neighbour means."""
    pos = avg[avg > 0]
    mean = pos.sum() / n
    std = np.sqrt(((pos - mean) ** 2).sum() / (n - 1))
    return mean, std, mean + float(std_ratio) * std


def statistical_outlier_mask_host(points, nb_neighbors=20, std_ratio=2.0):
    p = _f32_cloud(points)
    n = len(p)
    if n <= 1:
        return np.zeros(n, bool), knn_mean_host(p, nb_neighbors), np.float64(0.0)
    avg = knn_mean_host(p, nb_neighbors)
    _, _, threshold = outlier_threshold_host(avg, n, std_ratio)
    return (avg > 0) & (avg < threshold), avg, np.float64(threshold)


def denoise_host(points, nb_neighbors=20, max_iter=64, return_indices=False):
    p = _f32_cloud(points)
    alive = np.arange(len(p))
    it = 0
    while it < max_iter and len(p):
        keep, _, _ = statistical_outlier_mask_host(p, nb_neighbors, 1.5 + 0.5 * it)
        it += 1
        removed = len(p) - int(keep.sum())
        p, alive = p[keep], alive[keep]
        if removed == 0:
            break
    return (p, it, alive) if return_indices else (p, it)


def height_filter_host(points, k_filter):
    p = _f32_cloud(points)
    if k_filter >= 1.0 or len(p) == 0:
        return p
    z = p[:, 2]
    return p[z < np.sort(z)[int(k_filter * len(z))]]


def to_sim_frame(points, sim_real_ratio):
    """perception.py:335-337: x sim_real_ratio in float32, then (x, y, z) -> (x, -z, y).  numpy array or torch tensor."""
    q = points * np.float32(sim_real_ratio) if isinstance(points, np.ndarray) else points * float(np.float32(sim_real_ratio))
    if isinstance(points, np.ndarray):
        return np.stack([q[:, 0], -q[:, 2], q[:, 1]], 1)
    import torch
    return torch.stack([q[:, 0], -q[:, 2], q[:, 1]], 1)


# ---------------------------------------------------------------------------------------------------------------------
# device path: csrc/ag_tabletop.hip through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
class DeviceCloud:
    """A cloud on the GPU: `pts` (cap, 3) fp32, the first `count[0]` rows valid (`count` (1,) int32 on the device).  `n` is the count where the
    host already knows it (None otherwise); `bound` >= count is what launches are sized by."""
    __slots__ = ("pts", "count", "n")

    def __init__(self, pts, count, n=None):
        self.pts, self.count, self.n = pts, count, n

    @property
    def bound(self):
        return int(self.pts.shape[0]) if self.n is None else self.n

    def size(self):
        """The number of points; reads the 4-byte count back unless the host knows it."""
        if self.n is None:
            self.n = int(self.count.item())
        return self.n

    def tensor(self):
        return self.pts[:self.size()]

    def numpy(self):
        return self.tensor().cpu().numpy()


def _torch():
    import torch
    return torch


def to_device_cloud(points, device=None):
    """numpy (n, 3) / a GPU tensor (n, 3) / a DeviceCloud -> DeviceCloud."""
    if isinstance(points, DeviceCloud):
        return points
    torch = _torch()
    if isinstance(points, torch.Tensor):
        from . import _lib
        _lib._require_gpu(points, "points")
        if points.dtype != torch.float32:
            raise TypeError(f"the cloud kernels take float32 points; got {points.dtype}")
        pts = points.contiguous()
    else:
        if device is None:
            raise ValueError("a host cloud needs `device=`")
        pts = torch.from_numpy(_f32_cloud(points)).to(device)
    n = int(pts.shape[0])
    if n > MAX_POINTS:
        raise ValueError(f"the device path takes clouds of up to {MAX_POINTS} points; got {n}")
    if n == 0:
        pts = torch.zeros((1, 3), dtype=torch.float32, device=pts.device)
    return DeviceCloud(pts, torch.tensor([n], dtype=torch.int32).to(pts.device), n)


def _on_device(x, device):
    return device is not None or isinstance(x, DeviceCloud) or (type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False))


def _scratch(dev, bound):
    from . import _lib
    nbytes = _lib.lib().ag_tabletop_workspace_bytes(int(bound))
    if nbytes == 0:
        raise ValueError(f"the device path takes clouds of up to {MAX_POINTS} points; got {bound}")
    return _lib.workspace(dev, nbytes), nbytes


def depth_to_points_device(depth_list, R_list, t_list, intr_list, bbox, keep_masks, stride, depth_threshold, device):
    torch = _torch()
    from . import _lib
    dev = torch.device(device)
    shapes = {tuple(np.shape(d)) for d in depth_list}
    if len(shapes) != 1 or len(next(iter(shapes))) != 2:
        raise ValueError(f"the device path takes cameras of one (H, W) shape; got {sorted(shapes)}")
    def image(x, np_dtype, torch_dtype):      # a host array or a tensor -> a tensor of that type on the device
        if isinstance(x, torch.Tensor):
            return x.to(device=dev, dtype=torch_dtype)
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(np_dtype))).to(dev)

    depth = torch.stack([image(d, np.float32, torch.float32) for d in depth_list]).contiguous()
    C, H, W = (int(s) for s in depth.shape)
    mask = None
    if keep_masks is not None:
        mask = torch.stack([image(m, bool, torch.bool) for m in keep_masks]).contiguous().view(torch.uint8)
        if mask.shape != depth.shape:
            raise ValueError(f"keep_masks are {tuple(mask.shape)}, the depth images {tuple(depth.shape)}")
    cams = torch.from_numpy(_camera_rows(R_list, t_list, intr_list)).to(dev)
    limits = torch.from_numpy(np.concatenate([[float(depth_threshold[0]), float(depth_threshold[1])], _box(bbox).reshape(6)])).to(dev)
    cap = C * (-(-H // stride)) * (-(-W // stride))
    if cap > MAX_POINTS:
        raise ValueError(f"{cap} strided pixels exceed the device path's {MAX_POINTS} points")
    pts = torch.empty((max(cap, 1), 3), dtype=torch.float32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws, nbytes = _scratch(dev, max(cap, 1))
    _lib.call("ag_depth_cloud", dev, depth, mask, cams, limits, C, H, W, int(stride), pts, count, ws, nbytes)
    return DeviceCloud(pts, count)


def voxel_down_sample_device(cloud, voxel_size, extent_checked=False):
    """The voxel merge on the device: keys by HIP, a stable `torch.sort` of the 64-bit keys (plumbing), membership and the in-order float64 mean
    by HIP, ordered compaction by lowest member index.  The sort key holds VOXEL_KEY_LIMIT voxels per axis: a cloud wider than that raises
    (checked with the count in one read, unless the caller vouches for the extent: `extent_checked`)."""
    torch = _torch()
    from . import _lib
    import ctypes
    dev = cloud.pts.device
    bound = cloud.bound
    out = torch.empty((max(bound, 1), 3), dtype=torch.float32, device=dev)
    count = torch.empty(2, dtype=torch.int32, device=dev)          # [count, status]
    if bound == 0:
        return DeviceCloud(out, torch.zeros(1, dtype=torch.int32, device=dev), 0)
    keys = torch.empty(bound, dtype=torch.int64, device=dev)
    ws, nbytes = _scratch(dev, bound)
    voxel = ctypes.c_double(float(voxel_size))
    _lib.call("ag_cloud_voxel_keys", dev, cloud.pts, cloud.count, bound, ctypes.byref(voxel), keys, count[1:], ws, nbytes)
    skeys, perm = torch.sort(keys, stable=True)
    _lib.call("ag_cloud_voxel_merge", dev, cloud.pts, cloud.count, bound, skeys, perm, out, count[:1], ws, nbytes)
    res = DeviceCloud(out, count[:1])
    if not extent_checked:
        n, status = (int(v) for v in count.cpu())
        if status:
            raise ValueError(f"voxel_down_sample: the cloud spans more than {VOXEL_KEY_LIMIT} voxels of {voxel_size} along an axis")
        res.n = n
    return res


def knn_mean_device(cloud, nb_neighbors=20):
    """-> (avg (bound,) float64 tensor, info (2,) int32 tensor: [points finished by the brute-force pass, grid cells])."""
    torch = _torch()
    from . import _lib
    if not 1 <= int(nb_neighbors) <= MAX_NEIGHBORS:
        raise ValueError(f"the neighbour kernels are built for 1 <= nb_neighbors <= {MAX_NEIGHBORS}; got {nb_neighbors}")
    dev = cloud.pts.device
    bound = max(cloud.bound, 1)
    avg = torch.empty(bound, dtype=torch.float64, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    ws, nbytes = _scratch(dev, bound)
    _lib.call("ag_cloud_knn_mean", dev, cloud.pts, cloud.count, bound, int(nb_neighbors), avg, info, ws, nbytes)
    return avg, info


def outlier_filter_device(cloud, avg, std_ratio):
    """-> (kept cloud, keep (bound,) uint8, stats (3,) float64 [mean, std, threshold], progress (1,) int32: the new count, bit-complemented
    when nothing was removed)."""
    torch = _torch()
    from . import _lib
    import ctypes
    dev = cloud.pts.device
    bound = max(cloud.bound, 1)
    out = torch.empty((bound, 3), dtype=torch.float32, device=dev)
    count = torch.empty(2, dtype=torch.int32, device=dev)          # [count, progress]
    keep = torch.empty(bound, dtype=torch.uint8, device=dev)
    stats = torch.empty(3, dtype=torch.float64, device=dev)
    ws, nbytes = _scratch(dev, bound)
    ratio = ctypes.c_double(float(std_ratio))
    _lib.call("ag_cloud_outlier_filter", dev, cloud.pts, cloud.count, bound, avg, ctypes.byref(ratio), stats, keep, out, count, ws, nbytes)
    return DeviceCloud(out, count[:1]), keep, stats, count[1:]


def select_device(cloud, flags=None, z_below=None):
    """Ordered compaction of a cloud: the points whose `flags` byte is non-zero, or whose z is < `z_below` (a (1,) fp32 device tensor)."""
    torch = _torch()
    from . import _lib
    dev = cloud.pts.device
    bound = max(cloud.bound, 1)
    out = torch.empty((bound, 3), dtype=torch.float32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws, nbytes = _scratch(dev, bound)
    _lib.call("ag_cloud_select", dev, cloud.pts, cloud.count, bound, flags, z_below, out, count, ws, nbytes)
    return DeviceCloud(out, count)


def denoise_device(cloud, nb_neighbors=20, max_iter=64, stats=None):
    """The reference's loop on the device.  The host reads ONE 4-byte word per iteration (the new count, complemented when the iteration removed
    nothing) and nothing else.  `stats`: a list that receives, per iteration, the device tensors (info, threshold stats) for later inspection."""
    it = 0
    while it < max_iter and cloud.n != 0:
        avg, info = knn_mean_device(cloud, nb_neighbors)
        cloud, _keep, st, progress = outlier_filter_device(cloud, avg, 1.5 + 0.5 * it)
        it += 1
        if stats is not None:
            stats.append((info, st))
        word = int(progress.item())
        cloud.n = ~word if word < 0 else word
        if word < 0:
            break
    return cloud, it


def height_filter_device(cloud, k_filter):
    torch = _torch()
    if k_filter >= 1.0:
        return cloud
    n = cloud.size()
    if n == 0:
        return cloud
    z_thresh = torch.kthvalue(cloud.pts[:n, 2], int(k_filter * n) + 1).values.reshape(1).contiguous()      # the order statistic: plumbing
    return select_device(cloud, z_below=z_thresh)


# ---------------------------------------------------------------------------------------------------------------------
# public surface
# ---------------------------------------------------------------------------------------------------------------------
def depth_to_points(depth_list, R_list, t_list, intr_list, bbox, keep_masks=None, stride=4, depth_threshold=(0, 2), device=None):
    """Un-project, move to the board frame, crop.  -> (n, 3) float32, or a DeviceCloud with `device=` (cameras of one shape)."""
    if device is None:
        return depth_to_points_host(depth_list, R_list, t_list, intr_list, bbox, keep_masks, stride, depth_threshold)
    return depth_to_points_device(depth_list, R_list, t_list, intr_list, bbox, keep_masks, stride, depth_threshold, device)


def voxel_down_sample(points, voxel_size, device=None):
    if not _on_device(points, device):
        return voxel_down_sample_host(points, voxel_size)
    return voxel_down_sample_device(to_device_cloud(points, device), voxel_size)


def statistical_outlier_mask(points, nb_neighbors=20, std_ratio=2.0, device=None):
    """-> (keep, avg, threshold): numpy (bool (n,), float64 (n,), float64) on the host; on the device tensors of the cloud's `bound` rows
    (uint8, float64) and a 0-d float64 tensor, nothing read back."""
    if not _on_device(points, device):
        return statistical_outlier_mask_host(points, nb_neighbors, std_ratio)
    cloud = to_device_cloud(points, device)
    avg, _ = knn_mean_device(cloud, nb_neighbors)
    _, keep, stats, _ = outlier_filter_device(cloud, avg, std_ratio)
    return keep, avg, stats[2]


def denoise(points, nb_neighbors=20, max_iter=64, device=None):
    """-> (cloud, iterations)."""
    if not _on_device(points, device):
        return denoise_host(points, nb_neighbors, max_iter)
    return denoise_device(to_device_cloud(points, device), nb_neighbors, max_iter)


def height_filter(points, k_filter, device=None):
    if not _on_device(points, device):
        return height_filter_host(points, k_filter)
    return height_filter_device(to_device_cloud(points, device), k_filter)


def get_tabletop_points(depth_list, R_list, t_list, intr_list, bbox, keep_masks=None, stride=4, depth_threshold=(0, 2), use_raw=False,
                        k_filter=1.0, device=None):
    """perception.py:151-256 with the keep-masks as inputs: crop, then (unless `use_raw`, which also ignores the masks) voxel merge at 0.5 mm,
    the denoise loop and the height filter.  -> (n, 3) float32, or a DeviceCloud."""
    masks = None if use_raw else keep_masks
    if device is None:
        p = depth_to_points_host(depth_list, R_list, t_list, intr_list, bbox, masks, stride, depth_threshold)
        if use_raw:
            return p
        p, _ = denoise_host(voxel_down_sample_host(p, VOXEL_SIZE))
        return height_filter_host(p, k_filter)
    cloud = depth_to_points_device(depth_list, R_list, t_list, intr_list, bbox, masks, stride, depth_threshold, device)
    if use_raw:
        return cloud
    box = _box(bbox)
    extent_ok = bool(np.all((box[:, 1] - box[:, 0]) / VOXEL_SIZE + 2 < VOXEL_KEY_LIMIT))     # the crop bounds the cloud: no read-back needed
    cloud, _ = denoise_device(voxel_down_sample_device(cloud, VOXEL_SIZE, extent_checked=extent_ok))
    return height_filter_device(cloud, k_filter)


def state_from_depth(depth_list, R_list, t_list, intr_list, bbox, keep_masks=None, stride=4, depth_threshold=(0, 2), k_filter=1.0, *,
                     sim_real_ratio, fps_radius, max_nobj=100, device="cuda:0", return_details=False):
    """`get_state_cur` (perception.py:318-349) from the depth images on: the tabletop cloud, x sim_real_ratio, (x, y, z) -> (x, -z, y), then the
    two farthest-point passes of `construct_graph` (perception.py:266-279).  The RNG draws stay on the host in the host code's order (start of
    pass 1, start of pass 2), so one `np.random.seed` gives the same key points on either path.
    -> state_cur (n_kp, 3) fp32: a tensor on `device`, ready for `ChunkedPlanner.trajectory_optimization`; numpy from the host path with
    device=None.  The device is the default: this function feeds a planner that runs there, and at four 720 x 1280 images the device path took
    4.6 ms end to end against 355 ms for the host path in the same run (bench_tabletop.py).
    `return_details`: (state_cur, obj_kps, picked indices into obj_kps)."""
    from . import sampling
    radius = float(fps_radius)
    if device is None:
        obj_kps = to_sim_frame(get_tabletop_points(depth_list, R_list, t_list, intr_list, bbox, keep_masks, stride, depth_threshold, False, k_filter),
                               sim_real_ratio)
        if len(obj_kps) == 0:
            raise ValueError("state_from_depth: no point survived the crop and the filters")
        idx = sampling.fps(obj_kps, max_nobj, radius)
        return (obj_kps[idx], obj_kps, idx) if return_details else obj_kps[idx]
    torch = _torch()
    cloud = get_tabletop_points(depth_list, R_list, t_list, intr_list, bbox, keep_masks, stride, depth_threshold, False, k_filter, device)
    n = cloud.size()
    if n == 0:
        raise ValueError("state_from_depth: no point survived the crop and the filters")
    obj_kps = to_sim_frame(cloud.pts[:n], sim_real_ratio).contiguous()
    dev = obj_kps.device
    k1 = min(int(max_nobj), n)
    start1 = np.random.randint(0, n)
    start2 = np.random.randint(k1)
    i32 = lambda v: torch.tensor([v], dtype=torch.int32).to(dev)
    picks = sampling.two_pass_tensors(obj_kps[None], i32(n), i32(k1), i32(start1), i32(start2),
                                      torch.tensor([sampling.radius_as_compared(radius)], dtype=torch.float64).to(dev), k1)
    idx = picks[0, :int(picks[0, k1].item())].long()
    state_cur = obj_kps[idx]
    return (state_cur, obj_kps, idx) if return_details else state_cur
