"""Key-point down-sampling used to turn a recorded particle cloud into graph nodes — SURVEY.md §8f row n3.

`fps` mirrors src/dynamics/dataset/graph.py:8-36: a farthest-point pass down to `max_nobj` points followed by a
radius-limited farthest-point pass (`fps_rad_idx`, src/dynamics/utils.py:10-24).  The first pass is
`dgl.geometry.farthest_point_sampler` in the reference (DGL 1.x/2.x, not vendored and not installed here); its published
algorithm is restated in `farthest_point_sampler` below: start at `start_idx`, keep for every point the squared distance
to the nearest picked point, pick the arg-max (first index on ties), repeat.  Parity of that stage is therefore pinned to
the algorithm, not to DGL outputs.  Both passes draw from numpy's global RNG in the reference's order (start index of pass 1,
optional radius draw, start index of pass 2), so `np.random.seed(s)` reproduces the reference's node sets.

Two paths, one result.  numpy input (and `device=None`) runs the host code below, which is the statement of the arithmetic.  A GPU tensor, or
a `device`, runs the HIP kernel `ag_fps` (csrc/ag_fps.hip): one workgroup per cloud, the cloud in registers, the same fp32 operations in the same
order and the same lowest-index tie rule, so both paths return the same indices bit for bit (tests/test_fps.py) — and the RNG draws stay on the
host in the host code's order, so `np.random.seed(s)` gives the same node set on either path.  Measured on one MI355X against that machine's
CPU (bench_fps.py): 2 000 points / max_nobj 200 take 6.2 ms on the host and 0.49 ms on the device end to end, 4 096 / 1 000 take
56 ms and 1.8 ms, 64 clouds of 2 000 points 382 ms and 0.9 ms as one `fps_batch`.  The device call won at every measured size, so no size needs to
stay on the host for speed; the host path stays the default because it needs no GPU (dataset worker processes).
"""
import numpy as np

FPS_SQUARED, FPS_NORM = 0, 1        # AG_FPS_SQUARED / AG_FPS_NORM (include/adaptigraph_hip.h)
FPS_RESIDENT_POINTS = 8192          # AG_FPS_RESIDENT_POINTS: larger clouds take the streaming form of the kernel


def _is_gpu_tensor(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "is_cuda") and x.is_cuda


def radius_as_compared(radius):
    """The double `ag_fps` must be given so that its `distance > radius` (float32 against double, as doubles) answers what the host's
    `near.max() > radius` answers under the installed numpy: numpy >= 2 compares a float32 with a Python float IN float32 (the radius is rounded
    first), numpy 1.x and any np.float64 radius compare in float64."""
    return float((np.float32(0) + radius).dtype.type(radius))


def fps_device(pts, count, start, K, metric, radius=None):
    """`ag_fps` on device tensors, enqueued on the current stream with no host synchronisation (safe under stream capture).
    pts (B,N,3) fp32 contiguous; count (B) int32 or None (all N points valid); start (B) int32; radius (B) float64 or None (FPS_NORM only: stop
    once every point is within radius[b] of a pick).  -> (idx (B,K) int32 with -1 past a cloud's last pick, n (B) int32 picks made)."""
    import torch
    from . import _lib
    _lib._require_gpu(pts, "pts")
    if pts.dtype != torch.float32:
        raise TypeError(f"ag_fps computes in float32; got {pts.dtype} (cast explicitly if rounding the cloud is intended)")
    assert pts.dim() == 3 and pts.shape[2] == 3 and pts.is_contiguous()
    B, N = int(pts.shape[0]), int(pts.shape[1])
    dev = pts.device
    for t, dt in ((count, torch.int32), (start, torch.int32), (radius, torch.float64)):
        assert t is None or (t.device == dev and t.dtype == dt and t.shape == (B,) and t.is_contiguous())
    L = _lib.lib()
    ws_bytes = L.ag_fps_workspace_bytes(B, N)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    idx = torch.empty((B, int(K)), dtype=torch.int32, device=dev)
    n = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.call("ag_fps", dev, pts, count, start, B, N, int(K), int(metric), radius, idx, n, ws, ws_bytes)
    return idx, n


def farthest_point_sampler(pos, npoints, start_idx=None):
    """pos (B,N,3) array-like -> (B,npoints) int64 indices, DGL semantics (squared distances, first arg-max).
    A GPU tensor takes the device path and returns an int64 tensor on its device (what DGL returns); the start indices are drawn on the host
    exactly as below (one draw per cloud, in order)."""
    if _is_gpu_tensor(pos):
        import torch
        B, N, _ = pos.shape
        assert 0 < npoints <= N
        start = [np.random.randint(0, N) if start_idx is None else int(start_idx) for _ in range(B)]
        idx, _n = fps_device(pos.contiguous(), None, torch.tensor(start, dtype=torch.int32).to(pos.device), npoints, FPS_SQUARED)
        return idx.long()
    pos = np.asarray(pos, np.float32)
    B, N, _ = pos.shape
    assert 0 < npoints <= N
    out = np.zeros((B, npoints), np.int64)
    for b in range(B):
        cur = np.random.randint(0, N) if start_idx is None else int(start_idx)
        near = np.full(N, np.inf, np.float32)
        for k in range(npoints):
            out[b, k] = cur
            d = pos[b] - pos[b, cur]
            near = np.minimum(near, (d * d).sum(1, dtype=np.float32))
            cur = int(near.argmax())
    return out


def fps_rad_idx(pcd, radius):
    """Farthest-point picks until every point is within `radius` of a pick -> (picked points, their indices).
    A GPU tensor (N,3) takes the device path and returns tensors.  That path is float32 only: the host code computes in the dtype it is given,
    so a float64 tensor raises TypeError instead of being rounded silently."""
    if _is_gpu_tensor(pcd):
        import torch
        if pcd.dtype != torch.float32:
            raise TypeError(f"fps_rad_idx on the GPU computes in float32; got {pcd.dtype}")
        n = int(pcd.shape[0])
        first = np.random.randint(n)
        idx, cnt = fps_device(pcd.contiguous()[None], None, torch.tensor([first], dtype=torch.int32).to(pcd.device), n, FPS_NORM,
                              torch.tensor([radius_as_compared(radius)], dtype=torch.float64).to(pcd.device))
        picks = idx[0, :int(cnt.item())].long()
        return pcd[picks], picks
    first = np.random.randint(pcd.shape[0])
    picks = [first]
    near = np.linalg.norm(pcd - pcd[first], axis=1)
    while near.max() > radius:
        nxt = near.argmax()
        picks.append(nxt)
        near = np.minimum(near, np.linalg.norm(pcd - pcd[nxt], axis=1))
    picks = np.stack(picks, axis=0)
    return pcd[picks], picks


def _draw_radius(fps_radius_range):
    if type(fps_radius_range) == float:
        return fps_radius_range
    if len(fps_radius_range) == 2:
        return np.random.uniform(fps_radius_range[0], fps_radius_range[1])
    raise ValueError(f"Invalid fps_radius_range: {fps_radius_range}.")


def two_pass_tensors(pts, n, k1, start1, start2, radius, K):
    """Both passes of `fps` on device tensors, no host synchronisation: pts (B,N,3) fp32 padded clouds, n (B) int32 their sizes, k1 (B) int32 =
    min(max_nobj, n), start1 / start2 (B) int32, radius (B) float64 (see radius_as_compared), K = max(k1).
    -> (B,K+1) int32: the picked indices into each cloud (-1 behind the last) and, in column K, their number."""
    import torch
    B = pts.shape[0]
    coarse, _ = fps_device(pts, n, start1, K, FPS_SQUARED)                       # (B,K): cloud b has exactly k1[b] picks, then -1
    coarse_pts = torch.gather(pts, 1, coarse.clamp_min(0).long()[:, :, None].expand(B, K, 3)).contiguous()
    fine, n_fine = fps_device(coarse_pts, k1, start2, K, FPS_NORM, radius)
    picked = torch.where(fine >= 0, torch.gather(coarse, 1, fine.clamp_min(0).long()), fine)
    return torch.cat([picked, n_fine[:, None]], 1)


def _two_pass_device(clouds, start1, radii, start2, max_nobj, device):
    """Both passes of `fps` for a list of (n_i,3) clouds on `device`, one launch per pass: pass 1 (squared distances) down to min(max_nobj, n_i)
    points from start1[i], a gather of the picked points, pass 2 (norms) from start2[i] until every picked point is within radii[i] of a pick,
    the composition of the two index lists on the device and ONE copy back.  -> [int32 index array per cloud]."""
    import torch
    dev = torch.device(device)
    B = len(clouds)
    n = [int(c.shape[0]) for c in clouds]
    k1 = [min(int(max_nobj), m) for m in n]
    N, K = max(n), max(k1)
    host = np.zeros((B, N, 3), np.float32)
    for b, c in enumerate(clouds):
        host[b, :n[b]] = np.asarray(c).astype(np.float32)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)
    radius = torch.tensor([radius_as_compared(r) for r in radii], dtype=torch.float64).to(dev)
    back = two_pass_tensors(torch.from_numpy(host).to(dev), i32(n), i32(k1), i32(start1), i32(start2), radius, K).cpu().numpy()
    return [back[b, :back[b, K]].astype(np.int32) for b in range(B)]


def fps_batch(clouds, max_nobj, fps_radius_range, device):
    """[(n_i,3) arrays] -> [index arrays]: `fps` of every cloud on `device`, all clouds in one launch per pass (padded to the largest).  The RNG
    is drawn cloud by cloud in the order successive `fps` calls draw it (start of pass 1, radius if a range, start of pass 2), so the result
    equals `[fps(c, max_nobj, fps_radius_range) for c in clouds]` element for element under the same seed."""
    start1, radii, start2 = [], [], []
    for c in clouds:
        n = c.shape[0]
        start1.append(np.random.randint(0, n))
        radii.append(_draw_radius(fps_radius_range))
        start2.append(np.random.randint(min(max_nobj, n)))
    if not clouds:
        return []
    return [np.array(i) for i in _two_pass_device(clouds, start1, radii, start2, max_nobj, device)]


def fps(obj_kp_start, max_nobj, fps_radius_range, verbose=False, device=None):
    """obj_kp_start (N,3) -> indices (n_fps,) into it; `fps_radius_range` is a float or a [lo, hi] range to draw from.
    `device` (e.g. "cuda:0"): both passes run there (`ag_fps`), the three RNG draws stay on the host in the order below; same indices."""
    if device is not None:
        idx = fps_batch([obj_kp_start], max_nobj, fps_radius_range, device)[0]
        if verbose:
            print(f"FPS num particles: {len(idx)} with index list \n {idx}. \n")
        return idx
    n = obj_kp_start.shape[0]
    coarse = farthest_point_sampler(obj_kp_start[None].astype(np.float32), min(max_nobj, n),
                                    start_idx=np.random.randint(0, n))[0].astype(np.int32)
    if type(fps_radius_range) == float:
        radius = fps_radius_range
    elif len(fps_radius_range) == 2:
        radius = np.random.uniform(fps_radius_range[0], fps_radius_range[1])
    else:
        raise ValueError(f"Invalid fps_radius_range: {fps_radius_range}.")
    _, fine = fps_rad_idx(obj_kp_start[coarse].astype(np.float32), radius)
    idx = coarse[fine.astype(np.int32)]
    if verbose:
        print(f"FPS num particles: {len(idx)} with index list \n {idx}. \n")
    return np.array(idx)
