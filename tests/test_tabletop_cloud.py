"""The tabletop cloud from depth images (adaptigraph_amd/perception.py, csrc/ag_tabletop.hip): the host statement against hand-checkable cases
and an O(n^2) computation written here, and the HIP path against the host statement on the same inputs.  open3d is not available, so parity
is pinned to the algorithm as the module docstring states it, not to library outputs."""
import ctypes
import os

import numpy as np
import pytest
import torch

from adaptigraph_amd import _lib, perception as P, sampling, synth

DEV = "cuda:0"
EYE, ZERO = np.eye(3), np.zeros(3)
BIG_BOX = np.array([[-1e6, 1e6]] * 3)


# ------------------------------------------------------------------------------------------------------ inputs
def curve_cloud(seed, n_curve=1500, n_out=30):
    """A noisy curve plus uniform outliers in a larger box, fp32."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0, 1, n_curve)
    curve = np.stack([0.4 * t, 0.1 * np.sin(2 * np.pi * t), np.full(n_curve, 0.02)], 1) + rng.normal(0, 0.002, (n_curve, 3))
    out = rng.uniform([-0.3, -0.5, -0.2], [0.7, 0.5, 0.4], (n_out, 3))
    return np.concatenate([curve, out])[rng.permutation(n_curve + n_out)].astype(np.float32)


def uniform_cloud(seed, n, scale=1.0):
    return (np.random.default_rng(seed).uniform(0, 1, (n, 3)) * scale).astype(np.float32)


def reference_mask(p32, nb, ratio):
    """The contract in three lines of O(n^2) numpy (lexsort: the total order (d2, j))."""
    p = p32.astype(np.float64)
    n, k = len(p), min(nb, len(p))
    d2 = ((p[:, None, 0] - p[None, :, 0]) ** 2 + (p[:, None, 1] - p[None, :, 1]) ** 2) + (p[:, None, 2] - p[None, :, 2]) ** 2
    nbr = np.stack([np.lexsort((np.arange(n), d2[i]))[:k] for i in range(n)])
    avg = np.array([sum(np.sqrt(d2[i, j]) for j in nbr[i]) / k for i in range(n)])
    pos = avg[avg > 0]
    mean = pos.sum() / n
    thr = mean + ratio * np.sqrt(((pos - mean) ** 2).sum() / (n - 1)) if n > 1 else 0.0
    return (avg > 0) & (avg < thr) & (n > 1), avg, thr


def margin(avg, thr):
    """min |avg - threshold| / threshold over the points the threshold decides (avg > 0)."""
    a = avg[avg > 0]
    return np.inf if len(a) == 0 or thr <= 0 else float(np.min(np.abs(a - thr)) / thr)


def checked_host_denoise(p, max_iter=64):
    """denoise_host step by step, asserting on HOST values that no decision of any iteration is closer than 1e-9 to its threshold."""
    alive, it = np.arange(len(p)), 0
    while it < max_iter and len(p):
        keep, avg, thr = P.statistical_outlier_mask_host(p, 20, 1.5 + 0.5 * it)
        if len(p) > 2:
            assert margin(avg, thr) >= 1e-9, (it, margin(avg, thr))
        it += 1
        removed = len(p) - int(keep.sum())
        p, alive = p[keep], alive[keep]
        if removed == 0:
            break
    return p, it, alive


def cameras(rng, C, H, W):
    """Tilted extrinsics and pinhole intrinsics; depths with zeros, NaNs and values beyond the limit; masks."""
    R, t, K, depth, masks = [], [], [], [], []
    for _ in range(C):
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        R.append(q * np.sign(np.linalg.det(q)))
        t.append(rng.uniform(-0.2, 0.2, 3))
        K.append(np.array([[40.0 + rng.uniform(0, 5), 0, W / 2.0], [0, 42.0 + rng.uniform(0, 5), H / 2.0], [0, 0, 1.0]]))
        d = rng.uniform(0.2, 2.6, (H, W)).astype(np.float32)
        pick = rng.random((H, W))
        d[pick < 0.05] = 0.0
        d[(pick >= 0.05) & (pick < 0.1)] = np.nan
        d[(pick >= 0.1) & (pick < 0.12)] = 7.5
        depth.append(d)
        masks.append(rng.random((H, W)) < 0.8)
    return depth, R, t, K, masks


# ------------------------------------------------------------------------------------------------------ CPU: the host statement
def test_tabletop_entry_points_and_argument_checks():
    L = _lib.lib()
    names = ("ag_tabletop_workspace_bytes", "ag_depth_cloud", "ag_cloud_voxel_keys", "ag_cloud_voxel_merge", "ag_cloud_knn_mean",
             "ag_cloud_outlier_filter", "ag_cloud_select")
    for name in names:
        assert name in _lib.EXPORTS and hasattr(L, name)
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "adaptigraph_hip.h")).read()
    assert f"#define AG_TABLETOP_MAX_POINTS (1 << 20)\n" in header and P.MAX_POINTS == 1 << 20 >= 230400
    assert f"#define AG_TABLETOP_MAX_NEIGHBORS {P.MAX_NEIGHBORS}\n" in header
    assert f"#define AG_TABLETOP_VOXEL_KEY_LIMIT (1 << 21)\n" in header and P.VOXEL_KEY_LIMIT == 1 << 21
    need = L.ag_tabletop_workspace_bytes(1000)
    assert 0 < need < L.ag_tabletop_workspace_bytes(230400) < 64 << 20
    assert L.ag_tabletop_workspace_bytes(0) == 0 and L.ag_tabletop_workspace_bytes(P.MAX_POINTS + 1) == 0
    buf, ws = (ctypes.c_char * 64)(), (ctypes.c_char * need)()
    one = ctypes.c_double(1.0)
    assert L.ag_cloud_knn_mean(buf, buf, P.MAX_POINTS + 1, 20, buf, buf, ws, need, None) == -1 and b"AG_TABLETOP_MAX_POINTS" in L.ag_last_error()
    assert L.ag_cloud_knn_mean(buf, buf, 1000, 21, buf, buf, ws, need, None) == -1 and b"k = 21" in L.ag_last_error()
    assert L.ag_cloud_knn_mean(None, buf, 1000, 20, buf, buf, ws, need, None) == -1 and b"null" in L.ag_last_error()
    assert L.ag_cloud_knn_mean(buf, buf, 1000, 20, buf, buf, ws, need - 1, None) == -3 and b"workspace" in L.ag_last_error()
    assert L.ag_cloud_select(buf, buf, 1000, None, None, buf, buf, ws, need, None) == -1 and b"one of them" in L.ag_last_error()
    assert L.ag_cloud_select(buf, buf, 1000, buf, buf, buf, buf, ws, need, None) == -1
    assert L.ag_cloud_voxel_keys(buf, buf, 1000, ctypes.byref(ctypes.c_double(0.0)), buf, buf, ws, need, None) == -1
    assert L.ag_cloud_outlier_filter(buf, buf, 1000, buf, ctypes.byref(one), buf, buf, None, buf, ws, need, None) == -1
    assert L.ag_depth_cloud(buf, None, buf, buf, 4, 2048, 2048, 1, buf, buf, ws, need, None) == -1 and b"strided pixels" in L.ag_last_error()
    assert L.ag_depth_cloud(buf, None, buf, buf, 1, 8, 8, 0, buf, buf, ws, need, None) == -1
    assert "memory" in P.__doc__ and "open3d" in P.__doc__            # what was restated from memory is said where a reader looks first


def test_depth_to_points_exact_cases():
    """Identity intrinsics / extrinsics and power-of-two depths: p = (u d, v d, d) exactly."""
    d = np.full((3, 5), 0.5, np.float32)
    d[0, 1], d[1, 2], d[2, 0], d[2, 4] = np.nan, 2.0, 0.0, 0.25
    pts, pix = P.depth_to_points_host([d], [EYE], [ZERO], [EYE], BIG_BOX, stride=1, depth_threshold=(0, 2), return_pixels=True)
    kept = {(int(v), int(u)) for _, v, u in pix}
    assert (0, 1) not in kept and (1, 2) not in kept and (2, 0) not in kept            # NaN; d == hi (strict); d == lo (strict)
    assert len(pts) == 12 and pts.dtype == np.float32
    assert np.array_equal(pix[:, 1] * 5 + pix[:, 2], np.sort(pix[:, 1] * 5 + pix[:, 2]))          # row-major
    for (c, v, u), p in zip(pix, pts):
        assert np.array_equal(p, np.float32([u * d[v, u], v * d[v, u], d[v, u]]))
    # the crop is inclusive on both sides: planes exactly at x = 0.5 (u = 1) and x = 1.5 (u = 3), y = 0.5 .. 1.0 (v = 1, 2)
    box = np.array([[0.5, 1.5], [0.5, 1.0], [0.0, 1.0]])
    pts, pix = P.depth_to_points_host([d], [EYE], [ZERO], [EYE], box, stride=1, return_pixels=True)
    assert sorted((int(v), int(u)) for _, v, u in pix) == [(1, 1), (1, 3), (2, 1), (2, 2), (2, 3), (2, 4)]      # (2, 4): 0.25 * (4, 2, 1) = (1, 0.5, 0.25)
    # masks, the stride (odd sizes: the tails), two cameras in camera-major order
    m = np.ones((3, 5), bool)
    m[2, 2] = False
    pts, pix = P.depth_to_points_host([d, d], [EYE, EYE], [ZERO, np.array([0, 0, 1.0])], [EYE, EYE], BIG_BOX, [m, m], stride=2, return_pixels=True)
    assert [tuple(r) for r in pix] == [(0, 0, 0), (0, 0, 2), (0, 0, 4), (0, 2, 4), (1, 0, 0), (1, 0, 2), (1, 0, 4), (1, 2, 4)]
    assert np.array_equal(pts[4:, 2], pts[:4, 2] + 1) and np.array_equal(P.depth_to_points([d], [EYE], [ZERO], [EYE], BIG_BOX, stride=1),
                                                                         P.depth_to_points_host([d], [EYE], [ZERO], [EYE], BIG_BOX, stride=1))


def test_voxel_down_sample_hand_cases():
    v = 0.5
    # origin = min - v / 2 = -0.25: voxel 0 = [-0.25, 0.25), voxel 1 = [0.25, 0.75)
    two_in_one = np.float32([[0, 0, 0], [0.125, 0, 0]])
    assert np.array_equal(P.voxel_down_sample(two_in_one, v), np.float32([[0.0625, 0, 0]]))
    straddle = np.float32([[0, 0, 0], [0.1875, 0, 0], [0.3125, 0, 0]])
    assert np.array_equal(P.voxel_down_sample(straddle, v), np.float32([[0.09375, 0, 0], [0.3125, 0, 0]]))
    on_plane = np.float32([[0, 0, 0], [0.25, 0, 0], [0.75, 0, 0]])            # exactly origin + 1 v and origin + 2 v: they open voxels 1 and 2
    assert np.array_equal(P.voxel_keys_host(on_plane, v)[:, 0], [0, 1, 2])
    assert np.array_equal(P.voxel_down_sample(on_plane, v), on_plane)
    # output order = ascending lowest member index; the mean adds members in ascending index
    mixed = np.float32([[0.875, 0, 0], [0, 0, 0], [0.8125, 0, 0], [0.0625, 0, 0], [0.4, 0, 0]])
    assert np.array_equal(P.voxel_down_sample(mixed, v), np.float32([[(0.875 + 0.8125) / 2, 0, 0], [0.03125, 0, 0], [0.4, 0, 0]]))
    assert P.voxel_down_sample(np.zeros((0, 3), np.float32), v).shape == (0, 3)


@pytest.mark.parametrize("n", [1, 2, 19, 20, 21])
def test_outlier_mask_against_the_quadratic_reference(n):
    p = uniform_cloud(n, n)
    keep, avg, thr = P.statistical_outlier_mask(p, 20, 2.0)
    want_keep, want_avg, want_thr = reference_mask(p, 20, 2.0)
    assert np.array_equal(keep, want_keep) and np.allclose(avg, want_avg, rtol=1e-14, atol=0) and np.isclose(thr, want_thr, rtol=1e-14)
    if n == 1:
        assert not keep.any()
    if n == 2:
        assert not keep.any() and avg[0] == avg[1] == thr            # the exact tie: strict <, both removed


def test_outlier_mask_duplicates_and_accelerated_search():
    p = np.concatenate([uniform_cloud(3, 60), np.tile(np.float32([[0.5, 0.5, 0.5]]), (25, 1))])
    keep, avg, thr = P.statistical_outlier_mask(p, 20, 2.0)
    want_keep, want_avg, want_thr = reference_mask(p, 20, 2.0)
    assert np.all(avg[60:] == 0) and not keep[60:].any()            # 25 duplicates: their 20 nearest are at distance 0
    assert np.array_equal(keep, want_keep) and np.allclose(avg, want_avg, rtol=1e-14, atol=0) and np.isclose(thr, want_thr, rtol=1e-14)
    pos = avg[:60]
    assert np.isclose(thr, pos.sum() / 85 + 2.0 * np.sqrt(((pos - pos.sum() / 85) ** 2).sum() / 84), rtol=1e-14)      # duplicates: out of the sums, in n
    big = np.concatenate([uniform_cloud(4, 5000), np.tile(np.float32([[0.25, 0.25, 0.25]]), (30, 1))])            # the k-d tree path and its redo
    assert np.array_equal(P.knn_mean_host(big, 20), P.knn_mean_host(big, 20, accelerate=False))


def test_denoise_terminates_with_the_reference_ratios(monkeypatch):
    p = curve_cloud(0)
    ratios = []
    real = P.statistical_outlier_mask_host
    monkeypatch.setattr(P, "statistical_outlier_mask_host", lambda pts, nb, r: ratios.append(r) or real(pts, nb, r))
    out, it = P.denoise(p)
    assert ratios == [1.5 + 0.5 * r for r in range(it)] and 2 <= it < 64
    monkeypatch.undo()
    want, want_it, alive = checked_host_denoise(p)
    assert it == want_it and np.array_equal(out, want) and np.array_equal(out, p[alive]) and 1400 < len(out) < 1530
    keep, _, _ = P.statistical_outlier_mask(out, 20, 1.5 + 0.5 * (it - 1))
    assert keep.all()                                                  # the last iteration removed nothing
    assert P.denoise(p, max_iter=1)[1] == 1
    assert P.denoise(np.zeros((0, 3), np.float32)) [1] == 0


def test_height_filter_host():
    p = np.float32([[0, 0, 3], [1, 0, 1], [2, 0, 2], [3, 0, 1], [4, 0, 2], [5, 0, 0]])
    assert P.height_filter(p, 1.0) is not None and np.array_equal(P.height_filter(p, 1.0), p)
    assert np.array_equal(P.height_filter(p, 0.5)[:, 0], [1, 3, 5])            # sorted z = 0 1 1 2 2 3: z_thresh = z[3] = 2, strict <
    assert len(P.height_filter(p, 0.0)) == 0


def test_get_tabletop_points_chains_the_host_stages():
    s = synth.tabletop_scene(2, 48, 64, seed=1, band=0.12)
    args = (s["depth"], s["R"], s["t"], s["intr"], s["bbox"])
    crop = P.depth_to_points(*args, keep_masks=s["masks"], stride=2)
    want = P.height_filter_host(P.denoise_host(P.voxel_down_sample_host(crop, P.VOXEL_SIZE))[0], 0.8)
    got = P.get_tabletop_points(*args, keep_masks=s["masks"], stride=2, k_filter=0.8)
    assert np.array_equal(got, want) and 50 < len(got) < len(crop)
    raw = P.get_tabletop_points(*args, keep_masks=s["masks"], stride=2, use_raw=True)
    assert np.array_equal(raw, P.depth_to_points(*args, keep_masks=None, stride=2)) and len(raw) > len(crop)
    np.random.seed(5)
    state, kps, idx = P.state_from_depth(*args, keep_masks=s["masks"], stride=2, sim_real_ratio=10.0, fps_radius=0.2, device=None,
                                         return_details=True)
    full = P.get_tabletop_points(*args, keep_masks=s["masks"], stride=2)
    assert np.array_equal(kps, np.stack([full[:, 0] * np.float32(10), -(full[:, 2] * np.float32(10)), full[:, 1] * np.float32(10)], 1))
    np.random.seed(5)
    assert np.array_equal(idx, sampling.fps(kps, 100, 0.2)) and np.array_equal(state, kps[idx]) and state.dtype == np.float32


# ------------------------------------------------------------------------------------------------------ GPU: the HIP path against the host path
gpu = pytest.mark.gpu


def same_bits_twice(fn):
    a, b = fn(), fn()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    return a


@gpu
@pytest.mark.parametrize("C,H,W,stride,seed", [(2, 32, 48, 4, 0), (1, 33, 47, 1, 1)])
def test_depth_to_points_device(C, H, W, stride, seed):
    rng = np.random.default_rng(seed)
    depth, R, t, K, masks = cameras(rng, C, H, W)
    box = np.array([[-0.6, 0.9], [-0.7, 0.8], [-1.0, 0.75]])            # cuts the cloud
    # conditions on the inputs, from host values: nothing within relative 1e-9 of a depth limit (exact zeros aside: 0 > 0 is the same exact
    # comparison on both paths) or of a crop plane (checked at 1e-6 on the fp32-rounded points of an uncropped run, which implies it)
    lo, hi = 0.0, 2.0
    for d in depth:
        f = d[np.isfinite(d) & (d != 0)].astype(np.float64)
        assert np.all(np.abs(f - hi) > 1e-9 * hi) and np.all(np.abs(f - lo) > 1e-9)
    everything = P.depth_to_points_host(depth, R, t, K, BIG_BOX, masks, stride, (lo, hi)).astype(np.float64)
    for a in range(3):
        for plane in box[a]:
            assert np.all(np.abs(everything[:, a] - plane) > 1e-6 * max(1.0, abs(plane)))
    want, pix = P.depth_to_points_host(depth, R, t, K, box, masks, stride, (lo, hi), return_pixels=True)
    assert 0.1 * len(everything) < len(want) < 0.9 * len(everything)
    run = lambda: (lambda c: (c.pts[:c.size()], c.count))(P.depth_to_points(depth, R, t, K, box, masks, stride, (lo, hi), device=DEV))
    got = same_bits_twice(run)[0].cpu().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)            # the same kept pixels ...
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))), np.abs(got - want).max()      # ... in the same order
    # without masks, and use_raw
    raw = P.get_tabletop_points(depth, R, t, K, box, masks, stride, (lo, hi), use_raw=True, device=DEV).numpy()
    want_raw = P.depth_to_points_host(depth, R, t, K, box, None, stride, (lo, hi))
    assert raw.shape == want_raw.shape and np.all(np.abs(raw.astype(np.float64) - want_raw) <= np.spacing(np.abs(want_raw)))


def stacked_cloud(n, seed):
    """Two "cameras" seeing the same surface points up to 0.2 mm of jitter, interleaved by a permutation."""
    rng = np.random.default_rng(seed)
    m = (n + 1) // 2
    base = np.stack([rng.uniform(0, 0.04, m), rng.uniform(0, 0.03, m), rng.normal(0.01, 0.0003, m)], 1)
    both = np.concatenate([base + rng.uniform(-1e-4, 1e-4, (m, 3)), base + rng.uniform(-1e-4, 1e-4, (m, 3))])[:n]
    return both[rng.permutation(n)].astype(np.float32)


@gpu
@pytest.mark.parametrize("n", [1, 2, 257, 3000])
def test_voxel_down_sample_device(n):
    p = stacked_cloud(n, n)
    want = P.voxel_down_sample_host(p, 0.0005)
    if n >= 257:
        assert 0.5 * n <= len(want) < 0.95 * n            # voxels with one, two and more members
    run = lambda: (lambda c: (c.pts[:c.size()], c.count))(P.voxel_down_sample(p, 0.0005, device=DEV))
    got = same_bits_twice(run)[0].cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    if n == 3000:            # a coarse voxel: many members per voxel; and a cloud too wide for the sort key is refused
        assert np.array_equal(P.voxel_down_sample(p, 0.004, device=DEV).numpy(), P.voxel_down_sample_host(p, 0.004))
        with pytest.raises(ValueError, match="voxels"):
            P.voxel_down_sample(np.float32([[0, 0, 0], [3000.0, 0, 0]]), 0.0005, device=DEV)


def outlier_clouds():
    rng = np.random.default_rng(7)
    cases = {f"uniform{n}": uniform_cloud(n, n) for n in (1, 2, 19, 20, 21, 257)}
    cases["curve1530"] = curve_cloud(0)
    cases["duplicates"] = np.concatenate([uniform_cloud(3, 300), np.tile(np.float32([[0.5, 0.5, 0.5]]), (25, 1)),
                                          np.tile(np.float32([[0.25, 0.5, 0.125]]), (7, 1))])
    # 512 points in [0, 1]^2 x [0, 1/16]: the grid rule (about eight points per cell: h = sqrt(8 * 1 * 1 / 512) = 1/8 exactly, 9 x 9 x 1 cells
    # from the cloud's minimum 0) puts every lattice point below exactly on a cell border in x and in y
    lattice = np.stack(np.meshgrid(np.arange(9) / 8, np.arange(9) / 8, np.arange(3) / 32, indexing="ij"), -1).reshape(-1, 3)
    cases["cell_borders"] = np.concatenate([lattice, rng.uniform(0, 1, (512 - 243, 3)) * [1, 1, 1 / 16]]).astype(np.float32)
    cases["two_clusters"] = np.concatenate([uniform_cloud(5, 400, 0.01), uniform_cloud(6, 400, 0.01) + np.float32([3.0, 0, 0])])
    cases["far_point"] = np.concatenate([uniform_cloud(8, 600, 0.05), np.float32([[40.0, -25.0, 10.0]])])
    return cases


OUTLIER_CLOUDS = outlier_clouds()
_HOST_MASKS = {}


def host_mask(name, ratio=2.0):
    if (name, ratio) not in _HOST_MASKS:
        _HOST_MASKS[(name, ratio)] = P.statistical_outlier_mask_host(OUTLIER_CLOUDS[name], 20, ratio)
    return _HOST_MASKS[(name, ratio)]


@gpu
@pytest.mark.parametrize("name", list(OUTLIER_CLOUDS))
def test_statistical_outlier_mask_device(name):
    p = OUTLIER_CLOUDS[name]
    n = len(p)
    keep, avg, thr = host_mask(name)
    if n != 2:                      # (n = 2 is the deliberate exact tie: avg == threshold, removed on both paths)
        assert margin(avg, thr) >= 1e-9, margin(avg, thr)
    got_keep, got_avg, got_thr = same_bits_twice(lambda: P.statistical_outlier_mask(p, 20, 2.0, device=DEV))
    got_keep, got_avg, got_thr = got_keep.cpu().numpy().astype(bool)[:n], got_avg.cpu().numpy()[:n], float(got_thr)
    assert np.array_equal(got_avg == 0, avg == 0)
    assert np.all(np.abs(got_avg - avg) <= 1e-14 * avg), float(np.max(np.abs(got_avg - avg) / np.maximum(avg, 1e-300)))
    assert np.array_equal(got_keep, keep)
    assert np.array_equal((got_avg > 0) & (got_avg < got_thr), keep)            # the threshold's decision for every point, from device values
    assert abs(got_thr - float(thr)) <= 1e-12 * abs(float(thr))
    if n == 2:
        assert not got_keep.any() and got_avg[0] == got_avg[1] == got_thr
    cloud = P.to_device_cloud(p, DEV)
    avg2, info = P.knn_mean_device(cloud, 20)
    assert torch.equal(avg2[:n].cpu(), torch.from_numpy(got_avg))
    brute, cells = (int(v) for v in info.cpu())
    assert 0 <= brute <= n and cells >= 1
    if name == "far_point":
        assert brute >= 1                # too far for the ring limit: finished by the brute-force pass
    if name == "cell_borders":
        assert cells == 81               # the grid the case was built for
    if name == "two_clusters":
        assert cells > 20                # an empty span of many cells between the clusters
    if name == "curve1530":
        assert brute < n // 4            # the grid resolves the bulk
        for k in (1, 5):                 # fewer neighbours than the kernels' capacity
            small, _ = P.knn_mean_device(cloud, k)
            assert np.all(np.abs(small[:n].cpu().numpy() - P.knn_mean_host(p, k)) <= 1e-14 * P.knn_mean_host(p, k))


@gpu
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_denoise_device(seed):
    p = curve_cloud(seed)
    want, want_it, alive = checked_host_denoise(p)
    assert 2 <= want_it <= 8
    cloud, it = P.denoise(p, device=DEV)
    assert it == want_it and cloud.n == len(want) == int(cloud.count.item())
    assert np.array_equal(cloud.numpy(), want)            # the points are distinct: the same rows = the same surviving indices, in order
    again, it2 = P.denoise(p, device=DEV)
    assert it2 == it and np.array_equal(again.numpy(), cloud.numpy())
    assert P.denoise(p, max_iter=1, device=DEV)[1] == 1


@gpu
def test_device_stages_do_not_synchronise_the_host():
    """What a denoise iteration calls reads nothing back: the loop's own 4-byte read of `progress` is its only one.  Counts stay device words."""
    p = curve_cloud(0)
    keep, _, _ = P.statistical_outlier_mask_host(p, 20, 1.5)
    z = torch.full((1,), 0.02, dtype=torch.float32, device=DEV)

    resident = P.to_device_cloud(p, DEV)

    def stages():
        cloud = P.DeviceCloud(resident.pts, resident.count)                     # n unknown: as behind a stage whose count the host has not read
        merged = P.voxel_down_sample_device(cloud, P.VOXEL_SIZE, extent_checked=True)
        avg, _info = P.knn_mean_device(cloud, 20)
        kept, _keep, _stats, progress = P.outlier_filter_device(cloud, avg, 1.5)
        return merged, kept, progress, P.select_device(kept, z_below=z)

    stages()                        # (warm: the scratch buffer exists)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        merged, kept, progress, low = stages()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert int(progress.item()) == int(kept.count.item()) == int(keep.sum()) < len(p)
    assert np.array_equal(kept.numpy(), p[keep]) and np.array_equal(low.numpy(), p[keep][p[keep][:, 2] < np.float32(0.02)])
    assert np.array_equal(merged.numpy(), P.voxel_down_sample_host(p, P.VOXEL_SIZE))


@gpu
def test_denoise_device_all_outlier_clouds_end_empty():
    for p in (np.tile(np.float32([[0.1, 0.2, 0.3]]), (40, 1)), np.float32([[0, 0, 0], [1, 0, 0]]), np.float32([[1, 2, 3]])):
        assert len(P.denoise_host(p)[0]) == 0
        cloud, it = P.denoise(p, device=DEV)
        assert it == 1 and cloud.n == 0 and int(cloud.count.item()) == 0 and cloud.numpy().shape == (0, 3)
    cloud, it = P.denoise(np.zeros((0, 3), np.float32), device=DEV)
    assert it == 0 and cloud.numpy().shape == (0, 3)


@gpu
def test_height_filter_device():
    rng = np.random.default_rng(3)
    p = rng.uniform(0, 1, (700, 3)).astype(np.float32)
    p[:, 2] = np.round(p[:, 2] * 16) / 16                  # ties in z
    for k in (0.5, 1.0, 0.0, 0.999):
        got = P.height_filter(p, k, device=DEV).numpy()
        assert np.array_equal(got, P.height_filter_host(p, k)), k
    assert 200 < len(P.height_filter_host(p, 0.5)) < 350            # strict < at a tied threshold keeps fewer than half
    flags = torch.from_numpy((rng.random(700) < 0.3).astype(np.uint8)).to(DEV)
    picked = P.select_device(P.to_device_cloud(p, DEV), flags=flags)
    assert np.array_equal(picked.numpy(), p[flags.cpu().numpy().astype(bool)])


@gpu
@pytest.mark.parametrize("fill", ["half", "none", "all"])
def test_select_device_behind_more_than_256_blocks(fill):
    """The last blocks of the compaction have more than 256 block sums in front of them (over 65 536 points): the second trip of the strided sum
    in their base offset.  The count is not a multiple of 256 and lies below the bound; flag bytes other than 0 and 1 count as set."""
    bound, n = 66013, 66001
    rng = np.random.default_rng(17)
    p = rng.uniform(-1, 1, (bound, 3)).astype(np.float32)
    flags = {"half": np.where(rng.random(bound) < 0.5, rng.integers(1, 256, bound), 0), "none": np.zeros(bound), "all": np.full(bound, 7)}[fill]
    flags = flags.astype(np.uint8)
    assert fill != "half" or (0.45 * n < np.count_nonzero(flags[:n]) < 0.55 * n and flags.max() > 1 and flags[n:].any())
    cloud = P.DeviceCloud(torch.from_numpy(p).to(DEV), torch.tensor([n], dtype=torch.int32, device=DEV))
    assert cloud.bound == bound
    picked = P.select_device(cloud, flags=torch.from_numpy(flags).to(DEV))
    want = p[:n][flags[:n] != 0]
    assert len(want) == {"half": len(want), "none": 0, "all": n}[fill]
    assert torch.equal(picked.count.cpu(), torch.tensor([len(want)], dtype=torch.int32))
    assert torch.equal(picked.pts[:len(want)].cpu(), torch.from_numpy(want))


@gpu
def test_tabletop_end_to_end_device():
    s = synth.tabletop_scene(2, 48, 64, seed=1, band=0.12)
    args = (s["depth"], s["R"], s["t"], s["intr"], s["bbox"])
    crop = P.depth_to_points_host(*args, s["masks"], 2)
    merged = P.voxel_down_sample_host(crop, P.VOXEL_SIZE)
    clean, it, _ = checked_host_denoise(merged)
    want = P.height_filter_host(clean, 0.8)
    assert 50 < len(want) < len(crop)
    # the chained host stages start from the DEVICE crop's coordinates where the two differ in the last place (they may, by one unit): the later
    # stages are then held to equality on identical inputs
    dev_crop = P.depth_to_points(*args, keep_masks=s["masks"], stride=2, device=DEV).numpy()
    assert dev_crop.shape == crop.shape and np.all(np.abs(dev_crop.astype(np.float64) - crop) <= np.spacing(np.abs(crop)))
    if not np.array_equal(dev_crop, crop):
        clean, it, _ = checked_host_denoise(P.voxel_down_sample_host(dev_crop, P.VOXEL_SIZE))
        want = P.height_filter_host(clean, 0.8)
    run = lambda: (lambda c: (c.pts[:c.size()], c.count))(P.get_tabletop_points(*args, keep_masks=s["masks"], stride=2, k_filter=0.8, device=DEV))
    got = same_bits_twice(run)[0].cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    # key points: the same indices as the host two-pass sampler on that cloud under one seed
    np.random.seed(11)
    state, kps, idx = P.state_from_depth(*args, keep_masks=s["masks"], stride=2, k_filter=0.8, sim_real_ratio=10.0, fps_radius=0.2, device=DEV,
                                         return_details=True)
    assert state.is_cuda and state.dtype == torch.float32 and state.shape == (len(idx), 3)
    host_kps = P.to_sim_frame(want, 10.0)
    assert np.array_equal(kps.cpu().numpy(), host_kps)
    np.random.seed(11)
    want_idx = sampling.fps(host_kps, 100, 0.2)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(state.cpu().numpy(), host_kps[want_idx]) and 3 <= len(want_idx) <= 100
