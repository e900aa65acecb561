"""The tabletop cloud kernels (csrc/ag_tabletop.hip) at the sizes and grids tests/test_tabletop_cloud.py does not reach: more brute-force points
than brute_kernel has workgroups, more than 65 536 points behind every producer of the compaction's block sums, more grid cells than the
single-block scan has threads, degenerate bounding boxes, device counts that are not the bound, the top corner of the voxel key space, one voxel
of 66 001 members, and a small cloud in scratch a large one has used.  The reference is the host statement of adaptigraph_amd/perception.py and
the tolerances are those of test_tabletop_cloud.py.  The conditions on the inputs (margins, kept shares, key values, grid sizes) are host-only
tests of their own, so a session without a GPU checks them too; the device tests repeat the ones their comparison rests on."""
import ctypes

import numpy as np
import pytest
import torch

from adaptigraph_amd import _lib, perception as P
from test_tabletop_cloud import BIG_BOX, DEV, EYE, ZERO, cameras, curve_cloud, margin, same_bits_twice, uniform_cloud

gpu = pytest.mark.gpu
K_BRUTE_BLOCKS, K_WIDE, SCAN_ROWS = 2048, 1024, 256            # kBruteBlocks, kWide of ag_tabletop.hip; kScanRows of ag_block_dev.h

_CACHE = {}


def once(key, fn):
    """A host reference is computed once per session and shared (nothing writes to it)."""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def host_mask(name, p, ratio=2.0, accelerate=True):
    def compute():
        avg = P.knn_mean_host(p, 20, accelerate=accelerate)
        thr = P.outlier_threshold_host(avg, len(p), ratio)[2] if len(p) > 1 else 0.0
        return (avg > 0) & (avg < thr) & (len(p) > 1), avg, float(thr)
    return once(("mask", name, ratio), compute)


# ------------------------------------------------------------------------------------------------------ device plumbing
def padded(p, bound, filler=None):
    """`p` in the first rows of a (bound, 3) fp32 array.  Behind them: NaN rows alternating with copies of real rows (`filler`, default `p`) —
    a NaN shows in a bounding box, a voxel key or a mean; a copy shows among the neighbours, the voxel members and the kept rows."""
    out = np.full((bound, 3), np.nan, np.float32)
    out[:len(p)] = p
    src = p if filler is None else filler
    for r in range(len(p) + 1, bound, 2):
        out[r] = src[(r * 7) % len(src)]
    return out


def device_cloud(rows, count):
    """A cloud whose count the host does not know: launches are sized by the rows, the kernels read `count`."""
    return P.DeviceCloud(torch.from_numpy(np.ascontiguousarray(rows, np.float32)).to(DEV), torch.tensor([count], dtype=torch.int32, device=DEV))


def knn_direct(cloud, k):
    """ag_cloud_knn_mean itself, with `avg` NaN before the call -> (avg (bound,), info (2,)) on the host."""
    dev = cloud.pts.device
    bound = int(cloud.pts.shape[0])
    avg = torch.full((bound,), float("nan"), dtype=torch.float64, device=dev)
    info = torch.full((2,), -7, dtype=torch.int32, device=dev)
    ws, nbytes = P._scratch(dev, bound)
    _lib.call("ag_cloud_knn_mean", dev, cloud.pts, cloud.count, bound, int(k), avg, info, ws, nbytes)
    return avg.cpu().numpy(), [int(v) for v in info.cpu()]


def assert_avg(got, want):
    assert not np.isnan(got).any()
    assert np.array_equal(got == 0, want == 0)
    assert np.all(np.abs(got - want) <= 1e-14 * want), float(np.max(np.abs(got - want) / np.maximum(want, 1e-300)))


def assert_mask_device(p, want, ratio=2.0):
    keep, avg, thr = want
    n = len(p)
    got_keep, got_avg, got_thr = same_bits_twice(lambda: P.statistical_outlier_mask(p, 20, ratio, device=DEV))
    got_keep, got_avg, got_thr = got_keep.cpu().numpy().astype(bool)[:n], got_avg.cpu().numpy()[:n], float(got_thr)
    assert_avg(got_avg, avg)
    assert np.array_equal(got_keep, keep)
    assert np.array_equal((got_avg > 0) & (got_avg < got_thr), keep)
    assert abs(got_thr - thr) <= 1e-12 * abs(thr)


# ------------------------------------------------------------------------------------------------------ A: more than 2 048 brute-force points
def halo_and_blob():
    """A dense blob sets the cell edge; the sparse halo around it finds no 20th neighbour within three rings of such cells."""
    def make():
        rng = np.random.default_rng(1)
        halo = rng.uniform(0, 1, (2600, 3)) * [1, 1, 0.01]
        blob = rng.uniform(0, 1, (40000, 3)) * 0.01 + [0.5, 0.5, 0]
        return np.concatenate([halo, blob])[rng.permutation(42600)].astype(np.float32)
    return once("halo", make)


def test_halo_and_blob_input_conditions():
    p = halo_and_blob()
    keep, avg, thr = host_mask("halo", p)
    assert margin(avg, thr) >= 1e-9, margin(avg, thr)
    assert 0.9 * len(p) < keep.sum() < len(p) and (avg > 0).all()
    # the halo is what the grid cannot resolve: outside the blob's box grown by its own edge there are more points than brute_kernel has workgroups
    outside = np.any((p < np.float32([0.49, 0.49, -0.01])) | (p > np.float32([0.52, 0.52, 0.02])), axis=1)
    assert outside.sum() > K_BRUTE_BLOCKS + 400


@gpu
def test_brute_kernel_takes_a_second_trip_and_the_scan_many_cells():
    """Gap 1 (brute_kernel's grid-stride loop: `info[0] > 2048` listed points on 2 048 workgroups, every one of them compared with the host and
    none left at the NaN the buffer held before) and gap 3 (cell_scan_kernel with `per > 1`: `info[1] > 1024` cells).  Predicted from a numpy
    restatement of the grid rule: 2 595 brute-force points, 174 x 174 x 2 = 60 552 cells; the device reported [2595, 60552]."""
    p = halo_and_blob()
    n, bound = len(p), len(p) + 300
    keep, avg, thr = host_mask("halo", p)
    assert margin(avg, thr) >= 1e-9
    cloud = device_cloud(padded(p, bound), n)
    got, (brute, cells) = knn_direct(cloud, 20)
    print("halo_and_blob info", [brute, cells])
    assert brute > K_BRUTE_BLOCKS and cells > K_WIDE, (brute, cells)
    assert_avg(got[:n], avg)
    assert np.isnan(got[n:]).all()                       # nothing behind the count was written
    again, info2 = knn_direct(cloud, 20)
    assert np.array_equal(again[:n], got[:n]) and info2 == [brute, cells]
    assert_mask_device(p, (keep, avg, thr))
    for k in (1, 5):                                      # fewer neighbours than the lists hold, on both kernels
        small, (brute_k, _) = knn_direct(cloud, k)
        assert_avg(small[:n], once(("halo_k", k), lambda: P.knn_mean_host(p, k)))
        assert np.isnan(small[n:]).all() and 0 <= brute_k <= brute


# ------------------------------------------------------------------------------------------------------ B: above 65 536 points through every stage
SHEET_N = 66001


def sheet():
    return once("sheet", lambda: (np.random.default_rng(2).uniform(0, 1, (SHEET_N, 3)) * [0.4, 0.3, 0.002]).astype(np.float32))


def test_sheet_input_conditions():
    p = sheet()
    assert len(p) > 256 * SCAN_ROWS                    # block_offset's second strided trip: more than 256 block sums in front of the last blocks
    keep, avg, thr = host_mask("sheet", p)
    assert margin(avg, thr) >= 1e-9, margin(avg, thr)
    assert keep.sum() == 64036
    assert len(np.unique(p, axis=0)) == len(p)         # distinct rows: equal rows = equal surviving indices
    fine = once("sheet_fine", lambda: P.voxel_down_sample_host(p, 0.0005))
    assert 256 * SCAN_ROWS - 512 < len(fine) < len(p)
    assert len(P.voxel_down_sample_host(p, 10.0)) == 1 and np.array_equal(P.voxel_down_sample_host(p, 1e-6), p)
    assert P.voxel_keys_host(p, 1e-6).max() < P.VOXEL_KEY_LIMIT
    assert [len(P.height_filter_host(p, k)) for k in (0.5, 0.999)] == [33000, 65934]


@gpu
@pytest.mark.parametrize("voxel", [0.0005, 10.0, 1e-6])
def test_sheet_voxel_merge(voxel):
    """Gap 2 behind voxel_mean_kernel + flag_sums_kernel (66 001 flags; at 0.0005 and 1e-6 the output is above 65 536 - 512 rows as well) and
    gap 7: at 10.0 one thread walks one run of 66 001 members, and the row must be the host's in-order float64 mean, bit for bit."""
    p = sheet()
    want = P.voxel_down_sample_host(p, voxel)
    assert len(want) == {0.0005: 65025, 10.0: 1, 1e-6: SHEET_N}[voxel]
    if voxel == 10.0:
        s = np.zeros(3)
        for row in p.astype(np.float64):                 # the contract said once more, by hand: members in ascending index
            s = s + row
        assert np.array_equal(want, (s / len(p)).astype(np.float32)[None])
    run = lambda: (lambda c: (c.pts[:c.size()], c.count))(P.voxel_down_sample(p, voxel, device=DEV))
    got, count = same_bits_twice(run)
    assert int(count.item()) == len(want)
    assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want)


@gpu
def test_sheet_outlier_mask_and_filter():
    """Gap 2 behind outlier_flag_kernel's store_flag, with outlier_stats_kernel and bounds_kernel at 65 trips per thread and cell_scan_kernel
    at more than one cell per thread (`info[1] > 1024`).  One mask iteration; the host loop would be the slow part."""
    p = sheet()
    keep, avg, thr = host_mask("sheet", p)
    assert margin(avg, thr) >= 1e-9
    assert_mask_device(p, (keep, avg, thr))
    cloud = P.to_device_cloud(p, DEV)

    def one_iteration():
        dev_avg, info = P.knn_mean_device(cloud, 20)
        kept, dev_keep, stats, progress = P.outlier_filter_device(cloud, dev_avg, 2.0)
        return kept.pts[:int(keep.sum())], kept.count, dev_keep, stats, progress, info

    rows, count, dev_keep, stats, progress, info = same_bits_twice(one_iteration)
    assert int(info[1]) > K_WIDE and 0 <= int(info[0]) <= len(p)
    assert int(count.item()) == int(progress.item()) == int(keep.sum()) == 64036
    assert np.array_equal(dev_keep.cpu().numpy().astype(bool), keep)
    assert np.array_equal(rows.cpu().numpy(), p[keep])


@gpu
@pytest.mark.parametrize("k_filter", [0.5, 0.999])
def test_sheet_height_filter(k_filter):
    """Gap 2 behind below_flag_kernel's store_flag."""
    p = sheet()
    want = P.height_filter_host(p, k_filter)
    assert 0 < len(want) < len(p)
    run = lambda: (lambda c: (c.pts[:c.size()], c.count))(P.height_filter(p, k_filter, device=DEV))
    got, count = same_bits_twice(run)
    assert int(count.item()) == len(want) and np.array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------------ C: depth images
CROP = np.array([[-0.6, 0.9], [-0.7, 0.8], [-1.0, 0.75]])
LO, HI = 0.0, 2.0


def big_images():
    return once("images", lambda: cameras(np.random.default_rng(0), 2, 150, 221))


def depth_limit_condition(depth):
    for d in depth:
        f = d[np.isfinite(d) & (d != 0)].astype(np.float64)
        assert np.all(np.abs(f - HI) > 1e-9 * HI) and np.all(np.abs(f - LO) > 1e-9)


def depth_conditions(depth, R, t, K, masks, stride):
    """test_depth_to_points_device's conditions: nothing within 1e-9 of a depth limit (exact zeros aside) or within 1e-6 of a crop plane; the crop
    keeps between 10 % and 90 %.  -> the host's points."""
    depth_limit_condition(depth)
    everything = P.depth_to_points_host(depth, R, t, K, BIG_BOX, masks, stride, (LO, HI)).astype(np.float64)
    for a in range(3):
        for plane in CROP[a]:
            assert np.all(np.abs(everything[:, a] - plane) > 1e-6 * max(1.0, abs(plane)))
    want = P.depth_to_points_host(depth, R, t, K, CROP, masks, stride, (LO, HI))
    assert 0.1 * len(everything) < len(want) < 0.9 * len(everything)
    return want


@pytest.mark.parametrize("masked", [True, False])
def test_big_images_input_conditions(masked):
    depth, R, t, K, masks = big_images()
    assert len(depth) * depth[0].size > 256 * SCAN_ROWS
    want = once(("images", masked), lambda: depth_conditions(depth, R, t, K, masks if masked else None, 1))
    assert len(want) > 1000


def assert_points(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)))


@gpu
@pytest.mark.parametrize("masked", [True, False])
def test_depth_to_points_above_65536_pixels(masked):
    """Gap 2 behind depth_points_kernel's store_flag: 2 x 150 x 221 = 66 300 strided pixels, 259 block sums."""
    depth, R, t, K, masks = big_images()
    m = masks if masked else None
    want = once(("images", masked), lambda: depth_conditions(depth, R, t, K, m, 1))
    run = lambda: (lambda c: (c.pts[:c.size()], c.count))(P.depth_to_points(depth, R, t, K, CROP, m, 1, (LO, HI), device=DEV))
    got, count = same_bits_twice(run)
    assert int(count.item()) == len(want)
    assert_points(got.cpu().numpy(), want)


@gpu
def test_depth_to_points_small_corners():
    """One-pixel images, a stride beyond both sizes, and mask bytes other than 0 and 1 (given to ag_depth_cloud itself: the Python path turns
    masks into booleans first)."""
    one = [np.float32([[0.5]]), np.float32([[np.nan]]), np.float32([[1.0]]), np.float32([[2.0]])]            # kept, NaN, kept, d == hi (strict)
    cams = ([EYE] * 4, [ZERO, ZERO, np.array([0.25, 0, 0]), ZERO], [EYE] * 4)
    want = P.depth_to_points_host(one, *cams, BIG_BOX, None, 1, (LO, HI))
    assert np.array_equal(want, np.float32([[0, 0, 0.5], [0.25, 0, 1.0]]))
    for stride in (1, 4):
        got = P.depth_to_points(one, *cams, BIG_BOX, None, stride, (LO, HI), device=DEV)
        assert got.bound == 4 and np.array_equal(got.numpy(), want)
    assert np.array_equal(P.depth_to_points(one[:1], [EYE], [ZERO], [EYE], BIG_BOX, [np.zeros((1, 1), bool)], 1, (LO, HI), device=DEV).numpy(),
                          np.zeros((0, 3), np.float32))
    rng = np.random.default_rng(5)
    depth, R, t, K, masks = cameras(rng, 3, 5, 7)
    for d in depth:
        d[0, 0] = rng.uniform(0.5, 1.5)                   # the one pixel a stride of 9 reads
    depth_limit_condition(depth)
    want = P.depth_to_points_host(depth, R, t, K, BIG_BOX, None, 9, (LO, HI))
    got =P.depth_to_points(depth, R, t, K, BIG_BOX, None, 9, (LO, HI), device=DEV)
    assert got.bound == 3 and len(want) == 3
    assert_points(got.numpy(), want)
    # mask bytes: any non-zero byte allows the pixel
    C, H, W = 2, 33, 47
    depth, R, t, K, _ = cameras(rng, C, H, W)
    mask = np.where(rng.random((C, H, W)) < 0.7, rng.integers(1, 256, (C, H, W)), 0).astype(np.uint8)
    assert mask.max() > 1 and (mask == 0).any()
    depth_limit_condition(depth)
    want = P.depth_to_points_host(depth, R, t, K, BIG_BOX, list(mask != 0), 1, (LO, HI))
    unmasked = P.depth_to_points_host(depth, R, t, K, BIG_BOX, None, 1, (LO, HI))
    assert 0.5 * len(unmasked) < len(want) < 0.9 * len(unmasked)
    dev = torch.device(DEV)
    cap = C * H * W
    pts = torch.full((cap, 3), float("nan"), dtype=torch.float32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws, nbytes = P._scratch(dev, cap)
    limits = np.concatenate([[LO, HI], BIG_BOX.reshape(6)])
    _lib.call("ag_depth_cloud", dev, torch.from_numpy(np.stack(depth)).to(dev), torch.from_numpy(mask).to(dev),
              torch.from_numpy(P._camera_rows(R, t, K)).to(dev), torch.from_numpy(limits).to(dev), C, H, W, 1, pts, count, ws, nbytes)
    assert int(count.item()) == len(want)
    assert_points(pts[:len(want)].cpu().numpy(), want)
    assert torch.isnan(pts[len(want):]).all()


# ------------------------------------------------------------------------------------------------------ D: degenerate boxes
def degenerate_clouds():
    def make():
        rng = np.random.default_rng(11)
        line = np.stack([rng.uniform(0, 0.5, 400), np.full(400, 0.25), np.full(400, -0.5)], 1).astype(np.float32)
        dup = line.copy()
        dup[100:125] = dup[7]                             # 25 copies of one point (with the original: 26, more than the 20 neighbours)
        plane = np.stack([rng.uniform(0, 0.5, 500), rng.uniform(0, 0.25, 500), np.full(500, 0.125)], 1).astype(np.float32)
        # a box of 1e30 x 1e-40 x 0 (fp32 subnormals in y): spread along x, and a bulk of order 1e-40 with one point at x = 1e30
        spread = np.stack([rng.uniform(0, 1, 400) * 1e30, rng.uniform(0, 1, 400) * 1e-40, np.zeros(400)], 1).astype(np.float32)
        bulk = np.stack([rng.uniform(0, 1, 499) * 1e-40, rng.uniform(0, 1, 499) * 1e-40, np.zeros(499)], 1)
        far = np.concatenate([bulk[:250], [[1e30, 0.5e-40, 0.0]], bulk[250:]]).astype(np.float32)
        return {"line": line, "line_duplicates": dup, "plane": plane, "thin_spread": spread, "thin_far": far}
    return once("degenerate", make)


DEGENERATE = ("line", "line_duplicates", "plane", "thin_spread", "thin_far")


def restated_grid(p32):
    """choose_grid, fit_grid and the two rounds of grid_refine_kernel said in numpy float64, for a box with e3 = 0 (no cube root to agree on)
    -> (e2 as the kernel computes it, the first guess's edge / e1, its dims, the final dims, whether a refine round changed the grid)."""
    p = p32.astype(np.float64)
    n = len(p)
    nc_max = 64
    while nc_max < 4 * n and nc_max < 1 << 20:
        nc_max *= 2
    o, e = p.min(0), p.max(0) - p.min(0)
    e1, e3 = e.max(), e.min()
    e2 = max(0.0, (e[0] + e[1] + e[2]) - e1 - e3)
    assert e3 == 0.0

    def fit(h):
        for _ in range(256):
            dims = np.floor(e / h) + 1.0
            if dims[0] * dims[1] * dims[2] <= nc_max:
                return h, dims.astype(np.int64)
            h *= 1.25
        return 2.0 * e1 + 1.0, np.ones(3, np.int64)

    per = 8.0 / n
    h = np.sqrt(per * e1 * e2)
    if not h > 0:
        h = per * e1
    if not h > 0:
        h = 1.0
    h, dims = fit(h)
    first_h, first, refined = h, dims, False
    for _ in range(2):
        cell = np.clip(np.floor((p - o) / h), 0, dims - 1).astype(np.int64)
        occupied = len(np.unique(cell, axis=0))
        if n > 1.5 * 8.0 * occupied:
            new_h, new_dims = fit(h * np.sqrt(8.0 * occupied / n))
            if new_h < h:
                h, dims, refined = new_h, new_dims, True
    return e2, first_h / e1, first, dims, refined


@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_input_conditions(name):
    p = degenerate_clouds()[name]
    extent = p.max(0).astype(np.float64) - p.min(0)
    assert 300 <= len(p) <= 600
    keep, avg, thr = host_mask(name, p, accelerate=False)
    assert margin(avg, thr) >= 1e-9, margin(avg, thr)
    assert 0 < keep.sum() < len(p)
    e2, h_over_e1, first, dims, refined = restated_grid(p)
    if name.startswith("line"):
        assert extent[1] == extent[2] == 0 and extent[0] > 0            # e2 = e3 = 0 exactly: sqrt and cbrt give 0, the edge is per * e1
        assert e2 == 0 and h_over_e1 == 8.0 / len(p) and list(first) == [len(p) // 8 + 1, 1, 1] and not refined
        assert (avg == 0).sum() == (26 if name == "line_duplicates" else 0)
    if name == "plane":
        assert extent[2] == 0 and extent[0] > 0 and extent[1] > 0 and e2 == extent[1]
        assert first[0] > 1 and first[1] > 1 and first[2] == 1 and not refined
    if name.startswith("thin"):
        # the middle extent is below half a unit in the last place of the largest, so choose_grid's e2 = (e0 + e1 + e2) - e1 - e3 is 0 and the
        # edge is per * e1 although the box is no line
        assert extent[0] > 0.9e30 and 0 < extent[1] < 1.01e-40 and extent[2] == 0 and e2 == 0 and h_over_e1 == 8.0 / len(p)
        assert refined == (name == "thin_far") and (name == "thin_far" or len(np.unique(p[:, 0])) == len(p))
        assert name != "thin_far" or (p[:, 0] > 1).sum() == 1


@gpu
@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_boxes(name):
    """Gap 4.  The line takes choose_grid's `h = per * e1` (its box has e2 = e3 = 0 exactly, and `info[1]` is the n / 8 + 1 cells that edge gives)
    and the plane has e3 = 0.  The two thin clouds have a box of 1e30 x 1e-40 x 0.  A restatement that takes the middle extent as it is predicts
    for `thin_far` that fit_grid's 256 growth trips run out, the one-cell fallback, and 23 cells with one brute-force point after the refine
    rounds.  The kernel does not go that way: its e2 = (e0 + e1 + e2) - e1 - e3 loses an extent below half a unit in the last place of e1, so
    it takes `h = per * e1` again (restated_grid, which the cell counts below are held to).  An e2 that survives the subtraction is at least
    1e-16 e1, the first edge then at least 1e-11 e1, and 1.25^256 = 6e24 covers that: no finite box reaches the one-cell fallback.
    The device reported info = [brute, cells]: line [3, 51], line_duplicates [2, 51], plane [0, 72], thin_spread [0, 51], thin_far [1, 1954]
    (thin_far: 63 cells at first, two refine rounds from its 2 occupied cells, as restated_grid says)."""
    p = degenerate_clouds()[name]
    n = len(p)
    want = host_mask(name, p, accelerate=False)
    assert margin(want[1], want[2]) >= 1e-9
    got, (brute, cells) = knn_direct(device_cloud(p, n), 20)
    print("degenerate info", name, [brute, cells])
    assert_avg(got, want[1])
    assert 0 <= brute <= n and cells >= 1
    assert cells == int(restated_grid(p)[3].prod())
    assert_mask_device(p, want)


# ------------------------------------------------------------------------------------------------------ E: counts
CUTS = (1, 255, 256, 257, 700)
CUT_BOUND = 768                  # three blocks: behind a cut the last block is empty, and the one the cut falls in full (256) or partial
CUT_VOXEL = 0.2


def cut_cloud():
    return once("cut", lambda: uniform_cloud(23, 700))


@pytest.mark.parametrize("n", CUTS)
def test_cut_input_conditions(n):
    p = cut_cloud()[:n]
    keep, avg, thr = host_mask(("cut", n), p, accelerate=False)
    assert margin(avg, thr) >= 1e-9, margin(avg, thr)
    assert n < 3 or 0 < keep.sum() < n
    assert n < 255 or len(P.voxel_down_sample_host(p, CUT_VOXEL)) < 0.7 * n            # voxels of several members


def entry_points(cloud, avg, flags, z):
    """Every entry point that takes a count, on one cloud -> host values."""
    merged = P.voxel_down_sample_device(cloud, CUT_VOXEL)
    kept, keep, stats, progress = P.outlier_filter_device(cloud, avg, 2.0)
    by_flag, by_z = P.select_device(cloud, flags=flags), P.select_device(cloud, z_below=z)
    return {"merged": merged.numpy(), "kept": kept.numpy(), "keep": keep.cpu().numpy(), "stats": stats.cpu().numpy(), "progress": int(progress.item()),
            "by_flag": by_flag.numpy(), "by_z": by_z.numpy()}


@gpu
@pytest.mark.parametrize("n", CUTS)
def test_count_below_the_bound_at_every_entry_point(n):
    """Gap 5: rows behind the count are NaN or copies of real rows, and (for the filter and the selections) the words behind it would be kept
    if a stage read them.  Every result is that of the cloud cut to its count."""
    p = cut_cloud()[:n]
    keep, avg, thr = host_mask(("cut", n), p, accelerate=False)
    assert margin(avg, thr) >= 1e-9
    cloud = device_cloud(padded(p, CUT_BOUND, cut_cloud()), n)
    assert cloud.bound == CUT_BOUND and torch.isnan(cloud.pts[n:]).any() and torch.isfinite(cloud.pts[n:]).any()
    got_avg, (brute, cells) = knn_direct(cloud, 20)
    assert_avg(got_avg[:n], avg)
    assert np.isnan(got_avg[n:]).all() and 0 <= brute <= n and cells >= 1
    rng = np.random.default_rng(n)
    avg_in = got_avg.copy()
    avg_in[n:] = np.median(avg) if n > 1 else 1.0          # behind the count: values the threshold would keep, and the statistics count
    flags = np.where(rng.random(CUT_BOUND) < 0.5, rng.integers(1, 256, CUT_BOUND), 0).astype(np.uint8)
    flags[n:] = 9
    z = np.float32(0.5)
    got = entry_points(cloud, torch.from_numpy(avg_in).to(DEV), torch.from_numpy(flags).to(DEV), torch.tensor([z], dtype=torch.float32, device=DEV))
    cut = entry_points(P.to_device_cloud(p, DEV), torch.from_numpy(avg_in[:n].copy()).to(DEV), torch.from_numpy(flags[:n].copy()).to(DEV),
                       torch.tensor([z], dtype=torch.float32, device=DEV))
    assert np.array_equal(got["merged"], P.voxel_down_sample_host(p, CUT_VOXEL))
    assert np.array_equal(got["kept"], p[keep]) and np.array_equal(got["keep"][:n].astype(bool), keep) and not got["keep"][n:].any()
    assert got["progress"] == (int(keep.sum()) if keep.sum() < n else ~n)
    assert abs(got["stats"][2] - thr) <= 1e-12 * abs(thr)
    assert np.array_equal(got["by_flag"], p[flags[:n] != 0]) and np.array_equal(got["by_z"], p[p[:, 2] < z])
    for name in got:                                     # and the bits of the same call on the cut cloud
        assert np.array_equal(got[name][:n] if name == "keep" else got[name], cut[name]), name


@gpu
@pytest.mark.parametrize("count", [-5, CUT_BOUND + 100])
def test_count_outside_zero_to_the_bound(count):
    """Gap 5, cloud_count's clamp: a negative count is an empty cloud at every entry point, a count above the bound is the bound."""
    rng = np.random.default_rng(3)
    p = np.concatenate([cut_cloud(), uniform_cloud(29, CUT_BOUND - 700)])
    cloud = device_cloud(p, count)
    flags = torch.from_numpy(np.where(rng.random(CUT_BOUND) < 0.5, 3, 0).astype(np.uint8)).to(DEV)
    z = torch.tensor([0.5], dtype=torch.float32, device=DEV)
    got_avg, (brute, cells) = knn_direct(cloud, 20)
    if count < 0:
        assert np.isnan(got_avg).all() and brute == 0 and cells >= 1
        got = entry_points(cloud, torch.full((CUT_BOUND,), 0.01, dtype=torch.float64, device=DEV), flags, z)
        assert got["progress"] == ~0 and not got["keep"].any()
        for name in ("merged", "kept", "by_flag", "by_z"):
            assert got[name].shape == (0, 3), name
        return
    keep, avg, thr = host_mask("cut_full", p, accelerate=False)
    assert margin(avg, thr) >= 1e-9
    assert_avg(got_avg, avg)
    dev_avg = torch.from_numpy(got_avg).to(DEV)
    got, full = entry_points(cloud, dev_avg, flags, z), entry_points(device_cloud(p, CUT_BOUND), dev_avg, flags, z)
    assert np.array_equal(got["merged"], P.voxel_down_sample_host(p, CUT_VOXEL)) and np.array_equal(got["kept"], p[keep])
    assert got["progress"] == int(keep.sum()) < CUT_BOUND
    assert np.array_equal(got["by_flag"], p[flags.cpu().numpy() != 0]) and np.array_equal(got["by_z"], p[p[:, 2] < np.float32(0.5)])
    for name in got:
        assert np.array_equal(got[name], full[name]), name


# ------------------------------------------------------------------------------------------------------ F: voxel key borders
TOP = 2.0 ** 20 - 0.75            # voxel 0.5, origin -0.25: key floor((TOP + 0.25) / 0.5) = 2^21 - 1, the last one the sort key holds
OVER = 2.0 ** 20 - 0.25           # key 2^21: refused


def corner_clouds():
    far, mate = np.float32([TOP] * 3), np.float32([2.0 ** 20 - 0.5] * 3)            # `mate` lies in the same voxel as `far`
    origin = np.zeros(3, np.float32)
    return {"origin_first": np.stack([origin, far]), "far_first": np.stack([far, origin]), "two_in_the_corner": np.stack([far, origin, mate, origin])}


def test_voxel_key_border_input_conditions():
    last = P.VOXEL_KEY_LIMIT - 1
    for name, p in corner_clouds().items():
        assert np.isin(p.astype(np.float64), [0.0, TOP, 2.0 ** 20 - 0.5]).all()            # exact in fp32
        keys = P.voxel_keys_host(p, 0.5)
        assert keys.max() == last and np.array_equal(keys[p[:, 0] > 0], np.full((int((p[:, 0] > 0).sum()), 3), last)), name
        assert (last * P.VOXEL_KEY_LIMIT + last) * P.VOXEL_KEY_LIMIT + last == 2 ** 63 - 1            # the key the rows behind the count get
    assert np.array_equal(P.voxel_down_sample_host(corner_clouds()["two_in_the_corner"], 0.5), np.float32([[2.0 ** 20 - 0.625] * 3, [0, 0, 0]]))
    for axis in range(3):
        wide = np.float32([[0, 0, 0], [TOP] * 3])
        wide[1, axis] = OVER
        keys = P.voxel_keys_host(wide, 0.5)
        assert float(wide[1, axis]) == OVER and keys[1, axis] == P.VOXEL_KEY_LIMIT and keys.max(0).tolist().count(last) == 2


@gpu
@pytest.mark.parametrize("name", ["origin_first", "far_first", "two_in_the_corner"])
def test_voxel_key_top_corner(name):
    """Gap 6: a real point with the key 2^63 - 1 is merged (status 0) and equals the host; with 50 NaN rows behind the count, which get the same
    key, only the stable sort and voxel_mean_kernel's `e < n` keep them out of that voxel."""
    p = corner_clouds()[name]
    want = P.voxel_down_sample_host(p, 0.5)
    assert len(want) == 2
    got = P.voxel_down_sample(p, 0.5, device=DEV)
    assert got.n == 2 and np.array_equal(got.numpy(), want)
    rows = np.full((len(p) + 50, 3), np.nan, np.float32)
    rows[:len(p)] = p
    cloud = device_cloud(rows, len(p))
    dev = cloud.pts.device
    bound = cloud.bound
    keys = torch.empty(bound, dtype=torch.int64, device=dev)
    out = torch.full((bound, 3), float("nan"), dtype=torch.float32, device=dev)
    words = torch.full((2,), -7, dtype=torch.int32, device=dev)            # [count, status]
    ws, nbytes = P._scratch(dev, bound)
    _lib.call("ag_cloud_voxel_keys", dev, cloud.pts, cloud.count, bound, ctypes.byref(ctypes.c_double(0.5)), keys, words[1:], ws, nbytes)
    host_keys = P.voxel_keys_host(p, 0.5)
    assert np.array_equal(keys[:len(p)].cpu().numpy(), (host_keys[:, 0] * P.VOXEL_KEY_LIMIT + host_keys[:, 1]) * P.VOXEL_KEY_LIMIT + host_keys[:, 2])
    assert (keys[len(p):] == 2 ** 63 - 1).all() and int(keys[:len(p)].max()) == 2 ** 63 - 1
    skeys, perm = torch.sort(keys, stable=True)
    _lib.call("ag_cloud_voxel_merge", dev, cloud.pts, cloud.count, bound, skeys, perm, out, words[:1], ws, nbytes)
    assert words.cpu().tolist() == [2, 0]
    assert np.array_equal(out[:2].cpu().numpy(), want) and torch.isnan(out[2:]).all()


@gpu
@pytest.mark.parametrize("axis", [None, 0, 1, 2])
def test_voxel_key_limit_is_refused(axis):
    """Gap 6, the refuse side of the border: key 2^21 on all three axes, or on one axis with 2^21 - 1 on the others."""
    p = np.float32([[0, 0, 0], [OVER if axis is None else TOP] * 3])
    if axis is not None:
        p[1, axis] = OVER
    with pytest.raises(ValueError, match="voxels"):
        P.voxel_down_sample(p, 0.5, device=DEV)
    with pytest.raises(ValueError, match="voxels"):
        P.voxel_down_sample(p[::-1].copy(), 0.5, device=DEV)


# ------------------------------------------------------------------------------------------------------ G: scratch reuse
@gpu
def test_small_clouds_after_a_large_one_in_the_same_scratch():
    """Gap 8: the grow-only scratch holds the 66 001-point sheet's cell_start, sorted, work, flags and sums behind a small cloud's extent; the
    small clouds' results are, bit for bit, what the same calls gave before, and the host's."""
    small = {"curve": curve_cloud(0), "tiny": uniform_cloud(21, 21)}
    big = P.to_device_cloud(sheet(), DEV)

    def run(p):
        cloud = P.to_device_cloud(p, DEV)
        avg, info = P.knn_mean_device(cloud, 20)
        kept, keep, stats, progress = P.outlier_filter_device(cloud, avg, 2.0)
        merged = P.voxel_down_sample_device(cloud, 0.004)
        return [avg, info, kept.tensor(), keep, stats, progress, merged.tensor(), merged.count]

    before = {name: run(p) for name, p in small.items()}
    dev = torch.device(DEV)
    big_avg, big_info = P.knn_mean_device(big, 20)
    big_merged = P.voxel_down_sample_device(big, 0.0005)
    assert int(big_info[1]) > K_WIDE and big_merged.n == 65025
    held = _lib.workspace(dev, 1)
    assert held.numel() >= _lib.lib().ag_tabletop_workspace_bytes(SHEET_N)            # the buffer the small clouds get now is the sheet's
    for name, p in small.items():
        after = run(p)
        assert _lib.workspace(dev, 1) is held
        assert all(torch.equal(a, b) for a, b in zip(before[name], after)), name
        keep, avg, thr = host_mask(("small", name), p, accelerate=False)
        assert margin(avg, thr) >= 1e-9
        assert_avg(after[0].cpu().numpy(), avg)
        assert np.array_equal(after[3].cpu().numpy().astype(bool), keep) and np.array_equal(after[2].cpu().numpy(), p[keep])
        assert np.array_equal(after[6].cpu().numpy(), P.voxel_down_sample_host(p, 0.004))
