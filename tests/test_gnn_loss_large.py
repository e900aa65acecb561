"""The matching losses where tests/test_gnn_loss.py stops: `ag_emd` in its two widest forms (8 columns per lane with every register slot
occupied, 16 columns per lane up to the limit) against tests/golden/gnn_loss_large.npz (scipy's assignments, `tools/gen_loss_golden.py large`),
costs that overflow fp32, `ag_emd_backward` beyond one trip of its strided loops, `ag_hausdorff` above 48 KB of dynamic LDS, and the value and
gradient of `gnn_loss.HausdorffLoss` / the masked modules against the formula of loss.py in float64.  Nothing here imports scipy or the reference."""
import functools
import itertools
import time

import numpy as np
import pytest
import torch

from conftest import load_golden
from adaptigraph_amd import _lib, gnn_loss, losses
from test_gnn_loss import (DEV, assert_within_one_ulp, case, check_hausdorff, cost_matrix, expected_value, inverse, ref_grads, run_emd, tg)

GAUSS = [(512, 512), (513, 300), (300, 513), (640, 1024), (1000, 1000), (1024, 1024)]
CHAINS = [(1024, 1024), (513, 1024)]
MASKED1024_COUNTS = [(700, 900), (0, 500), (3, 1024), (1024, 1), (513, 512)]
LIMIT = _lib.AG_EMD_MAX_POINTS


@functools.lru_cache(maxsize=None)
def large():
    return load_golden("gnn_loss_large")


def columns_per_lane(points):
    """The emd_kernel instantiation the launch picks for max(N, M) = points."""
    return next(c for c in (1, 2, 4, 8, 16) if points <= 64 * c)


# what every Gaussian case is in the fixture for, from its shape alone: a regenerated fixture cannot silently stop covering the class
PURPOSE = {
    "s512x512": lambda N, M: columns_per_lane(max(N, M)) == 8 and min(N, M) > 64 * 7,              # all eight slots of CPL = 8, rows and columns
    "s513x300": lambda N, M: columns_per_lane(max(N, M)) == 16 and max(N, M) == 513 and N > M,     # the first size of CPL = 16, rows on y
    "s300x513": lambda N, M: columns_per_lane(max(N, M)) == 16 and max(N, M) == 513 and N < M,     # ... rows on x
    "s640x1024": lambda N, M: M == LIMIT and 512 < N < M,                                          # all sixteen slots, rectangular
    "s1000x1000": lambda N, M: N == M == 1000,                                                     # the benchmarked shape of DESIGN.md §8.9
    "s1024x1024": lambda N, M: N == M == LIMIT,                                                    # the limit
}


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


@functools.lru_cache(maxsize=None)
def solved(name, broadcast):
    x, y, xm, ym, _ = case(name, broadcast, large())
    t0 = time.perf_counter()
    got = run_emd(x, y, xm, ym)
    print("emd", name, "broadcast" if broadcast else "batched", f"{1e3 * (time.perf_counter() - t0):.1f} ms with copies")
    return got


def check_forward(name, broadcast):
    """col, row, the value both ways, and the same bits on a second call -> (x, y, xm, ym, col, out, got_col, got_row)."""
    g = large()
    x, y, xm, ym, col = case(name, broadcast, g)
    assert int(g[name + "_unique"]) == 1
    out, got_col, got_row = solved(name, broadcast)
    assert torch.equal(torch.from_numpy(got_col), torch.from_numpy(col))
    assert torch.equal(torch.from_numpy(got_row), torch.from_numpy(inverse(col, y.shape[1])))
    assert_within_one_ulp(out, expected_value(x, y, col))
    total, K = g[name + ("_totalb" if broadcast else "_total")], (col >= 0).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        assert_within_one_ulp(out, (total / K).astype(np.float32))
    out2, col2, row2 = run_emd(x, y, xm, ym)
    assert np.array_equal(bits(out), bits(out2)) and np.array_equal(got_col, col2) and np.array_equal(got_row, row2)
    return x, y, xm, ym, col, out, got_col, got_row


# ------------------------------------------------------------------ 2: forward on the large fixture
@pytest.mark.gpu
@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("N,M", GAUSS)
def test_large_assignment_and_value(N, M, broadcast):
    """Gaussian clouds, B = 2: scipy's assignment index for index and the fp64 mean rounded once, in emd_kernel<8> with every slot occupied
    and in emd_kernel<16> from its first size to the limit."""
    name = f"s{N}x{M}"
    x, y, _, _, col, _, _, _ = check_forward(name, broadcast)
    assert x.shape == (2, N, 3) and y.shape == (1 if broadcast else 2, M, 3)
    assert PURPOSE[name](N, M)
    assert ((col >= 0).sum(1) == min(N, M)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("N,M", CHAINS)
def test_large_chain(N, M):
    """x_n = (n,0,0) descending, y_m = (m+0.4,0,0): every augmentation walks the chain built so far, through all sixteen register slots."""
    x, y, _, _, col, _, _, _ = check_forward(f"chain{N}x{M}", False)
    assert x.shape == (1, N, 3) and y.shape == (1, M, 3) and columns_per_lane(max(N, M)) == 16 and M == LIMIT
    assert np.array_equal(x[0, :, 0], np.arange(N, dtype=np.float32)[::-1]) and np.array_equal(y[0, :, 0], np.arange(M, dtype=np.float32) + np.float32(0.4))
    assert np.array_equal(col[0], np.arange(N)[::-1])                    # (the point at n is the one of coordinate N - 1 - n)


@pytest.mark.gpu
@pytest.mark.parametrize("broadcast", [False, True])
def test_masked1024(broadcast):
    """1024 slots a side under emd_kernel<16>, the valid points scattered: compaction over sixteen ballots a side, three rows in 1024 columns,
    one row, the rows on y, a valid count either side of 512, an empty side."""
    x, y, xm, ym, col, out, got_col, got_row = check_forward("masked1024", broadcast)
    assert x.shape == (5, LIMIT, 3) and y.shape == (1 if broadcast else 5, LIMIT, 3)
    assert [int(v) for v in xm.sum(1)] == [c[0] for c in MASKED1024_COUNTS]
    assert [int(v) for v in ym.sum(1)] == [c[1] for c in MASKED1024_COUNTS][:ym.shape[0]]
    for b in range(5):                                                    # scattered: the valid points are no prefix of the slots
        for m in (xm[b], ym[b if not broadcast else 0]):
            v = np.flatnonzero(m)
            assert len(v) in (0, LIMIT) or v[-1] >= len(v)
    assert np.isnan(out[1]) and (got_col[1] == -1).all() and (got_row[1] == -1).all() and np.isfinite(out[[0, 2, 3, 4]]).all()
    assert (got_col[xm == 0] == -1).all()
    assert (got_row[np.broadcast_to(ym, got_row.shape) == 0] == -1).all()
    want = [min(int(xm[b].sum()), int(ym[0 if broadcast else b].sum())) for b in range(5)]
    assert [int(v) for v in (got_col >= 0).sum(1)] == want and [int(v) for v in (got_row >= 0).sum(1)] == want


@pytest.mark.gpu
@pytest.mark.parametrize("broadcast", [False, True])
def test_few_valid_points_in_1024_slots(broadcast):
    """Rows and columns both few under emd_kernel<16>: the `masked_small` case of the small fixture (3 to 6 valid points a side, its optimum
    proved by brute force in test_gnn_loss_cpu.py) scattered over 1024 slots a side whose other points are masked out.  The pairs are the
    fixture's under the scattering, and the value has the bits of the 9 x 7 call."""
    g = load_golden("gnn_loss_cases")
    xs, ys, xms, yms = g["masked_small_x"], g["masked_small_y"], g["masked_small_xm"], g["masked_small_ym"]
    if broadcast:
        ys, yms = ys[:1], yms[:1]
    small_out, small_col, small_row = run_emd(xs, ys, xms, yms)
    if not broadcast:
        assert np.array_equal(small_col, g["masked_small_col"])
    rng = np.random.default_rng(61)
    px, py = np.sort(rng.permutation(LIMIT)[:xs.shape[1]]), np.sort(rng.permutation(LIMIT)[:ys.shape[1]])      # slot of every small point
    assert px[-1] >= 512 and py[-1] >= 512 and px[0] < 512 and py[0] < 512
    x, y = rng.standard_normal((3, LIMIT, 3)).astype(np.float32), rng.standard_normal((ys.shape[0], LIMIT, 3)).astype(np.float32)
    xm, ym = np.zeros((3, LIMIT), np.uint8), np.zeros((ys.shape[0], LIMIT), np.uint8)
    x[:, px], y[:, py], xm[:, px], ym[:, py] = xs, ys, xms, yms
    assert xm.sum(1).max() <= 6 and ym.sum(1).max() <= 6
    out, col, row = run_emd(x, y, xm, ym)
    want_col, want_row = np.full((3, LIMIT), -1, np.int32), np.full((3, LIMIT), -1, np.int32)
    want_col[:, px] = np.where(small_col >= 0, py[np.maximum(small_col, 0)], -1)
    want_row[:, py] = np.where(small_row >= 0, px[np.maximum(small_row, 0)], -1)
    assert (small_col >= 0).any(1).all() and np.array_equal(col, want_col) and np.array_equal(row, want_row)
    assert np.array_equal(bits(out), bits(small_out)) and np.isfinite(out).all()


# ------------------------------------------------------------------ 3: costs that overflow fp32
def small_clouds(seed, shape):
    return (np.round(np.random.default_rng(seed).standard_normal(shape) * 4096.0) / 4096.0).astype(np.float32)


@pytest.mark.gpu
def test_every_cost_overflowing_is_nan_and_alone():
    """Finite coordinates 4e38 apart: every pair cost of sample 1 is +inf, no finite path exists, the sample is NaN with -1 throughout and the
    other samples have the bits they have without it."""
    x, y = small_clouds(71, (3, 5, 3)), small_clouds(72, (3, 5, 3))
    x[1, :, 0], y[1, :, 0] = np.float32(-2e38), np.float32(2e38)
    assert np.isfinite(x).all() and np.isfinite(y).all()
    with np.errstate(over="ignore"):
        assert np.isposinf(cost_matrix(x[1], y[1])).all()
    out, col, row = run_emd(x, y)
    assert np.isnan(out[1]) and (col[1] == -1).all() and (row[1] == -1).all()
    out2, col2, row2 = run_emd(x[[0, 2]], y[[0, 2]])
    assert np.isfinite(out2).all() and (col2 >= 0).all()
    assert np.array_equal(bits(out[[0, 2]]), bits(out2)) and np.array_equal(col[[0, 2]], col2) and np.array_equal(row[[0, 2]], row2)
    xb, yb = np.concatenate([x, x[::-1]]), y[1:2]                         # the overflowing cloud as the broadcast y: every sample NaN
    with np.errstate(over="ignore"):
        assert all(np.isposinf(cost_matrix(xb[b], yb[0])).any(1).all() for b in range(6))
    out3, col3, row3 = run_emd(xb, yb)
    assert np.isnan(out3).all() and (col3 == -1).all() and (row3 == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("far", [0, 2, 3])
def test_an_unreachable_column_is_never_needed(far):
    """3 x 4 with one y point at 1e30: its column is all +inf and three finite columns remain, so the answer is that of the 3 x 3 problem
    without the point (and the brute-force optimum), the far point unmatched."""
    x, y3 = small_clouds(73, (1, 3, 3)), small_clouds(74, (1, 3, 3))
    keep = np.array([m for m in range(4) if m != far])
    y = np.zeros((1, 4, 3), np.float32)
    y[0, keep], y[0, far] = y3[0], np.float32([1e30, 0, 0])
    with np.errstate(over="ignore"):
        C = cost_matrix(x[0], y[0])
    assert np.isposinf(C[:, far]).all() and np.isfinite(C[:, keep]).all() and np.isfinite(y).all()
    out, col, row = run_emd(x, y)
    out3, col3, row3 = run_emd(x, y3)
    assert np.isfinite(out3).all() and np.array_equal(bits(out), bits(out3))
    assert np.array_equal(col[0], keep[col3[0]]) and np.array_equal(row[0, keep], row3[0]) and row[0, far] == -1
    totals = {p: sum(float(C[n, keep[p[n]]]) for n in range(3)) for p in itertools.permutations(range(3))}
    best = min(totals, key=totals.get)
    assert sorted(totals.values())[1] - totals[best] > 1e-3               # (the optimum is unique)
    assert np.array_equal(col3[0], np.array(best)) and out[0] == np.float32(totals[best] / 3)


# ------------------------------------------------------------------ 4: backward beyond one trip of the strided loops
@pytest.mark.gpu
@pytest.mark.parametrize("name,broadcast", [("s513x300", False), ("s513x300", True), ("s300x513", False), ("s300x513", True),
                                            ("masked1024", False), ("masked1024", True)])
def test_large_gradients_vs_float64_autograd(name, broadcast):
    """emd_bwd_kernel's loops `for (i = tid; i < Q; i += 256)` at Q = 300 (two trips, the second partial), 513 (three) and 1024 (four, full),
    with unmatched points on either side; the check and the bound of test_gradients_vs_float64_autograd."""
    x, y, xm, ym, col = case(name, broadcast, large())
    assert max(x.shape[1], y.shape[1]) > 2 * 256 and min(x.shape[1], y.shape[1]) > 256
    w = np.random.default_rng(3).uniform(0.5, 2.0, x.shape[0])
    rx, ry = ref_grads(x, y, col, w)
    X, Y = tg(x).requires_grad_(), tg(y).requires_grad_()
    masks = (None if xm is None else tg(xm), None if ym is None else tg(ym))
    out, got_col, got_row = losses.emd(X, Y, *masks, return_assignment=True)
    with torch.no_grad():
        plain = losses.emd(X, Y, *masks)
    assert torch.equal(out.detach().view(torch.int32), plain.view(torch.int32))      # the same value bits with and without grad
    assert torch.equal(got_col.cpu(), torch.from_numpy(col))
    gx, gy = torch.autograd.grad(out, [X, Y], grad_outputs=tg(w.astype(np.float32)))
    gx, gy, row = gx.cpu().numpy(), gy.cpu().numpy(), got_row.cpu().numpy()
    for label, got, ref in (("gx", gx, rx), ("gy", gy, ry)):
        assert got.shape == ref.shape
        err, scale = np.abs(got - ref).max(), np.abs(ref).max()
        print("emd", label, name, "broadcast" if broadcast else "batched", "max abs error", err, "of", scale)
        assert err <= 1e-5 * scale + 1e-12
    unmatched_x, unmatched_y = col < 0, (row < 0).all(0, keepdims=True) if broadcast else row < 0
    assert (unmatched_x.any() or x.shape[1] < y.shape[1]) and (unmatched_y.any() or x.shape[1] > y.shape[1])      # the larger side has some
    assert (gx[unmatched_x] == 0).all() and (gy[unmatched_y] == 0).all()             # exactly 0 on unmatched and masked points
    if xm is not None:
        assert (gx[xm == 0] == 0).all() and (gy[ym == 0] == 0).all() and (gx[1] == 0).all()


# ------------------------------------------------------------------ 5: hausdorff above 48 KB of LDS
@pytest.mark.gpu
@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("B,N,M,masked", [(2, 3000, 1200, False), (2, 6399, 6401, False), (3, 5000, 4100, True)])
def test_hausdorff_with_more_than_48_kb_of_lds(B, N, M, masked, broadcast):
    """Both clouds in dynamic LDS past the 48 KB a kernel gets without asking, up to the limit N + M = 12 800 with odd sizes; the values and
    indices are the bits of the formula in numpy, evaluated block by block."""
    assert 3 * (N + M) * 4 > 48 * 1024 and N + M <= 12800
    rng = np.random.default_rng(1000 + N)
    x, y = rng.standard_normal((B, N, 3)).astype(np.float32), rng.standard_normal((B, M, 3)).astype(np.float32)
    xm = ym = None
    if masked:
        xm, ym = (rng.random((B, N)) < 0.7).astype(np.uint8), (rng.random((B, M)) < 0.7).astype(np.uint8)
        xm[1] = 0                                                         # an empty side
        assert 0.65 < xm[[0, 2]].mean() < 0.75 and 0.65 < ym.mean() < 0.75
    yy, yym = (y[:1], None if ym is None else ym[:1]) if broadcast else (y, ym)
    t0 = time.perf_counter()
    val, arg = check_hausdorff(x, yy, xm, yym)
    print("hausdorff", (B, N, M), "broadcast" if broadcast else "batched", f"{time.perf_counter() - t0:.2f} s with the numpy reference")
    val2, arg2 = losses.hausdorff(tg(x), tg(yy), None if xm is None else tg(xm), None if yym is None else tg(yym))
    assert torch.equal(val.view(torch.int32), val2.view(torch.int32)) and torch.equal(arg, arg2)
    if masked:
        assert torch.isnan(val[1]).all() and (arg[1] == -1).all() and torch.isfinite(val[[0, 2]]).all()
        a = arg.cpu().numpy()
        for b in (0, 2):
            assert xm[b, a[b, [0, 3]]].all() and yym[0 if broadcast else b, a[b, [1, 2]]].all()
    else:
        assert torch.isfinite(val).all()


# ------------------------------------------------------------------ 6: the modules against float64
def valid(mask, b, count):
    return np.arange(count) if mask is None else np.flatnonzero(mask[b if mask.shape[0] > 1 else 0])


def hausdorff_loss_f64(pred, label, xm=None, ym=None):
    """loss.py:67-77 in float64 torch with masked points removed per sample: dis = ||x - y||, max over the batch of max_n min_m plus max over
    the batch of max_m min_n; a sample with an empty side takes no part.  -> (loss, grad pred, grad label, winning sample per direction), NaN and
    None when no sample has two valid sides.  Asserts that the arg-max is well defined: per direction the two largest nearest-neighbour
    distances of the batch, and the two smallest distances at the winning point, differ by more than 1e-3."""
    B = pred.shape[0]
    P, L = torch.from_numpy(pred).double().requires_grad_(), torch.from_numpy(label).double().requires_grad_()
    mins, owner, dis = ([], []), ([], []), {}
    for b in range(B):
        lb = b if label.shape[0] == B else 0
        vx, vy = valid(xm, b, pred.shape[1]), valid(ym, lb, label.shape[1])
        if len(vx) == 0 or len(vy) == 0:
            continue
        d = torch.norm(P[b][vx][:, None, :] - L[lb][vy][None, :, :], 2, dim=2)
        dis[b] = d.detach()
        for k, axis in ((0, 1), (1, 0)):
            mins[k].append(d.min(axis)[0])
            owner[k].extend((b, i) for i in range(d.shape[k]))
    if not dis:
        return float("nan"), None, None, None
    loss, winners = 0, []
    for k in (0, 1):
        allmins = torch.cat(mins[k])
        top = torch.sort(allmins.detach(), descending=True)
        assert len(allmins) == 1 or float(top.values[0] - top.values[1]) > 1e-3, "near-tie between directed maxima"
        b, i = owner[k][int(top.indices[0])]
        to_others = torch.sort(dis[b][i] if k == 0 else dis[b][:, i]).values
        assert len(to_others) == 1 or float(to_others[1] - to_others[0]) > 1e-3, "near-tie at the winning point"
        winners.append(b)
        loss = loss + allmins.max()
    gp, gl = torch.autograd.grad(loss, [P, L])
    return float(loss.detach()), gp.numpy(), gl.numpy(), winners


def as_module_mask(mask):
    """None, one (B,N) array for both clouds, or a pair -> ((xm, ym) as arrays, the module's mask= argument)."""
    if mask is None:
        return (None, None), None
    if isinstance(mask, np.ndarray):
        return (mask, mask), tg(mask).bool()
    return (mask[0], mask[1]), (tg(mask[0]).bool(), tg(mask[1]).bool())


def check_hausdorff_module(pred, label, mask=None):
    """HausdorffLoss(pred, label, mask=) on the device against hausdorff_loss_f64: value at relative 1e-5, both gradients at 1e-5 of their scale.
    mask: None, one (B,N) array for both clouds, or a pair."""
    (xm, ym), module_mask = as_module_mask(mask)
    want, rp, rl, winners = hausdorff_loss_f64(pred, label, xm, ym)
    P, L = tg(pred).requires_grad_(), tg(label).requires_grad_()
    got = gnn_loss.HausdorffLoss()(P, L, mask=module_mask)
    assert got.dim() == 0
    print("HausdorffLoss", float(got.detach()), "float64", want, "winning samples", winners)
    assert abs(float(got.detach()) - want) <= 1e-5 * abs(want)
    gp, gl = torch.autograd.grad(got, [P, L])
    for name, g, ref in (("pred", gp.cpu().numpy(), rp), ("label", gl.cpu().numpy(), rl)):
        assert g.shape == ref.shape
        err, scale = np.abs(g - ref).max(), np.abs(ref).max()
        print("HausdorffLoss grad", name, "max abs error", err, "of", scale)
        assert err <= 1e-5 * scale + 1e-12
    return want, rp, rl, winners


def module_clouds(seed, B=4, N=40, M=50):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, N, 3)).astype(np.float32), rng.standard_normal((B, M, 3)).astype(np.float32)


FAR_X, FAR_Y = np.float32([6.0, 0.25, -0.5]), np.float32([0.5, -7.0, 0.25])


@pytest.mark.gpu
def test_hausdorff_loss_different_samples_win_the_two_directions():
    pred, label = module_clouds(81)
    pred[1, 7], label[2, 11] = FAR_X, FAR_Y
    _, rp, rl, winners = check_hausdorff_module(pred, label)
    assert winners == [1, 2]
    assert np.flatnonzero(np.abs(rp).sum((1, 2))).tolist() == [1, 2] and np.abs(rp[1, 7]).sum() > 0 and np.abs(rl[2, 11]).sum() > 0


@pytest.mark.gpu
def test_hausdorff_loss_one_sample_wins_both_and_single_points_double():
    pred, label = module_clouds(82)
    pred[3, 5], label[3, 9] = FAR_X, FAR_Y
    _, rp, rl, winners = check_hausdorff_module(pred, label)
    assert winners == [3, 3] and (rp[:3] == 0).all() and (rl[:3] == 0).all()
    # N = M = 1: both directions select the one pair of the same sample, so its two points get twice the unit vector
    pred, label = module_clouds(83, N=1, M=1)
    far = int(np.argmax(np.linalg.norm(pred[:, 0].astype(np.float64) - label[:, 0].astype(np.float64), axis=1)))
    _, rp, rl, winners = check_hausdorff_module(pred, label)
    assert winners == [far, far]
    u = pred[far, 0].astype(np.float64) - label[far, 0].astype(np.float64)
    u /= np.linalg.norm(u)
    assert np.allclose(rp[far, 0], 2 * u, rtol=0, atol=1e-12) and np.allclose(rl[far, 0], -2 * u, rtol=0, atol=1e-12)
    assert (np.delete(rp, far, 0) == 0).all() and (np.delete(rl, far, 0) == 0).all()


@pytest.mark.gpu
def test_hausdorff_loss_broadcast_label_takes_the_gradient_on_its_one_cloud():
    pred, label = module_clouds(84)
    label = label[:1].copy()
    pred[2, 3], label[0, 4] = FAR_X, FAR_Y
    pred[3, :, 1] += np.float32(1.5)                                      # sample 3 is the farthest from the far label point
    _, rp, rl, winners = check_hausdorff_module(pred, label)
    assert winners == [2, 3] and rl.shape == (1, 50, 3)
    assert np.abs(rl[0, 4]).sum() > 0 and np.count_nonzero(np.abs(rl[0]).sum(1)) == 2      # the far point, and the nearest of pred[2, 3]


@pytest.mark.gpu
@pytest.mark.parametrize("spelling", ["single", "pair"])
def test_hausdorff_loss_masked_out_winner(spelling):
    """The point that wins without the mask is masked out: the loss with the mask differs, and the gradient goes to the valid winner."""
    rng = np.random.default_rng(85)
    if spelling == "single":
        pred, label = module_clouds(86, N=45, M=45)
        mask = (rng.random((4, 45)) < 0.8).astype(np.uint8)
        masks = (mask, mask)
    else:
        pred, label = module_clouds(87)
        masks = mask = ((rng.random((4, 40)) < 0.8).astype(np.uint8), (rng.random((4, 50)) < 0.8).astype(np.uint8))
    pred[1, 7] = FAR_X
    masks[0][1, 7] = 0
    unmasked, _, _, won = hausdorff_loss_f64(pred, label)
    assert won[0] == 1
    want, rp, _, winners = check_hausdorff_module(pred, label, mask)
    print("HausdorffLoss float64 without the mask", unmasked, "with", want)
    assert abs(unmasked - want) > 1e-3 * want                             # (a hundred times the bound of the comparison)
    assert (rp[1, 7] == 0).all() and (rp[masks[0] == 0] == 0).all()


@pytest.mark.gpu
def test_hausdorff_loss_empty_samples():
    """A sample with an empty side never wins, whatever its points; every sample empty gives NaN."""
    pred, label = module_clouds(88)
    rng = np.random.default_rng(89)
    xm, ym = (rng.random((4, 40)) < 0.8).astype(np.uint8), (rng.random((4, 50)) < 0.8).astype(np.uint8)
    xm[2] = 0
    label[2, 5], ym[2, 5] = np.float32([0, -20, 0]), 1                    # would win max_m min_n by far if sample 2 took part
    want, rp, rl, winners = check_hausdorff_module(pred, label, (xm, ym))
    assert 2 not in winners and want < 15.0 and (rp[2] == 0).all() and (rl[2] == 0).all()
    P, L = tg(pred).requires_grad_(), tg(label)
    got = gnn_loss.HausdorffLoss()(P, L, mask=(tg(np.zeros_like(xm)).bool(), tg(ym).bool()))
    assert got.dim() == 0 and torch.isnan(got)
    assert np.isnan(hausdorff_loss_f64(pred, label, np.zeros_like(xm), ym)[0])


def chamfer_loss_f64(pred, label, xm, ym):
    """loss.py:8-17 per sample over the valid points, averaged over the batch, in float64."""
    total = 0.0
    for b in range(pred.shape[0]):
        vx, vy = np.flatnonzero(xm[b]), np.flatnonzero(ym[b])
        d = np.linalg.norm(pred[b][vx][:, None, :].astype(np.float64) - label[b][vy][None, :, :].astype(np.float64), axis=2)
        total += d.min(1).mean() + d.min(0).mean()
    return total / pred.shape[0]


@pytest.mark.gpu
@pytest.mark.parametrize("spelling", ["single", "pair"])
def test_chamfer_loss_with_a_mask(spelling):
    rng = np.random.default_rng(90)
    if spelling == "single":
        pred, label = module_clouds(91, N=45, M=45)
        xm = ym = (rng.random((4, 45)) < 0.7).astype(np.uint8)
        module_mask = tg(xm).bool()
    else:
        pred, label = module_clouds(92)
        xm, ym = (rng.random((4, 40)) < 0.7).astype(np.uint8), (rng.random((4, 50)) < 0.7).astype(np.uint8)
        module_mask = (tg(xm).bool(), tg(ym).bool())
    assert xm.any(1).all() and ym.any(1).all() and not xm.all() and not ym.all()
    want = chamfer_loss_f64(pred, label, xm, ym)
    got = gnn_loss.ChamferLoss()(tg(pred), tg(label), mask=module_mask)
    print("ChamferLoss masked", spelling, float(got), "float64", want, "unmasked", chamfer_loss_f64(pred, label, np.ones_like(xm), np.ones_like(ym)))
    assert got.dim() == 0 and abs(float(got) - want) <= 1e-5 * abs(want)
    assert abs(chamfer_loss_f64(pred, label, np.ones_like(xm), np.ones_like(ym)) - want) > 1e-3 * want      # (the mask matters)
