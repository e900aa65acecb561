"""The matching losses on the GPU: `losses.emd` (ag_emd / ag_emd_backward), `losses.hausdorff` (ag_hausdorff), the modules of `gnn_loss` and the
`loss_funcs` key of `train.train`, against tests/golden/gnn_loss_cases.npz (scipy's assignments and the reference's loss values, recorded by
tools/gen_loss_golden.py).  Nothing here imports scipy or the reference."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from adaptigraph_amd import _lib, gnn_loss, losses

DEV = "cuda:0"
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 3), (63, 64), (64, 65), (65, 64), (100, 100), (129, 257), (257, 129)]


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("gnn_loss_cases")


def tg(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cost_matrix(x, y):
    """(N,3), (M,3) -> (N,M) fp32: c = sqrt((dx dx + dy dy) + dz dz), every product rounded to fp32 on its own."""
    x, y = x.astype(np.float32), y.astype(np.float32)
    d0, d1, d2 = (x[:, None, c] - y[None, :, c] for c in range(3))       # (one contiguous (N,M) plane per coordinate: the same operations)
    return np.sqrt((d0 * d0 + d1 * d1) + d2 * d2).astype(np.float32)


def inverse(col, M):
    row = np.full((col.shape[0], M), -1, np.int32)
    for b in range(col.shape[0]):
        n = np.flatnonzero(col[b] >= 0)
        row[b, col[b, n]] = n
    return row


def expected_value(x, y, col):
    """np.float32(S / K) per sample: S accumulated left to right in float64 over the pairs (n, col[n]) in ascending n; NaN when K = 0."""
    out = np.full(x.shape[0], np.nan, np.float32)
    for b in range(x.shape[0]):
        yb = y[b if y.shape[0] == x.shape[0] else 0]
        C = cost_matrix(x[b], yb)
        S, K = 0.0, 0
        for n in range(x.shape[1]):
            if col[b, n] >= 0:
                S += float(C[n, col[b, n]])
                K += 1
        if K:
            out[b] = np.float32(S / K)
    return out


def case(name, broadcast=False, g=None):
    """x, y, xm, ym, col of a fixture case; broadcast: y[:1] (and ym[:1]) for every sample, with the assignment recorded for that.
    g: the loaded fixture file, gnn_loss_cases by default."""
    g = golden() if g is None else g
    x, y = g[name + "_x"], g[name + "_y"]
    xm, ym = (g[name + "_xm"], g[name + "_ym"]) if name + "_xm" in g else (None, None)
    if broadcast:
        return x, y[:1], xm, None if ym is None else ym[:1], g[name + "_colb"]
    return x, y, xm, ym, g[name + "_col"]


def run_emd(x, y, xm=None, ym=None):
    out, col, row = losses.emd(tg(x), tg(y), None if xm is None else tg(xm), None if ym is None else tg(ym), return_assignment=True)
    return out.cpu().numpy(), col.cpu().numpy(), row.cpu().numpy()


@functools.lru_cache(maxsize=None)
def solved(name, broadcast):
    x, y, xm, ym, col = case(name, broadcast)
    return run_emd(x, y, xm, ym)


def assert_within_one_ulp(got, want):
    assert got.dtype == np.float32 and want.dtype == np.float32
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    print("emd value", got[ok], "expected", want[ok])
    assert (np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64)) <= np.spacing(np.abs(want[ok])).astype(np.float64)).all()


# ------------------------------------------------------------------ 1, 2: assignment and value
@pytest.mark.gpu
@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("N,M", SHAPES)
def test_assignment_equals_scipy(N, M, broadcast):
    """One column per lane and the step to two, rectangular both ways, the training shape; B = 3 different clouds."""
    x, y, _, _, col = case(f"s{N}x{M}", broadcast)
    assert x.shape == (3, N, 3) and y.shape == (1 if broadcast else 3, M, 3) and int(golden()[f"s{N}x{M}_unique"]) == 1
    _, got_col, got_row = solved(f"s{N}x{M}", broadcast)
    assert torch.equal(torch.from_numpy(got_col), torch.from_numpy(col))
    assert torch.equal(torch.from_numpy(got_row), torch.from_numpy(inverse(col, M)))


@pytest.mark.gpu
@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("N,M", SHAPES)
def test_value_is_the_fp64_mean_rounded_once(N, M, broadcast):
    x, y, _, _, col = case(f"s{N}x{M}", broadcast)
    out, _, _ = solved(f"s{N}x{M}", broadcast)
    assert_within_one_ulp(out, expected_value(x, y, col))
    total = golden()[f"s{N}x{M}_totalb" if broadcast else f"s{N}x{M}_total"]
    assert_within_one_ulp(out, (total / min(N, M)).astype(np.float32))


# ------------------------------------------------------------------ 3: masks
@pytest.mark.gpu
@pytest.mark.parametrize("broadcast", [False, True])
def test_masked_clouds(broadcast):
    """Padded clouds whose valid counts differ per sample and per side; sample 1 has an empty side, sample 3 every point valid."""
    x, y, xm, ym, col = case("masked", broadcast)
    assert xm[1].sum() == 0 and xm[3].all() and (broadcast or ym[3].all())
    assert len({int(v) for v in xm.sum(1)}) == 4
    out, got_col, got_row = solved("masked", broadcast)
    assert np.isnan(out[1]) and (got_col[1] == -1).all() and (got_row[1] == -1).all()
    assert torch.equal(torch.from_numpy(got_col), torch.from_numpy(col))
    assert torch.equal(torch.from_numpy(got_row), torch.from_numpy(inverse(col, y.shape[1])))
    assert (got_col[xm == 0] == -1).all()
    assert_within_one_ulp(out, expected_value(x, y, col))


# ------------------------------------------------------------------ 4: structure
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain64x64", "chain65x130"])
def test_chain(name):
    x, y, _, _, col = case(name)
    out, got_col, got_row = solved(name, False)
    assert torch.equal(torch.from_numpy(got_col), torch.from_numpy(col))
    assert torch.equal(torch.from_numpy(got_row), torch.from_numpy(inverse(col, y.shape[1])))
    assert_within_one_ulp(out, expected_value(x, y, col))


@pytest.mark.gpu
def test_near_rigid_recovers_the_permutation():
    x, y, _, _, col = case("rigid")
    perm = golden()["rigid_perm"]                                 # y[b, m] ~ x[b, perm[b, m]]
    _, got_col, got_row = solved("rigid", False)
    assert x.shape == (3, 100, 3)
    assert torch.equal(torch.from_numpy(got_row), torch.from_numpy(perm))
    assert torch.equal(torch.from_numpy(got_col), torch.from_numpy(col))


@pytest.mark.gpu
def test_exact_permutation_has_value_zero():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 100, 3)).astype(np.float32)
    perm = np.stack([rng.permutation(100) for _ in range(3)])
    y = np.stack([x[b][perm[b]] for b in range(3)])
    out, _, got_row = run_emd(x, y)
    assert (out == 0.0).all() and np.array_equal(got_row, perm)


# ------------------------------------------------------------------ 5: ties
@pytest.mark.gpu
def test_ties_give_one_optimal_injection_every_time():
    x, y, _, _, _ = case("ties")
    assert x.shape == (3, 27, 3) and int(golden()["ties_unique"]) == 0
    out, col, row = run_emd(x, y)
    out2, col2, row2 = run_emd(x, y)
    assert np.array_equal(out, out2) and np.array_equal(col, col2) and np.array_equal(row, row2)
    for b in range(3):
        assert sorted(col[b].tolist()) == list(range(27))
        assert np.array_equal(row[b][col[b]], np.arange(27))
        C = cost_matrix(x[b], y[b]).astype(np.float64)
        total, want = float(sum(C[n, col[b, n]] for n in range(27))), float(golden()["ties_total"][b])
        print("ties: total", total, "optimum", want)
        assert abs(total - want) <= 1e-9 * want


# ------------------------------------------------------------------ 6: non-finite input
@pytest.mark.gpu
def test_non_finite_sample_is_nan_and_alone():
    g = golden()
    x, y = g["s100x100_x"][:, :5].copy(), g["s100x100_y"][:, :5].copy()
    x[1, 2, 0], y[1, 0, 1] = np.nan, np.inf
    out, col, row = run_emd(x, y)
    assert np.isnan(out[1]) and (col[1] == -1).all() and (row[1] == -1).all()
    out2, col2, row2 = run_emd(x[[0, 2]], y[[0, 2]])
    assert np.isfinite(out2).all()
    assert np.array_equal(out[[0, 2]], out2) and np.array_equal(col[[0, 2]], col2) and np.array_equal(row[[0, 2]], row2)


# ------------------------------------------------------------------ 7: gradients
def ref_grads(x, y, col, w):
    """float64 torch autograd of sum_b w_b mean_pairs ||x_n - y_col[n]|| (loss.py:46-54 per sample) with the fixture's assignment."""
    X, Y = torch.from_numpy(x).double().requires_grad_(), torch.from_numpy(y).double().requires_grad_()
    loss = 0
    for b in range(x.shape[0]):
        n = np.flatnonzero(col[b] >= 0)
        if len(n) == 0:
            continue
        Yb = Y[b if y.shape[0] == x.shape[0] else 0]
        loss = loss + w[b] * torch.norm(X[b][n] - Yb[col[b, n]], 2, dim=1).mean()
    gx, gy = torch.autograd.grad(loss, [X, Y])
    return gx.numpy(), gy.numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name,broadcast", [("s64x65", False), ("s64x65", True), ("s65x64", False), ("masked", False), ("masked", True)])
def test_gradients_vs_float64_autograd(name, broadcast):
    x, y, xm, ym, col = case(name, broadcast)
    w = np.random.default_rng(3).uniform(0.5, 2.0, x.shape[0])
    rx, ry = ref_grads(x, y, col, w)
    X, Y = tg(x).requires_grad_(), tg(y).requires_grad_()
    out = losses.emd(X, Y, None if xm is None else tg(xm), None if ym is None else tg(ym))
    with torch.no_grad():
        plain = losses.emd(X, Y, None if xm is None else tg(xm), None if ym is None else tg(ym))
    assert torch.equal(out.detach().nan_to_num(-1.0), plain.nan_to_num(-1.0))      # the same value bits with and without grad
    gx, gy = torch.autograd.grad(out, [X, Y], grad_outputs=tg(w.astype(np.float32)))
    for label, got, ref in (("gx", gx.cpu().numpy(), rx), ("gy", gy.cpu().numpy(), ry)):
        assert got.shape == ref.shape
        err, scale = np.abs(got - ref).max(), np.abs(ref).max()
        print("emd", label, name, "broadcast" if broadcast else "batched", "max abs error", err, "of", scale)
        assert err <= 1e-5 * scale + 1e-12


# ------------------------------------------------------------------ 8: capture
@pytest.mark.gpu
def test_forward_and_backward_replay_from_a_hip_graph():
    rng = np.random.default_rng(41)
    B, N, M = 3, 37, 70

    def draw():
        return (tg(rng.standard_normal((B, N, 3)).astype(np.float32)), tg(rng.standard_normal((1, M, 3)).astype(np.float32)),
                tg(rng.uniform(0.5, 2.0, B).astype(np.float32)))

    x0, y0, w0 = draw()
    X, Y, W = x0.clone().requires_grad_(), y0.clone().requires_grad_(), w0.clone()

    def step(X, Y, W):
        out, col, row = losses.emd(X, Y, return_assignment=True)
        return (out, col, row) + torch.autograd.grad(out, [X, Y], grad_outputs=W)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                           # warm-up off the capture (allocator)
        step(X, Y, W)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        static = step(X, Y, W)
    for _ in range(3):
        x, y, w = draw()
        with torch.no_grad():
            X.copy_(x), Y.copy_(y), W.copy_(w)
        gr.replay()
        torch.cuda.synchronize()
        eager = step(x.clone().requires_grad_(), y.clone().requires_grad_(), w)
        for a, b in zip(static, eager):
            assert torch.equal(a.detach(), b.detach())


# ------------------------------------------------------------------ 9: refusals
@pytest.mark.gpu
def test_refusals_launch_nothing():
    L = _lib.lib()
    limit = _lib.AG_EMD_MAX_POINTS
    x, y = torch.zeros((2, limit + 1, 3), device=DEV), torch.zeros((2, 8, 3), device=DEV)
    xm, ym = torch.ones((2, limit + 1), dtype=torch.uint8, device=DEV), torch.ones((2, 8), dtype=torch.uint8, device=DEV)
    out = torch.full((2,), 7.0, device=DEV)
    col = torch.full((2, limit + 1), 7, dtype=torch.int32, device=DEV)
    row = torch.full((2, limit + 1), 7, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def emd(N, M, xmask=None, ymask=None):
        return L.ag_emd(p(x), xmask, p(y), ymask, 2, N, M, 1, p(out), p(col), p(row), None)

    assert emd(0, 8) == -1 and emd(8, 0) == -1                                          # N or M of 0
    assert emd(limit + 1, 8) == -1 and b"AG_EMD_MAX_POINTS" in L.ag_last_error()      # above the limit
    assert emd(8, limit + 1) == -1
    assert emd(8, 8, p(xm), None) == -1 and emd(8, 8, None, p(ym)) == -1 and b"both masks" in L.ag_last_error()
    assert L.ag_hausdorff(p(x), None, p(y), None, 2, 0, 8, 1, p(out), p(col), None) == -1
    assert L.ag_hausdorff(p(x), p(xm), p(y), None, 2, 8, 8, 1, p(out), p(col), None) == -1
    assert L.ag_hausdorff(p(x), None, p(y), None, 2, 12000, 801, 1, p(out), p(col), None) == -1
    assert L.ag_emd_backward(p(x), p(y), p(col), p(row), p(out), 2, 8, limit + 1, 1, p(x), None, None) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (col == 7).all() and (row == 7).all()                  # nothing was launched
    with pytest.raises(ValueError, match="both masks"):
        losses.emd(x[:, :8], y, xm[:, :8], None)
    with pytest.raises(ValueError, match="1 or 2"):                                      # By not in {1, B}
        losses.emd(x[:, :8], torch.zeros((3, 8, 3), device=DEV))
    with pytest.raises(RuntimeError, match="AG_EMD_MAX_POINTS"):
        losses.emd(x, y)
    with pytest.raises(RuntimeError):
        losses.emd(x[:, :0], y)
    with pytest.raises(RuntimeError, match="no CPU path"):                               # a CPU tensor
        losses.emd(torch.zeros(2, 8, 3), y)
    with pytest.raises(RuntimeError, match="no CPU path"):
        losses.hausdorff(torch.zeros(2, 8, 3), y)
    ok = losses.emd(x[:, :limit], y)                                                     # the limit itself is served
    assert ok.shape == (2,) and (ok == 0.0).all()


# ------------------------------------------------------------------ 10: hausdorff
def hausdorff_numpy(x, y, xm, ym, rows=512):
    """values (B,2) fp32 and arg (B,4) by the formula in numpy fp32, the cost matrix evaluated `rows` valid x points at a time (at the size limit
    the whole matrix and its temporaries would be hundreds of MB).  np.argmax / np.argmin return the first (lowest) index inside a block; across
    blocks a later block replaces a running minimum only when strictly lower and the running maximum only when strictly higher, so the lowest
    index wins as in `hausdorff_numpy_whole`."""
    B = x.shape[0]
    val, arg = np.full((B, 2), np.nan, np.float32), np.full((B, 4), -1, np.int32)
    for b in range(B):
        by = b if y.shape[0] == B else 0
        vx = np.arange(x.shape[1]) if xm is None else np.flatnonzero(xm[b])
        vy = np.arange(y.shape[1]) if ym is None else np.flatnonzero(ym[by])
        if len(vx) == 0 or len(vy) == 0:
            continue
        yv = y[by][vy]
        best, bn, bm = np.float32(-1.0), -1, -1                           # max_n min_m with its n and that n's nearest m (compact positions)
        cmin, carg = np.full(len(vy), np.inf, np.float32), np.full(len(vy), -1, np.int64)      # min_n per m so far, and its n
        for i0 in range(0, len(vx), rows):
            C = cost_matrix(x[b][vx[i0:i0 + rows]], yv)
            rmin = C.min(1)
            n = int(np.argmax(rmin))
            if rmin[n] > best:
                best, bn, bm = rmin[n], i0 + n, int(np.argmin(C[n]))
            blk, blk_arg = C.min(0), C.argmin(0)
            lower = blk < cmin
            cmin[lower], carg[lower] = blk[lower], i0 + blk_arg[lower]
        m = int(np.argmax(cmin))
        val[b] = best, cmin[m]
        arg[b] = vx[bn], vy[bm], vy[m], vx[carg[m]]
    return val, arg


def hausdorff_numpy_whole(x, y, xm, ym):
    """`hausdorff_numpy` on the whole cost matrix at once: what the block-wise form is checked against on the CPU."""
    B = x.shape[0]
    val, arg = np.full((B, 2), np.nan, np.float32), np.full((B, 4), -1, np.int32)
    for b in range(B):
        by = b if y.shape[0] == B else 0
        vx = np.arange(x.shape[1]) if xm is None else np.flatnonzero(xm[b])
        vy = np.arange(y.shape[1]) if ym is None else np.flatnonzero(ym[by])
        if len(vx) == 0 or len(vy) == 0:
            continue
        C = cost_matrix(x[b][vx], y[by][vy])
        n = int(np.argmax(C.min(1)))
        m = int(np.argmax(C.min(0)))
        val[b] = C.min(1)[n], C.min(0)[m]
        arg[b] = vx[n], vy[int(np.argmin(C[n]))], vy[m], vx[int(np.argmin(C[:, m]))]
    return val, arg


def check_hausdorff(x, y, xm=None, ym=None):
    val, arg = losses.hausdorff(tg(x), tg(y), None if xm is None else tg(xm), None if ym is None else tg(ym))
    want_val, want_arg = hausdorff_numpy(x, y, xm, ym)
    got = val.cpu()
    assert torch.equal(torch.isnan(got), torch.from_numpy(np.isnan(want_val)))
    assert torch.equal(got.nan_to_num(-1.0), torch.from_numpy(want_val).nan_to_num(-1.0))
    assert torch.equal(arg.cpu(), torch.from_numpy(want_arg))
    return val, arg


@pytest.mark.gpu
@pytest.mark.parametrize("N,M", [(1, 1), (63, 64), (257, 129)])
def test_hausdorff_values_are_the_formula_bits(N, M):
    x, y, _, _, _ = case(f"s{N}x{M}")
    check_hausdorff(x, y)
    check_hausdorff(x, y[:1])


@pytest.mark.gpu
def test_hausdorff_masks_ties_and_an_empty_side():
    x, y, xm, ym, _ = case("masked")
    val, arg = check_hausdorff(x, y, xm, ym)
    assert torch.isnan(val[1]).all() and (arg[1] == -1).all()
    check_hausdorff(x, y[:1], xm, ym[:1])
    # duplicated points on an integer grid: every min and max is attained several times; the lowest index wins
    rng = np.random.default_rng(9)
    gx, gy = rng.integers(0, 3, (2, 300, 3)).astype(np.float32), rng.integers(0, 3, (2, 280, 3)).astype(np.float32) + np.float32(0.5)
    gx[:, 150:] = gx[:, :150]
    gy[:, 140:] = gy[:, :140]
    val, arg = check_hausdorff(gx, gy)
    assert (arg.cpu().numpy()[:, [0, 3]] < 150).all() and (arg.cpu().numpy()[:, [1, 2]] < 140).all()


# ------------------------------------------------------------------ 11: modules
@pytest.mark.gpu
def test_modules_match_the_reference_values():
    g = golden()
    x, y, ref = tg(g["modules_x"]), tg(g["modules_y"]), g["modules_ref"]
    assert x.shape == (4, 100, 3) and y.shape == (4, 100, 3)
    for module, want in zip((gnn_loss.ChamferLoss(), gnn_loss.EarthMoverLoss(), gnn_loss.HausdorffLoss()), ref):
        got = module(x, y)
        assert got.dim() == 0
        print(type(module).__name__, float(got), "reference", float(want))
        assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want))
    # differentiable as they stand
    X = x.clone().requires_grad_()
    for module in (gnn_loss.ChamferLoss(), gnn_loss.EarthMoverLoss(), gnn_loss.HausdorffLoss()):
        (gx,) = torch.autograd.grad(module(X, y), [X])
        assert torch.isfinite(gx).all() and gx.abs().sum() > 0
    # mask=: padded slots take no part
    xm = torch.ones((4, 100), dtype=torch.bool, device=DEV)
    xm[:, 90:] = False
    full = gnn_loss.EarthMoverLoss()(x[:, :90].contiguous(), y[:, :90].contiguous())
    assert torch.equal(gnn_loss.EarthMoverLoss()(x, y, mask=xm), full)


# ------------------------------------------------------------------ 12: training
@pytest.mark.gpu
def test_unrolled_loss_with_the_emd_closure(weights):
    from adaptigraph_amd.train_model import unrolled_loss
    from test_train import batch_from, golden_csr, trainable
    g = load_golden("train_rope")
    model = trainable(weights).train()
    data = {k: tg(v) for k, v in batch_from(g).items()}
    data.update(Rr=golden_csr(g, g["b_attrs"].shape[1]), Rs=None)
    mask = data["obj_mask"]
    seen = []

    def spy(pred, label):
        v = losses.emd(pred, label, mask[:, :pred.shape[1]], mask[:, :pred.shape[1]]).mean()
        seen.append(v.detach().clone())
        return v

    funcs = gnn_loss.build_loss_funcs(gnn_loss.parse_loss_spec([["emd", 1]]), mask)
    loss = unrolled_loss(model, data, 3, funcs)
    unrolled_loss(model, data, 3, [(spy, 1)])
    assert len(seen) == 3 and torch.equal(loss.detach(), seen[0] + seen[1] + seen[2]) and torch.isfinite(loss)
    loss.backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert sum(float(p.grad.abs().sum()) for p in model.parameters()) > 0


@pytest.fixture()
def dataset_dir(tmp_path):
    from test_eval_rollout import write_dataset
    g_eval = load_golden("evalrollout_rope")
    write_dataset(str(tmp_path), g_eval)
    return g_eval, str(tmp_path)


@pytest.mark.gpu
def test_train_without_the_key_is_unchanged_and_with_it_runs(dataset_dir, monkeypatch):
    from adaptigraph_amd import train as agtrain
    from test_train import train_config
    g_eval, root = dataset_dir
    calls = []
    real = agtrain.unrolled_loss

    def spy(*args, **kwargs):
        loss = real(*args, **kwargs)
        calls.append((len(args), sorted(kwargs), float(loss.detach())))
        return loss

    monkeypatch.setattr(agtrain, "unrolled_loss", spy)

    def run(**extra):
        cfg = train_config(root, g_eval, DEV)
        cfg["train_config"].update(n_epochs=1, n_iters_per_epoch={"train": 2, "valid": 1}, random_seed=3, **extra)
        del calls[:]
        hist = agtrain.train(cfg)
        return hist, list(calls)

    hist, plain = run()
    assert [c[:2] for c in plain] == [(3, [])] * 3                          # unrolled_loss(model, data, n_future), exactly as before
    assert hist["train"][0] == float(np.mean([c[2] for c in plain[:2]])) and hist["valid"][0] == plain[2][2]
    hist_mse, as_mse = run(loss_funcs=[["mse", 1]])                         # the same objective spelled out: the same losses
    assert [c[2] for c in as_mse] == [c[2] for c in plain] and [c[0] for c in as_mse] == [4] * 3
    hist_emd, with_emd = run(loss_funcs=[["mse", 1], ["emd", 0.5]])
    assert len(with_emd) == 3 and np.isfinite([c[2] for c in with_emd]).all() and np.isfinite(hist_emd["train"]).all()
    assert with_emd[0][2] > plain[0][2]                                     # (the emd term is positive)
    with pytest.raises(ValueError, match="unknown loss"):
        run(loss_funcs=[["sinkhorn", 1]])
    assert calls == []                                                      # refused at start-up
