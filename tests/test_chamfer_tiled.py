"""The tiled chamfer (ag_chamfer_tiled / ag_chamfer_tiled_backward, `tiled=True` in adaptigraph_amd.losses): bit equality with the
LDS-resident kernels wherever both apply (across a query-tile boundary and two chunk boundaries), the reference formula and float64
autograd beyond the resident limit, HIP-graph capture, and refusals that are error codes."""
import ctypes

import numpy as np
import pytest
import torch

from adaptigraph_amd import _lib, losses

DEV = "cuda:0"
LIMIT = 12800                                   # N + M of the resident kernels


def _tile_sizes():
    tq, to = ctypes.c_int(0), ctypes.c_int(0)
    _lib.lib().ag_chamfer_tile_sizes(ctypes.byref(tq), ctypes.byref(to))
    return tq.value, to.value


TQ, TO = _tile_sizes()


def tg(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return t.data_ptr() if t is not None else None


# ------------------------------------------------------------------ CPU side
def test_tile_sizes_leave_room_for_the_bitwise_shapes():
    """A query tile is four points per thread of a 256-thread workgroup; a shape that crosses one tile boundary on one side and two chunk
    boundaries on the other must still fit the resident kernels it is compared with."""
    assert TQ == 1024 and TO >= 4 and TO % 4 == 0
    assert (TQ + 1) + (2 * TO + 1) <= LIMIT


def test_workspace_size_and_argument_refusals_are_codes():
    """Every check runs before the first HIP call, so none of this needs a GPU (the pointers are never followed)."""
    L = _lib.lib()
    assert L.ag_chamfer_tiled_workspace_bytes(2, 1000, 11801) >= 2 * 12801 * 4
    assert L.ag_chamfer_tiled_workspace_bytes(1, 1 << 24, 1 << 24) >= (2 << 24) * 4
    for bad in ((0, 5, 5), (1, 0, 5), (1, 5, 0), (1, (1 << 24) + 1, 5), (1, 5, (1 << 24) + 1)):
        assert L.ag_chamfer_tiled_workspace_bytes(*bad) == 0
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    need = L.ag_chamfer_tiled_workspace_bytes(2, 3, 4)
    assert need >= 2 * 7 * 4
    args = (2, 3, 4, 1, p, None, None)
    assert L.ag_chamfer_tiled(p, None, p, None, *args, p, need - 1, None) == -3          # AG_ERR_WS: one byte short
    assert b"workspace" in L.ag_last_error()
    assert L.ag_chamfer_tiled(p, None, p, None, *args, None, need, None) == -3           # no workspace at all
    assert L.ag_chamfer_tiled(p, p, p, None, *args, p, need, None) == -1                 # one mask without the other
    assert b"both masks" in L.ag_last_error()
    assert L.ag_chamfer_tiled(p, None, p, p, *args, p, need, None) == -1
    assert L.ag_chamfer_tiled(p, None, p, None, 2, 3, 4, 1, p, p, None, p, need, None) == -1      # one index output without the other
    assert L.ag_chamfer_tiled(p, None, p, None, 2, 0, 4, 1, p, None, None, p, need, None) == -1   # N = 0
    assert b"N=0" in L.ag_last_error()
    assert L.ag_chamfer_tiled(p, None, p, None, 2, 3, (1 << 24) + 1, 1, p, None, None, p, need, None) == -1
    assert L.ag_chamfer_tiled(None, None, p, None, *args, p, need, None) == -1
    assert L.ag_chamfer_tiled_backward(p, p, p, None, p, p, p, 2, 3, 4, 1, p, None, None) == -1
    assert L.ag_chamfer_tiled_backward(p, None, p, None, p, p, p, 2, 0, 4, 1, p, None, None) == -1
    assert L.ag_chamfer_tiled_backward(p, None, p, None, p, p, p, 2, 3, (1 << 24) + 1, 1, p, None, None) == -1
    assert L.ag_chamfer_tiled_backward(p, None, p, None, None, p, p, 2, 3, 4, 1, p, None, None) == -1


def test_tiled_refuses_cpu_tensors_like_the_default():
    with pytest.raises(RuntimeError, match="no CPU path"):
        losses.chamfer(torch.zeros(2, 5, 3), torch.zeros(1, 4, 3), tiled=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        losses.mean_chamfer_device(torch.zeros(2, 5, 3), torch.zeros(2, 4, 3), torch.ones(2, 5), torch.ones(2, 4), tiled=True)


# ------------------------------------------------------------------ GPU: the same bits as the resident kernels
def _fwd_idx(tiled, x, xm, y, ym, y_batched):
    """out, idx_x, idx_y straight from the C ABI (either form)."""
    L = _lib.lib()
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    ix = torch.full((B, N), -7, dtype=torch.int32, device=x.device)
    iy = torch.full((B, M), -7, dtype=torch.int32, device=x.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if tiled:
        nbytes = L.ag_chamfer_tiled_workspace_bytes(B, N, M)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        rc = L.ag_chamfer_tiled(_ptr(x), _ptr(xm), _ptr(y), _ptr(ym), B, N, M, y_batched, _ptr(out), _ptr(ix), _ptr(iy), _ptr(ws), nbytes, stream)
    else:
        rc = L.ag_chamfer_fwd_idx(_ptr(x), _ptr(xm), _ptr(y), _ptr(ym), B, N, M, y_batched, _ptr(out), _ptr(ix), _ptr(iy), stream)
    assert rc == 0, L.ag_last_error()
    torch.cuda.synchronize()
    return out, ix, iy


def _value_and_grads(tiled, x, xm, y, ym, w):
    """out, gx, gy through adaptigraph_amd.losses under autograd (the public functions where they take the case: `mean_chamfer_device` has no
    broadcast target, so a masked broadcast goes through the autograd function both wrap)."""
    X, Y = x.clone().requires_grad_(), y.clone().requires_grad_()
    if xm is None:
        out = losses.chamfer(X, Y, tiled=tiled)
    elif y.shape[0] == x.shape[0]:
        out = losses.mean_chamfer_device(X, Y, xm, ym, tiled=tiled)
    else:
        out = losses._Chamfer.apply(X, Y, xm, ym, tiled)
    gx, gy = torch.autograd.grad(out, [X, Y], grad_outputs=w)
    return out.detach(), gx, gy


def _same(a, b):
    """bit equality, NaN equal to NaN"""
    return a.shape == b.shape and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0)) and torch.equal(a.isnan(), b.isnan())


def _masks(rng, B, N, M, By):
    """~70 % valid; where the shape has them: sample 0 loses its first whole query tile of x and (a target per sample) the first whole
    chunk of y, the last target cloud loses its second chunk, and sample 1 loses every particle (value NaN, gradient zero)."""
    xm, ym = rng.random((B, N)) < 0.7, rng.random((By, M)) < 0.7
    xm[:, -1] = ym[:, -1] = True
    if N > TQ:
        xm[0, :TQ] = False
    if M > TO and By > 1:
        ym[0, :TO] = False
    if M > 2 * TO:
        ym[By - 1, TO:2 * TO] = False
    xm[1] = False
    return xm, ym


def _check_bitwise(x, xm, y, ym, batched, w):
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    assert N + M <= LIMIT, "the resident form must apply"
    yb = 1 if (batched and B > 1) else 0
    o0, ix0, iy0 = _fwd_idx(False, x, xm, y, ym, yb)
    o1, ix1, iy1 = _fwd_idx(True, x, xm, y, ym, yb)
    assert _same(o0, o1) and torch.equal(ix0, ix1) and torch.equal(iy0, iy1)
    assert int(ix1.min()) >= -1 and int(ix1.max()) < M and int(iy1.min()) >= -1 and int(iy1.max()) < N
    v0, gx0, gy0 = _value_and_grads(False, x, xm, y, ym, w)
    v1, gx1, gy1 = _value_and_grads(True, x, xm, y, ym, w)
    assert _same(v0, o0) and _same(v1, o0)
    assert torch.equal(gx0, gx1) and torch.equal(gy0, gy1) and gy1.shape == y.shape
    assert torch.isfinite(gx1).all() and torch.isfinite(gy1).all()
    with torch.no_grad():                                   # the form without indices
        if xm is None:
            assert _same(losses.chamfer(x, y, tiled=True), o0)
        elif batched:
            assert _same(losses.mean_chamfer_device(x, y, xm, ym, tiled=True), o0)
    return o1, ix1, iy1, gx1, gy1


BITWISE = [(3, TQ + 1, TO + 2, True), (5, 37, 2 * TO + 1, False), (2, 1, 1, True)]      # B, N, M, y per sample


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,N,M,batched", BITWISE)
def test_tiled_is_bit_equal_to_the_resident_kernels(B, N, M, batched, masked):
    rng = np.random.default_rng(B * 100003 + N * 17 + M + masked)
    By = B if batched else 1
    x = tg(rng.normal(0, 2, (B, N, 3)).astype(np.float32))
    y = tg(rng.normal(0.3, 2, (By, M, 3)).astype(np.float32))
    w = tg(rng.uniform(0.5, 2.0, B).astype(np.float32))
    xm = ym = None
    if masked:
        xm, ym = (tg(m.astype(np.uint8)) for m in _masks(rng, B, N, M, By))
    out, ix, iy, gx, gy = _check_bitwise(x, xm, y, ym, batched, w)
    if masked:
        assert torch.isnan(out[1]) and float(gx[1].abs().max()) == 0.0 and int(ix[1].max()) == -1 and int(iy[1].max()) == -1
        if batched:
            assert float(gy[1].abs().max()) == 0.0
        assert torch.isfinite(out[0]) and (B < 3 or torch.isfinite(out[2:]).all())
        valid = xm[0].bool()
        assert bool((ix[0][~valid] == -1).all()) and bool((ix[0][valid] >= 0).all())
        assert float(gx[0][~valid].abs().sum()) == 0.0
    else:
        assert torch.isfinite(out).all() and int(ix.min()) >= 0 and int(iy.min()) >= 0


@pytest.mark.gpu
def test_tiled_ties_go_to_the_lowest_index_across_chunks():
    """The same target point at index 5 and at index TO + 5 (two chunks), a particle that sits exactly on it (distance 0: u(0) = 0), and a
    duplicated particle: both forms pick the lower index, and the gradient stays finite and equal."""
    rng = np.random.default_rng(11)
    B, N, M = 2, 37, 2 * TO + 1
    x = rng.normal(0, 2, (B, N, 3)).astype(np.float32)
    y = rng.normal(0.3, 2, (1, M, 3)).astype(np.float32)
    y[0, TO + 5] = y[0, 5]
    x[0, 3] = y[0, 5]
    x[:, 30] = x[:, 4]
    w = tg(np.array([1.5, 0.75], np.float32))
    out, ix, iy, gx, gy = _check_bitwise(tg(x), None, tg(y), None, False, w)
    assert int(ix[0, 3]) == 5 and int(iy[0, 5]) == 3 and int(iy[0, TO + 5]) == 3
    assert not bool((iy == 30).any()) and torch.equal(ix[:, 30], ix[:, 4])


# ------------------------------------------------------------------ GPU: beyond the resident limit
def _ref_chamfer(x, y):
    """losses.py:4-10 for one sample in float32 numpy, in row chunks of the (M, N) distance table: x (N,3), y (M,3)."""
    N, M = len(x), len(y)
    min_over_n = np.empty(M, np.float32)
    min_over_m = np.full(N, np.inf, np.float32)
    for r0 in range(0, M, 1024):
        dis = np.sqrt(((x[None, :, :] - y[r0:r0 + 1024, None, :]) ** 2).sum(-1, dtype=np.float32))      # (rows, N)
        min_over_n[r0:r0 + 1024] = dis.min(1)
        min_over_m = np.minimum(min_over_m, dis.min(0))
    return np.float32(min_over_n.mean(dtype=np.float32) + min_over_m.mean(dtype=np.float32))


@pytest.mark.gpu
def test_goal_cloud_beyond_the_limit_matches_the_reference_formula():
    """The planner's call of plan.py:139-146: 1 000 rope particles against every point of a goal cloud of 11 801."""
    rng = np.random.default_rng(21)
    B, N, M = 2, 1000, 11801
    assert N + M > LIMIT
    x = rng.normal(0, 2, (B, N, 3)).astype(np.float32)
    y = rng.normal(0.3, 2, (1, M, 3)).astype(np.float32)
    ref = np.array([_ref_chamfer(x[b], y[0]) for b in range(B)])
    got = losses.chamfer(tg(x), tg(y), tiled=True).cpu().numpy()
    err = np.abs(got - ref).max()
    print("tiled chamfer", (B, N, M), "max abs error", err, "ref", ref)
    assert err <= 5e-6 * max(1.0, float(np.abs(ref).max()))
    with pytest.raises(RuntimeError, match="LDS-resident limit"):      # the default keeps its refusal
        losses.chamfer(tg(x), tg(y))


@pytest.mark.gpu
def test_masked_clouds_beyond_the_limit_match_the_reference_formula():
    rng = np.random.default_rng(22)
    B, N, M = 1, 6401, 6400
    assert N + M > LIMIT
    x = rng.normal(0, 2, (B, N, 3)).astype(np.float32)
    y = rng.normal(0.3, 2, (B, M, 3)).astype(np.float32)
    xm, ym = rng.random((B, N)) < 0.7, rng.random((B, M)) < 0.7
    ref = np.array([_ref_chamfer(x[0][xm[0]], y[0][ym[0]])])
    got = losses.mean_chamfer(tg(x), tg(y), tg(xm), tg(ym), tiled=True)
    err = np.abs(got - ref).max()
    print("tiled masked chamfer", (B, N, M), "max abs error", err, "ref", ref)
    assert got.shape == (B,) and err <= 5e-6 * max(1.0, float(np.abs(ref).max()))
    with pytest.raises(RuntimeError, match="LDS-resident limit"):
        losses.mean_chamfer(tg(x), tg(y), tg(xm), tg(ym))


def _ref_grads(x, y, xm, ym, w):
    """float64 torch autograd of sum_b w_b chamfer_b over the masked-in points (losses.py:4-24), the argmin of every min found in float64.
    A float32 squared distance carries a relative error of at most a few 2^-24 (three rounded products and two sums of rounded differences:
    below 5e-7), so the float32 kernels pick the same pair whenever best and second best differ by more than 1e-6 of the second; the data
    is checked to keep four times that gap."""
    B = x.shape[0]
    X, Y = torch.from_numpy(x).double().requires_grad_(), torch.from_numpy(y).double().requires_grad_()
    loss = 0
    for b in range(B):
        by = b if y.shape[0] == B else 0
        xb, yb = X[b, np.nonzero(xm[b])[0]], Y[by, np.nonzero(ym[by])[0]]
        with torch.no_grad():
            d2 = torch.cdist(yb, xb) ** 2                    # (My, Nx)
            for dd in (d2, d2.t()):
                two = dd.topk(2, dim=1, largest=False).values
                assert bool((two[:, 1] - two[:, 0] > 4e-6 * two[:, 1]).all()), "near-tie in the test data"
            nn_y, nn_x = d2.argmin(1), d2.argmin(0)
        loss = loss + w[b] * (torch.linalg.vector_norm(yb - xb[nn_y], dim=-1).mean() + torch.linalg.vector_norm(xb - yb[nn_x], dim=-1).mean())
    gx, gy = torch.autograd.grad(loss, [X, Y])
    return gx.numpy(), gy.numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("batched,masked", [(False, False), (False, True), (True, False), (True, True)])
def test_tiled_gradients_beyond_the_limit_vs_float64_autograd(batched, masked):
    rng = np.random.default_rng(32 + 2 * batched + masked)       # (seeds whose clouds pass the near-tie check of _ref_grads)
    B, N, M = 2, 300, 12600
    assert N + M > LIMIT
    By = B if batched else 1
    x = rng.normal(0, 2, (B, N, 3)).astype(np.float32)
    y = rng.normal(0.3, 2, (By, M, 3)).astype(np.float32)
    xm, ym = np.ones((B, N), bool), np.ones((By, M), bool)
    if masked:
        xm, ym = rng.random((B, N)) < 0.7, rng.random((By, M)) < 0.7
    w = rng.uniform(0.5, 2.0, B)
    rx, ry = _ref_grads(x, y, xm, ym, w)
    dev = (tg(x), tg(xm.astype(np.uint8)) if masked else None, tg(y), tg(ym.astype(np.uint8)) if masked else None, tg(w.astype(np.float32)))
    out, gx, gy = _value_and_grads(True, *dev)
    out2, gx2, gy2 = _value_and_grads(True, *dev)
    assert torch.equal(out, out2) and torch.equal(gx, gx2) and torch.equal(gy, gy2)      # no atomics: the same bits every call
    assert torch.isfinite(out).all()
    for name, got, ref in (("gx", gx.cpu().numpy(), rx), ("gy", gy.cpu().numpy(), ry)):
        assert got.shape == ref.shape
        err, scale = np.abs(got - ref).max(), np.abs(ref).max()
        print("tiled chamfer", name, (B, N, M), "batched" if batched else "broadcast", "masked" if masked else "", "max abs error", err, "of", scale)
        assert err <= 1e-5 * scale + 1e-12


# ------------------------------------------------------------------ GPU: capture
@pytest.mark.gpu
def test_tiled_forward_and_backward_replay_from_a_hip_graph():
    """Forward with indices and backward (a broadcast target: the row sum too) captured on one stream; three replays on new inputs copied
    into the static tensors, each equal to the eager result bit for bit."""
    rng = np.random.default_rng(41)
    B, N, M = 3, 37, 2 * TO + 1

    def draw():
        return (tg(rng.normal(0, 2, (B, N, 3)).astype(np.float32)), tg(rng.normal(0.3, 2, (1, M, 3)).astype(np.float32)),
                tg(rng.uniform(0.5, 2.0, B).astype(np.float32)))

    x0, y0, w0 = draw()
    X, Y, W = x0.clone().requires_grad_(), y0.clone().requires_grad_(), w0.clone()

    def step():
        out = losses.chamfer(X, Y, tiled=True)
        return (out,) + torch.autograd.grad(out, [X, Y], grad_outputs=W)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                           # warm-up off the capture (allocator, the stream's workspace)
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        static = step()
    for _ in range(3):
        x, y, w = draw()
        with torch.no_grad():
            X.copy_(x), Y.copy_(y), W.copy_(w)
        gr.replay()
        torch.cuda.synchronize()
        eager = _value_and_grads(True, x, None, y, None, w)
        for a, b in zip(static, eager):
            assert torch.equal(a.detach(), b)
