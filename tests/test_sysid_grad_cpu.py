"""Sys-id by gradient without a GPU: the statements the GPU tests of tests/test_sysid_grad.py are held to — `ag_edge_views` as a stable argsort
(and as the per-sample counting sort the kernel runs), the model step's state update and its adjoint in float64 — and the argument checks of
`ag_edge_views`, `ag_step_update_*` and `optimize(method=...)`, which all answer before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch

from adaptigraph_amd import _lib, configs, graph, train_ops
from adaptigraph_amd.forward_dynamics import block_sum, step_update_ops

MIN, MEAN = _lib.AG_HEIGHT_MIN, _lib.AG_HEIGHT_MASKED_MEAN


# ------------------------------------------------------------------ ag_edge_views
def edge_views_np(row_ptr, send, B, N):
    """What ag_edge_views must write: send_perm = the stable ascending-sender order of the edges, col_ptr = the prefix of the per-sender counts."""
    E = int(row_ptr[B * N])
    s = np.asarray(send[:E], np.int64)
    perm = np.argsort(s, kind="stable").astype(np.int32)
    col_ptr = np.concatenate([[0], np.cumsum(np.bincount(s, minlength=B * N))]).astype(np.int32)
    return perm, col_ptr


def edge_views_counting_sort(row_ptr, send, B, N):
    """The kernel's algorithm step by step: per sample count -> scan -> scatter 256 edges at a time in edge order, four waves of 64 in turn, a lane's
    rank among the lanes with its sender from one ballot per bit of the sender index."""
    E = int(row_ptr[B * N])
    perm = np.full(E, -1, np.int32)
    col_ptr = np.zeros(B * N + 1, np.int32)
    n_bits = int(max(N - 1, 0)).bit_length()
    for b in range(B):
        e0, e1 = int(row_ptr[b * N]), int(row_ptr[(b + 1) * N])
        cnt = np.zeros(N, np.int64)
        for e in range(e0, e1):
            cnt[send[e] - b * N] += 1
        first = np.concatenate([[0], np.cumsum(cnt)[:-1]]) if N else cnt
        col_ptr[b * N:(b + 1) * N] = e0 + first
        cur = first.copy()
        for w0 in range(e0, e1, 64):                       # one wave's 64 edges; waves and chunks in edge order
            lanes = np.arange(w0, min(w0 + 64, e1))
            key = np.asarray(send[lanes], np.int64) - b * N
            same = np.ones((len(lanes), len(lanes)), bool)  # same[i, j]: lane j is in lane i's ballot mask
            for bit in range(n_bits):
                on = (key >> bit) & 1
                same &= on[:, None] == on[None, :]
            rank = np.array([same[i, :i].sum() for i in range(len(lanes))])
            at = cur[key].copy()                            # every lane reads the counter before a group's first lane moves it
            perm[e0 + at + rank] = lanes
            for i in np.nonzero(rank == 0)[0]:
                cur[key[i]] = at[i] + same[i].sum()
    col_ptr[B * N] = row_ptr[B * N]
    return perm, col_ptr


def csr_of(lists, N):
    """[(recv_local, send_local)] per sample, receiver-sorted -> (row_ptr, recv, send) as ag_build_edges lays them out (global node ids)."""
    B = len(lists)
    row_ptr, recv, send = np.zeros(B * N + 1, np.int32), [], []
    for b, (r, s) in enumerate(lists):
        r, s = np.asarray(r, np.int64), np.asarray(s, np.int64)
        assert (np.diff(r) >= 0).all()
        row_ptr[b * N + 1:(b + 1) * N + 1] = np.bincount(r, minlength=N)
        recv.append(r + b * N)
        send.append(s + b * N)
    row_ptr = np.cumsum(row_ptr).astype(np.int32)
    cat = lambda xs: np.concatenate(xs).astype(np.int32) if xs else np.zeros(0, np.int32)
    return row_ptr, cat(recv), cat(send)


_RNG = np.random.default_rng(5)
HAND_MADE = {
    "empty graph": ([([], [])], 4),
    "all edges to one sender": ([(sorted(list(range(5)) * 2), [3] * 10)], 5),
    "senders absent": ([([0, 0, 2, 4, 4, 4], [5, 1, 1, 5, 0, 1])], 6),
    "B = 3, empty middle sample": ([([0, 1, 1, 2], [2, 2, 0, 1]), ([], []), ([1, 2, 2], [0, 0, 1])], 3),
    "equal senders across waves": ([(np.sort(_RNG.integers(0, 70, 300)), _RNG.integers(0, 7, 300))] * 2, 70),
}


@pytest.mark.parametrize("case", list(HAND_MADE))
def test_edge_views_statement_on_hand_made_lists(case):
    lists, N = HAND_MADE[case]
    B = len(lists)
    row_ptr, recv, send = csr_of(lists, N)
    perm, col_ptr = edge_views_np(row_ptr, send, B, N)
    E = len(send)
    assert perm.shape == (E,) and col_ptr.shape == (B * N + 1,) and col_ptr[0] == 0 and col_ptr[-1] == E
    assert sorted(perm.tolist()) == list(range(E))
    s = send[perm]
    assert (np.diff(s) >= 0).all() and all(perm[i] < perm[i + 1] for i in range(E - 1) if s[i] == s[i + 1])      # ascending sender, stable
    for n in range(B * N):
        assert (s[col_ptr[n]:col_ptr[n + 1]] == n).all()
    perm2, col2 = edge_views_counting_sort(row_ptr, send, B, N)
    assert np.array_equal(perm, perm2) and np.array_equal(col_ptr, col2)
    pad = lambda a: torch.from_numpy(np.concatenate([a, np.zeros(3, np.int32)]))       # (the builder's buffers are longer than the edge count)
    v = train_ops.EdgeViews(graph.CSREdges(torch.from_numpy(row_ptr), pad(recv), pad(send), B, N, E + 3))
    assert v.E == E and np.array_equal(v.send_perm.numpy(), perm) and np.array_equal(v.col_ptr.numpy(), col_ptr)
    assert v.send_perm.dtype == torch.int32 and v.col_ptr.dtype == torch.int32


def test_edge_views_entry_point_rejects_bad_arguments():
    L = _lib.lib()
    buf = (ctypes.c_int32 * 16)()
    assert L.ag_edge_views(None, buf, 1, 4, buf, buf, None, None) == -1 and b"ag_edge_views: null argument" in L.ag_last_error()
    assert L.ag_edge_views(buf, buf, 0, 4, buf, buf, None, None) == -1 and b"bad sizes" in L.ag_last_error()
    assert L.ag_edge_views(buf, buf, 1, 0, buf, buf, None, None) == -1
    assert L.ag_edge_views(buf, buf, 1 << 16, 1 << 15, buf, buf, buf, None) == -1                      # B * N beyond int32
    big = 8193                                                                                       # counters beyond LDS: the workspace holds them
    assert L.ag_edge_views_workspace_bytes(3, 8192) == 0 and L.ag_edge_views_workspace_bytes(3, big) == 3 * big * 4
    assert L.ag_edge_views(buf, buf, 3, big, buf, buf, None, None) != 0 and b"workspace" in L.ag_last_error()


# ------------------------------------------------------------------ the state update and its adjoint, float64
def step_update64(pred, states, delta, rec, repeat, ai, mode, mask, raise_by):
    """The state update in float64 numpy -> (states, rec)."""
    n_p = pred.shape[1]
    rec = np.where((repeat == ai)[:, None, None], pred, rec)
    y = pred[:, :, 1].min(1) if mode == MIN else (pred[:, :, 1] * mask).sum(1) / mask.sum(1)
    new = np.concatenate([pred, states[:, -1, n_p:] + delta[:, n_p:]], 1)
    new[:, n_p:, 1] = (y + raise_by)[:, None]
    return np.concatenate([states[:, 1:], new[:, None]], 1), rec


def step_update_adjoint64(pred, repeat, ai, mode, mask, g_states, g_rec):
    """The adjoint the kernel is held to, in float64 numpy: (g_pred, g_states_in, g_delta, g_rec_in) from the gradients of the two outputs.
    The record's rows go to the prediction; the tool rows' y gradients, summed, to the FIRST particle at the minimum (min mode) or 1 / count
    to every masked-in particle (mean mode); tool x and z pass through to the newest frame and to delta; the shift drops the oldest frame."""
    n_p = pred.shape[1]
    hit = (repeat == ai)[:, None, None]
    g_new = g_states[:, -1]
    g_pred = g_new[:, :n_p] + np.where(hit, g_rec, 0.0)
    G = g_new[:, n_p:, 1].sum(1)
    if mode == MIN:
        g_pred[np.arange(len(pred)), pred[:, :, 1].argmin(1), 1] += G          # (numpy's argmin: the first occurrence)
    else:
        g_pred[:, :, 1] += mask * (G / mask.sum(1))[:, None]
    through = g_new.copy()
    through[:, :n_p] = 0.0
    through[:, :, 1] = 0.0
    g_in = np.zeros_like(g_states)
    g_in[:, 1:] = g_states[:, :-1]
    g_in[:, -1] += through
    return g_pred, g_in, through, np.where(hit, 0.0, g_rec)


def step_case(B, n_p, n_t, H, seed, tie=False):
    rng = np.random.default_rng(seed)
    N = n_p + n_t
    c = dict(pred=rng.normal(0, 1, (B, n_p, 3)), states=rng.normal(0, 1, (B, H, N, 3)), delta=rng.normal(0, 0.1, (B, N, 3)),
             rec=rng.normal(0, 1, (B, n_p, 3)), g_states=rng.normal(0, 1, (B, H, N, 3)), g_rec=rng.normal(0, 1, (B, n_p, 3)))
    c = {k: v.astype(np.float32).astype(np.float64) for k, v in c.items()}      # fp32 values: the GPU tests feed the same numbers to the kernels
    mask = rng.random((B, n_p)) < 0.7
    mask[:, 0] = True
    if B > 1:
        mask[1] = True
    if tie:
        c["pred"][:, :2, 1] = c["pred"][:, :, 1].min() - 1.0                     # particles 0 and 1 share the minimum
    c.update(mask=mask, repeat=np.arange(B).astype(np.int32) + 1)               # sample b records at step b + 1
    return c


@pytest.mark.parametrize("mode", [MIN, MEAN])
@pytest.mark.parametrize("B,n_p,n_t,H,ai,raise_by", [(1, 2, 1, 4, 1, 0.0), (3, 25, 5, 4, 2, 0.1), (2, 65, 1, 1, 7, 0.1), (2, 300, 5, 2, 1, 0.0)])
def test_step_update_adjoint_statement_vs_autograd_of_the_tensor_ops(mode, B, n_p, n_t, H, ai, raise_by):
    c = step_case(B, n_p, n_t, H, seed=B * 100 + n_p)
    t = {k: torch.from_numpy(c[k]).requires_grad_() for k in ("pred", "states", "delta", "rec")}
    rep, mask = torch.from_numpy(c["repeat"]), torch.from_numpy(c["mask"])
    states, rec = step_update_ops(t["pred"], t["states"], t["delta"], t["rec"], rep, ai, mode, mask, raise_by)
    s64, r64 = step_update64(c["pred"], c["states"], c["delta"], c["rec"], c["repeat"], ai, mode, c["mask"], raise_by)
    assert np.abs(states.detach().numpy() - s64).max() <= 1e-14 and np.array_equal(rec.detach().numpy(), r64)
    grads = torch.autograd.grad([states, rec], [t["pred"], t["states"], t["delta"], t["rec"]],
                                [torch.from_numpy(c["g_states"]), torch.from_numpy(c["g_rec"])])
    want = step_update_adjoint64(c["pred"], c["repeat"], ai, mode, c["mask"], c["g_states"], c["g_rec"])
    for name, got, ref in zip(("pred", "states", "delta", "rec"), grads, want):
        assert np.abs(got.numpy() - ref).max() <= 1e-13, name
    assert np.abs(want[1][:, 0]).max() == 0.0 or H == 1                          # nothing reaches the oldest frame through the shift
    assert np.abs(want[2][:, :n_p]).max() == 0.0 and np.abs(want[2][:, :, 1]).max() == 0.0


def test_step_update_adjoint_statement_sends_a_tie_to_the_first_particle():
    c = step_case(2, 9, 5, 4, seed=3, tie=True)
    g_pred = step_update_adjoint64(c["pred"], c["repeat"], 99, MIN, c["mask"], c["g_states"], np.zeros_like(c["g_rec"]))[0]
    G = c["g_states"][:, -1, 9:, 1].sum(1)
    assert np.allclose(g_pred[:, 0, 1] - c["g_states"][:, -1, 0, 1], G) and np.array_equal(g_pred[:, 1, 1], c["g_states"][:, -1, 1, 1])


def test_block_sum_is_the_workgroup_order():
    """256 strided partials, the xor butterfly of each wave, (w0 + w1) + (w2 + w3): spelled out with Python floats rounded to fp32."""
    rng = np.random.default_rng(0)
    for n in (1, 65, 256, 700):
        x = (rng.normal(0, 1, (2, n)) * 10.0 ** rng.integers(-3, 4, (2, n))).astype(np.float32)
        got = block_sum(torch.from_numpy(x)).numpy()
        for b in range(2):
            part = np.zeros(256, np.float32)
            for i in range(n):
                part[i % 256] = np.float32(part[i % 256] + x[b, i])
            v = part.reshape(4, 64)
            for o in (32, 16, 8, 4, 2, 1):
                v = (v + v[:, np.arange(64) ^ o]).astype(np.float32)
            w = v[:, 0]
            assert got[b] == np.float32(np.float32(w[0] + w[1]) + np.float32(w[2] + w[3]))


def test_step_update_entry_points_reject_bad_arguments():
    L = _lib.lib()
    f = (ctypes.c_float * 64)()
    i = (ctypes.c_int32 * 4)()
    m = (ctypes.c_uint8 * 16)()
    ok = dict(B=1, H=4, N=3, n_p=2)
    fwd = lambda mode=MIN, mask=None, **kw: L.ag_step_update_forward(f, f, f, None, i, mask, *[{**ok, **kw}[k] for k in ("B", "H", "N", "n_p")], 1,
                                                                     mode, 0.0, f, f, None)
    bwd = lambda mode=MIN, mask=None, **kw: L.ag_step_update_backward(f, i, mask, *[{**ok, **kw}[k] for k in ("B", "H", "N", "n_p")], 1, mode, f, f,
                                                                      f, f, f, f, None)
    for call in (fwd, bwd):
        assert call(B=0) == -1 and b"bad sizes" in L.ag_last_error()
        assert call(H=0) == -1 and call(n_p=0) == -1 and call(N=1) == -1                              # tool rows: N >= n_p
        assert call(mode=2) == -1 and b"height_mode" in L.ag_last_error()
        assert call(mode=MEAN) == -1 and b"needs obj_mask" in L.ag_last_error()
    assert L.ag_step_update_forward(None, f, f, None, i, m, 1, 4, 3, 2, 1, MEAN, 0.0, f, f, None) == -1 and b"null argument" in L.ag_last_error()
    assert L.ag_step_update_backward(f, i, m, 1, 4, 3, 2, 1, MEAN, None, f, f, f, f, f, None) == -1 and b"null argument" in L.ag_last_error()


# ------------------------------------------------------------------ optimize(method=...)
def test_optimize_checks_its_method_before_any_gpu_work():
    from adaptigraph_amd import physics_param_optimizer as ppo
    ns = configs.ppm_optimizer_stub("rope", {"rope": torch.tensor([0.5])})
    ns.device = "cuda:0"                                                          # never touched: the check comes first
    data = ([np.zeros(4, np.float32)], [np.zeros((3, 3), np.float32)], None, [np.zeros((3, 3), np.float32)])
    with pytest.raises(ValueError, match="method='newton'"):
        ppo.optimize(ns, *data, method="newton")
    with pytest.raises(ValueError, match="n_starts"):
        ppo.optimize(ns, *data, method="gd", n_starts=-1)
    with pytest.raises(ValueError, match="method='bo'"):
        ppo.PhysicsParamOnlineOptimizer(configs.task_config("rope"), None, "rope", "cpu", ".", method="bo")
    assert ppo.METHODS == ("sweep", "gd")
    assert ppo.PhysicsParamOnlineOptimizer(configs.task_config("rope"), None, "rope", "cpu", ".").method == "sweep"
    xs = ppo._first_generation(1, 60, np.array([0.5]), 42)
    assert xs.shape == (20, 1) and xs[0, 0] == ppo.PARAM_LO and xs[-1, 0] == ppo.PARAM_HI
    xs = ppo._first_generation(2, 60, np.array([0.5, 0.5]), 42)
    assert xs.shape == (12, 2) and xs.min() >= ppo.PARAM_LO and xs.max() <= ppo.PARAM_HI
