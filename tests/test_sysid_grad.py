"""Sys-id by gradient on the MI355X: `ag_edge_views` against the torch arrays of `EdgeViews`, `ag_step_update_forward / _backward` against the tensor
ops of the drivers and the float64 adjoint of tests/test_sysid_grad_cpu.py, `dynamics_masked_differentiable` against `dynamics_masked` and a
float64 CPU restatement of the masked rollout on the same edge lists, `checkpoint_steps`, and `optimize(method="gd")` against the sweep."""
import os

import numpy as np
import pytest
import torch

from adaptigraph_amd import _lib, configs, graph, losses, synth, train_ops
from adaptigraph_amd import forward_dynamics as fd
from adaptigraph_amd.plan_utils import decode_action
from oracle import ag_oracle as ago
from test_grad_rollout import _step64
from test_sysid_grad_cpu import MEAN, MIN, edge_views_np, step_case, step_update_adjoint64

DEV = "cuda:0"


def tg(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------ ag_edge_views
EDGE_CASES = {   # material, particles, samples, radius, topk, connect_tools_all, emptied sample
    "rope-24 x 3": ("rope", 24, 3, 0.5, 10, False, None),
    "granular-70, 5 tools, x 2": ("granular", 70, 2, 0.4, 20, False, None),
    "cloth-36, connect_tools_all": ("cloth", 36, 2, 0.75, 5, True, None),
    "N = 257": ("rope", 256, 2, 0.5, 10, False, None),
    "second sample without edges": ("rope", 24, 3, 0.5, 10, False, 1),
    "N = 8201: counters in the workspace": ("rope", 8200, 1, 0.5, 5, False, None),
}


def _edges(case):
    mat, n, B, radius, topk, connect, emptied = EDGE_CASES[case]
    g = synth.make_graph_inputs(mat, n, B, seed=7, spacing=0.1)
    mask = g["mask"].copy()
    if emptied is not None:
        mask[emptied] = False
    return graph.build_edges(tg(g["state"][:, -1]), radius, tg(mask), tg(g["tool_mask"]), topk, connect, "batch", max_tools=g["n_tools"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_edge_views_on_the_device_are_the_torch_arrays(case):
    csr = _edges(case)
    ref = train_ops.EdgeViews(csr)
    got, again = train_ops.EdgeViews(csr, device_views=True), train_ops.EdgeViews(csr, device_views=True)
    assert got.E == ref.E and (ref.E > 0 or case.startswith("second"))
    for v in (got, again):
        assert v.send_perm.dtype == torch.int32 and v.col_ptr.dtype == torch.int32 and v.send_perm.is_contiguous()
        assert torch.equal(v.send_perm, ref.send_perm) and torch.equal(v.col_ptr, ref.col_ptr)
        assert torch.equal(v.recv, ref.recv) and torch.equal(v.send, ref.send) and torch.equal(v.row_ptr, ref.row_ptr)
    perm, col_ptr = edge_views_np(csr.row_ptr.cpu().numpy(), csr.edge_send.cpu().numpy(), csr.B, csr.N)
    assert np.array_equal(got.send_perm.cpu().numpy(), perm) and np.array_equal(got.col_ptr.cpu().numpy(), col_ptr)
    if case.startswith("second"):
        n_rel = csr.n_rel().cpu().numpy()
        assert n_rel[1] == 0 and n_rel[0] > 0 and n_rel[2] > 0


@pytest.mark.gpu
def test_edge_views_replay_in_a_captured_graph():
    csr = _edges("granular-70, 5 tools, x 2")
    ref = train_ops.EdgeViews(csr)
    dev = csr.row_ptr.device
    perm = torch.full((csr.edge_send.numel(),), -1, dtype=torch.int32, device=dev)
    col_ptr = torch.full((csr.B * csr.N + 1,), -1, dtype=torch.int32, device=dev)
    ws = torch.empty(256, dtype=torch.uint8, device=dev)
    run = lambda: _lib.call("ag_edge_views", dev, csr.row_ptr, csr.edge_send, csr.B, csr.N, col_ptr, perm, ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for _ in range(3):
        perm.fill_(-1)
        col_ptr.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(perm[:ref.E], ref.send_perm) and torch.equal(col_ptr, ref.col_ptr)


# ------------------------------------------------------------------ the state update
STEP_SHAPES = [(1, 2, 1), (3, 25, 5), (2, 65, 1), (2, 700, 5)]      # B, particles, tools; the last: more than one chunk, strided partial sums


def _step_tensors(c, grad=False):
    t = {k: tg(c[k].astype(np.float32)) for k in ("pred", "states", "delta", "rec", "g_states", "g_rec")}
    if grad:
        for k in ("pred", "states", "delta", "rec"):
            t[k].requires_grad_()
    return t, tg(c["repeat"]), tg(c["mask"])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [MIN, MEAN])
@pytest.mark.parametrize("raise_by", [0.0, 0.1])
@pytest.mark.parametrize("B,n_p,n_t", STEP_SHAPES)
def test_step_update_forward_is_the_tensor_ops(mode, raise_by, B, n_p, n_t):
    c = step_case(B, n_p, n_t, 4, seed=n_p)
    t, rep, mask = _step_tensors(c)
    for ai in (1, B, 99):                                   # repeat = 1 .. B: the first step's sample, the last step's, nobody
        want = fd.step_update_ops(t["pred"], t["states"], t["delta"], t["rec"], rep, ai, mode, mask, raise_by)
        got = fd.step_update(t["pred"], t["states"], t["delta"], t["rec"], rep, ai, mode, mask, raise_by)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), ai
        assert int((rep == ai).sum()) == (0 if ai == 99 else 1)
        hit = (rep == ai)[:, None, None]
        assert torch.equal(got[1], torch.where(hit, t["pred"], t["rec"]))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [MIN, MEAN])
@pytest.mark.parametrize("B,n_p,n_t", STEP_SHAPES[:3])
def test_step_update_backward_vs_float64_adjoint(mode, B, n_p, n_t):
    """Every output element is a sum of at most n_t + 4 terms (the newest frame's gradient, the record's, the n_t tool rows' y gradients in G,
    and in mean mode the division by the count): one fp32 rounding per term, n_terms * 2^-23 * max|term|."""
    c = step_case(B, n_p, n_t, 4, seed=n_p + 1)
    for ai in (1, 99):
        t, rep, mask = _step_tensors(c, grad=True)
        out = fd.step_update(t["pred"], t["states"], t["delta"], t["rec"], rep, ai, mode, mask, 0.1)
        ins = [t[k] for k in ("pred", "states", "delta", "rec")]
        got = torch.autograd.grad(out, ins, [t["g_states"], t["g_rec"]], retain_graph=True)
        again = torch.autograd.grad(out, ins, [t["g_states"], t["g_rec"]])
        want = step_update_adjoint64(c["pred"], c["repeat"], ai, mode, c["mask"], c["g_states"], c["g_rec"])
        G = np.abs(c["g_states"][:, -1, n_p:, 1].sum(1)).max()
        bound = (n_t + 4) * 2.0 ** -23 * max(np.abs(c["g_states"]).max(), np.abs(c["g_rec"]).max(), G)
        for name, a, b, ref in zip(("pred", "states", "delta", "rec"), got, again, want):
            assert torch.equal(a, b), name                                       # one fixed order: the same bits on every call
            err = np.abs(a.cpu().numpy().astype(np.float64) - ref).max()
            print(f"step update backward {name}: B={B} n_p={n_p} mode={mode} ai={ai} err={err:.3e} bound={bound:.3e}")
            assert a.shape == ref.shape and err <= bound, (name, err, bound)


@pytest.mark.gpu
def test_step_update_backward_sends_a_tie_to_particle_0():
    c = step_case(2, 9, 5, 4, seed=3, tie=True)
    t, rep, mask = _step_tensors(c, grad=True)
    assert bool((t["pred"][:, 0, 1] == t["pred"][:, 1, 1]).all()) and bool((t["pred"][:, 2:, 1] > t["pred"][:, :1, 1]).all())
    out = fd.step_update(t["pred"], t["states"], t["delta"], t["rec"], rep, 99, MIN, None, 0.0)
    g_states = torch.zeros_like(t["states"])
    g_states[:, -1, 9:, 1] = 1.0                                                  # only the tool height carries gradient
    g_pred, = torch.autograd.grad(out[0], t["pred"], g_states)
    want = torch.zeros_like(g_pred)
    want[:, 0, 1] = 5.0
    assert torch.equal(g_pred, want)


# ------------------------------------------------------------------ the masked differentiable rollout
@pytest.fixture
def exact_chains():
    prev = train_ops.CHAIN_PRECISION
    train_ops.CHAIN_PRECISION = 0                          # exact fp32 MFMA in the differentiable path (the engine side: precision 0)
    yield
    train_ops.CHAIN_PRECISION = prev


W0 = "particle_encoder.model.0.weight"


def _weights2(weights):
    """The seed-0 set with a second physics column in the first node layer: a seeded permutation of the first (tests/test_model_configs.py)."""
    w = {k: v.copy() for k, v in weights.items()}
    w[W0] = np.insert(w[W0], 3, w[W0][np.random.default_rng(2).permutation(w[W0].shape[0]), 2], axis=1)
    return w


def _material_config(mat, dims):
    params = [{"name": "particle_radius", "use": False, "min": 0.0, "max": 1.0}]
    params += [{"name": f"param{i}", "use": True, "min": 0.0, "max": 1.0} for i in range(dims)]
    return {"material_index": {mat: 0}, mat: {"physics_params": params}}


def _model(weights, mat, dims=1):
    from adaptigraph_amd.model import DynamicsPredictor
    m = DynamicsPredictor(configs.model_config(), _material_config(mat, dims), configs.dataset_config(mat), DEV)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in (weights if dims == 1 else _weights2(weights)).items()})
    return m.to(DEV).eval().set_option("precision", 0)


def _ppm(mat, dims=1):
    ppm = configs.ppm_optimizer_stub(mat)
    ppm.material_dims = {mat: dims}
    ppm.task_config["material_dims"] = {mat: dims}
    ppm.physics_param = {mat: torch.full((dims,), 0.5, device=DEV)}
    return ppm


def _masked_inputs(mat, n, bsz, seed, len_lo, len_hi):
    """bsz start clouds of n slots with different valid counts (n, n - 3, n - 7, ..; padding rows zero) and one push each of len_lo .. len_hi steps."""
    obj, act = synth.make_mpc_inputs(mat, n, bsz, n_look=1, seed=seed, len_lo=len_lo, len_hi=len_hi, spacing=0.1)
    rng = np.random.default_rng(seed + 100)
    state, mask = np.zeros((bsz, n, 3), np.float32), np.zeros((bsz, n), bool)
    for b in range(bsz):
        c = n - (0, 3, 7, 2, 5, 1, 6, 4)[b % 8]
        state[b, :c] = obj[:c] + rng.normal(0, 0.003, (c, 3)).astype(np.float32)
        mask[b, :c] = True
    return state, mask, act[:, 0].copy()


ROLLOUT_CASES = [("rope", 20, 31), ("granular", 30, 32)]      # material, particle slots, seed; bsz 3, pushes of 2 .. 4 steps


@pytest.mark.gpu
@pytest.mark.parametrize("mat,n,seed", ROLLOUT_CASES)
def test_dynamics_masked_differentiable_values_match_dynamics_masked(weights, exact_chains, mat, n, seed):
    state, mask, act = _masked_inputs(mat, n, 3, seed, 2.0, 4.9)
    model, ppm = _model(weights, mat), _ppm(mat)
    phys = {mat: tg(np.array([[0.3], [0.5], [0.8]], np.float32))}
    ref = fd.dynamics_masked(tg(state), tg(mask), tg(act), model, DEV, ppm, physics_param=phys)
    a = tg(act).requires_grad_()
    got = fd.dynamics_masked_differentiable(tg(state), tg(mask), a, model, DEV, ppm, physics_param=phys)
    assert set(got) == set(ref) and got["state_seqs"].requires_grad and got["state_seqs"].shape == ref["state_seqs"].shape
    assert len(set(a[:, 3].int().tolist())) > 1                                   # the samples' pushes differ in length
    assert torch.equal(got["action_seqs"].detach(), ref["action_seqs"])
    assert float((got["state_seqs"].detach() - ref["state_seqs"]).abs().max()) <= 1e-4


def _rollout_masked64(W, task, state, mask, action, phys, edge_log, check_edges=True):
    """dynamics_masked_differentiable restated in float64 on the CPU on the recorded edge lists (one entry per model step): state (B,n,3),
    mask (B,n) numpy bool, action (B,4), phys (B,d).  check_edges: the oracle's edge builder on THIS rollout's states gives the same lists."""
    n_his, ratio = task["n_his"], task["sim_real_ratio"]
    bsz, n_obj = state.shape[0], state.shape[1]
    n_t = task["eef_num"]
    N = n_obj + n_t
    decoded, repeat = decode_action(action[:, None], push_length=task["push_length"])
    d, repeat, th = decoded[:, 0], repeat[:, 0], action[:, 2]
    m = torch.from_numpy(mask).double()
    cnt = m.sum(1)
    raise_by = 0.01 * ratio if task["gripper_enable"] else 0.0
    height = lambda s: (s[:, :, 1] * m).sum(1) / cnt + raise_by
    offs = [float(p[1]) * ratio for p in task["pusher_points"]]
    y = height(state)
    if n_t == 1:
        eef = torch.stack([d[:, 0], y, d[:, 1]], -1)[:, None]
    else:
        eef = torch.stack([torch.stack([d[:, 0] + o * torch.sin(th) if i else d[:, 0], y, d[:, 1] - o * torch.cos(th) if i else d[:, 1]], -1)
                           for i, o in enumerate(offs)], 1)
    dlt = torch.stack([d[:, 2] - d[:, 0], torch.zeros_like(y), d[:, 3] - d[:, 1]], -1)[:, None].expand(bsz, n_t, 3)
    states = torch.cat([state[:, None].expand(bsz, n_his, n_obj, 3), eef[:, None].expand(bsz, n_his, n_t, 3)], 2)
    delta = torch.cat([torch.zeros((bsz, n_obj, 3), dtype=torch.float64), dlt], 1)
    attrs = torch.zeros((bsz, N, 2), dtype=torch.float64)
    attrs[:, :n_obj, 0] = m
    attrs[:, n_obj:, 1] = 1
    p_inst = torch.zeros((bsz, n_obj, task["max_n"]), dtype=torch.float64)
    p_inst[:, :, 0] = (torch.arange(n_obj)[None] < cnt[:, None]).double()
    full, tmask = np.ones((bsz, N), bool), np.zeros((bsz, N), bool)
    full[:, :n_obj] = mask
    tmask[:, n_obj:] = True
    rec = torch.zeros((bsz, n_obj, 3), dtype=torch.float64)
    n_steps = int(repeat.max())
    own = edge_log is None                                  # (the restatement on its own graphs: a CPU-only check of this function)
    edge_log = [None] * n_steps if own else edge_log
    assert n_steps == len(edge_log)
    for ai in range(1, 1 + n_steps):
        if check_edges or own:
            n_rel, recv, send = ago.build_edges(states[:, -1].detach().float().numpy(), task["adj_thresh"], full, tmask, task["topk"],
                                                task["connect_tools_all"], "batch")
            if own:
                edge_log[ai - 1] = [(recv[b, :n_rel[b]], send[b, :n_rel[b]]) for b in range(bsz)]
            for b in range(bsz):
                assert np.array_equal(recv[b, :n_rel[b]], edge_log[ai - 1][b][0]) and np.array_equal(send[b, :n_rel[b]], edge_log[ai - 1][b][1]), \
                    f"edge lists differ at model step {ai}, sample {b}"
        pred = _step64(W, states, attrs, p_inst, delta, phys, edge_log[ai - 1])
        rec = torch.where((repeat == ai)[:, None, None], pred, rec)
        tool = states[:, -1, n_obj:] + delta[:, n_obj:]
        tool = torch.stack([tool[..., 0], height(pred)[:, None].expand(bsz, n_t), tool[..., 2]], -1)
        states = torch.cat([states[:, 1:], torch.cat([pred, tool], 1)[:, None]], 1)
    return rec


def _masked_chamfer64(x, y, xm, ym):
    out = []
    for b in range(x.shape[0]):
        d = torch.cdist(y[b][torch.from_numpy(ym[b])], x[b][torch.from_numpy(xm[b])])
        out.append(d.min(1).values.mean() + d.min(0).values.mean())
    return torch.stack(out)


@pytest.mark.gpu
@pytest.mark.parametrize("mat,n,seed", ROLLOUT_CASES)
def test_masked_rollout_gradients_vs_float64_restatement(weights, exact_chains, monkeypatch, mat, n, seed):
    task = configs.task_config(mat)
    state, mask, act = _masked_inputs(mat, n, 3, seed, 2.0, 4.9)
    target = state[:, ::2] + np.array([0.3, 0.0, 0.2], np.float32)
    tmask = mask[:, ::2]
    wts = np.array([1.0, 0.7, 1.3])
    phys0 = np.array([[0.3], [0.5], [0.8]], np.float32)
    model, ppm = _model(weights, mat), _ppm(mat)
    log, build = [], graph.build_edges

    def recording_build(*a, **kw):
        csr = build(*a, **kw)
        log.append(csr.to_lists())
        return csr
    monkeypatch.setattr(graph, "build_edges", recording_build)
    S, A, P = tg(state).requires_grad_(), tg(act).requires_grad_(), tg(phys0).requires_grad_()
    out = fd.dynamics_masked_differentiable(S, tg(mask), A, model, DEV, ppm, physics_param={mat: P})
    err = losses.mean_chamfer_device(out["state_seqs"], tg(target), tg(mask), tg(tmask))
    gs, ga, gp = torch.autograd.grad((err * tg(wts.astype(np.float32))).sum(), [S, A, P])
    monkeypatch.setattr(graph, "build_edges", build)

    W = {k: torch.from_numpy(v).double() for k, v in weights.items()}
    S64, A64, P64 = (torch.from_numpy(x).double().requires_grad_() for x in (state, act, phys0))
    T64 = torch.from_numpy(target).double()

    def loss64(S_, A_, P_):
        seq = _rollout_masked64(W, task, S_, mask, A_, P_, log)
        return seq, (_masked_chamfer64(seq, T64, mask, tmask) * torch.from_numpy(wts)).sum()
    seq64, l64 = loss64(S64, A64, P64)
    assert float((out["state_seqs"].detach().cpu().double() - seq64.detach())[torch.from_numpy(mask)].abs().max()) <= 1e-4
    gs64, ga64, gp64 = torch.autograd.grad(l64, [S64, A64, P64])
    for name, got, ref in (("state_init", gs, gs64), ("action", ga, ga64), ("physics_param", gp, gp64)):
        e, scale = float((got.cpu().double() - ref).abs().max()), float(ref.abs().max())
        print(f"masked rollout gradient {mat} {name}: err={e:.3e} max|ref|={scale:.3e}")
        assert scale > 0 and e <= 1e-3 * scale, (name, e, scale)
    assert float(gs[~tg(mask)].abs().max()) == 0.0 and float(gs64[~torch.from_numpy(mask)].abs().max()) == 0.0      # masked-in rows only
    assert float(ga[:, 3].abs().max()) == 0.0 and all(float(ga[:, c].abs().max()) > 0.0 for c in range(3))          # the length only counts steps
    # central differences of the restatement, and no edge list changes under them (checked inside the rollout, step by step)
    for which, idx, ref in ((0, (1, 2, 0), gs64), (1, (2, 0), ga64), (1, (0, 2), ga64), (2, (0, 0), gp64)):
        h, vals = 1e-6, []
        for sign in (1.0, -1.0):
            args = [S64.detach().clone(), A64.detach().clone(), P64.detach().clone()]
            args[which][idx] += sign * h
            with torch.no_grad():
                vals.append(float(loss64(*args)[1]))
        fdiff = (vals[0] - vals[1]) / (2 * h)
        assert abs(fdiff - float(ref[idx])) <= 1e-6 + 1e-4 * abs(fdiff), (which, idx, fdiff, float(ref[idx]))


# ------------------------------------------------------------------ checkpoint_steps
def _grads(out, leaves, w):
    return torch.autograd.grad((out["state_seqs"] * w).sum(), leaves)


@pytest.mark.gpu
def test_checkpoint_steps_keeps_every_bit_in_both_drivers(weights, exact_chains):
    mat = "rope"
    model, ppm = _model(weights, mat), _ppm(mat)
    state, mask, act = _masked_inputs(mat, 30, 3, 41, 4.0, 4.9)                  # 4 model steps
    w = tg(np.random.default_rng(1).normal(0, 1, (3, 30, 3)).astype(np.float32))
    res = []
    for ck in (False, True):
        S, A, P = tg(state).requires_grad_(), tg(act).requires_grad_(), torch.tensor([[0.3], [0.5], [0.8]], device=DEV, requires_grad=True)
        out = fd.dynamics_masked_differentiable(S, tg(mask), A, model, DEV, ppm, physics_param={mat: P}, checkpoint_steps=ck)
        res.append((out["state_seqs"].detach(),) + _grads(out, [S, A, P], w))
    assert all(torch.equal(a, b) for a, b in zip(*res)) and float(res[0][3].abs().max()) > 0
    res = []
    for ck in (False, True):
        A, P = tg(act[:, None]).requires_grad_(), torch.tensor([0.4], device=DEV, requires_grad=True)
        ppm.physics_param = {mat: P}
        out = fd.dynamics_differentiable(tg(state[0]), A, model, DEV, ppm, checkpoint_steps=ck)
        res.append((out["state_seqs"].detach(),) + _grads(out, [A, P], w[:, None]))
    assert all(torch.equal(a, b) for a, b in zip(*res)) and float(res[0][2].abs().max()) > 0


@pytest.mark.gpu
def test_checkpoint_steps_needs_less_memory(weights):
    mat = "rope"
    model, ppm = _model(weights, mat), _ppm(mat)
    state, mask, act = _masked_inputs(mat, 60, 8, 42, 6.0, 6.9)                  # 6 model steps, bsz 8
    peak = {}
    for ck in (False, True, False, True):                                        # (the first pair also warms caches and workspaces up)
        P = torch.full((8, 1), 0.5, device=DEV, requires_grad=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        out = fd.dynamics_masked_differentiable(tg(state), tg(mask), tg(act), model, DEV, ppm, physics_param={mat: P}, checkpoint_steps=ck)
        out["state_seqs"].square().sum().backward()
        torch.cuda.synchronize()
        peak[ck] = torch.cuda.max_memory_allocated()
        del out, P
    print(f"peak bytes, forward + backward, 6 steps x 8 samples x 61 nodes: plain {peak[False]}, checkpoint_steps {peak[True]}")
    assert peak[True] < peak[False], peak


# ------------------------------------------------------------------ identification
def _interactions(model, ppm, mat, planted, n=40, n_int=4, seed=51):
    """n_int interactions of <= n particles whose observed clouds come from dynamics_masked at the planted parameter."""
    state, mask, act = _masked_inputs(mat, n, n_int, seed, 2.0, 4.9)
    phys = {mat: torch.tensor(planted, dtype=torch.float32, device=DEV)}
    real = fd.dynamics_masked(tg(state), tg(mask), tg(act), model, DEV, ppm, physics_param=phys)["state_seqs"].cpu().numpy()
    counts = mask.sum(1)
    return [act[i] for i in range(n_int)], [state[i, :counts[i]] for i in range(n_int)], [real[i, :counts[i]] for i in range(n_int)]


def _online(weights, mat, dims, save_dir, method):
    from adaptigraph_amd.physics_param_optimizer import PhysicsParamOnlineOptimizer
    task = dict(configs.task_config(mat), max_nobj=40, material_dims={mat: dims})
    return PhysicsParamOnlineOptimizer(task, _model(weights, mat, dims), mat, DEV, save_dir, method=method)


ITERATIONS = 30


@pytest.mark.gpu
def test_gd_recovers_a_planted_parameter_no_worse_than_the_sweep(weights, exact_chains, tmp_path):
    from adaptigraph_amd import physics_param_optimizer as ppo
    ppm = _online(weights, "rope", 1, str(tmp_path), "gd")
    acts, inits, reals = _interactions(ppm.model, ppm, "rope", [0.3])
    _, err_sweep, err0 = ppo.optimize(ppm, acts, inits, reals, reals, iterations=ITERATIONS, method="sweep")
    for i in range(4):
        np.savez(os.path.join(tmp_path, f"interaction_{i}.npz"), act=acts[i], state_init=inits[i], state_pred=reals[i], state_real=reals[i])
    p, err, err_init = ppm.optimize(3, iterations=ITERATIONS)                    # method="gd" through the file contract
    print(f"1-D identification: planted 0.3, gd {float(p[0]):.5f} error {err:.3e}; sweep error {err_sweep:.3e}; initial {err_init:.3e}")
    assert err_init == err0 and err <= err_sweep
    assert abs(float(p[0]) - 0.3) <= 0.02
    assert abs(float(ppm.physics_param["rope"][0]) - float(p[0])) < 1e-6
    saved = np.load(os.path.join(tmp_path, "ppo_3.npz"))
    assert set(saved.files) == {"physics_param", "error", "error_init"} and float(saved["error"]) == err


@pytest.mark.gpu
def test_gd_on_two_parameters_is_no_worse_than_the_sweep(weights, exact_chains, tmp_path):
    from adaptigraph_amd import physics_param_optimizer as ppo
    ppm = _online(weights, "rope", 2, str(tmp_path), "gd")
    acts, inits, reals = _interactions(ppm.model, ppm, "rope", [0.3, 0.7])
    _, err_sweep, _ = ppo.optimize(ppm, acts, inits, reals, reals, iterations=ITERATIONS, method="sweep")
    p, err, err0, res = ppo.optimize(ppm, acts, inits, reals, reals, iterations=ITERATIONS, method="gd", return_res=True)
    print(f"2-D identification: planted (0.3, 0.7), gd ({float(p[0]):.5f}, {float(p[1]):.5f}) error {err:.3e}; sweep error {err_sweep:.3e}; initial {err0:.3e}")
    assert err <= err_sweep and err <= err0
    assert res["x_iters"].shape[1] == 2 and len(res["x_iters"]) == len(res["func_vals"]) >= ITERATIONS
    assert res["x_iters"].min() >= ppo.PARAM_LO and res["x_iters"].max() <= ppo.PARAM_HI
