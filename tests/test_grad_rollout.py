"""Differentiable planning on the MI355X: the HIP chamfer backward (ag_chamfer_fwd_idx / ag_chamfer_backward) against float64 torch
autograd, `dynamics_differentiable` against the engine's `dynamics`, its action / physics gradients against a float64 CPU restatement
of the rollout on the same edge lists, and `GradientPlanner` on a rope."""
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adaptigraph_amd import configs, graph, losses, mpc, synth, train_ops
from adaptigraph_amd.forward_dynamics import dynamics, dynamics_differentiable
from adaptigraph_amd.plan_utils import decode_action
from oracle import ag_oracle as ago

DEV = "cuda:0"


def tg(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------ chamfer backward
_OFF = np.array([0.1, 0.15, 0.05])


def _pt(rng, c, off):
    return (np.stack([c // 400, (c // 20) % 20, c % 20], -1) + off + rng.uniform(-0.005, 0.005, (len(c), 3))).astype(np.float32)


def _clouds(rng, B, N, M, batched):
    """x (B,N,3) and y (B|1,M,3) on distinct cells of a 20^3 lattice (y offset by _OFF, +- 0.005 jitter), within a sample the smaller
    cloud's cells a subset of the larger's: every nearest neighbour is far ahead of the second (the reference check asserts it)."""
    if not batched:                                          # one target cloud: every sample's particles sit on cells of it
        assert N <= M
        cy = rng.choice(8000, M, replace=False)
        return np.stack([_pt(rng, cy[rng.choice(M, N, replace=False)], 0.0) for _ in range(B)]), _pt(rng, cy, _OFF)[None]
    xs, ys = [], []
    for _ in range(B):
        cells = rng.choice(8000, max(N, M), replace=False)
        cx, cy = (cells, cells[rng.choice(len(cells), M, replace=False)]) if N >= M else (cells[rng.choice(len(cells), N, replace=False)], cells)
        xs.append(_pt(rng, cx, 0.0))
        ys.append(_pt(rng, cy, _OFF))
    return np.stack(xs), np.stack(ys)


def _ref_grads(x, y, xm, ym, w):
    """float64 autograd of sum_b w_b chamfer_b (losses.py:4-24 on the masked-in points); the min's argmin found in float64, with the
    near-tie check.  -> (gx (B,N,3), gy (By,M,3)) numpy."""
    B = x.shape[0]
    X = torch.from_numpy(x).double().requires_grad_()
    Y = torch.from_numpy(y).double().requires_grad_()
    loss = 0
    for b in range(B):
        by = b if y.shape[0] == B else 0
        ix, iy = np.nonzero(xm[b])[0], np.nonzero(ym[by])[0]
        if len(ix) == 0 or len(iy) == 0:
            continue
        xb, yb = X[b, ix], Y[by, iy]
        with torch.no_grad():
            d = torch.cdist(yb, xb)                          # (My, Nx)
            for dd in (d, d.t()):
                if dd.shape[1] > 1:
                    two = dd.topk(2, dim=1, largest=False).values
                    assert float(((two[:, 1] ** 2 - two[:, 0] ** 2)).min()) > 1e-3, "near-tie in the test data"
            nn_y, nn_x = d.argmin(1), d.argmin(0)
        cy = torch.linalg.vector_norm(yb - xb[nn_y], dim=-1).mean()
        cx = torch.linalg.vector_norm(xb - yb[nn_x], dim=-1).mean()
        loss = loss + w[b] * (cx + cy)
    gx, gy = torch.autograd.grad(loss, [X, Y], allow_unused=True) if torch.is_tensor(loss) else (None, None)
    gx = np.zeros_like(x, np.float64) if gx is None else gx.numpy()
    gy = np.zeros_like(y, np.float64) if gy is None else gy.numpy()
    return gx, gy


CHAMFER_CASES = [  # B, N, M, y batched, masked, coincident points
    (1, 37, 53, True, False, False), (7, 211, 97, True, False, True), (7, 1, 1, False, False, False), (7, 300, 1, True, False, False),
    (1, 6399, 6401, False, False, False), (7, 129, 255, False, False, True), (7, 150, 140, True, True, False), (1, 1, 500, True, True, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,M,batched,masked,coincide", CHAMFER_CASES)
def test_chamfer_backward_vs_float64_autograd(B, N, M, batched, masked, coincide):
    rng = np.random.default_rng(N * 7 + M + B)
    By = B if batched else 1
    x, y = _clouds(rng, B, N, M, batched)
    if coincide:
        y[0, 0] = x[0, 0]                                   # a zero-length pair: u(0) = 0
    xm = np.ones((B, N), bool)
    ym = np.ones((By, M), bool)
    if masked:
        xm = rng.random((B, N)) < 0.7
        ym = rng.random((By, M)) < 0.7
        xm[:, 0] = ym[:, 0] = True
        if B > 1:
            xm[1] = False                                   # an empty row: NaN value, zero gradient
            ym[min(2, By - 1)] = False
    w = rng.uniform(0.5, 2.0, B)
    X, Y = tg(x).requires_grad_(), tg(y).requires_grad_()
    if masked:
        out = losses.mean_chamfer_device(X, Y, tg(xm), tg(ym))
        with torch.no_grad():
            ref_val = losses.mean_chamfer_device(X, Y, tg(xm), tg(ym))
    else:
        out = losses.chamfer(X, Y)
        with torch.no_grad():
            ref_val = losses.chamfer(X, Y)
    assert torch.equal(out.detach(), ref_val) or torch.equal(out.detach().nan_to_num(7.0), ref_val.nan_to_num(7.0))
    gx, gy = torch.autograd.grad(out, [X, Y], grad_outputs=tg(w.astype(np.float32)), retain_graph=True)
    gx2, gy2 = torch.autograd.grad(out, [X, Y], grad_outputs=tg(w.astype(np.float32)))
    assert torch.equal(gx, gx2) and torch.equal(gy, gy2)                       # no atomics: the same bits every call
    rx, ry = _ref_grads(x, y, xm, ym, w)
    for got, ref in ((gx.cpu().numpy(), rx), (gy.cpu().numpy(), ry)):
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max() + 1e-12, (np.abs(got - ref).max(), np.abs(ref).max())
    if masked and B > 1:
        assert not torch.isfinite(out[1]) and float(gx[1].abs().max()) == 0.0


@pytest.mark.gpu
def test_chamfer_grad_entry_points_keep_the_limit():
    x = torch.zeros((1, 6401, 3), device=DEV, requires_grad=True)
    y = torch.zeros((1, 6400, 3), device=DEV)
    with pytest.raises(RuntimeError, match="LDS-resident limit"):
        losses.chamfer(x, y)


# ------------------------------------------------------------------ rollout values and gradients
@pytest.fixture
def exact_chains():
    prev = train_ops.CHAIN_PRECISION
    train_ops.CHAIN_PRECISION = 0                          # exact fp32 MFMA in the differentiable path (the engine side: precision 0)
    yield
    train_ops.CHAIN_PRECISION = prev


def _model(weights, mat):
    from adaptigraph_amd.model import DynamicsPredictor
    m = DynamicsPredictor(configs.model_config(), configs.material_config(mat), configs.dataset_config(mat), DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    return m.to(DEV).eval().set_option("precision", 0)


def _ppm(mat, phys):
    ppm = configs.ppm_optimizer_stub(mat)
    ppm.physics_param = {mat: phys}
    return ppm


ROLLOUT_CASES = [("rope", 60, 2, 1, 3.9, 0.1, 3), ("granular", 80, 1, 1, 3.9, 0.1, 4), ("cloth", 81, 2, 1, 2.9, 0.1, 5), ("rope", 200, 1, 1, 2.9, 0.1, 6)]


@pytest.mark.gpu
@pytest.mark.parametrize("mat,n,n_look,len_lo,len_hi,spacing,seed", ROLLOUT_CASES)
def test_dynamics_differentiable_values_match_dynamics(weights, exact_chains, mat, n, n_look, len_lo, len_hi, spacing, seed):
    state, act = synth.make_mpc_inputs(mat, n, 6, n_look=n_look, seed=seed, len_lo=len_lo, len_hi=len_hi, spacing=spacing)
    model = _model(weights, mat)
    ppm = _ppm(mat, torch.tensor([0.5], device=DEV))
    ref = dynamics(tg(state), tg(act), model, DEV, ppm)
    a = tg(act).requires_grad_()
    got = dynamics_differentiable(tg(state), a, model, DEV, ppm)
    assert got["state_seqs"].requires_grad
    assert torch.equal(got["action_seqs"].detach(), ref["action_seqs"])
    assert float((got["state_seqs"].detach() - ref["state_seqs"]).abs().max()) <= 1e-4


def _lin(W, x, k):
    return x @ W[k + ".weight"].t() + W[k + ".bias"]


def _mlp(W, x, k):
    for i in (0, 2, 4):
        x = F.relu(_lin(W, x, f"{k}.model.{i}"))
    return x


def _step64(W, state, attrs, p_inst, delta, phys, edges, pstep=3):
    """One model step in float64 on the CPU with index gathers / index_add over per-sample edge lists (model.py:129-313)."""
    B, H, N, _ = state.shape
    n_p = p_inst.shape[1]
    sn = torch.cat([state[:, 1:] - state[:, :-1], state[:, -1:]], 1).transpose(1, 2).reshape(B, N, -1)
    ph = torch.cat([phys[:, None].expand(B, n_p, -1), phys.new_zeros(B, N - n_p, phys.shape[1])], 1)
    p_in = torch.cat([attrs, ph, delta], 2)
    grp = torch.cat([p_inst, p_inst.new_zeros(B, N - n_p, p_inst.shape[2])], 1)
    out = []
    for b in range(B):
        r, s = (torch.from_numpy(e.astype(np.int64)) for e in edges[b])
        rel = torch.cat([attrs[b][r], attrs[b][s], (grp[b][r] - grp[b][s]).abs().sum(1, keepdim=True), sn[b][r] - sn[b][s]], 1)
        enc_n, enc_e = _mlp(W, p_in[b], "particle_encoder"), _mlp(W, rel, "relation_encoder")
        h = enc_n
        for _ in range(pstep):
            eff = F.relu(_lin(W, torch.cat([enc_e, h[r], h[s]], 1), "relation_propagator.linear"))
            agg = torch.zeros_like(h).index_add(0, r, eff)
            h = F.relu(_lin(W, torch.cat([enc_n, agg], 1), "particle_propagator.linear") + h)
        m = _lin(W, F.relu(_lin(W, F.relu(_lin(W, h[:n_p], "non_rigid_predictor.linear_0")), "non_rigid_predictor.linear_1")),
                 "non_rigid_predictor.linear_2")
        out.append(state[b, -1, :n_p] + m.clamp(-100, 100))
    return torch.stack(out)


def _rollout64(W, task, state, action, phys, edge_log):
    """dynamics_differentiable restated in float64 on the CPU, rolled out on the recorded edge lists (one entry per model step); checks that
    the oracle's edge builder on this rollout's own states gives the same lists."""
    n_his, ratio = task["n_his"], task["sim_real_ratio"]
    bsz, n_look = action.shape[:2]
    n_obj, n_t = state.shape[0], task["eef_num"]
    N = n_obj + n_t
    decoded, repeat = decode_action(action, push_length=task["push_length"])
    attrs = torch.zeros((bsz, N, 2), dtype=torch.float64)
    attrs[:, :n_obj, 0] = 1
    attrs[:, n_obj:, 1] = 1
    p_inst = torch.zeros((bsz, n_obj, task["max_n"]), dtype=torch.float64)
    p_inst[:, :, 0] = 1
    mask, tmask = np.ones((bsz, N), bool), np.zeros((bsz, N), bool)
    tmask[:, n_obj:] = True
    raise_by = 0.01 * ratio if task["gripper_enable"] else 0.0
    offs = [float(p[1]) * ratio for p in task["pusher_points"]]
    k, seqs, obj = 0, [], state[None].expand(bsz, n_obj, 3)
    for li in range(n_look):
        if li > 0:
            obj = seqs[-1].detach()
        y = obj[:, :, 1].min(1).values + raise_by
        d, th = decoded[:, li], action[:, li, 2]
        if n_t == 1:
            eef = torch.stack([d[:, 0], y, d[:, 1]], -1)[:, None]
        else:
            eef = torch.stack([torch.stack([d[:, 0] + o * torch.sin(th) if i else d[:, 0], y, d[:, 1] - o * torch.cos(th) if i else d[:, 1]], -1)
                               for i, o in enumerate(offs)], 1)
        dlt = torch.stack([d[:, 2] - d[:, 0], torch.zeros_like(y), d[:, 3] - d[:, 1]], -1)[:, None].expand(bsz, n_t, 3)
        states = torch.cat([obj[:, None].expand(bsz, n_his, n_obj, 3), eef[:, None].expand(bsz, n_his, n_t, 3)], 2)
        delta = torch.cat([torch.zeros((bsz, n_obj, 3), dtype=torch.float64), dlt], 1)
        rec = torch.zeros((bsz, n_obj, 3), dtype=torch.float64)
        for ai in range(1, 1 + int(repeat[:, li].max())):
            n_rel, recv, send = ago.build_edges(states[:, -1].detach().float().numpy(), task["adj_thresh"], mask, tmask, task["topk"],
                                                task["connect_tools_all"], "batch")
            if edge_log is None:                            # (the restatement's own graphs: checked against the oracle rollout on the CPU)
                own = [(recv[b, :n_rel[b]], send[b, :n_rel[b]]) for b in range(bsz)]
                pred = _step64(W, states, attrs, p_inst, delta, phys, own)
            for b in range(bsz if edge_log is not None else 0):
                assert np.array_equal(recv[b, :n_rel[b]], edge_log[k][b][0]) and np.array_equal(send[b, :n_rel[b]], edge_log[k][b][1]), \
                    f"edge lists differ at model step {k}, sample {b}"
            if edge_log is not None:
                pred = _step64(W, states, attrs, p_inst, delta, phys, edge_log[k])
            k += 1
            rec = torch.where((repeat[:, li] == ai)[:, None, None], pred, rec)
            tool = states[:, -1, n_obj:] + delta[:, n_obj:]
            yc = pred[:, :, 1].min(1).values + raise_by
            tool = torch.stack([tool[..., 0], yc[:, None].expand(bsz, n_t), tool[..., 2]], -1)
            states = torch.cat([states[:, 1:], torch.cat([pred, tool], 1)[:, None]], 1)
        seqs.append(rec)
    assert edge_log is None or k == len(edge_log)
    return torch.stack(seqs, 1)


def _chamfer64(x, y):
    d = torch.cdist(y.expand(x.shape[0], -1, -1), x)
    return d.min(2).values.mean(1) + d.min(1).values.mean(1)


@pytest.mark.gpu
@pytest.mark.parametrize("mat,n,n_look,seed", [("rope", 60, 2, 11), ("granular", 60, 1, 12)])
def test_rollout_gradients_vs_float64_restatement(weights, exact_chains, monkeypatch, mat, n, n_look, seed):
    task = configs.task_config(mat)
    state, act = synth.make_mpc_inputs(mat, n, 4, n_look=n_look, seed=seed, len_lo=1, len_hi=2.9, spacing=0.1)
    target = (state[::2] + np.array([0.3, 0.0, 0.2], np.float32)).astype(np.float32)
    bbox = np.array([[state[:, 0].min() - 1, state[:, 0].max() + 1], [state[:, 2].min() - 1, state[:, 2].max() + 1]])
    pen = {"rope": losses.rope_penalty, "granular": losses.granular_penalty}[mat]
    pen = partial(pen, sim_real_ratio=task["sim_real_ratio"])
    model = _model(weights, mat)
    log, build = [], graph.build_edges

    def recording_build(*a, **kw):
        csr = build(*a, **kw)
        log.append(csr.to_lists())
        return csr
    monkeypatch.setattr(graph, "build_edges", recording_build)

    # GPU: reward (chamfer + penalty + box) w.r.t. the actions; mean chamfer w.r.t. the physics parameter
    a = tg(act).requires_grad_()
    phys = torch.tensor([0.5], device=DEV, requires_grad=True)
    out = dynamics_differentiable(tg(state), a, model, DEV, _ppm(mat, phys))
    reward = mpc.running_cost(out["state_seqs"], a, tg(state), partial(losses.chamfer, y=tg(target)[None]), pen, bbox)["reward_seqs"]
    ga, = torch.autograd.grad(reward.sum(), a, retain_graph=True)
    gp, = torch.autograd.grad(losses.chamfer(out["state_seqs"][:, -1], tg(target)[None]).mean(), phys)
    monkeypatch.setattr(graph, "build_edges", build)

    # float64 CPU restatement on the same edge lists
    W = {k: torch.from_numpy(v).double() for k, v in weights.items()}
    A = torch.from_numpy(act).double().requires_grad_()
    P = torch.tensor([0.5], dtype=torch.float64, requires_grad=True)
    S, T = torch.from_numpy(state).double(), torch.from_numpy(target).double()

    def reward64(A_, P_=P):
        seq = _rollout64(W, task, S, A_, P_[None].expand(A_.shape[0], 1), log)
        return seq, mpc.running_cost(seq, A_, S, partial(_chamfer64, y=T[None]), pen, bbox)["reward_seqs"]
    seq64, r64 = reward64(A)
    assert float((out["state_seqs"].detach().cpu().double() - seq64.detach()).abs().max()) <= 1e-4
    ga64, = torch.autograd.grad(r64.sum(), A, retain_graph=True)
    gp64, = torch.autograd.grad(_chamfer64(seq64[:, -1], T[None]).mean(), P)
    ga_, gp_ = ga.cpu().double(), gp.cpu().double()
    assert float((ga_ - ga64).abs().max()) <= 1e-3 * float(ga64.abs().max()), (ga_, ga64)
    assert float((gp_ - gp64).abs().max()) <= 1e-3 * max(float(gp64.abs().max()), 1e-6), (gp_, gp64)
    # which coordinates carry gradient: x, z and theta of the last push do (earlier pushes reach the cost only through the penalty and
    # box terms: the object state is detached between pushes, forward_dynamics.py:38), the push length (a step count) never does
    assert float(ga[..., 3].abs().max()) == 0.0
    for c in range(3):
        assert float(ga[:, -1, c].abs().max()) > 0.0
    # sanity anchor: central differences of the restatement (same edges) on three action coordinates
    for (b, l, c) in ((0, 0, 0), (1, 0, 1), (2, n_look - 1, 2)):
        h = 1e-6
        Ap, Am = A.detach().clone(), A.detach().clone()
        Ap[b, l, c] += h
        Am[b, l, c] -= h
        with torch.no_grad():
            fd = float((reward64(Ap)[1].sum() - reward64(Am)[1].sum()) / (2 * h))
        assert abs(fd - float(ga64[b, l, c])) <= 1e-4 * max(1.0, abs(fd)), (b, l, c, fd, float(ga64[b, l, c]))


# ------------------------------------------------------------------ gradient planner
@pytest.mark.gpu
def test_gradient_planner_raises_reward_on_rope(weights):
    mat = "rope"
    task = configs.task_config(mat)
    state, _ = synth.make_mpc_inputs(mat, 60, 1, seed=21, spacing=0.1)
    target = (state[::2] + np.array([0.4, 0.0, 0.3], np.float32)).astype(np.float32)
    bbox = np.array([[state[:, 0].min() - 2, state[:, 0].max() + 2], [state[:, 2].min() - 2, state[:, 2].max() + 2]])
    model = _model(weights, mat)
    ppm = _ppm(mat, torch.tensor([0.5], device=DEV))
    lo, hi = tg(np.array(task["action_lower_lim"], np.float32)), tg(np.array(task["action_upper_lim"], np.float32))
    c0 = state.mean(0)
    act0 = tg(np.array([[c0[0], c0[2] - 0.3, 1.57, 3.5]], np.float32))
    cfg = dict(action_dim=4, model_rollout_fn=partial(dynamics_differentiable, model=model, device=DEV, ppm_optimizer=ppm),
               evaluate_traj_fn=partial(mpc.running_cost, error_func=partial(losses.chamfer, y=tg(target)[None]),
                                        penalty_func=partial(losses.rope_penalty, sim_real_ratio=task["sim_real_ratio"]), bbox=bbox),
               n_sample=16, n_look_ahead=1, n_update_iter=5, reward_weight=500.0, action_lower_lim=lo, action_upper_lim=hi,
               planner_type="GD", device=DEV, noise_level=0.3, verbose=True, lr=0.02)
    torch.manual_seed(0)
    res = mpc.GradientPlanner(cfg).trajectory_optimization(tg(state), act0)
    assert set(res) == {"act_seq", "model_outputs", "eval_outputs", "best_model_output", "best_eval_output"}
    means = [float(e["reward_seqs"].detach().mean()) for e in res["eval_outputs"]]
    assert len(means) == 5 and means[-1] > means[0], means
    assert bool(((res["act_seq"] >= lo) & (res["act_seq"] <= hi)).all())
    assert res["act_seq"].shape == (1, 4) and torch.isfinite(res["best_eval_output"]["reward_seqs"]).all()
