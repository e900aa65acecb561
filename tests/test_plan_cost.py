"""The planner's trajectory cost as one device call (`ag_plan_cost`, `mpc.running_cost_fused`): argument checks and the tensor-op fallback
on the CPU; on the GPU the per-cloud terms exactly against float32 numpy, the values against the float64 mirror next to the float32
tensor-op path, NaN propagation, the planner step and HIP-graph capture."""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

from conftest import golden_files, load_golden
from adaptigraph_amd import _lib, configs, losses, mpc, synth

CASES = [n for n in golden_files("mppi_") if n != "mppi_sampling"]
PEN_T = {"rope": losses.rope_penalty, "granular": losses.granular_penalty, "cloth": losses.cloth_penalty}
T_ERR, T_COL, T_BOX, T_NEAR, T_FAR, T_XLO, T_XHI, T_ZLO, T_ZHI = range(9)


def params(B=4, L=2, n=10, penalty=1, criterion=1, ratio=10.0):
    return _lib.PlanCostParams(B, L, n, penalty, criterion, ratio)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_plan_cost_rejects_bad_arguments_without_a_gpu():
    """Every check runs before any HIP call: a code and a message, no crash (the pointers are never dereferenced)."""
    L = _lib.lib()
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda prm, st=p, ac=p, si=p, er=p, rw=p, ws=p, nb=1 << 20: L.ag_plan_cost(ctypes.byref(prm) if prm is not None else None, st, ac, si, er,
                                                                                      rw, None, ws, nb, None)
    assert call(None) == -1 and b"null parameters" in L.ag_last_error()
    for kw in (dict(st=None), dict(ac=None), dict(si=None), dict(rw=None)):
        assert call(params(), **kw) == -1 and b"null argument" in L.ag_last_error(), kw
    for kw in (dict(B=0), dict(L=0), dict(n=0), dict(B=-3)):
        assert call(params(**kw)) == -1 and b"at least 1" in L.ag_last_error(), kw
    for pen in (-1, 4):
        assert call(params(penalty=pen)) == -1 and b"unknown penalty" in L.ag_last_error()
    for crit in (-1, 2):
        assert call(params(criterion=crit)) == -1 and b"unknown criterion" in L.ag_last_error()
    assert call(params(criterion=_lib.AG_ERROR_GIVEN), er=None) == -1 and b"needs error_in" in L.ag_last_error()
    need = L.ag_plan_cost_workspace_bytes(ctypes.byref(params()))
    assert call(params(), nb=need - 1) == -3 and b"workspace" in L.ag_last_error()
    assert call(params(), ws=None) == -3


def test_plan_cost_workspace_grows_with_clouds_not_particles():
    L = _lib.lib()
    size = lambda **kw: L.ag_plan_cost_workspace_bytes(ctypes.byref(params(**kw)))
    assert size(B=1, L=1, n=1) > 0
    assert size(B=1000, L=3, n=7) >= 1000 * 3 * _lib.AG_PLAN_TERMS * 4
    assert size(B=2000, L=3, n=7) > size(B=1000, L=3, n=7) and size(B=1000, L=6, n=7) > size(B=1000, L=3, n=7)
    assert size(B=1000, L=3, n=7) == size(B=1000, L=3, n=100000)
    assert size(B=0) == 0 and size(penalty=9) == 0 and L.ag_plan_cost_workspace_bytes(None) == 0


def _mean_dist(state, target):
    return (state - target[None]).norm(dim=-1).mean(dim=1)


@pytest.mark.parametrize("name", CASES)
def test_fused_cost_on_cpu_tensors_is_running_cost(name):
    g = load_golden(name)
    mat, ratio = str(g["material"]), float(g["sim_real_ratio"])
    st, ac, sc = (torch.from_numpy(g[k]) for k in ("state_seqs", "action", "state_cur"))
    box = torch.from_numpy(g["box"])
    pen = partial(PEN_T[mat], sim_real_ratio=ratio)
    want = mpc.running_cost(st, ac, sc, error_func=partial(losses.box_loss, target=box), penalty_func=pen, bbox=g["bbox"])["reward_seqs"]
    got = mpc.running_cost_fused(st, ac, sc, g["bbox"], mat, sim_real_ratio=ratio, box_target=box)["reward_seqs"]
    assert np.array_equal(got.numpy(), want.numpy()) and np.abs(got.numpy() - g["reward_box"]).max() <= 1e-6
    ef = partial(_mean_dist, target=sc + 0.25)
    want = mpc.running_cost(st, ac, sc, error_func=ef, penalty_func=pen, bbox=g["bbox"])["reward_seqs"]
    got = mpc.running_cost_fused(st, ac, sc, g["bbox"], mat, sim_real_ratio=ratio, error_func=ef)["reward_seqs"]
    assert np.array_equal(got.numpy(), want.numpy())
    with pytest.raises(ValueError):
        mpc.running_cost_fused(st, ac, sc, g["bbox"], mat, sim_real_ratio=ratio)
    with pytest.raises(ValueError):
        mpc.running_cost_fused(st, ac, sc, g["bbox"], mat, error_func=ef, box_target=box)
    with pytest.raises(ValueError):
        mpc.running_cost_fused(st, ac, sc, g["bbox"], "sand", box_target=box)


def test_fused_cost_keeps_the_tensor_op_gradient():
    g = load_golden("mppi_rope60")
    ratio = float(g["sim_real_ratio"])
    st, sc = torch.from_numpy(g["state_seqs"]), torch.from_numpy(g["state_cur"])
    k = int(sc[:, 0].argmax())                                 # pushes that start just beyond the contact distance of the rope's end: a gradient
    base = torch.from_numpy(g["action"]).clone()               # that is not all zeros
    step = 0.002 * torch.arange(base.shape[0] * base.shape[1], dtype=torch.float32).reshape(base.shape[0], base.shape[1])
    base[..., 0] = sc[k, 0] + 0.02 * ratio + 0.005 + step
    base[..., 1] = sc[k, 2]
    box = torch.from_numpy(g["box"])
    grads = []
    for fused in (False, True):
        ac = base.clone().requires_grad_()
        if fused:
            r = mpc.running_cost_fused(st, ac, sc, g["bbox"], "rope", sim_real_ratio=ratio, box_target=box)["reward_seqs"]
        else:
            r = mpc.running_cost(st, ac, sc, error_func=partial(losses.box_loss, target=box),
                                 penalty_func=partial(losses.rope_penalty, sim_real_ratio=ratio), bbox=g["bbox"])["reward_seqs"]
        (-r.mean()).backward()
        grads.append(ac.grad.clone())
    assert float(grads[0].abs().max()) > 0 and torch.equal(grads[0], grads[1])


# -------------------------------------------------------------------------------------------------- the value inputs
def cost_terms(state, action, state_cur, error_func, penalty_func, bbox):
    """mpc.running_cost line by line, keeping the terms: error, collision, box (bsz, L) and the reward (bsz,)."""
    bsz, L = state.shape[0], state.shape[1]
    error = error_func(state.reshape(bsz * L, state.shape[2], state.shape[3])).reshape(bsz, L)
    error_weight = 2.0 / (error.max() + 1e-6)
    collision = penalty_func(state, action, state_cur)
    lo, hi = state.min(dim=2).values, state.max(dim=2).values
    bbox = torch.as_tensor(bbox, dtype=state.dtype, device=state.device)
    margins = torch.stack([lo[..., 0] - bbox[0, 0], bbox[0, 1] - hi[..., 0], lo[..., 2] - bbox[1, 0], bbox[1, 1] - hi[..., 2]], dim=-1)
    box = torch.exp(-margins.clamp_min(0) * 100.0).max(dim=-1).values
    reward = -error_weight * error[:, -1] - 5.0 * collision.mean(dim=1) - 5.0 * box.mean(dim=1)
    return error, collision, box, reward


VALUE_BBOX = np.array([[-1.0, 5.0], [-1.0, 5.0]])
VALUE_BOX = np.array([[1.0, 2.5], [1.5, 3.0]], np.float32)


def make_value_inputs(penalty, B, L, n, seed):
    """Clouds uniform in a 4 x 4 square at sim_real_ratio 1; every push starts (granular: has one end of the pusher) `size + u` from a chosen
    particle of the cloud it is measured against, u uniform in [0, 0.04] and `size` the penalty's contact distance; against the workspace
    [-1, 5]^2 a third of the samples have a particle within 0.03 inside an edge, a third one outside, the rest are a unit away."""
    rng = np.random.default_rng(seed)
    state = np.empty((B, L, n, 3), np.float32)
    state[..., 0] = rng.uniform(0, 4, (B, L, n))
    state[..., 1] = rng.uniform(0, 0.1, (B, L, n))
    state[..., 2] = rng.uniform(0, 4, (B, L, n))
    init = state[0, 0].copy()
    init[:, [0, 2]] = rng.uniform(0, 4, (n, 2))
    if n > 1:
        for b in range(B):
            for l in range(L):
                kind, edge, j = b % 3, rng.integers(4), rng.integers(n)
                if kind == 2:
                    continue
                off = rng.uniform(0.0, 0.03) if kind == 0 else -rng.uniform(0.0, 0.03)
                state[b, l, j, 0 if edge < 2 else 2] = (-1.0 + off) if edge % 2 == 0 else (5.0 - off)
    size = 0.005 if penalty == "cloth" else 0.02
    action = np.zeros((B, L, 4), np.float32)
    action[..., 2] = rng.uniform(-3.14, 3.14, (B, L))
    action[..., 3] = rng.uniform(5, 15, (B, L))
    for b in range(B):
        for l in range(L):
            prev = init if (l == 0 or penalty == "cloth") else state[b, l - 1]
            j, phi, d = rng.integers(n), rng.uniform(0, 2 * np.pi), size + rng.uniform(0, 0.04)
            pt = prev[j, [0, 2]].astype(np.float64) + d * np.array([np.cos(phi), np.sin(phi)])
            if penalty == "granular":          # `pt` is the end off = +1 of the pusher
                th = float(action[b, l, 2])
                pt = pt - 0.05 * np.array([np.sin(th), -np.cos(th)])
            action[b, l, 0:2] = pt
    return state, action, init


def chamfer64(x, y):
    """losses.py:4-10 on CPU tensors of any dtype."""
    dis = torch.cdist(y.expand(x.shape[0], -1, -1), x)          # (B, M, N)
    return dis.min(dim=2).values.mean(dim=1) + dis.min(dim=1).values.mean(dim=1)


def value_target(n, seed=3):
    rng = np.random.default_rng(seed)
    t = np.zeros((1, min(n, 150), 3), np.float32)
    t[..., [0, 2]] = rng.uniform(1, 3, (1, t.shape[1], 2))
    return t


def reference64(penalty, criterion, state, action, init):
    st, ac, si = (torch.from_numpy(a).double() for a in (state, action, init))
    ef = partial(losses.box_loss, target=torch.from_numpy(VALUE_BOX).double()) if criterion == "box" else \
        partial(chamfer64, y=torch.from_numpy(value_target(state.shape[2])).double())
    return cost_terms(st, ac, si, ef, partial(PEN_T[penalty], sim_real_ratio=1.0), VALUE_BBOX)


VALUE_SHAPES = [(p, c, 256, 2, 200) for p in ("rope", "cloth", "granular") for c in ("box", "chamfer")] + [("rope", "chamfer", 64, 1, 1000)]


@pytest.mark.parametrize("penalty", ["rope", "cloth", "granular"])
def test_value_inputs_exercise_the_terms(penalty):
    """The construction's own condition, on the float64 reference alone and without a GPU: at least half of the collision terms and a
    quarter of the box terms lie strictly between 0.01 and 0.99."""
    _, col, box, _ = reference64(penalty, "box", *make_value_inputs(penalty, 256, 2, 200, seed=11))
    mid = lambda t: float(((t > 0.01) & (t < 0.99)).double().mean())
    assert mid(col) >= 0.5 and mid(box) >= 0.25, (mid(col), mid(box))


# ---------------------------------------------------------------------------------------------------------------- GPU
DEV = "cuda:0"
EXACT_SHAPES = [(1, 1, 1), (5, 1, 63), (3, 2, 64), (7, 3, 65), (2, 2, 4100), (1030, 1, 200)]


def tg(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def make_exact_inputs(B, L, n, where, seed, spread=4.0, reach=0.3):
    """Random clouds in which particle `where` (0 or n - 1) of EVERY cloud sets two of its extents (xlo and zhi for even b, xhi and zlo for odd b,
    at +-9: far from every other particle) and every push starts next to that particle of the cloud it is measured against."""
    rng = np.random.default_rng(seed)
    state = rng.uniform(0, spread, (B, L, n, 3)).astype(np.float32)
    init = rng.uniform(0, spread, (n, 3)).astype(np.float32)
    sign = np.where(np.arange(B) % 2 == 0, -1.0, 1.0).astype(np.float32)[:, None]
    state[:, :, where, 0] = 9 * sign + rng.uniform(0, 0.5, (B, L)).astype(np.float32)
    state[:, :, where, 2] = -9 * sign + rng.uniform(0, 0.5, (B, L)).astype(np.float32)
    init[where, 0], init[where, 2] = -9.25, 9.25
    action = rng.uniform(-1, 1, (B, L, 4)).astype(np.float32)
    action[..., 2] = 0.0                                        # theta = 0: sin = 0 and cos = 1 exactly
    prev = np.concatenate([np.broadcast_to(init[None, None], (B, 1, n, 3)), state[:, :-1]], 1)
    action[..., 0] = prev[:, :, where, 0] + rng.uniform(-reach, reach, (B, L)).astype(np.float32)
    action[..., 1] = prev[:, :, where, 2] + rng.uniform(-reach, reach, (B, L)).astype(np.float32)
    return state, action, init


def near_far32(cloud, px, pz):
    """float32, every product and sum rounded separately: sqrt(min(dx*dx + dz*dz)), sqrt(max(...)) and the arg-min over the particles."""
    dx, dz = (np.float32(px) - cloud[:, 0]).astype(np.float32), (np.float32(pz) - cloud[:, 2]).astype(np.float32)
    d2 = ((dx * dx).astype(np.float32) + (dz * dz).astype(np.float32)).astype(np.float32)
    return np.sqrt(d2.min(), dtype=np.float32), np.sqrt(d2.max(), dtype=np.float32), int(d2.argmin())


def fused_terms(penalty, state, action, init, ratio=1.0, bbox=VALUE_BBOX, **kw):
    if "error_func" not in kw:
        kw.setdefault("box_target", VALUE_BOX)
    out = mpc.running_cost_fused(tg(state), tg(action), tg(init), bbox, penalty, sim_real_ratio=ratio, return_terms=True, **kw)
    return out["terms"].cpu().numpy(), out["reward_seqs"].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("B,L,n", EXACT_SHAPES)
def test_terms_exact(B, L, n):
    for where in sorted({0, n - 1}):
        state, action, init = make_exact_inputs(B, L, n, where, seed=B + n + where)
        prev = np.concatenate([np.broadcast_to(init[None, None], (B, 1, n, 3)), state[:, :-1]], 1)
        st = tg(state)
        lo, hi = st.min(dim=2).values, st.max(dim=2).values
        samples = sorted(set(range(min(B, 4))) | {B - 1, B // 2})
        for penalty in ("rope", "cloth", "granular", None):
            out = mpc.running_cost_fused(st, tg(action), tg(init), VALUE_BBOX, penalty, sim_real_ratio=1.0, box_target=VALUE_BOX, return_terms=True)
            terms = out["terms"]
            for k, want in ((T_XLO, lo[..., 0]), (T_XHI, hi[..., 0]), (T_ZLO, lo[..., 2]), (T_ZHI, hi[..., 2])):
                assert torch.equal(terms[..., k], want), (penalty, where, k)
            if n > 1:      # the marked particle really is the one that sets them
                assert torch.equal(terms[0, :, T_XLO], st[0, :, where, 0]) and torch.equal(terms[0, :, T_ZHI], st[0, :, where, 2])
            again = mpc.running_cost_fused(st, tg(action), tg(init), VALUE_BBOX, penalty, sim_real_ratio=1.0, box_target=VALUE_BOX, return_terms=True)
            assert torch.equal(again["terms"], terms) and torch.equal(again["reward_seqs"], out["reward_seqs"])
            t = terms.cpu().numpy()
            if penalty is None:
                assert not t[..., [T_COL, T_NEAR, T_FAR]].any()
                continue
            for b in samples:
                for l in range(L):
                    cloud = init if penalty == "cloth" else prev[b, l]
                    x0, z0 = action[b, l, 0], action[b, l, 1]
                    if penalty == "granular":      # theta = 0: the nine points (x0 + off * 0, z0 + off * (-0.05))
                        pts = [(np.float32(x0 + np.float32(o) * np.float32(0.0)), np.float32(z0 + np.float32(o) * np.float32(-0.05)))
                               for o in np.arange(-1, 1.01, 0.25)]
                        near = min(near_far32(cloud, px, pz)[0] for px, pz in pts)
                        far = np.float32(0)
                    else:
                        near, far, arg = near_far32(cloud, x0, z0)
                        assert arg == where or (penalty == "cloth" and l > 0)      # (cloth measures every push against state_init)
                        far = far if penalty == "cloth" else np.float32(0)
                    assert t[b, l, T_NEAR] == near and t[b, l, T_FAR] == far, (penalty, where, b, l, t[b, l], near, far)


@pytest.mark.gpu
def test_cloth_normaliser_with_and_without_the_clamp():
    """f = min(farthest, 0.4 ratio) / max f: a small cloth whose farthest particle is beyond 0.4 for some grasp points (f = 1 exactly for them, less
    for the others) and for none (the largest f is a distance, not the cap)."""
    rng = np.random.default_rng(2)
    B, L, n = 37, 2, 81
    state = rng.uniform(0, 0.2, (B, L, n, 3)).astype(np.float32)
    init = rng.uniform(0, 0.2, (n, 3)).astype(np.float32)
    for reach, binds in ((0.5, True), (0.05, False)):
        action = rng.uniform(-reach, 0.2 + reach, (B, L, 4)).astype(np.float32)
        t, _ = fused_terms("cloth", state, action, init)
        far, near = t[..., T_FAR].astype(np.float64), t[..., T_NEAR].astype(np.float64)
        cap = float(np.float32(0.4))
        assert (far > cap).any() == binds and (far < cap).any()
        f = np.minimum(far, cap)
        assert f.max() == (cap if binds else far.max())
        want = 1.0 - np.exp(-np.maximum(near - float(np.float32(0.005)), 0) * 100.0) - 0.2 * f / f.max()
        assert np.abs(t[..., T_COL] - want).max() <= 1e-6
        if binds:
            hit = far > cap
            want_hit = (np.float32(1.0) - np.exp(-np.maximum(t[..., T_NEAR] - np.float32(0.005), np.float32(0)) * np.float32(100.0), dtype=np.float32))
            assert np.abs(t[..., T_COL][hit] - (want_hit[hit] - np.float32(0.2))).max() <= 5e-7      # (two roundings and exp's last bits, below 1)


@pytest.mark.gpu
def test_box_term_is_one_on_and_beyond_a_workspace_edge():
    state, action, init = make_exact_inputs(6, 2, 65, 0, seed=8)
    edge_x = float(state[0, 1, 0, 0])                          # sample 0's xlo particle of step 1 sits exactly on this edge
    t, _ = fused_terms("rope", state, action, init, bbox=np.array([[edge_x, 100.0], [-100.0, 100.0]]))
    assert t[0, 1, T_XLO] == np.float32(edge_x) and t[0, 1, T_BOX] == 1.0
    beyond = t[..., T_XLO] < np.float32(edge_x)
    assert beyond.any() and (t[..., T_BOX][beyond] == 1.0).all()
    inside = t[..., T_XLO] > np.float32(edge_x) + 1
    assert inside.any() and (t[..., T_BOX][inside] < 1e-30).all()


def worst(a, ref):
    return float((a.detach().double().cpu() - ref).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("penalty,criterion,B,L,n", VALUE_SHAPES)
def test_values_against_float64_next_to_the_tensor_op_path(penalty, criterion, B, L, n):
    """Both float32 evaluations against the float64 mirror on the same inputs: e_fused <= 2 e_parent + 1e-6 per term and for the reward."""
    state, action, init = make_value_inputs(penalty, B, L, n, seed=B + n)
    ref = reference64(penalty, criterion, state, action, init)
    mid = lambda t: float(((t > 0.01) & (t < 0.99)).double().mean())
    assert mid(ref[1]) >= 0.5 and mid(ref[2]) >= 0.25, (mid(ref[1]), mid(ref[2]))
    st, ac, si = tg(state), tg(action), tg(init)
    if criterion == "box":
        ef, kw = partial(losses.box_loss, target=tg(VALUE_BOX)), dict(box_target=VALUE_BOX)
    else:
        ef = partial(losses.chamfer, y=tg(value_target(n)))
        kw = dict(error_func=ef)
    parent = cost_terms(st, ac, si, ef, partial(PEN_T[penalty], sim_real_ratio=1.0), VALUE_BBOX)
    assert torch.equal(parent[3], mpc.running_cost(st, ac, si, ef, partial(PEN_T[penalty], sim_real_ratio=1.0), VALUE_BBOX)["reward_seqs"])
    out = mpc.running_cost_fused(st, ac, si, VALUE_BBOX, penalty, sim_real_ratio=1.0, return_terms=True, **kw)
    fused = (out["terms"][..., T_ERR], out["terms"][..., T_COL], out["terms"][..., T_BOX], out["reward_seqs"])
    for name, r, p, f in zip(("error", "collision", "box", "reward"), ref, parent, fused):
        e_parent, e_fused = worst(p, r), worst(f, r)
        print(f"plan_cost values {penalty} {criterion} {B}x{L}x{n} {name}: e_parent {e_parent:.3e} e_fused {e_fused:.3e}")
        assert e_fused <= 2 * e_parent + 1e-6, (name, e_fused, e_parent)


@pytest.mark.gpu
@pytest.mark.parametrize("criterion", ["box", "given"])
def test_nan_goes_where_the_tensor_ops_carry_it(criterion):
    for penalty in ("rope", "cloth", "granular"):
        state, action, init = make_value_inputs(penalty, 12, 2, 70, seed=5)
        state[4, 0, 69, 2] = np.nan
        st, ac, si = tg(state), tg(action), tg(init)
        if criterion == "box":
            ef, kw = partial(losses.box_loss, target=tg(VALUE_BOX)), dict(box_target=VALUE_BOX)
        else:
            given = torch.linspace(0.5, 1.5, 24, device=DEV)
            ef = lambda s: given
            kw = dict(error_func=ef)
        want = mpc.running_cost(st, ac, si, ef, partial(PEN_T[penalty], sim_real_ratio=1.0), VALUE_BBOX)["reward_seqs"]
        got = mpc.running_cost_fused(st, ac, si, VALUE_BBOX, penalty, sim_real_ratio=1.0, **kw)["reward_seqs"]
        assert torch.equal(torch.isnan(got), torch.isnan(want)), (penalty, got, want)
        assert bool(torch.isnan(want).all()) == (criterion == "box") and bool(torch.isnan(want[4]))
        ok = ~torch.isnan(want)
        assert float((got[ok] - want[ok]).abs().max() if ok.any() else 0.0) <= 1e-4


@pytest.mark.gpu
def test_mppi_step_scored_by_the_fused_cost(weights):
    """The set-up of test_mppi.test_mppi_step_vs_oracle_chain, scored the old way and with penalty="rope" on the same samples."""
    from adaptigraph_amd.model import DynamicsPredictor
    mat = "rope"
    task = configs.task_config(mat)
    state, act = synth.make_mpc_inputs(mat, 120, 24, seed=17, len_lo=2, len_hi=4.9, spacing=0.1)
    target = (state[::3] + np.array([0.3, 0.0, 0.2], np.float32)).astype(np.float32)
    bbox = np.array([[state[:, 0].min() - 1, state[:, 0].max() + 1], [state[:, 2].min() - 1, state[:, 2].max() + 1]])
    lo, hi = np.array(task["action_lower_lim"], np.float32), np.array(task["action_upper_lim"], np.float32)
    model = DynamicsPredictor(configs.model_config(), configs.material_config(mat), configs.dataset_config(mat), DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    model = model.to(DEV).eval().set_option("precision", 0)
    ppm = configs.ppm_optimizer_stub(mat)
    ppm.physics_param = {mat: torch.tensor([0.5], device=DEV)}
    ef, pf = partial(losses.chamfer, y=tg(target)[None]), partial(losses.rope_penalty, sim_real_ratio=task["sim_real_ratio"])
    old = mpc.MPPIPlanner(model, DEV, ppm, ef, pf, bbox, lo, hi, n_sample=24, reward_weight=500.0, noise_level=1.0)
    new = mpc.MPPIPlanner(model, DEV, ppm, ef, pf, bbox, lo, hi, n_sample=24, reward_weight=500.0, noise_level=1.0, penalty="rope")
    assert new.evaluate_traj.func is mpc.running_cost_fused and old.evaluate_traj.func is mpc.running_cost
    seq_old, r_old, out_old = old.step(tg(state), tg(act))
    seq_old, r_old, states = seq_old.clone(), r_old.clone(), out_old["state_seqs"].clone()
    seq_new, r_new, out_new = new.step(tg(state), tg(act))
    assert torch.equal(out_new["state_seqs"], states)
    st64, ac64, si64 = states.double().cpu(), tg(act).double().cpu(), tg(state).double().cpu()
    r64 = mpc.running_cost(st64, ac64, si64, partial(chamfer64, y=torch.from_numpy(target)[None].double()),
                           partial(losses.rope_penalty, sim_real_ratio=float(task["sim_real_ratio"])), bbox)["reward_seqs"]
    e_parent, e_fused = worst(r_old, r64), worst(r_new, r64)
    print(f"plan_cost planner step reward: e_parent {e_parent:.3e} e_fused {e_fused:.3e}")
    assert e_fused <= 2 * e_parent + 1e-6
    assert float((seq_new - seq_old).abs().max()) <= 1e-5


@pytest.mark.gpu
def test_fused_cost_is_captured_in_a_graph_and_replays_on_new_inputs():
    sets = [tuple(tg(a) for a in make_value_inputs("granular", 33, 2, 130, seed=s)) for s in range(4)]
    given = [torch.rand(66, device=DEV) + 0.1 * s for s in range(4)]
    st, ac, si, er = (t.clone() for t in (*sets[0], given[0]))
    run = lambda: mpc.running_cost_fused(st, ac, si, VALUE_BBOX, "granular", sim_real_ratio=1.0, error_func=lambda s: er, return_terms=True)
    run()                                                      # (the grow-only workspace exists before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for s in (1, 2, 3):
        for dst, src in zip((st, ac, si, er), (*sets[s], given[s])):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        got_r, got_t = out["reward_seqs"].clone(), out["terms"].clone()
        eager = run()
        assert torch.equal(got_r, eager["reward_seqs"]) and torch.equal(got_t, eager["terms"]), s
        assert bool(torch.isfinite(got_r).all())
