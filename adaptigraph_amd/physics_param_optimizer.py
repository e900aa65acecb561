"""Online physics-parameter identification on the engine — SURVEY.md §8f row n2.

Mirrors src/planning/physics_param_optimizer.py: `dynamics_error` (:178-226) is the objective — roll every recorded
interaction forward with a candidate parameter (`dynamics_masked`) and average the masked chamfer distance to the observed
clouds — and `PhysicsParamOnlineOptimizer` keeps the interaction-file / `ppo_<i>.npz` contract (:33-72).

The reference minimises the objective with skopt's GP-BO (1 parameter) or CMA-ES (>1), ≈50 sequential evaluations of a
batch of a handful of graphs each.  Neither package exists here, and a sequential black-box search is the wrong shape for
this engine anyway: graphs in a batch are independent, so ALL candidates of a search generation are evaluated in ONE rollout
of `candidates x interactions` graphs (`dynamics_error_batch`).  `optimize` therefore does a dense batched sweep of
[-0.2, 1.2] followed by batched zoom refinements (1-D), or a batched cross-entropy search (>1-D): same objective, same
bounds, same outputs, different (derivative-free) search.

`optimize(..., method="gd")` searches by gradient instead: the objective is differentiable end to end (`dynamics_masked_differentiable`, the
masked chamfer's HIP backward), and one gradient step costs one forward and one backward however many parameters there are.
"""
import copy
import glob
import os

import numpy as np
import torch

from .forward_dynamics import dynamics_masked, dynamics_masked_differentiable
from .losses import mean_chamfer_device

PARAM_LO, PARAM_HI = -0.2, 1.2      # gp_minimize bounds / CMA bounds of the reference (:99, :151)


def _pad_interactions(ppm_optimizer, state_init_list, state_real_list, actions):
    """Ragged clouds -> (len_act, max_nobj, 3) tensors + masks, actions -> (len_act, 4)   (:190-216)."""
    device = ppm_optimizer.device
    max_nobj = ppm_optimizer.task_config["max_nobj"]
    n = len(actions)
    init = np.zeros((n, max_nobj, 3), np.float32)
    real = np.zeros((n, max_nobj, 3), np.float32)
    init_mask = np.zeros((n, max_nobj), bool)
    real_mask = np.zeros((n, max_nobj), bool)
    for i in range(n):
        a, b = np.asarray(state_init_list[i]), np.asarray(state_real_list[i])
        if a.shape[0] > max_nobj or b.shape[0] > max_nobj:      # np.pad with a negative width raises in the reference
            raise ValueError(f"interaction {i}: more than max_nobj={max_nobj} particles")
        init[i, :a.shape[0]], init_mask[i, :a.shape[0]] = a, True
        real[i, :b.shape[0]], real_mask[i, :b.shape[0]] = b, True
    to = lambda x: torch.from_numpy(x).to(device)
    act = torch.from_numpy(np.stack([np.asarray(a, np.float32) for a in actions], 0)).to(device)
    return to(init), to(init_mask), to(real), to(real_mask), act


@torch.no_grad()
def dynamics_error_batch(candidates, ppm_optimizer, state_init_list, state_real_list, actions):
    """candidates (C, d) -> (C,) mean error of each candidate, all C x len(actions) graphs in one rollout."""
    device = ppm_optimizer.device
    assert len(ppm_optimizer.material_dims) == 1, "only support single material now"
    material = next(iter(ppm_optimizer.material_dims))
    cand = torch.as_tensor(np.asarray(candidates, np.float32), device=device).reshape(len(candidates), -1)
    C, n = cand.shape[0], len(actions)
    init, init_mask, real, real_mask, act = _pad_interactions(ppm_optimizer, state_init_list, state_real_list, actions)
    rep = lambda x: x[None].expand((C,) + tuple(x.shape)).reshape((C * n,) + tuple(x.shape[1:]))
    out = dynamics_masked(rep(init), rep(init_mask), rep(act), ppm_optimizer.model, device, ppm_optimizer,
                          physics_param={material: cand[:, None, :].expand(C, n, -1).reshape(C * n, -1)})
    err = mean_chamfer_device(out["state_seqs"], rep(real), rep(init_mask), rep(real_mask))
    return err.reshape(C, n).double().mean(dim=1).cpu().numpy()


def dynamics_error(physics_param, ppm_optimizer, state_init_list, state_real_list, actions):
    """The reference objective (:178-226): float mean over interactions of the masked chamfer error for ONE parameter."""
    physics_param = copy.deepcopy(physics_param)
    device = ppm_optimizer.device
    if isinstance(physics_param, (list, np.ndarray)):
        assert len(ppm_optimizer.material_dims) == 1, "only support single material now"
        material = next(iter(ppm_optimizer.material_dims))
        physics_param = {material: torch.tensor(physics_param, dtype=torch.float32, device=device)}
    init, init_mask, real, real_mask, act = _pad_interactions(ppm_optimizer, state_init_list, state_real_list, actions)
    physics_param = {k: v.reshape(-1) for k, v in physics_param.items()}       # optimize_cma passes (1, d)
    out = dynamics_masked(init, init_mask, act, ppm_optimizer.model, device, ppm_optimizer, physics_param=physics_param)
    err = mean_chamfer_device(out["state_seqs"].detach(), real, init_mask, real_mask)
    return float(err.double().mean().item())


METHODS = ("sweep", "gd")
GD_LR = (0.1, 1e-4)         # Adam's step size at the first and the last iteration, geometric in between.  The objective is a mean of DISTANCES: V-shaped at
                            # its minimum, where a gradient keeps its length however close the parameter is, so only a shrinking step settles; and Adam
                            # moves a coordinate by about the step size whatever the gradient's length, so the steps must add up to the way from the
                            # first generation's best point to the minimum: 0.1 / (1 - 0.001^(1/29)) = 0.47 of the 1.4-wide box at 30 iterations
                            # (a first step of 0.03 adds up to 0.14 there: on the two-parameter task of bench_sysid.py every start stalled short)
GD_BETAS = (0.5, 0.9)       # short memories: across the V the gradient changes sign from one step to the next


def _first_generation(dims, iterations, init_param, seed):
    """The candidates of the sweep's first generation: the grid over the box (1-D), the seeded normal cloud around the current parameter (> 1-D)."""
    if dims == 1:
        return np.linspace(PARAM_LO, PARAM_HI, max(5, iterations // 3), dtype=np.float64)[:, None]
    rng = np.random.default_rng(seed)
    return np.clip(init_param.astype(np.float64) + 0.2 * rng.standard_normal((max(8, iterations // 5), dims)), PARAM_LO, PARAM_HI)


def _optimize_gd(ppm_optimizer, ev, dims, init_param, iterations, n_starts, seed, state_init_list, state_real_list, actions, checkpoint_steps):
    """Identification by gradient: the best `1 + n_starts` candidates of one batched sweep generation, improved TOGETHER by Adam — each iteration is
    one forward and one backward of `starts x interactions` graphs through dynamics_masked_differentiable and the differentiable masked chamfer,
    whatever the number of parameters — clamped to the box after every step; one host read per iteration (the points and their objective).
    The last point and the best-scoring point of every start are then scored by the sweep's own objective (dynamics_error_batch), so that the
    choice among them does not depend on the differentiable path's arithmetic.  -> (x_iters, func_vals, scored) of every evaluated point;
    scored: the point's value is the sweep's objective (not the differentiable path's)."""
    device = ppm_optimizer.device
    material = ppm_optimizer.material
    xs = _first_generation(dims, iterations, init_param, seed)
    fs = ev(xs)
    history_x, history_f = [xs], [fs]
    starts = xs[np.argsort(fs, kind="stable")[: 1 + max(0, int(n_starts))]]
    S, n = starts.shape[0], len(actions)
    init, init_mask, real, real_mask, act = _pad_interactions(ppm_optimizer, state_init_list, state_real_list, actions)
    rep = lambda x: x[None].expand((S,) + tuple(x.shape)).reshape((S * n,) + tuple(x.shape[1:]))
    init_r, imask_r, real_r, rmask_r, act_r = rep(init), rep(init_mask), rep(real), rep(real_mask), rep(act)
    P = torch.tensor(starts, dtype=torch.float32, device=device, requires_grad=True)
    opt = torch.optim.Adam([P], lr=GD_LR[0], betas=GD_BETAS)
    T = int(iterations)
    for t in range(T):
        opt.param_groups[0]["lr"] = GD_LR[0] * (GD_LR[1] / GD_LR[0]) ** (t / max(T - 1, 1))
        opt.zero_grad(set_to_none=True)
        out = dynamics_masked_differentiable(init_r, imask_r, act_r, ppm_optimizer.model, device, ppm_optimizer,
                                             physics_param={material: P[:, None, :].expand(S, n, dims).reshape(S * n, dims)},
                                             checkpoint_steps=checkpoint_steps)
        err = mean_chamfer_device(out["state_seqs"], real_r, imask_r, rmask_r).reshape(S, n).double().mean(dim=1)
        err.sum().backward()
        host = torch.cat([P.detach().double().reshape(-1), err.detach()]).cpu().numpy()      # the iteration's one host read
        history_x.append(host[: S * dims].reshape(S, dims)); history_f.append(host[S * dims:])
        opt.step()
        with torch.no_grad():
            P.clamp_(PARAM_LO, PARAM_HI)
    gx, gf = np.concatenate(history_x[1:]).reshape(T, S, dims), np.concatenate(history_f[1:]).reshape(T, S)
    best_seen = gx[np.nanargmin(np.where(np.isfinite(gf), gf, np.inf), axis=0), np.arange(S)]
    final = np.concatenate([P.detach().double().cpu().numpy(), best_seen])
    history_x.append(final); history_f.append(ev(final))
    scored = np.concatenate([np.ones(len(xs), bool), np.zeros(T * S, bool), np.ones(len(final), bool)])
    return np.concatenate(history_x), np.concatenate(history_f), scored


def optimize(ppm_optimizer, actions, state_init_list, state_pred_list, state_real_list, num_optim_trials=1, iter_idx=0,
             iterations=50, return_res=False, seed=42, method="sweep", n_starts=3, checkpoint_steps=False):
    """Same contract as the reference's `optimize` / `optimize_cma` (:75-175): -> (ppm, error, init_error[, res]).
    `iterations` bounds the number of objective evaluations PER INTERACTION SET exactly as n_calls does there; they are
    spent in batched generations.
    method: "sweep" — the derivative-free batched search; "gd" — gradient descent from the sweep's first generation (`_optimize_gd`), where
    `iterations` bounds the gradient steps and `n_starts` further starts run beside the generation's best (checkpoint_steps: see
    forward_dynamics.dynamics_masked_differentiable)."""
    if method not in METHODS:
        raise ValueError(f"optimize: method={method!r}, expected one of {METHODS}")
    if int(n_starts) < 0:
        raise ValueError(f"optimize: n_starts={n_starts} (>= 0)")
    dims = sum(ppm_optimizer.material_dims.values())
    material = ppm_optimizer.material
    init_param = ppm_optimizer.physics_param[material].detach().float().cpu().numpy().reshape(-1)
    ev = lambda c: dynamics_error_batch(c, ppm_optimizer, state_init_list, state_real_list, actions)
    init_error = float(ev(init_param[None])[0])
    if iterations == 0:
        return init_error
    if iterations < 0:
        iterations = 200
    history_x, history_f, scored = [], [], None
    if method == "gd":
        X, F, scored = _optimize_gd(ppm_optimizer, ev, dims, init_param, iterations, n_starts, seed, state_init_list, state_real_list, actions,
                            checkpoint_steps)
        history_x, history_f = [X], [F]
    elif dims == 1:
        per_gen = max(5, iterations // 3)
        lo, hi = PARAM_LO, PARAM_HI
        for _ in range(3):                                   # sweep, then zoom twice around the incumbent
            xs = np.linspace(lo, hi, per_gen, dtype=np.float64)[:, None]
            fs = ev(xs)
            history_x.append(xs); history_f.append(fs)
            k = int(np.argmin(fs))
            step = (hi - lo) / (per_gen - 1)
            lo, hi = max(PARAM_LO, xs[k, 0] - step), min(PARAM_HI, xs[k, 0] + step)
    else:
        rng = np.random.default_rng(seed)
        pop = max(8, iterations // 5)
        mean, std = init_param.astype(np.float64), np.full(dims, 0.2)          # CMA sigma0 of the reference (:147)
        for _ in range(5):
            xs = np.clip(mean + std * rng.standard_normal((pop, dims)), PARAM_LO, PARAM_HI)
            fs = ev(xs)
            history_x.append(xs); history_f.append(fs)
            elite = xs[np.argsort(fs)[: max(2, pop // 4)]]
            mean, std = elite.mean(0), elite.std(0) + 1e-3
    X, F = np.concatenate(history_x), np.concatenate(history_f)
    best = X[int(np.argmin(F if scored is None else np.where(scored, F, np.inf)))].astype(np.float32)
    error = dynamics_error(best.tolist(), ppm_optimizer, state_init_list, state_real_list, actions)
    res = {"x_iters": X, "func_vals": F, "x": best, "fun": error}
    return (best, error, init_error, res) if return_res else (best, error, init_error)


optimize_cma = optimize      # one batched search covers both of the reference's entry points


class PhysicsParamOnlineOptimizer:
    """Same attributes and file contract as the reference class (:18-72)."""

    def __init__(self, task_config, model, material, device, save_dir, method="sweep"):
        if method not in METHODS:
            raise ValueError(f"PhysicsParamOnlineOptimizer: method={method!r}, expected one of {METHODS}")
        self.method = method
        self.task_config = task_config
        self.model = model
        self.material = material
        self.device = device
        self.save_dir = save_dir
        self.physics_param = dict()
        self.material_indices = task_config["material_indices"]
        self.material_dims = task_config["material_dims"]
        self.fps_radius = task_config["fps_radius"]
        self.adj_thresh = task_config["adj_thresh"]
        self.eef_num = task_config["eef_num"]
        self.physics_param[self.material] = torch.tensor([0.5], device=device).repeat(self.material_dims[self.material])

    def optimize(self, i, iterations=50):
        files = sorted(glob.glob(os.path.join(self.save_dir, "interaction_*.npz")))
        assert len(files) == i + 1, f"interaction list {len(files)} != {i + 1}"
        act, state_init, state_pred, state_real = [], [], [], []
        for f in files:
            res = np.load(f)
            act.append(res["act"]); state_init.append(res["state_init"])
            state_pred.append(res["state_pred"]); state_real.append(res["state_real"])
        assert iterations > 0
        ppm, error, error_init, _ = optimize(self, act, state_init, state_pred, state_real, iter_idx=i, iterations=iterations,
                                             return_res=True, method=self.method)
        self.physics_param[self.material] = torch.tensor(ppm, dtype=torch.float32, device=self.device).clamp(-0.2, 1.2)
        np.savez(os.path.join(self.save_dir, f"ppo_{i}.npz"), physics_param=np.array(ppm), error=error, error_init=error_init)
        return ppm, error, error_init
