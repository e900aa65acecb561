"""Gradient planner (mpc.GradientPlanner, the reference Planner's 'GD' branch) on CPU: pinned to the reference's own run on an analytic
toy rollout (tests/golden/planner_gd_toy.npz, tools/gen_golden_gd.py) under the same torch seed."""
from functools import partial

import numpy as np
import pytest
import torch

from conftest import load_golden
from adaptigraph_amd import mpc


def _toy_rollout(state_cur, act_seqs):
    """The analytic model_rollout_fn the golden was generated with (tools/gen_golden.py:toy_rollout); differentiable in the actions."""
    n, L = act_seqs.shape[0], act_seqs.shape[1]
    disp = torch.stack([torch.sin(act_seqs[..., 0]) * act_seqs[..., 3], 0.1 * act_seqs[..., 2], torch.cos(act_seqs[..., 1])], -1)
    return {"state_seqs": state_cur[None, None] + 0.05 * torch.cumsum(disp, 1)[:, :, None, :] * torch.ones(n, L, state_cur.shape[0], 1)}


def _toy_cost(state_seqs, act_seqs, state_cur=None, weights=None, target=None):
    return {"reward_seqs": -((state_seqs[:, -1] - target[None]) ** 2).sum((1, 2)) - 0.01 * (act_seqs ** 2).sum((1, 2))}


def _config(g, rollout, sampler=None):
    tt = lambda k: torch.from_numpy(g[k].copy())      # noqa: E731
    cfg = dict(action_dim=4, model_rollout_fn=rollout, evaluate_traj_fn=partial(_toy_cost, target=tt("target")), n_sample=int(g["n_sample"]),
               n_look_ahead=2, n_update_iter=int(g["n_update_iter"]), reward_weight=20.0, action_lower_lim=tt("lim_lo"),
               action_upper_lim=tt("lim_hi"), planner_type="GD", device="cpu", noise_level=float(g["noise_level"]), lr=float(g["lr"]))
    if sampler is not None:
        cfg["sampling_action_seq_fn"] = sampler
    return cfg, tt


def test_gradient_planner_matches_reference_gd_branch():
    g = load_golden("planner_gd_toy")
    seen, draws, holder = [], [], []

    def rollout(state, acts):
        seen.append(acts.detach().clone().numpy())
        return _toy_rollout(state, acts)

    def sampler(act_seq, iter_index=0):
        a = holder[-1].sample_action_sequences_default(act_seq)
        draws.append(a.detach().clone().numpy())
        return a

    cfg, tt = _config(g, rollout, sampler)
    torch.manual_seed(int(g["seed"]))
    planner = mpc.GradientPlanner(cfg)
    holder.append(planner)
    res = planner.trajectory_optimization(tt("state_cur"), tt("act0"))
    assert set(res) == {"act_seq", "model_outputs", "eval_outputs", "best_model_output", "best_eval_output"}
    assert np.abs(draws[0] - g["draw"]).max() <= 1e-6
    n_iter = int(g["n_update_iter"])
    assert len(seen) == n_iter + 1
    for i in range(n_iter):
        assert np.abs(seen[i] - g["iter_act_seqs"][i]).max() <= 1e-6, f"iteration {i}"
    assert np.abs(res["act_seq"].detach().numpy() - g["act_seq"]).max() <= 1e-6
    assert np.abs(seen[-1][0] - g["act_seq"]).max() <= 1e-6
    assert np.abs(res["best_eval_output"]["reward_seqs"].detach().numpy() - g["best_reward"]).max() <= 1e-5
    lo, hi = tt("lim_lo"), tt("lim_hi")
    assert bool(((res["act_seq"] >= lo) & (res["act_seq"] <= hi)).all())


def test_gradient_planner_raises_on_nan_gradient():
    g = load_golden("planner_gd_toy")

    def rollout(state, acts):
        out = _toy_rollout(state, acts)["state_seqs"]
        return {"state_seqs": out * torch.sqrt(-torch.ones_like(acts[:, :1, :1, None].sum(-1, keepdim=True)))}      # sqrt(-1): NaN

    cfg, tt = _config(g, rollout)
    with pytest.raises(FloatingPointError):
        mpc.GradientPlanner(cfg).trajectory_optimization(tt("state_cur"), tt("act0"))


def test_planner_gd_type_still_refused():
    g = load_golden("planner_gd_toy")
    cfg, tt = _config(g, _toy_rollout)
    with pytest.raises(NotImplementedError):
        mpc.Planner(cfg).trajectory_optimization(tt("state_cur"), tt("act0"))
