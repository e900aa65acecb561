#!/usr/bin/env python3
"""Generate tests/golden/planner_gd_toy.npz by RUNNING the reference Planner's 'GD' branch (CPU, this container only).

    python tools/gen_golden_gd.py

The reference Planner (src/planning/real_world/planner.py:279-310: sample, Adam on the samples, -mean(reward).backward(), clip, argmax)
runs on the analytic toy rollout and cost of the MPPI fixture (tools/gen_golden.py: toy_rollout / toy_cost, restated in
tests/test_grad_rollout_cpu.py) under a fixed torch seed.  The fixture holds inputs, the sampler's draw, the action sequences every
rollout saw (per iteration, then the best one), the final act_seq and its reward: data only.
"""
import contextlib
import io
import os
import sys
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import save, t, toy_cost, toy_rollout  # noqa: E402
from ref_import import import_reference  # noqa: E402


def main():
    torch.set_num_threads(1)
    R = import_reference()
    rng = np.random.default_rng(78)
    state_cur = t(rng.normal(0, 1, (12, 3)).astype(np.float32))
    target = state_cur + t(np.array([0.3, 0.0, -0.2], np.float32))
    lo, hi = t(np.array([-3.0, -3.0, -3.14, 1.0], np.float32)), t(np.array([3.0, 3.0, 3.14, 6.0], np.float32))
    act0 = t(np.array([[0.5, -0.5, 0.3, 3.0], [1.0, 0.2, -0.4, 2.0]], np.float32))
    n_sample, n_iter, lr, noise, seed = 16, 4, 0.05, 0.4, 123
    seen, draws, holder = [], [], []

    def rollout(state, acts):
        seen.append(acts.detach().clone().numpy())
        return toy_rollout(state, acts)

    def sampler(act_seq, iter_index=0):
        a = holder[-1].sample_action_sequences_default(act_seq)
        draws.append(a.detach().clone().numpy())
        return a

    cfg = dict(action_dim=4, model_rollout_fn=rollout, evaluate_traj_fn=partial(toy_cost, target=target), n_sample=n_sample, n_look_ahead=2,
               n_update_iter=n_iter, reward_weight=20.0, action_lower_lim=lo, action_upper_lim=hi, planner_type="GD", device="cpu",
               noise_level=noise, lr=lr, sampling_action_seq_fn=sampler)
    torch.manual_seed(seed)
    planner = R.Planner(cfg)
    holder.append(planner)
    with contextlib.redirect_stdout(io.StringIO()):
        res = planner.trajectory_optimization(state_cur, act0.clone())
    assert len(seen) == n_iter + 1 and len(draws) == 1
    save("planner_gd_toy", state_cur=state_cur.numpy(), target=target.numpy(), lim_lo=lo.numpy(), lim_hi=hi.numpy(), act0=act0.numpy(),
         n_sample=np.int64(n_sample), n_update_iter=np.int64(n_iter), lr=np.float64(lr), noise_level=np.float64(noise), seed=np.int64(seed),
         draw=draws[0], iter_act_seqs=np.stack(seen[:n_iter]), act_seq=res["act_seq"].detach().numpy(),
         best_reward=res["best_eval_output"]["reward_seqs"].detach().numpy())


if __name__ == "__main__":
    main()
