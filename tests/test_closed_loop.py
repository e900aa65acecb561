"""The closed planning loop (adaptigraph_amd/closed_loop.py, plan.py:212-315): its records and its window with a stub planner on the host
environment, and one run with the real planner on the device environment."""
import glob
import os
from functools import partial

import numpy as np
import pytest
import torch

from adaptigraph_amd import configs, losses, mpc
from adaptigraph_amd.closed_loop import run_closed_loop
from test_sim_env import make_env

DEV = "cuda:0"
KEYS = {"act", "act_all", "state_pred", "state_pred_all", "pcd_real", "state_real", "state_init"}


class StubPlanner:
    """Returns the window it is given, shifted by a fixed amount, and zeros for the model's prediction."""

    def __init__(self):
        self.n_look_ahead, self.calls = None, []

    def trajectory_optimization(self, state_cur, act_seq):
        assert act_seq.shape == (self.n_look_ahead, 4)
        self.calls.append((state_cur.clone(), act_seq.clone()))
        plan = torch.tensor([0.3, 0.5, np.pi / 2, 3.0]).repeat(self.n_look_ahead, 1) + 0.001 * act_seq
        return {"act_seq": plan, "best_model_output": {"state_seqs": torch.zeros(1, self.n_look_ahead, state_cur.shape[0], 3)}}


class SeededEnv:
    """An environment whose every observation starts from one np.random.seed: the same scene gives the same key points."""

    def __init__(self, env):
        self.env, self.task_config, self.step, self.step_gripper = env, env.task_config, env.step, env.step_gripper

    def get_state_cur(self, *args, **kwargs):
        np.random.seed(3)
        return self.env.get_state_cur(*args, **kwargs)


def test_closed_loop_records_what_the_reference_records(tmp_path):
    env, planner = make_env("rope", None), StubPlanner()
    lo, hi = torch.tensor([-1.0, -1.0, -3.14, 2.0]), torch.tensor([1.0, 1.0, 3.14, 4.0])
    criteria = lambda cloud: ((cloud - torch.tensor([0.0, 0.03, -0.5])) ** 2).sum(-1).mean()      # noqa: E731
    torch.manual_seed(0)
    np.random.seed(0)
    acts, errors = run_closed_loop(env, planner, criteria, 3, 2, lo, hi, 0.2, save_dir=str(tmp_path))
    files = sorted(glob.glob(os.path.join(str(tmp_path), "interaction_*.npz")))
    assert [os.path.basename(f) for f in files] == [f"interaction_{i}.npz" for i in range(3)]
    assert acts.shape == (3, 4) and len(errors) == 4 and all(isinstance(e, float) and np.isfinite(e) for e in errors)
    windows = [2, 2, 1]                                   # the window shrinks at the last step
    assert [c[1].shape[0] for c in planner.calls] == windows and planner.n_look_ahead == 2
    for i, f in enumerate(files):
        rec = np.load(f)
        assert set(rec.files) == KEYS
        n = rec["state_init"].shape[0]
        assert rec["act"].shape == (4,) and rec["act_all"].shape == (windows[i], 4) and np.array_equal(rec["act"], rec["act_all"][0])
        assert rec["state_pred"].shape == (n, 3) and rec["state_pred_all"].shape == (windows[i], n, 3)
        assert rec["state_init"].dtype == np.float32 and rec["state_real"].ndim == 2 and rec["state_real"].shape[1] == 3
        assert rec["pcd_real"].ndim == 2 and rec["pcd_real"].shape[1] == 3 and len(rec["pcd_real"]) >= len(rec["state_real"])
        assert np.array_equal(rec["state_init"], planner.calls[i][0].numpy()) and np.array_equal(rec["act"], acts[i].numpy())
    # the sliding window: row 1 of a plan is row 0 of the next window, the new last row a draw inside the limits
    for i in (0, 1):
        nxt = planner.calls[i + 1][1]
        assert torch.equal(nxt[0], torch.from_numpy(np.load(files[i])["act_all"][1]))
    assert bool(((planner.calls[1][1][1] >= lo) & (planner.calls[1][1][1] <= hi)).all())
    torch.manual_seed(0)
    first = torch.rand((2, 4)) * (hi - lo) + lo
    assert torch.equal(planner.calls[0][1], first)


@pytest.mark.gpu
def test_closed_loop_with_the_planner_on_the_device(tmp_path):
    from adaptigraph_amd.forward_dynamics import dynamics
    from adaptigraph_amd.model import DynamicsPredictor
    mat = "rope"
    task = configs.task_config(mat)
    torch.manual_seed(0)
    model = DynamicsPredictor(configs.model_config(), configs.material_config(mat), configs.dataset_config(mat), DEV).to(DEV).eval()
    ppm = configs.ppm_optimizer_stub(mat)
    ppm.physics_param = {mat: torch.tensor([0.5], device=DEV)}
    tg = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)      # noqa: E731
    lo, hi = tg([-1.0, 0.2, 1.3, 5.0]), tg([1.0, 0.3, 1.8, 8.0])          # pushes of 0.5 .. 0.8 across the rope from z > 0
    criteria = partial(losses.chamfer, y=tg([[0.1 * i - 1.0, 0.03, -0.5] for i in range(20)])[None])
    cfg = dict(action_dim=4, model_rollout_fn=partial(dynamics, model=model, device=DEV, ppm_optimizer=ppm),
               evaluate_traj_fn=partial(mpc.running_cost, error_func=criteria, penalty_func=partial(losses.rope_penalty, sim_real_ratio=task["sim_real_ratio"]),
                                        bbox=np.array([[-3.0, 3.0], [-3.0, 3.0]])),
               n_sample=32, n_look_ahead=2, n_update_iter=1, reward_weight=task["reward_weight"], action_lower_lim=lo, action_upper_lim=hi,
               planner_type="MPPI", device=DEV, noise_level=0.3)
    planner = mpc.Planner(cfg)
    env = SeededEnv(make_env(mat, DEV))
    acts, errors = run_closed_loop(env, planner, criteria, 2, 2, lo, hi, task["fps_radius"], save_dir=str(tmp_path))
    assert acts.shape == (2, 4) and acts.is_cuda and len(errors) == 3 and all(np.isfinite(e) for e in errors)
    assert bool(((acts >= lo) & (acts <= hi)).all())
    rec = [np.load(os.path.join(str(tmp_path), f"interaction_{i}.npz")) for i in range(2)]
    assert all(set(r.files) == KEYS for r in rec)
    assert rec[0]["act_all"].shape == (2, 4) and rec[1]["act_all"].shape == (1, 4) and rec[1]["state_pred_all"].shape[0] == 1
    assert np.isfinite(rec[0]["state_pred_all"]).all() and rec[0]["state_pred"].shape == rec[0]["state_init"].shape
    assert np.array_equal(rec[1]["state_init"], rec[0]["state_real"])     # nothing moved between the two observations
    assert not np.array_equal(rec[0]["state_init"], rec[0]["state_real"])  # the push did move the rope
