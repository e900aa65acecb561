"""The closed planning loop of the reference (src/planning/plan.py:212-315): observe, plan, act, slide the action window, observe again, record,
draw (viz.planning_frame, the reference's visualize_img), score, optionally identify the physics parameter.  The environment is anything with `SimEnv`'s surface
(`get_state_cur(fps_radius, return_cloud=True)`, `step`, `step_gripper`, `task_config`), the planner anything with the
`trajectory_optimization(state_cur, act_seq)` of `mpc.Planner` / `mpc.ChunkedPlanner` and an `n_look_ahead` attribute."""
import os

import numpy as np
import torch


def run_closed_loop(env, planner, criteria, n_actions, n_look_ahead, action_lower_lim, action_upper_lim, fps_radius, save_dir=None,
                    ppm_optimizer=None, use_ppo=False, viz=False, target_state=None, target_box=None, video=False):
    """plan.py:212-315.  `criteria` maps a cloud (1, n, 3) in simulator units to a 0-d error tensor; action_lower_lim / action_upper_lim are
    (action_dim,) tensors on the planner's device; the random draws are the reference's (`torch.rand` for the first window, then one row per
    step).  With `save_dir` step i writes interaction_{i}.npz with the reference's keys (plan.py:286-295) -- act, act_all, state_pred,
    state_pred_all, pcd_real, state_real, state_init -- which PhysicsParamOnlineOptimizer.optimize reads back; `use_ppo` calls
    `ppm_optimizer.optimize(i, iterations=50)` after every step.  With `viz` (and `save_dir`) step i also writes rgb_vis_{i}_0.png after planning
    and rgb_vis_{i}_1.png after the second observation (plan.py:262-283): viz.planning_image over the environment's own render, with
    `target_state` (m, 3) in simulator units or `target_box` ((x_min, x_max), (z_min, z_max)) as the overlay.  Drawing needs SimEnv's `render`
    and cameras; it draws no random number and reads nothing the loop does not read, so the actions, the errors and the records are those of
    viz=False.  With `video` (which needs `viz` and `save_dir`) the same images also go into save_dir/rgb_vis.avi, rgb_vis_{i}_0 then rgb_vis_{i}_1 in
    step order at 1 fps (plan.py:328-339), Motion-JPEG (jpeg.VideoWriter) encoded where the images are -- on the environment's device, before
    they are copied for the PNGs -- and nothing else changes.  -> (res_act_seq (n_actions, action_dim), error_seq of n_actions + 1 floats:
    the error before the first action and after every action).
    The window of step i is min(n_actions - i, n_look_ahead) rows, so that act_all and state_pred_all have the length plan.py:284-285 asserts;
    the reference shortens its window one step later and trips those assertions at the last step whenever n_look_ahead > 1 (its shipped
    configurations use 1)."""
    device = action_upper_lim.device
    action_dim = action_upper_lim.shape[0]
    full_look_ahead = int(n_look_ahead)
    gripper = bool(env.task_config.get("gripper_enable", False))
    if use_ppo and (ppm_optimizer is None or save_dir is None):
        raise ValueError("run_closed_loop: use_ppo needs ppm_optimizer and save_dir (the optimizer reads the recorded interactions)")
    if video and not (viz and save_dir is not None):
        raise ValueError("run_closed_loop: video needs viz and save_dir (the video is made of the drawn images)")
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
    reel = []      # the video's writer, opened at the first image (which gives the size)

    def numpy_of(x):
        return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)

    def observe():
        state, cloud = env.get_state_cur(fps_radius, return_cloud=True)
        if not isinstance(state, torch.Tensor):
            state = torch.from_numpy(np.ascontiguousarray(state, np.float32))
        return state.to(device=device, dtype=torch.float32), numpy_of(cloud)

    def draw(i, tag, state_init, res, state_after=None):
        from . import jpeg, viz
        image = viz.planning_image(env, state_init, res["best_model_output"]["state_seqs"][0][0], numpy_of(res["act_seq"][0]),
                                   target_state=target_state, target_box=target_box, state_after=state_after)
        if video:
            if not reel:
                reel.append(jpeg.VideoWriter(os.path.join(save_dir, "rgb_vis.avi"), image.shape[0], image.shape[1], 1,
                                             device=image.device if isinstance(image, torch.Tensor) else None))
            reel[0].add(image[None])
        viz.write_png(os.path.join(save_dir, f"rgb_vis_{i}_{tag}.png"), image)

    def error_of(cloud):
        return float(criteria(torch.from_numpy(cloud)[None].to(device)).item())

    act_seq = torch.rand((full_look_ahead, action_dim), device=device) * (action_upper_lim - action_lower_lim) + action_lower_lim
    res_act_seq = torch.zeros((n_actions, action_dim), device=device)
    error_seq = []
    for i in range(n_actions):
        window = min(n_actions - i, full_look_ahead)              # sliding window: never past the last action
        act_seq = act_seq[:window]
        planner.n_look_ahead = window
        state_cur, obj_pcd = observe()
        if i == 0:
            error_seq.append(error_of(obj_pcd))
        res = planner.trajectory_optimization(state_cur, act_seq)
        res = {k: v.detach().clone() if isinstance(v, torch.Tensor) else v for k, v in res.items()}
        act = numpy_of(res["act_seq"][0])
        if viz and save_dir is not None:
            draw(i, 0, state_cur, res)
        (env.step_gripper if gripper else env.step)(act)
        res_act_seq[i] = res["act_seq"][0].detach().clone()
        act_seq = torch.cat([res["act_seq"][1:],
                             torch.rand((1, action_dim), device=device) * (action_upper_lim - action_lower_lim) + action_lower_lim], dim=0)
        state_real, pcd_real = observe()
        if save_dir is not None:
            pred = res["best_model_output"]["state_seqs"]
            assert res["act_seq"].shape[0] == window and pred[0].shape[0] == window          # plan.py:284-285
            np.savez(os.path.join(save_dir, f"interaction_{i}.npz"), act=act, act_all=numpy_of(res["act_seq"]), state_pred=numpy_of(pred[0, 0]),
                     state_pred_all=numpy_of(pred[0]), pcd_real=pcd_real, state_real=numpy_of(state_real), state_init=numpy_of(state_cur))
            if viz:
                draw(i, 1, state_cur, res, state_after=state_real)
        error_seq.append(error_of(pcd_real))
        if use_ppo:
            ppm_optimizer.optimize(i, iterations=50)
    if reel:
        reel[0].close()
    planner.n_look_ahead = full_look_ahead
    return res_act_seq, error_seq
