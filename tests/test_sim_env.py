"""SimEnv (adaptigraph_amd/sim_env.py): RealEnv's observation and action surface over the three simulators.  On the host: what the cameras see
un-projects back onto the particles, and a step is the simulator's own push.  On the device: the host environment's images and key points, bit
for bit."""
import functools
import math

import numpy as np
import pytest
import torch

from adaptigraph_amd import configs, render, sim
from adaptigraph_amd.sim_env import SimEnv, decode_action, to_board_frame

DEV = "cuda:0"
H, W = 90, 160
PARAMS = {"rope": sim.SimParams(substeps=2, speed=0.04, record_every=4, settle=3),
          "granular": sim.PileParams(substeps=2, iters=2, speed=0.04, record_every=4, settle=3),
          "cloth": sim.ClothParams(substeps=2, iters=2, speed=0.1, lift=0.3, record_every=4, settle=3)}
ACTIONS = {"rope": np.array([0.3, 0.5, math.pi / 2, 8.0]),           # from z = 0.5 across the rope to z = -0.3
           "granular": np.array([-1.5, 0.1, math.pi, 5.0]),           # the board from x = -1.5 into the pile, to x = -0.5
           "cloth": np.array([1.05, 0.15, math.pi, 6.0])}             # the edge particle (1.05, 0.15) dragged outwards by 0.6


def make_scene(material):
    rng = np.random.default_rng(4)
    if material == "rope":
        i = np.arange(32)
        rope = np.stack([0.09 * (i - 15.5), np.full(32, sim.DEFAULT.r), 0.05 * np.sin(0.4 * i)], 1)
        return sim.RopeScene.from_ropes([rope.astype(np.float32)], stiffness=[0.5])
    if material == "granular":
        gx, gz = np.meshgrid((np.arange(8) - 3.5) * 0.25, (np.arange(8) - 3.5) * 0.25)
        xz = np.stack([gx.ravel(), gz.ravel()], 1) + rng.uniform(-0.01, 0.01, (64, 2))
        return sim.PileScene.from_piles([np.stack([xz[:, 0], np.full(64, 0.1), xz[:, 1]], 1).astype(np.float32)], [0.1])
    gx, gz = np.meshgrid((np.arange(8) - 3.5) * 0.3, (np.arange(8) - 3.5) * 0.3)
    cloth = np.stack([gx, np.full_like(gx, sim.CLOTH_DEFAULT.r), gz], 2).astype(np.float32)
    return sim.ClothScene.from_cloths([cloth], sf=[0.5])


def make_env(material, device):
    """Cameras half a metre above a 0.3 m scene, so that a 3 mm particle still covers pixels of a 90 x 160 image."""
    cams = render.look_at_cameras([(0.2, 0.2, -0.3), (0.2, -0.2, -0.3), (-0.2, -0.2, -0.3), (-0.2, 0.2, -0.3)], (0, 0, 0), H, W, 50.0, up=(0, 0, -1))
    return SimEnv(material, make_scene(material), configs.task_config(material), cams, device, PARAMS[material], image_size=(H, W), stride=1)


def act(env, material):
    return (env.step_gripper if material == "cloth" else env.step)(ACTIONS[material].copy())


def decoded(material):
    """plan_utils.py:22-29 and, for the gripper, real_env.py:262-263 with 5 mm = 0.05 simulator units, restated."""
    task = configs.task_config(material)
    xs, zs, th, rep = ACTIONS[material]
    xe, ze = xs - task["push_length"] * int(rep) * np.cos(th), zs - task["push_length"] * int(rep) * np.sin(th)
    if material == "cloth":
        xs = xs - 0.05 * (xe - xs) / np.sqrt((xe - xs) ** 2 + (ze - zs) ** 2)
        zs = zs - 0.05 * (ze - zs) / np.sqrt((xe - xs) ** 2 + (ze - zs) ** 2)
    return np.array([[xs, zs, xe, ze]], np.float32)


@functools.lru_cache(maxsize=None)
def host_run(material):
    """The host environment once per material: images and key points before and after one step."""
    env = make_env(material, None)
    out = {"scene0": env.scene}
    for when in ("before", "after"):
        if when == "after":
            out["push"] = act(env, material)
        depth, ids = env.render()
        np.random.seed(7)
        out[when] = (depth.copy(), ids.copy(), env.get_state_cur(configs.task_config(material)["fps_radius"]), env.scene)
    return out


# ------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("material", ["rope", "granular", "cloth"])
def test_host_env_sees_the_particles_and_steps_like_the_simulator(material):
    run = host_run(material)
    scene0, params = run["scene0"], PARAMS[material]
    push = decoded(material)
    assert np.array_equal(run["push"], push[0]) and np.array_equal(decode_action(ACTIONS[material], 0.1)[:2], ACTIONS[material][:2])
    host = {"rope": sim.rope_push_host, "granular": sim.pile_push_host, "cloth": sim.cloth_push_host}[material]
    x, v = host(scene0, push, params)[-2:]
    depth, ids, state, scene = run["after"]
    assert np.array_equal(scene.x, x) and np.array_equal(scene.v, v) and not np.array_equal(x, scene0.x)
    if material == "cloth":
        assert (sim.cloth_push_host(scene0, push, params)[3] >= 0).any()          # the gripper did grasp the cloth
    r = float(scene0.rho[0]) if material == "granular" else float(params.r)
    n = int(scene0.n[0])
    for when in ("before", "after"):
        depth, ids, state, scene = run[when]
        assert depth.shape == (4, H, W) and depth.dtype == np.float32 and len(np.unique(ids[ids >= 0])) > n // 2
        assert state.dtype == np.float32 and state.shape[1] == 3 and len(state) >= 3
        d = np.linalg.norm(state[:, None, :].astype(np.float64) - scene.x[0, None, :n].astype(np.float64), axis=2).min(1)
        print(f"{material} {when}: {len(state)} key points, farthest from a particle centre {d.max():.6f} (r = {r})")
        assert d.max() <= r + 1e-5


def test_obs_has_real_env_layout():
    env = make_env("rope", None)
    obs = env.get_obs(get_depth=True)
    assert sorted(obs) == sorted([f"depth_{i}" for i in range(4)] + [f"mask_{i}" for i in range(4)])
    depth, ids = env.render()
    for i in range(4):
        assert obs[f"depth_{i}"].shape == (1, H, W) and obs[f"depth_{i}"].dtype == np.float32 and obs[f"mask_{i}"].dtype == bool
        assert np.array_equal(obs[f"mask_{i}"][0], ids[i] >= 0) and np.array_equal(obs[f"depth_{i}"][0], depth[i])
        assert obs[f"mask_{i}"].any() and 0.2 < obs[f"depth_{i}"][obs[f"mask_{i}"]].min() < 0.6       # metres
    R_list, t_list = env.get_extrinsics()
    assert len(env.get_intrinsics()) == len(R_list) == len(t_list) == 4 and env.get_bbox().shape == (3, 2)
    x = env.scene.x[0, :5]
    board = to_board_frame(x, 10.0)
    assert board.dtype == np.float32 and np.array_equal(board, np.stack([x[:, 0] * np.float32(0.1), x[:, 2] * np.float32(0.1), -(x[:, 1] * np.float32(0.1))], 1))
    with pytest.raises(ValueError, match="E = 1"):
        SimEnv("rope", sim.RopeScene.from_ropes([x, x], stiffness=[0.5, 0.5]), configs.task_config("rope"), device=None)


# ------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("material", ["rope", "granular", "cloth"])
def test_device_env_is_the_host_env(material):
    run = host_run(material)
    env = make_env(material, DEV)
    for when in ("before", "after"):
        if when == "after":
            act(env, material)
        want_d, want_i, want_state, want_scene = run[when]
        depth, ids = env.render()
        assert depth.is_cuda and torch.equal(ids.cpu(), torch.from_numpy(want_i))
        assert torch.equal(depth.cpu().view(torch.int32), torch.from_numpy(want_d.view(np.int32)))
        obs = env.get_obs()
        assert obs["depth_3"].shape == (1, H, W) and obs["mask_3"].dtype == torch.bool and obs["mask_3"].is_cuda
        np.random.seed(7)
        state = env.get_state_cur(configs.task_config(material)["fps_radius"])
        assert state.is_cuda and torch.equal(state.cpu(), torch.from_numpy(want_state))
        assert env.scene.x.is_cuda and torch.equal(env.scene.x.cpu(), torch.from_numpy(want_scene.x))
