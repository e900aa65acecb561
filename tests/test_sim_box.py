"""The box push kernel (csrc/ag_sim_box.hip through sim.box_push) against the host statement sim.box_push_host, bit for bit: every
particles-per-thread class and a partly filled last wave, several episodes in one launch, the branches of the pusher step (a miss, a corner, a
start inside the footprint), determinism, graph capture, argument errors, and the box through the dataset writer into train() with two physics
parameters, through SimEnv and through the closed planning loop."""
import math
import os
from functools import partial

import numpy as np
import pytest
import torch

from adaptigraph_amd import configs, datagen, sim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
NAMES = ("obj", "eef", "pose_frames", "n_frames", "pose", "vel")
# a push 0.65 long at 0.05 per step: 14 steps (frames after steps 0, 4, 8, 12), 2 substeps of 2 corrections, 6 settle steps
SMALL = sim.BoxParams(substeps=2, iters=2, speed=0.05, record_every=4, settle=6)
HIT = np.array([0.4, -1.0, 0.4, -0.35], F32)      # meets the long face of a 2.0 x 1.0 box at the origin, off its centre


def box(grid, com=(0.1, -0.05), angle=0.3, size=(2.0, 1.0), n_max=None):
    return sim.BoxScene.from_boxes([size], [com], [angle], grids=[grid], n_max=n_max)


def boxes(grids, coms, angles, n_max=None):
    return sim.BoxScene.from_boxes([(2.0, 1.0)] * len(grids), coms, angles, grids=grids, n_max=n_max)


def assert_same(scene, push, params=SMALL, f_max=None):
    host = sim.box_push_host(scene, push, params, f_max)
    got = sim.box_push(scene, push, params, f_max, device=DEV)
    for name, h, d in zip(NAMES, host, got):
        assert d.device.type == "cuda" and torch.equal(d.cpu(), torch.from_numpy(h)), name
    return host


@pytest.mark.parametrize("grid", [(2, 2), (3, 85), (16, 16), (2, 129), (3, 341), (32, 32)])
def test_one_episode_equals_the_host_at_every_size_class(grid):
    """n = 4: one lane of one wave; 255: the last lane of the workgroup idle; 256: one particle in every thread; 258: the second particle of
    two threads; 1023: the fourth particle of all but one; 1024: four particles in every thread.  A turned box, its centre of mass off centre,
    hit off centre: it translates and turns, and the push ends while it moves."""
    scene = box(grid)
    obj, eef, poses, n_frames, pose, vel = assert_same(scene, HIT[None])
    assert n_frames[0] == 5 and obj.shape == (1, 5, grid[0] * grid[1], 3) and np.isfinite(obj).all()
    assert np.abs(pose - scene.pose).max() > 0.1 and abs(vel[0, 2]) > 0 and abs(math.atan2(pose[0, 3], pose[0, 2]) - 0.3) > 0.01


def test_three_episodes_of_different_grids_share_one_launch():
    """2 x 2, 20 x 13 and 7 x 5 under n_max = 300; pushes of 14, 9 and 22 steps: 5, 4 and 7 frames under one F_max; the middle one misses.  Rows
    behind n and frames behind n_frames stay zero, also with more frames than any push writes."""
    scene = boxes([(2, 2), (20, 13), (7, 5)], [(0.0, 0.1), (0.3, -0.2), (-0.35, 0.3)], [0.0, 1.0, -2.0], n_max=300)
    push = np.stack([HIT, np.array([3.0, 3.0, 3.4, 3.0], F32), np.array([-0.6, 0.2, 0.4, -0.1], F32)])
    obj, eef, poses, n_frames, pose, vel = assert_same(scene, push)
    assert list(n_frames) == [5, 4, 7] and np.array_equal(pose[1], scene.pose[1]) and not vel[1].any() and vel[0].any() and vel[2].any()
    assert not obj[0, :, 4:].any() and not obj[2, :, 35:].any() and not obj[0, 5:].any() and not obj[1, 4:].any() and not poses[1, 4:].any()
    assert_same(scene, push, f_max=10)


def test_a_turned_box_at_rest_that_the_pusher_misses_stays_put():
    scene = box((9, 4), com=(0.2, 0.1), angle=2.2)
    obj, eef, poses, n_frames, pose, vel = assert_same(scene, np.array([[3.0, 3.0, 3.5, 3.2]], F32))
    assert all(np.array_equal(obj[0, f], scene.x[0]) for f in range(4)) and np.array_equal(pose, scene.pose) and not vel.any()


def test_a_pusher_that_starts_touching_a_corner():
    """An axis-aligned 2.0 x 1.0 box about the origin: the pusher starts 0.05 beyond the corner (1.0, 0.5) on both axes, 0.07 < R from it, so
    both clamps bind at once and the normal is diagonal; it moves on into the corner."""
    scene = box((8, 4), com=(0.0, 0.0), angle=0.0)
    obj, eef, poses, n_frames, pose, vel = assert_same(scene, np.array([[1.05, 0.55, 0.55, 0.35]], F32))
    assert pose[0, 0] < -0.01 and pose[0, 1] < -0.01 and abs(pose[0, 3]) > 1e-3      # pushed along both axes, and turned


def test_a_pusher_that_starts_inside_the_footprint():
    """The centre starts 0.2 inside the face x_hi and leaves through it: the box jumps back by about 0.2 + R in the first substep."""
    scene = box((8, 4), com=(0.1, 0.0), angle=0.0)
    obj, eef, poses, n_frames, pose, vel = assert_same(scene, np.array([[0.8, 0.1, 0.15, 0.1]], F32))
    assert poses[0, 0, 0] < scene.pose[0, 0] - 0.25 and np.isfinite(obj).all()
    deep = assert_same(scene, np.array([[0.0, 0.3, 0.65, 0.3]], F32))      # nearest the face z_hi
    assert deep[2][0, 0, 1] < scene.pose[0, 1] - 0.2


def test_the_shipped_constants_one_push():
    """8 substeps, 2 corrections, a frame every 10 steps, 30 settle steps on the default grid of a 2.4 x 1.2 box (30 x 15 = 450 particles): a push
    1.0 long."""
    scene = sim.BoxScene.from_boxes([(2.4, 1.2)], [(0.3, -0.25)], [0.5])
    obj, eef, poses, n_frames, pose, vel = assert_same(scene, np.array([[0.2, -1.3, 0.5, -0.35]], F32), sim.BOX_DEFAULT)
    assert scene.n[0] == 450 and n_frames[0] == 11 and not vel.any() and np.abs(pose - scene.pose).max() > 0.1


def test_two_calls_give_the_same_bits_and_a_graph_replays_them():
    scene = boxes([(33, 31), (5, 4)], [(0.3, 0.2), (-0.1, 0.1)], [0.4, 1.9])
    push = np.stack([HIT, HIT])
    first = [t.clone() for t in sim.box_push(scene, push, SMALL, device=DEV)]
    again = sim.box_push(scene, push, SMALL, device=DEV)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    call = sim.DeviceBoxPush(scene, push, SMALL, device=DEV)
    pose0, vel0 = call.pose.clone(), call.vel.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # warm-up outside the capture
        call.launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call.pose.copy_(pose0)
        call.vel.copy_(vel0)
        call.launch()
    outs = (call.obj, call.eef, call.pose_frames, call.n_frames, call.pose, call.vel)
    for _ in range(3):      # every replay restores the state and rewrites every frame
        for t in outs:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, outs))


@pytest.mark.parametrize("what", ["n_max = 1025", "n_max = 3", "F_max too small", "iters = 0", "substeps = 0", "record_every = 0", "eps too small"])
def test_argument_errors_leave_the_outputs_untouched(what):
    scene = box((3, 3), n_max=1025 if what == "n_max = 1025" else None)
    if what == "n_max = 3":
        scene.q, scene.m = scene.q[:, :3].copy(), scene.m[:, :3].copy()
    call = sim.DeviceBoxPush(scene, HIT[None], SMALL, f_max=4 if what == "F_max too small" else None, device=DEV)      # the push writes 5
    E, n_max, F, n_push_max, substeps, iters, record_every, settle = call.dims
    if what in ("iters = 0", "substeps = 0", "record_every = 0"):
        zero = what.split(" ")[0]
        call.dims = (E, n_max, F, n_push_max, 0 if zero == "substeps" else substeps, 0 if zero == "iters" else iters,
                     0 if zero == "record_every" else record_every, settle)
    if what == "eps too small":      # (mu g) / eps = 49 000 > 8192: the integer sums could leave their bound
        call.floats = call.floats[:5] + (1e-4,) + call.floats[6:]      # (h, g, mu, r, R, eps, ...)
    outs = (call.obj, call.eef, call.pose_frames, call.n_frames, call.pose, call.vel)
    for t in outs:
        t.fill_(7)
    with pytest.raises(RuntimeError, match=r"ag_sim_box_push failed \(-1\)"):
        call.launch()
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outs)


def test_a_null_pointer_is_an_argument_error():
    call = sim.DeviceBoxPush(box((3, 3)), HIT[None], SMALL, device=DEV)
    call.pose_frames = None
    with pytest.raises(RuntimeError, match=r"ag_sim_box_push failed \(-1\)"):
        call.launch()


@pytest.mark.parametrize("what", ["n = 3", "n = n_max + 1", "n_push = 0", "n_push > n_push_max", "inertia = 0", "rho_max = 9"])
def test_an_episode_outside_the_bounds_writes_no_frame_and_nothing_else(what):
    """The per-episode n, step count, inertia and rho_max are device arrays the library's host checks cannot see: an episode with one of them
    outside the bounds gets n_frames = 0 and its outputs and state stay as they were (filled with a sentinel before the call), while its
    neighbour in the same launch is simulated as if alone.  box_push refuses such a scene with box_push_host's error before any launch."""
    scene = boxes([(5, 4), (5, 4)], [(0.1, 0.1), (-0.2, 0.3)], [0.3, 0.8])
    push = np.stack([HIT, HIT])
    call = sim.DeviceBoxPush(scene, push, SMALL, device=DEV)
    if what.startswith("n_push"):
        steps = call.n_push.cpu()
        steps[0] = 0 if what == "n_push = 0" else steps[0] + 1
        call.n_push.copy_(steps)
    else:
        field, value, msg = {"n = 3": ("n", 3, "n outside 4 .. 20"), "n = n_max + 1": ("n", 21, "n outside 4 .. 20"),
                             "inertia = 0": ("inertia", 0.0, "inertia <= 0"), "rho_max = 9": ("rho_max", 9.0, "rho_max outside")}[what]
        getattr(scene, field)[0] = value
        for run in (lambda: sim.box_push_host(scene, push, SMALL), lambda: sim.box_push(scene, push, SMALL, device=DEV)):
            with pytest.raises(ValueError, match=msg):
                run()
        call = sim.DeviceBoxPush(scene, push, SMALL, device=DEV)
    outs = (call.obj, call.eef, call.pose_frames, call.n_frames, call.pose, call.vel)
    for t in outs:
        t[0].fill_(7)
    call.launch()
    torch.cuda.synchronize()
    assert call.n_frames.tolist() == [0, 5] and all(bool((t[0] == 7).all()) for t in (call.obj, call.eef, call.pose_frames, call.pose, call.vel))
    alone = sim.box_push_host(boxes([(5, 4)], [(-0.2, 0.3)], [0.8]), push[1:], SMALL)
    for name, h, d in zip(NAMES, alone, outs):
        assert torch.equal(d[1:].cpu(), torch.from_numpy(h)), name


def tree_bytes(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


# a push 3.0 long at 0.02 per step, a frame every 5 steps: the 0.1 of travel per frame that BOX_DIST_THRESH is made for
GEN = sim.BoxParams(substeps=2, speed=0.02, record_every=5, settle=10)


def test_dataset_on_the_device_equals_the_host_and_trains_with_two_parameters(tmp_path):
    """4 episodes x 2 pushes (one launch per round of pushes): device= writes the bytes device=None writes.  train() then runs 3 epochs of 4
    iterations on it, the batches assembled on the host and on the device: the model's particle encoder takes attr 2 + action 3 + physics 2 = 7
    inputs, every batch carries box_physics_param (B, 2), and the logged loss is finite and lower in the last epoch than in the first."""
    from adaptigraph_amd import train as agtrain
    from adaptigraph_amd.dataset import DeviceBatcher, DynDataset
    host = datagen.generate_box_dataset(str(tmp_path / "host"), 4, 2, seed=11, device=None, params=GEN, push_length=3.0)
    dev = datagen.generate_box_dataset(str(tmp_path / "dev"), 4, 2, seed=11, device=DEV, params=GEN, push_length=3.0)
    files = tree_bytes(tmp_path / "dev")
    assert len(files) == 4 * 4 + 8 + 3 and files == tree_bytes(tmp_path / "host") and host["n_his"] == dev["n_his"]
    task = configs.task_config("box")
    ds = dict(dev, device=DEV, ratio={"train": [0, 0.75], "valid": [0.75, 1.0]}, verbose=False,
              randomness={"use": True, "state_noise": {"train": 0.0, "valid": 0.0}, "phys_noise": {"train": 0.0, "valid": 0.0}},
              datasets=[dict(name="box", max_nobj=200, max_nR=4000, fps_radius_range=[task["fps_radius"] - 0.01, task["fps_radius"] + 0.01],
                             adj_radius_range=[task["adj_thresh"] - 0.02, task["adj_thresh"] + 0.02], topk=task["topk"], connect_tool_all=False)])
    mat = configs.material_config("box")
    data = DynDataset(ds, mat, "train")
    np.random.seed(0)
    item = data[0]
    assert item["box_physics_param"].shape == (2,) and torch.equal(item["box_physics_param"], torch.from_numpy(data.physics_params[int(data.pair_lists[0][0])]["box"]))
    np.random.seed(0)
    batch = DeviceBatcher(data, torch.device(DEV)).batch([0, 5, 9])
    assert batch["box_physics_param"].shape == (3, 2) and torch.equal(batch["box_physics_param"][0].cpu(), item["box_physics_param"])
    for device_batches in (False, True):
        cfg = {"dataset_config": ds, "material_config": mat, "model_config": configs.model_config(),
               "train_config": {"random_seed": 42, "out_dir": str(tmp_path / f"log{int(device_batches)}"), "phases": ["train", "valid"],
                                "num_workers": 0, "batch_size": 4, "n_epochs": 3, "log_interval": 1, "n_iters_per_epoch": {"train": 4, "valid": 1},
                                "device_batches": device_batches}}
        hist = agtrain.train(cfg)
        print(f"device_batches={device_batches}: train {hist['train']}, valid {hist['valid']}")
        assert len(hist["train"]) == 3 and np.isfinite(hist["train"]).all() and np.isfinite(hist["valid"]).all()
        assert hist["train"][-1] < hist["train"][0]
        weights = torch.load(os.path.join(cfg["train_config"]["out_dir"], "box", "checkpoints", "latest.pth"), map_location="cpu")
        first = next(v for k, v in weights.items() if k.startswith("particle_encoder") and v.ndim == 2)
        assert 7 in first.shape


def cameras():
    """Cameras half a metre above a 0.3 m scene, so that a 4 mm particle still covers pixels of a 90 x 160 image."""
    from adaptigraph_amd import render
    return render.look_at_cameras([(0.2, 0.2, -0.3), (0.2, -0.2, -0.3), (-0.2, -0.2, -0.3), (-0.2, 0.2, -0.3)], (0, 0, 0), 90, 160, 50.0, up=(0, 0, -1))


def make_env(device):
    from adaptigraph_amd.sim_env import SimEnv
    scene = sim.BoxScene.from_boxes([(1.6, 1.6)], [(0.25, -0.15)], [0.2], grids=[(16, 16)])
    return SimEnv("box", scene, configs.task_config("box"), cameras(), device, SMALL, image_size=(90, 160), stride=1), scene


def test_sim_env_on_the_device_equals_the_host_environment():
    action = np.array([0.5, -1.3, -math.pi / 2, 7.0])                        # from z = -1.3 along +z for 0.7, off the centre of mass
    fps_radius = configs.task_config("box")["fps_radius"]
    seen = {}
    for device in (None, DEV):
        env, scene0 = make_env(device)
        push = env.step(action.copy())
        np.random.seed(7)
        state = env.get_state_cur(fps_radius)
        depth, ids = env.render()
        to_np = (lambda t: t.cpu().numpy()) if device else np.asarray
        seen[device] = (push, to_np(env.scene.x), to_np(env.scene.pose), to_np(env.scene.vel), to_np(state), to_np(depth), to_np(ids))
        assert device is None or (env.scene.pose.is_cuda and env.scene.x.is_cuda and state.is_cuda)
    for name, h, d in zip(("push", "x", "pose", "vel", "state_cur", "depth", "ids"), seen[None], seen[DEV]):
        assert np.array_equal(h, d), name
    assert not np.array_equal(seen[None][1], scene0.x) and len(seen[None][4]) >= 10 and (seen[None][6] >= 0).any()


class SeededEnv:
    """An environment whose every observation starts from one np.random.seed: the same scene gives the same key points."""

    def __init__(self, env):
        self.env, self.task_config, self.step, self.step_gripper = env, env.task_config, env.step, env.step_gripper

    def get_state_cur(self, *args, **kwargs):
        np.random.seed(3)
        return self.env.get_state_cur(*args, **kwargs)


def test_closed_loop_of_two_actions_on_a_16_x_16_box(tmp_path):
    """run_closed_loop unchanged, with the planner on the device, a model of two physics parameters and the box environment on the device: two
    actions planned, simulated and recorded."""
    from adaptigraph_amd import losses, mpc
    from adaptigraph_amd.closed_loop import run_closed_loop
    from adaptigraph_amd.forward_dynamics import dynamics
    from adaptigraph_amd.model import DynamicsPredictor
    task = configs.task_config("box")
    torch.manual_seed(0)
    model = DynamicsPredictor(configs.model_config(), configs.material_config("box"), configs.dataset_config("box"), DEV).to(DEV).eval()
    assert model.material_dim == 2
    ppm = configs.ppm_optimizer_stub("box")
    ppm.physics_param = {"box": torch.tensor([0.75, 0.35], device=DEV)}
    tg = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)      # noqa: E731
    lo, hi = tg([-0.6, -1.3, -1.7, 6.0]), tg([0.6, -1.2, -1.4, 9.0])      # pushes of 0.6 .. 0.8 along +z, 0.2 or more beyond the face z_lo
    criteria = partial(losses.chamfer, y=tg([[0.1 * i - 0.8, 0.04, 1.0] for i in range(17)])[None])
    no_penalty = lambda state, action, state_cur: torch.zeros(state.shape[:2], dtype=state.dtype, device=state.device)      # noqa: E731
    cfg = dict(action_dim=4, model_rollout_fn=partial(dynamics, model=model, device=DEV, ppm_optimizer=ppm),
               evaluate_traj_fn=partial(mpc.running_cost, error_func=criteria, penalty_func=no_penalty, bbox=np.array([[-3.0, 3.0], [-3.0, 3.0]])),
               n_sample=32, n_look_ahead=2, n_update_iter=1, reward_weight=task["reward_weight"], action_lower_lim=lo, action_upper_lim=hi,
               planner_type="MPPI", device=DEV, noise_level=0.3)
    env = SeededEnv(make_env(DEV)[0])
    acts, errors = run_closed_loop(env, mpc.Planner(cfg), criteria, 2, 2, lo, hi, task["fps_radius"], save_dir=str(tmp_path))
    assert acts.shape == (2, 4) and acts.is_cuda and len(errors) == 3 and all(np.isfinite(e) for e in errors)
    assert bool(((acts >= lo) & (acts <= hi)).all())
    rec = [np.load(os.path.join(str(tmp_path), f"interaction_{i}.npz")) for i in range(2)]
    assert rec[0]["act_all"].shape == (2, 4) and rec[1]["act_all"].shape == (1, 4) and np.isfinite(rec[0]["state_pred_all"]).all()
    assert np.array_equal(rec[1]["state_init"], rec[0]["state_real"])     # nothing moved between the two observations
    assert not np.array_equal(rec[0]["state_init"], rec[0]["state_real"])  # the push did move the box
