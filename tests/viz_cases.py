"""Set-ups shared by tests/test_viz_cpu.py and tests/test_viz.py: a camera with a known projection, awkward display lists, and copies of the
smallest environments, planner stub and dataset fixture that the tests of those paths use (test_sim_env.py, test_sim_box.py,
test_closed_loop.py, test_scripted_rollout.py), copied so that this feature's tests do not depend on those files."""
import functools
import os
import pickle

import numpy as np
import torch

from adaptigraph_amd import configs, render, sim

DEV = "cuda:0"
H, W = 24, 40


def camera(H=H, W=W):
    """One camera a metre above the origin looking down the board's z: fx = fy, the principal point at the image centre."""
    return render.camera_rows(*render.look_at_cameras([(0.0, 0.0, -1.0)], (0, 0, 0), H, W, 60.0, up=(0, 1, 0)))


CAMS = camera()


def at_pixels(pixels, cams=CAMS, depth=1.0):
    """World points whose projection truncates to the given integer pixels (aimed at the pixel's half: half a pixel from every rounding)."""
    fx, fy, cx, cy = cams[0, 21:]
    R, t = cams[0, 9:18].reshape(3, 3), cams[0, 18:21]
    half = lambda z: z + 0.5 if z >= 0 else z - 0.5      # noqa: E731  (trunc goes toward zero)
    return np.array([R @ (np.array([(half(x) - cx) / fx, (half(y) - cy) / fy, 1.0]) * depth) + t for x, y in pixels], np.float32)


def awkward_list(rng, n_extra=40, H=H, W=W, cams=CAMS):
    """Primitives across every image edge, wholly outside, endpoints behind the camera, NaN points, out-of-range indices, sizes 0 and 64, bad
    kinds, sizes and layers -> pts, prims, styles.  Shared with the GPU tests."""
    px = [(-4, 5), (W + 3, 7), (5, -6), (9, H + 4), (-30, -30), (W + 50, H + 50), (0, 0), (W - 1, H - 1), (W // 2, H // 2), (3, H - 2)]
    px += [(int(rng.integers(-20, W + 20)), int(rng.integers(-20, H + 20))) for _ in range(n_extra)]
    pts = at_pixels(px, cams)
    special = np.array([[0.0, 0.0, -2.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -1.0], [1e6, 0.0, 0.0], [0.0, 0.0, -0.96]], np.float32)
    pts = np.concatenate([pts, special])      # behind the camera, NaN, inf, at the camera, far outside +-16 383, nearer than near
    n = len(pts)
    styles = [[0, 0, 0, 0x111111], [0, 64, 0, 0x222222], [1, 0, 0, 0x333333], [1, 64, 1, 0x444444], [1, 3, 0, 0x555555], [0, 4, 1, 0x666666],
              [2, 3, 0, 0x777777], [1, 65, 0, 0x888888], [0, -1, 0, 0x999999], [1, 2, 2, 0xAAAAAA], [1, 1, 1, 0xBBBBBB], [0, 7, 0, 0xCCCCCC]]
    prims = [[int(rng.integers(0, n)), int(rng.integers(0, n)), int(rng.integers(0, len(styles))), 0] for _ in range(6 * n)]
    prims += [[-1, 0, 4, 0], [0, n, 4, 0], [0, 1, len(styles), 0], [0, 1, -1, 0], [n, n, 0, 0], [2, n + 7, 11, 0]]      # a disc with a bad b is dropped too
    prims += [[i, j, 3, 0] for i, j in ((0, 1), (2, 3), (4, 5), (n - 1, 0), (0, n - 6), (n - 5, n - 5))]
    prims.sort(key=lambda p: p[2] not in (1, 3))      # the two styles of size 64 first (a stable sort): they cover a small image whole
    return pts, np.array(prims, np.int32), np.array(styles, np.int32)


# ------------------------------------------------------------------------------------------------------ environments, planner, dataset
def env_cameras():
    """Cameras half a metre above a 0.3 m scene, so that a particle of a few millimetres still covers pixels of a 90 x 160 image."""
    return render.look_at_cameras([(0.2, 0.2, -0.3), (0.2, -0.2, -0.3), (-0.2, -0.2, -0.3), (-0.2, 0.2, -0.3)], (0, 0, 0), 90, 160, 50.0, up=(0, 0, -1))


def rope_env(device):
    """test_sim_env.make_env("rope", device): a 32-particle rope."""
    from adaptigraph_amd.sim_env import SimEnv
    i = np.arange(32)
    rope = np.stack([0.09 * (i - 15.5), np.full(32, sim.DEFAULT.r), 0.05 * np.sin(0.4 * i)], 1)
    scene = sim.RopeScene.from_ropes([rope.astype(np.float32)], stiffness=[0.5])
    return SimEnv("rope", scene, configs.task_config("rope"), env_cameras(), device, sim.SimParams(substeps=2, speed=0.04, record_every=4, settle=3),
                  image_size=(90, 160), stride=1)


def box_env(device):
    """test_sim_box.make_env(device): a 16 x 16 box."""
    from adaptigraph_amd.sim_env import SimEnv
    scene = sim.BoxScene.from_boxes([(1.6, 1.6)], [(0.25, -0.15)], [0.2], grids=[(16, 16)])
    return SimEnv("box", scene, configs.task_config("box"), env_cameras(), device,
                  sim.BoxParams(substeps=2, iters=2, speed=0.05, record_every=4, settle=6), image_size=(90, 160), stride=1)


class StubPlanner:
    """test_closed_loop's: returns the window it is given, shifted by a fixed amount, and zeros for the model's prediction."""

    def __init__(self):
        self.n_look_ahead, self.calls = None, []

    def trajectory_optimization(self, state_cur, act_seq):
        assert act_seq.shape == (self.n_look_ahead, 4)
        self.calls.append((state_cur.clone(), act_seq.clone()))
        plan = torch.tensor([0.3, 0.5, np.pi / 2, 3.0]).repeat(self.n_look_ahead, 1) + 0.001 * act_seq
        return {"act_seq": plan, "best_model_output": {"state_seqs": torch.zeros(1, self.n_look_ahead, state_cur.shape[0], 3)}}


class SeededEnv:
    """test_closed_loop's: every observation starts from one np.random.seed; everything else is the environment's."""

    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        return getattr(self.env, name)

    def get_state_cur(self, *args, **kwargs):
        np.random.seed(3)
        return self.env.get_state_cur(*args, **kwargs)


@functools.lru_cache(maxsize=None)
def engine_model(material, precision):
    """test_scripted_rollout.engine_model: the golden seed-0 weights on the engine."""
    from conftest import load_golden
    from adaptigraph_amd.model import DynamicsPredictor
    w = load_golden("weights_seed0")
    m = DynamicsPredictor(configs.model_config(), configs.material_config(material), configs.dataset_config(material), DEV)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    m = m.to(DEV).eval()
    m.set_option("precision", precision)
    return m


def rollout_dataset_on_disk(root):
    """test_scripted_rollout's `dataset` fixture: the golden evaluation dataset in the reference's on-disk format under `root` -> g, config."""
    from conftest import load_golden
    g = load_golden("evalrollout_rope")
    name = str(g["data_name"])
    prep = os.path.join(root, "preprocess", name)
    os.makedirs(os.path.join(prep, "frame_pairs"))
    eef, obj = [], []
    for e in range(len(g["n_frames"])):
        os.makedirs(os.path.join(root, "sim_data", name, f"{e:06}"))
        with open(os.path.join(root, "sim_data", name, f"{e:06}", "property_params.pkl"), "wb") as f:
            pickle.dump({"particle_radius": 0.03, "stiffness": float(g["stiffness"][e])}, f)
        n = int(g["n_frames"][e])
        eef.append(g["eef_pos"][e, :n])
        obj.append(g["obj_pos"][e, :n])
        for k in range(int(g["n_push"][e])):
            np.savetxt(os.path.join(prep, "frame_pairs", f"{e:06}_{k + 1:02}.txt"), g[f"pairs_{e}_{k + 1}"], fmt="%d")
    with open(os.path.join(prep, "positions.pkl"), "wb") as f:
        pickle.dump({"eef_pos": eef, "obj_pos": obj}, f)
    ds = configs.dataset_config("rope")
    ds.update(data_dir=os.path.join(root, "sim_data"), prep_data_dir=os.path.join(root, "preprocess"), device=DEV,
              ratio={"train": [0, 0.34], "valid": [0.34, 1.0]},
              datasets=[dict(name="rope", max_nobj=int(g["max_nobj"]), max_nR=int(g["max_nR"]), fps_radius_range=[0.18, 0.22],
                             adj_radius_range=[0.48, 0.52], topk=10, connect_tool_all=False)])
    mat = configs.material_config("rope")
    mat["rope"]["physics_params"][1].update(min=0.0, max=1.0)
    return g, {"dataset_config": ds, "material_config": mat, "model_config": configs.model_config(),
               "train_config": {"random_seed": 42, "out_dir": os.path.join(root, "log")}, "rollout_config": {"out_dir": os.path.join(root, "rollout")}}
