"""`SimEnv`: a stand-in for the reference's `RealEnv` (src/planning/real_world/real_env.py:152-276) over the project's own simulators (sim/),
seen through simulated depth cameras (render.py).  It has RealEnv's observation and action surface -- `get_obs`, `get_intrinsics`,
`get_extrinsics`, `get_bbox`, `step`, `step_gripper` -- so the loop of plan.py:229-315 (closed_loop.run_closed_loop) runs against it, and
`get_state_cur`, which is perception.state_from_depth on the rendered images.

Frames.  The simulators work in simulator units with y up; the cameras, like the reference's calibration board, in metres with the table in
the plane z = 0 and z pointing DOWN.  A simulator point (x, y, z) is the board point (x s, z s, -(y s)) with s = float32(1 / sim_real_ratio)
-- float32 multiplications, which round the same on the host and on the device -- the inverse of perception.to_sim_frame.  A particle is
rendered as a sphere of the simulator's radius (`r`, or the pile's `rho`) times s.  The tool is not rendered: the robot retracts before every
observation (real_env.py:232, :240).

Actions are the planner's (x_start, z_start, theta, repeat) in simulator units, decoded by the reference's `decode_action_single`
(plan_utils.py:22-29); the reference divides them by sim_real_ratio only to talk to the robot, so nothing is divided here.  The 5 mm by which
`step_gripper` moves the start back along the drag (real_env.py:262-263) is 0.005 sim_real_ratio simulator units.

With `device=None` everything runs on the host statements (rope_push_host, render_depth_host, the host perception); with a device every step
is one launch of the material's Device*Push with x, v kept on the device, every observation one ag_render_depth launch, and no image leaves
the GPU on the way to `state_cur`.
"""
import dataclasses

import numpy as np

from . import perception, render, sim

# material: (default parameters, host push, device call)
SIMULATORS = {"rope": (sim.DEFAULT, sim.rope_push_host, sim.DevicePush),
              "granular": (sim.PILE_DEFAULT, sim.pile_push_host, sim.DevicePilePush),
              "cloth": (sim.CLOTH_DEFAULT, sim.cloth_push_host, sim.DeviceClothPush),
              "box": (sim.BOX_DEFAULT, sim.box_push_host, sim.DeviceBoxPush)}
MATERIALS = tuple(SIMULATORS)
DEFAULT_BBOX = ((-0.7, 0.7), (-0.7, 0.7), (-0.5, 0.05))      # board frame, metres: the work area and everything above the table (z is down)


def decode_action(action, push_length):
    """plan_utils.py:22-29 `decode_action_single`: (x_start, z_start, theta, repeat) -> x_start, z_start, x_end, z_end."""
    x_start, z_start, theta, repeat = action[0], action[1], action[2], int(action[3])
    return x_start, z_start, x_start - push_length * repeat * np.cos(theta), z_start - push_length * repeat * np.sin(theta)


def to_board_frame(points, sim_real_ratio):
    """Simulator (x, y, z) -> board (x s, z s, -(y s)), s = float32(1 / sim_real_ratio), in float32.  numpy array or torch tensor (..., 3)."""
    s = np.float32(1.0 / float(sim_real_ratio))
    q = points * s if isinstance(points, np.ndarray) else points * float(s)
    if isinstance(points, np.ndarray):
        return np.stack([q[..., 0], q[..., 2], -q[..., 1]], -1)
    import torch
    return torch.stack([q[..., 0], q[..., 2], -q[..., 1]], -1)


class SimEnv:
    """SimEnv(material, scene, task_config, cameras=None, device="cuda:0", params=None): `material` "rope" / "granular" / "cloth" / "box"; `scene` a
    RopeScene / PileScene / ClothScene / BoxScene with E = 1 (copied; `env.scene` is the current one, host arrays, or device tensors in x, v on the device
    path); `task_config` gives sim_real_ratio and push_length; `cameras` = (R_list, t_list, intr_list) in the board frame (default:
    render.default_cameras); `params` the simulator's parameters (default: the material's).  Keyword-only: `image_size` (H, W) of the cameras,
    `stride` of the perception, `bbox` (3, 2) the board-frame crop box, `near`, `far` the depth range in metres; `masks` where the keep-mask of
    an observation comes from: "ids" (the default) the renderer's id image, privileged knowledge; "color" the environment's own colour images
    through segment.keep_mask with `table_keys` (default: ColorKey.exact(viz.TABLE_COLOR)), what a user with real cameras would do."""

    def __init__(self, material, scene, task_config, cameras=None, device="cuda:0", params=None, *, image_size=(720, 1280), stride=4, bbox=None,
                 near=0.05, far=4.0, masks="ids", table_keys=None):
        if material not in MATERIALS:
            raise ValueError(f"SimEnv: material must be one of {MATERIALS}; got {material!r}")
        if masks not in ("ids", "color"):
            raise ValueError(f"SimEnv: masks must be \"ids\" or \"color\"; got {masks!r}")
        self.masks, self.table_keys = masks, table_keys
        if masks == "color" and table_keys is None:
            from . import segment, viz
            self.table_keys = [segment.ColorKey.exact(viz.TABLE_COLOR)]
        if scene.E != 1:
            raise ValueError("SimEnv: one episode per environment (E = 1)")
        self.material, self.task_config = material, task_config
        self.ratio = float(task_config["sim_real_ratio"])
        self.params = params if params is not None else SIMULATORS[material][0]
        self.H, self.W = int(image_size[0]), int(image_size[1])
        self.stride, self.near, self.far = int(stride), float(near), float(far)
        self.R_list, self.t_list, self.intr_list = cameras if cameras is not None else render.default_cameras(self.ratio, self.H, self.W)
        self.bbox = np.asarray(DEFAULT_BBOX if bbox is None else bbox, np.float64)
        self.plane = (0.0, 0.0, 1.0, 0.0)
        s = np.float32(1.0 / self.ratio)
        r_sim = np.asarray(scene.rho, np.float32) if material == "granular" else np.full(1, self.params.r, np.float32)
        self.radius = (r_sim * s).astype(np.float32)                 # (1,) metres
        self.n = np.asarray(scene.n, np.int32).reshape(1)
        self.device = None
        x, v = np.array(scene.x, np.float32), np.array(scene.v, np.float32)
        pose = np.array(scene.pose, np.float32) if material == "box" else None
        if device is not None:
            import torch
            self.device = torch.device(device)
            x, v = torch.from_numpy(x).to(self.device), torch.from_numpy(v).to(self.device)
            pose = torch.from_numpy(pose).to(self.device) if material == "box" else None
            self._renderer = render.DeviceRenderer(self.R_list, self.t_list, self.intr_list, self.H, self.W, self.plane, self.near, self.far, 1,
                                                   self.device)
            self._n_dev, self._radius_dev = torch.from_numpy(self.n).to(self.device), torch.from_numpy(self.radius).to(self.device)
        self.scene = dataclasses.replace(scene, x=x, pose=pose, vel=v) if material == "box" else dataclasses.replace(scene, x=x, v=v)

    # ---- RealEnv's observation surface
    def render(self):
        """-> depth (C, H, W) float32 metres, id (C, H, W) int32 (the particle, -1 the table, -2 nothing): numpy, or tensors on the device path
        (views of the renderer's buffers, which the next observation overwrites)."""
        pts = to_board_frame(self.scene.x, self.ratio)
        if self.device is None:
            depth, ids = render.render_depth_host(pts, self.n, self.radius, self.R_list, self.t_list, self.intr_list, self.H, self.W, self.plane,
                                                  self.near, self.far)
        else:
            depth, ids = self._renderer.launch(pts.contiguous(), self._n_dev, self._radius_dev)
        self.last_ids = ids[0]      # what the cameras saw last: the closed loop's pictures are drawn over it
        return depth[0], ids[0]

    def color(self, ids):
        """The colour images of id images `ids` (C, H, W) as `render` returns them -> (C, H, W, 4) uint8 RGBA: viz.draw with an empty display
        list over background mode 2, every particle viz.PALETTE[id % 4], the table and the void viz.TABLE_COLOR and viz.VOID_COLOR.  The
        device path is one ag_draw call into the environment's own canvas, which the next call overwrites."""
        from . import viz
        C = len(self.R_list)
        frames = np.array([[c, 0, 0, c] for c in range(C)], np.int32)
        if self.device is None:
            return viz.draw_host(np.zeros((0, 3), np.float32), np.zeros((0, 4), np.int32), np.zeros((0, 4), np.int32), frames,
                                 render.camera_rows(self.R_list, self.t_list, self.intr_list), self.H, self.W, 256, 2, ids, viz.PALETTE,
                                 viz.TABLE_COLOR, viz.VOID_COLOR, self.near)
        import torch
        if getattr(self, "_canvas", None) is None:
            self._canvas = viz.DeviceCanvas(render.camera_rows(self.R_list, self.t_list, self.intr_list), self.H, self.W, C, 1, self.near, self.device)
            self._frames = torch.from_numpy(frames).to(self.device)
            self._palette = torch.tensor(viz.PALETTE, dtype=torch.int32, device=self.device)
            self._no_pts = torch.zeros((0, 3), dtype=torch.float32, device=self.device)
            self._no_rows = torch.zeros((0, 4), dtype=torch.int32, device=self.device)
        return self._canvas.launch(self._no_pts, self._no_rows, self._no_rows, self._frames, 256, 2, ids.contiguous(), self._palette,
                                   viz.TABLE_COLOR, viz.VOID_COLOR)

    def get_obs(self, get_color=False, get_depth=True):
        """{"depth_i": (1, H, W) float32 in metres, "mask_i": (1, H, W) bool} per camera i (real_env.py:152-198 with one observation step) and,
        with `get_color`, "color_i": (1, H, W, 3) uint8, the sphere splat in `color`'s colours.  The mask stands for what the reference gets
        from its detection and segmentation models.  masks="ids": the pixel shows a particle, read off the renderer's id image.  masks="color":
        the environment looks at its own colour images -- rendered whatever `get_color` says, by the one ag_draw call of `color` -- and the mask
        is segment.keep_mask(color, table_keys): every pixel that is not table (perception.py:203-209).  The images are flat-coloured, so that
        is ids != render.ID_PLANE; it differs from the "ids" mask on the void pixels only, whose depth 0 depth_to_points drops under
        depth_threshold = (0, far), so `get_state_cur` is the same, bit for bit."""
        obs = {}
        by_color = self.masks == "color" and get_depth
        if get_depth or get_color:
            depth, ids = self.render()
        if get_color or by_color:
            rgba = self.color(ids)
        if get_color:
            for i in range(len(self.R_list)):
                obs[f"color_{i}"] = rgba[i][None, :, :, :3]
        if get_depth:
            keep = self._keep_mask(rgba) if by_color else ids >= 0
            for i in range(len(self.R_list)):
                obs[f"depth_{i}"] = depth[i][None]
                obs[f"mask_{i}"] = keep[i][None]
        return obs

    def _keep_mask(self, rgba):
        """segment.keep_mask of the colour images (C, H, W, 4) -> (C, H, W) bool, on the environment's path; a tensor of its own on the device
        (a copy out of the segmenter's buffer), so an observation keeps its masks as it does with masks="ids"."""
        from . import segment
        if self.device is None:
            return segment.keep_mask_host(rgba, self.table_keys)
        if getattr(self, "_segmenter", None) is None:
            self._segmenter = segment.DeviceSegmenter(len(self.R_list), self.H, self.W, self.device)
        return self._segmenter.keep_mask(rgba, self.table_keys).clone()

    def get_intrinsics(self):
        return [np.array(K, np.float64) for K in self.intr_list]

    def get_extrinsics(self):
        return [np.array(R, np.float64) for R in self.R_list], [np.array(t, np.float64) for t in self.t_list]

    def get_bbox(self):
        return self.bbox.copy()

    def get_state_cur(self, fps_radius, max_nobj=100, return_cloud=False):
        """perception.state_from_depth on the rendered images and masks -> state_cur (n_kp, 3) float32 in simulator units (a tensor on the
        device path); with `return_cloud` also the whole tabletop cloud in simulator units, the reference's obj_pcd."""
        obs = self.get_obs()
        C = len(self.R_list)
        state, cloud, _ = perception.state_from_depth(
            [obs[f"depth_{i}"][-1] for i in range(C)], *self.get_extrinsics(), self.get_intrinsics(), self.get_bbox(),
            keep_masks=[obs[f"mask_{i}"][-1] for i in range(C)], stride=self.stride, depth_threshold=(0, self.far), sim_real_ratio=self.ratio,
            fps_radius=fps_radius, max_nobj=max_nobj, device=self.device, return_details=True)
        return (state, cloud) if return_cloud else state

    # ---- RealEnv's action surface
    def _push(self, segment):
        """One push: the last two results of the material's push are its new state (x, v; the box's pose and velocity).  The box's x, what
        the cameras see, is the last frame of the push: frame frames_of(n_push) - 1, a number the host knows without reading anything back."""
        push = np.asarray(segment, np.float64).astype(np.float32).reshape(1, 4)
        _, host, device_call = SIMULATORS[self.material]
        if self.device is None:
            out = host(self.scene, push, self.params)
        else:
            out = device_call(self.scene, push, self.params, device=self.device).validate().launch()
        if self.material == "box":
            last = int(sim.frames_of(sim.push_steps(push, self.params)[0], self.params)[0]) - 1
            self.scene = dataclasses.replace(self.scene, x=out[0][:, last], pose=out[-2], vel=out[-1])
        else:
            self.scene = dataclasses.replace(self.scene, x=out[-2], v=out[-1])
        return push[0]

    def step(self, action, decoded=False):
        """real_env.py:212-240: one push from the action's start to its end.  -> the (xs, zs, xe, ze) float32 that was simulated."""
        return self._push(action if decoded else decode_action(action, self.task_config["push_length"]))

    def step_gripper(self, action, decoded=False):
        """real_env.py:242-276: one grasp-and-drag; the start moves back by 5 mm along the drag as lines 262-263 compute it."""
        if self.material == "box":
            raise ValueError("SimEnv: a box is pushed, not grasped (step_gripper is for the cloth)")
        x_start, z_start, x_end, z_end = action if decoded else decode_action(action, self.task_config["push_length"])
        back = 0.005 * self.ratio
        x_start = x_start - back * (x_end - x_start) / np.sqrt((x_end - x_start) ** 2 + (z_end - z_start) ** 2)
        z_start = z_start - back * (z_end - z_start) / np.sqrt((x_end - x_start) ** 2 + (z_end - z_start) ** 2)
        return self._push((x_start, z_start, x_end, z_end))

    def stop(self):
        pass
