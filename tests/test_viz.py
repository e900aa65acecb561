"""ag_draw (csrc/ag_draw.hip) against the drawing statement (viz.draw_host), bit for bit, and the three places that draw: the evaluation
rollout, the closed loop and SimEnv's colour images."""
import os
from functools import partial

import numpy as np
import pytest
import torch

from adaptigraph_amd import configs, losses, mpc, render, viz
from viz_cases import SeededEnv, at_pixels, awkward_list, box_env, camera, engine_model, rollout_dataset_on_disk, rope_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def same(pts, prims, styles, frames, cams, H, W, *args, **kw):
    """The device image equals the host statement; -> the host image."""
    host = viz.draw_host(pts, prims, styles, frames, cams, H, W, *args, **kw)
    dev = viz.draw(pts, prims, styles, frames, cams, H, W, *args, device=DEV, **kw)
    assert dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == host.shape
    assert torch.equal(dev.cpu(), torch.from_numpy(host))
    return host


def random_list(rng, n_prim, H, W, cams, spread=12):
    """n_prim primitives of mixed kinds, sizes and layers between pixels in and around the image."""
    px = [(int(rng.integers(-spread, W + spread)), int(rng.integers(-spread, H + spread))) for _ in range(max(2 * n_prim, 2))]
    styles = np.array([[k, s, l, int(rng.integers(0, 1 << 24))] for k in (0, 1) for s in (0, 1, 2, 5, 9) for l in (0, 1)], np.int32)
    prims = np.stack([rng.integers(0, len(px), n_prim), rng.integers(0, len(px), n_prim), rng.integers(0, len(styles), n_prim),
                      np.zeros(n_prim, np.int64)], 1).astype(np.int32)
    return at_pixels(px, cams), prims, styles


@pytest.mark.parametrize("H,W", [(1, 1), (33, 65)])
@pytest.mark.parametrize("n_prim", [0, 1, 255, 256, 257, 600])
def test_image_sizes_and_chunk_edges(H, W, n_prim):
    cams = camera(H, W)
    pts, prims, styles = random_list(np.random.default_rng(n_prim), n_prim, H, W, cams)
    img = same(pts, prims, styles, [[0, 0, n_prim, 0]], cams, H, W, 128, color0=0x203040)
    if n_prim >= 255:      # something was drawn: the one pixel is not the background's; the larger image is a picture
        assert not (img[..., :3] == np.array([0x20, 0x30, 0x40], np.uint8)).all() and (H == 1 or len(np.unique(img.reshape(-1, 4), axis=0)) > 20)


def test_full_size_image_with_an_id_background():
    H, W = 720, 1280
    cams = camera(H, W)
    rng = np.random.default_rng(10)
    pts, prims, styles = random_list(rng, 600, H, W, cams, spread=40)
    ids = (np.add.outer(np.arange(H) // 37, np.arange(W) // 53) % 9 - 2).astype(np.int32)[None]
    img = same(pts, prims, styles, [[0, 0, 600, 0]], cams, H, W, 128, 2, ids, np.array(viz.PALETTE, np.int32), viz.TABLE_COLOR, viz.VOID_COLOR)
    assert len(np.unique(img.reshape(-1, 4), axis=0)) > 50


def test_a_full_list_in_one_tile_and_the_order_that_decides_pixels():
    H, W = 33, 65
    cams = camera(H, W)
    rng = np.random.default_rng(11)
    px = [(int(rng.integers(2, 30)), int(rng.integers(2, 30))) for _ in range(256)]      # every primitive inside tile (0, 0): a list of 256
    styles = np.array([[k, s, l, int(rng.integers(0, 1 << 24))] for k in (0, 1) for s in (3, 8, 20) for l in (0, 1)], np.int32)
    prims = np.stack([np.arange(256), rng.integers(0, 256, 256), rng.integers(0, len(styles), 256), np.zeros(256, np.int64)], 1).astype(np.int32)
    pts = at_pixels(px, cams)
    a = same(pts, prims, styles, [[0, 0, 256, 0]], cams, H, W, 90)
    b = same(pts, prims[::-1].copy(), styles, [[0, 0, 256, 0]], cams, H, W, 90)
    assert not np.array_equal(a, b)                                                       # the same primitives, the other order: other pixels
    # 300 primitives on one pixel box, both layers: two chunks feed one tile, the last of each layer wins
    prims = np.stack([np.full(300, 7), np.full(300, 7), np.arange(300) % len(styles), np.zeros(300, np.int64)], 1).astype(np.int32)
    img = same(pts, prims, styles, [[0, 0, 300, 0]], cams, H, W, 256)
    last_overlay = max(i for i in range(300) if styles[i % len(styles), 2] == 1)
    assert tuple(img[0, px[7][1], px[7][0], :3]) == tuple((int(styles[last_overlay % len(styles), 3]) >> s) & 255 for s in (16, 8, 0))


def test_every_dropped_primitive_rule_and_the_awkward_ones():
    H, W = 33, 65
    cams = camera(H, W)
    pts, prims, styles = awkward_list(np.random.default_rng(12), 60, H, W, cams)
    frames = [[0, 0, len(prims), 0], [0, -5, 40, 0], [0, len(prims) - 9, 100, 0], [0, 2 ** 31 - 5, 2 ** 31 - 1, 0], [0, 5, -3, 0], [7, 0, 9, 0], [-1, 0, 9, 0]]
    img = same(pts, prims, styles, frames, cams, H, W, 100, color0=0x010203)
    assert all((img[f] == np.array([1, 2, 3, 255], np.uint8)).all() for f in (3, 4, 5, 6)) and len(np.unique(img[0].reshape(-1, 4), axis=0)) > 6
    for alpha in (0, 256):
        same(pts, prims, styles, frames[:1], cams, H, W, alpha)


def test_three_frames_three_cameras_ragged_ranges_and_the_background_modes():
    H, W = 33, 65
    R, t, K = render.look_at_cameras([(0.0, 0.0, -1.0), (0.3, 0.1, -0.9), (-0.2, 0.3, -1.1)], (0, 0, 0), H, W, 60.0, up=(0, 1, 0))
    cams = render.camera_rows(R, t, K)
    rng = np.random.default_rng(13)
    pts, prims, styles = random_list(rng, 500, H, W, cams[:1])
    frames = [[2, 300, 200, 1], [0, 0, 0, 0], [1, 17, 283, 5]]
    same(pts, prims, styles, frames, cams, H, W, 128, color0=0x446688)
    bg = rng.integers(0, 256, (2, H, W, 4), dtype=np.uint8)
    img = same(pts, prims, styles, frames, cams, H, W, 128, 1, bg, color0=0x446688)
    assert np.array_equal(img[1, ..., :3], bg[0, ..., :3]) and not np.array_equal(img[0, ..., :3], bg[1, ..., :3])
    ids = rng.integers(-2, 12, (2, H, W)).astype(np.int32)
    same(pts, prims, styles, frames, cams, H, W, 128, 2, ids, np.array([0xFF0000, 0x00FF00, 0x0000FF], np.int32), 0x101010, 0x202020)


def test_canvas_launch_captures_into_a_graph():
    H, W = 33, 65
    cams = camera(H, W)
    rng = np.random.default_rng(14)
    lists = [random_list(np.random.default_rng(20 + i), 300, H, W, cams) for i in range(3)]
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt).contiguous()      # noqa: E731
    pts = up(lists[0][0], torch.float32)
    prims, styles = up(lists[0][1], torch.int32), up(lists[0][2], torch.int32)
    frames = up(np.array([[0, 0, 300, 0], [0, 100, 50, 0]], np.int32), torch.int32)
    canvas = viz.DeviceCanvas(cams, H, W, 2, len(lists[0][0]), device=DEV)
    canvas.launch(pts, prims, styles, frames, 128, color0=0x334455)                             # warm up: the first launch loads the code object
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = canvas.launch(pts, prims, styles, frames, 128, color0=0x334455)
    for i in (1, 2, 0):
        pts.copy_(up(lists[i][0], torch.float32))
        graph.replay()
        torch.cuda.synchronize()
        want = viz.draw_host(lists[i][0], lists[0][1], lists[0][2], frames.cpu().numpy(), cams, H, W, 128, color0=0x334455)
        assert torch.equal(out.cpu(), torch.from_numpy(want)), i
    assert rng is not None
    with pytest.raises(ValueError):
        canvas.launch(pts, prims, styles, frames.repeat(2, 1), 128)                             # more frames than the canvas holds
    with pytest.raises(ValueError):
        canvas.launch(pts.double(), prims, styles, frames, 128)


def test_draw_list_on_the_device_reads_csr_edges_without_a_host_read():
    from adaptigraph_amd.graph import build_edges
    rng = np.random.default_rng(15)
    B, N = 3, 9
    x = torch.from_numpy(rng.uniform(-0.2, 0.2, (B, N, 3)).astype(np.float32)).to(DEV)
    mask = torch.ones((B, N), dtype=torch.bool, device=DEV)
    tool = torch.zeros((B, N), dtype=torch.bool, device=DEV)
    tool[:, -1] = True
    csr = build_edges(x, 0.25, mask, tool, 4, False, "batch", max_tools=1)
    lists = csr.to_lists()
    for b in range(B):
        dev_list, host_list = viz.DrawList(DEV), viz.DrawList()
        for dl in (dev_list, host_list):
            first = dl.add_points(x[b])
            obj, tl = dl.style(viz.SEGMENT, 1, 0, viz.GREEN), dl.style(viz.SEGMENT, 1, 0, viz.RED)
            dl.begin_frame()
            if dl is dev_list:
                dl.add_edges(first, csr, None, obj, tl, N - 1, sample=b)
            else:
                dl.add_edges(first, lists[b][0], lists[b][1], obj, tl, N - 1)
        got, want = dev_list.tables()[1].cpu().numpy(), host_list.tables()[1]
        assert len(want) > 0 and np.array_equal(got[:len(want)], want) and (got[len(want):, :2] == -1).all() and len(got) == csr.e_cap // B
        cams = camera(33, 65)
        assert torch.equal(viz.draw(*dev_list.tables(), cams, 33, 65, device=DEV).cpu(), torch.from_numpy(viz.draw(*host_list.tables(), cams, 33, 65)))


# ------------------------------------------------------------------------------------------------------ the three places that draw
@pytest.mark.parametrize("material", ["rope", "box"])
def test_sim_env_colour_images_device_equals_host(material):
    make = box_env if material == "box" else rope_env
    host, dev = make(None).get_obs(get_color=True), make(DEV).get_obs(get_color=True)
    assert set(host) == set(dev) and sum(k.startswith("color_") for k in host) == 4
    for i in range(4):
        assert dev[f"color_{i}"].is_cuda and tuple(dev[f"color_{i}"].shape) == (1, 90, 160, 3)
        assert torch.equal(dev[f"color_{i}"].cpu(), torch.from_numpy(host[f"color_{i}"])) and len(np.unique(host[f"color_{i}"].reshape(-1, 3), axis=0)) >= 3
        assert torch.equal(dev[f"depth_{i}"].cpu(), torch.from_numpy(host[f"depth_{i}"]))


@pytest.mark.parametrize("scripted", [False, True])
def test_rollout_dataset_draws_every_step_and_returns_the_same_errors(tmp_path, monkeypatch, scripted):
    import adaptigraph_amd.eval_rollout as er
    from adaptigraph_amd.sim_env import to_board_frame
    root = str(tmp_path)
    g, cfg = rollout_dataset_on_disk(root)
    cfg["rollout_config"]["viz_size"] = (90, 160)
    model = engine_model("rope", 0)
    calls = []
    real = viz.write_rollout_record
    monkeypatch.setattr(viz, "write_rollout_record", lambda *a, **k: calls.append((a, k)) or real(*a, **k))
    curves = {}
    for flag in (False, True):
        out = os.path.join(root, f"viz{int(flag)}")
        os.makedirs(out)
        np.random.seed(int(g["seed"]))
        curves[flag] = er.rollout_dataset(model, DEV, cfg, out, viz=flag, scripted=scripted)
    assert np.array_equal(curves[False], curves[True]) and len(calls) == 1                       # drawing reads and never perturbs
    for e in (1, 2):
        for k in (1, 2):
            name = os.path.join(str(e), "short", f"error_{k}.txt")
            assert np.array_equal(np.loadtxt(os.path.join(root, "viz0", name)), np.loadtxt(os.path.join(root, "viz1", name)))
    (args, kw), = calls
    dirs, schedules = args[0], args[1]
    assert dirs == [os.path.join(root, "viz1", str(e), "short") for e in (1, 1, 2, 2)]
    want = sorted(os.path.join(d, f"{s:06}_{e:06}_{n}.png") for d, sched in zip(dirs, schedules) for s, e in sched for n in ("pred", "gt", "both"))
    got = sorted(os.path.join(dp, f) for dp, _, fs in os.walk(os.path.join(root, "viz1")) for f in fs if f.endswith(".png"))
    assert got == want and len(want) == 3 * sum(len(s) for s in schedules) > 0
    assert not [f for _, _, fs in os.walk(os.path.join(root, "viz0")) for f in fs if f.endswith(".png")]
    # the same display list over the host render, by the host statement: the same files
    host_dirs = [d.replace("viz1", "host") for d in dirs]
    for d in host_dirs:
        os.makedirs(d, exist_ok=True)
    real(host_dirs, *args[1:10], None, **kw)
    blue = 0
    for path in want:
        image = viz.read_png(path)
        assert np.array_equal(image, viz.read_png(path.replace("viz1", "host"))), path
        assert image.shape == ((90, 320, 3) if path.endswith("both.png") else (90, 160, 3))
        blue += int((image == np.array([0, 0, 255], np.uint8)).all(-1).sum())
    assert blue > 0                                                                              # key points were drawn
    first = want[0].replace("_both.png", "")
    assert np.array_equal(viz.read_png(first + "_both.png"), np.concatenate([viz.read_png(first + "_pred.png"), viz.read_png(first + "_gt.png")], 1))
    # launches of 6 frames, each with its own rollouts' points and primitives alone: the same files
    small_dirs = [d.replace("viz1", "small") for d in dirs]
    for d in small_dirs:
        os.makedirs(d, exist_ok=True)
    real(small_dirs, *args[1:], batch=6, **kw)
    assert all(np.array_equal(viz.read_png(path), viz.read_png(path.replace("viz1", "small"))) for path in want)
    # one time per picture (rollout.py:40-57, :140-146): the frame {start}_{end} shows the graph step t's forward reads, all at frame `start`
    pred, gt, eef, edges, n_kp, max_nobj, particles = args[2:9]
    ratio = configs.task_config("rope")["sim_real_ratio"]
    cam = [[x[0]] for x in render.default_cameras(ratio, 720, 1280)]      # at full size a 3 mm particle is a disc of three pixels' radius
    radius = np.array([np.float32(0.03) * np.float32(1.0 / ratio)], np.float32)
    for b, sched in enumerate(schedules):
        k = n_kp[b]
        assert torch.equal(pred[b, 0, :k], gt[b, 0, :k])                                         # the start graph: its key points ARE the recorded ones
        for t, (start, end) in enumerate(sched):
            kp, cloud = gt[b, t, :k].cpu().numpy(), np.asarray(particles[b][t], np.float32)
            assert np.array_equal(cloud, np.asarray(g["obj_pos"][dirs_episode(dirs[b])][start], np.float32))
            assert (kp[:, None, :] == cloud[None, :, :]).all(-1).any(1).all(), (b, t)            # every recorded key point is a particle of frame `start`
            assert torch.equal(eef[b, t].cpu(), torch.from_numpy(np.asarray(g["eef_pos"][dirs_episode(dirs[b])][start], np.float32)))
        for t in (0, len(sched) - 1):                                                            # and lies on that frame's rendered spheres
            cloud = to_board_frame(np.asarray(particles[b][t], np.float32), ratio)
            ids = render.render_depth_host(cloud[None], np.array([len(cloud)], np.int32), radius, *cam, 720, 1280, (0.0, 0.0, 1.0, 0.0))[1][0, 0]
            x, y, valid = viz.project_host(to_board_frame(gt[b, t, :k].cpu().numpy(), ratio), render.camera_rows(*cam)[0], 0.05)
            # (a key point out of view has no pixel; the golden recording has particles whose centre lies under the table plane, y < 0,
            # which the table hides: the sphere must show where its centre is above it)
            seen = valid & (x >= 0) & (x < 1280) & (y >= 0) & (y < 720) & (gt[b, t, :k, 1].cpu().numpy() > 0)
            assert seen.sum() >= 3 and (ids[y[seen], x[seen]] >= 0).all(), (b, t)
    # the edges of frame t are those of the drawn points: ag_build_edges of (key points, tool) of the same frame
    from adaptigraph_amd.graph import build_edges
    P = er._dataset_params(cfg["dataset_config"])
    for t in (0, max(len(s) for s in schedules) - 1):
        state = torch.cat([pred[:, t], eef[:, t]], 1)
        mask = torch.zeros(state.shape[:2], dtype=torch.bool, device=DEV)
        for b, k in enumerate(n_kp):
            mask[b, :k] = True
        mask[:, max_nobj:] = True
        tool = torch.zeros_like(mask)
        tool[:, max_nobj:] = True
        again = build_edges(state, P["adj_thresh"], mask, tool, P["topk"], P["connect_tool_all"], "single", max_tools=eef.shape[2])
        assert all(np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) for a, c in zip(again.to_lists(), edges[t].to_lists()))


def dirs_episode(path):
    """.../<episode>/short -> the episode's index."""
    return int(os.path.basename(os.path.dirname(path)))


def test_closed_loop_on_the_device_draws_without_changing_the_run(tmp_path):
    from adaptigraph_amd.closed_loop import run_closed_loop
    from adaptigraph_amd.forward_dynamics import dynamics
    from adaptigraph_amd.model import DynamicsPredictor
    mat = "rope"
    task = configs.task_config(mat)
    tg = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)      # noqa: E731
    lo, hi = tg([-1.0, 0.2, 1.3, 5.0]), tg([1.0, 0.3, 1.8, 8.0])
    target = tg([[0.1 * i - 1.0, 0.03, -0.5] for i in range(20)])
    runs = []
    for name, kw in (("plain", {}), ("viz", dict(viz=True, target_state=target))):
        torch.manual_seed(0)
        np.random.seed(0)
        model = DynamicsPredictor(configs.model_config(), configs.material_config(mat), configs.dataset_config(mat), DEV).to(DEV).eval()
        ppm = configs.ppm_optimizer_stub(mat)
        ppm.physics_param = {mat: torch.tensor([0.5], device=DEV)}
        criteria = partial(losses.chamfer, y=target[None])
        cfg = dict(action_dim=4, model_rollout_fn=partial(dynamics, model=model, device=DEV, ppm_optimizer=ppm),
                   evaluate_traj_fn=partial(mpc.running_cost, error_func=criteria,
                                            penalty_func=partial(losses.rope_penalty, sim_real_ratio=task["sim_real_ratio"]),
                                            bbox=np.array([[-3.0, 3.0], [-3.0, 3.0]])),
                   n_sample=32, n_look_ahead=2, n_update_iter=1, reward_weight=task["reward_weight"], action_lower_lim=lo, action_upper_lim=hi,
                   planner_type="MPPI", device=DEV, noise_level=0.3)
        out = tmp_path / name
        acts, errors = run_closed_loop(SeededEnv(rope_env(DEV)), mpc.Planner(cfg), criteria, 2, 2, lo, hi, task["fps_radius"],
                                       save_dir=str(out), **kw)
        runs.append((acts.cpu(), errors, [dict(np.load(str(out / f"interaction_{i}.npz"))) for i in range(2)]))
    (a0, e0, r0), (a1, e1, r1) = runs
    assert torch.equal(a0, a1) and e0 == e1
    assert all(set(x) == set(y) and all(np.array_equal(x[k], y[k]) for k in x) for x, y in zip(r0, r1))
    assert sorted(p.name for p in (tmp_path / "viz").glob("*.png")) == [f"rgb_vis_{i}_{j}.png" for i in range(2) for j in range(2)]
    assert not list((tmp_path / "plain").glob("*.png"))
    image = viz.read_png(str(tmp_path / "viz" / "rgb_vis_0_0.png"))
    colours = {tuple(c) for c in image.reshape(-1, 3)}
    assert image.shape == (90, 160, 3) and (202, 63, 41) in colours and (27, 74, 242) in colours
