"""ag_jpeg_encode (csrc/ag_jpeg.hip) against the JPEG statement (jpeg.jpeg_scan_host), byte for byte, and the places that use it: the closed
loop's video and the evaluation rollout's .jpg files and videos."""
import os
from functools import partial

import numpy as np
import pytest
import torch

from adaptigraph_amd import configs, jpeg, losses, mpc, viz
from jpeg_cases import content_cases, drawn, gradient, noise
from viz_cases import SeededEnv, engine_model, rollout_dataset_on_disk, rope_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def same(images, quality=90, subsampling="420", restart=8, encoder=None):
    """The device scans equal the host statement's, offsets included; -> the scans."""
    images = np.ascontiguousarray(images)
    want = jpeg.jpeg_scan_host(images, quality, subsampling, restart)
    F, H, W, C = images.shape
    enc = encoder or jpeg.DeviceEncoder(H, W, F, quality, subsampling, restart, channels=C, device=DEV)
    out, offsets = enc.launch(torch.from_numpy(images).to(DEV))
    at = offsets.cpu().numpy()
    assert offsets.dtype == torch.int64 and at.tolist() == np.concatenate([[0], np.cumsum([len(s) for s in want])]).tolist()
    data = out[:at[-1]].cpu().numpy().tobytes()
    got = [data[at[f]:at[f + 1]] for f in range(F)]
    assert got == want
    assert enc.scans(torch.from_numpy(images).to(DEV)) == want
    return got


@pytest.mark.parametrize("subsampling", ["444", "420"])
@pytest.mark.parametrize("H,W", [(1, 1), (7, 9), (8, 8), (9, 7), (15, 17), (16, 16), (17, 15), (1, 17), (16, 1), (8, 16), (33, 47)])
def test_image_sides_around_the_mcu(H, W, subsampling):
    same(noise(H, W, H * 100 + W)[None], 90, subsampling, 3)


@pytest.mark.parametrize("subsampling", ["444", "420"])
@pytest.mark.parametrize("restart", [1, 3, 8, jpeg.MAX_RESTART])
def test_restart_intervals_short_last_segments_and_one_segment(restart, subsampling):
    """33 x 47: 5 x 6 = 30 MCUs in 4:4:4 (restart 8: a last segment of 6; 16: of 14), 3 x 3 = 9 in 4:2:0 (8: a last segment of one MCU; 16: above
    the MCU count, one segment and no marker)."""
    scans = same(np.stack([drawn(33, 47)[..., :3], noise(33, 47, restart)]), 90, subsampling, restart)
    segments = jpeg.geometry(33, 47, subsampling, restart)[4]
    assert segments == {("444", 1): 30, ("444", 3): 10, ("444", 8): 4, ("444", 16): 2, ("420", 1): 9, ("420", 3): 3, ("420", 8): 2, ("420", 16): 1}[
        (subsampling, restart)]


@pytest.mark.parametrize("quality", [1, 50, 90, 100])
def test_qualities_and_three_frames_of_different_content(quality):
    frames = np.stack([gradient(33, 47), drawn(33, 47)[..., :3], noise(33, 47, quality)])
    scans = same(frames, quality, "420", 8)
    assert len(set(scans)) == 3 and scans[0] == same(frames[:1], quality, "420", 8)[0]


def test_rgba_frames_and_the_alpha_byte():
    rgba = drawn(33, 47)
    assert rgba.shape[-1] == 4
    a = same(rgba[None], 90, "420", 8)
    other = rgba.copy()
    other[..., 3] = 0
    assert same(other[None], 90, "420", 8) == a == same(np.ascontiguousarray(rgba[None, ..., :3]), 90, "420", 8)
    assert same(noise(17, 9, 2, 4)[None], 75, "444", 2) == same(noise(17, 9, 2, 4)[None, ..., :3], 75, "444", 2)


@pytest.mark.parametrize("name", sorted(content_cases()))
def test_every_coding_path_of_the_statement(name):
    images, quality, subsampling, restart = content_cases()[name]
    same(images, quality, subsampling, restart)


def test_one_full_size_frame():
    H, W = 720, 1280
    frame = gradient(H, W)
    frame[200:520, 300:900] = noise(320, 600, 8)
    frame[::7, ::5] = 255
    scans = same(frame[None], 90, "420", 8)
    assert 50000 < len(scans[0]) < jpeg.out_bytes(1, H, W, "420", 8)


def test_same_bytes_every_call_stale_scratch_and_a_partly_used_encoder():
    big = np.stack([noise(33, 47, s) for s in range(4)])
    enc = jpeg.DeviceEncoder(33, 47, 4, 100, "420", 8, channels=3, device=DEV)
    first = same(big, 100, "420", 8, encoder=enc)
    assert same(big, 100, "420", 8, encoder=enc) == first                               # two calls: the same bytes
    small = np.stack([np.full((33, 47, 3), 77, np.uint8), gradient(33, 47)])
    got = same(small, 100, "420", 8, encoder=enc)                                       # an encoder built for 4 frames, used for 2, after a larger call
    assert sum(map(len, got)) < sum(map(len, first)) // 4
    other = jpeg.DeviceEncoder(9, 7, 1, 50, "444", 1, channels=3, device=DEV)           # another geometry over the large call's scratch and output
    other.scratch, other.scratch_bytes, other.out, other.out_bytes = enc.scratch, enc.scratch_bytes, enc.out, enc.out_bytes
    same(big, 100, "420", 8, encoder=enc)
    same(noise(9, 7, 3)[None], 50, "444", 1, encoder=other)
    with pytest.raises(ValueError):
        enc.launch(torch.from_numpy(np.concatenate([big, big])).to(DEV))                # more frames than it holds
    with pytest.raises(ValueError):
        enc.launch(torch.from_numpy(big).to(DEV).float())
    assert enc.scans(torch.from_numpy(np.concatenate([big, small])).to(DEV)) == first + got      # `scans` takes them four at a time


def test_launch_captures_into_a_graph():
    H, W = 33, 47
    contents = [np.stack([noise(H, W, 30 + i, 4), drawn(H, W) if i % 2 else noise(H, W, 40 + i, 4)]) for i in range(3)]
    images = torch.from_numpy(contents[0]).to(DEV)
    enc = jpeg.DeviceEncoder(H, W, 2, 90, "420", 3, channels=4, device=DEV)
    enc.launch(images)                                                                  # warm up: the first launch loads the code object
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, offsets = enc.launch(images)
    for i in (1, 2, 0):
        images.copy_(torch.from_numpy(contents[i]).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        want = jpeg.jpeg_scan_host(contents[i], 90, "420", 3)
        at = offsets.cpu().numpy()
        data = out[:at[-1]].cpu().numpy().tobytes()
        assert [data[at[f]:at[f + 1]] for f in range(2)] == want, i


def test_encode_jpeg_and_video_writer_on_the_device_write_the_host_s_files(tmp_path):
    frames = np.stack([drawn(33, 47), noise(33, 47, 9, 4), drawn(33, 47)[::-1].copy()])
    assert jpeg.encode_jpeg(frames, 75, "444", 5, device=DEV) == jpeg.encode_jpeg(frames, 75, "444", 5)
    assert jpeg.encode_jpeg(torch.from_numpy(frames[0]).to(DEV), device=DEV) == jpeg.encode_jpeg(frames[0])
    for name, device in (("host", None), ("dev", DEV)):
        with jpeg.VideoWriter(str(tmp_path / f"{name}.avi"), 33, 47, 10, device=device) as out:
            out.add(torch.from_numpy(frames[:1]).to(DEV) if device else frames[:1])
            out.add(frames[1:])                                                         # two frames through an encoder built for one
    assert (tmp_path / "host.avi").read_bytes() == (tmp_path / "dev.avi").read_bytes()
    assert jpeg.avi_frames(str(tmp_path / "dev.avi")) == jpeg.encode_jpeg(frames)


# ------------------------------------------------------------------------------------------------------ where it is used
def test_closed_loop_video_on_the_device_is_the_host_s_file(tmp_path):
    from adaptigraph_amd.closed_loop import run_closed_loop
    from adaptigraph_amd.forward_dynamics import dynamics
    from adaptigraph_amd.model import DynamicsPredictor
    mat = "rope"
    task = configs.task_config(mat)
    tg = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)      # noqa: E731
    lo, hi = tg([-1.0, 0.2, 1.3, 5.0]), tg([1.0, 0.3, 1.8, 8.0])
    target = tg([[0.1 * i - 1.0, 0.03, -0.5] for i in range(20)])
    runs = []
    for name, video in (("viz", False), ("video", True)):
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
        acts, errors = run_closed_loop(SeededEnv(rope_env(DEV)), mpc.Planner(cfg), criteria, 2, 2, lo, hi, task["fps_radius"], save_dir=str(out),
                                       viz=True, target_state=target, video=video)
        runs.append((acts.cpu(), errors, [dict(np.load(str(out / f"interaction_{i}.npz"))) for i in range(2)]))
    (a0, e0, r0), (a1, e1, r1) = runs
    assert torch.equal(a0, a1) and e0 == e1
    assert all(set(x) == set(y) and all(np.array_equal(x[k], y[k]) for k in x) for x, y in zip(r0, r1))
    names = [f"rgb_vis_{i}_{j}.png" for i in range(2) for j in range(2)]
    assert sorted(p.name for p in (tmp_path / "video").iterdir() if p.suffix != ".npz") == sorted(names + ["rgb_vis.avi"])
    assert sorted(p.name for p in (tmp_path / "viz").iterdir() if p.suffix != ".npz") == names
    pngs = [viz.read_png(str(tmp_path / "video" / n)) for n in names]
    assert all(np.array_equal(p, viz.read_png(str(tmp_path / "viz" / n))) for p, n in zip(pngs, names))
    with jpeg.VideoWriter(str(tmp_path / "host.avi"), 90, 160, 1) as out:               # the host path: the statement over the same images
        out.add(np.stack(pngs))
    assert (tmp_path / "host.avi").read_bytes() == (tmp_path / "video" / "rgb_vis.avi").read_bytes()
    with pytest.raises(ValueError, match="video"):
        run_closed_loop(SeededEnv(rope_env(DEV)), None, None, 1, 1, lo, hi, 0.2, video=True)


@pytest.mark.parametrize("scripted", [False, True])
def test_rollout_dataset_jpg_files_and_videos_are_the_host_s(tmp_path, monkeypatch, scripted):
    import adaptigraph_amd.eval_rollout as er
    root = str(tmp_path)
    g, cfg = rollout_dataset_on_disk(root)
    cfg["rollout_config"]["viz_size"] = (90, 160)
    model = engine_model("rope", 0)
    calls = []
    real = viz.write_rollout_record
    monkeypatch.setattr(viz, "write_rollout_record", lambda *a, **k: calls.append((a, k)) or real(*a, **k))
    curves = {}
    for name, options in (("plain", None), ("png", {}), ("jpg", dict(viz_video=True, viz_format="jpg"))):
        out = os.path.join(root, name)
        os.makedirs(out)
        np.random.seed(int(g["seed"]))
        cfg["rollout_config"] = dict({"out_dir": cfg["rollout_config"]["out_dir"], "viz_size": (90, 160)}, **(options or {}))
        curves[name] = er.rollout_dataset(model, DEV, cfg, out, viz=options is not None, scripted=scripted)
    assert np.array_equal(curves["plain"], curves["png"]) and np.array_equal(curves["plain"], curves["jpg"]) and len(calls) == 2
    for e in (1, 2):
        for k in (1, 2):
            name = os.path.join(str(e), "short", f"error_{k}.txt")
            assert np.array_equal(np.loadtxt(os.path.join(root, "plain", name)), np.loadtxt(os.path.join(root, "jpg", name)))
    (args, kw) = calls[1]
    assert kw["video"] is True and kw["fmt"] == "jpg" and calls[0][1]["video"] is False and calls[0][1]["fmt"] == "png"
    dirs, schedules = args[0], args[1]
    listing = lambda top, ext: sorted(os.path.relpath(os.path.join(dp, f), top) for dp, _, fs in os.walk(top) for f in fs if f.endswith(ext))      # noqa: E731
    stems = sorted({os.path.join(os.path.relpath(d, os.path.join(root, "jpg")), f"{s:06}_{e:06}") for d, sched in zip(dirs, schedules) for s, e in sched})
    assert listing(os.path.join(root, "jpg"), ".jpg") == sorted(f"{s}_{n}.jpg" for s in stems for n in ("pred", "gt", "both"))
    assert listing(os.path.join(root, "jpg"), ".avi") == sorted(os.path.join(str(e), "short", f"{n}.avi") for e in (1, 2) for n in ("pred", "gt", "both"))
    assert not listing(os.path.join(root, "jpg"), ".png") and not listing(os.path.join(root, "png"), ".avi") + listing(os.path.join(root, "png"), ".jpg")
    # the same record by the host statements: the same files, byte for byte
    host_dirs = [d.replace(os.path.join(root, "jpg"), os.path.join(root, "host")) for d in dirs]
    for d in host_dirs:
        os.makedirs(d, exist_ok=True)
    real(host_dirs, *args[1:10], None, **kw)
    files = listing(os.path.join(root, "jpg"), ".jpg") + listing(os.path.join(root, "jpg"), ".avi")
    assert files == listing(os.path.join(root, "host"), ".jpg") + listing(os.path.join(root, "host"), ".avi")
    for f in files:
        assert open(os.path.join(root, "jpg", f), "rb").read() == open(os.path.join(root, "host", f), "rb").read(), f
    # a video holds its directory's frames in file-name order, and a .jpg is the .png of the other run, encoded
    for e in (1, 2):
        d = os.path.join(root, "jpg", str(e), "short")
        for n in ("pred", "both"):
            names = sorted(f for f in os.listdir(d) if f.endswith(f"_{n}.jpg"))
            assert jpeg.avi_frames(os.path.join(d, f"{n}.avi")) == [open(os.path.join(d, f), "rb").read() for f in names] and len(names) >= 2
            png = viz.read_png(os.path.join(root, "png", str(e), "short", names[0].replace(".jpg", ".png")))
            assert open(os.path.join(d, names[0]), "rb").read() == jpeg.encode_jpeg(png)[0]
