"""The cloth grasp-and-drag kernel (csrc/ag_sim_cloth.hip through sim.cloth_push) against the host statement sim.cloth_push_host, bit for bit:
the grid sizes at which the four-particles-per-thread layout and the tails of the twelve phases take another path, several episodes in one
launch, the degenerate pairs and picks, the shipped constants, determinism, graph capture, argument errors, and the dataset writer end to end
into train()."""
import os

import numpy as np
import pytest
import torch

from adaptigraph_amd import configs, datagen, sim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
NAMES = ("obj", "eef", "n_frames", "picked", "x", "v")
# a drag 1.0 long at 0.1 per step rising by 0.3: 11 steps, then 4 steps down (frames after steps 0, 4, 8, 12); 2 substeps of 2 sweeps, 3 settle steps
SMALL = sim.ClothParams(substeps=2, iters=2, speed=0.1, lift=0.3, record_every=4, settle=3)


def flat(nx, nz, l0=0.125, y=SMALL.r):
    """An axis-aligned grid of exact coordinates, centred at the origin."""
    gx, gz = np.meshgrid((np.arange(nx) - (nx - 1) / 2) * l0, (np.arange(nz) - (nz - 1) / 2) * l0)
    return np.stack([gx, np.full_like(gx, y), gz], 2).astype(F32)


def turned(nx, nz, seed, l0=0.05):
    """A grid turned about the vertical by a random angle (inexact coordinates), at spacing l0."""
    return sim.initial_cloth(np.random.default_rng(seed), nx, nz, side_range=((max(nx, nz) - 1) * l0,) * 2)[0]


def drag_from(p, dx=-0.9, dz=-0.4):
    return np.array([p[0], p[2], p[0] + dx, p[2] + dz], F32)


def assert_same(scene, action, params=SMALL, f_max=None):
    host = sim.cloth_push_host(scene, action, params, f_max)
    got = sim.cloth_push(scene, action, params, f_max, device=DEV)
    for name, h, d in zip(NAMES, host, got):
        assert d.device.type == "cuda" and torch.equal(d.cpu(), torch.from_numpy(h)), name
    return host


@pytest.mark.parametrize("nx,nz", [(2, 2), (3, 3), (2, 5), (5, 2), (5, 6), (31, 33), (32, 32), (33, 32), (64, 63), (64, 64)])
def test_one_episode_equals_the_host_at_every_size_class(nx, nz):
    """2 x 2: the minimum, no bend pair; 3 x 3: the first bend pair, one colour; 2 x 5, 5 x 2: bend in one direction only; 5 x 6: both colours of
    every family, odd and even rows; 31 x 33: 1 023 particles; 32 x 32: one full round of the workgroup; 33 x 32: the second particle of the
    first threads; 64 x 63: nearly full; 64 x 64: four particles in every thread.  Grasped at the corner (0, 0) and dragged away from the cloth."""
    cloth = turned(nx, nz, seed=100 * nx + nz)
    scene = sim.ClothScene.from_cloths([cloth], sf=[0.4], l0=[0.05])
    out = cloth[0, 0] - cloth[min(nz - 1, 2), min(nx - 1, 2)]
    out = out / np.linalg.norm(out)
    obj, eef, n_frames, picked, x, v = assert_same(scene, drag_from(cloth[0, 0], out[0], out[2])[None])
    assert n_frames[0] == 5 and picked[0, 0] == 0 and (picked[0] >= 0).sum() == min(nx * nz, 5) and eef.shape == (1, 5, 2, 3)
    assert np.abs(x - scene.x).max() > 0.3 and np.isfinite(x).all()


def test_three_episodes_of_different_grids_share_one_launch():
    """3 x 4, 40 x 17 and 9 x 9 under n_max = 680; drags of 11 + 4, 6 + 4 and 19 + 4 steps: 5, 4 and 7 frames under one F_max; the middle
    episode's grasp misses.  Rows behind n and frames behind n_frames stay zero, also with more frames than any drag writes."""
    cloths = [turned(3, 4, 1), turned(40, 17, 2), turned(9, 9, 3)]
    scene = sim.ClothScene.from_cloths(cloths, sf=[0.1, 0.6, 0.95], l0=[0.05] * 3)
    action = np.stack([drag_from(cloths[0][0, 0]), drag_from(cloths[1][0, 0] + F32(3.0), 0.5, 0.0), drag_from(cloths[2][0, 0], -1.7, -0.6)])
    obj, eef, n_frames, picked, x, v = assert_same(scene, action)
    assert list(n_frames) == [5, 4, 7] and picked[1].tolist() == [-1] * 5 and picked[0, 0] == 0 and picked[2, 0] == 0
    assert not x[0, 12:].any() and not obj[0, :, 12:].any() and not obj[2, :, 81:].any() and not obj[0, 5:].any() and not obj[1, 4:].any()
    assert_same(scene, action, f_max=10)


def test_pick_ties_go_to_the_lower_index():
    """An action exactly between two and exactly between four particles of a grid of exact coordinates, and a 2 x 2 cloth with four to grasp."""
    c = flat(4, 4)
    scene = sim.ClothScene.from_cloths([c, c, flat(2, 2)], sf=[0.5] * 3, l0=[0.125] * 3)
    mx, mz = (c[0, 0, 0] + c[0, 1, 0]) / 2, (c[0, 0, 2] + c[1, 0, 2]) / 2
    action = np.array([[mx, c[0, 0, 2], mx - 1, c[0, 0, 2]], [mx, mz, mx - 1, mz - 0.2], [0, 0, 0.7, 0.7]], F32)
    picked = assert_same(scene, action)[3]
    assert picked.tolist() == [[0, 1, 4, 5, 2], [0, 1, 4, 5, 2], [0, 1, 2, 3, -1]]


def test_two_particles_at_the_same_point():
    """Particle 1 starts on top of particle 0: len == 0 for their stretch pair in the first phase, which is skipped; nothing divides by 0."""
    c = flat(4, 3)
    c[0, 1] = c[0, 0]
    scene = sim.ClothScene.from_cloths([c], sf=[0.5], l0=[0.125])
    obj, eef, n_frames, picked, x, v = assert_same(scene, drag_from(c[2, 3], 0.9, 0.4)[None])
    assert np.isfinite(obj).all() and np.isfinite(v).all() and picked[0, 0] == 11


def test_a_grasp_that_holds_both_ends_of_a_pair():
    """The five grasped particles of a corner pick are neighbours: w_i + w_j == 0 for the pairs among them, which are skipped; the pins keep
    their mutual offsets through the whole drag."""
    c = turned(6, 6, 8)
    scene = sim.ClothScene.from_cloths([c], sf=[0.7], l0=[0.05])
    obj, eef, n_frames, picked, x, v = assert_same(scene, drag_from(c[0, 0])[None])
    assert sorted(picked[0].tolist()) == [0, 1, 2, 6, 7] or sorted(picked[0].tolist()) == [0, 1, 6, 7, 12]
    i, j = picked[0, 0], picked[0, 1]
    for f in range(n_frames[0] - 1):
        assert np.abs((obj[0, f, j] - obj[0, f, i]) - (scene.x[0, j] - scene.x[0, i])).max() < 1e-6


def test_a_drag_of_no_horizontal_length():
    """xs == xe and zs == ze: straight up and down again; the lateral vector is (0, 1) by definition."""
    c = turned(7, 5, 4)
    scene = sim.ClothScene.from_cloths([c], sf=[0.3], l0=[0.05])
    p = c[2, 3]
    obj, eef, n_frames, picked, x, v = assert_same(scene, np.array([[p[0], p[2], p[0], p[2]]], F32))
    assert picked[0, 0] == 17 and n_frames[0] == 3 and obj[0, 0, 17, 1] > SMALL.r and eef[0, 0, 0, 2] - eef[0, 0, 1, 2] == F32(2 * SMALL.finger)


def test_default_parameters_one_drag():
    """The shipped constants (4 substeps of 4 sweeps, a frame every 5 steps, 120 settle steps) on a 20 x 20 cloth 2.5 a side, a drag of 66 + 26 steps."""
    cloth, l0 = sim.initial_cloth(np.random.default_rng(0), 20, 20, side_range=(2.5, 2.5), rotate=False)
    scene = sim.ClothScene.from_cloths([cloth], sf=[0.5], l0=[l0])
    obj, eef, n_frames, picked, x, v = assert_same(scene, drag_from(cloth[0, 19], 1.2, 0.0)[None], sim.CLOTH_DEFAULT)
    assert n_frames[0] == 20 and not v.any() and np.abs(x - scene.x).max() > 1.0


def test_two_calls_give_the_same_bits_and_a_graph_replays_them():
    cloths = [turned(33, 32, 1), turned(6, 5, 2)]
    scene = sim.ClothScene.from_cloths(cloths, sf=[0.2, 0.8], l0=[0.05] * 2)
    action = np.stack([drag_from(c[0, 0]) for c in cloths])
    first = [t.clone() for t in sim.cloth_push(scene, action, SMALL, device=DEV)]
    again = sim.cloth_push(scene, action, SMALL, device=DEV)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    call = sim.DeviceClothPush(scene, action, SMALL, device=DEV)
    x0, v0 = call.x.clone(), call.v.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # warm-up outside the capture
        call.launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call.x.copy_(x0)
        call.v.copy_(v0)
        call.launch()
    outs = (call.obj, call.eef, call.n_frames, call.picked, call.x, call.v)
    for _ in range(3):      # every replay restores x, v and rewrites every frame
        for t in outs:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, outs))


@pytest.mark.parametrize("what", ["n_max = 4097", "n_max = 3", "F_max too small", "iters = 0", "substeps = 0", "record_every = 0"])
def test_argument_errors_leave_the_outputs_untouched(what):
    c = flat(4, 3)
    scene = sim.ClothScene.from_cloths([c], sf=[0.5], l0=[0.125], n_max={"n_max = 4097": 4097, "n_max = 3": 12}.get(what, 12))
    if what == "n_max = 3":
        scene.x, scene.v = scene.x[:, :3].copy(), scene.v[:, :3].copy()
    params = {"iters = 0": dict(iters=0), "substeps = 0": dict(substeps=0), "record_every = 0": dict(record_every=0)}.get(what, {})
    params = sim.ClothParams(**dict(dict(substeps=2, iters=2, speed=0.1, lift=0.3, record_every=4, settle=3), **params))
    if what in ("substeps = 0", "record_every = 0"):      # (the host's own step arithmetic divides by them: build the call with sound values first)
        call = sim.DeviceClothPush(scene, drag_from(c[0, 0])[None], SMALL, device=DEV)
        call.dims = call.dims[:4] + (int(params.substeps), call.dims[5], int(params.record_every), call.dims[7])
    else:
        call = sim.DeviceClothPush(scene, drag_from(c[0, 0])[None], params, f_max=4 if what == "F_max too small" else None, device=DEV)      # the drag writes 5
    outs = (call.obj, call.eef, call.n_frames, call.picked, call.x, call.v)
    for t in outs:
        t.fill_(7)
    with pytest.raises(RuntimeError, match=r"ag_sim_cloth_push failed \(-1\)"):
        call.launch()
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outs)


def test_a_null_pointer_is_an_argument_error():
    c = flat(4, 3)
    call = sim.DeviceClothPush(sim.ClothScene.from_cloths([c], sf=[0.5], l0=[0.125]), drag_from(c[0, 0])[None], SMALL, device=DEV)
    call.picked = None
    with pytest.raises(RuntimeError, match=r"ag_sim_cloth_push failed \(-1\)"):
        call.launch()


@pytest.mark.parametrize("what", ["nx = 1", "nx = 65", "nz = 1", "nx nz > n_max", "n1 = 0", "n2 = 0", "n1 + n2 > n_push_max"])
def test_an_episode_outside_the_bounds_writes_no_frame_and_nothing_else(what):
    """The per-episode grid sizes and step counts are device arrays the library's host checks cannot see: an episode with one of them outside
    the bounds gets n_frames = 0 and its outputs and state stay as they were, while its neighbour in the same launch is simulated as if alone.
    cloth_push refuses such a grid with cloth_push_host's error before any launch."""
    good = turned(5, 4, 5)
    scene = sim.ClothScene.from_cloths([good, good], sf=[0.5, 0.2], l0=[0.05] * 2)
    action = np.stack([drag_from(good[0, 0]), drag_from(good[0, 0])])
    call = sim.DeviceClothPush(scene, action, SMALL, device=DEV)
    if what.startswith("n1") or what.startswith("n2"):
        steps = call.steps.cpu()
        if what == "n1 + n2 > n_push_max":
            steps[0, 0] += 1
        else:
            steps[0, int(what[1]) - 1] = 0
        call.steps.copy_(steps)
    else:
        nx, nz = {"nx = 1": (1, 4), "nx = 65": (65, 4), "nz = 1": (5, 1), "nx nz > n_max": (7, 3)}[what]
        scene.nx[0], scene.nz[0] = nx, nz
        for run in (lambda: sim.cloth_push_host(scene, action, SMALL), lambda: sim.cloth_push(scene, action, SMALL, device=DEV)):
            with pytest.raises(ValueError, match="nx, nz outside 2 .. 64 or nx nz > n_max = 20"):
                run()
        call = sim.DeviceClothPush(scene, action, SMALL, device=DEV)
    outs = (call.obj, call.eef, call.n_frames, call.picked, call.x, call.v)
    for t in outs:
        t[0].fill_(7)
    call.launch()
    torch.cuda.synchronize()
    assert call.n_frames.tolist() == [0, 5] and all(bool((t[0] == 7).all()) for t in (call.obj, call.eef, call.picked, call.x, call.v))
    alone = sim.cloth_push_host(sim.ClothScene.from_cloths([good], sf=[0.2], l0=[0.05]), action[1:], SMALL)
    for name, h, d in zip(NAMES, alone, outs):
        assert torch.equal(d[1:].cpu(), torch.from_numpy(h)), name


def tree_bytes(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def test_dataset_on_the_device_equals_the_host_and_trains(tmp_path):
    """4 episodes x 2 drags of cloths of 8 to 12 particles a side, 1.0 to 1.2 long (one launch per round of drags): device= writes the bytes
    device=None writes; train() runs 2 iterations on it with the cloth material, the gripper's two tool points joined to every key point and
    topk 5, the batches assembled on the host and on the device, to a finite loss.  The reference's fps_radius_range [0.24, 0.26] is for cloths
    2 to 3 a side; scaled to these (0.4 of that size) it is [0.096, 0.104], the adjacency radius likewise."""
    from adaptigraph_amd import train as agtrain
    kw = dict(params=SMALL, grid=(8, 12), side_range=(1.0, 1.2))
    host = datagen.generate_cloth_dataset(str(tmp_path / "host"), 4, 2, seed=11, device=None, **kw)
    dev = datagen.generate_cloth_dataset(str(tmp_path / "dev"), 4, 2, seed=11, device=DEV, **kw)
    files = tree_bytes(tmp_path / "dev")
    assert len(files) == 4 + 8 + 3 and files == tree_bytes(tmp_path / "host") and host["n_his"] == dev["n_his"]
    for device_batches in (False, True):
        ds = dict(dev, device=DEV, ratio={"train": [0, 0.75], "valid": [0.75, 1.0]}, verbose=False,
                  randomness={"use": True, "state_noise": {"train": 0.05, "valid": 0.0}, "phys_noise": {"train": 0.0, "valid": 0.0}},
                  datasets=[dict(name="cloth", max_nobj=40, max_nR=1600, fps_radius_range=[0.096, 0.104], adj_radius_range=[0.28, 0.32], topk=5,
                                 connect_tool_all=True)])
        cfg = {"dataset_config": ds, "material_config": configs.material_config("cloth"), "model_config": configs.model_config(),
               "train_config": {"random_seed": 42, "out_dir": str(tmp_path / f"log{int(device_batches)}"), "phases": ["train", "valid"],
                                "num_workers": 0, "batch_size": 4, "n_epochs": 1, "log_interval": 1, "n_iters_per_epoch": {"train": 2, "valid": 1},
                                "device_batches": device_batches}}
        hist = agtrain.train(cfg)
        assert len(hist["train"]) == 1 and np.isfinite(hist["train"]).all() and np.isfinite(hist["valid"]).all()
