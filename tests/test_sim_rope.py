"""The rope push kernel (csrc/ag_sim.hip through sim.rope_push) against the host restatement sim.rope_push_host, bit for bit: the smallest
shapes at which the kernel takes another path, determinism, graph capture, argument errors, and the dataset writer end to end into train()."""
import os

import numpy as np
import pytest
import torch

from adaptigraph_amd import configs, datagen, sim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
# 13 push steps of 2 substeps (a push 0.5 long at 0.04 per step), a frame every 4 steps (4 does not divide 13: frames after steps 0, 4, 8, 12), 3 settle steps
SMALL = sim.SimParams(substeps=2, speed=0.04, record_every=4, settle=3)
ACROSS = lambda xm: np.array([xm, -0.25, xm, 0.25], F32)      # through the rope at x = xm, 0.5 long  # noqa: E731


def wavy_rope(n, seed):
    """n particles along x at spacing about 0.05 with a small lateral wave and jitter: nothing is exact, every constraint has work to do."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    p = np.stack([0.05 * i, np.full(n, SMALL.r), 0.02 * np.sin(0.7 * i)], 1) + rng.normal(0, 0.002, (n, 3)) * [1, 0, 1]
    return p.astype(F32)


def scene_of(ns, ws, kappas=None, seed=0):
    ropes = [wavy_rope(n, seed + k) for k, n in enumerate(ns)]
    return sim.RopeScene.from_ropes(ropes, w=ws, kappa=[0.35] * len(ns) if kappas is None else kappas)


def assert_same(scene, push, params=SMALL, f_max=None):
    host = sim.rope_push_host(scene, push, params, f_max)
    got = sim.rope_push(scene, push, params, f_max, device=DEV)
    for name, h, d in zip(("obj", "eef", "n_frames", "x", "v"), host, got):
        assert d.device.type == "cuda" and torch.equal(d.cpu(), torch.from_numpy(h)), name
    return host


@pytest.mark.parametrize("n", [2, 3, 5, 64, 65, 256])
def test_one_episode_equals_the_host_at_every_size_class(n):
    """n = 2: one stretch pair; 3: both passes; 5: clusters of 3; 64 / 65: the wave boundary; 256: the full workgroup.  Per n the cluster widths
    3, 16, n and n + 1 (skipped), where they differ and exist."""
    for w in sorted({3, min(16, n), n, n + 1}):
        scene = scene_of([n], [w], seed=n)
        obj, eef, n_frames, x, v = assert_same(scene, ACROSS(0.05 * (n // 2))[None])
        assert n_frames[0] == 5 and not np.array_equal(x, scene.x)      # 13 steps: frames after steps 0, 4, 8, 12 and the settle


def test_three_episodes_of_different_sizes_share_one_launch():
    """n = 5, 64, 37 and w = 3, 16, 37 under n_max = 64: the padding lanes of the smaller episodes; pushes of different lengths (13, 9 and 21 steps:
    4, 3 and 6 + 1 frames under one F_max)."""
    scene = scene_of([5, 64, 37], [3, 16, 37], kappas=[0.1, 0.6, 0.35])
    push = np.array([[0.1, -0.25, 0.1, 0.25], [1.6, -0.2, 1.6, 0.14], [0.9, -0.4, 0.95, 0.42]], F32)
    obj, eef, n_frames, x, v = assert_same(scene, push)
    assert list(n_frames) == [5, 4, 7] and not x[0, 5:].any() and not obj[0, :, 5:].any()
    assert_same(scene, push, f_max=9)      # more frames than any push writes: the rest stays zero


def test_a_push_that_misses_the_rope():
    scene = scene_of([40], [8])
    obj, eef, n_frames, x, v = assert_same(scene, np.array([[0.0, 1.0, 0.5, 1.0]], F32))
    assert np.abs(x - scene.x).max() < 0.05


def test_the_pusher_axis_passes_through_a_particle_exactly():
    """d == 0 at a substep, by construction: a straight rope at its rest spacing (spacing 1/16 along x, constant z: every stretch and ground
    operation of the first substep is exact and leaves x, z alone; no clusters) with particle 4 placed on the pusher's centre of substep 1."""
    n, m = 9, 4
    push = np.array([[0.25, -0.26, 0.25, 0.24]], F32)
    n_push, inv = sim.push_steps(push, SMALL)
    t = F32(1) * inv[0]
    c1 = np.array([push[0, 0] + (push[0, 2] - push[0, 0]) * t, push[0, 1] + (push[0, 3] - push[0, 1]) * t], F32)
    rope = np.stack([c1[0] + (np.arange(n) - m) / 16.0, np.full(n, SMALL.r), np.full(n, c1[1])], 1).astype(F32)
    assert rope[m, 0] == c1[0] and rope[m, 2] == c1[1] and np.all(np.diff(rope[:, 0]) == F32(1 / 16))
    scene = sim.RopeScene.from_ropes([rope], w=[0], kappa=[0.0])
    assert scene.l0[0] == F32(1 / 16)
    obj, eef, n_frames, x, v = assert_same(scene, push)
    assert np.isfinite(x).all() and np.isfinite(v).all()


def test_a_particle_lifted_above_the_ground():
    """`on` false for the first substeps: the lifted particles fall (and pull their neighbours up) while the pusher arrives."""
    scene = scene_of([33], [6])
    scene.x[0, 10:14, 1] += F32(0.05)
    scene.v[0, 20, 1] = F32(0.5)
    assert_same(scene, ACROSS(0.6)[None])


def test_default_parameters_one_push():
    """The shipped constants (8 substeps, a frame every 10 steps, 120 settle steps) on 48 particles: a short push, 21 steps."""
    scene = scene_of([48], [9])
    obj, eef, n_frames, x, v = assert_same(scene, np.array([[1.2, -0.1, 1.2, 0.1]], F32), sim.DEFAULT)
    assert n_frames[0] == 4


def test_two_calls_give_the_same_bits_and_a_graph_replays_them():
    scene = scene_of([65, 20], [16, 3])
    push = np.stack([ACROSS(1.6), ACROSS(0.5)])
    first = [t.clone() for t in sim.rope_push(scene, push, SMALL, device=DEV)]
    again = sim.rope_push(scene, push, SMALL, device=DEV)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    call = sim.DevicePush(scene, push, SMALL, device=DEV)
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
    for t in (call.obj, call.eef, call.n_frames, call.x, call.v):      # the replay restores x, v and rewrites every frame
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = (call.obj, call.eef, call.n_frames, call.x, call.v)
    assert all(torch.equal(a, b) for a, b in zip(first, got))


@pytest.mark.parametrize("what", ["n = 1", "n = 257", "F_max too small"])
def test_argument_errors_leave_the_outputs_untouched(what):
    n = {"n = 1": 1, "n = 257": 257}.get(what, 12)
    rope = np.stack([0.05 * np.arange(n), np.full(n, 0.03), np.zeros(n)], 1).astype(F32)
    scene = sim.RopeScene.from_ropes([rope], w=[3], kappa=[0.3])
    scene.l0[0] = F32(0.05)
    call = sim.DevicePush(scene, ACROSS(0.3)[None], SMALL, f_max=4 if what == "F_max too small" else None, device=DEV)      # the push writes 5
    outs = (call.obj, call.eef, call.n_frames, call.x, call.v)
    for t in outs:
        t.fill_(7)
    with pytest.raises(RuntimeError, match=r"ag_sim_rope_push failed \(-1\)"):
        call.launch()
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outs)


@pytest.mark.parametrize("bad_n", [1, 13])
def test_an_episode_outside_the_bounds_writes_no_frame_and_nothing_else(bad_n):
    """The per-episode n is a device array the library's host checks cannot see: under n_max = 12 an episode with n = 1 or 13 gets n_frames = 0
    and its outputs and state stay as they were, while its neighbour in the same launch is simulated as if alone.  rope_push refuses such
    a scene with rope_push_host's error before any launch."""
    good = wavy_rope(12, 5)
    scene = sim.RopeScene.from_ropes([good, good], w=[3, 4], kappa=[0.3, 0.3])
    scene.n[0] = bad_n
    push = np.stack([ACROSS(0.3), ACROSS(0.3)])
    for run in (lambda: sim.rope_push_host(scene, push, SMALL), lambda: sim.rope_push(scene, push, SMALL, device=DEV)):
        with pytest.raises(ValueError, match="n outside 2 .. 12"):
            run()
    call = sim.DevicePush(scene, push, SMALL, device=DEV)
    outs = (call.obj, call.eef, call.n_frames, call.x, call.v)
    for t in outs:
        t[0].fill_(7)
    call.launch()
    torch.cuda.synchronize()
    assert call.n_frames.tolist() == [0, 5] and all(bool((t[0] == 7).all()) for t in (call.obj, call.eef, call.x, call.v))
    alone = sim.rope_push_host(sim.RopeScene.from_ropes([good], w=[4], kappa=[0.3]), push[1:], SMALL)
    for name, h, d in zip(("obj", "eef", "n_frames", "x", "v"), alone, outs):
        assert torch.equal(d[1:].cpu(), torch.from_numpy(h)), name


def tree_bytes(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def test_dataset_on_the_device_equals_the_host_and_trains(tmp_path):
    """6 episodes x 2 pushes x 40 particles: device= writes the bytes device=None writes; train() runs 2 iterations on it with the batches assembled
    on the host and on the device, to a finite loss."""
    from adaptigraph_amd import train as agtrain
    host = datagen.generate_rope_dataset(str(tmp_path / "host"), 6, 2, seed=11, device=None, n_particles=40)
    dev = datagen.generate_rope_dataset(str(tmp_path / "dev"), 6, 2, seed=11, device=DEV, n_particles=40)
    files = tree_bytes(tmp_path / "dev")
    assert len(files) == 6 + 12 + 3 and files == tree_bytes(tmp_path / "host") and host["n_his"] == dev["n_his"]
    for device_batches in (False, True):
        ds = dict(dev, device=DEV, ratio={"train": [0, 0.67], "valid": [0.67, 1.0]}, verbose=False,
                  randomness={"use": True, "state_noise": {"train": 0.05, "valid": 0.0}, "phys_noise": {"train": 0.0, "valid": 0.0}},
                  datasets=[dict(name="rope", max_nobj=40, max_nR=800, fps_radius_range=[0.18, 0.22], adj_radius_range=[0.48, 0.52], topk=10,
                                 connect_tool_all=False)])
        cfg = {"dataset_config": ds, "material_config": configs.material_config("rope"), "model_config": configs.model_config(),
               "train_config": {"random_seed": 42, "out_dir": str(tmp_path / f"log{int(device_batches)}"), "phases": ["train", "valid"],
                                "num_workers": 0, "batch_size": 4, "n_epochs": 1, "log_interval": 1, "n_iters_per_epoch": {"train": 2, "valid": 1},
                                "device_batches": device_batches}}
        hist = agtrain.train(cfg)
        assert len(hist["train"]) == 1 and np.isfinite(hist["train"]).all() and np.isfinite(hist["valid"]).all()
