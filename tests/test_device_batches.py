"""Training batches assembled on the GPU (`DeviceBatcher`, adaptigraph_amd/dataset.py; `ag_gather_clouds` / `ag_assemble_batch`, csrc/ag_batch.hip)
against the host loader `default_collate([DynDataset[i] ...])` under the same numpy seed, and against the reference's own items.

Equality is exact (torch.equal) for everything that is not rotated.  The rotated tensors are compared as follows (`check_rotated`): the test restates
the host's `a @ rot` as the fused chain the kernel computes, fmaf(a2, r2j, fmaf(a1, r1j, a0 * r0j)) (products exact in float64, one rounding per
step), on the host's own pre-rotation values.  Where that restatement equals what the host returned, the device result must be torch.equal to the
host.  Where it does not (a numpy whose fp32 matmul rounds differently), the bound is derived, not measured: two correctly ordered evaluations of a
three-term fp32 dot product differ by at most 6 * 2^-24 * sum_i |a_i r_ij|.  The branch taken is printed per key."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch
from torch.utils.data import default_collate

from conftest import load_golden
from adaptigraph_amd import _lib, sampling
from adaptigraph_amd.dataset import DeviceBatcher, DynDataset, attach_edges, draw_batch_tables
from test_eval_rollout import write_dataset
from test_train import KEYS, train_config

DEV = "cuda:0"
ROTATED = ["state", "action", "eef_future", "action_future", "state_future"]
ENTRY_POINTS = ("ag_gather_clouds", "ag_assemble_batch")


def golden_config(root, use=True, radius_range=None, phys_noise=0.0, device="cpu"):
    g_eval = load_golden("evalrollout_rope")
    if not os.path.exists(os.path.join(root, "preprocess")):
        write_dataset(root, g_eval)
    cfg = train_config(root, g_eval, device)
    cfg["dataset_config"]["randomness"]["use"] = use
    cfg["dataset_config"]["randomness"]["phys_noise"]["train"] = phys_noise
    if radius_range is not None:
        cfg["dataset_config"]["datasets"][0]["fps_radius_range"] = radius_range
    return cfg


def new_dataset(cfg, phase="train"):
    """A fresh DynDataset: the physics noise accumulates in the dataset, so every run that is compared with another gets its own."""
    return DynDataset(cfg["dataset_config"], cfg["material_config"], phase=phase)


# ------------------------------------------------------------------------------------------------------ CPU
def test_batch_entry_points_are_exported():
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "adaptigraph_hip.h")).read()
    for name in ENTRY_POINTS:
        assert name in _lib.EXPORTS and hasattr(L, name) and f"int {name}(" in header
    assert "src/dynamics/dataset/dataset.py:10-252" in header
    assert [n for n, _ in _lib.BatchDims._fields_] == ["B", "H", "Fu", "no", "n_eef", "K", "n_mat", "mat_col", "n_episodes", "tool_f64"]
    for n, _ in _lib.BatchDims._fields_ + _lib.BatchOut._fields_:
        assert n in header


def test_batch_entry_points_reject_bad_arguments_without_a_gpu():
    L = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    good = dict(store=p, episodes=p, E=1, epi=p, frame=p, B=2, Nmax=10, pts=p, count=p)

    def gather(**kw):
        a = dict(good, **kw)
        return L.ag_gather_clouds(a["store"], a["episodes"], a["E"], a["epi"], a["frame"], a["B"], a["Nmax"], a["pts"], a["count"], None)

    for bad, word in ((dict(store=None), b"obj_store"), (dict(episodes=None), b"episodes"), (dict(epi=None), b"epi"), (dict(frame=None), b"frame"),
                      (dict(pts=None), b"pts"), (dict(count=None), b"count"), (dict(B=0), b"B=0"), (dict(Nmax=0), b"Nmax=0"),
                      (dict(E=0), b"n_episodes=0")):
        assert gather(**bad) == -1, bad                      # AG_ERR_ARG
        assert word in L.ag_last_error(), (bad, L.ag_last_error())

    dims0 = dict(B=2, H=4, Fu=3, no=5, n_eef=1, K=5, n_mat=4, mat_col=1, n_episodes=1, tool_f64=0)
    ptrs0 = dict(obj=p, tool=p, episodes=p, epi=p, frames=p, picks=p, noise=p, rot=p)
    out0 = {n: p for n, _ in _lib.BatchOut._fields_}

    def assemble(dims=None, out=None, **kw):
        a = dict(ptrs0, **kw)
        d = _lib.BatchDims(**dict(dims0, **(dims or {})))
        o = _lib.BatchOut(**dict(out0, **(out or {})))
        return L.ag_assemble_batch(ctypes.byref(d), a["obj"], a["tool"], a["episodes"], a["epi"], a["frames"], a["picks"], a["noise"], a["rot"],
                                   ctypes.byref(o), None)

    cases = [(dict(dims=dict(B=0)), b"B=0"), (dict(dims=dict(H=0)), b"H=0"), (dict(dims=dict(Fu=0)), b"Fu=0"), (dict(dims=dict(K=0)), b"K=0"),
             (dict(dims=dict(no=0)), b"no=0"), (dict(dims=dict(n_eef=0)), b"n_eef=0"), (dict(dims=dict(n_episodes=0)), b"n_episodes=0"),
             (dict(dims=dict(mat_col=4)), b"mat_col=4"), (dict(dims=dict(n_mat=0)), b"mat_col"),
             (dict(noise=None), b"noise is null"), (dict(rot=None), b"rot is null"),
             (dict(obj=None), b"obj_store"), (dict(tool=None), b"tool_store"), (dict(episodes=None), b"episodes"), (dict(epi=None), b"epi"),
             (dict(frames=None), b"frames"), (dict(picks=None), b"picks")]
    cases += [(dict(out={n: None}), ("out." + n).encode()) for n, _ in _lib.BatchOut._fields_]
    for bad, word in cases:
        assert assemble(**bad) == -1, bad
        assert word in L.ag_last_error(), (bad, L.ag_last_error())
    o = _lib.BatchOut(**out0)
    assert L.ag_assemble_batch(None, p, p, p, p, p, p, None, None, ctypes.byref(o), None) == -1 and b"dims" in L.ag_last_error()
    d = _lib.BatchDims(**dims0)
    assert L.ag_assemble_batch(ctypes.byref(d), p, p, p, p, p, p, None, None, None, None) == -1 and b"out is null" in L.ag_last_error()


def same_rng_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("radius_range", [0.2, [0.18, 0.22]])
@pytest.mark.parametrize("use", [True, False])
def test_draw_batch_tables_draws_the_rng_like_the_items(tmp_path, use, radius_range):
    """The host tables of a batch leave np.random exactly where the items leave it, with the same adjacency radii, the same accumulated
    physics parameters (noise switched on here) and — the fps draws being the first of every item — the same sampling starts."""
    cfg = golden_config(str(tmp_path), use, radius_range, phys_noise=0.01)
    indices = [5, 40, 5, 17, 0, 47]                               # both episodes of the split, one index twice
    a, b = new_dataset(cfg), new_dataset(cfg)
    np.random.seed(11)
    items = [a[i] for i in indices]
    state_items = np.random.get_state()
    np.random.seed(11)
    t = draw_batch_tables(b, indices)
    assert same_rng_state(state_items, np.random.get_state())
    assert np.array_equal(t["adj_thresh"], np.array([float(it["adj_thresh"]) for it in items])) and t["adj_thresh"].dtype == np.float64
    # (the items' physics parameters are views of the dataset's arrays: collated after the loop, every item shows its episode's final value)
    assert np.array_equal(t["phys_rope"], default_collate(items)["rope_physics_param"].numpy()) and t["phys_rope"].dtype == np.float32
    fresh = new_dataset(cfg).physics_params
    assert all(t["phys_rope"][k] != fresh[t["epi"][k]]["rope"] for k in range(6))      # the noise accumulated
    for e in range(len(a.physics_params)):
        assert np.array_equal(a.physics_params[e]["rope"], b.physics_params[e]["rope"])
    assert ("noise" in t) == use and ("rot" in t) == use
    assert np.array_equal(t["epi"], a.pair_lists[indices, 0]) and np.array_equal(t["frames"], a.pair_lists[indices, 1:])
    assert np.array_equal(t["fps_frame"], t["frames"][:, a.n_his - 1]) and (t["n"] == 120).all() and (t["k1"] == a.max_nobj).all()
    if use:
        assert t["noise"].shape == (6, a.n_his, a.state_dim, 3) and t["noise"].dtype == np.float64 and np.abs(t["noise"]).max() <= 0.05
        assert t["rot"].dtype == np.float32 and np.array_equal(t["rot"][:, 2], np.tile(np.float32([0, 0, 1]), (6, 1)))


def test_oversized_stores_raise_before_any_gpu_work(tmp_path):
    ds = new_dataset(golden_config(str(tmp_path)))
    need = 3 * 24 * 120 * 3 * 4 + 3 * 24 * 1 * 3 * 4 + 3 * 4 * 8
    with pytest.raises(ValueError, match=f"need {need} bytes"):
        DeviceBatcher(ds, DEV, max_bytes=need - 1)


# ------------------------------------------------------------------------------------------------------ GPU
def fused_rotation(a, r):
    """a (..., 3) fp32 @ r (3, 3) fp32 as fmaf(a2, r2j, fmaf(a1, r1j, a0 * r0j)): every product exact in float64, one rounding per step."""
    a64, r64 = a.astype(np.float64), r.astype(np.float64)
    acc = (a64[..., 0:1] * r64[0]).astype(np.float32)
    for i in (1, 2):
        acc = (a64[..., i:i + 1] * r64[i] + acc.astype(np.float64)).astype(np.float32)
    return acc


def host_items(cfg, indices, seed, monkeypatch):
    """-> (items, the same items with the rotation replaced by the identity, the rotation matrices): the second run draws the same numbers, but
    its angle is 0, so its tensors are the pre-rotation values (a @ identity is a, up to the sign of a zero)."""
    ds = new_dataset(cfg)
    np.random.seed(seed)
    items = [ds[int(i)] for i in indices]
    if not cfg["dataset_config"]["randomness"]["use"]:
        return items, None, None
    angles, real = [], np.random.uniform

    def uniform(low=0.0, high=1.0, size=None):
        v = real(low, high, size)
        if size is None and low == -np.pi:
            angles.append(v)
            return 0.0
        return v

    ds = new_dataset(cfg)
    with monkeypatch.context() as m:
        m.setattr(np.random, "uniform", uniform)
        np.random.seed(seed)
        plain = [ds[int(i)] for i in indices]
    rots = [np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=np.float32) for a in angles]
    assert len(rots) == len(indices)
    return items, plain, rots


def check_rotated(key, want, plain, rots, got, where):
    """want / plain: per-item host arrays after / before the rotation; got: the device tensor (B, ...).  See the module docstring."""
    want_all = np.stack(want)
    got = got.cpu().numpy()
    assert got.shape == want_all.shape and got.dtype == want_all.dtype, (key, where)
    if got.size == 0:
        return
    restated = np.stack([fused_rotation(p, r) for p, r in zip(plain, rots)])
    if np.array_equal(restated, want_all):
        print(f"[{where}] {key}: the host matmul is the fused chain -> exact comparison")
        assert np.array_equal(got, want_all), (key, where, np.abs(got - want_all).max())
    else:
        bound = np.stack([6 * 2.0 ** -24 * (np.abs(p.astype(np.float64))[..., :, None] * np.abs(r.astype(np.float64))[None]).sum(-2)
                          for p, r in zip(plain, rots)])
        diff = np.abs(got.astype(np.float64) - want_all.astype(np.float64))
        print(f"[{where}] {key}: the host matmul is NOT the fused chain -> derived bound; largest diff / bound = "
              f"{(diff / np.maximum(bound, 1e-300)).max():.3f}")
        assert (diff <= bound).all(), (key, where, float((diff - bound).max()))


def compare_with_host(cfg, indices, seed, monkeypatch, where, batcher_dataset=None):
    """One batch on the device against the collated host items under the same seed.  -> (host batch, device batch)."""
    use = cfg["dataset_config"]["randomness"]["use"]
    items, plain, rots = host_items(cfg, indices, seed, monkeypatch)
    host = default_collate(items)
    state_host = np.random.get_state() if not use else None
    batcher = DeviceBatcher(batcher_dataset if batcher_dataset is not None else new_dataset(cfg), DEV)
    np.random.seed(seed)
    dev = batcher.batch(indices)
    if not use:
        assert same_rng_state(state_host, np.random.get_state())
    assert list(dev.keys()) == list(host.keys())
    for k in host:
        assert dev[k].shape == host[k].shape and dev[k].dtype == host[k].dtype, (k, where, dev[k].shape, host[k].shape)
        assert dev[k].is_cuda == (k != "adj_thresh"), k
        if use and k in ROTATED:
            check_rotated(k, [it[k].numpy() for it in items], [it[k].numpy() for it in plain], rots, dev[k], where)
        else:
            assert torch.equal(dev[k].cpu(), host[k]), (k, where)
    return host, dev


INDEX_LISTS = {"golden": None, "repeated": [3, 9, 3, 3, 21], "two_episodes": [0, 47, 23, 24, 1, 46], "single": [30]}


@pytest.mark.gpu
@pytest.mark.parametrize("use", [False, True])
@pytest.mark.parametrize("name", list(INDEX_LISTS))
def test_batches_match_the_host_item_for_item(tmp_path, monkeypatch, name, use):
    """randomness off: every key torch.equal.  On: every key that is not rotated torch.equal — obj_mask and attrs pin the number of picks — and
    the rotated ones as `check_rotated` says, which pins the picks themselves (another pick is another point, far outside any rounding)."""
    cfg = golden_config(str(tmp_path), use, phys_noise=0.01 if name == "repeated" else 0.0)
    indices = INDEX_LISTS[name] or [int(i) for i in load_golden("train_rope")["idx"]]
    host, dev = compare_with_host(cfg, indices, 123, monkeypatch, f"{name}/use={use}")
    if name == "two_episodes":
        ds = new_dataset(cfg)
        assert len(set(ds.pair_lists[indices, 0])) == 2
    n_kp = host["obj_mask"].sum(1)
    assert (n_kp >= 1).all() and (n_kp < host["obj_mask"].shape[1]).any()       # some rows are padding
    if not use:
        pad = ~dev["obj_mask"]
        assert (dev["state"][:, :, :pad.shape[1]][pad[:, None].expand(-1, dev["state"].shape[1], -1)] == 0).all()


@pytest.mark.gpu
def test_batches_match_the_reference_items(tmp_path, monkeypatch):
    """The reference's own items (train_rope.npz: `idx` under seed + k), one sample per batch: the unrotated KEYS exactly, the rotated ones by the
    rule of `check_rotated` with the reference's values in the host's place (the host path equals them exactly:
    test_train.py::test_dataset_samples_match_reference)."""
    g = load_golden("train_rope")
    cfg = golden_config(str(tmp_path), True)
    batcher = DeviceBatcher(new_dataset(cfg), DEV)
    for k, i in enumerate(g["idx"]):
        seed = int(g["seed"]) + k
        items, plain, rots = host_items(cfg, [int(i)], seed, monkeypatch)
        np.random.seed(seed)
        dev = batcher.batch([int(i)])
        for key in KEYS:
            want = g["b_" + key][k]
            assert np.array_equal(items[0][key].numpy(), want), (key, k)
            if key in ROTATED:
                check_rotated(key, [want], [plain[0][key].numpy()], rots, dev[key], f"reference item {k}")
            else:
                assert np.array_equal(dev[key][0].cpu().numpy(), want), (key, k)


def write_synthetic(root, n_points, n_eef, tool_dtype, obj_dtype, H, Fu, T=10):
    """A dataset in the reference's layout (adaptigraph_amd/load.py) with one episode per entry of n_points."""
    rng = np.random.default_rng(1234)
    cfg = train_config(root, load_golden("evalrollout_rope"))          # the rope configuration; paths and sizes replaced below
    ds = cfg["dataset_config"]
    ds.update(data_dir=os.path.join(root, "sim_data"), prep_data_dir=os.path.join(root, "preprocess"), n_his=H, n_future=Fu,
              ratio={"train": [0, 1.0], "valid": [0, 1.0]})
    ds["datasets"][0].update(max_nobj=200, max_nR=4000, fps_radius_range=[0.05, 0.08], adj_radius_range=[0.1, 0.12])
    prep = os.path.join(root, "preprocess", ds["data_name"])
    os.makedirs(os.path.join(prep, "frame_pairs"))
    eef, obj = [], []
    for e, n in enumerate(n_points):
        os.makedirs(os.path.join(root, "sim_data", ds["data_name"], f"{e:06}"))
        with open(os.path.join(root, "sim_data", ds["data_name"], f"{e:06}", "property_params.pkl"), "wb") as f:
            pickle.dump({"particle_radius": 0.03, "stiffness": 0.2 + 0.1 * e}, f)
        base = rng.uniform(-0.5, 0.5, (1, n, 3))
        obj.append((base + 0.01 * rng.standard_normal((T, n, 3))).astype(obj_dtype))
        eef.append(rng.uniform(-0.5, 0.5, (T, n_eef, 3)).astype(tool_dtype))
        pairs = np.stack([np.arange(s, s + H + Fu) for s in range(T - H - Fu + 1)] + [np.arange(T - 1, T - 1 - H - Fu, -1)])
        np.savetxt(os.path.join(prep, "frame_pairs", f"{e:06}_01.txt"), pairs, fmt="%d")
    with open(os.path.join(prep, "positions.pkl"), "wb") as f:
        pickle.dump({"eef_pos": eef, "obj_pos": obj}, f)
    return cfg


SHAPES = {"ragged_small_and_streaming": dict(n_points=(300, 150, sampling.FPS_RESIDENT_POINTS + 808), n_eef=1, tool_dtype=np.float32,
                                             obj_dtype=np.float32, H=4, Fu=3),
          "float64_two_tools": dict(n_points=(260, 120), n_eef=2, tool_dtype=np.float64, obj_dtype=np.float64, H=4, Fu=3),
          "n_future_1": dict(n_points=(230, 64), n_eef=1, tool_dtype=np.float32, obj_dtype=np.float32, H=4, Fu=1),
          "n_his_1_float64_tool": dict(n_points=(210, 1), n_eef=1, tool_dtype=np.float64, obj_dtype=np.float32, H=1, Fu=2)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_ragged_and_edge_shapes_match_the_host(tmp_path, monkeypatch, name):
    """Episodes with different point counts, a cloud smaller than max_nobj, a cloud beyond AG_FPS_RESIDENT_POINTS (streaming ag_fps), float64
    tool positions (differences taken in float64, rounded afterwards: checked to matter below), n_future 1 (empty eef_future), two tool points,
    n_his 1, a one-point cloud.  Each with and without randomness, all samples of the dataset in one batch plus a batch of the small ones."""
    shape = SHAPES[name]
    cfg = write_synthetic(str(tmp_path), **shape)
    n_samples = len(new_dataset(cfg))
    everything = list(range(n_samples))
    per_epi = n_samples // len(shape["n_points"])
    for use in (False, True):
        cfg["dataset_config"]["randomness"]["use"] = use
        host, dev = compare_with_host(cfg, everything, 5, monkeypatch, f"{name}/all/use={use}")
        compare_with_host(cfg, everything[per_epi:2 * per_epi][::-1], 6, monkeypatch, f"{name}/second episode/use={use}")
        assert dev["eef_future"].shape[1] == shape["Fu"] - 1 and dev["eef_mask"].sum(1).tolist() == [shape["n_eef"]] * n_samples
        counts = host["obj_mask"].sum(1)
        for e, n in enumerate(shape["n_points"]):
            if n < 200:
                assert (counts[e * per_epi:(e + 1) * per_epi] <= n).all()
    if shape["tool_dtype"] == np.float64:
        ds = new_dataset(cfg)
        e64 = np.asarray(ds.eef_pos[0])
        assert not np.array_equal((e64[1:] - e64[:-1]).astype(np.float32), e64[1:].astype(np.float32) - e64[:-1].astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("use", [False, True])
def test_attach_edges_on_a_device_batch(tmp_path, monkeypatch, use):
    """Same row_ptr / receiver / sender arrays as on the collated host batch.  With randomness the comparison needs equal `state` tensors: where
    the host matmul is not the fused chain (see check_rotated) the edge sets may differ by rounding, and the test says so instead."""
    cfg = golden_config(str(tmp_path), use, device=DEV)
    indices = [0, 47, 23, 24, 1, 46, 12, 12]
    host, dev = compare_with_host(cfg, indices, 77, monkeypatch, f"edges/use={use}")
    if not torch.equal(dev["state"].cpu(), host["state"]):
        print("state differs from the host within the derived bound: edge comparison not applicable")
        return
    a = attach_edges(host, cfg["dataset_config"], DEV)
    b = attach_edges(dev, cfg["dataset_config"], DEV)
    assert set(a) == set(b) and "adj_thresh" not in b
    assert torch.equal(a["Rr"].row_ptr, b["Rr"].row_ptr) and int(a["Rr"].row_ptr[-1]) > 0
    n = int(a["Rr"].row_ptr[-1])
    assert torch.equal(a["Rr"].edge_recv[:n], b["Rr"].edge_recv[:n]) and torch.equal(a["Rr"].edge_send[:n], b["Rr"].edge_send[:n])
    assert b["edge_views"] is not None and b["Rs"] is None


@pytest.mark.gpu
def test_device_work_is_capture_safe(tmp_path, monkeypatch):
    """ag_gather_clouds + both sampling passes + ag_assemble_batch captured into a HIP graph once, replayed three times on new host tables: a host
    synchronisation inside would have failed the capture, and every replay equals the host."""
    cfg = golden_config(str(tmp_path), True)
    batcher = DeviceBatcher(new_dataset(cfg), DEV)
    lists = [[1, 2, 3, 40], [7, 7, 30, 45], [47, 0, 22, 25], [13, 14, 15, 16]]
    np.random.seed(900)
    t = batcher.draw(lists[0])
    n_max, K = int(t["n"].max()), int(t["k1"].max())
    static = {k: v.clone() for k, v in batcher.upload(t).items()}
    batcher.assemble(static, n_max, K)                       # warm-up outside the capture
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = batcher.assemble(static, n_max, K)
    for r, indices in enumerate(lists[1:]):
        seed = 901 + r
        items, plain, rots = host_items(cfg, indices, seed, monkeypatch)
        np.random.seed(seed)
        t = batcher.draw(indices)
        assert int(t["n"].max()) == n_max and int(t["k1"].max()) == K
        for k, v in batcher.upload(t).items():
            static[k].copy_(v)
        for v in out.values():
            if v is not static.get("phys_rope"):
                v.zero_()
        gr.replay()
        torch.cuda.synchronize()
        host = default_collate(items)
        for k in host:
            if k == "adj_thresh":
                assert np.array_equal(t["adj_thresh"], host[k].numpy())
            elif k in ROTATED:
                check_rotated(k, [it[k].numpy() for it in items], [it[k].numpy() for it in plain], rots, out[k], f"replay {r}")
            else:
                assert torch.equal(out[k].cpu(), host[k]), (k, r)


@pytest.mark.gpu
def test_train_with_device_batches(tmp_path):
    """train() with device_batches: finite histories of the host path's lengths.  Without randomness the batches are bit-equal to the host's, so
    if the host path repeats itself exactly (the training kernels are documented as bit-reproducible) the device-batch history must equal it
    exactly; if it does not, the device path may differ from a host run by at most the larger host-vs-host difference."""
    from adaptigraph_amd import train as agtrain

    def run(sub, use, device_batches):
        root = os.path.join(str(tmp_path), sub)
        os.makedirs(root)
        cfg = golden_config(root, use, device=DEV)
        cfg["train_config"]["device_batches"] = device_batches
        return agtrain.train(cfg)

    h1, h2, d = run("h1", False, False), run("h2", False, False), run("d", False, True)
    for hist in (h1, h2, d):
        assert len(hist["train"]) == 2 and len(hist["valid"]) == 2 and np.isfinite(hist["train"]).all() and np.isfinite(hist["valid"]).all()
    host_gap = max(abs(a - b) for ph in h1 for a, b in zip(h1[ph], h2[ph]))
    dev_gap = max(abs(a - b) for ph in h1 for a, b in zip(h1[ph], d[ph]))
    print(f"host vs host: {host_gap:.3e}; host vs device batches: {dev_gap:.3e}")
    if host_gap == 0.0:
        assert d == h1
    else:
        print("the host path does not repeat itself exactly on this machine")
        assert dev_gap <= host_gap
    r = run("r", True, True)
    hr = run("hr", True, False)
    assert [len(r[ph]) for ph in ("train", "valid")] == [len(hr[ph]) for ph in ("train", "valid")] == [2, 2]
    assert np.isfinite(r["train"]).all() and np.isfinite(r["valid"]).all()
    ds = new_dataset(golden_config(os.path.join(str(tmp_path), "h1"), True))
    with pytest.raises(ValueError, match="bytes"):
        DeviceBatcher(ds, DEV, max_bytes=1000)
