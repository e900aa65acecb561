"""The preprocess step (adaptigraph_amd/preprocess.py) against results of the reference's own functions (tests/golden/preprocess_pairs.npz, made
by tools/gen_preprocess_golden.py), and the rope dataset writer (adaptigraph_amd/datagen.py) on the host restatement of the simulator: what it
writes is what load.py and DynDataset read."""
import os

import numpy as np
import pytest

from conftest import load_golden
from adaptigraph_amd import configs, datagen, load, preprocess


def cases(g, prefix, first):
    i = 0
    while f"{prefix}_{i}_{first}" in g:
        yield i
        i += 1


def test_extract_push_equals_the_reference():
    g = load_golden("preprocess_pairs")
    seen = list(cases(g, "push", "eef"))
    assert len(seen) >= 12
    lengths = set()
    for i in seen:
        eef, (thresh, n_his, n_future, n_frames) = g[f"push_{i}_eef"], g[f"push_{i}_args"]
        pairs, cnt = preprocess.extract_push(eef, float(thresh), int(n_his), int(n_future), int(n_frames))
        want = g[f"push_{i}_pairs"]
        assert np.array_equal(pairs, want) and pairs.shape == want.shape and pairs.dtype == want.dtype, i
        assert cnt == int(g[f"push_{i}_cnt"]) == len(eef), i
        lengths.add(len(eef))
    assert {1, 2, 3, 60} <= lengths      # one frame, shorter than n_his, the longest path


def test_process_eef_equals_the_reference():
    g = load_golden("preprocess_pairs")
    seen = list(cases(g, "eef", "states"))
    assert len(seen) >= 6
    for i in seen:
        pos = g[f"eef_{i}_pos"]
        out = preprocess.process_eef(g[f"eef_{i}_states"], {"pos": pos.tolist(), "max_neef": len(pos)})
        want = g[f"eef_{i}_out"]
        assert np.array_equal(out, want) and out.shape == want.shape and out.dtype == want.dtype, i
    with pytest.raises(AssertionError):
        preprocess.process_eef(g["eef_0_states"], {"pos": [[0.0, 0.0, 1.0]], "max_neef": 2})


def tree_bytes(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def dataset_configs(ds):
    ds = dict(ds, ratio={"train": [0, 0.75], "valid": [0.75, 1.0]}, verbose=False,
              randomness={"use": True, "state_noise": {"train": 0.05, "valid": 0.0}, "phys_noise": {"train": 0.0, "valid": 0.0}},
              datasets=[dict(name="rope", max_nobj=24, max_nR=400, fps_radius_range=[0.18, 0.22], adj_radius_range=[0.48, 0.52], topk=10,
                             connect_tool_all=False)])
    return ds, configs.material_config("rope")


def test_host_dataset_is_read_back_by_the_loaders(tmp_path):
    """4 episodes x 2 pushes of 24 particles with device=None: the files load, every frame index lies inside its episode, DynDataset builds an
    item, and a second run with the same seed writes identical bytes."""
    E, K, n = 4, 2, 24
    ds = datagen.generate_rope_dataset(str(tmp_path / "a"), E, K, seed=7, device=None, n_particles=n)
    ds, mat = dataset_configs(ds)
    files = tree_bytes(tmp_path / "a")
    assert sorted(files) == sorted([f"sim_data/rope/{e:06}/property_params.pkl" for e in range(E)]
                                   + [f"preprocess/rope/frame_pairs/{e:06}_{k:02}.txt" for e in range(E) for k in range(1, K + 1)]
                                   + [f"preprocess/rope/{f}" for f in ("positions.pkl", "phys_range.txt", "metadata.txt")])
    assert files["preprocess/rope/metadata.txt"] == b"0.095,3,4"
    # the tuples step from one recorded frame to the next: a row with three push frames before it and three after it holds seven consecutive
    # frames (the push's last frame, after the settle, is left out: its pusher point is wherever the push ended)
    first = {e: 0 for e in range(E)}
    for e in range(E):
        for k in range(1, K + 1):
            rows = np.loadtxt(tmp_path / "a" / "preprocess" / "rope" / "frame_pairs" / f"{e:06}_{k:02}.txt", dtype=np.int64)
            mid = range(3, len(rows) - 1 - 3)
            assert len(rows) >= 10 and len(mid) >= 3      # pushes are 0.8 .. 1.6 long: 9 .. 17 push frames and the last one
            for f in mid:
                assert list(rows[f]) == list(range(first[e] + f - 3, first[e] + f + 4)), (e, k, f, rows[f])
            first[e] += len(rows)
    eef, obj = load.load_positions(ds)
    assert len(eef) == len(obj) == E
    T = [len(o) for o in obj]
    assert all(o.shape == (t, n, 3) and p.shape == (t, 1, 3) and o.dtype == p.dtype == np.float32 for o, p, t in zip(obj, eef, T))
    n_rows = 0
    for phase, lo, hi in (("train", 0, 3), ("valid", 3, 4)):
        pairs, phys = load.load_dataset(ds, mat, phase)
        assert len(phys) == E and all(0.0 <= float(p["rope"][0]) <= 1.0 for p in phys)
        assert pairs.shape[1] == 1 + ds["n_his"] + ds["n_future"] and set(pairs[:, 0]) == set(range(lo, hi))
        for row in pairs:
            assert 0 <= row[1:].min() and row[1:].max() < T[row[0]]
        n_rows += len(pairs)
    assert n_rows == sum(T)      # one row per recorded frame
    lo, hi = np.loadtxt(tmp_path / "a" / "preprocess" / "rope" / "phys_range.txt")
    assert 0.0 <= lo < hi <= 1.0
    from adaptigraph_amd.dataset import DynDataset
    np.random.seed(0)
    item = DynDataset(ds, mat, phase="train")[0]
    assert item["state"].shape[0] == ds["n_his"] and bool(np.isfinite(item["state"].numpy()).all()) and int(item["obj_mask"].sum()) >= 2
    datagen.generate_rope_dataset(str(tmp_path / "b"), E, K, seed=7, device=None, n_particles=n)
    assert tree_bytes(tmp_path / "b") == files
