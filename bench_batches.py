"""The data side of training, host loader against device batches, measured in ONE run on one machine.

A synthetic rope dataset (adaptigraph_amd/synth.py clouds, written to a temporary directory in the reference's on-disk layout, see
adaptigraph_amd/load.py) is turned into collated, edge-attached training batches three ways; per configuration the script reports the
milliseconds per batch, median over warmed repetitions, host clock around `next(loader)` + `attach_edges` + a device synchronisation:
  host_ms         DataLoader(DynDataset, num_workers=0) + attach_edges                       (the loader train() uses by default)
  fps_device_ms   the same with DynDataset(fps_device=): the sampling of every item on the GPU, item by item
  device_ms       DataLoader over the sample numbers + DeviceBatcher.batch + attach_edges     (train_config['device_batches'])
and for the last one its parts: draw_ms (the host's random numbers for the batch), data_side_event_ms (HIP events around the upload of the
host tables, ag_gather_clouds, both sampling passes and ag_assemble_batch).  All loaders shuffle and drop the last partial batch, so every
timed batch is full.  Before anything is timed one device batch is checked against the collated host items under the same seed.
`train_step_ms` is bench_train.py's step time (its defaults: batch 128), measured by a child process of this run, so the ratio loader : step
is on record from one machine and one run.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import pickle
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
CONFIGS = [dict(points=2000, max_nobj=200, batch=128)]
ROTATED = ("state", "action", "eef_future", "action_future", "state_future")


def write_dataset(root, cfg, points, n_episodes=16, n_frames=22, seed=0):
    """n_episodes rope episodes of n_frames frames: a base cloud that drifts a little from frame to frame, one tool point that moves."""
    from adaptigraph_amd import synth
    ds = cfg["dataset_config"]
    H, Fu, name = ds["n_his"], ds["n_future"], ds["data_name"]
    rng = np.random.default_rng(seed)
    prep = os.path.join(root, "preprocess", name)
    os.makedirs(os.path.join(prep, "frame_pairs"))
    eef, obj = [], []
    for e in range(n_episodes):
        os.makedirs(os.path.join(root, "sim_data", name, f"{e:06}"))
        with open(os.path.join(root, "sim_data", name, f"{e:06}", "property_params.pkl"), "wb") as f:
            pickle.dump({"particle_radius": 0.03, "stiffness": float(rng.uniform(0.1, 0.9))}, f)
        base, tool = synth.rope_cloud(points, 0.01, rng)
        drift = np.cumsum(rng.normal(0.0, 0.002, (n_frames, points, 3)), 0).astype(np.float32)
        obj.append(base[None] + drift)
        eef.append((tool[None] + np.linspace(0, 0.3, n_frames)[:, None, None] * np.array([0.0, 0.0, -1.0])).astype(np.float32))
        pairs = np.stack([np.arange(s, s + H + Fu) for s in range(n_frames - H - Fu + 1)])
        np.savetxt(os.path.join(prep, "frame_pairs", f"{e:06}_01.txt"), pairs, fmt="%d")
    with open(os.path.join(prep, "positions.pkl"), "wb") as f:
        pickle.dump({"eef_pos": eef, "obj_pos": obj}, f)


def make_config(root, max_nobj, device):
    from adaptigraph_amd import configs
    ds = configs.dataset_config("rope")
    ds.update(data_dir=os.path.join(root, "sim_data"), prep_data_dir=os.path.join(root, "preprocess"), device=device, verbose=False,
              ratio={"train": [0, 1.0], "valid": [0, 1.0]},
              randomness={"use": True, "state_noise": {"train": 0.05, "valid": 0.0}, "phys_noise": {"train": 0.0, "valid": 0.0}},
              datasets=[dict(name="rope", max_nobj=max_nobj, max_nR=4000, fps_radius_range=[0.18, 0.22], adj_radius_range=[0.48, 0.52], topk=10,
                             connect_tool_all=False)])
    mat = configs.material_config("rope")
    mat["rope"]["physics_params"][1].update(min=0.0, max=1.0)
    return {"dataset_config": ds, "material_config": mat}


def timed_batches(torch, next_batch, reps, warmup):
    ts = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        next_batch()
        torch.cuda.synchronize()
        if r >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def cycle(loader):
    while True:
        for batch in loader:
            yield batch


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20, help="timed batches per path (the median is reported)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batches_bench.txt"))
    args = ap.parse_args()
    import torch
    from torch.utils.data import DataLoader, default_collate
    from adaptigraph_amd.dataset import DeviceBatcher, DynDataset, attach_edges
    assert torch.cuda.is_available(), "bench_batches.py measures the GPU path: it needs an MI355X (no fallback)"
    dev = args.device
    rows = []
    for c in CONFIGS:
        with tempfile.TemporaryDirectory() as root:
            cfg = make_config(root, c["max_nobj"], dev)
            write_dataset(root, cfg, c["points"])
            dsc, B = cfg["dataset_config"], c["batch"]
            make = lambda **kw: DynDataset(dsc, cfg["material_config"], phase="train", **kw)
            host_ds, fps_ds, dev_ds = make(), make(fps_device=dev), make()
            batcher = DeviceBatcher(dev_ds, dev)

            # one device batch against the collated host items, same seed
            check = list(range(0, len(host_ds), max(1, len(host_ds) // 16)))[:16]
            np.random.seed(3)
            check_ds = make()
            want = default_collate([check_ds[i] for i in check])
            np.random.seed(3)
            got = batcher.batch(check)
            assert list(got) == list(want)
            for k in want:
                if k not in ROTATED:
                    assert torch.equal(got[k].cpu(), want[k]), k
            rotated_equal = all(torch.equal(got[k].cpu(), want[k]) for k in ROTATED)

            loader = lambda ds: cycle(DataLoader(ds, batch_size=B, shuffle=True, num_workers=0, drop_last=True))
            it_host, it_fps, it_idx = loader(host_ds), loader(fps_ds), loader(list(range(len(dev_ds))))
            torch.manual_seed(0)
            np.random.seed(0)
            data = attach_edges(batcher.batch(next(it_idx).tolist()), dsc, dev)
            n_kp, n_edges = data["obj_mask"].sum(1).float().mean().item(), int(data["Rr"].row_ptr[-1])
            device_ms = timed_batches(torch, lambda: attach_edges(batcher.batch(next(it_idx).tolist()), dsc, dev), args.reps, args.warmup)
            fps_device_ms = timed_batches(torch, lambda: attach_edges(next(it_fps), dsc, dev), args.reps, args.warmup)
            host_ms = timed_batches(torch, lambda: attach_edges(next(it_host), dsc, dev), args.reps, 1)

            draw, events = [], []
            for r in range(args.warmup + args.reps):
                idx = next(it_idx).tolist()
                t0 = time.perf_counter()
                t = batcher.draw(idx)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                batcher.assemble(batcher.upload(t), int(t["n"].max()), int(t["k1"].max()))
                e1.record()
                e1.synchronize()
                if r >= args.warmup:
                    draw.append((t1 - t0) * 1e3)
                    events.append(e0.elapsed_time(e1))
            rows.append(dict(c, samples=len(host_ds), n_his=dsc["n_his"], n_future=dsc["n_future"], key_points_mean=round(n_kp, 1),
                             edges_per_batch=n_edges, rotated_keys_bit_equal=rotated_equal,
                             host_ms=round(host_ms, 3), fps_device_ms=round(fps_device_ms, 3), device_ms=round(device_ms, 3),
                             draw_ms=round(statistics.median(draw), 3), data_side_event_ms=round(statistics.median(events), 3),
                             store_bytes=batcher.store_bytes))
    step = subprocess.run([sys.executable, os.path.join(ROOT, "bench_train.py"), "--steps", "20", "--warmup", "5"], capture_output=True, text=True,
                          timeout=300)
    assert step.returncode == 0, step.stderr[-2000:]
    train_step = json.loads(step.stdout.strip().splitlines()[-1])
    line = json.dumps(dict(bench="batches", device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, configs=rows,
                           train_step_ms=train_step["value"], train_step_workload=train_step["config"]["workload"]))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
