"""Key-point sampling (`sampling.fps`) on the host against the GPU path (`ag_fps`), measured in ONE run on one machine.

Per shape (uniform random cloud in the unit cube, fps_radius_range [0.18, 0.22]) it reports, as medians over warmed repetitions:
  host_ms    `sampling.fps(cloud, max_nobj, range)` — the numpy code, this machine's CPU
  device_ms  `sampling.fps(..., device=)` end to end: upload, both passes, the copy back, host clock around a call that ends in that copy
  kernel_ms  the device work alone (pass 1, gather, pass 2, index composition) between two HIP events
and the same for `fps_batch` over 64 clouds of 2 000 points against the loop of 64 host calls.  Every device result is checked against the
host result under the same seed before anything is timed.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import time

import numpy as np

SHAPES = [(2000, 200), (5000, 200), (20000, 200), (4096, 1000)]      # (cloud points, max_nobj)
RANGE = [0.18, 0.22]


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def kernel_ms(torch, sampling, clouds, max_nobj, dev, reps, warmup):
    n = [len(c) for c in clouds]
    k1 = [min(max_nobj, m) for m in n]
    host = np.zeros((len(clouds), max(n), 3), np.float32)
    for b, c in enumerate(clouds):
        host[b, :n[b]] = c
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)
    pts, n_t, k1_t = torch.from_numpy(host).to(dev), i32(n), i32(k1)
    s1, s2 = i32([m // 2 for m in n]), i32([k // 2 for k in k1])
    radius = torch.tensor([sampling.radius_as_compared(0.2)] * len(clouds), dtype=torch.float64).to(dev)
    ts = []
    for r in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sampling.two_pass_tensors(pts, n_t, k1_t, s1, s2, radius, max(k1))
        e1.record()
        e1.synchronize()
        if r >= warmup:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30, help="timed device repetitions per shape")
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "fps_bench.txt"))
    args = ap.parse_args()
    import torch
    from adaptigraph_amd import sampling
    assert torch.cuda.is_available(), "bench_fps.py measures the GPU path: it needs an MI355X (no fallback)"
    dev = args.device
    rng = np.random.default_rng(0)
    rows = []
    for n, max_nobj in SHAPES:
        cloud = rng.uniform(0, 1, (n, 3)).astype(np.float32)
        np.random.seed(1)
        want = sampling.fps(cloud, max_nobj, RANGE)
        np.random.seed(1)
        assert np.array_equal(sampling.fps(cloud, max_nobj, RANGE, device=dev), want), (n, max_nobj)
        rows.append(dict(points=n, max_nobj=max_nobj, picked=int(len(want)),
                         host_ms=round(median_ms(lambda: sampling.fps(cloud, max_nobj, RANGE), args.host_reps, 1), 3),
                         device_ms=round(median_ms(lambda: sampling.fps(cloud, max_nobj, RANGE, device=dev), args.reps, args.warmup), 3),
                         kernel_ms=round(kernel_ms(torch, sampling, [cloud], max_nobj, dev, args.reps, args.warmup), 3)))
    clouds = [rng.uniform(0, 1, (2000, 3)).astype(np.float32) for _ in range(64)]
    np.random.seed(2)
    want = [sampling.fps(c, 200, RANGE) for c in clouds]
    np.random.seed(2)
    got = sampling.fps_batch(clouds, 200, RANGE, dev)
    assert all(np.array_equal(a, b) for a, b in zip(want, got))
    batch = dict(clouds=64, points=2000, max_nobj=200,
                 host_ms=round(median_ms(lambda: [sampling.fps(c, 200, RANGE) for c in clouds], max(1, args.host_reps // 2), 1), 3),
                 device_ms=round(median_ms(lambda: sampling.fps_batch(clouds, 200, RANGE, dev), args.reps, args.warmup), 3),
                 kernel_ms=round(kernel_ms(torch, sampling, clouds, 200, dev, args.reps, args.warmup), 3))
    line = json.dumps(dict(bench="fps", device=torch.cuda.get_device_name(0), radius_range=RANGE, reps=args.reps, host_reps=args.host_reps,
                           single=rows, batch=batch))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
