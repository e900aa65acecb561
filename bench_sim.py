"""One rope push of E episodes (`sim.rope_push`, one HIP launch) against the host restatement (`sim.rope_push_host`), measured in ONE run on one machine.

Per case (E ropes of 128 particles from `sim.initial_rope`, stiffness spread over [0, 1], a push 1.004 long through the middle of every rope: 101 push
steps + 120 settle steps = 221 steps of 8 substeps, 11 + 1 frames, in every episode) it reports
  host_ms    `rope_push_host`, the numpy code on this machine's CPU (the median of --host-reps runs for one episode; the one run that makes
             the expected result for the batched cases, which take seconds to minutes)
  device_ms  `rope_push(..., device=)` end to end: upload, the launch, the copy of all five results back; host clock, median of warmed repetitions
  kernel_ms  the launch alone between two HIP events, median of warmed repetitions
The device results are checked against the host results, bit for bit, before anything is timed.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

CASES = [(1, 128), (64, 128), (1024, 128)]      # (episodes, particles)


def make_case(sim, E, n):
    rngs = [np.random.default_rng(100 + e) for e in range(E)]
    scene = sim.RopeScene.from_ropes([sim.initial_rope(g, n) for g in rngs], stiffness=np.linspace(0.0, 1.0, E) if E > 1 else [0.5])
    mid, nxt = scene.x[:, n // 2], scene.x[:, n // 2 + 1]
    t = (nxt - mid)[:, [0, 2]].astype(np.float64)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    normal = np.stack([-t[:, 1], t[:, 0]], 1)      # across the rope
    c = mid[:, [0, 2]].astype(np.float64)
    return scene, np.concatenate([c - 0.502 * normal, c + 0.502 * normal], 1).astype(np.float32)


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def kernel_ms(torch, sim, scene, push, dev, reps, warmup):
    call = sim.DevicePush(scene, push, device=dev)
    x0, v0 = call.x.clone(), call.v.clone()
    ts = []
    for r in range(warmup + reps):
        call.x.copy_(x0)
        call.v.copy_(v0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call.launch()
        e1.record()
        e1.synchronize()
        if r >= warmup:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20, help="timed device repetitions per case")
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "sim_bench.txt"))
    args = ap.parse_args()
    import torch
    from adaptigraph_amd import sim
    assert torch.cuda.is_available(), "bench_sim.py measures the GPU path: it needs an MI355X (no fallback)"
    dev = args.device
    rows = []
    for E, n in CASES:
        scene, push = make_case(sim, E, n)
        t0 = time.perf_counter()
        want = sim.rope_push_host(scene, push)
        first_ms = (time.perf_counter() - t0) * 1e3
        print(f"# {E} x {n}: host {first_ms:.0f} ms", file=sys.stderr, flush=True)
        got = sim.rope_push(scene, push, device=dev)
        assert all(torch.equal(d.cpu(), torch.from_numpy(h)) for d, h in zip(got, want)), (E, n)
        host_ms = first_ms if E > 1 else median_ms(lambda: sim.rope_push_host(scene, push), args.host_reps, 0)
        steps = sim.push_steps(push)[0] + sim.DEFAULT.settle
        assert steps.min() == steps.max() == 221 and want[2].min() == want[2].max() == 12      # every episode does the same work
        rows.append(dict(episodes=E, particles=n, steps=int(steps[0]), frames=int(want[2][0]),
                         host_ms=round(host_ms, 1),
                         device_ms=round(median_ms(lambda: [t.cpu() for t in sim.rope_push(scene, push, device=dev)], args.reps, args.warmup), 3),
                         kernel_ms=round(kernel_ms(torch, sim, scene, push, dev, args.reps, args.warmup), 3)))
    line = json.dumps(dict(bench="sim", device=torch.cuda.get_device_name(0), reps=args.reps, host_reps=args.host_reps, cases=rows))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
