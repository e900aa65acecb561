"""One push of E box episodes (`sim.box_push`, one HIP launch) against the host statement (`sim.box_push_host`), measured in ONE run on one machine.

Per case (E boxes 2.0 x 1.0 of k x k particles, each turned by its own angle and with its own centre of mass, pushed squarely into a long
face from 1.0 outside it over 5.0, a quarter of the side off the geometric centre: 500 or 501 push steps + 30 settle steps of 8 substeps of 2
corrections, 51 or 52 frames, in every episode) it reports
  host_ms    `box_push_host`, the numpy code on this machine's CPU, for the first `host_episodes` episodes of the case (all of one, four of more)
  device_ms  `box_push(..., device=)` end to end: upload, the launch, the copy of all six results back; host clock, median of warmed repetitions
  kernel_ms  the launch alone between two HIP events, median of warmed repetitions
  substep_us kernel_ms over the substeps of the longest episode: what one pass of predict, pusher, velocity, four sums and a barrier costs
The device results of the first `host_episodes` episodes are checked against the host results, bit for bit, and every other episode against a
second launch, before anything is timed.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

CASES = [(1, 16), (64, 16), (1024, 16), (1, 32), (64, 32), (1024, 32)]      # (episodes, particles per side)
HOST_EPISODES = 4
SIZE, LENGTH = (2.0, 1.0), 5.0


def make_case(sim, E, k):
    coms = [(0.3 * math.cos(1.0 + e), 0.3 * math.sin(2.0 + 3 * e)) for e in range(E)]
    angles = [2.0 * math.pi * e / max(E, 7) for e in range(E)]      # every episode turned by its own angle
    scene = sim.BoxScene.from_boxes([SIZE] * E, coms, angles, grids=[(k, k)] * E)
    push = []
    for e in range(E):
        X, Z, co, si = (float(c) for c in scene.pose[e].astype(np.float64))
        lx, lz0 = 0.25 * SIZE[0] - coms[e][0] * SIZE[0], -0.5 * SIZE[1] - 1.0 - coms[e][1] * SIZE[1]      # in the frame of the centre of mass
        push.append([X + co * lx - si * lz0, Z + si * lx + co * lz0, X + co * lx - si * (lz0 + LENGTH), Z + si * lx + co * (lz0 + LENGTH)])
    return scene, np.array(push, np.float32)


def first(sim, scene, push, m):
    import dataclasses
    fields = {f.name: getattr(scene, f.name)[:m] for f in dataclasses.fields(scene) if f.name != "r"}
    return sim.BoxScene(**fields, r=scene.r), push[:m]


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
    call = sim.DeviceBoxPush(scene, push, device=dev)
    pose0, vel0 = call.pose.clone(), call.vel.clone()
    ts = []
    for r in range(warmup + reps):
        call.pose.copy_(pose0)
        call.vel.copy_(vel0)
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
    ap.add_argument("--reps", type=int, default=5, help="timed device repetitions per case")
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "sim_box_bench.txt"))
    args = ap.parse_args()
    import torch
    from adaptigraph_amd import sim
    assert torch.cuda.is_available(), "bench_sim_box.py measures the GPU path: it needs an MI355X (no fallback)"
    dev = args.device
    P = sim.BOX_DEFAULT
    rows = []
    for E, k in CASES:
        scene, push = make_case(sim, E, k)
        m = min(E, HOST_EPISODES)
        sub = first(sim, scene, push, m)
        t0 = time.perf_counter()
        want = sim.box_push_host(*sub)
        first_ms = (time.perf_counter() - t0) * 1e3
        print(f"# {E} x {k * k}: host, {m} episodes, {first_ms:.0f} ms", file=sys.stderr, flush=True)
        f_max = int(sim.frames_of(sim.push_steps(push, P)[0], P).max())      # the host ran the first m alone: give it the case's frames to compare
        want = sim.box_push_host(*sub, f_max=f_max) if want[0].shape[1] != f_max else want
        got = [t.cpu() for t in sim.box_push(scene, push, device=dev)]
        again = [t.cpu() for t in sim.box_push(scene, push, device=dev)]
        assert all(torch.equal(d[:m], torch.from_numpy(h)) for d, h in zip(got, want)), (E, k)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), (E, k)
        del again
        host_ms = first_ms if E > 1 else median_ms(lambda: sim.box_push_host(*sub), args.host_reps, 0)
        steps = sim.push_steps(push, P)[0] + P.settle
        assert steps.min() >= 530 and steps.max() <= 531 and int(got[3].min()) >= 51                  # every episode does the same work
        assert float((got[4][:, :2] - torch.from_numpy(scene.pose[:, :2])).norm(dim=1).min()) > 0.1      # and its box was pushed away
        assert not bool(got[5].any())                                                                 # and has come to rest
        kms = kernel_ms(torch, sim, scene, push, dev, args.reps, args.warmup)
        rows.append(dict(episodes=E, particles=k * k, steps=int(steps.max()), frames=int(got[3].max()), host_episodes=m,
                         host_ms=round(host_ms, 1),
                         device_ms=round(median_ms(lambda: [t.cpu() for t in sim.box_push(scene, push, device=dev)], args.reps, args.warmup), 3),
                         kernel_ms=round(kms, 3), substep_us=round(1e3 * kms / (int(steps.max()) * P.substeps), 3)))
        print(f"# {rows[-1]}", file=sys.stderr, flush=True)
        del got
    line = json.dumps(dict(bench="sim_box", device=torch.cuda.get_device_name(0), reps=args.reps, host_reps=args.host_reps, cases=rows))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
