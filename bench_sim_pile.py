"""One board push of E granular episodes (`sim.pile_push`, one HIP launch) against the host statement (`sim.pile_push_host`), measured in ONE run on one machine.

Per case (E piles of k x k grains on a jittered lattice at 1.15 of their size -- 16 x 16 of size 0.15, 25 x 25 of size 0.1 -- and a push 1.004 long
driven obliquely into the pile's edge: 101 push steps + 120 settle steps = 221 steps of 8 substeps of 4 contact iterations, 11 + 1 frames, in every
episode) it reports
  host_ms    `pile_push_host`, the numpy code on this machine's CPU, for the first `host_episodes` episodes of the case (all of one, four of
             more: the batched host code takes minutes for 64 piles and hours for 1 024); the median of --host-reps runs for one episode
  device_ms  `pile_push(..., device=)` end to end: upload, the launch, the copy of all five results back; host clock, median of warmed repetitions
  kernel_ms  the launch alone between two HIP events, median of warmed repetitions
The device results of the first `host_episodes` episodes are checked against the host results, bit for bit, and every other episode against a
second launch, before anything is timed.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

CASES = [(1, 16, 0.15), (64, 16, 0.15), (1024, 16, 0.15), (1, 25, 0.1), (64, 25, 0.1), (1024, 25, 0.1)]      # (episodes, grains per side, grain size)
HOST_EPISODES = 4


def make_case(sim, E, k, scale):
    piles = []
    c = (np.arange(k) - (k - 1) / 2) * 1.15 * scale
    gx, gz = np.meshgrid(c, c, indexing="ij")
    for e in range(E):
        xz = np.stack([gx.ravel(), gz.ravel()], 1) + np.random.default_rng(100 + e).uniform(-0.03, 0.03, (k * k, 2)) * scale
        piles.append(np.stack([xz[:, 0], np.full(k * k, scale / 2), xz[:, 1]], 1).astype(np.float32))
    scene = sim.PileScene.from_piles(piles, [scale / 2] * E)
    a = np.deg2rad(20.0) + np.linspace(0.0, 0.2, E)      # into the -x edge, from outside it, a little more oblique from episode to episode
    x0 = c[0] - (0.3 + scale)
    push = np.stack([np.full(E, x0), np.full(E, 0.02), x0 + 1.004 * np.cos(a), 0.02 + 1.004 * np.sin(a)], 1).astype(np.float32)
    return scene, push


def first(sim, scene, push, m):
    return sim.PileScene(scene.n[:m], scene.rho[:m], scene.x[:m], scene.v[:m]), push[:m]


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
    call = sim.DevicePilePush(scene, push, device=dev)
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
    ap.add_argument("--reps", type=int, default=10, help="timed device repetitions per case")
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "sim_pile_bench.txt"))
    args = ap.parse_args()
    import torch
    from adaptigraph_amd import sim
    assert torch.cuda.is_available(), "bench_sim_pile.py measures the GPU path: it needs an MI355X (no fallback)"
    dev = args.device
    rows = []
    for E, k, scale in CASES:
        scene, push = make_case(sim, E, k, scale)
        m = min(E, HOST_EPISODES)
        sub = first(sim, scene, push, m)
        t0 = time.perf_counter()
        want = sim.pile_push_host(*sub)
        first_ms = (time.perf_counter() - t0) * 1e3
        print(f"# {E} x {k * k}: host, {m} episodes, {first_ms:.0f} ms", file=sys.stderr, flush=True)
        got = [t.cpu() for t in sim.pile_push(scene, push, device=dev)]
        again = [t.cpu() for t in sim.pile_push(scene, push, device=dev)]
        assert all(torch.equal(d[:m], torch.from_numpy(h)) for d, h in zip(got, want)), (E, k)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), (E, k)
        host_ms = first_ms if E > 1 else median_ms(lambda: sim.pile_push_host(*sub), args.host_reps, 0)
        steps = sim.push_steps(push, sim.PILE_DEFAULT)[0] + sim.PILE_DEFAULT.settle
        assert steps.min() == steps.max() == 221 and int(got[2].min()) == int(got[2].max()) == 12      # every episode does the same work
        assert float((got[3] - torch.from_numpy(scene.x)).abs().amax(dim=(1, 2)).min()) > 0.3          # and its board has moved grains
        rows.append(dict(episodes=E, grains=k * k, steps=int(steps[0]), frames=int(got[2][0]), host_episodes=m,
                         host_ms=round(host_ms, 1),
                         device_ms=round(median_ms(lambda: [t.cpu() for t in sim.pile_push(scene, push, device=dev)], args.reps, args.warmup), 3),
                         kernel_ms=round(kernel_ms(torch, sim, scene, push, dev, args.reps, args.warmup), 3)))
    line = json.dumps(dict(bench="sim_pile", device=torch.cuda.get_device_name(0), reps=args.reps, host_reps=args.host_reps, cases=rows))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
