"""Simulated depth cameras (`adaptigraph_amd.render`, csrc/ag_render.hip): the host statement against ONE ag_render_depth launch, measured in one run
on one machine, and one `SimEnv.get_state_cur` (render + tabletop cloud + key points).

Two scenes seen by the four default 720 x 1280 cameras over a table plane: a rope of 128 particles and a cloth of 64 x 64 = 4 096.  Per scene:
  host_ms              `render_depth_host(accelerate=True)`, numpy float64 on this machine's CPU (median of --host-reps)
  device_ms.end_to_end host clock around `render_depth(..., device=)` from host arrays (uploads, allocation and the launch) to a device synchronise
  device_ms.launch     the launch alone on resident inputs, by device events around --inner launches, per launch
  device_ms.depth_cloud_same_images   the bare `ag_depth_cloud` call (stride 2 and stride 4) on the images just rendered, by the same
                       events: the launch writes 8 bytes per pixel (about 29 MB), so a kernel that READS the same images is the honest yardstick
  write_GBps           those 8 bytes per pixel over the launch time: an achieved rate of the output alone, not a share of peak
  get_state_cur_ms     host clock around one `SimEnv.get_state_cur` on the device, ending in a synchronise
The device images are checked against the host's, bit for bit, before anything is timed.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import time

import numpy as np


def median_ms(fn, reps, warmup, sync=None):
    ts = []
    for r in range(warmup + reps):
        if sync:
            sync()
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        if r >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


def event_ms(torch, fn, reps, warmup, inner):
    """Median over `reps` windows of `inner` back-to-back calls, by device events, per call."""
    ts = []
    for r in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        if r >= warmup:
            ts.append(a.elapsed_time(b) / inner)
    return round(statistics.median(ts), 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20, help="timed device repetitions")
    ap.add_argument("--inner", type=int, default=20, help="launches per event window")
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "render_bench.txt"))
    args = ap.parse_args()
    import torch
    from adaptigraph_amd import _lib, configs, perception as P, render as Rd, sim
    from adaptigraph_amd.sim_env import DEFAULT_BBOX, SimEnv, to_board_frame
    assert torch.cuda.is_available(), "bench_render.py measures the GPU path: it needs an MI355X (no fallback)"
    dev = torch.device(args.device)
    sync = lambda: torch.cuda.synchronize(dev)
    H, W, ratio = args.height, args.width, 10.0
    cams = Rd.default_cameras(ratio, H, W)
    plane = (0.0, 0.0, 1.0, 0.0)
    bbox = np.asarray(DEFAULT_BBOX, np.float64)
    rng = np.random.default_rng(0)
    cloth, _ = sim.initial_cloth(rng, 64, 64)
    scenes = {"rope_128": (sim.RopeScene.from_ropes([sim.initial_rope(rng, 128)], stiffness=[0.5]), "rope", sim.DEFAULT.r),
              "cloth_4096": (sim.ClothScene.from_cloths([cloth], sf=[0.5]), "cloth", sim.CLOTH_DEFAULT.r)}
    rows = []
    for label, (scene, material, r) in scenes.items():
        pts = to_board_frame(scene.x, ratio)
        n = np.asarray(scene.n, np.int32).reshape(1)
        radius = np.array([np.float32(r) * np.float32(1.0 / ratio)], np.float32)
        # ---- parity first
        want_d, want_i = Rd.render_depth_host(pts, n, radius, *cams, H, W, plane)
        got_d, got_i = Rd.render_depth(pts, n, radius, *cams, H, W, plane, device=dev)
        assert np.array_equal(got_i.cpu().numpy(), want_i) and np.array_equal(got_d.cpu().numpy().view(np.int32), want_d.view(np.int32)), label
        # ---- timings
        host = median_ms(lambda: Rd.render_depth_host(pts, n, radius, *cams, H, W, plane), args.host_reps, 0)
        renderer = Rd.DeviceRenderer(*cams, H, W, plane, E=1, device=dev)
        res = [torch.from_numpy(a).to(dev) for a in (pts, n, radius)]
        launch = event_ms(torch, lambda: renderer.launch(*res), args.reps, args.warmup, args.inner)
        depth, mask = renderer.depth[0].contiguous(), (renderer.id[0] >= 0).contiguous().view(torch.uint8)
        cams21 = torch.from_numpy(P._camera_rows(*cams)).to(dev)
        limits = torch.from_numpy(np.concatenate([[0.0, 4.0], bbox.reshape(6)])).to(dev)
        cloud = {}
        for stride in (2, 4):      # (stride 1 would be 3.7 M pixels, more than the cloud kernels' AG_TABLETOP_MAX_POINTS)
            cap = 4 * (-(-H // stride)) * (-(-W // stride))
            if cap > P.MAX_POINTS:
                continue
            out, count = torch.empty((cap, 3), dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
            ws, nbytes = P._scratch(dev, cap)
            cloud[f"stride_{stride}"] = event_ms(torch, lambda: _lib.call("ag_depth_cloud", dev, depth, mask, cams21, limits, 4, H, W, stride, out,
                                                                          count, ws, nbytes), args.reps, args.warmup, args.inner)
            cloud[f"stride_{stride}_points"] = int(count.item())
        device = dict(end_to_end=median_ms(lambda: Rd.render_depth(pts, n, radius, *cams, H, W, plane, device=dev), args.reps, args.warmup, sync),
                      launch=launch, depth_cloud_same_images=cloud)
        env = SimEnv(material, scene, configs.task_config(material), cams, dev, image_size=(H, W))
        fps_radius = configs.task_config(material)["fps_radius"]
        state = median_ms(lambda: env.get_state_cur(fps_radius), args.reps, args.warmup, sync)
        rows.append(dict(case=label, particles=int(n[0]), particle_pixels=int((want_i >= 0).sum()), host_ms=host, device_ms=device,
                         write_GBps=round(8.0 * want_i.size / (launch * 1e-3) / 1e9, 1), get_state_cur_ms=state,
                         key_points=int(env.get_state_cur(fps_radius).shape[0])))
    line = json.dumps(dict(bench="render", device=torch.cuda.get_device_name(0), images=[4, H, W], tile=Rd.TILE, chunk=Rd.CHUNK, reps=args.reps,
                           inner=args.inner, host_reps=args.host_reps, rows=rows))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
