"""Rollout and planning records as images (`adaptigraph_amd.viz`, csrc/ag_draw.hip): the host statement against ONE ag_draw call, measured in one
run on one machine, next to what surrounds it in a written record.

Two cases at 720 x 1280 over a sphere-splat background (ag_render_depth's id images, background mode 2):
  eval_64_frames   64 evaluation frames: 32 rollout steps, a pred and a gt frame each, of a 100-key-point rope with its edge lists, the tool
                   and five steps of motion trails (viz.rollout_frames)
  planning_frame   one frame of the closed loop: start state and edges, three action arrows, a 400-point target cloud and the predicted state
                   and edges as the overlay (viz.planning_frame)
Per case:
  host_ms.draw / .render         `draw_host(accelerate=True)` and `render_depth_host` of the backgrounds, numpy on this machine's CPU: the median of
                                 --host-reps runs without warm-up, ONE run by default (the 64 frames take seconds); the device figures are medians
                                 of --reps windows after --warmup
  device_ms.launch               the ag_draw call alone (its two launches) on resident tables and backgrounds, by device events, per call
  device_ms.render_same_frames   the ag_render_depth launch that makes those backgrounds, by the same events: 8 bytes written per pixel against
                                 ag_draw's 4 written and 4 read, the yardstick for a kernel of this shape
  device_ms.end_to_end           host clock from host arrays (the particles and the display list's points uploaded, render, draw) to a synchronise
  device_ms.copy_to_host         the images' copy to host memory, what a written record pays next
  write_png_ms_per_frame         `write_png` of one frame (zlib level 6 on the host): it dominates a written record and is reported, not hidden
  write_GBps                     4 bytes per pixel over the launch time: an achieved rate of the output alone, not a share of peak
The device images are checked against the host's, bit for bit, before anything is timed.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import tempfile
import time

import numpy as np

from bench_render import event_ms, median_ms


def rope_rollout(rng, steps, n_kp, n_particles):
    """A rope drifting and bending over `steps` steps in simulator units: key points (pred, gt), the tool, the edges, all the particles."""
    s = np.linspace(-2.0, 2.0, n_particles)
    t = np.arange(steps)[:, None]
    full = np.stack([s[None, :] + 0.02 * t, np.full((steps, n_particles), 0.03), 0.4 * np.sin(1.5 * s[None, :] + 0.1 * t) + 0.03 * t], 2).astype(np.float32)
    pick = np.linspace(0, n_particles - 1, n_kp).astype(int)
    gt = full[:, pick]
    pred = gt + rng.normal(0, 0.01, gt.shape).astype(np.float32) * np.sqrt(1.0 + t[:, :, None])
    eef = np.stack([np.full(steps, 0.5) + 0.02 * t[:, 0], np.full(steps, 0.1), 1.0 - 0.04 * t[:, 0]], 1)[:, None, :].astype(np.float32)
    return pred, gt, eef, full


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10, help="timed device repetitions")
    ap.add_argument("--inner", type=int, default=5, help="calls per event window")
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=32, help="rollout steps of the evaluation case: two frames each")
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "viz_bench.txt"))
    args = ap.parse_args()
    import torch
    from adaptigraph_amd import render as Rd, sim, viz
    from adaptigraph_amd.sim_env import to_board_frame
    assert torch.cuda.is_available(), "bench_viz.py measures the GPU path: it needs an MI355X (no fallback)"
    dev = torch.device(args.device)
    sync = lambda: torch.cuda.synchronize(dev)      # noqa: E731
    H, W, ratio, max_nobj = args.height, args.width, 10.0, 100
    cam = [[x[0]] for x in Rd.default_cameras(ratio, H, W)]
    cams = Rd.camera_rows(*cam)
    plane = (0.0, 0.0, 1.0, 0.0)
    rng = np.random.default_rng(0)
    pred, gt, eef, full = rope_rollout(rng, args.steps, max_nobj, 400)
    edges = [viz.radius_edges_host(pred[t], 0.5, 10) for t in range(args.steps)]
    tool_edges = [(np.concatenate([r, np.full(3, max_nobj)]), np.concatenate([s, np.array([40, 50, 60])])) for r, s in edges]
    cases = {}
    cases["eval_64_frames"] = (viz.rollout_frames(pred[None], gt[None], eef[None], [tool_edges], [max_nobj], max_nobj, ratio,
                                                  backgrounds=[list(range(args.steps))]), full, 128)
    target = np.stack([rng.uniform(-1.5, 1.5, 400), np.full(400, 0.03), rng.uniform(-1.0, 1.0, 400)], 1).astype(np.float32)
    cases["planning_frame"] = (viz.planning_frame(gt[0], pred[1], (0.5, 1.0, 0.5, 0.9), 3, edges[0], edges[1], ratio, target_state=target), full[:1], 128)
    palette = np.asarray(viz.PALETTE, np.int32)
    rows = []
    for label, (dl, particles, alpha) in cases.items():
        pts, prims, styles, frames = dl.tables()
        E, F = len(particles), len(frames)
        scene = to_board_frame(particles, ratio)
        n = np.full(E, particles.shape[1], np.int32)
        radius = np.full(E, np.float32(sim.DEFAULT.r) * np.float32(1.0 / ratio), np.float32)
        # ---- parity first
        host_render = median_ms(lambda: Rd.render_depth_host(scene, n, radius, *cam, H, W, plane), args.host_reps, 0)
        ids = Rd.render_depth_host(scene, n, radius, *cam, H, W, plane)[1][:, 0]
        draw_args = (cams, H, W, alpha, 2, ids, palette, viz.TABLE_COLOR, viz.VOID_COLOR)
        want = viz.draw_host(pts, prims, styles, frames, *draw_args)
        host_draw = median_ms(lambda: viz.draw_host(pts, prims, styles, frames, *draw_args), args.host_reps, 0)
        renderer = Rd.DeviceRenderer(*cam, H, W, plane, E=E, device=dev)
        canvas = viz.DeviceCanvas(cams, H, W, F, len(pts), device=dev)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        res = [up(scene), up(n), up(radius)]
        tables = [up(pts), up(prims), up(styles), up(frames)]
        pal = up(palette)

        def draw_on_device():
            return canvas.launch(*tables, alpha, 2, renderer.id[:, 0], pal, viz.TABLE_COLOR, viz.VOID_COLOR)

        renderer.launch(*res)
        got = draw_on_device()
        assert np.array_equal(renderer.id[:, 0].cpu().numpy(), ids) and np.array_equal(got.cpu().numpy(), want), label
        # ---- timings
        launch = event_ms(torch, draw_on_device, args.reps, args.warmup, args.inner)
        render_launch = event_ms(torch, lambda: renderer.launch(*res), args.reps, args.warmup, args.inner)

        def end_to_end():
            renderer.launch(up(scene), res[1], res[2])
            tables[0] = up(pts)
            draw_on_device()

        e2e = median_ms(end_to_end, args.reps, args.warmup, sync)
        copy = median_ms(lambda: got.cpu(), args.reps, args.warmup, sync)
        with tempfile.TemporaryDirectory() as tmp:
            png = median_ms(lambda: viz.write_png(os.path.join(tmp, "frame.png"), want[0]), min(5, 3 * args.host_reps + 2), 1)
            png_bytes = os.path.getsize(os.path.join(tmp, "frame.png"))
        rows.append(dict(case=label, frames=F, backgrounds=E, points=int(len(pts)), primitives=int(len(prims)),
                         host_ms=dict(draw=host_draw, render=host_render),
                         device_ms=dict(launch=launch, render_same_frames=render_launch, end_to_end=e2e, copy_to_host=copy),
                         write_png_ms_per_frame=png, png_bytes=png_bytes, write_GBps=round(4.0 * F * H * W / (launch * 1e-3) / 1e9, 1)))
    line = json.dumps(dict(bench="viz", device=torch.cuda.get_device_name(0), image=[H, W], tile=Rd.TILE, chunk=Rd.CHUNK, reps=args.reps,
                           inner=args.inner, host_reps=args.host_reps, rows=rows))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
