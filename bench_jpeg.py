"""Records as JPEG frames (`adaptigraph_amd.jpeg`, csrc/ag_jpeg.hip): the host statement against ONE ag_jpeg_encode call, measured in one run on
one machine, next to what a written record pays today (the frames' copy to the host and `write_png`) and, where PIL imports, PIL's encoder as an
outside yardstick.

Two cases at 720 x 1280, RGBA frames drawn by ag_draw (bench_viz.py's evaluation frames: a 100-key-point rope with its edges, the tool and motion
trails over a sphere-splat background):
  eval_64_frames   the 64 frames of 32 rollout steps, one DeviceEncoder built for 64
  one_frame        the first of them, one DeviceEncoder built for 1
Quality 90, 4:2:0, a restart interval of 8 MCUs (the defaults).  Per case:
  host_ms_per_frame              `jpeg_scan_host`, numpy on this machine's CPU, over the first --host-frames frames (the 64 would take a minute)
  device_ms.launch               the ag_jpeg_encode call alone (its five launches) on resident frames, by device events, per call
  device_ms.encode               `DeviceEncoder.encode`, host clock: the call, the copy of the F + 1 offsets, the copy of exactly offsets[F] bytes,
                                 the files assembled as Python bytes
  today_ms.copy_to_host          the frames' copy to host memory (what the PNG path pays first), host clock to a synchronise
  today_ms.write_png_per_frame   `write_png` of one frame (zlib level 6 on one host thread); today_ms.total = copy + frames x that
  pil_ms_per_frame               PIL's JPEG encoder on a host frame with the same tables, subsampling and restart interval; null without PIL
  bytes_per_frame                the JPEG files' mean length, and one PNG's
  read_GBps                      4 bytes per pixel over the launch time: an achieved rate of the input alone, not a share of peak
The device scans are checked against the host statement's, byte for byte, before anything is timed.  Prints one JSON line and writes it to --out.
"""
import argparse
import io
import json
import os
import tempfile

import numpy as np

from bench_render import event_ms, median_ms
from bench_viz import rope_rollout


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10, help="timed device repetitions")
    ap.add_argument("--inner", type=int, default=5, help="calls per event window")
    ap.add_argument("--host-frames", type=int, default=2, help="frames the host statement and the parity check take")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=32, help="rollout steps: two frames each")
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "jpeg_bench.txt"))
    args = ap.parse_args()
    import torch
    from adaptigraph_amd import jpeg, render as Rd, sim, viz
    from adaptigraph_amd.sim_env import to_board_frame
    assert torch.cuda.is_available(), "bench_jpeg.py measures the GPU path: it needs an MI355X (no fallback)"
    dev = torch.device(args.device)
    sync = lambda: torch.cuda.synchronize(dev)      # noqa: E731
    H, W, ratio, max_nobj = args.height, args.width, 10.0, 100
    quality, subsampling, restart = 90, "420", 8
    # ---- the frames, drawn on the device
    cam = [[x[0]] for x in Rd.default_cameras(ratio, H, W)]
    cams = Rd.camera_rows(*cam)
    rng = np.random.default_rng(0)
    pred, gt, eef, full = rope_rollout(rng, args.steps, max_nobj, 400)
    edges = [viz.radius_edges_host(pred[t], 0.5, 10) for t in range(args.steps)]
    tool_edges = [(np.concatenate([r, np.full(3, max_nobj)]), np.concatenate([s, np.array([40, 50, 60])])) for r, s in edges]
    dl = viz.rollout_frames(pred[None], gt[None], eef[None], [tool_edges], [max_nobj], max_nobj, ratio, backgrounds=[list(range(args.steps))])
    pts, prims, styles, frames = dl.tables()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    E = len(full)
    renderer = Rd.DeviceRenderer(*cam, H, W, (0.0, 0.0, 1.0, 0.0), E=E, device=dev)
    renderer.launch(up(to_board_frame(full, ratio)), up(np.full(E, full.shape[1], np.int32)),
                    up(np.full(E, np.float32(sim.DEFAULT.r) * np.float32(1.0 / ratio), np.float32)))
    canvas = viz.DeviceCanvas(cams, H, W, len(frames), len(pts), device=dev)
    drawn = canvas.launch(up(pts), up(prims), up(styles), up(frames), 128, 2, renderer.id[:, 0].contiguous(), up(np.asarray(viz.PALETTE, np.int32)),
                          viz.TABLE_COLOR, viz.VOID_COLOR)
    sync()
    try:
        from PIL import Image
    except ImportError:
        Image = None
    lum, chrom = jpeg.quant_tables(quality)
    rows = []
    for label, images in (("eval_64_frames", drawn), ("one_frame", drawn[:1])):
        F = int(images.shape[0])
        k = min(args.host_frames, F)
        host_frames = images[:k].cpu().numpy()
        enc = jpeg.DeviceEncoder(H, W, F, quality, subsampling, restart, channels=4, device=dev)
        # ---- parity first
        want = jpeg.jpeg_scan_host(host_frames, quality, subsampling, restart)
        files = enc.encode(images)
        assert [f[len(enc.header):-2] for f in files[:k]] == want and len(files) == F, label
        # ---- timings
        host = median_ms(lambda: jpeg.jpeg_scan_host(host_frames, quality, subsampling, restart), 1, 0) / k
        launch = event_ms(torch, lambda: enc.launch(images), args.reps, args.warmup, args.inner)
        encode = median_ms(lambda: enc.encode(images), args.reps, args.warmup, sync)
        copy = median_ms(lambda: images.cpu(), args.reps, args.warmup, sync)
        with tempfile.TemporaryDirectory() as tmp:
            png = median_ms(lambda: viz.write_png(os.path.join(tmp, "frame.png"), host_frames[0]), 5, 1)
            png_bytes = os.path.getsize(os.path.join(tmp, "frame.png"))
        pil = None
        if Image is not None:
            rgb = Image.fromarray(np.ascontiguousarray(host_frames[0][..., :3]))
            pil = median_ms(lambda: rgb.save(io.BytesIO(), "JPEG", qtables=[[int(x) for x in lum], [int(x) for x in chrom]], subsampling=2,
                                             restart_marker_blocks=restart, optimize=False), 5, 1)
        rows.append(dict(case=label, frames=F, host_ms_per_frame=round(host, 3), host_frames=k,
                         device_ms=dict(launch=launch, encode=encode),
                         today_ms=dict(copy_to_host=copy, write_png_per_frame=png, total=round(copy + F * png, 3)),
                         pil_ms_per_frame=pil, bytes_per_frame=dict(jpeg=round(sum(map(len, files)) / F), png=png_bytes),
                         scratch_MB=round(enc.scratch_bytes / 1e6, 1), out_MB=round(enc.out_bytes / 1e6, 1),
                         read_GBps=round(4.0 * F * H * W / (launch * 1e-3) / 1e9, 1)))
        del enc
    line = json.dumps(dict(bench="jpeg", device=torch.cuda.get_device_name(0), image=[H, W], quality=quality, subsampling=subsampling, restart=restart,
                           reps=args.reps, inner=args.inner, rows=rows))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
