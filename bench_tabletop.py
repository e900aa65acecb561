"""The tabletop cloud from depth images (`adaptigraph_amd.perception`): the host statement against the HIP path, measured in ONE run on one machine.

Input: a synthetic scene (`synth.tabletop_scene`, generated here from a seed): four 720 x 1280 depth images of a board with a rope-like object,
range noise, flying pixels, holes and NaNs, and the keep-mask per camera.  Two rows: with the masks (the object's neighbourhood: what the closed
loop sees) and without them (the whole board inside the workspace: the 10^5-point end of the range).  Per row, medians over warmed repetitions:
  host_ms     per stage and end to end (`get_tabletop_points`, then `state_from_depth`), numpy float64 on this machine's CPU.  The neighbour search
              of the host path uses scipy's k-d tree when scipy imports (`knn_mean_host`); without scipy the host side is timed at stride 8 instead
              of 4 with the O(n^2) statement, and the row says so (`host_reduced`).
  device_ms   the same stages on the GPU, host clock around work that ends in a device synchronise: per stage on resident inputs, `end_to_end`
              from host arrays (upload included) to the final count, `state_from_depth` to state_cur on the device.
and the number of denoise iterations with the points each iteration sent to the brute-force pass.  Every device result is checked against the
host result before anything is timed.  Prints one JSON line and writes it to --out.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20, help="timed device repetitions")
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--band", type=float, default=0.05, help="half-width of the masked neighbourhood of the object, metres")
    ap.add_argument("--k-filter", type=float, default=0.95)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "tabletop_bench.txt"))
    args = ap.parse_args()
    import torch
    from adaptigraph_amd import perception as P, synth
    assert torch.cuda.is_available(), "bench_tabletop.py measures the GPU path: it needs an MI355X (no fallback)"
    dev = args.device
    sync = lambda: torch.cuda.synchronize(dev)
    try:
        import scipy.spatial      # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    scene = synth.tabletop_scene(4, args.height, args.width, seed=0, band=args.band)
    cam = (scene["R"], scene["t"], scene["intr"], scene["bbox"])
    rows = []
    for label, masks in (("masked", scene["masks"]), ("unmasked", None)):
        kw = dict(keep_masks=masks, stride=4)
        hkw = kw if have_scipy else dict(keep_masks=masks, stride=8)
        # ---- parity first: the device cloud against the host cloud, the key points under one seed
        crop = P.depth_to_points_host(scene["depth"], *cam, **kw)
        merged = P.voxel_down_sample_host(crop, P.VOXEL_SIZE)
        if have_scipy:
            clean, iters = P.denoise_host(merged)
            final = P.height_filter_host(clean, args.k_filter)
            got = P.get_tabletop_points(scene["depth"], *cam, k_filter=args.k_filter, device=dev, **kw).numpy()
            assert np.array_equal(got, final), (label, got.shape, final.shape)
            np.random.seed(3)
            want_state = P.state_from_depth(scene["depth"], *cam, k_filter=args.k_filter, sim_real_ratio=10.0, fps_radius=0.2, device=None, **kw)
            np.random.seed(3)
            got_state = P.state_from_depth(scene["depth"], *cam, k_filter=args.k_filter, sim_real_ratio=10.0, fps_radius=0.2, device=dev, **kw)
            assert np.array_equal(got_state.cpu().numpy(), want_state), label
        dcrop = P.depth_to_points(scene["depth"], *cam, device=dev, **kw)
        assert np.array_equal(dcrop.numpy(), crop) and np.array_equal(P.voxel_down_sample(dcrop, P.VOXEL_SIZE).numpy(), merged), label
        # ---- host
        hcrop = P.depth_to_points_host(scene["depth"], *cam, **hkw)
        hmerged = P.voxel_down_sample_host(hcrop, P.VOXEL_SIZE)
        hclean, hiters = P.denoise_host(hmerged)
        host = dict(points=int(len(hcrop)), merged=int(len(hmerged)), denoised=int(len(hclean)), denoise_iterations=int(hiters),
                    crop=median_ms(lambda: P.depth_to_points_host(scene["depth"], *cam, **hkw), args.host_reps, 1),
                    voxel=median_ms(lambda: P.voxel_down_sample_host(hcrop, P.VOXEL_SIZE), args.host_reps, 1),
                    denoise=median_ms(lambda: P.denoise_host(hmerged), args.host_reps, 0),
                    height=median_ms(lambda: P.height_filter_host(hclean, args.k_filter), args.host_reps, 1),
                    end_to_end=median_ms(lambda: P.get_tabletop_points(scene["depth"], *cam, k_filter=args.k_filter, **hkw), args.host_reps, 0),
                    state_from_depth=median_ms(lambda: P.state_from_depth(scene["depth"], *cam, k_filter=args.k_filter, sim_real_ratio=10.0,
                                                                          fps_radius=0.2, device=None, **hkw), args.host_reps, 0))
        # ---- device
        depth_t = [torch.from_numpy(d).to(dev) for d in scene["depth"]]
        masks_t = None if masks is None else [torch.from_numpy(m).to(dev) for m in masks]
        rkw = dict(keep_masks=masks_t, stride=4)
        dmerged = P.voxel_down_sample(dcrop, P.VOXEL_SIZE)
        stats = []
        dclean, diters = P.denoise_device(P.DeviceCloud(dmerged.pts, dmerged.count, dmerged.n), stats=stats)
        brute = [int(info[0].item()) for info, _ in stats]
        fresh = lambda c: P.DeviceCloud(c.pts, c.count, c.n)      # (denoise sets .n on the cloud it is given)
        device = dict(points=dcrop.size(), merged=dmerged.size(), denoised=dclean.size(), denoise_iterations=int(diters), brute_force_points=brute,
                      grid_cells=int(stats[0][0][1].item()) if stats else 0,
                      crop=median_ms(lambda: P.depth_to_points(depth_t, *cam, device=dev, **rkw), args.reps, args.warmup, sync),
                      voxel=median_ms(lambda: P.voxel_down_sample_device(fresh(dcrop), P.VOXEL_SIZE, extent_checked=True), args.reps, args.warmup, sync),
                      knn_mean_once=median_ms(lambda: P.knn_mean_device(dmerged, 20), args.reps, args.warmup, sync),
                      denoise=median_ms(lambda: P.denoise_device(fresh(dmerged)), args.reps, args.warmup, sync),
                      height=median_ms(lambda: P.height_filter_device(fresh(dclean), args.k_filter), args.reps, args.warmup, sync),
                      end_to_end_resident=median_ms(lambda: P.get_tabletop_points(depth_t, *cam, k_filter=args.k_filter, device=dev, **rkw).size(),
                                                    args.reps, args.warmup, sync),
                      end_to_end=median_ms(lambda: P.get_tabletop_points(scene["depth"], *cam, k_filter=args.k_filter, device=dev, **kw).size(),
                                           args.reps, args.warmup, sync),
                      state_from_depth=median_ms(lambda: P.state_from_depth(scene["depth"], *cam, k_filter=args.k_filter, sim_real_ratio=10.0,
                                                                            fps_radius=0.2, device=dev, **kw), args.reps, args.warmup, sync))
        rows.append(dict(case=label, host_reduced=not have_scipy, host_ms=host, device_ms=device))
    line = json.dumps(dict(bench="tabletop", device=torch.cuda.get_device_name(0), images=[4, args.height, args.width], stride=4, band=args.band,
                           k_filter=args.k_filter, host_neighbour_search="scipy cKDTree + exact redo" if have_scipy else "O(n^2) statement at stride 8",
                           reps=args.reps, host_reps=args.host_reps, rows=rows))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
