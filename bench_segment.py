"""Object masks from colour images (`adaptigraph_amd.segment`, csrc/ag_segment.hip): the numpy statement against the device calls, measured in one
run on one machine, next to scipy.ndimage where it imports.

Two scenes seen by SimEnv's four 720 x 1280 cameras, RGBA as ag_draw writes them:
  rope    a 100-particle rope
  cloth   a 64 x 64 cloth
Per scene, on the four colour images (C = 4):
  host_ms            the statement on this machine's CPU, once: color_mask_host, opening_host (r = 2), label_host, components_host, select_host,
                     fill_holes_host, keep_mask_host (table key only, SimEnv's call) and keep_mask_host with the whole chain
  scipy_ms           ndimage.binary_opening, label, binary_fill_holes on the same masks, per four images; null without scipy
  device_ms          each DeviceSegmenter stage on resident tensors by device events, the median of --reps windows of --inner calls after
                     --warmup windows, per call: color_mask, erode, opening, label, components, select (min_area), select_largest (keep_largest),
                     fill_holes, keep_mask (table key only) and keep_mask_chain (opening 1, closing 1, min_area 16, keep_largest 4, object keys, fill)
  label_on_noise_ms  `label` on four seeded noise masks at density 0.59 (4-connectivity: its percolation density), the labelling's worst case here
  state_cur_ms       SimEnv.get_state_cur with masks="ids" and masks="color", host clock to a synchronise, alternating
  min_MB             what a stage must move at least: the RGBA images in, a mask, the labels out
  label_GBps         (mask in + labels out) over the label time: an achieved rate, not a share of peak
The device results are checked against the statement, bit for bit, before anything is timed.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import time

import numpy as np

from bench_render import event_ms, median_ms


def rope_scene(sim, n=100):
    i = np.arange(n)
    rope = np.stack([0.05 * (i - (n - 1) / 2), np.full(n, sim.DEFAULT.r), 0.6 * np.sin(0.12 * i)], 1).astype(np.float32)
    return "rope", sim.RopeScene.from_ropes([rope], stiffness=[0.5])


def cloth_scene(sim, k=64, side=3.0):
    c = (np.arange(k) - (k - 1) / 2) * (side / (k - 1))
    gx, gz = np.meshgrid(c, c)
    cloth = np.stack([gx, np.full_like(gx, sim.CLOTH_DEFAULT.r), gz], 2).astype(np.float32)
    return "cloth", sim.ClothScene.from_cloths([cloth], sf=[0.5], l0=[side / (k - 1)])


def once_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, round((time.perf_counter() - t0) * 1e3, 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10, help="timed device windows")
    ap.add_argument("--inner", type=int, default=10, help="calls per event window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "segment_bench.txt"))
    args = ap.parse_args()
    import torch
    from adaptigraph_amd import configs, segment, sim, viz
    from adaptigraph_amd.sim_env import SimEnv
    assert torch.cuda.is_available(), "bench_segment.py measures the GPU path: it needs an MI355X (no fallback)"
    dev = torch.device(args.device)
    sync = lambda: torch.cuda.synchronize(dev)      # noqa: E731
    H, W = args.height, args.width
    try:
        from scipy import ndimage as ndi
    except ImportError:
        ndi = None
    table_keys = [segment.ColorKey.exact(viz.TABLE_COLOR)]
    object_keys = [segment.ColorKey(30, 50, 40, 120, 150, 255)]      # the palette: hues 39-40, S 63-93
    chain = dict(open_radius=1, close_radius=1, min_area=16, keep_largest=4, fill=True)
    ev = lambda fn: event_ms(torch, fn, args.reps, args.warmup, args.inner)      # noqa: E731
    rows = []
    for material, scene in (rope_scene(sim), cloth_scene(sim)):
        make = lambda **kw: SimEnv(material, scene, configs.task_config(material), None, dev, image_size=(H, W), **kw)      # noqa: E731
        env_ids, env_color = make(), make(masks="color")
        _, ids = env_ids.render()
        images = env_ids.color(ids).clone()
        C = int(images.shape[0])
        seg = segment.DeviceSegmenter(C, H, W, dev)
        host_images = images.cpu().numpy()
        # ---- the statement, once, and parity
        host = {}
        objects, host["color_mask"] = once_ms(lambda: segment.color_mask_host(host_images, object_keys))
        opened, host["opening_r2"] = once_ms(lambda: segment.opening_host(objects, 2))
        (labels, count), host["label"] = once_ms(lambda: segment.label_host(objects, 8))
        (table, _), host["components"] = once_ms(lambda: segment.components_host(labels, count, 64))
        selected, host["select"] = once_ms(lambda: segment.select_host(objects, 16, None, 8))
        largest, host["select_largest"] = once_ms(lambda: segment.select_host(objects, 0, 2, 8))
        filled, host["fill_holes"] = once_ms(lambda: segment.fill_holes_host(objects, 8))
        keep, host["keep_mask"] = once_ms(lambda: segment.keep_mask_host(host_images, table_keys))
        keep_chain, host["keep_mask_chain"] = once_ms(lambda: segment.keep_mask_host(host_images, table_keys, object_keys, **chain))
        d_objects = seg.color_mask(images, object_keys)
        d_labels, d_count = seg.label(d_objects, 8)
        same = lambda t, a: np.array_equal(t.cpu().numpy(), np.asarray(a))      # noqa: E731
        assert same(d_objects, objects) and same(seg.morph("opening", d_objects, 2), opened) and same(d_labels, labels) and same(d_count, count), material
        assert same(seg.components(d_labels, d_count, 64)[0], table) and same(seg.select(d_objects, 16), selected), material
        assert same(seg.select(d_objects, 0, 2), largest) and same(seg.fill_holes(d_objects), filled), material
        assert same(seg.keep_mask(images, table_keys), keep) and same(seg.keep_mask(images, table_keys, object_keys, **chain), keep_chain), material
        assert same(seg.keep_mask(images, table_keys), ids.cpu().numpy() != -1), material
        scipy_ms = None
        if ndi is not None:
            st = np.ones((5, 5), bool)
            scipy_ms = dict(opening_r2=once_ms(lambda: [ndi.binary_opening(m, st) for m in objects])[1],
                            label=once_ms(lambda: [ndi.label(m, np.ones((3, 3), int)) for m in objects])[1],
                            fill_holes=once_ms(lambda: [ndi.binary_fill_holes(m) for m in objects])[1])
        # ---- the device stages
        out = torch.empty_like(d_objects)
        device = dict(color_mask=ev(lambda: seg.color_mask(images, object_keys, out=out)),
                      erode_r2=ev(lambda: seg.morph("erode", d_objects, 2, out=out)),
                      opening_r2=ev(lambda: seg.morph("opening", d_objects, 2, out=out)),
                      label=ev(lambda: _lib_label(seg, d_objects, d_labels, d_count)),
                      components=ev(lambda: seg.components(d_labels, d_count, 64)),
                      select=ev(lambda: seg.select(d_objects, 16, None, 8, out=out)),
                      select_largest=ev(lambda: seg.select(d_objects, 0, 2, 8, out=out)),
                      fill_holes=ev(lambda: seg.fill_holes(d_objects, 8, out=out)),
                      keep_mask=ev(lambda: seg.keep_mask(images, table_keys)),
                      keep_mask_chain=ev(lambda: seg.keep_mask(images, table_keys, object_keys, **chain)))
        noise = torch.from_numpy(np.random.default_rng(59).random((C, H, W)) < 0.59).to(dev).view(torch.uint8)
        on_noise = {c: ev(lambda c=c: _lib_label(seg, noise, d_labels, d_count, c)) for c in (4, 8)}
        # ---- the closed loop's observation
        task = configs.task_config(material)
        state = {}
        for _ in range(2):      # alternating
            for name, env in (("ids", env_ids), ("color", env_color)):
                state.setdefault(name, []).append(median_ms(lambda env=env: env.get_state_cur(task["fps_radius"]), 5, 2, sync))
        np.random.seed(0)
        a = env_ids.get_state_cur(task["fps_radius"])
        np.random.seed(0)
        assert torch.equal(a, env_color.get_state_cur(task["fps_radius"])), material
        min_mb = dict(images_in=round(images.numel() / 1e6, 1), mask=round(C * H * W / 1e6, 1), labels=round(4 * C * H * W / 1e6, 1))
        rows.append(dict(scene=material, images=[C, H, W, int(images.shape[3])], components=[int(x) for x in count], host_ms=host, scipy_ms=scipy_ms,
                         device_ms=device, label_on_noise_ms={f"connectivity_{c}": v for c, v in on_noise.items()},
                         state_cur_ms={k: [min(v), max(v)] for k, v in state.items()}, min_MB=min_mb,
                         label_GBps=round(5.0 * C * H * W / (device["label"] * 1e-3) / 1e9, 1), scratch_MB=round(seg.scratch_bytes / 1e6, 1)))
        del seg, env_ids, env_color
    line = json.dumps(dict(bench="segment", device=torch.cuda.get_device_name(0), tile=[segment.TILE_H, segment.TILE_W], reps=args.reps, inner=args.inner,
                           scipy=None if ndi is None else __import__("scipy").__version__, rows=rows))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


def _lib_label(seg, mask, labels, count, connectivity=8):
    """ag_segment_label into given outputs: the call alone, without `label`'s two allocations."""
    from adaptigraph_amd import _lib
    C, H, W = (int(z) for z in mask.shape)
    _lib.call("ag_segment_label", seg.device, mask, C, H, W, connectivity, seg.scratch, seg.scratch_bytes, labels, count)


if __name__ == "__main__":
    main()
