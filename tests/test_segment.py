"""csrc/ag_segment.hip against the statement of adaptigraph_amd.segment, bit for bit: every content of segment_cases at every size and both
connectivities in one call per size, the colour keys, the morphology at the border, selection, holes, the keep rule end to end, a captured graph,
the error codes of the C ABI, and SimEnv(masks="color") against masks="ids"."""
import ctypes

import numpy as np
import pytest
import torch

from adaptigraph_amd import _lib, render, segment
import segment_cases as sc
from viz_cases import SeededEnv, StubPlanner, box_env, rope_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZE_IDS = [f"{h}x{w}" for h, w in sc.SIZES]


def up(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared cases are read-only)


def same(t, a):
    return np.array_equal(t.cpu().numpy(), np.asarray(a))


# ------------------------------------------------------------------------------------------------------------------ labelling
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("size", sc.SIZES, ids=SIZE_IDS)
def test_labels_counts_and_components_equal_the_statement(size, connectivity):
    names, masks = sc.stack(*size)
    want, want_count = sc.host_labels(*size, connectivity)
    seg = segment.DeviceSegmenter(len(names), *size, DEV)
    labels, count = seg.label(up(masks), connectivity)
    assert labels.dtype == torch.int32 and count.dtype == torch.int32 and count.is_cuda
    got, got_count = labels.cpu().numpy(), count.cpu().numpy()
    for i, name in enumerate(names):
        assert got_count[i] == want_count[i] and np.array_equal(got[i], want[i]), name
    cap = max(int(want_count.max()), 1)
    table, count2 = seg.components(labels, count, cap)
    want_table, _ = segment.components_host(want, want_count, cap)
    assert table.dtype == torch.int64 and torch.equal(count2, count)
    got_table = table.cpu().numpy()
    for i, name in enumerate(names):
        assert np.array_equal(got_table[i], want_table[i]), name
    small = max(cap // 2, 1)      # truncation: rows up to min(count, max_labels), the true count returned
    table, count2 = seg.components(labels, count, small)
    assert same(table, segment.components_host(want, want_count, small)[0]) and same(count2, want_count)


def test_thin_functions_take_the_device():
    names, masks = sc.stack(sc.TH + 1, sc.TW + 1)
    three = np.stack([masks[names.index(n)] for n in ("random_0.59", "empty", "spiral")])      # three contents in one call, one of them empty
    want, want_count = segment.label(three, 4)
    labels, count = segment.label(three, 4, device=DEV)
    assert labels.is_cuda and count.is_cuda and same(labels, want) and same(count, want_count)
    one, n = segment.label(up(three[2]), 4, device=DEV)
    assert one.shape == three[2].shape and same(one, want[2]) and int(n[0]) == want_count[2]
    table, cnt = segment.components(labels, count, 7, device=DEV)
    assert same(table, segment.components(want, want_count, 7)[0]) and same(cnt, want_count)
    for fn, args in ((segment.erode, (1,)), (segment.dilate, (2,)), (segment.opening, (1,)), (segment.closing, (1,)), (segment.fill_holes, (4,)),
                     (segment.select, (3, 2, 4))):
        got = fn(three, *args, device=DEV)
        assert got.dtype == torch.bool and same(got, fn(three, *args)), fn.__name__


def test_one_large_image_against_scipy():
    """720 x 1280 at the 4-connected percolation density: components that span hundreds of tiles (test_segment_cpu.py ties scipy's numbering to
    the statement)."""
    ndi = pytest.importorskip("scipy.ndimage")
    H, W = 720, 1280
    m = np.random.default_rng(59).random((1, H, W, 4)) < 0.59      # (four planes: an RGBA image's worth of bytes)
    m = m[..., 0]
    seg = segment.DeviceSegmenter(1, H, W, DEV)
    for connectivity, structure in ((4, None), (8, np.ones((3, 3), int))):
        want, n = ndi.label(m[0], structure)
        labels, count = seg.label(up(m), connectivity)
        assert int(count[0]) == n and same(labels[0], want), connectivity
        table, _ = seg.components(labels, count, 64)
        assert same(table[0, :, 0], np.bincount(want.ravel(), minlength=65)[1:65])


# ------------------------------------------------------------------------------------------------------------------ colour, morphology
@pytest.mark.parametrize("size", sc.SIZES, ids=SIZE_IDS)
def test_color_mask_equals_the_statement(size):
    seg = segment.DeviceSegmenter(3, *size, DEV)
    for channels in (3, 4):
        img = sc.random_images(3, *size, channels)
        for n, keys in sc.KEY_SETS.items():
            got = seg.color_mask(up(img), keys)
            assert got.dtype == torch.uint8 and same(got, segment.color_mask_host(img, keys)), (channels, n)
    assert not seg.color_mask(up(img), []).any()


def test_color_mask_floors_negative_hue_numerators():
    colours = np.array([[10, 20, 200], [200, 10, 190], [200, 20, 200], [255, 0, 1], [254, 0, 255], [3, 2, 1], [1, 2, 3], [0, 0, 0], [255, 255, 255]], np.uint8)
    img = np.ascontiguousarray(colours[None, None])      # (1, 1, n, 3)
    hsv = segment.hsv_host(colours)
    for k, (h, s, v) in enumerate(hsv.tolist()):
        got = segment.color_mask(img, [segment.ColorKey(h, h, s, s, v, v)], device=DEV)
        assert same(got, segment.color_mask_host(img, [segment.ColorKey(h, h, s, s, v, v)])) and bool(got[0, 0, k])
    assert hsv[0, 0] == 237 and hsv[1, 0] == 303


@pytest.mark.parametrize("size", sc.SIZES, ids=SIZE_IDS)
def test_morphology_equals_the_statement(size):
    H, W = size
    masks = np.stack([sc.random_mask(H, W, d) for d in sc.DENSITIES] + [np.ones((H, W), bool)])
    seg = segment.DeviceSegmenter(len(masks), H, W, DEV)
    dev = up(masks)
    for r in (0, 1, 2, segment.MAX_RADIUS):
        for op, host in (("erode", segment.erode_host), ("dilate", segment.dilate_host), ("opening", segment.opening_host), ("closing", segment.closing_host)):
            assert same(seg.morph(op, dev, r), host(masks, r)), (op, r)
        full = seg.morph("erode", dev, r)[-1].cpu().numpy()      # the border convention
        want = np.zeros((H, W), np.uint8)
        if H > 2 * r and W > 2 * r:
            want[r:H - r, r:W - r] = 1
        assert np.array_equal(full, want)
    assert torch.equal(seg.morph("dilate", dev, 0), dev.view(torch.uint8))
    again = dev.view(torch.uint8).clone()
    seg.morph("closing", again, 2, out=again)      # in place
    assert same(again, segment.closing_host(masks, 2))


# ------------------------------------------------------------------------------------------------------------------ selection, holes, keep rule
PICKED = ("rings", "checkerboard", "random_0.1", "random_0.41", "random_0.59", "random_0.9", "spiral", "empty", "full", "corner_anti")


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("size", [(sc.TH + 1, sc.TW + 1), (2 * sc.TH + 1, 3 * sc.TW - 1), (90, 160)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_select_and_fill_holes_equal_the_statement(size, connectivity):
    names, all_masks = sc.stack(*size)
    masks = np.stack([all_masks[names.index(n)] for n in PICKED])
    seg = segment.DeviceSegmenter(len(masks), *size, DEV)
    dev = up(masks)
    assert same(seg.fill_holes(dev, connectivity), segment.fill_holes_host(masks, connectivity))
    for min_area, k in ((0, None), (1, None), (2, None), (5, None), (0, 1), (0, 3), (0, 8), (3, 2), (10 ** 6, 4)):
        assert same(seg.select(dev, min_area, k, connectivity), segment.select_host(masks, min_area, k, connectivity)), (min_area, k)


def test_select_orders_equal_areas_by_label():
    m = np.zeros((1, 12, 20), bool)
    m[0, 1:3, 1:4] = m[0, 5:7, 1:4] = m[0, 10, 15:20] = True      # areas 6, 6, 5 ...
    m[0, 10, 14] = True                                              # ... 6: three of a kind
    seg = segment.DeviceSegmenter(1, 12, 20, DEV)
    for k in range(1, 5):
        got = seg.select(up(m), 0, k)
        assert same(got, segment.select_host(m, 0, k)) and int(got.sum()) == 6 * min(k, 3)


@pytest.mark.parametrize("channels", [3, 4])
def test_keep_mask_end_to_end(channels):
    size = (2 * sc.TH + 1, 3 * sc.TW - 1)
    names, masks = sc.stack(*size)
    pick = lambda *n: np.stack([masks[names.index(x)] for x in n])      # noqa: E731
    img = sc.painted(pick("random_0.9", "full", "rings", "random_0.59"), pick("rings", "random_0.1", "empty", "checkerboard"),
                     pick("corner_main", "random_0.41", "points", "spiral"), channels)
    seg = segment.DeviceSegmenter(4, *size, DEV)
    for kw in (dict(), dict(open_radius=1), dict(close_radius=2, min_area=4), dict(open_radius=1, close_radius=1, min_area=3, keep_largest=3, connectivity=4),
               dict(keep_largest=2)):
        for objects in (None, sc.OBJECT_KEYS):
            for fill in ((False, True) if objects else (False,)):
                want = segment.keep_mask_host(img, sc.TABLE_KEYS, objects, fill=fill, **kw)
                got = seg.keep_mask(up(img), sc.TABLE_KEYS, objects, fill=fill, **kw)
                assert got.dtype == torch.bool and same(got, want), (kw, objects is not None, fill)
    want = segment.keep_mask_host(img, sc.GREY_KEYS, sc.OBJECT_KEYS, fill=True, min_area=2)
    assert same(segment.keep_mask(img, sc.GREY_KEYS, sc.OBJECT_KEYS, fill=True, min_area=2, device=DEV), want)
    assert same(segment.keep_mask(up(img[0]), sc.GREY_KEYS, sc.OBJECT_KEYS, fill=True, min_area=2, device=DEV), want[0])


def test_one_segmenter_for_a_large_image_then_a_small_one():
    big, small = sc.random_mask(90, 160, 0.59)[None], sc.random_mask(sc.TH - 1, sc.TW + 3, 0.59)[None]
    seg = segment.DeviceSegmenter(2, 90, 160, DEV)
    first = [t.clone() for t in seg.label(up(big), 8)] + [seg.select(up(big), 3, 2).clone(), seg.fill_holes(up(big)).clone()]
    for _ in range(2):      # the small one after the large one; and the same bits twice
        labels, count = seg.label(up(small), 8)
        want, n = segment.label_host(small, 8)
        assert same(labels, want) and same(count, n)
        assert same(seg.select(up(small), 3, 2), segment.select_host(small, 3, 2)) and same(seg.fill_holes(up(small)), segment.fill_holes_host(small))
    again = list(seg.label(up(big), 8)) + [seg.select(up(big), 3, 2), seg.fill_holes(up(big))]
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert same(first[0], segment.label_host(big, 8)[0])
    with pytest.raises(ValueError):
        seg.label(up(np.zeros((3, 4, 5), bool)))            # more images than it holds
    with pytest.raises(ValueError):
        seg.label(up(np.zeros((1, 91, 160), bool)))         # more pixels than it holds
    with pytest.raises(ValueError):
        seg.label(np.zeros((1, 4, 5), bool))                # not on the device


def test_select_and_fill_holes_in_place_and_a_device_without_an_index():
    names, masks = sc.stack(2 * sc.TH + 1, 3 * sc.TW - 1)
    m = np.stack([masks[names.index(n)] for n in ("random_0.41", "rings", "random_0.9")])
    seg = segment.DeviceSegmenter(3, *m.shape[1:], "cuda")      # tensors report cuda:0
    assert seg.device == torch.device(DEV)
    a, b = up(m).view(torch.uint8), up(m).view(torch.uint8)
    assert seg.select(a, 3, 2, 4, out=a) is a and same(a, segment.select_host(m, 3, 2, 4))
    assert seg.fill_holes(b, 8, out=b) is b and same(b, segment.fill_holes_host(m, 8))


def test_keep_mask_captures_into_a_graph():
    """Nothing is read back, and every per-call word is written again by the call itself: three inputs through the same buffers."""
    size = (2 * sc.TH + 1, 3 * sc.TW - 1)
    names, masks = sc.stack(*size)
    pick = lambda *n: np.stack([masks[names.index(x)] for x in n])      # noqa: E731
    contents = [sc.painted(pick("random_0.9", "full"), pick("rings", "random_0.1"), pick("corner_main", "random_0.41")),
                sc.painted(pick("random_0.59", "rings"), pick("checkerboard", "empty"), pick("spiral", "points")),
                sc.painted(pick("empty", "random_0.41"), pick("full", "serpentine"), pick("empty", "random_0.1"))]
    kw = dict(open_radius=1, close_radius=1, min_area=3, keep_largest=4, fill=True)
    seg = segment.DeviceSegmenter(2, *size, DEV)
    images = up(contents[0])
    seg.keep_mask(images, sc.TABLE_KEYS, sc.OBJECT_KEYS, **kw)      # warm up: the first launch loads the code object
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = seg.keep_mask(images, sc.TABLE_KEYS, sc.OBJECT_KEYS, **kw)
    for i in (1, 2, 0):
        images.copy_(up(contents[i]))
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, segment.keep_mask_host(contents[i], sc.TABLE_KEYS, sc.OBJECT_KEYS, **kw)), i


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_error_codes_without_a_launch():
    L = _lib.lib()
    C, H, W = 1, 20, 30
    need = L.ag_segment_scratch_bytes(C, H, W)
    assert need >= 14 * C * H * W and L.ag_segment_scratch_bytes(0, H, W) == 0 and L.ag_segment_scratch_bytes(1, 65536, 65536) == 0
    buf = torch.zeros(need, dtype=torch.uint8, device=DEV)
    mask = torch.zeros((C, H, W), dtype=torch.uint8, device=DEV)
    labels, count = torch.full((C, H, W), -7, dtype=torch.int32, device=DEV), torch.full((C,), -7, dtype=torch.int32, device=DEV)
    out = torch.full((C, H, W), 9, dtype=torch.uint8, device=DEV)
    table = torch.full((C, 4, 8), -7, dtype=torch.int64, device=DEV)
    img = torch.zeros((C, H, W, 4), dtype=torch.uint8, device=DEV)
    keys = (ctypes.c_int32 * 6)(0, 359, 0, 255, 0, 255)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    m, s, lb, ct, o, tb, im = p(mask), p(buf), p(labels), p(count), p(out), p(table), p(img)
    ARG, WS = -1, -3
    calls = [
        # null pointers
        (ARG, b"null", lambda: L.ag_segment_label(None, C, H, W, 8, s, need, lb, ct, None)),
        (ARG, b"null", lambda: L.ag_segment_label(m, C, H, W, 8, None, need, lb, ct, None)),
        (ARG, b"null", lambda: L.ag_segment_label(m, C, H, W, 8, s, need, None, ct, None)),
        (ARG, b"null", lambda: L.ag_segment_label(m, C, H, W, 8, s, need, lb, None, None)),
        (ARG, b"null", lambda: L.ag_segment_color_mask(None, C, H, W, 4, keys, 1, o, None)),
        (ARG, b"null", lambda: L.ag_segment_color_mask(im, C, H, W, 4, None, 1, o, None)),
        (ARG, b"null", lambda: L.ag_segment_morph(m, C, H, W, 0, 1, s, need, None, None)),
        (ARG, b"null", lambda: L.ag_segment_components(lb, None, C, H, W, 4, tb, None)),
        (ARG, b"null", lambda: L.ag_segment_select(None, C, H, W, 8, 0, 0, s, need, o, None)),
        (ARG, b"null", lambda: L.ag_segment_fill_holes(m, C, H, W, 8, s, need, None, None)),
        (ARG, b"null", lambda: L.ag_segment_keep(None, None, C, H, W, o, None)),
        # H W beyond an int32 index
        (ARG, b"int32", lambda: L.ag_segment_label(m, C, 65536, 65536, 8, s, need, lb, ct, None)),
        (ARG, b"int32", lambda: L.ag_segment_color_mask(im, C, 65536, 32768, 4, keys, 1, o, None)),
        (ARG, b"int32", lambda: L.ag_segment_select(m, C, 46341, 46341, 8, 0, 0, s, need, o, None)),
        # a scratch smaller than the query
        (WS, b"ag_segment_scratch_bytes", lambda: L.ag_segment_label(m, C, H, W, 8, s, need - 1, lb, ct, None)),
        (WS, b"ag_segment_scratch_bytes", lambda: L.ag_segment_morph(m, C, H, W, 0, 1, s, need - 1, o, None)),
        (WS, b"ag_segment_scratch_bytes", lambda: L.ag_segment_select(m, C, H, W, 8, 0, 0, s, 0, o, None)),
        (WS, b"ag_segment_scratch_bytes", lambda: L.ag_segment_fill_holes(m, C, H, W, 8, s, need - 1, o, None)),
        # values out of range
        (ARG, b"connectivity", lambda: L.ag_segment_label(m, C, H, W, 6, s, need, lb, ct, None)),
        (ARG, b"radius", lambda: L.ag_segment_morph(m, C, H, W, 0, segment.MAX_RADIUS + 1, s, need, o, None)),
        (ARG, b"op", lambda: L.ag_segment_morph(m, C, H, W, 4, 1, s, need, o, None)),
        (ARG, b"keep_largest", lambda: L.ag_segment_select(m, C, H, W, 8, 0, 9, s, need, o, None)),
        (ARG, b"keys", lambda: L.ag_segment_color_mask(im, C, H, W, 4, keys, 9, o, None)),
        (ARG, b"channels", lambda: L.ag_segment_color_mask(im, C, H, W, 2, keys, 1, o, None)),
        (ARG, b"max_labels", lambda: L.ag_segment_components(lb, ct, C, H, W, 0, tb, None)),
        (ARG, b"C = 0", lambda: L.ag_segment_keep(m, None, 0, H, W, o, None)),
    ]
    for code, text, call in calls:
        assert call() == code and text in L.ag_last_error(), (text, L.ag_last_error())
    torch.cuda.synchronize()
    assert bool((labels == -7).all()) and bool((count == -7).all()) and bool((out == 9).all()) and bool((table == -7).all())      # no launch


# ------------------------------------------------------------------------------------------------------------------ the closed loop's eyes
def color_env(make, device):
    env = make(device)
    env.masks, env.table_keys = "color", sc.TABLE_KEYS      # (viz_cases builds the default environment; these are what masks="color" sets)
    return env


@pytest.mark.parametrize("make", [rope_env, box_env], ids=["rope", "box"])
def test_sim_env_sees_with_its_colour_images(make):
    by_ids, by_color, host = make(DEV), color_env(make, DEV), color_env(make, None)
    _, ids = by_ids.render()
    obs, obs_host = by_color.get_obs(), host.get_obs()
    for i in range(len(by_ids.R_list)):
        mask = obs[f"mask_{i}"]
        assert mask.is_cuda and mask.dtype == torch.bool and torch.equal(mask[0], ids[i] != render.ID_PLANE)
        assert same(mask, obs_host[f"mask_{i}"])
    assert bool((ids >= 0).any()) and bool((ids == render.ID_PLANE).any())
    states = []
    for env in (by_ids, by_color, host):
        np.random.seed(3)
        states.append(env.get_state_cur(0.1, 40))
    assert states[0].shape[0] > 3 and torch.equal(states[0], states[1]) and same(states[1], states[2])


def test_sim_env_masks_keyword_on_the_device():
    from adaptigraph_amd import configs, sim
    from adaptigraph_amd.sim_env import SimEnv
    from viz_cases import env_cameras
    i = np.arange(32)
    rope = np.stack([0.09 * (i - 15.5), np.full(32, sim.DEFAULT.r), 0.05 * np.sin(0.4 * i)], 1).astype(np.float32)
    scene = sim.RopeScene.from_ropes([rope], stiffness=[0.5])
    make = lambda **kw: SimEnv("rope", scene, configs.task_config("rope"), env_cameras(), DEV, image_size=(90, 160), stride=1, **kw)      # noqa: E731
    a, b, c = make(), make(masks="color"), make(masks="color", table_keys=sc.GREY_KEYS)
    assert a.masks == "ids" and b.table_keys == sc.TABLE_KEYS
    states = []
    for env in (a, b, c):
        np.random.seed(3)
        states.append(env.get_state_cur(0.1, 40))
    assert torch.equal(states[0], states[1]) and torch.equal(states[0], states[2])
    obs = b.get_obs(get_color=True)
    assert obs["color_0"].shape == (1, 90, 160, 3) and torch.equal(obs["mask_0"], c.get_obs()["mask_0"])
    kept = obs["mask_0"].clone()      # an observation owns its masks: the next one does not write into them
    black = b._segmenter.keep_mask(torch.zeros((4, 90, 160, 4), dtype=torch.uint8, device=DEV), b.table_keys)      # the buffer's next use
    assert bool(black.all()) and not bool(kept.all()) and torch.equal(obs["mask_0"], kept)
    assert b.get_obs()["mask_0"].data_ptr() != obs["mask_0"].data_ptr()


@pytest.mark.parametrize("make", [rope_env, box_env], ids=["rope", "box"])
def test_closed_loop_is_the_same_in_both_modes(make, tmp_path):
    from adaptigraph_amd.closed_loop import run_closed_loop
    lo, hi = torch.tensor([-1.0, -1.0, -3.14, 2.0]), torch.tensor([1.0, 1.0, 3.14, 4.0])
    criteria = lambda cloud: ((cloud - torch.tensor([0.0, 0.03, -0.5], device=cloud.device)) ** 2).sum(-1).mean()      # noqa: E731
    runs = []
    for name, env in (("ids", make(DEV)), ("color", color_env(make, DEV))):
        torch.manual_seed(0)
        np.random.seed(0)
        out = tmp_path / name
        acts, errors = run_closed_loop(SeededEnv(env), StubPlanner(), criteria, 2, 2, lo, hi, 0.2, save_dir=str(out))
        runs.append((acts.cpu(), errors, [dict(np.load(str(out / f"interaction_{i}.npz"))) for i in range(2)]))
    (a0, e0, r0), (a1, e1, r1) = runs
    assert torch.equal(a0, a1) and e0 == e1 and len(e0) == 3
    assert all(set(x) == set(y) and all(np.array_equal(x[k], y[k]) for k in x) for x, y in zip(r0, r1))
