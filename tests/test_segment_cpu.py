"""The statement of adaptigraph_amd.segment, without a GPU: the integer HSV, the colour keys, the morphology, the labelling and what is built on
it, each against a definition written out here in loops and, where scipy imports, against scipy.ndimage; and SimEnv(masks="color") on the host
path against masks="ids"."""
import numpy as np
import pytest

from adaptigraph_amd import render, segment, viz
import segment_cases as sc
import viz_cases


# ------------------------------------------------------------------------------------------------------------------ colour
def hsv_python(r, g, b):
    """The issue's formula with Python integers (`//` floors)."""
    mx, mn = max(r, g, b), min(r, g, b)
    d = mx - mn
    s = 0 if mx == 0 else (255 * d + mx // 2) // mx
    if d == 0:
        h = 0
    elif mx == r:
        h = ((60 * (g - b) + d // 2) // d) % 360
    elif mx == g:
        h = ((60 * (b - r) + d // 2) // d + 120) % 360
    else:
        h = ((60 * (r - g) + d // 2) // d + 240) % 360
    return h, s, mx


def test_hsv_of_known_colours():
    hsv = lambda *rgb: tuple(int(z) for z in segment.hsv_host(np.array(rgb, np.uint8)))      # noqa: E731
    assert [hsv(255, 0, 0)[0], hsv(0, 255, 0)[0], hsv(0, 0, 255)[0]] == [0, 120, 240]
    assert hsv(255, 0, 0) == (0, 255, 255)
    for v in (1, 77, 128, 255):
        assert hsv(v, v, v) == (0, 0, v)
    assert hsv(0, 0, 0) == (0, 0, 0)
    assert hsv(*sc.rgb_of(viz.TABLE_COLOR)) == (240, 11, 115) and hsv(*sc.rgb_of(viz.VOID_COLOR)) == (0, 0, 0)
    palette = [hsv(*sc.rgb_of(c)) for c in viz.PALETTE]
    assert palette == [(40, 73, 216), (39, 84, 201), (40, 63, 227), (39, 93, 189)]
    assert all(39 <= h <= 40 and 63 <= s <= 93 for h, s, _ in palette)


def test_hsv_floors_a_negative_numerator():
    """(10, 20, 200): the blue branch, numerator 60 (10 - 20) + 95 = -505 over 190: floor -3, truncation -2."""
    assert (60 * (10 - 20) + 95) // 190 == -3 and int((60 * (10 - 20) + 95) / 190) == -2
    assert tuple(segment.hsv_host(np.array([10, 20, 200], np.uint8))) == hsv_python(10, 20, 200) == (237, 242, 200)
    # (200, 10, 190): the red branch, numerator 60 (10 - 190) + 95 = -10 705 over 190: floor -57, truncation -56
    assert (60 * (10 - 190) + 95) // 190 == -57 and int((60 * (10 - 190) + 95) / 190) == -56
    assert tuple(segment.hsv_host(np.array([200, 10, 190], np.uint8))) == hsv_python(200, 10, 190) == (303, 242, 200)


def test_hsv_equals_the_formula_on_random_colours():
    img = sc.random_images(1, 40, 50, 4)[0]
    got = segment.hsv_host(img)
    assert got.dtype == np.int32 and got.shape == (40, 50, 3)
    want = np.array([[hsv_python(*(int(z) for z in px[:3])) for px in row] for row in img])
    assert np.array_equal(got, want)


def test_color_keys():
    img = sc.random_images(2, 30, 40, 3)
    hsv = segment.hsv_host(img)
    wrap = segment.ColorKey(330, 20, 10, 255, 10, 255)
    want = ((hsv[..., 0] >= 330) | (hsv[..., 0] <= 20)) & (hsv[..., 1] >= 10) & (hsv[..., 2] >= 10)
    got = segment.color_mask(img, [wrap])
    assert got.dtype == bool and np.array_equal(got, want) and want.any() and not want.all()
    assert np.array_equal(segment.color_mask(img, wrap), want)      # one key, not in a list
    for n, keys in sc.KEY_SETS.items():
        assert len(keys) == n
        assert np.array_equal(segment.color_mask(img, keys), np.any([segment.color_mask_host(img, [k]) for k in keys], 0))
    assert not segment.color_mask(img, []).any()
    exact = segment.ColorKey.exact(viz.TABLE_COLOR)
    assert exact == segment.ColorKey(240, 240, 11, 11, 115, 115) == segment.ColorKey.exact(sc.rgb_of(viz.TABLE_COLOR))
    # the table is separable from the particles and from the void by the exact key and by the loose grey key
    flat = np.array([sc.rgb_of(c) for c in (viz.TABLE_COLOR, viz.VOID_COLOR) + tuple(viz.PALETTE)], np.uint8)[None]
    for keys in (sc.TABLE_KEYS, sc.GREY_KEYS):
        assert segment.color_mask(flat, keys)[0].tolist() == [True, False, False, False, False, False]
    assert np.array_equal(segment.color_mask(img[0], [wrap]), want[0])      # a single image goes in and comes out without the leading axis


# ------------------------------------------------------------------------------------------------------------------ labelling
def flood_labels(mask, connectivity):
    """A stack-based fill started at every unvisited foreground pixel in raster order, numbered in that order."""
    H, W = mask.shape
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    labels = np.zeros((H, W), np.int32)
    m = mask.tolist()
    lab = labels.tolist()
    count = 0
    for y in range(H):
        for x in range(W):
            if m[y][x] and not lab[y][x]:
                count += 1
                lab[y][x] = count
                stack = [(y, x)]
                while stack:
                    cy, cx = stack.pop()
                    for dy, dx in steps:
                        ny, nx = cy + dy, cx + dx
                        if 0 <= ny < H and 0 <= nx < W and m[ny][nx] and not lab[ny][nx]:
                            lab[ny][nx] = count
                            stack.append((ny, nx))
    return np.array(lab, np.int32).reshape(H, W), count


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_label_host_against_a_flood_fill(size, connectivity):
    names, masks = sc.stack(*size)
    labels, count = sc.host_labels(*size, connectivity)
    assert labels.dtype == np.int32 and count.dtype == np.int32 and labels.shape == masks.shape and count.shape == (len(names),)
    for i, name in enumerate(names):
        want, n = flood_labels(masks[i], connectivity)
        assert count[i] == n and np.array_equal(labels[i], want), name
    H, W = size
    board = names.index("checkerboard")
    assert count[board] == ((H * W + 1) // 2 if connectivity == 4 or min(H, W) == 1 else 1)
    if H > 3 and W > 3:
        assert count[names.index("corner_main")] == count[names.index("corner_anti")] == (1 if connectivity == 8 else 2)
        assert count[names.index("serpentine")] == 1
        for comb in ("comb_last_row", "comb_first_row", "comb_last_column", "comb_first_column"):
            assert count[names.index(comb)] == 1, comb
    assert count[names.index("empty")] == 0 and count[names.index("full")] == 1


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_label_host_against_scipy(size, connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    names, masks = sc.stack(*size)
    labels, count = sc.host_labels(*size, connectivity)
    structure = np.ones((3, 3), int) if connectivity == 8 else ndi.generate_binary_structure(2, 1)
    for i, name in enumerate(names):
        want, n = ndi.label(masks[i], structure)
        assert count[i] == n and np.array_equal(labels[i], want), name


def test_label_of_a_single_image_and_a_stack():
    names, masks = sc.stack(90, 160)
    labels, count = sc.host_labels(90, 160, 8)
    one, n = segment.label(masks[3], 8)
    assert one.shape == (90, 160) and n.shape == (1,) and np.array_equal(one, labels[3]) and n[0] == count[3]
    three = np.stack([masks[names.index("random_0.59")], masks[names.index("empty")], masks[names.index("rings")]])
    got, cnt = segment.label(three.astype(np.uint8) * 255, 8)      # uint8, non-zero = set; numbering restarts in every image
    for k, name in enumerate(("random_0.59", "empty", "rings")):
        assert np.array_equal(got[k], labels[names.index(name)]) and cnt[k] == count[names.index(name)]


# ------------------------------------------------------------------------------------------------------------------ morphology
def erode_loops(m, r):
    H, W = m.shape
    out = np.zeros_like(m)
    for y in range(H):
        for x in range(W):
            out[y, x] = y - r >= 0 and y + r < H and x - r >= 0 and x + r < W and m[y - r:y + r + 1, x - r:x + r + 1].all()
    return out


def dilate_loops(m, r):
    H, W = m.shape
    out = np.zeros_like(m)
    for y in range(H):
        for x in range(W):
            out[y, x] = m[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1].any()
    return out


MORPH_SIZES = [(1, 1), (1, sc.TW + 1), (sc.TH + 1, 1), (sc.TH - 1, sc.TW - 1), (sc.TH + 1, sc.TW + 1)]


@pytest.mark.parametrize("size", MORPH_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_morphology_against_the_loop_definitions(size):
    H, W = size
    for r in (0, 1, 2, segment.MAX_RADIUS):
        for d in sc.DENSITIES + (1.0,):
            m = sc.random_mask(H, W, d) if d < 1 else np.ones((H, W), bool)
            e, di = erode_loops(m, r), dilate_loops(m, r)
            assert np.array_equal(segment.erode(m, r), e) and np.array_equal(segment.dilate(m, r), di), (r, d)
            assert np.array_equal(segment.opening(m, r), dilate_loops(e, r)) and np.array_equal(segment.closing(m, r), erode_loops(di, r)), (r, d)
            if r == 0:
                assert np.array_equal(e, m) and np.array_equal(di, m)
        full = segment.erode(np.ones((H, W), bool), r)      # the border convention: erosion eats r pixels of the image border
        want = np.zeros((H, W), bool)
        if H > 2 * r and W > 2 * r:
            want[r:H - r, r:W - r] = True
        assert np.array_equal(full, want) and full.sum() == max(H - 2 * r, 0) * max(W - 2 * r, 0)


def test_morphology_and_holes_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for H, W in ((sc.TH + 1, sc.TW + 1), (33, 47)):
        for d in sc.DENSITIES:
            m = sc.random_mask(H, W, d)
            for r in (0, 1, 2, 5):
                st = np.ones((2 * r + 1, 2 * r + 1), bool)
                for ours, theirs in ((segment.erode, ndi.binary_erosion), (segment.dilate, ndi.binary_dilation), (segment.opening, ndi.binary_opening),
                                     (segment.closing, ndi.binary_closing)):
                    assert np.array_equal(ours(m, r), theirs(m, structure=st)), (ours.__name__, r, d)
            assert np.array_equal(segment.fill_holes(m), ndi.binary_fill_holes(m))
            assert np.array_equal(segment.fill_holes(m, 4), ndi.binary_fill_holes(m, structure=np.ones((3, 3), bool)))
    m = sc.rings(33, 47)
    assert np.array_equal(segment.fill_holes(m), ndi.binary_fill_holes(m))


def fill_loops(m, connectivity):
    """The background components, under the dual connectivity, none of whose pixels lies on the image border."""
    bg, n = flood_labels(~m, 4 if connectivity == 8 else 8)
    out = m.copy()
    for k in range(1, n + 1):
        ys, xs = np.nonzero(bg == k)
        if ys.min() > 0 and xs.min() > 0 and ys.max() < m.shape[0] - 1 and xs.max() < m.shape[1] - 1:
            out[ys, xs] = True
    return out


@pytest.mark.parametrize("connectivity", [4, 8])
def test_fill_holes_against_the_definition(connectivity):
    for H, W in ((1, 1), (sc.TH + 1, sc.TW + 1), (2 * sc.TH + 1, 3 * sc.TW - 1)):
        c = sc.contents(H, W)
        for name in ("rings", "checkerboard", "spiral", "random_0.41", "random_0.59", "random_0.9", "empty", "full"):
            assert np.array_equal(segment.fill_holes(c[name], connectivity), fill_loops(c[name], connectivity)), (name, H, W)
    filled = segment.fill_holes(sc.rings(20, 30))
    assert filled.all()      # the outermost ring lies on the border: everything inside it is a hole
    assert not segment.fill_holes(np.zeros((5, 5), bool)).any()


# ------------------------------------------------------------------------------------------------------------------ table, selection
@pytest.mark.parametrize("connectivity", [4, 8])
def test_components_against_bincount_and_nonzero(connectivity):
    H, W = 2 * sc.TH + 1, 3 * sc.TW - 1
    names, masks = sc.stack(H, W)
    labels, count = sc.host_labels(H, W, connectivity)
    cap = int(count.max())
    table, got_count = segment.components(labels, count, cap)
    assert table.shape == (len(names), cap, 8) and table.dtype == np.int64 and np.array_equal(got_count, count)
    for i, name in enumerate(names):
        n = int(count[i])
        assert not table[i, n:].any(), name
        assert np.array_equal(table[i, :n, 0], np.bincount(labels[i].ravel(), minlength=n + 1)[1:]), name
        for k in range(1, min(n, 40) + 1):
            ys, xs = np.nonzero(labels[i] == k)
            border = int(ys.min() == 0 or xs.min() == 0 or ys.max() == H - 1 or xs.max() == W - 1)
            assert table[i, k - 1].tolist() == [len(ys), xs.min(), ys.min(), xs.max(), ys.max(), xs.sum(), ys.sum(), border], (name, k)
    ring = names.index("rings")
    assert table[ring, :count[ring], 7].tolist() == [1] + [0] * (int(count[ring]) - 1)      # only the outermost ring touches the border
    # truncation: fewer rows than components, the true count returned
    i = names.index("random_0.1")
    small, cnt = segment.components(labels[i], count[i:i + 1], 5)
    assert count[i] > 5 and small.shape == (5, 8) and cnt[0] == count[i] and np.array_equal(small, table[i, :5])
    with pytest.raises(ValueError):
        segment.components(labels, count, 0)


def test_select():
    m = np.zeros((12, 20), bool)
    m[1:3, 1:4] = True       # label 1, area 6
    m[5:7, 1:4] = True       # label 3, area 6  (raster order: the block at columns 10.. starts in row 4)
    m[4:9, 10:14] = True     # label 2, area 20
    m[10, 18] = True         # label 4, area 1
    labels, count = segment.label(m)
    assert count[0] == 4 and labels[1, 1] == 1 and labels[4, 10] == 2 and labels[5, 1] == 3 and labels[10, 18] == 4
    assert np.array_equal(segment.select(m), m)
    assert np.array_equal(segment.select(m, min_area=6), m & (labels != 4))          # exactly a component's area keeps it
    assert np.array_equal(segment.select(m, min_area=7), labels == 2)                # one above drops it
    assert np.array_equal(segment.select(m, keep_largest=1), labels == 2)
    assert np.array_equal(segment.select(m, keep_largest=2), (labels == 2) | (labels == 1))      # equal areas: the lower label
    assert np.array_equal(segment.select(m, keep_largest=3), m & (labels != 4))
    assert np.array_equal(segment.select(m, keep_largest=8), m)                      # more than there are: all
    assert np.array_equal(segment.select(m, min_area=2, keep_largest=8), m & (labels != 4))
    assert not segment.select(m, min_area=21).any()
    # any number of components: a checkerboard under 4-connectivity, every component of area 1
    board = sc.contents(sc.TH + 1, sc.TW + 1)["checkerboard"]
    assert np.array_equal(segment.select(board, min_area=1, connectivity=4), board) and not segment.select(board, min_area=2, connectivity=4).any()
    kept = segment.select(board, keep_largest=3, connectivity=4)
    assert kept.sum() == 3 and kept[0, 0] and kept[0, 2] and kept[0, 4]
    assert np.array_equal(segment.select(board, keep_largest=1, connectivity=8), board)


def test_keep_mask_is_the_reference_expression():
    names, masks = sc.stack(2 * sc.TH + 1, 3 * sc.TW - 1)
    pick = lambda *n: np.stack([masks[names.index(x)] for x in n])      # noqa: E731
    table, a, b = pick("random_0.9", "full", "rings"), pick("rings", "random_0.1", "empty"), pick("corner_main", "random_0.41", "points")
    img = sc.painted(table, a, b)
    t_mask = table & ~a & ~b
    assert np.array_equal(segment.color_mask(img, sc.TABLE_KEYS), t_mask) and np.array_equal(segment.color_mask(img, sc.GREY_KEYS), t_mask)
    assert np.array_equal(segment.color_mask(img, sc.OBJECT_KEYS), a | b)
    assert np.array_equal(segment.keep_mask(img, sc.TABLE_KEYS), ~t_mask)
    kw = dict(open_radius=1, close_radius=2, min_area=4, keep_largest=3, connectivity=4)
    chain = lambda m: segment.select(segment.closing(segment.opening(m, 1), 2), 4, 3, 4)      # noqa: E731
    t, o = chain(t_mask), segment.fill_holes(chain(a | b), 4)
    got = segment.keep_mask(img, sc.TABLE_KEYS, sc.OBJECT_KEYS, fill=True, **kw)
    assert got.dtype == bool and got.shape == table.shape and np.array_equal(got, ~(t & ~o))
    assert np.array_equal(segment.keep_mask(img, sc.TABLE_KEYS, sc.OBJECT_KEYS, **kw), ~(t & ~chain(a | b)))
    assert np.array_equal(segment.keep_mask(img[0, ..., :3], sc.GREY_KEYS), ~t_mask[0])


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_raise_value_error():
    m = np.zeros((4, 5), bool)
    img = np.zeros((1, 4, 5, 3), np.uint8)
    for fn in (segment.erode, segment.dilate, segment.opening, segment.closing):
        with pytest.raises(ValueError):
            fn(m, segment.MAX_RADIUS + 1)
        with pytest.raises(ValueError):
            fn(m, -1)
    for k in (0, 9, -1):
        with pytest.raises(ValueError):
            segment.select(m, keep_largest=k)
        with pytest.raises(ValueError):
            segment.keep_mask(img, sc.TABLE_KEYS, keep_largest=k)
    for c in (6, 0, 1, None):
        for fn in (segment.label, segment.fill_holes):
            with pytest.raises(ValueError):
                fn(m, c)
        with pytest.raises(ValueError):
            segment.select(m, connectivity=c)
        with pytest.raises(ValueError):
            segment.keep_mask(img, sc.TABLE_KEYS, connectivity=c)
    with pytest.raises(ValueError):
        segment.color_mask(img, [segment.ColorKey()] * 9)
    with pytest.raises(ValueError):
        segment.keep_mask(img, sc.TABLE_KEYS, open_radius=segment.MAX_RADIUS + 1)
    for bad in (img.astype(np.float32), img.astype(np.int32), np.zeros((4, 5), np.uint8), np.zeros((1, 4, 5, 2), np.uint8), np.zeros((1, 1, 4, 5, 3), np.uint8)):
        with pytest.raises(ValueError):
            segment.color_mask(bad, sc.TABLE_KEYS)
        with pytest.raises(ValueError):
            segment.keep_mask(bad, sc.TABLE_KEYS)
    for bad in (np.zeros((4, 5), np.float32), np.zeros((4, 5), np.int32), np.zeros(5, bool), np.zeros((1, 1, 4, 5), bool)):
        with pytest.raises(ValueError):
            segment.label(bad)
    assert segment.MAX_RADIUS >= 8 and (segment.TILE_H, segment.TILE_W) == (sc.TH, sc.TW)


def test_sim_env_refuses_an_unknown_masks_value():
    from adaptigraph_amd import configs, sim
    from adaptigraph_amd.sim_env import SimEnv
    i = np.arange(8)
    rope = np.stack([0.09 * i, np.full(8, sim.DEFAULT.r), 0.0 * i], 1).astype(np.float32)
    scene = sim.RopeScene.from_ropes([rope], stiffness=[0.5])
    with pytest.raises(ValueError, match="masks"):
        SimEnv("rope", scene, configs.task_config("rope"), None, None, masks="colour")
    env = SimEnv("rope", scene, configs.task_config("rope"), None, None, image_size=(24, 40), masks="color")
    assert env.masks == "color" and env.table_keys == [segment.ColorKey.exact(viz.TABLE_COLOR)]
    obs = env.get_obs()
    assert np.array_equal(obs["mask_0"][0], env.last_ids[0] != render.ID_PLANE) and "color_0" not in obs
    grey = SimEnv("rope", scene, configs.task_config("rope"), None, None, image_size=(24, 40), masks="color", table_keys=sc.GREY_KEYS)
    assert np.array_equal(grey.get_obs(get_color=True)["mask_1"], obs["mask_1"])


# ------------------------------------------------------------------------------------------------------------------ the closed loop's eyes
@pytest.mark.parametrize("make", [viz_cases.rope_env, viz_cases.box_env], ids=["rope", "box"])
def test_sim_env_sees_with_its_colour_images_on_the_host(make):
    by_ids, by_color = make(None), make(None)
    by_color.masks, by_color.table_keys = "color", sc.TABLE_KEYS      # (viz_cases builds the default environment)
    from adaptigraph_amd.sim_env import SimEnv
    assert SimEnv.__init__.__kwdefaults__["masks"] == "ids" and by_ids.masks == "ids"
    obs_ids, obs_color = by_ids.get_obs(), by_color.get_obs()
    assert "color_0" not in obs_color
    _, ids = by_ids.render()
    for i in range(len(by_ids.R_list)):
        mask = obs_color[f"mask_{i}"]
        assert mask.dtype == bool and mask.shape == (1, 90, 160)
        assert np.array_equal(mask[0], ids[i] != render.ID_PLANE)
        assert np.array_equal(obs_ids[f"mask_{i}"][0], ids[i] >= 0)
        assert np.array_equal(mask[0] & (ids[i] != render.ID_NONE), ids[i] >= 0)      # they differ on the void only
        assert np.array_equal(obs_color[f"depth_{i}"], obs_ids[f"depth_{i}"])
    assert (ids >= 0).any() and (ids == render.ID_PLANE).any()
    states = []
    for env in (by_ids, by_color):
        np.random.seed(3)
        states.append(env.get_state_cur(0.1, 40))
    assert states[0].shape[0] > 3 and np.array_equal(states[0], states[1])
    # the loose grey key sees the same
    by_color.table_keys = sc.GREY_KEYS
    np.random.seed(3)
    assert np.array_equal(by_color.get_state_cur(0.1, 40), states[0])
