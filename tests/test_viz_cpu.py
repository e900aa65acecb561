"""The drawing statement (adaptigraph_amd/viz.py:draw_host), the display lists, the PNG files and ag_draw's argument checks: no GPU."""
import ctypes
import itertools

import numpy as np
import pytest

from adaptigraph_amd import _lib, render, viz
from viz_cases import CAMS, H, W, StubPlanner, at_pixels, awkward_list, rope_env

WHITE = 0xFFFFFF


def one(kind, size, pixels, **kw):
    """One white primitive over black between the first and the last of `pixels` -> the covered mask."""
    img = viz.draw_host(at_pixels(pixels), [[0, len(pixels) - 1, 0, 0]], [[kind, size, 0, WHITE]], [[0, 0, 1, 0]], CAMS, H, W, **kw)
    assert img.shape == (1, H, W, 4) and img.dtype == np.uint8 and (img[..., 3] == 255).all()
    assert ((img[0, :, :, :3] == 255).all(-1) | (img[0, :, :, :3] == 0).all(-1)).all()
    return img[0, :, :, 0] == 255


def test_projection_lands_on_the_pixels_asked_for():
    px = [(0, 0), (W - 1, H - 1), (7, 3), (-3, -2), (W + 5, 2)]
    x, y, valid = viz.project_host(at_pixels(px), CAMS[0], 0.05)
    assert valid.all() and list(zip(x.tolist(), y.tolist())) == px


def test_hand_counts():
    assert [int(one(viz.DISC, r, [(12, 12)]).sum()) for r in (0, 1, 2, 5)] == [1, 5, 13, 81]
    assert [int(one(viz.SEGMENT, w, [(2, 3), (6, 3)]).sum()) for w in (1, 2)] == [5, 17]
    assert [int(one(viz.SEGMENT, w, [(2, 2), (6, 6)]).sum()) for w in (1, 2)] == [5, 17]
    assert [int(one(viz.SEGMENT, w, [(9, 9), (9, 9)]).sum()) for w in (1, 2)] == [1, 5]
    m = one(viz.SEGMENT, 1, [(2, 3), (6, 3)])
    assert m[3, 2:7].all() and m.sum() == 5
    m = one(viz.SEGMENT, 1, [(2, 2), (6, 6)])
    assert all(m[i, i] for i in range(2, 7))


def test_paint_order_blend_and_untouched_background():
    rng = np.random.default_rng(0)
    bg = rng.integers(0, 256, (1, H, W, 4), dtype=np.uint8)
    pts = at_pixels([(10, 10), (12, 10), (11, 10), (30, 5)])
    styles = [[0, 3, 0, 0x102030], [0, 3, 0, 0xA0B0C0], [0, 2, 1, 0x00FF40], [0, 2, 1, 0xFF0080]]
    prims = [[0, 0, 0, 0], [1, 1, 1, 0], [2, 2, 2, 0], [2, 2, 3, 0], [0, 0, 2, 0]]
    frames = [[0, 0, 5, 0]]
    px = lambda img, u, v: tuple(int(c) for c in img[0, v, u, :3])      # noqa: E731
    blend = lambda top, base, a: tuple((t * a + b * (256 - a) + 128) >> 8 for t, b in zip(top, base))      # noqa: E731
    for alpha in (0, 77, 128, 256):
        img = viz.draw_host(pts, prims, styles, frames, CAMS, H, W, alpha, 1, bg)
        assert np.array_equal(img[0, :, 20:, :3][:, :5], bg[0, :, 20:25, :3])                    # nothing drawn there: the background's bytes
        assert np.array_equal(img[0, 0], np.concatenate([bg[0, 0, :, :3], np.full((W, 1), 255, np.uint8)], 1))
        assert px(img, 7, 10) == (0x10, 0x20, 0x30)                                              # only the first disc
        assert px(img, 15, 10) == (0xA0, 0xB0, 0xC0)                                             # only the second
        # (11, 10): both opaque discs, the later one is the base; three overlay discs cover it, the last listed (index 4, centre (10, 10),
        # radius 2) wins
        assert px(img, 11, 10) == blend((0x00, 0xFF, 0x40), (0xA0, 0xB0, 0xC0), alpha)
        assert px(img, 13, 10) == blend((0xFF, 0x00, 0x80), (0xA0, 0xB0, 0xC0), alpha)           # overlay 3 is the last that covers (13, 10)
    assert px(viz.draw_host(pts, prims, styles, frames, CAMS, H, W, 0, 1, bg), 11, 10) == (0xA0, 0xB0, 0xC0)      # alpha 0: the base exactly
    assert px(viz.draw_host(pts, prims, styles, frames, CAMS, H, W, 256, 1, bg), 11, 10) == (0x00, 0xFF, 0x40)    # alpha 256: the top exactly


def test_accelerated_statement_is_the_plain_statement():
    pts, prims, styles = awkward_list(np.random.default_rng(1))
    frames = [[0, 0, len(prims), 0], [0, 10, 30, 0], [0, -5, 12, 0], [0, len(prims) - 3, 50, 0], [1, 0, 50, 0], [-1, 0, 50, 0], [0, 5, -2, 0]]
    a = viz.draw_host(pts, prims, styles, frames, CAMS, H, W, 100, 0, color0=0x010203)
    b = viz.draw_host(pts, prims, styles, frames, CAMS, H, W, 100, 0, color0=0x010203, accelerate=False)
    assert np.array_equal(a, b)
    assert len(np.unique(a[0].reshape(-1, 4), axis=0)) > 6                                       # a real picture, not one colour
    flat = np.broadcast_to(np.array([1, 2, 3, 255], np.uint8), (H, W, 4))
    assert all(np.array_equal(a[f], flat) for f in (4, 5, 6))                                    # no such camera, a negative count: background
    assert np.array_equal(a[2], viz.draw_host(pts, prims, styles, [[0, 0, 7, 0]], CAMS, H, W, 100, 0, color0=0x010203)[0])      # clipped to 0 ..
    assert np.array_equal(a[3], viz.draw_host(pts, prims[-3:], styles, [[0, 0, 3, 0]], CAMS, H, W, 100, 0, color0=0x010203)[0])  # .. n_prim


def test_dropped_primitives_leave_the_background():
    pts, _, styles = awkward_list(np.random.default_rng(2))
    n = len(pts)
    dropped = [[n - 6, n - 6, 11, 0], [n - 5, 8, 4, 0], [8, n - 4, 4, 0], [n - 3, n - 3, 11, 0], [n - 2, n - 2, 11, 0], [n - 1, n - 1, 11, 0],
               [8, 8, 6, 0], [8, 8, 7, 0], [8, 8, 8, 0], [8, 8, 9, 0], [-1, 8, 11, 0], [8, n, 11, 0], [8, 8, 12, 0], [8, 8, -1, 0]]
    for p in dropped:
        img = viz.draw_host(pts, [p], styles, [[0, 0, 1, 0]], CAMS, H, W, 256, 0, color0=0x0A0B0C)
        assert (img[0] == np.array([10, 11, 12, 255], np.uint8)).all(), p
    assert (viz.draw_host(pts, [[8, 8, 11, 0]], styles, [[0, 0, 1, 0]], CAMS, H, W)[0, H // 2, W // 2, :3] == 0xCC).all()      # the same disc, valid


def python_coverage(kind, size, ax, ay, bx, by, u, v):
    """The coverage rule of the module text in Python's unbounded integers."""
    ww, qx, qy = size * size, u - ax, v - ay
    if kind == viz.DISC:
        return qx * qx + qy * qy <= ww
    dx, dy = bx - ax, by - ay
    L2, s = dx * dx + dy * dy, qx * dx + qy * dy
    if L2 == 0 or s < 0:
        return 4 * (qx * qx + qy * qy) <= ww
    if s > L2:
        return 4 * ((u - bx) ** 2 + (v - by) ** 2) <= ww
    X = qx * dy - qy * dx
    return 4 * X * X <= ww * L2


def test_int64_coverage_is_the_unbounded_integers_at_the_extremes():
    big = viz.MAX_COORD
    assert big == 16383 and viz.MAX_SIZE == 64 and render.MAX_SIDE == 4096
    corners = [(x, y) for x in (-big, big) for y in (-big, big)]
    pixels = [(0, 0), (4095, 0), (0, 4095), (4095, 4095)]
    largest = 0
    for (ax, ay), (bx, by), (u, v), size in itertools.product(corners, corners, pixels, (0, 1, 64)):
        for kind in (viz.DISC, viz.SEGMENT):
            got = bool(viz.coverage(kind, size, ax, ay, bx, by, np.array([u]), np.array([v]))[0])
            assert got == python_coverage(kind, size, ax, ay, bx, by, u, v), (kind, size, ax, ay, bx, by, u, v)
        X = (u - ax) * (by - ay) - (v - ay) * (bx - ax)
        largest = max(largest, 4 * X * X, 64 * 64 * ((bx - ax) ** 2 + (by - ay) ** 2))
    assert 1.8e18 < largest < 2 ** 63 and 4 * (2 * 20478 * 32766) ** 2 < 2 ** 63               # the corners' largest term, and the bound of the proof
    # near misses and hits along a long thin segment: the exact test decides pixels one unit apart
    for u, v in ((2000, 2000), (2000, 2001), (2001, 2000), (1999, 2001)):
        for size in (1, 2, 3):
            assert bool(viz.coverage(1, size, -big, -big, big, big, np.array([u]), np.array([v]))[0]) == python_coverage(1, size, -big, -big, big, big, u, v)


def test_three_background_modes():
    none = (np.zeros((0, 3), np.float32), np.zeros((0, 4), np.int32), np.zeros((0, 4), np.int32))
    frames = [[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 2], [0, 0, 0, -1]]
    img = viz.draw_host(*none, frames, CAMS, H, W, 128, 0, color0=0x123456)
    assert (img == np.array([0x12, 0x34, 0x56, 255], np.uint8)).all()
    rng = np.random.default_rng(3)
    bg = rng.integers(0, 256, (2, H, W, 4), dtype=np.uint8)
    img = viz.draw_host(*none, frames, CAMS, H, W, 128, 1, bg, color0=0x123456)
    assert np.array_equal(img[:2, ..., :3], bg[..., :3]) and (img[..., 3] == 255).all()
    assert (img[2:] == np.array([0x12, 0x34, 0x56, 255], np.uint8)).all()                          # no such background: color0
    ids = rng.integers(-2, 9, (2, H, W)).astype(np.int32)
    ids[0, 0, :4] = [-1, -2, 7, 3]
    pal = np.array([0xFF0000, 0x00FF00, 0x0000FF], np.int32)
    img = viz.draw_host(*none, frames, CAMS, H, W, 128, 2, ids, pal, 0x101010, 0x202020)
    assert [tuple(p) for p in img[0, 0, :4, :3]] == [(16, 16, 16), (32, 32, 32), (0, 255, 0), (255, 0, 0)]      # table, void, 7 % 3, 3 % 3
    want = np.where(ids >= 0, pal[ids % 3], np.where(ids == -1, 0x101010, 0x202020))
    assert np.array_equal((img[:2, ..., 0].astype(int) << 16) | (img[:2, ..., 1].astype(int) << 8) | img[:2, ..., 2], want)
    for bad in (dict(bg_mode=3), dict(alpha=257), dict(bg_mode=1), dict(bg_mode=2, bg=ids), dict(bg_mode=1, bg=bg[:, :-1])):
        with pytest.raises(ValueError):
            viz.draw_host(*none, frames, CAMS, H, W, **bad)


@pytest.mark.parametrize("shape", [(1, 1, 3), (1, 1, 4), (33, 65, 3), (33, 65, 4)])
def test_png_round_trip(tmp_path, shape):
    img = np.random.default_rng(4).integers(0, 256, shape, dtype=np.uint8)
    path = str(tmp_path / "a.png")
    viz.write_png(path, img)
    assert np.array_equal(viz.read_png(path), img[:, :, :3])
    with pytest.raises(ValueError):
        viz.write_png(path, img.astype(np.float32))


def test_png_files_open_in_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    img = np.random.default_rng(5).integers(0, 256, (33, 65, 4), dtype=np.uint8)
    viz.write_png(str(tmp_path / "a.png"), img)
    with Image.open(str(tmp_path / "a.png")) as f:
        assert f.mode == "RGB" and f.size == (65, 33) and np.array_equal(np.asarray(f), img[:, :, :3])


def test_ag_draw_rejects_bad_arguments_without_a_gpu():
    L = _lib.lib()
    buf = (ctypes.c_int32 * 64)()
    near = ctypes.c_double(0.05)
    good = [buf, 1, buf, 1, buf, 1, buf, 1, buf, 1, ctypes.byref(near), 8, 8, 128, 0, None, 0, None, 0, 0, 0, buf, 256, buf, None]

    def call(**change):
        names = ["pts", "n_pts", "prims", "n_prim", "styles", "n_style", "frames", "F", "cams", "C", "near", "H", "W", "alpha", "bg_mode", "bg", "n_bg",
                 "palette", "n_pal", "color0", "color1", "scratch", "scratch_bytes", "out", "stream"]
        args = list(good)
        for k, v in change.items():
            args[names.index(k)] = v
        return L.ag_draw(*args)

    for change, word in ((dict(pts=None), b"null"), (dict(out=None), b"null"), (dict(scratch=None), b"null"), (dict(near=None), b"null"),
                         (dict(alpha=257), b"alpha"), (dict(alpha=-1), b"alpha"), (dict(H=0), b"H = 0"), (dict(W=4097), b"W = 4097"),
                         (dict(bg_mode=3), b"mode"), (dict(bg_mode=-1), b"mode"), (dict(F=0), b"F = 0"), (dict(C=0), b"C = 0"),
                         (dict(bg_mode=1), b"images"), (dict(bg_mode=2, bg=buf, n_bg=1), b"palette"), (dict(scratch_bytes=4), b"scratch"),
                         (dict(n_prim=-1), b"negative"), (dict(H=4096, W=4096, F=200000), b"exceed")):
        assert call(**change) == -1 and word in L.ag_last_error(), change
    assert L.ag_draw_scratch_bytes(100, 4) == 100 * 4 * 8 and L.ag_draw_scratch_bytes(0, 1) == 8 and L.ag_draw_scratch_bytes(5, 0) == 0


# ------------------------------------------------------------------------------------------------------ display lists
def test_add_edges_is_the_per_edge_loop():
    rng = np.random.default_rng(6)
    nodes = rng.normal(size=(7, 3)).astype(np.float32)
    recv, send = rng.integers(0, 7, 20), rng.integers(0, 7, 20)
    dl = viz.DrawList()
    dl.add_points(np.zeros((3, 3)))
    first = dl.add_points(nodes)
    obj, tool = dl.style(viz.SEGMENT, 1, 0, viz.GREEN), dl.style(viz.SEGMENT, 1, 0, viz.RED)
    dl.begin_frame()
    dl.add_edges(first, recv, send, obj, tool, 5)
    pts, prims, styles, frames = dl.tables()
    want = [[first + r, first + s, tool if (r >= 5 or s >= 5) else obj, 0] for r, s in zip(recv, send)]
    assert prims.tolist() == want and prims.dtype == np.int32 and frames.tolist() == [[0, 0, 20, 0]]
    assert styles.tolist() == [[1, 1, 0, 0x00FF00], [1, 1, 0, 0xFF0000]] and np.array_equal(pts[3:], nodes)
    # tool nodes kept elsewhere, and padded (-1) edges
    dl = viz.DrawList()
    dl.add_edges(10, [0, 5, 6, -1], [1, 0, 6, 2], 0, 1, 5, tool_offset=100)
    assert dl.tables()[1].tolist() == [[10, 11, 0, 0], [100, 10, 1, 0], [101, 101, 1, 0], [-1, -1, 0, 0]]


def test_add_discs_segments_and_arrows():
    dl = viz.DrawList()
    s = dl.style(viz.SEGMENT, 2, 0, viz.COLOR_ACTION)
    assert s == dl.style(viz.SEGMENT, 2, 0, viz.COLOR_ACTION) == 0 and dl.style(viz.DISC, 2, 0, 1) == 1
    dl.begin_frame(2, 5)
    dl.add_discs(np.arange(12, dtype=np.float32).reshape(4, 3), [1, 1, 0, 1])
    dl.begin_frame(1, 0)
    start, end = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.5]], np.float32), np.array([[2.0, 0.0, 0.0], [1.0, 3.0, 0.5]], np.float32)
    dl.add_arrows(start, end, s, tip=0.5)
    pts, prims, styles, frames = dl.tables()
    assert frames.tolist() == [[2, 0, 4, 5], [1, 4, 6, 0]] and prims[:4].tolist() == [[i, i, st, 0] for i, st in zip(range(4), [1, 1, 0, 1])]
    seg = lambda k: (pts[prims[k, 0]], pts[prims[k, 1]])      # noqa: E731
    for j in range(2):
        a, b = seg(4 + j)
        assert np.array_equal(a, start[j]) and np.array_equal(b, end[j])
        shaft = end[j] - start[j]
        heads = [seg(6 + j), seg(8 + j)]
        turns = []
        for a, b in heads:
            assert np.array_equal(a, end[j])
            h = b - a
            assert abs(np.linalg.norm(h) - 0.5 * np.linalg.norm(shaft)) < 1e-5 and abs(h[2]) < 1e-6       # tip |arrow| long, in the board's plane
            cosine = float(h @ -shaft / (np.linalg.norm(h) * np.linalg.norm(shaft)))
            assert abs(cosine - np.sqrt(0.5)) < 1e-5                                                      # 45 degrees off the reversed shaft
            turns.append(np.sign(np.cross(-shaft, h)[2]))
        assert sorted(turns) == [-1.0, 1.0]                                                               # one on either side


def toy_rollout():
    rng = np.random.default_rng(7)
    B, T, max_nobj, n_eef = 2, 7, 6, 1
    pred = rng.normal(size=(B, T, max_nobj, 3)).astype(np.float32)
    gt = rng.normal(size=(B, T, max_nobj, 3)).astype(np.float32)
    eef = rng.normal(size=(B, T, n_eef, 3)).astype(np.float32)
    edges = [[(np.array([0, 1, 6, 2]), np.array([1, 0, 3, 6])) for _ in range(T)] for _ in range(B)]
    return pred, gt, eef, edges, [5, 4], max_nobj, [7, 3]


def test_rollout_frames_counts_and_styles():
    pred, gt, eef, edges, n_kp, max_nobj, lengths = toy_rollout()
    dl = viz.rollout_frames(pred, gt, eef, edges, n_kp, max_nobj, None, lengths=lengths, backgrounds=[[10 * b + t for t in range(7)] for b in range(2)])
    pts, prims, styles, frames = dl.tables()
    assert len(frames) == 2 * (7 + 3)
    st = {tuple(s): i for i, s in enumerate(styles.tolist())}
    at = 0
    for b, steps in enumerate(lengths):
        for t in range(steps):
            for name in ("pred", "gt"):
                cam, first, count, bgi = frames[at].tolist()
                at += 1
                k, trail = n_kp[b], min(t, 5)
                assert (cam, bgi) == (0, 10 * b + t) and count == k + 1 + 4 + k * trail, (b, t, name)
                rows = prims[first:first + count]
                assert (rows[:k, 2] == st[(0, 4, 0, 0x0000FF)]).all() and (rows[:k, 0] == rows[:k, 1]).all()          # key points: blue, radius 4
                assert rows[k, 2] == st[(0, 3 if name == "pred" else 4, 0, 0xFF0000)]                               # the tool: red
                assert rows[k + 1:k + 5, 2].tolist() == [st[(1, 1, 0, 0x00FF00)]] * 2 + [st[(1, 1, 0, 0xFF0000)]] * 2  # object, tool edges
                src = pred if name == "pred" else gt
                assert np.array_equal(pts[rows[:k, 0]], src[b, t, :k]) and np.array_equal(pts[rows[k, 0]], eef[b, t, 0])
                assert np.array_equal(pts[rows[k + 3, 0]], eef[b, t, 0]) and np.array_equal(pts[rows[k + 3, 1]], src[b, t, 3])      # node 6 is the tool
                tr = rows[k + 5:]
                assert (tr[:, 2] == st[(1, 2, 1, 0x0000FF)]).all()                                                  # trails: overlay, width 2
                if trail:
                    assert np.array_equal(pts[tr[-k:, 0]], src[b, t, :k]) and np.array_equal(pts[tr[-k:, 1]], src[b, t - 1, :k])
                    assert np.array_equal(pts[tr[:k, 1]], src[b, t - trail, :k])
    assert at == len(frames) and frames[-1, 1] + frames[-1, 2] == len(prims)
    # simulator units go through the board frame
    dl2 = viz.rollout_frames(pred, gt, eef, edges, n_kp, max_nobj, 10.0, lengths=lengths)
    assert np.allclose(dl2.tables()[0][:, 2], -pts[:, 1] * np.float32(0.1)) and np.array_equal(dl2.tables()[1], prims)


def test_planning_frame_counts_and_styles():
    rng = np.random.default_rng(8)
    init, after, pred, target = (rng.normal(size=(5, 3)).astype(np.float32) for _ in range(4))
    e_init, e_pred, e_after = (np.arange(5), np.arange(5)[::-1]), (np.arange(4), np.arange(4) + 1), (np.array([0, 1]), np.array([1, 0]))
    common = dict(edges_init=e_init, edges_pred=e_pred, sim_real_ratio=10.0)
    dl = viz.planning_frame(init, pred, (0.1, 0.2, 0.3, 0.2), 3, target_state=target, **common)
    pts, prims, styles, frames = dl.tables()
    S = [tuple(s) for s in styles[prims[:, 2]].tolist()]
    want = ([(0, 5, 0, viz.COLOR_START)] * 5 + [(1, 2, 0, viz.COLOR_START)] * 5 + [(1, 2, 0, viz.COLOR_ACTION)] * 9 + [(0, 5, 1, viz.COLOR_TARGET)] * 5
            + [(0, 5, 1, viz.COLOR_PRED)] * 5 + [(1, 2, 1, viz.COLOR_PRED)] * 4)
    assert S == want and frames.tolist() == [[0, 0, len(want), 0]]
    assert (viz.COLOR_START, viz.COLOR_ACTION, viz.COLOR_PRED, viz.COLOR_TARGET) == (0xCA3F29, 0x1B4AF2, 0xED9E31, 0x1A8251)
    from adaptigraph_amd.sim_env import to_board_frame
    assert np.array_equal(pts[prims[:5, 0]], to_board_frame(init, 10.0))
    y = np.float32(init[:, 1].mean())
    shafts = prims[10:13]      # one arrow per repeat, each shifted by the push
    for i in range(3):
        assert np.allclose(pts[shafts[i, 0]], to_board_frame(np.array([0.1 + 0.2 * i, y, 0.2 + 0.0 * i], np.float32), 10.0), atol=1e-6)
        assert np.allclose(pts[shafts[i, 1]], to_board_frame(np.array([0.3 + 0.2 * i, y, 0.2], np.float32), 10.0), atol=1e-6)
    # the `_1` image: state_after and its edges instead of the start state; a target box instead of a cloud: four strokes
    dl = viz.planning_frame(init, pred, (0.1, 0.2, 0.3, 0.2), 1, target_box=((-1.0, 1.0), (-0.5, 0.5)), state_after=after, edges_after=e_after,
                            camera=2, background=2, **common)
    pts, prims, styles, frames = dl.tables()
    S = [tuple(s) for s in styles[prims[:, 2]].tolist()]
    assert S == ([(0, 5, 0, viz.COLOR_START)] * 5 + [(1, 2, 0, viz.COLOR_START)] * 2 + [(1, 2, 0, viz.COLOR_ACTION)] * 3
                 + [(1, 2, 1, viz.COLOR_TARGET)] * 4 + [(0, 5, 1, viz.COLOR_PRED)] * 5 + [(1, 2, 1, viz.COLOR_PRED)] * 4)
    assert frames.tolist() == [[2, 0, len(S), 2]] and np.array_equal(pts[prims[:5, 0]], to_board_frame(after, 10.0))
    img = viz.draw(pts, prims, styles, [[0, 0, len(S), 0]], CAMS, H, W, 128)
    assert img.shape == (1, H, W, 4) and isinstance(img, np.ndarray)                                  # device=None: the host statement


def test_radius_edges_host():
    x = np.array([[0, 0, 0], [0.1, 0, 0], [0.25, 0, 0], [2, 0, 0]], np.float32)
    r, s = viz.radius_edges_host(x, 0.2, 10)
    assert sorted(zip(r.tolist(), s.tolist())) == [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 1), (2, 2), (3, 3)]
    r, s = viz.radius_edges_host(x, 0.2, 2)
    assert (1, 2) not in set(zip(r.tolist(), s.tolist())) and (1, 0) in set(zip(r.tolist(), s.tolist()))


def test_sim_env_colour_images_on_the_host():
    env = rope_env(None)
    obs = env.get_obs(get_color=True)
    depth, ids = env.render()
    for i in range(4):
        c = obs[f"color_{i}"]
        assert c.shape == (1, 90, 160, 3) and c.dtype == np.uint8 and obs[f"depth_{i}"].shape == (1, 90, 160)
        want = np.where(ids[i] >= 0, np.asarray(viz.PALETTE)[ids[i] % len(viz.PALETTE)], np.where(ids[i] == -1, viz.TABLE_COLOR, viz.VOID_COLOR))
        assert np.array_equal((c[0, ..., 0].astype(int) << 16) | (c[0, ..., 1].astype(int) << 8) | c[0, ..., 2], want)
    assert (ids >= 0).any() and set(env.get_obs(get_color=True, get_depth=False)) == {f"color_{i}" for i in range(4)}


def test_closed_loop_draws_without_changing_the_run(tmp_path):
    import torch
    from adaptigraph_amd.closed_loop import run_closed_loop
    lo, hi = torch.tensor([-1.0, -1.0, -3.14, 2.0]), torch.tensor([1.0, 1.0, 3.14, 4.0])
    criteria = lambda cloud: ((cloud - torch.tensor([0.0, 0.03, -0.5])) ** 2).sum(-1).mean()      # noqa: E731
    runs = []
    for name, kw in (("plain", {}), ("viz", dict(viz=True, target_state=torch.tensor([[0.1 * i - 1.0, 0.03, -0.5] for i in range(20)])))):
        torch.manual_seed(0)
        np.random.seed(0)
        env = rope_env(None)
        out = tmp_path / name
        acts, errors = run_closed_loop(env, StubPlanner(), criteria, 2, 2, lo, hi, 0.2, save_dir=str(out), **kw)
        runs.append((acts, errors, [dict(np.load(str(out / f"interaction_{i}.npz"))) for i in range(2)], torch.rand(1), np.random.rand()))
    (a0, e0, r0, t0, n0), (a1, e1, r1, t1, n1) = runs
    assert torch.equal(a0, a1) and e0 == e1 and torch.equal(t0, t1) and n0 == n1                       # no random number drawn by the drawing
    assert all(set(x) == set(y) and all(np.array_equal(x[k], y[k]) for k in x) for x, y in zip(r0, r1))
    assert sorted(p.name for p in (tmp_path / "viz").glob("*.png")) == [f"rgb_vis_{i}_{j}.png" for i in range(2) for j in range(2)]
    assert not list((tmp_path / "plain").glob("*.png"))
    first, second = viz.read_png(str(tmp_path / "viz" / "rgb_vis_0_0.png")), viz.read_png(str(tmp_path / "viz" / "rgb_vis_0_1.png"))
    assert first.shape == (90, 160, 3) and not np.array_equal(first, second)
    colours = {tuple(c) for c in first.reshape(-1, 3)}
    assert (202, 63, 41) in colours and (27, 74, 242) in colours                                       # the start state and the action, opaque


def test_frames_per_launch_follows_the_byte_budget():
    assert viz.frames_per_launch(720, 1280) == 64 and viz.frames_per_launch(4096, 4096) == 2 and viz.frames_per_launch(1440, 2560) == 16
    assert viz.frames_per_launch(90, 160) == 64 * 64 and all(viz.frames_per_launch(h, w) % 2 == 0 for h, w in ((1, 1), (721, 1283), (33, 65)))


def test_rollout_record_is_the_same_whatever_the_batch(tmp_path):
    """Launches of 2 and of 8 frames get their own rollouts' points and primitives alone (chunks that end inside a rollout, span two, or
    hold one whole): the files are those of one launch for everything."""
    pred, gt, eef, _, n_kp, max_nobj, lengths = toy_rollout()
    rng = np.random.default_rng(9)
    scale = np.float32(0.3)
    schedules = [[(10 * b + t, 10 * b + t + 1) for t in range(n)] for b, n in enumerate(lengths)]
    particles = [[(rng.normal(size=(12, 3)) * scale).astype(np.float32) for _ in range(n)] for n in lengths]
    files = {}
    for batch in (None, 2, 8):
        dirs = [str(tmp_path / f"{batch}_{b}") for b in range(2)]
        for d in dirs:
            (tmp_path / d).mkdir()
        written = viz.write_rollout_record(dirs, schedules, pred * scale, gt * scale, eef * scale, None, n_kp, max_nobj, particles, "rope", None,
                                           H=45, W=80, batch=batch)
        assert len(written) == 3 * sum(lengths)
        files[batch] = [viz.read_png(p) for p in written]
    assert len({tuple(c) for c in files[None][0].reshape(-1, 3)}) >= 3                            # a picture: table, key points, more
    for batch in (2, 8):
        assert all(np.array_equal(a, b) for a, b in zip(files[None], files[batch]))
