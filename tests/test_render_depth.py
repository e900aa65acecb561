"""Simulated depth cameras (adaptigraph_amd/render.py, csrc/ag_render.hip): the host statement against itself without its pixel boxes and against
the un-projection of perception.py, and the HIP kernel against the host statement, bit for bit."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from adaptigraph_amd import _lib, perception as P, render as Rd, sim, sim_env

DEV = "cuda:0"
BIG_BOX = np.array([[-1e6, 1e6]] * 3)
TABLE = (0.0, 0.0, 1.0, 0.0)              # the board plane z = 0; the cameras sit at z < 0 (z points down)


def bits(depth):
    return np.ascontiguousarray(depth, np.float32).view(np.int32)


def cams_small(H, W, C=2, fov=40.0):
    pos = [(0.6, 0.6, -1.0), (-0.6, 0.5, -0.9), (0.1, -0.8, -1.1)][:C]
    return Rd.look_at_cameras(pos, (0.0, 0.0, 0.0), H, W, fov, up=(0.0, 0.0, -1.0))


def from_pixels(R, t, K, u, v, z):
    """World points that camera (R, t, K) sees at pixel (u, v) and depth z."""
    Kinv = np.linalg.inv(K)
    cam = (Kinv @ np.stack([u, v, np.ones_like(u)])) * z
    return (R @ cam).T + t


def edge_scene(H, W, near, r):
    """40 spheres placed through camera 0: on and beyond every image edge, behind the camera, inside the band c_2 - r <= near, random ones, and
    spheres 7 and 23 at one centre."""
    Rl, tl, Kl = cams_small(H, W)
    rng = np.random.default_rng(5)
    us = np.array([-3.0, 0.0, W / 2 - 0.5, W - 1.0, W + 2.0])
    vs = np.array([-3.0, 0.0, H / 2 - 0.5, H - 1.0, H + 2.0])
    uu, vv = (a.ravel() for a in np.meshgrid(us, vs))
    keep = ~((uu == us[2]) & (vv == vs[2]))                                   # 24 positions around the image
    u, v, z = list(uu[keep]), list(vv[keep]), list(rng.uniform(0.9, 1.5, 24))
    u += [10.0, 20.0, 30.0]; v += [10.0, 20.0, 30.0]; z += [-0.5, -1.2, -0.01]       # behind the camera
    u += [W / 6] * 3; v += [5 * H / 6] * 3; z += [near + 0.9 * r, near + 0.5 * r, near + 3.0 * r]      # inside the cull band (27, 28) and outside it (29)
    k = 40 - len(u)
    u += list(rng.uniform(5, W - 5, k)); v += list(rng.uniform(5, H - 5, k)); z += list(rng.uniform(0.8, 1.6, k))
    pts = from_pixels(Rl[0], tl[0], Kl[0], np.array(u), np.array(v), np.array(z))
    pts[7] = from_pixels(Rl[0], tl[0], Kl[0], np.array([W - 12.0]), np.array([10.0]), np.array([0.6]))[0]      # in front of all others
    pts[23] = pts[7]
    return pts.astype(np.float32)[None], (Rl, tl, Kl)


# ------------------------------------------------------------------------------------------------------ CPU: the host statement
@pytest.mark.parametrize("plane", [None, TABLE])
def test_accelerated_statement_equals_the_plain_one(plane):
    H, W, near, r = 48, 64, 0.05, 0.06
    pts, (Rl, tl, Kl) = edge_scene(H, W, near, r)
    n, rad = np.array([40], np.int32), np.array([r], np.float32)
    fast = Rd.render_depth_host(pts, n, rad, Rl, tl, Kl, H, W, plane, near, 4.0, accelerate=True)
    plain = Rd.render_depth_host(pts, n, rad, Rl, tl, Kl, H, W, plane, near, 4.0, accelerate=False)
    assert fast[0].shape == (1, 2, H, W) and fast[0].dtype == np.float32 and fast[1].dtype == np.int32
    assert np.array_equal(bits(fast[0]), bits(plain[0])) and np.array_equal(fast[1], plain[1])
    ids = fast[1]
    assert (ids[0, 0] == 7).sum() > 20 and not (ids == 23).any()              # one centre: the lower index is the id
    assert set(np.unique(ids)) - set(range(-2, 40)) == set() and (ids >= 0).sum() > 300
    assert not np.isin(ids[0, 0], [24, 25, 26]).any()                         # behind camera 0
    assert not np.isin(ids[0, 0], [27, 28]).any()                             # c_2 - r <= near: culled
    assert (ids[0, 0] == 29).sum() > 100
    if plane is None:
        assert (ids == -2).any() and not (ids == -1).any() and np.all((ids == -2) == (fast[0] == 0))
    else:
        assert (ids == -1).sum() > H * W


def test_round_trip_through_the_unprojection():
    """Render, un-project with perception.depth_to_points_host: every point lies on the sphere its pixel's id names, plane pixels on the table.
    Bound 1e-6: two fp32 roundings (the depth, the point) of quantities <= 2 along rays of |q| <= 1.5, about 4e-7."""
    H, W, r = 48, 64, 0.03
    Rl, tl, Kl = cams_small(H, W)
    rng = np.random.default_rng(11)
    pts = np.concatenate([rng.uniform(-0.3, 0.3, (60, 2)), rng.uniform(-0.2, -r, (60, 1))], 1).astype(np.float32)[None]
    depth, ids = Rd.render_depth_host(pts, np.array([60], np.int32), np.array([r], np.float32), Rl, tl, Kl, H, W, TABLE, 0.05, 2.0)
    assert float(depth.max()) < 2.0
    got, pix = P.depth_to_points_host(list(depth[0]), Rl, tl, Kl, BIG_BOX, keep_masks=list(ids[0] >= 0), stride=1, depth_threshold=(0, 2),
                                      return_pixels=True)
    assert len(got) == int((ids >= 0).sum()) > 200
    owner = ids[0][pix[:, 0], pix[:, 1], pix[:, 2]]
    dist = np.linalg.norm(got.astype(np.float64) - pts[0, owner].astype(np.float64), axis=1)
    err = float(np.abs(dist - np.float64(np.float32(r))).max())
    print(f"round trip: max | |p - c| - r | = {err:.3e} over {len(got)} pixels")
    assert err <= 1e-6
    table = P.depth_to_points_host(list(depth[0]), Rl, tl, Kl, BIG_BOX, keep_masks=list(ids[0] == -1), stride=1, depth_threshold=(0, 2))
    assert len(table) == int((ids == -1).sum()) > 200
    print(f"round trip: max |z| on the table = {float(np.abs(table[:, 2]).max()):.3e}")
    assert float(np.abs(table[:, 2]).max()) <= 1e-6


def test_intrinsics_must_be_a_pinhole():
    Rl, tl, Kl = cams_small(8, 8, C=1)
    pts, n, rad = np.zeros((1, 1, 3), np.float32), np.array([1], np.int32), np.array([0.1], np.float32)
    Rd.render_depth_host(pts, n, rad, Rl, tl, Kl, 8, 8)
    for i, j, val in ((0, 1, 0.5), (1, 0, 1e-3), (2, 0, 1e-6), (2, 1, 1.0), (2, 2, 2.0), (0, 0, -50.0)):
        K = Kl[0].copy()
        K[i, j] = val
        with pytest.raises(ValueError, match="pinhole"):
            Rd.render_depth_host(pts, n, rad, Rl, tl, [K], 8, 8)
        with pytest.raises(ValueError, match="pinhole"):
            Rd.render_depth(pts, n, rad, Rl, tl, [K], 8, 8, device=DEV)       # refused before anything touches a device


def test_cameras_look_at_the_table():
    Rl, tl, Kl = Rd.default_cameras(10.0)
    assert len(Rl) == 4 and "OURS" in Rd.default_cameras.__doc__
    for R, t, K in zip(Rl, tl, Kl):
        assert np.allclose(R.T @ R, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(R), 1.0)
        assert np.allclose(sorted(np.abs(t)), [0.6, 0.6, 1.0]) and t[2] == -1.0          # distance 6, height 10 over sim_real_ratio; z is down
        c = R.T @ (np.zeros(3) - t)                                                       # the table origin in the camera frame
        assert np.allclose(c[:2], 0, atol=1e-12) and c[2] > 0                             # on the optical axis, in front
        assert (R.T @ np.array([0.0, 0.0, -1.0]))[1] < 0                                  # the world's up is up in the image (y is down)
        assert K[0, 0] == K[1, 1] and K[0, 2] == 640 and K[1, 2] == 360
    assert sorted((np.sign(t[0]), np.sign(t[1])) for t in tl) == [(-1, -1), (-1, 1), (1, -1), (1, 1)]


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "adaptigraph_hip.h")).read()
    assert f"#define AG_RENDER_TILE {Rd.TILE}\n" in header and f"#define AG_RENDER_CHUNK {Rd.CHUNK}\n" in header
    assert f"#define AG_RENDER_MAX_SIDE {Rd.MAX_SIDE}\n" in header and f"#define AG_RENDER_MAX_PARTICLES {Rd.MAX_PARTICLES}\n" in header
    buf = (ctypes.c_char * 256)()
    good = dict(pts=buf, n=buf, radius=buf, cams=buf, plane=None, limits=buf, E=1, n_max=8, C=1, H=8, W=8, depth=buf, id=buf)
    call = lambda **kw: L.ag_render_depth(*dict(good, **kw).values(), None)
    for kw, text in (({"E": 0}, b"E = 0"), ({"C": 0}, b"C = 0"), ({"E": -1}, b"E = -1"), ({"H": 0}, b"H = 0"), ({"H": 4097}, b"H = 4097"),
                     ({"W": 0}, b"W = 0"), ({"W": 4097}, b"W = 4097"), ({"n_max": 0}, b"n_max = 0"), ({"n_max": 4097}, b"n_max = 4097")):
        assert call(**kw) == -1 and text in L.ag_last_error(), kw
    for name in ("pts", "n", "radius", "cams", "limits", "depth", "id"):
        assert call(**{name: None}) == -1 and b"null" in L.ag_last_error(), name


# ------------------------------------------------------------------------------------------------------ GPU: the kernel against the statement
def awkward_scene():
    """H, W = TILE + 13, 2 TILE + 6; three cameras; episodes of 0, 37 and CHUNK + 44 spheres with their own radii, the third with every centre
    inside tile (0, 0) of camera 0; rows behind n[e] are NaN."""
    H, W = Rd.TILE + 13, 2 * Rd.TILE + 6
    Rl, tl, Kl = cams_small(H, W, C=3)
    rng = np.random.default_rng(21)
    n = np.array([0, 37, Rd.CHUNK + 44], np.int32)
    pts = np.full((3, int(n.max()), 3), np.nan, np.float32)
    pts[1, :37] = np.concatenate([rng.uniform(-0.35, 0.35, (37, 2)), rng.uniform(-0.25, -0.05, (37, 1))], 1)
    m = int(n[2])
    pts[2, :m] = from_pixels(Rl[0], tl[0], Kl[0], rng.uniform(6, Rd.TILE - 6, m), rng.uniform(6, Rd.TILE - 6, m), rng.uniform(1.0, 1.4, m))
    return pts, n, np.array([0.03, 0.05, 0.02], np.float32), (Rl, tl, Kl), H, W


@functools.lru_cache(maxsize=None)
def awkward_reference(with_plane):
    pts, n, rad, (Rl, tl, Kl), H, W = awkward_scene()
    return Rd.render_depth_host(pts, n, rad, Rl, tl, Kl, H, W, TABLE if with_plane else None, 0.05, 4.0)


@pytest.mark.gpu
@pytest.mark.parametrize("with_plane", [False, True])
def test_device_equals_host_at_awkward_sizes(with_plane):
    pts, n, rad, (Rl, tl, Kl), H, W = awkward_scene()
    want_d, want_i = awkward_reference(with_plane)
    one_tile = want_i[2, 0]
    assert len(np.unique(one_tile[one_tile >= 0])) > Rd.CHUNK // 2 and one_tile[one_tile >= 0].max() >= Rd.CHUNK      # the list spans two chunks
    assert not (one_tile[Rd.TILE:] >= 0).any() and not (one_tile[:, Rd.TILE:] >= 0).any()
    depth, ids = Rd.render_depth(pts, n, rad, Rl, tl, Kl, H, W, TABLE if with_plane else None, 0.05, 4.0, device=DEV)
    assert depth.shape == (3, 3, H, W) and depth.dtype == torch.float32 and ids.dtype == torch.int32
    assert np.array_equal(ids.cpu().numpy(), want_i)
    assert np.array_equal(bits(depth.cpu().numpy()), bits(want_d))
    assert not (want_i[0] >= 0).any() and (want_i[1] >= 0).sum() > 100


@pytest.mark.gpu
@pytest.mark.parametrize("side", [1, Rd.TILE - 1])
def test_partial_tile_under_one_sphere(side):
    K = np.array([[2.0 * side, 0, side / 2.0], [0, 2.0 * side, side / 2.0], [0, 0, 1.0]])
    pts, n, rad = np.array([[[0.0, 0.0, 1.0]]], np.float32), np.array([1], np.int32), np.array([0.5], np.float32)
    args = (pts, n, rad, [np.eye(3)], [np.zeros(3)], [K], side, side, None, 0.05, 4.0)
    want_d, want_i = Rd.render_depth_host(*args)
    assert np.all(want_i == 0)
    depth, ids = Rd.render_depth(*args, device=DEV)
    assert np.array_equal(ids.cpu().numpy(), want_i) and np.array_equal(bits(depth.cpu().numpy()), bits(want_d))


@pytest.mark.gpu
def test_a_count_out_of_range_renders_as_empty():
    H, W = 20, 40
    Rl, tl, Kl = cams_small(H, W)
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.uniform(-0.3, 0.3, (3, 12, 2)), rng.uniform(-0.2, -0.05, (3, 12, 1))], 2).astype(np.float32)
    pts[:2] = np.nan
    n, rad = np.array([-5, 13, 12], np.int32), np.full(3, 0.05, np.float32)
    want_d, want_i = Rd.render_depth_host(pts, n, rad, Rl, tl, Kl, H, W, TABLE)
    assert np.all(want_i[:2] < 0) and (want_i[:2] == -1).any() and (want_i[2] >= 0).any()
    depth, ids = Rd.render_depth(pts, n, rad, Rl, tl, Kl, H, W, TABLE, device=DEV)
    assert np.array_equal(ids.cpu().numpy(), want_i) and np.array_equal(bits(depth.cpu().numpy()), bits(want_d))


def cloth_scene():
    cloth, _ = sim.initial_cloth(np.random.default_rng(2), 64, 64)
    pts = sim_env.to_board_frame(cloth.reshape(1, -1, 3), 10.0)
    return pts, np.array([4096], np.int32), np.array([np.float32(sim.CLOTH_DEFAULT.r) * np.float32(0.1)], np.float32)


@pytest.mark.gpu
def test_full_size_cloth_against_the_accelerated_host():
    pts, n, rad = cloth_scene()
    Rl, tl, Kl = Rd.default_cameras(10.0)
    want_d, want_i = Rd.render_depth_host(pts, n, rad, Rl, tl, Kl, 720, 1280, TABLE)
    assert len(np.unique(want_i[want_i >= 0])) > 3000
    depth, ids = Rd.render_depth(pts, n, rad, Rl, tl, Kl, 720, 1280, TABLE, device=DEV)
    assert torch.equal(ids.cpu(), torch.from_numpy(want_i)) and torch.equal(depth.cpu().view(torch.int32), torch.from_numpy(bits(want_d)))


@pytest.mark.gpu
def test_replayed_graph_gives_the_same_bits():
    pts, n, rad, (Rl, tl, Kl), H, W = awkward_scene()
    want_d, want_i = awkward_reference(True)
    r = Rd.DeviceRenderer(Rl, tl, Kl, H, W, TABLE, 0.05, 4.0, E=3, device=DEV)
    args = [torch.from_numpy(a).to(DEV) for a in (pts, n, rad)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # warm-up outside the capture
        r.launch(*args)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r.launch(*args)
    for _ in range(3):
        r.depth.fill_(-1.0)
        r.id.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(r.id.cpu().numpy(), want_i) and np.array_equal(bits(r.depth.cpu().numpy()), bits(want_d))
