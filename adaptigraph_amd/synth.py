"""Synthetic particle clouds and graph inputs.

Pure numpy, deterministic, shared by tools/gen_golden.py, tests/ and bench.py so that
every leg (reference goldens, CPU oracle, HIP path) sees the same bytes.

Conventions follow the reference's rollout driver (src/planning/forward_dynamics.py:83-123):
y is "up", object particles occupy slots [0, n_p), tool/eef key-points the trailing slots,
attrs[:, 0] = 1 for objects and attrs[:, 1] = 1 for tools, p_instance = 1 (one instance).
"""
import numpy as np

MATERIALS = {
    # adj radius / top-k / connect_tools_all / #tool points : src/config/planning/{rope,granular,cloth}.yaml:10-14
    "rope": dict(radius=0.5, topk=10, connect_tools_all=False, n_tools=1),
    "granular": dict(radius=0.4, topk=20, connect_tools_all=False, n_tools=5),
    "cloth": dict(radius=0.75, topk=5, connect_tools_all=True, n_tools=1),
}


def rope_cloud(n, spacing, rng):
    """Polyline x = i*s, y = 0, z = 3 sin(2 pi i / n) + N(0, 0.01^2); one tool near the middle."""
    i = np.arange(n, dtype=np.float64)
    pts = np.stack([i * spacing, np.zeros(n), 3.0 * np.sin(2 * np.pi * i / n)], -1)
    pts = pts + rng.normal(0.0, 0.01, pts.shape)
    tool = np.array([[pts[n // 2, 0], 0.0, pts[n // 2, 2] + 0.3]])
    return pts.astype(np.float32), tool.astype(np.float32)


def granular_cloud(n, rng, density=80.0):
    """n points uniform in a thin square slab with ~40 points per radius-0.4 disc; 5 tools on a 1.0 bar."""
    side = float(np.sqrt(n / density))
    pts = np.stack([rng.uniform(0, side, n), rng.uniform(0, 0.05, n), rng.uniform(0, side, n)], -1)
    c = side / 2
    off = np.array([0.0, 0.5, 0.25, -0.25, -0.5])
    tool = np.stack([np.full(5, c), np.full(5, 0.0), c + off], -1)
    return pts.astype(np.float32), tool.astype(np.float32)


def cloth_cloud(side, rng, tool_near=True):
    """side x side grid, spacing 0.25 in x-z, + N(0, 0.01^2); 1 tool above the grid centre (or far away)."""
    g = np.arange(side, dtype=np.float64) * 0.25
    xx, zz = np.meshgrid(g, g, indexing="ij")
    pts = np.stack([xx.ravel(), np.zeros(side * side), zz.ravel()], -1)
    pts = pts + rng.normal(0.0, 0.01, pts.shape)
    c = g[-1] / 2
    tool = np.array([[c, 0.05, c]]) if tool_near else np.array([[c, 50.0, c]])
    return pts.astype(np.float32), tool.astype(np.float32)


def make_cloud(material, n_obj, rng, **kw):
    if material == "rope":
        return rope_cloud(n_obj, kw.get("spacing", 0.1), rng)
    if material == "granular":
        return granular_cloud(n_obj, rng)
    if material == "cloth":
        side = int(round(np.sqrt(n_obj)))
        assert side * side == n_obj, "cloth wants a square particle count"
        return cloth_cloud(side, rng, kw.get("tool_near", True))
    raise ValueError(material)


def make_graph_inputs(material, n_obj, batch, seed=0, n_his=4, n_pad=0, **kw):
    """Batched model inputs in the reference's dict layout (minus Rr/Rs; edges are built separately).

    n_pad extra *invalid* object slots (mask False, position 0) sit between the objects and the tools,
    reproducing the dataset padding contract ("padded node slots").
    Sample b > 0 is sample 0 plus a small per-sample perturbation so batches are not replicas.
    """
    rng = np.random.default_rng(seed)
    obj, tool = make_cloud(material, n_obj, rng, **kw)
    n_t = tool.shape[0]
    n_p = n_obj + n_pad
    N = n_p + n_t
    state = np.zeros((batch, n_his, N, 3), np.float32)
    for b in range(batch):
        cur = np.zeros((N, 3), np.float32)
        cur[:n_obj] = obj + rng.normal(0, 0.003, obj.shape).astype(np.float32) * (b > 0)
        cur[n_p:] = tool
        for h in range(n_his):
            jit = rng.normal(0, 0.01, (N, 3)).astype(np.float32)
            jit[n_obj:n_p] = 0
            state[b, h] = cur + jit
        state[b, :, n_obj:n_p] = 0
    attrs = np.zeros((batch, N, 2), np.float32)
    attrs[:, :n_obj, 0] = 1
    attrs[:, n_p:, 1] = 1
    action = np.zeros((batch, N, 3), np.float32)
    action[:, n_p:] = np.array([0.1, 0.0, 0.0], np.float32)
    p_instance = np.zeros((batch, n_p, 1), np.float32)
    p_instance[:, :n_obj] = 1
    phys = np.full((batch, 1), 0.5, np.float32)
    mask = np.zeros((batch, N), bool)
    mask[:, :n_obj] = True
    mask[:, n_p:] = True
    tool_mask = np.zeros((batch, N), bool)
    tool_mask[:, n_p:] = True
    return dict(state=state, attrs=attrs, action=action, p_instance=p_instance, phys=phys,
                mask=mask, tool_mask=tool_mask, n_p=n_p, n_obj=n_obj, n_tools=n_t)


def make_mpc_inputs(material, n_obj, bsz, n_look=1, seed=0, len_lo=2, len_hi=6, **kw):
    """state_cur (n_obj,3) + action sequences (bsz, n_look, 4) = [x, z, theta, length] for dynamics()."""
    rng = np.random.default_rng(seed)
    obj, _ = make_cloud(material, n_obj, rng, **kw)
    lo = obj.min(0)
    hi = obj.max(0)
    act = np.zeros((bsz, n_look, 4), np.float32)
    act[..., 0] = rng.uniform(lo[0], hi[0], (bsz, n_look))
    act[..., 1] = rng.uniform(lo[2] - 0.3, hi[2] + 0.3, (bsz, n_look))
    act[..., 2] = rng.uniform(-3.14, 3.14, (bsz, n_look))
    act[..., 3] = rng.uniform(len_lo, len_hi, (bsz, n_look))
    return obj, act


def tabletop_scene(n_cam=4, H=720, W=1280, seed=0, band=0.015, noise=0.0008, speckle=0.005):
    """Depth images of a board (z = 0 in the board frame, 0.8 x 0.6 m) with a rope-like object (a 12 mm high ridge along y = 0.1 sin(8 x)),
    seen by `n_cam` cameras above the board's corners looking at its centre, for adaptigraph_amd.perception: range noise, `speckle` of the
    pixels pulled towards the camera (flying pixels), as many holes (0) and a few NaNs, and per camera the keep-mask a segmentation would give
    (the object's neighbourhood of half-width `band`, plus a few stray pixels).
    -> dict(depth [H,W] float32 list, masks [H,W] bool list, R, t, intr lists (camera -> board), bbox (3,2))."""
    rng = np.random.default_rng(seed)
    corners = [(0.55, 0.45), (-0.55, 0.45), (-0.55, -0.45), (0.55, -0.45)]
    K = np.array([[0.9 * W, 0.0, W / 2.0], [0.0, 0.9 * W, H / 2.0], [0.0, 0.0, 1.0]])
    Kinv = np.linalg.inv(K)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rays_cam = np.stack([Kinv[r, 0] * u + Kinv[r, 1] * v + Kinv[r, 2] for r in range(3)], -1)        # z component 1: depth = z_cam
    out = dict(depth=[], masks=[], R=[], t=[], intr=[], bbox=np.array([[-0.35, 0.35], [-0.25, 0.25], [-0.02, 0.15]]))
    for c in range(n_cam):
        cx, cy = corners[c % 4]
        pos = np.array([cx, cy, 0.7 + 0.03 * (c // 4)])
        f = -pos / np.linalg.norm(pos)
        r = np.cross(f, [0.0, 0.0, 1.0])
        r /= np.linalg.norm(r)
        R = np.stack([r, np.cross(f, r), f], 1)
        rays = rays_cam @ R.T
        with np.errstate(divide="ignore", invalid="ignore"):
            d0 = -pos[2] / rays[..., 2]
            hit = pos + d0[..., None] * rays
            near = np.abs(hit[..., 1] - 0.1 * np.sin(8.0 * hit[..., 0])) < 0.006
            near &= np.abs(hit[..., 0]) < 0.3
            d = np.where(near, (0.012 - pos[2]) / rays[..., 2], d0)
            hit = pos + d[..., None] * rays
        d = d + rng.normal(0.0, noise, d.shape)
        pick = rng.random(d.shape)
        d = np.where(pick < speckle, d * rng.uniform(0.5, 0.98, d.shape), d)
        d = np.where((pick >= speckle) & (pick < 2 * speckle), 0.0, d)
        d = np.where((pick >= 2 * speckle) & (pick < 2.1 * speckle), np.nan, d)
        d = np.where((d0 > 0) & (d0 < 3.0), d, 0.0)
        mask = (np.abs(hit[..., 1] - 0.1 * np.sin(8.0 * hit[..., 0])) < band) & (np.abs(hit[..., 0]) < 0.3 + band)
        mask |= rng.random(d.shape) < 0.002
        out["depth"].append(d.astype(np.float32)); out["masks"].append(mask)
        out["R"].append(R); out["t"].append(pos); out["intr"].append(K.copy())
    return out
