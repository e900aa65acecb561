"""Masks and colour images shared by tests/test_segment_cpu.py and tests/test_segment.py: every image size at which the labelling kernel takes
another path (sized from segment.TILE_H / TILE_W, so a change of tile moves them), and the contents on which a labelling goes wrong: the
equivalence found last, components that meet only where four tiles meet, percolating noise."""
import functools

import numpy as np

from adaptigraph_amd import segment, viz

TH, TW = segment.TILE_H, segment.TILE_W
SIZES = [(1, 1), (1, TW + 1), (TH + 1, 1), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, 3 * TW - 1), (90, 160)]
DENSITIES = (0.1, 0.41, 0.59, 0.9)      # 0.41 and 0.59: the percolation densities of the 8- and the 4-connected grid


def spiral(H, W):
    """A rectangular spiral one pixel wide with one-pixel gaps, from the top left corner inward until it cannot turn."""
    m = np.zeros((H, W), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    turns = 0
    while turns < 2:
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        ahead_free = 0 <= ny < H and 0 <= nx < W and not m[ny, nx] and not (0 <= ay < H and 0 <= ax < W and m[ay, ax])
        if ahead_free:
            y, x, turns = ny, nx, 0
            m[y, x] = True
        else:
            dy, dx, turns = dx, -dy, turns + 1      # right turn
    return m


def serpentine(H, W):
    """Full rows at every second line, joined alternately at the right and the left end: one component that crosses every tile border both ways."""
    m = np.zeros((H, W), bool)
    m[::2] = True
    for k, y in enumerate(range(1, H - 1, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = True
    return m


def corner_blocks(H, W, anti):
    """Two 3 x 3 blocks that touch only diagonally, at the point where four tiles meet (or the image's middle, where it has one tile)."""
    cy, cx = (TH if H > TH else H // 2), (TW if W > TW else W // 2)
    m = np.zeros((H, W), bool)
    if anti:
        m[max(cy - 3, 0):cy, cx:cx + 3] = True
        m[cy:cy + 3, max(cx - 3, 0):cx] = True
    else:
        m[max(cy - 3, 0):cy, max(cx - 3, 0):cx] = True
        m[cy:cy + 3, cx:cx + 3] = True
    return m


def rings(H, W):
    """Nested rectangular rings, one pixel wide, two pixels apart, the outermost on the image border: components inside holes inside components."""
    m = np.zeros((H, W), bool)
    k = 0
    while H - 2 * k >= 1 and W - 2 * k >= 1:
        m[k:H - k, k:W - k] = True
        if H - 2 * k > 2 and W - 2 * k > 2:
            m[k + 1:H - k - 1, k + 1:W - k - 1] = False
        k += 3
    return m


def random_mask(H, W, density, seed=0):
    return np.random.default_rng([seed, H, W, int(density * 100)]).random((H, W)) < density


def contents(H, W):
    """name -> (H, W) bool."""
    yy, xx = np.mgrid[:H, :W]
    c = {"empty": np.zeros((H, W), bool), "full": np.ones((H, W), bool)}
    points = np.zeros((H, W), bool)
    points[[0, 0, H - 1, H - 1, H // 2], [0, W - 1, 0, W - 1, W // 2]] = True
    c["points"] = points
    c["row_alternating"] = (yy == H // 2) & (xx % 2 == 0)
    c["column_alternating"] = (xx == W // 2) & (yy % 2 == 0)
    c["checkerboard"] = (yy + xx) % 2 == 0
    comb_rows = (xx % 2 == 0) | (yy == H - 1)      # teeth joined along the last row only: the equivalence is found last
    comb_cols = (yy % 2 == 0) | (xx == W - 1)
    c["comb_last_row"], c["comb_first_row"] = comb_rows, comb_rows[::-1].copy()
    c["comb_last_column"], c["comb_first_column"] = comb_cols, comb_cols[:, ::-1].copy()
    c["spiral"], c["serpentine"] = spiral(H, W), serpentine(H, W)
    c["corner_main"], c["corner_anti"] = corner_blocks(H, W, False), corner_blocks(H, W, True)
    c["rings"] = rings(H, W)
    for d in DENSITIES:
        c[f"random_{d}"] = random_mask(H, W, d)
    return c


@functools.lru_cache(maxsize=None)
def stack(H, W):
    """-> names, masks (n, H, W) bool: every content of one size in one call (one of them empty, all of them different)."""
    c = contents(H, W)
    masks = np.stack(list(c.values()))
    masks.setflags(write=False)
    return tuple(c), masks


@functools.lru_cache(maxsize=None)
def host_labels(H, W, connectivity):
    """The statement's labels and counts of stack(H, W): computed once, shared, read-only."""
    labels, count = segment.label_host(stack(H, W)[1], connectivity)
    labels.setflags(write=False)
    count.setflags(write=False)
    return labels, count


def random_images(C, H, W, channels, seed=0):
    """Seeded colour images: a third of the pixels anywhere in the cube, a third grey or nearly grey, a third dark: every branch of the hue."""
    rng = np.random.default_rng([seed, H, W, channels])
    img = rng.integers(0, 256, (C, H, W, channels), dtype=np.uint8)
    kind = rng.integers(0, 3, (C, H, W))
    grey = rng.integers(0, 256, (C, H, W, 1), dtype=np.uint8)
    near = np.clip(grey.astype(np.int32) + rng.integers(-2, 3, (C, H, W, 3)), 0, 255).astype(np.uint8)
    img[..., :3] = np.where((kind == 1)[..., None], near, img[..., :3])
    img[..., :3] = np.where((kind == 2)[..., None], img[..., :3] // 16, img[..., :3])
    return img


KEY_SETS = {
    1: [segment.ColorKey(100, 200, 40, 255, 30, 255)],
    3: [segment.ColorKey(330, 20, 10, 255, 10, 255), segment.ColorKey.exact(viz.TABLE_COLOR), segment.ColorKey(0, 359, 0, 30, 60, 170)],      # the first wraps
    8: [segment.ColorKey(40 * k, 40 * k + 15, 20 * k, 255, 0, 255 - 10 * k) for k in range(7)] + [segment.ColorKey(350, 5, 0, 255, 0, 255)],
}
OBJECT_COLORS = (viz.PALETTE[0], viz.PALETTE[3])
OBJECT_KEYS = [segment.ColorKey.exact(c) for c in OBJECT_COLORS]
TABLE_KEYS = [segment.ColorKey.exact(viz.TABLE_COLOR)]
GREY_KEYS = [segment.ColorKey(0, 359, 0, 30, 60, 170)]      # the loose table key


def rgb_of(color):
    return (color >> 16) & 255, (color >> 8) & 255, color & 255


def painted(table, obj_a, obj_b, channels=4):
    """(C, H, W) bool masks -> (C, H, W, channels) uint8: the void, then the table, then two object colours painted over it in this order."""
    img = np.zeros(table.shape + (channels,), np.uint8)
    img[..., 3:] = 255
    for m, color in ((table, viz.TABLE_COLOR), (obj_a, OBJECT_COLORS[0]), (obj_b, OBJECT_COLORS[1])):
        img[..., :3] = np.where(m[..., None], np.array(rgb_of(color), np.uint8), img[..., :3])
    return img
