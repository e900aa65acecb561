"""Images shared by tests/test_jpeg_cpu.py and tests/test_jpeg.py: the pictures the encoder is held to PIL on, and the inputs that enter every
coding path (chosen on the CPU from the statement's counters; test_jpeg_cpu.py asserts what each one enters)."""
import math

import numpy as np

from adaptigraph_amd import viz
from viz_cases import awkward_list, camera

PAD_FF_SEED = 20      # found by search over seeds 0 .. 1999: an 8 x 8 noise image whose only segment ends in a padded 0xFF byte (quality 50, 4:4:4)


def gray(a):
    return np.repeat(np.asarray(a, np.uint8)[..., None], 3, -1)


def gradient(H, W):
    """A smooth gradient with a saturated rectangle."""
    yy, xx = np.mgrid[:H, :W]
    img = np.stack([xx * 255 // max(W - 1, 1), yy * 255 // max(H - 1, 1), (xx + yy) * 255 // max(H + W - 2, 1)], -1).astype(np.uint8)
    img[H // 4:H // 2, W // 4:3 * W // 4] = (255, 0, 255)
    return img


def drawn(H, W):
    """A drawn frame: the awkward display list of viz_cases over a flat background, RGBA as ag_draw writes it."""
    cams = camera(H, W)
    pts, prims, styles = awkward_list(np.random.default_rng(3), 40, H, W, cams)
    return viz.draw_host(pts, prims, styles, [[0, 0, len(prims), 0]], cams, H, W, 128, color0=0x6E6E73)[0]


def noise(H, W, seed=1, channels=3):
    return np.random.default_rng(seed).integers(0, 256, (H, W, channels), dtype=np.uint8)


def pictures(H, W):
    """name -> (H, W, 3 or 4) uint8: what the fidelity tests encode."""
    return {"gradient": gradient(H, W), "drawn": drawn(H, W), "noise": noise(H, W)}


def highest_frequency(amplitude=22):
    """6 blocks that are the basis function (7, 7) of the DCT at a small amplitude: at quality 100 the coefficient at zig-zag position 63 sits behind
    runs of 16 zeros and more."""
    b = np.cos((2 * np.arange(8) + 1) * 7 * math.pi / 16)
    return gray(np.tile(np.clip(np.round(128 + amplitude * np.outer(b, b)), 0, 255), (2, 3)))


def checkerboard(H=16, W=24):
    yy, xx = np.mgrid[:H, :W]
    return gray(((yy + xx) % 2) * 255)


def block_board(H=16, W=24):
    """Alternating black and white 8 x 8 blocks."""
    yy, xx = np.mgrid[:H, :W]
    return gray(((yy // 8 + xx // 8) % 2) * 255)


def content_cases():
    """name -> (images (F, H, W, C), quality, subsampling, restart): one per coding path (test_jpeg_cpu.py says which)."""
    return {
        "zrl": (highest_frequency()[None], 100, "444", 8),
        "ac_category_10": (checkerboard()[None], 100, "444", 8),
        "dc_category_11": (block_board()[None], 100, "444", 8),
        "dc_category_11_420": (block_board(32, 48)[None], 100, "420", 8),
        "stuffing": (noise(33, 47)[None], 100, "420", 1),
        "pad_ff": (noise(8, 8, PAD_FF_SEED)[None], 50, "444", 1),
        "constant": (np.full((1, 20, 40, 3), 77, np.uint8), 90, "420", 2),
        "rst_wraps": (noise(24, 40, 5)[None], 50, "444", 1),
        "one_segment": (noise(16, 16, 6)[None], 90, "420", 8),
        "quality_1": (gradient(33, 47)[None], 1, "420", 3),
        "quality_49": (gradient(33, 47)[None], 49, "444", 3),
        "quality_50": (gradient(33, 47)[None], 50, "420", 8),
        "quality_100": (drawn(33, 47)[None], 100, "420", 16),
        "worst_case": (noise(64, 64, 7)[None], 100, "420", 16),
    }
