"""Baseline JPEG frames and Motion-JPEG (AVI) videos of the records: what the reference ends every record with -- `rgb_vis.mp4`
at 1 fps (src/planning/plan.py:328-339), `pred.mp4` / `gt.mp4` / `both.mp4` at 10 fps and per-step `.jpg` images (src/dynamics/rollout/
rollout.py:194-203, graph.py:163-225) -- from the standard library and numpy alone.  What it is NOT: no mp4 / H.264, no inter-frame coding, no
optimised or progressive Huffman tables, no audio, no OpenDML (a file stays under 2^31 - 1 bytes).

Two paths, one result.  `jpeg_scan_host` is the statement of the arithmetic, in numpy; `DeviceEncoder` is one call of csrc/ag_jpeg.hip (five
launches) and returns the same bytes.  Everything is integer arithmetic; `>>` is the arithmetic shift (floor).
Colour, per pixel (JFIF full range, 16-bit fixed point, ONE rounding rule: add 32768, shift right by 16; then clamp to 0 .. 255):
  Y  = ( 19595 R + 38470 G +  7471 B                + 32768) >> 16
  Cb = (-11059 R - 21709 G + 32768 B + (128 << 16)  + 32768) >> 16
  Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16)  + 32768) >> 16      (only Cb, Cr = 256 at B or R = 255 over G = 0 meet the clamp)
Subsampling: "444" has an MCU of 8 x 8 pixels with the blocks Y, Cb, Cr; "420" an MCU of 16 x 16 with Y00, Y01, Y10, Y11 (row-major 8 x 8
quarters), Cb, Cr, a chroma sample being (a + b + c + d + 2) >> 2 of the 2 x 2 clamped Cb (Cr) values.  A pixel past the image's last column or
row is the last column's or row's (the image is extended to whole MCUs by repetition).  MCUs go row by row.
Forward DCT of a block x (8 x 8, sample - 128, so -128 .. 127), with the matrix M[k][n] = round(2^13 a_k cos((2 n + 1) k pi / 16)), a_0 =
sqrt(1/8), a_k = 1/2, written out below as DCT_M:
  t[y][k] = ((sum_n M[k][n] x[y][n]) + 512) >> 10            rows:    the coefficient times 2^3
  u[j][k] = sum_y M[j][y] t[y][k]                            columns: the coefficient times 2^16
  int32: a row of M sums to at most 23 168 in magnitude (rows 0 and 4: 8 * 2 896), so |sum_n| <= 23 168 * 128 = 2 965 504 < 2^22 and |t| <= 2 897;
  |u| <= 23 168 * 2 897 = 67 117 696 < 2^27; the quantiser adds at most 255 * 2^15 = 8 355 840: < 7.6e7 < 2^31.  tests/test_jpeg_cpu.py holds
  the sign patterns that maximise each stage to Python's unbounded integers, and the largest coefficient (+127 / -128 over row 4's signs in both
  directions: 1 020) to the 1 023 that Huffman category 10 (AC) and, as a difference of two, category 11 (DC) can carry.
Quantisation: the Annex K luminance (Y) and chrominance (Cb, Cr) tables scaled by `quality` 1 .. 100 with the IJG rule -- s = 5000 // quality
below 50, 200 - 2 quality from 50 on; entry = (base s + 50) // 100 clamped to 1 .. 255 -- and q = sign(u) ((|u| + (d >> 1)) // d), d = entry << 16
(to nearest, halves away from zero, symmetric in sign).
Entropy coding: baseline Huffman with the four Annex K tables; per block the DC difference to the previous block of the same component (0 at the
start of a restart interval) as category + amplitude, then the AC coefficients in zig-zag order as (run, category) + amplitude with ZRL (0xF0) for
every 16 zeros in front of a coefficient, and EOB (0x00) unless coefficient 63 is non-zero.  The amplitude of v < 0 is v - 1 in `category` bits.
Restart intervals: one every `restart` MCUs; the segment is padded with 1-bits to a byte, every 0xFF data byte is followed by 0x00, and RSTm
(0xFF, 0xD0 + m, m counting from 0 mod 8) goes between segments, not after the last.  `restart` is 1 .. MAX_RESTART.
MAX_RESTART = 16 (AG_JPEG_MAX_RESTART): a block is at most 11 + 11 bits of DC (the longest DC code and the largest category) and 63 * (16 + 10)
of AC = 1 660 bits < BLOCK_BYTES = 208 bytes before stuffing, twice that after; the kernel keeps a segment's UNSTUFFED bits in LDS, 16 MCUs * 6
blocks * 208 = 19 968 bytes, a third of the 64 KiB a workgroup gets without asking and 8 resident workgroups per CU; a segment's slot in the
output is 2 * 208 * blocks + 2 (the marker) bytes.
"""
import struct
from fractions import Fraction

import numpy as np

MAX_RESTART = 16           # AG_JPEG_MAX_RESTART
BLOCK_BYTES = 208          # AG_JPEG_BLOCK_BYTES: an upper bound on one block's entropy-coded bytes before stuffing
MAX_SIDE = 4096            # AG_RENDER_MAX_SIDE
SUBSAMPLING = {"444": 0, "420": 1}      # AG_JPEG_444, AG_JPEG_420
FRAME_BUDGET = 1 << 30     # bytes of scratch and output per DeviceEncoder unless the caller says otherwise

DCT_M = np.array([[2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896],
                  [4017, 3406, 2276, 799, -799, -2276, -3406, -4017],
                  [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784],
                  [3406, -799, -4017, -2276, 2276, 4017, 799, -3406],
                  [2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896],
                  [2276, -4017, 799, 3406, -3406, -799, 4017, -2276],
                  [1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567],
                  [799, -2276, 3406, -4017, 4017, -3406, 2276, -799]], np.int32)
# natural (row-major) index of the coefficient at zig-zag position i
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
                   57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], np.int64)
# ITU-T T.81 Annex K.1, natural order
QUANT_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                       18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                       72, 92, 95, 98, 112, 100, 103, 99], np.int64)
QUANT_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                        + [99] * 32, np.int64)
# ITU-T T.81 Annex K.3: (codes of each length 1 .. 16, the symbols in code order) of the DC and AC tables, luminance then chrominance
_AC_TAIL = [0x10 * r + s for r in range(16) for s in range(1, 11)]      # (the tables' last rows are runs in order: only their heads differ)
HUFF_DC = (([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))), ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))))
HUFF_AC = (([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
            [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
             0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
             0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
             0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
             0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
             0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
             0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]),
           ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
            [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
             0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
             0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
             0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
             0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
             0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
             0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]))
assert all(sum(b) == len(v) for b, v in HUFF_DC + HUFF_AC) and all(sorted(v) == sorted([0x00, 0xF0] + _AC_TAIL) for _, v in HUFF_AC)


def huffman_codes(bits, vals):
    """T.81 Annex C: codes in order of length, counting up -> code (256,) and length (256,) int64 by symbol, length 0 for an absent symbol."""
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    c, at = 0, 0
    for n, count in enumerate(bits, 1):
        for _ in range(count):
            code[vals[at]], length[vals[at]] = c, n
            c, at = c + 1, at + 1
        c <<= 1
    return code, length


DC_CODES = tuple(huffman_codes(*t) for t in HUFF_DC)      # [0] luminance, [1] chrominance
AC_CODES = tuple(huffman_codes(*t) for t in HUFF_AC)


def quant_tables(quality):
    """-> (luminance, chrominance) (64,) int64 in natural order (module text: the IJG rule)."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError("jpeg: quality outside 1 .. 100")
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (QUANT_LUMA, QUANT_CHROMA))


def _check(H, W, quality, subsampling, restart):
    if not (1 <= int(H) <= MAX_SIDE and 1 <= int(W) <= MAX_SIDE):
        raise ValueError(f"jpeg: H, W outside 1 .. {MAX_SIDE}")
    if subsampling not in SUBSAMPLING:
        raise ValueError('jpeg: subsampling is "444" or "420"')
    if not 1 <= int(restart) <= MAX_RESTART:
        raise ValueError(f"jpeg: restart outside 1 .. {MAX_RESTART}")
    quant_tables(quality)


def geometry(H, W, subsampling, restart):
    """-> MCU side, blocks per MCU, MCU rows, MCU columns, segments per frame."""
    side, bpm = (8, 3) if subsampling == "444" else (16, 6)
    my, mx = -(-int(H) // side), -(-int(W) // side)
    return side, bpm, my, mx, -(-(my * mx) // int(restart))


def segment_bound(subsampling, restart):
    """The bytes a restart segment can take at most, stuffing and marker included (module text): a segment's slot."""
    return 2 * BLOCK_BYTES * (3 if subsampling == "444" else 6) * int(restart) + 2


def out_bytes(F, H, W, subsampling, restart):
    """ag_jpeg_out_bytes: F * segments * segment_bound."""
    return int(F) * geometry(H, W, subsampling, restart)[4] * segment_bound(subsampling, restart)


def scratch_bytes(F, H, W, subsampling, restart):
    """ag_jpeg_scratch_bytes, each part rounded up to 256 bytes: the coefficients (int16, 64 per block), a slot per segment, and per segment its
    length and its offset (int32), and the scan's sums (G // 256 + 2 int32), G = F * segments."""
    _, bpm, my, mx, nseg = geometry(H, W, subsampling, restart)
    G = int(F) * nseg
    up = lambda n: -(-n // 256) * 256      # noqa: E731
    return up(int(F) * my * mx * bpm * 128) + up(G * segment_bound(subsampling, restart)) + 2 * up(4 * G) + up(4 * (G // 256 + 2))


def frames_per_launch(H, W, subsampling="420", restart=8, budget=FRAME_BUDGET):
    """How many frames one DeviceEncoder takes under the byte budget (scratch and output, both worst case), at least 1."""
    return max(1, int(budget) // (scratch_bytes(1, H, W, subsampling, restart) + out_bytes(1, H, W, subsampling, restart)))


# ---------------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------------
def _host(a):
    return a.detach().cpu().numpy() if type(a).__module__.startswith("torch") else np.asarray(a)


def _frames(images):
    img = _host(images)
    if img.ndim == 3:
        img = img[None]
    if img.dtype != np.uint8 or img.ndim != 4 or img.shape[3] not in (3, 4) or img.shape[0] < 1:
        raise ValueError("jpeg: images are (F, H, W, 3 or 4) uint8, F >= 1")
    return img


def ycbcr_host(rgb):
    """(..., 3 or 4) uint8 -> Y, Cb, Cr int32 arrays (module text)."""
    r, g, b = (rgb[..., c].astype(np.int32) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32768) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32768) >> 16
    return tuple(np.clip(p, 0, 255) for p in (y, cb, cr))


def fdct_host(x):
    """(..., 8, 8) int32 samples minus 128 -> u (..., 8, 8) int32, the coefficients times 2^16 (module text)."""
    x = np.asarray(x, np.int32)
    t = (np.matmul(x, DCT_M.T) + np.int32(512)) >> 10
    return np.matmul(DCT_M, t)


def coefficients_host(images, quality, subsampling):
    """-> (F, blocks, 64) int32 quantised coefficients in zig-zag order, the blocks in scan order, and the blocks per MCU."""
    img = _frames(images)
    F, H, W = img.shape[:3]
    side, bpm, my, mx, _ = geometry(H, W, subsampling, 1)
    planes = [np.pad(p, ((0, 0), (0, my * side - H), (0, mx * side - W)), mode="edge") for p in ycbcr_host(img)]
    tiles = lambda p, k: p.reshape(F, my, k, 8, mx, k, 8).transpose(0, 1, 4, 2, 5, 3, 6).reshape(F, my, mx, k * k, 8, 8)      # noqa: E731
    if subsampling == "420":
        planes[1:] = [(p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2] + 2) >> 2 for p in planes[1:]]
    blocks = np.concatenate([tiles(planes[0], side // 8), tiles(planes[1], 1), tiles(planes[2], 1)], 3).reshape(F, my * mx * bpm, 8, 8)
    u = fdct_host(blocks - np.int32(128))
    lum, chrom = quant_tables(quality)
    d = (np.stack([lum] * (bpm - 2) + [chrom] * 2).astype(np.int32) << 16).reshape(bpm, 8, 8)
    d = np.tile(d, (my * mx, 1, 1))[None]
    q = np.sign(u) * ((np.abs(u) + (d >> 1)) // d)
    return q.reshape(F, -1, 64)[:, :, ZIGZAG].astype(np.int32), bpm


def _category(v):
    """The number of bits of |v| (0 for 0), by comparisons."""
    a = np.abs(v)
    return sum((a >= (1 << i)).astype(np.int64) for i in range(12))


def _scan_of_frame(coefs, bpm, restart, counters):
    """One frame's (blocks, 64) coefficients -> its scan bytes (module text).  Every coded item is an EVENT (bits, their number <= 59) with a sort
    key block * 66 + slot: slot 0 the DC, k the AC coefficient k with the ZRLs in front of it, 64 the EOB, 65 the segment's padding."""
    nblk = len(coefs)
    block = np.arange(nblk, dtype=np.int64)
    slot = block % bpm
    chroma = (slot >= bpm - 2).astype(np.int64)
    comp = np.where(chroma == 1, slot - (bpm - 3), 0)
    seg = block // (bpm * restart)
    nseg = int(seg[-1]) + 1
    # DC: the difference to the block of the same component before, 0 at a segment's start
    diff = coefs[:, 0].astype(np.int64).copy()
    for c in range(3):
        idx = np.nonzero(comp == c)[0]
        prev = np.concatenate([[0], coefs[idx[:-1], 0]])
        prev[np.concatenate([[True], seg[idx[1:]] != seg[idx[:-1]]])] = 0
        diff[idx] -= prev
    size = _category(diff)
    amp = np.where(diff < 0, diff + (1 << size) - 1, diff)
    dc_code, dc_len = (np.stack([t[i] for t in DC_CODES]) for i in (0, 1))
    keys = [block * 66]
    vals = [(dc_code[chroma, size] << size) | amp]
    lens = [dc_len[chroma, size] + size]
    counters["dc_category"] += np.bincount(size, minlength=12)
    # AC
    b, k = np.nonzero(coefs[:, 1:])
    k = k + 1
    prev = np.zeros_like(k)
    prev[1:] = np.where(b[1:] != b[:-1], 0, k[:-1])
    run = k - prev - 1
    v = coefs[b, k].astype(np.int64)
    size = _category(v)
    amp = np.where(v < 0, v + (1 << size) - 1, v)
    ac_code, ac_len = (np.stack([t[i] for t in AC_CODES]) for i in (0, 1))
    tb = chroma[b]
    sym = ((run & 15) << 4) | size
    zc, zl, nz = ac_code[tb, 0xF0], ac_len[tb, 0xF0], run >> 4
    zrl = np.where(nz >= 1, zc, 0) | np.where(nz >= 2, zc << zl, 0) | np.where(nz >= 3, zc << (2 * zl), 0)
    n = ac_len[tb, sym] + size
    keys.append(b * 66 + k)
    vals.append((zrl << n) | (ac_code[tb, sym] << size) | amp)
    lens.append(nz * zl + n)
    counters["zrl"] += int(nz.sum())
    counters["ac_category"] += np.bincount(size, minlength=11)
    # EOB
    e = np.nonzero(coefs[:, 63] == 0)[0]
    keys.append(e * 66 + 64)
    vals.append(ac_code[chroma[e], 0])
    lens.append(ac_len[chroma[e], 0])
    counters["eob"] += len(e)
    counters["eob_only_dc0"] += int(((coefs[:, 1:] == 0).all(1) & (diff == 0)).sum())
    # padding with 1-bits to a byte, per segment
    seg_bits = sum(np.bincount(seg[kk // 66], weights=ll, minlength=nseg).astype(np.int64) for kk, ll in zip(keys, lens))
    pad = (-seg_bits) % 8
    last = np.minimum((np.arange(nseg, dtype=np.int64) + 1) * bpm * restart, nblk) - 1
    keys.append(last * 66 + 65)
    vals.append((1 << pad) - 1)
    lens.append(pad)
    key, val, n = np.concatenate(keys), np.concatenate(vals).astype(np.int64), np.concatenate(lens).astype(np.int64)
    order = np.argsort(key, kind="stable")
    val, n = val[order], n[order]
    # the bits, most significant first
    start = np.cumsum(n) - n
    which = np.repeat(np.arange(len(n)), n)
    j = np.arange(int(n.sum()), dtype=np.int64) - start[which]
    data = np.packbits(((val[which] >> (n[which] - 1 - j)) & 1).astype(np.uint8))
    # stuffing and markers
    seg_len = (seg_bits + pad) // 8
    seg_start = np.cumsum(seg_len) - seg_len
    ff = data == 0xFF
    seg_of = np.repeat(np.arange(nseg), seg_len)
    pos = np.arange(len(data)) + (np.cumsum(ff) - ff) + 2 * seg_of
    out = np.zeros(len(data) + int(ff.sum()) + 2 * (nseg - 1), np.uint8)
    out[pos] = data
    marks = pos[seg_start[1:]] - 2      # (a segment is never empty: its first block has a DC code)
    out[marks] = 0xFF
    out[marks + 1] = 0xD0 + (np.arange(nseg - 1) % 8)
    counters["segments"] += nseg
    counters["rst"] += nseg - 1
    counters["stuffed"] += int(ff.sum())
    counters["pad_ff"] += int(((pad > 0) & (data[seg_start + seg_len - 1] == 0xFF)).sum())
    counters["max_segment_bytes"] = max(counters["max_segment_bytes"], int((seg_len + np.bincount(seg_of, weights=ff, minlength=nseg).astype(np.int64)).max()) + 2)
    return out.tobytes()


def jpeg_scan_host(images, quality=90, subsampling="420", restart=8, debug=False):
    """The statement (module text): images (F, H, W, 3 or 4) uint8 (alpha is ignored) -> the entropy-coded scan of every frame, a list of bytes.
    `debug=True` -> (scans, counters): what was emitted -- zrl, eob, eob_only_dc0 (blocks that are an EOB after a DC difference of 0), rst,
    segments, stuffed (0xFF data bytes), pad_ff (segments whose last, padded byte is 0xFF), dc_category (12,) and ac_category (11,) histograms,
    max_segment_bytes (stuffing and marker included)."""
    img = _frames(images)
    _check(img.shape[1], img.shape[2], quality, subsampling, restart)
    counters = {"zrl": 0, "eob": 0, "eob_only_dc0": 0, "rst": 0, "segments": 0, "stuffed": 0, "pad_ff": 0, "max_segment_bytes": 0,
                "dc_category": np.zeros(12, np.int64), "ac_category": np.zeros(11, np.int64)}
    scans = []
    for f in range(len(img)):      # (frame by frame: the bit expansion of one frame at a time)
        coefs, bpm = coefficients_host(img[f:f + 1], quality, subsampling)
        scans.append(_scan_of_frame(coefs[0], bpm, int(restart), counters))
    return (scans, counters) if debug else scans


# ---------------------------------------------------------------------------------------------------------------------
# the file around the scan
# ---------------------------------------------------------------------------------------------------------------------
def _segment(marker, body):
    return struct.pack(">BBH", 0xFF, marker, len(body) + 2) + body


def jpeg_header(H, W, quality=90, subsampling="420", restart=8):
    """SOI, APP0 (JFIF 1.01, no density), DQT x 2 (zig-zag order), SOF0, DHT x 4, DRI, SOS -> bytes; the scan and EOI follow."""
    _check(H, W, quality, subsampling, restart)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    for i, table in enumerate(quant_tables(quality)):
        out += _segment(0xDB, bytes([i]) + bytes(int(x) for x in table[ZIGZAG]))
    ysamp = 0x11 if subsampling == "444" else 0x22
    out += _segment(0xC0, struct.pack(">BHHB", 8, int(H), int(W), 3) + bytes([1, ysamp, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls, tables in ((0, HUFF_DC), (1, HUFF_AC)):
        for i, (bits, vals) in enumerate(tables):
            out += _segment(0xC4, bytes([(cls << 4) | i]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, struct.pack(">H", int(restart)))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


EOI = b"\xff\xd9"


def encode_jpeg(images, quality=90, subsampling="420", restart=8, device=None):
    """images (F, H, W, 3 or 4) uint8 (or one (H, W, C) image), array or tensor -> a list of bytes, one complete baseline JPEG file per frame.
    device=None is the statement; otherwise one DeviceEncoder built for these frames: the same bytes."""
    if device is None:
        img = _frames(images)
        head = jpeg_header(img.shape[1], img.shape[2], quality, subsampling, restart)
        return [head + scan + EOI for scan in jpeg_scan_host(img, quality, subsampling, restart)]
    import torch
    img = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(_frames(images)))
    img = (img[None] if img.dim() == 3 else img).to(device).contiguous()
    enc = DeviceEncoder(img.shape[1], img.shape[2], img.shape[0], quality, subsampling, restart, channels=img.shape[3], device=device)
    return enc.encode(img)


def write_jpeg(path, image, quality=90, subsampling="420", restart=8, device=None):
    """One (H, W, 3 or 4) uint8 image -> a baseline JPEG file."""
    with open(path, "wb") as fh:
        fh.write(encode_jpeg(image, quality, subsampling, restart, device)[0])


# ---------------------------------------------------------------------------------------------------------------------
# the device path
# ---------------------------------------------------------------------------------------------------------------------
class DeviceEncoder:
    """ag_jpeg_encode with its scratch, its output and its offsets preallocated for up to F frames of H x W x channels (as DeviceCanvas does for
    ag_draw).  `launch(images)` enqueues the five kernels on the current stream (no synchronisation, no allocation: it captures into a HIP graph)
    and returns (out, offsets[:F' + 1]): frame f's scan is out[offsets[f]:offsets[f + 1]]; the next launch overwrites both.  `scans` / `encode`
    add the two host copies -- the F' + 1 offsets, then exactly offsets[F'] bytes -- and return a list of bytes per frame (the scan; the file);
    they take any number of frames, F at a time."""

    def __init__(self, H, W, F=1, quality=90, subsampling="420", restart=8, channels=4, device="cuda:0"):
        import torch
        from . import _lib
        _check(H, W, quality, subsampling, restart)
        if int(F) < 1 or int(channels) not in (3, 4):
            raise ValueError("DeviceEncoder: F < 1 or channels not 3 or 4")
        self.device = torch.device(device)
        self.H, self.W, self.F, self.channels = int(H), int(W), int(F), int(channels)
        self.quality, self.subsampling, self.restart = int(quality), subsampling, int(restart)
        L, sub = _lib.lib(), SUBSAMPLING[subsampling]
        self.scratch_bytes = int(L.ag_jpeg_scratch_bytes(self.F, self.H, self.W, sub, self.restart))
        self.out_bytes = int(L.ag_jpeg_out_bytes(self.F, self.H, self.W, sub, self.restart))
        if self.scratch_bytes == 0 or self.out_bytes == 0 or self.out_bytes > 2 ** 31 - 1:
            raise ValueError(f"DeviceEncoder: {self.F} frames of {self.H} x {self.W} exceed one call (frames_per_launch)")
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=self.device)
        self.out = torch.empty(self.out_bytes, dtype=torch.uint8, device=self.device)
        self.offsets = torch.empty(self.F + 1, dtype=torch.int64, device=self.device)
        self.header = jpeg_header(self.H, self.W, self.quality, subsampling, self.restart)

    def launch(self, images):
        import torch
        from . import _lib
        F = int(images.shape[0]) if images.dim() == 4 else 0
        if (not isinstance(images, torch.Tensor) or images.device != self.device or images.dtype != torch.uint8 or not images.is_contiguous()
                or not 1 <= F <= self.F or tuple(images.shape[1:]) != (self.H, self.W, self.channels)):
            raise ValueError(f"DeviceEncoder: images must be a contiguous uint8 tensor (1 .. {self.F}, {self.H}, {self.W}, {self.channels}) on "
                             f"{self.device}")
        _lib.call("ag_jpeg_encode", self.device, images, F, self.H, self.W, self.channels, self.quality, SUBSAMPLING[self.subsampling], self.restart,
                  self.scratch, self.scratch_bytes, self.out, self.out_bytes, self.offsets)
        return self.out, self.offsets[:F + 1]

    def scans(self, images):
        scans = []
        for i in range(0, int(images.shape[0]), self.F):      # (more frames than it was built for: F at a time)
            out, offsets = self.launch(images[i:i + self.F])
            at = offsets.cpu().numpy()
            data = out[:int(at[-1])].cpu().numpy().tobytes()
            scans += [data[at[f]:at[f + 1]] for f in range(len(at) - 1)]
        return scans

    def encode(self, images):
        return [self.header + scan + EOI for scan in self.scans(images)]


# ---------------------------------------------------------------------------------------------------------------------
# Motion-JPEG in an AVI container
# ---------------------------------------------------------------------------------------------------------------------
AVI_MAX_BYTES = 2 ** 31 - 1


class VideoWriter:
    """A RIFF/AVI file with one MJPG video stream: `hdrl` (`avih`, `strl` = `strh` + `strf`, a BITMAPINFOHEADER), a `movi` list of `00dc` chunks
    (one JPEG file each, padded to even length) and `idx1`.  `add(frames)` takes images (F, H, W, 3 or 4) uint8 -- arrays, or tensors on
    `device` -- and encodes them (device=None: the statement), or a list of bytes, ready JPEG files of this size.  The frame counts and sizes
    are patched at `close`.  fps is carried as rate / scale (0.5 fps = 1 / 2).  A frame that would take the finished file past 2^31 - 1 bytes
    raises ValueError before anything of it is written; the file closes as a valid video of the frames before."""
    _HEAD = 12 + 12 + 8 + 56 + 12 + 8 + 56 + 8 + 40 + 12      # RIFF AVI, LIST hdrl, avih, LIST strl, strh, strf, LIST movi

    def __init__(self, path, H, W, fps, quality=90, subsampling="420", device=None, restart=8):
        _check(H, W, quality, subsampling, restart)
        rate = Fraction(fps).limit_denominator(1000000)
        if rate <= 0:
            raise ValueError("VideoWriter: fps must be positive")
        self.path, self.H, self.W, self.rate, self.scale = path, int(H), int(W), rate.numerator, rate.denominator
        self.quality, self.subsampling, self.restart, self.device = int(quality), subsampling, int(restart), device
        self._index, self._largest, self._encoder = [], 0, None
        self._fh = open(path, "wb")
        self._fh.write(self._head())
        self._bytes = self._HEAD      # the file's length so far

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _head(self):
        n, movi = len(self._index), 4 + sum(8 + size + (size & 1) for _, size in self._index)
        usec = (1000000 * self.scale + self.rate // 2) // self.rate
        avih = struct.pack("<14I", usec, 0, 0, 0x10, n, 0, 1, self._largest, self.W, self.H, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, n, self._largest, 0xFFFFFFFF, 0, 0, 0,
                           self.W, self.H)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.W, self.H, 1, 24, b"MJPG", self.W * self.H * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", 56) + strh + b"strf" + struct.pack("<I", 40) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", 56) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        riff = 4 + 8 + len(hdrl) + 8 + movi + 8 + 16 * n
        return (b"RIFF" + struct.pack("<I", riff) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl + b"LIST" + struct.pack("<I", movi)
                + b"movi")

    def _encode(self, frames):
        if self.device is None:
            return encode_jpeg(frames, self.quality, self.subsampling, self.restart)
        import torch
        img = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(_frames(frames)))
        img = (img[None] if img.dim() == 3 else img).to(self.device).contiguous()
        enc = self._encoder
        if enc is None or enc.channels != img.shape[3]:
            cap = min(max(int(img.shape[0]), 1), frames_per_launch(self.H, self.W, self.subsampling, self.restart))
            enc = self._encoder = DeviceEncoder(self.H, self.W, cap, self.quality, self.subsampling, self.restart, int(img.shape[3]), self.device)
        return enc.encode(img)

    def add(self, frames):
        if self._fh is None:
            raise ValueError("VideoWriter: closed")
        if not (isinstance(frames, (list, tuple)) and all(isinstance(x, (bytes, bytearray)) for x in frames)):
            shape = tuple(frames.shape)
            if shape[-3:-1] != (self.H, self.W):
                raise ValueError(f"VideoWriter: frames of {shape[-3:-1]}, the video is {(self.H, self.W)}")
            frames = self._encode(frames)
        for data in frames:
            size = len(data)
            if self._bytes + 8 + size + (size & 1) + 8 + 16 * (len(self._index) + 1) > AVI_MAX_BYTES:
                raise ValueError("VideoWriter: the file would pass 2^31 - 1 bytes (no OpenDML): close it and start another")
            self._fh.write(b"00dc" + struct.pack("<I", size) + bytes(data) + b"\0" * (size & 1))
            self._index.append((self._bytes - (self._HEAD - 4), size))      # the chunk's offset from the `movi` word
            self._bytes += 8 + size + (size & 1)
            self._largest = max(self._largest, size)

    def close(self):
        if self._fh is None:
            return
        self._fh.write(b"idx1" + struct.pack("<I", 16 * len(self._index))
                       + b"".join(b"00dc" + struct.pack("<III", 0x10, at, size) for at, size in self._index))
        self._fh.seek(0)
        self._fh.write(self._head())
        self._fh.close()
        self._fh = None


def avi_frames(path):
    """The `00dc` chunks of a file of VideoWriter, in order -> a list of bytes (JPEG files)."""
    data = open(path, "rb").read()
    if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError("avi_frames: not an AVI file")
    at = data.index(b"movi", 12) + 4
    end = at - 4 + struct.unpack("<I", data[at - 8:at - 4])[0]
    out = []
    while at < end:
        size = struct.unpack("<I", data[at + 4:at + 8])[0]
        if data[at:at + 4] == b"00dc":
            out.append(data[at + 8:at + 8 + size])
        at += 8 + size + (size & 1)
    return out
