"""The JPEG statement (adaptigraph_amd/jpeg.py:jpeg_scan_host), the files and videos around it and ag_jpeg_encode's argument checks: no GPU."""
import ctypes
import io
import os
import re
import struct
import warnings

import numpy as np
import pytest

from adaptigraph_amd import _lib, jpeg, viz
from jpeg_cases import PAD_FF_SEED, content_cases, noise, pictures
from viz_cases import StubPlanner, rope_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Ours against PIL's own file with the same tables, subsampling and restart interval (DESIGN.md §8.17 records the measurement): the PSNR gap is
# what two integer pipelines differ by in colour and DCT rounding (and, in 4:2:0, in how the 2 x 2 mean is rounded and an odd side is
# extended); the length gap likewise, the Huffman tables and the restart overhead being the same.  Worst gaps seen over the 24 settings below
# x 3 pictures: see the figures printed by the test; the margins stand just above them.
PSNR_MARGIN_DB = 0.1      # worst seen: 0.065 dB (the gradient, 33 x 47, quality 90, 4:4:4)
LENGTH_MARGIN = 0.05      # worst seen: + 4.3 % (the drawn frame, 33 x 47, quality 50, 4:2:0; at most + 0.3 % in 4:4:4 and at 64 x 64)


def psnr(a, b):
    mse = float(((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).mean())
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def pil_decode(data):
    Image = pytest.importorskip("PIL.Image")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with Image.open(io.BytesIO(data)) as im:
            im.load()
            return np.asarray(im.convert("RGB")), im.size


def pil_encode(image, quality, subsampling, restart):
    Image = pytest.importorskip("PIL.Image")
    lum, chrom = jpeg.quant_tables(quality)
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(image[..., :3])).save(buf, "JPEG", qtables=[[int(x) for x in lum], [int(x) for x in chrom]],
                                                               subsampling={"444": 0, "420": 2}[subsampling], restart_marker_blocks=restart,
                                                               optimize=False)
    return buf.getvalue()


def segments_of(data, marker):
    """The bodies of the header segments with this marker, in order."""
    out, at = [], 2
    while data[at + 1] != 0xDA:
        n = struct.unpack(">H", data[at + 2:at + 4])[0]
        if data[at + 1] == marker:
            out.append(data[at + 4:at + 2 + n])
        at += 2 + n
    return out


# ------------------------------------------------------------------------------------------------------ fidelity
@pytest.mark.parametrize("H,W", [(33, 47), (64, 64)])
@pytest.mark.parametrize("subsampling", ["444", "420"])
@pytest.mark.parametrize("quality", [50, 90])
def test_files_decode_in_pil_and_are_as_faithful_as_its_own(H, W, subsampling, quality):
    pytest.importorskip("PIL")
    for name, image in pictures(H, W).items():
        for restart in (1, 8):
            ours = jpeg.encode_jpeg(image[None], quality, subsampling, restart)[0]
            decoded, size = pil_decode(ours)                                          # without a warning
            assert size == (W, H)
            theirs = pil_encode(image, quality, subsampling, restart)
            assert segments_of(ours, 0xDB) == segments_of(theirs, 0xDB)               # the same quantisation tables,
            assert sorted(segments_of(ours, 0xC4)) == sorted(segments_of(theirs, 0xC4))      # Huffman tables
            assert segments_of(ours, 0xDD) == segments_of(theirs, 0xDD) and segments_of(ours, 0xC0) == segments_of(theirs, 0xC0)      # DRI, SOF0
            p_ours, p_theirs = psnr(decoded, image[..., :3]), psnr(pil_decode(theirs)[0], image[..., :3])
            print(f"{name} {H}x{W} q{quality} {subsampling} restart {restart}: PSNR ours {p_ours:.3f} PIL {p_theirs:.3f} gap {p_theirs - p_ours:+.3f} dB; "
                  f"bytes ours {len(ours)} PIL {len(theirs)} ({len(ours) / len(theirs) - 1:+.4f})")
            assert p_ours >= p_theirs - PSNR_MARGIN_DB, (name, restart)
            assert len(ours) <= len(theirs) * (1 + LENGTH_MARGIN), (name, restart)


def test_alpha_is_ignored_and_one_image_is_a_batch_of_one():
    rgba = noise(17, 9, 2, 4)
    a = jpeg.encode_jpeg(rgba[None], 75, "420", 3)
    assert a == jpeg.encode_jpeg(rgba[..., :3], 75, "420", 3) and len(a) == 1
    other = rgba.copy()
    other[..., 3] = 0
    assert jpeg.jpeg_scan_host(other[None], 75, "420", 3) == jpeg.jpeg_scan_host(rgba[None], 75, "420", 3)
    two = jpeg.jpeg_scan_host(np.stack([rgba, other[::-1].copy()]), 75, "444", 2)
    assert two[0] == jpeg.jpeg_scan_host(rgba[None], 75, "444", 2)[0] and two[1] != two[0]
    for bad in (dict(quality=0), dict(quality=101), dict(subsampling="422"), dict(restart=0), dict(restart=jpeg.MAX_RESTART + 1)):
        with pytest.raises(ValueError):
            jpeg.jpeg_scan_host(rgba[None], **bad)
    with pytest.raises(ValueError):
        jpeg.jpeg_scan_host(rgba[None].astype(np.float32))


# ------------------------------------------------------------------------------------------------------ every coding path
def counters_of(name):
    images, quality, subsampling, restart = content_cases()[name]
    scans, c = jpeg.jpeg_scan_host(images, quality, subsampling, restart, debug=True)
    return scans, c, images, restart


def test_every_coding_path_is_entered():
    scans, c, _, _ = counters_of("zrl")
    assert c["zrl"] > 0 and c["zrl"] >= 3 * 6                                          # three ZRLs in front of one coefficient: a 59-bit event
    assert counters_of("ac_category_10")[1]["ac_category"][10] > 0
    assert counters_of("dc_category_11")[1]["dc_category"][11] > 0 and counters_of("dc_category_11_420")[1]["dc_category"][11] > 0
    scans, c, _, _ = counters_of("stuffing")
    assert c["stuffed"] > 0 and b"\xff\x00" in scans[0] and scans[0].count(b"\xff\x00") >= c["stuffed"]
    scans, c, _, _ = counters_of("pad_ff")
    assert c["pad_ff"] == 1 and c["segments"] == 1 and scans[0].endswith(b"\xff\x00") and PAD_FF_SEED == 20
    scans, c, images, restart = counters_of("constant")
    blocks = 6 * 2 * 3                                                                 # 20 x 40 in 4:2:0: 2 x 3 MCUs of six blocks
    assert c["eob"] == blocks and c["ac_category"].sum() == 0 and c["segments"] == 3
    assert c["eob_only_dc0"] == blocks - c["segments"] and c["dc_category"][0] == c["eob_only_dc0"]      # all but each segment's first Y (grey: Cb = Cr = 128, a DC of 0)
    scans, c, _, _ = counters_of("rst_wraps")
    assert c["segments"] == 15 > 8 and c["rst"] == 14
    marks = [m.start() for m in re.finditer(b"\xff[\xd0-\xd7]", scans[0])]
    assert [scans[0][m + 1] - 0xD0 for m in marks] == [i % 8 for i in range(14)] and not scans[0].endswith(b"\xff\xd5")
    scans, c, _, restart = counters_of("one_segment")
    assert restart > 1 and c["segments"] == 1 and c["rst"] == 0 and not re.search(b"\xff[\xd0-\xd7]", scans[0])
    tables = {q: jpeg.quant_tables(q) for q in (1, 49, 50, 100)}
    assert all((t == 255).all() for t in tables[1]) and all((t == 1).all() for t in tables[100])      # both clamps
    assert tables[49][0][0] == (16 * (5000 // 49) + 50) // 100 == 16 and tables[50][0][0] == 16 and tables[49][0][63] == 101 and tables[50][0][63] == 99
    for name in ("quality_1", "quality_49", "quality_50", "quality_100"):
        scans, c, images, _ = counters_of(name)
        assert c["eob"] > 0 and len(scans) == 1
    assert counters_of("quality_1")[1]["ac_category"].sum() < counters_of("quality_100")[1]["ac_category"].sum()


def test_worst_case_bound_holds_by_arithmetic_and_on_noise():
    dc = max(int(length[:12].max()) for _, length in jpeg.DC_CODES) + 11               # the longest DC code and the largest category
    ac = max(int(length.max()) for _, length in jpeg.AC_CODES) + 10
    assert (dc, ac) == (22, 26) and dc + 63 * ac == 1660 <= 8 * jpeg.BLOCK_BYTES - 4
    assert all(int(length[0xF0]) <= 11 for _, length in jpeg.AC_CODES) and 3 * 11 + ac == 59 < 64      # an event fits 64 bits
    assert jpeg.segment_bound("420", jpeg.MAX_RESTART) == 2 * 208 * 96 + 2 and jpeg.segment_bound("444", 1) == 2 * 208 * 3 + 2
    assert jpeg.MAX_RESTART * 6 * jpeg.BLOCK_BYTES == 19968 < 65536                     # the kernel's bit buffer
    scans, c, images, restart = counters_of("worst_case")
    assert restart == jpeg.MAX_RESTART and c["stuffed"] > 0
    assert 96 * 60 < c["max_segment_bytes"] <= jpeg.segment_bound("420", restart)   # (a real load: over 60 bytes a block)
    assert len(scans[0]) <= jpeg.out_bytes(1, 64, 64, "420", restart)


def python_fdct(x):
    """fdct_host in Python's unbounded integers -> u and the largest magnitude of any intermediate."""
    M = [[int(v) for v in row] for row in jpeg.DCT_M]
    big = 0
    t = [[0] * 8 for _ in range(8)]
    for y in range(8):
        for k in range(8):
            s = sum(M[k][n] * int(x[y][n]) for n in range(8))
            big = max(big, abs(s) + 512)
            t[y][k] = (s + 512) >> 10
    u = [[sum(M[j][y] * t[y][k] for y in range(8)) for k in range(8)] for j in range(8)]
    return u, max(big, max(abs(v) for row in u for v in row))


def test_dct_stays_inside_int32_at_the_extreme_inputs():
    M = jpeg.DCT_M.astype(np.int64)
    assert int(np.abs(M).sum(1).max()) == 23168 and 23168 * 128 + 512 < 2 ** 22 and 23168 * 2897 + 255 * 2 ** 15 < 2 ** 31
    largest, worst_q = 0, 0
    for j in range(8):
        for k in range(8):
            sign = np.sign(np.outer(M[j], M[k]))
            for x in (np.where(sign > 0, 127, -128), np.where(sign > 0, -128, 127)):      # the patterns that maximise coefficient (j, k), both signs
                u, big = python_fdct(x.tolist())
                got = jpeg.fdct_host(x[None].astype(np.int32))[0]
                assert got.dtype == np.int32 and got.tolist() == u, (j, k)
                largest = max(largest, big)
                q = max((abs(v) + 32768) >> 16 for a, row in enumerate(u) for b, v in enumerate(row) if (a, b) != (0, 0))      # AC, at entry 1
                worst_q = max(worst_q, q)
                if (j, k) == (4, 4):
                    assert q == 1020
    for x in (np.full((8, 8), -128), np.full((8, 8), 127)):                             # the DC's extremes
        u, big = python_fdct(x.tolist())
        largest = max(largest, big)
        assert jpeg.fdct_host(x[None].astype(np.int32))[0].tolist() == u and (abs(u[0][0]) + 32768) >> 16 in (1024, 1016)
    assert largest + 255 * 2 ** 15 < 2 ** 31 and largest < 2 ** 27
    assert 1020 <= worst_q <= 1023 and 1024 + 1016 < 2048                               # AC category <= 10, a DC difference's <= 11


def test_kernel_tables_are_the_statement_s():
    src = open(os.path.join(ROOT, "adaptigraph_amd", "csrc", "ag_jpeg.hip")).read()

    def numbers(name):
        body = re.search(re.escape(name) + r"[^=;]*=\s*\{(.*?)\};", src, re.S).group(1)
        return [int(x, 0) for x in re.findall(r"-?0x[0-9a-fA-F]+|-?\d+", body)]

    assert numbers("kDct[64]") == jpeg.DCT_M.reshape(-1).tolist()
    assert numbers("kQuantBase[2][64]") == jpeg.QUANT_LUMA.tolist() + jpeg.QUANT_CHROMA.tolist()
    pos = numbers("kZigzagPos[64]")
    assert [pos[n] for n in jpeg.ZIGZAG] == list(range(64))
    for name, (bits, vals) in (("kDcLuma", jpeg.HUFF_DC[0]), ("kDcChroma", jpeg.HUFF_DC[1]), ("kAcLuma", jpeg.HUFF_AC[0]), ("kAcChroma", jpeg.HUFF_AC[1])):
        assert numbers("HuffSpec " + name) == list(bits) + list(vals), name
    header = open(os.path.join(ROOT, "include", "adaptigraph_hip.h")).read()
    assert f"#define AG_JPEG_MAX_RESTART {jpeg.MAX_RESTART}\n" in header and f"#define AG_JPEG_BLOCK_BYTES {jpeg.BLOCK_BYTES}\n" in header
    assert "#define AG_JPEG_444 0\n" in header and "#define AG_JPEG_420 1\n" in header and jpeg.SUBSAMPLING == {"444": 0, "420": 1}


# ------------------------------------------------------------------------------------------------------ AVI
def walk_avi(data):
    """Checks the structure of a file of VideoWriter -> (avih fields, strh fields, the 00dc chunks' bytes)."""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    found, chunks, index = {}, [], []

    def walk(at, end, depth):
        nonlocal movi_at
        while at < end:
            kind, size = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
            assert at % 2 == 0 and at + 8 + size <= end, (kind, at)
            if kind == b"LIST":
                name = data[at + 8:at + 12]
                if name == b"movi":
                    movi_at = at + 8
                walk(at + 12, at + 8 + size, depth + 1)
            elif kind == b"00dc":
                chunks.append((at, data[at + 8:at + 8 + size]))
            elif kind == b"idx1":
                index.extend(struct.unpack("<4sIII", data[i:i + 16]) for i in range(at + 8, at + 8 + size, 16))
                assert size % 16 == 0
            else:
                assert kind not in found
                found[kind] = data[at + 8:at + 8 + size]
            at += 8 + size + (size & 1)                                                 # chunks are padded to even length
        assert at == end

    movi_at = None
    walk(12, len(data), 0)
    assert set(found) == {b"avih", b"strh", b"strf"} and movi_at is not None
    avih, strh = struct.unpack("<14I", found[b"avih"]), struct.unpack("<4s4sIHHIIIIIIII4H", found[b"strh"])
    strf = struct.unpack("<IiiHH4sIiiII", found[b"strf"])
    assert strh[0] == b"vids" and strh[1] == b"MJPG" and strf[5] == b"MJPG" and strf[0] == 40 and strf[4] == 24
    assert avih[4] == strh[9] == len(chunks) == len(index) and avih[6] == 1 and avih[3] & 0x10
    assert (avih[8], avih[9]) == (strf[1], strf[2]) == (strh[15], strh[16])
    for (at, body), (kind, flags, offset, size) in zip(chunks, index):
        assert kind == b"00dc" and flags == 0x10 and movi_at + offset == at and size == len(body)
        assert data[at:at + 4] == b"00dc" and struct.unpack("<I", data[at + 4:at + 8])[0] == size
    assert avih[7] == strh[10] == max([len(b) for _, b in chunks], default=0)
    return avih, strh, [b for _, b in chunks]


def test_avi_structure_frames_and_edge_cases(tmp_path):
    pytest.importorskip("PIL")
    H, W = 33, 47
    frames = np.stack(list(pictures(H, W)[k][..., :3] for k in ("gradient", "drawn", "noise")))
    path = str(tmp_path / "a.avi")
    with jpeg.VideoWriter(path, H, W, 10, quality=90, subsampling="444") as out:
        out.add(frames[:2])
        out.add(frames[2])
        out.add(jpeg.encode_jpeg(frames[:1], 90, "444"))
    out.close()                                                                         # a second close changes nothing
    data = open(path, "rb").read()
    avih, strh, chunks = walk_avi(data)
    assert len(chunks) == 4 and avih[0] == 100000 and (strh[6], strh[7]) == (1, 10) and (avih[8], avih[9]) == (W, H)
    assert chunks == jpeg.encode_jpeg(frames, 90, "444") + jpeg.encode_jpeg(frames[:1], 90, "444") == jpeg.avi_frames(path)
    assert {len(c) & 1 for c in chunks} == {0, 1}                                        # odd and even lengths, both padded right (the walker)
    for chunk, image in zip(chunks, list(frames) + [frames[0]]):
        decoded, size = pil_decode(chunk)
        assert size == (W, H) and psnr(decoded, image) >= psnr(pil_decode(pil_encode(image, 90, "444", 8))[0], image) - PSNR_MARGIN_DB
    with pytest.raises(ValueError):
        out.add(frames[:1])                                                             # closed
    # no frame; one frame; half a frame per second as rate / scale
    with jpeg.VideoWriter(str(tmp_path / "empty.avi"), H, W, 1):
        pass
    avih, strh, chunks = walk_avi(open(str(tmp_path / "empty.avi"), "rb").read())
    assert chunks == [] and avih[4] == 0
    with jpeg.VideoWriter(str(tmp_path / "one.avi"), H, W, 0.5) as out:
        out.add(frames[:1])
        with pytest.raises(ValueError):
            out.add(frames[:1, :-1])                                                    # another size
    avih, strh, chunks = walk_avi(open(str(tmp_path / "one.avi"), "rb").read())
    assert len(chunks) == 1 and (strh[6], strh[7]) == (2, 1) and avih[0] == 2000000
    with pytest.raises(ValueError):
        jpeg.VideoWriter(str(tmp_path / "bad.avi"), H, W, 0)


def test_avi_refuses_to_pass_two_gigabytes_and_stays_valid(tmp_path):
    frames = noise(16, 16, 3)[None]
    path = str(tmp_path / "big.avi")
    out = jpeg.VideoWriter(path, 16, 16, 10)
    out.add(frames)
    size = len(jpeg.encode_jpeg(frames)[0])
    real = out._bytes
    out._bytes = jpeg.AVI_MAX_BYTES - (8 + size + (size & 1) + 8 + 16 * 2) + 1            # one byte short of room for the frame and its index
    with pytest.raises(ValueError, match="2\\^31"):
        out.add(frames)
    out._bytes -= 1
    assert out._bytes + 8 + size + (size & 1) + 8 + 16 * 2 == jpeg.AVI_MAX_BYTES            # exactly fits: accepted (checked without writing it)
    out._bytes = real
    out.close()
    assert len(walk_avi(open(path, "rb").read())[2]) == 1                               # the refused frame left no trace


# ------------------------------------------------------------------------------------------------------ the C ABI without a GPU
def test_ag_jpeg_encode_rejects_bad_arguments_and_sizes_its_buffers_without_a_gpu():
    L = _lib.lib()
    buf = (ctypes.c_int64 * 64)()
    big = 1 << 30
    names = ["images", "F", "H", "W", "channels", "quality", "subsampling", "restart", "scratch", "scratch_bytes", "out", "out_bytes", "offsets", "stream"]
    good = [buf, 1, 8, 8, 4, 90, 1, 8, buf, big, buf, big, buf, None]

    def call(**change):
        args = list(good)
        for k, v in change.items():
            args[names.index(k)] = v
        return L.ag_jpeg_encode(*args)

    for change, word in ((dict(images=None), b"null"), (dict(scratch=None), b"null"), (dict(out=None), b"null"), (dict(offsets=None), b"null"),
                         (dict(F=0), b"F = 0"), (dict(H=0), b"H = 0"), (dict(W=4097), b"W = 4097"), (dict(channels=2), b"channels = 2"),
                         (dict(channels=5), b"channels"), (dict(quality=0), b"quality = 0"), (dict(quality=101), b"quality"),
                         (dict(subsampling=2), b"subsampling"), (dict(subsampling=-1), b"subsampling"), (dict(restart=0), b"restart = 0"),
                         (dict(restart=17), b"restart = 17"), (dict(scratch_bytes=100), b"scratch"), (dict(out_bytes=100), b"out of 100"),
                         (dict(H=4096, W=4096, F=4096), b"exceed")):
        assert call(**change) == -1 and word in L.ag_last_error(), change
    for F, H, W, sub, restart in ((1, 8, 8, "444", 1), (3, 33, 47, "420", 3), (64, 720, 1280, "420", 8), (2, 1, 1, "420", 16), (5, 4096, 4096, "444", 16)):
        code = jpeg.SUBSAMPLING[sub]
        assert L.ag_jpeg_out_bytes(F, H, W, code, restart) == jpeg.out_bytes(F, H, W, sub, restart), (F, H, W, sub, restart)
        assert L.ag_jpeg_scratch_bytes(F, H, W, code, restart) == jpeg.scratch_bytes(F, H, W, sub, restart), (F, H, W, sub, restart)
    assert jpeg.out_bytes(1, 720, 1280, "420", 8) == 450 * (2 * 208 * 48 + 2) and jpeg.geometry(33, 47, "420", 3) == (16, 6, 3, 3, 3)
    assert L.ag_jpeg_out_bytes(0, 8, 8, 0, 1) == 0 and L.ag_jpeg_scratch_bytes(1, 8, 8, 2, 1) == 0 and L.ag_jpeg_scratch_bytes(1, 8, 8, 0, 17) == 0
    assert jpeg.frames_per_launch(720, 1280) >= 32 and jpeg.frames_per_launch(4096, 4096) >= 1


# ------------------------------------------------------------------------------------------------------ where it is used
def test_closed_loop_video_is_the_drawn_images_and_changes_nothing_else(tmp_path):
    pytest.importorskip("PIL")
    import torch
    from adaptigraph_amd.closed_loop import run_closed_loop
    lo, hi = torch.tensor([-1.0, -1.0, -3.14, 2.0]), torch.tensor([1.0, 1.0, 3.14, 4.0])
    criteria = lambda cloud: ((cloud - torch.tensor([0.0, 0.03, -0.5])) ** 2).sum(-1).mean()      # noqa: E731
    target = torch.tensor([[0.1 * i - 1.0, 0.03, -0.5] for i in range(20)])
    runs = []
    for name, video in (("plain", False), ("video", True)):
        torch.manual_seed(0)
        np.random.seed(0)
        out = tmp_path / name
        acts, errors = run_closed_loop(rope_env(None), StubPlanner(), criteria, 2, 2, lo, hi, 0.2, save_dir=str(out), viz=True, target_state=target,
                                       video=video)
        runs.append((acts, errors, [dict(np.load(str(out / f"interaction_{i}.npz"))) for i in range(2)], torch.rand(1), np.random.rand()))
    (a0, e0, r0, t0, n0), (a1, e1, r1, t1, n1) = runs
    assert torch.equal(a0, a1) and e0 == e1 and torch.equal(t0, t1) and n0 == n1
    assert all(set(x) == set(y) and all(np.array_equal(x[k], y[k]) for k in x) for x, y in zip(r0, r1))
    names = [f"rgb_vis_{i}_{j}.png" for i in range(2) for j in range(2)]
    assert sorted(p.name for p in (tmp_path / "video").iterdir() if p.suffix != ".npz") == sorted(names + ["rgb_vis.avi"])
    assert sorted(p.name for p in (tmp_path / "plain").iterdir() if p.suffix != ".npz") == names
    pngs = [viz.read_png(str(tmp_path / "video" / n)) for n in names]
    assert all(np.array_equal(p, viz.read_png(str(tmp_path / "plain" / n))) for p, n in zip(pngs, names))
    avih, strh, chunks = walk_avi(open(str(tmp_path / "video" / "rgb_vis.avi"), "rb").read())
    assert len(chunks) == 2 * 2 and (strh[6], strh[7]) == (1, 1) and (avih[8], avih[9]) == (160, 90)
    assert chunks == jpeg.encode_jpeg(np.stack(pngs))                                    # the drawn images, in step order
    for i, chunk in enumerate(chunks):                                                   # and each is nearer its own PNG than any other
        close = [psnr(pil_decode(chunk)[0], p) for p in pngs]
        assert int(np.argmax(close)) == i and close[i] >= 20.0, (i, close)
    for bad in (dict(viz=False, save_dir=str(tmp_path)), dict(viz=True, save_dir=None)):
        with pytest.raises(ValueError, match="video"):
            run_closed_loop(rope_env(None), StubPlanner(), criteria, 1, 1, lo, hi, 0.2, video=True, **bad)


def test_rollout_record_videos_and_jpg_files_on_the_host(tmp_path):
    rng = np.random.default_rng(7)
    B, T, max_nobj = 2, 3, 6
    pred, gt = (rng.normal(size=(B, T, max_nobj, 3)).astype(np.float32) * np.float32(0.3) for _ in range(2))
    eef = rng.normal(size=(B, T, 1, 3)).astype(np.float32) * np.float32(0.3)
    schedules = [[(10 * (1 - b) + t, 10 * (1 - b) + t + 1) for t in range(n)] for b, n in enumerate((3, 2))]      # rollout 1's files sort first
    particles = [[(rng.normal(size=(12, 3)) * 0.3).astype(np.float32) for _ in range(n)] for n in (3, 2)]
    args = (schedules, pred, gt, eef, None, [5, 4], max_nobj, particles, "rope", None)
    files = {}
    for name, kw in (("png", {}), ("video", dict(video=True)), ("jpg", dict(fmt="jpg", video=True))):
        d = str(tmp_path / name)
        os.makedirs(d)
        written = viz.write_rollout_record([d, d], *args, H=45, W=80, batch=4, **kw)      # both rollouts into one directory
        assert sorted(written) == sorted(os.path.join(d, f) for f in os.listdir(d))
        files[name] = sorted(os.listdir(d))
    stems = [f"{s:06}_{e:06}" for sched in schedules for s, e in sched]
    videos = ["both.avi", "gt.avi", "pred.avi"]
    assert files["png"] == sorted(f"{s}_{n}.png" for s in stems for n in ("pred", "gt", "both"))
    assert files["video"] == sorted(files["png"] + videos) and files["jpg"] == sorted([f.replace(".png", ".jpg") for f in files["png"]] + videos)
    for f in files["png"]:
        assert np.array_equal(viz.read_png(str(tmp_path / "png" / f)), viz.read_png(str(tmp_path / "video" / f)))
    for name in ("pred", "gt", "both"):
        avih, strh, chunks = walk_avi(open(str(tmp_path / "jpg" / f"{name}.avi"), "rb").read())
        assert (strh[6], strh[7]) == (1, 10) and (avih[8], avih[9]) == ((160, 45) if name == "both" else (80, 45))
        want = [open(str(tmp_path / "jpg" / f"{s}_{name}.jpg"), "rb").read() for s in sorted(stems)]      # file-name order
        assert chunks == want == jpeg.avi_frames(str(tmp_path / "video" / f"{name}.avi")) and len(chunks) == 5
        assert chunks == jpeg.encode_jpeg(np.stack([viz.read_png(str(tmp_path / "png" / f"{s}_{name}.png")) for s in sorted(stems)]))
    with pytest.raises(ValueError):
        viz.write_rollout_record([str(tmp_path)] * 2, *args, H=45, W=80, fmt="gif")


def test_rollout_options_read_the_format_and_the_video_switch():
    import adaptigraph_amd.eval_rollout as er
    plain = er._viz_options(None, ["a"])
    assert plain == {"dirs": ["a"], "size": (720, 1280), "radius": None, "format": "png", "video": False}      # the defaults: today's files
    cfg = {"rollout_config": {"viz_video": True, "viz_format": "jpg", "viz_size": (90, 160)}}
    assert er._viz_options(cfg, ["a", "b"]) == {"dirs": ["a", "b"], "size": (90, 160), "radius": None, "format": "jpg", "video": True}
    assert er._viz_options({"viz_video": True}, ["a"])["video"] is True                  # a driver's `viz` dict: the same keys
    assert er._viz_options({}, ["a"]) == plain
    with pytest.raises(ValueError):
        er._viz_options({"rollout_config": {"viz_format": "gif"}}, ["a"])
