"""The engine's host-side weight packing (csrc/ag_pack.hip), bit for bit, without a GPU: the number formats against torch's CPU casts, and the
packed image decoded from the documented layouts (csrc/ag_common.h; the comments above pack_first_layer and pack_layer_h3).  The packers are
compiled with tests/host/pack_probe.cpp into a stand-alone program under the host's address and undefined-behaviour sanitizers and run as a
child process; a sanitizer report fails the test."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adaptigraph_amd", "csrc")
F, ATTR, NHIS, ACT = 150, 2, 4, 3
FP, NT, CHUNK = 160, 5, 5120                   # padded width, 32-wide tiles, floats per chunk image (20 480 bytes)
DE = 2 * ATTR + 1 + 3 * NHIS                   # relation-encoder fan-in, 17
LO_FEAT0 = 2 * ATTR + 1                        # first input column whose fp16 residual the fp16 first layer also multiplies


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"      # (the Makefile's compiler)
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc: the packers use _Float16, which needs the ROCm compiler")
    exe = str(tmp_path_factory.mktemp("pack_probe") / "pack_probe")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "--offload-arch=gfx950"] + san +
                          [os.path.join(ROOT, "tests", "host", "pack_probe.cpp"), os.path.join(CSRC, "ag_pack.hip"), "-o", exe])

    def run(mode, payload, workdir):
        src, dst = os.path.join(workdir, mode + ".in"), os.path.join(workdir, mode + ".out")
        with open(src, "wb") as f:
            f.write(payload)
        # (leak checking needs ptrace rights some containers withhold; the probe frees everything through std::vector)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe, mode, src, dst], env=env, capture_output=True, text=True)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-4000:])
        with open(dst, "rb") as f:
            return f.read()
    return run


# ---------------------------------------------------------------- (a) number formats

def e4m3_expected(v):
    """torch's e4m3fn cast; from 464 (the midpoint between the largest finite value 448 and the absent 480) torch gives NaN, the engine saturates."""
    bits = v.to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()
    sat = (v.abs() >= 464).numpy()
    bits[sat] = 0x7e | (np.signbit(v.numpy()[sat]).astype(np.uint8) << 7)
    return bits


def f16_pair_expected(v):
    hi = v.to(torch.float16)
    lo = (v - hi.float()).to(torch.float16)
    return hi.view(torch.int16).numpy().view(np.uint16), lo.view(torch.int16).numpy().view(np.uint16)


def bf16_expected(v):
    return v.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def format_inputs():
    g = torch.Generator().manual_seed(0)
    normals = torch.randn(400_000, generator=g) * torch.exp2(torch.rand(400_000, generator=g) * 22 - 14)
    codes = torch.tensor([b for b in range(256) if b & 0x7f != 0x7f], dtype=torch.uint8)
    finite = codes.view(torch.float8_e4m3fn).float()                          # every finite e4m3 value
    mags = finite[finite >= 0].sort().values.unique()
    mid = torch.cat([(mags[:-1] + mags[1:]) / 2, torch.tensor([464.0])])      # (exact in fp32) + where the cast leaves the finite range
    mids = torch.cat([mid, torch.nextafter(mid, torch.tensor(float("inf"))), torch.nextafter(mid, torch.tensor(0.0))])
    special = torch.tensor([0.0, -0.0, 447.9, 448, 463.9, 2.0 ** -10, 2.0 ** -9, 65504, 65519.9, 1e-8, 500, -1e6])
    return torch.cat([normals, finite, mids, -mids, special]).contiguous()


def test_number_formats_match_torch_cpu_casts_bit_for_bit(probe, tmp_path):
    v = format_inputs()
    assert v.dtype == torch.float32 and len(v) >= 400_771 and bool(torch.isfinite(v).all())
    out = np.frombuffer(probe("formats", v.numpy().tobytes(), str(tmp_path)), np.uint8).reshape(len(v), 8)
    words = out[:, :6].copy().view(np.uint16)
    hi, lo = f16_pair_expected(v)
    assert np.array_equal(words[:, 0], bf16_expected(v))
    assert np.array_equal(words[:, 1], hi) and np.array_equal(words[:, 2], lo)
    assert np.array_equal(out[:, 6], e4m3_expected(v))
    big = (v.abs() >= 464).numpy()
    assert big.sum() >= 3 and set(out[big, 6] & 0x7f) == {0x7e}               # saturated, never the NaN pattern 0x7f
    assert not out[:, 7].any()


# ---------------------------------------------------------------- (b) layouts

def random_weights(phys_dim, seed):
    """The 22 tensors in state_dict order: normals over five octaves of scale, so that block maxima, hi / lo parts and rounding cases differ
    from element to element; a few blocks that are exactly zero or exactly fp16 (lo part zero: the all-zero-block scale)."""
    rng = np.random.default_rng(seed)
    dn = ATTR + phys_dim + ACT
    shapes = [(F, dn), (F, F), (F, F), (F, DE), (F, F), (F, F)]
    t = []
    for shape in shapes:
        t += [shape, (shape[0],)]
    t += [(F, 2 * F), (F,), (F, 3 * F), (F,), (F, F), (F,), (F, F), (F,), (3, F), (3,)]
    out = [(rng.standard_normal(s) * np.exp2(rng.uniform(-6, -1, s))).astype(np.float32) for s in t]
    out[8][3, 32:64] = 0.0                                             # W_RE1: a block with hi and lo both zero
    out[8][5, 64:96] = out[8][5, 64:96].astype(np.float16)            # ... and one whose lo part is zero
    out[10][7, :] = 0.0                                                # W_RE2: a zero row (its bias stays)
    return out


def pack(probe, tmp_path, phys_dim, tensors):
    cfg = struct.pack("<6if", F, NHIS, ATTR, phys_dim, ACT, 3, 100.0)
    raw = probe("image", cfg + b"".join(np.ascontiguousarray(x, np.float32).tobytes() for x in tensors), str(tmp_path))
    head = np.frombuffer(raw[:96], np.uint64)
    image = np.frombuffer(raw[96:], np.float32)
    assert len(image) == head[11]
    return {"off": head[:8].reshape(2, 4).astype(int), "off_h2": int(head[8]), "off_sc": int(head[9]), "h2_ok": bool(head[10]), "image": image}


def wide(W, bias, col0=0, K=F, n_tiles=NT):
    """One layer as [tiles][32 out rows][160 image columns]: columns [0, K) = W[:, col0 : col0 + K], column K = the bias, the rest zero."""
    m = np.zeros((n_tiles * 32, FP), np.float32)
    m[:W.shape[0], :K] = W[:, col0:col0 + K]
    if bias is not None:
        m[:W.shape[0], K] = bias
    return m.reshape(n_tiles, 32, FP)


def first(W, bias, residual_from=None):
    """A narrow first layer as [5 tiles][32 out rows][32 image columns]: the weights, the bias in column K, and (fp16 edge stack) behind it the
    weights of input columns residual_from .. K - 1 once more."""
    K = W.shape[1]
    m = np.zeros((NT * 32, 32), np.float32)
    m[:F, :K] = W
    m[:F, K] = bias
    if residual_from is not None:
        m[:F, K + 1:K + 1 + K - residual_from] = W[:, residual_from:]
    return m.reshape(NT, 32, 32)


def f32_image(m):
    """[..., 32 rows i, columns] -> the fp32 image: element (i, k) at 4 * ((k / 4) ^ ((i >> 1) & 7)) + k % 4 of its row (16-byte XOR swizzle)."""
    i = np.arange(32)[:, None, None]
    c = np.arange(m.shape[-1] // 4)[None, :, None]
    k = 4 * (c ^ ((i >> 1) & 7)) + np.arange(4)[None, None, :]           # the column stored at (i, 16-byte column c, p)
    return np.take_along_axis(m, np.broadcast_to(k.reshape(32, -1), m.shape[:-2] + (32, m.shape[-1])), axis=-1)


def fragments(m):
    """[..., 32 rows i, 16 * NU columns] -> [..., NU steps u, 64 lanes (h, i), 8 slots e]: slot e = column 16u + 8(e >> 2) + 4h + (e & 3)."""
    u, h, e = np.meshgrid(np.arange(m.shape[-1] // 16), np.arange(2), np.arange(8), indexing="ij")
    k = 16 * u + 8 * (e >> 2) + 4 * h + (e & 3)                              # [u][h][e]
    g = m[..., :, k]                                                         # [..., i, u, h, e]
    return np.moveaxis(g, -4, -2).reshape(m.shape[:-2] + (m.shape[-1] // 16, 64, 8))


def split_image(m, fp16):
    """The split fragment image of one tile set: [..., NU steps][hi | lo][64 lanes][8 slots] of 16-bit words."""
    v = torch.from_numpy(np.ascontiguousarray(m))
    if fp16:
        hi, lo = f16_pair_expected(v)
    else:
        hi = bf16_expected(v)
        lo = bf16_expected(v - v.to(torch.bfloat16).float())
    return np.stack([fragments(hi), fragments(lo)], axis=-3)


def chunks(words16, n_chunks):
    """16-bit words of whole tiles -> float chunk images, each zero-padded to 20 480 bytes."""
    per = words16.reshape(n_chunks, -1)
    out = np.zeros((n_chunks, CHUNK * 2), np.uint16)
    out[:, :per.shape[1]] = per
    return out.view(np.float32).reshape(-1)


def expected_stream(layers, mode):
    """mode 0: fp32 images, 1: split-bf16 fragment images.  layers: ("first", W, b) | ("wide", W, b, col0, n_tiles)"""
    parts = []
    for kind, W, b, *rest in layers:
        if kind == "first":
            m = first(W, b)
            steps = (W.shape[1] + 1 + 15) // 16                             # k16-steps that hold the K + 1 columns
            parts.append(f32_image(m).reshape(-1) if mode == 0 else chunks(split_image(m[..., :16 * steps], False), 1))
        else:
            m = wide(W, b, rest[0], F, rest[1])
            parts.append(f32_image(m).reshape(-1) if mode == 0 else chunks(split_image(m, False), rest[1]))
    return np.concatenate(parts)


def e8m0_expected(block_max):
    """floor(log2(max)) - 7 + 127 clamped to [1, 254]; 127 for an all-zero block"""
    _, e = np.frexp(block_max)                                               # max = f * 2^e, f in [0.5, 1): floor(log2 max) = e - 1
    return np.where(block_max > 0, np.clip(e - 1 - 7 + 127, 1, 254), 127).astype(np.uint8)


def h3_expected(W, b, col0=0):
    """One wide layer of the fp16 edge stack: its 5 chunk images (bytes) and its 5 x 128 scale dwords (bytes)."""
    m = torch.from_numpy(wide(W, b, col0))                                   # [5 tiles][32 i][160]
    hi16, _ = f16_pair_expected(m)
    hi = m.to(torch.float16).float()
    parts = {0: (m - hi).numpy(), 1: hi.numpy()}                             # group 0 of a lane's 32 bytes: W_lo, group 1: W_hi
    expo = {g: e8m0_expected(np.abs(p).reshape(NT, 32, NT, 32).max(-1)) for g, p in parts.items()}      # [tile][i][input tile t]
    img = np.zeros((NT, 20480), np.uint8)
    img[:, :10240] = fragments(hi16).reshape(NT, -1).view(np.uint8)
    t, h, q, p = np.meshgrid(np.arange(NT), np.arange(2), np.arange(4), np.arange(4), indexing="ij")
    k = 32 * t + 8 * q + 4 * h + p                                           # [t][h][q][p]: the column at byte 4q + p of lane (i, h), input tile t
    mx = np.zeros((NT, NT, 2, 32, 2, 16), np.uint8)                          # [tile][t][h][i][group][4q + p]
    for g, part in parts.items():
        scaled = np.ldexp(part[:, :, k], 127 - expo[g].astype(np.int32)[:, :, :, None, None, None])        # [tile][i][t][h][q][p]
        code = e4m3_expected(torch.from_numpy(np.ascontiguousarray(scaled.astype(np.float32))))
        mx[:, :, :, :, g, :] = np.transpose(code, (0, 2, 3, 1, 4, 5)).reshape(NT, NT, 2, 32, 16)
    img[:, 10240:] = mx.reshape(NT, -1)
    sc = np.full((NT, 2, 2, 32, 4), 0x7f, np.uint8)                          # [tile][dword][h][i][byte]; lanes of half h hold group h's exponents
    for g in (0, 1):
        sc[:, 0, g, :, :] = expo[g][:, :, :4]
        sc[:, 1, g, :, 0] = expo[g][:, :, 4]
    return img.reshape(-1), sc.reshape(-1)


@pytest.mark.parametrize("phys_dim", [0, 1, 2])
def test_packed_image_is_the_documented_layout_exactly(probe, tmp_path, phys_dim):
    t = random_weights(phys_dim, seed=phys_dim)
    (pe0, bpe0, pe1, bpe1, pe2, bpe2, re0, bre0, re1, bre1, re2, bre2, pp, bpp, rp, brp, d0, bd0, d1, bd1, d2, bd2) = t
    assert pe0.shape[1] == 5 + phys_dim
    got = pack(probe, tmp_path, phys_dim, t)
    image = got["image"]
    streams = [
        [("first", pe0, bpe0), ("wide", pe1, bpe1, 0, NT), ("wide", pe2, bpe2, 0, NT), ("wide", pp, bpp, 0, NT), ("wide", rp, None, F, NT),
         ("wide", rp, None, 2 * F, NT)],                                                                      # node_encode: 26 chunks
        [("first", re0, bre0), ("wide", re1, bre1, 0, NT), ("wide", re2, bre2, 0, NT), ("wide", rp, brp, 0, NT)],      # edge_encode: 16
        [("wide", pp, None, F, NT), ("wide", rp, None, F, NT), ("wide", rp, None, 2 * F, NT)],               # node_mid: 15
        [("wide", pp, None, F, NT), ("wide", d0, bd0, 0, NT), ("wide", d1, bd1, 0, NT), ("wide", d2, bd2, 0, 1)],      # node_last: 16
    ]
    want, at = [], 0
    for mode in (0, 1):
        for k, layers in enumerate(streams):
            assert got["off"][mode][k] == at
            want.append(expected_stream(layers, mode))
            at += len(want[-1])
    assert at == 2 * 73 * CHUNK == got["off_h2"]
    # the fp16 edge stack: the first layer as a split-fp16 image with the residual columns, then 15 units of [fp16 hi | block-scaled e4m3]
    m0 = first(re0, bre0, LO_FEAT0)
    assert np.array_equal(m0.reshape(NT * 32, 32)[:F, DE + 1:DE + 13], re0[:, 5:17]) and not m0[..., 30:].any()      # (the expectation: inputs 5..16 again)
    want.append(chunks(split_image(m0, True), 1))
    scales = []
    for W, b in ((re1, bre1), (re2, bre2), (rp, brp)):
        img, sc = h3_expected(W, b)
        want.append(img.view(np.float32))
        scales.append(sc.view(np.float32))
    assert got["off_sc"] == got["off_h2"] + 16 * CHUNK and len(image) == got["off_sc"] + 15 * 128
    want = np.concatenate(want + scales)
    # every byte: the values where the layout puts them, zero (0x7f in a scale dword) wherever it puts nothing
    assert len(want) == len(image)
    bad = np.flatnonzero(want.view(np.uint8) != image.view(np.uint8))
    assert bad.size == 0, f"{bad.size} bytes differ, first at byte {bad[0]} (chunk {bad[0] // 20480}, byte {bad[0] % 20480} of it)"
    assert got["h2_ok"]


def test_fp16_edge_stack_is_refused_for_a_weight_beyond_fp16(probe, tmp_path):
    t = random_weights(1, seed=7)
    assert pack(probe, tmp_path, 1, t)["h2_ok"]
    t[8][11, 13] = 7e4                                                        # one relation-encoder weight past 65504
    assert not pack(probe, tmp_path, 1, t)["h2_ok"]
