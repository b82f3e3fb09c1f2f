"""Baseline JPEG in float64 NumPy, written from ITU-T T.81 and the JFIF specification: what tests/test_jpeg_cpu.py and
tests/test_jpeg_gpu.py compare rag-gesture_amd/video.py and csrc/rg_jpeg.hip against.  Nothing here imports the package.

    quant_tables(quality)          Annex K.1 / K.2 scaled the libjpeg way, [64] each in zig-zag order
    unquantised(rgb)               float64 DCT coefficients [MCU][6][64] (zig-zag) of a uint8 [H, W, 3] picture: JFIF BT.601 full
                                   range, level shift, edge replication to multiples of 16, 2 x 2 chroma mean, orthonormal DCT-II
    coefficients(rgb, quality)     (int16 coefficients, near: bool of the same shape, True where |v| / q lies within DELTA of k + 0.5)
    entropy_intervals(coef, rows, cols)   per restart interval (= MCU row) its stuffed bytes with the RSTm behind it
    header(h, w, quality, cols) / jfif_file(...)    SOI APP0 DQT DQT SOF0 DHT x 4 DRI SOS ... EOI
    walk_avi(data)                 a minimal RIFF walker for the AVI files of video.AVIWriter
    images() / batch_images()      the pictures the tests use
"""
import struct

import numpy as np

DELTA = 2e-3          # quantisation steps: see the docstring of tests/test_jpeg_gpu.py for the fp32 bound it stands for
EXCLUDED_CAP = 0.01

LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                 95, 98, 112, 100, 103, 99], np.int64)
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                   99, 99, 99] + [99] * 32, np.int64)

DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5,
    0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9,
    0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2,
    0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17,
    0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
    0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7,
    0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2,
    0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]


def zigzag():
    """[64]: zig-zag position -> row-major index of the 8 x 8 block (T.81 figure 5), by walking the anti-diagonals."""
    order = []
    for s in range(15):
        cells = [(r, s - r) for r in range(8) if 0 <= s - r < 8]
        order += cells if s % 2 else cells[::-1]          # even diagonals run upwards (row falling)
    return np.array([r * 8 + c for r, c in order], np.int64)


ZZ = zigzag()


def quant_tables(quality):
    """-> (luma, chroma) int64 [64] in zig-zag order."""
    q = int(quality)
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255)[ZZ] for base in (LUMA, CHROMA))


def dct_matrix():
    k, n = np.arange(8)[:, None], np.arange(8)[None, :]
    c = np.sqrt(2.0 / 8.0) * np.cos((2 * n + 1) * k * np.pi / 16.0)
    c[0] = np.sqrt(1.0 / 8.0)
    return c


def unquantised(rgb):
    """uint8 [H, W, 3] -> (float64 [rows * cols, 6, 64] in zig-zag order, rows, cols)."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    h, w, _ = rgb.shape
    rows, cols = -(-h // 16), -(-w // 16)
    p = np.pad(rgb, ((0, rows * 16 - h), (0, cols * 16 - w), (0, 0)), mode="edge").astype(np.float64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b - 128.0
    cb = -0.168736 * r - 0.331264 * g + 0.5 * b
    cr = 0.5 * r - 0.418688 * g - 0.081312 * b
    half = lambda a: a.reshape(rows * 8, 2, cols * 8, 2).mean(axis=(1, 3))
    cb, cr = half(cb), half(cr)
    c = dct_matrix()
    out = np.zeros((rows, cols, 6, 64))
    for mr in range(rows):
        for mc in range(cols):
            ym = y[mr * 16:mr * 16 + 16, mc * 16:mc * 16 + 16]
            blocks = [ym[:8, :8], ym[:8, 8:], ym[8:, :8], ym[8:, 8:], cb[mr * 8:mr * 8 + 8, mc * 8:mc * 8 + 8],
                      cr[mr * 8:mr * 8 + 8, mc * 8:mc * 8 + 8]]
            for i, blk in enumerate(blocks):
                out[mr, mc, i] = (c @ blk @ c.T).reshape(64)[ZZ]
    return out.reshape(rows * cols, 6, 64), rows, cols


def coefficients(rgb, quality, delta=DELTA):
    """-> (int16 [MCU, 6, 64], near bool [MCU, 6, 64], rows, cols): sign(v) floor(|v| / q + 0.5), and where |v| / q is within
    delta of a rounding boundary k + 0.5 (there, and only there, an fp32 encoder may land on the other side)."""
    v, rows, cols = unquantised(rgb)
    ql, qc = quant_tables(quality)
    q = np.stack([ql] * 4 + [qc] * 2).astype(np.float64)[None]
    t = np.abs(v) / q
    k = np.floor(t + 0.5)
    near = np.abs(t - np.floor(t) - 0.5) <= delta
    return (np.sign(v) * k).astype(np.int16), near, rows, cols


# ------------------------------------------------------------------------------------------------------------ entropy coding
def huffman_codes(bits, vals):
    """Annex C: symbol -> (code, length)."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return table


DC_CODES = (huffman_codes(DC_LUMA_BITS, DC_VALS), huffman_codes(DC_CHROMA_BITS, DC_VALS))
AC_CODES = (huffman_codes(AC_LUMA_BITS, AC_LUMA_VALS), huffman_codes(AC_CHROMA_BITS, AC_CHROMA_VALS))


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, length):
        self.acc, self.n = (self.acc << length) | value, self.n + length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def _magnitude(v):
    """(category, the category's extra bits) of T.81 F.1.2.1 / F.1.2.2."""
    v = int(v)
    size = abs(v).bit_length()
    return size, (v if v >= 0 else v - 1) & ((1 << size) - 1)


def encode_block(bits, block, pred, comp):
    dc, ac = DC_CODES[comp], AC_CODES[comp]
    size, extra = _magnitude(int(block[0]) - pred)
    assert size <= 11
    bits.put(*dc[size])
    bits.put(extra, size)
    run = 0
    for k in range(1, 64):
        v = int(block[k])
        if v == 0:
            run += 1
            continue
        while run >= 16:
            bits.put(*ac[0xF0])
            run -= 16
        size, extra = _magnitude(v)
        assert size <= 10
        bits.put(*ac[(run << 4) | size])
        bits.put(extra, size)
        run = 0
    if run:
        bits.put(*ac[0x00])


def entropy_intervals(coef, rows, cols):
    """coef int [rows * cols, 6, 64] -> per MCU row its bytes: the stuffed codes, the last byte padded with 1 bits, and RSTm
    (m = row % 8) behind every row but the last."""
    coef = np.asarray(coef).reshape(rows, cols, 6, 64)
    out = []
    for r in range(rows):
        bits, pred = _Bits(), [0, 0, 0]
        for c in range(cols):
            for i in range(6):
                comp = 0 if i < 4 else i - 3
                encode_block(bits, coef[r, c, i], pred[comp], 0 if comp == 0 else 1)
                pred[comp] = int(coef[r, c, i, 0])
        data = bits.flush()
        if r + 1 < rows:
            data += bytes([0xFF, 0xD0 + r % 8])
        out.append(data)
    return out


def _segment(marker, body):
    return struct.pack(">BBH", 0xFF, marker, len(body) + 2) + body


def header(h, w, quality, cols):
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    out += _segment(0xDB, bytes([0]) + bytes(ql.tolist())) + _segment(0xDB, bytes([1]) + bytes(qc.tolist()))
    out += _segment(0xC0, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS), (0x01, DC_CHROMA_BITS, DC_VALS),
                              (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        out += _segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, struct.pack(">H", cols))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def jfif_from_coefficients(coef, h, w, quality):
    rows, cols = -(-h // 16), -(-w // 16)
    return header(h, w, quality, cols) + b"".join(entropy_intervals(coef, rows, cols)) + b"\xff\xd9"


def jfif_file(rgb, quality):
    coef, _, _, _ = coefficients(rgb, quality)
    return jfif_from_coefficients(coef, rgb.shape[0], rgb.shape[1], quality)


# ------------------------------------------------------------------------------------------------------------ pictures
def images():
    """name -> uint8 [H, W, 3]: noise with padding in both dimensions and two intervals; odd noise; a gradient of 17 MCUs per
    interval (102 blocks: more than a wave's lanes) and 10 intervals (the restart counter wraps); one black MCU."""
    rng = np.random.default_rng(20240607)
    y, x = np.mgrid[0:150, 0:272]
    grad = np.stack([x * 255 // 271, y * 255 // 149, (x + y) * 255 // 420], axis=-1).astype(np.uint8)
    return {"noise_40x24": rng.integers(0, 256, (24, 40, 3), dtype=np.uint8),
            "noise_17x23": rng.integers(0, 256, (23, 17, 3), dtype=np.uint8),
            "gradient_272x150": grad,
            "black_16x16": np.zeros((16, 16, 3), np.uint8)}


def batch_images():
    """Three frames of one size (40 x 56) with different content: noise, a gradient, flat grey with a bright square."""
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:40, 0:56]
    grad = np.stack([x * 4, y * 6, 255 - x * 4], axis=-1).astype(np.uint8)
    flat = np.full((40, 56, 3), 191, np.uint8)
    flat[10:30, 20:41] = (250, 240, 10)
    return np.stack([rng.integers(0, 256, (40, 56, 3), dtype=np.uint8), grad, flat])


def psnr(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    m = float((d * d).mean())
    return float("inf") if m == 0 else 10.0 * np.log10(255.0 ** 2 / m)


# ------------------------------------------------------------------------------------------------------------ RIFF
def riff_chunks(data, pos, end):
    """The chunks of data[pos:end] -> [(fourcc, payload offset, size, list type or None)], each padded to an even length."""
    out = []
    while pos < end:
        assert pos + 8 <= end, "a chunk header crosses the end of its list"
        cc, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        assert pos + 8 + size <= end, "chunk %r of %d bytes crosses the end of its list" % (cc, size)
        out.append((cc, pos + 8, size, data[pos + 8:pos + 12] if cc in (b"RIFF", b"LIST") else None))
        pos += 8 + size + (size & 1)
    assert pos == end or pos == end + 1, "the chunks do not fill their list"
    return out


def walk_avi(data):
    """An AVI file's bytes -> dict(avih=, streams=[(strh fields, strf bytes)], video=[payloads], audio=[payloads], index=[(id,
    flags, offset, size)], movi=offset of the 'movi' fourcc).  Asserts that every size is consistent, every chunk is padded to
    an even length and every idx1 entry points at its chunk."""
    top = riff_chunks(data, 0, len(data))
    assert len(top) == 1 and top[0][0] == b"RIFF" and top[0][3] == b"AVI " and 8 + top[0][2] == len(data)
    lists = riff_chunks(data, 12, len(data))
    assert [(c, t) for c, _, _, t in lists] == [(b"LIST", b"hdrl"), (b"LIST", b"movi"), (b"idx1", None)]
    (_, hoff, hsize, _), (_, moff, msize, _), (_, ioff, isize, _) = lists
    hdr = riff_chunks(data, hoff + 4, hoff + hsize)
    assert hdr[0][0] == b"avih" and hdr[0][2] == 56
    names = ("us_per_frame", "max_bytes_per_sec", "padding", "flags", "total_frames", "initial_frames", "streams",
             "suggested_buffer", "width", "height")
    avih = dict(zip(names, struct.unpack("<10I", data[hdr[0][1]:hdr[0][1] + 40])))
    streams = []
    for cc, off, size, typ in hdr[1:]:
        assert cc == b"LIST" and typ == b"strl"
        sub = riff_chunks(data, off + 4, off + size)
        assert [c for c, _, _, _ in sub] == [b"strh", b"strf"] and sub[0][2] == 56
        f = struct.unpack("<4s4sIHHIIIIIIII4H", data[sub[0][1]:sub[0][1] + 56])
        strh = dict(type=f[0], handler=f[1], flags=f[2], scale=f[6], rate=f[7], start=f[8], length=f[9], suggested_buffer=f[10],
                    quality=f[11], sample_size=f[12], frame=f[13:17])
        streams.append((strh, data[sub[1][1]:sub[1][1] + sub[1][2]]))
    assert avih["streams"] == len(streams)
    movi = moff                                               # the 'movi' fourcc sits at the list's payload offset
    video, audio, found = [], [], []
    for cc, off, size, _ in riff_chunks(data, moff + 4, moff + msize):
        assert cc in (b"00dc", b"01wb")
        (video if cc == b"00dc" else audio).append(data[off:off + size])
        found.append((cc, off - 8 - movi, size))
    assert isize % 16 == 0
    index = [struct.unpack("<4sIII", data[ioff + 16 * i:ioff + 16 * i + 16]) for i in range(isize // 16)]
    assert [(c, o, s) for c, _, o, s in index] == found, "idx1 does not list the chunks of movi"
    for cc, _, o, s in index:
        assert data[movi + o:movi + o + 4] == cc and struct.unpack("<I", data[movi + o + 4:movi + o + 8])[0] == s
    return dict(avih=avih, streams=streams, video=video, audio=audio, index=index, movi=movi)
