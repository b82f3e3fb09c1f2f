"""CPU: the host side of the Motion-JPEG path -- the float64 JPEG restatement the GPU tests compare against
(tests/golden/jpeg_fixture.py) read by an independent decoder (Pillow), video.AVIWriter walked chunk by chunk, the file header
video.JPEGEncoder puts in front of a scan, the C ABI of csrc/rg_jpeg.hip and the command line's new options."""
import ctypes
import importlib
import importlib.util
import io
import os
import re
import subprocess
import wave

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRY = {"rg_jpeg_dct_quant": 10, "rg_jpeg_entropy_count": 7, "rg_jpeg_entropy_write": 9}     # arguments, handle and stream included


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


jf = _load("jpeg_fixture")
QUALITIES = (50, 90, 100)


def _decode(data):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


# ------------------------------------------------------------------------------------------------------------ the fixture
def test_fixture_tables_are_the_standard_ones():
    assert jf.ZZ[:10].tolist() == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and sorted(jf.ZZ.tolist()) == list(range(64))
    assert jf.ZZ[-3:].tolist() == [55, 62, 63]
    ql, qc = jf.quant_tables(50)
    assert np.array_equal(ql, jf.LUMA[jf.ZZ]) and np.array_equal(qc, jf.CHROMA[jf.ZZ])          # quality 50 is Annex K itself
    assert (jf.quant_tables(100)[0] == 1).all() and jf.quant_tables(1)[0].max() == 255
    assert jf.quant_tables(90)[0][:4].tolist() == [3, 2, 2, 3] and jf.quant_tables(25)[0][0] == 32
    for codes, n in ((jf.DC_CODES[0], 12), (jf.DC_CODES[1], 12), (jf.AC_CODES[0], 162), (jf.AC_CODES[1], 162)):
        assert len(codes) == n
        words = sorted(format(c, "0%db" % l) for c, l in codes.values())
        assert not any(b.startswith(a) for a, b in zip(words, words[1:]))                         # a prefix code
    assert jf.DC_CODES[0][0] == (0b00, 2) and jf.AC_CODES[0][0x00] == (0b1010, 4) and jf.AC_CODES[0][0xF0] == (0b11111111001, 11)
    assert jf.AC_CODES[1][0x00] == (0b00, 2) and jf.AC_CODES[1][0xF0] == (0b1111111010, 10)
    c = jf.dct_matrix()
    assert np.allclose(c @ c.T, np.eye(8), atol=1e-14)


def test_fixture_files_decode_with_an_independent_decoder():
    Image = pytest.importorskip("PIL.Image")
    for name, img in jf.images().items():
        for q in QUALITIES:
            data = jf.jfif_file(img, q)
            im = _decode(data)
            assert im.size == (img.shape[1], img.shape[0]) and im.mode == "RGB", (name, q)
            dec = np.asarray(im)
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, "JPEG", quality=q, subsampling=2)
            own = np.asarray(Image.open(buf).convert("RGB"))
            print("%s q%d: %d bytes, PSNR %.2f dB (Pillow's own encoder %.2f dB)" % (name, q, len(data), jf.psnr(dec, img), jf.psnr(own, img)))
            if name.startswith("black"):
                assert not dec.any()
            else:                                   # as good as the decoder's own encoder at this quality (4:2:0, same tables)
                assert jf.psnr(dec, img) >= jf.psnr(own, img) - 0.5, (name, q)
    # 10 intervals: RST0 .. RST7, RST0 in this order, and none in the single-MCU picture
    data = jf.jfif_file(jf.images()["gradient_272x150"], 90)
    scan = data[data.index(b"\xff\xda"):]
    assert re.findall(rb"\xff([\xd0-\xd7])", scan) == [bytes([0xD0 + r % 8]) for r in range(9)]
    assert not re.search(rb"\xff[\xd0-\xd7]", jf.jfif_file(jf.images()["black_16x16"], 90))


def test_fixture_excludes_under_one_percent_of_its_own_coefficients():
    worst = 0.0
    pictures = dict(jf.images(), **{"batch_%d" % i: f for i, f in enumerate(jf.batch_images())})
    for name, img in pictures.items():
        for q in QUALITIES:
            coef, near, rows, cols = jf.coefficients(img, q)
            assert coef.shape == near.shape == (rows * cols, 6, 64) and coef.dtype == np.int16
            share = float(near.mean())
            worst = max(worst, share)
            assert share <= jf.EXCLUDED_CAP, (name, q, share)
            assert np.abs(coef[:, :, 1:]).max() <= 1023 and np.abs(coef[:, :, 0]).max() <= 1024
    print("largest excluded share at delta = %g: %.4f %%" % (jf.DELTA, 100 * worst))
    assert jf.DELTA <= 2e-3
    # the tie the cap is there for: a constant 255 picture at quality 50 has DC 1016 / 16 = 63.5 exactly
    _, near, _, _ = jf.coefficients(np.full((16, 16, 3), 255, np.uint8), 50)
    assert near[0, :4, 0].all()


def test_entropy_coder_on_hand_made_blocks():
    """The fixture's coder against codes written out by hand from Annex K.3."""
    z = np.zeros((1, 6, 64), np.int16)
    # all zero: every block is DC category 0 + EOB: luma 00 1010 x 4, chroma 00 00 x 2 -> 32 bits, no padding
    assert jf.entropy_intervals(z, 1, 1) == [bytes([0b00101000, 0b10100010, 0b10001010, 0b00000000])]
    one = z.copy()
    one[0, 0, 0] = -3                                   # DC difference -3: category 2 (code 011), bits 00; then Y01 sees +3: 011 11
    bits = "011" + "00" + "1010" + "011" + "11" + "1010" + "00" + "1010" + "00" + "1010" + "0000" + "0000"
    bits += "1" * (-len(bits) % 8)
    assert jf.entropy_intervals(one, 1, 1) == [int(bits, 2).to_bytes(len(bits) // 8, "big")]
    run = z.copy()
    run[0, 0, 17] = 1                                   # 16 zeros in front: ZRL, then run 0 size 1 (code 00) bit 1, EOB
    bits = "00" + "11111111001" + "00" + "1" + "1010" + ("00" + "1010") * 3 + "0000" + "0000"
    bits += "1" * (-len(bits) % 8)
    assert jf.entropy_intervals(run, 1, 1) == [int(bits, 2).to_bytes(len(bits) // 8, "big")]
    two = np.zeros((2, 6, 64), np.int16)                # two rows: RST0 between them, none at the end
    got = jf.entropy_intervals(two, 2, 1)
    assert got[0][-2:] == b"\xff\xd0" and got[1] == got[0][:-2]


# ------------------------------------------------------------------------------------------------------------ the file header
def test_encoder_header_is_the_fixtures(rg):
    v = rg.video
    assert v.ZIGZAG == tuple(jf.ZZ.tolist())
    for q in (1, 25, 50, 90, 100):
        for a, b in zip(v.quant_tables(q), jf.quant_tables(q)):
            assert a.dtype == np.uint8 and np.array_equal(a, b)
        assert v.jfif_header(150, 272, q) == jf.header(150, 272, q, 17)
    hdr = v.jfif_header(23, 17, 90)
    assert hdr[:4] == b"\xff\xd8\xff\xe0" and hdr[6:11] == b"JFIF\0"
    marks = [hdr[m.start() + 1] for m in re.finditer(rb"\xff(?=[\xc0\xc4\xdb\xdd\xda\xe0\xd8])", hdr)]
    assert marks == [0xD8, 0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    sof = hdr.index(b"\xff\xc0")
    assert hdr[sof + 4:sof + 19] == bytes([8, 0, 23, 0, 17, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])       # the true size; 2x2, 1x1, 1x1
    dri = hdr.index(b"\xff\xdd")
    assert hdr[dri + 2:dri + 6] == bytes([0, 4, 0, 2])                                                   # 2 MCUs per interval
    for bad in (0, 101):
        with pytest.raises(ValueError, match="quality"):
            v.quant_tables(bad)


# ------------------------------------------------------------------------------------------------------------ AVI
def _pcm(n, channels, seed=3):
    return np.random.default_rng(seed).integers(-32768, 32768, (n, channels)).astype(np.int16)


@pytest.mark.parametrize("channels,fps,rate", [(1, 30, 16000), (2, 25, 44100), (1, 7, 16001)])
def test_avi_writer_walks_clean(rg, tmp_path, channels, fps, rate):
    n = 5
    imgs = [np.roll(jf.images()["noise_17x23"], k, axis=1) for k in range(n)]
    files = [jf.jfif_file(im, 90 if k % 2 else 50) for k, im in enumerate(imgs)]          # odd and even lengths among them
    assert {len(f) & 1 for f in files} == {0, 1}
    pcm = _pcm(rate * n // fps + 977, channels)                                            # longer than the video
    path = str(tmp_path / "a.avi")
    with rg.video.AVIWriter(path, fps, 17, 23, audio=(rate, pcm)) as w:
        for f in files:
            w.add_frame(f)
    with open(path, "rb") as f:
        data = f.read()
    a = jf.walk_avi(data)
    assert a["avih"]["total_frames"] == n and a["avih"]["streams"] == 2 and a["avih"]["flags"] & 0x10
    assert (a["avih"]["width"], a["avih"]["height"]) == (17, 23) and a["avih"]["us_per_frame"] == round(1e6 / fps)
    (vh, vf), (ah, af) = a["streams"]
    assert (vh["type"], vh["handler"], vh["scale"], vh["rate"], vh["length"]) == (b"vids", b"MJPG", 1, fps, n)
    assert vh["frame"] == (0, 0, 17, 23) and vh["suggested_buffer"] == max(len(f) for f in files)
    assert len(vf) == 40 and vf[:4] == (40).to_bytes(4, "little") and vf[16:20] == b"MJPG"
    assert int.from_bytes(vf[4:8], "little") == 17 and int.from_bytes(vf[8:12], "little") == 23
    assert ah["type"] == b"auds" and ah["rate"] / ah["scale"] == rate and ah["sample_size"] == 2 * channels
    assert af == (1).to_bytes(2, "little") + channels.to_bytes(2, "little") + rate.to_bytes(4, "little") + \
        (rate * 2 * channels).to_bytes(4, "little") + (2 * channels).to_bytes(2, "little") + (16).to_bytes(2, "little") + b"\0\0"
    assert a["video"] == files and all(flags == 0x10 for _, flags, _, _ in a["index"])
    assert [c for c, _, _, _ in a["index"]] == [b"00dc", b"01wb"] * n
    back = np.frombuffer(b"".join(a["audio"]), "<i2").reshape(-1, channels)
    assert back.shape[0] == n * rate // fps == ah["length"] and np.array_equal(back, pcm[:back.shape[0]])     # cut at n / fps
    for k, chunk in enumerate(a["audio"]):                                                # frame k's interval, nothing else
        assert len(chunk) == 2 * channels * ((k + 1) * rate // fps - k * rate // fps)
    for f, im in zip(a["video"], imgs):
        assert _decode(f).size == (17, 23)


def test_avi_writer_without_audio_short_audio_and_float_samples(rg, tmp_path):
    files = [jf.jfif_file(jf.images()["black_16x16"], 90)] * 4
    path = str(tmp_path / "v.avi")
    with rg.video.AVIWriter(path, 30, 16, 16) as w:
        for f in files:
            w.add_frame(f)
    a = jf.walk_avi(open(path, "rb").read())
    assert a["avih"]["streams"] == 1 and len(a["streams"]) == 1 and a["video"] == files and not a["audio"]
    # float samples are rounded and clipped; a sound shorter than the video ends where it ends
    x = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 1.4 / 32768, 1.6 / 32768, -1.6 / 32768], np.float32)
    want = np.array([0, 16384, -16384, 32767, -32768, 32767, -32768, 1, 2, -2], np.int16)
    assert np.array_equal(rg.video.pcm16(x)[:, 0], want)
    wav = str(tmp_path / "s.wav")
    with wave.open(wav, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(100)
        f.writeframes(want.astype("<i2").tobytes())
    with rg.video.AVIWriter(path, 10, 16, 16, audio=wav) as w:                            # a path: read by audio.read_wav
        for f in files:
            w.add_frame(f)
    a = jf.walk_avi(open(path, "rb").read())
    assert np.array_equal(np.frombuffer(b"".join(a["audio"]), "<i2"), want) and len(a["audio"]) == 1 and len(a["video"]) == 4
    assert a["streams"][1][0]["length"] == 10


def test_avi_writer_names_the_two_gib_limit(rg, tmp_path, monkeypatch):
    monkeypatch.setattr(rg.video, "AVI_LIMIT", 4096)
    frame = jf.jfif_file(jf.images()["black_16x16"], 90)
    path = str(tmp_path / "big.avi")
    w = rg.video.AVIWriter(path, 30, 16, 16)
    with pytest.raises(rg.video.AVISizeError, match="2 GiB"):
        for _ in range(10):
            w.add_frame(frame)
    w.close()
    a = jf.walk_avi(open(path, "rb").read())                 # what was written before the limit is a whole file
    assert 1 <= len(a["video"]) < 10 and os.path.getsize(path) < 4096


# ------------------------------------------------------------------------------------------------------------ C ABI, command line
def test_header_has_the_prototypes_and_no_new_struct(rg):
    syms, protos = rg.capi.header_symbols(), rg.capi.header_prototypes()
    for s, n in ENTRY.items():
        assert s in syms and protos[s][0] is ctypes.c_int and len(protos[s][1]) == n, s
    assert protos["rg_jpeg_entropy_write"][1][-2] is ctypes.c_int64
    assert len(rg.capi.header_structs()) == 23 and rg.capi.header_version() >= 125
    consts = rg.capi.header_constants()
    assert (consts["RG_JPEG_MCU"], consts["RG_JPEG_BLOCKS"], consts["RG_JPEG_MAX_MCUS"]) == (16, 6, 4096)
    assert (rg.video.MCU, rg.video.BLOCKS) == (16, 6)


def test_library_exports_the_entry_points(rg):
    b = importlib.import_module("rag-gesture_amd.build")
    src = os.path.join(b.CSRC, "rg_jpeg.hip")
    assert src in b.sources() and b.flags_for(src) == b.FLAGS and "rg_jpeg.hip" not in b.PACKED_FP32_UNITS
    b.build(verbose=False)
    lib = rg.capi.load_library()
    assert lib.rg_version() >= 125
    for s, n in ENTRY.items():
        assert len(getattr(lib, s).argtypes) == n, s


def test_jpeg_kernels_use_no_scratch_and_fit_the_default_lds(tmp_path):
    b = importlib.import_module("rag-gesture_amd.build")
    src = os.path.join(b.CSRC, "rg_jpeg.hip")
    r = subprocess.run([b._hipcc()] + b.flags_for(src) + ["--cuda-device-only", "-S", src, "-o", str(tmp_path / "jpeg.s"),
                                                         "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"remark:\s+Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"remark:\s+LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == 3 and all("jpeg_" in n for n in names), names               # the transform, the coder counting and writing
    assert scratch == [0, 0, 0], dict(zip(names, scratch))
    assert max(lds) <= 64 * 1024, dict(zip(names, lds))


def test_command_line_accepts_the_new_options(rg):
    ap = rg.render.build_parser()
    a = ap.parse_args(["exp", "--smplx_path", "m.npz", "--mjpeg", "--quality", "75"])
    assert a.mjpeg and a.quality == 75 and not a.png
    d = ap.parse_args(["exp", "--smplx_path", "m.npz"])
    assert not d.mjpeg and d.quality == 90
    for bad in (["--mjpeg", "--png"], ["--mjpeg", "--quality", "0"]):
        with pytest.raises(SystemExit) as e:
            rg.render.main(["exp", "--smplx_path", "m.npz"] + bad)
        assert e.value.code == 2
