"""Rendered frames as a playable video without any program beside this package: Motion-JPEG in an AVI file, with the clip's sound.

    JPEGEncoder    uint8 RGB frames on the device -> baseline JPEG (ITU-T T.81: 8 bit, YCbCr 4:2:0, the Annex K.3 Huffman tables,
                   one restart interval per MCU row) in three launches per chunk of frames (csrc/rg_jpeg.hip):
                   rg_jpeg_dct_quant -> rg_jpeg_entropy_count -> (an exclusive sum of the lengths) -> rg_jpeg_entropy_write
    AVIWriter      RIFF 'AVI ' on the host: one 00dc chunk per frame, the sound as PCM16 in one 01wb chunk per frame, idx1
    write_mjpeg    the chunks of render.iter_gt_pred_side_by_side / iter_pred_retrieval_side_by_side -> an .avi file

The tools of the reference write H.264 in MP4 through ffmpeg (mogen/utils/visualization.py:71-136), and so does
render.write_video where there is an ffmpeg; this is the project's own encoder for the machines that have none.  No CPU
fallback: the encoder needs the device.
"""
import fractions
import os
import struct

import numpy as np
import torch

from . import audio as _audio
from . import capi

MCU = capi.header_constants()["RG_JPEG_MCU"]
BLOCKS = capi.header_constants()["RG_JPEG_BLOCKS"]

# T.81 Annex K.1 / K.2, row-major
LUMA_QUANT = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80,
              62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98,
              112, 100, 103, 99)
CHROMA_QUANT = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
                99, 99) + (99,) * 32
# zig-zag position -> row-major index (T.81 figure 5)
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
          49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# T.81 Annex K.3: (table class << 4 | destination, BITS, HUFFVAL) in the order the header lists them
_AC_LUMA = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
    "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8"
    "b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445"
    "464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6"
    "b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
HUFFMAN = ((0x00, bytes((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)), bytes(range(12))),
           (0x10, bytes((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125)), _AC_LUMA),
           (0x01, bytes((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)), bytes(range(12))),
           (0x11, bytes((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119)), _AC_CHROMA))

AVIF_HASINDEX = 0x10
AVIF_ISINTERLEAVED = 0x100
AVIIF_KEYFRAME = 0x10
AVI_LIMIT = 2 ** 31          # a RIFF file without the OpenDML extension: 2 GiB


class AVISizeError(RuntimeError):
    """The file would pass the 2 GiB an AVI without the OpenDML extension can hold."""


def quant_tables(quality):
    """Annex K.1 / K.2 scaled the way libjpeg does -> (luma, chroma), uint8 [64] each in zig-zag order."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality must lie in [1, 100], got %r" % (quality,))
    s = 5000 // q if q < 50 else 200 - 2 * q
    scaled = lambda base: np.clip((np.asarray(base, np.int64) * s + 50) // 100, 1, 255).astype(np.uint8)[list(ZIGZAG)]
    return scaled(LUMA_QUANT), scaled(CHROMA_QUANT)


def _segment(marker, body):
    return struct.pack(">BBH", 0xFF, marker, len(body) + 2) + body


def jfif_header(height, width, quality):
    """Everything of a JFIF file in front of the scan: SOI, APP0, DQT x 2, SOF0 (2x2, 1x1, 1x1), DHT x 4, DRI, SOS."""
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    out += _segment(0xDB, b"\0" + ql.tobytes()) + _segment(0xDB, b"\1" + qc.tobytes())
    out += _segment(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes((1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for ident, bits, vals in HUFFMAN:
        out += _segment(0xC4, bytes((ident,)) + bits + vals)
    out += _segment(0xDD, struct.pack(">H", -(-width // MCU)))             # one restart interval = one MCU row
    return out + _segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


class JPEGEncoder:
    """Baseline JPEG of uint8 RGB frames on the device.  frames: a device tensor [n, H, W, 3], contiguous or a column range of a
    contiguous buffer (a panel of a side-by-side picture); any H, W in [1, 65535]."""

    def __init__(self, device="cuda", quality=90, timed=False):
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise capi.RgError("JPEGEncoder needs the GPU (there is no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.h = capi.get_handle(self.device.index)
        self.quality = int(quality)
        ql, qc = quant_tables(self.quality)
        self.q_luma, self.q_chroma = torch.from_numpy(ql).to(self.device), torch.from_numpy(qc).to(self.device)
        self.headers = {}                # (H, W) -> the file's bytes in front of the scan
        self.bytes_per_pixel = 0.75      # the first guess of encode()'s buffer: a quarter of the raw frame
        self.timed, self._events = bool(timed), []

    # ------------------------------------------------------------------------------------------------------- launches
    def _check(self, frames):
        f = frames
        if not (torch.is_tensor(f) and f.is_cuda and f.dtype == torch.uint8 and f.ndim == 4 and f.shape[3] == 3):
            raise ValueError("frames must be a uint8 device tensor [n, H, W, 3]")
        n, H, W, _ = (int(x) for x in f.shape)
        if n < 1 or not (1 <= H <= 65535 and 1 <= W <= 65535):
            raise ValueError("frames must hold at least one frame of 1 .. 65535 pixels a side, got %s" % (tuple(f.shape),))
        s = f.stride()
        if not (s[3] == 1 and s[2] == 3 and s[1] % 3 == 0 and s[1] >= 3 * W and (n == 1 or s[0] == H * s[1])):
            raise ValueError("frames must be contiguous or a column range of a contiguous [n, H, pitch, 3] buffer, got strides %s" % (s,))
        return n, H, W, s[1] // 3

    def _timed(self, fn):
        if not self.timed:
            return fn()
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        out = fn()
        ev[1].record()
        self._events.append(ev)
        return out

    def device_ms(self):
        """The device time of every launch since the encoder was made (timed=True), in milliseconds."""
        torch.cuda.synchronize(self.device)
        return sum(a.elapsed_time(b) for a, b in self._events)

    def coefficients(self, frames):
        """-> int16 [n, MCU rows * MCU columns, 6, 64] on the device: the quantised DCT coefficients of the blocks Y00, Y01, Y10,
        Y11, Cb, Cr of every 16 x 16 MCU, in zig-zag order."""
        n, H, W, pitch = self._check(frames)
        rows, cols = -(-H // MCU), -(-W // MCU)
        coef = torch.empty(n, rows * cols, BLOCKS, 64, device=self.device, dtype=torch.int16)
        self.h.call("jpeg_dct_quant", frames.data_ptr(), n, H, W, pitch, self.q_luma, self.q_chroma, coef)
        return coef

    def count(self, coef, n, rows, cols):
        """The interval lengths of coefficients [n, rows * cols, 6, 64] -> (offsets int64 [n * rows], the exclusive sum of the
        lengths, and frame_off int64 [n + 1]), on the device."""
        lengths = torch.empty(n * rows, device=self.device, dtype=torch.int32)
        self.h.call("jpeg_entropy_count", coef, n, rows, cols, lengths)
        ends = torch.cumsum(lengths, 0, dtype=torch.int64)
        offsets = (ends - lengths).contiguous()
        frame_off = torch.cat([offsets[::rows], ends[-1:]]).contiguous()
        return offsets, frame_off

    def write(self, coef, n, rows, cols, offsets, out):
        """The intervals' bytes into out (uint8, contiguous, on the device) at their offsets; nothing beyond its end."""
        self.h.call("jpeg_entropy_write", coef, n, rows, cols, offsets, out.data_ptr(), int(out.numel()))

    def entropy(self, coef, rows, cols):
        """Coefficients [n, rows * cols, 6, 64] int16 on the device -> (bytes uint8 [total], frame_off int64 [n + 1]) on the
        device: frame i's scan is bytes[frame_off[i]:frame_off[i + 1]]."""
        if not (torch.is_tensor(coef) and coef.is_cuda and coef.dtype == torch.int16 and coef.is_contiguous()
                and coef.ndim == 4 and tuple(coef.shape[1:]) == (rows * cols, BLOCKS, 64)):
            raise ValueError("coef must be a contiguous int16 device tensor [n, %d, %d, 64]" % (rows * cols, BLOCKS))
        n = int(coef.shape[0])
        offsets, frame_off = self.count(coef, n, rows, cols)
        out = torch.empty(max(int(frame_off[-1]), 1), device=self.device, dtype=torch.uint8)
        self.write(coef, n, rows, cols, offsets, out)
        return out, frame_off

    def scan(self, frames):
        """-> (bytes uint8 [total], frame_off int64 [n + 1]), both on the device: the entropy-coded scans of the frames one after
        the other, exactly as long as they are."""
        n, H, W, _ = self._check(frames)
        return self._timed(lambda: self.entropy(self.coefficients(frames), -(-H // MCU), -(-W // MCU)))

    def header(self, height, width):
        key = (int(height), int(width))
        if key not in self.headers:
            self.headers[key] = jfif_header(key[0], key[1], self.quality)
        return self.headers[key]

    def encode(self, frames):
        """-> a list of n complete JFIF files (bytes).  One device-to-host copy per call: the frames' offsets and their scans
        travel in one buffer, sized by what the frames before took (a chunk that outgrows it is written and copied again)."""
        n, H, W, _ = self._check(frames)
        rows, cols = -(-H // MCU), -(-W // MCU)
        head = 8 * (n + 1)

        def launch():
            coef = self.coefficients(frames)
            return (coef,) + self.count(coef, n, rows, cols)
        coef, offsets, frame_off = self._timed(launch)
        capacity = int(n * (H * W * self.bytes_per_pixel + 1024))
        while True:
            packed = torch.empty(head + capacity, device=self.device, dtype=torch.uint8)
            packed[:head].view(torch.int64).copy_(frame_off)
            self._timed(lambda: self.write(coef, n, rows, cols, offsets, packed[head:]))
            host = packed.cpu().numpy()
            off = host[:head].view(np.int64)
            if off[-1] <= capacity:
                break
            capacity = int(off[-1]) * 5 // 4
            self.bytes_per_pixel = capacity / float(n * H * W)
        hdr, body = self.header(H, W), host[head:]
        return [hdr + body[off[i]:off[i + 1]].tobytes() + b"\xff\xd9" for i in range(n)]


# ----------------------------------------------------------------------------------------------------------- AVI
def pcm16(frames):
    """Samples as audio.read_wav returns them -> int16 [n, channels]: int16 as it is, int32 and packed 24-bit by their upper 16
    bits, float by round(x * 32768) clipped to the int16 range."""
    a = np.asarray(frames)
    if a.dtype == np.uint8:                                   # [n, channels, 3] or [n, 3] little-endian bytes
        if a.ndim not in (2, 3) or a.shape[-1] != 3:
            raise ValueError("24-bit samples must be [n, channels, 3] uint8, got %s" % (a.shape,))
        a = (a[..., 1].astype(np.uint16) | (a[..., 2].astype(np.uint16) << 8)).view(np.int16)
    elif a.dtype == np.int32:
        a = (a >> 16).astype(np.int16)
    elif a.dtype.kind == "f":
        a = np.clip(np.rint(a.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    elif a.dtype != np.int16:
        raise ValueError("audio must be int16, int32, float or packed 24-bit samples, got %s" % a.dtype)
    if a.ndim == 1:
        a = a[:, None]
    if a.ndim != 2 or a.shape[1] < 1:
        raise ValueError("audio must be [n] or [n, channels], got %s" % (a.shape,))
    return np.ascontiguousarray(a.astype("<i2", copy=False))


class AVIWriter:
    """A Motion-JPEG AVI file: RIFF 'AVI ' { LIST hdrl { avih, LIST strl { strh vids / MJPG, strf BITMAPINFOHEADER } [, LIST strl
    { strh auds, strf WAVEFORMATEX PCM } ] }, LIST movi { 00dc [, 01wb] per frame }, idx1 }.  audio: None, a WAV file's path, or
    (rate, samples) with the samples as audio.read_wav returns them; it is cut to frames / fps seconds (frame k is followed by
    the samples [k rate / fps, (k + 1) rate / fps); a frame past the sound's end has no 01wb chunk).  Every chunk is padded to
    an even length, every idx1 entry is a key frame with its offset counted from the 'movi' fourcc, and the sizes are patched
    when the file is closed.  A chunk that would take the file past 2 GiB raises AVISizeError; what was written stays valid."""

    def __init__(self, path, fps, width, height, audio=None):
        rate = fractions.Fraction(fps).limit_denominator(100000)
        if rate <= 0:
            raise ValueError("fps must be positive, got %r" % (fps,))
        self.path, self.rate, self.width, self.height = os.fspath(path), rate, int(width), int(height)
        if not (1 <= self.width <= 65535 and 1 <= self.height <= 65535):
            raise ValueError("width / height must lie in [1, 65535], got %d x %d" % (self.width, self.height))
        self.samples = self.sample_rate = None
        if audio is not None:
            if isinstance(audio, (str, os.PathLike)):
                sr, _, _, frames = _audio.read_wav(audio)
            else:
                sr, frames = audio
            self.sample_rate, self.samples = int(sr), pcm16(frames)
            if self.sample_rate < 1:
                raise ValueError("the audio's rate must be positive, got %r" % (sr,))
        self.frames = self.audio_frames = self.max_video = self.max_audio = 0
        self.index = []
        os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
        self.f = open(self.path, "wb")
        self.f.write(self._header(0))
        self.movi = self.f.tell() - 4                        # the 'movi' fourcc
        self.pos = self.f.tell()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _header(self, movi_size):
        n, num, den = self.frames, self.rate.numerator, self.rate.denominator
        has_audio = self.samples is not None
        seconds = max(n * den / num, 1e-9)
        strl = [self._strl(struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, den, num, 0, n, self.max_video, 0xFFFFFFFF, 0,
                                       0, 0, self.width, self.height),
                           struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0,
                                       0, 0))]
        if has_audio:
            ch = self.samples.shape[1]
            align, per_sec = 2 * ch, 2 * ch * self.sample_rate
            strl.append(self._strl(struct.pack("<4s4sIHHIIIIIIII4H", b"auds", b"\0\0\0\0", 0, 0, 0, 0, align, per_sec, 0, self.audio_frames,
                                               self.max_audio, 0xFFFFFFFF, align, 0, 0, 0, 0),
                                   struct.pack("<HHIIHHH", 1, ch, self.sample_rate, per_sec, align, 16, 0)))
        total = movi_size + 16 * len(self.index)
        avih = struct.pack("<14I", int(round(1e6 * den / num)), min(int(total / seconds), 0xFFFFFFFF), 0,
                           AVIF_HASINDEX | (AVIF_ISINTERLEAVED if has_audio else 0), n, 0, len(strl), max(self.max_video, self.max_audio),
                           self.width, self.height, 0, 0, 0, 0)
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"".join(strl)
        head = b"LIST" + struct.pack("<I", len(hdrl)) + hdrl + b"LIST" + struct.pack("<I", 4 + movi_size) + b"movi"
        riff = 4 + len(head) + movi_size + 8 + 16 * len(self.index)
        return b"RIFF" + struct.pack("<I", riff) + b"AVI " + head

    @staticmethod
    def _strl(strh, strf):
        body = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        return b"LIST" + struct.pack("<I", len(body)) + body

    def _chunk(self, fourcc, data):
        size = len(data)
        after = self.pos + 8 + size + (size & 1) + 8 + 16 * (len(self.index) + 1)         # ... and the index behind it
        if after >= AVI_LIMIT:
            raise AVISizeError("%s: frame %d would take the file past the 2 GiB limit of an AVI without the OpenDML extension"
                               % (self.path, self.frames))
        self.index.append((fourcc, AVIIF_KEYFRAME, self.pos - self.movi, size))
        self.f.write(fourcc + struct.pack("<I", size))
        self.f.write(data)
        if size & 1:
            self.f.write(b"\0")
        self.pos += 8 + size + (size & 1)

    def add_frame(self, jpeg):
        """One frame (a complete JPEG file's bytes), and the sound of its interval."""
        if self.f is None:
            raise ValueError("%s is closed" % self.path)
        self._chunk(b"00dc", jpeg)
        self.max_video = max(self.max_video, len(jpeg))
        if self.samples is not None:
            num, den = self.rate.numerator, self.rate.denominator
            lo = min(self.frames * self.sample_rate * den // num, self.samples.shape[0])
            hi = min((self.frames + 1) * self.sample_rate * den // num, self.samples.shape[0])
            if hi > lo:
                data = self.samples[lo:hi].tobytes()
                self._chunk(b"01wb", data)
                self.max_audio, self.audio_frames = max(self.max_audio, len(data)), hi
        self.frames += 1

    def close(self):
        if self.f is None:
            return
        f, self.f = self.f, None
        try:
            f.write(b"idx1" + struct.pack("<I", 16 * len(self.index)))
            f.write(b"".join(struct.pack("<4sIII", *e) for e in self.index))
            f.seek(0)
            f.write(self._header(self.pos - self.movi - 4))
        finally:
            f.close()


def write_mjpeg(frames_iter, path, fps, audio_path=None, quality=90, encoder=None):
    """The chunks of a renderer's generator (uint8 [c, H, W, 3] device tensors, each overwritten by the next) -> the AVI file
    `path`, with the sound of audio_path when that file exists (cut to the video's length).  Each chunk is encoded on the device
    and comes to the host as JPEG bytes, never as pixels.  -> the number of frames."""
    enc, writer, count = encoder, None, 0
    try:
        for chunk in frames_iter:
            if enc is None:
                enc = JPEGEncoder(chunk.device if torch.is_tensor(chunk) and chunk.is_cuda else "cuda", quality)
            chunk = torch.as_tensor(chunk).to(enc.device)
            if chunk.ndim == 3:
                chunk = chunk[None]
            files = enc.encode(chunk)
            if writer is None:
                audio = audio_path if audio_path and os.path.exists(audio_path) else None
                writer = AVIWriter(path, fps, int(chunk.shape[2]), int(chunk.shape[1]), audio)
            elif (int(chunk.shape[2]), int(chunk.shape[1])) != (writer.width, writer.height):
                raise ValueError("a chunk of %d x %d frames in a video of %d x %d" % (chunk.shape[2], chunk.shape[1], writer.width, writer.height))
            for f in files:
                writer.add_frame(f)
                count += 1
    finally:
        if writer is not None:
            writer.close()
    if writer is None:
        raise ValueError("no frames to encode")
    return count
