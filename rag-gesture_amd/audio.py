"""Audio onsets on the device: what beat alignment (evaluation.JointMetrics, `align` / `gt_align`) needs from a clip's
gt_audio.wav, without librosa.

    waveforms at 16 kHz --rg_onset_mel_db--> mel spectrogram in dB [frames, 128] and the clips' maxima
                        --rg_onset_pick----> normalised onset envelope, its 7-frame mean, the onset frames

The two kernels restate the defaults of librosa.onset.onset_detect(y, sr=16000, hop_length=512, units="time"), the call of
alignment.load_audio (mogen/models/utils/metric.py:64-76): an STFT of 2048 samples every 512, centred with zero padding, a
periodic Hann window, 128 Slaney mel filters up to 8 kHz, power_to_db with top_db = 80, the mean positive band difference
shifted by 3 frames, and peak_pick with pre_max 0, post_max 1, pre_avg 3, post_avg 4, wait 0, delta 0.07 (DESIGN.md "Audio
onsets").  Every clip of a call goes through the same two launches (concatenated samples, int64 offsets).

In front of that, recorded audio of any rate, channel count and sample format becomes 16 kHz mono on the device:

    WAV file --read_wav--> interleaved frames as stored --rg_resample_poly--> float32 mono at 16 kHz

`Resampler` decodes, downmixes (the mean of the channels, librosa.to_mono) and resamples by a polyphase Kaiser-windowed sinc
(`resample_filter`, DESIGN.md "Resampling"), one launch per group of clips that share rate, channels and format.  It stands where
the reference calls librosa.load and librosa.resample (mogen/datasets/beatx_dataset.py:474-475); parity with librosa's soxr_hq
filter is not pinned and not claimed.
"""
import ctypes
import math
import os
import struct
import wave

import numpy as np
import torch

from . import capi
from .evaluation import ALIGN_MASK, POSE_FPS

SR = 16000                       # evaluation.AUDIO_SR
N_FFT, HOP, N_MELS, MEL_STRIDE = (capi.header_constants()["RG_ONSET_" + k] for k in ("N_FFT", "HOP", "MELS", "MEL_STRIDE"))
N_BINS = N_FFT // 2 + 1
FMAX = 8000.0
TOP_DB = 80.0
PRE_AVG, POST_AVG = 3, 4         # 0.10 * sr // hop and 0.10 * sr // hop + 1
DELTA = 0.07

# resample_filter's defaults.  Measured for 48, 44.1, 32, 24, 22.05, 11.025 and 8 kHz input (DESIGN.md "Resampling"): at most
# 0.017 dB of droop up to 0.85 of the lower Nyquist, at least 54 dB of rejection from 1.05 of it, sum |h| per phase 1.72 .. 2.33
FILTER_ZEROS = 32
FILTER_BETA = 14.0
FILTER_ROLLOFF = 0.95
MAX_UP = 640                     # phases of the table (11.025 kHz); more is refused
PCM16, PCM24, PCM32, F32 = (capi.header_constants()["RG_RESAMPLE_" + k] for k in ("PCM16", "PCM24", "PCM32", "F32"))
RESAMPLE_TILE, MAX_CHANNELS = (capi.header_constants()["RG_RESAMPLE_" + k] for k in ("TILE", "MAX_CHANNELS"))
RESAMPLE_LDS = 64 * 1024         # bytes of a tile's staged input span (and, up to two phases, the table) the kernel may use
FORMAT_NAMES = {PCM16: "pcm16", PCM24: "pcm24", PCM32: "pcm32", F32: "f32"}
_SCALE = {PCM16: 2.0 ** -15, PCM24: 2.0 ** -23, PCM32: 2.0 ** -31, F32: 1.0}
_DTYPE = {PCM16: np.int16, PCM24: np.uint8, PCM32: np.int32, F32: np.float32}

OnsetMelArgs = capi.struct("rg_onset_mel_args")
OnsetPickArgs = capi.struct("rg_onset_pick_args")


def _hz_to_mel(f):
    """Slaney's scale: 200 / 3 Hz per mel below 1 kHz, logarithmic with step ln(6.4) / 27 above."""
    f = np.asarray(f, np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1.0) / 1000.0) / (np.log(6.4) / 27.0), f / (200.0 / 3.0))


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), m * (200.0 / 3.0))


def mel_filterbank():
    """librosa.filters.mel(sr=16000, n_fft=2048, n_mels=128, fmax=8000) restated -> [128, 1025] float64: triangles between 130
    equally spaced mel points over the bin frequencies linspace(0, 8000, 1025), each scaled by 2 / (f[i + 2] - f[i])."""
    f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(FMAX), N_MELS + 2))
    bins = np.linspace(0.0, SR / 2.0, N_BINS)
    lower = (bins[None, :] - f[:-2, None]) / (f[1:-1] - f[:-2])[:, None]
    upper = (f[2:, None] - bins[None, :]) / (f[2:] - f[1:-1])[:, None]
    return np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (f[2:] - f[:-2]))[:, None]


def mel_table(bank=None):
    """The filter bank as the kernel reads it: (start [128] int32, length [128] int32, weights [128, MEL_STRIDE] float32); every
    filter's support is one contiguous range of bins."""
    bank = mel_filterbank() if bank is None else np.asarray(bank, np.float64)
    start, length = np.zeros(N_MELS, np.int32), np.zeros(N_MELS, np.int32)
    weights = np.zeros((N_MELS, MEL_STRIDE), np.float32)
    for i, row in enumerate(bank):
        nz = np.nonzero(row)[0]
        if nz.size == 0:
            continue
        a, b = int(nz[0]), int(nz[-1]) + 1
        if b - a > MEL_STRIDE:
            raise ValueError("mel filter %d covers %d bins, more than %d" % (i, b - a, MEL_STRIDE))
        start[i], length[i] = a, b - a
        weights[i, :b - a] = row[a:b]
    return start, length, weights


def n_frames(n_samples):
    return 1 + int(n_samples) // HOP


def _float_wav(path):
    """A RIFF / WAVE file of 32-bit IEEE float samples (format tag 3, or the extensible tag with that sub-format), which the
    standard library's `wave` does not open -> (channels, rate, samples float32)."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError("%s: not a RIFF / WAVE file" % path)
    pos, fmt, samples = 12, None, None
    while pos + 8 <= len(data):
        tag, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if tag == b"fmt " and len(body) >= 16:
            code, channels, rate, _, _, bits = struct.unpack("<HHIIHH", body[:16])
            if code == 0xFFFE and len(body) >= 26:
                code = struct.unpack("<H", body[24:26])[0]
            fmt = (code, channels, rate, bits)
        elif tag == b"data":
            samples = body
        pos += 8 + size + (size & 1)
    if fmt is None or samples is None:
        raise ValueError("%s: no fmt or data chunk" % path)
    if fmt[0] != 3 or fmt[3] != 32:
        raise ValueError("%s: format tag %d with %d bits; PCM16 or 32-bit float expected" % (path, fmt[0], fmt[3]))
    return fmt[1], fmt[2], np.frombuffer(samples[:len(samples) // 4 * 4], "<f4").astype(np.float32)


def read_wav_16k(path):
    """A 16 kHz mono WAV file -> float32 samples: PCM16 (what the tools' sf.write(path, audio, 16000) produces) over 32768, or
    32-bit float as stored.  Any other rate or channel count is a ValueError: there is no resampler here."""
    path = os.fspath(path)
    try:
        with wave.open(path, "rb") as w:
            channels, rate, width = w.getnchannels(), w.getframerate(), w.getsampwidth()
            raw = w.readframes(w.getnframes()) if (channels, rate, width) == (1, SR, 2) else b""
        if width != 2:
            raise ValueError("%s: %d-bit PCM; the file must be PCM16 or 32-bit float" % (path, 8 * width))
        audio = np.frombuffer(raw, "<i2").astype(np.float32) / 32768.0
    except wave.Error:
        channels, rate, audio = _float_wav(path)
    if channels != 1 or rate != SR:
        raise ValueError("%s: %d Hz, %d channel(s); the file must be 16 kHz mono" % (path, rate, channels))
    return audio


def read_wav(path):
    """A WAV file of any rate and channel count -> (rate, channels, fmt, frames), nothing converted: fmt is PCM16, PCM24, PCM32
    or F32 and frames the interleaved samples as stored, [n, channels] int16 / int32 / float32, or [n, channels, 3] uint8 for
    24-bit samples (little-endian bytes).  8-bit files and every other format tag are a ValueError that names the file."""
    path = os.fspath(path)
    try:
        with wave.open(path, "rb") as w:
            channels, rate, width = w.getnchannels(), w.getframerate(), w.getsampwidth()
            raw = w.readframes(w.getnframes()) if width in (2, 3, 4) else b""
    except wave.Error:
        channels, rate, samples = _float_wav(path)
        if channels < 1:
            raise ValueError("%s: %d channels" % (path, channels))
        return rate, channels, F32, samples[:samples.size // channels * channels].reshape(-1, channels)
    if width not in (2, 3, 4):
        raise ValueError("%s: %d-bit PCM; the file must be 16-, 24- or 32-bit PCM or 32-bit float" % (path, 8 * width))
    n = len(raw) // (width * channels)
    raw = raw[:n * width * channels]
    if width == 3:
        return rate, channels, PCM24, np.frombuffer(raw, np.uint8).reshape(n, channels, 3)
    fmt, dt = (PCM16, "<i2") if width == 2 else (PCM32, "<i4")
    return rate, channels, fmt, np.frombuffer(raw, dt).astype(_DTYPE[fmt], copy=False).reshape(n, channels)


def resample_filter(rate, target=SR, zeros=FILTER_ZEROS, beta=FILTER_BETA, rolloff=FILTER_ROLLOFF):
    """The low-pass filter of a conversion rate -> target -> (up, down, half_len, h): up / down = target / rate in lowest terms,
    half_len = zeros * max(up, down), h the 2 half_len + 1 taps (float64) of a Kaiser-windowed sinc with its cutoff at
    rolloff / max(up, down) of the Nyquist frequency of the up-sampled signal, normalised to unit gain at 0 and scaled by up:
    scipy.signal.firwin(2 half_len + 1, rolloff / max(up, down), window=("kaiser", beta)) * up."""
    rate, target = int(rate), int(target)
    if rate <= 0 or target <= 0:
        raise ValueError("cannot resample from %d Hz to %d Hz" % (rate, target))
    g = math.gcd(rate, target)
    up, down = target // g, rate // g
    if up > MAX_UP:
        raise ValueError("%d Hz -> %d Hz needs %d filter phases, more than %d" % (rate, target, up, MAX_UP))
    half_len = zeros * max(up, down)
    cutoff = rolloff / max(up, down)
    t = np.arange(-half_len, half_len + 1, dtype=np.float64)
    h = cutoff * np.sinc(cutoff * t) * np.kaiser(2 * half_len + 1, beta)
    return up, down, half_len, h / h.sum() * up


def resample_table(up, half_len, h):
    """The filter as the kernel reads it -> (taps, coeff [up, taps] float32): coeff[p][j] = h[p + j up], 0 past the end of h,
    taps = 2 half_len // up + 1; float64 rounded once."""
    taps = 2 * half_len // up + 1
    padded = np.zeros(up * taps, np.float64)
    padded[:2 * half_len + 1] = h
    return taps, np.ascontiguousarray(padded.reshape(taps, up).T.astype(np.float32))


def n_resampled(n, up, down):
    """ceil(n up / down): the samples n input frames become."""
    return -(-int(n) * up // down)


def _as_frames(frames, what="clip"):
    """(fmt, channels, [n, channels(, 3)] array) of one clip's frames as Resampler.run takes them."""
    a = frames.numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
    if a.dtype == np.uint8:
        if a.ndim not in (2, 3) or a.shape[-1] != 3:
            raise ValueError("%s: packed 24-bit frames are [n, 3] or [n, channels, 3] bytes, got %s" % (what, a.shape))
        a, fmt = a[:, None, :] if a.ndim == 2 else a, PCM24
    else:
        fmt = {np.dtype(np.int16): PCM16, np.dtype(np.int32): PCM32, np.dtype(np.float32): F32}.get(a.dtype)
        if fmt is None or a.ndim not in (1, 2):
            raise ValueError("%s: frames are [n] or [n, channels] int16, int32 or float32 (or packed 24-bit bytes), got %s %s"
                             % (what, a.dtype, a.shape))
        a = a[:, None] if a.ndim == 1 else a
    if not 1 <= a.shape[1] <= MAX_CHANNELS:
        raise ValueError("%s: %d channels; 1 to %d are supported" % (what, a.shape[1], MAX_CHANNELS))
    return fmt, int(a.shape[1]), a


def decode_mono(frames):
    """One clip's frames (as Resampler.run takes them) -> float64 mono: every sample scaled, the mean of the channels."""
    fmt, channels, a = _as_frames(frames)
    if fmt == PCM24:
        b = a.astype(np.int32)
        a = ((b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)) ^ 0x800000) - 0x800000
    return (a.astype(np.float64) * _SCALE[fmt]).sum(axis=1) / channels


def cut_to_clip(audio, n):
    """evaluate.py:396-405: 16 kHz audio cut to a clip's n pose frames, then without ALIGN_MASK frames of audio at both ends."""
    audio = audio[:int(SR / POSE_FPS * n)]
    a_offset = int(ALIGN_MASK * (SR / POSE_FPS))
    return audio[a_offset:len(audio) - a_offset]


def clip_audio(pred_file, n, resampler=None):
    """evaluate.py:396-405: the gt_audio.wav beside pred_file cut to the clip's n pose frames, then without ALIGN_MASK frames of
    audio at both ends (what the onset detector hears; onset times count from that start).  The file must be 16 kHz mono unless
    a Resampler is given: then any file read_wav reads is brought to 16 kHz mono on the device first (a device tensor)."""
    path = os.path.join(os.path.dirname(pred_file), "gt_audio.wav")
    return cut_to_clip(read_wav_16k(path) if resampler is None else resampler.load([path])[0], n)


def clip_onsets(pred_file, n, detector):
    """Onset times (s) of one clip's audio after the cuts of clip_audio."""
    return detector.detect([clip_audio(pred_file, n)])[0]


class OnsetDetector:
    """onset_detect on the device for a list of clips per call (rg_onset_mel_db, rg_onset_pick)."""

    def __init__(self, device=None):
        self.device = capi.device_or_fail(device, "OnsetDetector")
        self.h = capi.get_handle(self.device.index)
        k = np.arange(N_FFT, dtype=np.float64)
        window = 0.5 - 0.5 * np.cos(2.0 * np.pi * k / N_FFT)
        twiddle = np.stack([np.cos(2.0 * np.pi * k / N_FFT), -np.sin(2.0 * np.pi * k / N_FFT)], axis=1)
        self.mel_start_host, self.mel_len_host, weights = mel_table()
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(self.device)
        self.window, self.twiddle = up(window, np.float32), up(twiddle, np.float32)       # float64 on the host, rounded once
        self.mel_start, self.mel_len = up(self.mel_start_host, np.int32), up(self.mel_len_host, np.int32)
        self.mel_weight = up(weights, np.float32)

    def run(self, waves):
        """waves: a list of 1-D float waveforms at 16 kHz (tensors or arrays, on the host or the device; an empty one has one
        silent frame).  -> dict of device tensors over all frames, clip after clip: db [F, 128] (clamped), x [F], avg [F],
        onset_frames [F] int32 and onset_count [n_clips] int32, with frame_off [n_clips + 1] (numpy int64)."""
        waves = list(waves)
        if not waves:
            raise ValueError("no clips")
        dev = self.device
        parts = []
        for i, w in enumerate(waves):
            w = torch.as_tensor(w)
            if w.ndim != 1 or not (w.dtype.is_floating_point):
                raise ValueError("clip %d must be a 1-D float waveform, got %s %s" % (i, w.dtype, tuple(w.shape)))
            parts.append(w.to(torch.float32))
        lens = [int(p.shape[0]) for p in parts]
        sample_off = np.zeros(len(parts) + 1, np.int64)
        sample_off[1:] = np.cumsum(lens)
        frame_off = np.zeros(len(parts) + 1, np.int64)
        frame_off[1:] = np.cumsum([n_frames(n) for n in lens])
        F = int(frame_off[-1])
        if F >= 2 ** 31 // N_MELS:
            raise ValueError("too many frames in one call (%d)" % F)
        if all(not p.is_cuda for p in parts):
            samples = torch.cat(parts).to(dev)                  # one copy for the whole batch
        else:
            samples = torch.cat([p.to(dev) for p in parts])
        if samples.numel() == 0:
            samples = torch.zeros(1, device=dev)
        samples = samples.contiguous()
        soff_dev, foff_dev = torch.from_numpy(sample_off).to(dev), torch.from_numpy(frame_off).to(dev)
        n_clips = len(parts)
        db = torch.empty(F, N_MELS, device=dev, dtype=torch.float32)
        clip_max = torch.empty(n_clips, device=dev, dtype=torch.int32)
        x = torch.empty(F, device=dev, dtype=torch.float32)
        avg = torch.empty(F, device=dev, dtype=torch.float32)
        frames = torch.empty(F, device=dev, dtype=torch.int32)
        count = torch.empty(n_clips, device=dev, dtype=torch.int32)
        a = OnsetMelArgs(samples=samples.data_ptr(), sample_off=soff_dev.data_ptr(), sample_off_host=sample_off.ctypes.data,
                         frame_off=foff_dev.data_ptr(), frame_off_host=frame_off.ctypes.data, window=self.window.data_ptr(),
                         twiddle=self.twiddle.data_ptr(), mel_start=self.mel_start.data_ptr(), mel_len=self.mel_len.data_ptr(),
                         mel_start_host=self.mel_start_host.ctypes.data, mel_len_host=self.mel_len_host.ctypes.data,
                         mel_weight=self.mel_weight.data_ptr(), db=db.data_ptr(), clip_max=clip_max.data_ptr(), n_clips=n_clips)
        self.h.call("onset_mel_db", ctypes.byref(a))
        b = OnsetPickArgs(db=db.data_ptr(), clip_max=clip_max.data_ptr(), frame_off=foff_dev.data_ptr(),
                          frame_off_host=frame_off.ctypes.data, x=x.data_ptr(), avg=avg.data_ptr(), onset_frames=frames.data_ptr(),
                          onset_count=count.data_ptr(), n_clips=n_clips, pre_avg=PRE_AVG, post_avg=POST_AVG, top_db=TOP_DB,
                          delta=DELTA)
        self.h.call("onset_pick", ctypes.byref(b))
        return dict(db=db, x=x, avg=avg, onset_frames=frames, onset_count=count, frame_off=frame_off)

    def envelopes(self, waves):
        """Per clip (x, avg): the normalised onset envelope and its 7-frame mean, [frames] fp32 device tensors."""
        r = self.run(waves)
        off = r["frame_off"]
        return [(r["x"][off[c]:off[c + 1]], r["avg"][off[c]:off[c + 1]]) for c in range(len(off) - 1)]

    def mel_db(self, waves):
        """Per clip the mel spectrogram in dB [frames, 128] (fp32, device), clamped at the clip's maximum - 80."""
        r = self.run(waves)
        off = r["frame_off"]
        return [r["db"][off[c]:off[c + 1]] for c in range(len(off) - 1)]

    def detect_frames(self, waves):
        """Per clip the onset frame indices, ascending (numpy int64)."""
        r = self.run(waves)
        off = r["frame_off"]
        count = r["onset_count"].cpu().numpy()
        frames = r["onset_frames"].cpu().numpy()
        return [frames[off[c]:off[c] + count[c]].astype(np.int64) for c in range(len(off) - 1)]

    def detect(self, waves):
        """Per clip the onset times in seconds (numpy float64, ascending): frame * 512 / 16000."""
        return [f.astype(np.float64) * HOP / SR for f in self.detect_frames(waves)]


class Resampler:
    """Recorded audio -> float32 mono at `target` Hz on the device (rg_resample_poly): decode, downmix and polyphase resampling
    in one launch per group of clips that share (rate, channels, format)."""

    def __init__(self, device=None, target=SR):
        self.device = capi.device_or_fail(device, "Resampler")
        self.h = capi.get_handle(self.device.index)
        self.target = int(target)
        self.tables = {}                 # rate -> (up, down, half_len, taps, coeff on the device); none for rate == target

    def table(self, rate):
        rate = int(rate)
        if rate not in self.tables:
            up, down, half_len, h = resample_filter(rate, self.target)
            taps, coeff = resample_table(up, half_len, h)
            span = (RESAMPLE_TILE - 1) * down // up + 1 + taps + (up * taps if up <= 2 else 0)
            if 4 * span > RESAMPLE_LDS:
                raise ValueError("%d Hz -> %d Hz: a tile's input span (%d samples) does not fit the kernel's LDS" % (rate, self.target, span))
            self.tables[rate] = (up, down, half_len, taps, torch.from_numpy(coeff).to(self.device))
        return self.tables[rate]

    def run(self, clips):
        """clips: a list of (frames, rate); frames on the host, [n] or [n, channels] int16 / int32 / float32, or the packed
        24-bit bytes of read_wav ([n, 3] or [n, channels, 3] uint8) -> a list of 1-D float32 device tensors at `target` Hz, in
        input order.  Per group of clips that share (rate, channels, format): one host-to-device copy (offsets and frames in one
        buffer) and one launch."""
        clips = list(clips)
        if not clips:
            raise ValueError("no clips")
        groups = {}
        for i, (frames, rate) in enumerate(clips):
            fmt, channels, a = _as_frames(frames, "clip %d" % i)
            if int(rate) != self.target:
                self.table(rate)                               # (refuses a rate before anything is copied)
            groups.setdefault((int(rate), channels, fmt), []).append((i, a))
        out = [None] * len(clips)
        for (rate, channels, fmt), members in groups.items():
            staged = self.stage(rate, channels, fmt, [a for _, a in members])
            y, out_off = self.launch(staged), staged["out_off"]
            for c, (i, _) in enumerate(members):
                out[i] = y[out_off[c]:out_off[c + 1]]
        return out

    def stage(self, rate, channels, fmt, arrays):
        """One group's frames ([n, channels(, 3)] arrays of one format) and both offset arrays in ONE buffer, copied to the
        device once -> what `launch` takes."""
        up, down, half_len, taps, coeff = (1, 1, 0, 1, None) if rate == self.target else self.table(rate)
        nc = len(arrays)
        src_off, out_off = np.zeros(nc + 1, np.int64), np.zeros(nc + 1, np.int64)
        src_off[1:] = np.cumsum([a.shape[0] for a in arrays])
        out_off[1:] = np.cumsum([n_resampled(a.shape[0], up, down) for a in arrays])
        head = 16 * (nc + 1)                                   # src_off, out_off, then the frames (16-byte aligned)
        body = [np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in arrays]
        size = sum(b.size for b in body)
        buf = np.zeros(head + max(size, 4), np.uint8)
        buf[:head // 2] = src_off.view(np.uint8)
        buf[head // 2:head] = out_off.view(np.uint8)
        np.concatenate(body, out=buf[head:head + size])
        return dict(dev=torch.from_numpy(buf).to(self.device), head=head, src_off=src_off, out_off=out_off, n_clips=nc, fmt=fmt,
                    channels=channels, filter=(up, down, half_len, taps), coeff=coeff)

    def launch(self, staged):
        """rg_resample_poly on a staged group -> the clips' samples one after the other, [out_off[-1]] float32."""
        s, dev, head = staged, staged["dev"], staged["head"]
        y = torch.empty(max(int(s["out_off"][-1]), 1), device=self.device, dtype=torch.float32)
        self.h.call("resample_poly", dev.data_ptr() + head, s["fmt"], s["channels"], dev.data_ptr(), s["src_off"].ctypes.data,
                    dev.data_ptr() + head // 2, s["out_off"].ctypes.data, s["n_clips"], *s["filter"], s["coeff"], y)
        return y

    def load(self, paths):
        """run over read_wav of every path."""
        clips = []
        for p in paths:
            rate, _, _, frames = read_wav(p)
            clips.append((frames, rate))
        return self.run(clips)

    @staticmethod
    def reference(frames, rate, target=SR, at=None):
        """The float64 restatement on the host (never a product path): y[m] = sum over k of h[m down - k up + half_len] x[k] on the
        decoded mean of the channels, for all ceil(n up / down) outputs, or for the output indices `at` only."""
        x = decode_mono(frames)
        if int(rate) == int(target):
            return x if at is None else x[np.asarray(at, np.int64)]
        up, down, half_len, h = resample_filter(rate, target)
        taps = 2 * half_len // up + 1
        hp = np.zeros(up * taps, np.float64)
        hp[:h.size] = h
        m = np.arange(n_resampled(x.size, up, down), dtype=np.int64) if at is None else np.asarray(at, np.int64)
        c = m * down + half_len
        p, k_hi = c % up, c // up
        y = np.zeros(m.size, np.float64)
        for j in range(taps):
            k = k_hi - j
            ok = (k >= 0) & (k < x.size)
            y[ok] += hp[p[ok] + j * up] * x[k[ok]]
        return y


def load_16k(paths, resampler=None):
    """WAV files of any rate, channel count and PCM16 / PCM24 / PCM32 / float32 format -> a list of 1-D float32 device tensors
    at 16 kHz mono: what features.WindowFeatures.for_clips, OnsetDetector.run and dataset.RawClip(audio=...) take."""
    return (Resampler() if resampler is None else resampler).load(paths)
