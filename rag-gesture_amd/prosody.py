"""Word prosodic prominence from speech and word timings, on the device: the `prominence` annotation ((word, start, end, value))
that discourse retrieval compares between a query and its candidates (rag/utils.py:171-228 map_conns_to_prominence picks the
connectives' values, rag/discourse_retrieval.py:172-192 scores 4 / (1 + 2 |difference|)).

The reference only CONSUMES such values: it reads prom/<recording>.prom, tab-separated `Basename start end word prominence
boundary`, which an offline wavelet-prosody tool wrote (mogen/datasets/beatx_dataset.py:660-670, :1005-1022).  Producing them is
this project's own addition, like audio.Resampler and align.CTCAligner.  The estimator follows the published recipe, restated as
arithmetic of its own (include/rg_gesture.h), in four launches for any number of recordings:

    16 kHz waveforms --rg_prosody_frames--> log energy, normalised cross-correlation, lag, log f0 per 10 ms frame
                     --rg_prosody_signal--> voicing, f0 filled across the gaps, a word-duration track; the three z-normalised and summed
                     --rg_prosody_cwt-----> a Mexican-hat wavelet transform of the sum at ten scales
                     --rg_prosody_words---> lines of maximum amplitude; per word the strongest peak line (prominence) and the
                                            strongest valley line behind its middle (boundary)

Word frames.  Frame t stands at t / 100 s; a word covers the frames whose time lies in [start, end).  Words must be sorted by start;
a word's first frame is clamped to the previous word's end frame; a word left without frames gets prominence = boundary = 0.

What is NOT claimed.  The values live on this estimator's own scale.  Parity with the tool that wrote BEAT-X's .prom files is not
pinned and not claimed (neither that tool nor annotated speech is available to the tests, which pin the arithmetic only).
Retrieval compares a DIFFERENCE of query and database prominences, so both sides must come from the same estimator: do not mix
these values with the shipped .prom files inside one database.
"""
import argparse
import json
import math
import os

import numpy as np
import torch

from . import capi

C = capi.header_constants()
SR = 16000
FRAME_RATE = 100
HOP, WIN, LAG_MIN, LAG_MAX = (C["RG_PROSODY_" + k] for k in ("HOP", "WIN", "LAG_MIN", "LAG_MAX"))
SCALES, TILE, HALO, N_TAPS = (C["RG_PROSODY_" + k] for k in ("SCALES", "TILE", "HALO", "TAPS"))
PROM_COLUMNS = ("Basename", "start", "end", "word", "prominence", "boundary")


def n_frames(n_samples):
    return 1 + int(n_samples) // HOP


def scales():
    """s_j = 2 * 2^(j / 2) frames."""
    return [2.0 * 2.0 ** (j / 2.0) for j in range(SCALES)]


def wavelet_taps():
    """The ten scales' Mexican-hat taps one after the other, float64: psi_j[k] = (1 - u^2) exp(-u^2 / 2) / sqrt(s_j), u = k / s_j,
    k = -R_j .. R_j, R_j = ceil(5 s_j).  -> (taps [RG_PROSODY_TAPS], radii)."""
    taps, radii = [], []
    for s in scales():
        R = int(math.ceil(5.0 * s))
        u = np.arange(-R, R + 1, dtype=np.float64) / s
        taps.append((1.0 - u * u) * np.exp(-0.5 * u * u) / math.sqrt(s))
        radii.append(R)
    taps = np.concatenate(taps)
    if taps.size != N_TAPS or max(radii) != HALO:
        raise capi.RgError("the wavelet table (%d taps, halo %d) disagrees with include/rg_gesture.h" % (taps.size, max(radii)))
    return taps, radii


def _first_frame_at(seconds):
    """The first frame t with t / 100 >= seconds (float64, the division as stated: no rounding surprise of seconds * 100)."""
    k = max(int(math.ceil(float(seconds) * FRAME_RATE)), 0)
    while k > 0 and (k - 1) / FRAME_RATE >= seconds:
        k -= 1
    while k / FRAME_RATE < seconds:
        k += 1
    return k


def word_frames(words, T):
    """words: [[[start, end], word], ...] of one recording of T frames -> (start_frame, end_frame) int32 arrays: the word-frame rule
    of the module docstring.  Words that are not sorted by start are a ValueError."""
    start, end = np.zeros(len(words), np.int32), np.zeros(len(words), np.int32)
    prev_end, prev_start = 0, -math.inf
    for i, seg in enumerate(words):
        s, e = float(seg[0][0]), float(seg[0][1])
        if not (math.isfinite(s) and math.isfinite(e)):
            raise ValueError("word %d (%r) has a time that is not finite" % (i, seg[1]))
        if s < prev_start:
            raise ValueError("word %d (%r) starts at %g s, before word %d (%g s): words must be sorted by start" % (i, seg[1], s, i - 1, prev_start))
        prev_start = s
        a = min(max(_first_frame_at(s), prev_end), T)
        b = min(max(_first_frame_at(e), a), T)
        start[i], end[i] = a, b
        prev_end = b
    return start, end


def _rows(path):
    with open(path, newline="") as f:
        for line in f.read().split("\n"):
            if line.strip("\r") != "":
                yield line.rstrip("\r").split("\t")


def read_prom(path):
    """A .prom file (tab-separated Basename, start, end, word, prominence, boundary; no header line) -> [(word, start, end,
    prominence), ...] as the dataset takes them; an empty word stays "" (the reference's fillna(""))."""
    return [r[:4] for r in read_prom_rows(path)]


def read_prom_rows(path):
    """-> [(word, start, end, prominence, boundary, basename), ...] of a .prom file."""
    out = []
    for n, cols in enumerate(_rows(path)):
        if len(cols) != len(PROM_COLUMNS):
            raise ValueError("%s: row %d has %d columns, expected %d (%s)" % (path, n + 1, len(cols), len(PROM_COLUMNS), ", ".join(PROM_COLUMNS)))
        out.append((cols[3], float(cols[1]), float(cols[2]), float(cols[4]), float(cols[5]), cols[0]))
    return out


def write_prom(path, basename, rows):
    """rows: (word, start, end, prominence) or (word, start, end, prominence, boundary) tuples (`run`'s) -> the reference's file
    layout; a missing boundary is written as 0.  Numbers are written so that they read back to the same float64."""
    with open(path, "w", newline="") as f:
        for r in rows:
            word = str(r[0])
            if "\t" in word or "\n" in word:
                raise ValueError("write_prom: the word %r holds a tab or a line break" % word)
            f.write("\t".join([str(basename), repr(float(r[1])), repr(float(r[2])), word, repr(float(r[3])),
                               repr(float(r[4]) if len(r) > 4 else 0.0)]) + "\n")


class ProminenceEstimator:
    """Word prominence (and boundary strength) for a list of recordings per call.  weights: of the normalised f0, energy and
    word-duration tracks in the analysed sum."""

    def __init__(self, device=None, weights=(1.0, 1.0, 0.5)):
        self.device = capi.device_or_fail(device, "ProminenceEstimator")
        self.h = capi.get_handle(self.device.index)
        self.weights = tuple(float(w) for w in weights)
        if len(self.weights) != 3:
            raise ValueError("weights: (f0, energy, duration)")
        taps, self.radii = wavelet_taps()
        self.taps = torch.from_numpy(taps.astype(np.float32)).to(self.device)          # float64 on the host, rounded once

    # ---- host side
    def _offsets(self, frame_off):
        frame_off = np.ascontiguousarray(np.asarray(frame_off, np.int64))
        if frame_off.ndim != 1 or frame_off.size < 2 or frame_off[0] != 0 or np.any(np.diff(frame_off) < 1):
            raise ValueError("frame_off: [n + 1] offsets from 0, every recording with at least one frame")
        return frame_off

    def layout(self, words, frame_off):
        """The words of every recording as the kernels read them (one host-to-device copy): word_off, start / end frames, start /
        end seconds in fp32.  words: per recording [[[start, end], word], ...]; a layout made here passes through unchanged."""
        if isinstance(words, dict):
            return words
        frame_off = self._offsets(frame_off)
        n = frame_off.size - 1
        words = [list(w) for w in words]
        if len(words) != n:
            raise ValueError("%d word lists for %d recordings" % (len(words), n))
        word_off = np.zeros(n + 1, np.int64)
        word_off[1:] = np.cumsum([len(w) for w in words])
        nw = int(word_off[-1])
        sf, ef = np.zeros(max(nw, 1), np.int32), np.zeros(max(nw, 1), np.int32)
        ws, we = np.zeros(max(nw, 1), np.float32), np.zeros(max(nw, 1), np.float32)
        for i, w in enumerate(words):
            a, b = int(word_off[i]), int(word_off[i + 1])
            try:
                sf[a:b], ef[a:b] = word_frames(w, int(frame_off[i + 1] - frame_off[i]))
            except ValueError as e:
                raise ValueError("recording %d: %s" % (i, e))
            ws[a:b] = [seg[0][0] for seg in w]
            we[a:b] = [seg[0][1] for seg in w]
        m = max(nw, 1)
        buf = np.concatenate([word_off.view(np.int32), sf, ef, ws.view(np.int32), we.view(np.int32)])
        dev = torch.from_numpy(buf).to(self.device)
        k = 2 * (n + 1)
        return dict(words=words, n_words=nw, word_off=word_off, start_frame=sf, end_frame=ef, word_off_dev=dev[:k].view(torch.int64),
                    start_frame_dev=dev[k:k + m], end_frame_dev=dev[k + m:k + 2 * m], word_start_dev=dev[k + 2 * m:k + 3 * m].view(torch.float32),
                    word_end_dev=dev[k + 3 * m:k + 4 * m].view(torch.float32))

    # ---- the four stages
    def frames(self, waves):
        """waves: a list of 1-D float waveforms at 16 kHz (tensors or arrays, host or device) -> dict of device tensors over all
        frames, recording after recording: energy, nccf, logf0 fp32 and lag int32 [F], with frame_off [n + 1] (numpy int64)."""
        waves = list(waves)
        if not waves:
            raise ValueError("no recordings")
        parts = []
        for i, w in enumerate(waves):
            w = torch.as_tensor(w)
            if w.ndim != 1 or not w.dtype.is_floating_point:
                raise ValueError("recording %d must be a 1-D float waveform, got %s %s" % (i, w.dtype, tuple(w.shape)))
            parts.append(w.to(torch.float32))
        dev, n = self.device, len(parts)
        lens = [int(p.shape[0]) for p in parts]
        sample_off, frame_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        sample_off[1:] = np.cumsum(lens)
        frame_off[1:] = np.cumsum([n_frames(k) for k in lens])
        F = int(frame_off[-1])
        if F >= 2 ** 31:
            raise ValueError("too many frames in one call (%d)" % F)
        samples = torch.cat(parts).to(dev) if all(not p.is_cuda for p in parts) else torch.cat([p.to(dev) for p in parts])
        if samples.numel() == 0:
            samples = torch.zeros(1, device=dev)
        samples = samples.contiguous()
        offs = torch.from_numpy(np.concatenate([sample_off, frame_off])).to(dev)
        out = dict(energy=torch.empty(F, device=dev), nccf=torch.empty(F, device=dev), lag=torch.empty(F, dtype=torch.int32, device=dev),
                   logf0=torch.empty(F, device=dev), frame_off=frame_off)
        self.h.call("prosody_frames", samples, offs[:n + 1], sample_off.ctypes.data, offs[n + 1:], frame_off.ctypes.data, n,
                    out["energy"], out["nccf"], out["lag"], out["logf0"])
        return out

    def signal(self, frames_out, words):
        """frames_out: `frames`' dict (energy, nccf, logf0 [F] fp32 on the device and frame_off); words: per recording [[[start, end],
        word], ...] or a `layout`.  -> dict: voiced int32, f0 (filled), f0z, ez, dz, c fp32 [F], status int32 [n] (1: no voiced frame),
        frame_off and the layout."""
        frame_off = self._offsets(frames_out["frame_off"])
        n, F, dev = frame_off.size - 1, int(frame_off[-1]), self.device
        energy, nccf, logf0 = (frames_out[k].to(dev).float().contiguous() for k in ("energy", "nccf", "logf0"))
        if not energy.shape == nccf.shape == logf0.shape == (F,):
            raise ValueError("energy, nccf and logf0 must hold the %d frames of frame_off" % F)
        lay = self.layout(words, frame_off)
        fo = torch.from_numpy(frame_off).to(dev)
        f32 = lambda: torch.empty(F, device=dev)
        out = dict(voiced=torch.empty(F, dtype=torch.int32, device=dev), f0=f32(), f0z=f32(), ez=f32(), dz=f32(), c=f32(),
                   status=torch.empty(n, dtype=torch.int32, device=dev), frame_off=frame_off, layout=lay)
        knot = torch.empty(F, dtype=torch.int32, device=dev)
        self.h.call("prosody_signal", energy, nccf, logf0, fo, frame_off.ctypes.data, lay["word_off_dev"], lay["word_off"].ctypes.data,
                    lay["start_frame_dev"], lay["end_frame_dev"], lay["start_frame"].ctypes.data, lay["end_frame"].ctypes.data,
                    lay["word_start_dev"], lay["word_end_dev"], n, *self.weights, out["voiced"], out["f0"], out["f0z"], out["ez"],
                    out["dz"], out["c"], knot, out["status"])
        return out

    def cwt(self, signal_out):
        """signal_out: a dict with c [F] fp32 on the device and frame_off -> dict: W [RG_PROSODY_SCALES, F] fp32, frame_off (and the
        layout, when signal_out carries one)."""
        frame_off = self._offsets(signal_out["frame_off"])
        n, F, dev = frame_off.size - 1, int(frame_off[-1]), self.device
        c = signal_out["c"].to(dev).float().contiguous()
        if c.shape != (F,):
            raise ValueError("c must hold the %d frames of frame_off" % F)
        tile_off = np.zeros(n + 1, np.int64)
        tile_off[1:] = np.cumsum((np.diff(frame_off) + TILE - 1) // TILE)
        offs = torch.from_numpy(np.concatenate([frame_off, tile_off])).to(dev)
        W = torch.empty(SCALES, F, device=dev)
        self.h.call("prosody_cwt", c, offs[:n + 1], frame_off.ctypes.data, offs[n + 1:], tile_off.ctypes.data, n, self.taps, W)
        out = dict(W=W, frame_off=frame_off)
        if "layout" in signal_out:
            out["layout"] = signal_out["layout"]
        return out

    def words(self, cwt_out, words=None):
        """cwt_out: a dict with W [RG_PROSODY_SCALES, F] fp32 on the device and frame_off; words as for `signal` (None: the layout
        cwt_out carries).  -> dict: peak_strength, valley_strength fp32 [F]; prominence, boundary fp32 and prom_frame, bnd_frame
        int32 [n words] (the frame, inside its recording, a word's value comes from; -1: none); word_off and the layout."""
        frame_off = self._offsets(cwt_out["frame_off"])
        n, F, dev = frame_off.size - 1, int(frame_off[-1]), self.device
        W = cwt_out["W"].to(dev).float().contiguous()
        if W.shape != (SCALES, F):
            raise ValueError("W must be [%d, %d]" % (SCALES, F))
        if words is None and "layout" not in cwt_out:
            raise ValueError("words: cwt_out carries no layout, so the words must be given")
        lay = self.layout(cwt_out["layout"] if words is None else words, frame_off)
        nw, m = lay["n_words"], max(lay["n_words"], 1)
        fo = torch.from_numpy(frame_off).to(dev)
        out = dict(peak_strength=torch.empty(F, device=dev), valley_strength=torch.empty(F, device=dev),
                   prominence=torch.zeros(m, device=dev), boundary=torch.zeros(m, device=dev),
                   prom_frame=torch.full((m,), -1, dtype=torch.int32, device=dev), bnd_frame=torch.full((m,), -1, dtype=torch.int32, device=dev))
        self.h.call("prosody_words", W, fo, frame_off.ctypes.data, lay["word_off_dev"], lay["word_off"].ctypes.data, lay["start_frame_dev"],
                    lay["end_frame_dev"], lay["start_frame"].ctypes.data, lay["end_frame"].ctypes.data, n, out["peak_strength"],
                    out["valley_strength"], out["prominence"], out["boundary"], out["prom_frame"], out["bnd_frame"])
        for k in ("prominence", "boundary", "prom_frame", "bnd_frame"):
            out[k] = out[k][:nw]
        out.update(word_off=lay["word_off"], layout=lay, frame_off=frame_off)
        return out

    # ---- composition
    def run_device(self, waves16k, words_per_recording):
        """The four stages -> `words`' dict (nothing read back)."""
        fr = self.frames(waves16k)
        lay = self.layout(words_per_recording, fr["frame_off"])
        return self.words(self.cwt(self.signal(fr, lay)))

    def run(self, waves16k, words_per_recording, boundaries=False):
        """waves16k: 16 kHz mono waveforms; words_per_recording: per recording [[[start, end], word], ...] (align_recording's form)
        -> per recording [(word, start, end, prominence), ...], the `prominence` annotation of dataset.RawClip and
        longform.window_annotations; with boundaries=True the tuples gain the boundary strength.  One read-back."""
        r = self.run_device(waves16k, words_per_recording)
        back = torch.cat([r["prominence"], r["boundary"]]).cpu().numpy()
        nw, off = r["layout"]["n_words"], r["word_off"]
        prom, bnd = back[:nw], back[nw:]
        out = []
        for i, segs in enumerate(r["layout"]["words"]):
            rows = []
            for k, seg in enumerate(segs):
                j = int(off[i]) + k
                row = (seg[1], float(seg[0][0]), float(seg[0][1]), float(prom[j]))
                rows.append(row + (float(bnd[j]),) if boundaries else row)
            out.append(rows)
        return out


def annotate(clip, estimator):
    """Fill clip.annotations["prominence"] of a dataset.RawClip from clip.audio (16 kHz mono) and clip.annotations["text_segments"]
    when it is empty; a clip that already has prominence values is left untouched.  -> the clip."""
    if clip.annotations.get("prominence"):
        return clip
    if clip.audio is None:
        raise ValueError("%s: no audio to estimate prominence from" % clip.name)
    segs = sorted(clip.annotations.get("text_segments") or [], key=lambda s: s[0][0])
    clip.annotations["prominence"] = estimator.run([clip.audio], [segs])[0]
    return clip


def main(argv=None):
    """python -m rag-gesture_amd.prosody <audio.wav> --words words.json -o out.prom [--resample_audio]"""
    from . import audio
    ap = argparse.ArgumentParser(description="word prominence and boundary strength of one recording, written as a .prom file")
    ap.add_argument("audio", help="a WAV file: 16 kHz mono, or anything audio.read_wav reads with --resample_audio")
    ap.add_argument("--words", required=True, help="JSON: [[[start, end], word], ...] in seconds (align.CTCAligner.align_recording's form)")
    ap.add_argument("-o", "--out", required=True, help="the .prom file to write")
    ap.add_argument("--basename", default=None, help="first column of the file (default: the audio file's name without its suffix)")
    ap.add_argument("--resample_audio", action="store_true", help="bring the file to 16 kHz mono on the device first (audio.Resampler)")
    a = ap.parse_args(argv)
    with open(a.words) as f:
        words = json.load(f)
    wave = audio.Resampler().load([a.audio])[0] if a.resample_audio else audio.read_wav_16k(a.audio)
    rows = ProminenceEstimator().run([wave], [words], boundaries=True)[0]
    write_prom(a.out, os.path.splitext(os.path.basename(a.audio))[0] if a.basename is None else a.basename, rows)
    return rows


if __name__ == "__main__":
    main()
