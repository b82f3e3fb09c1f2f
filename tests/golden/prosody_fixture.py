"""Float64 restatement (numpy) of the word-prominence estimator of rag-gesture_amd/prosody.py -- the arithmetic stated in
include/rg_gesture.h under "word prosodic prominence" -- and a deterministic synthetic-speech generator for its tests.

Nothing here comes from the tool that wrote BEAT-X's .prom files; parity with it is not pinned (prosody.py says why).

Stage 1 margins.  Exact equality of the device's lag with the restatement's is a sound demand only where the biased score's best
lag leads every other lag by more than both sides' rounding error: `frames` reports per frame
  lag_margin     the best biased score minus the best one more than one lag away,
  adj_margin     the best biased score minus the better neighbouring lag's,
  voicing_margin |nccf - 0.5|.
FIXTURE_SEEDS and PARITY_LENS are chosen so that every voiced frame has lag_margin >= MIN_LAG_MARGIN.  Adjacent lags DO tie at
half-integer periods (a gliding f0 crosses them; no choice of seeds avoids that), so frames with adj_margin < ADJ_MARGIN are left
out of the lag / logf0 comparison, at most MAX_LEFT_OUT of a clip's voiced frames.
"""
import math

import numpy as np

SR = 16000
HOP, WIN, LAG_MIN, LAG_MAX, SCALES, TILE = 160, 1024, 40, 266, 10, 256
NPROD = WIN - LAG_MAX - 1
FRAME_RATE = 100
MIN_LAG_MARGIN = 1e-3
ADJ_MARGIN = 1e-4
MAX_LEFT_OUT = 0.05
WEIGHTS = (1.0, 1.0, 0.5)
WORD_PAD = 0.03
FIXTURE_SEEDS = (0, 1, 2)
PARITY_LENS = (1, 159, 160, 161, 1023, 1024, 1025, 48000, 86400)
SCALE_FRAMES = [2.0 * 2.0 ** (j / 2.0) for j in range(SCALES)]
RADII = [int(math.ceil(5.0 * s)) for s in SCALE_FRAMES]
REACH = [int(math.ceil(s)) for s in SCALE_FRAMES]


# ------------------------------------------------------------------------------------------------------------ synthetic speech
def speech_clip(seed, n_samples, emphasis=None):
    """A run of words with silent gaps -> (y float32 [n_samples], words [[[start, end], word], ...]).  A word is five harmonics
    with amplitudes 1 / k^1.5 over an f0 that glides linearly between two values in 90 .. 240 Hz, under a sin^0.5 amplitude arc;
    1e-3 white noise lies over the whole clip.  The first word starts at 20 ms (the short clips hold speech too); a word the clip's
    end cuts ends with the clip.  The timings are a forced aligner's rather than the synthesiser's: a word's span takes WORD_PAD =
    30 ms of the silence on either side (gaps are at least 60 ms, so spans never overlap), because the frames that first and
    last hear a word -- where the finest scale has its maxima -- stand up to half an analysis window outside it.  emphasis = k:
    word k is 2.5 times louder, half an octave higher and 1.8 times longer than it would have been."""
    rng = np.random.RandomState(seed)
    y = np.zeros(n_samples, np.float64)
    words, t0, k = [], 0.02, 0
    while int(round(t0 * SR)) < n_samples:
        dur, gap = rng.uniform(0.25, 0.55), rng.uniform(0.06, 0.2)
        fa, fb = rng.uniform(90.0, 240.0), rng.uniform(90.0, 240.0)
        amp = rng.uniform(0.15, 0.3)
        if emphasis is not None:
            fa, fb, amp = 110.0 + 20.0 * rng.uniform(), 110.0 + 20.0 * rng.uniform(), 0.2
            dur = 0.3
            if k == emphasis:
                fa, fb, amp, dur = fa * 1.5, fb * 1.5, amp * 2.5, dur * 1.8
        a, m = int(round(t0 * SR)), int(round(dur * SR))
        u = (np.arange(m, dtype=np.float64) + 0.5) / m
        f0 = fa + (fb - fa) * u
        phase = 2.0 * np.pi * np.cumsum(f0) / SR
        tone = sum(np.sin(h * phase) / h ** 1.5 for h in range(1, 6))
        seg = amp * np.sin(np.pi * u) ** 0.5 * tone
        b = min(a + m, n_samples)
        y[a:b] += seg[:b - a]
        words.append([[max(a / SR - WORD_PAD, 0.0), min(b / SR + WORD_PAD, n_samples / SR)], "w%d" % k])
        t0, k = t0 + dur + gap, k + 1
    y += 1e-3 * rng.standard_normal(n_samples)
    return y.astype(np.float32), words


def fixture_clip(seed):
    """3 s of synthetic speech."""
    return speech_clip(seed, 48000)


def parity_clip(n):
    """The clip of n samples of the GPU parity test.  The seeds are chosen as FIXTURE_SEEDS are (module docstring); with 105 no
    voiced frame of the 1023 .. 1025-sample clips has adjacent lags that all but tie."""
    return speech_clip({48000: 182, 86400: 170}.get(n, 105), n)


def emphasis_clip(seed=7, word=3, n_samples=40000):
    """Words alike but for `word`, which is louder, higher and longer."""
    return speech_clip(seed, n_samples, emphasis=word)


def n_frames(n_samples):
    return 1 + int(n_samples) // HOP


# ------------------------------------------------------------------------------------------------------------ word frames
def first_frame_at(seconds):
    """The first frame t with t / 100 >= seconds."""
    k = max(int(math.ceil(seconds * FRAME_RATE)), 0)
    while k > 0 and (k - 1) / FRAME_RATE >= seconds:
        k -= 1
    while k / FRAME_RATE < seconds:
        k += 1
    return k


def word_frames(words, T):
    """[[[start, end], word], ...] -> (start_frame, end_frame): the frames whose time t / 100 lies in [start, end), the first frame
    clamped to the previous word's end frame, all inside [0, T]."""
    start, end, prev = [], [], 0
    for seg in words:
        a = min(max(first_frame_at(float(seg[0][0])), prev), T)
        b = min(max(first_frame_at(float(seg[0][1])), a), T)
        start.append(a)
        end.append(b)
        prev = b
    return np.asarray(start, np.int64), np.asarray(end, np.int64)


# ------------------------------------------------------------------------------------------------------------ stage 1
def frames(y):
    """-> dict over the T = 1 + n // 160 frames: energy, nccf, logf0 float64, lag int64, the three margins, and voiced (the
    float64 values put through stage 2's rule)."""
    y = np.asarray(y, np.float64)
    T = n_frames(y.size)
    pad = np.zeros(WIN // 2 + (T - 1) * HOP + WIN // 2, np.float64)
    pad[WIN // 2:WIN // 2 + y.size] = y
    lags = np.arange(LAG_MIN - 1, LAG_MAX + 2)
    cand = slice(1, lags.size - 1)
    bias = 0.05 * lags / LAG_MAX
    out = {k: np.zeros(T) for k in ("energy", "nccf", "logf0", "lag_margin", "adj_margin", "voicing_margin")}
    out["lag"] = np.zeros(T, np.int64)
    for t in range(T):
        x = pad[t * HOP:t * HOP + WIN]
        out["energy"][t] = math.log(np.dot(x, x) / WIN + 1e-10)
        a = x[:NPROD]
        B = np.lib.stride_tricks.sliding_window_view(x, NPROD)[lags]
        r = (B @ a) / np.sqrt(np.dot(a, a) * np.einsum("ij,ij->i", B, B) + 1e-20)
        score = (r - bias)[cand]
        k = int(np.argmax(score))                                    # (the first maximum: the smallest lag)
        far = np.ones(score.size, bool)
        far[max(k - 1, 0):k + 2] = False
        near = [score[j] for j in (k - 1, k + 1) if 0 <= j < score.size]
        out["lag_margin"][t] = score[k] - score[far].max()
        out["adj_margin"][t] = score[k] - max(near)
        i = k + 1                                                    # index into lags / r
        d = r[i - 1] - 2.0 * r[i] + r[i + 1]
        delta = 0.0 if d == 0.0 else min(max(0.5 * (r[i - 1] - r[i + 1]) / d, -0.5), 0.5)
        out["nccf"][t], out["lag"][t] = r[i], lags[i]
        out["logf0"][t] = math.log(16000.0 / (lags[i] + delta))
        out["voicing_margin"][t] = abs(r[i] - 0.5)
    out["voiced"] = voicing(out["energy"], out["nccf"])[0]
    return out


def voicing(energy, nccf):
    """Stage 2's rule, its comparisons made in float32 exactly as the kernel makes them -> (voiced bool, clamped energy float32)."""
    e32, n32 = np.asarray(energy).astype(np.float32), np.asarray(nccf).astype(np.float32)
    floor = np.float32(e32.max() - np.float32(11.5))
    return (n32 >= np.float32(0.5)) & (e32 >= floor), np.maximum(e32, floor)


# ------------------------------------------------------------------------------------------------------------ stage 2
def fill(values, knots):
    """Linear between knots, flat outside, zeros without knots (float64)."""
    values, idx = np.asarray(values, np.float64), np.nonzero(knots)[0]
    if idx.size == 0:
        return np.zeros(values.size)
    return np.interp(np.arange(values.size), idx, values[idx])


def znorm(v):
    v = np.asarray(v, np.float64)
    return (v - v.mean()) / max(v.std(), 1e-6)


def signal(energy, nccf, logf0, start_frame, end_frame, word_start, word_end, weights=WEIGHTS):
    """-> dict: voiced, f0 (filled), f0z, ez, dz, c, status."""
    T = len(energy)
    voiced, clamped = voicing(energy, nccf)
    f0 = fill(np.asarray(logf0, np.float64), voiced)
    knots, dur = np.zeros(T, bool), np.zeros(T)
    for a, b, s, e in zip(start_frame, end_frame, word_start, word_end):
        if a < b:
            mid = (int(a) + int(b) - 1) // 2
            knots[mid] = True
            dur[mid] = math.log(float(max(np.float32(e) - np.float32(s), np.float32(0.01))))
    dz = znorm(fill(dur, knots))
    f0z, ez = znorm(f0), znorm(clamped.astype(np.float64))
    return dict(voiced=voiced, f0=f0, f0z=f0z, ez=ez, dz=dz, c=weights[0] * f0z + weights[1] * ez + weights[2] * dz,
                status=0 if voiced.any() else 1)


# ------------------------------------------------------------------------------------------------------------ stage 3
def taps(j):
    s, R = SCALE_FRAMES[j], RADII[j]
    u = np.arange(-R, R + 1, dtype=np.float64) / s
    return (1.0 - u * u) * np.exp(-0.5 * u * u) / math.sqrt(s)


def cwt(c):
    """-> W [SCALES, T] float64: W[j][t] = sum over k of c[t + k] psi_j[k], c zero outside."""
    c = np.asarray(c, np.float64)
    return np.stack([np.correlate(np.pad(c, RADII[j]), taps(j), mode="valid") for j in range(SCALES)])


# ------------------------------------------------------------------------------------------------------------ stage 4
def _is_point(w, q):
    left = w[q - 1] if q > 0 else -np.inf
    right = w[q + 1] if q + 1 < w.size else -np.inf
    return w[q] > 0 and w[q] > left and w[q] >= right


def line_strengths(W):
    """-> [T] float64: the strength of the peak line that starts at every frame, 0 where none does.  Valleys: line_strengths(-W)."""
    W = np.asarray(W, np.float64)
    T = W.shape[1]
    out = np.zeros(T)
    for p in range(T):
        if not _is_point(W[0], p):
            continue
        strength, pos = W[0][p], p
        for j in range(1, SCALES):
            found = None
            for d in range(REACH[j] + 1):
                for q in ((pos - d,) if d == 0 else (pos - d, pos + d)):
                    if 0 <= q < T and _is_point(W[j], q):
                        found = q
                        break
                if found is not None:
                    break
            if found is None:
                break
            strength, pos = strength + W[j][found], found
        out[p] = strength
    return out


def _best(v, a, b):
    if a >= b or not (v[a:b] > 0).any():
        return 0.0, -1
    k = a + int(np.argmax(v[a:b]))                                   # (the first maximum: the lowest frame)
    return float(v[k]), k


def word_values(peak, valley, start_frame, end_frame):
    """-> dict: prominence, boundary float64 and prom_frame, bnd_frame int64 per word."""
    T, n = len(peak), len(start_frame)
    out = dict(prominence=np.zeros(n), boundary=np.zeros(n), prom_frame=np.full(n, -1, np.int64), bnd_frame=np.full(n, -1, np.int64))
    have = [w for w in range(n) if start_frame[w] < end_frame[w]]
    mid = {w: (int(start_frame[w]) + int(end_frame[w]) - 1) // 2 for w in have}
    for i, w in enumerate(have):
        out["prominence"][w], out["prom_frame"][w] = _best(peak, int(start_frame[w]), int(end_frame[w]))
        out["boundary"][w], out["bnd_frame"][w] = _best(valley, mid[w], mid[have[i + 1]] if i + 1 < len(have) else T)
    return out


def words_stage(W, start_frame, end_frame):
    peak, valley = line_strengths(W), line_strengths(-np.asarray(W, np.float64))
    out = word_values(peak, valley, start_frame, end_frame)
    out.update(peak_strength=peak, valley_strength=valley)
    return out


# ------------------------------------------------------------------------------------------------------------ the whole chain
def estimate(y, words, weights=WEIGHTS):
    """The four stages in float64 -> dict with every stage's outputs; rows = [(word, start, end, prominence, boundary), ...]."""
    fr = frames(y)
    T = fr["energy"].size
    sf, ef = word_frames(words, T)
    sg = signal(fr["energy"], fr["nccf"], fr["logf0"], sf, ef, [w[0][0] for w in words], [w[0][1] for w in words], weights)
    W = cwt(sg["c"])
    wd = words_stage(W, sf, ef)
    rows = [(w[1], float(w[0][0]), float(w[0][1]), float(wd["prominence"][i]), float(wd["boundary"][i])) for i, w in enumerate(words)]
    return dict(frames=fr, signal=sg, W=W, words=wd, start_frame=sf, end_frame=ef, rows=rows)


def left_out(fr):
    """Voiced frames whose adjacent lags all but tie: kept out of the lag / logf0 comparison."""
    return fr["voiced"] & (fr["adj_margin"] < ADJ_MARGIN)
