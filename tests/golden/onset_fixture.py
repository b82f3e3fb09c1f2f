"""Float64 restatement of librosa.onset.onset_detect(y, sr=16000, hop_length=512, units="time") with the library's defaults, and
the seeded synthetic clips the onset tests use.  numpy / scipy only; nothing here reads the product package.

    STFT      n_fft 2048, hop 512, centred with 1024 zeros at both ends, periodic Hann, frames = 1 + len // 512, power |X|^2
    mel       128 Slaney filters over 0 .. 8000 Hz (130 equally spaced mel points, triangles scaled by 2 / (f[i+2] - f[i]))
    dB        10 log10(max(1e-10, mel)), clamped from below at the clip's maximum - 80
    envelope  flux = mean over the bands of max(0, dB[:, t] - dB[:, t-1]); the vector of the frames - 1 differences is padded
              with 3 zeros in front (lag 1 + n_fft // (2 hop) = 2) and cut to `frames`: env[t] = flux between frames t-3 and t-2
    pick      all zero -> nothing; x = env - min, x /= max + tiny; avg[n] = mean(x[max(n-3, 0) : min(n+4, N)]);
              frame n is an onset when x[n] > 0 and x[n] >= avg[n] + 0.07 (pre_max 0, post_max 1, wait 0: nothing else thins)
    times     n * 512 / 16000
"""
import numpy as np
import scipy.fft
import scipy.ndimage

SR = 16000
N_FFT = 2048
HOP = 512
N_MELS = 128
N_BINS = N_FFT // 2 + 1
FMAX = 8000.0
TOP_DB = 80.0
AMIN = 1e-10
LAG_FRAMES = 1 + N_FFT // (2 * HOP)      # 3
PRE_AVG, POST_AVG = 3, 4
DELTA = 0.07
TINY = float(np.finfo(np.float32).tiny)

MIN_MARGIN = 5e-3                        # every fixture clip keeps |x - (avg + delta)| above this at every frame ...
MIN_ONSETS = 5                           # ... and has at least this many onsets
FIXTURE_LEN = 152533                     # 298 onset frames: a 300-frame clip after the evaluation cuts
FIXTURE_SEEDS = (6, 10)                  # margins 1.2e-2 and 1.3e-2, 22 and 29 onsets (test_onsets_cpu.py asserts the conditions)
# lengths of the envelope-parity test: one frame, both sides of a hop, both sides of the window, a few frames, the workload
PARITY_LENS = (1, 511, 512, 2047, 2048, 2049, 5 * 512 + 17, FIXTURE_LEN)


def hz_to_mel(f):
    f = np.asarray(f, np.float64)
    lin = f / (200.0 / 3)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), lin)


def mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), m * (200.0 / 3))


def mel_filterbank():
    """[128, 1025] float64."""
    f = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(FMAX), N_MELS + 2))
    bins = np.linspace(0.0, SR / 2.0, N_BINS)
    w = np.zeros((N_MELS, N_BINS))
    for i in range(N_MELS):
        lower = (bins - f[i]) / (f[i + 1] - f[i])
        upper = (f[i + 2] - bins) / (f[i + 2] - f[i + 1])
        w[i] = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (f[i + 2] - f[i]))
    return w


def mel_centres():
    return mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(FMAX), N_MELS + 2))[1:-1]


_MEL = None


def n_frames(n_samples):
    return 1 + n_samples // HOP


def power_frames(y):
    """[frames, 1025] float64."""
    y = np.asarray(y, np.float64).reshape(-1)
    frames = n_frames(y.shape[0])
    pad = np.concatenate([np.zeros(N_FFT // 2), y, np.zeros(N_FFT // 2)])
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)
    idx = np.arange(frames)[:, None] * HOP + np.arange(N_FFT)[None, :]
    seg = np.where(idx < pad.shape[0], pad[np.minimum(idx, pad.shape[0] - 1)], 0.0)
    return np.abs(scipy.fft.rfft(seg * win, axis=1)) ** 2


def mel_db(y, clamp=True):
    """[frames, 128] float64 dB, clamped at the clip's maximum - 80 unless clamp=False."""
    global _MEL
    if _MEL is None:
        _MEL = mel_filterbank()
    db = 10.0 * np.log10(np.maximum(AMIN, power_frames(y) @ _MEL.T))
    return np.maximum(db, db.max() - TOP_DB) if clamp else db


def envelope(db):
    frames = db.shape[0]
    flux = np.maximum(0.0, db[1:] - db[:-1]).mean(axis=1)
    return np.concatenate([np.zeros(LAG_FRAMES), flux])[:frames]


def moving_mean(x):
    """scipy's centred 7-frame mean with repeated edges, then the ends replaced by the mean over the samples that exist."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    avg = scipy.ndimage.uniform_filter1d(x, PRE_AVG + POST_AVG, mode="nearest", origin=0)
    for i in range(min(PRE_AVG, n)):
        avg[i] = np.mean(x[:i + POST_AVG])
    for i in range(max(n - POST_AVG + 1, 0), n):
        avg[i] = np.mean(x[max(i - PRE_AVG, 0):])
    return avg


def pick(env):
    """-> (onset frames, x, avg); x and avg are zero when the envelope is."""
    env = np.asarray(env, np.float64)
    if not env.any():
        return np.zeros(0, np.int64), np.zeros_like(env), np.zeros_like(env)
    x = env - env.min()
    x = x / (x.max() + TINY)
    avg = moving_mean(x)
    return np.nonzero((x > 0) & (x >= avg + DELTA))[0].astype(np.int64), x, avg


def detect(y, clamp=True):
    """dict(frames = onset frame indices, times, x, avg, margin = min |x - (avg + delta)|, db)."""
    db = mel_db(y, clamp)
    frames, x, avg = pick(envelope(db))
    return dict(frames=frames, times=frames * HOP / SR, x=x, avg=avg, margin=float(np.abs(x - (avg + DELTA)).min()), db=db)


def quantise(y):
    """Through PCM16 and back, as a WAV file stores it."""
    return (np.clip(np.round(np.asarray(y, np.float64) * 32768.0), -32768, 32767) / 32768.0).astype(np.float32)


def burst_clip(seed, n_samples=FIXTURE_LEN, gain=1.0):
    """Decaying tone bursts (150 .. 3000 Hz, 50 .. 300 ms, amplitudes 0.1 .. 0.8) over a 1e-3 Gaussian floor, as PCM16 values."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal(n_samples) * 1e-3
    n_bursts = max(1, int(round(n_samples / SR * 2.5)))
    for _ in range(n_bursts):
        start = int(rng.integers(0, max(1, n_samples - 1)))
        dur = int(rng.uniform(0.05, 0.3) * SR)
        t = np.arange(min(dur, n_samples - start)) / SR
        f, a = rng.uniform(150.0, 3000.0), rng.uniform(0.1, 0.8)
        y[start:start + t.shape[0]] += a * np.exp(-t / (dur / SR / 4.0)) * np.sin(2.0 * np.pi * f * t)
    return quantise(np.clip(y * gain, -1.0, 1.0))


_CACHE = {}


def fixture_clip(seed):
    """(waveform float32, detect(waveform)) of a fixture seed, computed once."""
    if seed not in _CACHE:
        y = burst_clip(seed)
        _CACHE[seed] = (y, detect(y))
    return _CACHE[seed]


def parity_clip(n_samples):
    """The envelope-parity clip of a length (seeded by the length), computed once."""
    key = ("parity", n_samples)
    if key not in _CACHE:
        y = fixture_clip(FIXTURE_SEEDS[0])[0] if n_samples == FIXTURE_LEN else burst_clip(1000 + n_samples, n_samples)
        _CACHE[key] = (y, detect(y))
    return _CACHE[key]


def clamp_clip():
    """A loud burst, then a floor more than 80 dB below it: 0.25 s of a 0.9 tone over 0.75 s of 2e-6 noise (float samples, not quantised)."""
    key = "clamp"
    if key not in _CACHE:
        rng = np.random.default_rng(99)
        n = SR
        y = rng.standard_normal(n) * 2e-6
        t = np.arange(n // 4) / SR
        y[:n // 4] += 0.9 * np.sin(2.0 * np.pi * 440.0 * t)
        y = y.astype(np.float32)
        _CACHE[key] = (y, detect(y), detect(y, clamp=False))
    return _CACHE[key]
