"""GPU: recorded audio to 16 kHz mono on the device (rg_resample_poly through audio.Resampler) against scipy.signal.resample_poly
in float64 on the decoded, downmixed input.

Error bound, per output, derived and not measured.  The device adds up taps products coeff_j x_j in fp32, one after the other.
Against the float64 sum of the same terms: coeff_j is h rounded once to fp32 (relative 2^-24), x_j is the decoded mean of the
channels in fp32 (int32 -> fp32, the channel sum and the multiply by 1 / channels: at most three roundings, none for 16- and
24-bit mono), and a serial sum of n terms, fused or not, is off by at most n 2^-24 sum |terms| to first order (Higham, Accuracy
and Stability of Numerical Algorithms, section 3.1).  Together at most (taps + 4) 2^-24 sum_j |coeff_j| |x_j|; the bound used
is (taps + 2) 2^-23 sum_j |coeff_j| |x_j| + 1e-30, twice that and more.
"""
import importlib
import importlib.util
import math
import os
import wave

import numpy as np
import pytest
import scipy.signal
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RATES = (48000, 44100, 22050, 8000)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fx, jf, fgdfx = _load("onset_fixture"), _load("joint_fixture"), _load("fgd_fixture")


@pytest.fixture(scope="module")
def rg():
    return importlib.import_module("rag-gesture_amd")


@pytest.fixture(scope="module")
def audio(rg):
    return rg.audio


@pytest.fixture(scope="module")
def res(audio):
    return audio.Resampler()


def _direct(x, up, down, half_len, h, at):
    """sum over k of h[m down - k up + half_len] x[k] for the outputs m in `at`, in float64, term by term."""
    taps = 2 * half_len // up + 1
    hp = np.zeros(up * taps, np.float64)
    hp[:h.size] = h
    c = np.asarray(at, np.int64) * down + half_len
    p, k_hi = c % up, c // up
    y = np.zeros(c.size, np.float64)
    for j in range(taps):
        k = k_hi - j
        ok = (k >= 0) & (k < x.size)
        y[ok] += hp[p[ok] + j * up] * x[k[ok]]
    return y


def _check(audio, got, frames, rate, parity=None, name=None):
    """One clip's device result against resample_poly in float64 on its decoded mean, output by output."""
    x = audio.decode_mono(frames)
    up, down, half_len, h = audio.resample_filter(rate)
    taps = 2 * half_len // up + 1
    n_out = math.ceil(x.size * up / down)
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == (n_out,)
    if n_out == 0:
        return 0.0
    ref = scipy.signal.resample_poly(x, up, down, window=h / up)
    bound = (taps + 2) * 2.0 ** -23 * _direct(np.abs(x), up, down, half_len, np.abs(h), np.arange(n_out)) + 1e-30
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    worst = float((err / bound).max())
    print("%s %5d Hz, %6d frames -> %6d: worst |y - ref| %.3e, worst error / bound %.4f" % (name or "", rate, x.size, n_out, err.max(), worst))
    assert (err <= bound).all(), (rate, x.size, worst)
    return worst


# ------------------------------------------------------------------------------------------ 1. rates x lengths
@pytest.mark.parametrize("rate", RATES)
def test_rates_and_lengths(audio, res, rate):
    """Clips shorter than the filter, n up % down zero and not, a tile boundary inside the clip (4097 frames give more than 1024
    outputs at every rate); each length alone and all of them in one launch, bit for bit the same."""
    up, down, half_len, h = audio.resample_filter(rate)
    taps = 2 * half_len // up + 1
    lens = (0, 1, 2, taps // 2, 1000, 4097)
    assert any(n * up % down for n in lens) == (down > 1) and math.ceil(4097 * up / down) > audio.RESAMPLE_TILE
    rng = np.random.default_rng(rate)
    clips = [rng.uniform(-1, 1, n).astype(np.float32) for n in lens]
    together = res.run([(c, rate) for c in clips])
    worst = 0.0
    for c, y in zip(clips, together):
        alone, = res.run([(c, rate)])
        assert torch.equal(alone, y), (rate, c.size)
        worst = max(worst, _check(audio, y, c, rate))
    assert 0.0 < worst <= 1.0


# ------------------------------------------------------------------------------------------ 2. clip isolation
def test_a_silent_clip_between_loud_ones_stays_silent(audio, res):
    rng = np.random.default_rng(7)
    loud = [(1e3 * rng.standard_normal(n)).astype(np.float32) for n in (2500, 1800)]
    y = res.run([(loud[0], 44100), (np.zeros(3000, np.float32), 44100), (loud[1], 44100)])
    assert y[1].shape == (math.ceil(3000 * 160 / 441),) == (1089,)
    assert not y[1].any() and bool((y[1] == 0.0).all())
    assert float(y[0].abs().max()) > 100.0 and float(y[2].abs().max()) > 100.0
    for c, got in zip(loud, (y[0], y[2])):
        _check(audio, got, c, 44100)


# ------------------------------------------------------------------------------------------ 3. formats and downmix
def _bytes24(v):
    return np.stack([(v >> s) & 255 for s in (0, 8, 16)], axis=-1).astype(np.uint8)


def test_formats_and_downmix(audio, res):
    rng = np.random.default_rng(11)
    s = rng.uniform(-1, 1, (2000, 2))
    s[:2] = ((-1.0, -1.0), (1.0, 1.0))                                           # both ends of every integer range
    stored = {audio.PCM16: np.clip(np.round(s * 2 ** 15), -2 ** 15, 2 ** 15 - 1).astype(np.int16),
              audio.PCM24: _bytes24(np.clip(np.round(s * 2 ** 23), -2 ** 23, 2 ** 23 - 1).astype(np.int32)),
              audio.PCM32: np.clip(np.round(s * 2 ** 31), -2 ** 31, 2 ** 31 - 1).astype(np.int64).astype(np.int32),
              audio.F32: s.astype(np.float32)}
    got = res.run([(a, 48000) for a in stored.values()])                         # four groups: a launch each
    for (fmt, a), y in zip(stored.items(), got):
        x = audio.decode_mono(a)
        assert np.abs(x - s.mean(axis=1)).max() <= 2.0 ** -15 and x[0] == -1.0
        _check(audio, y, a, 48000, name=audio.FORMAT_NAMES[fmt])
    # [a, a] stereo is mono a, bit for bit; so is [n, 1] and the packed mono layout [n, 3]
    a = stored[audio.PCM16][:, 0].copy()
    mono, twin, col = res.run([(a, 48000), (np.stack([a, a], axis=1), 48000), (a[:, None], 48000)])
    assert torch.equal(mono, twin) and torch.equal(mono, col) and bool(mono.any())
    b = stored[audio.PCM24][:, 0].copy()
    m24, c24 = res.run([(b, 48000), (b[:, None, :], 48000)])
    assert m24.shape == mono.shape and torch.equal(m24, c24)
    _check(audio, m24, b, 48000, name="pcm24 mono")


# ------------------------------------------------------------------------------------------ 4. the target rate
def test_target_rate_is_a_copy_with_the_downmix(audio):
    res = audio.Resampler()
    rng = np.random.default_rng(13)
    lr = rng.integers(-32768, 32768, (3001, 2)).astype(np.int16)
    lr[:2] = ((-32768, -32768), (32767, 32767))
    y, = res.run([(lr, 16000)])
    want = (lr[:, 0].astype(np.float32) + lr[:, 1].astype(np.float32)) * np.float32(0.5) / np.float32(32768.0)
    assert np.array_equal(want.astype(np.float64), (lr[:, 0].astype(np.float64) + lr[:, 1]) * 0.5 / 32768)      # (exact in fp32)
    assert y.shape == (3001,) and np.array_equal(y.cpu().numpy(), want)
    assert res.tables == {}                                                      # no filter was built
    f = rng.uniform(-1, 1, 700).astype(np.float32)
    assert np.array_equal(res.run([(f, 16000)])[0].cpu().numpy(), f) and res.tables == {}
    with pytest.raises(ValueError, match="no clips"):
        res.run([])
    with pytest.raises(ValueError, match="16001 Hz"):
        res.run([(f, 16001)])
    with pytest.raises(ValueError, match="clip 1"):
        res.run([(f, 48000), (f.astype(np.float64), 48000)])


# ------------------------------------------------------------------------------------------ 5. 64-bit indexing
def test_five_minutes_at_44100(audio, res):
    """13 600 000 frames at 44.1 kHz: m down passes 2^31 at output 4 869 577 and k up with it."""
    n, up, down = 13_600_000, 160, 441
    a = np.random.default_rng(17).integers(-32768, 32768, n).astype(np.int16)
    y, = res.run([(a, 44100)])
    n_out = 4_934_241
    assert y.shape == (n_out,) == (math.ceil(n * up / down),)
    edge = 4_869_576
    assert edge * down < 2 ** 31 < (edge + 2) * down and (n - 1) * up > 2 ** 31
    at = np.concatenate([np.arange(edge - 256, edge + 256), np.arange(n_out - 512, n_out)])
    _, _, half_len, h = audio.resample_filter(44100)
    x = audio.decode_mono(a)
    ref = _direct(x, up, down, half_len, h, at)
    bound = (177 + 2) * 2.0 ** -23 * _direct(np.abs(x), up, down, half_len, np.abs(h), at) + 1e-30
    err = np.abs(y[torch.from_numpy(at).to(y.device)].cpu().numpy().astype(np.float64) - ref)
    print("outputs around 2^31 / 441 and the last 512: worst |y - ref| %.3e, worst error / bound %.4f" % (err.max(), (err / bound).max()))
    assert np.abs(ref).max() > 0.1 and (err <= bound).all()


# ------------------------------------------------------------------------------------------ 6. grouping
def test_mixed_list_comes_back_in_input_order(audio, res):
    rng = np.random.default_rng(19)
    clips = [(rng.integers(-32768, 32768, 1500).astype(np.int16), 48000),
             (rng.integers(-32768, 32768, (1700, 2)).astype(np.int16), 44100),
             (rng.integers(-32768, 32768, 900).astype(np.int16), 16000),
             (rng.integers(-32768, 32768, 2100).astype(np.int16), 48000),
             (np.zeros(0, np.int16), 48000)]
    got = res.run(clips)
    assert [tuple(y.shape) for y in got] == [(500,), (617,), (900,), (700,), (0,)]
    for (frames, rate), y in zip(clips, got):
        assert torch.equal(res.run([(frames, rate)])[0], y)
        if rate != 16000:
            _check(audio, y, frames, rate)
    assert np.array_equal(got[2].cpu().numpy(), clips[2][0].astype(np.float32) / np.float32(32768.0))
    assert {44100, 48000} <= set(res.tables) and 16000 not in res.tables          # one table per rate, none for a copy


def test_load_reads_files(audio, res, tmp_path):
    rng = np.random.default_rng(23)
    a = rng.integers(-32768, 32768, (2205, 2)).astype(np.int16)
    b = rng.integers(-32768, 32768, 1600).astype(np.int16)
    _write_pcm16(tmp_path / "a.wav", a, 44100)
    _write_pcm16(tmp_path / "b.wav", b, 16000)
    ya, yb = audio.load_16k([tmp_path / "a.wav", tmp_path / "b.wav"], res)
    assert torch.equal(ya, res.run([(a, 44100)])[0]) and ya.shape == (800,)
    assert np.array_equal(yb.cpu().numpy(), audio.read_wav_16k(tmp_path / "b.wav"))


# ------------------------------------------------------------------------------------------ 7. wiring
def _write_pcm16(path, a, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if a.ndim == 1 else a.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(a).tobytes())


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "joint_metrics.npz"))


@pytest.fixture(scope="module")
def inp(gold):
    return jf.inputs(int(gold["seed"]))


def _stereo_44100(impulses):
    """The fixture's impulses at their 44.1 kHz positions, louder on the left channel."""
    s = np.zeros((int(44100 / 30 * jf.N_FRAMES), 2), np.int16)
    pos = np.round(impulses * 44100 / 16000).astype(np.int64)
    s[pos, 0], s[pos, 1] = 32767, 16000
    return s


@pytest.fixture(scope="module")
def folder(tmp_path_factory, rg, inp, gold):
    root = tmp_path_factory.mktemp("resample")
    names = jf.write_folder(str(root / "eval"), inp, rg.packing.save_sample_files)
    for name, imp in zip(names, inp["impulses"]):
        _write_pcm16(root / "eval" / name / "gt_audio.wav", _stereo_44100(imp), 44100)
    sd = fgdfx.state_dict(np.load(os.path.join(HERE, "golden", "fgd_eval.npz")))
    torch.save({"model_state": {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}}, str(root / "ckpt.bin"))
    return root


def test_evaluate_folder_resamples_on_request(rg, audio, folder, gold, inp):
    ev = rg.evaluation
    names = jf.clip_names()
    enc = ev.FGDEncoder(str(folder / "ckpt.bin"))
    sm = ev.SMPLXJoints(jf.smplx_model())
    args = dict(eval_n=jf.EVAL_N, smplx=sm, avg_vel=gold["avg_vel"], onsets="device")
    with pytest.raises(ValueError, match=r"gt_audio\.wav.*44100 Hz, 2 channel.*must be 16 kHz mono"):
        ev.evaluate_folder(str(folder / "eval"), enc, **args)
    used, t = {}, {}
    r = ev.evaluate_folder(str(folder / "eval"), enc, resample_audio=True, onsets_out=used, timings=t, **args)
    assert sorted(used) == sorted(names) and all(used[k].size >= 1 for k in names)
    assert "align_skipped" not in r and r["align"] > 0 and r["gt_align"] > 0 and 0 < t["onsets"] <= t["device"]
    # the float64 restatement of both steps on the same files; every clip keeps the onset fixtures' margin, so the frames are the same
    for name, imp in zip(names, inp["impulses"]):
        cut = audio.cut_to_clip(audio.Resampler.reference(_stereo_44100(imp), 44100), jf.EVAL_N)
        d = fx.detect(cut.astype(np.float32))
        assert cut.size == 23467 and d["margin"] >= fx.MIN_MARGIN and d["frames"].size >= 1, name
        assert np.array_equal(used[name], d["times"]), name
    r2 = ev.evaluate_folder(str(folder / "eval"), enc, resample_audio=True, batch_clips=4, **args)
    assert r2["align"] == pytest.approx(r["align"], rel=1e-13) and r2["gt_align"] == pytest.approx(r["gt_align"], rel=1e-13)
    pred_file = str(folder / "eval" / names[1] / "pred_motion.npz")
    one = audio.clip_audio(pred_file, jf.EVAL_N, resampler=audio.Resampler())
    assert one.is_cuda and one.shape == (23467,)
    get, why = ev.onset_source("device", resample_audio=True)
    assert why is None and np.array_equal(get(pred_file, jf.EVAL_N), used[names[1]])


def _click_track(rate, amp=0.1, seconds=6.0):
    """Twelve clicks, one every 0.5 s from 0.25 s on (a 1.5 kHz tone that decays in 4 ms), on noise of 1e-3, sampled at `rate`."""
    t = np.arange(int(rate * seconds)) / rate
    y = 1e-3 * np.random.default_rng(rate).standard_normal(t.size)
    for i in range(12):
        d = t - (0.25 + 0.5 * i)
        y[d >= 0] += amp * np.exp(-d[d >= 0] / 0.004) * np.sin(2.0 * np.pi * 1500.0 * d[d >= 0])
    return y.astype(np.float32)


def test_onsets_of_a_resampled_click_track(audio, res):
    """Clicks recorded at 48 kHz and resampled on the device give the onsets of the same clicks synthesised at 16 kHz.  The
    amplitude 0.1 was fixed on the host: the float64 restatements of both signals give the same onset frames, with margins of
    2.3e-2 and 1.7e-2 to the threshold."""
    y48, y16 = _click_track(48000), _click_track(16000)
    d48 = fx.detect(audio.Resampler.reference(y48, 48000).astype(np.float32))
    d16 = fx.detect(y16)
    assert np.array_equal(d48["frames"], d16["frames"]) and min(d48["margin"], d16["margin"]) >= fx.MIN_MARGIN
    assert d16["frames"].size >= 12
    det = audio.OnsetDetector()
    resampled, = res.run([(y48, 48000)])
    assert resampled.shape == (96000,)
    a, b = det.detect([resampled, y16])
    print("onsets (s) of the resampled track:", a.tolist())
    assert a.size == b.size >= 12 and float(np.abs(a - b).max()) <= 512 / 16000
