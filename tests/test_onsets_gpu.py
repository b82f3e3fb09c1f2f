"""GPU: audio onsets on the device (rg_onset_mel_db, rg_onset_pick through audio.OnsetDetector) against the float64 restatement of
librosa's onset_detect defaults in tests/golden/onset_fixture.py: the normalised envelope and its moving mean, the onset frames
(exactly), ragged batches, the -80 dB clamp, degenerate clips, and evaluate_folder(..., onsets="device") / the CLI end to end.

Envelope bound.  Measured on an MI355X over the eight parity lengths: worst |x - x_ref| = 2.096e-07, worst |avg - avg_ref| =
4.389e-08 (NOTEBOOK section 14).  The bounds are those values x 4, rounded up to one significant digit: 9e-7 and 2e-7, both far
under the 5e-4 that a tenth of the fixtures' 5e-3 threshold margin allows, which is what makes exact equality of the onset
frames a sound demand.

Constant DC.  A constant clip is NOT free of onsets under this algorithm: the zero padding of the centred STFT makes the first
two frames (half and three quarters of a window of signal) quieter than the third, the band differences between them are
positive, the envelope has its only peak at frame 3, and x[3] = 1 >= avg[3] + 0.07.  The float64 restatement finds that onset
too, so the degenerate-input test asks for what the restatement gives on DC (and for no NaN), an empty list for silence, and an
empty list for a DC clip of fewer than 4 frames, whose envelope is cut before the peak.
"""
import importlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
X_BOUND = 9e-7
AVG_BOUND = 2e-7


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
def det(rg):
    return rg.audio.OnsetDetector()


def _host(t):
    return t.cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------ 1. envelope parity
def test_envelope_parity(det, parity):
    """All eight lengths in one ragged call: one frame, both sides of a hop and of the window, a few frames, the workload."""
    assert X_BOUND <= 5e-4 and AVG_BOUND <= 5e-4
    clips = [fx.parity_clip(n) for n in fx.PARITY_LENS]
    got = det.envelopes([y for y, _ in clips])
    worst_x = worst_avg = 0.0
    for n, (y, d), (x, avg) in zip(fx.PARITY_LENS, clips, got):
        assert x.shape == avg.shape == (1 + n // 512,) and x.dtype == avg.dtype == torch.float32 and x.is_cuda
        ex, ea = float(np.abs(_host(x) - d["x"]).max()), float(np.abs(_host(avg) - d["avg"]).max())
        print("%6d samples, %3d frames: |x - x_ref| %.3e  |avg - avg_ref| %.3e" % (n, x.shape[0], ex, ea))
        worst_x, worst_avg = max(worst_x, ex), max(worst_avg, ea)
    assert any(d["x"].any() for _, d in clips[3:]) and clips[-1][1]["frames"].size >= fx.MIN_ONSETS
    parity.check("onsets: envelope x vs float64 restatement", worst_x, X_BOUND)
    parity.check("onsets: moving mean avg vs float64 restatement", worst_avg, AVG_BOUND)


# ------------------------------------------------------------------------------------------ 2. onset frames
def test_onset_frames_equal_the_restatement(det):
    ys = [fx.fixture_clip(s)[0] for s in fx.FIXTURE_SEEDS] + [fx.parity_clip(n)[0] for n in fx.PARITY_LENS]
    want = [fx.fixture_clip(s)[1] for s in fx.FIXTURE_SEEDS] + [fx.parity_clip(n)[1] for n in fx.PARITY_LENS]
    for s, d in zip(fx.FIXTURE_SEEDS, want):
        assert d["margin"] >= fx.MIN_MARGIN and d["frames"].size >= fx.MIN_ONSETS, s
    assert all(d["margin"] >= fx.MIN_MARGIN for d in want)                   # (the short parity clips keep the margin too)
    frames, times = det.detect_frames(ys), det.detect(ys)
    for i, d in enumerate(want):
        assert frames[i].dtype == np.int64 and np.array_equal(frames[i], d["frames"]), i
        assert times[i].dtype == np.float64 and np.array_equal(times[i], d["times"]), i
    assert all(np.all(np.diff(f) > 0) for f in frames)


# ------------------------------------------------------------------------------------------ 3. ragged batch
def test_ragged_batch_equals_one_clip_at_a_time(det):
    """Three lengths in one call; the middle clip is 40 dB quieter, so a maximum or a normalisation that leaks across clips moves
    its clamp floor (its quiet bands sit 60 dB under its own maximum, 100 dB under its neighbours') and its envelope."""
    loud_a = fx.burst_clip(21, 40000)
    quiet = (fx.burst_clip(22, 23467).astype(np.float64) * 0.01).astype(np.float32)
    loud_b = fx.burst_clip(23, 9000)
    ys = [loud_a, quiet, loud_b]
    together = det.run(ys)
    off = together["frame_off"]
    assert off.tolist() == [0, 79, 79 + 46, 79 + 46 + 18]
    counts = together["onset_count"].cpu().numpy()
    assert counts.min() >= 1
    for c, y in enumerate(ys):
        alone = det.run([y])
        n = int(counts[c])
        assert int(alone["onset_count"][0]) == n
        for k in ("x", "avg", "db"):
            assert torch.equal(alone[k], together[k][off[c]:off[c + 1]]), (c, k)
        assert torch.equal(alone["onset_frames"][:n], together["onset_frames"][off[c]:off[c] + n]), c
    d = fx.detect(quiet)
    x = together["x"][off[1]:off[2]]
    assert float(np.abs(_host(x) - d["x"]).max()) <= X_BOUND
    # the restatement with its neighbours' maximum as the clamp reference is a different envelope: the comparison above can fail
    db = fx.mel_db(quiet, clamp=False)
    leaked = fx.pick(fx.envelope(np.maximum(db, fx.mel_db(loud_a).max() - fx.TOP_DB)))[1]
    assert np.abs(leaked - d["x"]).max() > 1e-2
    # device tensors and host arrays are the same input
    again = det.run([torch.from_numpy(y).cuda() for y in ys])
    assert all(torch.equal(again[k], together[k]) for k in ("x", "avg", "db", "onset_count"))


# ------------------------------------------------------------------------------------------ 4. the clamp
def test_clamp_against_the_clips_maximum(det):
    """A 0.9 tone, then noise 113 dB below it.  Tolerance per value, from the restatement's own numbers: an fp32 FFT of N = 2048
    points has a relative 2-norm error of at most log2(N) eta, eta = mu + 4 u (sqrt 2 + mu) < 6.4 u for twiddles rounded once
    (mu <= u / sqrt 2, u = 2^-24; Higham, Accuracy and Stability of Numerical Algorithms, theorem 24.2), so no bin of a frame is
    further than E = 11 * 6.4 u ||X||_2 from its exact value, a band sum s = sum w_j |X_j|^2 moves by at most
    ds = sum w_j (2 |X_j| E + E^2), and dB, clamped at the floor's band sum s_floor, by at most 10 log10(1 + ds / max(s, s_floor));
    5e-5 dB on top for the fp32 window, weights, log10f and the subtraction of 80 (values up to 100 dB, a few ulp)."""
    y, d, unclamped = fx.clamp_clip()
    power = fx.power_frames(y)
    mel = fx.mel_filterbank()
    e = 11 * 6.4 * 2.0 ** -24 * np.sqrt(2.0 * power.sum(axis=1))                  # (both halves of the spectrum)
    ds = (2.0 * np.sqrt(power) * e[:, None] + e[:, None] ** 2) @ mel.T
    s = power @ mel.T
    s_floor = 10.0 ** ((d["db"].max() - fx.TOP_DB) / 10.0)
    tol = 10.0 * np.log10(1.0 + ds / np.maximum(s, s_floor)) + 5e-5
    tol = np.maximum(tol, tol.max(where=d["db"] == d["db"].max(), initial=0.0))     # (the floor moves with the maximum)
    db, = det.mel_db([y])
    got = _host(db)
    err = np.abs(got - d["db"])
    print("clamped dB: worst error %.3e dB, worst error / tolerance %.3f, tolerance up to %.3e" % (err.max(), (err / tol).max(), tol.max()))
    assert tol.max() < 2.0 and (err <= tol).all()                                 # (a missing clamp is off by 60 dB)
    floor = np.float32(np.float32(got.max()) - np.float32(80.0))
    assert got.min() == floor and (got == floor).mean() > 0.5                     # most of the clip lies on the floor
    assert unclamped["db"].min() == -100.0 and d["db"].min() > -45.0              # without the clamp: 60 dB further down
    (x, avg), = det.envelopes([y])
    assert float(np.abs(_host(x) - d["x"]).max()) <= X_BOUND and np.abs(unclamped["x"] - d["x"]).max() > 0.5
    assert np.array_equal(det.detect_frames([y])[0], d["frames"]) and d["margin"] >= fx.MIN_MARGIN


# ------------------------------------------------------------------------------------------ 6. degenerate inputs
def test_degenerate_inputs(det):
    silence, dc = np.zeros(16000, np.float32), np.full(16000, 0.5, np.float32)
    dc_short, empty = np.full(1500, 0.5, np.float32), np.zeros(0, np.float32)
    ys = [silence, dc, dc_short, empty]
    env, frames = det.envelopes(ys), det.detect(ys)
    for (x, avg), y in zip(env, ys):
        assert x.shape == (1 + len(y) // 512,) and bool(torch.isfinite(x).all()) and bool(torch.isfinite(avg).all())
    for i in (0, 2, 3):
        assert frames[i].size == 0 and frames[i].dtype == np.float64
        assert not env[i][0].any() and not env[i][1].any()
    want = fx.detect(dc)                                                          # (see the module docstring)
    assert want["frames"].tolist() == [3] and np.array_equal(frames[1], want["times"])
    assert float(np.abs(_host(env[1][0]) - want["x"]).max()) <= X_BOUND
    with pytest.raises(ValueError, match="no clips"):
        det.detect([])
    with pytest.raises(ValueError, match="clip 0 must be a 1-D float waveform"):
        det.detect([np.zeros((2, 100), np.float32)])
    with pytest.raises(ValueError, match="clip 1 must be a 1-D float waveform"):
        det.detect([silence, np.zeros(100, np.int16)])


# ------------------------------------------------------------------------------------------ 5. end to end
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "joint_metrics.npz"))


@pytest.fixture(scope="module")
def inp(gold):
    return jf.inputs(int(gold["seed"]))


@pytest.fixture(scope="module")
def folder(tmp_path_factory, rg, inp, gold):
    root = tmp_path_factory.mktemp("onsets")
    jf.write_folder(str(root / "eval"), inp, rg.packing.save_sample_files)
    np.savez(str(root / "model.npz"), **jf.smplx_model())
    np.save(str(root / "avg_vel.npy"), gold["avg_vel"])
    sd = fgdfx.state_dict(np.load(os.path.join(HERE, "golden", "fgd_eval.npz")))
    torch.save({"model_state": {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}}, str(root / "ckpt.bin"))
    return root


def _restated_onsets(root, names):
    """The restatement on what the tool cuts out of every clip's gt_audio.wav (evaluate.py:396-405)."""
    length, a_off = int(16000 / 30 * jf.EVAL_N), int(10 * (16000 / 30))
    out = {}
    for name in names:
        a = jf.read_wav(os.path.join(root, "eval", name, "gt_audio.wav"))[:length]
        d = fx.detect(a[a_off:len(a) - a_off])
        assert d["margin"] >= fx.MIN_MARGIN and d["frames"].size >= 1, name
        out[name] = d["times"]
    return out


def test_evaluate_folder_with_device_onsets(rg, folder, gold, inp):
    ev = rg.evaluation
    names = jf.clip_names()
    want = _restated_onsets(str(folder), names)
    enc = ev.FGDEncoder(str(folder / "ckpt.bin"))
    sm = ev.SMPLXJoints(jf.smplx_model())
    t, used = {}, {}
    r = ev.evaluate_folder(str(folder / "eval"), enc, eval_n=jf.EVAL_N, smplx=sm, avg_vel=gold["avg_vel"], onsets="device",
                           timings=t, onsets_out=used)
    assert sorted(used) == sorted(names) and all(np.array_equal(used[k], want[k]) for k in names)
    assert "align_skipped" not in r and 0 < t["onsets"] <= t["device"] and t["read"] >= 0
    jm = ev.JointMetrics(sm, avg_vel=gold["avg_vel"], eval_n=jf.EVAL_N)
    n = jf.EVAL_N
    jm.add([p[:n] for p in inp["pred"]], [g[:n] for g in inp["gt"]], betas=inp["betas"], onsets=[want[k] for k in names])
    ref = jm.compute()
    for k in ("align", "gt_align"):
        print("%s %.17g from the restatement's onsets %.17g" % (k, r[k], ref[k]))
        assert r[k] == pytest.approx(ref[k], rel=1e-13, abs=0)                   # (the same onsets: float64 round-off of the sums)
    # the same onsets passed back as a mapping, in two batches of clips, and clip by clip through the getter
    assert ev.evaluate_folder(str(folder / "eval"), enc, eval_n=jf.EVAL_N, smplx=sm, avg_vel=gold["avg_vel"], onsets=used) == r
    r2 = ev.evaluate_folder(str(folder / "eval"), enc, eval_n=jf.EVAL_N, smplx=sm, avg_vel=gold["avg_vel"], onsets="device",
                            batch_clips=4)
    assert r2["align"] == pytest.approx(r["align"], rel=1e-13) and r2["gt_align"] == pytest.approx(r["gt_align"], rel=1e-13)
    get, why = ev.onset_source("device")
    pred_file = str(folder / "eval" / names[1] / "pred_motion.npz")
    assert why is None and np.array_equal(get(pred_file, n), want[names[1]])
    assert np.array_equal(rg.audio.clip_onsets(pred_file, n, get.detector), want[names[1]])
    # a clip without onsets is the existing error
    silent = os.path.join(str(folder), "eval", names[2], "gt_audio.wav")
    keep = open(silent, "rb").read()
    try:
        jf.write_wav(silent, inp["n_samples"], np.zeros(0, np.int64))
        with pytest.raises(ValueError, match=names[2] + ".*no audio onsets"):
            ev.evaluate_folder(str(folder / "eval"), enc, eval_n=jf.EVAL_N, smplx=sm, avg_vel=gold["avg_vel"], onsets="device")
    finally:
        with open(silent, "wb") as f:
            f.write(keep)


def test_cli_saves_the_onsets_and_reads_them_back(rg, folder, capsys):
    ev = rg.evaluation
    base = [str(folder / "eval"), "--e_path", str(folder / "ckpt.bin"), "--eval_n", str(jf.EVAL_N), "--smplx_path",
            str(folder / "model.npz"), "--avg_vel_path", str(folder / "avg_vel.npy")]
    out = str(folder / "used_onsets.npz")
    ev.main(base + ["--onsets", "device", "--save_onsets", out])
    first = capsys.readouterr().out
    ev.main(base + ["--onsets", out])
    second = capsys.readouterr().out
    assert first == second and first.count("\n") == 1
    line = json.loads(first)
    assert line["align"] > 0 and line["gt_align"] > 0 and "align_skipped" not in line
    want = _restated_onsets(str(folder), jf.clip_names())
    with np.load(out) as f:
        assert sorted(f.files) == sorted(want) and all(np.array_equal(f[k], want[k]) for k in want)
