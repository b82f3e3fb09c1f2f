"""GPU: word prominence on the device (rg_prosody_frames / _signal / _cwt / _words through prosody.ProminenceEstimator) against the
float64 restatement in tests/golden/prosody_fixture.py.  Every stage is checked against the restatement FED THE DEVICE'S OWN
OUTPUT of the stage before, so a rounding difference early cannot flip a discrete decision later: stage 1 on the waveforms, stage 2
on the device's energy / nccf / logf0, stage 3 on the device's sum, stage 4 on the device's transform (whose float32 values float64
compares exactly as the device does).

Bounds.  Each is the worst absolute error measured on an MI355X over the fixture set (the three FIXTURE_SEEDS clips and the nine
PARITY_LENS clips in one ragged call) x 4, rounded up to one significant digit -- the rule of tests/test_onsets_gpu.py -- and goes
through parity.check.  Measured (NOTEBOOK section 26):
    stage 1  |energy| 1.720e-06  |nccf| 2.263e-06  |logf0| 3.712e-06 (1 460 voiced frames compared, no lag differs)
    stage 2  |f0| 2.384e-07  |f0z| 1.973e-06  |ez| 1.186e-07  |dz| 8.160e-07  |c| 2.033e-06
    stage 3  |W| 1.452e-05 (largest |W| 23.98)
    stage 4  |line strength| 5.960e-06  |prominence, boundary| 5.960e-06 (largest strength 111.4)
Two ceilings hold whatever is measured, and are asserted: the nccf bound stays at or under a tenth of the fixtures' MIN_LAG_MARGIN
(1e-4: what makes exact equality of the lags a sound demand), and the W bound is at most 1e-4 of the fixture set's largest |W|.
"""
import importlib
import importlib.util
import json
import os
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BOUNDS = dict(energy=7e-6, nccf=1e-5, logf0=2e-5, f0=1e-6, f0z=8e-6, ez=5e-7, dz=4e-6, c=9e-6, W=6e-5, strength=3e-5, word=3e-5)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fx = _load("prosody_fixture")


@pytest.fixture(scope="module")
def rg():
    return importlib.import_module("rag-gesture_amd")


@pytest.fixture(scope="module")
def est(rg):
    return rg.prosody.ProminenceEstimator()


def _host(t):
    return t.cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def clips():
    """The fixture set: (name, waveform, words)."""
    return [("seed %d" % s,) + fx.fixture_clip(s) for s in fx.FIXTURE_SEEDS] + [("len %d" % n,) + fx.parity_clip(n) for n in fx.PARITY_LENS]


@pytest.fixture(scope="module")
def staged(est, clips):
    """The four stages on the whole fixture set in one ragged call each, everything read back once for all the tests."""
    fr = est.frames([y for _, y, _ in clips])
    sg = est.signal(fr, [w for _, _, w in clips])
    cw = est.cwt(sg)
    wd = est.words(cw)
    off = fr["frame_off"]
    host = {k: _host(fr[k]) for k in ("energy", "nccf", "lag", "logf0")}
    host.update({k: _host(sg[k]) for k in ("voiced", "f0", "f0z", "ez", "dz", "c", "status")})
    host["W"] = _host(cw["W"])
    host.update({k: _host(wd[k]) for k in ("peak_strength", "valley_strength", "prominence", "boundary", "prom_frame", "bnd_frame")})
    return dict(fr=fr, sg=sg, cw=cw, wd=wd, off=off, host=host, layout=sg["layout"])


def _span(staged, i):
    return slice(int(staged["off"][i]), int(staged["off"][i + 1]))


def _wspan(staged, i):
    return slice(int(staged["layout"]["word_off"][i]), int(staged["layout"]["word_off"][i + 1]))


# ------------------------------------------------------------------------------------------ 1. frames
def test_frames_parity(clips, staged, parity):
    assert BOUNDS["nccf"] <= fx.MIN_LAG_MARGIN / 10
    h, off = staged["host"], staged["off"]
    worst = dict(energy=0.0, nccf=0.0, logf0=0.0)
    compared = wrong = 0
    for i, (name, y, _) in enumerate(clips):
        T = 1 + len(y) // 160
        assert off[i + 1] - off[i] == T, name
        ref, s = fx.frames(y), _span(staged, i)
        use = ref["voiced"] & ~fx.left_out(ref)
        assert (ref["lag_margin"][ref["voiced"]] >= fx.MIN_LAG_MARGIN).all() and fx.left_out(ref).sum() <= fx.MAX_LEFT_OUT * max(ref["voiced"].sum(), 1)
        e = {k: float(np.abs(h[k][s] - ref[k]).max()) for k in ("energy", "nccf")}
        e["logf0"] = float(np.abs(h["logf0"][s] - ref["logf0"])[use].max()) if use.any() else 0.0
        bad = int((h["lag"][s] != ref["lag"])[use].sum())
        print("%-10s %3d frames, %3d compared: |energy| %.3e |nccf| %.3e |logf0| %.3e, lags that differ %d"
              % (name, T, use.sum(), e["energy"], e["nccf"], e["logf0"], bad))
        compared, wrong = compared + int(use.sum()), wrong + bad
        worst = {k: max(worst[k], e[k]) for k in worst}
    for k in ("energy", "nccf", "logf0"):
        print("stage 1 worst |%s - ref| %.3e" % (k, worst[k]))
    assert staged["fr"]["lag"].dtype == torch.int32 and staged["fr"]["energy"].dtype == torch.float32
    assert compared >= 1000 and wrong == 0
    for k in ("energy", "nccf", "logf0"):
        parity.check("prosody: %s vs float64 restatement" % k, worst[k], BOUNDS[k])


# ------------------------------------------------------------------------------------------ 2. signal
def _ref_signal(h, s, lay, ws, weights=fx.WEIGHTS):
    words = lay["words"]
    flat = [seg for w in words for seg in w]
    return fx.signal(h["energy"][s], h["nccf"][s], h["logf0"][s], lay["start_frame"][ws], lay["end_frame"][ws],
                     [seg[0][0] for seg in flat[ws]], [seg[0][1] for seg in flat[ws]], weights)


def test_signal_parity(clips, staged, parity):
    h, lay = staged["host"], staged["layout"]
    worst = {k: 0.0 for k in ("f0", "f0z", "ez", "dz", "c")}
    for i, (name, _, _) in enumerate(clips):
        s, ws = _span(staged, i), _wspan(staged, i)
        ref = _ref_signal(h, s, lay, ws)
        assert np.array_equal(h["voiced"][s] != 0, ref["voiced"]), name
        assert int(h["status"][i]) == ref["status"], name
        e = {k: float(np.abs(h[k][s] - ref[k]).max()) for k in worst}
        print("%-10s voiced %3d: " % (name, ref["voiced"].sum()) + " ".join("|%s| %.3e" % (k, v) for k, v in e.items()))
        worst = {k: max(worst[k], e[k]) for k in worst}
    for k, v in worst.items():
        print("stage 2 worst |%s - ref| %.3e" % (k, v))
    assert h["voiced"].sum() >= 1000 and (h["voiced"] == 0).sum() >= 100
    for k, v in worst.items():
        parity.check("prosody: %s vs float64 restatement on the device's stage 1" % k, v, BOUNDS[k])


def test_signal_degenerate_cases(est, parity):
    """Silence (no voiced frame: zeros, status 1, no NaN), a single voiced frame, no words, one word -- one ragged call."""
    rng = np.random.RandomState(5)
    T = [40, 300, 37, 61]
    off = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    energy = rng.uniform(-6.0, -2.0, off[-1]).astype(np.float32)
    nccf = rng.uniform(0.0, 0.45, off[-1]).astype(np.float32)
    logf0 = rng.uniform(4.5, 5.5, off[-1]).astype(np.float32)
    energy[:40] = np.float32(np.log(1e-10))                          # silence as stage 1 writes it
    nccf[:40] = 0.0
    nccf[40 + 123] = 0.9                                             # the second recording's only voiced frame
    energy[40 + 123] = -1.0
    nccf[340:340 + 37:3] = 0.8                                       # the third and fourth have several
    nccf[377::2] = 0.7
    words = [[[[0.05, 0.2], "a"], [[0.2, 0.33], "b"]], [[[0.5, 0.9], "c"], [[1.0, 1.4], "d"], [[2.0, 2.9], "e"]], [], [[[0.1, 0.45], "f"]]]
    fr = dict(energy=torch.from_numpy(energy).cuda(), nccf=torch.from_numpy(nccf).cuda(), logf0=torch.from_numpy(logf0).cuda(), frame_off=off)
    sg = est.signal(fr, words)
    h = {k: _host(sg[k]) for k in ("voiced", "f0", "f0z", "ez", "dz", "c", "status")}
    h.update(energy=energy.astype(np.float64), nccf=nccf.astype(np.float64), logf0=logf0.astype(np.float64))
    assert all(np.isfinite(h[k]).all() for k in ("f0", "f0z", "ez", "dz", "c"))
    assert h["status"].tolist() == [1, 0, 0, 0]
    a = slice(0, 40)
    assert not h["voiced"][a].any() and not h["f0"][a].any() and not h["f0z"][a].any() and not h["ez"][a].any() and h["dz"][a].any()
    b = slice(40, 340)
    assert h["voiced"][b].sum() == 1 and (h["f0"][b] == float(logf0[40 + 123])).all() and not h["f0z"][b].any()
    c = slice(340, 377)
    assert not h["dz"][c].any() and h["voiced"][c].sum() == 13                # no words: the duration track is zero
    d = slice(377, 438)
    assert np.abs(h["dz"][d]).max() < 1e-6                                    # one word: one knot, a flat track
    lay, errs = sg["layout"], []
    for i in range(4):
        s, ws = slice(int(off[i]), int(off[i + 1])), slice(int(lay["word_off"][i]), int(lay["word_off"][i + 1]))
        ref = _ref_signal(h, s, lay, ws)
        assert np.array_equal(h["voiced"][s] != 0, ref["voiced"]) and int(h["status"][i]) == ref["status"]
        errs.append({k: float(np.abs(h[k][s] - ref[k]).max()) for k in ("f0", "f0z", "ez", "dz", "c")})
        print("item %d: " % i + " ".join("|%s| %.3e" % kv for kv in errs[-1].items()))
    for k in ("f0", "f0z", "ez", "dz", "c"):
        parity.check("prosody degenerate items: %s" % k, max(e[k] for e in errs), BOUNDS[k])


# ------------------------------------------------------------------------------------------ 3. cwt
def test_cwt_parity(clips, staged, parity):
    h = staged["host"]
    worst = biggest = 0.0
    for i, (name, _, _) in enumerate(clips):
        s = _span(staged, i)
        ref = fx.cwt(h["c"][s])
        err = np.abs(h["W"][:, s] - ref)
        print("%-10s |W - ref| %.3e of max |W| %.3e" % (name, err.max(), np.abs(ref).max()))
        worst, biggest = max(worst, float(err.max())), max(biggest, float(np.abs(ref).max()))
        T = ref.shape[1]
        if T > 2 * fx.TILE:                                          # both ends and both tile borders lie inside what was compared
            near = np.r_[0:fx.RADII[-1], fx.TILE - 3:fx.TILE + 3, 2 * fx.TILE - 3:2 * fx.TILE + 3, T - fx.RADII[-1]:T]
            assert np.abs(ref[:, near]).max() > 0.1 and err[:, near].max() <= err.max()
    print("stage 3 worst |W - ref| %.3e, largest |W| %.3e" % (worst, biggest))
    assert BOUNDS["W"] <= 1e-4 * biggest
    parity.check("prosody: W vs float64 restatement on the device's sum", worst, BOUNDS["W"])


# ------------------------------------------------------------------------------------------ 4. words
def _check_words(h_W, got, sf, ef, what):
    """got: the device's stage 4 on one recording (host arrays); the restatement traces lines in float64 on the device's W."""
    ref = fx.words_stage(h_W, sf, ef)
    for k in ("peak_strength", "valley_strength"):
        assert np.array_equal(got[k] > 0, ref[k] > 0), (what, k)                  # the frames that start a line
    assert np.array_equal(got["prom_frame"], ref["prom_frame"]) and np.array_equal(got["bnd_frame"], ref["bnd_frame"]), what
    es = max(float(np.abs(got[k] - ref[k]).max()) for k in ("peak_strength", "valley_strength"))
    ew = max(float(np.abs(got[k] - ref[k]).max()) if len(sf) else 0.0 for k in ("prominence", "boundary"))
    return ref, es, ew


def test_words_parity(clips, staged, parity):
    h, lay = staged["host"], staged["layout"]
    worst_s = worst_w = 0.0
    lines = 0
    for i, (name, _, _) in enumerate(clips):
        s, ws = _span(staged, i), _wspan(staged, i)
        got = {k: h[k][s] for k in ("peak_strength", "valley_strength")}
        got.update({k: h[k][ws] for k in ("prominence", "boundary", "prom_frame", "bnd_frame")})
        ref, es, ew = _check_words(h["W"][:, s], got, lay["start_frame"][ws], lay["end_frame"][ws], name)
        print("%-10s %2d words, %3d peak and %3d valley lines: |strength| %.3e |word values| %.3e (largest %.3e)"
              % (name, ws.stop - ws.start, (ref["peak_strength"] > 0).sum(), (ref["valley_strength"] > 0).sum(), es, ew, ref["peak_strength"].max()))
        worst_s, worst_w, lines = max(worst_s, es), max(worst_w, ew), lines + int((ref["peak_strength"] > 0).sum())
    print("stage 4 worst |strength - ref| %.3e, |prominence / boundary - ref| %.3e" % (worst_s, worst_w))
    assert lines >= 100
    parity.check("prosody: line strengths vs float64 restatement on the device's W", worst_s, BOUNDS["strength"])
    parity.check("prosody: prominence and boundary vs float64 restatement on the device's W", worst_w, BOUNDS["word"])


def test_words_cases(est, clips, staged, parity):
    """On the first fixture clip's transform, with words of the test's own: a word without frames, a word in which no line starts,
    and a last word that ends long before the recording does (its boundary range runs to the end)."""
    h = staged["host"]
    s = _span(staged, 0)
    T = s.stop - s.start
    peak, valley = h["peak_strength"][s], h["valley_strength"][s]
    quiet = next(t for t in range(20, T - 3) if not peak[t:t + 3].any())          # three frames in which no peak line starts
    # a last word of three frames whose strongest valley line from its middle on starts behind it
    last = next(a for a in range(quiet + 5, T - 30) if valley[a + 1:].max() > 0 and a + 1 + int(np.argmax(valley[a + 1:])) >= a + 3)
    at = lambda frame: frame / 100.0 - 0.005                          # (half a frame early: no time falls on a frame)
    words = [[[0.0, at(quiet - 5)], "early"], [[at(quiet - 10), at(quiet - 5)], "swallowed"], [[at(quiet), at(quiet + 3)], "flat"],
             [[at(last), at(last + 3)], "last"]]
    cw = dict(W=staged["cw"]["W"][:, s].contiguous(), frame_off=np.array([0, T], np.int64))
    wd = est.words(cw, [words])
    sf, ef = wd["layout"]["start_frame"], wd["layout"]["end_frame"]
    assert sf[1] == ef[1] and (sf[2], ef[2]) == (quiet, quiet + 3) and (sf[3], ef[3]) == (last, last + 3)
    got = {k: _host(wd[k]) for k in ("peak_strength", "valley_strength", "prominence", "boundary", "prom_frame", "bnd_frame")}
    assert np.array_equal(got["peak_strength"], peak) and np.array_equal(got["valley_strength"], valley)      # the lines do not depend on the words
    ref, es, ew = _check_words(h["W"][:, s], got, sf, ef, "cases")
    assert got["prominence"][1] == got["boundary"][1] == 0 and got["prom_frame"][1] == got["bnd_frame"][1] == -1
    assert got["prominence"][2] == 0 and got["prom_frame"][2] == -1 and got["prominence"].max() > 0
    mid = (int(sf[3]) + int(ef[3]) - 1) // 2
    tail = valley[mid:]
    assert got["boundary"][3] == tail.max() > 0 and got["bnd_frame"][3] == mid + int(np.argmax(tail)) >= ef[3]
    # the swallowed word stands between `early` and `flat`: early's boundary range ends at flat's middle
    assert got["bnd_frame"][0] < (quiet + quiet + 2) // 2
    parity.check("prosody cases: line strengths", es, BOUNDS["strength"])
    parity.check("prosody cases: prominence and boundary", ew, BOUNDS["word"])


# ------------------------------------------------------------------------------------------ 5. composition and batching
KEYS = ("peak_strength", "valley_strength", "prominence", "boundary", "prom_frame", "bnd_frame")


def test_run_equals_the_stages_and_a_batch_equals_its_items(est, clips, staged):
    rows = est.run([y for _, y, _ in clips], [w for _, _, w in clips], boundaries=True)
    prom, bnd = staged["wd"]["prominence"].cpu().numpy(), staged["wd"]["boundary"].cpu().numpy()
    k = 0
    for (name, _, words), r in zip(clips, rows):
        assert len(r) == len(words)
        for seg, row in zip(words, r):
            assert row == (seg[1], float(seg[0][0]), float(seg[0][1]), float(prom[k]), float(bnd[k])), name
            k += 1
    assert k == prom.size
    short = est.run([clips[0][1]], [clips[0][2]])[0]
    assert short == [r[:4] for r in rows[0]] and all(type(v) is float for v in short[0][1:])
    # the 3 s parity clip alone and as the middle item of three: every stage's every output, bit for bit
    mid = len(fx.FIXTURE_SEEDS) + fx.PARITY_LENS.index(48000)
    quiet = (clips[1][1].astype(np.float64) * 0.01).astype(np.float32)            # (a neighbour 40 dB down: its maximum must not leak)
    ys, ws = [clips[-1][1], clips[mid][1], quiet], [clips[-1][2], clips[mid][2], clips[1][2]]
    together, alone = est.run_device(ys, ws), est.run_device(ys[1:2], ws[1:2])
    fo, wo = together["frame_off"], together["word_off"]
    for key in KEYS:
        sl = slice(int(fo[1]), int(fo[2])) if key.endswith("strength") else slice(int(wo[1]), int(wo[2]))
        assert torch.equal(together[key][sl], alone[key]), key
    s = _span(staged, mid)
    assert torch.equal(alone["peak_strength"], staged["wd"]["peak_strength"][s]) and float(alone["prominence"].max()) > 0
    fr3, fr1 = est.frames(ys), est.frames(ys[1:2])
    sg3, sg1 = est.signal(fr3, ws), est.signal(fr1, ws[1:2])
    cw3, cw1 = est.cwt(sg3), est.cwt(sg1)
    sl = slice(int(fo[1]), int(fo[2]))
    for a, b, keys in ((fr3, fr1, ("energy", "nccf", "lag", "logf0")), (sg3, sg1, ("voiced", "f0", "f0z", "ez", "dz", "c"))):
        for key in keys:
            assert torch.equal(a[key][sl], b[key]), key
    assert torch.equal(cw3["W"][:, sl], cw1["W"]) and torch.equal(sg3["status"][1:2], sg1["status"])


# ------------------------------------------------------------------------------------------ 6. meaning
def test_the_emphasised_word_ranks_first_on_the_device(est):
    y, words = fx.emphasis_clip()
    rows = est.run([y], [words])[0]
    prom = np.array([r[3] for r in rows])
    print("prominence per word:", np.round(prom, 3).tolist())
    assert int(np.argmax(prom)) == 3 and prom[3] > 1.2 * np.delete(prom, 3).max()


# ------------------------------------------------------------------------------------------ 7. annotate and the CLI
def test_annotate_and_cli(rg, est, tmp_path):
    y, words = fx.fixture_clip(fx.FIXTURE_SEEDS[0])
    n = 90
    mk = lambda ann: rg.dataset.RawClip("clip", np.zeros((n, 165), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 100), np.float32),
                                        np.zeros(300), 2, annotations=ann, audio=y)
    want = est.run([y], [words])[0]
    clip = mk(dict(text_segments=words))
    assert clip.annotations["prominence"] == [] and rg.prosody.annotate(clip, est) is clip
    assert clip.annotations["prominence"] == want and len(want) == len(words) and max(r[3] for r in want) > 0
    cut = rg.longform.window_annotations({k: [clip.annotations[k]] for k in rg.dataset.ANNOTATION_KEYS}, 0.0, 2.0)["prominence"][0]
    assert 1 <= len(cut) < len(want) and cut == [r for r in want if r[2] <= 2.0]
    given = [("kept", 0.0, 0.5, 1.25)]
    clip = mk(dict(text_segments=words, prominence=given))
    rg.prosody.annotate(clip, est)
    assert clip.annotations["prominence"] == given
    # the CLI: a PCM16 file and a word list in, a .prom file out that reads back to run()'s tuples on what the file holds
    wav, wj, out = str(tmp_path / "take_01.wav"), str(tmp_path / "words.json"), str(tmp_path / "take_01.prom")
    pcm = np.clip(np.round(y.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    with wave.open(wav, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.tobytes())
    with open(wj, "w") as f:
        json.dump(words, f)
    rg.prosody.main([wav, "--words", wj, "-o", out])
    heard = est.run([rg.audio.read_wav_16k(wav)], [words], boundaries=True)[0]
    assert rg.prosody.read_prom(out) == [r[:4] for r in heard]
    assert [r[:5] for r in rg.prosody.read_prom_rows(out)] == heard and {r[5] for r in rg.prosody.read_prom_rows(out)} == {"take_01"}
    rg.prosody.main([wav, "--words", wj, "-o", out, "--resample_audio", "--basename", "b"])
    assert rg.prosody.read_prom(out) == [r[:4] for r in heard] and rg.prosody.read_prom_rows(out)[0][5] == "b"
