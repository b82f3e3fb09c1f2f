"""CPU: the word-prominence estimator's host side (rag-gesture_amd/prosody.py) and the conditions its float64 restatement
(tests/golden/prosody_fixture.py) must meet for the GPU test's exact comparisons to be sound: the fixtures' lag margins and the cap
on frames left out, the word-to-frame rule, .prom files, the annotation shape downstream code takes, what the estimate means on
a clip with one emphasised word, and the header's four entry points."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from oracle import retrieval as oret

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fx = _load("prosody_fixture")


@functools.lru_cache(None)
def _frames(kind, key):
    y, words = fx.fixture_clip(key) if kind == "seed" else fx.parity_clip(key)
    return fx.frames(y), words


CLIPS = [("seed", s) for s in fx.FIXTURE_SEEDS] + [("len", n) for n in fx.PARITY_LENS]


# ------------------------------------------------------------------------------------------ the fixture's own conditions
@pytest.mark.parametrize("kind,key", CLIPS)
def test_fixture_margins_and_cap(kind, key):
    fr, words = _frames(kind, key)
    n = 48000 if kind == "seed" else key
    T = 1 + n // 160
    assert fr["energy"].shape == fr["nccf"].shape == fr["lag"].shape == (T,)
    v = fr["voiced"]
    out = fx.left_out(fr)
    print("%s %s: %d frames, %d voiced, min lag margin %.3e, %d left out, min voicing margin %.3e"
          % (kind, key, T, v.sum(), fr["lag_margin"][v].min() if v.any() else np.inf, out.sum(), fr["voicing_margin"].min()))
    assert (fr["lag_margin"][v] >= fx.MIN_LAG_MARGIN).all()
    assert out.sum() <= fx.MAX_LEFT_OUT * max(v.sum(), 1)
    assert (fr["lag"] >= fx.LAG_MIN).all() and (fr["lag"] <= fx.LAG_MAX).all() and np.isfinite(fr["logf0"]).all()
    if n >= 1023:
        assert v.sum() >= 5 and (v & ~out).sum() >= 5                # there is something to compare
    if n >= 48000:
        assert len(words) >= 4 and v.sum() >= 0.5 * T and (~v).sum() >= 10


def test_fixture_clip_counts():
    assert len(fx.FIXTURE_SEEDS) >= 3 and fx.PARITY_LENS[:7] == (1, 159, 160, 161, 1023, 1024, 1025)
    T = [fx.n_frames(n) for n in fx.PARITY_LENS]
    assert T[:7] == [1, 1, 2, 2, 7, 7, 7] and T[7] == 301 and T[8] > 2 * fx.TILE > 2 * fx.RADII[-1]    # (a tile with a neighbour on both sides)
    assert 301 > fx.TILE and fx.RADII == [10, 15, 20, 29, 40, 57, 80, 114, 160, 227] and fx.REACH[1:] == [3, 4, 6, 8, 12, 16, 23, 32, 46]
    assert fx.NPROD == 757 and sum(2 * r + 1 for r in fx.RADII) == 1514


# ------------------------------------------------------------------------------------------ the header and the module
def test_header_exports_the_entry_points(rg):
    syms = rg.capi.header_symbols()
    assert {"rg_prosody_frames", "rg_prosody_signal", "rg_prosody_cwt", "rg_prosody_words"} <= set(syms)
    c = rg.capi.header_constants()
    assert c["RG_VERSION"] >= 127
    assert (c["RG_PROSODY_HOP"], c["RG_PROSODY_WIN"], c["RG_PROSODY_LAG_MIN"], c["RG_PROSODY_LAG_MAX"], c["RG_PROSODY_SCALES"]) == \
        (fx.HOP, fx.WIN, fx.LAG_MIN, fx.LAG_MAX, fx.SCALES)
    assert c["RG_PROSODY_TILE"] == fx.TILE and c["RG_PROSODY_HALO"] == fx.RADII[-1] and c["RG_PROSODY_TAPS"] == 1514
    taps, radii = rg.prosody.wavelet_taps()
    assert radii == fx.RADII and np.array_equal(taps, np.concatenate([fx.taps(j) for j in range(fx.SCALES)]))
    for j in range(fx.SCALES):                                       # a wavelet: no response to a constant, up to the cut at 5 s
        assert abs(fx.taps(j).sum()) < 1e-3 * np.abs(fx.taps(j)).sum()


def test_no_gpu_no_estimator(rg, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(rg.capi.RgError, match="no CPU fallback"):
        rg.prosody.ProminenceEstimator()


# ------------------------------------------------------------------------------------------ words -> frames
def test_word_frames_rule(rg):
    wf = rg.prosody.word_frames
    seg = lambda a, b, w="w": [[a, b], w]
    # frame t stands at t / 100 s and belongs to a word when start <= t / 100 < end
    s, e = wf([seg(0.0, 0.1), seg(0.1, 0.25), seg(0.251, 0.259), seg(0.3, 0.5)], 100)
    assert s.tolist() == [0, 10, 26, 30] and e.tolist() == [10, 25, 26, 50]          # (the third word lies between two frames)
    assert s.dtype == e.dtype == np.int32
    # times that are no multiple of 10 ms in binary: 0.07 * 100 > 7, and still frame 7 stands at 7 / 100 >= 0.07
    s, e = wf([seg(0.07, 0.29), seg(0.29, 0.57)], 100)
    assert s.tolist() == [7, 29] and e.tolist() == [29, 57]
    for k in range(0, 400):
        t = k / 100
        assert rg.prosody._first_frame_at(t) == k == fx.first_frame_at(t)
        assert rg.prosody._first_frame_at(np.nextafter(t, 1e9)) == k + 1 and rg.prosody._first_frame_at(np.nextafter(t, -1e9)) == max(k, 0)
    # overlap: the later word starts where the earlier one ended; a word swallowed whole is left without frames
    s, e = wf([seg(0.0, 0.3), seg(0.2, 0.4), seg(0.25, 0.35), seg(0.5, 0.6)], 100)
    assert s.tolist() == [0, 30, 40, 50] and e.tolist() == [30, 40, 40, 60]
    # the recording's end and negative times clamp
    s, e = wf([seg(-0.5, 0.05), seg(0.9, 1.5), seg(2.0, 3.0)], 100)
    assert s.tolist() == [0, 90, 100] and e.tolist() == [5, 100, 100]
    assert [a.tolist() for a in wf([], 10)] == [[], []]
    with pytest.raises(ValueError, match="sorted by start"):
        wf([seg(0.5, 0.6), seg(0.1, 0.2)], 100)
    with pytest.raises(ValueError, match="not finite"):
        wf([seg(0.5, float("nan"))], 100)
    # the fixture's own statement of the rule agrees
    for kind, key in CLIPS[:3]:
        words = _frames(kind, key)[1]
        a, b = fx.word_frames(words, 301)
        s, e = wf(words, 301)
        assert np.array_equal(a, s) and np.array_equal(b, e) and (e > s).all()


# ------------------------------------------------------------------------------------------ .prom files
def test_prom_round_trip_and_the_references_layout(rg, tmp_path):
    p = rg.prosody
    rows = [("so", 0.25, 0.5, 1.2345678901234567, 0.5), ("", 0.5, 0.75, 0.0, 0.0), ("because", 1.0 / 3.0, 2.0 / 3.0, 3.25e-7, 12.5)]
    path = str(tmp_path / "2_scott_0_1_1.prom")
    p.write_prom(path, "2_scott_0_1_1", rows)
    assert p.read_prom(path) == [r[:4] for r in rows]
    assert p.read_prom_rows(path) == [r + ("2_scott_0_1_1",) for r in rows]
    with open(path) as f:
        lines = f.read().splitlines()
    assert len(lines) == 3 and all(line.count("\t") == 5 and line.startswith("2_scott_0_1_1\t") for line in lines)
    p.write_prom(path, "b", [r[:4] for r in rows])                   # 4-tuples: the boundary column is written as 0
    assert [r[4] for r in p.read_prom_rows(path)] == [0.0, 0.0, 0.0] and p.read_prom(path) == [r[:4] for r in rows]
    # a file as the offline tool lays it out: Basename start end word prominence boundary, an empty word in the second row
    hand = str(tmp_path / "hand.prom")
    with open(hand, "w") as f:
        f.write("1_wayne_0_1_1\t0.00\t0.37\thello\t0.912\t0.104\n1_wayne_0_1_1\t0.37\t0.52\t\t0.000\t1.750\n"
                "1_wayne_0_1_1\t0.52\t0.90\tworld\t2.031\t0.000\n")
    assert p.read_prom(hand) == [("hello", 0.0, 0.37, 0.912), ("", 0.37, 0.52, 0.0), ("world", 0.52, 0.9, 2.031)]
    with pytest.raises(ValueError, match="row 1 has 5 columns"):
        bad = str(tmp_path / "bad.prom")
        with open(bad, "w") as f:
            f.write("x\t0\t1\tw\t0.5\n")
        p.read_prom(bad)
    with pytest.raises(ValueError, match="tab"):
        p.write_prom(path, "b", [("a\tb", 0.0, 1.0, 0.0)])


# ------------------------------------------------------------------------------------------ meaning, and the shape downstream
@functools.lru_cache(None)
def _emphasis():
    y, words = fx.emphasis_clip()
    return fx.estimate(y, words), words


def test_the_emphasised_word_ranks_first():
    est, words = _emphasis()
    prom = est["words"]["prominence"]
    print("prominence per word:", np.round(prom, 3).tolist())
    assert len(words) >= 5 and est["signal"]["status"] == 0
    assert int(np.argmax(prom)) == 3 and prom[3] > 1.2 * np.delete(prom, 3).max()
    assert (est["words"]["prom_frame"][prom > 0] >= 0).all() and (est["words"]["boundary"] >= 0).all()
    # every word's value comes from a line that starts inside the word
    for w, f in enumerate(est["words"]["prom_frame"]):
        assert f < 0 or est["start_frame"][w] <= f < est["end_frame"][w]


def test_rows_pass_through_the_annotation_consumers(rg, tmp_path):
    est, words = _emphasis()
    rows = [r[:4] for r in est["rows"]]                              # run()'s tuples: (word, start, end, prominence)
    # ... as a connective list sees them (rag/utils.py map_conns_to_prominence): the words' own values, by position
    got = oret.map_conns_to_prominence([words[1][1], words[3][1], "absent"], rows)
    assert got == {0: (words[1][1], rows[1][3]), 1: (words[3][1], rows[3][3]), 2: None}
    # ... cut to a window: the tuples fully inside, in window time
    t0, t1 = rows[1][1], rows[4][2]
    cut = rg.longform.window_annotations(dict(prominence=[rows]), t0, t1)["prominence"][0]
    assert [c[0] for c in cut] == [r[0] for r in rows[1:5]] and [c[3] for c in cut] == [r[3] for r in rows[1:5]]
    assert all(len(c) == 4 for c in cut) and cut[0][1] == 0.0 and cut[-1][2] == pytest.approx(t1 - t0)
    # ... and through a file
    path = str(tmp_path / "clip.prom")
    rg.prosody.write_prom(path, "clip", est["rows"])
    assert rg.prosody.read_prom(path) == rows
    assert "prominence" in rg.dataset.ANNOTATION_KEYS
