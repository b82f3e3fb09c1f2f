"""CPU: the host side of word timings and frame-aligned word features (rag-gesture_amd/align.py, features.BertFeatures.word_rows)
against tests/golden/ctc_fixture.py, and the fixture's own recurrence on cases whose answer is known by construction."""
import importlib
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fx = _load("ctc_fixture")


@pytest.fixture(scope="module")
def al():
    return importlib.import_module("rag-gesture_amd").align


def _tokens(al, words):
    return al.text_tokens(words, al.vocab_chars(fx.VOCAB, fx.BLANK, fx.DELIMITER), fx.VOCAB[fx.DELIMITER])


def test_header_constants(al):
    assert (al.MAX_VOCAB, al.MAX_STATES, al.PER) == (64, 4096, 16)
    assert importlib.import_module("rag-gesture_amd").capi.header_version() >= 126


def test_tokens_normalisation(al):
    V = fx.VOCAB
    words = ["Don’t", "42", "sToP", "<s>", "a|b", "..."]
    ids, word_of = _tokens(al, words)
    want = [V["D"], V["O"], V["N"], V["'"], V["T"], V["|"], V["S"], V["T"], V["O"], V["P"], V["|"], V["S"], V["|"], V["A"], V["B"]]
    assert ids == want                                      # "<s>" is its letter, never the special; "|" inside a word is dropped
    assert word_of == [0] * 5 + [-1] + [2] * 4 + [-1] + [3] + [-1] + [4, 4]
    assert (ids, word_of) == fx.tokens(words)
    assert V["<pad>"] not in ids and V["<s>"] not in ids and ids[0] != V["|"] and ids[-1] != V["|"]
    assert _tokens(al, ["42", "..."]) == ([], [])            # nothing alignable: no delimiter either
    assert _tokens(al, ["7", "go", "8"]) == ([V["G"], V["O"]], [1, 1])
    # a vocabulary with lower-case letters: as is first, then the other case
    chars = al.vocab_chars({"<pad>": 0, "|": 1, "a": 2, "B": 3}, 0, "|")
    assert al.text_tokens(["AbB"], chars, 1) == ([2, 3, 3], [0, 0, 0])


def test_time_rule_with_unalignable_words(al):
    words = ["12", "hi", "3", "4", "yo", "5"]
    ids, word_of = _tokens(al, words)                        # H I | Y O
    first, last = [2, 4, 6, 9, 11], [3, 5, 8, 10, 12]
    fs = np.arange(14) * 320
    got = al.word_times(words, word_of, first, last, fs, 14 * 320 - 100)
    total = (14 * 320 - 100) / 16000
    assert got == fx.word_times(words, word_of, first, last, fs, 14 * 320 - 100)
    assert got[1] == [[2 * 320 / 16000, 6 * 320 / 16000], "hi"] and got[4] == [[9 * 320 / 16000, 13 * 320 / 16000], "yo"]
    assert got[0] == [[0.0, got[1][0][0]], "12"]                                  # at the start: from 0
    assert got[2] == got[3][:1] + ["3"] and got[3] == [[got[1][0][1], got[4][0][0]], "4"]      # in the middle: between the neighbours
    assert got[5] == [[got[4][0][1], total], "5"]                                 # at the end: to the audio's end
    # the clamp: a last frame that reaches past the audio, and a frame table that is not 320 t
    fs2 = np.array([0, 320, 160000, 160320])
    got = al.word_times(["a", "b"], [0, -1, 1], [0, 1, 2], [0, 1, 3], fs2, 160500)
    assert got == [[[0.0, 320 / 16000], "a"], [[10.0, 160500 / 16000], "b"]]
    assert al.word_times(["1", "2"], [], [], [], fs2, 32000) == [[[0.0, 2.0], "1"], [[0.0, 2.0], "2"]]


def test_greedy_collapse(al):
    V = fx.VOCAB
    best = [0, V["H"], V["H"], 0, V["I"], V["|"], V["|"], 0, V["L"], 0, V["L"], V["L"], V["|"]]
    got = al.greedy_collapse(best, fx.BLANK, V["|"])
    assert got == fx.greedy(best)
    assert got == [[(V["H"], 1, 2), (V["I"], 4, 4)], [(V["L"], 8, 8), (V["L"], 10, 11)]]
    assert al.greedy_collapse([0, 0, V["|"], 0], fx.BLANK, V["|"]) == []


def test_word_rows():
    F = importlib.import_module("rag-gesture_amd").features
    pieces = {"so": [7], "unbelievable": [8, 9, 10], "day!": [11, 12]}
    tok = lambda text: [101] + [p for w in text.split() for p in pieces[w]] + [102]
    assert F.BertFeatures.word_rows(["so", "unbelievable", "day!"], tok) == [1, 2, 5, 7]
    assert F.BertFeatures.word_rows([], tok) == [1]
    joined = lambda text: [101] + ([99] if text == "so day!" else [p for w in text.split() for p in pieces[w]]) + [102]
    with pytest.raises(ValueError, match="so"):
        F.BertFeatures.word_rows(["so", "day!"], joined)
    empty = lambda text: [101] + [p for w in text.split() for p in {"so": [7], "~": []}[w]] + [102]
    with pytest.raises(ValueError, match="~"):
        F.BertFeatures.word_rows(["so", "~"], empty)


@pytest.mark.parametrize("T,L,kind", [(1, 1, "mixed"), (9, 4, "equal"), (40, 12, "mixed"), (200, 60, "mixed")])
def test_fixture_finds_a_planted_path(T, L, kind):
    rng = np.random.default_rng(100 + T)
    y = fx.random_tokens(rng, L, len(fx.VOCAB), kind=kind)
    path, E = fx.planted_path(rng, T, y)
    for dtype in (np.float64, np.float32):
        r = fx.viterbi(E, y, dtype=dtype)
        assert r["status"] == 0 and r["score"] == 0.0 and np.array_equal(r["path"], path)
        for j in range(L):
            frames = np.nonzero(path == 2 * j + 1)[0]
            assert (r["tok_first"][j], r["tok_last"][j]) == (frames[0], frames[-1])


def test_fixture_recurrence_fp32_equals_fp64_on_exact_emissions():
    rng = np.random.default_rng(7)
    for _ in range(20):
        T, L = int(rng.integers(1, 40)), int(rng.integers(1, 12))
        y = fx.random_tokens(rng, L, 32)
        E = fx.exact_emissions(rng, T, 32)
        a, b = fx.viterbi(E, y, dtype=np.float32), fx.viterbi(E, y, dtype=np.float64)
        assert a["status"] == b["status"] and np.array_equal(a["path"], b["path"]) and a["score"] == b["score"]
        if a["status"] == 0:
            assert fx.path_is_valid(a["path"], y) and fx.path_score(E, a["path"], y) == float(a["score"])
        else:
            assert T < L + sum(y[j] == y[j - 1] for j in range(1, L))
    r = fx.viterbi(fx.exact_emissions(rng, 3, 32), [7, 7, 9])          # AAB needs 4 frames
    assert r["status"] == 1 and not r["path"].any()


def test_fixture_word_frames_overwrite_and_clamp():
    hidden = np.arange(7 * 2, dtype=np.float64).reshape(7, 2)
    segs = [[[0.0, 0.4], "a"], [[0.2, 0.6], "b"], [[0.7, 0.7], "c"], [[0.9, 3.0], "d"]]
    out = fx.word_frames(hidden, [[1], [2, 3], [4], [5]], segs, 12, pose_fps=10)
    assert (out[0:2] == hidden[1]).all() and (out[2:6] == hidden[2:4].mean(0)).all()       # the later word wins frames 2, 3
    assert not out[6:9].any() and (out[9:] == hidden[5]).all() and out.shape == (12, 2)
