"""GPU: word timings and frame-aligned word features (csrc/rg_ctc.hip through rag-gesture_amd/align.py and
features.WindowFeatures(frame_words=True)) against the float64 restatement in tests/golden/ctc_fixture.py.

Bounds, each from the arithmetic and not from what the device gave:
  log-softmax   |logp - fixture| <= 2^-23 (|logp| + 8): one rounding each on x - max and on the final subtraction, expf / logf
                at a few ulp, a 6-level butterfly of terms in [0, 1] whose sum is >= 1.
  alignment     exact emissions (multiples of 1/8 in [-16, 0]: every fp32 sum of up to 1100 of them is exact) -> every output
                equal to the fixture's, bit for bit.
  float scores  the device path's float64 score within 2 T 2^-24 max|a| of the fixture's optimum (one add rounding per step on
                each of the two paths compared; max|a| = the larger of the two scores' magnitudes: the terms are all <= 0, so a
                path's partial sums never exceed its total in magnitude).
  word frames   per component 2^-23 sum_j |x_j| over the word's token rows (ctc_fixture.word_frames_bound).
Measured on an MI355X (NOTEBOOK section 25): log-softmax 0.789 of its bound at worst, word frames 0.277 of theirs, the float
case's device path was the fixture's optimum."""
import ctypes
import importlib
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fx = _load("ctc_fixture")
V32 = len(fx.VOCAB)


@pytest.fixture(scope="module")
def h(rg):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return rg.capi.get_handle(0)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ log-softmax
@pytest.mark.parametrize("V", [2, 32, 33, 64])
@pytest.mark.parametrize("rows", [1, 5, 499])
def test_log_softmax(rg, h, parity, rows, V):
    rng = np.random.default_rng(1000 * rows + V)
    x = rng.uniform(-30.0, 30.0, size=(rows, V)).astype(np.float32)
    x[rows // 2] = np.float32(rng.uniform(-30.0, 30.0))                   # a row of equal values
    x[0, 0], x[0, V - 1] = 30.0, -30.0
    buf = torch.full((rows * V + 8,), float("nan"))
    buf[:rows * V] = torch.from_numpy(x).view(-1)
    out = torch.full((rows * V + 8,), float("nan"), device="cuda")
    best = torch.full((rows + 4,), -7, dtype=torch.int32, device="cuda")
    h.call("ctc_log_softmax", buf.cuda(), rows, V, out, best)
    torch.cuda.synchronize()
    assert torch.isnan(out[rows * V:]).all() and (best[rows:] == -7).all()      # nothing written behind the last row
    got = out[:rows * V].view(rows, V).cpu().double().numpy()
    ref = fx.log_softmax(x)
    ratio = (np.abs(got - ref) / (2.0 ** -23 * (np.abs(ref) + 8.0))).max()
    print("rg_ctc_log_softmax rows=%d V=%d: max |err| = %.3e, max |err| / bound = %.3f" % (rows, V, np.abs(got - ref).max(), ratio))
    parity.check("rg_ctc_log_softmax rows=%d V=%d: worst |logp - fp64| / (2^-23 (|logp| + 8))" % (rows, V), ratio, 1.0)
    # best: exact where the top two differ by more than the bound (always, here, except the row of equal values: lowest index)
    top2 = np.sort(x, 1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 1e-5
    clear[rows // 2] = True
    assert np.array_equal(best[:rows].cpu().numpy()[clear], x.argmax(1)[clear]) and best[rows // 2].item() == 0
    for bad_v in (1, 65):
        with pytest.raises(rg.capi.RgError):
            h.call("ctc_log_softmax", out, 1, bad_v, out, best)


def test_log_softmax_ties_take_the_lower_index(rg, h):
    x = torch.tensor([[1.0, 5.0, 5.0, -2.0, 5.0], [0.0, -1.0, -1.0, 0.0, -3.0], [-4.0, -4.0, -4.0, -4.0, 9.0]], device="cuda")
    _, best = rg.align.log_softmax(h, x)
    assert best.tolist() == [1, 0, 4]


# ------------------------------------------------------------------------------------------------ alignment, exact
def _device_items(rg, h, items):
    """items: list of (E [T, V] float32, y) -> the device's outputs per item, from ONE call."""
    off = np.concatenate([[0], np.cumsum([e.shape[0] for e, _ in items])])
    logp = torch.from_numpy(np.concatenate([e for e, _ in items])).cuda()
    r = rg.align.viterbi(h, logp, off.tolist(), [y for _, y in items], fx.BLANK)
    torch.cuda.synchronize()
    path, first, last = r["path"].cpu().numpy(), r["tok_first"].cpu().numpy(), r["tok_last"].cpu().numpy()
    score, status, to = r["score"].cpu().numpy(), r["status"].cpu().numpy(), r["tok_off"]
    return [dict(path=path[off[i]:off[i + 1]], tok_first=first[to[i]:to[i + 1]], tok_last=last[to[i]:to[i + 1]], score=score[i],
                 status=int(status[i])) for i in range(len(items))]


def _same(got, ref):
    return (got["status"] == ref["status"] and np.array_equal(got["path"], ref["path"]) and np.array_equal(got["tok_first"], ref["tok_first"])
            and np.array_equal(got["tok_last"], ref["tok_last"])
            and np.float32(got["score"]).tobytes() == np.float32(ref["score"]).tobytes())


@pytest.mark.parametrize("T,L", [(1, 1), (2, 1), (7, 3), (64, 16), (65, 17), (499, 200), (1100, 511), (1100, 512)])
def test_align_exact(rg, h, T, L):
    """Token strings with repeated adjacent characters and with all characters equal; (64, 16) / (65, 17) cross a thread's 16
    states, (1100, 511) / (1100, 512) have S = 1023 / 1025: 64 threads' worth and one more."""
    rng = np.random.default_rng(31 * T + L)
    for kind in ("mixed", "equal"):
        y = fx.random_tokens(rng, L, V32, kind=kind)
        E = fx.exact_emissions(rng, T, V32)
        ref = fx.viterbi(E, y)
        assert ref["status"] == 0 and fx.path_is_valid(ref["path"], y)
        got = _device_items(rg, h, [(E, y)])[0]
        assert _same(got, ref), (T, L, kind)


def test_align_infeasible_and_refusals(rg, h):
    rng = np.random.default_rng(5)
    A, B = fx.VOCAB["A"], fx.VOCAB["B"]
    E3, E9 = fx.exact_emissions(rng, 3, V32), fx.exact_emissions(rng, 9, V32)
    bad, good = _device_items(rg, h, [(E3, [A, A, B]), (E9, [A, A, B])])           # AAB needs 4 frames
    assert bad["status"] == 1 and not bad["path"].any() and bad["score"] == -np.inf
    assert (bad["tok_first"] == -1).all() and (bad["tok_last"] == -1).all()
    assert _same(bad, fx.viterbi(E3, [A, A, B])) and _same(good, fx.viterbi(E9, [A, A, B]))
    # refused on the host, before any launch
    logp = torch.from_numpy(E9).cuda()
    with pytest.raises(rg.capi.RgError):
        rg.align.viterbi(h, logp, [0, 9], [[A] * 2048], fx.BLANK)                 # S = 4097
    with pytest.raises(rg.capi.RgError):
        rg.align.viterbi(h, logp, [0, 9], [[A, fx.BLANK, B]], fx.BLANK)           # a blank inside the target
    with pytest.raises(rg.capi.RgError):
        rg.align.viterbi(h, logp, [0, 9], [[A, V32]], fx.BLANK)                   # a token outside the vocabulary
    with pytest.raises(rg.capi.RgError):
        rg.align.viterbi(h, logp, [0, 8], [[A]], fx.BLANK)                        # offsets that do not cover the rows
    # the entry point's own checks of the host copies (the device tables are what a correct caller would send)
    i64 = lambda v: ((ctypes.c_int64 * len(v))(*v), torch.tensor(v, dtype=torch.int64, device="cuda"))
    ints = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")
    tokens = torch.full((4096,), A, dtype=torch.int32, device="cuda")

    def call(frame_off, tok_off, bp_off, words=64):
        (fh, fd), (th, td), (bh, bd) = i64(frame_off), i64(tok_off), i64(bp_off)
        h.call("ctc_align", logp, V32, fd, fh, tokens, td, th, 1, fx.BLANK, ints(words), bd, bh, ints(9), ints(4096), ints(4096),
               torch.zeros(1, device="cuda"), ints(1))

    call([0, 9], [0, 3], [0, 9])                                                  # (the well-formed call goes through)
    for frame_off, tok_off, bp_off in (([0, 9], [0, 2048], [0, 9 * 257]),         # S = 4097
                                       ([0, 9], [0, 3], [0, 8]),                  # scratch smaller than 9 x 1 words
                                       ([1, 9], [0, 3], [0, 9]), ([0, 9], [3, 3], [0, 9]), ([0, 0], [0, 3], [0, 9]),
                                       ([0, 9], [0, 0], [0, 9]), ([0, 9], [0, 3], [9, 0])):
        with pytest.raises(rg.capi.RgError):
            call(frame_off, tok_off, bp_off, words=9 * 257)
    torch.cuda.synchronize()


@pytest.mark.parametrize("T,L,kind", [(9, 4, "equal"), (120, 30, "mixed"), (700, 300, "mixed")])
def test_align_planted_path(rg, h, T, L, kind):
    """Per frame only the planted state's label scores 0, every other -4: the optimum is unique and is the planted path."""
    rng = np.random.default_rng(17 * T)
    y = fx.random_tokens(rng, L, V32, kind=kind)
    path, E = fx.planted_path(rng, T, y)
    got = _device_items(rg, h, [(E, y)])[0]
    assert got["status"] == 0 and got["score"] == 0.0 and np.array_equal(got["path"], path)
    for j in range(L):
        frames = np.nonzero(path == 2 * j + 1)[0]
        assert (got["tok_first"][j], got["tok_last"][j]) == (frames[0], frames[-1])
    # ... and the word timings it implies
    word_of = [j // 3 if j % 3 != 2 else -1 for j in range(L)]                     # words of two characters, a delimiter between
    words = ["w%d" % k for k in range((L + 2) // 3)]
    al = rg.align
    want = fx.word_times(words, word_of, [np.nonzero(path == 2 * j + 1)[0][0] for j in range(L)],
                         [np.nonzero(path == 2 * j + 1)[0][-1] for j in range(L)], np.arange(T) * 320, T * 320 + 80)
    assert al.word_times(words, word_of, got["tok_first"], got["tok_last"], np.arange(T) * 320, T * 320 + 80) == want


def test_align_float_emissions(rg, h, parity):
    T, L = 120, 30
    rng = np.random.default_rng(3)
    y = fx.random_tokens(rng, L, V32)
    logits = torch.from_numpy(rng.standard_normal((T, V32)).astype(np.float32) * 3.0).cuda()
    logp, _ = rg.align.log_softmax(h, logits)
    r = rg.align.viterbi(h, logp, [0, T], [y], fx.BLANK)
    torch.cuda.synchronize()
    E = logp.cpu().numpy()
    path = r["path"].cpu().numpy()
    assert r["status"].item() == 0 and fx.path_is_valid(path, y)
    ref = fx.viterbi(E.astype(np.float64), y)
    mine, best = fx.path_score(E, path, y), fx.path_score(E, ref["path"], y)
    bound = 2 * T * 2.0 ** -24 * max(abs(mine), abs(best))
    print("rg_ctc_align T=120 L=30 float emissions: |score - optimum| = %.3e, bound %.3e" % (abs(mine - best), bound))
    parity.check("rg_ctc_align T=120 L=30: fp64 score of the device path vs the fp64 optimum", abs(mine - best), bound)
    parity.check("rg_ctc_align T=120 L=30: the device's fp32 score vs the fp64 score of its path", abs(r["score"].item() - mine),
                 T * 2.0 ** -24 * abs(mine))
    first, last = r["tok_first"].cpu().numpy(), r["tok_last"].cpu().numpy()
    for j in range(L):
        frames = np.nonzero(path == 2 * j + 1)[0]
        assert (first[j], last[j]) == (frames[0], frames[-1])


def test_align_ragged_batch_equals_items_alone(rg, h):
    rng = np.random.default_rng(11)
    shapes = [(40, 12), (3, 1), (499, 150), (130, 65), (17, 8)]
    items = []
    for T, L in shapes:
        y = fx.random_tokens(rng, L, V32)
        items.append((np.asarray(fx.log_softmax(rng.standard_normal((T, V32)) * 2.0), np.float32), y))
    together = _device_items(rg, h, items)
    for i, it in enumerate(items):
        alone = _device_items(rg, h, [it])[0]
        assert _same(together[i], alone) and alone["status"] == 0 and fx.path_is_valid(alone["path"], it[1]), i


# ------------------------------------------------------------------------------------------------ word frames
D = 768
WINDOW_A = dict(frames=150, words=[([[0.0, 1.0], "one"], 1), ([[0.5, 2.0], "five"], 5), ([[3.0, 3.0], "none"], 2), ([[4.0, 4.5], "two"], 2),
                                   ([[9.5, 12.0], "past"], 3)])            # (segment, token rows): overlap, zero length, gap, past 150
WINDOW_B = dict(frames=37, words=[([[0.1, 0.3], "x"], 2), ([[0.2, 2.6], "y"], 1)])


def _word_frames_call(h, hidden, windows):
    """windows: list of dict(frames, words) whose token rows follow one another in `hidden`, a [CLS] row in front of and a [SEP]
    row behind every window's.  -> (device output rows per window, the fixture's arguments per window)."""
    tok, start, end, word_off, frame_off, args, r = [], [], [], [0], [0], [], 0
    for w in windows:
        r += 1                                                # [CLS]
        groups = []
        for seg, n in w["words"]:
            tok.append(r)
            s, e, _ = slice(int(seg[0][0] * 15), int(seg[0][1] * 15)).indices(w["frames"])
            start.append(s)
            end.append(e)
            groups.append(list(range(r, r + n)))
            r += n
        tok.append(r)                                         # [SEP] (and the next [CLS]): a word of no frames
        start.append(0)
        end.append(0)
        r += 1
        word_off.append(len(start))
        frame_off.append(frame_off[-1] + w["frames"])
        args.append((groups, [seg for seg, _ in w["words"]], w["frames"]))
    tok.append(r)
    assert r <= hidden.shape[0]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    n = len(windows)
    out = torch.full((frame_off[-1] + 2, D), float("nan"), device="cuda")
    h.call("word_frames", hidden, i32(tok), i32(start), i32(end), i32(word_off), (ctypes.c_int * (n + 1))(*word_off),
           torch.tensor(frame_off, dtype=torch.int64, device="cuda"), (ctypes.c_int64 * (n + 1))(*frame_off), n, D, out)
    torch.cuda.synchronize()
    assert torch.isnan(out[frame_off[-1]:]).all()             # frames beyond the windows are never written
    return [out[frame_off[j]:frame_off[j + 1]] for j in range(n)], args


def test_word_frames(rg, h, parity):
    torch.manual_seed(4)
    hidden = (torch.randn(40, D) * 3.0).cuda()
    (got_a, got_b), args = _word_frames_call(h, hidden, [WINDOW_A, WINDOW_B])
    host = hidden.cpu().numpy()
    worst = 0.0
    for got, (groups, segs, n_frames) in zip((got_a, got_b), args):
        ref, bound = fx.word_frames(host, groups, segs, n_frames), fx.word_frames_bound(host, groups, segs, n_frames)
        g = got.cpu().double().numpy()
        covered = bound.any(1)
        assert not g[~covered].any() and (~covered).any()                   # uncovered frames are exactly zero
        assert (np.abs(g - ref) <= bound).all()
        worst = max(worst, (np.abs(g - ref)[covered] / bound[covered]).max())
    print("rg_word_frames: worst |err| / (2^-23 sum |x_j|) = %.3f" % worst)
    parity.check("rg_word_frames: worst |mean - fp64| / (2^-23 sum_j |x_j|)", worst, 1.0)
    ga = got_a.cpu().numpy()
    assert np.array_equal(ga[7], ga[29]) and not np.array_equal(ga[0], ga[7])        # frames 7 .. 14: the later word won
    assert not ga[30:60].any() and ga[60:67].any() and not ga[67:142].any() and ga[142:].all()
    # each window alone: the same bits (window B's rows then start at row 0 of the tensor handed in)
    (alone_a,), _ = _word_frames_call(h, hidden, [WINDOW_A])
    (alone_b,), _ = _word_frames_call(h, hidden[15:].contiguous(), [WINDOW_B])
    assert torch.equal(_bits(alone_a), _bits(got_a)) and torch.equal(_bits(alone_b), _bits(got_b))
    with pytest.raises(rg.capi.RgError):
        h.call("word_frames", hidden, got_a, got_a, got_a, got_a, (ctypes.c_int * 2)(1, 1), got_a, (ctypes.c_int64 * 2)(0, 5), 1, D, got_a)


# ------------------------------------------------------------------------------------------------ the public interface
@pytest.fixture(scope="module")
def models():
    """Random-initialised encoders as tests/test_features_batch_gpu.py builds its own, and a random CTC head."""
    import transformers
    torch.manual_seed(2)
    bert = transformers.BertModel(transformers.BertConfig(vocab_size=500, num_hidden_layers=4), add_pooling_layer=False).eval()
    torch.manual_seed(1)
    w2v = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(num_hidden_layers=2)).eval()
    g = torch.Generator().manual_seed(6)
    return bert, w2v, torch.randn(V32, 768, generator=g) * 0.5, torch.randn(V32, generator=g) * 0.1


def _tokenizer():
    vocab = {}

    def tok(sentence):                                        # a word of k letters is ceil(k / 3) pieces: some words have several
        ids = [101]
        for w in sentence.split():
            for p in range(0, len(w), 3):
                ids.append(vocab.setdefault(w[p:p + 3] if p == 0 else "##" + w[p:p + 3], 110 + len(vocab)))
        return ids + [102]
    return tok


@pytest.fixture(scope="module")
def feats(rg, models):
    bert, w2v, lm_w, lm_b = models
    state = {"wav2vec2." + k: v for k, v in w2v.state_dict().items()}
    state.update({"lm_head.weight": lm_w, "lm_head.bias": lm_b})
    aligner = rg.align.CTCAligner.from_state(state, fx.VOCAB)
    bf, tok = rg.features.BertFeatures(bert.state_dict()), _tokenizer()
    on = rg.features.WindowFeatures(bf, aligner.w2v, tok, frame_words=True, aligner=aligner)
    off = rg.features.WindowFeatures(bf, aligner.w2v, tok, aligner=aligner)
    return aligner, on, off, tok


def _check_word(rg, res, segs, tok, n_frames):
    merged = rg.features.merge_disco_textsegs(segs)
    woff = rg.features.BertFeatures.word_rows([s[1] for s in merged], tok)
    groups = [list(range(woff[k], woff[k + 1])) for k in range(len(merged))]
    host = res["text_features"][0].cpu().numpy()
    ref, bound = fx.word_frames(host, groups, merged, n_frames), fx.word_frames_bound(host, groups, merged, n_frames)
    got = res["word"][0].cpu().double().numpy()
    assert res["word"].shape == (1, n_frames, 768) and (np.abs(got - ref) <= bound).all()
    assert not got[~bound.any(1)].any()


def test_window_features_frame_words(rg, feats):
    aligner, on, off, tok = feats
    torch.manual_seed(8)
    raw = torch.randn(1, 16000 * 19) * 0.1
    segs = [[[0.5, 0.9], "so"], [[0.5, 0.9], "me"], [[1.2, 1.8], "bigger"], [[2.0, 9.5], "houses"]]
    reqs = [(raw, 9.0, 19.0, "well that’s 42 remarkable"), (raw, 0.0, 10.0, segs), (raw, 9.0, 19.0, [])]
    got, plain = on.windows(reqs), off.windows(reqs)
    torch.cuda.synchronize()
    for g, p in zip(got, plain):
        assert sorted(set(g) - set(p)) == ["word"] and g["raw_word"] == p["raw_word"]
        assert torch.equal(_bits(g["audio"]), _bits(p["audio"]))
        assert torch.equal(_bits(g["text_features"][0]), _bits(p["text_features"][0]))
    timed = got[0]["text_segments"][0]
    assert [s[1] for s in timed] == "well that’s 42 remarkable".split() and "text_segments" not in got[1]
    assert timed == plain[0]["text_segments"][0] == aligner.align(got[0]["audio"], ["well that’s 42 remarkable"], n_samples=[160000])[0]
    flat = [t for s in timed for t in s[0]]
    assert flat == sorted(flat) and flat[0] >= 0.0 and flat[-1] <= 10.0 and timed[2][0] == [timed[1][0][1], timed[3][0][0]]
    _check_word(rg, got[0], timed, tok, 150)
    _check_word(rg, got[1], segs, tok, 150)
    assert got[1]["raw_word"] == ["some bigger houses"] and got[1]["word"][0, 30:142].all() and not got[1]["word"][0, 142:].any()
    assert got[2]["word"].shape == (1, 150, 768) and not got[2]["word"].any()
    # window(...) answers as windows([...]) does, request by request (the same launches on one window: the same bits)
    for r, g in zip(reqs, got):
        one, again = on.window(*r), on.windows([r])[0]
        assert sorted(one) == sorted(g) and one["raw_word"] == g["raw_word"]
        for key in ("audio", "word"):
            assert torch.equal(_bits(one[key]), _bits(again[key]))
        assert torch.equal(_bits(one["text_features"][0]), _bits(again["text_features"][0]))
        assert one.get("text_segments") == again.get("text_segments")
    with pytest.raises(rg.capi.RgError):
        rg.features.WindowFeatures(on.bert, on.w2v, tok, frame_words=True).windows(reqs[:1])      # a bare transcript, no aligner


def test_dataset_samples_carry_word(rg, feats):
    _, on, _, _ = feats
    dsf = _load("dataset_fixture")
    recs = [r for r in dsf.recordings() if r["poses"].shape[0] >= 301]
    model = {k: v for k, v in dsf.smplx_model().items() if k not in ("f", "weights", "posedirs")}
    pre = rg.dataset.ClipPreprocessor(model, pose_fps=dsf.POSE_FPS)
    ann = dict(text_segments=[[[1.3 * k, 1.3 * k + 0.4], w] for k, w in enumerate("so i went there and it was big".split())],
               discourse=[], prominence=[], gesture_labels=[])
    clips = [rg.dataset.RawClip(r["name"], r["poses"], r["trans"], r["expressions"], r["betas"], 3, annotations=ann) for r in recs]
    g = torch.Generator().manual_seed(9)
    raws = {c.name: torch.randn(1, 16000 * (c.n_raw // 30), generator=g) * 0.1 for c in clips}
    ds = rg.dataset.SMPLXClipDataset(clips, pre, features=on.for_clips(raws), pose_length=150, stride=5)
    assert len(ds) >= 2
    for k in range(len(ds)):
        s = ds[k]
        assert s["word"].shape == (150, 768) and s["audio"].shape == (499, 768)
        if not s["text_segments"]:
            assert not s["word"].any()
            continue
        f0, f1 = (int(s["text_segments"][0][0][i] * 15) for i in (0, 1))
        assert f1 > f0 and s["word"][f0:f1].all() and not s["word"][:f0].any()
    batch = ds.collate([0, len(ds) - 1])
    assert batch["word"].shape == (2, 150, 768) and torch.equal(batch["word"][1], ds[len(ds) - 1]["word"])


def test_align_recording(rg, feats):
    aligner = feats[0]
    n = 25 * 16000 - 7
    g = torch.Generator().manual_seed(12)
    wave = torch.randn(n, generator=g) * 0.1
    words = "so i went there and it was really big 42".split()
    segs, fs = aligner.align_recording(wave, " ".join(words), return_frames=True)
    keep, fs2 = aligner.recording_frames(n, 160000)
    assert keep == [499, 499, 249] and np.array_equal(fs, fs2) and len(fs) == 1247          # three chunks, the last one padded
    assert np.array_equal(fs, np.concatenate([c * 160000 + 320 * np.arange(k) for c, k in enumerate(keep)]))
    assert fs[-1] + 400 <= n < fs[-1] + 400 + 320                                          # the frames a 9.9996 s tail has
    assert [s[1] for s in segs] == words
    flat = [t for s in segs for t in s[0]]
    assert flat == sorted(flat) and flat[0] >= 0.0
    assert segs[-1][0][1] == n / 16000 and all(s[0][1] <= n / 16000 for s in segs)          # the clamp to the recording's length
    assert aligner.recording_frames(160000 + 399, 160000)[0] == [499, 0] and aligner.recording_frames(320000, 160000)[0] == [499, 499]
    tr = aligner.transcribe(aligner.w2v.batch(wave[:160000][None]))
    assert len(tr) == 1 and all(s[0][0] < s[0][1] <= 10.0 and s[1] for s in tr[0])
    flat = [t for s in tr[0] for t in s[0]]
    assert flat == sorted(flat)
