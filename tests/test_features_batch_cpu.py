"""CPU: the host side of the many-windows-per-call feature path (features.conv_layout, WindowFeatures.windows and its
adapters, the dataset's and the long-form driver's use of a batched `features` object).  No kernel runs here."""
import math

import pytest
import torch


KERNELS, STRIDES = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)


def _hf_lengths(n):
    """Wav2Vec2Model._get_feat_extract_output_lengths layer by layer (transformers modeling_wav2vec2.py: floor((L - k) / s) + 1);
    checked against the library itself where it is installed."""
    out = []
    for k, s in zip(KERNELS, STRIDES):
        n = (n - k) // s + 1
        out.append(n)
    return out


@pytest.mark.parametrize("n", [400, 16000, 16150, 159999, 160000, 160001])
def test_conv_layout(rg, n):
    lay = rg.features.conv_layout(n, KERNELS, STRIDES)
    assert lay == rg.features.conv_layout(n) and lay.n == n
    assert list(lay.T) == _hf_lengths(n)
    try:
        import transformers
    except ImportError:
        transformers = None
    if transformers is not None:
        m = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(num_hidden_layers=0))
        assert int(m._get_feat_extract_output_lengths(n)) == lay.T[-1]
    assert lay.n_pad % 320 == 0 and 0 <= lay.n_pad - n < 320 and lay.n_pad == STRIDES[0] * lay.T_pad[0]
    for i in range(7):
        assert lay.T_pad[i] >= lay.T[i] >= 1
        if i:
            assert lay.T_pad[i - 1] == STRIDES[i] * lay.T_pad[i]
    # the last element a VALID row reads, layer by layer down to the samples: inside the window's own valid rows / n samples
    for i in range(6, -1, -1):
        last = (lay.T[i] - 1) * STRIDES[i] + KERNELS[i] - 1          # row of layer i - 1 (sample for i = 0)
        assert last <= (lay.T[i - 1] if i else n) - 1
    # ... and row b * T_pad + t starts where window b's row t * stride of the previous layer starts
    for i in range(1, 7):
        for b, t in ((0, 0), (1, 0), (2, lay.T[i] - 1)):
            assert (b * lay.T_pad[i] + t) * STRIDES[i] == b * lay.T_pad[i - 1] + t * STRIDES[i]
    if n == 160000:
        assert lay.n_pad == n and lay.T_pad == (32000, 16000, 8000, 4000, 2000, 1000, 500) and lay.T[-1] == 499


def test_conv_layout_refuses_too_few_samples(rg):
    with pytest.raises(rg.capi.RgError):
        rg.features.conv_layout(399)
    with pytest.raises(rg.capi.RgError):
        rg.features.conv_layout(1000, (10, 3), (5,))


class _StubW2V:
    def __init__(self):
        self.calls, self.single = [], []

    def batch(self, waves, normalize=True, chunk=None):
        self.calls.append((waves.clone(), chunk))
        return waves[:, :499, None].expand(-1, -1, 768) + 0.0        # recognisable per window

    def __call__(self, wave):
        self.single.append(wave.clone())
        return wave[:499, None].expand(-1, 768) + 0.0


class _StubBert:
    def __init__(self):
        self.calls, self.single = [], []

    def batch(self, list_of_ids, layers=(-4, -3, -2, -1)):
        self.calls.append([i.clone() for i in list_of_ids])
        return [i.float()[:, None].expand(-1, 768) + 0.0 for i in list_of_ids]

    def __call__(self, ids):
        self.single.append(ids.clone())
        return ids.float()[:, None].expand(-1, 768) + 0.0


def _window_features(rg):
    vocab = {}
    tok = lambda sentence: [101] + [vocab.setdefault(w, 110 + len(vocab)) for w in sentence.split()] + [102]
    w2v, bert = _StubW2V(), _StubBert()
    return rg.features.WindowFeatures(bert, w2v, tok, sample_rate=1000), w2v, bert


SEGS = [[[9.5, 9.9], "so"], [[9.5, 9.9], "me"], [[10.2, 10.8], "big"], [[11.0, 11.5], "house"]]


def test_windows_requests_equal_window(rg):
    """Slicing, tail padding and tokenisation of `windows` are `window`'s; one batch call of each encoder per chunk."""
    wf, w2v, bert = _window_features(rg)
    torch.manual_seed(3)
    raw = torch.randn(1, 1000 * 19)
    reqs = [(raw, 9.0, 19.0, SEGS), (raw, 18.0, 28.0, []), (raw, 0.0, 10.0, SEGS[2:]), (raw, 12.5, 22.5, SEGS[:1]), (raw, 1.0, 11.0, [])]
    got = wf.windows(reqs, chunk=2)
    assert len(got) == 5 and len(w2v.calls) == len(bert.calls) == 3            # ceil(5 / 2) chunks, one call each per chunk
    assert [c[0].shape[0] for c in w2v.calls] == [2, 2, 1] and [len(c) for c in bert.calls] == [2, 2, 1]
    assert all(c[1] == c[0].shape[0] for c in w2v.calls)                       # the audio encoder does not split a chunk again
    assert not w2v.single and not bert.single
    want = [wf.window(*r) for r in reqs]
    waves = torch.cat([c[0] for c in w2v.calls])
    ids = [i for c in bert.calls for i in c]
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(waves[i], w2v.single[i]) and torch.equal(ids[i], bert.single[i]), i
        assert sorted(g) == sorted(w) == ["audio", "raw_word", "text_features"]
        assert g["raw_word"] == w["raw_word"] and g["audio"].shape == w["audio"].shape == (1, 499, 768)
        assert torch.equal(g["audio"], w["audio"]) and len(g["text_features"]) == 1
        assert torch.equal(g["text_features"][0], w["text_features"][0])
    assert got[0]["raw_word"] == ["some big house"] and ids[0].tolist() == [101, 110, 111, 112, 102]
    assert torch.equal(waves[1][:1000], raw[0, 18000:]) and not waves[1][1000:].any()   # the padded tail of the last window
    assert got[1]["raw_word"] == [""] and ids[1].tolist() == [101, 102]                  # empty transcript: [CLS] [SEP]
    assert ids[1].dtype == torch.long
    # default chunk without an audio encoder that states one: everything in one call
    wf2, w2v2, bert2 = _window_features(rg)
    assert len(wf2.windows(reqs)) == 5 and len(w2v2.calls) == len(bert2.calls) == 1
    assert wf2.windows([]) == [] and len(w2v2.calls) == 1


def test_windows_groups_requests_by_length(rg):
    """Windows of different sample counts in one call (a clip's whole span; a start time whose sample index truncates the other
    way): one pair of batch calls per length and chunk, the answers in request order and equal to `window`'s."""
    wf, w2v, bert = _window_features(rg)
    torch.manual_seed(4)
    raw = torch.randn(1, 1000 * 30)
    spans = [(0.0, 10.0), (0.0, 9.0), (2.0, 12.0), (1.0, 10.0), (3.0, 13.0), (0.0, 10.001), (4.0, 14.0)]
    reqs = [(raw, t0, t1, SEGS[i % 3:]) for i, (t0, t1) in enumerate(spans)]
    got = wf.windows(reqs, chunk=3)
    assert [tuple(c[0].shape) for c in w2v.calls] == [(3, 10000), (1, 10000), (2, 9000), (1, 10001)]
    assert [len(c) for c in bert.calls] == [3, 1, 2, 1]
    want = [wf.window(*r) for r in reqs]
    for g, w in zip(got, want):
        assert g["raw_word"] == w["raw_word"] and torch.equal(g["audio"], w["audio"])
        assert torch.equal(g["text_features"][0], w["text_features"][0])


def test_for_clips_adapter(rg):
    """for_clips: callable both ways (dataset: 4 arguments, run_many: 5), and the batched form under both names."""
    wf, w2v, bert = _window_features(rg)
    raws = {"a": torch.randn(1, 12000), "b": torch.randn(1, 15000)}
    ann = dict(text_segments=[SEGS[2:]])
    f = wf.for_clips(raws)
    one = f("b", 2.0, 12.0, ann)
    assert torch.equal(one["audio"], wf.window(raws["b"], 2.0, 12.0, SEGS[2:])["audio"]) and one["raw_word"] == ["big house"]
    assert f.windows.__func__ is f.batch.__func__
    n = len(w2v.calls)
    got = f.windows([("a", 0.0, 10.0, ann), ("b", 2.0, 12.0, ann)])
    assert len(w2v.calls) == n + 1 and len(got) == 2 and torch.equal(got[1]["audio"], one["audio"])
    g = wf.for_clips([raws["a"], raws["b"]])
    five = g(1, 0, 2.0, 12.0, ann)
    assert torch.equal(five["audio"], one["audio"])
    got = g.batch([(0, 1, 0.0, 10.0, ann), (1, 1, 2.0, 12.0, ann)])
    assert len(got) == 2 and torch.equal(got[1]["audio"], one["audio"]) and got[0]["audio"].shape == (1, 499, 768)


class _Pre:
    """What SMPLXClipDataset needs of a preprocessor to lay out its windows (nothing is prepared in this test)."""
    pose_fps = 15
    device = "cpu"

    def strided_frames(self, n_raw):
        return (n_raw + 1) // 2


def test_dataset_asks_for_feature_batches(rg):
    """A `features` object with `windows` gets ceil(n_windows / feature_batch) calls with the arguments of the per-window
    callable, and the dataset's samples hold the same values; a plain callable is still called once per window."""
    import numpy as np
    ds_mod = rg.dataset
    segs = [[[0.5 * k, 0.5 * k + 0.4], w] for k, w in enumerate("so i went there and it was big".split())]
    clips = [ds_mod.RawClip("c%d" % i, np.zeros((n, 165), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 100), np.float32),
                            np.zeros(300, np.float32), 0, annotations=dict(text_segments=segs, discourse=[], prominence=[], gesture_labels=[]))
             for i, n in enumerate((301, 331))]

    def single(name, t0, t1, ann):
        calls.append((name, t0, t1))
        v = float(len(name) + t0)
        return dict(audio=torch.full((1, 499, 768), v), text_features=[torch.full((len(ann["text_segments"][0]) + 2, 768), v)],
                    raw_word=["ignored"])

    class Batched:
        def __init__(self):
            self.calls = []

        def __call__(self, *a):
            raise AssertionError("the batched form must be used")

        def windows(self, requests):
            self.calls.append(len(requests))
            keep, out = list(calls), [single(*r) for r in requests]
            calls[:] = keep
            return out

    calls = []
    want = ds_mod.SMPLXClipDataset(clips, _Pre(), features=single, pose_length=150, stride=5)
    n = len(want)
    assert n == 5 and len(calls) == n
    for fb, n_calls in ((2, [2, 2, 1]), (5, [5]), (32, [5])):
        b = Batched()
        got = ds_mod.SMPLXClipDataset(clips, _Pre(), features=b, pose_length=150, stride=5, feature_batch=fb)
        assert b.calls == n_calls and len(b.calls) == math.ceil(n / fb)
        for k in range(n):
            assert sorted(got._side[k]) == sorted(want._side[k])
            assert torch.equal(got._side[k]["audio"], want._side[k]["audio"]) and got._side[k]["audio"].shape == (499, 768)
            assert torch.equal(got._side[k]["text_feature"], want._side[k]["text_feature"])
            assert got._side[k]["raw_word"] == want._side[k]["raw_word"] != "ignored"
            assert torch.equal(got.retrieval_samples[k]["text_feature"], want.retrieval_samples[k]["text_feature"])
    assert ds_mod.SMPLXClipDataset(clips, _Pre(), pose_length=150, stride=5).feature_batch == 32
    with pytest.raises(ValueError):
        ds_mod.SMPLXClipDataset(clips, _Pre(), features=Batched(), pose_length=150, stride=5, feature_batch=0)


def _recording_features(rg, sr=1000):
    """for_clips over stub encoders (1 kHz audio unless stated, so that the stub's 499 'frames' exist), and its per-window twin."""
    wf, w2v, bert = _window_features(rg)
    wf.sr = sr
    g = torch.Generator().manual_seed(6)
    raws = {"c0": torch.randn(1, sr * 12, generator=g), "c1": torch.randn(1, sr * 14, generator=g)}
    return wf, w2v, wf.for_clips(raws), (lambda name, t0, t1, ann: wf.window(raws[name], t0, t1, ann["text_segments"][0]))


def _zero_clips(rg, lengths):
    import numpy as np
    segs = [[[0.5 * k, 0.5 * k + 0.4], w] for k, w in enumerate("so i went there and it was big".split())]
    return [rg.dataset.RawClip("c%d" % i, np.zeros((n, 165), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 100), np.float32),
                               np.zeros(300, np.float32), 0, annotations=dict(text_segments=segs, discourse=[], prominence=[], gesture_labels=[]))
            for i, n in enumerate(lengths)]


def _same_sides(got, want):
    assert len(got) == len(want)
    for k in range(len(want)):
        assert torch.equal(got._side[k]["audio"], want._side[k]["audio"]), k
        assert torch.equal(got._side[k]["text_feature"], want._side[k]["text_feature"]), k


def test_dataset_full_mode_with_clips_of_different_length(rg):
    """mode="full": one window per clip over its whole span, so two clips give windows of two lengths.  The batched features
    object answers them (one group per length) with what the per-window callable gives."""
    wf, w2v, batched, single = _recording_features(rg)
    clips = _zero_clips(rg, (331, 391))                                   # 166 and 196 frames at 15 fps
    want = rg.dataset.SMPLXClipDataset(clips, _Pre(), features=single, mode="full")
    n_single = len(w2v.single)
    got = rg.dataset.SMPLXClipDataset(clips, _Pre(), features=batched, mode="full")
    assert len(got) == 2 and len(w2v.single) == n_single
    lengths = [c[0].shape[1] for c in w2v.calls]
    assert len(lengths) == 2 and lengths[0] != lengths[1]
    _same_sides(got, want)
    # feature_batch=None: the same object, window by window
    n_calls = len(w2v.calls)
    again = rg.dataset.SMPLXClipDataset(clips, _Pre(), features=batched, mode="full", feature_batch=None)
    assert len(w2v.calls) == n_calls and len(w2v.single) == n_single + 2
    _same_sides(again, want)


def test_dataset_stride_one_windows_of_truncated_lengths(rg):
    """stride=1 at 15 fps: window starts at every 1/15 s.  int(t1 * sr) - int(t0 * sr) is not the same for all of them at every
    sample rate and start (floating point: at 22.05 kHz the starts 3 / 15 s, 18 / 15 s, ... give 220499 samples); whatever the lengths are, the batched construction equals the per-window
    one and makes one batch call per (length, chunk)."""
    wf, w2v, batched, single = _recording_features(rg, sr=22050)         # a rate at which the truncation differs within 16 windows
    clips = _zero_clips(rg, (331, 391))
    want = rg.dataset.SMPLXClipDataset(clips, _Pre(), features=single, pose_length=150, stride=1)
    got = rg.dataset.SMPLXClipDataset(clips, _Pre(), features=batched, pose_length=150, stride=1, feature_batch=8)
    assert len(got) == 16 + 46
    lengths = {int(w.numel()) for w in w2v.single}
    assert len(lengths) > 1, lengths                                    # the case is really there
    assert sum(c[0].shape[0] for c in w2v.calls) == len(got)
    _same_sides(got, want)
