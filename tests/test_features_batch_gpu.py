"""GPU: conditioning features of MANY windows per call (features.Wav2Vec2Features.batch, BertFeatures.batch,
WindowFeatures.windows and their users in dataset.py / longform.py).
  kernels, one by one through the C ABI, against fp64 NumPy / torch references: rg_wave_normalize,
    rg_time_groupnorm_gelu_batched, rg_im2col_grouped_batched, rg_mha_bf16_ragged (bounds: tests/kernel_refs.py);
  the two encoders against the Hugging Face implementations (random-initialised, fp32 on the host), with the bounds of
    tests/test_features_gpu.py;
  no leakage between the windows of a batch (bit-identical outputs of the untouched windows);
  batched against the single-window path."""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu
transformers = pytest.importorskip("transformers")

HERE = os.path.dirname(os.path.abspath(__file__))


def relerr(a, b):
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def h(rg):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return rg.capi.get_handle(0)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


# ------------------------------------------------------------------------------------------------ kernels
def test_wave_normalize(rg, h, parity):
    """B = 3, n = 16150 (n_pad = 16320), row stride n + 7; means and deviations up to 0.2; window 2 is constant (variance 0:
    the formula gives 0 / sqrt(1e-7) = 0).  Bound 1e-6 relative (Frobenius): the mean and the variance are fp32 sums whose
    relative error is far below one rounding per element here (partial sums of 16 values, then a tree), and an element takes
    a subtraction, a division and the rounding of sqrt: about six roundings of 6e-8, of which the subtraction's counts in
    units of |x| / |x - mean| ~ 1.4 at mean = deviation."""
    B, n, n_pad, ldx = 3, 16150, 16320, 16157
    g = kr.rng(5)
    x = np.zeros((B, ldx), np.float32)
    x[0, :n] = (g.standard_normal(n) * 0.2 + 0.2).astype(np.float32)
    x[1, :n] = (g.standard_normal(n) * 0.05 - 0.1).astype(np.float32)
    x[2, :n] = np.float32(0.1)
    x[:, n:] = 1e30                                                     # behind the window: must not be read into it
    xd = x[:, :n].astype(np.float64)
    ref = (xd - xd.mean(1, keepdims=True)) / np.sqrt(xd.var(1, keepdims=True) + 1e-7)
    before = kr.canary(1, B * n_pad + 16)
    for normalize in (1, 0):
        o = before.cuda()
        h.call("wave_normalize", torch.from_numpy(x).cuda(), ldx, o, B, n, n_pad, normalize)
        torch.cuda.synchronize()
        oc = o.cpu()[0]
        assert torch.isnan(oc[B * n_pad:]).all()                          # nothing written behind the last window
        got = oc[:B * n_pad].view(B, n_pad)
        assert torch.isfinite(got).all() and not got[:, n:].any()         # padding exactly zero
        if not normalize:
            assert torch.equal(got[:, :n], torch.from_numpy(x[:, :n]))
            continue
        e = np.linalg.norm(got[:, :n].double().numpy() - ref) / np.linalg.norm(ref)
        parity.check("rg_wave_normalize B=3 n=16150: relative Frobenius error vs fp64", e, 1e-6)
        parity.check("rg_wave_normalize: constant window, max |out| (the formula gives 0)", got[2].abs().max().item(), 1e-6)
    with pytest.raises(rg.capi.RgError):
        h.call("wave_normalize", o, ldx, o, B, n, n - 1, 1)


def _gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def test_time_groupnorm_gelu_batched(rg, h, parity):
    """B = 3, T = 49 of T_pad = 50 rows, C = 512, junk rows = 1e30: statistics over t < T only, junk rows of the output zero.
    The single kernel has no test or stated bound: fp32 against fp64 at 1e-5 relative.  The bf16 output is the rounding of the
    fp32 one."""
    B, T, T_pad, C, eps = 3, 49, 50, 512, 1e-5
    x = kr.randn((B, T_pad, C), 11) * (0.5 + kr.randn((1, 1, C), 12).abs()) + 3.0 * kr.randn((B, 1, C), 13)
    x[:, T:] = 1e30
    gam, bet = 1 + 0.2 * kr.randn((C,), 14), 0.2 * kr.randn((C,), 15)
    xd = x[:, :T].double()
    mean, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    ref = _gelu64((xd - mean) / torch.sqrt(var + eps) * gam.double() + bet.double())
    b32, b16 = kr.canary(1, B * T_pad * C + 8), kr.canary(1, B * T_pad * C + 8, torch.int16)
    o32, o16, ws = b32.cuda(), b16.cuda(), torch.full((2 * B * C + 4,), float("nan"), device="cuda")
    h.call("time_groupnorm_gelu_batched", x.cuda(), gam.cuda(), bet.cuda(), o16, o32, B, T, T_pad, C, eps, ws)
    torch.cuda.synchronize()
    got, got16 = o32.cpu()[0], o16.cpu()[0]
    assert torch.isnan(got[B * T_pad * C:]).all() and torch.equal(got16[B * T_pad * C:], b16[0, B * T_pad * C:])
    assert torch.isnan(ws[2 * B * C:]).all() and torch.isfinite(ws[:2 * B * C]).all()
    got, got16 = got[:B * T_pad * C].view(B, T_pad, C), got16[:B * T_pad * C].view(B, T_pad, C)
    assert torch.isfinite(got).all() and not got[:, T:].any() and not got16[:, T:].any()
    parity.check("rg_time_groupnorm_gelu_batched B=3 T=49/50 C=512: relative Frobenius error vs fp64", relerr(got[:, :T].double(), ref), 1e-5)
    assert torch.equal(got16, kr.bf16_bits(got))
    # only one of the two outputs
    o32b = b32.cuda()
    h.call("time_groupnorm_gelu_batched", x.cuda(), gam.cuda(), bet.cuda(), None, o32b, B, T, T_pad, C, eps, ws)
    torch.cuda.synchronize()
    assert torch.equal(_bits(o32b.cpu()), _bits(o32.cpu()))
    for bad in ((B, T_pad + 1, T_pad, C), (B, T, T_pad, C + 2)):
        with pytest.raises(rg.capi.RgError):
            h.call("time_groupnorm_gelu_batched", x.cuda(), gam.cuda(), bet.cuda(), None, o32b, *bad, eps, ws)


def test_im2col_grouped_batched(rg, h):
    """B = 3, T = 49, the positional convolution's shape (C = 768, 16 groups, k = 128, padding 64): bit-exact against a NumPy
    gather of the bf16-rounded rows (the kernel only rounds), zero at both edges of EVERY window."""
    B, T, C, G, K, pad = 3, 49, 768, 16, 128, 64
    Cg = C // G
    x = kr.randn((B * T, C), 21)
    xb = kr.bf16_bits(x).numpy().reshape(B, T, G, Cg)
    padded = np.zeros((B, T + 2 * pad, G, Cg), np.int16)
    padded[:, pad:pad + T] = xb
    idx = np.arange(T)[:, None] + np.arange(K)[None, :]                                   # [T, K] rows of the padded window
    ref = padded[:, idx].transpose(3, 0, 1, 2, 4).reshape(G, B * T, K * Cg)              # [B, T, K, G, Cg] -> [G, B * T, K * Cg]
    n = G * B * T * K * Cg
    before = kr.canary(1, n + 8, torch.int16)
    o = before.cuda()
    h.call("im2col_grouped_batched", x.cuda(), o, B, T, C, G, K, pad)
    torch.cuda.synchronize()
    oc = o.cpu()[0]
    assert torch.equal(oc[n:], before[0, n:])
    got = oc[:n].numpy().reshape(G, B * T, K * Cg)
    assert np.array_equal(got, ref)
    g5 = got.reshape(G, B, T, K, Cg)
    for t in (0, 1, T - 1):        # row t reads window rows t + k - 64: nothing below 0 or from T on, whatever the neighbours hold
        assert not g5[:, :, t, :pad - t].any() and not g5[:, :, t, pad - t + T:].any()
        assert g5[:, :, t, pad - t:pad - t + T].any()
    with pytest.raises(rg.capi.RgError):
        h.call("im2col_grouped_batched", x.cuda(), o, B, T, C, 128, K, pad)               # 6 channels per group: not a multiple of 4


def _ragged_case(h, lengths, out_bf16, seed):
    H, hd = 12, 64
    D = H * hd
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    rows, ld, ldo = int(off[-1]), 3 * D + 8, D + 8
    x = kr.randn((rows + 3, ld), seed)
    xd = x.cuda()
    before = kr.canary(rows + 3, ldo, torch.int16 if out_bf16 else torch.float32)
    o = before.cuda()
    off_host = (ctypes.c_int * len(off))(*off.tolist())
    h.call("mha_bf16_ragged", xd.data_ptr(), ld, xd.data_ptr() + 4 * D, ld, xd.data_ptr() + 8 * D, ld, o, ldo, int(out_bf16),
           torch.from_numpy(off).cuda(), off_host, len(lengths), H, hd)
    torch.cuda.synchronize()
    oc = o.cpu()
    assert kr.untouched(oc, before, rows, 0, D), (lengths, out_bf16)       # rows outside every sequence and the pad columns
    worst = 0.0
    for s, L in enumerate(lengths):
        r0 = int(off[s])
        q, k, v = x[r0:r0 + L, :D], x[r0:r0 + L, D:2 * D], x[r0:r0 + L, 2 * D:3 * D]
        ref, e = kr.mha_ref(q, k, v, 1, H, L, L, hd, True)
        got = kr.from_bf16_bits(oc[r0:r0 + L, :D]) if out_bf16 else oc[r0:r0 + L, :D]
        bound, b_ulp = kr.bf16_bounds(ref, e) if out_bf16 else (e, e)
        assert kr.worst_ratio(got, ref, b_ulp) <= 1.0, (lengths, s, out_bf16)
        worst = max(worst, kr.worst_ratio(got, ref, bound))
    return worst


@pytest.mark.parametrize("out_bf16", [False, True])
def test_mha_bf16_ragged(rg, h, parity, out_bf16):
    """Lengths across the 16-row wave tile, the 64-row workgroup tile and the 32-key padding, in one launch; a second launch
    with a 300-row sequence takes the 512-key instantiation.  Against fp64 softmax attention on bf16-rounded K and V with
    rg_mha_bf16's own bound (kernel_refs.mha_ref)."""
    tag = "bf16" if out_bf16 else "fp32"
    r = _ragged_case(h, (2, 9, 33, 64, 65, 191), out_bf16, 31)
    parity.check("rg_mha_bf16_ragged hd=64 H=12 lengths (2, 9, 33, 64, 65, 191), %s out: worst |err| / bound" % tag, r, 1.0)
    r = _ragged_case(h, (17, 300), out_bf16, 32)
    parity.check("rg_mha_bf16_ragged hd=64 H=12 lengths (17, 300) (512-key variant), %s out: worst |err| / bound" % tag, r, 1.0)


def test_ragged_offset_tables_are_checked(rg, h):
    D = 768
    x, o = torch.zeros(16, 3 * D, device="cuda"), torch.zeros(16, D, device="cuda")
    ids, w = torch.zeros(16, dtype=torch.long, device="cuda"), torch.zeros(8, D, device="cuda")
    for off, hd in (((1, 4, 8), 64), ((0, 5, 3), 64), ((0, 4, 8), 48), ((0, 0, 0), 64)):
        off_host, off_dev = (ctypes.c_int * 3)(*off), torch.tensor(off, dtype=torch.int32, device="cuda")
        with pytest.raises(rg.capi.RgError):
            h.call("mha_bf16_ragged", x, 3 * D, x, 3 * D, x, 3 * D, o, D, 0, off_dev, off_host, 2, 12, hd)
    for off, max_pos in (((1, 4, 8), 8), ((0, 5, 3), 8), ((0, 4, 8), 3)):
        off_host, off_dev = (ctypes.c_int * 3)(*off), torch.tensor(off, dtype=torch.int32, device="cuda")
        with pytest.raises(rg.capi.RgError):
            h.call("embed_sum3_ragged", ids, w, w, w[0], o, off_dev, off_host, 2, D, max_pos)


# ------------------------------------------------------------------------------------------------ BERT
def _bert_ids(lengths, seed, vocab):
    g = torch.Generator().manual_seed(seed)
    out = []
    for L in lengths:
        ids = torch.randint(min(1000, vocab // 2), vocab, (L,), generator=g)
        ids[0], ids[-1] = 101, 102
        out.append(ids)
    return out


def test_bert_batch_full_shape(rg, parity):
    """bert-base-cased shape, lengths (2, 9, 47, 65) in one call, both precisions: every sequence against transformers and
    against the single-sequence path (same bounds; not bit-equality: the GEMM variant may depend on the row count)."""
    torch.manual_seed(0)
    model = transformers.BertModel(transformers.BertConfig(vocab_size=28996), add_pooling_layer=False).eval()
    ids = _bert_ids((2, 9, 47, 65), 1, 28996)
    refs = []
    with torch.no_grad():
        for i in ids:
            hs = model(input_ids=i[None], output_hidden_states=True).hidden_states
            refs.append((hs[0][0], torch.stack([hs[j] for j in (-4, -3, -2, -1)]).sum(0)[0]))
    for precision, tol in (("fp32", 1e-4), ("bf16", 2e-2)):
        feats = rg.features.BertFeatures(model.state_dict(), device="cuda", precision=precision)
        got = feats.batch(ids)
        st, off = feats.hidden_states_batch(ids)
        torch.cuda.synchronize()
        assert len(got) == 4 and len(st) == 13 and off == [0, 2, 11, 58, 123]
        for s, (i, (ref0, ref)) in enumerate(zip(ids, refs)):          # the order given
            assert got[s].shape == (i.numel(), 768)
            tag = "BERT-base batch, L=%d %s" % (i.numel(), precision)
            parity.check(tag + ": embeddings vs transformers", relerr(st[0][off[s]:off[s + 1]].cpu(), ref0), 1e-5)
            parity.check(tag + ": sum of the last four layers vs transformers", relerr(got[s].cpu(), ref), tol)
            parity.check(tag + ": batched vs the single-sequence path", relerr(got[s].cpu(), feats(i).cpu()), tol)


@pytest.fixture(scope="module")
def small_bert():
    """Four layers, as in test_features_gpu.test_window_features_callback: the sum of the last four hidden states needs them."""
    torch.manual_seed(2)
    return transformers.BertModel(transformers.BertConfig(vocab_size=500, num_hidden_layers=4), add_pooling_layer=False).eval()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_bert_batch_no_leakage(rg, small_bert, precision):
    """Replacing sequence 1's ids leaves every other sequence's output bit-identical (same shapes, same launches,
    deterministic kernels): a wrong row offset in the embedding or the attention would mix neighbours."""
    feats = rg.features.BertFeatures(small_bert.state_dict(), device="cuda", precision=precision)
    ids = _bert_ids((2, 9, 47, 65, 200), 3, 500)
    a = [t.clone() for t in feats.batch(ids)]
    ids2 = list(ids)
    ids2[1] = _bert_ids((9,), 4, 500)[0]
    b = feats.batch(ids2)
    torch.cuda.synchronize()
    assert not torch.equal(a[1], b[1])
    for s in (0, 2, 3, 4):
        assert torch.equal(_bits(a[s]), _bits(b[s])), s
    for bad in ([], [torch.zeros(0, dtype=torch.long)], [torch.zeros(513, dtype=torch.long)]):
        with pytest.raises(rg.capi.RgError):
            feats.batch(bad)


# ------------------------------------------------------------------------------------------------ wav2vec2
@pytest.fixture(scope="module")
def small_w2v():
    torch.manual_seed(1)
    return transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(num_hidden_layers=2)).eval()


def _waves(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, generator=g) * (0.03 + 0.04 * torch.rand(B, 1, generator=g)) + 0.02 * torch.randn(B, 1, generator=g)


def _w2v_oracle(model, waves):
    xn = (waves - waves.mean(1, keepdim=True)) / torch.sqrt(waves.var(1, unbiased=False, keepdim=True) + 1e-7)
    with torch.no_grad():
        return model.feature_extractor(xn).transpose(1, 2), model(xn).last_hidden_state


def _check_w2v(rg, parity, model, waves, precisions, tag, single=True):
    B, n = waves.shape
    ref_conv, ref = _w2v_oracle(model, waves)
    T = ref.shape[1]
    for precision, tol_conv, tol in precisions:
        feats = rg.features.Wav2Vec2Features(model.state_dict(), device="cuda", precision=precision)
        conv = feats.conv_features_batch(waves)
        got = feats.batch(waves)
        torch.cuda.synchronize()
        assert conv.shape == (B, T, 512) and got.shape == (B, T, 768)
        for b in range(B):
            name = "wav2vec2 batch %s, window %d %s" % (tag, b, precision)
            parity.check(name + ": conv features vs transformers", relerr(conv[b].cpu(), ref_conv[b]), tol_conv)
            parity.check(name + ": last hidden state vs transformers", relerr(got[b].cpu(), ref[b]), tol)
            if single:
                parity.check(name + ": batched vs the single-window path", relerr(got[b].cpu(), feats(waves[b]).cpu()), tol)
        if B > 1:      # chunked: the same windows, one per pass
            parity.check("wav2vec2 batch %s %s: chunk=1 vs one pass" % (tag, precision),
                         relerr(feats.batch(list(waves), chunk=1).cpu(), got.cpu()), tol)


BOTH = (("fp32", 2e-4, 2e-3), ("bf16", 2e-2, 3e-2))


@pytest.mark.parametrize("B,n", [(3, 16000), (2, 16150)])
def test_wav2vec2_batch(rg, parity, small_w2v, B, n):
    """1 s windows: n = 16000 (n_pad = n: every layer has ONE junk row per window, computed from the next window's first rows)
    and n = 16150 (not a multiple of 320: zero padding behind every window, 51 rows for 50 valid ones at the last layer)."""
    _check_w2v(rg, parity, small_w2v, _waves(B, n, 10 + B), BOTH, "B=%d n=%d" % (B, n))


def test_wav2vec2_batch_production_shape(rg, parity):
    """Two 10 s windows through the full 12 layers in bf16 (499 frames: the 512-key attention, M = 2 x 32000 rows at layer 0)."""
    torch.manual_seed(1)
    model = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config()).eval()
    _check_w2v(rg, parity, model, _waves(2, 160000, 7), BOTH[1:], "B=2 n=160000", single=False)


@pytest.mark.parametrize("n", [16000, 16150])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_wav2vec2_batch_no_leakage(rg, small_w2v, precision, n):
    """Replacing window 1's samples leaves windows 0 and 2 bit-identical: catches a wrong boundary in the junk rows, the
    group-norm statistics, the patch matrices or the attention."""
    feats = rg.features.Wav2Vec2Features(small_w2v.state_dict(), device="cuda", precision=precision)
    waves = _waves(3, n, 20)
    a, ca = feats.batch(waves).clone(), feats.conv_features_batch(waves).clone()
    waves2 = waves.clone()
    waves2[1] = _waves(1, n, 21)[0] * 3.0 + 0.5
    b, cb = feats.batch(waves2), feats.conv_features_batch(waves2)
    torch.cuda.synchronize()
    assert not torch.equal(a[1], b[1]) and not torch.equal(ca[1], cb[1])
    for w in (0, 2):
        assert torch.equal(_bits(ca[w]), _bits(cb[w])), w
        assert torch.equal(_bits(a[w]), _bits(b[w])), w
    with pytest.raises(rg.capi.RgError):
        feats.batch([waves[0], waves[1][:-1]])


# ------------------------------------------------------------------------------------------------ windows and their users
def _small_window_features(rg, small_bert, small_w2v):
    vocab = {}
    tok = lambda sentence: [101] + [vocab.setdefault(w, 110 + len(vocab)) for w in sentence.split()] + [102]
    return rg.features.WindowFeatures(rg.features.BertFeatures(small_bert.state_dict()),
                                      rg.features.Wav2Vec2Features(small_w2v.state_dict()), tok), tok


def test_window_features_windows(rg, small_bert, small_w2v):
    """The three requests of test_features_gpu.test_window_features_callback (whole window, padded tail, empty transcript) as
    ONE call: same assertions."""
    torch.manual_seed(2)
    wf, tok = _small_window_features(rg, small_bert, small_w2v)
    raw = torch.randn(1, 16000 * 19) * 0.1
    segs = [[[9.5, 9.9], "so"], [[9.5, 9.9], "me"], [[10.2, 10.8], "big"], [[11.0, 11.5], "house"]]
    out, tail, empty = wf.windows([(raw, 9.0, 19.0, segs), (raw, 18.0, 28.0, []), (raw, 9.0, 19.0, [])])
    assert out["raw_word"] == ["some big house"]
    assert out["audio"].shape == (1, 499, 768) and out["text_features"][0].shape == (5, 768)
    ids = torch.tensor(tok("some big house"))
    with torch.no_grad():
        hs = small_bert(input_ids=ids[None], output_hidden_states=True).hidden_states
        wave = raw[0, 9 * 16000:19 * 16000]
        ref_a = small_w2v(((wave - wave.mean()) / torch.sqrt(wave.var(unbiased=False) + 1e-7))[None]).last_hidden_state
    assert relerr(out["text_features"][0].cpu(), torch.stack(hs[-4:]).sum(0)[0]) <= 2e-2
    assert relerr(out["audio"].cpu(), ref_a) <= 3e-2
    assert tail["audio"].shape == (1, 499, 768) and tail["text_features"][0].shape == (2, 768) and tail["raw_word"] == [""]
    assert empty["text_features"][0].shape == (2, 768) and empty["raw_word"] == [""]
    assert relerr(empty["audio"].cpu(), ref_a) <= 3e-2
    one = wf.window(raw, 18.0, 28.0, [])
    assert relerr(tail["audio"].cpu(), one["audio"].cpu()) <= 3e-2
    assert relerr(tail["text_features"][0].cpu(), one["text_features"][0].cpu()) <= 2e-2


class _Counting:
    """A `features` object in both of its batched spellings that counts the batched calls."""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __call__(self, *a):
        return self.inner(*a)

    def batch(self, requests):
        self.calls.append(len(requests))
        return self.inner.batch(requests)

    windows = batch


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dataset_builds_features_in_batches(rg, parity, small_bert, small_w2v):
    """SMPLXClipDataset over the two long recordings of tests/golden/dataset_fixture.py (5 windows of 10 s at stride 5):
    ceil(5 / feature_batch) calls of `windows`, and samples equal to those built window by window with the same encoders."""
    fx = _load("dataset_fixture")
    recs = [r for r in fx.recordings() if r["poses"].shape[0] >= 301]
    model = {k: v for k, v in fx.smplx_model().items() if k not in ("f", "weights", "posedirs")}
    pre = rg.dataset.ClipPreprocessor(model, pose_fps=fx.POSE_FPS)
    words = "so i went there and it was big".split()
    ann = dict(text_segments=[[[1.3 * k, 1.3 * k + 0.4], w] for k, w in enumerate(words)], discourse=[], prominence=[], gesture_labels=[])
    clips = [rg.dataset.RawClip(r["name"], r["poses"], r["trans"], r["expressions"], r["betas"], 3, annotations=ann) for r in recs]
    g = torch.Generator().manual_seed(9)
    raws = {c.name: torch.randn(1, 16000 * (c.n_raw // 30), generator=g) * 0.1 for c in clips}
    wf, _ = _small_window_features(rg, small_bert, small_w2v)
    per_window = rg.dataset.SMPLXClipDataset(clips, pre, features=lambda name, t0, t1, a: wf.window(raws[name], t0, t1, a["text_segments"][0]),
                                             pose_length=150, stride=5)
    n = len(per_window)
    assert n == 5
    counting = _Counting(wf.for_clips(raws))
    ds = rg.dataset.SMPLXClipDataset(clips, pre, features=counting, pose_length=150, stride=5, feature_batch=2)
    assert counting.calls == [2, 2, 1] and len(counting.calls) == math.ceil(n / 2)
    worst_a = worst_t = 0.0
    for k in range(n):
        a, b = ds[k], per_window[k]
        assert sorted(a) == sorted(b) and a["raw_word"] == b["raw_word"] and a["sample_name"] == b["sample_name"]
        assert a["audio"].shape == (499, 768) and a["text_feature"].shape == b["text_feature"].shape
        for key in ds.TENSOR_KEYS:
            assert torch.equal(a[key], b[key]), key
        worst_a = max(worst_a, relerr(a["audio"].cpu(), b["audio"].cpu()))
        worst_t = max(worst_t, relerr(a["text_feature"].cpu(), b["text_feature"].cpu()))
        assert ds.retrieval_samples[k]["text_feature"] is ds._side[k]["text_feature"]
    parity.check("dataset: audio features, batched vs per-window construction (bf16)", worst_a, 3e-2)
    parity.check("dataset: text features, batched vs per-window construction (bf16)", worst_t, 2e-2)
    batch = ds.collate([0, 4])
    assert batch["audio"].shape == (2, 499, 768) and len(batch["text_features"]) == 2 and counting.calls == [2, 2, 1]


def test_run_many_asks_for_one_feature_batch_per_window(rg, small_bert, small_w2v):
    """LongformSynthesizer.run_many over 3 clips x 2 windows: a `features` object with `batch` gets 2 calls of 3 requests;
    the plain callable of the same encoders gives the same clips (shapes; finite)."""
    cfg = rg.synth.default_model_cfg(num_layers=2)
    vae_cfgs = rg.synth.synth_vae_cfgs(decoder_arch="all_encoder", num_layers=2)
    model = rg.build_architecture(rg.synth.reference_style_model_cfg(cfg, vae_cfgs), database=None, precision="bf16")
    model.load_state_dict(rg.synth.synth_full_state(0, cfg, vae_cfgs))
    model.eval()

    def clip(seed):
        p = rg.synth.synth_batch(1, seed=seed)
        d = {k: p[k] for k in rg.longform.MOTION_KEYS + rg.longform.REPEAT_KEYS
             if k in p and torch.is_tensor(p[k]) and p[k].dim() >= 2 and p[k].shape[1] == 150}
        d["text_segments"] = [[[[0.7 * k, 0.7 * k + 0.5], w] for k, w in enumerate("well that was a very long day".split())]]
        return d

    clips = [clip(s) for s in (11, 12, 13)]                    # 150 frames at 15 fps: windows [0, 10] s and [9, 19] s
    g = torch.Generator().manual_seed(5)
    raws = [torch.randn(1, 160000, generator=g) * 0.1 for _ in clips]
    wf, _ = _small_window_features(rg, small_bert, small_w2v)
    synth = rg.longform.LongformSynthesizer(model, overlap=15)
    copy = lambda d: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}
    counting = _Counting(wf.for_clips(raws))
    many = synth.run_many([copy(c) for c in clips], counting, noise_tape=rg.synth.ClipTapes([71, 72, 73]))
    assert counting.calls == [3, 3]
    plain = synth.run_many([copy(c) for c in clips], lambda ci, cidx, t0, t1, a: wf.window(raws[ci], t0, t1, a["text_segments"][0]),
                           noise_tape=rg.synth.ClipTapes([71, 72, 73]))
    for ci in range(3):
        assert len(many[ci]["windows"]) == 2 and many[ci]["windows"] == plain[ci]["windows"]
        assert many[ci]["poses"].shape == plain[ci]["poses"].shape and np.isfinite(many[ci]["poses"]).all()
