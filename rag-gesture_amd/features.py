"""Per-window conditioning features: the two pretrained encoders the reference runs in front of the
hot path, on the HIP extension.

    tools/longform_synthesis.py:64-82   get_text_feature: BERT-base-cased, hidden_states of `tokenizer.encode_plus(sentence)`,
                                        sum of the last four layers -> [L_tokens, 768]
    tools/longform_synthesis.py:84-94   get_wav2vec2_feature: Wav2Vec2Processor (zero-mean / unit-variance waveform) +
                                        Wav2Vec2Model("facebook/wav2vec2-base-960h").last_hidden_state -> [499, 768] per 10 s
    mogen/datasets/beatx_dataset.py:498-505, 823-832, 1171-1179   the same two calls when the dataset caches are built

Weights are the Hugging Face state dicts (`BertModel.state_dict()`, `Wav2Vec2Model.state_dict()`: the released
checkpoints cannot be fetched here, tests use random-initialised models of the same configuration as the oracle).
Tokenisation (WordPiece vocabulary file) stays with the caller: `BertFeatures` takes token ids.

Everything numeric is a launch of the C-ABI extension: rg_gemm (bf16 MFMA operands, fp32 accumulate; bias / GELU /
residual epilogues; the strided convolutions of the wav2vec2 feature extractor are GEMMs over OVERLAPPING rows of the
previous layer's [T, 512] output: row t = elements [t * stride * 512, + kernel * 512), no im2col), rg_mha_bf16 (softmax
attention on the matrix cores, 499 keys resident in LDS), rg_layernorm_res, and the small kernels of csrc/rg_features.hip.
precision="fp32": bf16x3 split operands in the GEMMs (parity checks).

Many windows per call: `Wav2Vec2Features.batch`, `BertFeatures.batch`, `WindowFeatures.windows` run B windows through the
same launches (the reference, like the single-window methods here, encodes one window at a time: beatx_dataset.py:823-832,
1171-1179, longform_synthesis.py:64-94).  `conv_layout` states how B audio windows share one GEMM per convolution layer.
"""
import collections
import ctypes

import torch

from . import capi, gemm as G


def _f32(t, dev):
    return t.detach().to(torch.float32).to(dev).contiguous()


ConvLayout = collections.namedtuple("ConvLayout", "n n_pad T T_pad")
W2V_KERNELS, W2V_STRIDES = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)
FEATURE_BATCH_BYTES = 8 << 30     # activations one Wav2Vec2Features.batch chunk may hold (the default `chunk` follows from it)


def conv_layout(n, kernels=W2V_KERNELS, strides=W2V_STRIDES):
    """How B windows of n samples go through the strided convolutions as ONE GEMM per layer.  Every window gets
    n_pad = P * ceil(n / P) samples (P = the product of the strides) and layer i T_pad[i] = n_pad / (strides[0] * ... *
    strides[i]) rows, so T_pad[i - 1] = strides[i] * T_pad[i]: row b * T_pad[i] + t of layer i starts at element
    (b * T_pad[i] + t) * strides[i] * C of layer i - 1, the start of row b * T_pad[i - 1] + t * strides[i] -- window b's own
    row t * strides[i].  T[i] = (T[i - 1] - kernels[i]) // strides[i] + 1 rows per window are valid; a valid row reads rows up to
    (T[i] - 1) * strides[i] + kernels[i] - 1 <= T[i - 1] - 1 of its own window, all valid.  Rows T[i] .. T_pad[i] are junk (they
    may read the next window or the zeroed tail behind the last one) and are dropped after the last layer."""
    if len(kernels) != len(strides):
        raise capi.RgError("conv_layout: %d kernel sizes for %d strides" % (len(kernels), len(strides)))
    period = 1
    for s in strides:
        period *= int(s)
    n = int(n)
    n_pad = period * ((n + period - 1) // period)
    T, T_pad, cur, pad = [], [], n, n_pad
    for k, s in zip(kernels, strides):
        cur, pad = (cur - int(k)) // int(s) + 1, pad // int(s)
        if cur < 1:
            raise capi.RgError("conv_layout: %d samples are too few for the convolution stack" % n)
        T.append(cur)
        T_pad.append(pad)
    return ConvLayout(n, n_pad, tuple(T), tuple(T_pad))


class _Linear:
    def __init__(self, w, b, dev, split):
        self.w = G.pack_weight(w.detach().float(), dev, split=split)
        self.b = _f32(b, dev) if b is not None else None
        self.n, self.k = w.shape


class _Encoder:
    """Post-norm transformer encoder stack shared by the two models (BertLayer / Wav2Vec2EncoderLayer):
    x -> LN1(x + O(MHA(x))) -> LN2(. + FF2(GELU(FF1(.))))."""

    def __init__(self, layers, heads, eps, dev, precision):
        self.layers, self.heads, self.eps, self.dev, self.precision = layers, heads, eps, dev, precision
        self.h = capi.get_handle(dev.index if dev.index is not None else torch.cuda.current_device())

    def lin(self, lw, x32, xbf, out, act=0, residual=None):
        """out = act(x W^T + b) (+ residual); bf16 mode multiplies the bf16 copy, fp32 mode the fp32 rows (bf16x3)."""
        M = x32.shape[0] if x32 is not None else xbf.shape[0]
        if self.precision == "bf16":
            a = xbf if xbf is not None else None
            if a is not None:
                G.gemm(self.h, M=M, N=lw.n, K=lw.k, W=lw.w, out=out, A=a, bias=lw.b, act=act, residual=residual)
                return
        G.gemm(self.h, M=M, N=lw.n, K=lw.k, W=lw.w, out=out, segs=[G.Seg(x32)], bias=lw.b, act=act, residual=residual)

    def layer_norm(self, x, res, g, b, want_bf16=True):
        out = torch.empty_like(x)
        obf = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16) if (want_bf16 and self.precision == "bf16") else None
        self.h.call("layernorm_res", x, res, g, b, out, x.shape[0], x.shape[1], float(self.eps), obf)
        return out, obf

    def attention(self, qkv, L, D):
        hd = D // self.heads
        q, k, v = qkv.data_ptr(), qkv.data_ptr() + 4 * D, qkv.data_ptr() + 8 * D
        if self.precision == "fp32" and L <= 192:
            o = torch.empty(L, D, device=self.dev)
            self.h.call("mha", q, 3 * D, k, 3 * D, v, 3 * D, o, D, 1, self.heads, L, L, hd)
            return o, None
        o = torch.empty(L, D, device=self.dev, dtype=torch.bfloat16 if self.precision == "bf16" else torch.float32)
        self.h.call("mha_bf16", q, 3 * D, k, 3 * D, v, 3 * D, o, D, int(self.precision == "bf16"), 1, self.heads, L, L, hd)
        return (None, o) if self.precision == "bf16" else (o, None)

    def run_rows(self, x, xbf, attend, collect=None):
        """`run` over the M rows of any number of sequences: attend(qkv [M, 3 D], out [M, D]) issues the attention launches
        (`out` is bf16 in bf16 mode, the out-projection's operand).  The activations are allocated once and reused by every
        layer (a layer's output gets its own tensor only when `collect` keeps it)."""
        M, D = x.shape
        bf, dev = self.precision == "bf16", self.dev
        act = torch.bfloat16 if bf else torch.float32
        qkv, a, t = torch.empty(M, 3 * D, device=dev), torch.empty(M, D, device=dev, dtype=act), torch.empty(M, D, device=dev)
        f = torch.empty(M, self.layers[0]["ff1"].n, device=dev, dtype=act) if self.layers else None
        x1, x1bf = torch.empty(M, D, device=dev), (torch.empty(M, D, device=dev, dtype=torch.bfloat16) if bf else None)
        xo, xobf = torch.empty(M, D, device=dev), (torch.empty(M, D, device=dev, dtype=torch.bfloat16) if bf else None)
        for lw in self.layers:
            self.lin(lw["qkv"], x, xbf, qkv)
            attend(qkv, a)
            self.lin(lw["o"], None if bf else a, a if bf else None, t, residual=x)
            self.h.call("layernorm_res", t, None, lw["ln1_g"], lw["ln1_b"], x1, M, D, float(self.eps), x1bf)
            self.lin(lw["ff1"], x1, x1bf, f, act=1)
            self.lin(lw["ff2"], None if bf else f, f if bf else None, t, residual=x1)
            if collect is not None:
                xo = torch.empty(M, D, device=dev)
            self.h.call("layernorm_res", t, None, lw["ln2_g"], lw["ln2_b"], xo, M, D, float(self.eps), xobf)
            x, xbf = xo, xobf
            if collect is not None:
                collect.append(x)
        return x

    def run(self, x, xbf, collect=None):
        L, D = x.shape
        bf = self.precision == "bf16"
        for lw in self.layers:
            qkv = torch.empty(L, 3 * D, device=self.dev)
            self.lin(lw["qkv"], x, xbf, qkv)
            a32, abf = self.attention(qkv, L, D)
            t = torch.empty(L, D, device=self.dev)
            self.lin(lw["o"], a32, abf, t, residual=x)
            x1, x1bf = self.layer_norm(t, None, lw["ln1_g"], lw["ln1_b"])
            f = torch.empty(L, lw["ff1"].n, device=self.dev, dtype=torch.bfloat16 if bf else torch.float32)
            self.lin(lw["ff1"], x1, x1bf, f, act=1)
            t2 = torch.empty(L, D, device=self.dev)
            self.lin(lw["ff2"], None if bf else f, f if bf else None, t2, residual=x1)
            x, xbf = self.layer_norm(t2, None, lw["ln2_g"], lw["ln2_b"])
            if collect is not None:
                collect.append(x)
        return x


class BertFeatures:
    """BertModel (bert-base-cased shapes) hidden states.  state: `BertModel.state_dict()` (keys may carry a `bert.`
    prefix).  __call__(input_ids [L]) -> [L, 768] = sum of the last four hidden states (longform_synthesis.py:72-80)."""

    def __init__(self, state, num_heads=12, device="cuda", precision="bf16", eps=1e-12):
        dev = self.dev = torch.device(device)
        sd = {(k[5:] if k.startswith("bert.") else k): v for k, v in state.items()}
        split = precision == "fp32"
        f = lambda k: _f32(sd[k], dev)
        self.word, self.pos = f("embeddings.word_embeddings.weight"), f("embeddings.position_embeddings.weight")
        self.type0 = f("embeddings.token_type_embeddings.weight")[0].contiguous()
        self.eg, self.eb = f("embeddings.LayerNorm.weight"), f("embeddings.LayerNorm.bias")
        layers, i = [], 0
        while "encoder.layer.%d.attention.self.query.weight" % i in sd:
            p = "encoder.layer.%d." % i
            qkv_w = torch.cat([sd[p + "attention.self.%s.weight" % n] for n in ("query", "key", "value")], 0)
            qkv_b = torch.cat([sd[p + "attention.self.%s.bias" % n] for n in ("query", "key", "value")], 0)
            layers.append(dict(
                qkv=_Linear(qkv_w, qkv_b, dev, split),
                o=_Linear(sd[p + "attention.output.dense.weight"], sd[p + "attention.output.dense.bias"], dev, split),
                ln1_g=f(p + "attention.output.LayerNorm.weight"), ln1_b=f(p + "attention.output.LayerNorm.bias"),
                ff1=_Linear(sd[p + "intermediate.dense.weight"], sd[p + "intermediate.dense.bias"], dev, split),
                ff2=_Linear(sd[p + "output.dense.weight"], sd[p + "output.dense.bias"], dev, split),
                ln2_g=f(p + "output.LayerNorm.weight"), ln2_b=f(p + "output.LayerNorm.bias")))
            i += 1
        self.enc = _Encoder(layers, num_heads, eps, dev, precision)
        self.h = self.enc.h

    def hidden_states(self, input_ids):
        ids = input_ids.to(self.dev).long().view(-1).contiguous()
        L, D = ids.shape[0], self.word.shape[1]
        if L > self.pos.shape[0]:
            raise capi.RgError("BertFeatures: %d tokens exceed the %d position embeddings" % (L, self.pos.shape[0]))
        e = torch.empty(L, D, device=self.dev)
        self.h.call("embed_sum3", ids, self.word, self.pos, self.type0, e, L, D)
        x, xbf = self.enc.layer_norm(e, None, self.eg, self.eb)
        states = [x]
        self.enc.run(x, xbf, collect=states)
        return states

    def __call__(self, input_ids, layers=(-4, -3, -2, -1)):
        st = self.hidden_states(input_ids)
        out = st[layers[0]].clone()
        for i in layers[1:]:
            out += st[i]
        return out

    def hidden_states_batch(self, list_of_ids):
        """-> (states: the 1 + n_layers hidden states of all sequences' rows [sum L_i, 768], off: row offsets [n + 1])."""
        ids = [torch.as_tensor(i).long().view(-1) for i in list_of_ids]
        if not ids:
            raise capi.RgError("BertFeatures.batch: no sequences")
        off = [0]
        for i in ids:
            if not 1 <= i.numel() <= self.pos.shape[0]:
                raise capi.RgError("BertFeatures.batch: a sequence of %d tokens (1 .. %d position embeddings)"
                                   % (i.numel(), self.pos.shape[0]))
            off.append(off[-1] + i.numel())
        n, M, D, H = len(ids), off[-1], self.word.shape[1], self.enc.heads
        all_ids = torch.cat([i.to(self.dev) for i in ids]).contiguous()
        off_host = (ctypes.c_int * (n + 1))(*off)
        off_dev = torch.tensor(off, dtype=torch.int32, device=self.dev)
        e = torch.empty(M, D, device=self.dev)
        self.h.call("embed_sum3_ragged", all_ids, self.word, self.pos, self.type0, e, off_dev, off_host, n, D, self.pos.shape[0])
        x, xbf = self.enc.layer_norm(e, None, self.eg, self.eb)
        hd = D // H

        def attend(qkv, o):
            q = qkv.data_ptr()
            if self.enc.precision == "bf16":
                self.h.call("mha_bf16_ragged", q, 3 * D, q + 4 * D, 3 * D, q + 8 * D, 3 * D, o, D, 1, off_dev, off_host, n, H, hd)
                return
            for s in range(n):      # parity mode: the exact fp32 kernel per sequence of up to 192 tokens, as `_Encoder.attention`
                                    # (the matrix-core kernel rounds K and V to bf16; longer sequences take it in both paths)
                r0, L = off[s], off[s + 1] - off[s]
                qs, os_ = q + 4 * 3 * D * r0, o.data_ptr() + 4 * D * r0
                if L <= 192:
                    self.h.call("mha", qs, 3 * D, qs + 4 * D, 3 * D, qs + 8 * D, 3 * D, os_, D, 1, H, L, L, hd)
                else:
                    self.h.call("mha_bf16", qs, 3 * D, qs + 4 * D, 3 * D, qs + 8 * D, 3 * D, os_, D, 0, 1, H, L, L, hd)

        states = [x]
        self.enc.run_rows(x, xbf, attend, collect=states)
        return states, off

    def batch(self, list_of_ids, layers=(-4, -3, -2, -1)):
        """list of token-id vectors [L_i] (any lengths <= 512) -> list of [L_i, 768] in the order given: `__call__` for all
        of them in the same launches (token rows concatenated; rg_embed_sum3_ragged, rg_mha_bf16_ragged)."""
        out, off = self.batch_rows(list_of_ids, layers)
        return [out[off[s]:off[s + 1]] for s in range(len(off) - 1)]

    def batch_rows(self, list_of_ids, layers=(-4, -3, -2, -1)):
        """`batch` as it holds its result: (all sequences' rows [sum L_i, 768], row offsets [n + 1])."""
        st, off = self.hidden_states_batch(list_of_ids)
        out = st[layers[0]].clone()
        for i in layers[1:]:
            out += st[i]
        return out, off

    @staticmethod
    def word_rows(words, tokenize):
        """The token positions of each word of the sentence " ".join(words) (mogen/datasets/beatx_dataset.py:1126-1161
        get_word_vectors collects every position whose word_id falls in the word's range: continuation pieces and split
        punctuation included).  tokenize(text) -> ids with [CLS] and [SEP] around them.  WordPiece tokenises
        white-space-separated words independently, so the words' own pieces, one word after the other, must be the
        sentence's: a tokenizer for which they are not is refused.  -> offsets [n_words + 1] into the sentence's token rows
        (the first is 1: behind [CLS]); word w is rows off[w] .. off[w + 1]."""
        sentence = [int(t) for t in tokenize(" ".join(words))][1:-1]
        off = [1]
        for word in words:
            piece = [int(t) for t in tokenize(word)][1:-1]
            a = off[-1] - 1
            if not piece or sentence[a:a + len(piece)] != piece:
                raise ValueError("word_rows: the pieces of %r are not where the sentence's tokens have them "
                                 "(the tokenizer does not treat white-space-separated words independently)" % (word,))
            off.append(off[-1] + len(piece))
        if off[-1] - 1 != len(sentence):
            raise ValueError("word_rows: the sentence has %d tokens behind those of its words (last word %r)"
                             % (len(sentence) - off[-1] + 1, words[-1] if words else ""))
        return off


class Wav2Vec2Features:
    """Wav2Vec2Model (wav2vec2-base shapes: 7 conv layers, feat_extract_norm "group", 12 post-norm encoder layers).
    state: `Wav2Vec2Model.state_dict()` (keys may carry a `wav2vec2.` prefix).
    __call__(waveform [n] at 16 kHz) -> last_hidden_state [T, 768] (T = 499 for 10 s), input normalised like
    Wav2Vec2FeatureExtractor(do_normalize=True) unless normalize=False."""

    def __init__(self, state, num_heads=12, device="cuda", precision="bf16", eps=1e-5, conv_stride=(5, 2, 2, 2, 2, 2, 2),
                 pos_groups=16):
        dev = self.dev = torch.device(device)
        sd = {(k[9:] if k.startswith("wav2vec2.") else k): v for k, v in state.items()}
        split = precision == "fp32"
        f = lambda k: _f32(sd[k], dev)
        self.precision, self.eps, self.stride = precision, eps, tuple(conv_stride)
        self.convs = []
        for i in range(len(self.stride)):
            w = sd["feature_extractor.conv_layers.%d.conv.weight" % i].detach().float()      # [C_out, C_in, k]
            b = sd.get("feature_extractor.conv_layers.%d.conv.bias" % i)
            self.convs.append(dict(lin=_Linear(w.permute(0, 2, 1).reshape(w.shape[0], -1), b, dev, split), k=w.shape[2], cin=w.shape[1]))
        self.gn_g, self.gn_b = f("feature_extractor.conv_layers.0.layer_norm.weight"), f("feature_extractor.conv_layers.0.layer_norm.bias")
        self.fp_g, self.fp_b = f("feature_projection.layer_norm.weight"), f("feature_projection.layer_norm.bias")
        self.fp = _Linear(sd["feature_projection.projection.weight"], sd["feature_projection.projection.bias"], dev, split)
        # positional convolution: weight_norm(dim=2) stored as (g, v) -- either parametrization naming
        pk = "encoder.pos_conv_embed.conv."
        if pk + "weight" in sd:
            w = sd[pk + "weight"].detach().float()
        else:
            g = sd.get(pk + "weight_g", sd.get(pk + "parametrizations.weight.original0")).detach().float()
            v = sd.get(pk + "weight_v", sd.get(pk + "parametrizations.weight.original1")).detach().float()
            w = v * (g / v.norm(p=2, dim=(0, 1), keepdim=True))
        C, Cg, K = w.shape                                                                       # [768, 48, 128]
        self.pos_groups, self.pos_k = pos_groups, K
        capi.require(C // pos_groups == Cg, "unsupported argument: requires C // pos_groups == Cg")
        pb = sd[pk + "bias"]
        self.pos = [_Linear(w[g * Cg:(g + 1) * Cg].permute(0, 2, 1).reshape(Cg, K * Cg), pb[g * Cg:(g + 1) * Cg], dev, split)
                    for g in range(pos_groups)]
        self.enc_g, self.enc_b = f("encoder.layer_norm.weight"), f("encoder.layer_norm.bias")
        layers, i = [], 0
        while "encoder.layers.%d.attention.q_proj.weight" % i in sd:
            p = "encoder.layers.%d." % i
            qkv_w = torch.cat([sd[p + "attention.%s_proj.weight" % n] for n in ("q", "k", "v")], 0)
            qkv_b = torch.cat([sd[p + "attention.%s_proj.bias" % n] for n in ("q", "k", "v")], 0)
            layers.append(dict(
                qkv=_Linear(qkv_w, qkv_b, dev, split),
                o=_Linear(sd[p + "attention.out_proj.weight"], sd[p + "attention.out_proj.bias"], dev, split),
                ln1_g=f(p + "layer_norm.weight"), ln1_b=f(p + "layer_norm.bias"),
                ff1=_Linear(sd[p + "feed_forward.intermediate_dense.weight"], sd[p + "feed_forward.intermediate_dense.bias"], dev, split),
                ff2=_Linear(sd[p + "feed_forward.output_dense.weight"], sd[p + "feed_forward.output_dense.bias"], dev, split),
                ln2_g=f(p + "final_layer_norm.weight"), ln2_b=f(p + "final_layer_norm.bias")))
            i += 1
        self.enc = _Encoder(layers, num_heads, eps, dev, precision)
        self.h = self.enc.h

    def conv_features(self, wave):
        """Feature extractor: [n] -> [T, 512] fp32 (Wav2Vec2FeatureEncoder; transposed to time-major)."""
        h, dev, bf = self.h, self.dev, self.precision == "bf16"
        n = wave.numel()
        x = torch.zeros(n + 64, device=dev)      # tail padding: the GEMM's 64-wide K tiles may look past the last sample
        x[:n] = wave.to(dev).float().view(-1)
        c0 = self.convs[0]
        T = (n - c0["k"]) // self.stride[0] + 1
        y = torch.empty(T, c0["lin"].n, device=dev)
        # layer 0: rows of 10 samples at a hop of 5 (fp32 source, K = 10)
        G.gemm(h, M=T, N=c0["lin"].n, K=c0["lin"].k, W=c0["lin"].w, out=y, segs=[G.Seg(x, ld=self.stride[0])], bias=c0["lin"].b)
        C = y.shape[1]
        cur = torch.empty(T, C, device=dev, dtype=torch.bfloat16 if bf else torch.float32)
        ws = torch.empty(2 * C, device=dev)
        h.call("time_groupnorm_gelu", y, self.gn_g, self.gn_b, cur if bf else None, None if bf else cur, T, C, float(self.eps), ws)
        out = None
        for i in range(1, len(self.convs)):
            cv, s = self.convs[i], self.stride[i]
            Tn = (T - cv["k"]) // s + 1
            last = i == len(self.convs) - 1
            if bf:
                out = torch.empty(Tn, cv["lin"].n, device=dev, dtype=torch.float32 if last else torch.bfloat16)
                G.gemm(h, M=Tn, N=cv["lin"].n, K=cv["lin"].k, W=cv["lin"].w, out=out, A=cur.view(-1), lda=s * C, bias=cv["lin"].b, act=1)
            else:
                out = torch.empty(Tn, cv["lin"].n, device=dev)
                G.gemm(h, M=Tn, N=cv["lin"].n, K=cv["lin"].k, W=cv["lin"].w, out=out, segs=[G.Seg(cur.view(-1), ld=s * C)],
                       bias=cv["lin"].b, act=1)
            cur, T = out, Tn
        return cur.float() if cur.dtype != torch.float32 else cur

    def __call__(self, wave, normalize=True):
        h, dev = self.h, self.dev
        x = wave.to(dev).float().view(-1)
        if normalize:   # Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm
            x = (x - x.mean()) / torch.sqrt(x.var(unbiased=False) + 1e-7)
        feats = self.conv_features(x)                                   # [T, 512]
        T = feats.shape[0]
        fn, fnbf = self.enc.layer_norm(feats, None, self.fp_g, self.fp_b)
        hid = torch.empty(T, self.fp.n, device=dev)
        self.enc.lin(self.fp, fn, fnbf, hid)
        D = hid.shape[1]
        # positional convolution: one patch matrix + GEMM per group, GELU, added to the hidden states, LayerNorm
        Cg, K = D // self.pos_groups, self.pos_k
        cols = torch.empty(self.pos_groups, T, K * Cg, device=dev, dtype=torch.bfloat16)
        h.call("im2col_grouped", hid, cols, T, D, self.pos_groups, K, K // 2)
        pos = torch.empty(T, D, device=dev)
        for g in range(self.pos_groups):
            lw = self.pos[g]
            o = pos[:, g * Cg:(g + 1) * Cg]
            if self.precision == "bf16":
                G.gemm(h, M=T, N=Cg, K=K * Cg, W=lw.w, out=o, A=cols[g], bias=lw.b, act=1)
            else:
                G.gemm(h, M=T, N=Cg, K=K * Cg, W=lw.w, out=o, segs=[G.Seg(cols[g].float())], bias=lw.b, act=1)
        x0, x0bf = self.enc.layer_norm(hid, pos, self.enc_g, self.enc_b)
        return self.enc.run(x0, x0bf)

    # ---- many windows per call
    def layout(self, n):
        return conv_layout(n, [c["k"] for c in self.convs], self.stride)

    def default_chunk(self, n):
        """Windows of n samples per pass such that the pass's activations stay within FEATURE_BATCH_BYTES: the layer-0
        output (fp32) and its normalised copy dominate the convolution stack (~130 MB per 10 s window in bf16 mode), the
        positional convolution's patch matrices, made after those are released, are ~98 MB."""
        lay, C, D = self.layout(n), self.convs[0]["lin"].n, self.fp.n
        e = 2 if self.precision == "bf16" else 4
        conv = lay.T_pad[0] * C * (4 + 2 * e)                    # layer 0 in fp32, its normalised copy, layers 1 .. 6 (a half each)
        T = lay.T[-1]
        pos = T * self.pos_k * D * (2 if e == 2 else 6)          # bf16 patch matrices (fp32 mode: and their fp32 copies)
        ff = self.enc.layers[0]["ff1"].n if self.enc.layers else 0
        enc = T * (12 * D + ff) * 4
        # the convolution buffers are free again when the patch matrices are made, and those when the layers run
        return max(1, int(FEATURE_BATCH_BYTES // (max(conv, pos) + enc)))

    def _rows_with_tail(self, rows, C, tail, dtype):
        """[rows, C] at the front of a flat buffer whose `tail` further elements are zero: the last window's junk rows and the
        GEMM's 64-wide K tiles look past the last row."""
        buf = torch.empty(rows * C + tail, device=self.dev, dtype=dtype)
        buf[rows * C:].zero_()
        return buf

    def _conv_batch(self, x, normalize):
        """x [B, n] fp32 on the device -> (conv features [B * T, 512] fp32, T): one launch per layer for all windows."""
        h, dev, bf = self.h, self.dev, self.precision == "bf16"
        B, n = x.shape
        lay, nl = self.layout(n), len(self.convs)
        act = torch.bfloat16 if bf else torch.float32
        tail = lambda i: (max(self.convs[i]["k"] - self.stride[i], 0) * self.convs[i]["cin"] + 64) if i < nl else 0
        xin = self._rows_with_tail(B, lay.n_pad, tail(0), torch.float32)
        h.call("wave_normalize", x, x.stride(0), xin, B, n, lay.n_pad, int(bool(normalize)))
        c0 = self.convs[0]
        C, M = c0["lin"].n, B * lay.T_pad[0]
        y = torch.empty(M, C, device=dev)
        G.gemm(h, M=M, N=C, K=c0["lin"].k, W=c0["lin"].w, out=y, segs=[G.Seg(xin, ld=self.stride[0])], bias=c0["lin"].b)
        cur = self._rows_with_tail(M, C, tail(1), act)
        ws = torch.empty(2 * B * C, device=dev)
        h.call("time_groupnorm_gelu_batched", y, self.gn_g, self.gn_b, cur if bf else None, None if bf else cur, B, lay.T[0],
               lay.T_pad[0], C, float(self.eps), ws)
        del y
        for i in range(1, nl):
            cv, s = self.convs[i], self.stride[i]
            M, N = B * lay.T_pad[i], cv["lin"].n
            buf = self._rows_with_tail(M, N, tail(i + 1), torch.float32 if (i == nl - 1 or not bf) else torch.bfloat16)
            out = buf[:M * N].view(M, N)
            if bf:
                G.gemm(h, M=M, N=N, K=cv["lin"].k, W=cv["lin"].w, out=out, A=cur, lda=s * C, bias=cv["lin"].b, act=1)
            else:
                G.gemm(h, M=M, N=N, K=cv["lin"].k, W=cv["lin"].w, out=out, segs=[G.Seg(cur, ld=s * C)], bias=cv["lin"].b, act=1)
            cur, C = buf, N
        T = lay.T[-1]
        feats = torch.empty(B * T, C, device=dev)
        h.call("copy_rows", cur, feats, B, T, C, lay.T_pad[-1], 0, T, 0)      # drop the junk rows
        return feats, T

    def _waves(self, waves):
        if isinstance(waves, (list, tuple)):
            if not waves or len({int(w.numel()) for w in waves}) != 1:
                raise capi.RgError("Wav2Vec2Features.batch: the windows of one call must have one length")
            waves = torch.stack([w.reshape(-1) for w in waves])
        if waves.dim() != 2 or waves.shape[0] < 1:
            raise capi.RgError("Wav2Vec2Features.batch: waveforms [B, n] expected")
        return waves.to(self.dev).float().contiguous()

    def conv_features_batch(self, waves, normalize=True):
        """[B, n] -> [B, T, 512]: the feature extractor's output of every window (parity checks; one pass, no chunking)."""
        x = self._waves(waves)
        feats, T = self._conv_batch(x, normalize)
        return feats.view(x.shape[0], T, -1)

    def _batch_pass(self, x, normalize):
        h, dev, B = self.h, self.dev, x.shape[0]
        feats, T = self._conv_batch(x, normalize)
        M = B * T
        fn, fnbf = self.enc.layer_norm(feats, None, self.fp_g, self.fp_b)
        hid = torch.empty(M, self.fp.n, device=dev)
        self.enc.lin(self.fp, fn, fnbf, hid)
        D, H = hid.shape[1], self.enc.heads
        Cg, K = D // self.pos_groups, self.pos_k
        cols = torch.empty(self.pos_groups, M, K * Cg, device=dev, dtype=torch.bfloat16)
        h.call("im2col_grouped_batched", hid, cols, B, T, D, self.pos_groups, K, K // 2)
        pos = torch.empty(M, D, device=dev)
        if self.precision != "bf16":
            cols = cols.float()                      # parity mode: the bf16x3 GEMM takes fp32 rows (one copy for all groups)
        descs = []
        for g in range(self.pos_groups):
            lw, o = self.pos[g], pos[:, g * Cg:(g + 1) * Cg]
            a = dict(A=cols[g]) if self.precision == "bf16" else dict(segs=[G.Seg(cols[g])])
            descs.append(G.make_desc(M=M, N=Cg, K=K * Cg, W=lw.w, out=o, bias=lw.b, act=1, **a))
        for g in range(0, self.pos_groups, 4):       # rg_gemm_grouped takes four problems: 16 groups are 4 launches
            part = descs[g:g + 4]
            h.call("gemm_grouped", ctypes.byref((G.GemmDesc * len(part))(*part)), len(part), keep=(cols, pos))
        del cols, descs                              # ~98 MB per window: released before the layers allocate
        x0, x0bf = self.enc.layer_norm(hid, pos, self.enc_g, self.enc_b)
        hd = D // H

        def attend(qkv, o):
            q = qkv.data_ptr()
            if self.precision == "fp32" and T <= 192:
                h.call("mha", q, 3 * D, q + 4 * D, 3 * D, q + 8 * D, 3 * D, o, D, B, H, T, T, hd)
            else:
                h.call("mha_bf16", q, 3 * D, q + 4 * D, 3 * D, q + 8 * D, 3 * D, o, D, int(self.precision == "bf16"), B, H, T, T, hd)

        return self.enc.run_rows(x0, x0bf, attend).view(B, T, D)

    def batch(self, waves, normalize=True, chunk=None):
        """waves [B, n] (or a list of B waveforms of one length; host or device) -> last_hidden_state [B, T, 768]: `__call__`
        for B windows in the same launches (`conv_layout`; rg_wave_normalize, rg_time_groupnorm_gelu_batched,
        rg_im2col_grouped_batched).  chunk: windows per pass (default: `default_chunk`, from FEATURE_BATCH_BYTES)."""
        x = self._waves(waves)
        B, n = x.shape
        chunk = self.default_chunk(n) if chunk is None else int(chunk)
        if chunk < 1:
            raise capi.RgError("Wav2Vec2Features.batch: chunk must be at least 1")
        if B <= chunk:
            return self._batch_pass(x, normalize)
        return torch.cat([self._batch_pass(x[b:b + chunk], normalize) for b in range(0, B, chunk)])


def merge_disco_textsegs(textsegs):
    """mogen/datasets/beatx_dataset.py:1099-1113: consecutive segments with identical (start, end) are one segment whose
    words are concatenated."""
    merged = []
    for i, seg in enumerate(textsegs):
        seg = [list(seg[0]), seg[1]]
        if i > 0 and seg[0] == list(textsegs[i - 1][0]):
            merged[-1][1] += seg[1]
        else:
            merged.append(seg)
    return merged


class WindowFeatures:
    """The per-window conditioning of tools/longform_synthesis.py:320-343 as the `features` callback of
    longform.LongformSynthesizer: wav2vec2 on the window's 16 kHz samples (`raw_audio` of the sample, [1, n]) and BERT
    (sum of the last four layers) on the window's transcript.  `tokenize(sentence) -> token ids` is the caller's
    WordPiece tokenizer (`tokenizer.encode_plus(sentence)["input_ids"]`); the models are BertFeatures / Wav2Vec2Features."""

    def __init__(self, bert, wav2vec2, tokenize, sample_rate=16000, frame_words=False, pose_fps=15, aligner=None):
        """frame_words: the answers also hold `word` [1, n_frames, 768], n_frames = round((t1 - t0) pose_fps): each word's
        vector (the mean of its token rows of `text_features`) written over the frames its span covers
        (mogen/datasets/beatx_dataset.py:858-869, word_rep="bert_framealigned"; rg_word_frames).  aligner: an
        align.CTCAligner on the same audio encoder; with it a request's text_segments may be a bare transcript (a string):
        the word timings then come from the window's own audio features, and the answer gains `text_segments=[segments]`."""
        self.bert, self.w2v, self.tokenize, self.sr = bert, wav2vec2, tokenize, sample_rate
        self.frame_words, self.pose_fps, self.aligner = bool(frame_words), pose_fps, aligner

    def window(self, raw_audio, t0, t1, text_segments):
        if self.frame_words or isinstance(text_segments, str):
            return self.windows([(raw_audio, t0, t1, text_segments)])[0]
        wave = self._wave(raw_audio, t0, t1)
        audio = self.w2v(wave).unsqueeze(0)
        sentence = " ".join(seg[1] for seg in merge_disco_textsegs(text_segments))
        ids = torch.as_tensor(self.tokenize(sentence), dtype=torch.long)
        return dict(audio=audio, raw_word=[sentence], text_features=[self.bert(ids)])

    def for_sample(self, raw_audio):
        """-> features(cidx, t0, t1, annotations) for LongformSynthesizer.run on that sample."""
        return lambda cidx, t0, t1, ann: self.window(raw_audio, t0, t1, ann["text_segments"][0])

    def _wave(self, raw_audio, t0, t1):
        """The window's samples, the tail of the last window padded with zeros."""
        a0, a1 = int(t0 * self.sr), int(t1 * self.sr)
        wave = raw_audio.view(-1)[a0:a1]
        if wave.numel() < a1 - a0:
            wave = torch.cat([wave, wave.new_zeros(a1 - a0 - wave.numel())])
        return wave

    def _aligned(self, requests, part, audio, n_samples):
        """part's requests' text_segments, those given as a bare transcript timed from the window's audio features [len(part),
        T, 768] (windows of n_samples samples); and which requests those were."""
        segs = {i: requests[i][3] for i in part}
        asked = [j for j, i in enumerate(part) if isinstance(segs[i], str)]
        if asked:
            if self.aligner is None:
                raise capi.RgError("WindowFeatures: a transcript without timings needs an aligner (align.CTCAligner)")
            if self.sr != 16000:
                raise capi.RgError("WindowFeatures: the aligner's time rule is that of 16 kHz audio, sample_rate is %s" % self.sr)
            got = self.aligner.align(audio[asked], [segs[part[j]] for j in asked], n_samples=[n_samples] * len(asked))
            for j, g in zip(asked, got):
                segs[part[j]] = g
        return segs, {part[j] for j in asked}

    def _frame_words(self, rows, off, merged, spans):
        """rg_word_frames over one BertFeatures.batch_rows result: window j's words merged[j] ([[start, end], word] in window
        time) own the token rows BertFeatures.word_rows says; the rows between two windows' words ([SEP], [CLS]) go to a
        word of no frames.  spans[j] = the window's length in seconds.  -> list of [1, n_frames_j, 768]."""
        tok_row, start, end, word_off, frame_off = [], [], [], [0], [0]
        for j, segs in enumerate(merged):
            n_frames = int(round(spans[j] * self.pose_fps))
            woff = BertFeatures.word_rows([s[1] for s in segs], self.tokenize)
            if off[j] + woff[-1] + 1 != off[j + 1]:
                raise capi.RgError("WindowFeatures: the words' tokens are not the sentence's")
            for k, s in enumerate(segs):
                # the reference's sample_wordenc[int(start * fps):int(end * fps)] = vec, Python floats, a slice of n_frames rows
                lo, hi, _ = slice(int(s[0][0] * self.pose_fps), int(s[0][1] * self.pose_fps)).indices(n_frames)
                tok_row.append(off[j] + woff[k])
                start.append(lo)
                end.append(hi)
            tok_row.append(off[j] + woff[-1])                # [SEP] and the next window's [CLS]
            start.append(0)
            end.append(0)
            word_off.append(len(start))
            frame_off.append(frame_off[-1] + n_frames)
        tok_row.append(off[-1])
        dev, D = rows.device, rows.shape[1]
        ints = torch.tensor(tok_row + start + end + word_off, dtype=torch.int32, device=dev)
        nw, n = len(start), len(merged)
        foff = torch.tensor(frame_off, dtype=torch.int64, device=dev)
        out = torch.empty(max(frame_off[-1], 1), D, device=dev)
        self.bert.h.call("word_frames", rows, ints[:nw + 1], ints[nw + 1:2 * nw + 1], ints[2 * nw + 1:3 * nw + 1], ints[3 * nw + 1:],
                         (ctypes.c_int * (n + 1))(*word_off), foff, (ctypes.c_int64 * (n + 1))(*frame_off), n, D, out)
        return [out[frame_off[j]:frame_off[j + 1]].unsqueeze(0) for j in range(n)]

    def windows(self, requests, chunk=None):
        """requests: list of (raw_audio, t0, t1, text_segments) -> list of what `window` returns for each, in the order
        given.  The windows of one sample count go together: ONE Wav2Vec2Features.batch and ONE BertFeatures.batch call per
        `chunk` of them (default: the audio encoder's default_chunk for that length), and with frame_words ONE rg_word_frames
        launch.  Windows of another length (a clip's whole span, a start time whose sample index truncates the other way) form
        groups of their own."""
        waves = [self._wave(*r[:3]) for r in requests]
        groups = {}
        for i, w in enumerate(waves):
            groups.setdefault(int(w.numel()), []).append(i)
        out = [None] * len(requests)
        for n, idx in groups.items():
            step = chunk
            if step is None:
                step = self.w2v.default_chunk(n) if hasattr(self.w2v, "default_chunk") else len(idx)
            for c in range(0, len(idx), int(step)):
                part = idx[c:c + int(step)]
                audio = self.w2v.batch(torch.stack([waves[i] for i in part]), chunk=len(part))
                segs, timed = self._aligned(requests, part, audio, n)
                merged = [merge_disco_textsegs(segs[i]) for i in part]
                sentences = [" ".join(s[1] for s in m) for m in merged]
                ids = [torch.as_tensor(self.tokenize(s), dtype=torch.long) for s in sentences]
                if self.frame_words:
                    rows, off = self.bert.batch_rows(ids)
                    text = [rows[off[j]:off[j + 1]] for j in range(len(part))]
                    word = self._frame_words(rows, off, merged, [requests[i][2] - requests[i][1] for i in part])
                else:
                    text = self.bert.batch(ids)
                for j, i in enumerate(part):
                    out[i] = dict(audio=audio[j:j + 1], raw_word=[sentences[j]], text_features=[text[j]])
                    if self.frame_words:
                        out[i]["word"] = word[j]
                    if i in timed:
                        out[i]["text_segments"] = [segs[i]]
        return out

    def for_clips(self, raw_audios):
        """raw_audios: the clips' 16 kHz samples by clip index (a list) or by recording name (a dict) -> the `features` of
        LongformSynthesizer.run_many and of dataset.SMPLXClipDataset, with the batched form both look for."""
        return ClipWindowFeatures(self, raw_audios)


class ClipWindowFeatures:
    """Callable as features(clip, t0, t1, annotations) (dataset.SMPLXClipDataset) and features(clip, cidx, t0, t1,
    annotations) (LongformSynthesizer.run_many): one `WindowFeatures.window`.  batch(requests) / windows(requests) take a
    list of those argument tuples and answer them with one `WindowFeatures.windows` call."""

    def __init__(self, window_features, raw_audios):
        self.wf, self.raw = window_features, raw_audios

    def _request(self, args):
        clip, (t0, t1, ann) = args[0], args[-3:]
        return self.raw[clip], t0, t1, ann["text_segments"][0]

    def __call__(self, *args):
        return self.wf.window(*self._request(args))

    def batch(self, requests):
        return self.wf.windows([self._request(r) for r in requests])

    windows = batch
