"""Word timings from speech and its transcript, on the device: the `text_segments` ([[start, end], word] in seconds) that the
dataset builder, the retrieval annotations and features.WindowFeatures(frame_words=True) consume.

The reference only CONSUMES such timings (annotation files a forced aligner wrote offline: mogen/datasets/beatx_dataset.py
:858-869 reads them); producing them is this project's own addition, like audio.Resampler.  The audio encoder that already
runs for the `audio` features, facebook/wav2vec2-base-960h, is a CTC model: its checkpoint carries `lm_head.{weight, bias}`
([32, 768]), so one more linear on hidden states already held gives character emissions, and a Viterbi alignment of those
against the transcript (csrc/rg_ctc.hip: rg_ctc_log_softmax, rg_ctc_align; the recurrence and its tie rule are stated in
include/rg_gesture.h and DESIGN) gives each character its frames.

Time rule.  Emission frame t of a window covers samples frame_sample[t] .. frame_sample[t] + 320 (frame_sample[t] = 320 t by
default: the encoder's stride).  A word starts at frame_sample[first frame of its first character] / 16000 and ends at
(frame_sample[last frame of its last character] + 320) / 16000, clamped to the audio's length.  A word none of whose
characters the vocabulary holds (digits, say) is unalignable: it spans from the previous aligned word's end (or 0) to the
next one's start (or the end of the audio).

Nothing here says how good the timings are on real speech, or how they compare with a forced aligner's: no checkpoint and no
annotated recording is available to the tests, which pin the arithmetic only.
"""
import ctypes

import numpy as np
import torch

from . import capi, features as F

SAMPLE_RATE = 16000
FRAME_STRIDE = 320          # samples between two emission frames (the product of the convolution strides)
FRAME_FIELD = 400           # samples one emission frame sees
C = capi.header_constants()
MAX_VOCAB, MAX_STATES, PER = C["RG_CTC_MAX_VOCAB"], C["RG_CTC_MAX_STATES"], C["RG_CTC_STATES_PER_THREAD"]


def _i64(values):
    values = [int(v) for v in values]
    return (ctypes.c_int64 * len(values))(*values), values


def log_softmax(h, logits):
    """logits [rows, V] fp32 on the device -> (logp [rows, V], best [rows] int32): rg_ctc_log_softmax."""
    rows, V = logits.shape
    logp = torch.empty_like(logits)
    best = torch.empty(rows, dtype=torch.int32, device=logits.device)
    h.call("ctc_log_softmax", logits, rows, V, logp, best)
    return logp, best


def viterbi(h, logp, frame_off, token_lists, blank=0):
    """rg_ctc_align over a ragged batch.  logp [rows, V] fp32 on the device; item i owns rows frame_off[i] .. frame_off[i + 1]
    and the tokens token_lists[i] (host integers).  -> dict of device tensors: path [rows] int32, tok_first / tok_last
    [sum L] int32, score [n] fp32, status [n] int32, and tok_off (host list).  Refused on the host, before any launch: a token
    outside [0, V) or equal to blank, an item without frames or tokens, more than RG_CTC_MAX_STATES states."""
    rows, V = logp.shape
    n = len(token_lists)
    if n < 1 or len(frame_off) != n + 1:
        raise capi.RgError("ctc align: %d items need %d frame offsets" % (n, n + 1))
    tok_off, bp_off, flat = [0], [0], []
    for i, toks in enumerate(token_lists):
        toks = [int(t) for t in toks]
        if any(t < 0 or t >= V or t == blank for t in toks):
            raise capi.RgError("ctc align: item %d holds a token outside [0, %d) or the blank (%d)" % (i, V, blank))
        S = 2 * len(toks) + 1
        if S > MAX_STATES:
            raise capi.RgError("ctc align: item %d has %d states (2 tokens + 1), at most %d" % (i, S, MAX_STATES))
        flat += toks
        tok_off.append(len(flat))
        bp_off.append(bp_off[-1] + max(int(frame_off[i + 1]) - int(frame_off[i]), 0) * ((S + PER - 1) // PER))
    if int(frame_off[-1]) != rows:
        raise capi.RgError("ctc align: the frame offsets end at %d, there are %d emission rows" % (int(frame_off[-1]), rows))
    dev = logp.device
    fo_host, fo = _i64(frame_off)
    to_host, _ = _i64(tok_off)
    bo_host, _ = _i64(bp_off)
    offs = torch.tensor(fo + tok_off + bp_off, dtype=torch.int64, device=dev)
    tokens = torch.tensor(flat if flat else [0], dtype=torch.int32, device=dev)
    backptr = torch.empty(max(bp_off[-1], 1), dtype=torch.int32, device=dev)
    out = dict(path=torch.empty(rows, dtype=torch.int32, device=dev), tok_first=torch.empty(max(len(flat), 1), dtype=torch.int32, device=dev),
               tok_last=torch.empty(max(len(flat), 1), dtype=torch.int32, device=dev), score=torch.empty(n, device=dev),
               status=torch.empty(n, dtype=torch.int32, device=dev))
    h.call("ctc_align", logp, V, offs[:n + 1], fo_host, tokens, offs[n + 1:2 * n + 2], to_host, n, int(blank), backptr, offs[2 * n + 2:], bo_host,
           out["path"], out["tok_first"], out["tok_last"], out["score"], out["status"])
    out["tok_first"], out["tok_last"] = out["tok_first"][:len(flat)], out["tok_last"][:len(flat)]
    out["tok_off"] = tok_off
    return out


def word_times(words, word_of_token, tok_first, tok_last, frame_sample, n_samples):
    """The time rule (module docstring) on the host.  words: the caller's strings; word_of_token[k]: the word of token k, -1
    for a delimiter; tok_first / tok_last [n tokens]: frames; frame_sample [T]: first sample of each frame.
    -> [[[start, end], word], ...] in seconds."""
    total = float(n_samples) / SAMPLE_RATE
    span = [None] * len(words)
    for k, w in enumerate(word_of_token):
        if w < 0:
            continue
        start = float(frame_sample[int(tok_first[k])]) / SAMPLE_RATE
        end = min(float(frame_sample[int(tok_last[k])] + FRAME_STRIDE) / SAMPLE_RATE, total)
        span[w] = [start, end] if span[w] is None else [span[w][0], end]
    out = []
    for i, word in enumerate(words):
        if span[i] is None:
            before = next((span[j][1] for j in range(i - 1, -1, -1) if span[j] is not None), 0.0)
            after = next((span[j][0] for j in range(i + 1, len(words)) if span[j] is not None), total)
            out.append([[before, after], word])
        else:
            out.append([list(span[i]), word])
    return out


def greedy_collapse(best, blank, delimiter_id):
    """Greedy CTC over one item's per-frame classes: runs of one class collapse, blanks go, the delimiter splits words.
    -> list of words, each a list of (class, first frame, last frame)."""
    words, cur, prev = [], [], None
    for t, c in enumerate(int(b) for b in best):
        if c == prev:
            if cur and c != blank and c != delimiter_id:
                cur[-1] = (c, cur[-1][1], t)
            continue
        prev = c
        if c == blank:
            continue
        if c == delimiter_id:
            if cur:
                words.append(cur)
            cur = []
            continue
        cur.append((c, t, t))
    if cur:
        words.append(cur)
    return words


def vocab_chars(vocab, blank=0, delimiter="|"):
    """What text may turn into: the vocabulary's single characters that are neither the blank nor the delimiter (specials
    such as <s> and <unk> are longer than one character and never come from text)."""
    return {c: int(i) for c, i in vocab.items() if len(c) == 1 and int(i) != int(blank) and c != delimiter and int(i) != int(vocab[delimiter])}


def text_tokens(words, chars, delimiter_id):
    """-> (ids, word_of_token): the classes of the words' characters that `chars` holds (tried as is, upper-cased, then
    lower-cased; a right single quotation mark reads as an apostrophe), one delimiter between consecutive alignable words
    (word_of_token -1), none at the ends.  A word with no character left contributes nothing: it is unalignable."""
    ids, word_of = [], []
    for w, word in enumerate(words):
        got = []
        for ch in word:
            ch = "'" if ch == "\u2019" else ch
            c = next((chars[c] for c in (ch, ch.upper(), ch.lower()) if len(c) == 1 and c in chars), None)
            if c is not None:
                got.append(c)
        if not got:
            continue
        if ids:
            ids.append(int(delimiter_id))
            word_of.append(-1)
        ids += got
        word_of += [w] * len(got)
    return ids, word_of


class CTCAligner:
    """w2v: the features.Wav2Vec2Features whose hidden states are aligned; weight [V, 768], bias [V]: the CTC head
    (`lm_head` of Wav2Vec2ForCTC); vocab: character -> class (the checkpoint's vocab.json); blank: the CTC blank's class
    (`<pad>` = 0 there); delimiter: the character that stands between words (`|`)."""

    def __init__(self, w2v, weight, bias, vocab, blank=0, delimiter="|"):
        self.w2v, self.h, self.dev = w2v, w2v.h, w2v.dev
        self.V, self.D = int(weight.shape[0]), int(weight.shape[1])
        if not 2 <= self.V <= MAX_VOCAB:
            raise capi.RgError("CTCAligner: %d classes (2 .. %d)" % (self.V, MAX_VOCAB))
        self.lm = F._Linear(weight, bias, self.dev, w2v.precision == "fp32")
        self.vocab, self.blank = dict(vocab), int(blank)
        if delimiter not in self.vocab:
            raise capi.RgError("CTCAligner: the delimiter %r is not in the vocabulary" % delimiter)
        self.delimiter, self.delimiter_id = delimiter, int(self.vocab[delimiter])
        if not (0 <= self.blank < self.V and all(0 <= int(i) < self.V for i in self.vocab.values())):
            raise capi.RgError("CTCAligner: a class outside [0, %d)" % self.V)
        self.chars = vocab_chars(self.vocab, self.blank, delimiter)
        self.char_of = {i: c for c, i in self.chars.items()}

    @classmethod
    def from_state(cls, state, vocab, **kw):
        """state: a `Wav2Vec2ForCTC.state_dict()` (wav2vec2.* and lm_head.*); kw: Wav2Vec2Features' (device, precision, ...)
        and this class's (blank, delimiter)."""
        mine = {k: kw.pop(k) for k in ("blank", "delimiter") if k in kw}
        return cls(F.Wav2Vec2Features(state, **kw), state["lm_head.weight"], state["lm_head.bias"], vocab, **mine)

    def tokens(self, words):
        """`text_tokens` with this aligner's vocabulary."""
        return text_tokens(words, self.chars, self.delimiter_id)

    # ---- device
    def emissions(self, hidden):
        """hidden [.., T, 768] fp32 on the device -> (logp [.., T, V], best [.., T] int32): the CTC head as the encoder's own
        linears go (rg_gemm), then rg_ctc_log_softmax."""
        x = hidden.to(self.dev).float().reshape(-1, hidden.shape[-1]).contiguous()
        if x.shape[1] != self.D:
            raise capi.RgError("CTCAligner.emissions: hidden states of width %d, the head takes %d" % (x.shape[1], self.D))
        logits = torch.empty(x.shape[0], self.V, device=self.dev)
        self.w2v.enc.lin(self.lm, x, None, logits)
        logp, best = log_softmax(self.h, logits)
        return logp.view(*hidden.shape[:-1], self.V), best.view(*hidden.shape[:-1])

    def _logp_items(self, x):
        """hidden states or log-probabilities, [B, T, .] or a list of [T_i, .] -> (logp rows [sum T_i, V], best or None, frame_off)."""
        items = list(x) if isinstance(x, (list, tuple)) else (list(x) if x.dim() == 3 else [x])
        if not items or any(i.dim() != 2 or i.shape[0] < 1 for i in items):
            raise capi.RgError("CTCAligner: [B, T, .] or a list of [T, .] with T >= 1 expected")
        off = [0]
        for i in items:
            off.append(off[-1] + i.shape[0])
        rows = (x.reshape(-1, x.shape[-1]) if torch.is_tensor(x) else torch.cat([i.to(self.dev) for i in items])).to(self.dev)
        if rows.shape[1] == self.D and self.D != self.V:
            logp, best = self.emissions(rows)
            return logp, best, off
        if rows.shape[1] != self.V:
            raise capi.RgError("CTCAligner: rows of width %d are neither hidden states (%d) nor log-probabilities (%d)"
                               % (rows.shape[1], self.D, self.V))
        return rows.float().contiguous(), None, off

    def align(self, hidden_or_logp, transcripts, frame_sample=None, n_samples=None, strict=True):
        """transcripts: per item a list of words (or a string, split at white space).  frame_sample: per item the first
        sample of each frame (default 320 t); n_samples: per item the audio's length (default: the last frame's last sample).
        -> per item [[[start, end], word], ...] with the caller's word strings (module docstring: time rule).  An item whose
        transcript cannot be laid onto its frames (fewer frames than tokens plus adjacent equal tokens) raises ValueError;
        with strict=False its answer is None.  One launch, one read-back."""
        logp, _, off = self._logp_items(hidden_or_logp)
        n = len(off) - 1
        words = [t.split() if isinstance(t, str) else list(t) for t in transcripts]
        if len(words) != n:
            raise capi.RgError("CTCAligner.align: %d transcripts for %d items" % (len(words), n))
        toks = [self.tokens(w) for w in words]
        live = [i for i in range(n) if toks[i][0]]
        firsts = lasts = status = None
        if live:
            # the items with something to align, their rows gathered when some item has none
            if len(live) == n:
                rows, foff = logp, off
            else:
                rows = torch.cat([logp[off[i]:off[i + 1]] for i in live])
                foff = [0]
                for i in live:
                    foff.append(foff[-1] + off[i + 1] - off[i])
            r = viterbi(self.h, rows, foff, [toks[i][0] for i in live], self.blank)
            back = torch.cat([r["tok_first"], r["tok_last"], r["status"], r["score"].view(torch.int32)]).cpu().numpy()
            nt = r["tok_off"][-1]
            firsts, lasts, status, tok_off = back[:nt], back[nt:2 * nt], back[2 * nt:2 * nt + len(live)], r["tok_off"]
        out = [None] * n
        for i in range(n):
            T = off[i + 1] - off[i]
            fs = np.arange(T, dtype=np.int64) * FRAME_STRIDE if frame_sample is None or frame_sample[i] is None else np.asarray(frame_sample[i])
            total = int(fs[-1]) + FRAME_FIELD if n_samples is None or n_samples[i] is None else int(n_samples[i])
            if i not in live:
                out[i] = word_times(words[i], [], [], [], fs, total)
                continue
            k = live.index(i)
            if status[k] != 0:
                if strict:
                    raise ValueError("CTCAligner.align: item %d: %d frames cannot hold its %d tokens" % (i, T, len(toks[i][0])))
                continue
            a, b = tok_off[k], tok_off[k + 1]
            out[i] = word_times(words[i], toks[i][1], firsts[a:b], lasts[a:b], fs, total)
        return out

    def transcribe(self, hidden_or_logp, frame_sample=None, n_samples=None):
        """Greedy CTC: per item [[[start, end], WORD], ...] from the per-frame best classes (runs collapsed, blanks dropped,
        split at the delimiter), timed by the same rule.  For recordings without a transcript; one read-back."""
        logp, best, off = self._logp_items(hidden_or_logp)
        if best is None:
            best = logp.argmax(-1)       # (log-probabilities handed in: no emissions were computed here)
        best = best.cpu().numpy()
        out = []
        for i in range(len(off) - 1):
            T = off[i + 1] - off[i]
            fs = np.arange(T, dtype=np.int64) * FRAME_STRIDE if frame_sample is None or frame_sample[i] is None else np.asarray(frame_sample[i])
            total = float(int(fs[-1]) + FRAME_FIELD if n_samples is None or n_samples[i] is None else int(n_samples[i])) / SAMPLE_RATE
            segs = []
            for word in greedy_collapse(best[off[i]:off[i + 1]], self.blank, self.delimiter_id):
                word = [w for w in word if w[0] in self.char_of]          # (specials such as <unk> are not text)
                if not word:
                    continue
                text = "".join(self.char_of[c] for c, _, _ in word)
                segs.append([[float(fs[word[0][1]]) / SAMPLE_RATE, min(float(fs[word[-1][2]] + FRAME_STRIDE) / SAMPLE_RATE, total)], text])
            out.append(segs)
        return out

    def recording_frames(self, n, n_chunk):
        """How a recording of n samples goes through the encoder in chunks of n_chunk: -> (frames kept per chunk, frame_sample):
        the last chunk is zero-padded to n_chunk and keeps only the frames a recording of its true length would have."""
        full, rest = divmod(int(n), int(n_chunk))
        per = self.w2v.layout(n_chunk).T[-1]
        keep = [per] * full
        if rest >= FRAME_FIELD:
            keep.append(min(per, self.w2v.layout(rest).T[-1]))
        elif rest:
            keep.append(0)
        fs = np.concatenate([c * int(n_chunk) + FRAME_STRIDE * np.arange(k, dtype=np.int64) for c, k in enumerate(keep)]) if keep else np.zeros(0, np.int64)
        return keep, fs

    def align_recording(self, wave16k, transcript, chunk_seconds=10.0, return_frames=False):
        """A whole recording (16 kHz mono samples) and its transcript -> [[[start, end], word], ...]: what
        dataset.RawClip(annotations=dict(text_segments=...)) takes.  The encoder runs over consecutive chunks of chunk_seconds
        in one Wav2Vec2Features.batch call; the chunks' emissions are joined in time and aligned ONCE, so no word is cut at a
        chunk border."""
        wave = torch.as_tensor(wave16k).reshape(-1).float()
        n, n_chunk = wave.numel(), int(round(chunk_seconds * SAMPLE_RATE))
        keep, fs = self.recording_frames(n, n_chunk)
        if not len(fs):
            raise capi.RgError("align_recording: %d samples are too few for one emission frame" % n)
        padded = wave.new_zeros(len(keep) * n_chunk)
        padded[:n] = wave
        hidden = self.w2v.batch(padded.view(len(keep), n_chunk))
        rows = torch.cat([hidden[c, :k] for c, k in enumerate(keep)])
        segs = self.align([rows], [transcript], frame_sample=[fs], n_samples=[n])[0]
        return (segs, fs) if return_frames else segs
