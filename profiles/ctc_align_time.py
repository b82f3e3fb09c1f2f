"""Word timings and word frames for 32 windows of 10 s (T = 499 emission frames, L = 200 target tokens each: 40 words and the
delimiters between them), random hidden states and a random CTC head (NOTEBOOK.md, "Word timings and frame-aligned word
features"):
  emissions_align  CTCAligner.emissions (the 768 -> 32 linear, rg_ctc_log_softmax) + rg_ctc_align, device events around the
                   launches; align_wall_s is a host clock around CTCAligner.align, which ends in its one read-back
  word_frames      rg_word_frames over the 32 windows' token rows (42 per window) onto 150 frames each
ROUNDS rounds after a warm-up.  Prints one JSON line; --out FILE also writes it.

    python profiles/ctc_align_time.py [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOWS, T, WORDS, ROUNDS = 32, 499, 40, 5
LETTERS = "ETAONIHSRDLUMWCFGYPBVK"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import transformers
    rg = importlib.import_module("rag-gesture_amd")
    vocab = {"<pad>": 0, "<s>": 1, "</s>": 2, "<unk>": 3, "|": 4}
    vocab.update({c: 5 + i for i, c in enumerate(LETTERS + "'XJQZ")})
    torch.manual_seed(0)
    w2v = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(num_hidden_layers=1)).eval()
    state = {"wav2vec2." + k: v for k, v in w2v.state_dict().items()}
    state.update({"lm_head.weight": torch.randn(32, 768) * 0.5, "lm_head.bias": torch.zeros(32)})
    aligner = rg.align.CTCAligner.from_state(state, vocab)
    # 39 words of four letters and one of five: 161 letters + 39 delimiters = 200 tokens
    words = ["".join(LETTERS[(5 * w + k) % len(LETTERS)] for k in range(5 if w == 0 else 4)) for w in range(WORDS)]
    assert len(aligner.tokens(words)[0]) == 200
    hidden = torch.randn(WINDOWS, T, 768, device="cuda")
    toks = [aligner.tokens(words)[0]] * WINDOWS
    off = [T * i for i in range(WINDOWS + 1)]
    ids = {}
    tok = lambda s: [101] + [ids.setdefault(w, 200 + len(ids)) for w in s.split()] + [102]
    bert = transformers.BertModel(transformers.BertConfig(vocab_size=500, num_hidden_layers=1), add_pooling_layer=False).eval()
    wf = rg.features.WindowFeatures(rg.features.BertFeatures(bert.state_dict()), aligner.w2v, tok, frame_words=True)
    rows = torch.randn(WINDOWS * (WORDS + 2), 768, device="cuda")
    roff = [(WORDS + 2) * i for i in range(WINDOWS + 1)]
    merged = [[[[0.24 * w, 0.24 * w + 0.2], word] for w, word in enumerate(words)]] * WINDOWS
    ev = lambda: torch.cuda.Event(enable_timing=True)
    out = dict(windows=WINDOWS, frames=T, tokens=200, emissions_align_ms=[], align_wall_s=[], word_frames_ms=[])
    for r in range(ROUNDS + 1):
        a, b, c, d = ev(), ev(), ev(), ev()
        a.record()
        logp, _ = aligner.emissions(hidden)
        res = rg.align.viterbi(aligner.h, logp.view(-1, 32), off, toks, aligner.blank)
        b.record()
        torch.cuda.synchronize()
        assert int(res["status"].sum()) == 0
        t0 = time.perf_counter()
        segs = aligner.align(hidden, [words] * WINDOWS)
        wall = time.perf_counter() - t0
        assert len(segs) == WINDOWS and len(segs[0]) == WORDS
        c.record()
        word = wf._frame_words(rows, roff, merged, [10.0] * WINDOWS)
        d.record()
        torch.cuda.synchronize()
        assert word[0].shape == (1, 150, 768)
        if r:                                                  # (round 0 warms every code object and shape)
            out["emissions_align_ms"].append(a.elapsed_time(b))
            out["align_wall_s"].append(wall)
            out["word_frames_ms"].append(c.elapsed_time(d))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
