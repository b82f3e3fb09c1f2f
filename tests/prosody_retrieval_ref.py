"""Float64 restatement of the `prosody` retrieval method (exemplars by word prominence), for the tests: pure Python / numpy,
nothing imported from the product's retrieval module.

The method is this project's own (the reference names it and raises NotImplementedError), so there is no reference arithmetic
to match: this file states the arithmetic a second time, independently of the HIP kernel and of the host code around it.

  database   per entry the list (cleaned lower-case word, start, end, prominence) and a speaker id
  queries    up to `max_queries` words of the clip, by descending prominence, at least `min_gap` seconds apart
  score      per (query word, entry), over the entry's words j with a finite prominence, in float64 and in this association:
                 s_j   = (4 / (1 + 2 |prom_j - p_q|) + 2 sim(word_j, query word)) + 1 / (1 + 4 |dur_j - dur_q|)
                 score = max_j s_j (the lowest j among equals) + (3 if the speakers are equal else 0),  top = that j
             and score 0, top -1 for an entry without such a word; sim = fuzzywuzzy's partial_ratio / 100 through difflib
  ranking    entries of score > 0 by descending score (stable in entry order), the leading tiers of bit-equal score while fewer
             than 10 are held, multi-member tiers reordered by descending text similarity (stable), the first 10
Every product of the score is by a power of two, hence exact; IEEE float64 division is correctly rounded: the device kernel
must give the same bits.
"""
from difflib import SequenceMatcher

import numpy as np

RANK_MAX = 10


def clean(s):
    return "".join(c for c in str(s) if c.isalnum() or c.isspace())


def wordprom(samples):
    """sample_name -> [(cleaned lower-case word, start, end, prominence)] of every prominence record with a cleanable word."""
    out = {}
    for smp in samples:
        rows = []
        for rec in smp["prominence"]:
            w = clean(rec[0]).lower()
            if w:
                rows.append((w, rec[1], rec[2], rec[3]))
        out[smp["sample_name"]] = rows
    return out


def prosody_queries(prominence, max_queries=3, min_gap=1.0, min_prominence=None, motion_seconds=10.0):
    """-> (query_bounds {i: (word, "prosody", start, end)} in ascending start order, [prominence of query i])."""
    cand = []
    for k, rec in enumerate(prominence):
        w, s, e, p = clean(rec[0]).lower(), float(rec[1]), float(rec[2]), rec[3]
        if p is None or not np.isfinite(float(p)):
            continue
        if min_prominence is not None and float(p) < min_prominence:
            continue
        if e > s and w != "" and s < motion_seconds and e > 0:
            cand.append((-float(p), s, k, w, e))
    cand.sort()                                   # descending prominence, then the earlier start, then list order
    held = []
    for negp, s, _, w, e in cand:
        if len(held) == max_queries:
            break
        if all(s >= he + min_gap or e <= hs - min_gap for _, hs, he, _ in held):
            held.append((w, s, e, -negp))
    held.sort(key=lambda h: h[1])
    return {i: (h[0], "prosody", h[1], h[2]) for i, h in enumerate(held)}, [h[3] for h in held]


def partial_ratio(s1, s2):
    """fuzzywuzzy 0.18 fuzz.partial_ratio in its pure-python (difflib) flavour."""
    if s1 == s2:
        return 100
    if len(s1) == 0 or len(s2) == 0:
        return 0
    shorter, longer = (s1, s2) if len(s1) <= len(s2) else (s2, s1)
    best = []
    for i, j, _ in SequenceMatcher(None, shorter, longer).get_matching_blocks():
        start = max(j - i, 0)
        r = SequenceMatcher(None, shorter, longer[start:start + len(shorter)]).ratio()
        if r > .995:
            return 100
        best.append(r)
    return int(round(100 * max(best)))


class Table:
    """The database as flat arrays: word_off [n + 1], word_code / word_prom / word_dur [W], spk [n], vocab (first-seen order)."""

    def __init__(self, entries, speakers):
        """entries: per entry [(word, start, end, prominence or None / NaN)]; speakers: per entry an int."""
        code, off, wc, wp, wd = {}, [0], [], [], []
        for rows in entries:
            for w, s, e, p in rows:
                wc.append(code.setdefault(w, len(code)))
                wp.append(float("nan") if p is None else float(p))
                wd.append(float(e) - float(s))
            off.append(len(wc))
        self.entries = [list(rows) for rows in entries]
        self.vocab = list(code)
        self.word_off = np.array(off, dtype=np.int64)
        self.word_code = np.array(wc, dtype=np.int64)
        self.word_prom = np.array(wp, dtype=np.float64)
        self.word_dur = np.array(wd, dtype=np.float64)
        self.spk = np.array(speakers, dtype=np.int64)
        self.n = len(self.entries)

    def sim_row(self, word):
        return np.array([partial_ratio(v, word) / 100 for v in self.vocab] or [0.0], dtype=np.float64)


def scores_loop(t, sim, p_q, dur_q, spk_q):
    """The definition, word by word: (score float64 [n], top int32 [n])."""
    score, top = np.zeros(t.n, dtype=np.float64), np.full(t.n, -1, dtype=np.int32)
    for e in range(t.n):
        best, at = None, -1
        for j in range(int(t.word_off[e]), int(t.word_off[e + 1])):
            p = t.word_prom[j]
            if not np.isfinite(p):
                continue
            s = (np.float64(4.0) / (1.0 + 2.0 * abs(p - p_q)) + 2.0 * sim[t.word_code[j]]) \
                + np.float64(1.0) / (1.0 + 4.0 * abs(t.word_dur[j] - dur_q))
            if best is None or s > best:
                best, at = s, j - int(t.word_off[e])
        if best is not None:
            score[e] = best + (3.0 if t.spk[e] == spk_q else 0.0)
            top[e] = at
    return score, top


def scores(t, sim, p_q, dur_q, spk_q):
    """The same, all words at once (numpy float64 elementwise arithmetic is the IEEE operation per element)."""
    score, top = np.zeros(t.n, dtype=np.float64), np.full(t.n, -1, dtype=np.int32)
    W = int(t.word_off[-1])
    if W == 0:
        return score, top
    s = (4.0 / (1.0 + 2.0 * np.abs(t.word_prom - p_q)) + 2.0 * sim[t.word_code]) + 1.0 / (1.0 + 4.0 * np.abs(t.word_dur - dur_q))
    s = np.where(np.isfinite(t.word_prom), s, -np.inf)
    counts = np.diff(t.word_off)
    full = np.flatnonzero(counts > 0)                       # (the words between two non-empty entries' starts are the first one's)
    starts = t.word_off[:-1][full]
    m = np.maximum.reduceat(s, starts)
    seg = np.repeat(np.arange(len(full)), counts[full])
    first = np.minimum.reduceat(np.where(s == m[seg], np.arange(W), W), starts)
    ok = m > -np.inf
    score[full[ok]] = m[ok] + np.where(t.spk[full[ok]] == spk_q, 3.0, 0.0)
    top[full[ok]] = (first - starts)[ok]
    return score, top


def text_similarity(q, f):
    """mean_i q[i] . f[i] over the common rows: fp32 products summed in float64."""
    n = min(q.shape[0], f.shape[0])
    if n == 0:
        return 0.0
    return float((np.asarray(q[:n], dtype=np.float32) * np.asarray(f[:n], dtype=np.float32)).astype(np.float64).sum() / n)


def ranking_walk(score, tie_sim):
    """score float64 [n]; tie_sim(entry) -> similarity.  Returns at most RANK_MAX entries."""
    order = sorted((e for e in range(len(score)) if score[e] > 0), key=lambda e: -score[e])     # stable: entry order inside a tier
    ranked, i = [], 0
    while i < len(order) and len(ranked) < RANK_MAX:
        j = i
        while j < len(order) and score[order[j]] == score[order[i]]:
            j += 1
        tier = order[i:j]
        if len(tier) > 1:
            sims = {e: tie_sim(e) for e in tier}
            tier = sorted(tier, key=lambda e: -sims[e])
        ranked += tier
        i = j
    return ranked[:RANK_MAX]


def retrieve(samples, prominence, speaker_id, text_features, **selection):
    """One clip against the database built from the raw records `samples` (synth.synth_retrieval_samples' shape):
    -> (sample_indexes, d_bounds, query_bounds) as the product's prosody_retrieval_batch returns them per clip."""
    wp = wordprom(samples)
    names = [smp["sample_name"] for smp in samples]
    t = Table([wp[n] for n in names], [int(smp["speaker_id"]) for smp in samples])
    feats = [np.asarray(smp["text_feature"], dtype=np.float32) for smp in samples]
    q_feat = np.asarray(text_features, dtype=np.float32)
    qb, proms = prosody_queries(prominence, **selection)
    sample_indexes, d_bounds = {}, {}
    for i in range(len(qb)):
        word, _, s, e = qb[i]
        score, top = scores(t, t.sim_row(word), proms[i], e - s, int(speaker_id))
        ranked = ranking_walk(score, lambda c: text_similarity(q_feat, feats[c]))
        sample_indexes[i] = [names[c] for c in ranked]
        d_bounds[i] = {}
        for c in ranked:
            w, ws, we, _ = t.entries[c][top[c]]
            d_bounds[i][names[c]] = (w, "prosody", round(ws, 3), round(we, 3))
    if not qb:
        return {}, {}, {}
    return sample_indexes, d_bounds, qb
