"""Motion-exemplar retrieval: replicated DB on the GPU, discourse scoring sweep + text-similarity
tie-break as HIP reductions, exemplar placement and `re_dict` assembly.

Mirrors (names, argument meaning, result schema):
  mogen/models/transformers/raggesture.py:157-303 RetrievalDatabase.__init__ (DB dicts),
      :313-477 retrieve (method dispatch, self-exclusion, num_retrieval), :479-884 forward
      (exemplar fetch + VAE encode, placement, re_dict)
  mogen/models/transformers/rag/discourse_retrieval.py:8-316, rag/utils.py:86-132, 171-228
What runs where: string handling (connective cleaning, vocabulary coding, prominence matching) is
host string logic exactly as in the reference; the O(N_db) score sweep (float64, reference operation
order -> bit-identical scores) and the tie-break similarity reduction run on the GPU over an
integer-coded CSR copy of the DB (`DiscourseIndex`); the ranking walk over the sweep's survivors is
stated once, in the native library's host code (csrc/rg_retrieval_host.h), for all methods.  A fourth method, `prosody`
(exemplars by word prominence: ProsodyIndex, prosody_queries, prosody_retrieval_batch), is this project's own: the reference
names it and raises.
A fifth, `motion` (exemplars by a motion example: MotionIndex, motion_retrieval_batch), is this project's own too: the
reference has no counterpart.
The LMDB-backed cache of the reference (6 LMDB dicts) is replaced by in-memory dicts handed in by
the caller (`metadata=` or `dataset.retrieval_samples`); `lmdb` is not available in this image.
"""
import copy
import ctypes
import json
import os
import re

import numpy as np
import torch

from . import capi


def _clean(s):
    return "".join([c for c in str(s) if c.isalnum() or c.isspace()])


def map_conns_to_prominence(conn_list, prominence_list):
    """rag/utils.py:171-228: attach prominence values to connectives (multi-word = average)."""
    relevant = {}
    residual = copy.deepcopy(conn_list)
    for dp in prominence_list:
        dp_word = _clean(dp[0])
        for si, sc in enumerate(conn_list):
            if si not in relevant:
                relevant[si] = []
            if residual[si] is None:
                continue
            sc = _clean(sc)
            if dp_word == sc or dp_word in sc.split():
                relevant[si].append((sc, dp[3]))
                if dp_word == sc or dp_word == sc.split()[-1]:
                    residual[si] = None
                break
    for si, dps in relevant.items():
        if len(dps) > 1:
            if dps[0][0] != _clean(conn_list[si]):
                raise ValueError("prominence words do not spell the connective %r" % (conn_list[si],))
            relevant[si] = (conn_list[si], sum([d[1] for d in dps]) / len(dps))
        else:
            relevant[si] = dps[0] if len(dps) > 0 else None
    if len(relevant) != len(conn_list):  # the reference drops into a debugger here
        raise ValueError("prominence list does not cover the connective list (reference would trap)")
    return relevant


def build_db_dicts(samples, stratified_db_creation=False, stratification_interval=15):
    """raggesture.py:244-276: DB dicts from per-sample records (sample_name, speaker_id, discourse,
    prominence, text_feature[, gesture_labels]), in iteration order; with stratified_db_creation only the windows
    whose in-sequence index (the number behind "/" in sample_name) is a multiple of the interval are kept (:250-255).
    idx_2_wordprom is this project's addition (the `prosody` method's DB side, not one of the reference's six LMDB dicts):
    per sample the (cleaned lower-case word, start, end, prominence) of every prominence record whose word survives the
    cleaning, in the record's order and in the sample's own window seconds."""
    if stratified_db_creation:
        samples = [smp for smp in samples if int(smp["sample_name"].split("/")[1]) % stratification_interval == 0]
    idx_2_text, idx_2_sense, idx_2_discbounds, idx_2_prominence = {}, {}, {}, {}
    for smp in samples:
        n, spk = smp["sample_name"], int(smp["speaker_id"])
        idx_2_text[n] = (smp["text_feature"], spk)
        idx_2_sense[n] = [spk] + [(d[1], d[0]) for d in smp["discourse"]]
        idx_2_discbounds[n] = [(d[1], d[0], d[4], d[5], d[6], d[7]) for d in smp["discourse"]]
        idx_2_prominence[n] = map_conns_to_prominence([d[0] for d in smp["discourse"]], smp["prominence"])
    out = dict(idx_2_text=idx_2_text, idx_2_sense=idx_2_sense, idx_2_discbounds=idx_2_discbounds,
               idx_2_prominence=idx_2_prominence)
    out["idx_2_wordprom"] = {smp["sample_name"]: [(w, p[1], p[2], p[3]) for p in smp["prominence"]
                                                  for w in [_clean(p[0]).lower()] if w] for smp in samples}
    if all("gesture_labels" in smp for smp in samples):   # raggesture.py:262
        out["idx_2_gesture_labels"] = {smp["sample_name"]: [int(smp["speaker_id"])] + list(smp["gesture_labels"])
                                       for smp in samples}
        out["idx_2_gestprom"] = {}                        # raggesture.py:270-272 (llm method)
        for smp in samples:
            words = [g["word"] for g in smp["gesture_labels"]]
            out["idx_2_gestprom"][smp["sample_name"]] = map_conns_to_prominence(words, smp["prominence"]) if words else {}
    return out


def to_device_async(host, dev):
    """Host tensor / array -> device without stalling the host: staged in page-locked memory (torch's caching host
    allocator keeps the block until the copy has run), copied asynchronously on the current stream.  A copy from pageable
    memory instead returns only after everything queued on that stream before it has run -- on a stream that holds a
    just-launched VAE graph that is milliseconds of host time, per copy."""
    t = torch.from_numpy(np.ascontiguousarray(host)) if isinstance(host, np.ndarray) else host
    if t.device.type != "cpu" or torch.device(dev).type == "cpu":
        return t.to(dev)
    return t.pin_memory().to(dev, non_blocking=True)

class DiscourseIndex:
    """Integer-coded, device-resident copy of the discourse DB (replicated per GPU)."""

    def __init__(self, db, device="cuda"):
        self.dev = torch.device(device)
        self.h = capi.get_handle(self.dev.index if self.dev.index is not None else torch.cuda.current_device())
        self.db = db
        self.names = list(db["idx_2_sense"].keys())
        self.name_to_idx = {n: i for i, n in enumerate(self.names)}
        self.sense_code, self.conn_code = {}, {}
        spk, off, rs, rc, rp = [], [0], [], [], []
        for n in self.names:
            rec = db["idx_2_sense"][n]
            spk.append(int(rec[0]))
            prom = db["idx_2_prominence"][n]
            for k, (sense, conn) in enumerate(rec[1:]):
                rs.append(self.sense_code.setdefault(sense, len(self.sense_code)))
                rc.append(self.conn_code.setdefault(conn, len(self.conn_code)))
                pv = prom.get(k)
                rp.append(float("nan") if pv is None else float(pv[1]))
            off.append(len(rs))
        i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=self.dev)
        self.spk, self.rel_off, self.rel_sense, self.rel_conn = i32(spk), i32(off), i32(rs or [0]), i32(rc or [0])
        self.rel_prom = torch.tensor(rp or [0.0], dtype=torch.float64, device=self.dev)
        feats = [db["idx_2_text"][n][0].float() for n in self.names]
        foff = np.zeros(len(feats) + 1, dtype=np.int64)
        foff[1:] = np.cumsum([f.shape[0] for f in feats])
        self.feat_off = torch.from_numpy(foff).to(self.dev)
        self.feats = torch.cat(feats, dim=0).to(self.dev).contiguous()
        self.dim = self.feats.shape[1]
        self.n = len(self.names)

    def query_params(self, queries):
        """[(sense, conn, speaker_id, q_prom)] -> the sweep's float64 [Q, 4] parameter rows (codes are exact as doubles)."""
        nan = float("nan")
        return np.array([[float(self.sense_code.get(sense, -2)), float(self.conn_code.get(conn, -1)), float(int(spk)),
                          nan if q_prom is None else float(q_prom)] for sense, conn, spk, q_prom in queries],
                        dtype=np.float64).reshape(len(queries), 4)

    def sweep_buffers(self, queries):
        """Device buffers of one sweep over `queries` [(sense, conn, speaker_id, q_prom)]: the query parameters (uploaded
        asynchronously from pinned memory), the selection workspace and the survivor lists.
        sweep_buffers / sweep_launch / sweep_async / collect are the sweep on its own: the search does not go through them
        (search_batch sweeps inside its one native call); bench.py's retrieval roofline times the sweep with exactly these
        four, and the tests read the survivor lists through them."""
        Q, n = len(queries), self.n
        cap = n
        params = to_device_async(self.query_params(queries), self.dev)
        e = lambda *shape, dt=torch.int32: torch.empty(*shape, dtype=dt, device=self.dev)
        return dict(Q=Q, cap=cap, params=params, ws=e(Q, self.h.lib.rg_select_workspace_doubles(n), dt=torch.float64),
                    cursor=e(Q), idx=e(Q, cap), top=e(Q, cap), score=e(Q, cap, dt=torch.float64))

    def sweep_launch(self, bufs):
        """The launches of one sweep + device-side candidate selection on the current stream (no allocation, no copy, no
        synchronisation): rg_discourse_select_fused (two launches, scores in registers).  Returns the ticket for collect().
        (bench.py's roofline times this call.)"""
        self.h.call("discourse_select_fused", self.spk, self.rel_off, self.rel_sense, self.rel_conn, self.rel_prom, self.n,
                    bufs["params"], bufs["Q"], bufs["ws"], bufs["cursor"], bufs["cap"], bufs["idx"], bufs["top"], bufs["score"])
        return dict(cursor=bufs["cursor"], idx=bufs["idx"], top=bufs["top"], score=bufs["score"], keep=bufs)

    def sweep_async(self, queries):
        """Launch sweep + device-side candidate selection for a list of (sense, conn, speaker_id, q_prom)
        without any host synchronisation; returns a ticket for collect() (or, its device lists, for rank_survivors)."""
        return self.sweep_launch(self.sweep_buffers(queries))

    @staticmethod
    def collect(ticket):
        """One synchronisation for the whole batch: per query (entry idx ascending, score, top_rel_idx) on the host.  For
        bench.py's roofline and the tests; the search ranks the device lists natively (search_batch, rank_survivors)."""
        counts = ticket["cursor"].cpu().numpy()
        m = int(counts.max()) if counts.size else 0
        idx = ticket["idx"][:, :m].cpu().numpy()
        top = ticket["top"][:, :m].cpu().numpy()
        score = ticket["score"][:, :m].cpu().numpy()
        out = []
        for q, c in enumerate(counts):
            o = np.argsort(idx[q, :c], kind="stable")
            out.append((idx[q, :c][o], score[q, :c][o], top[q, :c][o]))
        return out

    def _ranked(self, name, head, q_feats):
        """rg_<name>(*head, the queries' feature table, the result arrays) on the current stream -> per query (ranked entry
        indices (at most 10), each one's top index) as lists; q_feats: per query its clip's fp32 [Lq, dim] device features."""
        Q = len(q_feats)
        qp = np.array([t.data_ptr() for t in q_feats], dtype=np.uint64)
        ql = np.array([t.shape[0] for t in q_feats], dtype=np.int32)
        n_ranked, entry, top = np.zeros(Q, dtype=np.int32), np.zeros((Q, 10), dtype=np.int32), np.zeros((Q, 10), dtype=np.int32)
        self.h.call(name, *head, qp.ctypes.data, ql.ctypes.data, n_ranked.ctypes.data, entry.ctypes.data, top.ctypes.data)
        entry, top = entry.tolist(), top.tolist()
        return [(entry[q][:k], top[q][:k]) for q, k in enumerate(n_ranked.tolist())]

    def search_batch(self, queries, q_feats):
        """The whole search of a batch in one native call (rg_discourse_search_batch, on the current stream): sweep, survivor
        pack, one read-back, the ranking on the host, one launch for every tie tier, one read-back, the tie-break walk.
        queries: [(sense, conn, speaker_id, q_prom)]; q_feats: per query relation its clip's fp32 [Lq, dim] device features.
        Returns per query relation (ranked entry indices (at most 10), each one's top relation index) as lists."""
        Q = len(queries)
        if Q == 0:
            return []
        capi.require(len(q_feats) == Q, "search_batch: one feature tensor per query relation")
        params = self.query_params(queries)
        return self._ranked("discourse_search_batch", (self.spk, self.rel_off, self.rel_sense, self.rel_conn, self.rel_prom, self.n,
                                                       self.feats, self.feat_off, self.dim, params.ctypes.data, Q), q_feats)

    def rank_survivors(self, cursor, idx, top, score, q_feats):
        """search_batch from its survivor pack on (rg_rank_survivors_batch, on the current stream), over the device survivor
        lists of any sweep over this index's entries (sweep_async's, or GestureTypeIndex.sweep's): cursor int32 [Q], idx / top
        int32 [Q, cap], score float64 [Q, cap].  Returns what search_batch returns."""
        Q, cap = idx.shape
        if Q == 0:
            return []
        capi.require(len(q_feats) == Q and cursor.numel() == Q and top.shape == idx.shape == score.shape,
                     "rank_survivors: one feature tensor and one survivor list per query")
        return self._ranked("rank_survivors_batch", (cursor, idx, top, score, Q, cap, self.feats, self.feat_off, self.n, self.dim),
                            q_feats)

    def pack_rows(self, rows=0):
        """Rows of the handle's survivor block (search_batch reads it back in one copy); rows > 0 sets it (tests)."""
        return int(self.h.lib.rg_retrieval_pack_rows(self.h._h, int(rows)))


def discourse_queries(discourse, prominence, speaker_id):
    """The (sense, connective, speaker, query prominence) tuples discourse_retrieval sweeps the DB with."""
    conns = [d[0] for d in discourse]
    q_prom = map_conns_to_prominence(conns, prominence)
    return [(d[1], d[0], speaker_id, None if q_prom[i] is None else q_prom[i][1]) for i, d in enumerate(discourse)]


def discourse_query_bounds(discourse):
    """query_bounds of discourse_retrieval (rag/discourse_retrieval.py:20-23): relation -> (connective, sense, start, end)."""
    return {i: (d[0].lower(), d[1], d[6], d[7]) for i, d in enumerate(discourse)}


def discourse_bounds(db, names):
    """Bounds getter of the discourse method for ranked_results: (entry, top relation index) -> the reported bounds."""
    def bounds(e, t):
        b = db["idx_2_discbounds"][names[e]][t]
        return (b[1], b[0], round(b[4], 3), round(b[5], 3))
    return bounds


def ranked_results(names, ranked, bounds, n_q=None):
    """ranked: per query (entries, tops) as DiscourseIndex.search_batch / rank_survivors return them; bounds(entry, top) ->
    the bounds reported for that entry.  Returns (sample_indexes, d_bounds) keyed 0.. as the reference's retrieval functions
    build them.  n_q (the motion method): per query the number of chunks of its example, handed to the getter as a third
    argument -- bounds(entry, top, n_q[query]).  Pure host code: needs no device."""
    sample_indexes, d_bounds = {}, {}
    for qi, (entries, tops) in enumerate(ranked):
        sample_indexes[qi] = [names[e] for e in entries]
        get = bounds if n_q is None else (lambda e, t, k=n_q[qi]: bounds(e, t, k))
        d_bounds[qi] = {names[e]: get(e, t) for e, t in zip(entries, tops)}
    return sample_indexes, d_bounds


def discourse_retrieval_batch(index, clips):
    """[(discourse, prominence, speaker_id, encoded_text)] -> per clip (sample_indexes, d_bounds, query_bounds): the search
    of every clip's query relations as ONE DiscourseIndex.search_batch call (two host synchronisations per batch)."""
    queries, feats, n_rel = [], [], []
    for discourse, prominence, speaker_id, encoded_text in clips:
        qs = discourse_queries(discourse, prominence, speaker_id) if len(discourse) else []
        if qs:
            feats += [encoded_text.to(index.dev).float().contiguous()] * len(qs)
        queries += qs
        n_rel.append(len(qs))
    ranked = index.search_batch(queries, feats)
    bounds = discourse_bounds(index.db, index.names)
    out, pos = [], 0
    for (discourse, _, _, _), n in zip(clips, n_rel):
        si, db_b = ranked_results(index.names, ranked[pos:pos + n], bounds)
        out.append((si, db_b, discourse_query_bounds(discourse)))
        pos += n
    return out


def discourse_retrieval(index, discourse, prominence, speaker_id, encoded_text):
    """Same contract as rag/discourse_retrieval.py:8-316 (returns sample_indexes, d_bounds,
    query_bounds) with the DB sweep, the candidate selection and the tie-break similarity on the GPU:
    one clip through discourse_retrieval_batch."""
    return discourse_retrieval_batch(index, [(discourse, prominence, speaker_id, encoded_text)])[0]


_NEP50 = int(np.__version__.split(".")[0]) >= 2


def partial_ratio_host(s1, s2):
    """fuzzywuzzy 0.18 `fuzz.partial_ratio`, pure-python flavour (the package calls difflib.SequenceMatcher when
    python-Levenshtein is absent, as in the reference's requirements.txt).  Host form of rg_partial_ratio: used for
    single pairs and for strings longer than the kernel handles."""
    from difflib import SequenceMatcher
    if s1 is None or s2 is None:
        return 0
    if s1 == s2:
        return 100
    if len(s1) == 0 or len(s2) == 0:
        return 0
    shorter, longer = (s1, s2) if len(s1) <= len(s2) else (s2, s1)
    scores = []
    for i, j, _ in SequenceMatcher(None, shorter, longer).get_matching_blocks():
        start = j - i if j - i > 0 else 0
        r = SequenceMatcher(None, shorter, longer[start:start + len(shorter)]).ratio()
        if r > .995:
            return 100
        scores.append(r)
    return int(round(100 * max(scores)))


def fuzzy_word_similarity(db_word, query_word):
    """The reference's get_word_similarity_score as it effectively behaves (rag/utils.py:239-272): its word2vec /
    fasttext models are never defined, every call raises inside the `try` and returns
    `fuzz.partial_ratio(word1, word2) / 100`.  This is the DEFAULT `word_similarity` of RetrievalDatabase; whole
    vocabularies go through the device form (rg_partial_ratio) in GestureTypeIndex.sweep."""
    return partial_ratio_host(db_word, query_word) / 100


class FuzzyVocabulary:
    """A vocabulary of DB words as code-point rows on the device, for rg_partial_ratio (the default word similarity): what
    GestureTypeIndex and ProsodyIndex each keep of their own words."""

    def __init__(self, words, h, dev):
        self.words, self.h, self.dev = list(words), h, dev
        self.pr_max = int(h.lib.rg_partial_ratio_max_len())
        codes = np.zeros((max(1, len(self.words)), self.pr_max), dtype=np.int32)
        lens = np.zeros(max(1, len(self.words)), dtype=np.int32)
        for v, w in enumerate(self.words):
            lens[v] = len(w)
            cp = [ord(ch) for ch in w[:self.pr_max]]
            codes[v, :len(cp)] = cp
        self.codes, self.lens = torch.from_numpy(codes).to(dev), torch.from_numpy(lens).to(dev)

    def similarities(self, words):
        """[len(words), max(1, len(vocabulary))] float64 on the device: partial_ratio(vocabulary word, query word) / 100 for
        every query word, one rg_partial_ratio launch each; pairs with a string beyond the kernel's length are patched from
        the host."""
        V = max(1, len(self.words))
        out = torch.empty(len(words), V, dtype=torch.float64, device=self.dev)
        for q, word in enumerate(words):
            cp = (ctypes.c_int * max(1, len(word)))(*[ord(ch) for ch in word])
            self.h.call("partial_ratio", self.codes, self.lens, V, self.pr_max, cp, len(word), out[q])
        long_rows = [v for v, w in enumerate(self.words) if len(w) > self.pr_max]
        for q, word in enumerate(words):
            rows = range(len(self.words)) if len(word) > self.pr_max else long_rows
            for v in rows:
                out[q, v] = fuzzy_word_similarity(self.words[v], word)
        if not self.words:
            out.zero_()
        return out


class GestureTypeIndex:
    """Device copy of the DB's semantic gesture labels (raggesture.py:262 idx_2_gesture_labels, beat labels dropped
    like gesture_type_retrieval.py:57-59 does): CSR over entries with integer-coded types and words.  Shares the
    entry order, names and text-feature table (tie-break) with a DiscourseIndex."""

    def __init__(self, db, base):
        self.base, self.dev, self.h, self.n = base, base.dev, base.h, base.n
        self.type_code, self.word_code, self.labels = {}, {}, []
        spk, off, lt, lw, lp = [], [0], [], [], []
        gestprom = db.get("idx_2_gestprom")
        for n in base.names:
            rec = db["idx_2_gesture_labels"][n]
            spk.append(int(rec[0]))
            labs = [g for g in rec[1:] if g["name"] != "beat"]
            self.labels.append(labs)
            for g in labs:
                lt.append(self.type_code.setdefault(g["name"], len(self.type_code)))
                lw.append(self.word_code.setdefault(g["word"], len(self.word_code)))
            off.append(len(lt))
            if gestprom is not None:      # aligned with ALL labels of the sample (beat included), llm_retrieval.py:293-299
                for gi, g in enumerate(rec[1:]):
                    if g["name"] != "beat":
                        pv = gestprom[n][gi]
                        lp.append(float("nan") if pv is None else float(pv[1]))
        i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=self.dev)
        self.spk, self.lab_off, self.lab_type, self.lab_word = i32(spk), i32(off), i32(lt or [0]), i32(lw or [0])
        self.lab_prom = None if gestprom is None else torch.tensor(lp or [0.0], dtype=torch.float64, device=self.dev)
        self.vocab = list(self.word_code.keys())
        self.fuzzy = FuzzyVocabulary(self.vocab, self.h, self.dev)   # code-point rows for rg_partial_ratio

    def fuzzy_similarities(self, words):
        """[len(words), len(vocab)] float64 on the device: partial_ratio(vocab word, query word) / 100 for every query
        word (FuzzyVocabulary.similarities)."""
        return self.fuzzy.similarities(words)

    def sweep(self, queries, word_similarity, spk_bonus=2.0, proms=None):
        """[(type, word, speaker_id)] (+ per-query prominence, None = unknown: the llm method) -> the device survivor lists
        (cursor [Q], idx / top / score [Q, n]: entry, top label index and score of the entries that can be visited, as
        DiscourseIndex.rank_survivors takes them); the word-similarity vector of each query word is computed here (host: the
        similarity model is the caller's), the scores and the selection on the device; nothing is read back."""
        Q, n = len(queries), self.n
        nws = self.h.lib.rg_select_workspace_doubles(n)
        score = torch.empty(Q, n, dtype=torch.float64, device=self.dev)
        top = torch.empty(Q, n, dtype=torch.int32, device=self.dev)
        ws = torch.empty(Q, nws, dtype=torch.float64, device=self.dev)
        cursor = torch.zeros(Q, dtype=torch.int32, device=self.dev)
        o_idx = torch.empty(Q, n, dtype=torch.int32, device=self.dev)
        o_top = torch.empty(Q, n, dtype=torch.int32, device=self.dev)
        o_score = torch.empty(Q, n, dtype=torch.float64, device=self.dev)
        if word_similarity is fuzzy_word_similarity:
            # the reference's effective similarity (python floats -> float64 scores): whole vocabulary on the device
            sims = self.fuzzy_similarities([q[1] for q in queries])
            f32 = [0] * Q
        else:
            raw = [[word_similarity(w, q[1]) for w in self.vocab] or [0.0] for q in queries]
            # float32 similarities make the reference's score float32 only under NumPy >= 2 promotion rules (NEP 50); the
            # reference pins numpy < 1.24, where scalar-scalar arithmetic promotes to float64: follow the installed numpy
            f32 = [int(_NEP50 and any(isinstance(v, np.float32) for v in row)) for row in raw]
            sims = torch.tensor([[float(v) for v in row] for row in raw], dtype=torch.float64, device=self.dev)
        if proms is not None and self.lab_prom is None:
            raise capi.RgError("llm retrieval needs idx_2_gestprom in the DB metadata (raggesture.py:270-272)")
        nan = float("nan")
        for q, (q_type, q_word, speaker_id) in enumerate(queries):
            self.h.call("gesture_scores", self.spk, self.lab_off, self.lab_type, self.lab_word,
                        self.lab_prom if proms is not None else None, sims[q], n, self.type_code.get(q_type, -2),
                        self.word_code.get(q_word, -1), int(speaker_id), float(spk_bonus),
                        nan if proms is None or proms[q] is None else float(proms[q]), f32[q], score[q], top[q])
            self.h.call("select_top_scores", score[q], top[q], n, ws[q], cursor[q:], n, o_idx[q], o_top[q], o_score[q])
        return dict(cursor=cursor, idx=o_idx, top=o_top, score=o_score)

    def bounds(self, e, t):
        """Bounds getter of the gesture_type / llm methods for ranked_results: (entry, top label index) -> the reported bounds."""
        b = self.labels[e][t]
        return (b["word"], b["name"], round(b["start"], 3), round(b["end"], 3))


def gesture_type_retrieval(gindex, gesture_labels, speaker_id, encoded_text, word_similarity):
    """Same contract as rag/gesture_type_retrieval.py:8-176 (sample_indexes, d_bounds, query_gest_bounds); the DB
    sweep, the candidate selection and the tie-break text similarity run on the GPU, `word_similarity(db_word,
    query_word)` is the reference's get_word_similarity_score (an external embedding model: supplied by the caller)."""
    gesture_labels = [g for g in gesture_labels if g["name"] != "beat"]
    d_bounds, sample_indexes, query_bounds = {}, {}, {}
    if len(gesture_labels) == 0:
        return sample_indexes, d_bounds, query_bounds
    query_bounds = {i: (g["word"].lower(), g["name"], g["start"], g["end"]) for i, g in enumerate(gesture_labels)}
    sample_indexes, d_bounds = _gesture_ranked(gindex, [(g["name"], g["word"], speaker_id) for g in gesture_labels],
                                               encoded_text, word_similarity, 2.0, None)
    return sample_indexes, d_bounds, query_bounds


def _clean_str(s):
    return "".join([c for c in s if c.isalnum() or c.isspace()])


def llm_query_bounds(gesture_labels, text_times):
    """rag/llm_retrieval.py:191-262: align the LLM's (word, type) labels with the clip's word timings
    [((start, end), word), ...]; multi-word labels span their words, a label is closed by its last word, the result is
    keyed 0.. in order of first occurrence in the text."""
    q_types = [g["name"] for g in gesture_labels]
    q_words = [_clean_str(g["word"].lower()) for g in gesture_labels]
    open_, spans = [True] * len(q_words), {}
    for (t_start, t_end), t_word in ((t[0], t[1]) for t in text_times):
        t_word = _clean_str(t_word.lower())
        for qi, q_word in enumerate(q_words):
            if not open_[qi]:
                continue
            parts = q_word.split()
            if q_word == t_word or t_word in parts:
                spans.setdefault(qi, []).append((t_start, t_end))
                if q_word == t_word or t_word == parts[-1]:
                    open_[qi] = False
                break
    return {k: (q_words[qi], q_types[qi], min(a for a, _ in sp), max(b for _, b in sp))
            for k, (qi, sp) in enumerate(spans.items())}


def llm_retrieval(gindex, text, text_times, speaker_id, prominence, encoded_text, word_similarity, llm_output):
    """Same contract as rag/llm_retrieval.py:166-466; `llm_output(text) -> str` replaces get_llm_output (the GPT
    call: use LLMResponseCache.get), the label alignment is host string work, the DB sweep (type / speaker / word /
    prominence score), selection and tie-break run on the GPU."""
    if text.strip() == "":
        return {}, {}, {}
    labels = parse_gesture_labels_from_llm_output(llm_output(text))
    if len(labels) == 0:
        return {}, {}, {}
    query_bounds = llm_query_bounds(labels, text_times)
    if len(query_bounds) == 0:
        return {}, {}, {}
    nq = len(query_bounds)
    q_types, q_words = [query_bounds[i][1] for i in range(nq)], [query_bounds[i][0] for i in range(nq)]
    q_prom = map_conns_to_prominence(q_words, prominence)
    proms = [None if q_prom[i] is None else q_prom[i][-1] for i in range(nq)]
    si, db_b = _gesture_ranked(gindex, [(t, w, speaker_id) for t, w in zip(q_types, q_words)], encoded_text,
                               word_similarity, 1.0, proms)
    return si, db_b, query_bounds


def _gesture_ranked(gindex, queries, encoded_text, word_similarity, spk_bonus, proms):
    """The labels' sweep, then the ranking of its device survivor lists (every label against this clip's features)."""
    base = gindex.base
    q_dev = encoded_text.to(base.dev).float().contiguous()
    swept = gindex.sweep(queries, word_similarity, spk_bonus, proms)
    ranked = base.rank_survivors(swept["cursor"], swept["idx"], swept["top"], swept["score"], [q_dev] * len(queries))
    return ranked_results(base.names, ranked, gindex.bounds)


# ------------------------------------------------------------------------------------- the prosody method (this project's own)
# The reference names a fourth retrieval method, `prosody`, hands it the query's audio and prominence list and raises
# NotImplementedError (raggesture.py:426-431; rag/prosodic_prominence.py is empty).  What follows is NOT the reference's
# arithmetic: it is this project's scoring over what align.py and prosody.py produce (timed words and their prominence), built
# from the reference's prominence term 4 / (1 + 2 |dp|) and its ranking walk.  Query and DB must be annotated by the same
# estimator (prosody.ProminenceEstimator's scale is its own).  How good the exemplars are on real speech is not claimed.
class ProsodyIndex:
    """Device copy of the DB's timed, prominence-annotated words (build_db_dicts' idx_2_wordprom): CSR over entries with
    word_off int32 [n + 1], word_code int32 [W] (index into the vocabulary of distinct cleaned words), word_prom float64 [W]
    (NaN = unknown), word_dur float64 [W] (end - start, computed on the host in float64) and spk int32 [n].  Shares the entry
    order, names, handle and text-feature table (tie-break) with the DiscourseIndex `base`."""

    def __init__(self, db, base):
        self.base, self.dev, self.h, self.n = base, base.dev, base.h, base.n
        self.word_code_of, self.words = {}, []
        off, wc, wp, wd = [0], [], [], []
        for n in base.names:
            rec = [(str(w), float(s), float(e), float("nan") if p is None else float(p)) for w, s, e, p in db["idx_2_wordprom"][n]]
            self.words.append(rec)
            for w, s, e, p in rec:
                wc.append(self.word_code_of.setdefault(w, len(self.word_code_of)))
                wp.append(p)
                wd.append(e - s)
            off.append(len(wc))
        self.spk = base.spk
        self.n_words = len(wc)
        self.word_off_host = np.array(off, dtype=np.int32)
        self.word_off = torch.from_numpy(self.word_off_host).to(self.dev)
        self.word_code = torch.tensor(wc or [0], dtype=torch.int32, device=self.dev)
        self.word_prom = torch.tensor(wp or [0.0], dtype=torch.float64, device=self.dev)
        self.word_dur = torch.tensor(wd or [0.0], dtype=torch.float64, device=self.dev)
        self.vocab = list(self.word_code_of.keys())
        self.fuzzy = FuzzyVocabulary(self.vocab, self.h, self.dev)

    def scores(self, queries):
        """[(cleaned word, prominence, duration, speaker_id)] -> (score float64 [Q, n], top int32 [Q, n]) on the device:
        one rg_partial_ratio launch per distinct query word, then ONE rg_prosody_scores_batched launch; nothing is read back."""
        Q, n = len(queries), self.n
        distinct = list(dict.fromkeys(q[0] for q in queries))
        rows = self.fuzzy.similarities(distinct)
        if len(distinct) != Q:
            pick = [distinct.index(q[0]) for q in queries]
            rows = rows.index_select(0, to_device_async(np.array(pick, dtype=np.int64), self.dev))
        params = to_device_async(np.array([[float(p), float(d), float(int(spk))] for _, p, d, spk in queries],
                                          dtype=np.float64).reshape(Q, 3), self.dev)
        score = torch.empty(Q, n, dtype=torch.float64, device=self.dev)
        top = torch.empty(Q, n, dtype=torch.int32, device=self.dev)
        self.h.call("prosody_scores_batched", self.spk, self.word_off, self.word_off_host.ctypes.data, self.word_code,
                    self.word_prom, self.word_dur, n, self.n_words, rows.contiguous(), rows.shape[1], params, Q, score, top)
        return score, top

    def sweep(self, queries):
        """scores + rg_select_top_scores_batched -> the device survivor lists DiscourseIndex.rank_survivors takes."""
        Q, n = len(queries), self.n
        score, top = self.scores(queries)
        e = lambda *shape, dt=torch.int32: torch.empty(*shape, dtype=dt, device=self.dev)
        out = dict(cursor=e(Q), idx=e(Q, n), top=e(Q, n), score=e(Q, n, dt=torch.float64))
        ws = e(Q, self.h.lib.rg_select_workspace_doubles(n), dt=torch.float64)
        self.h.call("select_top_scores_batched", score, top, n, Q, ws, out["cursor"], n, out["idx"], out["top"], out["score"])
        return out

    def bounds(self, e, t):
        """Bounds getter for ranked_results: (entry, top word index) -> the reported bounds."""
        w, s, en, _ = self.words[e][t]
        return (w, "prosody", round(s, 3), round(en, 3))


def prosody_queries(prominence, max_queries=3, min_gap=1.0, min_prominence=None, motion_seconds=10.0):
    """The query words of one clip for the prosody method, from its prominence list [(word, start, end, value)]: candidates
    have a finite prominence (>= min_prominence if given), end > start, a word that survives cleaning, and overlap the clip
    (start < motion_seconds, end > 0); they are visited by descending prominence (ties: the earlier start) and accepted while
    at least `min_gap` seconds clear of every accepted word, until `max_queries` are held.  (One latent chunk is 15 frames at
    15 fps = 1 s: the default gap keeps two query words out of one chunk.)
    Returns (query_bounds, proms): query_bounds[i] = (cleaned lower-case word, "prosody", start, end) keyed 0.. in ascending
    start order (place_exemplars walks the query points with a running end), proms[i] the word's prominence."""
    cand = []
    for rec in prominence or []:
        w, s, e, p = _clean(rec[0]).lower(), float(rec[1]), float(rec[2]), rec[3]
        p = float("nan") if p is None else float(p)
        if not np.isfinite(p) or (min_prominence is not None and p < min_prominence):
            continue
        if not (e > s and w and s < motion_seconds and e > 0):
            continue
        cand.append((w, s, e, p))
    held = []
    for c in sorted(cand, key=lambda c: (-c[3], c[1])):
        if len(held) >= max_queries:
            break
        if all(c[1] >= h[2] + min_gap or c[2] <= h[1] - min_gap for h in held):
            held.append(c)
    held.sort(key=lambda c: c[1])
    return {i: (c[0], "prosody", c[1], c[2]) for i, c in enumerate(held)}, [c[3] for c in held]


def prosody_retrieval_batch(pindex, clips, max_queries=3, min_gap=1.0, min_prominence=None, motion_seconds=10.0):
    """[(prominence, speaker_id, text_features)] -> per clip (sample_indexes, d_bounds, query_bounds), the contract of the
    reference's retrieval functions; a clip without a query word gives three empty dicts.  The query words of every clip go
    through ONE sweep launch and one selection; the ranking (tier cut, text-similarity tie-break) is rank_survivors'."""
    picked = [prosody_queries(prom, max_queries, min_gap, min_prominence, motion_seconds) for prom, _, _ in clips]
    queries, feats = [], []
    for (_, speaker_id, text_features), (qb, proms) in zip(clips, picked):
        if qb:
            feats += [text_features.to(pindex.dev).float().contiguous()] * len(qb)
        queries += [(qb[i][0], proms[i], qb[i][3] - qb[i][2], speaker_id) for i in range(len(qb))]
    if not queries:
        return [({}, {}, {}) for _ in clips]
    swept = pindex.sweep(queries)
    ranked = pindex.base.rank_survivors(swept["cursor"], swept["idx"], swept["top"], swept["score"], feats)
    out, pos = [], 0
    for qb, _ in picked:
        if not qb:
            out.append(({}, {}, {}))
            continue
        si, db_b = ranked_results(pindex.base.names, ranked[pos:pos + len(qb)], pindex.bounds)
        out.append((si, db_b, qb))
        pos += len(qb)
    return out


# -------------------------------------------------------------------------------------- the motion method (this project's own)
# Exemplars by a motion example: "put a gesture like THIS at second 4".  The reference has no counterpart -- method, scoring and
# arithmetic are this project's.  A caller's snippet cannot be spliced in as an exemplar (an exemplar is DDIM-inverted under
# its own text, audio and speaker, and a snippet has none), so the search finds the database window position whose VAE posterior
# means are nearest to the snippet's, and that entry is the exemplar.  How good the found exemplars are on real motion is not
# measured and not claimed.  Long-form synthesis does not offer the method: its window annotations cannot carry examples yet.
MOTION_PARTS = ("upper", "hands", "face", "lowertrans")       # the model's part order (diffusion_architecture.py:146-149)
MOTION_DEFAULT_WEIGHTS = (1.0, 1.0, 0.0, 0.0)                 # upper body and hands; see motion_query_fields on the lower part
MOTION_EXAMPLE_KEYS = ("motion_upper", "motion_lower", "motion_face", "motion_hands", "trans", "facial", "contact")


def motion_query_fields(query, chunk=15, n_lat=10, where="motion query"):
    """One entry of conditions["motion_queries"][b], (start_s, end_s, example[, weights]), checked on the host ->
    (start_s, end_s, example, weights as four floats, n_q).  example: the seven per-frame tensors of MOTION_EXAMPLE_KEYS at the
    pose rate, chunk * n_q frames each with 1 <= n_q <= n_lat.  weights: four finite, non-negative numbers over MOTION_PARTS,
    not all zero; default upper body and hands only.  (The lower part's input carries the root translation relative to the FIRST
    FRAME OF THE ENCODED SPAN -- a database window's first frame, but an example's own first frame -- so an example cut from
    the middle of a window does not reproduce that window's lower-part latents; weigh it only for examples whose translation is
    expressed the way a window's is.)  A bad query raises ValueError with `where` in front."""
    def bad(msg):
        return ValueError("%s: %s" % (where, msg))
    if not isinstance(query, (tuple, list)) or len(query) not in (3, 4):
        raise bad("expected (start_s, end_s, example[, weights])")
    start_s, end_s, example = float(query[0]), float(query[1]), query[2]
    if not (np.isfinite(start_s) and np.isfinite(end_s) and start_s <= end_s):
        raise bad("start_s must be <= end_s (got %r, %r)" % (query[0], query[1]))
    missing = [k for k in MOTION_EXAMPLE_KEYS if not isinstance(example, dict) or k not in example]
    if missing:
        raise bad("the example lacks %s" % ", ".join(missing))
    frames = {int(example[k].shape[0]) for k in MOTION_EXAMPLE_KEYS}
    if len(frames) != 1:
        raise bad("the example's tensors hold different numbers of frames %s" % sorted(frames))
    frames = frames.pop()
    if frames % chunk != 0:
        raise bad("the example holds %d frames, not a multiple of the %d-frame chunk" % (frames, chunk))
    n_q = frames // chunk
    if not 1 <= n_q <= n_lat:
        raise bad("the example holds %d chunks, expected 1 ... %d" % (n_q, n_lat))
    w = MOTION_DEFAULT_WEIGHTS if len(query) == 3 or query[3] is None else tuple(float(v) for v in query[3])
    if len(w) != len(MOTION_PARTS):
        raise bad("weights: one per part %s expected, got %d" % (MOTION_PARTS, len(w)))
    if not all(np.isfinite(v) and v >= 0 for v in w):
        raise bad("weights must be finite and non-negative, got %r" % (w,))
    if not any(v > 0 for v in w):
        raise bad("weights must not all be zero")
    return start_s, end_s, example, tuple(w), n_q


def pack_motion_queries(qlats, weights, speakers, bonuses, dev):
    """Per query its latents (fp32 [4, n_q, D], any device), four part weights, a speaker id and a speaker bonus -> the
    argument arrays of rg_motion_scores_batched: qlat (one ragged device array), q_off / params on the device and the host."""
    q_off = np.zeros(len(qlats) + 1, dtype=np.int32)
    q_off[1:] = np.cumsum([int(t.shape[1]) for t in qlats])
    params = np.array([[float(v) for v in w] + [float(int(s)), float(b)] for w, s, b in zip(weights, speakers, bonuses)],
                      dtype=np.float64).reshape(len(qlats), 6)
    qlat = torch.cat([t.to(dev).float().reshape(-1) for t in qlats]) if qlats else torch.zeros(0, device=dev)
    return dict(qlat=qlat.contiguous(), q_off_host=q_off, q_off=to_device_async(q_off, dev), params_host=params,
                params=to_device_async(params, dev), Q=len(qlats))


class MotionIndex:
    """The database's motion latents on the device: `lat` fp32 [n_entries, 4, L, D], contiguous -- per entry (the DiscourseIndex's
    order) and part (MOTION_PARTS) the VAE posterior MEAN of each of its L = max_seq_len // motion_framechunksize chunks: 80 KiB
    per entry at L = 10, D = 512, 2.7 GB at 32 768 entries.  Shares handle, names, `spk` and the text-feature table (tie-break)
    with the DiscourseIndex `base`.  There is no eviction: build() refuses a database beyond its byte budget."""

    def __init__(self, base, lat, chunk=15, fps=15):
        capi.require(lat.dim() == 4 and lat.shape[0] == base.n and lat.shape[1] == len(MOTION_PARTS) and lat.dtype == torch.float32
                     and lat.is_contiguous() and lat.device == base.feats.device, "MotionIndex: lat must be a contiguous fp32 "
                     "[n_entries, 4, L, D] tensor on the index's device")
        self.base, self.dev, self.h, self.n, self.spk = base, base.dev, base.h, base.n, base.spk
        self.lat, self.L, self.D, self.chunk, self.fps = lat, int(lat.shape[2]), int(lat.shape[3]), int(chunk), int(fps)

    @staticmethod
    def table_bytes(n_entries, n_lat, latent_dim):
        return int(n_entries) * len(MOTION_PARTS) * int(n_lat) * int(latent_dim) * 4

    @classmethod
    def build(cls, base, gre, fetch, n_lat, chunk=15, fps=15, motion_index_bytes=4 << 30, batch=64):
        """Encode every entry of `base` (fetch(name) -> its record, as db.dataset[name]) with the posterior-only launches the
        exemplar cache warms itself with (GestureRepEncoder.encode_posteriors), `batch` entries per call, and keep the means."""
        n, D = base.n, gre.vae_latent_dim
        need = cls.table_bytes(n, n_lat, D)
        if need > int(motion_index_bytes):
            raise capi.RgError("MotionIndex: %d entries need %d bytes of motion latents, motion_index_bytes allows %d (there is "
                               "no eviction: raise the budget or search a smaller database)" % (n, need, int(motion_index_bytes)))
        lat = torch.empty(n, len(MOTION_PARTS), n_lat, D, device=base.dev)
        R = len(MOTION_PARTS) * n_lat
        for i in range(0, n, batch):
            names = base.names[i:i + batch]
            mu = posterior_means(gre, [fetch(name) for name in names], n_lat, chunk)
            lat[i:i + len(names)].view(len(names) * R, D).copy_(mu)
        return cls(base, lat, chunk, fps)

    def scores(self, queries, with_sums=False):
        """queries: pack_motion_queries' dict, or a list of (qlat fp32 [4, n_q, D], weights, speaker_id, bonus) ->
        (score float64 [Q, n], top int32 [Q, n]) on the device (and, with_sums, S_p(o*) fp32 [Q, n, 4]): ONE
        rg_motion_scores_batched launch; nothing is read back."""
        if not isinstance(queries, dict):
            queries = pack_motion_queries([q[0] for q in queries], [q[1] for q in queries], [q[2] for q in queries],
                                          [q[3] for q in queries], self.dev)
        Q, n = queries["Q"], self.n
        score = torch.empty(Q, n, dtype=torch.float64, device=self.dev)
        top = torch.empty(Q, n, dtype=torch.int32, device=self.dev)
        sums = torch.empty(Q, n, len(MOTION_PARTS), dtype=torch.float32, device=self.dev) if with_sums else None
        self.h.call("motion_scores_batched", self.lat, n, self.L, self.D, self.spk, queries["qlat"], queries["q_off"],
                    queries["q_off_host"].ctypes.data, queries["params"], queries["params_host"].ctypes.data, Q, score, top, sums)
        return (score, top, sums) if with_sums else (score, top)

    def sweep(self, queries):
        """scores + rg_select_top_scores_batched -> the device survivor lists DiscourseIndex.rank_survivors takes."""
        score, top = self.scores(queries)
        Q, n = score.shape
        e = lambda *shape, dt=torch.int32: torch.empty(*shape, dtype=dt, device=self.dev)
        out = dict(cursor=e(Q), idx=e(Q, n), top=e(Q, n), score=e(Q, n, dt=torch.float64))
        ws = e(Q, self.h.lib.rg_select_workspace_doubles(n), dt=torch.float64)
        self.h.call("select_top_scores_batched", score, top, n, Q, ws, out["cursor"], n, out["idx"], out["top"], out["score"])
        return out

    def bounds(self, e, t, n_q):
        """Bounds getter for ranked_results: (entry, best offset o*, the query's chunks) -> the reported bounds, the seconds of
        chunks o* ... o* + n_q of the entry's window."""
        return ("motion", "motion", t * self.chunk / self.fps, (t + n_q) * self.chunk / self.fps)


def posterior_means(gre, recs, n_lat, chunk=15):
    """fp32 [len(recs) * 4 * n_lat, D] on the device: the posterior means of the records' chunks, record-major, then part
    (MOTION_PARTS), then chunk -- one GestureRepEncoder.encode_posteriors call, padded to a multiple of 4 records as the
    exemplar cache pads (padding = copies of the first record, stored nowhere)."""
    dev, D, M = gre.dev, gre.vae_latent_dim, len(recs)
    Mp = -(-M // 4) * 4
    R = len(MOTION_PARTS) * n_lat
    rows = np.full((len(MOTION_PARTS), Mp * n_lat), -1, dtype=np.int32)
    for m in range(M):
        for p in range(len(MOTION_PARTS)):
            rows[p, m * n_lat:(m + 1) * n_lat] = m * R + p * n_lat + np.arange(n_lat)
    pick = list(range(M)) + [0] * (Mp - M)
    stack = lambda k: torch.stack([recs[m][k] for m in pick]).to(dev).float().contiguous()
    capi.require(stack("motion_upper").shape[1] == n_lat * chunk, "motion index: frames per record != n_lat chunks")
    mu, logvar = (torch.empty(M * R, D, device=dev) for _ in range(2))
    gre.encode_posteriors(stack("motion_upper"), stack("motion_lower"), stack("motion_face"), stack("motion_hands"),
                          stack("trans"), stack("facial"), stack("contact"), to_device_async(rows, dev), mu, logvar)
    return mu


def example_latents(gre, examples, n_lat, chunk=15):
    """examples: [(example dict of MOTION_EXAMPLE_KEYS, n_q)] -> (qlat, q_off): the posterior means of every example's chunks as
    ONE ragged fp32 device array (example i owns the 4 n_q D floats behind float 4 D q_off[i], laid out [4][n_q][D]) and the
    int32 [Q + 1] chunk offsets on the host.  All examples go through ONE encode_posteriors call: each is padded with zero
    frames to a whole window of its own (the call takes whole windows; in a window of its own an example's translation stays
    relative to its own first frame), the windows to a multiple of 4, and the padding chunks are stored nowhere.  This relies on
    a chunk's posterior depending on that chunk alone -- the encoder runs one sequence per chunk."""
    dev, D, Q = gre.dev, gre.vae_latent_dim, len(examples)
    q_off = np.zeros(Q + 1, dtype=np.int32)
    q_off[1:] = np.cumsum([n_q for _, n_q in examples])
    Wp = -(-Q // 4) * 4
    rows = np.full((len(MOTION_PARTS), Wp * n_lat), -1, dtype=np.int32)
    for i, (_, n_q) in enumerate(examples):
        for p in range(len(MOTION_PARTS)):
            rows[p, i * n_lat:i * n_lat + n_q] = int(q_off[i]) * len(MOTION_PARTS) + p * n_q + np.arange(n_q)
    padded = {}
    for k in MOTION_EXAMPLE_KEYS:
        t = torch.zeros(Wp, n_lat * chunk, int(examples[0][0][k].shape[-1]), device=dev)
        for i, (ex, n_q) in enumerate(examples):
            t[i, :n_q * chunk] = ex[k].to(dev).float()
        padded[k] = t
    total = int(q_off[-1]) * len(MOTION_PARTS)
    mu, logvar = (torch.empty(total, D, device=dev) for _ in range(2))
    gre.encode_posteriors(padded["motion_upper"], padded["motion_lower"], padded["motion_face"], padded["motion_hands"],
                          padded["trans"], padded["facial"], padded["contact"], to_device_async(rows, dev), mu, logvar)
    return mu.view(-1), q_off


def motion_retrieval_batch(mindex, gre, clips, speaker_bonus=0.0):
    """[(motion_queries, speaker_id, text_features)] -> per clip (sample_indexes, d_bounds, query_bounds), the contract of the
    reference's retrieval functions; motion_queries: the clip's list of (start_s, end_s, example[, weights]) (see
    motion_query_fields), possibly empty -- a clip without queries gives three empty dicts.  One example encode, one sweep launch,
    one selection and one rank_survivors (tier cut, text-similarity tie-break against the clip's features) for all queries of
    the batch.  query_bounds[qi] = ("motion", "motion", start_s, end_s), keyed 0.. in ascending start_s (place_exemplars walks
    the query points with a running end); d_bounds[qi][name] = ("motion", "motion", seconds of the best chunk range)."""
    held, examples, weights, speakers, feats = [], [], [], [], []
    for b, (queries, speaker_id, text_features) in enumerate(clips):
        fields = [motion_query_fields(q, mindex.chunk, mindex.L, "clip %d, motion query %d" % (b, i))
                  for i, q in enumerate(queries or [])]
        fields.sort(key=lambda f: f[0])           # (stable: equal starts keep the caller's order)
        held.append(fields)
        for _, _, example, w, n_q in fields:
            examples.append((example, n_q))
            weights.append(w)
            speakers.append(speaker_id)
        if fields:
            feats += [text_features.to(mindex.dev).float().contiguous()] * len(fields)
    if not examples:
        return [({}, {}, {}) for _ in clips]
    qlat, q_off = example_latents(gre, examples, mindex.L, mindex.chunk)
    params = np.array([list(w) + [float(int(s)), float(speaker_bonus)] for w, s in zip(weights, speakers)],
                      dtype=np.float64).reshape(len(examples), 6)
    packed = dict(qlat=qlat, q_off_host=q_off, q_off=to_device_async(q_off, mindex.dev), params_host=params,
                  params=to_device_async(params, mindex.dev), Q=len(examples))
    swept = mindex.sweep(packed)
    ranked = mindex.base.rank_survivors(swept["cursor"], swept["idx"], swept["top"], swept["score"], feats)
    out, pos = [], 0
    for fields in held:
        if not fields:
            out.append(({}, {}, {}))
            continue
        si, db_b = ranked_results(mindex.base.names, ranked[pos:pos + len(fields)], mindex.bounds, n_q=[f[4] for f in fields])
        out.append((si, db_b, {i: ("motion", "motion", f[0], f[1]) for i, f in enumerate(fields)}))
        pos += len(fields)
    return out


def place_exemplars(retr_indexes, retr_bounds, query_bounds, retrieval_method="discourse", fps=15, chunk=15,
                    motion_len=150):
    """Time -> latent-index placement of raggesture.py:542-760.  Returns a list of
    (query_point, sample_name, placed) in visiting order, where placed is None (the exemplar was
    fetched and VAE-encoded by the reference but then skipped) or
    ((retr_lat_start, retr_lat_end), (start_lat, end_lat))."""
    latent_len = motion_len // chunk
    prev_end = -1
    out = []
    for qp, smp_idxs in retr_indexes.items():
        if len(smp_idxs) == 0 or qp not in query_bounds:
            continue
        _, _, q_start, q_end = query_bounds[qp]
        if q_start > q_end:
            continue
        for smp in smp_idxs:
            _, _, r_start, r_end = retr_bounds[qp][smp]
            q_start = max(0, q_start)
            q_end = min(motion_len / fps, q_end)
            q_start, q_end = int(q_start * fps), int(q_end * fps)
            if not q_start // chunk < q_end // chunk + 1:
                raise ValueError("empty query span")
            # the motion method reports the exemplar's chunk range itself (o*, o* + n_q as seconds): it is taken as it
            # stands, without the word margins below
            lat_range = (int(round(r_start * fps)) // chunk, int(round(r_end * fps)) // chunk) if retrieval_method == "motion" else None
            if retrieval_method in ("gesture_type", "llm") and (r_end - r_start) > 0.9:
                r_start, r_end = max(0, r_start - 0.2), min(motion_len / fps, r_end + 0.1)
            else:
                r_start, r_end = max(0, r_start - 0.666), min(motion_len / fps, r_end + 0.333)
            r_start, r_end = int(r_start * fps), int(r_end * fps)
            if r_start == r_end:
                out.append((qp, smp, None))
                continue
            if r_end == motion_len:
                r_end = motion_len - 1
                r_start = max(0, r_start - 1)
            r_lat_start, r_lat_end = r_start // chunk, r_end // chunk + 1
            if lat_range is not None:
                r_lat_start, r_lat_end = lat_range
            mid_lat = ((q_start + q_end) // 2) // chunk
            n = r_lat_end - r_lat_start
            side = n // 2
            if n == 1:
                s, e = mid_lat - side, mid_lat + side + 1
            elif n == 2:
                s, e = mid_lat, mid_lat + side + 1
            elif n % 2 == 1:
                s, e = mid_lat - side - 1, mid_lat + side
            else:
                s, e = mid_lat - side, mid_lat + side
            if s < 0:
                s, e = 0, n
            if e > latent_len:
                s -= e - latent_len
                e = latent_len
            if s < prev_end:
                s = prev_end
                e = s + n
                if e > latent_len:
                    e = latent_len
                    n = e - s
                    if n <= 0:
                        out.append((qp, smp, None))
                        continue
                    r_lat_end = r_lat_start + n
            prev_end = e
            out.append((qp, smp, ((r_lat_start, r_lat_end), (s, e))))
    return out


LMDB_DICTS = ("idx_2_text", "idx_2_sense", "idx_2_discbounds", "idx_2_gesture_labels", "idx_2_prominence", "idx_2_gestprom")


def read_lmdb_dicts(lmdb_paths):
    """The reference's six retrieval caches (raggesture.py:90-155 `LMDBDict`, :219-224: one LMDB environment per dict
    under `lmdb_paths`, ascii keys in cursor order = sample-name order, values `pyarrow.serialize`d, tensors stored as
    numpy arrays and converted back for idx_2_text) -> the metadata dict RetrievalDatabase takes, or None when the
    caches cannot be read here (directory missing / empty, or `lmdb` / the legacy `pyarrow.deserialize` absent --
    pyarrow >= 2 removed that serializer; this image has neither lmdb nor it).  Raises only on a corrupt cache."""
    import os
    try:
        import lmdb
        import pyarrow
    except ImportError:
        return None
    if not hasattr(pyarrow, "deserialize") or lmdb_paths is None or not os.path.isdir(str(lmdb_paths)):
        return None
    out = {}
    for name in LMDB_DICTS:
        path = os.path.join(str(lmdb_paths), name)
        if not os.path.isdir(path):
            if name in ("idx_2_text", "idx_2_sense", "idx_2_discbounds", "idx_2_prominence"):
                return None
            continue
        env = lmdb.open(path, readonly=True, lock=False)
        d = {}
        with env.begin(write=False) as txn:
            for key, val in txn.cursor():
                v = pyarrow.deserialize(val)
                if name == "idx_2_text":   # torch_converter=True (:219)
                    v = torch.from_numpy(v) if isinstance(v, np.ndarray) else \
                        [torch.from_numpy(x) if isinstance(x, np.ndarray) else x for x in v] if isinstance(v, list) else v
                d[key.decode("ascii")] = v
        env.close()
        if name in ("idx_2_text", "idx_2_sense") and not d:
            return None      # fresh checkout: the reference rebuilds the caches from the dataset (:226-243)
        out[name] = d
    return out


class RetrievalDatabase:
    """Drop-in for raggesture.py:157-884 `RetrievalDatabase` (inference; the reference's `discourse`, `gesture_type` and
    `llm` methods, and `prosody`, which the reference names and refuses: exemplars by word prominence, this project's own
    scoring -- see ProsodyIndex; it needs conditions["prominence"] only, and query and DB annotated by the same estimator;
    and `motion`, which the reference does not know: exemplars by a motion example, conditions["motion_queries"][b] = a list of
    (start_s, end_s, example[, weights]) -- see motion_query_fields and MotionIndex; quality on real motion is not claimed).

    `dataset[name]` must return the per-sample dict the reference reads (motion, motion_upper/lower/
    face/hands, facial, trans, contact, motion_mask, word, audio, speaker_id).  DB metadata comes
    from `metadata` (dict of idx_2_text / idx_2_sense / idx_2_discbounds / idx_2_prominence; idx_2_wordprom for the
    prosody method) or from `dataset.retrieval_samples` (raw records, see build_db_dicts)."""
    CACHE_CAP = 4096   # clips kept in the write-only test_indexes / test_dbounds / test_qbounds dicts
    # keys of the reference's constructor (raggesture.py:159-184) that only size its TRAINING-time retrieval encoders
    # (never built or used at inference): accepted and ignored, anything else is an error
    REFERENCE_TRAINING_KEYS = frozenset(("motion_feat_dim", "output_dim", "num_layers", "num_motion_layers", "kinematic_coef",
                                         "num_heads", "ff_size", "stride", "sa_block_cfg", "ffn_cfg", "dropout"))

    def __init__(self, num_retrieval=None, topk=None, latent_dim=512, text_latent_dim=768, max_seq_len=150,
                 motion_fps=15, motion_framechunksize=15, dataset=None, metadata=None, device="cuda", word_similarity=None,
                 llm_output=None, stratified_db_creation=False, stratification_interval=15, lmdb_paths=None,
                 new_lmdb_cache=False, prosody_max_queries=3, prosody_min_gap=1.0, prosody_min_prominence=None,
                 motion_index_bytes=4 << 30, motion_speaker_bonus=0.0, **_cfg):
        """DB metadata, in this order: `metadata=` (the six dicts), the reference's LMDB caches under `lmdb_paths`
        (when readable here and new_lmdb_cache is off, raggesture.py:219-243), `dataset.retrieval_samples` (raw
        records -> build_db_dicts, what the reference does when its caches are empty).
        prosody_max_queries / prosody_min_gap / prosody_min_prominence: the query-word selection of the prosody method
        (prosody_queries); constructor arguments, not configuration keys the reference would not know.
        motion_index_bytes / motion_speaker_bonus: the motion method -- the byte budget of the table of motion latents (MotionIndex;
        a database that does not fit is refused, nothing is evicted) and what an entry of the query clip's speaker gains."""
        unknown = sorted(set(_cfg) - self.REFERENCE_TRAINING_KEYS)
        if unknown:
            raise capi.RgError("RetrievalDatabase: unknown configuration key(s) %s" % ", ".join(unknown))
        if metadata is None and not new_lmdb_cache:
            metadata = read_lmdb_dicts(lmdb_paths)
        if metadata is None:
            samples = getattr(dataset, "retrieval_samples", None)
            if samples is None:
                raise capi.RgError("RetrievalDatabase needs `metadata=`, readable LMDB caches under lmdb_paths=%r (lmdb and "
                                   "the legacy pyarrow.deserialize must be importable) or `dataset.retrieval_samples`"
                                   % (lmdb_paths,))
            metadata = build_db_dicts(samples, stratified_db_creation, stratification_interval)
        self.dataset = dataset
        self.num_retrieval, self.topk = num_retrieval or 1, topk
        self.max_seq_len, self.motion_fps, self.motion_framechunksize = max_seq_len, motion_fps, motion_framechunksize
        self.latent_dim, self.text_latent_dim = latent_dim, text_latent_dim
        self.index = DiscourseIndex(metadata, device)
        # gesture_type / llm methods: need idx_2_gesture_labels in the metadata.  word_similarity(db_word, query_word):
        # None = the reference's effective behaviour, fuzz.partial_ratio / 100 (rag/utils.py:239-272; device form
        # rg_partial_ratio); a callable = the embedding-model similarity the reference's comments intend
        self.gesture_index = GestureTypeIndex(metadata, self.index) if "idx_2_gesture_labels" in metadata else None
        self.word_similarity = fuzzy_word_similarity if word_similarity is None else word_similarity
        # prosody method: needs idx_2_wordprom (build_db_dicts writes it; the reference's six LMDB dicts do not hold it)
        self.prosody_index = ProsodyIndex(metadata, self.index) if "idx_2_wordprom" in metadata else None
        self.prosody_kwargs = dict(max_queries=prosody_max_queries, min_gap=prosody_min_gap,
                                   min_prominence=prosody_min_prominence, motion_seconds=max_seq_len / motion_fps)
        # motion method: the table of the entries' motion latents needs the VAE: build_motion_index, or the first motion search
        self.motion_index, self.motion_index_bytes, self.motion_speaker_bonus = None, int(motion_index_bytes), float(motion_speaker_bonus)
        self._motion_gre = None
        # llm method: `llm_output(text) -> str` stands for get_llm_output (rag/llm_retrieval.py:69-96, the GPT call);
        # an LLMResponseCache (cached answers, BASELINE config 5) or any callable
        self.llm_output = llm_output.get if isinstance(llm_output, LLMResponseCache) else llm_output
        self.test_indexes, self.test_dbounds, self.test_qbounds = {}, {}, {}
        self.phase_ms = None  # dict: MotionDiffusion's phase profiler also collects the sub-phases here

    def retrieve(self, retr_method, text_features, discourse, prominence, speaker_id, idx=None, ready=None,
                 gesture_labels=None, text=None, text_times=None, motion_queries=None, gesture_rep_encoder=None):
        """raggesture.py:313-477, eval branch: the reference reads its per-idx cache only under `self.training` (:335);
        in eval every call recomputes and overwrites test_indexes[idx] -- so do we (the dicts are written for parity
        of that side effect only, bounded to the last CACHE_CAP clips)."""
        if retr_method not in ("discourse", "gesture_type", "llm", "prosody", "motion"):
            raise NotImplementedError("retrieval method %r (the methods are discourse, gesture_type, llm, prosody and motion; "
                                      "the last two are this project's own: the reference raises for prosody, "
                                      "raggesture.py:431, and does not know motion)" % retr_method)
        if True:
            if ready is not None:
                si, db_b, qb = ready
            elif retr_method == "prosody":
                si, db_b, qb = self.prosody_batch([(prominence, speaker_id, text_features)])[0]
            elif retr_method == "motion":
                si, db_b, qb = self.motion_batch([(motion_queries, speaker_id, text_features)], gesture_rep_encoder)[0]
            elif retr_method in ("gesture_type", "llm"):
                if self.gesture_index is None:
                    raise capi.RgError("%s retrieval needs idx_2_gesture_labels in the DB metadata (raggesture.py:262)" % retr_method)
                if retr_method == "gesture_type":
                    si, db_b, qb = gesture_type_retrieval(self.gesture_index, gesture_labels, speaker_id, text_features,
                                                          self.word_similarity)
                else:
                    if self.llm_output is None:
                        raise capi.RgError("llm retrieval needs `llm_output=` (an LLMResponseCache or a callable text -> answer)")
                    si, db_b, qb = llm_retrieval(self.gesture_index, text, text_times, speaker_id, prominence, text_features,
                                                 self.word_similarity, self.llm_output)
            else:
                si, db_b, qb = discourse_retrieval(self.index, discourse, prominence, speaker_id, text_features)
            self.test_indexes.setdefault(idx, {})[retr_method] = si
            self.test_dbounds.setdefault(idx, {})[retr_method] = db_b
            self.test_qbounds.setdefault(idx, {})[retr_method] = qb
            while len(self.test_indexes) > self.CACHE_CAP:
                old = next(iter(self.test_indexes))
                for d in (self.test_indexes, self.test_dbounds, self.test_qbounds):
                    d.pop(old, None)
        data = {q: [s for s in idxs if s != idx][:self.num_retrieval] for q, idxs in si.items()}
        return data, db_b, qb

    def prosody_batch(self, clips):
        """prosody_retrieval_batch over this database with its constructor's selection settings."""
        if getattr(self, "prosody_index", None) is None:
            raise capi.RgError("prosody retrieval needs idx_2_wordprom in the DB metadata (build_db_dicts writes it from the "
                               "records' prominence lists; the reference's six LMDB dicts do not hold it)")
        return prosody_retrieval_batch(self.prosody_index, clips, **self.prosody_kwargs)

    def build_motion_index(self, gesture_rep_encoder, batch=64):
        """The table of the entries' motion latents (MotionIndex.build over `dataset`), `batch` entries per encode; kept until
        discard_motion_index (new VAE weights).  Returns it."""
        if self.dataset is None:
            raise capi.RgError("motion retrieval needs `dataset=` (the entries' motion records are VAE-encoded into the index)")
        if gesture_rep_encoder is None:
            raise capi.RgError("motion retrieval needs the model's gesture_rep_encoder (its VAE encoders produce the latents)")
        self.motion_index = MotionIndex.build(self.index, gesture_rep_encoder, lambda name: self.dataset[name],
                                              self.max_seq_len // self.motion_framechunksize, self.motion_framechunksize,
                                              self.motion_fps, getattr(self, "motion_index_bytes", 4 << 30), batch)
        self._motion_gre = gesture_rep_encoder
        return self.motion_index

    def discard_motion_index(self):
        self.motion_index = self._motion_gre = None

    def _motion_ready(self, gesture_rep_encoder):
        """(index, encoder) of the motion method; the index is built on first use."""
        gre = gesture_rep_encoder if gesture_rep_encoder is not None else getattr(self, "_motion_gre", None)
        if getattr(self, "motion_index", None) is None or (gre is not None and gre is not self._motion_gre):
            self.build_motion_index(gre)
        return self.motion_index, self._motion_gre

    def motion_batch(self, clips, gesture_rep_encoder=None):
        """motion_retrieval_batch over this database: clips [(motion_queries, speaker_id, text_features)]."""
        if not any(queries for queries, _, _ in clips):
            return [({}, {}, {}) for _ in clips]
        mindex, gre = self._motion_ready(gesture_rep_encoder)
        return motion_retrieval_batch(mindex, gre, clips, getattr(self, "motion_speaker_bonus", 0.0))

    def nearest_motions(self, example, k=10, weights=None, speaker_id=None, gesture_rep_encoder=None):
        """The k database window positions nearest to `example` (a dict of MOTION_EXAMPLE_KEYS, see motion_query_fields), for
        inspecting and de-duplicating a database: [(name, offset_chunk, d_norm)] in ascending d_norm (then entry order), d_norm
        = d(o*) / (n_q D sum_p w_p), 0 for a bit-equal copy.  speaker_id: only that speaker's entries.  One launch, read back
        once; no speaker bonus, no text tie-break."""
        mindex, gre = self._motion_ready(gesture_rep_encoder)
        _, _, example, w, n_q = motion_query_fields((0.0, 0.0, example, weights), mindex.chunk, mindex.L, "nearest_motions")
        qlat, q_off = example_latents(gre, [(example, n_q)], mindex.L, mindex.chunk)
        score, top = mindex.scores([(qlat.view(len(MOTION_PARTS), n_q, mindex.D), w, -1, 0.0)])
        both = torch.stack([score[0], top[0].to(torch.float64), mindex.spk.to(torch.float64)]).cpu().numpy()
        d_norm = 1.0 / both[0] - 1.0
        keep = np.arange(mindex.n) if speaker_id is None else np.flatnonzero(both[2] == int(speaker_id))
        order = keep[np.argsort(d_norm[keep], kind="stable")][:int(k)]
        return [(mindex.base.names[e], int(both[1][e]), float(d_norm[e])) for e in order]

    def __call__(self, *a, **k):
        return self.forward(*a, **k)

    @staticmethod
    def _clip_text(conditions, b):
        """The transcript the llm method prompts with.  The reference hands llm_retrieval conditions["text"]
        (raggesture.py:501), which MotionDiffusion fills with the frame-aligned word EMBEDDINGS
        (diffusion_architecture.py:190) -- `text.strip()` cannot run on those; the transcript string is what
        the same dict carries as "raw_text" (:191), so a non-string "text" falls back to it."""
        for key in ("text", "raw_text"):
            v = conditions.get(key)
            if v is not None and not torch.is_tensor(v) and len(v) > b and isinstance(v[b], str):
                return v[b]
        return None

    def _db_entries(self):
        """Entries of the database (what an exemplar posterior cache would hold at most), None if the dataset cannot say."""
        try:
            return max(len(self.dataset), self.index.n)
        except TypeError:
            return self.index.n

    def _tick(self, name):
        """Sub-phase wall times (with device syncs) when a profiler dict is attached; else a no-op."""
        if self.phase_ms is None:
            return
        import time
        torch.cuda.synchronize()
        now = time.perf_counter()
        if name is not None:
            self.phase_ms[name] = self.phase_ms.get(name, 0.0) + (now - self._t_last) * 1e3
        self._t_last = now

    def encode_exemplars(self, gre, names, recs, noise, dev):
        """VAE latents of the visited exemplars (names / their records, in visiting order): draws their noise in the
        reference's order, then encodes them in one batch.  Returns (latent fp32 [E, 4 L + 3, D], fork): `fork` is an event
        recorded on the current stream BEFORE the encode was queued (what on_exemplars orders its work after)."""
        L, D, E = self.max_seq_len // self.motion_framechunksize, self.latent_dim, len(names)
        stack = lambda k: torch.stack([r[k] for r in recs]).to(dev).float().contiguous()
        if noise is not None and not getattr(noise, "order_free", False):
            # explicit noise: the reference draws 4 x [L,1,D] per exemplar, exemplar-major (rsample order)
            eps = [[noise.draw((L, 1, D)) for _ in range(4)] for _ in range(E)]
            eps_list = [torch.cat([e[p].to(dev) for e in eps], dim=0) for p in range(4)]
        else:
            draw = noise.draw if noise is not None else (lambda shape: torch.randn(*shape, device=dev))
            eps_list = [draw((E * L, 1, D)) for _ in range(4)]  # generator noise: order is immaterial
        fork = torch.cuda.Event()     # work started by on_exemplars orders itself after this point, not after the encode
        fork.record()
        # The exemplar posterior cache, where the model has one (vae.ExemplarPosteriorCache): only exemplars it has not seen
        # are encoded -- the posterior is a function of the record and the VAE weights -- and one launch reparameterises all
        # of them with this call's noise.  Same bits as the batch encode below.
        cache = getattr(gre, "exemplar_cache", None)
        lat = cache.latents(names, recs, eps_list, L, entries=self._db_entries()) if cache is not None else None
        if lat is None:
            # batch of Ep = E rounded up to a multiple of 4 (padding = copies of exemplar 0 with zero noise, dropped below):
            # the captured encode graphs exist per Ep, not per exemplar count
            Ep = -(-E // 4) * 4
            padr = lambda t: t if t.shape[0] == Ep else torch.cat([t, t[:1].expand(Ep - E, *t.shape[1:])], dim=0).contiguous()
            eps_list = [torch.cat([e, e.new_zeros((Ep - E) * L, 1, D)], dim=0) if Ep != E else e for e in eps_list]
            lat, _ = gre.encode(padr(stack("motion_upper")), padr(stack("motion_lower")), padr(stack("motion_face")),
                                padr(stack("motion_hands")), padr(stack("trans")), padr(stack("facial")), padr(stack("contact")),
                                padr(stack("motion_mask")), eps_list)
            lat = lat[:E]
        return lat, fork

    def forward(self, conditions, lengths, device, idx=None, retrieval_method="gesture_type", gesture_rep_encoder=None,
                noise=None, on_exemplars=None, search_stream=None, inputs_ready=None):
        """conditions: the model's kwargs dict (text_features, discourse, prominence, speaker_ids, ...)."""
        gre = gesture_rep_encoder
        dev = torch.device(device)
        B = len(conditions["text_features"])
        chunk, L = self.motion_framechunksize, self.max_seq_len // self.motion_framechunksize
        T, D = 4 * L + 3, self.latent_dim
        tick = self._tick
        tick(None)
        # The DB sweeps, their read-back and the host-side ranking walk only need the query annotations: on a
        # stream of their own (search_stream, waiting for `inputs_ready` only) they do not queue behind the
        # caller's pending work on the current stream (the batch VAE encode), and the walk overlaps with it.
        import contextlib
        ctx = torch.cuda.stream(search_stream) if search_stream is not None else contextlib.nullcontext()
        if search_stream is not None and inputs_ready is not None:
            search_stream.wait_event(inputs_ready)
        with ctx:
            plans, ex = [], []
            spks = [int(v) for v in conditions["speaker_ids"][:, 0].tolist()]
            ready = {}
            if retrieval_method == "discourse":
                # one native call per batch: two host synchronisations, one launch for all tie tiers
                ready = dict(enumerate(discourse_retrieval_batch(self.index, [
                    (conditions["discourse"][b], conditions["prominence"][b], spks[b], conditions["text_features"][b])
                    for b in range(B)])))
            elif retrieval_method == "prosody":
                # all clips' query words in one sweep launch; needs the prominence lists only
                ready = dict(enumerate(self.prosody_batch([
                    (conditions["prominence"][b], spks[b], conditions["text_features"][b]) for b in range(B)])))
            elif retrieval_method == "motion":
                # all clips' examples in one encode and one sweep launch; a clip without queries gets no exemplar
                mq = conditions.get("motion_queries") or [[] for _ in range(B)]
                ready = dict(enumerate(self.motion_batch([(mq[b], spks[b], conditions["text_features"][b]) for b in range(B)], gre)))
            for b in range(B):
                spk = spks[b]
                ri, rb, qb = self.retrieve(retrieval_method, conditions["text_features"][b],
                                           (conditions.get("discourse") or [None] * B)[b],
                                           (conditions.get("prominence") or [None] * B)[b], spk, idx=idx[b] if idx is not None else None,
                                           ready=ready.get(b),
                                           gesture_labels=(conditions.get("gesture_labels") or [None] * B)[b],
                                           text=self._clip_text(conditions, b),
                                           text_times=(conditions.get("text_times") or [None] * B)[b])
                plan = place_exemplars(ri, rb, qb, retrieval_method, self.motion_fps, chunk, self.max_seq_len)
                plans.append((plan, rb, qb))
                for qp, name, placed in plan:
                    ex.append((b, qp, name, placed))
        tick("retrieval.search")
        self.last_exemplars = [(b, qp, name, placed is not None) for b, qp, name, placed in ex]   # visiting order (tests)
        # ---- fetch + VAE-encode every visited exemplar in one batch (noise in the reference's order)
        recs = [self.dataset[name] for _, _, name, _ in ex]
        lat, fork = self.encode_exemplars(gre, [name for _, _, name, _ in ex], recs, noise, dev) if ex else (None, None)
        E = len(ex)
        if on_exemplars is not None and ex:
            # the caller may start work that needs the exemplars' conditioning only (their K/V projections) on other
            # streams while this stream VAE-encodes their motion; the encode (one graph launch) is queued first so
            # that the device is not left waiting for the host to issue the projections' launches
            on_exemplars(ex, recs, fork)
        tick("retrieval.exemplar_encode")
        retr_se, query_se, retr_lats, names_out, type2words = ([{} for _ in range(B)] for _ in range(5))
        zero_motion = torch.zeros(B, T, D, device=dev)
        if self.dataset is None:
            raise capi.RgError("RetrievalDatabase.forward needs `dataset=` (the exemplars' motion / audio / text records); "
                               "metadata alone only supports retrieve()")
        tmpl = self.dataset[0]
        raw_motion = torch.zeros(B, self.max_seq_len, tmpl["motion"].shape[-1], device=dev)
        raw_trans = torch.zeros(B, self.max_seq_len, tmpl["trans"].shape[-1], device=dev)
        raw_facial = torch.zeros(B, self.max_seq_len, tmpl["facial"].shape[-1], device=dev)
        # all row copies of the exemplar canvases are gathered into index lists and issued as one gather/scatter
        # per tensor (a guided batch has ~50 exemplars x 7 small copies otherwise); later spans overwrite earlier
        # ones exactly as the reference's sequential slice assignments do (index_copy_ with unique keys)
        lat_dst, lat_src, frame_dst, frame_src = [], [], [], []
        lmask = gre.latent_mask(torch.stack([r["motion_mask"] for r in recs])) if ex else None
        for e, (b, qp, name, placed) in enumerate(ex):
            if placed is None:
                continue
            (r0, r1), (s0, s1) = placed
            rec, (plan, rb, qb) = recs[e], plans[b]
            retr_se[b][qp], query_se[b][qp] = (r0, r1), (s0, s1)
            retr_lats[b][qp] = dict(retr_motion_latent=lat[e:e + 1], retr_text=rec["word"].unsqueeze(0).to(dev),
                                    retr_audio=rec["audio"].unsqueeze(0).to(dev),
                                    retr_spkid=rec["speaker_id"].unsqueeze(0).to(dev),
                                    retr_motion_mask=lmask[e:e + 1])
            span = np.arange(s1 - s0)
            for part in range(4):
                o = part * (L + 1)
                lat_dst.append(b * T + o + s0 + span)
                lat_src.append(e * T + o + r0 + span)
            frames = np.arange((s1 - s0) * chunk)
            frame_dst.append(b * self.max_seq_len + s0 * chunk + frames)
            frame_src.append(e * self.max_seq_len + r0 * chunk + frames)
            q_word, q_type = qb[qp][0], qb[qp][1]
            r_word, r_type = rb[qp][name][0], rb[qp][name][1]
            type2words[b][qp] = (q_word, q_type, r_word, r_type)
            names_out[b][q_word] = name
        if lat_dst:
            def idx(dst, src):
                # a row written twice keeps its LAST source (sequential slice assignment); index_copy_ needs unique keys
                dst, src = np.concatenate(dst), np.concatenate(src)
                _, last = np.unique(dst[::-1], return_index=True)
                keep = len(dst) - 1 - last
                return to_device_async(dst[keep], dev), to_device_async(src[keep], dev)
            dst, src = idx(lat_dst, lat_src)
            zero_motion.view(B * T, D).index_copy_(0, dst, lat.reshape(E * T, D).index_select(0, src))
            dst, src = idx(frame_dst, frame_src)
            for canvas, key in ((raw_motion, "motion"), (raw_trans, "trans"), (raw_facial, "facial")):
                allrec = torch.stack([r[key] for r in recs]).to(dev).float()
                canvas.view(B * self.max_seq_len, -1).index_copy_(0, dst, allrec.view(E * self.max_seq_len, -1).index_select(0, src))
        src_mask = (zero_motion != 0).any(dim=-1).to(torch.int)
        raw_latent_mask = src_mask.clone()
        raw_motion_latents = zero_motion.clone()
        # (face and lower-body rows; as two slices: a LIST index is uploaded from pageable memory, and that copy returns
        # only after everything queued on this stream -- the exemplar encode -- has run)
        for r0, r1 in ((2 * L + 2, 3 * L + 2), (3 * L + 3, T)):
            src_mask[:, r0:r1] = 0
            raw_motion_latents[:, r0:r1, :] = 0
        tick("retrieval.assemble")
        return dict(re_text=None, re_motion=None, re_mask=src_mask,
                    raw_motion_latents=raw_motion_latents.view(B, self.num_retrieval, T, D),
                    raw_motion=raw_motion.view(B, self.num_retrieval, self.max_seq_len, -1),
                    raw_trans=raw_trans.view(B, self.num_retrieval, self.max_seq_len, -1),
                    raw_facial=raw_facial.view(B, self.num_retrieval, self.max_seq_len, -1),
                    raw_sample_names=names_out, raw_type2words=type2words, raw_latent_mask=raw_latent_mask,
                    retr_startends=retr_se, query_startends=query_se, retr_uncropped_latents=retr_lats)


# ---------------------------------------------------------------------------------------------- LLM guidance (host side)
_LLM_LABEL_RX = re.compile(r"[\"\']*([\w \-\']+\w)[\"\']*\,\s*[\"\']*(?P<gesttype>b*eat|m*etaphoric|iconic|deictic)", re.MULTILINE)


def parse_gesture_labels_from_llm_output(llm_output):
    """rag/llm_retrieval.py:131-165: the "(word, type)" pairs of an LLM answer -> [{"word", "name"}], beat labels and
    duplicates (pairs repeated in the model's explanation) dropped.  Same regular expression as the reference."""
    labels = []
    for m in _LLM_LABEL_RX.finditer(llm_output):
        t = m.group("gesttype")
        if "etaphoric" in t:
            name = "metaphoric"
        elif "eat" in t:
            name = "beat"
        elif "iconic" in t:
            name = "iconic"
        else:
            name = "deictic"
        labels.append({"word": m.group(1).strip(), "name": name})
    out = []
    for g in labels:
        if g["name"] != "beat" and g not in out:
            out.append(g)
    return out


class LLMResponseCache:
    """Response cache for the LLM call of the llm retrieval method (rag/llm_retrieval.py:72-96 calls the API for
    every window of every clip; BASELINE config 5 runs on cached calls).  `call(text) -> str` is supplied by the
    user (there is no network code here); answers are keyed by the exact prompt text and persisted as JSON."""

    def __init__(self, path=None, call=None):
        self.path, self.call, self.hits, self.misses = path, call, 0, 0
        self.data = {}
        if path is not None and os.path.exists(path):
            with open(path, "r", encoding="utf-8") as f:
                self.data = json.load(f)

    def get(self, text):
        if text in self.data:
            self.hits += 1
            return self.data[text]
        if self.call is None:
            raise KeyError("no cached LLM answer for this text and no `call` to produce one")
        self.misses += 1
        self.data[text] = self.call(text)
        if self.path is not None:
            with open(self.path, "w", encoding="utf-8") as f:
                json.dump(self.data, f, ensure_ascii=False, indent=0)
        return self.data[text]

    def labels(self, text):
        """parse(get(text)); the empty text short-circuits like llm_retrieval (:180-181)."""
        return [] if text.strip() == "" else parse_gesture_labels_from_llm_output(self.get(text))
