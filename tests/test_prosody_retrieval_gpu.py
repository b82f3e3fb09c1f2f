"""The `prosody` retrieval method on the device: the sweep kernel against the float64 restatement (bits), the batched search
against it (names, bounds), and the method through the model.  No tolerance anywhere: scores are compared as bits, indices
and names exactly."""
import numpy as np
import pytest
import torch

import prosody_retrieval_ref as ref

pytestmark = pytest.mark.gpu
GI = [0] * 25 + list(range(25))


# ------------------------------------------------------------------------------------------------ the kernel, hand-built DB
N = 301
WIDE = range(100, 164)     # 64 entries of 80 words: whatever the tile origin, one whole tile holds more words than are staged


def _hand_db(rg):
    """-> (entries [(word, start, end, prominence)] per entry, speakers, vocabulary words)."""
    pr_max = int(rg.capi.load_library().rg_partial_ratio_max_len())
    g = np.random.Generator(np.random.PCG64(301))
    vocab = ["alpha", "beta", "gamma", "round", "around", "big", "bigger", "that one", "over there", "a"] + \
            ["word%02d" % k for k in range(49)] + ["x" * (pr_max + 3)]
    assert len(vocab) == 60

    def rows(k):
        out, t = [], 0.0
        for _ in range(k):
            s = t + float(g.integers(0, 4)) * 0.05
            e = s + float(g.integers(1, 9)) * 0.05
            t = e
            out.append((vocab[int(g.integers(0, len(vocab)))], s, e, None if g.uniform() < 0.15 else float(g.integers(0, 13)) * 0.25))
        return out

    entries = [rows(int(g.integers(0, 13))) for _ in range(N)]
    entries[0], entries[N - 1] = [], []                                     # no words, first and last
    entries[1] = [("alpha", 0.0, 0.5, None), ("beta", 0.5, 1.0, float("nan")), ("big", 1.0, 1.5, None)]   # nothing known
    entries[2] = [("gamma", 2.0, 2.25, 1.75)]                               # one word
    entries[3] = rows(257)                                                  # more than a wave's and a workgroup's worth
    entries[3][200] = ("alpha", 50.0, 50.5, 1.0)                            # its best word for query 0 sits deep in the row ...
    entries[3][40] = ("alpha", 10.0, 10.5, 1.0)                             # ... twice, bit-equal: the lower index is reported
    entries[4] = [("beta", 0.0, 0.5, 2.0), ("alpha", 1.0, 1.5, 1.0), ("big", 2.0, 2.25, 0.5), ("alpha", 3.0, 3.5, 1.0)]  # a bit-equal pair
    for e in (5, 6, 7, 31, 32, 33):                                         # the same words in neighbouring entries (and tiles)
        entries[e] = [("round", 1.0, 1.5, 1.75), ("that one", 2.0, 2.75, 0.5)]
    for e in WIDE:
        entries[e] = rows(80)
    speakers = [int(g.integers(0, 3)) for _ in range(N)]
    speakers[5], speakers[6], speakers[7] = 2, 2, 1
    return entries, speakers, vocab


QUERIES = [("alpha", 1.0, 0.5, 1),                # a vocabulary word; p_q and dur_q equal DB values (both differences 0)
           ("zebra", 0.37, 0.3, 0),               # not in the vocabulary
           ("word07", 2.2, 0.21, 9),              # a speaker no entry has
           ("round", 1.75, 0.05, 2),              # p_q equal to a DB prominence, a very short query word
           (None, 0.5, 0.05, 0)]                  # (filled in: the word longer than the device similarity handles)


@pytest.fixture(scope="module")
def hand(rg):
    assert torch.cuda.is_available()
    entries, speakers, vocab = _hand_db(rg)
    names = ["e%03d" % e for e in range(N)]
    db = dict(idx_2_sense={n: [speakers[e]] for e, n in enumerate(names)},
              idx_2_prominence={n: {} for n in names},
              idx_2_text={n: (torch.zeros(1, 8), speakers[e]) for e, n in enumerate(names)},
              idx_2_wordprom={n: entries[e] for e, n in enumerate(names)})
    pindex = rg.retrieval.ProsodyIndex(db, rg.retrieval.DiscourseIndex(db, "cuda"))
    table = ref.Table(entries, speakers)
    queries = [(q[0] or vocab[-1],) + q[1:] for q in QUERIES]
    want = [ref.scores(table, table.sim_row(w), p, d, s) for w, p, d, s in queries]      # computed once, shared, not modified
    return dict(pindex=pindex, table=table, queries=queries, want=want, entries=entries)


def _bits(score):
    return score.cpu().numpy().view(np.int64)


def test_index_layout(rg, hand):
    p, t = hand["pindex"], hand["table"]
    assert p.n == N and p.vocab == t.vocab and 55 <= len(p.vocab) <= 60
    assert any(len(w) > p.fuzzy.pr_max for w in p.vocab)
    assert p.word_off.dtype == torch.int32 and np.array_equal(p.word_off.cpu().numpy(), t.word_off)
    assert p.word_code.dtype == torch.int32 and np.array_equal(p.word_code.cpu().numpy(), t.word_code)
    assert p.word_dur.dtype == torch.float64 and p.word_dur.cpu().numpy().tobytes() == t.word_dur.tobytes()
    assert p.word_prom.dtype == torch.float64 and np.array_equal(p.word_prom.cpu().numpy(), t.word_prom, equal_nan=True)
    assert np.array_equal(p.spk.cpu().numpy(), t.spk)
    counts = np.diff(t.word_off)
    assert counts[0] == counts[-1] == 0 and counts[2] == 1 and counts[3] == 257 and counts[list(WIDE)].sum() == 64 * 80


@pytest.mark.parametrize("which", [[0], [1], [2], [3], [4], [0, 1, 2, 3, 4]], ids=lambda w: "Q%d_%s" % (len(w), "".join(map(str, w))))
def test_sweep_equals_restatement_bitwise(rg, hand, which):
    queries = [hand["queries"][i] for i in which]
    score, top = hand["pindex"].scores(queries)
    torch.cuda.synchronize()
    assert score.shape == top.shape == (len(which), N) and score.dtype == torch.float64 and top.dtype == torch.int32
    got_s, got_t = _bits(score), top.cpu().numpy()
    for row, i in enumerate(which):
        want_s, want_t = hand["want"][i]
        bad = np.flatnonzero((got_s[row] != want_s.view(np.int64)) | (got_t[row] != want_t))
        assert bad.size == 0, "query %d: %d entries differ, first %d: got (%r, %d) want (%r, %d)" % (
            i, bad.size, bad[0], score[row, bad[0]].item(), got_t[row, bad[0]], want_s[bad[0]], want_t[bad[0]])


def test_sweep_edge_entries(rg, hand):
    """What the hand-built entries are there for, read off the device result (the restatement agrees: test above)."""
    score, top = hand["pindex"].scores(hand["queries"])
    s, t = score.cpu().numpy(), top.cpu().numpy()
    for q in range(5):
        assert s[q, 0] == s[q, N - 1] == s[q, 1] == 0.0 and t[q, 0] == t[q, N - 1] == t[q, 1] == -1
        assert t[q, 2] == 0 and s[q, 2] > 0
    # query 0: "alpha", prominence 1.0, duration 0.5 -> an identical DB word scores 4 + 2 + 1 exactly (+ 3 for speaker 1)
    assert t[0, 4] == 1 and t[0, 3] == 40
    spk = hand["table"].spk
    assert s[0, 4] == 7.0 + (3.0 if spk[4] == 1 else 0.0) and s[0, 3] == 7.0 + (3.0 if spk[3] == 1 else 0.0)
    # equal words in neighbouring entries: equal scores up to the speaker bonus (query 3 is speaker 2: entries 5, 6 have it)
    assert s[3, 5] == s[3, 6] == s[3, 7] + 3.0 == s[3, 31] + (3.0 if spk[31] != 2 else 0.0) and t[3, 5] == t[3, 31] == 0
    # a speaker nobody has: no entry carries the bonus, every score stays below the term maxima 4 + 2 + 1
    assert s[2].max() <= 7.0
    # the entries beyond the staged words are scored like any other
    assert all((t[q, list(WIDE)] >= 0).all() and (t[q, list(WIDE)] < 80).all() for q in range(5))


def test_sweep_is_repeatable(rg, hand):
    a = hand["pindex"].scores(hand["queries"])
    b = hand["pindex"].scores(hand["queries"])
    torch.cuda.synchronize()
    assert a[0].data_ptr() != b[0].data_ptr()
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[1], b[1])


def test_sweep_argument_checks(rg, hand):
    p = hand["pindex"]
    sim = torch.zeros(1, len(p.vocab), dtype=torch.float64, device="cuda")
    par = torch.zeros(1, 3, dtype=torch.float64, device="cuda")
    sc, tp = torch.empty(1, N, dtype=torch.float64, device="cuda"), torch.empty(1, N, dtype=torch.int32, device="cuda")

    def call(off_host, n_words=p.n_words, V=len(p.vocab), Q=1):
        p.h.call("prosody_scores_batched", p.spk, p.word_off, off_host.ctypes.data, p.word_code, p.word_prom, p.word_dur, N,
                 n_words, sim, V, par, Q, sc, tp)

    good = p.word_off_host
    call(good)
    for bad in (good + 1, np.concatenate([good[:5], good[3:4], good[6:]])):
        with pytest.raises(rg.capi.RgError, match="offsets"):
            call(np.ascontiguousarray(bad, dtype=np.int32))
    with pytest.raises(rg.capi.RgError, match="n_words"):
        call(good, n_words=p.n_words - 1)
    for kw in (dict(V=0), dict(Q=0)):
        with pytest.raises(rg.capi.RgError, match="shape"):
            call(good, **kw)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- the search
SEEDS = (3, 4, 6)


def _search_samples(rg):
    """synth_retrieval_samples(300) with three entries rewritten into exact copies of clip 0's strongest word: a top tier of
    three bit-equal scores, which only the text similarity orders."""
    smp = rg.synth.synth_retrieval_samples(300, tie_groups=True)
    q = rg.synth.synth_llm_query(SEEDS[0])
    qb, proms = ref.prosody_queries(q["prominence"])
    k = int(np.argmax(proms))
    word, _, s, e = qb[k]
    for i in (20, 120, 220):
        smp[i] = dict(smp[i], speaker_id=q["speaker_id"], discourse=[], gesture_labels=[],
                      prominence=[("uh", 0.5, 0.7, 0.1), (word, 2.0, 2.0 + (e - s), proms[k])])
    return smp, k


@pytest.fixture(scope="module")
def searched(rg):
    smp, k = _search_samples(rg)
    db = rg.retrieval.build_db_dicts(smp)
    pindex = rg.retrieval.ProsodyIndex(db, rg.retrieval.DiscourseIndex(db, "cuda"))
    clips = [rg.synth.synth_llm_query(seed) for seed in SEEDS]
    return dict(smp=smp, pindex=pindex, clips=clips, tie_query=k)


def test_search_equals_restatement(rg, searched):
    clips = searched["clips"]
    got = rg.retrieval.prosody_retrieval_batch(searched["pindex"], [(c["prominence"], c["speaker_id"], c["text_features"])
                                                                     for c in clips])
    assert len(got) == len(clips)
    for b, c in enumerate(clips):
        want = ref.retrieve(searched["smp"], c["prominence"], c["speaker_id"], c["text_features"].numpy())
        si, db_b, qb = got[b]
        assert qb == want[2] and 1 <= len(qb) <= 3
        assert si == want[0], "clip %d: ranked names differ" % b
        assert db_b == want[1], "clip %d: reported bounds differ" % b
        assert all(len(v) == 10 for v in si.values())
    # the planted tier: the three copies lead clip 0's strongest word, in text-similarity order
    names = [s["sample_name"] for s in searched["smp"]]
    lead = got[0][0][searched["tie_query"]][:3]
    assert sorted(lead) == sorted(names[i] for i in (20, 120, 220))
    q_feat = clips[0]["text_features"].numpy()
    sims = [ref.text_similarity(q_feat, searched["smp"][names.index(n)]["text_feature"].numpy()) for n in lead]
    assert sims[0] > sims[1] > sims[2]


def test_search_without_query_words(rg, searched):
    c = searched["clips"][1]
    got = rg.retrieval.prosody_retrieval_batch(searched["pindex"], [([], 3, c["text_features"]),
                                                                    (c["prominence"], c["speaker_id"], c["text_features"]),
                                                                    ([("mm", 1.0, 1.0, 2.0)], 3, c["text_features"])])
    assert got[0] == ({}, {}, {}) and got[2] == ({}, {}, {})
    want = ref.retrieve(searched["smp"], c["prominence"], c["speaker_id"], c["text_features"].numpy())
    assert got[1] == want
    assert rg.retrieval.prosody_retrieval_batch(searched["pindex"], [([], 3, c["text_features"])]) == [({}, {}, {})]


# ---------------------------------------------------------------------------------------------------------- through the model
OUT_KEYS = ("prev_latentout", "pred_upper", "pred_lower", "pred_hands", "pred_facepose", "pred_exps", "pred_transl")


@pytest.fixture(scope="module")
def guided(rg):
    """The L2 all_encoder model of test_pipeline_gpu's retrieval-database test, over a 300-entry synthetic dataset."""
    cfg = rg.synth.default_model_cfg(num_layers=2)
    vae_cfgs = rg.synth.synth_vae_cfgs(decoder_arch="all_encoder", num_layers=2)
    ds = rg.synth.SyntheticDataset(300, seed=31)
    model = rg.build_architecture(rg.synth.reference_style_model_cfg(cfg, vae_cfgs, with_retrieval=True), database=ds,
                                  precision="bf16")
    model.load_state_dict(rg.synth.synth_full_state(0, cfg, vae_cfgs))
    return model.eval(), ds


def _batch(rg, ds, prominence):
    qs = [rg.synth.synth_llm_query(41), rg.synth.synth_llm_query(42)]
    d = rg.synth.synth_batch(2, seed=8)
    del d["discourse"]                                   # the method needs the prominence lists only
    d["prominence"] = [q["prominence"] if use else [] for q, use in zip(qs, prominence)]
    d["text_features"] = [q["text_features"] for q in qs]
    d["speaker_ids"] = torch.tensor([[q["speaker_id"]] * 150 for q in qs])
    d["sample_name"] = ["query_a", ds.names[3]]
    return d


def _run(rg, model, data, method="prosody"):
    ikw = dict(use_inversion=True, insertion_guidance=True, guidance_iters=GI, guidance_lr=0.1, noise_tape=rg.synth.NoiseTape(77))
    out = model(**dict(data, retrieval_method=method, inference_kwargs=ikw))
    torch.cuda.synchronize()
    return {k: out[k].detach().clone() for k in OUT_KEYS}, list(model.model.database.last_exemplars)


def _expected_exemplars(rg, ds, data):
    want = []
    for b in range(2):
        si, db_b, qb = ref.retrieve(ds.retrieval_samples, data["prominence"][b], int(data["speaker_ids"][b, 0]),
                                    data["text_features"][b].numpy())
        sel = {q: [s for s in names if s != data["sample_name"][b]][:1] for q, names in si.items()}
        want += [(b, qp, name, placed is not None) for qp, name, placed in rg.retrieval.place_exemplars(sel, db_b, qb, "prosody")]
    return want


def test_model_with_prosody_retrieval(rg, guided):
    model, ds = guided
    data = _batch(rg, ds, (True, True))
    assert "discourse" not in data and all(len(p) for p in data["prominence"])
    out, ex = _run(rg, model, data)
    want = _expected_exemplars(rg, ds, data)
    assert ex == want and {b for b, _, _, _ in ex} == {0, 1} and sum(placed for _, _, _, placed in ex) >= 2
    assert all(torch.isfinite(v).all() for v in out.values())
    again, ex2 = _run(rg, model, _batch(rg, ds, (True, True)))
    assert ex2 == ex and all(torch.equal(out[k], again[k]) for k in OUT_KEYS)


def test_model_clip_without_prominence_takes_the_base_path(rg, guided):
    model, ds = guided
    # one of two clips without a prominence list: no exemplar for it, the other keeps its own
    mixed = _batch(rg, ds, (True, False))
    out, ex = _run(rg, model, mixed)
    assert ex == _expected_exemplars(rg, ds, mixed) and ex and {b for b, _, _, _ in ex} == {0}
    assert all(torch.isfinite(v).all() for v in out.values())
    # no prominence at all: the run is the base path's, bit for bit (the discourse method over empty relation lists)
    none = _batch(rg, ds, (False, False))
    out, ex = _run(rg, model, none)
    base_data = dict(_batch(rg, ds, (False, False)), discourse=[[], []])
    base, ex_base = _run(rg, model, base_data, method="discourse")
    assert ex == [] and ex_base == [] and all(torch.equal(out[k], base[k]) for k in OUT_KEYS)
