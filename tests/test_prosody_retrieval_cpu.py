"""The `prosody` retrieval method (exemplars by word prominence), host side: the DB dict, the query-word selection, the header
and the dispatch.  No device: the kernel and the search are tested in test_prosody_retrieval_gpu.py."""
import numpy as np
import pytest

import prosody_retrieval_ref as ref

PARENT_KEYS = ("idx_2_text", "idx_2_sense", "idx_2_discbounds", "idx_2_prominence", "idx_2_gesture_labels", "idx_2_gestprom")


def _same(a, b):
    import torch
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_build_db_dicts_adds_wordprom_and_moves_nothing(rg):
    smp = rg.synth.synth_retrieval_samples(40)
    db = rg.retrieval.build_db_dicts(smp)
    assert sorted(db) == sorted(PARENT_KEYS + ("idx_2_wordprom",))
    again = {k: v for k, v in rg.retrieval.build_db_dicts(smp).items() if k in PARENT_KEYS}
    assert list(again) == [k for k in db if k != "idx_2_wordprom"]          # same keys in the same order
    assert all(_same(db[k], again[k]) for k in again)
    # every cleanable word, in the record's order, in the sample's own seconds
    assert list(db["idx_2_wordprom"]) == [s["sample_name"] for s in smp]
    assert db["idx_2_wordprom"] == ref.wordprom(smp)
    assert sum(len(v) for v in db["idx_2_wordprom"].values()) == sum(len(s["prominence"]) for s in smp) > 40
    # cleaning: punctuation and case go, a word of punctuation alone is dropped
    one = dict(smp[0], prominence=[("Well,", 0.1, 0.3, 1.0), ("...", 0.3, 0.4, 2.0), ("don't", 0.5, 0.9, None)], discourse=[])
    assert rg.retrieval.build_db_dicts([one])["idx_2_wordprom"][one["sample_name"]] == [("well", 0.1, 0.3, 1.0), ("dont", 0.5, 0.9, None)]
    # stratified creation filters the new dict like the others
    strat = rg.retrieval.build_db_dicts(smp, stratified_db_creation=True, stratification_interval=30)
    assert list(strat["idx_2_wordprom"]) == list(strat["idx_2_sense"]) and 0 < len(strat["idx_2_sense"]) < 40


CLIP = [("so", 0.2, 0.5, 0.7),          # 0
        ("BIG,", 1.0, 1.4, 2.5),        # 1  one of two equal maxima: the earlier wins the first slot
        ("the", 1.8, 1.9, 2.4),         # 2  0.4 s behind word 1: dropped for the gap
        ("house", 3.0, 3.5, float("nan")),   # 3  unknown prominence
        ("was", 4.0, 4.0, 2.9),         # 4  zero length
        ("huge", 5.0, 5.6, 2.5),        # 5  the other maximum
        ("there", 7.0, 7.3, 1.1),       # 6
        ("late", 10.2, 10.6, 3.0)]      # 7  past the clip's 10 s


def test_prosody_queries_selection(rg):
    pq = rg.retrieval.prosody_queries
    qb, proms = pq(CLIP)
    assert qb == {0: ("big", "prosody", 1.0, 1.4), 1: ("huge", "prosody", 5.0, 5.6), 2: ("there", "prosody", 7.0, 7.3)}
    assert proms == [2.5, 2.5, 1.1]
    # the two equal maxima: with one slot the earlier one is taken
    assert pq(CLIP, max_queries=1) == ({0: ("big", "prosody", 1.0, 1.4)}, [2.5])
    assert pq(CLIP, max_queries=2)[0] == {0: ("big", "prosody", 1.0, 1.4), 1: ("huge", "prosody", 5.0, 5.6)}
    # the pair 0.4 s apart: without a gap the weaker one is a query too, and the result is still in start order
    qb0, proms0 = pq(CLIP, min_gap=0.0)
    assert [qb0[i][0] for i in range(3)] == ["big", "the", "huge"] and proms0 == [2.5, 2.4, 2.5]
    # exactly `min_gap` clear is clear (start >= end + gap)
    assert pq([("a", 0.0, 0.5, 2.0), ("b", 1.5, 2.0, 1.0)])[0] == {0: ("a", "prosody", 0.0, 0.5), 1: ("b", "prosody", 1.5, 2.0)}
    assert pq([("a", 0.0, 0.5, 2.0), ("b", 1.25, 2.0, 1.0)])[0] == {0: ("a", "prosody", 0.0, 0.5)}
    # a weaker word in FRONT of an accepted one: its end must be a gap before the accepted start
    assert pq([("a", 0.0, 0.5, 1.0), ("b", 1.25, 2.0, 2.0)])[0] == {0: ("b", "prosody", 1.25, 2.0)}
    # the floor on prominence, a longer clip, words that clean to nothing, no words
    assert pq(CLIP, min_prominence=2.45)[0] == {0: ("big", "prosody", 1.0, 1.4), 1: ("huge", "prosody", 5.0, 5.6)}
    assert pq(CLIP, max_queries=1, motion_seconds=11.0)[0] == {0: ("late", "prosody", 10.2, 10.6)}
    assert pq([("?!", 1.0, 2.0, 3.0), ("x", -2.0, -1.0, 3.0), ("y", 2.0, 3.0, None)]) == ({}, [])
    assert pq([]) == ({}, []) and pq(None) == ({}, [])
    # the restatement the device tests rank against selects the same
    g = np.random.Generator(np.random.PCG64(7))
    for seed in range(20):
        prom = rg.synth.synth_llm_query(seed)["prominence"]
        for kw in (dict(), dict(max_queries=2), dict(min_gap=0.3, max_queries=5), dict(min_prominence=float(g.uniform(0, 2)))):
            assert pq(prom, **kw) == ref.prosody_queries(prom, **kw)


def test_restatement_vectorised_equals_its_definition():
    """The two forms of the float64 restatement (word-by-word loop, whole-array numpy) agree bit for bit, ties included."""
    g = np.random.Generator(np.random.PCG64(11))
    words = ["w%d" % k for k in range(12)]
    entries = []
    for e in range(60):
        k = int(g.integers(0, 7)) if e % 9 else 0
        rows = [(words[int(g.integers(0, 12))], 0.0, float(g.integers(1, 5)) / 4, None if g.uniform() < 0.2 else float(g.integers(0, 6)) / 2)
                for _ in range(k)]
        entries.append(rows)
    t = ref.Table(entries, [int(g.integers(0, 3)) for _ in entries])
    for word, p_q, dur_q, spk_q in (("w3", 1.5, 0.5, 1), ("zz", 0.25, 0.05, 7)):
        sim = t.sim_row(word)
        a, b = ref.scores_loop(t, sim, p_q, dur_q, spk_q), ref.scores(t, sim, p_q, dur_q, spk_q)
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
        assert (a[1] >= 0).sum() > 30 and (a[1] == -1).sum() >= 7


def test_header_declares_the_sweep(rg):
    assert "rg_prosody_scores_batched" in rg.capi.header_symbols()
    assert rg.capi.header_constants()["RG_VERSION"] >= 132
    restype, argtypes = rg.capi.header_prototypes()["rg_prosody_scores_batched"]
    assert len(argtypes) == 16          # handle, 14 pointers and sizes, stream: no argument block


def _stub_database(rg, metadata):
    """A RetrievalDatabase around `metadata` without a device: the indices are stubbed."""
    db = object.__new__(rg.retrieval.RetrievalDatabase)
    db.num_retrieval, db.index, db.gesture_index, db.prosody_index = 1, None, None, None
    db.prosody_kwargs = dict(max_queries=3, min_gap=1.0, min_prominence=None, motion_seconds=10.0)
    db.test_indexes, db.test_dbounds, db.test_qbounds = {}, {}, {}
    assert "idx_2_wordprom" not in metadata
    return db


def test_dispatch_without_wordprom_and_unknown_method(rg):
    meta = {k: v for k, v in rg.retrieval.build_db_dicts(rg.synth.synth_retrieval_samples(8)).items() if k in PARENT_KEYS}
    assert sorted(meta) == sorted(rg.retrieval.LMDB_DICTS)          # the reference's six dicts: no word table
    db = _stub_database(rg, meta)
    with pytest.raises(rg.capi.RgError, match="idx_2_wordprom"):
        db.retrieve("prosody", None, None, CLIP, 3)
    with pytest.raises(NotImplementedError):
        db.retrieve("nonsense", None, None, CLIP, 3)
