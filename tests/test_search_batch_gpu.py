"""GPU: the batched exemplar search (one rg_discourse_search_batch call per batch -- sweep, survivor pack, one read-back, host
ranking, one launch for all tie tiers, one read-back; rg_rank_survivors_batch: the same from the pack on, over the lists of
any sweep) against the oracle (oracle/retrieval.py: retrieval, selection, placement), computed once on the CPU.  Everything
compared is compared exactly.

The database (a few hundred hand-made entries) is built so that the ranking meets: a tie tier that straddles the 10th place,
single-member tiers, fewer than 10 positive survivors, no positive survivor, a clip without relations, equal similarities
inside a tier, and a tier of more than 256 entries -- the test asserts that each of them occurs.

The oracle's tie-break similarities are fp32 (torch.mm, like the reference), the kernel's accumulate fp32 products in float64:
the anchor holds where both order every tier alike.  For the five clips over this database the oracle ranks the same with
fp32 and with float64 features (checked on the CPU; clip 0 gives [10, 4, 0]); should a changed seed break that, change the
seed, never an assertion."""
import zlib

import numpy as np
import pytest
import torch

from oracle import retrieval as oret

S0, S1, S2, S_NOBODY = "Contingency.Cause", "Expansion.Conjunction", "Comparison.Contrast", "Temporal.Nowhere"
FILLER = ("filler1", 0.05, 0.1, 1.0)


def _rel(conn, sense, cs):
    return (conn, sense, "a1", "a2", max(0.0, cs - 1.0), cs + 1.4, cs, cs + 0.4)


def _samples():
    g = np.random.default_rng(77)
    feat = lambda: torch.from_numpy(g.standard_normal((int(g.integers(8, 49)), 768)).astype(np.float32))
    recs = []

    def add(spk, disc, prom, f=None):
        recs.append(dict(sample_name="%d_spk%02d_0_%d/%d" % (spk, spk, len(recs), 15 * (len(recs) % 7)), speaker_id=spk,
                         discourse=disc, prominence=sorted(prom + [FILLER], key=lambda p: p[1]),
                         text_feature=feat() if f is None else f))
    q0 = _query_features()[0]
    for i in range(300):           # one tie tier of 300: same sense, connective, speaker, no prominence
        # eight of them resemble clip 0's text most, in four pairs of IDENTICAL features: equal similarities at the tier's head
        add(3, [_rel("because", S0, 1.0)], [], 3.0 * q0[:16 + 4 * ((i - 100) // 2)].clone() if 100 <= i < 108 else None)
    for p in (1.5, 1.0, 0.5):      # the same with a known prominence: three scores above the tier, one entry each
        add(3, [_rel("because", S0, 1.0)], [("because", 1.0, 1.4, p)])
    for i in range(4):             # the only entries of sense S1
        add(5, [_rel("so", S1, 2.0), _rel("because", S0, 4.0)] if i == 0 else [_rel("so", S1, 2.0)], [])
    for i in range(40):            # sense S2 with prominences all different: single-member tiers throughout
        add(int(g.integers(0, 25)), [_rel("but", S2, 1.0)], [("but", 1.0, 1.4, 0.05 + 0.07 * i)])
    for i in range(30):            # entries without any relation
        add(int(g.integers(0, 25)), [], [])
    return recs


def _query_features():
    g = torch.Generator().manual_seed(3)
    return [torch.randn(l, 768, generator=g) for l in (40, 12, 25, 48, 31)]


def _clips():
    """Five clips with 3, 0, 1, 3 and 3 relations."""
    f = _query_features()
    c0 = dict(discourse=[_rel("because", S0, 1.0), _rel("so", S1, 3.0), _rel("while", S_NOBODY, 5.0)],
              prominence=[FILLER, ("because", 1.0, 1.4, 1.5), ("so", 3.0, 3.4, 0.7)], speaker_id=3)
    c1 = dict(discourse=[], prominence=[FILLER], speaker_id=4)
    c2 = dict(discourse=[_rel("because", S0, 2.0)], prominence=[FILLER], speaker_id=9)
    c3 = dict(discourse=[_rel("but", S2, 1.0), _rel("so", S1, 3.0), _rel("because", S0, 5.0)],
              prominence=[FILLER, ("but", 1.0, 1.4, 1.02), ("because", 5.0, 5.4, 1.0)], speaker_id=5)
    c4 = dict(discourse=[_rel("although", S2, 1.0), _rel("because", S1, 3.0), _rel("so", S0, 5.0)],
              prominence=[FILLER], speaker_id=3)
    clips = [c0, c1, c2, c3, c4]
    for c, t in zip(clips, f):
        c["text_features"] = t
    return clips


class _Dataset:
    def __init__(self, rg, samples):
        self.rg, self.names, self.retrieval_samples = rg, [s["sample_name"] for s in samples], samples

    def __len__(self):
        return len(self.names)

    def __getitem__(self, key):
        name = self.names[0] if isinstance(key, int) else key
        d = self.rg.synth.synth_batch(1, seed=zlib.crc32(name.encode()) & 0x7FFFFFFF)
        out = {k: d[k][0] for k in ("motion", "motion_upper", "motion_lower", "motion_face", "motion_hands", "facial",
                                    "trans", "contact", "motion_mask", "word", "audio")}
        out["speaker_id"] = d["speaker_ids"][0]
        out["sample_name"] = name
        return out


@pytest.fixture(scope="module")
def vae(rg):
    vae_cfgs = rg.synth.synth_vae_cfgs(decoder_arch="all_encoder")
    P = {}
    for i, part in enumerate(rg.synth.PARTS):
        P.update(rg.synth.synth_vae_state(101 + i, vae_cfgs[part], prefix="gesture_rep_encoder.%s_vae." % part))
    return rg.vae.GestureRepEncoder(P, vae_cfgs, "cuda", "fp32")


@pytest.fixture(scope="module")
def rdb(rg):
    return rg.retrieval.RetrievalDatabase(num_retrieval=1, dataset=_Dataset(rg, _samples()), device="cuda")


def _cond(clips):
    return dict(text_features=[c["text_features"] for c in clips], discourse=[c["discourse"] for c in clips],
                prominence=[c["prominence"] for c in clips],
                speaker_ids=torch.tensor([[c["speaker_id"]] * 150 for c in clips]))


def _forward(rdb, vae, clips, method="discourse", extra=None):
    """Everything the search decides, for one forward: the visited exemplars, the placements, the whole ranking per clip."""
    for d in (rdb.test_indexes, rdb.test_dbounds, rdb.test_qbounds):
        d.clear()
    idx = ["clip_%d" % b for b in range(len(clips))]
    re = rdb(dict(_cond(clips), **(extra or {})), [150] * len(clips), "cuda", idx=idx, retrieval_method=method, gesture_rep_encoder=vae)
    return dict(last_exemplars=list(rdb.last_exemplars), retr_startends=re["retr_startends"], query_startends=re["query_startends"],
                names=re["raw_sample_names"], type2words=re["raw_type2words"], indexes=dict(rdb.test_indexes),
                dbounds=dict(rdb.test_dbounds), qbounds=dict(rdb.test_qbounds))


def _expected(retrieved, method="discourse"):
    """What _forward returns for a batch, from the oracle: retrieved = per clip the oracle's (sample_indexes, d_bounds,
    query_bounds); selection (own name "clip_<b>"), visiting order and placement as oracle.retrieval.database_forward."""
    out = dict(last_exemplars=[], retr_startends=[], query_startends=[], names=[], type2words=[], indexes={}, dbounds={}, qbounds={})
    for b, (si, dbb, qb) in enumerate(retrieved):
        own = "clip_%d" % b
        out["indexes"][own], out["dbounds"][own], out["qbounds"][own] = {method: si}, {method: dbb}, {method: qb}
        sel = oret.select_retrieved(si, own, 1)
        placed = oret.place_exemplars(sel, dbb, qb, method)
        for qp, smp_idxs in sel.items():     # (every visited exemplar is fetched, placed or not)
            if len(smp_idxs) == 0 or qp not in qb or qb[qp][2] > qb[qp][3]:
                continue
            out["last_exemplars"].append((b, qp, smp_idxs[0], qp in placed))
        out["retr_startends"].append({qp: v[1] for qp, v in placed.items()})
        out["query_startends"].append({qp: v[2] for qp, v in placed.items()})
        out["names"].append({qb[qp][0]: v[0] for qp, v in placed.items()})
        out["type2words"].append({qp: (qb[qp][0], qb[qp][1], dbb[qp][v[0]][0], dbb[qp][v[0]][1]) for qp, v in placed.items()})
    return out


@pytest.fixture(scope="module")
def oracle_clips():
    """The oracle's discourse retrieval of each of the five clips, once."""
    db = oret.build_db_dicts(_samples())
    return [oret.discourse_retrieval(c["discourse"], c["prominence"], c["speaker_id"], db, c["text_features"]) for c in _clips()]


@pytest.fixture(scope="module")
def expected(oracle_clips):
    """The five clips as one batch."""
    return _expected(oracle_clips)


def _tiers(surv):
    """The score tiers of one query's survivors (entries ascending, scores) that the walk can reach, grouped by equal score."""
    entry, score = surv[0], surv[1]
    tiers, held = [], 0
    for sc in sorted({v for v in score.tolist() if v > 0}, reverse=True):
        if held >= 10:
            break
        tiers.append([int(e) for e, v in zip(entry, score) if v == sc])
        held += len(tiers[-1])
    return tiers


@pytest.mark.gpu
def test_database_holds_every_kind_of_ranking(rg, rdb):
    """From the sweep's survivors (grouped by equal score here) and the similarities of one rg_text_diag_sim_many launch."""
    R, index = rg.retrieval, rdb.index
    kinds = set()
    clips = _clips()
    assert [len(c["discourse"]) for c in clips] == [3, 0, 1, 3, 3]
    for c in clips:
        if not c["discourse"]:
            kinds.add("no relations")
            continue
        q_dev = c["text_features"].cuda()
        swept = index.collect(index.sweep_async(R.discourse_queries(c["discourse"], c["prominence"], c["speaker_id"])))
        tiers = [_tiers(surv) for surv in swept]
        multi = [t for ts in tiers for t in ts if len(t) > 1]
        pe = np.array([e for t in multi for e in t], dtype=np.int32)
        sims = torch.empty(len(pe), dtype=torch.float64, device="cuda")
        if len(pe):
            qp, ql, pq = np.array([q_dev.data_ptr()], dtype=np.uint64), np.array([q_dev.shape[0]], dtype=np.int32), np.zeros(len(pe), dtype=np.int32)
            index.h.call("text_diag_sim_many", qp.ctypes.data, ql.ctypes.data, 1, pe.ctypes.data, pq.ctypes.data, len(pe), index.feats,
                         index.feat_off, index.n, index.dim, sims)
        sims = np.split(sims.cpu().numpy(), np.cumsum([len(t) for t in multi])[:-1]) if multi else []
        for ts in tiers:
            held = np.cumsum([0] + [len(t) for t in ts])
            kinds |= {"straddle" for i in range(len(ts)) if held[i] < 10 < held[i + 1]}
            kinds |= {"single" for t in ts if len(t) == 1} | {"more than 256" for t in ts if len(t) > 256}
            kinds |= {"fewer than 10"} if 0 < held[-1] < 10 else set()
            kinds |= {"none positive"} if held[-1] == 0 else set()
        for s in sims:
            head = np.sort(s)[::-1][:10]
            kinds |= {"equal similarities"} if len(np.unique(head)) < len(head) else set()
    assert kinds == {"no relations", "straddle", "single", "more than 256", "fewer than 10", "none positive", "equal similarities"}, kinds


def _same(a, b):
    assert a["last_exemplars"] == b["last_exemplars"]
    for k in ("retr_startends", "query_startends", "names", "type2words", "indexes", "dbounds", "qbounds"):
        assert a[k] == b[k], k


@pytest.mark.gpu
def test_batch_equals_the_oracle(rdb, vae, expected):
    new = _forward(rdb, vae, _clips())
    _same(new, expected)
    assert len(new["last_exemplars"]) >= 8 and new["indexes"]["clip_1"]["discourse"] == {}
    assert [len(v) for v in new["indexes"]["clip_0"]["discourse"].values()] == [10, 4, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("b", [0, 1, 2])
def test_batch_of_one_clip(rdb, vae, oracle_clips, b):
    """Clips of 3, 0 and 1 relations, each alone in its batch."""
    _same(_forward(rdb, vae, [_clips()[b]]), _expected([oracle_clips[b]]))


@pytest.mark.gpu
def test_retrieve_equals_the_oracle(rdb, oracle_clips):
    for c, (si, dbb, qb) in zip(_clips(), oracle_clips):
        got = rdb.retrieve("discourse", c["text_features"], c["discourse"], c["prominence"], c["speaker_id"], idx="own")
        assert got + (dict(rdb.test_indexes["own"]),) == (oret.select_retrieved(si, "own", 1), dbb, qb, {"discourse": si})


@pytest.mark.gpu
def test_survivor_block_grows_when_a_batch_does_not_fit(rdb, vae, expected):
    """A block of 64 rows against more than 600 survivors: the pack writes the counts alone, the host grows the block and
    packs again -- same answer; the next batch fits at once."""
    index = rdb.index
    try:
        assert index.pack_rows(64) == 64
        _same(_forward(rdb, vae, _clips()), expected)
        grown = index.pack_rows()
        assert grown >= 600
        _same(_forward(rdb, vae, _clips()), expected)
        assert index.pack_rows() == grown
    finally:
        index.pack_rows(4096)
    assert index.pack_rows() == 4096


@pytest.mark.gpu
def test_rank_survivors_equals_search_batch(rg, rdb):
    """rg_rank_survivors_batch over the device lists of sweep_async for the five clips == rg_discourse_search_batch on the same
    queries, with the default survivor block and with a 64-row one (the grow path); its argument checks refuse a null
    pointer, n_queries == 0 and dim % 4 != 0 before anything is launched."""
    R, index = rg.retrieval, rdb.index
    queries, feats = [], []
    for c in _clips():
        qs = R.discourse_queries(c["discourse"], c["prominence"], c["speaker_id"]) if c["discourse"] else []
        queries += qs
        feats += [c["text_features"].cuda()] * len(qs)
    assert len(queries) == 10
    want = index.search_batch(queries, feats)
    assert [len(e) for e, _ in want[:3]] == [10, 4, 0]
    t = index.sweep_async(queries)
    try:
        for rows in (4096, 64):
            assert index.pack_rows(rows) == rows
            assert index.rank_survivors(t["cursor"], t["idx"], t["top"], t["score"], feats) == want
        assert index.pack_rows() >= 600
    finally:
        index.pack_rows(4096)
    # refused calls: the result arrays keep their sentinel, the next good call is unaffected
    Q, cap = t["idx"].shape
    qp = np.array([f.data_ptr() for f in feats], dtype=np.uint64)
    ql = np.array([f.shape[0] for f in feats], dtype=np.int32)
    n_ranked, entry, top = (np.full(shape, -7, dtype=np.int32) for shape in ((Q,), (Q, 10), (Q, 10)))
    good = [t["cursor"], t["idx"], t["top"], t["score"], Q, cap, index.feats, index.feat_off, index.n, index.dim, qp.ctypes.data,
            ql.ctypes.data, n_ranked.ctypes.data, entry.ctypes.data, top.ctypes.data]
    for pos, bad, msg in ((0, None, "null pointer"), (3, None, "null pointer"), (10, None, "null pointer"), (14, None, "null pointer"),
                          (4, 0, "bad shape"), (9, index.dim + 2, "bad shape")):
        args = list(good)
        args[pos] = bad
        with pytest.raises(rg.capi.RgError, match=msg):
            index.h.call("rank_survivors_batch", *args)
    assert (n_ranked == -7).all() and (entry == -7).all() and (top == -7).all()
    assert index.rank_survivors(t["cursor"], t["idx"], t["top"], t["score"], feats) == want


@pytest.mark.gpu
def test_gesture_type_ranking_equals_the_oracle(rg, vae):
    """gesture_type: the labels' survivor lists stay on the device and are ranked by rg_rank_survivors_batch; retrieval,
    selection and placement equal the oracle's.  On this 300-sample database the oracle ranks both clips' labels the same
    with fp32 and with float64 text features (checked on the CPU), so its fp32 tie-break is a valid anchor here."""
    smp = rg.synth.synth_retrieval_samples(300)
    db = rg.retrieval.RetrievalDatabase(num_retrieval=1, dataset=_Dataset(rg, smp), device="cuda",
                                        word_similarity=rg.synth.synth_word_similarity)
    qs = [rg.synth.synth_query(21), rg.synth.synth_query(22)]
    clips = [dict(q, text_features=q["text_features"]) for q in qs]
    labels = [rg.synth.synth_gesture_query(21, 3), rg.synth.synth_gesture_query(22, 2)]
    odb = oret.build_db_dicts(smp)
    want = _expected([oret.gesture_type_retrieval(labels[b], qs[b]["speaker_id"], odb["idx_2_gesture_labels"], qs[b]["text_features"],
                                                  odb["idx_2_text"], rg.synth.synth_word_similarity) for b in range(2)], "gesture_type")
    new = _forward(db, vae, clips, "gesture_type", extra=dict(gesture_labels=labels))
    _same(new, want)
    assert len(new["last_exemplars"]) >= 2
