"""GPU: the batched exemplar search (RetrievalDatabase.batched_search: one rg_discourse_search_batch call per batch -- sweep,
survivor pack, one read-back, host ranking, one launch for all tie tiers, one read-back) against the path it replaces (a
sweep, four read-backs, one launch and one upload per tie tier), which the same object takes with the option off.  Everything
compared is compared exactly.

The database (a few hundred hand-made entries) is built so that the ranking meets: a tie tier that straddles the 10th place,
single-member tiers, fewer than 10 positive survivors, no positive survivor, a clip without relations, equal similarities
inside a tier, and a tier of more than 256 entries -- the test asserts, with the existing path's own tier logic, that each of
them occurs."""
import zlib

import numpy as np
import pytest
import torch

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


def _forward(rdb, vae, clips, method="discourse", on=True, extra=None):
    """Everything the search decides, for one forward: the visited exemplars, the placements, the whole ranking per clip."""
    rdb.batched_search = on
    assert rdb.batched_search is on and rdb.index.batched_sims is on
    for d in (rdb.test_indexes, rdb.test_dbounds, rdb.test_qbounds):
        d.clear()
    idx = ["clip_%d" % b for b in range(len(clips))]
    re = rdb(dict(_cond(clips), **(extra or {})), [150] * len(clips), "cuda", idx=idx, retrieval_method=method, gesture_rep_encoder=vae)
    return dict(last_exemplars=list(rdb.last_exemplars), retr_startends=re["retr_startends"], query_startends=re["query_startends"],
                names=re["raw_sample_names"], type2words=re["raw_type2words"], indexes=dict(rdb.test_indexes),
                dbounds=dict(rdb.test_dbounds), qbounds=dict(rdb.test_qbounds))


@pytest.fixture(scope="module")
def old_path(rdb, vae):
    """The option off, once: the five clips as one batch."""
    out = _forward(rdb, vae, _clips(), on=False)
    rdb.batched_search = True
    return out


@pytest.mark.gpu
def test_database_holds_every_kind_of_ranking(rg, rdb):
    """With the existing path's tier logic (collect's order, _cut_tiers, the similarities of sims_async)."""
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
        for surv in swept:
            sims = []
            tiers, _ = R._cut_tiers(index, q_dev, surv, sims)
            held = np.cumsum([0] + [len(t) for t, _ in tiers])
            kinds |= {"straddle" for i in range(len(tiers)) if held[i] < 10 < held[i + 1]}
            kinds |= {"single" for t, _ in tiers if len(t) == 1} | {"more than 256" for t, _ in tiers if len(t) > 256}
            kinds |= {"fewer than 10"} if 0 < held[-1] < 10 else set()
            kinds |= {"none positive"} if held[-1] == 0 else set()
            for t, slot in tiers:
                if slot is not None:
                    s = sims[slot].cpu().numpy()
                    head = np.sort(s)[::-1][:10]
                    kinds |= {"equal similarities"} if len(np.unique(head)) < len(head) else set()
    assert kinds == {"no relations", "straddle", "single", "more than 256", "fewer than 10", "none positive", "equal similarities"}, kinds


def _same(a, b):
    assert a["last_exemplars"] == b["last_exemplars"]
    for k in ("retr_startends", "query_startends", "names", "type2words", "indexes", "dbounds", "qbounds"):
        assert a[k] == b[k], k


@pytest.mark.gpu
def test_batch_equals_the_old_path(rdb, vae, old_path):
    new = _forward(rdb, vae, _clips(), on=True)
    _same(new, old_path)
    assert len(new["last_exemplars"]) >= 8 and new["indexes"]["clip_1"]["discourse"] == {}
    assert [len(v) for v in new["indexes"]["clip_0"]["discourse"].values()] == [10, 4, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("b", [0, 1, 2])
def test_batch_of_one_clip(rdb, vae, b):
    """Clips of 3, 0 and 1 relations, each alone in its batch."""
    clip = [_clips()[b]]
    _same(_forward(rdb, vae, clip, on=True), _forward(rdb, vae, clip, on=False))


@pytest.mark.gpu
def test_retrieve_equals_the_old_path(rdb):
    for c in _clips():
        got = {}
        for on in (True, False):
            rdb.batched_search = on
            got[on] = rdb.retrieve("discourse", c["text_features"], c["discourse"], c["prominence"], c["speaker_id"], idx="own")
            got[on] += (dict(rdb.test_indexes["own"]),)
        assert got[True] == got[False]
    rdb.batched_search = True


@pytest.mark.gpu
def test_survivor_block_grows_when_a_batch_does_not_fit(rdb, vae, old_path):
    """A block of 64 rows against more than 600 survivors: the pack writes the counts alone, the host grows the block and
    packs again -- same answer; the next batch fits at once."""
    index = rdb.index
    try:
        assert index.pack_rows(64) == 64
        _same(_forward(rdb, vae, _clips(), on=True), old_path)
        grown = index.pack_rows()
        assert grown >= 600
        _same(_forward(rdb, vae, _clips(), on=True), old_path)
        assert index.pack_rows() == grown
    finally:
        index.pack_rows(4096)
    assert index.pack_rows() == 4096


@pytest.mark.gpu
def test_gesture_type_tiers_in_one_launch(rg, vae):
    """gesture_type: the tie tiers of a clip's labels go through one rg_text_diag_sim_many launch and one read-back."""
    smp = rg.synth.synth_retrieval_samples(300)
    db = rg.retrieval.RetrievalDatabase(num_retrieval=1, dataset=_Dataset(rg, smp), device="cuda",
                                        word_similarity=rg.synth.synth_word_similarity)
    qs = [rg.synth.synth_query(21), rg.synth.synth_query(22)]
    clips = [dict(q, text_features=q["text_features"]) for q in qs]
    labels = dict(gesture_labels=[rg.synth.synth_gesture_query(21, 3), rg.synth.synth_gesture_query(22, 2)])
    new = _forward(db, vae, clips, "gesture_type", on=True, extra=labels)
    _same(new, _forward(db, vae, clips, "gesture_type", on=False, extra=labels))
    assert len(new["last_exemplars"]) >= 2
