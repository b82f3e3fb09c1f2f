"""The `motion` retrieval method (exemplars by a motion example) on the device: the sweep kernel against the float64
restatement, the index against the VAE's posterior encode, and the method through the model.

The sweep's fp32 sums S_p are compared within (n_q D + 2) 2^-24 relative -- the bound of a sum of n_q D non-negative terms of
one subtraction and one fused multiply-add each, not a measured tolerance; everything behind them (the float64 score from the
device's own sums, indices, names, independence of the batch) exactly."""
import numpy as np
import pytest
import torch

import motion_retrieval_ref as ref

pytestmark = pytest.mark.gpu

N, L, D = 70, 10, 512
N_QS = (1, 2, 3, 7, 10)
WEIGHTS = ((1.0, 1.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 1.0))
QSPK = (0, 1, 2, 7, 1)            # the queries' speakers (7: nobody's)


def _base(rg, spk, seed=9):
    """A DiscourseIndex over len(spk) entries that carries speakers and tie-break text features only."""
    g = np.random.Generator(np.random.PCG64(seed))
    names = ["m%03d" % e for e in range(len(spk))]
    feats = {n: torch.from_numpy(g.standard_normal((int(g.integers(3, 7)), 8)).astype(np.float32)) for n in names}
    db = dict(idx_2_sense={n: [int(spk[e])] for e, n in enumerate(names)}, idx_2_prominence={n: {} for n in names},
              idx_2_text={n: (feats[n], int(spk[e])) for e, n in enumerate(names)})
    return rg.retrieval.DiscourseIndex(db, "cuda"), feats


@pytest.fixture(scope="module")
def kern(rg):
    assert torch.cuda.is_available()
    lat, spk, qlats = ref.fixture(0, N, L, D, N_QS)
    base, feats = _base(rg, spk)
    mindex = rg.retrieval.MotionIndex(base, torch.from_numpy(lat).cuda())
    # the restatement, computed once and shared (not modified): per weights and query (score, top, S, d) at bonus 0
    want = {(wi, qi): ref.scores(lat, spk, qlats[qi], w, QSPK[qi], 0.0) for wi, w in enumerate(WEIGHTS) for qi in range(len(N_QS))}
    return dict(mindex=mindex, lat=lat, spk=spk, qlats=qlats, want=want, base=base, feats=feats)


def _queries(kern, wi, which, bonus=0.0):
    return [(torch.from_numpy(kern["qlats"][qi]).clone(), WEIGHTS[wi], QSPK[qi], bonus) for qi in which]


def _check_against_restatement(kern, mindex, lat, spk, wi, which, count):
    """One launch against the restatement; returns (pairs whose `top` the fp32 bound leaves undecided, pairs)."""
    score, top, sums = mindex.scores(_queries(kern, wi, which), with_sums=True)
    torch.cuda.synchronize()
    n = lat.shape[0]
    assert score.shape == top.shape == (len(which), n) and sums.shape == (len(which), n, 4)
    assert score.dtype == torch.float64 and top.dtype == torch.int32 and sums.dtype == torch.float32
    score, top, sums = score.cpu().numpy(), top.cpu().numpy(), sums.cpu().numpy()
    w = WEIGHTS[wi]
    left_out = 0
    for row, qi in enumerate(which):
        n_q = N_QS[qi]
        _, top64, S64, d64 = kern["want"][(wi, qi)] if count else ref.scores(lat, spk, kern["qlats"][qi], w, QSPK[qi], 0.0)
        b = ref.sum_bound(n_q, D)
        assert ((top[row] >= 0) & (top[row] <= L - n_q)).all()
        # (1) the device's sums at the device's offset, within the bound of the exact ones
        at = S64[np.arange(n), :, top[row]]                                   # [n, 4]
        for p in range(4):
            if w[p] > 0:
                err = np.abs(sums[row, :, p].astype(np.float64) - at[:, p]) / at[:, p]
                print("weights %r n_q %d part %d: max relative error of S_p %.3g (bound %.3g)" % (w, n_q, p, err.max(), b))
                assert (err <= b).all(), (w, n_q, p, err.max(), b)
            else:
                assert (sums[row, :, p] == 0).all()
        # (2) the score from the device's own sums, in float64: bit for bit
        d_dev = ref.distances(sums[row][:, :, None], w)[:, 0]
        again = ref.score_of(d_dev, n_q, D, w, spk, QSPK[qi], 0.0)
        assert again.tobytes() == score[row].tobytes(), (w, n_q, np.flatnonzero(again != score[row])[:5])
        # (3) the offset, wherever the runner-up is further away than the bound lets either move
        if d64.shape[1] > 1:
            srt = np.sort(d64, axis=1)
            decided = srt[:, 1] * (1 - 2 * b) > srt[:, 0] * (1 + 2 * b)
        else:
            decided = np.ones(n, dtype=bool)
        assert np.array_equal(top[row][decided], top64[decided]), (w, n_q)
        left_out += int((~decided).sum())
    return left_out, len(which) * n


# ----------------------------------------------------------------------------------------------------------------- the sweep
def test_sweep_against_restatement_mixed_batch(rg, kern):
    """Q = 5, n_q = 1, 2, 3, 7, 10 mixed in one launch, for each of the three weightings: 1 050 (query, entry) pairs."""
    out = total = 0
    for wi in range(len(WEIGHTS)):
        a, b = _check_against_restatement(kern, kern["mindex"], kern["lat"], kern["spk"], wi, [0, 1, 2, 3, 4], True)
        out, total = out + a, total + b
    print("offset left undecided by the fp32 bound for %d of %d pairs" % (out, total))
    assert total == 1050 and out <= 0.02 * total


@pytest.mark.parametrize("wi", range(len(WEIGHTS)), ids=lambda wi: "w" + "".join("%g" % v for v in WEIGHTS[wi]))
@pytest.mark.parametrize("qi", range(len(N_QS)), ids=lambda qi: "nq%d" % N_QS[qi])
def test_sweep_against_restatement_single_query(rg, kern, wi, qi):
    _check_against_restatement(kern, kern["mindex"], kern["lat"], kern["spk"], wi, [qi], True)


def test_sweep_one_entry(rg, kern):
    lat, spk = kern["lat"][41:42].copy(), kern["spk"][41:42].copy()
    base, _ = _base(rg, spk)
    one = rg.retrieval.MotionIndex(base, torch.from_numpy(lat).cuda())
    for wi in range(len(WEIGHTS)):
        _check_against_restatement(kern, one, lat, spk, wi, [0, 1, 2, 3, 4], False)
        _check_against_restatement(kern, one, lat, spk, wi, [2], False)


def test_sweep_shorter_window(rg):
    """L < 10 takes the kernel's general path (bounds as predicates instead of per-n_q unrolled code): a small table of its own,
    n_q = 1, 2, 6 of L = 6, D = 64, all parts weighed unevenly."""
    Ls, Ds, n_qs, w = 6, 64, (1, 2, 6), (0.5, 1.0, 2.0, 0.25)
    lat, spk, qlats = ref.fixture(3, 9, Ls, Ds, n_qs)
    lat[5, :, 0:2, :] = lat[5, :, 3:5, :]                            # two offsets of entry 5 tie for a query cut from it
    qlats[1] = lat[5, :, 3:5, :].copy()
    base, _ = _base(rg, spk)
    short = rg.retrieval.MotionIndex(base, torch.from_numpy(lat).cuda())
    score, top, sums = short.scores([(torch.from_numpy(q), w, 1, 0.5) for q in qlats], with_sums=True)
    score, top, sums = score.cpu().numpy(), top.cpu().numpy(), sums.cpu().numpy()
    assert top[1, 5] == 0 and score[1, 5] == (1.5 if spk[5] == 1 else 1.0)
    for row, q in enumerate(qlats):
        n_q, b = n_qs[row], ref.sum_bound(n_qs[row], Ds)
        s64, t64, S64, d64 = ref.scores(lat, spk, q, w, 1, 0.5)
        at = S64[np.arange(9), :, top[row]]
        ok = at > 0
        assert (np.abs(sums[row].astype(np.float64) - at)[ok] <= b * at[ok]).all() and (sums[row][~ok] == 0).all()
        again = ref.score_of(ref.distances(sums[row][:, :, None], w)[:, 0], n_q, Ds, w, spk, 1, 0.5)
        assert again.tobytes() == score[row].tobytes()
        srt = np.sort(d64, axis=1)
        decided = srt[:, 1] * (1 - 2 * b) > srt[:, 0] * (1 + 2 * b) if d64.shape[1] > 1 else np.ones(9, dtype=bool)
        decided[5] |= row == 1                                       # (the planted tie: exactly equal on the device too)
        assert np.array_equal(top[row][decided], t64[decided])


@pytest.fixture(scope="module")
def planted(rg, kern):
    """Entry 37's chunks 4 ... 6 are the example, bit for bit; the same chunks sit in entry 12 at offset 0."""
    lat = kern["lat"].copy()
    lat[12, :, 0:3, :] = lat[37, :, 4:7, :]
    return dict(mindex=rg.retrieval.MotionIndex(kern["base"], torch.from_numpy(lat).cuda()), lat=lat, q=torch.from_numpy(lat[37, :, 4:7, :].copy()))


@pytest.mark.parametrize("w", WEIGHTS + ((0.3, 2.5, 0.0, 7.0),), ids=lambda w: "w" + "_".join("%g" % v for v in w))
def test_planted_example_scores_exactly_one(rg, kern, planted, w):
    spk = kern["spk"]
    score, top = planted["mindex"].scores([(planted["q"], w, int(spk[37]), 0.0), (planted["q"], w, int(spk[37]), 0.25)])
    s, t = score.cpu().numpy(), top.cpu().numpy()
    assert s[0, 37] == 1.0 and t[0, 37] == 4 and s[0, 12] == 1.0 and t[0, 12] == 0
    assert s[1, 37] == 1.25 and s[1, 12] == (1.25 if spk[12] == spk[37] else 1.0)
    others = np.delete(s[0], [12, 37])
    assert (others < 1.0).all() and (others > 0).all()


def test_planted_example_ranks_first(rg, kern, planted):
    mindex, base, spk = planted["mindex"], kern["base"], kern["spk"]
    g = np.random.Generator(np.random.PCG64(77))
    q_feat = torch.from_numpy(g.standard_normal((5, 8)).astype(np.float32))
    queries = [(planted["q"], WEIGHTS[0], 7, 0.0), (planted["q"], WEIGHTS[1], int(spk[37]), 0.25)]
    score, _ = mindex.scores(queries)
    swept = mindex.sweep(queries)
    ranked = base.rank_survivors(swept["cursor"], swept["idx"], swept["top"], swept["score"], [q_feat.cuda()] * 2)
    counts = swept["cursor"].cpu().numpy()
    for q in range(2):
        entries, tops = ranked[q]
        alive = set(swept["idx"][q, :counts[q]].cpu().tolist())
        assert {12, 37} <= alive                                   # both copies survive the selection
        # the ranking walk of the restatement over the DEVICE's scores orders the entries as the device does
        names = base.names
        walk = ref.ranking_walk(score[q].cpu().numpy(), lambda e: ref.text_similarity(q_feat.numpy(), kern["feats"][names[e]].numpy()))
        assert entries == walk and len(entries) == 10
        assert dict(zip(entries, tops))[37] == 4 and dict(zip(entries, tops))[12] == 0
    # without a bonus the two copies tie at exactly 1.0 and lead, in text-similarity order
    sims = {e: ref.text_similarity(q_feat.numpy(), kern["feats"][base.names[e]].numpy()) for e in (12, 37)}
    assert ranked[0][0][:2] == sorted((12, 37), key=lambda e: -sims[e])
    # with the bonus for entry 37's speaker it is first on its own unless entry 12 shares the speaker
    assert ranked[1][0][0] == 37 or spk[12] == spk[37]


def test_parts_without_weight_are_not_read(rg, kern):
    for wi, dead in ((0, (2, 3)), (2, (0, 1, 2))):
        lat = kern["lat"].copy()
        lat[:, list(dead), :, :] = np.nan
        poisoned = rg.retrieval.MotionIndex(kern["base"], torch.from_numpy(lat).cuda())
        queries = _queries(kern, wi, [0, 1, 2, 3, 4])
        for q in queries:                        # the queries' rows of those parts as well
            q[0][list(dead)] = float("nan")
        score, top = poisoned.scores(queries)
        clean = kern["mindex"].scores(_queries(kern, wi, [0, 1, 2, 3, 4]))
        assert torch.isfinite(score).all()
        assert torch.equal(score.view(torch.int64), clean[0].view(torch.int64)) and torch.equal(top, clean[1])


def test_speaker_bonus_is_added_for_matching_speakers_only(rg, kern):
    plain, top0 = kern["mindex"].scores(_queries(kern, 0, [0, 1, 2, 3, 4], 0.0))
    bonus, top1 = kern["mindex"].scores(_queries(kern, 0, [0, 1, 2, 3, 4], 0.5))
    plain, bonus = plain.cpu().numpy(), bonus.cpu().numpy()
    assert torch.equal(top0, top1)
    for row, speaker in enumerate(QSPK):
        same = kern["spk"] == speaker
        assert np.array_equal(bonus[row][same], plain[row][same] + 0.5) and np.array_equal(bonus[row][~same], plain[row][~same])
        assert same.any() == (speaker != 7)


def test_a_batch_equals_its_queries_alone_and_repeats(rg, kern):
    for wi in range(len(WEIGHTS)):
        queries = _queries(kern, wi, [0, 1, 2, 3, 4], 0.125)
        batch = kern["mindex"].scores(queries, with_sums=True)
        again = kern["mindex"].scores(queries, with_sums=True)
        assert batch[0].data_ptr() != again[0].data_ptr()
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(batch, again))
        for row, q in enumerate(queries):
            alone = kern["mindex"].scores([q], with_sums=True)
            assert all(torch.equal(a[row:row + 1].view(torch.int32), b.view(torch.int32)) for a, b in zip(batch, alone)), (wi, row)


def test_argument_refusals_leave_the_outputs_untouched(rg, kern):
    m = kern["mindex"]
    qlat = torch.zeros(2 * 4 * 10 * D, device="cuda")
    score = torch.full((2, N), -7.0, dtype=torch.float64, device="cuda")
    top = torch.full((2, N), -7, dtype=torch.int32, device="cuda")
    sums = torch.full((2, N, 4), -7.0, dtype=torch.float32, device="cuda")

    def call(off, weights, Dd=D):
        off = np.asarray(off, dtype=np.int32)
        Q = len(off) - 1
        par = np.array([list(w) + [0.0, 0.0] for w in weights], dtype=np.float64).reshape(Q, 6)
        m.h.call("motion_scores_batched", m.lat, N, L, Dd, m.spk, qlat, torch.from_numpy(off).cuda(), off.ctypes.data,
                 torch.from_numpy(par).cuda(), par.ctypes.data, Q, score, top, sums)

    ok = (1.0, 1.0, 0.0, 0.0)
    for off, weights, word in (([0, 0], [ok], "n_q"), ([0, 11], [ok], "n_q"), ([0, 3, 2], [ok, ok], "not decrease"),
                               ([0, 3], [(0.0, 0.0, 0.0, 0.0)], "all be zero"), ([0, 3], [(1.0, -1.0, 0.0, 0.0)], "non-negative"),
                               ([0, 3], [(1.0, float("nan"), 0.0, 0.0)], "finite")):
        with pytest.raises(rg.capi.RgError, match=word):
            call(off, weights)
    with pytest.raises(rg.capi.RgError, match="multiple of 4"):
        call([0, 3], [ok], Dd=510)
    torch.cuda.synchronize()
    assert (score == -7.0).all() and (top == -7).all() and (sums == -7.0).all()
    call([0, 3, 5], [ok, ok])                    # the same buffers are written by a call that is accepted
    torch.cuda.synchronize()
    assert (score > 0).all() and (top >= 0).all()


# ------------------------------------------------------------------------------------------- the index, through the model
OUT_KEYS = ("prev_latentout", "pred_upper", "pred_lower", "pred_hands", "pred_facepose", "pred_exps", "pred_transl")
GI = [0] * 25 + list(range(25))
PLANT, AT, NQ = 137, 4, 3          # the example: chunks 4 ... 6 of database window 137


def _model(rg, ds, **kw):
    cfg = rg.synth.default_model_cfg(num_layers=2)
    vae_cfgs = rg.synth.synth_vae_cfgs(decoder_arch="all_encoder", num_layers=2)
    model = rg.build_architecture(rg.synth.reference_style_model_cfg(cfg, vae_cfgs, with_retrieval=True), database=ds,
                                  precision="bf16", **kw)
    model.load_state_dict(rg.synth.synth_full_state(0, cfg, vae_cfgs))
    return model.eval()


@pytest.fixture(scope="module")
def guided(rg):
    """The 2-layer all_encoder model and 300-entry synthetic database of test_prosody_retrieval_gpu's `guided` fixture, with the
    table of motion latents built."""
    ds = rg.synth.SyntheticDataset(300, seed=31)
    model = _model(rg, ds)
    mindex = model.build_motion_index(batch=64)
    assert mindex is model.model.database.motion_index
    return model, ds


def _records_means(rg, model, ds, entries):
    gre = model.model.gesture_rep_encoder
    names = model.model.database.index.names
    mu = rg.retrieval.posterior_means(gre, [ds[names[e]] for e in entries], L)
    return mu.view(len(entries), 4, L, D)


def test_index_rows_equal_a_fresh_posterior_encode(rg, guided):
    model, ds = guided
    mindex = model.model.database.motion_index
    assert mindex.lat.shape == (300, 4, L, D) and mindex.lat.dtype == torch.float32 and mindex.lat.is_contiguous()
    assert torch.isfinite(mindex.lat).all()
    for entries in ([0, 1, 2], [63, 64, 65, 299], [PLANT]):          # across the build's batches of 64, other batch sizes
        fresh = _records_means(rg, model, ds, entries)
        assert torch.equal(mindex.lat[entries], fresh), entries
    assert not torch.equal(mindex.lat[0], mindex.lat[1])


def _example(ds, name, first_chunk, n_chunks):
    rec = ds[name]
    return {k: rec[k][15 * first_chunk:15 * (first_chunk + n_chunks)].clone() for k in ref.EXAMPLE_KEYS}


def test_a_chunk_in_its_window_equals_the_chunk_in_a_padded_example(rg, guided):
    """What the padded example encode relies on: a chunk's posterior depends on that chunk alone.  It holds bit for bit for the
    upper body, the hands and the face at any offset; the lower part's input carries the translation relative to the first frame
    of the encoded span, so its chunks agree only for an example that starts where its window starts."""
    model, ds = guided
    db = model.model.database
    gre, mindex, name = model.model.gesture_rep_encoder, db.motion_index, db.index.names[PLANT]
    qlat, q_off = rg.retrieval.example_latents(gre, [(_example(ds, name, AT, NQ), NQ), (_example(ds, name, 0, 2), 2),
                                                     (_example(ds, name, 9, 1), 1)], L)
    assert q_off.tolist() == [0, 3, 5, 6] and qlat.numel() == 6 * 4 * D
    mid = qlat[:NQ * 4 * D].view(4, NQ, D)
    head = qlat[NQ * 4 * D:5 * 4 * D].view(4, 2, D)
    last = qlat[5 * 4 * D:].view(4, 1, D)
    for p in (0, 1, 2):
        assert torch.equal(mid[p], mindex.lat[PLANT, p, AT:AT + NQ]), p
        assert torch.equal(head[p], mindex.lat[PLANT, p, 0:2]), p
        assert torch.equal(last[p], mindex.lat[PLANT, p, 9:10]), p
    assert torch.equal(head[3], mindex.lat[PLANT, 3, 0:2])


def test_a_table_beyond_the_budget_is_refused(rg, guided):
    model, ds = guided
    db = model.model.database
    need = rg.retrieval.MotionIndex.table_bytes(300, L, D)
    with pytest.raises(rg.capi.RgError, match="motion_index_bytes"):
        rg.retrieval.MotionIndex.build(db.index, model.model.gesture_rep_encoder, lambda n: ds[n], L, motion_index_bytes=need - 1)


def _batch(rg, ds, with_query=True):
    qs = [rg.synth.synth_llm_query(41), rg.synth.synth_llm_query(42)]
    d = rg.synth.synth_batch(2, seed=8)
    d["text_features"] = [q["text_features"] for q in qs]
    d["speaker_ids"] = torch.tensor([[q["speaker_id"]] * 150 for q in qs])
    d["sample_name"] = ["query_a", ds.names[3]]
    d["motion_queries"] = [[(4.0, 5.0, _example(ds, ds.names[PLANT], AT, NQ))] if with_query else [], []]
    return d


def _ikw(rg):
    return dict(use_inversion=True, insertion_guidance=True, guidance_iters=GI, guidance_lr=0.1, noise_tape=rg.synth.NoiseTape(77))


def _run(rg, model, data, method="motion"):
    out = model(**dict(data, retrieval_method=method, inference_kwargs=_ikw(rg)))
    torch.cuda.synchronize()
    return {k: out[k].detach().clone() for k in OUT_KEYS}, list(model.model.database.last_exemplars), out["retrieval_dict"]


def test_model_with_motion_retrieval(rg, guided):
    model, ds = guided
    db = model.model.database
    assert db.index.names == ds.names
    name = db.index.names[PLANT]
    out, ex, rd = _run(rg, model, _batch(rg, ds))
    # clip 0 reports the database window its example was cut from, chunks 4 ... 6, centred on second 4-5 (chunks 2 ... 4);
    # clip 1 has no query and no exemplar
    assert ex == [(0, 0, name, True)]
    assert rd["retr_startends"] == [{0: (AT, AT + NQ)}, {}] and rd["query_startends"] == [{0: (2, 5)}, {}]
    ranked = db.test_indexes["query_a"]["motion"]
    assert list(ranked) == [0] and ranked[0][0] == name and len(ranked[0]) == 10
    assert db.test_dbounds["query_a"]["motion"][0][name] == ("motion", "motion", 4.0, 7.0)
    assert list(db.test_dbounds["query_a"]["motion"][0]) == ranked[0]
    assert db.test_qbounds["query_a"]["motion"] == {0: ("motion", "motion", 4.0, 5.0)}
    assert all(torch.isfinite(v).all() for v in out.values())
    again, ex2, _ = _run(rg, model, _batch(rg, ds))
    assert ex2 == ex and all(torch.equal(out[k], again[k]) for k in OUT_KEYS)
    # without any query the run is the base path's, bit for bit (the discourse method over empty relation lists); with the
    # query, clip 0 differs from it
    none, ex_none, _ = _run(rg, model, _batch(rg, ds, with_query=False))
    base_data = _batch(rg, ds, with_query=False)
    del base_data["motion_queries"]
    base, ex_base, _ = _run(rg, model, base_data, method="discourse")
    assert ex_none == [] and ex_base == [] and all(torch.equal(none[k], base[k]) for k in OUT_KEYS)
    assert not torch.equal(out["prev_latentout"][0], base["prev_latentout"][0])


def test_model_clip_without_queries_equals_the_base_path(rg, guided):
    """The second clip of the mixed batch (no query) gets what the base path gets: three empty dicts from the search, no
    exemplar, and the rows of the retrieval dict a batch without any query has for it.  (Its generated motion is NOT compared
    with that batch's: the noise tape is consumed in order and the first clip's exemplar draws from it first, so the second
    clip samples from other noise with an exemplar in the batch than without -- under every method.  The whole batch against
    the base path, bit for bit, is test_model_with_motion_retrieval's last part.)"""
    model, ds = guided
    db = model.model.database
    data = _batch(rg, ds)
    found = db.motion_batch([(data["motion_queries"][b], 3, data["text_features"][b]) for b in range(2)], model.model.gesture_rep_encoder)
    assert found[1] == ({}, {}, {}) and list(found[0][0]) == [0]
    _, ex, mixed = _run(rg, model, data)
    _, _, none = _run(rg, model, _batch(rg, ds, with_query=False))
    assert [b for b, _, _, _ in ex] == [0]
    for key in ("re_mask", "raw_motion_latents", "raw_motion", "raw_trans", "raw_facial", "raw_latent_mask"):
        assert torch.equal(mixed[key][1], none[key][1]) and not mixed[key][1].any(), key
        if key in ("re_mask", "raw_motion_latents", "raw_latent_mask"):
            assert mixed[key][0].any(), key                       # (the first clip does hold its exemplar)
    for key in ("retr_startends", "query_startends", "retr_uncropped_latents", "raw_sample_names"):
        assert mixed[key][1] == {} and none[key][1] == {} and none[key][0] == {} and list(mixed[key][0]) in ([0], ["motion"])


def test_submit_and_flush_equal_the_synchronous_call(rg, guided):
    model, ds = guided
    want, ex, _ = _run(rg, model, _batch(rg, ds))
    pipe = _model(rg, ds, async_results=True, calibrate_lanes=False)
    got = []
    first = pipe.submit(**dict(_batch(rg, ds), retrieval_method="motion", inference_kwargs=_ikw(rg)))
    for out in ([first] if first is not None else []) + pipe.flush():
        with torch.cuda.stream(out["done_stream"]):
            got.append({k: out[k].clone() for k in OUT_KEYS})
    torch.cuda.synchronize()
    assert len(got) == 1 and list(pipe.model.database.last_exemplars) == ex
    assert pipe.model.database.motion_index is not None            # built on the first motion call
    assert all(torch.equal(got[0][k], want[k]) for k in OUT_KEYS)
    # new weights: the table of the old VAE's latents goes
    cfg, vae_cfgs = rg.synth.default_model_cfg(num_layers=2), rg.synth.synth_vae_cfgs(decoder_arch="all_encoder", num_layers=2)
    pipe.load_state_dict(rg.synth.synth_full_state(0, cfg, vae_cfgs))
    assert pipe.model.database.motion_index is None


def test_nearest_motions(rg, guided):
    model, ds = guided
    db = model.model.database
    name = db.index.names[PLANT]
    near = db.nearest_motions(_example(ds, name, AT, NQ), k=5)
    assert len(near) == 5 and near[0] == (name, AT, 0.0)
    assert all(a[2] <= b[2] for a, b in zip(near, near[1:])) and near[1][2] > 0
    spks = db.index.spk.cpu().tolist()
    only = db.nearest_motions(_example(ds, name, AT, NQ), k=300, speaker_id=spks[PLANT])
    assert only[0] == (name, AT, 0.0) and {n for n, _, _ in only} == {db.index.names[e] for e in range(300) if spks[e] == spks[PLANT]}
