"""GPU: the grouped co-batched chains of the pipeline (MotionDiffusion(grouped_chains=True), the default: the chains of one
rotation of the batch lanes park and then advance as ONE chain of grouped launches, rg_seq2_forward_many) against the chains as
they were (grouped_chains=False: one chain per lane).  Same bits, so every comparison is torch.equal.  Two-layer models, two
clips per batch, the sessions forced into the flagship's launch form (twin), which batches this small do not take by themselves."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("pred_upper", "pred_lower", "pred_facepose", "pred_hands", "pred_transl", "pred_exps", "pred_contact", "prev_latentout")
GI = [2] * 25 + [0] * 25
B = 2
# fill-and-drain runs: 4 (no co-batched chain at all), 5 (one chain, alone at the flush), 8 (a complete window, then the drain),
# 9 (a window and a lone chain), 13 (two complete windows and a lone chain), 1 -- 40 in all, so the rotation over the four
# lanes is back at lane 0 when the sequence of runs is repeated
RUNS = (4, 5, 8, 9, 13, 1)
FORM = dict(seq_pairs=False, seq_duo=True, seq_twin=True)


def _batches(rg, n, dev):
    out = []
    for i in range(n):
        d = rg.synth.synth_batch(B, seed=700 + i, device=dev)
        qs = [rg.synth.synth_query(40 * i + j) for j in range(B)]
        d["discourse"] = [q["discourse"] for q in qs]
        d["prominence"] = [q["prominence"] for q in qs]
        d["text_features"] = [q["text_features"].to(dev) for q in qs]
        d["speaker_ids"] = torch.tensor([[q["speaker_id"]] * 150 for q in qs], device=dev)
        out.append(d)
    return out


def _run(rg, model, batches, n, kind=lambda i: ("guided", 0.1)):
    """One fill-and-drain run of n submissions; the results in the order they were handed out (submission order)."""
    got = []

    def keep(out):
        with torch.cuda.stream(out["done_stream"]):
            got.append({k: out[k].clone() for k in KEYS})
    for i in range(n):
        d = dict(batches[i])
        d["trans"] = batches[i]["trans"].clone()
        what, lr = kind(i)
        ikw = dict(noise_tape=rg.synth.NoiseTape(5000 + i))
        if what != "base":
            ikw.update(use_inversion=True, insertion_guidance=True, guidance_iters=GI, guidance_lr=lr)
        out = model.submit(**dict(d, retrieval_method="discourse", inference_kwargs=ikw))
        if out is not None:
            keep(out)
    for out in model.flush():
        keep(out)
    torch.cuda.synchronize()
    assert len(got) == n and model.flush() == [] and not model._parked
    return got


@pytest.fixture(scope="module")
def world(rg):
    """(model with grouped chains, model without, batches, the runs' results without): four batch lanes, two clips per batch."""
    dev = torch.device("cuda", 0)
    cfg = rg.synth.default_model_cfg(num_layers=2)
    vae_cfgs = rg.synth.synth_vae_cfgs(decoder_arch="all_encoder")
    models = []
    for grouped in (True, False):
        db = rg.synth.SyntheticDataset(512, seed=11, device=dev, feat_device=dev)
        m = rg.build_architecture(rg.synth.reference_style_model_cfg(cfg, vae_cfgs, with_retrieval=True), database=db, device=dev,
                                  calibrate_lanes=False, batch_lanes=4, async_results=True, grouped_chains=grouped, session_options=dict(FORM))
        m.load_state_dict(rg.synth.synth_full_state(0, cfg, vae_cfgs))
        m.eval()
        assert m.grouped_chains == grouped and m.batch_lanes == 4
        models.append(m)
    batches = _batches(rg, max(RUNS), dev)
    want = {n: _run(rg, models[1], batches, n) for n in RUNS}
    return models[0], models[1], batches, want


def _same(got, want, tag):
    assert len(got) == len(want), tag
    for i, (a, b) in enumerate(zip(got, want)):
        for k in KEYS:
            assert torch.isfinite(b[k]).all() and torch.equal(a[k], b[k]), (tag, "batch %d" % i, k, (a[k] - b[k]).abs().max().item())


def _many(model):
    return [k for k in model._graphs if k[0] == "cobatch_many"]


def _alone(model):
    return [k for k in model._graphs if k[0] == "cobatch"]


def test_grouped_chains_equal_the_chains_lane_by_lane(rg, world):
    """Runs of 4, 5, 8, 9, 13 and 1 submissions, option on against off: every result tensor of every batch in submission order,
    and as many results as submissions.  The grouped graph exists -- for the one set of lanes, at most one per window parity,
    whatever the lanes' own histories -- and a per-lane chain only where one was alone at a flush (the last submission of the
    runs of 5, 9 and 13: the 9th, 26th and 39th of the sequence, on lanes 0, 1 and 2 of the continuing rotation), one each;
    the sessions are in the twin form; a second identical sequence of runs captures no graph at all."""
    on, off, batches, want = world
    for n in RUNS:
        _same(_run(rg, on, batches, n), want[n], "run of %d" % n)
    many = _many(on)
    assert 1 <= len(many) <= 2 and all(tuple(o[2] for o in k[1]) == (0, 1, 2, 3) for k in many), many
    assert len({tuple(o[3] for o in k[1]) for k in many}) == len(many) and all(len({o[3] for o in k[1]}) == 1 for k in many)   # one slot per window
    assert sorted(k[3] for k in _alone(on)) == [0, 1, 2], _alone(on)
    assert not _many(off) and sorted({k[3] for k in _alone(off)}) == [0, 1, 2, 3]
    forms = {(s.sq.duo, s.sq.twin) for k, s in on._sessions.items() if k[1] == "cobatch"}
    assert forms == {(True, True)}, forms
    seen, captures = set(on._graphs), on.graph_captures
    for n in RUNS:
        _same(_run(rg, on, batches, n), want[n], "second sequence, run of %d" % n)
    assert on.graph_captures == captures and set(on._graphs) == seen


def test_grouped_chains_without_graphs(rg, world):
    """The same chains as eager launches (use_graphs off): the ordering between the caller's stream, the lanes' streams, the
    grouped chain's and the tails' is the streams' own, not a graph's.  A window and a lone chain."""
    on, off, batches, want = world
    on.use_graphs = False
    try:
        got = _run(rg, on, batches, 9)
    finally:
        on.use_graphs = True
    _same(got, want[9], "eager")


def test_a_batch_that_cannot_join_sends_the_parked_chains_first(rg, world):
    """Eleven submissions of which the third has another guidance rate -- its sampling is the chain of the seventh submission,
    in the middle of the second rotation's window, and fits neither the two chains parked in front of it nor the one behind
    -- and the tenth no exemplar inversion at all: the chains parked before each go first, grouped among themselves (twice a
    group of two) or alone, and the results stay in submission order (the pipeline itself refuses to hand them out otherwise)."""
    on, off, batches, want = world
    kind = lambda i: ("guided", 0.05) if i == 2 else (("base", 0.0) if i == 9 else ("guided", 0.1))
    ref = _run(rg, off, batches, 11, kind)
    before, r = set(_many(on)), on._submitted % 4         # (r: the lane of the run's first submission in the continuing rotation)
    _same(_run(rg, on, batches, 11, kind), ref, "mixed")
    new = [k for k in _many(on) if k not in before]
    pair = lambda a, b: tuple(sorted((a % 4, b % 4)))
    # submissions 5 and 6 in front of the odd chain; submissions 8 and 9 in front of the base batch
    assert sorted(tuple(o[2] for o in k[1]) for k in new) == sorted([pair(r, r + 1), pair(r + 3, r + 4)]), new
    assert any(k[3] == (r + 2) % 4 for k in _alone(on))   # the odd chain itself (submission 7), alone on its lane


def test_two_batch_lanes(rg, world):
    """A rotation over two lanes: windows of two chains."""
    on, off, batches, want = world
    try:
        for m in (on, off):
            m.batch_lanes = 2
        ref = _run(rg, off, batches, 7)
        _same(_run(rg, on, batches, 7), ref, "two lanes")
        assert any(tuple(o[2] for o in k[1]) == (0, 1) for k in _many(on))
    finally:
        for m in (on, off):
            m.batch_lanes = 4
