"""GPU: the grouped drain of the co-batched pipeline (MotionDiffusion(grouped_drain=True), the default: the pending batches
that flush() finishes together run their sampling loops as ONE chain of grouped launches, rg_seq_forward_many) against the
drain as it was (grouped_drain=False: one chain per batch).  Same bits, so every comparison is torch.equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("pred_upper", "pred_lower", "pred_facepose", "pred_hands", "pred_transl", "pred_exps", "pred_contact", "prev_latentout")
GI = [2] * 25 + [0] * 25
B = 2
# fill-and-drain runs: as many submissions as lanes, one and five more (a lane then holds a batch whose predecessor went through
# a co-batched chain), and two (a drain of two batches) -- 20 in all, so the rotation over the four lanes is back at lane 0
RUNS = (4, 5, 9, 2)


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


@pytest.fixture(scope="module")
def world(rg):
    """(model with the grouped drain, model without, batches): two-layer models with four batch lanes, two clips per batch."""
    dev = torch.device("cuda", 0)
    cfg = rg.synth.default_model_cfg(num_layers=2)
    vae_cfgs = rg.synth.synth_vae_cfgs(decoder_arch="all_encoder")
    models = []
    for grouped in (True, False):
        db = rg.synth.SyntheticDataset(512, seed=11, device=dev, feat_device=dev)
        m = rg.build_architecture(rg.synth.reference_style_model_cfg(cfg, vae_cfgs, with_retrieval=True), database=db, device=dev,
                                  calibrate_lanes=False, batch_lanes=4, async_results=True, grouped_drain=grouped)
        m.load_state_dict(rg.synth.synth_full_state(0, cfg, vae_cfgs))
        m.eval()
        assert m.grouped_drain == grouped and m.batch_lanes == 4
        models.append(m)
    return models[0], models[1], _batches(rg, max(RUNS), dev)


def _run(rg, model, batches, n, lr=lambda i: 0.1, plain=False):
    """One fill-and-drain run of n submissions; the results in the order they were handed out (submission order)."""
    got = []

    def keep(out):
        with torch.cuda.stream(out["done_stream"]):
            got.append({k: out[k].clone() for k in KEYS})
    for i in range(n):
        d = dict(batches[i])
        d["trans"] = batches[i]["trans"].clone()
        ikw = dict(use_inversion=True, noise_tape=rg.synth.NoiseTape(5000 + i))
        if not plain:
            ikw.update(insertion_guidance=True, guidance_iters=GI, guidance_lr=lr(i))
        out = model.submit(**dict(d, retrieval_method="discourse", inference_kwargs=ikw))
        if out is not None:
            keep(out)
    for out in model.flush():
        keep(out)
    torch.cuda.synchronize()
    assert len(got) == n and model.flush() == []
    return got


def _same(got, want, tag):
    for i, (a, b) in enumerate(zip(got, want)):
        for k in KEYS:
            assert torch.isfinite(b[k]).all() and torch.equal(a[k], b[k]), (tag, "batch %d" % i, k, (a[k] - b[k]).abs().max().item())


def _many(model):
    return [k for k in model._graphs if k[0] in ("guided_many", "sample_many")]


def test_grouped_drain_equals_the_drain_batch_by_batch(rg, world):
    """Runs of 4, 5, 9 and 2 submissions, option on against off: every result tensor of every batch, in submission order.  The
    grouped graphs exist -- one per set of draining lanes, whatever the slots the lanes' earlier batches took -- and the old
    ones do not; a second identical sequence of runs captures no graph at all."""
    on, off, batches = world
    want = [_run(rg, off, batches, n) for n in RUNS]
    for n, w in zip(RUNS, want):
        _same(_run(rg, on, batches, n), w, "run of %d" % n)
    lanes = sorted(tuple(o[2] for o in k[1]) for k in _many(on))
    assert lanes == [(0, 1, 2, 3), (2, 3)] and all(      # (the run of two follows 18 submissions: lanes 2 and 3)
        k[0] == "guided_many" for k in _many(on)), lanes
    assert not any(k[0] == "guided" for k in on._graphs) and not _many(off) and any(k[0] == "guided" for k in off._graphs)
    seen, captures = set(on._graphs), on.graph_captures
    for n, w in zip(RUNS, want):
        _same(_run(rg, on, batches, n), w, "second sequence, run of %d" % n)
    assert on.graph_captures == captures and set(on._graphs) == seen


def test_grouped_drain_without_graphs(rg, world):
    """The same chain as eager launches (use_graphs off): the ordering between the lanes' streams, the grouped chain's and the
    tails' is the streams' own, not a graph's."""
    on, off, batches = world
    want = _run(rg, off, batches, 5)
    on.use_graphs = False
    try:
        got = _run(rg, on, batches, 5)
    finally:
        on.use_graphs = True
    _same(got, want, "eager")


def test_a_batch_that_does_not_qualify_drains_alone(rg, world):
    """Four pending batches of which the third has another guidance rate: it finishes in a chain of its own between the others'
    tails (results stay in submission order), the other three share theirs.  And plain DDIM sampling (no insertion guidance)
    groups too."""
    on, off, batches = world
    lr = lambda i: 0.05 if i == 2 else 0.1
    _same(_run(rg, on, batches, 4, lr), _run(rg, off, batches, 4, lr), "mixed guidance rates")
    three = [k for k in _many(on) if len(k[1]) == 3]
    alone = [k for k in on._graphs if k[0] == "guided"]
    assert len(three) == 1 and len(alone) == 1
    assert sorted([o[2] for o in three[0][1]] + [alone[0][2]]) == [0, 1, 2, 3]      # (lanes: three in the group, the odd one's own)
    _same(_run(rg, on, batches, 4, plain=True), _run(rg, off, batches, 4, plain=True), "plain sampling")
    assert any(k[0] == "sample_many" and len(k[1]) == 4 for k in on._graphs)
