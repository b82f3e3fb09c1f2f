"""GPU: the twin form of rg_seq2_forward (rg_seq_args.twin: one workgroup per clip runs the clip's conditional sequence and its
classifier-free twin TOGETHER) against the other launch forms.  The project's invariant is that every form gives
rg_seq_forward's bits, so every comparison here is torch.equal."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FORMS = dict(one=dict(seq_duo=False), duo=dict(seq_duo=True), twin=dict(seq_duo=True, seq_twin=True))


@pytest.fixture(scope="module")
def weights(rg):
    """(layers, tokens) -> DenoiserWeights, built once: T = 43 (the model's), T = 27 (< 32: the third token block is empty),
    and one full-depth model."""
    assert torch.cuda.is_available()
    out = {}
    for L, frames in ((2, 150), (2, 90), (8, 150)):
        cfg = rg.synth.default_model_cfg(num_layers=L)
        cfg["max_seq_len"] = frames
        W = rg.denoiser.DenoiserWeights(rg.synth.synth_denoiser_state(0, cfg), cfg, rg.schedule.Schedule(), "cuda")
        assert W.seq_streams is not None
        out[L, W.T] = W
    assert sorted(out) == [(2, 27), (2, 43), (8, 43)]
    return out


def _case(rg, B, T, seed, empty=False):
    """Inputs of B clips: motion masks with masked tokens, query masks that mask rows of every condition (other rows per
    condition and clip), optionally a clip without a valid token."""
    data = rg.synth.synth_batch(B, seed=seed)
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal((B, T, 512)).astype(np.float32)).cuda()
    n = (T - 3) // 4
    mm = torch.ones(B, T)
    mm[:, [n, 2 * n + 1, 3 * n + 2]] = 0
    mm[B - 1, T - 5:] = 0                  # a clip with masked motion tokens
    if empty:
        mm[B - 1] = 0                      # ... or without a valid token (the self-attention softmax over an empty set)
    qm = {c: torch.ones(B, T) for c in rg.denoiser.CONDS}
    for k, c in enumerate(rg.denoiser.CONDS):
        qm[c][:, [n, 2 * n, 3 * n]] = 0    # the separator rows, as the reference masks them
        qm[c][0, k] = 0                    # clip 0: one more row per condition, in the first token block
        qm[c][B - 1, T - 1 - k] = 0        # the last clip: in the last (partly filled) block
    return data, x, mm, qm


def _session(rg, W, B, case, **form):
    data, x, mm, qm = case
    sess = rg.denoiser.DenoiserSession(W, B, engine="seq", **form)
    sess.set_conditions(data["word"], data["audio"], data["speaker_ids"], mm, qm)
    assert sess.sq.twin == bool(form.get("seq_twin")) and sess.sq.args.twin == int(sess.sq.twin) and sess.sq.args.pairs == 0
    return sess


@pytest.mark.parametrize("T", [43, 27])
@pytest.mark.parametrize("B,empty", [(1, False), (3, False), (3, True)], ids=["B1", "B3", "B3-last-clip-all-masked"])
def test_twin_form_is_bit_identical(rg, weights, B, T, empty):
    """Head rows of all 2 B sequences: twin == one workgroup per sequence (rg_seq_forward) == two sequences of a kind per
    workgroup; B = 1 (nothing beside the clip), B = 3 (odd: the other two-sequence form computes a lone sequence twice), a
    partly empty third token block (T = 43) and an empty one (T = 27), masked query rows of every condition, a clip whose
    tokens are all masked; a replay gives the same bits."""
    W = weights[2, T]
    case = _case(rg, B, T, 100 + B, empty)
    outs = {}
    for name, form in FORMS.items():
        sess = _session(rg, W, B, case, **form)
        outs[name] = [sess.forward(case[1], step).clone() for step in (49, 7, 49)]
        torch.cuda.synchronize()
    for name in ("duo", "twin"):
        for i, (a, b) in enumerate(zip(outs[name], outs["one"])):
            a, b = a.view(2 * B, T, 512), b.view(2 * B, T, 512)
            assert torch.isfinite(a).all()
            for s in range(2 * B):
                assert torch.equal(a[s], b[s]), (name, i, "sequence %d" % s, (a[s] - b[s]).abs().max().item())
    assert torch.equal(outs["twin"][0], outs["twin"][2]) and not torch.equal(outs["one"][0], outs["one"][1])


@pytest.mark.parametrize("split", [0, 1, 3])
def test_twin_form_two_step_groups(rg, weights, split):
    """Clips [split, B) at another diffusion step in the same launch == the two separate forwards, and == the other forms."""
    B, T = 3, 43
    W = weights[2, T]
    case = _case(rg, B, T, 200)
    x = case[1]
    twin, one = _session(rg, W, B, case, **FORMS["twin"]), _session(rg, W, B, case, **FORMS["one"])
    both = twin.forward(x, 40, 9, split).clone().view(2, B, T, 512)
    a = twin.forward(x, 40).clone().view(2, B, T, 512)
    b = twin.forward(x, 9).clone().view(2, B, T, 512)
    ref = one.forward(x, 40, 9, split).clone().view(2, B, T, 512)
    torch.cuda.synchronize()
    assert torch.equal(both[:, :split], a[:, :split]) and torch.equal(both[:, split:], b[:, split:])
    assert torch.equal(both, ref) and not torch.equal(a, b)


def test_twin_form_full_depth(rg, weights):
    """L = 8: the fetch program at its full length (2 + 8 x 34 + 2 segments and the sentinel)."""
    B, T = 2, 43
    W = weights[8, T]
    case = _case(rg, B, T, 300)
    outs = {}
    for name, form in FORMS.items():
        sess = _session(rg, W, B, case, **form)
        outs[name] = [sess.forward(case[1], *st).clone() for st in ((49,), (23, 40, 1))]
        torch.cuda.synchronize()
    for name in ("duo", "twin"):
        for a, b in zip(outs[name], outs["one"]):
            assert torch.isfinite(a).all() and torch.equal(a, b), (name, (a - b).abs().max().item())


def test_twin_tail_equals_the_glue_launch(rg, weights):
    """With glue_ctr set a twin workgroup updates its clip itself (both head rows are its own: no arrival, the counters are not
    touched): whole loops, every forward ending with the step's update, against the same loops with the update in launches of
    their own -- a co-batched loop (n_b > 0; guided sampling with a first-step in_seq) and a guided sampling loop with an
    in_seq (n_b = 0), three runs each.  Then the SAME session runs the loop once more as two sequences of a kind per
    workgroup, whose tail counts arrivals: the counters kept the parity it expects."""
    T, D, n_a, n_b = 43, 512, 2, 3
    W = weights[2, T]
    S = W.schedule.num_timesteps
    g = np.random.Generator(np.random.PCG64(12))
    rnd = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32)).cuda()
    da, db = rg.synth.synth_batch(n_a, seed=5), rg.synth.synth_batch(n_b, seed=6)
    xa0, xb0 = rnd(n_a, T, D), rnd(n_b, T, D)
    inverted = rnd(S, n_a, T, D) * (torch.rand(S, n_a, T, 1, device="cuda") > 0.6)
    in_seq = rnd(n_a, T, D) * (torch.rand(n_a, T, 1, device="cuda") > 0.5)
    noise = rnd(S, n_a, T, D)
    GI = [2] * 25 + [0] * 25
    sc = rg.denoiser.DenoiserSession(W, n_a + n_b, engine="seq", **FORMS["twin"])
    ones = lambda n: {c: torch.ones(n, T) for c in rg.denoiser.CONDS}
    sc.set_conditions(da["word"], da["audio"], da["speaker_ids"], torch.ones(n_a, T), ones(n_a), offset=0, finalize=False)
    sc.set_conditions(db["word"], db["audio"], db["speaker_ids"], torch.ones(n_b, T), ones(n_b), offset=n_a)
    sa = rg.denoiser.DenoiserSession(W, n_a, engine="seq", **FORMS["twin"])
    sa.set_conditions(da["word"], da["audio"], da["speaker_ids"], torch.ones(n_a, T), ones(n_a))

    def cobatched(tail):
        x_all, out_b = torch.cat([xa0, xb0]).contiguous(), torch.empty(S, n_b, T, D, device="cuda")
        rg.sampler.cobatched_loop(sc, x_all, n_a, out_b, inverted_a=inverted, guidance_iters=GI, guidance_lr=0.1,
                                  inseq_noise_a=noise, in_seq_a=in_seq, tail_glue=tail)
        torch.cuda.synchronize()
        assert (sc.sq.args.glue_ctr is not None) == tail
        return x_all, out_b

    def alone(tail):
        rg.sampler.TAIL_GLUE = tail
        try:
            x = rg.sampler.ddim_guided_sample_loop(sa, xa0.clone(), inverted, GI, 0.1, noise, in_seq=in_seq)
        finally:
            rg.sampler.TAIL_GLUE = True
        torch.cuda.synchronize()
        assert (sa.sq.args.glue_ctr is not None) == tail
        return (x,)

    for loop, sess in ((cobatched, sc), (alone, sa)):
        ref = loop(False)
        assert all(torch.isfinite(t).all() for t in ref)
        for run in range(3):
            got = loop(True)
            assert all(torch.equal(a, b) for a, b in zip(got, ref)), (loop.__name__, "run %d of the tail form differs" % run)
        assert int(sess.sq.glue_ctr.abs().sum()) == 0          # 150 twin launches with the tail on: no arrival was counted
    # the same session, its counters as the twin launches left them, as two sequences of a kind per workgroup
    ref = cobatched(False)
    sc.sq.twin, sc.sq.args.twin = False, 0
    got = cobatched(True)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    assert sc.sq.glue_ctr.tolist() == [2 * S] * (n_a + n_b)      # two arrivals per clip and launch
    sc.sq.twin, sc.sq.args.twin = True, 1
    got = cobatched(True)
    assert all(torch.equal(a, b) for a, b in zip(got, ref)) and sc.sq.glue_ctr.tolist() == [2 * S] * (n_a + n_b)


def test_twin_refusals(rg, weights):
    """twin together with pairs, and a twin flag out of range, return the error instead of launching."""
    B, T = 2, 43
    W = weights[2, T]
    case = _case(rg, B, T, 400)
    x = case[1]
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = torch.full((2 * B * T, 512), 7.0, device="cuda")
    sess = _session(rg, W, B, case, **FORMS["twin"])
    a = sess.sq.args
    a.x, a.step, a.step_b, a.split, a.head = x.data_ptr(), 5, 5, B, head.data_ptr()
    a.pairs = 1
    assert sess.sq._fn(sess.h._h, ctypes.byref(a), stream()) != 0 and b"twin" in sess.h.lib.rg_last_error(sess.h._h)
    a.pairs, a.twin = 0, 2
    assert sess.sq._fn(sess.h._h, ctypes.byref(a), stream()) != 0 and b"twin" in sess.h.lib.rg_last_error(sess.h._h)
    torch.cuda.synchronize()
    assert bool((head == 7.0).all())                       # nothing ran
    for bad in (dict(seq_pairs=True, seq_duo=True), dict(seq_duo=False)):
        with pytest.raises(rg.capi.RgError):
            rg.denoiser.DenoiserSession(W, B, engine="seq", seq_twin=True, **bad)
