"""GPU: rg_seq_forward_many (the forwards of several sessions in ONE launch: workgroup -> (session, block of the session), then
rg_seq_kernel's body on that session's arguments) against rg_seq_forward session by session, and the sampling loops built on
it (sampler.sample_loop_many) against the loops one by one.  A grouped launch must give rg_seq_forward's bits, tail included,
so every comparison here is torch.equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GI = [2] * 25 + [0] * 25


@pytest.fixture(scope="module")
def weights(rg):
    """tokens -> DenoiserWeights of a two-layer model, built once: T = 43 (the model's) and T = 27 (the third token block empty)."""
    assert torch.cuda.is_available()
    out = {}
    for frames in (150, 90):
        cfg = rg.synth.default_model_cfg(num_layers=2)
        cfg["max_seq_len"] = frames
        W = rg.denoiser.DenoiserWeights(rg.synth.synth_denoiser_state(0, cfg), cfg, rg.schedule.Schedule(), "cuda")
        assert W.seq_streams is not None
        out[W.T] = W
    assert sorted(out) == [27, 43]
    return out


def _rnd(seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32)).cuda()


def _session(rg, W, B, seed, empty=False):
    """A one-workgroup-per-sequence session of B clips with its conditions set: motion masks with masked tokens, query masks
    that mask rows of every condition (other rows per condition and clip), optionally a clip without a valid token."""
    T = W.T
    data = rg.synth.synth_batch(B, seed=seed)
    n = (T - 3) // 4
    mm = torch.ones(B, T)
    mm[:, [n, 2 * n + 1, 3 * n + 2]] = 0
    mm[B - 1, T - 5:] = 0
    if empty:
        mm[B - 1] = 0                      # no valid token: the self-attention softmax over an empty set
    qm = {c: torch.ones(B, T) for c in rg.denoiser.CONDS}
    for k, c in enumerate(rg.denoiser.CONDS):
        qm[c][:, [n, 2 * n, 3 * n]] = 0    # the separator rows, as the reference masks them
        qm[c][0, k] = 0                    # clip 0: one more masked query row per condition, in the first token block
        qm[c][B - 1, T - 1 - k] = 0        # the last clip: in the last (partly filled) block
    sess = rg.denoiser.DenoiserSession(W, B, engine="seq", seq_duo=False)
    sess.set_conditions(data["word"], data["audio"], data["speaker_ids"], mm, qm)
    assert sess.sq.groupable()
    return sess


@pytest.mark.parametrize("T", [43, 27])
@pytest.mark.parametrize("Bs,empty", [((1,), False), ((3, 1), False), ((2, 3, 1), False), ((2, 3, 1), True)],
                         ids=["B1", "B3+1", "B2+3+1", "B2+3+1-a-clip-all-masked"])
def test_grouped_forward_is_bit_identical(rg, weights, Bs, T, empty):
    """Head rows of every sequence of every session: one grouped launch == rg_seq_forward per session, each session at a step
    of its own (one of them with two step groups); one session alone, sessions of odd and unequal sizes (a session's first
    workgroup is at an odd place in the grid), masked query rows of every condition, a clip whose tokens are all masked in the
    MIDDLE session; a second grouped launch gives the same bits."""
    W = weights[T]
    rnd = _rnd(10 * len(Bs) + T)
    sessions = [_session(rg, W, B, 100 + 7 * k + B, empty and k == 1) for k, B in enumerate(Bs)]
    xs = [rnd(B, T, 512) for B in Bs]
    calls = [dict(x=xs[k], step=(49, 7, 23)[k]) for k in range(len(Bs))]
    if len(Bs) > 1:
        calls[1].update(step_b=31, split=1)
    ref = [s.forward(**kw).clone() for s, kw in zip(sessions, calls)]
    got = []
    for rep in range(2):
        for s in sessions:
            s.head.fill_(float("nan"))
        heads = rg.denoiser.DenoiserSession.forward_many(sessions, calls)
        got.append([h.clone() for h in heads])
    torch.cuda.synchronize()
    for k, B in enumerate(Bs):
        a, b = got[0][k].view(2 * B, T, 512), ref[k].view(2 * B, T, 512)
        assert torch.isfinite(b).all()
        for q in range(2 * B):
            assert torch.equal(a[q], b[q]), ("session %d" % k, "sequence %d" % q, (a[q] - b[q]).abs().max().item())
        assert torch.equal(got[1][k], got[0][k])
    if len(Bs) > 1:
        assert not torch.equal(ref[0].view(2, Bs[0], T, 512)[:, 0], ref[1].view(2, Bs[1], T, 512)[:, 0])


@pytest.mark.parametrize("T", [43, 27])
def test_grouped_forward_tails(rg, weights, T):
    """With glue_ctr set every session's forward ends with ITS loop step's update, read from the session's place in the
    parameter block: sessions in the sampling form (the next step's in_seq marks rows, two guidance iterations), in the
    inversion form (the level also kept) and without a tail, in one launch; two consecutive steps, so that the arrival
    counters carry over; head rows and x after each against rg_seq_forward with the tail on, session by session.  Then a
    whole guided loop on one of the sessions, whose tail counts arrivals on the counters the grouped launches left."""
    W = weights[T]
    S = W.schedule.num_timesteps
    Bs, D = (2, 3, 1, 2), 512
    rnd = _rnd(500 + T)
    sessions = [_session(rg, W, B, 300 + k, empty=(k == 1)) for k, B in enumerate(Bs)]
    x0 = [rnd(B, T, D) for B in Bs]
    in_seq = [rnd(B, T, D) * (torch.rand(B, T, 1, device="cuda") > 0.5) for B in Bs]
    noise = [rnd(B, T, D) for B in Bs]
    glue = rg.sampler._glue

    def calls(xs, keep, i):
        return [dict(x=xs[0], step=i, glue=glue(sessions[0], 0.1, i=i, x_a=xs[0], n_a=Bs[0], nxt=in_seq[0], noise_nxt=noise[0], g_next=2)),
                dict(x=xs[1], step=S - 1 - i, glue=glue(sessions[1], k=S - 1 - i, x_b=xs[1], keep_b=keep, n_b=Bs[1])),
                dict(x=xs[2], step=i),
                dict(x=xs[3], step=i, glue=glue(sessions[3], 0.1, i=i, x_a=xs[3], n_a=Bs[3], nxt=None))]

    def run(many):
        xs, keep, seen = [x.clone() for x in x0], torch.zeros(Bs[1], T, D, device="cuda"), []
        for i in (30, 29):
            cs = calls(xs, keep, i)
            if many:
                rg.denoiser.DenoiserSession.forward_many(sessions, cs)
            else:
                for s, kw in zip(sessions, cs):
                    s.forward(**kw)
            seen.append([s.head.clone() for s in sessions] + [x.clone() for x in xs] + [keep.clone()])
        torch.cuda.synchronize()
        return seen
    ref = run(False)
    ctr = [s.sq.glue_ctr.tolist() for s in sessions]
    assert ctr == [[4] * Bs[0], [4] * Bs[1], [0] * Bs[2], [4] * Bs[3]]          # two arrivals per clip and launch with a tail
    got = run(True)
    for step, (g, r) in enumerate(zip(got, ref)):
        for j, (a, b) in enumerate(zip(g, r)):
            assert torch.isfinite(b).all() and torch.equal(a, b), ("step %d" % step, "tensor %d" % j, (a - b).abs().max().item())
    assert not torch.equal(ref[0][4], x0[0]) and not torch.equal(ref[1][4], ref[0][4])      # x moved, step after step
    assert [s.sq.glue_ctr.tolist() for s in sessions] == [[8] * Bs[0], [8] * Bs[1], [0] * Bs[2], [8] * Bs[3]]
    # the counting form on session 1, its counters as the grouped launches left them
    sess, B = sessions[1], Bs[1]
    inverted = rnd(S, B, T, D) * (torch.rand(S, B, T, 1, device="cuda") > 0.6)
    nz = rnd(S, B, T, D)
    rg.sampler.TAIL_GLUE = False
    try:
        want = rg.sampler.ddim_guided_sample_loop(sess, x0[1].clone(), inverted, GI, 0.1, nz, in_seq=in_seq[1])
    finally:
        rg.sampler.TAIL_GLUE = True
    have = rg.sampler.ddim_guided_sample_loop(sess, x0[1].clone(), inverted, GI, 0.1, nz, in_seq=in_seq[1])
    torch.cuda.synchronize()
    assert torch.isfinite(want).all() and torch.equal(have, want)
    assert sess.sq.glue_ctr.tolist() == [8 + 2 * S] * B


def test_grouped_forward_refuses_on_the_device_side_too(rg, weights):
    """What the entry point refuses reaches the caller as an error and nothing runs: sessions of two models, a session in
    another launch form."""
    a, b = _session(rg, weights[43], 1, 1), _session(rg, weights[27], 1, 2)
    xa, xb = torch.zeros(1, 43, 512, device="cuda"), torch.zeros(1, 27, 512, device="cuda")
    for s in (a, b):
        s.head.fill_(7.0)
    with pytest.raises(rg.capi.RgError, match="rg_seq_forward_many: the sessions must agree in L, T and S"):
        rg.denoiser.DenoiserSession.forward_many([a, b], [dict(x=xa, step=3), dict(x=xb, step=3)])
    duo = rg.denoiser.DenoiserSession(weights[43], 1, engine="seq", seq_duo=True)
    with pytest.raises(rg.capi.RgError, match="one-workgroup-per-sequence"):
        rg.denoiser.DenoiserSession.forward_many([a, duo], [dict(x=xa, step=3), dict(x=xa, step=3)])
    torch.cuda.synchronize()
    assert bool((a.head == 7.0).all()) and bool((b.head == 7.0).all())


@pytest.mark.parametrize("guided", [True, False])
def test_many_session_loop_equals_the_loops_one_by_one(rg, weights, guided):
    """sample_loop_many over sessions of 2, 1 and 3 clips, the full schedule: every session's x == ddim_guided_sample_loop
    (guided; a first-step in_seq for two of the sessions) or ddim_sample_loop (plain, with in_seq) on that session alone."""
    T, D, Bs = 43, 512, (2, 1, 3)
    W = weights[T]
    S = W.schedule.num_timesteps
    rnd = _rnd(900 + guided)
    sessions = [_session(rg, W, B, 600 + k) for k, B in enumerate(Bs)]
    x0 = [rnd(B, T, D) for B in Bs]
    in_seq = [rnd(B, T, D) * (torch.rand(B, T, 1, device="cuda") > 0.5) if k != 1 else None for k, B in enumerate(Bs)]
    noise = [rnd(S, B, T, D) for B in Bs]
    inverted = [rnd(S, B, T, D) * (torch.rand(S, B, T, 1, device="cuda") > 0.6) for B in Bs] if guided else None
    want = []
    for k, sess in enumerate(sessions):
        if guided:
            want.append(rg.sampler.ddim_guided_sample_loop(sess, x0[k].clone(), inverted[k], GI, 0.1, noise[k], in_seq=in_seq[k]))
        else:
            want.append(rg.sampler.ddim_sample_loop(sess, x0[k].clone(), in_seq=in_seq[k], inseq_noise=noise[k]))
    xs = [x.clone() for x in x0]
    assert rg.sampler.many_ok(sessions, xs)
    have = rg.sampler.sample_loop_many(sessions, xs, in_seq, noise, inverted, GI if guided else None, 0.1)
    torch.cuda.synchronize()
    for k in range(len(Bs)):
        assert torch.isfinite(want[k]).all() and not torch.equal(want[k], x0[k])
        assert have[k] is xs[k] and torch.equal(have[k], want[k]), ("session %d" % k, (have[k] - want[k]).abs().max().item())
    assert [s.sq.glue_ctr.tolist() for s in sessions] == [[4 * S] * B for B in Bs]      # both loops ran with the tail on
    # where the sessions cannot share launches the loops run one by one: same bits
    duo = rg.denoiser.DenoiserSession(W, 1, engine="seq", seq_duo=True)
    assert not rg.sampler.many_ok([sessions[0], duo], [xs[0], xs[1]])
