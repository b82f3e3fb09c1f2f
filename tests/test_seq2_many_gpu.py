"""GPU: rg_seq2_forward_many (the twin-form forwards of several sessions in ONE launch: workgroup -> (session, clip of the
session), then rg_seq2_twin_kernel's body on that session's arguments) against rg_seq2_forward session by session, and the
co-batched loops built on it (sampler.cobatched_loop_many) against the loops one by one.  A grouped launch must give
rg_seq2_forward's bits, tail included, so every comparison here is torch.equal."""
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


def _session(rg, W, B, seed, empty=False, twin=True):
    """A twin-form session of B clips with its conditions set: motion masks with masked tokens, query masks that mask rows of
    every condition (other rows per condition and clip), optionally a clip without a valid token."""
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
    sess = rg.denoiser.DenoiserSession(W, B, engine="seq", seq_duo=True, seq_twin=twin)
    sess.set_conditions(data["word"], data["audio"], data["speaker_ids"], mm, qm)
    assert sess.sq.groupable_twin() == bool(twin) and not sess.sq.groupable()
    return sess


@pytest.mark.parametrize("T", [43, 27])
@pytest.mark.parametrize("Bs,empty", [((1,), False), ((3, 1), False), ((2, 3, 1), False), ((2, 3, 1), True)],
                         ids=["B1", "B3+1", "B2+3+1", "B2+3+1-a-clip-all-masked"])
def test_grouped_twin_forward_is_bit_identical(rg, weights, Bs, T, empty):
    """Head rows of every sequence of every session: one grouped launch == rg_seq2_forward (twin) per session, each session at a
    step of its own (the sessions of more than one clip with two step groups, `split` inside; the others with one); one session
    alone, sessions of odd and unequal sizes, masked query rows of every condition, a clip whose tokens are all masked in the
    MIDDLE session; a second grouped launch gives the same bits."""
    W = weights[T]
    rnd = _rnd(10 * len(Bs) + T)
    sessions = [_session(rg, W, B, 100 + 7 * k + B, empty and k == 1) for k, B in enumerate(Bs)]
    xs = [rnd(B, T, 512) for B in Bs]
    calls = [dict(x=xs[k], step=(49, 7, 23)[k]) for k in range(len(Bs))]
    for k, B in enumerate(Bs):
        if B > 1:
            calls[k].update(step_b=31 + k, split=1 if k else B - 1)
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
def test_grouped_twin_forward_tails(rg, weights, T):
    """With glue_ctr set every session's forward ends with ITS loop step's update, read from the session's place in the
    parameter block: sessions in the co-batched form (both groups, two step groups, the next step's in_seq marks rows, two
    guidance iterations, the level kept), in the sampling form, in the inversion form and without a tail, in one launch; two
    consecutive steps; head rows, x and the kept levels after each against rg_seq2_forward with the tail on, session by
    session.  The twin form leaves the arrival counters alone: a counting-form loop on one of the sessions' clips afterwards
    (the same weights, the one-workgroup-per-sequence form on the same counters' parity) still equals its reference."""
    W = weights[T]
    S = W.schedule.num_timesteps
    Bs, D = (3, 2, 3, 1, 2), 512
    rnd = _rnd(500 + T)
    sessions = [_session(rg, W, B, 300 + k, empty=(k == 2)) for k, B in enumerate(Bs)]
    x0 = [rnd(B, T, D) for B in Bs]
    in_seq = [rnd(B, T, D) * (torch.rand(B, T, 1, device="cuda") > 0.5) for B in Bs]
    noise = [rnd(B, T, D) for B in Bs]
    glue = rg.sampler._glue

    def calls(xs, keeps, i):
        k = S - 1 - i
        return [dict(x=xs[0], step=i, step_b=k, split=1, glue=glue(sessions[0], 0.1, i=i, x_a=xs[0][:1], n_a=1, nxt=in_seq[0][:1], noise_nxt=noise[0][:1],
                                                                  g_next=2, k=k, x_b=xs[0][1:], keep_b=keeps[0], n_b=2)),
                dict(x=xs[1], step=i, glue=glue(sessions[1], 0.1, i=i, x_a=xs[1], n_a=Bs[1], nxt=in_seq[1], noise_nxt=noise[1], g_next=2)),
                dict(x=xs[2], step=k, glue=glue(sessions[2], k=k, x_b=xs[2], keep_b=keeps[1], n_b=Bs[2])),
                dict(x=xs[3], step=i),
                dict(x=xs[4], step=i, step_b=k, split=1, glue=glue(sessions[4], 0.1, i=i, x_a=xs[4][:1], n_a=1, nxt=None, k=k, x_b=xs[4][1:],
                                                                  keep_b=keeps[2], n_b=1))]

    def run(many):
        xs, seen = [x.clone() for x in x0], []
        keeps = [torch.zeros(2, T, D, device="cuda"), torch.zeros(Bs[2], T, D, device="cuda"), torch.zeros(1, T, D, device="cuda")]
        for i in (30, 29):
            cs = calls(xs, keeps, i)
            if many:
                rg.denoiser.DenoiserSession.forward_many(sessions, cs)
            else:
                for s, kw in zip(sessions, cs):
                    s.forward(**kw)
            seen.append([s.head.clone() for s in sessions] + [x.clone() for x in xs] + [k.clone() for k in keeps])
        torch.cuda.synchronize()
        return seen
    ref = run(False)
    got = run(True)
    for step, (g, r) in enumerate(zip(got, ref)):
        for j, (a, b) in enumerate(zip(g, r)):
            assert torch.isfinite(b).all() and torch.equal(a, b), ("step %d" % step, "tensor %d" % j, (a - b).abs().max().item())
    n = len(Bs)
    assert not torch.equal(ref[0][n], x0[0]) and not torch.equal(ref[1][n], ref[0][n])      # x moved, step after step
    assert all(bool((t != 0).any()) for t in ref[1][2 * n:])                                  # every kept level was written
    assert [s.sq.glue_ctr.tolist() for s in sessions] == [[0] * B for B in Bs]              # the twin form counts no arrivals
    # the counting form on session 1's counters, as the grouped launches left them
    sess, B = sessions[1], Bs[1]
    one = rg.denoiser.DenoiserSession(W, B, engine="seq", seq_duo=False)
    one.src_mask.copy_(sess.src_mask)
    one.qmask.copy_(sess.qmask)
    one.sq.afrag.copy_(sess.sq.afrag)
    one.sq.glue_ctr = sess.sq.glue_ctr
    inverted = rnd(S, B, T, D) * (torch.rand(S, B, T, 1, device="cuda") > 0.6)
    nz = rnd(S, B, T, D)
    rg.sampler.TAIL_GLUE = False
    try:
        want = rg.sampler.ddim_guided_sample_loop(one, x0[1].clone(), inverted, GI, 0.1, nz, in_seq=in_seq[1])
    finally:
        rg.sampler.TAIL_GLUE = True
    have = rg.sampler.ddim_guided_sample_loop(one, x0[1].clone(), inverted, GI, 0.1, nz, in_seq=in_seq[1])
    twin = rg.sampler.ddim_guided_sample_loop(sess, x0[1].clone(), inverted, GI, 0.1, nz, in_seq=in_seq[1])
    torch.cuda.synchronize()
    assert torch.isfinite(want).all() and torch.equal(have, want) and torch.equal(twin, want)
    assert sess.sq.glue_ctr.tolist() == [2 * S] * B


def test_grouped_twin_forward_refusals_run_nothing(rg, weights):
    """What the entry point refuses reaches the caller as an error and nothing runs (sentinel-filled heads stay untouched): a
    session that is not in the twin form in the list, `pairs`, sessions of unequal T, too many sessions."""
    W = weights[43]
    a, b, c = _session(rg, W, 1, 1), _session(rg, weights[27], 1, 2), _session(rg, W, 2, 3)
    duo = _session(rg, W, 1, 4, twin=False)
    xa, xb, xc = torch.zeros(1, 43, 512, device="cuda"), torch.zeros(1, 27, 512, device="cuda"), torch.zeros(2, 43, 512, device="cuda")
    every = (a, b, c, duo)
    for s in every:
        s.head.fill_(7.0)
    many = rg.denoiser.DenoiserSession.forward_many
    with pytest.raises(rg.capi.RgError, match="rg_seq2_forward_many: the sessions must agree in L, T and S"):
        many([a, b], [dict(x=xa, step=3), dict(x=xb, step=3)])
    with pytest.raises(rg.capi.RgError, match="one-workgroup-per-sequence"):          # (the host side: the families never mix)
        many([a, duo], [dict(x=xa, step=3), dict(x=xa, step=3)])
    # ... and the entry point itself, underneath the host side's own check
    import ctypes

    def raw(sqs, calls):
        args = [sq._set_args(**kw) for sq, kw in zip(sqs, calls)]
        ptrs = (ctypes.c_void_p * len(args))(*[ctypes.addressof(x) for x in args])
        a.h.call("seq2_forward_many", ctypes.cast(ptrs, ctypes.c_void_p), len(args))
    with pytest.raises(rg.capi.RgError, match="rg_seq2_forward_many: every session must be in the twin form"):
        raw([a.sq, duo.sq], [dict(x=xa, step=3), dict(x=xa, step=3)])
    c.sq.args.pairs = 1
    try:
        with pytest.raises(rg.capi.RgError, match="rg_seq2_forward_many: twin and pairs are two launch forms"):
            raw([a.sq, c.sq], [dict(x=xa, step=3), dict(x=xc, step=3)])
    finally:
        c.sq.args.pairs = 0
    n = rg.seqfwd.MANY_MAX + 1
    with pytest.raises(rg.capi.RgError, match="rg_seq2_forward_many: too many sessions"):
        raw([a.sq] * n, [dict(x=xa, step=3)] * n)
    with pytest.raises(rg.capi.RgError, match="1 to %d sessions" % rg.seqfwd.MANY_MAX):
        many([a] * n, [dict(x=xa, step=3)] * n)
    torch.cuda.synchronize()
    assert all(bool((s.head == 7.0).all()) for s in every)


@pytest.mark.parametrize("Bs,n_as", [((3, 2), (1, 1)), ((2, 4, 3), (1, 1, 2))], ids=["2-sessions", "3-sessions"])
def test_cobatched_loop_many_equals_the_loops_one_by_one(rg, weights, Bs, n_as):
    """cobatched_loop_many over 2 and 3 twin sessions, the full schedule: every session's sampled rows and every inversion level
    == cobatched_loop on that session alone (guided, a first-step in_seq for all but one of the sessions)."""
    T, D = 43, 512
    W = weights[T]
    S = W.schedule.num_timesteps
    rnd = _rnd(900 + len(Bs))
    sessions = [_session(rg, W, B, 600 + k) for k, B in enumerate(Bs)]
    x0 = [rnd(B, T, D) for B in Bs]
    in_seq = [rnd(n, T, D) * (torch.rand(n, T, 1, device="cuda") > 0.5) if k != 1 else None for k, n in enumerate(n_as)]
    noise = [rnd(S, n, T, D) for n in n_as]
    inverted = [rnd(S, n, T, D) * (torch.rand(S, n, T, 1, device="cuda") > 0.6) for n in n_as]
    want = []
    for k, sess in enumerate(sessions):
        out = torch.zeros(S, Bs[k] - n_as[k], T, D, device="cuda")
        x, _ = rg.sampler.cobatched_loop(sess, x0[k].clone(), n_as[k], out, inverted_a=inverted[k], guidance_iters=GI, guidance_lr=0.1,
                                         inseq_noise_a=noise[k], in_seq_a=in_seq[k])
        want.append((x, out))
    xs = [x.clone() for x in x0]
    outs = [torch.zeros(S, B - n, T, D, device="cuda") for B, n in zip(Bs, n_as)]
    assert rg.sampler.cobatched_many_ok(sessions, xs, n_as)
    rg.sampler.cobatched_loop_many(sessions, xs, n_as, outs, inverted_as=inverted, guidance_iters=GI, guidance_lr=0.1,
                                   inseq_noise_as=noise, in_seq_as=in_seq)
    torch.cuda.synchronize()
    for k in range(len(Bs)):
        assert torch.isfinite(want[k][0]).all() and torch.isfinite(want[k][1]).all() and not torch.equal(want[k][0], x0[k])
        assert torch.equal(xs[k], want[k][0]), ("session %d" % k, (xs[k] - want[k][0]).abs().max().item())
        assert torch.equal(outs[k], want[k][1]), ("session %d levels" % k, (outs[k] - want[k][1]).abs().max().item())
    assert [s.sq.glue_ctr.tolist() for s in sessions] == [[0] * B for B in Bs]
    # where the sessions cannot share launches the loops run one by one: same bits
    duo = _session(rg, W, 2, 700, twin=False)
    assert not rg.sampler.cobatched_many_ok([sessions[0], duo], [xs[0], x0[0][:2]], [1, 1])
    xs2, outs2 = [x0[0].clone(), x0[0][:2].clone()], [torch.zeros(S, Bs[0] - 1, T, D, device="cuda"), torch.zeros(S, 1, T, D, device="cuda")]
    rg.sampler.cobatched_loop_many([sessions[0], duo], xs2, [n_as[0], 1], outs2, inverted_as=[inverted[0], inverted[0][:, :1]], guidance_iters=GI,
                                   guidance_lr=0.1, inseq_noise_as=[noise[0], noise[0][:, :1]], in_seq_as=[in_seq[0], None])
    torch.cuda.synchronize()
    if n_as[0] == 1:
        assert torch.equal(xs2[0], want[0][0]) and torch.equal(outs2[0], want[0][1])
