"""Host logic of the sampler loops and of forward()'s noise draws, checked without a GPU against word-for-word copies of what
they replaced: the five loop functions of sampler.py with `_glue_sampling` / `_step` (three hand-written rg_glue_args fills, two
unfused steps), and the block of forward() that made every random draw of a batch.  The loops run on stand-in tensors (a
pointer and a shape) and a session that records every launch it is asked for; a loop's trace -- every h.call with its
arguments, every forward with step, step_b, split and the BYTES of its glue struct, every cfg_* update -- must be
the same list, event by event."""
import ctypes
import itertools
import types

import pytest
import torch

S, T, D = 50, 43, 512
GI = tuple((3 * j + 1) % 7 for j in range(S))        # guidance iterations that differ from step to step
LR = 0.1


class _T:
    """Stand-in for a contiguous fp32 device tensor: a pointer and a shape; rows are indexed and sliced by pointer arithmetic."""
    is_cuda, dtype = True, torch.float32

    def __init__(self, shape, ptr, log=None):
        self.shape, self.ptr, self.log = tuple(shape), ptr, log

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self.ptr

    def __getitem__(self, k):
        row = 4
        for n in self.shape[1:]:
            row *= n
        if isinstance(k, slice):
            start, stop, step = k.indices(self.shape[0])
            assert step == 1
            return _T((max(stop - start, 0),) + self.shape[1:], self.ptr + start * row, self.log)
        assert 0 <= k < self.shape[0]
        return _T(self.shape[1:], self.ptr + k * row, self.log)

    def copy_(self, other):
        self.log.append(("copy_", _plain(self), _plain(other)))
        return self


def _plain(v):
    """A recorded argument as a value that compares by content."""
    if isinstance(v, _T):
        return ("tensor", v.ptr, v.shape)
    if isinstance(v, ctypes.Structure):
        return bytes(v)
    if hasattr(v, "_obj"):              # ctypes.byref(struct)
        return bytes(v._obj)
    return v


class _Session:
    """What the loops use of a DenoiserSession; every launch goes into self.log."""

    def __init__(self, rg, B, seq_engine):
        self.log, self.B, self._next = [], B, 1 << 20
        cfg = rg.synth.default_model_cfg(num_layers=1)
        self.w = types.SimpleNamespace(schedule=rg.schedule.Schedule(), T=T, D=D, cfg=cfg, js=self.tensor(4, D))
        self.head = self.tensor(2 * B * T, D)
        self.sq = object() if seq_engine else None
        self.h = types.SimpleNamespace(recorder=None, call=lambda name, *a: self.log.append((name,) + tuple(_plain(v) for v in a)))
        assert self.w.schedule.num_timesteps == S

    def tensor(self, *shape):
        t = _T(shape, self._next, self.log)
        self._next += 4 * int(torch.Size(shape).numel()) + 256
        return t

    def forward(self, x, step, step_b=None, split=None, glue=None):
        self.log.append(("forward", _plain(x), step, step_b, split, None if glue is None else bytes(glue)))

    def _rec(name):
        return lambda self, *a, **k: self.log.append((name,) + tuple(_plain(v) for v in a) + tuple((n, _plain(v)) for n, v in sorted(k.items())))

    cfg_ddim, cfg_ddim_rows, cfg_ddpm = _rec("cfg_ddim"), _rec("cfg_ddim_rows"), _rec("cfg_ddpm")


# ---------------------------------------------------------------------------------------------------------------------------
# The loops as they were before they shared one step builder, word for word (`GlueArgs`, `capi`, `_p` and `_tail_ok`, which
# did not change, are the product's: the `ref` fixture binds them).


def _glue_sampling(sess, x, i, nxt, noise_nxt, g_next, lr):
    """rg_glue_args of a sampling step at respaced index i over ALL clips of the session (its group a): this step's CFG + DDIM
    update of x, then the NEXT step's guidance update (g_next iterations) and in-sequence replacement on the rows nxt marks."""
    sch, w, B, T = sess.w.schedule, sess.w, sess.B, sess.w.T
    a = GlueArgs()
    a.out_c_a, a.out_u_a, a.x_a, a.js = _p(sess.head), _p(sess.head[B * T:]), _p(x), _p(w.js)
    a.n_a, a.n_b, a.T, a.D = B, 0, T, w.D
    a.wc_a, a.wu_a = sch.cfg_weights(w.cfg["scale_func_cfg"], i)
    a.c_recip_a, a.c_recipm1_a, a.ca_a, a.cb_a = float(sch.c_recip[i]), float(sch.c_recipm1[i]), float(sch.c_prev_a[i]), float(sch.c_prev_b[i])
    a.in_seq_next, a.noise_next = _p(nxt), (None if nxt is None else _p(noise_nxt))
    a.g_iter_next, a.lr = (int(g_next) if nxt is not None else 0), float(lr)
    if i > 0:
        a.s_ab_next, a.s_1mab_next = float(sch.s_ab[i - 1]), float(sch.s_1mab[i - 1])
    return a


def _step(sess, x, i, in_seq=None, noise=None):
    """One ddim_sample call at respaced index i, in place on x [B,T,D]."""
    sch, w, h = sess.w.schedule, sess.w, sess.h
    if in_seq is not None:
        h.call("inseq_replace", x, in_seq, noise, sess.B * w.T, w.D, float(sch.s_ab[i]), float(sch.s_1mab[i]))
    sess.forward(x, i)
    sess.cfg_ddim(x, x, i, sch.c_prev_a[i], sch.c_prev_b[i])


def ddim_sample_loop(sess, x, in_seq=None, inseq_noise=None):
    """x: start noise [B,T,D] (updated in place and returned).  in_seq [B,T,D] or None;
    inseq_noise [S,B,T,D] = the randn_like(in_seq) draws, indexed by step."""
    sch, w = sess.w.schedule, sess.w
    S = sch.num_timesteps
    if _tail_ok(sess, x):        # one launch per step: the first step's insertion in front, every later one in the tail before it
        if in_seq is not None:
            sess.h.call("inseq_replace", x, in_seq, inseq_noise[S - 1], sess.B * w.T, w.D, float(sch.s_ab[S - 1]), float(sch.s_1mab[S - 1]))
        for i in range(S - 1, -1, -1):
            nxt = in_seq if i > 0 else None
            sess.forward(x, i, glue=_glue_sampling(sess, x, i, nxt, None if nxt is None else inseq_noise[i - 1], 0, 0.0))
        return x
    for i in range(S - 1, -1, -1):
        _step(sess, x, i, in_seq, None if in_seq is None else inseq_noise[i])
    return x


def p_sample_loop(sess, x, noise):
    """Ancestral sampling (gaussian_diffusion.py:805-905 `p_sample_loop`, fixed_large variance): x = start noise
    [B,T,D] (updated in place and returned), noise [S,B,T,D] = the randn_like(x) draw of every step."""
    S = sess.w.schedule.num_timesteps
    for i in range(S - 1, -1, -1):
        sess.forward(x, i)
        sess.cfg_ddpm(x, x, i, noise[i])
    return x


def ddim_reverse_sample_loop(sess, x, out):
    """DDIM inversion of x [B,T,D] (clean -> noise); out [S,B,T,D] receives every level
    (out[k] = latent at alphas_cumprod_next[k]), x is updated in place to out[S-1]."""
    sch, w = sess.w.schedule, sess.w
    if _tail_ok(sess, x) and out.is_contiguous() and out.dtype == torch.float32:
        B, T = sess.B, w.T           # one launch per step: x advances in place, the forward's tail also writes the level kept
        for i in range(sch.num_timesteps):
            a = GlueArgs()
            a.out_c_b, a.out_u_b, a.x_b, a.x_b_copy, a.js = _p(sess.head), _p(sess.head[B * T:]), _p(x), _p(out[i]), _p(w.js)
            a.n_a, a.n_b, a.T, a.D = 0, B, T, w.D
            a.wc_b, a.wu_b = sch.cfg_weights(w.cfg["scale_func_cfg"], i)
            a.c_recip_b, a.c_recipm1_b, a.ca_b, a.cb_b = float(sch.c_recip[i]), float(sch.c_recipm1[i]), float(sch.c_next_a[i]), float(sch.c_next_b[i])
            sess.forward(x, i, glue=a)
        return out
    cur = x
    for i in range(sch.num_timesteps):
        sess.forward(cur, i)
        sess.cfg_ddim(cur, out[i], i, sch.c_next_a[i], sch.c_next_b[i])   # the update writes level i in place of a copy
        cur = out[i]
    x.copy_(cur)
    return out


def ddim_guided_sample_loop(sess, x, inverted, guidance_iters, guidance_lr, inseq_noise, in_seq=None):
    """Insertion-guided sampling.  inverted [S,B,T,D] (zero rows = not guided); on every step but
    the first the reference sets in_seq = inverted[i], runs g_iter gradient steps on
    mse(x*mask, in_seq) and then ddim_sample re-inserts q_sample(in_seq) on the masked rows."""
    sch, w, h = sess.w.schedule, sess.w, sess.h
    S = sch.num_timesteps
    capi.require(len(guidance_iters) == S == inverted.shape[0],
            "unsupported argument: requires len(guidance_iters) == S == inverted.shape[0]")
    if _tail_ok(sess, x):        # one launch per step (as ddim_sample_loop; the next step's guidance update rides along)
        if in_seq is not None:
            h.call("inseq_replace", x, in_seq, inseq_noise[S - 1], sess.B * w.T, w.D, float(sch.s_ab[S - 1]), float(sch.s_1mab[S - 1]))
        for i in range(S - 1, -1, -1):
            nxt = inverted[i - 1] if i > 0 else None
            sess.forward(x, i, glue=_glue_sampling(sess, x, i, nxt, None if nxt is None else inseq_noise[i - 1],
                                                   guidance_iters[i - 1] if i > 0 else 0, guidance_lr))
        return x
    for i in range(S - 1, -1, -1):
        if i != S - 1:
            in_seq = inverted[i]
            h.call("guidance_update", x, in_seq, sess.B * w.T, w.D, int(guidance_iters[i]), float(guidance_lr))
        _step(sess, x, i, in_seq, None if in_seq is None else inseq_noise[i])
    return x


def cobatched_loop(sess, x_all, n_a, out_b, inverted_a=None, guidance_iters=None, guidance_lr=0.1, inseq_noise_a=None,
                   in_seq_a=None, fused_glue=True, tail_glue=True):
    """Two loops advancing in the same launches, one denoiser forward per step for both:
      clips [0, n_a) of the session: the (insertion-guided) DDIM sampling loop of one batch, exactly
        ddim_guided_sample_loop / ddim_sample_loop (inverted_a None) on x_all[:n_a], in place;
      clips [n_a, B): the DDIM inversion of the NEXT batch's exemplars, exactly ddim_reverse_sample_loop on x_all[n_a:]:
        out_b [S, B - n_a, T, D] receives every level.
    Step k runs the sampling at respaced index S-1-k and the inversion at index k.  Rows of a batch never mix in any
    kernel, so each group gets what its own loop would give; the point is the launch count and size: a forward over
    M = 2 (8 + 24) 43 rows costs ~1.1x the forward over the 24 exemplars alone (NOTEBOOK 6b; with the seq engine: one workgroup per sequence, the launch time does not depend on the count up to 256)."""
    sch, w, h = sess.w.schedule, sess.w, sess.h
    S, B, T, D = sch.num_timesteps, sess.B, w.T, w.D
    n_b = B - n_a
    xa, xb = x_all[:n_a], x_all[n_a:]
    in_seq = in_seq_a
    if fused_glue and h.recorder is None:
        # what lies between two forwards as ONE launch (rg_cobatch_glue: this step's two updates + the next step's guidance and
        # insertion on the sampling rows) instead of four; the first step's insertion in front of the loop as before
        if in_seq is not None:
            h.call("inseq_replace", xa, in_seq, inseq_noise_a[S - 1], n_a * T, D, float(sch.s_ab[S - 1]), float(sch.s_1mab[S - 1]))
        head = sess.head

        def p(t):
            if t is None:
                return None
            if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
                raise capi.RgError("rg_cobatch_glue: contiguous fp32 device tensors expected")
            return t.data_ptr()
        cfgw = lambda step: sch.cfg_weights(w.cfg["scale_func_cfg"], step)
        # tail_glue: the forward's own workgroups do that launch's work as they finish (the one that ends a clip's second
        # sequence updates the clip: rg_seq_args.glue_ctr, csrc/rg_tail.h) -- a loop step is ONE launch
        tail = bool(tail_glue) and _tail_ok(sess, x_all) and 0 < n_a < B
        for k in range(S):
            i = S - 1 - k
            if not tail:
                sess.forward(x_all, i, step_b=k, split=n_a)
            a = GlueArgs()
            a.out_c_a, a.out_u_a, a.x_a = p(head), p(head[B * T:]), p(xa)
            a.out_c_b, a.out_u_b, a.x_b, a.x_b_copy = p(head[n_a * T:]), p(head[(B + n_a) * T:]), p(xb), p(out_b[k])
            nxt = None
            if i > 0:
                nxt = inverted_a[i - 1] if inverted_a is not None else in_seq_a
            a.in_seq_next, a.noise_next = p(nxt), (None if nxt is None else p(inseq_noise_a[i - 1]))
            a.js = p(w.js)
            a.n_a, a.n_b, a.T, a.D = n_a, n_b, T, D
            a.g_iter_next = int(guidance_iters[i - 1]) if (nxt is not None and inverted_a is not None) else 0
            a.wc_a, a.wu_a = cfgw(i)
            a.c_recip_a, a.c_recipm1_a, a.ca_a, a.cb_a = float(sch.c_recip[i]), float(sch.c_recipm1[i]), float(sch.c_prev_a[i]), float(sch.c_prev_b[i])
            a.wc_b, a.wu_b = cfgw(k)
            a.c_recip_b, a.c_recipm1_b, a.ca_b, a.cb_b = float(sch.c_recip[k]), float(sch.c_recipm1[k]), float(sch.c_next_a[k]), float(sch.c_next_b[k])
            a.lr = float(guidance_lr)
            if i > 0:
                a.s_ab_next, a.s_1mab_next = float(sch.s_ab[i - 1]), float(sch.s_1mab[i - 1])
            if tail:
                sess.forward(x_all, i, step_b=k, split=n_a, glue=a)
                continue
            h.call("cobatch_glue", ctypes.byref(a))
        return x_all, out_b
    for k in range(S):
        i = S - 1 - k
        if inverted_a is not None and i != S - 1:
            in_seq = inverted_a[i]
            h.call("guidance_update", xa, in_seq, n_a * T, D, int(guidance_iters[i]), float(guidance_lr))
        if in_seq is not None:
            h.call("inseq_replace", xa, in_seq, inseq_noise_a[i], n_a * T, D, float(sch.s_ab[i]), float(sch.s_1mab[i]))
        sess.forward(x_all, i, step_b=k, split=n_a)
        sess.cfg_ddim_rows(0, n_a, xa, xa, i, sch.c_prev_a[i], sch.c_prev_b[i])
        sess.cfg_ddim_rows(n_a, n_b, xb, xb, k, sch.c_next_a[k], sch.c_next_b[k], x_out2=out_b[k])
    return x_all, out_b


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref(rg):
    globals().update(capi=rg.capi, GlueArgs=rg.sampler.GlueArgs, _p=rg.sampler._p, _tail_ok=rg.sampler._tail_ok)
    return types.SimpleNamespace(**{n: globals()[n] for n in (
        "ddim_sample_loop", "ddim_guided_sample_loop", "ddim_reverse_sample_loop", "p_sample_loop", "cobatched_loop")})


def _cases(B, n_a):
    """(name, run(loops, sess)) of every loop call that is traced, for a session of B clips whose first n_a are sampled."""
    out = []
    for with_in_seq in (False, True):
        out.append(("sample in_seq=%d" % with_in_seq, lambda m, s, f=with_in_seq: m.ddim_sample_loop(
            s, s.tensor(B, T, D), in_seq=s.tensor(B, T, D) if f else None, inseq_noise=s.tensor(S, B, T, D) if f else None)))
        out.append(("guided in_seq=%d" % with_in_seq, lambda m, s, f=with_in_seq: m.ddim_guided_sample_loop(
            s, s.tensor(B, T, D), s.tensor(S, B, T, D), GI, LR, s.tensor(S, B, T, D), in_seq=s.tensor(B, T, D) if f else None)))
    out.append(("reverse", lambda m, s: m.ddim_reverse_sample_loop(s, s.tensor(B, T, D), s.tensor(S, B, T, D))))
    out.append(("ddpm", lambda m, s: m.p_sample_loop(s, s.tensor(B, T, D), s.tensor(S, B, T, D))))
    for guided, fused, tail in itertools.product((True, False), (True, False), (True, False)):
        def co(m, s, guided=guided, fused=fused, tail=tail):
            x_all = s.tensor(B, T, D)
            kw = dict(inverted_a=s.tensor(S, n_a, T, D), guidance_iters=GI) if guided else dict(in_seq_a=s.tensor(n_a, T, D))
            m.cobatched_loop(s, x_all, n_a, s.tensor(S, B - n_a, T, D), guidance_lr=LR, inseq_noise_a=s.tensor(S, n_a, T, D),
                             fused_glue=fused, tail_glue=tail, **kw)
        out.append(("cobatched guided=%d fused=%d tail=%d" % (guided, fused, tail), co))
    return out


def test_every_loop_queues_what_it_queued_before_with_the_same_glue_bytes(rg, ref):
    """84 traces: ddim_sample_loop and ddim_guided_sample_loop with and without in_seq, ddim_reverse_sample_loop, p_sample_loop,
    cobatched_loop guided and unguided with in_seq_a under the four fused_glue x tail_glue settings; each with the tail paths
    available (a sequence engine) and not; sessions of (B, n_a) = (3, 1), (2, 2), (2, 0).  The copy above and the product
    must record the same events.  So that empty traces cannot pass, the count of forwards that carry a glue is checked
    against what the paths imply: with a sequence engine the two sampling loops (x2 for in_seq) and the inversion take the tail
    path in every session (5 loops x 50 steps x 3 sessions), the co-batched loop only with fused_glue, tail_glue and
    0 < n_a < B, i.e. (3, 1) guided and unguided (2 x 50): 850."""
    traces = events = glued = 0
    for (B, n_a), seq_engine in itertools.product(((3, 1), (2, 2), (2, 0)), (True, False)):
        for name, run in _cases(B, n_a):
            logs = []
            for loops in (ref, rg.sampler):
                sess = _Session(rg, B, seq_engine)
                run(loops, sess)
                logs.append(sess.log)
            where = "%s B=%d n_a=%d seq_engine=%d" % (name, B, n_a, seq_engine)
            assert len(logs[0]) == len(logs[1]) >= S, where      # (at least the forward of every step)
            for n, (a, b) in enumerate(zip(*logs)):
                assert a == b, "%s: event %d" % (where, n)
            traces, events = traces + 1, events + len(logs[1])
            glued += sum(1 for e in logs[1] if e[0] == "forward" and e[5] is not None)
    print("traces %d events %d forwards with a glue %d" % (traces, events, glued))
    assert traces == 84 and events >= 11288 and glued == 850


# ---------------------------------------------------------------------------------------------------------------------------
def _draws_before(tape, dev, B, T, D, S, use_inversion, use_insertion_guidance, visualize_inversion, inference_type,
                  use_prev_latent, prev_latent, use_outpaint, retrieval_motion_latents, retrieval_dict, _TorchNoise):
    """The block of forward() that drew a batch's noise before pipeline.draw_batch_noise, word for word (its `self.inference_type`
    is the argument), with what it read from forward()'s locals as arguments and what it left there returned."""
    # ---- every random draw happens here, for the whole batch, in the reference's order
    start_noise, invl = None, None
    if use_inversion:
        start_noise = tape.draw((B, T, D)).to(dev).contiguous()
        if use_insertion_guidance:
            invl = torch.zeros(S, B, T, D, device=dev)
        x = start_noise
    else:
        x = tape.draw((B, T, D)).to(dev).contiguous()
    if use_inversion and visualize_inversion and not isinstance(tape, _TorchNoise):
        # the reconstruction check of every exemplar (diffusion_architecture.py:366-379) is a 50-step DDIM loop that
        # draws randn_like(x) per step (sigma = 0: never used): keep an explicit tape aligned
        for b in range(B):
            for _ in retrieval_dict["retr_uncropped_latents"][b]:
                for _ in range(S):
                    tape.draw((1, T, D))
    in_seq = None
    if use_prev_latent and prev_latent is not None:
        in_seq = prev_latent
    elif use_outpaint:
        in_seq = retrieval_motion_latents
    ddpm = inference_type == "ddpm"
    ddpm_noise = None
    if ddpm:
        # diffusion_architecture.py:424-432: p_sample_loop with a FRESH randn start (the inversion / in_seq results
        # above are computed and ignored by this branch, as in the reference); one randn_like(x) per step
        if use_inversion:   # start_noise was drawn (and spliced) for nothing; p_sample_loop draws its own start
            x = tape.draw((B, T, D)).to(dev).contiguous()
        if isinstance(tape, _TorchNoise):
            ddpm_noise = tape.draw((S, B, T, D))
        else:
            ddpm_noise = torch.empty(S, B, T, D, device=dev)
            for i in range(S - 1, -1, -1):
                ddpm_noise[i].copy_(tape.draw((B, T, D)).to(dev))
        in_seq = None
    need_noise = (in_seq is not None or use_insertion_guidance) and not ddpm
    inseq_noise = None
    if need_noise:
        # the reference draws randn_like(in_seq) then randn_like(x) on every step (the latter is
        # multiplied by sigma = 0); keep the tape aligned
        first = S - 1
        cur_has = in_seq is not None
        if isinstance(tape, _TorchNoise):
            # generator noise: which draw lands on which step is immaterial -> one launch for all steps
            inseq_noise = tape.draw((S, B, T, D))
        else:
            inseq_noise = torch.empty(S, B, T, D, device=dev)
            for i in range(S - 1, -1, -1):
                has = cur_has if i == first or not use_insertion_guidance else True
                if has:
                    inseq_noise[i].copy_(tape.draw((B, T, D)).to(dev))
                tape.draw((B, T, D))
    elif not isinstance(tape, _TorchNoise) and not ddpm:
        for _ in range(S):
            tape.draw((B, T, D))
    return x, start_noise, invl, inseq_noise, ddpm_noise, in_seq


class _CountingTape:
    """A noise tape that is not order-free: the n-th draw is a tensor full of n; the shapes are logged."""

    def __init__(self):
        self.shapes = []

    def draw(self, shape, device=None):
        self.shapes.append(tuple(shape))
        return torch.full(shape, float(len(self.shapes)))


def test_a_batchs_noise_is_drawn_in_the_order_and_lands_where_it_did(rg, monkeypatch):
    """pipeline.draw_batch_noise against the block it replaced, for every combination of use_inversion, insertion guidance
    (only with inversion), an in_seq present, ddpm and visualize_inversion, at B = 3 clips with 0, 2 and 1 exemplars,
    T = 15, D = 8, S = 50 -- with a tape that numbers its draws (same shapes in the same order, every tensor equal: each
    draw landed on the same step) and with the generator tape (same tensors, generator left in the same state).
    (A guided batch without in_seq never writes, and never reads, the first step's row of inseq_noise: torch.empty hands out
    zeros here, so that the row compares.)"""
    P = rg.pipeline
    monkeypatch.setattr(torch, "empty", torch.zeros)
    B, T_, D_, n_ex = 3, 15, 8, (0, 2, 1)
    rd = dict(retr_uncropped_latents=[{q: None for q in range(n)} for n in n_ex])
    prev = torch.ones(B, T_, D_)
    same = lambda a, b: (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))
    runs = 0
    for inv, guid, has, ddpm, vis in itertools.product((False, True), repeat=5):
        if guid and not inv:
            continue
        for kind in ("counting", "generator"):
            if kind == "counting":
                tapes = [_CountingTape(), _CountingTape()]
            else:
                tapes = [P._TorchNoise("cpu", torch.Generator().manual_seed(1234)) for _ in range(2)]
            before = _draws_before(tapes[0], "cpu", B, T_, D_, S, inv, guid, vis, "ddpm" if ddpm else "ddim",
                                   has, prev if has else None, False, None, rd, P._TorchNoise)
            after = P.draw_batch_noise(tapes[1], "cpu", B, T_, D_, S, inv, guid, vis, ddpm, has, n_ex)
            where = (inv, guid, has, ddpm, vis, kind)
            assert len(after) == 5 and all(same(a, b) for a, b in zip(before, after)), where
            assert (before[5] is not None) == (has and not ddpm), where      # (in_seq itself stays with forward())
            if kind == "counting":
                assert tapes[0].shapes == tapes[1].shapes and tapes[0].shapes, where
            else:
                assert torch.equal(tapes[0].generator.get_state(), tapes[1].generator.get_state()), where
            runs += 1
    assert runs == 2 * 24
