"""DDIM sampling / inversion / insertion-guided loops on top of DenoiserSession.

Mirrors the reference's samplers for the inference configuration (START_X prediction, eta = 0,
no clipping): mogen/models/utils/gaussian_diffusion.py
  :1042-1135 ddim_sample_loop(_progressive)   -> ddim_sample_loop
  :1137-1230 ddim_reverse_sample_loop          -> ddim_reverse_sample_loop
  :1233-1395 ddim_guided_sample_loop           -> ddim_guided_sample_loop
  :910-1001  ddim_sample (in_seq replacement + DDIM update)
Every step is a fixed sequence of kernel launches with no host read-back (CFG weights and
DDIM coefficients come from 50-entry host tables), so a whole loop can be captured into one
graph (`GraphedLoop`).  Noise is explicit: the caller supplies the tensors the reference would
have drawn from torch's global generator.
"""
import ctypes

import torch

from . import capi

from .seqfwd import GlueArgs, MANY_MAX      # (rg_glue_args: also the tail of rg_seq_args; sessions per grouped launch)

SPLICE_MAX = capi.header_constants()["RG_SPLICE_MAX"]
SpliceTable = capi.struct("rg_splice_table")      # (rg_splice_many)


TAIL_GLUE = True     # the loops below end every forward with the step's update (rg_seq_args.glue_ctr, csrc/rg_tail.h) where they can


def _tail_ok(sess, x):
    """The loop step's update can ride at the end of the forward: sequence-stationary engine, x updated in place."""
    return (TAIL_GLUE and getattr(sess, "tail_glue", True) and getattr(sess, "sq", None) is not None and sess.h.recorder is None and x.is_cuda and x.is_contiguous()
            and x.dtype == torch.float32 and x.shape[0] == sess.B)


def _p(t):
    if t is None:
        return None
    if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
        raise capi.RgError("rg_cobatch_glue: contiguous fp32 device tensors expected")
    return t.data_ptr()


def _glue(sess, lr=0.0, *, i=None, x_a=None, n_a=0, nxt=None, noise_nxt=None, g_next=0, k=None, x_b=None, keep_b=None, n_b=0):
    """rg_glue_args of one loop step: what a forward's tail (or rg_cobatch_glue) does to x.  Clips [0, n_a) of the session are
    the sampling group (given by i, its respaced index): this step's CFG + DDIM update of x_a, then the NEXT step's guidance
    update (g_next iterations at lr) and in-sequence replacement on the rows nxt marks (noise_nxt: its randn draw).  Clips
    [n_a, n_a + n_b) are the inversion group (given by k): its CFG + reverse-DDIM update of x_b, the level also kept in
    keep_b.  A group that is not given leaves its fields zero."""
    sch, w, head, B, T = sess.w.schedule, sess.w, sess.head, sess.B, sess.w.T
    a = GlueArgs()
    a.js, a.n_a, a.n_b, a.T, a.D, a.lr = _p(w.js), n_a, n_b, T, w.D, float(lr)
    if i is not None:
        a.out_c_a, a.out_u_a, a.x_a = _p(head), _p(head[B * T:]), _p(x_a)
        a.wc_a, a.wu_a = sch.cfg_weights(w.cfg["scale_func_cfg"], i)
        a.c_recip_a, a.c_recipm1_a, a.ca_a, a.cb_a = float(sch.c_recip[i]), float(sch.c_recipm1[i]), float(sch.c_prev_a[i]), float(sch.c_prev_b[i])
        a.in_seq_next, a.noise_next = _p(nxt), (None if nxt is None else _p(noise_nxt))
        a.g_iter_next = int(g_next) if nxt is not None else 0
        if i > 0:
            a.s_ab_next, a.s_1mab_next = float(sch.s_ab[i - 1]), float(sch.s_1mab[i - 1])
    if k is not None:
        a.out_c_b, a.out_u_b, a.x_b, a.x_b_copy = _p(head[n_a * T:]), _p(head[(B + n_a) * T:]), _p(x_b), _p(keep_b)
        a.wc_b, a.wu_b = sch.cfg_weights(w.cfg["scale_func_cfg"], k)
        a.c_recip_b, a.c_recipm1_b, a.ca_b, a.cb_b = float(sch.c_recip[k]), float(sch.c_recipm1[k]), float(sch.c_next_a[k]), float(sch.c_next_b[k])
    return a


def _insert_first(sess, x, n, in_seq, inseq_noise):
    """The first step's in-sequence replacement on x [n,T,D], in front of a loop whose later ones ride in the tail of the step before."""
    if in_seq is not None:
        sch, w, S = sess.w.schedule, sess.w, sess.w.schedule.num_timesteps
        sess.h.call("inseq_replace", x, in_seq, inseq_noise[S - 1], n * w.T, w.D, float(sch.s_ab[S - 1]), float(sch.s_1mab[S - 1]))


def _step(sess, x, i, in_seq=None, noise=None, g_iter=None, lr=0.0, n=None, inv=None):
    """One unfused step at respaced index i, in place on x [n,T,D] (n: default all clips of the session): guidance update
    (g_iter given) -> in_seq replacement -> forward -> CFG + DDIM.  inv = (x_all, k, x_b, keep_b), the row-range form: x is
    clips [0, n) of the session's x_all; the same forward serves inversion step k of the others (x_b, level also into keep_b)."""
    sch, w, h = sess.w.schedule, sess.w, sess.h
    n = sess.B if n is None else n
    if g_iter is not None:
        h.call("guidance_update", x, in_seq, n * w.T, w.D, int(g_iter), float(lr))
    if in_seq is not None:
        h.call("inseq_replace", x, in_seq, noise, n * w.T, w.D, float(sch.s_ab[i]), float(sch.s_1mab[i]))
    if inv is None:
        sess.forward(x, i)
        sess.cfg_ddim(x, x, i, sch.c_prev_a[i], sch.c_prev_b[i])
        return
    x_all, k, x_b, keep_b = inv
    sess.forward(x_all, i, step_b=k, split=n)
    sess.cfg_ddim_rows(0, n, x, x, i, sch.c_prev_a[i], sch.c_prev_b[i])
    sess.cfg_ddim_rows(n, sess.B - n, x_b, x_b, k, sch.c_next_a[k], sch.c_next_b[k], x_out2=keep_b)


def _sample_loop(sess, x, in_seq, inseq_noise, inverted=None, guidance_iters=None, lr=0.0):
    """ddim_sample_loop (inverted None) / ddim_guided_sample_loop: they differ in the in_seq of every step after the first."""
    S = sess.w.schedule.num_timesteps
    if _tail_ok(sess, x):        # one launch per step: the first step's insertion in front, every later one (and its guidance update) in the tail before it
        _insert_first(sess, x, sess.B, in_seq, inseq_noise)
        for i in range(S - 1, -1, -1):
            nxt = None if i == 0 else (inverted[i - 1] if inverted is not None else in_seq)      # in_seq of the step after this one
            sess.forward(x, i, glue=_glue(sess, lr, i=i, x_a=x, n_a=sess.B, nxt=nxt, noise_nxt=None if nxt is None else inseq_noise[i - 1],
                                          g_next=guidance_iters[i - 1] if inverted is not None and i > 0 else 0))
        return x
    for i in range(S - 1, -1, -1):
        g_iter = None
        if inverted is not None and i != S - 1:
            in_seq, g_iter = inverted[i], guidance_iters[i]
        _step(sess, x, i, in_seq, None if in_seq is None else inseq_noise[i], g_iter, lr)
    return x


def many_ok(sessions, xs):
    """The loops of these sessions can advance in grouped launches (sample_loop_many): the tail holds for each, every session
    is in the one-workgroup-per-sequence form, and all belong to one model."""
    return (1 < len(sessions) <= MANY_MAX and all(_tail_ok(s, x) and s.sq.groupable() for s, x in zip(sessions, xs))
            and all(s.w is sessions[0].w for s in sessions) and len({id(s) for s in sessions}) == len(sessions))


def sample_loop_many(sessions, xs, in_seqs, inseq_noises, inverteds=None, guidance_iters=None, lr=0.0):
    """_sample_loop for several sessions at once -- ddim_sample_loop (inverteds None) or ddim_guided_sample_loop of session k on
    xs[k] with in_seqs[k], inseq_noises[k], inverteds[k] -- as ONE launch per step for all of them (rg_seq_forward_many):
    independent chains that are ready together (a pipeline's pending batches when it drains) advance in the time of one.
    Same bits as the loops one by one, which is also what runs where many_ok does not hold."""
    n = len(sessions)
    inverteds = [None] * n if inverteds is None else inverteds
    capi.require(all(v is None or len(guidance_iters) == sessions[0].w.schedule.num_timesteps == v.shape[0] for v in inverteds),
                 "unsupported argument: requires len(guidance_iters) == S == inverted.shape[0]")
    if not many_ok(sessions, xs):
        for k in range(n):
            _sample_loop(sessions[k], xs[k], in_seqs[k], inseq_noises[k], inverteds[k], guidance_iters, lr)
        return xs
    S = sessions[0].w.schedule.num_timesteps
    for k, sess in enumerate(sessions):
        _insert_first(sess, xs[k], sess.B, in_seqs[k], inseq_noises[k])
    for i in range(S - 1, -1, -1):
        calls = []
        for k, sess in enumerate(sessions):
            nxt = None if i == 0 else (inverteds[k][i - 1] if inverteds[k] is not None else in_seqs[k])
            calls.append(dict(x=xs[k], step=i, glue=_glue(
                sess, lr, i=i, x_a=xs[k], n_a=sess.B, nxt=nxt, noise_nxt=None if nxt is None else inseq_noises[k][i - 1],
                g_next=guidance_iters[i - 1] if inverteds[k] is not None and i > 0 else 0)))
        type(sessions[0]).forward_many(sessions, calls)
    return xs


def ddim_sample_loop(sess, x, in_seq=None, inseq_noise=None):
    """x: start noise [B,T,D] (updated in place and returned).  in_seq [B,T,D] or None;
    inseq_noise [S,B,T,D] = the randn_like(in_seq) draws, indexed by step."""
    return _sample_loop(sess, x, in_seq, inseq_noise)


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
    sch = sess.w.schedule
    if _tail_ok(sess, x) and out.is_contiguous() and out.dtype == torch.float32:
        for i in range(sch.num_timesteps):      # one launch per step: x advances in place, the forward's tail also writes the level kept
            sess.forward(x, i, glue=_glue(sess, k=i, x_b=x, keep_b=out[i], n_b=sess.B))
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
    capi.require(len(guidance_iters) == sess.w.schedule.num_timesteps == inverted.shape[0],
            "unsupported argument: requires len(guidance_iters) == S == inverted.shape[0]")
    return _sample_loop(sess, x, in_seq, inseq_noise, inverted, guidance_iters, guidance_lr)


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
    h, S, B = sess.h, sess.w.schedule.num_timesteps, sess.B
    n_b = B - n_a
    xa, xb = x_all[:n_a], x_all[n_a:]
    in_seq = in_seq_a
    if fused_glue and h.recorder is None:
        # what lies between two forwards as ONE launch (rg_cobatch_glue: this step's two updates + the next step's guidance and
        # insertion on the sampling rows) instead of four; the first step's insertion in front of the loop as before
        _insert_first(sess, xa, n_a, in_seq, inseq_noise_a)
        # tail_glue: the forward's own workgroups do that launch's work as they finish (the one that ends a clip's second
        # sequence updates the clip: rg_seq_args.glue_ctr, csrc/rg_tail.h) -- a loop step is ONE launch
        tail = bool(tail_glue) and _tail_ok(sess, x_all) and 0 < n_a < B
        for k in range(S):
            i = S - 1 - k
            if not tail:
                sess.forward(x_all, i, step_b=k, split=n_a)
            nxt = None if i == 0 else (inverted_a[i - 1] if inverted_a is not None else in_seq_a)
            a = _glue(sess, guidance_lr, i=i, x_a=xa, n_a=n_a, nxt=nxt, noise_nxt=None if nxt is None else inseq_noise_a[i - 1],
                      g_next=guidance_iters[i - 1] if inverted_a is not None and i > 0 else 0, k=k, x_b=xb, keep_b=out_b[k], n_b=n_b)
            if tail:
                sess.forward(x_all, i, step_b=k, split=n_a, glue=a)
            else:
                h.call("cobatch_glue", ctypes.byref(a))
        return x_all, out_b
    for k in range(S):
        i, g_iter = S - 1 - k, None
        if inverted_a is not None and i != S - 1:
            in_seq, g_iter = inverted_a[i], guidance_iters[i]
        _step(sess, xa, i, in_seq, None if in_seq is None else inseq_noise_a[i], g_iter, guidance_lr, n_a, (x_all, k, xb, out_b[k]))
    return x_all, out_b


def cobatched_many_ok(sessions, x_alls, n_as):
    """The co-batched loops of these sessions can advance in grouped launches (cobatched_loop_many): the tail holds for each
    with both groups present, every session is in the twin form, and all belong to one model."""
    return (1 < len(sessions) <= MANY_MAX and all(_tail_ok(s, x) and s.sq.groupable_twin() and 0 < n < s.B for s, x, n in zip(sessions, x_alls, n_as))
            and all(s.w is sessions[0].w for s in sessions) and len({id(s) for s in sessions}) == len(sessions))


def cobatched_loop_many(sessions, x_alls, n_as, out_bs, inverted_as=None, guidance_iters=None, guidance_lr=0.1, inseq_noise_as=None,
                        in_seq_as=None, tail_glue=True):
    """cobatched_loop for several sessions at once -- session j: clips [0, n_as[j]) of x_alls[j] sample (inverted_as[j],
    inseq_noise_as[j], in_seq_as[j]), the rest invert into out_bs[j] -- as ONE launch per step for all of them
    (rg_seq2_forward_many): the co-batched chains of a pipeline's lanes, ready together once per rotation, advance in the time
    of one and fill the chip from one stream.  Same bits as the loops one by one, which is also what runs where
    cobatched_many_ok does not hold."""
    n = len(sessions)
    none = [None] * n
    inverted_as = none if inverted_as is None else inverted_as
    inseq_noise_as = none if inseq_noise_as is None else inseq_noise_as
    in_seq_as = none if in_seq_as is None else in_seq_as
    if not (tail_glue and cobatched_many_ok(sessions, x_alls, n_as)):
        for j in range(n):
            cobatched_loop(sessions[j], x_alls[j], n_as[j], out_bs[j], inverted_a=inverted_as[j], guidance_iters=guidance_iters,
                           guidance_lr=guidance_lr, inseq_noise_a=inseq_noise_as[j], in_seq_a=in_seq_as[j], tail_glue=tail_glue)
        return x_alls, out_bs
    S = sessions[0].w.schedule.num_timesteps
    for j, sess in enumerate(sessions):
        _insert_first(sess, x_alls[j][:n_as[j]], n_as[j], in_seq_as[j], inseq_noise_as[j])
    for k in range(S):
        i = S - 1 - k
        calls = []
        for j, sess in enumerate(sessions):
            n_a = n_as[j]
            nxt = None if i == 0 else (inverted_as[j][i - 1] if inverted_as[j] is not None else in_seq_as[j])
            calls.append(dict(x=x_alls[j], step=i, step_b=k, split=n_a, glue=_glue(
                sess, guidance_lr, i=i, x_a=x_alls[j][:n_a], n_a=n_a, nxt=nxt, noise_nxt=None if nxt is None else inseq_noise_as[j][i - 1],
                g_next=guidance_iters[i - 1] if inverted_as[j] is not None and i > 0 else 0, k=k, x_b=x_alls[j][n_a:], keep_b=out_bs[j][k],
                n_b=sess.B - n_a)))
        type(sessions[0]).forward_many(sessions, calls)
    return x_alls, out_bs


class GraphedLoop:
    """Capture fn() (a fixed launch sequence over static buffers) into a HIP graph and replay it.
    torch.cuda.CUDAGraph is used purely as the capture/replay plumbing."""

    def __init__(self, fn, warmup=True):
        if warmup:  # first call outside capture: lazy module loads, allocator warm-up
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                fn()
            torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with capi.capture(self.graph):
            fn()

    def replay(self):
        self.graph.replay()
