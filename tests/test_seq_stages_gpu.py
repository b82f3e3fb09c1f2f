"""GPU: the fused denoiser forward (rg_seq_forward, csrc/rg_seq.hip) stage by stage against the fp64 references of
tests/kernel_refs.py ("Fused stacks"), through the kernel's diagnostic dumps (rg_seq_args.dump / dump_stage / dump_layer).

Teacher forcing: the reference of a stage starts from the kernel's own dump of the stage before it (exact fp32 values), so no
error accumulates over more than one block and a failure names its stage, layer, sequence kind, token block and wave.  The
references are built from the reference state dict, the model's AdaLN table and the header's formulas -- never from the packed
streams of seqfwd.py -- so a packing mistake fails here.  The cross-attention A matrices are the test's own (random, installed
with SeqForward.set_a): nothing depends on rg_cond_kv.  test_kernel_refs_cpu.py shows on the CPU that the bounds hold for a
correct emulation and that the listed wrong variants exceed them at their stage.

The other launch forms (two sequences per workgroup, its twin form, the pairs forms) must give rg_seq_forward's bits at every
stage, not only at the head."""
import ctypes

import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

L = 2
SENT = -123456.75          # sentinel of the dump buffers (exact in fp32; no stage produces it)
LAYER_STAGES = [(0, 1)] + [(l, s) for l in range(L) for s in kr.SEQ_STAGES]          # every dump of a launch, in forward order


@pytest.fixture(scope="module")
def models(rg):
    """T -> (DenoiserWeights on the device, SeqModel: the fp64 parameters from the same state dict and the model's AdaLN table)."""
    assert torch.cuda.is_available()
    cache = {}

    def get(T):
        if T not in cache:
            cfg = rg.synth.default_model_cfg(num_layers=L)
            cfg["max_seq_len"] = kr.seq_frames(T)          # T = 4 (max_seq_len / frame_chunk_size) + 3: 15, 27, 43 and 47 are all reachable
            sd = kr.off_centre(rg.synth.synth_denoiser_state(0, cfg))
            W = rg.denoiser.DenoiserWeights(sd, cfg, rg.schedule.Schedule(), "cuda")
            assert W.seq_streams is not None and W.T == T
            cache[T] = (W, kr.SeqModel(lambda name: sd[name].float(), W.ss.cpu(), L, T))
        return cache[T]
    return get


def _session(rg, W, c, **form):
    data = rg.synth.synth_batch(c.B, seed=c.B)
    sess = rg.denoiser.DenoiserSession(W, c.B, engine="seq", **form)
    sess.set_conditions(data["word"], data["audio"], data["speaker_ids"], c.mm, {n: c.qm[k] for k, n in enumerate(rg.denoiser.CONDS)})
    sess.sq.set_a(c.A.cuda(), 0, c.B)          # the test's own cross-attention matrices
    return sess


def _dumps(sess, c, x):
    """{(layer, stage): CPU dump buffer [2 B + 1, 48, 512]} of every stage, one launch each (a sentinel row block behind)."""
    out = {}
    for l, stage in LAYER_STAGES:
        buf = torch.full((2 * c.B + 1, 48, kr.DM), SENT, device="cuda")
        sess.sq.run(x, c.step, c.step_b, c.split, dump=buf, dump_stage=stage, dump_layer=l)
        out[l, stage] = buf
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _written(stage, B):
    """Sequences a stage dumps: stages 11-13 exist for the conditional ones only."""
    return B if stage in (11, 12, 13) else 2 * B


@pytest.mark.parametrize("launch", kr.SEQ_LAUNCHES, ids=lambda la: "B%d-T%d-step%d%s" % (la[:3] + ("-and-%d" % la[3] if la[3] is not None else "",)))
def test_seq_forward_every_stage_against_fp64(rg, parity, models, launch):
    """Every element of the rows < T of all sequences at the embedding, at the seven stages of both layers and at the head:
    worst |err| / bound <= 1, one parity line per stage.  The classifier-free part of the stage 11-13 dumps and everything
    behind [2 B][48][512] keep the sentinel; masked query rows of stages 11-13 lie on the 1/16 grid, an element within its bound
    of a rounding tie may sit one grid step away (counted, at most 5 % of the masked elements)."""
    c = kr.seq_launch_case(*launch)
    B, T = c.B, c.T
    W, m = models(T)
    sess = _session(rg, W, c, seq_duo=False)
    x = c.x.cuda()
    head = sess.sq.run(x, c.step, c.step_b, c.split).clone().view(2 * B, T, kr.DM).cpu()
    dumps = _dumps(sess, c, x)
    tag = "seq stages B%d T%d step %d/%d split %d" % (B, T, c.step, c.step_b, c.split)

    def check(name, got, ref):
        r = kr.worst_ratio(got, ref[0], ref[1])
        print("%s %s: worst |err| / bound %.3f" % (tag, name, r))
        if not r <= 1.0:
            print("   " + kr.where_worst(got, ref[0], ref[1], B))
        parity.check("%s %s worst |err| / bound" % (tag, name), r, 1.0)

    for (l, stage), buf in dumps.items():
        n = _written(stage, B)
        assert bool((buf[n:] == SENT).all()), "layer %d stage %d wrote outside its %d sequences" % (l, stage, n)
        assert torch.isfinite(buf[:n]).all()
    X = dumps[0, 1][:2 * B, :T]
    check("embedding", X, kr.seq_stage_ref(1, m, c, 0, {}))
    for l in range(L):
        state = {"in": X}
        for stage in kr.SEQ_STAGES:
            got = dumps[l, stage][:_written(stage, B), :T]
            ref = kr.seq_stage_ref(stage, m, c, l, kr.seq_stage_inputs(stage, c, state))
            if len(ref) == 3:
                msk = (c.qm[stage - 11] == 0)[:, :, None].expand_as(got)
                ties, masked = int(ref[2].sum()), int(msk.sum())
                print("%s layer %d stage %d: %d of %d masked elements within their bound of a rounding tie" % (tag, l, stage, ties, masked))
                assert ties <= 0.05 * masked
                assert torch.equal(got[msk] * 16, torch.round(got[msk] * 16))          # exact multiples of 1/16
            check("layer %d stage %d" % (l, stage), got, ref)
            state[stage] = got
        X = state[4]
    check("head", head, kr.seq_stage_ref(0, m, c, 0, dict(X=X)))


FORMS = dict(duo=dict(seq_duo=True), twin=dict(seq_duo=True, seq_twin=True), pairs_duo=dict(seq_pairs=True, seq_duo=True),
             pairs_one=dict(seq_pairs=True, seq_duo=False))


@pytest.mark.parametrize("T", [27, 43])
def test_other_launch_forms_give_the_same_bits_at_every_stage(rg, models, T):
    """rg_seq2_forward (two sequences of a kind per workgroup), its twin form and the pairs forms of both kernels: every stage
    dump -- rows < T of every sequence the stage writes, and the sentinel everywhere else -- equals rg_seq_forward's bit for bit,
    on a launch with two step groups, B = 3."""
    c = kr.seq_launch_case(3, T, 40, 9, 1)
    B = c.B
    W, _ = models(T)
    x = c.x.cuda()
    ref = _dumps(_session(rg, W, c, seq_duo=False), c, x)
    for name, form in FORMS.items():
        sess = _session(rg, W, c, **form)
        assert sess.sq._entry == ("seq2_forward" if form["seq_duo"] else "seq_forward") and sess.sq.args.pairs == int(bool(form.get("seq_pairs")))
        got = _dumps(sess, c, x)
        for (l, stage), buf in got.items():
            n = _written(stage, B)
            assert bool((buf[n:] == SENT).all()), (name, l, stage, "wrote outside its sequences")
            for s in range(n):
                assert torch.equal(buf[s, :T], ref[l, stage][s, :T]), (name, "layer %d stage %d sequence %d" % (l, stage, s),
                                                                        (buf[s, :T] - ref[l, stage][s, :T]).abs().max().item())


def _profiled(h, variant, launch):
    """(launches, total_ms, total_flops) that rg_profile_end reports under `variant` for the eager launches `launch` makes."""
    n, ms, fl = ctypes.c_int64(-1), ctypes.c_double(-1.0), ctypes.c_double(-1.0)
    torch.cuda.synchronize()
    assert h.lib.rg_profile_begin(h._h) == 0
    try:
        launch()
    finally:
        assert h.lib.rg_profile_end(h._h, variant, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl)) == 0
    return n.value, ms.value, fl.value


def test_every_entry_point_is_profiled_as_one_launch_of_the_models_flops(rg, models):
    """The profiling scope and the FLOP model that the entry points share (csrc/rg_common.h rg_prof_scope,
    csrc/rg_seq_host.h rg_seq_flops): one eager forward between rg_profile_begin and rg_profile_end is ONE launch of variant 3,
    of B ((16 L + 2) u + 5 L a + (10 L + 2) u + 2 L a) FLOPs (u = 2 T 512^2: a unit GEMM, a = 2 T 32 32 16: an attention
    product over the heads; integers in a double: compared exactly) and of some duration -- through rg_seq_forward,
    rg_seq2_forward and its twin kernel alike; an rg_gemm launch is counted under its own variant, not under 3."""
    B, T = 2, 27
    c = kr.seq_launch_case(B, T, 40, None, None)
    W, _ = models(T)
    x = c.x.cuda()
    forms = dict(seq_forward=dict(seq_duo=False), seq2_forward=dict(seq_duo=True), seq2_forward_twin=dict(seq_duo=True, seq_twin=True))
    u, a = 2 * T * 512 * 512, 2 * T * 32 * 32 * 16
    flops = B * ((16 * L + 2) * u + 5 * L * a + (10 * L + 2) * u + 2 * L * a)
    for name, form in forms.items():
        sess = _session(rg, W, c, **form)
        assert sess.sq._entry == name.replace("_twin", "") and sess.sq.args.twin == int(name.endswith("twin"))
        n, ms, fl = _profiled(sess.h, 3, lambda: sess.forward(x, c.step))
        assert (n, fl) == (1, float(flops)) and ms > 0, (name, n, ms, fl, flops)
    h = sess.h
    M, N, K = 64, 128, 64
    A = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    Wp, out = rg.gemm.pack_weight(torch.randn(N, K), "cuda"), torch.empty(M, N, device="cuda")
    gemm = lambda: rg.gemm.gemm(h, M=M, N=N, K=K, W=Wp, A=A, out=out)
    assert _profiled(h, 3, gemm)[0] == 0
    n, ms, fl = _profiled(h, 1, gemm)             # (bf16 A operand: variant 1)
    assert (n, fl) == (1, 2.0 * M * N * K) and ms > 0
