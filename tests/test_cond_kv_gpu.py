"""GPU: rg_cond_kv (csrc/rg_condkv.hip) -- the condition side's projection, token softmax and A = softmax_N(K)^T V of every layer
in one launch -- through the C ABI against the fp64 reference of tests/kernel_refs.py ("Condition side": formulas, bounds, input
families and their derivation; test_kernel_refs_cpu.py shows on the CPU that a correct emulation is inside the bounds and seven
wrong variants are outside).  The shapes are chosen for the kernel's control flow, not for the workload: every wave split
wpc = ceil(N / 64) = 1 .. 8, every clip packing cpw = 8 / wpc, idle waves, partly filled last workgroups, pad rows.  Every element
of A is compared, the outputs sit inside canary buffers the way set_conditions places them in a session's a_pre / afrag, the
bf16 fragments must be the packing of the fp32 matrices bit for bit, and repeated launches must give the same bits.
Then the dispatcher around the kernel: DenoiserSession.set_conditions with one condition beyond 512 tokens, which takes the
grouped GEMMs + rg_kv_reduce for that condition only."""
import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def h(rg):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return rg.capi.get_handle(0)


def _canaries(B, L):
    out = torch.full((L, 3, B + 2, 16, 32, 32), float("nan"))
    frag = torch.full((L, 3, B + 2, 8, 2, 2, 64, 8), 0x7FC1, dtype=torch.int16)
    return out, frag


def _outside_intact(got, before, B):
    """True when `got` equals `before` bit for bit outside [:, 1, 1:1 + B]."""
    view = torch.int32 if got.element_size() == 4 else torch.int16
    a, b = got.contiguous().view(view).clone(), before.contiguous().view(view).clone()
    a[:, 1, 1:1 + B] = 0
    b[:, 1, 1:1 + B] = 0
    return bool(torch.equal(a, b))


def _launch(h, dev, out, frag, B, N, L):
    xhat, w, bias = dev
    h.call("cond_kv", xhat, w, bias, out[0, 1, 1:1 + B], out.stride(0), None if frag is None else frag[0, 1, 1:1 + B],
           0 if frag is None else frag.stride(0), B, N, L)
    torch.cuda.synchronize()


@pytest.mark.parametrize("N,B,L,family", kr.COND_KV_RUNS, ids=["%d-%d-%d-%s" % r for r in kr.COND_KV_RUNS])
def test_cond_kv_vs_fp64(rg, h, parity, N, B, L, family):
    """One (shape, family): placement inside the canaries, every element of A against the fp64 reference, the fragments against
    the packing of the written A, a launch without fragments, and a repeated launch."""
    c = kr.cond_kv_case(N, B, L, family, kr.cond_kv_seed(N, B, L, family))
    dev = (c.xhat.cuda(), c.w.cuda(), c.bias.cuda())
    out0, frag0 = _canaries(B, L)
    out, frag = out0.cuda(), frag0.cuda()
    _launch(h, dev, out, frag, B, N, L)
    oc, fc = out.cpu(), frag.cpu()
    assert _outside_intact(oc, out0, B) and _outside_intact(fc, frag0, B), (N, B, L, family)
    A = oc[:, 1, 1:1 + B].contiguous()
    ref, bound = kr.cond_kv_ref(c)
    ratio = kr.worst_ratio(A, ref, bound)
    wpc, cpw = kr.cond_kv_split(N)
    print("rg_cond_kv N=%d B=%d L=%d %s (wpc %d, cpw %d): A worst |err| / bound %.4f" % (N, B, L, family, wpc, cpw, ratio))
    assert torch.isfinite(A).all(), (N, B, L, family)
    if family == "zeros":       # K = b_K for every token: P = 1 / N and every row of A is the value bias
        want = c.bias.double()[:, None, 512:].view(L, 1, 16, 1, 32).expand_as(ref)
        assert kr.worst_ratio(A, want, bound) <= 1.0
    # the fragments: the bf16 packing of the fp32 matrices the launch wrote, bit for bit
    assert torch.equal(fc[:, 1, 1:1 + B], rg.seqfwd.a_fragments(A).view(torch.int16)), (N, B, L, family)
    # without fragments: the same A, and nothing else
    out2, frag2 = out0.cuda(), frag0.cuda()
    _launch(h, dev, out2, None, B, N, L)
    assert torch.equal(out2.cpu().view(torch.int32), oc.view(torch.int32)) and torch.equal(frag2.cpu(), frag0), (N, B, L, family)
    # a repeated launch: the partial sums and matrices are added in a fixed order
    out3, frag3 = out0.cuda(), frag0.cuda()
    _launch(h, dev, out3, frag3, B, N, L)
    assert torch.equal(out3.cpu().view(torch.int32), oc.view(torch.int32)) and torch.equal(frag3.cpu(), fc), (N, B, L, family)
    parity.check("rg_cond_kv N=%d B=%d L=%d %s: A, worst |err| / bound" % (N, B, L, family), ratio, 1.0)


def test_cond_kv_host_refusals(rg, h):
    """Shapes and pointers the entry point refuses: an RgError before any launch, nothing written."""
    N, B, L = 65, 2, 1
    c = kr.cond_kv_case(N, B, L, "grid", 1)
    xhat, w, bias = c.xhat.cuda(), c.w.cuda(), c.bias.cuda()
    big = torch.zeros(B, 513, 512, dtype=torch.bfloat16, device="cuda")      # (what a 513-token launch would read, were it made)
    out0, frag0 = _canaries(B, L)
    out, frag = out0.cuda(), frag0.cuda()
    o, f = out[0, 1, 1:1 + B], frag[0, 1, 1:1 + B]
    so, sf = out.stride(0), frag.stride(0)
    bad = {"n_tok 0": (xhat, w, bias, o, so, f, sf, B, 0, L), "n_tok 513": (big, w, bias, o, so, f, sf, B, 513, L),
           "B 0": (xhat, w, bias, o, so, f, sf, 0, N, L), "L 0": (xhat, w, bias, o, so, f, sf, B, N, 0),
           "null xhat": (None, w, bias, o, so, f, sf, B, N, L), "null w": (xhat, None, bias, o, so, f, sf, B, N, L),
           "null bias": (xhat, w, None, o, so, f, sf, B, N, L), "null out": (xhat, w, bias, None, so, f, sf, B, N, L)}
    for name, args in bad.items():
        with pytest.raises(rg.capi.RgError):
            h.call("cond_kv", *args)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu().view(torch.int32), out0.view(torch.int32)) and torch.equal(frag.cpu(), frag0), name
    h.call("cond_kv", xhat, w, bias, o, so, f, sf, B, N, L)      # the handle is still good
    torch.cuda.synchronize()
    assert torch.isfinite(out[:, 1, 1:1 + B]).all()


# ----------------------------------------------------------------------------------------------- the dispatcher around it
def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def test_set_conditions_mixes_fused_and_grouped_conditions(rg):
    """DenoiserSession.set_conditions takes the fused launch per condition only up to 512 tokens.  With a 513-token audio
    condition that condition alone falls back to the grouped GEMMs + rg_kv_reduce, the other two stay fused, and the
    fragments of ALL conditions must then be repacked from a_pre (SeqForward.set_a).  Everything is compared bit for bit with
    sessions that take one path only, and a session filled in two calls with the same session filled in one."""
    cfg = rg.synth.default_model_cfg(num_layers=2)
    P = rg.synth.synth_denoiser_state(0, cfg)
    W = rg.denoiser.DenoiserWeights(P, cfg, rg.schedule.Schedule(), "cuda")
    TEXT, AUDIO, SPK = (rg.denoiser.CONDS.index(n) for n in ("xf_text", "xf_audio", "xf_spk"))

    def filled(B, data, audio, calls, **kw):
        sess = rg.denoiser.DenoiserSession(W, B, engine="seq", **kw)
        sess.a_pre.fill_(float("nan"))
        mm = torch.ones(B, 43)
        for o0, o1, fin in calls:
            sess.set_conditions(data["word"][o0:o1], audio[o0:o1], data["speaker_ids"][o0:o1], mm[o0:o1], None, offset=o0, finalize=fin)
        torch.cuda.synchronize()
        assert torch.isfinite(sess.a_pre).all()
        return sess

    data = rg.synth.synth_batch(3, seed=4321)
    long_audio = torch.cat((data["audio"], data["audio"][:, :14]), dim=1)
    assert long_audio.shape[1] == 513
    mixed = filled(3, data, long_audio, [(0, 3, True)])
    grouped = filled(3, data, long_audio, [(0, 3, True)], kv_fused=False)
    fused = filled(3, data, data["audio"], [(0, 3, True)])
    assert torch.equal(_bits(mixed.a_pre[:, AUDIO]), _bits(grouped.a_pre[:, AUDIO]))
    for ci in (TEXT, SPK):
        assert torch.equal(_bits(mixed.a_pre[:, ci]), _bits(fused.a_pre[:, ci])), ci
    assert not torch.equal(_bits(mixed.a_pre[:, AUDIO]), _bits(fused.a_pre[:, AUDIO]))      # (the 14 repeated rows do weigh)
    for sess in (mixed, grouped, fused):
        assert torch.equal(_bits(sess.sq.afrag), _bits(rg.seqfwd.a_fragments(sess.a_pre)))
    data5 = rg.synth.synth_batch(5, seed=4322)
    long5 = torch.cat((data5["audio"], data5["audio"][:, :14]), dim=1)
    once = filled(5, data5, long5, [(0, 5, True)])
    twice = filled(5, data5, long5, [(0, 2, False), (2, 5, True)])
    assert torch.equal(_bits(twice.a_pre), _bits(once.a_pre)) and torch.equal(_bits(twice.sq.afrag), _bits(once.sq.afrag))
    assert torch.equal(_bits(once.sq.afrag), _bits(rg.seqfwd.a_fragments(once.a_pre)))
