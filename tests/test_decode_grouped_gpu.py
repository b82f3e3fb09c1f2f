"""GPU: the decode of a batch as grouped launches of all four body parts (GestureRepEncoder(grouped_decode=True), the default):

  * rg_decode_outputs -- the output conversions of the four decoders in one launch -- against the seven launches it replaces,
  * rg_vdec_step with its own ends (latent / table / frames of rg_vdec_args) against the launches around it that they replace,
  * GestureRepEncoder.decode and a pipelined run with the option on against the option off,
  * the launch sequence itself: 2 nb + 2 grouped decoder launches of four parts with the option on, the sequence as it was,
    part after part, with it off.

The option changes how the same arithmetic on the same rows is issued, never a bit: every comparison is torch.equal.
Shapes: the shallowest stacks the fused decoder takes -- num_layers 3 (nb = 1: four launches) and 5 (nb = 2: the skip branch on
both sides of the middle) -- with 1 and 3 clips; the 160 tokens of a sequence are fixed by the kernel."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ("upper", "lower", "face", "hands", "transl", "exps", "contact")
PATHS = {"grouped": dict(part_streams=False, grouped=True), "single_chain": dict(part_streams=False, grouped=False),
         "part_streams": dict(part_streams=True)}
DEPTHS = (3, 5)


def _randn(seed, *shape):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(g.standard_normal(shape).astype(np.float32)).cuda()


@pytest.fixture(scope="module")
def weights(rg):
    """num_layers -> (vae_cfgs, state): the four parts' synthetic VAEs, once per depth."""
    out = {}
    for nl in DEPTHS:
        vae_cfgs = rg.synth.synth_vae_cfgs(decoder_arch="all_encoder", num_layers=nl)
        P = {}
        for i, part in enumerate(rg.synth.PARTS):
            P.update(rg.synth.synth_vae_state(301 + i, vae_cfgs[part], prefix="gesture_rep_encoder.%s_vae." % part))
        out[nl] = (vae_cfgs, P)
    return out


@pytest.fixture(scope="module")
def encoders(rg, weights):
    """(num_layers, path) -> GestureRepEncoder with the joint counts of the synthetic clips (decode() needs them; encode sets
    them in real use).  One encoder serves both settings of the option: decode() reads it per call."""
    d = rg.synth.synth_batch(1, seed=5)
    out = {}
    for nl in DEPTHS:
        vae_cfgs, P = weights[nl]
        for path, kw in PATHS.items():
            gre = rg.vae.GestureRepEncoder(P, vae_cfgs, "cuda", "bf16", **kw)
            assert gre.grouped_decode is True, "the option is on by default"
            assert all(v.vdec is not None and v.vdec.st.nb == (nl - 1) // 2 for v in gre.vaes.values())
            gre._set_joint_counts(d["motion_upper"], d["motion_lower"], d["motion_face"], d["motion_hands"], d["trans"])
            out[nl, path] = gre
    return out


def _latent(B, seed=77):
    z = _randn(seed, B, 43, 512)
    z[:, [10, 21, 32]] = 0
    return z


def _decode(gre, z, on):
    gre.grouped_decode = on
    try:
        out = [t.clone() for t in gre.decode(z)]
    finally:
        gre.grouped_decode = True
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ rg_decode_outputs
@pytest.mark.parametrize("rows", [150, 450])
def test_decode_outputs_equals_the_seven_launches(rg, encoders, rows):
    """The four parts' real widths and column offsets; outputs filled with NaN beforehand, so an element that the one launch
    does not write shows."""
    gre = encoders[3, "grouped"]
    h = gre.h
    widths = [gre.vaes[p].nfeats for p in rg.vae.PARTS]
    joints = [gre.uj, gre.hj, gre.fj, gre.lj]
    n_exp, n_con = widths[2] - 6 * gre.fj, widths[3] - 6 * gre.lj - gre.tj
    assert widths[0] == 6 * gre.uj and widths[1] == 6 * gre.hj and n_exp > 0 and n_con > 0
    src = [_randn(10 + i, rows, w) for i, w in enumerate(widths)]
    nan = lambda w: torch.full((rows, w), float("nan"), device="cuda")
    # (part, output width, first source column) of the plain copies: exps of face; transl and contact of lowertrans
    copies = [(2, n_exp, 6 * gre.fj), (3, gre.tj, 6 * gre.lj), (3, n_con, 6 * gre.lj + gre.tj)]
    want_aa, want_c = [nan(3 * j) for j in joints], [nan(w) for _, w, _ in copies]
    for i in range(4):
        h.call("6d_to_aa", src[i], widths[i], 0, want_aa[i], 3 * joints[i], rows, joints[i])
    for (i, w, c0), out in zip(copies, want_c):
        h.call("copy_cols", src[i], widths[i], c0, out, w, 0, rows, w, 0, 0)
    got_aa, got_c = [nan(3 * j) for j in joints], [nan(w) for _, w, _ in copies]
    ptrs = lambda ts: (ctypes.c_void_p * 4)(*[None if t is None else t.data_ptr() for t in ts])
    ints = lambda vs: (ctypes.c_int * 4)(*vs)
    h.call("decode_outputs", 4, ptrs(src), ints(widths), ptrs(got_aa), ints(joints),
           ptrs([None, None, got_c[0], got_c[1]]), ints([0, 0, copies[0][2], copies[1][2]]), ints([0, 0, n_exp, gre.tj]),
           ptrs([None, None, None, got_c[2]]), ints([0, 0, 0, copies[2][2]]), ints([0, 0, 0, n_con]), rows)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(got_aa + got_c, want_aa + want_c)):
        assert not torch.isnan(b).any(), i
        assert torch.equal(a, b), (i, (a - b).abs().max().item())
    # fewer than four parts, and a column range that does not fit its source is refused
    one = nan(3 * joints[1])
    h.call("decode_outputs", 1, ptrs(src[1:2] + [None] * 3), ints(widths[1:2] + [0] * 3), ptrs([one, None, None, None]),
           ints(joints[1:2] + [0] * 3), ptrs([None] * 4), ints([0] * 4), ints([0] * 4), ptrs([None] * 4), ints([0] * 4), ints([0] * 4), rows)
    torch.cuda.synchronize()
    assert torch.equal(one, want_aa[1])
    with pytest.raises(rg.capi.RgError):
        h.call("decode_outputs", 1, ptrs(src[1:2] + [None] * 3), ints(widths[1:2] + [0] * 3), ptrs([one, None, None, None]),
               ints(joints[1:2] + [0] * 3), ptrs([got_c[0], None, None, None]), ints([widths[1] - 1, 0, 0, 0]), ints([2, 0, 0, 0]),
               ptrs([None] * 4), ints([0] * 4), ints([0] * 4), rows)


# ------------------------------------------------------------------------------------------------ decode(): on == off
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nl", DEPTHS)
def test_decode_with_the_option_equals_without(encoders, nl, B):
    """All seven outputs in the three launch paths, option on against option off -- and the paths against each other."""
    z = _latent(B)
    ref = None
    for path in PATHS:
        gre = encoders[nl, path]
        off, on = _decode(gre, z, False), _decode(gre, z, True)
        for nm, a, b in zip(NAMES, on, off):
            assert a.shape == b.shape and not torch.isnan(b).any(), (path, nm)
            assert torch.equal(a, b), (path, nm, (a - b).abs().max().item())
        ref = ref or off
        for nm, a, b in zip(NAMES, off, ref):
            assert torch.equal(a, b), (path, nm)


def test_debug_keep_hands_out_the_decoder_outputs_in_front_of_the_conversion(encoders):
    """debug_keep keeps its meaning: (part, decoder output [B * frames, nfeats]) of every part, the same bits on and off."""
    z = _latent(1)
    gre = encoders[3, "grouped"]
    kept = {}
    for on in (False, True):
        gre.debug_keep = []
        try:
            _decode(gre, z, on)
            kept[on] = [(p, t.clone()) for p, t in gre.debug_keep]
        finally:
            gre.debug_keep = None
    assert [p for p, _ in kept[True]] == [p for p, _ in kept[False]] == list(gre.vaes)
    for (p, a), (_, b) in zip(kept[True], kept[False]):
        assert a.shape == (150, gre.vaes[p].nfeats) and torch.equal(a, b), p


# ------------------------------------------------------------------------------------------------ the launch sequence
def _issued(gre, z, on):
    """Names (and, for the grouped decoder launch, the number of parts) of the launches one decode() issues."""
    h, log = gre.h, []
    real = h.call

    def call(name, *args, stream=None, keep=None):
        if not (h.recorder is not None and stream is None):      # (a recorded call is issued later, through here again)
            log.append((name, args[1]) if name == "vdec_step_grouped" else name)
        return real(name, *args, stream=stream, keep=keep)

    h.call = call
    try:
        _decode(gre, z, on)
    finally:
        del h.call
    return log


@pytest.mark.parametrize("nl", DEPTHS)
def test_launch_sequence(encoders, nl):
    nb = (nl - 1) // 2
    z = _latent(1)
    log = _issued(encoders[nl, "grouped"], z, True)
    assert log == [("vdec_step_grouped", 4)] * (2 * nb + 2) + ["gemm_grouped", "decode_outputs"], log
    # without the option: the jobs differ in length, so the recorder issues them one after the other, as it always did
    tails = (["6d_to_aa"], ["6d_to_aa"], ["6d_to_aa", "copy_cols"], ["6d_to_aa", "copy_cols", "copy_cols"])
    part = ["copy_rows", "add_rows"] + ["vdec_step"] * (2 * nb + 2) + ["copy_rows", "gemm"]
    want_off = [n for t in tails for n in part + t]
    assert _issued(encoders[nl, "grouped"], z, False) == want_off
    assert _issued(encoders[nl, "single_chain"], z, False) == want_off
    # one chain without the recorder, option on: the same launches singly, the conversions still as one
    assert _issued(encoders[nl, "single_chain"], z, True) == (["vdec_step"] * (2 * nb + 2) + ["gemm"]) * 4 + ["decode_outputs"]


# ------------------------------------------------------------------------------------------------ rg_vdec_step's own ends
@pytest.fixture(scope="module")
def vdec_cases(encoders):
    """(num_layers, nseq) -> (latent, reference by row_off): the old form -- zeros / copy_rows / add_rows in front of the stack,
    copy_rows behind it -- computed once and left unchanged."""
    out = {}
    for nl in DEPTHS:
        vae = encoders[nl, "single_chain"].vaes["upper"]
        h, table = vae.h, vae.pe_dec[:160].contiguous()
        for nseq in (1, 3):
            lat = _randn(400 + nseq, nseq, 43, 512)          # every row non-zero: a wrong row shows
            ref = {}
            for row_off in (0, 11, 22, 33):
                x = torch.zeros(nseq * 160, 512, device="cuda")
                h.call("copy_rows", lat, x, nseq, 10, 512, 43, row_off, 160, 0)
                pos = torch.empty_like(x)
                h.call("add_rows", x, table, pos, x.numel(), 160 * 512)
                x0 = x.clone()
                y = vae.vdec.run(x, pos, nseq)
                fr = torch.empty(nseq * 150, 512, device="cuda")
                h.call("copy_rows", y, fr, nseq, 150, 512, 160, 10, 150, 0)
                ref[row_off] = (x0, pos, y, fr)
            torch.cuda.synchronize()
            out[nl, nseq] = (lat, ref)
    return out


@pytest.mark.parametrize("nseq", [1, 3])
@pytest.mark.parametrize("nl", DEPTHS)
def test_vdec_own_ends_equal_the_launches_around_it(encoders, vdec_cases, nl, nseq):
    vae = encoders[nl, "single_chain"].vaes["upper"]
    table = vae.pe_dec[:160].contiguous()
    lat, ref = vdec_cases[nl, nseq]
    nan = lambda rows: torch.full((rows, 512), float("nan"), device="cuda")
    for row_off in (0, 11, 22, 33):
        x0, pos0, y0, fr0 = ref[row_off]
        # all three: the input rows from the latent, pos from the table, the frame rows stored compactly
        x, pos, fr = nan(nseq * 160), nan(nseq * 160), nan(nseq * 150)
        got = vae.vdec.run(x, pos, nseq, latent=lat, row_off=row_off, n_lat=10, table=table, frames=fr)
        assert got is fr and torch.equal(fr, fr0), (row_off, (fr - fr0).abs().max().item())
        assert torch.equal(pos, pos0), row_off                     # what launch 0 left for the later launches
    # each pointer alone: a null pointer keeps that end as it was
    x0, pos0, y0, fr0 = ref[11]
    x = nan(nseq * 160)
    assert torch.equal(vae.vdec.run(x, pos0.clone(), nseq, latent=lat, row_off=11, n_lat=10), y0)       # x updated in place
    pos = nan(nseq * 160)
    assert torch.equal(vae.vdec.run(x0.clone(), pos, nseq, table=table), y0) and torch.equal(pos, pos0)
    fr, x = nan(nseq * 150), x0.clone()
    assert torch.equal(vae.vdec.run(x, pos0.clone(), nseq, n_lat=10, frames=fr), fr0)
    assert torch.equal(vae.vdec.run(x0.clone(), pos0.clone(), nseq), y0)                                  # none: the old call


def test_vdec_own_ends_refuse_rows_outside_the_latent(rg, encoders):
    vae = encoders[3, "single_chain"].vaes["upper"]
    x, pos = torch.zeros(160, 512, device="cuda"), torch.zeros(160, 512, device="cuda")
    lat = torch.zeros(1, 43, 512, device="cuda")
    with pytest.raises(rg.capi.RgError):
        vae.vdec.run(x, pos, 1, latent=lat, row_off=34, n_lat=10)            # rows [34, 44) of 43
    a = rg.vencfwd.VdecArgs()
    st = vae.vdec.st
    a.wstream, a.pstream, a.x, a.pos = st.wstream.data_ptr(), st.pstream.data_ptr(), x.data_ptr(), pos.data_ptr()
    bufs = [torch.empty(n, device="cuda", dtype=torch.uint8) for n in (4 * 48 * 1024, 2 * 160 * 512 * 2, 2 * 160 * 512 * 2, 4 * st.nb * 8 * 12 * 64 * 4 * 4)]
    a.qimg, a.kbuf, a.vt, a.xbuf = (b.data_ptr() for b in bufs)
    a.nseq, a.nb, a.step = 1, st.nb, 0
    a.latent, a.lat_T, a.lat_row0, a.n_lat = lat.data_ptr(), 43, 34, 10
    with pytest.raises(rg.capi.RgError):                                       # the entry point's own check
        vae.h.call("vdec_step", ctypes.byref(a))


# ------------------------------------------------------------------------------------------------ the pipeline
def _clone(v):
    if torch.is_tensor(v):
        return v.clone()
    if isinstance(v, dict):
        return {k: _clone(x) for k, x in v.items() if not x.__class__.__module__.startswith("torch") or torch.is_tensor(x)}
    if isinstance(v, (list, tuple)):
        return [_clone(x) for x in v]
    return v


def _same(a, b, path="results"):
    if torch.is_tensor(a) or torch.is_tensor(b):
        assert torch.is_tensor(a) and torch.is_tensor(b) and a.shape == b.shape and torch.equal(a.cpu(), b.cpu()), path
    elif isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], "%s[%r]" % (path, k))
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (path, i))
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), path
    elif a.__class__.__module__.startswith("torch"):     # events, streams of an asynchronous result: not data
        pass
    else:
        assert a == b, path


def test_pipelined_run_with_the_option_equals_without(rg):
    """Three batches of two clips through submit() / flush(), model option on (the default) against off: every tensor of the
    results.  A 2-layer denoiser, the shallowest VAEs the fused stacks take, a database of 64 entries."""
    dev = torch.device("cuda", 0)
    cfg = rg.synth.default_model_cfg(num_layers=2)
    vae_cfgs = rg.synth.synth_vae_cfgs(decoder_arch="all_encoder", num_layers=3)
    db = rg.synth.SyntheticDataset(64, seed=11, device=dev, feat_device=dev)
    P = rg.synth.synth_full_state(0, cfg, vae_cfgs)
    B, N = 2, 3
    batches = []
    for i in range(N):
        d = rg.synth.synth_batch(B, seed=900 + i, device=dev)
        qs = [rg.synth.synth_query(50 * i + j) for j in range(B)]
        d["discourse"], d["prominence"] = [q["discourse"] for q in qs], [q["prominence"] for q in qs]
        d["text_features"] = [q["text_features"].to(dev) for q in qs]
        d["speaker_ids"] = torch.tensor([[q["speaker_id"]] * 150 for q in qs], device=dev)
        batches.append(d)
    results = {}
    for on in (False, True):
        model = rg.build_architecture(rg.synth.reference_style_model_cfg(cfg, vae_cfgs, with_retrieval=True), database=db,
                                      device=dev, async_results=True, **({} if on else dict(grouped_decode=False)))
        model.load_state_dict(P)
        model.eval()
        assert model.grouped_decode is on and model.model.gesture_rep_encoder.grouped_decode is on
        got = []
        take = lambda out: got.append(_clone(out))
        for i in range(N):
            d = dict(batches[i], trans=batches[i]["trans"].clone())
            ikw = dict(use_inversion=True, insertion_guidance=True, guidance_iters=[2] * 25 + [0] * 25, guidance_lr=0.1,
                       noise_tape=rg.synth.NoiseTape(4000 + i))
            out = model.submit(**dict(d, retrieval_method="discourse", inference_kwargs=ikw))
            if out is not None:
                with torch.cuda.stream(out["done_stream"]):
                    take(out)
            del out
        for out in model.flush():
            with torch.cuda.stream(out["done_stream"]):
                take(out)
        torch.cuda.synchronize()
        assert len(got) == N
        results[on] = got
    _same(results[True], results[False])
