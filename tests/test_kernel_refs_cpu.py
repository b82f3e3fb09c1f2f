"""CPU: the bounds of tests/kernel_refs.py, checked before any kernel runs.  A float32 / bf16 emulation of each kernel's
rounding contract must stay inside the bounds against the fp64 reference (loose enough for a correct kernel), and deliberately
wrong variants -- a dropped probability column, statistics of the neighbouring head group, a one-pass variance -- must exceed them (tight
enough to fail on a subtle error).  Same seeds and shapes as the GPU tests.  The stages of the fused stacks (rg_seq_forward,
rg_venc_forward, rg_vdec_step) are emulated one by one, teacher-forced like their GPU tests, with the wrong variants of
kr.SEQ_MUTANTS, kr.VENC_MUTANTS and kr.VDEC_MUTANTS; the condition side's one launch (rg_cond_kv) at every wave split and clip
packing with those of kr.COND_KV_MUTANTS."""
import pytest
import torch

import kernel_refs as kr


def _sa_inputs(R, T, D, seed):
    ld = 3 * D + 8
    qkv = kr.randn((R * T, ld), seed)
    qkv[:, :D] = kr.softmax_heads(qkv[:, :D], D)
    mask = torch.ones(R, T)
    mask[:, [10, 21, 32]] = 0
    mask[1] = 0                      # one row of the batch fully masked
    return qkv, mask


@pytest.mark.parametrize("mfma", [False, True])
@pytest.mark.parametrize("T", [33, 43, 64])
def test_sa_emulation_inside_bounds_and_mutants_outside(T, mfma):
    R, D = 3, 256
    qkv, mask = _sa_inputs(R, T, D, 100 + T)
    y, by = kr.sa_ref(qkv, mask, R, T, D, mfma)
    st, bst = kr.group_stats(y, 128), kr.group_stats_bound(y, by, 128)
    ye, se = kr.sa_emulate(qkv, mask, R, T, D, mfma)
    ry, rs = kr.worst_ratio(ye, y, by), kr.worst_ratio(se, st, bst)
    print("sa emulation T=%d mfma=%d: y %.3f stats %.3f" % (T, mfma, ry, rs))
    assert torch.isfinite(ye).all() and ry <= 1.0 and rs <= 1.0
    assert (ye.view(R, T, D)[1] == 0).all()                       # the fully masked row: y = 0
    yd, sd = kr.sa_emulate(qkv, mask, R, T, D, mfma, drop=(5, 7))  # one probability column dropped
    assert kr.worst_ratio(yd, y, by) > 1.0
    _, sw = kr.sa_emulate(qkv, mask, R, T, D, mfma, swap_stats=True)   # statistics slot of the neighbouring head group
    assert kr.worst_ratio(sw, st, bst) > 1.0


def test_ca_emulation_grid_rounding():
    R, Rc, T, D, nc = 4, 2, 43, 256, 3
    H = D // 32
    q3 = kr.softmax_heads(kr.randn((R * T, nc * D), 201), nc * D)
    Apre, Aunc = kr.randn((nc, Rc, H, 32, 32), 202, 0.3), kr.randn((nc, H, 32, 32), 203, 0.3)
    qm = torch.ones(nc, R, T)
    qm[0, 1, [10, 20, 30]] = 0
    qm[2, 3, [10, 20, 30]] = 0
    y, e, tie = kr.ca_ref(q3, Apre, Aunc, qm, R, Rc, T, D, nc)
    ye = kr.ca_emulate(q3, Apre, Aunc, qm, R, Rc, T, D, nc)
    assert kr.worst_ratio(ye, y, e) <= 1.0
    msk = (qm == 0).permute(1, 2, 0).reshape(R * T, nc, 1).expand(R * T, nc, D).reshape(R * T, nc * D)
    assert torch.equal(ye[msk] * 16, torch.round(ye[msk] * 16))   # exact multiples of 1/16
    print("ca emulation: %d near-tie elements of %d masked" % (int(tie.sum()), int(msk.sum())))
    wrong = kr.ca_emulate(q3, Apre, Aunc, None, R, Rc, T, D, nc)   # no rounding on the masked rows
    assert kr.worst_ratio(wrong, y, e) > 1.0


@pytest.mark.parametrize("N", [1, 9, 499])
def test_kv_reduce_emulation(N):
    B, D = 2, 128
    kv = kr.randn((B * N, 2 * D + 4), 300 + N)
    kv[:, 5] = torch.from_numpy(kr.rng(310 + N).uniform(-80, 80, B * N)).float()
    A, bound = kr.kv_reduce_ref(kv, B, N, D)
    assert kr.worst_ratio(kr.kv_reduce_emulate(kv, B, N, D), A, bound) <= 1.0
    if N > 1:       # a wrong variant: the value columns of the neighbouring head
        assert kr.worst_ratio(kr.kv_reduce_emulate(kv, B, N, D).roll(1, dims=1), A, bound) > 1.0


@pytest.mark.parametrize("hd,Sk", [(16, 17), (32, 33), (64, 192), (64, 499), (128, 65)])
@pytest.mark.parametrize("mfma", [False, True])
def test_mha_emulation(hd, Sk, mfma):
    if not mfma and Sk > 192:
        return
    B, H, Sq = 2, 3, 17
    x = kr.randn((B * max(Sq, Sk), 3 * H * hd + 8), 400 + hd + Sk)
    q, k, v = x[:B * Sq, :H * hd], x[:B * Sk, H * hd:2 * H * hd], x[:B * Sk, 2 * H * hd:3 * H * hd]
    for qs in (1.0, 60.0 / hd ** 0.5):        # plain scores, and score magnitudes near 60
        o, bound = kr.mha_ref(q * qs, k, v, B, H, Sq, Sk, hd, mfma)
        r = kr.worst_ratio(kr.mha_emulate(q * qs, k, v, B, H, Sq, Sk, hd, mfma), o, bound)
        print("mha emulation hd=%d Sk=%d mfma=%d qscale=%.1f: %.3f" % (hd, Sk, mfma, qs, r))
        assert r <= 1.0
    o, bound = kr.mha_ref(q, k, v, B, H, Sq, Sk, hd, mfma)
    assert kr.worst_ratio(kr.mha_emulate(q, k, v, B, H, Sq, Sk, hd, mfma, drop_key=Sk // 2), o, bound) > 1.0


@pytest.mark.parametrize("dim", [61, 64, 512, 768])
def test_layernorm_emulation(dim):
    x = kr.randn((5, dim), 500 + dim)
    x[3] += 1000.0                              # mean 1e3, unit spread
    g, b = 1 + 0.2 * kr.randn((dim,), 501), 0.2 * kr.randn((dim,), 502)
    for eps in (1e-12, 1e-5):
        ref, bound = kr.layernorm_ref(x, None, g, b, eps)
        assert kr.worst_ratio(kr.layernorm_emulate(x, None, g, b, eps), ref, bound) <= 1.0
        assert kr.worst_ratio(kr.layernorm_emulate(x, None, g, b, eps, one_pass=True), ref, bound) > 1.0


@pytest.mark.parametrize("seg_len,nparts", [(512, 4), (64, 8), (512, 1)])
def test_stylization_emulation(seg_len, nparts):
    x = kr.randn((18, seg_len), 600 + seg_len) * 2.0 + 0.3
    g, b = 1 + 0.2 * kr.randn((seg_len,), 601), 0.2 * kr.randn((seg_len,), 602)
    ss = kr.randn((2 * seg_len,), 603, 0.3)
    stats = kr.group_stats(x.double(), seg_len // nparts).float()
    for sc, sh in ((None, None), (ss[:seg_len], ss[seg_len:])):
        ref, e = kr.styl_ref(x.double(), 0.0, g.double(), b.double(), None if sc is None else sc.double(), None if sh is None else sh.double(), nparts + 1)
        bm, bu = kr.bf16_bounds(ref, e)
        got = kr.styl_emulate(x, stats, g, b, sc, sh)
        assert kr.worst_ratio(got, ref, bu) <= 1.0 and kr.worst_ratio(got, ref, bm) <= 1.0
        wrong = kr.styl_emulate(x, stats.roll(1, dims=0), g, b, sc, sh)       # the statistics of the neighbouring row
        assert kr.worst_ratio(wrong, ref, bm) > 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# fused GEMM: every case of test_gemm_kernels_gpu.py whose grid does not depend on the CU count, on the CPU emulation
_GEMM = kr.gemm_cases(256)
_GEMM_MUTANTS = {"trunc_a": "e1", "drop_k_tail": "g1", "tbias_row": "e2", "res_ldo": "g3", "stats_slot": "g1", "softmax_shift": "e2",
                 "ln_kpad": "g7", "styl_noscale": "e3", "gb_group0": "e9", "wlo_no_hilo": "e8"}


def _gemm_ratios(c, ref, got):
    """worst |err| / bound of every output of a GEMM case (no element excluded), bf16 outputs in both forms of bf16_bounds."""
    r = {}
    if c.out_bf16:
        bm, bu = kr.bf16_bounds(ref["out"], ref["e"])
        r["out"], r["out ulp"] = kr.worst_ratio(got["out"], ref["out"], bm), kr.worst_ratio(got["out"], ref["out"], bu)
    else:
        r["out"] = kr.worst_ratio(got["out"], ref["out"], ref["e"])
    if c.want_stats:
        r["stats"] = kr.worst_ratio(got["stats"], ref["stats"], ref["e_stats"])
    if c.want_out2:
        bm, bu = kr.bf16_bounds(ref["out2"], ref["e2"])
        r["out2"], r["out2 ulp"] = kr.worst_ratio(got["out2"], ref["out2"], bm), kr.worst_ratio(got["out2"], ref["out2"], bu)
    return r


@pytest.mark.parametrize("name", [n for n in _GEMM if "more workgroups" not in n])
def test_gemm_emulation_inside_bounds_and_mutants_outside(name):
    c = _GEMM[name]()
    ref = kr.gemm_ref(c)
    r = _gemm_ratios(c, ref, kr.gemm_emulate(c))
    print("gemm emulation %s [%s]: %s" % (name, c.variant, "  ".join("%s %.3f" % kv for kv in r.items())))
    assert max(r.values()) <= 1.0, r
    for mutant, key in _GEMM_MUTANTS.items():
        if name.split()[0] == key:
            rm = _gemm_ratios(c, ref, kr.gemm_emulate(c, mutant))
            print("   mutant %s: %s" % (mutant, "  ".join("%s %.3g" % kv for kv in rm.items())))
            assert max(rm.values()) > 1.0, (mutant, rm)


def test_gemm_every_mutant_has_a_case():
    keys = {n.split()[0] for n in _GEMM}
    assert set(_GEMM_MUTANTS) == set(kr.GEMM_MUTANTS) and set(_GEMM_MUTANTS.values()) <= keys


# ---------------------------------------------------------------------------------------------------------------------------
# fused denoiser stack (rg_seq_forward and its other launch forms): the stage references of test_seq_stages_gpu.py on the CPU
# emulation, teacher-forced like the GPU test (every stage starts from the emulation's own output of the stage before it)
@pytest.fixture(scope="module")
def seq_model(rg):
    """T -> SeqModel of the two-layer synthetic denoiser the GPU test runs (rows off centre: kr.off_centre),
    with the AdaLN table computed on the CPU."""
    cache = {}

    def get(T):
        if T not in cache:
            cfg = rg.synth.default_model_cfg(num_layers=2)
            cfg["max_seq_len"] = kr.seq_frames(T)
            sd = kr.off_centre(rg.synth.synth_denoiser_state(0, cfg))
            g = lambda name: sd[name].float()
            cache[T] = kr.SeqModel(g, kr.adaln_table(g, 2, rg.schedule.Schedule().timestep_map), 2, T)
        return cache[T]
    return get


def _seq_chain(m, c, mutant=None, layers=None):
    """Every stage of the launch c on the emulation: {(layer, stage): (worst |err| / bound, median bound / rms(ref), near-tie
    elements, masked elements)}; layer -1 = the embedding (stage 1), layer L = the head (stage 0)."""
    res, detail = {}, {}
    res["detail"] = detail       # stages 11-13: (worst ratio of the unmasked rows, masked elements outside their bound, ... off the grid)

    def one(key, stage, l, inp):
        got = kr.seq_stage_emulate(stage, m, c, l, inp, mutant)
        ref = kr.seq_stage_ref(stage, m, c, l, inp)
        ties = masked = 0
        assert torch.isfinite(got).all()
        r = kr.worst_ratio(got, ref[0], ref[1])
        if len(ref) == 3:      # stages 11-13: the masked rows' bound is 0 or one grid step, so the ratio there is 0, 1 or "infinite"
            msk = (c.qm[stage - 11] == 0)[:, :, None].expand_as(got)
            ties, masked = int(ref[2].sum()), int(msk.sum())
            detail[key] = (kr.worst_ratio(got[~msk], ref[0][~msk], ref[1][~msk]),
                           int(((got.double() - ref[0]).abs() > ref[1])[msk].sum()), int((got[msk] * 16 != torch.round(got[msk] * 16)).sum()))
        res[key] = (r, float((ref[1] / ref[0].pow(2).mean().sqrt()).median()), ties, masked)
        return got

    X = one((-1, 1), 1, 0, {})
    L = m.L if layers is None else layers
    for l in range(L):
        state = {"in": X}
        for stage in kr.SEQ_STAGES:
            state[stage] = one((l, stage), stage, l, kr.seq_stage_inputs(stage, c, state))
        X = state[4]
    one((L, 0), 0, 0, dict(X=X))
    return res


@pytest.mark.parametrize("launch", [la for la in kr.SEQ_LAUNCHES if la[0] == 1], ids=lambda la: "B%d-T%d-step%d" % la[:3])
def test_seq_stage_emulation_inside_bounds(seq_model, launch):
    """The unmutated emulation stays inside the bound at every stage of both layers and at the head, on the inputs of the GPU
    launches with B = 1, and at most 5 % of the masked-row elements of stages 11-13 lie within their bound of a rounding tie.

    Median bound / rms(ref) per stage, measured on this test (information, not a limit): embedding 6e-4, stage 10 2e-2 to 3e-2,
    stage 2 7e-3 to 1e-2, stages 11-13 2e-2 to 3e-2, stage 3 5e-3, stage 4 8e-3 to 1.1e-2 (the statistical tier: eight standard deviations of the variance
    model, the emulation's worst element at 0.35 to 0.4 of it), head 2e-3."""
    c = kr.seq_launch_case(*launch)
    res = _seq_chain(seq_model(c.T), c)
    res.pop("detail")
    for (l, stage), (r, rel, ties, masked) in res.items():
        print("seq emulation %s layer %d stage %2d: worst |err| / bound %.3f   median bound / rms(ref) %.2e%s"
              % ("B%d T%d step %d" % launch[:3], l, stage, r, rel, "   near ties %d / %d" % (ties, masked) if masked else ""))
        assert r <= 1.0, (l, stage, r)
        assert ties <= 0.05 * masked, (l, stage, ties, masked)


# mutant -> the launch (B, T, step, step_b, split) it is shown on: the smallest B at which it changes anything
_SEQ_MUTANT_LAUNCH = {mu: (1, 43, 49, None, None) for mu in kr.SEQ_MUTANTS}
_SEQ_MUTANT_LAUNCH["styl_step"] = _SEQ_MUTANT_LAUNCH["ffn_styl_step"] = (3, 27, 40, 9, 1)          # two step groups need two clips
_SEQ_MUTANT_LAUNCH["pad_rows"] = (1, 27, 49, None, None)     # an empty third token block: 21 padded rows


@pytest.mark.parametrize("mutant", sorted(kr.SEQ_MUTANTS))
def test_seq_stage_mutants_exceed_the_bound_at_their_stage(seq_model, mutant):
    """Each deliberately wrong emulation exceeds the bound at the stage it belongs to and stays inside it at every stage
    before (first layer; the chain is teacher-forced, so the stages behind it see their own inputs again)."""
    c = kr.seq_launch_case(*_SEQ_MUTANT_LAUNCH[mutant])
    res = _seq_chain(seq_model(c.T), c, mutant, layers=1)
    target = kr.SEQ_MUTANTS[mutant]
    order = [1] + list(kr.SEQ_STAGES)
    if target in (11, 12, 13):
        un, wrong, off = res["detail"][(0, target)]
        print("seq mutant %-16s stage %2d: unmasked rows worst |err| / bound %.3g; masked elements outside their bound %d, off the 1/16 grid %d"
              % (mutant, target, un, wrong, off))
        assert (un > 1.0) if mutant == "a_blocks_swapped" else (wrong > 0 and off > 0)
    print("seq mutant %-16s caught at stage %2d: worst |err| / bound %.3g   (stages before: %s)"
          % (mutant, target, min(res[(0, target)][0], 9.99e99), "  ".join("%d: %.3f" % (s, res[(-1 if s == 1 else 0, s)][0]) for s in order[:order.index(target)])))
    for s in order[:order.index(target)]:
        assert res[(-1 if s == 1 else 0, s)][0] <= 1.0, (mutant, "already outside at stage %d" % s)
    assert res[(0, target)][0] > 1.0, (mutant, res[(0, target)][0])


def test_rounded_tier_flags_exactly_the_ties():
    """`_rounded`: where it reports distance 0, every fp32 value within e of x rounds to the same bf16 number."""
    x = kr.randn((4096,), 77).double() * 3
    e = x.abs() * 2.0 ** -14
    xb, E = kr._rounded(x, e)
    for sgn in (-1.0, 1.0):
        moved = kr.bf16((x + sgn * e).float()).double()
        assert bool(((moved == xb) | (E > 0)).all())
        assert bool(((moved - xb).abs() <= E + 1e-300).all())
    assert 0 < int((E > 0).sum()) < x.numel() // 4


# ---------------------------------------------------------------------------------------------------------------------------
# fused VAE encoder stack (rg_venc_forward): the block references of test_venc_stages_gpu.py on the CPU emulation
@pytest.fixture(scope="module")
def venc_model(rg):
    cache = {}

    def get(num_layers):
        if num_layers not in cache:
            sd = rg.synth.synth_vae_state(kr.VENC_SEED, rg.synth.default_vae_cfg("upper", num_layers=num_layers))
            cache[num_layers] = kr.VencModel(sd, num_layers)
        return cache[num_layers]
    return get


def _venc_chain(m, X, mutant=None):
    """worst |err| / bound and median bound / rms(ref) behind every block (teacher-forced on the emulation) and of `out`."""
    outs, res = [], []
    for b in range(2 * m.nb + 1):
        sk = m.skip_of(b)
        Xs = outs[sk] if sk is not None else None
        got = kr.venc_block_emulate(m, b, X, Xs, mutant)
        ref, bound = kr.venc_block_ref(m, b, X, Xs)
        assert torch.isfinite(got).all()
        res.append((kr.worst_ratio(got, ref, bound), float((bound / ref.pow(2).mean().sqrt()).median())))
        outs.append(got)
        X = got
    ref, bound = kr.venc_final_ref(m, X)
    res.append((kr.worst_ratio(kr.venc_final_emulate(m, X), ref, bound), float((bound / ref.pow(2).mean().sqrt()).median())))
    return res


@pytest.mark.parametrize("num_layers,S,nseq", [c for c in kr.VENC_CASES if c[2] == 1])
def test_venc_block_emulation_inside_bounds(venc_model, num_layers, S, nseq):
    """The unmutated emulation stays inside the bound behind every block and at `out`.

    Median bound / rms(ref), measured on this test (information, not a limit): 6e-3 to 9e-3 behind every block (the bound is
    eight standard deviations of the variance model; the emulation's worst element sits at 0.3 to 0.45 of it), 1e-5 at `out`."""
    m = venc_model(num_layers)
    res = _venc_chain(m, kr.venc_input(nseq, S, num_layers))
    for b, (r, rel) in enumerate(res):
        print("venc emulation layers %d S %d %s: worst |err| / bound %.3f   median bound / rms(ref) %.2e"
              % (num_layers, S, "block %d" % b if b < len(res) - 1 else "out", r, rel))
        assert r <= 1.0, (b, r)


_VENC_MUTANT_BLOCK = dict(no_scale=0, norm2_for_norm1=0, skip_swapped=3)


@pytest.mark.parametrize("mutant,first", sorted(_VENC_MUTANT_BLOCK.items()))
def test_venc_block_mutants_exceed_the_bound_at_their_block(venc_model, mutant, first):
    """first: the first block the wrong variant touches (the skip linear sits in front of the output blocks: block nb + 1)."""
    assert set(_VENC_MUTANT_BLOCK) == set(kr.VENC_MUTANTS)
    m = venc_model(5)
    res = _venc_chain(m, kr.venc_input(1, 17, 5), mutant)
    print("venc mutant %-16s caught at block %d: worst |err| / bound %.3g   (blocks before: %s)"
          % (mutant, first, res[first][0], "  ".join("%.3f" % r for r, _ in res[:first])))
    assert all(r <= 1.0 for r, _ in res[:first]) and res[first][0] > 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# block-fused VAE decoder (rg_vdec_step): the launch references of test_vdec_stages_gpu.py on the CPU emulation
@pytest.fixture(scope="module")
def vdec_model(rg):
    cache = {}

    def get(num_layers):
        if num_layers not in cache:
            sd = rg.synth.synth_vae_state(kr.VDEC_SEED, rg.synth.default_vae_cfg("upper", num_layers=num_layers))
            cache[num_layers] = kr.VdecModel(sd, num_layers)
        return cache[num_layers]
    return get


def _vdec_chain(m, X, mutant=None):
    """Teacher-forced on the emulation, in the order a decode passes them: [(name, worst |err| / bound, median bound / rms(ref))]
    with the names "<b> skip" (output blocks: the residual behind the skip linear, worst-case tier), "<b> q" / "<b> k" / "<b> v"
    (the stored bf16 projections, worst-case tier: the larger of the half-ulp form and the MARGIN form of `bf16_bounds`),
    "<b> out" (the state behind block b, statistical tier) and "final"."""
    pos = X + m.table
    res, outs, prev = [], [], None
    rel = lambda ref, bound: float((bound / ref.pow(2).mean().sqrt()).median())
    for b in range(2 * m.nb + 1):
        sk = m.skip_of(b)
        Xs = outs[sk] if sk is not None else None
        em = kr.vdec_block_emulate(m, b, X, pos, Xs, mutant, prev)
        if sk is not None:
            ref, bound = kr.vdec_skip_ref(m, b, X, Xs)
            res.append(("%d skip" % b, kr.worst_ratio(em.x, ref, bound), rel(ref, bound)))
        else:
            assert torch.equal(em.x, X)
        proj = kr.vdec_proj_ref(m, b, em.x, pos)
        for nm in ("q", "k", "v"):
            ref, e = proj[nm]
            bound, b_ulp = kr.bf16_bounds(ref, e)
            got = getattr(em, nm)
            res.append(("%d %s" % (b, nm), max(kr.worst_ratio(got, ref, b_ulp), kr.worst_ratio(got, ref, bound)), rel(ref, b_ulp)))
        ref, bound = kr.vdec_block_ref(m, b, em.x, pos)
        assert torch.isfinite(em.out).all()
        res.append(("%d out" % b, kr.worst_ratio(em.out, ref, bound), rel(ref, bound)))
        outs.append(em.out)
        X, prev = em.out, (em.k, em.v)
    ref, bound = kr.vdec_final_ref(m, X)
    res.append(("final", kr.worst_ratio(kr.vdec_final_emulate(m, X, mutant), ref, bound), rel(ref, bound)))
    return res


@pytest.mark.parametrize("kind", kr.VDEC_KINDS)
@pytest.mark.parametrize("num_layers", [3, 5])
def test_vdec_emulation_inside_bounds(vdec_model, num_layers, kind):
    """The unmutated emulation stays inside the bound in all three tiers -- the skip linear and the stored Q, K, V (worst case),
    the state behind every block and the final norm (statistical) -- for the product's input and for dense rows.

    Measured on this test (information, not a limit): statistical tier 0.33 to 0.58 of the bound behind every block, median
    bound / rms(ref) 6e-3 to 1e-2 (eight standard deviations of the variance model), 0.03 at the final norm; skip linear 1e-4 to
    3e-4; Q, K, V 0.83 to 0.96 of half a bf16 ulp + the accumulation bound (a rounding to nearest fills half an ulp by
    construction).  The dense input needed no change of the variance model."""
    m = vdec_model(num_layers)
    res = _vdec_chain(m, kr.vdec_input(1, num_layers, kind))
    for name, r, rel in res:
        print("vdec emulation layers %d %-6s %-7s: worst |err| / bound %.3g   median bound / rms(ref) %.2e" % (num_layers, kind, name, r, rel))
    for name, r, rel in res:
        assert r <= 1.0, (name, r)


# wrong variant -> the first block or buffer it touches (num_layers 5: blocks 0 .. 4, the skip linears in front of 3 and 4)
_VDEC_MUTANT_FIRST = dict(no_scale="0 q", k_no_pos="0 k", v_with_pos="0 v", heads_of_32="0 out", stale_tile="0 out",
                          drop_last_keys="0 out", norm2_for_norm1="0 out", skip_swapped="3 skip", no_final_norm="final")


@pytest.mark.parametrize("kind", kr.VDEC_KINDS)
@pytest.mark.parametrize("mutant", kr.VDEC_MUTANTS)
def test_vdec_mutants_exceed_the_bound_where_they_first_touch(vdec_model, mutant, kind):
    """Every deliberately wrong emulation is inside every bound before the first block or buffer it touches and outside there.
    "stale_tile" reads zeros at block 0 and the previous block's keys and values behind it: it is outside behind EVERY block."""
    assert set(_VDEC_MUTANT_FIRST) == set(kr.VDEC_MUTANTS)
    m = vdec_model(5)
    res = _vdec_chain(m, kr.vdec_input(1, 5, kind), mutant)
    names = [n for n, _, _ in res]
    first = names.index(_VDEC_MUTANT_FIRST[mutant])
    print("vdec mutant %-16s %-6s caught at %-6s: worst |err| / bound %.3g   (before: %s)   (behind: %s)"
          % (mutant, kind, names[first], min(res[first][1], 9.99e99), "  ".join("%.3f" % r for _, r, _ in res[:first]),
             "  ".join("%s %.3g" % (n, min(r, 9.99e99)) for n, r, _ in res[first + 1:] if n.endswith("out"))))
    assert all(r <= 1.0 for _, r, _ in res[:first]), (mutant, [(n, r) for n, r, _ in res[:first] if r > 1.0])
    assert res[first][1] > 1.0, (mutant, res[first][1])
    if mutant == "stale_tile":
        assert all(r > 1.0 for n, r, _ in res if n.endswith("out"))


# ----------------------------------------------------------------------------------------------- condition side (rg_cond_kv)
@pytest.mark.parametrize("N,B,L,family", kr.COND_KV_RUNS, ids=["%d-%d-%d-%s" % r for r in kr.COND_KV_RUNS])
def test_cond_kv_emulation_inside_bound_and_mutants_outside(N, B, L, family):
    """Same cases, families and seeds as test_cond_kv_gpu.py.  The fp32 emulation of rg_cond_kv's rounding contract is inside
    the bound in every family; on the `grid` family (exact projection: the bound has no accumulation term) every wrong variant
    is outside it on every case it applies to.  The figures are printed; the module docstring of kernel_refs.py quotes them."""
    c = kr.cond_kv_case(N, B, L, family, kr.cond_kv_seed(N, B, L, family))
    A, bound = kr.cond_kv_ref(c)
    assert A.shape == (L, B, 16, 32, 32) and A.dtype == torch.float64 and torch.isfinite(bound).all()
    got = kr.cond_kv_emulate(c)
    r = kr.worst_ratio(got, A, bound)
    line = "cond_kv N=%d B=%d L=%d %s: emulation %.4f" % (N, B, L, family, r)
    assert torch.isfinite(got).all() and r <= 1.0, line
    if family == "zeros":       # K = b_K for every token: P = 1 / N, every row of A is the value bias
        want = c.bias.double()[:, None, 512:].view(L, 1, 16, 1, 32).expand_as(A)
        assert kr.worst_ratio(A, want, bound) <= 1.0 and kr.worst_ratio(got, want, bound) <= 1.0
    ratios = {m: kr.worst_ratio(kr.cond_kv_emulate(c, m), A, bound) for m in kr.COND_KV_MUTANTS if kr.cond_kv_mutant_applies(m, N, B, L)}
    print(line + "".join("  %s %.3g" % (m, min(v, 9.99e99)) for m, v in ratios.items()))
    if family == "grid":
        assert all(v > 1.0 for v in ratios.values()), ratios


def test_cond_kv_every_mutant_has_a_case_and_the_grid_projection_is_exact():
    for m in kr.COND_KV_MUTANTS:
        assert any(kr.cond_kv_mutant_applies(m, *c) for c in kr.COND_KV_CASES), m
    # the wave splits and packings the cases are chosen for: every wpc, a partly filled last workgroup, idle waves
    assert {kr.cond_kv_split(N)[0] for N, _, _ in kr.COND_KV_CASES} == set(range(1, 9))
    assert any(B % kr.cond_kv_split(N)[1] for N, B, _ in kr.COND_KV_CASES) and any(8 % kr.cond_kv_split(N)[0] for N, _, _ in kr.COND_KV_CASES)
    # `grid` inputs: the fp32 projection (any summation order: torch's matmul and the emulation's sixteen 32-deep steps) equals
    # the fp64 one bit for bit, and every value is a multiple of 2^-9 below 2^9
    c = kr.cond_kv_case(150, 3, 3, "grid", kr.cond_kv_seed(150, 3, 3, "grid"))
    x, w = c.xhat.float().view(-1, 512), c.w.float().view(-1, 512)
    kv64 = x.double() @ w.double().T + c.bias.double().view(1, -1)
    kv32 = x @ w.T + c.bias.view(1, -1)
    assert torch.equal(kv32.double(), kv64)
    assert torch.equal(kv64 * 512, torch.round(kv64 * 512)) and float(kv64.abs().max()) < 512
    stepped = kr._cond_project_f32(c, False).permute(1, 2, 0, 3).reshape(-1, 3 * 1024)
    assert torch.equal(stepped.double(), kv64)
    assert float(x.abs().max()) <= 4 and float(w.abs().max()) <= 0.125 and float(c.bias.abs().max()) <= 0.5
