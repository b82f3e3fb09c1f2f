"""CPU: the bounds of tests/kernel_refs.py, checked before any kernel runs.  A float32 / bf16 emulation of each kernel's
rounding contract must stay inside the bounds against the fp64 reference (loose enough for a correct kernel), and deliberately
wrong variants -- a dropped probability column, statistics of the neighbouring head group, a one-pass variance -- must exceed them (tight
enough to fail on a subtle error).  Same seeds and shapes as the GPU tests."""
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
