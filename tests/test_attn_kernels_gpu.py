"""GPU: the per-op kernels of csrc/rg_attn.hip, one by one through the C ABI, against fp64 references on the CPU
(tests/kernel_refs.py: formulas, bounds and their derivation).  Every element of every output is compared; outputs are
allocated wider and longer than the kernel should write and the sentinel around the written region must survive bit for bit."""
import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def h(rg):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return rg.capi.get_handle(0)


def _refused(rg, h, name, *args):
    with pytest.raises(rg.capi.RgError):
        h.call(name, *args)
    return True


def _sa_masks(R, T):
    sep = torch.ones(R, T)
    sep[:, [10, 21, 32]] = 0
    one = torch.zeros(R, T)
    one[0, 0], one[1, T - 1], one[2, 17] = 1, 1, 1
    last = torch.ones(R, T)
    last[:, T - 1] = 0
    full = sep.clone()
    full[1] = 0
    return {"ones": torch.ones(R, T), "separators": sep, "one valid token": one, "last token masked": last, "row 1 fully masked": full}


def _perm(n, seed, device="cuda"):
    """A shuffled work list with interleaved -1 (idle) entries."""
    g = kr.rng(seed)
    items = g.permutation(n).tolist()
    out = []
    for i, it in enumerate(items):
        if i % 3 == 0:
            out.append(-1)
        out.append(it)
    out.append(-1)
    return torch.tensor(out, dtype=torch.int32, device=device)


@pytest.mark.parametrize("T", [33, 40, 43, 48, 49, 57, 64])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_sa_attention(rg, h, parity, mode, T):
    R, D = 3, 256
    G = D // 128
    ldqkv, ldy = 3 * D + 8, D + 8
    qkv = kr.randn((R * T, ldqkv), 1000 + T)
    qkv[:, :D] = kr.softmax_heads(qkv[:, :D], D)
    qd = qkv.cuda()
    rows = R * T + 2
    if mode == 2 and T > 48:
        y = torch.zeros(rows, ldy, dtype=torch.int16, device="cuda")
        st = torch.zeros(R * T, G, 2, device="cuda")
        assert _refused(rg, h, "sa_attention", qd, ldqkv, torch.ones(R, T, device="cuda"), y, ldy, st, R, T, D, None, 0, 2)
        return
    worst_y = worst_s = worst_u = 0.0
    for name, mask in _sa_masks(R, T).items():
        if name == "last token masked" and T % 8 == 0:
            continue
        before = kr.canary(rows, ldy, torch.int16 if mode == 2 else torch.float32)
        y = before.cuda()
        st = torch.full((R * T + 1, G, 2), float("nan"), device="cuda")
        h.call("sa_attention", qd, ldqkv, mask.cuda(), y, ldy, st, R, T, D, None, 0, mode)
        torch.cuda.synchronize()
        yc, sc = y.cpu(), st.cpu()
        assert kr.untouched(yc, before, R * T, 0, D), (mode, T, name)
        assert torch.isnan(sc[R * T]).all()
        ref, e = kr.sa_ref(qkv, mask, R, T, D, mode != 0)
        got = kr.from_bf16_bits(yc[:R * T, :D]) if mode == 2 else yc[:R * T, :D]
        by, by_ulp = kr.bf16_bounds(ref, e) if mode == 2 else (e, e)
        ry, ru = kr.worst_ratio(got, ref, by), kr.worst_ratio(got, ref, by_ulp)
        rs = kr.worst_ratio(sc[:R * T], kr.group_stats(ref, 128), kr.group_stats_bound(ref, e, 128))
        print("sa_attention mode %d T=%d mask=%s: y %.3f stats %.3f" % (mode, T, name, ry, rs))
        assert torch.isfinite(got).all() and torch.isfinite(sc[:R * T]).all(), (mode, T, name)
        if name == "row 1 fully masked":
            assert (got.view(R, T, D)[1] == 0).all() and (sc[:R * T].view(R, T, G, 2)[1] == 0).all()
        worst_y, worst_s, worst_u = max(worst_y, ry), max(worst_s, rs), max(worst_u, ru)
        if name == "separators":      # perm: shuffled work list with idle blocks, same bits
            perm = _perm(R * G, 7 + T)
            y2, st2 = before.cuda(), torch.full_like(st, float("nan"))
            h.call("sa_attention", qd, ldqkv, mask.cuda(), y2, ldy, st2, R, T, D, perm, perm.numel(), mode)
            torch.cuda.synchronize()
            assert torch.equal(y2.cpu().view(torch.int16), yc.view(torch.int16))
            assert torch.equal(st2.cpu()[:R * T], sc[:R * T])
    parity.check("rg_sa_attention mode %d T=%d: stats, worst |err| / bound over all masks" % (mode, T), worst_s, 1.0)
    if mode == 2:
        parity.check("rg_sa_attention mode 2 T=%d: bf16 y within half a bf16 ulp of the fp32 bound" % T, worst_u, 1.0)
    parity.check("rg_sa_attention mode %d T=%d: y, worst |err| / bound over all masks" % (mode, T), worst_y, 1.0)


@pytest.mark.parametrize("T", [43, 64, 5])
@pytest.mark.parametrize("Rc", [4, 2, 0])
def test_ca_attention(rg, h, parity, Rc, T):
    R, D, nc = 4, 256, 3
    H, G = D // 32, D // 128
    q3 = kr.softmax_heads(kr.randn((R * T, nc * D), 2000 + T), nc * D)
    Apre, Aunc = kr.randn((nc, max(Rc, 1), H, 32, 32), 2001, 0.3), kr.randn((nc, H, 32, 32), 2002, 0.3)
    qm = torch.ones(nc, R, T)
    for c, r in ((0, 1), (2, 3), (1, 0)):
        qm[c, r, [t for t in (10, 20, 30) if t < T] or [T - 1]] = 0
    worst_y = worst_s = 0.0
    ties = 0
    for qmask in (None, qm):
        before = kr.canary(R * T + 2, nc * D)
        y = before.cuda()
        st = torch.full((nc * R * T + 1, G, 2), float("nan"), device="cuda")
        args = (q3.cuda(), Apre.cuda(), Aunc.cuda(), None if qmask is None else qmask.cuda())
        h.call("ca_attention", *args, y, st, R, Rc, T, D, nc, None, 0)
        torch.cuda.synchronize()
        yc, sc = y.cpu(), st.cpu()
        assert kr.untouched(yc, before, R * T, 0, nc * D) and torch.isnan(sc[nc * R * T]).all()
        ref, e, tie = kr.ca_ref(q3, Apre[:, :Rc], Aunc, qmask, R, Rc, T, D, nc)
        got = yc[:R * T]
        if qmask is not None:
            msk = (qmask == 0).permute(1, 2, 0).reshape(R * T, nc, 1).expand(R * T, nc, D).reshape(R * T, nc * D)
            assert torch.equal(got[msk] * 16, torch.round(got[msk] * 16))        # exact multiples of 1/16
            exact = msk & ~tie
            assert torch.equal(got[exact].double(), ref[exact])                  # == the fp64 y rounded to the grid
            ties += int(tie.sum())
        worst_y = max(worst_y, kr.worst_ratio(got, ref, e))
        sref = kr.group_stats(ref.view(R * T, nc, D).permute(1, 0, 2), 128)       # [nc, R*T, G, 2]
        sb = kr.group_stats_bound(ref.view(R * T, nc, D).permute(1, 0, 2), e.view(R * T, nc, D).permute(1, 0, 2), 128)
        worst_s = max(worst_s, kr.worst_ratio(sc[:nc * R * T].view(nc, R * T, G, 2), sref, sb))
        perm = _perm(R * nc * G, 11 + T)
        y2, st2 = before.cuda(), torch.full_like(st, float("nan"))
        h.call("ca_attention", *args, y2, st2, R, Rc, T, D, nc, perm, perm.numel())
        torch.cuda.synchronize()
        assert torch.equal(y2.cpu().view(torch.int32), yc.view(torch.int32)) and torch.equal(st2.cpu()[:-1], sc[:-1])
    print("ca_attention Rc=%d T=%d: %d masked elements within their bound of a rounding tie" % (Rc, T, ties))
    parity.check("rg_ca_attention Rc=%d T=%d: y (1/16 grid on masked rows), worst |err| / bound" % (Rc, T), worst_y, 1.0)
    parity.check("rg_ca_attention Rc=%d T=%d: stats, worst |err| / bound" % (Rc, T), worst_s, 1.0)


@pytest.mark.parametrize("N", [1, 7, 8, 9, 77, 499])
def test_kv_reduce(rg, h, parity, N):
    B, D = 2, 128
    H = D // 32
    kv = kr.randn((B * N, 2 * D + 4), 3000 + N)
    kv[:, 5] = torch.from_numpy(kr.rng(3100 + N).uniform(-80, 80, B * N)).float()      # a key column with a large spread
    before = kr.canary(B * H * 32 + 3, 32)
    A = before.cuda()
    h.call("kv_reduce", kv.cuda(), 2 * D + 4, A, B, N, D)
    torch.cuda.synchronize()
    assert kr.untouched(A, before, B * H * 32, 0, 32)
    ref, bound = kr.kv_reduce_ref(kv, B, N, D)
    parity.check("rg_kv_reduce N=%d: A, worst |err| / bound" % N, kr.worst_ratio(A.cpu()[:B * H * 32].view(B, H, 32, 32), ref, bound), 1.0)


def test_split_transpose_bf16_is_exact(rg, h):
    n = 5
    A = kr.randn((n, 32, 32), 4000)
    before = kr.canary(n * 2 * 32 + 2, 32, torch.int16)
    At = before.cuda()
    h.call("split_transpose_bf16", A.cuda(), At, n)
    torch.cuda.synchronize()
    assert kr.untouched(At, before, n * 2 * 32, 0, 32)
    got = At.cpu()[:n * 2 * 32].view(n, 2, 32, 32)
    hi = A.transpose(1, 2).to(torch.bfloat16)
    lo = (A.transpose(1, 2) - hi.float()).to(torch.bfloat16)
    assert torch.equal(got[:, 0], hi.view(torch.int16)) and torch.equal(got[:, 1], lo.view(torch.int16))


@pytest.mark.parametrize("dim", [64, 512])
def test_row_stats(rg, h, parity, dim):
    rows = 5
    x = kr.randn((rows, dim), 5000 + dim)
    st = torch.full((rows + 1, dim // 64, 2), float("nan"), device="cuda")
    h.call("row_stats", x.cuda(), st, rows, dim)
    torch.cuda.synchronize()
    assert torch.isnan(st[rows]).all()
    xd = x.double()
    r = kr.worst_ratio(st.cpu()[:rows], kr.group_stats(xd, 64), kr.group_stats_bound(xd, torch.zeros_like(xd), 64))
    parity.check("rg_row_stats dim=%d: worst |err| / bound" % dim, r, 1.0)


@pytest.mark.parametrize("K", [1, 63, 64, 65, 512])
def test_linear_f32(rg, h, parity, K):
    M, N = 3, 5
    a, w, bias = kr.randn((M, K), 6000 + K), kr.randn((N, K), 6001 + K), kr.randn((N,), 6002)
    silu = lambda t: t * torch.sigmoid(t)
    worst = 0.0
    for si in (0, 1):
        for so in (0, 1):
            for b in (None, bias):
                before = kr.canary(M + 2, N)
                out = before.cuda()
                h.call("linear_f32", a.cuda(), w.cuda(), None if b is None else b.cuda(), out, M, N, K, si, so)
                torch.cuda.synchronize()
                assert kr.untouched(out, before, M, 0, N)
                x = silu(a.double()) if si else a.double()
                acc = x @ w.double().T + (b.double() if b is not None else 0.0)
                mag = x.abs() @ w.double().abs().T + (b.double().abs() if b is not None else 0.0)
                # K-term dot product of inputs that carry 4 U each (the input SiLU), a bias add, an output SiLU (slope <= 1.1)
                e = ((K + 1 + 4 * si) * kr.U) * mag
                ref = silu(acc) if so else acc
                bound = kr.MARGIN * ((1.1 * e + 4 * kr.U * ref.abs()) if so else e)
                worst = max(worst, kr.worst_ratio(out.cpu()[:M], ref, bound))
    parity.check("rg_linear_f32 K=%d: all SiLU flag pairs, bias on / off, worst |err| / bound" % K, worst, 1.0)


@pytest.mark.parametrize("dim", [4, 512])
def test_gather_rows_is_exact(rg, h, dim):
    table = kr.randn((9, dim), 7000 + dim)
    idx = torch.tensor([8, 0, 3, 3, 7, 1, 0, 8], dtype=torch.int64)
    before = kr.canary(idx.numel() + 2, dim)
    out = before.cuda()
    h.call("gather_rows", table.cuda(), idx.cuda(), out, idx.numel(), dim)
    torch.cuda.synchronize()
    assert kr.untouched(out, before, idx.numel(), 0, dim)
    assert torch.equal(out.cpu()[:idx.numel()], table[idx])


def _bf16_tab(shape, seed):
    """A table of bf16 rows as int16 bit patterns."""
    return kr.bf16_bits(kr.randn(shape, seed))


@pytest.mark.parametrize("T", [43, 8])
@pytest.mark.parametrize("Ru", [0, 3])
def test_ca_stylize(rg, h, parity, Ru, T):
    """rg_split_transpose_bf16 -> rg_ca_stylize / rg_ca_stylize_groups: Q A, the 1/16 rounding on masked query rows, LayerNorm,
    * (1 + scale) + shift, SiLU, bf16 on the conditional row groups; the classifier-free row groups are the table row of the
    right flag and the right step group, bit for bit."""
    Rc, D, nc = 3, 512, 3
    H, R, ldo = D // 32, Rc + Ru, nc * D + 8
    q3 = kr.softmax_heads(kr.randn((Rc * T, nc * D), 8000 + T), nc * D)
    A = kr.randn((nc, Rc, H, 32, 32), 8001, 0.3)
    gamma, beta = 1 + 0.2 * kr.randn((nc, D), 8002), 0.2 * kr.randn((nc, D), 8003)
    ss_a, ss_b = kr.randn((nc, 2 * D), 8004, 0.3), kr.randn((nc, 2 * D), 8005, 0.3)
    tab_a, tab_b = _bf16_tab((2, nc * D), 8006), _bf16_tab((2, nc * D), 8007)
    qm = torch.ones(nc, R, T)
    for c, r in ((0, 1), (2, 0), (1, 2), (0, R - 1), (2, R - 1)):
        qm[c, r, [t for t in (10, 20, 30) if t < T] or [1, T - 1]] = 0
    # the hi / lo planes, computed by the kernel under test and checked exactly against their definition
    At = torch.zeros(nc * Rc * H, 2, 32, 32, dtype=torch.int16, device="cuda")
    h.call("split_transpose_bf16", A.cuda(), At, nc * Rc * H)
    torch.cuda.synchronize()
    assert torch.equal(At.cpu(), kr.split_transpose_ref(A.view(-1, 32, 32)))
    dev = dict(q3=q3.cuda(), g=gamma.cuda(), b=beta.cuda(), ss_a=ss_a.cuda(), ss_b=ss_b.cuda(), tab_a=tab_a.cuda(), tab_b=tab_b.cuda())
    worst = worst_u = 0.0
    ties = 0
    for qmask in (None, qm):
        for split in (None, 0, 1, 2, 3):
            before = kr.canary(R * T + 2, ldo, torch.int16)
            out = before.cuda()
            qd = None if qmask is None else qmask.cuda()
            tab = dev["tab_a"] if Ru else None
            if split is None:
                h.call("ca_stylize", dev["q3"], At, qd, dev["g"], dev["b"], dev["ss_a"], tab, out, ldo, Rc, Ru, T, D, nc)
                sp = R
            else:
                h.call("ca_stylize_groups", dev["q3"], At, qd, dev["g"], dev["b"], dev["ss_a"], tab, out, ldo, Rc, Ru, T, D, nc,
                       dev["ss_b"], dev["tab_b"] if Ru else None, split)
                sp = split
            torch.cuda.synchronize()
            oc = out.cpu()
            assert kr.untouched(oc, before, R * T, 0, nc * D), (Ru, T, split)
            ss_rows = torch.stack([ss_b if r >= sp else ss_a for r in range(Rc)])
            ref, e, nt = kr.ca_stylize_ref(q3, A, None if qmask is None else qmask[:, :Rc].contiguous(), gamma, beta, ss_rows, Rc, T, D, nc)
            ties += nt
            got = kr.from_bf16_bits(oc[:Rc * T, :nc * D])
            assert torch.isfinite(got).all()
            bm, bu = kr.bf16_bounds(ref, e)
            worst, worst_u = max(worst, kr.worst_ratio(got, ref, bm)), max(worst_u, kr.worst_ratio(got, ref, bu))
            for u in range(Ru):      # classifier-free row groups: the table row of the right flag and step group, bit for bit
                t_ = tab_b if u >= sp else tab_a
                flag = torch.zeros(T, nc, dtype=torch.long) if qmask is None else (qmask[:, Rc + u] == 0).long().T
                exp = torch.stack([t_[flag[:, c], c * D:(c + 1) * D] for c in range(nc)], dim=1).reshape(T, nc * D)
                assert torch.equal(oc[(Rc + u) * T:(Rc + u + 1) * T, :nc * D], exp), (Ru, T, split, u)
    print("ca_stylize Ru=%d T=%d: %d masked elements within their bound of a rounding tie" % (Ru, T, ties))
    parity.check("rg_ca_stylize(_groups) Ru=%d T=%d: bf16 out within half a bf16 ulp of the fp32 bound" % (Ru, T), worst_u, 1.0)
    parity.check("rg_ca_stylize(_groups) Ru=%d T=%d: qmask on / off, all splits, worst |err| / bound" % (Ru, T), worst, 1.0)


@pytest.mark.parametrize("seg_len", [512, 64])
@pytest.mark.parametrize("unc_nseg", [0, 3])
def test_stylize(rg, h, parity, unc_nseg, seg_len):
    """rg_stylize / rg_stylize_groups: IDENT, LN and two STYL segments in one call (statistics in 1, 4 and 8 parts), M = 18 rows
    = [2 halves][3 sequences][3 tokens] (not a multiple of the 4 rows of a workgroup), classifier-free rows [9, 18) from the
    table for the first unc_nseg segments, and the two-step split."""
    import ctypes
    G = __import__("importlib").import_module("rag-gesture_amd.gemm")
    T, nseq, nseg = 3, 3, 4
    M, m_cond = 2 * nseq * T, nseq * T
    ld, ldo = seg_len + 4, nseg * seg_len + 8
    modes, nparts = (G.A_IDENT, G.A_LN, G.A_STYL, G.A_STYL), (1, 1, 4, 8)
    src = [kr.randn((M, ld), 9000 + s + seg_len) * (1.0 + s) + 0.3 * s for s in range(nseg)]
    gam = [1 + 0.2 * kr.randn((seg_len,), 9010 + s) for s in range(nseg)]
    bet = [0.2 * kr.randn((seg_len,), 9020 + s) for s in range(nseg)]
    ss_a = [kr.randn((2 * seg_len,), 9030 + s, 0.3) for s in range(nseg)]
    ss_b = [kr.randn((2 * seg_len,), 9040 + s, 0.3) for s in range(nseg)]
    # the statistics are inputs: fp64 partial sums rounded to fp32 (U each; the kernel adds the nparts of them: depth nparts + 1)
    stats = [kr.group_stats(x[:, :seg_len].double(), seg_len // p).float() for x, p in zip(src, nparts)]
    tab = _bf16_tab((2, max(unc_nseg, 1) * seg_len), 9050)
    qm = torch.ones(nseg, M)
    qm[0, 10], qm[2, 10], qm[1, 17], qm[0, 2] = 0, 0, 0, 0
    keep = [t.cuda() for t in src + gam + bet + ss_a + ss_b + stats] + [tab.cuda(), qm.cuda()]
    dsrc, dgam, dbet, dssa, dssb, dst = (keep[i * nseg:(i + 1) * nseg] for i in range(6))
    segs = (G.ASegment * G.MAX_SEG)()
    for s in range(nseg):
        segs[s].src, segs[s].ld, segs[s].mode = dsrc[s].data_ptr(), ld, modes[s]
        if modes[s] != G.A_IDENT:
            segs[s].stats, segs[s].nparts, segs[s].gamma, segs[s].beta = dst[s].data_ptr(), nparts[s], dgam[s].data_ptr(), dbet[s].data_ptr()
        if modes[s] == G.A_STYL:
            segs[s].scale_shift = dssa[s].data_ptr()
    worst = worst_u = 0.0
    for qmask in (None, qm):
        for split in (None, 1, 2, nseq):
            before = kr.canary(M + 2, ldo, torch.int16)
            out = before.cuda()
            fixed = (ctypes.byref(segs), nseg, seg_len, M, out, ldo, m_cond, unc_nseg, keep[-2] if unc_nseg else None,
                     None if qmask is None else keep[-1])
            if split is None:
                h.call("stylize", *fixed)
                sp = nseq
            else:
                h.call("stylize_groups", *fixed, (ctypes.c_void_p * nseg)(*[t.data_ptr() for t in dssb]), T, nseq, split)
                sp = split
            torch.cuda.synchronize()
            oc = out.cpu()
            assert kr.untouched(oc, before, M, 0, nseg * seg_len), (seg_len, unc_nseg, split)
            rows_b = torch.tensor([(r // T) % nseq >= sp for r in range(M)])
            for s in range(nseg):
                blk = oc[:M, s * seg_len:(s + 1) * seg_len]
                rows = list(range(m_cond if s < unc_nseg else M))
                if s < unc_nseg:      # classifier-free rows: the table row of the right flag, bit for bit
                    flag = torch.zeros(M, dtype=torch.long) if qmask is None else (qmask[s] == 0).long()
                    assert torch.equal(blk[m_cond:], tab[flag[m_cond:], s * seg_len:(s + 1) * seg_len]), (s, split)
                x = src[s][rows, :seg_len].double()
                if modes[s] == G.A_IDENT:
                    assert torch.equal(blk[rows], kr.bf16_bits(src[s][rows, :seg_len]))
                    continue
                if modes[s] == G.A_LN:
                    ref, e = kr.styl_ref(x, 0.0, gam[s].double(), bet[s].double(), None, None, nparts[s] + 1)
                else:
                    ss = torch.stack([ss_b[s] if rows_b[r] else ss_a[s] for r in rows]).double()
                    ref, e = kr.styl_ref(x, 0.0, gam[s].double(), bet[s].double(), ss[:, :seg_len], ss[:, seg_len:], nparts[s] + 1)
                got = kr.from_bf16_bits(blk[rows])
                bm, bu = kr.bf16_bounds(ref, e)
                worst, worst_u = max(worst, kr.worst_ratio(got, ref, bm)), max(worst_u, kr.worst_ratio(got, ref, bu))
    tag = "seg_len=%d unc_nseg=%d" % (seg_len, unc_nseg)
    parity.check("rg_stylize(_groups) %s: LN / STYL out within half a bf16 ulp of the fp32 bound" % tag, worst_u, 1.0)
    parity.check("rg_stylize(_groups) %s: LN / STYL segments, all splits, worst |err| / bound" % tag, worst, 1.0)
