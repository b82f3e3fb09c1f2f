"""GPU: the per-op kernels of csrc/rg_vae.hip, one by one through the C ABI, against fp64 references on the CPU
(tests/kernel_refs.py: formulas, bounds and their derivation).  Every element of every output is compared; outputs are
allocated wider and longer than the kernel should write and the sentinel around the written region must survive bit for bit."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import kernel_refs as kr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def h(rg):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return rg.capi.get_handle(0)


def _qkv(B, H, hd, Sq, Sk, seed, qscale=1.0):
    """q, k, v as column slices of one [rows, 3*H*hd + 8] tensor (how the product passes them)."""
    ld = 3 * H * hd + 8
    x = kr.randn((B * max(Sq, Sk), ld), seed)
    x[:, :H * hd] *= qscale
    return x, ld


def _slices(xd, H, hd):
    return xd[:, :H * hd], xd[:, H * hd:2 * H * hd], xd[:, 2 * H * hd:3 * H * hd]


def _ptr(t, col):
    return t.data_ptr() + 4 * col


@pytest.mark.parametrize("hd", [16, 32, 64, 128])
def test_mha_fp32(rg, h, parity, hd):
    B, H = 2, 3
    ldo = H * hd + 8
    worst = 0.0
    for Sk, Sq in [(sk, sq) for sk in (1, 17, 64, 65, 160, 192) for sq in (1, 31, 33, 160)] + [(154, 17)]:
        x, ld = _qkv(B, H, hd, Sq, Sk, 100 * hd + Sk + Sq)
        xd = x.cuda()
        before = kr.canary(B * Sq + 2, ldo)
        o = before.cuda()
        if (Sk * (2 * hd + 5) + 4 * hd) * 4 > 160 * 1024:      # K / V of one head do not fit LDS (hd = 128: Sk <= 154): refused
            with pytest.raises(rg.capi.RgError):
                h.call("mha", _ptr(xd, 0), ld, _ptr(xd, H * hd), ld, _ptr(xd, 2 * H * hd), ld, o, ldo, B, H, Sq, Sk, hd)
            continue
        h.call("mha", _ptr(xd, 0), ld, _ptr(xd, H * hd), ld, _ptr(xd, 2 * H * hd), ld, o, ldo, B, H, Sq, Sk, hd)
        torch.cuda.synchronize()
        assert kr.untouched(o, before, B * Sq, 0, H * hd), (hd, Sk, Sq)
        q, k, v = _slices(x, H, hd)
        ref, bound = kr.mha_ref(q[:B * Sq], k[:B * Sk], v[:B * Sk], B, H, Sq, Sk, hd, False)
        worst = max(worst, kr.worst_ratio(o.cpu()[:B * Sq, :H * hd], ref, bound))
    parity.check("rg_mha (fp32) hd=%d: Sk in 1..192, Sq in 1..160, worst |err| / bound" % hd, worst, 1.0)
    with pytest.raises(rg.capi.RgError):
        h.call("mha", _ptr(xd, 0), ld, _ptr(xd, H * hd), ld, _ptr(xd, 2 * H * hd), ld, o, ldo, B, H, 1, 193, hd)


def _mha_bf16_case(h, parity, hd, Sq, Sk, out_bf16, seed, qscale=1.0, grouped_n=0):
    B, H = 2, 3
    ldo = H * hd + 8
    x, ld = _qkv(B, H, hd, Sq, Sk, seed, qscale)
    xd = x.cuda()
    before = kr.canary(B * Sq + 2, ldo, torch.int16 if out_bf16 else torch.float32)
    o = before.cuda()
    h.call("mha_bf16", _ptr(xd, 0), ld, _ptr(xd, H * hd), ld, _ptr(xd, 2 * H * hd), ld, o, ldo, int(out_bf16), B, H, Sq, Sk, hd)
    torch.cuda.synchronize()
    oc = o.cpu()
    assert kr.untouched(oc, before, B * Sq, 0, H * hd), (hd, Sq, Sk, out_bf16)
    q, k, v = _slices(x, H, hd)
    ref, e = kr.mha_ref(q[:B * Sq], k[:B * Sk], v[:B * Sk], B, H, Sq, Sk, hd, True)
    got = kr.from_bf16_bits(oc[:B * Sq, :H * hd]) if out_bf16 else oc[:B * Sq, :H * hd]
    bound, b_ulp = kr.bf16_bounds(ref, e) if out_bf16 else (e, e)
    r = kr.worst_ratio(got, ref, bound)
    assert kr.worst_ratio(got, ref, b_ulp) <= 1.0, (hd, Sq, Sk, out_bf16)     # within half a bf16 ulp of the fp32 bound
    if grouped_n:      # the grouped launch of n problems == the single calls, bit for bit
        xs = [xd] + [kr.randn(tuple(x.shape), seed + 10 + i).cuda() for i in range(1, grouped_n)]
        singles, outs = [oc], [before.cuda() for _ in range(grouped_n)]
        for xi in xs[1:]:
            oi = before.cuda()
            h.call("mha_bf16", _ptr(xi, 0), ld, _ptr(xi, H * hd), ld, _ptr(xi, 2 * H * hd), ld, oi, ldo, int(out_bf16), B, H, Sq, Sk, hd)
            singles.append(oi.cpu())
        arr = lambda ps: (ctypes.c_void_p * grouped_n)(*ps)
        h.call("mha_bf16_grouped", grouped_n, arr([_ptr(t, 0) for t in xs]), ld, arr([_ptr(t, H * hd) for t in xs]), ld,
               arr([_ptr(t, 2 * H * hd) for t in xs]), ld, arr([t.data_ptr() for t in outs]), ldo, int(out_bf16), B, H, Sq, Sk, hd)
        torch.cuda.synchronize()
        view = torch.int16 if out_bf16 else torch.int32
        for a, b in zip(outs, singles):
            assert torch.equal(a.cpu().view(view), b.view(view)), (hd, Sq, Sk, grouped_n)
    return r


@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("hd", [128, 64, 32, 16])
def test_mha_bf16(rg, h, parity, hd, out_bf16):
    worst = 0.0
    n = 0
    for Sq in (1, 15, 16, 17, 63, 65):
        for Sk in (1, 17, 31, 32, 33, 160, 192):
            n += 1
            g = 1 + (n % 4) if (Sq in (17, 65) and Sk in (33, 192)) else 0
            worst = max(worst, _mha_bf16_case(h, parity, hd, Sq, Sk, out_bf16, 1000 * hd + 10 * Sq + Sk, grouped_n=g))
    tag = "bf16" if out_bf16 else "fp32"
    r = _mha_bf16_case(h, parity, hd, 17, 33, out_bf16, 77 + hd, qscale=60.0 / hd ** 0.5)
    parity.check("rg_mha_bf16 hd=%d, %s out: score magnitudes near 60, worst |err| / bound" % (hd, tag), r, 1.0)
    parity.check("rg_mha_bf16 hd=%d, %s out: Sq 1..65 x Sk 1..192 (+ grouped == single), worst |err| / bound" % (hd, tag), worst, 1.0)


@pytest.mark.parametrize("out_bf16", [False, True])
def test_mha_bf16_512_key_variant(rg, h, parity, out_bf16):
    worst = 0.0
    for i, Sk in enumerate((193, 499, 512)):
        for Sq in (1, 15, 16, 17, 63, 65):
            worst = max(worst, _mha_bf16_case(h, parity, 64, Sq, Sk, out_bf16, 9000 + Sk + Sq, grouped_n=(2 + i) if Sq == 17 else 0))
    parity.check("rg_mha_bf16 hd=64, Sk in {193, 499, 512}, %s out: worst |err| / bound" % ("bf16" if out_bf16 else "fp32"), worst, 1.0)


def test_mha_bf16_refusals(rg, h):
    x = torch.zeros(2 * 193, 3 * 3 * 48 + 8, device="cuda")
    o = torch.zeros(2 * 4, 3 * 48 + 8, device="cuda")
    for hd, Sk in ((32, 193), (48, 17), (128, 193), (64, 513)):
        with pytest.raises(rg.capi.RgError):
            h.call("mha_bf16", x, x.shape[1], x, x.shape[1], x, x.shape[1], o, o.shape[1], 0, 2, 3, 4, Sk, hd)


@pytest.mark.parametrize("dim", [61, 64, 512, 768])
@pytest.mark.parametrize("rows", [1, 5])
def test_layernorm(rg, h, parity, rows, dim):
    x, res = kr.randn((rows, dim), 200 + dim), kr.randn((rows, dim), 201 + dim)
    x[rows - 1] += 1000.0                     # mean 1e3, unit spread: the two-pass variance must survive it
    g, b = 1 + 0.2 * kr.randn((dim,), 202), 0.2 * kr.randn((dim,), 203)
    xd, rd, gd, bd = x.cuda(), res.cuda(), g.cuda(), b.cuda()
    worst = 0.0
    cases = [("layernorm", None, 1e-5, w16) for w16 in (False, True)]
    cases += [("layernorm_res", r, eps, w16) for r in (None, res) for eps in (1e-12, 1e-5) for w16 in (False, True)]
    for name, r, eps, w16 in cases:
        before, before16 = kr.canary(rows + 2, dim), kr.canary(rows + 2, dim, torch.int16)
        out, o16 = before.cuda(), before16.cuda()
        if name == "layernorm":
            h.call("layernorm", xd, gd, bd, out, rows, dim, o16 if w16 else None)
        else:
            h.call("layernorm_res", xd, None if r is None else rd, gd, bd, out, rows, dim, eps, o16 if w16 else None)
        torch.cuda.synchronize()
        oc = out.cpu()
        assert kr.untouched(oc, before, rows, 0, dim)
        assert kr.untouched(o16, before16, rows if w16 else 0, 0, dim)
        if w16:
            assert torch.equal(o16.cpu()[:rows], kr.bf16_bits(oc[:rows]))          # the bf16 copy == bf16(out) exactly
        ref, bound = kr.layernorm_ref(x, r, g, b, eps)
        worst = max(worst, kr.worst_ratio(oc[:rows], ref, bound))
    parity.check("rg_layernorm / rg_layernorm_res rows=%d dim=%d: worst |err| / bound" % (rows, dim), worst, 1.0)


def test_add_rows_copy_rows_copy_cols_are_exact(rg, h):
    I64 = rg.capi.I64
    # add_rows: period < n and period == n
    a, b = kr.randn((6, 40), 300), kr.randn((2, 40), 301)
    for bb, period in ((b, 80), (kr.randn((6, 40), 302), 240)):
        before = kr.canary(7, 40)
        out = before.cuda()
        h.call("add_rows", a.cuda(), bb.cuda(), out, I64(240), I64(period))
        torch.cuda.synchronize()
        assert kr.untouched(out, before, 6, 0, 40)
        assert torch.equal(out.cpu()[:6], a + bb.repeat(240 // period, 1))
    # copy_rows: [groups, rows_src_per, dim] -> [groups, rows_dst_per, dim], and the rows_src_per = 0 broadcast
    G, dim = 3, 12
    src, dst0 = kr.randn((G, 5, dim), 303), kr.randn((G, 7, dim), 304)
    dst = dst0.cuda()
    h.call("copy_rows", src.cuda(), dst, G, 2, dim, 5, 3, 7, 4)
    exp = dst0.clone()
    exp[:, 4:6] = src[:, 3:5]
    assert torch.equal(dst.cpu(), exp)
    dst = dst0.cuda()
    h.call("copy_rows", src.cuda(), dst, G, 2, dim, 0, 1, 7, 0)
    exp = dst0.clone()
    exp[:, 0:2] = src[0, 1:3]
    assert torch.equal(dst.cpu(), exp)
    # copy_cols: plain, and columns 0 / 2 relative to the first frame of each 15-frame clip
    rows, frames = 30, 15
    for ncols in (3, 40):
        s, d0 = kr.randn((rows, ncols + 5), 305 + ncols), kr.randn((rows + 1, ncols + 9), 306)
        for fr, mask in ((frames, 0b101), (0, 0b101), (frames, 0)):
            d = d0.cuda()
            h.call("copy_cols", s.cuda(), ncols + 5, 2, d, ncols + 9, 4, rows, ncols, fr, mask)
            exp = d0.clone()
            blk = s[:, 2:2 + ncols].clone()
            if fr > 0:
                for c in range(min(ncols, 32)):
                    if (mask >> c) & 1:
                        blk[:, c] = blk[:, c] - s.view(rows // fr, fr, -1)[:, :1, 2 + c].expand(-1, fr).reshape(rows)
            exp[:rows, 4:4 + ncols] = blk
            assert torch.equal(d.cpu(), exp), (ncols, fr, mask)


def test_vae_reparam_and_cached(rg, h, parity):
    E, nch, D, seq = 3, 4, 64, 5
    T = 4 * nch + 3
    slots = [2, 0, 1]
    cache_rows = 3 * 4 * nch
    mu, lv = kr.randn((cache_rows, D), 400), kr.randn((cache_rows, D), 401, 0.5)
    eps = [kr.randn((E * nch, D), 402 + p) for p in range(4)]
    lat = torch.full((E + 1, T, D), float("nan"), device="cuda")
    h.call("vae_reparam_cached", mu.cuda(), lv.cuda(), torch.tensor(slots, dtype=torch.int32, device="cuda"),
           *[e.cuda() for e in eps], lat, E, nch, D, cache_rows)
    torch.cuda.synchronize()
    got = lat.cpu()
    assert torch.isnan(got[E]).all()
    ref = torch.zeros(E, T, D, dtype=torch.float64)
    mag = torch.zeros(E, T, D, dtype=torch.float64)
    for e in range(E):
        for p in range(4):
            r = slots[e] * 4 * nch + p * nch
            sd = torch.exp(lv[r:r + nch].double()) ** 0.5
            ref[e, p * (nch + 1):p * (nch + 1) + nch] = mu[r:r + nch].double() + sd * eps[p][e * nch:(e + 1) * nch].double()
            mag[e, p * (nch + 1):p * (nch + 1) + nch] = mu[r:r + nch].double().abs() + (sd * eps[p][e * nch:(e + 1) * nch].double()).abs() * (1 + lv[r:r + nch].double().abs())
    # expf (2 U, argument error U |logvar|), sqrtf, a product and a sum: 8 U of the magnitudes
    bound = kr.MARGIN * 8 * kr.U * mag
    for s in (nch, 2 * nch + 1, 3 * nch + 2):
        assert (got[:E, s] == 0).all()
    parity.check("rg_vae_reparam_cached: worst |err| / bound", kr.worst_ratio(got[:E], ref, bound), 1.0)
    # rg_vae_reparam on the same posteriors (enc [B*n_chunks, seq, D], tokens 0 / 1 = mu / logvar), one part at a time
    lat2 = torch.full((E, T, D), float("nan"), device="cuda")
    for p in range(4):
        enc = kr.randn((E * nch, seq, D), 410 + p)
        for e in range(E):
            r = slots[e] * 4 * nch + p * nch
            enc[e * nch:(e + 1) * nch, 0], enc[e * nch:(e + 1) * nch, 1] = mu[r:r + nch], lv[r:r + nch]
        h.call("vae_reparam", enc.cuda(), seq, eps[p].cuda(), lat2, E, nch, D, T, p * (nch + 1))
    torch.cuda.synchronize()
    got2 = lat2.cpu()
    keep = [t for t in range(T) if t not in (nch, 2 * nch + 1, 3 * nch + 2)]
    assert torch.equal(got2[:, keep], got[:E, keep])                   # both kernels agree bit for bit
    assert torch.isnan(got2[:, [nch, 2 * nch + 1, 3 * nch + 2]]).all()  # rows outside the written blocks are untouched
    # a slot outside the cache: NaN rows (documented, safe), separators zero, neighbours intact
    lat3 = torch.full((E + 1, T, D), 7.0, device="cuda")
    h.call("vae_reparam_cached", mu.cuda(), lv.cuda(), torch.tensor([2, 3, 1], dtype=torch.int32, device="cuda"),
           *[e.cuda() for e in eps], lat3, E, nch, D, cache_rows)
    torch.cuda.synchronize()
    got3 = lat3.cpu()
    assert torch.isnan(got3[1, keep]).all() and (got3[1, [nch, 2 * nch + 1, 3 * nch + 2]] == 0).all()
    assert torch.equal(got3[0], got[0]) and torch.equal(got3[2], got[2]) and (got3[E] == 7.0).all()


def test_interp_blend_scatter(rg, h, parity):
    B, dim = 2, 7
    worst = 0.0
    for scale in (1, 2, 3):
        for n in (1, 2, 75):
            x = kr.randn((B, n, dim), 500 + 10 * scale + n)
            before = kr.canary(B * n * scale + 2, dim)
            out = before.cuda()
            h.call("interp_linear", x.cuda(), out, B, n, dim, scale)
            torch.cuda.synchronize()
            assert kr.untouched(out, before, B * n * scale, 0, dim)
            ref = F.interpolate(x.double().permute(0, 2, 1), scale_factor=scale, mode="linear", align_corners=False).permute(0, 2, 1)
            mag = F.interpolate(x.double().abs().permute(0, 2, 1), scale_factor=scale, mode="linear", align_corners=False).permute(0, 2, 1)
            # fp32 source coordinate (3 operations on values <= n * scale: absolute 3 U n scale on the weight, which multiplies a
            # difference of neighbours <= 2 max|x|), then two products and a sum
            bound = kr.MARGIN * (4 * kr.U * mag + 3 * kr.U * n * scale * 2 * float(x.abs().max()))
            worst = max(worst, kr.worst_ratio(out.cpu()[:B * n * scale].view(B, n * scale, dim), ref, bound))
    parity.check("rg_interp_linear scale 1..3, n in {1, 2, 75}: worst |err| / bound", worst, 1.0)
    n, worst = 9, 0.0
    for overlap in (1, 2, 5, n):
        prev, cur = kr.randn((B, overlap, dim), 600 + overlap), kr.randn((B, n, dim), 601 + overlap)
        c = cur.cuda()
        h.call("blend_linear", prev.cuda(), c, B, n, dim, overlap)
        torch.cuda.synchronize()
        got = c.cpu()
        assert torch.equal(got[:, overlap:], cur[:, overlap:])
        wn = torch.linspace(0, 1, overlap, dtype=torch.float64).view(1, overlap, 1)
        ref = prev.double() * (1 - wn) + cur[:, :overlap].double() * wn
        # weights carry 3 U (a product, a difference, 1 - w), then two products and a sum
        bound = kr.MARGIN * 6 * kr.U * (prev.double().abs() + cur[:, :overlap].double().abs())
        worst = max(worst, kr.worst_ratio(got[:, :overlap], ref, bound))
    parity.check("rg_blend_linear overlap in {1, 2, 5, n}: worst |err| / bound", worst, 1.0)
    # scatter_joints with joints that belong to no part
    rows, J = 5, 9
    part = [0, -1, 2, 1, 3, -1, 0, 2, 1]
    joint = [1, 0, 0, 1, 0, 0, 0, 2, 0]
    parts = [kr.randn((rows, w), 700 + i) for i, w in enumerate((2 * 3 + 2, 2 * 3, 3 * 3 + 1, 1 * 3))]
    before = kr.canary(rows + 1, J * 3)
    out = before.cuda()
    args = []
    for p in parts:
        args += [p.cuda(), p.shape[1]]
    h.call("scatter_joints", *args, torch.tensor(part, dtype=torch.int32, device="cuda"),
           torch.tensor(joint, dtype=torch.int32, device="cuda"), out, rows, J)
    torch.cuda.synchronize()
    assert kr.untouched(out, before, rows, 0, J * 3)
    exp = torch.zeros(rows, J * 3)
    for j in range(J):
        if part[j] >= 0:
            exp[:, 3 * j:3 * j + 3] = parts[part[j]][:, 3 * joint[j]:3 * joint[j] + 3]
    assert torch.equal(out.cpu()[:rows], exp)


def test_blend_aa_with_an_overlap_of_one_frame(rg, h):
    """torch.linspace(0, 1, 1) = [0]: with overlap = 1 the first frame is the previous motion's last frame through
    axis-angle -> 6D -> axis-angle, i.e. what the kernel gives for that frame without a blend; the other frames are unchanged."""
    B, n, J = 2, 4, 5
    g = kr.rng(800)
    prev = torch.from_numpy(g.uniform(-1.5, 1.5, (B, 1, J * 3)).astype("float32"))
    cur = torch.from_numpy(g.uniform(-1.5, 1.5, (B, n, J * 3)).astype("float32"))
    swapped = cur.clone()
    swapped[:, 0] = prev[:, 0]
    a, b = torch.full((B, n, J * 3), float("nan"), device="cuda"), torch.full((B, n, J * 3), float("nan"), device="cuda")
    h.call("blend_aa", prev.cuda(), cur.cuda(), a, B, n, J, 1)
    h.call("blend_aa", None, swapped.cuda(), b, B, n, J, 0)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert (a.cpu()[:, 0] - prev[:, 0]).abs().max() <= 1e-5      # (angles below pi: the round trip returns the rotation vector)
