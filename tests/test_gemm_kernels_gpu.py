"""GPU: every kernel variant and fused epilogue of the rg_gemm family (csrc/rg_gemm.hip, rg_gemm_dma.hip, rg_gemm_big.hip,
rg_gemm_epi.h) against the fp64 reference of tests/kernel_refs.py (`gemm_ref`: formulas, bounds and their derivation).  Every
element of every output is compared; every written buffer has a wider leading dimension and extra rows filled with a
sentinel that must survive bit for bit (past column N, past row M, the ld - N padding, the elements in front of an offset
`out`).  The variants are selected with rg_set_gemm_path / rg_set_gemm_waves, both restored to 0 afterwards; grids that must
exceed the CU count are sized from rg_num_cus.

Which instantiation each case reaches, read off the dispatch (rg_gemm in rg_gemm.hip, rg_gemm_dma_launch, dma_depth,
rg_gemm_big_launch); launch<A_BF16, SPLIT, FAST>, dma_launch<A_BF16, SPLIT, NS (ring), NW (waves)>; M of the "more workgroups
than CUs" cases is given for 256 CUs:

  case instantiation          path waves     M x    N x   K   features
  g1  launch<0,0,0>            0     0      65 x  160 x  78   ragged K, odd ld, stats ragged N
  g2  launch<0,0,0>            1     0       1 x   61 x   8   one row, ragged tile
  g3  launch<0,0,0>            1     0     129 x  192 x 200   LN, tbias 43, residual ldr % 4 != 0, out2
  g4  launch<0,0,0>            1     0     200 x  384 x 448   4 segments STYL LN IDENT LN short last, gb_group, softmax N
  g5  launch<0,1,0>            0     0      65 x  160 x  78   W_lo ragged K, GELU libm
  g6  launch<0,1,0>            1     0     129 x  192 x 256   W_lo LN + STYL, softmax 32
  g7  launch<1,0,0>            1     0      63 x  128 x 200   bf16 A, folded LN 9 partials, stats
  g8  launch<1,0,0>            1     0     200 x  256 x 256   bf16 A gb_group, bf16 out at +4 B, ldo % 8 != 0
  g9  launch<0,0,0>            1     0      63 x  160 x   8   split_col 128 ragged rest, odd ldo2
  ga  launch<0,0,0>            1     0      65 x  128 x   8   full tiles, fp32 ldo % 4 != 0
  gb  launch<0,0,0>            1     0      64 x   32 x 512   one head N 32, K 512, softmax 32
  gc  launch<1,0,0>            1     0     129 x  128 x 512   bf16 A K 512, GELU bf16 out streamed
  f1  launch<0,0,1>            3     0     129 x  192 x 256   FAST fp32 A, ReLU bf16 out
  f2  launch<1,0,1>            3     0      65 x  256 x 512   FAST bf16 A, a_row_mod, residual, out at +4 B
  f3  launch<0,0,1>            3     0      65 x  128 x 256   FAST fp32 A, tbias 43, softmax N, stats
  d1  dma_launch<1,0,4,8>      0     0      64 x  128 x  64   one K tile
  d2  dma_launch<1,0,4,8>      2     0      65 x  160 x 128   GELU bf16 out, ragged second tile (path 2)
  d3  dma_launch<1,0,4,4>      5     4     129 x  384 x 192   folded LN 4, stats, out2, residual, 3 K tiles (path 5)
  d4  dma_launch<1,0,2,8>      0     8    2112 x 1024 x  64   more workgroups than CUs, 8 waves, ring 2 > K
  d5  dma_launch<1,0,2,4>      0     4    1408 x 1536 x 128   more workgroups than CUs, 4 waves, tbias 43, softmax 512 of 1536
  d6  dma_launch_pair          0     0    2112 x 1024 x 128   two workgroups per CU, folded LN 8, residual
  d7  dma_launch_pair          0    16     129 x  256 x 320   two workgroups per CU forced, 5 K tiles
  d8  dma_launch_narrow        0     0      65 x  192 x 320   tile_n 64, folded LN 1, stats per 64, out2, residual
  d9  dma_launch<1,0,4,8>      0     0     129 x  256 x 512   split_col 128 of 256
  da  dma_launch<1,0,4,4>      0     4     200 x  320 x  64   split_col 256 of 320, stats, ReLU
  db  dma_launch<1,0,4,8>      0     0     129 x  256 x 128   bf16 A gb_group 128, a_row_mod
  dc  dma_launch_pair          0    16      65 x  160 x 128   two workgroups per CU forced, tbias 43, softmax 64
  dd  dma_launch_narrow        0     0      63 x   64 x  64   tile_n 64 one tile N 64, tbias 43, softmax 32
  de  dma_launch<1,0,4,8>      0     0      65 x  160 x 192   folded LN 9 partials (scalar loop)
  df  dma_launch<1,0,4,8>      0     0      63 x   32 x  64   one head N 32
  dg  dma_launch_pair          0    16     129 x  128 x 128   two workgroups per CU forced, folded LN 9 partials
  e1  dma_launch<0,0,4,8>      0     0      65 x  128 x  64   plain one K tile
  e2  dma_launch<0,0,4,4>      0     0     129 x  160 x 512   LN 1 partial, softmax 32, tbias 43
  e3  dma_launch<0,0,3,4>      0     0     200 x  192 x 640   4 segments STYL LN IDENT IDENT short last, col_offset
  e4  dma_launch<0,0,3,8>      0     8      65 x  128 x 704   4 segments, 8 waves
  e5  dma_launch<0,0,2,4>      0     0    2112 x 1024 x  64   LN, more workgroups than CUs, residual, stats
  e6  dma_launch<0,0,2,8>      0     8    2112 x 1024 x 128   plain a_row_mod, more workgroups than CUs, 8 waves, out2
  e7  dma_launch<0,1,3,4>      0     0     129 x  160 x 192   W_lo LN, 3 K tiles
  e8  dma_launch<0,1,3,4>      0     0      63 x  128 x  64   W_lo STYL, softmax 32, GELU libm
  e9  dma_launch<0,0,4,4>      0     0      65 x  384 x 256   LN gb_group 128
  ea  dma_launch<0,0,4,8>      0     0     129 x  256 x 128   plain, residual ldr != ldo, out2, stats
  eb  dma_launch<0,0,4,4>      0     0      65 x  256 x 192   LN, ReLU bf16 out, split_col 128, residual
  ec  dma_launch<0,0,4,8>      0     0      64 x   64 x 128   one narrow tile N 64, GELU bf16 out
  s1  dma_launch_styl<5,8>     0     0     129 x  160 x 320   a_styl 5 K tiles, residual
  s2  dma_launch_styl<5,8>     0     0      65 x  128 x  64   a_styl one K tile, 1 partial
  s3  dma_launch_styl<5,8>     0     0      63 x  128 x 512   a_styl K 512, out2, 8 partials
  s4  dma_launch_styl<3,4>     0     0    2112 x 1024 x  64   a_styl more workgroups than CUs
  s5  dma_launch_styl<5,8>     0     0      65 x  160 x  64   a_styl tbias 43, softmax 32, stats
  b1  big_launch<256>          4     0     200 x  384 x 128   128x256 ragged half, folded LN 4, stats, out2, residual
  b2  big_launch<128>          6     0     129 x  192 x 320   128x128 ragged, GELU bf16 out
  b3  big_launch<128,2,4>      7     0      65 x  256 x 512   128x128 ring 2, softmax N, tbias 43, split_col 128
  b4  big_launch<256>          4     0     129 x  512 x 192   128x256 gb_group 256
  b5  big_launch<256>          4     0     129 x  384 x 128   128x256 split_col 128 inside the tile, ragged half, a_row_mod
  b6  big_launch<128>          6     0     200 x  256 x 128   128x128 folded LN 9 partials, tbias 43
(the W_lo LDS-DMA ring only fits the LDS with one segment, so LN + STYL together in W_lo mode run on the generic kernel: g6.)

What is not crossed, and why.  The epilogue (rg_gemm_epi.h: `epilogue`) is one function that every kernel calls with (tile
origin, tile width, optional prefetched residual, optional LDS row statistics); bias, tbias, softmax, activation, statistics
and the six store paths do not depend on the caller beyond those arguments.  So every epilogue feature runs at least once per
CALLING CONVENTION -- generic / FAST (no prefetch, no LDS statistics), LDS-DMA with residual prefetch and LDS statistics (bf16 A:
d3, d6; fp32 A: ea, eb, e5), the two-per-CU kernel without prefetch (d6, d7, dc, dg), the 64-wide tile (d8, dd), the stylized
kernel (s1, s3, s5) and the big kernel's 128-column sub-tiles (b1, b3, b5, b6) -- and not once per ring depth or wave count, which
only change the K loop.  K-loop features (a_row_mod, gb_group, segments, W_lo, a_styl) run on every kernel whose loads implement
them: a_row_mod generic fp32 / FAST bf16 (f2) / LDS-DMA bf16 (db) / LDS-DMA fp32 (e6) / big (b5); gb_group generic fp32 (g4) and
bf16 (g8), LDS-DMA fp32 (e9) and bf16 (db), big (b4).  Stylized A admits neither a_row_mod nor gb_group nor tile_n 64 nor W_lo
(gemm_validate); tile_n 64 admits no split_col; W_lo admits fp32 segments only.
"""
import ctypes

import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

REQUIRED = ("launch<0,0,0>", "launch<0,1,0>", "launch<1,0,0>", "launch<0,0,1>", "launch<1,0,1>",
            "dma_launch<1,0,4,8>", "dma_launch<1,0,4,4>", "dma_launch<1,0,2,8>", "dma_launch<1,0,2,4>",
            "dma_launch<0,0,4,8>", "dma_launch<0,0,4,4>", "dma_launch<0,0,3,8>", "dma_launch<0,0,3,4>", "dma_launch<0,0,2,8>",
            "dma_launch<0,0,2,4>", "dma_launch<0,1,3,4>", "dma_launch_pair", "dma_launch_narrow", "dma_launch_styl<5,8>",
            "dma_launch_styl<3,4>", "big_launch<256>", "big_launch<128>", "big_launch<128,2,4>")
NAMES = list(kr.gemm_cases(256))


@pytest.fixture(scope="module")
def h(rg):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return rg.capi.get_handle(0)


@pytest.fixture(scope="module")
def cases(h):
    return kr.gemm_cases(h.lib.rg_num_cus(h._h))


def test_num_cus_and_every_instantiation_has_a_case(h, cases):
    assert h.lib.rg_num_cus(h._h) == torch.cuda.get_device_properties(h.device).multi_processor_count
    assert list(cases) == NAMES
    assert {c().variant for c in cases.values()} == set(REQUIRED)


class _Buf:
    """A sentinel-filled device buffer [rows, ld] that starts `off` elements into its allocation."""

    def __init__(self, rows, ld, dtype, off=0):
        self.rows, self.ld, self.off = rows, ld, off
        self.before = kr.canary(1, off + rows * ld + 8, dtype)
        self.dev = self.before.cuda()
        self.view = self.dev.view(-1)[off:off + rows * ld].view(rows, ld)

    def tensor(self):
        return self.view.view(torch.bfloat16) if self.view.dtype == torch.int16 else self.view

    def read(self, M, n):
        """The written region [M, n] (bf16 as float) after asserting that nothing else changed."""
        got = self.dev.cpu()
        sl = slice(self.off, self.off + self.rows * self.ld)
        g2, b2 = got.view(-1)[sl].view(self.rows, self.ld), self.before.view(-1)[sl].view(self.rows, self.ld)
        edge = lambda t: torch.cat((t.view(-1)[:self.off], t.view(-1)[sl.stop:]))[None, :]
        assert kr.untouched(g2, b2, M, 0, n), "written outside [%d, %d]" % (M, n)
        assert kr.untouched(edge(got), edge(self.before), 0, 0, 0), "written outside the buffer's rows"
        w = g2[:M, :n]
        return kr.from_bf16_bits(w.contiguous()) if w.dtype == torch.int16 else w


def _prepare(G, c):
    """Device tensors, sentinel buffers and the descriptor of case c."""
    dev = "cuda"
    M, N, K = c.M, c.N, c.K
    kw = dict(M=M, N=N, K=K, W=G.pack_weight(c.w, dev, split=c.wlo), a_row_mod=c.a_row_mod, gb_group=c.gb_group,
              gb_stride=c.gb_stride if c.gb_group else 0, act=c.act, softmax_cols=c.softmax_cols, split_col=c.split_col, tile_n=c.tile_n)
    if c.kind == "f32":
        src = c.src.to(dev)
        up = lambda t: None if t is None else t.to(dev)
        kw.update(seg_len=c.seg_len, segs=[G.Seg(src, ld=c.ld, mode=m, stats=up(c.stats[i]), gamma=up(c.gamma[i]), beta=up(c.beta[i]),
                                                 scale_shift=up(c.ss[i]), col_offset=c.col[i]) for i, m in enumerate(c.modes)])
    else:
        kw.update(A=c.a.to(dev).bfloat16(), lda=c.lda)
        if c.kind == "styl":
            kw.update(a_styl=G.Seg(None, ld=0, stats=c.st.to(dev), gamma=c.gain.to(dev), beta=c.offset.to(dev)))
    if c.ln:
        kw.update(ln_stats=c.ln_stats.to(dev), ln_c1=c.c1.to(dev))
    if c.bias is not None:
        kw.update(bias=c.bias.to(dev))
    if c.tb:
        kw.update(tbias=c.tbias.to(dev), tb_period=c.tb)
    if c.res is not None:
        kw.update(residual=c.res.to(dev), ldr=c.ldr)
    bufs = {"out": _Buf(M + 2, c.ldo, torch.int16 if c.out_bf16 else torch.float32, c.out_off)}
    kw.update(out=bufs["out"].tensor(), ldo=c.ldo)
    if c.want_stats:
        t = 64 if c.tile_n == 64 else 128
        bufs["stats"] = _Buf(M + 1, 2 * ((N + t - 1) // t), torch.float32)
        kw.update(stats_out=bufs["stats"].view)
    if c.want_out2:
        bufs["out2"] = _Buf(M + 2, c.ldo2, torch.int16)
        kw.update(out2=bufs["out2"].tensor())
    return G.make_desc(**kw), kw, bufs


def _check(c, bufs, parity, label):
    """Every element of every output of case c against the fp64 reference; one parity line with the worst ratio."""
    M, N = c.M, c.N
    ref = kr.gemm_ref(c)
    n_out = c.split_col or N
    got = bufs["out"].read(M, n_out)
    assert torch.isfinite(got).all(), label
    r = {}
    if c.out_bf16:
        bm, bu = kr.bf16_bounds(ref["out"], ref["e"])
        r["out"], r["out ulp"] = kr.worst_ratio(got, ref["out"], bm), kr.worst_ratio(got, ref["out"], bu)
    else:
        r["out"] = kr.worst_ratio(got, ref["out"], ref["e"])
    if c.want_stats:
        st = bufs["stats"].read(M, bufs["stats"].ld).view(M, -1, 2)
        r["stats"] = kr.worst_ratio(st, ref["stats"], ref["e_stats"])
    if c.want_out2:
        g2 = bufs["out2"].read(M, N - c.split_col)
        bm, bu = kr.bf16_bounds(ref["out2"], ref["e2"])
        r["out2"], r["out2 ulp"] = kr.worst_ratio(g2, ref["out2"], bm), kr.worst_ratio(g2, ref["out2"], bu)
    print("rg_gemm %s: %s" % (label, "  ".join("%s %.4f" % kv for kv in r.items())))
    head, _, tail = label.partition(" | ")          # the output's kind goes in front of the description: names are cut at 78
    for k, v in r.items():
        if k != "out":
            parity.check("rg_gemm %s %s | %s" % (head, k, tail), v, 1.0)
    parity.check("rg_gemm %s out | %s" % (head, tail), r["out"], 1.0)


def _label(c):
    return "%s %s %dx%dx%d | %s" % (c.name.split()[0], c.variant, c.M, c.N, c.K, c.name.split(" ", 1)[1])


@pytest.mark.parametrize("name", NAMES)
def test_gemm_case(rg, h, parity, cases, name):
    c = cases[name]()
    desc, kw, bufs = _prepare(rg.gemm, c)
    assert h.lib.rg_set_gemm_path(h._h, c.path) == 0 and h.lib.rg_set_gemm_waves(h._h, c.waves) == 0
    try:
        rg.gemm.launch(h, desc, keep=kw)
        torch.cuda.synchronize()
    finally:
        h.lib.rg_set_gemm_path(h._h, 0)
        h.lib.rg_set_gemm_waves(h._h, 0)
    _check(c, bufs, parity, _label(c))


@pytest.mark.parametrize("family,path,M,N,K,kw", [
    ("generic", 1, 65, 160, 78, dict(stats=True)),
    ("LDS-DMA", 0, 129, 160, 192, dict(kind="bf16", res=True, ldr_pad=4, out2=True)),
    ("big-tile", 4, 129, 256, 128, dict(kind="bf16", act=1, out_bf16=True)),
])
def test_grouped_launch_against_reference(rg, h, parity, family, path, M, N, K, kw):
    """rg_gemm_grouped: four descriptors of one signature in one launch (blockIdx.y picks the descriptor), each against its
    own reference."""
    G = rg.gemm
    cs = [kr.gemm_case("grouped %s %d" % (family, i), M, N, K, 7900 + 10 * path + i, **kw) for i in range(4)]
    prep = [_prepare(G, c) for c in cs]
    arr = (G.GemmDesc * 4)(*[p[0] for p in prep])
    launches = ctypes.c_int64(-1)
    assert h.lib.rg_set_gemm_path(h._h, path) == 0
    try:
        assert h.lib.rg_profile_begin(h._h) == 0          # counts the rg_gemm launches: a fallback to single launches makes four
        rc = h.lib.rg_gemm_grouped(h._h, arr, 4, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert h.lib.rg_profile_end(h._h, 0 if cs[0].kind == "f32" else 1, ctypes.byref(launches), None, None) == 0
        torch.cuda.synchronize()
    finally:
        h.lib.rg_set_gemm_path(h._h, 0)
    assert rc == 0, h.lib.rg_last_error(h._h).decode()
    assert launches.value == 1, "the four descriptors share a signature: one launch with blockIdx.y = descriptor, got %d" % launches.value
    for i, c in enumerate(cs):
        _check(c, prep[i][2], parity, "grouped[%d] %s %dx%dx%d | four descriptors, one launch" % (i, family, M, N, K))


def _bad_tb(d):
    d.tb_period = 0


def _bad_split_no_out2(d):
    d.out2 = None


def _set(field, value):
    def f(d):
        setattr(d, field, value)
    return f


@pytest.mark.parametrize("what,mutate,message", [
    ("tbias with tb_period 0", _bad_tb, "tb_period"),
    ("tbias with a negative tb_period", _set("tb_period", -43), "tb_period"),
    ("split_col without out2", _bad_split_no_out2, "split_col"),
    ("split_col not a multiple of 128", _set("split_col", 64), "split_col"),
    ("split_col = N", _set("split_col", 256), "split_col"),
    ("split_col negative", _set("split_col", -128), "split_col"),
    ("softmax_cols > N", _set("softmax_cols", 288), "softmax_cols"),
    ("ln_stats without ln_c1", _set("ln_c1", None), "ln_c1"),
    ("ln_stats with ln_nparts 0", _set("ln_nparts", 0), "ln_nparts"),
    ("bf16 A with K % 8 != 0", _set("K", 60), "K % 8"),
])
def test_validation_rejects_on_the_host(rg, h, what, mutate, message):
    """Descriptors the epilogue cannot handle are refused by gemm_validate, which rg_gemm and rg_gemm_grouped run on the
    host before anything is launched: a non-zero code, the reason in rg_last_error, and `out` / `out2` keep their sentinel."""
    G = rg.gemm
    c = kr.gemm_case("valid", 64, 256, 64, 7999, kind="bf16", tb=43, ln=2, out2=True, split_col=128)
    desc, kw, bufs = _prepare(G, c)
    mutate(desc)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for call in (lambda: h.lib.rg_gemm(h._h, ctypes.byref(desc), s), lambda: h.lib.rg_gemm_grouped(h._h, ctypes.byref(desc), 1, s)):
        assert call() != 0, what
        assert message in h.lib.rg_last_error(h._h).decode(), (what, h.lib.rg_last_error(h._h).decode())
    torch.cuda.synchronize()
    for b in bufs.values():
        b.read(0, 0)
