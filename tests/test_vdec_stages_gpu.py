"""GPU: the block-fused VAE decoder (rg_vdec_step, csrc/rg_vdec.hip) launch by launch against the fp64 references of
tests/kernel_refs.py ("Fused stacks": the decoder's tiers), and the exact edges that the HIP-against-HIP tests of
test_decode_grouped_gpu.py leave out.

The launches are issued here one by one, as vencfwd.VdecForward.run issues them, with every buffer the kernel writes -- x, pos,
kbuf, vt, qimg, xbuf, dump, frames -- a view inside a sentinel-filled allocation.  Teacher forcing: what launch `step` computes is
compared with references that start from what the kernel itself left behind launch step - 1 (exact fp32 values):

  dump            the state behind block step - 1 against `vdec_block_ref` of the residual x of launch step - 1 (statistical tier);
                  launch 0: the input, bit for bit; after the last launch x against `vdec_final_ref` of the last dump
  x               the dump bit for bit at input and middle blocks; at output blocks within `vdec_skip_ref` of this dump and the dump
                  behind block skip_of(step) (worst-case tier)
  kbuf, vt, qimg  the parity half step & 1 of the keys (row-major) and values (feature-major) and the tiles' Q images against
                  `vdec_proj_ref` of that x and the exact pos (worst-case tier: half a bf16 ulp + the accumulation bound first,
                  then the MARGIN form); the other parity half and pos bit-identical before and after the launch

test_kernel_refs_cpu.py shows on the CPU that a correct emulation stays inside all of these bounds and that each of
kr.VDEC_MUTANTS -- a tile reading the other parity's keys, a missing 1 / sqrt(16), pos added to V or left out of K, heads of 32,
norm2's parameters in norm1's place, 16 dropped keys, exchanged halves of the skip linear, no final norm -- leaves them at the
first buffer it touches.

Measured worst |err| / bound of the kernel over all cases, launches and both inputs (information, not limits; beside them the CPU
emulation's): see `test_vdec_every_launch_against_fp64`."""
import ctypes

import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

SENT = -123456.75          # fp32 sentinel (exact; the decoder does not produce it)
SENT16 = 0x7FC1            # bf16 buffers are read back as int16 bit patterns: a NaN the kernel does not produce
PAD = 48 * 512             # sentinel elements in front of and behind every buffer (one tile's dump)
S, TR, TP, DM = kr.VDEC_S, kr.VDEC_TILE, 48, kr.DM
BUFS = ("x", "pos", "qimg", "kbuf", "vt", "xbuf", "dump", "frames")


@pytest.fixture(scope="module")
def stacks(rg):
    """(num_layers, seed) -> (handle, VencStreams of the decoder stack on the device, VdecModel: the fp64 parameters from the
    same state dict)."""
    assert torch.cuda.is_available()
    cache = {}

    def get(num_layers, seed=kr.VDEC_SEED):
        if (num_layers, seed) not in cache:
            vcfg = rg.synth.default_vae_cfg("upper", num_layers=num_layers)
            assert rg.vencfwd.decoder_supported(vcfg, "bf16", vcfg["num_frames"] // vcfg["frame_chunk_size"])
            sd = rg.synth.synth_vae_state(seed, vcfg)
            st = rg.vencfwd.VencStreams(sd, "decoder", num_layers, vcfg["num_heads"] * 8, torch.device("cuda"))
            cache[num_layers, seed] = (rg.capi.get_handle(torch.cuda.current_device()), st, kr.VdecModel(sd, num_layers))
        return cache[num_layers, seed]
    return get


class _Buf:
    """`t`: n elements for the kernel, inside an allocation of PAD + n + PAD elements filled with the sentinel."""

    def __init__(self, n, dtype=torch.float32):
        self.n, self.sent = n, SENT if dtype == torch.float32 else SENT16
        self.all = torch.full((n + 2 * PAD,), self.sent, dtype=dtype, device="cuda")
        self.t = self.all[PAD:PAD + n]


class _Run:
    """The buffers and argument block of one decode, as vencfwd.VdecForward.run sets them up (sizes: include/rg_gesture.h
    rg_vdec_args), each inside sentinels.  x / pos: [nseq, 160, 512] CPU tensors or None (the sentinel: "any buffer")."""

    def __init__(self, rg, h, st, nseq, x=None, pos=None, dumps=True, latent=None, row_off=0, n_lat=0, table=None, frames=False):
        self.rg, self.h, self.st, self.nseq, self.nb = rg, h, st, nseq, st.nb
        self.b = dict(x=_Buf(nseq * S * DM), pos=_Buf(nseq * S * DM), qimg=_Buf(4 * nseq * TP * DM, torch.int16),
                      kbuf=_Buf(2 * nseq * S * DM, torch.int16), vt=_Buf(2 * nseq * DM * S, torch.int16),
                      xbuf=_Buf(4 * nseq * st.nb * 8 * 12 * 64 * 4))
        if dumps:
            self.b["dump"] = _Buf(4 * nseq * TP * DM)
        if frames:
            self.b["frames"] = _Buf(nseq * (S - n_lat) * DM)
        if x is not None:
            self.b["x"].t.copy_(x.reshape(-1))
        if pos is not None:
            self.b["pos"].t.copy_(pos.reshape(-1))
        self.latent = None if latent is None else latent.cuda().contiguous()
        self.table = None if table is None else table.cuda().contiguous()
        self.row_off, self.n_lat = row_off, n_lat
        self.last = 2 * st.nb + 1

    def args(self, step):
        a = self.rg.vencfwd.VdecArgs()
        ptr = lambda nm: self.b[nm].t.data_ptr() if nm in self.b else None
        a.wstream, a.pstream = self.st.wstream.data_ptr(), self.st.pstream.data_ptr()
        a.x, a.pos, a.qimg, a.kbuf, a.vt, a.xbuf, a.dump, a.frames = (ptr(nm) for nm in BUFS)
        a.nseq, a.nb, a.step = self.nseq, self.nb, step
        a.latent, a.table = (None if t is None else t.data_ptr() for t in (self.latent, self.table))
        a.lat_T, a.lat_row0, a.n_lat = 0 if self.latent is None else int(self.latent.shape[1]), self.row_off, self.n_lat
        if "dump" in self.b:
            self.b["dump"].t.fill_(SENT)          # a launch that does not write its dump must not pass on the previous one
        return a

    def launch(self, step):
        a = self.args(step)
        self.h.call("vdec_step", ctypes.byref(a), keep=(a, self))
        return self.snapshot()

    def snapshot(self):
        """name -> the whole allocation on the CPU, after checking the sentinels around every buffer."""
        torch.cuda.synchronize()
        snap = {nm: b.all.cpu() for nm, b in self.b.items()}
        for nm, t in snap.items():
            n, sent = self.b[nm].n, self.b[nm].sent
            assert bool((t[:PAD] == sent).all()) and bool((t[PAD + n:] == sent).all()), "wrote outside " + nm
        return snap


def _in(snap, nm):
    return snap[nm][PAD:len(snap[nm]) - PAD]


def _same(a, b):
    """Bit for bit (NaN patterns and signed zeros included)."""
    iv = lambda t: t.contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)
    return a.shape == b.shape and bool(torch.equal(iv(a), iv(b)))


def _rows(tiles, nseq):
    """[4 nseq, 48, 512] per tile -> [nseq, 160, 512]: rows < 40 of each tile (the rest is padding)."""
    return tiles.reshape(nseq, 4, TP, DM)[:, :, :TR].reshape(nseq, S, DM)


def _state(snap, nm, nseq):
    return _in(snap, nm).view(nseq, S, DM)


@pytest.mark.parametrize("kind", kr.VDEC_KINDS)
@pytest.mark.parametrize("num_layers,nseq", kr.VDEC_CASES)
def test_vdec_every_launch_against_fp64(rg, parity, stacks, num_layers, nseq, kind):
    """Every element of the 160 rows behind every launch: the dump, the residual x, K, V and the Q image (module docstring); nb =
    1 and 2 blocks per side (one and two skip levels), 1 and 3 sequences (4 and 12 tiles), the product's input (10 latent rows, 150
    zero queries) and dense rows.  Sentinels around every buffer behind every launch; x of a run with dumps == x of a run without.

    Worst |err| / bound, the kernel's / the CPU emulation's (test_kernel_refs_cpu.py), over all cases (information, not limits):
      state behind a block (statistical)      0.33 - 0.61   /  0.33 - 0.58
      final norm (statistical)                0.025 - 0.031 /  0.027 - 0.033
      skip linear (worst case)                2.8e-4 - 4.5e-4 / 1.3e-4 - 2.6e-4
      Q, K, V, half a bf16 ulp form           0.84 - 0.96   /  0.83 - 0.96
      Q, K, V, MARGIN form                    0.45 - 0.47   /  (below the half-ulp form)"""
    h, st, m = stacks(num_layers)
    nb = st.nb
    assert nb == m.nb == (num_layers - 1) // 2
    x0 = kr.vdec_input(nseq, num_layers, kind)
    pos = x0 + m.table
    tag = "vdec stages layers %d nseq %d %s" % (num_layers, nseq, kind)
    worst = {}

    def check(stage, name, got, ref, bound):
        r = kr.worst_ratio(got, ref, bound)
        print("%s %s: worst |err| / bound %.3g" % (tag, name, r))
        if not r <= 1.0:
            print("   " + kr.where_worst(got, ref, bound))
        worst[stage] = max(worst.get(stage, 0.0), r)

    plain = _Run(rg, h, st, nseq, x0, pos, dumps=False)
    for step in range(plain.last + 1):
        snap = plain.launch(step)
    x_plain = _state(snap, "x", nseq)
    assert torch.isfinite(x_plain).all()

    run = _Run(rg, h, st, nseq, x0, pos)
    prev, states, x_res = run.snapshot(), [], None
    for step in range(run.last + 1):
        cur = run.launch(step)
        assert _same(cur["pos"], prev["pos"]), "launch %d changed pos" % step
        d = _rows(_in(cur, "dump"), nseq)
        assert torch.isfinite(d).all()
        if step == 0:
            assert _same(d, x0), "launch 0: the dump is not the input"
        else:
            check("block (statistical)", "block %d" % (step - 1), d, *kr.vdec_block_ref(m, step - 1, x_res, pos))
        states.append(d)
        x_now = _state(cur, "x", nseq)
        if step == run.last:
            check("final norm (statistical)", "final norm", x_now, *kr.vdec_final_ref(m, d))
            assert _same(x_now, x_plain), "x changes with the dumps"
            for nm in ("qimg", "kbuf", "vt", "xbuf"):
                assert _same(cur[nm], prev[nm]), "the last launch wrote " + nm
            break
        if step <= nb:
            assert _same(x_now, d), "launch %d: x is not the state behind block %d" % (step, step - 1)
        else:
            check("skip linear (worst case)", "skip linear %d" % step, x_now, *kr.vdec_skip_ref(m, step, d, states[m.skip_of(step) + 1]))
        par = step & 1
        kb, vt = _in(cur, "kbuf").view(2, nseq, S, DM), _in(cur, "vt").view(2, nseq, DM, S)
        assert _same(kb[1 - par], _in(prev, "kbuf").view(2, nseq, S, DM)[1 - par]), "launch %d wrote the other parity's keys" % step
        assert _same(vt[1 - par], _in(prev, "vt").view(2, nseq, DM, S)[1 - par]), "launch %d wrote the other parity's values" % step
        got = dict(q=_rows(kr.from_bf16_bits(kr.vdec_qimg_rows(_in(cur, "qimg"), 4 * nseq)), nseq),
                   k=kr.from_bf16_bits(kb[par].contiguous()), v=kr.from_bf16_bits(vt[par].contiguous()).transpose(1, 2))
        proj = kr.vdec_proj_ref(m, step, x_now, pos)
        for nm in ("q", "k", "v"):
            ref, e = proj[nm]
            bound, b_ulp = kr.bf16_bounds(ref, e)
            check("%s (worst case, half a bf16 ulp)" % nm.upper(), "%s %d half ulp" % (nm.upper(), step), got[nm], ref, b_ulp)
            check("%s (worst case, MARGIN)" % nm.upper(), "%s %d" % (nm.upper(), step), got[nm], ref, bound)
        prev, x_res = cur, x_now
    for stage in ("block (statistical)", "final norm (statistical)", "skip linear (worst case)", "Q (worst case, half a bf16 ulp)",
                  "Q (worst case, MARGIN)", "K (worst case, half a bf16 ulp)", "K (worst case, MARGIN)",
                  "V (worst case, half a bf16 ulp)", "V (worst case, MARGIN)"):
        parity.check("%s %s worst |err| / bound" % (tag, stage), worst[stage], 1.0)


# ------------------------------------------------------------------------------------------------ exact edges
ROW_OFF, LAT_T = 7, 7 + 159 + 3          # the clip's latent holds rows [7, 7 + n_lat) for every n_lat, and three more


@pytest.mark.parametrize("nseq", [1, 3])
@pytest.mark.parametrize("n_lat", [1, 39, 40, 41, 159])
def test_vdec_own_ends_at_the_tile_boundaries(rg, stacks, n_lat, nseq):
    """latent / table / frames of rg_vdec_args with the latent rows ending one row into the first tile, on either side of the
    first tile boundary and one row before the end, against plain torch: launch 0's dump = cat(latent rows, zeros), pos = that +
    table (one fp32 add), frames = rows >= n_lat of the x that a run without `frames` leaves, x untouched by a last launch that
    stores frames; the run with the kernel's own input == the run that is handed the same x and pos."""
    h, st, m = stacks(3)
    lat = kr.randn((nseq, LAT_T, DM), 9700 + 10 * n_lat + nseq)          # every row non-zero: a wrong row shows
    x0 = torch.cat((lat[:, ROW_OFF:ROW_OFF + n_lat], torch.zeros(nseq, S - n_lat, DM)), dim=1)
    pos0 = x0 + m.table
    ends = dict(latent=lat, row_off=ROW_OFF, n_lat=n_lat, table=m.table)
    a = _Run(rg, h, st, nseq, **ends)
    for step in range(a.last + 1):
        snap = a.launch(step)
        if step == 0:
            assert _same(_rows(_in(snap, "dump"), nseq), x0), "launch 0's dump"
            assert _same(_state(snap, "x", nseq), x0), "x behind launch 0"
        assert _same(_state(snap, "pos", nseq), pos0), "pos behind launch %d" % step
    xa = _state(snap, "x", nseq)
    assert torch.isfinite(xa).all()
    given = _Run(rg, h, st, nseq, x0, pos0, dumps=False)
    for step in range(given.last + 1):
        snap = given.launch(step)
    assert _same(_state(snap, "x", nseq), xa), "the run that builds its own input differs from the run that is handed it"
    f = _Run(rg, h, st, nseq, dumps=False, frames=True, **ends)
    for step in range(f.last):
        before = f.launch(step)
    snap = f.launch(f.last)
    assert _same(snap["x"], before["x"]), "the last launch wrote x although it stores frames"
    assert _same(_in(snap, "frames").view(nseq, S - n_lat, DM), xa[:, n_lat:]), "frames"


@pytest.mark.parametrize("num_layers,widths", [(5, (1, 3)), (3, (3, 1, 2, 1))])
def test_vdec_grouped_launches_of_unequal_width(rg, stacks, num_layers, widths):
    """rg_vdec_step_grouped with n = 2 and n = 4 stacks of different weights and different numbers of sequences (the narrower
    groups' workgroups past 4 nseq return at once): behind every launch every buffer of every group, the dump included, equals
    the single launches' bit for bit, the sentinels around it too."""
    n = len(widths)
    single, grouped = [], []
    for i, nseq in enumerate(widths):
        h, st, m = stacks(num_layers, kr.VDEC_SEED + 10 * (i + 1))
        x0 = kr.randn((nseq, S, DM), 9800 + 10 * i + num_layers)
        for runs in (single, grouped):
            runs.append(_Run(rg, h, st, nseq, x0, x0 + m.table))
    for step in range(single[0].last + 1):
        ref = [r.launch(step) for r in single]
        blocks = [r.args(step) for r in grouped]
        h.call("vdec_step_grouped", ctypes.byref((rg.vencfwd.VdecArgs * n)(*blocks)), n, keep=(blocks, grouped))
        for i, r in enumerate(grouped):
            got = r.snapshot()
            for nm in got:
                assert _same(got[nm], ref[i][nm]), "launch %d group %d (nseq %d): %s differs from the single launch" % (step, i, widths[i], nm)
    assert all(torch.isfinite(_in(s, "x")).all() for s in ref)
