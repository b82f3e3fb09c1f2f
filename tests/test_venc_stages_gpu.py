"""GPU: the fused VAE encoder stack (rg_venc_forward, csrc/rg_venc.hip) block by block against the fp64 references of
tests/kernel_refs.py ("Fused stacks"), through rg_venc_args.dump / dump_block.

Teacher forcing: the reference of block b starts from the kernel's own dump behind block b - 1 (exact fp32 values), an output
block also from the dump it takes its skip state from; `out` is the final LayerNorm of the last dump.  The references read the
state dict of synth_vae_state, not the packed streams of vencfwd.py.  test_kernel_refs_cpu.py shows on the CPU that the bounds
hold for a correct emulation and that a missing softmax scale, exchanged halves of the skip linear and norm2's parameters in
norm1's place exceed them."""
import ctypes

import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

SENT = -123456.75          # sentinel around `out` and `dump` (exact in fp32; the encoder does not produce it)
SQ = 24                    # row stride of a workgroup's two sequences in the dump


@pytest.fixture(scope="module")
def stacks(rg):
    """num_layers -> (handle, VencStreams on the device, VencModel: the fp64 parameters from the same state dict)."""
    assert torch.cuda.is_available()
    cache = {}

    def get(num_layers):
        if num_layers not in cache:
            vcfg = rg.synth.default_vae_cfg("upper", num_layers=num_layers)
            assert rg.vencfwd.supported(vcfg, "bf16")
            sd = rg.synth.synth_vae_state(kr.VENC_SEED, vcfg)
            st = rg.vencfwd.VencStreams(sd, "encoder", num_layers, vcfg["num_heads"], torch.device("cuda"))
            cache[num_layers] = (rg.capi.get_handle(torch.cuda.current_device()), st, kr.VencModel(sd, num_layers))
        return cache[num_layers]
    return get


def _run(rg, h, st, x, nseq, S, dump_block):
    """One launch with `out` and `dump` inside sentinel-filled buffers (VencForward.run allocates `out` itself).  Returns
    (out [nseq, S, 512], dump [workgroups, 48, 512] or None), after checking the sentinels around both."""
    # (mirrors vencfwd.VencForward.run line for line -- the argument block, the xbuf size [ceil(nseq / 2)][nb][8][12][64][4] of
    #  include/rg_gesture.h: rg_venc_args -- except that `out` and `dump` are views into the sentinel buffers)
    nwg = (nseq + 1) // 2
    obuf = torch.full(((nseq + 2) * S, kr.DM), SENT, device="cuda")
    dbuf = torch.full(((nwg + 2) * 48, kr.DM), SENT, device="cuda")
    xbuf = torch.empty(nwg * st.nb * 8 * 12 * 64 * 4, device="cuda")
    a = rg.vencfwd.VencArgs()
    a.wstream, a.pstream = st.wstream.data_ptr(), st.pstream.data_ptr()
    a.x, a.out, a.xbuf = x.data_ptr(), obuf[S:].data_ptr(), xbuf.data_ptr()
    a.dump = dbuf[48:].data_ptr() if dump_block >= 0 else None
    a.nseq, a.S, a.nb, a.dump_block = nseq, S, st.nb, dump_block
    h.call("venc_forward", ctypes.byref(a), keep=(a, x, obuf, dbuf, xbuf))
    torch.cuda.synchronize()
    ob, db = obuf.cpu(), dbuf.cpu()
    assert bool((ob[:S] == SENT).all()) and bool((ob[(nseq + 1) * S:] == SENT).all()), "wrote outside out"
    assert bool((db[:48] == SENT).all()) and bool((db[(nwg + 1) * 48:] == SENT).all()), "wrote outside dump"
    if dump_block < 0:
        assert bool((db == SENT).all())
    out = ob[S:(nseq + 1) * S].view(nseq, S, kr.DM)
    return out, (db[48:(nwg + 1) * 48].view(nwg, 48, kr.DM) if dump_block >= 0 else None)


def _state(dump, nseq, S):
    """[nseq, S, 512] out of a dump: sequence 2 w in rows [0, S) of workgroup w, sequence 2 w + 1 in rows [24, 24 + S)."""
    return torch.stack([dump[i // 2, (i % 2) * SQ:(i % 2) * SQ + S] for i in range(nseq)])


@pytest.mark.parametrize("num_layers,S,nseq", kr.VENC_CASES)
def test_venc_forward_every_block_against_fp64(rg, parity, stacks, num_layers, S, nseq):
    """Every element of the rows < S behind every block and of `out`: worst |err| / bound <= 1, one parity line each; nb = 1 and
    2 blocks per side, S from 2 to the full 24 rows, a lone sequence in a workgroup (nseq 1 and 3); sentinels around `out` and
    `dump`; `out` of a launch with a dump equals `out` of a launch without, bit for bit."""
    h, st, m = stacks(num_layers)
    assert st.nb == m.nb == (num_layers - 1) // 2
    x = kr.venc_input(nseq, S, num_layers)
    xd = x.cuda().view(nseq * S, kr.DM).contiguous()
    out, _ = _run(rg, h, st, xd, nseq, S, -1)
    assert torch.isfinite(out).all()
    tag = "venc stages layers %d S %d nseq %d" % (num_layers, S, nseq)

    def check(name, got, ref, bound):
        r = kr.worst_ratio(got, ref, bound)
        print("%s %s: worst |err| / bound %.3f" % (tag, name, r))
        if not r <= 1.0:
            print("   " + kr.where_worst(got, ref, bound))
        parity.check("%s %s worst |err| / bound" % (tag, name), r, 1.0)

    X, states = x, []
    for b in range(2 * m.nb + 1):
        out_b, dump = _run(rg, h, st, xd, nseq, S, b)
        assert torch.equal(out_b, out), "block %d: out changes with the dump" % b
        got = _state(dump, nseq, S)
        assert torch.isfinite(got).all()
        sk = m.skip_of(b)
        check("block %d" % b, got, *kr.venc_block_ref(m, b, X, states[sk] if sk is not None else None))
        states.append(got)
        X = got
    check("out", out, *kr.venc_final_ref(m, X))
