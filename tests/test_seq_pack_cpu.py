"""CPU: the stream packing of the sequence-stationary forward (rag-gesture_amd/seqfwd.py) against the indexing the kernel
uses (csrc/rg_seq.hip), written out element by element."""
import numpy as np
import torch


def _bf(t):
    return t.to(torch.bfloat16).float()


def test_pack_unit_is_the_mfma_operand_image(rg):
    SQ = rg.seqfwd
    W = torch.randn(512, 512)
    pk = SQ.pack_unit(W).float()            # [8 waves][64 fragments][64 lanes][8]
    Wb = _bf(W)
    rng = np.random.default_rng(0)
    for _ in range(2000):
        w, s, j, lane, e = (int(rng.integers(n)) for n in (8, 16, 4, 64, 8))
        nl, g = lane & 15, lane >> 4
        # kernel: fragment 4 s + j of wave w, lane (nl, g), element e = A[i = nl][k = 8 g + e] of block (j, s)
        assert pk[w, 4 * s + j, lane, e] == Wb[64 * w + 16 * j + nl, 32 * s + 8 * g + e]


def test_pack_kv_orders_heads_then_key_value(rg):
    SQ = rg.seqfwd
    Wk, Wv = torch.randn(512, 512), torch.randn(512, 512)
    pk = SQ.pack_kv(Wk, Wv).float()         # [8][128][64][8]
    src = (_bf(Wk), _bf(Wv))
    rng = np.random.default_rng(1)
    for _ in range(2000):
        w, h, kv, s, j2, lane, e = (int(rng.integers(n)) for n in (8, 2, 2, 16, 2, 64, 8))
        nl, g = lane & 15, lane >> 4
        frag = ((h * 2 + kv) * 16 + s) * 2 + j2          # consumption order: head, key | value, step, block of the head
        assert pk[w, frag, lane, e] == src[kv][64 * w + 32 * h + 16 * j2 + nl, 32 * s + 8 * g + e]


def test_a_fragments_enumerate_the_contraction_like_the_query_accumulators(rg):
    SQ = rg.seqfwd
    A = torch.randn(2, 3, 2, 16, 32, 32)    # [L][3][B][H][i][j]
    fr = SQ.a_fragments(A)                  # [L][3][B][8 waves][2 heads][2 blocks][64][8]
    assert fr.shape == (2, 3, 2, 8, 2, 2, 64, 8) and fr.dtype == torch.bfloat16
    rng = np.random.default_rng(2)
    for _ in range(2000):
        l, c, b, w, hh, jb, lane, e = (int(rng.integers(n)) for n in (2, 3, 2, 8, 2, 2, 64, 8))
        jj, g = lane & 15, lane >> 4
        i = 4 * g + e if e < 4 else 16 + 4 * g + e - 4
        a = A[l, c, b, 2 * w + hh, i, 16 * jb + jj]
        assert fr[l, c, b, w, hh, jb, lane, e].float() == _bf(a)


def test_unit_slots_are_the_headers(rg):
    """The unit slots of a layer are defined once, in include/rg_gesture.h (RG_SEQ_UPL, RG_SEQ_U_*): the values the kernels
    walk the streams by, and seqfwd.py packs by the same ones."""
    SQ, C = rg.seqfwd, rg.capi.header_constants()
    names = "KV KV2 Q SAO MIXX Q3_0 MIX_0 Q3_1 MIX_1 Q3_2 MIX_2 FF1_0 FF2_0 FF1_1 FF2_1 FFO".split()
    assert C["RG_SEQ_UPL"] == 16 and SQ.UPL == 16
    assert sorted(k for k in C if k.startswith("RG_SEQ_U_")) == sorted("RG_SEQ_U_" + n for n in names)
    for i, n in enumerate(names):
        assert C["RG_SEQ_U_" + n] == i and getattr(SQ, "U_" + n) == i, n
