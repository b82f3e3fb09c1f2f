"""GPU: rg_text_diag_sim_many (every tie tier of a batch in one launch, one workgroup per (entry, query) pair) against
rg_text_diag_sim called once per query -- the two kernels share the per-candidate arithmetic, so the float64 results must be
EQUAL, bit for bit (torch.equal).  Feature lengths around the queries' lengths (1, 2, 149, 150, 151), queries of 1, 7 and 150
tokens, pair lists of 1, 5 and 300 pairs with the same candidate under two queries and twice under one; the output buffer sits
inside sentinels."""
import numpy as np
import pytest
import torch

DIM = 768
LENGTHS = [1, 2, 149, 150, 151, 3, 8, 17, 48, 64, 100, 7, 6, 150, 1, 33, 75, 149, 12, 5,
           2, 151, 90, 10, 20, 30, 40, 50, 60, 70, 80, 9, 11, 13, 128, 15, 16, 4, 150, 19]
LQ = [1, 7, 150]
SENTINEL = -777.25


@pytest.fixture(scope="module")
def table(rg):
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(sum(LENGTHS), DIM, generator=g).cuda()
    off = torch.tensor(np.concatenate([[0], np.cumsum(LENGTHS)]), dtype=torch.int64).cuda()
    queries = [torch.randn(l, DIM, generator=g).cuda() for l in LQ]
    h = rg.capi.get_handle()
    ref = {}                                     # (entry, query) -> float64 of rg_text_diag_sim, computed once per query
    for qi, q in enumerate(queries):
        cand = torch.arange(len(LENGTHS), dtype=torch.int32).cuda()
        out = torch.empty(len(LENGTHS), dtype=torch.float64).cuda()
        h.call("text_diag_sim", q, q.shape[0], feats, off, cand, len(LENGTHS), DIM, out)
        for e, v in enumerate(out.cpu()):
            ref[(e, qi)] = v
    return h, feats, off, queries, ref


def _pairs(n):
    if n == 1:
        return [(4, 2)]
    if n == 5:
        return [(3, 0), (3, 1), (3, 1), (0, 2), (39, 0)]                      # entry 3 under two queries and twice under one
    rng = np.random.default_rng(5)
    p = [(int(e), int(q)) for e, q in zip(rng.integers(0, len(LENGTHS), n - 6), rng.integers(0, 3, n - 6))]
    return [(2, 1), (2, 2), (2, 2)] + p + [(0, 0), (4, 2), (38, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_pairs", [1, 5, 300])
def test_many_equals_one_launch_per_query(table, n_pairs):
    h, feats, off, queries, ref = table
    pairs = _pairs(n_pairs)
    assert len(pairs) == n_pairs
    qp = np.array([q.data_ptr() for q in queries], dtype=np.uint64)
    ql = np.array(LQ, dtype=np.int32)
    pe, pq = np.array([p[0] for p in pairs], dtype=np.int32), np.array([p[1] for p in pairs], dtype=np.int32)
    buf = torch.full((n_pairs + 16,), SENTINEL, dtype=torch.float64).cuda()
    h.call("text_diag_sim_many", qp.ctypes.data, ql.ctypes.data, len(queries), pe.ctypes.data, pq.ctypes.data, n_pairs,
           feats, off, len(LENGTHS), DIM, buf[8:8 + n_pairs])
    got = buf.cpu()
    assert torch.equal(got[8:8 + n_pairs], torch.stack([ref[p] for p in pairs]))
    assert bool((got[:8] == SENTINEL).all()) and bool((got[8 + n_pairs:] == SENTINEL).all())


@pytest.mark.gpu
def test_many_refuses_bad_pairs(rg, table):
    """Every index is checked on the host before anything is launched."""
    h, feats, off, queries, _ = table
    qp = np.array([q.data_ptr() for q in queries], dtype=np.uint64)
    ql = np.array(LQ, dtype=np.int32)
    out = torch.empty(2, dtype=torch.float64).cuda()
    for pe, pq in (([0, len(LENGTHS)], [0, 0]), ([0, -1], [0, 0]), ([0, 1], [0, 3]), ([0, 1], [-1, 0])):
        pe, pq = np.array(pe, dtype=np.int32), np.array(pq, dtype=np.int32)
        with pytest.raises(rg.capi.RgError, match="pair out of range"):
            h.call("text_diag_sim_many", qp.ctypes.data, ql.ctypes.data, 3, pe.ctypes.data, pq.ctypes.data, 2, feats, off,
                   len(LENGTHS), DIM, out)
