"""GPU: rg_text_diag_sim_many (every tie tier of a batch in one launch, one workgroup per (entry, query) pair) against torch on
the CPU with the kernel's arithmetic: fp32 products, a float64 sum, divided by n = min(Lq, Ld).  The kernel adds the same
K = n * 768 addends in another order, so per pair |difference| <= (K - 1) * 2^-53 * sum|product_i| / n: the worst case of any
summation order of the same addends (derived, not measured).  What does hold bit for bit: a pair's value does not depend on its
place in a launch, or on the launch.  Feature lengths around the queries' lengths (1, 2, 149, 150, 151), queries of 1, 7 and 150
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
    ref, off_cpu, feats_cpu = {}, np.concatenate([[0], np.cumsum(LENGTHS)]), feats.cpu()
    for qi, q in enumerate(queries):             # (entry, query) -> (float64 reference, bound), computed once
        q = q.cpu()
        for e, ld in enumerate(LENGTHS):
            n = min(q.shape[0], ld)
            prod = (q[:n] * feats_cpu[off_cpu[e]:off_cpu[e] + n]).double()          # fp32 products
            ref[(e, qi)] = (prod.sum() / n, float((n * DIM - 1) * 2.0 ** -53 * prod.abs().sum() / n))
    return h, feats, off, queries, ref


def _pairs(n):
    if n == 1:
        return [(4, 2)]
    if n == 5:
        return [(3, 0), (3, 1), (3, 1), (0, 2), (39, 0)]                      # entry 3 under two queries and twice under one
    rng = np.random.default_rng(5)
    p = [(int(e), int(q)) for e, q in zip(rng.integers(0, len(LENGTHS), n - 6), rng.integers(0, 3, n - 6))]
    return [(2, 1), (2, 2), (2, 2)] + p + [(0, 0), (4, 2), (38, 2)]


def _launch(h, feats, off, queries, pairs):
    """One launch over `pairs` into a buffer inside sentinels -> the whole buffer on the host (values at [8 : 8 + len(pairs)])."""
    qp = np.array([q.data_ptr() for q in queries], dtype=np.uint64)
    ql = np.array(LQ, dtype=np.int32)
    pe, pq = np.array([p[0] for p in pairs], dtype=np.int32), np.array([p[1] for p in pairs], dtype=np.int32)
    buf = torch.full((len(pairs) + 16,), SENTINEL, dtype=torch.float64).cuda()
    h.call("text_diag_sim_many", qp.ctypes.data, ql.ctypes.data, len(queries), pe.ctypes.data, pq.ctypes.data, len(pairs),
           feats, off, len(LENGTHS), DIM, buf[8:8 + len(pairs)])
    return buf.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("n_pairs", [1, 5, 300])
def test_many_equals_the_cpu_reference(table, n_pairs):
    h, feats, off, queries, ref = table
    pairs = _pairs(n_pairs)
    assert len(pairs) == n_pairs
    got = _launch(h, feats, off, queries, pairs)
    assert bool((got[:8] == SENTINEL).all()) and bool((got[8 + n_pairs:] == SENTINEL).all())
    got = got[8:8 + n_pairs]
    for p, v in zip(pairs, got):
        want, bound = ref[p]
        assert abs(float(v) - float(want)) <= bound, (p, float(v), float(want), bound)
    # bit level: the same pair twice in one launch, and again in a second launch (the list reversed), gives identical bits
    bits = got.view(torch.int64).tolist()
    first = {}
    assert all(first.setdefault(p, b) == b for p, b in zip(pairs, bits))
    assert n_pairs == 1 or len(first) < n_pairs
    again = _launch(h, feats, off, queries, pairs[::-1])[8:8 + n_pairs]
    assert again.view(torch.int64).tolist()[::-1] == bits


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
