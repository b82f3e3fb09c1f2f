"""The `prosody` retrieval method at the benchmark's database size (NOTEBOOK.md, "Exemplars by word prominence"): 32 768
entries of about 25 timed words each over a 2 000-word vocabulary, 16 clips x 3 query words = 48 queries.  Timed in one run,
after a warm-up, REPS repetitions each, medians:
  sweep_ms    rg_prosody_scores_batched alone (similarity rows, parameters and outputs resident), device events around the launch
  search_ms   the whole prosody_retrieval_batch (query selection, 48 similarity launches, sweep, selection, ranking with its
              read-backs), device events around the call; search_wall_ms is a host clock around the same call (it ends in a
              read-back, so the device is idle when it returns); sims_ms is its similarity part alone (one rg_partial_ratio
              launch per distinct query word), device events
  numpy_ms    the float64 restatement of the 48 sweeps (tests/prosody_retrieval_ref.py scores, whole-array numpy), host clock
The warm-up also checks what is timed: the sweep's scores equal the restatement's as float64 bits and its word indices exactly.
sweep_bytes = the word table once + the similarity rows and parameters + a float64 score and an int32 index per (query, entry);
achieved = sweep_bytes / sweep time, beside the 8 TB/s HBM peak bench.py prices `roofline_retrieval` against.
Prints one JSON line and writes it to --out (default profiles/prosody_retrieval_time.json).

    python profiles/prosody_retrieval_time.py [--out FILE] [--entries N] [--reps R]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK = 8.0e12          # B/s, as bench.py
CLIPS, VOCAB, FEAT_ROWS, DIM = 16, 2000, 6, 768


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prosody_retrieval_time.json"))
    ap.add_argument("--entries", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    import numpy as np
    import torch
    import prosody_retrieval_ref as ref
    rg = importlib.import_module("rag-gesture_amd")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    n, reps = args.entries, args.reps
    g = np.random.Generator(np.random.PCG64(132))
    vocab = ["w%04d" % k if k % 3 else "word%dx" % k for k in range(VOCAB)]
    names = ["%d_e_0_%d/0" % (e % 25, e) for e in range(n)]
    counts = g.integers(10, 41, size=n)                         # 25 words an entry on average
    entries, speakers = [], (np.arange(n) % 25).tolist()
    for e in range(n):
        k = int(counts[e])
        start = np.cumsum(g.uniform(0.05, 0.4, size=k))
        dur = g.uniform(0.1, 0.5, size=k)
        prom = g.uniform(0, 3, size=k)
        code = g.integers(0, VOCAB, size=k)
        entries.append([(vocab[int(code[j])], float(start[j]), float(start[j] + dur[j]), None if j % 11 == 10 else float(prom[j]))
                        for j in range(k)])
    feats = torch.randn(n * FEAT_ROWS, DIM, device="cuda")
    db = dict(idx_2_sense={nm: [speakers[e]] for e, nm in enumerate(names)}, idx_2_prominence={nm: {} for nm in names},
              idx_2_text={nm: (feats[e * FEAT_ROWS:(e + 1) * FEAT_ROWS], speakers[e]) for e, nm in enumerate(names)},
              idx_2_wordprom={nm: entries[e] for e, nm in enumerate(names)})
    pindex = rg.retrieval.ProsodyIndex(db, rg.retrieval.DiscourseIndex(db, "cuda"))
    clips = []
    for c in range(CLIPS):
        t = np.cumsum(g.uniform(0.3, 0.6, size=20))
        clips.append(([(vocab[int(g.integers(0, VOCAB))], float(t[j]), float(t[j] + g.uniform(0.1, 0.3)), float(g.uniform(0, 3)))
                       for j in range(20)], c % 25, torch.randn(24, DIM, device="cuda")))
    queries = []
    for prom, spk, _ in clips:
        qb, proms = rg.retrieval.prosody_queries(prom)
        queries += [(qb[i][0], proms[i], qb[i][3] - qb[i][2], spk) for i in range(len(qb))]
    Q = len(queries)
    assert Q == 3 * CLIPS
    # ---- resident operands of the sweep alone
    sim = pindex.fuzzy.similarities([q[0] for q in queries])
    par = torch.tensor([[p, d, float(s)] for _, p, d, s in queries], dtype=torch.float64, device="cuda")
    score = torch.empty(Q, n, dtype=torch.float64, device="cuda")
    top = torch.empty(Q, n, dtype=torch.int32, device="cuda")

    def sweep():
        pindex.h.call("prosody_scores_batched", pindex.spk, pindex.word_off, pindex.word_off_host.ctypes.data, pindex.word_code,
                      pindex.word_prom, pindex.word_dur, n, pindex.n_words, sim, sim.shape[1], par, Q, score, top)

    search = lambda: rg.retrieval.prosody_retrieval_batch(pindex, clips)
    table = ref.Table(entries, speakers)
    sim_host = sim.cpu().numpy()
    restate = lambda: [ref.scores(table, sim_host[q], queries[q][1], queries[q][2], queries[q][3]) for q in range(Q)]
    # ---- warm-up, and what is timed is checked
    for _ in range(3):
        sweep()
        found = search()
    torch.cuda.synchronize()
    want = restate()
    got_s, got_t = score.cpu().numpy(), top.cpu().numpy()
    bit_equal = all(got_s[q].tobytes() == want[q][0].tobytes() and np.array_equal(got_t[q], want[q][1]) for q in range(Q))
    assert bit_equal, "the sweep and its restatement differ at the timed size"
    assert all(len(v) == 10 for si, _, _ in found for v in si.values())
    ev = lambda: torch.cuda.Event(enable_timing=True)
    words = list(dict.fromkeys(q[0] for q in queries))
    sweep_ms, search_ms, search_wall_ms, numpy_ms, sims_ms = [], [], [], [], []
    for _ in range(reps):                                      # the three alternate: a drift of the box touches all of them
        a, b, c, d, e, f = ev(), ev(), ev(), ev(), ev(), ev()
        a.record()
        sweep()
        b.record()
        torch.cuda.synchronize()
        e.record()
        pindex.fuzzy.similarities(words)
        f.record()
        torch.cuda.synchronize()
        c.record()
        t0 = time.perf_counter()
        search()
        wall = time.perf_counter() - t0
        d.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        restate()
        numpy_ms.append((time.perf_counter() - t0) * 1e3)
        sweep_ms.append(a.elapsed_time(b))
        sims_ms.append(e.elapsed_time(f))
        search_ms.append(c.elapsed_time(d))
        search_wall_ms.append(wall * 1e3)
    nbytes = lambda *ts: sum(t.numel() * t.element_size() for t in ts)
    table_bytes = nbytes(pindex.spk, pindex.word_off, pindex.word_code, pindex.word_prom, pindex.word_dur)
    sweep_bytes = table_bytes + nbytes(sim, par) + Q * n * 12
    med = statistics.median
    ach = sweep_bytes / (med(sweep_ms) * 1e-3)
    out = dict(entries=n, words=pindex.n_words, vocab=len(pindex.vocab), queries=Q, reps=reps, bit_equal=bit_equal,
               sweep_ms=round(med(sweep_ms), 4), sweep_ms_min_max=[round(min(sweep_ms), 4), round(max(sweep_ms), 4)],
               search_ms=round(med(search_ms), 3), search_wall_ms=round(med(search_wall_ms), 3),
               sims_ms=round(med(sims_ms), 3), distinct_query_words=len(words),
               numpy_ms=round(med(numpy_ms), 1), table_bytes=table_bytes, sweep_bytes=sweep_bytes,
               sweep_achieved_GBps=round(ach / 1e9, 1), hbm_peak_GBps=HBM_PEAK / 1e9, sweep_frac_of_hbm_peak=round(ach / HBM_PEAK, 5),
               word_evaluations=Q * pindex.n_words)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
