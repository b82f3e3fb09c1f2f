"""The `motion` retrieval method at the benchmark's database size (NOTEBOOK.md, "Exemplars by a motion example"): 32 768
entries of random fp32 motion latents [4, 10, 512], 16 clips x 3 examples of 3 chunks = 48 queries, default weights (upper body
and hands).  Timed in one run, after three warm-up rounds, REPS repetitions each, medians:
  sweep_ms       rg_motion_scores_batched alone, 48 queries (latents, parameters and outputs resident), device events around the launch
  sweep_q1_ms    the same launch with ONE query: the table is staged once per launch whatever the number of queries, so the two
                 times differ by the queries' arithmetic, not by another pass over the table
  search_ms      the whole motion_retrieval_batch (validation, one example encode, sweep, selection, ranking with its
                 read-backs), device events around the call; search_wall_ms is a host clock around the same call
  numpy_ms       the float64 restatement of the 48 sweeps (tests/motion_retrieval_ref.py scores) on the host, over the first
                 --numpy-entries entries and scaled to the whole table (numpy_entries in the output says how many were computed)
  discourse_sweep_ms   the discourse sweep of the same session over the same entries, timed as bench.py's `roofline_retrieval`
                 times it (20 launches between two device events), for comparison
The warm-up also checks what is timed: over the first --numpy-entries entries the sweep's offsets equal the restatement's
wherever the fp32 bound decides them, and the scores agree within that bound.
sweep_bytes = the weighted parts of the table once; sweep_flops = 3 per term (subtract, multiply, add) of every S_p(o).
Bounds beside them: the 8 TB/s HBM peak bench.py uses and the 157 TFLOP/s fp32 vector peak (plain, unpacked fp32 reaches a third
of that at most: one subtraction and one fused multiply-add per term where the peak counts two packed fused multiply-adds).
Prints one JSON line and writes it to --out (default profiles/motion_retrieval_time.json).

    python profiles/motion_retrieval_time.py [--out FILE] [--entries N] [--reps R] [--numpy-entries M]
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
FP32_PEAK = 157.0e12       # FLOP/s, fp32 vector (and fp32 MFMA) peak of the MI355X
CLIPS, PER_CLIP, NQ, L, D = 16, 3, 3, 10, 512
WEIGHTS = (1.0, 1.0, 0.0, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_retrieval_time.json"))
    ap.add_argument("--entries", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--numpy-entries", type=int, default=2048)
    args = ap.parse_args()
    import numpy as np
    import torch
    import motion_retrieval_ref as ref
    rg = importlib.import_module("rag-gesture_amd")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    n, reps, m = args.entries, args.reps, min(args.numpy_entries, args.entries)
    samples = rg.synth.synth_retrieval_samples(n, feat_device="cuda")
    base = rg.retrieval.DiscourseIndex(rg.retrieval.build_db_dicts(samples), "cuda")
    gen = torch.Generator(device="cuda").manual_seed(133)
    lat = torch.randn(n, 4, L, D, device="cuda", generator=gen)
    mindex = rg.retrieval.MotionIndex(base, lat)
    Q = CLIPS * PER_CLIP
    qlats = [torch.randn(4, NQ, D, device="cuda", generator=gen) for _ in range(Q)]
    packed = rg.retrieval.pack_motion_queries(qlats, [WEIGHTS] * Q, [q % 25 for q in range(Q)], [0.0] * Q, "cuda")
    packed1 = rg.retrieval.pack_motion_queries(qlats[:1], [WEIGHTS], [0], [0.0], "cuda")
    score, top = (torch.empty(Q, n, dtype=dt, device="cuda") for dt in (torch.float64, torch.int32))

    def sweep(p=packed):
        mindex.h.call("motion_scores_batched", lat, n, L, D, mindex.spk, p["qlat"], p["q_off"], p["q_off_host"].ctypes.data,
                      p["params"], p["params_host"].ctypes.data, p["Q"], score, top, None)

    # ---- the whole search: a VAE for the example encode, examples cut from synthetic clips
    cfg, vae_cfgs = rg.synth.default_model_cfg(), rg.synth.synth_vae_cfgs(decoder_arch="all_encoder")
    gre = rg.vae.GestureRepEncoder(rg.synth.synth_full_state(0, cfg, vae_cfgs), vae_cfgs, "cuda", "bf16")
    src = rg.synth.synth_batch(CLIPS, seed=7, device="cuda")
    clips = []
    for b in range(CLIPS):
        ex = lambda f0: {k: src[k][b, f0:f0 + 15 * NQ] for k in rg.retrieval.MOTION_EXAMPLE_KEYS}
        clips.append(([(1.0 + 3 * i, 2.0 + 3 * i, ex(45 * i)) for i in range(PER_CLIP)], b % 25, torch.randn(24, 768, device="cuda")))
    search = lambda: rg.retrieval.motion_retrieval_batch(mindex, gre, clips)
    lat_host, spk_host = lat[:m].cpu().numpy(), mindex.spk[:m].cpu().numpy()
    q_host = [q.cpu().numpy() for q in qlats]
    restate = lambda: [ref.scores(lat_host, spk_host, q_host[q], WEIGHTS, q % 25, 0.0) for q in range(Q)]
    # ---- the discourse sweep of the same session (bench.py retrieval_roofline's way)
    dq = []
    for b in range(CLIPS):
        c = rg.synth.synth_query(b)
        dq += rg.retrieval.discourse_queries(c["discourse"], c["prominence"], c["speaker_id"])
    bufs = base.sweep_buffers(dq)
    # ---- warm-up, and what is timed is checked
    for _ in range(3):
        sweep()
        sweep(packed1)
        found = search()
        base.sweep_launch(bufs)
    sweep()
    torch.cuda.synchronize()
    want = restate()
    got_s, got_t = score[:, :m].cpu().numpy(), top[:, :m].cpu().numpy()
    bound = ref.sum_bound(NQ, D)
    for q in range(Q):
        s64, t64, _, d64 = want[q]
        srt = np.sort(d64, axis=1)
        decided = srt[:, 1] * (1 - 2 * bound) > srt[:, 0] * (1 + 2 * bound)
        assert np.array_equal(got_t[q][decided], t64[decided]), "the sweep's offsets and the restatement's differ at the timed size"
        assert np.all(np.abs(got_s[q] - s64) <= 2 * bound * s64), "the sweep's scores leave the fp32 bound at the timed size"
    assert all(len(v) == 10 for si, _, _ in found for v in si.values())
    ev = lambda: torch.cuda.Event(enable_timing=True)
    sweep_ms, sweep1_ms, search_ms, search_wall_ms, numpy_ms, disc_ms = [], [], [], [], [], []
    for _ in range(reps):                                      # they alternate: a drift of the box touches all of them
        a, b, c, d, e, f, g, h = (ev() for _ in range(8))
        a.record()
        sweep()
        b.record()
        torch.cuda.synchronize()
        c.record()
        sweep(packed1)
        d.record()
        torch.cuda.synchronize()
        e.record()
        t0 = time.perf_counter()
        search()
        wall = time.perf_counter() - t0
        f.record()
        torch.cuda.synchronize()
        g.record()
        for _ in range(20):
            base.sweep_launch(bufs)
        h.record()
        torch.cuda.synchronize()
        sweep_ms.append(a.elapsed_time(b))
        sweep1_ms.append(c.elapsed_time(d))
        search_ms.append(e.elapsed_time(f))
        search_wall_ms.append(wall * 1e3)
        disc_ms.append(g.elapsed_time(h) / 20)
    for _ in range(3):
        t0 = time.perf_counter()
        restate()
        numpy_ms.append((time.perf_counter() - t0) * 1e3 * n / m)
    med = statistics.median
    parts = sum(1 for w in WEIGHTS if w > 0)
    sweep_bytes = n * parts * L * D * 4
    sweep_flops = 3 * Q * n * parts * (L - NQ + 1) * NQ * D
    ach_b, ach_f = sweep_bytes / (med(sweep_ms) * 1e-3), sweep_flops / (med(sweep_ms) * 1e-3)
    db_bytes = sum(t.numel() * t.element_size() for t in (base.spk, base.rel_off, base.rel_sense, base.rel_conn, base.rel_prom))
    disc_alg = len(dq) * (db_bytes + n * 12)
    out = dict(entries=n, queries=Q, chunks_per_query=NQ, weights=list(WEIGHTS), reps=reps,
               sweep_ms=round(med(sweep_ms), 4), sweep_ms_min_max=[round(min(sweep_ms), 4), round(max(sweep_ms), 4)],
               sweep_q1_ms=round(med(sweep1_ms), 4), sweep_q1_ms_min_max=[round(min(sweep1_ms), 4), round(max(sweep1_ms), 4)],
               sweep_ms_per_query_beyond_the_first=round((med(sweep_ms) - med(sweep1_ms)) / (Q - 1), 5),
               sweep_bytes=sweep_bytes, sweep_achieved_GBps=round(ach_b / 1e9, 1), hbm_peak_GBps=HBM_PEAK / 1e9,
               sweep_frac_of_hbm_peak=round(ach_b / HBM_PEAK, 5),
               sweep_q1_achieved_GBps=round(sweep_bytes / (med(sweep1_ms) * 1e-3) / 1e9, 1),
               sweep_flops=sweep_flops, sweep_achieved_GFLOPs=round(ach_f / 1e9, 1), fp32_peak_GFLOPs=FP32_PEAK / 1e9,
               sweep_frac_of_fp32_peak=round(ach_f / FP32_PEAK, 5),
               search_ms=round(med(search_ms), 3), search_wall_ms=round(med(search_wall_ms), 3),
               numpy_ms=round(med(numpy_ms), 1), numpy_entries=m,
               discourse_sweep_ms=round(med(disc_ms), 4), discourse_queries=len(dq),
               discourse_sweep_achieved_GBps=round(disc_alg / (med(disc_ms) * 1e-3) / 1e9, 1))
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
