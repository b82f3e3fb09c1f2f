"""Launch time of the grouped twin forward (rg_seq2_forward_many) at the flagship's co-batched shape: sessions of 64 clips
(16 sampling + 48 inverting, two step groups), L = 8, T = 43, device events around 20 launches, alone on the chip.
  grouped:   1, 2 and 4 sessions in one launch (64, 128, 256 workgroups), one stream;
  two lanes: one session on each of two streams at the same time (what the pipeline did before grouped chains).
python profiles/twin_many_time.py  ->  profiles/r11_twin_many_launch.txt"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

rg = importlib.import_module("rag-gesture_amd")
from oracle import denoiser as od  # noqa: E402

B, NA, T, N, REPS = 64, 16, 43, 4, 20
cfg = rg.synth.default_model_cfg(num_layers=8)
W = rg.denoiser.DenoiserWeights(rg.synth.synth_denoiser_state(0, cfg), cfg, rg.schedule.Schedule(), "cuda")
mm = torch.ones(B, T)
mm[:, [10, 21, 32]] = 0
sessions, xs = [], []
for k in range(N):
    data = rg.synth.synth_batch(B, seed=3 + k)
    sess = rg.denoiser.DenoiserSession(W, B, engine="seq", seq_duo=True, seq_twin=True)
    sess.set_conditions(data["word"], data["audio"], data["speaker_ids"], mm, od.make_query_masks(mm))
    sessions.append(sess)
    xs.append(torch.randn(B, T, 512, device="cuda"))
many = rg.denoiser.DenoiserSession.forward_many


def fn_all(fn, streams):
    if not streams:
        fn(None)
    for i, s in enumerate(streams):
        with torch.cuda.stream(s):
            fn(i)


def timed(fn, streams=()):
    """us per call of fn over REPS calls; with `streams`, fn(i) runs on streams[i] and the time is that of all of them."""
    cur = torch.cuda.current_stream()
    for _ in range(3):
        fn_all(fn, streams)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in streams:
        s.wait_stream(cur)
    for _ in range(REPS):
        fn_all(fn, streams)
    for s in streams:
        cur.wait_stream(s)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS


print("rg_seq2_forward_many, sessions of %d clips (%d + %d), L = 8, T = %d, %d launches per figure" % (B, NA, B - NA, T, REPS))
for n in (1, 2, 4):
    calls = [dict(x=xs[k], step=20, step_b=30, split=NA) for k in range(n)]
    for rep in range(3):
        us = timed(lambda _: many(sessions[:n], [dict(c) for c in calls]))
        print("grouped  n=%d (%3d workgroups) run %d: %8.1f us per launch, %7.1f us per session" % (n, n * B, rep, us, us / n), flush=True)
one = lambda i: sessions[i or 0].forward(xs[i or 0], 20, 30, NA)
for rep in range(3):
    us = timed(one)
    print("rg_seq2_forward alone (64 workgroups)   run %d: %8.1f us per launch" % (rep, us), flush=True)
streams = [torch.cuda.Stream(), torch.cuda.Stream()]
for rep in range(3):
    us = timed(one, streams)
    print("two lanes, one session each (2 x 64)    run %d: %8.1f us per pair of launches, %7.1f us per session" % (rep, us, us / 2), flush=True)
