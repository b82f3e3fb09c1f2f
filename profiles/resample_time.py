"""16 clips x 60 s of 48 kHz stereo PCM16 -> 16 kHz mono (NOTEBOOK.md section 20): rg_resample_poly through audio.Resampler, device
events around 20 launches at a time after a warm-up, next to scipy.signal.resample_poly with the same filter in 16 processes (one
clip each, decode included) on the same host.  Prints one JSON line; --out FILE also writes it.

    python profiles/resample_time.py [--out FILE]
"""
import argparse
import importlib
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_CLIPS, SECONDS, RATE = 16, 60, 48000
CLIPS = None


def host_one(i):
    import scipy.signal
    audio = importlib.import_module("rag-gesture_amd").audio
    up, down, _, h = audio.resample_filter(RATE)
    return scipy.signal.resample_poly(audio.decode_mono(CLIPS[i]), up, down, window=h / up).astype(np.float32)[:4]


def main():
    global CLIPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    CLIPS = [np.random.default_rng(100 + i).integers(-32768, 32768, (SECONDS * RATE, 2)).astype(np.int16) for i in range(N_CLIPS)]
    out = {}
    with multiprocessing.get_context("fork").Pool(16) as pool:          # (before this process touches the GPU; the clips are inherited)
        pool.map(host_one, range(N_CLIPS))                               # warm-up: imports, the filter
        t0 = time.perf_counter()
        pool.map(host_one, range(N_CLIPS), chunksize=1)
        out["scipy_16_processes_s"] = time.perf_counter() - t0
    import torch
    audio = importlib.import_module("rag-gesture_amd").audio
    res = audio.Resampler()
    clips = [(c, RATE) for c in CLIPS]
    y = res.run(clips)                                                   # warm-up: the table, the code object
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y = res.run(clips)
    torch.cuda.synchronize()
    out["run_wall_s"] = time.perf_counter() - t0                        # host packing + one copy from pageable memory + the launch
    staged = res.stage(RATE, 2, audio.PCM16, CLIPS)
    res.launch(staged)
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            res.launch(staged)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / 20.0)
    taps = res.table(RATE)[3]
    med = float(np.median(times))
    n_out = sum(int(t.shape[0]) for t in y)
    out.update(launch_ms=times, launch_ms_median=med, outputs=n_out, taps=taps,
               gflop_per_s=2.0 * taps * n_out / (med * 1e-3) / 1e9, source_gb_per_s=sum(c.nbytes for c in CLIPS) / (med * 1e-3) / 1e9)
    ref = audio.Resampler.reference(CLIPS[3][:5000], RATE)               # (its first 1600 outputs do not reach frame 5000)
    out["max_abs_err_first_1600_of_clip_3"] = float(np.abs(y[3][:1600].cpu().numpy() - ref[:1600]).max())
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
