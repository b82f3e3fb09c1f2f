"""Word prominence of one 10-minute recording (synthetic speech of tests/golden/prosody_fixture.py, 9.6 M samples, 60 001 frames):
  device_ms   device events around ProminenceEstimator.run_device (the four launches and the host's building and upload of the
              offset and word tables between them), ROUNDS rounds after a warm-up; run_wall_s is a host clock around
              ProminenceEstimator.run, which ends in its one read-back
  fixture_s   the float64 restatement (prosody_fixture.estimate, numpy) on the CPU of the same run, once, stage by stage
and the largest difference of the two answers' prominence values.  Prints one JSON line; --out FILE also writes it.

    python profiles/prosody_time.py [--out FILE] [--seconds 600]
"""
import argparse
import importlib
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=600.0)
    args = ap.parse_args()
    import numpy as np
    import torch
    rg = importlib.import_module("rag-gesture_amd")
    spec = importlib.util.spec_from_file_location("prosody_fixture", os.path.join(ROOT, "tests", "golden", "prosody_fixture.py"))
    fx = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fx)
    y, words = fx.speech_clip(11, int(args.seconds * 16000))
    est = rg.prosody.ProminenceEstimator()
    wave = torch.from_numpy(y).cuda()
    ev = lambda: torch.cuda.Event(enable_timing=True)
    out = dict(seconds=args.seconds, samples=int(y.size), frames=fx.n_frames(y.size), words=len(words), device_ms=[], run_wall_s=[])
    for r in range(ROUNDS + 1):
        a, b = ev(), ev()
        a.record()
        est.run_device([wave], [words])
        b.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = est.run([wave], [words])[0]
        wall = time.perf_counter() - t0
        if r:                                                  # (round 0 warms every code object)
            out["device_ms"].append(a.elapsed_time(b))
            out["run_wall_s"].append(wall)
    stages = {}
    t0 = time.perf_counter()
    fr = fx.frames(y)
    stages["frames"] = time.perf_counter() - t0
    sf, ef = fx.word_frames(words, fr["energy"].size)
    t0 = time.perf_counter()
    sg = fx.signal(fr["energy"], fr["nccf"], fr["logf0"], sf, ef, [w[0][0] for w in words], [w[0][1] for w in words])
    stages["signal"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    W = fx.cwt(sg["c"])
    stages["cwt"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    wd = fx.words_stage(W, sf, ef)
    stages["words"] = time.perf_counter() - t0
    out["fixture_s"] = sum(stages.values())
    out["fixture_stage_s"] = stages
    got = np.array([r[3] for r in rows])
    out["largest_prominence"] = float(wd["prominence"].max())
    # (end to end, so an early rounding difference may move a line: reported, not asserted -- the tests compare stage by stage)
    out["worst_prominence_difference"] = float(np.abs(got - wd["prominence"]).max())
    out["words_that_differ_by_more_than_1e-3"] = int((np.abs(got - wd["prominence"]) > 1e-3).sum())
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
