"""CPU: `bench.py --dump-outputs DIR` writes the last timed batch's arrays as DIR/<name>.npy (float32, float64 kept,
integers as float64) and keeps all files together under its byte limit by writing a fixed, seeded sample of a large array."""
import importlib.util
import os
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    bench.torch = torch       # (main() imports torch after the launch decision)
    return bench


def test_dump_writes_every_array_of_the_last_batch(tmp_path):
    bench = _bench()
    g = torch.Generator().manual_seed(0)
    out = dict(pred_upper=torch.randn(2, 150, 78, generator=g).bfloat16(), prev_latentout=torch.randn(2, 43, 512, generator=g),
               score=torch.randn(5, generator=g, dtype=torch.float64), rows=torch.arange(7), done_stream=None)
    wl = types.SimpleNamespace(kind="guided", last_out=out)
    names = bench.dump_outputs(wl, str(tmp_path / "d"))
    assert names == ["pred_upper", "prev_latentout", "rows", "score"]
    assert sorted(os.listdir(tmp_path / "d")) == [n + ".npy" for n in names]
    a = np.load(tmp_path / "d" / "pred_upper.npy")
    assert a.dtype == np.float32 and np.array_equal(a, out["pred_upper"].float().numpy())
    assert np.array_equal(np.load(tmp_path / "d" / "prev_latentout.npy"), out["prev_latentout"].numpy())
    s = np.load(tmp_path / "d" / "score.npy")
    assert s.dtype == np.float64 and np.array_equal(s, out["score"].numpy())
    r = np.load(tmp_path / "d" / "rows.npy")
    assert r.dtype == np.float64 and np.array_equal(r, np.arange(7))


def test_dump_samples_what_exceeds_the_limit(tmp_path):
    bench = _bench()
    bench.DUMP_LIMIT = 4096
    big = torch.arange(10000, dtype=torch.float32).reshape(100, 100)
    small = torch.ones(10)
    wl = types.SimpleNamespace(kind="base", last_out=dict(a_big=big, b_small=small))
    bench.dump_outputs(wl, str(tmp_path / "x"))
    bench.dump_outputs(wl, str(tmp_path / "y"))
    a = np.load(tmp_path / "x" / "a_big.npy")
    assert a.ndim == 1 and a.nbytes <= 2048 and np.all(np.diff(a) > 0) and set(a) <= set(range(10000))
    assert np.array_equal(a, np.load(tmp_path / "y" / "a_big.npy"))        # the same sample every time
    assert np.array_equal(np.load(tmp_path / "x" / "b_small.npy"), small.numpy())
    total = sum(os.path.getsize(tmp_path / "x" / f) - 128 for f in os.listdir(tmp_path / "x"))   # (128-byte .npy headers)
    assert total <= bench.DUMP_LIMIT


def test_dump_longform_writes_every_clip(tmp_path):
    bench = _bench()
    last = {c: dict(poses=np.full((300, 165), c, np.float32), expressions=np.zeros((300, 100), np.float32),
                    trans=np.zeros((300, 3), np.float32), latents=[None], windows=[(0, 150)]) for c in range(2)}
    wl = types.SimpleNamespace(kind="longform", last=last)
    names = bench.dump_outputs(wl, str(tmp_path))
    assert names == ["clip00_expressions", "clip00_poses", "clip00_trans", "clip01_expressions", "clip01_poses", "clip01_trans"]
    assert np.array_equal(np.load(tmp_path / "clip01_poses.npy"), last[1]["poses"])
