"""CPU: SRGR (rag-gesture_amd/evaluation.py) -- the host resampling of sem_score against the vectors the reference's
F.interpolate produced (tests/golden/srgr.npz, made by make_srgr_golden.py) and its edge cases, the new C-ABI symbol and
argument block, the command-line flags, and the golden file against the fixture stream."""
import ctypes
import importlib
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "srgr.npz")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


sf = _load("srgr_fixture")


@pytest.fixture(scope="module")
def rg():
    return importlib.import_module("rag-gesture_amd")


@pytest.fixture(scope="module")
def ev(rg):
    return rg.evaluation


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_resampling_matches_the_reference_vectors(ev, gold):
    seed = int(gold["seed"])
    for i, s in enumerate(sf.sem_scores(seed, sf.MOTION_FPS)):
        got = ev.sem_at_pose_rate(s, sf.MOTION_FPS)
        want = gold["sem30_%d" % i]
        assert got.dtype == np.float32 and got.shape == want.shape == (2 * s.shape[0],)
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
    for i, s in enumerate(sf.sem_scores(seed, 30)):
        assert np.array_equal(ev.sem_at_pose_rate(s, 30), gold["sem30_30_%d" % i])
    # the fixture has the vectors the issue asks for: one all zero, one that resamples to exactly n, one to more
    lens = [gold["sem30_%d" % i].shape[0] for i in range(sf.N_CLIPS)]
    assert lens[0] == sf.EVAL_N and max(lens) > sf.EVAL_N and not gold["sem30_%d" % sf.ZERO_CLIP].any()
    vals = np.concatenate(sf.sem_scores(seed, sf.MOTION_FPS))
    assert set(np.round(vals * 10).astype(int).tolist()) <= set(range(11)) and np.array_equal(vals, np.float32(np.round(vals * 10) / 10))


def test_resampling_edge_cases(ev):
    one = ev.sem_at_pose_rate([0.4], 15)
    assert one.dtype == np.float32 and np.array_equal(one, np.float32([0.4, 0.4]))
    x = np.float32([0.1, 0.9, 0.0, 0.3, 1.0])
    same = ev.sem_at_pose_rate(x, 30)
    assert same.dtype == np.float32 and np.array_equal(same, x)
    for fps in (15, 10, 6):
        y = ev.sem_at_pose_rate(x, fps)
        k = 30 // fps
        assert y.shape == (5 * k,) and y[0] == x[0] and y[-1] == x[-1]
        # a restatement, float64: output i reads source position (i + 0.5) / k - 0.5
        src = np.clip((np.arange(5 * k) + 0.5) / k - 0.5, 0.0, None)
        lo = np.floor(src).astype(int)
        hi = np.minimum(lo + 1, 4)
        want = (1 - (src - lo)) * x[lo].astype(np.float64) + (src - lo) * x[hi].astype(np.float64)
        np.testing.assert_allclose(y, want, rtol=1e-6, atol=0)
    assert ev.sem_at_pose_rate(np.zeros(0, np.float32), 15).shape == (0,)
    for bad in (20, 7, 45, 0):
        with pytest.raises(ValueError, match="multiple of motion_fps"):
            ev.sem_at_pose_rate(x, bad)
    with pytest.raises(ValueError, match="1-D"):
        ev.sem_at_pose_rate(np.zeros((2, 3)), 15)


def test_header_symbol_and_struct_layout(rg):
    assert "rg_srgr_clip_sums" in rg.capi.header_symbols()
    assert rg.capi.header_version() >= 116
    assert rg.capi.header_prototypes()["rg_srgr_clip_sums"] == (ctypes.c_int, [ctypes.c_void_p] * 3)
    lib = rg.capi.load_library()
    assert hasattr(lib, "rg_srgr_clip_sums") and lib.rg_version() == rg.capi.header_version()


def test_command_line_flags(ev):
    ap = ev.build_parser()
    a = ap.parse_args(["folder", "--e_path", "e.bin"])
    assert a.sem_scores is None and a.motion_fps == 15
    a = ap.parse_args(["folder", "--e_path", "e.bin", "--smplx_path", "m.npz", "--sem_scores", "sem.npz", "--motion_fps", "30"])
    assert a.sem_scores == "sem.npz" and a.motion_fps == 30
    with pytest.raises(SystemExit):                                   # SRGR is computed on the SMPL-X joints
        ev.main(["folder", "--e_path", "e.bin", "--sem_scores", "sem.npz"])


def test_sem_source(ev, tmp_path):
    f = str(tmp_path / "test" / "3_scott_0_3_3" / "pred_motion.npz")
    scores = {"test/3_scott_0_3_3": np.float32([0.0, 0.5, 1.0])}
    assert np.array_equal(ev.sem_source(scores)(f), scores["test/3_scott_0_3_3"])
    np.savez(str(tmp_path / "sem.npz"), **scores)
    get = ev.sem_source(str(tmp_path / "sem.npz"))
    assert np.array_equal(get(f), scores["test/3_scott_0_3_3"])
    with pytest.raises(ValueError, match="no sem scores for clip test/4_wayne_0_4_4"):
        get(str(tmp_path / "test" / "4_wayne_0_4_4" / "pred_motion.npz"))


def test_golden_matches_the_fixture(gold):
    """The golden holds what the issue asks for, and belongs to the fixture stream the GPU tests rebuild."""
    assert list(gold["clip_names"]) == sf.clip_names() and sf.N_CLIPS >= 4
    assert float(gold["margin"]) >= 1e-3 and 0.2 < float(gold["share"]) < 0.8
    n = sf.EVAL_N
    assert gold["joints_pred"].shape == gold["joints_gt"].shape == (2, n, 165) and gold["joints_pred"].dtype == np.float32
    assert gold["count"].dtype == np.int64 and gold["count"].sum() == round(float(gold["share"]) * n * sf.N_CLIPS * 55)
    for tag in ("", "_30"):
        rate = gold["rate" + tag]
        assert rate[sf.ZERO_CLIP] == 0.0 and (np.delete(rate, sf.ZERO_CLIP) > 0).all()
        assert rate.sum() * n / (n * sf.N_CLIPS) == pytest.approx(float(gold["score" + tag]), rel=1e-12)
    # the stored joints give the stored counts, and none of their joint-frames is nearer the threshold than the margin
    d = np.abs(gold["joints_pred"].astype(np.float64) - gold["joints_gt"]).reshape(2, n, 55, 3).sum(-1)
    assert [(x < 0.3).sum() for x in d] == gold["count"][:2].tolist()
    assert np.abs(d - 0.3).min() >= float(gold["margin"]) - 1e-6
    assert os.path.getsize(GOLD) < 128 * 1024
