"""CPU: SMPL-X joint metrics (rag-gesture_amd/evaluation.py) -- model-file loading and rejection, the host GAHR / align
bookkeeping against the reference's scores (tests/golden/joint_metrics.npz, made by make_joint_metrics_golden.py), onset
sources, multimodality file discovery, and the new C-ABI symbols and argument blocks."""
import ctypes
import importlib
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "joint_metrics.npz")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


jf = _load("joint_fixture")


@pytest.fixture(scope="module")
def rg():
    return importlib.import_module("rag-gesture_amd")


@pytest.fixture(scope="module")
def ev(rg):
    return rg.evaluation


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_model_loading_accepts_variants(ev):
    m = jf.smplx_model()
    a = ev.load_smplx_model(m)
    assert a["parents"][0] == -1 and list(a["parents"][1:]) == jf.SMPLX_PARENTS[1:]
    assert a["J_dirs"].shape == (55, 3, 300)
    assert np.allclose(a["J_template"], m["J_regressor"] @ m["v_template"], rtol=0, atol=1e-15)
    assert np.array_equal(a["pose_mean"][75:120], m["hands_meanl"]) and not a["pose_mean"][:75].any()
    m2 = dict(m, kintree_table=m["kintree_table"].copy())
    m2["kintree_table"][0, 0] = -1
    assert np.array_equal(ev.load_smplx_model(m2)["parents"], a["parents"])
    flat = {k: v for k, v in m.items() if not k.startswith("hands_mean")}
    assert not ev.load_smplx_model(flat, flat_hand_mean=True)["pose_mean"].any()


def test_model_file_round_trip(ev, tmp_path):
    p = str(tmp_path / "SMPLX_NEUTRAL_2020.npz")
    np.savez(p, **jf.smplx_model())
    a, b = ev.load_smplx_model(p), ev.load_smplx_model(jf.smplx_model())
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("change, msg", [
    (lambda m: m.pop("J_regressor"), "missing key J_regressor"),
    (lambda m: m.update(kintree_table=m["kintree_table"][:, :54]), r"kintree_table has shape \(2, 54\)"),
    (lambda m: m["kintree_table"].__setitem__((0, 5), 7), "parent of joint 5 is 7"),
    (lambda m: m.update(shapedirs=m["shapedirs"][..., :299]), r"shapedirs has shape .*>= 300"),
    (lambda m: m["kintree_table"].__setitem__((0, 0), 3), "root entry"),
    (lambda m: m.pop("hands_meanr"), "missing key hands_meanr"),
    (lambda m: m.update(v_template=m["v_template"][:-1]), "v_template has shape"),
])
def test_model_loading_rejects(ev, change, msg):
    m = jf.smplx_model()
    m["kintree_table"] = m["kintree_table"].copy()
    change(m)
    with pytest.raises(ev.SMPLXModelError, match=msg):
        ev.load_smplx_model(m)
    assert issubclass(ev.SMPLXModelError, ValueError)


def _beat_lists(gold, tag, i):
    flat = gold["beats_%s_%d" % (tag, i)]
    return [row[row >= 0] for row in flat]


def test_align_bookkeeping_matches_reference(ev, gold):
    n = jf.EVAL_N
    tot = {"pred": 0.0, "gt": 0.0}
    for i in range(jf.N_CLIPS):
        on = gold["onsets_%d" % i]
        for tag in ("pred", "gt"):
            a = ev.calculate_align(on, _beat_lists(gold, tag, i))
            assert a == pytest.approx(float(gold["align_%s_%d" % (tag, i)]), rel=1e-12, abs=1e-15)
            tot[tag] += a * (n - 2 * ev.ALIGN_MASK)
    den = n * jf.N_CLIPS - 2 * jf.N_CLIPS * ev.ALIGN_MASK
    assert tot["pred"] / den == pytest.approx(float(gold["score_align"]), rel=1e-12)
    assert tot["gt"] / den == pytest.approx(float(gold["score_gt_align"]), rel=1e-12)


def test_gahr_edge_cases(ev):
    assert ev.gahr([], [0.5]) == 0.0                                  # no motion beat: exp(-inf)
    assert ev.gahr([0.5], [0.5, 0.5]) == 1.0
    with pytest.raises(ZeroDivisionError):
        ev.gahr([0.1], [])


def test_onset_sources(ev, tmp_path, monkeypatch):
    f = str(tmp_path / "test" / "3_scott_0_3_3" / "pred_motion.npz")
    assert ev.clip_key(f) == "test/3_scott_0_3_3"
    get, why = ev.onset_source({"test/3_scott_0_3_3": [0.25, 1.5]})
    assert why is None and np.array_equal(get(f, 64), [0.25, 1.5])
    with pytest.raises(ValueError, match="no onsets for clip test/4_wayne"):
        get(str(tmp_path / "test" / "4_wayne_0_4_4" / "pred_motion.npz"), 64)
    monkeypatch.setitem(sys.modules, "librosa", None)                 # import librosa -> ImportError
    get, why = ev.onset_source(None)
    assert get is None and "librosa" in why


def test_mm_file_discovery_and_speaker_filter(ev, tmp_path):
    for name, reps in (("mm/0_scott_1_0", 5), ("mm/1_wayne_1_1", 3), ("mm/2_scott_1_2", 2)):
        for k in range(reps):
            d = tmp_path / (name + "_rep%d" % k)
            d.mkdir(parents=True)
            (d / "pred_motion.npz").write_bytes(b"")
    groups = ev.find_mm_groups(str(tmp_path))
    assert [os.path.basename(d) for d, _ in groups] == ["0_scott_1_0_rep0", "1_wayne_1_1_rep0", "2_scott_1_2_rep0"]
    assert [len(f) for _, f in groups] == [5, 3, 2]
    assert groups[1][1][-1].endswith(os.path.join("1_wayne_1_1_rep2", "pred_motion.npz"))
    assert [os.path.basename(d) for d, _ in ev.find_mm_groups(str(tmp_path), "scott")] == ["0_scott_1_0_rep0", "2_scott_1_2_rep0"]


def test_multimodality_rejects_bad_groups(ev):
    clip = np.zeros((64, 165), np.float32)
    with pytest.raises(ValueError, match="g1: 1 samples"):
        ev.multimodality(None, [[clip, clip], [clip]], names=["g0", "g1"])
    with pytest.raises(ValueError, match="group 0: samples of different lengths"):
        ev.multimodality(None, [[clip, clip[:40]]])


def test_header_symbols_and_struct_layout(rg):
    syms = rg.capi.header_symbols()
    for s in ("rg_smplx_joints", "rg_joint_clip_stats", "rg_pair_distance_sums"):
        assert s in syms
    assert rg.capi.header_version() >= 113
    protos = rg.capi.header_prototypes()
    assert protos["rg_smplx_joints"][1] == [ctypes.c_void_p] * 3


def test_golden_fixture_regenerates(gold):
    """The fixture stream is what the golden was made from (the clips feed the GPU end-to-end test)."""
    inp = jf.inputs(int(gold["seed"]))
    for i in range(jf.N_CLIPS):
        assert np.array_equal(jf.onset_times(inp, i), gold["onsets_%d" % i])
    assert list(gold["clip_names"]) == jf.clip_names()
    m = jf.smplx_model()
    sm = _load("smplx_fk")
    assert np.allclose(jf.avg_vel(inp, sm.load_model(m)), gold["avg_vel"], rtol=1e-12, atol=0)
