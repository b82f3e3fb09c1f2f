"""No GPU: the host side of rg.dataset (raw SMPL-X recordings -> model inputs) against the float64 restatement of
mogen/datasets/beatx_dataset.py in tests/golden/dataset_fixture.py, and the fixture's own conditions."""
import ctypes
import importlib
import importlib.util
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fx = _load("dataset_fixture")
JOINT_BOUND = 1e-5               # the joint bound of tests/test_dataset_gpu.py


@pytest.fixture(scope="module")
def ds_mod(rg):
    return rg.dataset


class _HostPreprocessor:
    """What SMPLXClipDataset needs of a preprocessor before the first sample is read (no device)."""
    pose_fps, stride, device = fx.POSE_FPS, fx.STRIDE, "cpu"

    def strided_frames(self, n_raw):
        return -(-n_raw // self.stride)

    def prepare(self, clips):
        raise AssertionError("the CPU tests read no sample")


def _clips(ds_mod, annotations=None, audio=None):
    return [ds_mod.RawClip(r["name"], r["poses"], r["trans"], r["expressions"], r["betas"], sid,
                           annotations=None if annotations is None else annotations[i], audio=None if audio is None else audio[i])
            for i, (r, sid) in enumerate(zip(fx.recordings(), fx.SPEAKER_IDS))]


def test_module_is_exposed(rg):
    assert rg.dataset.SMPLXClipDataset and rg.dataset.ClipPreprocessor and rg.dataset.window_table and rg.dataset.RawClip


RELEASED = dict(pose_fps=15, pose_length=150, stride=5, clean_first_seconds=0, clean_final_seconds=0)


@pytest.mark.parametrize("mode", ["train", "test", "full"])
@pytest.mark.parametrize("n_frames", [0, 1, 31, 149, 150, 151, 164, 165, 166, 451, 1000])
def test_window_table_released_config(ds_mod, mode, n_frames):
    got = ds_mod.window_table(n_frames, mode=mode, **RELEASED)
    assert got == fx.window_table(n_frames, mode=mode, **RELEASED)
    assert all(0 <= s < e <= n_frames for s, e in got)
    if mode != "full":
        assert all(e - s == 150 for s, e in got)


def test_window_table_known_counts(ds_mod):
    wt = ds_mod.window_table
    assert wt(149, **RELEASED) == [] and wt(31, **RELEASED) == [] and wt(1, **RELEASED) == []     # shorter than one window
    assert wt(151, **RELEASED) == [(0, 150)]                       # whole seconds only: 151 frames are 10 s = 150 frames
    assert wt(151, **dict(RELEASED, stride=1)) == [(0, 150)]
    assert wt(166, **dict(RELEASED, stride=1)) == [(i, i + 150) for i in range(16)]
    assert wt(166, **RELEASED) == [(0, 150), (5, 155), (10, 160), (15, 165)]
    assert wt(451, mode="test", **RELEASED) == [(0, 150), (150, 300), (300, 450)]
    assert wt(451, mode="full", **RELEASED) == [(0, 450)]
    assert wt(14, mode="full", **RELEASED) == []                   # no whole second: nothing to cut
    # audio one second shorter than the motion: the usable length is the audio's
    assert wt(166, audio_seconds=10, **dict(RELEASED, stride=1)) == [(0, 150)]
    assert wt(166, audio_seconds=10, mode="full", **RELEASED) == [(0, 150)]
    assert wt(166, audio_seconds=12, **RELEASED) == wt(166, **RELEASED)
    # clean seconds move both ends
    kw = dict(RELEASED, clean_first_seconds=1, clean_final_seconds=2)
    assert wt(451, **kw) == fx.window_table(451, **kw) and wt(451, **kw)[0] == (15, 165) and wt(451, **kw)[-1][1] <= 420
    with pytest.raises(ValueError):
        wt(100, mode="val")


def test_idmapping(ds_mod):
    beat = [1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 15, 16, 17, 18, 20, 21, 22, 23, 24, 25, 27, 28, 30]
    got = [ds_mod.idmapping(i) for i in beat]
    assert got == [fx.idmapping(i) for i in beat]
    assert sorted(got) == list(range(25))
    assert (ds_mod.idmapping(30), ds_mod.idmapping(28), ds_mod.idmapping(27)) == (7, 13, 18)


def test_rawclip_load(ds_mod, tmp_path):
    recs = fx.recordings()
    paths = fx.write_npz(str(tmp_path), recs)
    for p, r, sid in zip(paths, recs, fx.SPEAKER_IDS):
        c = ds_mod.RawClip.load(p)
        assert c.name == r["name"] and c.speaker_id == sid and c.n_raw == r["poses"].shape[0]
        assert np.array_equal(c.poses, r["poses"]) and np.array_equal(c.trans, r["trans"])
        assert np.array_equal(c.expressions, r["expressions"]) and np.array_equal(c.betas, r["betas"])
        assert c.poses.dtype == np.float32
    assert ds_mod.RawClip.load(paths[1], speaker_id=3).speaker_id == 3
    for key in ("poses", "trans", "expressions", "betas"):
        bad = str(tmp_path / ("no_%s.npz" % key))
        np.savez(bad, **{k: recs[3][k] for k in ("poses", "trans", "expressions", "betas") if k != key})
        with pytest.raises(ValueError, match="missing key %s" % key):
            ds_mod.RawClip.load(bad, speaker_id=0)
    noname = str(tmp_path / "wayne.npz")
    np.savez(noname, **{k: recs[3][k] for k in ("poses", "trans", "expressions", "betas")})
    with pytest.raises(ValueError, match="speaker"):
        ds_mod.RawClip.load(noname)
    with pytest.raises(ValueError, match="trans holds"):
        ds_mod.RawClip("x", recs[3]["poses"], recs[3]["trans"][:-1], recs[3]["expressions"], recs[3]["betas"], 0)


def _annotations(rg, seed):
    q = rg.synth.synth_query(seed)
    segs = [[[0.5 * k, 0.5 * k + 0.4], w] for k, w in enumerate("so i went there and it was big".split())]
    labels = [dict(name="iconic", word="big", start=3.5, end=3.9), dict(name="beat", word="so", start=10.2, end=10.9)]
    return dict(discourse=q["discourse"], prominence=q["prominence"] + [("filler", 5.0, 5.2, 1.0)], text_segments=segs,
                gesture_labels=labels)


def _stub_features(name, t0, t1, ann):
    return dict(text_features=[torch.full((3, 4), float(t0))], audio=torch.zeros(1, 5, 4), word=torch.ones(1, 150, 4),
                raw_word=["ignored"])


def test_dataset_windows_names_annotations_and_records(rg, ds_mod):
    ann = [_annotations(rg, 40 + i) for i in range(len(fx.NAMES))]
    ds = ds_mod.SMPLXClipDataset(_clips(ds_mod, ann), _HostPreprocessor(), features=_stub_features, pose_length=150, stride=1)
    want = [(ci, i, s, e) for ci, n in enumerate(fx.RAW_LENS)
            for i, (s, e) in enumerate(fx.window_table(-(-n // fx.STRIDE), pose_length=150, stride=1))]
    assert ds.windows == want and len(ds) == 17
    assert ds.names == ["%s/%d" % (fx.NAMES[ci], i) for ci, i, _, _ in want]
    assert ds.names[0] == "5_stewart_0_5_5/0" and ds.names[1] == "13_lu_0_6_6/0" and ds.names[-1] == "13_lu_0_6_6/15"
    for k, (ci, i, s, e) in enumerate(want):
        t0, t1 = s / 15, e / 15
        cut = rg.longform.window_annotations({key: [v] for key, v in ann[ci].items()}, t0, t1)
        rec, side = ds.retrieval_samples[k], ds._side[k]
        assert rec["sample_name"] == ds.names[k] and rec["speaker_id"] == fx.SPEAKER_IDS[ci]
        for key in ("discourse", "prominence", "gesture_labels"):
            assert rec[key] == cut[key][0] and side[key] == cut[key][0]
        assert side["text_segments"] == cut["text_segments"][0]
        assert side["raw_word"] == " ".join(seg[1] for seg in rg.features.merge_disco_textsegs(cut["text_segments"][0]))
        assert torch.equal(rec["text_feature"], torch.full((3, 4), float(t0)))
        assert side["audio"].shape == (5, 4) and side["word"].shape == (150, 4)
    assert ds._side[0]["raw_word"] == "so i went there and it was big"
    assert ds._side[5]["raw_word"] == "i went there and it was big"          # window 4 of the last clip starts at 4 / 15 s
    # the records are what RetrievalDatabase builds its dicts from, including the stratification filter on "/<i>"
    db = rg.retrieval.build_db_dicts(ds.retrieval_samples)
    assert list(db["idx_2_sense"]) == ds.names and "idx_2_gesture_labels" in db
    strat = rg.retrieval.build_db_dicts(ds.retrieval_samples, stratified_db_creation=True, stratification_interval=15)
    assert list(strat["idx_2_sense"]) == ["5_stewart_0_5_5/0", "13_lu_0_6_6/0", "13_lu_0_6_6/15"]
    # audio a second shorter than the motion: the last clip falls back to one window
    audio = [None] * 5 + [np.zeros(10 * 16000 + 15999, np.float32)]
    short = ds_mod.SMPLXClipDataset(_clips(ds_mod, ann, audio), _HostPreprocessor(), pose_length=150, stride=1)
    assert short.names == ["5_stewart_0_5_5/0", "13_lu_0_6_6/0"]
    assert "text_feature" not in short.retrieval_samples[0]                  # no features: the keys are absent
    with pytest.raises(KeyError):
        rg.retrieval.build_db_dicts(short.retrieval_samples)
    full = ds_mod.SMPLXClipDataset(_clips(ds_mod), _HostPreprocessor(), mode="full")
    assert full.windows == [(3, 0, 0, 30), (4, 0, 0, 150), (5, 0, 0, 165)]


def test_part_columns_are_the_masks(rg, ds_mod):
    cols = ds_mod.part_columns()
    masks = rg.packing.part_masks()
    assert cols.dtype == np.int32 and cols.shape == (159,)
    o = 0
    for part, w in (("upper", 39), ("lower", 27), ("hands", 90), ("face", 3)):
        assert np.array_equal(cols[o:o + w], np.nonzero(masks[part])[0])
        o += w


def test_restatement_matches_recorded_and_meets_the_fixture_conditions():
    """dataset.npz is the restatement's output for the seeded recordings; the restatement alone leaves at most 2 % of the
    contact flags near the threshold, has at least 20 % of the others in each class, and every joint's mean velocity is
    >= 0.05 m/s (the conditions tests/test_dataset_gpu.py relies on)."""
    gold = np.load(os.path.join(HERE, "golden", "dataset.npz"))
    rest = fx.restated()
    assert int(gold["seed"]) == fx.SEED
    for i, n in enumerate(fx.RAW_LENS):
        assert rest["feetv_%d" % i].shape == (-(-n // fx.STRIDE), 4)
        assert np.allclose(rest["feetv_%d" % i], gold["feetv_%d" % i], rtol=0, atol=1e-12)
        assert np.array_equal(rest["contact_%d" % i], gold["contact_%d" % i])
        assert np.all(rest["contact_%d" % i][-1] == 1)
    assert np.allclose(rest["avg_vel"], gold["avg_vel"], rtol=1e-12, atol=0)
    for bound in (JOINT_BOUND, 5e-5):
        near, ones = fx.contact_statistics(rest, bound)
        assert near <= 0.02 and 0.2 <= ones <= 0.8, (bound, near, ones)
    assert rest["avg_vel"].min() >= 0.05
    assert max(np.abs(r["trans"]).max() for r in fx.recordings()) <= 1.0


def test_model_loader_gives_expression_joint_directions(rg):
    m = fx.smplx_model()
    small = {k: v for k, v in m.items() if k not in ("f", "weights", "posedirs")}      # faces, skinning and posedirs are not needed
    a = rg.evaluation.load_smplx_model(small)
    want = np.einsum("jv,vdk->jdk", m["J_regressor"].astype(np.float64), m["shapedirs"][..., 300:400].astype(np.float64))
    assert a["J_expr"].shape == (55, 3, 100) and np.allclose(a["J_expr"], want, rtol=0, atol=1e-15)
    assert "J_expr" not in rg.evaluation.load_smplx_model(dict(small, shapedirs=m["shapedirs"][..., :300]))


def test_library_exports_the_new_entry_points(rg):
    capi = rg.capi
    lib = capi.load_library()
    protos = capi.header_prototypes()
    for s in ("rg_smplx_joints_expr", "rg_clip_prepare", "rg_joint_speed_sums"):
        assert s in capi.header_symbols() and hasattr(lib, s), s
        assert protos[s] == (ctypes.c_int, [ctypes.c_void_p] * 3)
    assert lib.rg_version() == capi.header_version() >= 118


def test_argument_blocks_match_the_header(rg):
    """Field by field, the ctypes structures against the C declarations of include/rg_gesture.h."""
    import re
    with open(rg.capi.HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "int64_t": ctypes.c_int64}
    for name, cls in (("rg_smplx_joints_expr_args", rg.evaluation.SmplxJointsExprArgs),
                      ("rg_clip_prepare_args", rg.dataset.ClipPrepareArgs), ("rg_joint_speed_args", rg.dataset.JointSpeedArgs)):
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S).group(1)
        want = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if decl:
                ty, field = decl.rsplit(" ", 1)
                want.append((field, ctypes.c_void_p if "*" in ty else ctype[ty.replace("const ", "")]))
        assert [(n, t) for n, t in cls._fields_] == want, name
