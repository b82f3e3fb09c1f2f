"""GPU: raw SMPL-X recordings -> model inputs on the device (rg_smplx_joints_expr, rg_clip_prepare, rg_joint_speed_sums)
against the float64 restatement of mogen/datasets/beatx_dataset.py in tests/golden/dataset_fixture.py, and SMPLXClipDataset as
the `database=` of build_architecture."""
import importlib
import importlib.util
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fx = _load("dataset_fixture")
JOINT_BOUND = 1e-5                                   # max abs error of a joint coordinate (m), |trans| <= 1 m
CONTACT_MARGIN = 2 * np.sqrt(3.0) * JOINT_BOUND      # two joints, each off by at most the bound per coordinate
VEL_BOUND = 2 * np.sqrt(3.0) * JOINT_BOUND * 30      # the forward difference of two such joints over dt = 1 / 30
GI = [0] * 25 + list(range(25))


@pytest.fixture(scope="module")
def recs():
    return fx.recordings()


@pytest.fixture(scope="module")
def ref(recs):
    """The restatement, computed once: 30 fps joints of every recording, the kept frames' feetv / contact, avg_vel."""
    m = fx.lbs.load_model(fx.smplx_model())
    j30 = [fx.joints(m, r) for r in recs]
    cont = [fx.contacts(fx.strided(j)) for j in j30]
    return dict(j30=j30, feetv=[c[0] for c in cont], contact=[c[1] for c in cont],
                avg_vel=fx.mean_velocity([j for j in j30 if j.shape[0] >= 2]))


@pytest.fixture(scope="module")
def raw_clips(rg, recs):
    return [rg.dataset.RawClip(r["name"], r["poses"], r["trans"], r["expressions"], r["betas"], sid)
            for r, sid in zip(recs, fx.SPEAKER_IDS)]


@pytest.fixture(scope="module")
def pre(rg):
    model = {k: v for k, v in fx.smplx_model().items() if k not in ("f", "weights", "posedirs")}   # not needed on this path
    return rg.dataset.ClipPreprocessor(model, pose_fps=fx.POSE_FPS)


@pytest.fixture(scope="module")
def prepared(pre, raw_clips):
    return pre.prepare(raw_clips)


def test_joints_with_expression_and_translation(rg, parity, pre, recs, ref, prepared):
    """All 55 joints of every fixture frame at 30 fps (SMPLXJoints.joints(expressions=, transl=)) and of the kept frames
    (prepare's strided launch) against smplx_lbs.lbs(...)[1] + transl."""
    got = pre.smplx.joints([r["poses"] for r in recs], betas=[r["betas"] for r in recs],
                           expressions=[r["expressions"] for r in recs], transl=[r["trans"] for r in recs]).cpu().numpy()
    want = np.concatenate(ref["j30"])
    assert got.shape == want.shape == (sum(fx.RAW_LENS), 55, 3)
    err = np.abs(got - want).max()
    print("joints with expression and translation, 30 fps: max abs error %.3e m" % err)
    parity.check("dataset: joints with expression + transl vs float64 (m)", err, JOINT_BOUND)
    kept = np.concatenate([p["joints"].cpu().numpy() for p in prepared])
    err = np.abs(kept - np.concatenate([fx.strided(j) for j in ref["j30"]])).max()
    print("joints of the kept frames: max abs error %.3e m" % err)
    parity.check("dataset: joints of the kept frames vs float64 (m)", err, JOINT_BOUND)


def test_parts_and_strided_rows_are_bit_exact(rg, recs, prepared):
    masks = rg.packing.part_masks()
    for r, p in zip(recs, prepared):
        n = -(-r["poses"].shape[0] // fx.STRIDE)
        host = {k: v.cpu().numpy() for k, v in p.items() if torch.is_tensor(v)}
        assert host["motion"].shape == (n, 165) and host["motion"].dtype == np.float32
        assert np.array_equal(host["motion"], r["poses"][::2])
        assert np.array_equal(host["trans"], r["trans"][::2]) and host["trans"].shape == (n, 3)
        assert np.array_equal(host["facial"], r["expressions"][::2]) and host["facial"].shape == (n, 100)
        for part, w in (("upper", 39), ("lower", 27), ("hands", 90), ("face", 3)):
            assert host["motion_" + part].shape == (n, w)
            assert np.array_equal(host["motion_" + part], r["poses"][::2][:, masks[part]]), part
        want = fx.part_gathers(r["poses"][::2], masks)
        assert all(np.array_equal(host["motion_" + k], want[k]) for k in want)
        assert np.array_equal(host["beta"], np.repeat(r["betas"].astype(np.float32)[None], n, 0))
        assert host["speaker_id"].dtype == np.int64 and host["speaker_id"].shape == (n,)
    # the gathers invert rg_scatter_joints
    p = prepared[4]
    back = rg.packing.scatter_parts(*(p["motion_" + k][None].contiguous() for k in ("upper", "lower", "hands", "face")))[0]
    keep = np.zeros(165, bool)
    for m in masks.values():
        keep |= m
    assert torch.equal(back[:, torch.from_numpy(keep).to(back.device)], p["motion"][:, torch.from_numpy(keep).to(back.device)])


def test_contacts(rg, pre, raw_clips, ref, prepared):
    got = [p["contact"].cpu().numpy() for p in prepared]
    for g, n in zip(got, fx.RAW_LENS):
        assert g.shape == (-(-n // fx.STRIDE), 4) and set(np.unique(g)) <= {0.0, 1.0}
        assert np.all(g[-1] == 1.0)                                  # a clip's last kept frame
    assert np.all(got[0] == 1.0) and np.all(got[1] == 1.0)           # the one-frame clips (1 and 2 raw frames)
    flags, want, feetv = (np.concatenate(x).ravel() for x in (got, ref["contact"], ref["feetv"]))
    near = np.abs(feetv - fx.CONTACT_THRESHOLD) <= CONTACT_MARGIN
    print("contact flags: %d, left out near the threshold: %d, ones among the rest: %.3f, mismatches: %d"
          % (flags.size, near.sum(), want[~near].mean(), (flags[~near] != want[~near]).sum()))
    assert np.array_equal(flags[~near], want[~near])
    assert near.mean() <= 0.02
    assert 0.2 <= want[~near].mean() <= 0.8
    # no difference crosses a clip boundary: every clip alone gives the bits it gives inside the batch
    for c, p in zip(raw_clips, prepared):
        alone = pre.prepare([c])[0]
        for k in ("contact", "joints", "motion", "motion_lower"):
            assert torch.equal(alone[k], p[k]), (c.name, k)


def test_mean_velocity_and_cli(rg, parity, pre, raw_clips, recs, ref, tmp_path):
    long_enough = [c for c in raw_clips if c.n_raw >= 2]
    got = pre.mean_velocity(long_enough)
    assert got.dtype == np.float64 and got.shape == (55,)
    assert ref["avg_vel"].min() >= 0.05
    err = np.abs(got - ref["avg_vel"]).max()
    print("mean velocity: max abs error %.3e m/s (bound %.3e), min avg_vel %.3f" % (err, VEL_BOUND, ref["avg_vel"].min()))
    parity.check("dataset: mean joint velocity vs float64 (m/s)", err, VEL_BOUND)
    # a clip's sums do not depend on its neighbours
    sums = pre.speed_sums(long_enough)
    assert np.array_equal(sums[2], pre.speed_sums(long_enough[2:3])[0])
    with pytest.raises(ValueError, match=fx.NAMES[0]):
        pre.mean_velocity(raw_clips)                                 # the one-frame recording, by name
    folder = tmp_path / "smplxflame_30"
    folder.mkdir()
    fx.write_npz(str(folder), recs[1:])
    model_path, out = str(tmp_path / "SMPLX_NEUTRAL_2020.npz"), str(tmp_path / "mean_vel_smplxflame_30.npy")
    np.savez(model_path, **fx.smplx_model())
    assert rg.dataset.main(["mean-vel", str(folder), "--smplx_path", model_path, "-o", out]) == 0
    assert np.allclose(np.load(out), got, rtol=1e-13, atol=0)        # (the folder's file order: another order of the fp64 sum)
    jm = rg.evaluation.JointMetrics(pre.smplx, avg_vel=out)
    assert jm is not None


def _annotations(rg, seed):
    q = rg.synth.synth_query(seed)
    return dict(discourse=q["discourse"], prominence=q["prominence"] + [("filler", 5.0, 5.2, 1.0)],
                text_segments=[[[0.5 * k, 0.5 * k + 0.4], w] for k, w in enumerate("so i went there and it was big".split())])


def _stub_features(name, t0, t1, ann):
    """Deterministic stand-in for wav2vec2 / BERT on the window, in LongformSynthesizer's batch-of-one layout."""
    g = torch.Generator().manual_seed(zlib.crc32(("%s|%.6f" % (name, t0)).encode()) & 0x7FFFFFFF)
    L = 12 + int(torch.randint(0, 20, (1,), generator=g))
    return dict(audio=torch.randn(1, 499, 768, generator=g), word=torch.randn(1, 150, 768, generator=g),
                text_features=[torch.randn(L, 768, generator=g)])


class _DictDataset:
    """A plain dict-backed dataset, assembled by hand."""

    def __init__(self, samples, records):
        self.samples, self.retrieval_samples = samples, records
        self.names = [s["sample_name"] for s in samples]

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, key):
        return self.samples[self.names.index(key) if isinstance(key, str) else key]


def test_dataset_is_a_drop_in_database(rg, pre, recs, tmp_path):
    paths = fx.write_npz(str(tmp_path), recs)
    clips = [rg.dataset.RawClip.load(p, annotations=_annotations(rg, 60 + i)) for i, p in enumerate(paths)]
    ds = rg.dataset.SMPLXClipDataset(clips, pre, features=_stub_features, pose_length=150, stride=1)
    assert len(ds) == 17 and ds.names[:3] == [fx.NAMES[4] + "/0", fx.NAMES[5] + "/0", fx.NAMES[5] + "/1"]
    # two windows of one clip overlap by 149 frames: views of one buffer (the clip was prepared once)
    a, b = ds[1], ds[fx.NAMES[5] + "/1"]
    for k in ds.TENSOR_KEYS:
        assert a[k].shape[0] == b[k].shape[0] == 150
        assert a[k].untyped_storage().data_ptr() == b[k].untyped_storage().data_ptr(), k
        assert b[k].data_ptr() - a[k].data_ptr() == a[k].shape[1] * 4 and torch.equal(a[k][1:], b[k][:-1])
    assert a["contact"].shape == (150, 4) and a["motion"].shape == (150, 165) and a["motion_length"] == 150
    assert torch.equal(a["motion_mask"], torch.ones(150, device=a["motion"].device))
    assert a["beta"].shape == (150, 300) and a["speaker_id"].dtype == torch.int64 and a["speaker_id"].shape == (150,)
    assert int(a["speaker_id"][0]) == fx.SPEAKER_IDS[5] and a["sample_name"] == fx.NAMES[5] + "/0" and a["sample_idx"] == 1
    batch = ds.collate([0, 1])
    assert batch["motion"].shape == (2, 150, 165) and batch["speaker_ids"].shape == (2, 150)
    assert batch["sample_name"] == ds.names[:2] and batch["sample_idx"] == [0, 1] and batch["motion_length"] == [150, 150]
    assert len(batch["text_features"]) == 2 and batch["audio"].shape == (2, 499, 768) and batch["word"].shape == (2, 150, 768)
    assert isinstance(batch["raw_word"][0], str) and len(batch["discourse"]) == 2

    # the same samples by hand: the restatement's arrays (NumPy slicing of the raw recordings) + the device's contacts
    dev = pre.device
    masks = rg.packing.part_masks()
    contact = [p["contact"] for p in ds.prepared()]
    samples = []
    for k, (ci, i, s, e) in enumerate(ds.windows):
        r = recs[ci]
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        pose = fx.strided(r["poses"])[s:e]
        smp = dict(motion=up(pose), trans=up(fx.strided(r["trans"])[s:e]), facial=up(fx.strided(r["expressions"])[s:e]),
                   contact=contact[ci][s:e].clone(), motion_mask=torch.ones(e - s, device=dev), motion_length=e - s,
                   beta=up(np.repeat(r["betas"].astype(np.float32)[None], e - s, 0)),
                   speaker_id=torch.full((e - s,), fx.SPEAKER_IDS[ci], dtype=torch.int64, device=dev),
                   sample_name="%s/%d" % (r["name"], i), sample_idx=k)
        smp.update({"motion_" + part: up(v) for part, v in fx.part_gathers(pose, masks).items()})
        ann = rg.longform.window_annotations({key: [v] for key, v in _annotations(rg, 60 + ci).items()}, s / 15, e / 15)
        smp.update({key: v[0] for key, v in ann.items()})
        smp["raw_word"] = " ".join(seg[1] for seg in rg.features.merge_disco_textsegs(smp["text_segments"]))
        f = _stub_features(r["name"], s / 15, e / 15, ann)
        smp.update(audio=f["audio"][0], word=f["word"][0], text_feature=f["text_features"][0])
        samples.append(smp)
    records = [dict(sample_name=s["sample_name"], speaker_id=int(s["speaker_id"][0]), discourse=s["discourse"],
                    prominence=s["prominence"], gesture_labels=s["gesture_labels"], text_feature=s["text_feature"]) for s in samples]
    hand = _DictDataset(samples, records)

    def hand_collate(idx):
        b = [hand[i] for i in idx]
        out = {k: torch.stack([x[k] for x in b]) for k in ds.TENSOR_KEYS + ("motion_mask", "beta", "audio", "word")}
        out["speaker_ids"] = torch.stack([x["speaker_id"] for x in b])
        out["text_features"] = [x["text_feature"] for x in b]
        out.update({k: [x[k] for x in b] for k in ds.LIST_KEYS})
        return out

    cfg = rg.synth.default_model_cfg(num_layers=2)
    vae_cfgs = rg.synth.synth_vae_cfgs(decoder_arch="all_encoder", num_layers=2)
    P = rg.synth.synth_full_state(0, cfg, vae_cfgs)
    ikw = dict(use_inversion=True, insertion_guidance=True, guidance_iters=GI, guidance_lr=0.1)
    outs = []
    for database, collate in ((ds, ds.collate), (hand, hand_collate)):
        model = rg.build_architecture(rg.synth.reference_style_model_cfg(cfg, vae_cfgs, with_retrieval=True), database=database)
        model.load_state_dict(P)
        out = model(**collate([0, 1]), retrieval_method="discourse", inference_kwargs=dict(ikw, noise_tape=rg.synth.NoiseTape(5)))
        torch.cuda.synchronize()
        outs.append(out)
    rd = outs[0]["retrieval_dict"]
    assert sum(len(x) for x in rd["retr_startends"]) >= 1, "the windows should retrieve exemplars from their neighbours"
    assert outs[0]["retrieval_dict"]["raw_sample_names"] == outs[1]["retrieval_dict"]["raw_sample_names"]
    for k in ("pred_upper", "pred_lower", "pred_hands", "pred_facepose", "pred_exps", "pred_transl", "prev_latentout"):
        assert torch.isfinite(outs[0][k]).all(), k
        assert torch.equal(outs[0][k], outs[1][k]), k
