"""GPU: SMPL-X mesh vertices (rg_mesh_transforms + rg_mesh_blend_skin) against the float64 restatement tests/golden/smplx_lbs.py
on a full-size synthetic model, and the face metrics (rg_mesh_face_sums) against the reference's printed l2 / lvel
(tests/golden/face_metrics.npz, made by make_face_metrics_golden.py), on ragged batches, for batch invariance and errors."""
import importlib
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "face_metrics.npz")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ff, lbs, fgdfx = _load("face_fixture"), _load("smplx_lbs"), _load("fgd_fixture")


@pytest.fixture(scope="module")
def ev():
    return importlib.import_module("rag-gesture_amd").evaluation


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def full():
    return ff.full_model()


@pytest.fixture(scope="module")
def full_mesh(ev, full):
    return ev.SMPLXMesh(full)


def _random_poses(rng, n):
    aa = rng.uniform(-0.6, 0.6, (n, 165))
    dirs = rng.standard_normal((n, 55, 3))
    dirs /= np.linalg.norm(dirs, axis=2, keepdims=True)
    ang = rng.choice([1e-4, np.pi - 1e-3, np.pi + 0.3, 5.0], (n, 55, 1))
    pick = rng.random((n, 55, 1)) < 0.3
    return np.where(pick, dirs * ang, aa.reshape(n, 55, 3)).reshape(n, 165).astype(np.float32)


def test_full_size_vertices_match_float64(ev, full, full_mesh):
    rng = np.random.default_rng(3)
    m = lbs.load_model(full)
    clips = [_random_poses(rng, 9), _random_poses(rng, 7)]
    betas = [rng.standard_normal(300), rng.standard_normal(300) * 0.5]
    exprs = [rng.standard_normal((9, 100)).astype(np.float32), rng.standard_normal((7, 100)).astype(np.float32)]
    transl = [rng.uniform(-1, 1, (9, 3)).astype(np.float32), rng.uniform(-1, 1, (7, 3)).astype(np.float32)]
    got = full_mesh.vertices(clips, betas, exprs, transl).cpu().numpy()
    want = np.concatenate([lbs.lbs(m, c, b, e, t)[0] for c, b, e, t in zip(clips, betas, exprs, transl)])
    assert got.shape == (16, 10475, 3)
    assert np.abs(got - want).max() <= 2e-5
    folded = full_mesh.vertices(clips, betas, exprs, transl, fold=True).cpu().numpy()     # (fold first, then the hand means)
    want = np.concatenate([lbs.lbs(m, lbs.fold(c), b, e, t)[0] for c, b, e, t in zip(clips, betas, exprs, transl)])
    assert np.abs(folded - want).max() <= 2e-5


def test_transforms_joints_match_smplx_joints(ev, full, full_mesh):
    rng = np.random.default_rng(4)
    clips = [_random_poses(rng, 10), _random_poses(rng, 6)]
    betas = [rng.standard_normal(300), np.zeros(300)]
    j = torch.empty(16, 55, 3, device=full_mesh.device, dtype=torch.float32)
    full_mesh.vertices(clips, betas, joints=j)
    want = ev.SMPLXJoints(full).joints(clips, betas).cpu().numpy()
    assert np.abs(j.cpu().numpy() - want).max() <= 1e-5


@pytest.fixture(scope="module")
def folder(tmp_path_factory, gold):
    packing = importlib.import_module("rag-gesture_amd").packing
    root = tmp_path_factory.mktemp("face")
    ff.write_folder(str(root / "eval"), ff.inputs(int(gold["seed"])), packing.save_sample_files)
    return root


def test_evaluate_folder_end_to_end(ev, gold, folder):
    enc = ev.FGDEncoder(fgdfx.state_dict(np.load(os.path.join(HERE, "golden", "fgd_eval.npz"))))
    t = {}
    r = ev.evaluate_folder(str(folder / "eval"), enc, eval_n=ff.EVAL_N, mesh=ev.SMPLXMesh(ff.smplx_model()), timings=t)
    for k in ("l2", "lvel"):
        assert r[k] == pytest.approx(float(gold["score_" + k]), rel=1e-4), k
        assert r[k] == pytest.approx(float(gold["f64_" + k]), rel=1e-4), k
    plain = ev.evaluate_folder(str(folder / "eval"), enc, eval_n=ff.EVAL_N)
    assert set(plain) == {"fgd", "clips", "latents", "frames"} and plain["fgd"] == r["fgd"]
    one = ev.evaluate_folder(str(folder / "eval"), enc, eval_n=ff.EVAL_N, mesh=ev.SMPLXMesh(ff.smplx_model()), batch_clips=1)
    assert one["l2"] == r["l2"] and one["lvel"] == r["lvel"]


def _ragged(seed, lens):
    rng = np.random.default_rng(seed)
    inp = ff.inputs(seed, n_clips=len(lens), n=max(lens))
    pred = [p[:n] for p, n in zip(inp["pred"], lens)]
    gt = [g[:n] for g, n in zip(inp["gt"], lens)]
    pe = [e[:n] for e, n in zip(inp["pred_exprs"], lens)]
    ge = [e[:n] for e, n in zip(inp["gt_exprs"], lens)]
    betas = [b * rng.uniform(0.5, 1.5) for b in inp["betas"]]
    return pred, gt, pe, ge, betas


LENS = [2, 300, 37, 3, 129, 65, 300, 5, 211, 64, 2, 99, 150, 17, 33, 250, 71, 8, 190, 127, 3, 44, 277, 61]


def test_ragged_full_size_matches_float64(ev, full, full_mesh):
    pred, gt, pe, ge, betas = _ragged(11, LENS)
    fm = ev.FaceMetrics(full_mesh, eval_n=300)
    fm.add(pred, gt, pe, ge, betas)
    got = fm.compute()
    m = lbs.load_model(full)
    l2 = lvel = 0.0
    for i, n in enumerate(LENS):
        rec = lbs.face_vertices(m, pred[i], pe[i], betas[i])
        tar = lbs.face_vertices(m, gt[i], ge[i], betas[i])
        a, b = lbs.face_scores(rec, tar)
        l2, lvel = l2 + a, lvel + b
    assert got["l2"] == pytest.approx(l2 / sum(LENS), rel=1e-4)
    assert got["lvel"] == pytest.approx(lvel / sum(LENS), rel=1e-4)
    assert isinstance(got["l2"], float) and isinstance(got["lvel"], float)


def test_batch_invariance(ev, full_mesh):
    lens = LENS[:10]
    pred, gt, pe, ge, betas = _ragged(12, lens)
    fm = ev.FaceMetrics(full_mesh, eval_n=300)
    batch = fm.add(pred, gt, pe, ge, betas)
    for i in (0, 4, 9):
        alone = ev.FaceMetrics(full_mesh, eval_n=300).add([pred[i]], [gt[i]], [pe[i]], [ge[i]], [betas[i]])
        assert np.array_equal(alone[0], batch[i]), i
    sub = ev.FaceMetrics(full_mesh, eval_n=300).add(pred[3:7], gt[3:7], pe[3:7], ge[3:7], betas[3:7])
    assert np.array_equal(sub, batch[3:7])


def test_errors_name_the_clip(ev, full_mesh, folder, tmp_path):
    pred, gt, pe, ge, betas = _ragged(13, [5, 1, 4])
    fm = ev.FaceMetrics(full_mesh)
    with pytest.raises(ValueError, match="clip 1"):
        fm.add(pred, gt, pe, ge, betas)
    pred, gt, pe, ge, betas = _ragged(14, [6, 6])
    with pytest.raises(ValueError, match="clip 1"):
        fm.add(pred, gt, [pe[0], pe[1][:4]], ge, betas)
    assert fm.clips == 0
    # a folder whose prediction holds fewer expression rows than poses
    import shutil
    root = tmp_path / "short"
    shutil.copytree(str(folder / "eval"), str(root))
    name = ff.clip_names()[2]
    f = root / name / "pred_motion.npz"
    with np.load(str(f)) as z:
        fields = {k: z[k] for k in z.files}
    fields["expressions"] = fields["expressions"][:10]
    np.savez(str(f), **fields)
    enc = ev.FGDEncoder(fgdfx.state_dict(np.load(os.path.join(HERE, "golden", "fgd_eval.npz"))))
    with pytest.raises(ValueError, match=name):
        ev.evaluate_folder(str(root), enc, eval_n=ff.EVAL_N, mesh=ev.SMPLXMesh(ff.smplx_model()))
