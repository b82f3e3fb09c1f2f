"""Result bits of everything that runs the SMPL-X forward kinematics (NOTEBOOK.md section 24): from seeded inputs and the synthetic
models of tests/golden/*_fixture.py, one .npy per result under OUT.  Uses only names two trees of this project share
(rg.evaluation.*, rg.mesh.*, rg.dataset.*), so the dumps of two commits can be compared file by file with `cmp`.

    python profiles/smplx_fk_dump.py OUT [--root TREE]        # TREE: the checkout whose package is imported (default: this one)
"""
import argparse
import importlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def fixture(root, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def random_poses(rng, n):
    """Angles near 0, near pi and beyond pi among ordinary ones (tests/test_face_metrics_gpu.py)."""
    aa = rng.uniform(-0.6, 0.6, (n, 165))
    dirs = rng.standard_normal((n, 55, 3))
    dirs /= np.linalg.norm(dirs, axis=2, keepdims=True)
    ang = rng.choice([1e-4, np.pi - 1e-3, np.pi + 0.3, 5.0], (n, 55, 1))
    pick = rng.random((n, 55, 1)) < 0.3
    return np.where(pick, dirs * ang, aa.reshape(n, 55, 3)).reshape(n, 165).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--root", default=os.path.dirname(HERE))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    rg = importlib.import_module("rag-gesture_amd")
    assert os.path.dirname(os.path.dirname(os.path.abspath(rg.__file__))) == root, rg.__file__
    ev, ff, dfx = rg.evaluation, fixture(root, "face_fixture"), fixture(root, "dataset_fixture")
    os.makedirs(args.out, exist_ok=True)

    def save(name, x):
        x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
        np.save(os.path.join(args.out, name + ".npy"), np.ascontiguousarray(x))

    rng = np.random.default_rng(2027)
    model = ff.smplx_model()
    sm, mesh = ev.SMPLXJoints(model), rg.mesh.SMPLXMesh(model)
    lens = [1, 6, 2, 37, 64, 5]
    clips = [random_poses(rng, n) for n in lens]
    betas = [rng.standard_normal(300) for _ in lens]
    exprs = [rng.standard_normal((n, 100)).astype(np.float32) for n in lens]
    transl = [rng.uniform(-1, 1, (n, 3)).astype(np.float32) for n in lens]
    save("joints_plain", sm.joints(clips))
    save("joints_fold", sm.joints(clips, fold=True))
    save("joints_betas", sm.joints(clips, betas))
    save("joints_betas_fold", sm.joints(clips, betas, fold=True))
    save("joints_root_norm", sm.joints(clips, betas, root_norm=True))
    save("joints_expr_transl", sm.joints(clips, betas, expressions=exprs, transl=transl))
    save("joints_expr_transl_fold", sm.joints(clips, betas, fold=True, expressions=exprs, transl=transl))
    save("joints_transl_only", sm.joints(clips, None, transl=transl))
    dev = sm.device
    cat = lambda xs: torch.from_numpy(np.concatenate(xs)).to(dev)
    raw_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    clip_off = np.concatenate([[0], np.cumsum([-(-n // 2) for n in lens])]).astype(np.int32)
    save("joints_strided_2", sm.joints_strided(cat(clips), cat(exprs), cat(transl), raw_off, clip_off, 2, betas=betas))

    for fold in (False, True):
        j = torch.empty(sum(lens), 55, 3, device=dev, dtype=torch.float32)
        save("vertices_fold%d" % fold, mesh.vertices(clips, betas, exprs, transl, fold=fold, joints=j))
        save("vertices_joints_fold%d" % fold, j)
    j = torch.empty(sum(lens), 55, 3, device=dev, dtype=torch.float32)
    save("vertices_bare", mesh.vertices(clips, joints=j))
    save("vertices_bare_joints", j)

    big = [n for n in lens if n >= 2]
    pred, gt = [random_poses(rng, n) for n in big], [random_poses(rng, n) for n in big]
    fm = rg.mesh.FaceMetrics(mesh)
    save("face_sums", fm.add(pred, gt, [rng.standard_normal((n, 100)).astype(np.float32) for n in big],
                             [rng.standard_normal((n, 100)).astype(np.float32) for n in big], betas=betas[:len(big)]))
    save("face_metrics", np.array([fm.compute()[k] for k in ("l2", "lvel")], np.float64))

    n, C = 40, 5
    jm = ev.JointMetrics(sm, avg_vel=rng.uniform(0.05, 0.5, 55))
    jm.add([random_poses(rng, n) for _ in range(C)], [random_poses(rng, n) for _ in range(C)],
           betas=[rng.standard_normal(300) for _ in range(C)], onsets=[np.sort(rng.uniform(0, 0.6, 4)) for _ in range(C)],
           retrieval=[random_poses(rng, n) if i % 2 else None for i in range(C)],
           sem_scores=[rng.uniform(0, 1, n // 2 + 1).astype(np.float32) for _ in range(C)])
    res = jm.compute()
    save("joint_metrics", np.array([res[k] for k in sorted(res)], np.float64))
    save("joint_metrics_pred_joints", torch.cat(jm.pred_joints))

    recs = dfx.recordings()
    raw = [rg.dataset.RawClip(r["name"], r["poses"], r["trans"], r["expressions"], r["betas"], sid)
           for r, sid in zip(recs, dfx.SPEAKER_IDS)]
    dmodel = {k: v for k, v in dfx.smplx_model().items() if k not in ("f", "weights", "posedirs")}
    pre = rg.dataset.ClipPreprocessor(dmodel, pose_fps=dfx.POSE_FPS)
    for i, p in enumerate(pre.prepare(raw)):
        for k in sorted(p):
            if torch.is_tensor(p[k]):
                save("dataset_clip%d_%s" % (i, k), p[k])
    save("dataset_mean_velocity", pre.mean_velocity([c for c in raw if c.n_raw >= 2]))
    torch.cuda.synchronize()
    print("wrote %d files to %s" % (len(os.listdir(args.out)), args.out))


if __name__ == "__main__":
    main()
