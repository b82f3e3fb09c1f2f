"""Seeded inputs of tests/golden/face_metrics.npz: a small synthetic SMPL-X model with the full key set the mesh needs
(v_template, shapedirs with 300 shape + 100 expression components, posedirs [V, 3, 486], sparse skinning weights, J_regressor,
kintree_table, hand means) and clips with smooth expressions and jaw angles that cross pi.  Used by
make_face_metrics_golden.py (with the reference) and by tests/test_face_metrics_*.py (without it).  full_model() is the same
construction at the real file's size."""
import os

import numpy as np

SMPLX_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
                 20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38,
                 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53]
N_VERTS = 300
N_SHAPE = 400
EVAL_N = 64
N_FRAMES = 70                    # saved clip length; the evaluation keeps the first EVAL_N (the reference needs n == eval_n)
N_CLIPS = 4
MODEL_SEED = 91
SEED = 1234                      # the clips of face_metrics.npz
POSE_FPS = 30
AUDIO_SR = 16000


def smplx_model(seed=MODEL_SEED, n_verts=N_VERTS, scale=1.0):
    """{key: array} of a SMPLX_NEUTRAL_2020.npz: the real kintree_table (root stored as 2**32-1), a unit-scale v_template,
    J_regressor rows that are convex mixes of 4 vertices, shapedirs / posedirs of small random directions, and per vertex 1-6
    random joints with positive weights summing to 1 (float32, as in the real file)."""
    rng = np.random.default_rng(seed)
    jr = np.zeros((55, n_verts))
    for j in range(55):
        idx = rng.choice(n_verts, 4, replace=False)
        w = rng.random(4) + 0.2
        jr[j, idx] = w / w.sum()
    w = np.zeros((n_verts, 55), np.float32)
    k = rng.integers(1, 7, n_verts)
    for v in range(n_verts):
        j = rng.choice(55, k[v], replace=False)
        x = (rng.random(k[v]) + 0.1).astype(np.float32)
        w[v, j] = x / x.sum()
    kt = np.array([SMPLX_PARENTS, list(range(55))], dtype=np.int64)
    kt[0, 0] = 2 ** 32 - 1
    return dict(kintree_table=kt, J_regressor=jr.astype(np.float32),
                v_template=(rng.uniform(-1, 1, (n_verts, 3)) * scale).astype(np.float32),
                shapedirs=(rng.standard_normal((n_verts, 3, N_SHAPE)) * 3e-3 * scale).astype(np.float32),
                posedirs=(rng.standard_normal((n_verts, 3, 486)) * 3e-3 * scale).astype(np.float32),
                weights=w, hands_meanl=rng.uniform(-0.3, 0.3, 45).astype(np.float32),
                hands_meanr=rng.uniform(-0.3, 0.3, 45).astype(np.float32), f=np.zeros((1, 3), np.int64))


def full_model(seed=7):
    """The same construction at the size of SMPLX_NEUTRAL_2020.npz: 10 475 vertices."""
    return smplx_model(seed, n_verts=10475)


def smooth(rng, n, k, amp):
    """[n, k] float32: per channel an offset and a sum of 3 sinusoids (periods 0.5-3 s)."""
    t = np.arange(n)[:, None] / POSE_FPS
    out = rng.uniform(-amp, amp, (1, k))
    for _ in range(3):
        f = rng.uniform(1 / 3.0, 2.0, (1, k))
        ph = rng.uniform(0, 2 * np.pi, (1, k))
        out = out + amp / 2 * rng.uniform(0.3, 1.0, (1, k)) * np.sin(2 * np.pi * f * t + ph)
    return out.astype(np.float32)


def clip_poses(rng, n):
    """[n, 165]: smooth small body / hand angles, and a jaw whose angle sweeps through pi (3.0 .. 3.3) in part of the clip."""
    p = smooth(rng, n, 165, 0.4)
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    ang = 3.15 + 0.25 * np.sin(2 * np.pi * rng.uniform(0.3, 1.0) * np.arange(n) / POSE_FPS + rng.uniform(0, 2 * np.pi))
    ang[: n // 3] = 0.3 + 0.1 * np.arange(n // 3) / n                     # a stretch of ordinary angles
    p[:, 66:69] = (axis[None] * ang[:, None]).astype(np.float32)
    return p


def inputs(seed=SEED, n_clips=N_CLIPS, n=N_FRAMES):
    rng = np.random.default_rng(seed)
    pred = [clip_poses(rng, n) for _ in range(n_clips)]
    gt = [clip_poses(rng, n) for _ in range(n_clips)]
    pred_e = [smooth(rng, n, 100, 1.0) for _ in range(n_clips)]
    gt_e = [smooth(rng, n, 100, 1.0) for _ in range(n_clips)]
    betas = [rng.standard_normal(300) * (0.0 if i == 1 else 1.0) for i in range(n_clips)]
    trans = [smooth(rng, n, 3, 0.5) for _ in range(2 * n_clips)]
    return dict(pred=pred, gt=gt, pred_exprs=pred_e, gt_exprs=gt_e, betas=betas, trans=trans)


def clip_names(n_clips=N_CLIPS):
    return ["test/%d_face_0_%d_%d" % (i, i, i) for i in range(n_clips)]


def write_folder(root, inp, save_sample_files):
    """root/test/<clip>/{pred,gt}_motion.npz (save_sample_files layout) with the fixture's expressions and translations; the
    ground truth's betas overwritten with the fixture's."""
    names = clip_names(len(inp["pred"]))
    C = len(names)
    save_sample_files(root, names, (np.stack(inp["pred"]), np.stack(inp["pred_exprs"]), np.stack(inp["trans"][:C])),
                      (np.stack(inp["gt"]), np.stack(inp["gt_exprs"]), np.stack(inp["trans"][C:])))
    for i, name in enumerate(names):
        gfile = os.path.join(root, name, "gt_motion.npz")
        with np.load(gfile) as f:
            fields = {k: f[k] for k in f.files}
        fields["betas"] = inp["betas"][i]
        np.savez(gfile, **fields)
    return names


def restated_scores(model, inp, eval_n=EVAL_N):
    """(l2, lvel) of the folder in float64 by smplx_lbs.py, the reference's formulas."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("smplx_lbs", os.path.join(os.path.dirname(os.path.abspath(__file__)), "smplx_lbs.py"))
    lbs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lbs)
    m = lbs.load_model(model)
    l2 = lvel = 0.0
    total = 0
    for i in range(len(inp["pred"])):
        n = min(inp["pred"][i].shape[0], eval_n)
        rec = lbs.face_vertices(m, inp["pred"][i][:n], inp["pred_exprs"][i][:n], inp["betas"][i])
        tar = lbs.face_vertices(m, inp["gt"][i][:n], inp["gt_exprs"][i][:n], inp["betas"][i])
        a, b = lbs.face_scores(rec, tar)
        l2, lvel, total = l2 + a, lvel + b, total + n
    return l2 / total, lvel / total
