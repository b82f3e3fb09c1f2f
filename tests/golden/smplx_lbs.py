"""A float64 NumPy restatement of smplx.lbs.lbs as smplx.SMPLX.forward calls it (num_betas=300, num_expression_coeffs=100,
use_pca=False): the pose mean (hand means) added to the full pose, shapedirs[..., :300] and the expression directions
shapedirs[..., 300:400] concatenated, J = J_regressor @ v_shaped (the joints move with the expression), batch_rodrigues
with its +1e-8, pose_feature = (R[1:] - I).flatten() against posedirs [V * 3, 486]^T, the rigid chain, linear blend
skinning, then transl.  Also the face scores of tools/evaluate.py:328-367.  smplx is a third-party package; this is test
infrastructure only and is never imported by the product."""
import numpy as np

N_JOINTS = 55
N_BETAS = 300
N_EXPR = 100


def load_model(path_or_dict, flat_hand_mean=False):
    m = np.load(path_or_dict) if isinstance(path_or_dict, str) else path_or_dict
    parents = np.asarray(m["kintree_table"])[0].astype(np.int64)
    parents[0] = -1
    sd = np.asarray(m["shapedirs"], np.float64)
    pose_mean = np.zeros(165)
    if not flat_hand_mean:
        pose_mean[75:120] = m["hands_meanl"]
        pose_mean[120:165] = m["hands_meanr"]
    nv = np.asarray(m["v_template"]).shape[0]
    return dict(parents=parents, v_template=np.asarray(m["v_template"], np.float64),
                dirs=np.concatenate([sd[..., :N_BETAS], sd[..., N_BETAS:N_BETAS + N_EXPR]], 2),
                posedirs=np.asarray(m["posedirs"], np.float64).reshape(nv * 3, -1).T,
                J_regressor=np.asarray(m["J_regressor"], np.float64), weights=np.asarray(m["weights"], np.float64),
                pose_mean=pose_mean)


def batch_rodrigues(rot_vecs):
    v = np.asarray(rot_vecs, np.float64).reshape(-1, 3)
    angle = np.linalg.norm(v + 1e-8, axis=1, keepdims=True)
    d = v / angle
    c, s = np.cos(angle)[:, :, None], np.sin(angle)[:, :, None]
    rx, ry, rz = d[:, 0], d[:, 1], d[:, 2]
    z = np.zeros_like(rx)
    K = np.stack([z, -rz, ry, rz, z, -rx, -ry, rx, z], axis=1).reshape(-1, 3, 3)
    return np.eye(3)[None] + s * K + (1.0 - c) * (K @ K)


def fold(poses):
    """evaluate.py:261-280's axis-angle -> 6D -> axis-angle round trip on exact arithmetic: each rotation vector's angle
    mapped into [0, pi] (an angle in (pi, 2 pi) becomes the opposite axis)."""
    p = np.asarray(poses, np.float64).reshape(-1, 3).copy()
    th = np.linalg.norm(p, axis=1)
    ph = np.mod(th, 2 * np.pi)
    s = np.where(th > 0, np.where(ph > np.pi, ph - 2 * np.pi, ph) / np.where(th > 0, th, 1), 0.0)
    return (p * s[:, None]).reshape(np.shape(poses))


def lbs(model, full_pose, betas=None, expression=None, transl=None, chunk=32):
    """full_pose [F, 165] in SMPL-X order, betas [<= 300] (one for all frames) or None, expression [F, 100] or None, transl
    [F, 3] or None -> (vertices [F, V, 3], joints [F, 55, 3]) float64 (joints without transl added, as J_transformed).
    Frames go through in chunks (memory only: every frame is computed on its own)."""
    p = np.asarray(full_pose, np.float64).reshape(-1, 165) + model["pose_mean"]
    F = p.shape[0]
    b = np.zeros(N_BETAS) if betas is None else np.asarray(betas, np.float64).reshape(-1)
    b = np.pad(b, (0, N_BETAS - b.shape[0]))
    e = np.zeros((F, N_EXPR)) if expression is None else np.asarray(expression, np.float64).reshape(F, N_EXPR)
    if F > chunk:
        parts = [lbs(model, (p - model["pose_mean"])[i:i + chunk], b, e[i:i + chunk],
                     None if transl is None else np.asarray(transl).reshape(F, 3)[i:i + chunk], chunk) for i in range(0, F, chunk)]
        return np.concatenate([v for v, _ in parts]), np.concatenate([j for _, j in parts])
    nv = model["v_template"].shape[0]
    coef = np.concatenate([np.broadcast_to(b, (F, N_BETAS)), e], 1)
    v_shaped = model["v_template"][None] + (coef @ model["dirs"].reshape(nv * 3, -1).T).reshape(F, nv, 3)
    J = np.einsum("jv,fvd->fjd", model["J_regressor"], v_shaped)
    R = batch_rodrigues(p.reshape(-1, 3)).reshape(F, N_JOINTS, 3, 3)
    pose_feature = (R[:, 1:] - np.eye(3)).reshape(F, -1)
    v_posed = v_shaped + (pose_feature @ model["posedirs"]).reshape(F, -1, 3)
    parents = model["parents"]
    rel = J.copy()
    rel[:, 1:] -= J[:, parents[1:]]
    T = np.zeros((F, N_JOINTS, 4, 4))
    T[:, :, :3, :3] = R
    T[:, :, :3, 3] = rel
    T[:, :, 3, 3] = 1.0
    chain = [T[:, 0]]
    for i in range(1, N_JOINTS):
        chain.append(chain[parents[i]] @ T[:, i])
    G = np.stack(chain, 1)
    joints = G[:, :, :3, 3].copy()
    A = G[:, :, :3, :].copy()
    A[:, :, :, 3] -= np.einsum("fjab,fjb->fja", G[:, :, :3, :3], J)
    Tv = (model["weights"][None] @ A.reshape(F, N_JOINTS, 12)).reshape(F, nv, 3, 4)
    verts = np.einsum("fvab,fvb->fva", Tv[..., :3], v_posed) + Tv[..., 3]
    if transl is not None:
        verts = verts + np.asarray(transl, np.float64).reshape(F, 1, 3)
    return verts, joints


def face_vertices(model, poses, exprs, betas):
    """evaluate.py:328-355 for one side of one clip: only the folded jaw, zero everything else, that side's expressions, the
    ground truth's betas -> [n, V * 3]."""
    n = poses.shape[0]
    full = np.zeros((n, 165))
    full[:, 66:69] = fold(np.asarray(poses, np.float64)[:, 66:69])
    return lbs(model, full, betas, exprs)[0].reshape(n, -1)


def face_scores(rec, tar):
    """(l2, lvel) contributions of one clip, evaluate.py:361-364, the reference's formulas in float64:
    MSELoss(rec, tar) * n and L1Loss(rec[1:] - tar[:-1], tar[1:] - tar[:-1]) * n."""
    n = rec.shape[0]
    l2 = np.mean((rec - tar) ** 2) * n
    lvel = np.mean(np.abs((rec[1:] - tar[:-1]) - (tar[1:] - tar[:-1]))) * n
    return l2, lvel


def face_scores_simplified(rec, tar):
    """The same two numbers from the identity (rec[t] - tar[t-1]) - (tar[t] - tar[t-1]) = rec[t] - tar[t]."""
    n = rec.shape[0]
    d = rec - tar
    return np.mean(d ** 2) * n, np.mean(np.abs(d[1:])) * n
