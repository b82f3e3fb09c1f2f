"""A float64 NumPy restatement of the SMPL-X forward kinematics used by the joint metrics: smplx.lbs.batch_rodrigues and
batch_rigid_transform (the posed joints J_transformed), with the rest joints J_regressor (v_template + shapedirs . betas) and the
pose_mean (hand means) that smplx.SMPLX.forward adds.  smplx is a third-party package; this is test infrastructure only and is
never imported by the product."""
import numpy as np

N_JOINTS = 55


def load_model(path_or_dict, num_betas=300):
    """-> dict(parents [55] int64 (root -1), J_template [55, 3], J_dirs [55, 3, num_betas], pose_mean [165]) in float64."""
    m = np.load(path_or_dict) if isinstance(path_or_dict, str) else path_or_dict
    parents = np.asarray(m["kintree_table"])[0].astype(np.int64)
    parents[0] = -1
    jr = np.asarray(m["J_regressor"], np.float64)
    vt = np.asarray(m["v_template"], np.float64)
    sd = np.asarray(m["shapedirs"], np.float64)[..., :num_betas]
    pose_mean = np.zeros(165)
    pose_mean[75:120] = m["hands_meanl"]
    pose_mean[120:165] = m["hands_meanr"]
    return dict(parents=parents, J_template=jr @ vt, J_dirs=np.einsum("jv,vdk->jdk", jr, sd), pose_mean=pose_mean)


def rest_joints(model, betas=None):
    if betas is None:
        return model["J_template"].copy()
    b = np.asarray(betas, np.float64).reshape(-1)
    return model["J_template"] + model["J_dirs"][..., :b.shape[0]] @ b


def batch_rodrigues(rot_vecs):
    """[N, 3] -> [N, 3, 3], with smplx's +1e-8 inside the norm."""
    v = np.asarray(rot_vecs, np.float64)
    angle = np.linalg.norm(v + 1e-8, axis=1, keepdims=True)
    d = v / angle
    c, s = np.cos(angle)[:, :, None], np.sin(angle)[:, :, None]
    rx, ry, rz = d[:, 0], d[:, 1], d[:, 2]
    z = np.zeros_like(rx)
    K = np.stack([z, -rz, ry, rz, z, -rx, -ry, rx, z], axis=1).reshape(-1, 3, 3)
    return np.eye(3)[None] + s * K + (1.0 - c) * (K @ K)


def posed_joints(full_pose, rest, parents, pose_mean=None):
    """full_pose [F, 165] axis-angle in SMPL-X full_pose order, rest [55, 3] or [F, 55, 3] -> [F, 55, 3] float64."""
    p = np.asarray(full_pose, np.float64).reshape(-1, 165)
    if pose_mean is not None:
        p = p + pose_mean
    F = p.shape[0]
    R = batch_rodrigues(p.reshape(-1, 3)).reshape(F, N_JOINTS, 3, 3)
    J = np.broadcast_to(np.asarray(rest, np.float64), (F, N_JOINTS, 3))
    rel = J.copy()
    rel[:, 1:] -= J[:, parents[1:]]
    G = np.zeros((F, N_JOINTS, 4, 4))
    G[:, :, :3, :3] = R
    G[:, :, :3, 3] = rel
    G[:, :, 3, 3] = 1.0
    chain = [G[:, 0]]
    for i in range(1, N_JOINTS):
        chain.append(chain[parents[i]] @ G[:, i])
    return np.stack(chain, axis=1)[:, :, :3, 3]
