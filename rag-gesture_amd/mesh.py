"""SMPL-X mesh vertices on the device and the face metrics of the reference's tools/evaluate.py (l2 loss, lvel loss).

    load_smplx_mesh  SMPLX_NEUTRAL_2020.npz -> float64 arrays: bases, J_regressor products, sparse skinning lists
    SMPLXMesh        smplx.lbs as SMPLX.forward calls it: rg_mesh_transforms (per frame: coefficients, skinning transforms)
                     + rg_mesh_blend_skin (blend-shape GEMM on fp32 MFMA, skinning in its epilogue)
    FaceMetrics      evaluate.py:328-367, :431-432: per clip the mean squared and (frame 0 excluded) mean absolute difference
                     of the predicted and ground-truth face meshes, summed on the device per clip (rg_mesh_face_sums)

A call gathers only its active blend columns into a basis [K x 3V] cached per mode:
    "full"  the 100 expression and 486 pose-feature columns (vertices());
    "face"  the 100 expression columns and the jaw's 9 (FaceMetrics).  evaluate.py's face calls pose only the jaw: the other
            pose features are R - I = 0 (zero rotations) or constant (the hands' mean pose), so they go into the base in
            float64 on the host;
    "beta"  the 300 shape columns: the per-clip base v_template + shapedirs . betas (+ the constant columns) is a GEMM with
            one row per clip.
The joints come from J_regressor . v_shaped, so they move with the expression: J = J_clip + J_expr . psi per frame.
DESIGN.md "SMPL-X face metrics" covers precision, determinism and the lvel identity.
"""
import collections
import ctypes

import numpy as np
import torch

from . import capi
from .smplx import EVAL_N, IN_DIM, N_BETAS, N_EXPR, N_JOINTS, SMPLXModelError, clip_list, load_smplx_model, offsets

N_POSE_FEAT = (N_JOINTS - 1) * 9
JAW = 22
ROW_TILE = 64                    # rows of a rg_mesh_blend_skin tile
VERT_TILE = 64                   # vertices of a tile (192 columns)
K_STEP = 16
FACE_GROUPS = 8                  # vertex-tile groups of a face launch (at most; fixed per model, so the per-clip sums do not
                                 # depend on the batch)
RG_MESH_RAW, RG_MESH_VERTICES, RG_MESH_FACE = (capi.header_constants()[k] for k in ("RG_MESH_RAW", "RG_MESH_VERTICES", "RG_MESH_FACE"))

MeshTransformsArgs = capi.struct("rg_mesh_transforms_args")
MeshBlendArgs = capi.struct("rg_mesh_blend_args")
MeshFaceSumsArgs = capi.struct("rg_mesh_face_sums_args")


def _round_up(x, m):
    return -(-x // m) * m


def rodrigues64(v):
    """smplx.lbs.batch_rodrigues in float64: [N, 3] -> [N, 3, 3] (with its +1e-8 inside the norm)."""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    ang = np.linalg.norm(v + 1e-8, axis=1, keepdims=True)
    d = v / ang
    c, s = np.cos(ang)[:, :, None], np.sin(ang)[:, :, None]
    z = np.zeros(len(v))
    K = np.stack([z, -d[:, 2], d[:, 1], d[:, 2], z, -d[:, 0], -d[:, 1], d[:, 0], z], 1).reshape(-1, 3, 3)
    return np.eye(3)[None] + s * K + (1.0 - c) * (K @ K)


def load_smplx_mesh(src, flat_hand_mean=False):
    """SMPLX_NEUTRAL_2020.npz (a path or a mapping) -> dict, float64 unless noted: everything load_smplx_model returns, plus
    v_template [V, 3], shape_dirs [V, 3, 300], expr_dirs [V, 3, 100] (shapedirs[..., 300:400]), posedirs [V, 3, 486],
    J_expr [55, 3, 100] = J_regressor @ expr_dirs, and the exact nonzeros of weights [V, 55] as per-vertex lists: skin_n [V]
    int32, skin_j [V, max_nnz] int32, skin_w [V, max_nnz] (zero-padded), max_nnz, and faces: the triangle list `f` as [F, 3]
    int32, or None when the file holds no `f` (only rendering needs it: render.SMPLXRenderer)."""
    if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__"):
        with np.load(src, allow_pickle=False) as f:
            src = {k: f[k] for k in f.files}
    if not isinstance(src, collections.abc.Mapping):
        raise SMPLXModelError("expected a path or a mapping of SMPL-X arrays")
    base = load_smplx_model(src, flat_hand_mean)
    nv = np.asarray(src["J_regressor"]).shape[1]

    def arr(key, shape, what):
        if key not in src:
            raise SMPLXModelError("missing key %s" % key)
        v = np.asarray(src[key])
        if v.ndim != len(shape) or any(w is not None and s != w for s, w in zip(v.shape, shape)):
            raise SMPLXModelError("%s has shape %s, expected %s" % (key, v.shape, what))
        v = v.astype(np.float64)
        if not np.all(np.isfinite(v)):
            raise SMPLXModelError("%s holds non-finite values" % key)
        return v

    vt = arr("v_template", (nv, 3), "(%d, 3)" % nv)
    sd = arr("shapedirs", (nv, 3, None), "(%d, 3, >= %d)" % (nv, N_BETAS + N_EXPR))
    if sd.shape[2] < N_BETAS + N_EXPR:
        raise SMPLXModelError("shapedirs has shape %s, expected (%d, 3, >= %d): 300 shape and 100 expression components"
                              % (sd.shape, nv, N_BETAS + N_EXPR))
    pd = arr("posedirs", (nv, 3, N_POSE_FEAT), "(%d, 3, %d)" % (nv, N_POSE_FEAT))
    w = arr("weights", (nv, N_JOINTS), "(%d, %d)" % (nv, N_JOINTS))
    jr = np.asarray(src["J_regressor"], np.float64)
    nz = w != 0
    skin_n = nz.sum(1).astype(np.int32)
    max_nnz = max(1, int(skin_n.max()))             # (a vertex without weights skins to the origin, as in smplx.lbs)
    skin_j = np.zeros((nv, max_nnz), np.int32)
    skin_w = np.zeros((nv, max_nnz), np.float64)
    for v in range(nv):
        j = np.nonzero(nz[v])[0]
        skin_j[v, :len(j)] = j
        skin_w[v, :len(j)] = w[v, j]
    faces = None
    if "f" in src:
        faces = np.asarray(src["f"])
        if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or faces.dtype.kind not in "iu":
            raise SMPLXModelError("f has shape %s and type %s, expected integer (F, 3)" % (faces.shape, faces.dtype))
        if int(faces.min()) < 0 or int(faces.max()) >= nv:
            raise SMPLXModelError("f holds vertex indices outside [0, %d)" % nv)
        faces = np.ascontiguousarray(faces, np.int32)
    expr = sd[..., N_BETAS:N_BETAS + N_EXPR]
    base.update(faces=faces, v_template=vt, shape_dirs=sd[..., :N_BETAS], expr_dirs=expr, posedirs=pd, weights=w,
                J_expr=np.einsum("jv,vdk->jdk", jr, expr), skin_n=skin_n, skin_j=skin_j, skin_w=skin_w, max_nnz=max_nnz,
                n_verts=nv)
    return base


class SMPLXMesh:
    """SMPL-X vertices of axis-angle clips on the device: what smplx.SMPLX.forward(...)["vertices"] computes (num_betas=300,
    num_expression_coeffs=100, use_pca=False).  No CPU fallback: capi.RgError without a GPU."""

    def __init__(self, model_path_or_dict, flat_hand_mean=False, device=None):
        m = load_smplx_mesh(model_path_or_dict, flat_hand_mean)
        self.model = m
        self.n_verts, self.max_nnz = m["n_verts"], m["max_nnz"]
        self.faces = m["faces"]                      # [F, 3] int32 (host) or None: the model file's triangle list
        self.d_pad = 3 * _round_up(self.n_verts, VERT_TILE)
        self.device = capi.device_or_fail(device, "SMPLXMesh")
        self.h = capi.get_handle(self.device.index)
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(self.device, dt)
        self.parents = m["parents"]
        self.parents_dev = dev(self.parents, torch.int32)
        self.pose_mean_host = m["pose_mean"]
        self.pose_mean = None if not np.any(self.pose_mean_host) else dev(self.pose_mean_host, torch.float32)
        self.j_expr = dev(m["J_expr"], torch.float32)
        self.skin_n, self.skin_j = dev(m["skin_n"], torch.int32), dev(m["skin_j"], torch.int32)
        self.skin_w = dev(m["skin_w"], torch.float32)
        self._modes = {}

    # ---------------------------------------------------------------------------------------------- per-mode bases
    def _pad_cols(self, x):
        """[K, V, 3] float64 -> [K, d_pad] float64, column 3v + c."""
        out = np.zeros((x.shape[0], self.d_pad))
        out[:, :3 * self.n_verts] = x.reshape(x.shape[0], -1)
        return out

    def _mode(self, mode):
        """(basis [k_pad, d_pad] fp32 device, constant base [1, d_pad] fp32 device, pf_col [55] int32 host + device, k_pad)."""
        if mode in self._modes:
            return self._modes[mode]
        m = self.model
        const = m["v_template"].copy()
        pf_col = np.full(N_JOINTS, -1, np.int32)
        if mode == "beta":
            cols = np.moveaxis(m["shape_dirs"], 2, 0)
        else:
            pose_cols = [JAW] if mode == "face" else list(range(1, N_JOINTS))
            for i, j in enumerate(pose_cols):
                pf_col[j] = N_EXPR + 9 * i
            sel = np.concatenate([np.arange(9 * (j - 1), 9 * j) for j in pose_cols])
            cols = np.concatenate([np.moveaxis(m["expr_dirs"], 2, 0), np.moveaxis(m["posedirs"][..., sel], 2, 0)], 0)
            if mode == "face":
                # every other joint: R = I exactly (zero pose, +1e-8 inside the norm) or the hand mean, the same in every row
                feat = (rodrigues64(self.pose_mean_host.reshape(N_JOINTS, 3))[1:] - np.eye(3)).reshape(-1)
                feat[9 * (JAW - 1):9 * JAW] = 0.0
                const += np.einsum("vdk,k->vd", m["posedirs"], feat)
        k_pad = _round_up(cols.shape[0], K_STEP)
        basis = np.zeros((k_pad, self.d_pad))
        basis[:cols.shape[0]] = self._pad_cols(cols)
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(self.device, dt)
        entry = (dev(basis, torch.float32), dev(self._pad_cols(const[None]), torch.float32), pf_col, dev(pf_col, torch.int32), k_pad)
        self._modes[mode] = entry
        return entry

    def _clip_bases(self, betas, const):
        """Per clip v_template + shapedirs . betas (+ the mode's constant columns): rg_mesh_blend_skin RAW, one row per clip.
        -> [C, d_pad] fp32 device."""
        basis, _, _, _, k_pad = self._mode("beta")
        C = len(betas)
        coeff = torch.zeros(_round_up(C, ROW_TILE), k_pad, dtype=torch.float32)
        coeff[:C, :N_BETAS] = torch.from_numpy(np.stack(betas))
        coeff = coeff.to(self.device)
        out = torch.empty(C, self.d_pad, device=self.device, dtype=torch.float32)
        a = MeshBlendArgs(coeff=coeff.data_ptr(), basis=basis.data_ptr(), base=const.data_ptr(), out=out.data_ptr(),
                          mode=RG_MESH_RAW, n_clips=1, rows=C, coeff_rows=coeff.shape[0], k_pad=k_pad, n_verts=self.n_verts,
                          d_pad=self.d_pad, max_nnz=self.max_nnz, n_groups=1, base_per_clip=0)
        self.h.call("mesh_blend_skin", ctypes.byref(a))
        return out

    def _betas(self, betas, C):
        if betas is None:
            return [np.zeros(N_BETAS)] * C
        if len(betas) != C:
            raise ValueError("%d betas for %d clips" % (len(betas), C))
        out = []
        for b in betas:
            b = np.asarray(b, np.float64).reshape(-1)
            if b.shape[0] > N_BETAS:
                raise ValueError("betas has %d entries, the model uses %d" % (b.shape[0], N_BETAS))
            out.append(np.pad(b, (0, N_BETAS - b.shape[0])))
        return out

    def _transforms(self, poses, exprs, betas, off, mode, fold, joints=None):
        """rg_mesh_transforms for rows poses [R, 165] / exprs [R, 100] (device) of clips off (rows) with betas [C][300]
        -> (coeff [R rounded up to 64, k_pad], A [R, 55, 12], the mode entry)."""
        entry = self._mode(mode)
        _, _, pf_host, pf_dev, k_pad = entry
        m = self.model
        jclip = m["J_template"][None] + np.einsum("jdk,ck->cjd", m["J_dirs"], np.stack(betas))
        jclip_dev = torch.from_numpy(jclip.astype(np.float32)).to(self.device)
        R = int(off[-1])
        coeff = torch.zeros(_round_up(max(R, 1), ROW_TILE), k_pad, device=self.device, dtype=torch.float32)
        A = torch.empty(R, N_JOINTS, 12, device=self.device, dtype=torch.float32)
        off_dev = torch.from_numpy(off).to(self.device)
        a = MeshTransformsArgs(poses=poses.data_ptr(), exprs=None if exprs is None else exprs.data_ptr(),
                               j_clip=jclip_dev.data_ptr(), j_expr=self.j_expr.data_ptr(),
                               pose_mean=None if self.pose_mean is None else self.pose_mean.data_ptr(),
                               parents=self.parents_dev.data_ptr(), parents_host=self.parents.ctypes.data,
                               clip_off=off_dev.data_ptr(), clip_off_host=off.ctypes.data, pf_col=pf_dev.data_ptr(),
                               pf_col_host=pf_host.ctypes.data, coeff=coeff.data_ptr(), A=A.data_ptr(),
                               joints=None if joints is None else joints.data_ptr(), n_clips=len(off) - 1, k_pad=k_pad,
                               fold=int(bool(fold)))
        self.h.call("mesh_transforms", ctypes.byref(a))
        return coeff, A, entry, off_dev

    @staticmethod
    def _rows(clips, lens, width, what, dev):
        """Per clip [>= n_i, width] (or None: zeros) -> [sum n_i, width] fp32 device."""
        if clips is None:
            return None
        if len(clips) != len(lens):
            raise ValueError("%d %s for %d clips" % (len(clips), what, len(lens)))
        out = []
        for i, (c, n) in enumerate(zip(clips, lens)):
            c = torch.as_tensor(c)
            if c.ndim != 2 or c.shape[1] != width or c.shape[0] < n:
                raise ValueError("clip %d: %s must be [>= %d, %d], got %s" % (i, what, n, width, tuple(c.shape)))
            out.append(c[:n].to(dev, torch.float32))
        return torch.cat(out, 0).contiguous()

    def vertices(self, poses, betas=None, expressions=None, transl=None, fold=False, joints=None):
        """poses: [B, n, 165] or a list of [n_i, 165] axis-angle clips (device or host); betas: None or one [<= 300] per clip;
        expressions / transl: None or per clip [>= n_i, 100] / [>= n_i, 3].  fold: evaluate.py's 6D round trip (angles into
        [0, pi]).  -> [sum n_i, V, 3] fp32 device tensor, clip after clip.  joints: an optional [sum n_i, 55, 3] fp32 device
        tensor that receives the posed joints (without transl)."""
        clips = clip_list(poses)
        if not clips:
            raise ValueError("no clips")
        lens = [int(c.shape[0]) for c in clips]
        off = offsets(lens)
        R = int(off[-1])
        if R >= 2 ** 31 // max(self.d_pad, N_JOINTS * 12):
            raise ValueError("too many frames in one call (%d)" % R)
        dev = self.device
        b = self._betas(betas, len(clips))
        aa = torch.cat([torch.as_tensor(c).to(dev, torch.float32) for c in clips], 0).contiguous()
        ex = self._rows(expressions, lens, N_EXPR, "expressions", dev)
        tr = self._rows(transl, lens, 3, "transl", dev)
        if joints is not None and (tuple(joints.shape) != (R, N_JOINTS, 3) or joints.dtype != torch.float32 or not joints.is_cuda):
            raise ValueError("joints must be a [%d, 55, 3] fp32 device tensor" % R)
        coeff, A, (basis, const, _, _, k_pad), off_dev = self._transforms(aa, ex, b, off, "full", fold, joints)
        bases = self._clip_bases(b, const)
        out = torch.empty(R, self.n_verts, 3, device=dev, dtype=torch.float32)
        if R == 0:
            return out
        a = MeshBlendArgs(coeff=coeff.data_ptr(), basis=basis.data_ptr(), base=bases.data_ptr(), clip_off=off_dev.data_ptr(),
                          clip_off_host=off.ctypes.data, A=A.data_ptr(), skin_n=self.skin_n.data_ptr(),
                          skin_j=self.skin_j.data_ptr(), skin_w=self.skin_w.data_ptr(),
                          transl=None if tr is None else tr.data_ptr(), out=out.data_ptr(), mode=RG_MESH_VERTICES,
                          n_clips=len(clips), rows=R, coeff_rows=coeff.shape[0], k_pad=k_pad, n_verts=self.n_verts,
                          d_pad=self.d_pad, max_nnz=self.max_nnz, n_groups=1, base_per_clip=1)
        self.h.call("mesh_blend_skin", ctypes.byref(a))
        return out

    def face_sums(self, pred_jaw, gt_jaw, pred_exprs, gt_exprs, betas, lens):
        """The face launch: per clip i of lens[i] frames, pred_jaw / gt_jaw [sum lens, 3] and pred_exprs / gt_exprs
        [sum lens, 100] (device, clip after clip), betas [C][300] -> [C, 2] float64 host: sum over frames of the sums over
        vertices and coordinates of (rec - tar)^2, and the same of |rec - tar| over frames 1..n-1 (folded jaws, zero body,
        hands at their mean, the gt betas for both: evaluate.py:328-355)."""
        dev = self.device
        F = int(sum(lens))
        poses = torch.zeros(2 * F, IN_DIM, device=dev, dtype=torch.float32)
        poses[0::2, 3 * JAW:3 * JAW + 3] = pred_jaw
        poses[1::2, 3 * JAW:3 * JAW + 3] = gt_jaw
        exprs = torch.empty(2 * F, N_EXPR, device=dev, dtype=torch.float32)
        exprs[0::2], exprs[1::2] = pred_exprs, gt_exprs
        pair_off = offsets(lens)
        off = np.ascontiguousarray(2 * pair_off, np.int32)
        coeff, A, (basis, const, _, _, k_pad), off_dev = self._transforms(poses, exprs, betas, off, "face", True)
        bases = self._clip_bases(betas, const)
        groups = min(FACE_GROUPS, self.d_pad // (3 * VERT_TILE))
        partial = torch.empty(F * groups * 2, device=dev, dtype=torch.float64)
        a = MeshBlendArgs(coeff=coeff.data_ptr(), basis=basis.data_ptr(), base=bases.data_ptr(), clip_off=off_dev.data_ptr(),
                          clip_off_host=off.ctypes.data, A=A.data_ptr(), skin_n=self.skin_n.data_ptr(),
                          skin_j=self.skin_j.data_ptr(), skin_w=self.skin_w.data_ptr(), partial=partial.data_ptr(),
                          partial_len=partial.numel(), mode=RG_MESH_FACE, n_clips=len(lens), rows=2 * F,
                          coeff_rows=coeff.shape[0], k_pad=k_pad, n_verts=self.n_verts, d_pad=self.d_pad,
                          max_nnz=self.max_nnz, n_groups=groups, base_per_clip=1)
        self.h.call("mesh_blend_skin", ctypes.byref(a))
        sums = torch.empty(len(lens), 2, device=dev, dtype=torch.float64)
        pair_dev = torch.from_numpy(pair_off).to(dev)
        s = MeshFaceSumsArgs(partial=partial.data_ptr(), pair_off=pair_dev.data_ptr(), pair_off_host=pair_off.ctypes.data,
                             sums=sums.data_ptr(), n_clips=len(lens), n_groups=groups)
        self.h.call("mesh_face_sums", ctypes.byref(s))
        return sums.cpu().numpy()


class FaceMetrics:
    """l2 loss and lvel loss of evaluate.py:328-367, :431-432 over clips added batch by batch.  Per clip of n frames and
    D = 3V coordinates: l2 += mean((rec - tar)^2) * n, lvel += mean over frames 1..n-1 of |rec - tar| * n (the reference's
    |(rec[1:] - tar[:-1]) - (tar[1:] - tar[:-1])|, simplified); both are divided by the total frame count."""

    def __init__(self, mesh, eval_n=EVAL_N):
        self.mesh, self.eval_n = mesh, int(eval_n)
        self.reset()

    def reset(self):
        self.l2, self.lvel, self.frames, self.clips = 0.0, 0.0, 0, 0
        self.clip_sums = []

    def add(self, pred_poses, gt_poses, pred_exprs, gt_exprs, betas=None, names=None):
        """pred_poses / gt_poses: [B, n, 165] or lists of [n_i, 165] axis-angle clips; pred_exprs / gt_exprs: per clip
        [>= n, 100]; betas: the ground truth's [<= 300] per clip (used for both, evaluate.py:226) or None (zeros).  Each clip is
        truncated to eval_n frames, its ground truth to the prediction's length.  -> the clips' [C, 2] float64 sums (see
        SMPLXMesh.face_sums)."""
        sm = self.mesh
        pred, gt = clip_list(pred_poses), clip_list(gt_poses)
        C = len(pred)
        if len(gt) != C:
            raise ValueError("%d predicted clips but %d ground-truth clips" % (C, len(gt)))
        for what, v in (("pred_exprs", pred_exprs), ("gt_exprs", gt_exprs), ("betas", betas), ("names", names)):
            if v is not None and len(v) != C:
                raise ValueError("%d %s for %d clips" % (len(v), what, C))
        if C == 0:
            raise ValueError("no clips")
        name = lambda i: names[i] if names is not None else "clip %d" % (self.clips + i)
        lens = []
        for i in range(C):
            n = min(int(pred[i].shape[0]), self.eval_n)
            if int(gt[i].shape[0]) < n:
                raise ValueError("%s: ground truth has %d frames, the prediction %d" % (name(i), gt[i].shape[0], n))
            if n < 2:
                raise ValueError("%s: %d frames, the face metrics need at least 2 (the reference's lvel is NaN)" % (name(i), n))
            for what, e in (("predicted", pred_exprs[i]), ("ground-truth", gt_exprs[i])):
                if e.ndim != 2 or e.shape[1] != N_EXPR:
                    raise ValueError("%s: %s expressions must be [n, %d], got %s" % (name(i), what, N_EXPR, tuple(e.shape)))
                if int(e.shape[0]) < n:
                    raise ValueError("%s: %s expressions have %d rows, the clip %d frames" % (name(i), what, e.shape[0], n))
            lens.append(n)
        dev = sm.device

        def cat(xs, sl):
            parts = [x[:n][:, sl] for x, n in zip(xs, lens)]
            if all(isinstance(q, np.ndarray) for q in parts):           # one host -> device copy
                return torch.from_numpy(np.ascontiguousarray(np.concatenate(parts, 0), np.float32)).to(dev)
            return torch.cat([torch.as_tensor(q).to(dev, torch.float32) for q in parts], 0)
        jaw = slice(3 * JAW, 3 * JAW + 3)
        sums = sm.face_sums(cat(pred, jaw), cat(gt, jaw), cat(pred_exprs, slice(None)), cat(gt_exprs, slice(None)),
                            sm._betas(betas, C), lens)
        D = 3 * sm.n_verts
        for (s2, s1), n in zip(sums.tolist(), lens):
            self.l2 += s2 / (n * D) * n                  # evaluate.py:361-364: MSELoss(...).item() * n
            self.lvel += s1 / ((n - 1) * D) * n          # L1Loss over (n - 1) x D, * n
        self.frames += sum(lens)
        self.clips += C
        self.clip_sums.append(sums)
        return sums

    def compute(self):
        """-> dict(l2, lvel), float64."""
        if not self.clips:
            raise ValueError("no clips added")
        return dict(l2=self.l2 / self.frames, lvel=self.lvel / self.frames)
