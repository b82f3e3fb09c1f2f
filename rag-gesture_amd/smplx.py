"""The SMPL-X model on the host and its joints on the device: what evaluation.py, mesh.py, dataset.py and render.py share.

load_smplx_model reads the joint side of SMPLX_NEUTRAL_2020.npz; SMPLXJoints runs the forward kinematics of the 55 joints
(rg_smplx_joints, and with expression / translation / strided raw rows rg_smplx_joints_expr; csrc/rg_smplx.h holds the
kinematics the kernels share).  clip_list() and offsets() are how every caller turns its poses into a list of [n_i, 165] clips
and the int32 row-offset table the kernels take.
"""
import collections
import ctypes
import os

import numpy as np
import torch

from . import capi

N_JOINTS = 55
IN_DIM = N_JOINTS * 3            # axis-angle channels of a pose row
N_BETAS = 300                    # smplx.create(..., num_betas=300) (evaluate.py:117-126)
N_EXPR = 100                     # num_expression_coeffs=100: shapedirs[..., 300:400]
EVAL_N = 300                     # evaluate.py:231-232: every clip is cut to its first 300 frames

SmplxJointsArgs = capi.struct("rg_smplx_joints_args")
SmplxJointsExprArgs = capi.struct("rg_smplx_joints_expr_args")


class SMPLXModelError(ValueError):
    pass


def clip_list(poses):
    """[B, n, 165] or [n, 165] axis-angle (tensor or array), or a list of [n_i, 165] clips -> the list of clips."""
    if torch.is_tensor(poses) or isinstance(poses, np.ndarray):
        if poses.ndim == 2:
            poses = poses[None]
        if poses.ndim != 3 or poses.shape[-1] != IN_DIM:
            raise ValueError("poses must be [B, n, %d] axis-angle, got %s" % (IN_DIM, tuple(poses.shape)))
        return [poses[b] for b in range(poses.shape[0])]
    clips = list(poses)
    for i, c in enumerate(clips):
        if c.ndim != 2 or c.shape[-1] != IN_DIM:
            raise ValueError("clip %d must be [n, %d] axis-angle, got %s" % (i, IN_DIM, tuple(c.shape)))
    return clips


def offsets(lens):
    """Clip lengths -> the int32 table [0, n_0, n_0 + n_1, ...] of the kernels' clip_off / raw_off / pair_off arguments."""
    off =np.zeros(len(lens) + 1, np.int32)
    off[1:] = np.cumsum(lens)
    return off


def load_smplx_model(src, flat_hand_mean=False):
    """SMPLX_NEUTRAL_2020.npz (a path or a mapping) -> dict of float64 arrays: parents [55] (root -1), J_template [55, 3] =
    J_regressor @ v_template, J_dirs [55, 3, 300] = J_regressor @ shapedirs[..., :300] and pose_mean [165] (zero but for the
    hand means hands_meanl / hands_meanr, which SMPLX.forward adds unless flat_hand_mean).  A file whose shapedirs hold the
    100 expression components too (the real one does) also gives J_expr [55, 3, 100] = J_regressor @ shapedirs[..., 300:400]:
    how the rest joints move with the expression.  Faces, skinning weights and posedirs are not read."""
    if isinstance(src, (str, os.PathLike)):
        with np.load(src, allow_pickle=False) as f:
            src = {k: f[k] for k in f.files}
    if not isinstance(src, collections.abc.Mapping):
        raise SMPLXModelError("expected a path or a mapping of SMPL-X arrays")

    def arr(key, ndim):
        if key not in src:
            raise SMPLXModelError("missing key %s" % key)
        v = np.asarray(src[key])
        if v.ndim != ndim:
            raise SMPLXModelError("%s has %d dimensions, expected %d" % (key, v.ndim, ndim))
        return v

    kt = arr("kintree_table", 2)
    if kt.shape != (2, N_JOINTS):
        raise SMPLXModelError("kintree_table has shape %s, expected (2, %d)" % (kt.shape, N_JOINTS))
    parents = kt[0].astype(np.int64)
    if parents[0] in (-1, 2 ** 32 - 1):
        parents[0] = -1
    else:
        raise SMPLXModelError("kintree_table root entry is %d, expected -1 or 2**32-1" % parents[0])
    for i in range(1, N_JOINTS):
        if not 0 <= parents[i] < i:
            raise SMPLXModelError("kintree_table: parent of joint %d is %d, not in [0, %d)" % (i, parents[i], i))
    jr = arr("J_regressor", 2).astype(np.float64)
    if jr.shape[0] != N_JOINTS:
        raise SMPLXModelError("J_regressor has shape %s, expected (%d, V)" % (jr.shape, N_JOINTS))
    nv = jr.shape[1]
    vt = arr("v_template", 2).astype(np.float64)
    if vt.shape != (nv, 3):
        raise SMPLXModelError("v_template has shape %s, expected (%d, 3)" % (vt.shape, nv))
    sd = arr("shapedirs", 3)
    if sd.shape[:2] != (nv, 3) or sd.shape[2] < N_BETAS:
        raise SMPLXModelError("shapedirs has shape %s, expected (%d, 3, >= %d)" % (sd.shape, nv, N_BETAS))
    ed = sd[..., N_BETAS:N_BETAS + N_EXPR].astype(np.float64) if sd.shape[2] >= N_BETAS + N_EXPR else None
    sd = sd[..., :N_BETAS].astype(np.float64)
    pose_mean = np.zeros(IN_DIM, np.float64)
    if not flat_hand_mean:
        for key, col in (("hands_meanl", 25 * 3), ("hands_meanr", 40 * 3)):
            hm = arr(key, 1)
            if hm.shape != (45,):
                raise SMPLXModelError("%s has shape %s, expected (45,)" % (key, hm.shape))
            pose_mean[col:col + 45] = hm
    for key, v in (("J_regressor", jr), ("v_template", vt), ("shapedirs", sd), ("pose_mean", pose_mean)):
        if not np.all(np.isfinite(v)):
            raise SMPLXModelError("%s holds non-finite values" % key)
    out = dict(parents=parents.astype(np.int32), J_template=jr @ vt, J_dirs=np.einsum("jv,vdk->jdk", jr, sd),
               pose_mean=pose_mean)
    if ed is not None:
        if not np.all(np.isfinite(ed)):
            raise SMPLXModelError("shapedirs holds non-finite values")
        out["J_expr"] = np.einsum("jv,vdk->jdk", jr, ed)
    return out


class SMPLXJoints:
    """The 55 posed SMPL-X joints of axis-angle clips on the device (rg_smplx_joints): the J_transformed that
    smplx.SMPLX.forward(..., return_joints=True) computes with zero translation and zero expression.  With `expressions=`
    or `transl=` (rg_smplx_joints_expr) the rest joints move with the expression and the translation is added: the joints of
    smplx.SMPLX.forward(betas, transl, expression, ...) as beatx_dataset.py:373-415 calls it."""

    def __init__(self, model_path_or_dict, flat_hand_mean=False, device=None):
        m = load_smplx_model(model_path_or_dict, flat_hand_mean)
        self.parents, self.J_template, self.J_dirs, self.pose_mean_host = m["parents"], m["J_template"], m["J_dirs"], m["pose_mean"]
        self.device = capi.device_or_fail(device, "SMPLXJoints")
        self.h = capi.get_handle(self.device.index)
        self.parents_dev = torch.from_numpy(self.parents).to(self.device)
        self.pose_mean = None if not np.any(self.pose_mean_host) else \
            torch.from_numpy(self.pose_mean_host.astype(np.float32)).to(self.device)
        self.J_expr = m.get("J_expr")               # None: the file holds no expression components
        self.j_expr_dev = None if self.J_expr is None else torch.from_numpy(self.J_expr.astype(np.float32)).to(self.device)

    def rest_joints(self, betas=None):
        """[55, 3] float64: J_template + J_dirs . betas (betas [<= 300], zero-padded; None: zeros)."""
        if betas is None:
            return self.J_template.copy()
        b = np.asarray(betas, np.float64).reshape(-1)
        if b.shape[0] > N_BETAS:
            raise ValueError("betas has %d entries, the model uses %d" % (b.shape[0], N_BETAS))
        return self.J_template + self.J_dirs[..., :b.shape[0]] @ b

    def joints_strided(self, poses, expressions, transl, raw_off, clip_off, stride, betas=None, fold=False):
        """rg_smplx_joints_expr on concatenated raw rows: poses [R, 165], expressions [R, 100] or None, transl [R, 3] or None
        (fp32 device tensors), raw_off / clip_off [n_clips + 1] int32 host tables (include/rg_gesture.h): output frame t of
        clip c reads raw row raw_off[c] + t * stride.  -> [clip_off[-1], 55, 3] fp32 device tensor."""
        n_clips = len(raw_off) - 1
        if expressions is not None and self.j_expr_dev is None:
            raise SMPLXModelError("the model file's shapedirs hold no expression components (expected >= %d columns)"
                                  % (N_BETAS + N_EXPR))
        if betas is not None and len(betas) != n_clips:
            raise ValueError("%d betas for %d clips" % (len(betas), n_clips))
        rest = np.stack([self.rest_joints(None if betas is None else betas[i]) for i in range(n_clips)])
        raw_off, clip_off = np.ascontiguousarray(raw_off, np.int32), np.ascontiguousarray(clip_off, np.int32)
        if clip_off[-1] >= 2 ** 31 // IN_DIM or raw_off[-1] >= 2 ** 31 // IN_DIM:
            raise ValueError("too many frames in one call (%d)" % max(clip_off[-1], raw_off[-1]))
        dev = self.device
        for t, w in ((poses, IN_DIM), (expressions, N_EXPR), (transl, 3)):
            if t is not None and (t.device != dev or t.dtype != torch.float32 or not t.is_contiguous()
                                  or tuple(t.shape) != (poses.shape[0], w)):
                raise ValueError("expected contiguous fp32 [%d, %d] tensors on %s" % (poses.shape[0], w, dev))
        rest_dev = torch.from_numpy(rest.astype(np.float32)).to(dev)
        roff_dev, coff_dev = torch.from_numpy(raw_off).to(dev), torch.from_numpy(clip_off).to(dev)
        out = torch.empty(int(clip_off[-1]), N_JOINTS, 3, device=dev, dtype=torch.float32)
        ptr = lambda t: None if t is None else t.data_ptr()
        a = SmplxJointsExprArgs(poses=poses.data_ptr(), exprs=ptr(expressions), transl=ptr(transl), rest=rest_dev.data_ptr(),
                                j_expr=ptr(self.j_expr_dev), pose_mean=ptr(self.pose_mean), parents=self.parents_dev.data_ptr(),
                                parents_host=self.parents.ctypes.data, clip_off=coff_dev.data_ptr(),
                                clip_off_host=clip_off.ctypes.data, raw_off=roff_dev.data_ptr(), raw_off_host=raw_off.ctypes.data,
                                joints=out.data_ptr(), n_clips=n_clips, raw_rows=int(poses.shape[0]), stride=int(stride),
                                fold=int(bool(fold)))
        self.h.call("smplx_joints_expr", ctypes.byref(a))
        return out

    def joints(self, poses, betas=None, fold=False, root_norm=False, expressions=None, transl=None):
        """poses: [B, n, 165] or a list of [n_i, 165] axis-angle clips (device or host); betas: None, or one [300] vector per
        clip.  -> [sum n_i, 55, 3] fp32 device tensor, clip after clip.  fold: the angle folding of evaluate.py's 6D round trip
        (include/rg_gesture.h).  root_norm: joints relative to the clip's root at frame 0 (evaluate.py:373-377; the posed root
        is the rest root for every frame, so the rest joints are shifted by it).
        expressions / transl: None, or per clip [n_i, 100] / [n_i, 3] in the layout of poses: the joints then move with the
        expression and the translation is added (rg_smplx_joints_expr; not with root_norm)."""
        clips = clip_list(poses)
        if not clips:
            raise ValueError("no clips")
        if betas is not None and len(betas) != len(clips):
            raise ValueError("%d betas for %d clips" % (len(betas), len(clips)))
        if expressions is not None or transl is not None:
            if root_norm:
                raise ValueError("root_norm is defined for joints without expression and translation")
            off = offsets([int(c.shape[0]) for c in clips])
            rows = lambda xs: [xs[b] for b in range(xs.shape[0])] if (torch.is_tensor(xs) or isinstance(xs, np.ndarray)) \
                and xs.ndim == 3 else ([xs] if (torch.is_tensor(xs) or isinstance(xs, np.ndarray)) else list(xs))
            cat = lambda xs, w: None if xs is None else torch.cat(
                [torch.as_tensor(x).reshape(-1, w).to(self.device, torch.float32) for x in rows(xs)], 0).contiguous()
            aa, ex, tr = cat(clips, IN_DIM), cat(expressions, N_EXPR), cat(transl, 3)
            for t, what in ((ex, "expressions"), (tr, "transl")):
                if t is not None and t.shape[0] != aa.shape[0]:
                    raise ValueError("%s hold %d frames, the poses %d" % (what, t.shape[0], aa.shape[0]))
            return self.joints_strided(aa, ex, tr, off, off, 1, betas=betas, fold=fold)
        rest = np.stack([self.rest_joints(None if betas is None else betas[i]) for i in range(len(clips))])
        if root_norm:
            rest = rest - rest[:, :1]
        off = offsets([int(c.shape[0]) for c in clips])
        if off[-1] >= 2 ** 31 // IN_DIM:
            raise ValueError("too many frames in one call (%d)" % off[-1])
        dev = self.device
        aa = torch.cat([torch.as_tensor(c).to(dev, torch.float32) for c in clips], 0).contiguous()
        rest_dev = torch.from_numpy(rest.astype(np.float32)).to(dev)
        off_dev = torch.from_numpy(off).to(dev)
        out = torch.empty(int(off[-1]), N_JOINTS, 3, device=dev, dtype=torch.float32)
        a = SmplxJointsArgs(poses=aa.data_ptr(), rest=rest_dev.data_ptr(),
                            pose_mean=None if self.pose_mean is None else self.pose_mean.data_ptr(),
                            parents=self.parents_dev.data_ptr(), parents_host=self.parents.ctypes.data,
                            clip_off=off_dev.data_ptr(), clip_off_host=off.ctypes.data, joints=out.data_ptr(),
                            n_clips=len(clips), fold=int(bool(fold)))
        self.h.call("smplx_joints", ctypes.byref(a))
        return out
