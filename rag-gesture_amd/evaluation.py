"""Fréchet gesture distance (FGD): the FGD half of the reference's tools/evaluate.py, on the device.

    aa [n, 165] --rg_aa_to_6d--> 6D [n, 330] --4 x rg_fgd_encoder_layer--> latents [n/16, 240]   (evaluate.py:255-275)
    latents --rg_latent_moments (fp64)--> mean, covariance --numpy float64 eigh--> FGD          (evaluate.py:436, metric.py:246-321)

The encoder is EMAGE's VAESKConv.map2latent (eval_models/model.py:12-107, :231-251) with the hyper-parameters evaluate.py:87-97
sets; its whole structure (block masks, pool matrices) is read from the checkpoint's state dict, so no SMPL-X file is needed.
`tr sqrtm(S1 S2)` is computed as the sum of sqrt(eigenvalues of A S2 A), A = S1^(1/2), both by numpy.linalg.eigh with negative
eigenvalues clipped to 0: it never yields the reference's imaginary-component ValueError (-> 1e10), the one deliberate
difference (DESIGN.md "FGD evaluation").

The joint half (DESIGN.md "SMPL-X joint metrics"): SMPLXJoints (smplx.py) runs the forward kinematics of the 55 SMPL-X joints
(rg_smplx_joints), JointMetrics the L1div, beat alignment, diversity and MPJPE numbers of evaluate.py:286-464
(rg_joint_clip_stats, rg_pair_distance_sums, GAHR on the host in float64), multimodality() the mm_all of evaluate_mm.py.
With one sem_score vector per clip JointMetrics adds SRGR (evaluate.py:413-426, metric.py:30-52): sem_at_pose_rate resamples the
vector on the host, rg_srgr_clip_sums counts and weighs the joint-frames under the threshold on the device.
The onsets of beat alignment are passed in, or detected from the clips' audio on the device (onsets="device", audio.py).
With foot=True (--foot) the foot skating numbers of foot.FootMetrics are added (this project's own: DESIGN.md "Foot skating").
"""
import argparse
import collections
import ctypes
import glob
import json
import math
import os
import time

import numpy as np
import torch

from . import capi
from .capi import device_or_fail as _device_or_fail  # noqa: F401  (the name callers and tests read from here)
from .mesh import FaceMetrics, SMPLXMesh, load_smplx_mesh  # noqa: F401
from .smplx import (EVAL_N, IN_DIM, N_BETAS, N_EXPR, N_JOINTS, SMPLXJoints, SMPLXModelError,  # noqa: F401
                    SmplxJointsArgs, SmplxJointsExprArgs, clip_list, load_smplx_model, offsets)

SIX_D = N_JOINTS * 6             # the encoder's input (evaluate.py:262-264)
LATENT_DIM = 240                 # vae_length
N_LAYERS = 4                     # vae_layer
GROUPS = 10                      # skeleton.py:575 nn.GroupNorm(10, out_channels)
GN_EPS = 1e-5
TIME_STRIDE = 1 << N_LAYERS      # frames per latent row
WINDOW = 32                      # vae_test_len: evaluate.py trims every clip to a multiple of it

FgdLayerArgs = capi.struct("rg_fgd_layer_args")


class FGDCheckpointError(ValueError):
    pass


# ---------------------------------------------------------------------------------------------------- checkpoint -> packed layers
def _load_state(src):
    """evaluate.py:29-48: a path (torch.save'd dict with "model_state"), a model_state mapping or a VAESKConv state dict;
    a `module.` prefix (DataParallel) is stripped when the first key has one."""
    if isinstance(src, (str, os.PathLike)):
        obj = torch.load(src, map_location="cpu", weights_only=True)
        if not isinstance(obj, collections.abc.Mapping) or "model_state" not in obj:
            raise FGDCheckpointError("%s: expected a checkpoint dict with a 'model_state' entry" % (src,))
        src = obj["model_state"]
    elif isinstance(src, collections.abc.Mapping) and "model_state" in src:
        src = src["model_state"]
    if not isinstance(src, collections.abc.Mapping) or not src:
        raise FGDCheckpointError("expected a non-empty state dict")
    keys = list(src.keys())
    strip = keys[0].startswith("module.")
    out = {}
    for k, v in src.items():
        k = k[len("module."):] if strip and k.startswith("module.") else k
        out[k] = v.detach().to("cpu", torch.float64).numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64)
    return out


def _get(sd, key, shape):
    if key not in sd:
        raise FGDCheckpointError("missing key %s" % key)
    v = sd[key]
    if tuple(v.shape) != tuple(shape):
        raise FGDCheckpointError("%s has shape %s, expected %s" % (key, tuple(v.shape), tuple(shape)))
    if not np.all(np.isfinite(v)):
        raise FGDCheckpointError("%s holds non-finite values" % key)
    return v


def _shape_of(sd, key, ndim):
    if key not in sd:
        raise FGDCheckpointError("missing key %s" % key)
    if sd[key].ndim != ndim:
        raise FGDCheckpointError("%s has %d dimensions, expected %d" % (key, sd[key].ndim, ndim))
    return sd[key].shape


def _check_mask(key, mask, edges, cpe_in, cpe_out):
    """A SkeletonConv mask (skeleton.py:58-61): 0 / 1, the same for every tap, and per output edge one set of whole input edges."""
    if not np.all((mask == 0) | (mask == 1)):
        raise FGDCheckpointError("%s is not a 0/1 mask" % key)
    m = mask[:, :, 0]
    if not np.all(mask == m[:, :, None]):
        raise FGDCheckpointError("%s differs between kernel taps" % key)
    blocks = m.reshape(edges, cpe_out, edges, cpe_in)
    if not (np.all(blocks == blocks[:, :1]) and np.all(blocks == blocks[:, :, :, :1])):
        raise FGDCheckpointError("%s is not block-structured by edge (%d edges, %d -> %d channels per edge)"
                                 % (key, edges, cpe_in, cpe_out))
    if not np.all(m.any(axis=1)):
        raise FGDCheckpointError("%s leaves an output channel without inputs" % key)
    return m


def _check_pool(key, w, edges, cpe):
    """A SkeletonPool matrix (skeleton.py:229-234): every output edge the mean of 1+ input edges, channel by channel, every input
    edge used once.  -> (source channels, weights) per output channel, padded with -1 / 0."""
    if w.shape[1] != edges * cpe or w.shape[0] % cpe:
        raise FGDCheckpointError("%s has shape %s, not [k * %d, %d]" % (key, tuple(w.shape), cpe, edges * cpe))
    e_out = w.shape[0] // cpe
    blocks = w.reshape(e_out, cpe, edges, cpe)
    eye = np.eye(cpe)
    pairs = []
    for i in range(e_out):
        srcs = [j for j in range(edges) if np.any(blocks[i, :, j])]
        if not srcs or any(not np.array_equal(blocks[i, :, j], blocks[i, 0, j, 0] * eye) for j in range(edges)):
            raise FGDCheckpointError("%s: output edge %d is not a per-channel mean of input edges" % (key, i))
        if any(blocks[i, 0, j, 0] != np.float32(1.0 / len(srcs)) for j in srcs):
            raise FGDCheckpointError("%s: output edge %d does not average its %d input edges" % (key, i, len(srcs)))
        pairs.append(srcs)
    used = sorted(j for s in pairs for j in s)
    if used != list(range(edges)):
        raise FGDCheckpointError("%s does not use every input edge exactly once" % key)
    k = max(len(s) for s in pairs)
    src = np.full((e_out * cpe, k), -1, np.int32)
    wt = np.zeros((e_out * cpe, k), np.float32)
    for i, s in enumerate(pairs):
        for q, j in enumerate(s):
            src[i * cpe:(i + 1) * cpe, q] = j * cpe + np.arange(cpe)
            wt[i * cpe:(i + 1) * cpe, q] = w[i * cpe, j * cpe]
    return src, wt, e_out


def pack_encoder(state):
    """Validate a VAESKConv state dict (encoder.* keys; decoder / fc_* are ignored) and pack every layer: per output channel the
    input channels its mask keeps, with the 4 residual taps and the shortcut weight (a gathered, block-sparse layout).  Returns
    a list of per-layer dicts of numpy arrays and sizes."""
    sd = _load_state(state)
    layers, c_in, edges = [], SIX_D, N_JOINTS
    for i in range(N_LAYERS):
        p = "encoder.layers.%d.0." % i
        c_out = _shape_of(sd, p + "residual.0.weight", 3)[0]
        if c_out % edges or c_out % GROUPS:
            raise FGDCheckpointError("%sresidual.0.weight: %d output channels do not split into %d edges and %d groups"
                                     % (p, c_out, edges, GROUPS))
        cpe_in, cpe_out = c_in // edges, c_out // edges
        w = _get(sd, p + "residual.0.weight", (c_out, c_in, 4))
        m = _check_mask(p + "residual.0.mask", _get(sd, p + "residual.0.mask", (c_out, c_in, 4)), edges, cpe_in, cpe_out)
        ws = _get(sd, p + "shortcut.weight", (c_out, c_in, 1))
        ms = _check_mask(p + "shortcut.mask", _get(sd, p + "shortcut.mask", (c_out, c_in, 1)), edges, cpe_in, cpe_out)
        if not np.array_equal(m, ms):
            raise FGDCheckpointError("%sshortcut.mask differs from %sresidual.0.mask" % (p, p))
        L = dict(c_in=c_in, c_out=c_out, b_res=_get(sd, p + "residual.0.bias", (c_out,)),
                 gamma=_get(sd, p + "residual.1.weight", (c_out,)), beta=_get(sd, p + "residual.1.bias", (c_out,)),
                 b_sc=_get(sd, p + "shortcut.bias", (c_out,)), edges=edges, density=float(m.mean()))
        row_ptr = np.zeros(c_out + 1, np.int32)
        cols, wr, wsc = [], [], []
        for o in range(c_out):
            keep = np.nonzero(m[o])[0]
            cols.append(keep)
            wr.append(w[o, keep, :])
            wsc.append(ws[o, keep, 0])
            row_ptr[o + 1] = row_ptr[o] + len(keep)
        L.update(row_ptr=row_ptr, col=np.concatenate(cols).astype(np.int32), w_res=np.concatenate(wr).astype(np.float32),
                 w_sc=np.concatenate(wsc).astype(np.float32))
        if p + "common.0.weight" in sd:
            pw = _get(sd, p + "common.0.weight", (_shape_of(sd, p + "common.0.weight", 2)[0], c_out))
            src, wt, e_next = _check_pool(p + "common.0.weight", pw, edges, cpe_out)
            L.update(pool_src=src, pool_w=wt, c_pool=src.shape[0])
        else:
            L.update(pool_src=None, pool_w=None, c_pool=c_out)
            e_next = edges
        layers.append(L)
        c_in, edges = L["c_pool"], e_next
    if c_in != LATENT_DIM:
        raise FGDCheckpointError("encoder.layers.%d.0 ends with %d channels, expected vae_length = %d" % (N_LAYERS - 1, c_in, LATENT_DIM))
    return layers


class FGDEncoder:
    """VAESKConv.map2latent on the device (one rg_fgd_encoder_layer launch per layer for the whole batch of clips)."""

    def __init__(self, state_dict_or_path, device=None):
        self.layers_host = pack_encoder(state_dict_or_path)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else torch.device(device).index or 0) \
            if torch.cuda.is_available() else None
        if self.device is None:
            raise capi.RgError("no GPU visible: FGDEncoder runs on the device (there is no CPU fallback)")
        self.h = capi.get_handle(self.device.index)
        dev = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(self.device, dt).contiguous()
        self.layers = []
        for L in self.layers_host:
            self.layers.append(dict(L, **{k: dev(L[k], torch.int32) for k in ("row_ptr", "col", "pool_src")},
                                    **{k: dev(L[k], torch.float32) for k in ("w_res", "w_sc", "b_res", "b_sc", "gamma", "beta", "pool_w")}))

    _clips = staticmethod(clip_list)

    def latents(self, poses):
        """poses: [B, n, 165] axis-angle (device or host), or a list of [n_i, 165] clips, every n_i a positive multiple of 16.
        -> [sum n_i / 16, 240] fp32 device tensor, clip after clip."""
        clips = self._clips(poses)
        if not clips:
            raise ValueError("no clips")
        lens = [int(c.shape[0]) for c in clips]
        for i, n in enumerate(lens):
            if n < TIME_STRIDE or n % TIME_STRIDE:
                raise ValueError("clip %d has %d frames: the encoder needs a positive multiple of %d" % (i, n, TIME_STRIDE))
        off = np.zeros(len(clips) + 1, np.int32)
        off[1:] = np.cumsum(lens)
        if off[-1] >= 2 ** 31 // SIX_D:
            raise ValueError("too many frames in one call (%d)" % off[-1])
        dev = self.device
        aa = torch.cat([torch.as_tensor(c).to(dev, torch.float32) for c in clips], 0).contiguous()
        total = int(off[-1])
        x = torch.empty(total, SIX_D, device=dev, dtype=torch.float32)
        self.h.call("aa_to_6d", aa, IN_DIM, x, SIX_D, 0, total, N_JOINTS)       # straight into the layer-0 input
        off_host = np.ascontiguousarray(off)
        off_dev = torch.from_numpy(off_host).to(dev)
        rows = total // 2
        r = torch.empty(rows * max(L["c_out"] for L in self.layers), device=dev, dtype=torch.float32)
        s = torch.empty_like(r)
        for i, L in enumerate(self.layers):
            y = torch.empty(rows, L["c_pool"], device=dev, dtype=torch.float32)
            ptr = lambda t: None if t is None else t.data_ptr()
            a = FgdLayerArgs(x=x.data_ptr(), y=y.data_ptr(), r=r.data_ptr(), s=s.data_ptr(), clip_off=off_dev.data_ptr(),
                             clip_off_host=off_host.ctypes.data, row_ptr=L["row_ptr"].data_ptr(), col=L["col"].data_ptr(),
                             w_res=L["w_res"].data_ptr(), w_sc=L["w_sc"].data_ptr(), b_res=L["b_res"].data_ptr(),
                             b_sc=L["b_sc"].data_ptr(), gamma=L["gamma"].data_ptr(), beta=L["beta"].data_ptr(),
                             pool_src=ptr(L["pool_src"]), pool_w=ptr(L["pool_w"]), n_clips=len(clips), layer=i,
                             c_in=L["c_in"], c_out=L["c_out"], c_pool=L["c_pool"],
                             pool_k=0 if L["pool_src"] is None else L["pool_src"].shape[1], groups=GROUPS, eps=GN_EPS)
            self.h.call("fgd_encoder_layer", ctypes.byref(a))
            x, rows = y, rows // 2
        return x


# ---------------------------------------------------------------------------------------------------- statistics and distance
def latent_statistics(lat):
    """(mean [240], covariance [240, 240]) in float64 (np.mean / np.cov(rowvar=False), metric.py:253-256).  Device tensors
    go through rg_latent_moments (fp64 accumulation, two passes); host arrays through numpy float64."""
    if torch.is_tensor(lat) and lat.is_cuda:
        lat = lat.to(torch.float32).contiguous()
        if lat.ndim != 2 or lat.shape[0] < 2:
            raise ValueError("need a [N >= 2, d] latent matrix, got %s" % (tuple(lat.shape),))
        n, d = lat.shape
        mu = torch.empty(d, device=lat.device, dtype=torch.float64)
        cov = torch.empty(d, d, device=lat.device, dtype=torch.float64)
        capi.get_handle(lat.device.index).call("latent_moments", lat, n, d, mu, cov)
        return mu.cpu().numpy(), cov.cpu().numpy()
    a = lat.detach().cpu().numpy() if torch.is_tensor(lat) else np.asarray(lat)
    a = a.astype(np.float64)
    if a.ndim != 2 or a.shape[0] < 2:
        raise ValueError("need a [N >= 2, d] latent matrix, got %s" % (a.shape,))
    mu = a.mean(axis=0)
    c = a - mu
    return mu, (c.T @ c) / (a.shape[0] - 1)


def _sqrt_psd(s):
    w, v = np.linalg.eigh((s + s.T) * 0.5)
    return (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T


def frechet_distance_from_statistics(mu1, sigma1, mu2, sigma2):
    """||mu1 - mu2||^2 + tr S1 + tr S2 - 2 tr sqrtm(S1 S2) (metric.py:266-321), float64.  tr sqrtm(S1 S2) = sum sqrt(eig(A S2 A)),
    A = S1^(1/2) (S1 S2 is similar to A S2 A, which is symmetric PSD)."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, np.float64)), np.atleast_1d(np.asarray(mu2, np.float64))
    s1, s2 = np.atleast_2d(np.asarray(sigma1, np.float64)), np.atleast_2d(np.asarray(sigma2, np.float64))
    if mu1.shape != mu2.shape or s1.shape != s2.shape or s1.shape != (mu1.shape[0],) * 2:
        raise ValueError("mean / covariance shapes do not match: %s %s %s %s" % (mu1.shape, s1.shape, mu2.shape, s2.shape))
    a = _sqrt_psd(s1)
    m = a @ s2 @ a
    tr_covmean = np.sqrt(np.clip(np.linalg.eigvalsh((m + m.T) * 0.5), 0.0, None)).sum()
    diff = mu1 - mu2
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2.0 * tr_covmean)


def frechet_distance(lat_a, lat_b):
    """metric.py:252-260 FIDCalculator.frechet_distance on two [N, d] latent sets (device tensors or host arrays)."""
    return frechet_distance_from_statistics(*latent_statistics(lat_a), *latent_statistics(lat_b))


# ---------------------------------------------------------------------------------------------------- accumulation
def _trim(n, eval_n, window):
    n = min(n, eval_n)          # evaluate.py:231-232
    return n - n % window       # :267


class FGDEvaluator:
    """Accumulates prediction / ground-truth latents clip by clip (evaluate.py:169-275) and computes FGD (:436)."""

    def __init__(self, encoder, eval_n=EVAL_N, window=WINDOW):
        if window < TIME_STRIDE or window % TIME_STRIDE:
            raise ValueError("window must be a positive multiple of %d" % TIME_STRIDE)
        self.encoder, self.eval_n, self.window = encoder, int(eval_n), int(window)
        self.reset()

    def reset(self):
        self.pred_latents, self.gt_latents, self.clips, self.frames = [], [], 0, 0

    def add(self, pred_poses, gt_poses, names=None):
        """pred_poses / gt_poses: [B, n, 165] tensors (device or host) or lists of [n_i, 165] clips.  Each clip is truncated to
        eval_n frames and trimmed to a multiple of `window`; its ground truth to the prediction's length."""
        enc = self.encoder
        pred, gt = enc._clips(pred_poses), enc._clips(gt_poses)
        if len(pred) != len(gt):
            raise ValueError("%d predicted clips but %d ground-truth clips" % (len(pred), len(gt)))
        ps, gs = [], []
        for i, (p, g) in enumerate(zip(pred, gt)):
            name = names[i] if names is not None else "clip %d" % (self.clips + i)
            n = min(int(p.shape[0]), self.eval_n)
            if int(g.shape[0]) < n:
                raise ValueError("%s: ground truth has %d frames, the prediction %d" % (name, g.shape[0], n))
            m = _trim(n, self.eval_n, self.window)
            if m < self.window:
                raise ValueError("%s: %d frames after truncation, fewer than %d" % (name, n, self.window))
            ps.append(p[:m])
            gs.append(g[:m])
        lat = enc.latents(ps + gs)           # prediction and ground truth in one launch per layer
        k = sum(int(p.shape[0]) for p in ps) // TIME_STRIDE
        self.pred_latents.append(lat[:k])
        self.gt_latents.append(lat[k:])
        self.clips += len(ps)
        self.frames += sum(int(p.shape[0]) for p in ps)

    def latents(self):
        return torch.cat(self.pred_latents, 0), torch.cat(self.gt_latents, 0)

    def compute(self):
        if not self.pred_latents:
            raise ValueError("no clips added")
        return frechet_distance(*self.latents())


# ---------------------------------------------------------------------------------------------------- SMPL-X joint metrics
UPPER_BODY_JOINTS = (3, 6, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21)      # evaluate.py:107, :132
HAND_JOINTS = tuple(range(25, 55))                                           # evaluate.py:106
ALIGN_MASK = 10                  # evaluate.py:134: frames left out at both ends of a clip
ALIGN_SIGMA = 0.3                # metric.alignment(0.3, 7, ...) (evaluate.py:128-133)
BEAT_ORDER = 7
BEAT_THRESHOLD = 0.3             # metric.py:62
POSE_FPS = 30
AUDIO_SR = 16000
SRGR_THRESHOLD = 0.3             # metric.SRGR(threshold=0.3, joints=55) (evaluate.py:143)
SRGR_SCALE = 0.165               # metric.py:44-45: "srgr == 0.165 when all success, scale range to [0, 1]"
MOTION_FPS = 15                  # the rate of sem_score in the reference's test config (motion_fps)

JointStatsArgs = capi.struct("rg_joint_stats_args")
PairDistArgs = capi.struct("rg_pair_dist_args")
SrgrArgs = capi.struct("rg_srgr_args")


def pair_distance_sums(x, group_off):
    """rg_pair_distance_sums: x [N, D] fp32 device tensor, group_off [n_groups + 1] row offsets -> [n_groups] float64 (host):
    per group the sum over pairs i < j of ||x_i - x_j||."""
    x = x.reshape(x.shape[0], -1).to(torch.float32).contiguous()
    off = np.ascontiguousarray(group_off, np.int32)
    if off.ndim != 1 or off.shape[0] < 2 or off[0] != 0 or off[-1] != x.shape[0] or np.any(np.diff(off) < 0):
        raise ValueError("group_off must rise from 0 to %d" % x.shape[0])
    tiles = max(1, -(-int(np.diff(off).max()) // 32))
    n_groups = off.shape[0] - 1
    dev = x.device
    partial = torch.empty(n_groups * tiles * tiles, device=dev, dtype=torch.float64)
    out = torch.empty(n_groups, device=dev, dtype=torch.float64)
    off_dev = torch.from_numpy(off).to(dev)
    a = PairDistArgs(x=x.data_ptr(), group_off=off_dev.data_ptr(), group_off_host=off.ctypes.data, partial=partial.data_ptr(),
                     out=out.data_ptr(), partial_len=partial.numel(), n_groups=n_groups, dim=x.shape[1])
    capi.get_handle(dev.index).call("pair_distance_sums", ctypes.byref(a))
    return out.cpu().numpy()


def joint_clip_stats(joints, lens, mmae=None, retrieval=None):
    """rg_joint_clip_stats over joints [sum lens, 55, 3] (device), clip after clip.  mmae: [55] float64 device tensor or None
    (no beats); retrieval: None or (retr_joints, retr_poses, retr_off [n_clips] int32 host, joint_mask [55] uint8 device).
    -> (L1 partial sums [n_clips] float64 host, beat flags [sum lens, 55] uint8 device or None, MPJPE sums [n_clips] or None)."""
    dev = joints.device
    n_clips = len(lens)
    off = offsets(lens)
    off_dev = torch.from_numpy(off).to(dev)
    l1 = torch.empty(n_clips, device=dev, dtype=torch.float64)
    beats = torch.empty(int(off[-1]), N_JOINTS, device=dev, dtype=torch.uint8) if mmae is not None else None
    mp = ro_dev = None
    if retrieval is not None:
        mp = torch.empty(n_clips, device=dev, dtype=torch.float64)
        ro_dev = torch.from_numpy(np.ascontiguousarray(retrieval[2], np.int32)).to(dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    a = JointStatsArgs(joints=joints.data_ptr(), clip_off=off_dev.data_ptr(), clip_off_host=off.ctypes.data, l1_sum=l1.data_ptr(),
                       beats=ptr(beats), mmae=ptr(mmae), retr_joints=ptr(retrieval and retrieval[0]),
                       retr_poses=ptr(retrieval and retrieval[1]), retr_off=ptr(ro_dev), joint_mask=ptr(retrieval and retrieval[3]),
                       mpjpe_sum=ptr(mp), n_clips=n_clips, t_margin=ALIGN_MASK, order=BEAT_ORDER, dt=1.0 / POSE_FPS,
                       dt2=2.0 / POSE_FPS, threshold=BEAT_THRESHOLD)
    capi.get_handle(dev.index).call("joint_clip_stats", ctypes.byref(a))
    return l1.cpu().numpy(), beats, None if mp is None else mp.cpu().numpy()


def sem_at_pose_rate(sem, motion_fps, pose_fps=POSE_FPS):
    """evaluate.py:416-423: a clip's sem_score [m] at motion_fps -> float32 [floor(m * pose_fps / motion_fps)] at pose_fps, as
    F.interpolate(scale_factor=pose_fps / motion_fps, mode='linear') (align_corners=False) resamples it: output i reads the
    source position (i + 0.5) motion_fps / pose_fps - 0.5, clamped at 0, and blends its two neighbours, the upper one clamped at
    m - 1.  The blend is taken in float64 and rounded once.  Equal rates return the vector unchanged."""
    x = np.asarray(sem, np.float32)
    if x.ndim != 1:
        raise ValueError("sem must be a 1-D vector, got shape %s" % (x.shape,))
    motion_fps, pose_fps = int(motion_fps), int(pose_fps)
    if motion_fps < 1 or pose_fps % motion_fps:
        raise ValueError("pose_fps %d must be a multiple of motion_fps %d" % (pose_fps, motion_fps))
    if motion_fps == pose_fps or x.shape[0] == 0:
        return x
    m = x.shape[0]
    src = np.maximum((np.arange(m * pose_fps // motion_fps, dtype=np.float64) + 0.5) * motion_fps / pose_fps - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), m - 1)
    i1 = np.minimum(i0 + 1, m - 1)
    lam = src - i0
    return ((1.0 - lam) * x[i0].astype(np.float64) + lam * x[i1].astype(np.float64)).astype(np.float32)


def srgr_clip_sums(pred_joints, gt_joints, lens, weights, threshold=SRGR_THRESHOLD, n_joints=N_JOINTS):
    """rg_srgr_clip_sums over pred_joints / gt_joints [sum lens, n_joints, 3] (device), clip after clip, and weights [sum lens]
    (device or host, the sem score of every frame).  -> (sum over the joint-frames with |dx| + |dy| + |dz| < threshold of
    their frame's weight [n_clips] float64, the number of those joint-frames [n_clips] int64), both on the host."""
    dev = pred_joints.device
    n_clips = len(lens)
    off = offsets(lens)
    total = int(off[-1])
    if int(n_joints) < 1:
        raise ValueError("n_joints must be at least 1, got %d" % n_joints)
    if total >= 2 ** 31 // (3 * int(n_joints)):
        raise ValueError("too many frames in one call (%d)" % total)
    p = pred_joints.to(torch.float32).contiguous()
    g = gt_joints.to(dev, torch.float32).contiguous()
    w = torch.as_tensor(weights).to(dev, torch.float32).contiguous()
    if p.numel() != total * n_joints * 3 or g.numel() != p.numel() or w.numel() != total:
        raise ValueError("joints must hold %d x %d x 3 values and weights %d, got %d, %d and %d"
                         % (total, n_joints, total, p.numel(), g.numel(), w.numel()))
    off_dev = torch.from_numpy(off).to(dev)
    wsum = torch.empty(n_clips, device=dev, dtype=torch.float64)
    count = torch.empty(n_clips, device=dev, dtype=torch.int64)
    a = SrgrArgs(pred=p.data_ptr(), gt=g.data_ptr(), weights=w.data_ptr(), clip_off=off_dev.data_ptr(),
                 clip_off_host=off.ctypes.data, wsum=wsum.data_ptr(), count=count.data_ptr(), n_clips=n_clips,
                 n_joints=int(n_joints), threshold=float(threshold))
    capi.get_handle(dev.index).call("srgr_clip_sums", ctypes.byref(a))
    return wsum.cpu().numpy(), count.cpu().numpy()


def beat_lists(beats, lens, joints=UPPER_BODY_JOINTS):
    """Beat flags [sum lens, 55] (device or host) -> per clip {joint: window-relative beat frames} (alignment.load_pose)."""
    b = (beats.cpu().numpy() if torch.is_tensor(beats) else np.asarray(beats))[:, list(joints)]
    off = offsets(lens)
    return [{j: np.nonzero(b[off[c]:off[c + 1], q])[0] - ALIGN_MASK for q, j in enumerate(joints)} for c in range(len(lens))]


def gahr(a, b, sigma=ALIGN_SIGMA):
    """metric.py:206-217: mean over b of exp(-min_a |a - b|^2 / (2 sigma^2)), float64 (the reference's loop order)."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    l2_min = np.abs(a[None, :] - b[:, None]).min(axis=1) if a.size else np.full(b.shape[0], math.inf)    # (min is exact)
    total = 0
    for v in l2_min.tolist():
        total += math.exp(-(v ** 2) / (2 * sigma ** 2))
    return total / len(b)


def calculate_align(onsets, beat_lists, pose_fps=POSE_FPS, upper_body=UPPER_BODY_JOINTS, sigma=ALIGN_SIGMA):
    """metric.py:229-243: beat_lists[j] = window-relative beat frames of joint j (every joint, or a mapping joint -> list)."""
    vals = [gahr(np.asarray(beat_lists[j]) / pose_fps + 0, onsets, sigma) for j in upper_body]
    return sum(vals) / len(vals)


class JointMetrics:
    """L1div, diversity, beat alignment, MPJPE and SRGR of evaluate.py:286-464 over clips added batch by batch."""

    def __init__(self, smplx, avg_vel=None, eval_n=EVAL_N):
        self.smplx, self.eval_n = smplx, int(eval_n)
        self.mmae = None
        if avg_vel is not None:
            v = np.load(avg_vel) if isinstance(avg_vel, (str, os.PathLike)) else np.asarray(avg_vel)
            v = np.asarray(v, np.float64).reshape(-1)
            if v.shape[0] != N_JOINTS or not np.all(v > 0):
                raise ValueError("avg_vel must hold %d positive values, got shape %s" % (N_JOINTS, v.shape))
            self.mmae = torch.from_numpy(v).to(smplx.device)
        mask = np.zeros(N_JOINTS, np.uint8)
        mask[list(UPPER_BODY_JOINTS) + list(HAND_JOINTS)] = 1
        self.joint_mask = torch.from_numpy(mask).to(smplx.device)
        self.reset()

    def reset(self):
        self.l1 = [0.0, 0.0]
        self.frames = 0
        self.clips = 0
        self.align = [0.0, 0.0]
        self.align_clips, self.align_frames = 0, 0
        self.mpjpe_err, self.mpjpe_joints = 0.0, 0
        self.srgr_sum, self.srgr_clips = 0.0, 0
        self.pred_joints, self.gt_joints, self.lengths = [], [], []

    def add(self, pred_poses, gt_poses, betas=None, onsets=None, retrieval=None, names=None, sem_scores=None,
            motion_fps=MOTION_FPS):
        """pred_poses / gt_poses: [B, n, 165] or lists of [n_i, 165] axis-angle clips; betas: the ground truth's [300] per clip
        (evaluate.py:226, used for prediction, ground truth and retrieval) or None; onsets: per clip a 1-D array of onset
        times in seconds relative to sample a_offset (alignment.load_audio), or None; retrieval: per clip [>= n, 165] poses of
        the retrieved exemplar, or None; sem_scores: per clip the 1-D sem_score at motion_fps (SRGR, evaluate.py:413-426), which
        must cover the clip's evaluated frames once it is resampled to 30 fps (the reference raises an IndexError there)."""
        sm = self.smplx
        pred, gt = clip_list(pred_poses), clip_list(gt_poses)
        if len(pred) != len(gt):
            raise ValueError("%d predicted clips but %d ground-truth clips" % (len(pred), len(gt)))
        C = len(pred)
        for what, v in (("betas", betas), ("onsets", onsets), ("retrieval", retrieval), ("names", names),
                        ("sem_scores", sem_scores)):
            if v is not None and len(v) != C:
                raise ValueError("%d %s for %d clips" % (len(v), what, C))
        name = lambda i: names[i] if names is not None else "clip %d" % (self.clips + i)
        if C and self.clips and (sem_scores is not None) != (self.srgr_clips > 0):
            raise ValueError("%s: sem scores were given for %d of the %d clips before it: give them for every clip or for none"
                             % (name(0), self.srgr_clips, self.clips))
        ps, gs, rs, ws = [], [], [], []
        for i, (p, g) in enumerate(zip(pred, gt)):
            n = min(int(p.shape[0]), self.eval_n)
            if int(g.shape[0]) < n:
                raise ValueError("%s: ground truth has %d frames, the prediction %d" % (name(i), g.shape[0], n))
            if n < 2:
                raise ValueError("%s: %d frames, need at least 2" % (name(i), n))
            if onsets is not None:
                if n <= 2 * ALIGN_MASK:
                    raise ValueError("%s: %d frames, beat alignment needs more than %d" % (name(i), n, 2 * ALIGN_MASK))
                if len(onsets[i]) == 0:
                    raise ValueError("%s: no audio onsets (the reference divides by their count)" % name(i))
            r = None if retrieval is None else retrieval[i]
            if r is not None and int(r.shape[0]) < n:
                raise ValueError("%s: retrieval has %d frames, the prediction %d" % (name(i), r.shape[0], n))
            if sem_scores is not None:
                if sem_scores[i] is None:
                    raise ValueError("%s: no sem scores (they were given for other clips)" % name(i))
                w = sem_at_pose_rate(np.asarray(sem_scores[i]).reshape(-1), motion_fps, POSE_FPS)
                if w.shape[0] < n:
                    raise ValueError("%s: the sem scores cover %d frames at %d fps, the clip has %d"
                                     % (name(i), w.shape[0], POSE_FPS, n))
                ws.append(w[:n])
            ps.append(p[:n])
            gs.append(g[:n])
            rs.append(None if r is None else r[:n])
        if onsets is not None and self.mmae is None:
            raise ValueError("beat alignment needs avg_vel")
        lens = [int(p.shape[0]) for p in ps]
        b = None if betas is None else list(betas)
        joints = sm.joints(ps + gs, None if b is None else b + b, fold=True)       # evaluate.py:261-311
        n_pg = 2 * C
        ret_idx = [i for i in range(C) if rs[i] is not None]
        retr_off = np.full(n_pg, -1, np.int32)
        if ret_idx:
            rlen = [lens[i] for i in ret_idx]
            roff = offsets(rlen)
            retr_off[ret_idx] = roff[:-1]
            rposes = torch.cat([torch.as_tensor(rs[i]).to(sm.device, torch.float32) for i in ret_idx], 0).contiguous()
            rjoints = sm.joints([rposes[roff[k]:roff[k + 1]] for k in range(len(ret_idx))],
                                None if b is None else [b[i] for i in ret_idx])                  # evaluate.py:313-326
        l1h, beats, mph = joint_clip_stats(joints, lens + lens, self.mmae if onsets is not None else None,
                                           (rjoints, rposes, retr_off, self.joint_mask) if ret_idx else None)
        off = offsets(lens + lens)
        self.l1[0] += float(l1h[:C].sum())
        self.l1[1] += float(l1h[C:].sum())
        if ret_idx:
            self.mpjpe_err += float(sum(mph[i] for i in ret_idx))
            self.mpjpe_joints += sum(lens[i] * N_JOINTS for i in ret_idx)
        F = int(off[C])
        self.pred_joints.append(joints[:F])
        self.gt_joints.append(joints[F:])
        if sem_scores is not None:                                                                 # evaluate.py:426, metric.py:41-48
            wsum, _ = srgr_clip_sums(joints[:F], joints[F:], lens, np.concatenate(ws))
            for i in range(C):
                rate = wsum[i] * (1 / SRGR_SCALE) / (lens[i] * N_JOINTS)
                self.srgr_sum += rate * lens[i]
            self.srgr_clips += C
        if beats is not None:
            lists = beat_lists(beats, lens + lens)
            for i in range(C):
                w = lens[i] - 2 * ALIGN_MASK                                                       # evaluate.py:409-410
                on = np.asarray(onsets[i], np.float64)
                self.align[0] += calculate_align(on, lists[i]) * w
                self.align[1] += calculate_align(on, lists[C + i]) * w
            self.align_clips += C
            self.align_frames += sum(lens)
        self.lengths += lens
        self.frames += sum(lens)
        self.clips += C

    def _diversity(self, parts):
        n = set(self.lengths)
        if len(n) != 1:
            raise ValueError("diversity needs clips of one length, got lengths %s" % sorted(n))
        if self.clips < 2:
            raise ValueError("diversity needs at least 2 clips, got %d" % self.clips)
        n = n.pop()
        C = self.clips
        x = torch.cat(parts, 0).reshape(C, n * IN_DIM)
        s = pair_distance_sums(x, [0, C])[0]
        return s / n / ((C * C - C) / 2)                   # metric.py:339-344

    def compute(self):
        """-> dict(l1div, gt_l1div, div, gt_div, align, gt_align, mpjpe); align / gt_align are None when no onsets were
        given, mpjpe when no clip had a retrieval.  With sem scores the dict also has srgr (metric.py:51-52 SRGR.avg)."""
        if not self.clips:
            raise ValueError("no clips added")
        out = dict(l1div=self.l1[0] / self.frames, gt_l1div=self.l1[1] / self.frames,
                   div=self._diversity(self.pred_joints), gt_div=self._diversity(self.gt_joints), align=None, gt_align=None,
                   mpjpe=None if self.mpjpe_joints == 0 else self.mpjpe_err / self.mpjpe_joints)
        if self.align_clips:
            if self.align_clips != self.clips:
                raise ValueError("onsets were given for %d of %d clips" % (self.align_clips, self.clips))
            den = self.align_frames - 2 * self.align_clips * ALIGN_MASK                          # evaluate.py:439-440
            out.update(align=self.align[0] / den, gt_align=self.align[1] / den)
        if self.srgr_clips:
            if self.srgr_clips != self.clips:
                raise ValueError("sem scores were given for %d of %d clips" % (self.srgr_clips, self.clips))
            out["srgr"] = self.srgr_sum / self.frames
        return out


def multimodality(smplx, groups, eval_n=EVAL_N, names=None, batch_groups=256):
    """evaluate_mm.py:87-187: groups = per clip a list of its repetitions' [n, 165] poses.  Root-normalised joints of zero
    betas (no 6D round trip), per group the mean pairwise distance / n (metric.calculate_avg_distance), averaged over the
    groups evaluated (evaluate_mm.py:186 divides by the count of all rep0 files, which differs under --speaker_specific)."""
    groups = [list(g) for g in groups]
    if not groups:
        raise ValueError("no groups")
    lens = []
    for i, g in enumerate(groups):
        name = names[i] if names is not None else "group %d" % i
        if len(g) < 2:
            raise ValueError("%s: %d samples, multimodality needs at least 2" % (name, len(g)))
        ns = {min(int(p.shape[0]), eval_n) for p in g}
        if len(ns) != 1:
            raise ValueError("%s: samples of different lengths %s" % (name, sorted(ns)))
        lens.append(ns.pop())
    by_len = collections.defaultdict(list)
    for i, n in enumerate(lens):
        by_len[n].append(i)
    mm = np.zeros(len(groups))
    for n, idx in sorted(by_len.items()):
        for b0 in range(0, len(idx), batch_groups):
            chunk = idx[b0:b0 + batch_groups]
            clips = [p[:n] for i in chunk for p in groups[i]]
            j = smplx.joints(clips, None, fold=False, root_norm=True)               # evaluate_mm.py:158-177
            goff = offsets([len(groups[i]) for i in chunk])
            s = pair_distance_sums(j.reshape(len(clips), n * IN_DIM), goff)
            for k, i in enumerate(chunk):
                r = len(groups[i])
                mm[i] = s[k] / n / ((r * r - r) / 2)
    return float(sum(mm) / len(groups))


def find_mm_groups(npz_folder, speaker_specific=None, reps=5):
    """evaluate_mm.py:95-125: every */*_rep0 directory, filtered by "_<speaker>_"; per directory the rep0..rep{reps-1}
    pred_motion.npz files that exist.  Sorted (glob order is not).  -> list of (rep0 directory, [files])."""
    dirs = sorted(glob.glob(os.path.join(npz_folder, "*", "*_rep0")))
    if speaker_specific is not None:
        dirs = [d for d in dirs if "_" + speaker_specific + "_" in d]
    out = []
    for d in dirs:
        files = [os.path.join(d[:-len("rep0")] + "rep%d" % k, "pred_motion.npz") for k in range(reps)]
        out.append((d, [f for f in files if os.path.exists(f)]))
    return out


def evaluate_mm_folder(npz_folder, smplx, eval_n=EVAL_N, speaker_specific=None):
    groups = find_mm_groups(npz_folder, speaker_specific)
    if not groups:
        raise ValueError("no */*_rep0 directories under %s" % npz_folder)
    poses = []
    for d, files in groups:
        g = []
        for f in files:
            with np.load(f) as z:
                g.append(np.asarray(z["poses"], np.float32)[:eval_n])
        poses.append(g)
    return dict(mm_all=multimodality(smplx, poses, eval_n, names=[d for d, _ in groups]), mm_groups=len(groups))


# ---------------------------------------------------------------------------------------------------- folders
def find_clip_files(npz_folder, speaker_specific=None):
    """evaluate.py:169, :178-189: every */*/pred_motion.npz, filtered by "_<speaker>_" in the path; sorted (glob order is not)."""
    files = sorted(glob.glob(os.path.join(npz_folder, "*", "*", "pred_motion.npz")))
    if speaker_specific is not None:
        files = [f for f in files if "_" + speaker_specific + "_" in f]
    return files


def load_clip_pair(pred_file, eval_n=EVAL_N):
    """The `poses` of pred_motion.npz and its gt_motion.npz, truncated to eval_n frames; ground truth to the prediction's n."""
    with np.load(pred_file) as f:
        pred = np.asarray(f["poses"], np.float32)[:eval_n]
    gt_file = os.path.join(os.path.dirname(pred_file), "gt_motion.npz")
    with np.load(gt_file) as f:
        gt = np.asarray(f["poses"], np.float32)[:eval_n]
    if pred.ndim != 2 or pred.shape[1] != IN_DIM or gt.ndim != 2 or gt.shape[1] != IN_DIM:
        raise ValueError("%s: poses must be [n, %d]" % (pred_file, IN_DIM))
    if gt.shape[0] < pred.shape[0]:
        raise ValueError("%s: ground truth has %d frames, the prediction %d" % (gt_file, gt.shape[0], pred.shape[0]))
    return pred, gt[:pred.shape[0]]


def load_clip_record(pred_file, eval_n=EVAL_N, retrieval=True):
    """One read of a clip directory for FGD and the joint metrics: dict(pred, gt) as load_clip_pair, betas (the ground truth's,
    evaluate.py:226) and retrieval (retrieval_0.npz `poses` truncated to eval_n, or None; evaluate.py:199-205)."""
    d = os.path.dirname(pred_file)
    with np.load(pred_file) as f:
        pred = np.asarray(f["poses"], np.float32)[:eval_n]
    gt_file = os.path.join(d, "gt_motion.npz")
    with np.load(gt_file) as f:
        gt = np.asarray(f["poses"], np.float32)[:eval_n]
        betas = np.asarray(f["betas"], np.float64).reshape(-1) if "betas" in f.files else None
    if pred.ndim != 2 or pred.shape[1] != IN_DIM or gt.ndim != 2 or gt.shape[1] != IN_DIM:
        raise ValueError("%s: poses must be [n, %d]" % (pred_file, IN_DIM))
    if gt.shape[0] < pred.shape[0]:
        raise ValueError("%s: ground truth has %d frames, the prediction %d" % (gt_file, gt.shape[0], pred.shape[0]))
    rec = dict(pred=pred, gt=gt[:pred.shape[0]], betas=betas, retrieval=None)
    r_file = os.path.join(d, "retrieval_0.npz")
    if retrieval and os.path.exists(r_file):
        with np.load(r_file) as f:
            rec["retrieval"] = np.asarray(f["poses"], np.float32)[:eval_n]
    return rec


def clip_key(pred_file):
    """evaluate.py:183: "<dir>/<dir>" of a clip, the key of an onsets mapping."""
    return "/".join(os.path.dirname(os.path.abspath(pred_file)).split(os.sep)[-2:])


def librosa_onsets(pred_file, n):
    """evaluate.py:208-209, :396-405 with librosa: onset times (s) of the clip's gt_audio.wav, resampled to 16 kHz, cut to the
    n frames and without align_mask frames at both ends, relative to that start."""
    import librosa
    audio, sr = librosa.load(os.path.join(os.path.dirname(pred_file), "gt_audio.wav"))
    audio = librosa.resample(audio, orig_sr=sr, target_sr=AUDIO_SR)
    audio = audio[:int(AUDIO_SR / POSE_FPS * n)]
    a_offset = int(ALIGN_MASK * (AUDIO_SR / POSE_FPS))
    return librosa.onset.onset_detect(y=audio[a_offset:len(audio) - a_offset], sr=AUDIO_SR, hop_length=512, units="time")


def device_onsets(detector=None, resampler=None):
    """A getter (pred_file, n) -> onset times backed by one audio.OnsetDetector: the clip's gt_audio.wav (16 kHz mono) with the
    cuts of librosa_onsets, detected on the device.  getter.batch(pred_files, ns) runs a whole list of clips through one call of
    the detector; getter.seconds adds up the time spent in it.  With resampler (an audio.Resampler) the files may have any
    rate, channel count and format audio.read_wav reads: a batch is resampled on the device in grouped launches first (counted in
    getter.seconds), then cut."""
    from . import audio
    det = audio.OnsetDetector() if detector is None else detector

    def batch(pred_files, ns):
        if resampler is None:
            waves = [audio.clip_audio(f, n) for f, n in zip(pred_files, ns)]
        else:                                         # (rate, channels, format, frames as stored) of every file
            stored = [audio.read_wav(os.path.join(os.path.dirname(f), "gt_audio.wav")) for f in pred_files]
        t0 = time.perf_counter()
        if resampler is not None:
            waves = [audio.cut_to_clip(w, n) for w, n in zip(resampler.run([(s[3], s[0]) for s in stored]), ns)]
        out = det.detect(waves)                       # (ends with the copy of the onset frames to the host)
        get.seconds += time.perf_counter() - t0
        return out

    def get(pred_file, n):
        return batch([pred_file], [n])[0]
    get.batch, get.detector, get.resampler, get.seconds = batch, det, resampler, 0.0
    return get


def onset_source(onsets, resample_audio=False):
    """-> (function (pred_file, n) -> onset times, None) or (None, reason why beat alignment is skipped).  onsets: a mapping
    "<dir>/<dir>" -> onset times, "device" (audio.OnsetDetector on every clip's gt_audio.wav; with resample_audio behind an
    audio.Resampler, else the files must be 16 kHz mono), or None (librosa if importable)."""
    if isinstance(onsets, str) and onsets == "device":
        if resample_audio:
            from . import audio
            return device_onsets(resampler=audio.Resampler()), None
        return device_onsets(), None
    if onsets is not None:
        def from_mapping(pred_file, n):
            k = clip_key(pred_file)
            if k not in onsets:
                raise ValueError("%s: no onsets for clip %s" % (pred_file, k))
            return np.asarray(onsets[k], np.float64).reshape(-1)
        return from_mapping, None
    try:
        import librosa  # noqa: F401
    except ImportError:
        return None, "no onsets given and librosa is not importable"
    return librosa_onsets, None


def sem_source(sem_scores):
    """sem_scores: a mapping "<dir>/<dir>" (clip_key) -> 1-D sem_score, or the path of an .npz with those keys
    -> function pred_file -> the clip's vector (a ValueError that names the clip when it has no entry)."""
    if isinstance(sem_scores, (str, os.PathLike)):
        with np.load(sem_scores) as f:
            sem_scores = {k: f[k] for k in f.files}

    def from_mapping(pred_file):
        k = clip_key(pred_file)
        if k not in sem_scores:
            raise ValueError("%s: no sem scores for clip %s" % (pred_file, k))
        return np.asarray(sem_scores[k], np.float32).reshape(-1)
    return from_mapping


def load_face_record(pred_file, n):
    """The `expressions` of pred_motion.npz and gt_motion.npz (first n rows) and the ground truth's betas (None if absent) for
    the face metrics (evaluate.py:220-226)."""
    out = []
    for f in (pred_file, os.path.join(os.path.dirname(pred_file), "gt_motion.npz")):
        with np.load(f) as z:
            if "expressions" not in z.files:
                raise ValueError("%s: no expressions (the face metrics need them)" % f)
            e = np.asarray(z["expressions"], np.float32)
            betas = np.asarray(z["betas"], np.float64).reshape(-1) if "betas" in z.files else None
        if e.ndim != 2 or e.shape[0] < n:
            raise ValueError("%s: expressions have shape %s, the clip has %d frames" % (f, e.shape, n))
        out.append(e[:n])
    return out[0], out[1], betas


def load_foot_record(pred_file, n):
    """The `trans` of pred_motion.npz and gt_motion.npz (first n rows) for the foot metrics."""
    out = []
    for f in (pred_file, os.path.join(os.path.dirname(pred_file), "gt_motion.npz")):
        with np.load(f) as z:
            if "trans" not in z.files:
                raise ValueError("%s: no trans (the foot metrics need the translation)" % f)
            t = np.asarray(z["trans"], np.float32)
        if t.ndim != 2 or t.shape[1] != 3 or t.shape[0] < n:
            raise ValueError("%s: trans has shape %s, the clip has %d frames" % (f, t.shape, n))
        out.append(t[:n])
    return out[0], out[1]


def evaluate_folder(npz_folder, encoder, eval_n=EVAL_N, speaker_specific=None, batch_clips=256, timings=None, smplx=None,
                    avg_vel=None, onsets=None, retrieval=True, mesh=None, sem_scores=None, motion_fps=MOTION_FPS,
                    onsets_out=None, resample_audio=False, foot=False):
    """FGD of a folder written by packing.save_sample_files (evaluate.py:169-275, :436) -> dict(fgd, clips, latents, frames).
    With smplx (an SMPLXJoints) the joint metrics of JointMetrics.compute are added (evaluate.py:286-464); beat alignment
    needs avg_vel and onsets (a mapping "<dir>/<dir>" -> onset times, or "device": audio.OnsetDetector on every clip's 16 kHz
    gt_audio.wav, one call per batch_clips clips; else librosa on gt_audio.wav; without any of them the result has
    `align_skipped` instead of align / gt_align).  resample_audio (with onsets="device"): gt_audio.wav may have any rate, channel
    count and PCM16 / PCM24 / PCM32 / float32 format; a chunk's files are brought to 16 kHz mono on the device (audio.Resampler)
    before the cuts.  onsets_out: an optional dict that receives the onset times used, by clip_key.
    retrieval: read retrieval_0.npz where present (mpjpe).
    With mesh (an SMPLXMesh) the face metrics l2 / lvel of FaceMetrics.compute are added (evaluate.py:328-367, :431-432); they
    read `expressions` from both files, and the ground truth's betas (zeros where absent).
    With sem_scores (a mapping "<dir>/<dir>" -> the clip's 1-D sem_score at motion_fps, or the path of an .npz of them; needs
    smplx) srgr is added (evaluate.py:413-426, :447-449); a clip without an entry is an error.
    With foot (needs smplx; this project's own) skate / slide / gt_skate / gt_slide of foot.FootMetrics are
    added: foot skating of the joints with the files' `trans` added, at POSE_FPS, truncated like the poses.  The files carry no
    contact flags, so the two flag metrics are available from Python only.
    timings: an optional dict that receives the seconds spent reading files ("read") and on the device ("device"); with
    onsets="device" also "onsets", the part of "device" spent detecting them."""
    files = find_clip_files(npz_folder, speaker_specific)
    if not files:
        raise ValueError("no */*/pred_motion.npz under %s" % npz_folder)
    if sem_scores is not None and smplx is None:
        raise ValueError("sem_scores need smplx (SRGR is computed on the SMPL-X joints)")
    if foot and smplx is None:
        raise ValueError("foot needs smplx (foot skating is measured on the SMPL-X joints)")
    ev = FGDEvaluator(encoder, eval_n=eval_n)
    jm = skipped = get_onsets = None
    get_sem = None if sem_scores is None else sem_source(sem_scores)
    if smplx is not None:
        jm = JointMetrics(smplx, avg_vel=avg_vel, eval_n=eval_n)
        get_onsets, skipped = onset_source(onsets, resample_audio) if avg_vel is not None else (None, "no avg_vel given")
    fm = None if mesh is None else FaceMetrics(mesh, eval_n=eval_n)
    ft = None
    if foot:
        from .foot import FootMetrics
        ft = FootMetrics(smplx, fps=POSE_FPS)
    t_read = t_dev = 0.0
    for b0 in range(0, len(files), batch_clips):
        chunk = files[b0:b0 + batch_clips]
        t0 = time.perf_counter()
        if jm is None:
            pairs = [load_clip_pair(f, eval_n) for f in chunk]
            recs = [dict(pred=p, gt=g) for p, g in pairs]
        else:
            recs = [load_clip_record(f, eval_n, retrieval) for f in chunk]
            if get_onsets is not None:
                ns = [r["pred"].shape[0] for r in recs]
                found = get_onsets.batch(chunk, ns) if hasattr(get_onsets, "batch") else [get_onsets(f, n) for f, n in zip(chunk, ns)]
                for f, r, on in zip(chunk, recs, found):
                    r["onsets"] = on
                    if onsets_out is not None:
                        onsets_out[clip_key(f)] = np.asarray(on, np.float64)
            if get_sem is not None:
                for f, r in zip(chunk, recs):
                    r["sem"] = get_sem(f)
        if fm is not None:
            for f, r in zip(chunk, recs):
                r["pred_exprs"], r["gt_exprs"], r["face_betas"] = load_face_record(f, r["pred"].shape[0])
        if ft is not None:
            for f, r in zip(chunk, recs):
                r["pred_trans"], r["gt_trans"] = load_foot_record(f, r["pred"].shape[0])
        t1 = time.perf_counter()
        ev.add([r["pred"] for r in recs], [r["gt"] for r in recs], names=chunk)
        if jm is not None:
            betas = [r["betas"] if r["betas"] is not None else np.zeros(N_BETAS) for r in recs]
            sem = dict(sem_scores=[r["sem"] for r in recs], motion_fps=motion_fps) if get_sem is not None else {}
            jm.add([r["pred"] for r in recs], [r["gt"] for r in recs], betas=betas,
                   onsets=[r["onsets"] for r in recs] if get_onsets is not None else None,
                   retrieval=[r["retrieval"] for r in recs], names=chunk, **sem)
        if fm is not None:
            fm.add([r["pred"] for r in recs], [r["gt"] for r in recs], [r["pred_exprs"] for r in recs],
                   [r["gt_exprs"] for r in recs], betas=[r["face_betas"] if r["face_betas"] is not None else np.zeros(N_BETAS)
                                                         for r in recs], names=chunk)
        if ft is not None:
            ft.add([r["pred"] for r in recs], [r["pred_trans"] for r in recs], [r["gt"] for r in recs],
                   [r["gt_trans"] for r in recs], betas=betas)
        torch.cuda.synchronize()
        t_read, t_dev = t_read + (t1 - t0), t_dev + (time.perf_counter() - t1)
    t_on = getattr(get_onsets, "seconds", None)
    if t_on is not None:                                  # detected inside the reading phase: counted with the device
        t_read, t_dev = t_read - t_on, t_dev + t_on
    t0 = time.perf_counter()
    fgd = ev.compute()
    out = dict(fgd=fgd, clips=ev.clips, latents=sum(int(x.shape[0]) for x in ev.pred_latents), frames=ev.frames)
    if jm is not None:
        out.update(jm.compute())
        if skipped is not None:
            del out["align"], out["gt_align"]
            out["align_skipped"] = skipped
    if fm is not None:
        out.update(fm.compute())
    if ft is not None:
        out.update(ft.compute())
    t_dev += time.perf_counter() - t0
    if timings is not None:
        timings.update(read=t_read, device=t_dev)
        if t_on is not None:
            timings["onsets"] = t_on
    return out


def build_parser():
    ap = argparse.ArgumentParser(description="FGD (and with --smplx_path the SMPL-X joint metrics) of a folder of generated clips: "
                                             "tools/evaluate.py; with --mm the multimodality of tools/evaluate_mm.py")
    ap.add_argument("npz_folder_path")
    ap.add_argument("--e_path", help="EMAGE VAESKConv checkpoint (AESKConv_240_100.bin); required unless --mm")
    ap.add_argument("--eval_n", type=int, default=EVAL_N)
    ap.add_argument("--speaker_specific", default=None)
    ap.add_argument("--smplx_path", default=None, help="SMPLX_NEUTRAL_2020.npz: adds l1div, div, align, mpjpe")
    ap.add_argument("--avg_vel_path", default=None, help="mean_vel_smplxflame_30.npy (beat alignment)")
    ap.add_argument("--onsets", default=None, help="'device': detect the onsets of every clip's 16 kHz mono gt_audio.wav on the "
                                                   "device; else an npz of onset times per clip, keyed <dir>/<dir> (instead of librosa)")
    ap.add_argument("--save_onsets", default=None, help="write the onset times used to this npz, keyed <dir>/<dir> (a later run can "
                                                        "pass it as --onsets)")
    ap.add_argument("--resample_audio", action="store_true", help="with --onsets device: gt_audio.wav of any rate, channel count and "
                                                                  "PCM16 / PCM24 / PCM32 / float32 format is resampled to 16 kHz mono on the device")
    ap.add_argument("--mm", action="store_true", help="multimodality over */*_rep0..4 (needs --smplx_path)")
    ap.add_argument("--face", action="store_true", help="adds the face metrics l2 and lvel (needs --smplx_path)")
    ap.add_argument("--sem_scores", default=None, help="npz of sem_score vectors per clip, keyed <dir>/<dir>: adds srgr "
                                                       "(needs --smplx_path)")
    ap.add_argument("--motion_fps", type=int, default=MOTION_FPS, help="frame rate of the sem_score vectors")
    ap.add_argument("--foot", action="store_true", help="adds the foot skating metrics skate, slide, gt_skate and gt_slide from "
                                                        "the files' poses and trans (needs --smplx_path)")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.face and args.smplx_path is None:
        ap.error("--face needs --smplx_path")
    if args.foot and (args.smplx_path is None or args.mm):
        ap.error("--foot needs --smplx_path (and does not go with --mm)")
    if args.sem_scores is not None and (args.smplx_path is None or args.mm):
        ap.error("--sem_scores needs --smplx_path (and does not go with --mm)")
    if args.mm:
        if args.smplx_path is None:
            ap.error("--mm needs --smplx_path")
        print(json.dumps(evaluate_mm_folder(args.npz_folder_path, SMPLXJoints(args.smplx_path), eval_n=args.eval_n,
                                            speaker_specific=args.speaker_specific)))
        return
    if args.e_path is None:
        ap.error("--e_path is required")
    enc = FGDEncoder(args.e_path)
    if args.smplx_path is None:
        print(json.dumps(evaluate_folder(args.npz_folder_path, enc, eval_n=args.eval_n, speaker_specific=args.speaker_specific)))
        return
    onsets = None
    if args.onsets == "device":
        onsets = "device"
    elif args.onsets is not None:
        with np.load(args.onsets) as f:
            onsets = {k: f[k] for k in f.files}
    used = {} if args.save_onsets is not None else None
    result = evaluate_folder(args.npz_folder_path, enc, eval_n=args.eval_n, speaker_specific=args.speaker_specific,
                             smplx=SMPLXJoints(args.smplx_path), avg_vel=args.avg_vel_path, onsets=onsets,
                             mesh=SMPLXMesh(args.smplx_path) if args.face else None, sem_scores=args.sem_scores,
                             motion_fps=args.motion_fps, onsets_out=used, resample_audio=args.resample_audio, foot=args.foot)
    if used is not None:
        with open(args.save_onsets, "wb") as f:           # (np.savez(path) would append .npz to another suffix)
            np.savez(f, **used)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
