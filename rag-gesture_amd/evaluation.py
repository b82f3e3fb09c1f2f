"""Fréchet gesture distance (FGD): the FGD half of the reference's tools/evaluate.py, on the device.

    aa [n, 165] --rg_aa_to_6d--> 6D [n, 330] --4 x rg_fgd_encoder_layer--> latents [n/16, 240]   (evaluate.py:255-275)
    latents --rg_latent_moments (fp64)--> mean, covariance --numpy float64 eigh--> FGD          (evaluate.py:436, metric.py:246-321)

The encoder is EMAGE's VAESKConv.map2latent (eval_models/model.py:12-107, :231-251) with the hyper-parameters evaluate.py:87-97
sets; its whole structure (block masks, pool matrices) is read from the checkpoint's state dict, so no SMPL-X file is needed.
`tr sqrtm(S1 S2)` is computed as the sum of sqrt(eigenvalues of A S2 A), A = S1^(1/2), both by numpy.linalg.eigh with negative
eigenvalues clipped to 0: it never yields the reference's imaginary-component ValueError (-> 1e10), the one deliberate
difference (DESIGN.md "FGD evaluation").
"""
import argparse
import collections
import ctypes
import glob
import json
import os
import time

import numpy as np
import torch

from . import capi

N_JOINTS = 55
IN_DIM = N_JOINTS * 3            # axis-angle channels of a pose row
SIX_D = N_JOINTS * 6             # the encoder's input (evaluate.py:262-264)
LATENT_DIM = 240                 # vae_length
N_LAYERS = 4                     # vae_layer
GROUPS = 10                      # skeleton.py:575 nn.GroupNorm(10, out_channels)
GN_EPS = 1e-5
TIME_STRIDE = 1 << N_LAYERS      # frames per latent row
WINDOW = 32                      # vae_test_len: evaluate.py trims every clip to a multiple of it
EVAL_N = 300

_vp = ctypes.c_void_p


class FgdLayerArgs(ctypes.Structure):
    """include/rg_gesture.h rg_fgd_layer_args."""
    _fields_ = [("x", _vp), ("y", _vp), ("r", _vp), ("s", _vp), ("clip_off", _vp), ("clip_off_host", _vp), ("row_ptr", _vp),
                ("col", _vp), ("w_res", _vp), ("w_sc", _vp), ("b_res", _vp), ("b_sc", _vp), ("gamma", _vp), ("beta", _vp),
                ("pool_src", _vp), ("pool_w", _vp), ("n_clips", ctypes.c_int), ("layer", ctypes.c_int), ("c_in", ctypes.c_int),
                ("c_out", ctypes.c_int), ("c_pool", ctypes.c_int), ("pool_k", ctypes.c_int), ("groups", ctypes.c_int),
                ("eps", ctypes.c_float)]


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

    @staticmethod
    def _clips(poses):
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


def evaluate_folder(npz_folder, encoder, eval_n=EVAL_N, speaker_specific=None, batch_clips=256, timings=None):
    """FGD of a folder written by packing.save_sample_files (evaluate.py:169-275, :436) -> dict(fgd, clips, latents, frames).
    timings: an optional dict that receives the seconds spent reading files ("read") and on the device ("device")."""
    files = find_clip_files(npz_folder, speaker_specific)
    if not files:
        raise ValueError("no */*/pred_motion.npz under %s" % npz_folder)
    ev = FGDEvaluator(encoder, eval_n=eval_n)
    t_read = t_dev = 0.0
    for b0 in range(0, len(files), batch_clips):
        chunk = files[b0:b0 + batch_clips]
        t0 = time.perf_counter()
        pairs = [load_clip_pair(f, eval_n) for f in chunk]
        t1 = time.perf_counter()
        ev.add([p for p, _ in pairs], [g for _, g in pairs], names=chunk)
        torch.cuda.synchronize()
        t_read, t_dev = t_read + (t1 - t0), t_dev + (time.perf_counter() - t1)
    t0 = time.perf_counter()
    fgd = ev.compute()
    t_dev += time.perf_counter() - t0
    if timings is not None:
        timings.update(read=t_read, device=t_dev)
    return dict(fgd=fgd, clips=ev.clips, latents=sum(int(x.shape[0]) for x in ev.pred_latents), frames=ev.frames)


def main(argv=None):
    ap = argparse.ArgumentParser(description="FGD of a folder of generated clips (the FGD half of tools/evaluate.py)")
    ap.add_argument("npz_folder_path")
    ap.add_argument("--e_path", required=True, help="EMAGE VAESKConv checkpoint (AESKConv_240_100.bin)")
    ap.add_argument("--eval_n", type=int, default=EVAL_N)
    ap.add_argument("--speaker_specific", default=None)
    args = ap.parse_args(argv)
    enc = FGDEncoder(args.e_path)
    print(json.dumps(evaluate_folder(args.npz_folder_path, enc, eval_n=args.eval_n, speaker_specific=args.speaker_specific)))


if __name__ == "__main__":
    main()
