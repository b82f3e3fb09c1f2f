"""Foot skating measured and contact feet planted on the device (csrc/rg_foot.hip).

This project's own: the reference neither scores foot sliding nor reads the four contact flags its lower-body VAE decodes
(`pred_contact`).  The skating ratio follows Guided Motion Diffusion with its thresholds made rate-free; the height
of a foot is taken above that joint's own lowest point in the clip, so no floor level is needed.

    skate_sums    rg_foot_skate_sums: per clip the RG_FOOT_SUMS counts and sums
    FootMetrics   skate, slide (and gt_*, contact_*) over clips added batch by batch
    FootPlanter   rg_foot_plant: the translation minus the accumulated horizontal slide of the flagged feet (no IK: the poses
                  stay; the path drifts horizontally by what the feet slid, which is accepted)

Flag contact[t, k] belongs to the pair (t, t + 1) of joint dataset.CONTACT_JOINTS[k], as dataset.ClipPreprocessor makes it; a
clip's last flag is not read.  No CPU path: without a GPU the classes raise capi.RgError.
"""
import numpy as np
import torch

from . import capi, packing
from .dataset import CONTACT_JOINTS, CONTACT_THRESHOLD
from .smplx import N_JOINTS, clip_list, offsets

FOOT_SUMS = capi.header_constants()["RG_FOOT_SUMS"]
HEIGHT = 0.05                    # m: Guided Motion Diffusion's foot height
SPEED = 0.5                      # m/s: its 2.5 cm per frame at 20 fps
CONTACT_FLAG = 0.5               # a decoded flag at or above this counts as set
N_FLAGS = len(CONTACT_JOINTS)


def _rows(xs):
    """[B, n, w] or [n, w] (tensor or array) or a list of [n_i, w] -> the list of clips' rows."""
    if torch.is_tensor(xs) or isinstance(xs, np.ndarray):
        return [xs[b] for b in range(xs.shape[0])] if xs.ndim == 3 else [xs]
    return list(xs)


def _cat(xs, lens, width, dev, what):
    """The clips' rows as one contiguous fp32 [sum lens, width] device tensor (each clip cut to its length)."""
    rows = _rows(xs)
    if len(rows) != len(lens):
        raise ValueError("%d %s for %d clips" % (len(rows), what, len(lens)))
    parts = []
    for i, (x, n) in enumerate(zip(rows, lens)):
        if x.ndim != 2 or x.shape[1] != width or int(x.shape[0]) < n:
            raise ValueError("%s of clip %d must be [>= %d, %d], got %s" % (what, i, n, width, tuple(x.shape)))
        parts.append(torch.as_tensor(x[:n]).to(dev, torch.float32))
    return torch.cat(parts, 0).contiguous()


def _tables(lens, dev):
    lens = [int(n) for n in lens]
    if not lens:
        raise ValueError("no clips")
    off = offsets(lens)
    return off, torch.from_numpy(off).to(dev)


def _check(t, shape, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape):
        raise capi.RgError("%s: contiguous fp32 device tensor %s expected" % (what, list(shape)))


def skate_sums(joints, lens, contact=None, fps=30., height=HEIGHT, speed=SPEED, contact_threshold=CONTACT_FLAG,
               move_threshold=CONTACT_THRESHOLD):
    """joints [F, 55, 3] fp32 device tensor (world positions, clip after clip), lens: the clips' frame counts, contact None or
    [F, 4] fp32 on the same device -> float64 [C, RG_FOOT_SUMS] on the host (include/rg_gesture.h: pairs, skating pairs, grounded
    joint-pairs, their summed horizontal speed, flagged joint-pairs, their summed displacement, the moving ones among them)."""
    if not (torch.is_tensor(joints) and joints.is_cuda):
        raise capi.RgError("device tensor expected (foot skating is measured on the device; there is no CPU path)")
    dev = joints.device
    off, off_dev = _tables(lens, dev)
    F = int(off[-1])
    _check(joints, (F, N_JOINTS, 3), "joints")
    if contact is not None:
        _check(contact, (F, N_FLAGS), "contact")
    sums = torch.empty(len(off) - 1, FOOT_SUMS, device=dev, dtype=torch.float64)
    capi.get_handle(dev.index).call("foot_skate_sums", joints, contact, off_dev, off.ctypes.data, len(off) - 1, float(fps),
                                    float(height), float(speed), float(contact_threshold), float(move_threshold), sums)
    return sums.cpu().numpy()


def plant_translation(joints, contact, transl, lens, contact_threshold=CONTACT_FLAG, out=None):
    """rg_foot_plant on concatenated clips: joints [F, 55, 3], contact [F, 4], transl [F, 3] (fp32 device tensors) -> the planted
    translation [F, 3] (out: where to write it; it may be transl itself)."""
    if not (torch.is_tensor(joints) and joints.is_cuda):
        raise capi.RgError("device tensor expected (feet are planted on the device; there is no CPU path)")
    dev = joints.device
    off, off_dev = _tables(lens, dev)
    F = int(off[-1])
    _check(joints, (F, N_JOINTS, 3), "joints")
    _check(contact, (F, N_FLAGS), "contact")
    _check(transl, (F, 3), "transl")
    if out is None:
        out = torch.empty_like(transl)
    _check(out, (F, 3), "out")
    capi.get_handle(dev.index).call("foot_plant", joints, contact, transl, off_dev, off.ctypes.data, len(off) - 1,
                                    float(contact_threshold), out)
    return out


def _ratio(num, den):
    return None if den == 0 else float(num / den)


class FootMetrics:
    """Foot skating over clips added batch by batch, from the SMPL-X joints with the translation added:
        skate           pairs of frames in which a grounded foot joint moves faster than `speed` / all pairs
        slide           mean horizontal speed (m/s) of the grounded joint-pairs
        gt_skate, gt_slide       the same of the ground truth, when it was added
        contact_slide   mean displacement (m per frame at the flags' rate) of the joint-pairs whose flag is set
        contact_moving  the share of those that move at least dataset.CONTACT_THRESHOLD (the rule that made the flags)
    the last two when flags were added.  A ratio without a denominator is None."""

    def __init__(self, smplx, fps=30., height=HEIGHT, speed=SPEED, contact_threshold=CONTACT_FLAG,
                 move_threshold=CONTACT_THRESHOLD):
        self.smplx = smplx
        self.device = capi.device_or_fail(getattr(smplx, "device", None), "FootMetrics")
        self.kw = dict(fps=float(fps), height=float(height), speed=float(speed), contact_threshold=float(contact_threshold),
                       move_threshold=float(move_threshold))
        self.reset()

    def reset(self):
        self.sums, self.gt_sums = np.zeros(FOOT_SUMS), np.zeros(FOOT_SUMS)
        self.clips, self.has_gt, self.has_contact = 0, False, False

    def _sums(self, poses, transl, betas, contact):
        clips = clip_list(poses)
        lens = [int(c.shape[0]) for c in clips]
        dev = self.device
        joints = self.smplx.joints(clips, betas=betas, transl=_cat(transl, lens, 3, dev, "transl"))
        flags = None if contact is None else _cat(contact, lens, N_FLAGS, dev, "contact")
        return skate_sums(joints, lens, flags, **self.kw)

    def add(self, pred_poses, pred_transl, gt_poses=None, gt_transl=None, betas=None, contact=None):
        """pred_poses: clips as smplx.clip_list takes them; pred_transl: their [n_i, 3] translations in the same layout; gt_poses /
        gt_transl: the ground truth's (both or neither); betas: None or one [<= 300] vector per clip (used for both); contact:
        None or the clips' [n_i, 4] flags, which belong to the prediction.  -> the predicted clips' [C, RG_FOOT_SUMS] sums."""
        if (gt_poses is None) != (gt_transl is None):
            raise ValueError("gt_poses and gt_transl go together")
        sums = self._sums(pred_poses, pred_transl, betas, contact)
        if gt_poses is not None:
            if len(clip_list(gt_poses)) != sums.shape[0]:
                raise ValueError("%d predicted clips but %d ground-truth clips" % (sums.shape[0], len(clip_list(gt_poses))))
            self.gt_sums += self._sums(gt_poses, gt_transl, betas, None).sum(0)
            self.has_gt = True
        self.sums += sums.sum(0)
        self.has_contact = self.has_contact or contact is not None
        self.clips += sums.shape[0]
        return sums

    def compute(self):
        if not self.clips:
            raise ValueError("no clips added")
        s, g = self.sums, self.gt_sums
        out = dict(skate=_ratio(s[1], s[0]), slide=_ratio(s[3], s[2]))
        if self.has_gt:
            out.update(gt_skate=_ratio(g[1], g[0]), gt_slide=_ratio(g[3], g[2]))
        if self.has_contact:
            out.update(contact_slide=_ratio(s[5], s[4]), contact_moving=_ratio(s[6], s[4]))
        return out


class FootPlanter:
    """Takes out of a clip's translation the horizontal slide of the feet whose contact flag is set (rg_foot_plant): over a pair
    with flagged joints the translation moves back by their mean x/z displacement, and that correction accumulates.  The poses
    and the height stay as they are (no IK), a clip without a set flag comes back bit for bit, and the path drifts horizontally
    away from the predicted one by exactly what was taken out.  Not offered by long-form synthesis yet."""

    def __init__(self, smplx, contact_threshold=CONTACT_FLAG):
        self.smplx, self.contact_threshold = smplx, float(contact_threshold)
        self.device = capi.device_or_fail(getattr(smplx, "device", None), "FootPlanter")

    def plant(self, poses, transl, contact, betas=None):
        """poses: clips as smplx.clip_list takes them; transl / contact: their [n_i, 3] / [n_i, 4] rows in the same layout; betas:
        None or one vector per clip -> the planted translation in the layout of transl ([B, n, 3], [n, 3] or a list of
        [n_i, 3]), fp32 on the device."""
        clips = clip_list(poses)
        lens = [int(c.shape[0]) for c in clips]
        dev = self.device
        tr = _cat(transl, lens, 3, dev, "transl")
        joints = self.smplx.joints(clips, betas=betas, transl=tr)
        out = plant_translation(joints, _cat(contact, lens, N_FLAGS, dev, "contact"), tr, lens, self.contact_threshold)
        if torch.is_tensor(transl) or isinstance(transl, np.ndarray):
            return out.reshape(tuple(transl.shape))
        return list(torch.split(out, lens, 0))

    def plant_outputs(self, output, betas=None):
        """The dict a forward returns -> its pred_transl [B, n, 3] planted by its pred_contact, at the motion rate (the poses are
        packing.scatter_parts of the four predicted parts)."""
        poses = packing.scatter_parts(output["pred_upper"], output["pred_lower"], output["pred_hands"], output["pred_facepose"])
        return self.plant(poses, output["pred_transl"], output["pred_contact"], betas=betas)
