"""Foot skating measured and contact feet planted on the device (csrc/rg_foot.hip).

This project's own: the reference neither scores foot sliding nor reads the four contact flags its lower-body VAE decodes
(`pred_contact`).  The skating ratio follows Guided Motion Diffusion with its thresholds made rate-free; the height
of a foot is taken above that joint's own lowest point in the clip, so no floor level is needed.

    skate_sums    rg_foot_skate_sums: per clip the RG_FOOT_SUMS counts and sums
    FootMetrics   skate, slide (and gt_*, contact_*) over clips added batch by batch
    FootPlanter   rg_foot_plant: the translation minus the accumulated horizontal slide of the flagged feet (no IK: the poses
                  stay; the path drifts horizontally by what the feet slid, which is accepted)
    FootLocker    rg_foot_lock_targets + rg_foot_lock_ik (csrc/rg_footlock.hip): the flagged ankles pinned to
                  one world position per contact by analytic leg IK; the translation stays, nothing drifts

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
LOCK_STATS = capi.header_constants()["RG_FOOT_LOCK_STATS"]
LOCK_BLEND = 3                   # frames over which a lock's offset fades to zero outside a contact
LOCK_STRETCH = 0.995             # the furthest a locked ankle goes from its hip, in leg lengths


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
    away from the predicted one by exactly what was taken out.  Planting stays out of long-form synthesis by design (windows of
    a drifting translation do not blend): use FootLocker there."""

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


# --------------------------------------------------------------------------------------------------------------- the foot lock
def lock_targets(joints, contact, lens, contact_threshold=CONTACT_FLAG, blend=LOCK_BLEND):
    """rg_foot_lock_targets on concatenated clips: joints [F, 55, 3] (world positions), contact [F, 4] (fp32 device tensors; the
    two ankle columns are read) -> (offsets [F, 2, 3] float64 device tensor: what takes each ankle to its run's anchor, blended
    to zero over `blend` frames outside the runs; stats float64 [C, RG_FOOT_LOCK_STATS] on the host: member ankle-frames, runs,
    ankle-frames with a non-zero offset, the sum and the maximum of |d| over the member ankle-frames)."""
    if not (torch.is_tensor(joints) and joints.is_cuda):
        raise capi.RgError("device tensor expected (feet are locked on the device; there is no CPU path)")
    dev = joints.device
    off, off_dev = _tables(lens, dev)
    F = int(off[-1])
    _check(joints, (F, N_JOINTS, 3), "joints")
    _check(contact, (F, N_FLAGS), "contact")
    offsets_ = torch.empty(F, 2, 3, device=dev, dtype=torch.float64)
    stats = torch.empty(len(off) - 1, LOCK_STATS, device=dev, dtype=torch.float64)
    capi.get_handle(dev.index).call("foot_lock_targets", joints, contact, off_dev, off.ctypes.data, len(off) - 1,
                                    float(contact_threshold), int(blend), offsets_, stats)
    return offsets_, stats.cpu().numpy()


def lock_poses(smplx, poses, transl, offsets_, lens, betas=None, stretch=LOCK_STRETCH, out=None):
    """rg_foot_lock_ik on concatenated clips: poses [F, 165], transl [F, 3] (fp32 device tensors), offsets_ [F, 2, 3] float64 as
    lock_targets gives them, smplx an SMPLXJoints (rest joints, tree, pose mean), betas None or one vector per clip -> (the locked
    poses [F, 165]: only the channels of joints 1, 2, 4, 5, 7, 8 of frames with a non-zero offset differ; out: where to write
    them, it may be poses itself; reach [F, 2] fp32: |target - hip| / leg length, 0 where nothing was solved)."""
    if not (torch.is_tensor(poses) and poses.is_cuda):
        raise capi.RgError("device tensor expected (feet are locked on the device; there is no CPU path)")
    dev = poses.device
    off, off_dev = _tables(lens, dev)
    F, C = int(off[-1]), len(off) - 1
    _check(poses, (F, N_JOINTS * 3), "poses")
    _check(transl, (F, 3), "transl")
    if not (torch.is_tensor(offsets_) and offsets_.is_cuda and offsets_.dtype == torch.float64 and offsets_.is_contiguous()
            and tuple(offsets_.shape) == (F, 2, 3)):
        raise capi.RgError("offsets: contiguous float64 device tensor %s expected" % [F, 2, 3])
    if betas is not None and len(betas) != C:
        raise ValueError("%d betas for %d clips" % (len(betas), C))
    if out is None:
        out = torch.empty_like(poses)
    _check(out, (F, N_JOINTS * 3), "out")
    if betas is None:                                              # one template for every clip: uploaded once per model
        rest0 = getattr(smplx, "_lock_rest_dev", None)
        if rest0 is None or rest0.device != dev:
            rest0 = smplx._lock_rest_dev = torch.from_numpy(smplx.rest_joints().astype(np.float32)).to(dev)
        rest_dev = rest0.expand(C, N_JOINTS, 3).contiguous()
    else:
        rest = np.stack([smplx.rest_joints(betas[i]) for i in range(C)])
        rest_dev = torch.from_numpy(rest.astype(np.float32)).to(dev)
    reach = torch.empty(F, 2, device=dev, dtype=torch.float32)
    capi.get_handle(dev.index).call("foot_lock_ik", poses, transl, rest_dev, smplx.pose_mean, smplx.parents_dev,
                                    smplx.parents.ctypes.data, off_dev, off.ctypes.data, C, offsets_, float(stretch), out, reach)
    return out, reach


class FootLocker:
    """Pins each ankle whose contact flag is set to one world position for the length of its contact and re-solves the leg (hip,
    knee and ankle rotations) analytically so that the ankle gets there (rg_foot_lock_targets + rg_foot_lock_ik; DESIGN section
    19).  The complement of FootPlanter: the translation -- the root path -- stays exactly as predicted and nothing drifts, so
    it also serves a whole long-form recording (longform.LongformSynthesizer.run(locker=)).  Only the 18 channels of joints 1,
    2, 4, 5, 7, 8 can change; a frame without an offset, and so a clip without a set ankle flag, comes back bit for bit.  The
    toe flags are not read.  A target further than `stretch` leg lengths from the hip is approached and not met
    (`last_report["unreachable"]` counts those)."""

    def __init__(self, smplx, contact_threshold=CONTACT_FLAG, blend=LOCK_BLEND, stretch=LOCK_STRETCH):
        self.smplx, self.contact_threshold, self.blend, self.stretch = smplx, float(contact_threshold), int(blend), float(stretch)
        self.device = capi.device_or_fail(getattr(smplx, "device", None), "FootLocker")
        self.last_report = None

    def lock(self, poses, transl, contact, betas=None):
        """poses: clips as smplx.clip_list takes them; transl / contact: their [n_i, 3] / [n_i, 4] rows in the same layout; betas:
        None or one vector per clip -> the locked poses in the layout of poses ([B, n, 165], [n, 165] or a list of [n_i, 165]),
        fp32 on the device.  last_report: dict(stats float64 [C, RG_FOOT_LOCK_STATS], unreachable: the number of (frame, leg)
        with reach > stretch, max_reach)."""
        clips = clip_list(poses)
        lens = [int(c.shape[0]) for c in clips]
        dev = self.device
        aa = _cat(clips, lens, N_JOINTS * 3, dev, "poses")
        tr = _cat(transl, lens, 3, dev, "transl")
        joints = self.smplx.joints(clips, betas=betas, transl=tr)
        offsets_, stats = lock_targets(joints, _cat(contact, lens, N_FLAGS, dev, "contact"), lens, self.contact_threshold, self.blend)
        out, reach = lock_poses(self.smplx, aa, tr, offsets_, lens, betas=betas, stretch=self.stretch)
        r = reach.cpu().numpy()
        self.last_report = dict(stats=stats, unreachable=int((r > np.float32(self.stretch)).sum()), max_reach=float(r.max()))
        if torch.is_tensor(poses) or isinstance(poses, np.ndarray):
            return out.reshape(tuple(poses.shape))
        return list(torch.split(out, lens, 0))

    def lock_outputs(self, output, betas=None):
        """The dict a forward returns -> its poses [B, n, 165] (packing.scatter_parts of the four predicted parts) locked by
        its pred_contact along its pred_transl, at the motion rate."""
        poses = packing.scatter_parts(output["pred_upper"], output["pred_lower"], output["pred_hands"], output["pred_facepose"])
        return self.lock(poses, output["pred_transl"], output["pred_contact"], betas=betas)
