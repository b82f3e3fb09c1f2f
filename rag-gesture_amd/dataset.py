"""Model inputs, retrieval records and the mean-velocity file from raw SMPL-X recordings: the motion side of
mogen/datasets/beatx_dataset.py without smplx, librosa, lmdb or pyarrow.

    :195-200    idmapping                         -> idmapping
    :206-289    calculate_mean_velocity           -> ClipPreprocessor.mean_velocity (rg_smplx_joints_expr, rg_joint_speed_sums)
    :354-440    cache_generation, motion side     -> ClipPreprocessor.prepare (rg_smplx_joints_expr, rg_clip_prepare)
    :721-771, :806-808  _sample_from_clip windows -> window_table
    :991-1096   per-window annotations            -> longform.window_annotations (kept if fully inside, window time)
    :1182-1295  __getitem__                       -> SMPLXClipDataset.__getitem__
    builder.py:55-92  beatx_collate_fn            -> SMPLXClipDataset.collate

What is out of scope stays with the caller: parsing TextGrid / CSV / JSON annotation files (RawClip.annotations holds the
parsed, time-stamped lists) and LMDB writing.  RawClip.audio is a 16 kHz mono waveform; audio.load_16k reads WAV recordings of
other rates, channel counts and PCM / float formats and resamples them on the device (where the reference calls librosa.load and
librosa.resample, :474-475; parity with librosa's soxr_hq filter is not pinned), compressed formats stay with the caller.  The
kernels have no CPU path.

    python -m rag-gesture_amd.dataset mean-vel <folder of *.npz> --smplx_path SMPLX_NEUTRAL_2020.npz -o mean_vel_smplxflame_30.npy
"""
import argparse
import ctypes
import math
import os

import numpy as np
import torch

from . import capi, longform, packing
from .smplx import IN_DIM, N_BETAS, N_EXPR, N_JOINTS, SMPLXJoints, SMPLXModelError, offsets
from .features import merge_disco_textsegs

RAW_FPS = 30                     # the rate of a raw BEAT-X recording (beatx_dataset.py:356-357)
CONTACT_THRESHOLD = 0.01         # beatx_dataset.py:422
CONTACT_JOINTS = (7, 8, 10, 11)  # beatx_dataset.py:396
RAW_KEYS = ("poses", "trans", "expressions", "betas")       # what cache_generation reads of a recording (:355-364)
ANNOTATION_KEYS = ("text_segments", "discourse", "prominence", "gesture_labels")
PART_NAMES = ("upper", "lower", "hands", "face")            # order of rg_clip_prepare's part_cols
MEAN_VEL_BATCH_FRAMES = 1 << 16  # raw frames per launch of mean_velocity (43 MB of joints)

ClipPrepareArgs = capi.struct("rg_clip_prepare_args")
JointSpeedArgs = capi.struct("rg_joint_speed_args")


def idmapping(speaker):
    """beatx_dataset.py:195-200: the 25 BEAT-X speaker numbers (1-7, 9-13, 15-18, 20-25, 27, 28, 30) -> 0..24."""
    speaker = int(speaker)
    if speaker == 30:
        speaker = 8
    if speaker == 28:
        speaker = 14
    if speaker == 27:
        speaker = 19
    return speaker - 1


def part_columns():
    """[159] int32: the source columns of motion_upper (39), motion_lower (27), motion_hands (90), motion_face (3) in a
    165-column pose row, i.e. np.nonzero of packing.part_masks() (beatx_dataset.py:426-440 `pose[:, mask.astype(bool)]`)."""
    masks = packing.part_masks()
    return np.concatenate([np.nonzero(masks[p])[0] for p in PART_NAMES]).astype(np.int32)


class RawClip:
    """One raw recording: poses [F30, 165], trans [F30, 3], expressions [F30, 100] at 30 fps, betas [300], the speaker id
    the model is conditioned on (0..24), and optionally
      annotations: dict of the parsed, time-stamped lists of the whole recording in seconds -- text_segments
                   ([[start, end], text]), discourse (8-tuples (conn, sense, arg1, arg2, start, end, conn_start, conn_end)),
                   prominence ((word, start, end, value)), gesture_labels (dicts name / word / start / end): the shapes
                   longform.window_annotations cuts;
      audio:       the 16 kHz waveform [n] (only its length is used here: it bounds the usable seconds)."""

    def __init__(self, name, poses, trans, expressions, betas, speaker_id, annotations=None, audio=None):
        self.name = str(name)
        self.poses = np.ascontiguousarray(poses, np.float32)
        n = self.poses.shape[0]
        if self.poses.ndim != 2 or self.poses.shape[1] != IN_DIM:
            raise ValueError("%s: poses has shape %s, expected (n, %d)" % (name, self.poses.shape, IN_DIM))
        self.trans = np.ascontiguousarray(trans, np.float32).reshape(-1, 3)
        self.expressions = np.ascontiguousarray(expressions, np.float32).reshape(-1, N_EXPR)
        self.betas = np.ascontiguousarray(betas, np.float64).reshape(-1)
        for what, v in (("trans", self.trans), ("expressions", self.expressions)):
            if v.shape[0] != n:
                raise ValueError("%s: %s holds %d frames, poses %d" % (name, what, v.shape[0], n))
        if self.betas.shape[0] != N_BETAS:
            raise ValueError("%s: betas has %d entries, expected %d" % (name, self.betas.shape[0], N_BETAS))
        self.speaker_id = int(speaker_id)
        ann = dict(annotations or {})
        unknown = sorted(set(ann) - set(ANNOTATION_KEYS))
        if unknown:
            raise ValueError("%s: unknown annotation key(s) %s" % (name, ", ".join(unknown)))
        self.annotations = {k: list(ann.get(k) or []) for k in ANNOTATION_KEYS}
        self.audio = audio

    @property
    def n_raw(self):
        return self.poses.shape[0]

    @classmethod
    def load(cls, npz_path, speaker_id=None, annotations=None, audio=None, name=None):
        """A BEAT-X `<speaker number>_<speaker>_<...>.npz` (beatx_dataset.py:355-364).  speaker_id None: idmapping of the
        number the file name starts with (:464)."""
        name = os.path.splitext(os.path.basename(str(npz_path)))[0] if name is None else name
        with np.load(npz_path, allow_pickle=False) as f:
            missing = [k for k in RAW_KEYS if k not in f.files]
            if missing:
                raise ValueError("%s: missing key %s" % (npz_path, ", ".join(missing)))
            poses, trans, exprs, betas = (f[k] for k in RAW_KEYS)
        if speaker_id is None:
            head = name.split("_")[0]
            if not head.isdigit():
                raise ValueError("%s: the file name does not start with a speaker number; pass speaker_id=" % name)
            speaker_id = idmapping(int(head))
        return cls(name, poses, trans, exprs, betas, speaker_id, annotations=annotations, audio=audio)


def window_name(file_name, i):
    """beatx_dataset.py:986: sample i of a recording."""
    return "%s/%d" % (file_name, i)


def window_table(n_frames, pose_fps=15, pose_length=150, stride=5, clean_first_seconds=0, clean_final_seconds=0,
                 audio_seconds=None, mode="train"):
    """beatx_dataset.py:721-771, :806-808 -> [(start frame, end frame)] of a recording of n_frames frames at pose_fps, window
    i at position i (its sample is named window_name(file, i)).  audio_seconds: the whole seconds of the recording's audio
    (len(wave) // sample rate, :727), None: no audio.  mode "train": windows of pose_length every `stride` frames; "test":
    stride = pose_length (:764-766); "full": one window of the whole usable span (:757-759)."""
    if mode not in ("train", "test", "full"):
        raise ValueError("mode must be train, test or full, got %r" % (mode,))
    round_seconds = int(n_frames) // int(pose_fps)
    if audio_seconds is not None:
        round_seconds = min(int(audio_seconds), round_seconds)
    start = int(clean_first_seconds) * pose_fps
    end = (round_seconds - int(clean_final_seconds)) * pose_fps
    if mode == "full":
        cut = step = end - start
    elif mode == "test":
        cut = step = int(pose_length)
    else:
        cut, step = int(pose_length), int(stride)
    if cut <= 0 or step <= 0:
        return []
    n = math.floor((end - start - cut) / step) + 1
    return [(start + i * step, start + i * step + cut) for i in range(max(0, n))]


class ClipPreprocessor:
    """Raw recordings -> per-clip device tensors (rg_smplx_joints_expr + rg_clip_prepare) and the mean joint velocity
    (rg_smplx_joints_expr + rg_joint_speed_sums).  The model file needs J_regressor, v_template, shapedirs (400 columns),
    kintree_table and the hand means only."""

    def __init__(self, smplx_model_path_or_dict, pose_fps=15, device=None):
        if RAW_FPS % int(pose_fps):
            raise ValueError("pose_fps should be an aliquot part of %d, got %d" % (RAW_FPS, pose_fps))     # (:356)
        self.pose_fps, self.stride = int(pose_fps), RAW_FPS // int(pose_fps)
        self.smplx = smplx_model_path_or_dict if isinstance(smplx_model_path_or_dict, SMPLXJoints) \
            else SMPLXJoints(smplx_model_path_or_dict, device=device)
        if self.smplx.J_expr is None:
            raise SMPLXModelError("the model file's shapedirs hold no expression components (expected >= %d columns)"
                                  % (N_BETAS + N_EXPR))
        self.device = self.smplx.device
        self.h = self.smplx.h
        self.part_cols = part_columns()
        self.part_cols_dev = torch.from_numpy(self.part_cols).to(self.device)

    def _upload(self, clips):
        dev = self.device
        cat = lambda key: torch.from_numpy(np.concatenate([getattr(c, key) for c in clips], 0)).to(dev)
        return cat("poses"), cat("trans"), cat("expressions"), offsets([c.n_raw for c in clips])

    def strided_frames(self, n_raw):
        """len(x[::stride])."""
        return -(-int(n_raw) // self.stride)

    def prepare(self, clips):
        """-> one dict per clip of fp32 device tensors over its n = ceil(F30 / stride) kept frames: motion [n, 165], trans
        [n, 3], facial [n, 100], motion_upper [n, 39], motion_lower [n, 27], motion_hands [n, 90], motion_face [n, 3],
        contact [n, 4], joints [n, 55, 3] (with expression and translation), beta [n, 300] and speaker_id [n] int64.  The
        clips share two launches; a clip's tensors are slices of the launch's buffers."""
        clips = list(clips)
        if not clips:
            return []
        dev = self.device
        poses, trans, exprs, raw_off = self._upload(clips)
        clip_off = offsets([self.strided_frames(c.n_raw) for c in clips])
        F = int(clip_off[-1])
        joints = self.smplx.joints_strided(poses, exprs, trans, raw_off, clip_off, self.stride, betas=[c.betas for c in clips])
        new = lambda w: torch.empty(F, w, device=dev, dtype=torch.float32)
        out = dict(motion=new(IN_DIM), trans=new(3), facial=new(N_EXPR), motion_upper=new(39), motion_lower=new(27),
                   motion_hands=new(90), motion_face=new(3), contact=new(len(CONTACT_JOINTS)))
        roff_dev, coff_dev = torch.from_numpy(raw_off).to(dev), torch.from_numpy(clip_off).to(dev)
        a = ClipPrepareArgs(poses=poses.data_ptr(), trans=trans.data_ptr(), exprs=exprs.data_ptr(), joints=joints.data_ptr(),
                            part_cols=self.part_cols_dev.data_ptr(), part_cols_host=self.part_cols.ctypes.data,
                            clip_off=coff_dev.data_ptr(), clip_off_host=clip_off.ctypes.data, raw_off=roff_dev.data_ptr(),
                            raw_off_host=raw_off.ctypes.data, motion=out["motion"].data_ptr(), trans_out=out["trans"].data_ptr(),
                            facial=out["facial"].data_ptr(), upper=out["motion_upper"].data_ptr(),
                            lower=out["motion_lower"].data_ptr(), hands=out["motion_hands"].data_ptr(),
                            face=out["motion_face"].data_ptr(), contact=out["contact"].data_ptr(), n_clips=len(clips),
                            raw_rows=int(poses.shape[0]), stride=self.stride, threshold=CONTACT_THRESHOLD)
        self.h.call("clip_prepare", ctypes.byref(a))
        out["joints"] = joints
        res = []
        for i, c in enumerate(clips):
            lo, hi = int(clip_off[i]), int(clip_off[i + 1])
            d = {k: v[lo:hi] for k, v in out.items()}
            d["beta"] = torch.from_numpy(c.betas.astype(np.float32)).to(dev).unsqueeze(0).expand(hi - lo, N_BETAS)   # (:363)
            d["speaker_id"] = torch.full((hi - lo,), c.speaker_id, dtype=torch.int64, device=dev)                    # (:464-465)
            d["name"] = c.name
            res.append(d)
        return res

    def speed_sums(self, clips):
        """[n_clips, 55] float64 (host): per clip and joint the sum over its 30 fps frames of the velocity norm."""
        clips = list(clips)
        for c in clips:
            if c.n_raw < 2:
                raise ValueError("%s: a velocity needs at least 2 frames, the recording holds %d" % (c.name, c.n_raw))
        dev = self.device
        sums, i = [], 0
        while i < len(clips):
            j, rows = i + 1, clips[i].n_raw
            while j < len(clips) and rows + clips[j].n_raw <= MEAN_VEL_BATCH_FRAMES:
                rows += clips[j].n_raw
                j += 1
            batch = clips[i:j]
            poses, trans, exprs, off = self._upload(batch)
            joints = self.smplx.joints_strided(poses, exprs, trans, off, off, 1, betas=[c.betas for c in batch])
            off_dev = torch.from_numpy(off).to(dev)
            s = torch.empty(len(batch), N_JOINTS, device=dev, dtype=torch.float64)
            a = JointSpeedArgs(joints=joints.data_ptr(), clip_off=off_dev.data_ptr(), clip_off_host=off.ctypes.data,
                               sums=s.data_ptr(), n_clips=len(batch), dt=1.0 / RAW_FPS)
            self.h.call("joint_speed_sums", ctypes.byref(a))
            sums.append(s.cpu().numpy())
            i = j
        return np.concatenate(sums, 0) if sums else np.zeros((0, N_JOINTS))

    def mean_velocity(self, clips):
        """beatx_dataset.py:206-289 -> float64 [55]: the mean over all 30 fps frames of all recordings of every joint's
        velocity norm (m/s), the `avg_vel` of evaluation.JointMetrics."""
        clips = list(clips)
        if not clips:
            raise ValueError("no recordings")
        return self.speed_sums(clips).sum(0) / float(sum(c.n_raw for c in clips))


def motion_query(preprocessor, raw_clip, first_frame, n_chunks, start_s, end_s, weights=None, chunk=15):
    """One entry of conditions["motion_queries"][b] for the `motion` retrieval method (retrieval.motion_query_fields) from a raw
    recording: the example is frames [first_frame, first_frame + chunk * n_chunks) of the prepared clip (at the preprocessor's
    pose rate), `start_s` / `end_s` say where in the query clip the exemplar goes, weights (None: upper body and hands) weigh
    the four parts.  -> (start_s, end_s, example) or (start_s, end_s, example, weights)."""
    from .retrieval import MOTION_EXAMPLE_KEYS
    first_frame, n_chunks, chunk = int(first_frame), int(n_chunks), int(chunk)
    n = preprocessor.strided_frames(raw_clip.n_raw)
    if n_chunks < 1 or first_frame < 0 or first_frame + chunk * n_chunks > n:
        raise ValueError("%s: frames [%d, %d) are not inside the clip's %d frames at %d fps"
                         % (raw_clip.name, first_frame, first_frame + chunk * n_chunks, n, preprocessor.pose_fps))
    clip = preprocessor.prepare([raw_clip])[0]
    example = {k: clip[k][first_frame:first_frame + chunk * n_chunks] for k in MOTION_EXAMPLE_KEYS}
    return (float(start_s), float(end_s), example) if weights is None else (float(start_s), float(end_s), example, tuple(weights))


class SMPLXClipDataset:
    """The dataset object of `build_architecture(cfg.model, database=...)` and of test batches, over raw recordings.
    ds[i] / ds["<file>/<i>"] -> the per-sample dict of beatx_dataset.py:1262-1295; ds.retrieval_samples -> the records
    retrieval.build_db_dicts takes; ds.collate(indices) -> the kwargs of model(**data) (builder.py:55-92).

    features(clip_name, t0, t1, annotations) -> dict supplies the window's conditioning the way LongformSynthesizer takes it
    (a batch of one): `audio` [1, 499, 768], `word` [1, n, 768], `text_features` [tensor [L, 768]] (or the per-sample
    `text_feature`); rg.features.WindowFeatures.window fits.  annotations is longform.window_annotations' result for the
    window.  Without `features` those keys are absent from the samples and the records.  A `features` object that offers
    `windows(requests)` (requests: a list of those argument tuples; -> the list of their dicts:
    rg.features.WindowFeatures.for_clips fits) is asked for `feature_batch` windows per call instead of one by one
    (feature_batch=None: such an object is called window by window too).
    window_args: those of window_table (pose_length, stride, clean_first_seconds, clean_final_seconds, mode) and audio_sr.
    The recordings are prepared once, together, on first access to a sample; a window's tensors are views of its clip's."""
    TENSOR_KEYS = ("motion", "motion_upper", "motion_lower", "motion_face", "motion_hands", "contact", "trans", "facial")

    def __init__(self, clips, preprocessor, features=None, audio_sr=16000, feature_batch=32, **window_args):
        self.clips, self.pre, self.features = list(clips), preprocessor, features
        self.feature_batch = None if feature_batch is None else int(feature_batch)
        if self.feature_batch is not None and self.feature_batch < 1:
            raise ValueError("feature_batch must be at least 1 (None: call `features` window by window)")
        names = [c.name for c in self.clips]
        if len(set(names)) != len(names):
            raise ValueError("recording names must be unique")
        self.pose_fps = preprocessor.pose_fps
        self.windows = []                    # (clip index, window index in the clip, start frame, end frame)
        for ci, c in enumerate(self.clips):
            sec = None if c.audio is None else int(np.shape(c.audio)[-1]) // int(audio_sr)
            table = window_table(preprocessor.strided_frames(c.n_raw), pose_fps=self.pose_fps, audio_seconds=sec, **window_args)
            self.windows += [(ci, i, s, e) for i, (s, e) in enumerate(table)]
        self.names = [window_name(self.clips[ci].name, i) for ci, i, _, _ in self.windows]
        self.name_to_idx = {n: k for k, n in enumerate(self.names)}
        self._prepared = None
        if features is not None and self.feature_batch is not None and callable(getattr(features, "windows", None)):
            reqs = [self._window_request(k) for k in range(len(self.windows))]
            feats = []
            for i in range(0, len(reqs), self.feature_batch):
                feats += list(features.windows(reqs[i:i + self.feature_batch]))
            if len(feats) != len(reqs):
                raise ValueError("features.windows answered %d of %d windows" % (len(feats), len(reqs)))
            self._side = [self._window_side(k, feats[k], reqs[k]) for k in range(len(self.windows))]
        else:
            self._side = [self._window_side(k) for k in range(len(self.windows))]
        self.retrieval_samples = []
        for k, side in enumerate(self._side):
            rec = dict(sample_name=self.names[k], speaker_id=self.clips[self.windows[k][0]].speaker_id,
                       discourse=side["discourse"], prominence=side["prominence"], gesture_labels=side["gesture_labels"])
            if "text_feature" in side:
                rec["text_feature"] = side["text_feature"]
            self.retrieval_samples.append(rec)

    def _window_request(self, k):
        """(clip_name, t0, t1, annotations) of window k: the arguments of `features`."""
        ci, _, s, e = self.windows[k]
        clip = self.clips[ci]
        t0, t1 = s / self.pose_fps, e / self.pose_fps
        return clip.name, t0, t1, longform.window_annotations({key: [clip.annotations[key]] for key in ANNOTATION_KEYS}, t0, t1)

    def _window_side(self, k, feats=None, request=None):
        """Everything of window k that is not cut from the prepared motion: annotations in window time, raw_word, features
        (feats: the window's answer from a batched `features.windows` call to its `request`)."""
        name, t0, t1, ann = self._window_request(k) if request is None else request
        side = {key: ann[key][0] for key in ANNOTATION_KEYS}
        side["raw_word"] = " ".join(seg[1] for seg in merge_disco_textsegs(side["text_segments"]))     # (:1042-1047)
        if self.features is not None:
            for key, v in (self.features(name, t0, t1, ann) if feats is None else feats).items():
                if key == "text_features":
                    side["text_feature"] = v[0]
                elif key in ("audio", "word") and torch.is_tensor(v) and v.dim() == 3:
                    side[key] = v[0]
                elif key == "raw_word":
                    continue                 # (the dataset's own: the merged segments of the window)
                else:
                    side[key] = v
        return side

    def __len__(self):
        return len(self.windows)

    def prepared(self):
        if self._prepared is None:
            self._prepared = self.pre.prepare(self.clips)
        return self._prepared

    def __getitem__(self, key):
        if isinstance(key, str):
            if key not in self.name_to_idx:
                raise KeyError(key)
            k = self.name_to_idx[key]
        else:
            k = int(key)
            if not 0 <= k < len(self.windows):
                raise IndexError("sample %d of %d" % (k, len(self.windows)))
        ci, _, s, e = self.windows[k]
        clip = self.prepared()[ci]
        out = {name: clip[name][s:e] for name in self.TENSOR_KEYS}
        out.update(motion_length=e - s, motion_mask=torch.ones(e - s, device=self.pre.device), beta=clip["beta"][s:e],
                   speaker_id=clip["speaker_id"][s:e], sample_name=self.names[k], sample_idx=k)
        out.update(self._side[k])
        return out

    LIST_KEYS = ("motion_length", "raw_word", "text_segments", "gesture_labels", "discourse", "prominence", "sample_idx",
                 "sample_name")

    def collate(self, indices):
        """builder.py:55-92 beatx_collate_fn over ds[i] for i in indices: tensors stacked (new storage: the model re-zeroes
        `trans` in place), list-valued keys as lists, speaker_id -> speaker_ids, text_feature -> text_features."""
        batch = [self[i] for i in indices]
        if not batch:
            raise ValueError("no samples")
        out = {}
        for key in self.TENSOR_KEYS + ("motion_mask", "beta") + tuple(k for k in ("audio", "word") if k in batch[0]):
            out[key] = torch.stack([b[key] for b in batch])
        out["speaker_ids"] = torch.stack([b["speaker_id"] for b in batch])
        if "text_feature" in batch[0]:
            out["text_features"] = [b["text_feature"] for b in batch]
        for key in self.LIST_KEYS:
            out[key] = [b[key] for b in batch]
        return out


def load_folder(folder):
    """Every *.npz of a folder as RawClip, by file name (beatx_dataset.py:223-226)."""
    files = sorted(f for f in os.listdir(folder) if f.endswith(".npz"))
    if not files:
        raise ValueError("%s holds no .npz recording" % folder)
    return [RawClip.load(os.path.join(folder, f), speaker_id=0) for f in files]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m rag-gesture_amd.dataset")
    sub = ap.add_subparsers(dest="cmd", required=True)
    mv = sub.add_parser("mean-vel", help="the mean joint velocity of a folder of raw recordings (--avg_vel_path of the evaluation)")
    mv.add_argument("folder")
    mv.add_argument("--smplx_path", required=True, help="SMPLX_NEUTRAL_2020.npz")
    mv.add_argument("-o", "--output", default="mean_vel_smplxflame_30.npy")
    args = ap.parse_args(argv)
    avg = ClipPreprocessor(args.smplx_path, pose_fps=RAW_FPS).mean_velocity(load_folder(args.folder))
    np.save(args.output, avg)
    print("%s: %d joints, mean %.6f m/s" % (args.output, avg.shape[0], float(avg.mean())))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
