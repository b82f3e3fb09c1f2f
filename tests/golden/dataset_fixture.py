"""Seeded raw SMPL-X recordings and a float64 NumPy restatement of the motion side of mogen/datasets/beatx_dataset.py: the
yardstick of tests/test_dataset_*.py (the reference's dataset class needs smplx, librosa and lmdb).  Built on smplx_lbs.lbs
(expression and transl) and face_fixture.smplx_model (300 shape + 100 expression directions).  Every restating function cites
the reference lines it restates.  `python tests/golden/dataset_fixture.py` rewrites tests/golden/dataset.npz.

Recordings (30 fps): 1, 2, 3, 61 and 301 frames -- after stride 2: 1, 1, 2, 31 and 151 frames (odd and even tails, the
one-frame case).  The usable length of a recording is its WHOLE seconds (beatx_dataset.py:721), so the 151-frame clip gives
one 150-frame window, whatever the stride; a sixth recording of 331 frames (166 kept, 11 whole seconds = 165 usable frames)
is there for windows that overlap (16 windows under stride 1)."""
import importlib.util
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


lbs, ff = _load("smplx_lbs"), _load("face_fixture")

SEED = 2026
RAW_FPS = 30
POSE_FPS = 15
STRIDE = RAW_FPS // POSE_FPS
RAW_LENS = (1, 2, 3, 61, 301, 331)
# BEAT-X file names `<speaker number>_<speaker>_<...>`: the numbers 30, 28 and 27 are the ones idmapping moves (:195-200)
NAMES = ("1_wayne_0_1_1", "30_katya_0_2_2", "28_tiffnay_0_3_3", "27_yingqing_0_4_4", "5_stewart_0_5_5", "13_lu_0_6_6")
SPEAKER_IDS = (0, 7, 13, 18, 4, 12)
CONTACT_JOINTS = (7, 8, 10, 11)
CONTACT_THRESHOLD = 0.01
HOLD, MOVE = 11, 13                    # raw frames of a planted span and of a moving span
GOLD = os.path.join(HERE, "dataset.npz")


def smplx_model():
    return ff.smplx_model()


def warped_time(n):
    """[n] seconds: the clock runs for MOVE frames, then stands still for HOLD frames (pose and trans are held: planted)."""
    t, out = 0.0, []
    for i in range(n):
        out.append(t)
        if i % (HOLD + MOVE) < MOVE:
            t += 1.0 / RAW_FPS
    return np.asarray(out)


def smooth_at(rng, t, k, amp):
    """[len(t), k] float32: per channel an offset in [-amp, amp] and 3 sinusoids (0.33-2 Hz) of amplitude <= amp / 5."""
    t = np.asarray(t)[:, None]
    out = rng.uniform(-amp, amp, (1, k))
    for _ in range(3):
        f = rng.uniform(1 / 3.0, 2.0, (1, k))
        ph = rng.uniform(0, 2 * np.pi, (1, k))
        out = out + amp / 5 * rng.uniform(0.3, 1.0, (1, k)) * np.sin(2 * np.pi * f * t + ph)
    return out.astype(np.float32)


def recordings(seed=SEED):
    """[{name, poses [n, 165], trans [n, 3], expressions [n, 100], betas [300]}]: smooth poses, |trans| <= 1 m, non-zero
    betas and expressions; planted and moving spans alternate."""
    rng = np.random.default_rng(seed)
    out = []
    for name, n in zip(NAMES, RAW_LENS):
        t = warped_time(n)
        rec = dict(name=name, poses=smooth_at(rng, t, 165, 0.4), trans=smooth_at(rng, t, 3, 0.6),
                   expressions=smooth_at(rng, t, 100, 1.0), betas=rng.standard_normal(300))
        assert np.abs(rec["trans"]).max() <= 1.0
        out.append(rec)
    return out


def write_npz(folder, recs):
    """One `<name>.npz` per recording with the keys cache_generation reads (:355-364)."""
    paths = []
    for r in recs:
        paths.append(os.path.join(folder, r["name"] + ".npz"))
        np.savez(paths[-1], poses=r["poses"], trans=r["trans"], expressions=r["expressions"], betas=r["betas"],
                 model="smplx2020", gender="neutral", mocap_frame_rate=RAW_FPS)
    return paths


# ------------------------------------------------------------------------------------------------ the restatement (float64)
def idmapping(i):
    """beatx_dataset.py:195-200."""
    if i == 30:
        i = 8
    if i == 28:
        i = 14
    if i == 27:
        i = 19
    return i - 1


def strided(x, stride=STRIDE):
    """beatx_dataset.py:357-360: `pose_data[key][::stride]`."""
    return x[::stride]


def joints(model, rec, stride=1):
    """beatx_dataset.py:373-415 / :226-272: smplx(betas, transl, expression, the pose parts)["joints"][:, :55] of every kept
    frame -> [n, 55, 3] float64 (lbs returns J_transformed; smplx adds transl to the joints)."""
    p, e, t = (strided(rec[k], stride) for k in ("poses", "expressions", "trans"))
    return lbs.lbs(model, p, rec["betas"], e, None)[1] + np.asarray(t, np.float64)[:, None, :]


def contacts(j):
    """beatx_dataset.py:417-424 on the kept frames' joints [n, 55, 3] -> (feetv [n, 4], contact [n, 4] 0 / 1): feetv[t] =
    ||joint[t + 1] - joint[t]|| for joints (7, 8, 10, 11), feetv[last] = 0, contact = feetv < 0.01."""
    f = j[:, CONTACT_JOINTS, :]
    feetv = np.zeros((f.shape[0], len(CONTACT_JOINTS)))
    feetv[:-1] = np.linalg.norm(f[1:] - f[:-1], axis=-1)
    return feetv, (feetv < CONTACT_THRESHOLD).astype(np.float64)


def part_gathers(poses, masks):
    """beatx_dataset.py:426-440: `(pose * mask)[:, mask.astype(bool)]` per body part; masks: {part: bool [165]}."""
    return {k: (poses * m)[:, m.astype(bool)] for k, m in masks.items()}


def speed_norms(j30):
    """beatx_dataset.py:274-286 on one recording's 30 fps joints [n, 55, 3], n >= 2 -> [n, 55]: forward / central / backward
    differences over dt = 1 / 30, the norm per joint."""
    dt = 1.0 / RAW_FPS
    x = j30.reshape(j30.shape[0], -1).T
    vel = np.concatenate([(x[:, 1:2] - x[:, :1]) / dt, (x[:, 2:] - x[:, :-2]) / (2 * dt), (x[:, -1:] - x[:, -2:-1]) / dt], 1)
    return np.linalg.norm(vel.T.reshape(-1, 55, 3), axis=2)


def mean_velocity(all_j30):
    """beatx_dataset.py:287-288: the mean over the frames of all recordings -> [55]."""
    return np.mean(np.concatenate([speed_norms(j) for j in all_j30], 0), 0)


def window_table(n_frames, pose_fps=POSE_FPS, pose_length=150, stride=5, clean_first_seconds=0, clean_final_seconds=0,
                 audio_seconds=None, mode="train"):
    """beatx_dataset.py:721-771, :806-808 -> [(start, end)]."""
    round_seconds_skeleton = n_frames // pose_fps                                   # :721
    if audio_seconds is not None:
        round_seconds_skeleton = min(audio_seconds, round_seconds_skeleton)         # :737
    clip_s_t, clip_e_t = clean_first_seconds, round_seconds_skeleton - clean_final_seconds        # :743
    clip_s_f_pose, clip_e_f_pose = clip_s_t * pose_fps, clip_e_t * pose_fps         # :745
    if mode == "full":
        cut_length = clip_e_f_pose - clip_s_f_pose                                  # :757-759
        step = cut_length
    elif mode == "test":
        cut_length = step = pose_length                                             # :764-766
    else:
        cut_length, step = pose_length, stride                                      # :768-769
    if cut_length <= 0:
        return []
    num_subdivision = math.floor((clip_e_f_pose - clip_s_f_pose - cut_length) / step) + 1         # :771
    out = []
    for i in range(num_subdivision):                                                # :806-808
        start_idx = clip_s_f_pose + i * step
        out.append((start_idx, start_idx + cut_length))
    return out


def restated(recs=None):
    """What dataset.npz records: per recording the kept frames' feetv and contact, and avg_vel over the recordings of >= 2
    frames."""
    recs = recordings() if recs is None else recs
    m = lbs.load_model(smplx_model())
    out = {}
    j30 = []
    for i, r in enumerate(recs):
        j = joints(m, r)
        out["feetv_%d" % i], out["contact_%d" % i] = contacts(strided(j))
        if j.shape[0] >= 2:
            j30.append(j)
    out["avg_vel"] = mean_velocity(j30)
    return out


def contact_statistics(rest, bound):
    """(share of flags within 2 sqrt(3) bound of the threshold, share of ones among the others)."""
    feetv = np.concatenate([rest["feetv_%d" % i] for i in range(len(RAW_LENS))]).ravel()
    flag = np.concatenate([rest["contact_%d" % i] for i in range(len(RAW_LENS))]).ravel()
    near = np.abs(feetv - CONTACT_THRESHOLD) <= 2 * np.sqrt(3.0) * bound
    return near.mean(), flag[~near].mean()


if __name__ == "__main__":
    r = restated()
    np.savez_compressed(GOLD, seed=SEED, **{k: (v.astype(np.uint8) if k.startswith("contact") else v) for k, v in r.items()})
    print("near-threshold share %.4f, share of ones %.3f, min avg_vel %.3f" % (contact_statistics(r, 1e-5) + (r["avg_vel"].min(),)))
