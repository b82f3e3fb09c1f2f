"""Seeded inputs of tests/golden/srgr.npz: the evaluation folder of joint_fixture.py (its model, ground truth, betas, audio and
retrieval) with predictions that are the ground truth plus a pose perturbation, and one sem_score vector per clip.  Used by
make_srgr_golden.py (with the reference) and by tests/test_srgr_*.py (without it).

The perturbation is small on most frames (every joint far below the SRGR threshold) and large on a window of each clip (most
joints far above it), so that few joint-frames come near the threshold and a seed exists for which none does."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


jf = _load("joint_fixture")

EVAL_N = 32                      # one FGD window; the saved clips have jf.N_FRAMES = 70 frames
N_CLIPS = jf.N_CLIPS
MOTION_FPS = 15
POSE_FPS = 30
QUIET = 0.01                     # radians: the perturbation outside the window
LOUD = 1.2                       # ... inside it
WINDOW = (8, 14)                 # frames of the loud window (shortest, longest)
# sem_score lengths at MOTION_FPS: clip 0 resamples to exactly EVAL_N frames, clip 3 to 34, the others to 70; clip 2 is all zero
SEM_LEN = (16, 35, 35, 17, 35, 35)
ZERO_CLIP = 2
SEM_LEN_30 = (32, 70, 70, 33, 70, 70)     # the vectors of the second score, at 30 fps (no resampling)


def inputs(seed):
    """joint_fixture.inputs(seed) with pred = gt + perturbation."""
    inp = jf.inputs(seed)
    rng = np.random.default_rng([seed, 1])
    pred = []
    for g in inp["gt"]:
        n = g.shape[0]
        length = int(rng.integers(WINDOW[0], WINDOW[1] + 1))
        start = int(rng.integers(0, EVAL_N - length + 1))
        amp = np.full((n, 1), QUIET)
        amp[start:start + length] = LOUD
        pred.append((g + amp * rng.uniform(-1.0, 1.0, (n, 165))).astype(np.float32))
    inp["pred"] = pred
    # audio impulses inside the slice the reference's beat alignment reads for EVAL_N frames (it divides by their count)
    inp["impulses"] = [np.sort(rng.choice(np.arange(6000, 11000), int(rng.integers(2, 5)), replace=False)) for _ in range(N_CLIPS)]
    return inp


def _steps(rng, m):
    """[m] float32, piecewise constant with values from {0, 0.1, ..., 1.0}, about half of the segments zero."""
    out = np.zeros(m, np.float32)
    i = 0
    while i < m:
        k = int(rng.integers(2, 7))
        out[i:i + k] = np.float32(rng.integers(1, 11) / 10.0) if rng.random() < 0.55 else 0.0
        i += k
    return out


def sem_scores(seed, motion_fps=MOTION_FPS):
    """Per clip the sem_score vector at motion_fps (15: SEM_LEN, 30: SEM_LEN_30)."""
    lens = {MOTION_FPS: SEM_LEN, POSE_FPS: SEM_LEN_30}[motion_fps]
    rng = np.random.default_rng([seed, 2, motion_fps])
    out = [_steps(rng, m) for m in lens]
    out[ZERO_CLIP][:] = 0.0
    for i, v in enumerate(out):
        if i != ZERO_CLIP and not v[:EVAL_N * motion_fps // POSE_FPS].any():
            v[1:4] = np.float32(0.7)                 # (every other clip weighs at least some evaluated frames)
    return out


def clip_names():
    return jf.clip_names()


def write_folder(root, inp, save_sample_files):
    return jf.write_folder(root, inp, save_sample_files)
