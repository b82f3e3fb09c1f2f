"""Seeded inputs of tests/golden/joint_metrics.npz: a synthetic SMPL-X model file, smooth pose clips, an avg_vel vector,
impulse audio and retrieval exemplars.  Used by make_joint_metrics_golden.py (with the reference) and by
tests/test_joint_metrics_*.py (without it)."""
import os
import wave

import numpy as np

SMPLX_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
                 20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38,
                 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53]
N_VERTS = 48
N_SHAPE = 310                    # >= 300 betas (the real file has 300 + 100 expression components)
EVAL_N = 64
N_FRAMES = 70                    # saved clip length; the evaluation keeps the first EVAL_N
N_CLIPS = 6
SPEAKERS = ("scott", "wayne", "scott", "lawrence", "wayne", "scott")
RETRIEVAL_CLIPS = (0, 2, 3)
MM_REPS = (5, 3, 5)              # repetitions per multimodality group (group 1 misses rep3 and rep4)
MODEL_SEED = 77
AUDIO_SR = 16000
POSE_FPS = 30


def smplx_model(seed=MODEL_SEED):
    """{key: array} of a SMPLX_NEUTRAL_2020.npz: the real 55-entry kintree_table (root stored as 2**32-1), random
    v_template / J_regressor (each joint a convex mix of 4 vertices) / shapedirs, small hand means."""
    rng = np.random.default_rng(seed)
    jr = np.zeros((55, N_VERTS))
    for j in range(55):
        idx = rng.choice(N_VERTS, 4, replace=False)
        w = rng.random(4) + 0.2
        jr[j, idx] = w / w.sum()
    kt = np.array([SMPLX_PARENTS, list(range(55))], dtype=np.int64)
    kt[0, 0] = 2 ** 32 - 1
    return dict(kintree_table=kt, J_regressor=jr, v_template=rng.standard_normal((N_VERTS, 3)) * 0.3,
                shapedirs=rng.standard_normal((N_VERTS, 3, N_SHAPE)) * 2e-3,
                hands_meanl=rng.uniform(-0.2, 0.2, 45), hands_meanr=rng.uniform(-0.2, 0.2, 45),
                f=np.zeros((1, 3), np.int64))


def smooth_clip(rng, n=N_FRAMES, amp=0.5):
    """[n, 165] float32 axis-angle: per channel a sum of 3 sinusoids (periods 0.5-3 s), |angle| < 2 < pi for every joint."""
    t = np.arange(n)[:, None] / POSE_FPS
    out = rng.uniform(-0.3, 0.3, (1, 165))
    for _ in range(3):
        f = rng.uniform(1 / 3.0, 2.0, (1, 165))
        ph = rng.uniform(0, 2 * np.pi, (1, 165))
        out = out + amp / 3 * rng.uniform(0.3, 1.0, (1, 165)) * np.sin(2 * np.pi * f * t + ph)
    return out.astype(np.float32)


def inputs(seed):
    """Everything a fixture folder holds, from one seed: clips, betas, retrieval, onset impulses, mm groups."""
    rng = np.random.default_rng(seed)
    pred = [smooth_clip(rng) for _ in range(N_CLIPS)]
    gt = [smooth_clip(rng) for _ in range(N_CLIPS)]
    betas = [rng.standard_normal(300) * (0.0 if i == 1 else 1.0) for i in range(N_CLIPS)]
    retrieval = {}
    for i in RETRIEVAL_CLIPS:
        r = smooth_clip(rng)
        r[:, 3 * np.array([0, 1, 2, 4, 5])] = 0.0                     # joints the exemplar does not cover (whole joints)
        zero = rng.choice(55, 12, replace=False)
        r[:, (3 * zero[:, None] + np.arange(3)).ravel()] = 0.0
        retrieval[i] = r
    n_samples = int(AUDIO_SR / POSE_FPS * N_FRAMES)
    impulses = []
    for i in range(N_CLIPS):
        k = rng.integers(3, 9)
        impulses.append(np.sort(rng.choice(np.arange(6000, 28000), k, replace=False)))   # inside the evaluated slice
    mm = [[smooth_clip(rng, EVAL_N) for _ in range(r)] for r in MM_REPS]     # (evaluate_mm.py does not truncate expressions)
    return dict(pred=pred, gt=gt, betas=betas, retrieval=retrieval, impulses=impulses, n_samples=n_samples, mm=mm)


def clip_names():
    return ["test/%d_%s_0_%d_%d" % (i, s, i, i) for i, s in enumerate(SPEAKERS)]


def mm_names():
    return ["mm/%d_%s_1_%d" % (g, SPEAKERS[g], g) for g in range(len(MM_REPS))]


def write_wav(path, n_samples, impulses):
    a = np.zeros(n_samples, np.int16)
    a[impulses] = 32767
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(AUDIO_SR)
        w.writeframes(a.tobytes())


def read_wav(path):
    with wave.open(path, "rb") as w:
        a = np.frombuffer(w.readframes(w.getnframes()), np.int16)
    return a.astype(np.float32) / 32768.0


def write_folder(root, inp, save_sample_files):
    """The evaluation folder (save_sample_files layout: root/test/<clip>/{pred,gt}_motion.npz, gt_audio.wav, retrieval_0.npz).
    The ground truth's betas are overwritten with the
    fixture's (the saved files carry zeros)."""
    names = clip_names()
    z = lambda n: np.zeros((n, 100), np.float32)
    zt = lambda n: np.zeros((n, 3), np.float32)
    save_sample_files(root, names, (np.stack(inp["pred"]), np.stack([z(N_FRAMES)] * N_CLIPS), np.stack([zt(N_FRAMES)] * N_CLIPS)),
                      (np.stack(inp["gt"]), np.stack([z(N_FRAMES)] * N_CLIPS), np.stack([zt(N_FRAMES)] * N_CLIPS)))
    for i, name in enumerate(names):
        d = os.path.join(root, name)
        gfile = os.path.join(d, "gt_motion.npz")
        with np.load(gfile) as f:
            fields = {k: f[k] for k in f.files}
        fields["betas"] = inp["betas"][i]
        np.savez(gfile, **fields)
        write_wav(os.path.join(d, "gt_audio.wav"), inp["n_samples"], inp["impulses"][i])
        if i in inp["retrieval"]:
            np.savez(os.path.join(d, "retrieval_0.npz"), poses=inp["retrieval"][i])
    return names


def write_mm_folder(root, inp, save_sample_files):
    """root/mm/<clip>_rep<k>/pred_motion.npz, the layout evaluate_mm.py reads."""
    z = lambda n: np.zeros((n, 100), np.float32)
    zt = lambda n: np.zeros((n, 3), np.float32)
    for g, reps in enumerate(inp["mm"]):
        names = [mm_names()[g] + "_rep%d" % k for k in range(len(reps))]
        n = reps[0].shape[0]
        save_sample_files(root, names, (np.stack(reps), np.stack([z(n)] * len(reps)), np.stack([zt(n)] * len(reps))))


def onset_times(inp, i, n=EVAL_N):
    """alignment.load_audio of the impulse audio: impulse positions inside [a_offset, len - a_offset) of the first n frames,
    relative to a_offset, in seconds (what the stub onset detector returns)."""
    length = int(AUDIO_SR / POSE_FPS * n)
    a_off = int(10 * (AUDIO_SR / POSE_FPS))
    imp = inp["impulses"][i]
    imp = imp[(imp >= a_off) & (imp < length - a_off)]
    return (imp - a_off) / AUDIO_SR


def avg_vel(inp, model):
    """[55] float64: the mean velocity norm per joint of the ground-truth clips (float64 forward kinematics of smplx_fk.py),
    so that the 0.3 threshold falls inside the velocity range; 1 for joints that never move (the root)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("smplx_fk", os.path.join(os.path.dirname(os.path.abspath(__file__)), "smplx_fk.py"))
    smplx_fk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(smplx_fk)
    vs = []
    for i, g in enumerate(inp["gt"]):
        j = smplx_fk.posed_joints(g[:EVAL_N], smplx_fk.rest_joints(model, inp["betas"][i]), model["parents"], model["pose_mean"])
        vs.append(np.linalg.norm(np.diff(j, axis=0), axis=2) * POSE_FPS)
    m = np.concatenate(vs).mean(axis=0)
    return np.where(m > 1e-9, m, 1.0)
