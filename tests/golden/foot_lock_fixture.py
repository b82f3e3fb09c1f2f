"""Seeded inputs of the foot lock tests (tests/test_foot_lock_cpu.py, tests/test_foot_lock_gpu.py): a leg-shaped synthetic
SMPL-X model, pose clips with bent knees and runs of ankle flags, a clip whose targets lie out of reach, and the `walker`, a
kinematic gait under a drifting translation.  Up is y, forward is z.  Nothing here imports the product."""
import numpy as np

N_JOINTS = 55
SMPLX_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
                 20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38,
                 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53]
N_SHAPE = 310
THIGH = SHANK = 0.4
# no pair, one pair, the wave edge (63, 64, 65), one tile minus (150), the tile edge (256, 257), three tiles with carries in both
# directions (600)
LENS = (1, 2, 63, 64, 65, 150, 256, 257, 600)
BLEND = 3
HI, LO = (0.75, 1.0), (0.0, 0.25)                # a flag is drawn from one of the two: well away from 0.5


def rest_pose():
    """[55, 3] float32: pelvis at the origin, the legs straight down (hips 9 cm below and 8 cm beside it, thigh and shank 0.4 m,
    the foot 6 cm lower and 12 cm forward), a spine, and arms and fingers as short chains."""
    J = np.zeros((N_JOINTS, 3))
    step = {1: (0.08, -0.09, 0.0), 2: (-0.08, -0.09, 0.0), 3: (0.0, 0.11, -0.02), 4: (0.0, -THIGH, 0.0), 5: (0.0, -THIGH, 0.0),
            6: (0.0, 0.13, 0.01), 7: (0.0, -SHANK, 0.0), 8: (0.0, -SHANK, 0.0), 9: (0.0, 0.06, 0.01), 10: (0.0, -0.06, 0.12),
            11: (0.0, -0.06, 0.12), 12: (0.0, 0.2, -0.03), 13: (0.07, 0.11, -0.01), 14: (-0.07, 0.11, -0.01), 15: (0.0, 0.1, 0.03),
            16: (0.11, 0.03, 0.0), 17: (-0.11, 0.03, 0.0), 18: (0.26, 0.0, -0.01), 19: (-0.26, 0.0, -0.01), 20: (0.25, 0.0, 0.0),
            21: (-0.25, 0.0, 0.0)}
    for j in range(1, N_JOINTS):
        J[j] = J[SMPLX_PARENTS[j]] + (step[j] if j in step else ((0.03 if j < 40 else -0.03) * (1 + (j % 3) * 0.2), -0.005 * (j % 5), 0.01 * (j % 2)))
    return J.astype(np.float32)


def smplx_model(shape_scale=0.0):
    """{key: array} of an SMPL-X model file whose joints ARE its 55 vertices: identity J_regressor, v_template = rest_pose(),
    zero shapedirs (the betas move nothing; shape_scale > 0: seeded ones of that size, for the tests that pass betas), small
    hand means."""
    kt = np.array([SMPLX_PARENTS, list(range(N_JOINTS))], dtype=np.int64)
    kt[0, 0] = 2 ** 32 - 1
    rng = np.random.default_rng(7)
    shapedirs = np.random.default_rng(8).standard_normal((N_JOINTS, 3, N_SHAPE)) * shape_scale
    return dict(kintree_table=kt, J_regressor=np.eye(N_JOINTS), v_template=rest_pose().astype(np.float64),
                shapedirs=shapedirs, hands_meanl=rng.uniform(-0.2, 0.2, 45), hands_meanr=rng.uniform(-0.2, 0.2, 45),
                f=np.zeros((1, 3), np.int64))


def _smooth(rng, n, width, amp, fps=15.0):
    """[n, width]: per channel an offset and three sinusoids (periods 0.5 - 3 s): bounded by about amp."""
    t = np.arange(n)[:, None] / fps
    out = rng.uniform(-0.3, 0.3, (1, width)) * amp
    for _ in range(3):
        f = rng.uniform(1 / 3.0, 2.0, (1, width))
        ph = rng.uniform(0, 2 * np.pi, (1, width))
        out = out + amp / 3 * rng.uniform(0.3, 1.0, (1, width)) * np.sin(2 * np.pi * f * t + ph)
    return out


def _flags(rng, n, start_set):
    """One ankle's flags [n]: runs of set flags (1, 2, 5, 20 or 60 long) and gaps (1, 2: shorter than 2 blend; 6, 7, 13, 30:
    at and above it), drawn alternately."""
    c = np.zeros(n)
    t, on = 0, start_set
    while t < n:
        k = int(rng.choice((1, 2, 5, 20, 60) if on else (1, 2, 6, 7, 13, 30)))
        c[t:t + k] = rng.uniform(*(HI if on else LO), min(k, n - t))
        t, on = t + k, not on
    return c


def clip(rng, n, bend=1.0, leg_amp=0.12):
    """One clip -> poses [n, 165], transl [n, 3], contact [n, 4], float32.  Every joint moves smoothly (amplitude 0.4 rad; hips,
    knees and ankles `leg_amp`), the knees are flexed by `bend` rad on top (a leg of 0.8 m then spans about 0.70 m: a locked
    ankle has some 9 cm to go before the leg is stretched), the translation sways by about 3 cm.  Ankle 0 is flagged from frame
    0, ankle 1 up to the last pair; a clip of at least 257 frames has ankle 0 flagged across frame 256, the one of 600 frames
    ankle 1 flagged from 100 to 400 (a run that carries through a whole tile) and across frame 512.  The toe flags are noise: the
    lock does not read them."""
    poses = _smooth(rng, n, 165, 0.4)
    for j in (1, 2, 4, 5, 7, 8):
        poses[:, 3 * j:3 * j + 3] = _smooth(rng, n, 3, leg_amp)
    for j in (4, 5):
        poses[:, 3 * j] += bend
    transl = rng.uniform(-1, 1, 3) + _smooth(rng, n, 3, 0.03)
    contact = np.stack([_flags(rng, n, True), _flags(rng, n, False), rng.random(n), rng.random(n)], 1)
    hi = lambda k: rng.uniform(*HI, k)
    if n >= 2:
        contact[n - 2, 1] = hi(1)[0]
    if n >= 257:
        contact[250:min(262, n), 0] = hi(min(262, n) - 250)
    if n >= 600:
        contact[100:400, 1] = hi(300)
        contact[505:520, 1] = hi(15)
        contact[404:406, 1] = rng.uniform(*LO, 2)                   # a gap of two frames behind the long run
    return poses.astype(np.float32), transl.astype(np.float32), contact.astype(np.float32)


def clips(seed=0, lens=LENS, **kw):
    """-> poses [F, 165], transl [F, 3], contact [F, 4] (float32, clip after clip) and the list of lengths."""
    rng = np.random.default_rng(seed)
    parts = [clip(rng, n, **kw) for n in lens]
    return tuple(np.concatenate([p[i] for p in parts], 0) for i in range(3)) + (list(lens),)


def far_clip(seed=3, n=40):
    """A clip whose knees are almost straight (bend 0.25: the leg spans 0.79 of its 0.8 m) and whose translation travels 1 cm
    per frame under ankles flagged for the whole clip: the targets at both ends of the run lie out of reach."""
    rng = np.random.default_rng(seed)
    poses, transl, contact = clip(rng, n, bend=0.25, leg_amp=0.03)
    transl = (transl + np.arange(n)[:, None] * np.array([0.01, 0.0, 0.004])).astype(np.float32)
    contact[:, :2] = rng.uniform(*HI, (n, 2))
    return poses, transl, contact


def straight_clip(n=24):
    """The two fallbacks of the solve in one clip: an all-zero pose has exactly straight legs (hip, knee and ankle share x and z:
    the bend axis is the hip's own x), and under a purely vertical translation ramp with both ankles flagged throughout every
    target lies exactly on the hip-ankle line (the anchor's x and z are sums of n equal fp32 values over n: exact), so the swing
    is the identity.  The first 13 frames are pulled down and out of reach, the other 11 are pushed up and must bend."""
    poses = np.zeros((n, 165), np.float32)
    transl = np.stack([np.full(n, 0.3), 0.9 - 0.004 * np.arange(n), np.full(n, -0.2)], 1).astype(np.float32)
    contact = np.zeros((n, 4), np.float32)
    contact[:, :2] = 1.0
    return poses, transl, contact


# ---------------------------------------------------------------------------------------------------------------------- walker
WALK_N, WALK_PERIOD = 140, 20
WALK_STEP = 0.025                # m per frame forward (z)
WALK_DRIFT = 0.02                # m per frame sideways (x) added to the translation: twice the 1 cm of the contact rule
WALK_HIP = 0.66                  # m: the hips above the planted ankles


def _leg_angles(dz, h):
    """Hip and knee flexion (rotations about x) that put the ankle dz forward of and h below the hip, the knee in front."""
    r = np.sqrt(dz * dz + h * h)
    knee = np.pi - np.arccos(np.clip((THIGH ** 2 + SHANK ** 2 - r * r) / (2 * THIGH * SHANK), -1, 1))
    lead = np.arccos(np.clip((THIGH ** 2 + r * r - SHANK ** 2) / (2 * THIGH * r), -1, 1))
    return -(np.arctan2(dz, h) + lead), knee


def walker():
    """The legs swing under a root that moves at constant speed along z: each foot is planted for WALK_PERIOD frames at its
    landing spot (the hip passes over it), then swings forward by two step lengths, lifted by 5 to 10 cm.  The translation also
    drifts along x, so a planted ankle slides by WALK_DRIFT per frame.  -> poses [n, 165], transl [n, 3], contact [n, 4] (1 for
    the ANKLE of the stance foot of pair (t, t + 1), else 0; the toe flags stay 0), float32, and stance [n - 1] (0 left, 1 right)."""
    n, P = WALK_N, WALK_PERIOD
    t = np.arange(n)
    root_z = WALK_STEP * t
    poses = np.zeros((n, 165))
    for foot in range(2):
        phase = (t + foot * P) % (2 * P)                             # [0, P]: stance, (P, 2 P): swing
        cycle = (t + foot * P) // (2 * P)
        stance = phase <= P
        land = WALK_STEP * (2 * P * cycle - foot * P) + WALK_STEP * P / 2
        wz = np.where(stance, land, land + 2 * WALK_STEP * (phase - P))
        lift = np.where(stance, 0.0, 0.05 + 0.05 * np.sin(np.pi * (phase - P) / P))
        hip, knee = _leg_angles(wz - root_z, WALK_HIP - lift)
        poses[:, 3 * (1 + foot)], poses[:, 3 * (4 + foot)] = hip, knee
        poses[:, 3 * (7 + foot)] = -(hip + knee)                     # the sole stays level
    transl = np.stack([WALK_DRIFT * t, np.full(n, 0.9), root_z], 1)
    which = np.where((t[:-1] % (2 * P)) < P, 0, 1)
    contact = np.zeros((n, 4), np.float32)
    contact[t[:-1], which] = 1.0
    return poses.astype(np.float32), transl.astype(np.float32), contact, which
