"""Seeded inputs of the foot skating / planting tests (tests/test_foot_cpu.py, tests/test_foot_gpu.py): world joints made
directly, without forward kinematics, so that every outcome of the kernels' comparisons is well populated, and the `walker`, a
two-footed gait with a drifting translation.  Nothing here imports the product."""
import numpy as np

N_JOINTS = 55
CONTACT_JOINTS = (7, 8, 10, 11)
# no pair, one pair, the wave edge (63, 64, 65), one tile minus (150), the tile edge (256, 257), three tiles with carry (600)
LENS = (1, 2, 63, 64, 65, 150, 256, 257, 600)
FPS = 30.0


def clip(rng, n):
    """One clip of n frames -> joints [n, 55, 3], contact [n, 4], transl [n, 3], float32.
    A foot joint walks through steps that are still (exactly 0 or ~1 mm), slow (12-15 mm: above the 10 mm contact rule, below
    0.5 m/s at 30 fps) or fast (20-60 mm: above 0.5 m/s), at heights that are low (< 30 mm above its base) or lifted (80-300 mm)
    in runs; a flag is 0.75-1 or 0-0.25, set more often over still steps.  The other 51 joints hold noise."""
    joints = rng.standard_normal((n, N_JOINTS, 3)) * 0.5
    contact = np.zeros((n, 4))
    for k, j in enumerate(CONTACT_JOINTS):
        kind = rng.choice(4, n, p=(0.2, 0.2, 0.25, 0.35))                       # still 0, still ~1 mm, slow, fast
        mag = np.choose(kind, (np.zeros(n), rng.uniform(0.0005, 0.002, n), rng.uniform(0.012, 0.015, n), rng.uniform(0.02, 0.06, n)))
        ang = rng.uniform(0, 2 * np.pi, n)
        step = np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)
        xz = rng.uniform(-1, 1, 2) + np.concatenate([np.zeros((1, 2)), np.cumsum(step[:-1], 0)], 0)
        low = np.empty(n, bool)
        state = rng.random() < 0.5
        for t in range(n):
            if rng.random() < 0.2:
                state = not state
            low[t] = state
        y = rng.uniform(0.0, 0.1) + np.where(low, rng.uniform(0.0, 0.03, n), rng.uniform(0.08, 0.3, n))
        joints[:, j, 0], joints[:, j, 1], joints[:, j, 2] = xz[:, 0], y, xz[:, 1]
        flagged = rng.random(n) < np.where(kind < 2, 0.7, 0.35)
        contact[:, k] = np.where(flagged, rng.uniform(0.75, 1.0, n), rng.uniform(0.0, 0.25, n))
    transl = rng.uniform(-1, 1, 3) + np.cumsum(rng.standard_normal((n, 3)) * 0.01, 0)       # a random walk
    return joints.astype(np.float32), contact.astype(np.float32), transl.astype(np.float32)


def clips(seed=0, lens=LENS):
    """-> joints [F, 55, 3], contact [F, 4], transl [F, 3] (float32, clip after clip) and the list of lengths."""
    rng = np.random.default_rng(seed)
    parts = [clip(rng, n) for n in lens]
    return tuple(np.concatenate([p[i] for p in parts], 0) for i in range(3)) + (list(lens),)


# ---------------------------------------------------------------------------------------------------------------------- walker
WALK_N, WALK_PERIOD = 140, 20
WALK_STEP = 0.025                # m per frame forward (x): 0.75 m/s
WALK_DRIFT = 0.024               # m per frame sideways (z) added to the translation: 0.72 m/s, above the 0.5 m/s of `speed`


def walker():
    """Two feet alternate stance (WALK_PERIOD frames each) under a root that moves at constant speed along x; the translation
    also drifts along z, so the stance foot slides.  -> rel [n, 55, 3] float32 (the joints relative to the translation), transl
    [n, 3] float32 (with the drift), contact [n, 4] float32 (1 for the ANKLE of the stance foot of pair (t, t + 1), else 0:
    exactly one flagged joint per pair) and stance [n - 1] (its index k into CONTACT_JOINTS).
    The world joints are fp32(rel + transl), as the forward kinematics adds the translation.  Every coordinate stays in
    [-4, 4] with a maximum of at least 3.5 (test_foot_cpu.py's rounding argument needs both)."""
    n, P = WALK_N, WALK_PERIOD
    t = np.arange(n)
    root_x = WALK_STEP * t
    rel = np.zeros((n, N_JOINTS, 3))
    rel[:, :, 1] = np.linspace(-0.9, 0.6, N_JOINTS)[None]            # some body, never read
    for foot, (ka, kt) in enumerate(((0, 2), (1, 3))):               # left: joints 7, 10; right: 8, 11
        phase = (t + foot * P) % (2 * P)                             # [0, P]: stance, (P, 2 P): swing
        cycle = (t + foot * P) // (2 * P)
        stance = phase <= P
        # world x of the ankle: planted at its landing spot during stance, then forward by two step lengths during the swing
        land = WALK_STEP * (2 * P * cycle - foot * P) + WALK_STEP * P / 2
        wx = np.where(stance, land, land + 2 * WALK_STEP * (phase - P))
        wy = np.where(stance, 0.0, 0.10 + 0.05 * np.sin(np.pi * (phase - P) / P))     # lifted at once: never grounded in swing
        z = 0.1 if foot == 0 else -0.1
        for k, dx, dy in ((ka, 0.0, 0.08), (kt, 0.15, 0.02)):
            j = CONTACT_JOINTS[k]
            rel[:, j, 0], rel[:, j, 1], rel[:, j, 2] = wx - root_x + dx, wy + dy - 0.9, z
    transl = np.stack([root_x, np.full(n, 0.9), WALK_DRIFT * t], 1)
    which = np.where(((t[:-1]) % (2 * P)) < P, 0, 1)                 # pair (t, t + 1): left stance for t in [0, P), then right
    contact = np.zeros((n, 4), np.float32)
    contact[t[:-1], which] = 1.0
    return rel.astype(np.float32), transl.astype(np.float32), contact, which


def world(rel, transl):
    """fp32(rel + transl): the joints as the forward kinematics stores them."""
    return (rel.astype(np.float32) + transl.astype(np.float32)[:, None, :]).astype(np.float32)
