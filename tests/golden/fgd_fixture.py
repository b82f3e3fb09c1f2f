"""The inputs of tests/golden/fgd_eval.npz, regenerated from seeds instead of stored (keeps the fixture small).

Only exact operations feed the stored results: PCG64 integers and doubles, integer sums, IEEE-rounded float64 arithmetic and
power-of-two scaling, so every platform regenerates the same bits; the fixture stores checksums that the tests compare.
Used by make_fgd_golden.py (with the reference) and by tests/test_fgd_*.py (without it).
"""
import numpy as np

LENGTHS = (300, 150, 64, 45, 32)
CLIPS_PER_LENGTH = 2
EVAL_N, WINDOW = 300, 32
FD_SETS = ((200, 11), (4000, 12))      # (rows, seed) of the random latent pairs
CLIP_SEED = 2024
PARAM_SEED = 1234
# parameters of a VAESKConv state dict that are drawn here; masks and pool matrices come from the model's topology
PARAM_SUFFIXES = ("residual.0.weight", "residual.0.bias", "residual.1.weight", "residual.1.bias", "shortcut.weight",
                  "shortcut.bias")


def random_latents(n, seed):
    """Two correlated [n, 240] float64 latent sets that differ by a small scale and shift."""
    rng = np.random.default_rng(seed)
    mix = rng.standard_normal((240, 240)) / np.sqrt(240.0)
    a = rng.standard_normal((n, 240)) @ mix
    b = (rng.standard_normal((n, 240)) @ mix) * 1.02 + 0.01
    return a, b


def make_clips(rng):
    """Axis-angle [n, 165] float32 clips: a smooth random walk on a 2^-10 rad grid (integer steps), some joints exactly zero
    (as scatter_parts leaves the joints no part covers), two joints per clip rotated by within 1e-3 of pi."""
    clips = []
    for n in LENGTHS * CLIPS_PER_LENGTH:
        start = rng.integers(-600, 601, (1, 55, 3))
        steps = rng.integers(-12, 13, (n, 55, 3))
        walk = np.clip(start + np.cumsum(steps, axis=0), -1500, 1500)
        aa = walk.astype(np.float64) / 1024.0
        aa[:, rng.choice(55, 6, replace=False)] = 0.0
        for j in rng.choice(55, 2, replace=False):
            axis = rng.random(3) - 0.5
            axis = axis / np.sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2])
            aa[:, j] = axis * (np.pi - 1e-3 * rng.random((n, 1)))
        clips.append(aa.reshape(n, 165).astype(np.float32))
    return clips


def clip_sets():
    rng = np.random.default_rng(CLIP_SEED)
    return {"pred": make_clips(rng), "gt": make_clips(rng)}


def encoder_params(masks, seed=PARAM_SEED):
    """{key: float32 array} for every PARAM_SUFFIXES entry of the 4 encoder layers, shaped after `masks`
    ({"encoder.layers.i.0.residual.0.mask": [c_out, c_in, 4], ...}): weights uniform in +-1/sqrt(fan in) where the mask keeps
    them (zero elsewhere, as SkeletonConv.reset_parameters leaves them), biases likewise, GroupNorm gamma = 1 + U(-0.3, 0.3),
    beta = U(-0.3, 0.3)."""
    rng = np.random.default_rng(seed)
    out = {}
    for i in range(4):
        p = "encoder.layers.%d.0." % i
        for conv in ("residual.0.", "shortcut."):
            m = np.asarray(masks[p + conv + "mask"], np.float64)
            bound = 1.0 / np.sqrt(m.reshape(m.shape[0], -1).sum(axis=1))   # per output channel: 1 / sqrt(kept inputs x taps)
            out[p + conv + "weight"] = ((rng.random(m.shape) * 2.0 - 1.0) * bound[:, None, None] * m).astype(np.float32)
            out[p + conv + "bias"] = ((rng.random(m.shape[0]) * 2.0 - 1.0) * bound).astype(np.float32)
        c_out = masks[p + "residual.0.mask"].shape[0]
        out[p + "residual.1.weight"] = (1.0 + 0.6 * (rng.random(c_out) - 0.5)).astype(np.float32)
        out[p + "residual.1.bias"] = (0.6 * (rng.random(c_out) - 0.5)).astype(np.float32)
    return out


def checksum(arrays):
    """An order-dependent float64 fingerprint of a list of arrays (to detect a changed random stream)."""
    s = 0.0
    for k, a in enumerate(arrays):
        s += (k + 1) * float(np.asarray(a, np.float64).sum())
    return s


def state_dict(gold):
    """The full encoder state dict of the fixture: stored masks and pool matrices + regenerated parameters (float32 numpy)."""
    sd = {k[3:]: gold[k] for k in gold.files if k.startswith("sd/")}
    sd.update(encoder_params(sd))
    return sd
