"""Float64 numpy restatement of foot skating and contact planting (this project's own: the reference has no
counterpart).  Nothing here imports the product.

p[t, k] is the world position (fp32 input, taken to float64) of foot joint CONTACT_JOINTS[k] at frame t of a clip of n frames; a
pair is (t, t + 1); flag c[t, k] belongs to pair (t, t + 1).  Parameters reach the kernels as fp32, so they are rounded to fp32
here too.  Per joint-pair:
    h[t, k] = p[t, k].y - min_t p[t, k].y          grounded: h[t, k] < H and h[t + 1, k] < H
    s = fps * sqrt(dx * dx + dz * dz)              d = sqrt((dx * dx + dy * dy) + dz * dz)            flagged: c[t, k] >= cthr
Sums per clip: [pairs, pairs with a grounded joint of s > V, grounded joint-pairs, their sum of s, flagged joint-pairs, their sum
of d, flagged joint-pairs with d >= dthr].  Planting: off[0] = 0; off[t + 1] = off[t] - mean over the flagged k of (dx, dz), or
off[t] without one; out[t] = fp32(in[t] + off[t]) in x and z, y copied.  (off starts as -0.0: numerically the 0 of the
definition, and x + -0.0 is x for every x, -0 included.)
"""
import numpy as np

CONTACT_JOINTS = (7, 8, 10, 11)
FOOT_SUMS = 7
HEIGHT, SPEED, CONTACT_FLAG, MOVE = 0.05, 0.5, 0.5, 0.01


def par(x):
    return np.float64(np.float32(x))


def _clips(lens):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return [(int(off[i]), int(off[i + 1])) for i in range(len(lens))]


def pair_terms(joints, contact=None, fps=30., height=HEIGHT, speed=SPEED, contact_threshold=CONTACT_FLAG, move_threshold=MOVE):
    """One clip: joints [n, 55, 3], contact [n, 4] or None -> dict of the per-joint-pair quantities [n - 1, 4] (h0, h1, s, d, c,
    grounded, flagged, fast, moving) and `margins`: the relative distance |value - threshold| / |threshold| of EVERY comparison
    the definition names, taken or not (heights per frame and joint; s against V, c against cthr, d against dthr per
    joint-pair)."""
    p = np.asarray(joints)[:, list(CONTACT_JOINTS), :].astype(np.float64)
    fps, H, V, cthr, dthr = par(fps), par(height), par(speed), par(contact_threshold), par(move_threshold)
    h = p[:, :, 1] - p[:, :, 1].min(axis=0, keepdims=True)
    dx, dy, dz = (p[1:, :, i] - p[:-1, :, i] for i in range(3))
    xx, yy, zz = dx * dx, dy * dy, dz * dz
    s = fps * np.sqrt(xx + zz)
    d = np.sqrt((xx + yy) + zz)
    grounded = (h[:-1] < H) & (h[1:] < H)
    fast = s > V
    margins = [np.abs(h - H).ravel() / H, np.abs(s - V).ravel() / V]
    out = dict(h0=h[:-1], h1=h[1:], s=s, d=d, dx=dx, dz=dz, grounded=grounded, fast=fast)
    if contact is not None:
        c = np.asarray(contact)[:-1].astype(np.float64)
        out.update(c=c, flagged=c >= cthr, moving=d >= dthr)
        margins += [np.abs(c - cthr).ravel() / cthr, np.abs(d - dthr).ravel() / dthr]
    out["margins"] = np.concatenate(margins)
    return out


def skate_sums(joints, lens, contact=None, **kw):
    """-> float64 [C, 7] (sums in numpy's order; the kernel's order differs by at most terms * 2^-52 relative)."""
    out = np.zeros((len(lens), FOOT_SUMS))
    for i, (a, b) in enumerate(_clips(lens)):
        q = pair_terms(joints[a:b], None if contact is None else contact[a:b], **kw)
        g = q["grounded"]
        out[i, 0] = b - a - 1
        out[i, 1] = (g & q["fast"]).any(axis=1).sum()
        out[i, 2] = g.sum()
        out[i, 3] = q["s"][g].sum()
        if contact is not None:
            f = q["flagged"]
            out[i, 4] = f.sum()
            out[i, 5] = q["d"][f].sum()
            out[i, 6] = (f & q["moving"]).sum()
    return out


def metrics(sums, flags=False):
    s = np.asarray(sums).reshape(-1, FOOT_SUMS).sum(0)
    r = lambda a, b: None if b == 0 else float(a / b)
    out = dict(skate=r(s[1], s[0]), slide=r(s[3], s[2]))
    if flags:
        out.update(contact_slide=r(s[5], s[4]), contact_moving=r(s[6], s[4]))
    return out


def offsets(joints, contact, contact_threshold=CONTACT_FLAG):
    """One clip -> off float64 [n, 2] (x, z): the definition, pair after pair."""
    p = np.asarray(joints)[:, list(CONTACT_JOINTS), :].astype(np.float64)
    c = np.asarray(contact).astype(np.float64)
    cthr = par(contact_threshold)
    n = p.shape[0]
    off = np.full((n, 2), -0.0)
    for t in range(n - 1):
        sx = sz = np.float64(0.0)
        m = 0
        for k in range(4):
            if c[t, k] >= cthr:
                sx = sx + (p[t + 1, k, 0] - p[t, k, 0])
                sz = sz + (p[t + 1, k, 2] - p[t, k, 2])
                m += 1
        e = (-(sx / m), -(sz / m)) if m else (-0.0, -0.0)
        off[t + 1] = off[t, 0] + e[0], off[t, 1] + e[1]
    return off


def plant(joints, contact, transl, lens, contact_threshold=CONTACT_FLAG):
    """-> float32 [F, 3]."""
    transl = np.asarray(transl, np.float32)
    out = transl.copy()
    for a, b in _clips(lens):
        off = offsets(joints[a:b], contact[a:b], contact_threshold)
        out[a:b, 0] = (transl[a:b, 0].astype(np.float64) + off[:, 0]).astype(np.float32)
        out[a:b, 2] = (transl[a:b, 2].astype(np.float64) + off[:, 1]).astype(np.float32)
    return out


def flagged_mean_displacement(joints, contact, lens, contact_threshold=CONTACT_FLAG):
    """Per pair with at least one flagged joint: |mean over its flagged joints of (dx, dz)|, the worse of the two -> 1-D."""
    res = []
    for a, b in _clips(lens):
        if b - a < 2:
            continue
        q = pair_terms(joints[a:b], contact[a:b], contact_threshold=contact_threshold)
        f = q["flagged"]
        m = f.sum(1)
        for comp in ("dx", "dz"):
            res.append(np.abs((q[comp] * f).sum(1)[m > 0] / m[m > 0]))
    return np.concatenate(res) if res else np.zeros(0)
