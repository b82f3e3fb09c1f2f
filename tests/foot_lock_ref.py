"""Float64 numpy restatement of the foot lock (include/rg_gesture.h; this project's own: the reference has no
counterpart).  Nothing here imports the product; the kinematics are tests/golden/smplx_fk.py's.

Legs are (hip, knee, ankle) = (1, 4, 7) and (2, 5, 8); ankle k reads contact[:, k] (the toe flags are not read).  Flag c[t]
belongs to the pair (t, t + 1); a clip's last flag is not read.
    member  m[t] = (t <= n - 2 and c[t] >= cthr) or (t >= 1 and c[t - 1] >= cthr); a run is a maximal interval [s, e] of them
    anchor  A = mean over the run of p[t] (the ankle's world position, fp32 input taken to float64)
    offset  member: d[t] = A - p[t]; else (w1 d[e] + w2 d[s']) / max(1, w1 + w2), w(k) = max(0, 1 - k / (blend + 1)), e / s' the
            member frames on either side
    solve   per frame and leg with d != 0: the two-bone solve of `solve_leg`
Parameters reach the kernels as fp32, so they are rounded to fp32 here too.  `fk32=True` rounds every transform of the forward
kinematics (each local rotation and bone, each global transform as the chain is walked, and the sum position + translation) to
fp32, which is the precision in which the kernel stores them: the distance
between the two restatements is the sensitivity of the result to that rounding (tests/test_foot_lock_gpu.py derives its
tolerance from it)."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("smplx_fk", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smplx_fk.py"))
fk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fk)

LEGS = ((1, 4, 7), (2, 5, 8))
LEG_CHANNELS = sorted(3 * j + q for leg in LEGS for j in leg for q in range(3))
LOCK_STATS = 5
CONTACT_FLAG, BLEND, STRETCH = 0.5, 3, 0.995
STRAIGHT, ON_LINE = 1e-5, 1e-12                  # the fallbacks' thresholds (relative |cross product|)


def par(x):
    return np.float64(np.float32(x))


def _clips(lens):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return [(int(off[i]), int(off[i + 1])) for i in range(len(lens))]


# ------------------------------------------------------------------------------------------------------------------ targets
def members(c, contact_threshold=CONTACT_FLAG):
    """One ankle's flags [n] -> bool [n]."""
    n = c.shape[0]
    f = np.asarray(c, np.float64) >= par(contact_threshold)
    m = np.zeros(n, bool)
    if n >= 2:
        m[:-1] |= f[:-1]
        m[1:] |= f[:-1]
    return m


def runs(m):
    """bool [n] -> the list of (s, e), both ends included."""
    out, t, n = [], 0, len(m)
    while t < n:
        if m[t]:
            s = t
            while t + 1 < n and m[t + 1]:
                t += 1
            out.append((s, t))
        t += 1
    return out


def _weight(k, blend):
    return max(0.0, 1.0 - np.float64(k) / (np.float64(blend) + 1.0))


def clip_targets(joints, contact, contact_threshold=CONTACT_FLAG, blend=BLEND):
    """One clip: joints [n, 55, 3], contact [n, 4] -> offsets float64 [n, 2, 3], stats [5], and per ankle the run length that
    bounds a frame's rounding ([n, 2]: its own run's length, or the longer of its neighbours')."""
    n = joints.shape[0]
    d = np.zeros((n, 2, 3))
    span = np.zeros((n, 2))
    st = np.zeros(LOCK_STATS)
    for k in range(2):
        p = np.asarray(joints)[:, LEGS[k][2], :].astype(np.float64)
        m = members(np.asarray(contact)[:, k], contact_threshold)
        rs = runs(m)
        for s, e in rs:
            A = p[s:e + 1].sum(0) / np.float64(e - s + 1)
            d[s:e + 1, k] = A - p[s:e + 1]
            span[s:e + 1, k] = e - s + 1
        idx = np.arange(n)
        prev_end = np.maximum.accumulate(np.where(m, idx, -1))                       # the last member frame at or before t, or -1
        next_start = np.minimum.accumulate(np.where(m, idx, n)[::-1])[::-1]          # the first at or after t, or n
        run_len = dict((e, e - s + 1) for s, e in rs)
        run_len.update((s, e - s + 1) for s, e in rs)
        for t in np.flatnonzero(~m):
            e, s = int(prev_end[t]), int(next_start[t])
            w1 = _weight(t - e, blend) if e >= 0 else 0.0
            w2 = _weight(s - t, blend) if s < n else 0.0
            d1 = d[e, k] if w1 > 0 else np.zeros(3)
            d2 = d[s, k] if w2 > 0 else np.zeros(3)
            d[t, k] = (w1 * d1 + w2 * d2) / max(1.0, w1 + w2)
            if w1 > 0:
                span[t, k] = run_len[e]
            if w2 > 0:
                span[t, k] = max(span[t, k], run_len[s])
        length = np.sqrt((d[:, k, 0] ** 2 + d[:, k, 1] ** 2) + d[:, k, 2] ** 2)
        st[0] += m.sum()
        st[1] += len(rs)
        st[2] += (d[:, k] != 0).any(1).sum()
        st[3] += length[m].sum()
        st[4] = max(st[4], length[m].max() if m.any() else 0.0)
    return d, st, span


def targets(joints, contact, lens, contact_threshold=CONTACT_FLAG, blend=BLEND):
    """-> offsets float64 [F, 2, 3], stats float64 [C, 5], span [F, 2]."""
    parts = [clip_targets(joints[a:b], contact[a:b], contact_threshold, blend) for a, b in _clips(lens)]
    return np.concatenate([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.concatenate([p[2] for p in parts])


# ----------------------------------------------------------------------------------------------------------------------- IK
def transforms(poses, rest, parents, pose_mean=None, transl=None, fk32=False):
    """poses [F, 165], rest [55, 3] -> world rotations W [F, 55, 3, 3] and positions P [F, 55, 3] (with the translation),
    float64; fk32: every transform of the chain rounded to fp32, the position also after the translation is added."""
    p = np.asarray(poses, np.float64).reshape(-1, 165)
    if pose_mean is not None:
        p = p + pose_mean
    F = p.shape[0]
    R = fk.batch_rodrigues(p.reshape(-1, 3)).reshape(F, 55, 3, 3)
    J = np.asarray(rest, np.float64)
    rel = J.copy()
    rel[1:] -= J[parents[1:]]
    r32 = (lambda x: x.astype(np.float32).astype(np.float64)) if fk32 else (lambda x: x)
    R, rel = r32(R), r32(rel)
    W, P = [R[:, 0]], [np.broadcast_to(rel[0], (F, 3))]
    for i in range(1, 55):                       # (fk32: every transform of the chain is stored as fp32, as the kernel's LDS block)
        W.append(r32(W[parents[i]] @ R[:, i]))
        P.append(r32(P[parents[i]] + W[parents[i]] @ rel[i]))
    W, P = np.stack(W, 1), np.stack(P, 1)
    tr = np.zeros((F, 3)) if transl is None else np.asarray(transl, np.float64)
    return W, r32(P + tr[:, None])


def _angle(u, v):
    return np.arctan2(np.linalg.norm(np.cross(u, v)), np.dot(u, v))


def _rot(n, th):
    c, s = np.cos(th), np.sin(th)
    K = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return c * np.eye(3) + (1 - c) * np.outer(n, n) + s * K


def log_map(R):
    """Rotation matrix -> axis-angle, angle in [0, pi] (the three branches of the kernel's log_map)."""
    r = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s2, c2 = np.linalg.norm(r), np.trace(R) - 1.0
    if s2 >= 1e-9:
        return np.arctan2(s2, c2) / s2 * r
    if c2 > 0:
        return 0.5 * r
    ax = np.sqrt(np.maximum(0.0, 0.5 * (np.diag(R) + 1.0)))
    big = int(np.argmax(ax))
    for i in range(3):
        if i != big and R[big, i] + R[i, big] < 0:
            ax[i] = -ax[i]
    return np.pi * ax


def solve_leg(Wp, Wh, Wk, Wa, a, b, c, T, stretch=STRETCH):
    """World rotations of the hip's parent, hip, knee, ankle; positions of hip, knee, ankle; the ankle's target -> the three new
    local axis-angles [3, 3] (pose_mean not taken off), reach = |T - a| / (l1 + l2), and dict(straight, on_line, sin_bend: the
    relative |cross product| of the bend, sin_swing: of the swing)."""
    ab, ac, aT = b - a, c - a, T - a
    l1, l2, want = np.linalg.norm(ab), np.linalg.norm(c - b), np.linalg.norm(aT)
    dist = min(max(want, abs(l1 - l2) * (1.0 + 1e-3) + 1e-9), par(stretch) * (l1 + l2))
    A0, K0 = _angle(ac, ab), _angle(a - b, c - b)
    A1 = np.arccos(np.clip((l1 * l1 + dist * dist - l2 * l2) / (2.0 * l1 * dist), -1.0, 1.0))
    K1 = np.arccos(np.clip((l1 * l1 + l2 * l2 - dist * dist) / (2.0 * l1 * l2), -1.0, 1.0))
    n0 = np.cross(ac, ab)
    sin_bend = np.linalg.norm(n0) / (np.linalg.norm(ac) * l1)
    straight = sin_bend < STRAIGHT
    if straight:
        n0 = Wh[:, 0].copy()
    n0 = n0 / np.linalg.norm(n0)
    B0, B1 = _rot(n0, A1 - A0), _rot(n0, K1 - K0)
    n1 = np.cross(ac, aT)
    sin_swing = np.linalg.norm(n1) / (np.linalg.norm(ac) * want) if want > 0 else 0.0
    on_line = sin_swing < ON_LINE
    S = np.eye(3) if on_line else _rot(n1 / np.linalg.norm(n1), _angle(ac, aT))
    Wh2 = S @ B0 @ Wh
    Wk2 = S @ B0 @ B1 @ Wk
    aa = np.stack([log_map(Wp.T @ Wh2), log_map(Wh2.T @ Wk2), log_map(Wk2.T @ Wa)])
    return aa, want / (l1 + l2), dict(straight=straight, on_line=on_line, sin_bend=sin_bend, sin_swing=sin_swing, dist=dist,
                                           Wh2=Wh2, Wk2=Wk2)


def lock_clip(poses, transl, offsets, rest, parents, pose_mean=None, stretch=STRETCH, fk32=False):
    """One clip -> the locked poses float64 [n, 165] (the untouched channels are the input's values), reach float64 [n, 2] (0
    where nothing was solved), the list of the solves' diagnostics (t, k, dict) and the targets the solves aimed at [n, 2, 3]:
    this restatement's own ankle positions plus the offsets."""
    poses = np.asarray(poses)
    out = poses.astype(np.float64)
    n = poses.shape[0]
    W, P = transforms(poses, rest, parents, pose_mean, transl, fk32)
    reach = np.zeros((n, 2))
    aimed = P[:, [LEGS[0][2], LEGS[1][2]], :] + offsets
    info = []
    for t in range(n):
        for k, (hip, knee, ankle) in enumerate(LEGS):
            d = offsets[t, k]
            if not (d != 0).any():
                continue
            aa, reach[t, k], diag = solve_leg(W[t, parents[hip]], W[t, hip], W[t, knee], W[t, ankle], P[t, hip], P[t, knee], P[t, ankle],
                                              aimed[t, k], stretch)
            for i, j in enumerate((hip, knee, ankle)):
                out[t, 3 * j:3 * j + 3] = aa[i] - (0.0 if pose_mean is None else pose_mean[3 * j:3 * j + 3])
            info.append((t, k, diag))
    return out, reach, info, aimed


def lock(poses, transl, contact, lens, rest, parents, pose_mean=None, contact_threshold=CONTACT_FLAG, blend=BLEND, stretch=STRETCH,
         fk32=False, joints=None):
    """Concatenated clips (poses [F, 165] fp32, transl [F, 3] fp32, contact [F, 4]) with one rest [55, 3] -> dict(poses float64
    [F, 165], reach [F, 2], offsets [F, 2, 3], stats [C, 5], span [F, 2], info, joints: the fp32 world joints the targets were
    taken from, targets: the ankles' targets float64 [F, 2, 3]).  joints: the world joints to take the targets from (default:
    this restatement's own forward kinematics, rounded to fp32 as the device stores them).  aimed: the targets the solves used,
    which differ from `targets` by the fp32 rounding of the joints."""
    poses, transl = np.asarray(poses, np.float32), np.asarray(transl, np.float32)
    if joints is None:
        joints = (fk.posed_joints(poses, rest, parents, pose_mean).astype(np.float32) + transl[:, None]).astype(np.float32)
    offsets, stats, span = targets(joints, contact, lens, contact_threshold, blend)
    out, reach, info, aimed = [], [], [], []
    for a, b in _clips(lens):
        o, r, i, g = lock_clip(poses[a:b], transl[a:b], offsets[a:b], rest, parents, pose_mean, stretch, fk32)
        out.append(o)
        reach.append(r)
        aimed.append(g)
        info += [(a + t, k, d) for t, k, d in i]
    ank = joints[:, [LEGS[0][2], LEGS[1][2]], :].astype(np.float64)
    return dict(poses=np.concatenate(out), reach=np.concatenate(reach), offsets=offsets, stats=stats, span=span, info=info,
                joints=joints, targets=ank + offsets, aimed=np.concatenate(aimed))


def world_joints(poses, transl, rest, parents, pose_mean=None):
    """float64 joints with the translation."""
    return fk.posed_joints(poses, rest, parents, pose_mean) + np.asarray(transl, np.float64)[:, None]
