"""Seeded inputs of the rendering tests: a procedural figure of ten closed capsules (torso, head, upper arms, forearms, thighs,
shins; every face counter-clockwise seen from outside) wrapped as a synthetic SMPL-X model with face_fixture.smplx_model's keys
and the triangle list `f`, smooth random clips (some frames all zero: "inactive"), and a hand-made raster scene in fixed-point
screen coordinates.  full_model() is the same figure at the real file's size: 10 475 vertices (one of them in no face) and
20 908 faces.  Used by tests/test_render_*.py; nothing here comes from the reference."""
import numpy as np

N_SHAPE = 400
POSE_FPS = 30
SMPLX_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
                 20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38,
                 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53]

# (centre, axis, radius, half length) in metres: y up, the figure looks along +z, its left is +x
PARTS = [((0.0, 0.15, 0.0), 1, 0.16, 0.22), ((0.0, 0.64, 0.0), 1, 0.11, 0.0),
         ((0.32, 0.42, 0.0), 0, 0.05, 0.10), ((-0.32, 0.42, 0.0), 0, 0.05, 0.10),
         ((0.58, 0.42, 0.0), 0, 0.04, 0.10), ((-0.58, 0.42, 0.0), 0, 0.04, 0.10),
         ((0.09, -0.32, 0.0), 1, 0.07, 0.15), ((-0.09, -0.32, 0.0), 1, 0.07, 0.15),
         ((0.09, -0.74, 0.0), 1, 0.055, 0.15), ((-0.09, -0.74, 0.0), 1, 0.055, 0.15)]
SMALL_RES = [(8, 10), (8, 8)] + [(6, 6)] * 8                    # (segments, rings + 1) per part: 388 vertices + 1
FULL_RES = [(33, 55), (32, 32)] + [(24, 41)] * 8                # 10 474 vertices + 1, 20 908 faces
# approximate joint centres of the figure (the joints without an entry sit at their parent's)
JOINTS = {0: (0.0, -0.10, 0.0), 1: (0.09, -0.15, 0.0), 2: (-0.09, -0.15, 0.0), 3: (0.0, 0.05, 0.0), 4: (0.09, -0.53, 0.0),
          5: (-0.09, -0.53, 0.0), 6: (0.0, 0.20, 0.0), 7: (0.09, -0.93, 0.0), 8: (-0.09, -0.93, 0.0), 9: (0.0, 0.35, 0.0),
          12: (0.0, 0.50, 0.0), 13: (0.10, 0.42, 0.0), 14: (-0.10, 0.42, 0.0), 15: (0.0, 0.60, 0.0), 16: (0.19, 0.42, 0.0),
          17: (-0.19, 0.42, 0.0), 18: (0.45, 0.42, 0.0), 19: (-0.45, 0.42, 0.0), 20: (0.70, 0.42, 0.0), 21: (-0.70, 0.42, 0.0),
          22: (0.0, 0.58, 0.05)}


def capsule(centre, axis, radius, half, seg, rings):
    """A closed capsule along `axis`: (vertices [seg * (rings - 1) + 2, 3], faces [2 * seg * (rings - 1), 3]), outward CCW."""
    th = np.pi * np.arange(1, rings) / rings
    ph = 2 * np.pi * np.arange(seg) / seg
    ct, st = np.cos(th)[:, None], np.sin(th)[:, None]
    along = radius * ct + half * np.sign(np.round(ct, 12))
    ring = np.stack([radius * st * np.cos(ph)[None], along + 0 * ph[None], radius * st * np.sin(ph)[None]], -1).reshape(-1, 3)
    v = np.concatenate([[[0.0, radius + half, 0.0]], ring, [[0.0, -radius - half, 0.0]]])
    idx = lambda i, j: 1 + i * seg + (j % seg)
    f = []
    for j in range(seg):
        f.append((0, idx(0, j + 1), idx(0, j)))
        for i in range(rings - 2):
            f.append((idx(i, j), idx(i, j + 1), idx(i + 1, j + 1)))
            f.append((idx(i, j), idx(i + 1, j + 1), idx(i + 1, j)))
        f.append((len(v) - 1, idx(rings - 2, j), idx(rings - 2, j + 1)))
    f = np.asarray(f, np.int64)
    if axis == 0:                                    # y axis -> x axis by a rotation (keeps the orientation)
        v = np.stack([v[:, 1], -v[:, 0], v[:, 2]], 1)
    vol = np.einsum("fi,fi->", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]]))
    assert vol > 0, "faces must be counter-clockwise seen from outside"
    return v + np.asarray(centre)[None], f


def figure(res):
    vs, fs, n = [], [], 0
    for (c, ax, r, h), (seg, rings) in zip(PARTS, res):
        v, f = capsule(c, ax, r, h, seg, rings)
        vs.append(v)
        fs.append(f + n)
        n += len(v)
    vs.append(np.array([[0.0, 0.30, 0.30]]))         # a vertex that no face uses (the real file has such vertices too)
    return np.concatenate(vs), np.concatenate(fs)


def smplx_model(seed=17, res=SMALL_RES, dirs_scale=2e-3):
    """{key: array} like face_fixture.smplx_model, for the capsule figure: J_regressor rows are means of the 6 vertices
    nearest to the joint's centre, the skinning weights a soft assignment to the 4 nearest body joints, shapedirs / posedirs
    small random directions."""
    rng = np.random.default_rng(seed)
    v, f = figure(res)
    nv = len(v)
    centres = np.zeros((55, 3))
    for j in range(55):
        k = j
        while k not in JOINTS:
            k = SMPLX_PARENTS[k]
        centres[j] = JOINTS[k]
    jr = np.zeros((55, nv))
    for j in range(55):
        near = np.argsort(np.linalg.norm(v - centres[j], axis=1), kind="stable")[:6]
        jr[j, near] = 1.0 / 6
    body = np.array(sorted(JOINTS))
    d2 = ((v[:, None] - centres[body][None]) ** 2).sum(-1)
    w = np.zeros((nv, 55))
    top = np.argsort(d2, axis=1, kind="stable")[:, :4]
    for i in range(nv):
        x = np.exp(-(d2[i, top[i]] - d2[i, top[i, 0]]) / 0.06 ** 2)
        x[x < 1e-3] = 0.0
        w[i, body[top[i]]] = x / x.sum()
    w = w.astype(np.float32)
    w /= w.sum(1, keepdims=True)
    kt = np.array([SMPLX_PARENTS, list(range(55))], dtype=np.int64)
    kt[0, 0] = 2 ** 32 - 1
    return dict(kintree_table=kt, J_regressor=jr.astype(np.float32), v_template=v.astype(np.float32),
                shapedirs=(rng.standard_normal((nv, 3, N_SHAPE)) * dirs_scale).astype(np.float32),
                posedirs=(rng.standard_normal((nv, 3, 486)) * dirs_scale).astype(np.float32), weights=w.astype(np.float32),
                hands_meanl=rng.uniform(-0.3, 0.3, 45).astype(np.float32),
                hands_meanr=rng.uniform(-0.3, 0.3, 45).astype(np.float32), f=f.astype(np.uint32))


def full_model(seed=23):
    """10 475 vertices and 20 908 faces, the sizes of SMPLX_NEUTRAL_2020.npz."""
    m = smplx_model(seed, FULL_RES, dirs_scale=5e-4)
    assert m["v_template"].shape == (10475, 3) and m["f"].shape == (20908, 3)
    return m


def smooth(rng, n, k, amp):
    t = np.arange(n)[:, None] / POSE_FPS
    out = rng.uniform(-amp, amp, (1, k))
    for _ in range(3):
        f = rng.uniform(1 / 3.0, 2.0, (1, k))
        ph = rng.uniform(0, 2 * np.pi, (1, k))
        out = out + amp / 2 * rng.uniform(0.3, 1.0, (1, k)) * np.sin(2 * np.pi * f * t + ph)
    return out.astype(np.float32)


def clip(seed, n, zero_frames=()):
    """dict(poses [n, 165], transl [n, 3], expressions [n, 100], betas [300]): smooth, moderate angles, a root turn about y;
    the frames in zero_frames have an all-zero pose."""
    rng = np.random.default_rng(seed)
    poses = smooth(rng, n, 165, 0.25)
    poses[:, :3] = 0.0
    poses[:, 1] = smooth(rng, n, 1, 0.6)[:, 0]
    poses[list(zero_frames)] = 0.0
    transl = smooth(rng, n, 3, 0.15)
    return dict(poses=poses, transl=transl, expressions=smooth(rng, n, 100, 0.5),
                betas=(rng.standard_normal(300) * 0.5).astype(np.float64))


def raster_scene(width, height, seed=5):
    """A hand-made scene in screen space for the exact raster test: dict(screen [V, 2] int32 fixed point (8 sub-pixel bits),
    depth [V] float32, normal [V, 3] float32, faces [F, 3] int32).  Random triangles of both windings, each in a depth band of its
    own (bands more than 1e-3 apart, relative); a fan of triangles that share edges and a vertex exactly on pixel centres;
    exact duplicates of some faces (the lowest index must win); slivers thinner than a pixel; triangles partly and wholly off
    screen; one with a vertex behind znear."""
    rng = np.random.default_rng(seed)
    S = 256
    verts, depth, faces = [], [], []
    band = [0]

    def add(tri_px, z=None, slope=(0.0, 0.0, 0.0)):
        """z None: the next depth band, 1.0 + 0.004 k (k < 130: neighbours differ by more than 1e-3 relative, a slope uses at
        most half a band)."""
        if z is None:
            band[0] += 1
            z = 1.0 + 0.004 * band[0] + np.asarray(slope)
        base = len(verts)
        for (x, y), zz in zip(tri_px, np.broadcast_to(z, 3)):
            verts.append((int(np.floor(x * S + 0.5)), int(np.floor(y * S + 0.5))))
            depth.append(float(zz))
        faces.append((base, base + 1, base + 2))

    for _ in range(84):                                      # random triangles, both windings, each flat at its own depth
        c = rng.uniform((0, 0), (width, height))
        add(c + rng.uniform(-0.35, 0.35, (3, 2)) * min(width, height))
    for _ in range(10):                                      # sloped depth inside the band
        c = rng.uniform((0, 0), (width, height))
        add(c + rng.uniform(-0.3, 0.3, (3, 2)) * min(width, height), slope=rng.uniform(0.0, 0.002, 3))
    cx, cy = width // 2 + 0.5, height // 2 + 0.5             # a fan around a pixel centre, vertices on pixel centres: in
    ring = [(cx + dx, cy + dy) for dx, dy in ((40, 0), (28, 28), (0, 40), (-28, 28), (-40, 0), (-28, -28), (0, -40), (28, -28))]
    for k in range(8):                                       # front of everything, its faces share edges and never overlap
        add([(cx, cy), ring[(k + 1) % 8], ring[k]], 0.6)      # (counter-clockwise on the screen: front faces)
    first_dup = len(faces)
    for k in (0, 5, 20, 87, 95):                             # exact duplicates (same vertices, later face index)
        faces.append(faces[k])
    faces.append(faces[first_dup - 1])
    for _ in range(8):                                       # slivers
        p = rng.uniform((0, 0), (width, height))
        q = p + rng.uniform(-120, 120, 2)
        add([p, q, q + rng.uniform(-0.4, 0.4, 2)])
        add([p, q + rng.uniform(-0.4, 0.4, 2), q])
    add([(-300.0, -200.0), (width + 500.0, 40.0), (-100.0, height + 400.0)], 5.0)      # huge, mostly off screen
    add([(-300.0, -200.0), (-100.0, height + 400.0), (width + 500.0, 40.0)], 5.5)      # the same, other winding
    add([(-50.0, -60.0), (-10.0, -20.0), (-40.0, -5.0)])                               # wholly off screen
    add([(width + 5.0, 10.0), (width + 50.0, 40.0), (width + 20.0, 90.0)])
    add([(10.0, 10.0), (200.0, 30.0), (60.0, 220.0)], (0.5, 0.01, 0.5))                # a vertex behind znear: dropped
    add([(10.0, 10.0), (60.0, 220.0), (200.0, 30.0)], (0.5, 0.5, 0.01))
    n = len(verts)
    normal = rng.standard_normal((n, 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    return dict(screen=np.asarray(verts, np.int32), depth=np.asarray(depth, np.float32), normal=normal.astype(np.float32),
                faces=np.asarray(faces, np.int32))
