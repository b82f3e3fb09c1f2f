"""A NumPy restatement of the rendering pipeline from its definition (include/rg_gesture.h "SMPL-X clip rendering", DESIGN.md
"Rendering"): smplx.lbs, the pyrender PerspectiveCamera projection (yfov = pi / 3, znear = 0.05, no far plane), snapping to 8
sub-pixel bits, integer edge functions with the top-left rule, 1 / depth interpolation with the lowest face index winning ties, the
Lambert shading, the analytic checkerboard floor and the auto framing.  Every float step runs in `dtype` (float64: the reference
of the tests; float32: what the tests measure their pixel cap with); coverage is int64 in both.  Test infrastructure only."""
import numpy as np

N_JOINTS, N_BETAS, N_EXPR = 55, 300, 100
SUB = 256
COORD_MAX = 1 << 22
ZNEAR = 0.05
TAN_HALF_FOV = 0.57735026918962576451
AMBIENT = 0.35
FLOOR_HALF = 6.0
BACKGROUND = 191
GT_COLOR, PRED_COLOR = (180, 54, 54), (36, 73, 156)


# ------------------------------------------------------------------------------------------------------------- the mesh
def lbs(model, poses, betas=None, expressions=None, transl=None, dtype=np.float64):
    """smplx.lbs as SMPLX.forward calls it (see smplx_lbs.py), every array and product in `dtype` -> vertices [F, V, 3]."""
    dt = dtype
    c = lambda x: np.asarray(x, np.float64).astype(dt)
    parents = np.asarray(model["kintree_table"])[0].astype(np.int64)
    parents[0] = -1
    mean = np.zeros(165)
    mean[75:120], mean[120:165] = model["hands_meanl"], model["hands_meanr"]
    p = c(poses).reshape(-1, 165) + c(mean)
    F = p.shape[0]
    vt, sd = c(model["v_template"]), c(model["shapedirs"])
    nv = vt.shape[0]
    b = np.zeros(N_BETAS) if betas is None else np.pad(np.asarray(betas, np.float64).reshape(-1), (0, N_BETAS))[:N_BETAS]
    e = np.zeros((F, N_EXPR)) if expressions is None else np.asarray(expressions)[:F]
    coef = np.concatenate([np.broadcast_to(c(b), (F, N_BETAS)), c(e)], 1)
    v_shaped = vt[None] + (coef @ sd[..., :N_BETAS + N_EXPR].reshape(nv * 3, -1).T).reshape(F, nv, 3)
    J = np.einsum("jv,fvd->fjd", c(model["J_regressor"]), v_shaped)
    v = p.reshape(-1, 3)
    angle = np.linalg.norm(v + dt(1e-8), axis=1, keepdims=True)
    d = v / angle
    co, si = np.cos(angle)[:, :, None], np.sin(angle)[:, :, None]
    z = np.zeros_like(d[:, 0])
    K = np.stack([z, -d[:, 2], d[:, 1], d[:, 2], z, -d[:, 0], -d[:, 1], d[:, 0], z], 1).reshape(-1, 3, 3)
    R = (np.eye(3, dtype=dt)[None] + si * K + (dt(1.0) - co) * (K @ K)).reshape(F, N_JOINTS, 3, 3)
    v_posed = v_shaped + ((R[:, 1:] - np.eye(3, dtype=dt)).reshape(F, -1) @ c(model["posedirs"]).reshape(nv * 3, -1).T).reshape(F, nv, 3)
    rel = J.copy()
    rel[:, 1:] -= J[:, parents[1:]]
    T = np.zeros((F, N_JOINTS, 4, 4), dt)
    T[:, :, :3, :3], T[:, :, :3, 3], T[:, :, 3, 3] = R, rel, 1.0
    chain = [T[:, 0]]
    for i in range(1, N_JOINTS):
        chain.append(chain[parents[i]] @ T[:, i])
    G = np.stack(chain, 1)
    A = G[:, :, :3, :].copy()
    A[:, :, :, 3] -= np.einsum("fjab,fjb->fja", G[:, :, :3, :3], J)
    Tv = (c(model["weights"])[None] @ A.reshape(F, N_JOINTS, 12)).reshape(F, nv, 3, 4)
    verts = np.einsum("fvab,fvb->fva", Tv[..., :3], v_posed) + Tv[..., 3]
    if transl is not None:
        verts = verts + c(transl)[:F].reshape(F, 1, 3)
    assert verts.dtype == dt
    return verts


def active_mask(poses, tol=1e-6):
    p = np.asarray(poses)
    return np.any(np.abs(p.reshape(p.shape[0], -1)) > tol, axis=1)


def auto_framing(vertices, active=None, cam_y_offset=0.4):
    """The definition: over the active frames (all frames when none is active) floor_y = min y - 0.02; the camera, pitched by
    -8 degrees, at (mean x, (floor_y + max y) / 2 + cam_y_offset, mean z + 2).  -> (float32 [4, 4], floor_y)."""
    v = np.asarray(vertices, np.float64)
    if active is not None and np.any(active):
        v = v[np.asarray(active)]
    floor_y = v[..., 1].min() - 0.02
    a = np.deg2rad(-8.0)
    pose = np.array([[1, 0, 0, v[..., 0].mean()], [0, np.cos(a), -np.sin(a), 0.5 * (floor_y + v[..., 1].max()) + cam_y_offset],
                     [0, np.sin(a), np.cos(a), v[..., 2].mean() + 2.0], [0, 0, 0, 1]], np.float32)
    return pose, float(floor_y)


# ------------------------------------------------------------------------------------------------------------- one frame
def snap(px, dtype):
    v = np.floor(np.clip(px * dtype(SUB) + dtype(0.5), -COORD_MAX, COORD_MAX))
    return v.astype(np.int64)


def project(verts, cam, width, height, dtype=np.float64):
    """verts [V, 3] -> (screen int64 [V, 2], depth [V])."""
    dt = dtype
    cam = np.asarray(cam, np.float32).astype(dt)
    pc = (np.asarray(verts).astype(dt) - cam[:3, 3]) @ cam[:3, :3]           # R^T (p - t)
    z = -pc[:, 2]
    ok = z >= dt(ZNEAR)
    zs = np.where(ok, z, dt(1.0))
    th, aspect = dt(TAN_HALF_FOV), dt(width) / dt(height)
    sx = snap((pc[:, 0] / (zs * (aspect * th)) + dt(1.0)) * (dt(0.5) * dt(width)), dt)
    sy = snap((dt(1.0) - pc[:, 1] / (zs * th)) * (dt(0.5) * dt(height)), dt)
    screen = np.where(ok[:, None], np.stack([sx, sy], 1), 0)
    return screen, z


def vertex_normals(verts, faces, dtype=np.float64):
    """The normalised sum of cross(p1 - p0, p2 - p0) over the faces of each vertex; zero where there is none."""
    v = np.asarray(verts).astype(dtype)
    f = np.asarray(faces, np.int64)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.where(ln > 0, ln, 1), 0).astype(dtype)


def _edges(x, y, cx, cy):
    """The three edge functions (weights of v0, v1, v2 times the doubled area) at the pixel centres (cx, cy), int64, and the
    top-left biases."""
    e = []
    for a, b in ((1, 2), (2, 0), (0, 1)):
        dx, dy = int(x[b] - x[a]), int(y[b] - y[a])
        bias = 0 if ((dy == 0 and dx > 0) or dy < 0) else -1
        e.append((dx * (cy - int(y[a])) - dy * (cx - int(x[a])), bias))
    return e


def raster(screen, depth, faces, width, height, dtype=np.float64):
    """-> (face_id int64 [H, W] (-1: none), w [H, W] = the winning 1 / depth (0: none))."""
    dt = dtype
    S = np.asarray(screen, np.int64)
    z = np.asarray(depth).astype(dt)
    face_id = np.full((height, width), -1, np.int64)
    best = np.zeros((height, width), dt)
    half = SUB // 2
    for fi, (i0, i2, i1) in enumerate(np.asarray(faces, np.int64)):    # (v0, v2, v1): a front face, counter-clockwise to the
                                                                       # viewer, has a positive area on the y-down screen
        if z[i0] < dt(ZNEAR) or z[i1] < dt(ZNEAR) or z[i2] < dt(ZNEAR):
            continue
        x, y = S[[i0, i1, i2], 0], S[[i0, i1, i2], 1]
        area = int(x[1] - x[0]) * int(y[2] - y[0]) - int(y[1] - y[0]) * int(x[2] - x[0])
        if area <= 0:
            continue
        px0, px1 = max(-((-(int(x.min()) - half)) // SUB), 0), min((int(x.max()) - half) // SUB, width - 1)
        py0, py1 = max(-((-(int(y.min()) - half)) // SUB), 0), min((int(y.max()) - half) // SUB, height - 1)
        if px0 > px1 or py0 > py1:
            continue
        cx = (np.arange(px0, px1 + 1, dtype=np.int64) * SUB + half)[None, :]
        cy = (np.arange(py0, py1 + 1, dtype=np.int64) * SUB + half)[:, None]
        (e0, b0), (e1, b1), (e2, b2) = _edges(x, y, cx, cy)
        cover = (e0 + b0 >= 0) & (e1 + b1 >= 0) & (e2 + b2 >= 0)
        if not cover.any():
            continue
        inv = dt(1.0) / dt(area)
        w = (e0.astype(dt) * inv) * (dt(1.0) / z[i0]) + (e1.astype(dt) * inv) * (dt(1.0) / z[i1]) + (e2.astype(dt) * inv) * (dt(1.0) / z[i2])
        sub_best = best[py0:py1 + 1, px0:px1 + 1]
        win = cover & (w > sub_best)                       # strictly nearer: among equal depths the lowest index stays
        sub_best[win] = w[win]
        face_id[py0:py1 + 1, px0:px1 + 1][win] = fi
    return face_id, best


def resolve(face_id, w, screen, normal, faces, cam, width, height, color, floor_y=None, dtype=np.float64):
    """-> (rgb uint8 [H, W, 3], visible face_id [H, W] (-1 where the floor or the background shows), floor tile index [H, W]
    (-1: no floor)).  floor_y None: no floor."""
    dt = dtype
    cam = np.asarray(cam, np.float32).astype(dt)
    light = cam[:3, 2]
    rgb = np.full((height, width, 3), BACKGROUND, np.uint8)
    tile = np.full((height, width), -1, np.int64)
    vis = face_id.copy()
    if floor_y is not None:
        px, py = np.meshgrid(np.arange(width), np.arange(height))
        xn = (px.astype(dt) + dt(0.5)) / (dt(0.5) * dt(width)) - dt(1.0)
        yn = dt(1.0) - (py.astype(dt) + dt(0.5)) / (dt(0.5) * dt(height))
        th, aspect = dt(TAN_HALF_FOV), dt(width) / dt(height)
        cx, cy = xn * (aspect * th), yn * th
        d = [cam[k, 0] * cx + cam[k, 1] * cy - cam[k, 2] for k in range(3)]
        ok = d[1] != 0
        s = (dt(np.float32(floor_y)) - cam[1, 3]) / np.where(ok, d[1], dt(1.0))
        hx, hz = cam[0, 3] + s * d[0], cam[2, 3] + s * d[2]
        fh = dt(FLOOR_HALF)
        with np.errstate(divide="ignore"):
            hit = ok & (s > 0) & (hx >= -fh) & (hx < fh) & (hz >= -fh) & (hz < fh) & ((face_id < 0) | (dt(1.0) / np.where(s > 0, s, dt(1.0)) > w))
        ix, iz = np.floor(hx + fh).astype(np.int64), np.floor(hz + fh).astype(np.int64)
        shade = dt(AMBIENT) + (dt(1.0) - dt(AMBIENT)) * max(dt(0.0), light[1])
        col = np.where((ix + iz) % 2 == 0, dt(170.0), dt(120.0))
        val = np.floor(shade * col + dt(0.5))
        rgb[hit] = val[hit].astype(np.uint8)[:, None]
        tile[hit] = (ix * 12 + iz)[hit]
        vis[hit] = -1
    ys, xs = np.nonzero(vis >= 0)
    if len(ys):
        f = np.asarray(faces, np.int64)[vis[ys, xs]][:, [0, 2, 1]]
        S = np.asarray(screen, np.int64)
        X, Y = S[f, 0], S[f, 1]                                               # [P, 3]
        cxp, cyp = xs.astype(np.int64) * SUB + SUB // 2, ys.astype(np.int64) * SUB + SUB // 2
        e = []
        for a, b in ((1, 2), (2, 0), (0, 1)):
            e.append((X[:, b] - X[:, a]) * (cyp - Y[:, a]) - (Y[:, b] - Y[:, a]) * (cxp - X[:, a]))
        area = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
        inv = dt(1.0) / area.astype(dt)
        nrm = np.asarray(normal).astype(dt)
        n = sum((e[k].astype(dt) * inv)[:, None] * nrm[f[:, k]] for k in range(3))
        ln = np.sqrt((n * n).sum(1))
        ndl = np.where(ln > 0, np.maximum(dt(0.0), (n @ light) / np.where(ln > 0, ln, dt(1.0))), dt(0.0))
        shade = dt(AMBIENT) + (dt(1.0) - dt(AMBIENT)) * ndl
        c = np.asarray(color, np.float64).astype(dt)
        rgb[ys, xs] = np.minimum(np.floor(shade[:, None] * c[None] + dt(0.5)), dt(255.0)).astype(np.uint8)
    return rgb, vis, tile


def render_frame(verts, faces, cam, floor_y, width, height, color, active=True, dtype=np.float64):
    """One frame from world-space vertices [V, 3] -> (rgb, visible face_id, floor tile)."""
    screen, depth = project(verts, cam, width, height, dtype)
    if active:
        face_id, w = raster(screen, depth, faces, width, height, dtype)
    else:
        face_id, w = np.full((height, width), -1, np.int64), np.zeros((height, width), dtype)
    return resolve(face_id, w, screen, vertex_normals(verts, faces, dtype), faces, cam, width, height, color, floor_y, dtype)


def render_clip(model, clip, width, height, color=PRED_COLOR, cam=None, floor_y=None, dtype=np.float64, frames=None):
    """model: the raw SMPL-X dict; clip: dict(poses, transl, expressions, betas).  The framing (when not given) comes from the
    float64 vertices of the whole clip.  -> list over `frames` (default: all) of (rgb, face_id, tile)."""
    v = lbs(model, clip["poses"], clip.get("betas"), clip.get("expressions"), clip.get("transl"), dtype)
    act = active_mask(clip["poses"])
    if cam is None or floor_y is None:
        v64 = v if dtype == np.float64 else lbs(model, clip["poses"], clip.get("betas"), clip.get("expressions"), clip.get("transl"))
        cam_a, floor_a = auto_framing(v64, act)
        cam, floor_y = (cam_a if cam is None else cam), (floor_a if floor_y is None else floor_y)
    faces = np.asarray(model["f"], np.int64)
    idx = range(len(v)) if frames is None else frames
    return [render_frame(v[i], faces, cam, floor_y, width, height, color, bool(act[i]), dtype) for i in idx]


# ------------------------------------------------------------------------------------------------------------- comparing
def edge_zone(face_id, tile, faces):
    """bool [H, W]: pixels within one pixel (8-neighbourhood) of a silhouette or floor-tile edge of the reference image: a pair
    of 4-neighbours that show different kinds (mesh / floor / background), different floor tiles, or two mesh faces without a
    common vertex (an occlusion boundary inside the figure; neighbouring faces shade continuously)."""
    f = np.asarray(faces, np.int64)
    H, W = face_id.shape
    kind = np.where(face_id >= 0, 2, np.where(tile >= 0, 1, 0))
    mark = np.zeros((H, W), bool)
    for sl_a, sl_b in (((slice(None), slice(0, W - 1)), (slice(None), slice(1, W))), ((slice(0, H - 1), slice(None)), (slice(1, H), slice(None)))):
        ka, kb, fa, fb, ta, tb = kind[sl_a], kind[sl_b], face_id[sl_a], face_id[sl_b], tile[sl_a], tile[sl_b]
        diff = (ka != kb) | ((ka == 1) & (ta != tb))
        both = (ka == 2) & (kb == 2) & (fa != fb)
        if both.any():
            va, vb = f[fa[both]], f[fb[both]]
            shared = (va[:, :, None] == vb[:, None, :]).any((1, 2))
            d2 = diff.copy()
            d2[both] = ~shared
            diff = d2
        mark[sl_a] |= diff
        mark[sl_b] |= diff
    zone = mark.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            src = mark[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)]
            zone[max(0, dy):H - max(0, -dy), max(0, dx):W - max(0, -dx)] |= src
    return zone


def differing(a, b):
    """bool [H, W]: pixels of two uint8 images that differ by more than 1 LSB in some channel."""
    return (np.abs(a.astype(np.int16) - b.astype(np.int16)) > 1).any(-1)
