"""SMPL-X clips as pictures on the device: the videos of the reference's tools (mogen/utils/visualization.py:228-504).

    auto_framing                 compute_auto_framing: the camera pose and the floor height from a clip's vertices
    SMPLXRenderer                chunk by chunk: mesh.SMPLXMesh.vertices -> rg_render_project (screen positions in fixed point,
                                 depths, smooth normals) -> rg_render_bin (tiles per face) -> rg_render_raster (coverage, depth,
                                 shading, the analytic floor) into uint8 frames on the device
    render_gt_pred_side_by_side  GT red on the left, prediction blue on the right, one camera and floor from GT
    render_pred_retrieval_side_by_side   prediction blue on the left, the retrieved exemplar green on the right (hidden on its
                                 zero-pose frames), one camera and floor from the prediction; active_anchor places it
    save_png_sequence / write_video   PNGs with zlib alone / raw RGB piped to an ffmpeg found on the PATH
    video.write_mjpeg            (--mjpeg) Motion-JPEG AVI with the clip's sound, encoded on the device: needs no ffmpeg
    main                         python -m rag-gesture_amd.render <exp_dir> --smplx_path SMPLX_NEUTRAL_2020.npz

Geometry, coverage and depth follow the reference's camera (pyrender.PerspectiveCamera, yfov = pi / 3, znear = 0.05); the
shading is this project's own Lambert term (DESIGN.md "Rendering"), not pyrender's.  No CPU fallback.
"""
import argparse
import ctypes
import glob
import json
import math
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import torch

from . import capi, video
from .mesh import SMPLXMesh
from .smplx import IN_DIM, N_EXPR, SMPLXModelError

GT_COLOR = (180, 54, 54)
PRED_COLOR = (36, 73, 156)
RETR_COLOR = (54, 156, 73)       # visualization.py:522
CAM_PITCH_DEG = -8.0
FLOOR_MARGIN = 0.02
CAM_DISTANCE = 2.0
ACTIVE_TOL = 1e-6



class RenderEncoderError(RuntimeError):
    """No video encoder: write_video needs an ffmpeg executable on the PATH."""

RenderProjectArgs = capi.struct("rg_render_project_args")
RenderBinArgs = capi.struct("rg_render_bin_args")
RenderRasterArgs = capi.struct("rg_render_raster_args")


def vertex_face_csr(faces, n_verts):
    """faces [F, 3] -> (csr_off [V + 1], csr_face [3F]) int32: per vertex its faces, ascending (a face that names a vertex
    twice is listed twice)."""
    flat = np.asarray(faces, np.int64).reshape(-1)
    order = np.argsort(flat, kind="stable")
    off = np.zeros(n_verts + 1, np.int64)
    np.cumsum(np.bincount(flat, minlength=n_verts), out=off[1:])
    return off.astype(np.int32), (order // 3).astype(np.int32)


def active_frame_mask(poses, tol=ACTIVE_TOL):
    """visualization.py:228-237: frames whose pose has any entry above tol in magnitude.  [n, ...] tensor -> bool [n]."""
    p = torch.as_tensor(poses)
    return (p.reshape(p.shape[0], -1).abs() > tol).any(1)


class _Framing:
    """compute_auto_framing's reductions, accumulated chunk by chunk over the active frames and over all frames."""

    def __init__(self):
        self.stats = [None, None]                    # [active frames only, every frame]: (min y, max y, sum x, sum z, count)

    def add(self, vertices, active):
        v = torch.as_tensor(vertices)
        sets = (v[torch.as_tensor(active, device=v.device)] if active is not None else v[:0], v)
        for i, s in enumerate(sets):
            if s.shape[0] == 0:
                continue
            cur = (float(s[..., 1].min()), float(s[..., 1].max()), float(s[..., 0].double().sum()), float(s[..., 2].double().sum()),
                   s.shape[0] * s.shape[1])
            old = self.stats[i]
            self.stats[i] = cur if old is None else (min(old[0], cur[0]), max(old[1], cur[1]), old[2] + cur[2], old[3] + cur[3],
                                                     old[4] + cur[4])

    def result(self, cam_y_offset):
        st = self.stats[0] if self.stats[0] is not None else self.stats[1]
        if st is None:
            raise ValueError("auto_framing needs at least one frame")
        lo, hi, sx, sz, cnt = st
        floor_y = lo - FLOOR_MARGIN
        mid = 0.5 * (floor_y + hi)
        c, s = math.cos(math.radians(CAM_PITCH_DEG)), math.sin(math.radians(CAM_PITCH_DEG))
        pose = np.array([[1.0, 0.0, 0.0, sx / cnt], [0.0, c, -s, mid + cam_y_offset], [0.0, s, c, sz / cnt + CAM_DISTANCE],
                         [0.0, 0.0, 0.0, 1.0]], np.float32)
        return pose, floor_y


def auto_framing(vertices, active_mask=None, cam_y_offset=0.4):
    """visualization.py:302-336 compute_auto_framing.  vertices [n, V, 3] (a tensor on any device, or an array), active_mask
    bool [n] or None -> (camera_pose float32 [4, 4], floor_y): floor 0.02 below the lowest vertex, the camera pitched by -8
    degrees at (mean x, middle of floor and top + cam_y_offset, mean z + 2), over the active frames when there are any."""
    fr = _Framing()
    fr.add(vertices, active_mask)
    return fr.result(cam_y_offset)


def _anchor(fr, active_only=True):
    """[mean x, min y, mean z] float32 of a _Framing's active frames (of all frames when none is active, or not active_only)."""
    st = fr.stats[0] if active_only and fr.stats[0] is not None else fr.stats[1]
    if st is None:
        raise ValueError("active_anchor needs at least one frame")
    lo, _, sx, sz, cnt = st
    return np.array([sx / cnt, lo, sz / cnt], np.float32)


def vertex_anchor(vertices, active_mask=None, active_only=True):
    """visualization.py:291-299, the reduction of smplx_active_anchor: vertices [n, V, 3] (a tensor on any device, or an array),
    active_mask bool [n] or None -> float32 [mean x, min y, mean z] over the active frames when active_only and there are
    any, else over all frames."""
    fr = _Framing()
    fr.add(vertices, active_mask)
    return _anchor(fr, active_only)


def _cam16(camera_pose):
    cam = np.asarray(camera_pose, np.float32)
    if cam.shape != (4, 4) or not np.all(np.isfinite(cam)):
        raise ValueError("camera_pose must be a finite 4 x 4 matrix, got shape %s" % (cam.shape,))
    return (ctypes.c_float * 16)(*cam.reshape(-1).tolist())


class SMPLXRenderer:
    """Frames of SMPL-X clips on the device.  mesh: a mesh.SMPLXMesh whose model file holds the triangle list `f`."""

    def __init__(self, mesh, width=640, height=960, chunk_frames=32):
        if not isinstance(mesh, SMPLXMesh):
            raise ValueError("SMPLXRenderer needs a mesh.SMPLXMesh")
        if mesh.faces is None:
            raise SMPLXModelError("missing key f: rendering needs the model's triangle list")
        self.width, self.height, self.chunk = int(width), int(height), int(chunk_frames)
        if not (1 <= self.width <= 8160 and 1 <= self.height <= 8160):
            raise ValueError("width / height must lie in [1, 8160], got %d x %d" % (self.width, self.height))
        if not 1 <= self.chunk <= 65535:
            raise ValueError("chunk_frames must lie in [1, 65535], got %d" % self.chunk)
        self.mesh, self.device, self.h = mesh, mesh.device, mesh.h
        self.n_verts, self.n_faces = mesh.n_verts, int(mesh.faces.shape[0])
        if self.chunk * max(self.n_verts, self.n_faces) >= 2 ** 29:
            raise ValueError("chunk_frames * max(vertices, faces) must stay below 2^29")
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        off, lst = vertex_face_csr(mesh.faces, self.n_verts)
        self.faces, self.csr_off, self.csr_face = dev(mesh.faces), dev(off), dev(lst)
        c, V, F = self.chunk, self.n_verts, self.n_faces
        self.screen = torch.empty(c, V, 2, device=self.device, dtype=torch.int32)
        self.depth = torch.empty(c, V, device=self.device, dtype=torch.float32)
        self.normal = torch.empty(c, V, 3, device=self.device, dtype=torch.float32)
        self.box = torch.empty(c, F, device=self.device, dtype=torch.int32)

    # ------------------------------------------------------------------------------------------------------- launches
    def project(self, verts, cam):
        """rg_render_project + rg_render_bin for verts [c <= chunk_frames, V, 3] fp32 (device) into the renderer's buffers."""
        c = int(verts.shape[0])
        a = RenderProjectArgs(verts=verts.data_ptr(), faces=self.faces.data_ptr(), csr_off=self.csr_off.data_ptr(),
                              csr_face=self.csr_face.data_ptr(), screen=self.screen.data_ptr(), depth=self.depth.data_ptr(),
                              normal=self.normal.data_ptr(), cam=cam, frames=c, n_verts=self.n_verts, n_faces=self.n_faces,
                              width=self.width, height=self.height)
        self.h.call("render_project", ctypes.byref(a))
        self.bin(c)

    def bin(self, c):
        b = RenderBinArgs(screen=self.screen.data_ptr(), depth=self.depth.data_ptr(), faces=self.faces.data_ptr(),
                          box=self.box.data_ptr(), frames=c, n_verts=self.n_verts, n_faces=self.n_faces, width=self.width,
                          height=self.height)
        self.h.call("render_bin", ctypes.byref(b))

    def raster(self, c, out, cam, floor_y, color, active=None, col=0, face_id=None, draw_floor=True):
        """rg_render_raster of the renderer's buffers (c frames) into out [c, H, pitch, 3] uint8 (a contiguous device tensor)
        at column col."""
        r = RenderRasterArgs(screen=self.screen.data_ptr(), depth=self.depth.data_ptr(), normal=self.normal.data_ptr(),
                             faces=self.faces.data_ptr(), box=self.box.data_ptr(),
                             active=None if active is None else active.data_ptr(), out=out.data_ptr(),
                             face_id=None if face_id is None else face_id.data_ptr(), cam=cam, floor_y=float(floor_y),
                             color=(ctypes.c_float * 3)(*[float(x) for x in color]), draw_floor=int(bool(draw_floor)), frames=c,
                             n_verts=self.n_verts, n_faces=self.n_faces, width=self.width, height=self.height,
                             pitch=int(out.shape[2]), col=int(col))
        self.h.call("render_raster", ctypes.byref(r))

    # ------------------------------------------------------------------------------------------------------- inputs
    def _inputs(self, poses, transl, expressions, betas):
        dev = self.device
        p = torch.as_tensor(poses)
        if p.ndim != 2 or p.shape[1] != IN_DIM:
            raise ValueError("poses must be [n, %d], got %s" % (IN_DIM, tuple(p.shape)))
        n = int(p.shape[0])
        if n < 1:
            raise ValueError("poses holds no frame")
        p = p.to(dev, torch.float32).contiguous()

        def rows(x, width, what):
            if x is None:
                return None
            x = torch.as_tensor(x)
            if x.ndim != 2 or x.shape[1] != width:
                raise ValueError("%s must be [>= %d, %d], got %s" % (what, n, width, tuple(x.shape)))
            if x.shape[0] < n:
                raise ValueError("%s has %d rows, poses %d: %s is shorter than poses" % (what, x.shape[0], n, what))
            return x[:n].to(dev, torch.float32).contiguous()
        t, e = rows(transl, 3, "transl"), rows(expressions, N_EXPR, "expressions")
        b = None if betas is None else [np.asarray(betas, np.float64).reshape(-1)]
        return p, t, e, b, n

    def _chunks(self, n):
        return [(i, min(i + self.chunk, n)) for i in range(0, n, self.chunk)]

    def _vertices(self, p, t, e, b, i, j):
        return self.mesh.vertices([p[i:j]], betas=b, expressions=None if e is None else [e[i:j]],
                                  transl=None if t is None else [t[i:j]])

    def _framing(self, poses, transl, expressions, betas):
        p, t, e, b, n = self._inputs(poses, transl, expressions, betas)
        act = active_frame_mask(p)
        fr = _Framing()
        for i, j in self._chunks(n):
            fr.add(self._vertices(p, t, e, b, i, j), act[i:j])
        return fr

    def framing(self, poses, transl=None, expressions=None, betas=None, cam_y_offset=0.4):
        """auto_framing of a whole clip, chunk by chunk (the vertex buffer never holds more than chunk_frames frames)."""
        return self._framing(poses, transl, expressions, betas).result(cam_y_offset)

    def _color(self, color):
        c = [float(x) for x in tuple(color)[:3]]
        if len(c) != 3 or not all(0.0 <= x <= 255.0 for x in c):
            raise ValueError("color must be three values in [0, 255], got %r" % (color,))
        return c

    def _check_out(self, out, n, col):
        if not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.uint8 and out.ndim == 4 and out.shape[3] == 3):
            raise ValueError("out must be a uint8 device tensor [n, H, pitch, 3]")
        if not out.is_contiguous():
            raise ValueError("out must be contiguous (a non-contiguous out buffer cannot take a row pitch)")
        if out.shape[0] < n or out.shape[1] != self.height or col < 0 or col + self.width > out.shape[2]:
            raise ValueError("out is %s: it must hold %d frames of height %d and columns [%d, %d)"
                             % (tuple(out.shape), n, self.height, col, col + self.width))

    def frames(self, poses, transl=None, expressions=None, betas=None, color=PRED_COLOR, camera_pose=None, floor_y=None,
               out=None, col=0, timings=None):
        """A generator over chunks of at most chunk_frames frames: yields uint8 [c, H, W, 3] device tensors (views of `out`
        [n, H, pitch, 3] at column col when given, else a buffer that the NEXT chunk overwrites).  camera_pose / floor_y: None
        = auto_framing of this clip.  timings: a dict that receives mesh_ms / project_ms / raster_ms (device time, summed over
        the chunks) once the generator is exhausted."""
        p, t, e, b, n = self._inputs(poses, transl, expressions, betas)
        color = self._color(color)
        if out is not None:
            self._check_out(out, n, col)
        if camera_pose is None or floor_y is None:
            cam_auto, floor_auto = self.framing(p, t, e, None if b is None else b[0])
            camera_pose = cam_auto if camera_pose is None else camera_pose
            floor_y = floor_auto if floor_y is None else floor_y
        cam = _cam16(camera_pose)
        if not math.isfinite(float(floor_y)):
            raise ValueError("floor_y must be finite")
        act = active_frame_mask(p).to(torch.uint8).contiguous()
        own = None if out is not None else torch.empty(self.chunk, self.height, self.width, 3, device=self.device, dtype=torch.uint8)
        events = []
        for i, j in self._chunks(n):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if timings is not None else None
            if ev:
                ev[0].record()
            verts = self._vertices(p, t, e, b, i, j)
            if ev:
                ev[1].record()
            self.project(verts, cam)
            if ev:
                ev[2].record()
            dst, c0 = (out[i:j], col) if out is not None else (own[:j - i], 0)
            self.raster(j - i, dst, cam, floor_y, color, active=act[i:j], col=c0)
            if ev:
                ev[3].record()
                events.append(ev)
            yield dst[:, :, c0:c0 + self.width]
        if timings is not None:
            torch.cuda.synchronize(self.device)
            for k, name in enumerate(("mesh_ms", "project_ms", "raster_ms")):
                timings[name] = timings.get(name, 0.0) + sum(ev[k].elapsed_time(ev[k + 1]) for ev in events)

    def render(self, poses, transl=None, expressions=None, betas=None, color=PRED_COLOR, camera_pose=None, floor_y=None,
               out=None, col=0, timings=None):
        """-> uint8 [n, H, W, 3] on the device (out[:n, :, col:col + W] when out [>= n, H, pitch, 3] is given)."""
        n = int(torch.as_tensor(poses).shape[0])
        if out is None:
            out = torch.empty(n, self.height, self.width, 3, device=self.device, dtype=torch.uint8)
            col = 0
        for _ in self.frames(poses, transl, expressions, betas, color, camera_pose, floor_y, out, col, timings):
            pass
        return out[:n, :, col:col + self.width]


def iter_gt_pred_side_by_side(renderer, gt, pred, betas=None, timings=None):
    """visualization.py:443-504 as a generator over chunks: gt / pred = (poses, transl, expressions) of the same length; yields
    uint8 [c, H, 2W, 3] device tensors (overwritten by the next chunk), GT red in the left half, the prediction blue in the
    right half, camera and floor from GT."""
    n = int(torch.as_tensor(gt[0]).shape[0])
    if int(torch.as_tensor(pred[0]).shape[0]) != n:
        raise ValueError("gt has %d frames, pred %d" % (n, int(torch.as_tensor(pred[0]).shape[0])))
    cam, floor_y = renderer.framing(gt[0], gt[1], gt[2], betas)
    W = renderer.width
    buf = torch.empty(min(renderer.chunk, n), renderer.height, 2 * W, 3, device=renderer.device, dtype=torch.uint8)
    for i in range(0, n, renderer.chunk):
        j = min(i + renderer.chunk, n)
        cut = lambda x: None if x is None else x[i:j]
        for (po, tr, ex), color, col in ((gt, GT_COLOR, 0), (pred, PRED_COLOR, W)):
            renderer.render(po[i:j], cut(tr), cut(ex), betas, color, cam, floor_y, out=buf, col=col, timings=timings)
        yield buf[:j - i]


def render_gt_pred_side_by_side(renderer, gt, pred, betas=None, timings=None):
    """-> uint8 [n, H, 2W, 3] on the device (see iter_gt_pred_side_by_side; 300 frames of 1280 x 960 are 1.1 GB)."""
    n = int(torch.as_tensor(gt[0]).shape[0])
    out = torch.empty(n, renderer.height, 2 * renderer.width, 3, device=renderer.device, dtype=torch.uint8)
    i = 0
    for chunk in iter_gt_pred_side_by_side(renderer, gt, pred, betas, timings):
        out[i:i + chunk.shape[0]] = chunk
        i += chunk.shape[0]
    return out


def active_anchor(renderer, poses, transl=None, expressions=None, betas=None, active_only=True):
    """visualization.py:268-299 smplx_active_anchor, chunk by chunk on the device: float32 [mean x, min y, mean z] of the
    clip's vertices over its active frames (active_frame_mask); over all frames when none is active or active_only is False."""
    return _anchor(renderer._framing(poses, transl, expressions, betas), active_only)


def iter_pred_retrieval_side_by_side(renderer, pred, retr, betas=None, align=False, timings=None):
    """visualization.py:507-573 as a generator over chunks: pred / retr = (poses, transl, expressions) of the same length
    (transl / expressions may be None); yields uint8 [c, H, 2W, 3] device tensors (overwritten by the next chunk), the prediction
    blue in the left half, the retrieved exemplar green in the right half.  Both panels use the camera and the floor of the
    prediction (:534-563), and the retrieval mesh is hidden on its zero-pose frames, where the exemplar was not inserted.
    align=False draws the retrieval with its translation as it is: what tools/visualize.py:594 effectively does, because the
    subtraction of the anchor there is commented out.  align=True adds active_anchor(pred) - active_anchor(retr) to the
    retrieval's translation, which puts it at the prediction's floor level and horizontal position: what the reference's
    docstring (:526-529) describes."""
    n = int(torch.as_tensor(pred[0]).shape[0])
    if int(torch.as_tensor(retr[0]).shape[0]) != n:
        raise ValueError("pred has %d frames, the retrieval %d" % (n, int(torch.as_tensor(retr[0]).shape[0])))
    fr = renderer._framing(pred[0], pred[1], pred[2], betas)
    cam, floor_y = fr.result(0.4)
    if align:
        delta = _anchor(fr) - active_anchor(renderer, retr[0], retr[1], retr[2], betas)
        tr = torch.zeros(n, 3) if retr[1] is None else torch.as_tensor(retr[1])[:n].detach().cpu().to(torch.float32)
        retr = (retr[0], tr + torch.from_numpy(delta), retr[2])
    W = renderer.width
    buf = torch.empty(min(renderer.chunk, n), renderer.height, 2 * W, 3, device=renderer.device, dtype=torch.uint8)
    for i in range(0, n, renderer.chunk):
        j = min(i + renderer.chunk, n)
        cut = lambda x: None if x is None else x[i:j]
        for (po, tr, ex), color, col in ((pred, PRED_COLOR, 0), (retr, RETR_COLOR, W)):
            renderer.render(po[i:j], cut(tr), cut(ex), betas, color, cam, floor_y, out=buf, col=col, timings=timings)
        yield buf[:j - i]


def render_pred_retrieval_side_by_side(renderer, pred, retr, betas=None, align=False, timings=None):
    """-> uint8 [n, H, 2W, 3] on the device (see iter_pred_retrieval_side_by_side)."""
    n = int(torch.as_tensor(pred[0]).shape[0])
    out = torch.empty(n, renderer.height, 2 * renderer.width, 3, device=renderer.device, dtype=torch.uint8)
    i = 0
    for chunk in iter_pred_retrieval_side_by_side(renderer, pred, retr, betas, align, timings):
        out[i:i + chunk.shape[0]] = chunk
        i += chunk.shape[0]
    return out


# ----------------------------------------------------------------------------------------------------------- writers
def _host_frames(frames):
    """A tensor / array [n, H, W, 3] or an iterable of such chunks -> uint8 arrays [H, W, 3], one by one."""
    if torch.is_tensor(frames) or isinstance(frames, np.ndarray):
        frames = [frames]
    for chunk in frames:
        a = chunk.detach().cpu().numpy() if torch.is_tensor(chunk) else np.asarray(chunk)
        if a.ndim == 3:
            a = a[None]
        if a.ndim != 4 or a.shape[3] != 3 or a.dtype != np.uint8:
            raise ValueError("frames must be uint8 [n, H, W, 3], got %s %s" % (a.dtype, a.shape))
        for f in a:
            yield np.ascontiguousarray(f)


def encode_png(rgb, level=3):
    """uint8 [H, W, 3] -> the bytes of an 8-bit RGB PNG (filter 0 on every row; zlib is all it needs)."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w, _ = rgb.shape
    raw = np.empty((h, 1 + 3 * w), np.uint8)
    raw[:, 0] = 0
    raw[:, 1:] = rgb.reshape(h, 3 * w)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(raw.tobytes(), level)) + chunk(b"IEND", b""))


def save_png_sequence(frames, directory):
    """frames: [n, H, W, 3] uint8 or an iterable of chunks -> directory/000000.png, 000001.png, ...; returns the count."""
    os.makedirs(directory, exist_ok=True)
    k = 0
    for f in _host_frames(frames):
        with open(os.path.join(directory, "%06d.png" % k), "wb") as fh:
            fh.write(encode_png(f))
        k += 1
    return k


def write_video(frames_iter, path, fps, audio_path=None):
    """Raw RGB frames piped to ffmpeg (H.264, yuv420p, +faststart as visualization.py:111-136; with audio_path the sound is
    muxed as :71-108: aac 192k, -shortest).  Without an ffmpeg on the PATH: RenderEncoderError (use save_png_sequence)."""
    exe = shutil.which("ffmpeg")
    if exe is None:
        raise RenderEncoderError("ffmpeg not found on the PATH: cannot encode %s; write PNGs instead (save_png_sequence, "
                                 "or --png on the command line)" % path)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    proc, count = None, 0
    try:
        for f in _host_frames(frames_iter):
            if proc is None:
                h, w, _ = f.shape
                if h % 2 or w % 2:
                    raise ValueError("yuv420p needs an even width and height, got %d x %d" % (w, h))
                cmd = [exe, "-y", "-loglevel", "error", "-f", "rawvideo", "-pix_fmt", "rgb24", "-s", "%dx%d" % (w, h), "-r",
                       str(fps), "-i", "-"]
                if audio_path and os.path.exists(audio_path):
                    cmd += ["-i", audio_path, "-map", "0:v:0", "-map", "1:a:0", "-c:a", "aac", "-b:a", "192k", "-shortest"]
                else:
                    cmd += ["-an"]
                cmd += ["-c:v", "libx264", "-pix_fmt", "yuv420p", "-movflags", "+faststart", path]
                proc = subprocess.Popen(cmd, stdin=subprocess.PIPE)
            proc.stdin.write(f.tobytes())
            count += 1
    finally:
        if proc is not None:
            proc.stdin.close()
            rc = proc.wait()
    if proc is None:
        raise ValueError("no frames to encode")
    if rc != 0:
        raise RenderEncoderError("ffmpeg failed with status %d for %s" % (rc, path))
    return count


# ----------------------------------------------------------------------------------------------------------- command line
def _clip(path):
    with np.load(path, allow_pickle=False) as f:
        return f["poses"].astype(np.float32), f["trans"].astype(np.float32), f["expressions"].astype(np.float32)


def _retrieval_clip(path):
    """retrieval_0.npz (visualize.py:556-564) -> (poses, trans, expressions), trans / expressions None where the file has none;
    None when the poses are all zero (visualize.py:545: nothing was retrieved)."""
    with np.load(path, allow_pickle=False) as f:
        poses = f["poses"].astype(np.float32)
        if poses.sum() == 0:
            return None
        opt = lambda k: f[k].astype(np.float32) if k in f.files else None
        return poses, opt("trans"), opt("expressions")


def _write(it, d, stem, fps, png, encoder=None):
    audio = os.path.join(d, "gt_audio.wav")
    if encoder is not None:
        video.write_mjpeg(it, os.path.join(d, stem + ".avi"), fps, audio if os.path.exists(audio) else None, encoder=encoder)
    elif png:
        save_png_sequence(it, os.path.join(d, stem))
    else:
        write_video(it, os.path.join(d, stem + ".mp4"), fps, audio if os.path.exists(audio) else None)


def _render_retrieval(d, pred_file, renderer, fps, png, t, encoder=None):
    """pred_vs_retrieval of one clip directory (visualize.py:596-608); -> whether there was a retrieval to draw."""
    r_file = os.path.join(d, "retrieval_0.npz")
    retr = _retrieval_clip(r_file) if os.path.exists(r_file) else None
    if retr is None:
        return False
    pred = _clip(pred_file)
    n = min(pred[0].shape[0], retr[0].shape[0])
    for what, c in (("prediction", pred), ("retrieval", retr)):
        for x in c[1:]:
            if x is not None and x.shape[0] < n:
                raise ValueError("%s: the %s has %d poses but a trans / expressions array of %d rows" % (d, what, c[0].shape[0], x.shape[0]))
    cut = lambda c: tuple(None if x is None else x[:n] for x in c)
    _write(iter_pred_retrieval_side_by_side(renderer, cut(pred), cut(retr), None, timings=t), d, "pred_vs_retrieval", fps, png, encoder)
    return True


def render_folder(exp_dir, renderer, fps=30, png=False, retrieval=False, mjpeg=False, quality=90):
    """Every <exp_dir>/*/*/pred_motion.npz with a gt_motion.npz beside it (packing.save_sample_files) -> gt_vs_pred.mp4 (with
    gt_audio.wav muxed in when it is there) or gt_vs_pred/000000.png ... beside them.  -> dict(clips, frames, device_ms).
    retrieval: every clip directory whose retrieval_0.npz holds a non-zero `poses` also gets pred_vs_retrieval.mp4 or
    pred_vs_retrieval/000000.png ... (both clips cut to the shorter one), and the dict has retrieval_clips.
    mjpeg: gt_vs_pred.avi / pred_vs_retrieval.avi instead (video.write_mjpeg: Motion-JPEG of the given quality encoded on the
    device, gt_audio.wav as PCM), whatever png says, and the dict has encode_ms, the encoder's device time."""
    clips = frames = retrieval_clips = 0
    t = {}
    encoder = video.JPEGEncoder(renderer.device, quality, timed=True) if mjpeg else None
    for pred_file in sorted(glob.glob(os.path.join(exp_dir, "*", "*", "pred_motion.npz"))):
        d = os.path.dirname(pred_file)
        if retrieval:
            retrieval_clips += _render_retrieval(d, pred_file, renderer, fps, png, t, encoder)
        gt_file = os.path.join(d, "gt_motion.npz")
        if not os.path.exists(gt_file):
            continue
        gt, pred = _clip(gt_file), _clip(pred_file)
        n = min(gt[0].shape[0], pred[0].shape[0])
        for what, c in (("ground truth", gt), ("prediction", pred)):
            if c[1].shape[0] < c[0].shape[0] or c[2].shape[0] < c[0].shape[0]:
                raise ValueError("%s: the %s has %d poses but %d trans / %d expressions rows"
                                 % (d, what, c[0].shape[0], c[1].shape[0], c[2].shape[0]))
        gt, pred = tuple(x[:n] for x in gt), tuple(x[:n] for x in pred)
        _write(iter_gt_pred_side_by_side(renderer, gt, pred, None, timings=t), d, "gt_vs_pred", fps, png, encoder)
        clips, frames = clips + 1, frames + n
    out = dict(clips=clips, frames=frames, device_ms=sum(t.values()))
    if retrieval:
        out["retrieval_clips"] = retrieval_clips
    if encoder is not None:
        out["encode_ms"] = encoder.device_ms()
    return out


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m rag-gesture_amd.render",
                                 description="GT-vs-pred (and pred-vs-retrieval) videos of the clips a visualize run wrote")
    ap.add_argument("exp_dir")
    ap.add_argument("--smplx_path", required=True, help="SMPLX_NEUTRAL_2020.npz")
    ap.add_argument("--fps", type=int, default=30)
    ap.add_argument("--png", action="store_true", help="write gt_vs_pred/000000.png ... instead of gt_vs_pred.mp4")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=960)
    ap.add_argument("--chunk_frames", type=int, default=32)
    ap.add_argument("--retrieval", action="store_true", help="also write pred_vs_retrieval for the clips with a retrieval_0.npz")
    ap.add_argument("--mjpeg", action="store_true", help="write gt_vs_pred.avi (Motion-JPEG encoded on the device, gt_audio.wav as PCM): needs no ffmpeg")
    ap.add_argument("--quality", type=int, default=90, help="JPEG quality of --mjpeg, 1 .. 100")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.mjpeg and args.png:
        ap.error("--mjpeg and --png exclude each other")
    if not 1 <= args.quality <= 100:
        ap.error("--quality must lie in [1, 100]")
    if not args.png and not args.mjpeg and shutil.which("ffmpeg") is None:
        ap.error("ffmpeg not found on the PATH: pass --png to write PNG sequences or --mjpeg to write Motion-JPEG AVI files instead")
    renderer = SMPLXRenderer(SMPLXMesh(args.smplx_path), args.width, args.height, args.chunk_frames)
    print(json.dumps(render_folder(args.exp_dir, renderer, args.fps, args.png, args.retrieval, args.mjpeg, args.quality)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
