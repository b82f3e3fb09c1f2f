"""CPU: the rendering unit's C ABI (header, ctypes layouts, exports, zero scratch), the host side of render.py (auto framing,
PNG writer, the ffmpeg error, the vertex -> faces CSR, the model's triangle list) and the fixtures / the NumPy restatement the
GPU tests compare against (tests/golden/render_fixture.py, render_ref.py)."""
import ctypes
import importlib
import importlib.util
import os
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRY = ("rg_render_project", "rg_render_bin", "rg_render_raster")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rf, rr = _load("render_fixture"), _load("render_ref")


@pytest.fixture(scope="module")
def render(rg):
    return rg.render


def test_header_prototypes_and_struct_layouts(rg):
    syms, protos = rg.capi.header_symbols(), rg.capi.header_prototypes()
    for s in ENTRY:
        assert s in syms
        assert protos[s] == (ctypes.c_int, [ctypes.c_void_p] * 3), s
    assert rg.capi.header_version() >= 115
    consts = rg.capi.header_constants()      # (checked against the compiler in test_capi_cpu.py)
    assert [consts["RG_RENDER_" + k] for k in ("SUBPIXEL_BITS", "COORD_MAX", "TILE")] == [8, rr.COORD_MAX, 32] and rr.SUB == 1 << 8


def test_library_exports_the_entry_points(rg):
    b = importlib.import_module("rag-gesture_amd.build")
    assert os.path.join(b.CSRC, "rg_render.hip") in b.sources()
    b.build(verbose=False)
    lib = rg.capi.load_library()
    assert lib.rg_version() >= 115
    for s in ENTRY:
        fn = getattr(lib, s)
        assert fn.argtypes == [ctypes.c_void_p] * 3 and fn.restype == ctypes.c_int


def test_render_kernels_use_no_scratch_and_a_tile_of_lds(tmp_path):
    """The compiler's own resource report for every kernel of rg_render.hip, built with the product's flags: no scratch, the
    raster kernel's LDS is the 32 x 32 tile of 64-bit keys, and the 64-bit LDS maximum is one instruction (no float atomics,
    no global atomics)."""
    b = importlib.import_module("rag-gesture_amd.build")
    src = os.path.join(b.CSRC, "rg_render.hip")
    out = str(tmp_path / "render.s")
    r = subprocess.run([b._hipcc()] + b.flags_for(src) + ["--cuda-device-only", "-S", src, "-o", out,
                                                         "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"remark:\s+Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"remark:\s+LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == 3 and all("render_" in n for n in names), names
    assert scratch == [0, 0, 0], dict(zip(names, scratch))
    assert dict(zip(names, lds))[[n for n in names if "raster" in n][0]] == 32 * 32 * 8
    with open(out) as f:
        asm = f.read()
    assert "ds_max_u64" in asm or "ds_max_rtn_u64" in asm
    assert not re.search(r"\b(global|flat|buffer)_atomic", asm)
    assert not re.search(r"\bds_(add|max|min)_(rtn_)?f(32|64)\b", asm)


def test_auto_framing_on_a_hand_made_vertex_set(render):
    v = torch.tensor([[[0.0, -1.0, 0.5], [2.0, 1.0, 1.5]],              # active
                      [[10.0, -5.0, 10.0], [10.0, 5.0, 10.0]],          # inactive: must not count
                      [[1.0, -0.5, 1.0], [1.0, 0.5, 1.0]]])             # active
    act = torch.tensor([True, False, True])
    cam, floor_y = render.auto_framing(v, act)
    assert floor_y == pytest.approx(-1.02, abs=1e-7)
    c, s = np.cos(np.deg2rad(-8.0)), np.sin(np.deg2rad(-8.0))
    want = np.array([[1, 0, 0, 1.0], [0, c, -s, 0.5 * (-1.02 + 1.0) + 0.4], [0, s, c, 1.0 + 2.0], [0, 0, 0, 1]], np.float32)
    assert cam.dtype == np.float32 and cam.shape == (4, 4)
    assert np.allclose(cam, want, atol=1e-6)
    ref_cam, ref_floor = rr.auto_framing(v.numpy(), act.numpy())
    assert np.allclose(cam, ref_cam, atol=1e-6) and floor_y == pytest.approx(ref_floor, abs=1e-7)
    cam2, floor2 = render.auto_framing(v, torch.tensor([False, False, False]))       # nothing active: every frame counts
    assert floor2 == pytest.approx(-5.02, abs=1e-6) and cam2[0, 3] == pytest.approx(4.0, abs=1e-6)
    cam3, _ = render.auto_framing(v.numpy(), None, cam_y_offset=0.0)
    assert cam3[1, 3] == pytest.approx(0.5 * (-5.02 + 5.0), abs=1e-6)
    mask = render.active_frame_mask(torch.tensor([[0.0, 0.0], [0.0, 2e-6], [5e-7, 0.0]]))
    assert mask.tolist() == [False, True, False]


def _decode_png(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        pos += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, flt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + 3 * w)
    out = np.zeros((h, 3 * w), np.uint8)
    for y in range(h):                                   # un-filter (the PNG filter types 0 .. 2 on bytes, 3 bytes per pixel)
        t, row = int(raw[y, 0]), raw[y, 1:].astype(np.int64)
        assert t in (0, 1, 2)
        if t == 1:
            for x in range(3, 3 * w):
                row[x] = (row[x] + row[x - 3]) & 255
        elif t == 2 and y > 0:
            row = (row + out[y - 1]) & 255
        out[y] = row
    return out.reshape(h, w, 3)


def test_png_writer_round_trip(render, tmp_path):
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (3, 17, 23, 3), dtype=np.uint8)
    frames[1, :, :, :] = 191
    n = render.save_png_sequence(iter([torch.from_numpy(frames[:2]), frames[2:]]), str(tmp_path / "seq"))
    assert n == 3 and sorted(os.listdir(str(tmp_path / "seq"))) == ["000000.png", "000001.png", "000002.png"]
    for k in range(3):
        with open(str(tmp_path / "seq" / ("%06d.png" % k)), "rb") as f:
            assert np.array_equal(_decode_png(f.read()), frames[k])
    with pytest.raises(ValueError, match="uint8"):
        render.save_png_sequence(frames.astype(np.float32), str(tmp_path / "bad"))


def test_write_video_without_ffmpeg_names_the_png_fallback(render, tmp_path, monkeypatch):
    monkeypatch.setattr(render.shutil, "which", lambda name: None)
    frames = np.zeros((2, 4, 6, 3), np.uint8)
    with pytest.raises(render.RenderEncoderError, match="save_png_sequence"):
        render.write_video(iter([frames]), str(tmp_path / "x.mp4"), 30)
    assert not os.path.exists(str(tmp_path / "x.mp4"))
    with pytest.raises(SystemExit) as e:
        render.main([str(tmp_path), "--smplx_path", "none.npz"])
    assert e.value.code == 2


def test_vertex_face_csr_lists_each_vertex_faces_in_order(render):
    faces = np.array([[0, 1, 2], [2, 1, 3], [0, 2, 4], [4, 4, 1]])
    off, lst = render.vertex_face_csr(faces, 6)
    assert off.tolist() == [0, 2, 5, 8, 9, 12, 12]
    got = [lst[off[v]:off[v + 1]].tolist() for v in range(6)]
    assert got == [[0, 2], [0, 1, 3], [0, 1, 2], [1], [2, 3, 3], []]


def test_model_faces_are_optional_until_rendering(rg):
    m = rf.smplx_model()
    mesh = rg.mesh.load_smplx_mesh(m)
    assert mesh["faces"].dtype == np.int32 and np.array_equal(mesh["faces"], m["f"].astype(np.int32))
    no_f = {k: v for k, v in m.items() if k != "f"}
    assert rg.mesh.load_smplx_mesh(no_f)["faces"] is None            # the face metrics need no triangles
    for bad, what in ((np.zeros((4, 2), np.int64), "expected integer"), (np.full((2, 3), 389), "outside"),
                      (np.zeros((2, 3), np.float32), "expected integer")):
        with pytest.raises(rg.mesh.SMPLXModelError, match=what):
            rg.mesh.load_smplx_mesh(dict(no_f, f=bad))


def test_fixture_figure_is_closed_and_has_the_real_sizes():
    for m, nv, nf in ((rf.smplx_model(), 389, 736), (rf.full_model(), 10475, 20908)):
        f = m["f"].astype(np.int64)
        assert m["v_template"].shape == (nv, 3) and f.shape == (nf, 3)
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        key = e[:, 0] * nv + e[:, 1]
        assert len(np.unique(key)) == len(key)                          # every directed edge once ...
        assert np.array_equal(np.sort(key), np.sort(e[:, 1] * nv + e[:, 0]))   # ... and its opposite once: closed, consistent
        assert len(np.unique(f)) == nv - 1                              # one vertex belongs to no face
        assert np.allclose(m["weights"].sum(1), 1.0, atol=1e-6)


def test_reference_rules_on_tiny_cases():
    S = rr.SUB
    # two triangles sharing the diagonal of a 4 x 4 pixel square: every pixel centre belongs to exactly one of them
    sq = np.array([[0, 0], [4 * S, 0], [4 * S, 4 * S], [0, 4 * S]], np.int64)
    z = np.ones(4)
    faces = np.array([[0, 2, 1], [0, 3, 2]])                            # counter-clockwise on the (y down) screen
    fid, w = rr.raster(sq, z, faces, 6, 6)
    assert (fid[:4, :4] >= 0).all() and (fid[4:] < 0).all() and (fid[:, 4:] < 0).all()
    assert (fid[:4, :4] == 0).sum() == 10 and (fid[:4, :4] == 1).sum() == 6        # the diagonal is the upper right face's LEFT edge
    assert (rr.raster(sq, z, faces[:, [0, 2, 1]], 6, 6)[0] < 0).all()   # back faces
    # a vertex exactly on pixel centres: top-left rule (left and top edges in, right and bottom out)
    tri = np.array([[S // 2, S // 2], [S // 2, 3 * S + S // 2], [3 * S + S // 2, S // 2]], np.int64)
    fid, _ = rr.raster(tri, np.ones(3), np.array([[0, 1, 2]]), 5, 5)
    assert fid[0, 0] == 0 and fid[0, 2] == 0 and fid[2, 0] == 0 and fid[0, 3] < 0 and fid[3, 0] < 0 and fid[1, 2] < 0
    # equal depth: the lowest index wins; nearer wins whatever the index
    both = np.array([[0, 1, 2], [0, 1, 2]])
    assert set(np.unique(rr.raster(tri, np.ones(3), both, 5, 5)[0])) == {-1, 0}
    tri2 = np.concatenate([tri, tri])
    fid, _ = rr.raster(tri2, np.array([2.0, 2, 2, 1, 1, 1]), np.array([[0, 1, 2], [3, 4, 5]]), 5, 5)
    assert set(np.unique(fid)) == {-1, 1}
    # behind znear: dropped
    assert (rr.raster(tri, np.array([1.0, 0.04, 1.0]), np.array([[0, 1, 2]]), 5, 5)[0] < 0).all()


def test_float32_reference_stays_under_the_cap_on_the_small_fixture():
    """The end-to-end GPU test allows PIXEL_CAP = 4 x the share of pixels on which this restatement in float32 and in float64
    disagree (measured over all of that test's images, constants in tests/test_render_gpu.py); here the small model's images at
    the odd size are measured again: under the cap, and every differing pixel next to an edge."""
    gpu_test = _load_test("test_render_gpu")
    m = rf.smplx_model()
    name, _, seed, n, zero, frames = gpu_test.CASES[0]
    clip = rf.clip(seed, n, zero)
    a = rr.render_clip(m, clip, 333, 517, frames=frames)
    b = rr.render_clip(m, clip, 333, 517, dtype=np.float32, frames=frames)
    diff = total = 0
    for (ia, fa, ta), (ib, _, _) in zip(a, b):
        d = rr.differing(ia, ib)
        assert not (d & ~rr.edge_zone(fa, ta, m["f"])).any()
        diff, total = diff + int(d.sum()), total + d.size
    assert gpu_test.PIXEL_CAP == pytest.approx(4 * gpu_test.FLOAT32_REFERENCE_SHARE)
    assert diff / total <= gpu_test.PIXEL_CAP
    assert (a[1][1] < 0).all() and (a[0][1] >= 0).sum() > 10000          # the inactive frame shows no mesh, the others do


def _load_test(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod
