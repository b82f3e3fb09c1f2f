"""GPU: the rendering kernels (rg_render_project / rg_render_bin / rg_render_raster) and render.py against the NumPy restatement
tests/golden/render_ref.py in float64: exact coverage on a hand-made screen-space scene, whole clips end to end on the small and
the full-size capsule figure, the side-by-side buffer, chunking / run-to-run invariance, the command line, and the errors.

The end-to-end rule.  Coverage is integer arithmetic on positions snapped to 1 / 256 pixel, so an image can differ from the
float64 one by more than 1 LSB only where an fp32 vertex snapped to a neighbouring sub-pixel position and moved an edge across
a pixel centre.  Such pixels (a) lie within one pixel of a silhouette or floor-tile edge of the reference image and (b) are rare:
their share over a test's images is capped by PIXEL_CAP = 4 x FLOAT32_REFERENCE_SHARE, the share on which render_ref evaluated in
float32 and in float64 disagrees on the very images of test_end_to_end_matches_float64 (CASES x SIZES), measured on the CPU:
4 pixels of 3 932 805."""
import ctypes
import importlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# (name, model, clip seed, frames of the clip, all-zero frames, frames compared)
CASES = (("small", "smplx_model", 3, 6, (2,), (0, 2, 5)), ("full", "full_model", 4, 3, (), (0, 2)))
SIZES = ((640, 960), (333, 517))
FLOAT32_REFERENCE_SHARE = 4 / 3932805           # render_ref float32 vs float64 over CASES x SIZES (1.02e-6), measured on the CPU
PIXEL_CAP = 4 * FLOAT32_REFERENCE_SHARE         # the HIP kernels' operation order is not NumPy's


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rf, rr = _load("render_fixture"), _load("render_ref")


@pytest.fixture(scope="module")
def rg():
    return importlib.import_module("rag-gesture_amd")


@pytest.fixture(scope="module")
def models():
    return {"smplx_model": rf.smplx_model(), "full_model": rf.full_model()}


@pytest.fixture(scope="module")
def meshes(rg, models):
    return {k: rg.mesh.SMPLXMesh(m) for k, m in models.items()}


def _compare(got, ref, faces, what):
    """got uint8 [H, W, 3]; ref = (rgb, face_id, tile) of render_ref -> the number of pixels that differ by more than 1 LSB, all
    of which must lie in the reference image's edge zone."""
    rgb, fid, tile = ref
    d = rr.differing(got, rgb)
    outside = int((d & ~rr.edge_zone(fid, tile, faces)).sum())
    print("%s: %d of %d pixels differ by more than 1 LSB, %d of them away from an edge" % (what, int(d.sum()), d.size, outside))
    assert outside == 0, what
    return int(d.sum()), d.size


# ------------------------------------------------------------------------------------------------------------ 1. exact raster
@pytest.mark.parametrize("width,height", SIZES)
def test_raster_coverage_is_exact(rg, width, height):
    render = rg.render
    sc = rf.raster_scene(width, height)
    dev = torch.device("cuda", 0)
    h = rg.capi.get_handle(0)
    V, F = len(sc["depth"]), len(sc["faces"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    screen, depth, normal, faces = t(sc["screen"][None]), t(sc["depth"][None]), t(sc["normal"][None]), t(sc["faces"])
    box = torch.empty(1, F, device=dev, dtype=torch.int32)
    out = torch.zeros(1, height, width, 3, device=dev, dtype=torch.uint8)
    fid = torch.full((1, height, width), -7, device=dev, dtype=torch.int32)
    b = render.RenderBinArgs(screen=screen.data_ptr(), depth=depth.data_ptr(), faces=faces.data_ptr(), box=box.data_ptr(), frames=1,
                             n_verts=V, n_faces=F, width=width, height=height)
    h.call("render_bin", ctypes.byref(b))
    cam = np.eye(4, dtype=np.float32)
    color = (200.0, 150.0, 100.0)
    r = render.RenderRasterArgs(screen=screen.data_ptr(), depth=depth.data_ptr(), normal=normal.data_ptr(), faces=faces.data_ptr(),
                                box=box.data_ptr(), active=None, out=out.data_ptr(), face_id=fid.data_ptr(),
                                cam=(ctypes.c_float * 16)(*cam.reshape(-1).tolist()), floor_y=0.0,
                                color=(ctypes.c_float * 3)(*color), draw_floor=0, frames=1, n_verts=V, n_faces=F, width=width,
                                height=height, pitch=width, col=0)
    h.call("render_raster", ctypes.byref(r))
    got_id, got_rgb = fid[0].cpu().numpy().astype(np.int64), out[0].cpu().numpy()
    want_id, w = rr.raster(sc["screen"], sc["depth"], sc["faces"], width, height)
    want_rgb, _, _ = rr.resolve(want_id, w, sc["screen"], sc["normal"], sc["faces"], cam, width, height, color)
    wrong = int((got_id != want_id).sum())
    worst = int(np.abs(got_rgb.astype(np.int16) - want_rgb.astype(np.int16)).max())
    print("raster %dx%d: %d wrong face ids of %d pixels (%d covered), worst channel difference %d"
          % (width, height, wrong, want_id.size, int((want_id >= 0).sum()), worst))
    assert np.array_equal(got_id, want_id)
    assert worst <= 1
    assert (got_rgb[want_id < 0] == 191).all()
    # the scene does exercise what it is meant to
    shown = set(np.unique(want_id).tolist())
    dup = {102: 0, 103: 5, 104: 20, 105: 87, 106: 95, 107: 101}
    assert all(np.array_equal(sc["faces"][d], sc["faces"][o]) for d, o in dup.items())
    assert not shown & set(dup) and len(shown & set(dup.values())) >= 2      # the lowest index wins every tie
    assert {94, 95, 96, 97, 98, 99, 100, 101} <= shown and len(shown) > 40
    z = sc["depth"][sc["faces"]]
    assert not shown & set(np.nonzero((z < 0.05).any(1))[0].tolist())       # nothing of the faces that cross znear


# ------------------------------------------------------------------------------------------------------------ 2. end to end
def test_end_to_end_matches_float64(rg, models, meshes):
    diff = total = 0
    for name, mk, seed, n, zero, frames in CASES:
        model, clip = models[mk], rf.clip(seed, n, zero)
        for width, height in SIZES:
            r = rg.render.SMPLXRenderer(meshes[mk], width, height, chunk_frames=4)
            got = r.render(clip["poses"], clip["transl"], clip["expressions"], clip["betas"]).cpu().numpy()
            assert got.shape == (n, height, width, 3) and got.dtype == np.uint8
            cam, floor_y = r.framing(clip["poses"], clip["transl"], clip["expressions"], clip["betas"])
            v64 = rr.lbs(model, clip["poses"], clip["betas"], clip["expressions"], clip["transl"])
            ref_cam, ref_floor = rr.auto_framing(v64, rr.active_mask(clip["poses"]))
            assert np.abs(cam - ref_cam).max() <= 1e-5 and abs(floor_y - ref_floor) <= 1e-5
            # (the reference image takes the renderer's float32 camera: a last-bit difference of the camera is not the kernels')
            ref = rr.render_clip(model, clip, width, height, cam=cam, floor_y=floor_y, frames=frames)
            for i, fr in zip(frames, ref):
                d, t = _compare(got[i], fr, model["f"], "%s %dx%d frame %d" % (name, width, height, i))
                diff, total = diff + d, total + t
                if i in zero:
                    assert (fr[1] < 0).all()
                else:
                    assert (fr[1] >= 0).sum() > 0.1 * width * height / 4
    print("end to end: %d of %d pixels differ (share %.3e, cap %.3e, float32 reference %.3e)"
          % (diff, total, diff / total, PIXEL_CAP, FLOAT32_REFERENCE_SHARE))
    assert total == 3932805
    assert diff / total <= PIXEL_CAP


# ------------------------------------------------------------------------------------------------------------ 3. side by side
def test_side_by_side_is_two_renders_with_the_gt_camera(rg, meshes):
    render = rg.render
    r = render.SMPLXRenderer(meshes["smplx_model"], 333, 517, chunk_frames=3)
    gt, pred = rf.clip(8, 7, zero_frames=(1, 4)), rf.clip(9, 7, zero_frames=(4,))
    trip = lambda c: (c["poses"], c["transl"], c["expressions"])
    both = render.render_gt_pred_side_by_side(r, trip(gt), trip(pred), betas=gt["betas"])
    assert tuple(both.shape) == (7, 517, 666, 3) and both.dtype == torch.uint8 and both.is_cuda
    cam, floor_y = r.framing(*trip(gt), gt["betas"])
    left = r.render(*trip(gt), gt["betas"], render.GT_COLOR, cam, floor_y)
    right = r.render(*trip(pred), gt["betas"], render.PRED_COLOR, cam, floor_y)
    assert torch.equal(both[:, :, :333], left) and torch.equal(both[:, :, 333:], right)
    chunks = list(c.clone() for c in render.iter_gt_pred_side_by_side(r, trip(gt), trip(pred), betas=gt["betas"]))
    assert [c.shape[0] for c in chunks] == [3, 3, 1] and torch.equal(torch.cat(chunks), both)
    img = both.cpu().numpy().astype(np.int16)
    red = (img[..., 0] > img[..., 2] + 20)
    blue = (img[..., 2] > img[..., 0] + 20)
    assert red[0, :, :333].sum() > 5000 and not red[:, :, 333:].any()          # GT, red, in the left half only
    assert blue[0, :, 333:].sum() > 5000 and not blue[:, :, :333].any()
    assert not red[1].any() and not red[4].any() and not blue[4].any() and blue[1].any()      # inactive frames: no mesh pixel
    grey = (img[..., 0] == img[..., 1]) & (img[..., 1] == img[..., 2])
    assert grey[4].all() and np.array_equal(img[4, :, :333], img[4, :, 333:])  # floor and background only, the same in both


# ------------------------------------------------------------------------------------------------------------ 4. invariance
def test_chunking_and_reruns_give_identical_bytes(rg, meshes):
    clip = rf.clip(11, 33, zero_frames=(0, 13))
    args = (clip["poses"], clip["transl"], clip["expressions"], clip["betas"])
    base = None
    for chunk in (1, 7, 32):
        r = rg.render.SMPLXRenderer(meshes["smplx_model"], 200, 301, chunk_frames=chunk)
        cam, floor_y = r.framing(*args)
        out = r.render(*args, camera_pose=cam, floor_y=floor_y)
        again = r.render(*args, camera_pose=cam, floor_y=floor_y)
        assert torch.equal(out, again), chunk
        if base is None:
            base, base_cam, base_floor = out, cam, floor_y
        assert np.array_equal(cam, base_cam) and floor_y == base_floor
        assert torch.equal(out, base), chunk
    rf_full = rg.render.SMPLXRenderer(meshes["full_model"], 640, 960, chunk_frames=2)
    c = rf.clip(12, 3)
    a = rf_full.render(c["poses"], c["transl"], c["expressions"], c["betas"])
    b = torch.cat([x.clone() for x in rf_full.frames(c["poses"], c["transl"], c["expressions"], c["betas"])])
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ 5. command line
def test_command_line_writes_png_sequences(rg, models, meshes, tmp_path, capsys):
    render, model = rg.render, models["smplx_model"]
    np.savez(str(tmp_path / "model.npz"), **model)
    n = 5
    gts, preds = [rf.clip(21, n), rf.clip(22, n, zero_frames=(0,))], [rf.clip(23, n), rf.clip(24, n)]
    names = ["test/clip_a", "test/clip_b"]
    st = lambda cs, k: np.stack([c[k] for c in cs])
    rg.packing.save_sample_files(str(tmp_path / "exp"), names, (st(preds, "poses"), st(preds, "expressions"), st(preds, "transl")),
                                 (st(gts, "poses"), st(gts, "expressions"), st(gts, "transl")))
    assert render.main([str(tmp_path / "exp"), "--smplx_path", str(tmp_path / "model.npz"), "--png", "--width", "333", "--height",
                        "517", "--chunk_frames", "2"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(line) == {"clips", "frames", "device_ms"} and line["clips"] == 2 and line["frames"] == 2 * n and line["device_ms"] > 0
    cpu_test = _load_sibling("test_render_cpu")
    r = render.SMPLXRenderer(meshes["smplx_model"], 333, 517)
    diff = total = 0
    for name, gt, pred in zip(names, gts, preds):
        d = tmp_path / "exp" / name / "gt_vs_pred"
        assert sorted(os.listdir(str(d))) == ["%06d.png" % k for k in range(n)]
        cam, floor_y = r.framing(gt["poses"], gt["transl"], gt["expressions"])
        for k in (0, n - 1):
            with open(str(d / ("%06d.png" % k)), "rb") as f:
                img = cpu_test._decode_png(f.read())
            assert img.shape == (517, 666, 3)
            for half, c, color in ((img[:, :333], gt, rr.GT_COLOR), (img[:, 333:], pred, rr.PRED_COLOR)):
                ref = rr.render_clip(model, dict(c, betas=None), 333, 517, color, cam, floor_y, frames=[k])[0]
                a, b = _compare(half, ref, model["f"], "%s frame %d" % (name, k))
                diff, total = diff + a, total + b
    print("command line: %d of %d pixels differ (share %.3e, cap %.3e)" % (diff, total, diff / total, PIXEL_CAP))
    assert diff / total <= PIXEL_CAP


def _load_sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------------------ 6. errors
def test_errors_name_the_problem(rg, models, meshes):
    render = rg.render
    no_f = {k: v for k, v in models["smplx_model"].items() if k != "f"}
    mesh = rg.mesh.SMPLXMesh(no_f)
    assert mesh.faces is None and tuple(mesh.vertices([rf.clip(1, 2)["poses"]]).shape) == (2, 389, 3)   # the mesh itself works
    with pytest.raises(rg.mesh.SMPLXModelError, match="missing key f"):
        render.SMPLXRenderer(mesh)
    r = render.SMPLXRenderer(meshes["smplx_model"], 64, 96)
    clip = rf.clip(2, 6)
    with pytest.raises(ValueError, match="transl.*shorter than poses"):
        r.render(clip["poses"], clip["transl"][:4])
    with pytest.raises(ValueError, match="expressions.*shorter than poses"):
        r.render(clip["poses"], clip["transl"], clip["expressions"][:5])
    wide = torch.empty(6, 96, 128, 3, device=r.device, dtype=torch.uint8)
    with pytest.raises(ValueError, match="contiguous"):
        r.render(clip["poses"], out=wide[:, :, :64])
    with pytest.raises(ValueError, match="columns"):
        r.render(clip["poses"], out=wide, col=100)
    with pytest.raises(ValueError, match="poses must be"):
        r.render(clip["poses"][:, :100])
    with pytest.raises(ValueError, match="camera_pose"):
        r.render(clip["poses"], camera_pose=np.eye(3), floor_y=0.0)
    ok = r.render(clip["poses"], out=wide, col=64)                            # a panel inside a wider buffer is fine
    assert tuple(ok.shape) == (6, 96, 64, 3) and ok.data_ptr() == wide[:, :, 64:].data_ptr()
