"""GPU: the pred-vs-retrieval panels (render.py) on the small capsule figure of tests/golden/render_fixture.py: both halves
against plain renders with the prediction's camera and floor, the hidden mesh on the retrieval's zero-pose frames, the anchor
alignment, active_anchor against a float64 reduction, and render_folder / the command line with --retrieval."""
import importlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, N = 64, 96, 5
ZERO = (0, 4)                    # the retrieval's zero-pose frames; chunk_frames = 2 puts a chunk boundary inside the clip


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rf = _load("render_fixture")
trip = lambda c: (c["poses"], c["transl"], c["expressions"])


@pytest.fixture(scope="module")
def rg():
    return importlib.import_module("rag-gesture_amd")


@pytest.fixture(scope="module")
def model():
    return rf.smplx_model()


@pytest.fixture(scope="module")
def r(rg, model):
    return rg.render.SMPLXRenderer(rg.mesh.SMPLXMesh(model), W, H, chunk_frames=2)


@pytest.fixture(scope="module")
def clips():
    pred, retr = rf.clip(31, N), rf.clip(32, N, zero_frames=ZERO)
    retr["transl"] = retr["transl"] + np.float32([0.3, 0.1, -0.2])          # the exemplar stands somewhere else
    return pred, retr


def test_halves_are_renders_with_the_prediction_camera(rg, r, clips):
    render = rg.render
    pred, retr = clips
    betas = pred["betas"]
    both = render.render_pred_retrieval_side_by_side(r, trip(pred), trip(retr), betas=betas)
    assert tuple(both.shape) == (N, H, 2 * W, 3) and both.dtype == torch.uint8 and both.is_cuda
    # (a) the left half: the prediction, blue, framed by itself
    assert torch.equal(both[:, :, :W], r.render(*trip(pred), betas, color=render.PRED_COLOR))
    # (b) the right half: the retrieval, green, with the PREDICTION's camera and floor
    cam, floor_y = r.framing(*trip(pred), betas)
    right = r.render(*trip(retr), betas, render.RETR_COLOR, cam, floor_y)
    assert torch.equal(both[:, :, W:], right)
    own_cam, own_floor = r.framing(*trip(retr), betas)
    assert np.abs(own_cam - cam).max() > 0.05                                 # (the two framings do differ)
    chunks = [c.clone() for c in render.iter_pred_retrieval_side_by_side(r, trip(pred), trip(retr), betas=betas)]
    assert [c.shape[0] for c in chunks] == [2, 2, 1] and torch.equal(torch.cat(chunks), both)
    # (c) zero-pose frames show no mesh: the colour does not matter there, and it does on the other frames
    other = r.render(*trip(retr), betas, (200, 10, 10), cam, floor_y)
    for i in range(N):
        assert torch.equal(other[i], both[i, :, W:]) == (i in ZERO), i
    img = both.cpu().numpy().astype(np.int16)
    green = (img[..., 1] > img[..., 0] + 20) & (img[..., 1] > img[..., 2] + 20)
    blue = img[..., 2] > img[..., 0] + 20
    assert not green[:, :, :W].any() and not blue[:, :, W:].any() and blue[:, :, :W].reshape(N, -1).any(1).all()
    assert green[:, :, W:].reshape(N, -1).any(1).tolist() == [i not in ZERO for i in range(N)]
    with pytest.raises(ValueError, match="pred has 5 frames, the retrieval 4"):
        render.render_pred_retrieval_side_by_side(r, trip(pred), tuple(x[:4] for x in trip(retr)))


def test_align_moves_the_retrieval_by_the_anchor_difference(rg, r, clips, model):
    render = rg.render
    pred, retr = clips
    betas = pred["betas"]
    # (e) active_anchor against a float64 reduction over the mesh's vertices
    for c in (pred, retr):
        v = r.mesh.vertices([c["poses"]], betas=[betas], expressions=[c["expressions"]], transl=[c["transl"]]).cpu().numpy().astype(np.float64)
        act = np.abs(c["poses"]).max(1) > 1e-6
        got = render.active_anchor(r, *trip(c), betas)
        assert got.dtype == np.float32
        assert np.abs(got - [v[act][..., 0].mean(), v[act][..., 1].min(), v[act][..., 2].mean()]).max() <= 1e-5
        every = render.active_anchor(r, *trip(c), betas, active_only=False)
        assert np.abs(every - [v[..., 0].mean(), v[..., 1].min(), v[..., 2].mean()]).max() <= 1e-5
    assert act.tolist() == [i not in ZERO for i in range(N)]
    assert np.abs(render.active_anchor(r, *trip(retr), betas) - render.active_anchor(r, *trip(retr), betas, active_only=False)).max() > 1e-3
    # (d) align=True is align=False with the translation shifted by the anchor difference
    delta = render.active_anchor(r, *trip(pred), betas) - render.active_anchor(r, *trip(retr), betas)
    assert delta.dtype == np.float32 and np.abs(delta).max() > 0.05
    aligned = render.render_pred_retrieval_side_by_side(r, trip(pred), trip(retr), betas=betas, align=True)
    shifted = (retr["poses"], retr["transl"] + delta, retr["expressions"])
    plain = render.render_pred_retrieval_side_by_side(r, trip(pred), shifted, betas=betas)
    assert torch.equal(aligned, plain)
    unaligned = render.render_pred_retrieval_side_by_side(r, trip(pred), trip(retr), betas=betas)
    assert torch.equal(aligned[:, :, :W], unaligned[:, :, :W]) and not torch.equal(aligned[:, :, W:], unaligned[:, :, W:])
    # after the alignment the two anchors coincide
    moved = render.active_anchor(r, *shifted, betas)
    assert np.abs(moved - render.active_anchor(r, *trip(pred), betas)).max() <= 1e-5
    # a retrieval without a translation is moved from the origin
    no_t = render.render_pred_retrieval_side_by_side(r, trip(pred), (retr["poses"], None, retr["expressions"]), betas=betas, align=True)
    d0 = render.active_anchor(r, *trip(pred), betas) - render.active_anchor(r, retr["poses"], None, retr["expressions"], betas)
    want = render.render_pred_retrieval_side_by_side(r, trip(pred), (retr["poses"], np.zeros((N, 3), np.float32) + d0, retr["expressions"]),
                                                     betas=betas)
    assert torch.equal(no_t, want)


def test_render_folder_writes_the_retrieval_panels(rg, r, model, tmp_path, capsys):
    render = rg.render
    preds, gts = [rf.clip(41, N), rf.clip(42, N)], [rf.clip(43, N), rf.clip(44, N)]
    retr = rf.clip(45, N + 2, zero_frames=(0, 1))                              # longer than the prediction: cut to N
    names = ["test/clip_a", "test/clip_b"]
    st = lambda cs, k: np.stack([c[k] for c in cs])
    exp = str(tmp_path / "exp")
    rg.packing.save_sample_files(exp, names, (st(preds, "poses"), st(preds, "expressions"), st(preds, "transl")),
                                 (st(gts, "poses"), st(gts, "expressions"), st(gts, "transl")))
    np.savez(os.path.join(exp, names[0], "retrieval_0.npz"), betas=np.zeros(300), poses=retr["poses"], expressions=retr["expressions"],
             trans=retr["transl"])
    np.savez(os.path.join(exp, names[1], "retrieval_0.npz"), betas=np.zeros(300), poses=np.zeros((N, 165), np.float32),
             expressions=np.zeros((N, 100), np.float32), trans=np.zeros((N, 3), np.float32))       # nothing retrieved
    off = render.render_folder(exp, r, png=True)
    assert set(off) == {"clips", "frames", "device_ms"} and off["clips"] == 2
    for name in names:
        assert sorted(os.listdir(os.path.join(exp, name, "gt_vs_pred"))) == ["%06d.png" % k for k in range(N)]
        assert not os.path.exists(os.path.join(exp, name, "pred_vs_retrieval"))
    on = render.render_folder(exp, r, png=True, retrieval=True)
    assert set(on) == {"clips", "frames", "device_ms", "retrieval_clips"}
    assert on["retrieval_clips"] == 1 and on["clips"] == 2 and on["frames"] == off["frames"] == 2 * N
    d = os.path.join(exp, names[0], "pred_vs_retrieval")
    assert sorted(os.listdir(d)) == ["%06d.png" % k for k in range(N)]
    assert not os.path.exists(os.path.join(exp, names[1], "pred_vs_retrieval"))
    # the files hold the panels of render_pred_retrieval_side_by_side (no betas, no alignment, as tools/visualize.py calls it)
    want = render.render_pred_retrieval_side_by_side(r, trip(preds[0]), tuple(x[:N] for x in trip(retr))).cpu().numpy()
    cpu_test = _load_sibling("test_render_cpu")
    for k in (0, 2, N - 1):
        with open(os.path.join(d, "%06d.png" % k), "rb") as f:
            assert np.array_equal(cpu_test._decode_png(f.read()), want[k]), k
    # the command line
    np.savez(str(tmp_path / "model.npz"), **model)
    argv = [exp, "--smplx_path", str(tmp_path / "model.npz"), "--png", "--width", str(W), "--height", str(H), "--chunk_frames", "2"]
    assert render.main(argv) == 0
    assert set(json.loads(capsys.readouterr().out.strip().splitlines()[-1])) == {"clips", "frames", "device_ms"}
    assert render.main(argv + ["--retrieval"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["retrieval_clips"] == 1


def _load_sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod
