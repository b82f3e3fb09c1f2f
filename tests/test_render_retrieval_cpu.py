"""CPU: the pred-vs-retrieval panels of rag-gesture_amd/render.py -- the anchor reduction on host tensors against a NumPy
restatement of the reference's smplx_active_anchor (active frames only, no active frame, active_only=False), the retrieval
colour, reading retrieval_0.npz, and the command-line flag."""
import importlib

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def render():
    return importlib.import_module("rag-gesture_amd").render


def _anchor(v, mask=None):
    """[mean x, min y, mean z] in float64 over the frames of mask (all when None)."""
    v = np.asarray(v, np.float64)
    if mask is not None:
        v = v[mask]
    return np.array([v[..., 0].mean(), v[..., 1].min(), v[..., 2].mean()])


def test_vertex_anchor_against_numpy(render):
    rng = np.random.default_rng(3)
    v = (rng.standard_normal((7, 29, 3)) + np.array([0.4, -1.0, 2.0])).astype(np.float32)
    v[2, 5, 1] = -9.0                                   # the lowest vertex sits in an inactive frame
    mask = np.array([True, True, False, True, False, True, True])
    for src in (v, torch.from_numpy(v)):
        got = render.vertex_anchor(src, mask if src is v else torch.from_numpy(mask))
        assert got.dtype == np.float32 and got.shape == (3,)
        assert np.abs(got - _anchor(v, mask)).max() <= 1e-6 and got[1] > -9.0
        none_active = render.vertex_anchor(src, np.zeros(7, bool))              # no active frame: every frame counts
        assert np.abs(none_active - _anchor(v)).max() <= 1e-6 and none_active[1] == -9.0
        assert np.array_equal(render.vertex_anchor(src, None), none_active)
        assert np.array_equal(render.vertex_anchor(src, mask if src is v else torch.from_numpy(mask), active_only=False), none_active)
    with pytest.raises(ValueError, match="at least one frame"):
        render.vertex_anchor(v[:0])


def test_anchor_accumulates_over_chunks_like_one_pass(render):
    """active_anchor adds a clip chunk by chunk to one _Framing: the same numbers as the clip in one piece, and the framing
    that the same accumulation gives is auto_framing's."""
    rng = np.random.default_rng(4)
    v = rng.standard_normal((9, 17, 3)).astype(np.float32)
    mask = rng.random(9) < 0.6
    fr = render._Framing()
    for i in range(0, 9, 2):
        fr.add(torch.from_numpy(v[i:i + 2]), torch.from_numpy(mask[i:i + 2]))
    assert np.abs(render._anchor(fr) - _anchor(v, mask)).max() <= 1e-6
    assert np.abs(render._anchor(fr, active_only=False) - _anchor(v)).max() <= 1e-6
    cam, floor_y = fr.result(0.4)
    cam1, floor1 = render.auto_framing(v, mask)
    assert np.abs(cam - cam1).max() <= 1e-6 and floor_y == floor1


def test_colours_and_flags(render):
    assert render.RETR_COLOR == (54, 156, 73) and render.PRED_COLOR == (36, 73, 156) and render.GT_COLOR == (180, 54, 54)
    ap = render.build_parser()
    a = ap.parse_args(["exp", "--smplx_path", "m.npz"])
    assert a.retrieval is False and a.png is False and (a.fps, a.width, a.height, a.chunk_frames) == (30, 640, 960, 32)
    assert ap.parse_args(["exp", "--smplx_path", "m.npz", "--retrieval", "--png"]).retrieval is True


def test_retrieval_file_reading(render, tmp_path):
    poses = np.zeros((4, 165), np.float32)
    np.savez(str(tmp_path / "zero.npz"), poses=poses, trans=np.zeros((4, 3)), expressions=np.zeros((4, 100)))
    assert render._retrieval_clip(str(tmp_path / "zero.npz")) is None                  # nothing was retrieved
    poses[1:3, 7] = 0.25
    np.savez(str(tmp_path / "full.npz"), poses=poses, trans=np.ones((4, 3)), expressions=np.zeros((4, 100)))
    p, t, e = render._retrieval_clip(str(tmp_path / "full.npz"))
    assert p.dtype == t.dtype == e.dtype == np.float32 and p.shape == (4, 165) and t.shape == (4, 3) and e.shape == (4, 100)
    np.savez(str(tmp_path / "poses_only.npz"), poses=poses)
    p, t, e = render._retrieval_clip(str(tmp_path / "poses_only.npz"))
    assert t is None and e is None and np.array_equal(p, poses)
