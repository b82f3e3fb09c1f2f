"""GPU: the three entry points that run the forward kinematics of csrc/rg_smplx.h -- rg_smplx_joints, rg_smplx_joints_expr and
rg_mesh_transforms -- give the same joints bit for bit, clip by clip as in a batch, and refuse the same bad tables with the
texts they have always had."""
import copy
import ctypes
import importlib
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("face_fixture", os.path.join(HERE, "golden", "face_fixture.py"))
ff = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ff)

LENS = [1, 6, 2]          # 9 frames: three workgroups of four waves, the last with one live wave


@pytest.fixture(scope="module")
def rg():
    return importlib.import_module("rag-gesture_amd")


@pytest.fixture(scope="module")
def model():
    m = ff.smplx_model()                                  # the small model; its hand means are not zero
    assert np.any(m["hands_meanl"]) and np.any(m["hands_meanr"])
    return m


@pytest.fixture(scope="module")
def sm(rg, model):
    return rg.evaluation.SMPLXJoints(model)


@pytest.fixture(scope="module")
def mesh(rg, model):
    return rg.evaluation.SMPLXMesh(model)


def _random_poses(rng, n):
    """As _random_poses of test_face_metrics_gpu.py: angles near 0, near pi and beyond pi among ordinary ones."""
    aa = rng.uniform(-0.6, 0.6, (n, 165))
    dirs = rng.standard_normal((n, 55, 3))
    dirs /= np.linalg.norm(dirs, axis=2, keepdims=True)
    ang = rng.choice([1e-4, np.pi - 1e-3, np.pi + 0.3, 5.0], (n, 55, 1))
    pick = rng.random((n, 55, 1)) < 0.3
    return np.where(pick, dirs * ang, aa.reshape(n, 55, 3)).reshape(n, 165).astype(np.float32)


def _mesh_joints(mesh, clips, fold):
    j = torch.empty(sum(c.shape[0] for c in clips), 55, 3, device=mesh.device, dtype=torch.float32)
    mesh.vertices(clips, joints=j, fold=fold)
    return j


@pytest.mark.parametrize("fold", [False, True])
def test_entry_points_agree_bit_for_bit(sm, mesh, fold):
    rng = np.random.default_rng(11)
    clips = [_random_poses(rng, n) for n in LENS]
    betas = [rng.standard_normal(300) for _ in LENS]
    zeros = [np.zeros((n, 3), np.float32) for n in LENS]
    off = np.concatenate([[0], np.cumsum(LENS)])

    plain = sm.joints(clips, betas, fold=fold)                                    # rg_smplx_joints
    assert plain.shape == (9, 55, 3) and bool(torch.isfinite(plain).all())
    assert torch.equal(sm.joints(clips, betas, fold=fold, transl=zeros), plain)   # rg_smplx_joints_expr
    plain0 = sm.joints(clips, None, fold=fold)
    assert not torch.equal(plain0, plain)
    assert torch.equal(_mesh_joints(mesh, clips, fold), plain0)                   # rg_mesh_transforms

    # a clip of 0 frames between them (rows 1 .. 6 belong to the clip behind it)
    raw = torch.from_numpy(np.concatenate(clips)).to(sm.device)
    off4 = np.array([0, 1, 1, 7, 9], np.int32)
    b4 = [betas[0], rng.standard_normal(300), betas[1], betas[2]]
    assert torch.equal(sm.joints_strided(raw, None, None, off4, off4, 1, betas=b4, fold=fold), plain)

    # batch invariance: a clip alone gives its rows of the batch
    for i, c in enumerate(clips):
        rows = slice(off[i], off[i + 1])
        assert torch.equal(sm.joints([c], [betas[i]], fold=fold), plain[rows])
        assert torch.equal(sm.joints([c], [betas[i]], fold=fold, transl=[zeros[i]]), plain[rows])
        assert torch.equal(_mesh_joints(mesh, [c], fold), plain0[rows])


def _call_joints(sm, rg, parents, off):
    """rg_smplx_joints with the host tables given (the device tables stay good ones: a launch would be in bounds)."""
    off = np.ascontiguousarray(off, np.int32)
    n, dev = int(max(off)), sm.device
    poses = torch.zeros(n, 165, device=dev)
    rest = torch.zeros(len(off) - 1, 55, 3, device=dev)
    out = torch.empty(n, 55, 3, device=dev)
    off_dev = torch.from_numpy(np.sort(off) - off.min()).to(dev)
    a = rg.smplx.SmplxJointsArgs(poses=poses.data_ptr(), rest=rest.data_ptr(), pose_mean=None, parents=sm.parents_dev.data_ptr(),
                                 parents_host=parents.ctypes.data, clip_off=off_dev.data_ptr(), clip_off_host=off.ctypes.data,
                                 joints=out.data_ptr(), n_clips=len(off) - 1, fold=0)
    sm.h.call("smplx_joints", ctypes.byref(a))


def _call_expr(sm, rg, parents, off, raw_off=None, raw_rows=None):
    bad = copy.copy(sm)
    bad.parents = parents                                 # (parents_dev stays the model's)
    off = np.ascontiguousarray(off, np.int32)
    raw_off = off if raw_off is None else np.ascontiguousarray(raw_off, np.int32)
    rows = int(max(max(off), max(raw_off))) if raw_rows is None else raw_rows
    bad.joints_strided(torch.zeros(rows, 165, device=sm.device), None, None, raw_off, off, 1)


def _call_mesh(mesh, rg, parents, off):
    bad = copy.copy(mesh)
    bad.parents = parents
    off = np.ascontiguousarray(off, np.int32)
    bad._transforms(torch.zeros(int(max(off)), 165, device=mesh.device), None, [np.zeros(300)] * (len(off) - 1), off, "full", False)


# the texts of the RG_REQUIRE lines of rg_motion.hip, rg_clip.hip (check_tables) and rg_mesh.hip
ROOT = "joint 0 must be the root (parent < 0)"
RANGE = "parents[j] must lie in [0, j)"
START = {"rg_smplx_joints": "clip_off must start at 0", "rg_smplx_joints_expr": "clip_off and raw_off must start at 0",
         "rg_mesh_transforms": "clip_off must start at 0"}
DECREASE = {"rg_smplx_joints": "clip_off must not decrease", "rg_smplx_joints_expr": "clip_off and raw_off must not decrease",
            "rg_mesh_transforms": "clip_off must not decrease"}


@pytest.mark.parametrize("entry", ["rg_smplx_joints", "rg_smplx_joints_expr", "rg_mesh_transforms"])
def test_refusals_keep_their_texts(rg, sm, mesh, entry):
    call = {"rg_smplx_joints": lambda p, o: _call_joints(sm, rg, p, o), "rg_smplx_joints_expr": lambda p, o: _call_expr(sm, rg, p, o),
            "rg_mesh_transforms": lambda p, o: _call_mesh(mesh, rg, p, o)}[entry]
    good = np.ascontiguousarray(sm.parents, np.int32)
    good_off = [0, 1, 3]
    call(good, good_off)                                  # (the tables below differ from these in one entry each)

    def refused(parents, off, text, fn=call):
        with pytest.raises(rg.capi.RgError, match=re.escape("%s: %s" % (entry, text)) + "$"):
            fn(parents, off)

    rooted = good.copy()
    rooted[0] = 0
    refused(rooted, good_off, ROOT)
    for j, p in ((1, -1), (7, 7), (54, 55), (30, 31)):    # no parent; itself; past the joints; a later joint
        wrong = good.copy()
        wrong[j] = p
        refused(wrong, good_off, RANGE)
    both = rooted.copy()
    both[5] = 9
    refused(both, [1, 3], ROOT)                           # the order of the refusals: the root, the range, then the offsets
    wrong = good.copy()
    wrong[5] = 9
    refused(wrong, [1, 3], RANGE)
    refused(good, [1, 3], START[entry])
    refused(good, [0, 3, 2], DECREASE[entry])
    refused(good, [1, 3, 2], START[entry])
    if entry == "rg_smplx_joints_expr":
        refused(good, [0, 4], "raw_off ends beyond raw_rows", lambda p, o: _call_expr(sm, rg, p, o, raw_off=[0, 5], raw_rows=4))
