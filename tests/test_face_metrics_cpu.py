"""CPU: SMPL-X mesh loading for the face metrics (rag-gesture_amd/mesh.py load_smplx_mesh) and its rejections, the sparse
skinning lists, the lvel identity against the reference's formula, the golden's fixture stream
(tests/golden/face_metrics.npz, made by make_face_metrics_golden.py), the new C-ABI symbols and argument blocks, and the CLI."""
import ctypes
import importlib
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "face_metrics.npz")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ff, lbs = _load("face_fixture"), _load("smplx_lbs")


@pytest.fixture(scope="module")
def rg():
    return importlib.import_module("rag-gesture_amd")


@pytest.fixture(scope="module")
def ev(rg):
    return rg.evaluation


@pytest.fixture(scope="module")
def model():
    return ff.smplx_model()


def test_loader_accepts_fixture(ev, model, tmp_path):
    m = ev.load_smplx_mesh(model)
    V = ff.N_VERTS
    assert m["n_verts"] == V and m["v_template"].shape == (V, 3) and m["posedirs"].shape == (V, 3, 486)
    assert m["expr_dirs"].shape == (V, 3, 100) and m["shape_dirs"].shape == (V, 3, 300)
    jr = model["J_regressor"].astype(np.float64)
    assert np.allclose(m["J_expr"], np.einsum("jv,vdk->jdk", jr, model["shapedirs"][..., 300:400].astype(np.float64)),
                       rtol=0, atol=1e-15)
    assert m["max_nnz"] == int((model["weights"] != 0).sum(1).max()) and 1 <= m["max_nnz"] <= 6
    assert np.array_equal(m["pose_mean"][75:120], model["hands_meanl"].astype(np.float64))
    p = str(tmp_path / "SMPLX_NEUTRAL_2020.npz")
    np.savez(p, **model)
    m2 = ev.load_smplx_mesh(p)
    assert np.array_equal(m2["skin_w"], m["skin_w"]) and np.array_equal(m2["J_expr"], m["J_expr"])
    flat = {k: v for k, v in model.items() if not k.startswith("hands_mean")}
    assert not ev.load_smplx_mesh(flat, flat_hand_mean=True)["pose_mean"].any()


@pytest.mark.parametrize("key, value, match", [
    ("v_template", None, "missing key v_template"),
    ("shapedirs", None, "missing key shapedirs"),
    ("posedirs", None, "missing key posedirs"),
    ("weights", None, "missing key weights"),
    ("J_regressor", None, "missing key J_regressor"),
    ("kintree_table", None, "missing key kintree_table"),
    ("hands_meanl", None, "missing key hands_meanl"),
    ("shapedirs", lambda m: m["shapedirs"][..., :350], "shapedirs"),
    ("posedirs", lambda m: m["posedirs"][..., :480], "posedirs"),
    ("posedirs", lambda m: m["posedirs"].reshape(ff.N_VERTS * 3, 486), "posedirs"),
    ("weights", lambda m: m["weights"][:, :54], "weights"),
    ("weights", lambda m: m["weights"][:-1], "weights"),
    ("v_template", lambda m: m["v_template"][:, :2], "v_template"),
    ("hands_meanr", lambda m: m["hands_meanr"][:44], "hands_meanr"),
    ("posedirs", lambda m: np.where(np.arange(486) == 3, np.nan, m["posedirs"]), "posedirs holds non-finite"),
])
def test_loader_rejects(ev, model, key, value, match):
    m = dict(model)
    if value is None:
        del m[key]
    else:
        m[key] = value(model)
    with pytest.raises(ev.SMPLXModelError, match=match):
        ev.load_smplx_mesh(m)


def test_sparse_skinning_lists_reproduce_weights(ev, model):
    m = ev.load_smplx_mesh(model)
    rng = np.random.default_rng(0)
    A = rng.standard_normal((55, 12))
    w = model["weights"].astype(np.float64)
    dense = np.zeros((m["n_verts"], 12))
    for j in range(55):                               # weights @ A, summed in joint order
        dense += w[:, j:j + 1] * A[j]
    sparse = np.zeros_like(dense)
    for v in range(m["n_verts"]):
        for q in range(m["skin_n"][v]):
            sparse[v] += m["skin_w"][v, q] * A[m["skin_j"][v, q]]
    assert np.array_equal(sparse, dense)              # exact: the dropped terms are 0 * A
    assert np.array_equal(np.sort(m["skin_j"][0, :m["skin_n"][0]]), np.nonzero(model["weights"][0])[0])
    assert np.allclose(model["weights"].sum(1), 1.0, atol=1e-6)


def test_lvel_identity(model):
    m = lbs.load_model(model)
    inp = ff.inputs(5, n_clips=2, n=20)
    for i in range(2):
        rec = lbs.face_vertices(m, inp["pred"][i], inp["pred_exprs"][i], inp["betas"][i])
        tar = lbs.face_vertices(m, inp["gt"][i], inp["gt_exprs"][i], inp["betas"][i])
        a = lbs.face_scores(rec, tar)
        b = lbs.face_scores_simplified(rec, tar)
        assert a[0] == b[0]
        assert b[1] == pytest.approx(a[1], rel=1e-12)


def test_fold_keeps_the_rotation_and_crosses_pi():
    inp = ff.inputs(ff.SEED)
    jaw = np.concatenate([p[:, 66:69] for p in inp["pred"] + inp["gt"]]).astype(np.float64)
    ang = np.linalg.norm(jaw, axis=1)
    assert (ang > np.pi).any() and (ang < np.pi).any()
    f = lbs.fold(jaw)
    assert np.linalg.norm(f, axis=1).max() <= np.pi + 1e-12
    assert np.allclose(lbs.batch_rodrigues(f), lbs.batch_rodrigues(jaw), atol=1e-7)


def test_golden_fixture_regenerates(model):
    gold = np.load(GOLD)
    assert int(gold["seed"]) == ff.SEED and list(gold["clip_names"]) == ff.clip_names()
    l2, lvel = ff.restated_scores(model, ff.inputs(int(gold["seed"])))
    assert l2 == pytest.approx(float(gold["f64_l2"]), rel=1e-12)
    assert lvel == pytest.approx(float(gold["f64_lvel"]), rel=1e-12)
    for k in ("l2", "lvel"):                            # the reference (fp32 smplx outputs) agrees with float64
        assert float(gold["score_" + k]) == pytest.approx(float(gold["f64_" + k]), rel=1e-5)
    assert os.path.getsize(GOLD) <= 300 * 1024


def test_header_symbols_and_struct_layout(rg):
    mesh = rg.mesh
    syms = rg.capi.header_symbols()
    for s in ("rg_mesh_transforms", "rg_mesh_blend_skin", "rg_mesh_face_sums"):
        assert s in syms
    assert rg.capi.header_version() >= 114
    protos = rg.capi.header_prototypes()
    for s in ("rg_mesh_transforms", "rg_mesh_blend_skin", "rg_mesh_face_sums"):
        assert protos[s][1] == [ctypes.c_void_p] * 3, s
    consts = rg.capi.header_constants()      # (checked against the compiler in test_capi_cpu.py)
    assert [consts[k] for k in ("RG_MESH_RAW", "RG_MESH_VERTICES", "RG_MESH_FACE")] == [mesh.RG_MESH_RAW, mesh.RG_MESH_VERTICES, mesh.RG_MESH_FACE]


def test_face_flag_needs_smplx_path(ev, capsys):
    with pytest.raises(SystemExit) as e:
        ev.main(["some_folder", "--e_path", "x.bin", "--face"])
    assert e.value.code == 2
    assert "--face needs --smplx_path" in capsys.readouterr().err


def test_mesh_needs_a_gpu(ev, model, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(importlib.import_module("rag-gesture_amd").capi.RgError):
        ev.SMPLXMesh(model)
