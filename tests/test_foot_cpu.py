"""No GPU: foot skating and contact planting -- the header and the library's exports, the conditions the
seeded fixture must meet so that kernel and restatement decide every comparison alike, the restatement's own properties (the
walker among them), the command line's argument check, and the classes without a device.  The kernels are tested in
test_foot_gpu.py."""
import importlib.util
import os

import numpy as np
import pytest

import foot_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fx = _load("foot_fixture")


# --------------------------------------------------------------------------------------------------------------------- the ABI
def test_header_declares_the_entry_points(rg):
    capi = rg.capi
    assert {"rg_foot_skate_sums", "rg_foot_plant"} <= set(capi.header_symbols())
    assert capi.header_version() >= 134 and capi.header_constants()["RG_FOOT_SUMS"] == 7 == ref.FOOT_SUMS == rg.foot.FOOT_SUMS
    assert len(capi.header_structs()) == 23                      # plain arguments: no new argument block
    protos = capi.header_prototypes()
    assert len(protos["rg_foot_skate_sums"][1]) == 13 and len(protos["rg_foot_plant"][1]) == 10
    assert rg.foot.CONTACT_JOINTS == ref.CONTACT_JOINTS == fx.CONTACT_JOINTS == rg.dataset.CONTACT_JOINTS
    assert (rg.foot.HEIGHT, rg.foot.SPEED, rg.foot.CONTACT_FLAG, rg.dataset.CONTACT_THRESHOLD) == (ref.HEIGHT, ref.SPEED, ref.CONTACT_FLAG, ref.MOVE)


def test_library_exports_the_entry_points(rg):
    lib = rg.capi.load_library()
    assert hasattr(lib, "rg_foot_skate_sums") and hasattr(lib, "rg_foot_plant")
    assert lib.rg_version() == rg.capi.header_version()


def test_unit_is_built_with_the_default_flags(rg):
    b = importlib.import_module("rag-gesture_amd.build")
    src = os.path.join(b.CSRC, "rg_foot.hip")
    assert src in b.sources() and b.flags_for(src) == b.FLAGS and "rg_foot.hip" not in b.PACKED_FP32_UNITS
    with open(src) as f:
        assert "asm" not in f.read()


# --------------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_keeps_every_comparison_away_from_its_threshold():
    """Kernel and restatement compute a compared value in the same fp64 operations, but a test that leaned on that would
    fail for the wrong reason: no comparison of the fixture lies within a relative 1e-6 of its threshold (fp64 rounding is
    1e-16, the fp32 rounding of a parameter 6e-8), and every outcome is well populated."""
    joints, contact, transl, lens = fx.clips()
    assert tuple(lens) == (1, 2, 63, 64, 65, 150, 256, 257, 600) and joints.shape == (sum(lens), 55, 3)
    assert joints.dtype == contact.dtype == transl.dtype == np.float32
    margins, cls = [], {k: [] for k in ("grounded", "fast", "flagged", "moving", "skating")}
    a = 0
    for n in lens:
        q = ref.pair_terms(joints[a:a + n], contact[a:a + n], fps=fx.FPS)
        margins.append(q["margins"])
        cls["grounded"].append(q["grounded"].ravel())
        cls["skating"].append((q["grounded"] & q["fast"]).any(1))
        cls["flagged"].append(q["flagged"].ravel())
        cls["moving"].append(q["moving"][q["flagged"]])           # flagged-moving / flagged-still
        a += n
    margins = np.concatenate(margins)
    close = int((margins < 1e-6).sum())
    print("comparisons %d, within 1e-6 of a threshold %d, smallest margin %.3e" % (margins.size, close, margins.min()))
    assert margins.size > 20000 and close == 0
    for name in ("grounded", "skating", "flagged", "moving"):
        share = float(np.concatenate(cls[name]).mean())
        print("%s: %.3f" % (name, share))
        assert 0.1 <= share <= 0.9, (name, share)
    assert np.abs(contact - 0.5).min() >= 0.25                   # flags well away from 0.5


# --------------------------------------------------------------------------------------------- the restatement's properties
def test_restatement_without_flags_is_the_identity():
    joints, contact, transl, lens = fx.clips(1)
    transl[3, 0], transl[7, 2] = -0.0, -0.0                        # (x + -0.0 keeps the sign of a zero)
    out = ref.plant(joints, np.zeros_like(contact), transl, lens)
    assert out.tobytes() == transl.tobytes()
    assert np.array_equal(ref.skate_sums(joints, lens)[:, 4:], np.zeros((len(lens), 3)))


def test_restatement_leaves_the_height_alone():
    joints, contact, transl, lens = fx.clips(2)
    out = ref.plant(joints, contact, transl, lens)
    assert out[:, 1].tobytes() == transl[:, 1].tobytes() and not np.array_equal(out[:, 0], transl[:, 0])
    assert np.array_equal(out[np.cumsum([0] + lens[:-1])], transl[np.cumsum([0] + lens[:-1])])      # off[0] = 0


def test_restatement_one_flagged_joint_stands_still():
    """World joints = fp32(rel + transl): with joint k flagged over a run, planting holds its x and z up to the roundings of
    the translation and of that sum (three half-ulps of the largest coordinate on either side of the run's constant)."""
    rng = np.random.default_rng(5)
    n, k, run = 90, 2, (17, 61)
    rel, contact, transl = fx.clip(rng, n)
    contact[:] = 0.0
    contact[run[0]:run[1], k] = 1.0                               # pairs (17, 18) .. (60, 61)
    joints = fx.world(rel, transl)
    out = ref.plant(joints, contact, transl, [n])
    assert np.array_equal(out[:run[0] + 1], transl[:run[0] + 1])
    after = fx.world(rel, out)[:, fx.CONTACT_JOINTS[k], :]
    held = after[run[0]:run[1] + 1]
    bound = 6 * 2.0 ** -24 * max(np.abs(joints).max(), np.abs(transl).max(), np.abs(out).max())
    assert np.abs(held[:, [0, 2]] - held[0, [0, 2]]).max() <= bound
    before = joints[run[0]:run[1] + 1, fx.CONTACT_JOINTS[k], :]
    assert np.abs(before[:, [0, 2]] - before[0, [0, 2]]).max() > 1000 * bound
    d = (out - transl)[run[1]:, [0, 2]]                           # behind the run the offset stays
    assert np.abs(d - d[0]).max() <= 2.0 ** -22 * np.abs(out).max()


def walker_numbers(plant, sums):
    """The walker through `plant(joints, contact, transl, lens) -> [n, 3]` and `sums(joints, lens, contact) -> [1, 7]`: skate
    before and after planting, the worst |x, z - the run's first| of the stance ankle over its run, and the bound on it.
    Why 2^-22 max|p| holds: a coordinate after planting is the run's constant minus the rounding of the measured joint, plus
    the rounding of the planted translation, plus the rounding of rel + translation; every value lies in [-4, 4], so each is
    at most 2^-23, six of them between two frames 6 * 2^-23 = 12 * 2^-24, and max|p| >= 3.5 makes the bound 14 * 2^-24."""
    rel, transl, contact, which = fx.walker()
    n = rel.shape[0]
    joints = fx.world(rel, transl)
    assert 3.5 <= np.abs(joints).max() < 4.0 and np.abs(transl).max() < 4.0
    assert (contact[:-1].sum(1) == 1).all()
    s0 = sums(joints, [n], contact)
    out = plant(joints, contact, transl, [n])
    after = fx.world(rel, out)
    assert np.abs(out).max() < 4.0
    s1 = sums(after, [n], contact)
    worst = 0.0
    for r0 in range(0, n - 1, fx.WALK_PERIOD):
        r1 = min(r0 + fx.WALK_PERIOD, n - 1)
        assert (which[r0:r1] == which[r0]).all()
        p = after[r0:r1 + 1, fx.CONTACT_JOINTS[which[r0]], :][:, [0, 2]].astype(np.float64)
        worst = max(worst, np.abs(p - p[0]).max())
    return ref.metrics(s0)["skate"], ref.metrics(s1)["skate"], worst, 2.0 ** -22 * float(np.abs(after).max()), out, transl


def test_restatement_walker():
    before, after, worst, bound, out, transl = walker_numbers(ref.plant, lambda j, l, c: ref.skate_sums(j, l, c, fps=fx.FPS))
    print("walker: skate %.3f -> %.3f, stance ankle moves %.3e (bound %.3e)" % (before, after, worst, bound))
    assert before > 0.5 and after == 0.0 and worst <= bound
    assert out[:, 1].tobytes() == transl[:, 1].tobytes()
    assert np.abs(out[:, 2]).max() < 1e-5 and np.abs(out[:, 0] - transl[:, 0]).max() < 1e-5     # the drift is gone, the path stays


def test_restatement_metrics_without_a_denominator():
    joints, contact, transl, lens = fx.clips(3, lens=(1,))
    s = ref.skate_sums(joints, lens, contact)
    assert np.array_equal(s, np.zeros((1, 7)))
    assert ref.metrics(s, flags=True) == dict(skate=None, slide=None, contact_slide=None, contact_moving=None)


# ------------------------------------------------------------------------------------------------------------ the host side
def test_command_line_refuses_foot_without_a_model(rg, tmp_path, capsys):
    with pytest.raises(SystemExit) as info:
        rg.evaluation.main([str(tmp_path), "--e_path", "none.bin", "--foot"])
    assert info.value.code == 2 and "--foot needs --smplx_path" in capsys.readouterr().err
    args = rg.evaluation.build_parser().parse_args([str(tmp_path), "--foot", "--smplx_path", "m.npz"])
    assert args.foot is True and rg.evaluation.build_parser().parse_args([str(tmp_path)]).foot is False
    (tmp_path / "a" / "b").mkdir(parents=True)
    np.savez(str(tmp_path / "a" / "b" / "pred_motion.npz"), poses=np.zeros((2, 165), np.float32))
    with pytest.raises(ValueError, match="foot needs smplx"):
        rg.evaluation.evaluate_folder(str(tmp_path), None, foot=True)


def test_no_gpu_no_foot_classes(rg, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    class Model:
        device = None
    with pytest.raises(rg.capi.RgError, match="no GPU visible: FootPlanter"):
        rg.foot.FootPlanter(Model())
    with pytest.raises(rg.capi.RgError, match="no GPU visible: FootMetrics"):
        rg.foot.FootMetrics(Model())
    with pytest.raises(rg.capi.RgError, match="no CPU path"):
        rg.foot.skate_sums(torch.zeros(2, 55, 3), [2])
    with pytest.raises(rg.capi.RgError, match="no CPU path"):
        rg.foot.plant_translation(torch.zeros(2, 55, 3), torch.zeros(2, 4), torch.zeros(2, 3), [2])


def test_pack_outputs_takes_a_planter(rg):
    import inspect
    sig = inspect.signature(rg.packing.pack_outputs)
    assert list(sig.parameters) == ["output", "motion_fps", "target_fps", "planter", "betas"]
    assert sig.parameters["planter"].default is None and sig.parameters["betas"].default is None
