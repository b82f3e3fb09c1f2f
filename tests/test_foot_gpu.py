"""GPU: foot skating sums and contact planting (csrc/rg_foot.hip) against the float64 restatement
tests/foot_ref.py on the seeded clips of tests/golden/foot_fixture.py (lengths 1, 2, 63, 64, 65, 150, 256, 257, 600 in one call:
no pair, one pair, the wave edge, the tile edge, three tiles with carry), their independence of the launch, the way through the
forward kinematics, the walker, pack_outputs, the command line and the refusals."""
import importlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import foot_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fx, jf, fgdfx = _load("foot_fixture"), _load("joint_fixture"), _load("fgd_fixture")


def _sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


dev = lambda a: torch.from_numpy(np.array(a)).cuda()            # (a copy: the shared reference arrays are read-only)


@pytest.fixture(scope="module")
def foot(rg):
    return rg.foot


@pytest.fixture(scope="module")
def data():
    """The nine clips on the host and on the device, and the restatement's results (computed once, never changed)."""
    joints, contact, transl, lens = fx.clips()
    d = dict(joints=joints, contact=contact, transl=transl, lens=lens, J=dev(joints), C=dev(contact), T=dev(transl))
    d["sums"] = ref.skate_sums(joints, lens, contact, fps=fx.FPS)
    d["sums_noflags"] = ref.skate_sums(joints, lens, None, fps=fx.FPS)
    d["planted"] = ref.plant(joints, contact, transl, lens)
    for v in (joints, contact, transl, d["sums"], d["sums_noflags"], d["planted"]):
        v.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def smplx(rg):
    return rg.smplx.SMPLXJoints(jf.smplx_model())


def _check_sums(parity, tag, got, want, lens):
    assert got.shape == want.shape == (len(lens), 7) and got.dtype == np.float64
    for i in (0, 1, 2, 4, 6):
        assert np.array_equal(got[:, i], want[:, i]), (tag, i, got[:, i], want[:, i])
    for c, n in enumerate(lens):
        terms = 4 * (n - 1)
        for i in (3, 5):
            rel = 0.0 if got[c, i] == want[c, i] else abs(got[c, i] - want[c, i]) / abs(want[c, i])
            parity.check("foot sums %s: clip of %d frames, entry %d vs float64 restatement (relative)" % (tag, n, i), rel,
                         terms * 2.0 ** -52)


def test_sums_match_the_restatement(foot, data, parity):
    got = foot.skate_sums(data["J"], data["lens"], data["C"], fps=fx.FPS)
    _check_sums(parity, "with flags", got, data["sums"], data["lens"])
    assert (got[2:, 1:] > 0).all()                               # every entry is exercised by every clip with pairs to spare
    got = foot.skate_sums(data["J"], data["lens"], None, fps=fx.FPS)
    _check_sums(parity, "without flags", got, data["sums_noflags"], data["lens"])
    assert np.array_equal(got[:, 4:], np.zeros((len(data["lens"]), 3)))


def _plant_err(got, want):
    """max over the values of |got - want| / (2^-23 max(|want|, 2^-126)): <= 1 is the bound."""
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) /
                  (2.0 ** -23 * np.maximum(np.abs(want.astype(np.float64)), 2.0 ** -126))).max())


def test_planting_matches_the_restatement(foot, data, parity):
    out = foot.plant_translation(data["J"], data["C"], data["T"], data["lens"])
    got = out.cpu().numpy()
    parity.check("foot planting: nine clips vs float64 restatement, |out - ref| / (2^-23 |ref|)", _plant_err(got, data["planted"]), 1.0)
    assert got[:, 1].tobytes() == data["transl"][:, 1].tobytes()
    assert not np.array_equal(got[:, 0], data["transl"][:, 0])
    starts = np.cumsum([0] + data["lens"][:-1])
    assert np.array_equal(got[starts], data["transl"][starts])
    # all flags zero: bit-identical, signed zeros included
    t0 = data["transl"].copy()
    t0[5, 0], t0[900, 2] = -0.0, -0.0
    same = foot.plant_translation(data["J"], torch.zeros_like(data["C"]), dev(t0), data["lens"])
    assert same.cpu().numpy().tobytes() == t0.tobytes()
    # in place
    t = data["T"].clone()
    r = foot.plant_translation(data["J"], data["C"], t, data["lens"], out=t)
    assert r.data_ptr() == t.data_ptr() and torch.equal(t, out)


def test_a_clip_does_not_depend_on_the_launch(foot, data):
    lens = data["lens"]
    off = np.concatenate([[0], np.cumsum(lens)])
    i257 = lens.index(257)
    order = [i for i in range(len(lens)) if i != i257]
    order.insert(4, i257)                                       # the fifth of nine
    rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in order])
    lens9 = [lens[i] for i in order]
    a9 = int(sum(lens9[:4]))
    sl = slice(int(off[i257]), int(off[i257 + 1]))
    J1, C1, T1 = dev(data["joints"][sl]), dev(data["contact"][sl]), dev(data["transl"][sl])
    J9, C9, T9 = dev(data["joints"][rows]), dev(data["contact"][rows]), dev(data["transl"][rows])
    s1 = foot.skate_sums(J1, [257], C1, fps=fx.FPS)
    s9 = foot.skate_sums(J9, lens9, C9, fps=fx.FPS)
    assert s1[0].tobytes() == s9[4].tobytes()
    p1 = foot.plant_translation(J1, C1, T1, [257]).cpu().numpy()
    p9 = foot.plant_translation(J9, C9, T9, lens9).cpu().numpy()
    assert p1.tobytes() == p9[a9:a9 + 257].tobytes()


def _fk_inputs(seed, lens):
    rng = np.random.default_rng(seed)
    poses = [jf.smooth_clip(rng, n) for n in lens]
    transl = [(rng.uniform(-1, 1, 3) + np.cumsum(rng.standard_normal((n, 3)) * 0.01, 0)).astype(np.float32) for n in lens]
    flags = [np.where(rng.random((n, 4)) < 0.5, rng.uniform(0.75, 1, (n, 4)), rng.uniform(0, 0.25, (n, 4))).astype(np.float32)
             for n in lens]
    return poses, transl, flags


def test_through_the_forward_kinematics(foot, smplx, parity):
    lens = [2, 65, 150]
    poses, transl, flags = _fk_inputs(17, lens)
    contact = np.concatenate(flags)
    planted = foot.FootPlanter(smplx).plant(poses, transl, flags)
    assert isinstance(planted, list) and [tuple(p.shape) for p in planted] == [(n, 3) for n in lens]
    before = smplx.joints(poses, transl=transl).cpu().numpy()
    after = smplx.joints(poses, transl=planted).cpu().numpy()
    worst = ref.flagged_mean_displacement(after, contact, lens)
    assert worst.size > 100 and ref.flagged_mean_displacement(before, contact, lens).max() > 1e-3
    parity.check("foot planting through the FK: mean x/z displacement of a pair's flagged joints / max|joint|",
                 worst.max() / np.abs(after).max(), 8 * 2.0 ** -24)
    for p, t in zip(planted, transl):
        assert p.cpu().numpy()[:, 1].tobytes() == t[:, 1].tobytes()
    # FootMetrics against the restatement fed with the device's own joints
    fm = foot.FootMetrics(smplx, fps=30.)
    per_clip = fm.add(poses, transl, contact=flags)
    got = fm.compute()
    want_sums = ref.skate_sums(before, lens, contact, fps=30.)
    margins = np.concatenate([ref.pair_terms(before[a:a + n], contact[a:a + n])["margins"]
                              for a, n in zip(np.cumsum([0] + lens[:-1]), lens)])
    print("FK clips: smallest relative distance of a comparison from its threshold %.3e" % margins.min())
    assert margins.min() > 1e-9
    _check_sums(parity, "through the FK", per_clip, want_sums, lens)
    want = ref.metrics(want_sums, flags=True)
    assert set(got) == {"skate", "slide", "contact_slide", "contact_moving"} == set(want)
    assert got["skate"] == want["skate"] and got["contact_moving"] == want["contact_moving"]
    terms = 4 * sum(n - 1 for n in lens)
    for k in ("slide", "contact_slide"):
        parity.check("FootMetrics %s vs float64 restatement (relative)" % k, abs(got[k] - want[k]) / want[k], terms * 2.0 ** -52)
    fm.reset()
    fm.add(poses, transl, gt_poses=poses, gt_transl=planted)
    both = fm.compute()
    assert set(both) == {"skate", "slide", "gt_skate", "gt_slide"} and both["skate"] == got["skate"] and both["slide"] == got["slide"]


def test_walker_on_the_device(foot, parity):
    cpu = _sibling("test_foot_cpu")
    plant = lambda j, c, t, lens: foot.plant_translation(dev(j), dev(c), dev(t), lens).cpu().numpy()
    sums = lambda j, lens, c: foot.skate_sums(dev(j), lens, dev(c), fps=fx.FPS)
    before, after, worst, bound, out, transl = cpu.walker_numbers(plant, sums)
    print("walker on the device: skate %.3f -> %.3f, stance ankle moves %.3e (bound %.3e)" % (before, after, worst, bound))
    assert before > 0.5 and after == 0.0
    parity.check("walker on the device: the stance ankle's x / z over its run after planting vs 2^-22 max|p| (m)", worst, bound)
    assert out[:, 1].tobytes() == transl[:, 1].tobytes()


def test_pack_outputs_with_a_planter(rg, foot, smplx):
    g = torch.Generator(device="cuda").manual_seed(3)
    B, n = 2, 16
    r = lambda w, s=0.3: torch.randn(B, n, w, device="cuda", generator=g) * s
    out = dict(pred_upper=r(39), pred_lower=r(27), pred_hands=r(90), pred_facepose=r(3), pred_exps=r(100),
               pred_transl=torch.cumsum(r(3, 0.02), 1), pred_contact=torch.rand(B, n, 4, device="cuda", generator=g))
    planter = foot.FootPlanter(smplx)
    planted = planter.plant_outputs(out)
    assert tuple(planted.shape) == (B, n, 3) and not torch.equal(planted, out["pred_transl"])
    assert torch.equal(planted[:, :, 1], out["pred_transl"][:, :, 1])
    plain = rg.packing.pack_outputs(out)
    got = rg.packing.pack_outputs(out, planter=planter)
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    assert torch.equal(got[2], rg.packing.upsample_features(planted)) and tuple(got[2].shape) == (B, 2 * n, 3)
    none = rg.packing.pack_outputs(out, planter=None)
    for a, b in zip(none, plain):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    betas = [np.full(300, 0.5), np.zeros(300)]
    shaped = rg.packing.pack_outputs(out, planter=planter, betas=betas)[2]
    assert torch.equal(shaped, rg.packing.upsample_features(planter.plant_outputs(out, betas=betas)))


def test_command_line(rg, foot, tmp_path, capsys):
    ev = rg.evaluation
    B, n = 3, 40
    poses, transl, _ = _fk_inputs(29, [n] * (2 * B))
    names = ["test/%d_scott_0_%d_%d" % (i, i, i) for i in range(B)]
    ex = np.zeros((B, n, 100), np.float32)
    rg.packing.save_sample_files(str(tmp_path / "eval"), names, (np.stack(poses[:B]), ex, np.stack(transl[:B])),
                                 (np.stack(poses[B:]), ex, np.stack(transl[B:])))
    np.savez(str(tmp_path / "model.npz"), **jf.smplx_model())
    sd = fgdfx.state_dict(np.load(os.path.join(HERE, "golden", "fgd_eval.npz")))
    torch.save({"model_state": {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}}, str(tmp_path / "ckpt.bin"))
    base = [str(tmp_path / "eval"), "--e_path", str(tmp_path / "ckpt.bin"), "--smplx_path", str(tmp_path / "model.npz")]
    ev.main(base)
    plain = json.loads(capsys.readouterr().out)
    ev.main(base + ["--foot"])
    line = json.loads(capsys.readouterr().out)
    assert set(line) - set(plain) == {"skate", "slide", "gt_skate", "gt_slide"} and set(plain) <= set(line)
    assert all(line[k] == plain[k] or (line[k] != line[k] and plain[k] != plain[k]) for k in plain)
    fm = foot.FootMetrics(ev.SMPLXJoints(str(tmp_path / "model.npz")), fps=30.)
    fm.add(poses[:B], transl[:B], poses[B:], transl[B:], betas=[np.zeros(300)] * B)
    want = fm.compute()
    assert {k: line[k] for k in want} == want and want["skate"] is not None and want["gt_slide"] is not None


def test_refusals(rg, foot, data, parity):
    h = rg.capi.get_handle()
    lens = [3, 5]
    off = np.array([0, 3, 8], np.int32)
    J, C, T = data["J"][:8].contiguous(), data["C"][:8].contiguous(), data["T"][:8].contiguous()
    off_dev = dev(off)
    sums = torch.full((2, 7), -7.0, device="cuda", dtype=torch.float64)
    out = torch.full((8, 3), -7.0, device="cuda")
    nan = float("nan")

    def skate(**kw):
        a = dict(joints=J, contact=C, clip_off=off_dev, host=off, n=2, fps=30., height=0.05, speed=0.5, cthr=0.5, dthr=0.01, sums=sums)
        a.update(kw)
        host = a["host"]
        h.call("foot_skate_sums", a["joints"], a["contact"], a["clip_off"], None if host is None else host.ctypes.data, a["n"], a["fps"],
               a["height"], a["speed"], a["cthr"], a["dthr"], a["sums"])

    def plant(**kw):
        a = dict(joints=J, contact=C, trans=T, clip_off=off_dev, host=off, n=2, cthr=0.5, out=out)
        a.update(kw)
        host = a["host"]
        h.call("foot_plant", a["joints"], a["contact"], a["trans"], a["clip_off"], None if host is None else host.ctypes.data, a["n"],
               a["cthr"], a["out"])

    i32 = lambda *v: np.array(v, np.int32)
    both = [(dict(joints=None), "null pointer"), (dict(clip_off=None), "null pointer"), (dict(host=None), "null pointer"),
            (dict(n=0), "at least one clip"), (dict(n=-1), "at least one clip"),
            (dict(host=i32(1, 3, 8)), "clip_off must start at 0"), (dict(host=i32(0, 5, 3)), "clip_off must not decrease"),
            (dict(host=i32(0, 3, 3)), "empty clip"), (dict(host=i32(0, 0, 8)), "empty clip"),
            (dict(host=i32(0, 3, 2 ** 31 // 165)), "too many frames"), (dict(cthr=nan), "must be (a )?numbers?")]
    only_skate = [(dict(sums=None), "null pointer"), (dict(height=nan), "must be numbers"), (dict(speed=nan), "must be numbers"),
                  (dict(dthr=nan), "must be numbers"), (dict(fps=0.0), "fps must be positive"), (dict(fps=-30.0), "fps must be positive"),
                  (dict(fps=nan), "fps must be positive")]
    only_plant = [(dict(contact=None), "null pointer"), (dict(trans=None), "null pointer"), (dict(out=None), "null pointer")]
    for fn, name, cases in ((skate, "rg_foot_skate_sums", both + only_skate), (plant, "rg_foot_plant", both + only_plant)):
        for kw, text in cases:
            with pytest.raises(rg.capi.RgError, match=text) as info:
                fn(**kw)
            assert name in str(info.value), (kw, str(info.value))
    torch.cuda.synchronize()
    assert (sums == -7.0).all() and (out == -7.0).all()           # nothing was launched
    skate()
    plant()
    jh, ch, th = data["joints"][:8], data["contact"][:8], data["transl"][:8]
    want = ref.skate_sums(jh, lens, ch, fps=30.)
    _check_sums(parity, "behind the refusals", sums.cpu().numpy(), want, lens)
    parity.check("foot planting behind the refusals, |out - ref| / (2^-23 |ref|)", _plant_err(out.cpu().numpy(), ref.plant(jh, ch, th, lens)), 1.0)
    # contact may be null for the sums only
    skate(contact=None)
    assert np.array_equal(sums.cpu().numpy()[:, 4:], np.zeros((2, 3)))
