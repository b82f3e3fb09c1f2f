"""GPU: the foot lock (csrc/rg_footlock.hip) against the float64 restatement tests/foot_lock_ref.py on the
seeded clips of tests/golden/foot_lock_fixture.py (lengths 1, 2, 63, 64, 65, 150, 256, 257, 600 in one call), through the
existing forward kinematics, on the walker, its invariants, the out-of-reach clip, packing, long-form synthesis and the
refusals.

Tolerances.  The targets are fp64 sums in another order: (run length + 2) * 2^-52 * max|p| per offset (NOTEBOOK).  The IK's
transforms are fp32 where the restatement's are float64, so its pose channels are held to 4 x the restatement's own
sensitivity to transforms stored as fp32 (measured on the CPU over the fixture: 4.3e-07 rad, so the bound is 1.7e-06 rad; the
factor is a cushion for sinf / cosf, which that rounding model does not cover), and the ankle's distance from its target
through the existing forward kinematics to 2 x what the restatement's own poses, rounded to fp32, reach through that same
kernel."""
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

import foot_lock_ref as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, sub="golden"):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, sub, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fx, cpu = _load("foot_lock_fixture"), _load("test_foot_lock_cpu", "")
dev = lambda a, dt=None: torch.from_numpy(np.array(a, dtype=dt)).cuda()     # (a copy: the shared arrays are read-only)
ANKLES = [ref.LEGS[0][2], ref.LEGS[1][2]]
HIPS = [ref.LEGS[0][0], ref.LEGS[1][0]]
OTHER = [c for c in range(165) if c not in ref.LEG_CHANNELS]
U = 2.0 ** -52


@pytest.fixture(scope="module")
def foot(rg):
    return rg.foot


@pytest.fixture(scope="module")
def smplx(rg):
    return rg.smplx.SMPLXJoints(fx.smplx_model())


def _case(smplx, poses, transl, contact, lens):
    """Inputs on both sides, the device's own world joints, and the restatement fed with those joints (so that both take their
    targets from the same fp32 positions); computed once, never changed."""
    rest, parents, pose_mean = cpu.model()
    d = dict(poses=poses, transl=transl, contact=contact, lens=lens, P=dev(poses), T=dev(transl), C=dev(contact))
    split = lambda a: list(np.split(a, np.cumsum(lens)[:-1]))
    d["clips"], d["tclips"], d["cclips"] = split(poses), split(transl), split(contact)
    d["J"] = smplx.joints(d["clips"], transl=d["tclips"])
    d["joints"] = d["J"].cpu().numpy()
    d["ref"] = ref.lock(poses, transl, contact, lens, rest, parents, pose_mean, blend=fx.BLEND, joints=d["joints"])
    for v in (poses, transl, contact, d["joints"], d["ref"]["poses"], d["ref"]["offsets"], d["ref"]["reach"]):
        v.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def data(smplx):
    return _case(smplx, *fx.clips())


@pytest.fixture(scope="module")
def walk(smplx):
    poses, transl, contact, which = fx.walker()
    d = _case(smplx, poses, transl, contact, [poses.shape[0]])
    d["which"] = which
    return d


@pytest.fixture(scope="module")
def far(smplx):
    poses, transl, contact = fx.far_clip()
    return _case(smplx, poses, transl, contact, [poses.shape[0]])


@pytest.fixture(scope="module")
def pose_bound():
    s = cpu.sensitivity()
    print("sensitivity of the restatement to fp32 transforms %.3e rad -> pose bound %.3e rad" % (s, 4 * s))
    return 4 * s


def _locker(foot, smplx, **kw):
    return foot.FootLocker(smplx, blend=fx.BLEND, **kw)


# ------------------------------------------------------------------------------------------------------------------ targets
def _check_targets(parity, tag, got_off, got_stats, d):
    r = d["ref"]
    want, span, stats = r["offsets"], r["span"], r["stats"]
    pmax = float(np.abs(d["joints"][:, ANKLES]).max())
    assert got_off.shape == want.shape and got_off.dtype == np.float64 and got_stats.shape == stats.shape == (len(d["lens"]), 5)
    for i in (0, 1, 2):
        assert np.array_equal(got_stats[:, i], stats[:, i]), (tag, i, got_stats[:, i], stats[:, i])
    bound = (span + 2) * U * pmax                                   # [F, 2]
    assert np.array_equal(got_off[span == 0], np.zeros_like(got_off[span == 0])) and not want[span == 0].any()
    err = np.abs(got_off - want).max(2)
    parity.check("foot lock targets %s: |offset - restatement| / ((run + 2) 2^-52 max|p|)" % tag, (err / bound).max(), 1.0)
    off = np.concatenate([[0], np.cumsum(d["lens"])])
    for c, n in enumerate(d["lens"]):
        mem = np.stack([ref.members(d["contact"][off[c]:off[c + 1], k]) for k in range(2)], 1)
        b = bound[off[c]:off[c + 1]][mem]
        if not b.size:
            assert not got_stats[c].any()
            continue
        parity.check("foot lock targets %s: clip of %d frames, sum of |d| vs restatement (m)" % (tag, n),
                     abs(got_stats[c, 3] - stats[c, 3]), np.sqrt(3) * b.sum() + mem.sum() * U * stats[c, 3])
        parity.check("foot lock targets %s: clip of %d frames, max of |d| vs restatement (m)" % (tag, n),
                     abs(got_stats[c, 4] - stats[c, 4]), np.sqrt(3) * b.max())


def test_targets_match_the_restatement(foot, data, walk, parity):
    """Counts equal; offsets within (run length + 2) 2^-52 max|p| per coordinate (each of the two sums of a run of L positions
    errs by at most (L - 1) 2^-53 max|p| after the division, which and the subtraction add one rounding each); the sum of |d|
    within the sum of its terms' bounds (sqrt 3: three coordinates) plus its own reordering, the maximum within its term's."""
    for tag, d in (("nine clips", data), ("walker", walk)):
        off, stats = foot.lock_targets(d["J"], d["C"], d["lens"], 0.5, fx.BLEND)
        assert off.dtype == torch.float64 and tuple(off.shape) == (sum(d["lens"]), 2, 3)
        _check_targets(parity, tag, off.cpu().numpy(), stats, d)
    assert (data["ref"]["stats"][2:, :3] > 0).all()
    # blend = 0: zero outside the runs, the member frames as before
    off3, _ = foot.lock_targets(data["J"], data["C"], data["lens"], 0.5, fx.BLEND)
    off0, _ = foot.lock_targets(data["J"], data["C"], data["lens"], 0.5, 0)
    member = ref.targets(data["joints"], data["contact"], data["lens"], blend=0)[2] > 0          # [F, 2]
    got0, got3 = off0.cpu().numpy(), off3.cpu().numpy()
    assert not got0[~member].any() and got3[~member].any() and got0[member].tobytes() == got3[member].tobytes()


# ----------------------------------------------------------------------------------------------------------------------- IK
def _lock(foot, smplx, d, **kw):
    lk = _locker(foot, smplx, **kw)
    out = lk.lock(d["clips"], d["tclips"], d["cclips"])
    assert isinstance(out, list) and [tuple(o.shape) for o in out] == [(n, 165) for n in d["lens"]]
    return torch.cat(out, 0), lk.last_report


def test_ik_matches_the_restatement(foot, smplx, data, walk, far, pose_bound, parity):
    """Pose channels of the locked legs within 4 x the restatement's sensitivity to fp32 transforms (measured: 4.3e-07 rad,
    bound 1.733e-06 rad; on MI355X the nine clips differ by 2.754e-07, the walker by 1.098e-07, the out-of-reach clip by 4.206e-07
    rad); every other channel bit for bit; reach within fp32 rounding; the same frames solved."""
    for tag, d in (("nine clips", data), ("walker", walk), ("out-of-reach clip", far)):
        got, report = _lock(foot, smplx, d)
        g, r = got.cpu().numpy(), d["ref"]
        assert g.dtype == np.float32 and np.isfinite(g).all()
        assert g[:, OTHER].tobytes() == d["poses"][:, OTHER].tobytes()
        idle = ~(r["offsets"] != 0).any(2)
        for k, leg in enumerate(ref.LEGS):
            ch = [3 * j + q for j in leg for q in range(3)]
            assert g[idle[:, k]][:, ch].tobytes() == d["poses"][idle[:, k]][:, ch].tobytes()
        err = np.abs(g.astype(np.float64) - r["poses"])[:, ref.LEG_CHANNELS].max()
        print("%s: pose channels vs restatement %.3e rad (bound %.3e)" % (tag, err, pose_bound))
        parity.check("foot lock IK %s: pose channels vs float64 restatement (rad)" % tag, err, pose_bound)
        assert np.array_equal(report["stats"][:, :3], r["stats"][:, :3])
        assert report["unreachable"] == int((r["reach"] > ref.par(ref.STRETCH)).sum())
        # reach = |T - a| / (l1 + l2) from fp32 positions: hip and ankle each within 4 * 2^-24 max|p| (four fp32 levels of the
        # chain), and the fp32 rounding of the quotient
        pmax = float(np.abs(d["joints"]).max())
        assert abs(report["max_reach"] - r["reach"].max()) <= 8 * 2.0 ** -24 * pmax / (fx.THIGH + fx.SHANK) + 2.0 ** -24 * r["reach"].max()
    assert far["ref"]["reach"].max() > 1.0 and data["ref"]["reach"].max() < 0.99


def _through_fk(smplx, d, poses):
    """[F, 165] -> the ankles [F, 2, 3] and hips of the existing forward kinematics kernel (float64 copies of its fp32 joints)."""
    J = smplx.joints(list(np.split(np.asarray(poses, np.float32), np.cumsum(d["lens"])[:-1])), transl=d["tclips"]).cpu().numpy()
    return J[:, ANKLES].astype(np.float64), J[:, HIPS].astype(np.float64)


def _fk_numbers(foot, smplx, d):
    """Distance of the ankle from its target on reachable solved frames, through SMPLXJoints.joints (parent-commit code): of
    lock()'s poses, and of the restatement's poses rounded to fp32."""
    got, _ = _lock(foot, smplx, d)
    r = d["ref"]
    ok = (r["reach"] > 0) & (r["reach"] <= ref.par(ref.STRETCH))
    dist = lambda poses: np.linalg.norm(_through_fk(smplx, d, poses)[0] - r["targets"], axis=2)
    return dist(got.cpu().numpy()), dist(r["poses"].astype(np.float32)), ok, got


def test_through_the_existing_forward_kinematics(foot, smplx, data, parity):
    """lock()'s poses through SMPLXJoints.joints(..., transl=) -- the parent's kernel, not the code under test -- leave the ankle
    at most 2 x as far from its target as the restatement's poses, rounded to fp32, through that same kernel (measured on
    MI355X: 2.686e-07 m against 2.682e-07 m, so a bound of 5.4e-07 m; both are the fp32 of the kernel's chain at |p| < 2 m)."""
    mine, base, ok, _ = _fk_numbers(foot, smplx, data)
    print("ankle to target through the FK kernel: lock() %.3e m, restatement's fp32 poses %.3e m" % (mine[ok].max(), base[ok].max()))
    assert ok.sum() > 2000
    parity.check("foot lock through the FK: ankle to target on reachable frames vs 2 x the restatement's (m)", mine[ok].max(),
                 2 * base[ok].max())
    before = np.linalg.norm(data["joints"][:, ANKLES].astype(np.float64) - data["ref"]["targets"], axis=2)
    assert before[ok].max() > 1000 * base[ok].max()                # the lock had something to do


def test_walker_on_the_device(rg, foot, smplx, walk, parity):
    mine, base, ok, got = _fk_numbers(foot, smplx, walk)
    r, which, n, P = walk["ref"], walk["which"], walk["poses"].shape[0], fx.WALK_PERIOD
    bound = 2 * base[ok].max()
    ank = _through_fk(smplx, walk, got.cpu().numpy())[0]
    worst = 0.0
    for r0 in range(0, n - 1, P):
        r1 = min(r0 + P, n - 1)
        k = which[r0]
        anchor = r["targets"][r0, k]
        assert np.abs(r["targets"][r0:r1 + 1, k] - anchor).max() <= 1e-12       # one world position per run
        worst = max(worst, np.linalg.norm(ank[r0:r1 + 1, k] - anchor, axis=1).max())
    print("walker on the device: the stance ankle stays within %.3e m of its anchor (bound %.3e)" % (worst, bound))
    parity.check("walker on the device: stance ankle to its run's anchor vs 2 x the restatement's (m)", worst, bound)
    fm = foot.FootMetrics(smplx, fps=15.)
    fm.add(walk["clips"], walk["tclips"], contact=walk["cclips"])
    moving_before = fm.compute()["contact_moving"]
    fm.reset()
    fm.add([got], walk["tclips"], contact=walk["cclips"])
    moving_after = fm.compute()["contact_moving"]
    print("walker on the device: contact_moving %.3f -> %.3f" % (moving_before, moving_after))
    assert moving_before > 0.5 and moving_after == 0.0
    assert walk["T"].cpu().numpy().tobytes() == walk["transl"].tobytes()         # the translation is only read


# --------------------------------------------------------------------------------------------------------------- invariants
def test_invariants(foot, smplx, data):
    lens, P, T, C = data["lens"], data["P"], data["T"], data["C"]
    # no flag set: bit for bit, signed zeros included
    p0 = data["poses"].copy()
    p0[5, 3], p0[900, 12], p0[901, 23] = -0.0, -0.0, -0.0
    off, stats = foot.lock_targets(data["J"], torch.zeros_like(C), lens, 0.5, fx.BLEND)
    assert not off.cpu().numpy().any() and not np.signbit(off.cpu().numpy()).any() and not stats.any()
    same, reach = foot.lock_poses(smplx, dev(p0), T, off, lens)
    assert same.cpu().numpy().tobytes() == p0.tobytes() and not reach.cpu().numpy().any()
    assert np.isfinite(same.cpu().numpy()).all()
    # a clip does not depend on the launch around it: 257 frames alone against the fifth of nine
    o = np.concatenate([[0], np.cumsum(lens)])
    i257 = lens.index(257)
    order = [i for i in range(len(lens)) if i != i257]
    order.insert(4, i257)
    rows = np.concatenate([np.arange(o[i], o[i + 1]) for i in order])
    lens9 = [lens[i] for i in order]
    a9 = int(sum(lens9[:4]))
    sl = slice(int(o[i257]), int(o[i257 + 1]))
    take = lambda t, idx: t[torch.as_tensor(idx, device="cuda")].contiguous() if not isinstance(idx, slice) else t[idx].contiguous()
    off1, st1 = foot.lock_targets(take(data["J"], sl), take(C, sl), [257], 0.5, fx.BLEND)
    off9, st9 = foot.lock_targets(take(data["J"], rows), take(C, rows), lens9, 0.5, fx.BLEND)
    assert off1.cpu().numpy().tobytes() == off9[a9:a9 + 257].cpu().numpy().tobytes() and st1[0].tobytes() == st9[4].tobytes()
    assert st1[0, 0] > 0
    p1, r1 = foot.lock_poses(smplx, take(P, sl), take(T, sl), off1, [257])
    p9, r9 = foot.lock_poses(smplx, take(P, rows), take(T, rows), off9, lens9)
    assert p1.cpu().numpy().tobytes() == p9[a9:a9 + 257].cpu().numpy().tobytes()
    assert r1.cpu().numpy().tobytes() == r9[a9:a9 + 257].cpu().numpy().tobytes()
    # in place
    full_off, _ = foot.lock_targets(data["J"], C, lens, 0.5, fx.BLEND)
    out, reach = foot.lock_poses(smplx, P, T, full_off, lens)
    p = P.clone()
    res, reach2 = foot.lock_poses(smplx, p, T, full_off, lens, out=p)
    assert res.data_ptr() == p.data_ptr() and torch.equal(p, out) and torch.equal(reach, reach2) and not torch.equal(out, P)


def test_out_of_reach_targets_are_approached(foot, smplx, far, parity):
    """Finite outputs; an unreachable target is approached along the hip-target line: the ankle lies at stretch (l1 + l2) from
    the hip towards it, through the existing forward kinematics within 2 x what the restatement's fp32 poses reach."""
    got, report = _lock(foot, smplx, far)
    r = far["ref"]
    assert torch.isfinite(got).all()
    out_of_reach = r["reach"] > ref.par(ref.STRETCH)
    assert report["unreachable"] == int(out_of_reach.sum()) > 10 and report["max_reach"] > 1.0

    def miss(poses):
        ank, hip = _through_fk(smplx, far, poses)
        to = r["targets"] - hip
        want = hip + to / np.linalg.norm(to, axis=2, keepdims=True) * ref.par(ref.STRETCH) * (fx.THIGH + fx.SHANK)
        return np.linalg.norm(ank - want, axis=2)[out_of_reach].max(), np.linalg.norm(ank - r["targets"], axis=2)[out_of_reach].min()

    mine, base = miss(got.cpu().numpy()), miss(r["poses"].astype(np.float32))
    print("out of reach: ankle to the point on the hip-target line %.3e m (restatement's fp32 poses %.3e m)" % (mine[0], base[0]))
    parity.check("foot lock out of reach: ankle to stretch (l1 + l2) along the hip-target line vs 2 x the restatement's (m)", mine[0],
                 2 * base[0])
    assert mine[1] > 1e-4                                          # not met


def test_fallbacks_on_the_device(foot, smplx, pose_bound, parity):
    """The straight-legged clip: every solve is a straight leg (bend axis = the hip's own x) with its target exactly on the
    hip-ankle line (S = I), 26 of the 48 out of reach.  The restatement takes both fallbacks on every solve (asserted), and
    the kernel must be on the same branches to agree with it: pose channels within the IK bound, the hip turned by +A1 and the
    knee by -2 A1 about x (the definition's direction: thigh backwards, shank forwards) with nothing about y or z beyond that
    bound, finite outputs, every other channel bit for bit, reach and unreachable equal.  (log_map's branches next to zero and
    next to pi cannot be reached from poses stored as fp32; tests/test_foot_lock_cpu.py runs them in the kernel's own source
    compiled for the host.)"""
    poses, transl, contact = fx.straight_clip()
    d = _case(smplx, poses, transl, contact, [poses.shape[0]])
    r = d["ref"]
    assert len(r["info"]) == 48 and all(i["straight"] and i["on_line"] for _, _, i in r["info"])
    got, report = _lock(foot, smplx, d)
    g = got.cpu().numpy()
    assert np.isfinite(g).all() and g[:, OTHER].tobytes() == poses[:, OTHER].tobytes()
    err = np.abs(g.astype(np.float64) - r["poses"])[:, ref.LEG_CHANNELS].max()
    print("straight clip: pose channels vs restatement %.3e rad (bound %.3e)" % (err, pose_bound))
    parity.check("foot lock IK straight clip (both fallbacks): pose channels vs float64 restatement (rad)", err, pose_bound)
    for hip, knee, ankle in ref.LEGS:
        assert (g[:, 3 * hip] > 0.09).all() and (g[:, 3 * knee] < -0.18).all() and (g[:, 3 * ankle] > 0.09).all()
        for j in (hip, knee, ankle):
            assert np.abs(g[:, 3 * j + 1:3 * j + 3]).max() <= pose_bound
    assert report["unreachable"] == int((r["reach"] > ref.par(ref.STRETCH)).sum()) == 26
    assert np.array_equal(report["stats"][:, :3], r["stats"][:, :3]) and report["stats"][0, 2] == 48
    _, reach = foot.lock_poses(smplx, d["P"], d["T"], foot.lock_targets(d["J"], d["C"], d["lens"], 0.5, fx.BLEND)[0], d["lens"])
    assert np.abs(reach.cpu().numpy() - r["reach"]).max() <= 8 * 2.0 ** -24 * float(np.abs(d["joints"]).max()) / (fx.THIGH + fx.SHANK) \
        + 2.0 ** -24 * r["reach"].max()


# --------------------------------------------------------------------------------------------------------- the layers above
def test_pack_outputs_locked(rg, foot, smplx):
    g = torch.Generator(device="cuda").manual_seed(3)
    B, n = 2, 16
    r = lambda w, s=0.3: torch.randn(B, n, w, device="cuda", generator=g) * s
    out = dict(pred_upper=r(39), pred_lower=r(27), pred_hands=r(90), pred_facepose=r(3), pred_exps=r(100),
               pred_transl=torch.cumsum(r(3, 0.02), 1), pred_contact=torch.rand(B, n, 4, device="cuda", generator=g))
    locker = _locker(foot, smplx)
    locked = locker.lock_outputs(out)
    plain = rg.packing.pack_outputs(out)
    unlocked = rg.packing.scatter_parts(out["pred_upper"], out["pred_lower"], out["pred_hands"], out["pred_facepose"])
    assert tuple(locked.shape) == (B, n, 165) and not torch.equal(locked, unlocked)
    assert torch.equal(locked[:, :, OTHER], unlocked[:, :, OTHER]) and locker.last_report["stats"].shape == (B, 5)
    got = rg.packing.pack_outputs_locked(out, locker)
    assert torch.equal(got[0], rg.packing.upsample_motion(locked)) and tuple(got[0].shape) == (B, 2 * n, 165)      # locked, then upsampled
    assert torch.equal(got[1], plain[1]) and torch.equal(got[2], plain[2])
    none = rg.packing.pack_outputs(out, planter=None)
    for a, b in zip(none, plain):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert "planter" not in inspect.signature(rg.packing.pack_outputs_locked).parameters      # one correction or the other
    betas = [np.full(300, 0.5), np.zeros(300)]
    shaped = rg.packing.pack_outputs_locked(out, locker, betas=betas)[0]
    assert torch.equal(shaped, rg.packing.upsample_motion(locker.lock_outputs(out, betas=betas)))


def _longform_clip(rg, seeds, n=None):
    parts = [rg.synth.synth_batch(1, seed=s) for s in seeds]
    c = {k: torch.cat([p[k] for p in parts], dim=1) for k in rg.longform.MOTION_KEYS + rg.longform.REPEAT_KEYS
         if k in parts[0] and torch.is_tensor(parts[0][k]) and parts[0][k].dim() >= 2 and parts[0][k].shape[1] == 150}
    return c if n is None else {k: v[:, :n] for k, v in c.items()}


def test_longform_with_a_locker(rg, foot):
    """The 2-layer synthetic model of test_longform_batched_gpu.py, one clip of two windows and one of three, the second with
    betas (on a body model whose shape directions move the joints by centimetres, so that betas given to the wrong clip would
    show), at a target rate equal to the motion rate so that the result IS the blend.  run(locker=) equals locking the unlocked
    run's blend by hand with the contact track it returns, bit for bit; run_many equals run -- poses within the 1e-4 rad and
    the contact track within the relative 1e-5 that test_longform_batched_gpu.py holds poses and `trans` to, the same flags set;
    without a locker the result is today's, key for key and byte for byte.  An untrained model's flags are noise around some
    level, so a first pass returns the blended track and the threshold goes into the widest gap between its values around
    their median: about half of the flags are set, and none sits where the difference between the two drivers could flip it."""
    cfg = rg.synth.default_model_cfg(num_layers=2)
    vae_cfgs = rg.synth.synth_vae_cfgs(decoder_arch="all_encoder", num_layers=2)
    model = rg.build_architecture(rg.synth.reference_style_model_cfg(cfg, vae_cfgs), database=None, precision="fp32")
    model.load_state_dict(rg.synth.synth_full_state(0, cfg, vae_cfgs))
    model.eval()
    shaped = rg.smplx.SMPLXJoints(fx.smplx_model(shape_scale=2e-3))
    betas = [None, np.random.default_rng(5).standard_normal(300)]
    assert np.abs(shaped.rest_joints(betas[1]) - shaped.rest_joints()).max() > 0.02
    clips = [_longform_clip(rg, (11, 12), 260), _longform_clip(rg, (13, 14, 15), 300)]      # 2 and 3 windows (hop 135)
    audio = lambda ci, cidx: rg.synth.synth_batch(1, seed=1000 + 10 * ci + cidx)["audio"]
    synth = rg.longform.LongformSynthesizer(model, overlap=15, target_fps=15)
    copy = lambda d: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}
    same = lambda a, b: np.asarray(a).tobytes() == np.asarray(b).tobytes()
    feats_many = lambda ci, cidx, t0, t1, ann: dict(audio=audio(ci, cidx), text_features=None)
    many_betas = [np.zeros(300), betas[1]]                          # (zeros: the template, as None for run)
    probe = synth.run_many([copy(c) for c in clips], feats_many, noise_tape=rg.synth.ClipTapes([71, 72]), locker=_locker(foot, shaped))
    values = np.sort(np.concatenate([probe[ci]["contact"][:, :2].ravel() for ci in range(2)]).astype(np.float64))
    mid = values[int(0.4 * values.size):int(0.6 * values.size)]
    i = int(np.argmax(np.diff(mid)))
    level, gap = float(0.5 * (mid[i] + mid[i + 1])), float(mid[i + 1] - mid[i])
    print("flag threshold %.6f in a gap of %.3e (flags from %.4f to %.4f)" % (level, gap, values[0], values[-1]))
    locker = _locker(foot, shaped, contact_threshold=level)
    level = float(np.float32(level))                                # (the threshold crosses the C ABI as fp32)
    many = synth.run_many([copy(c) for c in clips], feats_many, noise_tape=rg.synth.ClipTapes([71, 72]), locker=locker, betas=many_betas)
    for ci, clip in enumerate(clips):
        feats = lambda cidx, t0, t1, ann, ci=ci: dict(audio=audio(ci, cidx), text_features=None)
        plain = synth.run(copy(clip), feats, noise_tape=rg.synth.NoiseTape(71 + ci))
        none = synth.run(copy(clip), feats, noise_tape=rg.synth.NoiseTape(71 + ci), locker=None, betas=None)
        assert set(plain) == set(none) == {"poses", "expressions", "trans", "latents", "windows"}
        assert all(same(plain[k], none[k]) for k in ("poses", "expressions", "trans")) and plain["windows"] == none["windows"]
        assert all(torch.equal(a, b) for a, b in zip(plain["latents"], none["latents"]))
        got = synth.run(copy(clip), feats, noise_tape=rg.synth.NoiseTape(71 + ci), locker=locker, betas=betas[ci])
        n = clip["motion"].shape[1]
        assert len(got["windows"]) == 2 + ci and set(got) == set(plain) | {"contact", "foot_lock"}
        assert all(same(plain[k], got[k]) for k in ("expressions", "trans")) and got["contact"].shape == (n, 4)
        hand = locker.lock(plain["poses"], plain["trans"], got["contact"], betas=None if betas[ci] is None else [betas[ci]])
        assert same(hand.cpu().numpy(), got["poses"]) and not same(plain["poses"], got["poses"])
        assert same(got["poses"][:, OTHER], plain["poses"][:, OTHER]) and np.isfinite(got["poses"]).all()
        assert got["foot_lock"]["stats"].shape == (1, 5) and got["foot_lock"]["stats"][0, 0] > 0
        if betas[ci] is not None:                                   # the betas matter: without them the legs come out differently
            bare = locker.lock(plain["poses"], plain["trans"], got["contact"]).cpu().numpy()
            assert np.abs(bare - got["poses"]).max() > 1e-2
        # run_many equals run
        ml = many[ci]
        assert set(ml) == set(got) and ml["windows"] == got["windows"]
        assert np.abs(np.stack([ml["contact"], got["contact"]])[:, :, :2] - level).min() > gap / 4      # no flag near the threshold in either driver
        assert np.array_equal(ml["contact"][:, :2] >= level, got["contact"][:, :2] >= level)
        assert np.array_equal(ml["foot_lock"]["stats"][:, :3], got["foot_lock"]["stats"][:, :3])
        d = np.abs(ml["contact"] - got["contact"]).max() / max(1e-9, np.abs(got["contact"]).max())
        dp = np.abs(ml["poses"] - got["poses"]).max()
        print("clip %d: run_many vs run, contact %.3e (relative), locked poses %.3e rad" % (ci, d, dp))
        assert d <= 1e-5 and dp <= 1e-4, (ci, d, dp)
        for k in ("expressions", "trans"):
            assert np.abs(ml[k] - got[k]).max() / max(1e-9, np.abs(got[k]).max()) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(rg, foot, smplx, data, parity):
    h = rg.capi.get_handle()
    lens = [3, 5]
    off = np.array([0, 3, 8], np.int32)
    J, C, P, T = (data[k][:8].contiguous() for k in ("J", "C", "P", "T"))
    off_dev = dev(off)
    offsets = torch.full((8, 2, 3), -7.0, device="cuda", dtype=torch.float64)
    stats = torch.full((2, 5), -7.0, device="cuda", dtype=torch.float64)
    out = torch.full((8, 165), -7.0, device="cuda")
    reach = torch.full((8, 2), -7.0, device="cuda")
    good = torch.zeros(8, 2, 3, device="cuda", dtype=torch.float64)
    rest = dev(np.stack([smplx.rest_joints()] * 2), np.float32)
    nan = float("nan")
    i32 = lambda *v: np.array(v, np.int32)

    def targets(**kw):
        a = dict(joints=J, contact=C, clip_off=off_dev, host=off, n=2, cthr=0.5, blend=3, offsets=offsets, stats=stats)
        a.update(kw)
        host = a["host"]
        h.call("foot_lock_targets", a["joints"], a["contact"], a["clip_off"], None if host is None else host.ctypes.data, a["n"],
               a["cthr"], a["blend"], a["offsets"], a["stats"])

    def ik(**kw):
        a = dict(poses=P, transl=T, rest=rest, parents=smplx.parents_dev, parents_host=smplx.parents, clip_off=off_dev, host=off, n=2,
                 offsets=good, stretch=0.995, out=out, reach=reach)
        a.update(kw)
        host, ph = a["host"], a["parents_host"]
        h.call("foot_lock_ik", a["poses"], a["transl"], a["rest"], smplx.pose_mean, a["parents"], None if ph is None else ph.ctypes.data,
               a["clip_off"], None if host is None else host.ctypes.data, a["n"], a["offsets"], a["stretch"], a["out"], a["reach"])

    both = [(dict(clip_off=None), "null pointer"), (dict(host=None), "null pointer"), (dict(offsets=None), "null pointer"),
            (dict(n=0), "at least one clip"), (dict(n=-1), "at least one clip"),
            (dict(host=i32(1, 3, 8)), "clip_off must start at 0"), (dict(host=i32(0, 5, 3)), "clip_off must not decrease"),
            (dict(host=i32(0, 3, 3)), "empty clip"), (dict(host=i32(0, 0, 8)), "empty clip"),
            (dict(host=i32(0, 3, 2 ** 31 // 165)), "too many frames")]
    only_targets = [(dict(joints=None), "null pointer"), (dict(contact=None), "null pointer"), (dict(stats=None), "null pointer"),
                    (dict(cthr=nan), "must be a number"), (dict(blend=-1), "blend must not be negative")]
    legs = smplx.parents.copy()
    legs[7] = 1
    loop = smplx.parents.copy()
    loop[3] = 3
    only_ik = [(dict(poses=None), "null pointer"), (dict(transl=None), "null pointer"), (dict(rest=None), "null pointer"),
               (dict(parents=None), "null pointer"), (dict(parents_host=None), "null pointer"), (dict(out=None), "null pointer"),
               (dict(reach=None), "null pointer"), (dict(stretch=0.0), r"stretch must lie in \(0, 1\]"),
               (dict(stretch=1.5), r"stretch must lie in \(0, 1\]"), (dict(stretch=-0.5), r"stretch must lie in \(0, 1\]"),
               (dict(stretch=nan), r"stretch must lie in \(0, 1\]"), (dict(parents_host=legs), "legs must be the chains"),
               (dict(parents_host=loop), r"parents\[j\] must lie in")]
    for fn, name, cases in ((targets, "rg_foot_lock_targets", both + only_targets), (ik, "rg_foot_lock_ik", both + only_ik)):
        for kw, text in cases:
            with pytest.raises(rg.capi.RgError, match=text) as info:
                fn(**kw)
            assert name in str(info.value), (kw, str(info.value))
    torch.cuda.synchronize()
    assert (offsets == -7.0).all() and (stats == -7.0).all() and (out == -7.0).all() and (reach == -7.0).all()    # nothing was launched
    targets()
    ik(offsets=offsets)
    want, want_stats, _ = ref.targets(data["joints"][:8], data["contact"][:8], lens, blend=3)
    assert np.array_equal(stats.cpu().numpy()[:, :3], want_stats[:, :3])
    assert np.abs(offsets.cpu().numpy() - want).max() <= 10 * U * np.abs(data["joints"][:8, ANKLES]).max()
    assert torch.isfinite(out).all() and torch.equal(out[:, OTHER], P[:, OTHER]) and (reach >= 0).all()
    ik(stretch=1.0)                                               # the closed end of (0, 1]
