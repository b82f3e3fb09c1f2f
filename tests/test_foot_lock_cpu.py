"""No GPU: the foot lock -- the header and the library's exports, the conditions the seeded fixture must meet
so that kernel and restatement take every branch alike, the restatement's own properties (the walker among them), and the
classes without a device.  The kernels are tested in test_foot_lock_gpu.py."""
import functools
import importlib
import importlib.util
import inspect
import os

import numpy as np
import pytest

import foot_lock_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fx = _load("foot_lock_fixture")


@functools.lru_cache(None)
def model():
    m = ref.fk.load_model(fx.smplx_model())
    return ref.fk.rest_joints(m), m["parents"], m["pose_mean"]


@functools.lru_cache(None)
def locked(which, fk32=False):
    """The restatement on the parity clips, the walker, the out-of-reach clip or the straight-legged clip (computed once; callers must not write)."""
    rest, parents, pose_mean = model()
    if which == "clips":
        poses, transl, contact, lens = fx.clips()
    elif which == "walker":
        poses, transl, contact, _ = fx.walker()
        lens = [poses.shape[0]]
    else:
        poses, transl, contact = fx.straight_clip() if which == "straight" else fx.far_clip()
        lens = [poses.shape[0]]
    r = ref.lock(poses, transl, contact, lens, rest, parents, pose_mean, blend=fx.BLEND, fk32=fk32)
    r.update(inputs=(poses, transl, contact, lens))
    return r


def sensitivity():
    """max over the fixture of |restatement on exact transforms - restatement on transforms stored as fp32|, per pose channel
    (rad): what the fp32 forward kinematics of the kernel may cost, before its sinf / cosf."""
    return max(float(np.abs(locked(w)["poses"] - locked(w, True)["poses"]).max()) for w in ("clips", "walker", "far", "straight"))


# --------------------------------------------------------------------------------------------------------------------- the ABI
def test_header_declares_the_entry_points(rg):
    capi = rg.capi
    assert {"rg_foot_lock_targets", "rg_foot_lock_ik"} <= set(capi.header_symbols())
    assert capi.header_version() >= 135 and capi.header_constants()["RG_FOOT_LOCK_STATS"] == 5 == ref.LOCK_STATS == rg.foot.LOCK_STATS
    assert len(capi.header_structs()) == 23                      # plain arguments: no new argument block
    protos = capi.header_prototypes()
    assert len(protos["rg_foot_lock_targets"][1]) == 11 and len(protos["rg_foot_lock_ik"][1]) == 15
    assert (rg.foot.CONTACT_FLAG, rg.foot.LOCK_BLEND, rg.foot.LOCK_STRETCH) == (ref.CONTACT_FLAG, ref.BLEND, ref.STRETCH)
    assert rg.foot.CONTACT_JOINTS[:2] == (ref.LEGS[0][2], ref.LEGS[1][2]) and fx.BLEND == ref.BLEND


def test_library_exports_the_entry_points(rg):
    lib = rg.capi.load_library()
    assert hasattr(lib, "rg_foot_lock_targets") and hasattr(lib, "rg_foot_lock_ik")
    assert lib.rg_version() == rg.capi.header_version()


def test_unit_is_built_with_the_default_flags(rg):
    b = importlib.import_module("rag-gesture_amd.build")
    src = os.path.join(b.CSRC, "rg_footlock.hip")
    assert src in b.sources() and b.flags_for(src) == b.FLAGS and "rg_footlock.hip" not in b.PACKED_FP32_UNITS
    assert os.path.join(b.CSRC, "rg_smplx.h") in b.deps(src)     # the shared forward kinematics
    assert os.path.join(b.CSRC, "rg_legik.h") in b.deps(src)     # the solve, which the host test below compiles too
    with open(src) as f:
        text = f.read()
    assert "asm" not in text and "atomic" not in text


# --------------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_model_is_leg_shaped():
    rest, parents, pose_mean = model()
    assert rest.shape == (55, 3) and np.array_equal(rest, rest.astype(np.float32))      # the device's fp32 copy is exact
    for hip, knee, ankle in ref.LEGS:
        assert parents[knee] == hip and parents[ankle] == knee and parents[hip] == 0
        assert abs(np.linalg.norm(rest[knee] - rest[hip]) - fx.THIGH) < 1e-6 and abs(np.linalg.norm(rest[ankle] - rest[knee]) - fx.SHANK) < 1e-6
    assert not pose_mean[:75].any()                               # the hand means do not reach the legs


def test_fixture_covers_the_cases_and_stays_away_from_every_branch():
    """Kernel and restatement must take the same branch everywhere without leaning on equal rounding: flags away from 0.5, no
    reach within a relative 1e-6 of stretch, bend and swing well away from the fallbacks' thresholds; no unreachable frame in
    the parity clips and the walker, some in the separate clip; and the runs the tiles need."""
    poses, transl, contact, lens = fx.clips()
    assert tuple(lens) == (1, 2, 63, 64, 65, 150, 256, 257, 600) and poses.shape == (sum(lens), 165)
    assert poses.dtype == transl.dtype == contact.dtype == np.float32
    assert np.abs(contact[:, :2] - 0.5).min() >= 0.25
    off = np.concatenate([[0], np.cumsum(lens)])
    for i, n in enumerate(lens):
        c = contact[off[i]:off[i + 1]]
        m0, m1 = ref.members(c[:, 0]), ref.members(c[:, 1])
        if n == 1:
            assert not m0.any() and not m1.any()
            continue
        assert m0[0] and m1[n - 1]                                 # a run from frame 0, a run to the last frame
        if n >= 257:
            assert m0[250:257].all() and m0[256]                  # across the tile edge
        if n == 600:
            r1 = ref.runs(m1)
            assert any(s <= 100 and e >= 400 for s, e in r1)       # a run that carries through a whole tile
            assert m1[505:520].all() and any(s == 511 - 6 or (s < 512 <= e) for s, e in r1)
            gaps = {b[0] - a[1] - 1 for a, b in zip(r1[:-1], r1[1:])} | {b[0] - a[1] - 1 for a, b in zip(ref.runs(m0)[:-1], ref.runs(m0)[1:])}
            assert min(gaps) < 2 * fx.BLEND < max(gaps)           # gaps shorter and longer than 2 blend
    stretch = ref.par(ref.STRETCH)
    for which, unreachable in (("clips", False), ("walker", False), ("far", True)):
        r = locked(which)
        solved = r["reach"] > 0
        assert solved.sum() == r["stats"][:, 2].sum() > 50
        over = int((r["reach"] > stretch).sum())
        assert (over > 10) if unreachable else over == 0, (which, over)
        assert np.abs(r["reach"][solved] / stretch - 1.0).min() > 1e-6
        bend = min(d["sin_bend"] for _, _, d in r["info"])
        swing = min(d["sin_swing"] for _, _, d in r["info"])
        print("%s: %d solves, %d out of reach, max reach %.4f, sin(bend) >= %.3e, sin(swing) >= %.3e"
              % (which, solved.sum(), over, r["reach"].max(), bend, swing))
        assert bend > 1000 * ref.STRAIGHT and swing > 1000 * ref.ON_LINE
        assert not any(d["straight"] or d["on_line"] for _, _, d in r["info"])


# --------------------------------------------------------------------------------------------- the restatement's properties
def test_restatement_meets_reachable_targets():
    """Through its own float64 forward kinematics the ankle lands on the target the solve aimed at within 1e-7 m (what is left
    is the +1e-8 inside SMPL-X's Rodrigues norm), and an out-of-reach target is approached along the hip-target line."""
    rest, parents, pose_mean = model()
    for which in ("clips", "walker", "far"):
        r = locked(which)
        poses, transl, contact, lens = r["inputs"]
        J = ref.world_joints(r["poses"], transl, rest, parents, pose_mean)
        J0 = ref.world_joints(poses, transl, rest, parents, pose_mean)
        ank = J[:, [ref.LEGS[0][2], ref.LEGS[1][2]]]
        err = np.linalg.norm(ank - r["aimed"], axis=2)
        ok = (r["reach"] > 0) & (r["reach"] <= ref.par(ref.STRETCH))
        print("%s: ankle to target %.3e m over %d reachable solves" % (which, err[ok].max(), ok.sum()))
        assert err[ok].max() <= 1e-7
        assert np.abs(J[:, [0, 1, 2]] - J0[:, [0, 1, 2]]).max() == 0.0          # pelvis and hips stay
        far = r["reach"] > ref.par(ref.STRETCH)
        if which == "far":
            hips = J[:, [ref.LEGS[0][0], ref.LEGS[1][0]]]
            leg = fx.THIGH + fx.SHANK
            want = hips + (r["aimed"] - hips) / np.linalg.norm(r["aimed"] - hips, axis=2, keepdims=True) * ref.par(ref.STRETCH) * leg
            assert far.sum() > 10 and np.linalg.norm(ank - want, axis=2)[far].max() <= 1e-6
            assert err[far].min() > 1e-4                           # not met


def test_restatement_changes_only_the_leg_channels():
    other = [c for c in range(165) if c not in ref.LEG_CHANNELS]
    assert len(ref.LEG_CHANNELS) == 18
    for which in ("clips", "walker"):
        r = locked(which)
        poses = r["inputs"][0]
        assert np.array_equal(r["poses"][:, other], poses[:, other].astype(np.float64))
        idle = ~(r["offsets"] != 0).any(2)                         # [F, 2]
        for k, leg in enumerate(ref.LEGS):
            ch = [3 * j + q for j in leg for q in range(3)]
            assert np.array_equal(r["poses"][idle[:, k]][:, ch], poses[idle[:, k]][:, ch].astype(np.float64))
        assert idle.any() and not idle.all()
    rest, parents, pose_mean = model()
    poses, transl, contact, lens = fx.clips()
    none = ref.lock(poses[:200], transl[:200], np.zeros_like(contact[:200]), [200], rest, parents, pose_mean)
    assert np.array_equal(none["poses"], poses[:200].astype(np.float64)) and not none["offsets"].any() and not none["stats"].any()
    toes = contact[:200].copy()
    toes[:, :2] = 0.0                                             # the toe flags alone lock nothing
    assert np.array_equal(ref.lock(poses[:200], transl[:200], toes, [200], rest, parents, pose_mean)["poses"], none["poses"])


def test_restatement_offsets_are_continuous():
    """Outside the runs an offset changes by at most max|d| / (blend + 1) per frame (per coordinate), also into and out of a
    run's end frames, wherever ONE run reaches the frames of the step: d = w d[e] and w changes by 1 / (blend + 1).  Where
    both neighbours reach a frame (a gap of at most 2 blend frames) the definition gives d = (w1 d[e] + w2 d[s']) / max(1, w1 +
    w2), whose step is at most (|d[e]| + |d[s']|) / (blend + 1) <= 2 max|d| / (blend + 1): the one-run bound cannot hold there
    (a gap of one frame between offsets +x and -x steps by x), so those steps are held to the two-run bound.  With blend = 0
    the offset is zero outside the runs."""
    r = locked("clips")
    poses, transl, contact, lens = r["inputs"]
    off = np.concatenate([[0], np.cumsum(lens)])
    one_run = two_runs = 0
    for i, n in enumerate(lens):
        d = r["offsets"][off[i]:off[i + 1]]
        for k in range(2):
            m = ref.members(contact[off[i]:off[i + 1], k])
            if n < 2:
                continue
            idx = np.arange(n)
            since = idx - np.maximum.accumulate(np.where(m, idx, -10 ** 6))            # frames since the last member frame
            until = np.minimum.accumulate(np.where(m, idx, 10 ** 6)[::-1])[::-1] - idx   # ... until the next one
            both = ~m & (since <= fx.BLEND) & (until <= fx.BLEND)
            step = np.abs(np.diff(d[:, k], axis=0)).max(1)
            outside = ~(m[:-1] & m[1:])
            two = outside & (both[:-1] | both[1:])
            bound = np.abs(d[:, k]).max() / (fx.BLEND + 1)
            assert (step[outside & ~two] <= bound * (1 + 1e-12)).all(), (n, k)
            assert (step[two] <= 2 * bound * (1 + 1e-12)).all(), (n, k)
            one_run, two_runs = one_run + int((outside & ~two).sum()), two_runs + int(two.sum())
    assert one_run > 200 and two_runs > 20
    d0, _, _ = ref.targets(r["joints"], contact, lens, blend=0)
    mem = np.stack([np.concatenate([ref.members(contact[off[i]:off[i + 1], k]) for i in range(len(lens))]) for k in range(2)], 1)
    assert not d0[~mem].any() and np.array_equal(d0[mem], r["offsets"][mem])


def test_restatement_walker():
    """The stance ankle slides by the drift before, and stands still over each run after the lock: through the float64
    forward kinematics within 2e-7 m (the fp32 rounding of the joints the anchors are taken from, 2^-24 * 1.6 m on either side of
    the run's mean).  The translation is not an output at all."""
    rest, parents, pose_mean = model()
    r = locked("walker")
    poses, transl, contact, lens = r["inputs"]
    _, _, _, which = fx.walker()
    n, P = poses.shape[0], fx.WALK_PERIOD
    J0 = ref.world_joints(poses, transl, rest, parents, pose_mean)
    J1 = ref.world_joints(r["poses"], transl, rest, parents, pose_mean)
    before = after = 0.0
    for r0 in range(0, n - 1, P):
        r1 = min(r0 + P, n - 1)
        assert (which[r0:r1] == which[r0]).all()
        j = ref.LEGS[which[r0]][2]
        before = max(before, np.abs(J0[r0:r1 + 1, j] - J0[r0, j]).max())
        after = max(after, np.abs(J1[r0:r1 + 1, j] - J1[r0, j]).max())
    print("walker: the stance ankle moves %.3f m over a run before, %.3e m after the lock" % (before, after))
    assert before > 0.3 and after <= 2e-7
    assert r["stats"][0, 1] == n // P and r["stats"][0, 0] == n - 1 + n // P - 1 + 1      # 7 runs; shared frames count twice


def test_sensitivity_is_what_fp32_transforms_cost():
    s = sensitivity()
    print("restatement on float64 transforms vs on fp32 transforms: %.3e rad per channel at most" % s)
    assert 1e-9 < s < 1e-5                                          # fp32 rounding of O(1) entries, amplified by the solve, not more


# -------------------------------------------------------------------------------------------------------------- the fallbacks
def test_restatement_takes_both_fallbacks_on_the_straight_clip():
    """Every solve of the straight-legged clip is a straight leg AND a target on the hip-ankle line, exactly (also with fp32
    transforms), far from the other side of either threshold; the leg bends about the hip's +x: hip and ankle turn by +A1, the
    knee by -2 A1 (thigh backwards, shank forwards -- the definition's choice, the reverse of the fixture's natural knees, whose
    hip channel is negative and knee channel positive), nothing turns about y or z, and through the float64 kinematics the
    ankle lands on its target, or at stretch (l1 + l2) straight below the hip."""
    rest, parents, pose_mean = model()
    for fk32 in (False, True):
        r = locked("straight", fk32)
        assert len(r["info"]) == 48 and all(d["straight"] and d["on_line"] for _, _, d in r["info"])
        assert all(d["sin_bend"] == 0.0 and d["sin_swing"] == 0.0 for _, _, d in r["info"])
    r = locked("straight")
    poses, transl, contact, lens = r["inputs"]
    stretch = ref.par(ref.STRETCH)
    far = r["reach"] > stretch
    assert far.sum() == 26 and (~far).sum() == 22 and np.abs(r["reach"] / stretch - 1).min() > 1e-3
    A1 = np.arccos(np.minimum(r["reach"], stretch))               # l1 = l2: cos A1 = dist / (l1 + l2)
    for k, (hip, knee, ankle) in enumerate(ref.LEGS):
        assert np.abs(r["poses"][:, 3 * hip] - A1[:, k]).max() < 1e-6 and np.abs(r["poses"][:, 3 * knee] + 2 * A1[:, k]).max() < 1e-6
        assert np.abs(r["poses"][:, 3 * ankle] - A1[:, k]).max() < 1e-6 and (r["poses"][:, 3 * hip] > 0.09).all()
        for j in (hip, knee, ankle):
            assert np.abs(r["poses"][:, 3 * j + 1:3 * j + 3]).max() < 1e-12
    J = ref.world_joints(r["poses"], transl, rest, parents, pose_mean)
    ank, hips = J[:, [7, 8]], J[:, [1, 2]]
    assert np.linalg.norm(ank - r["aimed"], axis=2)[~far].max() <= 1e-7
    below = hips - np.array([0.0, 1.0, 0.0]) * stretch * (fx.THIGH + fx.SHANK)
    assert np.linalg.norm(ank - below, axis=2)[far].max() <= 1e-6
    knees = J[:, [4, 5]]
    assert (knees[:, :, 2] < hips[:, :, 2] - 0.03).all()          # the knee goes backwards (z is forward)


def _host_solver(tmp_path):
    """csrc/rg_legik.h -- the source the kernel's lanes run -- compiled for the host: reads `L` + 9 numbers (log_map) or `S` + 4
    matrices, 4 points and stretch (leg_solve) per line, prints the results with 17 digits."""
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    csrc = os.path.join(os.path.dirname(HERE), "rag-gesture_amd", "csrc")
    src = tmp_path / "legik.cpp"
    src.write_text("""
#include <cstdio>
#include "rg_legik.h"
int main() {
  char kind;
  while (std::scanf(" %c", &kind) == 1) {
    if (kind == 'L') {
      m3 R;
      for (double& v : R.m) if (std::scanf("%lf", &v) != 1) return 1;
      double o[3];
      log_map(R, o);
      std::printf("%.17g %.17g %.17g\\n", o[0], o[1], o[2]);
    } else {
      m3 W[4];
      v3 p[4];
      double stretch, aa[9];
      for (m3& w : W) for (double& v : w.m) if (std::scanf("%lf", &v) != 1) return 1;
      for (v3& q : p) if (std::scanf("%lf %lf %lf", &q.x, &q.y, &q.z) != 3) return 1;
      if (std::scanf("%lf", &stretch) != 1) return 1;
      const double reach = leg_solve(W[0], W[1], W[2], W[3], p[0], p[1], p[2], p[3], stretch, aa);
      for (double v : aa) std::printf("%.17g ", v);
      std::printf("%.17g\\n", reach);
    }
  }
  return 0;
}
""")
    exe = tmp_path / "legik"
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", csrc, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(lines):
        text = "\n".join(" ".join([l[0]] + [repr(float(v)) for v in l[1:]]) for l in lines) + "\n"
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert out.returncode == 0
        return [np.array([float(v) for v in row.split()]) for row in out.stdout.splitlines()]
    return run


def _rot(axis, th):
    axis = np.asarray(axis, np.float64)
    return ref._rot(axis / np.linalg.norm(axis), th)


def test_the_kernels_solve_on_the_host_walks_every_branch(tmp_path):
    """The header the kernel's lanes run, compiled for the host, against the restatement within 1e-12 on every branch: log_map
    at the identity, next to zero (below its 1e-9), in the open interval, next to pi and at pi about three axes (the result
    must rotate back to the matrix); leg_solve on generic legs, on a straight leg with its target on the hip-ankle line (both
    fallbacks), in and out of reach, and with an ankle and a parent chosen so that the new ankle rotation is the identity
    (log_map next to zero) and the new hip rotation a half turn (log_map next to pi).  Poses stored as fp32 cannot reach those
    last two on the device; the same source does here."""
    run = _host_solver(tmp_path)
    rng = np.random.default_rng(19)
    mats = [np.eye(3)]
    for axis in ((1, 0, 0), (1, -2, 3), (-1, -1, 0.5)):
        mats += [_rot(axis, th) for th in (1e-10, 3e-10, 0.7, 2.9, np.pi - 1e-11, np.pi)]
    got = run([["L"] + list(R.ravel()) for R in mats])
    branches = set()
    for R, g in zip(mats, got):
        want = ref.log_map(R)
        r = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        branches.add("open" if np.linalg.norm(r) >= 1e-9 else ("zero" if np.trace(R) > 1 else "pi"))
        assert np.abs(g - want).max() <= 1e-12, (R, g, want)
        th = np.linalg.norm(g)
        assert th <= np.pi + 1e-12 and np.abs((_rot(g, th) if th > 0 else np.eye(3)) - R).max() <= 1e-9
    assert branches == {"open", "zero", "pi"}
    # leg_solve
    l = fx.THIGH
    a, down = np.array([0.38, 0.81, -0.2]), np.array([0.0, -1.0, 0.0])
    I = np.eye(3)
    straight = dict(Wp=I, Wh=I, Wk=I, Wa=I, a=a, b=a + l * down, c=a + 2 * l * down)
    cases = []
    for _ in range(6):                                            # generic bent legs, targets in reach
        Wh, Wk, Wa, Wp = (_rot(rng.standard_normal(3), rng.uniform(0.2, 1.5)) for _ in range(4))
        b = a + l * (Wh @ down)
        c = b + l * (Wk @ down)
        cases.append(dict(Wp=Wp, Wh=Wh, Wk=Wk, Wa=Wa, a=a, b=b, c=c, T=c + rng.uniform(-0.05, 0.05, 3)))
    cases.append(dict(straight, T=a + 0.7 * down))                # both fallbacks, in reach
    cases.append(dict(straight, T=a + 0.9 * down))                # both fallbacks, out of reach
    cases.append(dict(straight, T=a + 0.7 * down + np.array([0.1, 0.0, 0.05])))      # straight, off the line
    first = ref.solve_leg(I, I, I, I, a, straight["b"], straight["c"], a + 0.7 * down)[2]
    cases.append(dict(straight, T=a + 0.7 * down, Wa=first["Wk2"]))                   # the new ankle rotation is the identity
    cases.append(dict(straight, T=a + 0.7 * down, Wp=first["Wh2"] @ _rot((1, -2, 3), np.pi).T))      # the new hip rotation is a half turn
    order = ("Wp", "Wh", "Wk", "Wa", "a", "b", "c", "T")
    got = run([["S"] + [v for k in order for v in np.asarray(c[k]).ravel()] + [ref.par(ref.STRETCH)] for c in cases])
    flags = []
    for c, g in zip(cases, got):
        aa, reach, d = ref.solve_leg(*[c[k] for k in order])
        assert np.abs(g[:9] - aa.ravel()).max() <= 1e-12 and abs(g[9] - reach) <= 1e-15 and np.isfinite(g).all(), (c, g, aa)
        flags.append((bool(d["straight"]), bool(d["on_line"]), bool(reach > ref.par(ref.STRETCH))))
    assert [f[:2] for f in flags[:6]] == [(False, False)] * 6 and {f[2] for f in flags[:6]} == {False, True}
    assert flags[6:] == [(True, True, False), (True, True, True), (True, False, False), (True, True, False), (True, True, False)]
    assert np.abs(got[9][6:9]).max() <= 1e-12                     # log_map next to zero: no ankle rotation left
    assert abs(np.linalg.norm(got[10][:3]) - np.pi) <= 1e-9       # log_map next to pi: a half turn at the hip
    assert got[6][0] > 0 and got[6][3] < 0 and np.abs(got[6][[1, 2, 4, 5]]).max() <= 1e-12      # +x at the hip, -x at the knee


# ------------------------------------------------------------------------------------------------------------ the host side
def test_no_gpu_no_foot_lock(rg, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    class Model:
        device = None
    with pytest.raises(rg.capi.RgError, match="no GPU visible: FootLocker"):
        rg.foot.FootLocker(Model())
    with pytest.raises(rg.capi.RgError, match="no CPU path"):
        rg.foot.lock_targets(torch.zeros(2, 55, 3), torch.zeros(2, 4), [2])
    with pytest.raises(rg.capi.RgError, match="no CPU path"):
        rg.foot.lock_poses(Model(), torch.zeros(2, 165), torch.zeros(2, 3), torch.zeros(2, 2, 3, dtype=torch.float64), [2])


def test_the_layers_above_take_a_locker(rg):
    sig = inspect.signature(rg.packing.pack_outputs_locked)
    assert list(sig.parameters) == ["output", "locker", "motion_fps", "target_fps", "betas"]
    for fn in (rg.longform.LongformSynthesizer.run, rg.longform.LongformSynthesizer.run_many):
        p = inspect.signature(fn).parameters
        assert p["locker"].default is None and p["betas"].default is None
    sig = inspect.signature(rg.foot.FootLocker.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[2:]] == [("contact_threshold", 0.5), ("blend", 3), ("stretch", 0.995)]
