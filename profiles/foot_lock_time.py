"""Call times of the foot lock (rag-gesture_amd/foot.py: lock_targets + lock_poses) on synthetic clips (the
leg-shaped model and the seeded clips of tests/golden/foot_lock_fixture.py), at two sizes: 32 clips of 150 frames (a batch at the
motion rate) and one clip of 18 000 frames (a 10-minute recording at 30 fps: one workgroup walking 71 tiles twice).
  device_ms   device events around the forward kinematics (SMPLXJoints.joints_strided on device tensors), foot.lock_targets
              (which ends in the read-back of its stats) and foot.lock_poses; beside them foot.plant_translation on the same
              joints and flags: the yardstick, there was no lock before.  Warm, REPEATS repeats, the median and the extremes
  fixture_s   the float64 restatement on the CPU of the same run, once: tests/foot_lock_ref.py
These are call times of latency-bound launches, not a share of any peak.  Prints one JSON line; --out FILE also writes it.

    python profiles/foot_lock_time.py [--out FILE]
"""
import argparse
import importlib
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REPEATS = 30
SIZES = (("32x150", [150] * 32), ("1x18000", [18000]))


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    rg = importlib.import_module("rag-gesture_amd")
    fx, ref = _load("golden/foot_lock_fixture.py", "foot_lock_fixture"), _load("foot_lock_ref.py", "foot_lock_ref")
    model = fx.smplx_model()
    smplx = rg.smplx.SMPLXJoints(model)
    m = ref.fk.load_model(model)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    out = dict(repeats=REPEATS, blend=fx.BLEND, sizes={})
    for tag, lens in SIZES:
        poses, transl, flags, _ = fx.clips(seed=len(lens), lens=lens)
        P, T, C = (torch.from_numpy(a).cuda() for a in (poses, transl, flags))
        off = rg.smplx.offsets(lens)
        rows = dict(total=[], fk=[], targets=[], ik=[], plant=[])
        for r in range(REPEATS + 3):
            e = [ev() for _ in range(5)]
            e[0].record()
            joints = smplx.joints_strided(P, None, T, off, off, 1)
            e[1].record()
            offsets, stats = rg.foot.lock_targets(joints, C, lens, blend=fx.BLEND)
            e[2].record()
            locked, reach = rg.foot.lock_poses(smplx, P, T, offsets, lens)
            e[3].record()
            planted = rg.foot.plant_translation(joints, C, T, lens)
            e[4].record()
            torch.cuda.synchronize()
            if r >= 3:                                             # (the first rounds warm every code object and the allocator)
                rows["total"].append(e[0].elapsed_time(e[3]))
                for k, i in (("fk", 0), ("targets", 1), ("ik", 2), ("plant", 3)):
                    rows[k].append(e[i].elapsed_time(e[i + 1]))
        res = dict(clips=len(lens), frames=int(sum(lens)), device_ms_median={k: statistics.median(v) for k, v in rows.items()},
                   device_ms_min_max={k: [min(v), max(v)] for k, v in rows.items()})
        jh = joints.cpu().numpy()                                   # the restatement takes its targets from the device's joints
        t0 = time.perf_counter()
        want = ref.lock(poses, transl, flags, lens, ref.fk.rest_joints(m), m["parents"], m["pose_mean"], blend=fx.BLEND, joints=jh)
        res["fixture_s"] = time.perf_counter() - t0
        got = locked.cpu().numpy().astype(np.float64)
        res["counts_equal"] = bool(np.array_equal(stats[:, :3], want["stats"][:, :3]))
        res["offsets_worst_abs_difference"] = float(np.abs(offsets.cpu().numpy() - want["offsets"]).max())
        res["pose_channels_worst_abs_difference_rad"] = float(np.abs(got - want["poses"]).max())
        res["solved_leg_frames"] = int((reach > 0).sum().item())
        res["unreachable"] = int((reach > np.float32(rg.foot.LOCK_STRETCH)).sum().item())
        res["max_reach"] = float(reach.max().item())
        res["stats_sum"] = [float(v) for v in stats.sum(0)[:4]] + [float(stats[:, 4].max())]
        out["sizes"][tag] = res
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
