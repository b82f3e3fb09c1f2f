"""Call times of foot skating and contact planting (rag-gesture_amd/foot.py) on synthetic clips (the SMPL-X model and the smooth
poses of tests/golden/joint_fixture.py, random-walk translations, random flags), at two sizes: 32 clips of 150 frames (a batch
at the motion rate) and one clip of 18 000 frames (a 10-minute recording at 30 fps: one workgroup walking 71 tiles).
  device_ms   device events around the forward kinematics (SMPLXJoints.joints_strided on device tensors), foot.skate_sums
              (which ends in its read-back) and foot.plant_translation; warm, REPEATS repeats, the median and the parts
  fixture_s   the float64 restatement on the CPU of the same run, once: tests/golden/smplx_fk.py, then tests/foot_ref.py
These are call times of latency-bound launches, not a share of any peak.  Prints one JSON line; --out FILE also writes it.

    python profiles/foot_time.py [--out FILE]
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
    jf, fk, ref = _load("golden/joint_fixture.py", "joint_fixture"), _load("golden/smplx_fk.py", "smplx_fk"), _load("foot_ref.py", "foot_ref")
    model = jf.smplx_model()
    smplx = rg.smplx.SMPLXJoints(model)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    out = dict(repeats=REPEATS, sizes={})
    for tag, lens in SIZES:
        rng = np.random.default_rng(len(lens))
        poses = np.concatenate([jf.smooth_clip(rng, n) for n in lens])
        transl = np.concatenate([np.cumsum(rng.standard_normal((n, 3)) * 0.01, 0) for n in lens]).astype(np.float32)
        flags = np.where(rng.random((sum(lens), 4)) < 0.5, rng.uniform(0.75, 1, (sum(lens), 4)), rng.uniform(0, 0.25, (sum(lens), 4))).astype(np.float32)
        P, T, C = (torch.from_numpy(a).cuda() for a in (poses, transl, flags))
        off = rg.smplx.offsets(lens)
        rows = dict(total=[], fk=[], sums=[], plant=[])
        for r in range(REPEATS + 3):
            e = [ev() for _ in range(4)]
            e[0].record()
            joints = smplx.joints_strided(P, None, T, off, off, 1)
            e[1].record()
            sums = rg.foot.skate_sums(joints, lens, C)
            e[2].record()
            planted = rg.foot.plant_translation(joints, C, T, lens)
            e[3].record()
            torch.cuda.synchronize()
            if r >= 3:                                             # (the first rounds warm every code object and the allocator)
                rows["total"].append(e[0].elapsed_time(e[3]))
                for k, i in (("fk", 0), ("sums", 1), ("plant", 2)):
                    rows[k].append(e[i].elapsed_time(e[i + 1]))
        res = dict(clips=len(lens), frames=int(sum(lens)), device_ms_median={k: statistics.median(v) for k, v in rows.items()},
                   device_ms_min_max={k: [min(v), max(v)] for k, v in rows.items()})
        m = fk.load_model(model)
        stages = {}
        t0 = time.perf_counter()
        a = 0
        jd = []
        for n in lens:
            jd.append(fk.posed_joints(poses[a:a + n], fk.rest_joints(m), m["parents"], m["pose_mean"]) + transl[a:a + n, None, :].astype(np.float64))
            a += n
        stages["fk"] = time.perf_counter() - t0
        jh = joints.cpu().numpy()                                   # the restatement of the two kernels reads the device's joints
        t0 = time.perf_counter()
        want = ref.skate_sums(jh, lens, flags)
        stages["sums"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        wantp = ref.plant(jh, flags, transl, lens)
        stages["plant"] = time.perf_counter() - t0
        res["fixture_s"], res["fixture_stage_s"] = sum(stages.values()), stages
        res["joints_worst_abs_difference_from_float64"] = float(np.abs(jh - np.concatenate(jd)).max())
        res["counts_equal"] = bool(np.array_equal(sums[:, [0, 1, 2, 4, 6]], want[:, [0, 1, 2, 4, 6]]))
        res["sums_worst_relative_difference"] = float(np.max(np.abs(sums[:, [3, 5]] - want[:, [3, 5]]) / want[:, [3, 5]]))
        res["planting_worst_difference_in_fp32_roundings"] = float(
            (np.abs(planted.cpu().numpy().astype(np.float64) - wantp) / (2.0 ** -23 * np.maximum(np.abs(wantp.astype(np.float64)), 2.0 ** -126))).max())
        res["metrics"] = ref.metrics(sums, flags=True)
        out["sizes"][tag] = res
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
