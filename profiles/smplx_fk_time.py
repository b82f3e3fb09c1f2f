"""The three launches that run the SMPL-X forward kinematics at the evaluation's own shape, 256 clips of 300 frames (NOTEBOOK.md
section 24): rg_smplx_joints, rg_smplx_joints_expr (expressions and translation) and rg_mesh_transforms (every joint active,
expressions, the joints output), each after a warm-up with device events around 20 launches at a time, 5 times; the median counts.
Uses only the C entry points and capi, so any tree of this project that has them can be timed.  Prints one JSON line; --out FILE
also writes it.

    python profiles/smplx_fk_time.py [--root TREE] [--out FILE]       # TREE: the checkout whose library is timed (default: this one)
"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_CLIPS, FRAMES, NJ, NEXPR = 256, 300, 55, 100
PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15, 20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34,
           35, 20, 37, 38, 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53]             # SMPL-X kintree_table[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    rg = importlib.import_module("rag-gesture_amd")
    assert os.path.dirname(os.path.dirname(os.path.abspath(rg.__file__))) == root, rg.__file__
    capi = rg.capi
    h, dev = capi.get_handle(0), torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    R = N_CLIPS * FRAMES
    up = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    poses, exprs = up(rng.uniform(-0.6, 0.6, (R, NJ * 3))), up(rng.standard_normal((R, NEXPR)))
    transl, rest = up(rng.uniform(-1, 1, (R, 3))), up(rng.uniform(-1, 1, (N_CLIPS, NJ, 3)))
    j_expr, pose_mean = up(rng.standard_normal((NJ, 3, NEXPR)) * 1e-3), up(rng.uniform(-0.3, 0.3, NJ * 3))
    parents_host = np.array(PARENTS, np.int32)
    off_host = (np.arange(N_CLIPS + 1) * FRAMES).astype(np.int32)
    parents, off = up(parents_host, np.int32), up(off_host, np.int32)
    joints = torch.empty(R, NJ, 3, device=dev)
    k_pad = -(-(NEXPR + 9 * (NJ - 1)) // 16) * 16
    pf_host = np.array([-1] + [NEXPR + 9 * i for i in range(NJ - 1)], np.int32)
    pf = up(pf_host, np.int32)
    coeff, A = torch.zeros(-(-R // 64) * 64, k_pad, device=dev), torch.empty(R, NJ, 12, device=dev)
    common = dict(poses=poses.data_ptr(), pose_mean=pose_mean.data_ptr(), parents=parents.data_ptr(),
                  parents_host=parents_host.ctypes.data, clip_off=off.data_ptr(), clip_off_host=off_host.ctypes.data,
                  joints=joints.data_ptr(), n_clips=N_CLIPS, fold=1)
    blocks = {
        "smplx_joints": capi.struct("rg_smplx_joints_args")(rest=rest.data_ptr(), **common),
        "smplx_joints_expr": capi.struct("rg_smplx_joints_expr_args")(
            rest=rest.data_ptr(), exprs=exprs.data_ptr(), transl=transl.data_ptr(), j_expr=j_expr.data_ptr(), raw_off=off.data_ptr(),
            raw_off_host=off_host.ctypes.data, raw_rows=R, stride=1, **common),
        "mesh_transforms": capi.struct("rg_mesh_transforms_args")(
            j_clip=rest.data_ptr(), exprs=exprs.data_ptr(), j_expr=j_expr.data_ptr(), pf_col=pf.data_ptr(),
            pf_col_host=pf_host.ctypes.data, coeff=coeff.data_ptr(), A=A.data_ptr(), k_pad=k_pad, **common)}
    out = dict(root=os.path.basename(root), clips=N_CLIPS, frames=FRAMES)
    for name, a in blocks.items():
        launch = lambda: h.call(name, ctypes.byref(a))
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                launch()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / 20.0 * 1e3)
        out[name] = dict(launch_us=times, median_us=float(np.median(times)), checksum=float(joints.double().sum().item()))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
