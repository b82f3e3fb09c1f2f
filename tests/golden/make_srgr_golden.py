"""Generates tests/golden/srgr.npz: the reference's own tools/evaluate.py Evaluator.evaluate() with calculate_srgr=True on a
fixture folder (srgr_fixture.py, written by packing.save_sample_files).

    python tests/golden/make_srgr_golden.py

The stub modules are those of make_joint_metrics_golden.py (smplx.create -> smplx_fk.py in float64 returned as float32, librosa,
soundfile, mogen.datasets).  What they lack for SRGR is patched in here at run time: mmcv.Config.fromfile returns an object with
.data.test and .motion_fps, and mogen.datasets.build_dataset returns a dict "<dir>/<dir>" -> {"sem_score": tensor}, so that
evaluate.py:140-143 and :413-426 run unchanged and `srgr score:` is read from what the reference prints.

The seed is the first one for which every joint-frame's |diff - 0.3| is at least MARGIN (fp32 forward kinematics on the device
then cannot flip a decision) and the share of successful joint-frames lies strictly between 0.2 and 0.8.  Stored: the seed, that
margin, the share, the printed scores at motion_fps 15 and 30, per clip the rate of metric.SRGR.run and the success count, the
sem vectors as the reference resampled them, and the stub's joints of the first two clips.  Runs only where the reference exists.
"""
import contextlib
import importlib
import io
import os
import re
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

sys.dont_write_bytecode = True   # the reference is read-only: no __pycache__ there
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402
import fgd_fixture  # noqa: E402
import make_joint_metrics_golden as mj  # noqa: E402
import srgr_fixture as sf  # noqa: E402

N_STORED = 2                      # clips whose pred / gt joints are stored
MARGIN = 1e-3                     # smallest |diff - 0.3| over every joint-frame
THRESHOLD = 0.3
FIRST_SEED = 900
MAX_SEEDS = 20000


def _diffs(rc, model, inp):
    """Per clip (pred joints, gt joints) [n, 165] float32 of the reference's pipeline and diff [n, 55] as metric.py:41."""
    out = []
    for i in range(sf.N_CLIPS):
        jr = mj._ref_joints(rc, model, inp["pred"][i][:sf.EVAL_N], inp["betas"][i])
        jt = mj._ref_joints(rc, model, inp["gt"][i][:sf.EVAL_N], inp["betas"][i])
        out.append((jr, jt, np.sum(abs(jr.reshape(-1, 55, 3) - jt.reshape(-1, 55, 3)), 2)))
    return out


def _resample(sem, motion_fps):
    """evaluate.py:416-423."""
    t = torch.from_numpy(np.asarray(sem, np.float32)).unsqueeze(0).unsqueeze(0)
    if motion_fps != 30:
        t = torch.nn.functional.interpolate(t, scale_factor=30 / motion_fps, mode="linear")
    return t.squeeze(0).squeeze(0).cpu().numpy()


def main():
    ns = _ref_import.load_reference()
    rc = ns.rc
    _ref_import._pkg("mogen.models.eval_models", os.path.join(_ref_import.REF_ROOT, "mogen", "models", "eval_models"))
    packing = mj._load_packing()
    tmp = tempfile.mkdtemp()
    try:
        deps = os.path.join(tmp, "deps") + "/"
        os.makedirs(os.path.join(deps, "smplx_models", "smplx"))
        model_path = os.path.join(deps, "smplx_models", "smplx", "SMPLX_NEUTRAL_2020.npz")
        np.savez(model_path, **sf.jf.smplx_model())
        model = mj._install_stubs(model_path)
        # what the stubs lack for calculate_srgr (evaluate.py:140-143)
        cfg = types.SimpleNamespace(data=types.SimpleNamespace(test=None), motion_fps=sf.MOTION_FPS)
        dataset = {}
        sys.modules["mmcv"].Config = types.SimpleNamespace(fromfile=lambda path: cfg)
        sys.modules["mogen.datasets"].build_dataset = lambda test_cfg: dataset
        metric = importlib.import_module("mogen.models.utils.metric")
        evaluate = mj._load_tool("evaluate")
        model_mod = importlib.import_module("mogen.models.eval_models.model")

        for seed in range(FIRST_SEED, FIRST_SEED + MAX_SEEDS):
            inp = sf.inputs(seed)
            d = np.concatenate([x[2] for x in _diffs(rc, model, inp)]).astype(np.float64)
            margin, share = float(np.abs(d - THRESHOLD).min()), float((d < THRESHOLD).mean())
            if margin >= MARGIN and 0.2 < share < 0.8:
                break
        else:
            raise RuntimeError("no seed keeps the margin")
        print("seed", seed, "margin", margin, "share", share)

        ev_root = os.path.join(tmp, "eval")
        names = sf.write_folder(ev_root, inp, packing.save_sample_files)
        np.save(os.path.join(tmp, "avg_vel.npy"), sf.jf.avg_vel(inp, model))
        args = types.SimpleNamespace(deps_path=deps, variational=False, vae_test_len=32, vae_test_dim=330, vae_test_stride=20,
                                     vae_length=240, vae_layer=4, vae_grow=[1, 1, 2, 1])
        torch.manual_seed(0)
        net = model_mod.VAESKConv(args)
        sd = net.state_dict()
        structure = {k: v.numpy().astype(np.float32) for k, v in sd.items()
                     if k.startswith("encoder.") and (k.endswith(".mask") or ".common.0." in k)}
        sd.update({k: torch.from_numpy(v) for k, v in fgd_fixture.encoder_params(structure).items()})
        ckpt = os.path.join(tmp, "fgd.bin")
        torch.save({"model_state": sd}, ckpt)
        args.__dict__.update(npz_folder_path=ev_root, e_path=ckpt, avg_vel_path=os.path.join(tmp, "avg_vel.npy"),
                             speaker_specific=None, eval_n=sf.EVAL_N, calculate_srgr=True, audio_sr=16000, pose_fps=30,
                             device=torch.device("cpu"), test_cfg="unused.py")       # evaluate.py:50-104 without parse_args

        out = dict(seed=np.int64(seed), margin=np.float64(margin), share=np.float64(share), clip_names=np.array(names))
        per_clip = _diffs(rc, model, inp)
        for fps, tag in ((sf.MOTION_FPS, ""), (30, "_30")):
            sems = sf.sem_scores(seed, fps)
            cfg.motion_fps = fps
            dataset.clear()
            dataset.update({name: {"sem_score": torch.from_numpy(s)} for name, s in zip(names, sems)})
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf), torch.no_grad():
                evaluate.Evaluator(args).evaluate()
            text = buf.getvalue()
            sys.stderr.write(text)
            score = float(re.search(r"^srgr score: (\S+)$", text, flags=re.M).group(1))
            rates, counts = [], []
            for i, (jr, jt, diff) in enumerate(per_clip):
                n = jr.shape[0]
                sem30 = _resample(sems[i], fps)
                rates.append(metric.SRGR(threshold=0.3, joints=55).run(jr, jt, sem30))
                ones = metric.SRGR(threshold=0.3, joints=55).run(jr, jt, np.full(n, 0.165))     # success count / (n * 55)
                counts.append(int(round(ones * n * 55)))
                assert counts[-1] == int((diff < THRESHOLD).sum())
                out["sem30%s_%d" % (tag, i)] = sem30.astype(np.float32)
            assert abs(sum(r * sf.EVAL_N for r in rates) / (sf.EVAL_N * sf.N_CLIPS) - score) <= 1e-12 * max(score, 1e-300)
            out["score" + tag] = np.float64(score)
            out["rate" + tag] = np.asarray(rates, np.float64)
            out["count"] = np.asarray(counts, np.int64)
        assert abs(out["count"].sum() / (sf.EVAL_N * sf.N_CLIPS * 55) - share) < 1e-12
        out["joints_pred"] = np.stack([x[0] for x in per_clip[:N_STORED]])            # [N_STORED, n, 165] float32
        out["joints_gt"] = np.stack([x[1] for x in per_clip[:N_STORED]])
        path = os.path.join(HERE, "srgr.npz")
        np.savez_compressed(path, **out)
        print({k: out[k] for k in ("score", "score_30", "rate", "count")}, os.path.getsize(path))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
