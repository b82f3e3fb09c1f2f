"""Generates tests/golden/face_metrics.npz: the l2 loss / lvel loss that the reference's own tools/evaluate.py
Evaluator.evaluate() prints on a fixture folder (face_fixture.py, written by packing.save_sample_files).

    python tests/golden/make_face_metrics_golden.py

The reference needs smplx, librosa, soundfile and the mmcv dataset; they are replaced by the stubs of
make_joint_metrics_golden.py, except that smplx.create returns a module running smplx_lbs.py (float64 linear blend skinning
of the fixture model with expressions and pose blend shapes), whose vertices and joints are returned as float32.  The FGD
checkpoint comes from fgd_fixture.py, the audio and avg_vel only keep the other scores of evaluate.py running.  Stored: the
printed l2 / lvel, the same two from smplx_lbs.py in float64 (the reference's formulas), and the seed.  Runs only where the
reference exists.
"""
import contextlib
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
import face_fixture as ff  # noqa: E402
import fgd_fixture  # noqa: E402
import joint_fixture as jf  # noqa: E402
import make_joint_metrics_golden as mj  # noqa: E402
import smplx_lbs  # noqa: E402


class _StubSMPLX(torch.nn.Module):
    def __init__(self, model):
        super().__init__()
        self.m = model

    def forward(self, betas, transl, expression, jaw_pose, global_orient, body_pose, left_hand_pose, right_hand_pose,
                leye_pose, reye_pose, return_joints=True, return_verts=False, **kw):
        f = lambda t: t.detach().cpu().double().numpy()
        full = np.concatenate([f(global_orient), f(body_pose), f(jaw_pose), f(leye_pose), f(reye_pose), f(left_hand_pose),
                               f(right_hand_pose)], 1)           # SMPLX.forward full_pose order
        b = f(betas)
        if not np.all(b == b[:1]):
            raise RuntimeError("the stub expects one betas vector per call")
        verts, joints = smplx_lbs.lbs(self.m, full, b[0], f(expression), f(transl))
        out = np.zeros((full.shape[0], 127, 3))
        out[:, :55] = joints + f(transl)[:, None]
        return {"joints": torch.from_numpy(out.astype(np.float32)), "vertices": torch.from_numpy(verts.astype(np.float32))}


def main():
    ns = _ref_import.load_reference()
    del ns
    _ref_import._pkg("mogen.models.eval_models", os.path.join(_ref_import.REF_ROOT, "mogen", "models", "eval_models"))
    packing = mj._load_packing()
    tmp = tempfile.mkdtemp()
    try:
        deps = os.path.join(tmp, "deps") + "/"
        os.makedirs(os.path.join(deps, "smplx_models", "smplx"))
        model_path = os.path.join(deps, "smplx_models", "smplx", "SMPLX_NEUTRAL_2020.npz")
        raw = ff.smplx_model()
        np.savez(model_path, **raw)
        mj._install_stubs(model_path)                                   # librosa, soundfile, mmcv dataset (and a joint smplx)
        model = smplx_lbs.load_model(model_path)
        _ref_import._stub("smplx", create=lambda *a, **k: _StubSMPLX(model))
        evaluate = mj._load_tool("evaluate")
        import importlib
        model_mod = importlib.import_module("mogen.models.eval_models.model")

        inp = ff.inputs(ff.SEED)
        ev_root = os.path.join(tmp, "eval")
        names = ff.write_folder(ev_root, inp, packing.save_sample_files)
        n_samples = int(jf.AUDIO_SR / jf.POSE_FPS * ff.N_FRAMES)
        for i, name in enumerate(names):
            jf.write_wav(os.path.join(ev_root, name, "gt_audio.wav"), n_samples, np.array([8000 + 3000 * i, 20000]))
        np.save(os.path.join(tmp, "avg_vel.npy"), np.ones(55))

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
                             speaker_specific=None, eval_n=ff.EVAL_N, calculate_srgr=False, audio_sr=16000, pose_fps=30,
                             device=torch.device("cpu"), test_cfg=None)          # evaluate.py:50-104 without parse_args
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), torch.no_grad():
            evaluate.Evaluator(args).evaluate()
        text = buf.getvalue()
        sys.stderr.write(text)
        l2 = float(re.search(r"^l2 loss: (\S+)$", text, flags=re.M).group(1))
        lvel = float(re.search(r"^lvel loss: (\S+)$", text, flags=re.M).group(1))
        r_l2, r_lvel = ff.restated_scores(raw, inp)
        out = dict(seed=np.int64(ff.SEED), score_l2=np.float64(l2), score_lvel=np.float64(lvel), f64_l2=np.float64(r_l2),
                   f64_lvel=np.float64(r_lvel), clip_names=np.array(names))
        path = os.path.join(HERE, "face_metrics.npz")
        np.savez_compressed(path, **out)
        print(out, os.path.getsize(path))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
