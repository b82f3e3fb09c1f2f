"""Generates tests/golden/fgd_eval.npz: the reference's FGD path (tools/evaluate.py:255-275 and :436) on seeded data.

    python tests/golden/make_fgd_golden.py

Builds the reference's VAESKConv (mogen/models/eval_models) on CPU.  Its topology comes from a temporary npz holding only the
55-entry SMPL-X kintree_table (a data fact of the body model, not reference source), so no SMPL-X model file is needed.  The
parameters and the axis-angle clips are drawn from seeds by fgd_fixture.py and are NOT stored; stored are the model's masks and
pool matrices, checksums of the regenerated inputs, the reference's per-clip latents in fp64 (and how far its own fp32 run is
from them), and reference frechet_distance values on the latents and on random latent sets.
Runs only where the reference exists; nothing on the GPU box imports this file.
"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

sys.dont_write_bytecode = True   # the reference is read-only: no __pycache__ there
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402
import fgd_fixture as fx  # noqa: E402

# SMPL-X kintree_table[0] (parents of the 55 joints; the root's entry is unused by build_edge_topology)
SMPLX_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
                 20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38,
                 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53]


def main():
    ns = _ref_import.load_reference()
    _ref_import._pkg("mogen.models.eval_models", os.path.join(_ref_import.REF_ROOT, "mogen", "models", "eval_models"))
    model = importlib.import_module("mogen.models.eval_models.model")
    metric = importlib.import_module("mogen.models.utils.metric")
    rc = ns.rc

    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "smplx_models", "smplx"))
    np.savez(os.path.join(tmp, "smplx_models", "smplx", "SMPLX_NEUTRAL_2020.npz"),
             kintree_table=np.array([SMPLX_PARENTS, list(range(55))], dtype=np.int64))
    args = types.SimpleNamespace(deps_path=tmp + "/", variational=False, vae_test_len=32, vae_test_dim=330, vae_test_stride=20,
                                 vae_length=240, vae_layer=4, vae_grow=[1, 1, 2, 1])     # tools/evaluate.py:87-97
    torch.manual_seed(0)
    net = model.VAESKConv(args).eval()
    out = {}
    structure = {}
    for k, v in net.state_dict().items():
        if k.startswith("encoder.") and (k.endswith(".mask") or ".common.0." in k):
            structure[k] = v.numpy().astype(np.float32)
            out["sd/" + k] = structure[k]
    params = fx.encoder_params(structure)
    sd = net.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in params.items()})
    net.load_state_dict(sd)
    net64 = model.VAESKConv(args).double().eval()
    net64.load_state_dict(net.state_dict())
    out["param_checksum"] = np.float64(fx.checksum([params[k] for k in sorted(params)]))

    sets = fx.clip_sets()
    lat_all, lat_all64 = {}, {}
    for name, clips in sets.items():
        out["%s_clip_checksum" % name] = np.float64(fx.checksum(clips))
        lat32, lat64, rel = [], [], []
        for i, aa in enumerate(clips):
            n = min(aa.shape[0], fx.EVAL_N)
            with torch.no_grad():
                for dt, net_, dst in ((torch.float32, net, lat32), (torch.float64, net64, lat64)):
                    p = torch.from_numpy(aa[:n]).to(dt).reshape(1 * n, 55, 3)             # tools/evaluate.py:255-264
                    p = rc.matrix_to_rotation_6d(rc.axis_angle_to_matrix(p)).reshape(1, n, 330)
                    remain = n % fx.WINDOW                                                # :267-275
                    dst.append(net_.map2latent(p[:, :n - remain]).reshape(-1, 240).numpy())
            out["%s_lat64_%d" % (name, i)] = lat64[-1]
            rel.append(np.linalg.norm(lat32[-1].astype(np.float64) - lat64[-1]) / np.linalg.norm(lat64[-1]))
        out["%s_ref32_rel" % name] = np.array(rel)               # the reference's own fp32 run against its fp64 run, per clip
        lat_all[name], lat_all64[name] = np.concatenate(lat32, 0), np.concatenate(lat64, 0)
    out["n_clips"] = np.int64(len(sets["pred"]))
    out["fgd_e2e"] = np.float64(metric.FIDCalculator.frechet_distance(lat_all["pred"], lat_all["gt"]))    # :436
    out["fgd_e2e_lat64"] = np.float64(metric.FIDCalculator.frechet_distance(lat_all64["pred"], lat_all64["gt"]))
    for n, seed in fx.FD_SETS:
        a, b = fx.random_latents(n, seed)
        out["fd_seed_%d" % n] = np.int64(seed)
        out["fd_checksum_%d" % n] = np.float64(a.sum() + 2.0 * b.sum())
        out["fd_%d" % n] = np.float64(metric.FIDCalculator.frechet_distance(a, b))
    np.savez_compressed(os.path.join(HERE, "fgd_eval.npz"), **out)
    print("fgd_e2e", out["fgd_e2e"], out["fgd_e2e_lat64"], {n: out["fd_%d" % n] for n, _ in fx.FD_SETS})


if __name__ == "__main__":
    main()
