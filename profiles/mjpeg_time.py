"""The render tool on 4 clips x 64 frames of the full-size capsule figure at the default 640 x 960 panels (1280 x 960 frames), once
as PNG sequences (the host path: every frame copied to the host and deflated by zlib on one thread) and once as Motion-JPEG AVI
(video.write_mjpeg: encoded on the device), alternating, two rounds each after a warm-up (NOTEBOOK.md section 23).  Wall time is
a host clock around render_folder, which ends in a device synchronise; device_ms / encode_ms are the tool's own device events.
Prints one JSON line; --out FILE also writes it.

    python profiles/mjpeg_time.py [--out FILE]
"""
import argparse
import importlib
import importlib.util
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_CLIPS, FRAMES, ROUNDS = 4, 64, 2


def _fixture():
    spec = importlib.util.spec_from_file_location("render_fixture", os.path.join(ROOT, "tests", "golden", "render_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def tree_bytes(root, suffix):
    return sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(root) for f in fs if f.endswith(suffix))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    rg = importlib.import_module("rag-gesture_amd")
    rf = _fixture()
    out = dict(clips=N_CLIPS, frames_per_clip=FRAMES, width=1280, height=960, quality=90, png=[], mjpeg=[])
    with tempfile.TemporaryDirectory() as tmp:
        gts, preds = [rf.clip(40 + i, FRAMES) for i in range(N_CLIPS)], [rf.clip(60 + i, FRAMES) for i in range(N_CLIPS)]
        st = lambda cs, k: np.stack([c[k] for c in cs])
        exp = os.path.join(tmp, "exp")
        rg.packing.save_sample_files(exp, ["test/clip_%d" % i for i in range(N_CLIPS)],
                                     (st(preds, "poses"), st(preds, "expressions"), st(preds, "transl")),
                                     (st(gts, "poses"), st(gts, "expressions"), st(gts, "transl")))
        renderer = rg.render.SMPLXRenderer(rg.mesh.SMPLXMesh(rf.full_model()))
        warm = os.path.join(tmp, "warm")                                       # every code object and shape once, on one short clip
        rg.packing.save_sample_files(warm, ["test/w"], tuple(x[:1, :33] for x in (st(preds, "poses"), st(preds, "expressions"), st(preds, "transl"))),
                                     tuple(x[:1, :33] for x in (st(gts, "poses"), st(gts, "expressions"), st(gts, "transl"))))
        rg.render.render_folder(warm, renderer, png=True)
        rg.render.render_folder(warm, renderer, mjpeg=True)
        for _ in range(ROUNDS):
            for mode, kw, suffix in (("png", dict(png=True), ".png"), ("mjpeg", dict(mjpeg=True), ".avi")):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = rg.render.render_folder(exp, renderer, **kw)
                torch.cuda.synchronize()
                r["wall_s"] = time.perf_counter() - t0
                r["bytes_per_frame"] = tree_bytes(exp, suffix) / float(r["frames"])
                out[mode].append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
