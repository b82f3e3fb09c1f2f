"""GPU: SRGR on the device -- rg_srgr_clip_sums against the reference's per-clip rates and success counts on the reference's
own joints (tests/golden/srgr.npz, made by make_srgr_golden.py), against a float64 restatement on the shapes where the kernel
can go wrong, the margin that keeps fp32 forward kinematics from flipping a decision, and evaluate_folder end to end against
the score the reference printed."""
import importlib
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "srgr.npz")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


sf, fgdfx = _load("srgr_fixture"), _load("fgd_fixture")


@pytest.fixture(scope="module")
def ev():
    return importlib.import_module("rag-gesture_amd").evaluation


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def inp(gold):
    return sf.inputs(int(gold["seed"]))


@pytest.fixture(scope="module")
def sm(ev):
    return ev.SMPLXJoints(sf.jf.smplx_model())


# ------------------------------------------------------------------------------------------ 1. the reference's joints
def test_kernel_on_the_reference_joints(ev, gold):
    jp, jg = gold["joints_pred"], gold["joints_gt"]
    k, n = jp.shape[0], jp.shape[1]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda().reshape(k * n, 55, 3)
    for tag in ("", "_30"):
        w = np.concatenate([gold["sem30%s_%d" % (tag, i)][:n] for i in range(k)])
        wsum, count = ev.srgr_clip_sums(dev(jp), dev(jg), [n] * k, w)
        assert wsum.dtype == np.float64 and count.dtype == np.int64
        print("counts", count, "reference", gold["count"][:k])
        assert np.array_equal(count, gold["count"][:k])
        for i in range(k):
            rate = wsum[i] * (1 / 0.165) / (n * 55)
            print("clip %d rate%s %.17g reference %.17g" % (i, tag, rate, gold["rate" + tag][i]))
            assert rate == pytest.approx(float(gold["rate" + tag][i]), rel=1e-6)


# ------------------------------------------------------------------------------------------ 2. shapes
LENS = (1, 2, 33, 64, 65, 300)


def _case(seed, lens, nj, threshold):
    """pred / gt [sum lens, nj, 3] float32 whose L1 distances avoid the threshold by more than 1e-3, weights with zeros."""
    rng = np.random.default_rng(seed)
    F = sum(lens)
    gt = rng.standard_normal((F, nj, 3)).astype(np.float32)
    target = np.where(rng.random((F, nj)) < 0.5, rng.uniform(0.0, threshold - 0.01, (F, nj)),
                      rng.uniform(threshold + 0.01, 2 * threshold, (F, nj)))
    split = rng.dirichlet(np.ones(3), (F, nj)) * rng.choice([-1.0, 1.0], (F, nj, 3))
    pred = (gt + target[..., None] * split).astype(np.float32)
    w = (rng.integers(0, 11, F) / 10.0).astype(np.float32)
    w[rng.random(F) < 0.3] = 0.0
    d = np.abs(pred.astype(np.float64) - gt.astype(np.float64)).sum(-1)
    assert np.abs(d - threshold).min() > 1e-3 and 0.3 < (d < threshold).mean() < 0.7 and (w == 0).any() and (w > 0).any()
    return pred, gt, w, d


def _want(d, w, lens, threshold):
    off = np.concatenate([[0], np.cumsum(lens)])
    ok = d < threshold
    return (np.array([(ok[a:b] * w[a:b, None].astype(np.float64)).sum() for a, b in zip(off[:-1], off[1:])]),
            np.array([ok[a:b].sum() for a, b in zip(off[:-1], off[1:])], np.int64), off)


@pytest.mark.parametrize("nj,threshold", [(55, 0.3), (7, 0.5)])
def test_kernel_shapes_and_invariance(ev, nj, threshold):
    pred, gt, w, d = _case(11 + nj, LENS, nj, threshold)
    want_sum, want_count, off = _want(d, w, LENS, threshold)
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    kw = {} if (nj, threshold) == (55, 0.3) else dict(threshold=threshold, n_joints=nj)      # (the defaults are 0.3 and 55)
    wsum, count = ev.srgr_clip_sums(p, g, list(LENS), w, **kw)
    assert np.array_equal(count, want_count)
    for c in range(len(LENS)):
        assert wsum[c] == pytest.approx(want_sum[c], rel=1e-12, abs=0), c
    again = ev.srgr_clip_sums(p, g, list(LENS), w, **kw)
    assert np.array_equal(again[0], wsum) and np.array_equal(again[1], count)                 # run to run
    for c, n in enumerate(LENS):                                                               # alone = inside the batch
        a, b = off[c], off[c + 1]
        s1, c1 = ev.srgr_clip_sums(p[a:b].clone(), g[a:b].clone(), [n], w[a:b], **kw)
        assert s1[0] == wsum[c] and c1[0] == count[c], c
    if nj == 55:                                      # the other threshold on the same data gives other counts
        _, other = ev.srgr_clip_sums(p, g, list(LENS), w, threshold=0.45)
        assert np.array_equal(other, _want(d, w, LENS, 0.45)[1]) and (other >= count).all() and other.sum() > count.sum()


def test_kernel_rejects_bad_arguments(ev):
    x = torch.zeros(4, 55, 3, device="cuda")
    with pytest.raises(ValueError, match="joints must hold"):
        ev.srgr_clip_sums(x, x, [2, 2], np.zeros(3, np.float32))
    with pytest.raises(ValueError, match="n_joints must be at least 1"):
        ev.srgr_clip_sums(x, x, [4], np.zeros(4, np.float32), n_joints=0)
    s, c = ev.srgr_clip_sums(x, x, [0, 4], np.ones(4, np.float32))     # an empty clip: nothing to count
    assert s.tolist() == [0.0, 4.0 * 55] and c.tolist() == [0, 4 * 55]


# ------------------------------------------------------------------------------------------ 3. the margin
def test_device_joints_keep_the_margin(ev, gold, inp, sm):
    n, k = sf.EVAL_N, gold["joints_pred"].shape[0]
    clips = [inp["pred"][i][:n] for i in range(k)] + [inp["gt"][i][:n] for i in range(k)]
    j = sm.joints(clips, [inp["betas"][i] for i in range(k)] * 2, fold=True)
    want = np.concatenate([gold["joints_pred"], gold["joints_gt"]]).reshape(2 * k * n, 55, 3)
    err = float(np.abs(j.cpu().numpy().astype(np.float64) - want).max())
    print("largest joint error of the device FK %.3e, margin %.3e" % (err, float(gold["margin"])))
    # |dx| + |dy| + |dz| of a difference of two joints moves by at most 3 coordinates x 2 joints x err
    assert 6 * err < float(gold["margin"])
    w = np.concatenate([gold["sem30_%d" % i][:n] for i in range(k)])
    wsum, count = ev.srgr_clip_sums(j[:k * n], j[k * n:], [n] * k, w)
    assert np.array_equal(count, gold["count"][:k])
    for i in range(k):
        assert wsum[i] * (1 / 0.165) / (n * 55) == pytest.approx(float(gold["rate"][i]), rel=1e-6)


# ------------------------------------------------------------------------------------------ 4. end to end
@pytest.fixture(scope="module")
def folder(tmp_path_factory, inp):
    packing = importlib.import_module("rag-gesture_amd").packing
    root = tmp_path_factory.mktemp("srgr")
    sf.write_folder(str(root / "eval"), inp, packing.save_sample_files)
    return root


@pytest.fixture(scope="module")
def enc(ev):
    return ev.FGDEncoder(fgdfx.state_dict(np.load(os.path.join(HERE, "golden", "fgd_eval.npz"))))


def test_evaluate_folder_end_to_end(ev, gold, folder, enc, sm):
    seed, names = int(gold["seed"]), sf.clip_names()
    run = lambda **kw: ev.evaluate_folder(str(folder / "eval"), enc, eval_n=sf.EVAL_N, smplx=sm, **kw)
    plain = run()
    assert "srgr" not in plain
    sem15 = dict(zip(names, sf.sem_scores(seed, 15)))
    r = run(sem_scores=sem15, motion_fps=15)
    print("srgr %.17g reference %.17g" % (r["srgr"], float(gold["score"])))
    assert r["srgr"] == pytest.approx(float(gold["score"]), rel=1e-6)
    assert set(r) == set(plain) | {"srgr"} and all(r[k] == plain[k] for k in plain)
    assert run(sem_scores=sem15) == r                                                          # motion_fps defaults to 15
    r30 = run(sem_scores=dict(zip(names, sf.sem_scores(seed, 30))), motion_fps=30)
    print("srgr at 30 fps %.17g reference %.17g" % (r30["srgr"], float(gold["score_30"])))
    assert r30["srgr"] == pytest.approx(float(gold["score_30"]), rel=1e-6)
    assert all(r30[k] == plain[k] for k in plain)
    np.savez(str(folder / "sem.npz"), **sem15)
    assert run(sem_scores=str(folder / "sem.npz"), motion_fps=15) == r
    assert run(sem_scores=sem15, batch_clips=4)["srgr"] == pytest.approx(r["srgr"], rel=1e-14)  # two batches of clips
    # the plain FGD call is what it was
    assert set(ev.evaluate_folder(str(folder / "eval"), enc, eval_n=sf.EVAL_N)) == {"fgd", "clips", "latents", "frames"}


def test_evaluate_folder_errors_name_the_clip(ev, gold, folder, enc, sm, inp):
    seed, names = int(gold["seed"]), sf.clip_names()
    sem = dict(zip(names, sf.sem_scores(seed, 15)))
    run = lambda s, **kw: ev.evaluate_folder(str(folder / "eval"), enc, eval_n=sf.EVAL_N, smplx=sm, sem_scores=s, **kw)
    missing = {k: v for k, v in sem.items() if k != names[3]}
    with pytest.raises(ValueError, match="no sem scores for clip " + names[3]):
        run(missing)
    short = dict(sem)
    short[names[1]] = sem[names[1]][:15]                                # 30 frames at 30 fps, the clip has 32
    with pytest.raises(ValueError, match=names[1] + ".*cover 30 frames at 30 fps, the clip has 32"):
        run(short)
    with pytest.raises(ValueError, match=names[0] + ".*cover 16 frames"):
        run(sem, motion_fps=30)                                          # the 15 fps vectors read at 30 fps are too short
    with pytest.raises(ValueError, match="sem_scores need smplx"):
        ev.evaluate_folder(str(folder / "eval"), enc, eval_n=sf.EVAL_N, sem_scores=sem)
    n = sf.EVAL_N
    clips = [inp["pred"][i][:n] for i in range(2)], [inp["gt"][i][:n] for i in range(2)]
    vecs = sf.sem_scores(seed, 15)
    jm = ev.JointMetrics(sm, eval_n=n)
    with pytest.raises(ValueError, match="clipB: no sem scores"):
        jm.add(*clips, sem_scores=[vecs[0], None], names=["clipA", "clipB"])
    assert jm.clips == 0
    jm.add(*clips, names=["clipA", "clipB"])
    with pytest.raises(ValueError, match="clipC: sem scores were given for 0 of the 2 clips"):
        jm.add(*clips, sem_scores=vecs[:2], names=["clipC", "clipD"])
    jm.reset()
    jm.add(*clips, sem_scores=vecs[:2], names=["clipA", "clipB"])
    with pytest.raises(ValueError, match="clipC: sem scores were given for 2 of the 2 clips"):
        jm.add(*clips, names=["clipC", "clipD"])
    assert "srgr" in jm.compute()
