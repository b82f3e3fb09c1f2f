"""GPU: FGD evaluation on the device -- the skeleton-conv encoder (rg_fgd_encoder_layer) against the reference's per-clip latents
(tests/golden/fgd_eval.npz, made by make_fgd_golden.py), the masks really applied, batch-invariant bits, the fp64 moments, and
the end-to-end FGD of a saved folder against the reference's evaluate.py path."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fgd_eval.npz")


def _load_fixture_module():
    """tests/golden/fgd_fixture.py (the seeded inputs of fgd_eval.npz), loaded by path."""
    spec = importlib.util.spec_from_file_location("fgd_fixture", os.path.join(os.path.dirname(GOLD), "fgd_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fx = _load_fixture_module()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def sd(gold):
    full = fx.state_dict(gold)
    params = fx.encoder_params(full)
    assert fx.checksum([params[k] for k in sorted(params)]) == pytest.approx(float(gold["param_checksum"]), rel=1e-12)   # same stream
    return {k: torch.from_numpy(v) for k, v in full.items()}


@pytest.fixture(scope="module")
def sets(gold):
    s = fx.clip_sets()
    for name in ("pred", "gt"):
        assert fx.checksum(s[name]) == pytest.approx(float(gold["%s_clip_checksum" % name]), rel=1e-12)
    return s


@pytest.fixture(scope="module")
def enc(rg, sd):
    return rg.evaluation.FGDEncoder(sd)


def _clips(sets, name):
    out = []
    for aa in sets[name]:
        aa = aa[:300]
        out.append(aa[:aa.shape[0] - aa.shape[0] % 32])
    return out


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_latents_match_reference(enc, gold, sets, parity):
    worst_gpu = worst_ref = 0.0
    for name in ("pred", "gt"):
        for i, aa in enumerate(_clips(sets, name)):
            got = enc.latents(torch.from_numpy(aa).cuda()[None]).cpu().numpy().astype(np.float64)
            l64 = gold["%s_lat64_%d" % (name, i)]
            assert got.shape == l64.shape == (aa.shape[0] // 16, 240)
            worst_gpu = max(worst_gpu, _rel(got, l64))
            worst_ref = max(worst_ref, float(gold["%s_ref32_rel" % name][i]))
    parity.check("fgd encoder latents vs fp64 reference (worst clip, rel)", worst_gpu, 2e-5)
    parity.check("fgd reference fp32 latents vs fp64 (worst clip, rel; for scale)", worst_ref, 2e-5)


def test_masked_out_weights_are_ignored(rg, sd, enc, sets):
    junk = {}
    g = torch.Generator().manual_seed(5)
    for k, v in sd.items():
        v = v.clone()
        if k.endswith("residual.0.weight") or k.endswith("shortcut.weight"):
            m = sd[k.replace("weight", "mask")]
            v = torch.where(m > 0, v, 1e3 * torch.randn(v.shape, generator=g))
        junk[k] = v
    enc2 = rg.evaluation.FGDEncoder(junk)
    clips = _clips(sets, "pred")
    assert torch.equal(enc.latents(clips), enc2.latents(clips))


def test_ragged_batch_is_bit_identical(enc, sets):
    clips = _clips(sets, "pred") + _clips(sets, "gt")
    together = enc.latents(clips)
    alone = torch.cat([enc.latents([c]) for c in clips], 0)
    assert torch.equal(together, alone)
    rev = enc.latents(clips[::-1])
    k = 0
    parts = []
    for c in clips[::-1]:
        parts.append(rev[k:k + c.shape[0] // 16])
        k += c.shape[0] // 16
    assert torch.equal(torch.cat(parts[::-1], 0), together)


def test_device_moments_match_numpy(rg, parity):
    rng = np.random.default_rng(3)
    for n, d in ((4001, 240), (37, 240), (5, 7)):
        x = (rng.standard_normal((n, d)) * 0.3 + 0.7).astype(np.float32)
        mu, cov = rg.evaluation.latent_statistics(torch.from_numpy(x).cuda())
        x64 = x.astype(np.float64)
        parity.check("fgd device mean vs numpy fp64 (n=%d, d=%d, max abs)" % (n, d), np.abs(mu - x64.mean(0)).max(), 1e-12)
        parity.check("fgd device cov vs np.cov fp64 (n=%d, d=%d, rel)" % (n, d), _rel(cov, np.cov(x64, rowvar=False)), 1e-12)
        assert np.array_equal(cov, cov.T)


def test_evaluator_and_folder_match_reference_fgd(rg, enc, gold, sets, parity, tmp_path):
    ev = rg.evaluation
    want = float(gold["fgd_e2e"])
    full_p, full_g = sets["pred"], sets["gt"]
    e = ev.FGDEvaluator(enc)
    for p, g in zip(full_p[:4], full_g[:4]):           # one clip per add, then the rest in one go (device tensors)
        e.add(torch.from_numpy(p).cuda()[None], torch.from_numpy(g).cuda()[None])
    e.add([torch.from_numpy(p).cuda() for p in full_p[4:]], [torch.from_numpy(g).cuda() for g in full_g[4:]])
    parity.check("fgd FGDEvaluator vs reference evaluate.py FGD (rel)", abs(e.compute() / want - 1), 1e-4)
    assert e.clips == len(full_p)
    for i, (p, g) in enumerate(zip(full_p, full_g)):
        z = lambda a, w: np.zeros((a.shape[0], w), np.float32)
        rg.packing.save_sample_files(str(tmp_path), ["spk_%d_s/clip%02d" % (i % 3, i)], (p[None], z(p, 100)[None], z(p, 3)[None]),
                                     gt=(g[None], z(g, 100)[None], z(g, 3)[None]))
    res = ev.evaluate_folder(str(tmp_path), enc, batch_clips=3)
    parity.check("fgd evaluate_folder vs reference evaluate.py FGD (rel)", abs(res["fgd"] / want - 1), 1e-4)
    assert res["clips"] == len(full_p) and res["latents"] == 68 and res["frames"] == 68 * 16
    e.reset()
    with pytest.raises(ValueError):
        e.compute()
    sub = ev.evaluate_folder(str(tmp_path), enc, speaker_specific="1")
    assert sub["clips"] == len([i for i in range(len(full_p)) if i % 3 == 1])
