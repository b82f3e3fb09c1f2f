"""GPU: the exemplar posterior cache (vae.ExemplarPosteriorCache), the posterior-only store of rg_venc_forward, rg_vae_reparam_cached
and `skip_clip_encode` change WHEN the VAE encoders run, never what comes out: every comparison here is torch.equal against the
path that encodes everything on every call (cache_exemplar_latents=False, skip_clip_encode=False).

Shapes: the smallest VAE the fused encoder accepts (one block per side), a database of 8 entries, a 2-layer denoiser, 2 clips.
Exemplar counts 1, 3 and 5 reach the odd tail workgroup (two chunk sequences per workgroup, 10 per exemplar: never odd alone, so
the odd tail is exercised by the kernel-level test with 1 and 3 sequences), the padding to a multiple of 4 exemplars and the row
map; partial hits change which sequence shares a workgroup with which."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GI = [0] * 25 + list(range(25))
ENTRY_BYTES = 2 * 40 * 512 * 4          # (mu, logvar) x 4 parts x 10 chunks x 512 fp32


def same(a, b, path="results"):
    """torch.equal over nested dicts / lists / tuples of tensors; everything else by ==."""
    if torch.is_tensor(a) or torch.is_tensor(b):
        assert torch.is_tensor(a) and torch.is_tensor(b) and a.shape == b.shape and torch.equal(a.cpu(), b.cpu()), path
    elif isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), path
        for k in a:
            same(a[k], b[k], "%s[%r]" % (path, k))
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, "%s[%d]" % (path, i))
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), path
    elif a.__class__.__module__.startswith("torch"):     # events, streams of an asynchronous result: not data
        pass
    else:
        assert a == b, path


class Setup:
    def __init__(self, rg):
        self.rg = rg
        self.cfg = rg.synth.default_model_cfg(num_layers=2)
        self.vae_cfgs = rg.synth.synth_vae_cfgs(decoder_arch="all_encoder", num_layers=2)
        assert rg.vencfwd.num_blocks(self.vae_cfgs["upper"]["num_layers"]) == 1
        self.ds = rg.synth.SyntheticDataset(8, seed=31)
        self.P = rg.synth.synth_full_state(0, self.cfg, self.vae_cfgs)
        self.qs = [rg.synth.synth_query(41), rg.synth.synth_query(42)]
        self.plain = self.build(cache_exemplar_latents=False, skip_clip_encode=False)
        self.cached = self.build()
        assert self.plain.exemplar_cache is None and self.cached.exemplar_cache is not None

    def build(self, state=None, **kw):
        rg = self.rg
        m = rg.build_architecture(rg.synth.reference_style_model_cfg(self.cfg, self.vae_cfgs, with_retrieval=True),
                                  database=self.ds, **kw)
        m.load_state_dict(self.P if state is None else state)
        m.eval()
        return m

    def data(self):
        d = self.rg.synth.synth_batch(2, seed=8)
        d["discourse"], d["prominence"] = [q["discourse"] for q in self.qs], [q["prominence"] for q in self.qs]
        d["text_features"] = [q["text_features"] for q in self.qs]
        d["speaker_ids"] = torch.tensor([[q["speaker_id"]] * 150 for q in self.qs])
        d["sample_name"] = ["query_a", "query_b"]
        return d

    def forward(self, model, seed, ikw=None):
        """-> (results, tape position after the call)"""
        tape = self.rg.synth.NoiseTape(seed)
        out = model(**dict(self.data(), retrieval_method="discourse", inference_kwargs=dict(ikw or {}, noise_tape=tape)))
        torch.cuda.synchronize()
        return out, tape.count

    def exemplars(self, model, names, seed):
        """RetrievalDatabase.encode_exemplars for the given exemplar names -> (latent, tape position)."""
        tape = self.rg.synth.NoiseTape(seed)
        db = model.model.database
        lat, _ = db.encode_exemplars(model.model.gesture_rep_encoder, list(names), [self.ds[n] for n in names], tape, model.device)
        torch.cuda.synchronize()
        return lat, tape.count


@pytest.fixture(scope="module")
def su(rg):
    return Setup(rg)


GUIDED = dict(use_inversion=True, insertion_guidance=True, guidance_iters=GI, guidance_lr=0.1)


def test_cached_forward_equals_uncached(su):
    """One guided forward without the cache against one with it (cold: every exemplar is encoded into its slot), then a second
    cached forward (all hits): every tensor of the results, retrieval_dict and its retr_uncropped_latents included, and the
    tape position."""
    ref, n_ref = su.forward(su.plain, 77, GUIDED)
    n_ex = sum(len(x) for x in ref["retrieval_dict"]["retr_uncropped_latents"])
    assert n_ex >= 1, "the synthetic queries should retrieve exemplars"
    cache = su.cached.exemplar_cache
    cache.clear()
    h0, m0 = cache.hits, cache.misses
    cold, n_cold = su.forward(su.cached, 77, GUIDED)
    assert cache.misses > m0
    m1 = cache.misses
    warm, n_warm = su.forward(su.cached, 77, GUIDED)
    assert cache.misses == m1 and cache.hits > h0
    assert n_ref == n_cold == n_warm
    same(ref, cold)
    same(ref, warm)


@pytest.mark.parametrize("count", [1, 3, 5])
def test_exemplar_counts(su, count):
    """1, 3 and 5 exemplars (padding to 4 / 8 on both paths; the 5th is a repeat of the 2nd: one slot, two latents with their
    own noise): uncached, cached cold, cached warm."""
    names = su.ds.names[:4] + [su.ds.names[1]]
    names = names[:count]
    ref, n_ref = su.exemplars(su.plain, names, 5)
    cache = su.cached.exemplar_cache
    cache.clear()
    m0 = cache.misses
    cold, n_cold = su.exemplars(su.cached, names, 5)
    assert cache.misses - m0 == len(set(names))
    warm, n_warm = su.exemplars(su.cached, names, 5)
    assert cache.misses - m0 == len(set(names))
    assert n_ref == n_cold == n_warm == 4 * count
    assert ref.shape == cold.shape == (count, 43, 512)
    assert torch.equal(ref, cold) and torch.equal(ref, warm)


def test_partial_hits(su):
    """Two of five names warmed: the three others are encoded alone (other workgroup partners, other padding) into the slots
    the row map names."""
    names = su.ds.names[:5]
    ref, _ = su.exemplars(su.plain, names, 6)
    cache = su.cached.exemplar_cache
    cache.clear()
    assert su.cached.warm_exemplar_cache([names[1], names[3]]) == 2
    h0, m0 = cache.hits, cache.misses
    got, _ = su.exemplars(su.cached, names, 6)
    assert (cache.hits - h0, cache.misses - m0) == (2, 3)
    assert torch.equal(ref, got)
    assert su.cached.warm_exemplar_cache() == len(su.ds.names) - 5 and len(cache.slots) == len(su.ds.names)
    got, _ = su.exemplars(su.cached, names, 6)
    assert torch.equal(ref, got)


def test_eviction(su):
    """A cache of two entries, three distinct exemplars over two calls (and a batch that does not fit at all)."""
    m = su.build(exemplar_cache_bytes=2 * ENTRY_BYTES)
    cache = m.exemplar_cache
    a, b, c = su.ds.names[:3]
    for seed, names in ((1, [a, b]), (2, [c, a]), (3, [b]), (4, [a, b, c])):
        ref, n_ref = su.exemplars(su.plain, names, seed)
        got, n_got = su.exemplars(m, names, seed)
        assert torch.equal(ref, got) and n_ref == n_got, names
        assert cache.capacity == 2 and len(cache.slots) <= 2
    assert cache.evictions == 2 and cache.misses == 4


def test_invalidation_by_load_state_dict(su):
    """Posteriors depend on the VAE weights: after load_state_dict of another state a forward equals that of a model built
    fresh with that state."""
    P2 = su.rg.synth.synth_full_state(1, su.cfg, su.vae_cfgs)
    m = su.build()
    su.forward(m, 77, GUIDED)
    old = m.exemplar_cache
    assert old.misses > 0
    m.load_state_dict(P2)
    assert m.exemplar_cache is not old and not m.exemplar_cache.slots
    got, n_got = su.forward(m, 78, GUIDED)
    ref, n_ref = su.forward(su.build(state=P2), 78, GUIDED)
    assert n_got == n_ref
    same(ref, got)
    stale, _ = su.forward(su.cached, 78, GUIDED)
    assert not torch.equal(stale["prev_latentout"], ref["prev_latentout"])


@pytest.mark.parametrize("nseq", [1, 3])
def test_posterior_only_store(su, nseq):
    """rg_venc_forward_grouped, four parts, S = 17: the posterior-only form stores rows 0 / 1 of every mapped sequence -- the
    bits of the full-row form -- and nothing for a map entry of -1."""
    gre = su.cached.model.gesture_rep_encoder
    dev, S = gre.dev, 17
    g = torch.Generator(device="cpu").manual_seed(3)
    xs = [torch.randn(nseq * S, 512, generator=g).to(dev) for _ in range(4)]
    rows = torch.full((4, nseq), -1, dtype=torch.int32)
    for p in range(4):
        for i in range(nseq):
            if not (nseq == 3 and i == 1):          # the middle sequence of three is "padding"
                rows[p, i] = 2 + 3 * p + (nseq - 1 - i)       # scattered, part by part
    rows = rows.to(dev)
    fill = 7.0
    mu, lv = (torch.full((16, 512), fill, device=dev) for _ in range(2))
    full = [None] * 4
    vaes = [gre.vaes[p] for p in su.rg.vae.PARTS]

    def run_full(p):
        full[p] = vaes[p].venc.run(xs[p], nseq, S)
    gre._fan_out([lambda p=p: run_full(p) for p in range(4)], one_chain=True)
    gre._fan_out([lambda p=p: vaes[p].venc.run(xs[p], nseq, S, post=(rows[p], mu, lv)) for p in range(4)], one_chain=True)
    torch.cuda.synchronize()
    written = set()
    for p in range(4):
        out = full[p].view(nseq, S, 512)
        for i in range(nseq):
            r = int(rows[p, i])
            if r >= 0:
                written.add(r)
                assert torch.equal(mu[r], out[i, 0]) and torch.equal(lv[r], out[i, 1]), (p, i)
    assert len(written) == 4 * (nseq - (nseq == 3))
    rest = [r for r in range(16) if r not in written]
    assert bool((mu[rest] == fill).all()) and bool((lv[rest] == fill).all())


@pytest.mark.parametrize("mode", ["base", "guided", "prev_latent"])
def test_skip_clip_encode(su, mode):
    """Base (no inversion: the retrieved exemplars are encoded and not used), guided and use_prev_latent forwards with and
    without the batch's own VAE encode: every result key, `trans` after the call and the tape position."""
    m = su.plain
    ikw = {} if mode == "base" else dict(GUIDED)
    if mode == "prev_latent":
        g = torch.Generator(device="cpu").manual_seed(9)
        ikw.update(use_prev_latent=True, prev_latent=torch.randn(2, 43, 512, generator=g))
    assert m.skip_clip_encode is False
    ref, n_ref = su.forward(m, 12, ikw)
    m.skip_clip_encode = True
    try:
        got, n_got = su.forward(m, 12, ikw)
    finally:
        m.skip_clip_encode = False
    assert n_ref == n_got
    assert torch.equal(ref["trans"].cpu(), got["trans"].cpu()) and not torch.equal(got["trans"].cpu(), su.data()["trans"])
    same(ref, got)
