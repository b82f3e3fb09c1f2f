"""CPU: the N > 1 path (clip sharding + final result gather) with 2 gloo processes."""
import importlib
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = dict(pred_upper=39, pred_lower=27, pred_facepose=3, pred_hands=90, pred_transl=3, pred_exps=100)


def _fake_results(lo, hi):
    """Deterministic per-clip 'results': clip c, key k -> c + 0.01 * column index."""
    out = {}
    for k, w in WIDTHS.items():
        c = torch.arange(lo, hi, dtype=torch.float32).view(-1, 1, 1)
        out[k] = (c + 0.01 * torch.arange(w, dtype=torch.float32).view(1, 1, -1)).expand(-1, 150, -1).contiguous()
    return out


def _worker(rank, world, port, n_total, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    d = importlib.import_module("rag-gesture_amd.dist")
    data = dict(motion_upper=torch.zeros(n_total, 150, 39), sample_name=["c%d" % i for i in range(n_total)], flag=7)
    shard = d.shard_batch(data, rank, world)
    lo, hi = d.shard_range(n_total, rank, world)
    assert shard["motion_upper"].shape[0] == hi - lo and shard["sample_name"] == ["c%d" % i for i in range(lo, hi)]
    assert shard["flag"] == 7
    full = d.gather_results(_fake_results(lo, hi), n_total=n_total)
    want = _fake_results(0, n_total)
    ok = all(torch.equal(full[k], want[k]) for k in WIDTHS)
    full2 = d.gather_results(_fake_results(lo, hi))  # sizes exchanged instead of given
    ok = ok and all(torch.equal(full2[k], want[k]) for k in WIDTHS)
    q.put((rank, ok))
    dist.destroy_process_group()


def _run(n_total, port):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_total, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(0, True), (1, True)]


def test_shard_and_gather_even():
    _run(8, 29611)


def test_shard_and_gather_ragged():
    _run(5, 29612)


def test_shard_range_covers_everything():
    d = importlib.import_module("rag-gesture_amd.dist")
    for n in (1, 7, 10, 128):
        for w in (1, 2, 4, 8):
            spans = [d.shard_range(n, r, w) for r in range(w)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            assert max(h - l for l, h in spans) - min(h - l for l, h in spans) <= 1


def test_bench_launcher_starts_one_process_per_gpu():
    """`python bench.py --gpus N` (no torchrun environment) must start N rank processes with the
    torch.distributed.run environment; --dry-launch makes every rank report what it saw (no GPU)."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--dry-launch"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    ranks = json.loads(r.stdout.strip().splitlines()[-1])
    assert [x["rank"] for x in ranks] == [0, 1, 2] and [x["local_rank"] for x in ranks] == [0, 1, 2]
    assert all(x["world"] == 3 and x["master_addr"] == "127.0.0.1" for x in ranks)
    assert len({x["master_port"] for x in ranks}) == 1 and len({x["pid"] for x in ranks}) == 3
    # the 8-GPU node of BASELINE config 4: eight ranks, each on its own device, each with the hardware-queue setting in its
    # environment BEFORE torch is imported (the HIP runtime reads it once, at its first call), dmabuf IPC for RCCL
    env8 = {k: v for k, v in env.items() if k != "GPU_MAX_HW_QUEUES"}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--dry-launch"], env=env8,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    ranks = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(x["local_rank"] for x in ranks) == list(range(8)) and len({x["pid"] for x in ranks}) == 8
    assert all(x["hw_queues"] == "2" and x["torch_imported"] is False and x["ipc_legacy"] == "0" for x in ranks), ranks
    # a value the user has set wins
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-launch"],
                       env=dict(env8, GPU_MAX_HW_QUEUES="1"), capture_output=True, text=True, timeout=120)
    assert [x["hw_queues"] for x in json.loads(r.stdout.strip().splitlines()[-1])] == ["1", "1"]
    # under an external launcher the flag and the environment must agree
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--dry-launch"],
                       env=dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


# ---- long-form clip sharding (BASELINE config 5: 10 clips over 8 GPUs; tools/longform_synthesis.py:211, 256)
class _StubModel:
    """Stands for MotionDiffusion on CPU: outputs are deterministic functions of the window and of the clip's own
    prev-latent chain, so a wrong chain / a clip on the wrong rank / a mixed-up batch order changes the result."""

    class model:
        cfg = dict(frame_chunk_size=15)

    def __call__(self, **kw):
        m = kw["motion"].float()
        B = m.shape[0]
        prev = kw["inference_kwargs"]["prev_latent"]
        prev = torch.zeros(B, 43, 512) if prev is None else prev
        lat = prev * 0.5 + m.mean(dim=(1, 2)).view(B, 1, 1) + kw["audio"].float().mean(dim=(1, 2)).view(B, 1, 1)
        s = lat.mean(dim=(1, 2)).view(B, 1, 1)
        out = dict(kw, prev_latentout=lat, pred_upper=m[:, :, :39] + s, pred_lower=m[:, :, 39:66] + s,
                   pred_facepose=m[:, :, 66:69] + s, pred_hands=m[:, :, 69:159] + s, pred_transl=kw["trans"].float() + s,
                   pred_exps=kw["facial"].float() + s)
        return out


def _longform_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    rg = importlib.import_module("rag-gesture_amd")
    lf = rg.longform
    # CPU stand-ins for the HIP post-processing (blend / scatter / interpolation are covered on the GPU)
    lf.blend_window = lambda prev, cur, ov: tuple(torch.cat([p[:, :-ov], c], 1) for p, c in zip(prev, cur))
    lf.packing.scatter_parts = lambda up, lo, ha, fa: torch.cat([up, lo, fa, ha, torch.zeros_like(up[:, :, :6])], -1)
    lf.packing.upsample_motion = lambda t, s: t.repeat_interleave(s, dim=1)
    lf.packing.upsample_features = lambda t, s: t.repeat_interleave(s, dim=1)
    lens = [300, 150, 430, 200, 150]
    clips = []
    for ci, n in enumerate(lens):
        g = torch.Generator().manual_seed(ci)
        clips.append(dict(motion=torch.randn(1, n, 165, generator=g), trans=torch.randn(1, n, 3, generator=g),
                          facial=torch.randn(1, n, 100, generator=g), motion_mask=torch.ones(1, n),
                          speaker_ids=torch.zeros(1, n, dtype=torch.int64)))
    feats = lambda ci, cidx, t0, t1, ann: dict(audio=torch.full((1, 499, 768), float(ci + 0.1 * cidx)), text_features=None)
    synth = lf.LongformSynthesizer(_StubModel(), overlap=15)
    res = synth.run_many(clips, feats, gather=True)
    mine = synth.run_many(clips, feats, gather=False)
    q.put((rank, {ci: float(r["poses"].sum()) for ci, r in res.items()}, sorted(mine)))
    if world > 1:
        dist.destroy_process_group()


def test_longform_run_many_shards_clips_over_ranks():
    ctx = mp.get_context("spawn")
    out = {}
    for world, port in ((1, 29621), (2, 29622)):
        q = ctx.Queue()
        procs = [ctx.Process(target=_longform_worker, args=(r, world, port, q)) for r in range(world)]
        for p in procs:
            p.start()
        out[world] = sorted(q.get(timeout=180) for _ in procs)
        for p in procs:
            p.join(timeout=60)
    (_, single, all_clips), = out[1]
    assert all_clips == [0, 1, 2, 3, 4]
    (r0, g0, m0), (r1, g1, m1) = out[2]
    assert m0 == [0, 1, 2] and m1 == [3, 4], "contiguous balanced shards (dist.shard_range)"
    assert g0 == g1 == single, "every rank ends with every clip's result, equal to the single-process run"


# ---- the loop the driver launches with `--gpus N`: bench.run_steps (pipeline with late results + ONE all-gather at the end)
class _StubWorkload:
    """Hands results out two calls late, like the co-batched pipeline with whole batches alternating between two lanes."""

    def __init__(self, rank, B=4):
        self.rank, self.B, self.n, self.pending = rank, B, 0, []

    def _result(self, k):
        return torch.full((self.B, 150, 268), float(100 * self.rank + k))

    def step(self):
        self.pending.append(self._result(self.n))
        self.n += 1
        return self.pending.pop(0) if len(self.pending) > 2 else None

    def drain(self):
        out, self.pending = self.pending, []
        return out


def _bench_worker(rank, world, port, steps, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    bench = importlib.import_module("bench")
    wl = _StubWorkload(rank)
    synced = []
    got = bench.run_steps(wl, steps, dist, world, lambda: synced.append(True))
    ok = tuple(got.shape) == (world * steps * wl.B, 150, 268) and synced == [True] and wl.pending == []
    for r in range(world):          # rank r's batches, in submission order, in rank r's block of the gathered tensor
        for k in range(steps):
            blk = got[(r * steps + k) * wl.B:(r * steps + k + 1) * wl.B]
            ok = ok and bool((blk == float(100 * r + k)).all())
    # a second call on the same workload object (bench.py runs warm-up steps, then the timed steps)
    got2 = bench.run_steps(wl, 1, dist, world, None)
    ok = ok and tuple(got2.shape) == (world * wl.B, 150, 268) and bool((got2[:wl.B] == float(steps)).all())
    q.put((rank, ok))
    dist.destroy_process_group()


def test_bench_run_steps_gathers_once_at_the_end_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_bench_worker, args=(r, 2, 29613, 5, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(0, True), (1, True)]


def test_bench_run_steps_single_process_returns_the_list():
    bench = importlib.import_module("bench")
    wl = _StubWorkload(0)
    out = bench.run_steps(wl, 4)
    assert len(out) == 4 and all(float(o[0, 0, 0]) == k for k, o in enumerate(out))
