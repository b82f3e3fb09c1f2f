"""CPU: the host ranking of the batched exemplar search (csrc/rg_retrieval_host.h: rg_rank_cut_tiers + rg_rank_walk, what
rg_rank_survivors_batch / rg_discourse_search_batch run between their two read-backs) against the oracle's statement of the
reference's walk (oracle.retrieval.ranking_walk), in the manner of test_seq2_many_host_cpu.py: a stand-alone program includes
the header and ranks cases this test generates; there is no device here, so the tie-break similarities are fed directly (one
value per entry).  Compared exactly."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import retrieval as oret

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rag-gesture_amd", "csrc")

# input: per case a line "n", then n lines "entry top score sim" (hex floats), survivors in ANY order (the device appends them
# through an atomic cursor); output: per case "k e:t e:t ..."
PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>
#include "rg_retrieval_host.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n;
  while (std::fscanf(f, "%d", &n) == 1) {
    std::vector<int> idx(n), top(n);
    std::vector<double> score(n);
    std::map<int, double> sim;
    for (int i = 0; i < n; ++i) {
      char a[64], b[64];
      if (std::fscanf(f, "%d %d %63s %63s", &idx[i], &top[i], a, b) != 4) return 3;
      score[i] = std::strtod(a, nullptr);
      sim[idx[i]] = std::strtod(b, nullptr);
    }
    rg_rank_cut cut;
    rg_rank_cut_tiers(idx.data(), top.data(), score.data(), n, cut);
    std::vector<double> sims;                       // what the one similarity launch returns: the multi-member tiers' members
    for (const auto& t : cut.tiers)
      if (t.second > 1)
        for (int k = 0; k < t.second; ++k) sims.push_back(sim[cut.entry[t.first + k]]);
    if ((int)sims.size() != cut.multi_members()) return 4;
    int e[RG_RANK_MAX], tp[RG_RANK_MAX];
    const int k = rg_rank_walk(cut, sims.data(), e, tp);
    std::printf("%d", k);
    for (int i = 0; i < k; ++i) std::printf(" %d:%d", e[i], tp[i]);
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}
"""


def _case(scores, sims, rng):
    """entries (distinct, ascending), tops, scores, sims of one query relation's survivors."""
    n = len(scores)
    entry = np.sort(rng.choice(5000, size=n, replace=False)).astype(np.int64)
    top = rng.integers(0, 5, size=n)
    return entry, top, np.asarray(scores, dtype=np.float64), np.asarray(sims, dtype=np.float64)


def _cases():
    rng = np.random.default_rng(20251)
    u = lambda n: rng.uniform(-1, 1, size=n)
    named = {
        "tier straddles the 10th place": _case([9.0] * 3 + [7.0] * 12 + [2.0] * 4, u(19), rng),
        "tier ends on the 10th place": _case([9.0] * 4 + [7.0] * 6 + [2.0] * 5, u(15), rng),
        "single-member tiers": _case([13.0 - 0.5 * i for i in range(14)], u(14), rng),
        "single then tie": _case([12.5] + [9.0] * 11, u(12), rng),
        "fewer than 10 positive": _case([9.0, 9.0, 5.0, 2.0] + [0.0] * 8, u(12), rng),
        "no positive survivor": _case([0.0] * 6, u(6), rng),
        "no survivor": _case([], [], rng),
        "one survivor": _case([2.0], [0.3], rng),
        "equal similarities in a tier": _case([9.0] * 14, [0.25] * 5 + [0.5] * 4 + [0.25] * 5, rng),
        "all similarities equal": _case([9.0] * 2 + [6.0] * 20, [0.125] * 22, rng),
        "tier larger than 256": _case([9.0] * 2 + [7.0] * 300, u(302), rng),
        "tier larger than 256, coarse similarities": _case([7.0] * 700, rng.integers(0, 4, size=700) / 4.0, rng),
        "a similarity that is not a number": _case([9.0] * 13, [float("nan") if i in (2, 7) else v for i, v in enumerate(u(13))], rng),
        "scores one ulp apart": _case([9.0, np.nextafter(9.0, 10.0), 9.0, np.nextafter(9.0, 0.0)] * 4, u(16), rng),
    }
    out = list(named.items())
    for i in range(400):      # seeded random cases: scores from 4-6 distinct values, similarities often repeated
        levels = rng.choice([0.0, 2.0, 5.0, 6.0, 9.0, 9.0 + 4.0 / 3.0, 11.5, 13.0], size=int(rng.integers(4, 7)), replace=False)
        n = int(rng.integers(0, 41))
        sims = rng.integers(0, 6, size=n) / 8.0 if i % 3 == 0 else u(n)
        out.append(("random %d" % i, _case(rng.choice(levels, size=n), sims, rng)))
    return out, rng


def _oracle_ranking(entry, top, score, sim):
    """oracle.retrieval.ranking_walk over the survivors in ascending entry order (the DB's order); a tier is reordered as
    sort_sidx_by_textsimilarity reorders it: sorted by descending similarity, stable."""
    keys = entry.tolist()
    sim_of, top_of = dict(zip(keys, sim.tolist())), dict(zip(keys, top.tolist()))
    ranked = oret.ranking_walk(dict(zip(keys, score.tolist())), lambda tier: sorted(tier, key=sim_of.get, reverse=True))
    return [(e, top_of[e]) for e in ranked]


def _nan_ranking(entry, top, score, sim):
    """Python's sorted has no defined answer for a similarity that is not a number; the header documents one: NaN behind every
    number, stable.  Written out for the one tier of that case."""
    assert len(set(score.tolist())) == 1 and score[0] > 0 and np.isnan(sim).any()
    numbers = [i for i in range(len(entry)) if not np.isnan(sim[i])]
    order = sorted(numbers, key=lambda i: sim[i], reverse=True) + [i for i in range(len(entry)) if np.isnan(sim[i])]
    return [(int(entry[i]), int(top[i])) for i in order[:10]]


def _tiers(entry, score):
    """The score tiers the walk can reach (it stops once it holds 10), grouped by equal score here."""
    tiers, held = [], 0
    for sc in sorted({v for v in score.tolist() if v > 0}, reverse=True):
        if held >= 10:
            break
        tiers.append([int(e) for e, v in zip(entry, score) if v == sc])
        held += len(tiers[-1])
    return tiers


@pytest.fixture(scope="module")
def rank_exe(tmp_path_factory):
    """The stand-alone ranking program, compiled once."""
    cxx = shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(cxx), "no C++ compiler: the host ranking cannot be checked"
    d = tmp_path_factory.mktemp("rank")
    src, exe = d / "rank.cpp", d / "rank"
    src.write_text(PROGRAM)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _run(rank_exe, path, lines):
    """One case per (entry, top, score, sim) block in `lines` -> per case [(entry, top)] as the program ranks them."""
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([rank_exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = []
    for line in r.stdout.splitlines():
        f = line.split()
        assert int(f[0]) == len(f) - 1
        out.append([tuple(int(v) for v in p.split(":")) for p in f[1:]])
    return out


def _lines(entry, top, score, sim, order):
    return ["%d" % len(entry)] + ["%d %d %s %s" % (entry[i], top[i], float(score[i]).hex(), float(sim[i]).hex()) for i in order]


def test_host_ranking_equals_the_oracle_walk(rank_exe, tmp_path):
    cases, rng = _cases()
    want, kinds, lines = [], set(), []
    for name, (entry, top, score, sim) in cases:
        ranked = (_nan_ranking if name == "a similarity that is not a number" else _oracle_ranking)(entry, top, score, sim)
        want.append(ranked)
        tiers = _tiers(entry, score)
        sizes = [len(t) for t in tiers]
        held = np.cumsum([0] + sizes)
        kinds |= {"straddle" for i, s in enumerate(sizes) if held[i] < 10 < held[i + 1]}
        kinds |= {"single" for s in sizes if s == 1} | {"big" for s in sizes if s > 256}
        kinds |= {"few"} if 0 < len(ranked) < 10 else set()
        kinds |= {"none"} if len(entry) and not len(ranked) else set()
        kinds |= {"empty"} if not len(entry) else set()
        kinds |= {"equal sims" for t in tiers if len(t) > 1 and len({sim[list(entry).index(e)] for e in t}) < len(t)}
        lines += _lines(entry, top, score, sim, rng.permutation(len(entry)))             # the device's order is arbitrary
    assert kinds == {"straddle", "single", "big", "few", "none", "empty", "equal sims"}, kinds
    assert len(cases) == 414
    got = _run(rank_exe, tmp_path / "cases.txt", lines)
    assert len(got) == len(cases)
    for (name, _), g, ranked in zip(cases, got, want):
        assert g == [(int(e), int(t)) for e, t in ranked], name


def test_host_ranking_walk_matches_oracle_without_gpu(rg, rank_exe, tmp_path):
    """The host half of the product's discourse retrieval (survivor ordering, tier cut, tie-break ordering, the 10-entry walk
    in the compiled program; names and bounds in retrieval.ranked_results) against the oracle, on CPU: the device results it
    consumes (survivors of the top-score selection, tie-break similarities in float64) are produced here from the oracle's
    own scores."""
    R = rg.retrieval
    db = oret.build_db_dicts(rg.synth.synth_retrieval_samples(200, seed=2025))
    names = list(db["idx_2_sense"].keys())

    def sim(q, e):   # rag/utils.py:109-121 in float64, like rg_text_diag_sim_many
        f = db["idx_2_text"][names[e]][0].double()
        n = min(q.shape[0], f.shape[0])
        return float((q[:n].double() * f[:n]).sum() / n) if n else 0.0

    wants, lines = [], []
    for seed in (11, 12, 13, 14, 21, 22, 100, 101, 102):
        q = rg.synth.synth_query(seed)
        trace = []
        wants.append((q, oret.discourse_retrieval(q["discourse"], q["prominence"], q["speaker_id"], db, q["text_features"], trace)))
        assert len(trace) == len(q["discourse"])
        for t in trace:
            sc = np.array([float(t["score"][n]) for n in names])
            pos = np.sort(sc[sc > 0])[::-1]
            thr = pos[9] if len(pos) >= 10 else 0.0
            keep = np.nonzero((sc >= thr) & (sc > 0))[0]
            lines += _lines(keep, [t["top"].get(names[e], -1) for e in keep], sc[keep], [sim(q["text_features"], e) for e in keep],
                            range(len(keep)))
    got = _run(rank_exe, tmp_path / "survivors.txt", lines)
    pos = 0
    for q, want in wants:
        ranked = [([e for e, _ in g], [t for _, t in g]) for g in got[pos:pos + len(q["discourse"])]]
        pos += len(q["discourse"])
        si, d_bounds = R.ranked_results(names, ranked, R.discourse_bounds(db, names))
        assert si == want[0] and d_bounds == want[1] and R.discourse_query_bounds(q["discourse"]) == want[2]
    assert pos == len(got)
