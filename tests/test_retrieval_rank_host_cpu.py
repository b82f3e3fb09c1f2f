"""CPU: the host ranking of the batched exemplar search (csrc/rg_retrieval_host.h: rg_rank_cut_tiers + rg_rank_walk, what
rg_discourse_search_batch runs between its two read-backs) against the Python path it restates -- DiscourseIndex.collect's
entry order, _cut_tiers and _walk_tiers -- in the manner of test_seq2_many_host_cpu.py: a stand-alone program includes the
header and ranks cases this test generates; there is no device here, so the tie-break similarities are fed directly (one value
per entry).  Compared exactly."""
import importlib
import os
import shutil
import subprocess

import numpy as np

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


def _python_ranking(R, entry, top, score, sim):
    """The existing path: collect() hands survivors over in ascending entry order; _cut_tiers; _walk_tiers."""
    sim_of = dict(zip(entry.tolist(), sim.tolist()))

    class Index:
        @staticmethod
        def sims_async(q_dev, cand):
            return np.array([sim_of[e] for e in cand], dtype=np.float64)
    sims = []
    tiers, top_of = R._cut_tiers(Index, None, (entry, score, top), sims)
    return [(e, top_of[e]) for e in R._walk_tiers(tiers, sims)], tiers


def test_host_ranking_equals_the_python_path(tmp_path):
    R = importlib.import_module("rag-gesture_amd.retrieval")
    cxx = shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(cxx), "no C++ compiler: the host ranking cannot be checked"
    src, exe, inp = tmp_path / "rank.cpp", tmp_path / "rank", tmp_path / "cases.txt"
    src.write_text(PROGRAM)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases, rng = _cases()
    want, kinds, lines = [], set(), []
    for name, (entry, top, score, sim) in cases:
        ranked, tiers = _python_ranking(R, entry, top, score, sim)
        want.append(ranked)
        sizes = [len(t) for t, _ in tiers]
        held = np.cumsum([0] + sizes)
        kinds |= {"straddle" for i, s in enumerate(sizes) if held[i] < 10 < held[i + 1]}
        kinds |= {"single" for s in sizes if s == 1} | {"big" for s in sizes if s > 256}
        kinds |= {"few"} if 0 < len(ranked) < 10 else set()
        kinds |= {"none"} if len(entry) and not len(ranked) else set()
        kinds |= {"empty"} if not len(entry) else set()
        kinds |= {"equal sims" for (t, slot) in tiers if slot is not None and len({sim[list(entry).index(e)] for e in t}) < len(t)}
        o = rng.permutation(len(entry))             # the device's order is arbitrary
        lines.append("%d" % len(entry))
        lines += ["%d %d %s %s" % (entry[i], top[i], float(score[i]).hex(), float(sim[i]).hex()) for i in o]
    assert kinds == {"straddle", "single", "big", "few", "none", "empty", "equal sims"}, kinds
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    got = r.stdout.splitlines()
    assert len(got) == len(cases)
    for (name, _), line, ranked in zip(cases, got, want):
        f = line.split()
        assert int(f[0]) == len(f) - 1
        assert [tuple(int(v) for v in p.split(":")) for p in f[1:]] == [(int(e), int(t)) for e, t in ranked], name
