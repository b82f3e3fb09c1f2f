"""The `motion` retrieval method (exemplars by a motion example), host side: the float64 restatement's own invariants, the
query validation, the placement, ranked_results, the header and its argument checks, the dispatch.  No device: the kernel and
the search are tested in test_motion_retrieval_gpu.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import motion_retrieval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rag-gesture_amd", "csrc")


# ------------------------------------------------------------------------------------------- the restatement's own invariants
def test_restatement_planted_example_scores_exactly_one():
    lat, spk, _ = ref.fixture(0, 70)
    qlat = lat[37, :, 4:7, :].copy()
    for w in ((1, 1, 0, 0), (1, 1, 1, 1), (0, 0, 0, 1), (0.3, 2.5, 0, 7)):
        score, top, S, d = ref.scores(lat, spk, qlat, w, speaker=int(spk[37]), bonus=0.0)
        assert score[37] == 1.0 and top[37] == 4 and d[37, 4] == 0.0
        assert (np.delete(score, 37) < 1.0).all() and int(np.argmax(score)) == 37
    withb = ref.scores(lat, spk, qlat, (1, 1, 0, 0), speaker=int(spk[37]), bonus=0.5)[0]
    plain = ref.scores(lat, spk, qlat, (1, 1, 0, 0), speaker=int(spk[37]), bonus=0.0)[0]
    same = spk == spk[37]
    assert withb[37] == 1.5 and np.array_equal(withb[same], plain[same] + 0.5) and np.array_equal(withb[~same], plain[~same])


def test_restatement_tie_rule_picks_the_lowest_offset():
    lat, spk, _ = ref.fixture(1, 3)
    lat[1, :, 6:8, :] = lat[1, :, 2:4, :]              # entry 1 holds the same two chunks at offsets 2 and 6
    lat[2, :, :, :] = lat[2, :, :1, :]                 # entry 2: ten equal chunks, every offset ties
    q = lat[1, :, 2:4, :].copy()
    score, top, S, d = ref.scores(lat, spk, q)
    assert d[1, 2] == d[1, 6] == 0.0 and top[1] == 2 and score[1] == 1.0
    score, top, S, d = ref.scores(lat, spk, lat[2, :, 3:6, :].copy() + np.float32(0.5))
    assert len(set(d[2].tolist())) == 1 and d[2, 0] > 0 and top[2] == 0


def test_restatement_leaves_out_few_pairs_of_the_fixture():
    """The GPU test compares `top` only where the runner-up offset is further than the fp32 error bound allows to flip; on the
    fixture (chunks scaled by [0.25, 4]) that leaves out well under 2 % of the (query, entry) pairs."""
    for seed in range(4):
        lat, spk, qlats = ref.fixture(seed, 70)
        out = total = 0
        for w in ((1, 1, 0, 0), (1, 1, 1, 1), (0, 0, 0, 1)):
            for q in qlats:
                _, top, S, d = ref.scores(lat, spk, q, w)
                total += d.shape[0]
                if d.shape[1] == 1:
                    continue
                b = ref.sum_bound(q.shape[1], q.shape[2])
                srt = np.sort(d, axis=1)
                out += int((srt[:, 1] * (1 - 2 * b) <= srt[:, 0] * (1 + 2 * b)).sum())
        assert total == 3 * 5 * 70 and out <= 0.02 * total, (seed, out, total)


# ------------------------------------------------------------------------------------------------------------ query validation
def _example(frames=45, **over):
    widths = dict(motion_upper=39, motion_lower=27, motion_face=3, motion_hands=90, trans=3, facial=100, contact=4)
    ex = {k: torch.zeros(frames, w) for k, w in widths.items()}
    ex.update(over)
    return ex


def test_query_accepted(rg):
    f = rg.retrieval.motion_query_fields
    s, e, ex, w, n_q = f((1.0, 4.0, _example(45)))
    assert (s, e, w, n_q) == (1.0, 4.0, (1.0, 1.0, 0.0, 0.0), 3) == ref.validate_query((1.0, 4.0, _example(45)))[:2] + ((1.0, 1.0, 0.0, 0.0), 3)
    assert f((2.0, 2.0, _example(150), (0, 0, 0.5, 2)))[3:] == ((0.0, 0.0, 0.5, 2.0), 10)
    assert f((0.0, 1.0, _example(15), None))[3:] == ((1.0, 1.0, 0.0, 0.0), 1)


def _refused(rg, query, match):
    with pytest.raises(ValueError, match=match) as info:
        rg.retrieval.motion_query_fields(query, where="clip 3, motion query 1")
    assert "clip 3, motion query 1" in str(info.value)
    with pytest.raises(ValueError):
        ref.validate_query(query)


def test_query_refused_frames_not_a_multiple_of_the_chunk(rg):
    _refused(rg, (0.0, 1.0, _example(44)), "multiple")


def test_query_refused_no_chunk(rg):
    _refused(rg, (0.0, 1.0, _example(0)), "chunks")


def test_query_refused_more_chunks_than_a_window(rg):
    _refused(rg, (0.0, 1.0, _example(165)), "chunks")


def test_query_refused_start_behind_end(rg):
    _refused(rg, (4.0, 3.5, _example(45)), "start_s")


def test_query_refused_negative_weight(rg):
    _refused(rg, (0.0, 1.0, _example(45), (1, -0.5, 0, 0)), "non-negative")


def test_query_refused_weight_not_finite(rg):
    _refused(rg, (0.0, 1.0, _example(45), (1, float("nan"), 0, 0)), "finite")
    _refused(rg, (0.0, 1.0, _example(45), (float("inf"), 0, 0, 0)), "finite")


def test_query_refused_all_weights_zero(rg):
    _refused(rg, (0.0, 1.0, _example(45), (0, 0, 0, 0)), "all be zero")


def test_query_refused_tensors_of_different_lengths_or_missing(rg):
    _refused(rg, (0.0, 1.0, _example(45, trans=torch.zeros(30, 3))), "different numbers")
    ex = _example(45)
    del ex["contact"]
    _refused(rg, (0.0, 1.0, ex), "lacks contact")


# ------------------------------------------------------------------------------------------------------------------ placement
def _place(rg, queries):
    """place_exemplars over one clip's queries [(start_s, end_s, o*, n_q)], one exemplar each."""
    si = {i: ["e%d" % i] for i in range(len(queries))}
    db_b = {i: {"e%d" % i: ("motion", "motion", o * 15 / 15, (o + n) * 15 / 15)} for i, (_, _, o, n) in enumerate(queries)}
    qb = {i: ("motion", "motion", s, e) for i, (s, e, _, _) in enumerate(queries)}
    return [placed for _, _, placed in rg.retrieval.place_exemplars(si, db_b, qb, "motion")]


def test_placement_hand_worked(rg):
    # three chunks found at offset 4, wanted around second 4.0-5.0: middle frame 67 -> chunk 4; odd n: chunks 2 ... 5
    assert _place(rg, [(4.0, 5.0, 4, 3)]) == [((4, 7), (2, 5))]
    # no margins: the exemplar's range is the found one, also at the window's ends (the word methods would widen 0 ... 1 to 0 ... 2)
    assert _place(rg, [(0.2, 0.4, 0, 1)]) == [((0, 1), (0, 1))]
    assert _place(rg, [(6.0, 6.5, 9, 1)]) == [((9, 10), (6, 7))]
    # two chunks start AT the middle chunk, four chunks are centred
    assert _place(rg, [(3.0, 3.9, 5, 2)]) == [((5, 7), (3, 5))]
    assert _place(rg, [(5.0, 6.0, 1, 4)]) == [((1, 5), (3, 7))]
    # clamped at the window's start and end
    assert _place(rg, [(0.0, 0.5, 3, 5)]) == [((3, 8), (0, 5))]
    assert _place(rg, [(9.0, 10.0, 2, 3)]) == [((2, 5), (7, 10))]
    assert _place(rg, [(9.5, 12.0, 0, 7)]) == [((0, 7), (3, 10))]
    # a whole window
    assert _place(rg, [(2.0, 3.0, 0, 10)]) == [((0, 10), (0, 10))]


def test_placement_behind_a_previous_exemplar(rg):
    # the second wants chunks 3 ... 6, the first holds 2 ... 5: pushed to 5 ... 8
    assert _place(rg, [(4.0, 5.0, 4, 3), (5.0, 5.5, 0, 3)]) == [((4, 7), (2, 5)), ((0, 3), (5, 8))]
    # pushed against the window's end: shortened to what is left, the exemplar's range with it
    assert _place(rg, [(7.0, 8.0, 1, 4), (8.0, 9.0, 6, 4)]) == [((1, 5), (5, 9)), ((6, 7), (9, 10))]
    # nothing left
    assert _place(rg, [(8.0, 10.0, 0, 4), (9.0, 9.5, 5, 2)]) == [((0, 4), (6, 10)), None]


def test_placement_equals_the_restatement(rg):
    g = np.random.Generator(np.random.PCG64(5))
    for _ in range(300):
        qs, t = [], 0.0
        for _ in range(int(g.integers(1, 5))):
            s = t + float(g.uniform(0, 3))
            e = s + float(g.uniform(0, 3))
            n = int(g.integers(1, 11))
            qs.append((s, e, int(g.integers(0, 10 - n + 1)), n))
            t = s
        qs = [q for q in qs if q[0] <= 10.0]
        if qs:
            assert _place(rg, qs) == ref.place(qs)


# ------------------------------------------------------------------------------------------------------------ ranked_results
def test_ranked_results_unchanged_for_the_other_methods(rg):
    names = ["a", "b", "c", "d"]
    ranked = [([2, 0], [1, 5]), ([], []), ([3], [0])]
    seen = []

    def bounds(e, t):
        seen.append((e, t))
        return ("w%d" % e, "type", float(t), float(t) + 1)

    si, db_b = rg.retrieval.ranked_results(names, ranked, bounds)
    assert si == {0: ["c", "a"], 1: [], 2: ["d"]}
    assert db_b == {0: {"c": ("w2", "type", 1.0, 2.0), "a": ("w0", "type", 5.0, 6.0)}, 1: {}, 2: {"d": ("w3", "type", 0.0, 1.0)}}
    assert seen == [(2, 1), (0, 5), (3, 0)]                      # two arguments, as before
    # the motion method's getter receives the query's chunk count
    si2, db2 = rg.retrieval.ranked_results(names, ranked, lambda e, t, k: ("motion", "motion", float(t), float(t + k)), n_q=[3, 1, 7])
    assert si2 == si and db2[0] == {"c": ("motion", "motion", 1.0, 4.0), "a": ("motion", "motion", 5.0, 8.0)}
    assert db2[2] == {"d": ("motion", "motion", 0.0, 7.0)}


# -------------------------------------------------------------------------------------------------- header, checks, dispatch
def test_header_declares_the_sweep(rg):
    assert "rg_motion_scores_batched" in rg.capi.header_symbols()
    assert rg.capi.header_constants()["RG_VERSION"] >= 133
    restype, argtypes = rg.capi.header_prototypes()["rg_motion_scores_batched"]
    assert len(argtypes) == 16          # handle, 14 pointers and sizes, stream: no argument block


CHECK_PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "rg_retrieval_host.h"

static int run(const char* name, std::vector<int> off, std::vector<double> par, int L, int D) {
  unsigned mask = 99;
  const char* bad = rg_motion_check_queries(off.data(), par.data(), (int)off.size() - 1, L, D, &mask);
  std::printf("%s|%s|%u\n", name, bad ? bad : "ok", mask);
  return 0;
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  run("good", {0, 1, 3, 6, 13, 23}, {1, 1, 0, 0, 2, 0,  1, 1, 1, 1, 0, 0.5,  0, 0, 0, 1, 1, 0,  1, 0, 0, 0, 0, 0,  0.25, 4, 0, 0, 0, 0}, 10, 512);
  run("upper only", {0, 2}, {3, 0, 0, 0, 0, 0}, 10, 512);
  run("nq zero", {0, 2, 2}, {1, 1, 0, 0, 0, 0,  1, 1, 0, 0, 0, 0}, 10, 512);
  run("nq above L", {0, 11}, {1, 1, 0, 0, 0, 0}, 10, 512);
  run("decreasing", {0, 3, 2}, {1, 1, 0, 0, 0, 0,  1, 1, 0, 0, 0, 0}, 10, 512);
  run("start not zero", {1, 3}, {1, 1, 0, 0, 0, 0}, 10, 512);
  run("all zero", {0, 3}, {0, 0, 0, 0, 0, 0}, 10, 512);
  run("negative", {0, 3}, {1, -1, 0, 0, 0, 0}, 10, 512);
  run("nan", {0, 3}, {1, nan, 0, 0, 0, 0}, 10, 512);
  run("inf", {0, 3}, {inf, 1, 0, 0, 0, 0}, 10, 512);
  run("D", {0, 3}, {1, 1, 0, 0, 0, 0}, 10, 510);
  run("L", {0, 3}, {1, 1, 0, 0, 0, 0}, 11, 512);
  run("bonus", {0, 3}, {1, 1, 0, 0, 0, nan}, 10, 512);
  return 0;
}
"""


def test_host_argument_checks(tmp_path):
    """csrc/rg_retrieval_host.h rg_motion_check_queries -- what rg_motion_scores_batched refuses before it launches -- compiled
    into a program of its own."""
    cxx = shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = tmp_path / "check.cpp", tmp_path / "check"
    src.write_text(CHECK_PROGRAM)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {line.split("|")[0]: line.split("|")[1:] for line in out.splitlines()}
    assert got["good"] == ["ok", "15"] and got["upper only"] == ["ok", "1"]
    for name, word in (("nq zero", "n_q"), ("nq above L", "n_q"), ("decreasing", "not decrease"), ("start not zero", "start at 0"),
                       ("all zero", "all be zero"), ("negative", "non-negative"), ("nan", "finite"), ("inf", "finite"),
                       ("D", "multiple of 4"), ("L", "L <= 10"), ("bonus", "bonus")):
        assert word in got[name][0] and got[name][1] == "99", (name, got[name])       # refused, and the mask untouched


def _stub_database(rg):
    db = object.__new__(rg.retrieval.RetrievalDatabase)
    db.num_retrieval, db.index, db.gesture_index, db.prosody_index, db.motion_index = 1, None, None, None, None
    db.dataset, db._motion_gre = None, None
    db.test_indexes, db.test_dbounds, db.test_qbounds = {}, {}, {}
    return db


def test_dispatch(rg):
    db = _stub_database(rg)
    # a clip without queries needs neither index nor encoder: the base path
    assert db.retrieve("motion", None, None, None, 3, motion_queries=[]) == ({}, {}, {})
    assert db.retrieve("motion", None, None, None, 3) == ({}, {}, {})
    # with a query the index has to be built: without a dataset that is refused
    with pytest.raises(rg.capi.RgError, match="dataset"):
        db.retrieve("motion", None, None, None, 3, motion_queries=[(0.0, 1.0, _example(45))])
    with pytest.raises(NotImplementedError, match="motion"):
        db.retrieve("nonsense", None, None, None, 3)


def test_table_budget_arithmetic(rg):
    assert rg.retrieval.MotionIndex.table_bytes(1, 10, 512) == 80 * 1024
    assert rg.retrieval.MotionIndex.table_bytes(32768, 10, 512) == 2684354560 < (4 << 30)
