"""CPU: what rg_seq2_forward_many (the twin-form forwards of several sessions in one launch, csrc/rg_seq2.hip) requires of its
list of rg_seq_args (csrc/rg_seq_host.h rg_seq2_many_refusal), pinned without a device in the manner of
test_seq_many_host_cpu.py: a stand-alone program mutates a valid set of sessions and prints what the check answers.  Also: the
header declares the entry point and adds no argument block for it (the kernel's parameter block stays in the .hip file)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rag-gesture_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>
#include "rg_seq_host.h"

static float mem[4], other[4];
static void* const P = mem;

static rg_seq_args valid(int B) {
  rg_seq_args a;
  std::memset(&a, 0, sizeof a);
  a.wstream = a.pstream = a.ustream = a.afrag = P;
  a.x = a.tbias = a.src_mask = a.qmask = mem;
  a.head = a.xbuf = mem;
  a.gbuf = mem;
  a.L = 2; a.T = 27; a.S = 5; a.B = B;
  a.step = B % 5;
  a.twin = 1;
  return a;
}
static void good_glue(rg_seq_args& a) {      // the co-batched form: both groups
  a.glue_ctr = reinterpret_cast<int*>(mem);
  a.glue.n_a = 1; a.glue.n_b = a.B - 1; a.glue.T = a.T; a.glue.D = 512; a.glue.js = mem;
  a.glue.out_c_a = a.glue.out_u_a = mem; a.glue.x_a = mem;
  a.glue.out_c_b = a.glue.out_u_b = mem; a.glue.x_b = mem;
}

// a mutation of session `at` of a set of `n` valid sessions (B = 1, 2, ...)
struct mutation { const char* name; int n, at; std::function<void(rg_seq_args&)> apply; };
#define M(name, n, at, ...) {name, n, at, [](rg_seq_args& a) { __VA_ARGS__; }}
static const mutation MUT[] = {
  M("one", 1, 0, (void)a), M("two", 2, 0, (void)a), M("max", RG_SEQ_MANY_MAX, 0, (void)a),
  M("max, tails", RG_SEQ_MANY_MAX, RG_SEQ_MANY_MAX - 1, good_glue(a)),
  M("own step, split", 3, 1, a.step = 4; a.step_b = 2; a.split = 1),
  M("L differs", 2, 1, a.L = 3), M("T differs", 3, 2, a.T = 43), M("S differs", 2, 1, a.S = 6),
  M("wstream differs", 2, 1, a.wstream = other), M("pstream differs", 3, 1, a.pstream = other), M("ustream differs", 2, 1, a.ustream = other),
  M("afrag differs", 2, 1, a.afrag = other), M("xbuf differs", 2, 1, a.xbuf = other),
  M("not twin", 2, 1, a.twin = 0), M("not twin first", 2, 0, a.twin = 0), M("not twin alone", 1, 0, a.twin = 0), M("twin=2", 2, 1, a.twin = 2),
  M("pairs", 2, 1, a.pairs = 1), M("pairs, not twin", 2, 1, a.pairs = 1; a.twin = 0), M("pairs=2", 2, 1, a.pairs = 2),
  M("dump stage", 2, 1, a.dump_stage = 2; a.dump = mem), M("dump stage, no buffer", 2, 0, a.dump_stage = 2),
  M("no xbuf", 2, 1, a.xbuf = nullptr), M("no gbuf", 2, 0, a.gbuf = nullptr),
  M("head", 3, 2, a.head = nullptr), M("x", 2, 0, a.x = nullptr),
  M("T=49", 2, 1, a.T = 49), M("B=0", 2, 1, a.B = 0), M("step=S", 2, 1, a.step = a.S), M("step_b=-1", 4, 3, a.step_b = -1),
  M("glue n_a+n_b!=B", 2, 1, good_glue(a); a.glue.n_b = 2), M("glue T", 2, 1, good_glue(a); a.glue.T = 1),
  M("glue group b without x", 2, 1, good_glue(a); a.glue.x_b = nullptr),
  M("glue in_seq without noise", 2, 1, good_glue(a); a.glue.in_seq_next = mem),
  // two violations at once: the session's own come first, then the form, then what the sessions share
  M("head+L differs", 2, 1, a.head = nullptr; a.L = 3), M("not twin+T differs", 2, 1, a.twin = 0; a.T = 43), M("L+wstream differ", 2, 1, a.L = 3; a.wstream = other),
};

static void report(const char* name, const rg_seq_args* const* list, int n) { std::printf("%s\t%s\n", name, rg_seq2_many_refusal(list, n).c_str()); }

int main() {
  for (const mutation& m : MUT) {
    std::vector<rg_seq_args> a;
    for (int i = 0; i < m.n; ++i) a.push_back(valid(1 + i));
    m.apply(a[m.at]);
    std::vector<const rg_seq_args*> list;
    for (const rg_seq_args& s : a) list.push_back(&s);
    report(m.name, list.data(), m.n);
  }
  std::vector<rg_seq_args> a(RG_SEQ_MANY_MAX + 1, valid(1));
  std::vector<const rg_seq_args*> list;
  for (const rg_seq_args& s : a) list.push_back(&s);
  report("null list", nullptr, 2);
  report("n=0", list.data(), 0);
  report("n=-1", list.data(), -1);
  report("too many", list.data(), RG_SEQ_MANY_MAX + 1);
  list[1] = nullptr;
  report("null session", list.data(), 3);
  report("null session behind n", list.data(), 1);
  // n == 1 asks of a twin session what rg_seq2_forward asks of it
  rg_seq_args one = valid(3);
  const rg_seq_args* lone = &one;
  std::printf("n=1 as rg_seq2_forward\t%d\n", (int)(rg_seq2_many_refusal(&lone, 1).empty() && rg_seq_refusal(RG_SEQ2_ENTRY, &one).empty()));
  return 0;
}
"""

NAME = "rg_seq2_forward_many"
LIST = "null or empty list of sessions"
MANY = "too many sessions (at most RG_SEQ_MANY_MAX)"
AGREE = "the sessions must agree in L, T and S"
STREAMS = "the sessions must share the weight, parameter and table streams"
NOT_TWIN = "every session must be in the twin form (twin == 1): a grouped launch runs one workgroup per clip"
TWIN_RANGE = "twin must be 0 or 1"
TWIN_PAIRS = "twin and pairs are two launch forms: set one of them"
DUMP = "diagnostic dumps: use rg_seq2_forward"
BUFS = "the two-sequence forward needs its scratch buffers xbuf and gbuf"
# each session's own requirements: the texts of rg_seq_refusal (test_seq_host_cpu.py pins them for the other entry points)
NULL_ARGS, NULL_PTR, SHAPE, STEP = "null args", "null pointer", "unsupported shape (T <= 48, L <= 8)", "step out of range"
PAIRS_RANGE = "pairs must be 0 or 1"
GLUE = "glue_ctr: glue must cover the B clips (n_a + n_b == B, T, D = 512), its pointers set, no dump"
OK = None

EXPECT = {
    "one": OK, "two": OK, "max": OK, "max, tails": OK, "own step, split": OK, "afrag differs": OK, "xbuf differs": OK,
    "L differs": AGREE, "T differs": AGREE, "S differs": AGREE,
    "wstream differs": STREAMS, "pstream differs": STREAMS, "ustream differs": STREAMS,
    "not twin": NOT_TWIN, "not twin first": NOT_TWIN, "not twin alone": NOT_TWIN, "twin=2": TWIN_RANGE,
    "pairs": TWIN_PAIRS, "pairs, not twin": NOT_TWIN, "pairs=2": PAIRS_RANGE,
    "dump stage": DUMP, "dump stage, no buffer": DUMP, "no xbuf": BUFS, "no gbuf": BUFS,
    "head": NULL_PTR, "x": NULL_PTR, "T=49": SHAPE, "B=0": SHAPE, "step=S": STEP, "step_b=-1": STEP,
    "glue n_a+n_b!=B": GLUE, "glue T": GLUE, "glue group b without x": GLUE, "glue in_seq without noise": GLUE,
    "head+L differs": NULL_PTR, "not twin+T differs": NOT_TWIN, "L+wstream differ": AGREE,
    "null list": LIST, "n=0": LIST, "n=-1": LIST, "too many": MANY, "null session": NULL_ARGS, "null session behind n": OK,
}


def test_grouped_twin_forward_refusals(tmp_path):
    """Every refusal of rg_seq2_forward_many by its text; valid sets of 1, 2 and RG_SEQ_MANY_MAX twin sessions pass."""
    cxx = shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"      # (hipcc compiles a .cpp file for the host alone)
    assert os.path.exists(cxx), "no C++ compiler: the entry point's refusals cannot be pinned"
    src, exe = tmp_path / "many2.cpp", tmp_path / "many2"
    src.write_text(PROGRAM)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(line.split("\t") for line in r.stdout.splitlines())
    assert got.pop("n=1 as rg_seq2_forward") == "1"
    assert set(got) == set(EXPECT) and len(r.stdout.splitlines()) == len(EXPECT) + 1
    for case, want in EXPECT.items():
        assert got[case] == ("" if want is None else "%s: %s" % (NAME, want)), case


def test_header_declares_the_entry_point_and_no_new_block():
    import importlib
    capi = importlib.import_module("rag-gesture_amd.capi")
    assert len(capi.header_structs()) == 23
    assert capi.header_constants()["RG_VERSION"] >= 128
    restype, argtypes = capi.header_prototypes()["rg_seq2_forward_many"]
    assert len(argtypes) == 4 and "rg_seq2_forward_many" in capi.header_symbols()
    assert argtypes == capi.header_prototypes()["rg_seq_forward_many"][1]
