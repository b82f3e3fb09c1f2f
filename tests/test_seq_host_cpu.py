"""CPU: what the launch entry points of the denoiser forward require of their rg_seq_args (csrc/rg_seq_host.h: one
argument check for rg_seq_forward and rg_seq2_forward), pinned without a device: a stand-alone program
applies one mutation at a time to a valid argument block and prints what each entry point answers.  The expected texts are
those the entry points carried, each in its own copy, before they shared the check -- copied from there, not from the
header under test -- so the comparison is against what callers have always seen in rg_last_error."""
import os
import shutil
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rag-gesture_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <functional>
#include "rg_seq_host.h"

static float mem[4];
static void* const P = mem;

static rg_seq_args valid(int entry) {            // 0: rg_seq_forward, 1: rg_seq2_forward
  rg_seq_args a;
  std::memset(&a, 0, sizeof a);
  a.wstream = a.pstream = a.ustream = a.afrag = P;
  a.x = a.tbias = a.src_mask = a.qmask = mem;
  a.head = mem;
  if (entry >= 1) { a.xbuf = mem; a.gbuf = P; }
  a.L = a.B = a.T = a.S = 1;
  return a;
}
static void good_glue(rg_seq_args& a) {
  a.glue_ctr = reinterpret_cast<int*>(mem);
  a.glue.n_a = 1; a.glue.T = 1; a.glue.D = 512; a.glue.js = mem;
  a.glue.out_c_a = a.glue.out_u_a = mem; a.glue.x_a = mem;
}

struct mutation { const char* name; std::function<void(rg_seq_args&)> apply; };
#define M(name, ...) {name, [](rg_seq_args& a) { __VA_ARGS__; }}
static const mutation MUT[] = {
  M("valid", (void)a),
  M("wstream", a.wstream = nullptr), M("pstream", a.pstream = nullptr), M("ustream", a.ustream = nullptr), M("afrag", a.afrag = nullptr),
  M("x", a.x = nullptr), M("tbias", a.tbias = nullptr), M("src_mask", a.src_mask = nullptr), M("qmask", a.qmask = nullptr),
  M("head", a.head = nullptr),
  M("xbuf", a.xbuf = nullptr), M("gbuf", a.gbuf = nullptr),
  M("L=0", a.L = 0), M("L=9", a.L = 9), M("B=0", a.B = 0), M("T=0", a.T = 0), M("T=49", a.T = 49), M("T=48", a.T = 48; a.L = 8),
  M("step=S", a.step = a.S), M("step_b=-1", a.step_b = -1),
  M("dump_stage,no dump", a.dump_stage = 2), M("dump_stage,dump", a.dump_stage = 2; a.dump = mem),
  M("pairs=2", a.pairs = 2), M("pairs=1", a.pairs = 1),
  M("twin=2", a.twin = 2), M("twin=1,pairs=1", a.twin = 1; a.pairs = 1), M("twin=1", a.twin = 1),
  M("glue ok", good_glue(a)), M("glue n_a+n_b!=B", good_glue(a); a.glue.n_b = 1),
  // two violations at once: the first in the entry points' order wins
  M("head+L=0", a.head = nullptr; a.L = 0),
  M("gbuf+T=49", a.gbuf = nullptr; a.T = 49), M("T=49+step=S", a.T = 49; a.step = a.S), M("step=S+dump_stage", a.step = a.S; a.dump_stage = 2),
  M("dump_stage+pairs=2", a.dump_stage = 2; a.pairs = 2), M("pairs=2+twin=2", a.pairs = 2; a.twin = 2),
  M("twin=2+glue", good_glue(a); a.glue.n_b = 1; a.twin = 2), M("twin=2+twin&pairs", a.twin = 2; a.pairs = 1),
};

int main() {
  const rg_seq_entry* const entries[2] = {&RG_SEQ_ENTRY, &RG_SEQ2_ENTRY};
  for (int e = 0; e < 2; ++e) {
    std::printf("%d\tnull args\t%s\n", e, rg_seq_refusal(*entries[e], nullptr).c_str());
    for (const mutation& m : MUT) {
      rg_seq_args a = valid(e);
      m.apply(a);
      std::printf("%d\t%s\t%s\n", e, m.name, rg_seq_refusal(*entries[e], &a).c_str());
    }
  }
  const rg_seq_args a = valid(0);
  std::printf("flops\t%.1f\n", rg_seq_flops(a));
  return 0;
}
"""

# The texts of the entry points' RG_REQUIRE lines as they stood in csrc/rg_seq.hip and rg_seq2.hip (RG_REQUIRE
# puts "<entry point>: " in front).
NULL_ARGS = "null args"
NULL_PTR = "null pointer"
SHAPE = "unsupported shape (T <= 48, L <= 8)"
STEP = "step out of range"
DUMP = "dump_stage needs a dump buffer"
PAIRS = "pairs must be 0 or 1"
GLUE = "glue_ctr: glue must cover the B clips (n_a + n_b == B, T, D = 512), its pointers set, no dump"
BUFS2 = "the two-sequence forward needs its scratch buffers xbuf and gbuf"
TWIN_RANGE = "twin must be 0 or 1"
TWIN_PAIRS = "twin and pairs are two launch forms: set one of them"
OK = None

NAMES = ("rg_seq_forward", "rg_seq2_forward")
# case -> what (rg_seq_forward, rg_seq2_forward) answer; one entry: both
EXPECT = {
    "null args": NULL_ARGS, "valid": OK,
    **{p: NULL_PTR for p in ("wstream", "pstream", "ustream", "afrag", "x", "tbias", "src_mask", "qmask", "head")},
    "xbuf": (OK, BUFS2), "gbuf": (OK, BUFS2),
    "L=0": SHAPE, "L=9": SHAPE, "B=0": SHAPE, "T=0": SHAPE, "T=49": SHAPE, "T=48": OK,
    "step=S": STEP, "step_b=-1": STEP,
    "dump_stage,no dump": DUMP, "dump_stage,dump": OK,
    "pairs=2": PAIRS, "pairs=1": OK,
    "twin=2": (OK, TWIN_RANGE),                           # rg_seq_forward has never looked at twin
    "twin=1,pairs=1": (OK, TWIN_PAIRS),
    "twin=1": OK,
    "glue ok": OK, "glue n_a+n_b!=B": GLUE,
    "head+L=0": NULL_PTR, "gbuf+T=49": (SHAPE, BUFS2),
    "T=49+step=S": SHAPE, "step=S+dump_stage": STEP, "dump_stage+pairs=2": DUMP,
    "pairs=2+twin=2": PAIRS, "twin=2+glue": (GLUE, TWIN_RANGE), "twin=2+twin&pairs": (OK, TWIN_RANGE),
}


def test_entry_points_refuse_what_they_always_refused(tmp_path):
    """Every check of every entry point, alone and in pairs (the first in the old order wins), with the exact text; and the
    FLOP model of the smallest forward."""
    cxx = shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"      # (hipcc compiles a .cpp file for the host alone)
    assert os.path.exists(cxx), "no C++ compiler: the entry points' refusals cannot be pinned"
    src, exe = tmp_path / "refusals.cpp", tmp_path / "refusals"
    src.write_text(PROGRAM)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [line.split("\t") for line in r.stdout.splitlines()]
    got = {(int(e), case): text for e, case, text in rows[:-1]}
    assert len(got) == len(NAMES) * len(EXPECT) and {case for _, case in got} == set(EXPECT)
    for (e, case), text in sorted(got.items()):
        want = EXPECT[case][e] if isinstance(EXPECT[case], tuple) else EXPECT[case]
        assert text == ("" if want is None else "%s: %s" % (NAMES[e], want)), (NAMES[e], case)
    # L = B = T = 1: (16 + 2) u + 5 a + (10 + 2) u + 2 a, u = 2 x 512^2, a = 2 x 32 x 32 x 16
    assert rows[-1] == ["flops", "%.1f" % (30 * 2 * 512 * 512 + 7 * 2 * 32 * 32 * 16)]
