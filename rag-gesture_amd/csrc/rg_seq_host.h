// Host side of the denoiser forward's launch entry points (rg_seq.hip and rg_seq2.hip with their grouped forms): the
// argument check and the FLOP model.  Plain C++ without HIP: tests/test_seq_host_cpu.py compiles it alone.
#pragma once
#include <string>

#include "../../include/rg_gesture.h"

// An entry point: its name (a refusal reads "<name>: <text>", as RG_REQUIRE builds it from __func__) and the text of every check
// that only some of them make, NULL where this one does not: xbuf && gbuf; dump_stage == 0 (NULL: a dump stage is allowed
// and needs a dump buffer); twin is 0 or 1; not twin with pairs; twin == 0.  rg_seq_forward has never looked at `twin`
// (include/rg_gesture.h: "ignores it"): a refusal there would be a change of behaviour, so it has none.
struct rg_seq_entry { const char *name, *need_bufs, *no_dump, *twin_range, *twin_pairs, *no_twin; };
constexpr rg_seq_entry RG_SEQ_ENTRY = {"rg_seq_forward", nullptr, nullptr, nullptr, nullptr, nullptr};
constexpr rg_seq_entry RG_SEQ2_ENTRY = {"rg_seq2_forward", "the two-sequence forward needs its scratch buffers xbuf and gbuf", nullptr,
                                        "twin must be 0 or 1", "twin and pairs are two launch forms: set one of them", nullptr};

// What the entry points require of args->glue when args->glue_ctr is set (the loop step's update behind the forward: rg_tail.h).
inline bool rg_seq_glue_ok(const rg_seq_args& a) {
  if (!a.glue_ctr) return true;
  const rg_glue_args& g = a.glue;
  if (a.dump_stage || g.n_a < 0 || g.n_b < 0 || g.n_a + g.n_b != a.B || g.T != a.T || g.D != 512 || !g.js || g.g_iter_next < 0) return false;
  if (g.n_a && !(g.out_c_a && g.out_u_a && g.x_a)) return false;
  if (g.n_b && !(g.out_c_b && g.out_u_b && g.x_b)) return false;
  return !g.in_seq_next || g.noise_next;
}

// The first requirement of entry point `e` that `args` fails, as the text of rg_last_error, or "" when the launch may be made.
inline std::string rg_seq_refusal(const rg_seq_entry& e, const rg_seq_args* args) {
  const char* why = nullptr;
  if (!args) {
    why = "null args";
  } else {
    const rg_seq_args& a = *args;
    if (!(a.wstream && a.pstream && a.ustream && a.afrag && a.x && a.tbias && a.src_mask && a.qmask && a.head)) why = "null pointer";
    else if (e.need_bufs && !(a.xbuf && a.gbuf)) why = e.need_bufs;
    else if (!(a.L >= 1 && a.L <= 8 && a.B >= 1 && a.T >= 1 && a.T <= 48)) why = "unsupported shape (T <= 48, L <= 8)";
    else if (!(a.step >= 0 && a.step < a.S && a.step_b >= 0 && a.step_b < a.S)) why = "step out of range";
    else if (e.no_dump && a.dump_stage != 0) why = e.no_dump;
    else if (!e.no_dump && a.dump_stage != 0 && !a.dump) why = "dump_stage needs a dump buffer";
    else if (!(a.pairs == 0 || a.pairs == 1)) why = "pairs must be 0 or 1";
    else if (e.twin_range && !(a.twin == 0 || a.twin == 1)) why = e.twin_range;
    else if (e.twin_pairs && a.twin && a.pairs) why = e.twin_pairs;
    else if (e.no_twin && a.twin) why = e.no_twin;
    else if (!rg_seq_glue_ok(a)) why = "glue_ctr: glue must cover the B clips (n_a + n_b == B, T, D = 512), its pointers set, no dump";
  }
  return why ? std::string(e.name) + ": " + why : std::string();
}

// rg_seq_forward_many: the one-workgroup-per-sequence form of rg_seq_forward for every session, nothing of the other forms.
constexpr rg_seq_entry RG_SEQ_MANY_ENTRY = {"rg_seq_forward_many", nullptr, "diagnostic dumps: use rg_seq_forward", nullptr, nullptr,
                                            "the twin form is rg_seq2_forward's: a grouped launch runs one workgroup per sequence"};

// The first requirement of rg_seq_forward_many that the n sessions fail, or "": each session's own (rg_seq_refusal), the form,
// and what the sessions must share.
inline std::string rg_seq_many_refusal(const rg_seq_args* const* args, const int n) {
  const std::string name = std::string(RG_SEQ_MANY_ENTRY.name) + ": ";
  if (!args || n < 1) return name + "null or empty list of sessions";
  if (n > RG_SEQ_MANY_MAX) return name + "too many sessions (at most RG_SEQ_MANY_MAX)";
  for (int i = 0; i < n; ++i) {
    const std::string why = rg_seq_refusal(RG_SEQ_MANY_ENTRY, args[i]);
    if (!why.empty()) return why;
    const rg_seq_args &a = *args[i], &a0 = *args[0];
    if (a.pairs) return name + "pairs is another launch form: a grouped launch runs one workgroup per sequence";
    if (!(a.L == a0.L && a.T == a0.T && a.S == a0.S)) return name + "the sessions must agree in L, T and S";
    if (!(a.wstream == a0.wstream && a.pstream == a0.pstream && a.ustream == a0.ustream))
      return name + "the sessions must share the weight, parameter and table streams";
  }
  return std::string();
}

// rg_seq2_forward_many: the twin form of rg_seq2_forward for every session, nothing of the other forms.
constexpr rg_seq_entry RG_SEQ2_MANY_ENTRY = {"rg_seq2_forward_many", RG_SEQ2_ENTRY.need_bufs, "diagnostic dumps: use rg_seq2_forward",
                                             RG_SEQ2_ENTRY.twin_range, RG_SEQ2_ENTRY.twin_pairs, nullptr};

// The first requirement of rg_seq2_forward_many that the n sessions fail, or "": each session's own (rg_seq_refusal: what
// rg_seq2_forward asks, the glue included, and no dump), the twin form -- a session with pairs set fails either "twin and pairs"
// or this one -- and what the sessions must share.
inline std::string rg_seq2_many_refusal(const rg_seq_args* const* args, const int n) {
  const std::string name = std::string(RG_SEQ2_MANY_ENTRY.name) + ": ";
  if (!args || n < 1) return name + "null or empty list of sessions";
  if (n > RG_SEQ_MANY_MAX) return name + "too many sessions (at most RG_SEQ_MANY_MAX)";
  for (int i = 0; i < n; ++i) {
    const std::string why = rg_seq_refusal(RG_SEQ2_MANY_ENTRY, args[i]);
    if (!why.empty()) return why;
    const rg_seq_args &a = *args[i], &a0 = *args[0];
    if (!a.twin) return name + "every session must be in the twin form (twin == 1): a grouped launch runs one workgroup per clip";
    if (!(a.L == a0.L && a.T == a0.T && a.S == a0.S)) return name + "the sessions must agree in L, T and S";
    if (!(a.wstream == a0.wstream && a.pstream == a0.pstream && a.ustream == a0.ustream))
      return name + "the sessions must share the weight, parameter and table streams";
  }
  return std::string();
}

// Algorithmic FLOPs of a forward of B clips (bench.py's roofline): per layer all RG_SEQ_UPL units for a conditional sequence, 10 for
// a classifier-free one (its cross attention is tabulated); the embedding and the head for both.
inline double rg_seq_flops(const rg_seq_args& a) {
  const double unit = 2.0 * a.T * 512 * 512, att = 2.0 * a.T * 32 * 32 * 16;      // one 512 x 512 GEMM; one q A (or K^T V) over 16 heads
  const double cond = (RG_SEQ_UPL * a.L + 2) * unit + a.L * (2 + 3) * att, unc = (10 * a.L + 2) * unit + a.L * 2 * att;
  return a.B * (cond + unc);
}
