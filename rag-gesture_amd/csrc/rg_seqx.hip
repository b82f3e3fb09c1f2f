// One launch, two forms of the denoiser forward, chosen ON THE DEVICE when the launch starts (round 6).
//
// rg_seq2_forward (two sequences of a kind per workgroup: 64 workgroups x 1.37 ms for the pipeline's 128-sequence launches)
// costs 0.66 of the CU time of rg_seq_forward (one sequence per workgroup: 128 x 0.85 ms) and takes 1.6x as long.  With every
// lane of the pipeline busy the chip is full and CU time is what counts; while a pipeline fills or drains -- the first and
// the last rotation of a finite run, any gap in the traffic -- compute units idle and the latency of the 50 dependent
// launches of a chain is what counts.  The host cannot choose: chains are queued (as HIP graphs) up to 100 ms before they
// run, and it learns that no more work follows (flush()) after the last chains have been queued.  So the choice is made where
// the load is known: every lane publishes the workgroups its current launch holds (rg_lane_form, a one-thread kernel in front
// of each forward, in the same graph), takes the wide form when the other lanes' workgroups + its own wide launch fit the
// chip, and this kernel -- launched with the wide form's grid -- runs whichever form the lane's flag names; in the narrow
// form the surplus workgroups leave at once.  Both forms give the same bits (tests/test_denoiser_gpu.py), so the result of
// a batch never depends on the load.
// Bodies: csrc/rg_seq.hip (run_sequence, seq_block), csrc/rg_seq2.hip (run_pair, seq2_block), compiled here once more.
#define RG_SEQ_BODY_ONLY
// Pack form: this unit does NOT define RG_PACK2_ONE, so rg_seqx_kernel is built with the two-conversion bf16 pack
// (rg_common.h rg_pack2_bf16), while rg_seq_kernel and rg_seq2_kernel, units of their own, use the one-instruction form.  That is
// how this unit has always been built, and the two forms give the same bits.  Switching it is a change of the kernel the default
// four-lane pipeline runs -- its instructions and its register allocation (why that is delicate here) -- i.e. a
// performance change that needs its own register-count check, its own stress run and its own pull request.
#include "rg_common.h"
#include "rg_stationary.h"
#include "rg_tail.h"
#include "rg_seq_host.h"  // (all four before the bodies: they include them inside their namespaces)

namespace rgx_two {
#include "rg_seq2.hip"
}
namespace rgx_one {
#include "rg_seq.hip"
}

namespace {
constexpr int LDS_X = rgx_one::LDS_BYTES > rgx_two::LDS_BYTES ? rgx_one::LDS_BYTES : rgx_two::LDS_BYTES;

__global__ void __launch_bounds__(NTH) rg_seqx_kernel(const rg_seq_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  RG_OWN_THE_SIMD();
  // Written by rg_lane_form_kernel earlier on this stream.  EVERY workgroup of the launch must read the same value, on
  // whichever XCD it runs and however late it starts: an agent-scope atomic load (served coherently, not from a line this
  // XCD's L2 may have kept from an earlier launch), of a word that only this lane's own arbitration kernel writes and that
  // shares its 128-byte line with nothing another stream's kernels write (rg_lane_form: one line per lane).
  const int wide = a.form ? __builtin_amdgcn_readfirstlane(__hip_atomic_load(a.form, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : 0;
  if (wide) {
    if ((int)blockIdx.x < 2 * a.B) rgx_one::seq_block(a, blockIdx.x, 0, smem);
  } else {
    if ((int)blockIdx.x < rgx_two::seq2_grid(a.B, a.split, a.pairs)) rgx_two::seq2_block(a, blockIdx.x, smem);
  }
}

}  // namespace

extern "C" int rg_seqx_forward(rg_handle* h, const rg_seq_args* args_host, void* stream) {
  const std::string why = rg_seq_refusal(RG_SEQX_ENTRY, args_host);
  if (!why.empty()) { if (h) h->err = why; return RG_ERR_INVALID; }
  const rg_seq_args& a = *args_host;
  static rg_attr_once lds_once;
  RG_RESERVE_LDS(h, lds_once, rg_seqx_kernel, LDS_X);
  rg_prof_scope prof(h, stream, 3, rg_seq_flops(a));
  const int g2 = rgx_two::seq2_grid(a.B, a.split, a.pairs);
  hipLaunchKernelGGL(rg_seqx_kernel, dim3(2 * a.B > g2 ? 2 * a.B : g2), dim3(NTH), LDS_X, rg_stream(stream), a);
  RG_CHECK_LAUNCH(h);
  prof.stop();
  return RG_OK;
}
