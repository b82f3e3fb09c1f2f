// Device helpers of the sequence-stationary kernels (rg_seq.hip, rg_seq2.hip, rg_venc.hip, rg_vdec.hip): one workgroup of
// eight waves keeps its token rows on chip for a whole forward, the fp32 rows in registers (T layout: lane = token row
// 16 tb + l15, four consecutive features 16 j + 4 g4 + r of the wave's 64), the bf16 MFMA operand panels in LDS, and every
// wave streams its weight fragments for itself through a private LDS ring (rg_seq.hip).
// Only code whose instructions and arithmetic order are the same in every unit lives here; what differs stays with its unit.
// pack2 is rg_pack2_bf16 of the unit's RG_PACK2_ONE choice (rg_common.h).
#pragma once
#include "rg_common.h"
#include <type_traits>

// Lane-derived values are re-derived from an opaque copy of the lane id (`lane0`) wherever they are used: as loop invariants
// of a kernel's layer loop the address arithmetic of every unrolled LDS access would otherwise be hoisted in front of the loop
// and live (spilled) across it.
#define LANE_LOCAL()                      \
  int ln_ = lane0;                        \
  asm volatile("" : "+v"(ln_));         \
  const int lane = ln_, l15 = ln_ & 15, g4 = ln_ >> 4; \
  (void)lane; (void)l15; (void)g4

#ifdef RG_STAMPS
// Diagnostic build only (build.py RG_DIAG=1): wall-clock (100 MHz) time per category, summed per wave in the kernel's `tacc`
// (the categories: rg_seq.hip, rg_seq2.hip).
#define TSTART() const unsigned long long t0_ = __builtin_amdgcn_s_memrealtime()
#define TSTOP(cat) tacc[cat] += __builtin_amdgcn_s_memrealtime() - t0_
#else
#define TSTART()
#define TSTOP(cat)
#endif

namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((address_space(3))) void lds_void;

constexpr int DM = 512;        // model width
constexpr int TP = 48;         // token rows of a panel
constexpr int NW = 8;          // waves per workgroup; wave w owns features [64 w, 64 w + 64)
constexpr int NTH = NW * 64;

typedef f32x4 Acc[4][3];       // one sequence's T-layout rows: [16-feature block of the wave's 64][16-token block]

__device__ __forceinline__ unsigned short f2bf(float f) {
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ float bf2f(unsigned short b) { return __uint_as_float((unsigned)b << 16); }
__device__ __forceinline__ unsigned pack2(float lo, float hi) { return rg_pack2_bf16(lo, hi); }
__device__ __forceinline__ bf16x8 pack8(const float (&v)[8]) {
  return __builtin_bit_cast(bf16x8, u32x4{pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])});
}
// 8 fp32 values -> bf16 hi fragment and the bf16 residual fragment (hi * hi + hi * lo + lo * hi ~ fp32 products: the VAE units)
__device__ __forceinline__ void split_hl(const float (&v)[8], bf16x8& hi, bf16x8& lo) {
  u32x4 h, l;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const unsigned short a = f2bf(v[2 * q]), b = f2bf(v[2 * q + 1]);
    h[q] = (unsigned)a | ((unsigned)b << 16);
    l[q] = pack2(v[2 * q] - bf2f(a), v[2 * q + 1] - bf2f(b));
  }
  hi = __builtin_bit_cast(bf16x8, h);
  lo = __builtin_bit_cast(bf16x8, l);
}
__device__ __forceinline__ float silu_f(float v) {
  return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -1.44269504088896340736f));
}
__device__ __forceinline__ float gelu_fast(float v) { return rg_gelu_erf(v); }

template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory"); }
// lgkmcnt(0) as the BUILTIN: the compiler's wait-count bookkeeping sees it, so it does not add a wait of its own in front of
// the first use of a register that this wait already covers (after an inline-asm wait it does: a full lgkmcnt(0) right behind
// the next fragment's LDS read, which exposes that read's latency).  The empty asm keeps memory operations from crossing.
__device__ __forceinline__ void wait_lds() {
  __builtin_amdgcn_s_waitcnt(0xc07f);
  asm volatile("" ::: "memory");
}
__device__ __forceinline__ void bar() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

__device__ __forceinline__ void zero(Acc& a) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int tb = 0; tb < 3; ++tb) a[j][tb] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---- the wave's fetch cursor over its fetch program (one descriptor per segment in LDS, in consumption order, + a sentinel
// whose count is never reached).  All state is wave-uniform (scalar registers): the source of a fragment is a buffer
// descriptor of the segment (for this wave) + a scalar offset, the lane only adds its 16 bytes.  RD ring slots of 1 KiB, all
// of them in flight except the one being read.  Desc decodes one descriptor: {base of this wave's fragments, count}.
// The ring's first fill is the kernel's own loop, `cur.load_seg(); for (s < RD) cur.issue(s);`: unrolled inside a member
// function it comes out as other code (60 more instructions in rg_venc_kernel).
// 16-byte descriptors {address of wave 0 (64 bits), count, wave stride in fragments}: rg_seq, rg_venc, rg_vdec
struct rg_desc16 {
  static constexpr int BYTES = 16;
  static constexpr bool RARE_END = false;
  __device__ static __forceinline__ unsigned char* decode(const unsigned char* p, int wave, int& cnt) {
    const u32x4 d = *reinterpret_cast<const u32x4*>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane(d[0]), hi = __builtin_amdgcn_readfirstlane(d[1]);
    cnt = __builtin_amdgcn_readfirstlane(d[2]);
    const unsigned stride = __builtin_amdgcn_readfirstlane(d[3]);
    return reinterpret_cast<unsigned char*>(((unsigned long long)hi << 32) | lo) + ((size_t)(wave * stride) << 10);
  }
};

// 8-byte descriptors {address of wave 0 (48 bits), count (8), wave stride (8)}, a segment's end marked rare: rg_seq2
struct rg_desc8 {
  static constexpr int BYTES = 8;
  static constexpr bool RARE_END = true;
  __device__ static __forceinline__ unsigned char* decode(const unsigned char* p, int wave, int& cnt) {
    const u32x2 d = *reinterpret_cast<const u32x2*>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane(d[0]), w1 = __builtin_amdgcn_readfirstlane(d[1]);
    cnt = (w1 >> 16) & 0xffu;
    const unsigned stride = w1 >> 24;
    return reinterpret_cast<unsigned char*>(((unsigned long long)(w1 & 0xffffu) << 32) | lo) + ((size_t)(wave * stride) << 10);
  }
};

template <int RD_, class Desc>
struct rg_cursor {
  static constexpr int RD = RD_;
  unsigned char* const ring;     // the wave's RD slots
  const unsigned char* const desc;
  const int& wave;               // (the kernel's own: held by reference as the lambdas before this type did, the same code)
  const int lane16;
  int ie = 0, ir = 0;            // segment, fragment inside it
  int cnt = 0;
  __amdgpu_buffer_rsrc_t rsrc;
  int head = 0;                  // ring slot of the oldest fragment in flight

  __device__ __forceinline__ rg_cursor(unsigned char* ring_, const unsigned char* desc_, const int& wave_, int lane0)
      : ring(ring_), desc(desc_), wave(wave_), lane16(lane0 * 16) {}
  __device__ __forceinline__ void load_seg() {
    unsigned char* base = Desc::decode(desc + ie * Desc::BYTES, wave, cnt);
    rsrc = __builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7fffffff, 0x00020000);
  }
  __device__ __forceinline__ void advance() {
    if constexpr (Desc::RARE_END) {
      if (__builtin_expect(++ir == cnt, 0)) {
        ir = 0;
        ++ie;
        load_seg();
      }
    } else {
      if (++ir == cnt) {
        ir = 0;
        ++ie;
        load_seg();
      }
    }
  }
  // the stream's next fragment -> ring slot `slot` (LDS-DMA)
  __device__ __forceinline__ void issue(int slot) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void*)(ring + slot * 1024), 16, lane16, ir << 10, 0, 0);
    advance();
  }
  // ... or straight into registers
  __device__ __forceinline__ void issue_reg(u32x4& dst) {
    dst = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane16, ir << 10, 0);
    advance();
  }
  // consume(): the oldest fragment has landed (at most RD - 1 younger vector-memory operations outstanding); returns its slot.
  // release(): the slot's bytes are in registers -> refill it.
  __device__ __forceinline__ const unsigned char* consume() {
    wait_vmcnt<RD - 1>();
    return ring + head * 1024;
  }
  __device__ __forceinline__ void release() {
    wait_lds();
    issue(head);
    head = head + 1 == RD ? 0 : head + 1;
  }
};

// ---- unit GEMM: acc += W_unit x panel over K = 512 (16 steps of 32), one sequence; NJ weight fragments per step (NJ = 4: the
// wave's 64 features, NJ = 2: the 32 features of one head).  STD = false: T layout (A = weights); true: standard layout (A =
// panel).  The weight stream's fragments RD ... of the unit are loaded STRAIGHT INTO REGISTERS (eight in rotation, RD
// fragments in flight): only the unit's first RD fragments -- issued before the unit starts, across its epilogue -- come
// through the LDS ring; the last RD iterations refill the ring's slots for whatever the stream holds next.  One in-order
// pipeline, the destination depends on the fragment's position only; `head` leaves as it came.  (rg_seq2.hip has the
// two-sequence form, six panel fragments per k-step.)
template <int NJ, bool STD, class Cur, class A>
__device__ __forceinline__ void gemm_unit_reg(Cur& cur, A& acc, const unsigned char* panel, const int& lane0) {
  constexpr int RD = Cur::RD;
  static_assert((16 * NJ) % 8 == 0 && 8 % NJ == 0 && RD <= 8 && RD >= 2, "groups of eight fragments, RD in flight");
  LANE_LOCAL();
  const unsigned char* pl = panel + lane * 16;
  const unsigned char* rl = cur.ring + lane * 16;
  bf16x8 pf[3];
  u32x4 wr[8];
  int hs = cur.head;
  wait_vmcnt<RD - 1>();
  wr[0] = *reinterpret_cast<const u32x4*>(rl + hs * 1024);
  hs = hs + 1 == RD ? 0 : hs + 1;
#pragma unroll
  for (int tb = 0; tb < 3; ++tb) pf[tb] = *reinterpret_cast<const bf16x8*>(pl + ((tb * 16) << 10));
  auto group = [&](const int s0, auto first_tag, auto last_tag) {      // fragments [NJ s0, NJ s0 + 8)
    constexpr bool FIRST = decltype(first_tag)::value, LAST = decltype(last_tag)::value;
#pragma unroll
    for (int f = 0; f < 8; ++f) {
      const int j = f % NJ, s = s0 + f / NJ;
      if (FIRST && f + 1 < RD) {      // the next fragment sits in the ring: landed when at most RD - 2 younger loads are outstanding
        wait_vmcnt<RD - 2>();
        wr[f + 1] = *reinterpret_cast<const u32x4*>(rl + hs * 1024);
        hs = hs + 1 == RD ? 0 : hs + 1;
      }
      const bf16x8 wv = __builtin_bit_cast(bf16x8, wr[f]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int tb = 0; tb < 3; ++tb) {
        acc[j][tb] = STD ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[tb], wv, acc[j][tb], 0, 0, 0)
                         : __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv, pf[tb], acc[j][tb], 0, 0, 0);
        if (j == NJ - 1) {           // re-read for the next k-step right behind its last use (behind the panel's end: valid LDS, unused)
          pf[tb] = *reinterpret_cast<const bf16x8*>(pl + ((tb * 16 + s + 1) << 10));
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (LAST && f >= 8 - RD) {     // the stream's next RD items go to the ring (slots in the order they were read from)
        cur.issue(hs);
        hs = hs + 1 == RD ? 0 : hs + 1;
      } else {
        cur.issue_reg(wr[(f + RD) & 7]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  group(0, std::true_type(), std::false_type());
#pragma unroll 1
  for (int s0 = 8 / NJ; s0 < 16 - 8 / NJ; s0 += 8 / NJ) group(s0, std::false_type(), std::false_type());
  group(16 - 8 / NJ, std::false_type(), std::true_type());
}

// ---- parameter fragment [4][64] fp32 at the head of every unit: vector p for the wave's 64 features, T layout (features
// 16 j + 4 g4 + r)
__device__ __forceinline__ f32x4 par_t(const unsigned char* slot, int p, int j, int g4) {
  return *reinterpret_cast<const f32x4*>(slot + (p * 64 + 16 * j + 4 * g4) * 4);
}
__device__ __forceinline__ void add_bias_t(Acc& acc, const unsigned char* slot, const int& lane0) {
  LANE_LOCAL();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x4 b = par_t(slot, 0, j, g4);
#pragma unroll
    for (int tb = 0; tb < 3; ++tb) acc[j][tb] += b;
  }
}
// ---- T-layout values -> bf16 panel fragments (8-byte stores): features 64 wave + 16 j + 4 g4 + [0, 4) of token 16 tb + l15
__device__ __forceinline__ void panel_store(unsigned char* panel, const int& wave, int l15, int g4, int j, int tb, float v0, float v1, float v2, float v3) {
  const int s = 2 * wave + (j >> 1), gq = 2 * (j & 1) + (g4 >> 1);
  *reinterpret_cast<u32x2*>(panel + ((tb * 16 + s) << 10) + ((l15 + 16 * gq) << 4) + 8 * (g4 & 1)) = u32x2{pack2(v0, v1), pack2(v2, v3)};
}
__device__ __forceinline__ void write_raw(unsigned char* panel, const Acc& v, const int& wave, const int& lane0) {
  LANE_LOCAL();
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int tb = 0; tb < 3; ++tb) panel_store(panel, wave, l15, g4, j, tb, v[j][tb][0], v[j][tb][1], v[j][tb][2], v[j][tb][3]);
}

// ---- LayerNorm statistics of the three token rows a lane holds, the VAE units' form: per-wave sum and sum of squares in one
// pass over the registers, in a scalar loop, added up across the waves behind one barrier (partials: sStat [NW][TP][2]);
// variance = E[x^2] - mean^2 in fp32.  (The denoiser units sum with rg_sum_sq16, another association: different bits.)
__device__ __forceinline__ void row_stats_vae(const Acc& v, float (&mean)[3], float (&rstd)[3], float* const& sStat, const int& wave, const int& lane0) {
  LANE_LOCAL();
#pragma unroll
  for (int tb = 0; tb < 3; ++tb) {
    float s = 0.f, ss = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s += (v[j][tb][0] + v[j][tb][1]) + (v[j][tb][2] + v[j][tb][3]);
#pragma unroll
      for (int r = 0; r < 4; ++r) ss = fmaf(v[j][tb][r], v[j][tb][r], ss);
    }
    s = rg_xsum4(s);
    ss = rg_xsum4(ss);
    if (g4 == 0) *reinterpret_cast<float2*>(sStat + (wave * TP + 16 * tb + l15) * 2) = make_float2(s, ss);
  }
  bar();
#pragma unroll
  for (int tb = 0; tb < 3; ++tb) {
    float tot = 0.f, tot2 = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float2 p = *reinterpret_cast<const float2*>(sStat + (w * TP + 16 * tb + l15) * 2);
      tot += p.x;
      tot2 += p.y;
    }
    const float mu = tot * (1.0f / DM);
    mean[tb] = mu;
    rstd[tb] = rsqrtf(fmaxf(fmaf(-mu, mu, tot2 * (1.0f / DM)), 0.f) + 1e-5f);
  }
}

}  // namespace
