// Foot skating measured and contact feet planted (include/rg_gesture.h; this project's own: the reference
// has no counterpart).
//   rg_foot_skate_sums : per clip the RG_FOOT_SUMS counts and sums behind skate / slide / contact_slide / contact_moving
//   rg_foot_plant      : the translation minus the accumulated horizontal slide of the feet whose contact flag is set
// Both read the world positions of the four foot joints (7, 8, 10, 11) from joints [F][55][3] and walk a clip's pairs (t, t + 1)
// in tiles of FOOT_THREADS, one workgroup per clip: a clip's result depends on that clip alone.  Arithmetic in fp64 on the fp32
// inputs, every product and sum rounded on its own (no FMA contraction), so a term is the same double the numpy restatement
// of tests/foot_ref.py computes.  Latency-bound: a clip of 150 frames is one tile.
#include "rg_reduce.h"
#include "rg_smplx.h"

#pragma clang fp contract(off)

namespace {

constexpr int FOOT_THREADS = 256;
constexpr int FOOT_WAVES = FOOT_THREADS / 64;
constexpr int N_FOOT = 4;

__device__ __forceinline__ int foot_joint(int k) { return k < 2 ? 7 + k : 8 + k; }   // 7, 8, 10, 11 (dataset.CONTACT_JOINTS)

// joint k of pair t: both ends, as doubles
struct foot_pair {
  double x0, y0, z0, x1, y1, z1;
};
__device__ __forceinline__ foot_pair foot_load(const float* J, int t, int k) {
  const float* p0 = J + ((size_t)t * NJ + foot_joint(k)) * 3;
  const float* p1 = p0 + POSE_DIM;
  return {(double)p0[0], (double)p0[1], (double)p0[2], (double)p1[0], (double)p1[1], (double)p1[2]};
}

// the lowest y of each foot joint over the clip's n frames, for every thread (fp32 minimum: exact in any order); red [4][4]
__device__ __forceinline__ void foot_lowest(const float* J, int n, float (*red)[N_FOOT], double* ymin) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float m[N_FOOT];
#pragma unroll
  for (int k = 0; k < N_FOOT; ++k) m[k] = INFINITY;
  for (int t = threadIdx.x; t < n; t += FOOT_THREADS)
#pragma unroll
    for (int k = 0; k < N_FOOT; ++k) m[k] = fminf(m[k], J[((size_t)t * NJ + foot_joint(k)) * 3 + 1]);
#pragma unroll
  for (int k = 0; k < N_FOOT; ++k) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m[k] = fminf(m[k], __shfl_xor(m[k], s));
    if (lane == 0) red[wave][k] = m[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N_FOOT; ++k) {
    float v = red[0][k];
    for (int w = 1; w < FOOT_WAVES; ++w) v = fminf(v, red[w][k]);
    ymin[k] = (double)v;
  }
}

// one workgroup per clip.  A thread owns pair base + threadIdx.x of every tile and adds its four joints in order; the six
// running values are summed over the lanes (xor butterfly), the waves 0 to 3 and the tiles in order (rg_reduce.h's order).
__global__ void __launch_bounds__(FOOT_THREADS) foot_skate_kernel(const float* joints, const float* contact, const int* clip_off,
                                                                  float fps_, float height_, float speed_, float cthr_, float dthr_,
                                                                  double* sums) {
  constexpr int NV = RG_FOOT_SUMS - 1;                 // entries 1 .. 6 (entry 0 is the pair count)
  __shared__ float lowest[FOOT_WAVES][N_FOOT];
  __shared__ double red[FOOT_WAVES][NV];
  const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = clip_off[c], n = clip_off[c + 1] - r0;
  const float* J = joints + (size_t)r0 * POSE_DIM;
  const float* C = contact ? contact + (size_t)r0 * N_FOOT : nullptr;
  const double fps = fps_, height = height_, speed = speed_, cthr = cthr_, dthr = dthr_;
  double ymin[N_FOOT];
  foot_lowest(J, n, lowest, ymin);
  double acc[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) acc[i] = 0.0;
  for (int base = 0; base < n - 1; base += FOOT_THREADS) {
    const int t = base + threadIdx.x;
    double v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = 0.0;
    if (t < n - 1) {
      bool skating = false;
#pragma unroll
      for (int k = 0; k < N_FOOT; ++k) {
        const foot_pair p = foot_load(J, t, k);
        const double dx = p.x1 - p.x0, dy = p.y1 - p.y0, dz = p.z1 - p.z0;
        const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
        if (p.y0 - ymin[k] < height && p.y1 - ymin[k] < height) {      // grounded
          const double s = fps * sqrt(xx + zz);
          v[1] += 1.0;
          v[2] += s;
          skating = skating || s > speed;
        }
        if (C && (double)C[(size_t)t * N_FOOT + k] >= cthr) {                                  // flagged
          const double d = sqrt((xx + yy) + zz);
          v[3] += 1.0;
          v[4] += d;
          if (d >= dthr) v[5] += 1.0;
        }
      }
      v[0] = skating ? 1.0 : 0.0;
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum_f64(v[i]);
    __syncthreads();                                   // (the last tile's red has been read)
    if (lane == 0)
#pragma unroll
      for (int i = 0; i < NV; ++i) red[wave][i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      double s = 0.0;
      for (int w = 0; w < FOOT_WAVES; ++w) s += red[w][i];
      acc[i] += s;
    }
  }
  if (threadIdx.x == 0) {
    double* o = sums + (size_t)c * RG_FOOT_SUMS;
    o[0] = (double)(n - 1);
#pragma unroll
    for (int i = 0; i < NV; ++i) o[1 + i] = acc[i];
  }
}

// one workgroup per clip.  e[t] = -mean over the flagged joints of pair t of (dx, dz), or -0 without a flag; off[t + 1] is the
// inclusive prefix sum of e: inside a wave by shuffles, across the waves in order through LDS, from tile to tile in `carry`.
// Everything starts from -0.0, because x + -0.0 is x for EVERY x (x + +0.0 turns -0 into +0): a clip without flags comes back
// bit for bit.  A thread reads and writes the same row t + 1, so trans_out may be trans_in.
__global__ void __launch_bounds__(FOOT_THREADS) foot_plant_kernel(const float* joints, const float* contact, const float* trans_in,
                                                                  const int* clip_off, float cthr_, float* trans_out) {
  __shared__ double tot[FOOT_WAVES][2];
  const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = clip_off[c], n = clip_off[c + 1] - r0;
  const float* J = joints + (size_t)r0 * POSE_DIM;
  const float* C = contact + (size_t)r0 * N_FOOT;
  const float* in = trans_in + (size_t)r0 * 3;
  float* out = trans_out + (size_t)r0 * 3;
  const double cthr = cthr_;
  if (threadIdx.x == 0) {                              // off[0] = 0
    const float x = in[0], y = in[1], z = in[2];
    out[0] = x, out[1] = y, out[2] = z;
  }
  double carry_x = -0.0, carry_z = -0.0;
  for (int base = 0; base < n - 1; base += FOOT_THREADS) {
    const int t = base + threadIdx.x;
    double vx = -0.0, vz = -0.0;
    if (t < n - 1) {
      double sx = 0.0, sz = 0.0;
      int m = 0;
#pragma unroll
      for (int k = 0; k < N_FOOT; ++k)
        if ((double)C[(size_t)t * N_FOOT + k] >= cthr) {
          const foot_pair p = foot_load(J, t, k);
          sx += p.x1 - p.x0;
          sz += p.z1 - p.z0;
          ++m;
        }
      if (m > 0) vx = -(sx / (double)m), vz = -(sz / (double)m);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double ox = __shfl_up(vx, d), oz = __shfl_up(vz, d);
      if (lane >= d) vx = ox + vx, vz = oz + vz;
    }
    __syncthreads();                                   // (the last tile's tot has been read)
    if (lane == 63) tot[wave][0] = vx, tot[wave][1] = vz;
    __syncthreads();
    double px = carry_x, pz = carry_z;
    for (int w = 0; w < FOOT_WAVES; ++w) {
      if (w == wave) vx = px + vx, vz = pz + vz;       // off[t + 1]
      px += tot[w][0], pz += tot[w][1];
    }
    carry_x = px, carry_z = pz;
    if (t < n - 1) {
      const float* i1 = in + (size_t)(t + 1) * 3;
      const float x = i1[0], y = i1[1], z = i1[2];
      float* o1 = out + (size_t)(t + 1) * 3;
      o1[0] = (float)((double)x + vx);
      o1[1] = y;
      o1[2] = (float)((double)z + vz);
    }
  }
}

}  // namespace

extern "C" int rg_foot_skate_sums(rg_handle* h, const float* joints, const float* contact, const int* clip_off,
                                  const int* clip_off_host, int n_clips, float fps, float height, float speed, float contact_thr,
                                  float move_thr, double* sums, void* stream) {
  RG_REQUIRE(h, joints && clip_off && clip_off_host && sums, "null pointer");
  RG_REQUIRE(h, n_clips >= 1, "need at least one clip");
  const char* bad = bad_foot_clips(clip_off_host, n_clips);
  RG_REQUIRE(h, !bad, bad);
  RG_REQUIRE(h, height == height && speed == speed && contact_thr == contact_thr && move_thr == move_thr,
             "the thresholds (height, speed, contact_thr, move_thr) must be numbers");
  RG_REQUIRE(h, fps > 0.f, "fps must be positive");
  hipLaunchKernelGGL(foot_skate_kernel, dim3(n_clips), dim3(FOOT_THREADS), 0, rg_stream(stream), joints, contact, clip_off, fps,
                     height, speed, contact_thr, move_thr, sums);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_foot_plant(rg_handle* h, const float* joints, const float* contact, const float* trans_in, const int* clip_off,
                             const int* clip_off_host, int n_clips, float contact_thr, float* trans_out, void* stream) {
  RG_REQUIRE(h, joints && contact && trans_in && clip_off && clip_off_host && trans_out, "null pointer");
  RG_REQUIRE(h, n_clips >= 1, "need at least one clip");
  const char* bad = bad_foot_clips(clip_off_host, n_clips);
  RG_REQUIRE(h, !bad, bad);
  RG_REQUIRE(h, contact_thr == contact_thr, "the threshold contact_thr must be a number");
  hipLaunchKernelGGL(foot_plant_kernel, dim3(n_clips), dim3(FOOT_THREADS), 0, rg_stream(stream), joints, contact, trans_in,
                     clip_off, contact_thr, trans_out);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}
