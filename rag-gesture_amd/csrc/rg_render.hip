// SMPL-X clip rendering: what mogen/utils/visualization.py:339-440 draws per frame (one mesh of one colour over a checkerboard
// floor, pyrender's PerspectiveCamera), as a software rasteriser over a chunk of frames.
//   rg_render_project : per frame and vertex the snapped screen position (int32, 8 sub-pixel bits), the view depth and the
//                       smooth normal (area-weighted face normals gathered through a vertex -> faces CSR: a fixed order)
//   rg_render_bin     : per frame and face the range of 32 x 32 tiles it can cover, or "dropped" (behind znear, back face, off
//                       screen), one packed word
//   rg_render_raster  : one workgroup per tile and frame: it scans the frame's packed words (84 KB for 20 908 faces), rasterises
//                       the faces that reach its tile with 64-bit integer edge functions and the top-left rule into a 64-bit
//                       (1 / depth, ~face) maximum per pixel in LDS, then shades, intersects the floor and writes the pixels
// The definitions are in include/rg_gesture.h; the shading is the project's own (DESIGN.md "Rendering").
#include "rg_common.h"

namespace {

constexpr int T = RG_RENDER_TILE;
constexpr int SUB = RG_RENDER_SUBPIXEL_BITS;
constexpr int ONE = 1 << SUB;                   // one pixel in fixed point
constexpr int HALF = ONE / 2;
constexpr int THREADS = 256;
constexpr float ZNEAR = 0.05f;
constexpr float TAN_HALF_FOV = 0.57735026918962576451f;   // tan(pi / 6)
constexpr float AMBIENT = 0.35f;
constexpr float FLOOR_HALF = 6.0f;

typedef long long i64;
typedef unsigned long long u64;

__device__ __forceinline__ int snap(float px) {
  const float lim = (float)RG_RENDER_COORD_MAX;
  const float v = floorf(fminf(fmaxf(fmaf(px, (float)ONE, 0.5f), -lim), lim));
  return (int)v;
}

__device__ __forceinline__ bool index_ok(int i0, int i1, int i2, int n) {
  return ((unsigned)i0 < (unsigned)n) & ((unsigned)i1 < (unsigned)n) & ((unsigned)i2 < (unsigned)n);
}

__global__ void __launch_bounds__(THREADS) render_project_kernel(rg_render_project_args a) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= a.frames * a.n_verts) return;
  const int f = i / a.n_verts, v = i - f * a.n_verts;
  const float* vf = a.verts + (size_t)f * a.n_verts * 3;
  const float dx = vf[3 * v] - a.cam[3], dy = vf[3 * v + 1] - a.cam[7], dz = vf[3 * v + 2] - a.cam[11];
  const float xc = a.cam[0] * dx + a.cam[4] * dy + a.cam[8] * dz;
  const float yc = a.cam[1] * dx + a.cam[5] * dy + a.cam[9] * dz;
  const float z = -(a.cam[2] * dx + a.cam[6] * dy + a.cam[10] * dz);
  int sx = 0, sy = 0;
  if (z >= ZNEAR) {
    const float aspect = (float)a.width / (float)a.height;
    sx = snap((xc / (z * (aspect * TAN_HALF_FOV)) + 1.0f) * (0.5f * (float)a.width));
    sy = snap((1.0f - yc / (z * TAN_HALF_FOV)) * (0.5f * (float)a.height));
  }
  a.screen[2 * (size_t)i] = sx, a.screen[2 * (size_t)i + 1] = sy;
  a.depth[i] = z;

  float nx = 0.f, ny = 0.f, nz = 0.f;
  const int k1 = a.csr_off[v + 1];
  for (int k = a.csr_off[v]; k < k1; ++k) {
    const int fi = a.csr_face[k];
    if ((unsigned)fi >= (unsigned)a.n_faces) continue;
    const int i0 = a.faces[3 * fi], i1 = a.faces[3 * fi + 1], i2 = a.faces[3 * fi + 2];
    if (!index_ok(i0, i1, i2, a.n_verts)) continue;
    const float* p0 = vf + 3 * i0;
    const float* p1 = vf + 3 * i1;
    const float* p2 = vf + 3 * i2;
    const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
    const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
    nx += ay * bz - az * by;
    ny += az * bx - ax * bz;
    nz += ax * by - ay * bx;
  }
  const float len = sqrtf(nx * nx + ny * ny + nz * nz);
  if (len > 0.f) nx /= len, ny /= len, nz /= len;
  float* n = a.normal + 3 * (size_t)i;
  n[0] = nx, n[1] = ny, n[2] = nz;
}

// SWAP: a front face is counter-clockwise as the viewer sees it, i.e. its doubled area is NEGATIVE in the y-down screen
// coordinates.  The coverage code works on (v0, v2, v1), whose area is positive and whose edge functions are >= 0 inside.

// first / last pixel whose centre lies in [lo, hi] (fixed point)
__device__ __forceinline__ int first_px(int lo) { return (lo - HALF + ONE - 1) >> SUB; }
__device__ __forceinline__ int last_px(int hi) { return (hi - HALF) >> SUB; }

__global__ void __launch_bounds__(THREADS) render_bin_kernel(rg_render_bin_args a) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= a.frames * a.n_faces) return;
  const int f = i / a.n_faces, fi = i - f * a.n_faces;
  unsigned out = RG_RENDER_BOX_NONE;
  const int i0 = a.faces[3 * fi], i1 = a.faces[3 * fi + 2], i2 = a.faces[3 * fi + 1];      // (v0, v2, v1): see SWAP
  if (index_ok(i0, i1, i2, a.n_verts)) {
    const int* s = a.screen + (size_t)f * a.n_verts * 2;
    const float* d = a.depth + (size_t)f * a.n_verts;
    const bool near_ok = d[i0] >= ZNEAR && d[i1] >= ZNEAR && d[i2] >= ZNEAR;
    const int x0 = s[2 * i0], y0 = s[2 * i0 + 1], x1 = s[2 * i1], y1 = s[2 * i1 + 1], x2 = s[2 * i2], y2 = s[2 * i2 + 1];
    const i64 area = (i64)(x1 - x0) * (y2 - y0) - (i64)(y1 - y0) * (x2 - x0);
    const int px0 = max(first_px(min(x0, min(x1, x2))), 0), px1 = min(last_px(max(x0, max(x1, x2))), a.width - 1);
    const int py0 = max(first_px(min(y0, min(y1, y2))), 0), py1 = min(last_px(max(y0, max(y1, y2))), a.height - 1);
    if (near_ok && area > 0 && px0 <= px1 && py0 <= py1)
      out = (unsigned)(px0 / T) | (unsigned)(px1 / T) << 8 | (unsigned)(py0 / T) << 16 | (unsigned)(py1 / T) << 24;
  }
  a.box[i] = out;
}

struct FaceSetup {
  i64 e0, e1, e2;            // edge functions at the pixel centre (cx, cy): the weights of v0, v1, v2 times the area
  i64 sx0, sx1, sx2;         // their steps per pixel in x
  i64 sy0, sy1, sy2;         // ... and in y
  i64 area;
  int b0, b1, b2;            // 0 for a top or left edge, -1 otherwise
};

__device__ __forceinline__ int edge_bias(int dx, int dy) { return ((dy == 0 && dx > 0) || dy < 0) ? 0 : -1; }

__device__ __forceinline__ FaceSetup face_setup(int x0, int y0, int x1, int y1, int x2, int y2, int cx, int cy) {
  FaceSetup s;
  s.e0 = (i64)(x2 - x1) * (cy - y1) - (i64)(y2 - y1) * (cx - x1);
  s.e1 = (i64)(x0 - x2) * (cy - y2) - (i64)(y0 - y2) * (cx - x2);
  s.e2 = (i64)(x1 - x0) * (cy - y0) - (i64)(y1 - y0) * (cx - x0);
  s.sx0 = -(i64)(y2 - y1) * ONE, s.sx1 = -(i64)(y0 - y2) * ONE, s.sx2 = -(i64)(y1 - y0) * ONE;
  s.sy0 = (i64)(x2 - x1) * ONE, s.sy1 = (i64)(x0 - x2) * ONE, s.sy2 = (i64)(x1 - x0) * ONE;
  s.area = (i64)(x1 - x0) * (y2 - y0) - (i64)(y1 - y0) * (x2 - x0);
  s.b0 = edge_bias(x2 - x1, y2 - y1), s.b1 = edge_bias(x0 - x2, y0 - y2), s.b2 = edge_bias(x1 - x0, y1 - y0);
  return s;
}

__global__ void __launch_bounds__(THREADS) render_raster_kernel(rg_render_raster_args a, int tiles_x) {
  __shared__ u64 key[T * T];
  const int tid = threadIdx.x;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x, frame = blockIdx.y;
  for (int i = tid; i < T * T; i += THREADS) key[i] = 0;
  __syncthreads();
  const int* scr = a.screen + (size_t)frame * a.n_verts * 2;
  const float* dep = a.depth + (size_t)frame * a.n_verts;
  const int tile_x0 = tx * T, tile_y0 = ty * T;
  const int tile_x1 = min(tile_x0 + T, a.width) - 1, tile_y1 = min(tile_y0 + T, a.height) - 1;

  if (!a.active || a.active[frame]) {
    const unsigned* box = a.box + (size_t)frame * a.n_faces;
    for (int f = tid; f < a.n_faces; f += THREADS) {
      const unsigned b = box[f];
      const int bx0 = b & 255, bx1 = (b >> 8) & 255, by0 = (b >> 16) & 255, by1 = b >> 24;
      if (tx < bx0 || tx > bx1 || ty < by0 || ty > by1) continue;
      const int i0 = a.faces[3 * f], i1 = a.faces[3 * f + 2], i2 = a.faces[3 * f + 1];     // (in range: rg_render_bin checked)
      const int x0 = scr[2 * i0], y0 = scr[2 * i0 + 1], x1 = scr[2 * i1], y1 = scr[2 * i1 + 1], x2 = scr[2 * i2], y2 = scr[2 * i2 + 1];
      const int px0 = max(first_px(min(x0, min(x1, x2))), tile_x0), px1 = min(last_px(max(x0, max(x1, x2))), tile_x1);
      const int py0 = max(first_px(min(y0, min(y1, y2))), tile_y0), py1 = min(last_px(max(y0, max(y1, y2))), tile_y1);
      if (px0 > px1 || py0 > py1) continue;
      const FaceSetup s = face_setup(x0, y0, x1, y1, x2, y2, px0 * ONE + HALF, py0 * ONE + HALF);
      const float inv_area = 1.0f / (float)s.area;
      const float iz0 = 1.0f / dep[i0], iz1 = 1.0f / dep[i1], iz2 = 1.0f / dep[i2];
      const unsigned low = 0xffffffffu - (unsigned)f;
      i64 r0 = s.e0, r1 = s.e1, r2 = s.e2;
      for (int py = py0; py <= py1; ++py) {                     // (at most 32 x 32 steps: the tile)
        i64 e0 = r0, e1 = r1, e2 = r2;
        for (int px = px0; px <= px1; ++px) {
          if (((e0 + s.b0) | (e1 + s.b1) | (e2 + s.b2)) >= 0) {
            const float w = (float)e0 * inv_area * iz0 + (float)e1 * inv_area * iz1 + (float)e2 * inv_area * iz2;
            const u64 k = ((u64)__float_as_uint(w) << 32) | low;
            atomicMax(&key[(py - tile_y0) * T + (px - tile_x0)], k);
          }
          e0 += s.sx0, e1 += s.sx1, e2 += s.sx2;
        }
        r0 += s.sy0, r1 += s.sy1, r2 += s.sy2;
      }
    }
  }
  __syncthreads();

  const float aspect = (float)a.width / (float)a.height;
  const float lx = a.cam[2], ly = a.cam[6], lz = a.cam[10];
  for (int i = tid; i < T * T; i += THREADS) {
    const int px = tile_x0 + (i % T), py = tile_y0 + (i / T);
    if (px > tile_x1 || py > tile_y1) continue;
    const u64 k = key[i];
    int face = -1;
    float w = 0.f, r = 191.f, g = 191.f, bl = 191.f;
    if (k) {
      face = (int)(0xffffffffu - (unsigned)k);
      w = __uint_as_float((unsigned)(k >> 32));
    }
    bool floor_shows = false;
    if (a.draw_floor) {
      const float xn = ((float)px + 0.5f) / (0.5f * (float)a.width) - 1.0f;
      const float yn = 1.0f - ((float)py + 0.5f) / (0.5f * (float)a.height);
      const float cx = xn * (aspect * TAN_HALF_FOV), cy = yn * TAN_HALF_FOV;
      const float wx = a.cam[0] * cx + a.cam[1] * cy - a.cam[2];
      const float wy = a.cam[4] * cx + a.cam[5] * cy - a.cam[6];
      const float wz = a.cam[8] * cx + a.cam[9] * cy - a.cam[10];
      if (wy != 0.f) {
        const float s = (a.floor_y - a.cam[7]) / wy;
        const float hx = a.cam[3] + s * wx, hz = a.cam[11] + s * wz;
        if (s > 0.f && hx >= -FLOOR_HALF && hx < FLOOR_HALF && hz >= -FLOOR_HALF && hz < FLOOR_HALF && (face < 0 || 1.0f / s > w)) {
          floor_shows = true;
          const int parity = ((int)floorf(hx + FLOOR_HALF) + (int)floorf(hz + FLOOR_HALF)) & 1;
          const float c = parity ? 120.f : 170.f;
          const float v = floorf((AMBIENT + (1.f - AMBIENT) * fmaxf(0.f, ly)) * c + 0.5f);
          r = g = bl = v;
          face = -1;
        }
      }
    }
    if (face >= 0 && !floor_shows) {
      const int i0 = a.faces[3 * face], i1 = a.faces[3 * face + 2], i2 = a.faces[3 * face + 1];
      const FaceSetup s = face_setup(scr[2 * i0], scr[2 * i0 + 1], scr[2 * i1], scr[2 * i1 + 1], scr[2 * i2], scr[2 * i2 + 1],
                                     px * ONE + HALF, py * ONE + HALF);
      const float inv_area = 1.0f / (float)s.area;
      const float b0 = (float)s.e0 * inv_area, b1 = (float)s.e1 * inv_area, b2 = (float)s.e2 * inv_area;
      const float* n0 = a.normal + ((size_t)frame * a.n_verts + i0) * 3;
      const float* n1 = a.normal + ((size_t)frame * a.n_verts + i1) * 3;
      const float* n2 = a.normal + ((size_t)frame * a.n_verts + i2) * 3;
      const float nx = b0 * n0[0] + b1 * n1[0] + b2 * n2[0];
      const float ny = b0 * n0[1] + b1 * n1[1] + b2 * n2[1];
      const float nz = b0 * n0[2] + b1 * n1[2] + b2 * n2[2];
      const float len = sqrtf(nx * nx + ny * ny + nz * nz);
      const float ndl = len > 0.f ? fmaxf(0.f, (nx * lx + ny * ly + nz * lz) / len) : 0.f;
      const float shade = AMBIENT + (1.f - AMBIENT) * ndl;
      r = fminf(floorf(shade * a.color[0] + 0.5f), 255.f);
      g = fminf(floorf(shade * a.color[1] + 0.5f), 255.f);
      bl = fminf(floorf(shade * a.color[2] + 0.5f), 255.f);
    }
    unsigned char* o = a.out + (((size_t)frame * a.height + py) * a.pitch + a.col + px) * 3;
    o[0] = (unsigned char)r, o[1] = (unsigned char)g, o[2] = (unsigned char)bl;
    if (a.face_id) a.face_id[((size_t)frame * a.height + py) * a.width + px] = face;
  }
}

bool finite16(const float* m) {
  for (int i = 0; i < 16; ++i)
    if (!(m[i] == m[i]) || m[i] > 3.0e38f || m[i] < -3.0e38f) return false;
  return true;
}

constexpr int MAX_DIM = 255 * T;

}  // namespace

extern "C" int rg_render_project(rg_handle* h, const rg_render_project_args* args_host, void* stream) {
  RG_REQUIRE(h, args_host, "null argument block");
  const rg_render_project_args& a = *args_host;
  RG_REQUIRE(h, a.verts && a.faces && a.csr_off && a.csr_face && a.screen && a.depth && a.normal, "null pointer");
  RG_REQUIRE(h, a.frames >= 1 && a.n_verts >= 1 && a.n_faces >= 1, "need frames, n_verts, n_faces >= 1");
  RG_REQUIRE(h, (int64_t)a.frames * a.n_verts < (int64_t)1 << 29, "frames * n_verts must stay below 2^29");
  RG_REQUIRE(h, a.width >= 1 && a.height >= 1 && a.width <= MAX_DIM && a.height <= MAX_DIM, "width / height must lie in [1, 8160]");
  RG_REQUIRE(h, finite16(a.cam), "camera pose holds non-finite values");
  const int total = a.frames * a.n_verts;
  hipLaunchKernelGGL(render_project_kernel, dim3((total + THREADS - 1) / THREADS), dim3(THREADS), 0, rg_stream(stream), a);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_render_bin(rg_handle* h, const rg_render_bin_args* args_host, void* stream) {
  RG_REQUIRE(h, args_host, "null argument block");
  const rg_render_bin_args& a = *args_host;
  RG_REQUIRE(h, a.screen && a.depth && a.faces && a.box, "null pointer");
  RG_REQUIRE(h, a.frames >= 1 && a.n_verts >= 1 && a.n_faces >= 1, "need frames, n_verts, n_faces >= 1");
  RG_REQUIRE(h, (int64_t)a.frames * a.n_verts < (int64_t)1 << 29 && (int64_t)a.frames * a.n_faces < (int64_t)1 << 29,
             "frames * n_verts and frames * n_faces must stay below 2^29");
  RG_REQUIRE(h, a.width >= 1 && a.height >= 1 && a.width <= MAX_DIM && a.height <= MAX_DIM, "width / height must lie in [1, 8160]");
  const int total = a.frames * a.n_faces;
  hipLaunchKernelGGL(render_bin_kernel, dim3((total + THREADS - 1) / THREADS), dim3(THREADS), 0, rg_stream(stream), a);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_render_raster(rg_handle* h, const rg_render_raster_args* args_host, void* stream) {
  RG_REQUIRE(h, args_host, "null argument block");
  const rg_render_raster_args& a = *args_host;
  RG_REQUIRE(h, a.screen && a.depth && a.normal && a.faces && a.box && a.out, "null pointer");
  RG_REQUIRE(h, a.frames >= 1 && a.frames <= 65535 && a.n_verts >= 1 && a.n_faces >= 1, "need 1 <= frames <= 65535, n_verts, n_faces >= 1");
  RG_REQUIRE(h, (int64_t)a.frames * a.n_verts < (int64_t)1 << 29 && (int64_t)a.frames * a.n_faces < (int64_t)1 << 29,
             "frames * n_verts and frames * n_faces must stay below 2^29");
  RG_REQUIRE(h, a.width >= 1 && a.height >= 1 && a.width <= MAX_DIM && a.height <= MAX_DIM, "width / height must lie in [1, 8160]");
  RG_REQUIRE(h, a.col >= 0 && a.pitch >= 1 && (int64_t)a.col + a.width <= a.pitch, "the panel [col, col + width) must fit into pitch");
  RG_REQUIRE(h, finite16(a.cam) && a.floor_y == a.floor_y, "camera pose or floor_y holds non-finite values");
  for (int c = 0; c < 3; ++c) RG_REQUIRE(h, a.color[c] >= 0.f && a.color[c] <= 255.f, "color must lie in [0, 255]");
  const int tiles_x = (a.width + T - 1) / T, tiles_y = (a.height + T - 1) / T;
  hipLaunchKernelGGL(render_raster_kernel, dim3(tiles_x * tiles_y, a.frames), dim3(THREADS), 0, rg_stream(stream), a, tiles_x);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}
