// Baseline sequential JPEG (ITU-T T.81), 8 bit, YCbCr 4:2:0, of uint8 RGB frames on the device: what the Motion-JPEG writer of
// video.py needs.  Three entry points over the coefficient array [frame][MCU][Y00, Y01, Y10, Y11, Cb, Cr][64] int16 (zig-zag):
//   rg_jpeg_dct_quant    : one workgroup per MCU (16 x 16 pixels, one per thread) -- JFIF BT.601 in fp32, the 2 x 2 chroma mean, six
//                          orthonormal 8 x 8 DCTs as two 1-D passes through LDS, sign(v) floor(|v| / q + 0.5)
//   rg_jpeg_entropy_count: one wave per restart interval (one MCU row), one lane per block, 64 blocks at a time -- every lane
//                          counts the bits of its block's Huffman codes, a wave scan gives the block its bit position, the lanes put
//                          their codes into an LDS bit buffer with 32-bit LDS atomic ORs, then the wave walks the buffer's bytes
//                          (ballot + popcount place each byte behind the stuffed zeros of the 0xFF bytes in front of it)
//   rg_jpeg_entropy_write: the same coder, storing the bytes at the interval's final offset, and RSTm behind it
// The count launch stores nothing but the lengths; an exclusive scan of them (the caller's) makes the write launch exact: no
// interval is ever truncated, whatever the picture.
#include "rg_common.h"

namespace {

constexpr int WAVE = 64;
constexpr int BLOCKS_PER_MCU = 6;
// a block's codes at their longest: a DC difference (9 + 11 bits) and 63 AC values of a 16-bit code + 10 bits each
constexpr int MAX_BLOCK_BITS = 20 + 63 * 26;
constexpr int BUF_WORDS = (WAVE * MAX_BLOCK_BITS + 8 + 31) / 32 + 1;      // 64 blocks, up to 7 bits carried in, one word of slack

// zig-zag position k -> index in the 8 x 8 block, row-major (T.81 figure 5)
struct zigzag_t { unsigned char at[64]; };
constexpr zigzag_t make_zigzag() {
  zigzag_t z{};
  int r = 0, c = 0;
  for (int k = 0; k < 64; ++k) {
    z.at[k] = (unsigned char)(r * 8 + c);
    if ((r + c) % 2 == 0) {                      // moving up and to the right
      if (c == 7) ++r; else if (r == 0) ++c; else { --r; ++c; }
    } else {                                     // moving down and to the left
      if (r == 7) ++c; else if (c == 0) ++r; else { ++r; --c; }
    }
  }
  return z;
}
__constant__ zigzag_t ZIGZAG = make_zigzag();

// 0.5 cos(m pi / 16), m = 0 .. 31: the orthonormal DCT-II matrix is C[k][n] = HALF_COS[(2n + 1) k mod 32] for k > 0 and
// C[0][n] = 1 / sqrt(8) = HALF_COS[4]; each entry is the float nearest to the real value
struct halfcos_t { float at[32]; };
constexpr halfcos_t make_halfcos() {
  constexpr double c[9] = {1.0, 0.98078528040323044913, 0.92387953251128675613, 0.83146961230254523708, 0.70710678118654752440,
                           0.55557023301960222474, 0.38268343236508977173, 0.19509032201612826785, 0.0};
  halfcos_t t{};
  for (int m = 0; m < 32; ++m) {
    const int f = m & 15;                                        // cos((16 + f) pi / 16) = -cos(f pi / 16)
    const double v = f <= 8 ? c[f] : -c[16 - f];
    t.at[m] = (float)(0.5 * (m < 16 ? v : -v));
  }
  return t;
}
__constant__ halfcos_t HALF_COS = make_halfcos();

// The Annex K.3 tables as (size << 16 | code) per symbol, 0 where a symbol has no code: [DC luma, DC chroma][16] and
// [AC luma, AC chroma][256], the codes generated from BITS and HUFFVAL as Annex C does
struct huff_t { unsigned dc[2][16]; unsigned ac[2][256]; };
constexpr void huff_fill(unsigned* out, const unsigned char* bits, const unsigned char* vals) {
  unsigned code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = ((unsigned)len << 16) | code++;
    code <<= 1;
  }
}
constexpr huff_t make_huff() {
  constexpr unsigned char dc_l_bits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
  constexpr unsigned char dc_c_bits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
  constexpr unsigned char dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
  constexpr unsigned char ac_l_bits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
  constexpr unsigned char ac_l_vals[162] = {
      0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
      0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
      0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
      0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
      0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
      0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
      0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
      0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
  constexpr unsigned char ac_c_bits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
  constexpr unsigned char ac_c_vals[162] = {
      0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
      0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
      0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
      0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
      0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
      0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
      0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
      0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
  huff_t h{};
  huff_fill(h.dc[0], dc_l_bits, dc_vals);
  huff_fill(h.dc[1], dc_c_bits, dc_vals);
  huff_fill(h.ac[0], ac_l_bits, ac_l_vals);
  huff_fill(h.ac[1], ac_c_bits, ac_c_vals);
  return h;
}
__constant__ huff_t HUFF = make_huff();

// ---------------------------------------------------------------------------------------------------- rg_jpeg_dct_quant
// Workgroup (frame, MCU row, MCU column), thread (y, x) of the MCU's 16 x 16 pixels; a pixel past the frame's edge is the edge's.
__global__ void __launch_bounds__(256) jpeg_dct_quant_kernel(const unsigned char* __restrict__ frames, int height, int width, int pitch,
                                                             int mcu_rows, int mcu_cols, const unsigned char* __restrict__ q_luma,
                                                             const unsigned char* __restrict__ q_chroma, int16_t* __restrict__ coef) {
  __shared__ float px[BLOCKS_PER_MCU][64];        // the six blocks' samples, row-major; then their coefficients
  __shared__ float tmp[BLOCKS_PER_MCU][64];
  __shared__ float cbf[256], crf[256];            // chroma at full resolution
  __shared__ float cm[8][8];                      // the DCT matrix C[k][n]
  const int tid = threadIdx.x;
  const int64_t mcu = blockIdx.x;                 // over frames x MCU rows x MCU columns
  const int mc = (int)(mcu % mcu_cols), mr = (int)(mcu / mcu_cols % mcu_rows);
  const int64_t frame = mcu / mcu_cols / mcu_rows;
  if (tid < 64) {
    const int k = tid >> 3, n = tid & 7;
    cm[k][n] = HALF_COS.at[k == 0 ? 4 : ((2 * n + 1) * k) & 31];
  }
  const int ly = tid >> 4, lx = tid & 15;
  const int y = min(mr * 16 + ly, height - 1), x = min(mc * 16 + lx, width - 1);
  const unsigned char* p = frames + ((frame * height + y) * (int64_t)pitch + x) * 3;
  const float r = (float)p[0], g = (float)p[1], b = (float)p[2];
  px[(ly >> 3) * 2 + (lx >> 3)][(ly & 7) * 8 + (lx & 7)] = fmaf(0.299f, r, fmaf(0.587f, g, 0.114f * b)) - 128.0f;
  cbf[tid] = fmaf(-0.168736f, r, fmaf(-0.331264f, g, 0.5f * b));
  crf[tid] = fmaf(0.5f, r, fmaf(-0.418688f, g, -0.081312f * b));
  __syncthreads();
  if (tid < 128) {                                // the mean of each 2 x 2 block, rows first
    const float* src = tid < 64 ? cbf : crf;
    const int i = tid & 63, o = (i >> 3) * 32 + (i & 7) * 2;
    px[4 + (tid >> 6)][i] = ((src[o] + src[o + 1]) + (src[o + 16] + src[o + 17])) * 0.25f;
  }
  __syncthreads();
  for (int i = tid; i < BLOCKS_PER_MCU * 64; i += 256) {      // along the rows: tmp[b][y][u] = sum over x of C[u][x] px[b][y][x]
    const int blk = i >> 6, yy = (i >> 3) & 7, u = i & 7;
    float acc = 0.0f;
#pragma unroll
    for (int n = 0; n < 8; ++n) acc = fmaf(cm[u][n], px[blk][yy * 8 + n], acc);
    tmp[blk][yy * 8 + u] = acc;
  }
  __syncthreads();
  for (int i = tid; i < BLOCKS_PER_MCU * 64; i += 256) {      // down the columns: px[b][v][u] = sum over y of C[v][y] tmp[b][y][u]
    const int blk = i >> 6, v = (i >> 3) & 7, u = i & 7;
    float acc = 0.0f;
#pragma unroll
    for (int n = 0; n < 8; ++n) acc = fmaf(cm[v][n], tmp[blk][n * 8 + u], acc);
    px[blk][v * 8 + u] = acc;
  }
  __syncthreads();
  int16_t* dst = coef + mcu * (BLOCKS_PER_MCU * 64);
  for (int i = tid; i < BLOCKS_PER_MCU * 64; i += 256) {
    const int blk = i >> 6, k = i & 63;
    const float v = px[blk][ZIGZAG.at[k]];
    const float q = (float)(blk < 4 ? q_luma : q_chroma)[k];
    const float m = fminf(floorf(fabsf(v) / q + 0.5f), k == 0 ? 1024.0f : 1023.0f);    // (8-bit samples never reach the limits)
    dst[i] = (int16_t)(v < 0.0f ? -m : m);
  }
}

// ---------------------------------------------------------------------------------------------------- the entropy coder
__device__ __forceinline__ int bit_size(int v) { return 32 - __clz(v < 0 ? -v : v); }        // T.81 table F.1 / F.2: 0 for 0

// `n` bits (n <= 26, the value's upper bits zero) at bit position `pos` of the big-endian bit buffer
__device__ __forceinline__ void put_bits(unsigned* buf, int pos, unsigned value, int n) {
  const unsigned long long x = (unsigned long long)value << (64 - (pos & 31) - n);
  const unsigned hi = (unsigned)(x >> 32), lo = (unsigned)x;
  atomicOr(&buf[pos >> 5], hi);
  if (lo) atomicOr(&buf[(pos >> 5) + 1], lo);
}

// One block's codes: counted (buf == nullptr) or put at bit position pos.  c: the block's 64 coefficients; pred: the DC value
// the difference is taken from; dc / ac: the component's tables.  Values beyond the baseline's range (AC +-1023, DC difference
// +-2047) are clamped to it, so a block never takes more than MAX_BLOCK_BITS.  -> the position behind the block.
__device__ __forceinline__ int code_block(const int16_t* __restrict__ c, int pred, const unsigned* dc, const unsigned* ac, unsigned* buf, int pos) {
  const int diff = max(-2047, min(2047, (int)c[0] - pred));
  int s = bit_size(diff);
  unsigned e = dc[s];
  if (buf) put_bits(buf, pos, ((e & 0xffffu) << s) | (unsigned)((diff < 0 ? diff - 1 : diff) & ((1 << s) - 1)), (int)(e >> 16) + s);
  pos += (int)(e >> 16) + s;
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = max(-1023, min(1023, (int)c[k]));
    if (v == 0) { ++run; continue; }
    for (; run >= 16; run -= 16) {               // ZRL
      e = ac[0xf0];
      if (buf) put_bits(buf, pos, e & 0xffffu, (int)(e >> 16));
      pos += (int)(e >> 16);
    }
    s = bit_size(v);
    e = ac[(run << 4) | s];
    if (buf) put_bits(buf, pos, ((e & 0xffffu) << s) | (unsigned)((v < 0 ? v - 1 : v) & ((1 << s) - 1)), (int)(e >> 16) + s);
    pos += (int)(e >> 16) + s;
    run = 0;
  }
  if (run) {                                     // EOB
    e = ac[0];
    if (buf) put_bits(buf, pos, e & 0xffffu, (int)(e >> 16));
    pos += (int)(e >> 16);
  }
  return pos;
}

// One wave per restart interval = MCU row `row` of frame `frame`.  WRITE: the stuffed bytes go to out + offsets[interval], RSTm
// behind them unless the row is the frame's last, nothing at or beyond out + capacity; else lengths[interval] = their count.
template <bool WRITE>
__global__ void __launch_bounds__(WAVE) jpeg_entropy_kernel(const int16_t* __restrict__ coef, int mcu_rows, int mcu_cols,
                                                            int* __restrict__ lengths, const int64_t* __restrict__ offsets,
                                                            unsigned char* __restrict__ out, int64_t capacity) {
  __shared__ unsigned buf[BUF_WORDS];
  __shared__ unsigned dc_tab[2][16], ac_tab[2][256];
  const int lane = threadIdx.x;
  const int64_t interval = blockIdx.x;
  const int row = (int)(interval % mcu_rows);
  for (int i = lane; i < 32; i += WAVE) dc_tab[i >> 4][i & 15] = HUFF.dc[i >> 4][i & 15];
  for (int i = lane; i < 512; i += WAVE) ac_tab[i >> 8][i & 255] = HUFF.ac[i >> 8][i & 255];
  const int16_t* base = coef + interval * mcu_cols * (BLOCKS_PER_MCU * 64);
  const int n_blocks = mcu_cols * BLOCKS_PER_MCU;
  const unsigned long long below = (1ull << lane) - 1;
  const int64_t start = WRITE ? offsets[interval] : 0;
  int64_t written = 0;                           // bytes of the interval so far (wave-uniform)
  unsigned carry = 0;                            // the bits (carry_n < 8 of them) behind the last whole byte
  int carry_n = 0;
  for (int b0 = 0;; b0 += WAVE) {
    const bool last = b0 + WAVE >= n_blocks;     // (the pass that also pads the interval's last byte)
    for (int i = lane; i < BUF_WORDS; i += WAVE) buf[i] = 0;
    __syncthreads();
    const int blk = b0 + lane;
    const bool have = blk < n_blocks;
    const int16_t* c = base + (int64_t)blk * 64;
    int comp = 0, pred = 0;
    if (have) {                                  // the block in front of it of the same component, within the interval
      const int m = blk / BLOCKS_PER_MCU, j = blk % BLOCKS_PER_MCU;
      comp = j < 4 ? 0 : 1;
      if (j >= 1 && j <= 3) pred = c[-64];
      else if (m > 0) pred = c[j == 0 ? -3 * 64 : -BLOCKS_PER_MCU * 64];
    }
    const int bits = have ? code_block(c, pred, dc_tab[comp], ac_tab[comp], nullptr, 0) : 0;
    int incl = bits;                             // inclusive scan over the lanes
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const int t = __shfl_up(incl, d, WAVE);
      if (lane >= d) incl += t;
    }
    int total = carry_n + __shfl(incl, WAVE - 1, WAVE);
    if (lane == 0 && carry_n) atomicOr(&buf[0], carry << (32 - carry_n));
    if (have) code_block(c, pred, dc_tab[comp], ac_tab[comp], buf, carry_n + incl - bits);
    if (last && (total & 7)) {                   // the interval's last byte is filled with 1 bits
      const int pad = 8 - (total & 7);
      if (lane == 0) put_bits(buf, total, (1u << pad) - 1, pad);
      total += pad;
    }
    __syncthreads();
    const int n_bytes = total >> 3;
    for (int j0 = 0; j0 < n_bytes; j0 += WAVE) {
      const int j = j0 + lane;
      const bool valid = j < n_bytes;
      const unsigned byte = valid ? (buf[j >> 2] >> (24 - 8 * (j & 3))) & 0xffu : 0u;
      const bool ff = valid && byte == 0xffu;
      const unsigned long long mask = __ballot(ff);
      if (WRITE && valid) {
        const int64_t at = start + written + lane + __popcll(mask & below);
        if (at < capacity) out[at] = (unsigned char)byte;
        if (ff && at + 1 < capacity) out[at + 1] = 0;
      }
      written += min(WAVE, n_bytes - j0) + __popcll(mask);
    }
    carry_n = total & 7;
    carry = carry_n ? (buf[n_bytes >> 2] >> (32 - 8 * (n_bytes & 3) - carry_n)) & ((1u << carry_n) - 1) : 0u;
    __syncthreads();
    if (last) break;
  }
  const bool marker = row + 1 < mcu_rows;
  if (WRITE) {
    if (marker && lane < 2) {
      const int64_t at = start + written + lane;
      if (at < capacity) out[at] = lane == 0 ? 0xffu : (unsigned char)(0xd0 + (row & 7));
    }
  } else if (lane == 0) {
    lengths[interval] = (int)(written + (marker ? 2 : 0));
  }
}

int jpeg_check(rg_handle* h, const int16_t* coef, int n_frames, int mcu_rows, int mcu_cols) {
  RG_REQUIRE(h, coef, "null pointer");
  RG_REQUIRE(h, n_frames >= 1 && mcu_rows >= 1 && mcu_cols >= 1, "need at least one frame and one MCU");
  RG_REQUIRE(h, mcu_rows <= RG_JPEG_MAX_MCUS && mcu_cols <= RG_JPEG_MAX_MCUS, "more than 4096 MCUs a side: no baseline JPEG has more than 65535 pixels a side");
  RG_REQUIRE(h, (int64_t)n_frames * mcu_rows < (int64_t)1 << 31, "too many restart intervals in one call");
  return RG_OK;
}

}  // namespace

extern "C" int rg_jpeg_dct_quant(rg_handle* h, const unsigned char* frames, int n_frames, int height, int width, int pitch,
                                 const unsigned char* q_luma, const unsigned char* q_chroma, int16_t* coef, void* stream) {
  RG_REQUIRE(h, frames && q_luma && q_chroma && coef, "null pointer");
  RG_REQUIRE(h, n_frames >= 1 && height >= 1 && width >= 1, "need at least one frame of at least one pixel");
  RG_REQUIRE(h, height <= 65535 && width <= 65535, "a frame of more than 65535 pixels a side is no baseline JPEG");
  RG_REQUIRE(h, pitch >= width, "the row pitch (in pixels) must be at least the width");
  const int mcu_rows = (height + RG_JPEG_MCU - 1) / RG_JPEG_MCU, mcu_cols = (width + RG_JPEG_MCU - 1) / RG_JPEG_MCU;
  const int64_t mcus = (int64_t)n_frames * mcu_rows * mcu_cols;
  RG_REQUIRE(h, mcus < (int64_t)1 << 31, "too many MCUs in one call");
  hipLaunchKernelGGL(jpeg_dct_quant_kernel, dim3((unsigned)mcus), dim3(256), 0, rg_stream(stream), frames, height, width, pitch, mcu_rows,
                     mcu_cols, q_luma, q_chroma, coef);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_jpeg_entropy_count(rg_handle* h, const int16_t* coef, int n_frames, int mcu_rows, int mcu_cols, int* lengths, void* stream) {
  const int rc = jpeg_check(h, coef, n_frames, mcu_rows, mcu_cols);
  if (rc != RG_OK) return rc;
  RG_REQUIRE(h, lengths, "null pointer");
  hipLaunchKernelGGL(jpeg_entropy_kernel<false>, dim3((unsigned)(n_frames * mcu_rows)), dim3(WAVE), 0, rg_stream(stream), coef, mcu_rows,
                     mcu_cols, lengths, (const int64_t*)nullptr, (unsigned char*)nullptr, (int64_t)0);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}

extern "C" int rg_jpeg_entropy_write(rg_handle* h, const int16_t* coef, int n_frames, int mcu_rows, int mcu_cols, const int64_t* offsets,
                                     unsigned char* out, int64_t capacity, void* stream) {
  const int rc = jpeg_check(h, coef, n_frames, mcu_rows, mcu_cols);
  if (rc != RG_OK) return rc;
  RG_REQUIRE(h, offsets && out, "null pointer");
  RG_REQUIRE(h, capacity >= 1, "the byte buffer holds nothing");
  hipLaunchKernelGGL(jpeg_entropy_kernel<true>, dim3((unsigned)(n_frames * mcu_rows)), dim3(WAVE), 0, rg_stream(stream), coef, mcu_rows,
                     mcu_cols, (int*)nullptr, offsets, out, capacity);
  RG_CHECK_LAUNCH(h);
  return RG_OK;
}
