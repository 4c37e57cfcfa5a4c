// Baseline JPEG encoder on the device: what Pillow's `Image.save(quality=q)` writes for an RGB picture with
// default options -- sequential DCT, YCbCr 4:2:0 in one interleaved scan, the standard Huffman tables, no restart markers -- byte for
// byte, for Pillow builds on libjpeg-turbo (or libjpeg 6b; later IJG versions downsample differently).  Everything is integer.
//   restated: libjpeg's jccolor.c (rgb_ycc_convert), jcsample.c (h2v2_downsample, expand_right_edge), jcprepct.c (bottom edge),
//             jfdctint.c, jcdctmgr.c (forward_DCT's quantiser), jccoefct.c (dummy blocks), jchuff.c (encode_one_block, flush_bits).
// Nothing of a file's header is compiled in: the caller parses quantisation and Huffman tables out of a header its own Pillow wrote
// (footprints_amd.ops.jpeg_tables) and passes them as one device table; this file produces the entropy-coded scan.
// Six launches, phases separated by kernel boundaries; no workgroup waits for another:
//   blocks   one wave per MCU (16 x 16 pixels): clamped loads = edge replication, colour conversion, 2 x 2 downsample, level shift into
//            LDS; the 8-point passes over rows, then columns; quantiser; int16 coefficients in zigzag and scan order, dummy blocks
//            included; each block's AC bit count from a ballot of its non-zero coefficients
//   offsets  one workgroup per sample: DC bits from the previous block of the component, exclusive prefix sum with a carry over chunks,
//            zeroes the words the sample's bit stream will use and appends the closing one-bits
//   pack     one thread per block writes its codes at its bit offset; words that two blocks share are merged with atomicOr
//   count / place / scatter   FF bytes per 4 KiB chunk, one scan across the samples of the batch, the stuffed bytes of all samples back
//            to back in the output
#include "fp_common.h"

namespace {

struct JpegSample {         // fp_jpeg_sample
  int64_t offset;           // of the picture's first byte in the packed buffer; dense uint8 [h][w][3]
  int32_t h, w;
};

constexpr int TAB_Q = 0;            // uint32 [2][64]: quantisation tables in zigzag order (as a DQT segment holds them)
constexpr int TAB_DC = 128;         // uint32 [2][16]: code | length << 16 of a DC category
constexpr int TAB_AC = 160;         // uint32 [2][256]: code | length << 16 of a run / size symbol
constexpr int TAB_WORDS = 672;
constexpr int BLOCK_BITS = 20 + 63 * 26;    // worst case of one block: 9 + 11 DC bits, 63 times a 16-bit code with 10 value bits
constexpr int CHUNK = 4096;         // bytes of the unstuffed stream one workgroup of the stuffing kernels handles (256 threads x 16)
constexpr int LSTRIDE = 9;          // LDS row stride of an 8 x 8 block: the row pass reads without bank conflicts
constexpr int LBLOCK = 8 * LSTRIDE;

__constant__ unsigned char ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct JpegArgs {
  const unsigned char* src;
  int64_t src_bytes;
  const JpegSample* samples;
  const uint32_t* tab;      // [TAB_WORDS]
  unsigned char* out;
  int64_t out_bytes;
  int64_t* table;           // [B + 1][2]: offset and length of every sample's scan in out; row B = total bytes, status
  int16_t* coef;            // [B][max_blocks][64]
  uint32_t* bits;           // [B][max_blocks]: AC bits of a block, then its bit offset in the sample's stream
  uint32_t* stream;         // [B][stream_words]: the unstuffed bit streams
  uint32_t* info;           // [B][4]: bits, bytes of the unstuffed stream, FF bytes, accepted
  uint32_t* ffcount;        // [B][max_chunks]: FF bytes of a chunk, then the FF bytes before it
  int32_t B, max_h, max_w, max_blocks, max_chunks;
  int64_t stream_words;
};

__device__ __forceinline__ bool record_ok(const JpegArgs& a, const JpegSample& s) {
  if (s.h < 1 || s.w < 1 || s.h > 65535 || s.w > 65535 || s.h > a.max_h || s.w > a.max_w || s.offset < 0) return false;
  return s.offset + (int64_t)s.h * s.w * 3 <= a.src_bytes;
}

// 0 for 0; no coefficient of 8-bit samples reaches 16 bits, the bound keeps a lookup inside its table whatever the quantiser holds
__device__ __forceinline__ int bit_length(int v) { return min(32 - __clz(v < 0 ? -v : v), 15); }

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c's 8-point pass over d[0], d[stride], ...; first = rows (results scaled up by 4), else columns (scaled back down)
__device__ __forceinline__ void fdct_pass(int* d, int stride, bool first) {
  const int d0 = d[0], d1 = d[stride], d2 = d[2 * stride], d3 = d[3 * stride], d4 = d[4 * stride], d5 = d[5 * stride], d6 = d[6 * stride],
            d7 = d[7 * stride];
  const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  const int n = first ? 11 : 15;
  d[0] = first ? (t10 + t11) << 2 : descale(t10 + t11, 2);
  d[4 * stride] = first ? (t10 - t11) << 2 : descale(t10 - t11, 2);
  int z1 = (t12 + t13) * 4433;
  d[2 * stride] = descale(z1 + t13 * 6270, n);
  d[6 * stride] = descale(z1 - t12 * 15137, n);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int m4 = t4 * 2446, m5 = t5 * 16819, m6 = t6 * 25172, m7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7 * stride] = descale(m4 + z1 + z3, n);
  d[5 * stride] = descale(m5 + z2 + z4, n);
  d[3 * stride] = descale(m6 + z2 + z3, n);
  d[stride] = descale(m7 + z1 + z4, n);
}

__device__ __forceinline__ int quantise(int c, uint32_t q) {
  const uint32_t div = q << 3;
  const uint32_t t = ((uint32_t)(c < 0 ? -c : c) + (div >> 1)) / div;
  return c < 0 ? -(int)t : (int)t;
}

// blocks: grid = (ceil(max_mcus / 4), B), 256 threads = 4 waves, one MCU each
__global__ void __launch_bounds__(256) jpeg_blocks_kernel(const JpegArgs a) {
  __shared__ int data[4][6 * LBLOCK];
  __shared__ uint32_t tab[TAB_WORDS];
  const JpegSample s = a.samples[blockIdx.y];
  if (!record_ok(a, s)) return;                 // the offsets kernel reports it
  for (int i = threadIdx.x; i < TAB_WORDS; i += 256) tab[i] = a.tab[i];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int mw = (s.w + 15) >> 4, mh = (s.h + 15) >> 4;
  const int mcu = blockIdx.x * 4 + wave;
  const bool active = mcu < mw * mh;
  const int my = mcu / mw, mx = mcu - my * mw;
  int* d = data[wave];
  if (active) {
    // a lane owns one 2 x 2 cell: four luma samples and one sample of each chroma plane
    const int cy = lane >> 3, cx = lane & 7;
    const int ch = (s.h + 1) >> 1;
    const int x0 = min(mx * 16 + 2 * cx, s.w - 1), x1 = min(mx * 16 + 2 * cx + 1, s.w - 1);
    const int r = my * 8 + cy;                  // the chroma row; rows below the plane repeat its last row
    const int rc = min(r, ch - 1);
    const unsigned char* base = a.src + s.offset;
    int cb = 0, cr = 0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const int yl = min(2 * r + dy, s.h - 1), yc = min(2 * rc + dy, s.h - 1);
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const unsigned char* p = base + ((size_t)yl * s.w + (dx ? x1 : x0)) * 3;
        int R = p[0], G = p[1], B = p[2];
        const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
        const int row = (2 * cy + dy) & 7, col = (2 * cx + dx) & 7, blk = (cy >> 2) * 2 + (cx >> 2);
        d[blk * LBLOCK + row * LSTRIDE + col] = Y - 128;
        if (yc != yl) {
          p = base + ((size_t)yc * s.w + (dx ? x1 : x0)) * 3;
          R = p[0], G = p[1], B = p[2];
        }
        cb += (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
        cr += (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
      }
    }
    const int bias = 1 + (cx & 1);
    d[4 * LBLOCK + cy * LSTRIDE + cx] = ((cb + bias) >> 2) - 128;
    d[5 * LBLOCK + cy * LSTRIDE + cx] = ((cr + bias) >> 2) - 128;
  }
  __syncthreads();
  if (active && lane < 48) fdct_pass(d + (lane >> 3) * LBLOCK + (lane & 7) * LSTRIDE, 1, true);
  __syncthreads();
  if (active && lane < 48) fdct_pass(d + (lane >> 3) * LBLOCK + (lane & 7), LSTRIDE, false);
  __syncthreads();
  if (!active) return;
  // lane k owns coefficient k (zigzag order) of each of the six blocks
  const int nat = ZIGZAG[lane];
  const int at = (nat >> 3) * LSTRIDE + (nat & 7);
  // dummy blocks (jccoefct.c): outside the component's block grid the AC terms are zero and the DC repeats a neighbour's inside the MCU
  const bool col_in = mx * 2 + 1 < ((s.w + 7) >> 3), row_in = my * 2 + 1 < ((s.h + 7) >> 3);
  const uint32_t q0 = tab[TAB_Q];
  const int dc00 = quantise(d[0], q0);
  const int dc01 = col_in ? quantise(d[LBLOCK], q0) : dc00;
  const int dc10 = row_in ? quantise(d[2 * LBLOCK], q0) : dc01;
  const int dc11 = row_in ? (col_in ? quantise(d[3 * LBLOCK], q0) : dc10) : dc01;
  const size_t first = (size_t)blockIdx.y * a.max_blocks + (size_t)mcu * 6;
#pragma unroll
  for (int blk = 0; blk < 6; ++blk) {
    const int comp = blk < 4 ? 0 : 1;
    int v = quantise(d[blk * LBLOCK + at], tab[TAB_Q + comp * 64 + lane]);
    const bool dummy = (blk == 1 && !col_in) || (blk == 2 && !row_in) || (blk == 3 && !(row_in && col_in));
    if (dummy) v = lane ? 0 : (blk == 1 ? dc01 : blk == 2 ? dc10 : dc11);
    a.coef[(first + blk) * 64 + lane] = (int16_t)v;
    // AC bits: a non-zero coefficient pays for the zeros since the previous one (a 0xF0 per 16 of them), its symbol and its value bits
    const unsigned long long nz = __ballot(v != 0 && lane > 0);
    int bits = 0;
    if (v != 0 && lane > 0) {
      const unsigned long long below = nz & ((1ull << lane) - 1);
      const int prev = below ? 63 - __clzll(below) : 0;
      const int run = lane - prev - 1, size = bit_length(v);
      bits = (run >> 4) * (int)(tab[TAB_AC + comp * 256 + 0xF0] >> 16) + (int)(tab[TAB_AC + comp * 256 + (((run & 15) << 4) | size)] >> 16) + size;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bits += __shfl_xor(bits, o, 64);
    if (!(nz >> 63)) bits += (int)(tab[TAB_AC + comp * 256] >> 16);         // the block ends in zeros: EOB
    if (lane == 0) a.bits[first + blk] = (uint32_t)bits;
  }
}

// exclusive scan of one value per thread over the workgroup (256 threads); *total = the sum.  Every thread must call it.
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* wave_sums, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)inc, o, 64);
    if (lane >= o) inc += up;
  }
  __syncthreads();                  // the previous call's readers are done with wave_sums
  if (lane == 63) wave_sums[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t w = wave_sums[i];
    if (i < wave) before += w;
    all += w;
  }
  *total = all;
  return before + inc - v;
}

// offsets: grid = (B), one workgroup per sample
__global__ void __launch_bounds__(256) jpeg_offsets_kernel(const JpegArgs a) {
  __shared__ uint32_t wave_sums[4];
  __shared__ uint32_t dc_len[32];
  const int b = blockIdx.x;
  const JpegSample s = a.samples[b];
  uint32_t* info = a.info + (size_t)b * 4;
  if (!record_ok(a, s)) {
    if (threadIdx.x == 0) {
      info[0] = info[1] = info[2] = info[3] = 0;
      a.table[2 * (size_t)a.B + 1] = 1;         // every writer of the status stores the same value
    }
    return;
  }
  if (threadIdx.x < 32) dc_len[threadIdx.x] = a.tab[TAB_DC + threadIdx.x] >> 16;
  __syncthreads();
  const int nblocks = ((s.w + 15) >> 4) * ((s.h + 15) >> 4) * 6;
  const int16_t* coef = a.coef + (size_t)b * a.max_blocks * 64;
  uint32_t* bits = a.bits + (size_t)b * a.max_blocks;
  uint32_t carry = 0;
  for (int start = 0; start < nblocks; start += 1024) {         // 4 consecutive blocks per thread
    const int i0 = start + threadIdx.x * 4;
    uint32_t v[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = i0 + j;
      v[j] = 0;
      if (i < nblocks) {
        // the previous block of the same component: the block before (luma inside an MCU) or the previous MCU's last of that component
        const int m = i / 6, k = i - m * 6;
        const int prev = (k >= 1 && k <= 3) ? i - 1 : (m > 0 ? (m - 1) * 6 + (k == 0 ? 3 : k) : -1);
        const int diff = (int)coef[(size_t)i * 64] - (prev >= 0 ? (int)coef[(size_t)prev * 64] : 0);
        const int cat = bit_length(diff);
        v[j] = bits[i] + dc_len[(k < 4 ? 0 : 16) + cat] + cat;
      }
      sum += v[j];
    }
    uint32_t total;
    uint32_t off = carry + block_scan(sum, wave_sums, &total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i0 + j < nblocks) bits[i0 + j] = off;
      off += v[j];
    }
    carry += total;
  }
  // the words the pack kernel will OR into, and one more
  uint32_t* stream = a.stream + (size_t)b * a.stream_words;
  const uint32_t nwords = carry / 32 + 2;
  for (uint32_t i = threadIdx.x; i < nwords; i += 256) stream[i] = 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    info[0] = carry;
    info[1] = (carry + 7) / 8;
    info[3] = 1;
    const uint32_t pad = (8 - (carry & 7)) & 7;                // closing one-bits up to the byte boundary; they never cross a word
    if (pad) stream[carry / 32] = __builtin_bswap32(((1u << pad) - 1) << (32 - (carry & 31) - pad));
  }
}

// MSB-first bit writer over the big-endian words of a stream; a word the block does not own alone is merged atomically
struct BitWriter {
  uint32_t* word;
  unsigned long long acc;
  int n;
  bool shared;          // the next word to leave may hold another block's bits
  __device__ __forceinline__ void put(uint32_t code, int len) {
    acc = (acc << len) | code;
    n += len;
    if (n >= 32) {
      n -= 32;
      const uint32_t w = __builtin_bswap32((uint32_t)(acc >> n));
      if (shared) atomicOr(word, w);
      else *word = w;
      shared = false;
      ++word;
    }
  }
  __device__ __forceinline__ void finish() {
    if (n > 0) atomicOr(word, __builtin_bswap32((uint32_t)(acc << (32 - n))));
  }
};

// pack: grid = (ceil(max_blocks / 256), B), one thread per block
__global__ void __launch_bounds__(256) jpeg_pack_kernel(const JpegArgs a) {
  __shared__ uint32_t tab[32 + 512];
  const int b = blockIdx.y;
  const JpegSample s = a.samples[b];
  if (!record_ok(a, s)) return;
  const int nblocks = ((s.w + 15) >> 4) * ((s.h + 15) >> 4) * 6;
  if ((int)(blockIdx.x * 256) >= nblocks) return;
  for (int i = threadIdx.x; i < 32 + 512; i += 256) tab[i] = a.tab[TAB_DC + i];
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nblocks) return;
  const int16_t* coef = a.coef + (size_t)b * a.max_blocks * 64;
  const int m = i / 6, k = i - m * 6;
  const int prev = (k >= 1 && k <= 3) ? i - 1 : (m > 0 ? (m - 1) * 6 + (k == 0 ? 3 : k) : -1);
  const uint32_t* dc = tab + (k < 4 ? 0 : 16);
  const uint32_t* ac = tab + 32 + (k < 4 ? 0 : 256);
  const uint32_t off = a.bits[(size_t)b * a.max_blocks + i];
  BitWriter bw;
  bw.word = a.stream + (size_t)b * a.stream_words + off / 32;
  bw.acc = 0;
  bw.n = (int)(off & 31);
  bw.shared = true;
  const uint4* row = reinterpret_cast<const uint4*>(coef + (size_t)i * 64);
  int run = 0;
  for (int g = 0; g < 8; ++g) {
    const uint4 q = row[g];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int v = (int)(int16_t)(w[j >> 1] >> (16 * (j & 1)));
      if (g == 0 && j == 0) {
        const int diff = v - (prev >= 0 ? (int)coef[(size_t)prev * 64] : 0);
        const int cat = bit_length(diff);
        const uint32_t e = dc[cat];
        bw.put(((e & 0xffff) << cat) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1)), (int)(e >> 16) + cat);
        continue;
      }
      if (v == 0) {
        ++run;
        continue;
      }
      while (run > 15) {
        bw.put(ac[0xF0] & 0xffff, (int)(ac[0xF0] >> 16));
        run -= 16;
      }
      const int size = bit_length(v);
      const uint32_t e = ac[(run << 4) | size];
      bw.put(((e & 0xffff) << size) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1)), (int)(e >> 16) + size);
      run = 0;
    }
  }
  if (run) bw.put(ac[0] & 0xffff, (int)(ac[0] >> 16));
  bw.finish();
}

// the FF bytes among a thread's 16 bytes of a sample's unstuffed stream
__device__ __forceinline__ uint32_t load_chunk_bytes(const JpegArgs& a, int b, uint32_t nbytes, uint32_t pos, uint4* q) {
  *q = make_uint4(0, 0, 0, 0);
  if (pos >= nbytes) return 0;
  *q = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(a.stream + (size_t)b * a.stream_words) + pos);
  const uint32_t w[4] = {q->x, q->y, q->z, q->w};
  uint32_t n = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (pos + j < nbytes && ((w[j >> 2] >> (8 * (j & 3))) & 0xff) == 0xff) ++n;
  return n;
}

// count: grid = (max_chunks, B)
__global__ void __launch_bounds__(256) jpeg_count_kernel(const JpegArgs a) {
  __shared__ uint32_t wave_sums[4];
  const int b = blockIdx.y;
  const uint32_t nbytes = a.info[(size_t)b * 4 + 1];
  if (blockIdx.x * (uint32_t)CHUNK >= nbytes) return;
  uint4 q;
  uint32_t total;
  block_scan(load_chunk_bytes(a, b, nbytes, blockIdx.x * CHUNK + threadIdx.x * 16, &q), wave_sums, &total);
  if (threadIdx.x == 0) a.ffcount[(size_t)b * a.max_chunks + blockIdx.x] = total;
}

// place: one workgroup walks the samples in order: FF bytes before each chunk, then every sample's place in the output
__global__ void __launch_bounds__(256) jpeg_place_kernel(const JpegArgs a) {
  __shared__ uint32_t wave_sums[4];
  int64_t at = 0;
  for (int b = 0; b < a.B; ++b) {
    uint32_t* info = a.info + (size_t)b * 4;
    const uint32_t nbytes = info[1];
    const int nchunks = (int)((nbytes + CHUNK - 1) / CHUNK);
    uint32_t* ff = a.ffcount + (size_t)b * a.max_chunks;
    uint32_t carry = 0;
    for (int start = 0; start < nchunks; start += 256) {
      const int i = start + threadIdx.x;
      const uint32_t v = i < nchunks ? ff[i] : 0;
      uint32_t total;
      const uint32_t before = carry + block_scan(v, wave_sums, &total);
      if (i < nchunks) ff[i] = before;
      carry += total;
    }
    const int64_t len = (int64_t)nbytes + carry;
    const bool fits = info[3] != 0 && at + len <= a.out_bytes;
    __syncthreads();                                    // info[3] has been read by every thread
    if (threadIdx.x == 0) {
      info[2] = carry;
      if (info[3] != 0 && !fits) a.table[2 * (size_t)a.B + 1] = 1;       // the output buffer is too small for this sample
      info[3] = fits ? 1 : 0;
      a.table[2 * (size_t)b] = at;
      a.table[2 * (size_t)b + 1] = fits ? len : 0;
    }
    if (fits) at += len;
  }
  if (threadIdx.x == 0) a.table[2 * (size_t)a.B] = at;
}

// scatter: grid = (max_chunks, B): a thread writes its 16 bytes, a zero behind every FF
__global__ void __launch_bounds__(256) jpeg_scatter_kernel(const JpegArgs a) {
  __shared__ uint32_t wave_sums[4];
  const int b = blockIdx.y;
  const uint32_t* info = a.info + (size_t)b * 4;
  const uint32_t nbytes = info[1];
  if (info[3] == 0 || blockIdx.x * (uint32_t)CHUNK >= nbytes) return;
  const uint32_t pos = blockIdx.x * CHUNK + threadIdx.x * 16;
  uint4 q;
  uint32_t total;
  const uint32_t before = block_scan(load_chunk_bytes(a, b, nbytes, pos, &q), wave_sums, &total);
  if (pos >= nbytes) return;
  // inside the output: the place kernel accepted the sample whole
  unsigned char* o = a.out + a.table[2 * (size_t)b] + pos + a.ffcount[(size_t)b * a.max_chunks + blockIdx.x] + before;
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const unsigned char v = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
    if (pos + j < nbytes) {
      *o++ = v;
      if (v == 0xff) *o++ = 0;
    }
  }
}

// the workspace's parts, in bytes from its start
struct JpegLayout {
  int64_t coef, bits, stream, info, ffcount, total;
  int64_t stream_words;
  int32_t max_blocks, max_chunks;
};
bool layout_of(int32_t B, int32_t max_h, int32_t max_w, JpegLayout* l) {
  if (B < 1 || B > 65535 || max_h < 1 || max_w < 1 || max_h > 65535 || max_w > 65535) return false;
  const int64_t blocks = fp_ceil_div(max_w, 16) * fp_ceil_div(max_h, 16) * 6;
  if (blocks * BLOCK_BITS >= ((int64_t)1 << 31)) return false;          // bit offsets are 32-bit
  const int64_t stream_bytes = (fp_ceil_div(blocks * BLOCK_BITS, 8) + 8 + 15) & ~(int64_t)15;   // the zeroed word behind the last one
  l->max_blocks = (int32_t)blocks;
  l->max_chunks = (int32_t)fp_ceil_div(stream_bytes, CHUNK);
  l->stream_words = stream_bytes / 4;
  l->coef = 0;
  l->bits = l->coef + (int64_t)B * blocks * 128;
  l->stream = (l->bits + (int64_t)B * blocks * 4 + 15) & ~(int64_t)15;
  l->info = l->stream + (int64_t)B * stream_bytes;
  l->ffcount = l->info + (int64_t)B * 16;
  l->total = l->ffcount + (int64_t)B * l->max_chunks * 4;
  return l->total < ((int64_t)1 << 40);
}

}  // namespace

extern "C" int32_t fp_jpeg_sample_bytes(void) { return (int32_t)sizeof(JpegSample); }
extern "C" int32_t fp_jpeg_table_words(void) { return TAB_WORDS; }

extern "C" int64_t fp_jpeg_workspace_bytes(int32_t B, int32_t max_h, int32_t max_w) {
  JpegLayout l;
  return layout_of(B, max_h, max_w, &l) ? l.total : -1;
}

extern "C" int64_t fp_jpeg_max_scan_bytes(int32_t B, int32_t max_h, int32_t max_w) {
  JpegLayout l;
  if (!layout_of(B, max_h, max_w, &l)) return -1;
  return (int64_t)B * 2 * fp_ceil_div((int64_t)l.max_blocks * BLOCK_BITS, 8);
}

extern "C" int fp_jpeg_encode(const uint8_t* src, int64_t src_bytes, const void* samples, const uint32_t* tables, uint8_t* out, int64_t out_bytes,
                              int64_t* table, int32_t B, int32_t max_h, int32_t max_w, void* workspace, int64_t workspace_bytes,
                              fp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FP_REQUIRE(src && samples && tables && out && table && src_bytes > 0 && out_bytes > 0, "fp_jpeg_encode: bad arguments");
  JpegLayout l;
  FP_REQUIRE(layout_of(B, max_h, max_w, &l), "fp_jpeg_encode: bad sizes or too large (fp_jpeg_workspace_bytes)");
  FP_REQUIRE(workspace && workspace_bytes >= l.total, "fp_jpeg_encode: workspace too small (fp_jpeg_workspace_bytes)");
  FP_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)table & 7) == 0 && ((uintptr_t)tables & 3) == 0,
             "fp_jpeg_encode: the workspace must be 16-byte aligned, the result table 8-byte, the code tables 4-byte");
  unsigned char* ws = (unsigned char*)workspace;
  JpegArgs a;
  a.src = src; a.src_bytes = src_bytes; a.samples = (const JpegSample*)samples; a.tab = tables; a.out = out; a.out_bytes = out_bytes;
  a.table = table; a.coef = (int16_t*)(ws + l.coef); a.bits = (uint32_t*)(ws + l.bits); a.stream = (uint32_t*)(ws + l.stream);
  a.info = (uint32_t*)(ws + l.info); a.ffcount = (uint32_t*)(ws + l.ffcount);
  a.B = B; a.max_h = max_h; a.max_w = max_w; a.max_blocks = l.max_blocks; a.max_chunks = l.max_chunks; a.stream_words = l.stream_words;
  // the status of this call (a fill, not a launch through fp_launch: like fp_vis_overlay this call is not recorded into a launch plan)
  hipError_t e = hipMemsetAsync(table + 2 * (size_t)B, 0, 16, stream);
  if (e != hipSuccess) return fp_set_error((int)e, "fp_jpeg_encode: %s", hipGetErrorString(e));
  // the sample records live on the device: every kernel is launched for the largest sample and leaves early where it has nothing to do
  const unsigned chunks_x = (unsigned)l.max_chunks;          // below 2^16: the streams' bit offsets are 32-bit
  fp_launch(jpeg_blocks_kernel, dim3((unsigned)fp_ceil_div(l.max_blocks / 6, 4), B), dim3(256), 0, stream, a);
  int rc = fp_check_launch("fp_jpeg_encode(blocks)");
  if (rc) return rc;
  fp_launch(jpeg_offsets_kernel, dim3(B), dim3(256), 0, stream, a);
  rc = fp_check_launch("fp_jpeg_encode(offsets)");
  if (rc) return rc;
  fp_launch(jpeg_pack_kernel, dim3((unsigned)fp_ceil_div(l.max_blocks, 256), B), dim3(256), 0, stream, a);
  rc = fp_check_launch("fp_jpeg_encode(pack)");
  if (rc) return rc;
  fp_launch(jpeg_count_kernel, dim3(chunks_x, B), dim3(256), 0, stream, a);
  rc = fp_check_launch("fp_jpeg_encode(count)");
  if (rc) return rc;
  fp_launch(jpeg_place_kernel, dim3(1), dim3(256), 0, stream, a);
  rc = fp_check_launch("fp_jpeg_encode(place)");
  if (rc) return rc;
  fp_launch(jpeg_scatter_kernel, dim3(chunks_x, B), dim3(256), 0, stream, a);
  return fp_check_launch("fp_jpeg_encode(scatter)");
}
