// Baseline JPEG decoder on the device: what `PIL.Image.open(f).convert("RGB")` returns for a baseline file --
// SOF0, 8 bits, one interleaved scan, no restart markers, grey or YCbCr with luma sampling 1x1, 2x1 or 2x2 -- byte for byte, for Pillow
// builds on libjpeg-turbo or libjpeg 6b.  Everything is integer.
//   restated: libjpeg's jdhuff.c (decode_mcu's symbol loop, jpeg_make_d_derived_tbl's maxcode / valptr), jidctint.c, jdsample.c
//             (h2v1_fancy_upsample, h2v2_fancy_upsample with jdmainct.c's edge rows), jdcolor.c (the table form of ycc_rgb_convert).
// Nothing of a file's header is compiled in: the caller parses the markers (footprints_amd.ops.jpeg_parse), lays the entropy-coded
// segments of a batch one after the other and passes one table block per distinct set of quantisation and Huffman tables.
// Huffman decoding is serial per file, but the codes resynchronise: a decoder started at a wrong bit soon decodes the true symbols.  So a
// sample's scan is cut into subsequences of `subseq_bits` bits, one thread each, and a thread's exit state (bit position, block within
// the MCU, zigzag index) is the next thread's entry state; entry 0 is true, the others start as guesses and are iterated to a fixed
// point, which is the serial decode.  Launches, phases separated by kernel boundaries; no workgroup waits for another:
//   destuff   one workgroup per sample copies the scan without the zero byte behind every FF and pads it with one-bits
//   init      guessed entry states, zeroed coefficients, the record's verdict
//   sync      max_rounds launches, 64 subsequences per workgroup: hops loop in the kernel until nothing moves (at most 65); the exit of
//             a workgroup's last thread is stored for the next workgroup, which reads it in the NEXT launch; a sample none of whose
//             workgroups moved anything in a launch is settled and later launches leave at once
//   place     one workgroup per sample: exclusive scan of the blocks each subsequence completes; the sample's status
//   write     each thread decodes its subsequence once more and stores int16 coefficients [block][64] in natural order
//   dc        one workgroup per sample: prefix sums of the DC differences per component in scan order
//   idct      8 threads per block: dequantise, jidctint's column and row pass, +128, clamp, into component planes
//   colour    one thread per pixel: fancy upsampling of the chroma planes, YCbCr -> RGB, into the packed output
// fp_jpeg_decode_window decodes one rectangle (y0, x0, rh, rw) of every picture: the bytes of the whole picture's [y0:y0+rh, x0:x0+rw],
// dense at the sample's out_offset.  The entropy half is the same launches (a scan has no random access: every coefficient is decoded);
// the pixel half is proportional to the window.  The component planes stay frame-sized and keep the whole picture's addressing, so the
// upsampler's neighbours and edge clamps are the picture's; only the blocks the window needs are filled:
//   idct      the luma blocks that intersect the rectangle, and the chroma blocks that intersect its chroma footprint grown by one sample
//             on every side (clamped to the component): the fancy upsampler's far neighbour may lie in an MCU the window does not touch
//   colour    one thread per window pixel
#include <algorithm>

#include "fp_common.h"

namespace {

struct DecSample {          // fp_jpeg_decode_sample
  int64_t scan_offset;      // of the entropy-coded segment in `scans`
  int64_t out_offset;       // of the picture's first byte in `out`; dense uint8 [h][w][3]
  int32_t scan_bytes;       // of the segment, stuffed zero bytes included
  int32_t h, w;
  int32_t ncomp;            // 1 (grey) or 3 (YCbCr)
  int32_t hs, vs;           // luma sampling factors: 1x1, 2x1 or 2x2; the chroma components are 1x1
  int32_t table_set;        // index of the table block
  int32_t reserved;
};
struct DecWinSample {       // fp_jpeg_decode_window_sample: the same fields, then the rectangle; out_offset is the window's, dense uint8 [rh][rw][3]
  DecSample s;
  int32_t y0, x0, rh, rw;
};
struct Rect {
  int y0, x0, rh, rw;
};

// one table block, in 32-bit words
constexpr int TAB_SEL = 0;          // [3][4]: per component the quantisation table, the DC and the AC Huffman table (0..3, 0..1, 0..1)
constexpr int TAB_Q = 16;           // [4][64]: quantisation values in natural order
constexpr int TAB_H = 272;          // [4] Huffman tables: DC 0, DC 1, AC 0, AC 1
constexpr int H_LOOK = 0;           // [256]: length << 8 | symbol of the code the 8 bits begin with, 0 = longer than 8 bits
constexpr int H_MAXCODE = 256;      // [18]: largest code of a length (index 1..16), -1 = none
constexpr int H_VALOFF = 274;       // [18]: index of a length's first symbol minus its first code
constexpr int H_VAL = 292;          // [64]: the 256 symbols, four to a word, lowest byte first
constexpr int H_WORDS = 356;
constexpr int TAB_WORDS = TAB_H + 4 * H_WORDS;          // 1696

constexpr int GROUP = 64;           // subsequences (threads) per workgroup of the sync and write kernels
constexpr int STAGE_MAX_BITS = 2048;    // subsequences up to this length are decoded out of LDS: 2 * bits + 4 words per workgroup
constexpr int INFO = 8;             // int32 per sample at the start of the workspace
constexpr int I_BYTES = 0;          // bytes of the destuffed scan
constexpr int I_CHANGE = 1;         // 1 + the last sync launch in which a workgroup moved something
constexpr int I_HOPS = 2;           // the most hops a workgroup looped in one launch
constexpr int I_BLOCKS = 3;         // blocks the subsequences completed
constexpr int I_OK = 4;             // the record was accepted
constexpr int I_BAD = 5;            // the write pass met a code no table has or a zigzag index past 63

__constant__ unsigned char NATURAL[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct DecArgs {
  const unsigned char* scans;
  int64_t scans_bytes;
  const unsigned char* samples;     // [B] records of sample_stride bytes: DecSample, or DecWinSample when `windowed`
  const uint32_t* tables;   // [n_sets][TAB_WORDS]
  unsigned char* out;
  int64_t out_bytes;
  int32_t* status;          // [B + 1]
  int32_t* info;            // [B][INFO]
  unsigned char* stream;    // [B][stream_stride]: the destuffed scans
  unsigned long long* entry;    // [B][max_sub + 1]: entry states, bit position << 16 | block within the MCU << 8 | zigzag index
  unsigned long long* done;     // [B][max_sub]: the entry state a subsequence was last decoded from
  unsigned long long* exits;    // [B][max_sub]: and the state it left in
  uint32_t* count;          // [B][max_sub]: blocks it completed, then the index of its first block
  int16_t* coef;            // [B][max_blocks][64]
  unsigned char* planes;    // [B][3][plane_bytes]
  int64_t stream_stride, plane_bytes;
  int32_t B, n_sets, max_h, max_w, max_scan, subseq_bits, max_sub, max_blocks, round;
  int32_t stage_words;      // of the dynamic LDS of the sync and write kernels; 0 = subsequences too long to stage
  int32_t sample_stride, windowed, max_win_h, max_win_w;
};

constexpr unsigned long long NEVER = ~0ull;

__device__ __forceinline__ DecSample sample_of(const DecArgs& a, int b) {
  return *reinterpret_cast<const DecSample*>(a.samples + (size_t)b * a.sample_stride);
}
// the rectangle of the picture a sample writes: the whole picture unless the call is windowed
__device__ __forceinline__ Rect rect_of(const DecArgs& a, int b, const DecSample& s) {
  Rect r = {0, 0, s.h, s.w};
  if (a.windowed) {
    const DecWinSample* ws = reinterpret_cast<const DecWinSample*>(a.samples + (size_t)b * a.sample_stride);
    r.y0 = ws->y0, r.x0 = ws->x0, r.rh = ws->rh, r.rw = ws->rw;
  }
  return r;
}

__device__ __forceinline__ bool record_ok(const DecArgs& a, int b, const DecSample& s) {
  if (s.h < 1 || s.w < 1 || s.h > 65535 || s.w > 65535 || s.h > a.max_h || s.w > a.max_w) return false;
  if (s.scan_bytes < 1 || s.scan_bytes > a.max_scan || s.scan_offset < 0 || s.scan_offset + s.scan_bytes > a.scans_bytes) return false;
  if (s.table_set < 0 || s.table_set >= a.n_sets) return false;
  if (s.ncomp == 1) {
    if (s.hs != 1 || s.vs != 1) return false;
  } else if (s.ncomp == 3) {
    if (!((s.hs == 1 && s.vs == 1) || (s.hs == 2 && s.vs == 1) || (s.hs == 2 && s.vs == 2))) return false;
  } else {
    return false;
  }
  const Rect r = rect_of(a, b, s);
  if (a.windowed) {                 // not empty and inside the picture (h, w >= 1 here; rh, rw <= 65535 before they are subtracted)
    if (r.rh < 1 || r.rw < 1 || r.rh > a.max_win_h || r.rw > a.max_win_w || r.y0 < 0 || r.x0 < 0) return false;
    if (r.y0 > s.h - r.rh || r.x0 > s.w - r.rw) return false;
  }
  return s.out_offset >= 0 && s.out_offset + (int64_t)r.rh * r.rw * 3 <= a.out_bytes;
}

struct Geom {
  int mx, my, nb, nluma, nblocks;       // MCUs across and down, blocks per MCU, luma blocks per MCU, blocks of the scan
};
__device__ __forceinline__ Geom geom_of(const DecSample& s) {
  Geom g;
  g.mx = (s.w + 8 * s.hs - 1) / (8 * s.hs);
  g.my = (s.h + 8 * s.vs - 1) / (8 * s.vs);
  g.nluma = s.hs * s.vs;
  g.nb = s.ncomp == 1 ? 1 : g.nluma + 2;
  g.nblocks = g.mx * g.my * g.nb;       // at most 3 * 8192 * 8192
  return g;
}

// exclusive scan of one value per thread over a workgroup of NW waves; *total = the sum.  Every thread must call it.
template <int NW>
__device__ __forceinline__ uint32_t group_scan(uint32_t v, uint32_t* wave_sums, uint32_t* total) {
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
  for (int i = 0; i < NW; ++i) {
    const uint32_t w = wave_sums[i];
    if (i < wave) before += w;
    all += w;
  }
  *total = all;
  return before + inc - v;
}

// destuff: grid = (B), 1024 threads, 16 bytes each per turn: a zero byte whose predecessor is FF is dropped
__global__ void __launch_bounds__(1024) dec_destuff_kernel(const DecArgs a) {
  __shared__ uint32_t wave_sums[16];
  const int b = blockIdx.x;
  const DecSample s = sample_of(a, b);
  if (!record_ok(a, b, s)) return;                 // the init kernel reports it
  const unsigned char* src = a.scans + s.scan_offset;
  unsigned char* dst = a.stream + (size_t)b * a.stream_stride;
  const int n = s.scan_bytes;
  uint32_t carry = 0;                           // bytes written so far
  for (int start = 0; start < n; start += 1024 * 16) {
    const int p0 = start + (int)threadIdx.x * 16;
    unsigned char v[16];
    uint32_t keep = 0, kept = 0;
    unsigned char prev = p0 > 0 && p0 < n ? src[p0 - 1] : 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      v[j] = p0 + j < n ? src[p0 + j] : 0;
      if (p0 + j < n && !(v[j] == 0 && prev == 0xFF)) {
        keep |= 1u << j;
        ++kept;
      }
      prev = v[j];
    }
    uint32_t total;
    uint32_t at = carry + group_scan<16>(kept, wave_sums, &total);
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (keep >> j & 1) dst[at++] = v[j];      // at < n <= max_scan: inside the sample's part
    carry += total;
  }
  // one-bits behind the last byte, as libjpeg pads: up to the word boundary and two words more (stream_stride >= max_scan + 16)
  const uint32_t end = ((carry + 3) & ~3u) + 8;
  for (uint32_t i = carry + threadIdx.x; i < end; i += 1024) dst[i] = 0xFF;
  if (threadIdx.x == 0) a.info[(size_t)b * INFO + I_BYTES] = (int32_t)carry;
}

// init: grid = (x, B), 256 threads
__global__ void __launch_bounds__(256) dec_init_kernel(const DecArgs a) {
  const int b = blockIdx.y;
  const DecSample s = sample_of(a, b);
  int32_t* info = a.info + (size_t)b * INFO;
  const bool ok = record_ok(a, b, s);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    info[I_CHANGE] = 0;
    info[I_HOPS] = 0;
    info[I_BLOCKS] = 0;
    info[I_BAD] = 0;
    info[I_OK] = ok ? 1 : 0;
    if (!ok) {
      info[I_BYTES] = 0;
      a.status[b] = 1;
      atomicMax(a.status + a.B, 1);
    }
  }
  if (!ok) return;
  const int nsub = (int)(((int64_t)s.scan_bytes * 8 + a.subseq_bits - 1) / a.subseq_bits);      // an upper bound: the destuffed scan is shorter
  const size_t stride = (size_t)gridDim.x * 256, t = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (size_t g = t; g <= (size_t)min(nsub, a.max_sub); g += stride) {
    a.entry[(size_t)b * (a.max_sub + 1) + g] = (unsigned long long)g * a.subseq_bits << 16;
    if (g < (size_t)a.max_sub) a.done[(size_t)b * a.max_sub + g] = NEVER;
  }
  const Geom g = geom_of(s);
  uint4* coef = reinterpret_cast<uint4*>(a.coef + (size_t)b * a.max_blocks * 64);
  const size_t n16 = (size_t)min(g.nblocks, a.max_blocks) * 8;
  for (size_t i = t; i < n16; i += stride) coef[i] = make_uint4(0, 0, 0, 0);
}

// a sample's destuffed scan as big-endian words: one-bits beyond `words` of them.  A symbol's position depends on the symbol before it, so
// every peek is a dependent load: the words a workgroup's subsequences can touch are staged in LDS (`staged` of them from word `base`,
// byte-swapped already), where such a load costs a tenth of one from memory; anything else is read from memory
struct BitReader {
  const uint32_t* w;
  uint32_t words;
  const uint32_t* lds;
  uint32_t base, staged;
  __device__ __forceinline__ uint32_t word(uint32_t i) const {
    const uint32_t j = i - base;
    if (j < staged) return lds[j];
    return i < words ? __builtin_bswap32(w[i]) : 0xFFFFFFFFu;
  }
  // the words of subsequences g0 .. g0 + GROUP - 1 of S bits each, and the two a peek at the last bit reaches
  __device__ __forceinline__ void stage(uint32_t* buffer, uint32_t room, uint32_t g0, uint32_t S) {
    lds = buffer;
    base = (uint32_t)(((unsigned long long)g0 * S) >> 5);
    staged = room;
    for (uint32_t j = threadIdx.x; j < room; j += GROUP) buffer[j] = base + j < words ? __builtin_bswap32(w[base + j]) : 0xFFFFFFFFu;
  }
  __device__ __forceinline__ uint32_t peek32(uint32_t pos) const {
    const uint32_t i = pos >> 5;
    const unsigned long long two = (unsigned long long)word(i) << 32 | word(i + 1);
    return (uint32_t)(two >> (32 - (pos & 31)));
  }
};

// the Huffman tables of a sample in LDS
struct HuffLds {
  const uint32_t* t;        // [4][H_WORDS]
  // -> length (0 = a code no table has) and symbol of the code `v16` (16 bits, most significant first) begins with
  __device__ __forceinline__ int decode(int table, uint32_t v16, int* sym) const {
    const uint32_t* h = t + table * H_WORDS;
    const uint32_t e = h[H_LOOK + (v16 >> 8)];
    if (e) {
      *sym = (int)(e & 255);
      return (int)(e >> 8) & 15;
    }
    int len = 9;
    while (len <= 16 && (int)(v16 >> (16 - len)) > (int)h[H_MAXCODE + len]) ++len;
    if (len > 16) return 0;
    const uint32_t at = ((v16 >> (16 - len)) + h[H_VALOFF + len]) & 255;
    *sym = (int)(h[H_VAL + (at >> 2)] >> (8 * (at & 3))) & 255;
    return len;
  }
};

struct Span {
  uint32_t pos;
  int blk, k;
  uint32_t count;
  bool bad;
};

// decode from the state in `sp` until the bit position reaches `end`.  WRITE: store the coefficients of blocks first + count < nblocks
// and stop behind the last block; a code no table has or a zigzag index past 63 sets `bad`.  Otherwise (a guess may be at a wrong phase)
// a code no table has skips one bit and a zigzag index past 63 closes the block.  A symbol that would need bits beyond the scan ends
// the run.  Every turn moves at least one bit forward or leaves: at most end - pos turns.
template <bool WRITE>
__device__ __forceinline__ void decode_span(Span& sp, uint32_t end, uint32_t total_bits, const BitReader& br, const HuffLds& hf, const int* sel,
                                            int nb, int nluma, int16_t* coef, uint32_t first, uint32_t nblocks, const unsigned char* natural) {
  uint32_t pos = sp.pos;
  int blk = sp.blk, k = sp.k;
  uint32_t count = 0;
  while (pos < end) {
    if (WRITE && first + count >= nblocks) break;
    const int comp = blk < nluma ? 0 : blk - nluma + 1;
    const uint32_t p = br.peek32(pos);
    int sym = 0;
    const int len = hf.decode(k == 0 ? sel[comp * 4 + 1] : 2 + sel[comp * 4 + 2], p >> 16, &sym);
    if (len == 0) {
      if (WRITE) sp.bad = true;
      ++pos;
      continue;
    }
    const int s = sym & 15, r = k == 0 ? 0 : sym >> 4;
    if (pos + len + s > total_bits) break;
    int v = 0;
    if (s) {
      v = (int)((p << len) >> (32 - s));
      if (v < (1 << (s - 1))) v -= (1 << s) - 1;
    }
    int at = -1;
    if (k == 0) {
      at = 0;
      k = 1;
    } else if (s == 0) {
      if (r == 15) {
        k += 16;
        if (WRITE && k > 64) sp.bad = true;
      } else {
        k = 64;
      }
    } else {
      k += r;
      if (k > 63) {
        if (WRITE) sp.bad = true;
        k = 64;
      } else {
        at = natural[k];
        ++k;
      }
    }
    if (WRITE && at >= 0) coef[((size_t)first + count) * 64 + at] = (int16_t)v;        // first + count < nblocks <= max_blocks
    pos += len + s;
    if (k >= 64) {
      k = 0;
      blk = blk + 1 == nb ? 0 : blk + 1;
      ++count;
    }
  }
  sp.pos = pos;
  sp.blk = blk;
  sp.k = k;
  sp.count = count;
}

__device__ __forceinline__ unsigned long long pack_state(const Span& sp) { return (unsigned long long)sp.pos << 16 | (unsigned)sp.blk << 8 | (unsigned)sp.k; }

__device__ __forceinline__ void load_tables(const DecArgs& a, const DecSample& s, uint32_t* huff, int* sel, unsigned char* natural) {
  const uint32_t* tab = a.tables + (size_t)s.table_set * TAB_WORDS;
  for (int i = threadIdx.x; i < 4 * H_WORDS; i += GROUP) huff[i] = tab[TAB_H + i];
  if (threadIdx.x < 12) {
    // selectors index tables: keep them inside whatever the block holds
    const int v = (int)tab[TAB_SEL + threadIdx.x];
    sel[threadIdx.x] = (threadIdx.x & 3) == 0 ? (v & 3) : (v & 1);
  }
  natural[threadIdx.x] = NATURAL[threadIdx.x];
}

// sync: grid = (ceil(max_sub / GROUP), B), GROUP threads, one subsequence each; launched max_rounds times with a.round = 0, 1, ...
__global__ void __launch_bounds__(GROUP) dec_sync_kernel(const DecArgs a) {
  __shared__ uint32_t huff[4 * H_WORDS];
  __shared__ int sel[12];
  __shared__ unsigned char natural[64];
  __shared__ unsigned long long s_entry[GROUP + 1];
  extern __shared__ uint32_t s_stage[];
  const int b = blockIdx.y;
  int32_t* info = a.info + (size_t)b * INFO;
  if (!info[I_OK]) return;
  if (a.round > 0 && info[I_CHANGE] < a.round) return;          // nothing moved in the launch before: settled
  const DecSample s = sample_of(a, b);
  const uint32_t nbytes = (uint32_t)info[I_BYTES];
  const uint32_t total_bits = nbytes * 8;
  const uint32_t S = (uint32_t)a.subseq_bits;
  const uint32_t nsub = max((total_bits + S - 1) / S, 1u);       // <= max_sub: nbytes <= scan_bytes <= max_scan
  const uint32_t g0 = blockIdx.x * GROUP;
  if (g0 >= nsub) return;
  load_tables(a, s, huff, sel, natural);
  const uint32_t g = g0 + threadIdx.x;
  const bool valid = g < nsub;
  unsigned long long* entry = a.entry + (size_t)b * (a.max_sub + 1);
  // the entry of the subsequence behind this workgroup's last one; entry[nsub] exists and belongs to nobody
  const uint32_t last = min(g0 + GROUP, nsub);
  if (valid) s_entry[threadIdx.x] = entry[g];
  if (threadIdx.x == 0) s_entry[last - g0] = entry[last];
  const size_t at = (size_t)b * a.max_sub + g;
  unsigned long long done = valid ? a.done[at] : NEVER, exit_state = valid ? a.exits[at] : 0;
  uint32_t count = valid ? a.count[at] : 0;
  __syncthreads();
  const unsigned long long behind = s_entry[last - g0];
  const Geom gm = geom_of(s);
  BitReader br;
  br.w = reinterpret_cast<const uint32_t*>(a.stream + (size_t)b * a.stream_stride);
  br.words = (nbytes + 3) / 4 + 1;
  br.stage(s_stage, (uint32_t)a.stage_words, g0, S);            // the loop's first barrier comes before the first peek
  HuffLds hf;
  hf.t = huff;
  const uint32_t end = min((g + 1) * S, total_bits);
  int hops = 0;
  bool moved = true;
  for (; hops <= GROUP && moved; ++hops) {
    const unsigned long long e = valid ? s_entry[threadIdx.x] : 0;
    __syncthreads();                    // every thread has read its entry
    bool mine = false;
    if (valid) {
      if (e != done) {
        Span sp;
        sp.pos = (uint32_t)(e >> 16);
        sp.blk = (int)(e >> 8) & 255;
        sp.k = (int)e & 255;
        sp.bad = false;
        if (sp.blk >= gm.nb) sp.blk = 0;                // states come from this kernel: the bound costs nothing
        if (sp.k > 63) sp.k = 0;
        decode_span<false>(sp, end, total_bits, br, hf, sel, gm.nb, gm.nluma, nullptr, 0, 0, natural);
        exit_state = pack_state(sp);
        count = sp.count;
        done = e;
      }
      if (s_entry[threadIdx.x + 1] != exit_state) {    // only this thread writes that slot
        s_entry[threadIdx.x + 1] = exit_state;
        mine = true;
      }
    }
    moved = __syncthreads_or(mine) != 0;
  }
  if (valid) {
    a.done[at] = done;
    a.exits[at] = exit_state;
    a.count[at] = count;
    if (threadIdx.x > 0) entry[g] = s_entry[threadIdx.x];
  }
  if (threadIdx.x == 0) {
    const unsigned long long now = s_entry[last - g0];
    if (now != behind) entry[last] = now;
    if (now != behind || moved) atomicMax(info + I_CHANGE, a.round + 1);
    atomicMax(info + I_HOPS, hops);
  }
}

// place: grid = (B), 256 threads: the index of every subsequence's first block, and the sample's verdict
__global__ void __launch_bounds__(256) dec_place_kernel(const DecArgs a, int rounds) {
  __shared__ uint32_t wave_sums[4];
  const int b = blockIdx.x;
  int32_t* info = a.info + (size_t)b * INFO;
  if (!info[I_OK]) return;
  const DecSample s = sample_of(a, b);
  const uint32_t total_bits = (uint32_t)info[I_BYTES] * 8, S = (uint32_t)a.subseq_bits;
  const uint32_t nsub = max((total_bits + S - 1) / S, 1u);
  const bool settled = info[I_CHANGE] < rounds;
  uint32_t* count = a.count + (size_t)b * a.max_sub;
  uint32_t carry = 0;
  if (settled) {
    for (uint32_t start = 0; start < nsub; start += 256) {
      const uint32_t i = start + threadIdx.x;
      const uint32_t v = i < nsub ? count[i] : 0;
      uint32_t total;
      const uint32_t before = carry + group_scan<4>(v, wave_sums, &total);
      if (i < nsub) count[i] = before;
      carry += total;
    }
  }
  if (threadIdx.x == 0) {
    info[I_BLOCKS] = (int32_t)carry;
    const int st = !settled ? 2 : (carry != (uint32_t)geom_of(s).nblocks ? 3 : 0);
    if (st) {
      a.status[b] = st;
      atomicMax(a.status + a.B, st);
    }
  }
}

// write: grid = (ceil(max_sub / GROUP), B)
__global__ void __launch_bounds__(GROUP) dec_write_kernel(const DecArgs a) {
  __shared__ uint32_t huff[4 * H_WORDS];
  __shared__ int sel[12];
  __shared__ unsigned char natural[64];
  extern __shared__ uint32_t s_stage[];
  const int b = blockIdx.y;
  int32_t* info = a.info + (size_t)b * INFO;
  if (!info[I_OK] || a.status[b] != 0) return;
  const DecSample s = sample_of(a, b);
  const uint32_t nbytes = (uint32_t)info[I_BYTES];
  const uint32_t total_bits = nbytes * 8, S = (uint32_t)a.subseq_bits;
  const uint32_t nsub = max((total_bits + S - 1) / S, 1u);
  if (blockIdx.x * GROUP >= nsub) return;
  load_tables(a, s, huff, sel, natural);
  BitReader br;
  br.w = reinterpret_cast<const uint32_t*>(a.stream + (size_t)b * a.stream_stride);
  br.words = (nbytes + 3) / 4 + 1;
  br.stage(s_stage, (uint32_t)a.stage_words, blockIdx.x * GROUP, S);
  __syncthreads();
  const uint32_t g = blockIdx.x * GROUP + threadIdx.x;
  if (g >= nsub) return;
  const Geom gm = geom_of(s);
  HuffLds hf;
  hf.t = huff;
  const unsigned long long e = a.entry[(size_t)b * (a.max_sub + 1) + g];
  Span sp;
  sp.pos = (uint32_t)(e >> 16);
  sp.blk = (int)(e >> 8) & 255;
  sp.k = (int)e & 255;
  sp.bad = false;
  if (sp.blk >= gm.nb) sp.blk = 0;
  if (sp.k > 63) sp.k = 0;
  const uint32_t nblocks = (uint32_t)min(gm.nblocks, a.max_blocks);
  decode_span<true>(sp, min((g + 1) * S, total_bits), total_bits, br, hf, sel, gm.nb, gm.nluma, a.coef + (size_t)b * a.max_blocks * 64,
                    a.count[(size_t)b * a.max_sub + g], nblocks, natural);
  if (sp.bad) info[I_BAD] = 1;          // every writer stores the same value; the dc kernel turns it into the status
}

// dc: grid = (B), 256 threads, 4 consecutive blocks each per turn: the DC term of a block is the sum of its component's differences so far
__global__ void __launch_bounds__(256) dec_dc_kernel(const DecArgs a) {
  __shared__ uint32_t wave_sums[4];
  const int b = blockIdx.x;
  const int32_t* info = a.info + (size_t)b * INFO;
  if (!info[I_OK]) return;
  if (info[I_BAD]) {                    // corrupt: the planes are not made, the colour kernel leaves
    if (threadIdx.x == 0) {
      a.status[b] = 3;
      atomicMax(a.status + a.B, 3);
    }
    return;
  }
  if (a.status[b] != 0) return;
  const DecSample s = sample_of(a, b);
  const Geom gm = geom_of(s);
  const int nblocks = min(gm.nblocks, a.max_blocks);
  int16_t* coef = a.coef + (size_t)b * a.max_blocks * 64;
  uint32_t carry[3] = {0, 0, 0};
  for (int start = 0; start < nblocks; start += 1024) {
    const int i0 = start + threadIdx.x * 4;
    uint32_t v[4], sum[3] = {0, 0, 0};
    int comp[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = i0 + j;
      v[j] = 0;
      comp[j] = 0;
      if (i < nblocks) {
        const int k = i % gm.nb;
        comp[j] = k < gm.nluma ? 0 : k - gm.nluma + 1;
        v[j] = (uint32_t)(int)coef[(size_t)i * 64];
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (comp[j] == c) sum[c] += v[j];
      }
    }
    uint32_t off[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint32_t total;
      off[c] = carry[c] + group_scan<4>(sum[c], wave_sums, &total);
      carry[c] += total;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i0 + j >= nblocks) continue;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (comp[j] == c) {
          off[c] += v[j];
          coef[(size_t)(i0 + j) * 64] = (int16_t)off[c];
        }
    }
  }
}

// jidctint.c's 8-point pass; n = 11 for the columns (results scaled up by 4), 18 for the rows
__device__ __forceinline__ void idct_pass(const int* d, int* o, int n) {
  int z2 = d[2], z3 = d[6];
  int z1 = (z2 + z3) * 4433;
  int t2 = z1 - z3 * 15137, t3 = z1 + z2 * 6270;
  int t0 = (d[0] + d[4]) * 8192, t1 = (d[0] - d[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
  z1 = t0 + t3, z2 = t1 + t2, z3 = t0 + t2;
  int z4 = t1 + t3;
  const int z5 = (z3 + z4) * 9633;
  t0 *= 2446, t1 *= 16819, t2 *= 25172, t3 *= 12299;
  z1 *= -7373, z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
  const int r = 1 << (n - 1);
  o[0] = (t10 + t3 + r) >> n;
  o[7] = (t10 - t3 + r) >> n;
  o[1] = (t11 + t2 + r) >> n;
  o[6] = (t11 - t2 + r) >> n;
  o[2] = (t12 + t1 + r) >> n;
  o[5] = (t12 - t1 + r) >> n;
  o[3] = (t13 + t0 + r) >> n;
  o[4] = (t13 - t0 + r) >> n;
}

// the plane of component c of a sample: rows of `stride` bytes, padded to whole blocks
__device__ __forceinline__ int plane_stride(const Geom& g, const DecSample& s, int c) { return g.mx * 8 * (c == 0 ? s.hs : 1); }

struct IdctLds {
  int ws[32][8][9];
  uint32_t quant[4 * 64];
  int sel[3];
};

// 256 threads = 32 blocks x 8 columns, then x 8 rows: thread group threadIdx.x >> 3 transforms block `i` of the scan (when `active`) into
// its place in its component's plane.  Every thread of the workgroup must call it.
__device__ __forceinline__ void idct_blocks(const DecArgs& a, int b, const DecSample& s, const Geom& gm, bool active, int i, IdctLds& l) {
  int (*ws)[8][9] = l.ws;
  uint32_t* quant = l.quant;
  int* sel = l.sel;
  const uint32_t* tab = a.tables + (size_t)s.table_set * TAB_WORDS;
  quant[threadIdx.x] = tab[TAB_Q + threadIdx.x];
  if (threadIdx.x < 3) sel[threadIdx.x] = (int)tab[TAB_SEL + threadIdx.x * 4] & 3;
  __syncthreads();
  const int lb = threadIdx.x >> 3, c = threadIdx.x & 7;
  const int m = i / gm.nb, k = i - m * gm.nb;
  const int comp = k < gm.nluma ? 0 : k - gm.nluma + 1;
  if (active) {
    const int16_t* blk = a.coef + ((size_t)b * a.max_blocks + i) * 64;
    const uint32_t* q = quant + sel[comp] * 64;
    int d[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = (int)blk[r * 8 + c] * (int)q[r * 8 + c];
    idct_pass(d, o, 11);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[lb][r][c] = o[r];
  }
  __syncthreads();
  if (!active) return;
  int d[8], o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) d[j] = ws[lb][c][j];
  idct_pass(d, o, 18);
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lo |= (uint32_t)min(max(o[j] + 128, 0), 255) << (8 * j);
    hi |= (uint32_t)min(max(o[j + 4] + 128, 0), 255) << (8 * j);
  }
  const int myy = m / gm.mx, mxx = m - myy * gm.mx;
  const int bx = comp == 0 ? mxx * s.hs + k % s.hs : mxx, by = comp == 0 ? myy * s.vs + k / s.hs : myy;
  // inside the plane: bx * 8 + 8 <= stride <= max_w rounded up to 16, by * 8 + 8 <= max_h rounded up to 16
  unsigned char* plane = a.planes + ((size_t)b * 3 + comp) * a.plane_bytes;
  *reinterpret_cast<uint2*>(plane + (size_t)(by * 8 + c) * plane_stride(gm, s, comp) + bx * 8) = make_uint2(lo, hi);
}

// idct: grid = (ceil(max_blocks / 32), B), 256 threads
__global__ void __launch_bounds__(256) dec_idct_kernel(const DecArgs a) {
  __shared__ IdctLds lds;
  const int b = blockIdx.y;
  const int32_t* info = a.info + (size_t)b * INFO;
  if (!info[I_OK] || a.status[b] != 0) return;
  const DecSample s = sample_of(a, b);
  const Geom gm = geom_of(s);
  const int nblocks = min(gm.nblocks, a.max_blocks);
  if ((int)blockIdx.x * 32 >= nblocks) return;
  const int i = blockIdx.x * 32 + (threadIdx.x >> 3);
  idct_blocks(a, b, s, gm, i < nblocks, i, lds);
}

// the blocks a window needs, per dimension a first block and a count: of the luma plane those that intersect the rectangle; of a chroma
// plane those that intersect the rectangle's chroma footprint grown by one sample on every side and clamped to the component
struct WinBlocks {
  int lx0, ly0, lnx, lny, cx0, cy0, cnx, cny;
};
__device__ __forceinline__ WinBlocks win_blocks(const DecSample& s, const Rect& r) {
  WinBlocks w;
  w.lx0 = r.x0 >> 3, w.ly0 = r.y0 >> 3;
  w.lnx = ((r.x0 + r.rw - 1) >> 3) - w.lx0 + 1, w.lny = ((r.y0 + r.rh - 1) >> 3) - w.ly0 + 1;
  w.cx0 = w.cy0 = w.cnx = w.cny = 0;
  if (s.ncomp == 3) {
    const int cw = (s.w + s.hs - 1) / s.hs, ch = (s.h + s.vs - 1) / s.vs;
    const int xa = max(r.x0 / s.hs - 1, 0), xb = min((r.x0 + r.rw - 1) / s.hs + 1, cw - 1);
    const int ya = max(r.y0 / s.vs - 1, 0), yb = min((r.y0 + r.rh - 1) / s.vs + 1, ch - 1);
    w.cx0 = xa >> 3, w.cy0 = ya >> 3;
    w.cnx = (xb >> 3) - w.cx0 + 1, w.cny = (yb >> 3) - w.cy0 + 1;
  }
  return w;
}
// an upper bound of the blocks a span of n samples touches, whatever its origin
inline int64_t span_blocks(int64_t n) { return (n + 6) / 8 + 1; }

// window idct: grid = (ceil(items / 32), B) for items = the most blocks a window of max_win_h x max_win_w needs, 256 threads
__global__ void __launch_bounds__(256) dec_idct_window_kernel(const DecArgs a) {
  __shared__ IdctLds lds;
  const int b = blockIdx.y;
  const int32_t* info = a.info + (size_t)b * INFO;
  if (!info[I_OK] || a.status[b] != 0) return;
  const DecSample s = sample_of(a, b);
  const Geom gm = geom_of(s);
  const WinBlocks w = win_blocks(s, rect_of(a, b, s));
  const int nl = w.lnx * w.lny, nc = w.cnx * w.cny;             // each at most (65535 / 8 + 2)^2
  if ((int64_t)blockIdx.x * 32 >= (int64_t)nl + 2 * nc) return;
  const int j = blockIdx.x * 32 + (threadIdx.x >> 3);
  bool active = j < nl + 2 * nc;
  int i = 0;
  if (active) {
    if (j < nl) {
      const int by = w.ly0 + j / w.lnx, bx = w.lx0 + j % w.lnx;
      i = ((by / s.vs) * gm.mx + bx / s.hs) * gm.nb + (by % s.vs) * s.hs + bx % s.hs;
    } else {
      const int comp = 1 + (j - nl) / nc, q = (j - nl) % nc;
      i = ((w.cy0 + q / w.cnx) * gm.mx + w.cx0 + q % w.cnx) * gm.nb + gm.nluma + comp - 1;
    }
    active = i < min(gm.nblocks, a.max_blocks);                 // always, for a record record_ok accepted: the guard of the loads
  }
  idct_blocks(a, b, s, gm, active, i, lds);
}

// one pixel (y, x) of the picture into the three bytes at `o`
__device__ __forceinline__ void colour_pixel(const DecArgs& a, int b, const DecSample& s, int y, int x, unsigned char* o) {
  const Geom gm = geom_of(s);
  const unsigned char* p0 = a.planes + (size_t)b * 3 * a.plane_bytes;
  const int Y = p0[(size_t)y * plane_stride(gm, s, 0) + x];
  if (s.ncomp == 1) {
    o[0] = o[1] = o[2] = (unsigned char)Y;
    return;
  }
  const int cs = plane_stride(gm, s, 1);
  const int cw = (s.w + s.hs - 1) / s.hs, ch = (s.h + s.vs - 1) / s.vs;      // the component's own size: its edge
  int cc[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const unsigned char* p = p0 + (size_t)(c + 1) * a.plane_bytes;
    if (s.hs == 1) {
      cc[c] = p[(size_t)y * cs + x];
    } else {
      const int cx = x >> 1, nx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
      if (s.vs == 1) {
        const unsigned char* row = p + (size_t)y * cs;
        cc[c] = (3 * row[cx] + row[nx] + ((x & 1) ? 2 : 1)) >> 2;
      } else {
        const int cy = y >> 1, ny = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
        const unsigned char *row = p + (size_t)cy * cs, *nrow = p + (size_t)ny * cs;
        const int here = 3 * row[cx] + nrow[cx], there = 3 * row[nx] + nrow[nx];
        cc[c] = (3 * here + there + ((x & 1) ? 7 : 8)) >> 4;
      }
    }
  }
  const int cb = cc[0] - 128, cr = cc[1] - 128;
  const int R = Y + ((91881 * cr + 32768) >> 16);
  const int B = Y + ((116130 * cb + 32768) >> 16);
  const int G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
  o[0] = (unsigned char)min(max(R, 0), 255);
  o[1] = (unsigned char)min(max(G, 0), 255);
  o[2] = (unsigned char)min(max(B, 0), 255);
}

// colour: grid = (ceil(max_h * max_w / 256), B), one pixel per thread
__global__ void __launch_bounds__(256) dec_colour_kernel(const DecArgs a) {
  const int b = blockIdx.y;
  const int32_t* info = a.info + (size_t)b * INFO;
  if (!info[I_OK] || a.status[b] != 0) return;
  const DecSample s = sample_of(a, b);
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= (int64_t)s.h * s.w) return;
  const int y = (int)(pix / s.w), x = (int)(pix - (int64_t)y * s.w);
  colour_pixel(a, b, s, y, x, a.out + s.out_offset + pix * 3);          // inside out: record_ok
}

// window colour: grid = (ceil(max_win_h * max_win_w / 256), B), one pixel of the window per thread, dense [rh][rw][3] at out_offset
__global__ void __launch_bounds__(256) dec_colour_window_kernel(const DecArgs a) {
  const int b = blockIdx.y;
  const int32_t* info = a.info + (size_t)b * INFO;
  if (!info[I_OK] || a.status[b] != 0) return;
  const DecSample s = sample_of(a, b);
  const Rect r = rect_of(a, b, s);
  const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= (int64_t)r.rh * r.rw) return;
  const int py = (int)(pix / r.rw), px = (int)(pix - (int64_t)py * r.rw);
  colour_pixel(a, b, s, r.y0 + py, r.x0 + px, a.out + s.out_offset + pix * 3);      // inside out and inside the picture: record_ok
}

// the workspace's parts, in bytes from its start
struct DecLayout {
  int64_t info, stream, entry, done, exits, count, coef, planes, total;
  int64_t stream_stride, plane_bytes;
  int32_t max_sub, max_blocks;
};
bool layout_of(int32_t B, int32_t max_h, int32_t max_w, int32_t max_scan, int32_t subseq_bits, DecLayout* l) {
  if (B < 1 || B > 65535 || max_h < 1 || max_w < 1 || max_h > 65535 || max_w > 65535) return false;
  if (max_scan < 1 || max_scan >= (1 << 28) || subseq_bits < 32 || subseq_bits > (1 << 20)) return false;      // bit positions are 32-bit
  const int64_t pw = fp_ceil_div(max_w, 16) * 16, ph = fp_ceil_div(max_h, 16) * 16;
  l->plane_bytes = pw * ph;
  l->max_blocks = (int32_t)((pw / 8) * (ph / 8) * 3);            // 4:4:4 needs the most
  l->max_sub = (int32_t)fp_ceil_div((int64_t)max_scan * 8, subseq_bits);
  l->stream_stride = (((int64_t)max_scan + 15) & ~(int64_t)15) + 16;
  l->info = 0;
  l->stream = ((int64_t)B * INFO * 4 + 15) & ~(int64_t)15;
  l->entry = l->stream + (int64_t)B * l->stream_stride;
  l->done = l->entry + (int64_t)B * (l->max_sub + 1) * 8;
  l->exits = l->done + (int64_t)B * l->max_sub * 8;
  l->count = l->exits + (int64_t)B * l->max_sub * 8;
  l->coef = (l->count + (int64_t)B * l->max_sub * 4 + 15) & ~(int64_t)15;
  l->planes = l->coef + (int64_t)B * l->max_blocks * 128;
  l->total = l->planes + (int64_t)B * 3 * l->plane_bytes;
  return l->total < ((int64_t)1 << 40);
}

}  // namespace

extern "C" int32_t fp_jpeg_decode_sample_bytes(void) { return (int32_t)sizeof(DecSample); }
extern "C" int32_t fp_jpeg_decode_table_words(void) { return TAB_WORDS; }

extern "C" int64_t fp_jpeg_decode_workspace_bytes(int32_t B, int32_t max_h, int32_t max_w, int32_t max_scan_bytes, int32_t subseq_bits) {
  DecLayout l;
  return layout_of(B, max_h, max_w, max_scan_bytes, subseq_bits, &l) ? l.total : -1;
}
extern "C" int32_t fp_jpeg_decode_window_sample_bytes(void) { return (int32_t)sizeof(DecWinSample); }

namespace {

int check_launch(const char* who, const char* kernel) {
  char what[64];
  snprintf(what, sizeof(what), "%s(%s)", who, kernel);
  return fp_check_launch(what);
}

// What fp_jpeg_decode and fp_jpeg_decode_window share: the checks of the batch-level arguments, the kernels' arguments, and the entropy half
// -- the statuses cleared, then destuff, init, max_rounds x sync, place, write, dc -- after which the coefficients of every sample whose
// status is 0 are complete.  sample_bytes: of one record; win_h = win_w = 0: whole pictures.
int decode_entropy(const char* who, const uint8_t* scans, int64_t scan_bytes, const void* samples, int32_t sample_bytes, const uint32_t* tables,
                   int32_t n_table_sets, uint8_t* out, int64_t out_bytes, int32_t* status, int32_t B, int32_t max_h, int32_t max_w, int32_t win_h,
                   int32_t win_w, int32_t max_scan_bytes, int32_t subseq_bits, int32_t max_rounds, void* workspace, int64_t workspace_bytes,
                   hipStream_t stream, DecArgs* args, DecLayout* layout) {
  FP_REQUIRE(scans && samples && tables && out && status && scan_bytes > 0 && out_bytes > 0 && n_table_sets > 0, "%s: bad arguments", who);
  FP_REQUIRE(max_rounds >= 1 && max_rounds <= 65536, "%s: max_rounds must be 1..65536", who);
  DecLayout& l = *layout;
  FP_REQUIRE(layout_of(B, max_h, max_w, max_scan_bytes, subseq_bits, &l), "%s: bad sizes or too large (fp_jpeg_decode_workspace_bytes)", who);
  FP_REQUIRE(workspace && workspace_bytes >= l.total, "%s: workspace too small (fp_jpeg_decode_workspace_bytes)", who);
  FP_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)status & 3) == 0 && ((uintptr_t)tables & 3) == 0 && ((uintptr_t)samples & 7) == 0,
             "%s: the workspace must be 16-byte aligned, the sample records 8-byte, the status and the tables 4-byte", who);
  unsigned char* ws = (unsigned char*)workspace;
  DecArgs& a = *args;
  a.scans = scans; a.scans_bytes = scan_bytes; a.samples = (const unsigned char*)samples; a.tables = tables; a.out = out; a.out_bytes = out_bytes;
  a.status = status; a.info = (int32_t*)(ws + l.info); a.stream = ws + l.stream; a.entry = (unsigned long long*)(ws + l.entry);
  a.done = (unsigned long long*)(ws + l.done); a.exits = (unsigned long long*)(ws + l.exits); a.count = (uint32_t*)(ws + l.count);
  a.coef = (int16_t*)(ws + l.coef); a.planes = ws + l.planes; a.stream_stride = l.stream_stride; a.plane_bytes = l.plane_bytes;
  a.B = B; a.n_sets = n_table_sets; a.max_h = max_h; a.max_w = max_w; a.max_scan = max_scan_bytes; a.subseq_bits = subseq_bits;
  a.max_sub = l.max_sub; a.max_blocks = l.max_blocks; a.round = 0;
  a.stage_words = subseq_bits <= STAGE_MAX_BITS ? 2 * subseq_bits + 4 : 0;
  a.sample_stride = sample_bytes; a.windowed = win_h > 0 ? 1 : 0; a.max_win_h = win_h; a.max_win_w = win_w;
  const unsigned stage_bytes = (unsigned)a.stage_words * 4;
  // the statuses (a fill, not a launch through fp_launch: like fp_jpeg_encode this call is not recorded into a launch plan)
  hipError_t e = hipMemsetAsync(status, 0, ((size_t)B + 1) * 4, stream);
  if (e != hipSuccess) return fp_set_error((int)e, "%s: %s", who, hipGetErrorString(e));
  // the sample records live on the device: every kernel is launched for the largest sample and leaves early where it has nothing to do
  const unsigned groups = (unsigned)fp_ceil_div(l.max_sub, GROUP);
  fp_launch(dec_destuff_kernel, dim3(B), dim3(1024), 0, stream, a);
  int rc = check_launch(who, "destuff");
  if (rc) return rc;
  fp_launch(dec_init_kernel, dim3((unsigned)std::min<int64_t>(fp_ceil_div((int64_t)l.max_blocks * 8, 256 * 4), 4096), B), dim3(256), 0, stream, a);
  rc = check_launch(who, "init");
  if (rc) return rc;
  for (int r = 0; r < max_rounds; ++r) {
    a.round = r;
    fp_launch(dec_sync_kernel, dim3(groups, B), dim3(GROUP), stage_bytes, stream, a);
    rc = check_launch(who, "sync");
    if (rc) return rc;
  }
  fp_launch(dec_place_kernel, dim3(B), dim3(256), 0, stream, a, (int)max_rounds);
  rc = check_launch(who, "place");
  if (rc) return rc;
  fp_launch(dec_write_kernel, dim3(groups, B), dim3(GROUP), stage_bytes, stream, a);
  rc = check_launch(who, "write");
  if (rc) return rc;
  fp_launch(dec_dc_kernel, dim3(B), dim3(256), 0, stream, a);
  return check_launch(who, "dc");
}

}  // namespace

extern "C" int fp_jpeg_decode(const uint8_t* scans, int64_t scan_bytes, const void* samples, const uint32_t* tables, int32_t n_table_sets,
                              uint8_t* out, int64_t out_bytes, int32_t* status, int32_t B, int32_t max_h, int32_t max_w, int32_t max_scan_bytes,
                              int32_t subseq_bits, int32_t max_rounds, void* workspace, int64_t workspace_bytes, fp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  DecArgs a;
  DecLayout l;
  int rc = decode_entropy("fp_jpeg_decode", scans, scan_bytes, samples, (int32_t)sizeof(DecSample), tables, n_table_sets, out, out_bytes, status, B,
                          max_h, max_w, 0, 0, max_scan_bytes, subseq_bits, max_rounds, workspace, workspace_bytes, stream, &a, &l);
  if (rc) return rc;
  fp_launch(dec_idct_kernel, dim3((unsigned)fp_ceil_div(l.max_blocks, 32), B), dim3(256), 0, stream, a);
  rc = fp_check_launch("fp_jpeg_decode(idct)");
  if (rc) return rc;
  fp_launch(dec_colour_kernel, dim3((unsigned)fp_ceil_div((int64_t)max_h * max_w, 256), B), dim3(256), 0, stream, a);
  return fp_check_launch("fp_jpeg_decode(colour)");
}

extern "C" int fp_jpeg_decode_window(const uint8_t* scans, int64_t scan_bytes, const void* samples, const uint32_t* tables, int32_t n_table_sets,
                                     uint8_t* out, int64_t out_bytes, int32_t* status, int32_t B, int32_t max_h, int32_t max_w,
                                     int32_t max_win_h, int32_t max_win_w, int32_t max_scan_bytes, int32_t subseq_bits, int32_t max_rounds,
                                     void* workspace, int64_t workspace_bytes, fp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  FP_REQUIRE(max_win_h >= 1 && max_win_w >= 1 && max_win_h <= max_h && max_win_w <= max_w,
             "fp_jpeg_decode_window: max_win_h / max_win_w must be 1..max_h / 1..max_w");
  DecArgs a;
  DecLayout l;
  int rc = decode_entropy("fp_jpeg_decode_window", scans, scan_bytes, samples, (int32_t)sizeof(DecWinSample), tables, n_table_sets, out, out_bytes,
                          status, B, max_h, max_w, max_win_h, max_win_w, max_scan_bytes, subseq_bits, max_rounds, workspace, workspace_bytes,
                          stream, &a, &l);
  if (rc) return rc;
  // the most blocks a window needs: luma over the rectangle, two chroma planes over a footprint of at most the rectangle plus two samples
  const int64_t items = std::min<int64_t>(span_blocks(max_win_h) * span_blocks(max_win_w) + 2 * span_blocks(max_win_h + 2) * span_blocks(max_win_w + 2),
                                          l.max_blocks);
  fp_launch(dec_idct_window_kernel, dim3((unsigned)fp_ceil_div(items, 32), B), dim3(256), 0, stream, a);
  rc = fp_check_launch("fp_jpeg_decode_window(idct)");
  if (rc) return rc;
  fp_launch(dec_colour_window_kernel, dim3((unsigned)fp_ceil_div((int64_t)max_win_h * max_win_w, 256), B), dim3(256), 0, stream, a);
  return fp_check_launch("fp_jpeg_decode_window(colour)");
}

