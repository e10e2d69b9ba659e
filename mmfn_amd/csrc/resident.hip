// Batch assembly from a device-resident sample store (data.ResidentFrames): one launch gathers every field of a batch by sample
// index - what PackedFrames.batch (np.take into pinned memory), the host->device copy and the u8 -> f32 widening of stage_batch do
// in three steps on two processors.  Values are only moved (and u8 widened, which is exact): no arithmetic - except in the second
// entry point at the end of the file, which gathers the camera field alone and colour-jitters it on the way, and in the third, which
// gathers the LiDAR frames, the lane set and the target point and drops cells and lanes and moves the map on the way, and in the
// fourth, which is the second with a hue shift, a Gaussian blur (the one neighbourhood operation here: LDS tiles) and sensor noise,
// and in the fifth, which gathers the radar returns and the speed, drops and perturbs them and rebuilds the radar adjacency.
//   dense field   dst[b] = f32(src[index[b]])
//   coded field   dst[b] = palette[4-bit codes of src[index[b]]]: a few-valued float field kept at half a byte per element
//   ragged field  rows [off[i], off[i+1]) of the concatenated source -> dst[b, :count]; rows count..Lmax-1 = +0.0; count -> int32
// Memory-bound, so shaped as the elementwise kernels here: a workgroup owns a contiguous piece of ONE (field, sample) row, a lane
// moves 16 source bytes per access (16 u8 pixels -> four 16-byte stores; 4 floats -> one; 32 codes -> eight), no atomics; LDS holds
// only a coded field's 16-entry palette (16 banks, equal addresses broadcast: no conflicts) and the 4 KB of codes of its piece.
// A row whose
// source and destination are misaligned in the same way gets a scalar head up to the first 16-byte boundary and a scalar tail; one
// whose misalignments differ (a 405-float radar row landing at another batch slot) is moved element by element - such rows are
// a few KB.  The sample indices and the ragged prefix table are read from device memory, so a captured launch follows them.
#include "common.h"

namespace {
constexpr int NT = 256;
constexpr int UNROLL = 4;                       // 16-byte accesses per lane and workgroup piece
constexpr int64_t PIECE_BYTES = (int64_t)NT * 16 * UNROLL;   // source bytes per workgroup: 16 KB
// a coded byte becomes 8 bytes of stores: ONE access per lane = 4 KB of codes = 32 KB of stores per workgroup, between the f32
// piece's 16 KB and the u8 piece's 64 KB, so a 64 KB LiDAR code row spreads over 16 workgroups (512 at batch 32) and not 4
constexpr int64_t PIECE_BYTES_PAL4 = (int64_t)NT * 16;

struct GatherArgs {
  mmfn_gather_field f[MMFN_GATHER_MAX_FIELDS];
  int32_t first_block[MMFN_GATHER_MAX_FIELDS + 1];   // running sum of the fields' pieces per sample
  int32_t n_fields;
  int32_t batch;                                     // > 0: a 1-D grid with the sample as the fastest index (see the launch)
};

__device__ __forceinline__ float src_at(const uint8_t* s, int64_t j) { return (float)s[j]; }
__device__ __forceinline__ float src_at(const float* s, int64_t j) { return s[j]; }
__device__ __forceinline__ void move16(const uint8_t* s, float* d) {   // 16 pixels
  const uint4 u = *reinterpret_cast<const uint4*>(s);
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (float)((w[k] >> (8 * e)) & 0xffu);
    *reinterpret_cast<f32x4*>(d + 4 * k) = v;
  }
}
__device__ __forceinline__ void move16(const float* s, float* d) { *reinterpret_cast<f32x4*>(d) = *reinterpret_cast<const f32x4*>(s); }

// coded source: byte j of a row holds element 2j (low nibble) and 2j + 1 (high); pal = the 16-entry table in LDS
__device__ __forceinline__ void code_byte(const float* pal, uint32_t c, float* d) {
  d[0] = pal[c & 15u];
  d[1] = pal[(c >> 4) & 15u];
}

// source BYTES [lo, hi) of one coded row -> destination floats [2 lo, 2 hi); head = bytes before the row's first 16-byte boundary.
// The 16-byte part of a piece is at most NT accesses: lane t reads 16 bytes once and passes them through `stage`, because its own 32
// floats as eight stores would put the lanes of a store 128 bytes apart (measured on the LiDAR field alone at batch 32: 9.65 us,
// against 8.34 us for its f32 form and 6.30 us this way).  Turned in LDS, store k of a wave covers 1 KB in one run: lane l takes the two bytes at 128 k + 2 l of the wave's 1 KB
// of codes (consecutive halfwords: no bank conflict) and writes their four floats.  Every thread of the workgroup calls this.
__device__ __forceinline__ void move_piece_pal4(const uint8_t* __restrict__ s, float* __restrict__ d, const float* __restrict__ palette,
                                                float* pal, uint4* stage, int64_t lo, int64_t hi, bool first_piece, int head,
                                                bool vec_ok) {
  const int tid = threadIdx.x;
  int64_t a = lo;
  int nv = 0;                                       // 16-byte accesses of this piece: 0..NT, the same for every lane
  if (vec_ok) {
    if (first_piece) a = head;
    if (hi > a) nv = (int)((hi - a) / 16);
  }
  if (tid < 16) pal[tid] = palette[tid];
  if (tid < nv) stage[tid] = *reinterpret_cast<const uint4*>(s + a + (int64_t)tid * 16);
  __syncthreads();
  if (vec_ok) {
    if (first_piece && tid < head && tid < hi) code_byte(pal, s[tid], d + 2 * tid);
    const uint16_t* codes = reinterpret_cast<const uint16_t*>(stage);
    const int base = (tid >> 6) * 1024 + 2 * (tid & 63);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int byte = base + 128 * k;              // even, and nv * 16 is too: byte + 1 is inside as well
      if (byte < nv * 16) {
        const uint32_t c = codes[byte >> 1];
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = pal[(c >> (4 * e)) & 15u];
        *reinterpret_cast<f32x4*>(d + 2 * (a + byte)) = v;
      }
    }
    a += (int64_t)nv * 16;
  }
  for (int64_t j = a + tid; j < hi; j += NT) code_byte(pal, s[j], d + 2 * j);
}

// elements [lo, hi) of one destination row: copies below `valid`, zeros from there on.  V = elements per 16 source bytes.
template <typename T, int V>
__device__ __forceinline__ void move_piece(const T* __restrict__ s, float* __restrict__ d, int64_t valid, int64_t lo, int64_t hi,
                                           bool first_piece, int head, bool vec_ok) {
  const int tid = threadIdx.x;
  const int64_t copy_end = hi < valid ? hi : valid;
  int64_t a = lo;
  if (vec_ok) {
    if (first_piece) {   // (lo == 0) elements before the source's first 16-byte boundary
      if (tid < head && tid < copy_end) d[tid] = src_at(s, tid);
      a = head;
    }
    if (copy_end > a) {
      const int64_t nv = (copy_end - a) / V;
      for (int64_t v = tid; v < nv; v += NT) move16(s + a + v * V, d + a + v * V);
      a += nv * V;
    }
  }
  for (int64_t j = a + tid; j < copy_end; j += NT) d[j] = src_at(s, j);
  for (int64_t j = (lo > valid ? lo : valid) + tid; j < hi; j += NT) d[j] = 0.0f;
}

__global__ __launch_bounds__(NT) void gather_batch_kernel(const GatherArgs args, const int64_t* __restrict__ index, int64_t n) {
  __shared__ float pal[16];
  __shared__ uint4 stage[NT];                     // a coded piece's 16-byte accesses, turned for the stores
  const int blk = args.batch > 0 ? (int)(blockIdx.x / (unsigned)args.batch) : (int)blockIdx.x;
  const int b = args.batch > 0 ? (int)(blockIdx.x % (unsigned)args.batch) : (int)blockIdx.y;
  int k = 0;
  for (int i = 1; i < args.n_fields; ++i)
    if (blk >= args.first_block[i]) k = i;
  const mmfn_gather_field& F = args.f[k];
  const int piece = blk - args.first_block[k];
  int64_t i = index[b];
  i = i < 0 ? 0 : (i >= n ? n - 1 : i);          // the loader checks its indices on the host; never read outside the store
  int64_t valid, total, src0;
  if (F.row_off) {
    const int64_t o0 = F.row_off[i];
    int64_t c = F.row_off[i + 1] - o0;
    if (piece == 0 && threadIdx.x == 0 && F.count_out) F.count_out[b] = (int32_t)c;
    c = c < 0 ? 0 : (c > F.lmax ? (int64_t)F.lmax : c);
    valid = c * F.row_elems;
    total = (int64_t)F.lmax * F.row_elems;
    src0 = o0 * F.row_elems;
  } else {
    valid = total = F.row_elems;
    src0 = i * F.row_elems;
  }
  float* d = F.dst + (int64_t)b * F.dst_stride + F.dst_offset;
  if (F.src_type == MMFN_GATHER_PAL4) {           // dense only (the host refuses row_off): row i is row_elems / 2 bytes
    const int64_t nb = F.row_elems >> 1;
    const uint8_t* s = reinterpret_cast<const uint8_t*>(F.src) + i * nb;
    const int head = (int)((16 - ((uintptr_t)s & 15)) & 15);
    const bool vec_ok = (((uintptr_t)(d + 2 * head)) & 15) == 0;
    const int64_t lo = piece == 0 ? 0 : head + (int64_t)piece * PIECE_BYTES_PAL4;
    int64_t hi = head + (int64_t)(piece + 1) * PIECE_BYTES_PAL4;
    if (lo >= nb) return;                         // (the same for every lane of the workgroup)
    if (hi > nb) hi = nb;
    move_piece_pal4(s, d, F.palette, pal, stage, lo, hi, piece == 0, head, vec_ok);
    return;
  }
  const int esz = F.src_type == MMFN_GATHER_U8 ? 1 : 4;
  const int64_t per = PIECE_BYTES / esz;          // elements per piece
  const uintptr_t sa = (uintptr_t)F.src + (uintptr_t)src0 * esz;
  const int head = (int)(((16 - (sa & 15)) & 15) / esz);
  const bool vec_ok = (((uintptr_t)(d + head)) & 15) == 0;
  // piece p covers [p == 0 ? 0 : head + p * per, head + (p + 1) * per) of the row, so every piece but the first starts on a
  // 16-byte boundary of the source
  const int64_t lo = piece == 0 ? 0 : head + (int64_t)piece * per;
  int64_t hi = head + (int64_t)(piece + 1) * per;
  if (lo >= total) return;
  if (hi > total) hi = total;
  if (F.src_type == MMFN_GATHER_U8)
    move_piece<uint8_t, 16>(reinterpret_cast<const uint8_t*>(F.src) + src0, d, valid, lo, hi, piece == 0, head, vec_ok);
  else
    move_piece<float, 4>(reinterpret_cast<const float*>(F.src) + src0, d, valid, lo, hi, piece == 0, head, vec_ok);
}

// ---- camera colour jitter inside the gather (mmfn_gather_camera_jitter; formulas and draws: include/mmfn_hip.h) ------------------
// The traffic of the plain gather of the camera field.  A workgroup owns 2048 consecutive pixels of ONE (sample, frame); a lane owns
// 4 consecutive pixels per access: it loads them from each of the three channel planes (u8: three 4-byte loads, f32: three 16-byte
// loads), so saturation has R, G and B of a pixel in registers, and writes three 16-byte stores - the lanes of a store are adjacent,
// a wave's store covers 1 KB in one run.  (A lane owning 16 u8 pixels - one 16-byte load per plane, twelve stores with the lanes
// 64 bytes apart, 4096 pixels per workgroup - measured 14.4 us for the camera field at batch 32 against 10.5 us this way and
// 15.5 us for the plain gather launched on that field alone; profiles/resident_jitter_bench.txt.)
// The frame's scalars - sample, draws, factors, rectangle, row and column of the piece's first pixel (the one 64-bit division) -
// are the same in every lane: each lane works them out from scalar loads, no LDS and no barrier, so the pixel loads do not wait
// behind them.  A lane finds its row and column from there with one 32-bit division per access, and only in a frame that is erased.
constexpr int64_t JITTER_PIECE = (int64_t)NT * 8;   // pixels per workgroup

struct JitterFrame {
  float m, fc, fb, fs, tc;     // gray mean, the three factors, (1 - fc) * m
  int32_t erase;               // 0: this sample keeps every pixel
  int32_t y0, y1, x0, x1;      // the erased rectangle [y0, y1) x [x0, x1)
  int32_t row;                 // row and column of the piece's first pixel
  uint32_t col;
};

__device__ __forceinline__ float clamp255(float x) { return fminf(fmaxf(x, 0.0f), 255.0f); }

template <bool ERASE>
__device__ __forceinline__ void jitter_pixel(const JitterFrame& F, float& r, float& g, float& b, int32_t y, uint32_t x) {
  r = clamp255(fmaf(F.fc, r, F.tc));
  g = clamp255(fmaf(F.fc, g, F.tc));
  b = clamp255(fmaf(F.fc, b, F.tc));
  r = clamp255(F.fb * r);
  g = clamp255(F.fb * g);
  b = clamp255(F.fb * b);
  const float ts = (1.0f - F.fs) * fmaf(0.114f, b, fmaf(0.587f, g, 0.299f * r));
  r = clamp255(fmaf(F.fs, r, ts));
  g = clamp255(fmaf(F.fs, g, ts));
  b = clamp255(fmaf(F.fs, b, ts));
  if (ERASE && y >= F.y0 && y < F.y1 && (int32_t)x >= F.x0 && (int32_t)x < F.x1) r = g = b = F.m;
}

// row / column of pixel j >= lo of the piece that starts at pixel lo = (F.row, F.col): j - lo < 2048 + 16 and F.col < W < 2^31
__device__ __forceinline__ void jitter_pos(const JitterFrame& F, uint32_t W, int64_t j, int64_t lo, int32_t& y, uint32_t& x) {
  const uint32_t c = F.col + (uint32_t)(j - lo);
  const uint32_t q = c / W;
  y = F.row + (int32_t)q;
  x = c - q * W;
}
__device__ __forceinline__ void jitter_next(uint32_t W, int32_t& y, uint32_t& x) {
  if (++x == W) { x = 0; ++y; }
}

// 4 consecutive pixels of the three planes at s, s + HW, s + 2 HW -> d, d + HW, d + 2 HW; (y, x) = row and column of the first
template <bool ERASE>
__device__ __forceinline__ void jitter_vec(const JitterFrame& F, const uint8_t* s, float* d, int64_t HW, int32_t y, uint32_t x, uint32_t W) {
  const uint32_t wr = *reinterpret_cast<const uint32_t*>(s), wg = *reinterpret_cast<const uint32_t*>(s + HW),
                 wb = *reinterpret_cast<const uint32_t*>(s + 2 * HW);
  f32x4 vr, vg, vb;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float r = (float)((wr >> (8 * e)) & 0xffu), g = (float)((wg >> (8 * e)) & 0xffu), b = (float)((wb >> (8 * e)) & 0xffu);
    jitter_pixel<ERASE>(F, r, g, b, y, x);
    if (ERASE) jitter_next(W, y, x);
    vr[e] = r; vg[e] = g; vb[e] = b;
  }
  *reinterpret_cast<f32x4*>(d) = vr;
  *reinterpret_cast<f32x4*>(d + HW) = vg;
  *reinterpret_cast<f32x4*>(d + 2 * HW) = vb;
}
template <bool ERASE>
__device__ __forceinline__ void jitter_vec(const JitterFrame& F, const float* s, float* d, int64_t HW, int32_t y, uint32_t x, uint32_t W) {
  f32x4 vr = *reinterpret_cast<const f32x4*>(s), vg = *reinterpret_cast<const f32x4*>(s + HW), vb = *reinterpret_cast<const f32x4*>(s + 2 * HW);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float r = vr[e], g = vg[e], b = vb[e];
    jitter_pixel<ERASE>(F, r, g, b, y, x);
    if (ERASE) jitter_next(W, y, x);
    vr[e] = r; vg[e] = g; vb[e] = b;
  }
  *reinterpret_cast<f32x4*>(d) = vr;
  *reinterpret_cast<f32x4*>(d + HW) = vg;
  *reinterpret_cast<f32x4*>(d + 2 * HW) = vb;
}

// pixels [lo, hi) of one frame: s, d = its first plane; the planes are HW elements apart.  head = pixels before the planes' first
// vector boundary (4 bytes for u8, 16 for f32), vec_ok = the planes and the destination are aligned alike from there on.
template <typename T, bool ERASE>
__device__ __forceinline__ void jitter_piece(const JitterFrame& F, const T* __restrict__ s, float* __restrict__ d, int64_t HW, uint32_t W,
                                             int64_t lo, int64_t hi, bool first_piece, int head, bool vec_ok) {
  const int tid = threadIdx.x;
  auto one = [&](int64_t j) {
    float r = src_at(s, j), g = src_at(s, j + HW), b = src_at(s, j + 2 * HW);
    int32_t y = 0;
    uint32_t x = 0;
    if (ERASE) jitter_pos(F, W, j, lo, y, x);
    jitter_pixel<ERASE>(F, r, g, b, y, x);
    d[j] = r; d[j + HW] = g; d[j + 2 * HW] = b;
  };
  int64_t a = lo;
  if (vec_ok) {
    if (first_piece) {   // (lo == 0)
      if (tid < head && tid < hi) one(tid);
      a = head;
    }
    if (hi > a) {
      const int64_t nv = (hi - a) / 4;
      for (int64_t v = tid; v < nv; v += NT) {
        const int64_t j = a + v * 4;
        int32_t y = 0;
        uint32_t x = 0;
        if (ERASE) jitter_pos(F, W, j, lo, y, x);
        jitter_vec<ERASE>(F, s + j, d + j, HW, y, x, W);
      }
      a += nv * 4;
    }
  }
  for (int64_t j = a + tid; j < hi; j += NT) one(j);
}

__global__ __launch_bounds__(NT) void camera_jitter_kernel(const mmfn_camera_jitter_desc D, const int64_t* __restrict__ index, int64_t n) {
  const int piece = (int)blockIdx.x, b = (int)blockIdx.y, s = (int)blockIdx.z, S = D.n_frames;
  const int64_t HW = (int64_t)D.H * D.W, frame = 3 * HW;
  const int esz = D.src_type == MMFN_GATHER_U8 ? 1 : 4;
  const int align = D.src_type == MMFN_GATHER_U8 ? 4 : 16;   // bytes of a lane's load
  JitterFrame F;                                             // (the same in every lane)
  int64_t i = index[b];
  i = i < 0 ? 0 : (i >= n ? n - 1 : i);
  const uint64_t id = (uint64_t)(D.sample_id ? D.sample_id[i] : i);
  const uint64_t key = mmfn_rng_key(D.state, MMFN_RNG_STREAM_JITTER);
  uint32_t k[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) k[j] = mmfn_rng_u32(key, id * 8 + j) >> 8;
  const float m = D.gray_mean[i * S + s];
  F.m = m;
  F.fb = fmaf(D.brightness, fmaf(2.0f, (float)k[0] * (1.0f / 16777216.0f), -1.0f), 1.0f);
  F.fc = fmaf(D.contrast, fmaf(2.0f, (float)k[1] * (1.0f / 16777216.0f), -1.0f), 1.0f);
  F.fs = fmaf(D.saturation, fmaf(2.0f, (float)k[2] * (1.0f / 16777216.0f), -1.0f), 1.0f);
  F.tc = (1.0f - F.fc) * m;
  F.erase = k[3] < D.erase_thresh;
  F.y0 = F.y1 = F.x0 = F.x1 = F.row = 0;
  F.col = 0;
  if (F.erase) {
    const int32_t h = D.erase_h_min + (int32_t)(((uint64_t)k[4] * (uint64_t)(D.erase_h_max - D.erase_h_min + 1)) >> 24);
    const int32_t w = D.erase_w_min + (int32_t)(((uint64_t)k[5] * (uint64_t)(D.erase_w_max - D.erase_w_min + 1)) >> 24);
    F.y0 = (int32_t)(((uint64_t)k[7] * (uint64_t)(D.H - h + 1)) >> 24);
    F.x0 = (int32_t)(((uint64_t)k[6] * (uint64_t)(D.W - w + 1)) >> 24);
    F.y1 = F.y0 + h;
    F.x1 = F.x0 + w;
    if (piece) {   // the piece's first pixel, as computed below
      const uintptr_t sa0 = (uintptr_t)D.src[s] + (uintptr_t)(i * frame) * esz;
      const int64_t lo0 = (int64_t)(((align - (sa0 & (align - 1))) & (align - 1)) / esz) + (int64_t)piece * JITTER_PIECE;
      F.row = (int32_t)(lo0 / D.W);
      F.col = (uint32_t)(lo0 % D.W);
    }
  }
  const JitterFrame& f = F;
  float* d = D.dst + ((int64_t)b * S + s) * frame;
  const uintptr_t sa = (uintptr_t)D.src[s] + (uintptr_t)(i * frame) * esz;
  const int head = (int)(((align - (sa & (align - 1))) & (align - 1)) / esz);
  // vector accesses need the three source planes misaligned alike and the destination planes too (HW a multiple of 4 gives
  // both), and the destination on a 16-byte boundary where the source is on its own
  const bool vec_ok = HW % 4 == 0 && (((uintptr_t)(d + head)) & 15) == 0;
  const int64_t lo = piece == 0 ? 0 : head + (int64_t)piece * JITTER_PIECE;
  int64_t hi = head + (int64_t)(piece + 1) * JITTER_PIECE;
  if (lo >= HW) return;
  if (hi > HW) hi = HW;
  const uint32_t W = (uint32_t)D.W;
  if (D.src_type == MMFN_GATHER_U8) {
    const uint8_t* src = reinterpret_cast<const uint8_t*>(D.src[s]) + i * frame;
    if (f.erase) jitter_piece<uint8_t, true>(f, src, d, HW, W, lo, hi, piece == 0, head, vec_ok);
    else jitter_piece<uint8_t, false>(f, src, d, HW, W, lo, hi, piece == 0, head, vec_ok);
  } else {
    const float* src = reinterpret_cast<const float*>(D.src[s]) + i * frame;
    if (f.erase) jitter_piece<float, true>(f, src, d, HW, W, lo, hi, piece == 0, head, vec_ok);
    else jitter_piece<float, false>(f, src, d, HW, W, lo, hi, piece == 0, head, vec_ok);
  }
}

// ---- LiDAR dropout, lane dropout and map noise inside the gather (mmfn_gather_augment; draws and formulas: include/mmfn_hip.h) ---
// The traffic of the plain gather of these fields, which leave its table.  Workgroups [0, S * pieces) of a sample own a piece of ONE
// LiDAR (sample, frame) row, cut as gather_batch_kernel cuts it (16 KB of f32 / u8 source, 4 KB of codes through the same LDS turn)
// and masked in registers between load and store: a hash per element for the cell dropout, a rectangle test for the erasure.  The
// frame's scalars are the same in every lane, worked out from scalar loads as in the jitter.  An element's (y, x) is needed in an
// erased sample only: the offset of the piece's first element in its [H, W] plane is one 64-bit division per workgroup, a lane adds
// its distance from there, steps back by H * W where that runs past the plane's end (a piece is no longer than a plane; a plane
// shorter than a piece takes a 32-bit remainder instead) and divides by W once per access.
// The first workgroup of a sample owns its lane set and its target point (first, so that its chain of dependent loads runs beside
// the LiDAR pieces and not after them): keep bits of 256 lanes at a time, a prefix sum over the
// workgroup (ballot per wave, the waves' counts through LDS) that writes the kept lanes' numbers into a map in LDS, then one node
// (five floats) per lane and step through the kept lanes, then the zero rows.  A few KB per sample.
constexpr int AUG_MAX_LANES = MMFN_AUGMENT_MAX_LANES;

struct AugmentGrid {
  int32_t map_blocks;    // 1: workgroup 0 of a sample is its map workgroup (lane set, target point); 0: no such part
  int32_t pieces;        // workgroups per LiDAR (sample, frame) row; n_frames * pieces of them follow
  int32_t batch;
};

struct LidarFrame {
  uint64_t key, base;          // key of the element draws; id * C * H * W
  uint32_t cell_thresh;
  int32_t erase;               // 0: no rectangle in this sample
  uint32_t y0, y1, x0, x1;     // the erased rectangle [y0, y1) x [x0, x1)
  uint32_t H, W, HW;
  uint32_t p0;                 // offset of the piece's first element in its plane
  int32_t wrap_once;           // H * W >= a piece's elements: p0 + distance passes the plane's end at most once
};

// row / column of element j >= lo of the piece whose first element lo sits at plane offset F.p0: j - lo < 16 K + 32, HW < 2^31
__device__ __forceinline__ void lidar_pos(const LidarFrame& F, int64_t j, int64_t lo, uint32_t& y, uint32_t& x) {
  uint32_t p = F.p0 + (uint32_t)(j - lo);
  if (F.wrap_once) {
    if (p >= F.HW) p -= F.HW;
  } else {
    p %= F.HW;
  }
  const uint32_t q = p / F.W;
  y = q;
  x = p - q * F.W;
}
__device__ __forceinline__ void lidar_next(const LidarFrame& F, uint32_t& y, uint32_t& x) {
  if (++x == F.W) {
    x = 0;
    if (++y == F.H) y = 0;
  }
}
// element e of the row, value v, at (y, x) of its plane: v's bits, or +0.0
__device__ __forceinline__ float lidar_mask(const LidarFrame& F, float v, int64_t e, uint32_t y, uint32_t x) {
  bool drop = F.erase && y >= F.y0 && y < F.y1 && x >= F.x0 && x < F.x1;
  if (F.cell_thresh) drop |= (mmfn_rng_u32(F.key, F.base + (uint64_t)e) >> 8) < F.cell_thresh;
  return drop ? 0.0f : v;
}

// V consecutive elements from row element j on, at s -> d
__device__ __forceinline__ void lidar_vec(const LidarFrame& F, const float* s, float* d, int64_t j, uint32_t y, uint32_t x) {
  f32x4 v = *reinterpret_cast<const f32x4*>(s);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = lidar_mask(F, v[e], j + e, y, x);
    if (F.erase) lidar_next(F, y, x);
  }
  *reinterpret_cast<f32x4*>(d) = v;
}
__device__ __forceinline__ void lidar_vec(const LidarFrame& F, const uint8_t* s, float* d, int64_t j, uint32_t y, uint32_t x) {
  const uint4 u = *reinterpret_cast<const uint4*>(s);
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = lidar_mask(F, (float)((w[k] >> (8 * e)) & 0xffu), j + 4 * k + e, y, x);
      if (F.erase) lidar_next(F, y, x);
    }
    *reinterpret_cast<f32x4*>(d + 4 * k) = v;
  }
}

// elements [lo, hi) of one LiDAR row: move_piece with the mask between load and store (a dense row: nothing to zero-fill)
template <typename T, int V>
__device__ __forceinline__ void lidar_piece(const LidarFrame& F, const T* __restrict__ s, float* __restrict__ d, int64_t lo, int64_t hi,
                                            bool first_piece, int head, bool vec_ok) {
  const int tid = threadIdx.x;
  auto one = [&](int64_t j) {
    uint32_t y = 0, x = 0;
    if (F.erase) lidar_pos(F, j, lo, y, x);
    d[j] = lidar_mask(F, src_at(s, j), j, y, x);
  };
  int64_t a = lo;
  if (vec_ok) {
    if (first_piece) {   // (lo == 0)
      if (tid < head && tid < hi) one(tid);
      a = head;
    }
    if (hi > a) {
      const int64_t nv = (hi - a) / V;
      for (int64_t v = tid; v < nv; v += NT) {
        const int64_t j = a + v * V;
        uint32_t y = 0, x = 0;
        if (F.erase) lidar_pos(F, j, lo, y, x);
        lidar_vec(F, s + j, d + j, j, y, x);
      }
      a += nv * V;
    }
  }
  for (int64_t j = a + tid; j < hi; j += NT) one(j);
}

// source BYTES [lo, hi) of one coded LiDAR row: move_piece_pal4 with the mask after the palette lookup; F.p0 belongs to element 2 lo
__device__ __forceinline__ void lidar_piece_pal4(const LidarFrame& F, const uint8_t* __restrict__ s, float* __restrict__ d,
                                                 const float* __restrict__ palette, float* pal, uint4* stage, int64_t lo, int64_t hi,
                                                 bool first_piece, int head, bool vec_ok) {
  const int tid = threadIdx.x;
  auto one = [&](int64_t j) {   // byte j: elements 2 j and 2 j + 1
    const uint32_t c = s[j];
    uint32_t y = 0, x = 0;
    if (F.erase) lidar_pos(F, 2 * j, 2 * lo, y, x);
    d[2 * j] = lidar_mask(F, pal[c & 15u], 2 * j, y, x);
    if (F.erase) lidar_next(F, y, x);
    d[2 * j + 1] = lidar_mask(F, pal[(c >> 4) & 15u], 2 * j + 1, y, x);
  };
  int64_t a = lo;
  int nv = 0;                                       // 16-byte accesses of this piece: 0..NT, the same for every lane
  if (vec_ok) {
    if (first_piece) a = head;
    if (hi > a) nv = (int)((hi - a) / 16);
  }
  if (tid < 16) pal[tid] = palette[tid];
  if (tid < nv) stage[tid] = *reinterpret_cast<const uint4*>(s + a + (int64_t)tid * 16);
  __syncthreads();
  if (vec_ok) {
    if (first_piece && tid < head && tid < hi) one(tid);
    const uint16_t* codes = reinterpret_cast<const uint16_t*>(stage);
    const int base = (tid >> 6) * 1024 + 2 * (tid & 63);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int byte = base + 128 * k;              // even, and nv * 16 is too: byte + 1 is inside as well
      if (byte < nv * 16) {
        const uint32_t c = codes[byte >> 1];
        const int64_t j = 2 * (a + byte);
        uint32_t y = 0, x = 0;
        if (F.erase) lidar_pos(F, j, 2 * lo, y, x);
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = lidar_mask(F, pal[(c >> (4 * e)) & 15u], j + e, y, x);
          if (F.erase) lidar_next(F, y, x);
        }
        *reinterpret_cast<f32x4*>(d + j) = v;
      }
    }
    a += (int64_t)nv * 16;
  }
  for (int64_t j = a + tid; j < hi; j += NT) one(j);
}

__device__ __forceinline__ float draw_pm1(uint32_t k) { return fmaf(2.0f, (float)k * (1.0f / 16777216.0f), -1.0f); }

// the lane set and the target point of batch sample b = store row i, global id `id`: every thread of the workgroup calls this
__device__ __forceinline__ void map_block(const mmfn_gather_augment_desc& D, int b, int64_t i, uint64_t id, uint16_t* kept_lane,
                                          int* wave_count, float* rigid) {
  const int tid = threadIdx.x;
  const uint64_t key = mmfn_rng_key(D.map_state, MMFN_RNG_STREAM_MAP);
  if ((D.parts & MMFN_AUGMENT_TARGET) && tid < 2) {
    const float t = D.target_src[i * 2 + tid];
    const float w = draw_pm1(mmfn_rng_u32(key, id * 8 + 3 + tid) >> 8);
    D.target_dst[(int64_t)b * 2 + tid] = D.target_shift != 0.0f ? fmaf(D.target_shift, w, t) : t;
  }
  if (!(D.parts & MMFN_AUGMENT_LANES)) return;      // (the same for every lane of the workgroup)
  const bool moved = D.shift != 0.0f || D.yaw_rad != 0.0f;
  if (tid == 0 && moved) {                          // once per workgroup: the library's sinf / cosf are not short
    const float theta = D.yaw_rad * draw_pm1(mmfn_rng_u32(key, id * 8 + 2) >> 8);
    rigid[0] = cosf(theta);
    rigid[1] = sinf(theta);
    rigid[2] = D.shift * draw_pm1(mmfn_rng_u32(key, id * 8 + 0) >> 8);
    rigid[3] = D.shift * draw_pm1(mmfn_rng_u32(key, id * 8 + 1) >> 8);
  }
  const int64_t o0 = D.lane_row_off[i];
  const int64_t stored = D.lane_row_off[i + 1] - o0;
  const int rows = (int)(stored < 0 ? 0 : (stored > D.lmax ? (int64_t)D.lmax : stored));
  // the kept-lane map: kept_lane[r] = stored lane that lands at destination row r
  const uint64_t lane_key = mmfn_rng_key(D.map_state, MMFN_RNG_STREAM_LANE);
  int kept = 0;
  for (int j0 = 0; j0 < rows; j0 += NT) {
    const int j = j0 + tid;
    const bool keep = j < rows && (j == 0 || !((mmfn_rng_u32(lane_key, id * 65536 + (uint64_t)j) >> 8) < D.lane_thresh));
    const uint64_t wave_keep = __ballot(keep);
    if ((tid & 63) == 0) wave_count[tid >> 6] = __popcll(wave_keep);
    __syncthreads();
    int before = kept, all = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
      const int c = wave_count[w];
      if (w < (tid >> 6)) before += c;
      all += c;
    }
    if (keep) kept_lane[before + __popcll(wave_keep & ((1ull << (tid & 63)) - 1ull))] = (uint16_t)j;
    kept += all;
    __syncthreads();                                // wave_count is rewritten in the next round; kept_lane and rigid are read below
  }
  if (rows == 0) __syncthreads();                   // (rigid)
  if (tid == 0 && D.lane_count_out) D.lane_count_out[b] = (int32_t)(stored - (rows - kept));
  const float c = moved ? rigid[0] : 1.0f, s = moved ? rigid[1] : 0.0f, tx = moved ? rigid[2] : 0.0f, ty = moved ? rigid[3] : 0.0f;
  const int nodes = D.lane_nodes;
  const int64_t row_elems = (int64_t)nodes * 5;
  float* d = D.lane_dst + (int64_t)b * D.lmax * row_elems;
  const float* src = D.lane_src + o0 * row_elems;
  const int n_nodes = kept * nodes;                 // <= 4096 * lane_nodes, checked on the host to fit 31 bits
  for (int e = tid; e < n_nodes; e += NT) {
    const int r = e / nodes, nd = e - r * nodes;
    const float* p = src + (int64_t)kept_lane[r] * row_elems + nd * 5;
    float* q = d + (int64_t)e * 5;
    float x = p[0], y = p[1];
    const float f2 = p[2], f3 = p[3], f4 = p[4];
    if (moved && !(x == 0.0f && y == 0.0f && f2 == 0.0f && f3 == 0.0f && f4 == 0.0f)) {   // an all-zero node is padding
      const float xr = fmaf(c, x, fmaf(-s, y, tx));
      y = fmaf(s, x, fmaf(c, y, ty));
      x = xr;
    }
    q[0] = x; q[1] = y; q[2] = f2; q[3] = f3; q[4] = f4;
  }
  const int64_t total = (int64_t)D.lmax * row_elems;
  for (int64_t j = (int64_t)kept * row_elems + tid; j < total; j += NT) d[j] = 0.0f;
}

__global__ __launch_bounds__(NT) void gather_augment_kernel(const mmfn_gather_augment_desc D, const AugmentGrid G,
                                                            const int64_t* __restrict__ index, int64_t n) {
  __shared__ float pal[16];
  __shared__ uint4 stage[NT];                     // a coded piece's 16-byte accesses, turned for the stores
  __shared__ uint16_t kept_lane[AUG_MAX_LANES];
  __shared__ int wave_count[NT / 64];
  __shared__ float rigid[4];
  int blk = (int)(blockIdx.x / (unsigned)G.batch);
  const int b = (int)(blockIdx.x % (unsigned)G.batch);                                                // the sample is the fastest index
  int64_t i = index[b];
  i = i < 0 ? 0 : (i >= n ? n - 1 : i);
  const uint64_t id = (uint64_t)(D.sample_id ? D.sample_id[i] : i);
  if (blk < G.map_blocks) {
    map_block(D, b, i, id, kept_lane, wave_count, rigid);
    return;
  }
  blk -= G.map_blocks;
  const int s = blk / G.pieces, piece = blk - s * G.pieces, S = D.n_frames;
  const int64_t HW = (int64_t)D.H * D.W, row = HW * D.C;
  const int esz = D.src_type == MMFN_GATHER_F32 ? 4 : 1;
  const bool pal4 = D.src_type == MMFN_GATHER_PAL4;
  // in BYTES of the source (PAL4: a byte is two elements), as gather_batch_kernel cuts its rows
  const int64_t per = pal4 ? PIECE_BYTES_PAL4 : PIECE_BYTES / esz;
  const int64_t total = pal4 ? row >> 1 : row;
  const uintptr_t sa = (uintptr_t)D.lidar_src[s] + (uintptr_t)(i * total) * esz;
  const int head = (int)(((16 - (sa & 15)) & 15) / esz);
  float* d = D.lidar_dst + ((int64_t)b * S + s) * row;
  const bool vec_ok = (((uintptr_t)(d + (pal4 ? 2 * head : head))) & 15) == 0;
  const int64_t lo = piece == 0 ? 0 : head + (int64_t)piece * per;
  int64_t hi = head + (int64_t)(piece + 1) * per;
  if (lo >= total) return;                        // (the same for every lane of the workgroup)
  if (hi > total) hi = total;
  LidarFrame F;                                   // (the same in every lane)
  F.key = mmfn_rng_key(D.lidar_state, MMFN_RNG_STREAM_LIDAR_CELL);
  F.base = id * (uint64_t)row;
  F.cell_thresh = D.cell_thresh;
  F.H = (uint32_t)D.H; F.W = (uint32_t)D.W; F.HW = (uint32_t)HW;
  F.y0 = F.y1 = F.x0 = F.x1 = F.p0 = 0;
  F.wrap_once = HW >= (pal4 ? 2 * per : per) + 32;
  const uint64_t key = mmfn_rng_key(D.lidar_state, MMFN_RNG_STREAM_LIDAR);
  F.erase = (mmfn_rng_u32(key, id * 8 + 3) >> 8) < D.erase_thresh;
  if (F.erase) {
    uint32_t k[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = mmfn_rng_u32(key, id * 8 + 4 + j) >> 8;
    const uint32_t h = (uint32_t)D.erase_h_min + (uint32_t)(((uint64_t)k[0] * (uint64_t)(D.erase_h_max - D.erase_h_min + 1)) >> 24);
    const uint32_t w = (uint32_t)D.erase_w_min + (uint32_t)(((uint64_t)k[1] * (uint64_t)(D.erase_w_max - D.erase_w_min + 1)) >> 24);
    F.y0 = (uint32_t)(((uint64_t)k[3] * (uint64_t)(F.H - h + 1)) >> 24);
    F.x0 = (uint32_t)(((uint64_t)k[2] * (uint64_t)(F.W - w + 1)) >> 24);
    F.y1 = F.y0 + h;
    F.x1 = F.x0 + w;
    F.p0 = (uint32_t)((pal4 ? 2 * lo : lo) % HW);
  }
  const LidarFrame& f = F;
  if (pal4)
    lidar_piece_pal4(f, reinterpret_cast<const uint8_t*>(D.lidar_src[s]) + i * total, d, D.lidar_palette[s], pal, stage, lo, hi, piece == 0,
                     head, vec_ok);
  else if (D.src_type == MMFN_GATHER_U8)
    lidar_piece<uint8_t, 16>(f, reinterpret_cast<const uint8_t*>(D.lidar_src[s]) + i * row, d, lo, hi, piece == 0, head, vec_ok);
  else
    lidar_piece<float, 4>(f, reinterpret_cast<const float*>(D.lidar_src[s]) + i * row, d, lo, hi, piece == 0, head, vec_ok);
}

// ---- camera degradation inside the gather (mmfn_gather_camera_degrade; draws and formulas: include/mmfn_hip.h) -------------------
// The jitter launch with a hue shift, a Gaussian blur and sensor noise between the blends and the erased rectangle.  Whether a
// sample is blurred is its own draw, the same in every lane of a workgroup, so a workgroup branches once:
//   unblurred  the jitter's pointwise path (2048 consecutive pixels of one frame, four pixels per access), hue and noise in
//              registers between the blends and the rectangle: no halo, no LDS traffic, no barrier.
//   blurred    a BLUR_TH x BLUR_TW tile of one frame.  The tile plus an R-wide halo of all three planes is loaded element by
//              element (consecutive lanes on consecutive pixels of a row: the halo's start is not aligned to anything), mirrored
//              at the frame's border, blended and hue-shifted on the way into LDS - hue needs R, G and B of a pixel together,
//              and the filter must see the neighbours' shifted values.  A lane has the loads of four pixels in flight: with one
//              pixel at a time (a wave per row) the launch measured 73.4 us at B = 32 with every sample blurred, this way
//              50.3 us (profiles/resident_degrade_bench.txt).  Then per plane: rows filtered out of that image into a second LDS
//              buffer (a lane per column, taps d and -d paired: R + 1 multiplies), columns filtered out of it four pixels per
//              lane (16-byte LDS reads), noise, rectangle, and one 16-byte store where the four pixels are inside the frame and
//              the address allows, element stores otherwise.
// Tile: 32 x 64 pixels.  Image (32 + 16) x (64 + 16) x 3 planes = 45 KB at the largest radius 8, plus ONE plane of row-filtered
// values 48 x 64 = 12 KB (reused by the three planes, two barriers each): 57 KB, so two workgroups share a compute unit's 160 KB
// with room to spare, and the halo costs 1.9 x the tile's own loads and blends.  (16 x 64 would fit four workgroups but load
// 2.5 x; 64 x 64 loads 1.6 x but is alone on its compute unit.)  Rows of both buffers are read along x by consecutive lanes: no
// bank conflicts.  The LDS is dynamic, so a launch whose blur probability is 0 asks for none and keeps the jitter's occupancy;
// a launch that may blur gives it to every workgroup, blurred or not.
// The taps are worked out by lanes 0..R (one expf each) and normalised by every lane from LDS in one fixed order; the frame's
// other scalars come from scalar loads as in the jitter.
constexpr int BLUR_TH = 32, BLUR_TW = 64, BLUR_RMAX = MMFN_DEGRADE_MAX_RADIUS;
constexpr int BLUR_IN_H = BLUR_TH + 2 * BLUR_RMAX, BLUR_IN_W = BLUR_TW + 2 * BLUR_RMAX;
constexpr int BLUR_PLANE = BLUR_IN_H * BLUR_IN_W;                    // floats of one plane's image
constexpr int BLUR_MID = BLUR_IN_H * BLUR_TW;                        // floats of the row-filtered plane
constexpr int BLUR_LOADS = 4;                                        // pixels a lane has in flight while the image is loaded
constexpr size_t BLUR_LDS_BYTES = (size_t)(3 * BLUR_PLANE + BLUR_MID + 16) * sizeof(float);   // (+ the taps)

struct DegradeFrame {
  JitterFrame j;
  int32_t hue, noise;          // 0: the stage is off for this launch / this sample
  float shift;                 // hue shift, in turns
  float noise_std;
  uint64_t noise_key, noise_base;   // key of the element draws; (id * S + s) * 3 H W
};

__device__ __forceinline__ void hue_pixel(float shift, float& r, float& g, float& b) {
  const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
  const float c = mx - mn;
  const bool gray = mx == mn;
  const float s = c / (gray ? 1.0f : mx);
  const float inv = 1.0f / (gray ? 1.0f : c);
  const float rc = (mx - r) * inv, gc = (mx - g) * inv, bc = (mx - b) * inv;
  const float h6 = mx == r ? bc - gc : (mx == g ? 2.0f + rc - bc : 4.0f + gc - rc);
  float h = fmaf(h6, 1.0f / 6.0f, shift);
  h -= floorf(h);
  const float hs = h * 6.0f, fl = floorf(hs), f = hs - fl;
  int sector = (int)fl;
  if (sector >= 6) sector -= 6;                    // (h rounded up to 1)
  const float p = clamp255(mx * (1.0f - s)), q = clamp255(mx * (1.0f - s * f)), t = clamp255(mx * (1.0f - s * (1.0f - f)));
  r = sector == 0 || sector == 5 ? mx : (sector == 1 ? q : (sector == 4 ? t : p));
  g = sector == 1 || sector == 2 ? mx : (sector == 0 ? t : (sector == 3 ? q : p));
  b = sector == 3 || sector == 4 ? mx : (sector == 2 ? t : (sector == 5 ? q : p));
}

// element e of the frame (e = (c * H + y) * W + x), value v
__device__ __forceinline__ float degrade_noise(const DegradeFrame& F, float v, uint64_t e) {
  const uint64_t q = F.noise_base + e;
  const uint32_t n0 = mmfn_rng_u32(F.noise_key, 2 * q) >> 8, n1 = mmfn_rng_u32(F.noise_key, 2 * q + 1) >> 8;
  const float u1 = (float)(n0 + 1u) * (1.0f / 16777216.0f), u2 = (float)n1 * (1.0f / 16777216.0f);
  return clamp255(fmaf(F.noise_std, sqrtf(-2.0f * logf(u1)) * cosf(6.2831855f * u2), v));
}

// one pixel of the pointwise path: j = its offset in the plane, inside = it lies in the erased rectangle
__device__ __forceinline__ void degrade_pixel(const DegradeFrame& F, float& r, float& g, float& b, int64_t j, int64_t HW, bool inside) {
  jitter_pixel<false>(F.j, r, g, b, 0, 0);
  if (F.hue) hue_pixel(F.shift, r, g, b);
  if (F.noise) {
    r = degrade_noise(F, r, (uint64_t)j);
    g = degrade_noise(F, g, (uint64_t)(HW + j));
    b = degrade_noise(F, b, (uint64_t)(2 * HW + j));
  }
  if (inside) r = g = b = F.j.m;
}
__device__ __forceinline__ bool in_rect(const JitterFrame& F, int64_t y, int64_t x) { return y >= F.y0 && y < F.y1 && x >= F.x0 && x < F.x1; }

__device__ __forceinline__ f32x4 load4(const float* s) { return *reinterpret_cast<const f32x4*>(s); }
__device__ __forceinline__ f32x4 load4(const uint8_t* s) {
  const uint32_t w = *reinterpret_cast<const uint32_t*>(s);
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (float)((w >> (8 * e)) & 0xffu);
  return v;
}

// pixels [lo, hi) of one unblurred frame: jitter_piece with the two pointwise stages
template <typename T>
__device__ __forceinline__ void degrade_piece(const DegradeFrame& F, const T* __restrict__ s, float* __restrict__ d, int64_t HW, uint32_t W,
                                              int64_t lo, int64_t hi, bool first_piece, int head, bool vec_ok) {
  const int tid = threadIdx.x;
  const bool erase = F.j.erase != 0;
  auto one = [&](int64_t j) {
    float r = src_at(s, j), g = src_at(s, j + HW), b = src_at(s, j + 2 * HW);
    int32_t y = 0;
    uint32_t x = 0;
    if (erase) jitter_pos(F.j, W, j, lo, y, x);
    degrade_pixel(F, r, g, b, j, HW, erase && in_rect(F.j, y, x));
    d[j] = r; d[j + HW] = g; d[j + 2 * HW] = b;
  };
  int64_t a = lo;
  if (vec_ok) {
    if (first_piece) {   // (lo == 0)
      if (tid < head && tid < hi) one(tid);
      a = head;
    }
    if (hi > a) {
      const int64_t nv = (hi - a) / 4;
      for (int64_t v = tid; v < nv; v += NT) {
        const int64_t j = a + v * 4;
        int32_t y = 0;
        uint32_t x = 0;
        if (erase) jitter_pos(F.j, W, j, lo, y, x);
        f32x4 vr = load4(s + j), vg = load4(s + j + HW), vb = load4(s + j + 2 * HW);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float r = vr[e], g = vg[e], b = vb[e];
          degrade_pixel(F, r, g, b, j + e, HW, erase && in_rect(F.j, y, x));
          if (erase) jitter_next(W, y, x);
          vr[e] = r; vg[e] = g; vb[e] = b;
        }
        *reinterpret_cast<f32x4*>(d + j) = vr;
        *reinterpret_cast<f32x4*>(d + j + HW) = vg;
        *reinterpret_cast<f32x4*>(d + j + 2 * HW) = vb;
      }
      a += nv * 4;
    }
  }
  for (int64_t j = a + tid; j < hi; j += NT) one(j);
}

// index v of a row or column of n pixels, -n < v < 2 n - 1, mirrored at the border without repeating it
__device__ __forceinline__ int64_t reflect(int64_t v, int64_t n) { return v < 0 ? -v : (v >= n ? 2 * (n - 1) - v : v); }

// tile `tile` of one blurred frame: s, d = its first plane.  Every thread of the workgroup calls this.
template <typename T>
__device__ __forceinline__ void blur_tile(const DegradeFrame& F, const T* __restrict__ s, float* __restrict__ d, int H, int W, int R,
                                          float sigma, int tile, float* lds) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t HW = (int64_t)H * W;
  const int tiles_x = (int)(((uint32_t)W + BLUR_TW - 1) / BLUR_TW);
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int64_t y0 = (int64_t)ty * BLUR_TH, x0 = (int64_t)tx * BLUR_TW;
  const int th = (int)(H - y0 < BLUR_TH ? H - y0 : BLUR_TH), tw = (int)(W - x0 < BLUR_TW ? W - x0 : BLUR_TW);
  const int ih = th + 2 * R, iw = tw + 2 * R;      // <= BLUR_IN_H, BLUR_IN_W: R <= BLUR_RMAX is checked on the host
  float* in = lds;
  float* mid = lds + 3 * BLUR_PLANE;
  float* taps = mid + BLUR_MID;
  if (tid <= R) taps[tid] = expf(-(float)(tid * tid) / (2.0f * sigma * sigma));
  // the image's ih * iw pixels in row-major order, consecutive lanes on consecutive pixels; a lane issues the twelve loads of
  // four pixels before it blends the first, so that two workgroups per compute unit are enough to cover the loads' latency
  const int pixels = ih * iw;
  for (int first = tid; first < pixels; first += NT * BLUR_LOADS) {
    float r[BLUR_LOADS], g[BLUR_LOADS], b[BLUR_LOADS];
    int o[BLUR_LOADS];
#pragma unroll
    for (int u = 0; u < BLUR_LOADS; ++u) {
      const int idx = first + u * NT;
      const bool inside = idx < pixels;                // (outside: pixel (0, 0) of the image is loaded and dropped)
      const int ly = inside ? idx / iw : 0, lx = inside ? idx - ly * iw : 0;
      const int64_t j = reflect(y0 - R + ly, H) * W + reflect(x0 - R + lx, W);
      r[u] = src_at(s, j); g[u] = src_at(s, j + HW); b[u] = src_at(s, j + 2 * HW);
      o[u] = inside ? ly * BLUR_IN_W + lx : -1;
    }
#pragma unroll
    for (int u = 0; u < BLUR_LOADS; ++u) {
      if (o[u] < 0) continue;
      jitter_pixel<false>(F.j, r[u], g[u], b[u], 0, 0);
      if (F.hue) hue_pixel(F.shift, r[u], g[u], b[u]);
      in[o[u]] = r[u]; in[BLUR_PLANE + o[u]] = g[u]; in[2 * BLUR_PLANE + o[u]] = b[u];
    }
  }
  __syncthreads();
  float w[BLUR_RMAX + 1];
  float side = 0.0f;
#pragma unroll
  for (int k = 1; k <= BLUR_RMAX; ++k) {
    w[k] = k <= R ? taps[k] : 0.0f;
    side += w[k];
  }
  w[0] = taps[0];
  const float total = fmaf(2.0f, side, w[0]);
#pragma unroll
  for (int k = 0; k <= BLUR_RMAX; ++k) w[k] = w[k] / total;
  const bool erase = F.j.erase != 0;
#pragma unroll 1
  for (int c = 0; c < 3; ++c) {
    const float* pin = in + c * BLUR_PLANE;
    if (lane < tw) {
      for (int ly = wave; ly < ih; ly += NT / 64) {
        const float* p = pin + ly * BLUR_IN_W + lane + R;
        float acc = w[0] * p[0];
#pragma unroll
        for (int k = 1; k <= BLUR_RMAX; ++k)
          if (k <= R) acc = fmaf(w[k], p[-k] + p[k], acc);
        mid[ly * BLUR_TW + lane] = acc;
      }
    }
    __syncthreads();
    for (int q = tid; q < BLUR_TH * (BLUR_TW / 4); q += NT) {
      const int oy = q / (BLUR_TW / 4), ox = (q % (BLUR_TW / 4)) * 4;
      if (oy >= th || ox >= tw) continue;
      const float* p = mid + (oy + R) * BLUR_TW + ox;
      f32x4 acc = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = w[0] * acc[e];
#pragma unroll
      for (int k = 1; k <= BLUR_RMAX; ++k) {
        if (k <= R) {
          const f32x4 up = *reinterpret_cast<const f32x4*>(p - k * BLUR_TW), down = *reinterpret_cast<const f32x4*>(p + k * BLUR_TW);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = fmaf(w[k], up[e] + down[e], acc[e]);
        }
      }
      const int64_t y = y0 + oy, x = x0 + ox;
      const int64_t j = y * W + x;
      const int valid = tw - ox < 4 ? tw - ox : 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (e < valid) {
          if (F.noise) acc[e] = degrade_noise(F, acc[e], (uint64_t)(c * HW + j + e));
          if (erase && in_rect(F.j, y, x + e)) acc[e] = F.j.m;
        }
      }
      float* o = d + c * HW + j;
      if (valid == 4 && ((uintptr_t)o & 15) == 0) {
        *reinterpret_cast<f32x4*>(o) = acc;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < valid) o[e] = acc[e];
      }
    }
    __syncthreads();                                // mid is rewritten by the next plane
  }
}

__global__ __launch_bounds__(NT) void camera_degrade_kernel(const mmfn_camera_degrade_desc D, const int64_t* __restrict__ index, int64_t n,
                                                            int pieces, int tiles) {
  extern __shared__ __attribute__((aligned(16))) float degrade_lds[];
  const int blk = (int)blockIdx.x, b = (int)blockIdx.y, s = (int)blockIdx.z, S = D.n_frames;
  const int64_t HW = (int64_t)D.H * D.W, frame = 3 * HW;
  const int esz = D.src_type == MMFN_GATHER_U8 ? 1 : 4;
  const int align = D.src_type == MMFN_GATHER_U8 ? 4 : 16;   // bytes of a lane's load
  int64_t i = index[b];
  i = i < 0 ? 0 : (i >= n ? n - 1 : i);
  const uint64_t id = (uint64_t)(D.sample_id ? D.sample_id[i] : i);
  const uint64_t dkey = mmfn_rng_key(D.degrade_state, MMFN_RNG_STREAM_DEGRADE);
  uint32_t q[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) q[j] = mmfn_rng_u32(dkey, id * 8 + j) >> 8;
  const bool blur = q[1] < D.blur_thresh;
  if (blk >= (blur ? tiles : pieces)) return;                // (the same for every lane of the workgroup)
  DegradeFrame F;                                            // (the same in every lane)
  F.hue = D.hue != 0.0f;
  F.shift = D.hue * draw_pm1(q[0]);
  F.noise = q[3] < D.noise_thresh;
  F.noise_std = fmaf(D.noise_std_hi - D.noise_std_lo, (float)q[4] * (1.0f / 16777216.0f), D.noise_std_lo);
  F.noise_key = mmfn_rng_key(D.degrade_state, MMFN_RNG_STREAM_PIXEL_NOISE);
  F.noise_base = (id * (uint64_t)S + (uint64_t)s) * (uint64_t)frame;
  // the jitter's scalars, as camera_jitter_kernel works them out
  const uint64_t key = mmfn_rng_key(D.state, MMFN_RNG_STREAM_JITTER);
  uint32_t k[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) k[j] = mmfn_rng_u32(key, id * 8 + j) >> 8;
  const float m = D.gray_mean[i * S + s];
  JitterFrame& J = F.j;
  J.m = m;
  J.fb = fmaf(D.brightness, fmaf(2.0f, (float)k[0] * (1.0f / 16777216.0f), -1.0f), 1.0f);
  J.fc = fmaf(D.contrast, fmaf(2.0f, (float)k[1] * (1.0f / 16777216.0f), -1.0f), 1.0f);
  J.fs = fmaf(D.saturation, fmaf(2.0f, (float)k[2] * (1.0f / 16777216.0f), -1.0f), 1.0f);
  J.tc = (1.0f - J.fc) * m;
  J.erase = k[3] < D.erase_thresh;
  J.y0 = J.y1 = J.x0 = J.x1 = J.row = 0;
  J.col = 0;
  const uintptr_t sa = (uintptr_t)D.src[s] + (uintptr_t)(i * frame) * esz;
  const int head = (int)(((align - (sa & (align - 1))) & (align - 1)) / esz);
  if (J.erase) {
    const int32_t h = D.erase_h_min + (int32_t)(((uint64_t)k[4] * (uint64_t)(D.erase_h_max - D.erase_h_min + 1)) >> 24);
    const int32_t w = D.erase_w_min + (int32_t)(((uint64_t)k[5] * (uint64_t)(D.erase_w_max - D.erase_w_min + 1)) >> 24);
    J.y0 = (int32_t)(((uint64_t)k[7] * (uint64_t)(D.H - h + 1)) >> 24);
    J.x0 = (int32_t)(((uint64_t)k[6] * (uint64_t)(D.W - w + 1)) >> 24);
    J.y1 = J.y0 + h;
    J.x1 = J.x0 + w;
    if (blk && !blur) {   // the piece's first pixel
      const int64_t lo0 = (int64_t)head + (int64_t)blk * JITTER_PIECE;
      J.row = (int32_t)(lo0 / D.W);
      J.col = (uint32_t)(lo0 % D.W);
    }
  }
  const DegradeFrame& f = F;
  float* d = D.dst + ((int64_t)b * S + s) * frame;
  if (blur) {
    const float sigma = fmaf(D.blur_sigma_hi - D.blur_sigma_lo, (float)q[2] * (1.0f / 16777216.0f), D.blur_sigma_lo);
    if (D.src_type == MMFN_GATHER_U8)
      blur_tile(f, reinterpret_cast<const uint8_t*>(D.src[s]) + i * frame, d, D.H, D.W, D.blur_radius, sigma, blk, degrade_lds);
    else
      blur_tile(f, reinterpret_cast<const float*>(D.src[s]) + i * frame, d, D.H, D.W, D.blur_radius, sigma, blk, degrade_lds);
    return;
  }
  // vector accesses: as in camera_jitter_kernel
  const bool vec_ok = HW % 4 == 0 && (((uintptr_t)(d + head)) & 15) == 0;
  const int64_t lo = blk == 0 ? 0 : head + (int64_t)blk * JITTER_PIECE;
  int64_t hi = head + (int64_t)(blk + 1) * JITTER_PIECE;
  if (lo >= HW) return;
  if (hi > HW) hi = HW;
  if (D.src_type == MMFN_GATHER_U8)
    degrade_piece(f, reinterpret_cast<const uint8_t*>(D.src[s]) + i * frame, d, HW, (uint32_t)D.W, lo, hi, blk == 0, head, vec_ok);
  else
    degrade_piece(f, reinterpret_cast<const float*>(D.src[s]) + i * frame, d, HW, (uint32_t)D.W, lo, hi, blk == 0, head, vec_ok);
}

// ---- radar dropout and noise, speed noise inside the gather (mmfn_gather_radar_speed; draws and formulas: include/mmfn_hip.h) ----
// One workgroup per batch sample: 405 radar floats in, 405 + 6561 out (28 KB), so the launch is B small workgroups and its time
// is the launch's own.  Lanes 0..80 (the first two waves) each own a stored row: padding or not, kept or not, a ballot per wave
// and the first wave's count through LDS place it (map_block's prefix scheme, one round).  Then every lane takes elements of the
// kept rows - 324 values with their own logf / cosf where the column's std is not 0, 81 flags - to LDS and to the destination,
// the zero rows follow, and after a barrier all lanes stream the adjacency out of the written column 1 in LDS: consecutive lanes
// on consecutive addresses, element stores (both rows are odd counts of floats, so a sample's rows start at any 4-byte phase).
// The LDS reads of the adjacency stride by 5 floats, which is odd: no bank conflicts.  The speed is the last lane's, in a wave
// that has no row to decide.
constexpr int RADAR_ROWS = MMFN_RADAR_ROWS, RADAR_ELEMS = RADAR_ROWS * 5, RADAR_ADJ = RADAR_ROWS * RADAR_ROWS;
static_assert(RADAR_ROWS <= 128 && RADAR_ROWS <= NT, "a lane per stored row, draws at id * 128 + r");

// the camera's sensor noise draw (degrade_noise) out of two 24-bit draws
__device__ __forceinline__ float normal_draw(uint32_t n0, uint32_t n1) {
  const float u1 = (float)(n0 + 1u) * (1.0f / 16777216.0f), u2 = (float)n1 * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * logf(u1)) * cosf(6.2831855f * u2);
}

__global__ __launch_bounds__(NT) void radar_speed_kernel(const mmfn_radar_speed_desc D, const int64_t* __restrict__ index, int64_t n) {
  __shared__ float out[RADAR_ELEMS];               // the rows as written
  __shared__ uint8_t kept_row[RADAR_ROWS];         // kept_row[p] = stored row that lands at destination row p
  __shared__ int wave_count[NT / 64];
  const int tid = threadIdx.x, b = blockIdx.x;
  int64_t i = index[b];
  i = i < 0 ? 0 : (i >= n ? n - 1 : i);
  const uint64_t id = (uint64_t)(D.sample_id ? D.sample_id[i] : i);
  if ((D.parts & MMFN_SIGNAL_SPEED) && tid == NT - 1) {
    const uint64_t key = mmfn_rng_key(D.speed_state, MMFN_RNG_STREAM_SPEED);
    float v = D.speed_src[i];
    if ((mmfn_rng_u32(key, id * 8) >> 8) < D.speed_drop_thresh) {
      v = 0.0f;
    } else if (D.speed_std != 0.0f) {
      const float z = normal_draw(mmfn_rng_u32(key, id * 8 + 1) >> 8, mmfn_rng_u32(key, id * 8 + 2) >> 8);
      v = fmaxf(fmaf(D.speed_std, z, v), fminf(v, 0.0f));
    }
    D.speed_dst[b] = v;
  }
  if (!(D.parts & MMFN_SIGNAL_RADAR)) return;        // (the same for every lane of the workgroup)
  const float* src = D.radar_src + i * RADAR_ELEMS;
  bool keep = false;
  if (tid < RADAR_ROWS) {
    const float* p = src + tid * 5;
    const bool real = !(p[0] == 0.0f && p[1] == 0.0f && p[2] == 0.0f && p[3] == 0.0f && p[4] == 0.0f);
    keep = real && !((mmfn_rng_u32(mmfn_rng_key(D.radar_state, MMFN_RNG_STREAM_RADAR), id * 128 + (uint64_t)tid) >> 8) < D.point_thresh);
  }
  const uint64_t wave_keep = __ballot(keep);
  if ((tid & 63) == 0) wave_count[tid >> 6] = __popcll(wave_keep);
  __syncthreads();
  const int first = wave_count[0], kept = first + wave_count[1];     // (rows live in the first two waves only)
  if (keep) kept_row[(tid >> 6 ? first : 0) + __popcll(wave_keep & ((1ull << (tid & 63)) - 1ull))] = (uint8_t)tid;
  __syncthreads();
  const uint64_t noise_key = mmfn_rng_key(D.radar_state, MMFN_RNG_STREAM_RADAR_NOISE);
  float* d = D.radar_dst + (int64_t)b * RADAR_ELEMS;
  const int n_kept = kept * 5;
  for (int e = tid; e < n_kept; e += NT) {
    const int p = e / 5, c = e - p * 5, r = kept_row[p];
    float v = src[r * 5 + c];
    const float std_c = c == 0 ? D.depth_std : (c == 3 ? D.velocity_std : (c == 4 ? 0.0f : D.angle_std));
    if (std_c != 0.0f) {
      const uint64_t q = (id * 128 + (uint64_t)r) * 4 + (uint64_t)c;
      v = fmaf(std_c, normal_draw(mmfn_rng_u32(noise_key, 2 * q) >> 8, mmfn_rng_u32(noise_key, 2 * q + 1) >> 8), v);
      if (c == 0) v = fmaxf(v, 0.0f);
    }
    out[e] = v;
    d[e] = v;
  }
  for (int e = n_kept + tid; e < RADAR_ELEMS; e += NT) {
    out[e] = 0.0f;
    d[e] = 0.0f;
  }
  __syncthreads();
  float* a = D.adj_dst + (int64_t)b * RADAR_ADJ;
  for (int e = tid; e < RADAR_ADJ; e += NT) {
    const int row = e / RADAR_ROWS, col = e - row * RADAR_ROWS;
    a[e] = out[col * 5 + 1] - out[row * 5 + 1];
  }
}
}  // namespace

extern "C" int mmfn_sizeof_radar_speed_desc(void) { return (int)sizeof(mmfn_radar_speed_desc); }

extern "C" int mmfn_gather_radar_speed(const mmfn_radar_speed_desc* d, const int64_t* index, int B, int64_t n, void* stream) {
  if (!d || !index || (uintptr_t)index % 8 || B < 0 || B > 65535) return MMFN_EINVAL;
  if (d->parts < 1 || d->parts > (MMFN_SIGNAL_RADAR | MMFN_SIGNAL_SPEED) || (uintptr_t)d->sample_id % 8) return MMFN_EINVAL;
  if (d->parts & MMFN_SIGNAL_RADAR) {
    if (!d->radar_src || (uintptr_t)d->radar_src % 4 || !d->radar_dst || (uintptr_t)d->radar_dst % 4 || !d->adj_dst ||
        (uintptr_t)d->adj_dst % 4 || !d->radar_state || (uintptr_t)d->radar_state % 8)
      return MMFN_EINVAL;
    if (d->rows != MMFN_RADAR_ROWS || d->point_thresh > (1u << 24)) return MMFN_EINVAL;
    if (!(d->depth_std >= 0.0f && d->depth_std <= 4.0f)) return MMFN_EINVAL;            // (a NaN fails both comparisons)
    if (!(d->angle_std >= 0.0f && d->angle_std <= 0.1f)) return MMFN_EINVAL;
    if (!(d->velocity_std >= 0.0f && d->velocity_std <= 4.0f)) return MMFN_EINVAL;
  }
  if (d->parts & MMFN_SIGNAL_SPEED) {
    if (!d->speed_src || (uintptr_t)d->speed_src % 4 || !d->speed_dst || (uintptr_t)d->speed_dst % 4 || !d->speed_state ||
        (uintptr_t)d->speed_state % 8)
      return MMFN_EINVAL;
    if (d->speed_drop_thresh > (1u << 24)) return MMFN_EINVAL;
    if (!(d->speed_std >= 0.0f && d->speed_std <= 4.0f)) return MMFN_EINVAL;
  }
  if (B == 0) return 0;
  if (n < 1) return MMFN_EINVAL;
  hipLaunchKernelGGL(radar_speed_kernel, dim3((unsigned)B), dim3(NT), 0, (hipStream_t)stream, *d, index, n);
  MMFN_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmfn_sizeof_camera_degrade_desc(void) { return (int)sizeof(mmfn_camera_degrade_desc); }
extern "C" int mmfn_camera_degrade_tile_h(void) { return BLUR_TH; }
extern "C" int mmfn_camera_degrade_tile_w(void) { return BLUR_TW; }

extern "C" int mmfn_gather_camera_degrade(const mmfn_camera_degrade_desc* d, const int64_t* index, int B, int64_t n, void* stream) {
  if (!d || !index || (uintptr_t)index % 8 || B < 0 || B > 65535) return MMFN_EINVAL;
  if (d->n_frames < 1 || d->n_frames > MMFN_JITTER_MAX_FRAMES) return MMFN_EINVAL;
  if (d->src_type != MMFN_GATHER_U8 && d->src_type != MMFN_GATHER_F32) return MMFN_EINVAL;
  const int esz = d->src_type == MMFN_GATHER_F32 ? 4 : 1;
  for (int s = 0; s < d->n_frames; ++s)
    if (!d->src[s] || (uintptr_t)d->src[s] % esz) return MMFN_EINVAL;
  if (!d->dst || (uintptr_t)d->dst % 4 || !d->gray_mean || (uintptr_t)d->gray_mean % 4 || !d->state || (uintptr_t)d->state % 8 ||
      !d->degrade_state || (uintptr_t)d->degrade_state % 8 || (uintptr_t)d->sample_id % 8)
    return MMFN_EINVAL;
  if (d->H < 1 || d->W < 1) return MMFN_EINVAL;
  const float strength[3] = {d->brightness, d->contrast, d->saturation};
  for (float v : strength)
    if (!(v >= 0.0f && v <= 1.0f)) return MMFN_EINVAL;   // (a NaN fails both comparisons)
  if (d->erase_thresh > (1u << 24)) return MMFN_EINVAL;
  if (d->erase_thresh > 0 && (d->erase_h_min < 1 || d->erase_h_min > d->erase_h_max || d->erase_h_max > d->H || d->erase_w_min < 1 ||
                              d->erase_w_min > d->erase_w_max || d->erase_w_max > d->W))
    return MMFN_EINVAL;
  if (!(d->hue >= 0.0f && d->hue <= 0.5f)) return MMFN_EINVAL;
  if (d->blur_thresh > (1u << 24) || d->noise_thresh > (1u << 24)) return MMFN_EINVAL;
  if (d->blur_radius < 0 || d->blur_radius > MMFN_DEGRADE_MAX_RADIUS) return MMFN_EINVAL;
  if (d->blur_thresh > 0) {
    if (d->H <= d->blur_radius || d->W <= d->blur_radius) return MMFN_EINVAL;   // one mirror image must reach
    if (!(d->blur_sigma_lo > 0.0f && d->blur_sigma_lo <= d->blur_sigma_hi && d->blur_sigma_hi <= 2.6666667f + 1e-6f)) return MMFN_EINVAL;
  }
  if (d->noise_thresh > 0 && !(d->noise_std_lo >= 0.0f && d->noise_std_lo <= d->noise_std_hi && d->noise_std_hi <= 64.0f)) return MMFN_EINVAL;
  if (B == 0) return 0;
  if (n < 1) return MMFN_EINVAL;
  const int64_t pieces = ceil_div64((int64_t)d->H * d->W, JITTER_PIECE);   // (the first piece also takes the head, as in the gather)
  const int64_t tiles = d->blur_thresh ? ceil_div64(d->H, BLUR_TH) * ceil_div64(d->W, BLUR_TW) : 0;
  if (pieces > 0x7fffffff || tiles > 0x7fffffff) return MMFN_EINVAL;
  hipLaunchKernelGGL(camera_degrade_kernel, dim3((unsigned)(pieces > tiles ? pieces : tiles), (unsigned)B, (unsigned)d->n_frames), dim3(NT),
                     d->blur_thresh ? BLUR_LDS_BYTES : 0, (hipStream_t)stream, *d, index, n, (int)pieces, (int)tiles);
  MMFN_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmfn_sizeof_gather_augment_desc(void) { return (int)sizeof(mmfn_gather_augment_desc); }

extern "C" int mmfn_gather_augment(const mmfn_gather_augment_desc* d, const int64_t* index, int B, int64_t n, void* stream) {
  if (!d || !index || (uintptr_t)index % 8 || B < 0 || B > 65535) return MMFN_EINVAL;
  const int all = MMFN_AUGMENT_LIDAR | MMFN_AUGMENT_LANES | MMFN_AUGMENT_TARGET;
  if (d->parts == 0 || (d->parts & ~all) || (uintptr_t)d->sample_id % 8) return MMFN_EINVAL;
  AugmentGrid g = {0, 0, B};
  if (d->parts & MMFN_AUGMENT_LIDAR) {
    if (d->n_frames < 1 || d->n_frames > MMFN_AUGMENT_MAX_FRAMES) return MMFN_EINVAL;
    if (d->src_type != MMFN_GATHER_U8 && d->src_type != MMFN_GATHER_F32 && d->src_type != MMFN_GATHER_PAL4) return MMFN_EINVAL;
    if (d->C < 1 || d->H < 1 || d->W < 1) return MMFN_EINVAL;
    const int64_t plane = (int64_t)d->H * d->W;
    if (plane > 0x3fffffff || plane * d->C > ((int64_t)1 << 40)) return MMFN_EINVAL;   // (plane offsets are 32-bit in the kernel)
    const int64_t row = plane * d->C;
    const bool pal4 = d->src_type == MMFN_GATHER_PAL4;
    const int esz = d->src_type == MMFN_GATHER_F32 ? 4 : 1;
    if (pal4 && (row & 1)) return MMFN_EINVAL;
    for (int s = 0; s < d->n_frames; ++s) {
      if (!d->lidar_src[s] || (uintptr_t)d->lidar_src[s] % esz) return MMFN_EINVAL;
      if (pal4 && (!d->lidar_palette[s] || (uintptr_t)d->lidar_palette[s] % 4)) return MMFN_EINVAL;
    }
    if (!d->lidar_dst || (uintptr_t)d->lidar_dst % 4 || !d->lidar_state || (uintptr_t)d->lidar_state % 8) return MMFN_EINVAL;
    if (d->cell_thresh > (1u << 24) || d->erase_thresh > (1u << 24)) return MMFN_EINVAL;
    if (d->erase_thresh > 0 && (d->erase_h_min < 1 || d->erase_h_min > d->erase_h_max || d->erase_h_max > d->H || d->erase_w_min < 1 ||
                                d->erase_w_min > d->erase_w_max || d->erase_w_max > d->W))
      return MMFN_EINVAL;
    // (the first piece also takes the < 16-byte head, as in the gather)
    g.pieces = (int32_t)(pal4 ? ceil_div64(row / 2, PIECE_BYTES_PAL4) : ceil_div64(row * esz, PIECE_BYTES));
  }
  if (d->parts & (MMFN_AUGMENT_LANES | MMFN_AUGMENT_TARGET))
    if (!d->map_state || (uintptr_t)d->map_state % 8) return MMFN_EINVAL;
  if (d->parts & MMFN_AUGMENT_LANES) {
    if (!d->lane_src || (uintptr_t)d->lane_src % 4 || !d->lane_dst || (uintptr_t)d->lane_dst % 4 || !d->lane_row_off ||
        (uintptr_t)d->lane_row_off % 8 || (uintptr_t)d->lane_count_out % 4)
      return MMFN_EINVAL;
    if (d->lane_nodes < 1 || d->lane_nodes > (1 << 18) || d->lmax < 0 || d->lmax > MMFN_AUGMENT_MAX_LANES) return MMFN_EINVAL;
    if (d->lane_thresh > (1u << 24)) return MMFN_EINVAL;
    if (!(d->shift >= 0.0f && d->shift <= 64.0f)) return MMFN_EINVAL;                  // (a NaN fails both comparisons)
    if (!(d->yaw_rad >= 0.0f && d->yaw_rad <= 0.78539816339744831f + 1e-6f)) return MMFN_EINVAL;
  }
  if (d->parts & MMFN_AUGMENT_TARGET) {
    if (!d->target_src || (uintptr_t)d->target_src % 4 || !d->target_dst || (uintptr_t)d->target_dst % 4) return MMFN_EINVAL;
    if (!(d->target_shift >= 0.0f && d->target_shift <= 64.0f)) return MMFN_EINVAL;
  }
  if (B == 0) return 0;
  if (n < 1) return MMFN_EINVAL;
  g.map_blocks = (d->parts & (MMFN_AUGMENT_LANES | MMFN_AUGMENT_TARGET)) ? 1 : 0;
  const int64_t blocks = (d->parts & MMFN_AUGMENT_LIDAR ? (int64_t)g.pieces * d->n_frames : 0) + g.map_blocks;
  if (blocks * B > 0x7fffffff) return MMFN_EINVAL;
  // the sample is the fastest index of the 1-D grid, as in a gather launch with a coded field (see mmfn_gather_batch)
  hipLaunchKernelGGL(gather_augment_kernel, dim3((unsigned)(blocks * B)), dim3(NT), 0, (hipStream_t)stream, *d, g, index, n);
  MMFN_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmfn_sizeof_camera_jitter_desc(void) { return (int)sizeof(mmfn_camera_jitter_desc); }

extern "C" int mmfn_gather_camera_jitter(const mmfn_camera_jitter_desc* d, const int64_t* index, int B, int64_t n, void* stream) {
  if (!d || !index || (uintptr_t)index % 8 || B < 0 || B > 65535) return MMFN_EINVAL;
  if (d->n_frames < 1 || d->n_frames > MMFN_JITTER_MAX_FRAMES) return MMFN_EINVAL;
  if (d->src_type != MMFN_GATHER_U8 && d->src_type != MMFN_GATHER_F32) return MMFN_EINVAL;
  const int esz = d->src_type == MMFN_GATHER_F32 ? 4 : 1;
  for (int s = 0; s < d->n_frames; ++s)
    if (!d->src[s] || (uintptr_t)d->src[s] % esz) return MMFN_EINVAL;
  if (!d->dst || (uintptr_t)d->dst % 4 || !d->gray_mean || (uintptr_t)d->gray_mean % 4 || !d->state || (uintptr_t)d->state % 8 ||
      (uintptr_t)d->sample_id % 8)
    return MMFN_EINVAL;
  if (d->H < 1 || d->W < 1) return MMFN_EINVAL;
  const float strength[3] = {d->brightness, d->contrast, d->saturation};
  for (float v : strength)
    if (!(v >= 0.0f && v <= 1.0f)) return MMFN_EINVAL;   // (a NaN fails both comparisons)
  if (d->erase_thresh > (1u << 24)) return MMFN_EINVAL;
  if (d->erase_thresh > 0 && (d->erase_h_min < 1 || d->erase_h_min > d->erase_h_max || d->erase_h_max > d->H || d->erase_w_min < 1 ||
                              d->erase_w_min > d->erase_w_max || d->erase_w_max > d->W))
    return MMFN_EINVAL;
  if (B == 0) return 0;
  if (n < 1) return MMFN_EINVAL;
  const int64_t pieces = ceil_div64((int64_t)d->H * d->W, JITTER_PIECE);   // (the first piece also takes the head, as in the gather)
  if (pieces > 0x7fffffff) return MMFN_EINVAL;
  hipLaunchKernelGGL(camera_jitter_kernel, dim3((unsigned)pieces, (unsigned)B, (unsigned)d->n_frames), dim3(NT), 0, (hipStream_t)stream,
                     *d, index, n);
  MMFN_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmfn_sizeof_gather_table(void) { return (int)sizeof(mmfn_gather_table); }

extern "C" int mmfn_gather_batch(const mmfn_gather_table* table, const int64_t* index, int B, int64_t n, void* stream) {
  if (!table || !index || (uintptr_t)index % 8 || B < 0 || n < 0) return MMFN_EINVAL;
  if (table->n_fields < 1 || table->n_fields > MMFN_GATHER_MAX_FIELDS) return MMFN_EINVAL;
  GatherArgs args;
  args.n_fields = table->n_fields;
  int64_t blocks = 0;
  bool coded = false;
  for (int k = 0; k < table->n_fields; ++k) {
    const mmfn_gather_field& f = table->f[k];
    if (f.src_type != MMFN_GATHER_U8 && f.src_type != MMFN_GATHER_F32 && f.src_type != MMFN_GATHER_PAL4) return MMFN_EINVAL;
    const bool pal4 = f.src_type == MMFN_GATHER_PAL4;
    coded |= pal4;
    if (pal4 && (!f.palette || (uintptr_t)f.palette % 4 || (f.row_elems & 1) || f.row_off)) return MMFN_EINVAL;
    const int esz = f.src_type == MMFN_GATHER_F32 ? 4 : 1;
    if (!f.src || !f.dst || (uintptr_t)f.src % esz || (uintptr_t)f.dst % 4) return MMFN_EINVAL;
    if (f.row_elems < 0 || f.dst_stride < 0 || f.dst_offset < 0) return MMFN_EINVAL;
    int64_t total = f.row_elems;
    if (f.row_off) {
      if ((uintptr_t)f.row_off % 8 || (uintptr_t)f.count_out % 4 || f.lmax < 0) return MMFN_EINVAL;
      total *= f.lmax;
    }
    args.f[k] = f;
    args.first_block[k] = (int32_t)blocks;
    // (the first piece also takes the < 16-byte head, so piece p ends at head + (p + 1) * per: the last one still reaches the end)
    if (pal4) blocks += ceil_div64(total / 2, PIECE_BYTES_PAL4);
    else blocks += total ? ceil_div64(total * esz, PIECE_BYTES) : (f.row_off ? 1 : 0);   // an empty ragged field still writes its counts
    if (blocks > 0x7fffffff) return MMFN_EINVAL;
  }
  for (int k = table->n_fields; k <= MMFN_GATHER_MAX_FIELDS; ++k) args.first_block[k] = (int32_t)blocks;
  if (B == 0 || blocks == 0) return 0;
  if (n < 1 || B > 65535) return MMFN_EINVAL;
  // Workgroups are dealt to the chip in grid order, and with (piece, sample) order a batch whose pieces per sample are a multiple
  // of the dies (32 with the coded LiDAR frame of the vec model) sends every sample's camera pieces to the same compute units and
  // its lighter pieces to others: 25.9 us against 17.9 us at 31 pieces, measured.  A launch with a coded field therefore numbers
  // its workgroups with the sample fastest, so one piece of all samples is dealt round before the next piece (18.1 us at 28..34
  // pieces); a launch without one keeps the order it always had.
  args.batch = coded && blocks * B <= 0x7fffffff ? B : 0;
  const dim3 grid = args.batch ? dim3((unsigned)(blocks * B)) : dim3((unsigned)blocks, (unsigned)B);
  hipLaunchKernelGGL(gather_batch_kernel, grid, dim3(NT), 0, (hipStream_t)stream, args, index, n);
  MMFN_LAUNCH_CHECK();
  return 0;
}
