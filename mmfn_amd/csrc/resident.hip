// Batch assembly from a device-resident sample store (data.ResidentFrames): one launch gathers every field of a batch by sample
// index - what PackedFrames.batch (np.take into pinned memory), the host->device copy and the u8 -> f32 widening of stage_batch do
// in three steps on two processors.  Values are only moved (and u8 widened, which is exact): no arithmetic.
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
}  // namespace

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
