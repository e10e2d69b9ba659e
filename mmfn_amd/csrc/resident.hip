// Batch assembly from a device-resident sample store (data.ResidentFrames): one launch gathers every field of a batch by sample
// index - what PackedFrames.batch (np.take into pinned memory), the host->device copy and the u8 -> f32 widening of stage_batch do
// in three steps on two processors.  Values are only moved (and u8 widened, which is exact): no arithmetic.
//   dense field   dst[b] = f32(src[index[b]])
//   ragged field  rows [off[i], off[i+1]) of the concatenated source -> dst[b, :count]; rows count..Lmax-1 = +0.0; count -> int32
// Memory-bound, so shaped as the elementwise kernels here: a workgroup owns a contiguous piece of ONE (field, sample) row, a lane
// moves 16 source bytes per access (16 u8 pixels -> four 16-byte stores; 4 floats -> one), no LDS, no atomics.  A row whose
// source and destination are misaligned in the same way gets a scalar head up to the first 16-byte boundary and a scalar tail; one
// whose misalignments differ (a 405-float radar row landing at another batch slot) is moved element by element - such rows are
// a few KB.  The sample indices and the ragged prefix table are read from device memory, so a captured launch follows them.
#include "common.h"

namespace {
constexpr int NT = 256;
constexpr int UNROLL = 4;                       // 16-byte accesses per lane and workgroup piece
constexpr int64_t PIECE_BYTES = (int64_t)NT * 16 * UNROLL;   // source bytes per workgroup: 16 KB

struct GatherArgs {
  mmfn_gather_field f[MMFN_GATHER_MAX_FIELDS];
  int32_t first_block[MMFN_GATHER_MAX_FIELDS + 1];   // running sum of the fields' pieces per sample
  int32_t n_fields;
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
  const int blk = blockIdx.x, b = blockIdx.y;
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
  for (int k = 0; k < table->n_fields; ++k) {
    const mmfn_gather_field& f = table->f[k];
    if (f.src_type != MMFN_GATHER_U8 && f.src_type != MMFN_GATHER_F32) return MMFN_EINVAL;
    const int esz = f.src_type == MMFN_GATHER_U8 ? 1 : 4;
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
    blocks += total ? ceil_div64(total * esz, PIECE_BYTES) : (f.row_off ? 1 : 0);   // an empty ragged field still writes its counts
    if (blocks > 0x7fffffff) return MMFN_EINVAL;
  }
  for (int k = table->n_fields; k <= MMFN_GATHER_MAX_FIELDS; ++k) args.first_block[k] = (int32_t)blocks;
  if (B == 0 || blocks == 0) return 0;
  if (n < 1 || B > 65535) return MMFN_EINVAL;
  hipLaunchKernelGGL(gather_batch_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(NT), 0, (hipStream_t)stream, args, index, n);
  MMFN_LAUNCH_CHECK();
  return 0;
}
