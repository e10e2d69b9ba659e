// Fused AdamW over the flat parameter buffer (run_steps/phase2_train_net.py:110,256:
// torch.optim.AdamW defaults lr 1e-4, betas (0.9, 0.999), eps 1e-8, weight_decay 1e-2).
// HBM-bound: 28 B/param (read p,g,m,v; write p,m,v) in one pass with 16-byte accesses.
// The step count lives in device memory so the launch is hipGraph-replayable.  Per-tensor step counts (a tensor unfrozen late
// starts its bias correction at 1, as torch.optim.AdamW's state[p]["step"]): one counter per step class, RowSlots below.
// Momentum SGD (torch.optim.SGD) is a second update rule on the same buffers, tables and counters: SgdRule below, 20 B/param
// with the momentum buffer in the place of the first moment.
#include <algorithm>

#include "common.h"

namespace {
__global__ void step_advance_kernel(int64_t* step) { *step += 1; }
__global__ void step_advance_if_kernel(int64_t* step, const int32_t* ok) {
  if (*ok) *step += 1;
}

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, int64_t n, float lr, float beta1, float beta2,
                                                    float eps, float wd, const int64_t* __restrict__ step, float grad_scale) {
  const double t = (double)*step;
  // scalar prep in fp64 like torch's Python-side arithmetic, then rounded once to fp32
  const double bc1 = 1.0 - pow((double)beta1, t);
  const float bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, t));
  const float step_size = (float)((double)lr / bc1);
  const float decay = (float)(1.0 - (double)lr * (double)wd);
  const int64_t n4 = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    f32x4 pv = *reinterpret_cast<f32x4*>(p + i * 4);
    f32x4 gv = *reinterpret_cast<const f32x4*>(g + i * 4);
    f32x4 mv = *reinterpret_cast<f32x4*>(m + i * 4);
    f32x4 vv = *reinterpret_cast<f32x4*>(v + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gg = gv[e] * grad_scale;
      pv[e] *= decay;
      mv[e] = mv[e] + (gg - mv[e]) * (1.0f - beta1);
      vv[e] = vv[e] * beta2 + (1.0f - beta2) * gg * gg;
      const float denom = sqrtf(vv[e]) / bc2_sqrt + eps;
      pv[e] = pv[e] - step_size * (mv[e] / denom);
    }
    *reinterpret_cast<f32x4*>(p + i * 4) = pv;
    *reinterpret_cast<f32x4*>(m + i * 4) = mv;
    *reinterpret_cast<f32x4*>(v + i * 4) = vv;
  }
  // tail
  const int64_t i = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float gg = g[i] * grad_scale;
    float pv = p[i] * decay;
    const float mv = m[i] + (gg - m[i]) * (1.0f - beta1);
    const float vv = v[i] * beta2 + (1.0f - beta2) * gg * gg;
    pv = pv - step_size * (mv / (sqrtf(vv) / bc2_sqrt + eps));
    p[i] = pv; m[i] = mv; v[i] = vv;
  }
}
}  // namespace

extern "C" int mmfn_step_advance(int64_t* step, void* stream) {
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step);
  MMFN_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmfn_step_advance_if(int64_t* step, const int32_t* ok, void* stream) {
  if (!step || ((uintptr_t)step & 7) || !ok || ((uintptr_t)ok & 3)) return MMFN_EINVAL;
  hipLaunchKernelGGL(step_advance_if_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step, ok);
  MMFN_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmfn_adamw_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                              float eps, float weight_decay, const int64_t* step, float grad_scale, void* stream) {
  if (n <= 0) return 0;
  if (!step || (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15)) return MMFN_EINVAL;
  const int blocks = (int)std::min<int64_t>(ceil_div64(n / 4 + 1, 256), 4096);
  hipLaunchKernelGGL(adamw_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1, beta2, eps,
                     weight_decay, step, grad_scale);
  MMFN_LAUNCH_CHECK();
  return 0;
}

// ---- the grouped optimizer step: ONE kernel over update rules and slot maps, hyper-parameters in DEVICE memory -----------------
// torch.optim.AdamW param_groups (the reference defines decay / no-decay groups, model_vec.py:179-209) + a learning rate
// that may change every step without re-capturing a hipGraph: each group's hyper-parameters are a row of `hyper` [n_groups][8]
// in HBM, read by the kernel.  One byte per FOUR consecutive parameters (every tensor of the flat layout starts 16-byte aligned,
// so a float4 never straddles tensors) names the float4's SLOT: the scalars it steps with, formed once per block into LDS.
//   slot map  GroupSlots: slot = hyper group, one step count *step for all.  RowSlots: slot = ROW = (hyper group, step class).
//   rule      AdamwRule (28 B/param), AdamwAmsRule (+ max_exp_avg_sq, 36 B/param of an amsgrad group), SgdRule (20 B/param).
// A rule provides Scalars (32 B, one per slot), State (its state streams, passed by value; ok(): the host's pointer check),
// scalars<COEF>(hyper row, step count, coef) and step4(p, g, state, i, scalars), which steps one float4 and returns the new
// parameter; kClampSlot says what a stray group byte does.  A new rule is such a struct plus its two extern "C" entry points.
#define MMFN_ADAMW_MAX_GROUPS 16
namespace {
// ---- weight averaging (torch.optim.swa_utils.AveragedModel) --------------------------------------------------------------
// avg = src at the first update (*n_averaged == 0), else ATen's lerp(avg, src, w).  w as torch forms it: EMA lerps with the
// Python float 1 - decay rounded to fp32 (the host writes it to *ema_w), SWA with 1 / (n_averaged + 1), the reciprocal of an
// int64 tensor in fp32.  Both live in device memory: a captured step stays valid when the decay changes or the count grows.
struct AvgArgs {
  float* avg;
  const int64_t* n_averaged;
  const float* ema_w;
  int mode;
};

__device__ inline float avg_weight(const AvgArgs& a) {
  return a.mode == MMFN_AVG_EMA ? *a.ema_w : 1.0f / (float)(*a.n_averaged + 1);
}

// at::lerp (ATen/native/Lerp.h): the small-weight form below 0.5, the large-weight form from the end point above
__device__ inline float lerp_aten(float a, float p, float w) {
  return fabsf(w) < 0.5f ? a + w * (p - a) : p - (p - a) * (1.0f - w);
}

__device__ inline f32x4 lerp4(f32x4 a, f32x4 p, float w) {
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = lerp_aten(a[e], p[e], w);
  return r;
}

// the average's update of one float4 from the parameter pf; the count and the weight are uniform loads: the first update copies
// the parameter, later ones lerp
__device__ inline void avg_float4(const AvgArgs& avg, int64_t i, f32x4 pf) {
  f32x4 out = pf;
  if (*avg.n_averaged != 0) out = lerp4(*reinterpret_cast<const f32x4*>(avg.avg + i * 4), pf, avg_weight(avg));
  *reinterpret_cast<f32x4*>(avg.avg + i * 4) = out;
}

inline bool aligned16(const void* a, const void* b = nullptr) { return !(((uintptr_t)a | (uintptr_t)b) & 15); }

// ---- AdamW: hyper row {lr, beta1, beta2, eps, weight_decay, grad_scale, 0, amsgrad} ----------------------------------------------
struct GroupScalars { float step_size, decay, bc2_sqrt, beta1, beta2, eps, grad_scale, pad; };

// scalar prep in fp64 like torch's Python-side arithmetic, then rounded once to fp32; pad carries the amsgrad flag
template <bool COEF, bool AMS>
__device__ inline GroupScalars adamw_scalars(const float* __restrict__ h, int64_t count, const float* __restrict__ coef) {
  const double t = (double)count;
  const double lr = (double)h[0], beta1 = (double)h[1], beta2 = (double)h[2];
  GroupScalars s;
  s.step_size = (float)(lr / (1.0 - pow(beta1, t)));
  s.decay = (float)(1.0 - lr * (double)h[4]);
  s.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, t));
  s.beta1 = h[1]; s.beta2 = h[2]; s.eps = h[3]; s.grad_scale = COEF ? h[5] * *coef : h[5]; s.pad = AMS ? h[7] : 0.f;
  return s;
}

struct AdamwRule {
  using Scalars = GroupScalars;
  struct State {
    float* __restrict__ m;
    float* __restrict__ v;
    bool ok() const { return m && v && aligned16(m, v); }
  };
  static constexpr bool kClampSlot = false;   // a stray group byte indexes the scalars unclamped (the callers' tables are checked)
  template <bool COEF>
  static __device__ inline Scalars scalars(const float* __restrict__ h, int64_t count, const float* __restrict__ coef) {
    return adamw_scalars<COEF, false>(h, count, coef);
  }
  // The arithmetic relies on the contractions the compiler chooses for it (AdamwAmsRule spells them out): no fp contract pragma
  static __device__ inline f32x4 step4(float* __restrict__ p, const float* __restrict__ g, const State& st, int64_t i,
                                       const Scalars& s) {
    f32x4 pv = *reinterpret_cast<f32x4*>(p + i * 4);
    f32x4 gv = *reinterpret_cast<const f32x4*>(g + i * 4);
    f32x4 mv = *reinterpret_cast<f32x4*>(st.m + i * 4);
    f32x4 vv = *reinterpret_cast<f32x4*>(st.v + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gg = gv[e] * s.grad_scale;
      pv[e] *= s.decay;
      mv[e] = mv[e] + (gg - mv[e]) * (1.0f - s.beta1);
      vv[e] = vv[e] * s.beta2 + (1.0f - s.beta2) * gg * gg;
      const float denom = sqrtf(vv[e]) / s.bc2_sqrt + s.eps;
      pv[e] = pv[e] - s.step_size * (mv[e] / denom);
    }
    *reinterpret_cast<f32x4*>(p + i * 4) = pv;
    *reinterpret_cast<f32x4*>(st.m + i * 4) = mv;
    *reinterpret_cast<f32x4*>(st.v + i * 4) = vv;
    return pv;
  }
};

// ---- amsgrad (torch.optim.AdamW(amsgrad=True), the single-tensor non-capturable form) ------------------------------------------
// A fifth stream vmax holds the running maximum of the second moment: vmax = maximum(vmax, v_new), and the denominator is built
// from sqrtf(vmax) instead of sqrtf(v_new).  amsgrad is a per-group property: hyper[group][7] != 0 switches it on, and a float4 of
// a group without it neither loads nor stores vmax and gets the bits of AdamwRule.
// torch.maximum: NaN when either operand is NaN (fmaxf would drop it)
__device__ inline float max_nan(float a, float b) { return (a == a && !(b <= a)) ? b : a; }

struct AdamwAmsRule {
  using Scalars = GroupScalars;
  struct State {
    float* __restrict__ m;
    float* __restrict__ v;
    float* __restrict__ vmax;
    bool ok() const { return m && v && vmax && aligned16(m, v) && aligned16(vmax); }
  };
  static constexpr bool kClampSlot = false;   // as AdamwRule
  template <bool COEF>
  static __device__ inline Scalars scalars(const float* __restrict__ h, int64_t count, const float* __restrict__ coef) {
    return adamw_scalars<COEF, true>(h, count, coef);
  }
  // The element arithmetic is written out operation by operation, with the contractions the compiler chose for AdamwRule as
  // explicit fmaf calls and contraction switched off for the rest, so that the bits do not depend on what else reads the values
  // here: g * grad_scale - m is one fma, so are the two moment updates and p * decay - step_size * q.
  static __device__ inline f32x4 step4(float* __restrict__ p, const float* __restrict__ g, const State& st, int64_t i,
                                       const Scalars& s) {
#pragma clang fp contract(off)
    const bool ams = s.pad != 0.f;
    f32x4 pv = *reinterpret_cast<f32x4*>(p + i * 4);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i * 4);
    f32x4 mv = *reinterpret_cast<f32x4*>(st.m + i * 4);
    f32x4 vv = *reinterpret_cast<f32x4*>(st.v + i * 4);
    f32x4 xv = vv;
    if (ams) xv = *reinterpret_cast<f32x4*>(st.vmax + i * 4);
    const float omb1 = 1.0f - s.beta1, omb2 = 1.0f - s.beta2;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gg = gv[e] * s.grad_scale;
      mv[e] = __builtin_fmaf(omb1, __builtin_fmaf(gv[e], s.grad_scale, -mv[e]), mv[e]);
      vv[e] = __builtin_fmaf(s.beta2, vv[e], gg * (omb2 * gg));
      xv[e] = ams ? max_nan(xv[e], vv[e]) : vv[e];
      const float denom = sqrtf(xv[e]) / s.bc2_sqrt + s.eps;
      pv[e] = __builtin_fmaf(s.decay, pv[e], -(s.step_size * (mv[e] / denom)));
    }
    *reinterpret_cast<f32x4*>(p + i * 4) = pv;
    *reinterpret_cast<f32x4*>(st.m + i * 4) = mv;
    *reinterpret_cast<f32x4*>(st.v + i * 4) = vv;
    if (ams) *reinterpret_cast<f32x4*>(st.vmax + i * 4) = xv;
    return pv;
  }
};

// ---- momentum SGD (torch.optim.SGD, the single-tensor form) ----------------------------------------------------------------------
// One state stream buf (torch's momentum_buffer): 20 B per parameter (read p, g, buf; write p, buf), 12 B for a float4 of a
// group with momentum 0, which neither loads nor stores buf.  hyper row: {lr, momentum, dampening, nesterov, weight_decay,
// grad_scale, max_norm, 0}.  Per element
//     d   = g * grad_scale + weight_decay * p          (coupled decay)
//     buf = first ? d : momentum * buf + (1 - dampening) * d
//     p   = p - lr * (nesterov ? d + momentum * buf : buf)
// first: the slot's step count after the advance is 1 (torch: momentum_buffer is None).
struct SgdScalars { float lr, momentum, omd, wd, grad_scale, nesterov, first, pad; };

struct SgdRule {
  using Scalars = SgdScalars;
  struct State {
    float* __restrict__ buf;
    bool ok() const { return buf && aligned16(buf); }
  };
  static constexpr bool kClampSlot = true;   // a group byte that names no group of the table reads group 0, never past the LDS
  template <bool COEF>
  static __device__ inline Scalars scalars(const float* __restrict__ h, int64_t t, const float* __restrict__ coef) {
    SgdScalars s;
    s.lr = h[0]; s.momentum = h[1];
    s.omd = (float)(1.0 - (double)h[2]);   // in fp64 like torch's Python-side 1 - dampening, rounded once
    s.wd = h[4]; s.grad_scale = COEF ? h[5] * *coef : h[5];
    s.nesterov = h[3]; s.first = t == 1 ? 1.f : 0.f; s.pad = 0.f;
    return s;
  }
  // Written operation by operation with explicit fmaf calls and contraction switched off for the rest (as AdamwAmsRule), so
  // that the bits do not depend on the instance around it.
  static __device__ inline f32x4 step4(float* __restrict__ p, const float* __restrict__ g, const State& st, int64_t i,
                                       const Scalars& s) {
#pragma clang fp contract(off)
    const bool mom = s.momentum != 0.f, first = s.first != 0.f, nesterov = s.nesterov != 0.f, decay = s.wd != 0.f;
    f32x4 pv = *reinterpret_cast<f32x4*>(p + i * 4);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i * 4);
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (mom && !first) bv = *reinterpret_cast<f32x4*>(st.buf + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gg = gv[e] * s.grad_scale;
      const float d = decay ? __builtin_fmaf(s.wd, pv[e], gg) : gg;
      float u = d;
      if (mom) {
        bv[e] = first ? d : __builtin_fmaf(s.omd, d, s.momentum * bv[e]);
        u = nesterov ? __builtin_fmaf(s.momentum, bv[e], d) : bv[e];
      }
      pv[e] = __builtin_fmaf(-s.lr, u, pv[e]);
    }
    *reinterpret_cast<f32x4*>(p + i * 4) = pv;
    if (mom) *reinterpret_cast<f32x4*>(st.buf + i * 4) = bv;
    return pv;
  }
};

// ---- slot maps --------------------------------------------------------------------------------------------------------------------
// what the entry points hand a slot map's make(): the checked host-side description of the groups, counters and rows
struct SlotArgs {
  int n_groups;
  const int64_t* steps;   // *step, or class_steps [n_classes]: device memory, 8-byte aligned
  const int32_t* rows;    // HOST memory, [n_rows][2] = (group, class)
  int n_rows, n_classes;
};
inline bool groups_ok(const SlotArgs& a) {
  return a.n_groups >= 1 && a.n_groups <= MMFN_ADAMW_MAX_GROUPS && a.steps && !((uintptr_t)a.steps & 7);
}

// slot = hyper group; NULL bytes = everything in group 0.  MASK: byte MMFN_ADAMW_FROZEN is a float4 of a parameter that is not
// trained (requires_grad = False); the bytes are then mandatory, also with one group
struct GroupSlots {
  static constexpr int kMax = MMFN_ADAMW_MAX_GROUPS, kVariants = 16;
  static constexpr bool kMaskImplied = false;
  int n;
  const int64_t* step;
  __device__ int group(int s) const { return s; }
  __device__ int64_t count(int) const { return *step; }
  template <bool MASK, bool CLAMP>
  __device__ int slot(const uint8_t* __restrict__ slot_of, int64_t i) const {
    if (MASK && slot_of[i] == MMFN_ADAMW_FROZEN) return -1;
    const int b = slot_of ? slot_of[i] : 0;
    return (CLAMP && b >= n) ? 0 : b;
  }
  static bool make(GroupSlots& s, const SlotArgs& a, const uint8_t* slot_of, bool mask) {
    s = GroupSlots{a.n_groups, a.steps};
    return groups_ok(a) && (slot_of || !mask);
  }
};

// Per-tensor step counts: torch.optim.AdamW keeps state[p]["step"] per parameter and advances it only on the steps where the
// parameter has a gradient, so a tensor unfrozen late starts its bias correction at 1.  Tensors that took part in exactly the same
// step launches form a step CLASS with one int64 counter in class_steps (device memory).  slot = ROW = (hyper group, step class):
// the same bytes move as with GroupSlots, no per-tensor id stream.  The row map travels as a kernel argument, checked on the host.
struct AdamwRowMap {
  uint16_t cls[MMFN_ADAMW_MAX_ROWS];
  uint8_t group[MMFN_ADAMW_MAX_ROWS];
};
struct RowSlots {
  static constexpr int kMax = MMFN_ADAMW_MAX_ROWS, kVariants = 8;   // 254 * 32 B = 8128 B of LDS
  static constexpr bool kMaskImplied = true;                        // only the MASK instances exist, under the variants without the bit
  AdamwRowMap map;
  int n;
  const int64_t* class_steps;
  __device__ int group(int s) const { return map.group[s]; }
  __device__ int64_t count(int s) const { return class_steps[map.cls[s]]; }
  template <bool MASK, bool CLAMP>
  __device__ int slot(const uint8_t* __restrict__ slot_of, int64_t i) const {
    const int r = slot_of[i];
    return r >= n ? -1 : r;   // MMFN_ADAMW_FROZEN (a byte that names no row is treated alike: it never indexes past the rows in LDS)
  }
  static bool make(RowSlots& s, const SlotArgs& a, const uint8_t* slot_of, bool) {
    if (!groups_ok(a) || !slot_of || !a.rows || a.n_rows < 1 || a.n_rows > MMFN_ADAMW_MAX_ROWS || a.n_classes < 1 || a.n_classes > 65536)
      return false;
    s.n = a.n_rows;
    s.class_steps = a.steps;
    for (int r = 0; r < a.n_rows; ++r) {   // every entry inside its table
      const int32_t grp = a.rows[2 * r], cls = a.rows[2 * r + 1];
      if (grp < 0 || grp >= a.n_groups || cls < 0 || cls >= a.n_classes) return false;
      s.map.group[r] = (uint8_t)grp;
      s.map.cls[r] = (uint16_t)cls;
    }
    return true;
  }
};

// COEF: every slot's grad_scale is multiplied by *coef (the clip_grad_norm_ coefficient, written on the device by
// mmfn_grad_norm_finalize); COEF = false is the plain grouped step.  AVG: the new parameter is also folded into avg.avg
// (the weight average), from registers: 8 B more per parameter instead of a 12 B pass of its own.  GUARD (with COEF only): *ok
// is the non-finite guard's flag (mmfn_grad_norm_finalize_guard); when it is 0 the whole grid returns before it reads or writes
// anything, so parameters, state and the average keep their bits.  MASK: a frozen float4 (slot < 0) belongs to a parameter that
// is not trained: torch skips such a parameter entirely, so the float4 neither loads nor stores p or the state (no weight decay
// either); with AVG it loads p alone and the average still follows it, as AveragedModel lerps every parameter.
template <class Rule, class Slots, bool COEF, bool AVG, bool GUARD, bool MASK>
__global__ __launch_bounds__(256) void optim_step_kernel(float* __restrict__ p, const float* __restrict__ g, typename Rule::State st,
                                                         int64_t n, const uint8_t* __restrict__ slot_of,
                                                         const float* __restrict__ hyper, Slots slots, const float* __restrict__ coef,
                                                         AvgArgs avg, const int32_t* __restrict__ ok) {
  if (GUARD && !*ok) return;   // uniform over the grid: no barrier is left behind
  __shared__ typename Rule::Scalars gs[Slots::kMax];
  if ((int)threadIdx.x < slots.n)
    gs[threadIdx.x] = Rule::template scalars<COEF>(hyper + slots.group(threadIdx.x) * 8, slots.count(threadIdx.x), coef);
  __syncthreads();
  const int64_t n4 = (n + 3) >> 2;   // the flat buffers are padded to a multiple of 4 floats
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int s = slots.template slot<MASK, Rule::kClampSlot>(slot_of, i);
    if (s < 0) {
      if (AVG) avg_float4(avg, i, *reinterpret_cast<const f32x4*>(p + i * 4));
      continue;
    }
    f32x4 pv = Rule::step4(p, g, st, i, gs[s]);
    if (AVG) {
      // an empty asm makes the new parameter opaque here: without it the compiler packs and contracts the rule's arithmetic
      // differently once the lerp also reads it, and the step stops being bit-identical to the instance without AVG
      asm volatile("" : "+v"(pv));
      avg_float4(avg, i, pv);
    }
  }
}

template <bool GUARD>
__global__ __launch_bounds__(256) void weight_average_kernel(const float* __restrict__ src, int64_t n4, AvgArgs avg,
                                                             const int32_t* __restrict__ ok) {
  if (GUARD && !*ok) return;
  const bool copy = *avg.n_averaged == 0;
  const float w = copy ? 1.0f : avg_weight(avg);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    f32x4 out = *reinterpret_cast<const f32x4*>(src + i * 4);
    if (!copy) out = lerp4(*reinterpret_cast<const f32x4*>(avg.avg + i * 4), out, w);
    *reinterpret_cast<f32x4*>(avg.avg + i * 4) = out;
  }
}

// class_steps[c] += 1 for every class whose byte in `active` is set: one thread per class, plain stores
template <bool GUARD>
__global__ __launch_bounds__(256) void class_steps_advance_kernel(int64_t* __restrict__ class_steps, const uint8_t* __restrict__ active,
                                                                  int n_classes, const int32_t* __restrict__ ok) {
  if (GUARD && !*ok) return;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n_classes && active[c]) class_steps[c] = class_steps[c] + 1;
}

constexpr int kAdamwMaxBlocks = 4096;   // beyond 4 * 256 * this many floats the grid-stride loops go round again
int adamw_blocks(int64_t n) { return (int)std::min<int64_t>(ceil_div64(n / 4, 256), kAdamwMaxBlocks); }

// the average: 16-byte aligned floats, the count (and for EMA the weight) in device memory, a known mode
bool avg_args_ok(const AvgArgs& a) {
  if (a.mode != MMFN_AVG_EMA && a.mode != MMFN_AVG_SWA) return false;
  if (!a.avg || ((uintptr_t)a.avg & 15) || !a.n_averaged || ((uintptr_t)a.n_averaged & 7)) return false;
  return a.mode != MMFN_AVG_EMA || (a.ema_w && !((uintptr_t)a.ema_w & 3));
}
bool flag_ok(const int32_t* ok) { return ok && !((uintptr_t)ok & 3); }   // the non-finite guard's device flag

// What every entry point of the family does: the bits of `variant` (MMFN_ADAMW_COEF | _AVG | _GUARD | _MASK) are the template
// arguments.  A set bit makes its pointers mandatory; the pointers of a clear bit are ignored.  Every pointer the launch would read
// is there and aligned, every count in range, or nothing is launched.
template <class Rule, class Slots>
int launch_step(float* p, const float* g, typename Rule::State st, int64_t n, const uint8_t* slot_of, const float* hyper,
                const SlotArgs& sa, int variant, const float* coef, const AvgArgs& avg, const int32_t* ok, void* stream) {
  using Kernel = decltype(&optim_step_kernel<Rule, Slots, false, false, false, true>);
#define MMFN_STEP_ROW(MASK)                                                                                                     \
  {optim_step_kernel<Rule, Slots, false, false, false, MASK>, optim_step_kernel<Rule, Slots, true, false, false, MASK>,         \
   optim_step_kernel<Rule, Slots, false, true, false, MASK>, optim_step_kernel<Rule, Slots, true, true, false, MASK>, nullptr,  \
   optim_step_kernel<Rule, Slots, true, false, true, MASK>, nullptr, optim_step_kernel<Rule, Slots, true, true, true, MASK>}
  static const Kernel kInstances[2][8] = {   // by variant; nullptr: GUARD without COEF, which is not built
      MMFN_STEP_ROW(Slots::kMaskImplied), MMFN_STEP_ROW(true)};
#undef MMFN_STEP_ROW
  if (n <= 0) return 0;
  if (variant < 0 || variant >= Slots::kVariants || !kInstances[variant >> 3][variant & 7]) return MMFN_EINVAL;
  const bool with_coef = variant & MMFN_ADAMW_COEF, with_avg = variant & MMFN_ADAMW_AVG, guard = variant & MMFN_ADAMW_GUARD;
  const AvgArgs a = with_avg ? avg : AvgArgs{};
  Slots slots{};
  if (!p || !g || !aligned16(p, g) || !st.ok() || (n & 3) || !hyper || !Slots::make(slots, sa, slot_of, variant & MMFN_ADAMW_MASK) ||
      (with_coef && !coef) || (with_avg && !avg_args_ok(a)) || (guard && !flag_ok(ok)))
    return MMFN_EINVAL;
  hipLaunchKernelGGL(kInstances[variant >> 3][variant & 7], dim3(adamw_blocks(n)), dim3(256), 0, (hipStream_t)stream, p, g, st, n,
                     slot_of, hyper, slots, with_coef ? coef : nullptr, a, guard ? ok : nullptr);
  MMFN_LAUNCH_CHECK();
  return 0;
}
}  // namespace

extern "C" int mmfn_adamw_groups_f32(float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* group_of,
                                     const float* hyper, int n_groups, const int64_t* step, int variant, const float* coef,
                                     float* avg, const int64_t* n_averaged, const float* ema_w, int avg_mode, const int32_t* ok,
                                     void* stream) {
  return launch_step<AdamwRule, GroupSlots>(p, g, {m, v}, n, group_of, hyper, {n_groups, step, nullptr, 0, 0}, variant, coef,
                                            {avg, n_averaged, ema_w, avg_mode}, ok, stream);
}

extern "C" int mmfn_adamw_rows_f32(float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* row_of, const float* hyper,
                                   int n_groups, const int32_t* rows, int n_rows, const int64_t* class_steps, int n_classes,
                                   int variant, const float* coef, float* avg, const int64_t* n_averaged, const float* ema_w,
                                   int avg_mode, const int32_t* ok, void* stream) {
  return launch_step<AdamwRule, RowSlots>(p, g, {m, v}, n, row_of, hyper, {n_groups, class_steps, rows, n_rows, n_classes}, variant,
                                          coef, {avg, n_averaged, ema_w, avg_mode}, ok, stream);
}

extern "C" int mmfn_adamw_groups_ams_f32(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, const uint8_t* group_of,
                                         const float* hyper, int n_groups, const int64_t* step, int variant, const float* coef,
                                         float* avg, const int64_t* n_averaged, const float* ema_w, int avg_mode, const int32_t* ok,
                                         void* stream) {
  return launch_step<AdamwAmsRule, GroupSlots>(p, g, {m, v, vmax}, n, group_of, hyper, {n_groups, step, nullptr, 0, 0}, variant,
                                               coef, {avg, n_averaged, ema_w, avg_mode}, ok, stream);
}

extern "C" int mmfn_adamw_rows_ams_f32(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, const uint8_t* row_of,
                                       const float* hyper, int n_groups, const int32_t* rows, int n_rows, const int64_t* class_steps,
                                       int n_classes, int variant, const float* coef, float* avg, const int64_t* n_averaged,
                                       const float* ema_w, int avg_mode, const int32_t* ok, void* stream) {
  return launch_step<AdamwAmsRule, RowSlots>(p, g, {m, v, vmax}, n, row_of, hyper, {n_groups, class_steps, rows, n_rows, n_classes},
                                             variant, coef, {avg, n_averaged, ema_w, avg_mode}, ok, stream);
}

extern "C" int mmfn_sgd_groups_f32(float* p, const float* g, float* buf, int64_t n, const uint8_t* group_of, const float* hyper,
                                   int n_groups, const int64_t* step, int variant, const float* coef, float* avg,
                                   const int64_t* n_averaged, const float* ema_w, int avg_mode, const int32_t* ok, void* stream) {
  return launch_step<SgdRule, GroupSlots>(p, g, {buf}, n, group_of, hyper, {n_groups, step, nullptr, 0, 0}, variant, coef,
                                          {avg, n_averaged, ema_w, avg_mode}, ok, stream);
}

extern "C" int mmfn_sgd_rows_f32(float* p, const float* g, float* buf, int64_t n, const uint8_t* row_of, const float* hyper,
                                 int n_groups, const int32_t* rows, int n_rows, const int64_t* class_steps, int n_classes, int variant,
                                 const float* coef, float* avg, const int64_t* n_averaged, const float* ema_w, int avg_mode,
                                 const int32_t* ok, void* stream) {
  return launch_step<SgdRule, RowSlots>(p, g, {buf}, n, row_of, hyper, {n_groups, class_steps, rows, n_rows, n_classes}, variant, coef,
                                        {avg, n_averaged, ema_w, avg_mode}, ok, stream);
}


extern "C" int mmfn_adamw_max_blocks(void) { return kAdamwMaxBlocks; }

extern "C" int mmfn_class_steps_advance(int64_t* class_steps, const uint8_t* active, int n_classes, const int32_t* ok, void* stream) {
  if (!class_steps || ((uintptr_t)class_steps & 7) || !active || n_classes < 1 || n_classes > 65536 || ((uintptr_t)ok & 3))
    return MMFN_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((n_classes + 255) / 256);
  if (ok)
    hipLaunchKernelGGL(class_steps_advance_kernel<true>, grid, dim3(256), 0, st, class_steps, active, n_classes, ok);
  else
    hipLaunchKernelGGL(class_steps_advance_kernel<false>, grid, dim3(256), 0, st, class_steps, active, n_classes, ok);
  MMFN_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmfn_weight_average_f32(float* avg, const float* src, int64_t n, const int64_t* n_averaged, const float* ema_w, int mode,
                                       void* stream) {
  if (n <= 0) return 0;
  const AvgArgs a{avg, n_averaged, ema_w, mode};
  if (!src || ((uintptr_t)src & 15) || (n & 3) || !avg_args_ok(a)) return MMFN_EINVAL;
  hipLaunchKernelGGL(weight_average_kernel<false>, dim3(adamw_blocks(n)), dim3(256), 0, (hipStream_t)stream, src, n / 4, a,
                     (const int32_t*)nullptr);
  MMFN_LAUNCH_CHECK();
  return 0;
}

// ---- the non-finite guard's forms: the same launches behind the device flag *ok (1 = take the step, 0 = skip it) -------------
extern "C" int mmfn_weight_average_if_f32(float* avg, const float* src, int64_t n, const int64_t* n_averaged, const float* ema_w,
                                          int mode, const int32_t* ok, void* stream) {
  if (n <= 0) return 0;
  const AvgArgs a{avg, n_averaged, ema_w, mode};
  if (!src || ((uintptr_t)src & 15) || (n & 3) || !flag_ok(ok) || !avg_args_ok(a)) return MMFN_EINVAL;
  hipLaunchKernelGGL(weight_average_kernel<true>, dim3(adamw_blocks(n)), dim3(256), 0, (hipStream_t)stream, src, n / 4, a, ok);
  MMFN_LAUNCH_CHECK();
  return 0;
}

// dst = src over nbytes when (*flag != 0) == (when != 0), else nothing: the guard's rollback of the BatchNorm state (when = 0)
// and the gated copies of an attached average's buffers (when = 1).  16-byte body, 4-byte tail.
namespace {
__global__ __launch_bounds__(256) void copy_if_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, int64_t n_words,
                                                      const int32_t* __restrict__ flag, int when) {
  if ((*flag != 0) != (when != 0)) return;
  const int64_t n4 = n_words >> 2;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = tid; i < n4; i += (int64_t)gridDim.x * blockDim.x)
    reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
  const int64_t t = n4 * 4 + tid;
  if (t < n_words) dst[t] = src[t];
}
}  // namespace

extern "C" int mmfn_copy_if(void* dst, const void* src, int64_t nbytes, const int32_t* flag, int when, void* stream) {
  if (nbytes <= 0) return 0;
  if (!dst || !src || (((uintptr_t)dst | (uintptr_t)src) & 15) || (nbytes & 3) || !flag_ok(flag)) return MMFN_EINVAL;
  const int64_t n_words = nbytes / 4;
  const int blocks = (int)std::min<int64_t>(ceil_div64(n_words / 4 + 4, 256), 1024);
  hipLaunchKernelGGL(copy_if_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (uint32_t*)dst, (const uint32_t*)src, n_words,
                     flag, when);
  MMFN_LAUNCH_CHECK();
  return 0;
}

// ---- gradient accumulation over the flat buffer + global-norm partials --------------------------------------------------
// torch's `(loss / k).backward()` k times, then one optimizer step: acc += g per micro-step (ADD), g += acc; acc = 0 at the
// final one (FOLD: idempotent, a second FOLD adds zeros), the 1 / (k * world) scale and the clip coefficient go into AdamW.
// Optionally one fp64 sum of squares of the gradient as it LEAVES the kernel per workgroup, into partials[slot + blockIdx.x]:
// the global norm (clip_grad_norm_) from data already in registers.  The grid depends on n only, so the slots and the summation
// order are fixed: bitwise the same on every call, eager or replayed.  HBM-bound: ADD / FOLD move 12 B per float, NONE 4 B.
namespace {
constexpr int kAccumThreads = 256;
constexpr int64_t kAccumMaxBlocks = 1024;

int accum_blocks(int64_t n) { return (int)std::min<int64_t>(ceil_div64(n / 4, kAccumThreads), kAccumMaxBlocks); }

__device__ inline double sumsq4(f32x4 v) {
  return (double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2] + (double)v[3] * v[3];
}

// fixed-order block sum: 64-lane butterfly, then the four wave sums in wave order
__device__ inline double block_sum_f64(double s) {
  __shared__ double wsum[kAccumThreads / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kAccumThreads / 64; ++w) t += wsum[w];
  return t;
}

template <int MODE, bool PARTIALS>
__global__ __launch_bounds__(kAccumThreads) void grad_accum_kernel(float* __restrict__ g, float* __restrict__ acc, int64_t n4,
                                                                   double* __restrict__ partials) {
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kAccumThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kAccumThreads) {
    f32x4 gv = *reinterpret_cast<const f32x4*>(g + i * 4);
    if (MODE == MMFN_ACCUM_ADD) {
      f32x4 av = *reinterpret_cast<const f32x4*>(acc + i * 4);
      *reinterpret_cast<f32x4*>(acc + i * 4) = av + gv;
    } else if (MODE == MMFN_ACCUM_FOLD) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(acc + i * 4);
      gv = gv + av;
      *reinterpret_cast<f32x4*>(g + i * 4) = gv;
      *reinterpret_cast<f32x4*>(acc + i * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (PARTIALS) s += sumsq4(gv);
  }
  if (PARTIALS) {
    const double t = block_sum_f64(s);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
  }
}

template <int MODE>
void launch_accum(float* g, float* acc, int64_t n, double* partials, hipStream_t st) {
  const int blocks = accum_blocks(n);
  if (partials)
    hipLaunchKernelGGL((grad_accum_kernel<MODE, true>), dim3(blocks), dim3(kAccumThreads), 0, st, g, acc, n / 4, partials);
  else
    hipLaunchKernelGGL((grad_accum_kernel<MODE, false>), dim3(blocks), dim3(kAccumThreads), 0, st, g, acc, n / 4, partials);
}

__device__ inline bool finite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// one workgroup: the partials table summed in a fixed order (strided per thread, then the fixed block sum), norm = scale * sqrt.
// GUARD: *ok = isfinite(norm) and *skipped += !ok, plain stores from lane 0 (the non-finite guard: the launches behind it read *ok)
template <bool GUARD>
__global__ __launch_bounds__(kAccumThreads) void grad_norm_finalize_kernel(const double* __restrict__ partials, int n,
                                                                           const float* __restrict__ scale,
                                                                           const float* __restrict__ max_norm,
                                                                           float* __restrict__ norm, float* __restrict__ coef,
                                                                           int32_t* __restrict__ ok, int64_t* __restrict__ skipped) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += kAccumThreads) s += partials[i];
  const double t = block_sum_f64(s);
  if (threadIdx.x == 0) {
    const float nrm = (float)((double)*scale * sqrt(t));
    *norm = nrm;
    if (coef) {
      // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1); a NaN norm propagates into the step
      const float c = *max_norm / (nrm + 1e-6f);
      *coef = c > 1.0f ? 1.0f : c;
    }
    if (GUARD) {
      const bool good = finite_f32(nrm);
      *ok = good ? 1 : 0;
      if (!good) *skipped += 1;
    }
  }
}
}  // namespace

extern "C" int mmfn_grad_accum_blocks(int64_t n) { return n > 0 ? accum_blocks(n) : 0; }

extern "C" int mmfn_grad_accum_f32(float* g, float* acc, int64_t n, int mode, double* partials, void* stream) {
  if (n <= 0) return 0;
  if (!g || (n & 3) || ((uintptr_t)g & 15) || (mode != MMFN_ACCUM_NONE && (!acc || ((uintptr_t)acc & 15))) ||
      ((uintptr_t)partials & 7))
    return MMFN_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  switch (mode) {
    case MMFN_ACCUM_NONE:
      if (!partials) return MMFN_EINVAL;   // reads only: without partials it would do nothing
      launch_accum<MMFN_ACCUM_NONE>(g, acc, n, partials, st);
      break;
    case MMFN_ACCUM_ADD: launch_accum<MMFN_ACCUM_ADD>(g, acc, n, partials, st); break;
    case MMFN_ACCUM_FOLD: launch_accum<MMFN_ACCUM_FOLD>(g, acc, n, partials, st); break;
    default: return MMFN_EINVAL;
  }
  MMFN_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmfn_grad_norm_finalize(const double* partials, int n_partials, const float* scale, const float* max_norm,
                                       float* norm, float* coef, void* stream) {
  if (!partials || n_partials < 1 || !scale || !norm || (coef && !max_norm)) return MMFN_EINVAL;
  hipLaunchKernelGGL(grad_norm_finalize_kernel<false>, dim3(1), dim3(kAccumThreads), 0, (hipStream_t)stream, partials, n_partials,
                     scale, max_norm, norm, coef, (int32_t*)nullptr, (int64_t*)nullptr);
  MMFN_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmfn_grad_norm_finalize_guard(const double* partials, int n_partials, const float* scale, const float* max_norm,
                                             float* norm, float* coef, int32_t* ok, int64_t* skipped, void* stream) {
  if (!partials || ((uintptr_t)partials & 7) || n_partials < 1 || !scale || !norm || !coef || !max_norm || !ok ||
      ((uintptr_t)ok & 3) || !skipped || ((uintptr_t)skipped & 7))
    return MMFN_EINVAL;
  hipLaunchKernelGGL(grad_norm_finalize_kernel<true>, dim3(1), dim3(kAccumThreads), 0, (hipStream_t)stream, partials, n_partials,
                     scale, max_norm, norm, coef, ok, skipped);
  MMFN_LAUNCH_CHECK();
  return 0;
}

// ---- per-tensor statistics of a flat buffer: a segmented reduction in two launches ----------------------------------------------
// Tensors hold 2 .. 2.4 M floats, so every tensor is cut into chunks of kStatsChunk floats and one workgroup reduces one chunk
// into its own fp64 slot triple (sum of squares, max |x| over the finite entries, count of non-finite entries); a second launch
// combines each tensor's slots.  Slots and summation order depend on the table only: two calls on the same data agree bit for bit.
// table: int64 [n_tensors][3] = (offset, count, first chunk), offsets 16-byte aligned; entries past `count` are never read.
namespace {
constexpr int kStatsChunk = 16 * kAccumThreads;   // 4096 floats: four float4 per lane

struct Stats3 { double sumsq, maxabs, bad; };

__device__ inline void stats_add(Stats3& s, float x) {
  if (finite_f32(x)) s.maxabs = fmax(s.maxabs, (double)fabsf(x));
  else s.bad += 1.0;
  s.sumsq += (double)x * (double)x;   // (a non-finite entry makes the sum non-finite)
}

// fixed-order block reduction of the triple: 64-lane butterfly, then the four waves in wave order; the result is lane 0's
__device__ inline Stats3 block_stats(Stats3 s) {
  __shared__ double w3[kAccumThreads / 64][3];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s.sumsq += __shfl_xor(s.sumsq, off, 64);
    s.maxabs = fmax(s.maxabs, __shfl_xor(s.maxabs, off, 64));
    s.bad += __shfl_xor(s.bad, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    w3[threadIdx.x >> 6][0] = s.sumsq; w3[threadIdx.x >> 6][1] = s.maxabs; w3[threadIdx.x >> 6][2] = s.bad;
  }
  __syncthreads();
  Stats3 t{0.0, 0.0, 0.0};
  if (threadIdx.x == 0)
    for (int w = 0; w < kAccumThreads / 64; ++w) {
      t.sumsq += w3[w][0]; t.maxabs = fmax(t.maxabs, w3[w][1]); t.bad += w3[w][2];
    }
  return t;
}

__global__ __launch_bounds__(kAccumThreads) void tensor_stats_chunk_kernel(const float* __restrict__ flat,
                                                                           const int64_t* __restrict__ table, int n_tensors,
                                                                           double* __restrict__ slots) {
  // the tensor whose chunk range holds this workgroup: the last one with first chunk <= blockIdx.x (uniform binary search)
  const int64_t c = blockIdx.x;
  int lo = 0, hi = n_tensors - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid * 3 + 2] <= c) lo = mid; else hi = mid - 1;
  }
  const int64_t count = table[lo * 3 + 1];
  const int64_t base = (c - table[lo * 3 + 2]) * kStatsChunk;   // first element of the chunk inside the tensor
  const float* x = flat + table[lo * 3 + 0];
  Stats3 s{0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t i = base + ((int64_t)j * kAccumThreads + threadIdx.x) * 4;
    if (i + 4 <= count) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) stats_add(s, v[e]);
    } else {
      for (int64_t e = i; e < count; ++e) stats_add(s, x[e]);
    }
  }
  const Stats3 t = block_stats(s);
  if (threadIdx.x == 0) {
    slots[c * 3 + 0] = t.sumsq; slots[c * 3 + 1] = t.maxabs; slots[c * 3 + 2] = t.bad;
  }
}

// one workgroup per tensor: its chunk slots strided over the lanes, then the fixed block reduction
__global__ __launch_bounds__(kAccumThreads) void tensor_stats_combine_kernel(const int64_t* __restrict__ table, int64_t n_chunks,
                                                                             const double* __restrict__ slots, float scale,
                                                                             double* __restrict__ out) {
  const int t = blockIdx.x;
  const int64_t first = table[t * 3 + 2];
  const int64_t last = t + 1 < (int)gridDim.x ? table[(t + 1) * 3 + 2] : n_chunks;
  Stats3 s{0.0, 0.0, 0.0};
  for (int64_t c = first + threadIdx.x; c < last; c += kAccumThreads) {
    s.sumsq += slots[c * 3 + 0];
    s.maxabs = fmax(s.maxabs, slots[c * 3 + 1]);
    s.bad += slots[c * 3 + 2];
  }
  const Stats3 r = block_stats(s);
  if (threadIdx.x == 0) {
    const double a = fabs((double)scale);
    out[t * 3 + 0] = a * sqrt(r.sumsq);
    out[t * 3 + 1] = a * r.maxabs;
    out[t * 3 + 2] = r.bad;
  }
}
}  // namespace

extern "C" int mmfn_tensor_stats_chunk(void) { return kStatsChunk; }

extern "C" int mmfn_tensor_stats_f32(const float* flat, const int64_t* table, int n_tensors, int64_t n_chunks, float scale,
                                     double* out, double* workspace, void* stream) {
  if (!flat || ((uintptr_t)flat & 15) || !table || ((uintptr_t)table & 7) || !out || ((uintptr_t)out & 7) || !workspace ||
      ((uintptr_t)workspace & 7) || n_tensors < 1 || n_chunks < n_tensors || n_chunks > 0x7fffffff)
    return MMFN_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tensor_stats_chunk_kernel, dim3((unsigned)n_chunks), dim3(kAccumThreads), 0, st, flat, table, n_tensors, workspace);
  hipLaunchKernelGGL(tensor_stats_combine_kernel, dim3(n_tensors), dim3(kAccumThreads), 0, st, table, n_chunks, workspace, scale, out);
  MMFN_LAUNCH_CHECK();
  return 0;
}

// ---- one value over a set of ranges of a flat buffer ---------------------------------------------------------------------------
// The gradient ranges of frozen parameters are kept at +0.0 (a fused backward launch may write a frozen tensor's gradient as a
// byproduct): one launch per readiness group stores `value` over the group's frozen ranges.  The table has the format of
// mmfn_tensor_stats_f32 - (offset, count, first chunk), one workgroup per chunk of kStatsChunk floats - with counts that are
// multiples of 4, so every store is a whole float4 inside its range.
namespace {
__global__ __launch_bounds__(kAccumThreads) void fill_ranges_kernel(float* __restrict__ flat, const int64_t* __restrict__ table,
                                                                    int n_ranges, float value) {
  const int64_t c = blockIdx.x;
  int lo = 0, hi = n_ranges - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid * 3 + 2] <= c) lo = mid; else hi = mid - 1;
  }
  const int64_t count = table[lo * 3 + 1];
  const int64_t base = (c - table[lo * 3 + 2]) * kStatsChunk;
  float* x = flat + table[lo * 3 + 0];
  const f32x4 val{value, value, value, value};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t i = base + ((int64_t)j * kAccumThreads + threadIdx.x) * 4;
    if (i + 4 <= count) *reinterpret_cast<f32x4*>(x + i) = val;
  }
}
}  // namespace

// ---- the guard over frozen BatchNorm layers ---------------------------------------------------------------------------------
// *slot = NaN when any of x[0, n) is not finite, else 0.0: one more entry of the gradient-norm partials table.  With frozen
// trunks the backward that would have carried a non-finite activation into the gradient is not run (and a ReLU drops a NaN), so
// the guarded step also looks at what the forward left in the BatchNorm running statistics.  One workgroup: n is tens of thousands.
namespace {
__global__ __launch_bounds__(kAccumThreads) void nonfinite_slot_kernel(const float* __restrict__ x, int64_t n, double* __restrict__ slot) {
  double bad = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kAccumThreads)
    if (!finite_f32(x[i])) bad += 1.0;
  const double t = block_sum_f64(bad);
  if (threadIdx.x == 0) *slot = t > 0.0 ? __longlong_as_double(0x7ff8000000000000LL) : 0.0;
}
}  // namespace

extern "C" int mmfn_nonfinite_slot_f32(const float* x, int64_t n, double* slot, void* stream) {
  if (!x || ((uintptr_t)x & 3) || n < 1 || !slot || ((uintptr_t)slot & 7)) return MMFN_EINVAL;
  hipLaunchKernelGGL(nonfinite_slot_kernel, dim3(1), dim3(kAccumThreads), 0, (hipStream_t)stream, x, n, slot);
  MMFN_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmfn_fill_ranges_f32(float* flat, const int64_t* table, int n_ranges, int64_t n_chunks, float value, void* stream) {
  if (!flat || ((uintptr_t)flat & 15) || !table || ((uintptr_t)table & 7) || n_ranges < 1 || n_chunks < n_ranges ||
      n_chunks > 0x7fffffff)
    return MMFN_EINVAL;
  hipLaunchKernelGGL(fill_ranges_kernel, dim3((unsigned)n_chunks), dim3(kAccumThreads), 0, (hipStream_t)stream, flat, table, n_ranges,
                     value);
  MMFN_LAUNCH_CHECK();
  return 0;
}
