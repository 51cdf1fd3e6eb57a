// The bf16-MFMA tile helpers of the flash-style attention kernels (xattn.hip, mhsa_mfma.hip): a
// wave owns 16 rows of one side (fragments resident), the other side streams through LDS in
// 32-row blocks staged as bf16 [32][E + 8]; v_mfma_f32_16x16x32_bf16 throughout.
#pragma once
#include "common.h"

namespace avd {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f4;
typedef __attribute__((ext_vector_type(4))) unsigned u4;
typedef __attribute__((ext_vector_type(4))) short s4;
typedef __attribute__((ext_vector_type(2))) unsigned u2;

constexpr int XB = 32;          // keys (rows pass: queries) per streamed block
constexpr int XT = 256;         // threads per block: 4 waves x 16 owned rows / columns
constexpr int XQ = 64;          // owned rows / columns per block

__device__ __forceinline__ u2 tr4(const bf16* p) {
  const s4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s4*)(reinterpret_cast<uintptr_t>(p)));
  return __builtin_bit_cast(u2, v);
}
__device__ __forceinline__ bf16x8 frag8(u2 lo, u2 hi) {
  return __builtin_bit_cast(bf16x8, u4{lo.x, lo.y, hi.x, hi.y});
}
__device__ __forceinline__ f4 mma(bf16x8 a, bf16x8 b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x8 cvt8(float4 a, float4 b) {
  return bf16x8{(__bf16)a.x, (__bf16)a.y, (__bf16)a.z, (__bf16)a.w,
                (__bf16)b.x, (__bf16)b.y, (__bf16)b.z, (__bf16)b.w};
}
__device__ __forceinline__ bf16x8 pack8(const float (&p)[8]) {
  return bf16x8{(__bf16)p[0], (__bf16)p[1], (__bf16)p[2], (__bf16)p[3],
                (__bf16)p[4], (__bf16)p[5], (__bf16)p[6], (__bf16)p[7]};
}

// a strided f32 matrix: n rows of E features, leading dimension ld
struct Mat {
  const float* p;
  long long ld;
};

// stage rows r0 .. r0 + XB - 1 of two matrices as bf16 [XB][E + 8] each (16-byte row pad, as
// xent.hip); rows >= n zero.  A thread's 8-feature tasks are loaded CH at a time from both matrices
// before any is converted and stored, so a block's loads are in flight together (one round trip
// to memory per chunk, not one per task)
template <int E>
__device__ __forceinline__ void stage_pair(Mat m0, bf16* l0, Mat m1, bf16* l1, int n, int r0, int tid) {
  constexpr int PP = E + 8, V = E / 8, TASKS = XB * V, NT = (TASKS + XT - 1) / XT;
  constexpr int CH = E >= 512 ? 1 : (NT < 4 ? NT : 4);   // E = 512: the registers are full
  static_assert(NT % CH == 0, "whole chunks");
  auto chunk = [&](int c0) {
    float4 v[2][CH][2];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int t = tid + XT * (c0 + i), r = t / V, c = (t - r * V) * 8;
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        v[w][i][0] = v[w][i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < TASKS && r0 + r < n) {
          const Mat& m = w ? m1 : m0;
          const float4* s = reinterpret_cast<const float4*>(m.p + (size_t)(r0 + r) * m.ld + c);
          v[w][i][0] = s[0];
          v[w][i][1] = s[1];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int t = tid + XT * (c0 + i), r = t / V, c = (t - r * V) * 8;
      if (t < TASKS) {
        *reinterpret_cast<bf16x8*>(l0 + r * PP + c) = cvt8(v[0][i][0], v[0][i][1]);
        *reinterpret_cast<bf16x8*>(l1 + r * PP + c) = cvt8(v[1][i][0], v[1][i][1]);
      }
    }
  };
  if constexpr (E >= 512) {
#pragma unroll 1
    for (int c0 = 0; c0 < NT; c0 += CH) chunk(c0);      // rolled: no loads hoisted across chunks
  } else {
#pragma unroll
    for (int c0 = 0; c0 < NT; c0 += CH) chunk(c0);
  }
}

// the resident B fragments of 16 owned rows (n = row, k = 32 features per step); rows >= n zero
template <int E>
__device__ __forceinline__ void own_frags(Mat m, int n, int r0, int lane, bf16x8 (&f)[E / 32]) {
  const int r = r0 + (lane & 15), g = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < E / 32; ++ks) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (r < n) {
      const float4* s = reinterpret_cast<const float4*>(m.p + (size_t)r * m.ld + 32 * ks + 8 * g);
      a = s[0];
      b = s[1];
    }
    f[ks] = cvt8(a, b);
  }
}

// 32 x 16 block of dot products: st[h][e] = (block row 16 h + 4 g + e) . (owned row lane & 15)
template <int E>
__device__ __forceinline__ void scores(const bf16* lds, const bf16x8 (&own)[E / 32], int lane, f4 (&st)[2]) {
  constexpr int PP = E + 8;
  const int r16 = lane & 15, g = lane >> 4;
  st[0] = f4{0.f, 0.f, 0.f, 0.f};
  st[1] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < E / 32; ++ks) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(lds + (16 * h + r16) * PP + 32 * ks + 8 * g);
      st[h] = mma(a, own[ks], st[h]);
    }
  }
}

// acc[t] (features 16 (t0 + t) + 4 g .. + 3, owned row lane & 15) += block^T pv, NT feature tiles
template <int E, int NT>
__device__ __forceinline__ void accum(const bf16* lds, bf16x8 pv, int lane, int t0, f4 (&acc)[NT]) {
  constexpr int PP = E + 8;
  const int g = lane >> 4, q4 = (lane & 15) >> 2, p4 = lane & 3;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const bf16* b0 = lds + (4 * g + q4) * PP + 16 * (t0 + t) + 4 * p4;
    const bf16x8 a = frag8(tr4(b0), tr4(b0 + 16 * PP));
    acc[t] = mma(a, pv, acc[t]);
  }
}

}  // namespace avd
