// The "mix" stage of the gated and cross-attention fusion encoders (models/dino.py:237-259,
// 385-452), between the two towers' features [rows, 2E] (the cat) and fusion.
//
// CrossModalAttention.forward (dino.py:393-404), once per encoder call = per view, is
// single-head attention ACROSS the B samples of the call:
//
//   OUT = X + softmax(scale Q K^T) V        Q, K, V, X, OUT [B][E], scale = E^-0.5
//
// avd_xattn_fwd runs dirs x groups independent such problems in one launch (a step's views x
// the image->audio / audio->image directions), flash-style on the bf16 MFMA
// (v_mfma_f32_16x16x32_bf16) exactly as xent.hip's row pass: a wave owns 16 query rows (Q
// fragments resident), streams the keys in 32-key blocks staged as bf16 in LDS (K and V),
// S^T = K Q^T, online max / sum per query, O^T += V^T P^T with the S^T accumulator layout used
// as the B operand as is (V^T read with ds_read_b64_tr_b16).  Scores never reach HBM.
//
// avd_xattn_bwd recomputes P from the forward's row log-sum-exp:
//   rows pass    (wave = 16 queries, streams keys, twice): delta_i = sum_j P_ij dP_ij / sum_j P_ij
//                with dP = dO V^T (kept relative to the dP of the row's largest P, see the
//                kernel), then dS = P o (dP - delta), dQ = scale dS K
//   columns pass (wave = 16 keys, streams queries): dV = P^T dO, dK = scale dS^T Q
// A block owns its rows / columns outright: no split, no atomics, every sum in a fixed order.
// The feature accumulators are cut in chunks of EC columns (grid z) to bound the registers; each
// chunk recomputes S and dP, a few MFLOP.
//
// avd_gate_fwd / avd_gate_bwd: GatedMultiModalEncoder.forward (dino.py:245-259),
// sigmoid(gate) * features per half, the two gates read from device memory.
//
// avd_softmax_rows_fwd / _bwd: the row softmax of the plain (S in HBM) attention route of the
// fp32 parity mode, between avd_gemm calls.
#include <algorithm>
#include <math.h>

#include "attn_tiles.h"
#include "common.h"

using namespace avd;

namespace {

struct XaArgs {
  const float *q, *k, *v, *x, *go, *lse;     // go: dOUT (backward)
  float *out, *lse_out, *dq, *dk, *dv, *delta;
  long long ldq, dsq, ldk, dsk, ldv, dsv, ldx, dsx, ldo, dso;   // ldo / dso: OUT or dOUT
  long long lddq, dsdq, lddk, dsdk, lddv, dsdv;
  int groups, B;
  float scale;
};

// matrix of (direction d, group gi): base + d ds + gi B ld
__device__ __forceinline__ Mat sub(const float* p, long long ld, long long ds, int d, int gi, int B) {
  return Mat{p + (size_t)d * ds + (size_t)gi * B * ld, ld};
}

// ---------------------------------------------------------------- forward
// grid (ceil(B / 64), dirs * groups)
template <int E>
__global__ __launch_bounds__(XT) void xattn_fwd_kernel(XaArgs a) {
  __shared__ __attribute__((aligned(16))) bf16 kb[XB * (E + 8)];
  __shared__ __attribute__((aligned(16))) bf16 vb[XB * (E + 8)];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int g = lane >> 4, r16 = lane & 15;
  const int row0 = blockIdx.x * XQ + wave * 16, row = row0 + r16;
  const int d = blockIdx.y / a.groups, gi = blockIdx.y - d * a.groups, B = a.B;
  const Mat mk = sub(a.k, a.ldk, a.dsk, d, gi, B), mv = sub(a.v, a.ldv, a.dsv, d, gi, B);
  bf16x8 own[E / 32];
  own_frags<E>(sub(a.q, a.ldq, a.dsq, d, gi, B), B, row0, lane, own);
  f4 acc[E / 16];
#pragma unroll
  for (int t = 0; t < E / 16; ++t) acc[t] = f4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  const int nblk = (B + XB - 1) / XB;
  for (int b = 0; b < nblk; ++b) {
    __syncthreads();                          // block b - 1 no longer read
    stage_pair<E>(mk, kb, mv, vb, B, b * XB, tid);
    __syncthreads();
    f4 st[2];
    scores<E>(kb, own, lane, st);
    float v[8], bm = -INFINITY;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = b * XB + 16 * h + 4 * g + e;
        const float s = j < B ? st[h][e] * a.scale : -INFINITY;   // keys past B: out of max and sum
        v[4 * h + e] = s;
        bm = fmaxf(bm, s);
      }
    bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
    bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
    const float mn = fmaxf(m, bm);            // finite from block 0 on (key 0 exists: B >= 1)
    const float sc = __expf(m - mn);
    float p[8], ps = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      p[e] = __expf(v[e] - mn);
      ps += p[e];
    }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    l = l * sc + ps;
    m = mn;
#pragma unroll
    for (int t = 0; t < E / 16; ++t) acc[t] *= sc;
    accum<E, E / 16>(vb, pack8(p), lane, 0, acc);
  }
  if (row < B) {
    const float il = 1.f / l;
    const Mat mx = sub(a.x, a.ldx, a.dsx, d, gi, B);
    float* o = a.out + (size_t)d * a.dso + ((size_t)gi * B + row) * a.ldo;
    const float* xr = mx.p + (size_t)row * mx.ld;
#pragma unroll
    for (int t = 0; t < E / 16; ++t) {
      const float4 xv = *reinterpret_cast<const float4*>(xr + 16 * t + 4 * g);
      *reinterpret_cast<float4*>(o + 16 * t + 4 * g) =
          make_float4(xv.x + acc[t][0] * il, xv.y + acc[t][1] * il, xv.z + acc[t][2] * il,
                      xv.w + acc[t][3] * il);
    }
    if (a.lse_out && g == 0) a.lse_out[((size_t)d * a.groups + gi) * B + row] = m + logf(l);
  }
}

// ---------------------------------------------------------------- backward: rows (delta, dQ)
// grid (ceil(B / 64), dirs * groups, E / EC)
template <int E, int EC>
__global__ __launch_bounds__(XT) void xattn_bwd_rows_kernel(XaArgs a) {
  __shared__ __attribute__((aligned(16))) bf16 kb[XB * (E + 8)];
  __shared__ __attribute__((aligned(16))) bf16 vb[XB * (E + 8)];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int g = lane >> 4, r16 = lane & 15;
  const int row0 = blockIdx.x * XQ + wave * 16, row = row0 + r16;
  const int d = blockIdx.y / a.groups, gi = blockIdx.y - d * a.groups, B = a.B;
  const int t0 = blockIdx.z * (EC / 16);
  const Mat mk = sub(a.k, a.ldk, a.dsk, d, gi, B), mv = sub(a.v, a.ldv, a.dsv, d, gi, B);
  bf16x8 oq[E / 32], od[E / 32];
  own_frags<E>(sub(a.q, a.ldq, a.dsq, d, gi, B), B, row0, lane, oq);
  own_frags<E>(sub(a.go, a.ldo, a.dso, d, gi, B), B, row0, lane, od);
  const size_t srow = ((size_t)d * a.groups + gi) * B + row;
  const float lse = row < B ? a.lse[srow] : INFINITY;        // rows past B: p = 0
  const int nblk = (B + XB - 1) / XB;
  // delta = sum_j P dP / sum_j P is kept as c + dc around c = the dP of the row's largest P:
  // P recomputed from an f32 lse sums to 1 only within |lse| 2^-24, and in a row whose softmax is
  // nearly one-hot dP_top - delta is ~(1 - P_top) |dP|, far below what an f32 sum_j P dP resolves.
  // With dc = sum_j P (dP - c) / sum_j P the top key's own term is exactly zero, so
  // dS = P ((dP - c) - dc) keeps its relative accuracy however small it is.
  float c = 0.f, pm = -1.f, sp = 0.f, dcs = 0.f, dc = 0.f;
  f4 acc[EC / 16];
#pragma unroll
  for (int t = 0; t < EC / 16; ++t) acc[t] = f4{0.f, 0.f, 0.f, 0.f};
  for (int pass = 0; pass < 2; ++pass) {
    for (int b = 0; b < nblk; ++b) {
      __syncthreads();
      stage_pair<E>(mk, kb, mv, vb, B, b * XB, tid);
      __syncthreads();
      f4 st[2], dp[2];
      scores<E>(kb, oq, lane, st);
      scores<E>(vb, od, lane, dp);
      float p[8];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int j = b * XB + 16 * h + 4 * g + e;
          p[4 * h + e] = j < B ? __expf(st[h][e] * a.scale - lse) : 0.f;
        }
      if (pass == 0) {
        // the block's largest P of this row and its dP: over the lane's 8 keys, then the 4 lanes
        // of the row (larger P, then larger dP: every lane of the row ends with the same pair)
        float bp = -1.f, bc = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float dv = dp[e >> 2][e & 3];
          if (p[e] > bp || (p[e] == bp && dv > bc)) { bp = p[e]; bc = dv; }
        }
#pragma unroll
        for (int m = 16; m <= 32; m <<= 1) {
          const float op = __shfl_xor(bp, m, 64), oc = __shfl_xor(bc, m, 64);
          if (op > bp || (op == bp && oc > bc)) { bp = op; bc = oc; }
        }
        if (bp > pm) {                          // a new reference: sum P (dP - c) moves with it
          dcs += (c - bc) * sp;
          c = bc;
          pm = bp;
        }
        float part = 0.f, ps = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          part += p[e] * (dp[e >> 2][e & 3] - c);
          ps += p[e];
        }
        part += __shfl_xor(part, 16, 64);
        part += __shfl_xor(part, 32, 64);
        ps += __shfl_xor(ps, 16, 64);
        ps += __shfl_xor(ps, 32, 64);
        dcs += part;
        sp += ps;
      } else {
        float ds[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) ds[e] = p[e] * ((dp[e >> 2][e & 3] - c) - dc);
        accum<E, EC / 16>(kb, pack8(ds), lane, t0, acc);
      }
    }
    if (pass == 0) {
      dc = sp > 0.f ? dcs / sp : 0.f;           // rows past B: every P is zero
      if (blockIdx.z == 0 && g == 0 && row < B) a.delta[srow] = c + dc;
    }
  }
  if (row < B) {
    float* o = a.dq + (size_t)d * a.dsdq + ((size_t)gi * B + row) * a.lddq;
#pragma unroll
    for (int t = 0; t < EC / 16; ++t)
      *reinterpret_cast<float4*>(o + 16 * (t0 + t) + 4 * g) =
          make_float4(a.scale * acc[t][0], a.scale * acc[t][1], a.scale * acc[t][2], a.scale * acc[t][3]);
  }
}

// ---------------------------------------------------------------- backward: columns (dK, dV)
// grid (ceil(B / 64), dirs * groups, E / EC); after the rows pass (reads its delta)
template <int E, int EC>
__global__ __launch_bounds__(XT) void xattn_bwd_cols_kernel(XaArgs a) {
  __shared__ __attribute__((aligned(16))) bf16 qb[XB * (E + 8)];
  __shared__ __attribute__((aligned(16))) bf16 ob[XB * (E + 8)];
  __shared__ float lb[XB], db[XB];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int g = lane >> 4, r16 = lane & 15;
  const int col0 = blockIdx.x * XQ + wave * 16, col = col0 + r16;
  const int d = blockIdx.y / a.groups, gi = blockIdx.y - d * a.groups, B = a.B;
  const int t0 = blockIdx.z * (EC / 16);
  const Mat mq = sub(a.q, a.ldq, a.dsq, d, gi, B), mo = sub(a.go, a.ldo, a.dso, d, gi, B);
  bf16x8 ok[E / 32], ov[E / 32];
  own_frags<E>(sub(a.k, a.ldk, a.dsk, d, gi, B), B, col0, lane, ok);
  own_frags<E>(sub(a.v, a.ldv, a.dsv, d, gi, B), B, col0, lane, ov);
  const size_t sbase = ((size_t)d * a.groups + gi) * B;
  const int nblk = (B + XB - 1) / XB;
  f4 av[EC / 16], ak[EC / 16];
#pragma unroll
  for (int t = 0; t < EC / 16; ++t) av[t] = ak[t] = f4{0.f, 0.f, 0.f, 0.f};
  for (int b = 0; b < nblk; ++b) {
    __syncthreads();
    stage_pair<E>(mq, qb, mo, ob, B, b * XB, tid);
    if (tid < XB) {
      const int i = b * XB + tid;
      lb[tid] = i < B ? a.lse[sbase + i] : INFINITY;        // queries past B: p = 0
      db[tid] = i < B ? a.delta[sbase + i] : 0.f;
    }
    __syncthreads();
    f4 st[2], dp[2];
    scores<E>(qb, ok, lane, st);
    scores<E>(ob, ov, lane, dp);
    float p[8], ds[8];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ri = 16 * h + 4 * g + e;
        const float pv = col < B ? __expf(st[h][e] * a.scale - lb[ri]) : 0.f;
        p[4 * h + e] = pv;
        ds[4 * h + e] = pv * (dp[h][e] - db[ri]);
      }
    accum<E, EC / 16>(ob, pack8(p), lane, t0, av);
    accum<E, EC / 16>(qb, pack8(ds), lane, t0, ak);
  }
  if (col < B) {
    float* ovp = a.dv + (size_t)d * a.dsdv + ((size_t)gi * B + col) * a.lddv;
    float* okp = a.dk + (size_t)d * a.dsdk + ((size_t)gi * B + col) * a.lddk;
#pragma unroll
    for (int t = 0; t < EC / 16; ++t) {
      *reinterpret_cast<float4*>(ovp + 16 * (t0 + t) + 4 * g) =
          make_float4(av[t][0], av[t][1], av[t][2], av[t][3]);
      *reinterpret_cast<float4*>(okp + 16 * (t0 + t) + 4 * g) =
          make_float4(a.scale * ak[t][0], a.scale * ak[t][1], a.scale * ak[t][2], a.scale * ak[t][3]);
    }
  }
}

bool e_ok(int E) { return E == 32 || E == 64 || E == 128 || E == 256 || E == 512; }

// a strided operand: 16-byte aligned base, ld >= E, ld and the direction stride whole float4s
bool mat_ok(const void* p, long long ld, long long ds, int E) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld >= E && (ld & 3) == 0 && ds >= 0 && (ds & 3) == 0;
}

bool dims_ok(int dirs, int groups, int B, int E) {
  return e_ok(E) && B >= 1 && groups >= 1 && (dirs == 1 || dirs == 2) &&
         (long long)dirs * groups <= 65535 && (long long)dirs * groups * B <= 0x7fffffffLL;
}

template <int E>
void launch_bwd(const XaArgs& a, int dirs, hipStream_t st) {
  constexpr int EC = E > 128 ? 128 : E;
  const dim3 grid((a.B + XQ - 1) / XQ, dirs * a.groups, E / EC);
  xattn_bwd_rows_kernel<E, EC><<<grid, XT, 0, st>>>(a);
  xattn_bwd_cols_kernel<E, EC><<<grid, XT, 0, st>>>(a);
}

// ---------------------------------------------------------------- gates
constexpr int GT = 256;
constexpr int GROWS = 32;       // rows per block of the gate backward's first stage

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// out[r][c] = sigmoid(gate[c >= E]) * cat[r][c], c < 2E
__global__ __launch_bounds__(GT) void gate_fwd_kernel(const float* __restrict__ cat, long long ldc,
                                                      const float* gi, const float* ga,
                                                      float* __restrict__ out, long long ldo, int rows, int E) {
  const float si = sigmoidf(*gi), sa = sigmoidf(*ga);
  const long long n = (long long)rows * 2 * E;
  for (long long i = (long long)blockIdx.x * GT + threadIdx.x; i < n; i += (long long)gridDim.x * GT) {
    const int r = (int)(i / (2 * E)), c = (int)(i - (long long)r * 2 * E);
    out[(size_t)r * ldo + c] = (c < E ? si : sa) * cat[(size_t)r * ldc + c];
  }
}

// stage 1: block b owns rows [b GROWS, (b + 1) GROWS): dcat = sigmoid(gate) dout, and the block's
// partial sums of dout o cat per half -> parts[2][nb].  dcat may be dout itself (each element is
// read and then written by the same thread).
__global__ __launch_bounds__(GT) void gate_bwd_kernel(const float* dout, long long ldd,
                                                      const float* __restrict__ cat, long long ldc,
                                                      const float* gi, const float* ga,
                                                      float* dcat, long long lddc,
                                                      float* __restrict__ parts, int rows, int E) {
  __shared__ float sh[GT / 64];
  const float si = sigmoidf(*gi), sa = sigmoidf(*ga);
  const int r0 = blockIdx.x * GROWS, r1 = min(rows, r0 + GROWS);
  float a0 = 0.f, a1 = 0.f;
  for (int r = r0; r < r1; ++r)
    for (int c = threadIdx.x; c < 2 * E; c += GT) {
      const float dv = dout[(size_t)r * ldd + c], t = dv * cat[(size_t)r * ldc + c];
      a0 += c < E ? t : 0.f;
      a1 += c < E ? 0.f : t;
      dcat[(size_t)r * lddc + c] = (c < E ? si : sa) * dv;
    }
  const float s0 = block_sum<GT>(a0, sh), s1 = block_sum<GT>(a1, sh);
  if (threadIdx.x == 0) {
    parts[blockIdx.x] = s0;
    parts[gridDim.x + blockIdx.x] = s1;
  }
}

// stage 2: one block; dgate_h = s (1 - s) sum_b parts[h][b], lane-strided then a fixed tree
__global__ __launch_bounds__(GT) void gate_bwd_finish(const float* __restrict__ parts, int nb, const float* gi,
                                                      const float* ga, float* dgi, float* dga) {
  __shared__ float sh[GT / 64];
  float acc[2] = {0.f, 0.f};
  for (int b = threadIdx.x; b < nb; b += GT) {
    acc[0] += parts[b];
    acc[1] += parts[nb + b];
  }
  const float s0 = block_sum<GT>(acc[0], sh), s1 = block_sum<GT>(acc[1], sh);
  if (threadIdx.x == 0) {
    const float si = sigmoidf(*gi), sa = sigmoidf(*ga);
    *dgi = si * (1.f - si) * s0;
    *dga = sa * (1.f - sa) * s1;
  }
}

// ---------------------------------------------------------------- row softmax (plain route)
// one wave per row, in place: s[r][:C] = softmax(s[r][:C])
__global__ __launch_bounds__(XT) void softmax_rows_fwd_kernel(float* __restrict__ s, long long ld, int R, int C) {
  const int r = blockIdx.x * (XT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  float* row = s + (size_t)r * ld;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
  m = wave_max(m);
  float l = 0.f;
  for (int c = lane; c < C; c += 64) l += expf(row[c] - m);
  l = wave_sum(l);
  const float il = 1.f / l;
  for (int c = lane; c < C; c += 64) row[c] = expf(row[c] - m) * il;
}

// one wave per row, in place on dp: dp[r][c] = p[r][c] (dp[r][c] - sum_c' p[r][c'] dp[r][c'])
__global__ __launch_bounds__(XT) void softmax_rows_bwd_kernel(const float* __restrict__ p, long long ldp,
                                                              float* __restrict__ dp, long long lddp, int R, int C) {
  const int r = blockIdx.x * (XT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  const float* pr = p + (size_t)r * ldp;
  float* dr = dp + (size_t)r * lddp;
  float dot = 0.f;
  for (int c = lane; c < C; c += 64) dot += pr[c] * dr[c];
  dot = wave_sum(dot);
  for (int c = lane; c < C; c += 64) dr[c] = pr[c] * (dr[c] - dot);
}

}  // namespace

int avd_xattn_fwd(const float* q, long long ldq, long long dsq, const float* k, long long ldk, long long dsk,
                  const float* v, long long ldv, long long dsv, const float* x, long long ldx, long long dsx,
                  float* out, long long ldo, long long dso, float* lse, int dirs, int groups, int B, int E,
                  float scale, void* stream) {
  if (!q || !k || !v || !x || !out) return AVD_ERR_ARG;
  if (!dims_ok(dirs, groups, B, E)) return AVD_ERR_SHAPE;
  if (ldq < E || ldk < E || ldv < E || ldx < E || ldo < E) return AVD_ERR_SHAPE;
  if (!mat_ok(q, ldq, dsq, E) || !mat_ok(k, ldk, dsk, E) || !mat_ok(v, ldv, dsv, E) ||
      !mat_ok(x, ldx, dsx, E) || !mat_ok(out, ldo, dso, E))
    return AVD_ERR_ARG;
  XaArgs a{};
  a.q = q; a.k = k; a.v = v; a.x = x; a.out = out; a.lse_out = lse;
  a.ldq = ldq; a.dsq = dsq; a.ldk = ldk; a.dsk = dsk; a.ldv = ldv; a.dsv = dsv;
  a.ldx = ldx; a.dsx = dsx; a.ldo = ldo; a.dso = dso;
  a.groups = groups; a.B = B; a.scale = scale;
  hipStream_t st = avd_stream(stream);
  const dim3 grid((B + XQ - 1) / XQ, dirs * groups);
  switch (E) {
    case 32: xattn_fwd_kernel<32><<<grid, XT, 0, st>>>(a); break;
    case 64: xattn_fwd_kernel<64><<<grid, XT, 0, st>>>(a); break;
    case 128: xattn_fwd_kernel<128><<<grid, XT, 0, st>>>(a); break;
    case 256: xattn_fwd_kernel<256><<<grid, XT, 0, st>>>(a); break;
    default: xattn_fwd_kernel<512><<<grid, XT, 0, st>>>(a); break;
  }
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

int avd_xattn_bwd_ws(int dirs, int groups, int B, int E) {
  if (!dims_ok(dirs, groups, B, E)) return -1;
  return dirs * groups * B;       // delta, one float per query row
}

int avd_xattn_bwd(const float* dout, long long lddo, long long dsdo, const float* q, long long ldq,
                  long long dsq, const float* k, long long ldk, long long dsk, const float* v, long long ldv,
                  long long dsv, const float* lse, float* dq, long long lddq, long long dsdq, float* dk,
                  long long lddk, long long dsdk, float* dv, long long lddv, long long dsdv, float* ws,
                  long long ws_elems, int dirs, int groups, int B, int E, float scale, void* stream) {
  if (!dout || !q || !k || !v || !lse || !dq || !dk || !dv || !ws) return AVD_ERR_ARG;
  if (!dims_ok(dirs, groups, B, E)) return AVD_ERR_SHAPE;
  if (lddo < E || ldq < E || ldk < E || ldv < E || lddq < E || lddk < E || lddv < E) return AVD_ERR_SHAPE;
  if (!mat_ok(dout, lddo, dsdo, E) || !mat_ok(q, ldq, dsq, E) || !mat_ok(k, ldk, dsk, E) ||
      !mat_ok(v, ldv, dsv, E) || !mat_ok(dq, lddq, dsdq, E) || !mat_ok(dk, lddk, dsdk, E) ||
      !mat_ok(dv, lddv, dsdv, E))
    return AVD_ERR_ARG;
  if (ws_elems < avd_xattn_bwd_ws(dirs, groups, B, E)) return AVD_ERR_ARG;
  XaArgs a{};
  a.q = q; a.k = k; a.v = v; a.go = dout; a.lse = lse; a.dq = dq; a.dk = dk; a.dv = dv; a.delta = ws;
  a.ldq = ldq; a.dsq = dsq; a.ldk = ldk; a.dsk = dsk; a.ldv = ldv; a.dsv = dsv;
  a.ldo = lddo; a.dso = dsdo;
  a.lddq = lddq; a.dsdq = dsdq; a.lddk = lddk; a.dsdk = dsdk; a.lddv = lddv; a.dsdv = dsdv;
  a.groups = groups; a.B = B; a.scale = scale;
  hipStream_t st = avd_stream(stream);
  switch (E) {
    case 32: launch_bwd<32>(a, dirs, st); break;
    case 64: launch_bwd<64>(a, dirs, st); break;
    case 128: launch_bwd<128>(a, dirs, st); break;
    case 256: launch_bwd<256>(a, dirs, st); break;
    default: launch_bwd<512>(a, dirs, st); break;
  }
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

int avd_gate_fwd(const float* cat, long long ldc, const float* gate_image, const float* gate_audio,
                 float* out, long long ldo, int rows, int E, void* stream) {
  if (!cat || !gate_image || !gate_audio || !out) return AVD_ERR_ARG;
  if (rows < 1 || E < 1 || ldc < 2LL * E || ldo < 2LL * E) return AVD_ERR_SHAPE;
  const long long n = (long long)rows * 2 * E;
  const int grid = (int)std::min<long long>((n + GT - 1) / GT, 4096);
  gate_fwd_kernel<<<grid, GT, 0, avd_stream(stream)>>>(cat, ldc, gate_image, gate_audio, out, ldo, rows, E);
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

int avd_gate_bwd_ws(int rows, int E) {
  if (rows < 1 || E < 1) return -1;
  return 2 * ((rows + GROWS - 1) / GROWS);
}

int avd_gate_bwd(const float* dout, long long ldd, const float* cat, long long ldc, const float* gate_image,
                 const float* gate_audio, float* dcat, long long lddc, float* dgate_image,
                 float* dgate_audio, float* ws, long long ws_elems, int rows, int E, void* stream) {
  if (!dout || !cat || !gate_image || !gate_audio || !dcat || !dgate_image || !dgate_audio || !ws)
    return AVD_ERR_ARG;
  if (rows < 1 || E < 1 || ldd < 2LL * E || ldc < 2LL * E || lddc < 2LL * E) return AVD_ERR_SHAPE;
  if (ws_elems < avd_gate_bwd_ws(rows, E)) return AVD_ERR_ARG;
  const int nb = (rows + GROWS - 1) / GROWS;
  hipStream_t st = avd_stream(stream);
  gate_bwd_kernel<<<nb, GT, 0, st>>>(dout, ldd, cat, ldc, gate_image, gate_audio, dcat, lddc, ws, rows, E);
  gate_bwd_finish<<<1, GT, 0, st>>>(ws, nb, gate_image, gate_audio, dgate_image, dgate_audio);
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

int avd_softmax_rows_fwd(float* s, long long ld, int R, int C, void* stream) {
  if (!s) return AVD_ERR_ARG;
  if (R < 1 || C < 1 || ld < C) return AVD_ERR_SHAPE;
  softmax_rows_fwd_kernel<<<(R + XT / 64 - 1) / (XT / 64), XT, 0, avd_stream(stream)>>>(s, ld, R, C);
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

int avd_softmax_rows_bwd(const float* p, long long ldp, float* dp, long long lddp, int R, int C, void* stream) {
  if (!p || !dp) return AVD_ERR_ARG;
  if (R < 1 || C < 1 || ldp < C || lddp < C) return AVD_ERR_SHAPE;
  softmax_rows_bwd_kernel<<<(R + XT / 64 - 1) / (XT / 64), XT, 0, avd_stream(stream)>>>(p, ldp, dp, lddp, R, C);
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}
