// Multi-head self-attention of the ViT tower on the bf16 MFMA (v_mfma_f32_16x16x32_bf16): the
// contract of avd_mhsa_fwd / avd_mhsa_bwd (vit.hip) in bf16 mode, with the algorithm of xattn.hip.
//
//   ctx = dropout(softmax(scale Q K^T)) V      per (sequence n, head h), Q, K, V [T][dh]
//
// Forward, grid (ceil(T / 64), heads, N): a wave owns 16 query rows (Q fragments resident), the
// workgroup's 4 waves stream the T keys in 32-key blocks staged as bf16 in LDS (K and V),
// S^T = K Q^T so that a lane holds one query's scores, online max / sum per query,
// O^T += V^T (P o M)^T with the S^T accumulator layout as the B operand (V^T read with
// ds_read_b64_tr_b16).  The dropout mask M multiplies the unnormalised P that enters P V; the row
// sum l is that of the unmasked P, so ctx = (P / l o M) V as avd_mhsa_fwd defines it.
//
// Backward, P recomputed from the forward's row log-sum-exp, M regenerated:
//   rows pass    (wave = 16 queries, streams keys, twice): dP = (dO V^T) o M,
//                delta_i = sum_j P_ij dP_ij / sum_j P_ij kept relative to the dP of the row's
//                largest P (the comment at xattn_bwd_rows_kernel), dS = P o (dP - delta),
//                dQ = scale dS K; delta -> ws [N][heads][T]
//   columns pass (wave = 16 keys, streams queries): dV = (P o M)^T dO, dK = scale dS^T Q
// A workgroup owns its rows / columns outright: no split, no atomics, every sum in a fixed order.
// A wave or lane without a valid row still stages and meets every barrier; its rows are never
// written.  Scores never reach HBM.  The staging is split (stage_load / stage_store below): the
// next block's global loads are issued before the current block is computed.
#include <math.h>

#include "attn_tiles.h"
#include "common.h"

using namespace avd;

namespace {

struct MmArgs {
  const float *q, *k, *v, *go, *lse;         // go: dctx (backward)
  float *ctx, *lse_out, *dq, *dk, *dv, *delta;
  long long ldq, ldk, ldv, ldo, lddq, lddk, lddv;   // ldo: ctx or dctx
  int heads, T;
  float scale, p;
  unsigned long long seed;
  const unsigned long long* seed_off;
};

// head h of sequence n: rows n T .. n T + T - 1, columns h DH .. h DH + DH - 1
template <int DH>
__device__ __forceinline__ Mat head(const float* p, long long ld, int n, int h, int T) {
  return Mat{p + (size_t)n * T * ld + (size_t)h * DH, ld};
}

__device__ __forceinline__ unsigned long long site_seed(const MmArgs& a) {
  return a.p > 0.f && a.seed_off ? a.seed + a.seed_off[0] : a.seed;
}

// stage_pair in two halves: the global loads of block b + 1 are issued before block b is computed
// and wait in registers until it has been read (LDS keeps one buffer per matrix)
template <int DH>
struct Staged {
  static constexpr int V = DH / 8, TASKS = XB * V, NT = (TASKS + XT - 1) / XT;
  float4 v[2][NT][2];
};

template <int DH>
__device__ __forceinline__ void stage_load(Mat m0, Mat m1, int n, int r0, int tid, Staged<DH>& s) {
  using S = Staged<DH>;
#pragma unroll
  for (int i = 0; i < S::NT; ++i) {
    const int t = tid + XT * i, r = t / S::V, c = (t - r * S::V) * 8;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      s.v[w][i][0] = s.v[w][i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t < S::TASKS && r0 + r < n) {                     // rows >= n (and blocks past the last) zero
        const Mat& m = w ? m1 : m0;
        const float4* g = reinterpret_cast<const float4*>(m.p + (size_t)(r0 + r) * m.ld + c);
        s.v[w][i][0] = g[0];
        s.v[w][i][1] = g[1];
      }
    }
  }
}

template <int DH>
__device__ __forceinline__ void stage_store(const Staged<DH>& s, bf16* l0, bf16* l1, int tid) {
  using S = Staged<DH>;
#pragma unroll
  for (int i = 0; i < S::NT; ++i) {
    const int t = tid + XT * i, r = t / S::V, c = (t - r * S::V) * 8;
    if (t < S::TASKS) {
      *reinterpret_cast<bf16x8*>(l0 + r * (DH + 8) + c) = cvt8(s.v[0][i][0], s.v[0][i][1]);
      *reinterpret_cast<bf16x8*>(l1 + r * (DH + 8) + c) = cvt8(s.v[1][i][0], s.v[1][i][1]);
    }
  }
}

// ---------------------------------------------------------------- forward
template <int DH>
__global__ __launch_bounds__(XT) void mhsa_mfma_fwd_kernel(MmArgs a) {
  __shared__ __attribute__((aligned(16))) bf16 kb[XB * (DH + 8)];
  __shared__ __attribute__((aligned(16))) bf16 vb[XB * (DH + 8)];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int g = lane >> 4, r16 = lane & 15;
  const int row0 = blockIdx.x * XQ + wave * 16, row = row0 + r16;
  const int h = blockIdx.y, n = blockIdx.z, T = a.T;
  const Mat mk = head<DH>(a.k, a.ldk, n, h, T), mv = head<DH>(a.v, a.ldv, n, h, T);
  const unsigned long long sh = ((unsigned long long)n * a.heads + h) * T;
  const unsigned long long seed = site_seed(a);
  bf16x8 own[DH / 32];
  own_frags<DH>(head<DH>(a.q, a.ldq, n, h, T), T, row0, lane, own);
  f4 acc[DH / 16];
#pragma unroll
  for (int t = 0; t < DH / 16; ++t) acc[t] = f4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  const int nblk = (T + XB - 1) / XB;
  Staged<DH> sg;
  stage_load<DH>(mk, mv, T, 0, tid, sg);
  for (int b = 0; b < nblk; ++b) {
    __syncthreads();                          // block b - 1 no longer read
    stage_store<DH>(sg, kb, vb, tid);
    stage_load<DH>(mk, mv, T, (b + 1) * XB, tid, sg);     // in flight while block b is computed
    __syncthreads();
    f4 st[2];
    scores<DH>(kb, own, lane, st);
    float v[8], bm = -INFINITY;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = b * XB + 16 * hh + 4 * g + e;
        const float s = j < T ? st[hh][e] * a.scale : -INFINITY;   // keys past T: out of max and sum
        v[4 * hh + e] = s;
        bm = fmaxf(bm, s);
      }
    bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
    bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
    const float mn = fmaxf(m, bm);            // finite from block 0 on (key 0 exists: T >= 1)
    const float sc = __expf(m - mn);
    float p[8], ps = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      p[e] = __expf(v[e] - mn);
      ps += p[e];
    }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    l = l * sc + ps;                          // the unmasked row sum
    m = mn;
    if (a.p > 0.f) {
      const unsigned long long key0 = (sh + row) * T + b * XB + 4 * g;
#pragma unroll
      for (int e = 0; e < 8; ++e) p[e] *= dropout_scale(seed, key0 + 16 * (e >> 2) + (e & 3), a.p);
    }
#pragma unroll
    for (int t = 0; t < DH / 16; ++t) acc[t] *= sc;
    accum<DH, DH / 16>(vb, pack8(p), lane, 0, acc);
  }
  if (row < T) {
    const float il = 1.f / l;
    float* o = a.ctx + ((size_t)n * T + row) * a.ldo + (size_t)h * DH;
#pragma unroll
    for (int t = 0; t < DH / 16; ++t)
      *reinterpret_cast<float4*>(o + 16 * t + 4 * g) =
          make_float4(acc[t][0] * il, acc[t][1] * il, acc[t][2] * il, acc[t][3] * il);
    if (a.lse_out && g == 0) a.lse_out[sh + row] = m + logf(l);
  }
}

// ---------------------------------------------------------------- backward: rows (delta, dQ)
template <int DH>
__global__ __launch_bounds__(XT) void mhsa_mfma_bwd_rows_kernel(MmArgs a) {
  __shared__ __attribute__((aligned(16))) bf16 kb[XB * (DH + 8)];
  __shared__ __attribute__((aligned(16))) bf16 vb[XB * (DH + 8)];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int g = lane >> 4, r16 = lane & 15;
  const int row0 = blockIdx.x * XQ + wave * 16, row = row0 + r16;
  const int h = blockIdx.y, n = blockIdx.z, T = a.T;
  const Mat mk = head<DH>(a.k, a.ldk, n, h, T), mv = head<DH>(a.v, a.ldv, n, h, T);
  const unsigned long long sh = ((unsigned long long)n * a.heads + h) * T;
  const unsigned long long seed = site_seed(a);
  bf16x8 oq[DH / 32], od[DH / 32];
  own_frags<DH>(head<DH>(a.q, a.ldq, n, h, T), T, row0, lane, oq);
  own_frags<DH>(head<DH>(a.go, a.ldo, n, h, T), T, row0, lane, od);
  const float lse = row < T ? a.lse[sh + row] : INFINITY;          // rows past T: p = 0
  const int nblk = (T + XB - 1) / XB;
  // delta = c + dc, c = the dP of the row's largest P, dc = sum_j P (dP - c) / sum_j P: the top
  // key's own term is exactly zero, so dS = P ((dP - c) - dc) keeps its relative accuracy in a
  // nearly one-hot row (xattn_bwd_rows_kernel has the argument)
  float c = 0.f, pm = -1.f, sp = 0.f, dcs = 0.f, dc = 0.f;
  f4 acc[DH / 16];
#pragma unroll
  for (int t = 0; t < DH / 16; ++t) acc[t] = f4{0.f, 0.f, 0.f, 0.f};
  Staged<DH> sg;
  stage_load<DH>(mk, mv, T, 0, tid, sg);
  for (int pass = 0; pass < 2; ++pass) {
    for (int b = 0; b < nblk; ++b) {
      __syncthreads();
      stage_store<DH>(sg, kb, vb, tid);
      // the next block of this sweep, block 0 of the second sweep, or past the end (loads nothing)
      const int nb = b + 1 < nblk ? b + 1 : (pass == 0 ? 0 : nblk);
      stage_load<DH>(mk, mv, T, nb * XB, tid, sg);
      __syncthreads();
      f4 st[2], dp[2];
      scores<DH>(kb, oq, lane, st);
      scores<DH>(vb, od, lane, dp);
      float p[8];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int j = b * XB + 16 * hh + 4 * g + e;
          p[4 * hh + e] = j < T ? __expf(st[hh][e] * a.scale - lse) : 0.f;
        }
      if (a.p > 0.f) {                          // dP = (dO V^T) o M
        const unsigned long long key0 = (sh + row) * T + b * XB + 4 * g;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
          for (int e = 0; e < 4; ++e) dp[hh][e] *= dropout_scale(seed, key0 + 16 * hh + e, a.p);
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
        for (int mm = 16; mm <= 32; mm <<= 1) {
          const float op = __shfl_xor(bp, mm, 64), oc = __shfl_xor(bc, mm, 64);
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
        accum<DH, DH / 16>(kb, pack8(ds), lane, 0, acc);
      }
    }
    if (pass == 0) {
      dc = sp > 0.f ? dcs / sp : 0.f;           // rows past T: every P is zero
      if (g == 0 && row < T) a.delta[sh + row] = c + dc;
    }
  }
  if (row < T) {
    float* o = a.dq + ((size_t)n * T + row) * a.lddq + (size_t)h * DH;
#pragma unroll
    for (int t = 0; t < DH / 16; ++t)
      *reinterpret_cast<float4*>(o + 16 * t + 4 * g) =
          make_float4(a.scale * acc[t][0], a.scale * acc[t][1], a.scale * acc[t][2], a.scale * acc[t][3]);
  }
}

// ---------------------------------------------------------------- backward: columns (dK, dV)
// after the rows pass (reads its delta)
template <int DH>
__global__ __launch_bounds__(XT) void mhsa_mfma_bwd_cols_kernel(MmArgs a) {
  __shared__ __attribute__((aligned(16))) bf16 qb[XB * (DH + 8)];
  __shared__ __attribute__((aligned(16))) bf16 ob[XB * (DH + 8)];
  __shared__ float lb[XB], db[XB];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int g = lane >> 4, r16 = lane & 15;
  const int col0 = blockIdx.x * XQ + wave * 16, col = col0 + r16;
  const int h = blockIdx.y, n = blockIdx.z, T = a.T;
  const Mat mq = head<DH>(a.q, a.ldq, n, h, T), mo = head<DH>(a.go, a.ldo, n, h, T);
  const unsigned long long sh = ((unsigned long long)n * a.heads + h) * T;
  const unsigned long long seed = site_seed(a);
  bf16x8 ok[DH / 32], ov[DH / 32];
  own_frags<DH>(head<DH>(a.k, a.ldk, n, h, T), T, col0, lane, ok);
  own_frags<DH>(head<DH>(a.v, a.ldv, n, h, T), T, col0, lane, ov);
  const int nblk = (T + XB - 1) / XB;
  f4 av[DH / 16], ak[DH / 16];
#pragma unroll
  for (int t = 0; t < DH / 16; ++t) av[t] = ak[t] = f4{0.f, 0.f, 0.f, 0.f};
  Staged<DH> sg;
  stage_load<DH>(mq, mo, T, 0, tid, sg);
  for (int b = 0; b < nblk; ++b) {
    __syncthreads();
    stage_store<DH>(sg, qb, ob, tid);
    stage_load<DH>(mq, mo, T, (b + 1) * XB, tid, sg);     // in flight while block b is computed
    if (tid < XB) {
      const int i = b * XB + tid;
      lb[tid] = i < T ? a.lse[sh + i] : INFINITY;           // queries past T: p = 0
      db[tid] = i < T ? a.delta[sh + i] : 0.f;
    }
    __syncthreads();
    f4 st[2], dp[2];
    scores<DH>(qb, ok, lane, st);
    scores<DH>(ob, ov, lane, dp);
    float p[8], ds[8];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ri = 16 * hh + 4 * g + e;
        float pv = col < T ? __expf(st[hh][e] * a.scale - lb[ri]) : 0.f;
        float dpv = dp[hh][e];
        if (a.p > 0.f) {
          const float mk = dropout_scale(seed, (sh + b * XB + ri) * T + col, a.p);
          dpv *= mk;
          ds[4 * hh + e] = pv * (dpv - db[ri]);
          pv *= mk;                                         // dV takes P o M
        } else {
          ds[4 * hh + e] = pv * (dpv - db[ri]);
        }
        p[4 * hh + e] = pv;
      }
    accum<DH, DH / 16>(ob, pack8(p), lane, 0, av);
    accum<DH, DH / 16>(qb, pack8(ds), lane, 0, ak);
  }
  if (col < T) {
    float* ovp = a.dv + ((size_t)n * T + col) * a.lddv + (size_t)h * DH;
    float* okp = a.dk + ((size_t)n * T + col) * a.lddk + (size_t)h * DH;
#pragma unroll
    for (int t = 0; t < DH / 16; ++t) {
      *reinterpret_cast<float4*>(ovp + 16 * t + 4 * g) = make_float4(av[t][0], av[t][1], av[t][2], av[t][3]);
      *reinterpret_cast<float4*>(okp + 16 * t + 4 * g) =
          make_float4(a.scale * ak[t][0], a.scale * ak[t][1], a.scale * ak[t][2], a.scale * ak[t][3]);
    }
  }
}

constexpr int MM_TMAX = 256;

int mm_shape(int N, int heads, int T, int dh) {
  if (!(dh == 32 || dh == 64 || dh == 128) || heads < 1 || heads > 65535 || T < 1 || T > MM_TMAX ||
      N < 1 || N > 65535)
    return AVD_ERR_SHAPE;
  return AVD_OK;
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int DH>
void mm_launch(int which, const MmArgs& a, int N, hipStream_t st) {
  const dim3 grid((a.T + XQ - 1) / XQ, a.heads, N);
  if (which == 0) mhsa_mfma_fwd_kernel<DH><<<grid, XT, 0, st>>>(a);
  else if (which == 1) mhsa_mfma_bwd_rows_kernel<DH><<<grid, XT, 0, st>>>(a);
  else mhsa_mfma_bwd_cols_kernel<DH><<<grid, XT, 0, st>>>(a);
}

void mm_dispatch(int which, const MmArgs& a, int N, int dh, hipStream_t st) {
  if (dh == 32) mm_launch<32>(which, a, N, st);
  else if (dh == 64) mm_launch<64>(which, a, N, st);
  else mm_launch<128>(which, a, N, st);
}

}  // namespace

extern "C" {

int avd_mhsa_mfma_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v,
                      long long ldv, float* ctx, long long ldo, float* lse, int N, int heads, int T, int dh,
                      float scale, float p, unsigned long long seed, const unsigned long long* seed_off,
                      void* stream) {
  if (mm_shape(N, heads, T, dh) != AVD_OK) return AVD_ERR_SHAPE;
  if (!q || !k || !v || !ctx || !(p >= 0.f && p < 1.f)) return AVD_ERR_ARG;
  const long long E = (long long)heads * dh;
  if (ldq < E || ldk < E || ldv < E || ldo < E || (ldq | ldk | ldv | ldo) % 4 != 0) return AVD_ERR_ARG;
  if (!al16(q) || !al16(k) || !al16(v) || !al16(ctx)) return AVD_ERR_ARG;
  MmArgs a{};
  a.q = q; a.k = k; a.v = v; a.ctx = ctx; a.lse_out = lse;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
  a.heads = heads; a.T = T; a.scale = scale; a.p = p; a.seed = seed; a.seed_off = seed_off;
  mm_dispatch(0, a, N, dh, avd_stream(stream));
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

long long avd_mhsa_mfma_bwd_ws(int N, int heads, int T, int dh) {
  if (mm_shape(N, heads, T, dh) != AVD_OK) return -1;
  return (long long)N * heads * T;        // delta, one float per query row
}

int avd_mhsa_mfma_bwd(const float* dout, long long lddo, const float* q, long long ldq, const float* k,
                      long long ldk, const float* v, long long ldv, const float* lse, float* dq,
                      long long lddq, float* dk, long long lddk, float* dv, long long lddv, float* ws,
                      long long ws_elems, int N, int heads, int T, int dh, float scale, float p,
                      unsigned long long seed, const unsigned long long* seed_off, void* stream) {
  if (mm_shape(N, heads, T, dh) != AVD_OK) return AVD_ERR_SHAPE;
  if (!dout || !q || !k || !v || !lse || !dq || !dk || !dv || !ws || !(p >= 0.f && p < 1.f))
    return AVD_ERR_ARG;
  if (ws_elems < (long long)N * heads * T) return AVD_ERR_ARG;
  const long long E = (long long)heads * dh;
  if (lddo < E || ldq < E || ldk < E || ldv < E || lddq < E || lddk < E || lddv < E ||
      (lddo | ldq | ldk | ldv | lddq | lddk | lddv) % 4 != 0)
    return AVD_ERR_ARG;
  if (!al16(dout) || !al16(q) || !al16(k) || !al16(v) || !al16(dq) || !al16(dk) || !al16(dv))
    return AVD_ERR_ARG;
  MmArgs a{};
  a.q = q; a.k = k; a.v = v; a.go = dout; a.lse = lse; a.delta = ws;
  a.dq = dq; a.dk = dk; a.dv = dv;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = lddo; a.lddq = lddq; a.lddk = lddk; a.lddv = lddv;
  a.heads = heads; a.T = T; a.scale = scale; a.p = p; a.seed = seed; a.seed_off = seed_off;
  mm_dispatch(1, a, N, dh, avd_stream(stream));
  AVD_CHECK_LAUNCH();
  mm_dispatch(2, a, N, dh, avd_stream(stream));
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

}  // extern "C"
