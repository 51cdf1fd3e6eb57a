// The ViT encoders' kernels (AudioViTEncoder, models/dino_vit.py:27-63, 122-177, over
// nn.TransformerEncoderLayer): multi-head self-attention, residual + dropout + LayerNorm,
// GELU + dropout, patch rows and the token assembly.  Every GEMM around them is avd_gemm /
// avd_linear_bwd.
//
// Attention: one workgroup of 256 threads owns 16 rows of one (sequence, head) -- query rows in the
// forward and in the backward's row pass (delta, dQ), key rows in its column pass (dK, dV).  The
// other side's T <= 256 rows are one per thread: the thread holds its row in registers and forms
// its 16 scores against the tile in LDS with f32 fma; the [16][T] score / probability tile lives
// in LDS and never reaches HBM.  dt = AVD_BF16 rounds the MFMA operands of the tuned design (Q, K,
// V, dO, the probabilities fed to P V and P^T dO, dS) to bf16 and accumulates in f32 on the
// VALU; dt = AVD_F32 rounds nothing.  No atomics, every sum in a fixed order.
#include "common.h"

namespace avd {

constexpr int MH_TILE = 16;     // rows of the tile side
constexpr int MH_TMAX = 256;    // tokens = threads of the per-thread side
constexpr int MH_NT = 256;

template <bool BF>
__device__ __forceinline__ float rnd_op(float v) { return BF ? bf2f(f2bf(v)) : v; }

// row [DH] of a strided matrix into registers, rounded
template <int DH, bool BF>
__device__ __forceinline__ void load_row(const float* __restrict__ p, float (&r)[DH]) {
#pragma unroll
  for (int c = 0; c < DH; c += 4) {
    const float4 v = *reinterpret_cast<const float4*>(p + c);
    r[c] = rnd_op<BF>(v.x); r[c + 1] = rnd_op<BF>(v.y);
    r[c + 2] = rnd_op<BF>(v.z); r[c + 3] = rnd_op<BF>(v.w);
  }
}

// rows [nrows][DH] of a strided matrix (leading dimension ld) into tile[MH_TILE][DH], rounded;
// rows past nrows are zero
template <int DH, bool BF>
__device__ __forceinline__ void load_tile(const float* __restrict__ p, long long ld, int nrows,
                                          float* tile) {
  for (int e = threadIdx.x; e < MH_TILE * DH; e += MH_NT) {
    const int i = e / DH, c = e - i * DH;
    tile[e] = i < nrows ? rnd_op<BF>(p[(long long)i * ld + c]) : 0.f;
  }
}

template <int DH>
__device__ __forceinline__ float dot_tile(const float (&r)[DH], const float* trow) {
  float a = 0.f;
#pragma unroll
  for (int c = 0; c < DH; c += 4) {
    const float4 t = *reinterpret_cast<const float4*>(trow + c);
    a = fmaf(r[c], t.x, a); a = fmaf(r[c + 1], t.y, a);
    a = fmaf(r[c + 2], t.z, a); a = fmaf(r[c + 3], t.w, a);
  }
  return a;
}

// out[i][c] = alpha * sum_{j<T} w[i][j] m[j][c] for the tile's nrows rows: thread (c, row group)
// walks j, reading m coalesced across c; w [MH_TILE][MH_TMAX] in LDS
template <int DH, bool BF>
__device__ __forceinline__ void tile_matmul(const float* w, const float* __restrict__ m, long long ldm,
                                            int T, int nrows, float alpha, float* __restrict__ out,
                                            long long ldo) {
  constexpr int RG = MH_NT / DH;          // row groups: 8 / 4 / 2
  constexpr int RPT = MH_TILE / RG;       // rows per thread: 2 / 4 / 8
  const int c = threadIdx.x % DH, rg = threadIdx.x / DH;
  float acc[RPT];
#pragma unroll
  for (int k = 0; k < RPT; ++k) acc[k] = 0.f;
  for (int j = 0; j < T; ++j) {
    const float v = rnd_op<BF>(m[(long long)j * ldm + c]);
#pragma unroll
    for (int k = 0; k < RPT; ++k) acc[k] = fmaf(w[(rg * RPT + k) * MH_TMAX + j], v, acc[k]);
  }
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const int i = rg * RPT + k;
    if (i < nrows) out[(long long)i * ldo + c] = alpha * acc[k];
  }
}

struct MhsaArgs {
  const float *q, *k, *v, *dout, *lse_in, *delta_in;
  float *ctx, *lse, *dq, *dk, *dv, *delta;
  long long ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
  long long nall;       // N heads T: the rows of one ws section
  int T, heads;
  float scale, p;
  unsigned long long seed;
  const unsigned long long* seed_off;
};

// ---- forward: ctx = dropout(softmax(scale Q K^T)) V for 16 query rows
template <int DH, bool BF>
__global__ __launch_bounds__(MH_NT) void mhsa_fwd_kernel(MhsaArgs a) {
  __shared__ __attribute__((aligned(16))) float qt[MH_TILE * DH];
  __shared__ float s[MH_TILE * MH_TMAX];
  const int T = a.T, h = blockIdx.y, n = blockIdx.z, i0 = blockIdx.x * MH_TILE;
  const int nrows = min(MH_TILE, T - i0);
  const long long seq = (long long)n * T;
  const float* q = a.q + (seq + i0) * a.ldq + h * DH;
  const float* k = a.k + seq * a.ldk + h * DH;
  const float* v = a.v + seq * a.ldv + h * DH;
  unsigned long long seed = a.seed;
  if (a.p > 0.f && a.seed_off) seed += a.seed_off[0];
  load_tile<DH, BF>(q, a.ldq, nrows, qt);
  __syncthreads();
  const int j = threadIdx.x;
  if (j < T) {
    float kr[DH];
    load_row<DH, BF>(k + (long long)j * a.ldk, kr);
    for (int i = 0; i < nrows; ++i) s[i * MH_TMAX + j] = a.scale * dot_tile<DH>(kr, qt + i * DH);
  }
  __syncthreads();
  // row softmax: wave w owns rows w, w + 4, ...
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  for (int i = w; i < nrows; i += MH_NT / 64) {
    float m = -INFINITY;
    for (int jj = l; jj < T; jj += 64) m = fmaxf(m, s[i * MH_TMAX + jj]);
    m = wave_max(m);
    float sum = 0.f;
    for (int jj = l; jj < T; jj += 64) sum += expf(s[i * MH_TMAX + jj] - m);
    sum = wave_sum(sum);
    const float rsum = 1.f / sum;
    const unsigned long long key0 = (((unsigned long long)n * a.heads + h) * T + (i0 + i)) * T;
    for (int jj = l; jj < T; jj += 64) {
      float pr = expf(s[i * MH_TMAX + jj] - m) * rsum;     // (not exp(s - lse): lse rounds at |lse| eps)
      if (a.p > 0.f) pr *= dropout_scale(seed, key0 + jj, a.p);
      s[i * MH_TMAX + jj] = rnd_op<BF>(pr);
    }
    if (a.lse && l == 0) a.lse[((long long)n * a.heads + h) * T + i0 + i] = m + logf(sum);
  }
  __syncthreads();
  tile_matmul<DH, BF>(s, v, a.ldv, T, nrows, 1.f, a.ctx + (seq + i0) * a.ldo + h * DH, a.ldo);
}

// Sum over the 256 threads of v[i], i < 16, in double: a wave tree each, then the four waves in
// order.  out [16] and red [4][16] in LDS; out is valid for every thread on return.
__device__ __forceinline__ void tile_rows_sum_d(const double (&v)[MH_TILE], double (*red)[MH_TILE],
                                                double* out) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < MH_TILE; ++i) {
    const double t = wave_sum_d(v[i]);
    if (l == 0) red[w][i] = t;
  }
  __syncthreads();
  if (threadIdx.x < MH_TILE) {
    const int t = threadIdx.x;
    out[t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  }
  __syncthreads();
}

// The backward's probabilities and delta.  P is recomputed as exp(S - lse) and renormalised by its
// own row sum (corr = 1 / sum_j exp(S - lse), 1 up to the f32 rounding of lse, which at |lse| ~ 100
// is 7e-6 relative).  dS = P o (dP - delta) cancels: in a row whose softmax is nearly one-hot
// dP_top - delta is (1 - P_top) |dP|, while an f32 delta = sum_j P dP is only good to 6e-8 |dP|.
// So delta = sum_j P dP / sum_j P is formed in double from the very P and dP that enter dS -- then
// dP_j - delta = sum_l P_l (dP_j - dP_l) / sum_l P_l, which is well conditioned -- and handed to
// the column pass as a (hi, lo) pair of floats.  ws: corr [n] | delta hi [n] | delta lo [n], n =
// N heads T rows.

// ---- backward, row pass: corr, delta and dQ = scale dS K for 16 query rows
template <int DH, bool BF>
__global__ __launch_bounds__(MH_NT) void mhsa_bwd_row_kernel(MhsaArgs a) {
  __shared__ __attribute__((aligned(16))) float qt[MH_TILE * DH];    // Q, then dO
  __shared__ float s[MH_TILE * MH_TMAX];
  __shared__ double red[MH_NT / 64][MH_TILE];
  __shared__ double sp[MH_TILE], spd[MH_TILE];
  const int T = a.T, h = blockIdx.y, n = blockIdx.z, i0 = blockIdx.x * MH_TILE;
  const int nrows = min(MH_TILE, T - i0);
  const long long seq = (long long)n * T;
  const long long sh = ((long long)n * a.heads + h) * T;
  const float* k = a.k + seq * a.ldk + h * DH;
  unsigned long long seed = a.seed;
  if (a.p > 0.f && a.seed_off) seed += a.seed_off[0];
  const int j = threadIdx.x;
  float pr[MH_TILE], dp[MH_TILE];
  double acc[MH_TILE];
#pragma unroll
  for (int i = 0; i < MH_TILE; ++i) pr[i] = dp[i] = 0.f;
  load_tile<DH, BF>(a.q + (seq + i0) * a.ldq + h * DH, a.ldq, nrows, qt);
  __syncthreads();
  if (j < T) {
    float r[DH];
    load_row<DH, BF>(k + (long long)j * a.ldk, r);
#pragma unroll
    for (int i = 0; i < MH_TILE; ++i)
      if (i < nrows) pr[i] = expf(a.scale * dot_tile<DH>(r, qt + i * DH) - a.lse_in[sh + i0 + i]);
  }
#pragma unroll
  for (int i = 0; i < MH_TILE; ++i) acc[i] = (double)pr[i];
  tile_rows_sum_d(acc, red, sp);          // (its barriers also close the reads of the Q tile)
#pragma unroll
  for (int i = 0; i < MH_TILE; ++i)
    if (i < nrows) pr[i] *= (float)(1.0 / sp[i]);
  if (j < nrows) a.delta[sh + i0 + j] = (float)(1.0 / sp[j]);
  __syncthreads();
  load_tile<DH, BF>(a.dout + (seq + i0) * a.lddo + h * DH, a.lddo, nrows, qt);
  __syncthreads();
  if (j < T) {
    float r[DH];
    load_row<DH, BF>(a.v + (seq + j) * a.ldv + h * DH, r);
#pragma unroll
    for (int i = 0; i < MH_TILE; ++i) {
      if (i >= nrows) continue;
      dp[i] = dot_tile<DH>(r, qt + i * DH);
      if (a.p > 0.f) dp[i] *= dropout_scale(seed, (unsigned long long)(sh + i0 + i) * T + j, a.p);
    }
  }
#pragma unroll
  for (int i = 0; i < MH_TILE; ++i) acc[i] = (double)pr[i];
  tile_rows_sum_d(acc, red, sp);
#pragma unroll
  for (int i = 0; i < MH_TILE; ++i) acc[i] = (double)pr[i] * (double)dp[i];
  tile_rows_sum_d(acc, red, spd);
  if (j < nrows) {
    const double d = spd[j] / sp[j];
    const float hi = (float)d;
    a.delta[a.nall + sh + i0 + j] = hi;
    a.delta[2 * a.nall + sh + i0 + j] = (float)(d - (double)hi);
  }
  if (j < T) {
#pragma unroll
    for (int i = 0; i < MH_TILE; ++i)      // dS = P o (dP - delta)
      s[i * MH_TMAX + j] =
          i < nrows ? rnd_op<BF>(pr[i] * (float)((double)dp[i] - spd[i] / sp[i])) : 0.f;
  }
  __syncthreads();
  tile_matmul<DH, BF>(s, k, a.ldk, T, nrows, a.scale, a.dq + (seq + i0) * a.lddq + h * DH, a.lddq);
}

// ---- backward, column pass: dK = scale dS^T Q and dV = Pd^T dO for 16 key rows
template <int DH, bool BF>
__global__ __launch_bounds__(MH_NT) void mhsa_bwd_col_kernel(MhsaArgs a) {
  __shared__ __attribute__((aligned(16))) float kt[MH_TILE * DH];    // K, then V
  __shared__ float ds[MH_TILE * MH_TMAX];
  __shared__ float pd[MH_TILE * MH_TMAX];
  const int T = a.T, h = blockIdx.y, n = blockIdx.z, j0 = blockIdx.x * MH_TILE;
  const int nrows = min(MH_TILE, T - j0);
  const long long seq = (long long)n * T;
  const long long sh = ((long long)n * a.heads + h) * T;
  const float* q = a.q + seq * a.ldq + h * DH;
  const float* dout = a.dout + seq * a.lddo + h * DH;
  unsigned long long seed = a.seed;
  if (a.p > 0.f && a.seed_off) seed += a.seed_off[0];
  const int i = threadIdx.x;
  float pr[MH_TILE];
  load_tile<DH, BF>(a.k + (seq + j0) * a.ldk + h * DH, a.ldk, nrows, kt);
  __syncthreads();
  if (i < T) {
    float r[DH];
    load_row<DH, BF>(q + (long long)i * a.ldq, r);
    const float lse = a.lse_in[sh + i], corr = a.delta_in[sh + i];
#pragma unroll
    for (int jj = 0; jj < MH_TILE; ++jj)
      pr[jj] = jj < nrows ? expf(a.scale * dot_tile<DH>(r, kt + jj * DH) - lse) * corr : 0.f;
  }
  __syncthreads();
  load_tile<DH, BF>(a.v + (seq + j0) * a.ldv + h * DH, a.ldv, nrows, kt);
  __syncthreads();
  if (i < T) {
    float r[DH];
    load_row<DH, BF>(dout + (long long)i * a.lddo, r);
    const double delta = (double)a.delta_in[a.nall + sh + i] + (double)a.delta_in[2 * a.nall + sh + i];
#pragma unroll
    for (int jj = 0; jj < MH_TILE; ++jj) {
      float m = 1.f;
      if (a.p > 0.f && jj < nrows)
        m = dropout_scale(seed, (unsigned long long)(sh + i) * T + j0 + jj, a.p);
      const float dp = dot_tile<DH>(r, kt + jj * DH) * m;
      ds[jj * MH_TMAX + i] = rnd_op<BF>(pr[jj] * (float)((double)dp - delta));
      pd[jj * MH_TMAX + i] = rnd_op<BF>(pr[jj] * m);
    }
  }
  __syncthreads();
  tile_matmul<DH, BF>(ds, q, a.ldq, T, nrows, a.scale, a.dk + (seq + j0) * a.lddk + h * DH, a.lddk);
  tile_matmul<DH, BF>(pd, dout, a.lddo, T, nrows, 1.f, a.dv + (seq + j0) * a.lddv + h * DH, a.lddv);
}

// ---------------------------------------------------------------- LayerNorm
constexpr int LN_EMAX = 512;
constexpr int LN_PER = LN_EMAX / 64;     // elements per lane
constexpr int LN_NT = 256;

// y = LayerNorm(x + dropout(r)): one wave per row
__global__ __launch_bounds__(LN_NT) void ln_fwd_kernel(
    const float* __restrict__ x, long long ldx, const float* __restrict__ r, long long ldr,
    const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ y,
    long long ldy, float* __restrict__ z, float* __restrict__ mean, float* __restrict__ rstd,
    int rows, int E, float eps, float p, unsigned long long seed,
    const unsigned long long* __restrict__ seed_off) {
  const int row = blockIdx.x * (LN_NT / 64) + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (row >= rows) return;
  if (p > 0.f && seed_off) seed += seed_off[0];
  float v[LN_PER];
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < LN_PER; ++k) {
    const int c = l + 64 * k;
    v[k] = 0.f;
    if (c < E) {
      v[k] = x[(long long)row * ldx + c];
      if (r) v[k] += r[(long long)row * ldr + c] * dropout_scale(seed, (unsigned long long)row * E + c, p);
      if (z) z[(long long)row * E + c] = v[k];
    }
    sum += v[k];
  }
  const float mu = wave_sum(sum) / (float)E;
  float sq = 0.f;
#pragma unroll
  for (int k = 0; k < LN_PER; ++k) {
    const float d = (l + 64 * k < E) ? v[k] - mu : 0.f;
    sq = fmaf(d, d, sq);
  }
  const float rs = 1.0f / sqrtf(wave_sum(sq) / (float)E + eps);
#pragma unroll
  for (int k = 0; k < LN_PER; ++k) {
    const int c = l + 64 * k;
    if (c < E) y[(long long)row * ldy + c] = fmaf((v[k] - mu) * rs, gamma[c], beta[c]);
  }
  if (l == 0) {
    if (mean) mean[row] = mu;
    if (rstd) rstd[row] = rs;
  }
}

// dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma; dr = mask dx; per-block column
// partials of (dy xhat, dy) into parts[block][2][E]; a wave walks the block's rows in order
__global__ __launch_bounds__(LN_NT) void ln_bwd_kernel(
    const float* __restrict__ dy, long long lddy, const float* __restrict__ z,
    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma,
    float* __restrict__ dx, long long lddx, float* __restrict__ dr, long long lddr,
    float* __restrict__ parts, int rows, int E, int rpb, float p, unsigned long long seed,
    const unsigned long long* __restrict__ seed_off) {
  __shared__ float sh[LN_NT / 64][2][LN_EMAX];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (p > 0.f && seed_off) seed += seed_off[0];
  const int r0 = blockIdx.x * rpb, r1 = min(rows, r0 + rpb);
  float ag[LN_PER], ab[LN_PER], gm[LN_PER];
#pragma unroll
  for (int k = 0; k < LN_PER; ++k) {
    ag[k] = ab[k] = 0.f;
    gm[k] = (l + 64 * k < E) ? gamma[l + 64 * k] : 0.f;
  }
  for (int row = r0 + w; row < r1; row += LN_NT / 64) {
    const float mu = mean[row], rs = rstd[row];
    float d[LN_PER], xh[LN_PER];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < LN_PER; ++k) {
      const int c = l + 64 * k;
      d[k] = xh[k] = 0.f;
      if (c < E) {
        d[k] = dy[(long long)row * lddy + c];
        xh[k] = (z[(long long)row * E + c] - mu) * rs;
      }
      ag[k] = fmaf(d[k], xh[k], ag[k]);
      ab[k] += d[k];
      const float g = d[k] * gm[k];
      s1 += g;
      s2 = fmaf(g, xh[k], s2);
    }
    s1 = wave_sum(s1) / (float)E;
    s2 = wave_sum(s2) / (float)E;
#pragma unroll
    for (int k = 0; k < LN_PER; ++k) {
      const int c = l + 64 * k;
      if (c < E) {
        const float g = rs * (d[k] * gm[k] - s1 - xh[k] * s2);
        dx[(long long)row * lddx + c] = g;
        if (dr) dr[(long long)row * lddr + c] = g * dropout_scale(seed, (unsigned long long)row * E + c, p);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < LN_PER; ++k) {
    const int c = l + 64 * k;
    if (c < E) { sh[w][0][c] = ag[k]; sh[w][1][c] = ab[k]; }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * E; e += LN_NT) {
    const int t = e / E, c = e - t * E;
    float a = 0.f;
#pragma unroll
    for (int ww = 0; ww < LN_NT / 64; ++ww) a += sh[ww][t][c];
    parts[((long long)blockIdx.x * 2 + t) * E + c] = a;
  }
}

// dgamma[c] = sum_b parts[b][0][c], dbeta[c] = sum_b parts[b][1][c], in block order
__global__ void ln_bwd_reduce_kernel(const float* __restrict__ parts, int blocks, int E,
                                     float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 2 * E) return;
  double a = 0.0;
  for (int b = 0; b < blocks; ++b) a += (double)parts[(long long)b * 2 * E + e];
  if (e < E) dgamma[e] = (float)a; else dbeta[e - E] = (float)a;
}

// ---------------------------------------------------------------- GELU + dropout
__device__ __forceinline__ float vgelu_f(float z) { return 0.5f * z * (1.f + erff(z * 0.70710678118654752f)); }
__device__ __forceinline__ float vgelu_d(float z) {
  return 0.5f * (1.f + erff(z * 0.70710678118654752f)) + z * 0.39894228040143268f * expf(-0.5f * z * z);
}

__global__ void gelu_fwd_kernel(const float* __restrict__ x, float* __restrict__ out, long long n,
                                float p, unsigned long long seed,
                                const unsigned long long* __restrict__ seed_off) {
  if (p > 0.f && seed_off) seed += seed_off[0];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    out[i] = vgelu_f(x[i]) * dropout_scale(seed, (unsigned long long)i, p);
}

__global__ void gelu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dout,
                                float* __restrict__ dx, long long n, float p, unsigned long long seed,
                                const unsigned long long* __restrict__ seed_off) {
  if (p > 0.f && seed_off) seed += seed_off[0];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    dx[i] = dout[i] * dropout_scale(seed, (unsigned long long)i, p) * vgelu_d(x[i]);
}

// ---------------------------------------------------------------- patches and tokens
template <typename T>
__global__ void patchify_kernel(const T* __restrict__ x, float* __restrict__ out, int N, int H, int W,
                                int P) {
  const long long n = (long long)N * H * W;
  const int gw = W / P, gh = H / P;
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < n;
       o += (long long)gridDim.x * blockDim.x) {
    const int pw = (int)(o % P);
    long long t = o / P;
    const int ph = (int)(t % P); t /= P;
    const int gx = (int)(t % gw); t /= gw;
    const int gy = (int)(t % gh);
    const long long s = t / gh;
    out[o] = io<T>::ld(x, (s * H + (long long)gy * P + ph) * W + (long long)gx * P + pw);
  }
}

__global__ void tokens_fwd_kernel(const float* __restrict__ pe, const float* __restrict__ cls,
                                  const float* __restrict__ pos, float* __restrict__ tok, int N, int T,
                                  int E) {
  const long long n = (long long)N * T * E;
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < n;
       o += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(o % E);
    const long long rt = o / E;
    const int t = (int)(rt % T);
    const long long s = rt / T;
    const float v = t == 0 ? cls[c] : pe[(s * (T - 1) + t - 1) * E + c];
    tok[o] = v + pos[(long long)t * E + c];
  }
}

__global__ void tokens_bwd_kernel(const float* __restrict__ dtok, float* __restrict__ dpe, int N, int T,
                                  int E) {
  const long long n = (long long)N * (T - 1) * E;
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < n;
       o += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(o % E);
    const long long rt = o / E;
    const int t = (int)(rt % (T - 1));
    const long long s = rt / (T - 1);
    dpe[o] = dtok[(s * T + t + 1) * E + c];
  }
}

inline int ew_grid(long long n) { return (int)((n + 255) / 256 > 65536 ? 65536 : (n + 255) / 256); }

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int mhsa_shape(int N, int heads, int T, int dh) {
  if (!(dh == 32 || dh == 64 || dh == 128) || heads < 1 || T < 1 || T > MH_TMAX || N < 1 || N > 65535 ||
      heads > 65535)
    return AVD_ERR_SHAPE;
  return AVD_OK;
}

template <int DH, bool BF>
static void mhsa_launch(int which, const MhsaArgs& a, int N, hipStream_t st) {
  const dim3 grid((a.T + MH_TILE - 1) / MH_TILE, a.heads, N);
  if (which == 0) mhsa_fwd_kernel<DH, BF><<<grid, MH_NT, 0, st>>>(a);
  else if (which == 1) mhsa_bwd_row_kernel<DH, BF><<<grid, MH_NT, 0, st>>>(a);
  else mhsa_bwd_col_kernel<DH, BF><<<grid, MH_NT, 0, st>>>(a);
}

static void mhsa_dispatch(int which, const MhsaArgs& a, int N, int dh, int dt, hipStream_t st) {
  const bool bf = dt == AVD_BF16;
  if (dh == 32) bf ? mhsa_launch<32, true>(which, a, N, st) : mhsa_launch<32, false>(which, a, N, st);
  else if (dh == 64) bf ? mhsa_launch<64, true>(which, a, N, st) : mhsa_launch<64, false>(which, a, N, st);
  else bf ? mhsa_launch<128, true>(which, a, N, st) : mhsa_launch<128, false>(which, a, N, st);
}

}  // namespace avd

using namespace avd;

extern "C" {

int avd_mhsa_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v,
                 long long ldv, float* ctx, long long ldo, float* lse, int N, int heads, int T, int dh,
                 int dt, float scale, float p, unsigned long long seed,
                 const unsigned long long* seed_off, void* stream) {
  if (mhsa_shape(N, heads, T, dh) != AVD_OK) return AVD_ERR_SHAPE;
  if (dt != AVD_F32 && dt != AVD_BF16) return AVD_ERR_DTYPE;
  if (!q || !k || !v || !ctx || !(p >= 0.f && p < 1.f)) return AVD_ERR_ARG;
  const long long E = (long long)heads * dh;
  if (ldq < E || ldk < E || ldv < E || ldo < E || (ldq | ldk | ldv | ldo) % 4 != 0) return AVD_ERR_ARG;
  if (!al16(q) || !al16(k) || !al16(v) || !al16(ctx)) return AVD_ERR_ARG;
  MhsaArgs a{};
  a.q = q; a.k = k; a.v = v; a.ctx = ctx; a.lse = lse;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
  a.T = T; a.heads = heads; a.scale = scale; a.p = p; a.seed = seed; a.seed_off = seed_off;
  mhsa_dispatch(0, a, N, dh, dt, avd_stream(stream));
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

long long avd_mhsa_bwd_ws(int N, int heads, int T, int dh) {
  if (mhsa_shape(N, heads, T, dh) != AVD_OK) return -1;
  return 3ll * N * heads * T;
}

int avd_mhsa_bwd(const float* dout, long long lddo, const float* q, long long ldq, const float* k,
                 long long ldk, const float* v, long long ldv, const float* lse, float* dq,
                 long long lddq, float* dk, long long lddk, float* dv, long long lddv, float* ws,
                 long long ws_elems, int N, int heads, int T, int dh, int dt, float scale, float p,
                 unsigned long long seed, const unsigned long long* seed_off, void* stream) {
  if (mhsa_shape(N, heads, T, dh) != AVD_OK) return AVD_ERR_SHAPE;
  if (dt != AVD_F32 && dt != AVD_BF16) return AVD_ERR_DTYPE;
  if (!dout || !q || !k || !v || !lse || !dq || !dk || !dv || !ws || !(p >= 0.f && p < 1.f))
    return AVD_ERR_ARG;
  if (ws_elems < 3ll * N * heads * T) return AVD_ERR_ARG;
  const long long E = (long long)heads * dh;
  if (lddo < E || ldq < E || ldk < E || ldv < E || lddq < E || lddk < E || lddv < E ||
      (lddo | ldq | ldk | ldv | lddq | lddk | lddv) % 4 != 0)
    return AVD_ERR_ARG;
  if (!al16(dout) || !al16(q) || !al16(k) || !al16(v) || !al16(dq) || !al16(dk) || !al16(dv))
    return AVD_ERR_ARG;
  MhsaArgs a{};
  a.q = q; a.k = k; a.v = v; a.dout = dout; a.lse_in = lse; a.delta = ws; a.delta_in = ws;
  a.dq = dq; a.dk = dk; a.dv = dv;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.lddo = lddo; a.lddq = lddq; a.lddk = lddk; a.lddv = lddv;
  a.T = T; a.heads = heads; a.scale = scale; a.p = p; a.seed = seed; a.seed_off = seed_off;
  a.nall = (long long)N * heads * T;
  mhsa_dispatch(1, a, N, dh, dt, avd_stream(stream));
  AVD_CHECK_LAUNCH();
  mhsa_dispatch(2, a, N, dh, dt, avd_stream(stream));
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

static int ln_shape(int rows, int E) {
  return (rows >= 1 && E >= 32 && E <= LN_EMAX && E % 32 == 0) ? AVD_OK : AVD_ERR_SHAPE;
}

int avd_ln_fwd(const float* x, long long ldx, const float* r, long long ldr, const float* gamma,
               const float* beta, float* y, long long ldy, float* z, float* mean, float* rstd,
               int rows, int E, float eps, float p, unsigned long long seed,
               const unsigned long long* seed_off, void* stream) {
  if (ln_shape(rows, E) != AVD_OK) return AVD_ERR_SHAPE;
  if (!x || !gamma || !beta || !y || ldx < E || ldy < E || (r && ldr < E) || !(p >= 0.f && p < 1.f))
    return AVD_ERR_ARG;
  ln_fwd_kernel<<<avd_cdiv(rows, LN_NT / 64), LN_NT, 0, avd_stream(stream)>>>(
      x, ldx, r, ldr, gamma, beta, y, ldy, z, mean, rstd, rows, E, eps, r ? p : 0.f, seed, seed_off);
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

static int ln_blocks(int rows) {
  const int b = avd_cdiv(rows, 32);
  return b > 1024 ? 1024 : b;
}

long long avd_ln_bwd_ws(int rows, int E) {
  if (ln_shape(rows, E) != AVD_OK) return -1;
  return (long long)ln_blocks(rows) * 2 * E;
}

int avd_ln_bwd(const float* dy, long long lddy, const float* z, const float* mean, const float* rstd,
               const float* gamma, float* dx, long long lddx, float* dr, long long lddr, float* dgamma,
               float* dbeta, float* ws, long long ws_elems, int rows, int E, float p,
               unsigned long long seed, const unsigned long long* seed_off, void* stream) {
  if (ln_shape(rows, E) != AVD_OK) return AVD_ERR_SHAPE;
  if (!dy || !z || !mean || !rstd || !gamma || !dx || !dgamma || !dbeta || !ws || lddy < E || lddx < E ||
      (dr && lddr < E) || !(p >= 0.f && p < 1.f))
    return AVD_ERR_ARG;
  const int blocks = ln_blocks(rows);
  if (ws_elems < (long long)blocks * 2 * E) return AVD_ERR_ARG;
  const int rpb = avd_cdiv(rows, blocks);
  ln_bwd_kernel<<<blocks, LN_NT, 0, avd_stream(stream)>>>(dy, lddy, z, mean, rstd, gamma, dx, lddx, dr,
                                                          lddr, ws, rows, E, rpb, dr ? p : 0.f, seed,
                                                          seed_off);
  AVD_CHECK_LAUNCH();
  ln_bwd_reduce_kernel<<<avd_cdiv(2 * E, 256), 256, 0, avd_stream(stream)>>>(ws, blocks, E, dgamma, dbeta);
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

int avd_gelu_fwd(const float* x, float* out, long long rows, int C, float p, unsigned long long seed,
                 const unsigned long long* seed_off, void* stream) {
  if (rows < 1 || C < 1) return AVD_ERR_SHAPE;
  if (!x || !out || !(p >= 0.f && p < 1.f)) return AVD_ERR_ARG;
  const long long n = rows * C;
  gelu_fwd_kernel<<<ew_grid(n), 256, 0, avd_stream(stream)>>>(x, out, n, p, seed, seed_off);
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

int avd_gelu_bwd(const float* x, const float* dout, float* dx, long long rows, int C, float p,
                 unsigned long long seed, const unsigned long long* seed_off, void* stream) {
  if (rows < 1 || C < 1) return AVD_ERR_SHAPE;
  if (!x || !dout || !dx || !(p >= 0.f && p < 1.f)) return AVD_ERR_ARG;
  const long long n = rows * C;
  gelu_bwd_kernel<<<ew_grid(n), 256, 0, avd_stream(stream)>>>(x, dout, dx, n, p, seed, seed_off);
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

int avd_vit_patchify(const void* x, int dt, float* out, int N, int H, int W, int P, void* stream) {
  if (N < 1 || H < 1 || W < 1 || P < 1 || H % P != 0 || W % P != 0) return AVD_ERR_SHAPE;
  if (dt != AVD_F32 && dt != AVD_BF16) return AVD_ERR_DTYPE;
  if (!x || !out) return AVD_ERR_ARG;
  const long long n = (long long)N * H * W;
  if (dt == AVD_F32)
    patchify_kernel<float><<<ew_grid(n), 256, 0, avd_stream(stream)>>>((const float*)x, out, N, H, W, P);
  else
    patchify_kernel<bf16><<<ew_grid(n), 256, 0, avd_stream(stream)>>>((const bf16*)x, out, N, H, W, P);
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

int avd_vit_tokens_fwd(const float* pe, const float* cls, const float* pos, float* tok, int N, int T,
                       int E, void* stream) {
  if (N < 1 || T < 2 || E < 1) return AVD_ERR_SHAPE;
  if (!pe || !cls || !pos || !tok) return AVD_ERR_ARG;
  tokens_fwd_kernel<<<ew_grid((long long)N * T * E), 256, 0, avd_stream(stream)>>>(pe, cls, pos, tok, N,
                                                                                   T, E);
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

int avd_vit_tokens_bwd(const float* dtok, float* dpe, int N, int T, int E, void* stream) {
  if (N < 1 || T < 2 || E < 1) return AVD_ERR_SHAPE;
  if (!dtok || !dpe) return AVD_ERR_ARG;
  tokens_bwd_kernel<<<ew_grid((long long)N * (T - 1) * E), 256, 0, avd_stream(stream)>>>(dtok, dpe, N, T,
                                                                                         E);
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

}  // extern "C"
