// The recurrence of a one-layer bidirectional nn.LSTM followed by the mean over time
// (LSTMAudioEncoder.forward, models/dino.py:149-156: `x, _ = self.lstm(x); torch.mean(x, dim=1)`),
// forward and backward, for N sequences of T steps and hidden size H (16..128, multiple of 16).
//
// Everything that is a plain GEMM stays outside (avd_gemm / avd_linear_bwd): the input
// projections Gx = x W_ih^T + b_ih + b_hh come in, the pre-activation gate gradients dG go out.
// What is left is T dependent steps of  gates = Gx_t + h_{t-1} W_hh^T  and the pointwise cell.
//
// One persistent workgroup (4 waves) per (direction, block of 16 sequences) walks the T steps:
//   * the 16 sequences are the M rows of a 16x16 MFMA tile, 16 hidden units its columns; a wave
//     owns the unit tiles u = wave, wave + 4 and, per tile, the four gate accumulators
//     (i, f, g, o of the same (sequence, unit) land in the same lane and register), so the cell
//     state c, the pointwise math and the running sum of h never leave registers;
//   * the wave's slice of W_hh is loaded once, as MFMA B fragments held in registers for the
//     whole loop (bf16: 128 VGPRs per lane at H = 128; f32: 256);
//   * only h crosses waves: each step writes its 16 x H tile to the other half of a double
//     buffer in LDS (one barrier per step), where the next step reads it as the A operand;
//   * the next step's Gx tile is fetched into registers before the current step's MFMAs and is
//     the accumulators' initial value, so the gate sum costs no extra add.
// dt = 1 (bf16): v_mfma_f32_16x16x32_bf16, W_hh and the fed-back h rounded to bf16 (Gx, the cell
// state, the saved activations and the output mean stay f32; H = 16 / 48 pad K to 32 / 64 with
// zeros).  dt = 0 (f32 parity): v_mfma_f32_16x16x4_f32, an exact f32 fma chain.
//
// The backward walks the steps in the opposite order with the same ownership: dc and the mean's
// gradient stay in registers, dh_{t-1} = dG_t W_hh is the MFMA (K = 4H), and the 16 x 4H tile of
// dG crosses waves through LDS.
//
// Every wave executes every iteration of the time loop (the trip count is T for all, a ragged
// last block only masks its global loads and stores), so the barriers are uniform.  A block owns
// its outputs outright: no atomics, every sum in a fixed order, bitwise reproducible.
#include <math.h>

#include "common.h"

using namespace avd;

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f4;

constexpr int LB = 16;     // sequences per block (the MFMA tile's rows)
constexpr int LT = 256;    // threads per block: 4 waves

// MFMA traits per storage type of the operands.  B[k][col]: lane l holds col = l & 15 and
// k = KSTEP * s + (l >> 4) * PER + j (j < PER); A[row][k] the same with row = l & 15.
template <typename T> struct Mm;
template <> struct Mm<bf16> {
  static constexpr int KSTEP = 32, PAD = 8;
  typedef bf16x8 frag;
  template <typename F> static __device__ __forceinline__ frag load_b(F f, int s, int quad) {
    frag v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (__bf16)f(32 * s + 8 * quad + j);
    return v;
  }
  static __device__ __forceinline__ frag load_a(const bf16* row, int s, int quad) {
    return *reinterpret_cast<const frag*>(row + 32 * s + 8 * quad);
  }
  static __device__ __forceinline__ f4 mfma(frag a, frag b, f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ bf16 cvt(float v) { return f2bf(v); }
};
template <> struct Mm<float> {
  static constexpr int KSTEP = 4, PAD = 4;
  typedef float frag;
  template <typename F> static __device__ __forceinline__ frag load_b(F f, int s, int quad) {
    return f(4 * s + quad);
  }
  static __device__ __forceinline__ frag load_a(const float* row, int s, int quad) {
    return row[4 * s + quad];
  }
  static __device__ __forceinline__ f4 mfma(frag a, frag b, f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ float cvt(float v) { return v; }
};

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// saved state (save != 0): act [N][T][2][5][H] = sigmoid(i), sigmoid(f), tanh(g), sigmoid(o), c,
// then hprev [N][T][2][H] = the h the step at (n, t, dir) consumed (zeros at the direction's
// first step): dW_hh = dG^T hprev is then one strided GEMM over the N*T rows.
__host__ __device__ inline size_t act_elems(int N, int T, int H) { return (size_t)N * T * 2 * 5 * H; }

template <typename T, int H>
__global__ __launch_bounds__(LT) void lstm_fwd_kernel(const float* __restrict__ gx,
                                                      const float* __restrict__ whh0,
                                                      const float* __restrict__ whh1,
                                                      float* __restrict__ out, float* __restrict__ save,
                                                      int N, int Tn) {
  typedef Mm<T> M;
  constexpr int KP = (H + M::KSTEP - 1) / M::KSTEP * M::KSTEP;
  constexpr int KS = KP / M::KSTEP;
  constexpr int NU = H / 16;
  constexpr int TPW = (NU + 3) / 4;
  constexpr int LD = KP + M::PAD;
  __shared__ __attribute__((aligned(16))) T hbuf[2][LB][LD];

  const int dir = blockIdx.y, n0 = blockIdx.x * LB;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int col = lane & 15, quad = lane >> 4;
  const float* whh = dir ? whh1 : whh0;

  for (int i = threadIdx.x; i < 2 * LB * LD; i += LT) (&hbuf[0][0][0])[i] = M::cvt(0.f);

  typename M::frag wf[TPW][4][KS];
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int u = wave + 4 * i;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int s = 0; s < KS; ++s)
        wf[i][g][s] = M::load_b(
            [&](int k) {
              return (u < NU && k < H) ? whh[(size_t)(g * H + u * 16 + col) * H + k] : 0.f;
            },
            s, quad);
  }

  float c[TPW][4], hsum[TPW][4];
#pragma unroll
  for (int i = 0; i < TPW; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) c[i][r] = hsum[i][r] = 0.f;

  float* hprev = save ? save + act_elems(N, Tn, H) : nullptr;
  // (n, t) -> row of the [N][T][2] grids
  auto row_of = [&](int n, int t) { return ((size_t)n * Tn + t) * 2 + dir; };
  auto load_gx = [&](int t, f4 (&dst)[TPW][4]) {
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      const int u = wave + 4 * i;
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = n0 + quad * 4 + r;
          dst[i][g][r] = (u < NU && n < N) ? gx[row_of(n, t) * (4 * H) + g * H + u * 16 + col] : 0.f;
        }
    }
  };

  const int t0 = dir ? Tn - 1 : 0;
  if (save) {
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      const int u = wave + 4 * i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + quad * 4 + r;
        if (u < NU && n < N) hprev[row_of(n, t0) * H + u * 16 + col] = 0.f;
      }
    }
  }
  f4 gnext[TPW][4];
  load_gx(t0, gnext);
  __syncthreads();

  for (int s = 0; s < Tn; ++s) {
    const int t = dir ? Tn - 1 - s : s;
    const int tn = dir ? t - 1 : t + 1;          // the direction's next step (valid if s + 1 < Tn)
    const bool more = s + 1 < Tn;                // block-uniform
    f4 acc[TPW][4];
#pragma unroll
    for (int i = 0; i < TPW; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[i][g] = gnext[i][g];
    if (more) load_gx(tn, gnext);

    const T* hrow = &hbuf[s & 1][col][0];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const typename M::frag a = M::load_a(hrow, ks, quad);
#pragma unroll
      for (int i = 0; i < TPW; ++i)
        if (wave + 4 * i < NU) {
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[i][g] = M::mfma(a, wf[i][g][ks], acc[i][g]);
        }
    }

#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      const int u = wave + 4 * i;
      if (u < NU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float ig = sigm(acc[i][0][r]), fg = sigm(acc[i][1][r]);
          const float gg = tanhf(acc[i][2][r]), og = sigm(acc[i][3][r]);
          const float cn = fg * c[i][r] + ig * gg;
          const float h = og * tanhf(cn);
          c[i][r] = cn;
          hsum[i][r] += h;
          const int sq = quad * 4 + r, n = n0 + sq, unit = u * 16 + col;
          hbuf[(s + 1) & 1][sq][unit] = M::cvt(h);
          if (save && n < N) {
            float* a = save + row_of(n, t) * (5 * H) + unit;
            a[0] = ig; a[H] = fg; a[2 * H] = gg; a[3 * H] = og; a[4 * H] = cn;
            if (more) hprev[row_of(n, tn) * H + unit] = h;
          }
        }
      }
    }
    __syncthreads();
  }

  const float inv = 1.0f / (float)Tn;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int u = wave + 4 * i;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + quad * 4 + r;
      if (u < NU && n < N) out[(size_t)n * (2 * H) + dir * H + u * 16 + col] = hsum[i][r] * inv;
    }
  }
}

template <typename T, int H>
__global__ __launch_bounds__(LT) void lstm_bwd_kernel(const float* __restrict__ dout,
                                                      const float* __restrict__ whh0,
                                                      const float* __restrict__ whh1,
                                                      const float* __restrict__ save,
                                                      float* __restrict__ dg, int N, int Tn) {
  typedef Mm<T> M;
  constexpr int K4 = 4 * H;                      // a multiple of 64: no K padding
  constexpr int KS = K4 / M::KSTEP;
  constexpr int NU = H / 16;
  constexpr int TPW = (NU + 3) / 4;
  constexpr int LD = K4 + M::PAD;
  __shared__ __attribute__((aligned(16))) T dgb[2][LB][LD];

  const int dir = blockIdx.y, n0 = blockIdx.x * LB;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int col = lane & 15, quad = lane >> 4;
  const float* whh = dir ? whh1 : whh0;

  for (int i = threadIdx.x; i < 2 * LB * LD; i += LT) (&dgb[0][0][0])[i] = M::cvt(0.f);

  // dh_prev[seq][unit] = sum_j dG[seq][j] W_hh[j][unit]: B[k = j][col = unit]
  typename M::frag wf[TPW][KS];
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int u = wave + 4 * i;
#pragma unroll
    for (int s = 0; s < KS; ++s)
      wf[i][s] = M::load_b([&](int j) { return u < NU ? whh[(size_t)j * H + u * 16 + col] : 0.f; },
                           s, quad);
  }

  auto row_of = [&](int n, int t) { return ((size_t)n * Tn + t) * 2 + dir; };
  const float inv = 1.0f / (float)Tn;
  float dc[TPW][4], dhm[TPW][4];
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int u = wave + 4 * i;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + quad * 4 + r;
      dc[i][r] = 0.f;
      dhm[i][r] = (u < NU && n < N) ? dout[(size_t)n * (2 * H) + dir * H + u * 16 + col] * inv : 0.f;
    }
  }
  __syncthreads();

  for (int s = 0; s < Tn; ++s) {
    const int t = dir ? s : Tn - 1 - s;          // the direction's steps, last to first
    const int tp = dir ? t + 1 : t - 1;          // the step before t in the direction's order
    const bool has_prev = s + 1 < Tn;            // block-uniform
    float sv[TPW][4][6];                         // i, f, g, o, c_t, c_{t-1}
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      const int u = wave + 4 * i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + quad * 4 + r, unit = u * 16 + col;
        const bool ok = u < NU && n < N;
        const float* a = save + row_of(ok ? n : 0, t) * (5 * H) + (ok ? unit : 0);
#pragma unroll
        for (int q = 0; q < 5; ++q) sv[i][r][q] = ok ? a[q * H] : 0.f;
        sv[i][r][5] = (ok && has_prev) ? save[row_of(n, tp) * (5 * H) + 4 * H + unit] : 0.f;
      }
    }

    f4 acc[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) acc[i] = f4{0.f, 0.f, 0.f, 0.f};
    const T* drow = &dgb[s & 1][col][0];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const typename M::frag a = M::load_a(drow, ks, quad);
#pragma unroll
      for (int i = 0; i < TPW; ++i)
        if (wave + 4 * i < NU) acc[i] = M::mfma(a, wf[i][ks], acc[i]);
    }

#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      const int u = wave + 4 * i;
      if (u < NU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float ig = sv[i][r][0], fg = sv[i][r][1], gg = sv[i][r][2], og = sv[i][r][3];
          const float tc = tanhf(sv[i][r][4]), cp = sv[i][r][5];
          const float dh = dhm[i][r] + acc[i][r];
          const float dcl = dc[i][r] + dh * og * (1.f - tc * tc);
          dc[i][r] = dcl * fg;
          float da[4];
          da[0] = dcl * gg * ig * (1.f - ig);
          da[1] = dcl * cp * fg * (1.f - fg);
          da[2] = dcl * ig * (1.f - gg * gg);
          da[3] = dh * tc * og * (1.f - og);
          const int sq = quad * 4 + r, n = n0 + sq, unit = u * 16 + col;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            dgb[(s + 1) & 1][sq][q * H + unit] = M::cvt(da[q]);
            if (n < N) dg[row_of(n, t) * (4 * H) + q * H + unit] = da[q];
          }
        }
      }
    }
    __syncthreads();
  }
}

template <typename S, typename D>
__global__ void cast_kernel(const S* __restrict__ src, D* __restrict__ dst, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) io<D>::st(dst, (size_t)i, io<S>::ld(src, (size_t)i));
}

bool dims_ok(int N, int T, int H) { return N >= 1 && T >= 1 && H >= 16 && H <= 128 && H % 16 == 0; }

}  // namespace

int avd_lstm_ws(int N, int T, int H, long long* save_elems, long long* dg_elems) {
  if (!save_elems || !dg_elems) return AVD_ERR_ARG;
  if (!dims_ok(N, T, H)) return AVD_ERR_SHAPE;
  *save_elems = (long long)N * T * 2 * 6 * H;
  *dg_elems = (long long)N * T * 2 * 4 * H;
  return AVD_OK;
}

#define LSTM_DISPATCH(KERNEL, TY, ...)                                              \
  switch (H) {                                                                      \
    case 16: KERNEL<TY, 16><<<grid, LT, 0, st>>>(__VA_ARGS__); break;               \
    case 32: KERNEL<TY, 32><<<grid, LT, 0, st>>>(__VA_ARGS__); break;               \
    case 48: KERNEL<TY, 48><<<grid, LT, 0, st>>>(__VA_ARGS__); break;               \
    case 64: KERNEL<TY, 64><<<grid, LT, 0, st>>>(__VA_ARGS__); break;               \
    case 80: KERNEL<TY, 80><<<grid, LT, 0, st>>>(__VA_ARGS__); break;               \
    case 96: KERNEL<TY, 96><<<grid, LT, 0, st>>>(__VA_ARGS__); break;               \
    case 112: KERNEL<TY, 112><<<grid, LT, 0, st>>>(__VA_ARGS__); break;             \
    default: KERNEL<TY, 128><<<grid, LT, 0, st>>>(__VA_ARGS__); break;              \
  }

int avd_lstm_fwd(const float* gx, const float* whh_f, const float* whh_r, float* out, float* save,
                 int save_state, int dt, int N, int T, int H, void* stream) {
  if (!gx || !whh_f || !whh_r || !out || (save_state && !save)) return AVD_ERR_ARG;
  if (dt != AVD_F32 && dt != AVD_BF16) return AVD_ERR_DTYPE;
  if (!dims_ok(N, T, H)) return AVD_ERR_SHAPE;
  hipStream_t st = avd_stream(stream);
  const dim3 grid((N + LB - 1) / LB, 2);
  float* sv = save_state ? save : nullptr;
  if (dt == AVD_BF16) {
    LSTM_DISPATCH(lstm_fwd_kernel, bf16, gx, whh_f, whh_r, out, sv, N, T)
  } else {
    LSTM_DISPATCH(lstm_fwd_kernel, float, gx, whh_f, whh_r, out, sv, N, T)
  }
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

int avd_lstm_bwd(const float* dout, const float* whh_f, const float* whh_r, const float* save,
                 float* dg, int dt, int N, int T, int H, void* stream) {
  if (!dout || !whh_f || !whh_r || !save || !dg) return AVD_ERR_ARG;
  if (dt != AVD_F32 && dt != AVD_BF16) return AVD_ERR_DTYPE;
  if (!dims_ok(N, T, H)) return AVD_ERR_SHAPE;
  hipStream_t st = avd_stream(stream);
  const dim3 grid((N + LB - 1) / LB, 2);
  if (dt == AVD_BF16) {
    LSTM_DISPATCH(lstm_bwd_kernel, bf16, dout, whh_f, whh_r, save, dg, N, T)
  } else {
    LSTM_DISPATCH(lstm_bwd_kernel, float, dout, whh_f, whh_r, save, dg, N, T)
  }
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

int avd_cast(const void* src, int src_dt, void* dst, int dst_dt, long long n, void* stream) {
  if (!src || !dst) return AVD_ERR_ARG;
  if (n < 1) return AVD_ERR_SHAPE;
  hipStream_t st = avd_stream(stream);
  const unsigned grid = (unsigned)((n + 255) / 256);
  if (src_dt == AVD_BF16 && dst_dt == AVD_F32)
    cast_kernel<bf16, float><<<grid, 256, 0, st>>>((const bf16*)src, (float*)dst, n);
  else if (src_dt == AVD_F32 && dst_dt == AVD_BF16)
    cast_kernel<float, bf16><<<grid, 256, 0, st>>>((const float*)src, (bf16*)dst, n);
  else
    return AVD_ERR_DTYPE;
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}
