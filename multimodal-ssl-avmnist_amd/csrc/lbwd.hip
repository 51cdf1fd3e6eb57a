// One fused launch for the whole backward of the audio conv2 layer (56x56, 8 -> 16, 5x5 pad 2;
// CentralUnimodalAudio, unimodal.py:185-221 -> nn.Conv2d -> BatchNorm2d -> ReLU -> MaxPool2d):
//
//   dY = BN-backward apply (bnapply.h) of y and the pooled gradient    [N, 56, 56, 16]
//   dX = conv_transpose(dY, W)            (the input gradient)         [N, 56, 56, 8]
//   dW = sum_{n, p} dY[n, p] (x) X[n, p + tap - 2]   (weight gradient) [16][8][25]
//
// from ONE staged tile of dY.  Before, the step ran the apply (y + pooled gradient -> dY in HBM,
// bn_cl.hip), then the input gradient (conv_ws.hip) and the weight gradient (wgrad_ws.hip) side
// by side on two streams, each streaming the 719 MB dY at config-2 size: 3.8 GB of HBM traffic
// for the layer and two latency-bound kernels inflating each other.  Here a
// persistent block walks TH-row tiles of its samples; per tile it
//   * stages the dY tile with its 2-row / 2-column halo, formed in registers from y and the
//     pooled gradient (AP = 1; one 2x2 window x 8 channels per task, bit-identical to
//     bwd_apply_cl_kernel; AP = 2: the same dY with the gradient routed by the forward pool's
//     code words, bn_cl.hip, instead of a recomputed relu(bn(y)) argmax -- half the apply's
//     VALU work) or loaded from a dY tensor (AP = 0), and the X tile with its halo;
//   * runs the input gradient on it exactly as conv_ws_kernel's DgrA2 does (weights resident in
//     VGPRs, B fragments = one ds_read_b128 of the (tap, channel) k-group per pixel, same k
//     order: bit-identical dX);
//   * accumulates dW exactly as wgrad_ws_kernel's WgA2 does (M = dY channels, N = 13 column tiles
//     of (tap pair, 8 X channels), K = the tile's pixels, both operands by ds_read_b64_tr_b16),
//     in registers across all of the block's tiles; the four waves split the pixels and are
//     summed through LDS at the end; one deterministic f32 slab per block (avd_sum_rows).
// HBM per launch: y + pooled gradient + X read once, dX written once (1.6 GB at N = 7168), no dY.
//
// Second instantiation: the audio conv3 layer (28x28, 16 -> 32, 5x5 pad 2), LbA3 (0.86 GB per
// launch at N = 7168 for what were 2.0 GB in three launches).  What differs:
//   * rows are 28 pixels, so the weight gradient's 32-pixel k-steps are one row padded to W8 = 32
//     (WgA3's map, wgrad_ws.hip): the dY image keeps its pad columns zero for the whole launch and
//     the X image is W8 + 4 columns wide, zero past the map;
//   * the dY pixel stride is 48 elements (DgrA3's / WgA3's conflict-free image), the input
//     gradient's k-step is one tap x 32 dY channels in DgrA3's order (bit-identical dX), its D
//     tile is full (16 dX channels, no row pairs), and its 16-pixel groups cross row ends;
//   * 25 resident weight fragments (100 VGPRs) beside 2 x 25 dW accumulator tiles do not fit one
//     wave at two blocks per CU, so the waves specialise (SP): waves 0-1 run the input gradient,
//     waves 2-3 the weight gradient (13 column tiles x 2 row tiles each), and the resident
//     weights / the accumulators share one register array; all four waves stage.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "bnapply.h"

using namespace avd;

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f4;
typedef __attribute__((ext_vector_type(4))) unsigned u4;
typedef __attribute__((ext_vector_type(4))) short s4;
typedef __attribute__((ext_vector_type(2))) unsigned u2;

__device__ const u4 kZeroL = {0u, 0u, 0u, 0u};

constexpr int cdv(int a, int b) { return (a + b - 1) / b; }

// LBWD28_PFD, LBWD28_GB, LBWD28_WFD (build-time, for A/B builds of the 28^2 instantiation): the
// input gradient's read-ahead depth and groups per pass, the weight gradient's ring depth
#ifndef LBWD28_WFD
#define LBWD28_WFD 3
#endif

template <int V> using IC = std::integral_constant<int, V>;
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(IC<I>{});
    static_for<I + 1, N>(f);
  }
}

template <int CIN_, int COUT_, int H_, int W_, int TH_, int OCC_, int PFD_ = 6, int GB_ = 1, int NCW_ = 1,
          int RP_ = 0, int BAL_ = 0, int WGU_ = 0, int SP_ = 0>
struct Lb {
  static constexpr int CIN = CIN_, COUT = COUT_, K = 5, PAD = 2, H = H_, W = W_;   // the forward conv
  static constexpr int OCT = COUT / 8, XOCT = CIN / 8;          // 16-byte vectors per pixel
  static constexpr int W8 = (W + 7) & ~7;                       // weight-gradient row (8-pixel runs)
  static constexpr int TH = TH_, TPS = H / TH, OCC = OCC_, PFD = PFD_, GB = GB_;
  static constexpr int ITH = TH + K - 1, ITW = W + K - 1;        // staged rows / columns (halo)
  // dY tile [ITH][RS][PS]: DgrA2's conflict-free image (pixel stride 16 channels, rows padded
  // by 4 pixels); X tile [ITH][XW][XS]: WgA2's
  // (32 channels: DgrA3's / WgA3's 48-element pixel stride; X rows reach W8 + K - 1 columns so
  // the padded pixels of a weight-gradient row read zeros, not stale LDS)
  static constexpr int PS = COUT <= 16 ? COUT : COUT + 16, RS = ITW + 4, XW = W8 + K - 1, XS = CIN;
  static constexpr int DY_ELEMS = ITH * RS * PS, X_ELEMS = ITH * XW * XS;
  // input gradient: M = dX channels (8 rows of a 16-row tile, or all 16), N = 16-pixel groups,
  // K = (tap, dY channel) in conv_ws's order, 13 k-steps of 32 (32 dY channels: 25, one per tap)
  static constexpr int KK = K * K, KPAD = cdv(KK * COUT, 32) * 32;
  // RP (row pairs): one MFMA row tile = dX channels of TWO output rows (m < 8: row y, m >= 8: row
  // y + 1) over the 6 x 5 dY taps both rows need -- 15 k-steps per 16 pixels of a row pair
  // instead of 2 x 13, and no padding rows in the D tile (the layer is LDS-read bound: every
  // k-step reads a 16-byte im2col fragment per lane)
  static constexpr int RP = RP_, KTAPS = RP ? (K + 1) * K : KK;
  static constexpr int KS = cdv(KTAPS * COUT, 32);
  // SP (specialised waves): waves [0, 2) run the input gradient, waves [2, 4) the weight
  // gradient; otherwise all four run both
  static constexpr int SP = SP_, NDW = SP ? 2 : 4, NWW = SP ? 2 : 4;
  static constexpr int PIX = TH * W, NG = (RP ? PIX / 2 : PIX) / 16, GW = cdv(NG, NDW);
  // weight gradient: 13 column tiles (tap pair x 8 channels), K = PIX pixels in 32-pixel steps;
  // the 4 waves split NCW ways over column tiles (NW per wave) and NPW = 4 / NCW over k-steps
  // (16 X channels: 25 column tiles, one tap x 16 channels each; MT row tiles of 16 dY channels)
  static constexpr int MT = COUT / 16, NCT = CIN == 8 ? cdv(KK, 2) : KK, WKS = TH * W8 / 32;
  static constexpr int NCW = NCW_, NW = cdv(NCT, NCW), NPW = NWW / NCW;
  static constexpr int WT = (ITH / 2) * (ITW / 2) * OCT;          // AP: window x channel-octet tasks
  // BAL (balanced apply staging): slot 0 = the tasks of the TH / 2 window rows a continuation
  // tile forms anew (NEWT, spread over all four waves), slot 1 = the PAD window rows it copies
  // from the previous tile (OLDT) -- a continuation tile runs slot 0 only.  Without BAL the
  // tasks sit in linear order on the two slots, and in a continuation tile one wave has live
  // lanes in both and runs the apply twice while the other three wait at the barrier.
  static constexpr int BAL = BAL_;
  static constexpr int NEWT = (TH / 2) * (ITW / 2) * OCT, OLDT = WT - NEWT;
  static_assert(!BAL || (NEWT <= 256 && OLDT <= 256), "balanced staging: one slot each");
  // WGU: the weight gradient's k-step loop unrolled, each k-step's pixel origin a constant;
  // 2: also one fragment ring over all (k-step, column tile) pairs of the tile, WFD reads ahead
  // (13 column tiles per wave: two whole k-steps of fragments would not fit the registers)
  static constexpr int WGU = WGU_, WFD = LBWD28_WFD;
  static_assert(!WGU || NPW == 1, "unrolled weight gradient: every wave walks all k-steps");
  static_assert(WGU != 2 || W8 == 32, "fragment ring: one k-step = one padded row");
  static constexpr int DT = ITH * ITW * OCT;                      // AP = 0: 16-byte dY tasks
  static constexpr int XT = ITH * XW * XOCT;                      // 16-byte X tasks
  static constexpr int RED = (NPW - 1) * NCW * NW * MT * 64;      // f4 slots: pixel partials
  // two tile images (double buffer): tile i + 1 is staged while tile i's MFMAs run, one barrier
  // per tile (the apply's VALU work beside the MFMAs instead of between two barriers)
  static constexpr int BUF = DY_ELEMS + X_ELEMS;
  static constexpr int SMEM = 2 * BUF > RED * 8 ? 2 * BUF : RED * 8;
  static_assert((CIN == 8 && COUT == 16) || (CIN == 16 && COUT == 32), "k-group and column maps");
  static_assert(H % TH == 0 && TH % 2 == 0 && (TH * W8) % 32 == 0 && PIX % 16 == 0, "tiles");
  static_assert(TH >= 2 * PAD && W8 + PAD <= RS, "continuation rows, padded weight-gradient row");
  static_assert(SMEM * 2 <= 76 * 1024, "LDS (two blocks per CU: 160 KB)");
  static_assert(NWW % NCW == 0, "wave split");
  static_assert(!RP || (CIN == 8 && (KTAPS * COUT) % 32 == 0), "row-pair k-steps");
  // SP: the resident weights (input-gradient waves) and the accumulators (weight-gradient waves)
  // are one register array
  static_assert(!SP || (KS <= MT * NW && NPW == 1), "specialised waves: shared registers");
};

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
// bnapply.h's apply_window (gout layout 0), one channel pair at a time: the same IEEE operations
// in the same order (bit-identical dY), but only one pair's coefficients and values live at
// once -- the full-width version keeps ~80 temporaries across the window and spills here
__device__ __forceinline__ void apply_window_lean(const WinIn& in, const float* ct, int C, u4 (&out)[4]) {
  const unsigned yw[4][4] = {{in.y[0].x, in.y[0].y, in.y[0].z, in.y[0].w},
                             {in.y[1].x, in.y[1].y, in.y[1].z, in.y[1].w},
                             {in.y[2].x, in.y[2].y, in.y[2].z, in.y[2].w},
                             {in.y[3].x, in.y[3].y, in.y[3].z, in.y[3].w}};
  const unsigned gw[4] = {in.g0.x, in.g0.y, in.g0.z, in.g0.w};
  unsigned ow[4][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float2 sc = *reinterpret_cast<const float2*>(ct + 2 * e);
    const float2 sf = *reinterpret_cast<const float2*>(ct + C + 2 * e);
    const float2 k1 = *reinterpret_cast<const float2*>(ct + 2 * C + 2 * e);
    const float2 kx = *reinterpret_cast<const float2*>(ct + 3 * C + 2 * e);
    const float2 k0 = *reinterpret_cast<const float2*>(ct + 4 * C + 2 * e);
    float d[4][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float s_ = h ? sc.y : sc.x, f_ = h ? sf.y : sf.x;
      float yv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) yv[k] = h ? __uint_as_float(yw[k][e] & 0xffff0000u) : __uint_as_float(yw[k][e] << 16);
      float best = fmaxf(fmaf(yv[0], s_, f_), 0.f);
      int am = 0;
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        const float r = fmaxf(fmaf(yv[k], s_, f_), 0.f);
        if (r > best) { best = r; am = k; }
      }
      const float gg = h ? __uint_as_float(gw[e] & 0xffff0000u) : __uint_as_float(gw[e] << 16);
      const float dz = best > 0.f ? gg : 0.f;
      const float a1 = h ? k1.y : k1.x, ax = h ? kx.y : kx.x, a0 = h ? k0.y : k0.x;
#pragma unroll
      for (int k = 0; k < 4; ++k) d[k][h] = fmaf(a1, am == k ? dz : 0.f, fmaf(ax, yv[k], a0));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) ow[k][e] = pack_bf16x2(d[k][0], d[k][1]);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = u4{ow[k][0], ow[k][1], ow[k][2], ow[k][3]};
}

// pixel (within a 32-pixel k-step) of k = 8 g + 4 h + q (wgrad_ws.hip's kpix)
__device__ __forceinline__ int kpix(int g, int h, int q) { return 16 * (g >> 1) + 8 * h + 4 * (g & 1) + q; }

// dgrad k-groups (conv_ws.hip koff with CIN = 16): k-group 4 ks + g is tap (4 ks + g) / 2,
// channel chunk 8 (g & 1); padded k-groups (tap >= 25) read tap 0 against zero weights
template <class L>
constexpr int tapoff(int tap) { return ((tap / L::K) * L::RS + tap % L::K) * L::PS; }

template <class L, int AP>
__global__ __launch_bounds__(256, L::OCC) void lbwd_kernel(const bf16* __restrict__ ysrc,
                                                          const bf16* __restrict__ x,
                                                          const bf16* __restrict__ wk,
                                                          bf16* __restrict__ dx,
                                                          float* __restrict__ parts, int ntiles,
                                                          ApplyArgs aa) {
  __shared__ __attribute__((aligned(16))) bf16 smem[L::SMEM];
  // AP = 1: (scale, shift, k1, kx, k0) per group; AP = 2 (code-routed): (k1, kx, k0) only
  constexpr int CTR = AP == 1 ? 5 : 3;
  __shared__ __attribute__((aligned(16))) float ctab[AP ? APPLY_GMAX * CTR * L::COUT : 4];
  // dY tile (row ty0 - PAD + r, column c - PAD) then the X tile (same origin), per buffer
  bf16* dys = smem;
  bf16* xs = smem + L::DY_ELEMS;
  auto set_buf = [&](int b) {
    dys = smem + b * L::BUF;
    xs = dys + L::DY_ELEMS;
  };
  const int tid = threadIdx.x, wp = tid >> 6, lane = tid & 63;
  const int g = lane >> 4, r16 = lane & 15, q4 = r16 >> 2, p4 = r16 & 3;
  // SP: the wave's role (wave-uniform, so the role branches are scalar) and its index in the role
  const bool dgw = !L::SP || __builtin_amdgcn_readfirstlane(wp) < L::NDW;
  const bool wgw = !L::SP || !dgw;
  const int dwp = L::SP ? (wp & (L::NDW - 1)) : wp, wwp = L::SP ? (wp & (L::NWW - 1)) : wp;
  const int wc = wwp / L::NPW, wq = wwp % L::NPW;   // weight gradient: column group, pixel part

  // dY pad columns (a padded weight-gradient row reads PAD pixels past the halo): zero in both
  // buffers for the whole launch -- nothing stages them, and a continuation copy moves zeros
  if constexpr (L::W8 != L::W) {
    constexpr int PC = L::RS - L::ITW, CH = L::PS / 8;
    for (int i = tid; i < 2 * L::ITH * PC * CH; i += 256) {
      const int q = i % CH, t = i / CH, c = L::ITW + t % PC, rb = t / PC;
      const int b = rb / L::ITH, r = rb - b * L::ITH;
      *reinterpret_cast<u4*>(smem + b * L::BUF + (r * L::RS + c) * L::PS + 8 * q) = u4{0u, 0u, 0u, 0u};
    }
  }

  // ---- weight-gradient accumulators; SP: in the input-gradient waves the same registers hold
  // the resident weights (wa)
  f4 wacc[L::MT * L::NW];
  // ---- input-gradient weights (flipped, [16 rows][KPAD]; 8 dX channels: rows 8-15 zero), resident
  bf16x8 a[L::SP ? 1 : L::KS];
  auto wa = [&](auto jc) -> bf16x8 {
    constexpr int j = decltype(jc)::value;
    if constexpr (L::SP) return __builtin_bit_cast(bf16x8, wacc[j]);
    else return a[j];
  };
  if constexpr (L::SP) {
    if (dgw) {
#pragma unroll
      for (int j = 0; j < L::KS; ++j)
        wacc[j] = __builtin_bit_cast(f4, *reinterpret_cast<const bf16x8*>(wk + (size_t)r16 * L::KPAD + 32 * j + 8 * g));
    } else {
#pragma unroll
      for (int j = 0; j < L::MT * L::NW; ++j) wacc[j] = f4{0.f, 0.f, 0.f, 0.f};
    }
  } else if constexpr (L::RP) {
    // row m = (output row m >> 3, dX channel m & 7); k-group 4 j + g = staged-row offset /
    // filter column t = 2 j + (g >> 1) of the 6 x 5 window, dY channel half 8 (g & 1): the
    // filter row is t / 5 - (m >> 3) -- outside [0, 5) the weight is 0
#pragma unroll
    for (int j = 0; j < L::KS; ++j) {
      const int t = 2 * j + (g >> 1), kh = t / L::K - (r16 >> 3), kw = t % L::K;
      constexpr bf16x8 z = {};
      a[j] = (kh >= 0 && kh < L::K)
                 ? *reinterpret_cast<const bf16x8*>(wk + (size_t)(r16 & 7) * L::KPAD + (kh * L::K + kw) * L::COUT + 8 * (g & 1))
                 : z;
    }
  } else {
#pragma unroll
    for (int j = 0; j < L::KS; ++j) a[j] = *reinterpret_cast<const bf16x8*>(wk + (size_t)r16 * L::KPAD + 32 * j + 8 * g);
  }
  // k-group (ks, g) = taps 2 ks (g < 2) / 2 ks + 1 (g >= 2), channel half g & 1: the k-step part
  // of its offset is a compile-time immediate (tapoff), the lane part one of three registers
  // (32 dY channels, DgrA3's order: k-step j = tap j, the lane's k-group its channel octet g)
  const int ln_a = L::COUT == 32 ? 8 * g : (g >> 1) * L::PS + 8 * (g & 1);   // tap + 1 on the same row
  const int ln_b = (g >> 1) * (L::RS - (L::K - 1)) * L::PS + 8 * (g & 1);   // next filter row
  const int ln_c = (g >> 1) ? -tapoff<L>(L::KK - 1) : 8 * (g & 1);  // past the last tap: tap 0

  // ---- weight-gradient column offsets in the X tile (PAIR layout of wgrad_ws.hip)
  int xo[L::NW];
#pragma unroll
  for (int j = 0; j < L::NW; ++j) {
    int tap = L::CIN == 8 ? 2 * (wc * L::NW + j) + (p4 >> 1) : wc * L::NW + j;
    const int ch = L::CIN == 8 ? 4 * (p4 & 1) : 4 * p4;
    if (tap >= L::KK) tap = 0;
    xo[j] = ((tap / L::K) * L::XW + tap % L::K) * L::XS + ch;
  }
  if constexpr (!L::SP) {
#pragma unroll
    for (int j = 0; j < L::MT * L::NW; ++j) wacc[j] = f4{0.f, 0.f, 0.f, 0.f};
  }

  // ---- contiguous tile range of this block (tile = TH rows of one sample)
  const int per = ntiles / (int)gridDim.x, extra = ntiles % (int)gridDim.x;
  const int t0 = (int)blockIdx.x * per + min((int)blockIdx.x, extra);
  const int t1 = t0 + per + ((int)blockIdx.x < extra ? 1 : 0);

  // ---- staging slots: dY (AP: 2x2 windows of y + pooled gradient; else 16-byte dY tasks), X
  constexpr int HP = L::H / 2, WP = L::W / 2;
  constexpr int YT = AP ? L::WT : L::DT;
  constexpr int YSL = cdv(YT, 256), XSL = cdv(L::XT, 256);
  constexpr bool BAL = AP && L::BAL;
  static_assert(!BAL || YSL == 2, "balanced staging: two slots");
  // slot i's task of this thread, whether it exists, and whether a continuation tile skips it
  auto ytask = [&](int i) { return BAL ? (i == 0 ? tid + L::OLDT : tid) : tid + 256 * i; };
  auto yhas = [&](int i) { return BAL ? (i == 0 ? tid < L::NEWT : tid < L::OLDT) : tid + 256 * i < YT; };
  int ygo[YSL], ylo[YSL], yrow[YSL], ygg[YSL];
  int xgo[XSL], xlo[XSL], xrow[XSL];
#pragma unroll
  for (int i = 0; i < YSL; ++i) {
    const int task = ytask(i);
    const int q = task & (L::OCT - 1), w = task / L::OCT;   // COUT / 8 = 2 or 4 channel octets
    if constexpr (AP) {
      const int wc2 = w % (L::ITW / 2), wr = w / (L::ITW / 2);
      const int r = 2 * wr, c = 2 * wc2, ix = c - L::PAD;
      yrow[i] = r;
      ylo[i] = (r * L::RS + c) * L::PS + 8 * q;
      ygo[i] = (yhas(i) && ix >= 0 && ix < L::W) ? (r * L::W + ix) * L::COUT + 8 * q : -1;
      ygg[i] = (wr * WP + ix / 2) * L::COUT + 8 * q;
    } else {
      const int c = w % L::ITW, r = w / L::ITW, ix = c - L::PAD;
      yrow[i] = r;
      ylo[i] = (r * L::RS + c) * L::PS + 8 * q;
      ygo[i] = (task < YT && ix >= 0 && ix < L::W) ? (r * L::W + ix) * L::COUT + 8 * q : -1;
      ygg[i] = 0;
    }
  }
#pragma unroll
  for (int i = 0; i < XSL; ++i) {
    const int task = tid + 256 * i;
    const int q = task & (L::XOCT - 1), px = task / L::XOCT;
    const int c = px % L::XW, r = px / L::XW, ix = c - L::PAD;
    xrow[i] = r;
    xlo[i] = (r * L::XW + c) * L::XS + 8 * q;
    xgo[i] = (task < L::XT && ix >= 0 && ix < L::W) ? (r * L::W + ix) * L::CIN + 8 * q : -1;
  }
  if constexpr (AP == 1) apply_load_ctab<L::COUT>(ctab, aa, tid, 256);
  if constexpr (AP == 2) apply_load_ktab<L::COUT>(ctab, aa, tid, 256);

  WinIn wpre[AP ? YSL : 1];
  u4 ypre[AP ? 1 : YSL];
  u4 xpre[XSL];
  // cont: the block's previous tile is the rows just above this one in the same sample, so the
  // first 2 * PAD staged rows (dY and X) are copied from that tile's last rows instead of loaded
  // and recomputed (a third of the BN-backward apply and of the y / x loads)
  constexpr int RR = 2 * L::PAD;
  auto load_tile = [&](int ti, bool cont) {
    const int n = ti / L::TPS, ty0 = (ti - n * L::TPS) * L::TH;
    const long long row0 = (long long)n * L::H + ty0 - L::PAD;     // first staged row
    const bf16* by = ysrc + row0 * L::W * L::COUT;
    const bf16* bx = x + row0 * L::W * L::CIN;
#pragma unroll
    for (int i = 0; i < YSL; ++i) {
      if (BAL && i == 1 && cont) continue;     // (block-uniform) the copied rows' slot
      const bool ok = ygo[i] >= 0 && (unsigned)(ty0 - L::PAD + yrow[i]) < (unsigned)L::H &&
                      !(cont && yrow[i] < RR);
      const bf16* p = by + (ok ? ygo[i] : 0);
      if constexpr (AP) {
        wpre[i].y[0] = ldg16(ok ? (const void*)(p) : &kZeroL);
        wpre[i].y[1] = ldg16(ok ? (const void*)(p + L::COUT) : &kZeroL);
        wpre[i].y[2] = ldg16(ok ? (const void*)(p + L::W * L::COUT) : &kZeroL);
        wpre[i].y[3] = ldg16(ok ? (const void*)(p + (L::W + 1) * L::COUT) : &kZeroL);
        const bf16* gb = reinterpret_cast<const bf16*>(aa.gout) + ((long long)n * HP + (ty0 - L::PAD) / 2) * WP * L::COUT;
        wpre[i].g0 = ldg16(ok ? (const void*)(gb + ygg[i]) : &kZeroL);
        if constexpr (AP == 2) {
          // the forward's routing word of this (pooled pixel, channel octet): gout's index / 8
          const unsigned* cb = aa.codes + ((long long)n * HP + (ty0 - L::PAD) / 2) * WP * (L::COUT / 8);
          wpre[i].g1.x = ok ? __builtin_nontemporal_load(cb + (ygg[i] >> 3)) : 0u;
        }
      } else {
        ypre[i] = ldg16(ok ? (const void*)p : &kZeroL);
      }
    }
#pragma unroll
    for (int i = 0; i < XSL; ++i) {
      const bool ok = xgo[i] >= 0 && (unsigned)(ty0 - L::PAD + xrow[i]) < (unsigned)L::H &&
                      !(cont && xrow[i] < RR);
      xpre[i] = ldg16(ok ? (const void*)(bx + xgo[i]) : &kZeroL);
    }
  };
  auto store_tile = [&](int ti, bool cont, const bf16* pdys, const bf16* pxs) {
    const int n = ti / L::TPS, ty0 = (ti - n * L::TPS) * L::TH;
    if (cont) {
      // rows 0 .. RR-1 of this tile = rows TH .. TH+RR-1 of the previous one (other buffer)
      constexpr int DQ = RR * L::RS * L::PS / 8, XQ = RR * L::XW * L::XS / 8;   // 16-byte chunks
      const u4* sd = reinterpret_cast<const u4*>(pdys + L::TH * L::RS * L::PS);
      u4* dd = reinterpret_cast<u4*>(dys);
      for (int c = tid; c < DQ; c += 256) dd[c] = sd[c];
      const u4* sx = reinterpret_cast<const u4*>(pxs + L::TH * L::XW * L::XS);
      u4* dxs = reinterpret_cast<u4*>(xs);
      for (int c = tid; c < XQ; c += 256) dxs[c] = sx[c];
    }
#pragma unroll
    for (int i = 0; i < YSL; ++i) {
      if (BAL && i == 1 && cont) continue;
      const int task = ytask(i);
      if (!yhas(i) || (cont && yrow[i] < RR)) continue;
      if constexpr (AP) {
        u4 o[4] = {u4{0u, 0u, 0u, 0u}, u4{0u, 0u, 0u, 0u}, u4{0u, 0u, 0u, 0u}, u4{0u, 0u, 0u, 0u}};
        if (ygo[i] >= 0 && (unsigned)(ty0 - L::PAD + yrow[i]) < (unsigned)L::H) {
          const float* ct = ctab + (n / aa.B) * CTR * L::COUT + 8 * (task & (L::OCT - 1));
          if constexpr (AP == 2) apply_window_codes(wpre[i], ct, L::COUT, o);
          else apply_window_lean(wpre[i], ct, L::COUT, o);
        }
        *reinterpret_cast<u4*>(dys + ylo[i]) = o[0];
        *reinterpret_cast<u4*>(dys + ylo[i] + L::PS) = o[1];
        *reinterpret_cast<u4*>(dys + ylo[i] + L::RS * L::PS) = o[2];
        *reinterpret_cast<u4*>(dys + ylo[i] + (L::RS + 1) * L::PS) = o[3];
      } else {
        *reinterpret_cast<u4*>(dys + ylo[i]) = ypre[i];
      }
    }
#pragma unroll
    for (int i = 0; i < XSL; ++i)
      if (tid + 256 * i < L::XT && !(cont && xrow[i] < RR))
        *reinterpret_cast<u4*>(xs + xlo[i]) = xpre[i];
  };

  // ---- input gradient of one tile (conv_ws_kernel<DgrA2, false>'s tile body)
  auto dgrad_tile = [&](int ti) {
    const int n = ti / L::TPS, ty0 = (ti - n * L::TPS) * L::TH;
#pragma unroll 1
    for (int i0 = 0; i0 < L::GW; i0 += L::GB) {
      int base[L::GB], opix[L::GB];
      bool gv[L::GB];
#pragma unroll
      for (int b = 0; b < L::GB; ++b) {
        const int grp = dwp + L::NDW * (i0 + b);
        const int p = grp * 16 + r16;
        gv[b] = i0 + b < L::GW && grp < L::NG;
        int ry = p / L::W;
        const int rx = p - ry * L::W;
        if constexpr (L::RP) ry *= 2;                     // p enumerates (row pair, column)
        base[b] = gv[b] ? (ry * L::RS + rx) * L::PS : 0;
        opix[b] = ((n * L::H) + ty0 + ry + (L::RP ? (g >> 1) : 0)) * L::W + rx;
      }
      f4 acc[L::GB];
#pragma unroll
      for (int b = 0; b < L::GB; ++b) acc[b] = f4{0.f, 0.f, 0.f, 0.f};
      constexpr int PF = L::PFD;
      bf16x8 bq[PF + 1][L::GB];
      // k-step j: taps 2j, 2j + 1 -- the lane register by whether 2j + 1 starts a filter row
      // or lies past the last tap (compile-time per j)
      auto ld = [&](bf16x8 (&dst)[L::GB], auto jc) {
        constexpr int J = decltype(jc)::value;
        constexpr int t0 = 2 * J;
        if constexpr (L::COUT == 32) {
#pragma unroll
          for (int b = 0; b < L::GB; ++b)
            dst[b] = *reinterpret_cast<const bf16x8*>(dys + base[b] + ln_a + tapoff<L>(J));
          return;
        }
        const int ln = (!L::RP && t0 + 1 >= L::KK) ? ln_c : ((t0 % L::K) == L::K - 1 ? ln_b : ln_a);
#pragma unroll
        for (int b = 0; b < L::GB; ++b)
          dst[b] = *reinterpret_cast<const bf16x8*>(dys + base[b] + ln + tapoff<L>(t0));
      };
      static_for<0, (PF < L::KS ? PF : L::KS)>([&](auto jc) { ld(bq[decltype(jc)::value], jc); });
      // the fragment of k-step j + PF is read before the MFMA of k-step j, and scheduling
      // barriers keep it there: without them (round-6 ISA) the scheduler sank every read to its
      // MFMA, the ring collapsed to one register and each k-step waited out a whole LDS latency
      static_for<0, L::KS>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if constexpr (j + PF < L::KS) ld(bq[(j + PF) % (PF + 1)], IC<j + PF>{});
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int b = 0; b < L::GB; ++b) acc[b] = mma(wa(jc), bq[j % (PF + 1)][b], acc[b]);
        __builtin_amdgcn_sched_barrier(0);
      });
      // rows 4g..4g+3 of the D tile: dX channels 4 (g & 1).. of row y (g < 2) or, with RP, of
      // row y + 1 (g >= 2); without RP rows 8-15 are padding
      if constexpr (L::CIN == 16) {     // a full D tile: dX channels 4 g .. 4 g + 3 of the lane's pixel
#pragma unroll
        for (int b = 0; b < L::GB; ++b) {
          if (!gv[b]) continue;
          const uint32_t lo = pack_bf16x2(acc[b][0], acc[b][1]), hi = pack_bf16x2(acc[b][2], acc[b][3]);
          *reinterpret_cast<uint2*>(dx + (size_t)opix[b] * L::CIN + 4 * g) = make_uint2(lo, hi);
        }
      } else if (L::RP || g < 2) {
#pragma unroll
        for (int b = 0; b < L::GB; ++b) {
          if (!gv[b]) continue;
          const uint32_t lo = pack_bf16x2(acc[b][0], acc[b][1]), hi = pack_bf16x2(acc[b][2], acc[b][3]);
          *reinterpret_cast<uint2*>(dx + (size_t)opix[b] * L::CIN + 4 * (g & 1)) = make_uint2(lo, hi);
        }
      }
    }
  };

  // ---- weight gradient of one tile (wgrad_ws_kernel<WgA2>'s strip body), software-pipelined over k-steps: k-step ks + NPW's fragments (address
  // math included) are read before k-step ks's MFMAs, pinned by scheduling barriers
  auto wg_load = [&](int ks, u2 (&af)[2], u2 (&bb)[L::NW][2]) {
    int pa[2], xb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int P = 32 * ks + kpix(g, h, q4);
      const int r = P / L::W, ox = P - r * L::W;
      pa[h] = ((r + L::PAD) * L::RS + ox + L::PAD) * L::PS + 4 * p4;
      xb[h] = (r * L::XW + ox) * L::XS;
    }
    af[0] = tr4(dys + pa[0]);
    af[1] = tr4(dys + pa[1]);
#pragma unroll
    for (int j = 0; j < L::NW; ++j) {
      bb[j][0] = tr4(xs + xb[0] + xo[j]);
      bb[j][1] = tr4(xs + xb[1] + xo[j]);
    }
  };
  // WGU: k-step KS starts at the constant pixel 32 KS = (row r0, column c0); the lane's pixel
  // is kp < 32 further on, so its row is r0 or -- only where c0 + 31 >= W, and then for the
  // lanes with kp >= W - c0 -- r0 + 1.  The constant part of both offsets folds into the
  // ds_read offset fields; same pixels, fragments and MFMA order as wg_load.
  const int kp0 = kpix(g, 0, q4);                       // h = 1: kp0 + 8
  const int lpa = kp0 * L::PS + 4 * p4;
  int lxo[L::NW];
#pragma unroll
  for (int j = 0; j < L::NW; ++j) lxo[j] = kp0 * L::XS + xo[j];
  auto wg_load_c = [&](auto ksc, u2 (&af)[2], u2 (&bb)[L::NW][2]) {
    constexpr int P0 = 32 * decltype(ksc)::value, r0 = P0 / L::W, c0 = P0 % L::W;
    constexpr int cpa = ((r0 + L::PAD) * L::RS + c0 + L::PAD) * L::PS, cxb = (r0 * L::XW + c0) * L::XS;
    constexpr int wpa = (L::RS - L::W) * L::PS, wxb = (L::XW - L::W) * L::XS;   // one row on
    static_for<0, 2>([&](auto hc) {
      constexpr int h = decltype(hc)::value;
      int pa = lpa, xw = 0;
      if constexpr (c0 + 8 * h + 23 >= L::W) {          // kp0 <= 23
        const bool wr = kp0 + 8 * h >= L::W - c0;
        pa += wr ? wpa : 0;
        xw = wr ? wxb : 0;
      }
      af[h] = tr4(dys + pa + (cpa + 8 * h * L::PS));
#pragma unroll
      for (int j = 0; j < L::NW; ++j) bb[j][h] = tr4(xs + (lxo[j] + xw) + (cxb + 8 * h * L::XS));
    });
  };
  // the tile's interior pixel P (row P / W, column P % W) sits at dY tile row + PAD, column + PAD
  auto wgrad_tile = [&]() {
    if constexpr (L::WGU == 2) {
      // step s = (k-step s / NW = the tile's padded row, column tile s % NW): B fragments WFD
      // steps ahead of their MFMAs across k-step ends, the next row's MT A fragments read at the
      // row's first step; WgA3's pixel and column maps (kpix, xo)
      constexpr int S = L::WKS * L::NW, PF = L::WFD;
      u2 af[2][L::MT][2], bq[PF + 1][2];
      auto ld_a = [&](auto ksc, u2 (&dst)[L::MT][2]) {
        constexpr int cpa = ((decltype(ksc)::value + L::PAD) * L::RS + L::PAD) * L::PS;
#pragma unroll
        for (int m = 0; m < L::MT; ++m) {
          dst[m][0] = tr4(dys + lpa + (cpa + 16 * m));
          dst[m][1] = tr4(dys + lpa + (cpa + 16 * m + 8 * L::PS));
        }
      };
      auto ld_b = [&](auto sc, u2 (&dst)[2]) {
        constexpr int ks = decltype(sc)::value / L::NW, j = decltype(sc)::value % L::NW;
        constexpr int cxb = ks * L::XW * L::XS;
        dst[0] = tr4(xs + lxo[j] + cxb);
        dst[1] = tr4(xs + lxo[j] + (cxb + 8 * L::XS));
      };
      ld_a(IC<0>{}, af[0]);
      static_for<0, (PF < S ? PF : S)>([&](auto sc) { ld_b(sc, bq[decltype(sc)::value]); });
      static_for<0, S>([&](auto sc) {
        constexpr int s = decltype(sc)::value, ks = s / L::NW, j = s % L::NW;
        if constexpr (s + PF < S) ld_b(IC<s + PF>{}, bq[(s + PF) % (PF + 1)]);
        if constexpr (j == 0 && ks + 1 < L::WKS) ld_a(IC<ks + 1>{}, af[(ks + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        const bf16x8 b8 = frag8(bq[s % (PF + 1)][0], bq[s % (PF + 1)][1]);
#pragma unroll
        for (int m = 0; m < L::MT; ++m)
          wacc[m * L::NW + j] = mma(frag8(af[ks & 1][m][0], af[ks & 1][m][1]), b8, wacc[m * L::NW + j]);
        __builtin_amdgcn_sched_barrier(0);
      });
      return;
    }
    static_assert(L::WGU == 2 || L::MT == 1, "the k-step-buffered loops hold one A fragment");
    if constexpr (L::WGU) {
      u2 af[2][2], bb[2][L::NW][2];
      wg_load_c(IC<0>{}, af[0], bb[0]);
      static_for<0, L::WKS>([&](auto kc) {
        constexpr int ks = decltype(kc)::value, c = ks & 1;
        if constexpr (ks + 1 < L::WKS) wg_load_c(IC<ks + 1>{}, af[c ^ 1], bb[c ^ 1]);
        __builtin_amdgcn_sched_barrier(0);
        const bf16x8 a8 = frag8(af[c][0], af[c][1]);
#pragma unroll
        for (int j = 0; j < L::NW; ++j) wacc[j] = mma(a8, frag8(bb[c][j][0], bb[c][j][1]), wacc[j]);
        __builtin_amdgcn_sched_barrier(0);
      });
      return;
    }
    int ks = wq;
    if (ks >= L::WKS) return;
    u2 af[2][2], bb[2][L::NW][2];
    wg_load(ks, af[0], bb[0]);
#pragma unroll 2
    for (int it = 0; ks < L::WKS; ks += L::NPW, ++it) {
      const int c = it & 1;
      if (ks + L::NPW < L::WKS) wg_load(ks + L::NPW, af[c ^ 1], bb[c ^ 1]);
      __builtin_amdgcn_sched_barrier(0);
      const bf16x8 a8 = frag8(af[c][0], af[c][1]);
#pragma unroll
      for (int j = 0; j < L::NW; ++j) wacc[j] = mma(a8, frag8(bb[c][j][0], bb[c][j][1]), wacc[j]);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  {
    // tile ti in buffer (ti - t0) & 1: its MFMAs, then tile ti + 1 staged into the other buffer
    // (its loads were issued one tile earlier), then the loads of tile ti + 2; one barrier
    if (t0 < t1) {
      load_tile(t0, false);
      __syncthreads();   // ctab is written
      set_buf(0);
      store_tile(t0, false, nullptr, nullptr);
      if (t0 + 1 < t1) load_tile(t0 + 1, (t0 + 1) % L::TPS != 0);
      __syncthreads();
    }
    for (int ti = t0; ti < t1; ++ti) {
      const int b = (ti - t0) & 1;
      set_buf(b);
      if (dgw) dgrad_tile(ti);
      if (wgw) wgrad_tile();
      if (ti + 1 < t1) {
        const bf16* pd = dys;     // tile ti's images: its last rows may seed tile ti + 1
        const bf16* px = xs;
        set_buf(b ^ 1);   // last read by tile ti - 1, before the previous barrier
        store_tile(ti + 1, (ti + 1) % L::TPS != 0, pd, px);
        if (ti + 2 < t1) load_tile(ti + 2, (ti + 2) % L::TPS != 0);
      }
      __syncthreads();
    }
  }

  // ---- pixel-split dW partials -> wave 0 (fixed order), slab [co][ci][tap] through LDS
  f4* red = reinterpret_cast<f4*>(smem);
  __syncthreads();
  constexpr int NA = L::MT * L::NW;
  if (wgw && wq > 0) {
#pragma unroll
    for (int j = 0; j < NA; ++j) red[(((wq - 1) * L::NCW + wc) * NA + j) * 64 + lane] = wacc[j];
  }
  __syncthreads();
  if (wgw && wq == 0) {
#pragma unroll
    for (int w = 1; w < L::NPW; ++w)
#pragma unroll
      for (int j = 0; j < NA; ++j) wacc[j] += red[(((w - 1) * L::NCW + wc) * NA + j) * 64 + lane];
  }
  __syncthreads();
  constexpr int PER_CO = L::CIN * L::KK;
  float* tb = reinterpret_cast<float*>(smem);
  static_assert(L::COUT * PER_CO * 4 <= L::SMEM * 2, "slab tile fits");
  if (wgw && wq == 0) {
#pragma unroll
    for (int j = 0; j < L::NW; ++j) {
      const int tap = L::CIN == 8 ? 2 * (wc * L::NW + j) + (r16 >> 3) : wc * L::NW + j;
      const int ci = L::CIN == 8 ? (r16 & 7) : r16;
      if (tap >= L::KK) continue;
#pragma unroll
      for (int m = 0; m < L::MT; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          tb[(16 * m + 4 * g + i) * PER_CO + ci * L::KK + tap] = wacc[m * L::NW + j][i];
    }
  }
  __syncthreads();
  float4* o4 = reinterpret_cast<float4*>(parts + (size_t)blockIdx.x * L::COUT * PER_CO);
  const float4* t4 = reinterpret_cast<const float4*>(tb);
  for (int e = tid; e < L::COUT * PER_CO / 4; e += 256) o4[e] = t4[e];
}

// LBWD_BAL, LBWD_WGU (build-time, for A/B builds): 0 = the apply tasks in linear order on the
// two slots / the rolled weight-gradient loop with its per-k-step divisions
#ifndef LBWD_BAL
#define LBWD_BAL 1
#endif
#ifndef LBWD_WGU
#define LBWD_WGU 1
#endif
//        CIN COUT H   W  TH OCC PFD GB NCW RP BAL       WGU       SP
typedef Lb<8, 16, 56, 56, 8, 2, 3, 1, 4, 1, LBWD_BAL, LBWD_WGU> LbA2;   // audio conv2
// audio conv3: 4-row tiles (7 per sample, continuation rows reused), double-buffered 72 KB, two
// blocks per CU; waves 0-1 input gradient (7 groups of 16 pixels), waves 2-3 weight gradient
// (4 padded rows x 13 column tiles x 2 row tiles each)
#ifndef LBWD28_PFD
#define LBWD28_PFD 3
#endif
#ifndef LBWD28_GB
#define LBWD28_GB 1
#endif
typedef Lb<16, 32, 28, 28, 4, 2, LBWD28_PFD, LBWD28_GB, 2, 0, 0, 2, 1> LbA3;

template <class L>
int lb_occ_ap() {
  static int occ = 0;
  if (!occ) {
    // the least of the two apply variants, so one slab count serves both
    int o1 = 0, o2 = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o1, lbwd_kernel<L, 1>, 256, 0) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&o2, lbwd_kernel<L, 2>, 256, 0) == hipSuccess)
      occ = std::min(o1, o2);
    if (occ <= 0)
      occ = 1;
  }
  return occ;
}

int lb_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
  }
  return cus;
}

template <class L>
bool lb_is(int Cin, int H, int W, int Cout, int K, int pad) {
  return Cin == L::CIN && Cout == L::COUT && K == L::K && pad == L::PAD && H == L::H && W == L::W;
}

// the served shapes: the audio conv2 (56^2, 8 -> 16) and conv3 (28^2, 16 -> 32), 5x5 pad 2, bf16
bool lb_serves(int dt, int N, int Cin, int H, int W, int Cout, int K, int pad) {
  return dt == AVD_BF16 && !g_opts.generic_conv && N > 0 &&
         (lb_is<LbA2>(Cin, H, W, Cout, K, pad) || lb_is<LbA3>(Cin, H, W, Cout, K, pad));
}

template <class L>
int lb_slabs(int N) {
  return std::max(1, grid_cap(std::min(N * L::TPS, lb_cus() * lb_occ_ap<L>())));
}

}  // namespace

int avd_cl_layer_bwd_slabs(int dt, int N, int Cin, int H, int W, int Cout, int K, int pad) {
  if (!lb_serves(dt, N, Cin, H, W, Cout, K, pad)) return 0;
  return lb_is<LbA3>(Cin, H, W, Cout, K, pad) ? lb_slabs<LbA3>(N) : lb_slabs<LbA2>(N);
}

namespace {
template <class L>
int lbwd_launch_as(const void* y, const void* x, const void* wk_d, void* dx, float* parts, int slabs,
                   int N, bool ap, const ApplyArgs& aa, hipStream_t st) {
  const int ntiles = N * L::TPS;
  // the caller's slab count (the parts buffer it sized) is the grid: no re-derivation here
  if (slabs < 1 || slabs > ntiles) return AVD_ERR_ARG;
  if (ap && aa.codes)
    lbwd_kernel<L, 2><<<slabs, 256, 0, st>>>((const bf16*)y, (const bf16*)x, (const bf16*)wk_d, (bf16*)dx,
                                              parts, ntiles, aa);
  else if (ap)
    lbwd_kernel<L, 1><<<slabs, 256, 0, st>>>((const bf16*)y, (const bf16*)x, (const bf16*)wk_d, (bf16*)dx,
                                              parts, ntiles, aa);
  else
    lbwd_kernel<L, 0><<<slabs, 256, 0, st>>>((const bf16*)y, (const bf16*)x, (const bf16*)wk_d, (bf16*)dx,
                                              parts, ntiles, aa);
  AVD_CHECK_LAUNCH();
  return AVD_OK;
}

int lbwd_launch(const void* y, const void* gout, const float* scale, const float* shift,
                const unsigned* codes, const float* coef, const void* dy, const void* x,
                const void* wk_d, void* dx, float* parts, int slabs, int dt, int N, int B, int Cin,
                int H, int W, int Cout, int K, int pad, void* stream) {
  if (!lb_serves(dt, N, Cin, H, W, Cout, K, pad)) {
    avd_set_error(hipErrorInvalidValue);
    return AVD_ERR_SHAPE;
  }
  if (!x || !wk_d || !dx || !parts) return AVD_ERR_ARG;
  const bool ap = y != nullptr;
  if (ap ? (!gout || !coef || (codes ? false : (!scale || !shift))) : !dy) return AVD_ERR_ARG;
  if (ap && (B <= 0 || N % B || N / B > APPLY_GMAX)) return AVD_ERR_SHAPE;
  ApplyArgs aa{};
  aa.gout = gout; aa.scale = scale; aa.shift = shift; aa.coef = coef;
  aa.B = ap ? B : N; aa.G = ap ? N / B : 1;
  aa.codes = codes;
  hipStream_t st = avd_stream(stream);
  const void* src = ap ? y : dy;
  if (lb_is<LbA3>(Cin, H, W, Cout, K, pad))
    return lbwd_launch_as<LbA3>(src, x, wk_d, dx, parts, slabs, N, ap, aa, st);
  return lbwd_launch_as<LbA2>(src, x, wk_d, dx, parts, slabs, N, ap, aa, st);
}
}  // namespace

int avd_cl_layer_bwd(const void* y, const void* gout, const float* scale, const float* shift,
                     const float* coef, const void* dy, const void* x, const void* wk_d, void* dx,
                     float* parts, int slabs, int dt, int N, int B, int Cin, int H, int W, int Cout,
                     int K, int pad, void* stream) {
  return lbwd_launch(y, gout, scale, shift, nullptr, coef, dy, x, wk_d, dx, parts, slabs, dt, N, B,
                     Cin, H, W, Cout, K, pad, stream);
}

int avd_cl_layer_bwd_codes(const void* y, const void* gout, const unsigned* codes, const float* coef,
                           const void* x, const void* wk_d, void* dx, float* parts, int slabs, int dt,
                           int N, int B, int Cin, int H, int W, int Cout, int K, int pad, void* stream) {
  if (!y || !codes) return AVD_ERR_ARG;
  return lbwd_launch(y, gout, nullptr, nullptr, codes, coef, nullptr, x, wk_d, dx, parts, slabs, dt,
                     N, B, Cin, H, W, Cout, K, pad, stream);
}
