// The frozen LPIPS-VGG16 stack on the bf16 matrix cores (--lpips_dtype bf16; include/vts.h "bf16 path of the frozen VGG stack").
//   vts_conv3x3_bf16       stride-1 3x3 convolution as an implicit GEMM on v_mfma_f32_32x32x16_bf16, fp32 accumulators
//   vts_w3x3_bf16_pack     its weights, rounded to nearest even, forward or adjoint (taps flipped, channels swapped)
//   vts_bf16_nhwc_pad      fp32 NCHW -> the layout below (the stem's operand, channels padded with zeros)
//   vts_maxpool2_bf16(_bwd), vts_lpips_layer_bf16   the glue of vts_perceptual.hip in the same layout
// Layout: every activation and gradient map is bf16, channels last, with the next convolution's zero one-pixel border:
// [N][H + 2][W + 2][C].  A lane's 8-element k-fragment of the MFMA is then one 16-byte load, and the LPIPS head reads a pixel's channels
// contiguously.  Values are ReLU outputs (>= 0) or gradients that already carry the ReLU mask.
//
// The convolution: a workgroup (4 waves) owns 8 x 32 output pixels x 64 output channels of one image and walks the input channels in
// chunks of 32.  Per chunk the 10 x 34 halo of the input (64 B per pixel) and the 9 x 64 weight rows (64 B each) are staged through LDS,
// 16-byte slots XOR-swizzled by (row >> 2) & 3 so that the 16 lanes of one ds_read_b128 pass hit 16 different slots; the chunk after it
// is already on its way into registers while the 72 MFMAs per wave of this one run.  A = weights (row = output channel), B = pixels
// (column = x): a lane ends up with 4 consecutive output channels of one pixel per accumulator quad, an 8-byte channels-last store.
// No atomics; each output element is one k-ordered chain of MFMA accumulations, the same for every batch size and image index.
#include <algorithm>

#include "vts_internal.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short us4 __attribute__((ext_vector_type(4)));
typedef unsigned short us8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ unsigned short f2bf(float f) {      // round to nearest even
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
__device__ __forceinline__ float bf2f(unsigned short h) { return __uint_as_float((unsigned)h << 16); }

__device__ __forceinline__ void loss_add64(long long* slot, double v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)llrint(v * VTS_LOSS_SCALE));
}

constexpr int TH = 8, TW = 32, BCO = 64, KC = 32;
constexpr int HH = TH + 2, HWD = TW + 2, HPIX = HH * HWD;           // halo
constexpr int FLAT_PIX = 256, FLAT_IN_PIX = 576;                    // flat mode: output pixels / staged (padded) input pixels per workgroup
constexpr int W_UNITS = 9 * BCO * 4, W_PER_T = W_UNITS / 256;       // 16-byte units per chunk
constexpr int LDS_IN = FLAT_IN_PIX * 64, LDS_W = 9 * BCO * 64;

enum { EP_RELU_PAD = 1, EP_MASK_PAD = 2, EP_DX_F32 = 3 };

__device__ __forceinline__ int swz(int row, int slot) { return row * 64 + ((slot ^ ((row >> 2) & 3)) << 4); }

// FLAT (conv3x3_bf16_kernel<EP, true>, reported as "conv3x3_bf16_kernel<ep, flat>"; maps of at most 256 pixels whose padded form fits 576): a workgroup takes G WHOLE images -- its 256 MFMA columns are consecutive
// pixels of the flattened (image, y, x) index, its LDS holds those images' padded maps, which lie contiguously in memory -- so that the
// 4 x 4 and 2 x 2 maps of the deep layers on patch stacks fill the tile instead of one corner of it.  A pixel's result is the same chain.
template <int EP, bool FLAT>
__global__ __launch_bounds__(256) void conv3x3_bf16_kernel(const unsigned short* __restrict__ in, const unsigned short* __restrict__ wt,
                                                           const float* __restrict__ bias, void* __restrict__ outv, int N, int Cin, int Cout,
                                                           int H, int W, int tiles_x, const unsigned short* __restrict__ add,
                                                           const unsigned short* __restrict__ mask, int co_store) {
  constexpr int IN_PER_T = FLAT ? FLAT_IN_PIX * 4 / 256 : (HPIX * 4 + 255) / 256;
  __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_IN + LDS_W];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int PW = W + 2, PH = H + 2, nch = Cin / KC;
  const int co0 = blockIdx.y * BCO;
  const int CoutP = (Cout + BCO - 1) / BCO * BCO;
  // tiled: tiles_x = tile columns, blockIdx.z = image;  flat: tiles_x = G images per workgroup, blockIdx.x = image group
  const int ty = FLAT ? 0 : blockIdx.x / tiles_x, tx = FLAT ? 0 : blockIdx.x - ty * tiles_x;
  const int y0 = ty * TH, x0 = tx * TW;
  const int n0 = FLAT ? blockIdx.x * tiles_x : blockIdx.z;
  const int gv = FLAT ? min(tiles_x, N - n0) : 1;                       // images this workgroup really has
  const unsigned short* inb = in + (int64_t)n0 * PH * PW * Cin;

  // what this thread stages per chunk: offsets are fixed over the chunks apart from the channel base
  int64_t in_off[IN_PER_T];
  int in_lds[IN_PER_T];
#pragma unroll
  for (int i = 0; i < IN_PER_T; ++i) {
    const int u = tid + 256 * i;
    const int q = u >> 2, slot = u & 3;
    if (FLAT) {
      const bool ok = q < gv * PH * PW;
      in_off[i] = ok ? (int64_t)q * Cin + slot * 8 : -1;
      in_lds[i] = ok ? swz(q, slot) : -1;
    } else {
      const int py = q / HWD, px = q - py * HWD;
      const int gy = y0 + py, gx = x0 + px;
      const bool ok = q < HPIX && gy < PH && gx < PW;
      in_off[i] = ok ? ((int64_t)gy * PW + gx) * Cin + slot * 8 : -1;
      in_lds[i] = q < HPIX ? swz(q, slot) : -1;
    }
  }
  // the two pixels (MFMA column r of the wave's two 32-pixel groups) this lane's B fragments and results belong to
  int pn[2], py_[2], px_[2], qb[2];
  bool pv[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    if (FLAT) {
      const int p = wv * 64 + ni * 32 + r;
      pv[ni] = p < gv * H * W;
      // columns past the last image (a short last group: gv < G; LDS rows past gv * PH * PW are never staged) read pixel 0 of image 0
      // instead: MFMA columns are independent of each other and the epilogue stores nothing for them
      const int pc = pv[ni] ? p : 0;
      const int img = pc / (H * W), rem = pc - img * H * W;
      py_[ni] = rem / W;
      px_[ni] = rem - py_[ni] * W;
      pn[ni] = n0 + img;
      qb[ni] = img * PH * PW + py_[ni] * PW + px_[ni];
    } else {
      py_[ni] = y0 + 2 * wv + ni;
      px_[ni] = x0 + r;
      pn[ni] = n0;
      pv[ni] = py_[ni] < H && px_[ni] < W;
      qb[ni] = (2 * wv + ni) * HWD + r;
    }
  }
  const int qrow = FLAT ? PW : HWD;
  u32x4 rin[IN_PER_T], rw[W_PER_T];
#define VTS_BF16_STAGE_LOAD(ch)                                                                                                  \
  do {                                                                                                                          \
    _Pragma("unroll") for (int i = 0; i < IN_PER_T; ++i) {                                                                      \
      rin[i] = u32x4{0u, 0u, 0u, 0u};                                                                                          \
      if (in_off[i] >= 0) rin[i] = *reinterpret_cast<const u32x4*>(inb + in_off[i] + (ch) * KC);                                \
    }                                                                                                                           \
    _Pragma("unroll") for (int i = 0; i < W_PER_T; ++i) {                                                                       \
      const int u = tid + 256 * i;                                                                                              \
      const int tap = u >> 8, co = (u >> 2) & 63, slot = u & 3;                                                                 \
      rw[i] = *reinterpret_cast<const u32x4*>(wt + (((int64_t)tap * nch + (ch)) * CoutP + co0 + co) * KC + slot * 8);           \
    }                                                                                                                           \
  } while (0)
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  VTS_BF16_STAGE_LOAD(0);
  for (int ch = 0; ch < nch; ++ch) {
    __syncthreads();                               // the MFMAs of the chunk before have read their fragments
#pragma unroll
    for (int i = 0; i < IN_PER_T; ++i)
      if (in_lds[i] >= 0) *reinterpret_cast<u32x4*>(lds + in_lds[i]) = rin[i];
#pragma unroll
    for (int i = 0; i < W_PER_T; ++i) {
      const int u = tid + 256 * i;
      *reinterpret_cast<u32x4*>(lds + LDS_IN + swz(u >> 2, u & 3)) = rw[i];
    }
    __syncthreads();
    if (ch + 1 < nch) VTS_BF16_STAGE_LOAD(ch + 1);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int slot = s * 2 + h;
        bf16x8 a[2], b[2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) a[mi] = *reinterpret_cast<const bf16x8*>(lds + LDS_IN + swz(tap * BCO + mi * 32 + r, slot));
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) b[ni] = *reinterpret_cast<const bf16x8*>(lds + swz(qb[ni] + ky * qrow + kx, slot));
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int y = py_[ni], x = px_[ni], n = pn[ni];
    if (!pv[ni]) continue;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cb = co0 + mi * 32 + 8 * g + 4 * h;
        if (cb >= Cout) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[mi][ni][4 * g + e];
        if (EP == EP_DX_F32) {
          float* out = reinterpret_cast<float*>(outv);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (cb + e < co_store) out[(((int64_t)n * co_store + cb + e) * H + y) * W + x] = v[e];
          continue;
        }
        unsigned short* out = reinterpret_cast<unsigned short*>(outv) + (int64_t)n * PH * PW * Cout + cb;
        const int64_t o = ((int64_t)(y + 1) * PW + x + 1) * Cout;
        us4 res;
        if (EP == EP_RELU_PAD) {
          const f32x4 bv = bias ? *reinterpret_cast<const f32x4*>(bias + cb) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 4; ++e) res[e] = f2bf(fmaxf(v[e] + bv[e], 0.f));
        } else {
          const int64_t mo = (int64_t)n * PH * PW * Cout + cb + o;
          const us4 mv = *reinterpret_cast<const us4*>(mask + mo);
          us4 av = us4{0, 0, 0, 0};
          if (add) av = *reinterpret_cast<const us4*>(add + mo);
#pragma unroll
          for (int e = 0; e < 4; ++e) res[e] = bf2f(mv[e]) > 0.f ? f2bf(v[e] + bf2f(av[e])) : (unsigned short)0;
        }
        *reinterpret_cast<us4*>(out + o) = res;
        // the zero border next to this pixel
        const us4 z = us4{0, 0, 0, 0};
        const bool l = x == 0, rr = x == W - 1, t = y == 0, bt = y == H - 1;
        if (l) *reinterpret_cast<us4*>(out + ((int64_t)(y + 1) * PW) * Cout) = z;
        if (rr) *reinterpret_cast<us4*>(out + ((int64_t)(y + 1) * PW + W + 1) * Cout) = z;
        if (t) *reinterpret_cast<us4*>(out + (int64_t)(x + 1) * Cout) = z;
        if (bt) *reinterpret_cast<us4*>(out + ((int64_t)(H + 1) * PW + x + 1) * Cout) = z;
        if (l && t) *reinterpret_cast<us4*>(out) = z;
        if (rr && t) *reinterpret_cast<us4*>(out + (int64_t)(W + 1) * Cout) = z;
        if (l && bt) *reinterpret_cast<us4*>(out + ((int64_t)(H + 1) * PW) * Cout) = z;
        if (rr && bt) *reinterpret_cast<us4*>(out + ((int64_t)(H + 1) * PW + W + 1) * Cout) = z;
      }
  }
}

// packed weights [tap][AP / 32][BP][32]: a = input channel of the convolution (AP = A rounded up to 32), b = its output channel (BP = B
// rounded up to 64); zeros outside A x B
__global__ __launch_bounds__(256) void w3x3_bf16_pack_kernel(const float* __restrict__ w, int A, int B, int64_t sa, int64_t sb, int flip, int AP,
                                                             int BP, unsigned short* __restrict__ out) {
  const int64_t total = (int64_t)9 * AP * BP;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int cc = (int)(i & 31);
    int64_t t = i >> 5;
    const int b = (int)(t % BP);
    t /= BP;
    const int chunk = (int)(t % (AP / 32)), tap = (int)(t / (AP / 32));
    const int a = chunk * 32 + cc;
    out[i] = (a < A && b < B) ? f2bf(w[a * sa + b * sb + (flip ? 8 - tap : tap)]) : (unsigned short)0;
  }
}

// fp32 [N][C][H][W] -> bf16 [N][H + 2][W + 2][CP], zero border, zero channels >= C; thread = (padded pixel, 8-channel group)
__global__ __launch_bounds__(256) void bf16_nhwc_pad_kernel(const float* __restrict__ x, int C, int H, int W, int CP, int64_t total,
                                                            unsigned short* __restrict__ out) {
  const int G = CP / 8, PW = W + 2, PH = H + 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int g = (int)(i % G);
    int64_t p = i / G;
    const int px = (int)(p % PW);
    p /= PW;
    const int py = (int)(p % PH), n = (int)(p / PH);
    us8 v = us8{0, 0, 0, 0, 0, 0, 0, 0};
    if (py >= 1 && py <= H && px >= 1 && px <= W) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = g * 8 + j;
        if (c < C) v[j] = f2bf(x[(((int64_t)n * C + c) * H + py - 1) * W + px - 1]);
      }
    }
    *reinterpret_cast<us8*>(out + i * 8) = v;
  }
}

// out [N][OH + 2][OW + 2][C] <- 2 x 2 maximum of the interior of z [N][H + 2][W + 2][C] (values >= 0: ReLU outputs), zero border
__global__ __launch_bounds__(256) void maxpool2_bf16_kernel(const unsigned short* __restrict__ z, int C, int H, int W, int64_t total,
                                                            unsigned short* __restrict__ out) {
  const int G = C / 8, OH = H >> 1, OW = W >> 1, QW = OW + 2, QH = OH + 2, PW = W + 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int g = (int)(i % G);
    int64_t p = i / G;
    const int qx = (int)(p % QW);
    p /= QW;
    const int qy = (int)(p % QH), n = (int)(p / QH);
    us8 v = us8{0, 0, 0, 0, 0, 0, 0, 0};
    if (qy >= 1 && qy <= OH && qx >= 1 && qx <= OW) {
      const unsigned short* q = z + (((int64_t)n * (H + 2) + 2 * (qy - 1) + 1) * PW + 2 * (qx - 1) + 1) * C + g * 8;
      const us8 a = *reinterpret_cast<const us8*>(q), b = *reinterpret_cast<const us8*>(q + C);
      const us8 c = *reinterpret_cast<const us8*>(q + (int64_t)PW * C), d = *reinterpret_cast<const us8*>(q + (int64_t)PW * C + C);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float m = fmaxf(fmaxf(bf2f(a[j]), bf2f(b[j])), fmaxf(bf2f(c[j]), bf2f(d[j])));
        v[j] = (unsigned short)(__float_as_uint(fmaxf(m, 0.f)) >> 16);
      }
    }
    *reinterpret_cast<us8*>(out + i * 8) = v;
  }
}

// adjoint of the pooling: gz [N][H + 2][W + 2][C] (zero border) <- g [N][OH + 2][OW + 2][C] routed to the FIRST element (row-major) that
// holds its window's maximum where that is positive (the rule of vts_maxpool2_relu_bwd), plus g2 (z's layout, optional) where z > 0
__global__ __launch_bounds__(256) void maxpool2_bf16_bwd_kernel(const unsigned short* __restrict__ gr, const unsigned short* __restrict__ z,
                                                                const unsigned short* __restrict__ g2, int C, int H, int W, int64_t total,
                                                                unsigned short* __restrict__ gz) {
  const int G = C / 8, OH = H >> 1, OW = W >> 1, QW = OW + 2, PW = W + 2, PH = H + 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int g = (int)(i % G);
    int64_t p = i / G;
    const int px = (int)(p % PW);
    p /= PW;
    const int py = (int)(p % PH), n = (int)(p / PH);
    us8 v = us8{0, 0, 0, 0, 0, 0, 0, 0};
    if (py >= 1 && py <= H && px >= 1 && px <= W) {
      const int y = py - 1, x = px - 1, wy = y >> 1, wx = x >> 1;
      float r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = 0.f;
      const us8 own = *reinterpret_cast<const us8*>(z + i * 8);
      if (wy < OH && wx < OW) {
        const unsigned short* q = z + (((int64_t)n * PH + 2 * wy + 1) * PW + 2 * wx + 1) * C + g * 8;
        us8 e[4];
        e[0] = *reinterpret_cast<const us8*>(q);
        e[1] = *reinterpret_cast<const us8*>(q + C);
        e[2] = *reinterpret_cast<const us8*>(q + (int64_t)PW * C);
        e[3] = *reinterpret_cast<const us8*>(q + (int64_t)PW * C + C);
        const us8 gv = *reinterpret_cast<const us8*>(gr + (((int64_t)n * (OH + 2) + wy + 1) * QW + wx + 1) * C + g * 8);
        const int k = (y & 1) * 2 + (x & 1);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float f[4] = {bf2f(e[0][j]), bf2f(e[1][j]), bf2f(e[2][j]), bf2f(e[3][j])};
          const float m = fmaxf(fmaxf(f[0], f[1]), fmaxf(f[2], f[3]));
          bool first = f[k] == m && m > 0.f;
#pragma unroll
          for (int t = 0; t < 3; ++t) first = first && (t >= k || f[t] != m);
          if (first) r[j] = bf2f(gv[j]);
        }
      }
      if (g2) {
        const us8 tv = *reinterpret_cast<const us8*>(g2 + i * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (bf2f(own[j]) > 0.f) r[j] += bf2f(tv[j]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = f2bf(r[j]);
    }
    *reinterpret_cast<us8*>(gz + i * 8) = v;
  }
}

// LPIPS head of one tap on bf16 channels-last features (the arithmetic of lpips_layer_kernel in fp32): 8 lanes share a pixel, lane j takes
// the 16-byte channel groups j, j + 8, ...; the channel sums cross the 8 lanes by an XOR butterfly (every lane gets the same bits).
// dz0 (optional, bf16, z0's layout) gets its zero border here.
template <int CPL>
__global__ __launch_bounds__(256) void lpips_layer_bf16_kernel(const unsigned short* __restrict__ z0, const unsigned short* __restrict__ z1, int H,
                                                               int W, const float* __restrict__ w, float coeff, long long* __restrict__ loss,
                                                               unsigned short* __restrict__ dz0, float grad_coeff, int iters) {
  constexpr int C = CPL * 8, NG = CPL / 8;
  __shared__ float red[16];
  const int n = blockIdx.y, j = threadIdx.x & 7;
  const int PW = W + 2, PH = H + 2, HW = H * W;
  float sum = 0.f;
  for (int it = 0; it < iters; ++it) {          // `iters` groups of 32 pixels per workgroup: one fixed-point add per workgroup, not per 32 pixels
  const int pi = (blockIdx.x * iters + it) * 32 + (threadIdx.x >> 3);
  const bool live = pi < PH * PW;
  const int py = pi / PW, px = pi - py * PW;
  const bool inner = live && py >= 1 && py <= H && px >= 1 && px <= W;
  const int64_t base = ((int64_t)n * PH * PW + (live ? pi : 0)) * C;
  const float eps = 1e-10f;
  float f0[CPL], f1[CPL];
#pragma unroll
  for (int k = 0; k < NG; ++k) {
    us8 a = us8{0, 0, 0, 0, 0, 0, 0, 0}, b = a;
    if (inner) {
      a = *reinterpret_cast<const us8*>(z0 + base + (k * 8 + j) * 8);
      b = *reinterpret_cast<const us8*>(z1 + base + (k * 8 + j) * 8);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      f0[k * 8 + e] = fmaxf(bf2f(a[e]), 0.f);
      f1[k * 8 + e] = fmaxf(bf2f(b[e]), 0.f);
    }
  }
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    s0 = fmaf(f0[c], f0[c], s0);
    s1 = fmaf(f1[c], f1[c], s1);
  }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) {
    s0 += __shfl_xor(s0, o, 64);
    s1 += __shfl_xor(s1, o, 64);
  }
  const float r0 = sqrtf(s0), r1 = sqrtf(s1);
  const float i0 = 1.f / (r0 + eps), i1 = 1.f / (r1 + eps);
  float d = 0.f, S = 0.f;
#pragma unroll
  for (int k = 0; k < NG; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = k * 8 + e;
      const float t = f0[c] * i0 - f1[c] * i1;
      const float wt = w[(k * 8 + j) * 8 + e] * t;
      d = fmaf(wt, t, d);
      S = fmaf(wt, f0[c], S);
    }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) {
    d += __shfl_xor(d, o, 64);
    S += __shfl_xor(S, o, 64);
  }
  if (dz0 && live) {
    const float k1 = 2.f * grad_coeff / (float)HW * i0;
    const float k2 = r0 > 0.f ? 2.f * grad_coeff / (float)HW * S * i0 * i0 / r0 : 0.f;
#pragma unroll
    for (int k = 0; k < NG; ++k) {
      us8 o8;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = k * 8 + e;
        const float t = f0[c] * i0 - f1[c] * i1;
        o8[e] = (inner && f0[c] > 0.f) ? f2bf(k1 * w[(k * 8 + j) * 8 + e] * t - k2 * f0[c]) : (unsigned short)0;
      }
      *reinterpret_cast<us8*>(dz0 + base + (k * 8 + j) * 8) = o8;
    }
  }
  sum += inner && j == 0 ? d : 0.f;
  }
  const float acc = block_sum(sum, red);
  if (threadIdx.x == 0 && loss) loss_add64(loss, (double)acc * (double)coeff / (double)HW);
}

inline int blocks64(int64_t total) { return (int)((total + 255) / 256 < 65536 * 16 ? (total + 255) / 256 : 65536 * 16); }
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int64_t vts_w3x3_bf16_elems(int A, int B) {
  if (A < 1 || B < 1) return 0;
  return (int64_t)9 * ((A + 31) / 32 * 32) * ((B + 63) / 64 * 64);
}

extern "C" int vts_w3x3_bf16_pack(const float* w, int A, int B, int64_t sa, int64_t sb, int flip, void* wt, void* stream) {
  VTS_CHECK_ARG(w && wt && A >= 1 && B >= 1 && al16(wt), "vts_w3x3_bf16_pack: bad args");
  const int AP = (A + 31) / 32 * 32, BP = (B + 63) / 64 * 64;
  hipLaunchKernelGGL(w3x3_bf16_pack_kernel, dim3(blocks64((int64_t)9 * AP * BP)), dim3(256), 0, (hipStream_t)stream, w, A, B, sa, sb, flip, AP, BP,
                     reinterpret_cast<unsigned short*>(wt));
  vts_set_kernel("w3x3_bf16_pack_kernel");
  VTS_CHECK_LAUNCH("vts_w3x3_bf16_pack");
  return VTS_OK;
}

extern "C" int vts_conv3x3_bf16_ok(int N, int Cin, int Cout, int H, int W) {
  if (N < 1 || N > 65535 || H < 1 || W < 1 || Cin < 32 || Cout < 32 || Cin % 32 || Cout % 32) return 0;
  if ((int64_t)cdiv(H, TH) * cdiv(W, TW) > 0x7fffffff || cdiv(Cout, BCO) > 65535) return 0;
  return 1;
}

extern "C" int vts_conv3x3_bf16(const void* in, const void* wt, const float* bias, void* out, int N, int Cin, int Cout, int H, int W, int ep_mode,
                                const void* ep_add, const void* ep_mask, int co_store, void* stream) {
  VTS_CHECK_ARG(in && wt && out && al16(in) && al16(wt) && al16(out), "vts_conv3x3_bf16: null or misaligned pointer");
  VTS_CHECK_ARG(ep_mode >= EP_RELU_PAD && ep_mode <= EP_DX_F32, "vts_conv3x3_bf16: ep_mode %d", ep_mode);
  if (!vts_conv3x3_bf16_ok(N, Cin, Cout, H, W)) {
    vts_set_error("vts_conv3x3_bf16: N%d %d -> %d channels on %dx%d is not taken (channels must be multiples of 32)", N, Cin, Cout, H, W);
    return VTS_ERR_UNSUPPORTED;
  }
  VTS_CHECK_ARG(ep_mode != EP_MASK_PAD || (ep_mask && al16(ep_mask) && (!ep_add || al16(ep_add))), "vts_conv3x3_bf16: mask epilogue needs ep_mask");
  VTS_CHECK_ARG(ep_mode != EP_DX_F32 || (co_store >= 1 && co_store <= Cout), "vts_conv3x3_bf16: co_store %d", co_store);
  VTS_CHECK_ARG(!bias || al16(bias), "vts_conv3x3_bf16: misaligned bias");
  hipStream_t st = (hipStream_t)stream;
  auto* i16 = reinterpret_cast<const unsigned short*>(in);
  auto* w16 = reinterpret_cast<const unsigned short*>(wt);
  auto* a16 = reinterpret_cast<const unsigned short*>(ep_add);
  auto* m16 = reinterpret_cast<const unsigned short*>(ep_mask);
  static const char* const ep_name[4] = {"", "relu_pad", "mask_pad", "dx_f32"};
#define VTS_BF16_LAUNCH(EPV, FLATV, GRID, TX)                                                                                     \
  hipLaunchKernelGGL((conv3x3_bf16_kernel<EPV, FLATV>), GRID, dim3(256), 0, st, i16, w16, bias, out, N, Cin, Cout, H, W, TX, a16, m16, co_store)
  if (H * W <= FLAT_PIX && (H + 2) * (W + 2) <= FLAT_IN_PIX) {          // small maps: whole images, flattened
    const int G = std::min(FLAT_PIX / (H * W), FLAT_IN_PIX / ((H + 2) * (W + 2)));
    const dim3 grid(cdiv(N, G), cdiv(Cout, BCO), 1);
    if (ep_mode == EP_RELU_PAD) VTS_BF16_LAUNCH(EP_RELU_PAD, true, grid, G);
    else if (ep_mode == EP_MASK_PAD) VTS_BF16_LAUNCH(EP_MASK_PAD, true, grid, G);
    else VTS_BF16_LAUNCH(EP_DX_F32, true, grid, G);
    vts_set_kernel("conv3x3_bf16_kernel<%s, flat>", ep_name[ep_mode]);
  } else {
    const int tiles_x = cdiv(W, TW);
    const dim3 grid(tiles_x * cdiv(H, TH), cdiv(Cout, BCO), N);
    if (ep_mode == EP_RELU_PAD) VTS_BF16_LAUNCH(EP_RELU_PAD, false, grid, tiles_x);
    else if (ep_mode == EP_MASK_PAD) VTS_BF16_LAUNCH(EP_MASK_PAD, false, grid, tiles_x);
    else VTS_BF16_LAUNCH(EP_DX_F32, false, grid, tiles_x);
    vts_set_kernel("conv3x3_bf16_kernel<%s>", ep_name[ep_mode]);
  }
#undef VTS_BF16_LAUNCH
  VTS_CHECK_LAUNCH("vts_conv3x3_bf16");
  return VTS_OK;
}

extern "C" int vts_bf16_nhwc_pad(const float* x, int N, int C, int H, int W, int CP, void* out, void* stream) {
  VTS_CHECK_ARG(x && out && al16(out) && N >= 1 && C >= 1 && H >= 1 && W >= 1 && CP >= C && CP % 8 == 0, "vts_bf16_nhwc_pad: bad args");
  const int64_t total = (int64_t)N * (H + 2) * (W + 2) * (CP / 8);
  hipLaunchKernelGGL(bf16_nhwc_pad_kernel, dim3(blocks64(total)), dim3(256), 0, (hipStream_t)stream, x, C, H, W, CP, total,
                     reinterpret_cast<unsigned short*>(out));
  vts_set_kernel("bf16_nhwc_pad_kernel");
  VTS_CHECK_LAUNCH("vts_bf16_nhwc_pad");
  return VTS_OK;
}

extern "C" int vts_maxpool2_bf16(const void* z, int N, int C, int H, int W, void* out, void* stream) {
  VTS_CHECK_ARG(z && out && al16(z) && al16(out) && N >= 1 && C >= 8 && C % 8 == 0 && H >= 2 && W >= 2, "vts_maxpool2_bf16: bad args");
  const int64_t total = (int64_t)N * (H / 2 + 2) * (W / 2 + 2) * (C / 8);
  hipLaunchKernelGGL(maxpool2_bf16_kernel, dim3(blocks64(total)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const unsigned short*>(z), C, H, W,
                     total, reinterpret_cast<unsigned short*>(out));
  vts_set_kernel("maxpool2_bf16_kernel");
  VTS_CHECK_LAUNCH("vts_maxpool2_bf16");
  return VTS_OK;
}

extern "C" int vts_maxpool2_bf16_bwd(const void* g, const void* z, const void* g2, int N, int C, int H, int W, void* gz, void* stream) {
  VTS_CHECK_ARG(g && z && gz && al16(g) && al16(z) && al16(gz) && (!g2 || al16(g2)) && N >= 1 && C >= 8 && C % 8 == 0 && H >= 2 && W >= 2,
                "vts_maxpool2_bf16_bwd: bad args");
  const int64_t total = (int64_t)N * (H + 2) * (W + 2) * (C / 8);
  hipLaunchKernelGGL(maxpool2_bf16_bwd_kernel, dim3(blocks64(total)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const unsigned short*>(g),
                     reinterpret_cast<const unsigned short*>(z), reinterpret_cast<const unsigned short*>(g2), C, H, W, total,
                     reinterpret_cast<unsigned short*>(gz));
  vts_set_kernel("maxpool2_bf16_bwd_kernel");
  VTS_CHECK_LAUNCH("vts_maxpool2_bf16_bwd");
  return VTS_OK;
}

extern "C" int vts_lpips_layer_bf16(const void* z0, const void* z1, int N, int C, int H, int W, const float* w, float coeff, int64_t* loss_slot,
                                    void* dz0, float grad_coeff, void* stream) {
  VTS_CHECK_ARG(z0 && z1 && w && al16(z0) && al16(z1) && (!dz0 || al16(dz0)) && N >= 1 && N <= 65535 && H >= 1 && W >= 1, "vts_lpips_layer_bf16: bad args");
  if (C != 64 && C != 128 && C != 256 && C != 512) {
    vts_set_error("vts_lpips_layer_bf16: C = %d (64, 128, 256 or 512: the VGG16 taps)", C);
    return VTS_ERR_UNSUPPORTED;
  }
  auto* slot = reinterpret_cast<long long*>(loss_slot);
  auto* a = reinterpret_cast<const unsigned short*>(z0);
  auto* b = reinterpret_cast<const unsigned short*>(z1);
  auto* d = reinterpret_cast<unsigned short*>(dz0);
  const int groups = cdiv((H + 2) * (W + 2), 32), iters = std::max(1, std::min(16, groups / 64));
  const dim3 grid(cdiv(groups, iters), N);
  hipStream_t st = (hipStream_t)stream;
  if (C == 64) hipLaunchKernelGGL(lpips_layer_bf16_kernel<8>, grid, dim3(256), 0, st, a, b, H, W, w, coeff, slot, d, grad_coeff, iters);
  else if (C == 128) hipLaunchKernelGGL(lpips_layer_bf16_kernel<16>, grid, dim3(256), 0, st, a, b, H, W, w, coeff, slot, d, grad_coeff, iters);
  else if (C == 256) hipLaunchKernelGGL(lpips_layer_bf16_kernel<32>, grid, dim3(256), 0, st, a, b, H, W, w, coeff, slot, d, grad_coeff, iters);
  else hipLaunchKernelGGL(lpips_layer_bf16_kernel<64>, grid, dim3(256), 0, st, a, b, H, W, w, coeff, slot, d, grad_coeff, iters);
  vts_set_kernel("lpips_layer_bf16_kernel<%d>", C);
  VTS_CHECK_LAUNCH("vts_lpips_layer_bf16");
  return VTS_OK;
}
