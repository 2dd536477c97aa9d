// CLIP ViT image tower, forward and input-gradient backward (include/vts.h "CLIP ViT image tower"): skitG's style encoder, and the
// frozen feature extractor a vision-aided discriminator differentiates through.
//   vts_gemm_f16            skinny weight-streaming GEMM on v_mfma_f32_16x16x32_f16 (M = tokens x batch, a few hundred rows at most)
//   vts_layernorm_rows      row LayerNorm, fp32 statistics;  vts_layernorm_rows_bwd its input gradient
//   vts_vit_attention       one workgroup per (image, head), one wave per 16 queries, T <= 64, head dimension 64;  vts_vit_attention_bwd
//   vts_clip_preprocess     Pillow's fixed-point bicubic resize + CLIP normalisation, bit-exact with the host chain
//   vts_clip_area_preprocess / _bwd   the differentiable front end: area pooling + CLIP normalisation
//   vts_clip_visual_forward the whole tower as one call;  vts_clip_visual_forward_tape the same, keeping what the backward reads
//   vts_clip_visual_backward          the gradient of the tower's embedding and hidden states with respect to its input
// fp16 travels through the C ABI as uint16_t bit patterns and is _Float16 in here.
#include "vts_internal.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 half_t;

// ---- GEMM ------------------------------------------------------------------------------------------------------------------------------
// A workgroup (4 waves) owns the 32 output features n0 .. n0+31 over all M rows; blockIdx.y = z is the split of K.  The K/32 MFMA steps
// are dealt round-robin to the KS*4 waves of a slab (unit u = z*4 + wave takes steps u, u + KS*4, ...): every wave reads each W fragment
// it needs exactly once, straight from memory in the MFMA's B layout (lane l: W[n0 + (l&15)][k + 8*(l>>4) .. +7], 16 bytes), and the A
// fragments of all row tiles in the A layout (lane l: A[m0 + (l&15)][k + 8*(l>>4) .. +7]).  The accumulator of a 16x16 tile holds
// C[m0 + 4*(l>>4) + i][n0 + (l&15)] in element i.  The four waves' sums are added in wave order through LDS, the KS splits in split order
// by gemm_f16_reduce_kernel: no atomics, so repeats are bit-identical.
// aux (fp16 [M][N], may be NULL): with VTS_GEMM_QUICKGELU the pre-activation is written there too (the tape of the backward); with
// VTS_GEMM_QUICKGELU_BWD it is that saved pre-activation h, and v is multiplied by QuickGELU'(h) = s (1 + 1.702 h (1 - s)), s = sigmoid(1.702 h)
__device__ __forceinline__ void gemm_store(float v, int m, int n, int N, const half_t* bias, int epi, void* out, int out_f16, half_t* aux) {
  if (bias) v += (float)bias[n];
  const size_t o = (size_t)m * N + n;
  if (epi == VTS_GEMM_QUICKGELU) {
    if (aux) aux[o] = (half_t)v;
    v = v / (1.f + expf(-1.702f * v));
  } else if (epi == VTS_GEMM_QUICKGELU_BWD) {
    const float h = (float)aux[o], s = 1.f / (1.f + expf(-1.702f * h));
    v *= s * (1.f + 1.702f * h * (1.f - s));
  }
  if (epi == VTS_GEMM_RESIDUAL) {
    ((float*)out)[o] += v;
  } else if (out_f16) {
    ((half_t*)out)[o] = (half_t)v;
  } else {
    ((float*)out)[o] = v;
  }
}

// UNR steps of a wave are loaded before the first of their MFMAs issues, so a wave's few steps overlap their memory latency (these
// GEMMs are latency-bound: a wave has 1 .. 6 steps).  The four waves' accumulators meet in LDS (GT row tiles at a time, 64 KB at most)
// and all 256 threads sum them in wave order and run the epilogue: thread (wave w, lane l) owns element i = w of every 16x16 tile.
template <int MT, int UNR>
__global__ __launch_bounds__(256) void gemm_f16_kernel(const half_t* __restrict__ A, const half_t* __restrict__ W, const half_t* __restrict__ bias,
                                                        int M, int N, int K, int epi, void* out, int out_f16, float* part, int KS, half_t* aux) {
  constexpr int GT = MT < 8 ? MT : 8;
  __shared__ float red[4][GT * 2 * 4 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * 32, z = blockIdx.y;
  const bool two = n0 + 16 < N;      // N % 16 == 0: the slab's second half is whole or absent
  const half_t* w0 = W + (size_t)(n0 + r) * K + 8 * q;
  const half_t* w1 = W + (size_t)(n0 + (two ? 16 : 0) + r) * K + 8 * q;
  const int S = K / 32, U = KS * 4, u = z * 4 + wave;
  for (int mb = 0; mb < M; mb += MT * 16) {
    f32x4 acc[MT][2];
    const half_t* ap[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      acc[t][0] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
      int row = mb + t * 16 + r;
      row = row < M ? row : M - 1;        // row tail: read a valid row, never stored
      ap[t] = A + (size_t)row * K + 8 * q;
    }
    for (int s = u; s < S; s += U * UNR) {
      h8 b0[UNR], b1[UNR], a[UNR][MT];
#pragma unroll
      for (int j = 0; j < UNR; ++j) {
        const int sj = s + j * U;
        const int k = (sj < S ? sj : s) * 32;      // past the end: a valid address, the products are skipped
        b0[j] = *(const h8*)(w0 + k);
        b1[j] = *(const h8*)(w1 + k);
#pragma unroll
        for (int t = 0; t < MT; ++t) a[j][t] = *(const h8*)(ap[t] + k);
      }
#pragma unroll
      for (int j = 0; j < UNR; ++j) {
        if (s + j * U < S) {
#pragma unroll
          for (int t = 0; t < MT; ++t) {
            if (mb + t * 16 < M) {
              acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[j][t], b0[j], acc[t][0], 0, 0, 0);
              acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[j][t], b1[j], acc[t][1], 0, 0, 0);
            }
          }
        }
      }
    }
#pragma unroll
    for (int g0 = 0; g0 < MT; g0 += GT) {
      __syncthreads();      // the previous group's (chunk's) sums have been read
#pragma unroll
      for (int t = g0; t < g0 + GT && t < MT; ++t)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) red[wave][(((t - g0) * 2 + j) * 4 + i) * 64 + lane] = acc[t][j][i];
      __syncthreads();
#pragma unroll
      for (int t = g0; t < g0 + GT && t < MT; ++t)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int e = (((t - g0) * 2 + j) * 4 + wave) * 64 + lane;
          const int m = mb + t * 16 + q * 4 + wave, n = n0 + j * 16 + r;
          if (m < M && (j == 0 || two)) {
            const float v = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
            if (part)
              part[((size_t)z * M + m) * N + n] = v;
            else
              gemm_store(v, m, n, N, bias, epi, out, out_f16, aux);
          }
        }
    }
  }
}

__global__ void gemm_f16_reduce_kernel(const float* __restrict__ part, int KS, int M, int N, const half_t* __restrict__ bias, int epi, void* out,
                                       int out_f16, half_t* aux) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, MN = (int64_t)M * N;
  if (i >= MN) return;
  float v = part[i];
  for (int z = 1; z < KS; ++z) v += part[z * MN + i];
  gemm_store(v, (int)(i / N), (int)(i % N), N, bias, epi, out, out_f16, aux);
}

static int gemm_splits(int N, int K) {
  const int slabs = cdiv(N, 32), S = K / 32;
  int ks = 1;
  while (slabs * ks < 96 && ks < 8 && S >= ks * 2 * 4) ks *= 2;     // fill the chip, every wave of a slab keeps at least one step
  return ks;
}

// defer_ks != NULL: the raw sums go to ws as [ks][M][N] partials whatever ks is (1 included), *defer_ks = ks, and the caller's next kernel sums
// them in split order (the tower's residual GEMMs: vit_residual_ln_kernel adds bias and residual and normalises in the same pass)
static int gemm_launch(const half_t* A, const half_t* W, const half_t* bias, int M, int N, int K, int epi, void* out, int out_f16, float* ws,
                       int64_t ws_floats, hipStream_t st, int* defer_ks = nullptr, half_t* aux = nullptr) {
  VTS_CHECK_ARG(A && W && (out || defer_ks), "vts_gemm_f16: null pointer");
  VTS_CHECK_ARG(M >= 1 && N >= 1 && K >= 1, "vts_gemm_f16: bad shape M %d N %d K %d", M, N, K);
  VTS_CHECK_ARG(epi >= VTS_GEMM_NONE && epi <= VTS_GEMM_QUICKGELU_BWD && !(epi == VTS_GEMM_RESIDUAL && out_f16),
                "vts_gemm_f16: bad epilogue %d (out_f16 %d)", epi, out_f16);
  VTS_CHECK_ARG(epi == VTS_GEMM_QUICKGELU_BWD ? aux != nullptr : (aux == nullptr || epi == VTS_GEMM_QUICKGELU),
                "vts_gemm_f16: epilogue %d %s the [M][N] pre-activation buffer (vts_gemm_f16_aux)", epi, aux ? "does not take" : "needs");
  if (K % 32 || N % 16) {
    vts_set_error("vts_gemm_f16: K %d must be a multiple of 32 and N %d of 16", K, N);
    return VTS_ERR_UNSUPPORTED;
  }
  const int ks = gemm_splits(N, K);
  VTS_CHECK_ARG((ks == 1 && !defer_ks) || (ws && ws_floats >= (int64_t)ks * M * N), "vts_gemm_f16: workspace of %lld floats, needs %lld",
                (long long)ws_floats, (long long)ks * M * N);
  float* part = (ks > 1 || defer_ks) ? ws : nullptr;
  const dim3 grid(cdiv(N, 32), ks);
  const int mt = cdiv(M, 16);
#define VTS_GEMM_CASE(MT, UNR) \
  hipLaunchKernelGGL((gemm_f16_kernel<MT, UNR>), grid, dim3(256), 0, st, A, W, bias, M, N, K, epi, out, out_f16, part, ks, aux)
  if (mt <= 1) VTS_GEMM_CASE(1, 6);
  else if (mt <= 4) VTS_GEMM_CASE(4, 6);
  else if (mt <= 8) VTS_GEMM_CASE(8, 3);
  else if (mt <= 13) VTS_GEMM_CASE(13, 3);
  else VTS_GEMM_CASE(16, 2);
#undef VTS_GEMM_CASE
  VTS_CHECK_LAUNCH("vts_gemm_f16");
  if (defer_ks) {
    *defer_ks = ks;
    return VTS_OK;
  }
  if (ks > 1) {
    const int64_t MN = (int64_t)M * N;
    hipLaunchKernelGGL(gemm_f16_reduce_kernel, dim3((unsigned)cdiv64(MN, 256)), dim3(256), 0, st, ws, ks, M, N, bias, epi, out, out_f16, aux);
    VTS_CHECK_LAUNCH("vts_gemm_f16 (split reduce)");
  }
  return VTS_OK;
}

extern "C" int64_t vts_gemm_f16_ws_floats(int M, int N, int K) {
  if (M < 1 || N < 1 || K < 32 || K % 32 || N % 16) return 0;
  const int ks = gemm_splits(N, K);
  return ks > 1 ? (int64_t)ks * M * N : 0;
}

extern "C" int vts_gemm_f16(const uint16_t* A, const uint16_t* W, const uint16_t* bias, int M, int N, int K, int epilogue, void* out, int out_f16,
                            float* ws, int64_t ws_floats, void* stream) {
  return gemm_launch((const half_t*)A, (const half_t*)W, (const half_t*)bias, M, N, K, epilogue, out, out_f16, ws, ws_floats, (hipStream_t)stream);
}

extern "C" int vts_gemm_f16_aux(const uint16_t* A, const uint16_t* W, const uint16_t* bias, int M, int N, int K, int epilogue, void* out, int out_f16,
                                uint16_t* aux, float* ws, int64_t ws_floats, void* stream) {
  return gemm_launch((const half_t*)A, (const half_t*)W, (const half_t*)bias, M, N, K, epilogue, out, out_f16, ws, ws_floats, (hipStream_t)stream,
                     nullptr, (half_t*)aux);
}

// ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------
// one wave per row; mean, then the centred second moment (two passes over a row that the first pass left in cache), fp32 throughout.
// y may alias x when out_f16 == 0 and x_stride == D: a lane rewrites only the elements it alone reads.
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const float* x, int64_t x_stride, int rows, int D, const half_t* __restrict__ gamma,
                                                              const half_t* __restrict__ beta, float eps, void* y, int out_f16) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + (size_t)row * x_stride;
  // rows of up to 1024 values (every tower this file builds) live in registers: one trip to memory
  const bool in_regs = D <= 1024;
  float xv[16];
  float s = 0.f;
  if (in_regs) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int c = lane + 64 * j;
      xv[j] = c < D ? xr[c] : 0.f;
      s += xv[j];
    }
  } else {
    for (int c = lane; c < D; c += 64) s += xr[c];
  }
  const float mean = wave_sum(s) / (float)D;
  float v = 0.f;
  if (in_regs) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float d = lane + 64 * j < D ? xv[j] - mean : 0.f;
      v += d * d;
    }
  } else {
    for (int c = lane; c < D; c += 64) {
      const float d = xr[c] - mean;
      v += d * d;
    }
  }
  const float rstd = 1.f / sqrtf(wave_sum(v) / (float)D + eps);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (!in_regs) break;
    const int c = lane + 64 * j;
    if (c < D) {
      const float o = (xv[j] - mean) * rstd * (float)gamma[c] + (float)beta[c];
      if (out_f16)
        ((half_t*)y)[(size_t)row * D + c] = (half_t)o;
      else
        ((float*)y)[(size_t)row * D + c] = o;
    }
  }
  if (in_regs) return;
  for (int c = lane; c < D; c += 64) {
    const float o = (xr[c] - mean) * rstd * (float)gamma[c] + (float)beta[c];
    if (out_f16)
      ((half_t*)y)[(size_t)row * D + c] = (half_t)o;
    else
      ((float*)y)[(size_t)row * D + c] = o;
  }
}

static int layernorm_launch(const float* x, int64_t x_stride, int rows, int D, const half_t* gamma, const half_t* beta, float eps, void* y,
                            int out_f16, hipStream_t st) {
  VTS_CHECK_ARG(x && gamma && beta && y, "vts_layernorm_rows: null pointer");
  VTS_CHECK_ARG(rows >= 1 && D >= 1 && x_stride >= D, "vts_layernorm_rows: bad shape rows %d D %d stride %lld", rows, D, (long long)x_stride);
  hipLaunchKernelGGL(layernorm_rows_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, x, x_stride, rows, D, gamma, beta, eps, y, out_f16);
  VTS_CHECK_LAUNCH("vts_layernorm_rows");
  return VTS_OK;
}

extern "C" int vts_layernorm_rows(const float* x, int64_t x_stride, int rows, int D, const uint16_t* gamma, const uint16_t* beta, float eps, void* y,
                                  int out_f16, void* stream) {
  return layernorm_launch(x, x_stride, rows, D, (const half_t*)gamma, (const half_t*)beta, eps, y, out_f16, (hipStream_t)stream);
}

// Input gradient of the row LayerNorm (the tower is frozen: no gamma / beta gradients).  Statistics are recomputed from the saved fp32 row:
// xh = (x - mean) rstd, a = gamma dy, dx = rstd (a - mean(a) - xh mean(a xh)); accumulate != 0 adds into dx (the residual-gradient stream,
// row r at dx + r * dx_stride: ln_post's class-token rows are strided), and dx16 (may be NULL) receives the value dx then holds, in fp16,
// row r at r * D -- the next GEMM's A operand.  One wave per row; REGS: the row lives in registers (D <= 1024), else it is read per pass.
// dx may alias dy: a lane rewrites only the elements it alone reads.
template <bool REGS>
__global__ __launch_bounds__(256) void layernorm_rows_bwd_kernel(const float* dy, const float* x, int64_t x_stride, int rows, int D,
                                                                  const half_t* __restrict__ gamma, float eps, float* dx, int64_t dx_stride, int accumulate,
                                                                  half_t* dx16) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + (size_t)row * x_stride;
  const float* dyr = dy + (size_t)row * D;
  float* dxr = dx + (size_t)row * dx_stride;
  const int J = REGS ? 16 : (D + 63) / 64;
  float xv[REGS ? 16 : 1], av[REGS ? 16 : 1];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int c = lane + 64 * j;
    const float xc = c < D ? xr[c] : 0.f;
    if (REGS) {
      xv[j] = xc;
      av[j] = c < D ? (float)gamma[c] * dyr[c] : 0.f;
    }
    s += xc;
  }
  const float mean = wave_sum(s) / (float)D;
  float v = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int c = lane + 64 * j;
    const float d = c < D ? (REGS ? xv[j] : xr[c]) - mean : 0.f;
    v += d * d;
  }
  const float rstd = 1.f / sqrtf(wave_sum(v) / (float)D + eps);
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int c = lane + 64 * j;
    if (c < D) {
      const float a = REGS ? av[j] : (float)gamma[c] * dyr[c];
      s1 += a;
      s2 += a * (((REGS ? xv[j] : xr[c]) - mean) * rstd);
    }
  }
  const float m1 = wave_sum(s1) / (float)D, m2 = wave_sum(s2) / (float)D;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int c = lane + 64 * j;
    if (c < D) {
      const float a = REGS ? av[j] : (float)gamma[c] * dyr[c];
      float o = rstd * (a - m1 - ((REGS ? xv[j] : xr[c]) - mean) * rstd * m2);
      if (accumulate) o += dxr[c];
      dxr[c] = o;
      if (dx16) dx16[(size_t)row * D + c] = (half_t)o;
    }
  }
}

static int layernorm_bwd_launch(const float* dy, const float* x, int64_t x_stride, int rows, int D, const half_t* gamma, float eps, float* dx,
                                int64_t dx_stride, int accumulate, half_t* dx16, hipStream_t st) {
  VTS_CHECK_ARG(dy && x && gamma && dx, "vts_layernorm_rows_bwd: null pointer");
  VTS_CHECK_ARG(rows >= 1 && D >= 1 && x_stride >= D && dx_stride >= D, "vts_layernorm_rows_bwd: bad shape rows %d D %d strides %lld %lld", rows, D,
                (long long)x_stride, (long long)dx_stride);
  if (D <= 1024)
    hipLaunchKernelGGL(layernorm_rows_bwd_kernel<true>, dim3(cdiv(rows, 4)), dim3(256), 0, st, dy, x, x_stride, rows, D, gamma, eps, dx, dx_stride,
                       accumulate, dx16);
  else
    hipLaunchKernelGGL(layernorm_rows_bwd_kernel<false>, dim3(cdiv(rows, 4)), dim3(256), 0, st, dy, x, x_stride, rows, D, gamma, eps, dx, dx_stride,
                       accumulate, dx16);
  VTS_CHECK_LAUNCH("vts_layernorm_rows_bwd");
  return VTS_OK;
}

extern "C" int vts_layernorm_rows_bwd(const float* dy, const float* x, int64_t x_stride, int rows, int D, const uint16_t* gamma, float eps, float* dx,
                                      int64_t dx_stride, int accumulate, uint16_t* dx16, void* stream) {
  return layernorm_bwd_launch(dy, x, x_stride, rows, D, (const half_t*)gamma, eps, dx, dx_stride, accumulate, (half_t*)dx16, (hipStream_t)stream);
}

// ---- attention -------------------------------------------------------------------------------------------------------------------------
// One workgroup per (image, head), one wave per tile of 16 queries.  S = q k^T: 16x16 tiles over the key tiles, K = 64 in two MFMA steps, operands straight from the
// packed projection (rows past T read row T-1 and are masked / never stored).  Softmax in fp32 on the accumulator layout (a score row lives
// in the 16 lanes that share lane>>4: xor-shuffles 1, 2, 4, 8), P into LDS in the A layout's row-major form as TWO fp16 terms (the rounded
// value and the rounded remainder: P V then carries P to ~22 bits, so the fp32 softmax is not thrown away at the MFMA's input), V transposed
// into LDS so the B operand of P V (lane l: V[t = k + 8*(l>>4) .. +7][d = l&15]) is one 16-byte read.
#define VIT_LDP 72      // halfs per LDS row: 144 bytes keeps the 16-byte fragment reads aligned
__global__ __launch_bounds__(256) void vit_attention_kernel(const half_t* __restrict__ qkv, int T, int heads, float scale, half_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) half_t Ps[64 * VIT_LDP];
  __shared__ __attribute__((aligned(16))) half_t Pl[64 * VIT_LDP];
  __shared__ __attribute__((aligned(16))) half_t Vt[64 * VIT_LDP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int ld = 3 * heads * 64;
  const half_t* Q = qkv + (size_t)b * T * ld + h * 64;
  const half_t* Kp = Q + heads * 64;
  const half_t* V = Q + 2 * heads * 64;
  const int TT = (T + 15) >> 4;
  const int qt = wave;      // a wave owns one tile of 16 queries; all four transpose V
  // V^T into LDS: lane = token (zeros past T, so that P's zero columns never meet a non-finite value), wave = 16 of the 64 dimensions
  {
    h8 v0 = {0, 0, 0, 0, 0, 0, 0, 0}, v1 = v0;
    if (lane < T) {
      v0 = *(const h8*)(V + (size_t)lane * ld + wave * 16);
      v1 = *(const h8*)(V + (size_t)lane * ld + wave * 16 + 8);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      Vt[(wave * 16 + j) * VIT_LDP + lane] = v0[j];
      Vt[(wave * 16 + 8 + j) * VIT_LDP + lane] = v1[j];
    }
  }
  if (qt < TT) {
    f32x4 acc[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) acc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int tq = min(qt * 16 + r, T - 1);
    h8 qf[2], kf[2][4];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qf[ks] = *(const h8*)(Q + (size_t)tq * ld + ks * 32 + 8 * q);
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) kf[ks][kt] = *(const h8*)(Kp + (size_t)min(kt * 16 + r, T - 1) * ld + ks * 32 + 8 * q);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
        if (kt < TT) acc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qf[ks], kf[ks][kt], acc[kt], 0, 0, 0);
    // softmax over keys: element i of acc[kt] is score[query qt*16 + 4q + i][key kt*16 + r]
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s[4], mx = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        s[kt] = (kt * 16 + r < T) ? acc[kt][i] * scale : -INFINITY;
        mx = fmaxf(mx, s[kt]);
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      float sum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        s[kt] = expf(s[kt] - mx);      // key 0 is always live, so mx is finite; masked keys give exp(-inf) = 0
        sum += s[kt];
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) sum += __shfl_xor(sum, o, 64);
      const float inv = 1.f / sum;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const float pv = s[kt] * inv;
        const half_t hi = (half_t)pv;
        Ps[(qt * 16 + q * 4 + i) * VIT_LDP + kt * 16 + r] = hi;
        Pl[(qt * 16 + q * 4 + i) * VIT_LDP + kt * 16 + r] = (half_t)(pv - (float)hi);
      }
    }
  }
  __syncthreads();
  if (qt < TT) {
    const int steps = (T + 31) >> 5;
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < steps; ++ks) {
      const h8 pf = *(const h8*)(Ps + (qt * 16 + r) * VIT_LDP + ks * 32 + 8 * q);
      const h8 pl = *(const h8*)(Pl + (qt * 16 + r) * VIT_LDP + ks * 32 + 8 * q);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const h8 vf = *(const h8*)(Vt + (dt * 16 + r) * VIT_LDP + ks * 32 + 8 * q);
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pl, vf, o[dt], 0, 0, 0);
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pf, vf, o[dt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = qt * 16 + q * 4 + i;
        if (t < T) out[((size_t)b * T + t) * (heads * 64) + h * 64 + dt * 16 + r] = (half_t)o[dt][i];
      }
  }
}

static int attention_launch(const half_t* qkv, int B, int T, int heads, int head_dim, half_t* out, hipStream_t st) {
  VTS_CHECK_ARG(qkv && out, "vts_vit_attention: null pointer");
  VTS_CHECK_ARG(B >= 1 && heads >= 1, "vts_vit_attention: bad shape B %d heads %d", B, heads);
  if (head_dim != 64 || T < 1 || T > 64) {
    vts_set_error("vts_vit_attention: head dimension %d / T %d: only head dimension 64 and 1 <= T <= 64 are built (ViT-B/32 at 224^2)", head_dim, T);
    return VTS_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(vit_attention_kernel, dim3(B * heads), dim3(256), 0, st, qkv, T, heads, 0.125f, out);
  VTS_CHECK_LAUNCH("vts_vit_attention");
  return VTS_OK;
}

extern "C" int vts_vit_attention(const uint16_t* qkv, int B, int T, int heads, int head_dim, uint16_t* out, void* stream) {
  return attention_launch((const half_t*)qkv, B, T, heads, head_dim, (half_t*)out, (hipStream_t)stream);
}

// ---- attention backward ----------------------------------------------------------------------------------------------------------------
// One workgroup per (image, head), as the forward.  A wave recomputes the scores and P of its 16 queries exactly as the forward does, forms
// dP = dO V^T on the same accumulator layout (so dS = P o (dP - rowsum(dP o P)) needs only the softmax's own 16-lane row sums), and leaves P
// and dS in LDS, each as two fp16 terms (value and remainder, as the forward's P): P^T and dS^T for the products that reduce over the
// queries, dS for the one that reduces over the keys.  Rows of queries past T are written as zeros, so they add nothing to dK / dV.  The
// three output products then run tile by tile -- dV = P^T dO (wave = key tile), dQ = dS K / 8 (wave = query tile), dK = dS^T Q / 8 (wave =
// key tile) -- with their B operand (dO, K, Q transposed: Xt[d][token], zeros past T) staged through one LDS buffer in turn.
__device__ __forceinline__ void vit_stage_transposed(half_t* Xt, const half_t* X, int ld, int T, int lane, int wave) {
  h8 v0 = {0, 0, 0, 0, 0, 0, 0, 0}, v1 = v0;
  if (lane < T) {
    v0 = *(const h8*)(X + (size_t)lane * ld + wave * 16);
    v1 = *(const h8*)(X + (size_t)lane * ld + wave * 16 + 8);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    Xt[(wave * 16 + j) * VIT_LDP + lane] = v0[j];
    Xt[(wave * 16 + 8 + j) * VIT_LDP + lane] = v1[j];
  }
}

// out[tile*16 + ..][0 .. 63] = mul * (Ah + Al)[tile rows][0 .. T) Xt^T, rows past T not stored
__device__ __forceinline__ void vit_bwd_product(const half_t* Ah, const half_t* Al, const half_t* Xt, int tile, int T, int r, int q, float mul,
                                                half_t* out, int ld_out) {
  const int steps = (T + 31) >> 5;
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ks = 0; ks < steps; ++ks) {
    const h8 ah = *(const h8*)(Ah + (tile * 16 + r) * VIT_LDP + ks * 32 + 8 * q);
    const h8 al = *(const h8*)(Al + (tile * 16 + r) * VIT_LDP + ks * 32 + 8 * q);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const h8 xf = *(const h8*)(Xt + (dt * 16 + r) * VIT_LDP + ks * 32 + 8 * q);
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, xf, o[dt], 0, 0, 0);
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, xf, o[dt], 0, 0, 0);
    }
  }
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = tile * 16 + q * 4 + i;
      if (t < T) out[(size_t)t * ld_out + dt * 16 + r] = (half_t)(o[dt][i] * mul);
    }
}

__global__ __launch_bounds__(256) void vit_attention_bwd_kernel(const half_t* __restrict__ qkv, const half_t* __restrict__ dout, int T, int heads,
                                                                 float scale, half_t* __restrict__ dqkv) {
  __shared__ __attribute__((aligned(16))) half_t Pth[64 * VIT_LDP];       // P^T [key][query], value and remainder
  __shared__ __attribute__((aligned(16))) half_t Ptl[64 * VIT_LDP];
  __shared__ __attribute__((aligned(16))) half_t Sh[64 * VIT_LDP];        // dS [query][key]
  __shared__ __attribute__((aligned(16))) half_t Sl[64 * VIT_LDP];
  __shared__ __attribute__((aligned(16))) half_t Sth[64 * VIT_LDP];       // dS^T [key][query]
  __shared__ __attribute__((aligned(16))) half_t Stl[64 * VIT_LDP];
  __shared__ __attribute__((aligned(16))) half_t Xt[64 * VIT_LDP];        // dO^T, then K^T, then Q^T: [d][token]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int ld = 3 * heads * 64, ldo = heads * 64;
  const half_t* Q = qkv + (size_t)b * T * ld + h * 64;
  const half_t* Kp = Q + heads * 64;
  const half_t* V = Q + 2 * heads * 64;
  const half_t* dO = dout + (size_t)b * T * ldo + h * 64;
  half_t* dQ = dqkv + (size_t)b * T * ld + h * 64;
  const int TT = (T + 15) >> 4;
  const int qt = wave;
  vit_stage_transposed(Xt, dO, ldo, T, lane, wave);
  f32x4 p[4], ds[4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) p[kt] = ds[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (qt < TT) {
    f32x4 acc[4], dp[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) acc[kt] = dp[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int tq = min(qt * 16 + r, T - 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const h8 qf = *(const h8*)(Q + (size_t)tq * ld + ks * 32 + 8 * q);
      const h8 of = *(const h8*)(dO + (size_t)tq * ldo + ks * 32 + 8 * q);
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
        if (kt < TT) {
          const size_t tk = (size_t)min(kt * 16 + r, T - 1) * ld + ks * 32 + 8 * q;
          acc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qf, *(const h8*)(Kp + tk), acc[kt], 0, 0, 0);
          dp[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(of, *(const h8*)(V + tk), dp[kt], 0, 0, 0);
        }
    }
    // element i of acc[kt] / dp[kt] is [query qt*16 + 4q + i][key kt*16 + r]
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s[4], mx = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        s[kt] = (kt * 16 + r < T) ? acc[kt][i] * scale : -INFINITY;
        mx = fmaxf(mx, s[kt]);
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      float sum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        s[kt] = expf(s[kt] - mx);
        sum += s[kt];
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) sum += __shfl_xor(sum, o, 64);
      const float inv = 1.f / sum;
      float rs = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        s[kt] *= inv;
        rs += s[kt] * dp[kt][i];      // masked keys: P = 0 and dP finite (it was formed on key T-1's row)
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) rs += __shfl_xor(rs, o, 64);
      const bool live = qt * 16 + q * 4 + i < T;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        p[kt][i] = live ? s[kt] : 0.f;
        ds[kt][i] = live ? s[kt] * (dp[kt][i] - rs) : 0.f;
      }
    }
  }
  // every wave writes its 16 query rows (columns of the transposed forms) over all 64 keys: the arrays are whole, idle tiles are zeros
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = qt * 16 + q * 4 + i, col = kt * 16 + r;
      const float pv = p[kt][i], dv = ds[kt][i];
      const half_t ph = (half_t)pv, dh = (half_t)dv;
      const half_t pl = (half_t)(pv - (float)ph), dl = (half_t)(dv - (float)dh);
      Pth[col * VIT_LDP + row] = ph;
      Ptl[col * VIT_LDP + row] = pl;
      Sh[row * VIT_LDP + col] = dh;
      Sl[row * VIT_LDP + col] = dl;
      Sth[col * VIT_LDP + row] = dh;
      Stl[col * VIT_LDP + row] = dl;
    }
  __syncthreads();
  if (wave < TT) vit_bwd_product(Pth, Ptl, Xt, wave, T, r, q, 1.f, dQ + 2 * heads * 64, ld);      // dV
  __syncthreads();      // dO^T has been read
  vit_stage_transposed(Xt, Kp, ld, T, lane, wave);
  __syncthreads();
  if (wave < TT) vit_bwd_product(Sh, Sl, Xt, wave, T, r, q, scale, dQ, ld);                        // dQ
  __syncthreads();
  vit_stage_transposed(Xt, Q, ld, T, lane, wave);
  __syncthreads();
  if (wave < TT) vit_bwd_product(Sth, Stl, Xt, wave, T, r, q, scale, dQ + heads * 64, ld);         // dK
}

static int attention_bwd_launch(const half_t* qkv, const half_t* dout, int B, int T, int heads, int head_dim, half_t* dqkv, hipStream_t st) {
  VTS_CHECK_ARG(qkv && dout && dqkv, "vts_vit_attention_bwd: null pointer");
  VTS_CHECK_ARG(B >= 1 && heads >= 1, "vts_vit_attention_bwd: bad shape B %d heads %d", B, heads);
  if (head_dim != 64 || T < 1 || T > 64) {
    vts_set_error("vts_vit_attention_bwd: head dimension %d / T %d: only head dimension 64 and 1 <= T <= 64 are built (ViT-B/32 at 224^2)", head_dim, T);
    return VTS_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(vit_attention_bwd_kernel, dim3(B * heads), dim3(256), 0, st, qkv, dout, T, heads, 0.125f, dqkv);
  VTS_CHECK_LAUNCH("vts_vit_attention_bwd");
  return VTS_OK;
}

extern "C" int vts_vit_attention_bwd(const uint16_t* qkv, const uint16_t* dout, int B, int T, int heads, int head_dim, uint16_t* dqkv, void* stream) {
  return attention_bwd_launch((const half_t*)qkv, (const half_t*)dout, B, T, heads, head_dim, (half_t*)dqkv, (hipStream_t)stream);
}

// ---- pre-processing --------------------------------------------------------------------------------------------------------------------
// Pillow's ImagingResample (8 bits per channel): coefficients scaled by 2^22, accumulator started at 2^21, >> 22, clipped to a byte.
__device__ __forceinline__ int clip8(int ss) {
  ss >>= 22;
  return ss < 0 ? 0 : (ss > 255 ? 255 : ss);
}

__global__ void clip_resize_h_kernel(const float* __restrict__ x, int64_t rows, int W, const int* __restrict__ hb, const int* __restrict__ hk, int hks,
                                     uint8_t* __restrict__ tmp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * 224) return;
  const int j = (int)(i % 224);
  const float* xr = x + (i / 224) * W;
  int x0 = hb[2 * j], cnt = hb[2 * j + 1];
  x0 = min(max(x0, 0), W);
  cnt = max(0, min(cnt, min(hks, W - x0)));      // the tables come from the host: never read outside the row
  int ss = 1 << 21;
  for (int k = 0; k < cnt; ++k) {
    const int byte = ((int)(xr[x0 + k] * 255.f)) & 255;      // ToPILImage: mul(255).byte() -- truncation, then mod 256
    ss += byte * hk[j * hks + k];
  }
  tmp[i] = (uint8_t)clip8(ss);
}

__global__ void clip_resize_v_kernel(const uint8_t* __restrict__ tmp, int N, int H, const int* __restrict__ vb, const int* __restrict__ vk, int vks,
                                     const half_t* __restrict__ lut, half_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)N * 3 * 224 * 224) return;
  const int j = (int)(i % 224), y = (int)((i / 224) % 224);
  const int64_t nc = i / (224 * 224);
  int y0 = vb[2 * y], cnt = vb[2 * y + 1];
  y0 = min(max(y0, 0), H);
  cnt = max(0, min(cnt, min(vks, H - y0)));
  const uint8_t* col = tmp + (nc * H + y0) * 224 + j;
  int ss = 1 << 21;
  for (int k = 0; k < cnt; ++k) ss += (int)col[(int64_t)k * 224] * vk[y * vks + k];
  out[i] = lut[(int)(nc % 3) * 256 + clip8(ss)];
}

extern "C" int vts_clip_preprocess(const float* x, int N, int H, int W, const int* hb, const int* hk, int hks, const int* vb, const int* vk, int vks,
                                   const uint16_t* lut, uint8_t* tmp, uint16_t* out, void* stream) {
  VTS_CHECK_ARG(x && hb && hk && vb && vk && lut && tmp && out, "vts_clip_preprocess: null pointer");
  VTS_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && hks >= 1 && vks >= 1, "vts_clip_preprocess: bad shape N %d H %d W %d taps %d %d", N, H, W, hks, vks);
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)N * 3 * H;
  hipLaunchKernelGGL(clip_resize_h_kernel, dim3((unsigned)cdiv64(rows * 224, 256)), dim3(256), 0, st, x, rows, W, hb, hk, hks, tmp);
  VTS_CHECK_LAUNCH("vts_clip_preprocess (horizontal)");
  hipLaunchKernelGGL(clip_resize_v_kernel, dim3((unsigned)cdiv64((int64_t)N * 3 * 224 * 224, 256)), dim3(256), 0, st, tmp, N, H, vb, vk, vks,
                     (const half_t*)lut, (half_t*)out);
  VTS_CHECK_LAUNCH("vts_clip_preprocess (vertical)");
  return VTS_OK;
}

// The differentiable front end: (x * 0.5 + 0.5) -> adaptive average pooling to res x res with F.interpolate(mode='area')'s windows
// (rows floor(i H / res) .. ceil((i + 1) H / res), any H, W: windows overlap when upscaling) -> (v - mean_c) / std_c.
__constant__ float clip_mean_c[3] = {0.48145466f, 0.4578275f, 0.40821073f};
__constant__ float clip_std_c[3] = {0.26862954f, 0.26130258f, 0.27577711f};
__device__ __forceinline__ int area_lo(int i, int S, int res) { return (int)(((int64_t)i * S) / res); }
__device__ __forceinline__ int area_hi(int i, int S, int res) { return (int)(((int64_t)(i + 1) * S + res - 1) / res); }

__global__ void clip_area_kernel(const float* __restrict__ x, int N, int H, int W, int res, void* out, int out_f16) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)N * 3 * res * res) return;
  const int ox = (int)(i % res), oy = (int)((i / res) % res);
  const int64_t nc = i / ((int64_t)res * res);
  const int y0 = area_lo(oy, H, res), y1 = area_hi(oy, H, res), x0 = area_lo(ox, W, res), x1 = area_hi(ox, W, res);
  const float* xp = x + nc * H * W;
  float s = 0.f;
  for (int y = y0; y < y1; ++y)
    for (int xx = x0; xx < x1; ++xx) s += xp[(int64_t)y * W + xx];
  const int c = (int)(nc % 3);
  const float v = (s / (float)((y1 - y0) * (x1 - x0)) * 0.5f + 0.5f - clip_mean_c[c]) / clip_std_c[c];
  if (out_f16)
    ((half_t*)out)[i] = (half_t)v;
  else
    ((float*)out)[i] = v;
}

// gather form: an input pixel sums the output cells whose window holds it (rows floor(y res / H) .. ceil((y + 1) res / H) - 1 are the
// candidates; each is tested against its own window), each divided by its window's area; no atomics
__global__ void clip_area_bwd_kernel(const float* __restrict__ dy, int N, int H, int W, int res, float* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)N * 3 * H * W) return;
  const int xx = (int)(i % W), y = (int)((i / W) % H);
  const int64_t nc = i / ((int64_t)H * W);
  const int oy0 = max(area_lo(y, res, H) - 1, 0), oy1 = min(area_hi(y, res, H) + 1, res);
  const int ox0 = max(area_lo(xx, res, W) - 1, 0), ox1 = min(area_hi(xx, res, W) + 1, res);
  const float* dp = dy + nc * res * res;
  float s = 0.f;
  for (int oy = oy0; oy < oy1; ++oy) {
    const int y0 = area_lo(oy, H, res), y1 = area_hi(oy, H, res);
    if (y < y0 || y >= y1) continue;
    for (int ox = ox0; ox < ox1; ++ox) {
      const int x0 = area_lo(ox, W, res), x1 = area_hi(ox, W, res);
      if (xx >= x0 && xx < x1) s += dp[oy * res + ox] / (float)((y1 - y0) * (x1 - x0));
    }
  }
  dx[i] = s * 0.5f / clip_std_c[(int)(nc % 3)];
}

extern "C" int vts_clip_area_preprocess(const float* x, int N, int H, int W, int res, void* out, int out_f16, void* stream) {
  VTS_CHECK_ARG(x && out, "vts_clip_area_preprocess: null pointer");
  VTS_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && res >= 1 && res <= 4096 && H <= 32768 && W <= 32768, "vts_clip_area_preprocess: bad shape N %d H %d W %d res %d", N,
                H, W, res);
  hipLaunchKernelGGL(clip_area_kernel, dim3((unsigned)cdiv64((int64_t)N * 3 * res * res, 256)), dim3(256), 0, (hipStream_t)stream, x, N, H, W, res, out,
                     out_f16);
  VTS_CHECK_LAUNCH("vts_clip_area_preprocess");
  return VTS_OK;
}

extern "C" int vts_clip_area_preprocess_bwd(const float* dy, int N, int H, int W, int res, float* dx, void* stream) {
  VTS_CHECK_ARG(dy && dx, "vts_clip_area_preprocess_bwd: null pointer");
  VTS_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && res >= 1 && res <= 4096 && H <= 32768 && W <= 32768, "vts_clip_area_preprocess_bwd: bad shape N %d H %d W %d res %d",
                N, H, W, res);
  hipLaunchKernelGGL(clip_area_bwd_kernel, dim3((unsigned)cdiv64((int64_t)N * 3 * H * W, 256)), dim3(256), 0, (hipStream_t)stream, dy, N, H, W, res, dx);
  VTS_CHECK_LAUNCH("vts_clip_area_preprocess_bwd");
  return VTS_OK;
}

// ---- the tower -------------------------------------------------------------------------------------------------------------------------
// conv1 with kernel = stride = patch is a GEMM over the gathered patches: row (n, gy, gx), column (c, py, px) -- conv1.weight's own order.
__global__ void vit_patch_gather_kernel(const half_t* __restrict__ x, int N, int R, int P, half_t* __restrict__ rows) {
  const int G = R / P, Kp = 3 * P * P;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)N * G * G * Kp) return;
  const int k = (int)(i % Kp);
  const int64_t row = i / Kp;
  const int gx = (int)(row % G), gy = (int)((row / G) % G), n = (int)(row / (G * G));
  const int px = k % P, py = (k / P) % P, c = k / (P * P);
  rows[i] = x[(((size_t)n * 3 + c) * R + gy * P + py) * R + gx * P + px];
}

// x[n][0] = class_embedding + pos[0];  x[n][1 + g] = tokens[n][g] + pos[1 + g]
__global__ void vit_embed_kernel(const float* __restrict__ tok, const half_t* __restrict__ cls, const half_t* __restrict__ pos, int N, int T, int Wd,
                                 float* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)N * T * Wd) return;
  const int c = (int)(i % Wd), t = (int)((i / Wd) % T), n = (int)(i / ((int64_t)Wd * T));
  const float v = t == 0 ? (float)cls[c] : tok[((size_t)n * (T - 1) + t - 1) * Wd + c];
  x[i] = v + (float)pos[(size_t)t * Wd + c];
}

// The tower's residual GEMMs (out_proj, c_proj) leave [KS][M][D] partial sums; this kernel finishes them and runs the LayerNorm that
// follows in the same pass: xo[m] = x[m] + bias + sum_z part[z][m] (split order), then h[m] = LayerNorm(xo[m]) in fp16 (gamma NULL: no
// LayerNorm -- the last block, whose successor ln_post reads the class tokens only).  xo is x itself, or the tape's next slot (a lane
// rewrites only the elements it alone reads).  One wave per row, the row in registers (D <= 1024).
__global__ __launch_bounds__(256) void vit_residual_ln_kernel(const float* __restrict__ part, int KS, int M, int D, const half_t* __restrict__ bias,
                                                               const float* x, float* xo, const half_t* __restrict__ gamma,
                                                               const half_t* __restrict__ beta, float eps, half_t* __restrict__ h) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const size_t MD = (size_t)M * D, base = (size_t)row * D;
  // every load of a phase is issued before the first use: the row's 12 .. 16 values per lane travel together
  float xv[16], pv[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) pv[j] = lane + 64 * j < D ? part[base + lane + 64 * j] : 0.f;
  for (int z = 1; z < KS; ++z) {
    float t[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) t[j] = lane + 64 * j < D ? part[z * MD + base + lane + 64 * j] : 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) pv[j] += t[j];
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int c = lane + 64 * j;
    xv[j] = c < D ? x[base + c] : 0.f;
    pv[j] += c < D ? (float)bias[c] : 0.f;
  }
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    xv[j] += pv[j];
    s += xv[j];
  }
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (lane + 64 * j < D) xo[base + lane + 64 * j] = xv[j];
  if (!gamma) return;
  const float mean = wave_sum(s) / (float)D;
  float v = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float d = lane + 64 * j < D ? xv[j] - mean : 0.f;
    v += d * d;
  }
  const float rstd = 1.f / sqrtf(wave_sum(v) / (float)D + eps);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int c = lane + 64 * j;
    if (c < D) h[base + c] = (half_t)((xv[j] - mean) * rstd * (float)gamma[c] + (float)beta[c]);
  }
}

static int residual_ln_launch(const float* part, int ks, int M, int D, const half_t* bias, const float* x, float* xo, const half_t* gamma,
                              const half_t* beta, float eps, half_t* h, hipStream_t st) {
  hipLaunchKernelGGL(vit_residual_ln_kernel, dim3(cdiv(M, 4)), dim3(256), 0, st, part, ks, M, D, bias, x, xo, gamma, beta, eps, h);
  VTS_CHECK_LAUNCH("vts_clip_visual_forward (residual + LayerNorm)");
  return VTS_OK;
}

struct vit_plan {
  int T, G, Kp, M;
  int64_t ws_floats;
  // offsets into ws, in floats (every segment starts on a 16-byte boundary)
  int64_t patches, tok, x, h, qkv, att, mlp, cls, part, part_floats;
};

static inline int64_t up4(int64_t v) { return (v + 3) & ~(int64_t)3; }

static int vit_make_plan(const vts_clip_visual_cfg* c, int N, vit_plan* p) {
  VTS_CHECK_ARG(c, "vts_clip_visual_forward: null config");
  VTS_CHECK_ARG(N >= 1 && c->width >= 1 && c->layers >= 0 && c->heads >= 1 && c->patch >= 1 && c->resolution >= 1 && c->output_dim >= 1,
                "vts_clip_visual_forward: bad config (N %d width %d layers %d heads %d patch %d resolution %d output_dim %d)", N, c->width, c->layers,
                c->heads, c->patch, c->resolution, c->output_dim);
  const int Wd = c->width;
  const int G = c->resolution / c->patch, T = G * G + 1, Kp = 3 * c->patch * c->patch;
  if (Wd != 64 * c->heads || T > 64 || c->resolution % c->patch || Wd % 32 || Wd > 1024 || c->output_dim % 16 || Kp % 32) {
    vts_set_error("vts_clip_visual_forward: width %d heads %d patch %d resolution %d output_dim %d: built for head dimension 64, at most 64 tokens, "
                  "width %% 32 == 0, output_dim %% 16 == 0, width <= 1024 (ViT-B/32 at 224^2); the other CLIP towers are out of scope",
                  Wd, c->heads, c->patch, c->resolution, c->output_dim);
    return VTS_ERR_UNSUPPORTED;
  }
  p->T = T, p->G = G, p->Kp = Kp, p->M = N * T;
  const int64_t M = p->M, R = (int64_t)N * G * G;
  int64_t o = 0;
  p->patches = o, o += up4((R * Kp + 1) / 2);
  p->tok = o, o += up4(R * Wd);
  p->x = o, o += up4(M * Wd);
  p->h = o, o += up4((M * Wd + 1) / 2);
  p->qkv = o, o += up4((M * 3 * Wd + 1) / 2);
  p->att = o, o += up4((M * Wd + 1) / 2);
  p->mlp = o, o += up4((M * 4 * Wd + 1) / 2);
  p->cls = o, o += up4(((int64_t)N * Wd + 1) / 2);
  int64_t pf = vts_gemm_f16_ws_floats((int)R, Wd, Kp);
  const int64_t shapes[5][3] = {{M, 3 * Wd, Wd}, {M, Wd, Wd}, {M, 4 * Wd, Wd}, {M, Wd, 4 * Wd}, {N, c->output_dim, Wd}};
  for (int i = 0; i < 5; ++i) {
    const int64_t f = vts_gemm_f16_ws_floats((int)shapes[i][0], (int)shapes[i][1], (int)shapes[i][2]);
    pf = f > pf ? f : pf;
  }
  // the residual GEMMs always leave partials (ks >= 1): out_proj, c_proj
  const int64_t fo = (int64_t)gemm_splits(Wd, Wd) * M * Wd, fp = (int64_t)gemm_splits(Wd, 4 * Wd) * M * Wd;
  pf = fo > pf ? fo : pf;
  pf = fp > pf ? fp : pf;
  p->part = o, p->part_floats = pf, o += up4(pf);
  p->ws_floats = o;
  return VTS_OK;
}

extern "C" int64_t vts_clip_visual_weight_halfs(const vts_clip_visual_cfg* c) {
  vit_plan p;
  if (vit_make_plan(c, 1, &p) != VTS_OK) return -1;
  const int64_t Wd = c->width;
  return Wd * p.Kp + Wd + (int64_t)p.T * Wd + 2 * Wd + c->layers * (12 * Wd * Wd + 13 * Wd) + 2 * Wd + (int64_t)c->output_dim * Wd;
}

extern "C" int64_t vts_clip_visual_forward_ws_floats(const vts_clip_visual_cfg* c, int N) {
  vit_plan p;
  if (vit_make_plan(c, N, &p) != VTS_OK) return -1;
  return p.ws_floats;
}

// The tape of vts_clip_visual_forward_tape (offsets in floats; include/vts.h documents the layout): the residual stream after ln_pre and
// after every block, the stream before ln_pre, and per block the stream between its two halves, the packed qkv and c_fc's pre-activation.
struct vit_tape {
  int64_t xs, emb, layer0, layer_stride, mid, qkv, fc, floats;
};

static void vit_tape_plan(const vts_clip_visual_cfg* c, const vit_plan* p, vit_tape* t) {
  const int64_t MW = (int64_t)p->M * c->width;      // width % 32 == 0: every segment below is a multiple of 4 floats
  t->xs = 0;
  t->emb = (c->layers + 1) * MW;
  t->layer0 = t->emb + MW;
  t->mid = 0;
  t->qkv = MW;
  t->fc = t->qkv + 3 * MW / 2;
  t->layer_stride = t->fc + 4 * MW / 2;
  t->floats = t->layer0 + c->layers * t->layer_stride;
}

extern "C" int64_t vts_clip_visual_tape_floats(const vts_clip_visual_cfg* c, int N) {
  vit_plan p;
  vit_tape t;
  if (vit_make_plan(c, N, &p) != VTS_OK) return -1;
  vit_tape_plan(c, &p, &t);
  return t.floats;
}

// tape == NULL: the stream is updated in place in ws and nothing else is kept.  Otherwise every state of the stream goes to its slot of the
// tape, qkv is written there instead of ws, and c_fc's epilogue leaves its pre-activation there; the arithmetic is the same either way.
static int vit_forward(const vts_clip_visual_cfg* c, const uint16_t* w_, const uint16_t* x_, int N, float* out, float* ws, int64_t ws_floats,
                       float* tape, int64_t tape_floats, void* stream) {
  vit_plan p;
  vit_tape tp;
  int rc = vit_make_plan(c, N, &p);
  if (rc != VTS_OK) return rc;
  VTS_CHECK_ARG(w_ && x_ && out && ws, "vts_clip_visual_forward: null pointer");
  VTS_CHECK_ARG(ws_floats >= p.ws_floats, "vts_clip_visual_forward: workspace of %lld floats, needs %lld", (long long)ws_floats, (long long)p.ws_floats);
  VTS_CHECK_ARG(((uintptr_t)ws & 15) == 0 && ((uintptr_t)w_ & 15) == 0, "vts_clip_visual_forward: ws and w must be 16-byte aligned");
  vit_tape_plan(c, &p, &tp);
  VTS_CHECK_ARG(!tape || (tape_floats >= tp.floats && ((uintptr_t)tape & 15) == 0), "vts_clip_visual_forward_tape: tape of %lld floats, needs %lld, 16-byte aligned",
                (long long)tape_floats, (long long)tp.floats);
  hipStream_t st = (hipStream_t)stream;
  const int Wd = c->width, T = p.T, M = p.M, R = N * p.G * p.G;
  const float eps = 1e-5f;
  const half_t* w = (const half_t*)w_;
  half_t* patches = (half_t*)(ws + p.patches);
  float* tok = ws + p.tok;
  const int64_t MW = (int64_t)p.M * c->width;
  float* x = tape ? tape + tp.emb : ws + p.x;      // the stream's current state; with a tape it moves from slot to slot
  half_t* h = (half_t*)(ws + p.h);
  half_t* qkv = (half_t*)(ws + p.qkv);
  half_t* att = (half_t*)(ws + p.att);
  half_t* mlp = (half_t*)(ws + p.mlp);
  half_t* cls = (half_t*)(ws + p.cls);
  float* part = ws + p.part;
  // the weight buffer's segments, in the order include/vts.h documents
  const half_t* conv1 = w;
  w += (size_t)Wd * p.Kp;
  const half_t* cls_emb = w;
  w += Wd;
  const half_t* pos = w;
  w += (size_t)T * Wd;
  const half_t* ln_pre_w = w;
  const half_t* ln_pre_b = w + Wd;
  w += 2 * Wd;

  const int64_t ng = (int64_t)R * p.Kp;
  hipLaunchKernelGGL(vit_patch_gather_kernel, dim3((unsigned)cdiv64(ng, 256)), dim3(256), 0, st, (const half_t*)x_, N, c->resolution, c->patch, patches);
  VTS_CHECK_LAUNCH("vts_clip_visual_forward (patch gather)");
  if ((rc = gemm_launch(patches, conv1, nullptr, R, Wd, p.Kp, VTS_GEMM_NONE, tok, 0, part, p.part_floats, st)) != VTS_OK) return rc;
  hipLaunchKernelGGL(vit_embed_kernel, dim3((unsigned)cdiv64((int64_t)M * Wd, 256)), dim3(256), 0, st, tok, cls_emb, pos, N, T, Wd, x);
  VTS_CHECK_LAUNCH("vts_clip_visual_forward (embedding)");
  float* x0 = tape ? tape + tp.xs : x;
  if ((rc = layernorm_launch(x, Wd, M, Wd, ln_pre_w, ln_pre_b, eps, x0, 0, st)) != VTS_OK) return rc;
  x = x0;
  for (int l = 0; l < c->layers; ++l) {
    const half_t* ln1_w = w;
    const half_t* ln1_b = w + Wd;
    w += 2 * Wd;
    const half_t* in_w = w;
    w += (size_t)3 * Wd * Wd;
    const half_t* in_b = w;
    w += 3 * Wd;
    const half_t* out_w = w;
    w += (size_t)Wd * Wd;
    const half_t* out_b = w;
    w += Wd;
    const half_t* ln2_w = w;
    const half_t* ln2_b = w + Wd;
    w += 2 * Wd;
    const half_t* fc_w = w;
    w += (size_t)4 * Wd * Wd;
    const half_t* fc_b = w;
    w += 4 * Wd;
    const half_t* pj_w = w;
    w += (size_t)4 * Wd * Wd;
    const half_t* pj_b = w;
    w += Wd;
    int ks = 1;
    float* lt = tape ? tape + tp.layer0 + l * tp.layer_stride : nullptr;
    float* xmid = tape ? lt + tp.mid : x;
    float* xnext = tape ? tape + tp.xs + (l + 1) * MW : x;
    half_t* fc_pre = tape ? (half_t*)(lt + tp.fc) : nullptr;
    if (tape) qkv = (half_t*)(lt + tp.qkv);
    // (ln_1 of every block but the first ran fused with the previous block's c_proj)
    if (l == 0 && (rc = layernorm_launch(x, Wd, M, Wd, ln1_w, ln1_b, eps, h, 1, st)) != VTS_OK) return rc;
    if ((rc = gemm_launch(h, in_w, in_b, M, 3 * Wd, Wd, VTS_GEMM_NONE, qkv, 1, part, p.part_floats, st)) != VTS_OK) return rc;
    if ((rc = attention_launch(qkv, N, T, c->heads, 64, att, st)) != VTS_OK) return rc;
    if ((rc = gemm_launch(att, out_w, nullptr, M, Wd, Wd, VTS_GEMM_NONE, nullptr, 0, part, p.part_floats, st, &ks)) != VTS_OK) return rc;
    if ((rc = residual_ln_launch(part, ks, M, Wd, out_b, x, xmid, ln2_w, ln2_b, eps, h, st)) != VTS_OK) return rc;
    if ((rc = gemm_launch(h, fc_w, fc_b, M, 4 * Wd, Wd, VTS_GEMM_QUICKGELU, mlp, 1, part, p.part_floats, st, nullptr, fc_pre)) != VTS_OK) return rc;
    if ((rc = gemm_launch(mlp, pj_w, nullptr, M, Wd, 4 * Wd, VTS_GEMM_NONE, nullptr, 0, part, p.part_floats, st, &ks)) != VTS_OK) return rc;
    // the next block's ln_1 parameters are the next two segments of the buffer
    const bool last = l + 1 == c->layers;
    if ((rc = residual_ln_launch(part, ks, M, Wd, pj_b, xmid, xnext, last ? nullptr : w, last ? nullptr : w + Wd, eps, h, st)) != VTS_OK) return rc;
    x = xnext;
  }
  const half_t* ln_post_w = w;
  const half_t* ln_post_b = w + Wd;
  w += 2 * Wd;
  const half_t* projT = w;
  // ln_post on the class token of each image (row n*T of x), then @ proj
  if ((rc = layernorm_launch(x, (int64_t)T * Wd, N, Wd, ln_post_w, ln_post_b, eps, cls, 1, st)) != VTS_OK) return rc;
  return gemm_launch(cls, projT, nullptr, N, c->output_dim, Wd, VTS_GEMM_NONE, out, 0, part, p.part_floats, st);
}

extern "C" int vts_clip_visual_forward(const vts_clip_visual_cfg* c, const uint16_t* w, const uint16_t* x, int N, float* out, float* ws, int64_t ws_floats,
                                       void* stream) {
  return vit_forward(c, w, x, N, out, ws, ws_floats, nullptr, 0, stream);
}

extern "C" int vts_clip_visual_forward_tape(const vts_clip_visual_cfg* c, const uint16_t* w, const uint16_t* x, int N, float* out, float* ws,
                                            int64_t ws_floats, float* tape, int64_t tape_floats, void* stream) {
  VTS_CHECK_ARG(tape, "vts_clip_visual_forward_tape: null tape");
  return vit_forward(c, w, x, N, out, ws, ws_floats, tape, tape_floats, stream);
}

// ---- the tower's input-gradient backward ---------------------------------------------------------------------------------------------------
// The backward is linear in its cotangents and its GEMM operands are fp16, so the cotangents are normalised on the way in by a power of two
// found on the device (their largest magnitude goes to [1, 2)) and the factor is undone at dx: GAN-loss gradients of any size keep fp16's
// full precision and a scaled cotangent gives the scaled result to the bit.  sc[0] = the factor, sc[1] = its inverse, sc[4 ..] = partial maxima.
#define VIT_AMAX_BLOCKS 64
__global__ __launch_bounds__(256) void vit_absmax_kernel(const float* __restrict__ a, int64_t na, const float* __restrict__ b, int64_t nb,
                                                          float* __restrict__ sc) {
  __shared__ float red[4];
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < na + nb; i += (int64_t)VIT_AMAX_BLOCKS * 256)
    m = fmaxf(m, fabsf(i < na ? a[i] : b[i - na]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) sc[4 + blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(64) void vit_scale_kernel(float* __restrict__ sc) {
  float m = sc[4 + threadIdx.x];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (threadIdx.x == 0) {
    int e = 1;
    if (m > 0.f && m <= 3.0e38f) frexpf(m, &e);      // m = f 2^e, f in [0.5, 1); all-zero or non-finite cotangents: factor 1
    e = e > 120 ? 120 : (e < -120 ? -120 : e);
    sc[0] = ldexpf(1.f, 1 - e);
    sc[1] = ldexpf(1.f, e - 1);
  }
}

// g = (init ? 0 : g) + sc[0] * add (add NULL: nothing added); g16 (may be NULL) = fp16(g)
__global__ void vit_cotangent_kernel(float* __restrict__ g, const float* __restrict__ add, const float* __restrict__ sc, int init,
                                     half_t* __restrict__ g16, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = init ? 0.f : g[i];
  if (add) v += sc[0] * add[i];
  g[i] = v;
  if (g16) g16[i] = (half_t)v;
}

// d_out [N][od] -> fp16 [N][odp], scaled, the K padding of the proj GEMM zeroed
__global__ void vit_dout_half_kernel(const float* __restrict__ d, int N, int od, int odp, const float* __restrict__ sc, half_t* __restrict__ o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * odp) return;
  const int c = i % odp, n = i / odp;
  o[i] = c < od ? (half_t)(sc[0] * d[(size_t)n * od + c]) : (half_t)0.f;
}

// the token rows of d[N][T][W] (the class-token row dropped) as fp16 [N*(T-1)][W]
__global__ void vit_drop_cls_kernel(const float* __restrict__ d, int N, int T, int Wd, half_t* __restrict__ o) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)N * (T - 1) * Wd) return;
  const int c = (int)(i % Wd);
  const int64_t row = i / Wd;
  const int64_t n = row / (T - 1), t = row % (T - 1) + 1;
  o[i] = (half_t)d[((size_t)n * T + t) * Wd + c];
}

// the adjoint of vit_patch_gather_kernel: patches do not overlap, so every dx element is written once; the cotangent factor is undone here
__global__ void vit_patch_scatter_kernel(const float* __restrict__ rows, int N, int R, int P, const float* __restrict__ sc, float* __restrict__ dx) {
  const int G = R / P, Kp = 3 * P * P;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)N * G * G * Kp) return;
  const int k = (int)(i % Kp);
  const int64_t row = i / Kp;
  const int gx = (int)(row % G), gy = (int)((row / G) % G), n = (int)(row / (G * G));
  const int px = k % P, py = (k / P) % P, c = k / (P * P);
  dx[(((size_t)n * 3 + c) * R + gy * P + py) * R + gx * P + px] = rows[i] * sc[1];
}

struct vit_bwd_plan {
  int odp;
  int64_t sc, g, dh, g16, dmlp, datt, dqkv, dout, dcls, dtok, dpatch, part, part_floats, ws_floats;
};

static void vit_make_bwd_plan(const vts_clip_visual_cfg* c, int N, const vit_plan* p, vit_bwd_plan* b) {
  const int64_t Wd = c->width, M = p->M, R = (int64_t)N * p->G * p->G, MW = M * Wd;
  b->odp = (c->output_dim + 31) & ~31;
  int64_t o = 0;
  b->sc = o, o += up4(4 + VIT_AMAX_BLOCKS);
  b->g = o, o += MW;
  b->dh = o, o += MW;
  b->g16 = o, o += MW / 2;
  b->dmlp = o, o += 4 * MW / 2;
  b->datt = o, o += MW / 2;
  b->dqkv = o, o += 3 * MW / 2;
  b->dout = o, o += up4(((int64_t)N * b->odp + 1) / 2);
  b->dcls = o, o += up4((int64_t)N * Wd);
  b->dtok = o, o += up4((R * Wd + 1) / 2);
  b->dpatch = o, o += up4(R * p->Kp);
  // every product as the GEMM sees it: {rows, output features, reduction length}
  const int64_t shapes[6][3] = {{N, Wd, b->odp}, {M, 4 * Wd, Wd}, {M, Wd, 4 * Wd}, {M, Wd, Wd}, {M, Wd, 3 * Wd}, {R, p->Kp, Wd}};
  int64_t pf = 0;
  for (int i = 0; i < 6; ++i) {
    const int64_t f = vts_gemm_f16_ws_floats((int)shapes[i][0], (int)shapes[i][1], (int)shapes[i][2]);
    pf = f > pf ? f : pf;
  }
  b->part = o, b->part_floats = pf, o += up4(pf);
  b->ws_floats = o;
}

extern "C" int64_t vts_clip_visual_weight_t_halfs(const vts_clip_visual_cfg* c) {
  vit_plan p;
  if (vit_make_plan(c, 1, &p) != VTS_OK) return -1;
  const int64_t Wd = c->width;
  return p.Kp * Wd + c->layers * 12 * Wd * Wd + Wd * ((c->output_dim + 31) & ~31);
}

extern "C" int64_t vts_clip_visual_backward_ws_floats(const vts_clip_visual_cfg* c, int N) {
  vit_plan p;
  vit_bwd_plan b;
  if (vit_make_plan(c, N, &p) != VTS_OK) return -1;
  vit_make_bwd_plan(c, N, &p, &b);
  return b.ws_floats;
}

extern "C" int vts_clip_visual_backward(const vts_clip_visual_cfg* c, const uint16_t* w_, const uint16_t* wt_, const float* tape, int64_t tape_floats,
                                        int N, const float* d_out, const int* taps, int n_taps, const float* d_hidden, float* dx, float* ws,
                                        int64_t ws_floats, void* stream) {
  vit_plan p;
  vit_tape tp;
  vit_bwd_plan bp;
  int rc = vit_make_plan(c, N, &p);
  if (rc != VTS_OK) return rc;
  vit_tape_plan(c, &p, &tp);
  vit_make_bwd_plan(c, N, &p, &bp);
  VTS_CHECK_ARG(w_ && wt_ && tape && dx && ws, "vts_clip_visual_backward: null pointer");
  VTS_CHECK_ARG(n_taps >= 0 && n_taps <= c->layers + 1 && (n_taps == 0 || (taps && d_hidden)), "vts_clip_visual_backward: %d taps (0 .. %d, with their arrays)",
                n_taps, c->layers + 1);
  VTS_CHECK_ARG(d_out || n_taps > 0, "vts_clip_visual_backward: no cotangent: neither d_out nor a tapped hidden state");
  for (int i = 0; i < n_taps; ++i)
    VTS_CHECK_ARG(taps[i] >= 0 && taps[i] <= c->layers && (i == 0 || taps[i] > taps[i - 1]),
                  "vts_clip_visual_backward: tap %d is tape index %d: indices must ascend within 0 .. %d", i, taps[i], c->layers);
  VTS_CHECK_ARG(tape_floats >= tp.floats, "vts_clip_visual_backward: tape of %lld floats, needs %lld", (long long)tape_floats, (long long)tp.floats);
  VTS_CHECK_ARG(ws_floats >= bp.ws_floats, "vts_clip_visual_backward: workspace of %lld floats, needs %lld", (long long)ws_floats, (long long)bp.ws_floats);
  VTS_CHECK_ARG(((uintptr_t)ws & 15) == 0 && ((uintptr_t)w_ & 15) == 0 && ((uintptr_t)wt_ & 15) == 0 && ((uintptr_t)tape & 15) == 0,
                "vts_clip_visual_backward: ws, w, wt and tape must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int Wd = c->width, T = p.T, M = p.M, R = N * p.G * p.G, L = c->layers;
  const int64_t MW = (int64_t)M * Wd, W2 = (int64_t)Wd * Wd;
  const float eps = 1e-5f;
  const half_t* w = (const half_t*)w_;
  const half_t* wt = (const half_t*)wt_;
  float* sc = ws + bp.sc;
  float* g = ws + bp.g;
  float* dh = ws + bp.dh;
  half_t* g16 = (half_t*)(ws + bp.g16);
  half_t* dmlp = (half_t*)(ws + bp.dmlp);
  half_t* datt = (half_t*)(ws + bp.datt);
  half_t* dqkv = (half_t*)(ws + bp.dqkv);
  half_t* dout16 = (half_t*)(ws + bp.dout);
  float* dcls = ws + bp.dcls;
  half_t* dtok = (half_t*)(ws + bp.dtok);
  float* dpatch = ws + bp.dpatch;
  float* part = ws + bp.part;
  // the forward buffer's LayerNorm gains (include/vts.h layout) and the transposed buffer's matrices
  const half_t* ln_pre_w = w + (size_t)Wd * p.Kp + Wd + (size_t)T * Wd;
  const half_t* layers_w = ln_pre_w + 2 * Wd;
  const size_t layer_halfs = 12 * (size_t)W2 + 13 * (size_t)Wd;
  const half_t* ln_post_w = layers_w + L * layer_halfs;
  const half_t* conv1T = wt;
  const half_t* layers_t = wt + (size_t)p.Kp * Wd;
  const half_t* projB = layers_t + (size_t)L * 12 * W2;
  const unsigned mw_blocks = (unsigned)cdiv64(MW, 256);

  hipLaunchKernelGGL(vit_absmax_kernel, dim3(VIT_AMAX_BLOCKS), dim3(256), 0, st, d_out, d_out ? (int64_t)N * c->output_dim : 0, d_hidden,
                     (int64_t)n_taps * MW, sc);
  VTS_CHECK_LAUNCH("vts_clip_visual_backward (cotangent magnitude)");
  hipLaunchKernelGGL(vit_scale_kernel, dim3(1), dim3(64), 0, st, sc);
  VTS_CHECK_LAUNCH("vts_clip_visual_backward (cotangent factor)");
  // the topmost state that carries a cotangent: blocks above it see a zero gradient and are skipped
  int tap = n_taps - 1;      // the next tap to enter, from the top down
  const int top = d_out ? L : taps[tap];
  const float* top_tap = nullptr;
  if (tap >= 0 && taps[tap] == top) top_tap = d_hidden + (size_t)tap-- * MW;
  hipLaunchKernelGGL(vit_cotangent_kernel, dim3(mw_blocks), dim3(256), 0, st, g, top_tap, sc, 1, d_out ? nullptr : g16, MW);
  VTS_CHECK_LAUNCH("vts_clip_visual_backward (cotangent)");
  if (d_out) {
    hipLaunchKernelGGL(vit_dout_half_kernel, dim3(cdiv(N * bp.odp, 256)), dim3(256), 0, st, d_out, N, c->output_dim, bp.odp, sc, dout16);
    VTS_CHECK_LAUNCH("vts_clip_visual_backward (d_out)");
    if ((rc = gemm_launch(dout16, projB, nullptr, N, Wd, bp.odp, VTS_GEMM_NONE, dcls, 0, part, bp.part_floats, st)) != VTS_OK) return rc;
    // ln_post read the class token of each image: row n*T of the last state, and of its gradient
    if ((rc = layernorm_bwd_launch(dcls, tape + tp.xs + L * MW, (int64_t)T * Wd, N, Wd, ln_post_w, eps, g, (int64_t)T * Wd, 1, nullptr, st)) != VTS_OK)
      return rc;
    hipLaunchKernelGGL(vit_cotangent_kernel, dim3(mw_blocks), dim3(256), 0, st, g, (const float*)nullptr, sc, 0, g16, MW);
    VTS_CHECK_LAUNCH("vts_clip_visual_backward (gradient to fp16)");
  }
  for (int l = top - 1; l >= 0; --l) {
    const half_t* lw = layers_w + l * layer_halfs;
    const half_t* ln1_w = lw;
    const half_t* ln2_w = lw + 6 * (size_t)Wd + 4 * (size_t)W2;
    const half_t* inT = layers_t + (size_t)l * 12 * W2;
    const half_t* outT = inT + 3 * W2;
    const half_t* fcT = outT + W2;
    const half_t* pjT = fcT + 4 * W2;
    const float* lt = tape + tp.layer0 + l * tp.layer_stride;
    // g = dL/d(state l + 1).  MLP half: c_proj's input gradient times QuickGELU', c_fc's, ln_2's, added into the stream
    if ((rc = gemm_launch(g16, pjT, nullptr, M, 4 * Wd, Wd, VTS_GEMM_QUICKGELU_BWD, dmlp, 1, part, bp.part_floats, st, nullptr,
                          (half_t*)(lt + tp.fc))) != VTS_OK)
      return rc;
    if ((rc = gemm_launch(dmlp, fcT, nullptr, M, Wd, 4 * Wd, VTS_GEMM_NONE, dh, 0, part, bp.part_floats, st)) != VTS_OK) return rc;
    if ((rc = layernorm_bwd_launch(dh, lt + tp.mid, Wd, M, Wd, ln2_w, eps, g, Wd, 1, g16, st)) != VTS_OK) return rc;
    // attention half: out_proj's input gradient, the attention core's, in_proj's, ln_1's
    if ((rc = gemm_launch(g16, outT, nullptr, M, Wd, Wd, VTS_GEMM_NONE, datt, 1, part, bp.part_floats, st)) != VTS_OK) return rc;
    if ((rc = attention_bwd_launch((const half_t*)(lt + tp.qkv), datt, N, T, c->heads, 64, dqkv, st)) != VTS_OK) return rc;
    if ((rc = gemm_launch(dqkv, inT, nullptr, M, Wd, 3 * Wd, VTS_GEMM_NONE, dh, 0, part, bp.part_floats, st)) != VTS_OK) return rc;
    if ((rc = layernorm_bwd_launch(dh, tape + tp.xs + l * MW, Wd, M, Wd, ln1_w, eps, g, Wd, 1, g16, st)) != VTS_OK) return rc;
    if (tap >= 0 && taps[tap] == l) {
      hipLaunchKernelGGL(vit_cotangent_kernel, dim3(mw_blocks), dim3(256), 0, st, g, d_hidden + (size_t)tap * MW, sc, 0, g16, MW);
      VTS_CHECK_LAUNCH("vts_clip_visual_backward (tap)");
      --tap;
    }
  }
  // ln_pre, the embedding (class and positional embeddings are frozen: the class-token row ends here), conv1 as a GEMM, the patch scatter
  if ((rc = layernorm_bwd_launch(g, tape + tp.emb, Wd, M, Wd, ln_pre_w, eps, dh, Wd, 0, nullptr, st)) != VTS_OK) return rc;
  hipLaunchKernelGGL(vit_drop_cls_kernel, dim3((unsigned)cdiv64((int64_t)R * Wd, 256)), dim3(256), 0, st, dh, N, T, Wd, dtok);
  VTS_CHECK_LAUNCH("vts_clip_visual_backward (token rows)");
  if ((rc = gemm_launch(dtok, conv1T, nullptr, R, p.Kp, Wd, VTS_GEMM_NONE, dpatch, 0, part, bp.part_floats, st)) != VTS_OK) return rc;
  const int64_t ng = (int64_t)R * p.Kp;
  hipLaunchKernelGGL(vit_patch_scatter_kernel, dim3((unsigned)cdiv64(ng, 256)), dim3(256), 0, st, dpatch, N, c->resolution, c->patch, sc, dx);
  VTS_CHECK_LAUNCH("vts_clip_visual_backward (patch scatter)");
  return VTS_OK;
}
