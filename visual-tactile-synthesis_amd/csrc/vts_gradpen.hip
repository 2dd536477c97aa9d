// WGAN-GP gradient penalty (reference models/networks.py:550-583, cal_gradient_penalty, type 'mixed'): the device code around the
// discriminator passes -- the interpolate x^ = a real + (1 - a) fake with torch.cat on store, and the penalty
// lambda / N sum_n (||g_n + 1e-16|| - c)^2 of the input gradient g with the cotangent dP/dg as an operand affine.  Both are HBM-bound.
// Everything is summed in a fixed order (no float atomics; the one integer add into the loss slot commutes), so a second call
// gives the same bits.
#include "vts_internal.h"

namespace {

constexpr int GP_T = 256;           // threads per workgroup
constexpr int GP_E = 16;            // elements per thread and block
constexpr int GP_BLOCK = GP_T * GP_E;
constexpr int GP_MAX_WG = 256;      // workgroups per sample at most; beyond that a workgroup walks several blocks, in order

struct gp_side {
  const float *p0, *p1;  // the two concat sources (p1 may be NULL)
  int64_t ns0, ns1;      // their sample strides
  int64_t m0;            // elements per sample the first source supplies (channels * HW)
};

// element i of sample n of cat(p0, p1): both sources are channel slices, contiguous within a sample
__device__ __forceinline__ float gp_fetch(const gp_side& s, int n, int64_t i) {
  return i < s.m0 ? s.p0[n * s.ns0 + i] : s.p1[n * s.ns1 + (i - s.m0)];
}

__global__ __launch_bounds__(GP_T) void gp_interp_kernel(gp_side real, gp_side fake, const float* __restrict__ alpha, int64_t M,
                                                         float* __restrict__ out) {
  const int n = blockIdx.y;
  const float a = alpha[n], b = 1.f - a;
  const int64_t base = (int64_t)blockIdx.x * (GP_T * 4) + threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t i = base + j * GP_T;
    if (i < M) out[(int64_t)n * M + i] = a * gp_fetch(real, n, i) + b * gp_fetch(fake, n, i);
  }
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block sum in double, fixed order; valid in every thread.  `red` holds >= 16 doubles.
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < nw; ++i) t += red[i];
  return t;
}

// part[n * gridDim.x + w] = sum over the blocks w, w + gridDim.x, ... of sample n of (g + 1e-16)^2, in double
__global__ __launch_bounds__(GP_T) void gp_sumsq_kernel(const float* __restrict__ g, int64_t M, int nblocks, double* __restrict__ part) {
  __shared__ double red[16];
  const int n = blockIdx.y;
  const float* p = g + (int64_t)n * M;
  double acc = 0.0;
  for (int b = blockIdx.x; b < nblocks; b += gridDim.x) {
    const int64_t base = (int64_t)b * GP_BLOCK + threadIdx.x;
#pragma unroll
    for (int j = 0; j < GP_E; ++j) {
      const int64_t i = base + j * GP_T;
      if (i < M) {
        const double d = (double)p[i] + 1e-16;
        acc = fma(d, d, acc);
      }
    }
  }
  acc = block_sum_d(acc, red);
  if (threadIdx.x == 0) part[(int64_t)n * gridDim.x + blockIdx.x] = acc;
}

// one workgroup: per-sample norms from the partials (in order), the cotangent affine, the penalty (samples in a fixed order)
__global__ __launch_bounds__(GP_T) void gp_finish_kernel(const double* __restrict__ part, int wg, int N, int C, double lambda_over_n,
                                                         double constant, double coeff, double grad_coeff, long long* __restrict__ loss,
                                                         float* __restrict__ value, float* __restrict__ scale, float* __restrict__ shift) {
  __shared__ double red[16];
  double pen = 0.0;
  for (int n = threadIdx.x; n < N; n += GP_T) {
    double s = 0.0;
    for (int w = 0; w < wg; ++w) s += part[(int64_t)n * wg + w];
    const double norm = sqrt(s);
    pen += (norm - constant) * (norm - constant);
    const float sc = (float)(grad_coeff * 2.0 * lambda_over_n * (norm - constant) / norm);
    const float sh = (float)((double)sc * 1e-16);
    for (int c = 0; c < C; ++c) {
      if (scale) scale[(int64_t)n * C + c] = sc;
      if (shift) shift[(int64_t)n * C + c] = sh;
    }
  }
  pen = block_sum_d(pen, red) * lambda_over_n;
  if (threadIdx.x == 0) {
    if (value) value[0] = (float)pen;
    if (loss) atomicAdd(reinterpret_cast<unsigned long long*>(loss), (unsigned long long)llrint(coeff * pen * VTS_LOSS_SCALE));
  }
}

static inline int gp_nblocks(int64_t M) { return (int)cdiv64(M, GP_BLOCK); }
static inline int gp_wg(int64_t M) {
  const int nb = gp_nblocks(M);
  return nb < GP_MAX_WG ? nb : GP_MAX_WG;
}

}  // namespace

extern "C" int vts_gp_interp(const float* real0, int64_t real0_nstride, int real0_c, const float* real1, int64_t real1_nstride, int real1_c,
                             const float* fake0, int64_t fake0_nstride, int fake0_c, const float* fake1, int64_t fake1_nstride, int fake1_c,
                             const float* alpha, int N, int64_t HW, float* out, void* stream) {
  VTS_CHECK_ARG(real0 && fake0 && alpha && out && N >= 1 && N <= 65535 && HW >= 1 && real0_c >= 1 && fake0_c >= 1,
                "vts_gp_interp: bad args");
  VTS_CHECK_ARG((real1 ? real1_c >= 1 : real1_c == 0) && (fake1 ? fake1_c >= 1 : fake1_c == 0), "vts_gp_interp: a second source needs channels, none has none");
  const int C = real0_c + real1_c;
  VTS_CHECK_ARG(C == fake0_c + fake1_c, "vts_gp_interp: real has %d channels, fake %d", C, fake0_c + fake1_c);
  VTS_CHECK_ARG(real0_nstride >= real0_c * HW && fake0_nstride >= fake0_c * HW && (!real1 || real1_nstride >= real1_c * HW) &&
                    (!fake1 || fake1_nstride >= fake1_c * HW),
                "vts_gp_interp: a sample stride is smaller than the sample");
  const int64_t M = (int64_t)C * HW;
  const int64_t gx = cdiv64(M, GP_T * 4);
  VTS_CHECK_ARG(gx <= 0x7fffffff, "vts_gp_interp: sample too large");
  const gp_side r = {real0, real1, real0_nstride, real1_nstride, (int64_t)real0_c * HW};
  const gp_side f = {fake0, fake1, fake0_nstride, fake1_nstride, (int64_t)fake0_c * HW};
  hipLaunchKernelGGL(gp_interp_kernel, dim3((unsigned)gx, N), dim3(GP_T), 0, (hipStream_t)stream, r, f, alpha, M, out);
  vts_set_kernel("gp_interp_kernel");
  VTS_CHECK_LAUNCH("vts_gp_interp");
  return VTS_OK;
}

extern "C" int64_t vts_gp_penalty_ws_floats(int N, int64_t M) {
  if (N < 1 || M < 1) return 0;
  return 2 * (int64_t)N * gp_wg(M);   // one double per (sample, workgroup)
}

extern "C" int vts_gp_penalty(const float* g, int N, int64_t M, int C, float lambda_gp, float constant, float coeff, float grad_coeff,
                              int64_t* loss_out, float* value, float* scale, float* shift, float* ws, void* stream) {
  VTS_CHECK_ARG(g && ws && N >= 1 && N <= 65535 && M >= 1 && C >= 1, "vts_gp_penalty: bad args");
  VTS_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "vts_gp_penalty: the workspace holds doubles and must be 8-byte aligned");
  VTS_CHECK_ARG(cdiv64(M, GP_BLOCK) <= 0x7fffffff, "vts_gp_penalty: sample too large");
  const int nb = gp_nblocks(M), wg = gp_wg(M);
  double* part = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(gp_sumsq_kernel, dim3(wg, N), dim3(GP_T), 0, (hipStream_t)stream, g, M, nb, part);
  hipLaunchKernelGGL(gp_finish_kernel, dim3(1), dim3(GP_T), 0, (hipStream_t)stream, part, wg, N, C, (double)lambda_gp / N, (double)constant,
                     (double)coeff, (double)grad_coeff, reinterpret_cast<long long*>(loss_out), value, scale, shift);
  vts_set_kernel("gp_sumsq_kernel[%d blocks on %d workgroups]+gp_finish_kernel", nb, wg);
  VTS_CHECK_LAUNCH("vts_gp_penalty");
  return VTS_OK;
}
