// Batched Fréchet distance: the contract of vts_frechet_distance (vts_metrics.hip) for npairs pairs of feature sets in three launches,
// for the baselines' evaluation metrics (models/model_utils.py:431-561 on a batch: one pair per image for I_SIFID, two per tactile
// patch for T_SIFID, one per patch for TactilePatchFID(reduction='mean'), models/tactile_patch_fid.py:88-154).
//
//   1. fdb_moments_partial_kernel, grid (position chunk, side, pair): raw moments sum x and sum x x^T of 64-position chunks in float64.
//   2. fdb_moments_final_kernel, grid (side, pair): the partials are summed in block order -> mean and unbiased covariance.
//   3. fdb_solve_kernel, one 256-thread workgroup per pair: A = S1 S2, |A|_F, the coupled Newton-Schulz iteration
//      Y <- Y T / 2, Z <- T Z / 2 with T = 3I - Z Y from Y = A / |A|_F, Z = I (at most 60 steps, ended once tr Y has converged), and the
//      final scalar.  Y, Z and T stay in LDS for the whole iteration: three double[64][66] arrays = 101,376 B (a gfx950 workgroup may hold 160 KiB, so one workgroup per CU).  The
//      products run on v_mfma_f64_16x16x4_f64: wave w owns rows 16w .. 16w + 15; an A operand is one f64 per lane, A[lane & 15][lane >> 4],
//      B is B[lane >> 4][lane & 15], and the four results of a lane are C[(lane >> 4) + 4 i][lane & 15].  D <= 16 NT rows / columns beyond
//      the leading 16 NT x 16 NT block decouple (Y is zero and Z diagonal there), so only that block is iterated.
//
// The number of partial blocks of a pair depends on its P alone and nothing is shared between pairs, so the result of a pair does not
// depend on npairs or on its index; every reduction runs in a fixed order (deterministic).
#include "vts_internal.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int FB_D = 64, FB_CHUNK = 64, FB_NB = 16, FB_LD = FB_D + 2;
constexpr int64_t FB_PER = FB_D + FB_D * FB_D;                 // doubles of one set of moments: sum x [64], sum x x^T [64][64]
constexpr int64_t FB_SIDE = (int64_t)(FB_NB + 1) * FB_PER;     // FB_NB partials, then {mean, covariance}
constexpr int64_t FB_PAIR = 2 * FB_SIDE;

struct FdbArgs {
  const float* f[2];
  int64_t P[2], stride[2];
  int nb[2];
  int D;
  double* ws;
};

__global__ __launch_bounds__(256) void fdb_moments_partial_kernel(const FdbArgs a) {
  __shared__ float tile[FB_D][FB_CHUNK + 1];
  const int side = blockIdx.y, nb = a.nb[side];
  if ((int)blockIdx.x >= nb) return;
  const int64_t P = a.P[side];
  const float* __restrict__ f = a.f[side] + (int64_t)blockIdx.z * a.stride[side];
  const int tid = threadIdx.x, D = a.D;
  double sx = 0.0, sxx[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) sxx[i] = 0.0;
  const int d0 = tid >> 2, e0 = (tid & 3) * 16;      // this thread's 16 (d, e) pairs: d = d0, e = e0 .. e0 + 15
  for (int64_t base = (int64_t)blockIdx.x * FB_CHUNK; base < P; base += (int64_t)nb * FB_CHUNK) {
    __syncthreads();
    for (int e = tid; e < FB_D * FB_CHUNK; e += 256) {
      const int d = e / FB_CHUNK, j = e - d * FB_CHUNK;
      tile[d][j] = (d < D && base + j < P) ? f[(int64_t)d * P + base + j] : 0.f;
    }
    __syncthreads();
    for (int j = 0; j < FB_CHUNK; ++j) {
      const double v = tile[d0][j];
      if ((tid & 3) == 0) sx += v;
#pragma unroll
      for (int i = 0; i < 16; ++i) sxx[i] += v * (double)tile[e0 + i][j];
    }
  }
  double* o = a.ws + (int64_t)blockIdx.z * FB_PAIR + side * FB_SIDE + (int64_t)blockIdx.x * FB_PER;
  if ((tid & 3) == 0) o[d0] = sx;
#pragma unroll
  for (int i = 0; i < 16; ++i) o[FB_D + d0 * FB_D + e0 + i] = sxx[i];
}

// mean [64] and unbiased covariance [64][64] (zero rows / columns beyond D) of one (side, pair)
__global__ __launch_bounds__(256) void fdb_moments_final_kernel(const FdbArgs a) {
  __shared__ double mu[FB_D];
  const int side = blockIdx.x, nb = a.nb[side], tid = threadIdx.x, D = a.D;
  const double P = (double)a.P[side];
  const double* part = a.ws + (int64_t)blockIdx.y * FB_PAIR + side * FB_SIDE;
  double* stat = a.ws + (int64_t)blockIdx.y * FB_PAIR + side * FB_SIDE + FB_NB * FB_PER;
  if (tid < FB_D) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part[(int64_t)b * FB_PER + tid];
    mu[tid] = s / P;
    stat[tid] = mu[tid];
  }
  __syncthreads();
  for (int e = tid; e < FB_D * FB_D; e += 256) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part[(int64_t)b * FB_PER + FB_D + e];
    const int d = e / FB_D, c = e - d * FB_D;
    stat[FB_D + e] = (d < D && c < D) ? (s - P * mu[d] * mu[c]) / (P - 1.0) : 0.0;
  }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// acc[t] += (rows 16w.. of A) (columns 16t.. of B) over the leading 16 NT block; A, B in LDS with row stride FB_LD
template <int NT>
__device__ __forceinline__ void fdb_strip_product(const double (*A)[FB_LD], const double (*B)[FB_LD], int wave, int lane, f64x4* acc) {
  const int r = lane & 15, q = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < NT * 4; ++ks) {
    const double av = A[wave * 16 + r][ks * 4 + q];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, B[ks * 4 + q][t * 16 + r], acc[t], 0, 0, 0);
  }
}

template <int NT>
__global__ __launch_bounds__(256) void fdb_solve_kernel(const double* __restrict__ ws, int D, float* __restrict__ out) {
  __shared__ double Y[FB_D][FB_LD], Z[FB_D][FB_LD], T[FB_D][FB_LD];
  __shared__ double red[4], trs[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const bool active = wave < NT;      // wave-uniform: the MFMAs run with all lanes on
  const double* st1 = ws + (int64_t)blockIdx.x * FB_PAIR + FB_NB * FB_PER;
  const double* st2 = st1 + FB_SIDE;
  for (int e = tid; e < FB_D * FB_D; e += 256) {      // S1 -> Y, S2 -> Z
    const int i = e >> 6, j = e & 63;
    Y[i][j] = st1[FB_D + e];
    Z[i][j] = st2[FB_D + e];
  }
  __syncthreads();
  double base = 0.0;      // |mu1 - mu2|^2 + tr S1 + tr S2, in wave 0
  if (wave == 0) {
    double v = 0.0;
    if (lane < D) {
      const double df = st1[lane] - st2[lane];
      v = df * df + Y[lane][lane] + Z[lane][lane];
    }
    base = wave_sum_f64(v);
  }
  f64x4 ya[NT], za[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) ya[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  double fro = 0.0;
  if (active) {
    fdb_strip_product<NT>(Y, Z, wave, lane, ya);      // A = S1 S2
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) fro += ya[t][i] * ya[t][i];
  }
  fro = wave_sum_f64(fro);
  if (lane == 0) red[wave] = fro;
  __syncthreads();      // also: every wave has read S1, S2
  const double nrm = sqrt(((red[0] + red[1]) + red[2]) + red[3]);
  const double inv = nrm > 0.0 ? 1.0 / nrm : 0.0;
  if (active) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = wave * 16 + q + 4 * i, col = t * 16 + r;
        Y[row][col] = ya[t][i] * inv;
        Z[row][col] = row == col ? 1.0 : 0.0;
      }
  }
  __syncthreads();
  double tr_prev = 0.0;
  for (int it = 0; it < 60; ++it) {      // at most 60 iterations: condition numbers up to ~2^60
    if (active) {
#pragma unroll
      for (int t = 0; t < NT; ++t) ya[t] = f64x4{0.0, 0.0, 0.0, 0.0};
      fdb_strip_product<NT>(Z, Y, wave, lane, ya);
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = wave * 16 + q + 4 * i, col = t * 16 + r;
          T[row][col] = (row == col ? 3.0 : 0.0) - ya[t][i];
        }
    }
    __syncthreads();
    if (active) {      // Y T and T Z both read the old Y and Z: both results wait in registers for the barrier
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        ya[t] = f64x4{0.0, 0.0, 0.0, 0.0};
        za[t] = f64x4{0.0, 0.0, 0.0, 0.0};
      }
#pragma unroll
      for (int ks = 0; ks < NT * 4; ++ks) {
        const double yv = Y[wave * 16 + r][ks * 4 + q], tv = T[wave * 16 + r][ks * 4 + q];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          ya[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(yv, T[ks * 4 + q][t * 16 + r], ya[t], 0, 0, 0);
          za[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(tv, Z[ks * 4 + q][t * 16 + r], za[t], 0, 0, 0);
        }
      }
    }
    {      // tr Y of this iteration: the diagonal lies in tile t = wave, in the lanes with lane & 15 = (lane >> 4) + 4 i
      double d = 0.0;
      if (active) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (t == wave && r == q + 4 * i) d += 0.5 * ya[t][i];
      }
      d = wave_sum_f64(d);
      if (lane == 0) trs[wave] = d;
    }
    __syncthreads();
    const double tr_it = ((trs[0] + trs[1]) + trs[2]) + trs[3];
    if (active) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = wave * 16 + q + 4 * i, col = t * 16 + r;
          Y[row][col] = 0.5 * ya[t][i];
          Z[row][col] = 0.5 * za[t][i];
        }
    }
    __syncthreads();
    // Converged: tr Y -- the one quantity that is returned, and a similarity invariant: the sum over the eigen-directions, each of which
    // rises monotonically to its limit -- moves by less than 1e-9 of itself (the result is a float32: 6e-8).  Iterating on is not only
    // idle: where S1 S2 is rank-deficient (constant regions in a generated patch) rounding leaves eigenvalues of about -1e-20 |A|, which the
    // coupled iteration amplifies by 2.25 per step until Y and Z overflow near step 50, and the growing Z lifts the rounding floor of tr Y
    // (~1e-16 |Z|) on the way.  A direction still growing at the stop holds less than 2e-9 of the trace after >= 15 steps of growth by 1.5,
    // so it could have added at most sqrt(2e-9) * 1.5^-7.5 = 2e-6 of it.  The same value in every thread: the branch is uniform.
    if (it > 0 && fabs(tr_it - tr_prev) <= 1e-9 * fabs(tr_it)) break;
    tr_prev = tr_it;
  }
  if (wave == 0) {
    const double tr = wave_sum_f64(lane < D ? Y[lane][lane] : 0.0);
    if (lane == 0) out[blockIdx.x] = (float)(base - 2.0 * sqrt(nrm) * tr);
  }
}

// crop matrix of TactilePatchFID: out[c * 9 + fh * 3 + fw][n * oh * ow + y * ow + x] = src[n][c][y + fh][x + fw]
__global__ __launch_bounds__(256) void tfid_features_kernel(const float* __restrict__ src, int N, int H, int W, int clamp01, float* __restrict__ out) {
  const int oh = H - 2, ow = W - 2;
  const int64_t cols = (int64_t)N * oh * ow, col = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (col >= cols) return;
  const int row = blockIdx.y, c = row / 9, fh = (row - c * 9) / 3, fw = row - c * 9 - fh * 3;
  const int64_t n = col / (oh * ow);
  const int p = (int)(col - n * oh * ow), y = p / ow, x = p - y * ow;
  float v = src[((n * 2 + c) * H + y + fh) * W + x + fw];
  if (clamp01) v = fminf(fmaxf(v, 0.f), 1.f);
  out[(int64_t)row * cols + col] = v;
}

}  // namespace

extern "C" int64_t vts_frechet_batched_ws_floats(int npairs) { return npairs < 1 ? 0 : 2 * FB_PAIR * (int64_t)npairs; }

extern "C" int vts_frechet_distance_batched(const float* feat1, const float* feat2, int D, int64_t P1, int64_t P2, int npairs, int64_t stride1,
                                            int64_t stride2, float* out, float* ws, void* stream) {
  VTS_CHECK_ARG(feat1 && feat2 && out && ws && D >= 1 && D <= FB_D && P1 >= 2 && P2 >= 2, "vts_frechet_distance_batched: bad args (D <= 64, P >= 2)");
  VTS_CHECK_ARG(npairs >= 1 && npairs <= 65535, "vts_frechet_distance_batched: npairs %d (1 .. 65535)", npairs);
  VTS_CHECK_ARG(stride1 >= (int64_t)D * P1 && stride2 >= (int64_t)D * P2, "vts_frechet_distance_batched: a pair stride is below D * P");
  VTS_CHECK_ARG(((uintptr_t)ws & 7) == 0, "vts_frechet_distance_batched: ws must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  FdbArgs a;
  a.f[0] = feat1; a.f[1] = feat2; a.P[0] = P1; a.P[1] = P2; a.stride[0] = stride1; a.stride[1] = stride2; a.D = D;
  a.ws = reinterpret_cast<double*>(ws);
  for (int s = 0; s < 2; ++s) {
    const int64_t chunks = (a.P[s] + FB_CHUNK - 1) / FB_CHUNK;
    a.nb[s] = (int)(chunks < FB_NB ? chunks : FB_NB);
  }
  hipLaunchKernelGGL(fdb_moments_partial_kernel, dim3(a.nb[0] > a.nb[1] ? a.nb[0] : a.nb[1], 2, npairs), dim3(256), 0, st, a);
  hipLaunchKernelGGL(fdb_moments_final_kernel, dim3(2, npairs), dim3(256), 0, st, a);
  const double* w = a.ws;
  switch ((D + 15) / 16) {
    case 1: hipLaunchKernelGGL(fdb_solve_kernel<1>, dim3(npairs), dim3(256), 0, st, w, D, out); break;
    case 2: hipLaunchKernelGGL(fdb_solve_kernel<2>, dim3(npairs), dim3(256), 0, st, w, D, out); break;
    case 3: hipLaunchKernelGGL(fdb_solve_kernel<3>, dim3(npairs), dim3(256), 0, st, w, D, out); break;
    default: hipLaunchKernelGGL(fdb_solve_kernel<4>, dim3(npairs), dim3(256), 0, st, w, D, out); break;
  }
  VTS_CHECK_LAUNCH("vts_frechet_distance_batched");
  return VTS_OK;
}

extern "C" int vts_tfid_features(const float* src, int N, int H, int W, int clamp01, float* out, void* stream) {
  VTS_CHECK_ARG(src && out && N >= 1 && H >= 3 && W >= 3, "vts_tfid_features: bad args (src [N, 2, H, W] with H, W >= 3)");
  const int64_t cols = (int64_t)N * (H - 2) * (W - 2);
  VTS_CHECK_ARG(cdiv64(cols, 256) <= 0x7fffffff, "vts_tfid_features: too many crops");
  hipLaunchKernelGGL(tfid_features_kernel, dim3((unsigned)cdiv64(cols, 256), 18), dim3(256), 0, (hipStream_t)stream, src, N, H, W, clamp01, out);
  VTS_CHECK_LAUNCH("vts_tfid_features");
  return VTS_OK;
}
