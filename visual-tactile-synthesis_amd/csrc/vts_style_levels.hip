// The tiled style code of an Up block as a 16-class bias (reference models/networks.py:1600-1623 with --num_layer_style_code > 1:
// the 512-value code is tiled to [N, 512, h, w] at every styled decoder level and concatenated in front of ConvTranspose2d(4, 2, 1)).
// The tile is constant over the map, so its share of the transposed convolution depends only on WHICH kernel taps an output position
// reaches.  Output row oy of OH = 2 IH reads kernel rows
//     class 0  {1}     oy = 0            class 1  {1, 3}  even oy > 0
//     class 2  {0, 2}  odd oy < OH - 1   class 3  {2}     oy = OH - 1
// and columns follow the same rule: 4 x 4 position classes.  With r[n,c] = max(code[n,c], 0) (the block's ReLU in front of the
// convolution) and V[n,co,ky,kx] = sum_c r[n,c] W[c,co,ky,kx] over the style rows of the weight, the style term of the output is
// B[n,co,class(oy,ox)] = sum of V over the taps of the class.
//   forward   V (one small matrix product, fixed summation order), then out = act(out + B[class]) in place
//   backward  S[n,co,class] = sum of g over the positions of the class (per-workgroup partials, summed in a fixed order: no float
//             atomics, bitwise repeatable), dV[n,co,ky,kx] = sum of S over the classes that contain the tap, and
//             dW[c,co,ky,kx] = sum_n r[n,c] dV[n,co,ky,kx] written into the style rows of the weight gradient
// No tile is ever materialised (512 x 512 x 512 floats per image at level 0 of a 1024 x 1024 input).
#include "vts_internal.h"

namespace {

constexpr int KSPLIT = 4;        // waves of a V workgroup: each sums a quarter of the code, the quarters are added in order
constexpr int MAX_CHUNKS = 64;   // row chunks of one (n, co) plane in the class sums

inline int row_chunks(int OH) { return min(max(cdiv(OH, 16), 1), MAX_CHUNKS); }

// V[n][j] = sum_c max(code[n][c], 0) * w[c][j],  j = co * 16 + tap < J
__global__ __launch_bounds__(256) void style_v_kernel(const float* __restrict__ code, const float* __restrict__ w, int K, int J, float* __restrict__ V) {
  __shared__ float red[KSPLIT][64];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6, n = blockIdx.y;
  const int j = blockIdx.x * 64 + lane;
  const int kq = (K + KSPLIT - 1) / KSPLIT;
  const int c0 = q * kq, c1 = min(K, c0 + kq);
  float acc = 0.f;
  if (j < J)
    for (int c = c0; c < c1; ++c) acc += fmaxf(code[(int64_t)n * K + c], 0.f) * w[(int64_t)c * J + j];
  red[q][lane] = acc;
  __syncthreads();
  if (q == 0 && j < J) {
    float s = red[0][lane];
#pragma unroll
    for (int i = 1; i < KSPLIT; ++i) s += red[i][lane];
    V[(int64_t)n * J + j] = s;
  }
}

__device__ __forceinline__ int pos_class(int o, int O) { return o == 0 ? 0 : (o == O - 1 ? 3 : ((o & 1) ? 2 : 1)); }

// out[n, co, oy, ox] = act(out + B[class(oy, ox)]);  grid (pixel chunks, N * Cout)
__global__ __launch_bounds__(256) void style_bias_apply_kernel(const float* __restrict__ V, int Cout, int OH, int OW, float* __restrict__ out,
                                                                int64_t out_nstride, int act_out) {
  __shared__ float B[16];
  const int nc = blockIdx.y, n = nc / Cout, co = nc - n * Cout;
  if (threadIdx.x < 16) {
    const int ry = threadIdx.x >> 2, rx = threadIdx.x & 3;
    // taps of a class: {1}, {1, 3}, {0, 2}, {2}
    const int t0[4] = {1, 1, 0, 2}, t1[4] = {-1, 3, 2, -1};
    const float* v = V + (int64_t)nc * 16;
    float s = 0.f;
    for (int a = 0; a < 2; ++a) {
      const int ky = a ? t1[ry] : t0[ry];
      if (ky < 0) continue;
      for (int b = 0; b < 2; ++b) {
        const int kx = b ? t1[rx] : t0[rx];
        if (kx < 0) continue;
        s += v[ky * 4 + kx];
      }
    }
    B[threadIdx.x] = s;
  }
  __syncthreads();
  const int hw = OH * OW;
  const int per = (hw + gridDim.x - 1) / gridDim.x;
  const int i0 = blockIdx.x * per, i1 = min(hw, i0 + per);
  float* p = out + (int64_t)n * out_nstride + (int64_t)co * hw;
  for (int i = i0 + threadIdx.x; i < i1; i += 256) {
    const int oy = i / OW, ox = i - oy * OW;
    float t = p[i] + B[pos_class(oy, OH) * 4 + pos_class(ox, OW)];
    if (act_out == VTS_ACT_TANH) t = tanhf(t);
    p[i] = t;
  }
}

// part[(nc * chunks + chunk) * 16 + class] = sum of g over the chunk's rows of plane nc, by class;  grid (chunks, N * Cout)
__global__ __launch_bounds__(256) void style_class_sums_kernel(const float* __restrict__ g, int64_t g_nstride, int Cout, int OH, int OW, int rows,
                                                                float* __restrict__ part) {
  __shared__ float red[4][16];
  const int nc = blockIdx.y, n = nc / Cout, co = nc - n * Cout;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int IW = OW >> 1;
  const int r0 = blockIdx.x * rows, r1 = min(OH, r0 + rows);
  const float* p = g + (int64_t)n * g_nstride + (int64_t)co * OH * OW;
  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int oy = r0 + wv; oy < r1; oy += 4) {
    const float* row = p + (int64_t)oy * OW;
    float eb = 0.f, ei = 0.f, oi = 0.f, ob = 0.f;      // column classes 0 .. 3 of this row
    for (int c = lane; c < IW; c += 64) {
      const float a = row[2 * c], b = row[2 * c + 1];
      if (c == 0) eb += a; else ei += a;
      if (c == IW - 1) ob += b; else oi += b;
    }
    if (oy == 0) {
      acc[0] += eb, acc[1] += ei, acc[2] += oi, acc[3] += ob;
    } else if (oy == OH - 1) {
      acc[12] += eb, acc[13] += ei, acc[14] += oi, acc[15] += ob;
    } else if (oy & 1) {
      acc[8] += eb, acc[9] += ei, acc[10] += oi, acc[11] += ob;
    } else {
      acc[4] += eb, acc[5] += ei, acc[6] += oi, acc[7] += ob;
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float s = wave_sum(acc[i]);
    if (lane == 0) red[wv][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < 16)
    part[((int64_t)nc * gridDim.x + blockIdx.x) * 16 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// dV[nc][ky][kx] = sum over the classes that contain the tap of S[nc][class], S = the chunk partials added in chunk order
__global__ __launch_bounds__(256) void style_dv_kernel(const float* __restrict__ part, int NC, int chunks, float* __restrict__ dV) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= NC * 16) return;
  const int nc = t >> 4, ky = (t >> 2) & 3, kx = t & 3;
  // classes that contain a tap: 0 -> {2}, 1 -> {0, 1}, 2 -> {2, 3}, 3 -> {1}
  const int c0[4] = {2, 0, 2, 1}, c1[4] = {-1, 1, 3, -1};
  float s = 0.f;
  for (int a = 0; a < 2; ++a) {
    const int ry = a ? c1[ky] : c0[ky];
    if (ry < 0) continue;
    for (int b = 0; b < 2; ++b) {
      const int rx = b ? c1[kx] : c0[kx];
      if (rx < 0) continue;
      float S = 0.f;
      for (int k = 0; k < chunks; ++k) S += part[((int64_t)nc * chunks + k) * 16 + ry * 4 + rx];
      s += S;
    }
  }
  dV[t] = s;
}

// dw[c][j] (+)= sum_n max(code[n][c], 0) * dV[n][j];  grid (J / 256, K)
__global__ __launch_bounds__(256) void style_dw_kernel(const float* __restrict__ code, const float* __restrict__ dV, int N, int K, int J, float* __restrict__ dw,
                                                        int accumulate) {
  const int j = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
  if (j >= J) return;
  float s = 0.f;
  for (int n = 0; n < N; ++n) s += fmaxf(code[(int64_t)n * K + c], 0.f) * dV[(int64_t)n * J + j];
  float* o = dw + (int64_t)c * J + j;
  *o = accumulate ? *o + s : s;
}

// ---- the Linear(style_dim, P, bias=False) of style_code_mapping<j> at the outer levels (project mapping): P = h w C reaches 81920 rows at
// a 128 x 128 map, where the 1 x 1-convolution form of the inner levels (a 4 x 4 tap embedding of the weight) no longer fits ----

// z[n][p] = sum_k x[n][k] w[p][k]: one wavefront per weight row
__global__ __launch_bounds__(256) void style_linear_kernel(const float* __restrict__ x, const float* __restrict__ w, int N, int K, int P, float* __restrict__ z) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= P) return;
  const float* row = w + (int64_t)p * K;
  for (int n = 0; n < N; ++n) {
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s += x[(int64_t)n * K + k] * row[k];
    s = wave_sum(s);
    if (lane == 0) z[(int64_t)n * P + p] = s;
  }
}

// part[chunk][n][k] = sum over the chunk's rows p of dz[n][p] w[p][k];  grid (chunks, K / 256, N)
__global__ __launch_bounds__(256) void style_linear_dx_kernel(const float* __restrict__ dz, const float* __restrict__ w, int K, int P, int rows,
                                                               float* __restrict__ part) {
  const int k = blockIdx.y * 256 + threadIdx.x, n = blockIdx.z, N = gridDim.z;
  if (k >= K) return;
  const int p0 = blockIdx.x * rows, p1 = min(P, p0 + rows);
  float s = 0.f;
  for (int p = p0; p < p1; ++p) s += dz[(int64_t)n * P + p] * w[(int64_t)p * K + k];
  part[((int64_t)blockIdx.x * N + n) * K + k] = s;
}

// dx[i] = sum over the chunks, in order, of part[chunk][i];  i < N * K
__global__ __launch_bounds__(256) void style_linear_dx_sum_kernel(const float* __restrict__ part, int NK, int chunks, float* __restrict__ dx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= NK) return;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += part[(int64_t)c * NK + i];
  dx[i] = s;
}

// dw[p][k] (+)= sum_n dz[n][p] x[n][k]
__global__ __launch_bounds__(256) void style_linear_dw_kernel(const float* __restrict__ dz, const float* __restrict__ x, int N, int K, int P,
                                                               float* __restrict__ dw, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)P * K) return;
  const int p = (int)(i / K), k = (int)(i - (int64_t)p * K);
  float s = 0.f;
  for (int n = 0; n < N; ++n) s += dz[(int64_t)n * P + p] * x[(int64_t)n * K + k];
  dw[i] = accumulate ? dw[i] + s : s;
}

inline int linear_chunks(int P) { return min(max(cdiv(P, 256), 1), 512); }

bool shape_ok(int N, int K, int Cout, int OH, int OW) {
  return N >= 1 && K >= 1 && Cout >= 1 && OH >= 2 && OW >= 2 && !(OH & 1) && !(OW & 1) && (int64_t)OH * OW < (int64_t)1 << 31 &&
         (int64_t)N * Cout <= 65535 && K <= 65535 && N <= 65535;
}

}  // namespace

extern "C" int64_t vts_style_bias_ws_floats(int N, int Cout, int OH) {
  if (N < 1 || Cout < 1 || OH < 1) return 0;
  return (int64_t)N * Cout * 16 * (row_chunks(OH) + 1);
}

extern "C" int vts_style_bias(const float* code, int N, int K, const float* w, int Cout, int OH, int OW, float* out, int64_t out_nstride,
                              int act_out, float* ws, void* stream) {
  VTS_CHECK_ARG(code && w && out && ws, "vts_style_bias: null pointer");
  VTS_CHECK_ARG(shape_ok(N, K, Cout, OH, OW), "vts_style_bias: bad shape N %d K %d Cout %d out %d x %d (even sizes, N * Cout <= 65535)", N, K, Cout, OH, OW);
  VTS_CHECK_ARG(out_nstride >= (int64_t)Cout * OH * OW, "vts_style_bias: batch stride %lld below Cout * OH * OW", (long long)out_nstride);
  VTS_CHECK_ARG(act_out == VTS_ACT_NONE || act_out == VTS_ACT_TANH, "vts_style_bias: act_out must be NONE or TANH");
  hipStream_t st = (hipStream_t)stream;
  const int J = Cout * 16;
  hipLaunchKernelGGL(style_v_kernel, dim3(cdiv(J, 64), N), dim3(256), 0, st, code, w, K, J, ws);
  VTS_CHECK_LAUNCH("vts_style_bias (V)");
  const int gx = (int)min((int64_t)256, cdiv64((int64_t)OH * OW, 2048));
  hipLaunchKernelGGL(style_bias_apply_kernel, dim3(gx, N * Cout), dim3(256), 0, st, (const float*)ws, Cout, OH, OW, out, out_nstride, act_out);
  VTS_CHECK_LAUNCH("vts_style_bias (apply)");
  vts_set_kernel("style_v_kernel+style_bias_apply_kernel");
  return VTS_OK;
}

extern "C" int vts_style_bias_bwd(const float* g, int64_t g_nstride, const float* code, int N, int K, int Cout, int OH, int OW, float* dw,
                                  int accumulate, float* ws, void* stream) {
  VTS_CHECK_ARG(g && code && dw && ws, "vts_style_bias_bwd: null pointer");
  VTS_CHECK_ARG(shape_ok(N, K, Cout, OH, OW), "vts_style_bias_bwd: bad shape N %d K %d Cout %d out %d x %d (even sizes, N * Cout <= 65535)", N, K, Cout, OH, OW);
  VTS_CHECK_ARG(g_nstride >= (int64_t)Cout * OH * OW, "vts_style_bias_bwd: batch stride %lld below Cout * OH * OW", (long long)g_nstride);
  hipStream_t st = (hipStream_t)stream;
  const int chunks = row_chunks(OH), rows = cdiv(OH, chunks), NC = N * Cout, J = Cout * 16;
  float* part = ws;                                  // [NC][chunks][16]
  float* dV = ws + (int64_t)NC * chunks * 16;        // [NC][16]
  hipLaunchKernelGGL(style_class_sums_kernel, dim3(chunks, NC), dim3(256), 0, st, g, g_nstride, Cout, OH, OW, rows, part);
  VTS_CHECK_LAUNCH("vts_style_bias_bwd (class sums)");
  hipLaunchKernelGGL(style_dv_kernel, dim3(cdiv(NC * 16, 256)), dim3(256), 0, st, (const float*)part, NC, chunks, dV);
  VTS_CHECK_LAUNCH("vts_style_bias_bwd (dV)");
  hipLaunchKernelGGL(style_dw_kernel, dim3(cdiv(J, 256), K), dim3(256), 0, st, code, (const float*)dV, N, K, J, dw, accumulate);
  VTS_CHECK_LAUNCH("vts_style_bias_bwd (dW)");
  vts_set_kernel("style_class_sums_kernel+style_dv_kernel+style_dw_kernel");
  return VTS_OK;
}

extern "C" int64_t vts_style_linear_ws_floats(int N, int K, int P) {
  if (N < 1 || K < 1 || P < 1) return 0;
  return (int64_t)linear_chunks(P) * N * K;
}

extern "C" int vts_style_linear(const float* x, const float* w, int N, int K, int P, float* z, void* stream) {
  VTS_CHECK_ARG(x && w && z, "vts_style_linear: null pointer");
  VTS_CHECK_ARG(N >= 1 && K >= 1 && P >= 1, "vts_style_linear: bad shape N %d K %d P %d", N, K, P);
  hipLaunchKernelGGL(style_linear_kernel, dim3(cdiv(P, 4)), dim3(256), 0, (hipStream_t)stream, x, w, N, K, P, z);
  VTS_CHECK_LAUNCH("vts_style_linear");
  vts_set_kernel("style_linear_kernel");
  return VTS_OK;
}

extern "C" int vts_style_linear_bwd(const float* dz, const float* x, const float* w, int N, int K, int P, float* dw, int accumulate, float* dx,
                                    float* ws, void* stream) {
  VTS_CHECK_ARG(dz && x && dw, "vts_style_linear_bwd: null pointer");
  VTS_CHECK_ARG(N >= 1 && N <= 65535 && K >= 1 && P >= 1, "vts_style_linear_bwd: bad shape N %d K %d P %d", N, K, P);
  VTS_CHECK_ARG(!dx || (w && ws), "vts_style_linear_bwd: dx needs the weight and a workspace");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(style_linear_dw_kernel, dim3((unsigned)cdiv64((int64_t)P * K, 256)), dim3(256), 0, st, dz, x, N, K, P, dw, accumulate);
  VTS_CHECK_LAUNCH("vts_style_linear_bwd (dW)");
  if (dx) {
    const int chunks = linear_chunks(P), rows = cdiv(P, chunks);
    hipLaunchKernelGGL(style_linear_dx_kernel, dim3(chunks, cdiv(K, 256), N), dim3(256), 0, st, dz, w, K, P, rows, ws);
    VTS_CHECK_LAUNCH("vts_style_linear_bwd (dx partials)");
    hipLaunchKernelGGL(style_linear_dx_sum_kernel, dim3(cdiv(N * K, 256)), dim3(256), 0, st, (const float*)ws, N * K, chunks, dx);
    VTS_CHECK_LAUNCH("vts_style_linear_bwd (dx)");
  }
  vts_set_kernel(dx ? "style_linear_dw_kernel+style_linear_dx_kernel+style_linear_dx_sum_kernel" : "style_linear_dw_kernel");
  return VTS_OK;
}
