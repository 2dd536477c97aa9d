// Kernels of the SPADE generator (reference models/networks.py:2075-2200 SPADEGenerator, models/architecture.py:21-68
// SPADEResnetBlock, models/normalization.py:68-112 SPADE; spectral normalisation = torch.nn.utils.spectral_norm, applied at
// models/architecture.py:35-39).  The convolutions run on the library's existing families; what is new here is bandwidth-bound:
//   modulate      out = act(xhat * (1 + gamma) + beta), xhat = (x - mean[n,c]) * rstd[n,c]; gamma / beta are per-pixel maps.  The
//                 statistics come per (n, c) from vts_norm_stats (instance or batch grouping) or from the running statistics (eval), so
//                 the kernel is the same for all three.  It can store into the zero-bordered [H+2][W+2] layout the GEMM-class 3x3
//                 convolution reads.
//   modulate bwd  pass 1 (one wave or one workgroup per (n, c) plane): dgamma = g' xhat, dbeta = g', h = g' (1 + gamma) (stored in dx) and
//                 the plane sums of h and h xhat, g' = g act'(.);  finalize: group means (plane, or over the batch in a fixed order);
//                 pass 2: dx = rstd ((h - mean(h)) - (xhat - mean(xhat)) mean(h xhat)).  mean(xhat) is 0 in exact arithmetic; subtracting the
//                 mean of the xhat actually computed keeps sum(dx) over a group at rounding level of dx itself also where rstd is large
//                 (a 1 x 2 plane whose two values nearly coincide), as autograd through x - mean(x) does.
//                 Frozen statistics: dx = rstd h in pass 1, nothing else.
//   nearest       F.interpolate(mode="nearest") source index (ATen's float rule), its adjoint as a gather, the x2 forms.
//   spectral norm one power iteration (training) + sigma = u^T W v + W / sigma; backward (G - <G, W/sigma> u v^T) / sigma.
// Every reduction runs in a fixed order over a fixed launch shape: results are bitwise repeatable, there are no float atomics.
#include "vts_internal.h"

namespace {

constexpr int kMaxBlocks = 4096;

// 16-byte alignment of every pointer given: the four-floats-per-lane forms need it (a parameter that is a view into a flat buffer starts
// at an arbitrary float offset)
template <typename... P>
static inline bool aligned16(const P*... p) {
  return (((uintptr_t)p | ...) & 15) == 0;
}

static inline int flat_grid(int64_t work, int block = 256) {
  const int64_t b = cdiv64(work, block);
  return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

// ---------------------------------------------------------------- modulate ----------------------------------------------------------------
// flat over the unpadded tensor, four consecutive pixels of one plane per thread (HW % 4 == 0)
__global__ __launch_bounds__(256) void spade_mod_fwd_v4(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, int64_t total4, int hw4, int act,
                                                         float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int64_t nc = i / hw4;
    const float m = mean[nc], r = rstd[nc];
    const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i], gv = reinterpret_cast<const f32x4*>(gamma)[i], bv = reinterpret_cast<const f32x4*>(beta)[i];
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = vts_act((xv[k] - m) * r * (1.f + gv[k]) + bv[k], act);
    reinterpret_cast<f32x4*>(out)[i] = o;
  }
}

// flat over the (padded) output: interior computed, border of `pad` pixels zero
__global__ __launch_bounds__(256) void spade_mod_fwd_pad(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, int64_t total, int H, int W, int pad,
                                                          int act, float* __restrict__ out) {
  const int PW = W + 2 * pad, plane = (H + 2 * pad) * PW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t nc = i / plane;
    const int p = (int)(i - nc * plane);
    const int y = p / PW - pad, xx = p % PW - pad;
    float v = 0.f;
    if ((unsigned)y < (unsigned)H && (unsigned)xx < (unsigned)W) {
      const int64_t j = nc * H * W + (int64_t)y * W + xx;
      v = vts_act((x[j] - mean[nc]) * rstd[nc] * (1.f + gamma[j]) + beta[j], act);
    }
    out[i] = v;
  }
}

// pass 1 of the backward.  WAVE: one wavefront per plane (four planes per workgroup), else one workgroup per plane.
template <bool WAVE>
__global__ __launch_bounds__(256) void spade_mod_bwd_sums(const float* __restrict__ g, int gpad, const float* __restrict__ x, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           int64_t NC, int H, int W, int act, int frozen, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, float* __restrict__ dx, float* __restrict__ sums) {
  __shared__ float red[48];
  const int64_t nc = WAVE ? (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) : (int64_t)blockIdx.x;
  const bool live = nc < NC;           // (WAVE: the tail wavefronts of the last workgroup own no plane; uniform per wavefront)
  const int t0 = WAVE ? (threadIdx.x & 63) : threadIdx.x, step = WAVE ? 64 : 256;
  const int hw = H * W, GW = W + 2 * gpad;
  float s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (live) {
    const float m = mean[nc], r = rstd[nc];
    const int64_t base = nc * hw, gbase = nc * (int64_t)(H + 2 * gpad) * GW;
    for (int j = t0; j < hw; j += step) {
      const int y = j / W, xx = j - y * W;
      const float xh = (x[base + j] - m) * r, ga = 1.f + gamma[base + j];
      const float gp = g[gbase + (int64_t)(y + gpad) * GW + xx + gpad] * vts_act_grad(xh * ga + beta[base + j], act);
      const float h = gp * ga;
      dgamma[base + j] = gp * xh;
      dbeta[base + j] = gp;
      dx[base + j] = frozen ? h * r : h;
      s1 += h;
      s2 += h * xh;
      s3 += xh;
    }
  }
  if (frozen) return;
  if (WAVE) {
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    s3 = wave_sum(s3);
  } else {
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red + 16);
    s3 = block_sum(s3, red + 32);
  }
  if (live && t0 == 0) {
    sums[nc] = s1;
    sums[NC + nc] = s2;
    sums[2 * NC + nc] = s3;
  }
}

// group means of the three sums: mode 0 the plane itself, mode 1 all planes of the channel, added in batch order
__global__ __launch_bounds__(256) void spade_mod_bwd_means(const float* __restrict__ sums, int N, int C, int HW, int mode, float* __restrict__ means) {
  const int64_t NC = (int64_t)N * C, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= NC) return;
  float a, b, e;
  if (mode == 0) {
    a = sums[i] / (float)HW;
    b = sums[NC + i] / (float)HW;
    e = sums[2 * NC + i] / (float)HW;
  } else {
    const int c = (int)(i % C);
    a = b = e = 0.f;
    for (int n = 0; n < N; ++n) {
      a += sums[(int64_t)n * C + c];
      b += sums[NC + (int64_t)n * C + c];
      e += sums[2 * NC + (int64_t)n * C + c];
    }
    const float cnt = (float)N * (float)HW;
    a /= cnt;
    b /= cnt;
    e /= cnt;
  }
  means[i] = a;
  means[NC + i] = b;
  means[2 * NC + i] = e;
}

// pass 2: dx holds h on entry
__global__ __launch_bounds__(256) void spade_mod_bwd_apply(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ means, int64_t NC, int hw, float* __restrict__ dx) {
  const int64_t total = NC * hw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t nc = i / hw;
    const float r = rstd[nc], xh = (x[i] - mean[nc]) * r;
    dx[i] = r * ((dx[i] - means[nc]) - (xh - means[2 * NC + nc]) * means[NC + nc]);
  }
}

// eval: the running statistics of BatchNorm2d(affine=False) broadcast over the batch in the [N*C] layout the modulate kernels read
__global__ __launch_bounds__(256) void spade_eval_stats_kernel(const float* __restrict__ rm, const float* __restrict__ rv, float eps, int N, int C,
                                                                float* __restrict__ mean, float* __restrict__ rstd) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)N * C) return;
  const int c = (int)(i % C);
  mean[i] = rm[c];
  rstd[i] = 1.f / sqrtf(rv[c] + eps);
}

// dz = g (1 - y^2), y = tanh(z): the output activation of the generator (networks.py:2198)
__global__ __launch_bounds__(256) void tanh_bwd_kernel(const float* __restrict__ g, const float* __restrict__ y, int64_t n, float* __restrict__ dz) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dz[i] = g[i] * (1.f - y[i] * y[i]);
}

// the same, four pixels of one plane per lane (hw % 4 == 0)
__global__ __launch_bounds__(256) void spade_mod_bwd_apply_v4(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                               const float* __restrict__ means, int64_t NC, int hw4, float* __restrict__ dx) {
  const int64_t total4 = NC * hw4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int64_t nc = i / hw4;
    const float m = mean[nc], r = rstd[nc], a = means[nc], b = means[NC + nc], e = means[2 * NC + nc];
    const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
    f32x4 d = reinterpret_cast<f32x4*>(dx)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = r * ((d[k] - a) - ((xv[k] - m) * r - e) * b);
    reinterpret_cast<f32x4*>(dx)[i] = d;
  }
}

// ---------------------------------------------------------------- nearest ----------------------------------------------------------------
// ATen's nearest_neighbor_compute_source_index with its identity / halving shortcuts (upsample_nearest2d, scale = in / out in float)
__device__ __forceinline__ int nearest_src(int dst, int in, int out, float scale) {
  if (in == out) return dst;
  if (out == 2 * in) return dst >> 1;
  const int s = (int)floorf((float)dst * scale);
  return s < in - 1 ? s : in - 1;
}

__global__ __launch_bounds__(256) void nearest_fwd_kernel(const float* __restrict__ x, int64_t NC, int IH, int IW, int OH, int OW, float sh, float sw,
                                                           float* __restrict__ out) {
  const int64_t total = NC * OH * OW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ox = (int)(i % OW);
    const int64_t t = i / OW;
    const int oy = (int)(t % OH);
    const int64_t nc = t / OH;
    out[i] = x[(nc * IH + nearest_src(oy, IH, OH, sh)) * IW + nearest_src(ox, IW, OW, sw)];
  }
}

// first destination index that maps to `src` or beyond it, found by walking the (monotone) forward rule from a safe start
__device__ __forceinline__ int nearest_first(int src, int in, int out, float scale) {
  int o = (int)((int64_t)src * out / in) - 2;
  if (o < 0) o = 0;
  while (o < out && nearest_src(o, in, out, scale) < src) ++o;
  return o;
}

__global__ __launch_bounds__(256) void nearest_bwd_kernel(const float* __restrict__ dout, int64_t NC, int IH, int IW, int OH, int OW, float sh, float sw,
                                                           float* __restrict__ din, int accumulate) {
  const int64_t total = NC * IH * IW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ix = (int)(i % IW);
    const int64_t t = i / IW;
    const int iy = (int)(t % IH);
    const int64_t nc = t / IH;
    const int x0 = nearest_first(ix, IW, OW, sw);
    float acc = 0.f;
    for (int oy = nearest_first(iy, IH, OH, sh); oy < OH && nearest_src(oy, IH, OH, sh) == iy; ++oy)
      for (int ox = x0; ox < OW && nearest_src(ox, IW, OW, sw) == ix; ++ox) acc += dout[(nc * OH + oy) * OW + ox];
    din[i] = accumulate ? din[i] + acc : acc;
  }
}

__global__ __launch_bounds__(256) void nearest_up2_kernel(const float* __restrict__ x, int64_t NC, int H, int W, float* __restrict__ out) {
  const int64_t total = NC * H * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int xx = (int)(i % W);
    const int64_t row = i / W;   // nc * H + y
    const float v = x[i];
    float2* o = reinterpret_cast<float2*>(out + (row * 2) * (2 * W) + 2 * xx);   // even offsets: 8-byte aligned
    o[0] = make_float2(v, v);
    o[W] = make_float2(v, v);
  }
}

__global__ __launch_bounds__(256) void nearest_up2_bwd_kernel(const float* __restrict__ dout, int64_t NC, int H, int W, float* __restrict__ din, int accumulate) {
  const int64_t total = NC * H * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int xx = (int)(i % W);
    const int64_t row = i / W;
    const float2* o = reinterpret_cast<const float2*>(dout + (row * 2) * (2 * W) + 2 * xx);
    const float2 a = o[0], b = o[W];
    const float s = (a.x + a.y) + (b.x + b.y);
    din[i] = accumulate ? din[i] + s : s;
  }
}

// ---------------------------------------------------------------- spectral norm ----------------------------------------------------------------
constexpr int kSnRows = 64;   // rows of W one workgroup of the W^T u pass adds up

// part[rs][j] = sum over the rows i of slab rs of W[i][j] u[i]   (lane = column: coalesced rows)
__global__ __launch_bounds__(256) void sn_wtu_kernel(const float* __restrict__ w, const float* __restrict__ u, int Co, int K, float* __restrict__ part) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= K) return;
  const int i0 = blockIdx.y * kSnRows, i1 = min(Co, i0 + kSnRows);
  float acc = 0.f;
  for (int i = i0; i < i1; ++i) acc += w[(int64_t)i * K + j] * u[i];
  part[(int64_t)blockIdx.y * K + j] = acc;
}

// one workgroup: v = t / max(|t|, eps), t[j] = sum of the slabs in order
__global__ __launch_bounds__(1024) void sn_v_kernel(const float* __restrict__ part, int RS, int K, float eps, float* __restrict__ v) {
  __shared__ float red[16];
  float ss = 0.f;
  for (int j = threadIdx.x; j < K; j += 1024) {
    float t = 0.f;
    for (int r = 0; r < RS; ++r) t += part[(int64_t)r * K + j];
    v[j] = t;
    ss += t * t;
  }
  const float nrm = fmaxf(sqrtf(block_sum(ss, red)), eps);
  for (int j = threadIdx.x; j < K; j += 1024) v[j] = v[j] / nrm;    // (each thread rewrites only what it wrote)
}

// s[i] = W[i] . v, one workgroup per row
__global__ __launch_bounds__(256) void sn_wv_kernel(const float* __restrict__ w, const float* __restrict__ v, int K, int vec, float* __restrict__ s) {
  __shared__ float red[16];
  const float* row = w + (int64_t)blockIdx.x * K;
  float acc = 0.f;
  if (vec) {
    for (int j = threadIdx.x; j < K / 4; j += 256) {
      const f32x4 a = reinterpret_cast<const f32x4*>(row)[j], b = reinterpret_cast<const f32x4*>(v)[j];
      acc += (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
    }
  } else {
    for (int j = threadIdx.x; j < K; j += 256) acc += row[j] * v[j];
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) s[blockIdx.x] = acc;
}

// one workgroup: training u <- s / max(|s|, eps); sigma = u . s
__global__ __launch_bounds__(1024) void sn_sigma_kernel(const float* __restrict__ s, int Co, int training, float eps, float* __restrict__ u,
                                                         float* __restrict__ sigma) {
  __shared__ float red[32];
  float nrm = 1.f;
  if (training) {
    float ss = 0.f;
    for (int i = threadIdx.x; i < Co; i += 1024) ss += s[i] * s[i];
    nrm = fmaxf(sqrtf(block_sum(ss, red)), eps);
  }
  float d = 0.f;
  for (int i = threadIdx.x; i < Co; i += 1024) {
    float ui;
    if (training) {
      ui = s[i] / nrm;
      u[i] = ui;
    } else {
      ui = u[i];
    }
    d += ui * s[i];
  }
  d = block_sum(d, red + 16);
  if (threadIdx.x == 0) sigma[0] = d;
}

__global__ __launch_bounds__(256) void sn_scale_kernel(const float* __restrict__ w, const float* __restrict__ sigma, int64_t n, float* __restrict__ out) {
  const float sg = sigma[0];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = w[i] / sg;
}

// rowdot[i] = G[i] . Wsn[i]
__global__ __launch_bounds__(256) void sn_bwd_dot_kernel(const float* __restrict__ g, const float* __restrict__ wsn, int K, float* __restrict__ rowdot) {
  __shared__ float red[16];
  const float *a = g + (int64_t)blockIdx.x * K, *b = wsn + (int64_t)blockIdx.x * K;
  float acc = 0.f;
  for (int j = threadIdx.x; j < K; j += 256) acc += a[j] * b[j];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) rowdot[blockIdx.x] = acc;
}

// one workgroup: total[0] = sum of rowdot in a fixed order
__global__ __launch_bounds__(256) void sn_bwd_total_kernel(const float* __restrict__ rowdot, int Co, float* __restrict__ total) {
  __shared__ float red[16];
  float d = 0.f;
  for (int i = threadIdx.x; i < Co; i += 256) d += rowdot[i];
  d = block_sum(d, red);
  if (threadIdx.x == 0) total[0] = d;
}

// dw[i][j] (+)= (G[i][j] - d u[i] v[j]) / sigma, d = total[0]; blockIdx.y = row
__global__ __launch_bounds__(256) void sn_bwd_apply_kernel(const float* __restrict__ g, const float* __restrict__ total, const float* __restrict__ u,
                                                            const float* __restrict__ v, const float* __restrict__ sigma, int Co, int K,
                                                            float* __restrict__ dw, int accumulate) {
  const int i = blockIdx.y;
  const float du = total[0] * u[i], sg = sigma[0];
  for (int j = blockIdx.x * 256 + threadIdx.x; j < K; j += gridDim.x * 256) {
    const int64_t o = (int64_t)i * K + j;
    const float val = (g[o] - du * v[j]) / sg;
    dw[o] = accumulate ? dw[o] + val : val;
  }
}

}  // namespace

extern "C" int vts_spade_modulate(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, int N, int C, int H,
                                  int W, int act, float* out, int out_pad, void* stream) {
  VTS_CHECK_ARG(x && mean && rstd && gamma && beta && out, "vts_spade_modulate: null pointer");
  VTS_CHECK_ARG(N >= 1 && C >= 1 && H >= 1 && W >= 1 && (out_pad == 0 || out_pad == 1) && (act == VTS_ACT_NONE || act == VTS_ACT_LRELU),
                "vts_spade_modulate: bad shape / out_pad %d / act %d", out_pad, act);
  VTS_CHECK_ARG((int64_t)(H + 2) * (W + 2) < (1ll << 31), "vts_spade_modulate: plane too large");
  const int64_t NC = (int64_t)N * C;
  hipStream_t st = (hipStream_t)stream;
  if (out_pad == 0 && ((H * W) & 3) == 0 && aligned16(x, gamma, beta, out)) {
    const int64_t total4 = NC * (H * W / 4);
    hipLaunchKernelGGL(spade_mod_fwd_v4, dim3(flat_grid(total4)), dim3(256), 0, st, x, mean, rstd, gamma, beta, total4, H * W / 4, act, out);
    vts_set_kernel("spade_mod_fwd_v4");
  } else {
    const int64_t total = NC * (H + 2 * out_pad) * (W + 2 * out_pad);
    hipLaunchKernelGGL(spade_mod_fwd_pad, dim3(flat_grid(total)), dim3(256), 0, st, x, mean, rstd, gamma, beta, total, H, W, out_pad, act, out);
    vts_set_kernel("spade_mod_fwd_pad");
  }
  VTS_CHECK_LAUNCH("vts_spade_modulate");
  return VTS_OK;
}

extern "C" int vts_spade_eval_stats(const float* running_mean, const float* running_var, float eps, int N, int C, float* mean, float* rstd,
                                    void* stream) {
  VTS_CHECK_ARG(running_mean && running_var && mean && rstd && N >= 1 && C >= 1, "vts_spade_eval_stats: bad args");
  hipLaunchKernelGGL(spade_eval_stats_kernel, dim3((unsigned)cdiv64((int64_t)N * C, 256)), dim3(256), 0, (hipStream_t)stream, running_mean,
                     running_var, eps, N, C, mean, rstd);
  VTS_CHECK_LAUNCH("vts_spade_eval_stats");
  vts_set_kernel("spade_eval_stats_kernel");
  return VTS_OK;
}

extern "C" int64_t vts_spade_modulate_bwd_ws_floats(int N, int C) { return 6ll * N * C; }

extern "C" int vts_spade_modulate_bwd(const float* g, int g_pad, const float* x, const float* mean, const float* rstd, const float* gamma,
                                      const float* beta, int N, int C, int H, int W, int mode, int act, float* dgamma, float* dbeta, float* dx,
                                      float* ws, void* stream) {
  VTS_CHECK_ARG(g && x && mean && rstd && gamma && beta && dgamma && dbeta && dx, "vts_spade_modulate_bwd: null pointer");
  VTS_CHECK_ARG(N >= 1 && C >= 1 && H >= 1 && W >= 1 && (g_pad == 0 || g_pad == 1) && mode >= 0 && mode <= 2 &&
                    (act == VTS_ACT_NONE || act == VTS_ACT_LRELU),
                "vts_spade_modulate_bwd: bad shape / g_pad %d / mode %d / act %d", g_pad, mode, act);
  VTS_CHECK_ARG((int64_t)(H + 2) * (W + 2) < (1ll << 31), "vts_spade_modulate_bwd: plane too large");
  VTS_CHECK_ARG(mode == 2 || ws, "vts_spade_modulate_bwd: the training modes need the workspace");
  const int64_t NC = (int64_t)N * C;
  const int frozen = mode == 2;
  hipStream_t st = (hipStream_t)stream;
  float *sums = ws, *means = ws ? ws + 3 * NC : nullptr;
  const bool wave = H * W <= 1024;
  if (wave)
    hipLaunchKernelGGL(spade_mod_bwd_sums<true>, dim3((unsigned)cdiv64(NC, 4)), dim3(256), 0, st, g, g_pad, x, mean, rstd, gamma, beta, NC, H, W, act,
                       frozen, dgamma, dbeta, dx, sums);
  else
    hipLaunchKernelGGL(spade_mod_bwd_sums<false>, dim3((unsigned)NC), dim3(256), 0, st, g, g_pad, x, mean, rstd, gamma, beta, NC, H, W, act, frozen,
                       dgamma, dbeta, dx, sums);
  VTS_CHECK_LAUNCH("vts_spade_modulate_bwd (sums)");
  if (frozen) {
    vts_set_kernel(wave ? "spade_mod_bwd_sums<wave> frozen" : "spade_mod_bwd_sums<block> frozen");
    return VTS_OK;
  }
  hipLaunchKernelGGL(spade_mod_bwd_means, dim3((unsigned)cdiv64(NC, 256)), dim3(256), 0, st, sums, N, C, H * W, mode, means);
  VTS_CHECK_LAUNCH("vts_spade_modulate_bwd (means)");
  const bool v4 = ((H * W) & 3) == 0 && aligned16(x, dx);
  if (v4)
    hipLaunchKernelGGL(spade_mod_bwd_apply_v4, dim3(flat_grid(NC * (H * W / 4))), dim3(256), 0, st, x, mean, rstd, means, NC, H * W / 4, dx);
  else
    hipLaunchKernelGGL(spade_mod_bwd_apply, dim3(flat_grid(NC * H * W)), dim3(256), 0, st, x, mean, rstd, means, NC, H * W, dx);
  VTS_CHECK_LAUNCH("vts_spade_modulate_bwd (apply)");
  if (wave)
    vts_set_kernel(v4 ? "spade_mod_bwd_sums<wave>+spade_mod_bwd_means+spade_mod_bwd_apply_v4" : "spade_mod_bwd_sums<wave>+spade_mod_bwd_means+spade_mod_bwd_apply");
  else
    vts_set_kernel(v4 ? "spade_mod_bwd_sums<block>+spade_mod_bwd_means+spade_mod_bwd_apply_v4" : "spade_mod_bwd_sums<block>+spade_mod_bwd_means+spade_mod_bwd_apply");
  return VTS_OK;
}

extern "C" int vts_tanh_bwd(const float* g, const float* y, int64_t n, float* dz, void* stream) {
  VTS_CHECK_ARG(g && y && dz && n >= 1, "vts_tanh_bwd: bad args");
  hipLaunchKernelGGL(tanh_bwd_kernel, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, g, y, n, dz);
  VTS_CHECK_LAUNCH("vts_tanh_bwd");
  vts_set_kernel("tanh_bwd_kernel");
  return VTS_OK;
}

extern "C" int vts_nearest_resize(const float* x, int64_t NC, int IH, int IW, int OH, int OW, float* out, void* stream) {
  VTS_CHECK_ARG(x && out && NC >= 1 && IH >= 1 && IW >= 1 && OH >= 1 && OW >= 1, "vts_nearest_resize: bad args");
  hipLaunchKernelGGL(nearest_fwd_kernel, dim3(flat_grid(NC * OH * OW)), dim3(256), 0, (hipStream_t)stream, x, NC, IH, IW, OH, OW, (float)IH / (float)OH,
                     (float)IW / (float)OW, out);
  VTS_CHECK_LAUNCH("vts_nearest_resize");
  vts_set_kernel("nearest_fwd_kernel");
  return VTS_OK;
}

extern "C" int vts_nearest_resize_bwd(const float* dout, int64_t NC, int IH, int IW, int OH, int OW, float* din, int accumulate, void* stream) {
  VTS_CHECK_ARG(dout && din && NC >= 1 && IH >= 1 && IW >= 1 && OH >= 1 && OW >= 1, "vts_nearest_resize_bwd: bad args");
  hipLaunchKernelGGL(nearest_bwd_kernel, dim3(flat_grid(NC * IH * IW)), dim3(256), 0, (hipStream_t)stream, dout, NC, IH, IW, OH, OW,
                     (float)IH / (float)OH, (float)IW / (float)OW, din, accumulate);
  VTS_CHECK_LAUNCH("vts_nearest_resize_bwd");
  vts_set_kernel("nearest_bwd_kernel");
  return VTS_OK;
}

extern "C" int vts_nearest_up2(const float* x, int64_t NC, int H, int W, float* out, void* stream) {
  VTS_CHECK_ARG(x && out && NC >= 1 && H >= 1 && W >= 1, "vts_nearest_up2: bad args");
  VTS_CHECK_ARG(((uintptr_t)out & 7) == 0, "vts_nearest_up2: out must be 8-byte aligned (float2 stores)");
  hipLaunchKernelGGL(nearest_up2_kernel, dim3(flat_grid(NC * H * W)), dim3(256), 0, (hipStream_t)stream, x, NC, H, W, out);
  VTS_CHECK_LAUNCH("vts_nearest_up2");
  vts_set_kernel("nearest_up2_kernel");
  return VTS_OK;
}

extern "C" int vts_nearest_up2_bwd(const float* dout, int64_t NC, int H, int W, float* din, int accumulate, void* stream) {
  VTS_CHECK_ARG(dout && din && NC >= 1 && H >= 1 && W >= 1, "vts_nearest_up2_bwd: bad args");
  VTS_CHECK_ARG(((uintptr_t)dout & 7) == 0, "vts_nearest_up2_bwd: dout must be 8-byte aligned (float2 loads)");
  hipLaunchKernelGGL(nearest_up2_bwd_kernel, dim3(flat_grid(NC * H * W)), dim3(256), 0, (hipStream_t)stream, dout, NC, H, W, din, accumulate);
  VTS_CHECK_LAUNCH("vts_nearest_up2_bwd");
  vts_set_kernel("nearest_up2_bwd_kernel");
  return VTS_OK;
}

extern "C" int64_t vts_spectral_norm_ws_floats(int Co, int K) { return (int64_t)cdiv(Co, kSnRows) * K + Co; }

extern "C" int vts_spectral_norm(const float* w, float* u, float* v, int Co, int K, int training, float eps, float* w_out, float* sigma, float* ws,
                                 int64_t ws_floats, void* stream) {
  VTS_CHECK_ARG(w && u && v && w_out && sigma && ws, "vts_spectral_norm: null pointer");
  VTS_CHECK_ARG(Co >= 1 && K >= 1 && Co <= 65535, "vts_spectral_norm: bad shape %d x %d", Co, K);
  VTS_CHECK_ARG(ws_floats >= vts_spectral_norm_ws_floats(Co, K), "vts_spectral_norm: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int RS = cdiv(Co, kSnRows);
  float *part = ws, *s = ws + (int64_t)RS * K;
  if (training) {
    hipLaunchKernelGGL(sn_wtu_kernel, dim3(cdiv(K, 256), RS), dim3(256), 0, st, w, u, Co, K, part);
    VTS_CHECK_LAUNCH("vts_spectral_norm (W^T u)");
    hipLaunchKernelGGL(sn_v_kernel, dim3(1), dim3(1024), 0, st, part, RS, K, eps, v);
    VTS_CHECK_LAUNCH("vts_spectral_norm (v)");
  }
  const int vec = (int)((K & 3) == 0 && aligned16(w, v));
  hipLaunchKernelGGL(sn_wv_kernel, dim3(Co), dim3(256), 0, st, w, v, K, vec, s);
  VTS_CHECK_LAUNCH("vts_spectral_norm (W v)");
  hipLaunchKernelGGL(sn_sigma_kernel, dim3(1), dim3(1024), 0, st, s, Co, training, eps, u, sigma);
  VTS_CHECK_LAUNCH("vts_spectral_norm (sigma)");
  hipLaunchKernelGGL(sn_scale_kernel, dim3(flat_grid((int64_t)Co * K)), dim3(256), 0, st, w, sigma, (int64_t)Co * K, w_out);
  VTS_CHECK_LAUNCH("vts_spectral_norm (scale)");
  if (training)
    vts_set_kernel(vec ? "sn_wtu_kernel+sn_v_kernel+sn_wv_kernel<vec>+sn_sigma_kernel+sn_scale_kernel"
                       : "sn_wtu_kernel+sn_v_kernel+sn_wv_kernel<scalar>+sn_sigma_kernel+sn_scale_kernel");
  else
    vts_set_kernel(vec ? "sn_wv_kernel<vec>+sn_sigma_kernel+sn_scale_kernel" : "sn_wv_kernel<scalar>+sn_sigma_kernel+sn_scale_kernel");
  return VTS_OK;
}

extern "C" int vts_spectral_norm_bwd(const float* g, const float* w_sn, const float* u, const float* v, const float* sigma, int Co, int K, float* dw,
                                     int accumulate, float* ws, int64_t ws_floats, void* stream) {
  VTS_CHECK_ARG(g && w_sn && u && v && sigma && dw && ws, "vts_spectral_norm_bwd: null pointer");
  VTS_CHECK_ARG(Co >= 1 && K >= 1 && Co <= 65535 && ws_floats >= Co + 1, "vts_spectral_norm_bwd: bad shape %d x %d or workspace", Co, K);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sn_bwd_dot_kernel, dim3(Co), dim3(256), 0, st, g, w_sn, K, ws);
  VTS_CHECK_LAUNCH("vts_spectral_norm_bwd (dot)");
  hipLaunchKernelGGL(sn_bwd_total_kernel, dim3(1), dim3(256), 0, st, ws, Co, ws + Co);
  VTS_CHECK_LAUNCH("vts_spectral_norm_bwd (total)");
  const int gx = cdiv(K, 256) < 16 ? cdiv(K, 256) : 16;
  hipLaunchKernelGGL(sn_bwd_apply_kernel, dim3(gx, Co), dim3(256), 0, st, g, ws + Co, u, v, sigma, Co, K, dw, accumulate);
  VTS_CHECK_LAUNCH("vts_spectral_norm_bwd (apply)");
  vts_set_kernel("sn_bwd_dot_kernel+sn_bwd_total_kernel+sn_bwd_apply_kernel");
  return VTS_OK;
}
