// Single-output-channel member of the vts_conv4x4 family: the prediction heads of the PatchGAN discriminators
// (Conv2d(ndf*8, 1, 4, stride 1, pad 2), reference models/networks.py:1739-1741) on full-size maps.
//
// On the 16 x 16 x 4 MFMA tiles of conv4x4_kernel one of the sixteen output-channel columns carries work: the 64 -> 1 head at
// 131 x 131 took 78 us for 8 images, against 4.3 us of HBM time for its 34.6 MB input.  This layer is a 1024-term dot product per
// output pixel, so it runs on the vector ALUs.  Until round 13 a 1024-thread workgroup owned a 32 x 32 output tile and walked the
// channels in 8 chunks of 8 through an LDS patch (load -> LDS -> barrier -> FMAs -> barrier per chunk): 28 us whatever the map size
// (N4 34^2 .. N8 130^2: 27.7 - 29.8 us), the depth of that chain.  Now the lane = pixel form of vts_conv_px.hip (conv_head_kernel
// below): no LDS patch, no barrier in the channel loop, and the time follows the map: 8.7 us (N4 34^2) .. 23.8 us (N8 130^2) where the
// chunk-serial form took 24.0 .. 28.0 on the same box (one launch in a HIP graph, tools/mb_heads.py; profiles/r13_latency_floors.md).
// Algorithmic bytes = 4 (in + out + w).  Exact fp32; the summation order over (channel, ky, kx) is fixed.
#include <limits.h>
#include <stdlib.h>

#include "vts_internal.h"

namespace {

struct HeadK {
  const float* x;
  const float *sc, *sh;
  int64_t ns;
  int C, IH, IW, OH, OW, pad, padx;
  const float* w;
  int ws_ci;
  const float* bias;
  float* out;
  int64_t ons;
  float slope;
  const float* ident;
};

constexpr int HK_MAXC = 512;
constexpr int HK_T = 4;      // output rows per workgroup
constexpr int HK_CU = 4;     // channels per load round of a wave
constexpr int HK_VL = 61;    // output columns per workgroup: lane l loads input column x0 - pad + l, taps 1..3 come from lanes l + 1..3

typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ float ld_buf(const rsrc_t& rs, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ float and_bits(float v, unsigned m) { return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) & m); }
// whole-wave DPP shift: lane i <- lane i + 1, 0 at the open end (as in vts_conv_px.hip)
__device__ __forceinline__ float from_next(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xF, 0xF, true));
}

// Lane = pixel form: a workgroup owns T output rows x 61 output columns of one image; its four waves split the channels (wave w takes
// channels 2w, 2w + 1, 8 + 2w, 8 + 2w + 1, ...: the channels of partial sum w, see chan below) and keep T accumulators per lane.  Per channel a wave loads the T + 3 input rows of the tile as one coalesced
// row load each (lane l = input column x0 - pad + l; row and column clamped into the map, so every load is unconditional and in
// range), applies normalise + LeakyReLU once per loaded value and zeroes what lies outside the map with a mask, takes the three
// neighbouring taps over whole-wave DPP shifts, and multiplies with the channel's 16 taps as wave-uniform scalars.  No LDS and no
// barrier in the channel loop: the loads of the next CU channels are in flight while the current CU are multiplied.  The waves'
// partial sums are combined through LDS once, in wave order.  hipcc packs the FMAs of two output rows into v_pk_fma_f32; 93 VGPRs.
// The largest map (N8 130^2, 23.8 us = 1.48 TB/s) is bound by vector-ALU issue, not by HBM: 7 loaded rows per 4 output rows.
template <int T, int CU>
__global__ __launch_bounds__(256) void conv_head_kernel(const HeadK p) {
  constexpr int R = T + 3;
  static_assert(T % 4 == 0, "the four waves split the rows of the final combination");
  __shared__ float red[4][T][64];
  const int tid = threadIdx.x, lane = tid & 63, n = blockIdx.z;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int oy0 = blockIdx.y * T, ox0 = blockIdx.x * HK_VL;
  const int iy0 = oy0 - p.pad, ix = ox0 - p.padx + lane;
  const unsigned cmask = (ix >= 0 && ix < p.IW) ? 0xFFFFFFFFu : 0u;
  const unsigned vo = (unsigned)min(max(ix, 0), p.IW - 1) * 4u;
  unsigned so[R], rmask[R];   // wave-uniform: byte offset of the (clamped) input row inside a plane, all-ones where the row is inside the map
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int iy = iy0 + r;
    so[r] = (unsigned)(min(max(iy, 0), p.IH - 1) * p.IW) * 4u;
    rmask[r] = (iy >= 0 && iy < p.IH) ? 0xFFFFFFFFu : 0u;
  }
  const int plane = p.IH * p.IW;
  const float* xb = p.x + n * p.ns;
  // The wave's j-th channel.  The summation order per output is the one this kernel has had since round 2, so that results do not change
  // with the form: four partial sums, partial sum g over the channels c with (c % 8) / 2 == g in ascending order (per channel ky, kx
  // ascending, one fma chain), combined as ((s0 + s1) + s2) + s3, then the bias.  Wave g computes partial sum g.
  auto chan = [&](int j) { return (j >> 1) * 8 + wv * 2 + (j & 1); };
  const int nch = 2 * (p.C >> 3) + min(max((p.C & 7) - 2 * wv, 0), 2);     // channels of this wave: chan(j) < C exactly for j < nch
  const int nround = (nch + CU - 1) / CU;
  float acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = 0.f;
  float rawA[CU][R], rawB[CU][R];
  auto load = [&](float (&raw)[CU][R], int round) {
#pragma unroll
    for (int u = 0; u < CU; ++u) {
      const int c = min(chan(round * CU + u), p.C - 1);
      const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(xb + (int64_t)c * plane), 0, plane * 4, 0x00020000);
#pragma unroll
      for (int r = 0; r < R; ++r) raw[u][r] = ld_buf(rs, vo, so[r]);
    }
  };
  // scale / shift (the identity {1, 0} where the input has no affine) and the 16 taps of the wave's NEXT channel: fetched by scalar loads
  // one channel ahead, so their latency sits under the current channel's FMAs
  const float* scb = p.sc ? p.sc + n * p.C : p.ident;
  const float* shb = p.sh ? p.sh + n * p.C : p.ident + 1;
  const int scs = p.sc ? 1 : 0, shs = p.sh ? 1 : 0;
  float wq[16], scq, shq;
  auto fetch_w = [&](int j) {
    const int c = min(chan(j), p.C - 1);
    const float* wp = p.w + (int64_t)c * p.ws_ci;
#pragma unroll
    for (int k = 0; k < 16; ++k) wq[k] = wp[k];
    scq = scb[c * scs];
    shq = shb[c * shs];
  };
  auto compute = [&](float (&raw)[CU][R], int round) {
#pragma unroll
    for (int u = 0; u < CU; ++u) {
      const int j = round * CU + u;
      float w[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) w[k] = wq[k];
      const float sc = scq, sh = shq;
      fetch_w(j + 1);
      if (j < nch) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float t = fmaf(raw[u][r], sc, sh);
          const float v0 = and_bits(fmaxf(t, 0.f) + p.slope * fminf(t, 0.f), cmask & rmask[r]);
          const float v1 = from_next(v0), v2 = from_next(v1), v3 = from_next(v2);
#pragma unroll
          for (int ky = 0; ky < 4; ++ky) {
            const int o = r - ky;
            if (o >= 0 && o < T) {
              acc[o] = fmaf(v0, w[ky * 4], acc[o]);
              acc[o] = fmaf(v1, w[ky * 4 + 1], acc[o]);
              acc[o] = fmaf(v2, w[ky * 4 + 2], acc[o]);
              acc[o] = fmaf(v3, w[ky * 4 + 3], acc[o]);
            }
          }
        }
      }
    }
  };
  fetch_w(0);
  load(rawA, 0);
  for (int i = 0; i < nround; i += 2) {
    if (i + 1 < nround) load(rawB, i + 1);
    compute(rawA, i);
    if (i + 2 < nround) load(rawA, i + 2);
    compute(rawB, i + 1);
  }
#pragma unroll
  for (int t = 0; t < T; ++t) red[wv][t][lane] = acc[t];
  __syncthreads();
  const float bias = p.bias ? p.bias[0] : 0.f;
  const int x = ox0 + lane;
#pragma unroll
  for (int j = 0; j < T / 4; ++j) {
    const int t = wv * (T / 4) + j, y = oy0 + t;
    const float s = ((red[0][t][lane] + red[1][t][lane]) + red[2][t][lane]) + red[3][t][lane];
    if (lane < HK_VL && x < p.OW && y < p.OH) p.out[n * p.ons + (int64_t)y * p.OW + x] = s + bias;
  }
}

// ---- small maps (the same heads on the D2 patch passes: 640 maps of 6x6 / 4x4 / 3x3 -> 7x7 / 5x5 / 4x4): one thread per output of
// IPB whole images per workgroup (IPB * OH * OW <= 256), the zero-haloed input planes of 16 channels at a time in LDS
// (normalise + LeakyReLU on load), taps as wave-uniform LDS broadcast reads.  The flattened-batch MFMA kernel took 73 us for the
// 640-patch pass (one of sixteen output-channel columns carries work); this is ~1 MFLOP per workgroup of plain FMAs.
struct HeadSK {
  const float* x;
  const float *sc, *sh;
  int64_t ns;
  int C, N, IH, IW, OH, OW, pad, padx;
  const float* w;
  int ws_ci;
  const float* bias;
  float* out;
  int64_t ons;
  float slope;
  int IPB, PH, PW, CK;   // CK: channels staged per pass (all of them when two images' worth fits in LDS: one pass, one latency chain)
};

__global__ __launch_bounds__(256) void conv_head_small_kernel(const HeadSK p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* tile = smem;                                   // [IPB][p.CK][PH * PW]
  float* wl = smem + p.IPB * p.CK * p.PH * p.PW;       // [CK][16]
  const int tid = threadIdx.x;
  const int n0 = blockIdx.x * p.IPB;
  const int nimg = min(p.IPB, p.N - n0);
  const int plane = p.PH * p.PW, ohw = p.OH * p.OW, ihw = p.IH * p.IW;
  const int img = tid / ohw, r = tid - img * ohw;
  const int oy = r / p.OW, ox = r - oy * p.OW;
  const bool active = img < nimg;
  const int base = img * p.CK * plane + oy * p.PW + ox;          // window origin of this output inside channel 0 of its image
  for (int i = tid; i < p.IPB * p.CK * plane; i += 256) tile[i] = 0.f;
  float acc = 0.f;
  for (int c0 = 0; c0 < p.C; c0 += p.CK) {
    __syncthreads();
    // batches of 8 elements per thread: all global loads of a batch are issued before the first LDS store (a load -> store loop
    // exposes the full memory latency per element: measured 52 us for this kernel)
    const int total = nimg * p.CK * ihw;
    for (int e0 = tid; e0 < total; e0 += 256 * 8) {
      float raw[8], fsc[8], fsh[8];
      int dst[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int e = e0 + j * 256;
        const int ee = min(e, total - 1);
        const int ic = ee / ihw, q = ee - ic * ihw;
        const int im = ic / p.CK, c = ic - im * p.CK;
        const int y = q / p.IW, x = q - y * p.IW;
        const int cc = min(c0 + c, p.C - 1), n = n0 + im;
        raw[j] = p.x[n * p.ns + (int64_t)cc * ihw + q];
        fsc[j] = p.sc ? p.sc[n * p.C + cc] : 1.f;
        fsh[j] = p.sh ? p.sh[n * p.C + cc] : 0.f;
        dst[j] = (e < total && c0 + c < p.C) ? (im * p.CK + c) * plane + (y + p.pad) * p.PW + x + p.padx : -1 - ((im * p.CK + c) * plane + (y + p.pad) * p.PW + x + p.padx);
        if (e >= total) dst[j] = INT_MIN;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float t = fmaf(raw[j], fsc[j], fsh[j]);
        if (dst[j] >= 0) tile[dst[j]] = fmaxf(t, 0.f) + p.slope * fminf(t, 0.f);
        else if (dst[j] != INT_MIN) tile[-1 - dst[j]] = 0.f;      // channel beyond C inside the last chunk
      }
    }
    for (int e = tid; e < p.CK * 16; e += 256) wl[e] = (c0 + (e >> 4) < p.C) ? p.w[(int64_t)(c0 + (e >> 4)) * p.ws_ci + (e & 15)] : 0.f;
    __syncthreads();
    if (active) {
#pragma unroll 4
      for (int c = 0; c < p.CK; ++c) {
        const float* t = tile + base + c * plane;
#pragma unroll
        for (int ky = 0; ky < 4; ++ky)
#pragma unroll
          for (int kx = 0; kx < 4; ++kx) acc = fmaf(t[ky * p.PW + kx], wl[c * 16 + ky * 4 + kx], acc);
      }
    }
  }
  if (active) p.out[(n0 + img) * p.ons + r] = acc + (p.bias ? p.bias[0] : 0.f);
}

}  // namespace

int vts_conv_head_try(const vts_conv_desc* d, hipStream_t st) {
  if (d->transposed || d->stride != 1 || d->Cout != 1 || d->in1.data || d->dmask.data || d->accumulate || d->act_out != VTS_ACT_NONE)
    return VTS_ERR_UNSUPPORTED;
  if (d->in0.C > HK_MAXC || d->in0.C < 8 || (int64_t)d->IH * d->IW * d->in0.C >= (1ll << 31)) return VTS_ERR_UNSUPPORTED;
  if ((int64_t)d->OH * d->OW < 1024) {
    // small maps with a large batch (D2 patch passes)
    const int padx = d->pad + d->pad_dx;
    if (d->N < 32 || d->OH * d->OW > 256 || d->pad < 0 || padx < 0 || d->IH + d->pad < d->OH + 3 - d->pad || d->IW + padx < d->OW + 3 - padx)
      return VTS_ERR_UNSUPPORTED;
    HeadSK q;
    q.x = d->in0.data; q.sc = d->in0.scale; q.sh = d->in0.shift; q.ns = d->in0.nstride; q.C = d->in0.C; q.N = d->N;
    q.IH = d->IH; q.IW = d->IW; q.OH = d->OH; q.OW = d->OW; q.pad = d->pad; q.padx = padx;
    q.w = d->w; q.ws_ci = d->ws_ci; q.bias = d->bias; q.out = d->out; q.ons = d->out_nstride; q.slope = vts_slope(d->act_in);
    q.PH = d->IH + 2 * d->pad; q.PW = d->IW + 2 * padx;
    q.IPB = 256 / (d->OH * d->OW);
    q.CK = d->in0.C;
    auto bytes = [&]() { return (int64_t)(q.IPB * q.CK * q.PH * q.PW + q.CK * 16) * 4; };
    while (q.IPB > 2 && bytes() > 60 * 1024) --q.IPB;
    if (bytes() > 60 * 1024) {      // not even two images with all channels: 16 channels per pass
      q.CK = 16;
      q.IPB = 256 / (d->OH * d->OW);
      while (q.IPB > 1 && bytes() > 60 * 1024) --q.IPB;
    }
    const int lds = (int)bytes();
    if (lds > 64 * 1024) return VTS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(conv_head_small_kernel, dim3(cdiv(d->N, q.IPB)), dim3(256), lds, st, q);
    vts_set_kernel("conv_head_small_kernel");
    VTS_CHECK_LAUNCH("vts_conv4x4 (head, small maps)");
    return VTS_OK;
  }
  HeadK k;
  k.x = d->in0.data; k.sc = d->in0.scale; k.sh = d->in0.shift; k.ns = d->in0.nstride; k.C = d->in0.C;
  k.IH = d->IH; k.IW = d->IW; k.OH = d->OH; k.OW = d->OW; k.pad = d->pad; k.padx = d->pad + d->pad_dx;
  k.w = d->w; k.ws_ci = d->ws_ci; k.bias = d->bias; k.out = d->out; k.ons = d->out_nstride;
  k.slope = vts_slope(d->act_in);
  k.ident = vts_ident();
  dim3 grid(cdiv(d->OW, HK_VL), cdiv(d->OH, HK_T), d->N);
  hipLaunchKernelGGL((conv_head_kernel<HK_T, HK_CU>), grid, dim3(256), 0, st, k);
  vts_set_kernel("conv_head_kernel<%d, %d>", HK_T, HK_CU);
  VTS_CHECK_LAUNCH("vts_conv4x4 (head)");
  return VTS_OK;
}
