// "Lane = pixel" members of the vts_conv4x4 family for THIN layers on full-size maps (round 3): the stride-2 Conv2d(4) forward of the
// outer U-Net encoder layers and of the first PatchGAN layers (reference thirdparty/unet/unet_parts_custom.py:9-47,
// models/networks.py:1696-1750), and the backward-data pass of the outer ConvTranspose2d(4, s2) decoder layers (the same operator).
//
// Why a second MFMA mapping.  conv4x4_kernel feeds v_mfma_f32_16x16x4_f32: N = 16 output channels, K = 4 taps x 4-channel chunks.  A layer
// with 10 output channels and 9 input channels fills 10/16 of N and 9/12 of K: the matrix pipe does 2.1x the useful work and the 9 -> 10
// layer at 1024^2 is MFMA-bound at 41 us where HBM allows 24.  Here the contraction runs on v_mfma_f32_4x4x1_16b_f32 -- sixteen
// independent 4 x 4 outer products per instruction, the same 256 flop / cycle / CU -- with the A-operand BROADCAST (CBSZ = 4: every block
// takes the A of block ABID; semantics and rate measured by tools/probes/mfma_4x4x1.hip):
//
//     D[lane][i] += A[4 * ABID + i] * B[lane]            i = 0..3
//
//   B = one input value per lane: lane l IS output pixel (y, x0 + l), so the operand of tap (ci, ky, kx) is in[ci][2y + ky - pad][2(x0 + l) + kx - pad]
//       -- loaded straight from global memory (four stride-2 dword loads per input row cover the four kx; the lines are shared through L1 / TA),
//       no LDS patch, no barrier in the channel loop, waves run independently;
//   A = ONE register per (input channel, block of 4 output channels): lane 4 * tap + i holds w[co = 4 * blk + i][ci][tap]; ABID = tap walks its
//       16 K-steps.  The images of all (ci, blk) are staged once per workgroup in LDS (Cin * NB * 256 bytes) and read with one
//       conflict-free ds_read_b32 per 16 * T MFMAs;
//   D = 4 output channels of the lane's pixel: channel planes go out as 256-byte rows straight from the accumulators.
// Output channels are padded to a multiple of 4 (10 -> 12, 20 -> 20, 8 -> 8), K is not padded at all.  Exact fp32 (k-ordered fma chain).
// A wave owns T output rows x 64 columns; a workgroup 4 T rows x 64 columns (rows of neighbouring waves share input rows through L1).
#include <stdlib.h>

#include <type_traits>

#include "vts_internal.h"

namespace {

// Register budget (round 5; second argument of __launch_bounds__ = minimum waves per SIMD): unconstrained, hipcc splits the allocation into
// architectural + accumulation halves and these HBM-bound members ran 3 - 6 waves per SIMD (80 - 164 registers); they fit 5 - 6 waves (<= 96 /
// <= 80) without a spill, and the extra waves hide the load latency: 9 -> 10 at 1024^2 66.4 -> 58.1 us, its input adjoint 90.6 -> 76.0,
// D1 layer 0 (N = 8) 52.8 -> 48.9, its image gradient 56.7 -> 47.0, 16 -> 8 transposed 60.2 -> 55.1; sum over the thin-layer shapes of
// tools/mb_px.py 958 -> 915 us (profiles/r05h_px_ab_launch_bounds.txt).  Six waves only where nothing spills (the convolution with <= 3
// channel blocks); eight waves spilled and ran 2 - 10x slower.
constexpr int px_min_waves(bool transposed, int nb) { return (!transposed && nb <= 3) ? 6 : 5; }


typedef __amdgpu_buffer_rsrc_t rsrc_t;
constexpr unsigned OOB_OFF = 0x40000000u;    // lane part of a byte offset outside the row (planes are < 2^30 bytes: checked by the host side)
constexpr unsigned ROW_OOB = 0x7F000000u;    // uniform part of a row above / below the map: the sum stays beyond every plane without wrapping

struct PxK {
  const float *s0, *s1, *sc0, *sh0, *sc1, *sh1;
  int64_t ns0, ns1;
  int C0, C1, Cin;
  int IH, IW, OH, OW, Cout, pad, padx;
  const float* w;
  int ws_co, ws_ci;
  const float* bias;
  float* out;
  int64_t ons;
  const float *dm, *dmsc, *dmsh;
  int64_t dmns;
  int dmC;
  float dm_slope;       // mask derivative as t > 0 ? 1 : slope
  int tanh_out;
  int accumulate;
  const float* ident;   // {1, 0}
  float slope_in;
  int identity_in;
  int xcd_swizzle;
  int tiles_x, tiles_y;
  float* stat_part;     // STATS 1: (mean, M2, count) per wave slot, the partial format of stats_partial_kernel (vts_norm.hip)
  float* bsum_part;     // STATS 2: (S1, S2') per wave slot, the layout of norm_bwd_partial_kernel
  int stat_spl;
  int N;
  int ablate;           // profiling only (env VTS_ABLATE): 1 skip the pixel loads, 2 skip the MFMAs, 4 skip the epilogue
};

// ABID is an immediate: a compile-time loop hands every tap its own constant
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>());
    static_for<I + 1, N>(f);
  }
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
// (a function of a scalar: __builtin_bit_cast applied directly to an ext-vector ELEMENT in an unrolled loop yields element 0 -- DESIGN.md)
__device__ __forceinline__ float and_bits(float v, unsigned m) { return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) & m); }
__device__ __forceinline__ float ld_buf(const rsrc_t& rs, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)voff, (int)soff, 0));
}
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 ld_buf2(const rsrc_t& rs, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)voff, (int)soff, 0));
}
// whole-wave DPP shifts (tools/probes/dpp_wave_shift.hip): lane i <- lane i + 1 / lane i - 1, 0 at the open end
__device__ __forceinline__ float from_next(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xF, 0xF, true));
}
__device__ __forceinline__ float from_prev(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xF, 0xF, true));
}

// NB: blocks of 4 output channels; T: output rows per wave; PP: parity of the horizontal padding; STATS: 0 plain, 1 output statistics,
// 2 sums of the normalisation backward.
//
// Input staging.  Measured on the 9 -> 10 layer at 1024^2 (tools/mb_px.py, VTS_ABLATE): four stride-2 dword loads per input row (one per
// kx) are bound by the texture addresser -- 59 us for the loads alone; one 16-byte load per row and lane (overlapping quads) costs
// 37 us and 48 more registers than this form, which takes 27 us: lane l loads ONE aligned column pair P_g = (2g, 2g + 1) per input row --
// a fully used 512-byte wave load -- and the two taps that belong to the neighbouring pairs come over whole-wave DPP shifts:
//   padding even (2m):      pixel xo = g + m   taps kx 0,1 = P_g          kx 2,3 = P_{g+1}                   63 pixels per wave (lanes 0..62)
//   padding odd  (2m + 1):  pixel xo = g + m   tap  kx 0 = P_{g-1}.y      kx 1,2 = P_g    kx 3 = P_{g+1}.x   62 pixels per wave (lanes 1..62)
// Pairs never straddle the left edge; an odd input width makes the last pair straddle the right edge (its second dword is masked).
// 84 - 110 registers: 4 - 5 waves per SIMD hide the load latency without any software pipelining beyond one channel of prefetch.
// Merge of the four waves' epilogue records of one tile (round 4): Chan's formula for the statistics (mean, M2, count), plain sums for the
// normalisation-backward pairs, waves 0 .. 3 in order (deterministic); ONE slot per workgroup -- the mergers behind read a quarter of the
// records they read with one slot per wave.  Every thread of the workgroup must call it (barrier).
template <int NB, int STATS>
__device__ __forceinline__ void px_merge_stats(const float* px_stat, const PxK& p, int n, int slot) {
  __syncthreads();
  const int co = threadIdx.x;
  if (co >= NB * 4 || co >= p.Cout) return;
  if (STATS == 1) {
    float cnt = 0.f, wm = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float* q = px_stat + (w * NB * 4 + co) * 3;
      cnt += q[2];
      wm = fmaf(q[2], q[0], wm);
    }
    const float mean = wm / fmaxf(cnt, 1.f);
    float m2 = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float* q = px_stat + (w * NB * 4 + co) * 3;
      const float d = q[0] - mean;
      m2 += q[1] + q[2] * d * d;
    }
    float* o = p.stat_part + (((int64_t)n * p.Cout + co) * p.stat_spl + slot) * 3;
    o[0] = mean + (p.bias ? p.bias[co] : 0.f);
    o[1] = m2;
    o[2] = cnt;
  } else {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float* q = px_stat + (w * NB * 4 + co) * 3;
      s1 += q[0];
      s2 += q[1];
    }
    float* o = p.bsum_part + (((int64_t)n * p.Cout + co) * p.stat_spl + slot) * 2;
    o[0] = s1;
    o[1] = s2;
  }
}

template <int NB, int T, int PP, int STATS>
__global__ __launch_bounds__(256, px_min_waves(false, NB)) void conv_px_s2_kernel(const PxK p) {
  constexpr int R = 2 * T + 2;   // input rows under T output rows
  constexpr int VL = PP ? 62 : 63, L0 = PP ? 1 : 0;
  extern __shared__ float wl[];  // [ci][blk][64]: A-operand images
  __shared__ float px_stat[STATS ? 4 * NB * 4 * 3 : 1];   // per-wave statistics / backward-sum records of the tile, merged at the end
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int iplane = p.IH * p.IW;
  const int oplane = p.OH * p.OW;
  {
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    if (p.xcd_swizzle) {   // every XCD walks one contiguous run of tiles (as conv4x4_kernel): neighbours meet in the same L2
      const int gx = gridDim.x, gy = gridDim.y, nwg = gx * gy * (int)gridDim.z;
      const int lin = bx + gx * (by + gy * bz);
      const int q = nwg >> 3, r = nwg & 7, xcd = lin & 7, idx = lin >> 3;
      const int lin2 = xcd * q + min(xcd, r) + idx;
      bz = lin2 / (gx * gy);
      const int rem = lin2 - bz * (gx * gy);
      by = rem / gx;
      bx = rem - by * gx;
    }
    const int n = bz;
    const int x0 = bx * VL, y0 = (by * 4 + wave) * T;
    const int xo = x0 + lane - L0;
    const int g = xo - ((p.padx - PP) >> 1);

    // lane part of the byte offset of the lane's column pair; uniform parts of the R input rows
    const unsigned vo = (g >= 0 && 2 * g < p.IW) ? (unsigned)g * 8u : OOB_OFF;
    const unsigned m0 = vo != OOB_OFF ? 0xFFFFFFFFu : 0u, m1 = (g >= 0 && 2 * g + 1 < p.IW) ? 0xFFFFFFFFu : 0u;
    const bool iw_odd = p.IW & 1;
    unsigned so[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int iy = 2 * y0 - p.pad + r;
      so[r] = (iy >= 0 && iy < p.IH) ? (unsigned)(iy * p.IW) * 4u : ROW_OOB;
    }
    const float* sb0 = p.s0 + n * p.ns0;
    const float* sb1 = p.s1 + n * p.ns1;

    auto load_px = [&](int ci, f32x2 (&v)[R], float& sc, float& sh) {
      {
        const int ccl = min(ci, p.Cin - 1);
        const bool first = ccl < p.C0;
        const int cl = first ? ccl : ccl - p.C0;
        const float* scp = first ? p.sc0 : p.sc1;
        const float* shp = first ? p.sh0 : p.sh1;
        const int aidx = n * (first ? p.C0 : p.C1) + cl;
        const bool hsc = scp != nullptr, hsh = shp != nullptr;
        sc = (hsc ? scp : p.ident)[hsc ? aidx : 0];
        sh = (hsh ? shp : p.ident)[hsh ? aidx : 1];
      }
      const bool cok = ci < p.Cin;
      const int cc = cok ? ci : 0;
      const bool first = cc < p.C0;
      const float* base = (first ? sb0 : sb1) + (int64_t)(first ? cc : cc - p.C0) * iplane;
      const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, cok ? iplane * 4 : 0, 0x00020000);
      if (p.ablate & 1) return;
#pragma unroll
      for (int r = 0; r < R; ++r) v[r] = ld_buf2(rs, vo, so[r]);
    };
    auto load_a = [&](int ci, float (&a)[NB]) {
      const float* src = wl + min(ci, p.Cin - 1) * (NB * 64) + lane;
#pragma unroll
      for (int b = 0; b < NB; ++b) a[b] = src[b * 64];
    };
    // pad( act( x * scale + shift ) ) on the loaded pairs (every element once, before the taps are distributed): the loads returned 0
    // outside the map, which an affine would move -- rows outside get scale = shift = 0, columns outside are masked
    auto finish = [&](f32x2 (&v)[R], float sc, float sh) {
      if (!p.identity_in) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const bool rok = so[r] != ROW_OOB;   // uniform
          const float scr = rok ? sc : 0.f, shr = rok ? sh : 0.f;
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const float t = fmaf(v[r][j], scr, shr);
            const float a = fmaxf(t, 0.f) + p.slope_in * fminf(t, 0.f);
            v[r][j] = and_bits(a, j ? m1 : m0);
          }
        }
      } else if (iw_odd) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float y = v[r][1];
          v[r][1] = and_bits(y, m1);
        }
      }
    };

    f32x4 acc[T][NB];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[t][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto mm = [&](const float (&a)[NB], const f32x2 (&v)[R]) {
      if (p.ablate & 2) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) s += v[r][0] + v[r][1];
        acc[0][0][0] += s * a[0];
        return;
      }
      float b[R][4];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (PP == 0) {
          b[r][0] = v[r][0];
          b[r][1] = v[r][1];
          b[r][2] = from_next(v[r][0]);
          b[r][3] = from_next(v[r][1]);
        } else {
          b[r][0] = from_prev(v[r][1]);
          b[r][1] = v[r][0];
          b[r][2] = v[r][1];
          b[r][3] = from_next(v[r][0]);
        }
      }
      static_for<0, 16>([&](auto tc) {
        constexpr int tap = decltype(tc)::value, ky = tap >> 2, kx = tap & 3;
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
          for (int bl = 0; bl < NB; ++bl) acc[t][bl] = __builtin_amdgcn_mfma_f32_4x4x1f32(a[bl], b[2 * t + ky][kx], acc[t][bl], 4, tap, 0);
      });
    };

    f32x2 va[R] = {}, vb[R] = {};
    float aa[NB], ab[NB];
    float sca, sha, scb, shb;
    load_px(0, va, sca, sha);   // in flight while the weights are staged
    for (int e = tid; e < p.Cin * NB * 64; e += 256) {
      const int l = e & 63, r = e >> 6;
      const int blk = r % NB, ci = r / NB;
      const int co = blk * 4 + (l & 3), tap = l >> 2;
      wl[e] = co < p.Cout ? p.w[(int64_t)co * p.ws_co + (int64_t)ci * p.ws_ci + tap] : 0.f;
    }
    __syncthreads();
    load_a(0, aa);
    // two channels per trip (register sets a / b), no exit inside the body: at the top of a trip set a holds channel ci
    for (int ci = 0; ci + 1 < p.Cin; ci += 2) {
      load_px(ci + 1, vb, scb, shb);
      load_a(ci + 1, ab);
      finish(va, sca, sha);
      mm(aa, va);
      load_px(ci + 2, va, sca, sha);   // beyond Cin: num_records = 0, no memory traffic
      load_a(ci + 2, aa);
      finish(vb, scb, shb);
      mm(ab, vb);
    }
    if (p.Cin & 1) {
      finish(va, sca, sha);
      mm(aa, va);
    }

    if (p.ablate & 4) {
      float s = 0.f;
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int b = 0; b < NB; ++b) s += acc[t][b][0] + acc[t][b][1] + acc[t][b][2] + acc[t][b][3];
      if (s == 123.456f) p.out[0] = s;
      return;
    }
    // ---- epilogue: lane = pixel, register = channel: every (row, channel) is one 252- / 248-byte row segment.  Branch-free per block of 4
    // channels: rows beyond OH / channels beyond Cout carry an out-of-range uniform offset (the hardware drops the access), a missing
    // bias / mask affine reads the identity constants, the mask derivative is the slope form; all loads of a block are issued together.
    const int onb = p.Cout * oplane * 4;
    const rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc((void*)(p.out + n * p.ons), 0, onb, 0x00020000);
    const rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.dm ? p.dm + n * p.dmns : p.out), 0, p.dm ? p.dmC * oplane * 4 : 0, 0x00020000);
    const bool xok = lane >= L0 && lane < L0 + VL && xo < p.OW;
    const unsigned vox = xok ? (unsigned)xo * 4u : OOB_OFF;
    const int slot = by * p.tiles_x + bx;
    const int nvy = min(max(p.OH - y0, 0), T);
    const float cnt = (float)(nvy * min(max(p.OW - x0, 0), VL));
    const float* biasp = p.bias ? p.bias : p.ident + 1;
    const float* dscp = (p.dm && p.dmsc) ? p.dmsc + n * p.dmC : p.ident;
    const float* dshp = (p.dm && p.dmsh) ? p.dmsh + n * p.dmC : p.ident + 1;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      unsigned soff[T][4];
      float bias[4], dsc[4], dsh[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int co = b * 4 + i, coc = min(co, p.Cout - 1);
        bias[i] = biasp[p.bias ? coc : 0];
        dsc[i] = dscp[(p.dm && p.dmsc) ? coc : 0];
        dsh[i] = dshp[(p.dm && p.dmsh) ? coc : 0];
#pragma unroll
        for (int t = 0; t < T; ++t) soff[t][i] = (co < p.Cout && y0 + t < p.OH) ? (unsigned)(co * oplane + (y0 + t) * p.OW) * 4u : ROW_OOB;
      }
      float dmv[T][4], prev[T][4];
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          dmv[t][i] = 1.f;
          prev[t][i] = 0.f;
        }
      if (p.dm) {
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) dmv[t][i] = ld_buf(drs, vox, soff[t][i]);
      }
      if (p.accumulate) {
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) prev[t][i] = ld_buf(ors, vox, soff[t][i]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const bool ok = xok && soff[t][i] != ROW_OOB;
          const float raw = acc[t][b][i];
          if (STATS == 1) {           // (the host enables this only for the plain "store acc + bias" form); sums before the bias
            const float m = ok ? raw : 0.f;
            s1 += m;
            s2 = fmaf(m, m, s2);
          }
          const float tn = fmaf(dmv[t][i], dsc[i], dsh[i]);
          const float v = fmaf(raw + bias[i], tn > 0.f ? 1.f : p.dm_slope, prev[t][i]);
          if (STATS == 2 && ok) {
            s1 += v;
            s2 = fmaf(v, tn, s2);
          }
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ors, (int)vox, (int)soff[t][i], 0);
        }
        if (STATS != 0) {
          s1 = wave_sum(s1);
          s2 = wave_sum(s2);
          const int co = b * 4 + i;
          if (lane == 0) {      // this wave's record; the four waves of the tile are merged below (one slot per workgroup: round 4)
            float* q = px_stat + (wave * NB * 4 + co) * 3;
            if (STATS == 1) {
              const float mean = s1 / fmaxf(cnt, 1.f);
              q[0] = mean;
              q[1] = fmaxf(s2 - s1 * mean, 0.f);
              q[2] = cnt;
            } else {
              q[0] = s1;
              q[1] = s2;
            }
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);   // one block at a time
    }
    if (STATS != 0) px_merge_stats<NB, STATS>(px_stat, p, n, slot);
  }
}

// ---- stride-2 TRANSPOSED member (ConvTranspose2d(4, s2) forward of the outer decoder layers, backward-data of the stride-2 Conv2d(4)
// layers; reference thirdparty/unet/unet_parts_custom.py:49-79, models/networks.py:1696-1750): replaces convt2_thin_kernel, whose packed
// FMAs are bound by the wave-uniform LDS reads of their weights (one 16-byte read per two FMAs, shared by four SIMDs).
// Lane l IS low-resolution column qx: it owns the 2 x 2 output quad (2 qy + a, 2 qx + b) of T low-resolution rows for all output
// channels.  Phase (a, b) takes taps ky = ((a + pad) & 1) + 2 j, kx = ((b + pad) & 1) + 2 i from the input at row qy + ps - 1 + d, column
// qx + ps - 1 + e (ps = pad / 2; d, e < 3 for odd, < 2 for even padding): the lane loads ONE value per input row -- a coalesced 256-byte
// wave load -- and the columns beside it come over whole-wave DPP shifts (62 / 63 positions per wave).  All 16 taps of a channel are the
// 16 K-steps of one A image (ABID = tap); an output row leaves as (b = 0, b = 1) pairs: 8-byte stores of 496 / 504 contiguous bytes.
__device__ __forceinline__ float tanh_fast(float x) {   // branch-free; absolute error < 1.2e-7 (the output is O(1): images in [-1, 1])
  const float t = __expf(-2.f * fabsf(x));
  return copysignf((1.f - t) / (1.f + t), x);
}

template <int NB, int T, int PP, int STATS>
__global__ __launch_bounds__(256, px_min_waves(true, NB)) void convt_px_s2_kernel(const PxK p) {
  constexpr int ND = PP ? 3 : 2;
  constexpr int R = T + ND - 1;   // input rows under T low-resolution rows
  constexpr int VL = PP ? 62 : 63, L0 = PP ? 1 : 0;
  extern __shared__ float wl[];  // [ci][blk][64]: A-operand images
  __shared__ float px_stat[STATS ? 4 * NB * 4 * 3 : 1];   // per-wave statistics / backward-sum records of the tile, merged at the end
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int iplane = p.IH * p.IW;
  const int oplane = p.OH * p.OW;
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (p.xcd_swizzle) {
    const int gx = gridDim.x, gy = gridDim.y, nwg = gx * gy * (int)gridDim.z;
    const int lin = bx + gx * (by + gy * bz);
    const int q = nwg >> 3, r = nwg & 7, xcd = lin & 7, idx = lin >> 3;
    const int lin2 = xcd * q + min(xcd, r) + idx;
    bz = lin2 / (gx * gy);
    const int rem = lin2 - bz * (gx * gy);
    by = rem / gx;
    bx = rem - by * gx;
  }
  const int n = bz;
  const int ps = (p.pad - PP) >> 1;
  const int x0 = bx * VL, qy0 = (by * 4 + wave) * T;
  const int qx = x0 + lane - L0;
  const int cl = qx + ps;                      // the column this lane loads: e = 1 (odd padding) / e = 1 via the own value of lane + ... see taps()
  const int col = PP ? cl : cl - 1;            // even padding: the lane loads e = 0 and takes e = 1 from its right neighbour
  const unsigned vo = (col >= 0 && col < p.IW) ? (unsigned)col * 4u : OOB_OFF;
  const unsigned m0 = vo != OOB_OFF ? 0xFFFFFFFFu : 0u;
  unsigned so[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int iy = qy0 + ps - 1 + r;
    so[r] = (iy >= 0 && iy < p.IH) ? (unsigned)(iy * p.IW) * 4u : ROW_OOB;
  }
  const float* sb0 = p.s0 + n * p.ns0;
  const float* sb1 = p.s1 + n * p.ns1;

  auto load_px = [&](int ci, float (&v)[R], float& sc, float& sh) {
    {
      const int ccl = min(ci, p.Cin - 1);
      const bool first = ccl < p.C0;
      const int c2 = first ? ccl : ccl - p.C0;
      const float* scp = first ? p.sc0 : p.sc1;
      const float* shp = first ? p.sh0 : p.sh1;
      const int aidx = n * (first ? p.C0 : p.C1) + c2;
      const bool hsc = scp != nullptr, hsh = shp != nullptr;
      sc = (hsc ? scp : p.ident)[hsc ? aidx : 0];
      sh = (hsh ? shp : p.ident)[hsh ? aidx : 1];
    }
    const bool cok = ci < p.Cin;
    const int cc = cok ? ci : 0;
    const bool first = cc < p.C0;
    const float* base = (first ? sb0 : sb1) + (int64_t)(first ? cc : cc - p.C0) * iplane;
    const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, cok ? iplane * 4 : 0, 0x00020000);
    if (p.ablate & 1) return;
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = ld_buf(rs, vo, so[r]);
  };
  auto load_a = [&](int ci, float (&a)[NB]) {
    const float* src = wl + min(ci, p.Cin - 1) * (NB * 64) + lane;
#pragma unroll
    for (int b = 0; b < NB; ++b) a[b] = src[b * 64];
  };
  auto finish = [&](float (&v)[R], float sc, float sh) {
    if (p.identity_in) return;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const bool rok = so[r] != ROW_OOB;   // uniform
      const float t = fmaf(v[r], rok ? sc : 0.f, rok ? sh : 0.f);
      const float a = fmaxf(t, 0.f) + p.slope_in * fminf(t, 0.f);
      v[r] = and_bits(a, m0);
    }
  };

  f32x4 acc[T][2][2][NB];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int k = 0; k < NB; ++k) acc[t][a][b][k] = (f32x4){0.f, 0.f, 0.f, 0.f};
  auto mm = [&](const float (&aw)[NB], const float (&v)[R]) {
    if (p.ablate & 2) {
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < R; ++r) s += v[r];
      acc[0][0][0][0][0] += s * aw[0];
      return;
    }
    float x[R][ND];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (PP) {
        x[r][0] = from_prev(v[r]);
        x[r][1] = v[r];
        x[r][2] = from_next(v[r]);
      } else {
        x[r][0] = v[r];
        x[r][1] = from_next(v[r]);
      }
    }
    static_for<0, 16>([&](auto tc) {
      constexpr int tap = decltype(tc)::value, ky = tap >> 2, kx = tap & 3;
      constexpr int a = (ky + PP) & 1, b = (kx + PP) & 1;            // the phase this tap feeds ((a + PP) & 1 == ky & 1)
      constexpr int d = (a + PP - ky) / 2 + 1, e = (b + PP - kx) / 2 + 1;
      static_assert(d >= 0 && d < ND && e >= 0 && e < ND, "tap outside the neighbourhood");
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int k = 0; k < NB; ++k) acc[t][a][b][k] = __builtin_amdgcn_mfma_f32_4x4x1f32(aw[k], x[t + d][e], acc[t][a][b][k], 4, tap, 0);
    });
  };

  float va[R] = {}, vb[R] = {};
  float aa[NB], ab[NB];
  float sca, sha, scb, shb;
  load_px(0, va, sca, sha);   // in flight while the weights are staged
  for (int e = tid; e < p.Cin * NB * 64; e += 256) {
    const int l = e & 63, r = e >> 6;
    const int blk = r % NB, ci = r / NB;
    const int co = blk * 4 + (l & 3), tap = l >> 2;
    wl[e] = co < p.Cout ? p.w[(int64_t)co * p.ws_co + (int64_t)ci * p.ws_ci + tap] : 0.f;
  }
  __syncthreads();
  load_a(0, aa);
  for (int ci = 0; ci + 1 < p.Cin; ci += 2) {
    load_px(ci + 1, vb, scb, shb);
    load_a(ci + 1, ab);
    finish(va, sca, sha);
    mm(aa, va);
    load_px(ci + 2, va, sca, sha);
    load_a(ci + 2, aa);
    finish(vb, scb, shb);
    mm(ab, vb);
  }
  if (p.Cin & 1) {
    finish(va, sca, sha);
    mm(aa, va);
  }
  if (p.ablate & 4) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int k = 0; k < NB; ++k) s += acc[t][0][0][k][0] + acc[t][0][1][k][1] + acc[t][1][0][k][2] + acc[t][1][1][k][3];
    if (s == 123.456f) p.out[0] = s;
    return;
  }

  // ---- epilogue: per output row (t, a) and channel one pair (b = 0, 1) per lane.  Branch-free as in conv_px_s2_kernel; an odd output
  // width (the pair of the last column would run into the next row) takes dword accesses instead of 8-byte ones (uniform).
  const int onb = p.Cout * oplane * 4;
  const rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc((void*)(p.out + n * p.ons), 0, onb, 0x00020000);
  const rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.dm ? p.dm + n * p.dmns : p.out), 0, p.dm ? p.dmC * oplane * 4 : 0, 0x00020000);
  const bool lok = lane >= L0 && lane < L0 + VL && qx >= 0;
  const bool ok0 = lok && 2 * qx < p.OW, ok1 = lok && 2 * qx + 1 < p.OW;
  const bool pairs = (p.OW & 1) == 0;   // uniform
  const unsigned vx0 = ok0 ? (unsigned)qx * 8u : OOB_OFF, vx1 = ok1 ? (unsigned)qx * 8u + 4u : OOB_OFF;
  const int slot = by * p.tiles_x + bx;
  const int nvy = min(max(p.OH - 2 * qy0, 0), 2 * T);
  const float cnt = (float)(nvy * min(max(p.OW - 2 * x0, 0), 2 * VL));
  const float* biasp = p.bias ? p.bias : p.ident + 1;
  const float* dscp = (p.dm && p.dmsc) ? p.dmsc + n * p.dmC : p.ident;
  const float* dshp = (p.dm && p.dmsh) ? p.dmsh + n * p.dmC : p.ident + 1;
#pragma unroll
  for (int k = 0; k < NB; ++k) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = k * 4 + i, coc = min(co, p.Cout - 1);
      const float bias = biasp[p.bias ? coc : 0];
      const float dsc = dscp[(p.dm && p.dmsc) ? coc : 0], dsh = dshp[(p.dm && p.dmsh) ? coc : 0];
      unsigned soff[T][2];
      f32x2 dmv[T][2], prev[T][2];
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          const int y = 2 * (qy0 + t) + a;
          soff[t][a] = (co < p.Cout && y < p.OH) ? (unsigned)(co * oplane + y * p.OW) * 4u : ROW_OOB;
          dmv[t][a] = (f32x2){1.f, 1.f};
          prev[t][a] = (f32x2){0.f, 0.f};
        }
      if (p.dm) {
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
          for (int a = 0; a < 2; ++a) {
            if (pairs) dmv[t][a] = ld_buf2(drs, vx0, soff[t][a]);
            else dmv[t][a] = (f32x2){ld_buf(drs, vx0, soff[t][a]), ld_buf(drs, vx1, soff[t][a])};
          }
      }
      if (p.accumulate) {
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
          for (int a = 0; a < 2; ++a) {
            if (pairs) prev[t][a] = ld_buf2(ors, vx0, soff[t][a]);
            else prev[t][a] = (f32x2){ld_buf(ors, vx0, soff[t][a]), ld_buf(ors, vx1, soff[t][a])};
          }
      }
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          const bool rok = soff[t][a] != ROW_OOB;   // uniform
          float o[2];   // (scalars: __builtin_bit_cast of an ext-vector ELEMENT yields element 0 -- the compiler issue noted in DESIGN.md)
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            const bool ok = rok && (b ? ok1 : ok0);
            const float raw = acc[t][a][b][k][i];
            if (STATS == 1) {
              const float m = ok ? raw : 0.f;
              s1 += m;
              s2 = fmaf(m, m, s2);
            }
            float val = raw + bias;
            if (p.tanh_out) val = tanh_fast(val);
            const float tn = fmaf(dmv[t][a][b], dsc, dsh);
            val = fmaf(val, tn > 0.f ? 1.f : p.dm_slope, prev[t][a][b]);
            if (STATS == 2 && ok) {
              s1 += val;
              s2 = fmaf(val, tn, s2);
            }
            o[b] = val;
          }
          if (pairs) {
            const f32x2 o2 = {o[0], o[1]};
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(__attribute__((ext_vector_type(2))) unsigned, o2), ors, (int)vx0, (int)soff[t][a], 0);
          } else {
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o[0]), ors, (int)vx0, (int)soff[t][a], 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o[1]), ors, (int)vx1, (int)soff[t][a], 0);
          }
        }
      if (STATS != 0) {
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        if (lane == 0) {
          float* q = px_stat + (wave * NB * 4 + co) * 3;
          if (STATS == 1) {
            const float mean = s1 / fmaxf(cnt, 1.f);
            q[0] = mean;
            q[1] = fmaxf(s2 - s1 * mean, 0.f);
            q[2] = cnt;
          } else {
            q[0] = s1;
            q[1] = s2;
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);   // one channel at a time
    }
  }
  if (STATS != 0) px_merge_stats<NB, STATS>(px_stat, p, n, slot);
}

template <int NB, int T, int PP>
int pxt_launch_pp(const PxK& k, int N, int stats, hipStream_t st) {
  const dim3 grid(k.tiles_x, k.tiles_y, N), block(256);
  const size_t lds = (size_t)k.Cin * NB * 64 * sizeof(float);
  if (stats == 1) hipLaunchKernelGGL((convt_px_s2_kernel<NB, T, PP, 1>), grid, block, lds, st, k);
  else if (stats == 2) hipLaunchKernelGGL((convt_px_s2_kernel<NB, T, PP, 2>), grid, block, lds, st, k);
  else hipLaunchKernelGGL((convt_px_s2_kernel<NB, T, PP, 0>), grid, block, lds, st, k);
  vts_set_kernel("convt_px_s2_kernel<%d, %d, %d, %d>", NB, T, PP, stats);
  VTS_CHECK_LAUNCH("vts_conv4x4 (transposed, lane = pixel)");
  return VTS_OK;
}
template <int NB, int T>
int pxt_launch(const PxK& k, int N, int stats, hipStream_t st) {
  return (k.pad & 1) ? pxt_launch_pp<NB, T, 1>(k, N, stats, st) : pxt_launch_pp<NB, T, 0>(k, N, stats, st);
}

template <int NB, int T, int PP>
int px_launch_pp(const PxK& k, int N, int stats, hipStream_t st) {
  const dim3 grid(k.tiles_x, k.tiles_y, N), block(256);
  const size_t lds = (size_t)k.Cin * NB * 64 * sizeof(float);
  if (stats == 1) hipLaunchKernelGGL((conv_px_s2_kernel<NB, T, PP, 1>), grid, block, lds, st, k);
  else if (stats == 2) hipLaunchKernelGGL((conv_px_s2_kernel<NB, T, PP, 2>), grid, block, lds, st, k);
  else hipLaunchKernelGGL((conv_px_s2_kernel<NB, T, PP, 0>), grid, block, lds, st, k);
  vts_set_kernel("conv_px_s2_kernel<%d, %d, %d, %d>", NB, T, PP, stats);
  VTS_CHECK_LAUNCH("vts_conv4x4 (lane = pixel)");
  return VTS_OK;
}
template <int NB, int T>
int px_launch(const PxK& k, int N, int stats, hipStream_t st) {
  return (k.padx & 1) ? px_launch_pp<NB, T, 1>(k, N, stats, st) : px_launch_pp<NB, T, 0>(k, N, stats, st);
}

}  // namespace

// VTS_ERR_UNSUPPORTED: not a thin full-size stride-2 convolution, use the other members.  stat_part / bsum_part: epilogue partials wanted
// (at most one of them); *stat_spl = slots per (n, channel) written.
int vts_conv_px_try(const vts_conv_desc* d, hipStream_t st, float* stat_part, float* bsum_part, int64_t part_floats, int* stat_spl) {
  static const int enabled = vts_tune_set("VTS_NO_PX") ? 0 : 1;
  // measured (tools/mb_px.py, profiles/r03d_px_microbench.txt): the 4x4x1 MFMA sustains 11 - 13 cycles per instruction (8 nominal), so
  // the mapping pays while the padding of the 16x16x4 tiles costs more than that: up to 12 output channels (9 -> 10 at 1024^2: 71 -> 64 us,
  // 4 -> 8 / 7 -> 8: 73 -> 54 / 59 -> 41 us, 3 -> 10 with mask: 37 -> 32 us); at 16 - 20 channels conv4x4_kernel is 15 - 30 % faster
  constexpr int max_nb = 3;            // blocks of 4 output channels (16 - 20 channels: 10 -> 20 at 512^2 42 vs 35 us, 8 -> 16 at 513^2 51 vs 37 us on conv4x4_kernel)
  constexpr int min_hw = 128 * 128;    // output pixels (no lower bound: + 0.4 % on the step, round 5)
  const int Cin = d->in0.C + (d->in1.data ? d->in1.C : 0);
  const int nb = (d->Cout + 3) / 4;
  static const int enabled_t = vts_tune_set("VTS_NO_PXT") ? 0 : 1;
  constexpr int max_nb_t = 3;          // (transposed 40 -> 10: 88 vs 62 us on conv4x4_kernel)
  if (d->stride != 2 || d->pad_dx != 0 && d->transposed) return VTS_ERR_UNSUPPORTED;
  // (transposed, measured: 10 -> 3 / 10 -> 2 at 1024^2 42 -> 36 / 41 -> 35 us, 16 -> 8 at 513^2 72 -> 59 us (N 8), 8 -> 4 at 1025^2 62 -> 56 us;
  //  with 9 - 12 output channels only where convt2_thin_kernel was the alternative (10 -> 9: 180 -> 90 us; 40 -> 10: 88 vs 62 us on conv4x4_kernel))
  if (d->transposed ? (!enabled_t || nb > max_nb_t || (nb == 3 && Cin > 10) || d->pad < 0) : (!enabled || nb > max_nb)) return VTS_ERR_UNSUPPORTED;
  if ((int64_t)d->OH * d->OW < min_hw || (int64_t)Cin * nb * 256 > 64 * 1024) return VTS_ERR_UNSUPPORTED;
  if (d->act_in == VTS_ACT_TANH || d->dmask_act == VTS_ACT_TANH) return VTS_ERR_UNSUPPORTED;
  if (d->transposed ? (d->act_out != VTS_ACT_NONE && d->act_out != VTS_ACT_TANH) : d->act_out != VTS_ACT_NONE) return VTS_ERR_UNSUPPORTED;
  if ((int64_t)d->Cout * d->OH * d->OW * 4 >= (int64_t)OOB_OFF || (int64_t)d->IH * d->IW * 4 >= (int64_t)OOB_OFF) return VTS_ERR_UNSUPPORTED;
  if (d->dmask.data && (int64_t)d->dmask.C * d->OH * d->OW * 4 >= (int64_t)OOB_OFF) return VTS_ERR_UNSUPPORTED;
  constexpr int T = 2;
  PxK k;
  k.s0 = d->in0.data; k.sc0 = d->in0.scale; k.sh0 = d->in0.shift; k.ns0 = d->in0.nstride; k.C0 = d->in0.C;
  k.s1 = d->in1.data; k.sc1 = d->in1.scale; k.sh1 = d->in1.shift; k.ns1 = d->in1.nstride;
  k.C1 = d->in1.data ? d->in1.C : 0;
  k.Cin = Cin;
  k.IH = d->IH; k.IW = d->IW; k.OH = d->OH; k.OW = d->OW; k.Cout = d->Cout; k.pad = d->pad; k.padx = d->pad + d->pad_dx;
  k.w = d->w; k.ws_co = d->ws_co; k.ws_ci = d->ws_ci; k.bias = d->bias; k.out = d->out; k.ons = d->out_nstride;
  k.dm = d->dmask.data; k.dmsc = d->dmask.scale; k.dmsh = d->dmask.shift; k.dmns = d->dmask.nstride; k.dm_slope = d->dmask.data ? vts_slope(d->dmask_act) : 1.f; k.dmC = d->dmask.C;
  k.tanh_out = d->act_out == VTS_ACT_TANH;
  k.accumulate = d->accumulate;
  k.N = d->N;
  k.ident = vts_ident();
  VTS_CHECK_ARG(k.ident, "vts_conv4x4: could not allocate the identity constants");
  k.slope_in = vts_slope(d->act_in);
  k.identity_in = (d->act_in == VTS_ACT_NONE && !d->in0.scale && !d->in0.shift && !(d->in1.data && (d->in1.scale || d->in1.shift))) ? 1 : 0;
  k.xcd_swizzle = 1;   // XCD-aware workgroup order (the hardware order measured + 0.5 % on the step, round 5)
  static const int ablate = vts_tune("VTS_ABLATE", 0);
  k.ablate = ablate;
  int Tt = 0;
  if (d->transposed) {   // tiles of the low-resolution grid
    const int QH = (d->OH + 1) / 2, QW = (d->OW + 1) / 2;
    Tt = nb <= 2 ? 2 : 1;
    k.tiles_x = cdiv(QW, (d->pad & 1) ? 62 : 63);
    k.tiles_y = cdiv(QH, 4 * Tt);
  } else {
    k.tiles_x = cdiv(d->OW, (k.padx & 1) ? 62 : 63);
    k.tiles_y = cdiv(d->OH, 4 * T);
  }
  k.stat_spl = k.tiles_x * k.tiles_y;      // one slot per workgroup tile (round 4; one per wave before)
  int stats = 0;
  k.stat_part = nullptr; k.bsum_part = nullptr;
  if (stat_part || bsum_part) {
    const int64_t need = (int64_t)d->N * d->Cout * k.stat_spl * (stat_part ? 3 : 2);
    if (part_floats >= need) {
      stats = stat_part ? 1 : 2;
      k.stat_part = stat_part; k.bsum_part = bsum_part;
    }
  }
  if (stat_spl) *stat_spl = stats ? k.stat_spl : 0;
  if (d->transposed) {
    switch (nb) {
      case 1: return pxt_launch<1, 2>(k, d->N, stats, st);
      case 2: return pxt_launch<2, 2>(k, d->N, stats, st);
      default: return pxt_launch<3, 1>(k, d->N, stats, st);
    }
  }
  switch (nb) {
    case 1: return px_launch<1, 2>(k, d->N, stats, st);
    case 2: return px_launch<2, 2>(k, d->N, stats, st);
    default: return px_launch<3, 2>(k, d->N, stats, st);
  }
}
