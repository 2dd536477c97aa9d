// Network-level entry point (`vts_unet_fwd`): the inference forward of the reference's generator
//   CustomUnetGenerator.forward   models/networks.py:1430-1645
//   Down / Up                     thirdparty/unet/unet_parts_custom.py:9-37, 40-79
// as ONE C call over the library's own operators, for hosts that are not Python (the Python product drives the same operators from
// vts/engine.py:unet_forward, which also keeps what a backward needs; the two produce bit-identical outputs:
// tests/test_network_abi_gpu.py).  The schedule:
//   down_i (i = 0 .. nd-1)   [LeakyReLU(0.2) ->] Conv2d(4, 2, 1) [-> InstanceNorm2d]     (down0: convolution only; the innermost: no norm)
//   up_i   (i = nd-1 .. 0)   ReLU -> ConvTranspose2d(4, 2, 1) on cat(x, skip_i) [-> InstanceNorm2d]; up0: Tanh
//   layers nls-1 .. 0 exist twice (visual branch / tactile branch `_T`), both fed by up_nls's output
// Nothing is materialised between the layers but the RAW convolution outputs: LeakyReLU / ReLU, the InstanceNorm scale / shift and the
// skip concatenation are applied by the consuming convolution on load (vts_conv4x4's operand pairs), the statistics come out of the
// producing convolution's epilogue (vts_conv4x4_norm).  No allocation: the caller passes vts_unet_forward_ws_floats(d) floats.
#include <stdint.h>

#include <algorithm>

#include "vts_internal.h"

#define VTS_CHECK_HIP(x)                                                        \
  do {                                                                         \
    hipError_t e__ = (x);                                                      \
    if (e__ != hipSuccess) {                                                   \
      vts_set_error("vts_unet_forward: %s: %s", #x, hipGetErrorString(e__));   \
      return VTS_ERR_LAUNCH;                                                   \
    }                                                                          \
  } while (0)

namespace {

struct Plan {
  int64_t act_off[VTS_UNET_MAX_DOWNS];     // raw encoder outputs
  int64_t upact_off[2][VTS_UNET_MAX_DOWNS];  // raw decoder outputs per branch (layer 0 writes d->out)
  int64_t stat_off[3][VTS_UNET_MAX_DOWNS];   // [4][N*C] scale, shift, mean, rstd: encoder, decoder branch 0 / 1
  int64_t conv_ws[2], conv_ws_floats;      // k-split partials / stand-alone statistics scratch (never live together), one per lane
  int64_t stat_ws[2], stat_ws_floats;      // epilogue statistics partials, one per lane
  int64_t total;
};

int up_cout(const vts_unet_desc* d, int branch, int i) { return branch ? d->upT_cout[i] : d->up_cout[i]; }

// the convolution descriptors of the schedule, in launch order: shared by the workspace planner and the launcher
struct Layer {
  vts_conv_desc c;
  bool normed;
  int C;                  // output channels
  int64_t stat;           // offset of its statistics block (normed)
  int lane;               // 1: a layer of the tactile branch (runs on d->side_stream when given)
};

int build(const vts_unet_desc* d, float* ws, const Plan& P, Layer* L, int* count) {
  const int nd = d->num_downs, nls = d->num_layer_separate;
  const int N = d->N;
  int n = 0;
  auto stats_operand = [&](float* data, int C, int64_t hw, int64_t stat_off, bool normed) {
    vts_operand o{};
    o.data = data; o.C = C; o.nstride = (int64_t)C * hw;
    if (normed) { o.scale = ws + stat_off; o.shift = ws + stat_off + (int64_t)N * C; }
    return o;
  };
  vts_operand feat[VTS_UNET_MAX_DOWNS];
  for (int i = 0; i < nd; ++i) {
    Layer& l = L[n++];
    l = Layer{};
    const int oh = d->H >> (i + 1), ow = d->W >> (i + 1);
    vts_conv_desc& c = l.c;
    if (i == 0) { c.in0 = d->in0; c.in1 = d->in1; } else c.in0 = feat[i - 1];
    const int cin = c.in0.C + c.in1.C;
    c.N = N; c.IH = d->H >> i; c.IW = d->W >> i; c.OH = oh; c.OW = ow; c.Cout = d->channels[i];
    c.stride = 2; c.pad = 1; c.transposed = 0;
    c.w = d->down_w[i]; c.ws_co = cin * 16; c.ws_ci = 16; c.bias = d->down_b[i];
    c.out = ws + P.act_off[i]; c.out_nstride = (int64_t)c.Cout * oh * ow;
    c.act_in = i ? VTS_ACT_LRELU : VTS_ACT_NONE; c.act_out = VTS_ACT_NONE;
    l.normed = i > 0 && i < nd - 1; l.C = c.Cout; l.stat = P.stat_off[0][i];
    feat[i] = stats_operand(c.out, c.Cout, (int64_t)oh * ow, l.stat, l.normed);
  }
  const int out_c = d->up_cout[0] + (nls > 0 ? d->upT_cout[0] : 0);
  vts_operand trunk = feat[nd - 1];
  for (int branch = 0; branch < (nls > 0 ? 2 : 1); ++branch) {
    vts_operand x = trunk;
    // branch 0 walks the shared trunk (nd-1 .. nls) and then its own layers; branch 1 only its own layers, from the trunk's end
    for (int i = (branch ? nls - 1 : nd - 1); i >= 0; --i) {
      Layer& l = L[n++];
      l = Layer{};
      const int ih = d->H >> (i + 1), iw = d->W >> (i + 1);
      const bool own = i < nls;
      const int b = own ? branch : 0;
      vts_conv_desc& c = l.c;
      c.in0 = x;
      if (i != 0 && i != nd - 1) c.in1 = feat[i];                 // skip connection: torch.cat([x, skip], 1)
      else if (i == nd - 1 && d->style.C > 0) c.in1 = d->style;   // the tiled style code enters at the innermost block
      const int cout = up_cout(d, b, i);
      c.N = N; c.IH = ih; c.IW = iw; c.OH = 2 * ih; c.OW = 2 * iw; c.Cout = cout;
      c.stride = 2; c.pad = 1; c.transposed = 1;
      c.w = b ? d->upT_w[i] : d->up_w[i]; c.ws_co = 16; c.ws_ci = cout * 16; c.bias = b ? d->upT_b[i] : d->up_b[i];
      if (i == 0) {
        c.out = d->out + (b ? (int64_t)d->up_cout[0] * d->H * d->W : 0); c.out_nstride = (int64_t)out_c * d->H * d->W;
      } else {
        c.out = ws + P.upact_off[b][i]; c.out_nstride = (int64_t)cout * c.OH * c.OW;
      }
      c.act_in = VTS_ACT_RELU; c.act_out = i == 0 ? VTS_ACT_TANH : VTS_ACT_NONE;
      l.normed = i != 0; l.C = cout; l.stat = P.stat_off[1 + b][i]; l.lane = branch;
      x = stats_operand(c.out, cout, (int64_t)c.OH * c.OW, l.stat, l.normed);
      if (!branch && i == nls) trunk = x;
    }
  }
  *count = n;
  return VTS_OK;
}

int check(const vts_unet_desc* d) {
  VTS_CHECK_ARG(d, "vts_unet_forward: null descriptor");
  const int nd = d->num_downs, nls = d->num_layer_separate;
  VTS_CHECK_ARG(nd >= 2 && nd <= VTS_UNET_MAX_DOWNS && nls >= 0 && nls < nd, "vts_unet_forward: num_downs %d / num_layer_separate %d", nd, nls);
  VTS_CHECK_ARG(d->N >= 1 && d->H >= 1 && d->W >= 1 && d->H % (1 << nd) == 0 && d->W % (1 << nd) == 0,
                "vts_unet_forward: H, W must be divisible by %d, got %dx%d", 1 << nd, d->H, d->W);
  VTS_CHECK_ARG(d->in0.data && d->in0.C >= 1 && (d->in1.C == 0 || d->in1.data) && d->out, "vts_unet_forward: null input / output");
  for (int i = 0; i < nd; ++i) {
    VTS_CHECK_ARG(d->channels[i] >= 1 && d->down_w[i] && d->up_w[i] && d->up_cout[i] >= 1, "vts_unet_forward: layer %d incomplete", i);
    VTS_CHECK_ARG(i >= nls || (d->upT_w[i] && d->upT_cout[i] >= 1), "vts_unet_forward: tactile branch layer %d incomplete", i);
    // the decoder mirrors the encoder: up_i's input is cat(up_{i+1} output, skip_i)
    VTS_CHECK_ARG(i == 0 || d->up_cout[i] == d->channels[i - 1], "vts_unet_forward: up%d emits %d channels, down%d has %d", i, d->up_cout[i], i - 1,
                  d->channels[i - 1]);
    VTS_CHECK_ARG(i == 0 || i >= nls || d->upT_cout[i] == d->channels[i - 1], "vts_unet_forward: up%d_T emits %d channels, down%d has %d", i,
                  d->upT_cout[i], i - 1, d->channels[i - 1]);
  }
  VTS_CHECK_ARG(d->style.C == 0 || d->style.data, "vts_unet_forward: style operand without data");
  return VTS_OK;
}

int plan(const vts_unet_desc* d, Plan& P) {
  const int nd = d->num_downs, nls = d->num_layer_separate;
  const int64_t N = d->N;
  int64_t off = 0;
  auto take = [&](int64_t n) { const int64_t o = off; off += (n + 63) / 64 * 64; return o; };
  for (int i = 0; i < nd; ++i) {
    const int64_t hw = (int64_t)(d->H >> (i + 1)) * (d->W >> (i + 1));
    P.act_off[i] = take(N * d->channels[i] * hw);
    P.stat_off[0][i] = take(4 * N * d->channels[i]);
  }
  for (int b = 0; b < 2; ++b)
    for (int i = 1; i < nd; ++i) {
      P.upact_off[b][i] = P.stat_off[1 + b][i] = 0;
      if (b && i >= nls) continue;
      const int64_t hw = (int64_t)(d->H >> i) * (d->W >> i);
      const int c = up_cout(d, b, i);
      P.upact_off[b][i] = take(N * c * hw);
      P.stat_off[1 + b][i] = take(4 * N * c);
    }
  P.upact_off[0][0] = P.upact_off[1][0] = P.stat_off[1][0] = P.stat_off[2][0] = 0;
  // scratch: sized over the schedule's descriptors (built against a null workspace: only shapes matter)
  Layer L[3 * VTS_UNET_MAX_DOWNS];
  int n = 0;
  build(d, reinterpret_cast<float*>(uintptr_t(4096)), P, L, &n);    // (a placeholder base: only the shapes are read)
  int64_t cw = 0, sw = 0;
  for (int k = 0; k < n; ++k) {
    const vts_conv_desc& c = L[k].c;
    if ((int64_t)c.OH * c.OW <= 64 * 64) cw = std::max(cw, vts_conv4x4_ws_floats(&c));
    if (L[k].normed) {
      sw = std::max(sw, vts_conv4x4_norm_ws_floats(&c));
      cw = std::max(cw, vts_norm_ws_floats(c.N, c.Cout, c.OH * c.OW));
    }
  }
  P.conv_ws_floats = cw; P.stat_ws_floats = sw;
  for (int lane = 0; lane < 2; ++lane) {
    P.conv_ws[lane] = take(cw);
    P.stat_ws[lane] = take(sw);
  }
  P.total = off;
  return VTS_OK;
}

}  // namespace

extern "C" int64_t vts_unet_forward_ws_floats(const vts_unet_desc* d) {
  if (check(d) != VTS_OK) return -1;
  Plan P{};
  plan(d, P);
  return P.total;
}

// fork / join events of the two-lane form (created once per host thread; recorded and waited on inside the caller's stream order, so the
// call stays capturable into a HIP graph)
// (set 0: the forward, set 1: the backward -- a graph that captures both records each pair once)
static int lane_events(hipEvent_t* fork, hipEvent_t* join, int set = 0) {
  static thread_local hipEvent_t ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  if (!ev[set][0]) {
    VTS_CHECK_HIP(hipEventCreateWithFlags(&ev[set][0], hipEventDisableTiming));
    VTS_CHECK_HIP(hipEventCreateWithFlags(&ev[set][1], hipEventDisableTiming));
  }
  *fork = ev[set][0]; *join = ev[set][1];
  return VTS_OK;
}

extern "C" int vts_unet_forward(const vts_unet_desc* d, float* ws, int64_t ws_floats, void* stream) {
  const int rc0 = check(d);
  if (rc0 != VTS_OK) return rc0;
  Plan P{};
  plan(d, P);
  VTS_CHECK_ARG(ws && ws_floats >= P.total, "vts_unet_forward: workspace of %lld floats, need %lld", (long long)ws_floats, (long long)P.total);
  Layer L[3 * VTS_UNET_MAX_DOWNS];
  int n = 0;
  build(d, ws, P, L, &n);
  const bool lanes = d->side_stream && d->side_stream != stream && d->num_layer_separate > 0;
  hipEvent_t fork = nullptr, join = nullptr;
  if (lanes) {
    const int rc = lane_events(&fork, &join);
    if (rc != VTS_OK) return rc;
  }
  bool forked = false;
  // an error after the fork still joins the side stream (inside a graph capture a dangling fork invalidates the capture; outside, the
  // side stream would be left unordered with the caller's stream)
  auto finish = [&](int rc) {
    if (forked && (hipEventRecord(join, (hipStream_t)d->side_stream) != hipSuccess || hipStreamWaitEvent((hipStream_t)stream, join, 0) != hipSuccess) && rc == VTS_OK) {
      vts_set_error("vts_unet_forward: joining the side stream failed");
      return (int)VTS_ERR_LAUNCH;
    }
    return rc;
  };
  for (int k = 0; k < n; ++k) {
    vts_conv_desc& c = L[k].c;
    // the visual branch's own layers follow the trunk on `stream`; the tactile branch (all at the end of the list) runs on the side
    // stream from the trunk's last layer on.  The fork is recorded when the first own layer of the visual branch is reached.
    const bool own0 = lanes && !forked && k >= d->num_downs + (d->num_downs - d->num_layer_separate);
    if (own0) {
      VTS_CHECK_HIP(hipEventRecord(fork, (hipStream_t)stream));
      forked = true;
      if (hipStreamWaitEvent((hipStream_t)d->side_stream, fork, 0) != hipSuccess) {
        forked = false;
        vts_set_error("vts_unet_forward: forking the side stream failed");
        return VTS_ERR_LAUNCH;
      }
    }
    const int lane = lanes ? L[k].lane : 0;
    void* st = lane ? d->side_stream : stream;
    if ((int64_t)c.OH * c.OW <= 64 * 64) { c.ws = ws + P.conv_ws[lane]; c.ws_floats = P.conv_ws_floats; }
    if (!L[k].normed) {
      const int rc = vts_conv4x4(&c, st);
      if (rc != VTS_OK) return finish(rc);
      continue;
    }
    vts_norm_desc nd{};
    const int64_t NC = (int64_t)c.N * L[k].C;
    float* stt = ws + L[k].stat;
    nd.x = c.out; nd.nstride = c.out_nstride; nd.N = c.N; nd.C = L[k].C; nd.HW = c.OH * c.OW; nd.mode = 0;
    nd.eps = 1e-5f; nd.momentum = 0.1f;          // nn.InstanceNorm2d defaults (models/networks.py:139)
    nd.scale = stt; nd.shift = stt + NC; nd.mean_out = stt + 2 * NC; nd.rstd_out = stt + 3 * NC;
    int fused = 0;
    int rc = vts_conv4x4_norm(&c, &nd, ws + P.stat_ws[lane], P.stat_ws_floats, &fused, st);
    if (rc != VTS_OK) return finish(rc);
    if (fused >= 2) rc = vts_norm_stats_from_partials(&nd, ws + P.stat_ws[lane], fused - 2, st);
    else if (fused == 0) rc = vts_norm_stats(&nd, ws + P.conv_ws[lane], st);
    if (rc != VTS_OK) return finish(rc);
  }
  return finish(VTS_OK);
}

// ---- the backward (`vts_unet_bwd`): vts/engine.py:_unet_backward / _unet_backward_encoder as one call ---------------------
// Reads the forward's Plan region of `ws` (raw outputs, statistics); everything the backward itself needs is carved out behind it, one
// region per buffer and per launch (gradient maps, k-split / statistics scratch, epilogue sums, weight-gradient partials), so nothing is
// shared between the two lanes and the region list is the same in the sizing pass and in the launching pass.  The schedule:
//   decoder lanes  lane b = 0 (visual, `stream`) / 1 (tactile, side stream): up_i / up_i_T for i = 0 .. nls-1, each lane into its own
//                  buffers; then their two contributions to the shared tensors (the skip features 1 .. nls-1, the gradient w.r.t. the
//                  trunk's output) are summed as engine.py's total(a, b): vts_pad_affine(a, res = b)
//   trunk          up_i for i = nls .. nd-1
//   encoder        down_i for i = nd-1 .. 0
//   one vts_wgrad_reduce_batch over the deferred weight-gradient partials of all of them
// Per up block (engine.py:up_bwd): InstanceNorm backward of the output gradient (skipped where the producing convolution's k-split
// epilogue applied it, vts_norm_bwd_from_partials where its tiled epilogue left the sums), the deferred weight gradient on
// cat(input, skip | style), the bias gradient of the outermost block, the backward-data convolution into the input's gradient with
// bwd_sums "in" (not at the innermost block nor at the split point i == nls-1, where the two lanes' parts are summed first), and the
// skip feature's gradient through the skip slice of the weight.
namespace {

struct Bwd {
  const vts_unet_desc* d;
  const vts_unet_grads* g;
  float* ws;
  const Plan* P;
  const Layer* L;
  bool dry;                         // sizing pass: regions are taken, nothing is launched
  int64_t off;
  vts_reduce_job jobs[3 * VTS_UNET_MAX_DOWNS];
  int njobs;

  float* take(int64_t n) {
    float* p = ws + off;
    off += (n + 63) / 64 * 64;
    return p;
  }
};

// a gradient map and what its producing convolution left for the normalisation backward that reads it next
struct Grad {
  float* data;
  int C;
  int64_t nstride;
  int slots;                        // -1: InstanceNorm backward already applied; > 0: epilogue sums in `part`; 0: none
  float* part;
};

vts_operand plain(const float* p, int C, int64_t nstride) {
  vts_operand o{};
  o.data = p; o.C = C; o.nstride = nstride;
  return o;
}

int64_t hw_at(const vts_unet_desc* d, int s) { return (int64_t)(d->H >> s) * (d->W >> s); }

// InstanceNorm2d backward of g in place, against the layer output x (raw) with statistics block `stat` (engine.py / ops.norm_bwd)
int norm_bwd_in(Bwd& B, Grad& g, const float* x, int64_t x_nstride, int HW, const float* stat, void* st) {
  const int64_t NC = (int64_t)B.d->N * g.C;
  vts_norm_bwd_desc nb{};
  nb.dy = g.data; nb.x = x; nb.nstride = x_nstride; nb.N = B.d->N; nb.C = g.C; nb.HW = HW; nb.mode = 0;
  nb.mean = stat + 2 * NC; nb.rstd = stat + 3 * NC; nb.ngroups = 1;
  float* nws = B.take(vts_norm_ws_floats(B.d->N, g.C, HW));
  if (B.dry) return VTS_OK;
  const int slots = g.slots;
  g.slots = 0;
  if (slots == -1) return VTS_OK;
  if (slots > 0) return vts_norm_bwd_from_partials(&nb, g.part, slots, nullptr, st);
  return vts_norm_bwd(&nb, nws, st);
}

// the backward-data convolution (vts_conv4x4 / with bwd_sums "in": vts_conv4x4_bsums), k-split scratch for small maps
int conv_bwd(Bwd& B, vts_conv_desc& c, bool bsums, Grad* out, void* st) {
  if ((int64_t)c.OH * c.OW <= 64 * 64) {
    c.ws_floats = vts_conv4x4_ws_floats(&c);
    c.ws = B.take(c.ws_floats);
  }
  if (!bsums) {
    if (out) out->slots = 0;
    return B.dry ? VTS_OK : vts_conv4x4(&c, st);
  }
  const int64_t pf = vts_conv4x4_norm_ws_floats(&c);
  float* part = B.take(pf);
  if (B.dry) return VTS_OK;
  int slots = -1;                   // the normalisation behind `out` is InstanceNorm2d(affine=False)
  const int rc = vts_conv4x4_bsums(&c, part, pf, &slots, st);
  out->slots = slots; out->part = part;
  return rc;
}

// deferred weight gradient: partials into a region of their own, one reduce job
int wgrad(Bwd& B, vts_wgrad_desc& w, void* st) {
  w.defer = 1; w.accumulate = 0;
  const int64_t n = vts_wgrad4x4_ws_floats(&w);
  float* part = B.take(n);
  const int64_t nel = (int64_t)(w.lo0.C + w.lo1.C) * (w.hi0.C + w.hi1.C) * 16;
  if (B.dry) return VTS_OK;
  vts_reduce_job& j = B.jobs[B.njobs++];
  j = vts_reduce_job{};
  j.dw = w.dw; j.nel = nel; j.accumulate = 0; j.nseg = 1; j.part[0] = part; j.pw[0] = (int)(n / nel);
  return vts_wgrad4x4(&w, part, st);
}

int bias_sum(Bwd& B, const Grad& g, int HW, float* db, void* st) {
  float* cws = B.take(vts_channel_sum_ws_floats(B.d->N, g.C, HW));
  if (B.dry || !db) return VTS_OK;
  return vts_channel_sum(g.data, g.nstride, B.d->N, g.C, HW, db, 0, cws, nullptr, st);
}

// engine.py:up_bwd for block i of branch b: gin = gradient w.r.t. the block's output (normalised for i > 0), into `tin` (gradient w.r.t.
// the block's input) and `tskip` (w.r.t. its skip feature)
int up_bwd(Bwd& B, int b, int i, Grad& gin, Grad* tin, Grad* tskip, bool bsums, void* st) {
  const vts_unet_desc* d = B.d;
  const int nd = d->num_downs, nls = d->num_layer_separate;
  const Layer& l = B.L[b ? 2 * nd + (nls - 1 - i) : nd + (nd - 1 - i)];
  const vts_conv_desc& f = l.c;     // the forward convolution of this block
  const int cout = l.C;
  const int ohw = f.OH * f.OW;
  int rc;
  if (i != 0 && (rc = norm_bwd_in(B, gin, f.out, f.out_nstride, ohw, B.ws + l.stat, st)) != VTS_OK) return rc;
  vts_wgrad_desc w{};
  w.lo0 = f.in0; w.lo1 = f.in1; w.hi0 = plain(gin.data, cout, gin.nstride);
  w.act_lo = VTS_ACT_RELU; w.act_hi = VTS_ACT_NONE;
  w.N = d->N; w.LH = f.IH; w.LW = f.IW; w.HH = f.OH; w.HW = f.OW; w.stride = 2; w.pad = 1;
  w.dw = b ? B.g->upT_dw[i] : B.g->up_dw[i];
  if ((rc = wgrad(B, w, st)) != VTS_OK) return rc;
  if (i == 0 && (rc = bias_sum(B, gin, ohw, b ? B.g->upT_db[0] : B.g->up_db[0], st)) != VTS_OK) return rc;
  const int cin0 = f.in0.C;
  vts_conv_desc c{};
  c.in0 = plain(gin.data, cout, gin.nstride);
  c.N = d->N; c.IH = f.OH; c.IW = f.OW; c.OH = f.IH; c.OW = f.IW; c.Cout = cin0;
  c.stride = 2; c.pad = 1; c.transposed = 0;
  c.w = f.w; c.ws_co = cout * 16; c.ws_ci = 16;
  c.out = tin->data; c.out_nstride = tin->nstride;
  c.dmask = f.in0; c.dmask_act = VTS_ACT_RELU;
  if ((rc = conv_bwd(B, c, bsums, tin, st)) != VTS_OK) return rc;
  if (i != 0 && i != nd - 1) {      // the skip connection: its slice of the weight, into the skip feature's gradient
    vts_conv_desc s = c;
    s.ws = nullptr; s.ws_floats = 0;
    s.w = f.w + (int64_t)cin0 * cout * 16; s.Cout = f.in1.C;
    s.out = tskip->data; s.out_nstride = tskip->nstride;
    s.dmask = f.in1;
    if ((rc = conv_bwd(B, s, false, tskip, st)) != VTS_OK) return rc;
  }
  return VTS_OK;
}

int bwd_check(const vts_unet_desc* d, const vts_unet_grads* g) {
  const int rc = check(d);
  if (rc != VTS_OK) return rc;
  VTS_CHECK_ARG(g, "vts_unet_backward: null gradient struct");
  VTS_CHECK_ARG(g->d_raw, "vts_unet_backward: null d_raw");
  const int nd = d->num_downs, nls = d->num_layer_separate;
  const int out_c = d->up_cout[0] + (nls > 0 ? d->upT_cout[0] : 0);
  VTS_CHECK_ARG(g->d_raw_nstride == 0 || g->d_raw_nstride >= (int64_t)out_c * d->H * d->W, "vts_unet_backward: d_raw_nstride %lld below %d x %d x %d",
                (long long)g->d_raw_nstride, out_c, d->H, d->W);
  for (int i = 0; i < nd; ++i) {
    VTS_CHECK_ARG(g->down_dw[i] && (!d->down_b[i] || g->down_db[i]), "vts_unet_backward: down%d gradient missing (down_dw / down_db[%d])", i, i);
    VTS_CHECK_ARG(g->up_dw[i] && (!d->up_b[i] || g->up_db[i]), "vts_unet_backward: up%d gradient missing (up_dw / up_db[%d])", i, i);
    VTS_CHECK_ARG(i >= nls || (g->upT_dw[i] && (!d->upT_b[i] || g->upT_db[i])), "vts_unet_backward: up%d_T gradient missing (upT_dw / upT_db[%d])", i, i);
    // the grid of vts_pad_affine (the lanes' sum) carries (n, c) in 16 bits
    VTS_CHECK_ARG((int64_t)d->N * d->channels[i] <= 65535, "vts_unet_backward: N x channels[%d] = %lld above 65535", i, (long long)d->N * d->channels[i]);
  }
  return VTS_OK;
}

// the whole schedule; `sync` = (fork, join) events when the tactile lane runs on the side stream
int run_bwd(Bwd& B, void* stream, void* side, hipEvent_t fork, hipEvent_t join) {
  const vts_unet_desc* d = B.d;
  const vts_unet_grads* g = B.g;
  const int nd = d->num_downs, nls = d->num_layer_separate;
  const int N = d->N;
  auto map = [&](int i) {           // a gradient buffer shaped like feats[i] / the input of up_i: [N][channels[i]][H >> (i+1)][W >> (i+1)]
    Grad r{};
    r.C = d->channels[i]; r.nstride = (int64_t)r.C * hw_at(d, i + 1);
    r.data = B.take(N * r.nstride);
    return r;
  };
  Grad dfeat[VTS_UNET_MAX_DOWNS], dxs[VTS_UNET_MAX_DOWNS], dxl[2][VTS_UNET_MAX_DOWNS], dfl[2][VTS_UNET_MAX_DOWNS];
  for (int i = 0; i < nd; ++i) {
    dfeat[i] = map(i);
    dxs[i] = i < nd - 1 ? map(i) : Grad{};
    for (int b = 0; b < 2; ++b) {
      dxl[b][i] = i < nls ? map(i) : Grad{};
      dfl[b][i] = (i > 0 && i < nls) ? map(i) : Grad{};
    }
  }
  const int out_c = d->up_cout[0] + (nls > 0 ? d->upT_cout[0] : 0);
  const int64_t raw_ns = g->d_raw_nstride ? g->d_raw_nstride : (int64_t)out_c * d->H * d->W;
  int rc;
  // biases in front of an InstanceNorm: exact zeros (every gradient pointer is overwritten)
  if (!B.dry) {
    bool ok = true;
    auto zero = [&](float* p, int n) { ok = ok && (!p || hipMemsetAsync(p, 0, sizeof(float) * n, (hipStream_t)stream) == hipSuccess); };
    for (int i = 1; i < nd; ++i) {
      if (i < nd - 1) zero(g->down_db[i], d->channels[i]);
      zero(g->up_db[i], d->up_cout[i]);
      if (i < nls) zero(g->upT_db[i], d->upT_cout[i]);
    }
    if (!ok) {
      vts_set_error("vts_unet_backward: zeroing the bias gradients failed");
      return VTS_ERR_LAUNCH;
    }
  }
  // decoder lanes: lane 1 (tactile) first on the side stream, then lane 0 on `stream` (engine.py:_run_lanes)
  auto lane = [&](int b, void* st) {
    for (int i = 0; i < nls; ++i) {
      Grad gin{};
      if (i == 0) {
        gin.data = const_cast<float*>(g->d_raw) + (b ? (int64_t)d->up_cout[0] * d->H * d->W : 0);
        gin.C = b ? d->upT_cout[0] : d->up_cout[0]; gin.nstride = raw_ns;
      } else {
        gin = dxl[b][i - 1];
      }
      const int r = up_bwd(B, b, i, gin, &dxl[b][i], &dfl[b][i], i != nls - 1, st);
      if (r != VTS_OK) return r;
      if (i > 0) dxl[b][i - 1] = gin;
    }
    return (int)VTS_OK;
  };
  bool forked = false;
  auto finish = [&](int r) {
    if (forked && (hipEventRecord(join, (hipStream_t)side) != hipSuccess || hipStreamWaitEvent((hipStream_t)stream, join, 0) != hipSuccess) && r == VTS_OK) {
      vts_set_error("vts_unet_backward: joining the side stream failed");
      return (int)VTS_ERR_LAUNCH;
    }
    return r;
  };
  if (nls > 0) {
    if (side && !B.dry) {
      if (hipEventRecord(fork, (hipStream_t)stream) != hipSuccess || hipStreamWaitEvent((hipStream_t)side, fork, 0) != hipSuccess) {
        vts_set_error("vts_unet_backward: forking the side stream failed");
        return VTS_ERR_LAUNCH;
      }
      forked = true;
    }
    if ((rc = lane(1, side ? side : stream)) != VTS_OK) return finish(rc);
    if ((rc = lane(0, stream)) != VTS_OK) return finish(rc);
    if ((rc = finish(VTS_OK)) != VTS_OK) return rc;
    forked = false;
    // total(a, b) = a + b into the shared buffers (ops.pad_affine with res)
    auto total = [&](const Grad& a, const Grad& bb, Grad& dst, int s) {
      if (B.dry) return (int)VTS_OK;
      vts_operand o = plain(a.data, a.C, a.nstride);
      dst.slots = 0;
      return vts_pad_affine(&o, N, d->H >> s, d->W >> s, 0, 0, 0, 0, 0, VTS_ACT_NONE, bb.data, dst.data, 0, stream);
    };
    for (int i = 1; i < nls; ++i)
      if ((rc = total(dfl[0][i], dfl[1][i], dfeat[i], i + 1)) != VTS_OK) return rc;
    if ((rc = total(dxl[0][nls - 1], dxl[1][nls - 1], dxs[nls - 1], nls)) != VTS_OK) return rc;
  }
  // the shared trunk (everything when nls == 0)
  for (int i = nls; i < nd; ++i) {
    Grad gin{};
    if (i == 0) {
      gin.data = const_cast<float*>(g->d_raw); gin.C = d->up_cout[0]; gin.nstride = raw_ns;
    } else {
      gin = dxs[i - 1];
    }
    Grad* tin = i == nd - 1 ? &dfeat[nd - 1] : &dxs[i];
    if ((rc = up_bwd(B, 0, i, gin, tin, &dfeat[i], i != nd - 1 && !(nls > 0 && i == nls - 1), stream)) != VTS_OK) return rc;
    if (i > 0) dxs[i - 1] = gin;
  }
  // the encoder
  for (int i = nd - 1; i >= 0; --i) {
    const Layer& l = B.L[i];
    const vts_conv_desc& f = l.c;
    Grad& gi = dfeat[i];
    const int ohw = f.OH * f.OW;
    if (l.normed && (rc = norm_bwd_in(B, gi, f.out, f.out_nstride, ohw, B.ws + l.stat, stream)) != VTS_OK) return rc;
    vts_wgrad_desc w{};
    w.lo0 = plain(gi.data, gi.C, gi.nstride); w.hi0 = f.in0; w.hi1 = f.in1;
    w.act_lo = VTS_ACT_NONE; w.act_hi = i ? VTS_ACT_LRELU : VTS_ACT_NONE;
    w.N = N; w.LH = f.OH; w.LW = f.OW; w.HH = f.IH; w.HW = f.IW; w.stride = 2; w.pad = 1;
    w.dw = g->down_dw[i];
    if ((rc = wgrad(B, w, stream)) != VTS_OK) return rc;
    if (!l.normed && (rc = bias_sum(B, gi, ohw, g->down_db[i], stream)) != VTS_OK) return rc;
    if (i > 0) {
      vts_conv_desc c{};
      c.in0 = plain(gi.data, gi.C, gi.nstride);
      c.N = N; c.IH = f.OH; c.IW = f.OW; c.OH = f.IH; c.OW = f.IW; c.Cout = f.in0.C;
      c.stride = 2; c.pad = 1; c.transposed = 1;
      c.w = f.w; c.ws_co = 16; c.ws_ci = f.in0.C * 16;
      c.out = dfeat[i - 1].data; c.out_nstride = dfeat[i - 1].nstride;
      c.dmask = f.in0; c.dmask_act = VTS_ACT_LRELU;
      c.accumulate = i - 1 > 0;     // dfeat[i-1] already holds the skip contribution of up_{i-1}
      if ((rc = conv_bwd(B, c, i - 1 > 0, &dfeat[i - 1], stream)) != VTS_OK) return rc;
    }
  }
  if (B.dry) return VTS_OK;
  return vts_wgrad_reduce_batch(B.jobs, B.njobs, stream);
}

int64_t bwd_total(const vts_unet_desc* d, const vts_unet_grads* g, const Plan& P) {
  Layer L[3 * VTS_UNET_MAX_DOWNS];
  int n = 0;
  float* base = reinterpret_cast<float*>(uintptr_t(4096));
  build(d, base, P, L, &n);
  Bwd B{};
  B.d = d; B.g = g; B.ws = base; B.P = &P; B.L = L; B.dry = true; B.off = P.total;
  run_bwd(B, nullptr, nullptr, nullptr, nullptr);
  return B.off;
}

}  // namespace

extern "C" int64_t vts_unet_backward_ws_floats(const vts_unet_desc* d) {
  if (check(d) != VTS_OK) return -1;
  Plan P{};
  plan(d, P);
  vts_unet_grads g{};              // sizes only depend on the descriptor
  g.d_raw = reinterpret_cast<const float*>(uintptr_t(4096));
  return bwd_total(d, &g, P);
}

extern "C" int vts_unet_backward(const vts_unet_desc* d, const vts_unet_grads* g, float* ws, int64_t ws_floats, void* stream) {
  const int rc0 = bwd_check(d, g);
  if (rc0 != VTS_OK) return rc0;
  Plan P{};
  plan(d, P);
  const int64_t need = bwd_total(d, g, P);
  VTS_CHECK_ARG(ws && ws_floats >= need, "vts_unet_backward: workspace of %lld floats, need %lld (vts_unet_backward_ws_floats)", (long long)ws_floats,
                (long long)need);
  Layer L[3 * VTS_UNET_MAX_DOWNS];
  int n = 0;
  build(d, ws, P, L, &n);
  const bool lanes = d->side_stream && d->side_stream != stream && d->num_layer_separate > 0;
  hipEvent_t fork = nullptr, join = nullptr;
  if (lanes) {
    const int rc = lane_events(&fork, &join, 1);
    if (rc != VTS_OK) return rc;
  }
  Bwd B{};
  B.d = d; B.g = g; B.ws = ws; B.P = &P; B.L = L; B.dry = false; B.off = P.total;
  return run_bwd(B, stream, lanes ? d->side_stream : nullptr, fork, join);
}
