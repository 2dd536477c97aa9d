// Network-level entry points (`vts_msd_fwd`), round 6: the forward of the reference's discriminators
//   NLayerDiscriminator.forward        models/networks.py:1696-1750   -> vts_patchgan_forward (one PatchGAN = one scale)
//   MultiscaleDiscriminator.forward    models/networks.py:1649-1691   -> vts_msd_forward (num_D PatchGANs over an average-pooled pyramid)
// in TRAINING mode -- BatchNorm2d normalises with the statistics of the batch and advances its running statistics, as every discriminator
// call of a reference training step does (models/sinskitG_model.py:1361, 1374, 1490, 1567, 1584, 1781) -- as ONE C call over the library's
// own operators; the workspace keeps the pyramid, the raw layer outputs and the statistics, which vts_patchgan_backward / vts_msd_backward
// (below) read.  The Python product takes this path for its forward-only discriminator
// passes (the full-resolution D2 visualisation pass, the D2 term of the generator step: vts/engine.py:_scale_lane) and drives the same
// operators layer by layer where a backward follows; the two are bit-identical (tests/test_network_abi_gpu.py).  The schedule of one PatchGAN:
//   conv 0 (stride 2)                                   raw output; LeakyReLU(0.2) is applied by the next convolution on load
//   conv j (stride 2, the last but one stride 1) -> BatchNorm2d: statistics from the convolution's epilogue (vts_conv4x4_norm) or a
//                                                      statistics pass; scale / shift are applied by the next convolution on load
//   conv n-1 (stride 1, 1 channel)                      the prediction map (skipped with run_head = 0: a pass that exists for the
//                                                      BatchNorm running statistics at this scale)
// No allocation: the caller passes vts_patchgan_forward_ws_floats(d) / vts_msd_forward_ws_floats(d) floats.
#include <stdint.h>

#include <algorithm>

#include "vts_internal.h"

namespace {

struct PgPlan {
  int n;                                          // convolutions that run
  int oh[VTS_PATCHGAN_MAX_CONVS], ow[VTS_PATCHGAN_MAX_CONVS];
  int64_t act_off[VTS_PATCHGAN_MAX_CONVS];        // raw convolution outputs (the head writes d->pred)
  int64_t stat_off[VTS_PATCHGAN_MAX_CONVS];       // [4][N * C]: scale, shift, mean, rstd of a normalised layer
  int64_t conv_ws, conv_ws_floats, stat_ws, stat_ws_floats;
  int64_t total;
};

int pg_check(const vts_patchgan_desc* d, const char* who) {
  VTS_CHECK_ARG(d, "%s: null descriptor", who);
  VTS_CHECK_ARG(d->n_convs >= 2 && d->n_convs <= VTS_PATCHGAN_MAX_CONVS, "%s: n_convs %d (2 .. %d)", who, d->n_convs, VTS_PATCHGAN_MAX_CONVS);
  VTS_CHECK_ARG(d->N >= 1 && d->H >= 1 && d->W >= 1, "%s: bad shape N %d, %d x %d", who, d->N, d->H, d->W);
  VTS_CHECK_ARG(d->in0.data && d->in0.C >= 1 && (d->in1.C == 0 || d->in1.data), "%s: null input", who);
  for (int j = 0; j < d->n_convs; ++j) {
    VTS_CHECK_ARG(d->w[j] && d->cout[j] >= 1 && (d->stride[j] == 1 || d->stride[j] == 2), "%s: convolution %d incomplete (cout %d, stride %d)", who, j,
                  d->cout[j], d->stride[j]);
    VTS_CHECK_ARG(!(d->gamma[j] || d->beta[j]) || (d->gamma[j] && d->beta[j]), "%s: BatchNorm of convolution %d needs both weight and bias", who, j);
    VTS_CHECK_ARG(!d->running_mean[j] == !d->running_var[j], "%s: running_mean / running_var of convolution %d come as a pair", who, j);
    VTS_CHECK_ARG(!d->stat_mean_out[j] == !d->stat_uvar_out[j], "%s: stat_mean_out / stat_uvar_out of convolution %d come as a pair", who, j);
  }
  VTS_CHECK_ARG(!d->gamma[0] && !d->gamma[d->n_convs - 1], "%s: the first and the last convolution carry no BatchNorm (networks.py:1703-1741)", who);
  VTS_CHECK_ARG(!d->run_head || d->pred, "%s: run_head without a prediction buffer", who);
  return VTS_OK;
}

// the convolution descriptors of the schedule, in launch order: shared by the workspace planner and the launcher
void pg_layers(const vts_patchgan_desc* d, float* ws, const PgPlan& P, vts_conv_desc* L) {
  vts_operand cur0 = d->in0, cur1 = d->in1;
  int h = d->H, w = d->W;
  for (int j = 0; j < P.n; ++j) {
    vts_conv_desc& c = L[j];
    c = vts_conv_desc{};
    c.in0 = cur0; c.in1 = cur1;
    const int cin = cur0.C + cur1.C;
    c.N = d->N; c.IH = h; c.IW = w; c.OH = P.oh[j]; c.OW = P.ow[j]; c.Cout = d->cout[j];
    c.stride = d->stride[j]; c.pad = 2; c.transposed = 0;
    c.w = d->w[j]; c.ws_co = cin * 16; c.ws_ci = 16; c.bias = d->b[j];
    const bool head = j == d->n_convs - 1;
    c.out = head ? d->pred : ws + P.act_off[j];
    c.out_nstride = (int64_t)c.Cout * c.OH * c.OW;
    c.act_in = j ? VTS_ACT_LRELU : VTS_ACT_NONE; c.act_out = VTS_ACT_NONE;
    cur0 = vts_operand{};
    cur0.data = c.out; cur0.C = c.Cout; cur0.nstride = c.out_nstride;
    if (d->gamma[j]) { cur0.scale = ws + P.stat_off[j]; cur0.shift = ws + P.stat_off[j] + (int64_t)d->N * c.Cout; }
    cur1 = vts_operand{};
    h = c.OH; w = c.OW;
  }
}

void pg_plan(const vts_patchgan_desc* d, PgPlan& P) {
  int64_t off = 0;
  auto take = [&](int64_t n) { const int64_t o = off; off += (n + 63) / 64 * 64; return o; };
  P.n = d->run_head ? d->n_convs : d->n_convs - 1;
  int h = d->H, w = d->W;
  for (int j = 0; j < P.n; ++j) {
    // Conv2d(kernel 4, stride s, padding 2): networks.py:1703, 1716, 1728, 1739
    P.oh[j] = (h + 4 - 4) / d->stride[j] + 1; P.ow[j] = (w + 4 - 4) / d->stride[j] + 1;
    h = P.oh[j]; w = P.ow[j];
    P.act_off[j] = P.stat_off[j] = 0;
    if (j != d->n_convs - 1) P.act_off[j] = take((int64_t)d->N * d->cout[j] * h * w);
    if (d->gamma[j]) P.stat_off[j] = take(4 * (int64_t)d->N * d->cout[j]);
  }
  vts_conv_desc L[VTS_PATCHGAN_MAX_CONVS];
  pg_layers(d, reinterpret_cast<float*>(uintptr_t(4096)), P, L);      // (a placeholder base: only the shapes are read)
  int64_t cw = 0, sw = 0;
  for (int j = 0; j < P.n; ++j) {
    const vts_conv_desc& c = L[j];
    if ((int64_t)c.OH * c.OW <= 64 * 64) cw = std::max(cw, vts_conv4x4_ws_floats(&c));
    if (d->gamma[j]) {
      sw = std::max(sw, vts_conv4x4_norm_ws_floats(&c));
      cw = std::max(cw, vts_norm_ws_floats(c.N, c.Cout, c.OH * c.OW));
    }
  }
  P.conv_ws_floats = cw; P.stat_ws_floats = sw;
  P.conv_ws = take(cw); P.stat_ws = take(sw);
  P.total = off;
}

int pg_run(const vts_patchgan_desc* d, float* ws, const PgPlan& P, void* stream) {
  vts_conv_desc L[VTS_PATCHGAN_MAX_CONVS];
  pg_layers(d, ws, P, L);
  for (int j = 0; j < P.n; ++j) {
    vts_conv_desc& c = L[j];
    if ((int64_t)c.OH * c.OW <= 64 * 64) { c.ws = ws + P.conv_ws; c.ws_floats = P.conv_ws_floats; }
    if (!d->gamma[j]) {
      const int rc = vts_conv4x4(&c, stream);
      if (rc != VTS_OK) return rc;
      continue;
    }
    vts_norm_desc nd{};
    const int64_t NC = (int64_t)c.N * c.Cout;
    float* stt = ws + P.stat_off[j];
    nd.x = c.out; nd.nstride = c.out_nstride; nd.N = c.N; nd.C = c.Cout; nd.HW = c.OH * c.OW; nd.mode = 1;
    nd.eps = d->eps; nd.momentum = d->momentum;
    nd.gamma = d->gamma[j]; nd.beta = d->beta[j];
    nd.running_mean = d->running_mean[j]; nd.running_var = d->running_var[j]; nd.num_batches_tracked = d->num_batches_tracked[j];
    nd.stat_mean_out = d->stat_mean_out[j]; nd.stat_uvar_out = d->stat_uvar_out[j];
    nd.scale = stt; nd.shift = stt + NC; nd.mean_out = stt + 2 * NC; nd.rstd_out = stt + 3 * NC;
    int fused = 0;
    int rc = vts_conv4x4_norm(&c, &nd, ws + P.stat_ws, P.stat_ws_floats, &fused, stream);
    if (rc != VTS_OK) return rc;
    if (fused >= 2) rc = vts_norm_stats_from_partials(&nd, ws + P.stat_ws, fused - 2, stream);
    else if (fused == 0) rc = vts_norm_stats(&nd, ws + P.conv_ws, stream);
    if (rc != VTS_OK) return rc;
  }
  return VTS_OK;
}

struct MsdPlan {
  vts_patchgan_desc s[VTS_MSD_MAX_SCALES];      // the scales with their inputs resolved (pooled levels in the workspace)
  PgPlan p[VTS_MSD_MAX_SCALES];
  int64_t pool_off[VTS_MSD_MAX_SCALES][2];      // pooled level of in0 / in1 for scale >= 1
  int64_t scale_ws[VTS_MSD_MAX_SCALES];
  int64_t total;
};

int msd_check(const vts_msd_desc* d) {
  VTS_CHECK_ARG(d, "vts_msd_forward: null descriptor");
  VTS_CHECK_ARG(d->num_D >= 1 && d->num_D <= VTS_MSD_MAX_SCALES, "vts_msd_forward: num_D %d (1 .. %d)", d->num_D, VTS_MSD_MAX_SCALES);
  VTS_CHECK_ARG(d->scale[0].in0.data && d->scale[0].in0.C >= 1, "vts_msd_forward: scale 0 carries the input");
  return VTS_OK;
}

int msd_plan(const vts_msd_desc* d, float* ws, MsdPlan& M) {
  int64_t off = 0;
  auto take = [&](int64_t n) { const int64_t o = off; off += (n + 63) / 64 * 64; return o; };
  int h = d->scale[0].H, w = d->scale[0].W;
  const int N = d->scale[0].N, c0 = d->scale[0].in0.C, c1 = d->scale[0].in1.C;
  for (int s = 0; s < d->num_D; ++s) {
    M.s[s] = d->scale[s];
    M.s[s].N = N; M.s[s].H = h; M.s[s].W = w;
    if (s > 0) {
      // AvgPool2d(3, stride 2, padding 1, count_include_pad False) of the level above (networks.py:1670, 1688)
      M.pool_off[s][0] = take((int64_t)N * c0 * h * w);
      M.pool_off[s][1] = c1 ? take((int64_t)N * c1 * h * w) : 0;
      vts_operand a{}, b{};
      a.data = ws + M.pool_off[s][0]; a.C = c0; a.nstride = (int64_t)c0 * h * w;
      if (c1) { b.data = ws + M.pool_off[s][1]; b.C = c1; b.nstride = (int64_t)c1 * h * w; }
      M.s[s].in0 = a; M.s[s].in1 = b;
    }
    const int rc = pg_check(&M.s[s], "vts_msd_forward");
    if (rc != VTS_OK) return rc;
    pg_plan(&M.s[s], M.p[s]);
    M.scale_ws[s] = take(M.p[s].total);
    h = (h + 1) / 2; w = (w + 1) / 2;
  }
  M.total = off;
  return VTS_OK;
}

}  // namespace

extern "C" int64_t vts_patchgan_forward_ws_floats(const vts_patchgan_desc* d) {
  if (pg_check(d, "vts_patchgan_forward") != VTS_OK) return -1;
  PgPlan P{};
  pg_plan(d, P);
  return P.total;
}

extern "C" int vts_patchgan_forward(const vts_patchgan_desc* d, float* ws, int64_t ws_floats, void* stream) {
  const int rc = pg_check(d, "vts_patchgan_forward");
  if (rc != VTS_OK) return rc;
  PgPlan P{};
  pg_plan(d, P);
  VTS_CHECK_ARG(ws && ws_floats >= P.total, "vts_patchgan_forward: workspace of %lld floats, need %lld", (long long)ws_floats, (long long)P.total);
  return pg_run(d, ws, P, stream);
}

extern "C" int64_t vts_msd_forward_ws_floats(const vts_msd_desc* d) {
  if (msd_check(d) != VTS_OK) return -1;
  MsdPlan M{};
  if (msd_plan(d, reinterpret_cast<float*>(uintptr_t(4096)), M) != VTS_OK) return -1;
  return M.total;
}

extern "C" int vts_msd_forward(const vts_msd_desc* d, float* ws, int64_t ws_floats, void* stream) {
  int rc = msd_check(d);
  if (rc != VTS_OK) return rc;
  MsdPlan M{};
  rc = msd_plan(d, ws, M);
  if (rc != VTS_OK) return rc;
  VTS_CHECK_ARG(ws && ws_floats >= M.total, "vts_msd_forward: workspace of %lld floats, need %lld", (long long)ws_floats, (long long)M.total);
  for (int s = 0; s < d->num_D; ++s) {
    if (s > 0) {
      const vts_patchgan_desc& up = M.s[s - 1];
      // a lazily normalised operand cannot be pooled as stored: the pyramid is built from the RAW inputs, as the reference pools them
      VTS_CHECK_ARG(!up.in0.scale && !up.in0.shift && !up.in1.scale && !up.in1.shift, "vts_msd_forward: the input operands must be plain tensors (no scale / shift)");
      rc = vts_avgpool3s2(up.in0.data, up.in0.nstride, up.N, up.in0.C, up.H, up.W, const_cast<float*>(M.s[s].in0.data), stream);
      if (rc == VTS_OK && up.in1.C) rc = vts_avgpool3s2(up.in1.data, up.in1.nstride, up.N, up.in1.C, up.H, up.W, const_cast<float*>(M.s[s].in1.data), stream);
      if (rc != VTS_OK) return rc;
    }
    rc = pg_run(&M.s[s], ws + M.scale_ws[s], M.p[s], stream);
    if (rc != VTS_OK) return rc;
  }
  return VTS_OK;
}

// ---- the backward (`vts_msd_bwd`): vts/engine.py:_msd_scale_backward / msd_backward as one call ----------------------------
// Per PatchGAN, convolution j = n-1 .. 0: the BatchNorm backward of the incoming gradient (vts_norm_bwd_from_partials where the
// backward-data convolution above left its epilogue sums, else vts_norm_bwd), the deferred weight gradient and the bias gradient, and the
// backward-data convolution into the gradient of the layer below (vts_conv4x4_bsums when a BatchNorm follows; the GEMM-class route of
// _flat4 on wide layers) -- or, at j = 0, into the input gradient.  Everything the backward needs beyond the forward's workspace is carved
// out behind it, one region per buffer and per launch; a sizing pass walks the same schedule without launching.
namespace {

// engine.py:_flat4 with the product's defaults (VTS_FLAT_D 1, VTS_FLAT_MIN_C 64, VTS_WIDE_MIN_CI 64, VTS_WIDE_MIN_CO 128)
bool flat4(int co, int ci, int j, int oh, int ow, int st) {
  if (j == 0 || ci < 64) return false;
  if (vts_conv4x4_flat_ok(oh, ow, st * (oh - 1) + 4, st * (ow - 1) + 4, 0)) return co >= 64 || ci >= 256;
  return co >= 128 && co % 4 == 0 && ci % 4 == 0;
}

struct DBwd {
  float* ws;
  bool dry;
  int64_t off;
  vts_reduce_job jobs[VTS_MSD_MAX_SCALES * VTS_PATCHGAN_MAX_CONVS];
  int njobs;
  float* take(int64_t n) {
    float* p = ws + off;
    off += (n + 63) / 64 * 64;
    return p;
  }
};

bool pg_param_grads(const vts_patchgan_grads* g, int n) {
  for (int j = 0; j < n; ++j)
    if (g->dw[j] || g->db[j] || g->dgamma[j] || g->dbeta[j]) return true;
  return false;
}

int pg_grads_check(const vts_patchgan_desc* d, const vts_patchgan_grads* g, const char* who, int s) {
  VTS_CHECK_ARG(d->run_head, "%s: the backward needs the workspace of a forward with run_head = 1", who);
  VTS_CHECK_ARG(g, "%s: null gradient struct", who);
  VTS_CHECK_ARG(g->dpred, "%s: scale %d has no dpred", who, s);
  if (!pg_param_grads(g, d->n_convs)) return VTS_OK;
  for (int j = 0; j < d->n_convs; ++j)
    VTS_CHECK_ARG(g->dw[j] && (!d->b[j] || g->db[j]) && (!d->gamma[j] || (g->dgamma[j] && g->dbeta[j])),
                  "%s: scale %d, convolution %d: parameter gradient missing (dw / db / dgamma / dbeta: all or none)", who, s, j);
  return VTS_OK;
}

// one PatchGAN; d_in / d_in_acc: where the input gradient goes (NULL: none)
int pg_bwd(DBwd& B, const vts_patchgan_desc* d, float* ws, const PgPlan& P, const vts_patchgan_grads* g, float* d_in, int d_in_acc,
           void* stream) {
  vts_conv_desc L[VTS_PATCHGAN_MAX_CONVS];
  pg_layers(d, ws, P, L);
  const bool pgr = pg_param_grads(g, d->n_convs);
  const int N = d->N;
  int rc;
  // the gradient w.r.t. the output of convolution j (raw for j = n-1; w.r.t. the normalised output where a BatchNorm follows)
  float* gd = const_cast<float*>(g->dpred);
  int slots = 0;
  float* part = nullptr;
  for (int j = d->n_convs - 1; j >= 0; --j) {
    const vts_conv_desc& f = L[j];
    const int co = f.Cout, cin = f.in0.C + f.in1.C;
    const int oh = f.OH, ow = f.OW, h = f.IH, w = f.IW, st = f.stride;
    const int64_t ons = (int64_t)co * oh * ow;
    if (d->gamma[j]) {
      vts_norm_bwd_desc nb{};
      const int64_t NC = (int64_t)N * co;
      nb.dy = gd; nb.x = f.out; nb.nstride = f.out_nstride; nb.N = N; nb.C = co; nb.HW = oh * ow; nb.mode = 1;
      nb.mean = ws + P.stat_off[j] + 2 * NC; nb.rstd = ws + P.stat_off[j] + 3 * NC;
      nb.gamma = d->gamma[j]; nb.dgamma = pgr ? g->dgamma[j] : nullptr; nb.dbeta = pgr ? g->dbeta[j] : nullptr;
      nb.accumulate_param_grads = g->accumulate; nb.ngroups = 1;
      float* nws = B.take(vts_norm_ws_floats(N, co, oh * ow));
      if (!B.dry) {
        rc = slots > 0 ? vts_norm_bwd_from_partials(&nb, part, slots, d->beta[j], stream) : vts_norm_bwd(&nb, nws, stream);
        if (rc != VTS_OK) return rc;
      }
    }
    vts_operand go{};
    go.data = gd; go.C = co; go.nstride = ons;
    if (pgr) {
      vts_wgrad_desc wd{};
      wd.lo0 = go; wd.hi0 = f.in0; wd.hi1 = f.in1;
      wd.act_lo = VTS_ACT_NONE; wd.act_hi = j ? VTS_ACT_LRELU : VTS_ACT_NONE;
      wd.N = N; wd.LH = oh; wd.LW = ow; wd.HH = h; wd.HW = w; wd.stride = st; wd.pad = 2;
      wd.dw = g->dw[j]; wd.accumulate = g->accumulate; wd.defer = 1;
      const int64_t n = vts_wgrad4x4_ws_floats(&wd);
      float* wp = B.take(n);
      const int64_t nel = (int64_t)cin * co * 16;
      if (!B.dry) {
        vts_reduce_job& q = B.jobs[B.njobs++];
        q = vts_reduce_job{};
        q.dw = g->dw[j]; q.nel = nel; q.accumulate = g->accumulate; q.nseg = 1; q.part[0] = wp; q.pw[0] = (int)(n / nel);
        if ((rc = vts_wgrad4x4(&wd, wp, stream)) != VTS_OK) return rc;
      }
      float* cws = B.take(vts_channel_sum_ws_floats(N, co, oh * ow));
      rc = VTS_OK;
      if (!B.dry && g->db[j]) {
        if (!d->gamma[j]) rc = vts_channel_sum(gd, ons, N, co, oh * ow, g->db[j], g->accumulate, cws, nullptr, stream);
        else if (!g->accumulate) rc = hipMemsetAsync(g->db[j], 0, sizeof(float) * co, (hipStream_t)stream) == hipSuccess ? (int)VTS_OK : (int)VTS_ERR_LAUNCH;
        if (rc != VTS_OK) return rc;
      }
    }
    if (j > 0) {
      const vts_operand& prev = f.in0;                // the layer below (raw output + its BatchNorm scale / shift)
      const int64_t pns = (int64_t)cin * h * w;
      float* tgt = B.take(N * pns);
      const int qh = st == 1 ? oh + 2 : oh + 1, qw = st == 1 ? ow + 2 : ow + 1;
      slots = 0;
      if (flat4(co, cin, j, oh, ow, st) && (cin % 4 == 0 || vts_conv4x4_flat_ok(h, w, qh, qw, st == 2))) {
        // the GEMM-class route: the output gradient zero-padded, the adjoint taps packed, then the LeakyReLU derivative mask
        float* raw = B.take(N * pns);
        float* pad = B.take((int64_t)N * co * qh * qw);
        float* wt = B.take((int64_t)co * 16 * ((cin + 3) / 4 * 4));
        const int64_t wsn = vts_conv4x4_wide_ws_floats(N, co, cin, h, w, qh, qw, st == 2);
        float* cws = wsn ? B.take(wsn) : nullptr;
        if (!B.dry) {
          rc = vts_pad_affine(&go, N, oh, ow, st == 1 ? 1 : 0, 1, st == 1 ? 1 : 0, 1, 0, VTS_ACT_NONE, nullptr, pad, 0, stream);
          if (rc == VTS_OK) rc = vts_w4x4_pack(f.w, co, cin, 16 * (int64_t)cin, 16, st == 1 ? 1 : 0, wt, stream);
          if (rc == VTS_OK) rc = vts_conv4x4_wide(pad, wt, nullptr, raw, N, co, cin, qh, qw, h, w, st, st == 2, cws, wsn, stream);
          if (rc == VTS_OK) rc = vts_act_bwd(raw, &prev, N, h * w, VTS_ACT_LRELU, tgt, 0, stream);
          if (rc != VTS_OK) return rc;
        }
      } else {
        vts_conv_desc c{};
        c.in0 = go;
        c.N = N; c.IH = oh; c.IW = ow; c.OH = h; c.OW = w; c.Cout = cin;
        c.stride = st; c.pad = 2; c.transposed = 1;
        c.w = f.w; c.ws_co = 16; c.ws_ci = cin * 16;
        c.out = tgt; c.out_nstride = pns;
        c.dmask = prev; c.dmask_act = VTS_ACT_LRELU;
        if ((int64_t)h * w <= 64 * 64) {
          c.ws_floats = vts_conv4x4_ws_floats(&c);
          c.ws = B.take(c.ws_floats);
        }
        if (d->gamma[j - 1]) {        // a BatchNorm follows: the epilogue also emits its backward's sums
          const int64_t pf = vts_conv4x4_norm_ws_floats(&c);
          part = B.take(pf);
          if (!B.dry && (rc = vts_conv4x4_bsums(&c, part, pf, &slots, stream)) != VTS_OK) return rc;
        } else if (!B.dry && (rc = vts_conv4x4(&c, stream)) != VTS_OK) {
          return rc;
        }
      }
      gd = tgt;
    } else if (d_in) {                // w.r.t. the second concat source, or the only one (in1.C == 0)
      const int c0 = d->in1.C ? d->in0.C : 0, c1 = d->in1.C ? d->in1.C : d->in0.C;
      vts_conv_desc c{};
      c.in0 = go;
      c.N = N; c.IH = oh; c.IW = ow; c.OH = h; c.OW = w; c.Cout = c1;
      c.stride = st; c.pad = 2; c.transposed = 1;
      c.w = f.w + (int64_t)c0 * 16; c.ws_co = 16; c.ws_ci = cin * 16;
      c.out = d_in; c.out_nstride = (int64_t)c1 * h * w; c.accumulate = d_in_acc;
      if ((int64_t)h * w <= 64 * 64) {
        c.ws_floats = vts_conv4x4_ws_floats(&c);
        c.ws = B.take(c.ws_floats);
      }
      if (!B.dry && (rc = vts_conv4x4(&c, stream)) != VTS_OK) return rc;
    }
  }
  return VTS_OK;
}

int pg_bwd_check_all(const vts_patchgan_desc* d, const vts_patchgan_grads* g, const char* who) {
  int rc = pg_check(d, who);
  if (rc == VTS_OK) rc = pg_grads_check(d, g, who, 0);
  return rc;
}

int64_t pg_bwd_total(const vts_patchgan_desc* d, const vts_patchgan_grads* g, const PgPlan& P) {
  DBwd B{};
  B.ws = reinterpret_cast<float*>(uintptr_t(4096)); B.dry = true; B.off = P.total;
  pg_bwd(B, d, B.ws, P, g, g->d_in, g->d_in_accumulate, nullptr);
  return B.off;
}

// all scales; the input gradient merged over the pyramid (engine.py:_merge_input_grads)
int msd_bwd(DBwd& B, const vts_msd_desc* d, const MsdPlan& M, const vts_msd_grads* g, void* stream) {
  float* din[VTS_MSD_MAX_SCALES] = {nullptr};
  const int N = M.s[0].N;
  const int c1 = M.s[0].in1.C ? M.s[0].in1.C : M.s[0].in0.C;
  int rc;
  for (int s = 0; s < d->num_D; ++s) {
    if (g->d_in) din[s] = B.take((int64_t)N * c1 * M.s[s].H * M.s[s].W);
    float* sws = B.ws + M.scale_ws[s];
    if ((rc = pg_bwd(B, &M.s[s], sws, M.p[s], &g->scale[s], din[s], 0, stream)) != VTS_OK) return rc;
  }
  if (B.njobs && !B.dry && (rc = vts_wgrad_reduce_batch(B.jobs, B.njobs, stream)) != VTS_OK) return rc;
  B.njobs = 0;
  if (!g->d_in) return VTS_OK;
  float* sum = g->d_in_accumulate ? B.take((int64_t)N * c1 * M.s[0].H * M.s[0].W) : nullptr;
  if (B.dry) return VTS_OK;
  for (int s = d->num_D - 1; s >= 1; --s)
    if ((rc = vts_avgpool3s2_bwd(din[s], N, c1, M.s[s - 1].H, M.s[s - 1].W, din[s - 1], (int64_t)c1 * M.s[s - 1].H * M.s[s - 1].W, 1, stream)) != VTS_OK)
      return rc;
  const int64_t n0 = (int64_t)N * c1 * M.s[0].H * M.s[0].W;
  if (g->d_in_accumulate) {           // d_in + d0 (torch's add_), through a region of its own
    vts_operand o{};
    o.data = g->d_in; o.C = c1; o.nstride = (int64_t)c1 * M.s[0].H * M.s[0].W;
    if ((rc = vts_pad_affine(&o, N, M.s[0].H, M.s[0].W, 0, 0, 0, 0, 0, VTS_ACT_NONE, din[0], sum, 0, stream)) != VTS_OK) return rc;
    if (hipMemcpyAsync(g->d_in, sum, sizeof(float) * n0, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
      vts_set_error("vts_msd_backward: copying the input gradient failed");
      return VTS_ERR_LAUNCH;
    }
  } else if (hipMemcpyAsync(g->d_in, din[0], sizeof(float) * n0, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
    vts_set_error("vts_msd_backward: copying the input gradient failed");
    return VTS_ERR_LAUNCH;
  }
  return VTS_OK;
}

int msd_bwd_prepare(const vts_msd_desc* d, const vts_msd_grads* g, MsdPlan& M, int64_t* need) {
  int rc = msd_check(d);
  if (rc != VTS_OK) return rc;
  if ((rc = msd_plan(d, reinterpret_cast<float*>(uintptr_t(4096)), M)) != VTS_OK) return rc;
  VTS_CHECK_ARG(g, "vts_msd_backward: null gradient struct");
  for (int s = 0; s < d->num_D; ++s)
    if ((rc = pg_grads_check(&M.s[s], &g->scale[s], "vts_msd_backward", s)) != VTS_OK) return rc;
  const int c1 = M.s[0].in1.C ? M.s[0].in1.C : M.s[0].in0.C;
  VTS_CHECK_ARG(!g->d_in || (int64_t)M.s[0].N * c1 <= 65535, "vts_msd_backward: N x C of the input gradient above 65535");
  DBwd B{};
  B.ws = reinterpret_cast<float*>(uintptr_t(4096)); B.dry = true; B.off = M.total;
  msd_bwd(B, d, M, g, nullptr);
  *need = B.off;
  return VTS_OK;
}

}  // namespace

extern "C" int64_t vts_patchgan_backward_ws_floats(const vts_patchgan_desc* d) {
  if (pg_check(d, "vts_patchgan_backward") != VTS_OK) return -1;
  PgPlan P{};
  pg_plan(d, P);
  vts_patchgan_grads g{};            // (the sizes depend on the descriptor only)
  g.dpred = reinterpret_cast<const float*>(uintptr_t(4096));
  for (int j = 0; j < d->n_convs; ++j) g.dw[j] = reinterpret_cast<float*>(uintptr_t(4096));
  g.d_in = reinterpret_cast<float*>(uintptr_t(4096));
  return pg_bwd_total(d, &g, P);
}

extern "C" int vts_patchgan_backward(const vts_patchgan_desc* d, const vts_patchgan_grads* g, float* ws, int64_t ws_floats, void* stream) {
  int rc = pg_bwd_check_all(d, g, "vts_patchgan_backward");
  if (rc != VTS_OK) return rc;
  PgPlan P{};
  pg_plan(d, P);
  const int64_t need = vts_patchgan_backward_ws_floats(d);
  VTS_CHECK_ARG(ws && ws_floats >= need, "vts_patchgan_backward: workspace of %lld floats, need %lld (vts_patchgan_backward_ws_floats)",
                (long long)ws_floats, (long long)need);
  DBwd B{};
  B.ws = ws; B.dry = false; B.off = P.total;
  if ((rc = pg_bwd(B, d, ws, P, g, g->d_in, g->d_in_accumulate, stream)) != VTS_OK) return rc;
  return B.njobs ? vts_wgrad_reduce_batch(B.jobs, B.njobs, stream) : VTS_OK;
}

extern "C" int64_t vts_msd_backward_ws_floats(const vts_msd_desc* d) {
  if (msd_check(d) != VTS_OK) return -1;
  vts_msd_grads g{};
  for (int s = 0; s < d->num_D; ++s) {
    g.scale[s].dpred = reinterpret_cast<const float*>(uintptr_t(4096));
    for (int j = 0; j < VTS_PATCHGAN_MAX_CONVS; ++j) g.scale[s].dw[j] = reinterpret_cast<float*>(uintptr_t(4096));
  }
  g.d_in = reinterpret_cast<float*>(uintptr_t(4096));
  g.d_in_accumulate = 1;
  MsdPlan M{};
  int64_t need = -1;
  // (the widest case: parameter gradients and an accumulated input gradient; a gradient check failure here is a descriptor error)
  for (int s = 0; s < d->num_D; ++s)
    for (int j = 0; j < d->scale[s].n_convs && j < VTS_PATCHGAN_MAX_CONVS; ++j) {
      if (d->scale[s].b[j]) g.scale[s].db[j] = g.scale[s].dw[j];
      if (d->scale[s].gamma[j]) g.scale[s].dgamma[j] = g.scale[s].dbeta[j] = g.scale[s].dw[j];
    }
  if (msd_bwd_prepare(d, &g, M, &need) != VTS_OK) return -1;
  return need;
}

extern "C" int vts_msd_backward(const vts_msd_desc* d, const vts_msd_grads* g, float* ws, int64_t ws_floats, void* stream) {
  MsdPlan M{};
  int64_t need = 0;
  int rc = msd_bwd_prepare(d, g, M, &need);
  if (rc != VTS_OK) return rc;
  const int64_t most = vts_msd_backward_ws_floats(d);
  VTS_CHECK_ARG(ws && ws_floats >= most, "vts_msd_backward: workspace of %lld floats, need %lld (vts_msd_backward_ws_floats)", (long long)ws_floats,
                (long long)most);
  if ((rc = msd_plan(d, ws, M)) != VTS_OK) return rc;
  DBwd B{};
  B.ws = ws; B.dry = false; B.off = M.total;
  return msd_bwd(B, d, M, g, stream);
}
