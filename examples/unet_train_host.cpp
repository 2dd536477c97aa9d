// A host that is NOT Python TRAINING the generator on libvts_hip.so (the network-level entries vts_unet_forward /
// vts_unet_backward of include/vts.h): K steps of an L1 regression of the generator's output onto a target image, without torch:
//   unet_train_host <in.bin> <target.bin> <steps> <weights_out.bin>
// in.bin      the format of examples/unet_infer_host.cpp (the generator's weights and its input; num_layer_separate >= 1, style_C = 0, an
//             output of 3 visual + 2 tactile channels)
// target.bin  float [N][5][H][W]
// Per step, all on one stream (the tactile branch on a side stream):
//   1. vts_unet_forward                                  g_out = G(input), post-Tanh
//   2. vts_l1 per image and part (visual 3, tactile 2)   loss = mean |g_out - target|, its gradient d fake_I / d fake_T
//   3. vts_g_out_grad with an all-ones mask              d_raw = d loss / d pre-Tanh output
//   4. vts_unet_backward                                 every parameter gradient, into one flat buffer laid out like the parameters
//   5. vts_adam_flat over the flat parameter buffer      torch.optim.Adam(lr 2e-4, betas (0.5, 0.999), eps 1e-8)
// prints the loss of every step and writes the final weights (the flat buffer: in.bin's parameter order).
// Build: hipcc -O2 -I include examples/unet_train_host.cpp -L visual-tactile-synthesis_amd -lvts_hip -Wl,-rpath,'$ORIGIN/..' -o <bin>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "vts.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
#define VTS_OK_OR_FAIL(x, name) do { if ((x) != VTS_OK) { fprintf(stderr, "%s: %s\n", name, vts_last_error()); return 3; } } while (0)

static bool read_exact(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

static float* upload(const std::vector<float>& h) {
  float* p = nullptr;
  if (hipMalloc(&p, sizeof(float) * h.size()) != hipSuccess || hipMemcpy(p, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice) != hipSuccess) {
    fprintf(stderr, "device upload failed\n");
    exit(2);
  }
  return p;
}

int main(int argc, char** argv) {
  if (argc != 5) { fprintf(stderr, "usage: %s <in.bin> <target.bin> <steps> <weights_out.bin>\n", argv[0]); return 1; }
  const int steps = atoi(argv[3]);
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  int32_t hdr[9];
  if (!read_exact(f, hdr, sizeof hdr) || hdr[0] != 0x55535456) { fprintf(stderr, "bad header\n"); return 1; }
  vts_unet_desc d{};
  d.N = hdr[1]; d.H = hdr[2]; d.W = hdr[3]; d.num_downs = hdr[4]; d.num_layer_separate = hdr[5];
  const int c0 = hdr[6], c1 = hdr[7], nd = d.num_downs, nls = d.num_layer_separate, N = d.N;
  if (nd < 2 || nd > VTS_UNET_MAX_DOWNS || nls < 1 || hdr[8] != 0 || steps < 1) { fprintf(stderr, "unsupported configuration\n"); return 1; }
  int32_t chan[3][VTS_UNET_MAX_DOWNS];
  for (int k = 0; k < 3; ++k)
    if (!read_exact(f, chan[k], sizeof(int32_t) * nd)) { fprintf(stderr, "short file\n"); return 1; }
  for (int i = 0; i < nd; ++i) { d.channels[i] = chan[0][i]; d.up_cout[i] = chan[1][i]; d.upT_cout[i] = chan[2][i]; }
  if (d.up_cout[0] != 3 || d.upT_cout[0] != 2) { fprintf(stderr, "the output must be 3 visual + 2 tactile channels\n"); return 1; }
  const int64_t HW = (int64_t)d.H * d.W;
  std::vector<float> x0((size_t)(N * c0 * HW)), x1((size_t)(N * c1 * HW));
  if (!read_exact(f, x0.data(), sizeof(float) * x0.size()) || !read_exact(f, x1.data(), sizeof(float) * x1.size())) { fprintf(stderr, "short file\n"); return 1; }
  // the parameters, in file order, into one flat buffer (Adam runs over it as one tensor); offsets per parameter
  std::vector<int64_t> sizes;
  for (int i = 0; i < nd; ++i) {
    const int cin_down = i == 0 ? c0 + c1 : d.channels[i - 1];
    const int cin_up = i == nd - 1 ? d.channels[i] : (i == 0 ? d.channels[0] : 2 * d.channels[i]);
    sizes.push_back((int64_t)d.channels[i] * cin_down * 16); sizes.push_back(d.channels[i]);
    sizes.push_back((int64_t)cin_up * d.up_cout[i] * 16); sizes.push_back(d.up_cout[i]);
    if (i < nls) { sizes.push_back((int64_t)cin_up * d.upT_cout[i] * 16); sizes.push_back(d.upT_cout[i]); }
  }
  int64_t total = 0;
  for (int64_t s : sizes) total += s;
  std::vector<float> hp((size_t)total);
  if (!read_exact(f, hp.data(), sizeof(float) * hp.size())) { fprintf(stderr, "short file\n"); return 1; }
  fclose(f);
  std::vector<float> target((size_t)(N * 5 * HW));
  FILE* t = fopen(argv[2], "rb");
  if (!t || !read_exact(t, target.data(), sizeof(float) * target.size())) { fprintf(stderr, "%s: short or missing\n", argv[2]); return 1; }
  fclose(t);

  float* P = upload(hp);
  float *G = nullptr, *m = nullptr, *v = nullptr;
  HIP_OK(hipMalloc(&G, sizeof(float) * total));
  HIP_OK(hipMalloc(&m, sizeof(float) * total));
  HIP_OK(hipMalloc(&v, sizeof(float) * total));
  HIP_OK(hipMemset(m, 0, sizeof(float) * total));
  HIP_OK(hipMemset(v, 0, sizeof(float) * total));
  vts_unet_grads g{};
  int64_t off = 0;
  size_t k = 0;
  for (int i = 0; i < nd; ++i) {
    d.down_w[i] = P + off; g.down_dw[i] = G + off; off += sizes[k++];
    d.down_b[i] = P + off; g.down_db[i] = G + off; off += sizes[k++];
    d.up_w[i] = P + off; g.up_dw[i] = G + off; off += sizes[k++];
    d.up_b[i] = P + off; g.up_db[i] = G + off; off += sizes[k++];
    if (i < nls) {
      d.upT_w[i] = P + off; g.upT_dw[i] = G + off; off += sizes[k++];
      d.upT_b[i] = P + off; g.upT_db[i] = G + off; off += sizes[k++];
    }
  }
  d.in0 = vts_operand{upload(x0), nullptr, nullptr, c0, c0 * HW};
  d.in1 = vts_operand{c1 ? upload(x1) : nullptr, nullptr, nullptr, c1, c1 * HW};
  float* tgt = upload(target);
  float *out = nullptr, *dI = nullptr, *dT = nullptr, *d_raw = nullptr;
  HIP_OK(hipMalloc(&out, sizeof(float) * N * 5 * HW));
  HIP_OK(hipMalloc(&dI, sizeof(float) * N * 3 * HW));
  HIP_OK(hipMalloc(&dT, sizeof(float) * N * 2 * HW));
  HIP_OK(hipMalloc(&d_raw, sizeof(float) * N * 5 * HW));
  float* mask = upload(std::vector<float>((size_t)(N * HW), 1.f));
  int64_t* loss = nullptr;
  HIP_OK(hipMalloc(&loss, sizeof(int64_t)));
  d.out = out;
  g.d_raw = d_raw;
  hipStream_t st, side;
  HIP_OK(hipStreamCreate(&st));
  HIP_OK(hipStreamCreate(&side));
  d.side_stream = side;
  const int64_t need = vts_unet_backward_ws_floats(&d);        // the forward's workspace is its prefix
  if (need < 0) { fprintf(stderr, "vts_unet_backward_ws_floats: %s\n", vts_last_error()); return 3; }
  float* ws = nullptr;
  HIP_OK(hipMalloc(&ws, sizeof(float) * (size_t)need));
  const float coeff = 1.f / (float)(N * 5 * HW);                 // nn.L1Loss: the mean over every element
  for (int s = 1; s <= steps; ++s) {
    HIP_OK(hipMemsetAsync(loss, 0, sizeof(int64_t), st));
    VTS_OK_OR_FAIL(vts_unet_forward(&d, ws, need, st), "vts_unet_forward");
    for (int n = 0; n < N; ++n) {
      VTS_OK_OR_FAIL(vts_l1(out + (int64_t)n * 5 * HW, tgt + (int64_t)n * 5 * HW, 3 * HW, coeff, loss, dI + (int64_t)n * 3 * HW, 0, st), "vts_l1");
      VTS_OK_OR_FAIL(vts_l1(out + (int64_t)(n * 5 + 3) * HW, tgt + (int64_t)(n * 5 + 3) * HW, 2 * HW, coeff, loss, dT + (int64_t)n * 2 * HW, 0, st), "vts_l1");
    }
    VTS_OK_OR_FAIL(vts_g_out_grad(dI, dT, mask, out, N, d.H, d.W, d_raw, st), "vts_g_out_grad");
    VTS_OK_OR_FAIL(vts_unet_backward(&d, &g, ws, need, st), "vts_unet_backward");
    VTS_OK_OR_FAIL(vts_adam_flat(P, G, m, v, total, 2e-4f, 0.5f, 0.999f, 1e-8f, s, 1.f, st), "vts_adam_flat");
    int64_t h = 0;
    HIP_OK(hipMemcpyAsync(&h, loss, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    printf("step %d: L1 loss %.6f\n", s, (double)h / VTS_LOSS_SCALE);
  }
  HIP_OK(hipMemcpy(hp.data(), P, sizeof(float) * hp.size(), hipMemcpyDeviceToHost));
  FILE* o = fopen(argv[4], "wb");
  if (!o || fwrite(hp.data(), sizeof(float), hp.size(), o) != hp.size()) { perror(argv[4]); return 1; }
  fclose(o);
  printf("trained %d steps: N %d, %d x %d, %lld parameters, %lld workspace floats\n", steps, N, d.H, d.W, (long long)total, (long long)need);
  return 0;
}
