// Loss of the 2-D poke / image autoencoders (reference models/conv_poke_encoder.py:68-78, models/first_stage_image_conv.py:138-149):
//
//     rec_loss = |x - rec| + perc_weight * p            (p: [N,1,1,1], broadcast over the C * S elements of a sample)
//     nll      = sum(rec_loss / exp(logvar) + logvar) / N
//
// with `logvar` a TRAINED scalar parameter.  ipoke_l1_loss takes its scale as a host float; here the scale exp(-logvar) / N lives on
// the device, so the step needs no device-to-host copy: one pass over the decoder's output applies the output activation, writes the
// reconstruction, the gradient w.r.t. the pre-activation value and a per-workgroup partial of sum |x - rec|; a one-workgroup pass adds the
// partials and the perceptual values in a FIXED order (double, no float atomics: the value is reproducible run to run) and writes the
// value and its gradients w.r.t. logvar and p.  HBM-bound streaming work: every element is read once and written twice.
#include "common.h"

namespace ipoke {

constexpr int kNllBlocks = 1024;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// block-wide sum of doubles in a fixed order; `red` holds blockDim.x / 64 doubles
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < nw; ++i) t += red[i];
  return t;
}

// pre [N*S][ld] fp32 channels-last, x [N][C][S] fp32 (sample stride x_sn; NULL: only rec is written).  The activation and the
// gradient's factor are evaluated in double and rounded once: rec is the correctly rounded value of tanh, and the gradient carries one
// fp32 rounding.  Padding columns (c >= C) of rec / grad_pre are written as zeros.
__global__ __launch_bounds__(256) void l1_nll_kernel(const float* __restrict__ pre, int ld, int act, const float* __restrict__ x, int N, int C,
                                                     int S, long x_sn, const float* __restrict__ logvar, float* __restrict__ rec, int ld_rec,
                                                     float* __restrict__ grad_pre, int ld_grad, double* __restrict__ partials) {
  __shared__ double red[4];
  const long total = (long)N * S * ld;
  const double k = (grad_pre && logvar) ? exp(-(double)logvar[0]) / (double)N : 0.0;
  double acc = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long m = i / ld; const int c = (int)(i - m * ld);
    if (c >= C) {
      if (c < ld_rec) rec[m * ld_rec + c] = 0.f;
      if (grad_pre && c < ld_grad) grad_pre[m * ld_grad + c] = 0.f;
      continue;
    }
    const float f = pre[i];
    double t = (double)f, dact = 1.0;
    if (act == IPOKE_ACT_TANH) { t = tanh((double)f); dact = 1.0 - t * t; }
    const float r = (float)t;
    rec[m * ld_rec + c] = r;
    if (x) {
      const int n = (int)(m / S), s = (int)(m - (long)n * S);
      const float d = r - x[(long)n * x_sn + (long)c * S + s];
      acc += (double)fabsf(d);
      if (grad_pre) grad_pre[m * ld_grad + c] = d > 0.f ? (float)(k * dact) : (d < 0.f ? (float)(-k * dact) : 0.f);
    }
  }
  if (partials) {
    const double tot = block_sum_f64(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = tot;
  }
}

// out[0] = nll, out[1] = sum |x - rec|, out[2] = d nll / d logvar; grad_p[n] = C * S * w * exp(-logvar) / N
__global__ __launch_bounds__(256) void l1_nll_final_kernel(const double* __restrict__ partials, int n_part, const float* __restrict__ logvar,
                                                           const float* __restrict__ p, const float* __restrict__ perc_weight, int N, int C,
                                                           int S, float* __restrict__ out, float* __restrict__ grad_p) {
  __shared__ double red[4];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < n_part; i += 256) a += partials[i];
  if (p) for (int i = threadIdx.x; i < N; i += 256) b += (double)p[i];
  a = block_sum_f64(a, red);
  b = block_sum_f64(b, red);
  const double lv = (double)logvar[0], cs = (double)C * (double)S;
  const double w = p ? (double)perc_weight[0] : 0.0;
  const double k = exp(-lv) / (double)N;
  if (threadIdx.x == 0) {
    const double data = (a + cs * w * b) * k;
    out[0] = (float)(data + cs * lv);
    out[1] = (float)a;
    out[2] = (float)(cs - data);
  }
  if (grad_p) for (int i = threadIdx.x; i < N; i += 256) grad_p[i] = (float)(cs * w * k);
}

}  // namespace ipoke

using namespace ipoke;
#define STREAM(s) reinterpret_cast<hipStream_t>(s)

extern "C" long ipoke_l1_nll_partials(void) { return kNllBlocks; }

extern "C" int ipoke_l1_nll(const float* pre_cl, int ld, int act, const float* x_nchw, int N, int C, int S, int64_t x_sn,
                            const float* logvar, const float* p, const float* perc_weight, float* out, float* rec_cl, int ld_rec,
                            float* grad_pre, int ld_grad, float* grad_p, double* partials, void* stream) {
  IPK_REQUIRE(pre_cl && rec_cl && N > 0 && C > 0 && S > 0 && ld >= C && ld_rec >= C, "bad arguments");
  IPK_REQUIRE(act == IPOKE_ACT_NONE || act == IPOKE_ACT_TANH, "the autoencoders' output activation is none or tanh");
  IPK_REQUIRE(!x_nchw || (logvar && out && partials && x_sn >= (int64_t)C * S), "a target needs logvar, out and the partials scratch");
  IPK_REQUIRE(x_nchw || (!grad_pre && !p && !grad_p), "gradients and the perceptual term need a target");
  IPK_REQUIRE(!grad_pre || ld_grad >= C, "grad_pre pitch must cover the channels");
  IPK_REQUIRE((p != nullptr) == (perc_weight != nullptr), "p and perc_weight come together");
  IPK_REQUIRE(!grad_p || p, "grad_p needs p");
  const long total = (long)N * S * ld;
  long g = (total + 255) / 256;
  g = g < 1 ? 1 : (g > kNllBlocks ? kNllBlocks : g);
  hipLaunchKernelGGL(l1_nll_kernel, dim3((int)g), dim3(256), 0, STREAM(stream), pre_cl, ld, act, x_nchw, N, C, S, (long)x_sn, logvar, rec_cl,
                     ld_rec, grad_pre, ld_grad, x_nchw ? partials : nullptr);
  IPK_LAUNCH_CHECK();
  if (x_nchw) {
    hipLaunchKernelGGL(l1_nll_final_kernel, dim3(1), dim3(256), 0, STREAM(stream), (const double*)partials, (int)g, logvar, p, perc_weight, N, C,
                       S, out, grad_p);
    IPK_LAUNCH_CHECK();
  }
  return IPOKE_OK;
}
