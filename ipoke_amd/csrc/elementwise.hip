// Element-wise / reduction kernels of the flow: ActNorm (+fused channel permutation), affine coupling
// transform with log-det, NLL loss, layout conversion, fused Adam-amsgrad.  All arithmetic fp32.
//
// Flow state layout: S[B*64][ld] fp32, row = (sample, position), columns = channels ("positions
// major").  A layer acting on the first C channels leaves columns >= C untouched (they are the
// channels the multi-scale architecture has already split off, reference macow2.py:888-899).
#include "common.h"
#ifndef IPK_CHAIN_PRIO
#define IPK_CHAIN_PRIO 1      // the chain's elementwise kernels raise their wave priority like its GEMMs (gemm.hip)
#endif

namespace ipoke {

// ------------------------------------------------------------------ layout conversion
// NCHW [B][C][P] <-> state [B][P][ld]; one block per sample.
__global__ void nchw_to_state_kernel(const float* __restrict__ x, float* __restrict__ s, int C, int P, int ld) {
  const int b = blockIdx.x;
  const float* xb = x + (long)b * C * P;
  float* sb = s + (long)b * P * ld;
  const FDiv fP(P);
  for (int i = threadIdx.x; i < C * P; i += blockDim.x) {
    const int c = fP.div(i), p = i - c * P;        // read coalesced along p
    sb[(long)p * ld + c] = xb[i];
  }
}
__global__ void state_to_nchw_kernel(const float* __restrict__ s, float* __restrict__ x, int C, int P, int ld) {
  const int b = blockIdx.x;
  float* xb = x + (long)b * C * P;
  const float* sb = s + (long)b * P * ld;
  const FDiv fP(P);
  for (int i = threadIdx.x; i < C * P; i += blockDim.x) {
    const int c = fP.div(i), p = i - c * P;
    xb[i] = sb[(long)p * ld + c];
  }
}
// cond [B][Cc][P] fp32 -> ELU -> T [B][P][Cc]   (the MCF blocks concatenate h before their ELU,
// macow_utils.py:429-431, so ELU(h) is shared by all 800 blocks and computed once)
template <typename T>
__global__ void cond_prepare_kernel(const float* __restrict__ h, T* __restrict__ out, int Cc, int P, int act) {
  const int b = blockIdx.x;
  const float* hb = h + (long)b * Cc * P;
  T* ob = out + (long)b * P * Cc;
  const FDiv fP(P);
  for (int i = threadIdx.x; i < Cc * P; i += blockDim.x) {
    const int c = fP.div(i), p = i - c * P;
    ob[(long)p * Cc + c] = ET<T>::from_f32(act_apply(act, hb[i]));
  }
}

// out[m][j] = T(state[m][off + j*stride]) for j < C, zero for C <= j < ldo  (conditioning channels of a NICE coupling,
// continuous or even/odd "skip" split: macow2.py:364-375) -- gives the coupling net a dense, padded operand.
template <typename T>
__global__ void extract_cols_kernel(const float* __restrict__ s, int ld, int off, int stride, int C, T* __restrict__ out, int ldo,
                                    long M) {
  if (IPK_CHAIN_PRIO) __builtin_amdgcn_s_setprio(2);
  const long total = M * ldo;
  const FDiv fldo(ldo);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long m = fldo.div(i); const int j = (int)(i - m * ldo);
    out[i] = ET<T>::from_f32(j < C ? s[m * ld + off + (long)j * stride] : 0.f);
  }
}

// dst[m][0:C] = src[m][0:C], both in the matrix cores' dtype, 16 bytes per thread (condition_nice: the activated conditioning map
// behind conv2's output in the coupling net's hidden tile, macow_utils.py:328-332)
__global__ void copy_cols16_kernel(const u32x4* __restrict__ src, long lds16, u32x4* __restrict__ dst, long ldd16, int c16, long M) {
  if (IPK_CHAIN_PRIO) __builtin_amdgcn_s_setprio(2);
  const long total = M * c16;
  const FDiv fc16(c16);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long m = fc16.div(i); const int j = (int)(i - m * c16);
    dst[m * ldd16 + j] = src[m * lds16 + j];
  }
}

// ------------------------------------------------------------------ ActNorm (+ Shuffle)
// out[m][c0 + j] = in[m][c0 + idx[j]] * exp(ls[idx[j]]) + bias[idx[j]]   (idx == NULL: identity)
// ls/bias == NULL: pure permutation.  Columns outside [c0, c0+C) are copied.
__global__ void actnorm_fwd_kernel(const float* __restrict__ in, float* __restrict__ out, int M, int ld, int c0, int C,
                                   const float* __restrict__ ls, const float* __restrict__ bias,
                                   const int* __restrict__ idx) {
  if (IPK_CHAIN_PRIO) __builtin_amdgcn_s_setprio(2);
  const long total = (long)M * ld;
  const FDiv fld(ld);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int col = fld.mod(i);
    const long row = fld.div(i);
    const int j = col - c0;
    float v;
    if (j >= 0 && j < C) {
      const int src = idx ? idx[j] : j;
      v = in[row * ld + c0 + src];
      if (ls) v = v * expf(ls[src]) + bias[src];
    } else {
      v = in[i];
    }
    out[i] = v;
  }
}
// inverse: first undo the permutation (x'[idx[j]] = y[j]), then x = (x' - bias) / (exp(ls) + 1e-8)
__global__ void actnorm_inv_kernel(const float* __restrict__ in, float* __restrict__ out, int M, int ld, int c0, int C,
                                   const float* __restrict__ ls, const float* __restrict__ bias,
                                   const int* __restrict__ inv_idx) {
  const long total = (long)M * ld;
  const FDiv fld(ld);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int col = fld.mod(i);
    const long row = fld.div(i);
    const int c = col - c0;
    float v;
    if (c >= 0 && c < C) {
      const int src = inv_idx ? inv_idx[c] : c;     // out channel c came from shuffled position src
      v = in[row * ld + c0 + src];
      if (ls) v = (v - bias[c]) / (expf(ls[c]) + 1e-8f);
    } else {
      v = in[i];
    }
    out[i] = v;
  }
}
// The same with the conditioning operand of the coupling inverted NEXT as a second output (what extract_cols would read back out of
// `out` in a launch of its own): ext[m][j] = T(out[m][e_off + j*e_stride]) for j < e_C, zero for e_C <= j < ext_ld (ext_ld - e_C <= ld)
template <typename T>
__global__ void actnorm_inv_ext_kernel(const float* __restrict__ in, float* __restrict__ out, int M, int ld, int c0, int C,
                                       const float* __restrict__ ls, const float* __restrict__ bias,
                                       const int* __restrict__ inv_idx, T* __restrict__ ext, int ext_ld, int e_off, int e_stride,
                                       int e_C) {
  const long total = (long)M * ld;
  const int pad = ext_ld - e_C;
  const FDiv fld(ld), fes(e_stride);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int col = fld.mod(i);
    const long row = fld.div(i);
    const int c = col - c0;
    float v;
    if (c >= 0 && c < C) {
      const int src = inv_idx ? inv_idx[c] : c;
      v = in[row * ld + c0 + src];
      if (ls) v = (v - bias[c]) / (expf(ls[c]) + 1e-8f);
    } else {
      v = in[i];
    }
    out[i] = v;
    const int rel = col - e_off;
    if (fes.strided_hit(rel, e_C)) ext[row * ext_ld + fes.div(rel)] = ET<T>::from_f32(v);
    if (col < pad) ext[row * ext_ld + e_C + col] = ET<T>::from_f32(0.f);
  }
}
// backward.  x = saved input of the layer.  One block per sample; per-sample partial sums of the
// parameter gradients go to part[b][2C] (reduced over b by ipoke_reduce_rows):
//   dx[m][c0+idx[j]] = dy[m][c0+j] * exp(ls[idx[j]])
//   dls[c] = sum_m dy'[m][c] * x[m][c] * exp(ls[c]) + P * sum_b dld[b] ;  dbias[c] = sum_m dy'[m][c]
__global__ __launch_bounds__(1024) void actnorm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                           float* __restrict__ dx, int P, int ld, int c0, int C,
                                                           const float* __restrict__ ls, const int* __restrict__ idx,
                                                           const float* __restrict__ dld, float* __restrict__ part) {
  if (IPK_CHAIN_PRIO) __builtin_amdgcn_s_setprio(2);
  extern __shared__ float sm[];   // [2][rows_par][C]
  const int tid = threadIdx.x, b = blockIdx.x;
  const long row0 = (long)b * P;
  const FDiv fC(C), fld(ld);
  const int rows_par = fC.div((int)blockDim.x);      // host guarantees >= 1
  const int j = fC.mod(tid), r0 = fC.div(tid);
  // pass-through columns first (independent of everything else), four elements per thread in flight
  for (int i0 = tid; i0 < P * ld; i0 += 4 * blockDim.x) {
    float v[4]; bool w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * blockDim.x;
      const int col = fld.mod(i);
      w[u] = i < P * ld && (col < c0 || col >= c0 + C);
      if (w[u]) v[u] = dy[row0 * ld + i];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) if (w[u]) dx[row0 * ld + i0 + u * blockDim.x] = v[u];
  }
  float a_ls = 0.f, a_b = 0.f;
  if (r0 < rows_par) {
    const int src = idx ? idx[j] : j;
    const float e = ls ? expf(ls[src]) : 1.f;
    for (int m0 = r0; m0 < P; m0 += 4 * rows_par) {       // four rows per thread with all loads in flight
      float g[4], xv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int m = m0 + u * rows_par;
        g[u] = 0.f; xv[u] = 0.f;
        if (m < P) {
          g[u] = dy[(row0 + m) * ld + c0 + j];
          if (ls) xv[u] = x[(row0 + m) * ld + c0 + src];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int m = m0 + u * rows_par;
        if (m < P) {
          dx[(row0 + m) * ld + c0 + src] = g[u] * e;
          a_ls += g[u] * xv[u] * e;
          a_b += g[u];
        }
      }
    }
  }
  if (!ls) return;
  if (r0 < rows_par) { sm[r0 * C + j] = a_ls; sm[(rows_par + r0) * C + j] = a_b; }
  __syncthreads();
  if (tid < C) {
    const int s = idx ? idx[tid] : tid;     // thread tid accumulated channel s
    float t_ls = 0.f, t_b = 0.f;
    for (int r = 0; r < rows_par; ++r) { t_ls += sm[r * C + tid]; t_b += sm[(rows_par + r) * C + tid]; }
    part[(long)b * 2 * C + s] = t_ls + (float)P * dld[b];
    part[(long)b * 2 * C + C + s] = t_b;
  }
}
// data-dependent init (reference macow2.py:526-539): statistics of y0 = x*exp(ls0)+b0 over all rows,
// unbiased std, then ls <- log(1/(std+1e-6)), bias <- -mean/(std+1e-6).  One block per channel.
__global__ void actnorm_init_kernel(const float* __restrict__ x, int M, int ld, int c0, float* __restrict__ ls,
                                    float* __restrict__ bias) {
  __shared__ float red[8];
  const int c = blockIdx.x;
  const float e = expf(ls[c]), b0 = bias[c];
  float s = 0.f;
  for (int m = threadIdx.x; m < M; m += blockDim.x) s += x[(long)m * ld + c0 + c] * e + b0;
  const float mean = block_sum(s, red) / (float)M;
  float v = 0.f;
  for (int m = threadIdx.x; m < M; m += blockDim.x) {
    const float d = x[(long)m * ld + c0 + c] * e + b0 - mean;
    v += d * d;
  }
  const float var = block_sum(v, red) / (float)(M - 1);
  if (threadIdx.x == 0) {
    const float inv = 1.f / (sqrtf(var) + 1e-6f);
    ls[c] = logf(inv);
    bias[c] = -mean * inv;
  }
}

// ------------------------------------------------------------------ affine coupling transform
// raw[m][0:Cp] = mu, raw[m][Cp:2Cp] = s, given as `nsplit` fp32 partial sums (split-K conv output)
// plus bias.  scale = tanh(s/2)+1 (macow_utils.py:49-52);  transformed channel i lives in state
// column t_off + i*t_stride.  One block per sample: the per-sample log-det is a block reduction.
struct AffineArgs {
  const float* raw; int nsplit; long split_stride; int ldraw;     // raw + s*split_stride + m*ldraw + col
  const float* bias;                                              // [2*Cp] or NULL
  int Cp, t_off, t_stride;
  int P, ld;
};
constexpr int kAffPre = 2;      // transformed elements per thread requested ahead (256 threads: 16 rows x <= 32 channels)
// sum the split-K partials (+bias) of `rows` positions starting at row0 into LDS: raw_s[p][0:2Cp]
__device__ __forceinline__ void affine_stage_raw(const AffineArgs& a, long row0, int rows, float* raw_s) {
  const int n2 = 2 * a.Cp;
  const FDiv fn2(n2);
  for (int e = threadIdx.x; e < rows * n2; e += blockDim.x) {
    const int p = fn2.div(e), j = e - p * n2;
    const float* r = a.raw + (row0 + p) * a.ldraw + j;
    // every split's partial is requested at once (nsplit <= 32): one memory latency instead of nsplit / 8
    float v[32];
#pragma unroll
    for (int u = 0; u < 32; ++u) v[u] = u < a.nsplit ? r[(long)u * a.split_stride] : 0.f;
    for (int s = 32; s < a.nsplit; ++s) v[0] += r[(long)s * a.split_stride];
#pragma unroll
    for (int w = 16; w >= 1; w >>= 1)
#pragma unroll
      for (int u = 0; u < w; ++u) v[u] += v[u + w];
    float t = v[0];
    if (a.bias) t += a.bias[j];
    raw_s[e] = t;
  }
  __syncthreads();
}
// untouched channels of `rows` positions: out = in
__device__ __forceinline__ void affine_copy_rest(const AffineArgs& a, long row0, int rows, const float* __restrict__ in,
                                                 float* __restrict__ out) {
  const int total = rows * a.ld;
  const FDiv fld(a.ld), fts(a.t_stride);
  for (int i0 = threadIdx.x; i0 < total; i0 += 4 * blockDim.x) {
    float v[4]; bool w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * blockDim.x;
      const int col = fld.mod(i);
      const bool transformed = fts.strided_hit(col - a.t_off, a.Cp);
      w[u] = i < total && !transformed;
      if (w[u]) v[u] = in[row0 * a.ld + i];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) if (w[u]) out[row0 * a.ld + i0 + u * blockDim.x] = v[u];
  }
}
// grid = B * Q: Q slices of P/Q positions per sample (Q = 4 when the log-det slot is 4 wide, like the MCF kernels)
// ext (optional): the transformed channels once more as a dense, zero-padded [M][ext_ld] operand of the compute dtype -- the
// conditioning input of the NEXT coupling when that one conditions on exactly these channels (coupling*_up -> coupling*_dn),
// which saves its extract_cols launch
template <typename T>
__device__ __forceinline__ void affine_ext_store(void* ext, int ext_ld, long row, int i, float v) {
  reinterpret_cast<T*>(ext)[row * ext_ld + i] = ET<T>::from_f32(v);
}
__device__ __forceinline__ void affine_ext_pad(const AffineArgs& a, void* ext, int ext_ld, int ext_bf16, long row0, int rows) {
  const int pad = ext_ld - a.Cp;
  for (int e = threadIdx.x; e < rows * pad; e += blockDim.x) {
    const int p = e / pad, i = a.Cp + (e - p * pad);
    if (ext_bf16) affine_ext_store<bf16_t>(ext, ext_ld, row0 + p, i, 0.f); else affine_ext_store<float>(ext, ext_ld, row0 + p, i, 0.f);
  }
}
__global__ void affine_fwd_kernel(AffineArgs a, const float* __restrict__ in, float* __restrict__ out,
                                  float* __restrict__ scale_out, float* __restrict__ logdet_slot, int slot_stride, int Q,
                                  void* __restrict__ ext, int ext_ld, int ext_bf16) {
  kernarg_prefetch<(int)sizeof(AffineArgs) + 64>();
  if (IPK_CHAIN_PRIO) __builtin_amdgcn_s_setprio(2);
  extern __shared__ float raw_s[];
  __shared__ float red[8];
  const int b = blockIdx.x / Q, q = blockIdx.x % Q;
  const int rows = a.P / Q;
  const long row0 = (long)b * a.P + (long)q * rows;
  const FDiv fCp(a.Cp);
  // the transformed channels' inputs are requested BEFORE the split-K partials are staged (they used to be loaded behind the staging
  // barrier: one more dependent memory round trip in a kernel that is nothing but such round trips)
  float xin[kAffPre];
#pragma unroll
  for (int u = 0; u < kAffPre; ++u) {
    const int e = threadIdx.x + u * blockDim.x;
    xin[u] = 0.f;
    if (e < rows * a.Cp) { const int p = fCp.div(e), i = e - p * a.Cp; xin[u] = in[(row0 + p) * a.ld + a.t_off + (long)i * a.t_stride]; }
  }
  affine_copy_rest(a, row0, rows, in, out);
  affine_stage_raw(a, row0, rows, raw_s);
  float ld_acc = 0.f;
  for (int e = threadIdx.x, u = 0; e < rows * a.Cp; e += blockDim.x, ++u) {
    const int p = fCp.div(e), i = e - p * a.Cp;
    const float mu = raw_s[p * 2 * a.Cp + i];
    const float sc = tanhf(0.5f * raw_s[p * 2 * a.Cp + a.Cp + i]) + 1.f;
    const long off = (row0 + p) * a.ld + a.t_off + (long)i * a.t_stride;
    const float y = sc * (u < kAffPre ? xin[u < kAffPre ? u : 0] : in[off]) + mu;
    out[off] = y;
    if (ext) { if (ext_bf16) affine_ext_store<bf16_t>(ext, ext_ld, row0 + p, i, y); else affine_ext_store<float>(ext, ext_ld, row0 + p, i, y); }
    if (scale_out) scale_out[(row0 + p) * a.Cp + i] = sc;
    ld_acc += logf(sc);
  }
  if (ext && ext_ld > a.Cp) affine_ext_pad(a, ext, ext_ld, ext_bf16, row0, rows);
  const float tot = block_sum(ld_acc, red);
  if (threadIdx.x == 0 && logdet_slot) logdet_slot[(long)b * slot_stride + q] = tot;
}
__global__ void affine_inv_kernel(AffineArgs a, const float* __restrict__ in, float* __restrict__ out, int Q,
                                  void* __restrict__ ext, int ext_ld, int ext_bf16) {
  extern __shared__ float raw_s[];
  const int b = blockIdx.x / Q, q = blockIdx.x % Q;
  const int rows = a.P / Q;
  const long row0 = (long)b * a.P + (long)q * rows;
  const FDiv fCp(a.Cp);
  float xin[kAffPre];                      // (requested before the staging of the partials: see affine_fwd_kernel)
#pragma unroll
  for (int u = 0; u < kAffPre; ++u) {
    const int e = threadIdx.x + u * blockDim.x;
    xin[u] = 0.f;
    if (e < rows * a.Cp) { const int p = fCp.div(e), i = e - p * a.Cp; xin[u] = in[(row0 + p) * a.ld + a.t_off + (long)i * a.t_stride]; }
  }
  affine_copy_rest(a, row0, rows, in, out);
  affine_stage_raw(a, row0, rows, raw_s);
  for (int e = threadIdx.x, u = 0; e < rows * a.Cp; e += blockDim.x, ++u) {
    const int p = fCp.div(e), i = e - p * a.Cp;
    const float mu = raw_s[p * 2 * a.Cp + i];
    const float sc = tanhf(0.5f * raw_s[p * 2 * a.Cp + a.Cp + i]) + 1.f;
    const long off = (row0 + p) * a.ld + a.t_off + (long)i * a.t_stride;
    const float y = ((u < kAffPre ? xin[u < kAffPre ? u : 0] : in[off]) - mu) / (sc + 1e-12f);      // macow_utils.py:64
    out[off] = y;
    if (ext) { if (ext_bf16) affine_ext_store<bf16_t>(ext, ext_ld, row0 + p, i, y); else affine_ext_store<float>(ext, ext_ld, row0 + p, i, y); }
  }
  if (ext && ext_ld > a.Cp) affine_ext_pad(a, ext, ext_ld, ext_bf16, row0, rows);
}
// backward.  x = saved layer input, scale = saved scales.  Produces
//   dx (zp channels: dy*scale, others: dy copied),  dparams T [m][ldp] = [dmu | ds | 0 pad],
//   per-sample column sums of dparams (for the conv bias gradient) into dbias_part[b][2Cp].
template <typename T>
__global__ __launch_bounds__(1024) void affine_bwd_kernel(int Cp, int t_off, int t_stride, int P, int ld,
                                                          const float* __restrict__ dy, const float* __restrict__ x,
                                                          const float* __restrict__ scale, const float* __restrict__ dld,
                                                          float* __restrict__ dx, T* __restrict__ dparams, int ldp,
                                                          float* __restrict__ dbias_part) {
  kernarg_prefetch<84>();
  if (IPK_CHAIN_PRIO) __builtin_amdgcn_s_setprio(2);
  // Thread (r0, i) owns transformed channel i of rows r0, r0 + rows_par, ...: it loads (dy, scale, x) once for BOTH outputs
  // (d mu, d s), keeps their column sums in registers and hands them to a deterministic LDS reduction.  (Rounds 1-2: every
  // element of dparams was its own work item -- dy and scale loaded twice -- and the column sums were 2 Cp * P LDS float
  // atomics on 2 Cp addresses: 11.5 us per launch in the train step, 215 launches per step.)
  extern __shared__ float sm[];      // [rows_par][2*Cp] partial column sums
  const int b = blockIdx.x, tid = threadIdx.x;
  const long row0 = (long)b * P;
  const FDiv fCp(Cp), fld(ld), fts(t_stride);
  const int rows_par = fCp.div((int)blockDim.x);        // host guarantees Cp <= blockDim.x
  const int i = fCp.mod(tid), r0 = fCp.div(tid);
  const float g_ld = dld[b];
  // this thread's elements first (their loads head the queue), then the untouched channels
  float g[4], sc[4], xv[4];
  float a_mu = 0.f, a_s = 0.f;
  const bool act = r0 < rows_par;
  for (int m0 = r0; act && m0 < P; m0 += 4 * rows_par) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = m0 + u * rows_par;
      g[u] = 0.f; sc[u] = 1.f; xv[u] = 0.f;
      if (m < P) {
        const long off = (row0 + m) * ld + t_off + (long)i * t_stride;
        g[u] = dy[off]; xv[u] = x[off];
        sc[u] = scale[(row0 + m) * Cp + i];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = m0 + u * rows_par;
      if (m < P) {
        const float t = sc[u] - 1.f;                                         // tanh(s/2)
        const float ds = (g[u] * xv[u] + g_ld / sc[u]) * 0.5f * (1.f - t * t);
        dx[(row0 + m) * ld + t_off + (long)i * t_stride] = g[u] * sc[u];
        dparams[(row0 + m) * ldp + i] = ET<T>::from_f32(g[u]);               // d mu
        dparams[(row0 + m) * ldp + Cp + i] = ET<T>::from_f32(ds);            // d s
        a_mu += g[u]; a_s += ds;
      }
    }
  }
  if (act) { sm[r0 * 2 * Cp + i] = a_mu; sm[r0 * 2 * Cp + Cp + i] = a_s; }
  {   // untouched channels: four elements per thread in flight
    const int total = P * ld;
    for (int i0 = tid; i0 < total; i0 += 4 * blockDim.x) {
      float v[4]; bool w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = i0 + u * blockDim.x;
        const int col = fld.mod(e);
        const bool transformed = fts.strided_hit(col - t_off, Cp);
        w[u] = e < total && !transformed;
        if (w[u]) v[u] = dy[row0 * ld + e];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) if (w[u]) dx[row0 * ld + i0 + u * blockDim.x] = v[u];
    }
  }
  {   // K padding of dparams (read by the conv3 data-gradient and weight-gradient GEMMs)
    const int pad = ldp - 2 * Cp;
    const FDiv fpad(pad);
    for (int e = tid; e < P * pad; e += blockDim.x) {
      const int p = fpad.div(e), j = 2 * Cp + (e - p * pad);
      dparams[(row0 + p) * ldp + j] = ET<T>::from_f32(0.f);
    }
  }
  __syncthreads();
  if (dbias_part && tid < 2 * Cp) {
    const int used = rows_par < P ? rows_par : P;
    float t = 0.f;
    for (int r = 0; r < used; ++r) t += sm[r * 2 * Cp + tid];
    dbias_part[(long)b * 2 * Cp + tid] = t;
  }
}
// ------------------------------------------------------------------ affine coupling + the ActNorm (+ Shuffle) that follows it
// MaCowStep / MultiScalePrior put an ActNorm2dFlow (optionally with a channel shuffle) right behind a coupling (macow2.py:1066-1117,
// 569-593).  Both are row-wise maps of the [M][ld] state; as two launches they cost two dependent kernel boundaries and two round trips
// through memory for 330 KB of state.  Fused: the block keeps its rows of the coupling's output in LDS (the shuffle needs whole rows)
// and writes BOTH states -- `out` (the coupling's output = the ActNorm's saved input, may be NULL when nothing is saved) and `out2`.
struct ActNormArgs { int c0, C; const float* ls; const float* bias; const int* idx; };
__global__ void affine_actnorm_fwd_kernel(AffineArgs a, ActNormArgs n, const float* __restrict__ in, float* __restrict__ out,
                                          float* __restrict__ out2, float* __restrict__ scale_out, float* __restrict__ logdet_slot,
                                          int slot_stride, int Q) {
  kernarg_prefetch<(int)(sizeof(AffineArgs) + sizeof(ActNormArgs)) + 48>();
  if (IPK_CHAIN_PRIO) __builtin_amdgcn_s_setprio(2);
  extern __shared__ float raw_s[];                 // [rows][2Cp] raw (mu, s), then [rows][ld] the coupling's output rows
  __shared__ float red[8];
  const int b = blockIdx.x / Q, q = blockIdx.x % Q;
  const int rows = a.P / Q;
  const long row0 = (long)b * a.P + (long)q * rows;
  const FDiv fCp(a.Cp);
  float* tile = raw_s + rows * 2 * a.Cp;
  // requested ahead of everything that waits: the transformed channels' inputs and -- when a thread keeps its column over the rows it
  // writes (blockDim a multiple of ld) -- the ActNorm parameters of that column (index, then scale / bias: two dependent loads that
  // used to sit behind the last barrier)
  float xin[kAffPre];
#pragma unroll
  for (int u = 0; u < kAffPre; ++u) {
    const int e = threadIdx.x + u * blockDim.x;
    xin[u] = 0.f;
    if (e < rows * a.Cp) { const int p = fCp.div(e), i = e - p * a.Cp; xin[u] = in[(row0 + p) * a.ld + a.t_off + (long)i * a.t_stride]; }
  }
  const FDiv fld(a.ld), fts(a.t_stride);
  const bool col_fixed = fld.mod((int)blockDim.x) == 0;
  int an_src = -1; float an_e = 1.f, an_b = 0.f;
  if (col_fixed) {
    const int j = fld.mod((int)threadIdx.x) - n.c0;
    if (j >= 0 && j < n.C) {
      an_src = n.idx ? n.idx[j] : j;
      if (n.ls) { an_e = expf(n.ls[an_src]); an_b = n.bias[an_src]; }
    }
  }
  {   // untouched channels -> tile (and `out`)
    const int total = rows * a.ld;
    for (int i0 = threadIdx.x; i0 < total; i0 += 4 * blockDim.x) {
      float v[4]; bool w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * blockDim.x;
        const int col = fld.mod(i);
        const bool transformed = fts.strided_hit(col - a.t_off, a.Cp);
        w[u] = i < total && !transformed;
        if (w[u]) v[u] = in[row0 * a.ld + i];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (w[u]) { tile[i0 + u * blockDim.x] = v[u]; if (out) out[row0 * a.ld + i0 + u * blockDim.x] = v[u]; }
    }
  }
  affine_stage_raw(a, row0, rows, raw_s);
  float ld_acc = 0.f;
  for (int e = threadIdx.x, u = 0; e < rows * a.Cp; e += blockDim.x, ++u) {
    const int p = fCp.div(e), i = e - p * a.Cp;
    const float mu = raw_s[p * 2 * a.Cp + i];
    const float sc = tanhf(0.5f * raw_s[p * 2 * a.Cp + a.Cp + i]) + 1.f;
    const int col = a.t_off + i * a.t_stride;
    const long off = (row0 + p) * a.ld + col;
    const float y = sc * (u < kAffPre ? xin[u < kAffPre ? u : 0] : in[off]) + mu;
    tile[p * a.ld + col] = y;
    if (out) out[off] = y;
    if (scale_out) scale_out[(row0 + p) * a.Cp + i] = sc;
    ld_acc += logf(sc);
  }
  const float tot = block_sum(ld_acc, red);          // (its barriers also publish the tile)
  if (threadIdx.x == 0 && logdet_slot) logdet_slot[(long)b * slot_stride + q] = tot;
  for (int e = threadIdx.x; e < rows * a.ld; e += blockDim.x) {
    const int p = fld.div(e), col = e - p * a.ld;
    const int j = col - n.c0;
    float v;
    if (j >= 0 && j < n.C) {
      if (col_fixed) {
        v = tile[p * a.ld + n.c0 + an_src];
        if (n.ls) v = v * an_e + an_b;
      } else {
        const int src = n.idx ? n.idx[j] : j;
        v = tile[p * a.ld + n.c0 + src];
        if (n.ls) v = v * expf(n.ls[src]) + n.bias[src];
      }
    } else {
      v = tile[e];
    }
    out2[(row0 + p) * a.ld + col] = v;
  }
}

// backward of that pair in one launch: dy2 = gradient w.r.t. the ActNorm's output, x1 = its saved input (the coupling's output), x0 = the
// coupling's saved input.  Phase A is actnorm_bwd_kernel with the gradient it passes on kept in LDS ([P][ld]), phase B affine_bwd_kernel
// reading it from there.  part: [B][2 C] ActNorm partials (NULL without parameters), dbias_part: [B][2 Cp] coupling-bias partials.
template <typename T>
__global__ __launch_bounds__(1024) void actnorm_affine_bwd_kernel(ActNormArgs n, int Cp, int t_off, int t_stride, int P, int ld,
                                                                  const float* __restrict__ dy2, const float* __restrict__ x1,
                                                                  const float* __restrict__ x0, const float* __restrict__ scale,
                                                                  const float* __restrict__ dld, float* __restrict__ dx,
                                                                  T* __restrict__ dparams, int ldp, float* __restrict__ part,
                                                                  float* __restrict__ dbias_part) {
  kernarg_prefetch<(int)sizeof(ActNormArgs) + 96>();
  if (IPK_CHAIN_PRIO) __builtin_amdgcn_s_setprio(2);
  extern __shared__ float sm[];                    // [P][ld] gradient w.r.t. the coupling's output, then the partial-sum area
  const int tid = threadIdx.x, b = blockIdx.x;
  const long row0 = (long)b * P;
  float* g1 = sm;
  float* ps = sm + P * ld;                         // max(2 * rows_par_n * C, rows_par_a * 2 * Cp) floats
  const float g_ld = dld[b];
  // ---- phase A: ActNorm (+ shuffle) backward into the LDS tile
  {
    const int C = n.C, c0 = n.c0;
    const FDiv fC(C);
    const int rows_par = fC.div((int)blockDim.x);
    const int j = fC.mod(tid), r0 = fC.div(tid);
    float a_ls = 0.f, a_b = 0.f;
    if (r0 < rows_par) {
      const int src = n.idx ? n.idx[j] : j;
      const float e = n.ls ? expf(n.ls[src]) : 1.f;
      for (int m0 = r0; m0 < P; m0 += 4 * rows_par) {
        float g[4], xv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int m = m0 + u * rows_par;
          g[u] = 0.f; xv[u] = 0.f;
          if (m < P) {
            g[u] = dy2[(row0 + m) * ld + c0 + j];
            if (n.ls) xv[u] = x1[(row0 + m) * ld + c0 + src];
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int m = m0 + u * rows_par;
          if (m < P) {
            g1[m * ld + c0 + src] = g[u] * e;
            a_ls += g[u] * xv[u] * e;
            a_b += g[u];
          }
        }
      }
    }
    if (C < ld) {        // columns outside the ActNorm window pass through
      const int rest = ld - C;
      const FDiv frest(rest);
      for (int e = tid; e < P * rest; e += blockDim.x) {
        const int m = frest.div(e), k = e - m * rest;
        const int col = k < c0 ? k : k + C;
        g1[m * ld + col] = dy2[(row0 + m) * ld + col];
      }
    }
    if (n.ls && r0 < rows_par) { ps[r0 * C + j] = a_ls; ps[(rows_par + r0) * C + j] = a_b; }
    __syncthreads();
    if (n.ls && tid < C) {
      const int s_ = n.idx ? n.idx[tid] : tid;     // thread tid accumulated channel s_
      float t_ls = 0.f, t_b = 0.f;
      for (int r = 0; r < rows_par; ++r) { t_ls += ps[r * C + tid]; t_b += ps[(rows_par + r) * C + tid]; }
      part[(long)b * 2 * C + s_] = t_ls + (float)P * g_ld;
      part[(long)b * 2 * C + C + s_] = t_b;
    }
    __syncthreads();                                // ps is reused below
  }
  // ---- phase B: the coupling's backward, its incoming gradient read from the tile
  const FDiv fCp(Cp), fld(ld), fts(t_stride);
  const int rows_par = fCp.div((int)blockDim.x);
  const int i = fCp.mod(tid), r0 = fCp.div(tid);
  float a_mu = 0.f, a_s = 0.f;
  const bool act = r0 < rows_par;
  for (int m0 = r0; act && m0 < P; m0 += 4 * rows_par) {
    float g[4], sc[4], xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = m0 + u * rows_par;
      g[u] = 0.f; sc[u] = 1.f; xv[u] = 0.f;
      if (m < P) {
        const int col = t_off + i * t_stride;
        g[u] = g1[m * ld + col]; xv[u] = x0[(row0 + m) * ld + col];
        sc[u] = scale[(row0 + m) * Cp + i];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int m = m0 + u * rows_par;
      if (m < P) {
        const float t = sc[u] - 1.f;
        const float ds = (g[u] * xv[u] + g_ld / sc[u]) * 0.5f * (1.f - t * t);
        dx[(row0 + m) * ld + t_off + (long)i * t_stride] = g[u] * sc[u];
        dparams[(row0 + m) * ldp + i] = ET<T>::from_f32(g[u]);
        dparams[(row0 + m) * ldp + Cp + i] = ET<T>::from_f32(ds);
        a_mu += g[u]; a_s += ds;
      }
    }
  }
  if (act) { ps[r0 * 2 * Cp + i] = a_mu; ps[r0 * 2 * Cp + Cp + i] = a_s; }
  for (int e = tid; e < P * ld; e += blockDim.x) {      // untouched channels
    const bool transformed = fts.strided_hit(fld.mod(e) - t_off, Cp);
    if (!transformed) dx[row0 * ld + e] = g1[e];
  }
  {
    const int pad = ldp - 2 * Cp;
    const FDiv fpad(pad);
    for (int e = tid; e < P * pad; e += blockDim.x) {
      const int p = fpad.div(e), j = 2 * Cp + (e - p * pad);
      dparams[(row0 + p) * ldp + j] = ET<T>::from_f32(0.f);
    }
  }
  __syncthreads();
  if (dbias_part && tid < 2 * Cp) {
    const int used = rows_par < P ? rows_par : P;
    float t = 0.f;
    for (int r = 0; r < used; ++r) t += ps[r * 2 * Cp + tid];
    dbias_part[(long)b * 2 * Cp + tid] = t;
  }
}

// dst[c] = sum_r src[r][c]
__global__ void reduce_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int R, int ncols) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncols; c += gridDim.x * blockDim.x) {
    float t = 0.f;
    for (int r = 0; r < R; ++r) t += src[(long)r * ncols + c];
    dst[c] = t;
  }
}

// ------------------------------------------------------------------ log-det bookkeeping and the loss
// logdet[b] = const_term + sum_l slots[l][b*slot_w .. +slot_w)
// one block per sample; the ~1000 layer slots are summed in a fixed order (thread-strided partials, then a block tree)
__global__ void logdet_finalize_kernel(const float* __restrict__ slots, int nslots, int B, int slot_w, float const_term,
                                       const float* __restrict__ const_dev, float* __restrict__ logdet) {
  __shared__ float red[8];
  const int b = blockIdx.x;
  float t = 0.f;
  for (int i = threadIdx.x; i < nslots * slot_w; i += blockDim.x) {
    const int l = i / slot_w, w = i - l * slot_w;
    t += slots[((long)l * B + b) * slot_w + w];
  }
  const float tot = block_sum(t, red);
  if (threadIdx.x == 0) logdet[b] = tot + const_term + (const_dev ? const_dev[0] : 0.f);
}
// out_scalar[0] = P * sum over `n` ActNorm layers of sum_c log_scale  (batch independent, macow2.py:512)
struct LsRef { long off; int C; };                  // 16 bytes with the tail padding (ipoke_actnorm_logdet_ref_size)
__global__ void actnorm_logdet_kernel(const float* __restrict__ params, const LsRef* __restrict__ refs, int n, int P,
                                      float* __restrict__ out_scalar) {
  __shared__ float red[16];
  float t = 0.f;
  // C <= 64 per layer: blockDim / 64 layers per pass (fixed assignment -> deterministic sum); eight passes' loads in flight at once --
  // with 4 layers per pass and one dependent (descriptor, value) pair per iteration the 515 layers of the shipped flows took 170 us on
  // the chain's queue, once per forward pass
  const int sub = threadIdx.x >> 6, c = threadIdx.x & 63, per = blockDim.x >> 6;
  for (int l0 = sub; l0 < n; l0 += 8 * per) {
    LsRef r[8]; float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int l = l0 + u * per; r[u] = l < n ? refs[l] : LsRef{0, 0}; }
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = c < r[u].C ? params[r[u].off + c] : 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) t += v[u];
  }
  for (int l = 0; l < n; ++l)                       // layers wider than 64 channels (not in the shipped configs)
    for (int cc = 64 + threadIdx.x; cc < refs[l].C; cc += blockDim.x) t += params[refs[l].off + cc];
  const float tot = block_sum(t, red);
  if (threadIdx.x == 0) out_scalar[0] = tot * (float)P;
}
// FlowLoss (loss.py:13-31,75-79): loss = mean_b 0.5*sum z^2 - w * mean_b logdet.
// Writes scalars[0..2] = (loss, nll, nlogdet) and the gradients d_out = z/B (state layout), dld[b] = -w/B.
__global__ void flow_nll_kernel(const float* __restrict__ z, const float* __restrict__ logdet, int B, int P, int C, int ld,
                                float w, float* __restrict__ scalars, float* __restrict__ d_out, float* __restrict__ dld) {
  __shared__ float red[16];
  float t = 0.f;
  const long total = (long)B * P * ld;
  const float invB = 1.f / (float)B;
  if ((ld & 3) == 0 && (((uintptr_t)z | (uintptr_t)d_out) & 15) == 0) {
    // 16-byte groups, four per thread in flight (one workgroup: the value is a fixed-order sum; 72 us -> ~10 us at B = 20)
    const long groups = total >> 2;
    for (long g0 = threadIdx.x; g0 < groups; g0 += 4L * blockDim.x) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long g = g0 + (long)u * blockDim.x;
        v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (g < groups) {
          v[u] = *reinterpret_cast<const f32x4*>(z + 4 * g);
          const int col = (int)((4 * g) % ld);
#pragma unroll
          for (int q = 0; q < 4; ++q) if (col + q >= C) v[u][q] = 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long g = g0 + (long)u * blockDim.x;
        if (g < groups) {
#pragma unroll
          for (int q = 0; q < 4; ++q) t += v[u][q] * v[u][q];
          if (d_out) {
            f32x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = v[u][q] * invB;
            *reinterpret_cast<f32x4*>(d_out + 4 * g) = o;
          }
        }
      }
    }
  } else {
    for (long i = threadIdx.x; i < total; i += blockDim.x) {
      const int col = (int)(i % ld);
      const float v = col < C ? z[i] : 0.f;
      t += v * v;
      if (d_out) d_out[i] = v * invB;
    }
  }
  const float ss = block_sum(t, red);
  float l = 0.f;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    l += logdet[b];
    if (dld) dld[b] = -w * invB;
  }
  const float lsum = block_sum(l, red);
  if (threadIdx.x == 0) {
    const float nll = 0.5f * ss * invB, nld = -lsum * invB;
    scalars[0] = nll + w * nld; scalars[1] = nll; scalars[2] = nld;
  }
}

// ------------------------------------------------------------------ Adam with amsgrad (torch.optim.Adam semantics)
__global__ void adam_amsgrad_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                    float* __restrict__ v, float* __restrict__ vmax, long n, AdamHyper h) {
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      f32x4 pp = *reinterpret_cast<f32x4*>(p + i), gg = *reinterpret_cast<const f32x4*>(g + i);
      f32x4 mm = *reinterpret_cast<f32x4*>(m + i), vv = *reinterpret_cast<f32x4*>(v + i);
      f32x4 vx = *reinterpret_cast<f32x4*>(vmax + i);
      adam_amsgrad_update4(pp, gg, mm, vv, vx, h);
      *reinterpret_cast<f32x4*>(p + i) = pp; *reinterpret_cast<f32x4*>(m + i) = mm;
      *reinterpret_cast<f32x4*>(v + i) = vv; *reinterpret_cast<f32x4*>(vmax + i) = vx;
    } else {
      for (long k = i; k < n; ++k) adam_amsgrad_update(p[k], g[k], m[k], v[k], vmax[k], h);
    }
  }
}

// dst[e.dst + c] = sum_{r < R * e.rmul} src[e.src + r*e.ld + c], c < e.ncols -- one block per entry (multi-tensor reduction)
struct ReduceEntry { long src, dst; int ld, ncols, rmul, pad; };     // rmul rows per sample (>= 1)
__global__ void reduce_rows_multi_kernel(const float* __restrict__ src, float* __restrict__ dst, const ReduceEntry* __restrict__ ent,
                                         int R) {
  const ReduceEntry e = ent[blockIdx.x];
  for (int c = threadIdx.x; c < e.ncols; c += blockDim.x) {
    float t = 0.f;
    const int rows = R * (e.rmul > 0 ? e.rmul : 1);
    const float* col = src + e.src + c;
    // sixteen rows requested at once, added in row order (the same sum as one row at a time -- 20 .. 80 dependent memory round trips,
    // 49 us per launch on the optimizer's queue, which the backward pass is bound by)
    int r = 0;
    for (; r + 16 <= rows; r += 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = col[(long)(r + u) * e.ld];
#pragma unroll
      for (int u = 0; u < 16; ++u) t += v[u];
    }
    for (; r < rows; ++r) t += col[(long)r * e.ld];
    dst[e.dst + c] = t;
  }
}

static inline int grid_for(long n, int block, int cap = 2048) {
  long g = (n + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace ipoke

using namespace ipoke;
#define STREAM(s) reinterpret_cast<hipStream_t>(s)

extern "C" int ipoke_nchw_to_state(const float* x, float* state, int B, int C, int P, int ld, void* stream) {
  IPK_REQUIRE(x && state && C <= ld, "bad arguments");
  hipLaunchKernelGGL(nchw_to_state_kernel, dim3(B), dim3(256), 0, STREAM(stream), x, state, C, P, ld);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_state_to_nchw(const float* state, float* x, int B, int C, int P, int ld, void* stream) {
  IPK_REQUIRE(x && state && C <= ld, "bad arguments");
  hipLaunchKernelGGL(state_to_nchw_kernel, dim3(B), dim3(256), 0, STREAM(stream), state, x, C, P, ld);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_cond_prepare(const float* cond, void* out, int B, int Cc, int P, int act, int dtype, void* stream) {
  IPK_REQUIRE(cond && out, "null tensor");
  if (dtype == IPOKE_BF16)
    hipLaunchKernelGGL(cond_prepare_kernel<bf16_t>, dim3(B), dim3(256), 0, STREAM(stream), cond, (bf16_t*)out, Cc, P, act);
  else
    hipLaunchKernelGGL(cond_prepare_kernel<float>, dim3(B), dim3(256), 0, STREAM(stream), cond, (float*)out, Cc, P, act);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

extern "C" int ipoke_extract_cols(const float* state, int ld, int off, int stride, int C, void* out, int ldo, int64_t M, int dtype,
                                  void* stream) {
  IPK_REQUIRE(state && out && C >= 1 && ldo >= C && off + (C - 1) * stride < ld, "bad arguments");
  if (dtype == IPOKE_BF16)
    hipLaunchKernelGGL(extract_cols_kernel<bf16_t>, dim3(grid_for(M * ldo, 256)), dim3(256), 0, STREAM(stream), state, ld, off, stride,
                       C, (bf16_t*)out, ldo, (long)M);
  else
    hipLaunchKernelGGL(extract_cols_kernel<float>, dim3(grid_for(M * ldo, 256)), dim3(256), 0, STREAM(stream), state, ld, off, stride,
                       C, (float*)out, ldo, (long)M);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_copy_cols(const void* src, int lds, void* dst, int ldd, int C, int64_t M, int dtype, void* stream) {
  const int esz = dtype == IPOKE_BF16 ? 2 : 4, e16 = 16 / esz;
  IPK_REQUIRE(src && dst && C >= 1 && lds >= C && ldd >= C, "bad arguments");
  IPK_REQUIRE(C % e16 == 0 && lds % e16 == 0 && ldd % e16 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
              (reinterpret_cast<uintptr_t>(dst) & 15) == 0, "copy_cols moves 16-byte units: widths, pitches and bases must be multiples of 16 bytes");
  hipLaunchKernelGGL(copy_cols16_kernel, dim3(grid_for(M * (C / e16), 256)), dim3(256), 0, STREAM(stream), (const u32x4*)src,
                     (long)(lds / e16), (u32x4*)dst, (long)(ldd / e16), C / e16, (long)M);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_actnorm_fwd(const float* in, float* out, int M, int ld, int c0, int C, const float* log_scale,
                                 const float* bias, const int32_t* idx, void* stream) {
  IPK_REQUIRE(in && out && c0 >= 0 && c0 + C <= ld, "bad arguments");
  IPK_REQUIRE((log_scale == nullptr) == (bias == nullptr), "log_scale and bias come together");
  hipLaunchKernelGGL(actnorm_fwd_kernel, dim3(grid_for((long)M * ld, 256)), dim3(256), 0, STREAM(stream), in, out, M, ld,
                     c0, C, log_scale, bias, idx);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_actnorm_inv(const float* in, float* out, int M, int ld, int c0, int C, const float* log_scale,
                                 const float* bias, const int32_t* inv_idx, void* stream) {
  IPK_REQUIRE(in && out && c0 >= 0 && c0 + C <= ld, "bad arguments");
  hipLaunchKernelGGL(actnorm_inv_kernel, dim3(grid_for((long)M * ld, 256)), dim3(256), 0, STREAM(stream), in, out, M, ld,
                     c0, C, log_scale, bias, inv_idx);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_actnorm_inv_ext(const float* in, float* out, int M, int ld, int c0, int C, const float* log_scale,
                                     const float* bias, const int32_t* inv_idx, void* ext, int ext_ld, int e_off, int e_stride,
                                     int e_C, int dtype, void* stream) {
  if (!ext) return ipoke_actnorm_inv(in, out, M, ld, c0, C, log_scale, bias, inv_idx, stream);
  IPK_REQUIRE(in && out && c0 >= 0 && c0 + C <= ld, "bad arguments");
  IPK_REQUIRE(e_C >= 1 && e_stride >= 1 && e_off >= 0 && e_off + (long)(e_C - 1) * e_stride < ld, "conditioning columns outside the state");
  IPK_REQUIRE(ext_ld >= e_C && ext_ld - e_C <= ld, "ext_ld: at least e_C, padding no wider than the state");
  IPK_REQUIRE(dtype == IPOKE_F32 || dtype == IPOKE_BF16, "dtype");
  const dim3 grid(grid_for((long)M * ld, 256));
  if (dtype == IPOKE_BF16)
    hipLaunchKernelGGL(actnorm_inv_ext_kernel<bf16_t>, grid, dim3(256), 0, STREAM(stream), in, out, M, ld, c0, C, log_scale, bias, inv_idx,
                       static_cast<bf16_t*>(ext), ext_ld, e_off, e_stride, e_C);
  else
    hipLaunchKernelGGL(actnorm_inv_ext_kernel<float>, grid, dim3(256), 0, STREAM(stream), in, out, M, ld, c0, C, log_scale, bias, inv_idx,
                       static_cast<float*>(ext), ext_ld, e_off, e_stride, e_C);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_actnorm_bwd(const float* dy, const float* x, float* dx, int M, int ld, int c0, int C,
                                 const float* log_scale, const int32_t* idx, const float* dld, int B, int P,
                                 float* part, void* stream) {
  IPK_REQUIRE(dy && dx && C >= 1 && C <= 256 && c0 + C <= ld && M == B * P, "bad arguments");
  IPK_REQUIRE(!log_scale || (x && dld && part), "parameter gradients need x, dld and the partial-sum buffer");
  const int block = 1024;
  const int rows_par = block / C;
  hipLaunchKernelGGL(actnorm_bwd_kernel, dim3(B), dim3(block), 2 * rows_par * C * sizeof(float), STREAM(stream), dy, x, dx,
                     P, ld, c0, C, log_scale, idx, dld, part);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_actnorm_init(const float* x, int M, int ld, int c0, int C, float* log_scale, float* bias, void* stream) {
  IPK_REQUIRE(x && log_scale && bias && M >= 2, "bad arguments");
  hipLaunchKernelGGL(actnorm_init_kernel, dim3(C), dim3(256), 0, STREAM(stream), x, M, ld, c0, log_scale, bias);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}

static int check_affine(const ipoke_affine_desc* d) {
  IPK_REQUIRE(d && d->raw && d->Cp >= 1 && d->nsplit >= 1 && d->t_stride >= 1, "bad affine descriptor");
  IPK_REQUIRE(d->t_off + (d->Cp - 1) * d->t_stride < d->ld, "transformed channels exceed the state width");
  return IPOKE_OK;
}
static AffineArgs to_args(const ipoke_affine_desc* d) {
  AffineArgs a;
  a.raw = d->raw; a.nsplit = d->nsplit; a.split_stride = d->split_stride; a.ldraw = d->ldraw; a.bias = d->bias;
  a.Cp = d->Cp; a.t_off = d->t_off; a.t_stride = d->t_stride; a.P = d->P; a.ld = d->ld;
  return a;
}
extern "C" int ipoke_affine_fwd_ext(const ipoke_affine_desc* d, const float* in, float* out, float* scale_out,
                                    float* logdet_slot, int slot_stride, int B, void* ext, int ext_ld, int dtype, void* stream) {
  int rc = check_affine(d); if (rc) return rc;
  IPK_REQUIRE(in && out, "null state");
  IPK_REQUIRE(!ext || (ext_ld >= d->Cp && (dtype == IPOKE_BF16 || dtype == IPOKE_F32)), "bad extra operand output");
  const int Q = (slot_stride >= 4 || !logdet_slot) && d->P % 4 == 0 ? 4 : 1;
  hipLaunchKernelGGL(affine_fwd_kernel, dim3(B * Q), dim3(256), (size_t)(d->P / Q) * 2 * d->Cp * sizeof(float), STREAM(stream), to_args(d),
                     in, out, scale_out, logdet_slot, slot_stride < 1 ? 1 : slot_stride, Q, ext, ext_ld, dtype == IPOKE_BF16 ? 1 : 0);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_affine_fwd(const ipoke_affine_desc* d, const float* in, float* out, float* scale_out,
                                float* logdet_slot, int slot_stride, int B, void* stream) {
  return ipoke_affine_fwd_ext(d, in, out, scale_out, logdet_slot, slot_stride, B, nullptr, 0, IPOKE_F32, stream);
}
extern "C" int ipoke_affine_inv_ext(const ipoke_affine_desc* d, const float* in, float* out, int B, void* ext, int ext_ld, int dtype,
                                    void* stream) {
  int rc = check_affine(d); if (rc) return rc;
  IPK_REQUIRE(in && out, "null state");
  IPK_REQUIRE(!ext || (ext_ld >= d->Cp && (dtype == IPOKE_BF16 || dtype == IPOKE_F32)), "bad extra operand output");
  const int Q = d->P % 4 == 0 ? 4 : 1;
  hipLaunchKernelGGL(affine_inv_kernel, dim3(B * Q), dim3(256), (size_t)(d->P / Q) * 2 * d->Cp * sizeof(float), STREAM(stream), to_args(d), in, out, Q,
                     ext, ext_ld, dtype == IPOKE_BF16 ? 1 : 0);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_affine_inv(const ipoke_affine_desc* d, const float* in, float* out, int B, void* stream) {
  return ipoke_affine_inv_ext(d, in, out, B, nullptr, 0, IPOKE_F32, stream);
}
extern "C" int ipoke_affine_bwd(int Cp, int t_off, int t_stride, int P, int ld, const float* dy, const float* x,
                                const float* scale, const float* dld, float* dx, void* dparams, int ldp,
                                float* dbias_part, int B, int dtype, void* stream) {
  IPK_REQUIRE(dy && x && scale && dld && dx && dparams && ldp >= 2 * Cp && Cp >= 1 && 2 * Cp <= 1024, "bad arguments");
  const size_t sm = (size_t)(1024 / Cp) * 2 * Cp * sizeof(float);
  if (dtype == IPOKE_BF16)
    hipLaunchKernelGGL(affine_bwd_kernel<bf16_t>, dim3(B), dim3(1024), sm, STREAM(stream), Cp, t_off, t_stride, P, ld, dy, x,
                       scale, dld, dx, (bf16_t*)dparams, ldp, dbias_part);
  else
    hipLaunchKernelGGL(affine_bwd_kernel<float>, dim3(B), dim3(1024), sm, STREAM(stream), Cp, t_off, t_stride, P, ld, dy, x,
                       scale, dld, dx, (float*)dparams, ldp, dbias_part);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_affine_actnorm_fwd(const ipoke_affine_desc* d, const float* in, float* out, float* out2, float* scale_out,
                                        float* logdet_slot, int slot_stride, int B, int c0, int C, const float* log_scale, const float* bias,
                                        const int32_t* idx, void* stream) {
  int rc = check_affine(d); if (rc) return rc;
  IPK_REQUIRE(in && out2 && in != out2 && C >= 1 && c0 >= 0 && c0 + C <= d->ld, "bad arguments");
  IPK_REQUIRE((log_scale == nullptr) == (bias == nullptr), "log_scale and bias come together");
  const int Q = (slot_stride >= 4 || !logdet_slot) && d->P % 4 == 0 ? 4 : 1;
  const ActNormArgs n{c0, C, log_scale, bias, idx};
  const size_t lds = (size_t)(d->P / Q) * (2 * d->Cp + d->ld) * sizeof(float);
  hipLaunchKernelGGL(affine_actnorm_fwd_kernel, dim3(B * Q), dim3(256), lds, STREAM(stream), to_args(d), n, in, out, out2, scale_out,
                     logdet_slot, slot_stride < 1 ? 1 : slot_stride, Q);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_actnorm_affine_bwd(int c0, int C, const float* log_scale, const int32_t* idx, const float* dy2, const float* x1,
                                        float* part, int Cp, int t_off, int t_stride, int P, int ld, const float* x0, const float* scale,
                                        const float* dld, float* dx, void* dparams, int ldp, float* dbias_part, int B, int dtype,
                                        void* stream) {
  IPK_REQUIRE(dy2 && x0 && scale && dld && dx && dparams && ldp >= 2 * Cp && Cp >= 1 && 2 * Cp <= 1024, "bad arguments");
  IPK_REQUIRE(C >= 1 && C <= 256 && c0 >= 0 && c0 + C <= ld && P * ld <= 8192, "bad ActNorm window / state tile");
  IPK_REQUIRE(!log_scale || (x1 && part), "parameter gradients need the saved input and the partial-sum buffer");
  const ActNormArgs n{c0, C, log_scale, nullptr, idx};
  const size_t psn = (size_t)2 * (1024 / C) * C, psa = (size_t)(1024 / Cp) * 2 * Cp;
  const size_t lds = ((size_t)P * ld + (psn > psa ? psn : psa)) * sizeof(float);
  if (dtype == IPOKE_BF16)
    hipLaunchKernelGGL(actnorm_affine_bwd_kernel<bf16_t>, dim3(B), dim3(1024), lds, STREAM(stream), n, Cp, t_off, t_stride, P, ld, dy2, x1,
                       x0, scale, dld, dx, (bf16_t*)dparams, ldp, part, dbias_part);
  else
    hipLaunchKernelGGL(actnorm_affine_bwd_kernel<float>, dim3(B), dim3(1024), lds, STREAM(stream), n, Cp, t_off, t_stride, P, ld, dy2, x1,
                       x0, scale, dld, dx, (float*)dparams, ldp, part, dbias_part);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
__global__ void spin_delay_kernel(long ticks) {
  const long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
/* developer probe: occupy `stream` with one wave for about `us` microseconds (constant 100 MHz counter) */
extern "C" int ipoke_spin_delay(int us, void* stream) {
  IPK_REQUIRE(us >= 0 && us <= 1000, "bad delay");
  hipLaunchKernelGGL(spin_delay_kernel, dim3(1), dim3(64), 0, STREAM(stream), (long)us * 100);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_reduce_rows(const float* src, float* dst, int R, int ncols, void* stream) {
  IPK_REQUIRE(src && dst, "null tensor");
  hipLaunchKernelGGL(reduce_rows_kernel, dim3(grid_for(ncols, 128)), dim3(128), 0, STREAM(stream), src, dst, R, ncols);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_reduce_entry_size(void) { return (int)sizeof(ReduceEntry); }
extern "C" int ipoke_reduce_rows_multi(const float* src, float* dst, const void* entries_dev, int nentries, int R, void* stream) {
  IPK_REQUIRE(src && dst && entries_dev && nentries >= 1 && R >= 1, "bad arguments");
  hipLaunchKernelGGL(reduce_rows_multi_kernel, dim3(nentries), dim3(128), 0, STREAM(stream), src, dst,
                     (const ReduceEntry*)entries_dev, R);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_logdet_finalize(const float* slots, int nslots, int B, int slot_w, float const_term,
                                     const float* const_dev, float* logdet, void* stream) {
  IPK_REQUIRE(logdet && (nslots == 0 || slots), "bad arguments");
  hipLaunchKernelGGL(logdet_finalize_kernel, dim3(B), dim3(256), 0, STREAM(stream), slots, nslots, B, slot_w,
                     const_term, const_dev, logdet);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_actnorm_logdet_ref_size(void) { return (int)sizeof(LsRef); }
extern "C" int ipoke_actnorm_logdet(const float* params, const void* refs_dev, int n, int P, float* out_scalar, void* stream) {
  IPK_REQUIRE(params && refs_dev && out_scalar, "null tensor");
  hipLaunchKernelGGL(actnorm_logdet_kernel, dim3(1), dim3(1024), 0, STREAM(stream), params, (const LsRef*)refs_dev, n, P,
                     out_scalar);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_flow_nll(const float* z_state, const float* logdet, int B, int P, int C, int ld, float logdet_weight,
                              float* scalars3, float* d_out_state, float* dld, void* stream) {
  IPK_REQUIRE(z_state && logdet && scalars3, "null tensor");
  hipLaunchKernelGGL(flow_nll_kernel, dim3(1), dim3(1024), 0, STREAM(stream), z_state, logdet, B, P, C, ld, logdet_weight,
                     scalars3, d_out_state, dld);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
extern "C" int ipoke_adam_amsgrad_step(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, float lr,
                                       float beta1, float beta2, float eps, float weight_decay, int step,
                                       float grad_scale, void* stream) {
  return ipoke_adam_amsgrad_step_grid(p, g, m, v, vmax, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, 0, stream);
}
extern "C" int ipoke_adam_amsgrad_step_grid(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, float lr,
                                            float beta1, float beta2, float eps, float weight_decay, int step,
                                            float grad_scale, int max_blocks, void* stream) {
  IPK_REQUIRE(p && g && m && v && vmax && n > 0 && step >= 1, "bad arguments");
  IPK_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vmax) & 15) == 0, "16-byte alignment");
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  // Persistent grid-stride launch: 4096 workgroups saturate HBM when the update runs alone; an update issued underneath
  // other work (max_blocks, the overlapped data-parallel path) uses one workgroup per CU so that it does not take every
  // wave slot of the chip for its whole duration (85.2 -> 81.3 ms when measured on one GPU).
  const int adam_blocks = max_blocks > 0 ? max_blocks : 4096;
  const AdamHyper h{lr / (float)bc1, beta1, beta2, eps, weight_decay, (float)sqrt(bc2), grad_scale};
  hipLaunchKernelGGL(adam_amsgrad_kernel, dim3(grid_for((n + 3) / 4, 256, adam_blocks)), dim3(256), 0, STREAM(stream), p, g, m, v,
                     vmax, (long)n, h);
  IPK_LAUNCH_CHECK();
  return IPOKE_OK;
}
