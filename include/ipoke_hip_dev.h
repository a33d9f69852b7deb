/*
 * libipoke_hip -- developer / test hooks of the library (NOT part of the drop-in boundary of include/ipoke_hip.h): kernel-dispatch
 * overrides and dispatch introspection for the parity tests, in-situ event timing for bench.py's roofline objects, repeated launches
 * and a spin kernel for the probe scripts.  Same conventions as ipoke_hip.h (status codes, ipoke_last_error, `stream` = hipStream_t).
 */
#ifndef IPOKE_HIP_DEV_H
#define IPOKE_HIP_DEV_H

#include "ipoke_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n back-to-back native launches of the same convolution (kernel timing without host round trips) */
int ipoke_conv_forward_repeat(const ipoke_conv_desc* d, int dtype, int n, void* stream);
/* Test hook: kernel-dispatch switch `name` ("c64": conv3x3_c64, "halo16": conv3x3_halo16) <- value (0 off, 1 the measured default
 * rule, 2 wherever the kernel can run; < 0: back to the default rule 1).  "nn128" (scripts/probe_pair_dgrad.py): 2 = the K-major GEMM
 * (ipoke_conv_desc.w_kmajor) on its 128 x 128 tile whatever M, instead of the 80- / 160-row tiles the cost rule picks.  "nt128"
 * (scripts/probe_pair_coupling.py): the same for the wide N-major GEMMs (Nout > 64): the 128 x 128 tile with one K pass, i.e. the tile
 * and the K order of ipoke_conv_pair_coupling.  "cpl_split" <- 4 / 8 / 16 / 32: ipoke_conv3x3_coupling runs that many K slices where
 * tiles x slices <= 256 and slices <= Kc / 64 (< 0: back to its rule, which picks by M) -- with hidden / 128 the slices of
 * ipoke_conv_pair_coupling, at any M. */
int ipoke_set_dispatch_override(const char* name, int value);
/* Test hook: the kernel family the calling thread's last ipoke_conv_forward was dispatched to (ipoke_conv_pair_dgrad and ipoke_conv_pair_coupling report IPOKE_KERNEL_IGEMM) */
enum { IPOKE_KERNEL_NONE = 0, IPOKE_KERNEL_IGEMM = 1, IPOKE_KERNEL_S8 = 2, IPOKE_KERNEL_HALO = 3, IPOKE_KERNEL_HALO16 = 4, IPOKE_KERNEL_C64 = 5, IPOKE_KERNEL_K8 = 6 };
int ipoke_last_conv_kernel(void);
/* Test hook: the weight-gradient kernel the calling thread's last ipoke_conv_wgrad / ipoke_conv_wgrad_batched was dispatched to
 * (TN: igemm_tn_kernel, the generic form -- f32 and unaligned operands; TN_GLDS / TN_NARROW: the LDS-DMA kernel, 128 x 128 / 64 x 256
 * tiles; LAT8: wgrad3x3_lat8 on the 8x8 latent; HALO: wgrad3x3_halo on large maps) */
enum { IPOKE_WGRAD_KERNEL_NONE = 0, IPOKE_WGRAD_KERNEL_TN = 1, IPOKE_WGRAD_KERNEL_TN_GLDS = 2, IPOKE_WGRAD_KERNEL_TN_NARROW = 3,
       IPOKE_WGRAD_KERNEL_LAT8 = 4, IPOKE_WGRAD_KERNEL_HALO = 5 };
int ipoke_last_wgrad_kernel(void);

/* Test hook: the launch grid of ipoke_posture_nn for (N, K, M): out[0..3] = query blocks, candidate chunks, candidates per chunk (a whole
 * number of tiles; the last chunk may be shorter and end in a ragged tile), candidates per LDS tile. */
int ipoke_posture_nn_grid(int N, int K, int M, int* out);

/* developer probe: one wave spinning for about `us` microseconds on `stream` */
int ipoke_spin_delay(int us, void* stream);

/* In-situ timing for the benchmark's roofline objects: between ipoke_timing_start() and ipoke_timing_stop() every launch of
 * a tagged kernel family is bracketed by HIP events on the stream it is launched on (the rest of the step runs as usual).
 * Tags: 1 = ipoke_conv_forward with a 1x1 kernel and Nout = K >= 1024 (the NICE conv2 GEMM -- where ipoke_conv_pair_coupling takes it, that
 *       launch, i.e. conv2 + conv3 + coupling; its data gradient too unless that is read from the K-major weight: tag 6),
 *       2 = ipoke_conv_wgrad / _batched of the same shape (a batched launch counts once per problem and its time is divided
 *       by the problem count), 3 = ipoke_macow_unit_fwd, 4 = ipoke_macow_unit_bwd. */
#define IPOKE_TAG_NT_SQUARE 1
#define IPOKE_TAG_TN_SQUARE 2
#define IPOKE_TAG_UNIT_FWD 3
#define IPOKE_TAG_UNIT_BWD 4
#define IPOKE_TAG_UNIT_INV 5
#define IPOKE_TAG_NN_SQUARE 6     /* the same square GEMM with the weight read K-major (ipoke_conv_desc.w_kmajor): the conv2 data gradient */
/* every other ipoke_conv_forward launch is tagged by the kernel family the dispatcher chose (IPOKE_TAG_CONV_BASE + IPOKE_KERNEL_*), every
 * other weight gradient IPOKE_TAG_WGRAD; both carry their algorithmic work: FLOPs = 2 * rows * Nout * taps * channels (transposed
 * strided forms: divided by the stride product -- the taps that meet an input pixel), bytes = input + weights + output, each once. */
#define IPOKE_TAG_CONV_BASE 16
#define IPOKE_TAG_WGRAD 32
int ipoke_timing_start(void);
int ipoke_timing_start_all(void);   /* also the IPOKE_TAG_CONV_* / IPOKE_TAG_WGRAD families */
int ipoke_timing_stop(const int* tags, int ntags, int* counts, double* mean_us);
/* Test hook: on != 0 makes every recorded launch count ONCE -- a launch that carries several units of work (ipoke_macow_unit2_*: two
 * MaCowUnits, which the counts above report as two) then shows as the one launch it is; 0: back to counting units. */
int ipoke_timing_raw_launches(int on);
/* per tag: launches, SUM of durations (us), SUM of algorithmic FLOPs and bytes -- the per-configuration rooflines of bench.py */
int ipoke_timing_stop_ex(const int* tags, int ntags, int* counts, double* total_us, double* flops, double* bytes);

/* Test hook: sizeof of the descriptor structs of ipoke_hip.h in the order conv, wgrad, affine, coupling_epi, mcf, unit_pair, flow_config,
 * norm, norm_bwd, rowscale_bwd, sn_job, wgrad_adam (out: at least 12 entries; returns the count) -- the binding's own structs must match. */
int ipoke_desc_sizes(int32_t* out, int n);

/* Test hook: make the flow's next polled pass report a hand-off time-out (which = 0: the row-split unit scratch, 1: the fused
 * conv3 + coupling scratch) -- exercises the engine's IPOKE_ERR_STATE + scratch re-initialisation path (ipoke_flow_handoff_timeouts) */
int ipoke_flow_test_inject_timeout(ipoke_flow* f, int which, void* stream);

/* Test hook: on != 0 makes the flow's backward pass issue the conv2 and conv1 data gradients of every coupling net as two launches
 * even where ipoke_conv_pair_dgrad applies, the second with that kernel's slices (splitk = hidden / 128): every gradient must come out
 * bit-identical (the parity test of the fused launch); 0: back to the default.  Drops the handle's captured graphs. */
int ipoke_flow_test_split_pair_dgrad(ipoke_flow* f, int on);
/* Test hook: on != 0 makes the flow's forward and reverse passes issue conv2 and conv3 + coupling of every coupling net as two launches
 * even where ipoke_conv_pair_coupling applies -- conv2 on the 128 x 128 tile ("nt128"), the second launch at hidden / 128 slices
 * ("cpl_split"; the engine sets and clears both switches around its launches while the hook is on): every state, log-det and
 * gradient must come out bit-identical (the parity test of the fused launch); 0: back to the default.  Drops the handle's captured graphs. */
int ipoke_flow_test_split_pair_coupling(ipoke_flow* f, int on);

/* Test hook: on > 0 makes the flow's forward, backward and reverse passes run every MaCowUnit in a launch of its own even where two
 * adjacent units of equal width would share one (ipoke_macow_unit2_fwd / _bwd / _inv); on < 0 makes them share one wherever
 * ipoke_macow_unit2_applicable says yes, also in a direction whose measured default is a launch per unit (the reverse pass): every
 * state, log-det and gradient must come out bit-identical (the parity test of the two-unit launch); 0: back to the default.  Drops
 * the handle's captured graphs. */
int ipoke_flow_test_split_unit2(ipoke_flow* f, int on);

/* Test hook: forward unroll of the ConvGRU as one launch (1), as launches per phase (0); < 0 goes back to the default (1) */
int ipoke_gru_set_fused(int mode);
/* Test hook: byte offsets into the ConvGRU unroll's workspace and row widths (in elements) of its per-(cell, step) buffers:
 * out[2 k], out[2 k + 1] for k = XH, XHR, UR, U, O, DO, DUR (operands [x | h], [x | h r]; pre-activations ur, the update gate u, the
 * candidate's pre-activation o; the gradients of o and ur); out[14] = ipoke_gru_workspace_bytes; out[15 .. 20] the weight operands:
 * offset of cell 0's slots, bytes per cell, and within a cell the offsets of the ur, ur^T, o and o^T operands.  Buffer k of (cell l,
 * step t) starts (l T + t) B H W rows behind its offset.  Needs n >= 21; returns the number of entries.  No device is touched. */
int ipoke_gru_workspace_layout(const ipoke_gru_desc* d, int dtype, int64_t* out, int n);
/* Test hook: the form ipoke_gru_unroll_forward takes for these arguments where a workgroup may ask for `lds_limit` bytes of LDS: 1 the
 * fused form (bf16, 8 x 8 map, Cx = Ch in {32, 64}, ldx, ldh multiples of 8 and ldo of 4, x0 / h0 16-byte and out 8-byte aligned, and the
 * LDS of BOTH the forward and the backward kernel within the limit), 0 the launch-per-phase form.  The pointers are not dereferenced. */
int ipoke_gru_fused_applicable(const ipoke_gru_desc* d, int dtype, int ldx, int ldh, int ldo, const void* x0, const void* h0, const void* out,
                               int64_t lds_limit);
/* Test hook: the form of the last forward pass on record for `workspace`: 1 fused, 0 launch-per-phase, -1 none on record */
int ipoke_gru_workspace_form(const void* workspace);

#ifdef __cplusplus
}
#endif
#endif
