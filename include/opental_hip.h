/* include/opental_hip.h -- C ABI of libopental_hip.so (MI355X / gfx950, HIP).
 *
 * Drop-in boundary for the OpenTAL/AFSD detection hot path.  Every entry point takes plain
 * device pointers + sizes + a hipStream_t (passed as void*), launches asynchronously on that
 * stream, never synchronises, and returns
 *     0            success
 *    <0            argument error (OTAL_E_*), nothing was launched
 *    >0            a hipError_t from the launch
 * State: a call owns nothing persistent except three process-wide, mutex-guarded registries that exist for launch economy --
 * the named option switches (otal_set_option), the event ring of otal_stream_wait, and the record of DEFERRED split-K
 * reductions (otal_conv_defer_reduces .. otal_conv_flush_reduces).  The first two are safe from any number of host threads.
 * The deferred record is ONE list per process: concurrent calls cannot corrupt it, but "defer, launch weight gradients, flush"
 * is a protocol of one logical issuer at a time (a training step); leave it off (the default) to get launches that touch no
 * shared state at all.  Everything else -- workspaces, prologue regions, sign bits, winner bytes -- is caller-owned memory.
 * No exceptions cross this boundary; no torch types appear in it.  All tensors are contiguous,
 * channel-major, exactly as the reference lays them out: features (B,C,T) / (B,C,T,H,W),
 * proposals (B,N,4).
 *
 * Reference interfaces replaced (Cogito2012/OpenTAL):
 *   otal_bmp_fwd / otal_bmp_bwd    <- pybind module boundary_max_pooling_cuda.forward/backward,
 *                                     AFSD/prop_pooling/boundary_max_pooling_cuda.cpp:21-55,
 *                                     kernels AFSD/prop_pooling/boundary_max_pooling_kernel.cu:17-145
 *   (later sections of this header cite theirs next to each declaration)
 */
#ifndef OPENTAL_HIP_H
#define OPENTAL_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTAL_ABI_VERSION 26

/* argument errors */
#define OTAL_E_NULL      (-1)  /* null pointer */
#define OTAL_E_SHAPE     (-2)  /* non-positive / inconsistent size */
#define OTAL_E_ODD_C     (-3)  /* pooling needs an even channel count (two halves) */
#define OTAL_E_BATCH     (-4)  /* segments batch != feature batch (reference reads out of bounds) */
#define OTAL_E_DTYPE     (-5)  /* unsupported dtype code */
#define OTAL_E_LEVELS    (-6)  /* bad level table */
#define OTAL_E_UNSUPPORTED (-7)

/* dtype codes for feature tensors; proposals/segments are always float32 */
#define OTAL_F32  0
#define OTAL_BF16 1
#define OTAL_F16  2   /* otal_bmp_*: the reference's AT_DISPATCH_FLOATING_TYPES_AND_HALF (boundary_max_pooling_kernel.cu:99,:131) */
#define OTAL_F64  3   /* otal_bmp_* only */

#define OTAL_MAX_LEVELS 8

int otal_abi_version(void);
const char* otal_error_string(int code);
/* Named integer switches that select kernel variants -- the references of the A/B tests:
 *   OTAL_CONV_NO1A OTAL_CONV_NO1AW OTAL_CONV_1A_NOTILE OTAL_CONV_1A_WGS OTAL_W1A_SPLITS  (Conv3d_1a)
 *   OTAL_CONV_NODIRECT OTAL_CONV_DIRECT_MINTILES OTAL_CONV_DIRECT_MINTILES512 OTAL_CONV_DIRECT_XPF2  (direct 3x3x3)
 *   OTAL_CONV_NOWDIRECT OTAL_WDIRECT_BLOCKS  (direct 3x3x3 weight gradient)
 *   OTAL_CONV_NO1X1STREAM OTAL_CONV_NOW1X1 OTAL_CONV_NOPROJ OTAL_CONV_NOPROJW OTAL_CONV_NO1DTILE OTAL_CONV_NOW1D
 *   OTAL_POOL_NO133 OTAL_POOL_NOROWS OTAL_LOSS_NOSTAGE
 * A switch starts from the environment variable of the same name, read once at its first use -- the launch path itself
 * never calls getenv; otal_set_option changes it at run time (OTAL_E_UNSUPPORTED for a name not listed here),
 * otal_get_option reads it (dflt for a name not listed here). */
int otal_set_option(const char* name, int value);
int otal_get_option(const char* name, int dflt);
/* Stream fork / join for callers that spread independent launches of this library over several HIP streams (the host
 * side runs weight gradients beside the data-gradient chain): everything given to `waiter` after the call runs behind
 * what `signaler` has been given so far.  One hipEventRecord + hipStreamWaitEvent on an event of an internal ring
 * (no timing); legal while the streams are being captured into a hipGraph (the waiter joins the capture). */
int otal_stream_wait(void* waiter, void* signaler);

/* ------------------------------------------------------------------ BoundaryMaxPooling ----
 * out[n,c,k] = max_{i in [l,r]} in[n,c,i];  (l,r) = clamp(trunc(seg[n,k,2*(c>=C/2)+{0,1}]), 0, T-1);
 * strict '>' scan from l (ties keep the lowest index, NaN never replaces, l>r gives in[l]).
 * Replaces boundary_max_pooling_cuda.forward (boundary_max_pooling_cuda.cpp:21-34).
 * seg_batch must equal B. */
int otal_bmp_fwd(const void* in, const float* seg, void* out,
                 int B, int C, int T, int N, int seg_batch, int dtype, void* stream);

/* grad_in[n,c,argmax] += grad_out[n,c,k], contributions added in ascending k (deterministic; the
 * reference uses atomicAdd in undefined order).  grad_in is fully written (zeros included).
 * compat_ref_stride != 0 reproduces the reference launcher, which takes tscale from
 * grad_output.size(2) (= N) instead of T (boundary_max_pooling_kernel.cu:121): rows are then
 * addressed and clamped with stride N inside the same (B,C,T) buffers.
 * Replaces boundary_max_pooling_cuda.backward (boundary_max_pooling_cuda.cpp:36-50). */
int otal_bmp_bwd(const void* grad_out, const void* in, const float* seg, void* grad_in,
                 int B, int C, int T, int N, int seg_batch, int compat_ref_stride,
                 int dtype, void* stream);

/* Level-batched form: ONE launch pools every pyramid level.  `in` is (B,C,Ttot) holding the
 * levels side by side along T (level l = columns [t_start[l], t_start[l+1])), `seg` is
 * (B,Ntot,4) with each level's proposals in level-local coordinates (columns
 * [n_start[l], n_start[l+1])), out is (B,C,Ntot).  nlev <= OTAL_MAX_LEVELS; both tables have
 * nlev+1 entries.  With nlev == 1 this is otal_bmp_fwd.  Replaces the 6 per-level calls of
 * ProposalBranch.forward inside the level loop (AFSD/thumos14/BDNet.py:333,:386-389). */
int otal_bmp_fwd_levels(const void* in, const float* seg, void* out,
                        int B, int C, int nlev, const int* t_start, const int* n_start,
                        int dtype, void* stream);
int otal_bmp_bwd_levels(const void* grad_out, const void* in, const float* seg, void* grad_in,
                        int B, int C, int nlev, const int* t_start, const int* n_start,
                        int dtype, void* stream);

/* ------------------------------------------------------- implicit-GEMM convolution (MFMA) ----
 * One kernel family for Conv1d (H=W=1) and Conv3d, fp32 in / fp32 accumulate on
 * v_mfma_f32_32x32x2_f32.  Replaces, on the hot path, torch.nn.Conv1d inside Unit1D
 * (AFSD/common/layers.py:178-214), torch.nn.Conv3d inside Unit3D (AFSD/common/i3d_backbone.py:7-87,
 * AFSD/common/layers.py:106-175) and their autograd backward (cuDNN in the reference).
 *
 * geom   : 28 ints  B,Cin,Cout, Ti,Hi,Wi, To,Ho,Wo, kt,kh,kw, st,sh,sw, pt,ph,pw, nlev, lev[0..8]
 *          (pt/ph/pw = FRONT pad of the reference's SAME rule; out-of-range taps read zero;
 *          nlev > 1: level-packed stride-1 Conv1d, taps do not cross level boundaries)
 * strides: 4 int64  x batch stride, x channel stride, y batch stride, y channel stride (elements);
 *          pointers are pre-offset to the first channel, so channel slices of a concat buffer
 *          are read / written in place.
 * ws     : workspace for a launch's tables, weight packs and split-K slabs.  otal_conv_workspace_bytes(geom, mode) is
 *          the size at which every kernel that may serve the geometry -- fp32 or bf16 operands, fp32- or bf16-stored
 *          contiguous tensors -- takes all the splits it wants: the largest tables-plus-slabs over the steps of its
 *          plans, by the functions the launchers themselves use (conv_select.h: conv_launch_shape).  A smaller one lowers
 *          the split factor (and so changes the fp32 summation order); one too small for a kernel's tables moves the
 *          launch to the next kernel of its plan or is OTAL_E_UNSUPPORTED.  A pair launch of a 1-D layer takes twice
 *          the bytes; a strided or misaligned view whose plan differs from the contiguous one may get fewer splits.  Split-K partials are reduced in a fixed order (deterministic).
 * mode   : 0 forward, 1 data gradient, 2 weight gradient.
 * precision: 0 = fp32 operands on v_mfma_f32_32x32x2_f32 (exact fp32, the parity path);
 *            1 = operands rounded to bf16 when staged into LDS, v_mfma_f32_32x32x16_bf16, fp32
 *                accumulation and fp32 tensors in HBM (the throughput path).
 *            bit 1 (value 2), otal_conv_dgrad only: `wt_packed` points at the FORWARD-layout weight
 *                (Cout, Cin, kvol); the launch re-orders it itself (no otal_conv_pack_wt call needed).
 *            bit 2 (value 4), with bit 0: the LARGE activation operand of the call is STORED as bf16 in HBM
 *                (otal_conv_fwd: y; otal_conv_wgrad / otal_conv_dgrad: dy) -- the pointer is passed through the float*
 *                parameter, strides stay in ELEMENTS.  Only geometries for which otal_conv_half_storage() returns 1
 *                (16-byte aligned pointer, y strides multiples of 8); anything else is OTAL_E_UNSUPPORTED.  The values
 *                are the ones the consumer's bf16 operand rounding produces from the fp32 tensor, so the forward
 *                results do not change; the backbone uses it for Conv3d_1a's output and its gradient (604 MB each).
 *            bit 3 (value 8), with bits 0 and 2 (ABI 23): the tensor on the layer's INPUT side is stored as bf16 as well
 *                (otal_conv_fwd: x; otal_conv_wgrad: x; otal_conv_dgrad: dx) -- every activation and data gradient between two
 *                backbone layers is then a bf16 tensor (half the bytes; operands, accumulators and results are those of the
 *                fp32-tensor kernels fed with the same bf16 values, outputs rounded to nearest even once).  No accumulate.
 *            bit 4 (value 16), otal_conv_dgrad with bit 3: out_mask is a bf16 tensor (the activation itself) -- required
 *                whenever out_mask is given together with bit 3.
 *                otal_conv_half_storage(geom, strides, mode, precision incl. bit 3) says whether a kernel exists
 *                (16-byte aligned pointers; batch / channel strides and positions per sample multiples of 8). */
int otal_conv_half_storage(const int* geom, const int64_t* strides, int mode, int precision);
size_t otal_conv_workspace_bytes(const int* geom, int mode);

/* y = act(scale[co] * conv(x, w) + shift[co]); scale/shift nullable (frozen BN folded, or bias). */
int otal_conv_fwd(const int* geom, const int64_t* strides, const float* x, const float* w,
                  const float* scale, const float* shift, float* y, int relu, int precision,
                  const void* prologue, void* ws, size_t ws_bytes, void* stream);

/* dx (+)= m * conv_transpose(dy, w); when out_mask/out_scale are given,
 * m = (out_mask[dx offset] > 0) * out_scale[ci]: the ReLU + frozen-BN backward of the layer that
 * PRODUCED x, folded into the store (out_mask has dx's layout), so the gradient handed to that layer
 * is already the gradient w.r.t. its convolution output.  wt_packed = otal_conv_pack_wt(w). */
int otal_conv_dgrad(const int* geom, const int64_t* strides, const float* dy, const float* wt_packed,
                    float* dx, int accumulate, const float* out_mask, const float* out_scale,
                    int precision, const void* prologue, void* ws, size_t ws_bytes, void* stream);

/* dw (+)= sum_{b,pos} dy[b,co,pos] * x[b,ci,pos*s + tap - pad] */
int otal_conv_wgrad(const int* geom, const int64_t* strides, const float* x, const float* dy,
                    float* dw, int accumulate, int precision, const void* prologue, void* ws, size_t ws_bytes,
                    void* stream);

/* PAIR launches (ABI 20): TWO problems of the same geometry, strides and options in ONE launch -- arrays of two pointers
 * each, results as of two separate calls (bit-identical: a workgroup never sees the other problem).  For the 1-D
 * temporal layers the model applies as siblings -- the loc / conf towers and the two ProposalBranches
 * (AFSD/thumos14/BDNet.py:64-113,:333-412 run them one after the other) -- whose launches sit at about twice the launch
 * floor: two of them in one grid cost what one does.  Only the geometries of the one-launch 1-D kernels (stride 1,
 * k = 1 / 3, H = W = 1, channels % 128 == 0, precision bit 0 set); anything else returns OTAL_E_UNSUPPORTED and the
 * caller issues the two launches itself.  otal_conv_dgrad_pair takes forward-layout weights (precision bit 1 implied). */
int otal_conv_fwd_pair(const int* geom, const int64_t* strides, const float* const* x, const float* const* w,
                       const float* const* scale, const float* const* shift, float* const* y, int relu, int precision,
                       const void* const* prologue, void* ws, size_t ws_bytes, void* stream);
int otal_conv_dgrad_pair(const int* geom, const int64_t* strides, const float* const* dy, const float* const* w,
                         float* const* dx, int precision, const void* const* prologue, void* ws, size_t ws_bytes, void* stream);
int otal_conv_wgrad_pair(const int* geom, const int64_t* strides, const float* const* x, const float* const* dy,
                         float* const* dw, int precision, void* ws, size_t ws_bytes, void* stream);

/* Persistent prologues.  A bf16 launch first builds its tables and (fwd / dgrad) re-packs the weights to bf16; by default
 * that happens inside every launch, in the workspace.  A caller that runs the same layers repeatedly (a training loop) can
 * own one region per (layer, mode) instead and pass it as `prologue` (NULL = build in the workspace):
 *   otal_conv_prologue_bytes : region size, 0 when this launch has no reusable prologue (generic kernel)
 *   otal_conv_prologue       : fill the region now; for fwd / dgrad also emit the descriptor (host memory,
 *                              otal_conv_prologue_desc_bytes) and return the workgroups it needs; wgrad regions hold a
 *                              geometry-only table and never need refreshing
 *   otal_conv_prologue_batch : after the weights changed, refresh n fwd / dgrad regions in ONE launch from the
 *                              descriptors copied to DEVICE memory; device_starts[n+1] = prefix sums of the workgroup
 *                              counts otal_conv_prologue returned, total_blocks = their sum
 * The regions must be refreshed before the first launch that follows a weight update. */
size_t otal_conv_prologue_bytes(const int* geom, const int64_t* strides, int mode, int precision);
size_t otal_conv_prologue_desc_bytes(void);
int otal_conv_prologue(const int* geom, const int64_t* strides, int mode, const float* w, int precision, void* region,
                       size_t region_bytes, void* host_desc, void* stream);
int otal_conv_prologue_batch(int n, const void* device_descs, const int* device_starts, int total_blocks, void* stream);

/* Deferred weight-gradient reductions.  Nobody reads a weight gradient before the optimizer / the gradient all-reduce, so
 * its split-K reduce need not follow its GEMM: after otal_conv_defer_reduces(1), otal_conv_wgrad launches whose reduction is
 * the plain fixed-order slab sum leave their slabs in the workspace and record the reduction instead of launching it;
 * otal_conv_deferred_end() != 0 then is the address one past those slabs -- the caller must hand every later launch workspace
 * BEHIND it until otal_conv_flush_reduces(stream) has run all recorded reductions (up to 24; more flush by themselves) as
 * ONE launch.  Launches with unaligned slabs reduce at once as before (deferred_end() == 0); the direct 3x3x3 kernels, whose
 * slabs needed a transposing reduce until round 6, now write slabs in dW's own layout and are recorded like the others.  otal_conv_defer_reduces(0) needs an empty record.  The summation order is the one of the
 * immediate reduce for >= 16 slabs (quarter sums in slab order, (q0+q1)+(q2+q3)); deterministic.  Process-wide record behind a
 * mutex: one logical issuer at a time (see the preamble).  Replaces nothing in the reference (autograd of nn.Conv1d / nn.Conv3d, i3d_backbone.py:33-43,
 * layers.py:187-192, has no split-K); it removes ~40 of this library's own launches per training step. */
int otal_conv_defer_reduces(int on);
size_t otal_conv_deferred_end(void);
int otal_conv_deferred_count(void);
int otal_conv_flush_reduces(void* stream);

/* Which kernel served the calling thread's most recent otal_conv_fwd / _dgrad / _wgrad (ABI 25): "generic", "proj", "conv1a",
 * "conv1d_tile", "direct", "chunked", "conv1a_wgrad", "proj_wgrad", "wgrad_direct", "wgrad1x1_wide", "vector" or "wgrad1d";
 * "" after a call that failed.  A static string, valid for the life of the process; for tests that must know whether a
 * kernel ran or refused and passed the launch on. */
const char* otal_conv_last_kernel(void);

/* (Cout,Cin,kvol) -> (Cin,Cout,kvol): the A operand of the data-gradient GEMM. */
int otal_conv_pack_wt(const float* w, float* wt, int Cout, int Cin, int kvol, void* stream);

/* ------------------------------------------------------------------ GroupNorm + ReLU ----
 * y = relu(GroupNorm_G(x) * gamma + beta) on (B,C,T); statistics per (sample, group, level)
 * (nlev <= 1 or lev == NULL: one level).  stats: (B,G,nlev,2) {mean, rstd}, kept for backward.
 * Replaces nn.GroupNorm(32, C) + nn.ReLU after each Unit1D / Unit3D of the pyramid
 * (AFSD/thumos14/BDNet.py:67-103,:129-203,:274-284). */
int otal_gn_relu_fwd(const float* x, const float* gamma, const float* beta, float* y, float* stats,
                     int B, int C, int T, int G, float eps, int relu, int nlev, const int* lev, void* stream);
/* dx and per-(sample,channel) partial sums partial[(b*3 + {0,1,2})*C + c] = {d_gamma, d_beta, sum_t dx}
 * (sum over b by the caller, e.g. otal_sum_partials; sum_t dx is the gradient of the preceding convolution's bias).
 * dy_batch_stride (elements; 0 = C*T): dy may be a channel slice of a wider (B, Ctot, T) map -- the gradient of a
 * torch.cat along the channels (BDNet.py:111) is read in place instead of through a contiguous copy. */
int otal_gn_relu_bwd(const float* dy, int64_t dy_batch_stride, const float* x, const float* gamma, const float* beta,
                     const float* stats, float* dx, float* partial, int B, int C, int T, int G,
                     int relu, int nlev, const int* lev, void* stream);
/* The same for TWO maps of one shape in one launch (ABI 20; see the convolution pair launches). */
int otal_gn_relu_fwd_pair(const float* const* x, const float* const* gamma, const float* const* beta, float* const* y,
                          float* const* stats, int B, int C, int T, int G, float eps, int relu, int nlev, const int* lev,
                          void* stream);
int otal_gn_relu_bwd_pair(const float* const* dy, const int64_t* dy_batch_stride, const float* const* x,
                          const float* const* gamma, const float* const* beta, const float* const* stats, float* const* dx,
                          float* const* partial, int B, int C, int T, int G, int relu, int nlev, const int* lev, void* stream);
/* Batch sums of MANY layers' partials in one launch: for item i, dst{0,1,2}[i][c] = sum_b partial[i][(b*3 + r)*C + c]
 * (r = 0,1,2; ascending b; a NULL dst row is skipped).  Replaces the per-layer torch sum over the batch that follows
 * every GroupNorm backward (21 per step); the destinations may be slices of a flat gradient arena. */
int otal_sum_partials(int n_items, const float* const* partial, float* const* dst0, float* const* dst1,
                      float* const* dst2, const int* channels, const int* batches, void* stream);

/* Which kernel served the calling thread's most recent max-pool, GroupNorm or glue call (ABI 26): otal_maxpool3d_* -> the
 * instantiation ("maxpool133_s2_w8_nn_fwd", "maxpoolk33_s2_bwd<3,bf16,bf16>" = <kt, x or dx storage, y or dy storage>,
 * "maxpool333_rows_fwd<12,f32>", "maxpool333_sep_bwd<6,v4>", "maxpool3d_fwd_lds<333/111>", "maxpool3d_bwd<generic>", ...);
 * otal_gn_relu_* -> the host-side path ("gn_relu_fwd<single>" / "<pair>", "gn_relu_bwd<pair,keep_dx,terms=0>",
 * "gn_relu_bwd<single,no_keep_dx,terms=3>"); otal_sum_partials -> "sum_partials"; otal_convert_storage ->
 * "convert_storage<to_bf16>" / "<to_f32>"; otal_masked_scale_copy -> "masked_scale_copy<4>" / "<1>" (vector width);
 * otal_pyramid_merge_fwd / _bwd -> "pyramid_merge_fwd" / "_bwd".  "" after a call that launched nothing.  A static string,
 * valid for the life of the process; for tests that must know which of a call's kernels ran. */
const char* otal_layer_last_kernel(void);

/* ------------------------------------------------------------------ MaxPool3dSamePadding ----
 * geom: 17 ints B,C, Ti,Hi,Wi, To,Ho,Wo, kt,kh,kw, st,sh,sw, pt,ph,pw (front pads; ZERO padding);
 * strides as for the convolution.  argtap: (B,C,To,Ho,Wo) uint8, OPAQUE to the caller: written by _fwd, consumed by
 * _bwd with the same geometry.  (Content: the winner's tap index (dt*kh+dh)*kw+dw, 255 = a padded zero won; for the
 * 3x3x3 / stride 1 / pad 1 pools on 12x12, 6x6 and 3x3 planes the maximum is taken separably and the byte of position p
 * holds three 2-bit axis taps: w stage bits 1:0, h stage 3:2, t stage 5:4 -- see csrc/pool3d.hip.)  In every case the
 * winner is the FIRST maximum in (dt,dh,dw) scan order with the zero padding taking part.
 * Replaces MaxPool3dSamePadding.forward (AFSD/common/layers.py:9-35) and its autograd backward. */
int otal_maxpool3d_fwd(const int* geom, const int64_t* strides, const float* x, float* y,
                       unsigned char* argtap, void* stream);
/* out_mask/out_scale (nullable pair): dx contribution *= (out_mask[dx offset] > 0) * out_scale[c]. */
int otal_maxpool3d_bwd(const int* geom, const int64_t* strides, const float* dy,
                       const unsigned char* argtap, float* dx, int accumulate,
                       const float* out_mask, const float* out_scale, void* stream);
/* The same pair with the producer's ReLU mask carried as SIGN BITS of the pool input instead of re-reading the fp32
 * activations in the backward pass (604 MB -> 19 MB for MaxPool3d_2a): _fwd_signbits also writes signbits
 * (otal_maxpool3d_signbits_bytes(), opaque), _bwd_signbits applies (bit set) * out_scale[c].  Strided 3x3 pools
 * ((1,3,3)/(1,2,2), (3,3,3)/(2,2,2)) only: _signbits_bytes returns 0 elsewhere and the calls OTAL_E_UNSUPPORTED. */
size_t otal_maxpool3d_signbits_bytes(const int* geom, const int64_t* strides);
int otal_maxpool3d_fwd_signbits(const int* geom, const int64_t* strides, const float* x, float* y,
                                unsigned char* argtap, unsigned char* signbits, void* stream);
int otal_maxpool3d_bwd_signbits(const int* geom, const int64_t* strides, const float* dy, const unsigned char* argtap,
                                float* dx, int accumulate, const unsigned char* signbits, const float* out_scale,
                                void* stream);
/* The same pair with the LARGE tensor stored as bf16: _fwd_signbits_h reads a bf16 pool input (written by otal_conv_fwd
 * with precision bit 2), _bwd_signbits_h writes dx as bf16 (round to nearest even; no accumulate) for otal_conv_wgrad
 * with precision bit 2.  (1,3,3)/(1,2,2) pools only. */
int otal_maxpool3d_fwd_signbits_h(const int* geom, const int64_t* strides, const void* x_bf16, float* y,
                                  unsigned char* argtap, unsigned char* signbits, void* stream);
int otal_maxpool3d_bwd_signbits_h(const int* geom, const int64_t* strides, const float* dy, const unsigned char* argtap,
                                  void* dx_bf16, const unsigned char* signbits, const float* out_scale, void* stream);
/* The general bf16-storage forms (ABI 23).  `io` says which tensors are STORED as bf16 (strides stay in elements).
 *   _fwd_io  io: bit 0 x, bit 1 y.  1 = _fwd_signbits_h; 3 = both: the strided 3x3 pools ((1,3,3)/(1,2,2), (3,3,3)/(2,2,2)) and
 *            the 3x3x3 / stride-1 branch pools on 12 x 12 and 6 x 6 planes.  A max-pool commutes with the monotonic bf16
 *            rounding and its winners are copied, not rounded: the output equals the fp32 pool's output rounded once.
 *            bit 2 (value 4, with 3; round 5): the caller guarantees x >= +0 everywhere -- the output of a conv + ReLU, which
 *            is what MaxPool3d_2a / 3a / 4a read (AFSD/common/i3d_backbone.py:194-244) -- and the (1,3,3)/(1,2,2) pools then
 *            run on ordered integer keys (the bf16 bit patterns themselves; v_max3_u32 over bits << 16 | tap priority):
 *            same winners, values and sign bits on such inputs; a -0.0 is read as +0.0, a NaN is not ordered.
 *   _bwd_io  io: bit 0 dx, bit 1 dy, bit 2 out_mask.  1 = _bwd_signbits_h; 3 / 7 = all of them: strided pools with the sign-bit
 *            mask and a plain store; branch pools with a bf16 out_mask tensor, `accumulate` = read the bf16 dx, add this
 *            pool's contribution in fp32, round to nearest even once (the second producer of an Inception module's input
 *            gradient, AFSD/common/i3d_backbone.py:116-121 under autograd).
 * signbits / out_mask / out_scale nullable as in the fp32 entry points; anything else is OTAL_E_UNSUPPORTED. */
int otal_maxpool3d_fwd_io(const int* geom, const int64_t* strides, const void* x, void* y, unsigned char* argtap,
                          unsigned char* signbits, int io, void* stream);
int otal_maxpool3d_bwd_io(const int* geom, const int64_t* strides, const void* dy, const unsigned char* argtap, void* dx,
                          int accumulate, const void* out_mask, const float* out_scale, const unsigned char* signbits, int io,
                          void* stream);
/* fp32 <-> bf16 storage conversion of a (B, C, P) map (dense positions, batch / channel strides in elements: channel slices of
 * a concat buffer): the boundary between the backbone's bf16-stored tensors and the fp32 tensors around them (the endpoints
 * handed to the pyramid, AFSD/thumos14/BDNet.py:307-308, and their gradients).  to_bf16 != 0: fp32 -> bf16, round to nearest
 * even; 0: bf16 -> fp32, exact.  P, the strides: multiples of 8; pointers 16-byte aligned. */
int otal_convert_storage(const void* src, int64_t src_bs, int64_t src_cs, void* dst, int64_t dst_bs, int64_t dst_cs,
                         int to_bf16, int B, int C, int P, void* stream);

/* ------------------------------------------------------------------ head output tails ----
 * Everything between the head convolutions and CoarsePyramid's outputs (AFSD/thumos14/BDNet.py:337-353,:399-412,:538-556;
 * AFSD/anet/BDNet.py:307-320,:366-376) for n_items <= 8 maps at once: raw[i] (B, channels[i], N) -> out[i] (B, N, channels[i]),
 *   modes[i] 0: the permute(0,2,1).contiguous() only;
 *            1: ScaleExp per pyramid level, exp(scales[l] * x) * level_strides[l] (level_strides null = 1: THUMOS14);
 *            2: permute + DirichletLayer.compute_uncertainty with evidence 'exp' into unct[i] (B, N).
 *            3, 4: mode 2 with evidence 'relu' / 'softplus' (BDNet.py:541-549; backward: 0 at z <= 0 / sigmoid(z), 1 above 20).
 * lev[0..nlev]: anchor ranges of the levels along N.  _bwd: draw[i] (B, C, N) from dout[i] (B, N, C) and dunct[i] (B, N)
 * (either may be null = zero) and dscales[nlev] (deterministic single-workgroup reduction). */
int otal_head_outputs_fwd(int n_items, const int* channels, const int* modes, const float* const* raw, float* const* out,
                          float* const* unct, const float* scales, int B, int N, int nlev, const int* lev,
                          const float* level_strides, void* stream);
int otal_head_outputs_bwd(int n_items, const int* channels, const int* modes, const float* const* raw,
                          const float* const* out, const float* const* unct, const float* const* dout,
                          const float* const* dunct, float* const* draw, const float* scales, float* dscales, int B,
                          int N, int nlev, const int* lev, const float* level_strides, void* stream);

/* ------------------------------------------------------------------ boundary (start / end) losses ----
 * calc_bce_loss (AFSD/thumos14/train.py:152-161; anet/train.py:136-144) on both channel halves of a boundary feature
 * map x (B, C, T) read in place through its batch / channel strides (time stride 1): half h in {0, 1},
 * m = mean over the half's channels of tanh(x), loss_h = mean over (b, t) of BCE(m, mask[b, mask_row0 + h, t * mask_step]).
 * terms (B, 2, T): the per-(b, t) BCE values (loss_h = sum / (B T)); dx (B, C, T) contiguous: d loss_h / d x for the
 * channels of half h (scale each half by the incoming gradient of its loss). */
int otal_boundary_bce(const float* x, int64_t x_batch_stride, int64_t x_channel_stride, const float* mask,
                      int64_t mask_batch_stride, int64_t mask_row_stride, int mask_row0, int mask_step, float* terms,
                      float* dx, int B, int C, int T, void* stream);

/* The tails of the n (<= 4) boundary losses of a step (train.py:193-201: the frame-level map with weight 1 and the two
 * level-0 proposal maps with weight 0.1): out2[h] = sum_i weights[i] * mean_{b,t} terms_i[b][h][t] in one launch, and
 * the matching backward out_i[b][c][t] = dx_i[b][c][t] * weights[i] * (c < C_i / 2 ? *g_start : *g_end) for all maps in
 * one launch (dx_i: as written by otal_boundary_bce; g_start / g_end: device scalars, NULL = 0). */
int otal_boundary_finish(int n, const float* const* terms, const float* weights, const int* T, int B, float* out2, void* stream);
int otal_boundary_scale(int n, const float* const* dx, float* const* out, const float* weights, const int* C, const int* T,
                        int B, const float* g_start, const float* g_end, void* stream);

/* ------------------------------------------------------------------ proposal window indices ----
 * loc (B,Ntot,2) -> level-space windows seg (B,Ntot,4) and frame-space windows frame_seg (B,Ntot,4)
 * for all levels at once; bit-exact restatement of the no_grad block of CoarsePyramid.forward
 * (AFSD/thumos14/BDNet.py:355-384).  lev: nlev+1 column starts of the levels inside Ntot. */
int otal_proposal_windows(const float* loc, float* seg, float* frame_seg, int B, int nlev,
                          const int* lev, float frame_num, void* stream);

/* ------------------------------------------------------------------ inference post-processing ----
 * otal_decode_clips: parse_output + decode_predictions + the threshold test of filtering
 * (AFSD/thumos14/test.py:79-162) for `nclips` clips in one launch.  Inputs are the model outputs
 * (nclips,A,.) as the reference lays them out; offsets/fps: per-clip frame offset and sampling rate.
 * Outputs: seg (nclips,A,2) seconds, score (nclips,K,A), unct/actn (nclips,A), flag (nclips,K,A) uint8
 * = score > conf_thresh && actionness > 0.5.  Both comparisons are strict on the fp32 values: an anchor with act == prop_act == 0
 * has actionness exactly 0.5 and is never flagged.  The two ends of a segment are clamped to [0, clip_length] independently, so
 * end < start and zero-width segments can come out; every element of every output is written for any A and K >= 1.  A refused
 * call (this entry, _ex and _ev) returns its code before any launch and writes nothing. */
int otal_decode_clips(const float* loc, const float* prop_loc, const float* priors, const float* conf,
                      const float* prop_conf, const float* center, const float* act, const float* prop_act,
                      const float* offsets, const float* fps, float* seg, float* score, float* unct,
                      float* actn, unsigned char* flag, int nclips, int A, int K, float clip_length,
                      float conf_thresh, void* stream);
/* otal_decode_clips_ex: otal_decode_clips for every THUMOS14 head, including the closed-set Softmax and EDL baselines
 * (os_head false; test.py:79-162 with use_edl F / T).  Arguments as otal_decode_clips, plus:
 *   score_fn    0 = Dirichlet mean with exp evidence (logits clamped to +-10), 1 = softmax exp(z - max) / sum (fp32);
 *               other values: OTAL_E_UNSUPPORTED;
 *   first_class 0 or 1; 1 drops class 0 (the background logit): score / flag are (nclips, K-1, A), while the softmax /
 *               Dirichlet normalisation and the uncertainty K / S still run over all K logits.
 * act / prop_act are nullable (together): without them no actionness factor is applied and flag = score > conf_thresh.
 * unct / actn are nullable; when given, unct is 0 with score_fn 1 and actn is 0 without act.
 * otal_decode_clips(...) == otal_decode_clips_ex(..., score_fn 0, first_class 0) bit for bit (it needs all four maps). */
int otal_decode_clips_ex(const float* loc, const float* prop_loc, const float* priors, const float* conf,
                         const float* prop_conf, const float* center, const float* act, const float* prop_act,
                         const float* offsets, const float* fps, float* seg, float* score, float* unct,
                         float* actn, unsigned char* flag, int nclips, int A, int K, float clip_length,
                         float conf_thresh, int score_fn, int first_class, void* stream);
/* otal_decode_clips_ev: otal_decode_clips_ex plus `evidence`, the evidence function of the Dirichlet scores and of the
 * uncertainty when score_fn is 0 (DirichletLayer.evidence_func, AFSD/thumos14/BDNet.py:541-549; model.evidence of the yaml):
 * 0 exp(clamp(z, +-10)), 1 relu, 2 softplus (beta 1, threshold 20); alpha = evidence + 1.  score_fn 1 ignores it.
 * evidence 0 == otal_decode_clips_ex(...) bit for bit; another value: OTAL_E_UNSUPPORTED.  An additive entry:
 * OTAL_ABI_VERSION is unchanged. */
int otal_decode_clips_ev(const float* loc, const float* prop_loc, const float* priors, const float* conf,
                         const float* prop_conf, const float* center, const float* act, const float* prop_act,
                         const float* offsets, const float* fps, float* seg, float* score, float* unct,
                         float* actn, unsigned char* flag, int nclips, int A, int K, float clip_length,
                         float conf_thresh, int score_fn, int first_class, int evidence, void* stream);
/* otal_decode_clips_2s: otal_decode_clips_ev for a two-stream run (rgb + flow networks, parse_output test.py:90-108) in one
 * launch, without the averaged maps ever being written.  loc .. prop_act: the rgb network's raw maps; flow_loc .. flow_prop_act:
 * the flow network's, same layouts; act / prop_act / flow_act / flow_prop_act are nullable, all four together.  One priors,
 * offsets, fps for both.  Every map value the decode reads is (rgb + flow) / 2 in fp32, taken in registers as a finished value
 * (never contracted with the arithmetic that follows), then exactly otal_decode_clips_ev's arithmetic: seg, score, actn and
 * flag are bit for bit what otal_decode_clips_ev writes on the maps (rgb + flow) / 2.
 *   conf_sign   +1, or -1 for the GCPL decode: the averaged conf / prop_conf are negated (softmax(-(rgb + flow) / 2)); another
 *               value: OTAL_E_UNSUPPORTED.
 *   unct_in, prop_unct_in, flow_unct_in, flow_prop_unct_in: the networks' OWN uncertainty maps (nclips, A), nullable, all four
 *               together.  Given (the output unct is then required):
 *               unct = ((unct_in + flow_unct_in) / 2 + (prop_unct_in + flow_prop_unct_in) / 2) / 2, in that association
 *               (parse_output :105-108, decode_predictions :122), whatever score_fn says; the uncertainty of the averaged logits
 *               is not computed.  Not given: unct as otal_decode_clips_ev writes it (0 with score_fn 1).
 * Checks in the order of the neighbouring entries: OTAL_E_NULL (a missing map of either network, a partial set of act or of
 * uncertainty maps), OTAL_E_SHAPE (nclips, A, K < 1), OTAL_E_UNSUPPORTED (score_fn, first_class), OTAL_E_SHAPE (K - first_class
 * < 1), OTAL_E_UNSUPPORTED (evidence, then conf_sign); a refused call returns before any launch and writes nothing.  An additive
 * entry: OTAL_ABI_VERSION is unchanged. */
int otal_decode_clips_2s(const float* loc, const float* prop_loc, const float* conf, const float* prop_conf,
                         const float* center, const float* act, const float* prop_act, const float* flow_loc,
                         const float* flow_prop_loc, const float* flow_conf, const float* flow_prop_conf,
                         const float* flow_center, const float* flow_act, const float* flow_prop_act,
                         const float* unct_in, const float* prop_unct_in, const float* flow_unct_in,
                         const float* flow_prop_unct_in, const float* priors, const float* offsets, const float* fps,
                         float* seg, float* score, float* unct, float* actn, unsigned char* flag, int nclips, int A, int K,
                         float clip_length, float conf_thresh, int score_fn, int first_class, int evidence, int conf_sign,
                         void* stream);
/* otal_softnms_classes: for every (video, class) gather the flagged candidates of the video's clips
 * [clip_start[v], clip_start[v+1]) in clip-major / anchor-minor order and run softnms_v2
 * (AFSD/common/segment_utils.py:128-162; get_video_detections, test.py:165-200).
 * out: (nvideos*K, top_k, out_cols) rows [start,end,decayed score,unct,actionness] in original index
 * order; counts: (nvideos*K); out_index (nullable): (nvideos*K, top_k) source row = clip*A + anchor,
 * relative to the video's first clip.  max_clips bounds the clips of one video.  out_cols 3..5: unct may be NULL when
 * out_cols == 3 and actn when out_cols <= 4 (the closed-set rows [start,end,score(,unct)]); the narrower rows are the leading
 * columns of the 5-column rows bit for bit.  A candidate with score == score_threshold takes part, and one whose decayed score
 * equals it stays; among equal scores the lowest index is taken first; start, end, unct and actn are copied unchanged, and so is
 * the score of a row that met no overlapping segment.  counts[v][k] <= min(top_k, candidates - 1), 0 for a video without clips;
 * rows and index entries at and past counts[v][k] are left untouched, so a problem never writes into its neighbours.  Zero-width
 * and reversed (end < start) candidates take part with the reference's arithmetic (width of the top segment clamped at 1e-5);
 * nothing is promised for NaN or Inf inputs.  top_k <= 0 or out_cols outside 3..5: OTAL_E_SHAPE; a refused call writes nothing. */
int otal_softnms_classes(const float* seg, const float* score, const float* unct, const float* actn,
                         const unsigned char* flag, const int* clip_start, int nvideos, int max_clips,
                         int A, int K, float sigma, int top_k, float score_threshold, float* out,
                         int* counts, int* out_index, int out_cols, void* stream);
/* A (video, class) problem keeps its candidates in LDS (<= ~7600 rows = 60 THUMOS14 windows).  The reference's host
 * loop has no such limit (test.py:165-200 handles a video of any length), so longer videos run from a caller-owned
 * global scratch: otal_softnms_scratch_bytes returns its size for a batch with `total_clips` clips in all and at most
 * `max_clips` per video (0 when every video fits LDS: max_clips * A <= 7680 rows, inclusive); otal_softnms_classes_ws =
 * otal_softnms_classes + that scratch; videos on either side of the limit may share a batch.
 * otal_softnms_classes itself returns OTAL_E_UNSUPPORTED when a scratch would be needed. */
size_t otal_softnms_scratch_bytes(int total_clips, int max_clips, int A, int K);
int otal_softnms_classes_ws(const float* seg, const float* score, const float* unct, const float* actn,
                            const unsigned char* flag, const int* clip_start, int nvideos, int max_clips,
                            int A, int K, float sigma, int top_k, float score_threshold, float* out,
                            int* counts, int* out_index, int out_cols, void* scratch, size_t scratch_bytes,
                            int total_clips, void* stream);
/* otal_detection_table (csrc/dettable.hip): the rows / counts of otal_softnms_classes_ws as one compact table, i.e. the
 * host loops get_video_prediction (AFSD/anet/test.py:159-200) and get_video_detections (AFSD/thumos14/test.py:165-200) plus
 * the known-ness scores of threshold.py:128-147, on the device.  The rule is stated in opental_amd/common/det_table.py
 * (table_reference).  rows (V, K, top_k, cols) fp32, cols 3..5 = [start, end, score(, uncertainty)(, actionness)];
 * counts (V, K) int32; durations (V) fp64 seconds or NULL.  Row (v, c, i) is valid when i < counts[v][c] and score > 0
 * (a NaN score is not); with durations or drop_empty also start = max(0, (double)r0), end = min(durations[v], (double)r1)
 * (without durations end = (double)r1) and the row is dropped when end <= start, compared in fp64.  Rows at and past
 * counts[v][c] are never read.  Outputs, each with room for V * K * top_k rows, filled for the N valid rows in (v, c, i)
 * ascending order and left untouched beyond: video, cls (0-based) int32; seg (., 2) fp64; sup (., 3) fp32 = score,
 * uncertainty, actionness (0.0f for a column the rows do not carry); known fp64 = 1 - ood under `scoring` (0..5 in the
 * order of thumos14/test.py: OOD_SCORES: uncertainty, confidence, uncertainty_actionness, a_by_inv_u, u_by_inv_a, half_au),
 * in fp64 from the widened fp32 columns with the operations and their order of the Python lambdas;
 * list_start (V * K + 1) int32 = exclusive prefix of the valid rows per (v, c), list_start[V * K] = N.
 * Three launches on `stream` (count, prefix, fill), no allocation, no synchronisation, no atomic: the table is the same
 * from run to run.  NULL pointer: OTAL_E_NULL; V, K, top_k < 1 or cols outside 3..5: OTAL_E_SHAPE; scoring outside 0..5 or
 * V * K * top_k >= 2^31: OTAL_E_UNSUPPORTED.  An additive entry: OTAL_ABI_VERSION is unchanged. */
int otal_detection_table(const float* rows, const int* counts, const double* durations, int V, int K, int top_k, int cols,
                         int drop_empty, int scoring, int* video, int* cls, double* seg, float* sup, double* known,
                         int* list_start, void* stream);
/* otal_anchor_stats (csrc/anchorstats.hip): the anchor diagnostics of a THUMOS14 detector before decoding and Soft-NMS -- per
 * anchor and stage (0 coarse, 1 refined) the matched label, one score and the EDL gradient, and their histograms
 * (experiments/analyze_actionness.py:226-339, experiments/analyze_gradnorm.py:173-189,:248-262).  The rule is stated in
 * opental_amd/common/anchor_stats.py (anchor_stats_reference).  Layouts of otal_detection_loss: loc (B,K,2) frames; conf,
 * prop_conf (B,K,C) logits; center (B,K); act, prop_act (B,K) or both NULL; priors (K); gt (B,G,3) = [start, end, label]
 * in units of the clip, padded; gvalid (B,G) uint8.
 *   labels   coarse = the loss's matching (first minimum of left + right over the valid ground truths that contain the
 *            anchor, 0 when none does); refined = coarse, 0 where the IoU of loc with the matched target is < overlap_thresh.
 *            fp32, the operations and order of the loss kernel.
 *   groups   0 known (1 <= label <= n_known), 1 unknown (label > n_known), 2 background (label 0).
 *   score    `target` 0..4 = uncertainty C/S, actionness sigmoid(act), confidence max_k alpha_k/S * sigmoid(center) (times the
 *            actionness with os_head), uncertainty * actionness, 0.5 (actionness + 1) uncertainty; alpha = exp(clamp(z, +-10))
 *            + 1 of the stage's logits, the actionness of the stage's map.
 *   gradient 1/alpha_y - C/S at the label's column: with os_head the anchors labelled 1..C at column label - 1, without it
 *            every anchor at column label (0 = background); a label outside the C columns gives no row; 0 where no row.
 * Outputs: hist_score int64 (2, 3, score_bins), bin min((int)floorf(v * score_bins), score_bins - 1), a NaN score counted
 * nowhere; hist_grad int64 (2, grad_bins) over |gradient| of the rows that count, edges i / grad_bins with 1e-6 added to the
 * last (the bins of reweight 2).  Both are ADDED to: a dataset accumulates over launches.  label int32, value fp32, grad fp32,
 * each (B,K,2) and each nullable (not written).
 * One launch on `stream`, one workgroup per sample, no allocation, no synchronisation; the counts are integers, so the result
 * is identical from run to run.  Checked before any read or launch: a NULL required pointer (everything but act, prop_act,
 * label, value, grad): OTAL_E_NULL; B, K, C, G, score_bins or grad_bins < 1: OTAL_E_SHAPE; target outside 0..4, a target that
 * uses the actionness without both maps (1, 3, 4, and 2 with os_head), one map without the other, n_known < 1, or
 * 6 score_bins + 2 grad_bins > 16384 (the histograms of a workgroup live in LDS): OTAL_E_UNSUPPORTED.
 * An additive entry: OTAL_ABI_VERSION is unchanged. */
int otal_anchor_stats(const float* loc, const float* conf, const float* prop_conf, const float* center, const float* act,
                      const float* prop_act, const float* priors, const float* gt, const unsigned char* gvalid, int B, int K,
                      int C, int G, float clip_length, float overlap_thresh, int os_head, int n_known, int target,
                      int score_bins, int grad_bins, long long* hist_score, long long* hist_grad, int* label, float* value,
                      float* grad, void* stream);
/* otal_anchor_stats_ev: otal_anchor_stats with the network's evidence function (grad_edl reads the model's evidence,
 * experiments/analyze_gradnorm.py:164-184): alpha = evidence(z) + 1 with evidence 0 exp, 1 relu, 2 softplus in S, in the
 * scores and in the gradient.  evidence 0 == otal_anchor_stats(...); another value: OTAL_E_UNSUPPORTED.  An additive entry:
 * OTAL_ABI_VERSION is unchanged. */
int otal_anchor_stats_ev(const float* loc, const float* conf, const float* prop_conf, const float* center, const float* act,
                         const float* prop_act, const float* priors, const float* gt, const unsigned char* gvalid, int B,
                         int K, int C, int G, float clip_length, float overlap_thresh, int os_head, int n_known, int target,
                         int score_bins, int grad_bins, long long* hist_score, long long* hist_grad, int* label,
                         float* value, float* grad, int evidence, void* stream);

/* ------------------------------------------------------------------ OpenMax baseline (csrc/openmax.hip) ----
 * Added under ABI 26 (new symbols only).  Feature rows are addressed by ELEMENT strides: row n (0 <= n < N), channel d at
 *     feat + (n / rows_per_batch) * sb + (n % rows_per_batch) * sr + d * sc,
 * so a contiguous (B, A, D) tensor (rows_per_batch A, sb A*D, sr D, sc 1) and a permuted view of a channel-major (B, D, A)
 * map (sb D*A, sr 1, sc A) are both read in place, each element once; both give the same bits.  MAVs are contiguous
 * (K, D) float, 16-byte aligned.  Limits: K <= 16, D <= 512, D % 16 == 0 (what one workgroup stages in LDS); beyond them
 * OTAL_E_UNSUPPORTED.  All sums over D run in fp32 in one fixed order (16 partial sums, channel d in partial d % 16, then a tree).
 *
 * otal_openmax_dist: compute_eucos_dist (AFSD/thumos14/openmax.py:7-9; the loops of test_openmax.py:319,324 and
 * openmax.py:56-62): dist = ||mav - f||_2 / 200 + (1 - cos(mav, f)).  labels NULL: dist is (N, K), every row against every
 * MAV.  labels (N) int32: dist is (N), row n against MAV labels[n]; a label outside [0, K) gives -1. */
int otal_openmax_dist(const float* feat, int N, int rows_per_batch, int64_t sb, int64_t sr, int64_t sc, const float* mav,
                      int K, int D, const int* labels, float* dist, void* stream);
/* otal_openmax_class_means: the per-class np.mean of test_openmax.py:317-318,322-323.  means (K, D) = mean of the rows with
 * labels[n] == k (0 for a class without rows), counts (K) int32; labels outside [0, K) are ignored.  Fixed summation order,
 * no floating-point atomics: two runs give the same bits.  Any K and D. */
int otal_openmax_class_means(const float* feat, int N, int rows_per_batch, int64_t sb, int64_t sr, int64_t sc,
                             const int* labels, int K, int D, float* means, int* counts, void* stream);
/* otal_openmax_probs: OpenMax.forward (openmax.py:42-86) for N rows in one launch.  logits: row n, class j at
 * logits[n * ldl + j] (ldl >= K; a `conf[:, 1:]` view has ldl = K + 1).  wb (K, 3) float = per class, prepared in float64
 * from the libMR fit (MetaRecognition.cpp:141-152,:211-216): off = small_score + (scale - translate), 1 / scale, shape;
 * w_score(d) = -expm1(-exp(shape * log1p((d - off) / scale))), 0 where the translated argument is <= 0.  R: the alpha rank,
 * 1 <= R <= K (else OTAL_E_UNSUPPORTED); the i-th largest logit gets alpha (R + 1 - i) / R, equal logits rank the higher
 * index first (numpy `argsort()[::-1]`).  probs (N, K + 1): column 0 is P(unknown).  The softmax subtracts the maximum
 * exponent (same value as the reference, no overflow).  Checks run in the order NULL, SHAPE, UNSUPPORTED, as in
 * otal_openmax_probs_wide: ldl < K together with K > 16 is OTAL_E_SHAPE. */
int otal_openmax_probs(const float* logits, int64_t ldl, const float* feat, int N, int rows_per_batch, int64_t sb, int64_t sr,
                       int64_t sc, const float* mav, const float* wb, int K, int D, int R, float* probs, void* stream);
/* otal_decode_clips_openmax: decode_output + the threshold test of `filtering` (test_openmax.py:141-189) for nclips clips in
 * one launch, next to otal_decode_clips_ex and with its output layout: seg (nclips, A, 2) seconds, score (nclips, K, A),
 * flag (nclips, K, A) uint8 = score > conf_thresh, K = C - first_class (conf / prop_conf are (nclips, A, C); the first
 * `first_class` logits -- the background -- are dropped, test_openmax.py:158-159), plus unknown (nclips, A) =
 * (P0 + P0_prop) / 2 * sigmoid(center), the reference's score row 0.  score = (P + P_prop) / 2 * sigmoid(center) with
 * P = OpenMax(mav, wb)(conf[:, first_class:], feat) and P_prop = OpenMax(mav_prop, wb_prop)(prop_conf[:, first_class:], F),
 * F = feat when refined_feature == 0 -- the reference as shipped feeds the COARSE feature to the refined stage
 * (test_openmax.py:159) -- and prop_feat when refined_feature == 1 (prop_feat / prop_feat_strides may be NULL otherwise).
 * feat_strides / prop_feat_strides: HOST arrays {sb, sr, sc} of (nclips, A, D) views.  No (N, K + 1) intermediate is written. */
int otal_decode_clips_openmax(const float* loc, const float* prop_loc, const float* priors, const float* conf,
                              const float* prop_conf, const float* center, const float* offsets, const float* fps,
                              const float* feat, const float* prop_feat, const int64_t* feat_strides,
                              const int64_t* prop_feat_strides, const float* mav, const float* mav_prop, const float* wb,
                              const float* wb_prop, float* seg, float* score, float* unknown, unsigned char* flag,
                              int nclips, int A, int C, int first_class, int D, int R, int refined_feature,
                              float clip_length, float conf_thresh, void* stream);

/* ------------------------------------------------------------------ OpenMax for up to 256 classes (csrc/openmax_wide.hip) ----
 * The ActivityNet1.3 OpenMax baseline has K = 150 classes: no MAV table fits in LDS.  Only the R largest logits of a row get a
 * non-zero alpha (openmax.py:42-73), every other class keeps its logit exactly and adds exactly 0 to the unknown sum, so a
 * row needs R distances: the R MAV rows are gathered from memory, O(R D + K) per row.  Feature view, MAVs, wb, ranking of
 * equal logits, w-score form and softmax as documented above.  Limits: 1 <= K <= 256, 16 <= D <= 512, D % 16 == 0,
 * 1 <= R <= K, MAVs 16-byte aligned; beyond them OTAL_E_UNSUPPORTED before any read or launch.  All sums over D run in fp32
 * in one fixed order (64 partial sums: channel d in partial d % 64; then a tree), independent of the feature's layout; no
 * atomics; every output element is written exactly once.
 *
 * otal_openmax_dist_wide: dist (N), row n against MAV labels[n]; -1 where the label is outside [0, K).  labels is required
 * (the all-pairs form at wide K has no user).  An additive entry: OTAL_ABI_VERSION is unchanged. */
int otal_openmax_dist_wide(const float* feat, int N, int rows_per_batch, int64_t sb, int64_t sr, int64_t sc, const float* mav,
                           int K, int D, const int* labels, float* dist, void* stream);
/* otal_openmax_probs_wide: otal_openmax_probs for K <= 256.  An additive entry: OTAL_ABI_VERSION is unchanged. */
int otal_openmax_probs_wide(const float* logits, int64_t ldl, const float* feat, int N, int rows_per_batch, int64_t sb,
                            int64_t sr, int64_t sc, const float* mav, const float* wb, int K, int D, int R, float* probs,
                            void* stream);
/* otal_decode_clips_openmax_wide: the arguments and outputs of otal_decode_clips_openmax for K = C - first_class <= 256, in one
 * launch; no (N, K + 1) intermediate is written.  The segments are those of ActivityNet inference (AFSD/anet/test.py:110-115):
 * priors[i] * clip_length -/+ the refined offsets, clamped to [0, clip_length], (+ offset) / fps -- the narrow decode's
 * formula; `priors` holds the A centres.  An additive entry: OTAL_ABI_VERSION is unchanged. */
int otal_decode_clips_openmax_wide(const float* loc, const float* prop_loc, const float* priors, const float* conf,
                                   const float* prop_conf, const float* center, const float* offsets, const float* fps,
                                   const float* feat, const float* prop_feat, const int64_t* feat_strides,
                                   const int64_t* prop_feat_strides, const float* mav, const float* mav_prop, const float* wb,
                                   const float* wb_prop, float* seg, float* score, float* unknown, unsigned char* flag,
                                   int nclips, int A, int C, int first_class, int D, int R, int refined_feature,
                                   float clip_length, float conf_thresh, void* stream);

/* ------------------------------------------------------------------ detection-head convolutions ----
 * The skinny Unit1D heads of one CoarsePyramid stage (AFSD/thumos14/BDNet.py:205-272, :337-353, :399-412;
 * AFSD/common/layers.py:178-214: SAME pad + nn.Conv1d(512, cout, k) + bias, cout = 1 / 2 / num_classes, k = 1 / 3) as
 * fp32 FMA kernels over LDS-staged (B, C, N) windows: ONE launch for the forward of all heads of a stage, TWO for their
 * backward (data gradients summed per input map; weight + bias gradients without split-K).
 *   head h reads input map x[in_idx[h]] (B, C, N), has weights w[h] (cout[h], C, ksize[h]) and bias[h] (cout[h]) or NULL,
 *   writes y[h] (B, cout[h], N).  lev (nlev + 1 column starts, or nlev <= 1): taps never cross a level boundary.
 *   backward: dy[h] (B, cout[h], N) or NULL (= zeros); dx[j] (B, C, N) or NULL (not needed) receives the SUM over the
 *   heads on input j; dw[h] like w[h]; db[h] (cout[h]) or NULL.  Plain stores, nothing is accumulated into.
 * Limits: C % 16 == 0, at most 8 heads on 4 inputs, at most 21 output channels per input, ksize 1 or 3;
 * otal_head_convs_supported() != 0 says the launches fit (callers fall back to otal_conv_* otherwise). */
int otal_head_convs_supported(int n_heads, int n_inputs, const int* in_idx, const int* cout, const int* ksize, int B, int C, int N);
int otal_head_convs_fwd(int n_heads, int n_inputs, const int* in_idx, const int* cout, const int* ksize,
                        const float* const* x, const float* const* w, const float* const* bias, float* const* y, int B, int C,
                        int N, int nlev, const int* lev, void* stream);
int otal_head_convs_bwd(int n_heads, int n_inputs, const int* in_idx, const int* cout, const int* ksize,
                        const float* const* x, const float* const* w, const float* const* dy, float* const* dx,
                        float* const* dw, float* const* db, int B, int C, int N, int nlev, const int* lev, void* stream);
/* The same with the two launches selectable: parts bit 0 = data gradients, bit 1 = weight / bias gradients (independent:
 * a caller may put them on different streams). */
int otal_head_convs_bwd_parts(int n_heads, int n_inputs, const int* in_idx, const int* cout, const int* ksize,
                        const float* const* x, const float* const* w, const float* const* dy, float* const* dx,
                        float* const* dw, float* const* db, int B, int C, int N, int nlev, const int* lev, int parts, void* stream);

/* ------------------------------------------------------------------ distance head (RPL / GCPL baselines) ----
 * RPLHead with one centre per class and the 'l2' metric (AFSD/common/layers.py:314-351; the conf_head / prop_conf_head of
 * AFSD/thumos14/BDNet.py:218-219,:248-249 under use_rpl), on the channel-major map where it lies:
 *   x (B, D, N), centers (C, D) -> dist (B, C, N),  dist[b][c][n] = 1/D sum_d (x[b][d][n] - centers[c][d])^2
 * as the direct sum of squared differences in fp32 (the reference expands |f|^2 - 2 f.c + |c|^2 around a matmul, between
 * two permuted copies).  ONE launch.  Backward, g (B, C, N):
 *   dx[b][d][n]    = 2/D sum_c g[b][c][n] (x[b][d][n] - centers[c][d])          parts bit 0 (dx NULL: not needed)
 *   dcenters[c][d] = 2/D sum_{b,n} g[b][c][n] (centers[c][d] - x[b][d][n])      parts bit 1
 * one launch each, independent (a caller may put them on different streams, as with otal_head_convs_bwd_parts).
 * Every sum runs in a fixed order with plain stores: no floating-point atomics, two runs give the same bits.
 * Limits: C <= 21, D <= 512, D % 16 == 0 (OTAL_E_UNSUPPORTED beyond). */
int otal_rpl_head_fwd(const float* x, const float* centers, float* dist, int B, int C, int D, int N, void* stream);
int otal_rpl_head_bwd(const float* x, const float* centers, const float* g, float* dx, float* dcenters, int B, int C, int D,
                      int N, int parts, void* stream);

/* ------------------------------------------------------------------ gradient hand-over to the backbone ----
 * dst[b][c][t][s] (+)= (z[b][c][t][s] > 0 ? scale[c] : 0) * src[b][c][t][s]   (scale NULL: 1; accumulate != 0: +=).
 * Every tensor has its own element strides {batch, channel, frame} and unit stride along s (the H*W plane), so src may be
 * the swapped-role projection gradient laid out [(b, t)][c][s] and dst / z channel slices of larger buffers.
 * Replaces what autograd runs between the pyramid projections (AFSD/thumos14/BDNet.py:129-155, :310-319) and the last
 * Inception modules (AFSD/common/i3d_backbone.py:33-43 F.relu + frozen BatchNorm3d backward): relu backward, the
 * BatchNorm scale and the contiguous copy of the permuted gradient -- three passes over the map in ATen. */
int otal_masked_scale_copy(const float* src, const int64_t* src_strides, const float* z, const int64_t* z_strides,
                           const float* scale, float* dst, const int64_t* dst_strides, int accumulate, int B, int C,
                           int T, int S, void* stream);

/* ------------------------------------------------------------------ optimizer ----
 * torch.optim.Adam with L2 weight decay (AFSD/thumos14/train.py:321-323) over one flat fp32
 * arena; g is multiplied by grad_scale first (1/world_size after a sum all-reduce). */
int otal_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);

/* The same update with the two bias corrections {1 - beta1^t, sqrt(1 - beta2^t)} read from DEVICE memory
 * (written by the host before the launch): no launch argument changes between steps, so a training step can be
 * captured once in a HIP graph and replayed.  Replaces the same reference lines as otal_adam_flat. */
int otal_adam_flat_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                       float beta2, float eps, float weight_decay, const float* bias_corr, float grad_scale,
                       void* stream);

/* Global L2 norm of the flat gradient and the coefficient torch.nn.utils.clip_grad_norm_ would scale it by, on the device
 * (the reference's per-step `stats/grad_norm` scalar and its clip line, AFSD/thumos14/train.py:134-141,:248-250):
 *   out[0] = float( sqrt( sum_i (double)g[i]^2 ) * (double)grad_scale )
 *   out[1] = max_norm <= 0 ? 1.0f : min(c, 1.0f) with c = (1.0f / (out[0] + 1e-6f)) * max_norm in float32 -- torch's
 *            `max_norm / (total_norm + 1e-6)` is reciprocal() * max_norm -- and a NaN c kept (torch's clamp keeps it).
 * fp64 accumulation, a grid and a reduction order that depend on n alone: the same bits on every run and every rank.
 * Two launches (per-block partial sums, then one block that folds them).  `partials` is a caller-owned workspace of
 * OTAL_GRAD_NORM_PARTIALS doubles (16 KB), 8-byte aligned, private to the stream while the call is in flight.
 * Null pointers: OTAL_E_NULL; n <= 0: OTAL_E_SHAPE, both before any launch.  An additive entry: OTAL_ABI_VERSION is unchanged. */
#define OTAL_GRAD_NORM_PARTIALS 2048
int otal_grad_norm(const float* g, int64_t n, float grad_scale, float max_norm, double* partials, float* out, void* stream);

/* otal_adam_flat_dev with the gradient clipped by its global norm: norm_coef points at otal_grad_norm's `out`, and the
 * update uses gi = (g * grad_scale) * norm_coef[1] + weight_decay * p.  With norm_coef[1] == 1.0f the result is
 * bit-identical to otal_adam_flat_dev.  Return codes as otal_adam_flat_dev.  An additive entry: OTAL_ABI_VERSION is unchanged. */
int otal_adam_flat_clip(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                        float eps, float weight_decay, const float* bias_corr, float grad_scale, const float* norm_coef,
                        void* stream);

/* otal_adam_flat_dev / otal_adam_flat_clip with the step's learning-rate multiplier and, optionally, the exponential moving
 * average of the weights in the same sweep (the rule: opental_amd/common/lr_schedule.py).  step_state points at FOUR device
 * floats {1 - beta1^t, sqrt(1 - beta2^t), lr multiplier, ema keep factor} the host writes before the launch (4-byte
 * alignment is enough): a per-step schedule changes no launch argument, so the captured step replays.  The update is the
 * existing one at the float32 rate lr * step_state[2]; with step_state[2] == 1.0f it is bit-identical to otal_adam_flat_dev
 * (norm_coef NULL) or otal_adam_flat_clip (norm_coef given).  ema != NULL: a fifth array of n floats,
 *   ema[i] = fmaf(p'[i] - ema[i], 1.0f - step_state[3], ema[i])   with p' the freshly updated parameter,
 * 9 floats of traffic per parameter where the update alone moves 7; p, m, v do not depend on its presence.  A keep factor of 1
 * leaves ema's bits; one of 0 gives fl(fl(p' - ema) + ema), the bits of p' wherever p' - ema is a float32 value (ema within a
 * factor two of p').  All five arrays 16-byte aligned: 16-byte accesses, else the whole call is element-wise.  ema == NULL:
 * step_state[3] is not used.  Return codes as otal_adam_flat_dev: OTAL_E_NULL for a NULL among p, g, m, v, step_state, the
 * shape error for n <= 0, both before any launch.  An additive entry: OTAL_ABI_VERSION is unchanged. */
int otal_adam_flat_sched(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1,
                         float beta2, float eps, float weight_decay, const float* step_state, float grad_scale,
                         const float* norm_coef, void* stream);

/* The non-finite-gradient guard of the training step (the rule: opental_amd/common/step_guard.py): the step is APPLIED iff
 * norm[0] -- otal_grad_norm's out[0] -- is finite, else SKIPPED, decided on the device so that a replayed step needs no host
 * round trip.  One launch of one workgroup.  `guard` is a caller-owned device record of OTAL_STEP_GUARD_BYTES bytes, 8-byte
 * aligned:
 *   int64 applied; int64 nonfinite; double pow1 (= beta1^applied); double pow2 (= beta2^applied); int32 apply;
 *   28 bytes reserved, zero.                             (a fresh record: zeros with pow1 = pow2 = 1.0)
 * applied:  ++applied, pow1 *= (double)beta1, pow2 *= (double)beta2, apply = 1;   skipped:  ++nonfinite, apply = 0.
 * step_state (4 floats, what otal_adam_flat_guard reads) <- {(float)(1.0 - pow1), (float)sqrt(1.0 - pow2), host_state[2],
 * host_state[3]} -- the bias corrections of the APPLIED count, by IEEE multiply / subtract / sqrt alone; host_state is the
 * record the host writes for otal_adam_flat_sched (only its lr multiplier and EMA keep factor are read), NULL: 1.0f and 0.0f.
 * loss_state != NULL with n_state > 0 (the criterion's cross-step loss state, loss_state_keep then required):
 *   applied: loss_state_keep[i] = loss_state[i];   skipped: loss_state[i] = loss_state_keep[i]   for i < n_state.
 * NULL among norm, guard, step_state, or a loss_state (n_state > 0) without loss_state_keep: OTAL_E_NULL; n_state < 0:
 * OTAL_E_SHAPE; n_state > OTAL_STEP_GATE_MAX_STATE: OTAL_E_UNSUPPORTED (the states in use are 50 and num_bins floats); all
 * before any launch, a refused call writes nothing.  An additive entry: OTAL_ABI_VERSION is unchanged. */
#define OTAL_STEP_GUARD_BYTES 64
#define OTAL_STEP_GATE_MAX_STATE 4096
int otal_step_gate(const float* norm, void* guard, const float* host_state, float* step_state, float beta1, float beta2,
                   float* loss_state, float* loss_state_keep, int n_state, void* stream);

/* otal_adam_flat_sched behind the guard: `guard` is the record otal_step_gate left.  guard->apply != 0: every array ends with
 * the bits otal_adam_flat_sched gives for the same arguments (one body, the same 16-byte and element-wise routes, norm_coef
 * and ema as there).  guard->apply == 0: every workgroup returns on a branch that is uniform across the grid, having read
 * that one word: no byte of p, m, v, ema moves.  Return codes as otal_adam_flat_sched, plus OTAL_E_NULL for guard.  An
 * additive entry: OTAL_ABI_VERSION is unchanged. */
int otal_adam_flat_guard(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1,
                         float beta2, float eps, float weight_decay, const float* step_state, float grad_scale,
                         const float* norm_coef, const void* guard, void* stream);

/* MultiSegmentLoss + EvidenceLoss ('log', exp evidence, IBM re-weighting, IoU calibration) + ActionnessLoss (PU BCE,
 * rank weight 0) of the OpenTAL final recipe, forward AND backward in one single-workgroup launch.
 * Replaces AFSD/thumos14/multisegment_loss.py:92-259, cls_loss.py:120-129,:132-168,:212-278,:288-339 and their autograd
 * graph.  All tensors fp32 contiguous: loc/prop_loc (B,K,2), conf/prop_conf (B,K,C), center/act/prop_act (B,K),
 * priors (K), gt (B,G,3) = padded [start,end,label] with gvalid (B,G) bytes; weight_accum (num_bins) is the IBM EMA
 * state, updated in place (conf first, then prop_conf, as the reference does).
 * losses: 7 floats {loc, conf, prop_loc, prop_conf (+IoU calibration), center, act, prop_act}, normalised as the
 * reference's forward.  grads (otal_detection_loss_grad_floats): d loss_i / d input of the term that owns it, in the
 * order dloc[loc term], dloc[center term], dprop_loc[prop_loc term], dprop_loc[center term] (each (B,K,2)),
 * dconf, dprop_conf ((B,K,C)), dcenter, dact, dprop_act ((B,K)).  scratch: otal_detection_loss_scratch_floats.
 * cls_mode 1 = the as-shipped THUMOS14 dispatch (AFSD/thumos14/train.py:27-31 overwrites cls_loss_type 'edl' with
 * 'focal'): the two classification terms are FocalLoss_Ori(balance_index 0, alpha = focal_alpha, gamma 2,
 * size_average False) on the softmax scores of the positive rows (cls_loss.py:6-78); no IBM, no IoU calibration.
 * Closed-set baselines (os_head false, C = classes + 1 with class 0 = background; multisegment_loss.py:196-231 without
 * os_head): EVERY anchor is classified against its matched label (0 where unmatched), normalised by N / PN as above.
 *   cls_mode 2 = EvidenceLoss 'log' with exp evidence (thumos14_open_edl.yaml); ibm_active must be 0
 *                (OTAL_E_UNSUPPORTED otherwise); iou_aware applies as in mode 0;
 *   cls_mode 3 = FocalLoss_Ori(balance_index 0, alpha = focal_alpha, gamma 2) on the softmax scores (thumos14_softmax.yaml);
 *                alpha[0] = focal_alpha belongs to the background.
 * In modes 2 and 3 act / prop_act may be NULL: losses 5 and 6 and the dact / dprop_act gradient slots are written as 0.
 * Any other cls_mode: OTAL_E_UNSUPPORTED. */
size_t otal_detection_loss_scratch_floats(int B, int K);
size_t otal_detection_loss_grad_floats(int B, int K, int C);
int otal_detection_loss(const float* loc, const float* conf, const float* prop_loc, const float* prop_conf,
                        const float* center, const float* act, const float* prop_act, const float* priors,
                        const float* gt, const unsigned char* gvalid, float* weight_accum, int B, int K, int C, int G,
                        float clip_length, float overlap_thresh, int ibm_active, int num_bins, float momentum,
                        int iou_aware, int cls_mode, float focal_alpha, float* losses, float* grads, float* scratch,
                        void* stream);

/* otal_detection_loss_ex: otal_detection_loss for the THUMOS14 loss ablations as well (configs/ablations/
 * thumos14_opental_{focal,ghm,ib,noACT}.yaml; AFSD/thumos14/cls_loss.py:221-256).  Arguments as otal_detection_loss, plus
 * `reweight`, the rule that weighs the EvidenceLoss rows that count (the positives in cls_mode 0, every anchor in cls_mode 2),
 * and rw_gamma.  An additive entry: OTAL_ABI_VERSION is unchanged.
 *   reweight 0 = otal_detection_loss(...) bit for bit, and cls_mode 2 accepts ibm_active as well: the IBM EMA over EVERY
 *                anchor of a closed set (noACT: os_head false with with_ibm);
 *   reweight 1 = focal-EDL: w = a_y (1 - max_k alpha_k / S)^rw_gamma with a_0 = focal_alpha, a_k = 1 - focal_alpha; the
 *                weight is NOT detached, the gradient includes per * dw/dz through the first maximum;
 *   reweight 2 = GHM: rows are binned by g = |1/alpha_y - C/S| into num_bins bins (edges i / num_bins, the last + 1e-6); bin
 *                0 also counts the M (C - 1) zeros of the other columns of the M rows that count; a populated bin's weight is
 *                1 / (its population, or with momentum > 0 its EMA weight_accum[i] = m * weight_accum[i] + (1 - m) * population)
 *                divided by the number of populated bins.  weight_accum (num_bins) is that EMA, updated in place (conf first,
 *                then prop_conf); momentum >= 0.  Counts are exact: the result does not depend on the order of the rows;
 *   reweight 3 = influence-balanced loss: w = 1 / (g |z|_1), no epsilon.
 * reweight 1..3 need cls_mode 0 or 2 and ibm_active 0; an epoch below the rule's start passes reweight 0 (the caller gates).
 * Anything else: OTAL_E_UNSUPPORTED, before any read or launch. */
int otal_detection_loss_ex(const float* loc, const float* conf, const float* prop_loc, const float* prop_conf,
                           const float* center, const float* act, const float* prop_act, const float* priors,
                           const float* gt, const unsigned char* gvalid, float* weight_accum, int B, int K, int C, int G,
                           float clip_length, float overlap_thresh, int ibm_active, int num_bins, float momentum,
                           int iou_aware, int cls_mode, float focal_alpha, int reweight, float rw_gamma, float* losses,
                           float* grads, float* scratch, void* stream);
/* otal_detection_loss_ev: otal_detection_loss_ex for cls_mode 0 and 2 with the other standard EDL settings of the reference
 * (AFSD/thumos14/cls_loss.py:171-190 get_loss_func / evidence_func, :193-209 mse_loss, :281-285 loglikelihood_loss;
 * training.edl_config.evidence and .loss_type of the yaml).  The arithmetic is csrc/evidence.h:
 *   evidence  0 exp(clamp(z, +-10)) (backward: exp(z) inside the closed interval, else 0), 1 relu (backward 0 at z == 0),
 *             2 softplus, beta 1, threshold 20 (backward 1 above the threshold, else sigmoid(z)); alpha = evidence + 1;
 *   loss_type 0 log S - log alpha_y, 1 digamma(S) - digamma(alpha_y) (fp32 recurrence up to 6, then the asymptotic series),
 *             2 mse: sum_k (y_k - alpha_k / S)^2 + sum_k alpha_k (S - alpha_k) / (S^2 (S + 1)).
 * The re-weighting rules (ibm_active, reweight 1..3) apply to loss_type 0 and 1 with the detached weights |1/alpha_y - C/S|
 * of the selected evidence; focal-EDL's weight carries gradient through d alpha / d z.  The reference's mse_loss applies no
 * rule: loss_type 2 with ibm_active or reweight != 0 is OTAL_E_UNSUPPORTED.  The IoU calibration uses u = C / S of the
 * selected evidence and no clamp: a relu row whose logits are all <= 0 has u = 1 and gives -inf, as the reference does.
 * (evidence, loss_type) = (0, 0) == otal_detection_loss_ex(...) bit for bit.  cls_mode 1 / 3, a kind out of range:
 * OTAL_E_UNSUPPORTED, before any read or launch.  An additive entry: OTAL_ABI_VERSION is unchanged. */
int otal_detection_loss_ev(const float* loc, const float* conf, const float* prop_loc, const float* prop_conf,
                           const float* center, const float* act, const float* prop_act, const float* priors,
                           const float* gt, const unsigned char* gvalid, float* weight_accum, int B, int K, int C, int G,
                           float clip_length, float overlap_thresh, int ibm_active, int num_bins, float momentum,
                           int iou_aware, int cls_mode, float focal_alpha, int reweight, float rw_gamma, int evidence,
                           int loss_type, float* losses, float* grads, float* scratch, void* stream);

/* The same for the ActivityNet1.3 recipe (ABI 22): AFSD/anet/multisegment_loss.py:87-301 with anet/cls_loss.py:78-246
 * (EvidenceLoss 'log', exp evidence, the closed-form influence-balanced weight 1 / (|z|_1 exp(ibm_coeff g) + 1e-10) whose
 * |z|_1 carries gradient, IoU calibration as each sample's mean) and :249-296 (ActionnessLoss with its rank hinge:
 * act_weight, act_margin).  Every term is evaluated per sample, normalised by that sample's counts and averaged over the
 * batch: one workgroup per sample + a seven-sum launch.  priors2 (K,2) = [centre, pyramid level]; level_bounds (nlev,2) =
 * the per-level (lower, upper] bounds on max(left, right) in frames (multisegment_loss.py:11); K <= 1024, nlev <= 8.
 * losses, grads: as otal_detection_loss (gradients already divided by B; otal_detection_loss_bwd applies);
 * scratch: 8 * B floats.  No state (this recipe's IBM weight has no EMA). */
int otal_detection_loss_anet(const float* loc, const float* conf, const float* prop_loc, const float* prop_conf,
                             const float* center, const float* act, const float* prop_act, const float* priors2,
                             const float* gt, const unsigned char* gvalid, int B, int K, int C, int G,
                             float clip_length, float overlap_thresh, const float* level_bounds, int nlev,
                             int ibm_active, float ibm_coeff, int iou_aware, float act_weight, float act_margin,
                             float* losses, float* grads, float* scratch, void* stream);
/* otal_detection_loss_anet_ex: otal_detection_loss_anet for the ActivityNet1.3 closed-set Softmax and EDL baselines as well
 * (os_head false: anet_softmax.yaml, anet_edl.yaml; multisegment_loss.py:226-257 without os_head).  Arguments as
 * otal_detection_loss_anet, plus cls_mode and focal_alpha, numbered as otal_detection_loss's:
 *   cls_mode 0 = the OpenTAL recipe above: otal_detection_loss_anet(...) == otal_detection_loss_anet_ex(..., 0, any, ...)
 *                bit for bit;
 *   cls_mode 2 = EvidenceLoss 'log' with exp evidence over all C logits (class 0 = background), EVERY anchor against its
 *                matched label (0 where unmatched); ibm_active must be 0 (OTAL_E_UNSUPPORTED otherwise); iou_aware as in
 *                mode 0, with u = C / S;
 *   cls_mode 3 = FocalLoss_Ori(balance_index 0, alpha = focal_alpha, gamma 2) on the softmax scores of every anchor;
 *                alpha[0] = focal_alpha belongs to the background; ibm_active and iou_aware are ignored.
 * In modes 2 and 3 act / prop_act may be NULL and act_weight / act_margin are ignored: losses 5 and 6 and the dact /
 * dprop_act gradient slots are written as 0.  Any other cls_mode: OTAL_E_UNSUPPORTED. */
int otal_detection_loss_anet_ex(const float* loc, const float* conf, const float* prop_loc, const float* prop_conf,
                                const float* center, const float* act, const float* prop_act, const float* priors2,
                                const float* gt, const unsigned char* gvalid, int B, int K, int C, int G,
                                float clip_length, float overlap_thresh, const float* level_bounds, int nlev,
                                int ibm_active, float ibm_coeff, int iou_aware, float act_weight, float act_margin,
                                int cls_mode, float focal_alpha, float* losses, float* grads, float* scratch, void* stream);
/* otal_detection_loss_anet_ev: otal_detection_loss_anet_ex for cls_mode 0 and 2 with the other standard EDL settings of the
 * reference's ActivityNet1.3 EvidenceLoss (AFSD/anet/cls_loss.py:153-172 get_loss_func / evidence_func, :175-191 mse_loss,
 * :242-246 loglikelihood_loss; training.edl_config.evidence and .loss_type of the yaml), numbered and computed as for
 * otal_detection_loss_ev (csrc/evidence.h; the four lanes of an anchor share its row through row_part / mse_part / row_finish):
 *   evidence  0 exp, 1 relu, 2 softplus; loss_type 0 log, 1 digamma, 2 mse (err + var, both summed).
 * ibm_active applies to loss_type 0 and 1: w = 1 / (|z|_1 exp(ibm_coeff g) + 1e-10) with the detached g = |1/alpha_y - C/S| of
 * the selected evidence, whatever the loss function; |z|_1 carries gradient.  Unlike _ex, cls_mode 2 takes ibm_active too
 * (the reference's with_ibm does not depend on os_head): every anchor, y = its matched label (0 = background), |z|_1 over all
 * C logits.  The reference's mse_loss applies no weight: loss_type 2 with ibm_active is OTAL_E_UNSUPPORTED.  The IoU
 * calibration uses u = C / S of the selected evidence and no clamp (a relu row with all logits <= 0 gives -inf, as the
 * reference does).  (evidence, loss_type) = (0, 0) == otal_detection_loss_anet_ex(...) bit for bit wherever that entry accepts
 * the call (it launches the same kernel instances).  cls_mode other than 0 or 2, a kind out of range, K > 1024, nlev > 8:
 * OTAL_E_UNSUPPORTED, before any read or launch; the null and shape checks are those of _ex.  An additive entry:
 * OTAL_ABI_VERSION is unchanged. */
int otal_detection_loss_anet_ev(const float* loc, const float* conf, const float* prop_loc, const float* prop_conf,
                                const float* center, const float* act, const float* prop_act, const float* priors2,
                                const float* gt, const unsigned char* gvalid, int B, int K, int C, int G,
                                float clip_length, float overlap_thresh, const float* level_bounds, int nlev,
                                int ibm_active, float ibm_coeff, int iou_aware, float act_weight, float act_margin,
                                int cls_mode, float focal_alpha, int evidence, int loss_type, float* losses, float* grads,
                                float* scratch, void* stream);

/* otal_detection_loss_rpl: the closed-set form of otal_detection_loss for the RPL and GCPL baselines (thumos14_open_rpl.yaml,
 * thumos14_open_gcpl.yaml; AFSD/thumos14/cls_loss.py:342-378 RPLoss, multisegment_loss.py:101-105,:201-204,:225-228).
 * Arguments as otal_detection_loss without the IBM / EMA state and the actionness maps; conf / prop_conf (B,K,C) are the
 * DISTANCES of otal_rpl_head_fwd.  Matching, the three localisation / quality terms, the layout of losses, grads and scratch
 * and otal_detection_loss_bwd are shared with cls_mode 2 / 3; losses 5 and 6 and the dact / dprop_act slots are 0.
 * The regulariser's (feats - centers[y]).pow(2).mean(1) equals d_i = dist[i][y_i], so the features are not an argument: their
 * gradient and the centres' are d loss / d dist pushed through otal_rpl_head_bwd.  With A = B K, CE_i the softmax
 * cross-entropy of row i against its matched label (0 = background), w = weight_pl:
 *   gcpl 0 (RPL)   coarse   (sum_i CE_i(dist_i / T) + w sum_i (d_i - radius)^2) / N
 *                  refined  ((1/A) sum_i CE_i(dist_i / T) + (w/A) sum_i (d_i - radius)^2) / PN
 *   gcpl 1 (GCPL)  coarse   (sum_i CE_i(-dist_i / T) + w/(2A) sum_i d_i) / N
 *                  refined  ((1/A) sum_i CE_i(-dist_i / T) + w/(2A) sum_i d_i) / PN
 * (the refined stage's mean that is still divided by PN, and GCPL's always-mean regulariser, are the reference's).
 * radius is the reference's never-trained one-element parameter (0).  gcpl other than 0 / 1, temperature <= 0 or
 * B K > 2048: OTAL_E_UNSUPPORTED. */
int otal_detection_loss_rpl(const float* loc, const float* conf, const float* prop_loc, const float* prop_conf,
                            const float* center, const float* priors, const float* gt, const unsigned char* gvalid,
                            int B, int K, int C, int G, float clip_length, float overlap_thresh, int gcpl,
                            float temperature, float weight_pl, float radius, float* losses, float* grads, float* scratch,
                            void* stream);

/* Backward of otal_detection_loss in one launch: the gradients w.r.t. the seven head outputs from the stored per-loss
 * gradients (`grads` as written by otal_detection_loss) and the incoming gradients of the seven losses g7[i] (device
 * scalars in the order loss_l, loss_c, loss_prop_l, loss_prop_c, loss_ct, loss_act, loss_prop_act; NULL = 0).
 * out: d_loc (2A) | d_prop_loc (2A) | d_conf (A C) | d_prop_conf (A C) | d_center (A) | d_act (A) | d_prop_act (A), A = B K.
 * Replaces the autograd of the weighted loss sum over multisegment_loss.py:92-259 (nine multiplies, two adds). */
int otal_detection_loss_bwd(const float* grads, const float* const* g7, float* out, int B, int K, int C, void* stream);

/* Clip preparation on the device: uint8 frames (T',Hs,Ws,3) -> normalised fp32 batch (B,3,T,Ho,Wo).
 * Replaces AFSD/common/thumos_dataset.py:136-137,:246-262 and videotransforms.py:44-124 (temporal zero padding,
 * random / centre crop, horizontal flip, float(), (x/255)*2-1, THWC -> CTHW).  params: device array of B records
 * {int64 frame0 (element offset of the clip's first frame in `frames`), int32 valid_t, crop_i, crop_j, flip}
 * = 24 bytes each (8-byte aligned); the random decisions are taken on the host exactly as the reference takes them.
 * flip bit 0 = mirror along W; flip bit 1 = the frames past valid_t are 127.5 before normalisation (exactly 0.0 after it),
 * the ActivityNet loader's padding (AFSD/common/anet_dataset.py:226-229), instead of 0 (-1.0 after it). */
int otal_prepare_clips(const unsigned char* frames, const void* params, float* out, int B, int T, int Hs, int Ws,
                       int Ho, int Wo, void* stream);
/* The same, plus the self-supervised branch's SPLICED clips from the same upload: out_ssl[b,:,t] = clip b's frame
 * frame_map[b*T + t] (frames >= valid_t, or a negative entry, are the zero padding).  Replaces THUMOS_Dataset.augment_
 * (AFSD/common/thumos_dataset.py:187-228: two time segments of the normalised clip change places), whose decisions stay
 * on the host.  `out` or `out_ssl` may be null (not both); frame_map is required with out_ssl. */
int otal_prepare_clips_map(const unsigned char* frames, const void* params, const int* frame_map, float* out,
                           float* out_ssl, int B, int T, int Hs, int Ws, int Ho, int Wo, void* stream);
/* otal_prepare_clips_map for source frames (T',Hs,Ws,C_src) written as C_out planes: out / out_ssl are (B,C_out,T,Ho,Wo).
 * Planes c < C_src are ((float)px / 255.0f) * 2.0f - 1.0f as above; planes C_src <= c < C_out are +0.0f everywhere, padding
 * frames included.  C_src = 2, C_out = 3 is how a 2-channel optical-flow clip is trained: Conv3d_1a multiplies the third
 * plane with an all-zero weight slice (common/i3d_backbone.py).  The same 24-byte records, flip bits and frame map; frame0
 * counts bytes of the C_src-channel buffer.  Supported: C_src in {2, 3} with C_src <= C_out <= 3 (else OTAL_E_UNSUPPORTED);
 * C_src = C_out = 3 gives otal_prepare_clips_map's result bit for bit.  Null and shape errors as above, answered before any
 * launch.  An additive entry: OTAL_ABI_VERSION is unchanged. */
int otal_prepare_clips_ch(const unsigned char* frames, const void* params, const int* frame_map, float* out, float* out_ssl,
                          int B, int C_src, int C_out, int T, int Hs, int Ws, int Ho, int Wo, void* stream);

/* Sliding windows of the inference path: B windows cut out of planar uint8 videos (C,Tv,H,W) resident on the device
 * -> normalised fp32 batch (B,C,T,H,W) in one pass.  Replaces AFSD/thumos14/test.py:67-76 prepare_clip per window
 * (float(), (x/255)*2-1 as torch evaluates it on the GPU: x times the fp32 reciprocal of 255; zero padding of a short
 * last window AFTER normalisation, unsqueeze) and the torch.cat of the
 * batch; test_cross_data.py:80-89 prepare_anet_clip gives the same values (127.5 padded before normalisation = 0.0).
 * params: device array of B records {uint64 src (device address of frame `offset`, channel 0, of the window's video),
 * int32 chan_stride4 (Tv*H*W/4), int32 valid_t (frames available from `offset`, <= T)} = 16 bytes each; H*W % 4 == 0
 * and 4-byte aligned videos (else OTAL_E_UNSUPPORTED). */
int otal_prepare_windows(const void* params, float* out, int B, int C, int T, int H, int W, void* stream);

/* ------------------------------------------------------------------ pyramid glue (ABI 24) ---- */

/* Pyramid merge (AFSD/thumos14/BDNet.py:310-326) in one launch: p0 (B,C,t0), p1 (B,C,t0/2) -> packed[:, :, :t0] = p0 +
 * nearest-upsampled p1 (source index t/2), packed[:, :, t0:t0+t0/2] = p1 (packed has T positions per row), and
 * frame (B,C,t0*up) = nearest-upsampled level 0 (source index t/up: F.interpolate(., [frame_num, 1])).  Backward: da, db
 * (B,C,T) gradients w.r.t. packed (first two levels read; db may be null), dframe (B,C,t0*up), dnext (B,C,t0/2; may be
 * null) the data gradient of the stride-2 layer reading level 1 -> dp0, dp1 (fixed summation order). */
int otal_pyramid_merge_fwd(const float* p0, const float* p1, float* packed, float* frame, int B, int C, int t0, int T,
                           int up, void* stream);
int otal_pyramid_merge_bwd(const float* da, const float* db, const float* dframe, const float* dnext, float* dp0, float* dp1,
                           int B, int C, int t0, int T, int up, void* stream);
/* otal_gn_relu_fwd with a strided destination: y[b*y_bs + c*y_cs + t] (a level slice of a packed buffer, a channel
 * slice of a concatenation buffer -- the torch.cat of AFSD/thumos14/BDNet.py:111 without the copy). */
int otal_gn_relu_fwd_to(const float* x, const float* gamma, const float* beta, float* y, int64_t y_bs, int64_t y_cs,
                        float* stats, int B, int C, int T, int G, float eps, int relu, int nlev, const int* lev, void* stream);
int otal_gn_relu_fwd_pair_to(const float* const* x, const float* const* gamma, const float* const* beta, float* const* y,
                             int64_t y_bs, int64_t y_cs, float* const* stats, int B, int C, int T, int G, float eps, int relu,
                             int nlev, const int* lev, void* stream);

/* otal_gn_relu_bwd whose output gradient is the SUM of n_terms (1..3) maps (B,C,dy_T[k] <= T) with their own batch / channel
 * strides (positions >= dy_T[k] of term k add nothing; summation order = term order): the gradient adds autograd issues for a
 * tensor with several consumers, done while the map is staged. */
int otal_gn_relu_bwd_sum(int n_terms, const float* const* dy, const int64_t* dy_bs, const int64_t* dy_cs, const int* dy_T,
                         const float* x, const float* gamma, const float* beta, const float* stats, float* dx, float* partial,
                         int B, int C, int T, int G, int relu, int nlev, const int* lev, void* stream);

/* otal_bmp_fwd_levels / otal_bmp_bwd_levels (fp32) with the pooled tensor (out resp. grad_out) a channel slice of a wider
 * (B,Ctot,N) buffer: pooled_bs = elements between samples (>= C*N).  The torch.cat of AFSD/thumos14/BDNet.py:111 and the
 * slice of its gradient, without copies. */
int otal_bmp_fwd_levels_to(const float* in, const float* seg, float* out, int64_t pooled_bs, int B, int C, int nlev,
                           const int* t_start, const int* n_start, void* stream);
int otal_bmp_bwd_levels_from(const float* grad_out, int64_t pooled_bs, const float* in, const float* seg, float* grad_in, int B,
                             int C, int nlev, const int* t_start, const int* n_start, void* stream);

/* ------------------------------------------------------------------ evaluation: greedy matching (csrc/eval.hip) ----
 * The prediction -> ground-truth matching of AFSD/evaluation/eval_detection.py (compute_average_precision_detection
 * :323-402, split_results_by_gt :405-456) for every group and tIoU threshold in ONE launch; the rule is stated in
 * opental_amd/evaluation/match.py (match_reference).  pred_seg (N, 2) and gt_seg (M, 2) hold [start, end] in fp64, sorted by
 * group; pred_start / gt_start are (ngroups + 1) non-decreasing offsets ending at N / M.  Predictions of a group are visited
 * in row order, a ground truth is taken once per threshold, thresholds are independent problems.  out (nthr, N):
 *   out[t][i] >= 0  the row of gt_seg that prediction i takes at thresholds[t]: among the untaken ground truths of its group
 *                   with not (tIoU < thresholds[t]) the one with the largest tIoU, the lowest row among equal tIoU;
 *   out[t][i] = -1  no such ground truth and some ground truth of the group has tIoU < thresholds[t], or the group has none;
 *   out[t][i] = -2  every ground truth of the group clears thresholds[t] and all are taken.
 * tIoU is fp64 in the operation order of utils_eval.segment_iou with an IEEE division, so every comparison equals numpy's.
 * *nonfinite (one int, zeroed by the caller) counts what makes the result unusable: every (prediction, ground truth) pair
 * with a non-finite tIoU (0 / 0 of two zero-length segments; treated as "not < threshold") and every group with
 * predictions and more than OTAL_EVAL_MAX_GT ground truths (all its predictions are written as -1).  A caller that reads a
 * non-zero counter discards `out`.  Pointers 16-byte aligned (segments) else OTAL_E_UNSUPPORTED; nthr > 32:
 * OTAL_E_UNSUPPORTED; ngroups < 0 or nthr < 1: OTAL_E_SHAPE; ngroups == 0 launches nothing.  An additive entry:
 * OTAL_ABI_VERSION is unchanged. */
#define OTAL_EVAL_MAX_GT 1024
int otal_eval_match(const double* pred_seg, const int* pred_start, const double* gt_seg, const int* gt_start,
                    const double* thresholds, int ngroups, int nthr, int* out, int* nonfinite, void* stream);

/* The labelled matching of the Wilderness-Impact pass (compute_wilderness_impact :604-728; the rule: match_labeled_reference
 * in opental_amd/evaluation/match.py).  As otal_eval_match, with pred_label (N) and gt_label (M) in the rows' order and these
 * differences: the ground truth that prediction i matches becomes taken only where gt_label == pred_label[i] (a true
 * positive); a false positive leaves it open for later predictions, so out[t][i] >= 0 can name the same row more than once.
 * -1 and -2 as above, "taken" read as "taken by a true positive".  max_tiou (N): the largest tIoU of prediction i over its
 * group's ground truths, whatever the threshold; 0 for a group without ground truth.  *nonfinite, the argument checks and
 * the return codes are otal_eval_match's; max_tiou is discarded with `out`.  An additive entry: OTAL_ABI_VERSION is unchanged. */
int otal_eval_match_labeled(const double* pred_seg, const int* pred_label, const int* pred_start, const double* gt_seg,
                            const int* gt_label, const int* gt_start, const double* thresholds, int ngroups, int nthr, int* out,
                            double* max_tiou, int* nonfinite, void* stream);

/* otal_average_precision (csrc/ap.hip): the average precision of every (class, tIoU threshold) from the codes of
 * otal_eval_match, i.e. the tail of compute_average_precision_detection (:388-402) with utils_eval.interpolated_prec_rec
 * (:20-29), on the device.  The rule is stated in opental_amd/evaluation/table_ap.py (ap_reference).
 *   codes (nthr, N) int32   out of otal_eval_match over group-sorted positions; >= 0 is a true positive;
 *   rank_pos (N) int32      the group-sorted position of the r-th row in (class, descending score, row) order;
 *   class_start (K + 1)     int32 offsets into rank_pos, non-decreasing, class_start[K] <= N (rows past it are in no class);
 *   gt_count (K) int32      ground truths per class (npos), all > 0;
 *   ap (nthr, K) fp64       every element is written; a class without rows gets 0.0.
 * Per (class, threshold): tp_cum_r = the true positives among the class's first r + 1 rows (int32), precision_r = tp_cum_r /
 * (r + 1), envelope_r = max over j >= r of precision_j, AP = sum over the true positives of (tp_cum_r / npos - (tp_cum_r - 1) /
 * npos) * envelope_r, all in fp64 with IEEE division.  One workgroup per (class, threshold) walks the class in chunks of
 * OTAL_AP_TILE rows from the back with carried count and carried maximum; the sum runs in one fixed order (inside a wave a
 * butterfly, the waves of a chunk in order, the chunks from the last to the first) that depends on OTAL_AP_TILE and the class
 * sizes alone: no atomic, no scratch, the same bits from run to run.  One launch on `stream`, no allocation, no
 * synchronisation.  class_start is clamped into 0 .. N and a rank_pos outside 0 .. N - 1 counts as a false positive.
 * NULL pointer: OTAL_E_NULL; N < 0, K < 1 or nthr < 1: OTAL_E_SHAPE; nthr > 32: OTAL_E_UNSUPPORTED.  The chunk bookkeeping
 * (int32 row numbers advanced by OTAL_AP_TILE) serves a class of up to OTAL_AP_MAX_CLASS_ROWS rows; no class is larger than
 * N, so the bound is checked on the host as N > OTAL_AP_MAX_CLASS_ROWS: OTAL_E_UNSUPPORTED, without reading class_start from
 * the device.  N == 0 writes zeros.  A refused call writes nothing.  An additive entry: OTAL_ABI_VERSION is unchanged. */
#define OTAL_AP_TILE 256
#define OTAL_AP_MAX_CLASS_ROWS (2147483647 - OTAL_AP_TILE)
int otal_average_precision(const int* codes, const int* rank_pos, const int* class_start, const int* gt_count, int N, int K,
                           int nthr, double* ap, void* stream);

/* otal_open_set_curves (csrc/oscurve.hip): AUROC, AUPR, FAR@95 and OSDR of every tIoU threshold from the matched detections
 * of the split pass, i.e. compute_auc_scores (:459-491) and compute_osdr_scores (:494-510) with the curve functions of
 * utils_eval, on the device.  The rule is stated in opental_amd/evaluation/table_open.py (open_reference).
 *   known (nthr, M) fp64    the known-ness of a threshold's matched detections, ascending, equal values by table row;
 *   flags (nthr, M) int32   bit 0: the matched ground truth is of an unknown class; bit 1: the predicted label equals the
 *                           ground truth's (ignored with bit 0); negative: an empty slot.  The list of a threshold is the
 *                           entries before its first empty slot, n <= M of them;
 *   out (nthr, 4) fp64      AUROC, AUPR, FAR@95, OSDR; every element is written, zeros for an empty list.
 * Per threshold, with ood = 1.0 - known (descending along the list), unknown the positive kind, P / Q the unknown / known
 * counts: a tie group ends where the next entry's ood differs; (fps, tps) at the group ends are the curve points
 * (_binary_clf_curve).  AUPR = sum over the group ends of (recall - previous recall) * tps / (end + 1), recall = tps / P (1.0
 * where P = 0).  The ROC points are the group ends that roc_curve's drop_intermediate keeps (the first, the last and those
 * whose second difference of fps or of tps is not 0) after (0, 0); AUROC = sum of (fpr - previous fpr) * (tpr + previous
 * tpr) / 2.0 over them, 0.0 where P = 0 or Q = 0; FAR@95 = the fpr of the first point with the smallest |tpr - 0.95|, 0.0 where
 * P = 0, NaN where Q = 0.  OSDR = the trapezoid sum over (1, 1), the cuts 0 .. n-2 (FPR = unknown entries at or behind the cut
 * / P, 0.0 where P = 0; CCR = correct entries behind the cut / Q, 1.0 where Q = 0), (0, 0).  All in fp64 with IEEE division.
 * One workgroup of OTAL_AP_TILE threads per threshold walks the list in chunks from the front with carried counts, carried
 * group ends and a carried best point; the three sums run in one fixed order (inside a wave a butterfly, the waves of a
 * chunk in order, the chunks in order, the last ROC point last) that depends on OTAL_AP_TILE and n alone: no atomic, no
 * scratch, the same bits from run to run.  One launch on `stream`, no allocation, no synchronisation.  NULL pointer:
 * OTAL_E_NULL; M < 0 or nthr < 1: OTAL_E_SHAPE; nthr > 32 or M > OTAL_AP_MAX_CLASS_ROWS: OTAL_E_UNSUPPORTED.  M == 0 writes
 * zeros.  A refused call writes nothing.  An additive entry: OTAL_ABI_VERSION is unchanged. */
int otal_open_set_curves(const double* known, const int* flags, int M, int nthr, double* out, void* stream);

/* otal_wilderness_impact (csrc/wi.hip): the Wilderness Impact of every (class, tIoU threshold) from the codes of
 * otal_eval_match_labeled, i.e. the tail of compute_wilderness_impact (:694-728) with utils_eval.interpolated_prec_rec
 * (:20-29), on the device.  The rule is stated in opental_amd/evaluation/table_wi.py (wi_reference, codes_reference).
 *   codes (nthr, N) int32   out of otal_eval_match_labeled over the positions of the pass order (video by video, table row
 *                           inside): >= 0 the row of gt_label matched, -1 background, -2 nothing;
 *   pred_label (N) int32    the label of a position's detection: 1 .. K, 0 = predicted unknown;
 *   gt_label (M) int32      the ground truths' labels in the rows that codes names: 1 .. K, 0 = unknown;
 *   n_known, n_unknown      the ground truths of the known classes (Kt >= 1) and of unknown ones (U >= 0), both and their
 *                           sum below OTAL_WI_MAX_GT = 2^24, where the host rule's float32 counts stop being exact;
 *   out (nthr, K) fp64      every element is written.
 * A row's outcome is match.wi_outcome_codes': with lp / lg the two labels, a matched row is tp_u2u (lp == lg == 0), tp_k2k
 * (lp == lg > 0), fp_u2k (lg == 0 < lp), fp_k2u (lp == 0 < lg) or fp_k2k; a background row is fp_bg2u (lp == 0) or fp_bg2k,
 * which counts as fp_k2k; code -2 has none.  A code outside -2 .. M - 1 or a label outside 0 .. K has none either and
 * gt_label is read at no other place than a code inside 0 .. M - 1.  Per (class c, threshold), with A_r / F_r the rows up to
 * and including r that are tp_k2k or fp_k2k / fp_u2k with lp == c + 1 and U_r those that are tp_u2u (int32):
 * precision_r = A_r / ((A_r + F_r) + 1e-6), envelope_r = max over j >= r of precision_j, recall_r = Kt / ((Kt + U) - U_r), and
 * WI = recall_0 * envelope_0 + the sum over the tp_u2u rows r > 0 of (recall_r - Kt / ((Kt + U) - (U_r - 1))) * envelope_r, all
 * in fp64 with IEEE division.  One workgroup of OTAL_AP_TILE threads per (class, threshold) walks the N rows in chunks from
 * the back with carried counts and a carried maximum; the sum runs in one fixed order (inside a wave a butterfly, the waves
 * of a chunk in order, the chunks from the last to the first) that depends on OTAL_AP_TILE and N alone: no atomic, no
 * scratch, the same bits from run to run.  One launch on `stream`, no allocation, no synchronisation.  NULL pointer:
 * OTAL_E_NULL; N < 0, M < 0, K < 1, nthr < 1, n_known < 1 or n_unknown < 0: OTAL_E_SHAPE; nthr > 32, N >
 * OTAL_AP_MAX_CLASS_ROWS or a ground-truth count at or above OTAL_WI_MAX_GT: OTAL_E_UNSUPPORTED.  N == 0 writes zeros.  A
 * refused call writes nothing.  An additive entry: OTAL_ABI_VERSION is unchanged. */
#define OTAL_WI_MAX_GT 16777216
int otal_wilderness_impact(const int* codes, const int* pred_label, const int* gt_label, int n_known, int n_unknown, int N,
                           int M, int nthr, int K, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
