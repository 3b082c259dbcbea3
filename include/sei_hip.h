/*
 * sei_hip.h -- C ABI of libsei_hip.so: the MI355X (gfx950) kernels behind the proposed-loss
 * training hot path of Scale-Equivariant-Imaging.
 *
 * Conventions (every entry point):
 *   - extern "C", returns int: 0 = ok, otherwise a hipError_t value (launch errors) or
 *     SEI_ERR_* (argument errors detected on the host BEFORE anything is launched). Never throws.
 *   - all tensor pointers are DEVICE pointers owned by the caller; nothing is allocated inside.
 *   - `stream` is a hipStream_t (passed as void* so that C callers need no HIP headers); all work
 *     is enqueued on it and the call returns without synchronising. No hidden globals: re-entrant.
 *   - float32 storage unless the name says bf16 (bf16 = upper 16 bits of an IEEE float32, passed as
 *     uint16_t*), float32 accumulation everywhere.
 *   - image tensors at the physics/loss boundary are NCHW planar ("planes" = B*C images of H x W);
 *     U-Net activations are NHWC ("rows" = B*H*W pixels of C contiguous channels).
 *
 * Each group cites the reference code (paths under the reference repo) whose arithmetic it replaces.
 * The reference is pure Python; it has no FFI of its own -- INTEGRATION.md shows the ctypes
 * binding a maintainer would add at each call site.
 */
#ifndef SEI_HIP_H
#define SEI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEI_OK 0
#define SEI_ERR_BAD_ARG 10001      /* NULL pointer, non-positive size, unsupported size */
#define SEI_ERR_TOO_LARGE 10002    /* a tile would not fit in LDS / a tap count above the limit */

/* ---------------------------------------------------------------------------------------------
 * STABLE SURFACE -- what a maintainer binding the reference's own modules needs (INTEGRATION.md section B shows the
 * ctypes stub for each at its reference call site); names, argument meaning and error behaviour are kept across ABI
 * versions:
 *   sei_abi_version, sei_build_target
 *   physics      sei_blur_sep_circ, sei_blur_dense_circ, sei_blur_dense_pad (+ _work_floats), sei_resample_sepband,
 *                sei_circ_filter_sep
 *   EI transform sei_scale_resample_fwd, sei_scale_resample_bwd
 *   loss terms   sei_axpy, sei_sure_terms, sei_mse_terms
 *   U-Net (f32)  sei_conv3x3_fwd, sei_conv3x3_bwd_weight, sei_dwconv7_fwd, sei_dwconv7_bwd_weight (+ _workspace),
 *                sei_ln_fwd, sei_ln_bwd (+ sei_ln_bwd_workspace), sei_gemm_f32, sei_colsum_f32, sei_sepmap2
 *   U-Net (bf16) sei_cast_bf16, sei_ln_fwd_bf16, sei_gemm_bf16nt
 *   optimizer    sei_adam_fused, sei_sgd_fused (+ sei_sgd_partials, sei_sgd_penalty_finish), sei_adam_anchor_fused
 *                (+ sei_adam_anchor_partials)
 *   baselines    sei_tv_prox (+ sei_tv_prox_work_floats), sei_bm3d_match (+ sei_bm3d_ref_blocks), sei_bm3d_ht,
 *                sei_bm3d_wiener, sei_bm3d_finish
 * INTERNAL -- everything else in this header: fused, schedule-specific (_ex, _ws, _dw2*, _plan, _eligible, _parts,
 * _count ...), SwinIR and measurement entry points that this build's own host layer (models/_ops.py, graphs.py, optim.py,
 * bench.py) calls. They are exported and documented here because that host layer sits above the C ABI, but they follow the
 * kernels: they may change with SEI_ABI_VERSION.
 * --------------------------------------------------------------------------------------------- */

/* ABI version of this header; sei_abi_version() returns the value the library was built with. Adding an entry point
 * is backward compatible and does not change it: sei_circ_filter_sep, sei_blur_sep_circ_lds, sei_resample_sepband_lds,
 * sei_blur_dense_pad, sei_blur_dense_pad_work_floats, sei_blur_decimate (+ _work_floats) and the sei_bm3d_* family joined version 12 that way (a binding written against an earlier 12 keeps working; one that needs a new symbol checks
 * for it by name). */
#define SEI_ABI_VERSION 12
int sei_abi_version(void);
/* Fills name[0..n) with the gfx target the code objects were built for ("gfx950"). */
int sei_build_target(char *name, int n);

/* Events that cross a hipGraph boundary: sei_event_record_external() issued on a capturing stream becomes an
 * event-record node of the graph (hipEventRecordExternal), recorded anew at that point of every replay;
 * sei_stream_wait_event() on another (non-captured) stream, issued after the replay was enqueued, waits for it.
 * `stream` arguments are hipStream_t; `event` is an opaque handle from sei_event_create. */
int sei_event_create(void **event);
int sei_event_destroy(void *event);
int sei_event_record_external(void *event, void *stream);
int sei_stream_wait_event(void *stream, void *event);

/* Measurement aid (bench.py): node counts of a captured hipGraph_t -- kernel nodes and all nodes. */
int sei_graph_node_counts(void *graph, int *kernel_nodes, int *all_nodes);

/* ---------------------------------------------------------------------------------------------
 * Physics: circular blur.
 * Replaces BlurV2.A, src/physics/blur/__init__.py:205-223 (rfft2 * OTF -> irfft2 == circular
 * convolution) and, with transpose=1, its autograd backward / A_adjoint (:225-227) == circular
 * correlation. Also serves the legacy Blur/conv/conv_transpose, :9-194 (same arithmetic).
 *   y[p,i,j] = sum_{a,b} tv[a]*th[b] * x[p, (i-a+kv/2) mod H, (j-b+kh/2) mod W]     (transpose=0)
 *   y[p,i,j] = sum_{a,b} tv[a]*th[b] * x[p, (i+a-kv/2) mod H, (j+b-kh/2) mod W]     (transpose=1)
 * tv (kv taps) and th (kh taps) are the rank-1 factors of the kernel (device pointers).
 * kv, kh <= 63.
 * One workgroup stages a 64 x 64 output tile with its halo in LDS; from 37 taps per axis on that is more than 64 KiB, and
 * the kernel's dynamic-LDS allowance is raised once per device on the first such call (see "Launches above 64 KiB of
 * LDS" below).
 * sei_blur_sep_circ_lds: the dynamic LDS bytes of the launch sei_blur_sep_circ would make for these taps and this image
 * (host arithmetic, nothing is launched; the entry point sizes its launch with the same function); 0 where it refuses.
 * ------------------------------------------------------------------------------------------- */
int sei_blur_sep_circ(const float *x, float *y, const float *tv, const float *th, int kv, int kh,
                      int planes, int H, int W, int transpose, void *stream);
size_t sei_blur_sep_circ_lds(int kv, int kh, int H, int W);
/* Non-separable kernels (loaded from a file, src/physics/__init__.py:20-22): k is (kv,kh) row-major. */
int sei_blur_dense_circ(const float *x, float *y, const float *k, int kv, int kh, int planes,
                        int H, int W, int transpose, void *stream);

/* The legacy Blur's other boundaries (src/physics/blur/__init__.py:34-161, conv / conv_transpose with padding
 * 'replicate', 'reflect', 'valid') for non-separable kernels; k is (kv,kh) row-major, H x W the IMAGE's extents in both
 * directions. mode: 1 replicate, 2 reflect, 3 valid (0, circular, is SEI_ERR_BAD_ARG: sei_blur_dense_circ is the circular
 * route). Per axis of K taps and image length n, (s, p) = (K/2, K/2) for odd K >= 3, (K/2 - 1, K/2) for even K, (0, 1)
 * for K = 1 (the reference flips the filter and zero-extends it to an odd length, at least 3):
 *   same-size modes  y[i]  = sum_a c[a] x[map(i - a + s)],     map(e) = min(max(e, 0), n-1)                   (replicate)
 *                                                              map(e) = e < 0 ? -e : e > n-1 ? 2(n-1) - e : e (reflect; needs
 *                                                              p <= n-1, SEI_ERR_BAD_ARG otherwise)
 *   valid            y[i'] = sum_a c[a] x[i' + p - a + s],     i' in [0, n - 2p)   (needs n > 2p, SEI_ERR_BAD_ARG otherwise)
 * in two dimensions the tensor product of the two axis rules applied to k[a,b]; y is (planes, H - 2pv, W - 2ph) in valid.
 * transpose = 1: the exact transpose (x is then the measurement-sized image -- the cropped one in valid -- and y is
 * H x W): out[u,v] = sum of Z[e,f] over the positions (e,f), e in [-pv, H-1+pv], f in [-ph, W-1+ph], that the two axis
 * maps send to (u,v), where Z[e,f] = sum_{a,b} k[a,b] x[e + a - sv, f + b - sh] with x zero outside its extent. Two
 * launches: Z into `work`, then a gather per output in a fixed order (no atomics: the same bits on every run); valid has
 * one preimage per position and is one launch, Z written straight to y.
 * sei_blur_dense_pad_work_floats: the floats `work` must hold: planes (H + 2pv) (W + 2ph) for the transposes of
 * replicate and reflect, 0 otherwise (work may then be NULL) -- and 0 for arguments the entry point refuses.
 * Limits as sei_blur_dense_circ: taps <= 63 per axis (SEI_ERR_TOO_LARGE beyond; a tile with its halo then fits 64 KiB of
 * LDS). SEI_ERR_BAD_ARG also on NULL pointers and when y or work overlap another operand. */
int sei_blur_dense_pad(const float *x, float *y, const float *k, int kv, int kh, int planes, int H, int W, int mode,
                       int transpose, float *work, void *stream);
size_t sei_blur_dense_pad_work_floats(int planes, int H, int W, int kv, int kh, int mode, int transpose);

/* INTERNAL (joined version 12 as an addition). The classical super-resolution degradation, blur then decimation, as one
 * operator (physics/blur_downsampling.py; no counterpart in the reference, whose src/physics/__init__.py:11 asks for it):
 * the blur above sampled at (phase_v :: rate, phase_h :: rate), evaluating the kept samples only. k is (kv,kh) row-major,
 * H x W the IMAGE's extents in both directions, rate 1..8, phases in [0, rate) and below the extent of their axis.
 * mode: 0 circular (the rule of sei_blur_dense_circ: map(e) = e mod n, S = K/2), 1 replicate, 2 reflect (the rules of
 * sei_blur_dense_pad: (S, p) as there; reflect needs p <= n-1). 3, valid, is SEI_ERR_BAD_ARG: the image is then not rate
 * times the measurement. Per axis of length n, n_out = (n - phase + rate - 1) / rate:
 *   transpose = 0   y[i'] = sum_a c[a] x[map(rate i' + phase - a + S)],   i' in [0, n_out);   x (planes,H,W), y (planes,
 *                   n_out_v, n_out_h). With rate 1 this is the blur itself.
 *   transpose = 1   the exact transpose: x is the measurement-sized image, y is H x W,
 *                   out[u] = sum over (i', a) with map(rate i' + phase - a + S) == u of c[a] x[i'].
 * A gather in a fixed order, no atomics: the same bits on every run. Each pixel visits only the taps whose residue mod
 * rate reaches it. Replicate / reflect: the zero-boundary correlation on the canvas extended by p goes to `work`, then the
 * fold of sei_blur_dense_pad (two launches). Circular: one launch, the wraps are folded in the kernel, whatever their
 * number (kernels larger than the image included); work may be NULL.
 * sei_blur_decimate_work_floats: the floats `work` must hold: planes (H + 2pv) (W + 2ph) for the transposes of replicate
 * and reflect, 0 otherwise -- and 0 for arguments the entry point refuses (the phases are taken as 0).
 * Taps <= 63 per axis (SEI_ERR_TOO_LARGE beyond). No launch asks for more than 64 KiB of LDS: the forward tile (16 x 32
 * measurement pixels) is halved until its footprint, (tile - 1) rate + K per axis, fits. SEI_ERR_BAD_ARG on NULL pointers,
 * on a rate or phase outside its range, and when y or work overlap another operand; all before any launch. */
int sei_blur_decimate(const float *x, float *y, const float *k, int kv, int kh, int planes, int H, int W, int mode,
                      int rate, int phase_v, int phase_h, int transpose, float *work, void *stream);
size_t sei_blur_decimate_work_floats(int planes, int H, int W, int kv, int kh, int mode, int rate, int transpose);

/* ---------------------------------------------------------------------------------------------
 * Physics: separable dense circular filter  y[p] = C_v * x[p] * C_h^T  with full circulants
 *   C_v[i][r] = cv[(i - r) mod H],  C_h[c][j] = ch[(c - j) mod W]
 * given by their first columns cv (H floats) and ch (W floats), device pointers.
 * Replaces CTLikeFilter.A / A_dagger, src/physics/ct_like_filter.py:10-18 (filter1d along H then W; each filter1d,
 * :20-39, is irfft(rfft(x) * otf), i.e. multiplication by a real SYMMETRIC circulant whose first column the caller
 * builds on the host), and one filter1d alone when the other axis gets the identity column {1, 0, ..., 0}.
 * There is no transposed form and no `transpose` argument: with symmetric circulants the operator is its own
 * adjoint, so the autograd backward of a call is the same call. (First columns that are not symmetric are applied as
 * given, as the formula above says.)
 * One launch, no intermediate in global memory: one workgroup per (plane, strip of 32 output columns); the row pass
 * result stays in LDS until the column pass has consumed it. Each output keeps four partial sums per pass.
 * Any H, W >= 1. SEI_ERR_TOO_LARGE when the workgroup's tiles exceed LDS (160 KiB): 512 x 512 fits (137 KiB), the
 * bound is 136 * (H + W) + 1 KiB <= 160 KiB up to the rounding of the extents to 4 / 8 / 32.
 * Launches above 64 KiB of LDS (sei_circ_filter_sep, sei_blur_sep_circ, sei_resample_sepband): the one piece of state
 * behind these entry points. Above 64 KiB the kernel's dynamic-LDS allowance is raised once per device
 * (hipFuncSetAttribute to the 160 KiB of a CU, on the first such call; idempotent, one bit per (kernel, device)
 * remembered). That first call must be an eager one: a stream capture of such an extent comes after an eager call of
 * the same entry point on that device.
 * ------------------------------------------------------------------------------------------- */
int sei_circ_filter_sep(const float *x, float *y, const float *cv, const float *ch, int planes, int H, int W,
                        void *stream);

/* ---------------------------------------------------------------------------------------------
 * Physics: separable banded resampling  y[p] = Wv * x[p] * Wh^T.
 * Replaces Downsampling.A, src/physics/downsampling/__init__.py:16-19
 * (F.interpolate bicubic antialias=True), its autograd backward / true adjoint (:21-31, the
 * transposed band matrices), the deprecated adjoint (:33-34, plain bicubic upsample), and the
 * antialias pre-filter of the EI transform, src/transforms.py:46-57.
 * Band form per axis: row o of W has nb consecutive weights w[o*nb .. o*nb+nb) starting at input
 * index lo[o] (entries beyond the band are zero-padded; lo is non-decreasing; lo[o]+nb may exceed
 * the input size only on zero weights). stepv/steph = max_o (lo[o+1]-lo[o]) of each axis (the
 * caller built the bands on the host and knows it); it bounds the LDS footprint of a tile.
 * One workgroup stages the input footprint of a 16 x 32 output tile, ((tile - 1) * step + band) per axis, in LDS: a
 * 1356 x 2040 photograph resized to 256 x 385 (step 6, band 22) takes 105 KiB, so the kernel's dynamic-LDS allowance is
 * raised once per device on the first call above 64 KiB (see "Launches above 64 KiB of LDS" above). Where the footprint
 * exceeds the 160 KiB of a CU (reductions by 8 and more) the output tile is halved, the wider footprint first, until it
 * fits: SEI_ERR_TOO_LARGE only when the bands of a single output pixel do not.
 * sei_resample_sepband_lds: the dynamic LDS bytes of the launch sei_resample_sepband would make (host arithmetic,
 * nothing is launched; the entry point sizes its launch with the same function); 0 where it refuses.
 * ------------------------------------------------------------------------------------------- */
int sei_resample_sepband(const float *x, float *y, int planes, int Hi, int Wi, int Ho, int Wo,
                         const float *wv, const int *lov, int nbv, int stepv,
                         const float *wh, const int *loh, int nbh, int steph, void *stream);
size_t sei_resample_sepband_lds(int Hi, int Wi, int Ho, int Wo, int nbv, int stepv, int nbh, int steph);

/* ---------------------------------------------------------------------------------------------
 * EI transform: per-image zoom-out by bicubic grid sampling with reflection.
 * Replaces padded_downsampling_transform + get_downsampling_grid, src/transforms.py:27-43,60-83
 * (F.grid_sample bicubic / reflection / align_corners=True on the grid (g - c)/rate + c); the grid
 * is generated in-kernel, never materialised. rate: (B,), center: (B,2) = (cx, cy) per image.
 * x is (B,C,Hi,Wi), y is (B,C,H,W); (Hi,Wi) = (H,W) except for --ScalingTransform__antialias, where the
 * reference samples the pre-shrunk image on the grid of the original shape (transforms.py:63-76).
 * _bwd accumulates d x (must be zero-filled by the caller) -- only needed with
 * --no-ProposedLoss__stop_gradient.
 * ------------------------------------------------------------------------------------------- */
/* The scale transform's per-image parameters from its two uniform draws (sample_from / sample_downsampling_parameters,
 * /root/reference/src/transforms.py:5-24): rate[i] = table[floor(ntable * u[i])], center[2 i + k] = 2 v[2 i + k] - 1
 * (u (B), v (B, 2) uniform in [0, 1) from the caller's generator): the reference's float32 operations, one launch. */
int sei_scale_params(const float *u, const float *v, const float *table, int ntable, int B, float *rate, float *center,
                     void *stream);
int sei_scale_resample_fwd(const float *x, float *y, const float *rate, const float *center,
                           int B, int C, int Hi, int Wi, int H, int W, void *stream);
int sei_scale_resample_bwd(const float *gy, float *gx, const float *rate, const float *center,
                           int B, int C, int Hi, int Wi, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Nearest-neighbour rotation about the image centre: the `Rotations` option of the equivariant loss
 * (src/losses/__init__.py:84-91 -> deepinv.transform.Rotate -> torchvision.transforms.functional.rotate with
 * its defaults: NEAREST, no expand, zero fill).  x, y: (planes, H, W).  (t00 t01; t10 t11) is the linear part
 * of torchvision's inverse affine matrix for the angle, rounded to float32 by the caller:
 * (cos a, -sin a; sin a, cos a) with a = the angle in radians.  _bwd accumulates into a zero-filled gx.
 * ------------------------------------------------------------------------------------------- */
int sei_rotate_nearest_fwd(const float *x, float *y, int planes, int H, int W, float t00, float t01, float t10,
                           float t11, void *stream);
int sei_rotate_nearest_bwd(const float *gy, float *gx, int planes, int H, int W, float t00, float t01, float t10,
                           float t11, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Loss-side streaming kernels.
 * sei_axpy: out = a + alpha*b  (GaussianNoise y + sigma*n, deepinv; SURE probe y + tau*b,
 *           src/losses/sure.py:24).
 * sei_sure_terms: src/losses/sure.py:24-31,57-62. Over the interior [m:H-m, m:W-m] of every plane:
 *   out[0] = sum b*(y2-y1)/tau ,  out[1] = sum (y1-y)^2      (sums; the caller divides)
 *   and, fused, the gradients of  L = c_mse*out[1] + c_div*out[0]  w.r.t. y1 and y2:
 *   g1 = 2*c_mse*(y1-y) - c_div*b/tau ,  g2 = c_div*b/tau   (zero outside the interior).
 *   margin_div / margin_mse select the two interiors separately (cropped_div flag, sure.py:51-54).
 *   `work` must hold 2*SEI_REDUCE_BLOCKS floats.
 * sei_mse_terms: deepinv mse metric used by EILoss (src/losses/__init__.py:117-122):
 *   out[0] = sum (a-b)^2 ; ga = scale*(a-b) (caller passes scale = 2*alpha/N). `work` as above.
 * ------------------------------------------------------------------------------------------- */
#define SEI_REDUCE_BLOCKS 256
int sei_axpy(const float *a, const float *b, float alpha, float *out, size_t n, void *stream);
/* out[0:n] = a, out[n:2n] = a + alpha b (sei_axpy's arithmetic): the 2B-image input [y, y + tau b] of the fused SURE pass
 * (src/losses/sure.py:24 + the model call on y) in one launch instead of axpy + torch.cat. n % 4 == 0, 16-byte aligned. */
int sei_stack_axpy(const float *a, const float *b, float alpha, float *out, size_t n, void *stream);
/* The eager prologue of a proposed-loss step (csrc/draws.hip).
 * sei_proposed_draws: the step's device-side draws in ONE launch, on the random stream of the torch calls they replace
 * (uniform draws bit-identical, normal draws to <= 3 ulp: csrc/draws.hip) --
 * torch.randn(B, C, H - 2m, W - 2m) into the interior of b (src/losses/sure.py:13-22; the border of b is not touched),
 * torch.rand(B) -> rate = table[floor(ntable u)], torch.rand(B, 2) -> centre = 2 u - 1 (src/transforms.py:5-24),
 * torch.randn(B, C, H, W) -> noise (deepinv GaussianNoise inside EILoss) -- for torch's CUDA generator at (seed, offset):
 * element i of each tensor = component x of rocrand_normal4 / rocrand_uniform4 of Philox4x32-10 (seed, subsequence i,
 * offset + 4 k), k = 0..3 in the order above. The caller advances the generator's offset by 16. B C H W <=
 * sei_proposed_draws_max_numel() (torch's one-element-per-thread regime), offset % 4 == 0.
 * sei_crop_window: out (planes, S, S) = the S x S window of y (planes, H, W) at (i0, j0), zero where the window leaves y
 * (src/crop.py:26-57 applied to a batch: the offset is drawn over the zero-padded extent). */
int sei_proposed_draws(unsigned long long seed, unsigned long long offset, float *b, int B, int C, int H, int W, int margin,
                       const float *table, int ntable, float *rate, float *center, float *noise, void *stream);
size_t sei_proposed_draws_max_numel(void);
int sei_crop_window(const float *y, float *out, int planes, int H, int W, int i0, int j0, int S, void *stream);
/* Glue of the step that torch ops used to provide (one launch each, so that a captured step holds no ATen kernel):
 * sei_concat2_f32: out = [a | b] (na, nb % 4 == 0; nb = 0: a plain copy) -- the joint backward's 3B-row gradient, a model
 * input into its arena buffer; sei_scale_dev_f32: out = x * (*scalar), the scalar on the device -- a loss term's stored
 * gradient times the incoming gradient of its value; sei_add_scalars: *out = *a + *b -- the sum of two loss terms. */
int sei_concat2_f32(const float *a, size_t na, const float *b, size_t nb, float *out, void *stream);
int sei_scale_dev_f32(const float *x, const float *scalar, float *out, size_t n, void *stream);
int sei_add_scalars(const float *a, const float *b, float *out, void *stream);
/* base[off_k .. off_k + len_k) = 0 for up to 8 (off, len) pairs of elements (HOST array of 2 * count values): the gaps of
 * the flat gradient bucket between the weight gradients that the captured step stores, in ONE launch (optimizer.zero_grad,
 * demo/train.py:258). */
int sei_zero_ranges(float *base, const unsigned long long *off_len_pairs, int count, void *stream);
int sei_sure_terms(const float *y, const float *y1, const float *y2, const float *b, int planes,
                   int H, int W, int margin_div, int margin_mse, float tau, float c_mse,
                   float c_div, float *out2, float *g1, float *g2, float *work, void *stream);
int sei_mse_terms(const float *a, const float *b, size_t n, float scale, float *out1, float *ga,
                  float *work, void *stream);

/* The two entry points above with the LOSS VALUE formed on the device as well (no chain of 0-dim torch kernels behind them):
 * sei_sure_loss: out3[0] = divergence sum, out3[1] = squared-error sum, out3[2] = c_mse out3[1] + c_div out3[0] - cst
 * (src/losses/sure.py:57-66: mse + 2 sigma^2 div - sigma^2 / B); y1 / y2 and g1 / g2 may be the two halves of one 2B-image
 * tensor (ProposedLoss evaluates A on both model outputs at once). sei_mse_loss: out2[0] = sum (a - b)^2, out2[1] =
 * value_scale out2[0] (deepinv's mse metric times the EI weight, src/losses/__init__.py:117-122). */
int sei_sure_loss(const float *y, const float *y1, const float *y2, const float *b, int planes, int H, int W,
                  int margin_div, int margin_mse, float tau, float c_mse, float c_div, float cst, float *out3, float *g1,
                  float *g2, float *work, void *stream);
int sei_mse_loss(const float *a, const float *b, size_t n, float grad_scale, float value_scale, float *out2, float *ga,
                 float *work, void *stream);
/* UNSURE (Tachella, Davies, Jacques: SURE with an unknown noise level; restated from the paper): sei_sure_loss with the
 * constant sigma^2 replaced by a Lagrange multiplier that lives in DEVICE memory and is moved by gradient ascent inside the
 * call, so that a captured step replays it. state = {eta, m, k, unused} (16-byte aligned): eta stands for sigma^2, m is the
 * averaged ascent direction, k the number of updates so far (as a float).
 *   stage 1   sei_sure_loss's with c_div = 2 state[0] inv_n_div read by every workgroup: g1 / g2 carry the multiplier as
 *             it stood BEFORE this call's update. y1 / y2 and g1 / g2 may be the halves of one 2B-image tensor.
 *   stage 2   out3 = {div sum, mse sum, c_mse out3[1] + 2 eta d}, d = out3[0] inv_n_div (no constant term); then, if
 *             `update` (0 or 1): g = 2 d, m' = g when k == 0 else momentum m + (1 - momentum) g, eta' = eta + step_size m',
 *             k' = k + 1. eta is not clamped. With update == 0 the state is not written.
 * Refused: what sei_sure_loss refuses, a null or misaligned state, momentum outside [0, 1), a non-finite step_size.
 * sei_axpy_sqrt_dev: out = a + sqrt(max(*p, 0)) b with p in device memory (the measurement noise of the equivariant branch
 * at the estimated level); sei_axpy's alignment. */
int sei_sure_loss_unsure(const float *y, const float *y1, const float *y2, const float *b, int planes, int H, int W,
                         int margin_div, int margin_mse, float tau, float c_mse, float inv_n_div, float step_size,
                         float momentum, int update, float *state, float *out3, float *g1, float *g2, float *work,
                         void *stream);
int sei_axpy_sqrt_dev(const float *a, const float *b, const float *p, float *out, size_t n, void *stream);
/* Poisson-Gaussian UNSURE (the same paper's signal-dependent case; restated from it): the noise variance at a pixel is
 * sigma^2 + gain * (clean value) with BOTH levels unknown, so the single multiplier becomes the affine weight eta + gamma y_i
 * inside the divergence, with one multiplier per zero-expected-divergence constraint. sei_sure_loss_unsure's two launches
 * with a third partial sum. state = {eta, m_eta, k, 0, gamma, m_gamma, 0, 0} (16-byte aligned; slots 0..2 as above).
 *   stage 1   D0 = sum_int_d b (y2 - y1) inv_tau, D1 = sum_int_d y b (y2 - y1) inv_tau, the mse sum; the gradients with
 *             the multipliers as they stood on entry: g2_i = ((2 w_i) inv_n_div) b_i inv_tau, w_i = fmaf(gamma, y_i, eta),
 *             g1_i = 2 c_mse (y1 - y)_i - g2_i, zero outside the respective interiors. y1 / y2 and g1 / g2 may be the
 *             halves of one 2B-image tensor. `work` holds 3 * SEI_REDUCE_BLOCKS floats.
 *   stage 2   out4 = {D0, D1, mse sum, c_mse out4[2] + 2 (eta d0 + gamma d1)}, d = D inv_n_div; then, if `update`, the
 *             ascent step above for each multiplier: eta along g = 2 d0 by step_eta, gamma along g = 2 d1 by step_gamma, one
 *             shared momentum, k' = k + 1 once. Neither multiplier is clamped. With update == 0 the state is not written.
 * With gamma == 0 (and step_gamma == 0) out4[0], out4[2], out4[3], g1, g2 and state[0..2] are sei_sure_loss_unsure's bits.
 * Refused: what sei_sure_loss_unsure refuses, and a non-finite step_gamma.
 * sei_axpy_hetero_dev: out_i = a_i + sqrt(max(fmaf(state[4], a_i, state[0]), 0)) b_i (the measurement noise of the equivariant
 * branch at the estimated, signal-dependent level); sei_axpy's float4 body, tail and alignment. */
int sei_sure_loss_unsure_pg(const float *y, const float *y1, const float *y2, const float *b, int planes, int H, int W,
                            int margin_div, int margin_mse, float tau, float c_mse, float inv_n_div, float step_eta,
                            float step_gamma, float momentum, int update, float *state, float *out4, float *g1, float *g2,
                            float *work, void *stream);
int sei_axpy_hetero_dev(const float *a, const float *b, const float *state, float *out, size_t n, void *stream);
/* Numerator of the luma PSNR of the evaluation step (reference src/metrics.py:10-13: kornia rgb_to_ycbcr's
 * Y = 0.299 R + 0.587 G + 0.114 B, torchmetrics PSNR with data_range 1): out1[0] = sum over the npix pixels of
 * (Y(a) - Y(b))^2 for planar RGB images a, b of shape (3, npix). `work` holds SEI_REDUCE_BLOCKS floats. */
int sei_luma_sqerr(const float *a, const float *b, size_t npix, float *out1, float *work, void *stream);
/* Luma SSIM of the evaluation step (reference src/metrics.py:15-18: kornia's Y as above, then torchmetrics
 * structural_similarity_index_measure with its defaults and data_range 1): out[i] = the mean over the (H-10) x (W-10)
 * windows that lie inside the image of the SSIM of Y(a[i]) and Y(b[i]) under the 11 x 11 Gaussian window of sigma 1.5
 * (torchmetrics reflect-pads by 5 and crops 5: the two cancel). a, b: `batch` planar RGB images (3, H, W), contiguous,
 * 4-byte aligned; H, W >= 11. `work` holds sei_ssim_luma_work_floats(batch, H, W) floats (0 = arguments refused).
 * Deterministic: no atomics; an image's result does not depend on the batch it is in. */
int sei_ssim_luma(const float *a, const float *b, int batch, int H, int W, float *out, float *work, void *stream);
size_t sei_ssim_luma_work_floats(int batch, int H, int W);

/* Equivariant bootstrap of the evaluation step (csrc/bootstrap_kernels.hip, bootstrap.py; Tachella and Pereyra,
 * "Equivariant bootstrapping for uncertainty quantification in imaging inverse problems", restated from the paper: no
 * package is ported and no parity with one is claimed). For replica r the host forms a_r = T_r x, measures it again through
 * the physics with fresh noise, reconstructs it as b_r, and takes the error of b_r against a_r as a sample of the error of x
 * against the truth. T_r is the padded zoom-out of the EI loss (bicubic A = -0.75, reflection, align_corners=True) by
 * rate[r] about (center[2r], center[2r + 1]) = (cx, cy). All three work on a grid laid out by rows and columns: pixel
 * (i, j) has the base coordinates x = (2 / W) j - 1, y = (2 / H) i - 1, in scale_taps' float32 operation order
 * (sei_scale_resample_fwd keeps the reference's transposed meshgrid; where H == W the two are the same bits).
 *   sei_boot_scale_fwd: y[r] = T_r x for r < B, sampled at (g - c) / rate + c. x is ONE (C, H, W) image that every replica
 *     reads; y is (B, C, H, W). The taps of a pixel are computed once for all channels.
 *   sei_boot_luma_diff: d[i] = Y(q(a_i)) - Y(q(b_i)) per pixel and out[i] = the sum of d[i]^2 over the image, for `batch`
 *     planar images a, b of shape (3, npix), contiguous, 4-byte aligned. q(t) = min(max(rintf(t * 255) / 255, 0), 1) with a
 *     correctly rounded division and ties to even (test.py's quantize_and_clamp in float32, bit for bit),
 *     Y = 0.299 R + 0.587 G + 0.114 B unfused and left to right (sei_luma_sqerr's). d is (batch, npix). `work` holds
 *     sei_boot_luma_diff_work_floats(batch, npix) floats (0 = arguments refused): the per-workgroup sums, which one wave per
 *     image adds in index order, in double. No atomics; an image's workgroups depend on npix alone, so its sum does not
 *     depend on the batch it is in.
 *   sei_boot_pullback_accum: msq[p] = (accumulate ? msq[p] : 0) + sum_{r < B} v_r^2, v_r the same bicubic gather from the
 *     (H, W) plane d[r] at rate (g - c) + c (the sample points lie inside the image; taps past the border reflect), added
 *     in the order of r as acc = fmaf(v_r, v_r, acc): calls over consecutive chunks of replicas, the later ones with
 *     accumulate != 0, leave the bits of one call over all of them. The gather is an interpolating pull-back, not the
 *     inverse of T_r. One thread per pixel.
 * SEI_ERR_BAD_ARG on NULL pointers, non-positive counts, 2^30 pixels or more per plane (npix of sei_boot_luma_diff
 * included), more than 65535 images in sei_boot_luma_diff; nothing is launched then. */
int sei_boot_scale_fwd(const float *x, float *y, const float *rate, const float *center, int B, int C, int H, int W,
                       void *stream);
int sei_boot_luma_diff(const float *a, const float *b, int batch, size_t npix, float *d, float *out, float *work,
                       void *stream);
size_t sei_boot_luma_diff_work_floats(int batch, size_t npix);
int sei_boot_pullback_accum(const float *d, const float *rate, const float *center, int B, int H, int W, float *msq,
                            int accumulate, void *stream);

/* Noise levels from measurements alone (csrc/noise_est_kernels.hip, noise_estimation.py; DESIGN 4.20: the project's own
 * definition, no parity with a published estimator is claimed). The operators here are blurs and antialiased downsamplings,
 * so the diagonal Haar detail of y is almost pure noise. Constants: L = 64 intensity levels, K = 256 magnitude bins, lattice
 * 510, c = 0.6744897501960817 (the median of |N(0, 1)|), LEVEL_LO = 6, LEVEL_HI = 57, N_MIN = 256.
 *   sei_noise_quad_hist: for every non-overlapping 2 x 2 quad (a b / c d) of every plane of the float32 (planes, H, W) tensor
 *     y, top-left corner at an even row and an even column (a trailing odd row or column is ignored), in float32, unfused,
 *     in this order:
 *       s = ((a + b) + (c + d)) * 0.25f,   t = ((a - b) - (c - d)) * 0.5f;
 *       the quad counts only if all four pixels satisfy 0 < p < 1 (clipped and non-finite pixels are dropped);
 *       l = clamp((int)floorf(s * 64.f), 0, 63),   k = min(255, (int)floorf(fabsf(t) * 510.f + 0.5f)), product and sum rounded
 *       separately (bins one 8-bit half-step wide, centred on the lattice of quantised images; bin 255 takes the overflow);
 *       hist[l][k] += 1.
 *     hist: L x K unsigned 64-bit counters in device memory, 8-byte aligned. accumulate = 0 zeroes them first, on the stream;
 *     otherwise calls add up, so a folder pools into one histogram. Integer counts: independent of the order of the atomics,
 *     bit-reproducible. y: 4-byte aligned; a 16-byte aligned y with W % 4 == 0 takes the float4 path, the same counts.
 *   sei_noise_fit: out8 = (sigma, eta, gamma, levels_used, quads_counted, flags, 0, 0) in double precision, sequential loops
 *     in index order. Interpolated median med(h) of a K-bin row with total n: half = n / 2, j = the first bin whose inclusive
 *     prefix sum is >= half, below = the prefix sum before j, lo = max(j - 0.5, 0), hi = j + 0.5,
 *     med = (lo + (hi - lo) * (half - below) / h[j]) / 510. sigma = med(sum over l of hist[l]) / c. Level l is used when
 *     LEVEL_LO <= l <= LEVEL_HI, its total n_l >= N_MIN and its median bin is not 255; v_l = (med(hist[l]) / c)^2,
 *     m_l = (l + 0.5) / 64, weight w_l = n_l. (eta, gamma): the weighted least-squares line v = eta + gamma m from the centred
 *     sums (mbar = sum w m / sum w, vbar likewise, gamma = sum w (m - mbar)(v - vbar) / sum w (m - mbar)^2,
 *     eta = vbar - gamma mbar). Flags: 1 an empty histogram (sigma, eta, gamma NaN; the counts 0); 2 the pooled median is in
 *     bin 255 (sigma NaN); 4 fewer than two used levels or no spread of m (gamma = 0, eta = sigma^2); 8 gamma < 0 (gamma = 0,
 *     eta = vbar); 16 eta < 0 (eta = 0, gamma = sum w m v / sum w m^2).
 * SEI_ERR_BAD_ARG on NULL pointers, planes < 1, H < 2, W < 2 or H * W >= 2^30; nothing is launched then. */
int sei_noise_quad_hist(const float *y, int planes, int H, int W, unsigned long long *hist, int accumulate, void *stream);
int sei_noise_fit(const unsigned long long *hist, double *out8, void *stream);

/* Tiled inference (csrc/tile_kernels.hip, tiling.py, test.py --tile): one (C, H, W) image is cut into
 * overlapping tiles, a model runs on batches of them, and the tiles it returns are blended into one image. The plan of an
 * axis of length n with tile T and overlap v, 0 <= 2 v <= T: n <= T gives one tile of extent Te = n at origin 0; otherwise
 * Te = T, the stride is s = T - v, and the origins are 0, s, 2s, ... strictly below n - T followed by n - T (the last tile is
 * shifted back to end on the border; nothing is padded). Tiles are the product grid of the two axes, t = ty * nx + tx.
 * Origins are not passed: they follow from (H, Th, sy, ny) as o_k = k * sy for k < ny - 1 and o_last = H - Th, and the overlap
 * is Th - sy (on a single-tile axis it only caps the feather window). All extents are in pixels of the tensors of the call:
 * a plan multiplied by an integer is the plan of the multiplied image, which is how the output of an SR model is blended.
 * Window weight of position i inside a tile of extent Te at origin o, an integer:
 *   window 0 (uniform): 1;   window 1 (feather): min(i + 1, Te - i, max(v, 1));
 *   window 2 (crop): 1 if lo <= i < Te - hi, else 0, with lo = 0 if o == 0 else v / 2, hi = 0 if o + Te == n else v - v / 2
 *   (integer division: each pixel comes from tiles that see at least v / 2 pixels of context around it).
 *   sei_tile_gather: tiles[t - t0] = x[:, oy : oy + Th, ox : ox + Tw] for t = t0 .. t0 + n - 1, a contiguous (n, C, Th, Tw)
 *     batch; a bit-for-bit copy.
 *   sei_tile_blend: out[c, y, x] = (sum over the tiles t0 .. t0 + n - 1 that cover (y, x), in ascending t, of
 *     wy * wx * tiles[t - t0][c, y - oy, x - ox]) / (Sy(y) * Sx(x)), Sy and Sx the per-axis sums of the weights over every tile
 *     of the plan. The sum is acc = fmaf(w, value, acc), w = (float)(wy * wx) (exact: Th, Tw <= 2048), from 0 when
 *     accumulate == 0 and from the numerators already in out otherwise; a tile whose weight at a pixel is 0 is not read there.
 *     finish != 0 divides (correctly rounded, as sei_boot_luma_diff divides). Calls over consecutive chunks of tiles, the later
 *     ones with accumulate != 0 and the last with finish != 0, leave the bits of one call over all tiles: gather form, a thread
 *     owns output pixels and finds their at most 3 x 3 covering tiles arithmetically; no atomics.
 * Pointers are 4-byte aligned; 16-byte accesses are used wherever four floats of a row sit on the 16-byte grid, scalar ones
 * elsewhere, with the same bits. SEI_ERR_BAD_ARG, with nothing launched, on NULL or misaligned pointers, non-positive extents
 * or C, Th or Tw above 2048, a stride above its tile, 2 (Th - sy) > Th where ny > 1 (likewise x), a (H, Th, sy, ny) that is not
 * the plan above (ny == 1 needs Th == H; otherwise (ny - 2) sy < H - Th <= (ny - 1) sy; likewise x), window outside 0 .. 2,
 * t0 < 0, n < 1, t0 + n > ny * nx, 2^30 pixels or more per plane, 2^31 (tile, channel) planes or more in the chunk, or an image
 * that overlaps the tile batch. */
int sei_tile_gather(const float *x, float *tiles, int C, int H, int W, int Th, int Tw, int sy, int sx, int ny, int nx,
                    int t0, int n, void *stream);
int sei_tile_blend(const float *tiles, float *out, int C, int H, int W, int Th, int Tw, int sy, int sx, int ny, int nx,
                   int window, int t0, int n, int accumulate, int finish, void *stream);

/* LPIPS v0.1 on AlexNet features (csrc/lpips_kernels.hip; reference src/metrics.py: pyiqa.create_metric("lpips")), float32.
 * For an H x W RGB image in [0, 1] (H, W >= 31: below that the second pool has nothing to work on):
 *   v = ((2 x - 1) - shift) / scale per channel, shift = (-0.030, -0.088, -0.188), scale = (0.458, 0.448, 0.450);
 *   layer 0: relu(conv(v; 3 -> 64, k 11, stride 4, zero pad 2)), then maxpool(3, stride 2, floor mode, no padding);
 *   layer 1: relu(conv(64 -> 192, k 5, pad 2)), then the same pool;  layers 2, 3, 4: relu(conv(k 3, pad 1)) with
 *   192 -> 384, 384 -> 256, 256 -> 256 channels. The zero padding of layer 0 pads v, not x: a padded tap contributes 0.
 *   d_l = mean over pixels of sum_c lin_l[c] (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2 for the two images' maps of
 *   layer l, |.| the norm over the channels of the pixel; LPIPS = d_0 + d_1 + d_2 + d_3 + d_4.
 * Every entry takes the IMAGE extents H, W and the layer index and derives its own extents from them. Maps are
 * channels-last, [image][pixel][C], 16-byte aligned.
 *   sei_lpips_conv_relu: layer 0 reads `n` planar (3, H, W) images, 4-byte aligned, the first `split` of them from x and
 *     the rest from x2 (NULL with split == n), and applies the input scaling on load; layers 1 .. 4 read the n maps at x (the
 *     POOLED map for layers 1 and 2; x2 and split are ignored). w: the weight repacked to [Cout][K], 16-byte aligned: layer 0
 *     K = 384 = torch's (64, 3 * 11 * 11) rows padded with zeros; layers 1 .. 4 K = k * k * Cin in (ky, kx, ci) order (torch's
 *     weight.permute(0, 2, 3, 1)). bias [Cout]. y: n maps [Hout * Wout][Cout]. An implicit GEMM on the exact-float32 matrix
 *     instructions; the k-ordered chain is closed every 256 k.
 *   sei_lpips_maxpool: the pool behind layer 0 or 1, x = that layer's n maps.
 *   sei_lpips_layer_dist: out[i] = d_layer of fa's and fb's i-th maps (accumulate = 0) or out[i] += d_layer (accumulate != 0:
 *     called for layers 0 .. 4 in order it leaves the LPIPS). lin [C], non-negative. `work` holds 1024 floats per image, the
 *     per-workgroup partial sums, which one workgroup per image adds in index order in double.
 *   sei_lpips_work_floats: the floats one evaluation of `batch` pairs needs for everything between the images and the result
 *     (the 2 * batch maps of layer 0, its pooled maps, layer 1, its pooled maps, layers 2, 3, 4, in that order, then the
 *     partial sums); 0 = arguments refused.
 * SEI_ERR_BAD_ARG on NULL or misaligned pointers, non-positive counts, a layer outside its range and extents below 31 (or
 * above 32768, or more than 2^28 pixels); nothing is launched then. Deterministic: no atomics, and the grids depend on the
 * extents only, so an image's result does not depend on the batch it is in. */
int sei_lpips_conv_relu(const float *x, const float *x2, int split, const float *w, const float *bias, float *y, int layer,
                        int n, int H, int W, void *stream);
int sei_lpips_maxpool(const float *x, float *y, int layer, int n, int H, int W, void *stream);
int sei_lpips_layer_dist(const float *fa, const float *fb, const float *lin, int layer, int batch, int H, int W, float *out,
                         int accumulate, float *work, void *stream);
size_t sei_lpips_work_floats(int batch, int H, int W);

/* ---------------------------------------------------------------------------------------------
 * Baselines of the evaluation driver (csrc/tv_kernels.hip; reference src/models/tv.py).
 *
 * sei_tv_prox: `iters` iterations of the primal-dual loop for prox_{ths TV}(z), isotropic TV with Neumann differences
 * (deepinv v0.2.0's TVDenoiser as models/tv.py restates it: tau = 0.01, sigma = 1 / (8 tau), rho = 1.99), on `planes`
 * independent planes:
 *     x  = (x2 - tau nabla^T(u2) + tau z) / (1 + tau)
 *     v  = u2 + sigma nabla(2 x - x2);   u = v / max(|v|_2 / ths, 1)      per pixel, over the two directions
 *     x2 = x2 + rho (x - x2);   u2 = u2 + rho (u - u2)
 * z and x2 are [planes][H][W]; u2 is [2][planes][H][W], the vertical differences then the horizontal ones. x2 and u2
 * hold the incoming state and, on return, the state after `iters` iterations (the prox is x2). `work` holds
 * sei_tv_prox_work_floats(planes, H, W) = 3 planes H W floats (0 = arguments refused): the launches alternate between
 * the state and this copy. H, W >= 1 (tiled: no limit from LDS), iters >= 1, ths > 0; pointers 4-byte aligned.
 * SEI_ERR_BAD_ARG on NULL / non-positive arguments and when z, x2, u2 or work overlap; SEI_ERR_TOO_LARGE only where
 * the index arithmetic would overflow (more than 2^31 - 1 tiles, an extent above 2^30).
 * Deterministic, no atomics, and exact under splitting: a call of a + b iterations leaves the bits that a call of a
 * followed by a call of b leaves, whatever the schedule.
 *   _ex: the schedule as per-call arguments: tile = 32 | 64 and k = 1 | 2 | 4 | 5 | 10 | 20 iterations per launch
 *   (0 = the default of each); anything else is SEI_ERR_BAD_ARG. Same bits for every choice. */
int sei_tv_prox(const float *z, float *x2, float *u2, int planes, int H, int W, float ths, int iters, float *work,
                void *stream);
int sei_tv_prox_ex(const float *z, float *x2, float *u2, int planes, int H, int W, float ths, int iters, int tile, int k,
                   float *work, void *stream);
size_t sei_tv_prox_work_floats(int planes, int H, int W);

/* The Deep Image Prior decoder (reference src/models/dip.py; deepinv v0.2.0's ConvDecoder as models/dip.py restates it),
 * float32, ONE image, C = 32 channels (anything else: SEI_ERR_BAD_ARG). Activations are channels-last [H * W][32]; weights
 * are in torch's layout, as they lie in the flat parameter bucket: w [32][32][3][3], head w [Cout][32]. A stage stores
 * a_l = relu(conv3x3(nearest_upsample(BN_{l-1}(a_{l-1}))) + bias); BN_{l-1} reaches it as ss_prev = {scale[32], shift[32]}
 * applied on load (NULL: the identity, the first stage reading z), the nearest index is torch's
 * min(floor(dst * (float(in) / float(out))), in - 1), and the zero padding is zero AFTER the affine. Neither the
 * upsampled nor the normalised tensor is stored.
 *   sei_dip_stage_fwd        a_out [Hout * Wout][32] and stats = {mean[32], rstd[32], scale[32], shift[32]} of ITS batch
 *                            norm (training mode: biased variance over the Hout * Wout pixels, eps; scale = gamma rstd,
 *                            shift = beta - mean scale; stats + 64 is the next stage's ss_prev). Per-workgroup (sum, M2)
 *                            partials, combined pairwise in double: no cancellation.
 *   sei_dip_head_fwd         x_hat [Cout][H * W] (NCHW) = w BN(a) + bias, 1 <= Cout <= 8; ss = that BN's {scale, shift}.
 *   sei_dip_head_bwd         from g_x [Cout][H * W]: g_bn [H * W][32] (gradient at the BN's output), g_w [Cout][32], g_bias.
 *   sei_dip_stage_bwd_bn     g [H * W][32] holds the gradient at the BN's output and, on return, the gradient at the
 *                            convolution's output: relu_mask scale (g - mean(g) - x_norm mean(g x_norm)); g_gamma[32] =
 *                            sum g x_norm, g_beta[32] = sum g, with g_beta == g_gamma + 32 (their place in the bucket).
 *   sei_dip_stage_bwd_data   g_prev [Hin * Win][32]: the gradient at BN_{l-1}'s output -- the transposed convolution
 *                            gathered over the block of destination pixels that each source pixel feeds (no scatter).
 *   sei_dip_stage_bwd_weight g_w [32][32][3][3] and g_bias[32]; reads a_prev through the forward's load path.
 *   sei_dip_adam             torch.optim.Adam's update (sei_adam_fused's arithmetic, gradient scale 1) with the step's six
 *                            scalars read from the DEVICE array that sei_adam_scalars_to_device fills: a captured launch
 *                            serves every step.
 * `work` holds sei_dip_work_floats(H, W, C, Cout) floats for the OUTPUT extent of the call (0 = arguments refused); a
 * decoder takes the maximum over its stages. Extents 1 .. 16384 (beyond: SEI_ERR_TOO_LARGE); activation pointers 16-byte
 * aligned, everything else 4-byte. No atomics, fixed summation order: the same bits on every run. */
size_t sei_dip_work_floats(int H, int W, int C, int Cout);
int sei_dip_stage_fwd(const float *a_prev, const float *ss_prev, const float *w, const float *bias, const float *gamma,
                      const float *beta, float *a_out, float *stats, int Hin, int Win, int Hout, int Wout, int C, float eps,
                      float *work, void *stream);
int sei_dip_head_fwd(const float *a, const float *ss, const float *w, const float *bias, float *x_hat, int H, int W, int C,
                     int Cout, void *stream);
int sei_dip_head_bwd(const float *g_x, const float *a, const float *ss, const float *w, float *g_bn, float *g_w,
                     float *g_bias, int H, int W, int C, int Cout, float *work, void *stream);
int sei_dip_stage_bwd_bn(float *g, const float *a, const float *stats, float *g_gamma, float *g_beta, int H, int W, int C,
                         float *work, void *stream);
int sei_dip_stage_bwd_data(const float *g_conv, const float *w, float *g_prev, int Hin, int Win, int Hout, int Wout, int C,
                           void *stream);
int sei_dip_stage_bwd_weight(const float *g_conv, const float *a_prev, const float *ss_prev, float *g_w, float *g_bias,
                             int Hin, int Win, int Hout, int Wout, int C, float *work, void *stream);
int sei_dip_adam(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n, const float *hyper6,
                 void *stream);

/* ---------------------------------------------------------------------------------------------
 * U-Net (src/models/convolutional.py), NHWC activations ("rows" = B*H*W pixels of C channels).
 * Parameter-gradient outputs (gw, gb, ggamma, gbeta, colsum `out`) are ACCUMULATED into with float
 * atomics: zero them (or keep the running gradient in them) before the call.
 *
 * sei_conv3x3_fwd: UNet.in_conv / out_conv, :174-176 (3x3, zero 'same' padding, small channel counts).
 *   x is NCHW (nchw_in=1) or NHWC; y likewise (nchw_out); optional residual `res` in y's layout (the
 *   global residual x + x0, :246-247). transposed=1 evaluates the DATA gradient instead: pass the
 *   forward weight (Cout_f,Cin_f,3,3) with Cin=Cout_f, Cout=Cin_f, x = upstream gradient.
 * sei_conv3x3_bwd_weight: gw (Cout,Cin,3,3) += sum_p gy[p,co] x[p+tap,ci]; gb (Cout) += sum_p gy.
 * sei_dwconv7_fwd: ConvBlock.conv1, :36-38 -- depthwise 7x7, zero pad 3, w is (C,1,7,7) as torch stores
 *   it, bias may be NULL; y = conv + bias + res_scale*res when res != NULL (NHWC, same shape).
 *   flip=1 correlates with the flipped taps = the data gradient.
 * sei_dwconv7_bwd_weight: gw (C,49) += sum_p gy[p,c] x[p+tap,c]; gbias (C) += sum_p gy (may be NULL).
 * sei_ln_fwd / sei_ln_bwd: channel LayerNorm, :21-30 (eps inside the sqrt, biased variance). fwd
 *   saves per-row mean and rstd; bwd needs the fwd INPUT x. C <= 8192.
 * sei_gemm_f32: every 1x1 Conv2d (:40,42,106,143) and its gradients as a row-major GEMM on the
 *   exact-f32 matrix cores: D[M,N] = op(A)[M,K] * op(B)[K,N] with a fused epilogue.
 *   A is (M,K) row-major when transA=0, (K,M) row-major when transA=1;
 *   B is (K,N) row-major when transB=0, (N,K) row-major when transB=1. D is (M,N) row-major.
 *   SEI_EPI_ACCUM may split K across workgroups and combine with float atomics.
 *   sei_gemm_f32_ex adds a batch of `batch` independent problems (element strides) and a switch to
 *   forbid split-K (bitwise reproducible accumulation).
 * sei_sepmap2: IdealDownsample / IdealUpsample (:54-92,113-133) as the real separable rank-2 map
 *   y[b,:,:,c] = L1 X R1^T + L2 X R2^T (L: (Ho,Hi), R: (Wo,Wi), row-major), the DFT-matrix form of the
 *   reference's rfft2/fftshift/mask-or-embed/irfft2 sequence including its discarded ifftshift.
 *   Backward = the same call with the transposed matrices. `work` >= 2*B*Hi*Wo*C floats.
 * sei_colsum_f32: out[n] += sum_m X[m,n]  (bias gradients of the 1x1 convolutions).
 * sei_adam_fused: torch.optim.Adam step (demo/train.py:157-186; amsgrad=False) over one flat bucket;
 *   grad is multiplied by grad_scale first (1/world_size after a summing all-reduce). step >= 1.
 *   grad may be bf16 (grad_is_bf16: the all-reduced, bf16-compressed gradient bucket of parallel.py).
 *   param_bf16 (optional): bf16 copy of the updated parameters, written in the same pass.
 * ------------------------------------------------------------------------------------------- */
int sei_conv3x3_fwd(const float *x, const float *w, const float *bias, const float *res, float *y,
                    int B, int H, int W, int Cin, int Cout, int nchw_in, int nchw_out, int transposed,
                    void *stream);
int sei_conv3x3_bwd_weight(const float *x, const float *gy, float *gw, float *gb, int B, int H, int W,
                           int Cin, int Cout, int nchw_x, int nchw_gy, void *stream);
/* Two-stage form for the network's end convolutions (3 <-> 32 channels, UNet.in_conv / out_conv): _parts_count = the number
 * of partial rows the launch leaves (0: shape not served -- use sei_conv3x3_bwd_weight), each Cout * Cin * 9 + Cout floats:
 * the weight gradient in torch's (Cout, Cin, 3, 3) layout followed by the bias gradient. sei_fold_many adds the rows into
 * the gradients (SEI_FOLD_SPLIT with split = Cout * Cin * 9: a = gw, b = gb). No atomics. */
size_t sei_conv3x3_bwd_weight_parts_count(int B, int H, int W, int Cin, int Cout, int nchw_x, int nchw_gy);
int sei_conv3x3_bwd_weight_parts(const float *x, const float *gy, float *part, int B, int H, int W, int Cin, int Cout,
                                 int nchw_x, int nchw_gy, void *stream);

int sei_dwconv7_fwd(const float *x, const float *w, const float *bias, const float *res,
                    float res_scale, float *y, int B, int H, int W, int C, int flip, void *stream);
/* `work` holds per-workgroup partial sums (two-stage reduction, no atomics); it must have at least
 * sei_dwconv7_bwd_weight_workspace(B,H,W,C) floats. */
size_t sei_dwconv7_bwd_weight_workspace(int B, int H, int W, int C);
/* gw = gbias = NULL: the fold is left to sei_fold_many (kind SEI_FOLD_DWCONV7) -- the partial sums stay in `work`,
 * [workspace / (50 C)][50][C] floats. */
int sei_dwconv7_bwd_weight(const float *x, const float *gy, float *gw, float *gbias, int B, int H,
                           int W, int C, float *work, size_t work_floats, void *stream);
/* The same three with the caller's explicit kernel choice: seg = 0 chooses by shape (LDS-tiled, whole-image or
 * generic; what the plain entry points pass), seg = 1..64 takes the generic sliding-window kernels with that many
 * output columns per worker segment (tests compare the paths bit for bit). Per call, no library state. */
int sei_dwconv7_fwd_ex(const float *x, const float *w, const float *bias, const float *res,
                       float res_scale, float *y, int B, int H, int W, int C, int flip, int seg, void *stream);
size_t sei_dwconv7_bwd_weight_workspace_ex(int B, int H, int W, int C, int seg);
int sei_dwconv7_bwd_weight_ex(const float *x, const float *gy, float *gw, float *gbias, int B, int H,
                              int W, int C, float *work, size_t work_floats, int seg, void *stream);
/* (sei_dwconv7_fwd_ex only: seg = 65 takes the first LDS-tiled kernel, seg = 66 the pipelined LDS-DMA kernel
 * (H, W >= 8, C % 32 == 0, 16-byte aligned x / w; SEI_ERR_BAD_ARG otherwise) that seg = 0 prefers from 1024
 * (tile, channel group) stages on; all three agree bit for bit.)
 *
 * ConvBlock.conv1 -> LayerNorm (src/models/convolutional.py:36-39 with :21-30) in one call:
 *   h1 = dwconv7(x) + bias (f32, kept: the LayerNorm backward re-reads it), h2 = LN_C(h1) * gamma + beta as bf16
 *   (out16 = 1) or f32, mean / rstd per pixel. C = 32 on images of at least 8 x 8: ONE launch (a workgroup owns all
 *   channels of its pixels; LDS-DMA double-buffered halo tiles, half-wave transposing reductions); any other shape:
 *   sei_dwconv7_fwd followed by sei_ln_fwd[_bf16]. sei_dwconv7_ln_fwd_launches tells which (1 or 2).
 *   _ex: fuse = 0 as above, 1 = the fused launch (C = 32 or 128, else SEI_ERR_BAD_ARG), 2 = the two launches. */
int sei_dwconv7_ln_fwd(const float *x, const float *w, const float *bias, const float *gamma, const float *beta,
                       float *h1, void *h2, int out16, float *mean, float *rstd, int B, int H, int W, int C,
                       float eps, void *stream);
int sei_dwconv7_ln_fwd_ex(const float *x, const float *w, const float *bias, const float *gamma, const float *beta,
                          float *h1, void *h2, int out16, float *mean, float *rstd, int B, int H, int W, int C,
                          float eps, int fuse, void *stream);
size_t sei_dwconv7_ln_fwd_launches(int B, int H, int W, int C);

int sei_ln_fwd(const float *x, const float *gamma, const float *beta, float *y, float *mean,
               float *rstd, size_t rows, int C, float eps, void *stream);
/* bwd: gx is written, ggamma/gbeta are accumulated (+=). `work` holds per-row statistics and the
 * per-workgroup parameter-gradient partials that are folded in a fixed order (bitwise reproducible);
 * it needs sei_ln_bwd_workspace(rows, C) floats (0 for shapes served by the scalar kernels, which
 * accumulate with float atomics: C not 4*2^k below 512, or not a multiple of 4 above). */
size_t sei_ln_bwd_workspace(size_t rows, int C);
/* ggamma = gbeta = NULL: the fold is left to sei_fold_many -- the partial sums stay in `work`, [sei_ln_bwd_part_count]
 * [2 C] floats from float sei_ln_bwd_part_offset on (allowed where the count is > 0: not for the atomics shapes). */
size_t sei_ln_bwd_part_offset(size_t rows, int C);
size_t sei_ln_bwd_part_count(size_t rows, int C);
int sei_ln_bwd(const float *x, const float *gamma, const float *mean, const float *rstd,
               const float *gy, float *gx, float *ggamma, float *gbeta, size_t rows, int C,
               float *work, size_t work_floats, void *stream);
/* The same with a second gradient of the LayerNorm's input added in the same pass: gx = LN'(gy) + res (res may be NULL).
 * What autograd otherwise does with an extra elementwise kernel where a U-Net level's output feeds both the downsampler
 * and the skip connection (/root/reference/src/models/convolutional.py:226-232: `skips.append(x)` next to
 * `downsampling_layers[lvl](x)`). Shapes with sei_ln_bwd_part_count(rows, C) > 0 only. */
int sei_ln_bwd_res(const float *x, const float *gamma, const float *mean, const float *rstd,
                   const float *gy, const float *res, float *gx, float *ggamma, float *gbeta, size_t rows, int C,
                   float *work, size_t work_floats, void *stream);

/* The second stage of MANY two-stage reductions in one launch: the LayerNorm parameter gradients and depthwise weight
 * gradients of a whole backward pass (reference: the autograd of src/models/convolutional.py:21-39 accumulates each of
 * them into its parameter's .grad; here a reducing kernel leaves per-workgroup partial sums and a fold adds them up in a
 * fixed order). A job is ONE destination and the partial-sum arrays of up to three launches that add to it (the model
 * calls of a step that share the parameter), folded one after the other into the running value. The entry points that
 * are handed their destinations fold with the same device routine, one job per launch (the order of the additions is
 * stated once, at fold_entries in csrc/reduce_kernels.hip): bit-identical, in 1 launch instead of ~50 (U-Net step) / ~146
 * (SwinIR step).
 *   SEI_FOLD_SPLIT:   part[s]: [groups[s]][ncol]; entry e adds to a[e] (e < split), b[e - split] (e < 2 split) or
 *                     c[e - 2 split] (c may be NULL: dropped) -- sei_ln_bwd (ncol = 2 C, split = C),
 *                     sei_rowgemm_lnbwd_bf16 (ncol = 3 C), a plain column sum (ncol = split);
 *   SEI_FOLD_DWCONV7: part[s]: [groups[s]][50][split = C]; entry (t, c) adds to a[c * 49 + t] for t < 49 and to b[c]
 *                     (b may be NULL) for t = 49 -- sei_dwconv7_bwd_weight.
 * Destinations of different jobs must differ (checked). The partial sums must stay untouched until this launch. */
#define SEI_FOLD_SPLIT 0
#define SEI_FOLD_DWCONV7 1
#define SEI_FOLD_MAX_JOBS 48   /* (48 x 80 bytes of job table + the count: under the 4-KiB kernel-argument block) */
typedef struct SeiFoldJob {
    float *a, *b, *c;
    int ncol, split, kind, nseg;
    const float *part[3];
    int groups[3];
    int reserved;
} SeiFoldJob;
int sei_fold_many(const SeiFoldJob *jobs, int njobs, void *stream);

#define SEI_EPI_NONE 0
#define SEI_EPI_BIAS 1            /* D = acc + bias[n]                                        */
#define SEI_EPI_BIAS_GELU 2       /* D = acc + bias[n]; D2 = gelu(D)   (two outputs)          */
#define SEI_EPI_BIAS_RES 3        /* D = acc + bias[n] + R1 (+ R2 if non-NULL)                */
#define SEI_EPI_MUL_DGELU 4       /* D = acc * gelu'(R1)                                      */
#define SEI_EPI_ACCUM 5           /* D += acc   (gradient accumulation)                       */
#define SEI_EPI_BIAS_ROWSCALE 6   /* D = acc + bias[n]*R1[m]                                  */
#define SEI_EPI_BIAS_SCALE_RES 7  /* D = R2 + R1[m]*(acc + bias[n])  (stochastic depth: one factor per row; not in the
                                     quadrant-schedule kernel: sei_gemm_bf16nt takes a 128-row tile for it) */
int sei_gemm_f32(const float *A, const float *B, float *D, int M, int N, int K, int transA,
                 int transB, int epilogue, const float *bias, const float *R1, const float *R2,
                 float *D2, void *stream);
int sei_gemm_f32_ex(const float *A, const float *B, float *D, int M, int N, int K, int transA,
                    int transB, int epilogue, const float *bias, const float *R1, const float *R2,
                    float *D2, int batch, long long strideA, long long strideB, long long strideD,
                    int allow_splitk, void *stream);

/* Same contract on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16): A and B are float32 in HBM and
 * are rounded to bf16 (round-to-nearest-even) while being staged into LDS; accumulation, epilogue
 * and D stay float32. Throughput mode (--compute_dtype bf16); parity claims are made with sei_gemm_f32. */
int sei_gemm_bf16_ex(const float *A, const float *B, float *D, int M, int N, int K, int transA,
                     int transB, int epilogue, const float *bias, const float *R1, const float *R2,
                     float *D2, int batch, long long strideA, long long strideB, long long strideD,
                     int allow_splitk, void *stream);

/* sei_gemm_bf16_ex with per-operand storage types: a_is_bf16 / b_is_bf16 = the operand is bf16 in HBM. */
int sei_gemm_bf16_mixed(const void *A, int a_is_bf16, const void *B, int b_is_bf16, float *D, int M, int N,
                        int K, int transA, int transB, int epilogue, const float *bias, const float *R1,
                        const float *R2, float *D2, int batch, long long strideA, long long strideB,
                        long long strideD, int allow_splitk, void *stream);

/* bf16-mode support (all streaming): f32 -> bf16 cast; weight shadows w16 (R,C) and its transpose
 * wt16 (C,R) from the f32 master weight w (R,C) (either output may be NULL); channel LayerNorm with a
 * bf16 output (same statistics as sei_ln_fwd); column sums of a bf16 matrix (out[n] += sum_m X[m,n]). */
int sei_cast_bf16(const float *x, uint16_t *y, size_t n, void *stream);
int sei_weight_shadow_bf16(const float *w, uint16_t *w16, uint16_t *wt16, int R, int C, void *stream);
int sei_ln_fwd_bf16(const float *x, const float *gamma, const float *beta, uint16_t *y, float *mean,
                    float *rstd, size_t rows, int C, float eps, void *stream);
int sei_colsum_bf16(const uint16_t *X, float *out, size_t M, int N, void *stream);
/* Split-bf16 GEMM mode (--compute_dtype bf16x3: models/_ops.py gemm_x3; reference src/models/convolutional.py:33-51, float32
 * 1x1 convolutions). planes: 2 n bf16 -- planes[i] = bf16(x[i]) (head), planes[n + i] = bf16(x[i] - head) (remainder);
 * n % 4 == 0. A product a b is then evaluated as a_lo b_hi + a_hi b_lo + a_hi b_hi by three sei_gemm_bf16nt launches that
 * accumulate in float32; the two epilogues that are not additive run as the element-wise passes below (exact erf forms,
 * as SEI_EPI_BIAS_GELU / SEI_EPI_MUL_DGELU of sei_gemm_f32 apply them). */
int sei_split_bf16x2(const float *x, uint16_t *planes, size_t n, void *stream);
/* Three planes, for a reduction concatenated over the three products (weight gradients: planes of a reduction-major
 * operand stack along the reduction index, so ONE launch with K' = 3 K sums them): pattern 0 = [head, head, remainder]
 * (the A side), 1 = [head, remainder, head] (the B side). planes: 3 n bf16; n % 4 == 0. */
int sei_split_bf16x3(const float *x, uint16_t *planes, size_t n, int pattern, void *stream);
int sei_gelu_f32(const float *x, float *y, size_t n, void *stream);            /* y = gelu(x) */
int sei_mul_dgelu_f32(float *d, const float *h, size_t n, void *stream);      /* d *= gelu'(h) */
/* x (R,C) float32 or bf16 -> x16 (R,C) bf16 copy (optional, float32 input only) and xt16 (C,ldt) bf16
 * transpose (optional) whose columns R..ldt-1 are zero: a K-padded operand for sei_gemm_bf16nt.
 * colsum (optional): colsum[c] += sum_r x[r][c] in float32 -- the bias gradient, from the same pass. */
int sei_cast_transpose_bf16(const void *x, int x_is_bf16, uint16_t *x16, uint16_t *xt16, int R, int C,
                            int ldt, float *colsum, void *stream);
/* The plain cast with a WEIGHTED column sum in the same pass: colsum[c] += sum_r row_weight[r] x[r][c] (un-rounded input).
 * In models/_ops.DownsampleFn16 the 1x1 convolution runs behind the ideal downsampler (src/models/convolutional.py:136-150
 * commuted), where its bias enters as bias[c] * s[row], s = the resampler's response to a constant image: the bias gradient
 * is this weighted sum of the output gradient's rows, taken while that gradient is cast for the GEMMs. C % 4 == 0. */
int sei_cast_bf16_colsum_weighted(const float *x, uint16_t *x16, const float *row_weight, float *colsum, int R, int C,
                                  void *stream);
/* The same cast with its (weighted when row_weight != NULL) column sums left as PARTIAL sums, one row of C floats per row
 * block: part[g][c], g < sei_cast_bf16_colsum_parts_count(R, C) (0: shape not taken, C % 4 != 0). The bias gradients of a
 * backward pass (src/models/convolutional.py:33-51, 96-150: every 1x1 convolution's bias) then join the pass's other
 * partial sums in ONE sei_fold_many launch (SEI_FOLD_SPLIT, ncol = split = C) instead of ending every cast in one float
 * atomic per column and workgroup -- which is what sized the atomics form's grid (512 workgroups; 2048 here). ABI 11. */
size_t sei_cast_bf16_colsum_parts_count(int R, int C);
int sei_cast_bf16_colsum_parts(const float *x, uint16_t *x16, const float *row_weight, float *part, int R, int C,
                               void *stream);

/* Several bf16 transposes in ONE launch: job k copies src (R, C) bf16 to dst (C, R). The fused pointwise MLP's backward
 * (sei_mlp_fused_bwd) reads both 1x1 weights of a ConvBlock transposed (src/models/convolutional.py:33-51: conv2 / conv3);
 * their bf16 copies change with every optimizer step, so a step re-transposes the 8 small matrices of the two fused
 * levels: one launch instead of 8 of ~9 us. */
#define SEI_TRANSPOSE_MAX_JOBS 16
typedef struct SeiTransposeJob {
    const uint16_t *src;
    uint16_t *dst;
    int R, C;
} SeiTransposeJob;
int sei_transpose_bf16_many(const SeiTransposeJob *jobs, int njobs, void *stream);

/* Large-shape bf16 GEMM with bf16 operands in HBM:  D[M,N] = op(A) * op(B),  f32 accumulation.
 * Each operand is stored either K-contiguous (a_rmajor = 0: A is (M,K) row-major, b_rmajor = 0: B is (N,K)
 * row-major -- the "NT" form) or reduction-major (a_rmajor = 1: A is (K,M) row-major; b_rmajor = 1: B is
 * (K,N) row-major). lda / ldb = row strides in elements of the operand as stored (multiples of 8).
 * Forward 1x1 convolutions: A = activations, B = bf16 weight (N,K): both K-contiguous.
 * Data gradients dX = dY W: A = dY K-contiguous, B = the SAME bf16 weight read reduction-major.
 * Weight gradients dW += dY^T X (SEI_EPI_ACCUM): both operands reduction-major (reduction over pixels).
 * Direct-to-LDS staging (global_load_lds); reduction-major tiles are consumed with the transposing LDS
 * read ds_read_b64_tr_b16, so no transposed copies exist anywhere. 8 waves, 128x128 / 192x256 / 96x256
 * tiles. D32 (float) and/or D16 (bf16) receive the epilogue result; SEI_EPI_BIAS_GELU also writes gelu(D)
 * to D2_16 (bf16). Needs K % 8 == 0 (K tails are fed from a zero page), M % 8 == 0 / N % 8 == 0 for a
 * reduction-major A / B, 16-byte aligned operands. May split K (float atomics on D32, zero-filled first
 * unless accumulating) when the output is narrow. */
int sei_gemm_bf16nt(const uint16_t *A, int lda, int a_rmajor, const uint16_t *B, int ldb, int b_rmajor,
                    float *D32, uint16_t *D16, int M, int N, int K, int epilogue, const float *bias,
                    const float *R1, const float *R2, uint16_t *D2_16, void *stream);

/* Weight gradient of two passes in one launch: D[M,N] (+)= A1^T B1 + A2^T B2, bf16 operands stored
 * reduction-major (A1 (K1,M), A2 (K2,M), row stride lda; B1 (K1,N), B2 (K2,N), row stride ldb), f32 D.
 * accumulate=0 stores D (the first write of a step into a gradient that need not be zeroed first);
 * accumulate=1 adds. One pass over the 4*M*N-byte gradient instead of two read-modify-writes.
 * (reference: the two model calls per step of ProposedLoss, src/losses/__init__.py, whose 1x1-conv weight
 * gradients torch sums in AccumulateGrad.) */
int sei_gemm_bf16nt_dw2(const uint16_t *A1, const uint16_t *A2, int lda, const uint16_t *B1, const uint16_t *B2,
                        int ldb, float *D32, int M, int N, int K1, int K2, int accumulate, void *stream);

/* The two entry points above with the caller's explicit schedule choice (tests of every tile variant, tools/):
 * tile = 0 lets the dispatcher decide (what the plain entry points pass); 1, 2, 3, 5 = 128x128, 128x256, 192x256,
 * 96x256 tiles of the 128x128-style loop; 15 / 16 = its single-stage / 128x256 reduction-major variants;
 * 30-33 = the quadrant schedule of gemm_bf16pq.h with 256x256, 288x256, 288x128, 256x128 tiles (the 128-column ones on
 * three LDS stages; 38 / 39 = 288x128 / 256x128 on two). band > 0 fixes
 * the band width of the XCD-aware tile order (0 = automatic). A choice the operands do not allow falls back to
 * the automatic one. Per call: the library keeps no mutable state. */
int sei_gemm_bf16nt_ex(const uint16_t *A, int lda, int a_rmajor, const uint16_t *B, int ldb, int b_rmajor,
                       float *D32, uint16_t *D16, int M, int N, int K, int epilogue, const float *bias,
                       const float *R1, const float *R2, uint16_t *D2_16, int tile, int band, void *stream);
int sei_gemm_bf16nt_dw2_ex(const uint16_t *A1, const uint16_t *A2, int lda, const uint16_t *B1,
                           const uint16_t *B2, int ldb, float *D32, int M, int N, int K1, int K2, int accumulate,
                           int tile, void *stream);

/* sei_gemm_bf16nt with a bf16 result (SEI_EPI_MUL_DGELU or SEI_EPI_NONE) that also accumulates the result's column sums:
 * colsum[n] += sum_m D16[m][n] (the rounded values, as sei_colsum_bf16 over D16 would add them). In a ConvBlock's backward
 * (src/models/convolutional.py:33-51) D16 = gh3 = (dY W3) gelu'(h3) and its column sums are conv2's bias gradient: where
 * the launch takes the quadrant kernel unsplit they ride in its epilogue (no pass over gh3), elsewhere the column-sum
 * kernel follows. */
int sei_gemm_bf16nt_colsum(const uint16_t *A, int lda, int a_rmajor, const uint16_t *B, int ldb, int b_rmajor,
                           uint16_t *D16, int M, int N, int K, int epilogue, const float *R1, float *colsum, void *stream);

/* The schedule sei_gemm_bf16nt would take for a GEMM of these shapes, WITHOUT launching anything (host arithmetic only:
 * callable on a machine with no GPU): (family << 48) | (tile rows << 32) | (tile columns << 16) | K splits, with
 * family 1 = gemm_bf16nt_kernel (the 128x128-style loop, whatever its tile), 2 = gemm_bf16pq_kernel (the quadrant
 * schedule); 0 = arguments the entry point would refuse. out_f32 / out_bf16: which of D32 / D16 the call passes.
 * Operands are taken as densely packed and 16-byte aligned. For tests that pin which kernels the TIMED batch runs
 * (tests/test_loss_gpu.py::test_timed_configuration_vs_oracle): a dispatch change cannot silently move the benchmarked
 * launch set away from what the oracle comparison covered. (The reference has no counterpart: its GEMMs are torch's,
 * src/models/convolutional.py:33-51.) */
size_t sei_gemm_bf16nt_plan(int a_rmajor, int b_rmajor, int out_f32, int out_bf16, int M, int N, int K, int epilogue);

/* Split-K through slabs (ABI 11). sei_gemm_bf16nt_ex and sei_gemm_bf16nt_colsum (colsum != NULL: D16 only,
 * SEI_EPI_MUL_DGELU or SEI_EPI_NONE) with a caller-owned workspace for the K slices of the quadrant kernel: `ws` points to
 * ws_bytes (>= 16 KiB) of device memory, 256-byte aligned, whose FIRST 16 KiB ARE ZERO before the first call (tile counters:
 * every call leaves them zero again; the remainder needs no initialisation) and which only one stream uses at a time.
 * Each K slice of a tile stores its accumulators into its slab (write-through), draws a ticket from the tile's counter, and
 * the slice that draws the last one adds the other slabs to its registers and runs the whole epilogue: no zero-fill
 * launch, no float atomics (1.3 TB/s chip-wide on MI355X against ~6 TB/s of plain stores), results that do not depend on
 * the order in which slices finish when there are two of them, and EVERY epilogue may split (bf16 / GELU / GELU' results
 * and riding column sums included), which the atomics form could not offer. No workgroup waits for another. ws = NULL, a
 * workspace too small for the launch (16 KiB + tiles * slices * tile bytes) or a launch off the quadrant kernel: exactly
 * the entry points above. tile / band: as sei_gemm_bf16nt_ex (0 = automatic). splitk > 0 asks for that many slices where
 * the schedule can split (tests, experiments).
 * (The reference's GEMMs are torch's: src/models/convolutional.py:33-51, 96-150; this is how their K-heavy, row-poor
 * shapes -- 288 ... 3456 rows at the two deepest U-Net levels -- fill 256 CUs.)
 * sei_gemm_bf16nt_plan_ws: the schedule with a workspace of ws_bytes (as sei_gemm_bf16nt_plan; bit 15 of the split count
 * set when the slices meet in slabs). */
int sei_gemm_bf16nt_ws(const uint16_t *A, int lda, int a_rmajor, const uint16_t *B, int ldb, int b_rmajor,
                       float *D32, uint16_t *D16, int M, int N, int K, int epilogue, const float *bias,
                       const float *R1, const float *R2, uint16_t *D2_16, float *colsum, void *ws, size_t ws_bytes,
                       int tile, int band, int splitk, void *stream);
size_t sei_gemm_bf16nt_plan_ws(int a_rmajor, int b_rmajor, int out_f32, int out_bf16, int M, int N, int K, int epilogue,
                               size_t ws_bytes);

#ifdef SEI_TUNING
/* Tools-only build (make tuning -> libsei_hip_tuning.so; not part of libsei_hip.so).
 * sei_debug_tr_probe: what ds_read_b64_tr_b16 delivers for a 64x128 LDS image (tools/probe_tr_read.py).
 * sei_debug_set_nt_tile: process-wide default for the tile / band arguments above (100 + b = band b), so the
 * experiment scripts can steer GEMMs launched by the model code; adds tile codes 4, 11-14 (LDS-ring variants),
 * 20 (the 256x256 ping-pong schedule of gemm_bf16pp.h) and 34-37 (timing-only ablations, wrong results). */
int sei_debug_tr_probe(const uint16_t *in, uint16_t *out, int r0, int c0, void *stream);
int sei_debug_set_nt_tile(int code);
#endif

/* The ideal resamplers of the DEEPEST levels in one pass (csrc/sepmap_small.hip): input extents <= 8, output extents
 * <= 24, C % 64 == 0 -- the 6 x 6 and 3 x 3 images a 48-pixel crop becomes at 2048 - 8192 channels
 * (IdealDownsample / IdealUpsample, src/models/convolutional.py:54-92,113-133). x (B, Hi, Wi, C) -> y (B, Ho, Wo, C), NHWC
 * float32, y = L1 X R1^T + L2 X R2^T per image and channel, float32 FMAs; L1, L2: (Ho, Hi), R1, R2: (Wo, Wi) row-major
 * device arrays. One workgroup item = one image x 64 channels through LDS; no HBM intermediate. _eligible: 1 / 0. */
size_t sei_sepmap2_small_eligible(int B, int Hi, int Wi, int Ho, int Wo, int C);
int sei_sepmap2_small(const float *x, void *y, int out_bf16, int B, int Hi, int Wi, int Ho, int Wo, int C,
                      const float *L1, const float *R1, const float *L2, const float *R2, void *stream);
/* out_bf16 = 1 (and sei_sepmap2_bf16_out16 below for the matrix-core kernel): y is bf16, the float32 result rounded once
 * to nearest even -- the operand of the 1x1 convolution that models/_ops.DownsampleFn16 evaluates BEHIND the ideal
 * downsampler (src/models/convolutional.py:136-150 commuted): no float32 copy of the resampled tensor, no cast pass. */
int sei_sepmap2_bf16_out16(const float *x, uint16_t *y16, int B, int Hi, int Wi, int Ho, int Wo, int C,
                           const uint16_t *packed, void *stream);

int sei_sepmap2(const float *x, float *y, int B, int Hi, int Wi, int Ho, int Wo, int C,
                const float *L1, const float *R1, const float *L2, const float *R2, float *work,
                size_t work_floats, void *stream);
/* The same map with the four matrices packed for the kernel's scalar loads (what the build's host code uses):
 * RW[j][j'][t] = R_t[j'][j] with j' padded to a multiple of 24 (zeros), LH[i][t][i'] = L_t[i'][i] with i' padded
 * to a multiple of 24. Results are bit-identical to sei_sepmap2. */
/* The same map in the bf16 throughput mode, on the matrix cores (sepmap_mfma.hip): activations rounded to bf16 (x before
 * the W product, the intermediate between the products), the four matrices as bf16 head + remainder (exact to ~2^-17),
 * f32 accumulation and output. Eligible shapes only (sei_sepmap2_bf16_eligible: 12 <= Hi, Wi <= 64 with the
 * intermediate of one image x 16 channels in LDS, C % 16 == 0); SEI_ERR_BAD_ARG otherwise -- the caller takes
 * sei_sepmap2_packed. `packed`: the matrices in the kernel's LDS image, made once per map by sei_sepmap2_bf16_pack from
 * L1, L2: (Ho, Hi), R1, R2: (Wo, Wi) float32 row-major into sei_sepmap2_bf16_pack_elems(..) uint16 elements. */
int sei_sepmap2_bf16(const float *x, float *y, int B, int Hi, int Wi, int Ho, int Wo, int C, const uint16_t *packed,
                     void *stream);
int sei_sepmap2_bf16_pack(const float *L1, const float *R1, const float *L2, const float *R2, uint16_t *packed, int Hi,
                          int Wi, int Ho, int Wo, void *stream);
size_t sei_sepmap2_bf16_eligible(int B, int Hi, int Wi, int Ho, int Wo, int C);
size_t sei_sepmap2_bf16_pack_elems(int Hi, int Wi, int Ho, int Wo);
/* The same map at LARGE extents (Hi or Wi in 65 .. 256: the x4 network's 96- and 192-pixel levels, the un-cropped 256-pixel
 * series) on the matrix cores (csrc/sepmap_big.hip): both products as one batched constant-matrix GEMM kernel -- the matrix
 * (bf16 head + remainder) in registers, the activations streamed once through LDS -- with a bf16 intermediate in `work`
 * (sei_sepmap2_big_work_elems uint16). `packed` (sei_sepmap2_big_pack_elems uint16) from sei_sepmap2_big_pack, once per
 * map. sei_sepmap2_big_eligible != 0 says which shapes are built (C % 16 == 0); others stay on sei_sepmap2_packed. */
size_t sei_sepmap2_big_eligible(int B, int Hi, int Wi, int Ho, int Wo, int C);
size_t sei_sepmap2_big_pack_elems(int Hi, int Wi, int Ho, int Wo);
size_t sei_sepmap2_big_work_elems(int B, int Hi, int Wi, int Ho, int Wo, int C);
int sei_sepmap2_big_pack(const float *L1, const float *R1, const float *L2, const float *R2, uint16_t *packed,
                         int Hi, int Wi, int Ho, int Wo, void *stream);
int sei_sepmap2_big(const float *x, float *y, int B, int Hi, int Wi, int Ho, int Wo, int C, const uint16_t *packed,
                    uint16_t *work, void *stream);
int sei_sepmap2_packed(const float *x, float *y, int B, int Hi, int Wi, int Ho, int Wo, int C,
                       const float *RW, const float *LH, float *work, size_t work_floats, void *stream);

int sei_colsum_f32(const float *X, float *out, size_t M, int N, void *stream);
/* out[n] += sum_m row_weight[m] * X[m,n]: the bias gradient of a 1x1 convolution applied AFTER the ideal
 * downsampler (models/_ops.py, DownsampleFn: the bias enters as bias[n] * s[m], s = the resampler's response
 * to a constant image). */
int sei_colsum_weighted_f32(const float *X, const float *row_weight, float *out, size_t M, int N, void *stream);

/* Fused pointwise MLP of a ConvBlock at the shallow U-Net levels (csrc/mlp_fused.hip; C = 32 or 128; reference:
 * src/models/convolutional.py:40-51): out (M, C) = res_scale * x + conv3(gelu(conv2(h2))), h2 (M, C) bf16 = the
 * LayerNorm output, W2 (4C, C) and W3 (C, 4C) the bf16 1x1-convolution weights as stored, b2 / b3 float. The 4C-wide
 * hidden activation stays in registers (accumulator tiles re-used as MFMA operands).
 * sei_mlp_fused_bwd: from go (M, C) float: gh2 (M, C) float = gradient w.r.t. h2; go16 (M, C), h4 = gelu(h3) (M, 4C) and
 * gh3 (M, 4C) in bf16 = the operands of the two weight-gradient GEMMs (h3 = conv2(h2) is recomputed). W3T (4C, C) and
 * W2T (C, 4C) are the transposed bf16 weights. (Bias gradients: column sums of go and gh3, sei_colsum_*.)
 * sei_mlp_fused_eligible(M, C) != 0 where the fused form is built to win: C = 32, and C = 128 with M a multiple of 144
 * (csrc/mlp128.hip: nine-wave workgroups of 144 pixels, the weights through an LDS-DMA ring); the entry points take any
 * M for both widths, the caller takes the GEMMs where this says 0. */
size_t sei_mlp_fused_eligible(long long M, int C);
int sei_mlp_fused_fwd(const uint16_t *h2, const uint16_t *W2, const float *b2, const uint16_t *W3, const float *b3,
                      const float *x, float res_scale, float *out, int M, int C, void *stream);
int sei_mlp_fused_bwd(const float *go, const uint16_t *h2, const uint16_t *W2, const float *b2, const uint16_t *W3T,
                      const uint16_t *W2T, float *gh2, uint16_t *go16, uint16_t *h4, uint16_t *gh3, int M, int C,
                      void *stream);

/* ---- SwinIR building blocks (csrc/swin_kernels.hip; reference: deepinv.models.SwinIR as configured at
 * src/models/__init__.py:51-74 = the official SwinIR network_swinir.py; parity unpinned, see oracle/swinir_path.py).
 *
 * sei_swin_attn_fwd: WindowAttention.forward for every 8x8 window and head of a batch of B images of HxW tokens
 * (H, W multiples of 8). qkv (B*H*W, 3*heads*head_dim) = the qkv projection of the tokens in natural (b, y, x)
 * order; out (B*H*W, heads*head_dim) in the same order. The cyclic shift by `shift` (torch.roll of
 * SwinTransformerBlock.forward), window_partition / window_reverse, the relative-position bias
 * (table ((2*8-1)^2, heads), index computed in-kernel) and the -100 mask of shifted windows are index arithmetic
 * inside the kernel. scale = head_dim^-0.5 (applied to q first, as the reference). head_dim 30 (SwinIR), 32, 16, 8.
 * sei_swin_attn_bwd: dqkv (every element written) and dtable (+=, float atomics) from dout; the probabilities are
 * recomputed from qkv. Both forms ADD into dtable, never overwrite it: the caller zeroes it once per step. */
int sei_swin_attn_fwd(const float *qkv, const float *table, float *out, int B, int H, int W, int heads,
                      int head_dim, int shift, float scale, void *stream);
int sei_swin_attn_bwd(const float *qkv, const float *table, const float *dout, float *dqkv, float *dtable,
                      int B, int H, int W, int heads, int head_dim, int shift, float scale, void *stream);
/* The same two on the bf16 MFMA (csrc/swin_attn_mfma.hip, throughput mode): qkv (B*H*W, 3*heads*32) and out / dout
 * (B*H*W, heads*32) in bf16, every head padded from 30 to 32 dims (the pad dims must be zero in qkv; they come out
 * zero). dqkv is bf16, dtable float (+=).
 * lse (heads, B*(H/8)*(W/8) windows in partition order, 64 queries) float: the rows' log-sum-exp of the scaled, biased
 * and masked scores in log2 units, written by the forward pass when non-NULL and REQUIRED by the backward pass, which
 * rebuilds the probabilities from it (one exponential per element, no row maxima / sums) and takes
 * rowsum(dout * out) from the forward output `out` (ABI 9). */
int sei_swin_attn_fwd_bf16(const uint16_t *qkv, const float *table, uint16_t *out, float *lse, int B, int H, int W,
                           int heads, int shift, float scale, void *stream);
int sei_swin_attn_bwd_bf16(const uint16_t *qkv, const float *table, const uint16_t *out, const float *lse,
                           const uint16_t *dout, uint16_t *dqkv, float *dtable, int B, int H, int W, int heads,
                           int shift, float scale, void *stream);
/* Padded-grid form of an NHWC batch for the 3x3 convolutions with many channels (RSTB.conv, conv_after_body,
 * conv_before_upsample, upsample.*): xp = guard_rows zero rows of C floats, then (B, H+2, W+2, C) with a zero
 * border, then guard_rows zero rows. On that grid the convolution is nine row-shifted GEMMs over the same flat
 * array (row offset dy*(W+2)+dx), with no im2col buffer. sei_unpad_nhwc takes the interior of a (B, H+2, W+2, C)
 * result back to (B, H, W, C), applies LeakyReLU(0.01) when act = 1, then adds `res` when non-NULL. C % 4 == 0. */
int sei_pad_nhwc(const float *x, float *xp, int B, int H, int W, int C, int guard_rows, void *stream);
int sei_unpad_nhwc(const float *xp, const float *res, float *y, int B, int H, int W, int C, int act, void *stream);
/* y[m, n] = row_scale[m] * x[m, n] (row_scale may be NULL = 1), times 1 or 0.01 by the sign of leaky_gate[m, n]
 * when leaky_gate is non-NULL: the backward of stochastic depth (timm DropPath) and of LeakyReLU. N % 4 == 0. */
int sei_rowscale(const float *x, const float *row_scale, const float *leaky_gate, float *y, size_t M, int N,
                 void *stream);

/* ---- SwinIR throughput (bf16) path: csrc/swin_bf16_kernels.hip, csrc/gemm_bf16nt.hip ----
 * sei_pack: dst[i] = map[i] >= 0 ? src[map[i]] : 0, as bf16 (to_bf16 = 1) or float: the float32 parameter bucket into
 * the padded / permuted layouts the bf16 GEMMs read (heads 30 -> 32, channels 180 -> 192, 3x3 weights tap-major).
 * sei_unpack_add: dst[map[i]] += src[i] for map[i] >= 0: gradients in GEMM-output layout back into the bucket (a
 * parameter element appears at most once in a map). */
int sei_pack(const float *src, const int *map, void *dst, size_t n, int to_bf16, void *stream);
int sei_unpack_add(const float *src, const int *map, float *dst, size_t n, void *stream);
/* LayerNorm over C <= 256 channels (C % 4 == 0) of float32 rows -> bf16 rows of ldy elements, zeros beyond C; with
 * ones_col (ldy > C) column C holds 1.0, so that the weight gradient dY^T [LN(x) | 1] of the linear layer behind it
 * carries that layer's bias gradient in its column C (no separate column-sum pass over dY). */
int sei_ln_fwd_bf16_pad(const float *x, const float *gamma, const float *beta, uint16_t *y, float *mean,
                        float *rstd, size_t rows, int C, int ldy, float eps, int ones_col, void *stream);
/* Its backward: gx (rows, C) = LN'(gy) (+ res if non-NULL); gy float32 with row stride ldg; ggamma / gbeta += through
 * per-workgroup partial sums in `work` (>= sei_swin_partials_floats(C) floats) folded by a second launch: deterministic,
 * no atomics. */
size_t sei_swin_partials_floats(int C);
int sei_ln_bwd_pad(const float *x, const float *gamma, const float *mean, const float *rstd, const float *gy,
                   const float *res, float *gx, float *ggamma, float *gbeta, size_t rows, int C, int ldg,
                   float *work, size_t work_floats, void *stream);
/* y16[m, :C] = bf16(row_scale[m] * x[m, :]) (row_scale may be NULL), zeros up to ldy; colsum[c] += sum_m of the
 * scaled rows when non-NULL (the bias gradient of the linear layer whose output gradient this is; partial sums in
 * `work`, as sei_ln_bwd_pad). */
int sei_cast_pad_bf16(const float *x, const float *row_scale, uint16_t *y, float *colsum, size_t rows, int C,
                      int ldy, float *work, size_t work_floats, void *stream);
/* sei_pad_nhwc with bf16 output and the channel count padded from C to Cp (zeros). */
int sei_pad_nhwc_bf16(const float *x, uint16_t *xp, int B, int H, int W, int C, int Cp, int guard_rows, void *stream);
/* The same with channel C (the first padding channel, Cp > C) set to 1.0 in every row when ones_col: as the input grid
 * of a 3x3 convolution it meets zero weight columns in the forward product, and in the weight gradient
 * (sei_gemm_bf16nt_dw2_taps: D[t][n][c] = sum_rows gy[r][n] x[r + shift_t][c]) column C of every tap then holds
 * sum_rows gy[r][n] -- the convolution's BIAS gradient (nn.Conv2d.bias; reference construction
 * src/models/__init__.py:51-74), without a column-sum pass over gy. */
int sei_pad_nhwc_bf16_ones(const float *x, uint16_t *xp, int B, int H, int W, int C, int Cp, int guard_rows, int ones_col,
                           void *stream);
/* 3x3 convolution (stride 1, zero padding 1) as ONE implicit GEMM on that grid: D[r, n] = sum over taps t and
 * channels c of Ap[r + row_off9[t], c] * B[n, t * cin_pad + c] (+ bias[n]); Ap points at row 0 of the padded grid
 * (behind the guard rows), cin_pad % 64 == 0, B (N, 9 * cin_pad) bf16 tap-major. The im2col matrix exists only as
 * LDS tiles: every k-tile of the LDS-DMA stream is a 64-channel slice of one tap, fetched from the same array at that
 * tap's row shift. Rows r of the border are computed too (discard them: sei_unpad_nhwc). */
int sei_gemm_bf16nt_conv(const uint16_t *Ap, int cin_pad, const int *row_off9, const uint16_t *B, int ldb,
                         float *D32, uint16_t *D16, int M, int N, int epilogue, const float *bias, void *stream);
/* The same convolution with sei_unpad_nhwc in its epilogue: y (Bimg, H, W, N) float32 = [LeakyReLU 0.01 when act = 1]
 * (conv + bias) [+ res], Ap the zero-bordered (H + 2) x (W + 2) grids of Bimg images; the border pixels are computed and
 * dropped by the row-patch epilogue, the (grid rows, N) intermediate is never written. N % 4 == 0; res (same layout as
 * y) requires bias. Reference: nn.Conv2d(3x3, padding 1) (+ residual / LeakyReLU) of deepinv's SwinIR (RSTB.conv,
 * conv_after_body, the upsampler), forward and -- with the transposed tap-major weights -- data gradient. */
int sei_gemm_bf16nt_conv_unpad(const uint16_t *Ap, int cin_pad, const int *row_off9, const uint16_t *B, int ldb, float *y,
                               const float *res, int Bimg, int H, int W, int N, const float *bias, int act, void *stream);

int sei_adam_fused(float *param, const void *grad, int grad_is_bf16, float *exp_avg, float *exp_avg_sq,
                   size_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                   float grad_scale, uint16_t *param_bf16, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Optimizer step inside the weight-gradient GEMM (one GPU, bf16 mode; demo/train.py:157-186 + :262-270 fused):
 * sei_gemm_bf16nt_dw2_adam computes the same two-segment product as sei_gemm_bf16nt_dw2 -- the COMPLETE
 * gradient of an (M, N) weight for this step -- and, instead of storing it, applies torch.optim.Adam's update to
 * param / exp_avg / exp_avg_sq (and the bf16 shadow, optional) in the epilogue: the 4 B/parameter gradient is
 * neither written nor read back.  Identical per-element arithmetic to sei_adam_fused with grad_scale = 1.
 * hyper: DEVICE array of 6 floats for this step, {beta1, beta2, eps, weight_decay, lr / (1 - beta1^t),
 * 1 / sqrt(1 - beta2^t)}; sei_adam_scalars fills a HOST array with exactly the values sei_adam_fused derives from
 * (lr, betas, eps, weight_decay, step), so that fused and separate steps agree bit for bit.
 * ------------------------------------------------------------------------------------------- */
int sei_gemm_bf16nt_dw2_adam(const uint16_t *A1, const uint16_t *A2, int lda, const uint16_t *B1, const uint16_t *B2,
                             int ldb, float *param, float *exp_avg, float *exp_avg_sq, uint16_t *param_bf16,
                             const float *hyper, int M, int N, int K1, int K2, void *stream);
/* The same with the caller's schedule choice (tests of both kernels, tools/): tile 0 = the dispatcher's choice, 1 = the
 * 128 x 128 loop (gemm_bf16nt_kernel<..., ADAM>), 16 = the same loop's 128 x 256 tile on 32-row stages (M % 128 == 0 and
 * N % 256 == 0; every result bit-identical to tile 1: the same MFMA steps in the same order), 30 / 33 = the quadrant
 * schedule's 256 x 256 / 256 x 128 tiles with the same epilogue (gemm_bf16pq_kernel<..., ADAM>); a choice the operands do
 * not allow falls back to the 128 x 128 loop.
 * sei_gemm_bf16nt_dw2_adam_plan: the schedule such a call would take, coded as sei_gemm_bf16nt_plan's and likewise host
 * arithmetic only; 0 = arguments the entry point would refuse. */
int sei_gemm_bf16nt_dw2_adam_ex(const uint16_t *A1, const uint16_t *A2, int lda, const uint16_t *B1, const uint16_t *B2,
                                int ldb, float *param, float *exp_avg, float *exp_avg_sq, uint16_t *param_bf16,
                                const float *hyper, int M, int N, int K1, int K2, int tile, void *stream);
size_t sei_gemm_bf16nt_dw2_adam_plan(int M, int N, int K1, int K2, int tile);
/* Up to eight such GEMMs in ONE launch on the 128 x 256 tile (tile 16 above), one after the other (problem-major, every
 * job's tiles in the order the job would take alone): the jobs' workgroups share the chip's slots, so one job's main loops
 * run under another's parameter streams instead of every launch running all its loops and then all its epilogues. Per
 * job the MFMA steps, their order and the Adam arithmetic are those of sei_gemm_bf16nt_dw2_adam_ex (tiles 1 and 16):
 * every parameter, moment and bf16-copy bit is the same. One `hyper` serves all jobs. The table is copied into the
 * launch's arguments: it need not outlive the call. SEI_ERR_BAD_ARG, with nothing launched: njobs outside
 * 1..SEI_ADAM_GROUP_MAX_JOBS, a job that sei_gemm_bf16nt_dw2_adam_ex would refuse, M % 128 != 0 or N % 256 != 0, or two
 * jobs whose state arrays overlap.
 * sei_gemm_bf16nt_dw2_adam_groupable (host arithmetic): 1 = a problem the grouped launch takes AND gains from -- whole
 * 128 x 256 tiles, and too few of them to run many rounds of workgroups on its own. */
#define SEI_ADAM_GROUP_MAX_JOBS 8
typedef struct SeiAdamGemmJob {
    const uint16_t *A1, *A2;         /* (K1, lda) / (K2, lda) bf16, reduction-major as sei_gemm_bf16nt_dw2's */
    const uint16_t *B1, *B2;         /* (K1, ldb) / (K2, ldb) */
    float *param, *exp_avg, *exp_avg_sq;     /* (M, N), dense */
    uint16_t *param_bf16;            /* NULL, or the bf16 copy of param */
    int lda, ldb, M, N, K1, K2;
} SeiAdamGemmJob;
int sei_gemm_bf16nt_dw2_adam_group(const SeiAdamGemmJob *jobs, int njobs, const float *hyper, void *stream);
size_t sei_gemm_bf16nt_dw2_adam_groupable(int M, int N, int K1, int K2);
int sei_adam_scalars(float lr, float beta1, float beta2, float eps, float weight_decay, int step, float *out6_host,
                     void *stream);
/* the same values written to a DEVICE array by a launch on `stream` (what a training loop calls before every replay of
 * a captured step: stream-ordered, nothing on the host to overwrite while the GPU lags behind) */
int sei_adam_scalars_to_device(float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                               float *dev6, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Fine-tuning step (demo/train.py:157-186 with --fine_tuning; src/losses/weights_distance_loss.py): torch.optim.SGD
 * without momentum over elements [lo, hi) of one flat bucket, with the weights-distance penalty
 * lambd * sum_k mean((anchor_k - p_k)^2) / K and its gradient folded into the same pass. All pointers are the BUCKET's
 * (element 0), 16-byte aligned (param_bf16: 8). Per element, float32:
 *   d = p - anchor;  g' = grad_scale * g + 2 c d;  penalty += c d d (the p before the update);  p -= lr g'
 * and param_bf16 (optional) receives the bf16 copy of the updated p. coef64[b] = c = lambd / (K n_k) of the parameter
 * that owns elements [64 b, 64 b + 64): every parameter starts on a 64-element boundary of the bucket and the padding
 * (zero in every bucket: d = 0) changes nothing. anchor, coef64 and partials are given together or not at all (then
 * d = 0: plain SGD). lo, hi: multiples of 4, and of 64 with an anchor; anything else, NULL or misaligned pointers and an
 * empty range are SEI_ERR_BAD_ARG and nothing is launched.
 * The penalty is reproducible bit for bit: no float atomics; workgroup w writes its sum to partials[w] (double,
 * sei_sgd_partials(lo, hi, grid_cap) of them; 0 = arguments sei_sgd_fused refuses), and sei_sgd_penalty_finish -- one
 * workgroup -- adds `count` consecutive partials (of one or several sei_sgd_fused launches) in index order in double and
 * stores one float32 on the device. grid_cap: 0 = the library's grid (one two-quad trip per thread up to 2^20
 * workgroups), > 0 = at most that many workgroups, which then loop (tests, tools/exp_sgd.py). Same weights either way.
 * ------------------------------------------------------------------------------------------- */
size_t sei_sgd_partials(size_t lo, size_t hi, int grid_cap);
int sei_sgd_fused(float *param, const float *grad, const float *anchor, const float *coef64, size_t lo, size_t hi,
                  float lr, float grad_scale, uint16_t *param_bf16, double *partials, int grid_cap, void *stream);
int sei_sgd_penalty_finish(const double *partials, size_t count, float *penalty, void *stream);

/* The same step with torch.optim.Adam's update (--fine_tuning --optimizer Adam; amsgrad=False, coupled weight decay) over
 * elements [lo, hi) of the bucket: pointers are the BUCKET's (element 0), exp_avg and exp_avg_sq included, and coef64 is
 * indexed by the absolute block (element >> 6). Per element, float32, in this order (the library is built without
 * contraction, so the order is the contract):
 *   g' = grad_scale * g;  with an anchor: d = p - anchor;  g' = g' + (2 c) d;  penalty += (double)((c d) d)  (the p
 *   before the update);  then sei_adam_fused's update of (p, exp_avg, exp_avg_sq) from g', with lr / (1 - beta1^step) and
 *   1 / sqrt(1 - beta2^step) derived as sei_adam_fused derives them (double pow and sqrt, rounded once).
 * Without an anchor, and where p == anchor, the results are sei_adam_fused's bit for bit. exp_avg, exp_avg_sq, p and
 * (optional) the bf16 copy of the updated p are written in the same pass: 34 bytes per element with anchor and copy,
 * sei_adam_fused moves 30. Nothing outside [lo, hi) is read or written. Gradients are float32 only.
 * Argument rules are sei_sgd_fused's: anchor, coef64 and partials together or not at all; lo, hi multiples of 4, and of
 * 64 with an anchor; float streams 16-byte aligned, param_bf16 8, partials 8; step >= 1; grid_cap >= 0; anything else is
 * SEI_ERR_BAD_ARG and nothing is launched. Workgroup w writes its penalty sum to partials[w] from the same fixed shuffle
 * tree (sei_adam_anchor_partials(lo, hi, grid_cap) of them, sei_sgd_partials' values); sei_sgd_penalty_finish folds the
 * partials of one or several launches. */
size_t sei_adam_anchor_partials(size_t lo, size_t hi, int grid_cap);
int sei_adam_anchor_fused(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, const float *anchor,
                          const float *coef64, size_t lo, size_t hi, float lr, float beta1, float beta2, float eps,
                          float weight_decay, int step, float grad_scale, uint16_t *param_bf16, double *partials,
                          int grid_cap, void *stream);

/* The same two-segment weight gradient STORED as bf16 (whole-row 8-byte quads): with several GPUs and a bf16-compressed
 * gradient exchange the gradient is written straight into the exchange buffer (parallel.FlatGradientReducer.comm) --
 * no float32 copy of it, no cast pass (2.6 GB read + 1.3 GB written per step at the default size). Same rounding
 * (round-to-nearest-even of the float32 accumulator) as sei_cast_bf16 of the stored float32 gradient. */
/* The weight gradient of a 3x3 convolution on the zero-bordered grid (sei_gemm_bf16nt_conv), all taps in ONE launch:
 * D32 + t * tap_ld (M x N, float32) (+)= sum over rows r of A[r, :]^T B[r + tap_rows[t], :] for t < ntaps <= 9 -- the same
 * dY (A1 / A2: the step's two model calls, K1 / K2 grid rows; K2 = 0 for one) against the padded input grids B1 / B2
 * shifted by each tap's row offset (negative offsets reach into the guard rows in front of the grid).
 * Reference: the nine (ky, kx) slices of Conv2d.weight.grad, torch's conv2d backward (deepinv SwinIR's 3x3 convs). */
int sei_gemm_bf16nt_dw2_taps(const uint16_t *A1, const uint16_t *A2, int lda, const uint16_t *B1, const uint16_t *B2,
                             int ldb, float *D32, int M, int N, int K1, int K2, int accumulate, int ntaps,
                             const int *tap_rows, long long tap_ld, void *stream);

int sei_gemm_bf16nt_dw2_bf16out(const uint16_t *A1, const uint16_t *A2, int lda, const uint16_t *B1, const uint16_t *B2,
                                int ldb, uint16_t *D16, int M, int N, int K1, int K2, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Token-streaming GEMMs for layer-sized weights (token_gemm.hip; ABI 6): the linear layers of the reference's default
 * backbone, deepinv's SwinIR as built by src/models/__init__.py:51-74 (qkv / proj / fc1 / fc2 of every block:
 * nn.Linear forward, its data gradient and its weight gradient in torch's autograd), in the bf16 throughput mode.
 * One persistent workgroup per CU streams its share of the tokens once; the weight (gradient) stays in registers.
 *
 * sei_tokgrad_bf16: D (Mo, Ni; row stride ldd) += Y^T X over K1 + K2 tokens; Y1 / Y2: (K, ldy >= Mo), X1 / X2:
 * (K, ldx >= Ni) bf16, token-major as the layers store them; the two segments are the step's two model calls (K2 = 0:
 * one). Float atomics: D must hold the running gradient (or zeros). Eligible (sei_tokgrad_bf16_eligible != 0): Mo and Ni
 * multiples of 192 with at most eight 192 x 192 blocks (sei_tokgrad_bf16_blocks: sixteen), K1 and K2 multiples of 64, ldy and ldx multiples of 8, 16-byte
 * aligned operands. Same product as sei_gemm_bf16nt_dw2(..., accumulate = 1) up to the float summation order. */
#define SEI_TOKGRAD_MAX_BLOCKS 16
typedef struct SeiTokGradBlock {     /* one 192 x 192 block of a weight gradient: D += Y[:, y0:y0+192]^T X[:, x0:x0+192] */
    const uint16_t *Y1, *Y2;         /* (K1, ldy) / (K2, ldy) bf16; Y2 unused when K2 = 0 */
    const uint16_t *X1, *X2;         /* (K1, ldx) / (K2, ldx) */
    int ldy, ldx, y0, x0;            /* multiples of 8; y0 + 192 <= ldy, x0 + 192 <= ldx */
    float *D;                        /* the block's first element; row stride ldd >= 192 */
    int ldd;
} SeiTokGradBlock;
/* Up to eight blocks in ONE launch over the same K1 + K2 tokens (all four weight gradients of a Swin block = 3 + 1 + 2 + 2
 * blocks): the CUs are shared out between the blocks, so every workgroup walks nblocks times as many tokens and the
 * float atomics per output (one partial block per workgroup) shrink by the same factor. */
int sei_tokgrad_bf16_blocks(const SeiTokGradBlock *blocks, int nblocks, long long K1, long long K2, void *stream);
int sei_tokgrad_bf16(const uint16_t *Y1, const uint16_t *Y2, int ldy, const uint16_t *X1, const uint16_t *X2, int ldx,
                     float *D, int ldd, int Mo, int Ni, long long K1, long long K2, void *stream);
size_t sei_tokgrad_bf16_eligible(int Mo, int Ni, int ldy, int ldx, long long K1, long long K2);

/* Streamed weight gradients of the U-Net's shallow levels (csrc/dw_stream.hip): D (Mo, ldd >= Ni) += Y^T X over K1 + K2
 * pixels for every job of a table in ONE launch per block shape -- persistent workgroups that own a whole block of a gradient
 * in their accumulators and stream a contiguous pixel range once (LDS-DMA ring), dealt to the jobs in proportion to their
 * bytes. Replaces torch's conv2d weight gradient of the 1x1 convolutions of /root/reference/src/models/convolutional.py:40-42
 * (ConvBlock.conv2 / conv3), :106 (Upsample) and :143 (Downsample) where (Mo, Ni) is (128, 256 k) / (256 k, 128), k <= 4,
 * with K1, K2 multiples of 64, or (32, 128) / (128, 32) with K1, K2 multiples of 128; sei_dwstream_bf16_eligible() != 0
 * says so, sei_gemm_bf16nt_dw2 serves everything else. Y (K, ldy == Mo) and X (K, ldx == Ni) are bf16, pixel-major as
 * stored, in two row segments (the step's two model calls; K2 = 0: one). D is ADDED to with float atomics; so is gbias
 * (the bias gradient = the column sums of Y, from one more MFMA per fragment against a fragment of ones). */
#define SEI_DWSTREAM_MAX_JOBS 64
typedef struct SeiDwStreamJob {
    const uint16_t *Y1, *Y2;         /* (K1, ldy) / (K2, ldy) bf16; Y2 unused when K2 = 0 */
    const uint16_t *X1, *X2;         /* (K1, ldx) / (K2, ldx) */
    int ldy, ldx, Mo, Ni;
    float *D;
    int ldd, reserved;
    long long K1, K2;
    float *gbias;                    /* NULL, or (Mo): += the column sums of Y over all K1 + K2 pixels (the convolution's bias gradient) */
} SeiDwStreamJob;
int sei_dwstream_bf16_jobs(const SeiDwStreamJob *jobs, int njobs, void *stream);
size_t sei_dwstream_bf16_eligible(int Mo, int Ni, int ldy, int ldx, long long K1, long long K2);

/* sei_rowgemm_bf16: D (M, N) = epilogue(A W^T): A (M, lda >= K) bf16 rows, W (N, ldw >= K) bf16 -- the layer's matrix as
 * nn.Linear stores it (forward) or its transpose (data gradient), zero-padded to N in {192, 384, 576} rows and
 * K in {192, 384, 576} columns -- with the SEI_EPI_* epilogues of sei_gemm_bf16nt:
 *   SEI_EPI_BIAS            D16 = bf16(acc + bias)                                   (N 576, K 192: qkv)
 *   SEI_EPI_BIAS_RES        D32 = acc + bias + R1                                     (N 192, K 192 / 384: proj, fc2)
 *   SEI_EPI_BIAS_SCALE_RES  D32 = R2 + R1[row] (acc + bias)    (stochastic depth)     (the same two)
 *   SEI_EPI_BIAS_GELU       D32 = acc + bias (optional: may be NULL), D16 = bf16(gelu(acc + bias))   (N 384, K 192: fc1; nv = N)
 *   SEI_EPI_MUL_DGELU       D16 = bf16(acc gelu'(R1))                                 (N 384, K 192: fc2's data gradient)
 *   SEI_EPI_NONE            D16 = bf16(acc) (N 192, K 192)  or  D32 = acc (N 192, K 384 / 576)   (the other data gradients)
 * nv (a multiple of 4, <= N): valid columns of the float32 output, of bias and of the row-shaped R (ldr >= nv); bf16
 * outputs always receive all N columns (ld16 >= N; zeros where W's padding rows are zero). M a multiple of 64.
 * sei_rowgemm_bf16_eligible(M, N, K, epilogue, out16) != 0 says whether a combination is built; the caller takes
 * sei_gemm_bf16nt otherwise (same results up to the float summation order). */
int sei_rowgemm_bf16(const uint16_t *A, int lda, const uint16_t *W, int ldw, float *D32, int ld32, uint16_t *D16,
                     int ld16, long long M, int N, int K, int nv, int epilogue, const float *bias, const float *R1,
                     const float *R2, int ldr, void *stream);
size_t sei_rowgemm_bf16_eligible(long long M, int N, int K, int epilogue, int out16);

/* The data gradient of a linear layer that follows a LayerNorm, with the LayerNorm's backward in the epilogue (the
 * product never leaves the chip): gh = A W^T (A: (M, lda >= K) bf16; W: (192, ldw >= K) bf16, rows >= C zero; K 384 or
 * 576), then torch's native_layer_norm_backward over the C channels of every row plus the residual gradient:
 *   gx = rstd (gh gamma - mean_c(gh gamma) - xhat mean_c(gh gamma xhat)) + res,   xhat = (x - mean) rstd;
 *   ggamma += sum_rows gh xhat,  gbeta += sum_rows gh;
 * and, when y16 is given, the operand of the next weight / data gradient in the same pass:
 *   y16 (M, ldy >= 192; zeros past C) = bf16(gx row_scale[row]),  colsum += sum_rows gx row_scale[row]
 * (colsum: K = 384 only and optional -- at K = 576 no registers are left for the third column sum; the bias gradient it
 * would be then comes out of the weight gradient through sei_rowgemm_gelu_bf16's ones column).
 * x, res, gx: (M, C) float32 rows; mean, rstd, row_scale: M floats. work: sei_rowgemm_lnbwd_work_floats(C) floats (per-
 * workgroup column sums, folded by a second launch; ggamma = gbeta = NULL leaves that fold to sei_fold_many: the sums
 * stay in `work`, [min(M / 32, 256)][3][C] = for ggamma | gbeta | colsum). Replaces sei_gemm_bf16nt + sei_ln_bwd_pad (+ sei_cast_pad_bf16):
 * deepinv SwinIR's norm1 / norm2 in front of qkv / fc1 (reference construction: src/models/__init__.py:51-74). */
int sei_rowgemm_lnbwd_bf16(const uint16_t *A, int lda, const uint16_t *W, int ldw, long long M, int K, const float *x,
                           const float *gamma, const float *mean, const float *rstd, const float *res, float *gx, int C,
                           float *ggamma, float *gbeta, const float *row_scale, uint16_t *y16, int ldy, float *colsum,
                           float *work, size_t work_floats, void *stream);
size_t sei_rowgemm_lnbwd_bf16_eligible(long long M, int K, int C);
size_t sei_rowgemm_lnbwd_work_floats(int C);

/* fc2's data gradient through GELU with the GELU' input RECOMPUTED instead of stored: D16 (M, ld16 >= N) =
 * bf16((A W^T) * gelu'(A2 W2^T + bias2)), A = the gradient rows (M, lda >= K), W = fc2's matrix transposed (N, K);
 * A2 = fc1's input rows (M, lda2 >= K), W2 = fc1's matrix (N, K), bias2 its bias (nv entries) -- the second product is
 * the forward pass's pre-activation, bit for bit (same MFMA order as sei_rowgemm_bf16 with SEI_EPI_BIAS_GELU), so the
 * forward pass need not write it (D32 = NULL there) nor this pass read it: 1536 of the 2688 bytes per token of either
 * kernel. N = 384, K = 192 (deepinv SwinIR's Mlp: nn.Linear(180, 360) -> nn.GELU -> nn.Linear(360, 180), zero-padded).
 * Same result as sei_rowgemm_bf16(SEI_EPI_MUL_DGELU) on the stored pre-activation. */
int sei_rowgemm_dgelu_bf16(const uint16_t *A, int lda, const uint16_t *W, int ldw, const uint16_t *A2, int lda2,
                           const uint16_t *W2, int ldw2, const float *bias2, int nv, uint16_t *D16, int ld16, long long M,
                           int N, int K, void *stream);
size_t sei_rowgemm_dgelu_bf16_eligible(long long M, int N, int K);

/* A residual linear layer followed by a LayerNorm, in one launch: out (M, C) = res + [row_scale[row]] (A W^T + bias)
 * (SEI_EPI_BIAS_RES, or SEI_EPI_BIAS_SCALE_RES when row_scale is given: timm's DropPath) and, since a workgroup holds
 * whole rows of out, nn.LayerNorm(C, eps) of them: h16 (M, ldh >= 192) = bf16((out - mean) rstd gamma + beta), padding
 * columns zero except column C = 1.0 when ones_col (see sei_ln_fwd_bf16_pad), mean / rstd (M floats each) for the
 * backward. A (M, lda >= K) bf16, W (192, ldw >= K) bf16 with zero rows past C, K 192 or 384: deepinv SwinIR's
 * proj -> norm2 and fc2 -> the next block's norm1. Same values as sei_rowgemm_bf16 + sei_ln_fwd_bf16_pad (the LayerNorm
 * sums run over 16 lanes instead of 64: last-bit differences in mean / rstd). */
int sei_rowgemm_ln_bf16(const uint16_t *A, int lda, const uint16_t *W, int ldw, long long M, int K, int C, const float *bias,
                        const float *row_scale, const float *res, float *out, const float *gamma, const float *beta,
                        float eps, int ones_col, uint16_t *h16, int ldh, float *mean, float *rstd, void *stream);
size_t sei_rowgemm_ln_bf16_eligible(long long M, int K, int C);

/* fc1's forward alone (bf16 gelu output only, the float32 pre-activation is recomputed by sei_rowgemm_dgelu_bf16), with
 * column one_at of D16 written as 1.0 (-1: none): the weight gradient of the layer behind, D16^T-contracted over the tokens,
 * then carries that layer's BIAS gradient in column one_at (the qkv / fc1 trick of sei_ln_fwd_bf16_pad's ones_col, for
 * fc2). bias: all N entries (zeros in the padding). Same values as sei_rowgemm_bf16(SEI_EPI_BIAS_GELU, D32 = NULL). */
int sei_rowgemm_gelu_bf16(const uint16_t *A, int lda, const uint16_t *W, int ldw, const float *bias, int nv, uint16_t *D16,
                          int ld16, long long M, int N, int K, int one_at, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The DRUNet denoiser of the PlugAndPlay baseline (reference src/models/pnp.py -> deepinv's DRUNet, restated in
 * models/drunet.py): bias-free 3x3 convolutions at 64 / 128 / 256 / 512 channels (anything else: SEI_ERR_BAD_ARG), bf16
 * MFMA with float32 accumulation. Activations are bf16 channels-last on zero-bordered grids (B, H + 2, W + 2, C) with
 * W + 3 guard rows of C elements in front and behind (sei_pad_nhwc_bf16's layout); every grid pointer below is ROW 0 of
 * its grid (behind the guard rows). The residual trunk T is float32 with the same row indexing (no guard rows needed).
 * Weights are bf16, tap-major and K-contiguous: (N, taps * Cin), tap t = ky * kw + kx. Only interior rows are written:
 * the border of an output grid stays as the caller zeroed it, guard rows are read but never written and never reach a
 * result. No split-K, no atomics: the same bits on every run and at every position in the batch. Pointers 16-byte
 * aligned (x and the image of the tail: 4).
 *   sei_drunet_conv3x3  epilogue 0: Y16 = bf16(relu(conv(X))) (T_* NULL) -- ResBlock conv 1;
 *                       epilogue 1: T_out = T_in + conv(X) [+ T_skip], Y16 = bf16(T_out) -- ResBlock conv 2; T_out may be
 *                       T_in. T_skip is the U-Net skip added ahead of an up block (or of the tail).
 *   sei_drunet_down     nn.Conv2d(Cin, Cout, 2, 2): X is the (2 Ho, 2 Wo) grid, T_out / Y16 the (Ho, Wo) ones.
 *   sei_drunet_up       nn.ConvTranspose2d(Cin, Cout, 2, 2) in one launch: Wt (4 Cout, Cin), row (ky * 2 + kx) Cout + co;
 *                       X is the (H, W) grid, T_out / Y16 the (2 H, 2 W) ones.
 *   sei_drunet_head     conv3x3(cat(x, sigma)) for x (B, 3, H, W) float32 NCHW: Wt (Cout, 9 * 32), the four input channels
 *                       zero-padded to 32 (the constant channel is zero outside the image, so it is no bias); T_out and
 *                       Y16 = bf16(T_out). work: sei_drunet_work_bytes(B, H, W) bytes (0 = arguments refused).
 *   sei_drunet_tail     out (B, 3, H, W) float32 NCHW = conv3x3(X), Wt (16, 9 * Cin) with zero rows behind the third. */
size_t sei_drunet_work_bytes(int B, int H, int W);
int sei_drunet_conv3x3(const uint16_t *X, const uint16_t *Wt, int Cin, int Cout, int B, int H, int W, int epilogue,
                       const float *T_in, const float *T_skip, float *T_out, uint16_t *Y16, void *stream);
/* sei_drunet_conv3x3 with the tile chosen by the caller: a wave takes 16 pb grid rows x 64 channels, pb 1, 2 or 4, 0 = the
 * default (by the number of waves the launch has); anything else is SEI_ERR_BAD_ARG. Same bits for every pb. */
int sei_drunet_conv3x3_ex(const uint16_t *X, const uint16_t *Wt, int Cin, int Cout, int B, int H, int W, int epilogue,
                          const float *T_in, const float *T_skip, float *T_out, uint16_t *Y16, int pb, void *stream);
int sei_drunet_down(const uint16_t *X, const uint16_t *Wt, int Cin, int Cout, int B, int Ho, int Wo, float *T_out,
                    uint16_t *Y16, void *stream);
int sei_drunet_up(const uint16_t *X, const uint16_t *Wt, int Cin, int Cout, int B, int H, int W, float *T_out,
                  uint16_t *Y16, void *stream);
int sei_drunet_head(const float *x, float sigma, const uint16_t *Wt, int Cout, int B, int H, int W, float *T_out,
                    uint16_t *Y16, void *work, void *stream);
int sei_drunet_tail(const uint16_t *X, const uint16_t *Wt, int Cin, int B, int H, int W, float *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The DiffPIR baseline around that denoiser (models/diffpir.py, models/_cg.py; deepinv v0.2.0's sampling.DiffPIR and
 * optim.utils.conjugate_gradient restated): the data step's conjugate gradients with every scalar on the device, and the
 * sampling step. float32 streaming kernels over flat tensors of n >= 1 elements (16-byte lanes, a scalar tail); tensor
 * pointers 16-byte aligned. Each reduction leaves one partial per workgroup in `part` (sei_cg_partials(n) floats: the
 * launch shape depends on n only) and a one-workgroup fold in the library's fold order writes the scalar into the state:
 * no atomics, the same bits on every run. -ffp-contract=off: the expressions below are the float32 operations made.
 *
 * The solve is (A^T A + inv_gamma I) u = A^T y + inv_gamma u0 from u = 0, with deepinv's recurrences:
 *   sei_cg_init       b = Aty + u0 * inv_gamma;  x = 0;  r = p = b;  state.rs = r . r;  done = iterations = 0.
 *                     prologue = 1: u0 is first replaced by clamp(2 u0 - 1, -1, 1) / 2 + 0.5 (DiffPIR hands the denoiser's
 *                     output over); 0: taken as it is.
 *   [the caller's own kernels: AtAp = A^T A p]
 *   sei_cg_apply      Ap = AtAp + p * inv_gamma;  state.pAp = p . Ap.
 *   sei_cg_update     alpha = rs / pAp;  x += alpha p;  r -= alpha Ap;  state.rs_new = r . r;  iterations += 1;
 *                     done = 1 when sqrt(rs_new) < tol (tol = 0: never); otherwise state.beta = rs_new / rs and then
 *                     rs = rs_new (the fold behind the reduction is the one writer of the state and holds both values;
 *                     the many workgroups of sei_cg_direction could not overwrite an rs they still read).
 *   sei_cg_direction  p = r + p * beta, beta = rs_new / rs as sei_cg_update left it. Writes no state.
 * Once done is set, _apply, _update and _direction return without writing anything: x is what deepinv's `break` leaves,
 * updated by the stopping iteration, with p not advanced, however many further iterations the host has enqueued. The
 * host reads done and iterations when it chooses to (models/_cg.py: every few iterations); nothing else of the solve
 * leaves the device. */
typedef struct SeiCgState {
    float rs, pAp, rs_new;
    int done, iterations;
    float beta;           /* rs_new / rs of the last sei_cg_update, for sei_cg_direction */
    int reserved[2];
} SeiCgState;
size_t sei_cg_partials(size_t n);
int sei_cg_init(const float *u0, const float *Aty, float inv_gamma, int prologue, float *x, float *r, float *p, float *part,
                SeiCgState *state, size_t n, void *stream);
int sei_cg_apply(const float *p, const float *AtAp, float inv_gamma, float *Ap, float *part, SeiCgState *state, size_t n,
                 void *stream);
int sei_cg_update(float *x, float *r, const float *p, const float *Ap, float tol, float *part, SeiCgState *state, size_t n,
                  void *stream);
int sei_cg_direction(float *p, const float *r, const SeiCgState *state, size_t n, void *stream);
/* One DiffPIR sampling step in one pass, from the prox result u (in [0, 1] scale) and the current iterate x:
 *   x0 = 2 u - 1;  eps = (x - sa_t x0) / s1m_t;  x = sa_n x0 + s1m_n (sqrt(1 - zeta) eps + sqrt(zeta) nz)   (in place)
 *   xin = x / (2 sqrt(at_n)) + 0.5                                                        (the next denoiser input)
 * sa_* / s1m_* are sqrt(alphas_cumprod) / sqrt(1 - alphas_cumprod) at the current (t) and next (n) timestep, at_n the
 * next alphas_cumprod; the three square roots are taken once on the host. u, nz, xin must not overlap x. */
int sei_diffpir_sample(const float *u, float *x, const float *nz, float *xin, float sa_t, float s1m_t, float sa_n,
                       float s1m_n, float zeta, float at_n, size_t n, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The DPS baseline (models/dps.py; deepinv v0.2.0's sampling.DPS restated): every step differentiates the data term
 * through the denoiser, so the DRUNet family above gains the one launch its backward pass lacks, and the step itself runs
 * on float32 streaming kernels with every scalar on the device.
 *
 *   sei_drunet_conv3x3_masked   Y16 = bf16(conv(X)) where the bf16 grid Mask (the output's shape) is above zero, else 0:
 *                               the first half of a ResBlock's backward, Mask the taped ReLU output of its first
 *                               convolution and Wt the transposed weights of its second. Tiles, the interior-rows rule and
 *                               the bits-per-pb promise are sei_drunet_conv3x3's; Mask may not be Y16. (The transposed
 *                               operators are the forward's shapes with repacked weights: a 3x3 convolution with flipped
 *                               taps, down^T on sei_drunet_up, up^T on sei_drunet_down, tail^T on sei_drunet_head with
 *                               sigma = 0, head^T on sei_drunet_tail; the block's second half is epilogue 1.) */
int sei_drunet_conv3x3_masked(const uint16_t *X, const uint16_t *Wt, int Cin, int Cout, int B, int H, int W,
                              const uint16_t *Mask, uint16_t *Y16, void *stream);
int sei_drunet_conv3x3_masked_ex(const uint16_t *X, const uint16_t *Wt, int Cin, int Cout, int B, int H, int W,
                                 const uint16_t *Mask, uint16_t *Y16, int pb, void *stream);
/* The step kernels stream B images of m >= 1 floats each (B m contiguous floats; tensor pointers 16-byte aligned, the
 * per-image scalars 4; an image's start need not be aligned). -ffp-contract=off: the float32 operations as written.
 *   sei_dps_u         u = clamp(2 out - 1, -1, 1) / 2 + 0.5.
 *   sei_dps_residual  r = Au - y; f[b] = 0.5 ||r_b||^2; s[b] = 1 / (2 sqrt(f[b])), 0 where f[b] is not above 0. One partial
 *                     per workgroup in part (sei_dps_partials(B, m) floats, 0 = arguments refused) and a one-workgroup
 *                     fold in the library's fold order: no atomics, the same bits on every run and at every batch position.
 *   sei_dps_seed      seed = Atr where -1 <= 2 out - 1 <= 1 (the clamp's derivative, inclusive), else 0.
 *   sei_dps_step      x0 = clamp(2 out - 1, -1, 1);  x = ((c0 x0 + st nz) + c1 x) - (ginv s[b]) gx   (in place);
 *                     xin = x / den + 0.5 (den = 2 sqrt(alpha) of the next timestep; 2 behind the last pair, where xin is
 *                     the result). out, gx, nz and xin must not be x. */
size_t sei_dps_partials(int B, size_t m);
int sei_dps_u(const float *out, float *u, int B, size_t m, void *stream);
int sei_dps_residual(const float *Au, const float *y, float *r, float *part, float *f, float *s, int B, size_t m,
                     void *stream);
int sei_dps_seed(const float *Atr, const float *out, float *seed, int B, size_t m, void *stream);
int sei_dps_step(const float *out, const float *gx, const float *nz, const float *s, float *x, float *xin, float c0, float c1,
                 float st, float ginv, float den, int B, size_t m, void *stream);

/* ---- the BM3D baseline (models/bm3d.py; csrc/bm3d_kernels.hip). Reference: src/models/bm3d_deblurring.py calls the bm3d
 * package, which is not part of the reference tree: the algorithm is restated in models/bm3d.py and pinned by
 * tests/bm3d_ref.py. `planes` images of H x W float32 (H, W >= 8), blocks of 8 x 8. The reference positions of an axis of
 * extent m are 0, step, 2 step ... and m - 8 last; sei_bm3d_ref_blocks(H, W, step) is their number per plane (0 = arguments
 * refused), row-major over (row position, column position). Groups: pos[planes][ref blocks][n_max][2] int32 (row, column of a
 * block's first pixel) and counts[planes][ref blocks] int32, n_max one of 1, 2, 4, 8, 16, 32; window odd.
 *   sei_bm3d_match   per reference block at (r, c): d = sum(diff^2) / 64 against every block position (r', c') of the image
 *                    with |r' - r|, |c' - c| <= window / 2; the n_max smallest with d <= tau in the order (d, r', c'), cut to
 *                    the largest power of two not above their number. Slots behind the count hold (r, c). dist (may be
 *                    NULL): [planes][ref blocks][n_max] the kept distances, +inf behind the count. The same bits on every run.
 *   sei_bm3d_ht      8 x 8 DCT-II and Haar along the group, coefficients kept where |c| > lambd sqrt(var[plane][i]), group
 *                    weight 1 / (sum of var over the kept; 1 when none), inverse, and work[0] += w K block, work[1] += w K
 *                    (work: 2 x planes H W floats, zeroed by the call; K = kaiser(8, 2.0) x kaiser(8, 2.0)). coef (may be
 *                    NULL): [planes][ref blocks][n_max][64] doubles, the group's transform coefficients before the shrinkage.
 *                    Its transforms and its keep / drop decisions are in double (lambd is a double): they agree with a
 *                    float64 computation on the same float32 inputs except at ties of about 1e-15.
 *   sei_bm3d_wiener  the same with the shrinkage P^2 / (P^2 + var) from the pilot's group at the same positions and the
 *                    weight 1 / sum(W^2 var).
 *                    Both clamp positions to [0, H-8] x [0, W-8] and counts to a power of two in [1, n_max]: no index buffer
 *                    makes them touch memory outside the planes. agg: 0 sums a tile's blocks in LDS before the global float
 *                    atomics, 1 adds every block row to global memory; either way the result is reproducible to rounding
 *                    only. var: [planes][64].
 *   sei_bm3d_finish  out = work[0] / work[1] (0 where work[1] is 0).
 * SEI_ERR_BAD_ARG on NULL or misaligned pointers, planes < 1, H or W below 8, step < 1, an even or non-positive window, an
 * n_max outside the list, a negative or non-finite tau / lambd, agg outside {0, 1}; SEI_ERR_TOO_LARGE when the search region
 * or the tile's footprint does not fit 64 KiB of LDS, or the index arithmetic would overflow. */
size_t sei_bm3d_ref_blocks(int H, int W, int step);
int sei_bm3d_match(const float *img, int planes, int H, int W, int step, int window, float tau, int n_max, int *pos,
                   int *counts, float *dist, void *stream);
int sei_bm3d_ht(const float *noisy, const float *var, const int *pos, const int *counts, int planes, int H, int W, int step,
                int n_max, int window, double lambd, int agg, float *work, double *coef, void *stream);
int sei_bm3d_wiener(const float *noisy, const float *pilot, const float *var, const int *pos, const int *counts, int planes,
                    int H, int W, int step, int n_max, int window, int agg, float *work, void *stream);
int sei_bm3d_finish(const float *work, float *out, int planes, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The diffusion U-Net of the DiffPIR_DiffUNet baseline (models/diffunet.py; csrc/adm_kernels.hip): guided-diffusion's
 * "ADM" network as deepinv's DiffUNet(large_model=False) builds it, restated in models/diffunet.py and pinned by
 * tests/diffunet_ref.py. The layout is the DRUNet family's: float32 rows (R, C) on the row indexing of the zero-bordered
 * grid (B, H + 2, W + 2), R = B (H + 2) (W + 2); bf16 grids of the same rows with W + 3 guard rows in front and behind,
 * every grid pointer ROW 0 of its grid; bf16 weights (N, taps * Cin), tap t = 3 ky + kx. Only interior rows are read and
 * written (sei_adm_pack_image writes its whole grid): the border of a bf16 grid stays as the caller zeroed it, guard rows
 * are read by the 3x3 convolution but never written and never reach a result. No split-K and no atomics anywhere: the same
 * bits on every run and at every batch position. Pointers 16-byte aligned (statistics and NCHW images: 4).
 * An input "Xa | Xb" is the channel concatenation of two float32 buffers of Ca and Cb channels (Xb NULL with Cb = 0);
 * Ca, Cb multiples of 4, Ca + Cb a multiple of 128: 32 groups of a multiple of 4 channels, which may straddle the seam.
 *   sei_adm_gn_stats    stats[b][g] = (mean, 1 / sqrt(var + eps)) of group g of image b, biased variance, two passes in
 *                       float32 (a first mean m0, then the distances d from it: mean = m0 + E[d], M2 = sum d^2 - n E[d]^2)
 *                       per slice of 1024 pixels, one workgroup per (b, g, slice); above one slice a second launch
 *                       merges the slices' (mean, M2) from `part` in a fixed order. part: B sei_adm_gn_part_floats(H, W)
 *                       floats (0 = extents refused); the launch shape depends on the extents only.
 *   sei_adm_gn_apply    v = SiLU(((x - mean) rstd gamma + beta) [* (1 + mod[b][c]) + mod[b][C + c]]) with mod (B, 2 C) or
 *                       NULL; silu 0 leaves the SiLU out (attention's norm); stats NULL (then gamma, beta, mod NULL):
 *                       v = x. resample 0: written at the input's extents; 1: the 2x2 average of v into the (H / 2, W / 2) grid (H, W even); 2: v repeated 2x into the
 *                       (2 H, 2 W) grid. Y16 (a bf16 grid) and / or Y32 (float32 rows) of the OUTPUT's extents; H, W are
 *                       the input's.
 *   sei_adm_pack_image  x (B, 3, H, W) float32 NCHW -> the head's bf16 grid of 32 channels (x, zeros), borders zero.
 *   sei_adm_conv        v = (conv(X) + bias) [+ T_res]; T_out = v and / or Y16 = bf16(v), at least one. ntaps 9 (3x3, zero
 *                       padding 1) or 1 (1x1); Cin a multiple of 32, Cout of 64. T_out may be T_res.
 *   sei_adm_tail        out (B, 3, H, W) float32 NCHW = conv3x3(X) + bias: Wt (16, 9 Cin) and bias (16) with zeros behind
 *                       the third row / entry.
 *   sei_adm_attention   QKV16 bf16 rows (R, 3 C): head h of C / 64 owns channels [192 h, 192 h + 64) as q, the next 64 as
 *                       k, the next 64 as v. A16 (R, C) bf16, channels [64 h, 64 h + 64) = softmax_s((q_t . k_s) / 8) v_s
 *                       over the T = H W interior rows of the image: bf16 MFMA products, the row maximum subtracted, the
 *                       running maximum and sum in float32, the probabilities rounded to bf16 ahead of the second product.
 *                       Any T >= 1. */
size_t sei_adm_gn_part_floats(int H, int W);
int sei_adm_gn_stats(const float *Xa, int Ca, const float *Xb, int Cb, int B, int H, int W, float eps, float *stats,
                     float *part, void *stream);
int sei_adm_gn_apply(const float *Xa, int Ca, const float *Xb, int Cb, const float *stats, const float *gamma,
                     const float *beta, const float *mod, int silu, int B, int H, int W, int resample, uint16_t *Y16,
                     float *Y32, void *stream);
int sei_adm_pack_image(const float *x, uint16_t *G16, int B, int H, int W, void *stream);
int sei_adm_conv(const uint16_t *X, const uint16_t *Wt, const float *bias, int Cin, int Cout, int ntaps, int B, int H, int W,
                 const float *T_res, float *T_out, uint16_t *Y16, void *stream);
int sei_adm_tail(const uint16_t *X, const uint16_t *Wt, const float *bias, int Cin, int B, int H, int W, float *out,
                 void *stream);
int sei_adm_attention(const uint16_t *QKV16, int C, int B, int H, int W, uint16_t *A16, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SEI_HIP_H */
