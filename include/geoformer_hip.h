/* geoformer_hip.h - C ABI of libgeoformer_hip.so (MI355X / gfx950).
 *
 * The reference (ruc-aimc-lab/GeoFormer) is pure Python on torch and has no FFI of its own; the
 * path this library replaces sits behind torch.nn.Module.forward() calls.  Each entry point below
 * replaces the sequence of ATen ops of ONE reference function (cited as file:line, relative to the
 * reference checkout) and is what a ctypes binding inside that function would call
 * (see INTEGRATION.md).
 *
 * Conventions
 *   - plain pointers + sizes; all pointers are DEVICE pointers unless a name ends in _host;
 *   - the caller allocates and owns every buffer, including the workspace
 *     (size from the matching gf_*_workspace_bytes query);
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*), never
 *     synchronises, never allocates; safe to capture in a hipGraph;
 *   - returns 0 (GF_OK) or a negative gf_status; gf_last_error() gives the message;
 *   - dtype: GF_F32 (parity mode, exact-fp32 MFMA), GF_F16 or GF_BF16 (16-bit storage, fp32 accumulate);
 *   - data-dependent sizes (match counts) are produced in device memory; entry points that
 *     consume them read them from device memory too, so no host round trip is forced.
 */
#ifndef GEOFORMER_HIP_H_
#define GEOFORMER_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { GF_OK = 0, GF_ERR_INVALID_ARGUMENT = -1, GF_ERR_WORKSPACE = -2, GF_ERR_LAUNCH = -3 } gf_status;
typedef enum { GF_F32 = 0, GF_F16 = 1, GF_BF16 = 2 } gf_dtype;

/* Bumped whenever an existing entry point changes its signature or its defaults; a binding compares gf_abi_version() with the
 * GF_ABI_VERSION of the header it was written against at load time (geoformer_amd/_lib.py does) instead of calling shifted
 * arguments.  History: 1 = rounds 1-2; 2 = round 3 (gf_ransac_homography had gained `lm_iters` in the MIDDLE of its list: a
 * caller built against version 1 would have passed min_points as lm_iters); 3 = round 4: gf_ransac_homography is back to its
 * version-1 signature (no refinement), new arguments live in gf_ransac_homography_v2, appended at the END. */
/* 4 (round 4): the fragment stream of gf_conv3x3_nhwc deals the output channels differently (fused.py:pack_conv3x3_stream: a stream packed for
 * version 3 gives wrong channels) and GF_CONV_PAD16 now states that channels 196 .. 223 are padding; new: GF_CONV_S2, gf_lateral_upsample_add_nhwc. */
/* Still 4 with gf_pos_encode_ptrs / gf_fine_gather_ptrs and gf_pos_encode_ragged / gf_fine_gather_ragged (with gf_map_record): entries appended at
 * the end change no existing one; a binding that needs them fails at load on the missing symbol (geoformer_amd/_lib.py binds every name).
 * Likewise with the gf_keypoint_* entries, gf_fundamental_* (gf_fundamental_ransac_lo and its workspace query included), gf_linear_rows,
 * gf_index_rows, gf_fine_rows*, gf_abspose_* and gf_xyz_lookup (with gf_xyz_map), gf_track_link, gf_track_flatten and gf_triangulate*,
 * gf_covis_cluster, gf_sparse_rows and gf_covis_select, gf_bundle_workspace_bytes and gf_bundle_adjust, gf_bundle_pcg_workspace_bytes and gf_bundle_adjust_pcg,
 * gf_undistort_points and gf_distort_points, gf_relpose_* (four entries). */
#define GF_ABI_VERSION 4
int gf_abi_version(void);
const char* gf_last_error(void);

/* Optional per-kernel timing with HIP events on the launch stream (used by bench.py's `roofline`).
 * Tags: "k1_stats" (work = flops), "k1_conf" (work = algorithmic bytes), "k3_linear" (work = flops).
 * gf_linear_rows records under "k3_linear" too (with group_count it declares only the bytes that move whatever the counts are: weights + table).
 * gf_profile_collect synchronises on the recorded events and returns their summed time, count and work. */
void gf_profile_enable(int on);
void gf_profile_filter(const char* tag);   /* record only this tag (NULL: all): keeps the event count inside a timed region small */
int gf_profile_collect(const char* tag, double* total_ms, int* count, double* work);

/* ------------------------------------------------------------------------------------------
 * K1  dual-softmax correlation + mutual-nearest match extraction
 * replaces CoarseMatching.forward + get_coarse_match
 *          (model/loftr_src/loftr/utils/coarse_matching.py:90-130, :132-212)
 *
 *   sim  = <f0[n,i,:], f1[n,j,:]> / C / temperature       (-1e9 where !(mask0[n,i] & mask1[n,j]))
 *   conf = softmax(sim, dim=1) * softmax(sim, dim=2)       -> conf [N,L,S] fp32 (written unless conf == NULL, below)
 *   keep (n,i,j) iff conf > thr and conf is the maximum of its row and of its column; per row the
 *   first such column; rows emitted in (n,i) order, exactly like torch.where (:185-188).
 *   force_one != 0 reproduces the 'dataset_name' branch (:182-184): a sample without any match
 *   contributes (i=0, j=0).
 *
 *   f0 [N,L,C], f1 [N,S,C] of `dtype`, C a multiple of 64 (f16) / 32 (f32);
 *   mask0 [N,L], mask1 [N,S] uint8 (both NULL or both set);  scale0/scale1 [N,2] fp32 or NULL;
 *   w0c/w1c = coarse grid widths, scale = hw0_i[0]/hw0_c[0] (:193);
 *   outputs have capacity N*min(L,S) (+N when force_one): b/i/j_ids int64, mconf fp32,
 *   mkpts0_c/mkpts1_c [cap,2] fp32 (x,y);  counts int32[1+N]: total, then per sample.
 *
 *   MATCH-ONLY MODE (conf == NULL): the [N,L,S] matrix is not materialised - what inference.py:51-75 and
 *   eval_tool/immatch/modules/geoformer.py consume are the matches - and 2 x 164 MB of writes per 640x640 pair are
 *   saved; ids, mconf and keypoints are bit-identical to the contract mode's (entries the selection needs are
 *   recomputed with the sweep's own arithmetic).  Built for the configuration inference runs, see
 *   gf_dual_softmax_match_only_supported: 16-bit features, C = 256, L % 128 == 0, S % 64 == 0, no masks,
 *   force_one == 0; anything else with conf == NULL is GF_ERR_INVALID_ARGUMENT.
 *   gf_dual_softmax_conf_at returns single entries conf[b,i,j] afterwards (same features, the workspace of the
 *   last gf_dual_softmax_match call), bit-identical to what the contract mode writes.  gf_dual_softmax_match stamps
 *   the workspace with (N, L, S, C, temperature, f0, f1); conf_at compares the stamp with its own arguments ON THE
 *   DEVICE (no host synchronisation) and writes NaN for every entry if they differ, and for any b/i/j out of range.
 * ------------------------------------------------------------------------------------------ */
size_t gf_dual_softmax_workspace_bytes(int N, int L, int S);
int gf_dual_softmax_match_only_supported(int dtype, int L, int S, int C, int masked, int force_one);
int gf_dual_softmax_conf_at(const void* f0, const void* f1, int dtype, int N, int L, int S, int C, float temperature,
                            const int64_t* b, const int64_t* i, const int64_t* j, int P, float* out, void* workspace,
                            size_t workspace_bytes, void* stream);
int gf_dual_softmax_match(const void* f0, const void* f1, int dtype, int N, int L, int S, int C,
                          const uint8_t* mask0, const uint8_t* mask1, float temperature, float thr,
                          int force_one, int w0c, int w1c, float scale, const float* scale0,
                          const float* scale1, float* conf, int64_t* b_ids, int64_t* i_ids,
                          int64_t* j_ids, float* mconf, float* mkpts0_c, float* mkpts1_c,
                          int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K3 (training)  backward of the linear + LayerNorm / activation chain, mixed-16-bit step
 * what torch autograd derives for LoFTREncoderLayer.forward (model/loftr_src/loftr/loftr_module/transformer.py:45-60), the Geo
 *          layers (model/geo_transformer/transformer.py:49-66) and FinePreprocess' linears (fine_preprocess.py:61-72) when
 *          lightning/train_depth_geoformer.py:117-119 runs the step under 16-bit autocast; fp32 master weights / gradients.
 *   y = x W^T:   dX = dY W is gf_linear with the transposed weight;  dW = dY^T X is gf_linear_wgrad (fp32 [cout, cin], row
 *   stride lddw, optionally accumulated): the contraction runs over the T token rows of both operands (MFMA operands by
 *   transpose reads), split over token chunks, partials added in chunk order (deterministic).  cout, cin multiples of 8 (round 6; 128 before).
 *   gf_layernorm_forward keeps stats[t] = (mean, rstd); gf_layernorm_backward returns dy and dgamma / dbeta (fp32 [C],
 *   optionally accumulated); C in {128, 256, 512}.  gf_activation_backward: dz = dh * act'(z) from the OUTPUT h of the
 *   activation (kind 0 ReLU, 1 Tanh).  All activations GF_F16 or GF_BF16, statistics and parameter gradients fp32.
 * ------------------------------------------------------------------------------------------ */
size_t gf_linear_wgrad_workspace_bytes(long T, int cout, int cin);
int gf_linear_wgrad(const void* dy, long lddy, const void* x, long ldx, int dtype, long T, int cout, int cin, float* dw,
                    long lddw, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
int gf_layernorm_forward(const void* y, int dtype, long T, int C, const float* gamma, const float* beta, float eps, void* out,
                         float* stats, void* stream);
size_t gf_layernorm_backward_workspace_bytes(int C);
int gf_layernorm_backward(const void* dout, const void* y, const float* stats, int dtype, long T, int C, const float* gamma, void* dy,
                          float* dgamma, float* dbeta, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
int gf_activation_backward(const void* dh, const void* h, void* dz, size_t n, int kind, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * K2 (training)  backward of LinearAttention.forward (model/loftr_src/loftr/loftr_module/linear_attention.py:21-51), heads of 32
 *   given dout [N, L, H, 32]: dq [N, L, H*32], dk, dv [N, S, H*32] (contiguous) of out = phi(q) KV S / (phi(q) . Ksum + eps),
 *   KV = sum_s phi(k_s)^T (v_s / S), Ksum = sum_s phi(k_s), with the q / kv padding masks of :35-39.  q, k, v, dout: [N, L|S, H, 32]
 *   views with row strides in elements (GF_F16 / GF_BF16); fp32 arithmetic; the (image, head) states are sums of chunk partials
 *   in chunk order (deterministic).
 * ------------------------------------------------------------------------------------------ */
/* K8 (training): df0, df1 [M, 25, C] (`dtype`: GF_F32 / GF_F16 / GF_BF16) of FineMatching2.forward's confidence (model/fine_matching2.py:52-63:
 * sim = f0 f1^T / (C temperature), conf = softmax(sim, 1) * softmax(sim, 2)) given dconf fp32 [M, 25, 25]; fp32 arithmetic. */
int gf_fine_match_backward(const void* f0, const void* f1, int dtype, int M, int WW, int C, float temperature, const float* dconf,
                           void* df0, void* df1, void* stream);
size_t gf_linear_attention_backward_workspace_bytes(int N, int L, int S, int H);
int gf_linear_attention_backward(const void* q, const void* k, const void* v, const void* dout, int dtype, int N, int L, int S, int H,
                                 int D, long ldq, long ldk, long ldv, long ldo, const uint8_t* q_mask, const uint8_t* kv_mask, float eps,
                                 void* dq, void* dk, void* dv, void* workspace, size_t workspace_bytes, void* stream);
/* the same backward for the fine level's windows: q, k, v, dout, dq, dk, dv contiguous [Nw, Lw <= 32, 8 heads x 16] tensors, no masks
 * (the forward is gf_linear_attention's window form); one workgroup per window, fp32 arithmetic on the 16-bit operands. */
int gf_window_linear_attention_backward(const void* q, const void* k, const void* v, const void* dout, int dtype, int Nw, int Lw,
                                        float eps, void* dq, void* dk, void* dv, void* stream);

/* ------------------------------------------------------------------------------------------
 * K10 (training)  weight gradient of the backbone's 3x3 / stride 1 / pad 1 convolutions
 * replaces, for the training step, autograd's weight gradient of the BasicBlock / FPN-head convolutions
 *          (model/loftr_src/loftr/backbone/resnet_fpn.py:9-40,60-83; the library call is aten::convolution_backward, weights only).
 *   x  channels-last [N, H, W, cx], dy channels-last [N, H, W, cy] (GF_F16 / GF_BF16; cx, cy = STORED widths, multiples of 8 - the
 *   196-channel level is stored 224 wide), cin <= cx, cout <= cy the real widths;
 *   dw fp32 [cout][cin][3][3] (overwritten) = sum_n,y,x dy[n,y,x,co] * x[n, y+ky-1, x+kx-1, ci]; fp32 accumulation, partial sums
 *   per run of strip rows added in a fixed order (bit-reproducible).  workspace: gf_conv3x3_wgrad_workspace_bytes.
 * ------------------------------------------------------------------------------------------ */
size_t gf_conv3x3_wgrad_workspace_bytes(int N, int H, int W, int cin, int cout);
int gf_conv3x3_wgrad_nhwc(const void* x, const void* dy, int dtype, int N, int H, int W, int cx, int cy, int cin, int cout, float* dw,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K4 (training)  FullAttention.forward with saved softmax statistics, and its backward (flash form)
 * replaces, for the training step, model/geo_transformer/geo_attention.py:72-101 as GeoTransformer's 'self' branch calls it
 *          (model/geo_transformer/transformer.py:111-124: every cell of an image against the projected rows of its inlier cells,
 *          no masks) and the autograd backward through it.  Nothing of size L x S is stored.
 *   q [N, L, 4 x 64], k, v [N, S, 4 x 64]: row-strided views (ld* in elements, multiples of 8, 16-byte aligned rows; batch stride =
 *   rows x row stride), GF_F16 / GF_BF16; softmax_temp = 1 / sqrt(64) is applied to the fp32 logits (not folded into q).
 *   forward:  out [N, L, ldo] = softmax(q k^T softmax_temp) v, lse fp32 [N, 4, L] = log2 of the row's sum of exponentials (base 2,
 *             scaled logits: m + log2 l);  S == 0: out = 0.
 *   backward: dq [N, L, 256], dk, dv [N, S, 256] (contiguous, `dtype`) given out, dout [N, L, ld] and the forward's lse;
 *             P and dS are rounded to `dtype` for the second product of each pair, accumulation fp32, partial sums in a fixed
 *             order (bit-reproducible).  workspace: gf_full_attention_backward_workspace_bytes (the rows' dO . O).
 * ------------------------------------------------------------------------------------------ */
int gf_full_attention_train_forward(const void* q, const void* k, const void* v, int dtype, int N, int L, int S, int H, int D, long ldq,
                                    long ldk, long ldv, float softmax_temp, void* out, long ldo, float* lse, void* stream);
size_t gf_full_attention_backward_workspace_bytes(int N, int L, int H);
int gf_full_attention_backward(const void* q, const void* k, const void* v, const void* out, const void* dout, const float* lse,
                               int dtype, int N, int L, int S, int H, int D, long ldq, long ldk, long ldv, long ldo, long lddo,
                               float softmax_temp, void* dq, void* dk, void* dv, void* workspace, size_t workspace_bytes,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * K1 (training)  sparse-supervision focal loss on the dual-softmax confidence, forward and backward
 * replaces, for the training step, CoarseMatching.forward's conf_matrix (coarse_matching.py:113-125) as consumed by
 *          GeoLoss.compute_coarse_loss, focal / sparse_spvs / dual_softmax branch (loftr_loss.py:246-270), and the
 *          autograd backward through both.  Neither conf nor its gradient is materialised.
 *   f0 [N,L,256], f1 [N,S,256] (GF_F32 or GF_F16; the arithmetic is fp16 operands / fp32 accumulation),
 *   positives (pos_b, pos_i, pos_j)[P] = torch.where(conf_matrix_gt == 1), optional per-positive weight,
 *   optional padding masks uint8 [N,L] / [N,S] (pairs with a padded member: sim = -1e9, coarse_matching.py:123-124).
 *   forward:  pos_conf[k] = conf[b,i,j], pos_loss[k] = -alpha (1-p)^gamma log p * w  (p clamped to [1e-6, 1-1e-6]),
 *             pos_grad[k] = d pos_loss[k] / d log p.   loss_c = c_pos_w * mean_k pos_loss[k] is formed by the caller.
 *   backward: d_f0 [N,L,256], d_f1 [N,S,256] fp32 (overwritten) for  loss = scale * scale_dev[0] * sum_k pos_loss[k]
 *             (scale_dev: optional DEVICE scalar, NULL = 1; lets autograd hand the upstream gradient over without a
 *             host synchronisation);
 *             the workspace of the forward call must be passed unchanged (fp16 features and softmax statistics).
 *   L and S multiples of 128, C = 256.
 * ------------------------------------------------------------------------------------------ */
size_t gf_coarse_loss_workspace_bytes(int N, int L, int S);
int gf_coarse_loss_forward(const void* f0, const void* f1, int dtype, int N, int L, int S, int C, const uint8_t* mask0,
                           const uint8_t* mask1, float temperature, const int64_t* pos_b, const int64_t* pos_i, const int64_t* pos_j, int P,
                           const float* pos_weight, float alpha, float gamma, float* pos_conf, float* pos_loss,
                           float* pos_grad, void* workspace, size_t workspace_bytes, void* stream);
int gf_coarse_loss_backward(int N, int L, int S, int C, const uint8_t* mask0, const uint8_t* mask1, float temperature,
                            const int64_t* pos_b, const int64_t* pos_i,
                            const int64_t* pos_j, int P, const float* pos_grad, float scale, const float* scale_dev,
                            float* d_f0, float* d_f1, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * a1  position encoding add + flatten
 * replaces PositionEncodingSine.forward (model/loftr_src/loftr/utils/position_encoding.py:37-42)
 *          and the permute/reshape of model/full_model.py:69-77
 *   out[n, y*W+x, c] = x[n,c,y,x] + pe[y,x,c];  x viewed as [N,C,H,W] through element strides
 *   (NCHW or channels_last), pe fp32 [H,W,C] (host table built as position_encoding.py:22-35).
 *   x_dtype and out_dtype are independent: every pair of GF_F32 / GF_F16 / GF_BF16 is built (bf16 maps -> fp16 tokens is the
 *   'bf16_fp16' mode).  x is widened to fp32, the sum is rounded once to nearest even into out_dtype: the bits of torch's
 *   (x.float() + pe).to(out).  No clamp, no flush: a sum beyond fp16's range becomes +-inf.
 * ------------------------------------------------------------------------------------------ */
int gf_pos_encode(const void* x, int x_dtype, long sn, long sc, long sh, long sw, const float* pe,
                  void* out, int out_dtype, int N, int C, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------
 * K2  linear attention
 * replaces LinearAttention.forward (model/loftr_src/loftr/loftr_module/linear_attention.py:21-51)
 *   q [N,L,H,D], k,v [N,S,H,D] with row strides ldq/ldk/ldv (elements), masks uint8 or NULL,
 *   out [N,L,H*D] contiguous.  D in {16,32,64}, H*D in {64,128,192,256}.
 *   Rounding points in the 16-bit modes: the coarse shape (8 heads of 32) and the fine level's windows (8 heads of 16,
 *   L, S <= 32, 16-byte aligned rows) run on the matrix cores: phi(q), phi(k), KV / S and Ksum / S are rounded to the
 *   storage type, sums and the division are fp32 (oracle: linear_attention_fused / linear_attention_window); every other
 *   shape evaluates phi, the state and the normaliser in fp32 from the stored q, k, v.
 * ------------------------------------------------------------------------------------------ */
size_t gf_linear_attention_workspace_bytes(int N, int S, int H, int D);
int gf_linear_attention(const void* q, const void* k, const void* v, int dtype, int N, int L, int S, int H,
                        int D, long ldq, long ldk, long ldv, const uint8_t* q_mask, const uint8_t* kv_mask,
                        float eps, void* out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K9  the encoder layer in two launches (16-bit storage modes)
 * replaces LoFTREncoderLayer.forward as a whole (model/loftr_src/loftr/loftr_module/transformer.py:37-60 with
 *          LinearAttention.forward, linear_attention.py:21-51) and the part of the Geo layer after its attention
 *          (model/geo_transformer/transformer.py:56-66); d_model 256, 8 heads of 32 (linear attention).
 *   gf_encoder_kv_state: kv_state[n] = { KV[c][v] = sum_s phi(k)[s,c] v[s, head(c)*32 + v],  Ksum[c] = sum_s phi(k)[s,c] },
 *          k = W_k src, v = W_v src, phi = elu + 1, masked / out-of-range rows excluded; fp32 [N][256*32 + 256]
 *          (KV from the 16-bit rounded phi(k) and v, Ksum from the fp32 phi(k)).
 *          wstream_kv = W_k and W_v packed by geoformer_amd/fused.py:pack_kv_stream (256 KiB).
 *   gf_encoder_layer: out = x + LN2(W_2 act(W_1 [x | LN1(W_m msg)])) with
 *          msg = phi(W_q x) KV / (phi(W_q x) . Ksum + attn_eps)       when kv_state is given (S = source length), or
 *          msg = the given attention output [N*L, 256]                 when msg is given;
 *          wstream = fused.py:pack_layer_stream (1 MiB with W_q, 896 KiB without); ln_params = gamma1|beta1|gamma2|beta2
 *          fp32 [4][256]; activation 0 = ReLU, 1 = Tanh; row_flag / flag_rows as in gf_linear (0 -> out = x).
 *   Rounding points (what oracle/geoformer_oracle.py's storage mode mirrors): every MFMA operand is rounded to the
 *   storage type (phi(q), phi(k), v, KV/S, Ksum/S, msg, LN1 output, hidden activations); accumulation, LayerNorm,
 *   phi, the activation and the residual sum are fp32; out is rounded once.
 * ------------------------------------------------------------------------------------------ */
size_t gf_encoder_kv_workspace_bytes(int N, int S);
int gf_encoder_kv_state(const void* src, long ld, int dtype, int N, int S, const uint8_t* kv_mask,
                        const void* wstream_kv, float* kv_state, void* workspace, size_t workspace_bytes,
                        void* stream);
int gf_encoder_layer(const void* x, long ldx, const void* msg, long ldm, const float* kv_state, int S,
                     const uint8_t* q_mask, float attn_eps, const void* wstream, const float* ln_params, float eps1,
                     float eps2, int activation, const int32_t* row_flag, int flag_rows, void* out, long ldo, int dtype,
                     int N, int L, void* stream);
/*   gf_encoder_layer_kv (round 4): gf_encoder_layer in its linear-attention form (kv_state given) whose launch ALSO produces,
 *          for the images tail_first .. N-1, kv_state_out[n - tail_first] = gf_encoder_kv_state of their OUTPUT rows under
 *          wstream_tail - the W_k | W_v stream of the layer call that reads those rows as its source (transformer.py:95-100:
 *          the next layer's source is this layer's output).  The finished 128-token tile is still in the CU's LDS when the
 *          tail's weights arrive through the same ring: no second read of the features, no second launch; masked rows
 *          (q_mask) do not count, as in gf_encoder_kv_state with kv_mask = q_mask.  workspace: gf_encoder_kv_workspace_bytes(
 *          N - tail_first, L).  The states are bit-identical to gf_encoder_kv_state(out[tail_first:], ...)'s. */
int gf_encoder_layer_kv(const void* x, long ldx, const float* kv_state, int S, const uint8_t* q_mask, float attn_eps,
                        const void* wstream, const float* ln_params, float eps1, float eps2, int activation, void* out,
                        long ldo, int dtype, int N, int L, const void* wstream_tail, int tail_first, float* kv_state_out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K11 one encoder layer of the fine-level transformer in ONE launch (16-bit storage modes)
 * replaces LoFTREncoderLayer.forward (model/loftr_src/loftr/loftr_module/transformer.py:37-60) with LinearAttention.forward
 *          (linear_attention.py:21-51) as LocalFeatureTransformer.forward (:82-104) runs it on the fine windows
 *          (model/full_model.py:97-98: [M, W*W = 25, 128] tensors, 8 heads of 16, no masks).
 *   out[w] = x[w] + LN2(W_2 relu(W_1 [x[w] | LN1(W_m msg[w])])),
 *   msg[w] = phi(W_q x[w]) KV[w] / (phi(W_q x[w]) . Ksum[w] + attn_eps),  KV[w], Ksum[w] from phi(W_k src[w]), W_v src[w]
 *   x, src, out: [Nw][Lw][128] contiguous windows of `dtype` (src may be x: the 'self' layers), Lw <= 32;
 *   wstream = geoformer_amd/fused.py:pack_fine_layer_stream (320 KiB); ln_params = gamma1|beta1|gamma2|beta2 fp32 [4][128].
 *   Rounding points = those of the gf_linear / gf_linear_attention chain it replaces (q, k, v, phi(q), phi(k), KV/S, Ksum/S,
 *   the message, LN1 output, hidden activations and LN2 output rounded to the storage type; fp32 accumulation).
 * ------------------------------------------------------------------------------------------ */
int gf_fine_layer(const void* x, const void* src, void* out, int dtype, int Nw, int Lw, const void* wstream,
                  const float* ln_params, float eps1, float eps2, float attn_eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * K10 3x3 / stride 1 / pad 1 convolution of channels-last 16-bit maps with a fused epilogue (backbone)
 * replaces conv3x3 + BatchNorm(eval) [+ shortcut] + ReLU / LeakyReLU of BasicBlock.forward and of the FPN heads
 *          (model/loftr_src/loftr/backbone/resnet_fpn.py:9-40, :60-83, :100-116), BatchNorm folded into the weights
 *   out[n,y,x,:] = act( sum_{ky,kx} w[:, :, ky, kx] . x[n, y+ky-1, x+kx-1, :] + shift + residual[n,y,x,:] )
 *   x [N,H,W,cin], out / residual [N,H,W,cout] (GF_F16 or GF_BF16); fp32 accumulation starting from the shift; GF_F16 with
 *   act 0 / 1: the sum is rounded to half before the residual is added in packed half arithmetic and once more at the output (a
 *   separate convolution followed by gf_bias_act_nhwc rounds twice as well); GF_BF16 and LeakyReLU: residual and activation on
 *   the fp32 accumulators, ONE rounding at the output; act: 0 none, 1 ReLU, 2 LeakyReLU(slope in [0,1]), optionally
 *   | GF_CONV_PAD16 (cout = 224): the caller states that the output channels 196 .. 223 are zero padding (zero weights: the 196
 *   real channels of the reference's middle pyramid level in a 224-wide map) - 16 of them are not multiplied (the accumulator tile
 *   that holds only padding), their outputs are act(shift + residual) as everywhere;
 *   shift fp32 [cout] or NULL; residual or NULL; maps must hold fewer than 2^31 elements;
 *   wstream = geoformer_amd/fused.py:pack_conv3x3_stream(w); zeros = >= 64 bytes of zeroed device memory.
 *   Channel counts: gf_conv3x3_supported(cin, cout).
 * ------------------------------------------------------------------------------------------ */
#define GF_CONV_PAD16 0x100
/*   | GF_CONV_REM8 (round 4; Cin = 224 with Cout = 224 | GF_CONV_PAD16, or Cout = 128): the caller states that the INPUT channels
 *     200 .. 223 carry zero weights (196 real channels: the other side of the same padding) and passes the rem8 packing of the
 *     weights (fused.py:pack_conv3x3_stream(w, rem8=True)): channels 0 .. 191 run as six 32-channel chunks, channels 192 .. 199 as a
 *     remainder whose 9 taps x 8 channels fill three MFMA k-steps instead of a seventh chunk's nine - 114 instead of 126 sub-steps per
 *     tile, the result differs from the plain call only by the order of the fp32 sums. */
#define GF_CONV_REM8 0x200
/*   | GF_CONV_S2 (round 4; cin -> cout in gf_conv3x3s2_supported: 128 -> 224, 224 -> 256): STRIDE 2 - the first convolution of layer2 /
 *     layer3 (resnet_fpn.py:14-17 with stride = 2).  H x W is then the INPUT map; out (and residual) are [N][(H-1)/2+1][(W-1)/2+1][cout];
 *     wstream = fused.py:pack_conv3x3_stream(w, s2=True) (the taps listed parity plane by parity plane).  Replaces the last two
 *     F.conv2d / MIOpen calls + gf_bias_act_nhwc of the 16-bit backbone. */
#define GF_CONV_S2 0x400
int gf_conv3x3_supported(int cin, int cout);
int gf_conv3x3s2_supported(int cin, int cout);
int gf_conv3x3_nhwc(const void* x, const void* wstream, const float* shift, const void* residual, void* out,
                    const void* zeros, int N, int H, int W, int cin, int cout, int act, float slope, int dtype,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * K3  encoder-layer linears with fused epilogues
 * replaces the nn.Linear / LayerNorm / activation / concat / residual sequence of
 * LoFTREncoderLayer.forward (model/loftr_src/loftr/loftr_module/transformer.py:45-60 and
 * model/geo_transformer/transformer.py:49-66) and the two linears of FinePreprocess.forward
 * (model/loftr_src/loftr/loftr_module/fine_preprocess.py:61-72)
 *   out[m,n] = epi( sum_k [a1|a2][m,k] * w[n,k] + bias[n] + rowgroup_bias[m / rowgroup_rows, n] )
 *   a1 [M,k1] row stride lda1, a2 [M,k2] (k2 may be 0) - the two halves of torch.cat([x, message], 2);
 *   w [N, k1+k2] row-major (nn.Linear.weight); bias fp32 [N] or NULL; rowgroup_bias [M/rows, N] or NULL;
 *   epilogue: 0 none, 1 ReLU, 2 Tanh, 3 LayerNorm(gamma, beta, eps) over N,
 *             4 residual + LayerNorm(...) with optional predicate row_flag[m / flag_rows]
 *               (0 -> out = residual: the GeoTransformer "layer skipped for this sample" case);
 *   LayerNorm epilogues need N in {128, 256}; a rowgroup_bias needs N % 128 == 0 (its column tiles are read whole).
 * ------------------------------------------------------------------------------------------ */
int gf_linear(const void* a1, long lda1, int k1, const void* a2, long lda2, int k2, const void* w,
              const float* bias, const void* rowgroup_bias, int rowgroup_rows, int epilogue,
              const float* ln_gamma, const float* ln_beta, float ln_eps, const void* residual, long ldres,
              const int32_t* row_flag, int flag_rows, void* out, long ldo, int dtype, int M, int N,
              void* stream);

/* ------------------------------------------------------------------------------------------
 * homography RANSAC on the device
 * replaces the cv2.findHomography(kp0, kp1, cv2.RANSAC, 8.0) host round trip and the inlier
 * filtering of GeoModule.apply_RANSAC (model/geo_module.py:38-52).  OpenCV parity is unpinned;
 * the algorithm is the one stated in oracle/ransac_oracle.c (bit-exact inlier mask).
 *   mkpts0_c/mkpts1_c [cap,2] fp32 and counts int32[1+N] as written by gf_dual_softmax_match;
 *   gf_ransac_homography_v2 only - lm_iters: Levenberg-Marquardt steps on the inliers' forward transfer error behind the
 *   least-squares refit (OpenCV's findHomography appends 10 to its RANSAC; 0 = none = gf_ransac_homography); the inlier mask
 *   is the best hypothesis' either way;
 *   min_points: samples with fewer matches get no model (GeoModule passes 9: `len(kp0) > 8`, :46);
 *   integer_keypoints = 1: keypoints are truncated like the reference's .long() (GeoModule);
 *   0: sub-pixel keypoints are used as given (homography estimation from fine matches in the
 *   evaluation harness, eval_tool/immatch/utils/hpatches_helper.py:216);
 *   outputs: kp0/kp1 fp32 [cap,2] (the keypoints RANSAC saw), M fp64 [N,9], M_f32 / Minv_f32 [N,9]
 *   (the casts of :58 and :67), valid int32 [N] (0 = "M is None"), keep uint8 [cap] (inlier, or 1
 *   for every match of a sample without model: what feeds the occupancy maps of :82-94).
 * ------------------------------------------------------------------------------------------ */
size_t gf_ransac_workspace_bytes(int N, int iters);
int gf_ransac_homography(const float* mkpts0_c, const float* mkpts1_c, const int32_t* counts, int N,
                         int capacity, float scale, const float* scale0, const float* scale1, float thr,
                         int iters, uint32_t seed, int min_points, int integer_keypoints, float* kp0, float* kp1, double* M,
                         float* M_f32, float* Minv_f32, int32_t* valid, uint8_t* keep, void* workspace,
                         size_t workspace_bytes, void* stream);
int gf_ransac_homography_v2(const float* mkpts0_c, const float* mkpts1_c, const int32_t* counts, int N,
                            int capacity, float scale, const float* scale0, const float* scale1, float thr,
                            int iters, uint32_t seed, int min_points, int integer_keypoints, float* kp0, float* kp1, double* M,
                            float* M_f32, float* Minv_f32, int32_t* valid, uint8_t* keep, void* workspace,
                            size_t workspace_bytes, void* stream, int lm_iters);

/* ------------------------------------------------------------------------------------------
 * relative pose on the device (validation metrics)
 * replaces estimate_pose (model/loftr_src/utils/metrics.py:72-98: cv2.findEssentialMat(..., RANSAC) + cv2.recoverPose, one host
 * round trip per pair) and symmetric_epipolar_distance / compute_symmetrical_epipolar_errors (:30-69).  OpenCV parity is
 * unpinned; the algorithm is the one stated in geoformer_amd/csrc/pose_solver.h (five-point minimal solver, Sampson inliers,
 * closed-form decomposition, cheirality vote over the inliers), which also compiles for the host: bit-exact against that build.
 *   gf_pose_essential_ransac
 *     mkpts0/mkpts1 [cap,2] fp32 pixel keypoints sorted by pair, counts int32[1+N] (total, then per pair) in DEVICE memory;
 *     K0, K1 fp32 [N,9]; keypoints are normalised as (p - (K[0][2], K[1][2])) / (K[0][0], K[1][1]) (:76-77) and the threshold is
 *     pixel_thr / mean(K0[0][0], K1[1][1], K0[0][0], K1[1][1]) (:80), both computed on the device;
 *     iters: FIXED number of hypotheses per pair (no adaptive stop: that would need a host decision), a positive multiple of 32;
 *     a hypothesis = 5 distinct matches drawn by the counter-based hash of gf_ransac_homography from (seed, pair, hypothesis);
 *     outputs per pair: E fp64 [N,9] (Frobenius norm 1), R fp64 [N,9], t fp64 [N,3] (unit), valid int32 [N] (0 = the reference's
 *     `ret is None`: fewer than 5 matches, no hypothesis with 5 inliers, or no candidate in front of both cameras), n_inliers
 *     int32 [N], best int32 [N,2] (chosen hypothesis and root, -1 when invalid); inliers uint8 [cap] per match (all 0 for an
 *     invalid pair; entries past the total count are not written).
 *   gf_epipolar_errors
 *     m_bids int64 [M] pair of every match, T_0to1 fp32 [N,16], E = [t]x R; epi_errs fp32 [M] = (x1^T E x0)^2 (1 / (Ex0[0]^2 +
 *     Ex0[1]^2) + 1 / (E^Tx1[0]^2 + E^Tx1[1]^2)) on normalised coordinates, fp64 arithmetic rounded once (NaN for a pair id
 *     outside [0, N)).
 * ------------------------------------------------------------------------------------------ */
size_t gf_pose_workspace_bytes(int N, int iters);
int gf_pose_essential_ransac(const float* mkpts0, const float* mkpts1, const int32_t* counts, int N, int capacity,
                             const float* K0, const float* K1, float pixel_thr, int iters, uint32_t seed, double* E,
                             double* R, double* t, int32_t* valid, int32_t* n_inliers, int32_t* best, uint8_t* inliers,
                             void* workspace, size_t workspace_bytes, void* stream);
int gf_epipolar_errors(const float* mkpts0, const float* mkpts1, const int64_t* m_bids, int M, const float* T_0to1,
                       const float* K0, const float* K1, int N, float* epi_errs, void* stream);

/* ------------------------------------------------------------------------------------------
 * a8  window geometry
 * replaces get_map_keypoints (utils/common_utils.py:137-144) + warp_points_batch
 * (utils/homography.py:86-105) + generate_window (utils/common_utils.py:65-91) + the cell lookup of
 * sample_descriptors (utils/common_utils.py:171-181)
 *   H fp32 [N,9] maps the (hq x wq) coarse grid of the query image into the other image
 *   (Himg x Wimg pixels, coarse width wk); win int32 [N, hq*wq, ws*ws] = coarse cell sampled by each
 *   window position or -1 when out of bounds (or when valid[n] == 0).
 *   Optional outputs for tests: kps int32 [N,L,ws*ws,2] (the .long() window coordinates, 0 when
 *   out of bounds) and warped fp32 [N,L,2].
 * ------------------------------------------------------------------------------------------ */
int gf_window_geometry(const float* H, const int32_t* valid, int N, int hq, int wq, int Himg, int Wimg,
                       int wk, int scale, int window_size, const float* window_scale, int32_t* win,
                       int32_t* kps_or_null, float* warped_or_null, void* stream);

/* ------------------------------------------------------------------------------------------
 * a7  inlier occupancy maps + token lists
 * replaces model/geo_module.py:82-94 and the boolean-mask gathers feat[mask] of
 * model/geo_transformer/transformer.py:118,121
 *   map0 uint8 [N,L], map1 uint8 [N,S]; idx0 int32 [N,L], idx1 int32 [N,S] ascending cell lists;
 *   nidx int32 [N,2] their lengths.
 * ------------------------------------------------------------------------------------------ */
int gf_inlier_index(const float* kp0, const float* kp1, const uint8_t* keep, const int32_t* counts, int N,
                    int L, int S, int w0, int w1, int scale, uint8_t* map0, uint8_t* map1, int32_t* idx0,
                    int32_t* idx1, int32_t* nidx, void* stream);

/* ------------------------------------------------------------------------------------------
 * K4  self attention over the tokens at inlier cells
 * replaces FullAttention.forward (model/geo_transformer/geo_attention.py:72-101) as called from the
 * 'self' branch of GeoTransformer.forward (model/geo_transformer/transformer.py:111-124)
 *   q [N,L,256], kmap/vmap [N,L,256] = k_proj/v_proj of EVERY token (row strides ld*), idx/nkeys =
 *   the token list of gf_inlier_index; out [N,L,256]; nkeys == 0 -> zeros (layer skipped by caller).
 *   16-bit modes: q and kmap 16-byte aligned with row strides that are multiples of 8 elements (rows move as 16-byte pieces); with
 *   vmap aligned the same way the key / value rows are read from the maps directly (no gather pass; the workspace is then unused):
 *   with row strides below 8192 elements by the head form - one head and 128 queries per workgroup, rows through structured buffer
 *   descriptors - otherwise by the four-head form; both run the arithmetic below bit for bit.
 *   Arithmetic of the 16-bit modes (flash form): the softmax scale lives in the query operand, q' = round(q * log2(e) / sqrt(D)) to the
 *   storage type (one more 16-bit rounding of q), logits q' . k in fp32; per query a softmax reference that starts at the first key
 *   tile's maximum and moves up only when a tile's maximum exceeds it by more than 8 (log2 units); probabilities rounded to the
 *   storage type for P.V, their sum in fp32; mathematically softmax(Q K^T / sqrt(D)) V.  GF_F32: the exact running maximum, the
 *   scale applied to the fp32 logits, fp32 throughout.
 * ------------------------------------------------------------------------------------------ */
size_t gf_self_attention_workspace_bytes(int N, int L, int dtype);
int gf_self_attention_gathered(const void* q, const void* kmap, const void* vmap, int dtype, int N, int L, int H,
                               int D, long ldq, long ldk, long ldv, const int32_t* idx, long idx_stride,
                               const int32_t* nkeys, int nkeys_stride, void* out, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K5  windowed cross attention
 * replaces sample_descriptors (utils/common_utils.py:166-208) + FullAttention.forward with kv_mask
 * (model/geo_transformer/geo_attention.py:72-101) as called from the 'cross' branch of
 * GeoTransformer.forward (model/geo_transformer/transformer.py:125-139)
 *   q [N,L,256]; kmap/vmap [N,S,256] = k_proj/v_proj of every token of the OTHER image;
 *   win int32 [N,L,25] from gf_window_geometry; out [N,L,256] (zeros where all 25 are masked).
 * ------------------------------------------------------------------------------------------ */
int gf_window_cross_attention(const void* q, const void* kmap, const void* vmap, int dtype, int N, int L, int S,
                              int H, int D, long ldq, long ldk, long ldv, const int32_t* win, int WW,
                              const int32_t* valid, void* out, void* stream);
/* Backward of gf_window_cross_attention for the training step: dq [N,L,256] of `dtype`; dk, dv fp32 [N,S,256],
 * ZEROED by the caller - overlapping windows make them scatter-adds (fp32 atomics; the sums are rounded to the storage type once,
 * by the caller).  dout [N,L,256] contiguous.  Masked window positions and queries without a valid key get no gradient. */
int gf_window_cross_attention_backward(const void* q, const void* kmap, const void* vmap, const void* dout, int dtype, int N, int L,
                                       int S, int H, int D, long ldq, long ldk, long ldv, const int32_t* win, int WW, void* dq,
                                       float* dk, float* dv, void* stream);
/* the same gradients without atomics (round 6): dk, dv [N, S, 256] of `dtype` gathered cell by cell along the caller's inverse index of
 * `win` - entries int32 [N * L * WW] = l * WW + k of every (query, window position), sorted (stable) by global cell n * S + cell with the masked
 * positions (cell < 0) last; offsets int32 [N * S + 1] - so the sums run in a fixed order (bit-reproducible) and no fp32 maps are needed.
 * workspace: gf_window_cross_attention_backward_workspace_bytes (the per-(query, position, head) dlogit and p). */
size_t gf_window_cross_attention_backward_workspace_bytes(int N, int L, int WW);
int gf_window_cross_attention_backward_gather(const void* q, const void* kmap, const void* vmap, const void* dout, int dtype, int N, int L,
                                              int S, int H, int D, long ldq, long ldk, long ldv, const int32_t* win, int WW,
                                              const int32_t* entries, const int32_t* offsets, void* dq, void* dk, void* dv, void* workspace,
                                              size_t workspace_bytes, void* stream);
/* The same operation when the query map is hq x wq cells and the key map hk x wk cells (L = hq*wq, S = hk*wk, cells row-major as
 * gf_window_geometry numbers them).  16-bit storage: one workgroup per tile of 8 x 4 query cells and head; the windows of a
 * tile overlap, so the key / value rows of their bounding rectangle are staged in LDS once (a tile whose rectangle exceeds 144
 * cells reads its rows from global memory).  fp32 storage: forwards to gf_window_cross_attention.  Rows must be 16-byte
 * aligned (ld % 8 == 0). */
int gf_window_cross_attention_tiled(const void* q, const void* kmap, const void* vmap, int dtype, int N, int hq, int wq,
                                    int hk, int wk, int H, int D, long ldq, long ldk, long ldv, const int32_t* win,
                                    int WW, const int32_t* valid, void* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * K7  fine window extraction
 * replaces F.unfold + gather + coarse-row gather of FinePreprocess.forward
 * (model/loftr_src/loftr/loftr_module/fine_preprocess.py:41-61)
 *   feat_f0/1 viewed as [N,C,H,W] through strides (4 longs each); feat_c0 [N,L,CC], feat_c1 [N,S,CC];
 *   win_out [2M, W*W, C] (image0 windows then image1), ccat_out [2M, CC].
 *   feat_dtype (the fine maps) and dtype (feat_c*, win_out, ccat_out) are independent: every pair of GF_F32 / GF_F16 / GF_BF16 is
 *   built.  A window element is the map's value widened to fp32 and rounded once to nearest even into dtype (torch's
 *   x.float().to(dtype) for every bit pattern; no clamp, no flush: a finite bf16 value above 65504 becomes +-inf in fp16).  Two
 *   16-bit types with channels-last maps (C % 8 == 0, CC % 8 == 0, 16-byte aligned rows) take the one-wave-per-window kernel
 *   with 16-byte loads and stores, converting in registers when the types differ.
 * ------------------------------------------------------------------------------------------ */
int gf_fine_gather(const void* feat_f0, const void* feat_f1, int feat_dtype, const long* strides0,
                   const long* strides1, int H0, int W0, int H1, int W1, int C, const void* feat_c0,
                   const void* feat_c1, int dtype, int L, int S, int CC, const int64_t* b_ids,
                   const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride, int window,
                   void* win_out, void* ccat_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Backbone glue (fp16 inference backbone; the convolutions themselves stay on PyTorch-ROCm / MIOpen)
 * replaces the element-wise passes of BasicBlock.forward and the FPN merges
 *          (model/loftr_src/loftr/backbone/resnet_fpn.py:20-40 bn/relu/shortcut, :92-95 stem,
 *           :104-105 and :110-111 F.interpolate(..., align_corners=True) + add, :106-115 BN + LeakyReLU)
 *   channels-last tensors ([pixels, C] in memory), C % 4 == 0, 16-byte aligned, in-place allowed.
 *   gf_bias_act_nhwc:     out = act(x + bias[c] + residual);  bias fp32 [C] or NULL, residual or NULL;
 *                         act 0 none, 1 ReLU, 2 LeakyReLU(slope)
 *   gf_upsample_add_nhwc: out = hi + bilinear(lo -> HxW, align_corners=True);  lo [N,h,w,C], hi/out [N,H,W,C]
 * ------------------------------------------------------------------------------------------ */
int gf_bias_act_nhwc(const void* x, const float* bias, const void* residual, void* out, long pixels, int C, int act,
                     float slope, int dtype, void* stream);
int gf_upsample_add_nhwc(const void* lo, const void* hi, void* out, int N, int h, int w, int H, int W, int C,
                         int dtype, void* stream);
/*   gf_upsample_bilinear_backward_nhwc (training): dlo [N,h,w,C] = the gradient of bilinear(lo -> HxW, align_corners=True) with respect to lo
 *                         given dhi [N,H,W,C] (F.interpolate of resnet_fpn.py:104-105,:110-111 under autograd); a gather, no atomics. */
int gf_upsample_bilinear_backward_nhwc(const void* dhi, void* dlo, int N, int h, int w, int H, int W, int C, int dtype, void* stream);
/*   gf_conv1x1_upsample_add_nhwc: out = conv1x1(x; w [Cout,Cin]) + bilinear(lo -> HxW, align_corners=True): the FPN lateral
 *                         convolution with the top-down merge as its epilogue (resnet_fpn.py:109-111); fp16, Cin % 64 == 0 */
int gf_conv1x1_upsample_add_nhwc(const void* x, const void* w, const void* lo, void* out, int N, int h, int wl, int H,
                                 int W, int Cin, int Cout, int dtype, void* stream);

/* K12 (round 4): the same operation as gf_conv1x1_upsample_add_nhwc for the 1/2-scale lateral (cin 128 -> cout 224: layer1_outconv +
 * the merge with the upsampled 1/4-scale map, resnet_fpn.py:109-111) as a streaming kernel of its own - weights resident in LDS as MFMA
 * fragments (wfrag = geoformer_amd/fused.py:pack_lateral_frags(w)), pixel rows by LDS-DMA, the merge's taps requested in front of the
 * tile's MFMAs, 128-byte stores; W must be even.  gf_lateral_supported(cin, cout) names the built widths. */
int gf_lateral_supported(int cin, int cout);
int gf_lateral_upsample_add_nhwc(const void* x, const void* wfrag, const void* lo, void* out, int N, int h, int w, int H, int W,
                                 int cin, int cout, int dtype, void* stream);
/* 1x1 convolution of a channels-last 16-bit map, stride 1 or 2 (H, W even), no bias: out [N, H/s, W/s, Cout] = W x[n, s y, s x, :]
 * (resnet_fpn.py:23-27 the BasicBlock downsample shortcut conv1x1(stride 2), :69-71 layer3_outconv / layer2_outconv, with the
 * BatchNorm scale folded into w [Cout, Cin]); Cin, Cout multiples of 32. */
int gf_conv1x1_nhwc(const void* x, const void* w, void* out, int N, int H, int W, int Cin, int Cout, int stride, int dtype,
                    void* stream);
/*   gf_stem_conv7x7:      out[n,oy,ox,c] = relu(sum_{ky,kx} image[n, 2oy-3+ky, 2ox-3+kx] * weight[c,ky,kx] + shift[c])
 *                         = conv1 (7x7, stride 2, pad 3, 1 input channel) + bn1 (folded) + relu, resnet_fpn.py:60-62, :92;
 *                         image [N,H,W] fp32 or fp16, weight fp32 [C,7,7], shift fp32 [C], out fp16 [N,Ho,Wo,C], C = 128 */
int gf_stem_conv7x7(const void* image, int image_dtype, const float* weight, const float* shift, void* out, int N,
                    int H, int W, int C, void* stream);
/*   gf_stem_conv7x7_dt:   the same with the output / compute type as an argument (GF_F16 or GF_BF16: the operands of the matrix product
 *                         are rounded to it, accumulation fp32); image fp32 or of that type. */
int gf_stem_conv7x7_dt(const void* image, int image_dtype, const float* weight, const float* shift, void* out, int out_dtype, int N,
                       int H, int W, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * K8  fine matching
 * replaces FineMatching2.forward + get_fine_match (model/fine_matching2.py:21-126), M > 0 branch
 *   f0, f1 [M,25,C]; fine_matrix fp32 [M,25,25]; compacted mkpts0_f/mkpts1_f [Mf,2], mconf [Mf],
 *   m_bids int64 [Mf]; count int32 [1] = Mf (device).
 * ------------------------------------------------------------------------------------------ */
size_t gf_fine_match_workspace_bytes(int M);
int gf_fine_match(const void* f0, const void* f1, int dtype, int M, int WW, int C, float temperature, float thr,
                  const int64_t* b_ids, const float* mkpts0_c, const float* mkpts1_c, float coarse_scale,
                  float c2f_scale, float fine_scale, const float* scale0, const float* scale1,
                  float* fine_matrix, float* mkpts0_f, float* mkpts1_f, float* mconf, int64_t* m_bids,
                  int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Image preprocessing: decoded uint8 image -> gray -> resize -> the tensor the model consumes, one launch
 * replaces load_gray_scale_tensor_cv (eval_tool/immatch/utils/data_io.py:48-62): cv2.imread(IMREAD_GRAYSCALE),
 *          cv2.resize on the uint8 image (default INTER_LINEAR), to_tensor
 *   src  uint8 [hs, ws, channels], channels = 3 (RGB interleaved: gray = (R*4899 + G*9617 + B*1868 + 2^13) >> 14) or 1
 *        (already gray), rows src_row_stride_bytes apart (>= ws * channels: a crop or a padded image needs no copy);
 *   dst  dense [ht, wt]: GF_IMAGE_U8 = the resized gray image; GF_IMAGE_F32_NORMALISED = that image / 255 in fp32, the correctly rounded
 *        quotient (torch's `t / 255.0` on the CPU); GF_IMAGE_F32_NORMALISED_RCP = that image * fp32(1 / 255), which is what torch's DEVICE
 *        kernel computes for `t / 255.0` (a Python-scalar divisor becomes a multiplication by the rounded reciprocal there) and so what
 *        matcher.load_gray_scale_tensor's host path hands the model on a GPU; the two differ in the last bit for 126 of the 256 byte values.
 *   ws == wt and hs == ht: gray only;  ws == 2 wt and hs == 2 ht: (a + b + c + d + 2) >> 2;  otherwise OpenCV's 8-bit fixed-point bilinear
 *   (11-bit weights computed on the device from (d + 0.5) * size_ratio - 0.5 in fp64, unfused).  Bit-identical to
 *   geoformer_amd.matcher.cv2_resize_linear_u8(cv2_gray_u8(src), wt, ht).  No workspace.
 * ------------------------------------------------------------------------------------------ */
typedef enum { GF_IMAGE_U8 = 0, GF_IMAGE_F32_NORMALISED = 1, GF_IMAGE_F32_NORMALISED_RCP = 2 } gf_image_kind;
int gf_image_gray_resize(const void* src, int channels, int hs, int ws, long long src_row_stride_bytes, void* dst, int dst_kind,
                         int ht, int wt, void* stream);

/* ------------------------------------------------------------------------------------------
 * One image of a homography training pair, one launch: decoded uint8 image -> gray -> perspective warp -> resize ->
 * brightness / contrast -> the tensor the model consumes; no warped image is materialised
 * replaces get_pair (homodataset/HomoDataset.py:83-123): cv2.warpPerspective(image, M, (warp_w, warp_h)) at the warp's own
 *          resolution (INTER_LINEAR, BORDER_CONSTANT 0), cv2.resize of the uint8 result, the brightness / contrast group of aug_func
 *   src, channels, hs, ws, src_row_stride_bytes, dst, dst_kind, ht, wt   as gf_image_gray_resize; dst holds ht * wt contiguous elements
 *   minv  HOST pointer to 9 doubles, row-major: the INVERSE of the forward matrix M, inverted by the caller in fp64.  Copied into the
 *         launch's arguments (no device buffer, nothing to keep alive).  Every entry must be finite.
 *   warp_h, warp_w  size of the warp's destination image (the reference passes the source's size); the resize reads THAT image
 *   brightness_contrast  NULL, or a HOST pointer to {alpha, beta} (fp32): the resized uint8 value v becomes
 *         clip(trunc(fp32(v) * alpha + beta * 255), 0, 255) before the division (albumentations' uint8 look-up-table rule)
 *   The warp arithmetic is stated in geoformer_amd/csrc/warp_spec.h (OpenCV's 8-bit path: positions rounded to 1/32 pixel, integer
 *   bilinear weights, a tap outside the source counts 0; the numerators are evaluated per pixel, not incrementally per block - OpenCV
 *   parity is unpinned there).  Bit-identical to geoformer_amd.matcher.cv2_resize_linear_u8(geoformer_amd.train.homo_data.
 *   cv2_warp_perspective_u8(cv2_gray_u8(src), M, warp_w, warp_h), wt, ht) followed by homo_data.brightness_contrast_u8.
 *   minv == identity with warp_h == hs and warp_w == ws takes gf_image_gray_resize's path (same bits, no warp arithmetic): image 0 of a pair.
 *   No workspace.
 * ------------------------------------------------------------------------------------------ */
int gf_image_warp_resize(const void* src, int channels, int hs, int ws, long long src_row_stride_bytes, const double* minv,
                         int warp_h, int warp_w, void* dst, int dst_kind, int ht, int wt, const float* brightness_contrast,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * Address-table siblings of gf_pos_encode and gf_fine_gather: the maps of the N samples lie in SEPARATE allocations (feature maps
 * kept per image and matched many times) and are read where they lie - no copy into an [N, ...] batch first.  The only difference
 * from the sibling: sample n starts at table[n] (a table of N addresses in DEVICE memory, entries may repeat) instead of x + n * sn.
 * Same kernel, another map source (csrc/gf_maps.h): same arithmetic, same output bits as the sibling on torch.stack of the maps.
 *   *_align  the largest power of two, in bytes, that divides every table entry (the caller built the table on the host and knows;
 *            any smaller power of two is valid and only selects a slower form): the 8-channel vector form of the position encoding
 *            needs 32, the one-wave-per-window form of the gather 16 - the alignment conditions of the siblings, for every entry.
 *   strides  element strides of ONE map viewed as [C, H, W] (sc, sh, sw), common to all samples; gf_fine_gather_ptrs takes them as
 *            two arrays of 3.  N <= 65535 for gf_pos_encode_ptrs.  Everything else as in the sibling; feat_c0 / feat_c1 stay plain tensors.
 *   The table is read by the launch: it must stay valid (and unchanged) until the launch has run - stream order suffices.
 * ------------------------------------------------------------------------------------------ */
int gf_pos_encode_ptrs(const void* const* x_table, int x_dtype, long sc, long sh, long sw, int x_align, const float* pe,
                       void* out, int out_dtype, int N, int C, int H, int W, void* stream);
int gf_fine_gather_ptrs(const void* const* f0_table, const void* const* f1_table, int N, int feat_dtype, int feat_align,
                        const long* strides0, const long* strides1, int H0, int W0, int H1, int W1, int C,
                        const void* feat_c0, const void* feat_c1, int dtype, int L, int S, int CC, const int64_t* b_ids,
                        const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride, int window,
                        void* win_out, void* ccat_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ragged siblings of the two address-table entries - same kernel, another map source: the N maps of a batch may differ in EXTENT (images
 * of unequal sizes matched in one padded batch).  The device table holds one record per sample instead of a bare address, and the strides and the extent come from
 * the record instead of from the arguments.  The maps are anchored at the top left of a common canvas; a canvas position or a window tap
 * outside a sample's own extent reads as ZERO, whatever lies in memory behind the map - nothing outside [0, h) x [0, w) is ever loaded.
 * Output bits: those of gf_pos_encode / gf_fine_gather on the maps zero-padded at the right and bottom to the canvas and then stacked.
 *   gf_pos_encode_ragged   N, C, H, W describe the CANVAS (pe is [H][W][C], out [N][H*W][C]); every record needs h <= H, w <= W (the
 *            caller's promise, like the addresses).  mask_out: NULL, or uint8 [N][H][W] written by the same launch with
 *            (y < h_n && x < w_n) - the padding mask the matching path takes.  N <= 65535 (the sample is a grid dimension).
 *            The form is chosen per sample from its record (the rule of all three entries, whose strides are the launch's): 8 channels per lane where sc == 1 and sh, sw are multiples of 8 (and
 *            x_align >= 32, C % 8 == 0, pe and out 32-byte aligned), one element per lane for other channels-last maps (sc == 1), and
 *            the 32 x 32 transpose through LDS otherwise (contiguous [C, h, w] maps).
 *   gf_fine_gather_ragged  one table per side, N records each; H0 / W0 / H1 / W1 and the stride arrays of gf_fine_gather_ptrs are gone
 *            (w0c / w1c stay: the CANVAS width in coarse cells, which i_ids / j_ids count in).  One wave per window with 16-byte pieces where
 *            feat_align >= 16, both types are 16-bit and the record has sc == 1 and sh, sw multiples of 8; one workgroup per window otherwise.
 *   *_align  as in the _ptrs entries: the largest power of two, in bytes, that divides every record's base.
 *   The tables are read by the launch: they must stay valid (and unchanged) until the launch has run - stream order suffices.
 * ------------------------------------------------------------------------------------------ */
typedef struct gf_map_record {
    const void* base;      /* element [0][0][0] of the map, in DEVICE memory */
    long sc, sh, sw;       /* element strides of the map viewed as [C, h, w] */
    int h, w;              /* the map's own extent */
} gf_map_record;           /* 40 bytes: five 8-byte words, the last one h | (w << 32) */

int gf_pos_encode_ragged(const gf_map_record* x_table, int x_dtype, int x_align, const float* pe, void* out, int out_dtype,
                         int N, int C, int H, int W, unsigned char* mask_out, void* stream);
int gf_fine_gather_ragged(const gf_map_record* f0_table, const gf_map_record* f1_table, int N, int feat_dtype, int feat_align, int C,
                          const void* feat_c0, const void* feat_c1, int dtype, int L, int S, int CC, const int64_t* b_ids,
                          const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride, int window,
                          void* win_out, void* ccat_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Keypoint consolidation for SfM: pair matches -> one keypoint list per image + every match as a pair of keypoint indices
 * replaces quantize_keypoints, compute_keypoints, get_unique_matches_ids, matches_to_keypoint_ids and the score filter of
 *          process_matches_and_keypoints_exporth5 (eval_tool/immatch/utils/localize_sfm_helper.py:149-230, :353-355, :378-413)
 *
 * The rule (point order, cell, one point against a cell's centres, the filter's winner) is geoformer_amd/csrc/keypoint_spec.h; the serial host
 * form of the whole is csrc/host/keypoint_host.cpp, and the device path gives its bits.  psize <= 0 or dthres <= 0 selects the exact mode
 * (equal coordinates share a keypoint, no filter).  Inputs are fp32: matches [M][4] (x0, y0, x1, y1), scores [M], pair_offsets int32 [P + 1]
 * (ascending, first 0, last M: the rows of pair q), pair_images int32 [P][2].  M <= 2^30 - 1.  A row is dropped when its score is below
 * sc_thres or NaN, or a coordinate is not finite.
 *   SUPPORTED RANGES, checked BEFORE anything is launched (GF_ERR_INVALID_ARGUMENT): n_images <= 524288 (19 key bits); in the quantised mode
 *   psize finite and > 2, so that the cell index floor(c / psize) of any |c| <= 2^22 fits 22 signed bits.  What only the data can break is
 *   reported, never wrapped: a surviving row with a |coordinate| > 2^22 (quantised mode) sets bit 0 of counts[0] and is dropped; a pair whose
 *   image index lies outside [0, n_images) sets bit 1 and loses its rows.
 * The stages, each only enqueuing on `stream`; N = 2 M points in ARRIVAL order (pair, side, row).  The caller owns every buffer and runs the
 * three order-preserving primitives between the stages (a stable sort and two inclusive scans - any implementation):
 *   gf_keypoint_keys     clears counts (int32 [8]: [0] status bits, [4] K keypoints, [5] M' rows - valid after gf_keypoint_emit; the rest is
 *                        internal) and writes keys int64 [N] (dropped points: INT64_MAX), keys2 int64 [N] (exact mode only; may be NULL
 *                        otherwise), pts fp32 [N][2], pseg int32 [N] (2 * pair + side), seg_begin int32 [N]
 *   -> order int64 [N] = the permutation of a STABLE ascending sort by keys (exact mode: by (keys, keys2))
 *   gf_keypoint_heads    head int32 [N]: 1 at the sorted positions where a group starts          -> group_scan = inclusive scan of head
 *   gf_keypoint_walk     owner int32 [N] (arrival index of the point that created the point's keypoint; -1: dropped), slot int32 [N],
 *                        creator int32 [N] (0 / 1), cxy fp32 [N][2] (final coordinates, at the creating points)
 *   -> creator_scan = inclusive scan of creator (arrival order); seg_adj int32 [2 P]: for segment s = 2 * pair + side, (keypoints of all
 *      lower images + keypoints created for its image by earlier segments) - (creators before the segment's first point); kp_offsets
 *      int32 [n_images + 1]
 *   gf_keypoint_filter   keep int32 [M]: surviving rows that win both of their keypoints within their pair (unique == 0: every surviving
 *                        row).  The winner of a keypoint: the highest score, between equal scores the lower row.  -> keep_scan = inclusive scan
 *   gf_keypoint_emit     keypoints fp32 [K][2] image-major (room for N rows), ids int32 [M'][2] in row order (room for M rows),
 *                        pair_offsets_out int32 [P + 1], counts[4], counts[5]
 * workspace: gf_keypoint_workspace_bytes(M) bytes, the SAME buffer for gf_keypoint_walk and gf_keypoint_filter.  Bit-identical from run to run.
 * ------------------------------------------------------------------------------------------ */
size_t gf_keypoint_workspace_bytes(int M);
int gf_keypoint_keys(const float* matches, const float* scores, const int* pair_offsets, const int* pair_images, int P, int M,
                     int n_images, float sc_thres, float psize, float dthres, long long* keys, long long* keys2, float* pts,
                     int* pseg, int* seg_begin, int* counts, void* stream);
int gf_keypoint_heads(const long long* keys, const long long* keys2, const long long* order, int M, int* head, void* stream);
int gf_keypoint_walk(const long long* keys, const long long* order, const int* head, const int* group_scan, const float* pts,
                     const int* seg_begin, int M, float psize, float dthres, int* owner, int* slot, int* creator, float* cxy,
                     int* counts, void* workspace, size_t workspace_bytes, void* stream);
int gf_keypoint_filter(const float* scores, const int* pair_offsets, int P, int M, const int* owner, const int* slot, int unique,
                       int* keep, void* workspace, size_t workspace_bytes, void* stream);
int gf_keypoint_emit(const int* creator, const int* creator_scan, const int* pseg, const int* seg_adj, const float* cxy, const int* keep,
                     const int* keep_scan, const int* pair_offsets, const int* pair_images, int P, int M, const int* owner,
                     const int* kp_offsets, float* keypoints, int* ids, int* pair_offsets_out, int* counts, void* stream);

/* ------------------------------------------------------------------------------------------
 * Two-view geometric verification without intrinsics: fundamental-matrix RANSAC for every pair of a match list
 * (the uncalibrated counterpart of the per-pair geometric verification in eval_tool/immatch/utils/localize_sfm_helper.py; the reference has no
 * fundamental-matrix code).  OpenCV parity is unpinned; the algorithm is the one stated in geoformer_amd/csrc/fund_solver.h (box conditioning,
 * seven-point minimal solver, Sampson inliers in pixels; no refit, no local optimisation, no planar-degeneracy test), which also compiles for
 * the host (csrc/host/fund_host.cpp): bit-exact against that build.
 *   gf_fundamental_ransac
 *     matches fp32 [M,4] (x0, y0, x1, y1 in pixels), scores fp32 [M] or NULL, offsets int32 [N + 1] in DEVICE memory (ascending, first 0, last M:
 *     the rows of pair n - the layout of the keypoint consolidation; entries are clamped into [0, M] before use).  A row takes part iff its four
 *     coordinates are finite and, with scores, its score is not NaN and >= sc_thres (the filter of gf_keypoint_keys).
 *     iters: FIXED number of hypotheses per pair, a positive multiple of 64; hypothesis t of pair n draws its rows from (seed, n, t).
 *     N > 0 and N * (iters / 64) <= 16777216 (the workgroups of one launch); anything else is GF_ERR_INVALID_ARGUMENT, never wrapped.
 *     outputs: F fp64 [N,9] (x1^T F x0 = 0 in pixels, Frobenius norm 1; zeros when not valid), valid int32 [N] (1 iff at least 7 rows take part,
 *     both bounding boxes have an extent and a hypothesis produced a solution), n_inliers int32 [N], best int32 [N,2] (hypothesis, root; -1),
 *     inliers uint8 [M] (the winner's inlier set over the original rows: squared Sampson distance < pixel_thr^2; filtered rows 0).
 *     workspace: gf_fundamental_workspace_bytes(N, M, iters) bytes.  Three launches, no host synchronisation, bit-identical from run to run.
 * ------------------------------------------------------------------------------------------ */
size_t gf_fundamental_workspace_bytes(int N, int M, int iters);
int gf_fundamental_ransac(const float* matches, const float* scores, const int32_t* offsets, int N, int M, float sc_thres,
                          float pixel_thr, int iters, uint32_t seed, double* F, int32_t* valid, int32_t* n_inliers, int32_t* best,
                          uint8_t* inliers, void* workspace, size_t workspace_bytes, void* stream);
/*   gf_fundamental_ransac_lo
 *     gf_fundamental_ransac followed by a refit of every pair's winner on its inliers, on the device (one more launch, still no host
 *     synchronisation): up to refit_rounds times a normalised eight-point fit on the current inlier set (normal matrix summed in a fixed
 *     order, its smallest eigenvector by cyclic Jacobi with fixed sweep counts, rank 2 enforced), the inliers selected again over all rows
 *     that take part with the same pixel_thr, the candidate accepted iff it has at least as many inliers; stops at a rejected candidate, a
 *     failed fit, an unchanged set or fewer than 8 inliers.  The rule is the `refit` entry of geoformer_amd/csrc/fund_solver.h, bit-exact
 *     against the host build like everything above.  No Sampson re-weighting, no planar-degeneracy test, no adaptive stop.
 *     refit_rounds: 0 .. 8, anything else is GF_ERR_INVALID_ARGUMENT; 0 is exactly gf_fundamental_ransac, with rounds all 0.
 *     rounds int32 [N]: the refits accepted for the pair; 0 means F, n_inliers and inliers are the seven-point winner's, bit for bit.
 *     n_inliers never decreases through a refit.  best keeps naming the seven-point (hypothesis, root) that seeded the result.
 *     workspace: gf_fundamental_lo_workspace_bytes(N, M, iters) bytes. */
size_t gf_fundamental_lo_workspace_bytes(int N, int M, int iters);
int gf_fundamental_ransac_lo(const float* matches, const float* scores, const int32_t* offsets, int N, int M, float sc_thres,
                             float pixel_thr, int iters, uint32_t seed, double* F, int32_t* valid, int32_t* n_inliers, int32_t* best,
                             uint8_t* inliers, int refit_rounds, int32_t* rounds, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K3 with a row-address table as the A operand: a gather fused into the GEMM's operand staging.
 *   gf_linear_rows   out[m, :] = epi( row(m) . W^T + bias + rowgroup_bias ), row(m) = the k elements at address row_table[m] (DEVICE memory,
 *            M entries of 64 bits, entries may repeat), or k zeros where row_table[m] == 0.  Everything else as in gf_linear (single-part
 *            operand): w [N][k], bias, rowgroup_bias / rowgroup_rows, the epilogues, out / ldo.  16-bit types only (fp32:
 *            GF_ERR_INVALID_ARGUMENT), k a multiple of 64.  row_align: the CALLER'S PROMISE about the table - a power of two, in bytes, that
 *            divides every non-zero entry, at least 16 (rows are staged as 16-byte pieces).  The entries live in device memory and are
 *            not inspected: the argument exists so that a caller who cannot make the promise gets GF_ERR_INVALID_ARGUMENT instead of
 *            misaligned loads; it selects nothing.  Same tile walk, K loop and matrix-instruction order as gf_linear: the output
 *            bits are those of gf_linear on the rows copied into a buffer.  The table and the rows must stay valid until the launch has run.
 *            group_count (NULL: off): counts that live on the DEVICE.  The M rows come in groups of group_rows; int32
 *            group_count[g * group_count_stride] says how many leading rows of group g are wanted.  The other rows are don't-care: a
 *            128-row tile that holds none of the wanted rows is not computed and its rows of `out` stay UNWRITTEN; don't-care rows of
 *            other tiles are computed like any row (their table entries must be valid).  No host synchronisation.
 *   gf_index_rows    the table of a token list: rows[n][j] = x + (n * L + clamp(idx[n * idx_stride + j], 0, L - 1)) * row_bytes for x of N samples
 *            of L rows (int32 idx with at least L entries per sample; entries behind a sample's count may hold anything).  With
 *            gf_linear_rows and group_count: the k | v projection of GeoTransformer's self layers at the inlier tokens only.
 *   gf_fine_rows / gf_fine_rows_ptrs / gf_fine_rows_ragged   the tables of FinePreprocess.forward for gf_linear_rows, instead of the copies of
 *            gf_fine_gather and its siblings (same map sources, same meaning of every shared argument; 16-bit maps whose channel rows are
 *            contiguous and 16-byte aligned: sc == 1, sh and sw multiples of 8 elements - checked, for a ragged table the caller's promise):
 *            win_rows [2M][window^2]: the address of each tap's channel row (image0's windows first), 0 where gf_fine_gather writes zeros (a
 *            tap outside the map, or outside a ragged map's own extent); coarse_rows [2M]: the addresses of the coarse feature rows
 *            feat_c0[b][i], feat_c1[b][j] (what gf_fine_gather copies into ccat).  One launch, no host synchronisation.
 *            feat_align (_ptrs, _ragged): as in the gather's siblings a promise about the table entries, here required to be at least 16
 *            and otherwise unused - there is one form of the kernel.
 * ------------------------------------------------------------------------------------------ */
int gf_linear_rows(const uint64_t* row_table, int row_align, const int32_t* group_count, int group_count_stride, int group_rows, int k,
                   const void* w, const float* bias, const void* rowgroup_bias, int rowgroup_rows, int epilogue, const float* ln_gamma, const float* ln_beta, float ln_eps, const void* residual,
                   long ldres, const int32_t* row_flag, int flag_rows, void* out, long ldo, int dtype, int M, int N, void* stream);
int gf_index_rows(const void* x, long row_bytes, const int32_t* idx, long idx_stride, int N, int L, uint64_t* rows, void* stream);
int gf_fine_rows(const void* feat_f0, const void* feat_f1, const long* strides0, const long* strides1, int H0, int W0, int H1,
                 int W1, const void* feat_c0, const void* feat_c1, int L, int S, int CC, const int64_t* b_ids,
                 const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c, int stride, int window,
                 uint64_t* win_rows, uint64_t* coarse_rows, void* stream);
int gf_fine_rows_ptrs(const void* const* f0_table, const void* const* f1_table, int N, int feat_align, const long* strides0,
                      const long* strides1, int H0, int W0, int H1, int W1, const void* feat_c0, const void* feat_c1, int L,
                      int S, int CC, const int64_t* b_ids, const int64_t* i_ids, const int64_t* j_ids, int M, int w0c, int w1c,
                      int stride, int window, uint64_t* win_rows, uint64_t* coarse_rows, void* stream);
int gf_fine_rows_ragged(const gf_map_record* f0_table, const gf_map_record* f1_table, int N, int feat_align, const void* feat_c0,
                        const void* feat_c1, int L, int S, int CC, const int64_t* b_ids, const int64_t* i_ids,
                        const int64_t* j_ids, int M, int w0c, int w1c, int stride, int window, uint64_t* win_rows,
                        uint64_t* coarse_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * Localising query images: absolute-pose (P3P) RANSAC over 2-D - 3-D correspondences, one problem per query
 * (the step eval_aachen.py, eval_robotcar.py and eval_inloc.py leave to hloc and pycolmap; the reference has no code for it).  pycolmap
 * parity is unpinned; the algorithm is the one stated in geoformer_amd/csrc/abs_solver.h (box conditioning of the 3-D points, Grunert's P3P,
 * reprojection inliers in pixels, an optional Gauss-Newton refit on the inliers), which also compiles for the host
 * (csrc/host/abspose_host.cpp): bit-exact against that build.
 *   gf_abspose_ransac
 *     p2d fp32 [M,2] (u, v in query pixels), p3d fp32 [M,3] (world units), scores fp32 [M] or NULL, offsets int32 [N + 1] in DEVICE memory
 *     (ascending, first 0, last M: the rows of query n; entries are clamped into [0, M] before use), K fp32 [N,9] (row-major 3 x 3 per
 *     query; K[0], K[2], K[4], K[5] are used).  A row takes part iff its five numbers are finite and, with scores, its score is not NaN
 *     and >= sc_thres.
 *     iters: FIXED number of hypotheses per query, a positive multiple of 64; hypothesis t of query n draws its rows from (seed, n, t).
 *     N > 0 and N * (iters / 64) <= 16777216 (the workgroups of one launch); pixel_thr > 0; anything else is GF_ERR_INVALID_ARGUMENT.
 *     refit_rounds: 0 .. 8, anything else is GF_ERR_INVALID_ARGUMENT.  0: the P3P winner and nothing else (three launches).  R > 0: one
 *     more launch refits the winner on its inliers up to R times (three Gauss-Newton steps on the reprojection error, sums in a fixed
 *     order, inliers selected again, the candidate accepted iff it has at least as many inliers).
 *     outputs: R fp64 [N,9] and t fp64 [N,3] with x_cam = R X + t in world units (zeros when not valid), valid int32 [N] (1 iff at least
 *     4 rows take part, their 3-D box has an extent and a hypothesis produced a solution), n_inliers int32 [N], best int32 [N,2]
 *     (hypothesis, root of the seeding sample; -1), rounds int32 [N] (refits accepted; 0: every output is the P3P winner's), inliers uint8
 *     [M] (point in front of the camera and squared reprojection error < pixel_thr^2; filtered rows 0).
 *     workspace: gf_abspose_workspace_bytes(N, M, iters) bytes.  No host synchronisation, bit-identical from run to run.
 *   gf_xyz_lookup
 *     the 3-D side of the list: xyz fp32 [M,3] = the 3-D map of row i's pair sampled at the row's database keypoint.  table: P records in
 *     DEVICE memory, the map of pair p as [h][w][3] fp32 (a pixel without a 3-D point is NaN; base NULL: a pair without a map);
 *     pair_offsets int32 [P + 1] on the device (the rows of pair p; a row inside no pair gets NaN); the keypoint of row i is
 *     (pts[pts_stride * i], pts[pts_stride * i + 1]) = (x, y) with integer coordinates at pixel centres.  Bilinear over the four
 *     neighbours in fp64, rounded once; NaN when the point lies outside [0, w - 1] x [0, h - 1] or a neighbour is not finite.
 *     The table and the maps must stay valid until the launch has run - stream order suffices.
 * ------------------------------------------------------------------------------------------ */
typedef struct gf_xyz_map {
    const float* base;     /* element [0][0][0] of the map, in DEVICE memory */
    int h, w;              /* its extent */
} gf_xyz_map;              /* 16 bytes: the address, then h | (w << 32) */

size_t gf_abspose_workspace_bytes(int N, int M, int iters);
int gf_abspose_ransac(const float* p2d, const float* p3d, const float* scores, const int32_t* offsets, int N, int M, const float* K,
                      float sc_thres, float pixel_thr, int iters, uint32_t seed, int refit_rounds, double* R, double* t, int32_t* valid,
                      int32_t* n_inliers, int32_t* best, int32_t* rounds, uint8_t* inliers, void* workspace, size_t workspace_bytes,
                      void* stream);
int gf_xyz_lookup(const gf_xyz_map* table, int P, const int32_t* pair_offsets, const float* pts, long pts_stride, int M, float* xyz,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * Triangulating database tracks from known poses (the step localize_sfm_helper.py:reconstruct_database_pairs leaves to hloc's
 * triangulation and COLMAP's point_triangulator; the reference has no code for it).  COLMAP parity is unpinned; the algorithm is the one
 * stated in geoformer_amd/csrc/tri_solver.h (tracks = connected components of the keypoint match graph, two-view midpoint hypotheses,
 * reprojection inliers in pixels, an optional Gauss-Newton refit on the inliers), which also compiles for the host
 * (csrc/host/tri_host.cpp): bit-exact against that build.
 *   gf_track_link
 *     ids int32 [E,2] (per-image keypoint indices of every match row), id_off int32 [P + 1] (the rows of pair p), pair_images int32 [P,2],
 *     kp_off int32 [n_images + 1] (node of keypoint k of image i = kp_off[i] + k; last = n_nodes) - all in DEVICE memory.
 *     parent int32 [n_nodes] is set to the identity, then every row links its two nodes (lock-free union-find: compare-and-swap of the
 *     larger root onto the smaller).  Afterwards every component is one tree whose root is its smallest node.  status int32 [1]: bit 0
 *     (1) when a row named an image outside [0, n_images) or a keypoint its image does not have - such a row is skipped.
 *   gf_track_flatten
 *     parent[v] = the root of v for every node.  The partition and the roots do not depend on the order of execution.
 *   gf_triangulate
 *     track_off int32 [T + 1] in DEVICE memory (ascending, first 0, last n_obs: the observations of track k; entries are clamped into
 *     [0, n_obs] before use), obs_image int32 [n_obs] (ascending inside a track), obs_uv fp32 [n_obs,2] pixels, K fp32 [n_images,9],
 *     R fp64 [n_images,9], t fp64 [n_images,3] with x_cam = R X + t (an image without a pose: NaN - its observations take no part).
 *     pixel_thr > 0; cos_min_angle: the cosine of the smallest triangulation angle of a hypothesis pair; min_obs >= 2; refit 0 .. 8
 *     (0: the two-view midpoint winner and nothing else; R > 0: up to R refits on the inliers, three Gauss-Newton steps each, the
 *     candidate taken iff it has at least as many inliers); T * 64 < 2^31; anything else is GF_ERR_INVALID_ARGUMENT.  A track of effective
 *     length L has min(L (L - 1) / 2, 64) hypotheses: every pair up to L = 11, draws from (seed, track, t) above.
 *     outputs: X fp64 [T,3] (zeros when not valid), valid int32 [T], conflict int32 [T] (an image occurs twice: not triangulated),
 *     n_inliers int32 [T], hypothesis int32 [T] (the seeding pair; -1), rounds int32 [T] (refits accepted; 0: the midpoint's bits),
 *     err2 fp64 [T] (mean squared reprojection error of the inliers), inliers uint8 [n_obs] (0 for every observation of a track that
 *     is not valid).  T = 0 is a no-op.
 *     workspace: gf_triangulate_workspace_bytes(T, n_images) bytes.  No host synchronisation, bit-identical from run to run.
 * ------------------------------------------------------------------------------------------ */
int gf_track_link(const int32_t* ids, const int32_t* id_off, const int32_t* pair_images, int P, int E, const int32_t* kp_off, int n_images,
                  int n_nodes, int32_t* parent, int32_t* status, void* stream);
int gf_track_flatten(int32_t* parent, int n_nodes, void* stream);
size_t gf_triangulate_workspace_bytes(int T, int n_images);
int gf_triangulate(const int32_t* track_off, int T, int n_obs, const int32_t* obs_image, const float* obs_uv, const float* K,
                   const double* R, const double* t, int n_images, float pixel_thr, double cos_min_angle, int min_obs, int refit,
                   uint32_t seed, double* X, int32_t* valid, int32_t* conflict, int32_t* n_inliers, int32_t* hypothesis, int32_t* rounds,
                   double* err2, uint8_t* inliers, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sparse localisation against triangulated points: covisibility clustering of a query's database images, unique 2-D - 3-D rows, and the
 * choice of the winning cluster (what hloc's localize_sfm does with covisibility_clustering=True around pycolmap; the reference has no
 * code for it).  hloc / pycolmap parity is unpinned; the rule is the one stated in geoformer_amd/csrc/covis_spec.h, which also compiles
 * for the host (csrc/host/covis_host.cpp): integer work, byte-exact against that build and from run to run.
 * The pair-level tables are the caller's (O(pairs) bookkeeping): a contributing pair is 8 int32 words (query index, query image, database
 * image, first row and end row in ids, the column of ids holding the query's keypoint, the database image's position in its query's list,
 * 0); list_off [Q + 1] / list_img [L_total] are the per-query database lists in order of first appearance, sorted_img / sorted_pos the
 * same lists sorted by image id with the positions carried along.  Arrays whose names end in _host are HOST copies, read before anything
 * is enqueued: a list above 1024 entries, an image index outside [0, n_images), a row range outside ids and totals at or above 2^31 are
 * GF_ERR_INVALID_ARGUMENT.  What only the device sees (keypoint indices of match rows, point ids) is checked there: the row or keypoint
 * is skipped and a bit of status int32 [1] (zeroed by the caller) is set: 1 image range, 2 keypoint range, 4 point range, 8 list range.
 *   gf_covis_cluster
 *     kp_off int32 [n_images + 1], point_of_keypoint int32 [n_nodes] (-1: none), obs_offsets int32 [T + 1] and obs_image int32 [n_obs] of
 *     the points.  One workgroup per query: positions a and b of a list are linked iff a point has an observation in both images; a
 *     cluster is a connected component on the list alone (lock-free union-find in LDS, the larger root onto the smaller).  outputs:
 *     cluster int32 [L_total] (the cluster number of every position: clusters numbered in ascending order of their smallest position),
 *     n_clusters int32 [Q].  enable == 0: every position has cluster 0.
 *   gf_sparse_rows
 *     one thread per match row of the contributing pairs (pair_row_off int32 [C + 1]: their prefix sum, last = M0).  prob_base int32
 *     [Q + 1]: the exclusive scan of n_clusters.  outputs per row: row_kp (the node of the query keypoint), row_pt (the point of the
 *     database keypoint, -1), row_prob (prob_base[query] + cluster of the database image), keep uint8 (1 iff the row has a point).
 *   gf_covis_select
 *     valid, n_inliers, R, t, rounds [N] and inliers uint8 [M] as gf_abspose_ransac wrote them for the N problems; row_prob and slot int32
 *     [M0] (slot: the RANSAC row that stands for an original row, -1 for a dropped one).  One thread per query: the winner is its valid
 *     problem with the most inliers, then the lowest cluster.  outputs: winner int32 [Q] (a cluster number, -1), localized int32 [Q]
 *     (a winner with at least min_inliers inliers), Rq fp64 [Q,9], tq fp64 [Q,3], nin_q, rounds_q int32 [Q] (the winner's; zeros without
 *     one), is_win uint8 [N], mask uint8 [M0] (a row of a winning problem: the inlier byte of its slot; every other row 0).
 * ------------------------------------------------------------------------------------------ */
int gf_covis_cluster(const int32_t* kp_off, int n_images, const int32_t* point_of_keypoint, int n_nodes, const int32_t* obs_offsets, int T,
                     const int32_t* obs_image, int n_obs, const int32_t* list_off_host, const int32_t* list_img_host, const int32_t* list_off,
                     const int32_t* list_img, const int32_t* sorted_img, const int32_t* sorted_pos, int Q, int L_total, int enable,
                     int32_t* cluster, int32_t* n_clusters, int32_t* status, void* stream);
int gf_sparse_rows(const int32_t* pairs_host, const int32_t* pairs, const int32_t* pair_row_off, int C, int M0, const int32_t* ids, int E,
                   const int32_t* kp_off, int n_images, const int32_t* point_of_keypoint, int n_nodes, int T, const int32_t* list_off,
                   const int32_t* cluster, int L_total, const int32_t* prob_base, int Q, int32_t* row_kp, int32_t* row_pt, int32_t* row_prob,
                   uint8_t* keep, int32_t* status, void* stream);
int gf_covis_select(const int32_t* prob_base, int Q, int N, const int32_t* valid, const int32_t* n_inliers, const double* R, const double* t,
                    const int32_t* rounds, const uint8_t* inliers, int M, const int32_t* row_prob, const int32_t* slot, int M0,
                    int min_inliers, int32_t* winner, int32_t* localized, double* Rq, double* tq, int32_t* nin_q, int32_t* rounds_q,
                    uint8_t* is_win, uint8_t* mask, void* stream);

/* ------------------------------------------------------------------------------------------
 * Bundle adjustment: camera poses and 3-D points refined jointly (what hloc leaves to COLMAP's bundle adjuster; the reference has no code
 * for it).  COLMAP / Ceres parity is unpinned; the rule is the one stated in geoformer_amd/csrc/ba_spec.h - Levenberg-Marquardt on the
 * truncated squared reprojection error, the points eliminated (Schur complement), the 6F x 6F reduced camera system solved by a dense
 * Cholesky, every sum in a stated order - which also compiles for the host (csrc/host/ba_host.cpp): bit-exact against that build and from
 * run to run.
 *   gf_bundle_adjust
 *     Arrays whose names end in _host are HOST copies of the device tables of the same name, read before anything is enqueued.
 *     obs_off int32 [T + 1] (first 0, last n_obs, ascending: the observations of point p), obs_image int32 [n_obs], obs_uv fp32 [n_obs,2]
 *     pixels; img_off int32 [n_images + 1] / img_obs int32 [n_obs]: the same observations by image, ascending inside an image; cam_free
 *     int32 [n_images]: the free cameras numbered 0 .. F - 1 in ascending order of the image, -1 for a fixed one.  K fp32 [n_images,9],
 *     R_in fp64 [n_images,9], t_in fp64 [n_images,3] with x_cam = R X + t (NaN: an image without a pose - its observations take no part, and
 *     it keeps its bits), X_in fp64 [T,3].  thr > 0 (pixels: an observation takes part while its point is in front and its error below
 *     thr; every other one counts thr^2), 1 <= iters <= 64, F <= 128, T, n_obs, n_images >= 1, consistent tables: anything else is
 *     GF_ERR_INVALID_ARGUMENT.  F = 0 refines the points alone.
 *     outputs: R_out, t_out, X_out (images that are fixed or without a pose: the input bits), inliers uint8 [n_obs] (takes part at the final
 *     state), n_inliers int32 [T], cost fp64 [iters + 1] (never increases), accepted int32 [iters], lambda fp64 [iters + 1], status int32 [1]:
 *     1 a step failed and was rejected (the factorisation met a pivot that was not positive, or an update was not finite), 2 a point was
 *     held for an iteration (its damped 3 x 3 system failed the pivot test), 4 a free image has no pose.
 *     workspace: gf_bundle_workspace_bytes(T, n_obs, n_images, F) bytes.  All iterations are enqueued at once: the decision to accept a
 *     step is taken on the device.  No host synchronisation.
 * ------------------------------------------------------------------------------------------ */
size_t gf_bundle_workspace_bytes(int T, int n_obs, int n_images, int F);
int gf_bundle_adjust(const int32_t* obs_off_host, const int32_t* obs_image_host, const int32_t* img_off_host, const int32_t* img_obs_host,
                     const int32_t* cam_free_host, const int32_t* obs_off, int T, int n_obs, const int32_t* obs_image, const float* obs_uv,
                     const int32_t* img_off, const int32_t* img_obs, const int32_t* cam_free, int n_images, int F, const float* K,
                     const double* R_in, const double* t_in, const double* X_in, float thr, int iters, double* R_out, double* t_out,
                     double* X_out, uint8_t* inliers, int32_t* n_inliers, double* cost, int32_t* accepted, double* lambda, int32_t* status,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Bundle adjustment beyond 128 free cameras: the same Levenberg-Marquardt shell, the reduced camera system solved by matrix-free
 * preconditioned conjugate gradients (block-Jacobi preconditioner: the per-camera 6 x 6 blocks) instead of the dense Cholesky.  The rule
 * is geoformer_amd/csrc/ba_pcg_spec.h; the system matrix is never stored, the workspace is O(n_obs + T + F).  Bit-exact against the host
 * build (gf_ba_host_adjust_pcg in csrc/host/ba_host.cpp) and from run to run.
 *   gf_bundle_adjust_pcg
 *     The arguments of gf_bundle_adjust, and: 1 <= cg_iters <= 256 (the cap of CG iterations per LM iteration; running out is no failure,
 *     the cost test judges the step), 0 <= cg_tol < 1 and finite (CG stops once <r, M^-1 r> <= cg_tol^2 times its start), F <= 65536:
 *     anything else is GF_ERR_INVALID_ARGUMENT.  Further outputs: cg_used int32 [iters] (CG iterations completed in each LM iteration),
 *     cg_res fp64 [iters] (the last <r, M^-1 r> over its start; 1 before the first CG iteration completes, 0 when the right-hand side is 0
 *     or F = 0).  Status bit 1 also covers a PCG breakdown (a camera block that cannot be inverted, <p, S p> not positive).
 *     workspace: gf_bundle_pcg_workspace_bytes(T, n_obs, n_images, F) bytes (0 for arguments the entry point rejects).  All LM and CG
 *     iterations are enqueued at once; once a solve has stopped, its remaining launches return at once.  No host synchronisation.
 * ------------------------------------------------------------------------------------------ */
size_t gf_bundle_pcg_workspace_bytes(int T, int n_obs, int n_images, int F);
int gf_bundle_adjust_pcg(const int32_t* obs_off_host, const int32_t* obs_image_host, const int32_t* img_off_host, const int32_t* img_obs_host,
                         const int32_t* cam_free_host, const int32_t* obs_off, int T, int n_obs, const int32_t* obs_image, const float* obs_uv,
                         const int32_t* img_off, const int32_t* img_obs, const int32_t* cam_free, int n_images, int F, const float* K,
                         const double* R_in, const double* t_in, const double* X_in, float thr, int iters, int cg_iters, double cg_tol,
                         double* R_out, double* t_out, double* X_out, uint8_t* inliers, int32_t* n_inliers, double* cost, int32_t* accepted,
                         double* lambda, int32_t* status, int32_t* cg_used, double* cg_res, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * Lens distortion: match coordinates of real cameras -> pixels of an ideal pinhole camera with the same fx, fy, cx, cy, once, before any
 * geometry runs (what COLMAP's estimators do with their image points).  The rule is geoformer_amd/csrc/camera_spec.h: COLMAP's
 * SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL and OPENCV brought to one canonical record; undistortion by a guarded Newton iteration in
 * fp64.  Bit-exact against the host build (csrc/host/camera_host.cpp) and from run to run.  pycolmap parity is UNPINNED.
 *   gf_undistort_points
 *     pts: fp32 point list, row i at pts + pts_stride * i (x, y; pts_stride >= 2: 2 for an [P,2] list, 4 for one side of an [M,4] match
 *     block read in place), P rows cut into S segments by seg_offsets int32 [S+1] (ascending, from 0 to P); segment s belongs to camera
 *     seg_camera[s] (int32 [S]) of cameras fp64 [C,8] = fx, fy, cx, cy, k1, k2, p1, p2.
 *     out fp32 [P,2]: the ideal pixel, each coordinate rounded once to fp32; a camera without distortion passes the input bits through.
 *     status uint8 [P]: 0 fine, 1 non-finite input, 2 no pre-image found, 3 the row lies in no segment or its camera index is outside
 *     [0, C); on status != 0 both coordinates are NaN.  flags int32 [2], zeroed by the caller, only ever set to 1: [0] seg_offsets is not
 *     an ascending list from 0 to P, [1] a camera index outside the table.  P < 0, S < 0, C < 0, and with P > 0: S == 0, C == 0,
 *     pts_stride < 2 or a null pointer are GF_ERR_INVALID_ARGUMENT; P == 0 enqueues nothing.  One launch, no workspace.
 *   gf_distort_points
 *     The same arguments; out is the real-image pixel of an ideal pixel (closed form), status (may be NULL) 0, 1 or 3.
 * ------------------------------------------------------------------------------------------ */
int gf_undistort_points(const float* pts, long pts_stride, int P, const int32_t* seg_offsets, const int32_t* seg_camera, int S,
                        const double* cameras, int C, float* out, uint8_t* status, int32_t* flags, void* stream);
int gf_distort_points(const float* pts, long pts_stride, int P, const int32_t* seg_offsets, const int32_t* seg_camera, int S,
                      const double* cameras, int C, float* out, uint8_t* status, int32_t* flags, void* stream);

/* ------------------------------------------------------------------------------------------
 * Calibrated two-view verification: essential-matrix RANSAC with pose recovery for every pair of a match list, where intrinsics are known
 * (the offsets layout, the row filter and the refit contract of gf_fundamental_ransac*; the solver, the inlier test and the pose recovery
 * of gf_pose_essential_ransac).  The rule is geoformer_amd/csrc/rel_solver.h, which also compiles for the host
 * (csrc/host/relpose_host.cpp): bit-exact against that build and from run to run.  OpenCV parity is UNPINNED.  Profiler tag "rel_ransac".
 *   gf_relpose_ransac
 *     matches fp32 [M,4] (x0, y0, x1, y1 in pixels), scores fp32 [M] or NULL, offsets int32 [N + 1] in DEVICE memory (entries are clamped into
 *     [0, M] before use), K0, K1 fp32 [N,9] row-major intrinsics of the pair's two images.  A row takes part iff its four coordinates are finite
 *     and, with scores, its score is not NaN and >= sc_thres.  Coordinates are normalised by K; pixel_thr is divided by the mean focal length
 *     (ps_threshold).  A pair is estimated iff at least 5 rows take part and K0[0], K0[4], K1[0], K1[4] are finite and positive.
 *     iters: FIXED number of five-point hypotheses per pair, a positive multiple of 64; hypothesis t of pair n draws its rows from (seed, n, t).
 *     N > 0 and N * (iters / 32) <= 16777216 (the workgroups of one launch), pixel_thr positive and finite; anything else is
 *     GF_ERR_INVALID_ARGUMENT, never wrapped.
 *     outputs: E fp64 [N,9] (x1^T E x0 = 0 in normalised coordinates, Frobenius norm 1), R fp64 [N,9] and t fp64 [N,3] of unit length with
 *     x1 ~ R x0 + t, valid int32 [N] (1 iff the winner has at least 5 inliers, E decomposes and a candidate pose has an inlier in front of
 *     both cameras), n_inliers int32 [N], n_cheiral int32 [N] (the chosen candidate's votes), best int32 [N,2] (hypothesis, root; -1),
 *     inliers uint8 [M] (squared Sampson distance in normalised coordinates < thr^2; filtered rows 0).  Not valid: zeros, best -1.
 *     workspace: gf_relpose_workspace_bytes(N, M, iters) bytes.  Four launches, no host synchronisation.
 *   gf_relpose_ransac_lo
 *     followed by a refit of every pair's pose on its inliers (one more launch): up to refit_rounds times three Gauss-Newton steps on the
 *     signed Sampson residual over (R, t) with |t| = 1, sums in a fixed order, the inliers selected again over all rows that take part, the
 *     candidate accepted iff it has at least as many inliers; stops at a rejected candidate, a failed fit, an unchanged set or fewer than 6
 *     inliers.  refit_rounds: 0 .. 8; 0 is exactly gf_relpose_ransac, with rounds all 0.  rounds int32 [N]: the refits accepted; 0 means the
 *     five-point winner's bits.  After an accepted refit E = [t]x R scaled to norm 1.  n_inliers never decreases; best and n_cheiral keep
 *     describing the seeding hypothesis.  workspace: gf_relpose_lo_workspace_bytes(N, M, iters) bytes.
 * ------------------------------------------------------------------------------------------ */
size_t gf_relpose_workspace_bytes(int N, int M, int iters);
int gf_relpose_ransac(const float* matches, const float* scores, const int32_t* offsets, int N, int M, const float* K0, const float* K1,
                      float sc_thres, float pixel_thr, int iters, uint32_t seed, double* E, double* R, double* t, int32_t* valid,
                      int32_t* n_inliers, int32_t* n_cheiral, int32_t* best, uint8_t* inliers, void* workspace, size_t workspace_bytes,
                      void* stream);
size_t gf_relpose_lo_workspace_bytes(int N, int M, int iters);
int gf_relpose_ransac_lo(const float* matches, const float* scores, const int32_t* offsets, int N, int M, const float* K0, const float* K1,
                         float sc_thres, float pixel_thr, int iters, uint32_t seed, double* E, double* R, double* t, int32_t* valid,
                         int32_t* n_inliers, int32_t* n_cheiral, int32_t* best, uint8_t* inliers, int refit_rounds, int32_t* rounds,
                         void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GEOFORMER_HIP_H_ */
