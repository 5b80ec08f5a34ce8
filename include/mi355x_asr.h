/* mi355x_asr.h -- C ABI of libmi355x_asr.so: the MI355X (gfx950 / CDNA4) kernels behind the drop-in
 * Conformer-CTC training path (NeMo `EncDecCTCModel` + `ConformerEncoder`).
 *
 * The reference has NO C ABI on this path (its host code is Python calling ATen), so this boundary is defined
 * here, directly under the Python NeuralModule classes.  Conventions:
 *   - every entry point returns 0 on success, 1 = invalid argument (the Python binding raises ValueError, the
 *     reference's convention: conformer_encoder.py:569-578, features.py:288-305), 1000 + hipError_t = launch failure
 *     (RuntimeError);
 *   - all pointers are DEVICE pointers owned by the caller (torch allocates; kernels never allocate or free);
 *   - `stream` is a hipStream_t (0 = default stream); calls are asynchronous and re-entrant across streams;
 *   - dtype codes: 0 = float32, 1 = bfloat16 (raw 16-bit); lengths are int64 like the reference's LengthsType tensors;
 *   - activations are channels-last: [B, T, d] rows m = b*T + t; conv feature maps [B, T, F, C].
 *
 * Each declaration cites the reference interface (file:line under the NeMo tree) whose arithmetic it replaces.
 */
#ifndef MI355X_ASR_H
#define MI355X_ASR_H
#ifdef __cplusplus
extern "C" {
#endif

#define MI355X_DT_F32 0
#define MI355X_DT_BF16 1

/* ---- GEMM with fused epilogues ------------------------------------------------------------------------------
 * C[M,N] = epi( sum_k A(m,k) * B(n,k) ).  trans{A,B}=0: operand stored [rows][K] (K contiguous);
 * =1: stored [K][rows] (reduction-major: wgrad / P@V).  Batched: z in [0,batch): z0 = z % nb0, z1 = z / nb0,
 * operand offset = z0*s?0 + z1*s?1 (elements).  bf16 inputs run on MFMA, f32 inputs on an exact fp32 kernel.
 * Replaces: F.linear / Conv1d(k=1) / matmul / conv2d-as-GEMM in conformer_modules.py:382-387,321,343;
 * multi_head_attention.py:124-146,300-350; subsampling.py:231-253,431; conv_asr.py:445.                        */
enum {
  MI355X_EPI_STORE = 0,      /* C = alpha * dropout(acc + bias)                                                  */
  MI355X_EPI_SWISH_DROP = 1, /* aux_out = acc + bias ; C = dropout(swish(acc + bias))          (FFN linear1)     */
  MI355X_EPI_RESID = 2,      /* C(f32) = aux_in(f32) + alpha * dropout(acc + bias)             (residual branch) */
  MI355X_EPI_DSWISH = 3,     /* C = acc * dropmask * swish'(aux_in)                            (FFN dgrad)       */
  MI355X_EPI_RELU_MASK = 4,  /* C = relu(acc + bias) * [ (m % rows_per_b) / rows_inner < row_len[m / rows_per_b] ] */
  MI355X_EPI_MUL_POS = 5,    /* C = acc * (aux_in > 0)                                         (ReLU dgrad)      */
  /* the feed-forward pair with the Swish derivative taken in the FORWARD epilogue (which holds sigmoid(h) and the dropout mask
   * in registers anyway): aux_out = swish'(acc + bias) * dropmask instead of the pre-activation, and the backward epilogue is
   * one multiply (no exp / rcp / mask hash per element).  ConformerFeedForward, parts/submodules/conformer_modules.py:366-387 */
  MI355X_EPI_SWISH_DROP_G = 6, /* aux_out = swish'(acc + bias) * dropmask ; C = dropout(swish(acc + bias))        */
  MI355X_EPI_DSWISH_G = 7      /* C = acc * aux_in            (aux_in = the aux_out of MI355X_EPI_SWISH_DROP_G)   */
};
typedef struct mi355x_gemm_desc {
  const void* A; const void* B; void* C;
  int M, N, K;
  long long lda, ldb, ldc;          /* row pitch (elements) of the stored matrices                               */
  long long c_col_stride;           /* column stride of C (0/1 = dense); lets wgrad write the reference's layouts  */
  int transA, transB;
  int in_dtype;                     /* dtype of A and B                                                          */
  int c_dtype;                      /* dtype of C                                                                */
  int batch, nb0;
  long long sA0, sA1, sB0, sB1, sC0, sC1;
  const void* bias;                 /* f32 [N] or NULL                                                           */
  float alpha;
  int epilogue;
  int atomic;                       /* 1: atomicAdd into f32 C (required for splitk > 1)                         */
  int splitk;
  const void* aux_in; int aux_in_dtype;
  void* aux_out; int aux_out_dtype;
  long long ldaux;                  /* pitch of aux_in / aux_out (same batch offsets as C)                       */
  unsigned drop_key, drop_threshold; float drop_scale;   /* threshold 0 = dropout off                            */
  const void* row_len; int rows_per_b; int rows_inner;   /* EPI_RELU_MASK: int64 [B] valid lengths; optional with EPI_MUL_POS:
                                                          * the caller's promise that aux_in <= 0 on rows beyond them -- tiles that
                                                          * lie entirely there are zero-filled (through the row map) without a K loop */
  long long colsum_stride;          /* batch stride of colsum_out (elements)                                       */
  void* colsum_out;                 /* optional (bf16, transA=1, single-level batch): f32 [M] += sum_k A(k,m) -- the bias gradient
                                       of a Linear rides along with its weight-gradient GEMM                       */
  /* Implicit-GEMM convolution on channels-last feature maps (Conv2d of ConvSubsampling, subsampling.py:385-436, without
   * an im2col buffer).  gather (bf16, transA = 0, batch = 1, C % 64 == 0): row m = (b*nI + i)*nJ + j of A is gathered,
   * for K index tap*C + c, from A[b][i*si + di[tap]][j*sj + dj[tap]][c] of a [.., SI, SJ, C] grid (zero outside);
   * K must equal ntaps*C; lda is ignored.  rowmap: row m = (b*nI + i)*nJ + j of C and of aux_in/aux_out is stored at row
   * (b*OI + i*si + oi)*OJ + j*sj + oj (the dgrad of a strided conv writes one parity class of positions per launch). */
  const struct mi355x_conv_gather* gather;   /* NULL = dense A */
  const struct mi355x_row_map* rowmap;       /* NULL = dense C rows */
} mi355x_gemm_desc;
typedef struct mi355x_conv_gather {
  int nI, nJ, SI, SJ, C, si, sj, ntaps; int di[9], dj[9];
  int operand;   /* 0: A rows gathered as described above.  1: weight gradient -- B (transB = 1) is gathered instead: K runs
                    over the positions m = (b*nI + i)*nJ + j, N = C channels, batch index z (0..ntaps-1) selects the tap;
                    B points at the source grid, ldb / sB are ignored, transA must be 1 */
} mi355x_conv_gather;
typedef struct mi355x_row_map { int nI, nJ, OI, OJ, si, sj, oi, oj; } mi355x_row_map;
int mi355x_gemm(const mi355x_gemm_desc* desc, void* stream);
/* kernel-structure selection knobs for tests and A/B benchmarks (results do not depend on them beyond fp32 summation order).
 * key 4: the 256x256 tile structures (0 = never, 1 = where the tile count fills the chip (default), 2 = whenever N > 128);
 * key 5: the persistent 256x128 structure with overlapped epilogues (0 = never, 1 = where it measured faster (default),
 * 2 = wherever it can run); key 6: operands of the 256x256 structure prefetched through registers two K-tiles deep instead of
 * LDS-DMA (0 / 1 = default, for K-contiguous operands with K % 128 == 0); key 7: the same inside the 256x128 structure;
 * key 3: fp32 problems on the matrix cores, v_mfma_f32_32x32x2_f32 (1 = default, 0 = the vector-unit kernel);
 * key 8: the phase-staggered 256x256 structure on 16x16x32 MFMAs (0 never, 1 = default: K-contiguous layouts that fill the chip
 * with 256x256 tiles, dense or with gathered A rows; 2 = every problem it can run; 3 = as 1 plus the weight-gradient layouts,
 * 4 = as 1 plus the wide plain stores the persistent structure otherwise takes, 5 = as 1 plus its 128x256 tile where only that
 * fills the chip and K >= 768); key 9: start delay of every other first-round workgroup of that
 * structure in 10-ns ticks (experiment, default 0); key 10: its specialised epilogue rounds (1 = default, 0 = generic round);
 * key 11 (read only, value ignored): structure of the calling thread's last mi355x_gemm launch (800 + round = that structure, 810 = its
 * 128x256 tile, 0 = another one).
 * Returns the previous EFFECTIVE value (the environment default if the key was never set: always >= 0, and writing it back restores
 * exactly the earlier state), or -1 for an unknown key. */
int mi355x_gemm_config(int key, int value);
/* What mi355x_gemm would launch for `desc` under the current knobs, without launching (no GPU needed; pointers are checked for
 * alignment only).  Returns what mi355x_gemm's argument checks return (1 = rejected); on 0 out = { kernel id (csrc/gemm.hip: GemmKernel),
 * the key-11 code, grid x, y, z, workgroup size, dynamic LDS bytes, key-9 delay of this launch }. */
int mi355x_gemm_plan(const mi355x_gemm_desc* desc, int out[8]);
/* Up to 12 independent weight-gradient problems in one launch: every desc must be bf16, transA = transB = 1, atomic
 * f32 C with dense columns, no bias / aux / epilogue, and share K (the token count); descs[0].splitk applies to all.
 * colsum_out (the bias gradient) is honoured per problem.  See csrc/gemm.hip: gemm_bf16_grouped_tn_kernel. */
int mi355x_gemm_grouped(const mi355x_gemm_desc* descs, int n, void* stream);

/* ---- fused macaron feed-forward block, d_model = 512 (ConformerFeedForward.forward, parts/submodules/conformer_modules.py:366-387:
 * Linear -> Swish -> Dropout -> Linear, with the residual `residual + dropout(ff(x)) * fc_factor` of :174-181 / :209-215).
 * One launch: h (bf16 [M, d_ff], pitch ldh) = y @ W1^T + b1 is the only intermediate that reaches memory (backward needs it);
 * out f32 [M, 512] = x_resid + alpha * drop_res( drop_in(swish(h)) @ W2^T + b2 ).  y = LayerNorm output, bf16 [M, 512].
 * Dropout indices are those of the unfused GEMM epilogues: element (m, n) of [M, d_ff] resp. [M, 512] -> m * N + n.
 * The weights are PACKED bf16 images written by mi355x_ffn_pack, MFMA-fragment-major in the order the kernel consumes them.  A
 * fragment = 32 rows x 16 k = 1 KiB stored [hh][lr][8]: element (row lr, k = 8 hh + e) at (hh*32 + lr)*8 + e.
 *   "k512"   order of a logical A [d_ff][512]: fragment of rows c*64 + mt*32 .. +31, k = k16*16 .. +15 at ((c*32 + k16)*2 + mt) KiB
 *   "kchunk" order of a logical B [512][d_ff]: fragment of rows q*128 + mt4*32 .. +31, k = t*16 .. +15 at ((t*4 + q)*4 + mt4) KiB
 * w1_packed = k512(W1), w2_packed = kchunk(W2).  128 <= d_ff <= 2048, d_ff % 64 == 0; all pointers 16-byte aligned; pitches
 * multiples of 8 (ldx: of 4). */
int mi355x_ffn_fwd(const void* y, long long ldy, const void* w1_packed, const void* b1, const void* w2_packed, const void* b2,
                   const void* x_resid, long long ldx, void* h, long long ldh, void* out, long long ldo, int M, int d_model,
                   int d_ff, float alpha, unsigned drop_in_key, unsigned drop_in_threshold, float drop_in_scale,
                   unsigned drop_res_key, unsigned drop_res_threshold, float drop_res_scale, void* stream);
/* Its input-gradient chain in one launch (autograd of the same lines): df bf16 [M, 512] = the gradient of the block's output
 * through the residual scale and dropout; g = df @ W2; dh = g * dropmask_in * swish'(h) -> bf16 [M, d_ff] (pitch ldh; operand of
 * the W1 weight gradient); act = drop_in(swish(h)) -> bf16 [M, d_ff] (pitch ldh; RECOMPUTED operand of the W2 weight gradient);
 * dy bf16 [M, 512] = dh @ W1 (gradient w.r.t. the LayerNorm output).  w2t_packed = k512(W2^T), w1t_packed = kchunk(W1^T). */
int mi355x_ffn_bwd_dgrad(const void* df, long long lddf, const void* w2t_packed, const void* w1t_packed, const void* h,
                         long long ldh, void* dh, void* act, void* dy, long long lddy, int M, int d_model, int d_ff,
                         unsigned drop_in_key, unsigned drop_in_threshold, float drop_in_scale, void* stream);

/* The four images of n weight matrices in one launch (no reference analogue; runs once per optimizer step next to
 * mi355x_pack_weights).  Entry i: src = fp32 master weight, either linear1.weight [d_ff][512] (is_w2 = 0: writes k512(W1) and
 * kchunk(W1^T)) or linear2.weight [512][d_ff] (is_w2 = 1: writes kchunk(W2) and k512(W2^T)); both destinations 512 * d_ff bf16. */
typedef struct mi355x_ffn_pack_entry { const void* src; void* k512; void* kchunk; int d_ff; int is_w2; } mi355x_ffn_pack_entry;
int mi355x_ffn_pack(const void* table_dev, int n_entries, int max_d_ff, void* stream);

/* ---- log-mel front-end: FilterbankFeatures.forward, parts/preprocessing/features.py:423-502 --------------------
 * audio f32 [B,S], audio_len i64 [B] -> out f32 [B,n_mels,T] = log(mel_power + log_guard), T = 1 + S/hop.
 * fb_* = sparse rows of the (persistent) `fb` buffer: for mel m, weights fb_w[fb_off[m] .. +fb_len[m]) apply to FFT
 * bins fb_start[m]...  n_fft must be 512 (Hann window `window[win]` is centred in the FFT frame like torch.stft).
 * Any row layout is accepted; when every fb_off[m] is a multiple of 4 and fb_off[m+1] >= fb_off[m] + 4 * ceil(fb_len[m] / 4)
 * (`sparsify_filterbank` lays the rows out so) the default kernel reads a row as 16-byte vectors without end-of-row checks. */
int mi355x_logmel_fwd(const void* audio, const void* audio_len, const void* window, int win, int hop, int n_fft,
                      const void* fb_start, const void* fb_len, const void* fb_off, const void* fb_w, int n_mels,
                      float preemph, float dither, unsigned seed, float log_guard, void* out, int B, int S, int T,
                      void* stream);
/* which front-end kernel runs (tests and A/B): 2 (default) = FFT in registers (16 lanes per frame, 16-point DFTs on a lane's own
 * points, one LDS transpose, dither evaluated once per sample; profiles/r6_logmel.md; an odd hop takes variant 1), 1 = the
 * wave-synchronised radix-4 kernel (two frames in flight per wave, filterbank in LDS; profiles/r4_logmel.md), 0 = the round-1 kernel.
 * variant < 0 only queries.  Returns the previous setting.  Environment: MI355X_LOGMEL.  (features.py:423-502) */
int mi355x_logmel_config(int variant);
/* normalize_batch(..., 'per_feature') + pad fill, features.py:59-93,490-493.  x f32 [B,n_mels,T] -> y (y_dtype) */
int mi355x_feat_normalize(const void* x, const void* seq_len, void* y, int y_dtype, int B, int n_mels, int T,
                          int normalize, float pad_value, void* stream);

/* ---- convolution sub-sampling pieces: ConvSubsampling.forward, parts/submodules/subsampling.py:385-436,725-759 - */
int mi355x_subsample_conv1_fwd(const void* mel /*f32 [B,F,T]*/, const void* w /*[C,1,3,3]*/, const void* bias,
                               void* out /*[B,T1,F1,C]*/, int out_dtype, const void* len0, const void* len1, int B, int F,
                               int T, int C, void* stream);
int mi355x_subsample_conv1_bwd(const void* dout, int dtype, const void* mel, const void* len0, void* dw, void* db, int B,
                               int F, int T, int C, void* scratch /* optional f32 [ceil(T1/32)*B*10*C]: two-stage reduction */,
                               long long scratch_elems, void* stream);
int mi355x_im2col_3x3s2(const void* in /*[B,T1,F1,C]*/, void* col /*[B*T2*F2, 9C]*/, int dtype, int B, int T1, int F1, int C,
                        void* stream);
int mi355x_col2im_3x3s2_relu(const void* dcol, const void* act, void* din, int dtype, int B, int T1, int F1, int C,
                             void* stream);
/* The same four with the padding as an argument: `pad` zero rows / columns in FRONT of the grid, one behind it -- 1 = Conv2d(
 * padding = 1) (what the entries above run), 2 = CausalConv2D of `causal_downsampling: true` (parts/submodules/causal_convs.py:24-72,
 * subsampling.py:147-149,222-224: F.pad (2, 1) on time AND frequency, then no padding).  Output extents: floor((n + pad - 2) / 2) + 1. */
int mi355x_subsample_conv1_fwd_pad(const void* mel, const void* w, const void* bias, void* out, int out_dtype, const void* len0,
                                   const void* len1, int B, int F, int T, int C, int pad, void* stream);
int mi355x_subsample_conv1_bwd_pad(const void* dout, int dtype, const void* mel, const void* len0, void* dw, void* db, int B,
                                   int F, int T, int C, int pad, void* scratch, long long scratch_elems, void* stream);
int mi355x_im2col_3x3s2_pad(const void* in, void* col, int dtype, int B, int T1, int F1, int C, int pad, void* stream);
int mi355x_col2im_3x3s2_relu_pad(const void* dcol, const void* act, void* din, int dtype, int B, int T1, int F1, int C, int pad,
                                 void* stream);

/* 'dw_striding' sub-sampling (FastConformer x8, Squeezeformer x4; subsampling.py:142-215): depthwise Conv2d(C, C, 3, stride 2,
 * padding 1, groups = C) on a channels-last map in [B,T1,F1,C] -> out [B,T2,F2,C] (+ bias); w f32 [C,1,3,3].  The pointwise
 * convolution + ReLU + time mask that follow are mi355x_gemm (EPI_RELU_MASK).  Backward: din = (in > 0) * dgrad (the ReLU of the
 * previous stage), dw / dbias accumulated (+=); scratch f32 [min(1024, ceil(B*T2*F2/64)) * 10 * C]. */
int mi355x_dwconv2d_s2_fwd(const void* in, const void* w, const void* bias, void* out, int dtype, int B, int T1, int F1, int C,
                           void* stream);
int mi355x_dwconv2d_s2_bwd(const void* dout, const void* in, const void* w, void* din, void* dw, void* dbias, int dtype, int B,
                           int T1, int F1, int C, void* scratch, long long scratch_elems, void* stream);
/* ... with `pad` as above (CausalConv2D stages of the cache-aware streaming FastConformer recipes) */
int mi355x_dwconv2d_s2_fwd_pad(const void* in, const void* w, const void* bias, void* out, int dtype, int B, int T1, int F1, int C,
                               int pad, void* stream);
int mi355x_dwconv2d_s2_bwd_pad(const void* dout, const void* in, const void* w, void* din, void* dw, void* dbias, int dtype, int B,
                               int T1, int F1, int C, int pad, void* scratch, long long scratch_elems, void* stream);

/* ---- transducer head (FastConformer-Transducer): RNNTDecoder.predict / RNNTJoint.joint_after_projection,
 * nemo/collections/asr/modules/rnnt.py:700-830, 1640-1720; LSTM = common/parts/rnn.py:151-230 (torch gate order i,f,g,o).
 * The gate / projection / output-layer contractions are mi355x_gemm; these are the pieces between them. */
/* out (dtype) [U+1,B,H]: row 0 = zero start-of-sequence frame, row u+1 = emb[targets[b,u]] (blank id = padding row = 0) */
int mi355x_embed_sos_fwd(const void* targets /*i64 [B,U]*/, const void* emb /*f32 [V+1,H]*/, void* out, int dtype, int B, int U,
                         int H, int blank, void* stream);
int mi355x_embed_sos_bwd(const void* targets, const void* dx /*[U+1,B,H]*/, int dtype, void* demb /*f32 +=*/, int B, int U, int H,
                         int blank, void* stream);
/* one LSTM step: z f32 [B,4H] holds x W_ih^T + b_ih + h_prev W_hh^T on entry and the ACTIVATED gates on exit; c_prev may be
 * NULL (zero state); h is written in f32 and in the GEMM operand dtype */
int mi355x_lstm_cell_fwd(void* z, const void* b_hh, const void* c_prev, void* c, void* h, void* h_lp, int lp_dtype, int B, int H,
                         void* stream);
/* dh f32 [B,H]; dc f32 [B,H] in = d/dc_t from step t+1, out = d/dc_{t-1}; dz (dtype) [B,4H] = pre-activation gradients */
int mi355x_lstm_cell_bwd(const void* dh, void* dc, const void* act, const void* c, const void* c_prev, void* dz, int dz_dtype,
                         int B, int H, void* stream);
/* h [B,T,U1,J] = dropout(relu(f[b,t,:] + g[b,u,:])); backward: dh <- dh * (h > 0) * drop_scale in place, df [B,T,J] = sum_u */
int mi355x_joint_combine_fwd(const void* f, const void* g, void* h, int dtype, unsigned drop_key, unsigned drop_threshold,
                             float drop_scale, int B, int T, int U1, int J, void* stream);
int mi355x_joint_combine_bwd(void* dh, const void* h, void* df, int dtype, float drop_scale, int B, int T, int U1, int J,
                             void* stream);
/* dst (dtype) [M, Np] (pitch ld_out) = alpha * src f32 [M, N] (pitch ld_in), columns N..Np-1 zero: GEMM operand rows */
int mi355x_cast_rows(const void* src, long long ld_in, void* dst, int dst_dtype, long long ld_out, long long M, int N, int Np,
                     float alpha, void* stream);

/* ---- Squeezeformer block glue (BASELINE.json configs[4]): squeezeformer_modules.py:30-57 (ScaleBiasLayer), :139-181 (post-LN
 * block order), conformer_modules.py:267-275 ('swish' point-wise activation), subsampling.py:589-646 (TimeReductionModule),
 * squeezeformer_encoder.py:352-361 (time recovery).  `ld` = row pitch of a produced GEMM operand (>= d, multiple of 4; columns
 * [d, ld) are zero-filled) so that d_model % 8 != 0 (Medium: 324) still gives 16-byte aligned bf16 rows. */
/* y (dtype) [M, ld] = x f32 [M, d] * scale + bias   (scale = bias = NULL: plain cast, adaptive_scale = False) */
int mi355x_scale_bias_fwd(const void* x, const void* scale, const void* bias, void* y, int y_dtype, long long M, int d, int ld,
                          void* stream);
/* dres f32 [M, d] += dy * scale;  dscale[d] += colsum(dy * x);  dbias[d] += colsum(dy)   (dscale = dbias = NULL: skipped);
 * scratch: f32 work space of at least min(M, 512) * 2 * d elements (per-workgroup partial column sums) */
int mi355x_scale_bias_bwd(const void* dy, int dy_dtype, int ld, const void* x, const void* scale, void* dres, void* dscale,
                          void* dbias, long long M, int d, void* scratch, long long scratch_elems, void* stream);
/* y (dtype) [M, ld] = alpha * dropmask(m*d + c) * x f32 [M, d]  -- the dropout mask of a GEMM epilogue with N = d */
int mi355x_cast_pitched(const void* x, void* y, int y_dtype, long long M, int d, int ld, float alpha, unsigned drop_key,
                        unsigned drop_threshold, float drop_scale, void* stream);
/* out [M, C] = swish(in) * (t < len[b]),  rows m = b*T + t;  backward: din = dout * swish'(in) * mask */
int mi355x_swish_mask_fwd(const void* in, void* out, int dtype, const void* len, int T, long long M, int C, void* stream);
int mi355x_swish_mask_bwd(const void* in, const void* dout, void* din, int dtype, const void* len, int T, long long M, int C,
                          void* stream);
/* masked depthwise Conv1d(k=5, stride 2, pad 3) over time, cropped to ceil(T/2) frames: x f32 [B,T,d] -> out (dtype)
 * [B*ceil(T/2), ld]; w f32 [d,1,5].  backward: dx f32 [B,T,d] +=, dw +=, dbias += */
int mi355x_time_reduce_dwconv_fwd(const void* x, const void* len, const void* w, const void* bias, void* out, int out_dtype, int B,
                                  int T, int d, int ld, void* stream);
int mi355x_time_reduce_dwconv_bwd(const void* dout, int dout_dtype, int ld, const void* x, const void* len, const void* w, void* dx,
                                  void* dw, void* dbias, int B, int T, int d, void* stream);
/* out f32 [B,T,d] = skip + ys[b, t/2, :]  (ys f32 [B, ceil(T/2), d]);  backward: dys (dtype) [B*ceil(T/2), ld] = dx[2t'] + dx[2t'+1] */
int mi355x_time_recover_fwd(const void* skip, const void* ys, void* out, int B, int T, int d, void* stream);
int mi355x_time_recover_bwd(const void* dx, void* dys, int dys_dtype, int B, int T, int d, int ld, void* stream);

/* ---- LayerNorm (torch.nn.LayerNorm x5 per layer, conformer_modules.py:174-215) -------------------------------- */
int mi355x_layernorm_fwd(const void* x, int x_dtype, const void* gamma, const void* beta, void* y, int y_dtype, void* mean,
                         void* rstd, int M, int d, float eps, void* stream);
/* y1 = LN(x; gamma1, beta1) in f32 and y2 = LN(y1; gamma2, beta2) in y2_dtype in one pass (d = 512, 32-byte aligned pointers):
 * a ConformerLayer's norm_out followed by the next layer's norm_feed_forward1 (conformer_modules.py:205-231, :174-178) */
int mi355x_layernorm2_fwd(const void* x, const void* gamma1, const void* beta1, void* y1, void* mean1, void* rstd1,
                          const void* gamma2, const void* beta2, void* y2, int y2_dtype, void* mean2, void* rstd2, int M, int d,
                          float eps, void* stream);
/* The backward of that pair in one pass (d = 512): g = dres_in + dLN1(dy1; x1) is the gradient w.r.t. y1 (kept in registers),
 * dres_out (f32) = dLN2(g; x2), cast_out (optional bf16) = cast_scale * dropmask * dres_out; the four parameter gradients are
 * accumulated (+=).  LN1 = the LATER LayerNorm in forward order (norm_feed_forward1 of layer i+1, input x1 = layer i's output),
 * LN2 = the earlier one (norm_out of layer i, input x2). */
int mi355x_layernorm2_bwd(const void* dy1, int dy1_dtype, const void* x1, const void* gamma1, const void* mean1, const void* rstd1,
                          void* dgamma1, void* dbeta1, const void* dres_in, const void* x2, const void* gamma2, const void* mean2,
                          const void* rstd2, void* dgamma2, void* dbeta2, void* dres_out, int M, int d, void* cast_out,
                          float cast_scale, unsigned drop_key, unsigned drop_threshold, float drop_scale, void* stream);
/* dres (f32 [M,d]) = (accumulate ? dres : 0) + dLN/dx ; dgamma/dbeta (f32 [d]) are accumulated (+=).  Pass both or
 * neither (both NULL: input gradient only); exactly one of them NULL is MI_ERR_ARG.                                 */
int mi355x_layernorm_bwd(const void* dy, int dy_dtype, const void* x, int x_dtype, const void* gamma, const void* mean,
                         const void* rstd, void* dres, int accumulate, void* dgamma, void* dbeta, int M, int d, void* stream);
/* Same, and in the same pass cast_out (bf16 [M,d]) = cast_scale * dropmask * dres_new: the operand of the NEXT sub-block's
 * output-projection gradient GEMMs (the residual-branch gradient through that sub-block's dropout), which otherwise costs a
 * separate read of the fp32 gradient (mi355x_drop_scale_cast).  M*d % 8 == 0. */
int mi355x_layernorm_bwd_cast(const void* dy, int dy_dtype, const void* x, int x_dtype, const void* gamma, const void* mean,
                              const void* rstd, void* dres, int accumulate, void* dgamma, void* dbeta, int M, int d,
                              void* cast_out, float cast_scale, unsigned drop_key, unsigned drop_threshold, float drop_scale,
                              void* stream);
/* out[n] += alpha * sum_m x[m,n]  (bias / pos_bias gradients) */
int mi355x_colsum(const void* x, int x_dtype, long long ld, void* out, int M, int N, float alpha, void* stream);

/* ---- decoder log-softmax: conv_asr.py:468 ---------------------------------------------------------------------- */
int mi355x_log_softmax_fwd(const void* logits, long long ld_in, void* logp, long long ld_out, int M, int C, void* stream);
int mi355x_log_softmax_bwd(const void* dlogp, const void* logp, long long ld, void* dlogits, int out_dtype, long long ld_out,
                           int M, int C, float scale, void* stream);

/* ---- Conformer block glue (conformer_modules.py:324-331; multi_head_attention.py:259-270,305-307,343-346,137-140) */
/* row_offsets (optional, i64 [B+1], needs len): "PACKED ROWS" (length-aware kernels that skip padded frames) --
 * the [M, 2d] side (`in`, `din`) then holds only the valid frames of every utterance, utterance b at rows row_offsets[b] ..
 * row_offsets[b] + len[b] - 1, while the [M, d] side (`out`, `dout`) stays the padded [B*T, d] grid the depthwise convolution and
 * BatchNorm run on (their batch statistics include padded frames, conformer_modules.py:297,330-331).  M = B * T either way. */
int mi355x_glu_fwd(const void* in /*[M,2d]*/, void* out /*[M,d]*/, int dtype, const void* len, int T, long long M, int d,
                   const void* row_offsets, void* stream);
int mi355x_glu_bwd(const void* in, const void* dout, void* din, int dtype, const void* len, int T, long long M, int d,
                   const void* row_offsets, void* stream);
/* direction 0: packed[row_offsets[b] + t, 0:width] = padded[b*T + t, 0:width] for t < len[b];
 * direction 1: padded[b*T + t, 0:width] = t < len[b] ? packed[row_offsets[b] + t, 0:width] : 0 for every t < T.
 * M = B * T (rows of the padded grid), ld_* = row pitches in elements, width % (16 bytes / element size) == 0, dtype bf16 or f32. */
int mi355x_rows_pack(const void* src, void* dst, int dtype, long long ld_src, long long ld_dst, const void* len,
                     const void* row_offsets, int T, long long M, int width, int direction, void* stream);
int mi355x_drop_scale_cast(const void* in, int in_dtype, void* out, int out_dtype, long long n, float alpha,
                           unsigned drop_key, unsigned drop_threshold, float drop_scale, void* stream);
int mi355x_qbias(const void* qkv, long long ldq, const void* u, const void* v, void* qu, void* qv, int dtype, long long M,
                 int d, void* stream);
int mi355x_add2(const void* a, const void* b, int in_dtype, void* out, int out_dtype, long long ldo, long long M, int d,
                void* stream);
/* out[m, 0:d] = a + b (bf16, row pitch ldo) and, in the same pass, sum_ab[0:d] += column sums of a, sum_ab[d:2d] +=
 * column sums of b (f32).  Used for dq = dqu + dqv with the pos_bias_u / pos_bias_v gradients
 * (multi_head_attention.py:288-291): pos_bias_u.grad and pos_bias_v.grad must be adjacent ([2, d]).
 * scratch: f32 [ceil(M/32) * 2 * d] (two-stage reduction, no same-address atomics). */
int mi355x_add2_colsum(const void* a, const void* b, void* out, long long ldo, long long M, int d, void* sum_ab, void* scratch,
                       long long scratch_elems, void* stream);
/* ac f32 [H,B,T,Tp], bdf f32 [H,B,T,Pp] (bd before rel_shift) -> s (softmax, masked) and pd = dropout(s), pitch Tp   */
int mi355x_relpos_softmax_fwd(const void* ac, const void* bdf, void* s_out, void* pd_out, int out_dtype, const void* len,
                              int H, int B, int T, int Tp, int Pp, float scale, unsigned drop_key, unsigned drop_threshold,
                              float drop_scale, void* stream);
/* The same with a limited attention context (ConformerEncoder att_context_size = [left, right], att_context_style;
 * /root/reference/nemo/collections/asr/modules/conformer_encoder.py:794-823): ctx_style 0 = unlimited, 1 = 'regular', 2 =
 * 'chunked_limited'; a key outside the query's window is masked exactly like a padded one (multi_head_attention.py:137-146). */
int mi355x_relpos_softmax_fwd_ctx(const void* ac, const void* bdf, void* s_out, void* pd_out, int out_dtype, const void* len, int H,
                                  int B, int T, int Tp, int Pp, float scale, unsigned drop_key, unsigned drop_threshold,
                                  float drop_scale, int ctx_style, int ctx_left, int ctx_right, void* stream);
int mi355x_relpos_softmax_bwd(const void* dpd, int dpd_dtype, const void* s_in, void* dscore, void* dbdf, int s_dtype, int H,
                              int B, int T, int Tp, int Pp, float scale, unsigned drop_key, unsigned drop_threshold,
                              float drop_scale, void* stream);

/* ---- fused rel-pos attention (bf16; head width dk = 64 or 128 -- narrower / in-between heads are zero-padded inside the packed
 * weight images by the encoders: 44 -> 64, 81 -> 128): RelPositionMultiHeadAttention.forward, multi_head_attention.py:272-354.
 * qkv [B*T, ldq = 3d] (q|k|v), pos = linear_pos(pos_emb) [2T-1, ldp], bias_u/v f32 [H*d_k], len i64 [B]
 * -> ctx [B*T, ldo] bf16, lse f32 [B,H,T] (log-sum-exp of the masked scaled scores, kept for backward).
 * ctx_lo (optional, same layout as ctx): the bf16 ROUNDING RESIDUAL of ctx (O = ctx + ctx_lo to ~16 mantissa bits) for
 * mi355x_attn_delta -- the reference's softmax backward works on fp32 probabilities (multi_head_attention.py:137-138 under
 * autocast), i.e. without the error a delta taken from the rounded O alone puts on nearly-cancelling score gradients.
 * Dropout index of probability (b,h,i,j) = ((h*B+b)*T + i)*Tp + j.
 * row_offsets (optional, i64 [B+1]; every fused attention entry point takes it): PACKED ROWS -- the activation matrices (qkv, ctx,
 * ctx_lo; in backward qu, qv, dO, dqu, dqv, dq_out, dqkv) hold only the valid frames, utterance b at rows row_offsets[b] ..
 * row_offsets[b] + len[b] - 1, instead of b*T .. b*T + T - 1.  T stays the padded length: it fixes the positional geometry
 * (pos has 2T-1 rows) and the layout of the per-query statistics lse / delta [B,H,T] and of ds_out, which remain padded-indexed. */
int mi355x_relpos_flash_fwd(const void* qkv, long long ldq, const void* pos, long long ldp, const void* bias_u,
                            const void* bias_v, const void* len, void* ctx, void* ctx_lo, long long ldo, void* lse, int B, int H,
                            int T, int dk, int Tp, float scale, unsigned drop_key, unsigned drop_threshold, float drop_scale,
                            const void* row_offsets, void* stream);

/* backward of the fused attention.  delta[b,h,i] = sum_dv dO*(O + O_lo) (O_lo optional, see above).  dq kernel: qu = q+u, qv = q+v ([B*T,d] bf16, from
 * mi355x_qbias), recomputes P from lse, returns dQu and dQv ([B*T,d] bf16; dq = dQu+dQv, d pos_bias_{u,v} = column sums). */
int mi355x_attn_delta(const void* dO, const void* O, const void* O_lo, void* delta, int B, int H, int T, int d, const void* len,
                      const void* row_offsets, void* stream);
/* mi355x_attn_delta and mi355x_qbias (q = the first d columns of qkv rows of pitch ldq; multi_head_attention.py:288-291: q + pos_bias_u,
 * q + pos_bias_v) in ONE pass over the rows: everything the fused backward kernels need in front of them.  All pointers 16-byte
 * aligned, ldq % 8 == 0. */
int mi355x_attn_bwd_prep(const void* dO, const void* O, const void* O_lo, void* delta, const void* qkv, long long ldq,
                         const void* bias_u, const void* bias_v, void* qu, void* qv, int B, int H, int T, int d, const void* len,
                         const void* row_offsets, void* stream);
/* ds_out (optional): the score gradient in the layout of the reference's matrix_bd BEFORE rel_shift
 * (multi_head_attention.py:259-270), cut into 32 x 32 bf16 blocks for mi355x_relpos_flash_bwd_dpos:
 * X[h][b][it][s][q][cl] = dS[b,h, i = 32*it+q, j] at position c = T-1+j-i = T-32+32*(s-it)+cl, it < ceil(T/32), s <= ceil(T/32);
 * slots s <= ceil(len[b]/32) are written.  ds_elems = capacity of ds_out in elements, >= mi355x_relpos_ds_elems(B,H,T).
 * Outputs: dqu / dqv separately (both non-NULL), and / or dq_out = dQu + dQv as bf16 rows of pitch ld_dq (the q third of the
 * fused projection's [M, 3d] gradient) with bias_grads f32 [2 * H * 64] += column sums of dQu | dQv (d pos_bias_u | d pos_bias_v)
 * through cs_scratch, f32 [B * ceil(T / 128) * 2 * H * 64] (per-workgroup sums, added by a second-stage reduction launch). */
long long mi355x_relpos_ds_elems(int B, int H, int T);
int mi355x_relpos_flash_bwd_dq(const void* qu, const void* qv, const void* qkv, long long ldq, const void* pos, long long ldp,
                               const void* len, const void* dO, const void* lse, const void* delta, void* dqu, void* dqv,
                               void* ds_out, void* dq_out, long long ld_dq, void* bias_grads, void* cs_scratch,
                               long long cs_scratch_elems, int B, int H, int T, int dk, long long ds_elems, float scale,
                               unsigned drop_key, unsigned drop_threshold, float drop_scale, const void* row_offsets, void* stream);

/* dK and dV rows written into the k / v column blocks of dqkv [B*T, ldd = 3d] */
int mi355x_relpos_flash_bwd_dkv(const void* qu, const void* qv, const void* qkv, long long ldq, const void* pos, long long ldp,
                                const void* len, const void* dO, const void* lse, const void* delta, void* dqkv, long long ldd,
                                int B, int H, int T, int dk, int Tp, float scale, unsigned drop_key, unsigned drop_threshold,
                                float drop_scale, const void* row_offsets, void* stream);

/* SAVED PROBABILITIES (head width 64, padded rows): the forward already holds every probability in registers; exported once, the
 * two backward kernels need not rebuild S = Qu K^T, the positional band, the rel_shift and the exponentials.
 * mi355x_relpos_flash_fwd_p = mi355x_relpos_flash_fwd (ctx, ctx_lo, lse bit-identical) that also writes
 *   probs bf16 [(b*H+h)][query block it][key tile kt][lane][16]: the 32 x 32 un-normalised probabilities
 *     p~ = exp2((s - mref) * scale * log2 e) of queries 32*it .. +31 against keys 32*kt .. +31 before dropout, in the register order
 *     of the kernel: lane = (query & 31) + 32 * ((key >> 2) & 1), register r = (key & 3) + 4 * ((key & 31) >> 3); masked keys 0;
 *     both block indices run to NT4 = 4 * ceil(T / 128); key tiles kt >= ceil(len[b] / 32) are not written;
 *   mref f32 [(b*H+h)][kt][32 * NT4]: the raw-score reference point of query i in that step (the running maximum moves lazily
 *     and per query, so it travels with the tile).  P[i,j] = p~ * exp(mref * scale - lse).
 * probs_elems / mref_elems = capacities in elements, >= mi355x_relpos_probs_elems / mi355x_relpos_mref_elems (B, H, T).
 * The _p backward entry points produce what mi355x_relpos_flash_bwd_dq / _dkv produce, from probs and mref (one extra bf16 rounding
 * of each probability).  All three return MI_ERR_ARG for dk != 64, a row_offsets table or a short buffer. */
long long mi355x_relpos_probs_elems(int B, int H, int T);
long long mi355x_relpos_mref_elems(int B, int H, int T);
int mi355x_relpos_flash_fwd_p(const void* qkv, long long ldq, const void* pos, long long ldp, const void* bias_u, const void* bias_v,
                              const void* len, void* ctx, void* ctx_lo, long long ldo, void* lse, void* probs, long long probs_elems,
                              void* mref, long long mref_elems, int B, int H, int T, int dk, int Tp, float scale, unsigned drop_key,
                              unsigned drop_threshold, float drop_scale, const void* row_offsets, void* stream);
int mi355x_relpos_flash_bwd_dq_p(const void* probs, long long probs_elems, const void* mref, long long mref_elems, const void* qkv,
                                 long long ldq, const void* pos, long long ldp, const void* len, const void* dO, const void* lse,
                                 const void* delta, void* dqu, void* dqv, void* ds_out, void* dq_out, long long ld_dq,
                                 void* bias_grads, void* cs_scratch, long long cs_scratch_elems, int B, int H, int T, int dk,
                                 long long ds_elems, float scale, unsigned drop_key, unsigned drop_threshold, float drop_scale,
                                 const void* row_offsets, void* stream);
int mi355x_relpos_flash_bwd_dkv_p(const void* probs, long long probs_elems, const void* mref, long long mref_elems, const void* qu,
                                  const void* qkv, long long ldq, const void* len, const void* dO, const void* lse,
                                  const void* delta, void* dqkv, long long ldd, int B, int H, int T, int dk, float scale,
                                  unsigned drop_key, unsigned drop_threshold, float drop_scale, const void* row_offsets,
                                  void* stream);

/* dpos f32 [2T-1, ldd] += gradient w.r.t. pos = linear_pos(pos_emb) (multi_head_attention.py:296-300 backward), summed over
 * the batch: dpos[c, h, :] += sum_{b,i} dS[b,h,i,c-(T-1)+i] * qv[b,i,h,:], from the blocks written by
 * mi355x_relpos_flash_bwd_dq (ds_out).  partial (optional): f32 scratch of >= mi355x_relpos_dpos_partial_elems(B,H,T)
 * elements -> deterministic two-stage reduction instead of atomics.  dpos_cast (optional, needs `partial`): bf16 [2T-1, ldd]
 * copy of the updated dpos, written by the reduction stage (the operand of the linear_pos weight-gradient GEMM). */
long long mi355x_relpos_dpos_partial_elems(int B, int H, int T);
int mi355x_relpos_flash_bwd_dpos(const void* qv, const void* ds, const void* len, void* dpos, long long ldd, void* dpos_cast,
                                 void* partial, long long partial_elems, int B, int H, int T, int dk, long long ds_elems,
                                 const void* row_offsets, void* stream);

/* which depthwise-convolution kernels run (tests and A/B): 0 = the LDS-tile kernels (default: faster inside the training step),
 * 1 = the streaming kernel in the forward pass (bf16, k = 31, even d), 2 = in the backward pass too; level < 0 only queries.
 * Returns the previous level.
 * Environment: MI355X_DWCONV_STREAM.  (CausalConv1D depthwise, parts/submodules/conformer_modules.py:333-337) */
int mi355x_dwconv_config(int level);

/* ---- convolution module: depthwise conv + BatchNorm + Swish (conformer_modules.py:333-342, causal_convs.py:130-147) */
int mi355x_dwconv_fwd(const void* x, const void* w /*[d,1,k]*/, const void* bias, void* y, int dtype,
                      void* stats /*f64 [2,d] += (sum, sumsq) or NULL*/, int B, int T, int d, int ksize, void* stream);
/* GLU (+ pad mask) fused into the depthwise forward (conformer_modules.py:324-335: glu -> masked_fill -> depthwise_conv).  glu_in
 * [rows, 2d] = the pointwise conv's output (rows = B*T, or the packed valid frames with row_offsets i64 [B+1] as in mi355x_glu_fwd);
 * len i64 [B] (NULL: every frame valid); glu_out [B,T,d] receives the GLU output (zeros beyond len; backward's operand);
 * w, bias, y, stats as in mi355x_dwconv_fwd.  d must be a whole number of 16-byte chunks.  act: 0 = GLU as described, 1 = Swish of a
 * [rows, d] input instead (ConformerConvolution(pointwise_activation='swish'), squeezeformer_modules.py:60-203). */
int mi355x_dwconv_fwd_glu(const void* glu_in, const void* len, const void* row_offsets, void* glu_out, const void* w,
                          const void* bias, void* y, int dtype, void* stats, int B, int T, int d, int ksize, int act, void* stream);
int mi355x_dwconv_bwd(const void* dy, const void* x, const void* w, void* dx, void* dw, void* dbias, int dtype, int B, int T,
                      int d, int ksize, void* scratch /* optional f32 [4*B*(ksize+1)*d]: two-stage reduction, no atomics */,
                      long long scratch_elems, void* stream);
/* The depthwise convolution with asymmetric zero padding (ConformerConvolution's CausalConv1D, conv_context_size = [left, right] with
 * left + right + 1 = ksize; /root/reference/nemo/collections/asr/parts/submodules/causal_convs.py:89-150, conformer_modules.py:
 * 310-321): pad_left frames in front of the sequence, ksize - 1 - pad_left behind it; -1 = symmetric. */
int mi355x_dwconv_fwd_ctx(const void* x, const void* w, const void* bias, void* y, int dtype, void* stats, int B, int T, int d,
                          int ksize, int pad_left, void* stream);
int mi355x_dwconv_bwd_ctx(const void* dy, const void* x, const void* w, void* dx, void* dw, void* dbias, int dtype, int B, int T, int d,
                          int ksize, int pad_left, void* scratch, long long scratch_elems, void* stream);
int mi355x_bn_finalize(const void* stats, double count, void* mean, void* rstd, void* running_mean, void* running_var,
                       float momentum, float eps, int d, void* stream);
/* same, the element count read from device memory (f64 scalar): under SyncBatchNorm (conformer_ctc_bpe.yaml:209,
 * torch.nn.SyncBatchNorm gathers the per-rank counts) it is all-reduced together with the sums */
int mi355x_bn_finalize_dev_count(const void* stats, const void* count_dev, void* mean, void* rstd, void* running_mean,
                                 void* running_var, float momentum, float eps, int d, void* stream);
int mi355x_bn_eval_stats(const void* running_mean, const void* running_var, void* mean, void* rstd, float eps, int d,
                         void* stream);
int mi355x_bn_swish_fwd(const void* x, const void* mean, const void* rstd, const void* gamma, const void* beta, void* y,
                        int dtype, long long M, int d, void* stream);
/* training forward in one launch (nn.BatchNorm1d in training mode + Swish, conformer_modules.py:339-342): mean / rstd from the f64
 * sums (as mi355x_bn_finalize: `count` positions, or the count read from device memory when count_dev != NULL), written out for
 * backward, running statistics updated, y = swish(BN(x)).  Measured slower than mi355x_bn_finalize + mi355x_bn_swish_fwd at the
 * Large shape (every workgroup derives its channels' coefficients; tools/bn_bench.py) -- the encoders use the pair. */
int mi355x_bn_stats_swish_fwd(const void* x, const void* stats, double count, const void* count_dev, const void* gamma,
                              const void* beta, void* y, void* mean, void* rstd, void* running_mean, void* running_var,
                              float momentum, float eps, int dtype, long long M, int d, void* stream);
/* dgamma / dbeta (optional, both or neither): f32 [d] += the parameter gradients, i.e. the LOCAL sums of this call (what
 * mi355x_bn_param_grad adds when sums started from zero), with or without scratch.  dy, x, mean, rstd, gamma, beta and sums are all
 * required: a NULL one returns MI_ERR_ARG (1) before anything is launched. */
int mi355x_bn_swish_bwd_reduce(const void* dy, const void* x, const void* mean, const void* rstd, const void* gamma,
                               const void* beta, void* sums /*f64 [2,d] +=*/, void* dgamma, void* dbeta, int dtype, long long M,
                               int d, void* scratch /* optional f32 [ceil(M/32)*2*d]: two-stage reduction */,
                               long long scratch_elems, void* stream);
/* dx = gamma * rstd * (dz - sums[0] / count - xhat * sums[1] / count), dz = dy * swish'(gamma * xhat + beta); training == 0 (eval mode)
 * drops the two mean terms and never reads what `sums` points to.  Every pointer is required (sums included, in both modes): a NULL
 * one returns MI_ERR_ARG (1) before anything is launched. */
int mi355x_bn_swish_bwd_apply(const void* dy, const void* x, const void* mean, const void* rstd, const void* gamma,
                              const void* beta, const void* sums, double count, int training, void* dx, int dtype,
                              long long M, int d, void* stream);
int mi355x_bn_swish_bwd_apply_dev_count(const void* dy, const void* x, const void* mean, const void* rstd, const void* gamma,
                                        const void* beta, const void* sums, const void* count_dev, int training, void* dx,
                                        int dtype, long long M, int d, void* stream);
/* BatchNorm + Swish backward fused into the depthwise backward (the [B,T,d] gradient between mi355x_bn_swish_bwd_apply and
 * mi355x_dwconv_bwd is never materialised; same results, the intermediate rounded to the activation type as the two-launch form
 * rounds it).  dy = gradient w.r.t. the Swish output, cc = BatchNorm input (the depthwise conv's output), sums = f64 [2][d] left by
 * mi355x_bn_swish_bwd_reduce (all-reduced under SyncBatchNorm), count > 0 or count_dev (device f64).  x, w, dx, dw, dbias, scratch
 * as in mi355x_dwconv_bwd.  Optionally the GLU backward on the way out as well (glu_in != NULL: [rows, 2d] input of the GLU,
 * glu_din [rows, 2d] receives its gradient INSTEAD of dx; glu_len i64 [B] valid frames, zeros beyond them; glu_row_offsets i64 [B+1]:
 * glu_in / glu_din hold packed rows -- mi355x_glu_bwd's semantics; glu_act 1: Swish backward of a [rows, d] input instead,
 * mi355x_swish_mask_bwd's semantics).  Replaces conformer_modules.py:333-342 backward
 * (glu -> depthwise_conv -> batch_norm -> activation, walked backwards). */
int mi355x_dwconv_bwd_bnswish(const void* dy, const void* cc, const void* mean, const void* rstd, const void* gamma,
                              const void* beta, const void* sums, double count, const void* count_dev, int training, const void* x,
                              const void* w, void* dx, void* dw, void* dbias, const void* glu_in, void* glu_din, const void* glu_len,
                              const void* glu_row_offsets, int glu_act, int dtype, int B, int T, int d, int ksize, void* scratch,
                              long long scratch_elems, int defer_tap_reduce, void* stream);
/* defer_tap_reduce != 0 above: the kernel leaves the B * 4 partial slabs of the tap / bias gradients in `scratch` (which then has to
 * be the caller's own per layer) and THIS call adds them into dw [d, 1, k] / dbias [d] -- on whichever stream the caller likes:
 * only the optimizer reads them (depthwise_conv.weight.grad, conformer_modules.py:333). */
int mi355x_dwconv_tap_reduce(const void* scratch, long long scratch_elems, int B, int d, int ksize, void* dw, void* dbias,
                             void* stream);
int mi355x_bn_param_grad(const void* sums, void* dgamma, void* dbeta, int d, void* stream);

/* ---- CTC loss: CTCLoss.forward, losses/ctc.py:68-82 (torch ctc_loss, blank = V, zero_infinity) ------------------
 * logp f32 [B,Tmax,C]; targets i64 [B,Umax]; workspaces f32 [B,Tmax,2*Umax+1] each; nll f32 [B];
 * grad f32 [B,Tmax,C] = grad_scale * d(sum_b nll_b)/d logp  (may be NULL for loss only).                          */
int mi355x_ctc_loss(const void* logp, const void* targets, const void* in_len, const void* tgt_len, void* alpha_ws,
                    void* beta_ws, void* nll, void* grad, int B, int Tmax, int C, int Umax, int blank, float grad_scale,
                    int zero_infinity, void* stream);
/* lattice kernel of mi355x_ctc_loss: 1 (default; MI355X_CTC_WAVE) = alpha / beta rows resident in the registers of one wave each
 * (2U+1 <= 1024 states, no barrier per time-step), 0 = the LDS / barrier form for every size.  Returns the previous setting
 * (-1: not yet resolved from the environment). */
int mi355x_ctc_config(int wave);

/* x[r,:] *= vec[r] (f32): per-utterance upstream gradient applied to the CTC gradient (autograd of losses/ctc.py:52-66) */
int mi355x_row_scale(void* x, const void* vec, long long rows, long long cols, void* stream);

/* ---- optimizer / weight packing (modelPT.py:650-823 AdamW; no reference analogue for packing) ------------------ */
int mi355x_adamw_step(void* params, const void* grads, void* exp_avg, void* exp_avg_sq, long long n, float lr, float beta1,
                      float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);
/* AdamW with (a) an optional DEVICE scalar clip_coef[0] multiplied into the gradient -- global-norm clipping
 * (trainer.gradient_clip_val -> torch.nn.utils.clip_grad_norm_) without a host sync -- and (b) an optional EMA of the
 * weights updated in the same pass: ema = decay*ema + (1-decay)*w_new (nemo/collections/common/callbacks/ema.py:150-157). */
int mi355x_adamw_step_ex(void* params, const void* grads, void* exp_avg, void* exp_avg_sq, long long n, float lr, float beta1,
                         float beta2, float eps, float weight_decay, int step, float grad_scale, const void* clip_coef,
                         void* ema, float ema_decay, void* stream);
/* out_f64[0] += sum(grads^2) ; coef[0] = min(1, max_norm / (scale*sqrt(sum_i sumsq[i]) + 1e-6)), coef[1] = the norm */
int mi355x_grad_sumsq(const void* grads, long long n, void* out_f64, void* stream);
int mi355x_clip_coef(const void* sumsq_f64, int nbuf, float scale, float max_norm, void* coef_f32x2, void* stream);
typedef struct mi355x_pack_entry {
  const void* src; void* dst;       /* src f32; dst[r*pitch + c] = src[r1*sr1 + r2*sr2 + c1*sc1 + c2*sc2]              */
  int rows, cols, nr2, nc2;         /* r = r1*nr2 + r2 ; c = c1*nc2 + c2                                              */
  long long sr1, sr2, sc1, sc2, pitch;
  long long tile_begin;             /* exclusive prefix sum of ceil(rows/64)*ceil(cols/64); dst 16-B aligned           */
} mi355x_pack_entry;
int mi355x_pack_weights(const void* table_dev, int n_entries, long long total_tiles, int out_dtype, void* stream);
int mi355x_fill_f32(void* p, long long n, float value, void* stream);

/* library / build information */
const char* mi355x_asr_version(void);

/* Replayable launch sequences (the reference's analogue: nemo/utils/callbacks/cuda_graph.py:251, whole-step CUDA-graph capture).
 * A training step captured into a hipGraph freezes every kernel argument, including the dropout keys (drop_key above is a
 * by-value argument).  With a step word registered here, every kernel that takes a dropout key adds *dev_word (u32, device
 * memory) to the key at entry; the host advances the word once per step in front of the forward graph, so forward and
 * backward of one step regenerate the same masks and consecutive steps different ones.  The pointer is read when a launch is
 * ISSUED (it becomes a kernel argument): set it around the capture, reset it to NULL afterwards; launches issued with NULL
 * use their key as passed.  Process-wide. */
int mi355x_set_step_counter(const void* dev_word);
/* Measurement switch: with on = 1 every launch site of the library issues an EMPTY kernel on its stream instead of its own kernel
 * (results are garbage): the host pays the per-launch cost of a step while the GPU stays idle, i.e. the pure issue time of the
 * launch sequence (tools/host_phases.py).  Returns the previous value. */
int mi355x_set_null_launch(int on);

/* Launch tapes (csrc/tape.hip): a launch sequence captured as a hipGraph, re-issued as LIVE launches from one C loop.
 * What it replaces: the host-side walk over the encoder's modules -- nemo/collections/asr/modules/conformer_encoder.py:593-759
 * (forward_internal: pre_encode, pos_enc, the layer loop) and parts/submodules/conformer_modules.py:164-215 (one layer) -- once
 * a (shape, configuration) has been seen; the reference's own mechanism for the same cost is whole-step CUDA-graph capture
 * (nemo/utils/callbacks/cuda_graph.py:251).  A replayed hipGraph measured 3-4 % slower on the device than live launches on
 * this stack, the Python sequencer costs ~19 us of host time per launch: a tape issues the graph's nodes (kernels with
 * their frozen arguments, memsets, memcpys) in topological order with hipLaunchKernel on stream lanes -- lane 0 is the
 * stream passed to replay, lanes 1.. are the OTHER streams that took part in the capture (the weight-gradient side stream),
 * used again as they are -- with one event per cross-lane dependency.
 *   mi355x_tape_log_begin(origin)  before the capture starts: from here on every launch of the library notes the stream it is
 *                                  captured on (`origin` = the capturing stream -> lane 0; other streams -> lanes 1, 2, ...)
 *   mi355x_tape_from_graph         hip_graph = hipGraph_t (kept alive by the caller for as long as the tape is used: the kernel
 *                                  arguments stay inside its nodes); returns 0, 1 (bad argument), 2 (a node type a tape cannot
 *                                  re-issue, or arguments passed through `extra`: keep replaying the graph) or 1000 + hipError_t
 *   mi355x_tape_log_end()          after the last mi355x_tape_from_graph of the capture
 *   mi355x_tape_replay(t, s, join) join = 1: the ordering contract of hipGraphLaunch(exec, s) (s continues behind every lane);
 *                                  join = 0: the side lanes run on, as behind the live sequencer -- consumers of their results
 *                                  order themselves behind those streams (the optimizer slice / gradient bucket of a layer does)
 *   mi355x_tape_join(t, s)         s continues behind whatever t's side lanes hold now (what a replay with join = 0 left out)
 *   mi355x_tape_info               counts[6] = kernels, memsets, memcpys, empty nodes, lanes, cross-lane events */
/* A stream that belongs to its caller alone (non-blocking, HIP priority clamped to the device's range: 0 = default, negative =
 * more urgent).  torch.cuda.Stream() objects come out of a 32-entry round-robin pool and are SHARED once a process has created
 * more than 32: a capture stream, a weight-gradient stream and a copy stream must not be the same stream (csrc/tape.hip). */
int mi355x_stream_create(int priority, void** out_stream);
int mi355x_stream_destroy(void* stream);
typedef struct mi355x_tape mi355x_tape;
int mi355x_tape_log_begin(void* origin_stream);
int mi355x_tape_log_end(void);
int mi355x_tape_from_graph(void* hip_graph, int max_lanes, mi355x_tape** out);
int mi355x_tape_replay(mi355x_tape* tape, void* stream, int join);
int mi355x_tape_join(mi355x_tape* tape, void* stream);
int mi355x_tape_info(const mi355x_tape* tape, int* counts);
void mi355x_tape_destroy(mi355x_tape* tape);

/* Statistics mailbox (csrc/mailbox.hip): the SyncBatchNorm exchanges as ONE kernel launch each instead of a process-group
 * all_reduce.  What it replaces: the per-layer all_reduce of torch.nn.SyncBatchNorm (`trainer.sync_batchnorm: true`,
 * examples/asr/conf/conformer/conformer_ctc_bpe.yaml:209, over the BatchNorm1d of parts/submodules/conformer_modules.py:339 and
 * its backward) -- 36 latency-bound 8-KB collectives per Conformer-CTC-Large step that otherwise queue on the same RCCL stream
 * as the 64-MiB gradient buckets.  Every rank owns a mailbox in its HBM and maps its peers' through hipIpc handles; an exchange
 * stores the rank's n f64 values into every peer's mailbox (peer stores over xGMI), raises a sequence flag, waits for the `world`
 * flags in its own mailbox and sums the boxes in rank order (every rank gets bit-identical sums).  The sequence number lives
 * in device memory: a launch carries no per-call host state.
 *   mi355x_mailbox_create   collective in spirit (every rank creates one, same world / n_max): allocates + zeroes the mailbox and
 *                           writes its MI355X_MAILBOX_HANDLE_BYTES-byte IPC handle to handle_out -- the caller carries the handles
 *                           to the peers (torch.distributed.all_gather in nemo_amd/mailbox.py).  timeout_ms <= 0: 2000.
 *                           mem_kind: 0 = the first kind of memory that can be exported (uncached, fine-grained, plain), 1 | 2 | 3 = that one.
 *   mi355x_mailbox_open     map peer `peer`'s mailbox from its handle (peer == rank: no-op)
 *   mi355x_mailbox_exchange stats (f64 [n], n <= n_max, device memory) <- sum over ranks, in place, on `stream`
 *   mi355x_mailbox_status   out3 = {exchanges completed, 0 or 1 + the rank whose flag never arrived (latched: the exchange that timed
 *                           out and every later one return at once with `stats` set to NaN -- never the local sums -- and the
 *                           sequence number does not advance), kind of memory (1 uncached, 2 fine-grained, 3 plain)};
 *                           blocking copy -- diagnostics and tests
 *   mi355x_mailbox_poll     the same header WITHOUT blocking, for the training loop (once per optimizer step): enqueues a 16-byte
 *                           copy to pinned host memory on `stream` and reports what the previous poll's copy brought back;
 *                           out4 = {exchanges completed, latch, kind of memory, 1 if the values are new since the last call}
 * Returns 0, 1 (bad argument / a peer not opened), 2 (no memory of any kind) or 1000 + hipError_t. */
#define MI355X_MAILBOX_HANDLE_BYTES 64
typedef struct mi355x_mailbox mi355x_mailbox;
int mi355x_mailbox_create(int world, int rank, int n_max, int timeout_ms, int mem_kind, mi355x_mailbox** out, void* handle_out);
int mi355x_mailbox_open(mi355x_mailbox* mb, int peer, const void* handle);
int mi355x_mailbox_exchange(mi355x_mailbox* mb, void* stats_f64, int n, void* stream);
int mi355x_mailbox_status(mi355x_mailbox* mb, long long* out3);
int mi355x_mailbox_poll(mi355x_mailbox* mb, void* stream, long long* out4);
void mi355x_mailbox_destroy(mi355x_mailbox* mb);

/* Greedy CTC decoding on the device (GreedyCTCInfer._greedy_decode_logprobs, parts/submodules/ctc_greedy_decoding.py:333-361,
 * + the CTC collapse of AbstractCTCDecoding.decode_hypothesis, parts/submodules/ctc_decoding.py:545-575):
 * logp f32 [B,T,C], lens i64 [B] (NULL = T) -> tokens i32 [B,T] (folded, blank-free, -1 padded), out_len i32 [B],
 * score f32 [B] = sum of the arg-max log-probs of the non-blank frames. */
int mi355x_ctc_greedy_decode(const void* logp, const void* lens, void* tokens, void* out_len, void* score, int B, int T, int C,
                             int blank, void* stream);
/* same, and the frames behind every kept token: tok_start / tok_end i32 [B,T] (-1 padded) = the first / last frame of the run of
 * equal arg-max labels that produced the token (the char offsets of AbstractCTCDecoding._compute_offsets, ctc_decoding.py).
 * tokens, out_len and score are bit-identical to mi355x_ctc_greedy_decode's.  blank in [0, C). */
int mi355x_ctc_greedy_decode_ts(const void* logp, const void* lens, void* tokens, void* out_len, void* score, void* tok_start,
                                void* tok_end, int B, int T, int C, int blank, void* stream);

/* ---- confidence of a decoding step (the entropy-based measures of the reference's ConfidenceMethodConfig, parts/utils/
 * asr_confidence_utils.py), normalised so that a one-hot distribution gives 1 and the uniform one 0; nothing is clamped.  For a
 * distribution over V >= 2 classes with natural log-probabilities x_v, p_v = exp(x_v), S = sum_v p_v^alpha and
 * G = sum_v p_v^alpha * x_v (a class with x_v = -inf adds 0 to both), alpha > 0:
 *   method                    norm = LIN                            norm = EXP
 *   MAX_PROB (norm ignored)   (V max_v p_v - 1) / (V - 1)           same
 *   GIBBS, alpha = 1          1 + G / ln V                          (V exp(G) - 1) / (V - 1)
 *   GIBBS, alpha != 1         1 + G / (V^(1-alpha) ln V)            (exp(alpha G) - b) / (1 - b),  b = exp(-alpha V^(1-alpha) ln V)
 *   TSALLIS, alpha != 1       1 + (1 - S) / (V^(1-alpha) - 1)       (exp((S-1)/(alpha-1)) - b) / (1 - b),  b = exp((V^(1-alpha) - 1)/(alpha-1))
 *   RENYI, alpha != 1         1 + ln S / ((alpha-1) ln V)           (V S^(1/(alpha-1)) - 1) / (V - 1)
 * TSALLIS / RENYI with alpha == 1 exactly are the GIBBS alpha = 1 row.  The constants that depend on (V, alpha) alone come from the
 * caller, computed in double: k0 = ln V, k1 = V^(1-alpha), k2 = b of the row in use (0 where the row has none). */
#define MI355X_CONF_MAX_PROB 0   /* method */
#define MI355X_CONF_GIBBS 1
#define MI355X_CONF_TSALLIS 2
#define MI355X_CONF_RENYI 3
#define MI355X_CONF_NORM_LIN 0   /* entropy_norm */
#define MI355X_CONF_NORM_EXP 1
#define MI355X_CONF_AGG_MEAN 0   /* aggregation of frame confidences into a token's */
#define MI355X_CONF_AGG_MIN 1
#define MI355X_CONF_AGG_MAX 2
#define MI355X_CONF_AGG_PROD 3
/* mi355x_ctc_greedy_decode_ts, and confidences (distribution = all C columns of a frame, blank included): frame_conf f32 [B,T]
 * (0.0 beyond lens[b]) and tok_conf f32 [B,T] (0.0 beyond out_len[b]) = `aggregation` of frame_conf over tok_start .. tok_end
 * (exclude_blank != 0), or over previous token's tok_end + 1 .. tok_end (exclude_blank == 0; the first token from frame 0: the blank
 * frames in front of a token count, the frames behind the last token belong to none).  tokens, out_len, score, tok_start and
 * tok_end are bit-identical to mi355x_ctc_greedy_decode_ts's.  MI_ERR_ARG for C < 2, alpha <= 0, unknown enum values, a null
 * output. */
int mi355x_ctc_greedy_decode_conf(const void* logp, const void* lens, void* tokens, void* out_len, void* score, void* tok_start,
                                  void* tok_end, void* frame_conf, void* tok_conf, int B, int T, int C, int blank, int method,
                                  int norm, float alpha, float k0, float k1, float k2, int aggregation, int exclude_blank,
                                  void* stream);

/* CTC forced alignment: the Viterbi pass of the reference's forced aligner (tools/nemo_forced_aligner/utils/viterbi_decoding.py),
 * one launch per batch -- forward walk, backtrace and expansion.  logp f32 [B,Tmax,C] (-inf entries allowed); targets i64 [B,Umax];
 * in_len, tgt_len i64 [B].  States = the blank-extended sequence, S = 2U+1:
 *   v[0][0] = e(0,0), v[0][1] = e(0,1);  v[t][s] = max(v[t-1][s], v[t-1][s-1], v[t-1][s-2] if allowed) + e(t,s)
 * (skip only into a label state whose label differs from the one two states back), plain float32 natural-log arithmetic, so score
 * and path are bit-equal to a float32 restatement.  Ties: the first maximum in the order (stay, s-1, s-2); at the last frame state
 * S-1 unless v[S-2] > v[S-1].
 *   path      i32 [B,Tmax]  state index 0..2U for t < T, -1 beyond
 *   tok_start i32 [B,Umax]  first / last frame spent in state 2u+1; -1 for u >= U
 *   tok_end   i32 [B,Umax]
 *   score     f32 [B]       log-probability of the best path; -inf = infeasible (T < U + adjacent repeats, T <= 0 < U, or -inf
 *                           emissions on every path): path, tok_start, tok_end are then all -1.  T = 0 and U = 0: score 0.
 *   bp_ws     backpointer workspace, 8-byte aligned, B * Tmax * ((Umax + 8) & ~7) bytes: one byte per (blank, label) pair g and
 *             frame, bits 0-1 = predecessor choice of state 2g, bits 2-3 = of state 2g+1 (0 stay, 1 s-1, 2 s-2), rows padded to 8
 * 1 <= Umax <= 2048 (S <= 4097); MI_ERR_ARG otherwise, and for null pointers, non-positive sizes, blank outside [0, C). */
int mi355x_ctc_align(const void* logp, const void* targets, const void* in_len, const void* tgt_len, void* bp_ws, void* path,
                     void* tok_start, void* tok_end, void* score, int B, int Tmax, int C, int Umax, int blank, void* stream);
/* forward walk of mi355x_ctc_align: 1 (default; MI355X_CTC_ALIGN_WAVE) = lattice row resident in the registers of one wave where
 * 2*Umax+1 <= 1024, 0 = the LDS / barrier form for every size.  Returns the previous setting (-1: not yet resolved). */
int mi355x_ctc_align_config(int wave);

/* CTC prefix beam search (the `beam_batch` strategy), one launch per batch, utterances independent.  This entry runs without a
 * language model; mi355x_ctc_beam_decode_lm below is the same search with an n-gram model fused.
 * logp f32 [B,Tmax,C] log-probabilities (-inf entries allowed; rows beyond lens[b] are never read); lens i64 [B].
 * A beam = a prefix (a node (parent node, token) of a prefix tree), its length len, pb / pnb = log-probability of its alignments
 * that end in blank / in a non-blank, tot = logaddexp(pb, pnb).  Start: the empty prefix, pb = 0, pnb = -inf.  Per frame t:
 *   1. mx = max_c lp[t,c]; class c (blank included) is considered iff lp[t,c] >= mx - threshold (float32 subtract and compare)
 *   2. for every beam i with last token l_i (none for the empty prefix) and every considered c:
 *        c == blank : stay(i).pb  (+)= tot_i + lp[c]
 *        c == l_i   : stay(i).pnb (+)= pnb_i + lp[c]   and   ext(i,c).pnb (+)= pb_i + lp[c]
 *        otherwise  : ext(i,c).pnb (+)= tot_i + lp[c]                                   ((+) = log-add-exp)
 *   3. ext(i,c) IS stay(j) where beam j of the set holds the prefix of i followed by c: one candidate, contributions merged
 *   4. candidates with tot = -inf are dropped; the new set = the `beam` candidates of the largest rank = tot + beta * len.
 *      Order: (rank descending, key ascending), key = i for stay(i), beam + i*C + c for ext(i,c), i = slot of the beam in the
 *      ordered set of the previous frame -- a total order, so ties of rank are decided the same way on every run
 *   5. a kept extension in slot s becomes node 1 + t*beam + s (node 0 = the empty prefix) and stores (parent, token) at
 *      node_ws[2*(t*beam + s)]; a stay keeps its node.  The frame a token was created in is (node - 1) / beam.
 * Plain float32: logaddexp(a,b) = max + log1pf(expf(-|a-b|)), -inf handled; beta * len is rounded before it is added.
 *   tokens    i32 [B,beam,Tmax]  hypotheses in order, best first; -1 padded
 *   tok_frame i32 [B,beam,Tmax]  frame at which each token's node was created; -1 padded
 *   hyp_len   i32 [B,beam]       0 for absent hypotheses
 *   score     f32 [B,beam]       rank; -inf for absent hypotheses
 *   n_hyp     i32 [B]            number of hypotheses (< beam when the utterance is short); lens[b] = 0: one empty hypothesis, score 0
 *   node_ws   i32, 8-byte aligned, B * mi355x_ctc_beam_workspace_elems(Tmax, beam) elements (= 2 * Tmax * beam per utterance)
 * MI_ERR_ARG for null pointers, non-positive sizes, beam outside 1..64, blank outside [0, C), threshold <= 0 or NaN (+inf = no
 * pruning), NaN beta, C > 8192 (two rows of C floats in LDS; nothing in LDS grows with beam). */
int mi355x_ctc_beam_decode(const void* logp, const void* lens, void* node_ws, void* tokens, void* tok_frame, void* hyp_len,
                           void* score, void* n_hyp, int B, int Tmax, int C, int blank, int beam, float threshold, float beta,
                           void* stream);
/* i32 elements of node_ws per utterance; 0 for arguments mi355x_ctc_beam_decode rejects */
long long mi355x_ctc_beam_workspace_elems(int Tmax, int beam);

/* The search of mi355x_ctc_beam_decode with shallow fusion of a token-level back-off n-gram language model.
 * The model, of order N, gives ln p(c | context) for the labels c = 0 .. V-1, V = C-1 (so blank = C-1); the context is the last N-1
 * tokens of <s> followed by the prefix.  The value is the ARPA definition: the probability of the n-gram ctx.c where the file has
 * it, else backoff(ctx) + ln p(c | ctx[1:]) with backoff(ctx) = 0 for a ctx that is not in the file; the recursion ends at the
 * unigrams, which exist for every label.  File values are log10: the tables hold float32(float64(value) * ln 10).
 * lm(prefix) = the sum of the conditional log-probabilities of its tokens, lm(()) = 0; no </s> term is ever added.  lm is a function
 * of the prefix alone, so a stay and an extension that name the same prefix still are one candidate.
 * The search changes in the rank only:  rank = (tot + beta * len) + alpha * lm(prefix),  float32, in that association, each product
 * rounded before it is added.  Token pruning (acoustic only), pb / pnb, merging, the order of ties, the node tree and all outputs
 * are what they are above; `score` is the rank, so it includes alpha * lm.  alpha = 0 gives the bits of mi355x_ctc_beam_decode.
 * The model as a back-off automaton (S = n_states, A = n_arcs), all arrays on the device:
 *   state_arc_begin i32 [S+1]  the arcs of state s are [state_arc_begin[s], state_arc_begin[s+1]); a state = a context the file
 *                              holds as an n-gram of order < N; state 0 = the empty context, state 1 = <s>
 *   arc_tok  i32 [A]           the label of an arc, ascending inside a state; state 0 has exactly V arcs and arc c is label c
 *   arc_logp f32 [A]           ln p(label | the state's context)
 *   arc_next i32 [A]           the state of the longest suffix of context.label that is a state
 *   state_bo f32 [S]           the back-off weight (ln) of the state's context
 *   state_bo_next i32 [S]      the state of the longest proper suffix of the context that is a state (0 for one-token contexts)
 * A look-up of c in state s:  acc = 0; while c is not among the arcs of s: acc += state_bo[s], s = state_bo_next[s];
 * value = acc + arc_logp, next state = arc_next.  lm(prefix.c) = lm(prefix) + value, float32.
 * lm_ub: an upper bound of every look-up's value (what cannot beat the kept set is skipped by it; a looser bound only skips less).
 * The kernel bounds every chase (a back-off chain by S steps, a binary search by 32) and clamps every index to its table: tables
 * that break the rules above give a wrong score, never a hang.
 * MI_ERR_ARG for what mi355x_ctc_beam_decode refuses and for null tables, n_states < 2, n_arcs < C-1, blank != C-1, alpha < 0 or
 * NaN, NaN lm_ub. */
int mi355x_ctc_beam_decode_lm(const void* logp, const void* lens, void* node_ws, void* tokens, void* tok_frame, void* hyp_len,
                              void* score, void* n_hyp, int B, int Tmax, int C, int blank, int beam, float threshold, float beta,
                              const void* state_arc_begin, const void* arc_tok, const void* arc_logp, const void* arc_next,
                              const void* state_bo, const void* state_bo_next, int n_states, int n_arcs, float alpha, float lm_ub,
                              void* stream);

/* ---- resumable CTC prefix beam search (cache-aware streaming).  The two searches above, started from a per-utterance beam state
 * and returning the next one, so that a stream searched chunk by chunk gives bit-identical hypotheses, frames, lengths and scores
 * to one launch over all of its frames, for ANY cut into chunks: a frame does the same float32 operations in the same order.
 * State (device arrays, written out of place: state_out must not alias state_in; the same state_in stepped twice gives the same
 * result).  Per slot s < beam, [B, beam], slot order = the order of the set (ties of the next frame are broken by it):
 *   node, par, tok, len   i32   the beam's node, its parent node, its last token, its length       fresh stream: 0, -1, -1, 0
 *   h, hp                 u64   hash of the prefix and of the parent's prefix                       the root hash, 0
 *   pb, pnb, tot, brank   f32   as above; brank = the rank the slot was kept with (= its score)     slot 0: 0, -inf, 0, 0; else -inf
 *   lm_state, lm_sum      i32, f32   LM search only (may be NULL otherwise): automaton state, lm(prefix)            1 (<s>), 0
 * Per utterance, [B]:
 *   nb            i32   live beams; slots >= nb are not read                                                                     1
 *   frames_done   i32   frames consumed by earlier steps                                                                         0
 * state_in NULL, or state_in->node NULL: every stream is fresh (the one-shot search's initial values).  state_out is required.
 * The prefix tree persists: node_ws is i32 pairs [B, Tcap, beam] (8-byte aligned), owned by the caller, appended to in place; the
 * utterance's base is b * Tcap * beam pairs.  The extension kept in slot s of frame t of THIS chunk becomes node
 * 1 + (frames_done + t) * beam + s, stored at pair (frames_done + t) * beam + s, so (node - 1) / beam is the GLOBAL frame of the
 * token; merging and the output walk nodes that earlier launches wrote.  Replaying a chunk from the same state_in rewrites the same
 * pairs with the same values; two different continuations of one state need two trees.
 * logp f32 [B,Tmax,C] and lens i64 [B] describe this chunk.  Capacity: the step consumes min(lens[b], Tmax, Tcap - frames_done[b])
 * frames and writes frames_done + consumed; it never stores past the tree or the outputs whatever the state holds (frames_done, nb
 * and len are clamped to their ranges, node ids beyond Tcap * beam are not followed).  lens[b] = 0: the state passes through.
 * Outputs: the current n-best, chased out of the tree as above, tokens / tok_frame i32 [B,beam,Tcap] (tok_frame: global frames).
 * Positions at or beyond hyp_len[b,k] are NOT written (padding [B,beam,Tcap] on every chunk would cost more than the search):
 * slice by hyp_len.  hyp_len, score, n_hyp as above.  All five outputs NULL: the state advances and nothing is chased.
 * MI_ERR_ARG for what the one-shot entry refuses (with the five outputs all present or all NULL), a null state_out, a state (in
 * with a non-null node, or out) with a null array (lm_state / lm_sum: in the LM search only), state_out->node == state_in->node,
 * Tcap < 1, Tcap * beam > 0x3fffffff (node ids are 32-bit). */
typedef struct mi355x_ctc_beam_stream_state {
  int* node; int* par; int* tok; int* len; unsigned long long* h; unsigned long long* hp;
  float* pb; float* pnb; float* tot; float* brank; int* lm_state; float* lm_sum; int* nb; int* frames_done;
} mi355x_ctc_beam_stream_state;
int mi355x_ctc_beam_decode_stream(const void* logp, const void* lens, void* node_ws, void* tokens, void* tok_frame, void* hyp_len,
                                  void* score, void* n_hyp, int B, int Tmax, int C, int blank, int beam, float threshold,
                                  float beta, int Tcap, const mi355x_ctc_beam_stream_state* state_in,
                                  const mi355x_ctc_beam_stream_state* state_out, void* stream);
int mi355x_ctc_beam_decode_lm_stream(const void* logp, const void* lens, void* node_ws, void* tokens, void* tok_frame,
                                     void* hyp_len, void* score, void* n_hyp, int B, int Tmax, int C, int blank, int beam,
                                     float threshold, float beta, const void* state_arc_begin, const void* arc_tok,
                                     const void* arc_logp, const void* arc_next, const void* state_bo, const void* state_bo_next,
                                     int n_states, int n_arcs, float alpha, float lm_ub, int Tcap,
                                     const mi355x_ctc_beam_stream_state* state_in,
                                     const mi355x_ctc_beam_stream_state* state_out, void* stream);

/* ---- the search with one or two fusion models, and phrase boosting (context biasing).  A fusion model is a back-off automaton of
 * the six tables above with its weight `alpha` >= 0, the upper bound `ub` of a look-up's value (lm_ub above) and, optionally, a
 * seventh table:
 *   state_final f32 [S]   what alpha multiplies and the OUTPUT adds to a hypothesis that ends in state s (NULL: nothing)
 * With models m1 (and m2) the search above changes in the rank only:
 *   rank = ((tot + beta * len) + alpha1 * m1(prefix)) + alpha2 * m2(prefix),   float32, in that association, each product rounded
 * before it is added; m(prefix) is the running float32 sum of the look-ups as lm(prefix) is above.  Each model has its own state
 * and sum per beam.  At output -- the end of the one-shot search, every emitting step of the resumable one -- a hypothesis' score is
 *   (rank + alpha1 * state_final1[state1]) + alpha2 * state_final2[state2]     (a term only where the table is given)
 * and the n-best is ordered by that score, descending, ties by the hypothesis' slot in the search order, ascending.  The state a
 * resumable step writes holds the search's order and ranks, not the final ones, so any cut into chunks gives the bits of one launch.
 * An n-gram model: the six tables, state_final NULL.  One n-gram model alone gives the bits of mi355x_ctc_beam_decode_lm.
 * A boosting tree (modules/boosting_tree.py builds it) is the Aho-Corasick automaton of a set P of key phrases (non-empty token
 * sequences) in the same six tables: trie children are the arcs, the failure link is the back-off.  With context_score cs > 0 and
 * depth_scaling ds > 0 the k-th token of a phrase is worth ts(k) = cs (k = 1) or cs * ds (k > 1); part(m) = ts(1) + .. + ts(m),
 * full(p) = part(|p|).  For a prefix y:
 *   complete(y) = the sum of full(p) over every occurrence of a phrase p of P as a contiguous run of y (every end position;
 *                 overlapping and nested occurrences all count)
 *   pending(y)  = part(m), m = the length of the longest suffix of y that is a prefix of a phrase (a whole phrase counts), 0 if none
 *   inside the search   boost(y) = complete(y) + pending(y)          returned   boost_final(y) = complete(y)
 * so a phrase is paid for token by token while it is being spelled, the payment is taken back when the spelling fails, and a
 * phrase begun and not finished is not paid for in the returned score.  In the tables: the arc into trie node n carries
 * ts(depth n) + out(n), out(n) = the sum of full over the phrases that end at n or at a node of n's failure chain; the back-off
 * weight of n is part(depth fail(n)) - part(depth n); the root (state 0) has V arcs, a label that starts no phrase has value 0 and
 * next state 0; state 1 (the state the search starts in) is an arc-less alias of the root with back-off 0;
 * state_final[s] = -part(depth s).  Arc values are positive: `ub` is the bound that keeps the early-outs of the search exact.
 * MI_ERR_ARG for what mi355x_ctc_beam_decode refuses, blank != C-1, n_models outside 1..2, a null `models`, and per model a null
 * table (state_final may be null), n_states < 2, n_arcs < C-1, alpha < 0 or NaN, a NaN ub. */
typedef struct mi355x_ctc_beam_fusion {
  const void* state_arc_begin; const void* arc_tok; const void* arc_logp; const void* arc_next; const void* state_bo;
  const void* state_bo_next; const void* state_final;
  int n_states, n_arcs;
  float alpha, ub;
} mi355x_ctc_beam_fusion;
int mi355x_ctc_beam_decode_fused(const void* logp, const void* lens, void* node_ws, void* tokens, void* tok_frame, void* hyp_len,
                                 void* score, void* n_hyp, int B, int Tmax, int C, int blank, int beam, float threshold, float beta,
                                 const mi355x_ctc_beam_fusion* models, int n_models, void* stream);
/* The resumable form.  The state: `beams` as above (lm_state / lm_sum are the first model's and required), then the second model's
 * per-beam arrays [B, beam] (fresh stream: 1, 0), required with n_models = 2 and not read otherwise.  MI_ERR_ARG for what the
 * resumable entries and the one-shot fused entry refuse and for a missing fs_state / fs_sum with two models. */
typedef struct mi355x_ctc_beam_fused_state {
  mi355x_ctc_beam_stream_state beams;
  int* fs_state; float* fs_sum;
} mi355x_ctc_beam_fused_state;
int mi355x_ctc_beam_decode_fused_stream(const void* logp, const void* lens, void* node_ws, void* tokens, void* tok_frame,
                                        void* hyp_len, void* score, void* n_hyp, int B, int Tmax, int C, int blank, int beam,
                                        float threshold, float beta, const mi355x_ctc_beam_fusion* models, int n_models, int Tcap,
                                        const mi355x_ctc_beam_fused_state* state_in, const mi355x_ctc_beam_fused_state* state_out,
                                        void* stream);

/* ---- committing the stable prefix of a stream, and the search over what is left.  The resumable search above keeps every frame of
 * a stream in its tree.  mi355x_ctc_beam_commit takes the tokens that every live hypothesis shares out of the tree, makes the node
 * they end in the new root and drops every tree frame that no live hypothesis needs any more, so the tree of a stream that never
 * ends stays small.  It does integer work only: the float32 fields of a beam are copied as their bits.
 * The window of a stream (device arrays, all zero for a stream that was never committed):
 *   tok_base     i32 [B]         tokens committed so far
 *   frame_base   i32 [B]         global frames the stream had consumed at its last commit
 *   kept         i32 [B]         tree frames that survived the last commit
 *   frame_map    i32 [B, Tcap]   the global frame of each of the first `kept` tree frames
 * With fd = frames_done of the state, G = frame_base + fd - kept is the number of global frames consumed, and tree frame i is
 * global frame frame_map[i] if i < kept, else i - kept + frame_base.  A node's creation frame is that of its tree frame.
 * Per stream, with S = stable_frames (negative: never force):
 *  1. Forced pruning (S >= 0 only).  cut = G - S.  old(X) of a beam X is the deepest node of its chain (its own node, its parent,
 *     ... ) whose global creation frame is < cut, the root (node 0) if there is none.  X survives iff old(X) == old(slot 0); slot 0
 *     always does.  The survivors keep their order and every field bit for bit (pb, pnb, tot, brank, h, hp, len, tok, the models'
 *     states and sums); nb' is their number; the slots behind them get what the search leaves in an empty slot (node 0, par -1,
 *     tok -1, len 0, the root hash, 0, -inf four times, model state 1 and sum 0).  Identity is BY NODE, not by token sequence: a
 *     beam that spells the same old prefix under another node (the prefix fell out of the set and came back) is dropped.
 *  2. Common ancestor.  A is the deepest node on every survivor's chain (the root if none).  The tokens on the path root -> A and
 *     their global frames are written to com_tokens / com_frames [B, Tcap], positions 0 .. n_com[b]-1, in order.
 *  3. Re-rooting, and compaction in frame space.  Exactly the tree frames that hold a strict descendant of A on a survivor's chain
 *     stay, in order, renumbered 0 .. kept'-1.  Their `beam` pairs go to tree_out with the parent renumbered: A becomes 0, a node
 *     of a kept frame its new id 1 + new frame * beam + slot, anything else 0; a pair of a kept frame that is on no survivor's
 *     chain is written (0, -1).  The beams' node and par are renumbered the same way; a beam that IS A gets node 0 and par -1.
 *     frames_done' = kept', frame_base' = G, tok_base' = tok_base + n_com, frame_map' is composed from the old map.  len stays the
 *     GLOBAL length: the rank uses beta * len and keeps its bits.
 * After a forced commit every kept frame is younger than the cut, so kept' <= S: the memory of a stream is bounded.  With S < 0
 * the commit changes no result: committed tokens followed by the tail that mi355x_ctc_beam_decode_window_stream returns are the
 * hypotheses, frames, lengths and scores of the uncommitted search, bit for bit.
 * Out of place: state_out, window_out and tree_out are written, nothing of the input is; the same input committed twice gives the
 * same result.  workspace: i32, B * mi355x_ctc_beam_commit_workspace_elems(Tcap, beam).  n_models (0..2) says which model arrays
 * of the states are copied (lm_state / lm_sum from 1, fs_state / fs_sum at 2).
 * Whatever the state and the tree hold, nothing is stored outside the arrays given and every walk ends: frames_done, nb and kept
 * are clamped to their ranges (tok_base and frame_base to 0 .. 0x3fffffff, here and in the search below, so that no sum of
 * theirs overflows), a node id outside the frames that are done is the root, and a parent is followed only into an earlier frame.  A state that is not one of this search's gives a wrong answer.
 * MI_ERR_ARG for a null argument or array (model arrays as n_models asks), B < 1, beam outside 1..64, Tcap < 1,
 * Tcap * beam > 0x3fffffff, n_models outside 0..2, trees that are not 8-byte aligned, and aliasing of input and output (the
 * states' node arrays, the trees, the windows' frame_map or kept arrays). */
typedef struct mi355x_ctc_beam_window {
  int* tok_base; int* frame_base; int* kept; int* frame_map;
} mi355x_ctc_beam_window;
long long mi355x_ctc_beam_commit_workspace_elems(int Tcap, int beam);
int mi355x_ctc_beam_commit(const mi355x_ctc_beam_fused_state* state_in, const mi355x_ctc_beam_window* window_in, const void* tree_in,
                           const mi355x_ctc_beam_fused_state* state_out, const mi355x_ctc_beam_window* window_out, void* tree_out,
                           void* com_tokens, void* com_frames, void* n_com, void* workspace, int B, int beam, int Tcap,
                           int n_models, int stable_frames, void* stream);
/* mi355x_ctc_beam_decode_fused_stream (n_models 0..2; `models` may be NULL at 0) over a committed stream: `window` (required, read
 * only) is the record mi355x_ctc_beam_commit wrote with the state and the tree.  Three things differ, none inside a frame:
 *   len of state_in is clamped to tok_base + clamp(len - tok_base, 0, frames_done)
 *   the outputs hold the TAIL of each hypothesis, the tokens behind the committed ones: positions 0 .. len - tok_base - 1 are
 *   written and hyp_len = len - tok_base (score and n_hyp as ever)
 *   tok_frame is the global frame, through the window's map
 * MI_ERR_ARG for what mi355x_ctc_beam_decode_fused_stream refuses (but n_models = 0) and a null window or window array. */
int mi355x_ctc_beam_decode_window_stream(const void* logp, const void* lens, void* node_ws, void* tokens, void* tok_frame,
                                         void* hyp_len, void* score, void* n_hyp, int B, int Tmax, int C, int blank, int beam,
                                         float threshold, float beta, const mi355x_ctc_beam_fusion* models, int n_models, int Tcap,
                                         const mi355x_ctc_beam_fused_state* state_in, const mi355x_ctc_beam_fused_state* state_out,
                                         const mi355x_ctc_beam_window* window, void* stream);

/* SpectrogramAugmentation (nemo/collections/asr/modules/audio_preprocessing.py:443-553; SpecAugment._apply_masks
 * parts/submodules/spectr_augment.py:153-215, SpecCutout.forward :245-261): x[b, f0:f1, t0:t1] = value for n rectangles
 * rects[n][5] = (b, f0, f1, t0, t1) (int32, device memory; clipped to the tensor).  x: f32 [B, F, T], in place. */
int mi355x_fill_rects(void* x, const void* rects, int n, int B, int F, int T, float value, void* stream);
/* SpecAugment mask parameters (SpectrogramAugmentation's vectorised path, parts/submodules/spectr_augment.py:155-195) from the four
 * uniform draws the reference makes -- u_time_width, u_time_start f32 [B, time_masks]; u_freq_width, u_freq_start f32
 * [B, freq_masks] -- and the feature lengths len i64 [B]: rects i32 [B * (time_masks + freq_masks), 5] = (b, f0, f1, t0, t1), time
 * masks first, in the reference's f32 arithmetic (time_width: a fraction of the utterance when time_width_is_fraction, else frames). */
int mi355x_specaug_rects(const void* u_time_width, const void* u_time_start, const void* u_freq_width, const void* u_freq_start,
                         const void* len, void* rects, int B, int time_masks, int freq_masks, int F, int T, float time_width,
                         int time_width_is_fraction, int freq_width, void* stream);

/* ---- RNN-Transducer loss (FastConformer-Transducer, cfg 4) --------------------------------
 * Replaces the Numba-CUDA kernels behind RNNTLossNumba (nemo/collections/asr/parts/numba/rnnt_loss/rnnt_pytorch.py:39-98 ->
 * utils/cuda_utils/gpu_rnnt.py:125-231 -> gpu_rnnt_kernel.py:74-407 alphas / betas / grads, reduce.py denominator,
 * rnnt_helper.py:107-116 costs).  acts f32 [B,T,U1,V1] = joint LOGITS (the log-softmax is fused, as in the reference's
 * GPU path); labels i64 [B,U1-1] (padded); act_lens, label_lens i64 [B]; costs f32 [B] = -(1+fastemit_lambda) * log P(y|x);
 * grads f32 [B,T,U1,V1] (NULL = loss only) = grad_scale * d cost / d acts with the FastEmit term (gpu_rnnt_kernel.py:364-376)
 * and clamp (> 0: clip to [-clamp, clamp], :392-396); cells beyond an utterance's (T_b, U_b+1) are written as zeros.
 * workspace f32, at least mi355x_rnnt_workspace_elems(B,T,U1) elements.  U1 <= 1024.                                     */
int mi355x_rnnt_workspace_elems(int B, int T, int U1, long long* elems);
int mi355x_rnnt_loss(const void* acts, const void* labels, const void* act_lens, const void* label_lens, int B, int T, int U1,
                     int V1, int blank, float fastemit_lambda, float clamp, float grad_scale, void* costs, void* grads,
                     void* workspace, long long workspace_elems, void* stream);
/* Same, for the fused joint + loss path: logit rows with pitch ld_acts (>= V1; a multiple of 8 lets the joint GEMM store them
 * with vector accesses although V+1 = 1025 is odd), and the gradient written in grads_dtype with row pitch ld_grads --
 * MI355X_DT_BF16 with ld_grads % 8 == 0 is directly the K-contiguous operand of the joint's backward GEMMs (columns
 * [V1, ld_grads) zero-filled): no f32 gradient tensor, no cast pass. */
int mi355x_rnnt_loss_ex(const void* acts, long long ld_acts, const void* labels, const void* act_lens, const void* label_lens,
                        int B, int T, int U1, int V1, int blank, float fastemit_lambda, float clamp, float grad_scale, void* costs,
                        void* grads, int grads_dtype, long long ld_grads, void* workspace, long long workspace_elems,
                        void* stream);

/* ---- greedy transducer decoding on the device: GreedyBatchedRNNTInfer, nemo/collections/asr/parts/submodules/
 * rnnt_greedy_decoding.py:529-990 (batched greedy search; per utterance: state = 0, last = blank; for every frame t < enc_len[b], up
 * to max_symbols times: g = LSTM(emb[last], state), logits = out(relu(enc_proj[b,t] + pred(g))), k = argmax; blank -> next frame,
 * else emit (k, t), commit the state, last = k).  ONE launch for the batch, no host synchronisation per frame (the reference reads
 * `blank_mask.all()` back per inner iteration).  enc_proj [B, T, J] (f_dtype, row pitch ldf) = joint.enc(encoder output); emb f32
 * [V1, H] (row `blank` zero); one LSTM layer, torch gate order i, f, g, o: w_ih / w_hh [4H, H], w_pred [J, H], w_out [V1, J] in w_dtype
 * with row pitches ld_*; biases f32.  tokens / times i32 [B, max_out] (-1 padded; times optional), out_len i32 [B], score f32 [B]
 * (optional: sum of the emitted labels' log-probabilities), h_out / c_out f32 [B, H] (optional, both or neither: the final state).
 * max_symbols <= 0: unlimited.  H, J and the pitches multiples of 4.
 * Every form of the search -- this one, TDT, resumable, with confidences, with fusion models -- is one call of
 * mi355x_transducer_greedy_decode with a mi355x_transducer_greedy_desc; both are declared below, after the paragraphs that state
 * each form. */

/* ---- Token-and-Duration Transducer (TDT) loss: the objective of the reference's TDTLossNumba (rnnt_pytorch.py -> GPUTDT,
 * gpu_rnnt.py).  acts f32 [B,T,U1,V1+D] = joint LOGITS with row pitch ld_acts >= V1+D: V1 label logits (blank among them), then D
 * duration logits for durations[] (host array: integers, strictly ascending, durations[0] = 0, durations[D-1] <= 8, 2 <= D <= 8).
 * Blank arcs of duration d >= 1 move (t,u) -> (t+d,u), label arcs (t,u) -> (t+d,u+1) (d = 0 allowed); arc weight = label
 * log-prob + duration log-prob - sigma (sigma >= 0); a path ends with a blank arc landing on (T_b, U_b).  costs f32 [B] =
 * -log P(y|x); grads (NULL = loss only) = grad_scale * d cost / d acts in grads_dtype with row pitch ld_grads >= V1+D (bf16:
 * ld_grads % 8 == 0, columns [V1+D, ld_grads) zero-filled); cells beyond an utterance's (T_b, U_b+1) are zeros.  workspace f32,
 * at least mi355x_tdt_workspace_elems(B,T,U1,D) elements.  U1 <= 1024. */
int mi355x_tdt_workspace_elems(int B, int T, int U1, int D, long long* elems);
int mi355x_tdt_loss_ex(const void* acts, long long ld_acts, const void* labels, const void* act_lens, const void* label_lens, int B,
                       int T, int U1, int V1, int D, const int* durations, int blank, float sigma, float grad_scale, void* costs,
                       void* grads, int grads_dtype, long long ld_grads, void* workspace, long long workspace_elems, void* stream);

/* ---- greedy TDT decoding on the device (the descriptor's D and durations given): the RNN-T search's fields plus the duration set;
 * w_out [V1+D, J], b_out [V1+D].  Per utterance: t = 0; while t < enc_len[b]: k = argmax of the V1 label logits, d = durations[argmax
 * of the D duration logits] (first maximum wins for both); blank -> t += max(d, 1); else emit (k, t), commit the state, t += d, where
 * the max_symbols-th consecutive label of duration 0 (max_symbols > 0) is moved on by one frame.  At most max_out labels. */

/* ---- resumable greedy search (streaming transducer decoding: the reference's `partial_hypotheses`; the descriptor's state_out
 * given).  The searches above, started from a per-stream decoder state and returning the next one, so that a stream decoded
 * chunk by chunk gives bit-identical tokens, frame indices, lengths, score and final state to one launch over the whole sequence, for ANY cut into chunks.
 * State (device arrays, written out of place: state_out must not alias state_in):
 *   h, c          f32 [B, H]  committed LSTM state                                              fresh stream: 0
 *   last          i32 [B]     last emitted label (blank = the zero embedding row)                             blank
 *   score         f32 [B]     running sum of the emitted labels' log-probabilities                            0
 *   frames_done   i32 [B]     frames consumed by earlier chunks; added to every frame index written           0
 *   skip          i32 [B]     TDT: frames of this chunk an earlier duration already jumped over               0
 *   zero_run      i32 [B]     TDT: current run of labels emitted with duration 0                              0
 * (skip / zero_run may be NULL for the RNN-T search.)  state_in NULL = every stream is fresh.  The kernel rebuilds the pending
 * prediction step from (h, c, emb[last]) at entry.  enc_len[b] = the frames of THIS chunk (0: the state passes through, nothing is
 * emitted); frames_done_out = frames_done + enc_len[b]; TDT: skip_out = t - enc_len[b] when the last jump left the chunk, and a
 * chunk with skip >= enc_len[b] is skipped whole.  tokens / times / out_len hold this chunk's labels only; times are global frame
 * indices.  max_symbols counts per frame, so the RNN-T search carries no counter; max_symbols <= 0 bounds each CHUNK by max_out.
 * With max_symbols > 0 give max_out >= T * max_symbols: as in the one-shot search, labels beyond max_out are counted and scored but
 * not stored, and here they would also enter the carried state (last, h, c), which then contradicts what the caller received.
 * T >= 1 as for the one-shot search: a step in which no stream has a frame is not a launch (keep the state).  A one-shot call
 * (both states NULL, no models) launches its own instantiation of the kernel template, compiled without the state code. */
typedef struct mi355x_rnnt_stream_state {
  float* h; float* c; int* last; float* score; int* frames_done; int* skip; int* zero_run;
} mi355x_rnnt_stream_state;

/* ---- the searches above with the confidence of every emitted label (the descriptor's `conf` given): tok_conf f32
 * [B, max_out] (0.0 padded) and the measure (MI355X_CONF_*, k0..k2 for V = V1).  tok_conf[b, n] = the confidence of the step that
 * emitted label n, over the V1 label logits of that step (blank included; TDT: the duration logits take no part); blank steps are
 * not kept.  The sums ride in the pass that computes the step's log-sum-exp, relative to the maximum logit.  Everything else the
 * search writes is bit-identical to what it writes without a measure, and a stream cut into any chunks gives bit-identical tok_conf
 * to one launch: the value belongs to a label, so the stream state carries nothing new.  These launch their own instantiations of
 * the kernel template; a call without a measure launches the code it always has.  MI_ERR_ARG also for a null tok_conf,
 * alpha <= 0, unknown enum values. */
typedef struct mi355x_transducer_conf {
  int method, norm;   /* MI355X_CONF_*, MI355X_CONF_NORM_* */
  float alpha, k0, k1, k2;
} mi355x_transducer_conf;

/* ---- the greedy searches with shallow fusion (the descriptor's `models` given): one or two fusion models, the automata of
 * mi355x_ctc_beam_fusion above (an n-gram model: six tables; a boosting tree: the six and state_final), for RNN-T and TDT, one-shot
 * (both states NULL) and resumable (state_out given, state_in NULL = fresh streams).  The tables cover the labels 0 .. V1-2,
 * so blank == V1-1 is required.  `ub` is not read: this search has no early-outs.
 * Each stream keeps one automaton state per model; a fresh stream starts every model in state 1.  One step on frame t with the
 * label logits lg[0 .. V1):
 *   mi = the arg-max of lg (first maximum), as in the searches above.  mi == blank: the step is theirs -- the models never turn a
 *   blank into a label.  Otherwise the emitted label is the arg-max over v != blank (first maximum) of
 *     rank_v = ((lg[v] - lg[mi]) + alpha_0 * look_0(state_0, v)) + alpha_1 * look_1(state_1, v)
 *   in float32, in that association, each product rounded before it is added; look_m(s, v) is the look-up of model m from state s
 *   (ln p(v | s) of an n-gram model, the boost increment of a tree).  Every model then moves to the state behind the emitted label.
 *   TDT: the duration stays the arg-max of the duration logits; max_symbols, the jumps, skip and zero_run are unchanged.
 * Score: per emitted label k the running score gains (((lg[k] - lg[mi]) - log se) + alpha_0 * l_0) + alpha_1 * l_1, se = the sum of
 * exp(lg[v] - lg[mi]) over the V1 labels and l_m = look_m(state_m, k).  The `score` output is the running score with
 * alpha_m * state_final_m[state_m] added in model order wherever that table is given: the boost of a phrase that was begun and not
 * finished is taken back, as in the CTC search.  The stream state carries the running score WITHOUT those terms, so any cut into
 * chunks gives the bits of one launch -- tokens, frames, lengths, score, h / c and every field of the state -- and with every
 * alpha = 0 all of them are the bits of the search without models.  Parity with the reference's fused scores is not claimed: this
 * paragraph is the rule.
 * State: the resumable search's, and m_state_in / m_state_out i32 [B, 2], the automaton state of model m in column m (fresh
 * stream: 1; column 1 is neither read nor written with one model); m_state_in is read with state_in, m_state_out written with
 * state_out.  score, h_out / c_out as in the one-shot search, optional in both forms.
 * MI_ERR_ARG for what the search without models refuses, n_models outside 1..2, a null `models`, per model a null table
 * (state_final may be null), n_states < 2, n_arcs < V1-1, alpha < 0 or NaN; blank != V1-1; a state given with a null m_state_*;
 * state_in without state_out; aliased states. */

/* ---- the descriptor of a greedy search and its one entry.  A group that is absent selects the search without it:
 *   TDT         D == 0 and durations NULL: the RNN-T search.  Anything else must be a valid duration set (host array, as for
 *               mi355x_tdt_loss_ex).
 *   resumable   state_in and state_out NULL: the one-shot search.  state_out alone: fresh streams.  state_in without state_out:
 *               MI_ERR_ARG.
 *   confidence  conf NULL: none, and tok_conf is ignored.
 *   fusion      models NULL and n_models == 0: none, and m_state_* are ignored.  Anything else is a fusion request.
 * Confidences together with fusion models are refused with MI_ERR_ARG before anything is launched: the kernel template has no
 * such instantiation.  times, score and the pair h_out / c_out are optional in every form.  A NULL descriptor is MI_ERR_ARG.
 * The nine entries this one replaced (named here without the mi355x_ prefix), as descriptor settings:
 *   former entry                          TDT           states                    conf  models  passed as NULL
 *   rnnt_greedy_decode                    -             -                         -     -       -
 *   tdt_greedy_decode                     D, durations  -                         -     -       -
 *   {rnnt,tdt}_greedy_decode_stream       as above      state_out (+ state_in)    -     -       score, h_out, c_out
 *   {rnnt,tdt}_greedy_decode_conf         as above      -                         set   -       -
 *   {rnnt,tdt}_greedy_decode_stream_conf  as above      state_out (+ state_in)    set   -       score, h_out, c_out
 *   transducer_greedy_decode_fused        either        none, or as above         -     1..2    -                    */
typedef struct mi355x_transducer_greedy_desc {
  const void* enc_proj; const void* enc_len;                                           /* input (enc_len i64 [B])        */
  const void* emb; const void* w_ih; const void* w_hh; const void* w_pred; const void* w_out;   /* weights               */
  const void* b_ih; const void* b_hh; const void* b_pred; const void* b_out;
  const int* durations;                                                                /* TDT: host array [D]            */
  void* tokens; void* times; void* out_len; void* score; void* h_out; void* c_out;     /* outputs                        */
  const mi355x_rnnt_stream_state* state_in; const mi355x_rnnt_stream_state* state_out; /* resumable                      */
  const mi355x_transducer_conf* conf; void* tok_conf;                                  /* confidence                     */
  const mi355x_ctc_beam_fusion* models; const int* m_state_in; int* m_state_out;       /* fusion: models[n_models]       */
  long long ldf, ld_ih, ld_hh, ld_pred, ld_out;
  int f_dtype, w_dtype;
  int B, T, J, H, V1, blank, max_symbols, max_out;
  int D, n_models;
} mi355x_transducer_greedy_desc;
int mi355x_transducer_greedy_decode(const mi355x_transducer_greedy_desc* d, void* stream);

/* ---- the greedy searches for a prediction network of L = 1 + n_upper LSTM layers, L in 1..4: every form the descriptor above
 * states (RNN-T and TDT, one-shot and resumable, with confidences, with one or two fusion models, fp32 masters and bf16 images).
 * The descriptor keeps describing layer 0; the struct below adds layers 1 .. n_upper, all [4H, H] in the descriptor's w_dtype with
 * f32 biases.  THE RULE -- one prediction step on the input x = emb[last] with the committed state h[l], c[l], l = 0 .. L-1:
 *     z     = ((W_hh[l] . h[l] + b_hh[l]) + W_ih[l] . in_l) + b_ih[l]      in_0 = x, in_l = hn[l-1];  torch gate order i, f, g, o
 *     cn[l] = sigmoid(f) * c[l] + sigmoid(i) * tanh(g)
 *     hn[l] = sigmoid(o) * tanh(cn[l])
 *     gp    = W_pred . hn[L-1] + b_pred
 * in float32, in that association (every dot product a sum over lane-strided 4-vectors reduced across a wave; the layers run
 * in a chain from the bottom, an upper layer's two products in one pass over its rows).  Eval mode: no dropout between layers.
 * Emitting a label commits EVERY layer (h[l] <- hn[l], c[l] <- cn[l]) and runs the next step; a blank start-of-sequence input
 * skips layer 0's W_ih product alone.  Everything else is the one-layer search's: the arg-max rules, TDT durations and max_symbols,
 * score, confidence sums, fusion ranks, skip / zero_run / frames_done.
 * With n_upper > 0 every LSTM state is [L, B, H] (torch's LSTM state layout): h / c of both mi355x_rnnt_stream_state and h_out /
 * c_out.  The resumable form keeps its contract: any cut into chunks gives the bits of one launch -- tokens, frames, lengths,
 * score, every state field and tok_conf.
 * upper NULL or n_upper == 0: the entry above, with the same checks, the same kernels and the same bits ([B, H] states).
 * MI_ERR_ARG, before anything is launched: everything the entry above refuses; n_upper outside 0..3; in a used slot a null table
 * or a pitch that is not a multiple of 4; an LDS need of 4 * (5H + 4LH + 2J + V1 + D + 4) bytes above 160 KiB - 256 (x [H], then
 * h, c, hn, cn of every layer, the gates [4H], two [J] vectors and the logits; L = 1 is the 9H + ... of the one-layer search).
 * The deep kernels are instantiations of their own, all of them the resumable kernel (a one-shot call is a fresh stream with
 * no state to write); the one-layer calls launch the code they always have. */
typedef struct mi355x_transducer_lstm_layers {   /* layers 1 .. n_upper of the prediction network */
  int n_upper;                                    /* L - 1: 0 .. 3 */
  const void* w_ih[3]; const void* w_hh[3];       /* [4H, H] in the descriptor's w_dtype */
  const void* b_ih[3]; const void* b_hh[3];       /* f32 [4H] */
  long long ld_ih[3], ld_hh[3];                   /* row pitches, multiples of 4 */
} mi355x_transducer_lstm_layers;
int mi355x_transducer_greedy_decode_layers(const mi355x_transducer_greedy_desc* d, const mi355x_transducer_lstm_layers* upper,
                                           void* stream);

/* ---- cache-aware streaming inference (ConformerEncoder.cache_aware_stream_step; the `update_cache` paths of
 * RelPositionMultiHeadAttention and CausalConv1D).  Caches are f32 in the reference's layouts; in bf16 compute they hold the
 * bf16-rounded operands widened to f32, so a streamed chunk reads the same operand values as the offline forward.
 * mi355x_stream_cache_assemble: kv_in [B*(C+Tq), d] (dtype) = cat(cache [B,C,d] f32, y [B*Tq,d] dtype) along time; cache_next
 * [B,C,d] f32 = its last C rows (d % 4 == 0; C may be 0).
 * mi355x_stream_attn: q [B*Tq, ldq] (head h at column h*dk), kv [B*Tk, ldkv] (k of head h at h*dk, v at v_off + h*dk),
 * pos [2Tk-1, ldp] = linear_pos of the Tk table (row r <-> relative position Tk-1-r), bias_u / bias_v f32 [H*dk];
 * cache_len / chunk_len i64 [B].  Query i sits at key position C + i (C = Tk - Tq); score(i,j) = ((q_i+u).k_j + (q_i+v).p_{j+Tq-1-i})
 * * scale; key j is visible when C - cache_len[b] <= j < C + chunk_len[b] and, for chunk > 0, 0 <= (C+i)/chunk - j/chunk <=
 * left_chunks (< 0: unlimited).  ctx [B*Tq, ldo] (dtype); a row with no visible key is zero.  dk <= 128.
 * mi355x_stream_dwconv: x [B*Tq, d] (dtype), cache [B, d, K-1] f32 (left taps), w [d, K], bias [d] f32 -> y [B*Tq, d] (dtype),
 * cache_next [B, d, K-1] f32 = the last K-1 frames of cat(cache, x); K in {3, 5, 9, 31}; cache_next must not alias cache. */
int mi355x_stream_cache_assemble(const void* cache, const void* y, void* kv_in, void* cache_next, int dtype, int B, int C, int Tq,
                                 int d, void* stream);
int mi355x_stream_attn(const void* q, long long ldq, const void* kv, long long ldkv, long long v_off, const void* pos,
                       long long ldp, const void* bias_u, const void* bias_v, const void* cache_len, const void* chunk_len,
                       void* ctx, long long ldo, int dtype, int B, int H, int Tq, int Tk, int dk, int chunk, int left_chunks,
                       float scale, void* stream);
int mi355x_stream_dwconv(const void* x, const void* cache, const void* w, const void* bias, void* y, void* cache_next, int dtype,
                         int B, int Tq, int d, int ksize, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_ASR_H */
