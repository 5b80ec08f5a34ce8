// Greedy RNN-Transducer decoding on the device (FastConformer-Transducer, BASELINE.json configs[3]): the whole auto-regressive
// search of a batch in ONE launch, no host round trip per frame or per symbol.
//
// Replaces on the reference path: GreedyBatchedRNNTInfer (nemo/collections/asr/parts/submodules/rnnt_greedy_decoding.py:529-990;
// `_greedy_decode_blank_as_pad_loop_frames` :804-990 and the label-looping computer produce the same hypotheses), i.e. per
// utterance the textbook greedy search:
//     state = 0, last = blank (the start-of-sequence input is the zero embedding: blank_as_pad, rnnt.py:880-883)
//     for t < T_b:  repeat up to max_symbols times:
//         g = pred(emb[last], state)  ->  logits = out(relu(enc_proj[t] + pred_proj(g)))        (rnnt.py:1640-1720, joint_net = ReLU,
//         k = argmax logits;  blank -> next frame;  else emit (k, t), state <- state', last <- k          Dropout(eval: off), Linear)
// The reference runs it as a Python loop over frames with a device->host sync per inner iteration (`blank_mask.all()`, :931) and
// B x (prediction step + joint step) launches each; here a workgroup owns an utterance, keeps the LSTM state, the prediction
// projection and the logits in LDS, and streams the weights (fp32 masters, or the bf16 GEMM images) from L2 as matrix-vector
// products -- an HBM / L2-bandwidth-bound loop by nature (no reuse across the 1-row "batch" of a workgroup: not MFMA work).
// Outputs are integer token ids and frame indices: bit-exact against the oracle restatement (oracle/transducer_ref.py
// greedy_decode) and the reference-run fixture (tests/golden/ref_rnnt_greedy.json).
//
// Token-and-Duration Transducer (a descriptor with a duration set: the TDT instance of the same kernel): the output layer has V1 + D rows,
// label arg-max over the first V1 logits, duration arg-max over the last D, and the frame index advances by the predicted
// duration (a blank by at least one frame; a run of max_symbols labels predicted with duration 0 is moved on by one frame).
//
// Resumable search (a descriptor with state_out; mi355x_transducer_greedy_decode is the one entry): the same kernel started from a per-stream
// decoder state (committed h / c, last label, running score, frames consumed so far; TDT: frames already jumped over and the
// run of zero-duration labels) and writing the next one, out of place.  hn / cn / gp are NOT carried: they are rebuilt from
// (h, c, emb[last]) by one prediction step at entry -- the very step `emit` ran after the last label -- so a stream cut into any
// chunks takes the same decisions with the same arithmetic as one launch over the whole sequence: tokens, frame indices,
// lengths, score and final state are bit-identical.  The one-shot entry points are the fresh-state case.
//
// Prediction networks of L = 1 + n_upper LSTM layers (mi355x_transducer_greedy_decode_layers, L <= 4).  THE RULE: one prediction step on
// the input x = emb[last] with the committed state h[l], c[l], l = 0 .. L-1, is, layer by layer from the bottom,
//     z     = ((W_hh[l] . h[l] + b_hh[l]) + W_ih[l] . in_l) + b_ih[l]         in_0 = x, in_l = hn[l-1]   (torch gate order i, f, g, o)
//     cn[l] = sigmoid(f) * c[l] + sigmoid(i) * tanh(g),   hn[l] = sigmoid(o) * tanh(cn[l]),   gp = W_pred . hn[L-1] + b_pred
// in float32 and in that association: every dot product is a wave's sum over lane-strided 4-vectors, the recurrent product with
// its bias first, then the input product, then the input bias.  No dropout between layers (eval mode).  Emitting a label commits
// EVERY layer (h[l] <- hn[l], c[l] <- cn[l]) and runs the next step; a blank start-of-sequence input skips layer 0's W_ih product
// alone.  Layer 0 is the code of the one-layer search; an upper layer computes both of its products in ONE pass over the rows (two
// accumulators per row, so the loads of both matrices are in flight together and the layer costs one barrier less); the layers
// run in a chain, the recurrent products are not hoisted in front of it (that would need 4H more floats of LDS per layer for no
// fewer bytes read).  LDS holds h, c, hn, cn of every layer; all states on the device are [L, B, H] (torch's LSTM state layout).
// The arg-max rules, TDT durations, max_symbols, score, confidence sums, fusion ranks and skip / zero_run / frames_done are those
// of the one-layer search, and so is the resumable contract: any cut into chunks gives the bits of one launch.
#include "common.h"
#include "ctc_beam_fusion.h"
#include "mi355x_asr.h"
#include "tdt.h"

#define RD_THREADS 512
#define RD_WAVES 8

template <typename WT> __device__ __forceinline__ void rd_ld4(const WT* p, float (&v)[4]);
template <> __device__ __forceinline__ void rd_ld4<float>(const float* p, float (&v)[4]) { ld4<float>(p, v); }
template <> __device__ __forceinline__ void rd_ld4<bf16_t>(const bf16_t* p, float (&v)[4]) { ld4<bf16_t>(p, v); }

// out[r] (+)= sum_k W[r * ldw + k] * v[k] for r in [0, R): one wave per row (rows dealt round-robin to the 8 waves), lanes stride
// over k in 4-element vectors, fp32 accumulation, wave_sum.  `v` lives in LDS; K % 4 == 0.
template <typename WT, bool ACC>
__device__ __forceinline__ void rd_gemv(const WT* __restrict__ W, long long ldw, const float* v, int R, int K, const float* bias,
                                        float* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < R; r += RD_WAVES) {
    const WT* w = W + (long long)r * ldw;
    float a = 0.f;
    for (int k = lane * 4; k < K; k += 256) {
      float x[4];
      rd_ld4<WT>(w + k, x);
      const float4 y = *reinterpret_cast<const float4*>(v + k);
      a += x[0] * y.x + x[1] * y.y + x[2] * y.z + x[3] * y.w;
    }
    a = wave_sum(a);
    if (lane == 0) out[r] = (ACC ? out[r] : 0.f) + a + (bias ? bias[r] : 0.f);
  }
}

// out[r] = ((sum_k Wh[r, k] * vh[k] + bh[r]) + sum_k Wi[r, k] * vi[k]) + bi[r]: the two products of an upper LSTM layer in one pass over
// the rows (rd_gemv<false> on Wh followed by rd_gemv<true> on Wi gives these bits; here nothing waits between them)
template <typename WT>
__device__ __forceinline__ void rd_gemv2(const WT* __restrict__ Wh, long long ldh, const float* vh, const WT* __restrict__ Wi,
                                         long long ldi, const float* vi, int R, int K, const float* bh, const float* bi, float* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < R; r += RD_WAVES) {
    const WT* wh = Wh + (long long)r * ldh;
    const WT* wi = Wi + (long long)r * ldi;
    float a = 0.f, e = 0.f;
    for (int k = lane * 4; k < K; k += 256) {
      float x[4], u[4];
      rd_ld4<WT>(wh + k, x);
      rd_ld4<WT>(wi + k, u);
      const float4 y = *reinterpret_cast<const float4*>(vh + k);
      const float4 w = *reinterpret_cast<const float4*>(vi + k);
      a += x[0] * y.x + x[1] * y.y + x[2] * y.z + x[3] * y.w;
      e += u[0] * w.x + u[1] * w.y + u[2] * w.z + u[3] * w.w;
    }
    a = wave_sum(a);
    e = wave_sum(e);
    if (lane == 0) out[r] = ((0.f + a + bh[r]) + e) + bi[r];
  }
}

// the LSTM cell of an upper layer on the gate pre-activations z [4H] (i, f, g, o) and the committed cell state c: cn, hn.  Layer 0
// has the same loop inside the kernel: the one-layer instantiations are held to the instructions they have always had.
__device__ __forceinline__ void rd_lstm_cell(const float* z, const float* c, float* hn, float* cn, int H) {
  for (int j = threadIdx.x; j < H; j += RD_THREADS) {
    const float ig = 1.f / (1.f + expf(-z[j])), fg = 1.f / (1.f + expf(-z[H + j]));
    const float gg = tanhf(z[2 * H + j]), og = 1.f / (1.f + expf(-z[3 * H + j]));
    const float cc = fg * c[j] + ig * gg;
    cn[j] = cc;
    hn[j] = og * tanhf(cc);
  }
}

struct RnntDecP {
  const void* f; int f_dt; long long ldf;   // encoder projection [B, T, J] (rows of pitch ldf)
  const long long* enc_len;
  const float* emb;                          // [V1, H] fp32 (row `blank` is the zero padding row)
  const void *w_ih, *w_hh, *w_pred, *w_out;  // [4H, H], [4H, H], [J, H], [V1, J] (dtype w_dt, row pitches below)
  long long ld_ih, ld_hh, ld_pred, ld_out;
  const float *b_ih, *b_hh, *b_pred, *b_out;
  int* tokens; int* times; int* out_len; float* score;
  float* h_out; float* c_out;                // optional final state [B, H]
  mi355x_rnnt_stream_state sin, sout;        // resumable search: state to start from (sin.h null: fresh), state to write (sout.h null: none)
  int B, T, J, H, V1, blank, max_symbols, max_out;
  TdtDur dur;                                // TDT: duration set (dur.D = 0 for the RNN-T search)
};
// the parameter block of the CONF = true instantiations: the one above (untouched, so that the others take the very block they
// always took) and the confidence of every emitted label [B, max_out] with its measure
struct RnntDecPC : RnntDecP {
  float* tok_conf; MiConf conf;
};
// the parameter block of the NM > 0 instantiations (the fused search): the first one, the fusion models (room for two whatever
// NM; the second slot is not read at NM = 1) and the per-stream automaton states [B, 2] to start from (null: fresh streams, every
// model in state 1) and to write (null: none)
struct RnntDecPF : RnntDecP {
  ctc_beam_lm lm[2];
  const int* ms_in; int* ms_out;
};
// layers 1 .. n of the prediction network (mi355x_transducer_lstm_layers with typed pointers), and the parameter blocks of the DEEP
// instantiations: each of the three above (untouched) with the upper layers behind it, by value
struct RnntUpper {
  int n;
  const void *w_ih[3], *w_hh[3];
  const float *b_ih[3], *b_hh[3];
  long long ld_ih[3], ld_hh[3];
};
template <typename Base> struct RnntDecDeep : Base { RnntUpper up; };
template <bool CONF, int NM = 0, bool DEEP = false> struct RnntDecArg { typedef RnntDecP t; };
template <> struct RnntDecArg<true, 0> { typedef RnntDecPC t; };
template <> struct RnntDecArg<false, 1> { typedef RnntDecPF t; };
template <> struct RnntDecArg<false, 2> { typedef RnntDecPF t; };
template <bool CONF, int NM> struct RnntDecArg<CONF, NM, true> { typedef RnntDecDeep<typename RnntDecArg<CONF, NM>::t> t; };

// STREAM = false is the one-shot search: the state code folds away at compile time and the instantiation is the kernel the
// one-shot entry points have always launched.  CONF = false likewise: the sums of the confidence measure, their two block
// reductions and the store in `emit` exist in the CONF = true instantiations alone (the *_conf entry points).
//
// NM = the number of fusion models (a descriptor with `models`; STREAM = true, CONF = false only: a one-shot call is a
// fresh stream with no state to write).  NM = 0 is the search without models: everything below that names a model sits behind
// `if constexpr (NM > 0)` and those instantiations are the kernels they were.  With models a step whose arg-max is a label picks
// the label by rank_v = ((lg[v] - lg[mi]) + alpha_0 * look_0(state_0, v)) + alpha_1 * look_1(state_1, v) over v != blank (a blank
// arg-max stays a blank: the models never turn a blank into a label); the states are uniform over the workgroup.
//
// DEEP = a prediction network of L = 1 + p.up.n layers (the rule is at the top of this file; STREAM = true only, for the reason
// NM > 0 gives).  LDS then holds the block (h, c, hn, cn) of every layer, layer 0's where it always was and layer l's 4 * l * H floats
// behind it, and the state arrays are [L, B, H].  DEEP = false: none of it exists and the instantiations are the kernels they were.
template <typename WT, bool TDT, bool STREAM, bool CONF, int NM = 0, bool DEEP = false>
__global__ __launch_bounds__(RD_THREADS) void rnnt_greedy_kernel(typename RnntDecArg<CONF, NM, DEEP>::t p) {
  static_assert(NM == 0 || (STREAM && !CONF && NM <= 2), "the fused search is the resumable one, without confidences");
  static_assert(!DEEP || STREAM, "the deep search is the resumable one (a one-shot call: a fresh stream, no state to write)");
  extern __shared__ __attribute__((aligned(16))) float rd_smem[];
  const int H = p.H, J = p.J, V1 = p.V1;
  float* x = rd_smem;            // [H] embedding of the last emitted label
  float* h = x + H;              // committed state
  float* c = h + H;
  float* hn = c + H;             // state after consuming `last` (committed when the next label is emitted)
  float* cn = hn + H;
  float* z = cn + H;             // [4H] gate pre-activations
  int L = 1;                     // LSTM layers (uniform)
  if constexpr (DEEP) {          // (h, c, hn, cn) of the upper layers sit between layer 0's and z
    L = 1 + min(max(p.up.n, 0), 3);
    z = h + 4 * L * H;
  }
  float* gp = z + 4 * H;         // [J] prediction projection of hn
  float* a = gp + J;             // [J] relu(f_t + gp)
  float* lg = a + J;             // [V1] logits (TDT: [V1 + D], the duration logits behind the label logits)
  __shared__ float red_v[RD_WAVES];
  __shared__ int red_i[RD_WAVES];
  __shared__ int s_k, s_d;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int len = (int)min((long long)p.T, max(0LL, p.enc_len ? p.enc_len[b] : (long long)p.T));
  // where the search starts: a fresh stream, or the state an earlier chunk left (all of it uniform over the workgroup)
  const bool resume = STREAM && p.sin.h != nullptr;
  int last = p.blank, frames_done = 0, skip = 0, same = 0;
  float score = 0.f;
  // NM > 0: the automaton state of every model (fresh: 1), and what the look-ups of the step's winner gave: its label logit
  // relative to the arg-max, and per model the value and the state behind it (joint_step sets them, emit uses them)
  int m_state[NM > 0 ? NM : 1], f_next[NM > 0 ? NM : 1];
  float f_look[NM > 0 ? NM : 1], f_d = 0.f;
  if constexpr (NM > 0) {
#pragma unroll
    for (int k = 0; k < NM; ++k) {
      m_state[k] = p.ms_in ? __builtin_amdgcn_readfirstlane(p.ms_in[(long long)b * 2 + k]) : 1;
      f_next[k] = 1; f_look[k] = 0.f;
    }
  }
  if (resume) {
    last = p.sin.last[b]; score = p.sin.score[b]; frames_done = p.sin.frames_done[b];
    if (TDT) { skip = max(p.sin.skip[b], 0); same = p.sin.zero_run[b]; }
    if (last < 0 || last >= V1) last = p.blank;   // (a label outside the embedding table is never read)
    if constexpr (DEEP) {
      for (int l = 0; l < L; ++l)
        for (int i = tid; i < H; i += RD_THREADS) {
          h[l * 4 * H + i] = p.sin.h[((long long)l * p.B + b) * H + i]; c[l * 4 * H + i] = p.sin.c[((long long)l * p.B + b) * H + i];
        }
      for (int i = tid; i < H; i += RD_THREADS) x[i] = p.emb[(long long)last * H + i];
    } else {
      for (int i = tid; i < H; i += RD_THREADS) {
        h[i] = p.sin.h[(long long)b * H + i]; c[i] = p.sin.c[(long long)b * H + i]; x[i] = p.emb[(long long)last * H + i];
      }
    }
  } else {
    for (int i = tid; i < H; i += RD_THREADS) { h[i] = 0.f; c[i] = 0.f; x[i] = 0.f; }
    if constexpr (DEEP)
      for (int l = 1; l < L; ++l)
        for (int i = tid; i < H; i += RD_THREADS) { h[l * 4 * H + i] = 0.f; c[l * 4 * H + i] = 0.f; }
  }
  __syncthreads();

  // prediction step on (x, h, c): hn, cn, gp.  torch gate order i, f, g, o (common/parts/rnn.py:151-230 -> torch.nn.LSTM)
  auto pred_step = [&](bool x_zero) {
    rd_gemv<WT, false>((const WT*)p.w_hh, p.ld_hh, h, 4 * H, H, p.b_hh, z);
    __syncthreads();
    if (!x_zero) rd_gemv<WT, true>((const WT*)p.w_ih, p.ld_ih, x, 4 * H, H, p.b_ih, z);
    else for (int i = tid; i < 4 * H; i += RD_THREADS) z[i] += p.b_ih[i];
    __syncthreads();
    for (int j = tid; j < H; j += RD_THREADS) {
      const float ig = 1.f / (1.f + expf(-z[j])), fg = 1.f / (1.f + expf(-z[H + j]));
      const float gg = tanhf(z[2 * H + j]), og = 1.f / (1.f + expf(-z[3 * H + j]));
      const float cc = fg * c[j] + ig * gg;
      cn[j] = cc;
      hn[j] = og * tanhf(cc);
    }
    __syncthreads();
    const float* top = hn;   // hn of the last layer
    if constexpr (DEEP) {
      // (constant indices into the parameter block: the pointers come from scalar loads, no private copy of the tables)
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        if (l + 1 < L) {   // (uniform)
          float* hl = h + (l + 1) * 4 * H;   // this layer's h, c, hn, cn; its input: hn of the layer below, 2H in front of hl
          rd_gemv2<WT>((const WT*)p.up.w_hh[l], p.up.ld_hh[l], hl, (const WT*)p.up.w_ih[l], p.up.ld_ih[l], hl - 2 * H, 4 * H, H,
                       p.up.b_hh[l], p.up.b_ih[l], z);
          __syncthreads();
          rd_lstm_cell(z, hl + H, hl + 2 * H, hl + 3 * H, H);
          __syncthreads();
          top = hl + 2 * H;
        }
      }
    }
    rd_gemv<WT, false>((const WT*)p.w_pred, p.ld_pred, top, J, H, p.b_pred, gp);
    __syncthreads();
  };
  // `last` = blank is the zero embedding row (blank_as_pad); a chunk with no frame to look at takes no decision and needs no step
  if (!STREAM || len > skip) pred_step(!STREAM || last == p.blank);

  int n = 0;
  // CONF: sums of the step's label distribution relative to its maximum logit mv, d_v = lg[v] - mv:
  // cA = sum_v exp(alpha d_v), cB = sum_v exp(alpha d_v) d_v (set by joint_step, used by emit)
  float cA = 0.f, cB = 0.f;
  // joint on frame t and the current prediction projection: label arg-max -> s_k (TDT: duration index arg-max -> s_d), returns
  // sum_v exp(lg[v] - max) over the label logits
  auto joint_step = [&](int t) -> float {
    const char* frow = (const char*)p.f + ((long long)b * p.T + t) * p.ldf * (p.f_dt == MI_DT_F32 ? 4 : 2);
    for (int j = tid; j < J; j += RD_THREADS) {
      const float fv = p.f_dt == MI_DT_F32 ? ((const float*)frow)[j] : bf2f(((const bf16_t*)frow)[j]);
      a[j] = fmaxf(fv + gp[j], 0.f);
    }
    __syncthreads();
    rd_gemv<WT, false>((const WT*)p.w_out, p.ld_out, a, TDT ? V1 + p.dur.D : V1, J, p.b_out, lg);
    __syncthreads();
    // arg-max (lowest index among equal maxima, like torch.max) and log-sum-exp (score = sum of the emitted labels' log-probs)
    float bv = -INFINITY; int bi = 0x7fffffff;
    for (int v = tid; v < V1; v += RD_THREADS) { const float q = lg[v]; if (q > bv) { bv = q; bi = v; } }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
    __syncthreads();
    float mv = red_v[0]; int mi = red_i[0];
#pragma unroll
    for (int w = 1; w < RD_WAVES; ++w) if (red_v[w] > mv || (red_v[w] == mv && red_i[w] < mi)) { mv = red_v[w]; mi = red_i[w]; }
    float se = 0.f;
    float sa = 0.f, sb = 0.f;
    bool sums = false;   // (uniform)
    if constexpr (CONF) sums = p.conf.method != MI355X_CONF_MAX_PROB;
    for (int v = tid; v < V1; v += RD_THREADS) {
      const float d = lg[v] - mv;
      se += expf(d);
      if constexpr (CONF) {
        if (sums) {
          const float e = expf(p.conf.alpha * d);
          sa += e;
          sb += (d == -INFINITY) ? 0.f : e * d;
        }
      }
    }
    __syncthreads();   // (red_v is re-used by block_sum)
    se = block_sum(se, red_v);
    if (sums) { cA = block_sum(sa, red_v); cB = block_sum(sb, red_v); }
    int kf = mi;
    if constexpr (NM > 0) {
      if (mi != p.blank) {   // (uniform)
        // every lane ranks its labels with the models (bounded, clamped look-ups; the tables come from L2), then the block arg-max
        float rv = -INFINITY; int ri = 0x7fffffff;
        for (int v = tid; v < V1; v += RD_THREADS) {
          if (v == p.blank) continue;
          float r = lg[v] - mv;
#pragma unroll
          for (int k = 0; k < NM; ++k) {
            int nx;
            r += ctc_beam_alpha_lm(p.lm[k].alpha, ctc_beam_lm_lookup(p.lm[k], m_state[k], v, nx));
          }
          if (r > rv) { rv = r; ri = v; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float ov = __shfl_xor(rv, o, 64); const int oi = __shfl_xor(ri, o, 64);
          if (ov > rv || (ov == rv && oi < ri)) { rv = ov; ri = oi; }
        }
        __syncthreads();   // (red_v was read by block_sum)
        if (lane == 0) { red_v[wave] = rv; red_i[wave] = ri; }
        __syncthreads();
        float wv = red_v[0]; int wi = red_i[0];
#pragma unroll
        for (int w = 1; w < RD_WAVES; ++w) if (red_v[w] > wv || (red_v[w] == wv && red_i[w] < wi)) { wv = red_v[w]; wi = red_i[w]; }
        // the winner's look-ups again, by every thread at one address: values and states stay uniform (no rank is a number, e.g.
        // NaN logits: the arg-max itself)
        kf = __builtin_amdgcn_readfirstlane((wi < 0 || wi >= V1 || wi == p.blank) ? mi : wi);
        f_d = lg[kf] - mv;
#pragma unroll
        for (int k = 0; k < NM; ++k) {
          int nx = 0;
          f_look[k] = ctc_beam_lm_lookup(p.lm[k], m_state[k], kf, nx);
          f_next[k] = __builtin_amdgcn_readfirstlane(nx);
        }
      }
    }
    if (tid == 0) {
      s_k = kf;
      if (TDT) {   // first maximum wins, as for the labels
        int di = 0;
        for (int i = 1; i < p.dur.D; ++i) if (lg[V1 + i] > lg[V1 + di]) di = i;
        s_d = di;
      }
    }
    __syncthreads();
    return se;
  };
  // commit the state that consumed the previous label, consume the new one
  auto emit = [&](int k, int t, float se) {
    if (n < p.max_out) {
      if (tid == 0) {
        p.tokens[(long long)b * p.max_out + n] = k;
        if (p.times) p.times[(long long)b * p.max_out + n] = STREAM ? frames_done + t : t;
        if constexpr (CONF) {
          // log p_v = d_v - log se: S = cA / se^alpha, G = (cB - cA log se) / se^alpha, max_v p_v = 1 / se
          const float lse = logf(se), r = expf(-p.conf.alpha * lse);
          p.tok_conf[(long long)b * p.max_out + n] = mi_conf_value(p.conf, 1.f / se, cA * r, (cB - cA * lse) * r);
        }
      }
    }
    ++n;
    if (STREAM) last = k;
    // Score semantics: the sum of the emitted labels' LOG-PROBABILITIES (log-softmax of the joint's logits) -- what the
    // reference's search computes on CPU tensors.  On CUDA tensors its `_joint_step(log_normalize=None)` skips the
    // log-softmax and sums raw maximum logits instead (rnnt_greedy_decoding.py:257-259, 965): scores then differ by the
    // summed log-partition terms; the token ids, time stamps and lengths are the same either way.
    if constexpr (NM > 0) {
      // the label's log-prob (lg[k] - lg[mi]) - log se, then the models' terms in model order, each product rounded on its own
      float gain = f_d - logf(se);
#pragma unroll
      for (int m = 0; m < NM; ++m) { gain += ctc_beam_alpha_lm(p.lm[m].alpha, f_look[m]); m_state[m] = f_next[m]; }
      score += gain;
    } else {
      score += -logf(se);   // log-prob of the arg-max label = mv - (mv + log se)
    }
    for (int i = tid; i < H; i += RD_THREADS) { h[i] = hn[i]; c[i] = cn[i]; x[i] = p.emb[(long long)k * H + i]; }
    if constexpr (DEEP)
      for (int l = 1; l < L; ++l)
        for (int i = tid; i < H; i += RD_THREADS) { h[l * 4 * H + i] = hn[l * 4 * H + i]; c[l * 4 * H + i] = cn[l * 4 * H + i]; }
    __syncthreads();
    pred_step(false);
  };
  if constexpr (TDT) {
    // t advances by the predicted duration; the output budget bounds the search like max_symbols <= 0 below
    int t = STREAM ? skip : 0;   // frames an earlier chunk's duration already jumped over
    if (!STREAM) same = 0;
    while (t < len && n < p.max_out) {
      const float se = joint_step(t);
      const int k = s_k;
      const int di = s_d;
      int d = 0;
#pragma unroll
      for (int i = 0; i < TDT_MAXD; ++i) d = (i == di) ? p.dur.d[i] : d;
      if (k == p.blank) {   // a blank never stays on its frame
        t += max(d, 1);
        same = 0;
      } else {
        emit(k, t, se);
        same = d == 0 ? same + 1 : 0;
        if (d == 0 && p.max_symbols > 0 && same >= p.max_symbols) { d = 1; same = 0; }
        t += d;
      }
    }
    if (STREAM) skip = max(t - len, 0);
  } else {
    for (int t = 0; t < len; ++t) {
      // max_symbols <= 0 (the reference's `max_symbols_per_step=None`: unbounded inner loop, rnnt_greedy_decoding.py:620-700) is
      // bounded HERE by the output budget: a model that never emits blank would otherwise keep this workgroup -- and the GPU --
      // busy for ever.  Once max_out labels are out the search stops (out_len == max_out tells the caller it was cut short).
      for (int sym = 0; p.max_symbols > 0 ? sym < p.max_symbols : n < p.max_out; ++sym) {
        const float se = joint_step(t);
        const int k = s_k;
        if (k == p.blank) break;
        emit(k, t, se);
      }
    }
  }
  if constexpr (NM > 0) {
    // the `score` output takes back what a phrase begun and not finished was paid; the stream state keeps the running score
    if (tid == 0) {
      p.out_len[b] = n < p.max_out ? n : p.max_out;
      if (p.score) {
        float sc = score;
#pragma unroll
        for (int k = 0; k < NM; ++k)
          if (p.lm[k].fin) sc += ctc_beam_alpha_lm(p.lm[k].alpha, p.lm[k].fin[min(max(m_state[k], 0), p.lm[k].n_states - 1)]);
        p.score[b] = sc;
      }
      if (p.ms_out) {
#pragma unroll
        for (int k = 0; k < NM; ++k) p.ms_out[(long long)b * 2 + k] = m_state[k];
      }
    }
  } else {
    if (tid == 0) { p.out_len[b] = n < p.max_out ? n : p.max_out; if (p.score) p.score[b] = score; }
  }
  for (int i = tid + n; i < p.max_out; i += RD_THREADS) {   // pad (also when nothing was emitted)
    p.tokens[(long long)b * p.max_out + i] = -1;
    if (p.times) p.times[(long long)b * p.max_out + i] = -1;
    if constexpr (CONF) p.tok_conf[(long long)b * p.max_out + i] = 0.f;
  }
  if constexpr (DEEP) {   // [L, B, H]
    for (int l = 0; l < L; ++l)
      for (int i = tid; i < H; i += RD_THREADS) {
        const long long o = ((long long)l * p.B + b) * H + i;
        const float hv = h[l * 4 * H + i], cv = c[l * 4 * H + i];
        if (p.h_out) { p.h_out[o] = hv; p.c_out[o] = cv; }
        if (p.sout.h) { p.sout.h[o] = hv; p.sout.c[o] = cv; }
      }
  } else {
    if (p.h_out) for (int i = tid; i < H; i += RD_THREADS) { p.h_out[(long long)b * H + i] = h[i]; p.c_out[(long long)b * H + i] = c[i]; }
  }
  if (STREAM && p.sout.h) {
    if constexpr (!DEEP)
      for (int i = tid; i < H; i += RD_THREADS) { p.sout.h[(long long)b * H + i] = h[i]; p.sout.c[(long long)b * H + i] = c[i]; }
    if (tid == 0) {
      p.sout.last[b] = last; p.sout.score[b] = score; p.sout.frames_done[b] = frames_done + len;
      if (TDT) { p.sout.skip[b] = skip; p.sout.zero_run[b] = same; }
    }
  }
}

// The 16 DEEP instantiations, [weights][TDT][plain, with confidences, one model, two models], all of them the resumable kernel: a
// one-shot call is a fresh stream with no state to write.  The block is the one the shallow kernel of the same form takes, with
// the upper layers behind it.
template <typename Block>
static void greedy_issue_deep(const void* fn, const Block& block, const RnntUpper& up, int B, size_t shm, hipStream_t s) {
  RnntDecDeep<Block> q;
  static_cast<Block&>(q) = block;
  q.up = up;
  MI_LAUNCH((void (*)(RnntDecDeep<Block>))fn, dim3(B), dim3(RD_THREADS), shm, s, q);
}

// ---- the one entry of the greedy searches (include/mi355x_asr.h states the descriptor): RNN-T or TDT, one-shot or resumable, with
// the confidence of every emitted label or with one or two fusion models.  Every check is here; nothing is launched after a refusal.
// `upper` (mi355x_transducer_greedy_decode_layers): layers 1 .. n_upper of the prediction network; null or n_upper == 0 is the call
// without it, down to the kernel launched.
static int greedy_decode_impl(const mi355x_transducer_greedy_desc* d, const mi355x_transducer_lstm_layers* upper, hipStream_t s) {
  if (!d) return MI_ERR_ARG;
  if (!d->enc_proj || !d->emb || !d->w_ih || !d->w_hh || !d->b_ih || !d->b_hh || !d->w_pred || !d->w_out || !d->tokens || !d->out_len)
    return MI_ERR_ARG;
  const int B = d->B, H = d->H, J = d->J, V1 = d->V1;
  if (B <= 0 || d->T <= 0 || J <= 0 || H <= 0 || V1 <= 1 || d->max_out <= 0 || d->blank < 0 || d->blank >= V1) return MI_ERR_ARG;
  if ((H & 3) || (J & 3) || (d->ld_ih & 3) || (d->ld_hh & 3) || (d->ld_pred & 3) || (d->ld_out & 3) || (!d->h_out != !d->c_out))
    return MI_ERR_ARG;
  if ((d->f_dtype != MI_DT_F32 && d->f_dtype != MI_DT_BF16) || (d->w_dtype != MI_DT_F32 && d->w_dtype != MI_DT_BF16)) return MI_ERR_ARG;
  RnntDecPF p;   // the widest block; the base and the confidence block are cut from it below
  p.f = d->enc_proj; p.f_dt = d->f_dtype; p.ldf = d->ldf; p.enc_len = (const long long*)d->enc_len; p.emb = (const float*)d->emb;
  p.w_ih = d->w_ih; p.w_hh = d->w_hh; p.w_pred = d->w_pred; p.w_out = d->w_out;
  p.ld_ih = d->ld_ih; p.ld_hh = d->ld_hh; p.ld_pred = d->ld_pred; p.ld_out = d->ld_out;
  p.b_ih = (const float*)d->b_ih; p.b_hh = (const float*)d->b_hh; p.b_pred = (const float*)d->b_pred; p.b_out = (const float*)d->b_out;
  p.tokens = (int*)d->tokens; p.times = (int*)d->times; p.out_len = (int*)d->out_len; p.score = (float*)d->score;
  p.h_out = (float*)d->h_out; p.c_out = (float*)d->c_out;
  p.B = B; p.T = d->T; p.J = J; p.H = H; p.V1 = V1; p.blank = d->blank; p.max_symbols = d->max_symbols; p.max_out = d->max_out;
  const bool tdt = d->D != 0 || d->durations;   // D == 0 with no durations: the RNN-T search
  p.dur = {};
  if (tdt && tdt_durations(d->D, d->durations, &p.dur)) return MI_ERR_ARG;
  const bool fused = d->models || d->n_models != 0;
  if (d->conf && (fused || !d->tok_conf || !mi_conf_valid(V1, d->conf->method, d->conf->norm, d->conf->alpha)))
    return MI_ERR_ARG;   // (no instantiation has both the confidence sums and the models)
  if (d->state_in && !d->state_out) return MI_ERR_ARG;
  p.sin = {}; p.sout = {};
  for (int io = 0; io < 2; ++io) {   // a state is given whole (skip / zero_run: TDT only) or not at all
    const mi355x_rnnt_stream_state* st = io ? d->state_out : d->state_in;
    if (!st) continue;
    if (!st->h || !st->c || !st->last || !st->score || !st->frames_done || (tdt && (!st->skip || !st->zero_run))) return MI_ERR_ARG;
    (io ? p.sout : p.sin) = *st;
  }
  if (p.sin.h && p.sout.h && (p.sin.h == p.sout.h || p.sin.c == p.sout.c)) return MI_ERR_ARG;   // out of place
  p.ms_in = nullptr; p.ms_out = nullptr;
  if (fused) {
    if (!d->models || d->n_models < 1 || d->n_models > 2 || d->blank != V1 - 1) return MI_ERR_ARG;
    for (int k = 0; k < d->n_models; ++k) {   // the tables cover the labels 0 .. V1-2 (state 0's arc index is the label)
      const mi355x_ctc_beam_fusion& m = d->models[k];
      if (!m.state_arc_begin || !m.arc_tok || !m.arc_logp || !m.arc_next || !m.state_bo || !m.state_bo_next) return MI_ERR_ARG;
      if (m.n_states < 2 || m.n_arcs < V1 - 1 || !(m.alpha >= 0.f)) return MI_ERR_ARG;   // (a NaN fails its compare)
    }
    if ((d->state_in && !d->m_state_in) || (d->state_out && !d->m_state_out)) return MI_ERR_ARG;
    if (d->state_in && d->m_state_in == d->m_state_out) return MI_ERR_ARG;   // out of place
    for (int k = 0; k < 2; ++k) {   // (room for two whatever n_models: the second slot repeats the first and is not read)
      const mi355x_ctc_beam_fusion& m = d->models[k < d->n_models ? k : 0];
      p.lm[k] = {(const int*)m.state_arc_begin, (const int*)m.arc_tok, (const float*)m.arc_logp, (const int*)m.arc_next,
                 (const float*)m.state_bo, (const int*)m.state_bo_next, m.n_states, m.n_arcs, m.alpha, m.ub,
                 (const float*)m.state_final};
    }
    if (d->state_in) p.ms_in = d->m_state_in;
    if (d->state_out) p.ms_out = d->m_state_out;
  }
  RnntUpper up = {};
  if (upper) {
    if (upper->n_upper < 0 || upper->n_upper > 3) return MI_ERR_ARG;
    up.n = upper->n_upper;
    for (int l = 0; l < up.n; ++l) {
      if (!upper->w_ih[l] || !upper->w_hh[l] || !upper->b_ih[l] || !upper->b_hh[l] || (upper->ld_ih[l] & 3) || (upper->ld_hh[l] & 3))
        return MI_ERR_ARG;
      up.w_ih[l] = upper->w_ih[l]; up.w_hh[l] = upper->w_hh[l]; up.ld_ih[l] = upper->ld_ih[l]; up.ld_hh[l] = upper->ld_hh[l];
      up.b_ih[l] = (const float*)upper->b_ih[l]; up.b_hh[l] = (const float*)upper->b_hh[l];
    }
  }
  // x [H], (h, c, hn, cn) [4H] per layer, z [4H], gp and a [J], lg [V1 + D], and 4 floats of slack (one layer: 9H + ...)
  const size_t shm = ((size_t)5 * H + (size_t)4 * (1 + up.n) * H + (size_t)2 * J + V1 + p.dur.D + 4) * sizeof(float);
  if (shm > 160 * 1024 - 256) return MI_ERR_ARG;

  if (up.n > 0) {
#define RD_ROW(WT, TDT)                                                                                                          \
  {(const void*)rnnt_greedy_kernel<WT, TDT, true, false, 0, true>, (const void*)rnnt_greedy_kernel<WT, TDT, true, true, 0, true>, \
   (const void*)rnnt_greedy_kernel<WT, TDT, true, false, 1, true>, (const void*)rnnt_greedy_kernel<WT, TDT, true, false, 2, true>}
    static const void* const deep[2][2][4] = {{RD_ROW(float, false), RD_ROW(float, true)}, {RD_ROW(bf16_t, false), RD_ROW(bf16_t, true)}};
#undef RD_ROW
    const void* fn = deep[d->w_dtype == MI_DT_BF16][tdt][fused ? 1 + d->n_models : (d->conf ? 1 : 0)];
    hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    if (fused) {
      greedy_issue_deep<RnntDecPF>(fn, p, up, B, shm, s);
    } else if (d->conf) {
      RnntDecPC pc;
      static_cast<RnntDecP&>(pc) = p;
      pc.tok_conf = (float*)d->tok_conf;
      pc.conf = {d->conf->method, d->conf->norm, d->conf->alpha, d->conf->k0, d->conf->k1, d->conf->k2, (float)V1};
      greedy_issue_deep<RnntDecPC>(fn, pc, up, B, shm, s);
    } else {
      greedy_issue_deep<RnntDecP>(fn, p, up, B, shm, s);
    }
    return MI_OK;
  }

  // The 24 instantiations, [weights][TDT][mode]: the one-shot and the resumable kernel, each plain and with confidences, and the
  // resumable kernel with one and with two models (a fused one-shot call is a fresh stream with no state to write).
  enum { RD_ONESHOT = 0, RD_STREAM = 2, RD_FUSED = 3 };   // + 1: with confidences / + n_models
#define RD_ROW(WT, TDT)                                                                                                          \
  {(const void*)rnnt_greedy_kernel<WT, TDT, false, false>, (const void*)rnnt_greedy_kernel<WT, TDT, false, true>,                \
   (const void*)rnnt_greedy_kernel<WT, TDT, true, false>, (const void*)rnnt_greedy_kernel<WT, TDT, true, true>,                  \
   (const void*)rnnt_greedy_kernel<WT, TDT, true, false, 1>, (const void*)rnnt_greedy_kernel<WT, TDT, true, false, 2>}
  static const void* const kernels[2][2][6] = {{RD_ROW(float, false), RD_ROW(float, true)},
                                               {RD_ROW(bf16_t, false), RD_ROW(bf16_t, true)}};
#undef RD_ROW
  const int mode = fused ? RD_FUSED + d->n_models : (d->state_out ? RD_STREAM : RD_ONESHOT) + (d->conf ? 1 : 0);
  const void* fn = kernels[d->w_dtype == MI_DT_BF16][tdt][mode];
  hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  // the three parameter blocks are the three signatures
  auto issue = [&](auto kernel, const auto& block) { MI_LAUNCH(kernel, dim3(B), dim3(RD_THREADS), shm, s, block); };
  if (fused) {
    issue((void (*)(RnntDecPF))fn, p);
  } else if (d->conf) {
    RnntDecPC pc;
    static_cast<RnntDecP&>(pc) = p;
    pc.tok_conf = (float*)d->tok_conf;
    pc.conf = {d->conf->method, d->conf->norm, d->conf->alpha, d->conf->k0, d->conf->k1, d->conf->k2, (float)V1};
    issue((void (*)(RnntDecPC))fn, pc);
  } else {
    issue((void (*)(RnntDecP))fn, static_cast<const RnntDecP&>(p));
  }
  return MI_OK;
}

extern "C" int mi355x_transducer_greedy_decode(const mi355x_transducer_greedy_desc* d, void* stream) {
  mi_clear_errors();
  const int rc = greedy_decode_impl(d, nullptr, (hipStream_t)stream);
  return rc != MI_OK ? rc : mi_check_launch();
}

extern "C" int mi355x_transducer_greedy_decode_layers(const mi355x_transducer_greedy_desc* d, const mi355x_transducer_lstm_layers* upper,
                                                      void* stream) {
  mi_clear_errors();
  const int rc = greedy_decode_impl(d, upper, (hipStream_t)stream);
  return rc != MI_OK ? rc : mi_check_launch();
}
