/* t2amd.h — C ABI of the MI355X-native Tacotron2 (BERT_Tacotron2) hot path.
 *
 * The reference (PhucNguyenAH/tacotron2_subword) is pure Python on PyTorch and has no FFI;
 * its operator boundary for this path is the Python module API (model.py / attention.py).
 * Each entry point below names the reference interface it replaces (file:line, relative to
 * the reference checkout).  A ctypes binding a maintainer would add is shown in
 * INTEGRATION.md; tacotron2_subword_amd/_lib.py is that binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; fp32, row-major;
 *   - the caller owns every buffer (workspace sizes come from the *_ws_bytes queries);
 *   - work is enqueued on `stream` (a hipStream_t passed as void*); no call allocates device
 *     memory; no call synchronises except t2_decoder_infer (documented there);
 *   - return value 0 = OK, < 0 = error; t2_last_error() gives a thread-local message;
 *   - activations are channels-last: [B, T, C].  Conversion to the reference's [B, C, T]
 *     happens in t2_finalize_outputs.
 */
#ifndef T2AMD_H
#define T2AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T2_ATTN_SMA 0 /* StepwiseMonotonicAttention, attention.py:291-398 (hparams default) */
#define T2_ATTN_LSA 1 /* LocationSensitiveAttention, attention.py:25-85 */
#define T2_ATTN_DCA 4  /* DynamicConvolutionAttention (attention.py:195-289) */
#define T2_ATTN_GMM 3  /* GMMAttention version '2', K = 5 (attention.py:401-506) */
#define T2_ATTN_FWD2 2 /* ForwardAttentionV2 as model.py drives it (attention.py:87-151 with the never-updated log_alpha of
                          model.py:266-270,355): LSA energies, softmax over the first two positions; LSA weight layout */

/* RNG sites: a dropout keep-bit / noise sample is a pure function of (seed, site, index). */
enum {
    T2_SITE_PRENET1 = 1, T2_SITE_PRENET2 = 2, T2_SITE_PRENET1_SUB = 3, T2_SITE_PRENET2_SUB = 4,
    T2_SITE_ATT_H = 5, T2_SITE_ATT_C = 6, T2_SITE_ATT_H_SUB = 7, T2_SITE_ATT_C_SUB = 8,
    T2_SITE_DEC_H = 9, T2_SITE_DEC_C = 10, T2_SITE_NOISE = 11, T2_SITE_NOISE_SUB = 12,
    T2_SITE_ENC0 = 16,      /* +layer (0..2) */
    T2_SITE_ENCSUB0 = 20,   /* +layer (0..2) */
    T2_SITE_POSTNET0 = 24   /* +layer (0..4) */
};

const char* t2_last_error(void);
/* ABI version: bumped whenever a struct below grows or an argument changes meaning.  2 (round 3): t2_dims carries
 * score_mask_value[_sub], the layouts carry chain / chain_floats, norm_out of t2_adam_* is 4 floats.  A caller compiled
 * against another version passes structs of another size: check t2_version() == T2_ABI_VERSION before anything else.
 * 3: t2_decoder_layout carries usave / usaves / locsave / locsaves (LSA: tanh tile and location features of every step).
 * 4: t2_set_precision accepts mode 2 (split-bf16), the layout queries depend on the mode in force, t2_gemm_counts,
 *    t2_set_gemm_split_min_mflop. */
#define T2_ABI_VERSION 4
int t2_version(void);
/* Sticky status of the persistent kernels of the current device (the reference's nearest analogue: train.py:335-340,
 * which at least notices a NaN gradient norm).  A chain whose hand-off timed out writes a non-zero code into a word in
 * page-locked host memory; out_host[0] = that code (0 = fine), read with a plain load: no synchronisation.  While it is
 * non-zero t2_adam_step changes no parameter (norm_out[2] = 1), and t2_decoder_forward / t2_decoder_infer overwrite the
 * outputs of an aborted pass with NaN.  Only t2_chain_status_clear resets it. */
int t2_chain_status(uint32_t* out_host /* [4] */);
int t2_chain_status_clear(void);
/* tests: enqueue a kernel that reports `code` exactly as an aborting chain would */
int t2_debug_report_abort(uint32_t code, void* stream);
/* tests: occupy `workgroups` CUs (96 KB of LDS each, so no persistent workgroup fits beside one) for `milliseconds` on
 * `stream` — what a foreign kernel does to a persistent grid; every wait is bounded */
int t2_debug_occupy(int workgroups, int milliseconds, void* stream);
/* 1 when this process holds the device's claim on persistent kernels (an flock on /tmp/t2amd-persistent-<pci id>.lock,
 * taken at the first pass that could use them; env T2_CHAIN_FORCE=1 skips the test).  A process that does not get it runs
 * the per-step launch path: a persistent grid needs every CU, one process per GPU. */
int t2_chain_claimed(void);
/* Arithmetic type of the GEMM operands: 0 = fp32 (exact fp32 fma chains; the parity path, default),
 * 1 = bf16 operands with fp32 accumulation for the large GEMMs (fp32 storage, converted while
 * staging); recurrent state, BatchNorm statistics and attention recurrences stay fp32.
 * 2 = split-bf16: everything as in mode 0 except the large GEMMs (whole 128- or 256-tiles, K % 64 == 0, batch 1, both
 * extents >= 256, scratch given, at least 2^31 FLOP: t2_set_gemm_split_min_mflop), which run on the bf16 matrix pipe at
 * fp32-grade accuracy: each fp32 operand is staged as hi = bf16(x), lo = bf16(x - hi) (finite for |x| < 3.39e38) and
 * the product is hi.hi + lo.hi + hi.lo with fp32 accumulation, in one launch
 * (error per product about 3 * sqrt(K) * 2^-17 for unit-scale operands, a dozen times the fp32 kernel's own; whole-model
 * outputs stay within 1e-4 of the reference).  A product that does not qualify runs the exact fp32 kernel of mode 0; the
 * recurrent steps (unless t2_set_split_steps is on), the attention kernels, BatchNorm and the decode loop are mode 0's,
 * and the persistent chains do not run in this mode.  The staged operands take 6 bytes per element (mode 1: 2), so the scratch is larger:
 * t2_decoder_layout_query / t2_decoder_bwd_layout_query answer for the mode in force (B=64, T=400: forward +0.6 GB,
 * backward +0.6 GB), and the precision must NOT change between a layout query and the calls that use a workspace of that
 * size.  Callers of t2_conv_bn_* / t2_lstm_seq_* / t2_gemm_ex who want their products on the split path size the
 * scratch for 6 bytes per staged operand element; with less the product runs the exact kernel.  (In every mode the exact
 * kernel's automatic split-K factor is clamped by the scratch it is given, so "bit-identical to mode 0" means: to mode 0
 * with the same scratch size; no product of the model reaches that clamp.) */
int t2_set_precision(int mode);
int t2_get_precision(void);
/* Which kernel family the products took: calls of the GEMM layer since the last reset that launched [0] an exact fp32
 * kernel, [1] the converting bf16 kernel, [2] a bf16-source kernel on single-bf16 operands, [3] a bf16-source kernel on
 * split-bf16 operands.  Host counters, no synchronisation; reset != 0 clears them after the read. */
int t2_gemm_counts(uint64_t* out_host /* [4] */, int reset);
/* Mode 2: a qualifying product still runs the exact fp32 kernel when 2*M*N*K is below mflop * 1e6 (the split path's
 * two staging launches and tripled K do not pay on small products; default 2147, i.e. 2^31 FLOP, from the measured
 * break-even).  mflop < 0 restores the default; 0 sends every qualifying product to the split path (kernel tests on
 * small shapes). */
int t2_set_gemm_split_min_mflop(int mflop);
/* Split-bf16 recurrent steps, opt-in: 0 (default; env T2_SPLIT_STEPS=1 sets the initial value) leaves everything as
 * described above.  1, and ONLY while the precision mode is 2: the teacher-forced passes (t2_decoder_forward /
 * t2_decoder_backward, B <= 128, recurrent widths multiples of 256) run the per-step recurrent products of both
 * attention LSTMs and of the decoder LSTM, and the recurrent-input gradients of their BPTT, as three bf16 MFMA terms
 * with fp32 accumulation (hi.hi + lo.hi + hi.lo per 16-wide K step): hi / lo bf16 shadows of the recurrent weights
 * are cast once per pass, the fp32 activations / gate gradients are split inside the kernels.  Everything else keeps
 * mode 2's kernels: t2_decoder_infer (the decode loop keeps its bit-exact stop frame), the encoders' t2_lstm_seq_*,
 * the attention kernels, and the persistent chains (which do not run in mode 2).  In modes 0 and 1 the switch changes
 * no result and no layout.  With it on in mode 2 the shadow arena of the forward workspace holds a lo plane behind each
 * of the six shadows (w16a ... wt16d then name the hi planes), so t2_decoder_layout_query / t2_decoder_bwd_layout_query
 * answer for the pair (precision mode, this switch), and NEITHER may change between a layout query and the calls that
 * use a workspace of that size.  A pass that does not meet the shape conditions runs the exact kernels. */
int t2_set_split_steps(int on);
int t2_get_split_steps(void);
/* Which kernel family the per-step LSTM launches of the decoder entry points (t2_decoder_forward, t2_decoder_backward,
 * t2_decoder_infer) took since the last reset: forward steps [0] exact fp32, [1] bf16 operands, [2] split-bf16;
 * recurrent-input gradient products [3] exact fp32, [4] bf16 operands, [5] split-bf16.  The attention LSTMs of both
 * streams share one launch.  The persistent chains are not per-step launches and t2_lstm_seq_* is not a decoder entry
 * point: neither is counted.  Host counters, no synchronisation; reset != 0 clears them after the read. */
int t2_step_counts(uint64_t* out_host /* [6] */, int reset);
/* 1 (default): teacher-forced passes run the decoder-LSTM chain on an internal side stream, one chunk of steps
 * apart from the attention chain (fork/join inside the call; the caller's stream semantics are unchanged).  0: one stream. */
int t2_set_overlap(int on);
/* Persistent chain kernels (csrc/chain.hip), bf16 mode, default dims, B <= 128, SMA: 1 (default; env T2_CHAIN=0 turns it
 * off) runs ALL steps of the attention chain (both attention LSTMs + attention; model.py:322-369) and of the decoder-LSTM
 * chain (model.py:371-373) of a teacher-forced pass in one launch each, with the recurrent weights resident in registers
 * and h / ctx / query partials exchanged between workgroups through write-through stores whose 16-byte units carry a step
 * tag the consumers validate (teacher-forced passes; the decode loop and the encoder chains use arrival counters).  They need
 * the whole device (256 co-resident workgroups): ONE process per GPU, as the reference runs (distributed.py:181-200).
 * A chain that could not make progress for 1 s gives up and leaves a non-zero status word in the workspace
 * (t2_decoder_layout.chain); 0: one launch per step and kernel, as in round 1. */
int t2_set_chain(int on);
int t2_get_chain(void);
/* The backward pass's persistent chains (csrc/chain_bwd.hip; in effect only while t2_set_chain is on): 1 (default; env
 * T2_CHAIN_BWD=0 turns it off) runs the BPTT of the decoder LSTM (autograd of model.py:371-373) in one launch per step
 * range, W_hh^T resident in registers.  t2_decoder_backward then writes status word 2 of the forward workspace's chain block. */
int t2_set_chain_bwd(int on);
/* bf16 mode only.  1 (default): a large GEMM whose extents are whole 128x128x64 tiles first writes bf16 copies of its
 * fp32 operands (K contiguous) into the caller's scratch and runs the bf16-source kernel on them (half the operand
 * bytes per MFMA; implicit-conv operands included).  0: always convert while staging through LDS.  Same rounding
 * of the operands either way; only the summation order inside a dot product differs. */
int t2_set_gemm_staging(int on);
/* 1 (default; env T2_GEMM_FOLD=0 turns it off): work that only touches a product's output is done where the product stores
 * it: the gate term of dDOUT in t2_decoder_backward is a rank-1 addend of the mel product's stores, and t2_conv_bn_backward's
 * weight-gradient product (or its split-K reduce) writes [Cout][Cin][K] directly.  0: the separate K = 1 product over dDOUT
 * and the re-layout kernel.  Every result has the same bits either way; the switch lets one process compare the two. */
int t2_set_gemm_fold(int on);
/* 1 (default; env T2_BN_FUSE=0 turns it off): t2_conv_bn_forward (training) and t2_conv_bn_backward finish their column
 * reductions in the prologue of the kernel that consumes them instead of in launches of their own: the pass over the
 * centred squares finishes the mean, one stage-2 launch finishes var / invstd and updates the running statistics, the
 * dz kernel finishes d(beta) / d(gamma) and leaves the slab partials of d(bias), so dz is not read again (where the
 * re-laid-out weights have no room for them, Cin*K < 64, the separate column sum runs).  0: a stage-2 launch per
 * reduction and one for the running statistics.  Every result has the same bits either way: the order of additions of a column sum does not change.
 * t2_bn_fuse_counts: layer calls since the last reset that took [0] the fused forward, [1] the fused backward with the
 * d(bias) partials, [2] the fused backward with the separate column sum (host counters). */
int t2_set_bn_fuse(int on);
int t2_get_bn_fuse(void);
int t2_bn_fuse_counts(uint64_t* out_host /* [3] */, int reset);
/* 1 (default; env T2_DG_HANDOFF=0 turns it off): in bf16 mode, where t2_decoder_backward runs a persistent backward chain and
 * the products behind it share one row-major bf16 copy of the chain's gate gradients dG, the chain stores those bf16 rows itself
 * (round to nearest even, what the cast produces) at the head of the stream's own dG region of the backward workspace, writes
 * no fp32 rows, and the cast of dG into the copy is not launched; the plan decides per pass (t2_decoder_pass_plan: dg_rows_d,
 * dg_rows_a).  0: fp32 rows and the casts.  Every gradient has the same bits either way.
 * t2_dg_handoff_counts: casts of a dG buffer since the last reset that [0] were skipped because the chain had stored the rows,
 * [1] ran (host counters; a pass without a shared copy counts nothing). */
int t2_set_dg_handoff(int on);
int t2_get_dg_handoff(void);
int t2_dg_handoff_counts(uint64_t* out_host /* [2] */, int reset);
/* dst[row*K + k] (bf16) = src[row*ld + k] rounded to nearest even: the cast the library makes of an fp32 operand before a bf16
 * product.  rows and K multiples of 64, ld a multiple of 4, both pointers 16-byte aligned. */
int t2_stage_bf16(const float* src, long ld, void* dst, int rows, int K, void* stream);
/* Makes `stream` wait for everything the library has queued on its internal side stream of the current device
 * (t2_decoder_bwd_args.defer_weight_grads). */
int t2_side_join(void* stream);
/* t2_decoder_backward calls since the last reset (host counters): [0] returned with the weight-gradient tail still on the
 * side stream (defer_weight_grads in effect), [1] finished everything on the caller's stream. */
int t2_defer_counts(uint64_t* out_host /* [2] */, int reset);

/* Model dimensions (hparams.py:55-95). */
typedef struct t2_dims {
    int n_mel;          /* n_mel_channels * n_frames_per_step (80) */
    int prenet_dim;     /* 256 */
    int enc_dim;        /* encoder_embedding_dim E (512) */
    int att_rnn_dim;    /* 1024 */
    int dec_rnn_dim;    /* 1024 */
    int att_dim;        /* attention_dim A (128) */
    int loc_filters;    /* 32 */
    int loc_kernel;     /* 31 */
    int attention_kind; /* T2_ATTN_* */
    float p_att_dropout, p_dec_dropout, p_prenet_dropout; /* 0.1, 0.1, 0.5 */
    int n_streams;      /* 2 = BERT_Tacotron2 (phone + sub-word, model.py:142-207); 1 = classic single-stream Tacotron2
                           (the API GTA.py:6,57-59 expects): decoder_rnn takes [att_h|ctx], projections [dec_h|ctx];
                           the *_sub weights / memory_sub / align_sub are then ignored (0 is read as 2) */
    float score_mask_value, score_mask_value_sub; /* energy written over positions past an item's length: the attention
                           modules' score_mask_value (attention.py:37,79; train.py:77-78 sets the phone stream's to the fp16
                           minimum for fp16 runs).  Taken verbatim when score_mask_given != 0; otherwise 0 = the default, -infinity */
    int score_mask_given;  /* 1: the two values above are meant as written (an intentional 0.0 included); 0 (a zero-initialised
                              struct): a 0.0 there stands for the default */
} t2_dims;

/* Parameters of Decoder (model.py:128-207), reference state_dict names in comments. */
typedef struct t2_attention_weights {
    const float* wq;        /* query_layer.linear_layer.weight        [A, att_rnn] */
    const float* wm;        /* memory_layer.linear_layer.weight       [A, E] */
    const float* v;         /* v.weight | v.linear_layer.weight       [1, A] */
    const float* loc_conv;  /* location_layer.location_conv.conv.weight   [F,2,Kc] (LSA) */
    const float* loc_dense; /* location_layer.location_dense.linear_layer.weight [A,F] (LSA) */
    /* GMMAttention (T2_ATTN_GMM): wq = mlp.0.weight [A, att_rnn]; wm exists in the state_dict but is not used */
    const float* mlp_b1;    /* mlp.0.bias   [A] */
    const float* mlp_w2;    /* mlp.2.weight [15, A] */
    const float* mlp_b2;    /* mlp.2.bias   [15] */
    /* DynamicConvolutionAttention (T2_ATTN_DCA): wq = W.weight [A, att_rnn], mlp_b1 = W.bias [A], mlp_w2 = V.weight [168, A],
     * loc_conv = F.weight [8,1,21], loc_dense = U.weight [A,8], v = v.weight [1,A]; memory_layer is not used */
    const float* dca_T;     /* T.weight [A, 8] */
    const float* dca_bT;    /* T.bias   [A] */
    const float* dca_P;     /* P buffer [11] (prior taps; no gradient) */
} t2_attention_weights;
typedef struct t2_lstm_weights { const float *w_ih, *w_hh, *b_ih, *b_hh; } t2_lstm_weights;
typedef struct t2_decoder_weights {
    const float *prenet_w1, *prenet_w2;          /* decoder.prenet.layers.{0,1}.linear_layer.weight */
    const float *prenet_sub_w1, *prenet_sub_w2;  /* decoder.prenet_bert.layers.{0,1}... */
    t2_lstm_weights att, att_sub;                /* decoder.attention_rnn, decoder.attention_rnn_bert */
    t2_attention_weights attn, attn_sub;         /* decoder.attention_layer, decoder.attention_layer_bert */
    t2_lstm_weights dec;                         /* decoder.decoder_rnn */
    const float *proj_w, *proj_b;                /* decoder.linear_projection.linear_layer.{weight,bias} */
    const float *gate_w, *gate_b;                /* decoder.gate_layer.linear_layer.{weight,bias} */
} t2_decoder_weights;

/* Saved-activation workspace of one decoder pass.  Offsets are in floats from `ws`.
 * Per-frame buffers are TIME-MAJOR [T,B,*] (one step's rows are contiguous: the per-step kernels
 * then touch one or two pages instead of B pages); the alignment-shaped ones stay [B,T,Tin]. */
typedef struct t2_decoder_layout {
    size_t total_floats;
    size_t x, p1, p2, p1s, p2s;      /* [T,B,n_mel], prenet activations [T,B,prenet] */
    size_t pm, pms;                   /* processed memory [B,Tin,A], [B,Tsub,A] */
    size_t prea, preas;               /* attention-LSTM input pre-activations [T,B,4*Ha] */
    size_t ga, gas;                   /* activated gates i,f,g,o [T,B,4*Ha] */
    size_t cna, cnas, ca, cas;        /* cell before / after dropout [T,B,Ha] */
    size_t din;                       /* [T,B, 2*Ha+2*E] = att_h | ctx | att_h_sub | ctx_sub */
    size_t psel, psels;               /* SMA p_t [B,T,Tin], [B,T,Tsub] */
    size_t wcum, wcums;               /* LSA cumulative weights per step [B,T,Tin], [B,T,Tsub]; GMM: mixture means [T,B,8] */
    size_t pred, gd, cnd, cd;         /* decoder LSTM: pre-activations, gates [T,B,4*Hd], cells [T,B,Hd] */
    size_t dout;                      /* [T,B, Hd+2*E] = dec_h | ctx | ctx_sub */
    size_t qs, qss;                   /* processed query per step [T,B,A] */
    size_t qpart;                     /* per-step scratch [2][Ha/8][B][A] */
    size_t w1t;                       /* decode loop: transposed first prenet layers [2][n_mel][P] */
    /* bf16-operand mode (sizes in floats = bf16 elements / 2): weight shadows [W_hh | W_ih[:,P:]] per stream,
     * decoder W_hh, their transposes for the backward pass, and bf16 copies of DIN / dec_h */
    size_t w16a, w16as, w16d, wt16a, wt16as, wt16d, din16, dh16;
    size_t gemm_ws; size_t gemm_ws_floats;
    size_t chain; size_t chain_floats;   /* exchange buffers of the persistent chain kernels (t2_set_chain): word 0 = status of
                                          * the attention chain, word 1 = status of the decoder-LSTM chain (0 = OK), then query
                                          * partials, fragment-ordered h / ctx buffers of both chains, and the decode loop's mel
                                          * fragments and arrival counters */
    size_t usave, usaves;             /* LSA: tanh(q + pm + location term) of every step [T,B,A,Tin4], [T,B,A,Tsub4] (Tin4 = Tin rounded up to 4) and ... */
    size_t locsave, locsaves;         /* ... the location features [T,B,Tin,F], [T,B,Tsub,F]: written by the persistent forward
                                       * chain for the persistent backward chain (size 0 for the other attention kinds) */
} t2_decoder_layout;

int t2_decoder_layout_query(const t2_dims* dims, int B, int T, int Tin, int Tsub, t2_decoder_layout* out);

/* Teacher-forced decoder pass — replaces Decoder.forward (model.py:392-428) incl. both Prenets
 * (:13-24), initialize_decoder_states (:223-270) and T calls of Decoder.decode (:322-390). */
typedef struct t2_decoder_fwd_args {
    int B, T, Tin, Tsub;
    const float* memory;      /* [B,Tin,E]   linear_converter output */
    const float* memory_sub;  /* [B,Tsub,E] */
    const int32_t* mem_lengths;  /* [B] or NULL (no mask, as in Decoder.inference) */
    const int32_t* sub_lengths;
    const float* mels;        /* [B,n_mel,T] teacher frames (reference layout) */
    float* mel_out;           /* [B,T,n_mel] */
    float* gate_out;          /* [B,T] */
    float* align;             /* [B,T,Tin] */
    float* align_sub;         /* [B,T,Tsub] */
    float* ws;                /* t2_decoder_layout.total_floats floats */
    int training;             /* LSTM-state dropout + SMA noise on (model.train()) */
    int prenet_dropout;       /* 1 = reference behaviour (always on, model.py:23); 0 = off for deterministic parity */
    uint64_t seed;
    int phase;                /* 0: the whole pass.  1: only the part that does not read the memories (bf16 shadows, teacher
                               * inputs, both prenets, hoisted attention-LSTM input GEMMs) — may run on another stream while
                               * the encoders are still working.  2: the rest, on a workspace phase 1 has filled (the caller
                               * orders the two calls, e.g. with an event). */
} t2_decoder_fwd_args;
int t2_decoder_forward(const t2_dims* dims, const t2_decoder_weights* w, const t2_decoder_fwd_args* a, void* stream);

/* Backward of t2_decoder_forward (the autograd graph PyTorch builds for Decoder.forward in the
 * reference).  Gradients are written (not accumulated) into `g`, which has the shapes of the
 * weights; d_memory / d_memory_sub receive the gradient wrt the encoder memories.
 * Both attention kinds; for LSA the location-layer gradient pointers of t2_attention_grads must be set. */
typedef struct t2_lstm_grads { float *w_ih, *w_hh, *b_ih, *b_hh; } t2_lstm_grads;
typedef struct t2_attention_grads { float *wq, *wm, *v, *loc_conv, *loc_dense, *mlp_b1, *mlp_w2, *mlp_b2, *dca_T, *dca_bT, *dca_P; } t2_attention_grads;
typedef struct t2_decoder_grads {
    float *prenet_w1, *prenet_w2, *prenet_sub_w1, *prenet_sub_w2;
    t2_lstm_grads att, att_sub;
    t2_attention_grads attn, attn_sub;
    t2_lstm_grads dec;
    float *proj_w, *proj_b, *gate_w, *gate_b;
} t2_decoder_grads;
typedef struct t2_decoder_bwd_layout {
    size_t total_floats;
    size_t ddout, ddin, dgd, dga, dgas, dctx, dctxs, dq, dqs, dv, dvs, dpm, dpms, carry, carrys;
    size_t carryc, carrycs, dlconv, dlconvs, dldense, dldenses;   /* LSA: cumulative carry, per-item location-layer gradients; GMM: mean carry, per-item db2 / dW2; zero-sized for SMA */
    size_t dcd, dca, dcas, partd, parta, dp2, dp2s, dp1, dmel_t, dgate_t, dg16a, dg16d, colsum_ws, gemm_ws, gemm_ws_floats;
    size_t chain, chain_floats;   /* exchange buffers of the persistent backward chains (gate-gradient fragments, K-split partials,
                                   * boundary carries); their status words are words 2 (decoder-LSTM chain) and 3 (attention chain)
                                   * of the forward workspace's t2_decoder_layout.chain block */
} t2_decoder_bwd_layout;
int t2_decoder_bwd_layout_query(const t2_dims* dims, int B, int T, int Tin, int Tsub, t2_decoder_bwd_layout* out);
typedef struct t2_decoder_bwd_args {
    int B, T, Tin, Tsub;
    const float* memory; const float* memory_sub;
    const float* align; const float* align_sub;     /* forward outputs [B,T,Tin], [B,T,Tsub] */
    const float* d_mel;        /* [B,T,n_mel] */
    const float* d_gate;       /* [B,T] */
    const float* d_align;      /* [B,T,Tin] or NULL */
    const float* d_align_sub;  /* [B,T,Tsub] or NULL */
    float* d_memory;           /* [B,Tin,E] out */
    float* d_memory_sub;       /* [B,Tsub,E] out */
    const float* ws;           /* workspace filled by t2_decoder_forward */
    float* bws;                /* t2_decoder_bwd_layout.total_floats floats of scratch */
    int training; int prenet_dropout; uint64_t seed;   /* must equal the forward call's */
    int defer_weight_grads;    /* 1 (with t2_set_overlap on, T >= 32; per-step launches and persistent chains alike): d_memory /
                                * d_memory_sub are complete on `stream` when the call returns, the weight gradients in `g` are
                                * still being written on the library's side stream (with persistent chains the library forks
                                * it after the chains and the decoder-LSTM weight gradients go there too); call
                                * t2_side_join(stream) before reading them or releasing ws / bws.  0: everything is ordered on
                                * `stream`.  t2_defer_counts tells which of the two a call did. */
} t2_decoder_bwd_args;
int t2_decoder_backward(const t2_dims* dims, const t2_decoder_weights* w, const t2_decoder_grads* g,
                        const t2_decoder_bwd_args* a, void* stream);

/* Autoregressive decode — replaces Decoder.inference (model.py:430-492) for any B.
 * Per-item stop rule: stop_index[b] = first t with sigmoid(gate) > threshold.
 * Runs until every item has stopped or max_steps.  Every `poll_every` steps a device counter is copied to pinned
 * memory behind an event and the host reads the copy made two polls earlier, so it only blocks when it is more than
 * 2*poll_every steps ahead of the GPU (the queue never drains); the loop therefore runs up to 3*poll_every steps past
 * the last stop.  Returns the number of steps run in *steps_run_host; frames after an item's stop index are
 * computed-but-meaningless.  poll_every <= 0: 16 steps, or 32 with the persistent kernels.
 * bf16 mode, default dims, B <= 32, SMA / LSA, t2_set_chain on: each polling interval is ONE persistent launch
 * (csrc/chain.hip, decode mode) running the whole step — attention LSTMs, attention, decoder LSTM, projections + stop
 * rule, both prenets — with every recurrent weight resident in registers; status word 0 of t2_decoder_layout.chain. */
typedef struct t2_decoder_infer_args {
    int B, Tin, Tsub, max_steps, poll_every;
    float gate_threshold;
    const float* memory; const float* memory_sub;
    const int32_t* mem_lengths; const int32_t* sub_lengths;   /* NULL as in the reference */
    float* mel_out;     /* [B,max_steps,n_mel] */
    float* gate_out;    /* [B,max_steps] */
    float* align;       /* [B,max_steps,Tin] */
    float* align_sub;   /* [B,max_steps,Tsub] */
    int32_t* stop_index;/* [B] device, -1 = never crossed */
    int32_t* done_count;/* [1] device scratch */
    float* ws;          /* layout for T = max_steps */
    int prenet_dropout; uint64_t seed;
    int* steps_run_host;
} t2_decoder_infer_args;
int t2_decoder_infer(const t2_dims* dims, const t2_decoder_weights* w, const t2_decoder_infer_args* a, void* stream);

/* out[b,c,t] = t < lengths[b] ? in[b,t,c] : fill — the layout change + masked_fill of
 * BERT_Tacotron2.parse_output (model.py:531-541).  lengths may be NULL. */
int t2_finalize_bct(const float* in_btc, float* out_bct, int B, int T, int C, const int32_t* lengths, float fill, void* stream);
int t2_mask_bt(float* x, int B, int T, const int32_t* lengths, float fill, void* stream);

/* ---- Encoder / Postnet building blocks (channels-last frames x[B*T, C]) --------------------------
 * One Conv1d(k, same padding) + BatchNorm1d + activation + dropout layer, forward and backward:
 * replaces one nn.Sequential(ConvNorm, BatchNorm1d) + torch.tanh/F.relu + F.dropout of
 * Postnet.forward (model.py:65-70) / Encoder.forward (model.py:97-99).  act: 0 none, 1 relu, 2 tanh.
 * Dropout keep-bit index = (b*T + t)*Cout + c at `site`.  Saved tensors (z, mean, invstd) are
 * caller-owned and passed back to the backward call. */
typedef struct t2_conv_bn_args {
    int B, T, Cin, Cout, K;
    const float* x;                    /* [B*T, Cin] */
    const float* w; const float* bias; /* conv.weight [Cout,Cin,K], conv.bias [Cout] */
    const float* gamma; const float* beta;   /* BatchNorm weight / bias */
    float* run_mean; float* run_var;   /* running statistics: updated in training, read in eval */
    int training; float eps; int act; float drop_p; uint64_t seed; uint32_t site;
    const float* residual;             /* optional, added to the output (mel + postnet(mel), model.py:558) */
    float* z; float* mean; float* invstd; float* var;   /* saved: [B*T,Cout], [Cout] x3 */
    float* y;                          /* [B*T, Cout] */
    float* ws; size_t ws_floats;       /* scratch >= Cout*Cin*K + 128*Cout floats; anything beyond is used for bf16 operand staging (bf16 mode) */
    /* Optional bf16 hand-offs through a stack of layers (all zero: every GEMM operand is cast by the GEMM layer, as before).
     * y16: also write y as bf16 [B*T, Cout] (round to nearest even), for the next layer's x16.  handoff != 0, bf16 mode: the
     * conv product reads x16 (the previous layer's y16, [B*T, Cin]; may be NULL) and weights re-laid-out straight into bf16
     * instead of casting them, wherever that leaves the product's kernel and split-K unchanged (t2_conv_handoff_plan):
     * results are bit-identical either way.  Ignored in the other precision modes. */
    const void* x16; void* y16; int handoff;
} t2_conv_bn_args;
int t2_conv_bn_forward(const t2_conv_bn_args* a, void* stream);
typedef struct t2_conv_bn_bwd_args {
    int B, T, Cin, Cout, K;
    const float* x; const float* w; const float* gamma; const float* beta;
    const float* z; const float* mean; const float* invstd;
    int training; float eps; int act; float drop_p; uint64_t seed; uint32_t site;
    const float* dy;                   /* [B*T, Cout] */
    float* dw; float* dbias; float* dgamma; float* dbeta;
    float* dx; int dx_accumulate;      /* [B*T, Cin] or NULL */
    float* ws; size_t ws_floats;       /* scratch >= B*T*Cout + Cout*Cin*K + 128*Cout + split-K / bf16 staging space */
    /* Optional, as in t2_conv_bn_args: handoff != 0 (bf16 mode) writes dz once as bf16 for both products and the flipped
     * weights straight into bf16; x16 is the bf16 copy of x saved by the forward pass (NULL: x is cast). */
    const void* x16; int handoff;
} t2_conv_bn_bwd_args;
int t2_conv_bn_backward(const t2_conv_bn_bwd_args* a, void* stream);

/* nn.Embedding forward / weight gradient (model.py:501-502,546,551); ids are int64. */
int t2_embedding_forward(const int64_t* ids, const float* table, float* out, int rows, int dim, void* stream);
int t2_embedding_backward(const int64_t* ids, const float* dout, float* dtable, int rows, int dim, int vocab, void* stream);

/* LSTM recurrences over whole sequences with precomputed input pre-activations (time-major
 * [T,B,4H], biases included): the packed BiLSTM of Encoder.forward (model.py:104-112; lengths given)
 * or the unpacked one of Encoder.inference (:122-123; lengths NULL).  Up to 4 independent
 * sequences ("streams": directions / encoders) advance together, one kernel launch per time step.
 * Outputs beyond an item's length are zero and its state stays zero, which is exactly
 * pack_padded_sequence / pad_packed_sequence semantics for both directions. */
typedef struct t2_lstm_seq_args {
    int nstreams, B, T, H;
    const float* pre[4];     /* [T,B,4H] */
    const float* w_hh[4];    /* [4H,H] */
    int reverse[4];
    const int32_t* lengths;  /* [B] or NULL */
    float* h[4]; long ldh;   /* [T,B,*]: row stride ldh (lets two directions share one [T,B,2H] buffer) */
    float* c[4];             /* [T,B,H] saved cells */
    float* gates[4];         /* [T,B,4H] saved activated gates */
    float* ws; size_t ws_floats;   /* optional exchange space (t2_lstm_seq_chain_ws_floats): with it, H = 256, <= 2 streams,
                                      B <= 128 and t2_set_chain on, ALL steps run in one persistent launch (csrc/chain_enc.hip,
                                      exact fp32: the same arithmetic as the per-step kernels up to summation order) */
} t2_lstm_seq_args;
/* floats of exchange space the persistent BiLSTM chain needs (backward != 0: its BPTT, handed over as t2_lstm_seq_bwd_args.ws) */
size_t t2_lstm_seq_chain_ws_floats(int nstreams, int B, int H, int backward);
int t2_lstm_seq_forward(const t2_lstm_seq_args* a, void* stream);
typedef struct t2_lstm_seq_bwd_args {
    int nstreams, B, T, H;
    const float* w_hh[4]; int reverse[4];
    const float* h[4]; long ldh; const float* c[4]; const float* gates[4];
    const float* dh[4]; long lddh;   /* gradient on the outputs, [T,B,*] with row stride lddh; dh past an item's length must be
                                        finite: it is multiplied by the zero saved gates, not masked */
    float* dpre[4];                  /* out: gradient wrt pre-activations [T,B,4H] */
    float* dw_hh[4];                 /* out: [4H,H] */
    float* ws; size_t ws_floats;     /* scratch >= nstreams*(B*H + 8*B*H) + split-K space; also the persistent chain's exchange
                                        space when >= t2_lstm_seq_chain_ws_floats(nstreams, B, H, 1) */
} t2_lstm_seq_bwd_args;
int t2_lstm_seq_backward(const t2_lstm_seq_bwd_args* a, void* stream);

/* General GEMM with the full descriptor (see t2_gemm); crow_mod/crow_mul permute output rows:
 * row m is written to (m % crow_mod) * crow_mul + m / crow_mod (0 = identity).
 * act: 0 none, 1 relu, 2 tanh, 3 gelu (the exact form 0.5 x (1 + erf(x / sqrt 2)), forward only: the conv / BatchNorm
 * layers above take 0..2); any other value is refused. */
typedef struct t2_gemm_args {
    const float* A; const float* B; float* C; int M, N, K;
    long sam, sak, sbn, sbk, ldc; int batch; long bsA, bsB, bsC;
    float alpha, beta; const float* bias; int act; int crow_mod; long crow_mul;
    float* ws; size_t ws_bytes; int splitk;
} t2_gemm_args;
int t2_gemm_ex(const t2_gemm_args* a, void* stream);
/* Measurement (bench.py): average milliseconds of `reps` launches of this product on `stream`, bracketed by HIP events —
 * ms_total as t2_gemm_ex runs it (fp32 operands in: bf16 staging casts included), ms_kernel with both bf16 operand copies
 * made beforehand (the matrix kernel and its split-K reduce alone).  bf16 mode or split-bf16 mode (there: the hi / lo
 * staging, resp. both hi / lo copies made beforehand; scratch for 6 bytes per operand element), M, N multiples of 128, K of
 * 64, scratch given; refused in mode 0, and for a product that the mode in force does not run on a bf16-source kernel
 * reading both copies (t2_gemm_plan tells): nothing else is timed under these names. */
int t2_prof_gemm(const t2_gemm_args* a, int reps, float* ms_total, float* ms_kernel, void* stream);
/* What the GEMM layer would do with a product, decided on the host: launches nothing, needs no device, answers for the
 * precision mode, split threshold and staging switch in force.  The pointers of `a` are looked at for their alignment only.
 * opts (nullable) carries what t2_gemm_args cannot: an implicit-conv operand, fp32_only, and bf16 copies the caller would
 * hand over (a16 / b16 != 0: a copy with leading dimension lda16 / ldb16, k-major or K-contiguous; split16: the copies are
 * hi / lo parts in the split-bf16 layout).  A product the GEMM layer refuses returns its error code and message. */
enum { T2_GEMM_F32_64 = 0, T2_GEMM_F32_128, T2_GEMM_BF16CONV, T2_GEMM_SRC128, T2_GEMM_SRC256, T2_GEMM_SRC256KM };   /* kernel */
enum { T2_GEMM_OPERAND_FP32 = 0, T2_GEMM_OPERAND_STAGED, T2_GEMM_OPERAND_CALLER };                                  /* a_src, b_src */
typedef struct t2_gemm_plan_opts {
    int conv_a, conv_b, conv_T, conv_C, fp32_only;
    int a16, b16; long lda16, ldb16; int a16_kmajor, b16_kmajor, split16;
} t2_gemm_plan_opts;
typedef struct t2_gemm_plan_info {
    int kernel; const char* name;        /* name: as T2_GEMM_LOG prints it, "x3" in front when split (static string) */
    int split;                           /* the kernel reads hi / lo copies, K' = 3K */
    int splitk, kchunks;                 /* split-K factor; 16-wide K-chunks per split */
    int a_src, b_src;                    /* the kernel reads the fp32 operand, a copy staged into the scratch, the caller's copy */
    size_t stage_bytes_a, stage_bytes_b; /* scratch the staged copies take in front of the split-K partials */
} t2_gemm_plan_info;
int t2_gemm_plan(const t2_gemm_args* a, const t2_gemm_plan_opts* opts, t2_gemm_plan_info* out);
/* What a pass would do with a persistent chain (csrc/chain_plan.hip), decided on the host: launches nothing, needs no device,
 * never asks for the per-GPU claim — the three things the library asks the device and the process come as arguments (cus =
 * compute units, claimed = this process holds the device's persistent kernels, no_resident = T2_CHAIN_NO_RESIDENT is set).
 * kind: 0 decoder-LSTM chain, 1 SMA / 2 LSA attention chain (dec = 1: the decode loop), 3 encoder BiLSTM chain (NS =
 * directions, H; ws_floats = the caller's exchange space).  H is the chain's own hidden size; an attention chain's shape
 * carries the pass's P, M and Hd.  ws_floats: the exchange space of the pass (chain_floats of the layout queries), 0 = exactly
 * what this chain needs; the offsets of the parts a chain carves from the back of the space depend on it.  A refusal is no
 * error: covered = 0, reason / reason_text say why, and the pass takes the per-step launches.  Parts with bytes == 0 do not
 * exist for the chain; clear_*: what every launch zeroes first; pass_clear_bytes (forward): bytes from the head of the space
 * that the pass zeroes once, by mode (status words only / teacher-forced / decode loop). */
enum { T2_CHAIN_LSTM = 0, T2_CHAIN_SMA, T2_CHAIN_LSA, T2_CHAIN_ENC };                                               /* kind */
enum { T2_CHAIN_FORWARD = 0, T2_CHAIN_BACKWARD };                                                                   /* direction */
enum { T2_CHAIN_OK = 0, T2_CHAIN_REFUSE_SHAPE, T2_CHAIN_REFUSE_NO_INSTANCE, T2_CHAIN_REFUSE_DEVICE, T2_CHAIN_REFUSE_CLAIM,
       T2_CHAIN_REFUSE_QUERY_PART, T2_CHAIN_REFUSE_LDS, T2_CHAIN_REFUSE_LSA_RESIDENT, T2_CHAIN_REFUSE_SHORT_MEMORY,
       T2_CHAIN_REFUSE_LSA_SPLIT, T2_CHAIN_REFUSE_NO_SAVED_TILES, T2_CHAIN_REFUSE_WORKSPACE, T2_CHAIN_REFUSALS };    /* reason */
enum { T2_CHAIN_PARTS = 11 };               /* status, Q, X, XD, XM, cnt, PB, PBC, DQX, CARRYX, WDT (part_name) */
typedef struct t2_chain_shape {
    int kind, dec, NS, B, H, E, A, P, M, Hd, F, Kc, Tin[2];
    int saved_tiles;                         /* LSA backward: the forward chain left its tanh tile and location features */
    size_t ws_floats;
} t2_chain_shape;
typedef struct t2_chain_plan_info {
    int covered, reason; const char* reason_text;            /* static strings */
    int instance; const char* instance_name; int grid; size_t lds_bytes;
    int UT, RT, CS, MT, lds_Tc, lds_Tin, lds_Jp, lds_Jm, Jp[2], Jm[2];
    size_t q_bytes, total_bytes, ws_bytes;                   /* ws_bytes: the space the offsets were laid out in */
    size_t part_off[T2_CHAIN_PARTS], part_bytes[T2_CHAIN_PARTS]; const char* part_name[T2_CHAIN_PARTS];
    size_t clear_off, clear_bytes, pass_clear_bytes[3];
} t2_chain_plan_info;
int t2_chain_plan(const t2_chain_shape* shape, int direction, int cus, int claimed, int no_resident, t2_chain_plan_info* out);
/* What a decoder pass would do (csrc/decoder_plan.hip), decided on the host: launches nothing, needs no device, never asks for
 * the per-GPU claim.  Everything the library reads from the process and the device comes in env: the precision mode (0 fp32,
 * 1 bf16, 2 split-bf16), the switches (t2_set_split_steps, t2_set_chain, t2_set_chain_bwd, t2_set_overlap), cus / claimed /
 * no_resident as for t2_chain_plan, and (backward) saved_tiles = the forward pass ran the LSA chain, so that its workspace
 * holds the tanh tiles.  T: frames (decode loop: max_steps); defer_weight_grads: backward only; poll_every: decode loop only.
 * The result holds every decision of the pass (DESIGN.md section 3 has the rule of each field): both workspace layouts
 * (bwd_layout: backward only), the recurrent steps (use16 / split), the persistent chains (chain_a: attention chain, or the
 * whole decode loop; chain_b: decoder-LSTM chain; asked = the switches, the step mode and the attention kind let the pass plan
 * one, on = it runs, reason / reason_text otherwise; t2_chain_plan has the chain's own details), whether the chains overlap on
 * the side stream and the bounds of the step ranges they hand to each other, what the pass clears in its exchange space
 * (0 status words, 1 teacher-forced, 2 decode loop), over how many status words the outputs get the abort poison, the poll
 * interval, and the GEMM scratch as named parts in bytes from its start (bytes == 0: no such part): the bf16 copy of the
 * decoder LSTM's W_ih or W_ih^T (pre16), the shared bf16 copy of dG (share), the rest.  Backward: scratch is the carve while
 * the chains run (ddin_ws: what a range's dDIN product works in; chunk_cast: dG is cast range by range), tail_scratch the
 * carve of the leaf tail (tail_share); dec_wgrads says where the decoder-LSTM weight gradients are issued (0 in the range
 * loop on chain B's stream, 1 on the tail's stream; dec_wgrads_staged: their dG copy is already filled), tail_on_side the
 * tail's stream, nsplit the position splits of the per-step attention backward, dq_parts the partials the tail folds.
 * env.dg_handoff (t2_set_dg_handoff), env.gemm_staging (t2_set_gemm_staging) and dg_rows_d / dg_rows_a: the decoder-LSTM chain /
 * the attention chain stores its dG as bf16 rows at the head of bwd_layout.dgd / dga and dgas and the cast into the shared copy
 * is skipped: the switch on, the chain on, chunk_cast / tail_share, and every product that reads that dG takes the copy (whole
 * tiles, also of the products over B*T - B rows: B a multiple of 64); the carves are the same either way. */
enum { T2_PASS_FORWARD = 0, T2_PASS_BACKWARD, T2_PASS_INFER };                                                       /* pass */
enum { T2_PASS_MAX_BOUNDS = 64 };
typedef struct t2_pass_env {
    int precision, split_steps, chain, chain_bwd, overlap, cus, claimed, no_resident, saved_tiles, dg_handoff, gemm_staging;
} t2_pass_env;
typedef struct t2_pass_chain {
    int asked, on, reason; const char* reason_text;          /* static strings */
    int instance; const char* instance_name; int grid;
} t2_pass_chain;
typedef struct t2_scratch_carve {
    size_t w_ih16_off, w_ih16_bytes, dg16_off, dg16_bytes, rest_off, rest_bytes, total_bytes;
} t2_scratch_carve;
typedef struct t2_decoder_pass_plan_info {
    t2_decoder_layout layout; t2_decoder_bwd_layout bwd_layout;
    int use16, split, pre16;
    t2_scratch_carve scratch;
    t2_pass_chain chain_a, chain_b;
    int chained, clear, saves_tiles, overlap;
    int nbounds, bounds[T2_PASS_MAX_BOUNDS];
    int poison_words, poll; size_t shadow_floats;            /* shadow_floats: the decode loop's weight shadows and input rows */
    int defer, share, chunk_cast; size_t ddin_ws_off, ddin_ws_bytes;
    int dec_wgrads, dec_wgrads_staged, tail_on_side, tail_share;
    t2_scratch_carve tail_scratch;
    int nsplit, lsa_chain, dq_parts;
    int dg_rows_d, dg_rows_a;                                /* backward: a chain stores dG as bf16 rows, no cast (t2_set_dg_handoff) */
} t2_decoder_pass_plan_info;
int t2_decoder_pass_plan(const t2_dims* dims, int pass, int B, int T, int Tin, int Tsub, const t2_pass_env* env, int defer_weight_grads,
                         int poll_every, t2_decoder_pass_plan_info* out);
/* The hand-over rule of the conv stacks for the product (a, opts), opts->a16 / b16 naming the copies on offer: *taken = 1
 * and *out = the plan with them iff the product without copies stages every operand a copy is offered for, and with them
 * takes every copy and keeps its kernel, split-K factor and K-chunks per split; otherwise *taken = 0 and *out = the plan
 * without copies.  Launches nothing. */
int t2_conv_handoff_plan(const t2_gemm_args* a, const t2_gemm_plan_opts* opts, int* taken, t2_gemm_plan_info* out);
/* out[n] = sum_m x[m*ld + n]; scratch >= 64*N floats */
int t2_colsum(const float* x, long ld, int M, int N, float* out, float* scratch, void* stream);
int t2_mask_btc(float* x, int B, int T, int C, const int32_t* lengths, float fill, void* stream);

/* ---- Soft-DTW (checkpoint scoring) ---------------------------------------------------------------
 * Replaces the reference's soft_dtw_cuda.py: compute_softdtw_cuda (:34-75) / compute_softdtw_backward_cuda (:78-111),
 * the host loops it uses above 1024 frames (:185-239), and SoftDTW._euclidean_dist_func (:320-329) with its autograd
 * graph.  Indices are 1-based over a padded (N+2) x (M+2) grid, R[0,0] = 0, every other border cell +infinity;
 * R[i,j] = D[i-1,j-1] + softmin_gamma(R[i-1,j-1], R[i-1,j], R[i,j-1]); cells with 0 < bandwidth < |i - j| are skipped.
 * One workgroup per pair walks a skewed wavefront; a cell is a fixed function of its neighbours, so results are
 * bit-identical whatever the batch, the padding and the partition.  N, M <= 8192 each, any d >= 1, gamma > 0; larger
 * sizes are refused (there is no host detour).
 * Per-pair lengths (an extension, the reference has none): x_lengths[b] = n_b <= N, y_lengths[b] = m_b <= M (both or
 * neither; NULL = N, M).  Pair b is the problem x[b,:n_b], y[b,:m_b]: its value is R[n_b,m_b], E and the gradients are
 * zero in the padding.  A length below 1 gives value +infinity and zero gradients.
 * An unreachable end cell (0 < bandwidth < |n_b - m_b|) gives value +infinity and an all-zero E.
 *
 * t2_softdtw_plan is pure (no device): the partition of a pair and the scratch the calls below need.  Fails, with the
 * limit in the message, for N or M outside 1..8192, B < 1 and gamma <= 0. */
typedef struct t2_softdtw_plan_info {
    int threads;          /* per workgroup: whole 64-lane waves, at most 1024 */
    int rows_per_thread;  /* consecutive rows a thread owns: 1, 2, 4 or 8, the smallest with rows_per_thread * 1024 >= N */
    int passes;           /* of the wavefront: M + ceil(N / rows_per_thread) - 1 */
    size_t d_floats;      /* internal distance scratch Ds: B * passes * threads * rows_per_thread */
    size_t r_floats;      /* stored R (same layout); 0 when need_grad == 0: the forward then keeps O(N) state only */
    size_t e_floats;      /* E, [B,N,M] row-major; 0 when need_grad == 0 */
} t2_softdtw_plan_info;
int t2_softdtw_plan(int B, int N, int M, float gamma, int need_grad, t2_softdtw_plan_info* out);
/* Ds = pairwise squared Euclidean distances sum_c (x[b,i,c] - y[b,j,c])^2 (c ascending, fused multiply-adds), in the
 * internal layout [B][passes][threads][rows_per_thread] the wavefront reads with adjacent lanes on adjacent addresses. */
typedef struct t2_softdtw_dist_args {
    int B, N, M, d;
    const float* x;       /* [B,N,d] */
    const float* y;       /* [B,M,d] */
    float* Ds;            /* d_floats */
} t2_softdtw_dist_args;
int t2_softdtw_dist(const t2_softdtw_dist_args* a, void* stream);
/* value[b] = R[n_b, m_b].  Exactly one of D (a caller's distance matrix, row-major [B,N,M]: SoftDTW(dist_func=...)) and
 * Ds (t2_softdtw_dist's output) is given.  R == NULL: nothing but value is written.  R given (r_floats): R is stored
 * for t2_softdtw_backward. */
typedef struct t2_softdtw_fwd_args {
    int B, N, M;
    float gamma, bandwidth;           /* bandwidth 0 = off (SoftDTW(bandwidth=None)) */
    const float* D; const float* Ds;
    const int32_t* x_lengths; const int32_t* y_lengths;   /* [B] each, or both NULL */
    float* R;
    float* value;                     /* [B] */
} t2_softdtw_fwd_args;
int t2_softdtw_forward(const t2_softdtw_fwd_args* a, void* stream);
/* E[b,i,j] = d value[b] / d D[b,i,j], [B,N,M] row-major, from the R a forward call with the same arguments stored
 * (soft_dtw_cuda.py:158-174 without the multiplication by grad_output).  Enqueues a memset of E before the kernel. */
typedef struct t2_softdtw_bwd_args {
    int B, N, M;
    float gamma, bandwidth;
    const float* D; const float* Ds;
    const int32_t* x_lengths; const int32_t* y_lengths;
    const float* R;
    float* E;
} t2_softdtw_bwd_args;
int t2_softdtw_backward(const t2_softdtw_bwd_args* a, void* stream);
/* Gradient of value through the Euclidean distances, G = grad_out[b] * E:
 * dX[b,i,:] = 2 sum_j G[b,i,j] (x[b,i,:] - y[b,j,:]), dY[b,j,:] = -2 sum_i G[b,i,j] (x[b,i,:] - y[b,j,:]); sums in
 * ascending order, no atomics. */
typedef struct t2_softdtw_dist_bwd_args {
    int B, N, M, d;
    const float* x; const float* y;
    const float* E;                   /* [B,N,M] */
    const float* grad_out;            /* [B] */
    const int32_t* x_lengths; const int32_t* y_lengths;
    float* dX; float* dY;             /* [B,N,d], [B,M,d] */
} t2_softdtw_dist_bwd_args;
int t2_softdtw_dist_backward(const t2_softdtw_dist_bwd_args* a, void* stream);

/* ---- SSIM (the loss term of loss_function.py:10,24) -------------------------------------------------
 * Replaces the reference's ssim.py:17-37 (_ssim: five grouped conv2d with a Gaussian window under zero padding of ws/2,
 * the element-wise algebra of S and its mean) and the autograd graph behind it.  Images are N = B*C planes of H x W
 * fp32; every image carries its plane, row and column strides in elements, and one of its two inner strides must be 1
 * (an axis of size 1 counts).  The lane axis of the kernels is the one along which x is contiguous, so [B,1,80,T] and
 * the transposed view of a [B,T,80] buffer both run without a copy.  taps: the ws 1-D taps (ssim.py:7-9 as it rounds
 * them); ws odd, 1..31.  Moments, the subtraction E[xx] - mu^2 and the algebra of S and its derivatives are fp64, so
 * value and gradient stay accurate where the reference's fp32 statement cancels (log-mel silence).  Sums are taken in a
 * fixed order without atomics: results are bit-identical from run to run.  No call synchronises with the host.
 * The coefficient maps a forward call stores for the backward are fp64 too: the three terms of the gradient cancel.
 *
 * t2_ssim_plan (ssim.py:17-37) is pure (no device): the tiling and the scratch the calls need.  need_grad: 0 = none,
 * 1 = dx, 2 = dy, 3 = both.  Fails, naming the argument, for an even ws, ws > 31, need_grad outside 0..3, non-positive
 * sizes, and N*H*W beyond 2^31-1. */
typedef struct t2_ssim_plan_info {
    int tile_h, tile_w;       /* outputs per workgroup: rows x lane-axis columns */
    int tiles_h, tiles_w;     /* tiles per plane with W as the lane axis */
    long partials;            /* N * tiles_h * tiles_w: one fp64 partial sum per tile and plane */
    long partials_t;          /* the same count when H is the lane axis (x contiguous along H) */
    size_t partial_bytes;     /* scratch for the partials: 8 * max(partials, partials_t) */
    size_t map_bytes;         /* stored fp64 coefficient maps for the backward: 8 * N*H*W * (0, 3 for one gradient, 4 for both) */
    size_t lds_fwd_bytes, lds_bwd_bytes;   /* LDS per workgroup of the two kernels */
} t2_ssim_plan_info;
int t2_ssim_plan(int N, int H, int W, int ws, int need_grad, t2_ssim_plan_info* out);
typedef struct t2_ssim_image {
    float* p;
    long plane_stride, row_stride, col_stride;   /* in elements */
} t2_ssim_image;
/* ssim.py:17-37.  S per pixel, then value[0] = mean of S over everything (size_average=True, :34-35) and / or
 * items[b] = mean over C*H*W of item b (:36-37); map (nullable p) receives S itself.  need_grad != 0 also stores the
 * coefficient maps (coef, map_bytes) that t2_ssim_backward filters. */
typedef struct t2_ssim_fwd_args {
    int B, C, H, W, ws, need_grad;
    t2_ssim_image x, y, map;
    const float* taps;        /* [ws] */
    void* partial;            /* partial_bytes */
    void* coef;               /* map_bytes; NULL iff need_grad == 0 */
    float* value;             /* [1] or NULL */
    float* items;             /* [B] or NULL */
} t2_ssim_fwd_args;
int t2_ssim_forward(const t2_ssim_fwd_args* a, void* stream);
/* Gradient of ssim.py:17-37 from the coef a forward call with the same x, y, ws and need_grad stored:
 * dx(p) = g * (F[a - 2 b mu1 - c mu2](p) + 2 x(p) F[b](p) + y(p) F[c](p)), F the same zero-padded window, a, b, c the
 * derivatives of S by mu1, sigma1^2 and sigma12; dy the same with the images' roles swapped.  g = grad[0] / (N*H*W)
 * (per_item == 0) or grad[b] / (C*H*W) (per_item != 0), read on the device.  dx.p or dy.p may be NULL (not both). */
typedef struct t2_ssim_bwd_args {
    int B, C, H, W, ws, need_grad, per_item;
    t2_ssim_image x, y, dx, dy;
    const float* taps;
    const void* coef;         /* map_bytes, as the forward call left them */
    const float* grad;        /* [1], or [B] with per_item */
} t2_ssim_bwd_args;
int t2_ssim_backward(const t2_ssim_bwd_args* a, void* stream);

/* ---- BERT sentence encoder (text ids -> [CLS] vector) -----------------------------------------------
 * Replaces the CPU forward behind the reference's data_utils.py: get_embedding_cls (:28-46): BertModel (embeddings,
 * `layers` post-LayerNorm transformer layers, last hidden state; the pooler is not part of it), inference only.  What is
 * computed is BertModel(input_ids, attention_mask = the sentence's own tokens, token_type_ids = 0): every token attends
 * to every token of its own sentence (INTEGRATION.md says why this and not the positional call as the installed
 * transformers release reads it).  Exact fp32 on the matrix cores, whatever t2_set_precision says.
 *
 * A ragged batch is packed, not padded: token rows [total, hidden] addressed through cu_seqlens [B+1] (int32, device;
 * cu_seqlens[0] = 0, cu_seqlens[B] = total).  No mask tensor exists; keys beyond a sentence's length are never read.
 * Sums are taken in a fixed order without atomics, and a sentence's result does not depend on its place in the batch.
 * The kernels do not check ids against the tables: callers validate 0 <= id < vocab on the host (bert.py does).
 *
 * Packed weights, one device buffer of packed_floats floats, made by t2_bert_pack from 5 + 16 * layers device tensors in
 * this order (state-dict names, row-major [out, in] matrices as torch keeps them):
 *   embeddings.word_embeddings.weight [vocab, H], embeddings.position_embeddings.weight [max_pos, H],
 *   embeddings.token_type_embeddings.weight [type_vocab, H], embeddings.LayerNorm.weight, embeddings.LayerNorm.bias,
 *   then per layer i (encoder.layer.i.): attention.self.query.weight, .bias, attention.self.key.weight, .bias,
 *   attention.self.value.weight, .bias, attention.output.dense.weight, .bias, attention.output.LayerNorm.weight, .bias,
 *   intermediate.dense.weight [I, H], .bias, output.dense.weight [H, I], .bias, output.LayerNorm.weight, .bias.
 * Query, key and value are stored as one [3H, H] matrix with a [3H] bias. */
typedef struct t2_bert_config {
    int hidden, layers, heads, intermediate, vocab, max_pos, type_vocab;
    float ln_eps;             /* 1e-12 for BERT: the LayerNorms centre before they square */
} t2_bert_config;
typedef struct t2_bert_plan_info {
    size_t packed_floats;     /* the packed weight buffer */
    size_t workspace_bytes;   /* residual stream, fused QKV rows, context rows, FFN rows; the [B, .] rows of the CLS tail */
    int launches;             /* kernel launches of one forward call, each product counted as one */
} t2_bert_plan_info;
/* Pure (no device).  cls_only: the forward will be called without out_hidden, so the last layer runs its query
 * projection, attention, output projection, FFN and LayerNorms for the B [CLS] rows only.  Fails, naming the argument,
 * for a head dimension other than 64, hidden not a multiple of 64 or above 1024, intermediate not a multiple of 64,
 * max_len outside 1..min(512, max_pos), B < 1, and total_tokens outside B..B*max_len. */
int t2_bert_plan(const t2_bert_config* cfg, int B, long total_tokens, int max_len, int cls_only, t2_bert_plan_info* out);
int t2_bert_pack(const t2_bert_config* cfg, const float* const* tensors_dev, int n_tensors, float* packed, void* stream);
typedef struct t2_bert_fwd_args {
    int B; int total_tokens; int max_len;   /* max_len: an upper bound of every sentence's length (sizes grids and LDS) */
    const float* packed;
    const int32_t* ids;                     /* [total_tokens] */
    const int32_t* cu_seqlens;              /* [B + 1] */
    float* out_hidden;                      /* [total_tokens, H] last hidden state, or NULL: the CLS-only last layer */
    float* out_cls;                         /* [B, H] row cu_seqlens[b] of the last hidden state; NULL only with out_hidden */
    void* ws; size_t ws_bytes;              /* workspace_bytes of the plan with cls_only = (out_hidden == NULL) */
} t2_bert_fwd_args;
int t2_bert_forward(const t2_bert_config* cfg, const t2_bert_fwd_args* a, void* stream);
/* The kernels one by one (tests).  out[row] = LayerNorm(word[ids[row]] + type[0] + pos[row - cu_seqlens[b]]) for the rows
 * of sentence b; one wave per row, H a multiple of 64 up to 1024. */
typedef struct t2_bert_embed_ln_args {
    int B, total_tokens, max_len, H; float eps;
    const int32_t* ids; const int32_t* cu_seqlens;
    const float* word; const float* pos; const float* type; const float* ln_w; const float* ln_b;
    float* out;                             /* [total_tokens, H] */
} t2_bert_embed_ln_args;
int t2_bert_embed_ln(const t2_bert_embed_ln_args* a, void* stream);
/* out[row] = LayerNorm(x[row]) over H, rows [rows, H] contiguous; out == x runs in place. */
typedef struct t2_bert_layernorm_args {
    int rows, H; float eps;
    const float* x; const float* ln_w; const float* ln_b; float* out;
} t2_bert_layernorm_args;
int t2_bert_layernorm(const t2_bert_layernorm_args* a, void* stream);
/* out = softmax(Q K^T / 8) V per sentence and head, head dimension 64, sentence lengths 1..max_len <= 512.  q, k, v: the
 * first element of head 0 in row 0, row strides ldq, ldk, ldv in floats (multiples of 4, pointers 16-byte aligned): the
 * fused rows [total, 3H] are q = qkv, k = qkv + H, v = qkv + 2H, all with stride 3H.  nq_first_only == 0: q holds the
 * packed rows, out [total, ldo] too.  nq_first_only != 0: one query per sentence; q holds B rows (row b = the query of
 * sentence b, against the keys and values of the packed rows) and out is [B, ldo]. */
typedef struct t2_bert_attention_args {
    int B, heads, total_tokens, max_len, nq_first_only;
    const float* q; const float* k; const float* v; long ldq, ldk, ldv;
    const int32_t* cu_seqlens;
    float* out; long ldo;
} t2_bert_attention_args;
int t2_bert_attention(const t2_bert_attention_args* a, void* stream);

/* ---- HiFi-GAN generator (mel spectrogram -> waveform) ----------------------------------------------
 * Replaces the reference's hifigan_infer/hifigan_model.py: Generator.forward (:100-116), ResBlock1.forward (:35-42),
 * ResBlock2.forward (:63-68), as inference.py:172-206, best_checkpoint.py:191-228, streamlitNews.py:115-160 and
 * logger.py:19-33 call it.  Unlike the rest of this header the vocoder keeps torch's [B, C, L] layout (time contiguous)
 * and ignores t2_set_precision: it always computes in exact fp32 on the matrix cores.  Weights are the folded ones (after
 * remove_weight_norm, hifigan_model.py:118-124) in torch layout, Conv1d [Cout][Cin][k], ConvTranspose1d [Cin][Cout][k].
 * Supported: resblock kind 1 or 2; 80 mel channels; channel counts that are multiples of 8, up to 512; Conv1d kernels
 * 3, 5, 7, 11 at dilations 1, 2, 3, 5, 6, 12; ConvTranspose1d with kernel = 2 * stride, stride even and <= 16 (covers
 * (16,8), (8,4), (4,2)).  Everything else is refused with the offending value in t2_last_error; nothing else is ever
 * computed in its place.  No atomics, a fixed order for every sum: results are bit-identical from run to run and for an
 * item alone or inside a batch.  Ordinary launches on `stream`. */
#define T2_HIFIGAN_MAX_UPS 6
#define T2_HIFIGAN_MAX_KERNELS 6
#define T2_HIFIGAN_MAX_DILATIONS 3
#define T2_VOCODER_TIME_TILE 128 /* time positions per workgroup of the conv kernels (tests probe its edges) */
typedef struct t2_hifigan_config {       /* the fields of the reference's config_v*.json that Generator reads */
    int resblock;                        /* 1 or 2 (the json's "1" / "2") */
    int n_mel;                           /* 80: conv_pre's input channels (hifigan_model.py:81) */
    int upsample_initial_channel;
    int num_upsamples, upsample_rates[T2_HIFIGAN_MAX_UPS], upsample_kernel_sizes[T2_HIFIGAN_MAX_UPS];
    int num_kernels, resblock_kernel_sizes[T2_HIFIGAN_MAX_KERNELS];
    int num_dilations;                   /* per resblock: 3 for kind 1, 2 for kind 2 */
    int resblock_dilation_sizes[T2_HIFIGAN_MAX_KERNELS][T2_HIFIGAN_MAX_DILATIONS];
} t2_hifigan_config;
typedef struct t2_hifigan_plan_info {
    long out_len;            /* samples per item: T * product of the rates */
    size_t workspace_bytes;  /* five activation buffers of the widest stage */
    size_t packed_bytes;     /* all layers' weights in fragment order, and the biases */
    int n_layers;            /* conv_pre, ups[i], every resblock conv, conv_post: the order of the state dict */
    int time_tile;           /* T2_VOCODER_TIME_TILE */
} t2_hifigan_plan_info;
/* Pure host call (no device): validates cfg, B >= 1 and T >= 1 and sizes the buffers. */
int t2_hifigan_plan(const t2_hifigan_config* cfg, int B, int T, t2_hifigan_plan_info* out);
/* weights_host / biases_host: HOST arrays of n_layers DEVICE pointers in layer order.  Writes `packed` (packed_bytes); done
 * once per set of weights, not per call. */
int t2_hifigan_pack(const t2_hifigan_config* cfg, const float* const* weights_host, const float* const* biases_host, int n_layers,
                    float* packed, void* stream);
typedef struct t2_hifigan_fwd_args {
    int B, T, n_mel;         /* n_mel: channels of the tensor given, checked against cfg */
    const float* packed;
    const float* mel;        /* [B, n_mel, T] */
    float* workspace;        /* workspace_bytes */
    float* audio;            /* [B, 1, out_len] */
    float* pre_tanh;         /* debug output, nullable: conv_post's output before the tanh, [B, 1, out_len] */
} t2_hifigan_fwd_args;
int t2_hifigan_forward(const t2_hifigan_config* cfg, const t2_hifigan_fwd_args* a, void* stream);
/* A padded batch of mels of different lengths.  frames [B] (device, int32): item b's frame count.  It is read by the kernels
 * only, never by the host, and clamped there to [0, T], so that no value of it moves a load or a store out of a row.  Item b
 * is computed as if mel[b, :, :frames[b]] were run alone through t2_hifigan_forward: at every layer its row ends at
 * frames[b] * (the rates so far), with the zeros of the "same" padding behind it, and the time tiles, the order of every
 * sum and so the bits are those of that run.  What the mel holds at or behind frames[b] is never loaded (NaN and Inf
 * included).  audio and pre_tanh are exact zeros from frames[b] * prod(rates) on; sample_lengths [B] (device, int32,
 * nullable) receives that count.  frames[b] = 0 is legal: an all-zero row of length 0.  Workgroups whose tile lies behind
 * their item's end return at once, so the cost follows sum(frames), not B * T. */
typedef struct t2_hifigan_ragged_args {
    int B, T, n_mel;
    const float* packed;
    const float* mel;            /* [B, n_mel, T] */
    float* workspace;            /* workspace_bytes of t2_hifigan_plan(cfg, B, T) */
    float* audio;                /* [B, 1, out_len] */
    float* pre_tanh;             /* nullable, as in t2_hifigan_fwd_args */
    const int32_t* frames;       /* [B] */
    int32_t* sample_lengths;     /* [B], nullable */
} t2_hifigan_ragged_args;
int t2_hifigan_forward_ragged(const t2_hifigan_config* cfg, const t2_hifigan_ragged_args* a, void* stream);
/* Single layers, for the tests only (the generator runs the same kernels).  w in torch layout; packed_ws receives the
 * packed weights first: t2_vocoder_packed_floats(Cin, Cout, k, u) floats, u = 0 for Conv1d.
 * conv1d (stride 1, padding (k*d - d)/2): y = ((accumulate ? y : 0) + conv(leaky_relu(x, slope)) + bias + residual) * scale,
 *   x, y, residual [B, C, L]; bias and residual nullable.
 * conv_transpose1d (stride u, padding (k - u)/2): y [B, Cout, L*u] = convT(leaky_relu(x, slope)) + bias. */
typedef struct t2_vocoder_conv_args {
    int B, Cin, Cout, L, k, d, u;
    const float* x; const float* w; const float* bias; const float* residual;
    float* y; float* packed_ws;
    float slope; int accumulate; float scale;
} t2_vocoder_conv_args;
size_t t2_vocoder_packed_floats(int Cin, int Cout, int k, int u);
int t2_vocoder_conv1d(const t2_vocoder_conv_args* a, void* stream);              /* a->u must be 0 */
int t2_vocoder_conv_transpose1d(const t2_vocoder_conv_args* a, void* stream);    /* a->d, residual, accumulate unused */
/* Either layer (conv.u = 0: Conv1d, conv.u > 0: ConvTranspose1d) with per-item input lengths [B] (device, int32, clamped to
 * [0, L] in the kernel), for the tests only.  Item b's rows are taken to end at lengths[b]: x, residual and (with accumulate)
 * y are not read at or behind it, and y is LEFT UNTOUCHED from lengths[b] (Conv1d) or lengths[b] * u (ConvTranspose1d) on.
 * Inside, the bits are those of the item alone at L = lengths[b]. */
typedef struct t2_vocoder_conv_ragged_args {
    t2_vocoder_conv_args conv;
    const int32_t* lengths;
} t2_vocoder_conv_ragged_args;
int t2_vocoder_conv_ragged(const t2_vocoder_conv_ragged_args* a, void* stream);

/* ---- HiFi-GAN generator, training ------------------------------------------------------------------
 * The backward of hifigan_infer/hifigan_model.py: Generator.forward (:100-116), ResBlock1.forward (:35-42) and
 * ResBlock2.forward (:63-68), which the reference leaves to torch's autograd, and a forward that keeps what it reads.  Same
 * layouts, limits and arithmetic as above: exact fp32 on the matrix cores whatever t2_set_precision says, no atomics, every
 * sum in a fixed order and partial sums added ascending in fp64, so the bits repeat from run to run.  Fixed-length batches
 * only.  The multi-period discriminator is the next section; the GAN losses are element-wise torch in hifigan_infer/hifigan_model.py.
 * MultiScaleDiscriminator is not built. */
#define T2_HIFIGAN_TRAIN_OPS 5 /* kinds of launch-list entry: conv, conv_post, conv_post backward, weight gradient, data gradient */
typedef struct t2_hifigan_train_plan_info {
    long out_len;                /* samples per item */
    size_t tape_bytes;           /* the pre-activation input of every conv: conv_pre's output; per stage X and XS; per block r_m, t_m */
    size_t workspace_bytes;      /* backward: five gradient buffers of the widest stage, partial planes, conv_post's fp64 partials */
    size_t packed_bytes;         /* as t2_hifigan_plan */
    size_t packed_bwd_bytes;     /* the data-gradient packs of every layer but conv_post */
    size_t grad_floats;          /* the gradient arena: per layer dw (torch layout) then db, at t2_hifigan_grad_offsets */
    size_t part_bytes;           /* the largest layer's partial planes (inside workspace_bytes) */
    int n_layers;
    int n_forward_launches, n_backward_launches;      /* kernels per call, the mel's gradient included */
    int launches[T2_HIFIGAN_TRAIN_OPS];               /* launch-list entries per kind, forward and backward together */
} t2_hifigan_train_plan_info;
/* Pure host call (no device): the tape, the scratch and the launch list from cfg, B and T alone. */
int t2_hifigan_train_plan(const t2_hifigan_config* cfg, int B, int T, t2_hifigan_train_plan_info* out);
/* Offsets in floats of every layer's dw and db in the gradient arena; pure host. */
int t2_hifigan_grad_offsets(const t2_hifigan_config* cfg, size_t* w_offsets, size_t* b_offsets, int n_layers);
/* weights_host: a HOST array of n_layers DEVICE pointers (folded weights, torch layout, layer order).  Writes packed_bwd. */
int t2_hifigan_pack_backward(const t2_hifigan_config* cfg, const float* const* weights_host, int n_layers, float* packed_bwd, void* stream);
typedef struct t2_hifigan_train_fwd_args {
    int B, T, n_mel;
    const float* packed;         /* t2_hifigan_pack */
    const float* mel;            /* [B, n_mel, T] */
    float* tape;                 /* tape_bytes */
    float* audio;                /* [B, 1, out_len]: the bits of t2_hifigan_forward */
} t2_hifigan_train_fwd_args;
int t2_hifigan_forward_train(const t2_hifigan_config* cfg, const t2_hifigan_train_fwd_args* a, void* stream);
typedef struct t2_hifigan_bwd_args {
    int B, T, n_mel;
    const float* packed; const float* packed_bwd;
    const float* mel; const float* tape; const float* audio;     /* as t2_hifigan_forward_train read and wrote them */
    const float* d_audio;        /* [B, 1, out_len]: the gradient on the audio */
    float* workspace;            /* workspace_bytes */
    float* grads;                /* grad_floats; every dw and db is written.  Nullable (then d_mel must be given): no weight gradient is launched */
    float* d_mel;                /* nullable: [B, n_mel, T], conv_pre's data gradient */
} t2_hifigan_bwd_args;
int t2_hifigan_backward(const t2_hifigan_config* cfg, const t2_hifigan_bwd_args* a, void* stream);
/* Single kernels, for the tests only (the backward runs the same ones).  L is the layer's INPUT length throughout.
 * Data gradient of conv(leaky_relu(x, slope)) (Conv1d.forward as ResBlock1.forward :37-41 calls it; ConvTranspose1d as
 * Generator.forward :103-104): dx = (accumulate ? dx : 0) + (residual + lrelu'(x) * W^T dy) * scale, lrelu'(0) = slope as torch
 * has it; x nullable (no activation in front: conv_pre), residual nullable; dx, x, residual [B, Cin, L]; dy [B, Cout, L] or
 * [B, Cout, L*u]; dx must not overlap dy or residual (refused, before anything is written).  packed_ws: t2_vocoder_dgrad_packed_floats(Cin, Cout, k, u) floats. */
typedef struct t2_vocoder_dgrad_args {
    int B, Cin, Cout, L, k, d, u;
    const float* dy; const float* w; const float* x; const float* residual;
    float* dx; float* packed_ws;
    float slope; int accumulate; float scale;
} t2_vocoder_dgrad_args;
size_t t2_vocoder_dgrad_packed_floats(int Cin, int Cout, int k, int u);
int t2_vocoder_conv1d_dgrad(const t2_vocoder_dgrad_args* a, void* stream);             /* a->u must be 0 */
int t2_vocoder_conv_transpose1d_dgrad(const t2_vocoder_dgrad_args* a, void* stream);   /* a->d unused */
/* Weight and bias gradient of the same layers (u = 0: Conv1d, u > 0: ConvTranspose1d): dw in torch's layout, db [Cout]
 * nullable, both written; part: t2_vocoder_wgrad_part_floats(...) floats of scratch for the partial planes. */
typedef struct t2_vocoder_wgrad_args {
    int B, Cin, Cout, L, k, d, u;
    const float* x; const float* dy;
    float* dw; float* db; float* part;
    float slope;
} t2_vocoder_wgrad_args;
size_t t2_vocoder_wgrad_part_floats(int B, int Cin, int Cout, int L, int k, int d, int u);
int t2_vocoder_wgrad(const t2_vocoder_wgrad_args* a, void* stream);
/* conv_post and the tanh backwards (Generator.forward :112-114): d_pre = d_audio * (1 - audio^2); dx [B, C, L] = lrelu'(x; 0.01) *
 * w^T d_pre * scale; dw [C, 7], db [1].  part: t2_vocoder_post_part_doubles(B, C, L) doubles, 8-byte aligned. */
typedef struct t2_vocoder_post_bwd_args {
    int B, C, L;
    const float* x; const float* w; const float* audio; const float* d_audio;
    float* dx; float* dw; float* db; double* part;
    float scale;
} t2_vocoder_post_bwd_args;
size_t t2_vocoder_post_part_doubles(int B, int C, int L);
int t2_vocoder_post_backward(const t2_vocoder_post_bwd_args* a, void* stream);

/* ---- HiFi-GAN multi-period discriminator, forward and backward -------------------------------------
 * Replaces hifigan_infer/hifigan_model.py: DiscriminatorP.forward (:141-160), as MultiPeriodDiscriminator.forward (:174-187)
 * calls it, and its backward, which the reference leaves to torch's autograd.  One call runs one period discriminator over B
 * items: real and generated audio go in together as one batch, so the weights are read once.  Layout as torch has it: audio
 * [B, 1, T], feature map i [B, C[i+1], H[i+1], period]; conv i = convs[i] (:132-138) for i < 5, conv 5 = conv_post (:139).  The
 * reflect padding (:146-149) is index arithmetic; T with period - T % period > T - 1 is refused, where torch raises.  Weights are
 * the folded ones in torch layout [Cout][Cin][k][1].  Exact fp32 on the matrix cores whatever t2_set_precision says, no atomics,
 * every sum in a fixed order, partial sums added ascending in fp64: the bits repeat from run to run, and an item's feature maps
 * are those of the item run alone.  Periods 2..11; the reference's kernel size 5, stride 3 and widths only. */
#define T2_HIFIGAN_MPD_LAYERS 6
typedef struct t2_hifigan_mpd_plan_info {
    int period, B, T, pad;                                               /* pad: samples reflected on the right */
    int H[T2_HIFIGAN_MPD_LAYERS + 1], C[T2_HIFIGAN_MPD_LAYERS + 1];      /* [0]: the padded audio as [1][H][period]; [i + 1]: feature map i */
    int tiles[T2_HIFIGAN_MPD_LAYERS];        /* 128-column tiles per item of conv i's GEMM over the H * period positions; 0: not a GEMM */
    int splits[T2_HIFIGAN_MPD_LAYERS];       /* runs (partial planes) of conv i's weight gradient */
    size_t fmap_floats[T2_HIFIGAN_MPD_LAYERS];
    size_t w_offsets[T2_HIFIGAN_MPD_LAYERS], b_offsets[T2_HIFIGAN_MPD_LAYERS];   /* dw (torch layout) and db of conv i in the gradient arena, in floats */
    size_t packed_bytes;         /* forward pack: every conv's weights (GEMM layers in fragment order) and biases */
    size_t packed_bwd_bytes;     /* data-gradient packs of convs 1..4: three polyphase packs per strided conv */
    size_t workspace_bytes;      /* backward: two buffers of the largest feature map and the partial planes */
    size_t part_bytes;           /* the largest weight gradient's partial planes (inside workspace_bytes) */
    size_t grad_floats;          /* the gradient arena */
    int n_forward_launches, n_backward_launches;      /* kernels per call with every gradient asked for */
} t2_hifigan_mpd_plan_info;
/* Pure host call (no device): shapes, tiles, scratch and launch counts from (period, B, T) alone. */
int t2_hifigan_mpd_plan(int period, int B, int T, t2_hifigan_mpd_plan_info* out);
/* weights_host / biases_host: HOST arrays of T2_HIFIGAN_MPD_LAYERS DEVICE pointers.  The packs do not depend on period, B or T. */
int t2_hifigan_mpd_pack(const float* const* weights_host, const float* const* biases_host, float* packed, void* stream);
int t2_hifigan_mpd_pack_backward(const float* const* weights_host, float* packed_bwd, void* stream);
typedef struct t2_hifigan_mpd_fwd_args {
    int period, B, T;
    const float* packed;
    const float* audio;                          /* [B, 1, T] */
    float* fmap[T2_HIFIGAN_MPD_LAYERS];          /* every one written: leaky_relu(conv i) for i < 5, conv_post's output (the score) at 5 */
} t2_hifigan_mpd_fwd_args;
int t2_hifigan_mpd_forward(const t2_hifigan_mpd_fwd_args* a, void* stream);
typedef struct t2_hifigan_mpd_bwd_args {
    int period, B, T;
    const float* packed; const float* packed_bwd;
    const float* audio;
    const float* fmap[T2_HIFIGAN_MPD_LAYERS];    /* as t2_hifigan_mpd_forward wrote them: the tape (a map's sign gives lrelu') */
    const float* g_fmap[T2_HIFIGAN_MPD_LAYERS];  /* the upstream gradient on each feature map; [0..4] nullable, [5] (the score's) required */
    float* workspace;                            /* workspace_bytes */
    float* grads;                                /* grad_floats, every dw and db written.  Nullable: no weight gradient is launched */
    float* d_audio;                              /* [B, 1, T].  Nullable: the audio's gradient is not launched */
} t2_hifigan_mpd_bwd_args;
int t2_hifigan_mpd_backward(const t2_hifigan_mpd_bwd_args* a, void* stream);

/* ---- STFT analysis / synthesis and vocoder bias removal ---------------------------------------------
 * Replaces the reference's stft.py: STFT.transform (:77-105), STFT.inverse (:107-136) and STFT.forward (:138-141), with
 * audio_processing.py: window_sumsquare (:7-56), and the element-wise middle of bias_remover.py:
 * hifiganBiasRemover.forward (:31-36).  torch's [B, C, frames] layout, time contiguous; always exact fp32 on the matrix
 * cores, whatever t2_set_precision says.  No atomics, a fixed order for every sum: bit-identical from run to run and for
 * an item alone or inside a batch.  Ordinary launches on `stream`.
 * Supported: even filter_length N up to 4096, hop_length dividing N with N / hop <= 64.  Everything else is refused with
 * the offending values in t2_last_error. */
#define T2_STFT_FRAME_TILE 32 /* frames (analysis) / hop-sized output blocks (synthesis) per workgroup (tests probe its edges) */
#define T2_STFT_POLAR 0
#define T2_STFT_DENOISE 1
typedef struct t2_stft_plan_info {
    int bins;                /* N/2 + 1 */
    int overlap;             /* N / hop */
    int frame_tile;          /* T2_STFT_FRAME_TILE */
    int bin_tile;            /* 16: bins per 32-row basis tile (real and imaginary rows interleaved) */
    long out_len;            /* samples per item the synthesis writes: hop * (nf - 1) */
    size_t fwd_floats;       /* packed forward basis */
    size_t inv_floats;       /* packed inverse basis */
    size_t wsq_floats;       /* squared window: N doubles */
    size_t packed_bytes;     /* all three, in that order */
} t2_stft_plan_info;
/* Pure host call (no device).  Fails, with the values in the message, for odd N, N % hop != 0, N > 4096, N / hop > 64
 * and nf < 1. */
int t2_stft_plan(int N, int hop, int nf, t2_stft_plan_info* out);
/* forward_basis, inverse_basis: the module's windowed buffers, [2*(N/2+1)][N] (stft.py:74-75).  window_sq: the squared
 * window, centre-padded to N, in fp64 as window_sumsquare forms it (audio_processing.py:48-50; fp64 because numpy adds
 * it to the fp32 envelope in fp64); NULL for STFT(window=None).  All device pointers.  Writes `packed` (packed_bytes);
 * done once per module, not per call. */
int t2_stft_pack(int N, int hop, const float* forward_basis, const float* inverse_basis, const double* window_sq, float* packed, void* stream);
/* x [B, n], n > N/2, reflect-padded by N/2 per side in the loader (stft.py:84-89) -> [B, N/2+1, 1 + n/hop] each:
 * re, im = the conv1d of stft.py:91-99; mag = sqrt(re^2 + im^2), phase = atan2(im, re) (stft.py:101-103).  Every output
 * is nullable; at least one is given.
 * Accuracy: each element is a sequential fp32 chain of N fused multiply-adds.  Against fp64 it stays within 1e-6 * S
 * (S = sum |x_k| |basis_k|) when the products mix signs; that is a statistical bound, not a worst case.  A chain of one-signed
 * products -- the bin of a strong stationary tone, the DC bin under an offset -- errs by about 0.6 * sqrt(N) * 2^-24 * S
 * (0.9e-6 * S seen at N = 1024) and can exceed it; the worst case is N * 2^-24 * S. */
typedef struct t2_stft_analysis_args {
    int B, N, hop; long n;
    const float* x; const float* packed;
    float* re; float* im; float* mag; float* phase;
} t2_stft_analysis_args;
int t2_stft_analysis(const t2_stft_analysis_args* a, void* stream);
/* a, b [B, N/2+1, nf] -> y [B, 1, hop*(nf-1)]: conv_transpose1d with the inverse basis as an overlap-add GEMM, the
 * envelope division, the N/hop scale and the trim of stft.py:111-134.
 * mode T2_STFT_POLAR: a = magnitude, b = phase, X = (a cos b, a sin b) (stft.py:108-109).
 * mode T2_STFT_DENOISE: a = re, b = im of t2_stft_analysis; X = g * (re, im), g = max(|z| - strength*bias[k], 0) / |z|
 *   (0 where |z| = 0): bias_remover.py:32-35 without the atan2 and the sincos.  bias [N/2+1].
 * windowed = 0: STFT(window=None), no envelope and no scale (stft.py:117); y is then the trimmed overlap-add sum itself.
 * Precondition, not checked: windowed != 0 needs tables packed with a window_sq.  Tables packed with window_sq == NULL hold
 * an all-zero envelope, so the division would be skipped and the N/hop scale still applied: call with windowed = 0 then. */
typedef struct t2_stft_synthesis_args {
    int B, N, hop, nf, mode, windowed;
    const float* a; const float* b; const float* bias; float strength;
    const float* packed;
    float* y;
} t2_stft_synthesis_args;
int t2_stft_synthesis(const t2_stft_synthesis_args* a, void* stream);
/* The two calls for a padded batch of rows of different lengths.  The counts are int32 device arrays [B], read by the kernels
 * only (nothing synchronises) and clamped there to the row, so that no value of them moves a load or a store out of bounds.
 * Every item's bits are those of its run alone; what the inputs hold behind an item's count is never loaded (NaN and Inf
 * included); workgroups whose tile lies behind their item's end only write zeros.
 * analysis: lengths[b] samples of row b count.  The reflection is the item's own, it has nf_b = 1 + lengths[b] / hop frames,
 *   the planes keep the layout [B, N/2+1, 1 + n/hop] with exact zeros at frames >= nf_b, and frame_lengths (nullable)
 *   receives nf_b.  A row of lengths[b] <= N/2 samples, for which the reflect padding is undefined, has no frames: all zero,
 *   count 0.
 * synthesis: frame_lengths[b] frames of item b count (clamped to [0, nf]).  y keeps the layout [B, 1, hop*(nf-1)] with exact
 *   zeros from out_len_b = hop * (frame_lengths[b] - 1) on; sample_lengths (nullable) receives out_len_b.  A count below 1
 *   gives an all-zero row of length 0.  Both modes and windowed = 0 as in t2_stft_synthesis. */
typedef struct t2_stft_analysis_ragged_args {
    int B, N, hop; long n;
    const float* x; const float* packed;
    float* re; float* im; float* mag; float* phase;
    const int32_t* lengths;      /* [B] */
    int32_t* frame_lengths;      /* [B], nullable */
} t2_stft_analysis_ragged_args;
int t2_stft_analysis_ragged(const t2_stft_analysis_ragged_args* a, void* stream);
typedef struct t2_stft_synthesis_ragged_args {
    int B, N, hop, nf, mode, windowed;
    const float* a; const float* b; const float* bias; float strength;
    const float* packed;
    float* y;
    const int32_t* frame_lengths; /* [B] */
    int32_t* sample_lengths;      /* [B], nullable */
} t2_stft_synthesis_ragged_args;
int t2_stft_synthesis_ragged(const t2_stft_synthesis_ragged_args* a, void* stream);

/* ---- Log-mel front end (ragged waveforms -> log-mel spectrograms) -----------------------------------
 * Replaces the reference's layers.py: TacotronSTFT.mel_spectrogram (:60-80) with stft.py: STFT.transform (:77-105) and
 * audio_processing.py: dynamic_range_compression (:78-84); utils.py: mel_spectrogram's pad, torch.stft(center=False),
 * sqrt(re^2 + im^2 + 1e-9), mel matmul and log (:73-79); and so the mel extraction of Audio/tools.py: get_mel (:30-42),
 * GTA.py:48, softdtw.py:78-79 and best_checkpoint.py:426-427.  One kernel:
 *   out[b][m][f] = log(max(clip_val, sum_bin mel[m][bin] * sqrt(re^2 + im^2 + mag_eps)) * C),
 *   (re, im)[bin][f] = sum_k forward_basis[.][k] * xpad_b[f*hop + k],
 * xpad_b = the first len_b samples of row b reflect-padded by `pad` per side (index arithmetic, no copy); an item has
 * nf_b = (len_b + 2*pad - N) / hop + 1 frames, or none when len_b <= pad or len_b + 2*pad < N.
 *   pad = N/2, mag_eps = 0:          the TacotronSTFT convention (layers.py:76-79, stft.py:84-103), 1 + len/hop frames;
 *   pad = (N - hop)/2, mag_eps = 1e-9: the utils.mel_spectrogram convention (utils.py:73-79).
 * Always exact fp32 on the matrix cores, whatever t2_set_precision says.  The magnitudes never reach memory.  The mel sum
 * is formed per pass of 64 bins from zero and the passes are added in ascending order, one rounded add each: the bits do not
 * depend on the launch shape (splits), and an item alone equals the item inside a batch.  No atomics.
 * Supported: even N up to 4096, 1 <= hop <= N, 0 <= pad <= N/2, n_mels up to 128, n + 2*pad >= N, n <= INT32_MAX/2.
 * Everything else is refused with the offending name and value in t2_last_error. */
typedef struct t2_melspec_plan_info {
    int bins;                     /* N/2 + 1 */
    int passes;                   /* ceil(bins / 64): bins whose magnitudes one pass holds on the chip */
    int frame_tile;               /* T2_STFT_FRAME_TILE frames per workgroup */
    int row_tiles;                /* ceil(n_mels / 32) */
    int splits;                   /* contiguous pass ranges the plan spreads over workgroups (1: one launch, no scratch) */
    long nf_max;                  /* frames of a full row: (n + 2*pad - N) / hop + 1 */
    long frame_tiles;
    size_t fwd_floats;            /* packed forward basis (t2_stft_pack's order) */
    size_t mel_floats;            /* packed mel table */
    size_t packed_bytes;          /* both, in that order */
    size_t scratch_floats;        /* what t2_melspec needs with force_splits = 0: 0 when splits == 1 */
    size_t split_scratch_floats;  /* what any split launch needs: passes * B * nf_max * n_mels */
} t2_melspec_plan_info;
/* Pure host call (no device).  n: samples per row of x. */
int t2_melspec_plan(int N, int hop, int pad, int n_mels, long n, int B, t2_melspec_plan_info* out);
/* forward_basis [2*(N/2+1)][N] (the STFT module's windowed buffer, stft.py:74), mel_basis [n_mels][N/2+1]
 * (layers.py:48-51).  Device pointers.  Writes `packed` (packed_bytes); once per module, not per call. */
int t2_melspec_pack(int N, int n_mels, const float* forward_basis, const float* mel_basis, float* packed, void* stream);
typedef struct t2_melspec_args {
    int B, N, hop, pad, n_mels;
    long n;                       /* samples per row of x */
    const float* x;               /* [B, n] */
    const int* lengths;           /* [B] int32 on the device, or NULL (every item has n samples); clamped to [0, n] */
    const float* packed;
    float* out;                   /* [B, n_mels, nf_max], or [B, nf_max, n_mels] with time_major; frames >= nf_b hold pad_value */
    float* scratch;               /* split launches only */
    size_t scratch_floats;
    int* frame_lengths;           /* [B] int32: nf_b, or NULL */
    float mag_eps, clip_val, C, pad_value;
    int time_major;
    int return_power;             /* tests: magnitude^2 instead of the magnitude and no clamp / log: out = sum_bin mel * (re^2 + im^2 + mag_eps) */
    int force_splits;             /* 0: the plan's splits; 1..passes: that many (tests: the bits do not depend on it) */
    float* mel_sum;               /* NULL, or [B, nf_max, n_mels]: receives the mel sum before clamp and log at frames < nf_b (what
                                   * t2_melspec_backward takes); out's bits do not depend on it */
} t2_melspec_args;
int t2_melspec(const t2_melspec_args* a, void* stream);

/* ---- Log-mel and STFT analysis: backward with respect to the samples ---------------------------------
 * Replaces what torch autograd derives from the reference's layers.py: TacotronSTFT.mel_spectrogram (:60-80), stft.py:
 * STFT.transform (:77-105) and utils.py: mel_spectrogram (:73-79): the gradient of a loss on the log-mel (or on re, im)
 * with respect to the waveform.  With g = dL/dout and s the mel sum the forward kept:
 *   ds[m][f]  = g[m][f] / s[m][f] where s >= clip_val (torch.clamp's mask), else 0;
 *   dmag[bin] = sum_m mel[m][bin] * ds[m];
 *   dz        = dmag * z / mag where mag > 0, else exactly 0 (torch's sqrt backward gives 0 * inf = NaN at digital silence
 *               with mag_eps = 0; a clipped frame contributes exactly 0 here whatever z is);
 *   dxpad[t]  = sum_{f*hop + k = t} sum_c forward_basis[c][k] * dz[c][f]   (the synthesis kernel's overlap-add GEMM);
 *   dx[i]     = dxpad[pad+i] + [1 <= i <= pad] dxpad[pad-i] + [L-1-pad <= i <= L-2] dxpad[pad+2(L-1)-i] for i < L = len_b, else 0.
 * z is recomputed from x with the forward's table (the forward's bits), never stored by the forward.  Exact fp32 on the
 * matrix cores, no atomics, every sum in a fixed order: bit-identical from run to run and for an item alone or in a batch.
 * g at frames >= nf_b and x behind len_b are never read.  Beyond the forward's limits the backward needs hop dividing N
 * and N / hop <= 64; refused by name in t2_last_error otherwise.  No gradient for the bases. */
typedef struct t2_melspec_grad_plan_info {
    int bins, passes, row_tiles, overlap;
    long nf_max;
    long grid_x, grid_y, grid_z;  /* the bins-side kernel: 32-frame tiles, passes of 64 bins, items */
    long fold_grid_x, fold_grid_y;/* the samples-side GEMM: tiles of 32 hop-blocks over nf_max - 1 + N/hop, column groups of hop */
    size_t melt_floats;           /* packed transposed mel table */
    size_t basis_floats;          /* forward basis in the synthesis kernel's order (t2_stft_plan's inv_floats) */
    size_t packed_bytes;          /* both, in that order: what t2_melspec_grad_pack writes */
    size_t dz_floats;             /* workspace: d_re and d_im, B * bins * nf_max each */
    size_t dxpad_floats;          /* workspace: B * (n + 2*pad) */
    size_t workspace_floats;      /* both, in that order */
} t2_melspec_grad_plan_info;
/* Pure host call (no device). */
int t2_melspec_grad_plan(int N, int hop, int pad, int n_mels, long n, int B, t2_melspec_grad_plan_info* out);
/* forward_basis, mel_basis as for t2_melspec_pack.  Writes `packed` (packed_bytes); once per module and mel basis. */
int t2_melspec_grad_pack(int N, int hop, int n_mels, const float* forward_basis, const float* mel_basis, float* packed, void* stream);
typedef struct t2_melspec_backward_args {
    int B, N, hop, pad, n_mels;
    long n;
    const float* x;               /* [B, n], the forward's input */
    const int* lengths;           /* as the forward's */
    const float* packed;          /* t2_melspec_pack's */
    const float* grad_packed;     /* t2_melspec_grad_pack's */
    const float* mel_sum;         /* [B, nf_max, n_mels] from the forward */
    const float* g;               /* dL/dout in out's layout: [B, n_mels, nf_max], or [B, nf_max, n_mels] with g_time_major */
    float* workspace; size_t workspace_floats;
    float* dx;                    /* [B, n]; zero from len_b on */
    float mag_eps, clip_val;
    int g_time_major;
} t2_melspec_backward_args;
int t2_melspec_backward(const t2_melspec_backward_args* a, void* stream);
/* The samples side alone: the backward of t2_stft_analysis(_ragged) for gradients d_re, d_im [B, N/2+1, 1 + n/hop] of its re
 * and im outputs (either may be NULL: zeros), pad = N/2 (stft.py:84-99 under autograd).  basis_table: the forward basis in
 * the synthesis kernel's order: the second part of t2_melspec_grad_pack's buffer, or the inverse part of t2_stft_pack's when
 * it was handed the forward basis as its inverse_basis.  lengths: NULL, or sample counts as t2_stft_analysis_ragged takes
 * them.  dxpad: B * (n + N) floats of scratch.  dx [B, n]. */
typedef struct t2_stft_analysis_backward_args {
    int B, N, hop; long n;
    const float* d_re; const float* d_im;
    const float* basis_table;
    const int32_t* lengths;
    float* dxpad;
    float* dx;
} t2_stft_analysis_backward_args;
int t2_stft_analysis_backward(const t2_stft_analysis_backward_args* a, void* stream);

/* ---- Silence trim (leading and trailing silence of ragged 16-bit audio) ------------------------------
 * Replaces the reference's pydub trim: remove_silence.py:7-36 (detect_leading_silence and the loop around it) and
 * best_checkpoint.py:319-333, 495-520 (the same function and loop, with the start_silence / limit_silence counters), for mono
 * 16-bit audio that stays on the device.  What pydub's AudioSegment computes there, restated; N frames at `rate` Hz,
 * r = rate / 1000.0 as a double:
 *   len(sound)      len_ms = round(1000 * (double(N) / rate)), half to even;
 *   sound[a:b]      (ms, both clamped to len_ms) = frames [int(a * r), int(b * r)), zero frames appended where the data ends
 *                   before int(b * r) (at most int(0.5 * r) + 1 of them, when len_ms was rounded up); empty if b <= a;
 *   .dBFS           of n frames: rms = (unsigned) sqrt(sum x^2 / n) (audioop.rms; 0 for n = 0); -inf when rms == 0, else
 *                   20 * log10(rms / 32768);
 *   detect_leading_silence(sound, thr, chunk): trim = 0; while sound[trim : trim + chunk].dBFS < thr: trim += chunk, and None
 *                   as soon as trim > len_ms; the trailing silence is the same on the reversed frames;
 *   the cut         sound[start : len_ms - end]: up to int(0.5 * r) + 1 frames longer than the input, those frames zero.
 * The kernels decide in integers: R = the smallest rms in 1..32768 whose level is not below thr (host, the same log10), and a
 * chunk is silent iff S < n * R^2 with S the exact 64-bit sum of squares.  start = chunk * (first loud k with
 * chunk * k < len_ms).  Two kernels and a memset of the scratch on `stream`, no synchronisation, no float atomics (one integer
 * atomicMin per scan workgroup): bit-identical from run to run and for an item alone or inside a batch.
 * Stated differences: an item whose leading silence is found but whose trailing silence is None (possible because the
 * forward and the reversed chunk grid differ; the reference's `duration - None` raises there and its `except` drops the file)
 * gets length 0, its start_ms and end_ms = -1; fp32 input is clamped to [-32768, 32767] (NaN -> 0) before it is truncated
 * toward zero, where numpy's out-of-range cast is undefined. */
typedef struct t2_silence_plan_info {
    int R;                        /* threshold as an rms: 0 = nothing is silent (thr = -inf), 32769 = everything is (thr > 0) */
    int len_ms;                   /* len() of a full row of n frames */
    int chunks;                   /* chunks of a full row: ceil(len_ms / chunk_ms) */
    int chunks_per_group;         /* chunks one scan workgroup owns */
    int scan_grid[3];             /* chunk groups, B, 2 directions; scan_grid[0] == 0: no scan launch */
    int cut_grid[2];              /* column tiles of 1024 outputs, B */
    int block;                    /* threads per workgroup of both kernels */
    long out_width;               /* n + int(0.5 * r) + 1: samples per output row */
    size_t scratch_bytes;         /* the first-loud-chunk words, a 128-byte line each: 2 * B * 128 */
} t2_silence_plan_info;
/* Pure host call (no device).  n: samples per row.  Refuses, naming the argument: sample_rate < 4000, chunk_ms < 1, a NaN
 * threshold_db, n < 0, n > INT32_MAX / 2 (32-bit frame indices), B outside 1..65535. */
int t2_silence_plan(int sample_rate, int chunk_ms, double threshold_db, long n, int B, t2_silence_plan_info* out);
typedef struct t2_silence_args {
    int B; long n;                /* rows, samples per row of x */
    int sample_rate, chunk_ms;
    double threshold_db;
    const void* x;                /* [B, n] int16, or fp32 in int16 units with x_float (best_checkpoint.py:216-224 before astype) */
    int x_float;
    const int32_t* lengths;       /* [B] on the device, or NULL (every item has n frames); clamped to [0, n] */
    void* out;                    /* [B, out_width] int16, or fp32 = int16 * scale with out_float; zero from new_lengths[b] on; not x */
    int out_float; float scale;
    int32_t* new_lengths;         /* [B]: frames kept, 0 for a dropped item */
    int32_t* start_ms;            /* [B]: leading silence in ms, -1 for None */
    int32_t* end_ms;              /* [B]: trailing silence in ms, -1 for None or a dropped item */
    void* scratch; size_t scratch_bytes;
    int leading_only;             /* detect_leading_silence alone: only start_ms is written; out, new_lengths, end_ms may be NULL */
} t2_silence_args;
int t2_silence_trim(const t2_silence_args* a, void* stream);

/* ---- WaveGlow inference (mel spectrogram -> waveform) ------------------------------------------------
 * Replaces the reference's glow.py: WaveGlow.infer (:251-293), WN.forward (:153-175) and
 * Invertible1x1Conv.forward(reverse=True) (:88-97), as inference.py:160-170 and best_checkpoint.py:179-189 call them and as
 * bias_remover.py:38-74 (waveglowBiasRemover) does.  torch's [B, C, L] layout, time contiguous; always exact fp32 on the
 * matrix cores, whatever t2_set_precision says.  No atomics, a fixed order for every sum: bit-identical from run to run
 * and for an item alone or inside a batch.  Ordinary launches on `stream`.  fp32 only; the other direction of the flow
 * (waveform -> latent and log-likelihood) follows below.
 * With G = n_group, L = T*256/G and nc = n_channels, per flow k = n_flows-1 .. 0 (a0 / a1 = the halves of `audio`):
 *   x = start(a0); per layer i: acts = tanh(.)*sigmoid(.) of in_layers[i](x) + cond_layer(spect)[2nc*i : 2nc*(i+1)], the
 *   conditioning folded into the same GEMM (no [B, 2*nc*n_layers, L] tensor exists); x += / out += res_skip_layers[i](acts);
 *   a1 = (a1 - b) / exp(s) with (b, s) = end(out); audio = W^-1 cat(a0, a1); early flows prepend sigma * z.
 * Weights are the folded ones (g * v / ||v||) in torch layout; W^-1 is computed by the caller, once, in fp32 (glow.py:91).
 * Supported: kernel_size 3; n_layers 1..8; n_channels a multiple of 8 from 8 to 512; n_group even, 2..8; n_early_size
 * even; n_mel_channels * n_group a multiple of 8; B <= 65535.  Everything else is refused with the offending value in
 * t2_last_error; nothing else is ever computed in its place. */
#define T2_WAVEGLOW_MAX_LAYERS 8
#define T2_WAVEGLOW_KERNELS 5 /* kernel kinds of kernel_ms_host: upsample, start, gated conv, res_skip, coupling */
typedef struct t2_waveglow_config {      /* the constructor arguments of glow.py:179-180 and WN_config */
    int n_mel_channels, n_flows, n_group, n_early_every, n_early_size;
    int n_layers, n_channels, kernel_size;
} t2_waveglow_config;
typedef struct t2_waveglow_plan_info {
    long L;                  /* columns of every activation: T * 256 / n_group */
    long out_len;            /* samples per item: L * n_group (= T * 256 where n_group divides 256) */
    int n_remaining_channels;/* channels of the first noise plane (glow.py:205) */
    int n_noise_planes;      /* 1 + the number of early flows: [B, n_remaining, L], then [B, n_early_size, L] each, k descending */
    int n_tensors;           /* what t2_waveglow_pack takes: 2 + n_flows * (7 + 4 * n_layers) */
    int time_tile;           /* T2_VOCODER_TIME_TILE */
    size_t workspace_bytes;  /* spect, x, out, acts and two audio buffers */
    size_t packed_bytes;
} t2_waveglow_plan_info;
/* Pure host call (no device): validates cfg, B >= 1 and T >= 1 and sizes the buffers. */
int t2_waveglow_plan(const t2_waveglow_config* cfg, int B, int T, t2_waveglow_plan_info* out);
/* tensors_host: HOST array of n_tensors DEVICE pointers: upsample.weight [n_mel][n_mel][1024], upsample.bias, then per flow
 * k ascending: start.weight [nc][n_half], start.bias, cond_layer.weight [2*nc*n_layers][n_mel*G], cond_layer.bias,
 * (in_layers[i].weight [2nc][nc][3], .bias) for every i, (res_skip_layers[i].weight [2nc or nc][nc], .bias) for every i,
 * end.weight [2*n_half][nc], end.bias, W_inverse [c][c].  Writes `packed` (packed_bytes); once per set of weights. */
int t2_waveglow_pack(const t2_waveglow_config* cfg, const float* const* tensors_host, int n_tensors, float* packed, void* stream);
typedef struct t2_waveglow_infer_args {
    int B, T, n_mel;         /* n_mel: channels of the tensor given, checked against cfg */
    const float* packed;
    const float* mel;        /* [B, n_mel, T] */
    const float* const* noise_host;   /* HOST array of n_noise DEVICE pointers, the planes in the order of the plan */
    int n_noise;
    float sigma;
    float* workspace;        /* workspace_bytes */
    float* audio;            /* [B, out_len] */
    float* spect;            /* debug output, nullable: the upsampled, regrouped mel [B, n_mel*G, L] (glow.py:252-258) */
    float* flow_audio;       /* debug output, nullable: `audio` after the last-executed flow (k = 0), [B, G, L] */
    double* kernel_ms_host;  /* debug output, nullable: T2_WAVEGLOW_KERNELS totals in ms, every launch bracketed by events */
} t2_waveglow_infer_args;
int t2_waveglow_infer(const t2_waveglow_config* cfg, const t2_waveglow_infer_args* a, void* stream);
/* Single kernels, for the tests only (t2_waveglow_infer runs the same ones).  Weights in torch layout; packed_ws receives
 * the packed weights first: t2_waveglow_packed_floats(kind, ...) floats with kind 0 = gated conv (rows = nc, k0 = nc,
 * k1 = conditioning channels), 1 = res_skip (rows = 2nc or nc, k0 = nc), 2 = upsample (rows = k0 = n_mel). */
size_t t2_waveglow_packed_floats(int kind, int rows, int k0, int k1);
/* y [B, nc, L] = tanh(u[:nc]) * sigmoid(u[nc:]), u = conv(x; w_in, dilation d, "same") + b_in + w_cond spect + b_cond
 * (glow.py:160-166 with glow.py:28-40).  raw != 0 skips the gate: y [B, 2*nc, L] = u.  d in 1, 2, 4 .. 128. */
typedef struct t2_waveglow_gated_args {
    int B, nc, n_cond, L, d, raw;
    const float* x;          /* [B, nc, L] */
    const float* spect;      /* [B, n_cond, L] */
    const float* w_in; const float* b_in;       /* [2nc][nc][3], [2nc] */
    const float* w_cond; const float* b_cond;   /* the layer's rows of cond_layer: [2nc][n_cond], [2nc] */
    float* packed_ws; float* y;
} t2_waveglow_gated_args;
int t2_waveglow_gated_conv(const t2_waveglow_gated_args* a, void* stream);
/* rs = w acts + bias.  last == 0 (w [2nc][nc]): x += rs[:nc], out += rs[nc:];  last != 0 (w [nc][nc]): out += rs
 * (glow.py:168-173).  first != 0: `out` is taken as zero and not read (glow.py:156). */
typedef struct t2_waveglow_res_skip_args {
    int B, nc, L, first, last;
    const float* acts; const float* w; const float* bias;
    float* packed_ws; float* x; float* out;     /* [B, nc, L] each; x unused when last */
} t2_waveglow_res_skip_args;
int t2_waveglow_res_skip(const t2_waveglow_res_skip_args* a, void* stream);
/* spect [B, n_mel*G, L], L = T*256/G: spect[b, m*G + g, l] = ConvTranspose1d(n_mel, n_mel, 1024, stride=256)(mel)[b, m, l*G + g]
 * (glow.py:252-258); the 768 trailing samples are never computed. */
typedef struct t2_waveglow_upsample_args {
    int B, n_mel, T, n_group;
    const float* mel; const float* w; const float* bias;    /* [B, n_mel, T], [n_mel][n_mel][1024], [n_mel] */
    float* packed_ws; float* spect;
} t2_waveglow_upsample_args;
int t2_waveglow_upsample(const t2_waveglow_upsample_args* a, void* stream);
/* One flow's tail (glow.py:276-289): (b, s) = end(out); a1 = (in_scale*a1 - b) / exp(s); y = W_inverse cat(in_scale*a0, a1);
 * audio_out [B, n_early + 2*n_half, L] = cat(sigma * z, y).  audio_interleaved (nullable) [B, L, 2*n_half] receives y in
 * the order of the waveform (glow.py:291); audio_out is nullable when it is given. */
typedef struct t2_waveglow_couple_args {
    int B, nc, n_half, L, n_early;
    float in_scale, sigma;
    const float* out;        /* [B, nc, L] */
    const float* w_end; const float* b_end;     /* [2*n_half][nc], [2*n_half] */
    const float* audio_in;   /* [B, 2*n_half, L] */
    const float* w_inverse;  /* [2*n_half][2*n_half] */
    const float* z;          /* [B, n_early, L], unused when n_early == 0 */
    float* audio_out; float* audio_interleaved;
} t2_waveglow_couple_args;
int t2_waveglow_couple(const t2_waveglow_couple_args* a, void* stream);

/* ---- WaveGlow analysis (waveform -> latent and log-likelihood) -----------------------------------------
 * Replaces the reference's glow.py: WaveGlow.forward (:207-249), Invertible1x1Conv.forward (:98-102) and WaveGlowLoss
 * (:48-59), as waveglow/train.py:125-127 calls them -- the values only, no gradient.  The WN of a flow is the same in both
 * directions, so the upsample, start, gated conv and res_skip kernels are the ones above; around them, per flow
 * k = 0 .. n_flows-1 on audio regrouped to [B, G, L], L = n_samples / G (a tail of n_samples % G samples is dropped):
 *   if k % n_early_every == 0 and k > 0: the first n_early_size channels leave for z;  audio = W_k audio;
 *   (b, s) = end(WN_k(a0, spect));  a1 = exp(s) * a1 + b;  log_s[k] = s.
 * z [B, G, L] = the early outputs, k ascending, then the last flow's audio.  n_samples may exceed T*256 by up to 768: the
 * trailing samples of the transposed conv are then computed too (glow.py:215-218).  Sums are formed without atomics in a
 * fixed order and in fp64 from the first add: z, log_s, every sum and nll_item are bit-identical from run to run and for
 * an item alone or inside a batch. */
#define T2_WAVEGLOW_FORWARD_KERNELS 7 /* kinds of kernel_ms_host: upsample, start, gated conv, res_skip, head, tail, sums */
typedef struct t2_waveglow_forward_info {
    long L;                  /* columns of every activation: n_samples / n_group */
    int n_log_s_rows;        /* sum over the flows of n_half_k: log_s[k] is [B, n_half_k, L] */
    int n_tensors;           /* what t2_waveglow_pack takes */
    long n_blocks;           /* column blocks of 256 per item: one partial sum per (flow, item, block) and kind */
    size_t n_partials;       /* 2 * n_flows * B * n_blocks fp64 slots inside the workspace */
    size_t workspace_bytes;  /* spect, x, out, acts, two audio buffers, the partial sums, the per-item results */
    size_t packed_bytes;
} t2_waveglow_forward_info;
/* Pure host call (no device): validates cfg, B >= 1, T >= 1 and n_group <= n_samples <= (T-1)*256 + 1024 (glow.py:216). */
int t2_waveglow_forward_plan(const t2_waveglow_config* cfg, int B, int T, long n_samples, t2_waveglow_forward_info* out);
/* logdet [n_flows] = log |det W_k| of the matrices inside `packed` (packed with W_k where inference has W_k^-1): LU with
 * partial pivoting in fp64, rounded to fp32; NaN for a negative determinant, as torch.logdet.  Once per set of weights. */
int t2_waveglow_logdet(const t2_waveglow_config* cfg, const float* packed, float* logdet, void* stream);
typedef struct t2_waveglow_forward_args {
    int B, T, n_mel;         /* n_mel: channels of the mel given, checked against cfg */
    long n_samples;          /* N: samples per item of `audio` */
    const float* packed;     /* t2_waveglow_pack with W_k in the place of W_k^-1 */
    const float* logdet_w;   /* [n_flows], from t2_waveglow_logdet on the same buffer; nullable when neither logdet nor a sum is asked for */
    const float* mel;        /* [B, n_mel, T] */
    const float* audio;      /* [B, N] */
    float* workspace;        /* workspace_bytes */
    float* z;                /* [B, G, L]; nullable when a sum is asked for */
    float* const* log_s_host;/* nullable: HOST array of n_flows DEVICE pointers, log_s[k] [B, n_half_k, L] */
    float* logdet;           /* nullable: [n_flows], B * L * logdet_w[k] (glow.py:100) */
    float sigma;             /* of WaveGlowLoss; read only when a sum is asked for */
    double* sums;            /* nullable: [B][n_flows + 1], per item the sum of log_s[k] for every k, then the sum of z^2 */
    float* nll_item;         /* nullable: [B], (sum z^2 / (2 sigma^2) - sum log_s - L * sum logdet_w) / (G * L) */
    float* loss;             /* nullable: [1], the mean of the above over the items = WaveGlowLoss(sigma) */
    double* kernel_ms_host;  /* debug output, nullable: T2_WAVEGLOW_FORWARD_KERNELS totals in ms */
} t2_waveglow_forward_args;
int t2_waveglow_forward(const t2_waveglow_config* cfg, const t2_waveglow_forward_args* a, void* stream);
/* Single kernels, for the tests only (t2_waveglow_forward runs the same ones).
 * out[m] = log |det w[m]| of n matrices [c][c], c <= 8. */
int t2_waveglow_logdet_matrices(const float* w, int c, int n, float* out, void* stream);
/* audio_out [B, G, L] = w x regrouped audio: audio_out[b, r, l] = sum_g w[r][g] * audio[b, l*G + g] (glow.py:223, :233 at k = 0). */
typedef struct t2_waveglow_head_args {
    int B, n_group; long n_samples;
    const float* audio;      /* [B, n_samples] */
    const float* w;          /* [G][G] */
    float* audio_out;        /* [B, G, n_samples / G] */
} t2_waveglow_head_args;
int t2_waveglow_head(const t2_waveglow_head_args* a, void* stream);
/* One flow's tail (glow.py:240-246, then :229-233 of the next flow): (b, s) = end(out); v = cat(a0, exp(s) * a1 + b);
 * z[:, z_offset : z_offset + n_peel] = v[:n_peel]; audio_out [B, 2*n_half - n_peel, L] = w_next v[n_peel:].  On the last
 * flow n_peel = 2*n_half and w_next, audio_out are unused.  part_s, part_z (nullable, together) [B][ceil(L/256)]: the sums
 * of s and of the z^2 written, per item and block of 256 columns. */
typedef struct t2_waveglow_tail_args {
    int B, nc, n_half, L, n_peel, n_group, z_offset;
    const float* out;        /* [B, nc, L] */
    const float* w_end; const float* b_end;     /* [2*n_half][nc], [2*n_half] */
    const float* audio_in;   /* [B, 2*n_half, L] */
    const float* w_next;     /* [2*n_half - n_peel][2*n_half - n_peel] */
    float* audio_out; float* z; float* log_s;   /* z [B, n_group, L]; log_s (nullable) [B, n_half, L] */
    double* part_s; double* part_z;
} t2_waveglow_tail_args;
int t2_waveglow_tail(const t2_waveglow_tail_args* a, void* stream);

/* ---- WaveGlow training: the forward that keeps what the backward reads, and the backward ----------------
 * What waveglow/train.py:125-137 does on every batch.  t2_waveglow_train_forward is t2_waveglow_forward (the same launches,
 * the same bits for the same `packed`) that leaves in `saved`: spect once; per flow the mixed audio_in [B, c_k, L] and out
 * [B, nc, L]; per flow and layer x_i, tanh(u_a), sigmoid(u_b), [B, nc, L] each (acts = t * g is recomputed):
 *   saved floats = per * (n_mel*G + sum_k (c_k + nc * (1 + 3 * n_layers))),  per = B * L rounded up to a multiple of 4.
 * t2_waveglow_backward turns upstream gradients on z and on every log_s[k] (each nullable = zero) into the gradient of
 * every folded tensor, in t2_waveglow_pack's tensor order and torch layout, densely packed into `grad` (grad_floats =
 * the parameter count of the folded model; t2_waveglow_grad_offsets gives each tensor's offset).  Gradients with respect
 * to the mel and the audio are not formed.  Exact fp32 on the matrix cores, every sum in a fixed order that depends on
 * the shape alone, no atomics: `grad` is bit-identical from run to run. */
#define T2_WAVEGLOW_BACKWARD_KERNELS 8 /* kinds of kernel_ms_host: tail backward (+ its sums, the head), gate backward, conv backward, conditioning backward, weight gradient, its reduce, start backward, upsample backward */
typedef struct t2_waveglow_backward_info {
    long L;
    int n_tensors;
    size_t saved_bytes;      /* what t2_waveglow_train_forward writes (formula above) */
    size_t workspace_bytes;  /* of t2_waveglow_backward */
    size_t grad_floats;
    size_t packed_bwd_bytes; /* of t2_waveglow_pack_backward */
    size_t n_slots;          /* fp64 partial-sum slots of the tail backward: B * ceil(L / 256) * 4 */
} t2_waveglow_backward_info;
/* Pure host call: validates as t2_waveglow_forward_plan does. */
int t2_waveglow_backward_plan(const t2_waveglow_config* cfg, int B, int T, long n_samples, t2_waveglow_backward_info* out);
int t2_waveglow_grad_offsets(const t2_waveglow_config* cfg, size_t* offsets_host, int n_tensors);
/* The transposed operands of the data gradients, packed once per step from the tensors t2_waveglow_pack takes (W_k itself):
 * per flow and layer W_in with taps flipped and in/out swapped [nc] x [3 * 2nc], W_cond,i^T [n_mel*G] x [2nc], W_rs^T [nc] x [2nc | nc]. */
int t2_waveglow_pack_backward(const t2_waveglow_config* cfg, const float* const* tensors_host, int n_tensors, float* packed_bwd, void* stream);
typedef struct t2_waveglow_train_forward_args {
    t2_waveglow_forward_args fwd;
    float* saved;            /* saved_bytes of t2_waveglow_backward_plan */
} t2_waveglow_train_forward_args;
int t2_waveglow_train_forward(const t2_waveglow_config* cfg, const t2_waveglow_train_forward_args* a, void* stream);
typedef struct t2_waveglow_backward_args {
    int B, T, n_mel;
    long n_samples;
    const float* packed;     /* as given to t2_waveglow_train_forward */
    const float* packed_bwd;
    const float* saved;
    const float* mel;        /* [B, n_mel, T] */
    const float* audio;      /* [B, N] */
    const float* dz;         /* nullable: [B, G, L] */
    const float* const* dlog_s_host; /* nullable: HOST array of n_flows DEVICE pointers [B, n_half_k, L], each nullable */
    float* workspace;
    float* grad;             /* grad_floats */
    double* kernel_ms_host;  /* debug output, nullable: T2_WAVEGLOW_BACKWARD_KERNELS totals in ms */
} t2_waveglow_backward_args;
int t2_waveglow_backward(const t2_waveglow_config* cfg, const t2_waveglow_backward_args* a, void* stream);
/* Single kernels, for the tests only (t2_waveglow_backward runs the same ones).
 * Weight gradient: dw_x[m][c][j] = sum_{b,l} a[b,m,l] * x[b,c,l + (j - taps/2) d] (columns outside the row contribute nothing),
 * dw_spect[m][c] = sum a * spect (n_cond = 0: none), db[m] = sum a.  workspace: t2_waveglow_weight_grad_ws_floats floats. */
typedef struct t2_waveglow_weight_grad_args {
    int B, M, nc, n_cond, L, taps, d;   /* taps 3 with d >= 1, or taps 1 with d = 0 */
    int a_rows, x_rows;      /* rows per item of the buffers a and x lie in (their first M and nc rows are read); 0: M and nc */
    const float* a;          /* [B, a_rows, L] */
    const float* x;          /* [B, x_rows, L] */
    const float* spect;      /* [B, n_cond, L] */
    float* dw_x; float* dw_spect; float* db; float* workspace;
    float* db2;              /* nullable: a second destination of db, as cond_layer.bias's slice is */
} t2_waveglow_weight_grad_args;
size_t t2_waveglow_weight_grad_ws_floats(int M, int nc, int n_cond, int taps, int B, int L);
int t2_waveglow_weight_grad(const t2_waveglow_weight_grad_args* a, void* stream);
/* d_acts = w_rs^T [dx; d_out] (last: w_rs [nc][nc], d_out alone); du [B, 2nc, L] = [d_acts g (1 - t^2); d_acts t g (1 - g)],
 * acts [B, nc, L] = t g.  packed_ws: 2 * t2_waveglow_packed_floats(1, nc, nc, 0) floats. */
typedef struct t2_waveglow_gate_backward_args {
    int B, nc, L, last;
    const float* dx; const float* d_out; const float* w_rs; const float* t; const float* g;
    float* packed_ws; float* du; float* acts;
} t2_waveglow_gate_backward_args;
int t2_waveglow_gate_backward(const t2_waveglow_gate_backward_args* a, void* stream);
/* dx [B, nc, L] (+)= conv^T(du) through w_in [2nc][nc][3] at dilation d, d_spect [B, n_cond, L] (+)= w_cond^T du with w_cond
 * [2nc][n_cond]; first_*: store, else accumulate.  packed_ws: t2_waveglow_conv_backward_packed_floats floats. */
typedef struct t2_waveglow_conv_backward_args {
    int B, nc, n_cond, L, d, first_dx, first_spect;
    const float* du; const float* w_in; const float* w_cond;
    float* packed_ws; float* dx; float* d_spect;
} t2_waveglow_conv_backward_args;
size_t t2_waveglow_conv_backward_packed_floats(int nc, int n_cond);
int t2_waveglow_conv_backward(const t2_waveglow_conv_backward_args* a, void* stream);
/* One flow's tail backwards (see t2_waveglow_tail): d_next [B, C - n_peel, L] is the gradient on audio_out, dz / dlog_s the
 * upstream ones (nullable).  d_out [B, nc, L] = w_end^T [db; ds]; d_in [B, C, L] = (dV[:n_half], db exp(s)); dw_end [C][nc],
 * db_end [C], dw_next [C - n_peel]^2 from fp64 partials in `part` (B * ceil(L/256) * 4 * (C*nc + C + (C - n_peel)^2) doubles). */
typedef struct t2_waveglow_tail_backward_args {
    int B, nc, n_half, L, n_peel, n_group, z_offset;
    const float* out; const float* w_end; const float* b_end; const float* audio_in; const float* w_next; const float* d_next;
    const float* dz; const float* dlog_s;
    float* d_out; float* d_in; double* part; float* dw_end; float* db_end; float* dw_next;
} t2_waveglow_tail_backward_args;
int t2_waveglow_tail_backward(const t2_waveglow_tail_backward_args* a, void* stream);
/* Start backward: d_in[b, h, l] += sum_c w_start[c][h] * dx[b, c, l] for h < n_half (rows n_half.. of d_in [B, c, L] stay), and
 * dw_start [nc][n_half] = sum dx * audio_in[:, :n_half]^T, db_start [nc] = sum dx through the weight-gradient kernel (workspace:
 * t2_waveglow_weight_grad_ws_floats(nc, n_half, 0, 1, B, L) floats). */
typedef struct t2_waveglow_start_backward_args {
    int B, nc, c, n_half, L;
    const float* dx;         /* [B, nc, L] */
    const float* w_start;    /* [nc][n_half] */
    const float* audio_in;   /* [B, c, L] */
    float* d_in;             /* [B, c, L] */
    float* dw_start; float* db_start; float* workspace;
} t2_waveglow_start_backward_args;
int t2_waveglow_start_backward(const t2_waveglow_start_backward_args* a, void* stream);
/* Head backward: dw [G][G] = sum_{b,l} d_in[b, r, l] * audio[b, l*G + g], from fp64 partials in `part`
 * (B * ceil(L/256) * 4 * G*G doubles, L = n_samples / G). */
typedef struct t2_waveglow_head_backward_args {
    int B, n_group; long n_samples;
    const float* d_in;       /* [B, G, L] */
    const float* audio;      /* [B, n_samples] */
    double* part; float* dw;
} t2_waveglow_head_backward_args;
int t2_waveglow_head_backward(const t2_waveglow_head_backward_args* a, void* stream);
/* dw [n_mel][n_mel][1024], db [n_mel] of the transposed conv from d_spect [B, n_mel*G, n_samples / G]. */
typedef struct t2_waveglow_upsample_backward_args {
    int B, n_mel, T, n_group; long n_samples;
    const float* mel; const float* d_spect; float* dw; float* db;
} t2_waveglow_upsample_backward_args;
int t2_waveglow_upsample_backward(const t2_waveglow_upsample_backward_args* a, void* stream);

/* Gradient-norm clipping + Adam over a list of fp32 tensors — replaces torch.nn.utils.clip_grad_norm_ +
 * torch.optim.Adam.step of the training loop (train.py:322-330; Adam with weight decay added to the gradient).
 * `table` is a DEVICE array of n_tensors rows; row i covers chunks [first_chunk, first_chunk + t2_adam_chunks(numel))
 * and the rows are sorted by first_chunk (consecutive).  partial: n_chunks floats of scratch; norm_out: 2 floats
 * (total gradient norm, clip coefficient applied).  max_norm == 0 disables clipping.  step counts from 1.
 * Gradients are read, not modified (the coefficient is applied on the fly).
 * Parameters whose step counts differ (torch.optim.Adam corrects the bias per parameter): t2_adam_norm over the whole
 * table first, then one t2_adam_step per run of rows with equal step, with max_norm < 0 (= take the coefficient
 * t2_adam_norm left in norm_out[1]), `table` pointing at the run's first row and n_chunks = the run's chunk count. */
typedef struct t2_adam_tensor { float* p; const float* g; float* m; float* v; long numel; int first_chunk; int pad_; } t2_adam_tensor;
int t2_adam_chunks(long numel);
int t2_adam_step(const t2_adam_tensor* table, int n_tensors, int n_chunks, float* partial, float* norm_out, float max_norm,
                 float lr, float beta1, float beta2, float eps, float weight_decay, int step, void* stream);
int t2_adam_norm(const t2_adam_tensor* table, int n_tensors, int n_chunks, float* partial, float* norm_out, float max_norm, void* stream);
/* norm_out: FOUR floats — [0] total gradient norm, [1] clip coefficient (NaN when the norm is NaN, as clip_grad_norm_
 * makes it: every stepped parameter then turns NaN; 0 when the norm is infinite), [2] 1.0 when the update was skipped because the
 * device's sticky status word (t2_chain_status) was set, [3] reserved. */

/* In-situ kernel timing for bench.py's roofline figures: after t2_prof_enable(n) the decoder
 * drivers bracket each per-step kernel launch with HIP events on the launch stream (up to n
 * launches); t2_prof_collect synchronises on the last event and returns total milliseconds and
 * launch counts per kernel kind (host arrays of >= 8 entries):
 * 0 att-LSTM fwd, 1 attention fwd, 2 dec-LSTM fwd, 3 attention bwd, 4 att-LSTM bwd pointwise,
 * 5 att-LSTM bwd GEMM, 6 dec-LSTM bwd pointwise, 7 dec-LSTM bwd GEMM. */
int t2_prof_enable(int max_launches);
int t2_prof_collect(int n_kinds, double* total_ms_host, int* launches_host);

/* Unit-testable pieces. */
int t2_gemm(const float* A, const float* B, float* C, int M, int N, int K,
            long sam, long sak, long sbn, long sbk, long ldc,
            const float* bias, int act, float alpha, float beta,
            float* ws, size_t ws_bytes, int splitk, void* stream);
int t2_rng_keep_mask(uint64_t seed, uint32_t site, uint32_t n, float p, uint8_t* out, void* stream);
int t2_rng_normal(uint64_t seed, uint32_t site, uint32_t n, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* T2AMD_H */
