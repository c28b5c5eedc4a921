// BERT sentence encoder, inference only (include/t2amd.h "BERT sentence encoder"): what stands in front of the model,
// the [CLS] vector of data_utils.py:28-46.  Exact fp32 throughout, whatever t2_set_precision says; ordinary launches only.
//
// A ragged batch is packed: token rows [total, H] addressed through cu_seqlens [B+1].  The linear layers are gemm()
// products (fp32_only, per-column bias, GELU in the epilogue, beta = 1 for the residual add into the stream in place);
// this file adds the four kernels between them and the driver.
//
//   embed + LayerNorm / row LayerNorm: one wave per row, the row in registers (H / 64 <= 16 values per lane), mean first,
//   then the variance of the centred values (eps is 1e-12: E[x^2] - mean^2 would be noise), sums by a fixed butterfly.
//
//   attention: a workgroup of 4 waves owns (sentence, head, 32 query rows) and keeps the tile's whole score rows in LDS,
//   32 x (L32 + 1) floats with L32 = the length rounded up to 32: 64.1 KB at 512 tokens, so two workgroups share a CU's
//   160 KB.  Three phases, a barrier between them:
//     1. scores: wave w takes key tiles w, w + 4, ...; S = Q K^T on v_mfma_f32_32x32x2_f32 with both operands straight
//        from global memory.  The reduction index may be permuted as long as both operands agree, so lane (r, hk) holds
//        elements hk * 32 .. hk * 32 + 31 of row r of Q and of K: eight 16-byte loads of 128 contiguous bytes each, no
//        staging.  Step kk of the chain adds d = kk and d = 32 + kk.  Scores are scaled by 1/8 (exact) and land in LDS
//        with the lanes on adjacent keys.
//     2. softmax: wave w owns rows 8w .. 8w + 7; max, exp(s - max) written back unnormalised, the sum's reciprocal kept
//        per row; the columns between the length and L32 are zeroed so that phase 3 needs no mask.
//     3. context: wave w takes output columns (w & 1) * 32 .. + 31 and the key tiles of parity w >> 1; P from LDS (lane
//        (r, hk) holds keys hk * 16 .. + 15 of the tile), V from global with the lanes on adjacent columns.  The two key
//        halves are added through LDS in a fixed order, scaled by the row's reciprocal and stored.
//   Rows and keys past the sentence are never read (zeros enter the chains instead).  Nothing depends on the sentence's
//   place in the batch, and there are no atomics: a sentence's bits are the same in any batch order.
//   nq_first_only: the same kernel with one valid query row per sentence, read from a compact [B, .] buffer and written
//   to one: the last layer's CLS-only tail.
#include "../../include/t2amd.h"
#include "kernels.h"

namespace t2 {
namespace {

constexpr int kBertThreads = 256;
constexpr int kBertRowsPerWg = kBertThreads / kWave;      // LayerNorm: a wave per row
constexpr int kBertMaxPerLane = 16;                       // H <= 1024
constexpr int kBertQT = 32;                               // query rows per workgroup
constexpr int kBertHeadDim = 64;
constexpr int kBertMaxLen = 512;

// ------------------------------------------------------------------------------------------------------------------
// LayerNorm over a row held in registers
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void bert_ln_row(float (&v)[kBertMaxPerLane], int n, int H, float eps, const float* __restrict__ w,
                                            const float* __restrict__ b, float* __restrict__ out) {
    const int lane = threadIdx.x & (kWave - 1);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kBertMaxPerLane; ++i) if (i < n) s += v[i];
    const float mean = wave_sum(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < kBertMaxPerLane; ++i) if (i < n) { v[i] -= mean; q += v[i] * v[i]; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)H + eps);
#pragma unroll
    for (int i = 0; i < kBertMaxPerLane; ++i) if (i < n) { const int c = i * kWave + lane; out[c] = v[i] * rstd * w[c] + b[c]; }
}

__global__ void __launch_bounds__(kBertThreads) bert_embed_ln_kernel(const t2_bert_embed_ln_args a) {
    const int lane = threadIdx.x & (kWave - 1), b = blockIdx.y;
    const int p = blockIdx.x * kBertRowsPerWg + threadIdx.x / kWave;
    const int row0 = a.cu_seqlens[b], len = a.cu_seqlens[b + 1] - row0;
    if (p >= len || p >= a.max_len || row0 < 0 || row0 + p >= a.total_tokens) return;
    const long row = row0 + p;
    const float* wr = a.word + (long)a.ids[row] * a.H;
    const float* pr = a.pos + (long)p * a.H;
    const int n = a.H / kWave;
    float v[kBertMaxPerLane];
#pragma unroll
    for (int i = 0; i < kBertMaxPerLane; ++i) if (i < n) { const int c = i * kWave + lane; v[i] = (wr[c] + a.type[c]) + pr[c]; }
    bert_ln_row(v, n, a.H, a.eps, a.ln_w, a.ln_b, a.out + row * a.H);
}

__global__ void __launch_bounds__(kBertThreads) bert_layernorm_kernel(const t2_bert_layernorm_args a) {
    const int lane = threadIdx.x & (kWave - 1);
    const long row = (long)blockIdx.x * kBertRowsPerWg + threadIdx.x / kWave;
    if (row >= a.rows) return;
    const float* x = a.x + row * a.H;
    const int n = a.H / kWave;
    float v[kBertMaxPerLane];
#pragma unroll
    for (int i = 0; i < kBertMaxPerLane; ++i) if (i < n) v[i] = x[i * kWave + lane];
    bert_ln_row(v, n, a.H, a.eps, a.ln_w, a.ln_b, a.out + row * a.H);
}

// out[b] = x[cu_seqlens[b]]: the [CLS] rows of the residual stream
__global__ void __launch_bounds__(kBertThreads) bert_gather_cls_kernel(const float* __restrict__ x, const int* __restrict__ cu, int total, int H,
                                                                      float* __restrict__ out) {
    const int b = blockIdx.x, row = cu[b];
    if (row < 0 || row >= total) return;
    for (int c = threadIdx.x; c < H; c += kBertThreads) out[(long)b * H + c] = x[(long)row * H + c];
}

// ------------------------------------------------------------------------------------------------------------------
// ragged self-attention
// ------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int bert_round32(int n) { return (n + 31) & ~31; }
// LDS of a workgroup in floats: 32 row reciprocals, then the score rows (at least the 2 x 32 x 32 floats of the phase-3 hand-over)
inline size_t bert_attn_lds_floats(int max_len) {
    const size_t scores = (size_t)kBertQT * (bert_round32(max_len) + 1);
    return 32 + (scores > 2048 ? scores : 2048);
}

// 32 floats of a row, hk * 32 .. + 31 of the head's 64, or zeros
__device__ __forceinline__ void bert_load32(float (&r)[32], const float* p, bool valid) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
        if (valid) t = *reinterpret_cast<const f32x4*>(p + 4 * i);
        r[4 * i] = t.x; r[4 * i + 1] = t.y; r[4 * i + 2] = t.z; r[4 * i + 3] = t.w;
    }
}

__global__ void __launch_bounds__(kBertThreads) bert_attention_kernel(const t2_bert_attention_args a) {
    extern __shared__ float bert_smem[];
    float* inv = bert_smem;
    float* S = bert_smem + 32;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * kBertQT;
    const int row0 = a.cu_seqlens[b];
    const int len = a.cu_seqlens[b + 1] - row0;
    // (uniform over the workgroup, in front of every barrier) a sentence the arguments do not cover is left alone
    if (len < 1 || len > a.max_len || row0 < 0 || row0 + len > a.total_tokens) return;
    const int nq = a.nq_first_only ? 1 : len;
    if (q0 >= nq) return;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, r = lane & 31, hk = lane >> 5;
    const int nkt = (len + 31) >> 5, SP = nkt * 32 + 1;
    const long hoff = (long)h * kBertHeadDim;

    // phase 1: S = Q K^T / 8
    {
        float qf[32], kf[32];
        const bool qvalid = q0 + r < nq;
        const long qrow = a.nq_first_only ? b : row0 + q0 + r;
        bert_load32(qf, a.q + qrow * a.ldq + hoff + hk * 32, qvalid);
        for (int kt = wave; kt < nkt; kt += kBertThreads / kWave) {
            const int key = kt * 32 + r;
            bert_load32(kf, a.k + (long)(row0 + key) * a.ldk + hoff + hk * 32, key < len);
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
            for (int kk = 0; kk < 32; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[kk], kf[kk], acc, 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 16; ++e) S[((e & 3) + 8 * (e >> 2) + 4 * hk) * SP + kt * 32 + r] = acc[e] * 0.125f;
        }
    }
    __syncthreads();

    // phase 2: unnormalised softmax rows, zeros behind the length
    for (int i = 0; i < kBertQT / (kBertThreads / kWave); ++i) {
        const int qi = wave * (kBertQT / (kBertThreads / kWave)) + i;
        float* row = S + qi * SP;
        float m = -INFINITY;
        for (int k = lane; k < len; k += kWave) m = fmaxf(m, row[k]);
        m = wave_max(m);
        float sum = 0.f;
        for (int k = lane; k < nkt * 32; k += kWave) {
            const float p = k < len ? expf(row[k] - m) : 0.f;
            row[k] = p;
            sum += p;
        }
        sum = wave_sum(sum);
        if (lane == 0) inv[qi] = 1.0f / sum;
    }
    __syncthreads();

    // phase 3: O = P V
    const int dh = wave & 1, kh = wave >> 1;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    for (int kt = kh; kt < nkt; kt += 2) {
        const int key0 = kt * 32 + hk * 16;
        const float* vp = a.v + (long)(row0 + key0) * a.ldv + hoff + dh * 32 + r;
        float vf[16], pf[16];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) vf[kk] = key0 + kk < len ? vp[(long)kk * a.ldv] : 0.f;
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) pf[kk] = S[r * SP + key0 + kk];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pf[kk], vf[kk], acc, 0, 0, 0);
    }
    __syncthreads();                                   // every wave is done with the scores: their space takes the hand-over
    if (kh == 1) {
#pragma unroll
        for (int e = 0; e < 16; ++e) S[dh * 1024 + e * kWave + lane] = acc[e];
    }
    __syncthreads();
    if (kh == 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int qi = (e & 3) + 8 * (e >> 2) + 4 * hk;
            if (q0 + qi >= nq) continue;
            const float o = (acc[e] + S[dh * 1024 + e * kWave + lane]) * inv[qi];
            const long orow = a.nq_first_only ? b : row0 + q0 + qi;
            a.out[orow * a.ldo + hoff + dh * 32 + r] = o;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------------------------
int bert_check_h(const char* who, int H) {
    T2_REQUIRE(H >= kWave && H % kWave == 0 && H <= kWave * kBertMaxPerLane, "%s: hidden=%d must be a multiple of 64 between 64 and 1024", who, H);
    return 0;
}

int bert_embed_ln(const t2_bert_embed_ln_args& a, hipStream_t s) {
    T2_TRY_RC(bert_check_h("bert_embed_ln", a.H));
    T2_REQUIRE(a.B >= 1 && a.B <= 65535, "bert_embed_ln: B=%d outside 1..65535", a.B);
    T2_REQUIRE(a.max_len >= 1 && a.total_tokens >= 1, "bert_embed_ln: max_len=%d and total_tokens=%d must be at least 1", a.max_len, a.total_tokens);
    T2_REQUIRE(a.ids && a.cu_seqlens && a.word && a.pos && a.type && a.ln_w && a.ln_b && a.out, "bert_embed_ln: null pointer");
    bert_embed_ln_kernel<<<dim3((a.max_len + kBertRowsPerWg - 1) / kBertRowsPerWg, a.B), dim3(kBertThreads), 0, s>>>(a);
    T2_LAUNCH_CHECK();
    return 0;
}

int bert_layernorm(const t2_bert_layernorm_args& a, hipStream_t s) {
    T2_TRY_RC(bert_check_h("bert_layernorm", a.H));
    T2_REQUIRE(a.rows >= 1, "bert_layernorm: rows=%d must be at least 1", a.rows);
    T2_REQUIRE(a.x && a.ln_w && a.ln_b && a.out, "bert_layernorm: null pointer");
    bert_layernorm_kernel<<<dim3((a.rows + kBertRowsPerWg - 1) / kBertRowsPerWg), dim3(kBertThreads), 0, s>>>(a);
    T2_LAUNCH_CHECK();
    return 0;
}

int bert_attention(const t2_bert_attention_args& a, hipStream_t s) {
    T2_REQUIRE(a.B >= 1 && a.B <= 65535, "bert_attention: B=%d outside 1..65535", a.B);
    T2_REQUIRE(a.heads >= 1 && a.heads <= 65535, "bert_attention: heads=%d outside 1..65535", a.heads);
    T2_REQUIRE(a.max_len >= 1 && a.max_len <= kBertMaxLen, "bert_attention: max_len=%d outside 1..%d", a.max_len, kBertMaxLen);
    T2_REQUIRE(a.total_tokens >= 1, "bert_attention: total_tokens=%d must be at least 1", a.total_tokens);
    T2_REQUIRE(a.q && a.k && a.v && a.cu_seqlens && a.out, "bert_attention: null pointer");
    const long need = (long)a.heads * kBertHeadDim;
    T2_REQUIRE(a.ldq >= need && a.ldk >= need && a.ldv >= need && a.ldo >= need, "bert_attention: a row stride is below heads * 64 = %ld", need);
    auto al = [](const float* p, long ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; };
    T2_REQUIRE(al(a.q, a.ldq) && al(a.k, a.ldk) && al(a.v, a.ldv), "bert_attention: q, k and v need 16-byte aligned pointers and row strides that are multiples of 4");
    const size_t smem = bert_attn_lds_floats(a.max_len) * sizeof(float);
    T2_TRY_RC(t2_allow_dynamic_lds(reinterpret_cast<const void*>(bert_attention_kernel), smem));
    const int qtiles = a.nq_first_only ? 1 : (a.max_len + kBertQT - 1) / kBertQT;
    bert_attention_kernel<<<dim3(qtiles, a.heads, a.B), dim3(kBertThreads), smem, s>>>(a);
    T2_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// the model: packed weights, workspace, driver
// ------------------------------------------------------------------------------------------------------------------
struct BertLayerOff { size_t wqkv, bqkv, wo, bo, ln1w, ln1b, w1, b1, w2, b2, ln2w, ln2b; };
struct BertOff { size_t word, pos, type, lnw, lnb, layer0, per_layer, total; };

int bert_check_config(const t2_bert_config& c) {
    T2_REQUIRE(c.hidden >= 64 && c.hidden % 64 == 0 && c.hidden <= 1024, "bert: hidden=%d must be a multiple of 64 between 64 and 1024", c.hidden);
    T2_REQUIRE(c.heads >= 1 && c.hidden == c.heads * kBertHeadDim, "bert: head dim = hidden / heads = %d / %d must be 64", c.hidden, c.heads);
    T2_REQUIRE(c.intermediate >= 64 && c.intermediate % 64 == 0, "bert: intermediate=%d must be a multiple of 64", c.intermediate);
    T2_REQUIRE(c.layers >= 1, "bert: layers=%d must be at least 1", c.layers);
    T2_REQUIRE(c.vocab >= 1 && c.max_pos >= 1 && c.type_vocab >= 1, "bert: vocab=%d, max_pos=%d and type_vocab=%d must be at least 1", c.vocab, c.max_pos, c.type_vocab);
    T2_REQUIRE(c.ln_eps > 0.f, "bert: ln_eps=%g must be positive", (double)c.ln_eps);
    return 0;
}

BertOff bert_offsets(const t2_bert_config& c) {
    const size_t H = c.hidden, I = c.intermediate;
    BertOff o;
    o.word = 0; o.pos = o.word + (size_t)c.vocab * H; o.type = o.pos + (size_t)c.max_pos * H; o.lnw = o.type + (size_t)c.type_vocab * H;
    o.lnb = o.lnw + H; o.layer0 = o.lnb + H;
    o.per_layer = 3 * H * H + 3 * H + H * H + H + 2 * H + I * H + I + H * I + H + 2 * H;
    o.total = o.layer0 + o.per_layer * c.layers;
    return o;
}
BertLayerOff bert_layer_offsets(const t2_bert_config& c, const BertOff& o, int layer) {
    const size_t H = c.hidden, I = c.intermediate;
    BertLayerOff l;
    l.wqkv = o.layer0 + o.per_layer * layer; l.bqkv = l.wqkv + 3 * H * H; l.wo = l.bqkv + 3 * H; l.bo = l.wo + H * H;
    l.ln1w = l.bo + H; l.ln1b = l.ln1w + H; l.w1 = l.ln1b + H; l.b1 = l.w1 + I * H; l.w2 = l.b1 + I; l.b2 = l.w2 + H * I;
    l.ln2w = l.b2 + H; l.ln2b = l.ln2w + H;
    return l;
}

// workspace, in floats: the residual stream, the fused QKV (or KV) rows, the context rows, the FFN rows; the CLS tail's [B, .] rows
// The CLS tail needs no space of its own behind full layers (B <= T): its rows xc lie in the context rows, its queries qc
// in the third of the QKV rows that the last layer's KV product leaves free, its FFN rows fc in the FFN rows, and its
// context rows ctxc in the stream itself, which is dead once the KV product and the gather have read it.  A one-layer
// CLS-only model has no full layer: stream, KV rows, and xc, qc, fc behind them.
struct BertWs { size_t x, qkv, ctx, ffn, xc, qc, ctxc, fc, total; };
BertWs bert_workspace(const t2_bert_config& c, int B, long total, int cls_only) {
    const size_t H = c.hidden, I = c.intermediate, T = (size_t)total;
    BertWs w;
    w.x = 0; w.qkv = w.x + T * H; w.ctxc = w.x;
    if (cls_only && c.layers == 1) {
        w.xc = w.qkv + T * 2 * H; w.qc = w.xc + (size_t)B * H; w.fc = w.qc + (size_t)B * H; w.total = w.fc + (size_t)B * I;
        w.ctx = w.ffn = w.total;                           // unused
        return w;
    }
    w.ctx = w.qkv + T * 3 * H; w.ffn = w.ctx + T * H; w.total = w.ffn + T * I;
    w.xc = w.ctx; w.qc = w.qkv + T * 2 * H; w.fc = w.ffn;
    return w;
}

}  // namespace
}  // namespace t2

using namespace t2;

int t2_bert_plan(const t2_bert_config* cfg, int B, long total_tokens, int max_len, int cls_only, t2_bert_plan_info* out) {
    T2_REQUIRE(cfg && out, "t2_bert_plan: null pointer");
    T2_TRY_RC(bert_check_config(*cfg));
    const int lim = cfg->max_pos < kBertMaxLen ? cfg->max_pos : kBertMaxLen;
    T2_REQUIRE(max_len >= 1 && max_len <= lim, "bert: max_len=%d outside 1..min(512, max_pos=%d) = %d", max_len, cfg->max_pos, lim);
    T2_REQUIRE(B >= 1 && B <= 65535, "bert: B=%d outside 1..65535", B);
    T2_REQUIRE(total_tokens >= B && total_tokens <= (long)B * max_len, "bert: total_tokens=%ld outside B..B*max_len = %d..%ld", total_tokens, B, (long)B * max_len);
    T2_REQUIRE(total_tokens * (3L * cfg->hidden > cfg->intermediate ? 3L * cfg->hidden : cfg->intermediate) <= INT32_MAX,
               "bert: total_tokens=%ld times the widest row exceeds 2^31-1 elements", total_tokens);
    out->packed_floats = bert_offsets(*cfg).total;
    out->workspace_bytes = bert_workspace(*cfg, B, total_tokens, cls_only).total * sizeof(float);
    // embed; 7 per full layer (QKV, attention, output + residual, LayerNorm, FFN in, FFN out + residual, LayerNorm);
    // the CLS-only last layer: KV, gather, Q, attention, output, LayerNorm, FFN in, FFN out, LayerNorm; else the final gather
    out->launches = 1 + 7 * (cfg->layers - (cls_only ? 1 : 0)) + (cls_only ? 9 : 1);
    return 0;
}

int t2_bert_pack(const t2_bert_config* cfg, const float* const* tensors, int n_tensors, float* packed, void* stream) {
    T2_REQUIRE(cfg && tensors && packed, "t2_bert_pack: null pointer");
    T2_TRY_RC(bert_check_config(*cfg));
    const t2_bert_config& c = *cfg;
    T2_REQUIRE(n_tensors == 5 + 16 * c.layers, "t2_bert_pack: %d tensors given, %d layers take 5 + 16 * layers = %d", n_tensors, c.layers, 5 + 16 * c.layers);
    for (int i = 0; i < n_tensors; ++i) T2_REQUIRE(tensors[i], "t2_bert_pack: tensor %d is null", i);
    hipStream_t s = (hipStream_t)stream;
    const size_t H = c.hidden, I = c.intermediate;
    const BertOff o = bert_offsets(c);
    auto put = [&](size_t off, const float* src, size_t n) { return hipMemcpyAsync(packed + off, src, n * sizeof(float), hipMemcpyDeviceToDevice, s); };
    T2_CHECK_HIP(put(o.word, tensors[0], (size_t)c.vocab * H));
    T2_CHECK_HIP(put(o.pos, tensors[1], (size_t)c.max_pos * H));
    T2_CHECK_HIP(put(o.type, tensors[2], (size_t)c.type_vocab * H));
    T2_CHECK_HIP(put(o.lnw, tensors[3], H));
    T2_CHECK_HIP(put(o.lnb, tensors[4], H));
    for (int l = 0; l < c.layers; ++l) {
        const BertLayerOff lo = bert_layer_offsets(c, o, l);
        const float* const* t = tensors + 5 + 16 * l;
        for (int j = 0; j < 3; ++j) {                      // query, key, value -> one [3H, H] matrix and one [3H] bias
            T2_CHECK_HIP(put(lo.wqkv + j * H * H, t[2 * j], H * H));
            T2_CHECK_HIP(put(lo.bqkv + j * H, t[2 * j + 1], H));
        }
        T2_CHECK_HIP(put(lo.wo, t[6], H * H));   T2_CHECK_HIP(put(lo.bo, t[7], H));
        T2_CHECK_HIP(put(lo.ln1w, t[8], H));     T2_CHECK_HIP(put(lo.ln1b, t[9], H));
        T2_CHECK_HIP(put(lo.w1, t[10], I * H));  T2_CHECK_HIP(put(lo.b1, t[11], I));
        T2_CHECK_HIP(put(lo.w2, t[12], H * I));  T2_CHECK_HIP(put(lo.b2, t[13], H));
        T2_CHECK_HIP(put(lo.ln2w, t[14], H));    T2_CHECK_HIP(put(lo.ln2b, t[15], H));
    }
    return 0;
}

int t2_bert_embed_ln(const t2_bert_embed_ln_args* a, void* stream) {
    T2_REQUIRE(a, "t2_bert_embed_ln: null arguments");
    return bert_embed_ln(*a, (hipStream_t)stream);
}
int t2_bert_layernorm(const t2_bert_layernorm_args* a, void* stream) {
    T2_REQUIRE(a, "t2_bert_layernorm: null arguments");
    return bert_layernorm(*a, (hipStream_t)stream);
}
int t2_bert_attention(const t2_bert_attention_args* a, void* stream) {
    T2_REQUIRE(a, "t2_bert_attention: null arguments");
    return bert_attention(*a, (hipStream_t)stream);
}

int t2_bert_forward(const t2_bert_config* cfg, const t2_bert_fwd_args* a, void* stream) {
    T2_REQUIRE(cfg && a, "t2_bert_forward: null pointer");
    const t2_bert_config& c = *cfg;
    const int cls_only = a->out_hidden == nullptr;
    t2_bert_plan_info pl;
    T2_TRY_RC(t2_bert_plan(cfg, a->B, a->total_tokens, a->max_len, cls_only, &pl));
    T2_REQUIRE(a->packed && a->ids && a->cu_seqlens && a->ws, "t2_bert_forward: null pointer");
    T2_REQUIRE(a->out_hidden || a->out_cls, "t2_bert_forward: out_hidden and out_cls are both null");
    T2_REQUIRE(a->ws_bytes >= pl.workspace_bytes, "t2_bert_forward: workspace of %zu bytes, the plan asks for %zu", a->ws_bytes, pl.workspace_bytes);
    T2_REQUIRE((reinterpret_cast<uintptr_t>(a->ws) & 15) == 0 && (reinterpret_cast<uintptr_t>(a->packed) & 15) == 0, "t2_bert_forward: packed and ws must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int H = c.hidden, I = c.intermediate, B = a->B, T = a->total_tokens;
    const BertOff o = bert_offsets(c);
    const BertWs w = bert_workspace(c, B, T, cls_only);
    float* ws = static_cast<float*>(a->ws);
    float* x = ws + w.x; float* qkv = ws + w.qkv; float* ctx = ws + w.ctx; float* ffn = ws + w.ffn;
    float* xc = ws + w.xc; float* qc = ws + w.qc; float* ctxc = ws + w.ctxc; float* fc = ws + w.fc;
    const float* P = a->packed;

    // C[M, N] = act(A[M, K] W[N, K]^T + bias) + beta C
    auto linear = [&](const float* A, int M, int K, const float* W, const float* bias, int N, float* C, int act, float beta) {
        GemmDesc g = gemm_desc();
        g.A = A; g.sam = K; g.sak = 1; g.B = W; g.sbn = K; g.sbk = 1; g.C = C; g.ldc = N; g.M = M; g.N = N; g.K = K;
        g.bias1 = bias; g.act = act; g.beta = beta; g.fp32_only = 1;
        return gemm(g, s);
    };
    auto norm = [&](const float* in, int rows, size_t lw, size_t lb, float* out) {
        return bert_layernorm(t2_bert_layernorm_args{rows, H, c.ln_eps, in, P + lw, P + lb, out}, s);
    };

    T2_TRY_RC(bert_embed_ln(t2_bert_embed_ln_args{B, T, a->max_len, H, c.ln_eps, a->ids, a->cu_seqlens, P + o.word, P + o.pos, P + o.type, P + o.lnw, P + o.lnb, x}, s));
    for (int l = 0; l < c.layers; ++l) {
        const BertLayerOff lo = bert_layer_offsets(c, o, l);
        const bool last = l == c.layers - 1;
        if (last && cls_only) {
            // keys and values of every row, everything else for the B [CLS] rows
            T2_TRY_RC(linear(x, T, H, P + lo.wqkv + (size_t)H * H, P + lo.bqkv + H, 2 * H, qkv, ACT_NONE, 0.f));
            bert_gather_cls_kernel<<<dim3(B), dim3(kBertThreads), 0, s>>>(x, a->cu_seqlens, T, H, xc);
            T2_LAUNCH_CHECK();
            T2_TRY_RC(linear(xc, B, H, P + lo.wqkv, P + lo.bqkv, H, qc, ACT_NONE, 0.f));
            T2_TRY_RC(bert_attention(t2_bert_attention_args{B, c.heads, T, a->max_len, 1, qc, qkv, qkv + H, H, 2L * H, 2L * H, a->cu_seqlens, ctxc, H}, s));
            T2_TRY_RC(linear(ctxc, B, H, P + lo.wo, P + lo.bo, H, xc, ACT_NONE, 1.f));
            T2_TRY_RC(norm(xc, B, lo.ln1w, lo.ln1b, xc));
            T2_TRY_RC(linear(xc, B, H, P + lo.w1, P + lo.b1, I, fc, ACT_GELU, 0.f));
            T2_TRY_RC(linear(fc, B, I, P + lo.w2, P + lo.b2, H, xc, ACT_NONE, 1.f));
            T2_TRY_RC(norm(xc, B, lo.ln2w, lo.ln2b, a->out_cls));
            break;
        }
        T2_TRY_RC(linear(x, T, H, P + lo.wqkv, P + lo.bqkv, 3 * H, qkv, ACT_NONE, 0.f));
        T2_TRY_RC(bert_attention(t2_bert_attention_args{B, c.heads, T, a->max_len, 0, qkv, qkv + H, qkv + 2 * H, 3L * H, 3L * H, 3L * H, a->cu_seqlens, ctx, H}, s));
        T2_TRY_RC(linear(ctx, T, H, P + lo.wo, P + lo.bo, H, x, ACT_NONE, 1.f));
        T2_TRY_RC(norm(x, T, lo.ln1w, lo.ln1b, x));
        T2_TRY_RC(linear(x, T, H, P + lo.w1, P + lo.b1, I, ffn, ACT_GELU, 0.f));
        T2_TRY_RC(linear(ffn, T, I, P + lo.w2, P + lo.b2, H, x, ACT_NONE, 1.f));
        T2_TRY_RC(norm(x, T, lo.ln2w, lo.ln2b, last ? a->out_hidden : x));
    }
    if (!cls_only && a->out_cls) {
        bert_gather_cls_kernel<<<dim3(B), dim3(kBertThreads), 0, s>>>(a->out_hidden, a->cu_seqlens, T, H, a->out_cls);
        T2_LAUNCH_CHECK();
    }
    return 0;
}
