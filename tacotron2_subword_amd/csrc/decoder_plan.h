// Plan / executor split of the three decoder passes.  decoder_plan.hip decides — which recurrent steps a pass
// takes, which persistent chains, whether the two chains overlap and in which step ranges, where the bf16 copies lie in the
// GEMM scratch, where the decoder-LSTM weight gradients are issued, which stream the leaf tail takes — as pure functions of
// the canonical dims, the pass's Sizes and a PassEnv: no HIP call, no environment, no global.  decoder.hip executes a plan.
// t2_decoder_pass_plan hands the same plans to tests on a machine without a GPU.
#pragma once
#include <vector>

#include "../../include/t2amd.h"
#include "chain_plan.h"

namespace t2 {

struct Sizes {
    int B, T, Tin, Tsub, M, P, E, Ha, Hd, A, WD, WO, NS;     // NS: attention streams (2 = BERT_Tacotron2, 1 = classic Tacotron2)
};
Sizes sizes_of(const t2_dims& d, int B, int T, int Tin, int Tsub);

// What a pass plan needs to know about the process and the device.  pass_env_here() (decoder.hip) is the one place that asks
// (pass_plan_here, next to it, adds the per-GPU claim once a plan has accepted a chain).
struct PassEnv {
    int precision;                           // 0 fp32, 1 bf16 operands, 2 split-bf16 (t2_set_precision)
    bool split_steps;                        // t2_set_split_steps
    bool chain, chain_bwd, overlap;          // t2_set_chain, t2_set_chain_bwd, t2_set_overlap
    ChainEnv chain_env;
    bool saved_tiles;                        // backward: the forward workspace holds the LSA chain's tanh tiles and location features
    bool dg_handoff;                         // t2_set_dg_handoff: the backward chains may leave dG as bf16 rows
    bool gemm_staging, gemm_tiles256;        // t2_set_gemm_staging, T2_GEMM_256: what plan_gemm is asked with (which products take a copy of dG)
};

// Decode loop, bf16-operand mode: whole-cell weight shadows [W_hh | W_ih[:,P:] | W_ih[:,:P]] (attention LSTMs) and
// [W_ih | W_hh] (decoder LSTM) so that each cell is ONE K-contiguous product, plus the bf16 input rows the producing
// kernels write: att rows [2][NS][B][Ha+E+P] = [h | ctx | prenet], dec rows [2][B][WD+Hd] = [att_h | ctx | ... | dec_h],
// ping-pong on step parity (step t reads buffer t&1 and writes the recurrent parts into (t+1)&1).
struct InferShadows {
    int Ka, Kd; size_t wa[2], wd, rows_a, rows_d, total_floats;
};
InferShadows infer_shadows(const Sizes& z, size_t base);

// lo plane of an attention-LSTM shadow (w16a, w16as, wt16a, wt16as) / a decoder-LSTM shadow (w16d, wt16d), in floats
inline size_t split_lo_a(const Sizes& z, size_t hi) { return hi + (size_t)4 * z.Ha * (z.Ha + z.E) / 2; }
inline size_t split_lo_d(const Sizes& z, size_t hi) { return hi + (size_t)4 * z.Hd * z.Hd / 2; }

void layout_of(const t2_dims& d, const Sizes& z, const PassEnv& env, t2_decoder_layout* L);
void bwd_layout_of(const t2_dims& d, const Sizes& z, const PassEnv& env, t2_decoder_bwd_layout* L);

// shape conditions of the bf16-operand and split-bf16 recurrent steps: B <= 128, recurrent widths multiples of 256
bool step_shapes_ok(const Sizes& z);
bool use_bf16_steps(const Sizes& z, const PassEnv& env);       // precision mode 1
bool use_split_steps(const Sizes& z, const PassEnv& env);      // mode 2 with t2_set_split_steps on
// The recurrent steps of a teacher-forced pass.  The forward and the backward plan both ask here: the backward pass reads the
// weight shadows the forward pass cast into its workspace, so the two must agree, and this is the one statement of the rule.
struct StepMode { bool use16, split; };
StepMode teacher_step_mode(const Sizes& z, const PassEnv& env);
// The decode loop's own rule (whole-cell shadows: K = Ha + E + P and WD + Hd): kept as it is, see DESIGN.md §3
bool infer_use16(const Sizes& z, const InferShadows& I, const PassEnv& env);

// SMA attention backward: two workgroups per (item, stream) when one each would leave CUs idle
int attn_bwd_nsplit(const t2_dims& d, const Sizes& z);

// Step ranges handed from one chain to the other.  One range when the chains share a stream; otherwise about eight,
// with short ranges (16, 32 steps) at the END of time: that is where the forward pass's decoder-LSTM chain finishes
// after the attention chain, and where the backward pass's attention chain waits for the first decoder-LSTM range,
// so whatever the last range holds is exposed.  Even boundaries keep rows-per-range a multiple of 128 at B = 64.
std::vector<int> chunk_bounds(int T, bool overlap);

// A persistent chain of a pass.  asked: the switches, the step mode and the attention kind let the pass plan one; on: it
// was asked for and its plan covers the shape (plan.refusal == CHAIN_OK); otherwise plan.refusal says why not.
struct ChainUse { bool asked, on; ChainShape shape; ChainPlan plan; };

// The GEMM scratch of a pass (layout.gemm_ws, total bytes) as named parts, bytes from its start; bytes == 0: no such part.
//   w_ih16: bf16 copy of the decoder LSTM's W_ih (forward) / W_ih^T (backward), staged once per pass
//   dg16:   the shared row-major bf16 copy of dG that every product reading dG takes (backward)
//   rest:   what the products that read the copies work in (staging of their other operand, split-K partials)
struct ScratchPart { size_t off, bytes; };
struct ScratchCarve {
    ScratchPart w_ih16, dg16, rest; size_t total;
    ScratchPart whole() const { return ScratchPart{0, total}; }
};

// Teacher-forced forward (t2_decoder_forward) and decode loop (t2_decoder_infer)
struct DecPlan {
    bool teacher;
    Sizes z; t2_decoder_layout L; InferShadows I;    // I: decode loop only
    bool use16, split;                               // bf16-operand / split-bf16 recurrent steps
    bool pre16;                                      // forward, bf16 steps: the bf16 copy of W_ih heads the scratch (scratch.w_ih16)
    ScratchCarve scratch;
    ChainUse chain_a, chain_b;                       // attention chain (decode loop: the whole loop), decoder-LSTM chain
    bool chained;                                    // a persistent chain runs
    ChainWsClear clear;                              // what the pass zeroes in its exchange space
    bool saves_tiles;                                // the LSA chain leaves its tanh tiles and location features for the backward chain
    bool overlap; std::vector<int> bounds;           // forward: decoder-LSTM chain on the side stream, step ranges
    int poison_words;                                // > 0: the outputs get the abort poison over that many status words
    int poll;                                        // decode loop: steps per stop poll (= per persistent launch)
};
DecPlan plan_decoder_fwd(const t2_dims& d, const Sizes& z, const PassEnv& env);
DecPlan plan_decoder_infer(const t2_dims& d, const Sizes& z, const PassEnv& env, int poll_every);

enum WgradSite : int {
    WGRADS_CHAIN_B = 0,      // in the step-range loop, on the decoder-LSTM chain's stream, once its recurrence is done
    WGRADS_TAIL              // after the fork of the deferred tail, on the tail's stream, ahead of the streams' tails
};
struct BwdPlan {
    Sizes z; t2_decoder_layout L; t2_decoder_bwd_layout BL;
    bool use16, split;
    bool defer;                                      // the leaf tail stays on the side stream when the entry point returns
    ChainUse chain_a, chain_b;
    bool overlap; std::vector<int> bounds;
    // chain phase: W_ih^T as bf16 at the head of the scratch, the shared dG copy of the decoder LSTM behind it
    bool pre16, share, chunk_cast;                   // chunk_cast: dG is cast range by range, in front of each dDIN product
    ScratchCarve scratch; ScratchPart ddin_ws;       // ddin_ws: scratch of a range's dDIN product
    WgradSite dec_wgrads; bool dec_wgrads_staged;    // where the decoder-LSTM weight gradients are issued; dG copy already filled
    bool tail_on_side;                               // stream of the leaf tail: the side stream (defer) or the caller's
    // tail phase: each stream's shared dG copy heads the scratch (it overwrites the chain phase's)
    bool tail_share; ScratchCarve tail_scratch;
    int nsplit;                                      // position splits of the per-step attention backward
    bool lsa_chain; int dq_parts;                    // partials per dq row / per accumulator that the tail folds
    bool dca_acc_fits;                               // DCA: the per-item accumulators' sum fits the scratch
    // dG hand-off: a persistent chain writes dG as bf16 rows [BT][4H] at the head of the stream's own dG region (BL.dgd / dga /
    // dgas) in place of the fp32 rows; the shared copy is then that region, its cast is skipped, and the carves stay as they are
    // Only where EVERY product that reads that dG takes the copy (plan_gemm: whole tiles, K % 64 — also of the shifted products,
    // K = B*T - B, so B % 64 == 0 — and both operands k-major for the 256-tile weight gradients): a product that ignores the copy
    // reads the fp32 rows, which are then not there
    bool dg_rows_d, dg_rows_a;                       // decoder LSTM (chain B, chunk_cast) / both attention streams (chain A, tail_share)
};
BwdPlan plan_decoder_bwd(const t2_dims& d, const Sizes& z, const PassEnv& env, bool defer_weight_grads);

}  // namespace t2
