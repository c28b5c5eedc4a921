// Host state shared by the C-ABI layer (c_api.hip, which defines all of it) and the decoder drivers (decoder.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#define T2_TRY(expr)                \
    do {                            \
        int rc_ = (expr);           \
        if (rc_ != 0) return rc_;   \
    } while (0)

namespace t2 {

// In-situ kernel timing (t2_prof_enable / t2_prof_collect): a ProfScope brackets the launches of its scope with HIP
// events on the launch stream.  Off by default.
enum ProfKind { PK_LSTM_ATT_FWD = 0, PK_ATTN_FWD, PK_LSTM_DEC_FWD, PK_ATTN_BWD, PK_LSTM_ATT_BWD_PW, PK_LSTM_ATT_BWD_GEMM,
                PK_LSTM_DEC_BWD_PW, PK_LSTM_DEC_BWD_GEMM, PK_CHAIN_A_FWD, PK_CHAIN_B_FWD, PK_CHAIN_B_BWD, PK_CHAIN_A_BWD, PK_CHAIN_DEC, PK_COUNT };
struct ProfScope {
    hipStream_t s; bool on;
    ProfScope(int kind, hipStream_t st);
    ~ProfScope();
};

// Side stream of the decoder-LSTM chain and its events (one set per device)
struct Side { hipStream_t s = nullptr; std::vector<hipEvent_t> ev; };
int side_get(Side** out);
int stream_edge(Side& sd, size_t i, hipStream_t from, hipStream_t to);      // record on `from`, make `to` wait

// Pinned slots + events of the decode loop's stop polling (one set per device)
struct StopPoll { hipEvent_t ev[4] = {}; int32_t* host = nullptr; };
int stop_poll_get(StopPoll** out);

// Switches (t2_set_overlap, t2_set_chain, t2_set_chain_bwd, t2_set_split_steps, t2_set_dg_handoff)
extern int g_overlap, g_chain, g_chain_bwd, g_split_steps, g_dg_handoff;

// per-step LSTM launches of the decoder drivers since the last reset (t2_step_counts): forward step {exact, bf16, split},
// recurrent-input gradient {exact, bf16, split}, as the launchers report them
extern uint64_t g_step_counts[6];
int counted(int rc, int base, int family);

// t2_decoder_backward calls since the last reset (t2_defer_counts): [0] tail left on the side stream, [1] finished on the caller's
extern uint64_t g_defer_counts[2];

// casts of a dG buffer into its shared bf16 copy since the last reset (t2_dg_handoff_counts): [0] skipped, the chain stored
// the bf16 rows itself, [1] ran
extern uint64_t g_dg_cast_counts[2];

}  // namespace t2
