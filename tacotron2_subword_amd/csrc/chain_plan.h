// Plan / executor split of the persistent chains.  chain_plan.hip decides — whether a pass takes a chain, its
// tiling and kernel instance, what stays resident in LDS, where every exchange buffer lies in the pass's exchange space — as
// pure functions of a shape and a ChainEnv: no HIP call, no environment, no file.  chain.hip, chain_bwd.hip and chain_enc.hip
// execute a plan: offsets to pointers (apply), the memset the plan names, the instance the plan names.  t2_chain_plan hands
// the same plans to tests on a machine without a GPU.
#pragma once
#include "kernels.h"

namespace t2 {

// What a plan needs to know about the device and the process.  chain_env() (chain.hip) is the one place that asks.
struct ChainEnv { int cus; bool claimed; bool no_resident; };
// take_claim = false: `claimed` is reported true without asking, for a first pass over the pure plan — the per-GPU file lock
// is only asked for once the plan has accepted the shape (plan_here), so a process whose shapes are never covered takes no
// claim.  T2_CHAIN_NO_RESIDENT is read at every call (tests flip it inside one process).
ChainEnv chain_env(bool take_claim);

constexpr int CHAIN_ENC = 3;                 // `kind` of an encoder BiLSTM chain in a ChainShape (ChainKind has the decoder's)
struct ChainShape {
    int kind, dec, NS, B, H, E, A, P, M, Hd, F, Kc, Tin[2];   // encoder chains: NS = directions, H; nothing else
    int backward;                            // encoder chains only (the decoder's directions have a plan function each)
    bool saved_tiles;                        // LSA backward: the forward chain left its tanh tile and location features
    size_t ws_bytes;                         // exchange space of the pass; 0 = exactly what this chain needs (ChainPlan::total)
};

// (the decoder's chain shapes are stated by its pass plans, decoder_plan.hip, and copied into the descriptors from there)
ChainShape enc_chain_shape(int ND, int B, int H, int backward, size_t ws_bytes);

enum ChainRefusal : int {
    CHAIN_OK = 0,
    CHAIN_REFUSE_SHAPE,          // a dimension off the sizes the kernels are written for
    CHAIN_REFUSE_NO_INSTANCE,    // the tiling the shape asks for has no kernel instance (one stream, 97-128 rows)
    CHAIN_REFUSE_DEVICE,         // fewer than 256 CUs
    CHAIN_REFUSE_CLAIM,          // another process holds the device's persistent kernels
    CHAIN_REFUSE_QUERY_PART,     // the tiling's query partials outgrow their part of the exchange space (one stream, 65-96 rows)
    CHAIN_REFUSE_LDS,            // the carve exceeds 160 KB
    CHAIN_REFUSE_LSA_RESIDENT,   // LSA reads processed memory from LDS only and the longest memory does not fit
    CHAIN_REFUSE_SHORT_MEMORY,   // backward: a memory shorter than 16 positions (two position splits per item)
    CHAIN_REFUSE_LSA_SPLIT,      // LSA backward: a position split shorter than the conv halo or longer than 64
    CHAIN_REFUSE_NO_SAVED_TILES, // LSA backward: the forward pass ran on the launch path
    CHAIN_REFUSE_WORKSPACE,      // encoder chains: the caller's exchange space is too small
    CHAIN_REFUSALS
};
const char* chain_refusal_text(ChainRefusal r);

// Kernel instances: the executors' launcher tables are indexed by (instance - first instance of the file)
enum ChainInstance : int {
    CI_FWD_LSTM_11 = 0, CI_FWD_LSTM_12, CI_FWD_SMA_11, CI_FWD_SMA_21, CI_FWD_SMA_22, CI_FWD_LSA_11, CI_FWD_LSA_21, CI_FWD_LSA_22,
    CI_FWD_SMA_DEC, CI_FWD_LSA_DEC,                                                            // chain.hip      <UT, RT>
    CI_BWD_LSTM_1, CI_BWD_LSTM_2, CI_BWD_SMA_1, CI_BWD_SMA_2, CI_BWD_LSA_1, CI_BWD_LSA_2,      // chain_bwd.hip  <MT>
    CI_ENC_FWD, CI_ENC_BWD,                                                                    // chain_enc.hip
    CHAIN_INSTANCES
};
constexpr int CI_FWD_FIRST = CI_FWD_LSTM_11, CI_FWD_COUNT = CI_BWD_LSTM_1 - CI_FWD_FIRST;
constexpr int CI_BWD_FIRST = CI_BWD_LSTM_1, CI_BWD_COUNT = CI_ENC_FWD - CI_BWD_FIRST;
const char* chain_instance_name(int instance);

// Parts of an exchange space, in bytes from its start; bytes == 0: the chain has no such part
enum ChainPartId : int { CP_STATUS = 0, CP_Q, CP_X, CP_XD, CP_XM, CP_CNT, CP_PB, CP_PBC, CP_DQX, CP_CARRYX, CP_WDT, CHAIN_PARTS };
const char* chain_part_name(int part);
struct ChainPart { size_t off, bytes; };

struct ChainPlan {
    ChainRefusal refusal;                    // CHAIN_OK: covered, everything below is set
    int instance, grid; size_t lds_bytes;
    int UT, RT, CS;                          // forward tiling
    int MT, lds_Tc;                          // backward: row tiles, positions per split of the longest memory
    int lds_Tin, lds_Jp, lds_Jm, Jp[2], Jm[2];   // forward LDS residency (ChainDesc)
    size_t q_bytes;                          // query partials of the tiling (<= part[CP_Q].bytes)
    ChainPart part[CHAIN_PARTS];
    ChainPart clear;                         // what the executor zeroes in front of every launch (bytes == 0: nothing)
    size_t total, ws_bytes;                  // the least exchange space the chain needs; the space the offsets were laid out in
};

ChainPlan plan_chain_fwd(const ChainShape& z, const ChainEnv& env);
ChainPlan plan_chain_bwd(const ChainShape& z, const ChainEnv& env);
ChainPlan plan_enc_chain(const ChainShape& z, const ChainEnv& env);
// chain_fwd_ws_clear's range, from the head of a forward exchange space of ws_bytes (ChainWsClear)
ChainPart chain_fwd_clear_range(size_t ws_bytes, ChainWsClear what);

// The plan for the current device and process: the pure plan first, the claim only for a shape it accepts.
template <class Pure>
inline ChainPlan plan_here(Pure pure, const ChainShape& z) {
    ChainPlan p = pure(z, chain_env(false));
    if (p.refusal == CHAIN_OK) p = pure(z, chain_env(true));
    return p;
}

// The plan-owned fields of the kernel arguments; ws = start of the exchange space the plan was laid out in
void apply(const ChainPlan& p, float* ws, ChainDesc* d);
void apply(const ChainPlan& p, float* ws, ChainBwdDesc* d);
void apply(const ChainPlan& p, float* ws, EncChainDesc* d);
void apply(const ChainPlan& p, float* ws, EncChainBwdDesc* d);

// Executors: apply the plan, issue its memset, launch its instance.  ws_floats must be the space the plan was laid out in.
int chain_fwd(ChainDesc d, const ChainPlan& p, float* ws, size_t ws_floats, hipStream_t s);
int chain_bwd(ChainBwdDesc d, const ChainPlan& p, float* ws, size_t ws_floats, hipStream_t s);
int enc_chain_fwd(EncChainDesc d, const ChainPlan& p, float* ws, size_t ws_floats, hipStream_t s);
int enc_chain_bwd(EncChainBwdDesc d, const ChainPlan& p, float* ws, size_t ws_floats, hipStream_t s);

}  // namespace t2
