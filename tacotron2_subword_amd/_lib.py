"""ctypes binding of the C-ABI HIP library (include/t2amd.h).

The product path has no CPU fallback: if ``libt2amd.so`` is missing or a call fails, this
module raises.  Build the library with ``python -c "import __graft_entry__ as g; g.build()"``
(or ``tacotron2_subword_amd.build.build()``).
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("T2AMD_LIB") or os.path.join(_HERE, "libt2amd.so")     # (T2AMD_LIB: development builds of the same library)

ATTN_SMA, ATTN_LSA, ATTN_FWD2, ATTN_GMM, ATTN_DCA = 0, 1, 2, 3, 4

SITE = dict(PRENET1=1, PRENET2=2, PRENET1_SUB=3, PRENET2_SUB=4, ATT_H=5, ATT_C=6, ATT_H_SUB=7, ATT_C_SUB=8,
            DEC_H=9, DEC_C=10, NOISE=11, NOISE_SUB=12, ENC0=16, ENCSUB0=20, POSTNET0=24)

_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)


class Dims(C.Structure):
    _fields_ = [("n_mel", C.c_int), ("prenet_dim", C.c_int), ("enc_dim", C.c_int), ("att_rnn_dim", C.c_int),
                ("dec_rnn_dim", C.c_int), ("att_dim", C.c_int), ("loc_filters", C.c_int), ("loc_kernel", C.c_int),
                ("attention_kind", C.c_int), ("p_att_dropout", C.c_float), ("p_dec_dropout", C.c_float),
                ("p_prenet_dropout", C.c_float), ("n_streams", C.c_int),
                ("score_mask_value", C.c_float), ("score_mask_value_sub", C.c_float), ("score_mask_given", C.c_int)]


class AttentionWeights(C.Structure):
    _fields_ = [("wq", C.c_void_p), ("wm", C.c_void_p), ("v", C.c_void_p), ("loc_conv", C.c_void_p), ("loc_dense", C.c_void_p),
                ("mlp_b1", C.c_void_p), ("mlp_w2", C.c_void_p), ("mlp_b2", C.c_void_p),
                ("dca_T", C.c_void_p), ("dca_bT", C.c_void_p), ("dca_P", C.c_void_p)]


class LstmWeights(C.Structure):
    _fields_ = [("w_ih", C.c_void_p), ("w_hh", C.c_void_p), ("b_ih", C.c_void_p), ("b_hh", C.c_void_p)]


class DecoderWeights(C.Structure):
    _fields_ = [("prenet_w1", C.c_void_p), ("prenet_w2", C.c_void_p), ("prenet_sub_w1", C.c_void_p), ("prenet_sub_w2", C.c_void_p),
                ("att", LstmWeights), ("att_sub", LstmWeights), ("attn", AttentionWeights), ("attn_sub", AttentionWeights),
                ("dec", LstmWeights), ("proj_w", C.c_void_p), ("proj_b", C.c_void_p), ("gate_w", C.c_void_p), ("gate_b", C.c_void_p)]


_LAYOUT_FIELDS = ["total_floats", "x", "p1", "p2", "p1s", "p2s", "pm", "pms", "prea", "preas", "ga", "gas",
                  "cna", "cnas", "ca", "cas", "din", "psel", "psels", "wcum", "wcums", "pred", "gd", "cnd", "cd",
                  "dout", "qs", "qss", "qpart", "w1t", "w16a", "w16as", "w16d", "wt16a", "wt16as", "wt16d", "din16", "dh16",
                  "gemm_ws", "gemm_ws_floats", "chain", "chain_floats", "usave", "usaves", "locsave", "locsaves"]


class DecoderLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in _LAYOUT_FIELDS]


class DecoderFwdArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("Tin", C.c_int), ("Tsub", C.c_int),
                ("memory", C.c_void_p), ("memory_sub", C.c_void_p), ("mem_lengths", C.c_void_p), ("sub_lengths", C.c_void_p),
                ("mels", C.c_void_p), ("mel_out", C.c_void_p), ("gate_out", C.c_void_p), ("align", C.c_void_p),
                ("align_sub", C.c_void_p), ("ws", C.c_void_p), ("training", C.c_int), ("prenet_dropout", C.c_int),
                ("seed", C.c_uint64), ("phase", C.c_int)]


class DecoderInferArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("Tin", C.c_int), ("Tsub", C.c_int), ("max_steps", C.c_int), ("poll_every", C.c_int),
                ("gate_threshold", C.c_float),
                ("memory", C.c_void_p), ("memory_sub", C.c_void_p), ("mem_lengths", C.c_void_p), ("sub_lengths", C.c_void_p),
                ("mel_out", C.c_void_p), ("gate_out", C.c_void_p), ("align", C.c_void_p), ("align_sub", C.c_void_p),
                ("stop_index", C.c_void_p), ("done_count", C.c_void_p), ("ws", C.c_void_p),
                ("prenet_dropout", C.c_int), ("seed", C.c_uint64), ("steps_run_host", C.POINTER(C.c_int))]


class LstmGrads(C.Structure):
    _fields_ = LstmWeights._fields_


class AttentionGrads(C.Structure):
    _fields_ = AttentionWeights._fields_


class DecoderGrads(C.Structure):
    _fields_ = [("prenet_w1", C.c_void_p), ("prenet_w2", C.c_void_p), ("prenet_sub_w1", C.c_void_p), ("prenet_sub_w2", C.c_void_p),
                ("att", LstmGrads), ("att_sub", LstmGrads), ("attn", AttentionGrads), ("attn_sub", AttentionGrads),
                ("dec", LstmGrads), ("proj_w", C.c_void_p), ("proj_b", C.c_void_p), ("gate_w", C.c_void_p), ("gate_b", C.c_void_p)]


_BWD_LAYOUT_FIELDS = ["total_floats", "ddout", "ddin", "dgd", "dga", "dgas", "dctx", "dctxs", "dq", "dqs", "dv", "dvs",
                      "dpm", "dpms", "carry", "carrys", "carryc", "carrycs", "dlconv", "dlconvs", "dldense", "dldenses", "dcd", "dca", "dcas", "partd", "parta", "dp2", "dp2s", "dp1",
                      "dmel_t", "dgate_t", "dg16a", "dg16d", "colsum_ws", "gemm_ws", "gemm_ws_floats", "chain", "chain_floats"]


class DecoderBwdLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in _BWD_LAYOUT_FIELDS]


class DecoderBwdArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("Tin", C.c_int), ("Tsub", C.c_int),
                ("memory", C.c_void_p), ("memory_sub", C.c_void_p), ("align", C.c_void_p), ("align_sub", C.c_void_p),
                ("d_mel", C.c_void_p), ("d_gate", C.c_void_p), ("d_align", C.c_void_p), ("d_align_sub", C.c_void_p),
                ("d_memory", C.c_void_p), ("d_memory_sub", C.c_void_p), ("ws", C.c_void_p), ("bws", C.c_void_p),
                ("training", C.c_int), ("prenet_dropout", C.c_int), ("seed", C.c_uint64), ("defer_weight_grads", C.c_int)]


class ConvBnArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("K", C.c_int),
                ("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("run_mean", C.c_void_p), ("run_var", C.c_void_p),
                ("training", C.c_int), ("eps", C.c_float), ("act", C.c_int), ("drop_p", C.c_float), ("seed", C.c_uint64),
                ("site", C.c_uint32), ("residual", C.c_void_p),
                ("z", C.c_void_p), ("mean", C.c_void_p), ("invstd", C.c_void_p), ("var", C.c_void_p), ("y", C.c_void_p),
                ("ws", C.c_void_p), ("ws_floats", C.c_size_t),
                ("x16", C.c_void_p), ("y16", C.c_void_p), ("handoff", C.c_int)]      # optional bf16 hand-offs (zero: none)


class ConvBnBwdArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("K", C.c_int),
                ("x", C.c_void_p), ("w", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("z", C.c_void_p), ("mean", C.c_void_p), ("invstd", C.c_void_p),
                ("training", C.c_int), ("eps", C.c_float), ("act", C.c_int), ("drop_p", C.c_float), ("seed", C.c_uint64),
                ("site", C.c_uint32), ("dy", C.c_void_p),
                ("dw", C.c_void_p), ("dbias", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p),
                ("dx", C.c_void_p), ("dx_accumulate", C.c_int), ("ws", C.c_void_p), ("ws_floats", C.c_size_t),
                ("x16", C.c_void_p), ("handoff", C.c_int)]


_P4 = C.c_void_p * 4
_I4 = C.c_int * 4


class LstmSeqArgs(C.Structure):
    _fields_ = [("nstreams", C.c_int), ("B", C.c_int), ("T", C.c_int), ("H", C.c_int),
                ("pre", _P4), ("w_hh", _P4), ("reverse", _I4), ("lengths", C.c_void_p),
                ("h", _P4), ("ldh", C.c_long), ("c", _P4), ("gates", _P4), ("ws", C.c_void_p), ("ws_floats", C.c_size_t)]


class LstmSeqBwdArgs(C.Structure):
    _fields_ = [("nstreams", C.c_int), ("B", C.c_int), ("T", C.c_int), ("H", C.c_int),
                ("w_hh", _P4), ("reverse", _I4), ("h", _P4), ("ldh", C.c_long), ("c", _P4), ("gates", _P4),
                ("dh", _P4), ("lddh", C.c_long), ("dpre", _P4), ("dw_hh", _P4), ("ws", C.c_void_p), ("ws_floats", C.c_size_t)]


class GemmArgs(C.Structure):
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("sam", C.c_long), ("sak", C.c_long), ("sbn", C.c_long), ("sbk", C.c_long), ("ldc", C.c_long),
                ("batch", C.c_int), ("bsA", C.c_long), ("bsB", C.c_long), ("bsC", C.c_long),
                ("alpha", C.c_float), ("beta", C.c_float), ("bias", C.c_void_p), ("act", C.c_int),
                ("crow_mod", C.c_int), ("crow_mul", C.c_long), ("ws", C.c_void_p), ("ws_bytes", C.c_size_t), ("splitk", C.c_int)]


class GemmPlanOpts(C.Structure):
    _fields_ = [("conv_a", C.c_int), ("conv_b", C.c_int), ("conv_T", C.c_int), ("conv_C", C.c_int), ("fp32_only", C.c_int),
                ("a16", C.c_int), ("b16", C.c_int), ("lda16", C.c_long), ("ldb16", C.c_long),
                ("a16_kmajor", C.c_int), ("b16_kmajor", C.c_int), ("split16", C.c_int)]


class GemmPlanInfo(C.Structure):
    _fields_ = [("kernel", C.c_int), ("name", C.c_char_p), ("split", C.c_int), ("splitk", C.c_int), ("kchunks", C.c_int),
                ("a_src", C.c_int), ("b_src", C.c_int), ("stage_bytes_a", C.c_size_t), ("stage_bytes_b", C.c_size_t)]


CHAIN_PARTS = 11       # T2_CHAIN_PARTS
CHAIN_KINDS = dict(lstm=0, sma=1, lsa=2, enc=3)
CHAIN_REFUSE_SHAPE, CHAIN_REFUSE_NO_SAVED_TILES = 1, 10      # T2_CHAIN_REFUSE_*: the reasons the tests ask for by value


class ChainShape(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("kind", "dec", "NS", "B", "H", "E", "A", "P", "M", "Hd", "F", "Kc")] + \
               [("Tin", C.c_int * 2), ("saved_tiles", C.c_int), ("ws_floats", C.c_size_t)]


class ChainPlanInfo(C.Structure):
    _fields_ = [("covered", C.c_int), ("reason", C.c_int), ("reason_text", C.c_char_p),
                ("instance", C.c_int), ("instance_name", C.c_char_p), ("grid", C.c_int), ("lds_bytes", C.c_size_t)] + \
               [(n, C.c_int) for n in ("UT", "RT", "CS", "MT", "lds_Tc", "lds_Tin", "lds_Jp", "lds_Jm")] + \
               [("Jp", C.c_int * 2), ("Jm", C.c_int * 2), ("q_bytes", C.c_size_t), ("total_bytes", C.c_size_t), ("ws_bytes", C.c_size_t),
                ("part_off", C.c_size_t * CHAIN_PARTS), ("part_bytes", C.c_size_t * CHAIN_PARTS), ("part_name", C.c_char_p * CHAIN_PARTS),
                ("clear_off", C.c_size_t), ("clear_bytes", C.c_size_t), ("pass_clear_bytes", C.c_size_t * 3)]


PASS_KINDS = dict(forward=0, backward=1, infer=2)       # T2_PASS_*
PASS_MAX_BOUNDS = 64                                    # T2_PASS_MAX_BOUNDS


class PassEnv(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("precision", "split_steps", "chain", "chain_bwd", "overlap", "cus", "claimed", "no_resident", "saved_tiles", "dg_handoff", "gemm_staging")]


class PassChain(C.Structure):
    _fields_ = [("asked", C.c_int), ("on", C.c_int), ("reason", C.c_int), ("reason_text", C.c_char_p),
                ("instance", C.c_int), ("instance_name", C.c_char_p), ("grid", C.c_int)]


class ScratchCarve(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in ("w_ih16_off", "w_ih16_bytes", "dg16_off", "dg16_bytes", "rest_off", "rest_bytes", "total_bytes")]


class DecoderPassPlanInfo(C.Structure):
    _fields_ = [("layout", DecoderLayout), ("bwd_layout", DecoderBwdLayout)] + \
               [(n, C.c_int) for n in ("use16", "split", "pre16")] + [("scratch", ScratchCarve), ("chain_a", PassChain), ("chain_b", PassChain)] + \
               [(n, C.c_int) for n in ("chained", "clear", "saves_tiles", "overlap", "nbounds")] + [("bounds", C.c_int * PASS_MAX_BOUNDS)] + \
               [("poison_words", C.c_int), ("poll", C.c_int), ("shadow_floats", C.c_size_t)] + \
               [(n, C.c_int) for n in ("defer", "share", "chunk_cast")] + [("ddin_ws_off", C.c_size_t), ("ddin_ws_bytes", C.c_size_t)] + \
               [(n, C.c_int) for n in ("dec_wgrads", "dec_wgrads_staged", "tail_on_side", "tail_share")] + [("tail_scratch", ScratchCarve)] + \
               [(n, C.c_int) for n in ("nsplit", "lsa_chain", "dq_parts", "dg_rows_d", "dg_rows_a")]


class SoftDtwPlanInfo(C.Structure):
    _fields_ = [("threads", C.c_int), ("rows_per_thread", C.c_int), ("passes", C.c_int),
                ("d_floats", C.c_size_t), ("r_floats", C.c_size_t), ("e_floats", C.c_size_t)]


class SoftDtwDistArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("M", C.c_int), ("d", C.c_int), ("x", C.c_void_p), ("y", C.c_void_p), ("Ds", C.c_void_p)]


class SoftDtwFwdArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("M", C.c_int), ("gamma", C.c_float), ("bandwidth", C.c_float),
                ("D", C.c_void_p), ("Ds", C.c_void_p), ("x_lengths", C.c_void_p), ("y_lengths", C.c_void_p),
                ("R", C.c_void_p), ("value", C.c_void_p)]


class SoftDtwBwdArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("M", C.c_int), ("gamma", C.c_float), ("bandwidth", C.c_float),
                ("D", C.c_void_p), ("Ds", C.c_void_p), ("x_lengths", C.c_void_p), ("y_lengths", C.c_void_p),
                ("R", C.c_void_p), ("E", C.c_void_p)]


class SoftDtwDistBwdArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("M", C.c_int), ("d", C.c_int), ("x", C.c_void_p), ("y", C.c_void_p),
                ("E", C.c_void_p), ("grad_out", C.c_void_p), ("x_lengths", C.c_void_p), ("y_lengths", C.c_void_p),
                ("dX", C.c_void_p), ("dY", C.c_void_p)]


class SsimPlanInfo(C.Structure):
    _fields_ = [("tile_h", C.c_int), ("tile_w", C.c_int), ("tiles_h", C.c_int), ("tiles_w", C.c_int),
                ("partials", C.c_long), ("partials_t", C.c_long), ("partial_bytes", C.c_size_t), ("map_bytes", C.c_size_t),
                ("lds_fwd_bytes", C.c_size_t), ("lds_bwd_bytes", C.c_size_t)]


class SsimImage(C.Structure):
    _fields_ = [("p", C.c_void_p), ("plane_stride", C.c_long), ("row_stride", C.c_long), ("col_stride", C.c_long)]


class SsimFwdArgs(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("B", "C", "H", "W", "ws", "need_grad")] + \
               [("x", SsimImage), ("y", SsimImage), ("map", SsimImage), ("taps", C.c_void_p), ("partial", C.c_void_p),
                ("coef", C.c_void_p), ("value", C.c_void_p), ("items", C.c_void_p)]


class SsimBwdArgs(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("B", "C", "H", "W", "ws", "need_grad", "per_item")] + \
               [("x", SsimImage), ("y", SsimImage), ("dx", SsimImage), ("dy", SsimImage), ("taps", C.c_void_p), ("coef", C.c_void_p),
                ("grad", C.c_void_p)]


_I6 = C.c_int * 6


class BertConfig(C.Structure):
    _fields_ = [("hidden", C.c_int), ("layers", C.c_int), ("heads", C.c_int), ("intermediate", C.c_int), ("vocab", C.c_int),
                ("max_pos", C.c_int), ("type_vocab", C.c_int), ("ln_eps", C.c_float)]


class BertPlanInfo(C.Structure):
    _fields_ = [("packed_floats", C.c_size_t), ("workspace_bytes", C.c_size_t), ("launches", C.c_int)]


class BertFwdArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("total_tokens", C.c_int), ("max_len", C.c_int), ("packed", C.c_void_p), ("ids", C.c_void_p),
                ("cu_seqlens", C.c_void_p), ("out_hidden", C.c_void_p), ("out_cls", C.c_void_p), ("ws", C.c_void_p), ("ws_bytes", C.c_size_t)]


class BertEmbedLnArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("total_tokens", C.c_int), ("max_len", C.c_int), ("H", C.c_int), ("eps", C.c_float),
                ("ids", C.c_void_p), ("cu_seqlens", C.c_void_p), ("word", C.c_void_p), ("pos", C.c_void_p), ("type", C.c_void_p),
                ("ln_w", C.c_void_p), ("ln_b", C.c_void_p), ("out", C.c_void_p)]


class BertLayernormArgs(C.Structure):
    _fields_ = [("rows", C.c_int), ("H", C.c_int), ("eps", C.c_float), ("x", C.c_void_p), ("ln_w", C.c_void_p), ("ln_b", C.c_void_p),
                ("out", C.c_void_p)]


class BertAttentionArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("heads", C.c_int), ("total_tokens", C.c_int), ("max_len", C.c_int), ("nq_first_only", C.c_int),
                ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("ldq", C.c_long), ("ldk", C.c_long), ("ldv", C.c_long),
                ("cu_seqlens", C.c_void_p), ("out", C.c_void_p), ("ldo", C.c_long)]


class HifiganConfig(C.Structure):
    _fields_ = [("resblock", C.c_int), ("n_mel", C.c_int), ("upsample_initial_channel", C.c_int),
                ("num_upsamples", C.c_int), ("upsample_rates", _I6), ("upsample_kernel_sizes", _I6),
                ("num_kernels", C.c_int), ("resblock_kernel_sizes", _I6),
                ("num_dilations", C.c_int), ("resblock_dilation_sizes", (C.c_int * 3) * 6)]


class HifiganPlanInfo(C.Structure):
    _fields_ = [("out_len", C.c_long), ("workspace_bytes", C.c_size_t), ("packed_bytes", C.c_size_t),
                ("n_layers", C.c_int), ("time_tile", C.c_int)]


class HifiganFwdArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("n_mel", C.c_int), ("packed", C.c_void_p), ("mel", C.c_void_p),
                ("workspace", C.c_void_p), ("audio", C.c_void_p), ("pre_tanh", C.c_void_p)]


class VocoderConvArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("L", C.c_int), ("k", C.c_int), ("d", C.c_int), ("u", C.c_int),
                ("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("residual", C.c_void_p),
                ("y", C.c_void_p), ("packed_ws", C.c_void_p),
                ("slope", C.c_float), ("accumulate", C.c_int), ("scale", C.c_float)]


class HifiganRaggedArgs(C.Structure):
    _fields_ = HifiganFwdArgs._fields_ + [("frames", C.c_void_p), ("sample_lengths", C.c_void_p)]


class VocoderConvRaggedArgs(C.Structure):
    _fields_ = [("conv", VocoderConvArgs), ("lengths", C.c_void_p)]


HIFIGAN_TRAIN_OPS = ("conv", "conv_post", "conv_post_backward", "weight_gradient", "data_gradient")


class HifiganTrainPlanInfo(C.Structure):
    _fields_ = [("out_len", C.c_long), ("tape_bytes", C.c_size_t), ("workspace_bytes", C.c_size_t), ("packed_bytes", C.c_size_t),
                ("packed_bwd_bytes", C.c_size_t), ("grad_floats", C.c_size_t), ("part_bytes", C.c_size_t), ("n_layers", C.c_int),
                ("n_forward_launches", C.c_int), ("n_backward_launches", C.c_int), ("launches", C.c_int * len(HIFIGAN_TRAIN_OPS))]


class HifiganTrainFwdArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("n_mel", C.c_int), ("packed", C.c_void_p), ("mel", C.c_void_p),
                ("tape", C.c_void_p), ("audio", C.c_void_p)]


class HifiganBwdArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("n_mel", C.c_int), ("packed", C.c_void_p), ("packed_bwd", C.c_void_p),
                ("mel", C.c_void_p), ("tape", C.c_void_p), ("audio", C.c_void_p), ("d_audio", C.c_void_p),
                ("workspace", C.c_void_p), ("grads", C.c_void_p), ("d_mel", C.c_void_p)]


HIFIGAN_MPD_LAYERS = 6


class HifiganMpdPlanInfo(C.Structure):
    _fields_ = [("period", C.c_int), ("B", C.c_int), ("T", C.c_int), ("pad", C.c_int), ("H", C.c_int * (HIFIGAN_MPD_LAYERS + 1)),
                ("C", C.c_int * (HIFIGAN_MPD_LAYERS + 1)), ("tiles", C.c_int * HIFIGAN_MPD_LAYERS), ("splits", C.c_int * HIFIGAN_MPD_LAYERS),
                ("fmap_floats", C.c_size_t * HIFIGAN_MPD_LAYERS), ("w_offsets", C.c_size_t * HIFIGAN_MPD_LAYERS),
                ("b_offsets", C.c_size_t * HIFIGAN_MPD_LAYERS), ("packed_bytes", C.c_size_t), ("packed_bwd_bytes", C.c_size_t),
                ("workspace_bytes", C.c_size_t), ("part_bytes", C.c_size_t), ("grad_floats", C.c_size_t),
                ("n_forward_launches", C.c_int), ("n_backward_launches", C.c_int)]


class HifiganMpdFwdArgs(C.Structure):
    _fields_ = [("period", C.c_int), ("B", C.c_int), ("T", C.c_int), ("packed", C.c_void_p), ("audio", C.c_void_p),
                ("fmap", C.c_void_p * HIFIGAN_MPD_LAYERS)]


class HifiganMpdBwdArgs(C.Structure):
    _fields_ = [("period", C.c_int), ("B", C.c_int), ("T", C.c_int), ("packed", C.c_void_p), ("packed_bwd", C.c_void_p), ("audio", C.c_void_p),
                ("fmap", C.c_void_p * HIFIGAN_MPD_LAYERS), ("g_fmap", C.c_void_p * HIFIGAN_MPD_LAYERS),
                ("workspace", C.c_void_p), ("grads", C.c_void_p), ("d_audio", C.c_void_p)]


class VocoderDgradArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("L", C.c_int), ("k", C.c_int), ("d", C.c_int), ("u", C.c_int),
                ("dy", C.c_void_p), ("w", C.c_void_p), ("x", C.c_void_p), ("residual", C.c_void_p),
                ("dx", C.c_void_p), ("packed_ws", C.c_void_p),
                ("slope", C.c_float), ("accumulate", C.c_int), ("scale", C.c_float)]


class VocoderWgradArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("L", C.c_int), ("k", C.c_int), ("d", C.c_int), ("u", C.c_int),
                ("x", C.c_void_p), ("dy", C.c_void_p), ("dw", C.c_void_p), ("db", C.c_void_p), ("part", C.c_void_p),
                ("slope", C.c_float)]


class VocoderPostBwdArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("C", C.c_int), ("L", C.c_int),
                ("x", C.c_void_p), ("w", C.c_void_p), ("audio", C.c_void_p), ("d_audio", C.c_void_p),
                ("dx", C.c_void_p), ("dw", C.c_void_p), ("db", C.c_void_p), ("part", C.c_void_p),
                ("scale", C.c_float)]


VOCODER_TIME_TILE = 128      # include/t2amd.h T2_VOCODER_TIME_TILE


class StftPlanInfo(C.Structure):
    _fields_ = [("bins", C.c_int), ("overlap", C.c_int), ("frame_tile", C.c_int), ("bin_tile", C.c_int), ("out_len", C.c_long),
                ("fwd_floats", C.c_size_t), ("inv_floats", C.c_size_t), ("wsq_floats", C.c_size_t), ("packed_bytes", C.c_size_t)]


class StftAnalysisArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("hop", C.c_int), ("n", C.c_long), ("x", C.c_void_p), ("packed", C.c_void_p),
                ("re", C.c_void_p), ("im", C.c_void_p), ("mag", C.c_void_p), ("phase", C.c_void_p)]


class StftSynthesisArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("hop", C.c_int), ("nf", C.c_int), ("mode", C.c_int), ("windowed", C.c_int),
                ("a", C.c_void_p), ("b", C.c_void_p), ("bias", C.c_void_p), ("strength", C.c_float),
                ("packed", C.c_void_p), ("y", C.c_void_p)]


class StftAnalysisRaggedArgs(C.Structure):
    _fields_ = StftAnalysisArgs._fields_ + [("lengths", C.c_void_p), ("frame_lengths", C.c_void_p)]


class StftSynthesisRaggedArgs(C.Structure):
    _fields_ = StftSynthesisArgs._fields_ + [("frame_lengths", C.c_void_p), ("sample_lengths", C.c_void_p)]


STFT_FRAME_TILE = 32         # include/t2amd.h T2_STFT_FRAME_TILE
STFT_POLAR, STFT_DENOISE = 0, 1


class MelspecPlanInfo(C.Structure):
    _fields_ = [("bins", C.c_int), ("passes", C.c_int), ("frame_tile", C.c_int), ("row_tiles", C.c_int), ("splits", C.c_int),
                ("nf_max", C.c_long), ("frame_tiles", C.c_long), ("fwd_floats", C.c_size_t), ("mel_floats", C.c_size_t),
                ("packed_bytes", C.c_size_t), ("scratch_floats", C.c_size_t), ("split_scratch_floats", C.c_size_t)]


class MelspecArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("hop", C.c_int), ("pad", C.c_int), ("n_mels", C.c_int), ("n", C.c_long),
                ("x", C.c_void_p), ("lengths", C.c_void_p), ("packed", C.c_void_p), ("out", C.c_void_p), ("scratch", C.c_void_p),
                ("scratch_floats", C.c_size_t), ("frame_lengths", C.c_void_p),
                ("mag_eps", C.c_float), ("clip_val", C.c_float), ("C", C.c_float), ("pad_value", C.c_float),
                ("time_major", C.c_int), ("return_power", C.c_int), ("force_splits", C.c_int), ("mel_sum", C.c_void_p)]


class MelspecGradPlanInfo(C.Structure):
    _fields_ = [("bins", C.c_int), ("passes", C.c_int), ("row_tiles", C.c_int), ("overlap", C.c_int), ("nf_max", C.c_long),
                ("grid_x", C.c_long), ("grid_y", C.c_long), ("grid_z", C.c_long), ("fold_grid_x", C.c_long), ("fold_grid_y", C.c_long),
                ("melt_floats", C.c_size_t), ("basis_floats", C.c_size_t), ("packed_bytes", C.c_size_t),
                ("dz_floats", C.c_size_t), ("dxpad_floats", C.c_size_t), ("workspace_floats", C.c_size_t)]


class MelspecBackwardArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("hop", C.c_int), ("pad", C.c_int), ("n_mels", C.c_int), ("n", C.c_long),
                ("x", C.c_void_p), ("lengths", C.c_void_p), ("packed", C.c_void_p), ("grad_packed", C.c_void_p), ("mel_sum", C.c_void_p),
                ("g", C.c_void_p), ("workspace", C.c_void_p), ("workspace_floats", C.c_size_t), ("dx", C.c_void_p),
                ("mag_eps", C.c_float), ("clip_val", C.c_float), ("g_time_major", C.c_int)]


class StftAnalysisBackwardArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("hop", C.c_int), ("n", C.c_long), ("d_re", C.c_void_p), ("d_im", C.c_void_p),
                ("basis_table", C.c_void_p), ("lengths", C.c_void_p), ("dxpad", C.c_void_p), ("dx", C.c_void_p)]


class SilencePlanInfo(C.Structure):
    _fields_ = [("R", C.c_int), ("len_ms", C.c_int), ("chunks", C.c_int), ("chunks_per_group", C.c_int), ("scan_grid", C.c_int * 3),
                ("cut_grid", C.c_int * 2), ("block", C.c_int), ("out_width", C.c_long), ("scratch_bytes", C.c_size_t)]


class SilenceArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("n", C.c_long), ("sample_rate", C.c_int), ("chunk_ms", C.c_int), ("threshold_db", C.c_double),
                ("x", C.c_void_p), ("x_float", C.c_int), ("lengths", C.c_void_p), ("out", C.c_void_p), ("out_float", C.c_int), ("scale", C.c_float),
                ("new_lengths", C.c_void_p), ("start_ms", C.c_void_p), ("end_ms", C.c_void_p), ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
                ("leading_only", C.c_int)]


SILENCE_NONE_SILENT, SILENCE_ALL_SILENT = 0, 32769      # t2_silence_plan_info.R for a threshold of -inf / above 0 dBFS


class WaveglowConfig(C.Structure):
    _fields_ = [("n_mel_channels", C.c_int), ("n_flows", C.c_int), ("n_group", C.c_int), ("n_early_every", C.c_int), ("n_early_size", C.c_int),
                ("n_layers", C.c_int), ("n_channels", C.c_int), ("kernel_size", C.c_int)]


class WaveglowPlanInfo(C.Structure):
    _fields_ = [("L", C.c_long), ("out_len", C.c_long), ("n_remaining_channels", C.c_int), ("n_noise_planes", C.c_int), ("n_tensors", C.c_int),
                ("time_tile", C.c_int), ("workspace_bytes", C.c_size_t), ("packed_bytes", C.c_size_t)]


class WaveglowInferArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("n_mel", C.c_int), ("packed", C.c_void_p), ("mel", C.c_void_p),
                ("noise_host", C.POINTER(C.c_void_p)), ("n_noise", C.c_int), ("sigma", C.c_float),
                ("workspace", C.c_void_p), ("audio", C.c_void_p), ("spect", C.c_void_p), ("flow_audio", C.c_void_p),
                ("kernel_ms_host", C.POINTER(C.c_double))]


class WaveglowGatedArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("nc", C.c_int), ("n_cond", C.c_int), ("L", C.c_int), ("d", C.c_int), ("raw", C.c_int),
                ("x", C.c_void_p), ("spect", C.c_void_p), ("w_in", C.c_void_p), ("b_in", C.c_void_p), ("w_cond", C.c_void_p), ("b_cond", C.c_void_p),
                ("packed_ws", C.c_void_p), ("y", C.c_void_p)]


class WaveglowResSkipArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("nc", C.c_int), ("L", C.c_int), ("first", C.c_int), ("last", C.c_int),
                ("acts", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("packed_ws", C.c_void_p), ("x", C.c_void_p), ("out", C.c_void_p)]


class WaveglowUpsampleArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("n_mel", C.c_int), ("T", C.c_int), ("n_group", C.c_int),
                ("mel", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("packed_ws", C.c_void_p), ("spect", C.c_void_p)]


class WaveglowCoupleArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("nc", C.c_int), ("n_half", C.c_int), ("L", C.c_int), ("n_early", C.c_int), ("in_scale", C.c_float), ("sigma", C.c_float),
                ("out", C.c_void_p), ("w_end", C.c_void_p), ("b_end", C.c_void_p), ("audio_in", C.c_void_p), ("w_inverse", C.c_void_p), ("z", C.c_void_p),
                ("audio_out", C.c_void_p), ("audio_interleaved", C.c_void_p)]


class WaveglowForwardInfo(C.Structure):
    _fields_ = [("L", C.c_long), ("n_log_s_rows", C.c_int), ("n_tensors", C.c_int), ("n_blocks", C.c_long), ("n_partials", C.c_size_t),
                ("workspace_bytes", C.c_size_t), ("packed_bytes", C.c_size_t)]


class WaveglowForwardArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("n_mel", C.c_int), ("n_samples", C.c_long), ("packed", C.c_void_p), ("logdet_w", C.c_void_p),
                ("mel", C.c_void_p), ("audio", C.c_void_p), ("workspace", C.c_void_p), ("z", C.c_void_p), ("log_s_host", C.POINTER(C.c_void_p)),
                ("logdet", C.c_void_p), ("sigma", C.c_float), ("sums", C.c_void_p), ("nll_item", C.c_void_p), ("loss", C.c_void_p),
                ("kernel_ms_host", C.POINTER(C.c_double))]


class WaveglowHeadArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("n_group", C.c_int), ("n_samples", C.c_long), ("audio", C.c_void_p), ("w", C.c_void_p), ("audio_out", C.c_void_p)]


class WaveglowTailArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("nc", C.c_int), ("n_half", C.c_int), ("L", C.c_int), ("n_peel", C.c_int), ("n_group", C.c_int), ("z_offset", C.c_int),
                ("out", C.c_void_p), ("w_end", C.c_void_p), ("b_end", C.c_void_p), ("audio_in", C.c_void_p), ("w_next", C.c_void_p),
                ("audio_out", C.c_void_p), ("z", C.c_void_p), ("log_s", C.c_void_p), ("part_s", C.c_void_p), ("part_z", C.c_void_p)]


class WaveglowBackwardInfo(C.Structure):
    _fields_ = [("L", C.c_long), ("n_tensors", C.c_int), ("saved_bytes", C.c_size_t), ("workspace_bytes", C.c_size_t), ("grad_floats", C.c_size_t),
                ("packed_bwd_bytes", C.c_size_t), ("n_slots", C.c_size_t)]


class WaveglowTrainForwardArgs(C.Structure):
    _fields_ = [("fwd", WaveglowForwardArgs), ("saved", C.c_void_p)]


class WaveglowBackwardArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("n_mel", C.c_int), ("n_samples", C.c_long), ("packed", C.c_void_p), ("packed_bwd", C.c_void_p),
                ("saved", C.c_void_p), ("mel", C.c_void_p), ("audio", C.c_void_p), ("dz", C.c_void_p), ("dlog_s_host", C.POINTER(C.c_void_p)),
                ("workspace", C.c_void_p), ("grad", C.c_void_p), ("kernel_ms_host", C.POINTER(C.c_double))]


class WaveglowWeightGradArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("M", C.c_int), ("nc", C.c_int), ("n_cond", C.c_int), ("L", C.c_int), ("taps", C.c_int), ("d", C.c_int),
                ("a_rows", C.c_int), ("x_rows", C.c_int),
                ("a", C.c_void_p), ("x", C.c_void_p), ("spect", C.c_void_p), ("dw_x", C.c_void_p), ("dw_spect", C.c_void_p), ("db", C.c_void_p),
                ("workspace", C.c_void_p), ("db2", C.c_void_p)]


class WaveglowStartBackwardArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("nc", C.c_int), ("c", C.c_int), ("n_half", C.c_int), ("L", C.c_int), ("dx", C.c_void_p), ("w_start", C.c_void_p),
                ("audio_in", C.c_void_p), ("d_in", C.c_void_p), ("dw_start", C.c_void_p), ("db_start", C.c_void_p), ("workspace", C.c_void_p)]


class WaveglowHeadBackwardArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("n_group", C.c_int), ("n_samples", C.c_long), ("d_in", C.c_void_p), ("audio", C.c_void_p), ("part", C.c_void_p),
                ("dw", C.c_void_p)]


class WaveglowGateBackwardArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("nc", C.c_int), ("L", C.c_int), ("last", C.c_int), ("dx", C.c_void_p), ("d_out", C.c_void_p), ("w_rs", C.c_void_p),
                ("t", C.c_void_p), ("g", C.c_void_p), ("packed_ws", C.c_void_p), ("du", C.c_void_p), ("acts", C.c_void_p)]


class WaveglowConvBackwardArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("nc", C.c_int), ("n_cond", C.c_int), ("L", C.c_int), ("d", C.c_int), ("first_dx", C.c_int), ("first_spect", C.c_int),
                ("du", C.c_void_p), ("w_in", C.c_void_p), ("w_cond", C.c_void_p), ("packed_ws", C.c_void_p), ("dx", C.c_void_p), ("d_spect", C.c_void_p)]


class WaveglowTailBackwardArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("nc", C.c_int), ("n_half", C.c_int), ("L", C.c_int), ("n_peel", C.c_int), ("n_group", C.c_int), ("z_offset", C.c_int),
                ("out", C.c_void_p), ("w_end", C.c_void_p), ("b_end", C.c_void_p), ("audio_in", C.c_void_p), ("w_next", C.c_void_p), ("d_next", C.c_void_p),
                ("dz", C.c_void_p), ("dlog_s", C.c_void_p), ("d_out", C.c_void_p), ("d_in", C.c_void_p), ("part", C.c_void_p), ("dw_end", C.c_void_p),
                ("db_end", C.c_void_p), ("dw_next", C.c_void_p)]


class WaveglowUpsampleBackwardArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("n_mel", C.c_int), ("T", C.c_int), ("n_group", C.c_int), ("n_samples", C.c_long),
                ("mel", C.c_void_p), ("d_spect", C.c_void_p), ("dw", C.c_void_p), ("db", C.c_void_p)]


class AdamTensor(C.Structure):       # one row of the optimizer's device table (optim.py writes them)
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("numel", C.c_long),
                ("first_chunk", C.c_int), ("pad_", C.c_int)]


WAVEGLOW_KERNELS = ("upsample", "start", "gated_conv", "res_skip", "couple")      # include/t2amd.h T2_WAVEGLOW_KERNELS
WAVEGLOW_FORWARD_KERNELS = ("upsample", "start", "gated_conv", "res_skip", "head", "tail", "sums")      # T2_WAVEGLOW_FORWARD_KERNELS
WAVEGLOW_BACKWARD_KERNELS = ("tail_backward", "gate_backward", "conv_backward", "cond_backward", "weight_grad", "weight_grad_reduce", "start_backward",
                             "upsample_backward")      # T2_WAVEGLOW_BACKWARD_KERNELS
WAVEGLOW_GATED, WAVEGLOW_RES_SKIP, WAVEGLOW_UPSAMPLE = 0, 1, 2                      # kinds of t2_waveglow_packed_floats

# include/t2amd.h T2_ABI_VERSION.  tests/test_abi.py compiles the header and holds every struct above (size, field offsets,
# field count), every mirrored constant and every prototype below against it, and checks that the library exports each symbol.
ABI_VERSION = 4

# every symbol include/t2amd.h declares

EXPORTS = ["t2_last_error", "t2_version", "t2_chain_status", "t2_chain_status_clear", "t2_debug_report_abort", "t2_debug_occupy", "t2_chain_claimed", "t2_set_precision", "t2_get_precision", "t2_gemm_counts", "t2_set_gemm_split_min_mflop", "t2_set_split_steps", "t2_get_split_steps", "t2_step_counts", "t2_set_overlap", "t2_set_chain", "t2_get_chain", "t2_set_chain_bwd", "t2_set_gemm_staging", "t2_set_gemm_fold", "t2_set_bn_fuse", "t2_get_bn_fuse", "t2_bn_fuse_counts", "t2_set_dg_handoff", "t2_get_dg_handoff", "t2_dg_handoff_counts", "t2_stage_bf16", "t2_side_join", "t2_defer_counts", "t2_decoder_layout_query", "t2_decoder_forward", "t2_decoder_infer",
           "t2_decoder_bwd_layout_query", "t2_decoder_backward", "t2_decoder_pass_plan", "t2_prof_enable", "t2_prof_collect", "t2_adam_chunks", "t2_adam_step", "t2_adam_norm",
           "t2_conv_bn_forward", "t2_conv_bn_backward", "t2_embedding_forward", "t2_embedding_backward",
           "t2_lstm_seq_forward", "t2_lstm_seq_backward", "t2_lstm_seq_chain_ws_floats", "t2_gemm_ex", "t2_prof_gemm", "t2_gemm_plan", "t2_chain_plan", "t2_conv_handoff_plan", "t2_colsum", "t2_mask_btc",
           "t2_finalize_bct", "t2_mask_bt", "t2_gemm", "t2_rng_keep_mask", "t2_rng_normal",
           "t2_softdtw_plan", "t2_softdtw_dist", "t2_softdtw_forward", "t2_softdtw_backward", "t2_softdtw_dist_backward",
           "t2_ssim_plan", "t2_ssim_forward", "t2_ssim_backward",
           "t2_bert_plan", "t2_bert_pack", "t2_bert_forward", "t2_bert_embed_ln", "t2_bert_layernorm", "t2_bert_attention",
           "t2_hifigan_plan", "t2_hifigan_pack", "t2_hifigan_forward", "t2_hifigan_forward_ragged", "t2_vocoder_packed_floats", "t2_vocoder_conv1d", "t2_vocoder_conv_transpose1d",
           "t2_vocoder_conv_ragged", "t2_hifigan_train_plan", "t2_hifigan_grad_offsets", "t2_hifigan_pack_backward", "t2_hifigan_forward_train", "t2_hifigan_backward",
           "t2_vocoder_dgrad_packed_floats", "t2_vocoder_conv1d_dgrad", "t2_vocoder_conv_transpose1d_dgrad", "t2_vocoder_wgrad_part_floats", "t2_vocoder_wgrad",
           "t2_hifigan_mpd_plan", "t2_hifigan_mpd_pack", "t2_hifigan_mpd_pack_backward", "t2_hifigan_mpd_forward", "t2_hifigan_mpd_backward",
           "t2_vocoder_post_part_doubles", "t2_vocoder_post_backward", "t2_stft_analysis_ragged", "t2_stft_synthesis_ragged",
           "t2_stft_plan", "t2_stft_pack", "t2_stft_analysis", "t2_stft_synthesis", "t2_melspec_plan", "t2_melspec_pack", "t2_melspec",
           "t2_melspec_grad_plan", "t2_melspec_grad_pack", "t2_melspec_backward", "t2_stft_analysis_backward",
           "t2_silence_plan", "t2_silence_trim",
           "t2_waveglow_plan", "t2_waveglow_pack", "t2_waveglow_infer", "t2_waveglow_packed_floats", "t2_waveglow_gated_conv", "t2_waveglow_res_skip",
           "t2_waveglow_upsample", "t2_waveglow_couple", "t2_waveglow_forward_plan", "t2_waveglow_forward", "t2_waveglow_logdet",
           "t2_waveglow_logdet_matrices", "t2_waveglow_head", "t2_waveglow_tail",
           "t2_waveglow_backward_plan", "t2_waveglow_grad_offsets", "t2_waveglow_pack_backward", "t2_waveglow_train_forward", "t2_waveglow_backward",
           "t2_waveglow_weight_grad_ws_floats", "t2_waveglow_weight_grad", "t2_waveglow_gate_backward", "t2_waveglow_conv_backward_packed_floats",
           "t2_waveglow_conv_backward", "t2_waveglow_tail_backward", "t2_waveglow_upsample_backward", "t2_waveglow_start_backward", "t2_waveglow_head_backward"]

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: the HIP extension must be built (see __graft_entry__.build); "
                               "there is no CPU fallback for the product path")
        L = C.CDLL(LIB_PATH)
        L.t2_last_error.restype = C.c_char_p
        if L.t2_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} speaks ABI version {L.t2_version()}, this binding {ABI_VERSION}: rebuild the library "
                               "(the argument structs differ in size between versions)")
        # argtypes for every function with a parameter that is not a plain int (an untyped Python int is passed as a C int:
        # a 64-bit stream handle or pointer would arrive truncated), restype where it is not int
        L.t2_chain_status.argtypes = [C.POINTER(C.c_uint32)]
        L.t2_side_join.argtypes = [C.c_void_p]
        L.t2_adam_chunks.argtypes = [C.c_long]
        L.t2_adam_step.argtypes = [C.POINTER(AdamTensor), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float,
                                   C.c_float, C.c_float, C.c_int, C.c_void_p]
        L.t2_adam_norm.argtypes = [C.POINTER(AdamTensor), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        L.t2_debug_report_abort.argtypes = [C.c_uint32, C.c_void_p]
        L.t2_debug_occupy.argtypes = [C.c_int, C.c_int, C.c_void_p]
        L.t2_gemm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long,
                              C.c_long, C.c_long, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_size_t,
                              C.c_int, C.c_void_p]
        L.t2_rng_keep_mask.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
        L.t2_rng_normal.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.t2_decoder_layout_query.argtypes = [C.POINTER(Dims), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DecoderLayout)]
        L.t2_decoder_forward.argtypes = [C.POINTER(Dims), C.POINTER(DecoderWeights), C.POINTER(DecoderFwdArgs), C.c_void_p]
        L.t2_decoder_infer.argtypes = [C.POINTER(Dims), C.POINTER(DecoderWeights), C.POINTER(DecoderInferArgs), C.c_void_p]
        L.t2_decoder_bwd_layout_query.argtypes = [C.POINTER(Dims), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DecoderBwdLayout)]
        L.t2_decoder_backward.argtypes = [C.POINTER(Dims), C.POINTER(DecoderWeights), C.POINTER(DecoderGrads),
                                          C.POINTER(DecoderBwdArgs), C.c_void_p]
        L.t2_decoder_pass_plan.argtypes = [C.POINTER(Dims), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PassEnv), C.c_int, C.c_int,
                                           C.POINTER(DecoderPassPlanInfo)]
        L.t2_conv_bn_forward.argtypes = [C.POINTER(ConvBnArgs), C.c_void_p]
        L.t2_conv_bn_backward.argtypes = [C.POINTER(ConvBnBwdArgs), C.c_void_p]
        L.t2_embedding_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.t2_embedding_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.t2_lstm_seq_forward.argtypes = [C.POINTER(LstmSeqArgs), C.c_void_p]
        L.t2_lstm_seq_backward.argtypes = [C.POINTER(LstmSeqBwdArgs), C.c_void_p]
        L.t2_lstm_seq_chain_ws_floats.argtypes, L.t2_lstm_seq_chain_ws_floats.restype = [C.c_int, C.c_int, C.c_int, C.c_int], C.c_size_t
        L.t2_gemm_ex.argtypes = [C.POINTER(GemmArgs), C.c_void_p]
        L.t2_prof_gemm.argtypes = [C.POINTER(GemmArgs), C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p]
        L.t2_gemm_plan.argtypes = [C.POINTER(GemmArgs), C.POINTER(GemmPlanOpts), C.POINTER(GemmPlanInfo)]
        L.t2_chain_plan.argtypes = [C.POINTER(ChainShape), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ChainPlanInfo)]
        L.t2_conv_handoff_plan.argtypes = [C.POINTER(GemmArgs), C.POINTER(GemmPlanOpts), C.POINTER(C.c_int), C.POINTER(GemmPlanInfo)]
        L.t2_colsum.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.t2_mask_btc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p]
        L.t2_prof_enable.argtypes = [C.c_int]
        L.t2_gemm_counts.argtypes = [C.POINTER(C.c_uint64), C.c_int]
        L.t2_set_split_steps.argtypes = [C.c_int]
        L.t2_step_counts.argtypes = [C.POINTER(C.c_uint64), C.c_int]
        L.t2_bn_fuse_counts.argtypes = [C.POINTER(C.c_uint64), C.c_int]
        L.t2_defer_counts.argtypes = [C.POINTER(C.c_uint64), C.c_int]
        L.t2_dg_handoff_counts.argtypes = [C.POINTER(C.c_uint64), C.c_int]
        L.t2_stage_bf16.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.t2_set_gemm_split_min_mflop.argtypes = [C.c_int]
        L.t2_prof_collect.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.t2_finalize_bct.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p]
        L.t2_mask_bt.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p]
        L.t2_softdtw_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.POINTER(SoftDtwPlanInfo)]
        L.t2_softdtw_dist.argtypes = [C.POINTER(SoftDtwDistArgs), C.c_void_p]
        L.t2_softdtw_forward.argtypes = [C.POINTER(SoftDtwFwdArgs), C.c_void_p]
        L.t2_softdtw_backward.argtypes = [C.POINTER(SoftDtwBwdArgs), C.c_void_p]
        L.t2_softdtw_dist_backward.argtypes = [C.POINTER(SoftDtwDistBwdArgs), C.c_void_p]
        L.t2_ssim_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SsimPlanInfo)]
        L.t2_ssim_forward.argtypes = [C.POINTER(SsimFwdArgs), C.c_void_p]
        L.t2_ssim_backward.argtypes = [C.POINTER(SsimBwdArgs), C.c_void_p]
        L.t2_bert_plan.argtypes = [C.POINTER(BertConfig), C.c_int, C.c_long, C.c_int, C.c_int, C.POINTER(BertPlanInfo)]
        L.t2_bert_pack.argtypes = [C.POINTER(BertConfig), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p]
        L.t2_bert_forward.argtypes = [C.POINTER(BertConfig), C.POINTER(BertFwdArgs), C.c_void_p]
        L.t2_bert_embed_ln.argtypes = [C.POINTER(BertEmbedLnArgs), C.c_void_p]
        L.t2_bert_layernorm.argtypes = [C.POINTER(BertLayernormArgs), C.c_void_p]
        L.t2_bert_attention.argtypes = [C.POINTER(BertAttentionArgs), C.c_void_p]
        L.t2_hifigan_plan.argtypes = [C.POINTER(HifiganConfig), C.c_int, C.c_int, C.POINTER(HifiganPlanInfo)]
        L.t2_hifigan_pack.argtypes = [C.POINTER(HifiganConfig), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p]
        L.t2_hifigan_forward.argtypes = [C.POINTER(HifiganConfig), C.POINTER(HifiganFwdArgs), C.c_void_p]
        L.t2_vocoder_packed_floats.argtypes, L.t2_vocoder_packed_floats.restype = [C.c_int, C.c_int, C.c_int, C.c_int], C.c_size_t
        L.t2_vocoder_conv1d.argtypes = [C.POINTER(VocoderConvArgs), C.c_void_p]
        L.t2_vocoder_conv_transpose1d.argtypes = [C.POINTER(VocoderConvArgs), C.c_void_p]
        L.t2_stft_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(StftPlanInfo)]
        L.t2_stft_pack.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.t2_stft_analysis.argtypes = [C.POINTER(StftAnalysisArgs), C.c_void_p]
        L.t2_stft_synthesis.argtypes = [C.POINTER(StftSynthesisArgs), C.c_void_p]
        L.t2_hifigan_forward_ragged.argtypes = [C.POINTER(HifiganConfig), C.POINTER(HifiganRaggedArgs), C.c_void_p]
        L.t2_vocoder_conv_ragged.argtypes = [C.POINTER(VocoderConvRaggedArgs), C.c_void_p]
        L.t2_hifigan_train_plan.argtypes = [C.POINTER(HifiganConfig), C.c_int, C.c_int, C.POINTER(HifiganTrainPlanInfo)]
        L.t2_hifigan_grad_offsets.argtypes = [C.POINTER(HifiganConfig), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_int]
        L.t2_hifigan_pack_backward.argtypes = [C.POINTER(HifiganConfig), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p]
        L.t2_hifigan_forward_train.argtypes = [C.POINTER(HifiganConfig), C.POINTER(HifiganTrainFwdArgs), C.c_void_p]
        L.t2_hifigan_backward.argtypes = [C.POINTER(HifiganConfig), C.POINTER(HifiganBwdArgs), C.c_void_p]
        L.t2_vocoder_dgrad_packed_floats.argtypes, L.t2_vocoder_dgrad_packed_floats.restype = [C.c_int] * 4, C.c_size_t
        L.t2_vocoder_conv1d_dgrad.argtypes = [C.POINTER(VocoderDgradArgs), C.c_void_p]
        L.t2_vocoder_conv_transpose1d_dgrad.argtypes = [C.POINTER(VocoderDgradArgs), C.c_void_p]
        L.t2_vocoder_wgrad_part_floats.argtypes, L.t2_vocoder_wgrad_part_floats.restype = [C.c_int] * 7, C.c_size_t
        L.t2_vocoder_wgrad.argtypes = [C.POINTER(VocoderWgradArgs), C.c_void_p]
        L.t2_vocoder_post_part_doubles.argtypes, L.t2_vocoder_post_part_doubles.restype = [C.c_int] * 3, C.c_size_t
        L.t2_vocoder_post_backward.argtypes = [C.POINTER(VocoderPostBwdArgs), C.c_void_p]
        L.t2_hifigan_mpd_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(HifiganMpdPlanInfo)]
        L.t2_hifigan_mpd_pack.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]
        L.t2_hifigan_mpd_pack_backward.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]
        L.t2_hifigan_mpd_forward.argtypes = [C.POINTER(HifiganMpdFwdArgs), C.c_void_p]
        L.t2_hifigan_mpd_backward.argtypes = [C.POINTER(HifiganMpdBwdArgs), C.c_void_p]
        L.t2_stft_analysis_ragged.argtypes = [C.POINTER(StftAnalysisRaggedArgs), C.c_void_p]
        L.t2_stft_synthesis_ragged.argtypes = [C.POINTER(StftSynthesisRaggedArgs), C.c_void_p]
        L.t2_melspec_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_int, C.POINTER(MelspecPlanInfo)]
        L.t2_melspec_pack.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.t2_melspec.argtypes = [C.POINTER(MelspecArgs), C.c_void_p]
        L.t2_melspec_grad_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_int, C.POINTER(MelspecGradPlanInfo)]
        L.t2_melspec_grad_pack.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.t2_melspec_backward.argtypes = [C.POINTER(MelspecBackwardArgs), C.c_void_p]
        L.t2_stft_analysis_backward.argtypes = [C.POINTER(StftAnalysisBackwardArgs), C.c_void_p]
        L.t2_silence_plan.argtypes = [C.c_int, C.c_int, C.c_double, C.c_long, C.c_int, C.POINTER(SilencePlanInfo)]
        L.t2_silence_trim.argtypes = [C.POINTER(SilenceArgs), C.c_void_p]
        L.t2_waveglow_plan.argtypes = [C.POINTER(WaveglowConfig), C.c_int, C.c_int, C.POINTER(WaveglowPlanInfo)]
        L.t2_waveglow_pack.argtypes = [C.POINTER(WaveglowConfig), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p]
        L.t2_waveglow_infer.argtypes = [C.POINTER(WaveglowConfig), C.POINTER(WaveglowInferArgs), C.c_void_p]
        L.t2_waveglow_packed_floats.argtypes, L.t2_waveglow_packed_floats.restype = [C.c_int, C.c_int, C.c_int, C.c_int], C.c_size_t
        L.t2_waveglow_gated_conv.argtypes = [C.POINTER(WaveglowGatedArgs), C.c_void_p]
        L.t2_waveglow_res_skip.argtypes = [C.POINTER(WaveglowResSkipArgs), C.c_void_p]
        L.t2_waveglow_upsample.argtypes = [C.POINTER(WaveglowUpsampleArgs), C.c_void_p]
        L.t2_waveglow_couple.argtypes = [C.POINTER(WaveglowCoupleArgs), C.c_void_p]
        L.t2_waveglow_forward_plan.argtypes = [C.POINTER(WaveglowConfig), C.c_int, C.c_int, C.c_long, C.POINTER(WaveglowForwardInfo)]
        L.t2_waveglow_forward.argtypes = [C.POINTER(WaveglowConfig), C.POINTER(WaveglowForwardArgs), C.c_void_p]
        L.t2_waveglow_logdet.argtypes = [C.POINTER(WaveglowConfig), C.c_void_p, C.c_void_p, C.c_void_p]
        L.t2_waveglow_logdet_matrices.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.t2_waveglow_head.argtypes = [C.POINTER(WaveglowHeadArgs), C.c_void_p]
        L.t2_waveglow_tail.argtypes = [C.POINTER(WaveglowTailArgs), C.c_void_p]
        L.t2_waveglow_backward_plan.argtypes = [C.POINTER(WaveglowConfig), C.c_int, C.c_int, C.c_long, C.POINTER(WaveglowBackwardInfo)]
        L.t2_waveglow_grad_offsets.argtypes = [C.POINTER(WaveglowConfig), C.POINTER(C.c_size_t), C.c_int]
        L.t2_waveglow_pack_backward.argtypes = [C.POINTER(WaveglowConfig), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p]
        L.t2_waveglow_train_forward.argtypes = [C.POINTER(WaveglowConfig), C.POINTER(WaveglowTrainForwardArgs), C.c_void_p]
        L.t2_waveglow_backward.argtypes = [C.POINTER(WaveglowConfig), C.POINTER(WaveglowBackwardArgs), C.c_void_p]
        L.t2_waveglow_weight_grad_ws_floats.argtypes, L.t2_waveglow_weight_grad_ws_floats.restype = [C.c_int] * 6, C.c_size_t
        L.t2_waveglow_weight_grad.argtypes = [C.POINTER(WaveglowWeightGradArgs), C.c_void_p]
        L.t2_waveglow_gate_backward.argtypes = [C.POINTER(WaveglowGateBackwardArgs), C.c_void_p]
        L.t2_waveglow_conv_backward_packed_floats.argtypes, L.t2_waveglow_conv_backward_packed_floats.restype = [C.c_int, C.c_int], C.c_size_t
        L.t2_waveglow_conv_backward.argtypes = [C.POINTER(WaveglowConvBackwardArgs), C.c_void_p]
        L.t2_waveglow_tail_backward.argtypes = [C.POINTER(WaveglowTailBackwardArgs), C.c_void_p]
        L.t2_waveglow_upsample_backward.argtypes = [C.POINTER(WaveglowUpsampleBackwardArgs), C.c_void_p]
        L.t2_waveglow_start_backward.argtypes = [C.POINTER(WaveglowStartBackwardArgs), C.c_void_p]
        L.t2_waveglow_head_backward.argtypes = [C.POINTER(WaveglowHeadBackwardArgs), C.c_void_p]
        _lib = L
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"t2amd call failed ({rc}): {lib().t2_last_error().decode()}")


def ptr(t: torch.Tensor | None) -> int | None:
    """Device pointer of a contiguous CUDA(HIP) tensor; None -> NULL."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("t2amd: tensors must live on the GPU (no CPU fallback in the product path)")
    if not t.is_contiguous():
        raise RuntimeError("t2amd: tensor must be contiguous")
    return t.data_ptr()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def adam_table(address: int):
    """The `table` argument of t2_adam_norm / t2_adam_step: rows of AdamTensor at a device address."""
    return C.cast(address, C.POINTER(AdamTensor))


def lengths_arg(who: str, lengths, B: int, hi: int, dev, lo: int = 0, too_short=None) -> torch.Tensor:
    """Per-item lengths in the convention of stft.log_mel, as the int32 device tensor [B] the kernels take.  Python ints are
    checked here against [lo, hi] and an offender raises with its index and value (below lo: `too_short(i, v)` where given);
    a device tensor is not read back, so nothing synchronises: the kernels clamp it to the row."""
    if isinstance(lengths, torch.Tensor):
        if lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,) or lengths.device != dev:
            raise RuntimeError(f"{who}: lengths must be int32 [{B}] on {dev}, got {lengths.dtype} {tuple(lengths.shape)} on {lengths.device}")
        return lengths.detach().contiguous()
    try:
        vals = [int(v) for v in lengths]
    except TypeError:
        raise RuntimeError(f"{who}: lengths must be None, a list of {B} ints or an int32 tensor [{B}] on {dev}, got {lengths!r}") from None
    if len(vals) != B:
        raise RuntimeError(f"{who}: {len(vals)} lengths for a batch of {B}")
    for i, v in enumerate(vals):
        if v > hi:
            raise RuntimeError(f"{who}: lengths[{i}]={v} exceeds the {hi} a row holds")
        if v < lo:
            raise too_short(i, v) if too_short else RuntimeError(f"{who}: lengths[{i}]={v} is below {lo}")
    return torch.tensor(vals, dtype=torch.int32).to(dev)


def dims_from_hparams(hp, n_streams: int = 2) -> Dims:
    g = (lambda k: hp[k]) if isinstance(hp, dict) else (lambda k: getattr(hp, k))
    kind = {"StepwiseMonotonicAttention": ATTN_SMA, "ForwardAttentionV2": ATTN_FWD2, "GMMAttention": ATTN_GMM,
            "DynamicConvolutionAttention": ATTN_DCA}.get(g("attention"), ATTN_LSA)
    return Dims(int(g("n_mel_channels")) * int(g("n_frames_per_step")), int(g("prenet_dim")), int(g("encoder_embedding_dim")),
                int(g("attention_rnn_dim")), int(g("decoder_rnn_dim")), int(g("attention_dim")),
                int(g("attention_location_n_filters")), int(g("attention_location_kernel_size")), kind,
                float(g("p_attention_dropout")), float(g("p_decoder_dropout")), 0.5, n_streams)


def decoder_weights(P: dict, kind: int, prefix: str = "decoder.", single: bool = False) -> DecoderWeights:
    """Pack device pointers of a (reference-keyed) state dict; the tensors must outlive the call.
    single: classic one-stream decoder (no *_bert modules)."""
    p = lambda k: ptr(P[prefix + k])
    lstm = lambda n: LstmWeights(p(n + ".weight_ih"), p(n + ".weight_hh"), p(n + ".bias_ih"), p(n + ".bias_hh"))

    def attn(n):
        if kind == ATTN_SMA:
            return AttentionWeights(p(n + ".query_layer.linear_layer.weight"), p(n + ".memory_layer.linear_layer.weight"),
                                    p(n + ".v.weight"), None, None)
        if kind == ATTN_DCA:       # W plays the part of the query projection (attention.py:222, 244)
            return AttentionWeights(p(n + ".W.weight"), None, p(n + ".v.weight"), p(n + ".F.weight"), p(n + ".U.weight"),
                                    p(n + ".W.bias"), p(n + ".V.weight"), None, p(n + ".T.weight"), p(n + ".T.bias"), p(n + ".P"))
        if kind == ATTN_GMM:       # mlp.0 plays the part of the query projection (attention.py:412-415)
            return AttentionWeights(p(n + ".mlp.0.weight"), None, None, None, None,       # memory_layer is never read
                                    p(n + ".mlp.0.bias"), p(n + ".mlp.2.weight"), p(n + ".mlp.2.bias"))
        return AttentionWeights(p(n + ".query_layer.linear_layer.weight"), p(n + ".memory_layer.linear_layer.weight"),
                                p(n + ".v.linear_layer.weight"), p(n + ".location_layer.location_conv.conv.weight"),
                                p(n + ".location_layer.location_dense.linear_layer.weight"))
    none_l, none_a = LstmWeights(None, None, None, None), AttentionWeights()
    return DecoderWeights(p("prenet.layers.0.linear_layer.weight"), p("prenet.layers.1.linear_layer.weight"),
                          None if single else p("prenet_bert.layers.0.linear_layer.weight"),
                          None if single else p("prenet_bert.layers.1.linear_layer.weight"),
                          lstm("attention_rnn"), none_l if single else lstm("attention_rnn_bert"),
                          attn("attention_layer"), none_a if single else attn("attention_layer_bert"),
                          lstm("decoder_rnn"), p("linear_projection.linear_layer.weight"), p("linear_projection.linear_layer.bias"),
                          p("gate_layer.linear_layer.weight"), p("gate_layer.linear_layer.bias"))


DECODER_PARAM_KEYS_SMA = [
    "prenet.layers.0.linear_layer.weight", "prenet.layers.1.linear_layer.weight",
    "prenet_bert.layers.0.linear_layer.weight", "prenet_bert.layers.1.linear_layer.weight",
    "attention_rnn.weight_ih", "attention_rnn.weight_hh", "attention_rnn.bias_ih", "attention_rnn.bias_hh",
    "attention_rnn_bert.weight_ih", "attention_rnn_bert.weight_hh", "attention_rnn_bert.bias_ih", "attention_rnn_bert.bias_hh",
    "attention_layer.query_layer.linear_layer.weight", "attention_layer.memory_layer.linear_layer.weight", "attention_layer.v.weight",
    "attention_layer_bert.query_layer.linear_layer.weight", "attention_layer_bert.memory_layer.linear_layer.weight",
    "attention_layer_bert.v.weight",
    "decoder_rnn.weight_ih", "decoder_rnn.weight_hh", "decoder_rnn.bias_ih", "decoder_rnn.bias_hh",
    "linear_projection.linear_layer.weight", "linear_projection.linear_layer.bias",
    "gate_layer.linear_layer.weight", "gate_layer.linear_layer.bias"]


def _lsa_keys():
    out = []
    for k in DECODER_PARAM_KEYS_SMA:
        if k.endswith(".v.weight"):
            n = k[:-len(".v.weight")]
            out += [n + ".v.linear_layer.weight", n + ".location_layer.location_conv.conv.weight",
                    n + ".location_layer.location_dense.linear_layer.weight"]
        else:
            out.append(k)
    return out


DECODER_PARAM_KEYS_LSA = _lsa_keys()


def _gmm_keys():
    """Parameters that receive a gradient with GMMAttention: its memory_layer does not (never used, attention.py:401-506)."""
    out = []
    for k in DECODER_PARAM_KEYS_SMA:
        if ".query_layer." in k:
            n = k[:k.index(".query_layer.")]
            out += [n + ".mlp.0.weight", n + ".mlp.0.bias", n + ".mlp.2.weight", n + ".mlp.2.bias"]
        elif ".memory_layer." in k or k.endswith(".v.weight"):
            continue
        else:
            out.append(k)
    return out


DECODER_PARAM_KEYS_GMM = _gmm_keys()


def _dca_keys():
    """Parameters that receive a gradient with DynamicConvolutionAttention (memory_layer does not; P is a buffer)."""
    out = []
    for k in DECODER_PARAM_KEYS_SMA:
        if ".query_layer." in k:
            n = k[:k.index(".query_layer.")]
            out += [n + s for s in (".W.weight", ".W.bias", ".V.weight", ".F.weight", ".U.weight", ".T.weight", ".T.bias", ".v.weight")]
        elif ".memory_layer." in k or k.endswith(".v.weight"):
            continue
        else:
            out.append(k)
    return out


DECODER_PARAM_KEYS_DCA = _dca_keys()


def decoder_param_keys(kind: int, single: bool = False):
    keys = {ATTN_SMA: DECODER_PARAM_KEYS_SMA, ATTN_GMM: DECODER_PARAM_KEYS_GMM, ATTN_DCA: DECODER_PARAM_KEYS_DCA}.get(kind, DECODER_PARAM_KEYS_LSA)
    return [k for k in keys if "_bert" not in k] if single else keys


def decoder_grads(G: dict, prefix: str = "decoder.", single: bool = False, kind: int = ATTN_SMA) -> DecoderGrads:
    """Pack pointers of gradient buffers keyed like the weights."""
    p = lambda k: ptr(G[prefix + k])
    lstm = lambda n: LstmGrads(p(n + ".weight_ih"), p(n + ".weight_hh"), p(n + ".bias_ih"), p(n + ".bias_hh"))

    def attn(n):
        if kind == ATTN_SMA:
            return AttentionGrads(p(n + ".query_layer.linear_layer.weight"), p(n + ".memory_layer.linear_layer.weight"),
                                  p(n + ".v.weight"), None, None)
        if kind == ATTN_DCA:
            return AttentionGrads(p(n + ".W.weight"), None, p(n + ".v.weight"), p(n + ".F.weight"), p(n + ".U.weight"),
                                  p(n + ".W.bias"), p(n + ".V.weight"), None, p(n + ".T.weight"), p(n + ".T.bias"), None)
        if kind == ATTN_GMM:
            return AttentionGrads(p(n + ".mlp.0.weight"), None, None, None, None,
                                  p(n + ".mlp.0.bias"), p(n + ".mlp.2.weight"), p(n + ".mlp.2.bias"))
        return AttentionGrads(p(n + ".query_layer.linear_layer.weight"), p(n + ".memory_layer.linear_layer.weight"),
                              p(n + ".v.linear_layer.weight"), p(n + ".location_layer.location_conv.conv.weight"),
                              p(n + ".location_layer.location_dense.linear_layer.weight"))
    none_l, none_a = LstmGrads(None, None, None, None), AttentionGrads()
    return DecoderGrads(p("prenet.layers.0.linear_layer.weight"), p("prenet.layers.1.linear_layer.weight"),
                        None if single else p("prenet_bert.layers.0.linear_layer.weight"),
                        None if single else p("prenet_bert.layers.1.linear_layer.weight"),
                        lstm("attention_rnn"), none_l if single else lstm("attention_rnn_bert"),
                        attn("attention_layer"), none_a if single else attn("attention_layer_bert"),
                        lstm("decoder_rnn"), p("linear_projection.linear_layer.weight"), p("linear_projection.linear_layer.bias"),
                        p("gate_layer.linear_layer.weight"), p("gate_layer.linear_layer.bias"))


def decoder_bwd_layout(dims: Dims, B: int, T: int, Tin: int, Tsub: int) -> DecoderBwdLayout:
    L = DecoderBwdLayout()
    check(lib().t2_decoder_bwd_layout_query(C.byref(dims), B, T, Tin, Tsub, C.byref(L)))
    return L


def decoder_layout(dims: Dims, B: int, T: int, Tin: int, Tsub: int) -> DecoderLayout:
    L = DecoderLayout()
    check(lib().t2_decoder_layout_query(C.byref(dims), B, T, Tin, Tsub, C.byref(L)))
    return L


PROF_KINDS = ["att_lstm_fwd", "attention_fwd", "dec_lstm_fwd", "attention_bwd", "att_lstm_bwd_pointwise",
              "att_lstm_bwd_gemm", "dec_lstm_bwd_pointwise", "dec_lstm_bwd_gemm", "chain_a_fwd", "chain_b_fwd", "chain_b_bwd", "chain_a_bwd", "chain_dec"]


def prof_enable(max_launches: int) -> None:
    check(lib().t2_prof_enable(max_launches))


def prof_collect() -> dict:
    """{kind: (total_ms, launches)} of the launches recorded since prof_enable (HIP events on the launch stream)."""
    n = len(PROF_KINDS)
    ms, cnt = (C.c_double * n)(), (C.c_int * n)()
    check(lib().t2_prof_collect(n, ms, cnt))
    return {k: (ms[i], cnt[i]) for i, k in enumerate(PROF_KINDS)}


def set_chain(on: bool) -> None:
    """Persistent chain kernels for teacher-forced passes (include/t2amd.h: t2_set_chain)."""
    check(lib().t2_set_chain(int(bool(on))))


def set_chain_bwd(on: bool) -> None:
    check(lib().t2_set_chain_bwd(int(bool(on))))


def get_chain() -> bool:
    return bool(lib().t2_get_chain())


PRECISION_MODES = {"f32": 0, "fp32": 0, "bf16": 1, "bf16x3": 2}


def set_precision(mode: str) -> None:
    """"f32": exact fp32 GEMMs (parity path, default).  "bf16": bf16 operands / fp32 accumulate for large GEMMs and the
    recurrent steps (throughput mode).  "bf16x3": split-bf16 — the fp32 mode's arithmetic everywhere except the large
    GEMMs, which run as three bf16 products (hi.hi + lo.hi + hi.lo, fp32 accumulate) at fp32-grade accuracy.
    Workspaces are sized for the mode in force: set the mode before a pass is allocated, not between its calls."""
    check(lib().t2_set_precision(PRECISION_MODES[mode]))


def get_precision() -> str:
    return {0: "f32", 1: "bf16", 2: "bf16x3"}[lib().t2_get_precision()]


def gemm_counts(reset: bool = False):
    """(exact fp32, converting bf16, bf16-source on single-bf16 operands, bf16-source on split operands): products of the
    GEMM layer since the last reset, by the kernel family they launched."""
    out = (C.c_uint64 * 4)()
    check(lib().t2_gemm_counts(out, int(bool(reset))))
    return tuple(int(v) for v in out)


def set_split_steps(on: bool) -> None:
    """Split-bf16 recurrent LSTM steps of the teacher-forced passes (include/t2amd.h: t2_set_split_steps).  Acts only in
    precision mode "bf16x3"; workspaces are sized per (mode, switch): set it before a DecoderPass is created."""
    check(lib().t2_set_split_steps(int(bool(on))))


def get_split_steps() -> bool:
    return bool(lib().t2_get_split_steps())


def step_counts(reset: bool = False):
    """Per-step LSTM launches of the decoder entry points since the last reset: forward (exact, bf16, split), then
    recurrent-input gradient (exact, bf16, split)."""
    out = (C.c_uint64 * 6)()
    check(lib().t2_step_counts(out, int(bool(reset))))
    return tuple(int(v) for v in out)


def gemm_plan(args: GemmArgs, **opts) -> dict:
    """What the GEMM layer would do with the product `args` in the modes in force (t2_gemm_plan: nothing is launched, no
    device needed; the pointers count for their alignment only).  opts: the fields of t2_gemm_plan_opts.  Operand sources:
    0 fp32 operand, 1 copy staged into the scratch, 2 the caller's copy."""
    o, info = GemmPlanOpts(**opts), GemmPlanInfo()
    check(lib().t2_gemm_plan(C.byref(args), C.byref(o), C.byref(info)))
    return dict(kernel=info.kernel, name=info.name.decode(), split=bool(info.split), splitk=info.splitk, kchunks=info.kchunks,
                a_src=info.a_src, b_src=info.b_src, stage_bytes_a=info.stage_bytes_a, stage_bytes_b=info.stage_bytes_b)


def chain_plan(kind: str, backward: bool = False, *, cus: int = 256, claimed: bool = True, no_resident: bool = False, **shape) -> dict:
    """What a pass would do with a persistent chain (t2_chain_plan: nothing is launched, no device needed, no claim taken).
    kind: 'lstm', 'sma', 'lsa' or 'enc'; shape: the fields of t2_chain_shape (defaults: the decoder's fixed sizes, two
    streams).  Returns covered and, for a refusal, reason / reason_text; for a covered plan the instance, tiling, LDS
    residency, grid, dynamic LDS bytes and parts = {name: (offset, bytes)} of the exchange space."""
    z = dict(dec=0, NS=2, H=1024, E=512, A=128, P=256, M=80, Hd=1024, F=32, Kc=31, Tin=(100, 60), saved_tiles=1, ws_floats=0)
    z.update(shape)
    z["Tin"] = (C.c_int * 2)(*z["Tin"])
    info = ChainPlanInfo()
    check(lib().t2_chain_plan(C.byref(ChainShape(kind=CHAIN_KINDS[kind], **z)), int(bool(backward)), cus, int(claimed), int(no_resident), C.byref(info)))
    if not info.covered:
        return dict(covered=False, reason=info.reason, reason_text=info.reason_text.decode())
    out = {n: getattr(info, n) for n in ("instance", "grid", "lds_bytes", "UT", "RT", "CS", "MT", "lds_Tc", "lds_Tin", "lds_Jp", "lds_Jm",
                                         "q_bytes", "total_bytes", "ws_bytes")}
    out.update(covered=True, reason=0, instance_name=info.instance_name.decode(), Jp=list(info.Jp), Jm=list(info.Jm),
               parts={info.part_name[i].decode(): (info.part_off[i], info.part_bytes[i]) for i in range(CHAIN_PARTS) if info.part_bytes[i]},
               clear=(info.clear_off, info.clear_bytes), pass_clear_bytes=list(info.pass_clear_bytes))
    return out


def decoder_pass_plan(dims: Dims, kind: str, B: int, T: int, Tin: int, Tsub: int, *, defer_weight_grads: bool = False, poll_every: int = 0,
                      precision: str = "f32", split_steps: bool = False, chain: bool = True, chain_bwd: bool = True, overlap: bool = True,
                      cus: int = 256, claimed: bool = True, no_resident: bool = False, saved_tiles: bool = False, dg_handoff: bool = True, gemm_staging: bool = True) -> dict:
    """What a decoder pass would do (t2_decoder_pass_plan: nothing is launched, no device needed, no claim taken).  kind:
    'forward', 'backward' or 'infer' (T = max_steps); the keyword arguments after poll_every are the environment, all of
    it explicit: the modes and switches in force are NOT read.  Returns every decision of the pass: the layouts, use16 /
    split, the chains (asked, on, reason_text, instance_name), overlap and the step-range bounds, the GEMM scratch as
    parts {name: (offset, bytes)}, and for the backward the tail's carve, where the decoder-LSTM weight gradients go and
    what the tail folds (include/t2amd.h has the fields)."""
    env = PassEnv(PRECISION_MODES[precision], int(split_steps), int(chain), int(chain_bwd), int(overlap), cus, int(claimed), int(no_resident),
                  int(saved_tiles), int(dg_handoff), int(gemm_staging))
    info = DecoderPassPlanInfo()
    check(lib().t2_decoder_pass_plan(C.byref(dims), PASS_KINDS[kind], B, T, Tin, Tsub, C.byref(env), int(defer_weight_grads), poll_every, C.byref(info)))

    def chain_of(c):
        out = dict(asked=bool(c.asked), on=bool(c.on), reason=c.reason, reason_text=c.reason_text.decode())
        if c.on:
            out.update(instance=c.instance, instance_name=c.instance_name.decode(), grid=c.grid)
        return out

    def carve_of(c):
        return dict(w_ih16=(c.w_ih16_off, c.w_ih16_bytes), dg16=(c.dg16_off, c.dg16_bytes), rest=(c.rest_off, c.rest_bytes), total=c.total_bytes)

    out = dict(kind=kind, layout=info.layout, use16=bool(info.use16), split=bool(info.split), pre16=bool(info.pre16), scratch=carve_of(info.scratch),
               chain_a=chain_of(info.chain_a), chain_b=chain_of(info.chain_b), chained=bool(info.chained), overlap=bool(info.overlap),
               bounds=list(info.bounds[:info.nbounds]))
    if kind == "backward":
        out.update(bwd_layout=info.bwd_layout, defer=bool(info.defer), share=bool(info.share), chunk_cast=bool(info.chunk_cast),
                   ddin_ws=(info.ddin_ws_off, info.ddin_ws_bytes), dec_wgrads=("chain_b", "tail")[info.dec_wgrads],
                   dec_wgrads_staged=bool(info.dec_wgrads_staged), tail_on_side=bool(info.tail_on_side), tail_share=bool(info.tail_share),
                   tail_scratch=carve_of(info.tail_scratch), nsplit=info.nsplit, lsa_chain=bool(info.lsa_chain), dq_parts=info.dq_parts,
                   dg_rows_d=bool(info.dg_rows_d), dg_rows_a=bool(info.dg_rows_a))
    else:
        out.update(clear=("status", "teacher", "decode")[info.clear], saves_tiles=bool(info.saves_tiles), poison_words=info.poison_words)
    if kind == "infer":
        out.update(poll=info.poll, shadow_floats=info.shadow_floats)
    return out


def conv_handoff_plan(args: GemmArgs, **opts) -> dict:
    """The conv stacks' hand-over rule for the product `args` with the bf16 copies opts offers (t2_conv_handoff_plan): the
    plan as gemm_plan returns it plus taken = whether the copies are handed over."""
    o, info, taken = GemmPlanOpts(**opts), GemmPlanInfo(), C.c_int(0)
    check(lib().t2_conv_handoff_plan(C.byref(args), C.byref(o), C.byref(taken), C.byref(info)))
    return dict(taken=bool(taken.value), kernel=info.kernel, name=info.name.decode(), split=bool(info.split), splitk=info.splitk,
                kchunks=info.kchunks, a_src=info.a_src, b_src=info.b_src, stage_bytes_a=info.stage_bytes_a, stage_bytes_b=info.stage_bytes_b)


def set_gemm_fold(on: bool) -> None:
    """Gate term of dDOUT and the conv weight-gradient layout folded into the products' stores (default) or as passes of
    their own; the same bits either way (include/t2amd.h t2_set_gemm_fold)."""
    check(lib().t2_set_gemm_fold(1 if on else 0))


def set_bn_fuse(on: bool) -> None:
    """Conv + BatchNorm layers finish their column reductions in the consuming kernel's prologue (default) or in stage-2
    launches of their own; the same bits either way (include/t2amd.h t2_set_bn_fuse)."""
    check(lib().t2_set_bn_fuse(1 if on else 0))


def get_bn_fuse() -> bool:
    return bool(lib().t2_get_bn_fuse())


def bn_fuse_counts(reset: bool = False):
    """Conv + BatchNorm layer calls since the last reset: (fused forward, fused backward with d(bias) partials from the dz
    kernel, fused backward with the separate column sum)."""
    out = (C.c_uint64 * 3)()
    check(lib().t2_bn_fuse_counts(out, int(bool(reset))))
    return tuple(int(v) for v in out)


def set_dg_handoff(on: bool) -> None:
    """bf16 mode: the persistent backward chains store dG as bf16 rows and the casts into the shared copies are skipped
    (default), or fp32 rows and the casts; the same bits either way (include/t2amd.h t2_set_dg_handoff)."""
    check(lib().t2_set_dg_handoff(1 if on else 0))


def get_dg_handoff() -> bool:
    return bool(lib().t2_get_dg_handoff())


def dg_handoff_counts(reset: bool = False):
    """Casts of a dG buffer into its shared bf16 copy since the last reset: (skipped: the chain stored the rows, ran)."""
    out = (C.c_uint64 * 2)()
    check(lib().t2_dg_handoff_counts(out, int(bool(reset))))
    return tuple(int(v) for v in out)


def stage_bf16(src: torch.Tensor) -> torch.Tensor:
    """The library's cast of a row-major fp32 matrix into a bf16 operand (t2_stage_bf16): [rows, K] -> [rows, K] bf16."""
    rows, K = src.shape
    out = torch.empty(rows, K, dtype=torch.bfloat16, device=src.device)
    check(lib().t2_stage_bf16(ptr(src), src.stride(0), ptr(out), rows, K, stream()))
    return out


def defer_counts(reset: bool = False):
    """Decoder backward passes since the last reset: (weight-gradient tail left on the library's side stream, everything
    finished on the caller's stream) (include/t2amd.h t2_defer_counts)."""
    out = (C.c_uint64 * 2)()
    check(lib().t2_defer_counts(out, int(bool(reset))))
    return tuple(int(v) for v in out)


def set_gemm_split_min_mflop(mflop: int = -1) -> None:
    """"bf16x3": products below 2*M*N*K = mflop * 1e6 stay on the exact fp32 kernel (include/t2amd.h); -1 = the default."""
    check(lib().t2_set_gemm_split_min_mflop(int(mflop)))


def softdtw_plan(B: int, N: int, M: int, gamma: float = 1.0, need_grad: bool = False) -> SoftDtwPlanInfo:
    """The partition and scratch sizes of a soft-DTW batch (t2_softdtw_plan: nothing is launched, no device needed);
    raises for sizes over the limit and for gamma <= 0."""
    info = SoftDtwPlanInfo()
    check(lib().t2_softdtw_plan(B, N, M, gamma, int(bool(need_grad)), C.byref(info)))
    return info


def ssim_plan(N: int, H: int, W: int, ws: int = 11, need_grad: int = 0) -> SsimPlanInfo:
    """The tiling and scratch sizes of an SSIM call on N planes of H x W (t2_ssim_plan: nothing is launched, no device
    needed).  need_grad: 0 none, 1 dx, 2 dy, 3 both.  Raises for an even or too wide window and for sizes out of range."""
    info = SsimPlanInfo()
    check(lib().t2_ssim_plan(N, H, W, ws, int(need_grad), C.byref(info)))
    return info


def ssim_image(t: torch.Tensor | None) -> SsimImage:
    """A [B,C,H,W] fp32 device tensor as t2_ssim_image: its pointer and strides as they are (no copy); None -> NULL.
    The planes must be evenly spaced (B and C collapse to one plane axis)."""
    if t is None:
        return SsimImage(None, 0, 0, 0)
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4:
        raise RuntimeError("t2amd: an SSIM image must be a 4-D fp32 tensor on the GPU")
    B, Cn = t.shape[0], t.shape[1]
    sb, sc, sh, sw = t.stride()
    if B > 1 and Cn > 1 and sb != Cn * sc:
        raise RuntimeError("t2amd: SSIM image planes must be evenly spaced over batch and channel")
    return SsimImage(t.data_ptr(), sc if Cn > 1 else sb, sh, sw)


def ssim_forward(args: SsimFwdArgs) -> None:
    check(lib().t2_ssim_forward(C.byref(args), stream()))


def ssim_backward(args: SsimBwdArgs) -> None:
    check(lib().t2_ssim_backward(C.byref(args), stream()))


def bert_config(cfg) -> BertConfig:
    """t2_bert_config from a transformers BertConfig or a dict with its field names."""
    g = (lambda k, d=None: cfg.get(k, d)) if isinstance(cfg, dict) else (lambda k, d=None: getattr(cfg, k, d))
    return BertConfig(int(g("hidden_size")), int(g("num_hidden_layers")), int(g("num_attention_heads")), int(g("intermediate_size")),
                      int(g("vocab_size")), int(g("max_position_embeddings")), int(g("type_vocab_size", 2)), float(g("layer_norm_eps", 1e-12)))


def bert_plan(cfg: BertConfig, B: int, total_tokens: int, max_len: int, cls_only: bool = True) -> BertPlanInfo:
    """Packed-weight floats, workspace bytes and launch count of an encoder call (t2_bert_plan: pure host, no device needed);
    raises with the library's message for a configuration or a batch it refuses."""
    info = BertPlanInfo()
    check(lib().t2_bert_plan(C.byref(cfg), B, total_tokens, max_len, int(cls_only), C.byref(info)))
    return info


def hifigan_config(h) -> HifiganConfig:
    """The C-side configuration from the reference's ``h`` (attribute or key access on the fields Generator reads).
    Raises for what the struct cannot hold; everything else is for t2_hifigan_plan to judge."""
    g = (lambda k: h[k]) if isinstance(h, dict) else (lambda k: getattr(h, k))
    rates, ukernels = list(g("upsample_rates")), list(g("upsample_kernel_sizes"))
    rkernels, rdil = list(g("resblock_kernel_sizes")), [list(d) for d in g("resblock_dilation_sizes")]
    kind = str(g("resblock"))
    if not kind.lstrip("-").isdigit():
        raise RuntimeError(f"hifigan: resblock \"{kind}\" is not \"1\" or \"2\"")
    if len(rates) != len(ukernels) or len(rkernels) != len(rdil):
        raise RuntimeError("hifigan: upsample_rates / upsample_kernel_sizes and resblock_kernel_sizes / resblock_dilation_sizes must pair up")
    if len(rates) > 6 or len(rkernels) > 6:
        raise RuntimeError(f"hifigan: {len(rates)} upsampling stages / {len(rkernels)} resblock kernels, at most 6 each")
    nd = len(rdil[0]) if rdil else 0
    if any(len(d) != nd for d in rdil) or nd > 3:
        raise RuntimeError(f"hifigan: resblock_dilation_sizes={rdil} must hold equally many (at most 3) dilations per kernel")
    c = HifiganConfig()
    c.resblock, c.n_mel, c.upsample_initial_channel = int(kind), 80, int(g("upsample_initial_channel"))
    c.num_upsamples, c.num_kernels, c.num_dilations = len(rates), len(rkernels), nd
    for i, (u, k) in enumerate(zip(rates, ukernels)):
        c.upsample_rates[i], c.upsample_kernel_sizes[i] = int(u), int(k)
    for j, (k, ds) in enumerate(zip(rkernels, rdil)):
        c.resblock_kernel_sizes[j] = int(k)
        for m, d in enumerate(ds):
            c.resblock_dilation_sizes[j][m] = int(d)
    return c


def hifigan_plan(cfg: HifiganConfig, B: int, T: int) -> HifiganPlanInfo:
    """Output length and buffer sizes of a generator call (t2_hifigan_plan: pure host, no device needed); raises with the
    library's message for a configuration it refuses."""
    info = HifiganPlanInfo()
    check(lib().t2_hifigan_plan(C.byref(cfg), B, T, C.byref(info)))
    return info


def hifigan_train_plan(cfg: HifiganConfig, B: int, T: int) -> HifiganTrainPlanInfo:
    """Tape, scratch and launch counts of a training step of the generator (t2_hifigan_train_plan: pure host, no device needed)."""
    info = HifiganTrainPlanInfo()
    check(lib().t2_hifigan_train_plan(C.byref(cfg), B, T, C.byref(info)))
    return info


def hifigan_mpd_plan(period: int, B: int, T: int) -> HifiganMpdPlanInfo:
    """Shapes, tiles, scratch and launch counts of one period discriminator over B items of T samples (t2_hifigan_mpd_plan: pure
    host, no device needed); raises with the library's message for a T too short for the reflect padding."""
    info = HifiganMpdPlanInfo()
    check(lib().t2_hifigan_mpd_plan(period, B, T, C.byref(info)))
    return info


def hifigan_grad_offsets(cfg: HifiganConfig, n_layers: int):
    """(offsets of dw, offsets of db) per layer in the gradient arena of t2_hifigan_backward, in floats."""
    w, b = (C.c_size_t * n_layers)(), (C.c_size_t * n_layers)()
    check(lib().t2_hifigan_grad_offsets(C.byref(cfg), w, b, n_layers))
    return list(w), list(b)


def stft_plan(N: int, hop: int, nf: int = 1) -> StftPlanInfo:
    """Tile sizes, packed-table sizes and the synthesis output length (t2_stft_plan: pure host, no device needed); raises with
    the reason for odd N, N % hop != 0 and sizes the kernels do not take."""
    info = StftPlanInfo()
    check(lib().t2_stft_plan(N, hop, nf, C.byref(info)))
    return info


def melspec_plan(N: int, hop: int, pad: int, n_mels: int, n: int, B: int = 1) -> MelspecPlanInfo:
    """Bins, passes, frames of a full row, the splits the launch takes and the table and scratch sizes (t2_melspec_plan: pure
    host, no device needed); raises with the name and value of what the kernel does not take."""
    info = MelspecPlanInfo()
    check(lib().t2_melspec_plan(N, hop, pad, n_mels, n, B, C.byref(info)))
    return info


def melspec_grad_plan(N: int, hop: int, pad: int, n_mels: int, n: int, B: int = 1) -> MelspecGradPlanInfo:
    """Table and workspace sizes and the grids of the log-mel backward (t2_melspec_grad_plan: pure host, no device needed);
    raises with the name and value of what the backward does not take (hop not dividing N, N / hop > 64)."""
    info = MelspecGradPlanInfo()
    check(lib().t2_melspec_grad_plan(N, hop, pad, n_mels, n, B, C.byref(info)))
    return info


def silence_plan(sample_rate: int, chunk_ms: int, threshold_db: float, n: int, B: int = 1) -> SilencePlanInfo:
    """The threshold as an integer rms, the chunk count and output width of a full row, the scratch size and the launch shapes
    of a silence trim (t2_silence_plan: pure host arithmetic, no device needed)."""
    info = SilencePlanInfo()
    check(lib().t2_silence_plan(sample_rate, chunk_ms, threshold_db, n, B, C.byref(info)))
    return info


def waveglow_config(n_mel_channels, n_flows, n_group, n_early_every, n_early_size, WN_config) -> WaveglowConfig:
    """The constructor arguments of the reference's WaveGlow as the C struct; t2_waveglow_plan judges them."""
    return WaveglowConfig(int(n_mel_channels), int(n_flows), int(n_group), int(n_early_every), int(n_early_size),
                          int(WN_config["n_layers"]), int(WN_config["n_channels"]), int(WN_config["kernel_size"]))


def waveglow_plan(cfg: WaveglowConfig, B: int, T: int) -> WaveglowPlanInfo:
    """Output length, noise planes and buffer sizes of an infer call (t2_waveglow_plan: pure host, no device needed); raises with
    the library's message for what is not supported."""
    info = WaveglowPlanInfo()
    check(lib().t2_waveglow_plan(C.byref(cfg), B, T, C.byref(info)))
    return info


def waveglow_forward_plan(cfg: WaveglowConfig, B: int, T: int, n_samples: int) -> WaveglowForwardInfo:
    """Columns, log_s rows and buffer sizes of an analyze / nll call (t2_waveglow_forward_plan: pure host, no device needed);
    raises with the library's message for what is refused."""
    info = WaveglowForwardInfo()
    check(lib().t2_waveglow_forward_plan(C.byref(cfg), B, T, n_samples, C.byref(info)))
    return info


def waveglow_backward_plan(cfg: WaveglowConfig, B: int, T: int, n_samples: int) -> WaveglowBackwardInfo:
    """Buffer sizes of a training step (t2_waveglow_backward_plan: pure host, no device needed); raises with the library's message
    for what t2_waveglow_forward_plan refuses."""
    info = WaveglowBackwardInfo()
    check(lib().t2_waveglow_backward_plan(C.byref(cfg), B, T, n_samples, C.byref(info)))
    return info


def waveglow_grad_offsets(cfg: WaveglowConfig, n_tensors: int):
    """Offset in floats of every folded tensor's gradient inside the arena of t2_waveglow_backward, in t2_waveglow_pack's order."""
    out = (C.c_size_t * n_tensors)()
    check(lib().t2_waveglow_grad_offsets(C.byref(cfg), out, n_tensors))
    return list(out)
