"""ctypes loader for libblazr_hip.so (the C-ABI in include/blazr_hip.h).

The product path has NO fallback: if the shared library is missing or a compute call is made without a
gfx950 device, it raises.  Nothing here imports oracle/.
"""
import atexit
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BZ_LIB_PATH") or os.path.join(_HERE, "libblazr_hip.so")   # BZ_LIB_PATH: A/B builds of the library (tuning only)
_LIB = None
alive = True   # cleared at interpreter exit: handle destructors must not call into a torn-down HIP runtime


def _at_exit():
    global alive
    alive = False


atexit.register(_at_exit)

OK, E_INVALID, E_NODEVICE, E_HIP, E_UNSUPPORTED, E_NOTFOUND, E_OOM = 0, -1, -2, -3, -4, -5, -6
F32, F16, BF16, I64, I32, U32, U8 = range(7)
ABI_VERSION = 4
FWD_ALL_LOGITS = 1
GRAMMAR_REGULAR = 1
GRAMMAR_LDS_MAX_STATES = 128
GRAMMAR_ROW_FREE = 0xFFFFFFFF
ROPE_NONE, ROPE_LINEAR, ROPE_LLAMA3, ROPE_YARN = 0, 1, 2, 3
ARCH_LLAMA = 0
ARCH_MAMBA2 = 1
ARCH_DEEPSEEK2 = 2


class BlazrHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libblazr_hip error %d: %s" % (code, msg))
        self.code = code


class ModelConfig(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("arch", C.c_int32), ("hidden", C.c_int32), ("n_layers", C.c_int32),
                ("n_heads", C.c_int32), ("n_kv_heads", C.c_int32), ("head_dim", C.c_int32), ("inter", C.c_int32),
                ("vocab", C.c_int32), ("max_seq_len", C.c_int32), ("rms_eps", C.c_float), ("act_dtype", C.c_int32),
                ("tie_embeddings", C.c_int32), ("rope_theta", C.c_float), ("rope_interleaved", C.c_int32),
                ("rope_scaling", C.c_int32), ("rope_factor", C.c_float), ("rope_low_freq_factor", C.c_float),
                ("rope_high_freq_factor", C.c_float), ("rope_original_max_pos", C.c_int32),
                ("ssm_d_inner", C.c_int32), ("ssm_n_heads", C.c_int32), ("ssm_head_dim", C.c_int32), ("ssm_d_state", C.c_int32),
                ("ssm_n_groups", C.c_int32), ("ssm_conv_kernel", C.c_int32),
                ("mla_kv_lora_rank", C.c_int32), ("mla_q_lora_rank", C.c_int32), ("mla_nope_dim", C.c_int32), ("mla_rope_dim", C.c_int32),
                ("mla_v_dim", C.c_int32), ("moe_n_experts", C.c_int32), ("moe_top_k", C.c_int32), ("moe_n_shared", C.c_int32),
                ("moe_inter", C.c_int32), ("moe_first_dense", C.c_int32), ("moe_norm_topk", C.c_int32), ("moe_routed_scale", C.c_float),
                ("rope_beta_fast", C.c_float), ("rope_beta_slow", C.c_float), ("rope_attn_factor", C.c_float), ("mla_softmax_mscale", C.c_float),
                ("sliding_window", C.c_int32), ("sliding_window_pattern", C.c_int32),   # took two of the four reserved slots: 0 = full attention
                ("reserved", C.c_int32 * 2)]


class GenConfig(C.Structure):
    _fields_ = [("max_tokens", C.c_int32), ("temperature", C.c_float), ("repeat_penalty", C.c_float),
                ("repeat_last_n", C.c_int32), ("frequency_penalty", C.c_float), ("presence_penalty", C.c_float),
                ("top_k", C.c_int32), ("top_p", C.c_float), ("min_p", C.c_float), ("seed", C.c_uint64),
                ("eos_id", C.c_int64), ("use_graph", C.c_int32), ("paged", C.c_int32), ("block_size", C.c_int32),
                ("dry_multiplier", C.c_float), ("dry_base", C.c_int32), ("dry_allowed_length", C.c_int32), ("typical_p", C.c_float),
                ("dynatemp_range", C.c_float), ("dynatemp_exponent", C.c_float), ("mirostat_mode", C.c_int32), ("mirostat_tau", C.c_float),
                ("mirostat_eta", C.c_float), ("n_logit_bias", C.c_int32), ("logit_bias_ids", C.c_void_p), ("logit_bias_vals", C.c_void_p),
                ("reserved", C.c_int32 * 4)]


class ModelSource(C.Structure):
    _fields_ = [("format", C.c_int32), ("has_config", C.c_int32), ("weights_path", C.c_char * 1024), ("config_path", C.c_char * 1024)]


class DetectedArch(C.Structure):
    _fields_ = [("format", C.c_int32), ("num_layers", C.c_int32), ("tie_word_embeddings", C.c_int32), ("layer_types", C.c_uint8 * 512)]


class QuantInfo(C.Structure):
    _fields_ = [("quant_method", C.c_int32), ("group_size", C.c_int32), ("torch_dtype", C.c_int32)]


class GgufInfo(C.Structure):
    _fields_ = [("architecture", C.c_char * 64), ("n_tensors", C.c_int32), ("version", C.c_int32), ("dominant_ggml_type", C.c_int32),
                ("is_mla", C.c_int32), ("is_moe", C.c_int32), ("is_ssm", C.c_int32), ("file_size_bytes", C.c_uint64)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int32), ("total_ms", C.c_double), ("algo_bytes", C.c_double)]


class GenStats(C.Structure):
    _fields_ = [("prefill_ms", C.c_double), ("decode_ms", C.c_double), ("n_generated", C.c_int32),
                ("finish_reason", C.c_int32), ("ttft_ms", C.c_double), ("total_ms", C.c_double), ("itl_p50_ms", C.c_double),
                ("itl_p99_ms", C.c_double), ("itl_max_ms", C.c_double), ("decode_tok_per_s", C.c_double)]


class SpecConfig(C.Structure):
    _fields_ = [("num_speculative_tokens", C.c_int32), ("adaptive_depth", C.c_int32), ("reserved", C.c_int32 * 6)]


class SpecStats(C.Structure):
    _fields_ = [("iterations", C.c_int64), ("drafted_tokens", C.c_int64), ("accepted_tokens", C.c_int64), ("rejected_tokens", C.c_int64),
                ("verify_path", C.c_int32), ("final_depth", C.c_int32), ("draft_ms", C.c_double), ("verify_ms", C.c_double)]


SAMPLER_WINDOW_MAX = 256


class RowSampling(C.Structure):
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("min_p", C.c_float), ("repeat_penalty", C.c_float),
                ("frequency_penalty", C.c_float), ("presence_penalty", C.c_float), ("repeat_last_n", C.c_int32), ("seed", C.c_uint64),
                ("reserved", C.c_int32 * 4)]


ENGINE_MAX_STOP = 8
SCHED_ADMIT, SCHED_PREFILL, SCHED_LIVE, SCHED_COPY = 0, 1, 2, 3


class SchedAction(C.Structure):
    _fields_ = [("kind", C.c_int32), ("row", C.c_int32), ("id", C.c_int64), ("a", C.c_int32), ("b", C.c_int32)]


class SchedInfo(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("num_blocks", C.c_int32), ("park_blocks", C.c_int32), ("free_blocks", C.c_int32), ("owned_blocks", C.c_int32),
                ("waiting", C.c_int32), ("admitted", C.c_int32), ("live", C.c_int32)]


class SchedPrefixInfo(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("cached_blocks", C.c_int32), ("evictable_blocks", C.c_int32), ("referenced_blocks", C.c_int32),
                ("hits", C.c_int64), ("misses", C.c_int64), ("cached_tokens", C.c_int64), ("evictions", C.c_int64)]


class EnginePrefixStats(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("cached_blocks", C.c_int32), ("evictable_blocks", C.c_int32), ("referenced_blocks", C.c_int32),
                ("private_blocks", C.c_int32), ("reserved", C.c_int32), ("hits", C.c_int64), ("misses", C.c_int64), ("cached_tokens", C.c_int64),
                ("evictions", C.c_int64), ("prompt_tokens_skipped", C.c_int64), ("copy_launches", C.c_int64), ("copied_blocks", C.c_int64)]


class EngineConfig(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("num_blocks", C.c_int32), ("block_size", C.c_int32), ("max_seq_len", C.c_int32), ("prefill_chunk", C.c_int32),
                ("depth", C.c_int32), ("use_sampler", C.c_int32), ("prefix_cache", C.c_int32), ("logprobs", C.c_int32), ("reserved", C.c_int32 * 7)]


class Request(C.Structure):
    _fields_ = [("max_tokens", C.c_int32), ("n_stop", C.c_int32), ("stop_ids", C.c_int64 * 8), ("grammar_state", C.c_uint32), ("lora_slot", C.c_int32), ("reserved", C.c_int32 * 2),
                ("sampling", RowSampling)]


LOGIT_BIAS_MAX, TOP_LOGPROBS_MAX = 512, 20
BS_BIAS, BS_LOGPROBS = 1, 2


class LogprobsRecord(C.Structure):
    _fields_ = [("token", C.c_int64), ("logprob", C.c_float), ("lse", C.c_float), ("n_top", C.c_int32), ("top_ids", C.c_uint32 * TOP_LOGPROBS_MAX),
                ("top_logprobs", C.c_float * TOP_LOGPROBS_MAX)]


class ScoreConfig(C.Structure):
    _fields_ = [("top_n", C.c_int32), ("reserved", C.c_int32 * 7)]


class ScoreRow(C.Structure):
    _fields_ = [("target", C.c_int64), ("logit", C.c_float), ("logprob", C.c_float), ("lse", C.c_float), ("rank", C.c_int32), ("n_top", C.c_int32),
                ("top_ids", C.c_uint32 * TOP_LOGPROBS_MAX), ("top_logprobs", C.c_float * TOP_LOGPROBS_MAX)]


class ScoreTotal(C.Structure):
    _fields_ = [("sum_logprob", C.c_double), ("n_scored", C.c_int64)]


POOL_NONE, POOL_MEAN, POOL_CLS, POOL_LAST = 0, 1, 2, 3
POOLINGS = {"none": POOL_NONE, "mean": POOL_MEAN, "cls": POOL_CLS, "last": POOL_LAST}


class EmbedConfig(C.Structure):
    _fields_ = [("pooling", C.c_int32), ("normalize", C.c_int32), ("reserved", C.c_int32 * 6)]


class RequestExtras(C.Structure):
    _fields_ = [("logprobs", C.c_int32), ("top_logprobs", C.c_int32), ("n_logit_bias", C.c_int32), ("logit_bias_ids", C.c_void_p), ("logit_bias_vals", C.c_void_p),
                ("reserved", C.c_int32 * 4)]


class EngineLogprobs(C.Structure):
    _fields_ = [("id", C.c_int64), ("index", C.c_int32), ("token", C.c_int64), ("logprob", C.c_float), ("n_top", C.c_int32),
                ("top_ids", C.c_uint32 * TOP_LOGPROBS_MAX), ("top_logprobs", C.c_float * TOP_LOGPROBS_MAX)]


LORA_TARGETS = {"q": 1, "k": 2, "v": 4, "o": 8, "gate": 16, "up": 32, "down": 64}
LORA_ALL = 127


class LoraTableConfig(C.Structure):
    _fields_ = [("n_slots", C.c_int32), ("max_rank", C.c_int32), ("targets", C.c_uint32), ("reserved", C.c_int32 * 5)]


class EngineEvent(C.Structure):
    _fields_ = [("id", C.c_int64), ("token", C.c_int64), ("index", C.c_int32), ("finish_reason", C.c_int32), ("replay", C.c_int64)]


class RowsAttnPlan(C.Structure):
    _fields_ = [("kernel", C.c_int), ("scalar_limit", C.c_int), ("grid_slices", C.c_int), ("rows_per_pass", C.c_int), ("ws_bytes", C.c_size_t)]


class PromptTraits(C.Structure):
    _fields_ = ([(n, C.c_int) for n in ("arch", "act_dtype", "hidden", "inter", "n_layers", "n_heads", "n_kv_heads", "head_dim", "rep", "sliding_window",
                                        "sliding_window_pattern", "shapes_ok", "proj_16", "any_dense", "exact_cap", "gq_all", "gq_max_k")] +
                [("gq_max_n3k", C.c_ulonglong)] +
                [(n, C.c_int) for n in ("head_rows", "head_gemm", "spec_head", "mla_q_lora_rank", "mla_kv_lora_rank", "mla_rope_dim", "mla_nope_dim", "mla_v_dim",
                                        "ds_dims_ok", "ds_weights_act", "ssm_scan_ok", "ssm_groups_ok", "ssm_proj_ok")])


class PromptSwitches(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("prefill_min", "no_mfma_prefill", "no_gguf_prefill", "exact", "exact_max", "exact_i8_max")]


class PromptPlan(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("route", "exact", "attn", "head", "chunk")]


class PackedPlan(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("packed", "rows", "n_seq", "max_len")] + [("plan", PromptPlan)]


PLAN_PROMPT, PLAN_DECODE_BATCH, PLAN_VERIFY = 0, 1, 2
ROUTE_STEPS, ROUTE_ROWS, ROUTE_DSV2, ROUTE_MAMBA = 0, 1, 2, 3
PF_ATTN_NONE, PF_ATTN_MFMA, PF_ATTN_SCALAR, PF_ATTN_SCALAR_EXACT, PF_ATTN_ROWS = 0, 1, 2, 3, 4
HEAD_STEP, HEAD_GEMM, HEAD_GEMV_ROWS, HEAD_SPEC = 0, 1, 2, 3


# which kernels a decode step launches (bz_layer_plan)
class LinearTraits(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("kind", "N", "K", "wdt", "gw", "sk", "npf", "act_order", "bias")]


class FusedTraits(C.Structure):
    _fields_ = [("n_parts", C.c_int), ("fix_out", C.c_int), ("parts", LinearTraits * 3)]


class LayerTraits(C.Structure):
    _fields_ = ([(n, C.c_int) for n in ("arch", "act_dtype", "hidden", "inter", "n_heads", "n_kv_heads", "head_dim", "window", "lora_o", "lora_mlp", "down_slabs")] +
                [(n, FusedTraits) for n in ("qkv", "o", "gateup", "down")] + [("mla_x_ok", C.c_int * 3)] +
                [(n, C.c_int) for n in ("is_moe", "e_dt", "router_dt", "moe_inter", "moe_n_experts", "moe_slots", "ssm_d_inner", "ssm_n_groups")])


class StepSwitches(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("no_slim_qkv", "no_gq_slim", "no_gq_mix", "no_rows2", "no_attn_fusion", "no_attn_split", "no_attn_f32", "no_attn2_hd64",
                                       "no_mlp_fusion", "gguf_mlp_fusion", "dsv2_f32_sums", "no_moe_route_fusion")]


class LayerPlan(C.Structure):
    _fields_ = [("qkv_mix", C.c_int), ("qkv", C.c_int * 3), ("attn_short", C.c_int), ("attn_long", C.c_int), ("attn_kernel", C.c_int), ("o", C.c_int * 3),
                ("mlp", C.c_int), ("gateup_mix", C.c_int), ("gateup", C.c_int * 3), ("down", C.c_int * 3),
                ("mla_exact", C.c_int), ("moe_route_fused", C.c_int), ("moe_rows2", C.c_int)]


(LIN_NONE, LIN_Q4G, LIN_ROWS, LIN_Q4K, LIN_Q6K, LIN_Q80, LIN_Q5K, LIN_Q40, LIN_Q41, LIN_Q50, LIN_Q51, LIN_F8, LIN_MX4) = range(13)
(GEMV_NONE, GEMV_F8, GEMV_Q4G_SLIM, GEMV_Q4G, GEMV_ROWS2, GEMV_ROWS, GEMV_GQ_SLIM, GEMV_GQ, GEMV_UNSUPPORTED, GEMV_MX4) = range(10)
ATTN_PLAIN, ATTN_FUSED_Q4G, ATTN_FUSED_DENSE, ATTN_FUSED_Q4K, ATTN_SPLIT, ATTN_SPLIT_FUSED = range(6)
ATTN_K_DECODE, ATTN_K_ATTN2, ATTN_K_ATTN2F, ATTN_K_UNSUPPORTED = range(4)
MLP_SPLIT, MLP_Q4G, MLP_DENSE, MLP_GQ = range(4)


class EngineStats(C.Structure):
    _fields_ = [("replays", C.c_int64), ("free_blocks", C.c_int32), ("total_blocks", C.c_int32), ("park_blocks", C.c_int32), ("live_rows", C.c_int32),
                ("admitted", C.c_int32), ("waiting", C.c_int32), ("unread", C.c_int32), ("prompt_tokens", C.c_int64), ("generated_tokens", C.c_int64),
                ("admit_host_ms", C.c_double)]


# name -> (restype, argtypes); every symbol include/blazr_hip.h declares
P = C.c_void_p
SYMBOLS = {
    "bz_last_error": (C.c_char_p, []),
    "bz_abi_version": (C.c_int, []),
    "bz_device_open": (C.c_int, [C.c_int, C.POINTER(P)]),
    "bz_device_close": (C.c_int, [P]),
    "bz_device_synchronize": (C.c_int, [P]),
    "bz_device_memory_info": (C.c_int, [P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "bz_device_name": (C.c_int, [P, C.c_char_p, C.c_size_t]),
    "bz_device_stream": (P, [P]),
    "bz_tensor_from_host": (C.c_int, [P, C.c_int, C.POINTER(C.c_int64), C.c_int, P, C.POINTER(P)]),
    "bz_tensor_zeros": (C.c_int, [P, C.c_int, C.POINTER(C.c_int64), C.c_int, C.POINTER(P)]),
    "bz_tensor_free": (C.c_int, [P]),
    "bz_tensor_to_host": (C.c_int, [P, P, C.c_size_t]),
    "bz_tensor_nbytes": (C.c_int, [P, C.POINTER(C.c_size_t)]),
    "bz_tensor_copy_from_host": (C.c_int, [P, P, C.c_size_t]),
    "bz_event_record": (C.c_int, [P, C.POINTER(C.c_uint64)]),
    "bz_event_sync": (C.c_int, [P, C.c_uint64]),
    "bz_tensor_to_host_pipelined": (C.c_int, [P, C.c_uint64, P, C.c_size_t]),
    "bz_model_create": (C.c_int, [P, C.POINTER(ModelConfig), C.POINTER(P)]),
    "bz_model_free": (C.c_int, [P]),
    "bz_model_add_dense": (C.c_int, [P, C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.c_int, P]),
    "bz_model_add_awq": (C.c_int, [P, C.c_char_p, C.c_int64, C.c_int64, P, P, P, C.c_int]),
    "bz_model_add_gptq": (C.c_int, [P, C.c_char_p, C.c_int64, C.c_int64, P, P, P, P, P, C.c_int]),
    "bz_model_add_gguf": (C.c_int, [P, C.c_char_p, C.c_int, C.c_int64, C.c_int64, P]),
    "bz_model_add_fp8": (C.c_int, [P, C.c_char_p, C.c_int64, C.c_int64, P, P, C.c_int64, P]),
    "bz_model_add_mxfp4": (C.c_int, [P, C.c_char_p, C.c_int64, C.c_int64, P, P, P]),
    "bz_model_finalize": (C.c_int, [P]),
    "bz_model_get_config": (C.c_int, [P, C.POINTER(ModelConfig)]),
    "bz_model_weight_bytes": (C.c_int, [P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "bz_kv_create": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(P)]),
    "bz_kv_free": (C.c_int, [P]),
    "bz_kv_reset": (C.c_int, [P]),
    "bz_kv_seq_len": (C.c_int, [P]),
    "bz_kv_read": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, P]),
    "bz_paged_kv_create": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(P)]),
    "bz_paged_kv_free": (C.c_int, [P]),
    "bz_paged_kv_set_seq_len": (C.c_int, [P, C.c_int]),
    "bz_paged_kv_seq_len": (C.c_int, [P]),
    "bz_paged_kv_copy_slots": (C.c_int, [P, C.c_int, C.c_int, C.c_int]),
    "bz_paged_kv_read_block": (C.c_int, [P, C.c_int, C.c_int, C.c_int, P, C.c_size_t]),
    "bz_paged_kv_write_block": (C.c_int, [P, C.c_int, C.c_int, C.c_int, P, C.c_size_t]),
    "bz_forward_kv": (C.c_int, [P, P, C.c_int, P, C.c_int, P, C.c_uint32]),
    "bz_forward_paged": (C.c_int, [P, P, C.c_int, P, P, P, C.c_int, C.c_int, C.c_int, P, C.c_uint32]),
    "bz_forward_embed": (C.c_int, [P, P, C.c_int, P]),
    "bz_forward_layers_range": (C.c_int, [P, P, P, C.POINTER(C.c_int), C.c_int, P, C.c_int, C.c_int, C.c_int]),
    "bz_forward_head": (C.c_int, [P, P, P, C.c_int, C.c_int, P, C.c_uint32]),
    "bz_logits_to_token": (C.c_int, [P, P, C.c_int64, C.c_int64, P, P, C.c_int, C.c_float, C.c_float, C.c_float,
                                     C.c_float, C.c_int, C.c_float, C.c_float, C.c_uint64, P]),
    "bz_argmax_to_buf": (C.c_int, [P, P, C.c_int64, C.c_int64, P]),
    "bz_decode_graph_capture": (C.c_int, [P, P, C.POINTER(P)]),
    "bz_decode_graph_capture_paged": (C.c_int, [P, P, C.c_int, C.POINTER(P)]),
    "bz_decode_graph_seed": (C.c_int, [P, C.c_int64, C.c_int]),
    "bz_decode_graph_set_block_table": (C.c_int, [P, P, C.c_int]),
    "bz_decode_graph_replay": (C.c_int, [P]),
    "bz_decode_graph_read_token": (C.c_int, [P, C.c_int64, C.POINTER(C.c_int64)]),
    "bz_decode_graph_read_logits": (C.c_int, [P, P, C.c_size_t]),
    "bz_decode_graph_free": (C.c_int, [P]),
    "bz_decode_batch_graph_capture": (C.c_int, [P, P, C.c_int, C.c_int, C.POINTER(P)]),
    "bz_decode_batch_graph_seed": (C.c_int, [P, P, P, P]),
    "bz_decode_batch_graph_set_block_table": (C.c_int, [P, P]),
    "bz_decode_batch_graph_replay": (C.c_int, [P]),
    "bz_decode_batch_graph_read_tokens": (C.c_int, [P, C.c_int64, P]),
    "bz_decode_batch_graph_logits": (C.c_int, [P, C.POINTER(P)]),
    "bz_decode_batch_graph_free": (C.c_int, [P]),
    "bz_batch_sampler_create": (C.c_int, [P, C.c_int, C.c_int64, C.POINTER(P)]),
    "bz_batch_sampler_free": (C.c_int, [P]),
    "bz_batch_sampler_set_row": (C.c_int, [P, C.c_int, C.POINTER(RowSampling), P, C.c_int, C.c_int64]),
    "bz_batch_sampler_sample": (C.c_int, [P, P, P]),
    "bz_decode_batch_graph_capture_sampled": (C.c_int, [P, P, C.c_int, C.c_int, P, C.POINTER(P)]),
    "bz_logit_bias_dedupe": (C.c_int, [C.c_int64, P, P, C.c_int, P, P, C.POINTER(C.c_int)]),
    "bz_batch_sampler_enable": (C.c_int, [P, C.c_uint32]),
    "bz_batch_sampler_set_row_bias": (C.c_int, [P, C.c_int, P, P, C.c_int]),
    "bz_batch_sampler_set_row_logprobs": (C.c_int, [P, C.c_int, C.c_int]),
    "bz_batch_sampler_read_logprobs": (C.c_int, [P, C.POINTER(LogprobsRecord)]),
    "bz_decode_batch_graph_read_logprobs": (C.c_int, [P, C.c_int64, C.POINTER(LogprobsRecord)]),
    "bz_score_kv": (C.c_int, [P, P, C.c_int, P, C.c_int, P, C.POINTER(ScoreConfig), C.POINTER(ScoreRow), C.POINTER(ScoreTotal)]),
    "bz_score_paged": (C.c_int, [P, P, C.c_int, P, P, P, C.c_int, C.c_int, C.c_int, P, C.POINTER(ScoreConfig), C.POINTER(ScoreRow), C.POINTER(ScoreTotal)]),
    "bz_score_ssm": (C.c_int, [P, P, C.c_int, P, P, C.POINTER(ScoreConfig), C.POINTER(ScoreRow), C.POINTER(ScoreTotal)]),
    "bz_embed_kv": (C.c_int, [P, P, C.c_int, P, C.c_int, C.POINTER(EmbedConfig), P]),
    "bz_embed_paged": (C.c_int, [P, P, C.c_int, P, P, P, C.c_int, C.c_int, C.c_int, C.POINTER(EmbedConfig), P]),
    "bz_embed_ssm": (C.c_int, [P, P, C.c_int, P, C.POINTER(EmbedConfig), P]),
    "bz_embed_batch": (C.c_int, [P, P, P, C.c_int, P, C.POINTER(EmbedConfig), P]),
    "bz_score_batch": (C.c_int, [P, P, P, C.c_int, P, P, C.POINTER(ScoreConfig), C.POINTER(ScoreRow), C.POINTER(ScoreTotal)]),
    "bz_attn_packed": (C.c_int, [P, P, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P]),
    "bz_score_rows": (C.c_int, [P, P, C.c_int64, C.c_int64, P, C.POINTER(ScoreConfig), C.POINTER(ScoreRow)]),
    "bz_pool_rows": (C.c_int, [P, P, C.c_int64, C.c_int64, C.POINTER(EmbedConfig), P]),
    "bz_score_row_spec": (C.c_int, [P, C.c_int64, C.c_int64, C.c_int, C.POINTER(ScoreRow)]),
    "bz_pool_spec": (C.c_int, [P, C.c_int64, C.c_int64, C.POINTER(EmbedConfig), P]),
    "bz_generate": (C.c_int, [P, P, C.c_int, C.POINTER(GenConfig), P, C.POINTER(GenStats)]),
    "bz_profile_step": (C.c_int, [P, P, C.c_int64, C.c_int, C.c_int, C.POINTER(KernelTime), C.c_int, C.POINTER(C.c_int)]),
    "bz_profile_step_ssm": (C.c_int, [P, P, C.c_int64, C.c_int, C.POINTER(KernelTime), C.c_int, C.POINTER(C.c_int)]),
    "bz_ssm_state_create": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(P)]),
    "bz_ssm_state_free": (C.c_int, [P]),
    "bz_ssm_state_reset": (C.c_int, [P]),
    "bz_forward_paged_batch": (C.c_int, [P, P, C.c_int, P, P, P, C.c_int, P, P]),
    "bz_forward_ssm": (C.c_int, [P, P, C.c_int, P, P, C.c_uint32]),
    "bz_decode_graph_capture_ssm": (C.c_int, [P, P, C.POINTER(P)]),
    "bz_tune_rows": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "bz_tune_mlp": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "bz_probe_hbm_read": (C.c_int, [P, C.c_size_t, C.c_int, C.POINTER(C.c_double)]),
    "bz_expf_spec": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "bz_fp8_e4m3_spec": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "bz_conv1d_step": (C.c_int, [P, C.c_int, P, P, P]),
    "bz_ssm_step": (C.c_int, [P, C.c_int, P, P, P]),
    "bz_ssm_scan_rows": (C.c_int, [P, C.c_int, P, P, C.c_int, P, P, P]),
    "bz_ssm_state_read": (C.c_int, [P, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "bz_moe_route": (C.c_int, [P, C.c_int, P, P, P, P]),
    "bz_moe_grouped_gemv": (C.c_int, [P, C.c_int, C.c_int, P, C.c_int, P, P]),
    "bz_tune_gemv": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "bz_compute_dynamic_temperature": (C.c_float, [P, C.c_int64, C.c_float, C.c_float, C.c_float]),
    "bz_apply_dry_penalty": (C.c_int, [P, C.c_int64, P, C.c_int64, C.c_float, C.c_int, C.c_int]),
    "bz_apply_typical_filter": (C.c_int, [P, C.c_int64, C.c_float]),
    "bz_apply_logit_bias": (C.c_int, [P, C.c_int64, P, P, C.c_int]),
    "bz_compute_logprobs": (C.c_int, [P, C.c_int64, C.c_uint32, C.c_int, C.POINTER(C.c_float), P, P, C.POINTER(C.c_int)]),
    "bz_mirostat_create": (C.c_int, [C.c_float, C.c_float, C.c_uint64, C.POINTER(P)]),
    "bz_mirostat_sample": (C.c_int, [P, P, C.c_int64, C.c_float, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    "bz_mirostat_mu": (C.c_float, [P]),
    "bz_mirostat_free": (C.c_int, [P]),
    "bz_detect_model_source": (C.c_int, [C.c_char_p, C.POINTER(ModelSource)]),
    "bz_detect_architecture_from_names": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.POINTER(DetectedArch)]),
    "bz_config_from_hf_json": (C.c_int, [C.c_char_p, C.POINTER(ModelConfig), C.POINTER(QuantInfo)]),
    "bz_config_from_gguf": (C.c_int, [C.c_char_p, C.POINTER(ModelConfig), C.POINTER(GgufInfo)]),
    "bz_safetensors_describe": (C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "bz_load_model": (C.c_int, [P, C.c_char_p, C.POINTER(P), C.POINTER(ModelConfig)]),
    "bz_prefill_matmul": (C.c_int, [P, C.c_char_p, P, C.c_int, P]),
    "bz_quant_matmul": (C.c_int, [P, C.c_char_p, P, C.c_int, P]),
    "bz_dequant": (C.c_int, [P, C.c_char_p, P]),
    "bz_rms_norm": (C.c_int, [P, P, P, P, C.c_int, C.c_int, C.c_float, C.c_int, P, P]),
    "bz_rope": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int]),
    "bz_silu_mul": (C.c_int, [P, P, P, C.c_int64, C.c_int, P]),
    "bz_attn_decode": (C.c_int, [P, P, P, C.c_int, C.c_int, P]),
    "bz_paged_attn_decode": (C.c_int, [P, P, P, C.c_int, P, C.c_int, P]),
    "bz_paged_attn_decode_rows": (C.c_int, [P, P, P, C.c_int, P, C.c_int, P, C.c_int, P]),
    "bz_rows_attn_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P]),
    "bz_rows_attn_slice_len": (C.c_int, [C.c_int]),
    "bz_model_prompt_traits": (C.c_int, [P, C.POINTER(PromptTraits)]),
    "bz_prompt_plan": (C.c_int, [C.POINTER(PromptTraits), C.POINTER(PromptSwitches), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PromptPlan)]),
    "bz_packed_plan": (C.c_int, [C.POINTER(PromptTraits), C.POINTER(PromptSwitches), P, C.c_int, C.c_int, C.POINTER(PackedPlan)]),
    "bz_packed_targets_spec": (C.c_int, [P, P, C.c_int, P]),
    "bz_packed_totals_spec": (C.c_int, [P, P, C.c_int, C.POINTER(ScoreTotal)]),
    "bz_model_layer_traits": (C.c_int, [P, C.c_int, C.POINTER(LayerTraits)]),
    "bz_model_layer_plan": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(LayerPlan)]),
    "bz_layer_plan": (C.c_int, [C.POINTER(LayerTraits), C.POINTER(StepSwitches), C.c_int, C.POINTER(LayerPlan)]),
    "bz_step_attn_form": (C.c_int, [C.POINTER(LayerPlan), C.c_int, C.c_int, C.c_int]),
    "bz_kv_insert": (C.c_int, [P, P, C.c_int, C.c_int, P, P]),
    "bz_rope_caches": (C.c_int, [P, P, P]),
    "bz_grammar_compile": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(P)]),
    "bz_grammar_from_table": (C.c_int, [C.c_int, P, P, C.POINTER(P)]),
    "bz_grammar_table": (C.c_int, [P, P, P]),
    "bz_grammar_num_states": (C.c_int, [P]),
    "bz_grammar_current_state": (C.c_int, [P]),
    "bz_grammar_is_accepting": (C.c_int, [P]),
    "bz_grammar_reset": (C.c_int, [P]),
    "bz_grammar_free": (C.c_int, [P]),
    "bz_grammar_advance": (C.c_int, [P, P, C.c_size_t, C.POINTER(C.c_int)]),
    "bz_grammar_token_mask": (C.c_int, [P, P, P, C.c_int64, P]),
    "bz_grammar_to_device": (C.c_int, [P, P, P, P, C.c_int64, C.POINTER(P)]),
    "bz_device_grammar_set_state": (C.c_int, [P, C.c_uint32]),
    "bz_device_grammar_info": (C.c_int, [P, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]),
    "bz_device_grammar_free": (C.c_int, [P]),
    "bz_grammar_dfa_mask_logits": (C.c_int, [P, P, C.c_int64, C.c_int64, P, P]),
    "bz_grammar_concat": (C.c_int, [C.POINTER(P), C.c_int, C.POINTER(P), C.POINTER(C.c_int32)]),
    "bz_grammar_advance_tokens": (C.c_int, [P, P, P, C.c_int64, P, C.c_int64, C.POINTER(C.c_int)]),
    "bz_grammar_cursor_create": (C.c_int, [P, C.c_int, C.POINTER(P)]),
    "bz_grammar_cursor_free": (C.c_int, [P]),
    "bz_grammar_cursor_set_row": (C.c_int, [P, C.c_int, C.c_uint32]),
    "bz_grammar_cursor_read": (C.c_int, [P, P, P]),
    "bz_grammar_cursor_mask": (C.c_int, [P, P]),
    "bz_grammar_cursor_advance": (C.c_int, [P, P]),
    "bz_decode_batch_graph_capture_grammar": (C.c_int, [P, P, C.c_int, C.c_int, P, P, C.POINTER(P)]),
    "bz_decode_graph_capture_grammar": (C.c_int, [P, P, P, C.POINTER(P)]),
    "bz_decode_graph_capture_paged_grammar": (C.c_int, [P, P, C.c_int, P, C.POINTER(P)]),
    "bz_generate_grammar": (C.c_int, [P, P, C.c_int, C.POINTER(GenConfig), P, P, P, C.c_int64, P, C.POINTER(GenStats)]),
    "bz_sched_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(P)]),
    "bz_sched_free": (C.c_int, [P]),
    "bz_sched_submit": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "bz_sched_step": (C.c_int, [P, C.POINTER(SchedAction), C.c_int, C.POINTER(C.c_int)]),
    "bz_sched_finish": (C.c_int, [P, C.c_int64]),
    "bz_sched_info": (C.c_int, [P, C.POINTER(SchedInfo)]),
    "bz_sched_row": (C.c_int, [P, C.c_int, C.POINTER(C.c_int64), P, C.c_int, C.POINTER(C.c_int)]),
    "bz_sched_enable_prefix": (C.c_int, [P]),
    "bz_sched_submit_tokens": (C.c_int, [P, P, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "bz_sched_prefix_info": (C.c_int, [P, C.POINTER(SchedPrefixInfo)]),
    "bz_sched_prefix_flush": (C.c_int, [P, C.POINTER(C.c_int)]),
    "bz_engine_prefix_stats": (C.c_int, [P, C.POINTER(EnginePrefixStats)]),
    "bz_engine_prefix_flush": (C.c_int, [P, C.POINTER(C.c_int)]),
    "bz_engine_create": (C.c_int, [P, C.POINTER(EngineConfig), P, C.POINTER(P)]),
    "bz_engine_submit": (C.c_int, [P, P, C.c_int, C.POINTER(Request), C.POINTER(C.c_int64)]),
    "bz_engine_submit_ex": (C.c_int, [P, P, C.c_int, C.POINTER(Request), C.POINTER(RequestExtras), C.POINTER(C.c_int64)]),
    "bz_engine_poll_logprobs": (C.c_int, [P, C.POINTER(EngineLogprobs), C.c_int, C.POINTER(C.c_int)]),
    "bz_engine_cancel": (C.c_int, [P, C.c_int64]),
    "bz_engine_step": (C.c_int, [P, C.POINTER(C.c_int)]),
    "bz_engine_poll": (C.c_int, [P, C.POINTER(EngineEvent), C.c_int, C.POINTER(C.c_int)]),
    "bz_engine_stats": (C.c_int, [P, C.POINTER(EngineStats)]),
    "bz_engine_read_status": (C.c_int, [P, C.c_int64, P, C.POINTER(C.c_int32)]),
    "bz_engine_free": (C.c_int, [P]),
    "bz_spec_accept": (C.c_int, [P, P, C.c_int64, C.c_int64, P, P]),
    "bz_forward_kv_verify": (C.c_int, [P, P, C.c_int, P, C.c_int, P, C.POINTER(C.c_int32), P, C.POINTER(C.c_int32)]),
    "bz_speculative_create": (C.c_int, [P, P, C.POINTER(SpecConfig), C.POINTER(P)]),
    "bz_speculative_free": (C.c_int, [P]),
    "bz_lora_table_create": (C.c_int, [P, C.POINTER(LoraTableConfig)]),
    "bz_lora_create": (C.c_int, [P, C.c_int, C.c_float, C.c_int, C.POINTER(P)]),
    "bz_lora_add": (C.c_int, [P, C.c_char_p, C.c_int, P, C.POINTER(C.c_int64), P, C.POINTER(C.c_int64)]),
    "bz_lora_free": (C.c_int, [P]),
    "bz_lora_load": (C.c_int, [P, C.c_char_p, C.POINTER(P)]),
    "bz_lora_describe": (C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "bz_lora_attach": (C.c_int, [P, C.c_int, P]),
    "bz_lora_detach": (C.c_int, [P, C.c_int]),
    "bz_model_set_lora": (C.c_int, [P, C.c_int]),
    "bz_decode_batch_graph_set_adapters": (C.c_int, [P, P]),
    "bz_lora_apply": (C.c_int, [P, C.c_int, C.c_uint32, P, P, P, C.c_int, C.c_int, P]),
    "bz_generate_speculative": (C.c_int, [P, P, C.c_int, C.POINTER(GenConfig), P, C.POINTER(GenStats), C.POINTER(SpecStats)]),
}


def build(force=False):
    """Compile blazr_amd/csrc for gfx950 with hipcc (cross-compiles without a GPU)."""
    args = ["make", "-s", "-C", os.path.join(_HERE, "csrc")]
    if force:
        subprocess.run(args + ["clean"], check=True)
    subprocess.run(args, check=True)


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise BlazrHipError(E_NODEVICE, "%s not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                            "(there is no CPU fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)   # AttributeError here == a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if L.bz_abi_version() != ABI_VERSION:
            raise BlazrHipError(E_INVALID, "ABI version mismatch")
        _LIB = L
    return _LIB


def check(rc):
    if rc != OK:
        raise BlazrHipError(rc, lib().bz_last_error().decode("utf-8", "replace"))
