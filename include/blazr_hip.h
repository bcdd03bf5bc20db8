/*
 * blazr_hip.h -- C ABI of libblazr_hip.so: the MI355X (gfx950) forward path that sits where blazr's
 * `boostr` dependency sits today.
 *
 * blazr is generic over `R: boostr::Runtime` (/root/reference/src/engine/executor.rs:67-80).  A Rust
 * `HipRuntime` whose client methods forward to the functions below is the drop-in; the extern "C" block a
 * maintainer would add is shown in INTEGRATION.md.  Every entry point cites the reference interface it
 * replaces (file:line under /root/reference).
 *
 * Conventions
 *   - every function returns BZ_OK (0) or a negative BZ_E* code; bz_last_error() gives the message of the
 *     calling thread's last failure (boostr returns Result<_, E: Display>, stringified by blazr with
 *     anyhow!("...: {}", e), e.g. executor_generate.rs:138).  No C++ exception crosses the boundary.
 *   - handles are opaque; all device work is enqueued on the device handle's HIP stream; a cache / state
 *     object must not be used from two host threads at once (blazr owns one per request,
 *     executor_generate.rs:131,208,350).
 *   - plain pointers and sizes only.  "host" pointers are ordinary host memory; device memory is only
 *     reachable through bz_tensor handles.
 *   - there is NO CPU fallback: without a HIP device every compute entry point fails with BZ_E_NODEVICE.
 */
#ifndef BLAZR_HIP_H
#define BLAZR_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BZ_ABI_VERSION 4

enum {
  BZ_OK = 0,
  BZ_E_INVALID = -1,    /* bad argument / shape / state */
  BZ_E_NODEVICE = -2,   /* no usable HIP device */
  BZ_E_HIP = -3,        /* HIP runtime error (message has hipGetErrorString) */
  BZ_E_UNSUPPORTED = -4,/* valid request this build does not implement */
  BZ_E_NOTFOUND = -5,   /* tensor name not registered */
  BZ_E_OOM = -6
};

/* boostr::DType::{F32,F16,BF16,I64,I32,U32} (executor_cache.rs:178, awq.rs:194, gptq.rs:222) + U8 for raw blocks */
enum { BZ_F32 = 0, BZ_F16 = 1, BZ_BF16 = 2, BZ_I64 = 3, BZ_I32 = 4, BZ_U32 = 5, BZ_U8 = 6 };

/* ggml type ids accepted by bz_model_add_gguf (format::Gguf tensor_info().ggml_type, loader/gguf.rs:33) */
enum { BZ_GGML_F32 = 0, BZ_GGML_F16 = 1, BZ_GGML_Q4_0 = 2, BZ_GGML_Q4_1 = 3, BZ_GGML_Q5_0 = 6, BZ_GGML_Q5_1 = 7, BZ_GGML_Q8_0 = 8, BZ_GGML_Q4_K = 12, BZ_GGML_Q5_K = 13, BZ_GGML_Q6_K = 14, BZ_GGML_BF16 = 30 };

enum { BZ_ARCH_LLAMA = 0, BZ_ARCH_MAMBA2 = 1, BZ_ARCH_DEEPSEEK2 = 2 };
enum { BZ_ROPE_NONE = 0, BZ_ROPE_LINEAR = 1, BZ_ROPE_LLAMA3 = 2, BZ_ROPE_YARN = 3 };

typedef struct bz_device bz_device;
typedef struct bz_tensor bz_tensor;
typedef struct bz_model bz_model;
typedef struct bz_kv bz_kv;
typedef struct bz_paged_kv bz_paged_kv;
typedef struct bz_decode_graph bz_decode_graph;
typedef struct bz_ssm_state bz_ssm_state;

/* POD mirror of the fields of boostr::model::UniversalConfig that the forward path reads
 * (loader/safetensors/config.rs:31-95, loader/gguf.rs:101-306, config/blazr.rs:35-52). */
typedef struct {
  int32_t abi_version;     /* BZ_ABI_VERSION */
  int32_t arch;            /* BZ_ARCH_* */
  int32_t hidden, n_layers, n_heads, n_kv_heads, head_dim, inter, vocab;
  int32_t max_seq_len;
  float   rms_eps;         /* default 1e-5, gguf.rs:157-160 */
  int32_t act_dtype;       /* inference dtype: BZ_F16 for AWQ/GPTQ (awq.rs:69-71), BZ_F32 for GGUF (gguf.rs:305) */
  int32_t tie_embeddings;  /* lm_head aliases model.embed_tokens.weight */
  float   rope_theta;
  int32_t rope_interleaved;/* 0: HF half-split pairs, 1: GGML NORM pairs (2i,2i+1) */
  int32_t rope_scaling;    /* BZ_ROPE_* ; fields below per loader/safetensors/config.rs:83-95 */
  float   rope_factor, rope_low_freq_factor, rope_high_freq_factor;
  int32_t rope_original_max_pos;
  /* boostr::model::SsmConfig (loader/gguf.rs:219-262) -- BZ_ARCH_MAMBA2 only */
  int32_t ssm_d_inner, ssm_n_heads, ssm_head_dim, ssm_d_state, ssm_n_groups, ssm_conv_kernel;
  /* BZ_ARCH_DEEPSEEK2 only: AttentionConfig kv_latent_dim / q_latent_dim / d_rope (loader/gguf.rs:188-196) plus the HF head split,
   * MoeConfig expert_count / expert_used_count / shared experts (loader/gguf.rs:271-283).  For this arch `inter` is the dense MLP width of
   * layers < moe_first_dense, `n_kv_heads` / `head_dim` are ignored (the latent cache is created with n_kv = 1, head_dim = rank + rope). */
  int32_t mla_kv_lora_rank, mla_q_lora_rank, mla_nope_dim, mla_rope_dim, mla_v_dim;
  int32_t moe_n_experts, moe_top_k, moe_n_shared, moe_inter, moe_first_dense, moe_norm_topk;
  float   moe_routed_scale;
  /* BZ_ROPE_YARN (RopeScalingConfig beta_fast / beta_slow / attention_factor, loader/safetensors/config.rs:83-95 -- the reference maps them to None = the
   * defaults): 0 means default (beta_fast 32, beta_slow 1, attention_factor 0.1 ln(factor) + 1).  cos / sin are multiplied by the attention factor.
   * mla_softmax_mscale (DeepSeek-V2 YaRN, mscale_all_dim): the MLA softmax scale is multiplied by its square; 0 = 1. */
  float   rope_beta_fast, rope_beta_slow, rope_attn_factor, mla_softmax_mscale;
  /* BZ_ARCH_LLAMA only (AttentionConfig.sliding_window, config/blazr.rs:171): sliding_window W > 0 = the query at position p attends to positions
   * max(0, p - W + 1) .. p (W keys including itself; HF Mistral semantics), 0 = full attention.  sliding_window_pattern n > 1 = every n-th layer
   * (l % n == n - 1) is global and the others are windowed (Gemma2: 2); 0 / 1 = every layer windowed.  Both took formerly reserved slots, where zero
   * means what it always meant.  The KV cache stays full length: rows below the window are not read. */
  int32_t sliding_window, sliding_window_pattern;
  int32_t reserved[2];
} bz_model_config;

/* ---- errors / device ------------------------------------------------------------------------------- */
const char* bz_last_error(void);
int bz_abi_version(void);
/* boostr::CudaDevice::new(id) + CudaClient::new(device) (cli/run.rs:70-81) */
int bz_device_open(int device_id, bz_device** out);
int bz_device_close(bz_device* dev);
int bz_device_synchronize(bz_device* dev);
/* CudaDevice::memory_info() (cli/serve.rs:61) */
int bz_device_memory_info(bz_device* dev, size_t* free_bytes, size_t* total_bytes);
int bz_device_name(bz_device* dev, char* buf, size_t n);
/* raw hipStream_t of the handle (for callers that time with HIP events on the launch stream) */
void* bz_device_stream(bz_device* dev);

/* ---- tensors (Tensor<R>::from_slice / zeros / to_vec / record_event / to_vec_pipelined) --------------- */
int bz_tensor_from_host(bz_device* dev, int dtype, const int64_t* shape, int ndim, const void* host, bz_tensor** out);
int bz_tensor_zeros(bz_device* dev, int dtype, const int64_t* shape, int ndim, bz_tensor** out);
int bz_tensor_free(bz_tensor* t);
int bz_tensor_to_host(const bz_tensor* t, void* host, size_t bytes);           /* Tensor::to_vec (sampling.rs:49) */
int bz_tensor_nbytes(const bz_tensor* t, size_t* out);
int bz_tensor_copy_from_host(bz_tensor* t, const void* host, size_t bytes);
/* record_event() -> u64 ; to_vec_pipelined(event) (executor_cache.rs:199-204): event-synchronised D2H on a copy stream */
int bz_event_record(bz_device* dev, uint64_t* event_out);
int bz_event_sync(bz_device* dev, uint64_t event);
int bz_tensor_to_host_pipelined(const bz_tensor* t, uint64_t event, void* host, size_t bytes);

/* ---- model construction (VarMap::insert / insert_decomposed_quant / from_gguf -> LoadedModel::load) --- */
int bz_model_create(bz_device* dev, const bz_model_config* cfg, bz_model** out);
int bz_model_free(bz_model* m);
/* VarMap::insert(name, tensor) (awq.rs:104, regular.rs:89-117). HF tensor names; shape [N,K] or [N]. dtype F32/F16/BF16. */
int bz_model_add_dense(bz_model* m, const char* name, int dtype, const int64_t* shape, int ndim, const void* host);
/* DecomposedQuantTensor::new(qweight u32[K,N/8], scales f32[K/gs,N], qzeros f32[K/gs,N], None, Awq{gs}, [N,K]) (awq.rs:190-225) */
int bz_model_add_awq(bz_model* m, const char* name, int64_t N, int64_t K, const uint32_t* qweight, const float* scales,
                     const float* zeros, int group_size);
/* DecomposedQuantTensor::new(qweight u32[K/8,N], scales f32[G,N], qzeros u32[G,N/8], g_idx i32[K]?, Gptq{gs}, [N,K]) + bias f32[N]? (gptq.rs:198-259) */
int bz_model_add_gptq(bz_model* m, const char* name, int64_t N, int64_t K, const uint32_t* qweight, const float* scales,
                      const uint32_t* qzeros, const int32_t* g_idx, const float* bias, int group_size);
/* VarMap::from_gguf (gguf.rs:33): raw ggml blocks of one tensor, N rows of K weights */
int bz_model_add_gguf(bz_model* m, const char* name, int ggml_type, int64_t N, int64_t K, const void* raw_blocks);
/* FP8 (OCP E4M3, e4m3fn) weights of the *-FP8 / *-FP8-dynamic SafeTensors releases, run weight-only (W8A16): W[n][k] = scale[n] e4m3(weight[n][k]), one scale
 * per tensor (n_scale 1, broadcast) or per output row (n_scale N), optional f32 bias.  y = R(f32(scale[n] sum_k x[k] e4m3(weight[n][k])) + bias[n]): the sum
 * exact, the scale applied once to the finished sum.  N % 64 or K % 64: BZ_E_UNSUPPORTED; n_scale other than 1 or N, a non-finite scale, a NaN code (0x7F /
 * 0xFF) in the weights: BZ_E_INVALID, each naming the tensor.  Llama family only (Mamba2 / DeepSeek-V2: BZ_E_UNSUPPORTED at bz_model_finalize).  Beyond the
 * reference.  New symbol only: BZ_ABI_VERSION is unchanged. */
int bz_model_add_fp8(bz_model* m, const char* name, int64_t N, int64_t K, const uint8_t* weight /*[N][K] e4m3*/, const float* scale, int64_t n_scale /*1 or N*/,
                     const float* bias /*nullable [N]*/);
/* MXFP4 (OCP microscaling FP4) weights of the *-MXFP4 SafeTensors releases (Quark), run weight-only (W4A16): weight holds E2M1 codes (0..7 = 0, 0.5, 1, 1.5, 2,
 * 3, 4, 6; bit 3 the sign), two per byte -- the LOW nibble of byte j is element 2 j, the high nibble element 2 j + 1 -- and scale one E8M0 code per block of
 * 32 along K: W[n][k] = 2^(scale[n][k / 32] - 127) e2m1(weight[n][k]).  y = R(f32(sum_k x[k] W[n][k]) + bias[n]), the sum exact (double over exact products,
 * rounded to f32 once).  ASSUMPTION: the nibble order could not be checked against a published file; tests/mxfp4_cases.py (the writer) and this call define it,
 * and mx4_pair_bits in bz_mxfp4.hip is the one place that reads it.  N % 64 or K % 64: BZ_E_UNSUPPORTED; a scale code of 255 (NaN): BZ_E_INVALID; a scale code
 * of 253 or 254 (6 . 2^(c - 127) is not a finite f32): BZ_E_UNSUPPORTED; each naming the tensor.  Llama family and 16-bit activations only (Mamba2, DeepSeek-V2,
 * f32 activations, an MXFP4 lm_head: BZ_E_UNSUPPORTED at bz_model_finalize).  Beyond the reference.  New symbol only: BZ_ABI_VERSION is unchanged. */
int bz_model_add_mxfp4(bz_model* m, const char* name, int64_t N, int64_t K, const uint8_t* weight /*[N][K/2]*/, const uint8_t* scale /*[N][K/32]*/,
                       const float* bias /*nullable [N]*/);
/* LoadedModel::load(&config.model, &mut vb) (awq.rs:133-136): validates names/shapes, repacks weights into the
 * kernels' HBM layout, builds RoPE tables and workspaces.  Host copies passed to add_* may be freed afterwards. */
int bz_model_finalize(bz_model* m);
/* LoadedModel::{num_layers, num_kv_heads, head_dim, hidden_size, vocab_size, needs_kv_cache, needs_ssm_state} */
int bz_model_get_config(const bz_model* m, bz_model_config* out);
/* bytes of weights resident in HBM after repack, and the algorithmic bytes one decoded token streams */
int bz_model_weight_bytes(const bz_model* m, size_t* resident, size_t* per_token_stream);

/* ---- checkpoint ingestion (the loader either side of LoadedModel::load) ---------------- */
enum { BZ_FORMAT_SAFETENSORS = 0, BZ_FORMAT_GGUF = 1 };          /* loader/detect.rs:9-15 ModelFormat */
typedef struct { int32_t format; int32_t has_config; char weights_path[1024]; char config_path[1024]; } bz_model_source;   /* detect.rs:17-26 ModelSource */
/* detect_model_source(path) (loader/detect.rs:34-150): a .safetensors / .gguf file, or a directory (model.safetensors, pytorch_model.safetensors,
 * model-00001-of-*.safetensors, *.gguf in that order; SafeTensors preferred over GGUF); config.json / .yaml / .yml next to the weights. */
int bz_detect_model_source(const char* path, bz_model_source* out);
enum { BZ_LAYER_TRANSFORMER = 0, BZ_LAYER_MAMBA2 = 1, BZ_LAYER_MAMBA3 = 2, BZ_LAYER_MLA_MOE = 3, BZ_LAYER_MLA_MLP = 4 };   /* detection::LayerType */
typedef struct { int32_t format; /* 0 HuggingFace ("model." prefix), 1 Oxidizr */ int32_t num_layers, tie_word_embeddings; uint8_t layer_types[512]; } bz_detected_arch;
/* boostr::model::detection::detect_architecture_from_names as the reference's tests pin it (loader/safetensors/detect_arch.rs:200-315) */
int bz_detect_architecture_from_names(const char* const* names, int n, bz_detected_arch* out);
typedef struct { int32_t quant_method; /* 0 none, 1 awq, 2 gptq, 3 fp8, 4 mxfp4 (quark) */ int32_t group_size; int32_t torch_dtype; /* BZ_* or -1 */ } bz_quant_info;
/* HuggingFaceConfig::from_json(..).to_universal() + detect_dtype_from_config (loader/safetensors/config.rs:14-70,83-95): HF config.json text ->
 * config POD; quantization_config (detect_arch.rs:79-90,118-131,146-196) -> quant info.  AWQ / GPTQ force f16 (awq.rs:69-71). */
int bz_config_from_hf_json(const char* json_text, bz_model_config* cfg, bz_quant_info* quant);
typedef struct { char architecture[64]; int32_t n_tensors, version, dominant_ggml_type, is_mla, is_moe, is_ssm; uint64_t file_size_bytes; } bz_gguf_info;
/* config_from_gguf_metadata + get_gguf_info (loader/gguf.rs:101-306,309-346): GGUF metadata -> config POD (inference dtype f32, gguf.rs:305) */
int bz_config_from_gguf(const char* path, bz_model_config* cfg, bz_gguf_info* info);
/* SafeTensorsLoader::{tensor_names, tensor_info, is_sharded, num_shards, total_size} (regular.rs:38-61) as one JSON document */
int bz_safetensors_describe(const char* path, char* json_out, size_t cap, size_t* needed);
/* loaders.rs load_model -> regular.rs:20-86 / awq.rs:40-137 / gptq.rs:40-137 / gguf.rs:20-44: detect, configure, add every tensor, finalize */
int bz_load_model(bz_device* dev, const char* path, bz_model** out, bz_model_config* cfg_out);

/* ---- inference state ---------------------------------------------------------------------------------- */
/* LayeredKvCache::new_positional(layers,batch,kv_heads,initial_capacity,max_seq_len,head_dim,dtype,device) (executor_generate.rs:350-353) */
int bz_kv_create(bz_device* dev, int layers, int batch, int n_kv_heads, int initial_capacity, int max_seq_len, int head_dim,
                 int dtype, bz_kv** out);
int bz_kv_free(bz_kv* kv);
int bz_kv_reset(bz_kv* kv);
int bz_kv_seq_len(const bz_kv* kv);                    /* LayeredKvCache::seq_len() (executor_generate.rs:371) */
/* debug/test: copy K or V rows [0,len) of (layer, kv_head) to host as f32 [len][head_dim] */
int bz_kv_read(const bz_kv* kv, int layer, int kv_head, int which /*0=K,1=V*/, int len, float* host);
/* LayeredPagedKvCache::new(layers,num_blocks,block_size,kv_heads,head_dim,dtype,device) (executor_generate.rs:208-210) */
int bz_paged_kv_create(bz_device* dev, int layers, int num_blocks, int block_size, int n_kv_heads, int head_dim, int dtype,
                       bz_paged_kv** out);
int bz_paged_kv_free(bz_paged_kv* kv);
int bz_paged_kv_set_seq_len(bz_paged_kv* kv, int seq_len);  /* set_seq_len (executor_generate.rs:242,286) */
/* The first n_slots slots of block src -> block dst: every layer, K and V, every KV head (the prefix cache's copy-on-write; 16-byte vectors, head_dim % 8 == 0).
 * Waits for the copy.  BZ_E_INVALID for a block outside the pool, src == dst, n_slots outside 1 .. block_size. */
int bz_paged_kv_copy_slots(bz_paged_kv* kv, int src, int dst, int n_slots);
/* TEST AND DEBUG ACCESSOR, not part of the serving path: one block of one layer as stored ([kv_head][block_size][hd] in the pool's dtype), raw bytes to the
 * host; which: 0 = K, 1 = V.  Waits for the stream.  (The paged pool had no read-back; the copy kernel's tests need one.) */
int bz_paged_kv_read_block(const bz_paged_kv* kv, int layer, int block, int which, void* host, size_t nbytes);
/* TEST AND DEBUG ACCESSOR, the mirror of bz_paged_kv_read_block: raw bytes of one block of one layer from the host into the pool; waits for the stream.
 * (The paged pool has no insert op; tests of the batched decode attention inject caches through it -- engine/batch_decode.rs:35-150.) */
int bz_paged_kv_write_block(bz_paged_kv* kv, int layer, int block, int which, const void* host, size_t nbytes);
int bz_paged_kv_seq_len(const bz_paged_kv* kv);

/* LayeredSsmState::new(layers, batch, mamba_config, dtype, device) (executor_generate.rs:131-133): recurrent state
 * [layers][n_heads][head_dim][d_state] in `dtype` + conv window [layers][conv_dim][k-1] (docs/architecture.md:52-54) */
int bz_ssm_state_create(bz_model* m, int batch, int dtype, bz_ssm_state** out);
int bz_ssm_state_free(bz_ssm_state* s);
int bz_ssm_state_reset(bz_ssm_state* s);

/* ---- forward ------------------------------------------------------------------------------------------ */
/* process_decode_batch (engine/batch_decode.rs:35-150): N sequences, one new token each, one shared paged cache; slot_mapping I32[N],
 * block_table I32[N, max_blocks] (rows padded with 0), seq_lens host i32[N] (length of each sequence including the new token).
 * logits_out F32 [N, vocab].  int4 (no act-order) and dense 16-bit models share the weights across the batch (multi-row dot4 kernel up to 8
 * sequences, matrix-core GEMMs beyond); other formats run the sequences one after another. */
int bz_forward_paged_batch(bz_model* m, const bz_tensor* tokens, int N, bz_paged_kv* kv, const bz_tensor* slot_mapping, const bz_tensor* block_table,
                           int max_blocks, const int32_t* seq_lens, bz_tensor* logits_out);
/* LoadedModel::forward_with_ssm_state(&input, &mut ssm) (executor_generate.rs:137,148): Mamba2; tokens I64 [1,S].  S >= 8 on a dense 16-bit
 * model takes the batched prefill (matrix-core GEMMs + in-kernel scan over the tokens); the state it leaves continues like the per-token one. */
int bz_forward_ssm(bz_model* m, const bz_tensor* tokens, int S, bz_ssm_state* state, bz_tensor* logits_out, uint32_t flags);
#define BZ_FWD_ALL_LOGITS 1u  /* logits for all S positions ([S,V]); default: last position only ([1,V]) */
/* LoadedModel::forward_with_kv_cache(&input,&mut kv,position) (executor_generate.rs:357,372).
 * tokens: I64 [1,S] device tensor; logits_out: F32 [S or 1, vocab] device tensor (values rounded to act dtype). */
int bz_forward_kv(bz_model* m, const bz_tensor* tokens, int S, bz_kv* kv, int position, bz_tensor* logits_out, uint32_t flags);
/* LoadedModel::forward_with_paged_kv_cache(input,cache,slot_mapping,block_table,seq_len_k,start_pos) (executor_generate.rs:259-262,289-292).
 * slot_mapping I32 [S], block_table I32 [1,n_table] device tensors. */
int bz_forward_paged(bz_model* m, const bz_tensor* tokens, int S, bz_paged_kv* kv, const bz_tensor* slot_mapping,
                     const bz_tensor* block_table, int n_table, int seq_len_k, int start_pos, bz_tensor* logits_out, uint32_t flags);
/* forward_embed / forward_layers_range(hidden, prev_mlp, kv, start, end, position) / forward_head(hidden, prev_mlp)
 * (cli/swarm_forward.rs:205,239-263; executor_multimodal.rs:263-268).  hidden/prev_mlp: F32 [S,hidden] device tensors;
 * has_prev: in/out flag (prev_mlp = Option<Tensor>).  head(layers(embed(x))) == forward_kv(x) bit-for-bit. */
int bz_forward_embed(bz_model* m, const bz_tensor* tokens, int S, bz_tensor* hidden_out);
int bz_forward_layers_range(bz_model* m, bz_tensor* hidden, bz_tensor* prev_mlp, int* has_prev, int S, bz_kv* kv, int start,
                            int end, int position);
int bz_forward_head(bz_model* m, const bz_tensor* hidden, const bz_tensor* prev_mlp, int has_prev, int S, bz_tensor* logits_out,
                    uint32_t flags);

/* ---- sampling ----------------------------------------------------------------------------------------- */
/* SamplingOps::logits_to_token(logits, ids, cnts, n, repeat, freq, presence, temperature, top_k, top_p, min_p, seed)
 * -> I64[1] on device (engine/sampling.rs:445-460).  logits F32 [rows,vocab]: the LAST row is used (narrow).
 * ids I64[n], cnts I32[n] device tensors (may be NULL when n == 0). */
int bz_logits_to_token(bz_device* dev, const bz_tensor* logits, int64_t rows, int64_t vocab, const bz_tensor* ids,
                       const bz_tensor* cnts, int n, float repeat_penalty, float freq_penalty, float presence_penalty,
                       float temperature, int top_k, float top_p, float min_p, uint64_t seed, bz_tensor* token_out);
/* decode_graph::argmax_to_buf(client, logits, next_token_buf) (cuda_graphs.rs:107,128); argmax_on_gpu (executor_cache.rs:189-196) */
int bz_argmax_to_buf(bz_device* dev, const bz_tensor* logits, int64_t rows, int64_t vocab, bz_tensor* token_out);

/* ---- whole-step graph (Runtime::capture_graph + DecodeGraph, cuda_graphs.rs:97-189) --------------------- */
/* Captures one greedy decode step {embed(token_buf) -> layers -> head -> argmax -> token_buf, ++position} as a hipGraph
 * over stable buffers with a device-resident position.  The cache must already hold the prefill. */
int bz_decode_graph_capture(bz_model* m, bz_kv* kv, bz_decode_graph** out);
int bz_decode_graph_capture_paged(bz_model* m, bz_paged_kv* kv, int max_blocks, bz_decode_graph** out);
int bz_decode_graph_capture_ssm(bz_model* m, bz_ssm_state* state, bz_decode_graph** out);
/* DecodeGraph::seed_next_token (cuda_graphs.rs:149-163): first input token + its position */
int bz_decode_graph_seed(bz_decode_graph* g, int64_t token, int position);
/* paged only: block table for the sequence (host i32[n]) -- slot_mapping is derived on device from position */
int bz_decode_graph_set_block_table(bz_decode_graph* g, const int32_t* block_table, int n);
/* DecodeGraph::pre_replay_and_launch (cuda_graphs.rs:166-170): one graph launch = one token */
int bz_decode_graph_replay(bz_decode_graph* g);
/* event-pipelined read of the token produced by replay number `step` (0-based since seed) */
int bz_decode_graph_read_token(bz_decode_graph* g, int64_t step, int64_t* token_out);
/* last logits of the most recent replay (F32 [vocab]) copied to host */
int bz_decode_graph_read_logits(bz_decode_graph* g, float* host, size_t n);
int bz_decode_graph_free(bz_decode_graph* g);

/* ---- batched decode graph (Executor::capture_batched_graph / replay_batched_graph + BatchedGraphState, cuda_graphs_batched.rs:43-257) --------
 * ONE hipGraph decodes one token for N sequences over a shared paged cache: the weight-sharing multi-row step of bz_forward_paged_batch between
 * two bookkeeping kernels.  Stable-address device buffers as in BatchedGraphState (token_buf [N], slot_mapping [N], block_table [N, max_blocks],
 * next_token_buf [N]); beyond the reference (one shared seq_len_k) every sequence keeps its own device-resident position, the argmax
 * (batch_argmax_to_buf) is fed back on the device and the slot is derived from the block table, so consecutive replays need no host work.
 * Llama-family models that take the multi-row step (int4 without act-order, or dense 16-bit; 16-bit lm_head); 2 <= N <= 512. */
typedef struct bz_batch_graph bz_batch_graph;
int bz_decode_batch_graph_capture(bz_model* m, bz_paged_kv* kv, int N, int max_blocks, bz_batch_graph** out);
/* state before the first replay: tokens[i] = the token sequence i feeds next, seq_lens[i] = its length INCLUDING that token (batch_decode.rs:79-88),
 * block_table = host I32 [N, max_blocks] */
int bz_decode_batch_graph_seed(bz_batch_graph* g, const int64_t* tokens, const int32_t* seq_lens, const int32_t* block_table);
/* new block-table rows (a sequence is about to cross into a block the device table does not hold yet) */
int bz_decode_batch_graph_set_block_table(bz_batch_graph* g, const int32_t* block_table);
int bz_decode_batch_graph_replay(bz_batch_graph* g);
/* the N greedy tokens produced by replay `step` (0-based since the seed); waits for the device */
int bz_decode_batch_graph_read_tokens(bz_batch_graph* g, int64_t step, int64_t* tokens_out);
/* logits F32 [N, vocab] of the last replay: a device tensor owned by the graph (do not free) */
int bz_decode_batch_graph_logits(bz_batch_graph* g, bz_tensor** logits_out);
int bz_decode_batch_graph_free(bz_batch_graph* g);

/* Batched device sampler: what the reference's batched step does by calling logits_to_token_on_device once per sequence, each with its own gen_config
 * (engine/batch_decode.rs:149-168), as one fixed sequence of launches over all N rows.  Per row the token is what bz_logits_to_token (sampling.rs:445-460)
 * gives for that row alone with ids / cnts = the penalty window (sampling.rs:169-191) of the row's device-resident token history and seed = seed + draw index.
 * The handle owns parameters, history rings, draw counters and all workspace; a sample call allocates nothing, copies nothing from the host and does not
 * synchronise, so it can be captured into a hipGraph.  1 <= N <= 512, 1 <= V <= 2^20.  New symbols only: BZ_ABI_VERSION is unchanged. */
#define BZ_SAMPLER_WINDOW_MAX 256
typedef struct {
  float   temperature;          /* 0 = greedy on the penalised row, as bz_logits_to_token */
  int32_t top_k; float top_p, min_p;
  float   repeat_penalty, frequency_penalty, presence_penalty;
  int32_t repeat_last_n;        /* 1..BZ_SAMPLER_WINDOW_MAX whenever a penalty is active (default 64); else ignored */
  uint64_t seed;                /* draw number t of this row uses seed + t, as bz_generate uses gc->seed + i */
  int32_t reserved[4];
} bz_row_sampling;
typedef struct bz_batch_sampler bz_batch_sampler;
int bz_batch_sampler_create(bz_device* dev, int N /*1..512*/, int64_t V, bz_batch_sampler** out);
int bz_batch_sampler_free(bz_batch_sampler* s);
/* (re)configure one row: parameters, the token history it starts from (host, the last n_history tokens of the sequence, prompt included;
 * only the last BZ_SAMPLER_WINDOW_MAX are kept), and the index of its next draw.  Takes effect at the next sample / replay.  Rows start greedy. */
int bz_batch_sampler_set_row(bz_batch_sampler* s, int row, const bz_row_sampling* p, const int64_t* history, int n_history, int64_t draw_index);
/* logits F32 [N,V] -> tokens_out I64 [N]; appends each row's token to its history and increments its draw index.  Enqueued on the device stream. */
int bz_batch_sampler_sample(bz_batch_sampler* s, const bz_tensor* logits, bz_tensor* tokens_out);
/* bz_decode_batch_graph_capture with the sampler's launches where the argmax sits: same eligibility and refusals, plus BZ_E_INVALID when the sampler's
 * N or V differ from the graph's.  seed / replay / read_tokens / set_block_table / logits / free work unchanged; bz_batch_sampler_set_row between replays
 * reconfigures a row without a recapture.  The graph borrows the sampler: free the graph first. */
int bz_decode_batch_graph_capture_sampled(bz_model* m, bz_paged_kv* kv, int N, int max_blocks, bz_batch_sampler* s, bz_batch_graph** out);
/* Per-row logit bias and logprobs on the device (config/generation.rs:65-74 logit_bias / logprobs / top_logprobs per sequence of a batch; the reference's batched
 * path reports none: batch_engine.rs:305,429).  Opt-in per sampler: bz_batch_sampler_enable(flags) once, before the first sample or capture, allocates the
 * state; a sampler without it launches exactly what it launched before.  Order in a step (sampling.rs:414-431): logprobs phase A on the raw logits -> grammar
 * mask -> bias -> penalties / temperature / pick -> logprobs phase C.  New symbols only: BZ_ABI_VERSION is unchanged.
 *   bias (BZ_BS_BIAS): per row at most BZ_LOGIT_BIAS_MAX unique in-range (id, bias) entries.  set_row_bias dedupes on the host as bz_apply_logit_bias does (the
 *     last entry of an id wins, ids >= V are dropped: bz_logit_bias_dedupe is that step on its own, host only, outputs of n entries each); a non-finite bias, or
 *     more than BZ_LOGIT_BIAS_MAX entries after that, is BZ_E_INVALID naming the figure.  One launch adds the biases to the logits IN PLACE (the logits tensor of
 *     bz_batch_sampler_sample / the graph's logits show the biased rows) and keeps the raw values of those entries; -inf + bias stays -inf.
 *   logprobs (BZ_BS_LOGPROBS): per row top_n = -1 (off, the default) or 0..BZ_TOP_LOGPROBS_MAX.  On the row x as the lm_head wrote it (sampling.rs:197-256), with
 *     M = max x, e_i = the specified exp of x_i - M, q_i = floor(e_i * 2^40) as a 64-bit integer, S = sum q_i (exact in any order), lse = (float)log(S * 2^-40) + M:
 *     logprob of id i = x_i - lse in f32; top = the first min(top_n, V, 20) ids in (x descending, id ascending) order (NaN logits are never listed).
 *     One record per row and step: token, its logprob (from the RAW logit, whatever mask and bias did), lse, n_top (-1: the row has logprobs off, nothing else
 *     in the record is written), the top ids and their logprobs.
 *   set_row_bias / set_row_logprobs are stream-ordered and take effect at the next sample or replay without a recapture; BZ_E_INVALID on a sampler that did not
 *     enable the flag.  read_logprobs: the N records of the last bz_batch_sampler_sample call (waits for the stream).  bz_decode_batch_graph_read_logprobs: the
 *     N records of replay `step`, the companion of read_tokens (a pinned ring beside the token log, same range of steps). */
#define BZ_LOGIT_BIAS_MAX 512
#define BZ_TOP_LOGPROBS_MAX 20
enum { BZ_BS_BIAS = 1, BZ_BS_LOGPROBS = 2 };
typedef struct { int64_t token; float logprob; float lse; int32_t n_top; uint32_t top_ids[BZ_TOP_LOGPROBS_MAX]; float top_logprobs[BZ_TOP_LOGPROBS_MAX]; } bz_logprobs_record;
int bz_logit_bias_dedupe(int64_t V, const uint32_t* ids, const float* vals, int n, uint32_t* ids_out, float* vals_out, int* n_out);
int bz_batch_sampler_enable(bz_batch_sampler* s, uint32_t flags);
int bz_batch_sampler_set_row_bias(bz_batch_sampler* s, int row, const uint32_t* ids, const float* vals, int n);
int bz_batch_sampler_set_row_logprobs(bz_batch_sampler* s, int row, int top_n);
int bz_batch_sampler_read_logprobs(bz_batch_sampler* s, bz_logprobs_record* out /*[N]*/);
int bz_decode_batch_graph_read_logprobs(bz_batch_graph* g, int64_t step, bz_logprobs_record* out /*[N]*/);

/* ---- prompt scoring and pooled embeddings (beyond the reference's surface; new symbols only, BZ_ABI_VERSION unchanged) ------------------------------------
 * A prompt pass gives more than the next token.  Both calls below are a forward call (same cache writes, same seq_len bookkeeping, same LoRA handling, the same
 * prompt plan asked the same way) whose rows go to a SINK inside the library instead of a caller-owned [S, vocab] tensor.
 *
 * SCORE (echo + logprobs, perplexity, the loglikelihood requests of evaluation harnesses): targets[i] (host, [S]) is the token whose likelihood is read from row i
 *   -- the caller passes the tokens shifted by one, and -1 where nothing is wanted; a continuation is scored by a second call at position = len(context) on the
 *   same cache.  The call runs the head BZ_FWD_ALL_LOGITS would run for each chunk, with the same arguments, into a library-owned F32 [min(S, chunk), vocab]
 *   workspace (allocated on first use, grown when a later call needs more, owned by the model and freed with it: 1.05 GB for a full 2 048-row chunk at a 128 256
 *   vocabulary -- against S * vocab * 4 bytes in the caller's hands for ALL_LOGITS plus the copy to the host), so every record is the record of the ALL_LOGITS row
 *   by construction.  Per row x, the arithmetic of the batched sampler's logprobs above (sampling.rs:197-256): M = max x, q_i = floor(exp_spec(x_i - M) * 2^40),
 *   S = sum q_i (integer: order-free), lse = (float)log(S * 2^-40) + M, every logprob the f32 subtraction x - lse, top = the first min(top_n, V, 20) ids by (logit
 *   descending, id ascending).  Beyond it: the target's raw logit and its RANK = #{x_j > x_t} + #{x_j == x_t, j < t} (0-based; -0 ties with +0; a NaN logit is
 *   never counted; -1 when the target's own logit is NaN).  A row with target -1 is not scored: rank = -1, n_top = -1, logprob = lse = logit = 0.
 *   total (nullable): sum of the logprobs and their count, added on the host in row order over the scored rows whose logprob is finite.
 * EMBED (/v1/embeddings and /rerank: Executor::get_embeddings, engine/executor_embed.rs:33-55, whose comment asks for a forward_hidden that runs all layers and the
 *   final norm; pooling server/pooling.rs:4-47; cosine server/rerank.rs:139-171,206): the row of position s is the final RMSNorm of the residual stream plus the
 *   deferred residual, rounded to the activation dtype -- the row the lm_head reads -- delivered as F32 on every route; the head is not run.  pooling NONE copies
 *   the rows ([S, hidden]); CLS is row 0 of the call; LAST row S - 1; MEAN adds (double)x[s][j] in row order and returns (float)(sum / S).  ASSUMPTION: the
 *   reference's mean is an f32 running sum whose order its backend decides; a fixed-order double sum makes the result a pure function of the rows (the reference's
 *   own test vectors come out identical either way).  normalize: on the pooled vector (each row for NONE) norm = sqrt(sum (double)v_j^2), v_j = (float)((double)v_j
 *   / norm) when norm > 1e-12, else unchanged (pooling.rs:40-47).
 * BZ_E_INVALID naming the figure, before anything is enqueued: a target >= vocab or < -1, top_n outside 0..20, an unknown pooling, an `out` that is too small, and
 * whatever the forward call of the same name refuses (cache / architecture mismatch, positions).  Many short inputs in one pass: the packed batches below.  Not built:
 * scoring or embedding inside the request engine, a bidirectional (non-causal) mask for encoder-style embedding models. */
typedef struct { int32_t top_n; /* 0..20 */ int32_t reserved[7]; } bz_score_config;
typedef struct { int64_t target; float logit, logprob, lse; int32_t rank, n_top;
                 uint32_t top_ids[BZ_TOP_LOGPROBS_MAX]; float top_logprobs[BZ_TOP_LOGPROBS_MAX]; } bz_score_row;
typedef struct { double sum_logprob; int64_t n_scored; } bz_score_total;   /* host, added in row order over rows with a finite logprob */
enum { BZ_POOL_NONE = 0, BZ_POOL_MEAN = 1, BZ_POOL_CLS = 2, BZ_POOL_LAST = 3 };
typedef struct { int32_t pooling, normalize; int32_t reserved[6]; } bz_embed_config;
int bz_score_kv(bz_model* m, const bz_tensor* tokens, int S, bz_kv* kv, int position, const int64_t* targets /*host [S]*/, const bz_score_config* cfg,
                bz_score_row* rows_out /*host [S]*/, bz_score_total* total /*nullable*/);
int bz_score_paged(bz_model* m, const bz_tensor* tokens, int S, bz_paged_kv* kv, const bz_tensor* slot_mapping, const bz_tensor* block_table, int n_table,
                   int seq_len_k, int start_pos, const int64_t* targets, const bz_score_config* cfg, bz_score_row* rows_out, bz_score_total* total);
int bz_score_ssm(bz_model* m, const bz_tensor* tokens, int S, bz_ssm_state* state, const int64_t* targets, const bz_score_config* cfg, bz_score_row* rows_out,
                 bz_score_total* total);
int bz_embed_kv(bz_model* m, const bz_tensor* tokens, int S, bz_kv* kv, int position, const bz_embed_config* cfg, bz_tensor* out /*F32 [hidden], or [S,hidden] for NONE*/);
int bz_embed_paged(bz_model* m, const bz_tensor* tokens, int S, bz_paged_kv* kv, const bz_tensor* slot_mapping, const bz_tensor* block_table, int n_table,
                   int seq_len_k, int start_pos, const bz_embed_config* cfg, bz_tensor* out);
int bz_embed_ssm(bz_model* m, const bz_tensor* tokens, int S, bz_ssm_state* state, const bz_embed_config* cfg, bz_tensor* out);
/* Packed prompt batches: n_seq inputs in ONE prompt pass (the per-text loops of server/embeddings.rs:180 and server/rerank.rs:144; the continuations of a
 * loglikelihood request).  tokens I64 [T] holds the inputs end to end, seq_lens (host) their lengths, T = sum(seq_lens).  Packed row i is stored at row i of
 * `scratch`, a contiguous cache that can hold T rows (it grows up to its max_len; its content afterwards is unspecified and it is left reset), and rotated by its
 * position inside its own input; the attention keeps a query to its own input's keys (DESIGN.md section 4 "Packed prompt batches").  Where bz_packed_plan answers
 * packed = 0 (GQA groups other than 1 / 2 / 4 / 8, head_dim the MFMA kernel does not take on a 16-bit model whose longest input does not fit the scalar kernel,
 * DeepSeek-V2, models whose plan is STEPS, T below the row floor) the single-input call runs once per input inside the library -- reset, then what bz_embed_kv /
 * bz_score_kv run -- into the same layout: the single calls' bits.  Mamba2 models are refused (loop the _ssm calls).
 * bz_embed_batch: out F32 [n_seq, hidden], input i's pooled vector at row i -- bit for bit bz_pool_spec of the input's rows; NONE: all T rows, [T, hidden];
 *   normalize per pooled vector (per row for NONE).
 * bz_score_batch: rows_out [T]; targets host [T], NULL = the next token inside the row's input and -1 (not scored) on each input's last row; totals (nullable)
 *   [n_seq], per input, added on the host in row order.
 * BZ_E_INVALID naming the figure, before anything is enqueued: n_seq <= 0, a length <= 0, T over the scratch cache's capacity, T >= 2^31, an input longer than
 * max_seq_len, and what the single calls refuse.  New symbols only: BZ_ABI_VERSION is unchanged. */
int bz_embed_batch(bz_model* m, const bz_tensor* tokens /*I64 [T], packed*/, const int32_t* seq_lens /*host [n_seq]*/, int n_seq, bz_kv* scratch,
                   const bz_embed_config* cfg, bz_tensor* out /*F32 [n_seq, hidden]; NONE: [T, hidden]*/);
int bz_score_batch(bz_model* m, const bz_tensor* tokens, const int32_t* seq_lens, int n_seq, bz_kv* scratch, const int64_t* targets /*host [T], nullable*/,
                   const bz_score_config* cfg, bz_score_row* rows_out /*host [T]*/, bz_score_total* totals /*host [n_seq], nullable*/);
/* op level, as bz_pool_rows is: rotated q / k / v rows F32 [T, (nq + 2 nkv) hd] of a packed batch -> its attention output F32 [T, nq hd].  K / V are staged,
 * rounded to `dt` (BZ_F16 / BZ_BF16 / BZ_F32), into a cache of the call's own; the rows go through the kernels in the model's chunks of 2048.
 * form = BZ_PF_ATTN_MFMA | BZ_PF_ATTN_SCALAR | BZ_PF_ATTN_SCALAR_EXACT (below); window >= 0 (0: none).  n_seq = 1 runs the plain prompt launch of a single call
 * (no segment mask): the yardstick the packed forms are measured against.  Waits for the stream. */
int bz_attn_packed(bz_device* dev, const bz_tensor* qkv, const int32_t* seq_lens, int n_seq, int nq, int nkv, int hd, int dt, int form, int window, bz_tensor* out);
/* op level, as bz_spec_accept is: the records of logits F32 [R,V] rows (any R) against targets I64 [R] on the device; rows_out on the host (waits for the stream) */
int bz_score_rows(bz_device* dev, const bz_tensor* logits, int64_t R, int64_t V, const bz_tensor* targets, const bz_score_config* cfg, bz_score_row* rows_out);
/* op level: hidden F32 [S,H] rows -> out F32 [H] ([S,H] for NONE); waits for the stream (the column sums are the call's own) */
int bz_pool_rows(bz_device* dev, const bz_tensor* hidden, int64_t S, int64_t H, const bz_embed_config* cfg, bz_tensor* out);
/* The two definitions evaluated on the HOST, public for the reason bz_expf_spec is: a CPU-only test pins them against an independent restatement, and the device
 * tests compare the kernels with them.  They run the expressions the kernels run (composite key, integer term, sequential double sums). */
int bz_score_row_spec(const float* x, int64_t V, int64_t target, int top_n, bz_score_row* row_out);
int bz_pool_spec(const float* hidden, int64_t S, int64_t H, const bz_embed_config* cfg, float* out);

/* ---- host decode loop (Executor::generate contiguous branch, executor_generate.rs:341-410) ---------------- */
typedef struct {
  int32_t max_tokens;
  float   temperature;       /* 0 => greedy (generation.rs:262-264) */
  float   repeat_penalty;    /* reference default 1.1 (generation.rs:164-166); 1.0 disables */
  int32_t repeat_last_n;     /* 64 (commands.rs:40) */
  float   frequency_penalty, presence_penalty;
  int32_t top_k; float top_p, min_p; uint64_t seed;
  int64_t eos_id;            /* -1: none */
  int32_t use_graph;         /* --graphs (cli/run.rs:144-157): greedy only, penalties ignored as in the reference */
  int32_t paged;             /* --paged-attention */
  int32_t block_size;        /* 16 (inference.rs:189-191) */
  /* host-side sampler options (config/generation.rs:190-222; applied as sampling.rs:393-437 does: DRY, typical, logit bias, dynatemp, mirostat) */
  float   dry_multiplier;    /* 0 disables */
  int32_t dry_base;          /* default 2 */
  int32_t dry_allowed_length;
  float   typical_p;         /* 0 disables */
  float   dynatemp_range;    /* 0 disables */
  float   dynatemp_exponent; /* default 1.0 */
  int32_t mirostat_mode;     /* >= 2: Mirostat v2 replaces logits_to_token (sampling.rs:96-110) */
  float   mirostat_tau, mirostat_eta;
  int32_t n_logit_bias; const uint32_t* logit_bias_ids; const float* logit_bias_vals;
  int32_t reserved[4];
} bz_gen_config;
/* prefill_ms / decode_ms: host wall time of the prompt phase and of everything after it.  The other timing fields are the reference bench's
 * (/root/reference/src/cli/bench.rs:142-160,285-306), measured where its stream consumer measures them -- at the moment a token id has reached the host:
 *   ttft_ms = start -> first token; itl_*: time between consecutive tokens (p50 / p99 / max over the n_generated - 1 gaps, nearest-rank percentiles);
 *   total_ms = start -> last token; decode_tok_per_s = (n_generated - 1) / (total - ttft). */
typedef struct { double prefill_ms, decode_ms; int32_t n_generated; int32_t finish_reason; /* 0 length, 1 eos */
                 double ttft_ms, total_ms, itl_p50_ms, itl_p99_ms, itl_max_ms, decode_tok_per_s; } bz_gen_stats;
/* ---- host-side sampler pieces, each a line-for-line restatement of the reference's Rust (they run on the CPU there too) ---------------- */
float bz_compute_dynamic_temperature(const float* logits, int64_t vocab, float base, float range, float exponent);      /* sampling.rs:41-86 */
int bz_apply_dry_penalty(float* logits, int64_t vocab, const uint32_t* recent, int64_t n_recent, float multiplier, int base, int allowed_length);   /* :270-320 */
int bz_apply_typical_filter(float* logits, int64_t vocab, float typical_p);                                              /* :322-369 */
int bz_apply_logit_bias(float* logits, int64_t vocab, const uint32_t* ids, const float* bias, int n);                   /* :464-480 */
int bz_compute_logprobs(const float* logits, int64_t vocab, uint32_t chosen, int top_n, float* chosen_logprob, uint32_t* top_ids, float* top_logprobs,
                        int* n_top);                                                                                     /* :197-256 */
typedef struct bz_mirostat bz_mirostat;                                                                                  /* mirostat.rs:12-17 MirostatState */
int bz_mirostat_create(float tau, float eta, uint64_t seed, bz_mirostat** out);                                          /* mirostat.rs:19-34 */
int bz_mirostat_sample(bz_mirostat* s, const float* logits, int64_t vocab, float temperature, uint32_t* token, float* logprob);   /* :41-110 */
float bz_mirostat_mu(const bz_mirostat* s);
int bz_mirostat_free(bz_mirostat* s);
/* prompt: host i64[n_prompt]; out_tokens: host i64[max_tokens] */
int bz_generate(bz_model* m, const int64_t* prompt, int n_prompt, const bz_gen_config* gc, int64_t* out_tokens, bz_gen_stats* stats);

/* ---- grammar-constrained decoding (GrammarDfaOps, engine/executor.rs:67-80; engine/grammar.rs, engine/grammar_parser.rs) ------------------
 * bz_grammar = GrammarDfa (grammar.rs:21-64): transitions, accepting set, current state.  Host code: none of the bz_grammar_* functions needs a device.
 * A vocabulary is passed as its tokens' bytes back to back (`vocab_bytes`) and offsets[V+1] into them (offsets[0] == 0); blazr builds the same list
 * from tokenizer.decode(&[i]) (executor_generate.rs:104-113).  A token without bytes is allowed in every state (EOS and the other specials). */
typedef struct bz_grammar bz_grammar;
typedef struct bz_device_grammar bz_device_grammar;
#define BZ_GRAMMAR_REGULAR 1u
/* compile_grammar_to_dfa (grammar.rs:165-277) over parse_gbnf (grammar_parser.rs:47-190).
 *   flags == 0: the reference's semantics, quirks included (lines split at the first "::=", bodies at every '|' even inside quotes, '#' comment lines, escapes
 *     \n \t \" \\, class members `ch as u8`, only the first `root` rule expanded, a literal byte by byte, a class one state, EVERY OTHER element -- rule reference,
 *     negated class, name* name+ name? -- one byte of 0..=127; no `root` rule: one state, no transitions).  Differences, all unavoidable: the reference numbers
 *     states in HashMap order, here the numbering is canonical (breadth first from state 0, bytes ascending), so equality with the reference is equality of the
 *     language and of prefix viability; input on which the reference's parser never returns ('(' ')' or * + ? after a literal or a class: grammar_parser.rs:153-185
 *     consumes nothing) is BZ_E_UNSUPPORTED with line and column; so is a non-ASCII character outside quotes and brackets (char::is_alphanumeric is not carried).
 *     "Invalid GBNF rule: <line>" and "No rules found in GBNF grammar" are BZ_E_INVALID with the reference's messages.
 *   flags == BZ_GRAMMAR_REGULAR (beyond the reference): the regular subset of GBNF.  Quotes and brackets are honoured before '|'; groups ( ... ) with nested
 *     alternatives; * + ? after a literal, class, group or rule reference; [^...] = every byte 0..255 outside the ranges (classes are sets of bytes: UTF-8 passes
 *     through a negated class, a non-ASCII member is refused); any rule of the file may be referenced and is inlined (first definition of a name wins); a rule is
 *     one line.  Same escape table.  A recursive rule reachable from root, an undefined rule (root included), an unbalanced group or quote, more than 65535 DFA
 *     states: BZ_E_UNSUPPORTED.  Transitions into states that cannot reach an accepting state are removed; the DFA is not minimised. */
int bz_grammar_compile(const char* gbnf, uint32_t flags, bz_grammar** out);
/* a caller-compiled DFA (the fields of DeviceGrammarDfa are plain tensors, grammar.rs:130-138): table [num_states*256], -1 = no transition, every other entry
 * a state below num_states (else BZ_E_INVALID); accepting [num_states]; at most 65535 states */
int bz_grammar_from_table(int num_states, const int32_t* table, const uint8_t* accepting, bz_grammar** out);
int bz_grammar_table(const bz_grammar* g, int32_t* table_out /*[num_states*256], nullable*/, uint8_t* accepting_out /*[num_states], nullable*/);
int bz_grammar_num_states(const bz_grammar* g);      /* grammar.rs:62-64 */
int bz_grammar_current_state(const bz_grammar* g);   /* :57-59 */
int bz_grammar_is_accepting(const bz_grammar* g);    /* :47-49 */
int bz_grammar_reset(bz_grammar* g);                 /* :52-54 */
int bz_grammar_free(bz_grammar* g);
/* GrammarDfa::advance (grammar.rs:37-44) per byte exactly as the generate loop uses it (executor_generate.rs:159-161, the bool is dropped): a byte with no
 * transition leaves the state where it is and the loop goes on.  n_rejected (nullable): how many bytes had no transition. */
int bz_grammar_advance(bz_grammar* g, const uint8_t* bytes, size_t n, int* n_rejected);
/* n DFAs as one (beyond the reference): the result's table is the n tables stacked, every transition shifted by its grammar's offset; starts[i] is the state that
 * is grammar i's state 0 and the result's own current state is starts[0].  One uploaded table then serves requests with different grammars: a row's state alone
 * decides which language it is in.  More than 65535 states in total: BZ_E_UNSUPPORTED; n < 1 or a null entry: BZ_E_INVALID. */
int bz_grammar_concat(const bz_grammar* const* gs, int n, bz_grammar** out, int32_t* starts /*[n]*/);
/* bz_grammar_advance over the bytes of each of the n tokens in turn (same rule, n_rejected counts over all of them).  A token outside [0, V) is BZ_E_INVALID and
 * leaves g untouched. */
int bz_grammar_advance_tokens(bz_grammar* g, const uint8_t* vocab_bytes, const int64_t* offsets, int64_t V, const int64_t* tokens, int64_t n,
                              int* n_rejected /*nullable*/);
/* compute_token_mask (grammar.rs:69-84) from the current state: allowed_out[V] = 1 / 0.  The library-side checker of the kernel below. */
int bz_grammar_token_mask(const bz_grammar* g, const uint8_t* vocab_bytes, const int64_t* offsets, int64_t V, uint8_t* allowed_out);
/* GrammarDfa::to_device (grammar.rs:90-139).  The reference ships four f32 tensors because that is its tensor type system; here the next-state table is
 * uint16_t [num_states*256] with 0xFFFF = none (the value of boostr's INVALID_STATE, grammar.rs:9, is not visible), bytes are uint8_t packed into aligned words and
 * offsets uint32_t, and the tokens are stored in ascending byte length (results land at the caller's token index).  current_state is copied from g. */
int bz_grammar_to_device(bz_device* dev, const bz_grammar* g, const uint8_t* vocab_bytes, const int64_t* offsets, int64_t V, bz_device_grammar** out);
/* dg.current_state = dfa.current_state() (executor_generate.rs:163-165): a host field passed to the kernel as an argument, no device round trip */
int bz_device_grammar_set_state(bz_device_grammar* dg, uint32_t state);
/* the kernel stages the whole table in LDS up to this many states (64 KiB, so that two workgroups share a CU's 160 KiB) and reads it through L2 beyond;
 * bz_device_grammar_info reports which of the two a handle takes (lds_table 1 / 0).  Every out pointer is nullable. */
#define BZ_GRAMMAR_LDS_MAX_STATES 128
int bz_device_grammar_info(const bz_device_grammar* dg, int32_t* num_states, int64_t* vocab, uint32_t* state, int32_t* lds_table);
int bz_device_grammar_free(bz_device_grammar* dg);
/* GrammarDfaOps::grammar_dfa_mask_logits(&logits, grammar) (sampling.rs:415-419).  logits F32 [rows, vocab]; logits_out may be logits.  The LAST row is masked
 * (the only row logits_to_token reads; which rows boostr's kernel masks is not visible: a named assumption), other rows are copied unchanged.  A token is walked
 * from the current state through its bytes; a missing transition sets its logit to -inf, every other logit is copied bit for bit (mask_logits, grammar.rs:142-158).
 * vocab != the uploaded V: BZ_E_INVALID.  Enqueued on the device stream; no host synchronisation, no device-to-host copy.  A state that admits no token leaves an
 * all -inf row (the reference leaves that case undefined): bz_argmax_to_buf then returns what it returns for any all -inf row and the sampled path some id in [0, V). */
int bz_grammar_dfa_mask_logits(bz_device* dev, const bz_tensor* logits, int64_t rows, int64_t vocab, const bz_device_grammar* dg, bz_tensor* logits_out);
/* The cursor (beyond the reference, whose DFA state lives on the host): one device-resident DFA state per row of a decode batch, so that mask and advance need no
 * host step between tokens and can sit inside a captured graph.  Every row starts at dg's current state.  The cursor borrows dg: free the cursor first.
 *   set_row: a state below num_states, or BZ_GRAMMAR_ROW_FREE for an unconstrained row (never masked, never advanced); also zeroes the row's rejected count.
 *     Takes effect at the next launch or replay without a recapture, as bz_batch_sampler_set_row does.
 *   read: states[N] and (nullable) rejected[N] = bytes without a transition since the row was set; waits for the device.
 *   mask: logits F32 [N,V] in place, row r from state[r]: a token that dies gets -inf, nothing else is written (every other logit keeps its bits, FREE rows whole).
 *     One workgroup stages the table once (up to BZ_GRAMMAR_LDS_MAX_STATES states, else it reads through L2) and serves up to 64 rows with it.
 *   advance: tokens I64 [N]; row r walks the bytes of tokens[r] with bz_grammar_advance's rule.  A FREE row, an id outside [0, V) or a token without bytes changes
 *     nothing.  bz_grammar_to_device uploads the inverse of its length sort for this (per caller token id: first word and byte length).
 * mask and advance are enqueued on the device stream: no allocation, no copy from the host, no synchronisation. */
typedef struct bz_grammar_cursor bz_grammar_cursor;
#define BZ_GRAMMAR_ROW_FREE 0xFFFFFFFFu
int bz_grammar_cursor_create(const bz_device_grammar* dg, int N /*1..512*/, bz_grammar_cursor** out);
int bz_grammar_cursor_free(bz_grammar_cursor* c);
int bz_grammar_cursor_set_row(bz_grammar_cursor* c, int row, uint32_t state);
int bz_grammar_cursor_read(bz_grammar_cursor* c, uint32_t* states /*[N]*/, uint32_t* rejected /*[N], nullable*/);
int bz_grammar_cursor_mask(bz_grammar_cursor* c, bz_tensor* logits /*F32 [N,V], in place*/);
int bz_grammar_cursor_advance(bz_grammar_cursor* c, const bz_tensor* tokens /*I64 [N]*/);
/* The batched step with per-sequence grammars: batch advance -> multi-row forward -> mask_rows on the graph's logits -> the sampler's launches (s != NULL) or the
 * batch argmax -> advance_rows on the next-token buffer; mask before penalties / temperature / pick as sampling.rs:415-460.  One linear chain.  Eligibility and
 * refusals are those of bz_decode_batch_graph_capture(_sampled), plus BZ_E_INVALID when the cursor's N or V differ from the graph's or it lives on another device
 * handle.  seed / replay / read_tokens / set_block_table / logits / free work unchanged (logits shows the masked rows); bz_grammar_cursor_set_row between replays
 * hands a row to another grammar, or frees it, without a recapture.  The graph borrows the cursor (and the sampler): free the graph first. */
int bz_decode_batch_graph_capture_grammar(bz_model* m, bz_paged_kv* kv, int N, int max_blocks, bz_batch_sampler* s /*nullable: argmax*/, bz_grammar_cursor* c,
                                          bz_batch_graph** out);
/* bz_decode_graph_capture / _capture_paged with a cursor of N == 1 inside the step (both the short and the split-KV variant): after the head, mask -> argmax over
 * the masked row -> advance on the token buffer.  bz_decode_graph_read_logits returns the masked row.  Llama family only: Mamba2 and DeepSeek-V2 are
 * BZ_E_UNSUPPORTED; a cursor with N != 1, another V or another device handle is BZ_E_INVALID.  The graph borrows the cursor. */
int bz_decode_graph_capture_grammar(bz_model* m, bz_kv* kv, bz_grammar_cursor* c /*N == 1*/, bz_decode_graph** out);
int bz_decode_graph_capture_paged_grammar(bz_model* m, bz_paged_kv* kv, int max_blocks, bz_grammar_cursor* c, bz_decode_graph** out);
/* bz_generate with gen_config.grammar (executor_generate.rs:96-121): g == NULL is bz_generate.  With a grammar every branch (contiguous, paged, SSM) does per token
 * what the reference does, in its order (sampling.rs:385-460): host DRY / typical -> device mask -> logit bias -> penalties / temperature / logits_to_token; once the
 * token id is on the host, bz_grammar_advance with that token's bytes and set_state (executor_generate.rs:156-166, 302-312, 383-393).  Mirostat skips the mask
 * (sampling.rs:101-103) but still advances.  g is used from its current state and left in its final state; V must be the model's vocab.
 * use_graph = 1 with a grammar (beyond the reference, whose graph mode ignores grammars: cuda_graphs.rs is pure argmax_to_buf): a Llama-family model without an active
 * penalty (repeat_penalty == 1, frequency / presence == 0) takes the captured step of bz_decode_graph_capture(_paged)_grammar -- first token from the masked prompt
 * logits, a cursor seeded with the state after it, one replay per token, g brought to its final state with bz_grammar_advance_tokens.  Every other combination
 * (a penalty, which graph mode would ignore; Mamba2; DeepSeek-V2) takes the eager loop and gives the eager tokens. */
int bz_generate_grammar(bz_model* m, const int64_t* prompt, int n_prompt, const bz_gen_config* gc, bz_grammar* g /*nullable*/, const uint8_t* vocab_bytes,
                        const int64_t* offsets, int64_t V, int64_t* out_tokens, bz_gen_stats* stats);

/* ---- continuous batching: the request engine (engine/batch_engine.rs:91-169, 172-319, 322-445; engine/request_scheduler.rs:105-205;
 * config/inference.rs:89-90,136,142: max_batch_size, prefill_chunk_size, kv_pool_blocks) ------------------------------------------------
 * The scheduler (engine/request_scheduler.rs:105-205; batch_engine.rs:172-272 for the chunked prompt): host only, no device call, a pure function of its inputs.
 * The pool's last n_rows blocks are the rows' park blocks (row r parks in block num_blocks - n_rows + r); requests share the others.  Admission is FIFO without
 * skipping ahead: the head of the queue enters when a row is free and ceil((n_prompt + max_tokens) / block_size) blocks are free; it takes the lowest free row and the
 * lowest free blocks, all of them at once (growing on demand would need preemption).  prefill_chunk (0 = unlimited) prompt tokens per step over the admitted requests
 * that are not live yet, in admission order; a request prefills prompt[:-1] and becomes live in the step that completes it.  Ids count up from 0.
 *   step: the actions of one engine step, in order: BZ_SCHED_ADMIT {id, row, a = number of blocks}, BZ_SCHED_PREFILL {id, row, a .. b = prompt range},
 *         BZ_SCHED_LIVE {id, row}.  At most 3 * n_rows actions.
 *   finish: the request's end was harvested (or it was cancelled): its row and blocks are free from the next step on; a waiting request just leaves the queue.
 *
 * The prefix cache (engine/executor_cache.rs:39-131 prefix_cache_allocate; opt-in: bz_sched_enable_prefix before the first submit, bz_engine_config.prefix_cache).
 * With the switch off every decision above is unchanged.  With it on, requests submitted with their tokens (bz_sched_submit_tokens) share KV blocks; a request
 * submitted without tokens (bz_sched_submit) still works and never matches or publishes.
 *   cacheable: the F = (n_prompt - 1) / block_size full blocks of prompt[:-1].  The block that holds position n_prompt - 1 and every later one is written by decode
 *     and stays private, so a shared block is never written again.
 *   index: one entry per cached block, keyed by (parent entry, the block's block_size tokens); entry ids count up from 0, the root is parent -1.  THE KEY COMPARES
 *     THE TOKENS THEMSELVES.  A hash may speed a lookup but never decides a match: a collision would silently serve another prompt's KV (wrong tokens, no error).
 *   match at admission: walk the chain from the root over the request's full blocks: m <= F matched blocks.  Then, among the children of the last matched entry
 *     (of the root when m = 0), the one with the longest common token prefix j >= 1 with prompt[m*bs : n_prompt-1] (ties: the lowest entry id) is the copy
 *     source; j < block_size always.  The request's table starts with the m matched blocks, the rest are its own; ADMIT carries b = m (0 with the switch off); BZ_SCHED_COPY {id, row, a = source block,
 *     b = j} follows its ADMIT (the destination is its block at index m, see bz_sched_row), and its prompt starts at done = m*bs + j instead of 0.
 *     If done == n_prompt - 1 no PREFILL is emitted and LIVE comes in the admission step.
 *   reference counts: a matched block gains one reference per request using it, an entry a request published holds that request's reference; finish (or cancel)
 *     drops the references and frees the request's private blocks.  A cached block without a reference stays in the pool as evictable.  Every usable block is in
 *     exactly one state: free, private to one request, or cached (referenced or not).
 *   admission test: match first, hold the matched entries and the copy source, then require need - m <= free + evictable, where evictable counts the cached
 *     blocks that repeated leaf eviction could free: unreferenced, not a copy source named in this step, and with no such entry below them.  FIFO without
 *     skipping ahead, the lowest free row, the lowest free blocks first, as above.  A failed test changes nothing.
 *   use counter: one counter for the whole scheduler, incremented at every touch (no clock): at admission the matched entries root first, then the copy source;
 *     at publication the new entry.  An entry remembers the value of its last touch.
 *   eviction: only while the free blocks have run out, one block at a time: among the unreferenced entries without children that are not a copy source of this
 *     step, the one with the lowest use value (ties: the lowest block id) leaves the index and its block becomes free.
 *   publishing: in the step whose PREFILL covers the last slot of one of its own full prompt blocks, the block enters the index under the entry of the block
 *     before it (stream order then puts every later reader behind the writer).  If an equal entry exists already the request keeps its private duplicate and the
 *     chain goes on under the existing entry (untouched); if that entry has been evicted meanwhile the request publishes nothing more.  So a request admitted before
 *     the donor's chunk was issued does not match: prompts in flight are not deduplicated.
 *   cost: a lookup scans the children of one entry linearly with a full token compare (no hash), and the match is redone in every step for a queue head that
 *     keeps waiting: O(children * block_size) per matched block.  A root with thousands of distinct first blocks makes admission that much slower; known, not built.
 *   step: at most 4 * n_rows actions with the switch on (room for that many is required), 3 * n_rows with it off.
 *   prefix_info: cached = referenced + unreferenced entries; evictable as in the admission test; hit = an admission with tokens and done > 0, miss = one with
 *     done == 0; cached_tokens = the sum of done; evictions counts blocks evicted under pressure (flush is not counted).
 *   prefix_flush: drops every unreferenced cached block (leaf after leaf); *dropped_out (nullable) = how many. */
typedef struct bz_sched bz_sched;
enum { BZ_SCHED_ADMIT = 0, BZ_SCHED_PREFILL = 1, BZ_SCHED_LIVE = 2, BZ_SCHED_COPY = 3 };
typedef struct { int32_t kind, row; int64_t id; int32_t a, b; } bz_sched_action;
typedef struct { int32_t n_rows, num_blocks, park_blocks, free_blocks, owned_blocks, waiting, admitted, live; } bz_sched_info_t;
int bz_sched_create(int n_rows, int num_blocks, int block_size, int max_seq_len, int prefill_chunk, bz_sched** out);
int bz_sched_free(bz_sched* s);
int bz_sched_submit(bz_sched* s, int n_prompt, int max_tokens, int64_t* id_out);
int bz_sched_step(bz_sched* s, bz_sched_action* out, int max_out, int* n_out);
int bz_sched_finish(bz_sched* s, int64_t id);
int bz_sched_info(const bz_sched* s, bz_sched_info_t* out);
int bz_sched_row(const bz_sched* s, int row, int64_t* id_out /*-1: free*/, int32_t* blocks_out /*nullable*/, int max_blocks, int* n_blocks_out);
typedef struct { int32_t enabled, cached_blocks, evictable_blocks, referenced_blocks; int64_t hits, misses, cached_tokens, evictions; } bz_sched_prefix_info_t;
int bz_sched_enable_prefix(bz_sched* s);
int bz_sched_submit_tokens(bz_sched* s, const int64_t* prompt, int n_prompt, int max_tokens, int64_t* id_out);
int bz_sched_prefix_info(const bz_sched* s, bz_sched_prefix_info_t* out);
int bz_sched_prefix_flush(bz_sched* s, int* dropped_out /*nullable*/);
/* The engine (batch_engine.rs:91-169 BatchEngine::run, 322-445 the decode step and its harvest): one captured step of n_rows rows over a paged pool the engine owns;
 * every row is live or idle ON THE DEVICE, a live row ends there (stop id, or max_tokens reached) in the launch that sees its token, so several replays can be in
 * flight and their records read late.  An idle row feeds token 0 at position 0 of its own park block.  The caller drives: bz_engine_step is one scheduling iteration,
 * the library starts no thread.  Eligibility and refusals at create are those of bz_decode_batch_graph_capture (Mamba2 / DeepSeek-V2: BZ_E_UNSUPPORTED).
 *   step, in this order: (1) once `depth` replays are unread, wait for the oldest one's event and turn its record into events, releasing the rows and blocks of
 *     finished requests; (2) the scheduler's admissions and prompt chunks (bz_forward_paged on prompt[:-1]) and, for a request whose prompt is complete, the row
 *     writes that make it live (prompt[-1] at seq_len = n_prompt: its first token is draw 0 of the batched step, history = the prompt, masked from grammar_state) --
 *     all stream-ordered behind the replays already enqueued, without a read from the device or a wait; (3) one replay if any row is live in the host's view, else
 *     every unread record is drained.  busy_out = 0 when nothing is waiting, admitted or unread.
 *   submit: BZ_E_INVALID naming the figure when n_prompt + max_tokens > max_seq_len, when the request could never fit the pool, with more than 8 stop ids, with
 *     sampling other than greedy without penalties on an engine without a sampler, with a grammar state on an engine without a cursor.
 *   cancel: a waiting request leaves the queue; an admitted one's row is made idle by a stream-ordered write and its row and blocks are released; tokens of it that
 *     replays in flight still produce are dropped.  One event with finish_reason 2 (token -1) is queued.
 *   poll: events in order; a stop id is delivered as the request's last token (as bz_generate delivers eos_id).
 *   LoRA (config/generation.rs:142-145 lora_adapter, per request): lora_slot names a slot of the model's table (bz_lora_table_create before bz_engine_create).
 *     Submit refuses an empty or out-of-range slot (BZ_E_INVALID naming it).  The request's prompt chunks run under that slot, its row's slot id is written with
 *     the other row writes when it goes live and reset to -1 when the row goes idle; bz_lora_detach is refused from submit until the request's last record is
 *     read.  Cached KV rows depend on the adapter: a request with lora_slot != 0 neither looks up nor publishes prefix blocks.
 * The engine borrows the model and the cursor (free the engine first) and owns pool, sampler and graph. */
typedef struct {
  int32_t n_rows;          /* 2..512 */
  int32_t num_blocks;      /* the pool, park blocks (n_rows of them) included */
  int32_t block_size;
  int32_t max_seq_len;     /* per request: n_prompt + max_tokens; sets the block-table width */
  int32_t prefill_chunk;   /* prompt tokens per step, 0 = unlimited */
  int32_t depth;           /* replays in flight before the oldest record is read, 1..64 */
  int32_t use_sampler;     /* 1: the batched sampler picks (per-request parameters); 0: greedy argmax */
  int32_t prefix_cache;    /* 1: the prefix cache (shared prompt blocks, copy-on-write); 0: off (took the first reserved word) */
  int32_t logprobs;        /* 1: the engine's sampler is created with BZ_BS_BIAS | BZ_BS_LOGPROBS (needs use_sampler = 1); 0: off (took a reserved word) */
  int32_t reserved[7];
} bz_engine_config;
typedef struct {
  int32_t max_tokens;
  int32_t n_stop; int64_t stop_ids[8];
  uint32_t grammar_state;  /* BZ_GRAMMAR_ROW_FREE: unconstrained */
  int32_t lora_slot;       /* 0: none, k: slot k - 1 of the model's LoRA table (took the first reserved word, so a zeroed request behaves as before) */
  int32_t reserved[2];
  bz_row_sampling sampling;
} bz_request;
typedef struct { int64_t id; int64_t token; int32_t index; int32_t finish_reason; /* -1 running, 0 length, 1 stop, 2 cancelled */ int64_t replay; } bz_engine_event;
typedef struct { int64_t replays; int32_t free_blocks, total_blocks, park_blocks, live_rows, admitted, waiting, unread; int64_t prompt_tokens, generated_tokens;
                 double admit_host_ms; /* host time spent enqueueing prompt chunks and row writes */ } bz_engine_stats_t;
typedef struct bz_engine bz_engine;
int bz_engine_create(bz_model* m, const bz_engine_config* cfg, bz_grammar_cursor* cursor /*nullable, borrowed*/, bz_engine** out);
int bz_engine_submit(bz_engine* e, const int64_t* prompt, int n_prompt, const bz_request* rq, int64_t* id_out);
/* Per-request logit bias and logprobs (config/generation.rs:65-74), on an engine created with logprobs = 1 (else a non-NULL `ex` is BZ_E_INVALID).
 * bz_engine_submit is bz_engine_submit_ex with ex = NULL.  logprobs != 0: every token of the request gets a record with top_logprobs (0..20) alternatives;
 * logit_bias_*: n_logit_bias entries, checked and deduplicated as bz_batch_sampler_set_row_bias does.  The row's bias list and top_n are written with the other
 * row writes when the request goes live and cleared on the device when the row goes idle.  poll_logprobs: one entry per token event of a request that asked,
 * in event order (same id / index / token), harvested from the ring with the token record of the same replay; a cancelled request's entries are dropped. */
typedef struct { int32_t logprobs; int32_t top_logprobs; int32_t n_logit_bias; const uint32_t* logit_bias_ids; const float* logit_bias_vals; int32_t reserved[4]; } bz_request_extras;
typedef struct { int64_t id; int32_t index; int64_t token; float logprob; int32_t n_top; uint32_t top_ids[BZ_TOP_LOGPROBS_MAX]; float top_logprobs[BZ_TOP_LOGPROBS_MAX]; } bz_engine_logprobs;
int bz_engine_submit_ex(bz_engine* e, const int64_t* prompt, int n_prompt, const bz_request* rq, const bz_request_extras* ex /*nullable*/, int64_t* id_out);
int bz_engine_poll_logprobs(bz_engine* e, bz_engine_logprobs* out, int max_records, int* n_out);
int bz_engine_cancel(bz_engine* e, int64_t id);
int bz_engine_step(bz_engine* e, int* busy_out);
int bz_engine_poll(bz_engine* e, bz_engine_event* out, int max_events, int* n_out);
int bz_engine_stats(bz_engine* e, bz_engine_stats_t* out);
/* The prefix cache through the engine (prefix_cache = 1): submit hands the tokens to the scheduler; a step gathers its BZ_SCHED_COPY actions into ONE launch of
 * k_kv_copy_slots (triples staged in pinned memory, read from device memory; no allocation, no wait), enqueued ahead of that step's prompt chunks; a hit changes
 * only which positions are prefilled: the sampler's history is the whole prompt and the grammar start state is the request's.  free + private + cached ==
 * total - park at all times (bz_engine_stats.free_blocks with the counts below).  prompt_tokens_skipped = prompt positions served from cached blocks
 * (bz_engine_stats.prompt_tokens counts only what was prefilled).  prefix_flush drops every unreferenced cached block (*dropped_out nullable). */
typedef struct { int32_t enabled, cached_blocks, evictable_blocks, referenced_blocks, private_blocks, reserved; int64_t hits, misses, cached_tokens, evictions,
                 prompt_tokens_skipped, copy_launches, copied_blocks; } bz_engine_prefix_stats_t;
int bz_engine_prefix_stats(bz_engine* e, bz_engine_prefix_stats_t* out);
int bz_engine_prefix_flush(bz_engine* e, int* dropped_out /*nullable*/);
/* the status words (0 idle, 1 token, 2 + 4 * reason finished) of replay `replay` (within the last 1024), host [n_rows]; waits for that replay */
int bz_engine_read_status(bz_engine* e, int64_t replay, int32_t* status_out, int32_t* live_after_out /*nullable*/);
int bz_engine_free(bz_engine* e);

/* ---- speculative decoding (engine/generate_text.rs:41-44,61-136; engine/speculative.rs:99-125; config/inference.rs:197-208) -----------------
 * The reference takes this path whenever inference.speculative is configured (draft_model, num_speculative_tokens default 5, adaptive_depth) and hands the
 * work to boostr's SpeculativeModel::forward.  Here: a draft model proposes k tokens with k decode steps, the target verifies [t, d1 .. dk] (t = the last
 * committed token) in ONE forward whose rows are the decode step's rows bit for bit, and a kernel decides acceptance on the device.  Greedy only, so a
 * speculative run emits exactly the tokens bz_generate emits, whatever the draft proposes.  ASSUMPTION: boostr's acceptance rule for temperature > 0
 * (rejection sampling) is not visible in the reference and is not built; BZ_ABI_VERSION is unchanged (new symbols only).
 *
 * bz_spec_accept (op level; also what a caller with its own draft source -- n-gram / prompt lookup -- uses): per-row argmax of logits F32 [R,V] (ties to the lowest
 * index, as bz_argmax_to_buf), n_accept = length of the longest prefix with draft[i] == argmax[i] (draft I64 [R-1], nullable when R == 1),
 * record I64 [R+1] = {n_accept, tokens[0 .. n_accept], -1 ...} with tokens[i] = draft[i] for i < n_accept and tokens[n_accept] = argmax[n_accept]
 * (the correction, or the bonus token when everything was accepted).  1 <= R <= 16.  Enqueued on the device stream, no host synchronisation. */
int bz_spec_accept(bz_device* dev, const bz_tensor* logits, int64_t R, int64_t V, const bz_tensor* draft, bz_tensor* record);
/* The verify forward.  tokens I64 [1,R]: the last committed token, then R-1 draft tokens (1 <= R <= 16), at positions position .. position+R-1 of `kv`.
 * logits_out (nullable) F32 [R,vocab]: row r is what bz_forward_kv returns for token r alone at position+r.  n_accept / tokens_out (host, R entries: tokens[0 ..
 * n_accept], then -1) as bz_spec_accept defines them; one host synchronisation (the record's event-pipelined read).  Afterwards bz_kv_seq_len == position +
 * n_accept + 1: rows past it hold rejected tokens, no kernel reads them and the next forward overwrites them (no copy, no rollback).
 * path: 1 = the multi-row exact rows (f16 int4 model without act-order, GQA group 1/2/4/8, dense 16-bit lm_head, context within the exact row attention's LDS
 * bound -- about 6 k keys at 32/8 heads x 128): 8 rows per pass over the weights and over the lm_head; 0 = every other Llama-family model or context: the rows run on
 * the decode step token by token (correct, no gain).  Mamba2 / DeepSeek-V2: BZ_E_UNSUPPORTED. */
int bz_forward_kv_verify(bz_model* m, const bz_tensor* tokens, int R, bz_kv* kv, int position, bz_tensor* logits_out, int32_t* n_accept,
                         int64_t* tokens_out, int32_t* path);
/* SpeculativeConfig (config/inference.rs:197-208).  adaptive_depth -- ASSUMPTION, boostr's rule is not visible: after a fully accepted iteration k = min(k + 1, 15),
 * after one with fewer than half of its proposals accepted k = max(1, k - 1). */
typedef struct { int32_t num_speculative_tokens; /* 0 -> 5; 1..15 */ int32_t adaptive_depth; int32_t reserved[6]; } bz_spec_config;
/* iterations / accepted / rejected: generate_text.rs:130-135.  verify_path: 1 if every verify pass took the multi-row rows, 0 if any ran token by token, -1 if none
 * ran; final_depth: k after the last iteration; draft_ms / verify_ms: device time of the two phases (HIP events), summed over the iterations. */
typedef struct { int64_t iterations, drafted_tokens, accepted_tokens, rejected_tokens; int32_t verify_path; int32_t final_depth;
                 double draft_ms, verify_ms; } bz_spec_stats;
typedef struct bz_speculative bz_speculative;
/* Both models BZ_ARCH_LLAMA on one device handle (else BZ_E_UNSUPPORTED / BZ_E_INVALID), equal vocab sizes (else BZ_E_INVALID), num_speculative_tokens in 1..15
 * (else BZ_E_INVALID).  The handle borrows the models: free it first. */
int bz_speculative_create(bz_model* target, bz_model* draft, const bz_spec_config* cfg, bz_speculative** out);
int bz_speculative_free(bz_speculative* s);
/* generate_text.rs:61-136.  Prompt through both models' bz_forward_kv, first token = the target's argmax; per iteration the draft consumes the committed tokens it
 * has not seen (one, or two after a fully accepted iteration), proposes k tokens that stay on the device, the target verifies, ONE record read brings
 * n_accept + 1 tokens to the host.  k is clipped by max_tokens and by both models' max_seq_len.  Stops at the first eos_id among the emitted tokens
 * (finish_reason 1, nothing after it is written).  BZ_E_UNSUPPORTED: temperature != 0, any penalty (repeat_penalty != 1, frequency / presence != 0), DRY, typical,
 * dynatemp, Mirostat, logit bias, paged.  use_graph is accepted and ignored (the loop is eager).
 * bz_gen_stats keeps its definitions: ttft at the first token; inter-token gaps between the moments token ids reach the host -- the tokens of one iteration arrive
 * together, so gaps inside an iteration are 0 and the gap between iterations carries the whole iteration. */
int bz_generate_speculative(bz_speculative* s, const int64_t* prompt, int n_prompt, const bz_gen_config* gc, int64_t* out_tokens, bz_gen_stats* stats,
                            bz_spec_stats* spec_stats);

/* ---- LoRA adapters (config/generation.rs:142-145 GenerationConfig.lora_adapter; engine/lora.rs:138-257 the PEFT loader; executor.rs:397-420 and
 * server/lora.rs the registry) --------------------------------------------------------------------------------------------------------------
 * The reference loads and registers adapters and then only logs the request's choice (executor_generate.rs:49-59); here the arithmetic runs.  For an adapted
 * linear with base output b (bias included) and input row x (what the base linear sees, unpermuted), R = rounding to the activation dtype,
 * s = alpha / r in f32 (alpha / sqrt(r) with use_rslora):
 *     t_j = R(sum_k A[j,k] x_k)   u_n = R(sum_j B[n,j] t_j)   v_n = R(s u_n)   y_n = R(R(b_n) + v_n)
 * every sum exact (double over exact products) and rounded once to f32 before R; A [r,K] and B [N,r] are used at their stored values (f16 / bf16 / f32).
 * A row without an adapter gets y = R(b): what its consumer's own rounding gives without a table.  New symbols only: BZ_ABI_VERSION is unchanged.
 *
 * bz_lora_table_create: once, after bz_model_finalize and before any graph capture / engine create that should see it (a second call: BZ_E_INVALID;
 * Mamba2 / DeepSeek-V2: BZ_E_UNSUPPORTED).  The launches a step takes depend on `targets` alone, never on what is attached, so a captured graph stays
 * valid across attach / detach / set: a target un-fuses exactly the launch that hides its input or output (o: attention and o_proj as two launches; gate /
 * up / down: the split MLP; q / k / v: nothing, two launches more per layer).  Both kernels find the adapter through a device-resident table
 * slot -> {layer, target: A, B, r, s} and a device-resident slot id per row (-1: none). */
#define BZ_LORA_Q 1
#define BZ_LORA_K 2
#define BZ_LORA_V 4
#define BZ_LORA_O 8
#define BZ_LORA_GATE 16
#define BZ_LORA_UP 32
#define BZ_LORA_DOWN 64
#define BZ_LORA_ALL 127
typedef struct { int32_t n_slots; /* 1..64 */ int32_t max_rank; /* 1..128 */ uint32_t targets; /* BZ_LORA_* bits */ int32_t reserved[5]; } bz_lora_table_config;
typedef struct bz_lora bz_lora;
int bz_lora_table_create(bz_model* m, const bz_lora_table_config* cfg);
/* An adapter on the device (engine/lora.rs:138-257 LoraAdapter): rank, alpha, then one pair per adapted linear.  key = the module path with the PEFT prefix
 * stripped ("model.layers.3.self_attn.q_proj"); A host [rank, K], B host [N, rank], both of `dtype` (BZ_F16 / BZ_BF16 / BZ_F32).  bz_lora_free of an attached
 * adapter: BZ_E_INVALID. */
int bz_lora_create(bz_device* dev, int rank, float alpha, int use_rslora, bz_lora** out);
int bz_lora_add(bz_lora* a, const char* key, int dtype, const void* A, const int64_t* a_shape, const void* B, const int64_t* b_shape);
int bz_lora_free(bz_lora* a);
/* engine/lora.rs:138-257 rule for rule: `path` = a directory holding adapter_model.safetensors, or the file; optional adapter_config.json beside it gives r,
 * lora_alpha (and use_rslora); the config's rank wins over the first dimension of a lora_A; no or unparseable config: alpha = rank; the "base_model." prefix is
 * stripped, the suffix is ".lora_{A,B}.weight"; an A without a B is skipped; no lora_A at all, or no complete pair, is an error in the reference's words.
 * Beyond the reference, BZ_E_UNSUPPORTED naming the cause: use_dora, bias other than "none", a non-empty modules_to_save, a pair on lm_head / embed_tokens,
 * a pair whose two ranks disagree.  bz_lora_describe is the host-only parse (no device): JSON {"rank", "alpha", "use_rslora", "scaling", "pairs": {key: {"dtype",
 * "rank", "in", "out"}}}, buffer protocol of bz_safetensors_describe. */
int bz_lora_load(bz_device* dev, const char* path, bz_lora** out);
int bz_lora_describe(const char* path, char* json_out, size_t cap, size_t* needed);
/* Registry slots (executor.rs:397-420 LoraAdapterRegistry keeps name -> adapter; the names live in the Python layer).  attach: shapes against the model's
 * linears, targets within the table's mask, rank <= max_rank -- each error names the tensor and the figure; the slot is written by a stream-ordered copy and
 * the adapter is retained until detach.  detach waits for the model's stream; BZ_E_INVALID while the slot is the model's current one or a batch graph row /
 * admitted engine request uses it. */
int bz_lora_attach(bz_model* m, int slot, bz_lora* a);
int bz_lora_detach(bz_model* m, int slot);
/* The single-sequence "current adapter" (executor_generate.rs:49-59 resolves GenerationConfig.lora_adapter per request): a stream-ordered write of a device
 * scalar that every Llama-family step reads -- bz_forward_kv, bz_forward_paged, bz_generate*, the pieces API, captured decode graphs (a graph captured
 * earlier follows on its next replay), prompts.  slot = -1: none. */
int bz_model_set_lora(bz_model* m, int slot);
/* per-row slots (host, N entries, -1 = none) of a batched decode graph: stream-ordered, the next replay reads them */
int bz_decode_batch_graph_set_adapters(bz_batch_graph* g, const int32_t* slots);
/* Op level: the two kernels on rows of one fused group of layer `layer` -- targets = BZ_LORA_Q|K|V (N = the three widths stacked), BZ_LORA_O, BZ_LORA_GATE|UP or
 * BZ_LORA_DOWN.  x F32 [rows, K] (values of the activation dtype), base F32 [rows, N], row_slots host [rows], y_out F32 [rows, N].  form 0: the rows form
 * (x converted to the activation dtype's rows, y updated in place, as the batched path runs it); form 1: the decode form (rows == 1: x through the plain
 * prologue, base read as a VSrc, a fresh output row). */
int bz_lora_apply(bz_model* m, int layer, uint32_t targets, const bz_tensor* x, const bz_tensor* base, const int32_t* row_slots, int rows, int form, bz_tensor* y_out);

/* ---- measurement (methodology of /root/reference/src/cli/bench.rs:24-33,299-306) ----------------------- */
typedef struct { char name[48]; int32_t launches; double total_ms; double algo_bytes; } bz_kernel_time;
/* Runs `iters` eager decode steps (token at position, position+1, ...) with every kernel launched through
 * hipExtLaunchKernelGGL start/stop events on the compute stream and returns, per kernel, launches / summed dispatch time /
 * summed algorithmic bytes.  Durations are pure kernel times (comparable with rocprofv3 --kernel-trace). */
int bz_profile_step(bz_model* m, bz_kv* kv, int64_t token, int position, int iters, bz_kernel_time* out, int max_out, int* n_out);
/* the same for a Mamba2 model (advances `state` by `iters` tokens) */
int bz_profile_step_ssm(bz_model* m, bz_ssm_state* state, int64_t token, int iters, bz_kernel_time* out, int max_out, int* n_out);

/* Kernel tuning aid: mean dispatch time of the int4 GEMV kernel alone on synthetic [N,K] gs-128 weights rotated over `nbuf`
 * HBM buffers.  mode 0 plain x / 1 fused residual+RMSNorm prologue / 2 SiLU*up prologue; flags 0, or 8 = prefetch depth 4 instead of 2
 * (any other bit: BZ_E_INVALID). */
int bz_tune_gemv(bz_device* dev, int N, int K, int groups_per_wg, int mode, int nbuf, int iters, int flags, double* avg_us);

/* the same for the fused MLP kernel (norm + gate/up + SiLU*up + down) on synthetic int4 weights; flags must be 0 and stamps_out NULL
 * (otherwise BZ_E_INVALID) */
int bz_tune_mlp(bz_device* dev, int H, int I, int nbuf, int iters, int flags, double* avg_us, long long* stamps_out);

/* the same for the dense row GEMV (16-bit weights [N,K], wdt BZ_F16 / BZ_BF16); mode 0 plain, 1 residual + RMSNorm prologue, 2 SiLU*up prologue;
 * sk = split-K count (0: the loader's choice) */
int bz_tune_rows(bz_device* dev, int N, int K, int wdt, int mode, int sk, int nbuf, int iters, double* avg_us);

/* Measured HBM read ceiling of this device, GB/s: a streaming read of `bytes` (rotating buffers beyond the Infinity Cache) with the decode
 * kernels' load pattern and no arithmetic.  bench.py reports roofline fractions against the 8 TB/s spec peak AND against this number
 * (SURVEY.md 8d "record the measured peak on the box and report against both"). */
int bz_probe_hbm_read(bz_device* dev, size_t bytes, int iters, double* gbs);

/* ---- op-level entry points (parity tests; each is the kernel the forward path uses) ------------------------ */
/* QuantMatmulOps / dense matmul on a registered weight `name` ("….weight"): y[S,N] = x[S,K] W^T (+bias); x,y F32 device tensors */
int bz_quant_matmul(bz_model* m, const char* name, const bz_tensor* x, int S, bz_tensor* y);
/* Prefill GEMM on the matrix cores: y[S,N] = round16(x)[S,K] . W[N,K]^T, f32 accumulate, result unrounded.  Dense f16 / bf16 weights
 * (K % 64 == 0, x rounded to the weight dtype), or int4 group-quantised weights without act-order (AWQ / GPTQ: x rounded to f16, S >= 9).  The same kernel runs inside bz_forward_kv / bz_forward_paged when a dense 16-bit Llama-family model is given S >= 8 tokens
 * (regular.rs:89-117 bf16 SafeTensors path; boostr's matmul behind LoadedModel::forward_with_kv_cache at executor_generate.rs:357). */
int bz_prefill_matmul(bz_model* m, const char* name, const bz_tensor* x, int S, bz_tensor* y);
/* DequantOps: whole weight -> F32 [N,K] on host (from the REPACKED device layout: validates the repack) */
int bz_dequant(bz_model* m, const char* name, float* host_out);
/* NormalizationOps::rms_norm with optional fused residual: h' = round(h + prev) ; y = w * round(h' * rsqrt(mean(h'^2)+eps)) */
int bz_rms_norm(bz_device* dev, const bz_tensor* x, const bz_tensor* prev /*nullable*/, const bz_tensor* weight, int rows, int n,
                float eps, int act_dtype, bz_tensor* y, bz_tensor* h_out /*nullable*/);
/* RoPE on [S, n_heads, head_dim] F32 in place, positions position..position+S-1, using the model's cos/sin caches (rope_caches()) */
int bz_rope(bz_model* m, bz_tensor* x, int S, int n_heads, int position);
/* ActivationOps/BinaryOps: y = round(round(silu(gate)) * up) */
int bz_silu_mul(bz_device* dev, const bz_tensor* gate, const bz_tensor* up, int64_t n, int act_dtype, bz_tensor* y);
/* single-token attention of q F32 [n_heads, head_dim] over layer `layer` of the cache, first `len` positions */
int bz_attn_decode(bz_model* m, const bz_tensor* q, bz_kv* kv, int layer, int len, bz_tensor* out);
int bz_paged_attn_decode(bz_model* m, const bz_tensor* q, bz_paged_kv* kv, int layer, const bz_tensor* block_table, int len,
                         bz_tensor* out);
/* Batched decode attention (process_decode_batch, engine/batch_decode.rs:35-150).  A decode batch's attention keeps a row's scores in LDS up to scalar_limit
 * positions (38 888 / 18 416 / 8 180 / 3 062 at n_heads / n_kv_heads = 1 / 2 / 4 / 8); beyond, or from BZ_ROWS_SPLIT_MIN positions on, it runs as split-KV
 * over the rows' block tables + merge (head_dim 64 / 128, f16 / bf16 caches).
 * bz_rows_attn_plan: HOST ONLY, needs no device -- what a batch of N rows launches per layer at a decision length of `capacity` positions (the longest live row
 * of an eager step, the capacity of a graph) under a window of `window` keys (0: none).  kernel: 0 scalar, 1 split pair, -1 refused (then the call returns
 * BZ_E_UNSUPPORTED and the message names the limit).  ws_bytes = rows_per_pass * n_heads * grid_slices * (head_dim + 4) * 4, rows_per_pass = min(N, 512,
 * 128 MiB / (n_heads * grid_slices * (head_dim + 4) * 4)): a larger batch passes over its rows in sub-chunks.  BZ_ROWS_SPLIT_MIN is read, as the step reads it.
 * bz_rows_attn_slice_len: HOST ONLY -- positions per slice for a row of `len` keys (inside its window), the rule the device applies: 128, doubled until at
 * most 64 slices cover the row. */
typedef struct bz_rows_attn_plan_t { int kernel; int scalar_limit; int grid_slices; int rows_per_pass; size_t ws_bytes; } bz_rows_attn_plan_t;
int bz_rows_attn_plan(int n_heads, int n_kv_heads, int head_dim, int kv_dtype, int window, int N, int capacity, bz_rows_attn_plan_t* out);
int bz_rows_attn_slice_len(int len);
/* Which path a prompt, a decode batch or a speculative verify takes (DESIGN.md "Which path a prompt takes").
 * bz_prompt_traits_t: what the decision reads of a model, fixed at bz_model_finalize (nothing changes a linear's format afterwards); bz_model_prompt_traits
 * copies it out.  Flags are 0 / 1.  bz_prompt_switches_t: the six environment switches the decision depends on, read once per process.
 * bz_prompt_plan: HOST ONLY, needs no device -- the decision itself, a pure function of (traits, switches, kind, rows, total_len, kv_dtype).  sw == NULL: this
 * process's switches.  rows: prompt rows / sequences of a decode batch / verify rows; total_len: position + rows (decode batch: the longest sequence, or the
 * capacity of a graph); kv_dtype: the cache's element type.  BZ_NO_PF_ATTN_MFMA is read where the attention launcher reads it.
 * New symbols only: BZ_ABI_VERSION is unchanged. */
typedef struct bz_prompt_traits_t {
  int arch, act_dtype;
  int hidden, inter, n_layers, n_heads, n_kv_heads, head_dim, rep;   /* rep = n_heads / n_kv_heads */
  int sliding_window, sliding_window_pattern;                         /* with n_layers: whether every layer has the window */
  /* Llama family */
  int shapes_ok;      /* hidden, n_heads head_dim, inter multiples of 64; head_dim % 8 == 0, 256 % (head_dim / 8) == 0; rep 1 / 2 / 4 / 8 */
  int proj_16;        /* 16-bit activations and every projection one part: dense in the activation dtype, fp8, mxfp4, or int4 without act-order */
  int any_dense;      /* ... and one of them dense, fp8 or mxfp4 */
  int exact_cap;      /* 0: some projection lacks the multi-row int4 form; 1: all have it; 2: all have the integer-MFMA form too */
  int gq_all;         /* every part of every projection a block format without bias, one K per fused linear */
  int gq_max_k;       /* largest K of a fused linear */
  unsigned long long gq_max_n3k;   /* largest N_total * 3 * K of a fused linear (32-bit element offsets of the split GEMM) */
  /* lm_head */
  int head_rows;      /* one dense part with direct f32 output */
  int head_gemm;      /* weight dtype == activation dtype and K % 64 == 0 */
  int spec_head;      /* the multi-row exact lm_head of the speculative verify takes it */
  /* DeepSeek-V2 */
  int mla_q_lora_rank, mla_kv_lora_rank, mla_rope_dim, mla_nope_dim, mla_v_dim;
  int ds_dims_ok;     /* hidden, n_heads v_dim, moe_inter (MoE models) and inter (models with a dense layer) multiples of 64 */
  int ds_weights_act; /* every projection one dense part in the activation dtype, kv_b_proj and the experts too */
  /* Mamba2 */
  int ssm_scan_ok;    /* the in-kernel scan takes head_dim / d_state / n_groups / conv kernel */
  int ssm_groups_ok;  /* d_inner and n_heads divisible by n_groups */
  int ssm_proj_ok;    /* in_proj / out_proj one dense part in the activation dtype, K % 64 == 0 */
} bz_prompt_traits_t;
typedef struct bz_prompt_switches_t {
  int prefill_min;       /* BZ_PREFILL_MIN, default 8 */
  int no_mfma_prefill;   /* BZ_NO_MFMA_PREFILL set */
  int no_gguf_prefill;   /* BZ_NO_GGUF_PREFILL set */
  int exact;             /* BZ_EXACT_PREFILL, default -1: by prompt length */
  int exact_max;         /* BZ_EXACT_PREFILL_MAX, default 16 */
  int exact_i8_max;      /* BZ_EXACT_I8_MAX, default 0 */
} bz_prompt_switches_t;
enum { BZ_PLAN_PROMPT = 0, BZ_PLAN_DECODE_BATCH = 1, BZ_PLAN_VERIFY = 2 };
enum { BZ_ROUTE_STEPS = 0, BZ_ROUTE_ROWS = 1, BZ_ROUTE_DSV2 = 2, BZ_ROUTE_MAMBA = 3 };
enum { BZ_PF_ATTN_NONE = 0, BZ_PF_ATTN_MFMA = 1, BZ_PF_ATTN_SCALAR = 2, BZ_PF_ATTN_SCALAR_EXACT = 3, BZ_PF_ATTN_ROWS = 4 };
enum { BZ_HEAD_STEP = 0, BZ_HEAD_GEMM = 1, BZ_HEAD_GEMV_ROWS = 2, BZ_HEAD_SPEC = 3 };
/* route STEPS: token by token on the decode step (exact 0, attn NONE, head STEP, chunk 0).  exact: 0 MFMA GEMMs, 1 the multi-row exact rows, 2 the exact
 * integer-MFMA GEMMs.  attn ROWS: a decode batch -- scalar or split-KV per layer, by bz_rows_attn_plan.  head GEMM: one MFMA GEMM over a chunk where all its
 * rows are wanted, else as GEMV_ROWS (final norm + lm_head GEMV per wanted row); STEP: the decode step's head per wanted row (quantised lm_head).
 * chunk: rows per pass, 2048 or 512. */
typedef struct bz_prompt_plan_t { int route, exact, attn, head, chunk; } bz_prompt_plan_t;
int bz_model_prompt_traits(const bz_model* m, bz_prompt_traits_t* out);
int bz_prompt_plan(const bz_prompt_traits_t* t, const bz_prompt_switches_t* sw, int kind, int rows, int total_len, int kv_dtype, bz_prompt_plan_t* out);
/* HOST ONLY: what a packed prompt batch of these lengths does.  packed = 1 exactly when bz_prompt_plan(BZ_PLAN_PROMPT, rows = T, total_len = max_len) answers
 * BZ_ROUTE_ROWS -- a query reads at most its own input, so the longest input is the context (and what bounds the scalar attention's LDS); `plan` is that plan.
 * packed = 0: the single-input path once per input; `plan` is then the plan of the longest input alone.  BZ_E_INVALID naming the figure for n_seq <= 0, a
 * length <= 0 and T >= 2^31. */
typedef struct bz_packed_plan_t { int packed, rows, n_seq, max_len; bz_prompt_plan_t plan; } bz_packed_plan_t;
int bz_packed_plan(const bz_prompt_traits_t* t, const bz_prompt_switches_t* sw, const int32_t* seq_lens, int n_seq, int kv_dtype, bz_packed_plan_t* out);
/* HOST ONLY: the two definitions bz_score_batch applies on the host, public for the reason bz_score_row_spec is.  targets: row r reads the next token of its own
 * input, an input's last row -1.  totals: per input, the sum of the logprobs and their count in row order over the scored rows whose logprob is finite. */
int bz_packed_targets_spec(const int64_t* tokens /*[T]*/, const int32_t* seq_lens, int n_seq, int64_t* targets_out /*[T]*/);
int bz_packed_totals_spec(const bz_score_row* rows /*[T]*/, const int32_t* seq_lens, int n_seq, bz_score_total* totals_out /*[n_seq]*/);
/* Which kernels a decode step launches (DESIGN.md "Which kernels a decode step launches").  As above: bz_layer_traits_t is what the decision reads of one
 * layer, fixed at bz_model_finalize but for the two LoRA flags, which bz_lora_table_create sets from the table's mask; bz_step_switches_t the twelve environment
 * switches, read once per process; bz_layer_plan: HOST ONLY, needs no device -- the decision itself, a pure function of (traits, switches, kv_dtype).  The model
 * keeps one plan per layer and cache dtype (F32 / F16 / BF16); the step dispatches on it and decides one thing per call: the short or the long attention form,
 * from the context and BZ_SPLIT_MIN.  A fused linear is described by its parts (at most three).  Flags are 0 / 1.  New symbols only: BZ_ABI_VERSION is unchanged. */
enum { BZ_LIN_NONE = 0, BZ_LIN_Q4G = 1, BZ_LIN_ROWS = 2, BZ_LIN_Q4K = 3, BZ_LIN_Q6K = 4, BZ_LIN_Q80 = 5, BZ_LIN_Q5K = 6, BZ_LIN_Q40 = 7, BZ_LIN_Q41 = 8, BZ_LIN_Q50 = 9,
       BZ_LIN_Q51 = 10, BZ_LIN_F8 = 11, BZ_LIN_MX4 = 12 };
typedef struct bz_linear_traits_t {
  int kind, N, K;        /* BZ_LIN_* */
  int wdt;               /* ROWS: the weights' dtype */
  int gw, sk, npf;       /* k-groups per workgroup, split-K count, weight loads in flight: the layout choices of finalize */
  int act_order, bias;   /* GPTQ act-order permutation / bias present */
} bz_linear_traits_t;
typedef struct bz_fused_traits_t { int n_parts, fix_out; bz_linear_traits_t parts[3]; } bz_fused_traits_t;
typedef struct bz_layer_traits_t {
  int arch, act_dtype, hidden, inter, n_heads, n_kv_heads, head_dim;
  int window;                /* this layer's sliding window (0: full attention) */
  int lora_o, lora_mlp;      /* the LoRA table's mask covers o_proj / one of gate, up, down */
  int down_slabs;            /* the slab-major copy of a dense down_proj exists (k_mlp_dense reads it) */
  bz_fused_traits_t qkv, o, gateup, down;   /* DeepSeek-V2: [q ; kv_a], o_proj, a dense layer's gate/up and down; Mamba2: in_proj and out_proj in qkv and o */
  /* DeepSeek-V2 */
  int mla_x_ok[3];           /* per cache dtype: the exact decode MLA kernels take the shape and the model's longest context */
  int is_moe, e_dt, router_dt, moe_inter, moe_n_experts, moe_slots;   /* moe_slots = top_k + n_shared */
  /* Mamba2 */
  int ssm_d_inner, ssm_n_groups;
} bz_layer_traits_t;
typedef struct bz_step_switches_t {
  int no_slim_qkv, no_gq_slim, no_gq_mix, no_rows2;                          /* BZ_NO_SLIM_QKV, BZ_NO_GQ_SLIM, BZ_NO_GQ_MIX, BZ_NO_ROWS2 set */
  int no_attn_fusion, no_attn_split, no_attn_f32, no_attn2_hd64;             /* BZ_NO_ATTN_FUSION, BZ_NO_ATTN_SPLIT, BZ_NO_ATTN_F32, BZ_NO_ATTN2_HD64 set */
  int no_mlp_fusion, gguf_mlp_fusion, dsv2_f32_sums, no_moe_route_fusion;    /* BZ_NO_MLP_FUSION, BZ_GGUF_MLP_FUSION, BZ_DSV2_F32_SUMS, BZ_NO_MOE_ROUTE_FUSION set */
} bz_step_switches_t;
/* the kernel one GEMV launch takes (NONE: no such part) */
enum { BZ_GEMV_NONE = 0, BZ_GEMV_F8 = 1, BZ_GEMV_Q4G_SLIM = 2, BZ_GEMV_Q4G = 3, BZ_GEMV_ROWS2 = 4, BZ_GEMV_ROWS = 5, BZ_GEMV_GQ_SLIM = 6, BZ_GEMV_GQ = 7, BZ_GEMV_UNSUPPORTED = 8, BZ_GEMV_MX4 = 9 };
/* attention and o_proj: PLAIN = attention, then the o_proj GEMV(s); FUSED_*: one launch (int4 / dense 16-bit / Q4_K o_proj over an f32 cache); SPLIT: split-KV
 * partials + merge + o_proj GEMV; SPLIT_FUSED: split-KV partials + merge with the int4 o_proj */
enum { BZ_ATTN_PLAIN = 0, BZ_ATTN_FUSED_Q4G = 1, BZ_ATTN_FUSED_DENSE = 2, BZ_ATTN_FUSED_Q4K = 3, BZ_ATTN_SPLIT = 4, BZ_ATTN_SPLIT_FUSED = 5 };
/* the kernel behind a plain attention launch: k_attn_decode (one thread per position), k_attn2 (8 waves, 16-bit cache), k_attn2f (f32 cache) */
enum { BZ_ATTN_K_DECODE = 0, BZ_ATTN_K_ATTN2 = 1, BZ_ATTN_K_ATTN2F = 2, BZ_ATTN_K_UNSUPPORTED = 3 };
enum { BZ_MLP_SPLIT = 0, BZ_MLP_Q4G = 1, BZ_MLP_DENSE = 2, BZ_MLP_GQ = 3 };
/* qkv_mix (gateup_mix): a Q4_K part and a Q6_K part -- q/k and v of a Q4_K_M file -- in one slim launch; else qkv[i] per part.  attn_short: the form of a step of at most BZ_SPLIT_MIN keys (of its window, for a
 * windowed layer); attn_long: beyond.  attn_kernel, o[i]: what PLAIN and SPLIT launch.  mlp: a fused form, or SPLIT with gateup[i] and down[i] (filled for every
 * plan: what BZ_MLP_SPLIT would launch).  mla_exact / moe_route_fused / moe_rows2: DeepSeek-V2 -- the exact MLA kernels (else the f32 ones), router logits as
 * a ring GEMV with the top-k inside the gate/up launch (else the router launch), the balanced role kernel for the experts behind the router launch. */
typedef struct bz_layer_plan_t {
  int qkv_mix, qkv[3];
  int attn_short, attn_long, attn_kernel, o[3];
  int mlp, gateup_mix, gateup[3], down[3];
  int mla_exact, moe_route_fused, moe_rows2;
} bz_layer_plan_t;
int bz_model_layer_traits(const bz_model* m, int layer, bz_layer_traits_t* out);
int bz_model_layer_plan(const bz_model* m, int layer, int kv_dtype, bz_layer_plan_t* out);
int bz_layer_plan(const bz_layer_traits_t* t, const bz_step_switches_t* sw, int kv_dtype, bz_layer_plan_t* out);
/* HOST ONLY: the attention form (BZ_ATTN_*) of a step that sees `keys` positions (an eager step: position + 1; a graph: its capacity) on a layer with the given
 * window under BZ_SPLIT_MIN = split_min -- plan->attn_short up to split_min keys, or a window of at most that many, plan->attn_long beyond.  -1: null plan. */
int bz_step_attn_form(const bz_layer_plan_t* plan, int window, int keys, int split_min);
/* op-level twin of bz_paged_attn_decode for a decode batch (engine/batch_decode.rs:35-150): runs the attention the batched step would launch for these rows and
 * returns its 16-bit rows as F32.  q F32 [N, n_heads, hd] roped and rounded, block_table I32 [N, max_blocks], seq_lens HOST i32 [N], out F32 [N, n_heads, hd]. */
int bz_paged_attn_decode_rows(bz_model* m, const bz_tensor* q, bz_paged_kv* kv, int layer, const bz_tensor* block_table, int max_blocks,
                              const int32_t* seq_lens, int N, bz_tensor* out);
/* kv_insert kernel (cuda_graphs.rs:5): write k,v F32 [n_kv_heads, head_dim] at `position` (contiguous) */
int bz_kv_insert(bz_model* m, bz_kv* kv, int layer, int position, const bz_tensor* k, const bz_tensor* v);
/* ConvOps (engine/executor.rs:71) -- Mamba2 layer `layer`: depthwise causal conv1d STEP (+ bias, SiLU) over the raw in_proj row zx = [z | x B C | dt]
 * (F32 device, 2 d_inner + 2 n_groups d_state + n_heads values): xbc_out [d_inner + 2 n_groups d_state] F32; the layer's conv window inside `state`
 * (LayeredSsmState, docs/architecture.md:52-54: conv [conv_dim, k-1]) moves on by this token; the SSM state is not touched. */
int bz_conv1d_step(bz_model* m, int layer, bz_ssm_state* state, const bz_tensor* zx, bz_tensor* xbc_out);
/* The Mamba2 mixer's step as the decode path runs it (one launch: conv1d step + SiLU, h = exp(dt A) h + dt B x, y = C h + D x, gate y * silu(z)):
 * y_out [d_inner] F32 (before the gated RMSNorm); `state` (conv window + SSM state [n_heads, head_dim, d_state]) advances by one token
 * (forward_with_ssm_state, engine/executor_generate.rs:137,148). */
int bz_ssm_step(bz_model* m, int layer, bz_ssm_state* state, const bz_tensor* zx, bz_tensor* y_out);
/* The kernels the batched Mamba2 prompt route runs between the two GEMMs of layer `layer` (conv over the rows, the in-kernel scan over the tokens, the gated
 * RMSNorm), on S caller-provided in_proj rows: zx_rows F32 [S, 2 d_inner + 2 n_groups d_state + n_heads], each row [z | x B C | dt] already rounded to the
 * activation dtype.  xbc_out F32 [S, d_inner + 2 n_groups d_state] (conv + SiLU), y_out F32 [S, d_inner] (the gated y), yn_out F32 [S, d_inner] (the norm's
 * 16-bit rows, expanded; may be NULL; refused for an f32 model, whose prompts never take this route).  `state` advances by S tokens.  Any S >= 1: the
 * 8-token minimum belongs to the route, not to the kernels.  BZ_E_UNSUPPORTED for a state shape the scan does not take. */
int bz_ssm_scan_rows(bz_model* m, int layer, bz_ssm_state* state, const bz_tensor* zx_rows, int S, bz_tensor* xbc_out, bz_tensor* y_out, bz_tensor* yn_out);
/* One layer of a LayeredSsmState copied to the host as F32 (which = 0: SSM state [n_heads * head_dim * d_state], 1: conv window [conv_dim * (k-1)]);
 * n = the expected element count.  Test / debugging aid for the two entry points above (the state layouts are docs/architecture.md:52-54). */
int bz_ssm_state_read(const bz_ssm_state* state, int layer, int which, float* host, size_t n);
/* MoE router of DeepSeek-V2 layer `layer` (docs/architecture.md:108-119: softmax -> greedy top-k -> weights): hidden = the residual stream row [H] F32,
 * the layer's post-attention RMSNorm runs inside (as in the decode step).  sel_out I32 / w_out F32 [top_k + n_shared]: the routed experts in selection
 * order (ties -> lowest index), then the shared experts' slots (index n_experts + j, weight 1); xn_out (optional) F32 [H] the normalised row. */
int bz_moe_route(bz_model* m, int layer, const bz_tensor* hidden, bz_tensor* sel_out, bz_tensor* w_out, bz_tensor* xn_out);
/* Grouped expert GEMV over the stacked expert weights (engine/executor_cache.rs:218-219,344-348): slot s uses expert sel[s] (I32 device, n_slots <= 128).
 * which = 0: gate|up projections, x F32 [H] shared by all slots -> y F32 [n_slots][2 moe_inter];
 * which = 1: down projection with the SiLU(gate) * up prologue, x F32 [n_slots][2 moe_inter] -> y F32 [n_slots][H]. */
int bz_moe_grouped_gemv(bz_model* m, int layer, int which, const bz_tensor* sel, int n_slots, const bz_tensor* x, bz_tensor* y);
/* The exponential every kernel of this library uses (SiLU, softmax weights, sampling): ONE specified sequence of IEEE operations (range reduction by ln2
 * in two fma steps, degree-5 polynomial, exact 2^n scaling; < 1 ulp), evaluated here on the HOST for n values -- the same function body the device code
 * compiles, so a CPU-only test can pin it bit for bit against an independent restatement.  boostr's own exp (ActivationOps / softmax behind
 * executor.rs:67-80) is not visible; any faithful expf is "the" exp, and a specified one makes both sides of a parity test compute the same bits. */
int bz_expf_spec(const float* x, int n, float* y);
/* The E4M3 quantiser an FP8 KV pool would store with (OCP e4m3fn; groundwork, no pool uses it yet -- DESIGN.md section 4 "E4M3 quantiser"), evaluated on the HOST
 * for n values: bytes_out[i] = e4m3(x[i] * 2^-exp) -- multiply by 2^-exp (exact), clamp to +-448 in f32, round to nearest even with subnormals, NaN -> 0x7F --
 * and values_out[i] (nullable) = that byte read back, times 2^exp.  exp in [-5, 7]: inside it every value read back is a normal f16 below 65 504, exact in f16 and
 * in bf16.  Public for the reason bz_expf_spec is: it is the function body device code would compile, so a CPU-only test pins it bit for bit against an
 * independent restatement.  Beyond the reference.  New symbol only: BZ_ABI_VERSION is unchanged. */
int bz_fp8_e4m3_spec(const float* x, int n, int exp, uint8_t* bytes_out, float* values_out);
/* rope_caches() -> (cos, sin) F32 [max_pos, head_dim/2] copied to host */
int bz_rope_caches(bz_model* m, float* cos_host, float* sin_host);

#ifdef __cplusplus
}
#endif
#endif
