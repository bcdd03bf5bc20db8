// bz_internal.h -- internal types of libblazr_hip.so (host + device). Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <string>
#include <vector>
#include <unordered_map>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include "../../include/blazr_hip.h"

// ---------------------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------------------
void bz_set_error(const char* fmt, ...);
#define BZ_FAIL(code, ...) do { bz_set_error(__VA_ARGS__); return (code); } while (0)
#define BZ_HIP(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { \
  bz_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); return BZ_E_HIP; } } while (0)
#define BZ_TRY(expr) do { int rc__ = (expr); if (rc__ != BZ_OK) return rc__; } while (0)
// include/blazr_hip.h: "No C++ exception crosses the boundary" -- every status-returning extern "C" body sits between these two
// (an exception unwinding through extern "C" into a Rust / ctypes caller aborts the host or is undefined behaviour)
#define BZ_API_BEGIN try {
#define BZ_API_END } catch (const std::bad_alloc&) { bz_set_error("out of host memory (std::bad_alloc)"); return BZ_E_OOM; } \
  catch (const std::length_error& e__) { bz_set_error("size out of range (%s)", e__.what()); return BZ_E_OOM; }             \
  catch (const std::exception& e__) { bz_set_error("internal error: %s", e__.what()); return BZ_E_INVALID; }               \
  catch (...) { bz_set_error("internal error: unknown C++ exception"); return BZ_E_INVALID; }

// ---------------------------------------------------------------------------------------------------------
// device-visible PODs
// ---------------------------------------------------------------------------------------------------------
// A vector another kernel produced: plain f32 (already rounded to the activation dtype) or 64-bit fixed point
// (2^-32 units) accumulated by split-K GEMV blocks with integer atomics (exactly associative => deterministic).
struct VSrc { const void* p; int fix; };

enum { PRO_PLAIN = 0, PRO_NORM = 1, PRO_SILU = 2, PRO_GATED = 3, PRO_GATED2 = 4 };
// How a GEMV block builds its activation slice x[k0, k0+KR):
struct Pro {
  int mode;
  VSrc src;            // PLAIN: x[K]; NORM: deferred residual prev[H] (p == nullptr: none); SILU: gate at [0,I), up at [I,2I)
  const float* h_in;   // NORM: residual stream
  float* h_out;        // NORM: h' = R(h + prev), written by block 0 (nullptr: skip)
  const float* norm_w; // NORM
  float eps;
  int H;               // NORM: == K ; SILU: I
  int act;             // activation dtype for rounding (BZ_F32/F16/BF16)
  const int* perm;     // optional: x'[k] = x[perm[k]] (GPTQ act-order)
  int aux;             // GATED / GATED2: number of norm groups
  int aux2;            // GATED2: number of heads (h_in = per-head sums of v^2 from the SSM kernel, src = v = R(y * R(silu z)))
  int f32_sums;        // dense k_gemv_rows2: f32 FMA chains instead of the exact (double) sums -- the DeepSeek-V2 path sets it (k_gemv_rows2's EX)
};

// (the public BZ_LIN_* values: bz_linear_traits_t carries a kind as it is)
enum { LK_NONE = BZ_LIN_NONE, LK_Q4G = BZ_LIN_Q4G, LK_ROWS = BZ_LIN_ROWS, LK_Q4K = BZ_LIN_Q4K, LK_Q6K = BZ_LIN_Q6K, LK_Q80 = BZ_LIN_Q80, LK_Q5K = BZ_LIN_Q5K, LK_Q40 = BZ_LIN_Q40,
       LK_Q41 = BZ_LIN_Q41, LK_Q50 = BZ_LIN_Q50, LK_Q51 = BZ_LIN_Q51, LK_F8 = BZ_LIN_F8, LK_MX4 = BZ_LIN_MX4 };

// Device-resident linear layer in kernel layout.
struct LinearDev {
  int kind = LK_NONE;
  int N = 0, K = 0, gs = 0;
  int wdt = BZ_F16;         // ROWS: weight dtype
  void* w = nullptr;        // Q4G: [N/64][K/32][64 lanes][16 B]; ROWS: [N][K]; F8: [N][K] e4m3 bytes; MX4: [N/4][ceil(K/512)][1088 B] tiles, scales inside (bz_mxfp4.hip); GGUF kinds: see k_gemv_gq (zeros = Q6_K highs, hdr = headers, scales = f16 d)
  void* scales = nullptr;   // Q4G: f16 [N/64][G][64]; F8: f32 [N]
  void* zeros = nullptr;    // Q4G: u8  [N/64][G][64]  (AWQ z, GPTQ z+1); F8: u32 [N/16] row-block arrival counters of the split-K form (zero between launches)
  void* hdr = nullptr;      // K-quants: per-superblock headers
  int* perm = nullptr;      // GPTQ act-order
  float* bias = nullptr;
  int gw = 1;               // groups (of gs) per workgroup (split-K granularity)
  int sk = 1;               // ROWS / F8: split-K count (> 1 => fixed-point accumulator output)
  int npf = 2;              // groups of weight loads kept in flight per wave (2 or 4)
  size_t bytes = 0;         // resident bytes
  size_t algo_bytes = 0;    // minimal on-disk bytes (SURVEY 8d accounting)
  bool owned = true;
};

struct bz_device {
  int id = 0;
  hipStream_t stream = nullptr;
  hipStream_t copy_stream = nullptr;
  hipDeviceProp_t prop;
  std::vector<hipEvent_t> events;
  void* pinned = nullptr; size_t pinned_bytes = 0; // small pinned staging ring
  size_t pinned_off = 0;
  uint64_t event_counter = 0;
  float* scratch = nullptr;   // 4 KiB device scratch (sampling partials)
  void* samp_ws = nullptr;    // non-greedy sampling workspace (bz_sample.hip), grown on demand
  std::mutex mu;              // guards the per-device scratch / sampling workspace / staging ring (concurrent generate() calls share a device)
  int refs = 1;               // the handle itself + every live child object (tensor/model/cache/graph)
};
void bz_dev_retain(bz_device* d);
void bz_dev_release(bz_device* d);

struct bz_tensor {
  bz_device* dev = nullptr;
  void* ptr = nullptr;
  int dtype = BZ_F32;
  std::vector<int64_t> shape;
  size_t nbytes = 0;
  bool owned = true;
};

struct bz_kv {
  bz_device* dev = nullptr;
  int layers = 0, batch = 1, n_kv = 0, cap = 0, max_len = 0, hd = 0, dtype = BZ_F16;
  int seq_len = 0;
  void* k = nullptr; void* v = nullptr;   // [layer][kv_head][cap][hd]
};

struct bz_ssm_state {
  bz_device* dev = nullptr;
  int layers = 0, n_heads = 0, head_dim = 0, d_state = 0, conv_dim = 0, kc = 0, dtype = BZ_BF16;
  void* ssm = nullptr;      // [layers][n_heads][head_dim][d_state] in dtype
  float* conv = nullptr;    // [layers][conv_dim][kc-1] f32 (values representable in the activation dtype)
};

struct bz_paged_kv {
  bz_device* dev = nullptr;
  int layers = 0, num_blocks = 0, block_size = 16, n_kv = 0, hd = 0, dtype = BZ_F16;
  int seq_len = 0;
  void* k = nullptr; void* v = nullptr;   // [layer][block][kv_head][block_size][hd]
};

// how the attention kernel finds K/V rows
struct KvView {
  void* k; void* v;
  int dtype, hd, n_kv;
  int paged;
  long long layer_stride;   // elements between layers
  // contiguous: row(p) = base + ((kvh*cap + p) * hd)
  int cap;
  // paged: row(p) = base + (((block_table[p/bs] * n_kv + kvh) * bs + p%bs) * hd)
  int bs;
  const int* block_table;
  const int* slot;          // paged: write slot for the new token (nullptr: derive from pos via block_table)
};

size_t bz_dtype_size(int dtype);

// OCP E4M3 (e4m3fn, not fnuz) in software, host and device: the quantiser an FP8 KV pool would store with (no pool uses it yet -- DESIGN section 4 "E4M3
// quantiser") and its scalar decode.  stored byte = e4m3(x 2^-exp), value read = e4m3 2^exp.  x 2^-exp is exact, the clamp to +-448 happens in f32 (no conversion
// instruction's overflow mode takes part), rounding is to nearest even with subnormals (units of 2^-9), NaN -> 0x7F.
__host__ __device__ __forceinline__ float bz_pow2f(int e) { const unsigned b = (unsigned)(127 + e) << 23; float f; __builtin_memcpy(&f, &b, 4); return f; }   // -126 <= e <= 127
__host__ __device__ __forceinline__ unsigned bz_fp8_quant(float x, int exp) {
  if (x != x) return 0x7Fu;
  float y = x * bz_pow2f(-exp);
  y = y > 448.f ? 448.f : (y < -448.f ? -448.f : y);
  unsigned u; __builtin_memcpy(&u, &y, 4);
  const unsigned sign = (u >> 24) & 0x80u;
  u &= 0x7fffffffu;
  if (u < 0x3C800000u) {                      // below 2^-6: a multiple of 2^-9 -- one f32 add at 2^14, where an ulp is 2^-9, rounds to nearest even
    float a; __builtin_memcpy(&a, &u, 4);
    a += 16384.f;
    unsigned r; __builtin_memcpy(&r, &a, 4);
    return sign | (r - 0x46800000u);          // 0 .. 8 (8 = the smallest normal number's code)
  }
  u += 0x7FFFFu + ((u >> 20) & 1u);           // three mantissa bits stay
  return sign | ((u >> 20) - (120u << 3));    // exponent bias 127 -> 7; at most 0x7E after the clamp
}
__host__ __device__ __forceinline__ float bz_fp8_dequant(unsigned b, int exp) {
  const unsigned m = b & 0x7Fu;
  float f;
  if (m == 0x7Fu) { const unsigned n = 0x7FC00000u; __builtin_memcpy(&f, &n, 4); return f; }
  if (m < 8u) f = (float)m * 0.001953125f;    // subnormal: m 2^-9
  else { const unsigned u = (m + (120u << 3)) << 20; __builtin_memcpy(&f, &u, 4); }
  f *= bz_pow2f(exp);
  return (b & 0x80u) ? -f : f;
}

// per-launch timing records (bz_profile_step)
struct BzTimingRec { const char* label; double bytes; hipEvent_t e0, e1; };
struct BzTimingSink { std::vector<BzTimingRec> recs; };
void bzk_set_timing_sink(BzTimingSink* s);
BzTimingSink* bzk_timing_sink();
// launch helper: plain launch, or -- while a profile is being taken -- hipExtLaunchKernelGGL with start/stop events bound to the dispatch
// itself (pure kernel time on the launch stream, no inter-kernel gap)
#define BZ_LAUNCH(label, bytes, kernel, grid, block, smem, stream, ...)                                              \
  do {                                                                                                               \
    BzTimingSink* sink__ = bzk_timing_sink();                                                                        \
    if (sink__) {                                                                                                    \
      hipEvent_t e0__, e1__;                                                                                         \
      BZ_HIP(hipEventCreate(&e0__));                                                                                 \
      BZ_HIP(hipEventCreate(&e1__));                                                                                 \
      hipExtLaunchKernelGGL(kernel, grid, block, smem, stream, e0__, e1__, 0, __VA_ARGS__);                          \
      sink__->recs.push_back(BzTimingRec{label, (double)(bytes), e0__, e1__});                                       \
    } else {                                                                                                         \
      hipLaunchKernelGGL(kernel, grid, block, smem, stream, __VA_ARGS__);                                            \
    }                                                                                                                \
  } while (0)

// ---------------------------------------------------------------------------------------------------------
// kernel launchers (bz_kernels.hip)
// ---------------------------------------------------------------------------------------------------------
// Mamba2 side duty of the out_proj GEMV: shift the conv state of channels [ch0, ch0 + n) by this step's raw projection (see k_ssm_step)
struct ConvShift { float* cs; VSrc src; int x_off, ch0, n, kc; };

// MoE form of k_gemv_rows2: n slots, slot s -> expert sel[s] (sel == nullptr: the one dense matrix), its input row and its accumulator row
struct MoeSlots { const int* sel; long long expert_stride; int n; long long src_stride; long long acc_stride; int acc_slots; };

// in-launch MoE routing (k_gemv_rows2<NORM, ROUTE>): lg = the router logits as the fixed-point output of the previous launch
struct RouteArgs { const long long* lg; int E, top_k, n_shared; float routed_scale; int norm_topk; int* sel_out; float* w_out; };

// second (Q6_K) tile range of a mixed-format slim GGUF launch: tiles [nt4, ...) read these arrays with the tile index restarting at 0
struct GqMix { const uint4* Wq6; const uint2* Wh6; const uint4* Hd6; const __half* Dd6; int nt4; };
int bzk_gemv_gq_mix(hipStream_t s, const LinearDev& A, const LinearDev& B, const Pro& pro, const struct GemvOut& out);

struct GemvOut {
  long long* acc;        // Q4G/K-quants: fixed-point accumulator [N] (must be zero on entry)
  float* direct;         // ROWS: direct store [N] (rounded to act)
  long long* zero_buf;   // buffer this launch zeroes for the NEXT accumulate launch (nullptr: none)
  int zero_n;
  float* amax_val; int* amax_idx; // ROWS argmax partials per block (nullptr: off)
  ConvShift shift;       // ROWS: optional side duty (cs == nullptr: none)
};

int bzk_gemv(hipStream_t s, const LinearDev& L, const Pro& pro, const GemvOut& out, int act);
int bzk_gemv_rows_blocks(const LinearDev& L);
bool bzk_gemm_q4g_rows_ok(const LinearDev& L);
bool bzk_gemm_q4g_mfma_ok(const LinearDev& L, int xdt, int rows);   // int4 weights x f16 activations on the matrix cores (rows >= 9)
int bzk_gemm_q4g_mfma(hipStream_t s, const LinearDev& L, const void* x16, int S, int act, float* y, float* ws = nullptr, size_t ws_bytes = 0);   // ws: split-K partials (short prompts)
int bzk_gemm_q4g_rows(hipStream_t s, const LinearDev& L, int xdt, const void* x16, int rows, int act, long long* acc, float* y);
int bzk_rows_choose_sk(int N, int K);
// FP8 (E4M3) weights, one f32 scale per row (bz_fp8.hip): decode GEMV (direct, or split-K with the finish in the launch), W8A16 MFMA GEMM, read-back
int bzk_f8_choose_sk(int N, int K);
int bzk_gemv_f8(hipStream_t s, const LinearDev& L, const Pro& pro, const GemvOut& out, int act);
bool bzk_gemm_f8w_ok(const LinearDev& L, int xdt);
int bzk_gemm_f8w(hipStream_t s, const LinearDev& L, int dt, const void* x16, int S, int act, float* y, float* ws = nullptr, size_t ws_bytes = 0);
int bzk_dequant_f8(hipStream_t s, const LinearDev& L, float* out);
// MXFP4 weights (E2M1 codes, an E8M0 scale per block of 32), in tiles of four rows x 512 k that carry their scales (bz_mxfp4.hip): load-time repack, decode GEMV
// (direct output), W4A16 MFMA GEMM, read-back
size_t bzk_mx4_bytes(int N, int K);
int bzk_repack_mx4(hipStream_t s, const void* q, const void* sc, int N, int K, void* out);
int bzk_gemv_mx4(hipStream_t s, const LinearDev& L, const Pro& pro, const GemvOut& out, int act);
bool bzk_gemm_mx4w_ok(const LinearDev& L, int xdt);
int bzk_gemm_mx4w(hipStream_t s, const LinearDev& L, int dt, const void* x16, int S, int act, float* y, float* ws = nullptr, size_t ws_bytes = 0);
int bzk_dequant_mx4(hipStream_t s, const LinearDev& L, float* out);
int bzk_mlp_gq(hipStream_t s, const LinearDev& gu, const LinearDev& dn, int H, int I, const Pro& pro, long long* acc, long long* zero_buf, int zero_n);
// dense 16-bit form (k_mlp_dense): down_proj additionally stored slab-major [I / 32][H][32] (bzk_repack_down_slabs at finalize)
int bzk_repack_down_slabs(hipStream_t s, const void* w, int H, int I, void* out);
int bzk_mlp_dense(hipStream_t s, const LinearDev& gu, const LinearDev& dn, const void* down_slabs, int H, int I, const Pro& pro, long long* acc, long long* zero_buf, int zero_n);
int bzk_mlp_q4g(hipStream_t s, const LinearDev& gu, const LinearDev& dn, int H, int I, const Pro& pro, long long* acc, long long* zero_buf, int zero_n);   // number of workgroups the ROWS kernel uses (argmax partial count)
int bzk_repack_awq(hipStream_t s, const uint32_t* d_qweight, const float* d_scales, const float* d_zeros, int N, int K, int gs,
                   void* w_out, void* s_out, void* z_out);
int bzk_repack_gptq(hipStream_t s, const uint32_t* d_qweight, const float* d_scales, const uint32_t* d_qzeros, const int* d_perm,
                    const int* d_gidx, int N, int K, int gs, void* w_out, void* s_out, void* z_out);
int bzk_dequant_q4g(hipStream_t s, const LinearDev& L, float* out /*[N][K] device*/);
int bzk_dequant_rows(hipStream_t s, const LinearDev& L, float* out);
int bzk_repack_gq(hipStream_t s, int kind, const void* raw, int N, int K, void* wq, void* wh, void* hd, void* dd);
int bzk_dequant_gq(hipStream_t s, const LinearDev& L, float* out);
// block formats on the batched prompt path: the matrix as three f16 pieces per weight (bz_prefill.hip, k_pf_split3)
bool bzk_gq_split_ok(const LinearDev& L);
int bzk_gq_absmax(hipStream_t s, const LinearDev& L, unsigned* amax);
int bzk_gq_wscale(hipStream_t s, const unsigned* amax, float* wscale);
int bzk_gq_split3(hipStream_t s, const LinearDev& L, const float* wscale, void* out, int row0);
// exact W4 GEMM on the integer matrix cores (bz_prefill.hip: k_gemm_q4g_i8)
bool bzk_gemm_q4g_i8_ok(const LinearDev& L, int xdt);
size_t bzk_pf_quant_i8_bytes(int S, int K, size_t* par_off);
int bzk_pf_quant_i8(hipStream_t s, const void* x16, int S, int K, void* xq);
int bzk_gemm_q4g_i8(hipStream_t s, const LinearDev& L, const void* xq, int S, int act, float* y);
int bzk_pf_split3(hipStream_t s, const float* x, int S, int K, void* xs, float* rscale, const float* wscale);
int bzk_argmax_partials(hipStream_t s, const float* v, long long n, float* pval, int* pidx, int nb);
int bzk_embed(hipStream_t s, const void* table, int tdt, int gg, const long long* tok, int H, int act, float* h_out, const int* pos = nullptr,
              const float* cos_t = nullptr, const float* sin_t = nullptr, int half = 0, float* rope_cur = nullptr);   // rope_cur: stage [cos|sin] of *pos
int bzk_rope_row(hipStream_t s, const int* pos, const float* cos_t, const float* sin_t, int half, float* rope_cur);
int bzk_fix_to_f32(hipStream_t s, const long long* acc, int n, int act, float* out, const float* bias = nullptr, int grid = -1);   // bias: added in f32 to the rounded sum; grid >= 0: the accumulator's units are that dtype's
int bzk_fix_bias(hipStream_t s, long long* acc, const float* bias, int n, int act);   // acc <- R(fix2f(acc) + bias) in place, behind the producer (no-op without a bias)
int bzk_zero64(hipStream_t s, long long* p, int n);

struct AttnArgs {
  VSrc qkv;                 // [nq*hd | nkv*hd | nkv*hd]
  const float* cos_t; const float* sin_t; // [max_pos][hd/2]
  const float* rope_cur;    // [cos hd/2 | sin hd/2] of *pos, staged by bzk_embed / bzk_rope_row (head_dim 128 kernels read this, not the tables)
  int interleaved;
  const int* pos;           // device scalar: position of the new token
  int nq, nkv, hd, act;
  KvView kv; int layer;
  float* out;               // [nq*hd] f32 rounded
  long long* zero_buf; int zero_n;
  int q_only;               // op-level test: q given roped in qkv (plain), no insert, len = *pos
  int window;               // sliding window W of this layer (0: none): the kernels read keys [att_lo(len, W), len) only -- lo is derived on the device from *pos
};
// first key a query sees under a window of W keys (W <= 0: none), len = the query's position + 1
__host__ __device__ __forceinline__ int att_lo(int len, int W) { return W > 0 && len > W ? len - W : 0; }
int bzk_attn_decode(hipStream_t s, const AttnArgs& a);
int bzk_attn_oproj(hipStream_t s, const AttnArgs& a, const LinearDev& L, long long* acc);
// long-context path: split-KV partials + merge (see bz_kernels.hip); ws holds bzk_attn_split_ws_bytes(nq) bytes
int bzk_attn_split_slices(int positions);
size_t bzk_attn_split_ws_bytes(int nq);
int bzk_attn_split(hipStream_t s, const AttnArgs& a, int nsplit, float* ws);
int bzk_attn_merge(hipStream_t s, const AttnArgs& a, const float* ws, int nsplit);
int bzk_attn_merge_oproj(hipStream_t s, const AttnArgs& a, const float* ws, int nsplit, const LinearDev& L, long long* acc);
int bzk_kv_insert(hipStream_t s, const KvView& kv, int layer, const float* k, const float* v, const int* pos, int nkv, int hd);
int bzk_kv_read(hipStream_t s, const KvView& kv, int layer, int kvh, int which, int len, float* out);


// ---------------------------------------------------------------------------------------------------------
// which kernels a decode step launches (bz_step_plan.hip): the process's switches, every "does form X apply" predicate -- one definition each, which the plan
// and the launchers' refusals both call -- and the form of one GEMV launch.  They read plain structs: a flag where the device structs hold a pointer.
// ---------------------------------------------------------------------------------------------------------
#define XQ_NP 8   // activation planes stored per 32-k chunk (bz_dev.h)
struct GemvPro { int mode, H, perm, src_fix, aux; };                  // of a Pro
struct AttnShape { int nq, nkv, hd, kv_dtype, rope_cur, q_only; };     // of an AttnArgs
enum { OUT_ACC = 0, OUT_DIRECT = 1, OUT_AMAX = 2 };                    // of a GemvOut: fixed-point accumulator, direct f32 store, direct store with argmax partials
inline bz_linear_traits_t lin_traits(const LinearDev& L) { return bz_linear_traits_t{L.kind, L.N, L.K, L.wdt, L.gw, L.sk, L.npf, L.perm != nullptr, L.bias != nullptr}; }
inline GemvPro gemv_pro(const Pro& p) { return GemvPro{p.mode, p.H, p.perm != nullptr, p.src.fix, p.aux}; }
inline AttnShape attn_shape(const AttnArgs& a) { return AttnShape{a.nq, a.nkv, a.hd, a.kv.dtype, a.rope_cur != nullptr, a.q_only}; }
inline int out_kind(const GemvOut& o) { return o.amax_val ? OUT_AMAX : o.acc ? OUT_ACC : OUT_DIRECT; }
const bz_step_switches_t* bzk_step_switches();
size_t bzk_mlp_smem(int H);   // LDS of k_mlp_q4g
bool bzk_gemv_slim_ok(const bz_linear_traits_t& L, const GemvPro& p, const bz_step_switches_t& sw);
bool bzk_gq_slim_ok(const bz_linear_traits_t& L, const GemvPro& p, const bz_step_switches_t& sw);
bool bzk_gq_mix_ok(const bz_linear_traits_t& A, const bz_linear_traits_t& B, const GemvPro& p, const bz_step_switches_t& sw);
bool bzk_rows2_enabled(const bz_step_switches_t& sw);
bool bzk_rows2_ok(const bz_linear_traits_t& L, const GemvPro& p, int out, const bz_step_switches_t& sw);
bool bzk_moe_rows2_ok(int wdt, int K, const bz_step_switches_t& sw);   // the balanced role kernel takes the grouped expert GEMVs (16-bit weights)
bool bzk_mlp_fusable(const bz_linear_traits_t& gu, const bz_linear_traits_t& dn, int H, int I);   // (+ f16 activations: checked by the callers)
bool bzk_mlp_dense_fusable(const bz_linear_traits_t& gu, const bz_linear_traits_t& dn, bool down_slabs, int H, int I, int act, const bz_step_switches_t& sw);
bool bzk_mlp_gq_fusable(const bz_linear_traits_t& gu, const bz_linear_traits_t& dn, int H, int I, int act, const bz_step_switches_t& sw);   // GGUF Q4_K gate/up + Q4_K / Q6_K down, f32 activations
int bzk_attn_oproj_plan(const AttnShape& a, const bz_linear_traits_t& L, int& NW);   // int4 o_proj: column slices (0: not applicable) and waves
int bzk_attn2f_oproj_slices(const AttnShape& a, const bz_linear_traits_t& L, const bz_step_switches_t& sw);
int bzk_attn_dense_oproj_loads(const AttnShape& a, const bz_linear_traits_t& L, const bz_step_switches_t& sw);
int bzk_attn_oproj_form(const AttnShape& a, const bz_linear_traits_t& L, const bz_step_switches_t& sw);   // BZ_ATTN_FUSED_*, or BZ_ATTN_PLAIN: fused form not applicable
int bzk_attn_split_ok(const AttnShape& a);
int bzk_attn_merge_oproj_ok(const AttnShape& a, const bz_linear_traits_t& L);
int bzk_attn_kernel(const AttnShape& a, const bz_step_switches_t& sw);   // BZ_ATTN_K_*: the kernel behind bzk_attn_decode
int bzk_att_positions(int positions, int window, int split_min);   // the positions a layer's attention path is sized for (0: the plan's short form)
int bzk_gemv_form(const bz_linear_traits_t& L, const GemvPro& p, int out, int act, const bz_step_switches_t& sw);   // BZ_GEMV_*: the kernel behind bzk_gemv

// final argmax over partials (or full logits) -> token; optionally advance position and publish token
struct FinalArgs {
  const float* pval; const int* pidx; int nparts;   // partials from ROWS kernel
  long long* tok_out;       // next-token buffer (also the embed input of the next step)
  long long* tok_log; int* step; // optional token ring log[*step % logcap] = tok; ++*step
  int logcap;
  int* pos;                 // optional: ++*pos
  long long* zero_buf; int zero_n;
};
int bzk_argmax_final(hipStream_t s, const FinalArgs& a);
int bzk_logits_to_token(hipStream_t s, const float* logits, long long V, const long long* ids, const int* cnts, int n, float rp,
                        float fp, float pp, float temperature, int top_k, float top_p, float min_p, unsigned long long seed,
                        float* scratch /*[V]*/, long long* tok_out);
int bzk_rms_norm(hipStream_t s, const float* x, const float* prev, const float* w, int rows, int n, float eps, int act, float* y,
                 float* h_out);
int bzk_rope(hipStream_t s, float* x, int S, int nh, int hd, int position, const float* cos_t, const float* sin_t, int interleaved,
             int act);
int bzk_silu_mul(hipStream_t s, const float* g, const float* u, long long n, int act, float* y);

// DeepSeek-V2 kernels (MLA attention over the latent cache, MoE router / grouped GEMV / combine)
struct MlaArgs {
  VSrc qkv;                 // [n_heads (nope+rope) | rank | rope]: fused q_proj + kv_a_proj output
  const float* kv_norm; float eps;
  const void* wkvb; int wdt;   // kv_b_proj [n_heads (nope+v)][rank]
  const float* cos_t; const float* sin_t; const int* pos;
  int n_heads, rank, nope, rope, vdim, act;
  KvView kv; int layer;     // n_kv = 1, hd = rank + rope; contiguous or paged
  float* out;               // [n_heads vdim]
  float scale;
  // batched form (prompt rows, grid.y = token): q rows are f32 at qkv.p + token * q_stride, the latent rows of ALL the tokens are already
  // in the cache (bzk_mla_append_rows), token t attends over positions 0 .. pos0 + t, its output goes to out + t * out_stride
  int batch; int pos0; long long q_stride; long long out_stride;
  const float* kva;         // decode with q_lora_rank > 0: [latent | k_pe] of the current token when q comes from a separate projection (else nullptr)
  float* ws; int nsplit;    // decode over context slices (nsplit > 1): [n_heads][nsplit][rank + 2] partials (k_mla_attn<SPLIT> -> k_mla_merge)
};
int bzk_mla_nsplit(int n_heads);
// exact decode MLA (bz_kernels.hip k_mla_scores_x / k_mla_weights_x / k_mla_merge_x): wsd = n_heads * nsplit * (rank + 1) doubles,
// scw = n_heads * nsplit * (ceil(max_len / nsplit) + 1) floats, mxw = n_heads * nsplit floats
bool bzk_mla_x_ok(const MlaArgs& a, int max_len);
int bzk_mla_attn_x(hipStream_t s, const MlaArgs& a, int max_len, double* wsd, float* scw, float* mxw);
// prompt rows: latent RMSNorm + k_pe RoPE of rows s = 0 .. S-1 (source row s at kva + s * stride), appended to the cache at position pos0 + s
int bzk_mla_append_rows(hipStream_t s, const float* kva, long long stride, int S, const float* kv_norm, float eps, int rank, int rope, const float* cos_t, const float* sin_t,
                        int pos0, int act, const KvView& kv, int layer);
// MoE over prompt rows: routing (same arithmetic as the decode router), per-expert row lists, gather, combine
int bzk_moe_route_rows(hipStream_t s, int dt, const void* x16, int S, int H, const void* wr, int wdt, int E, int top_k, float routed_scale, int norm_topk, int* sel, float* wsel);
int bzk_moe_plan_rows(hipStream_t s, const int* sel, int S, int top_k, int E, int* counts, int* offsets, int* row_of, int* tok_of);
int bzk_moe_gather_rows(hipStream_t s, const void* x16, const int* tok_of, int rows, int H, void* xg16);
int bzk_moe_combine_rows(hipStream_t s, const float* ye, const int* row_of, const float* wsel, const float* ysh, int S, int top_k, int H, int act, float* out);
struct MoeGemvArgs {
  const void* w; long long expert_stride;       // elements between experts
  const int* sel;                               // [n_slots] expert index per slot
  int N, K;
  long long src_stride;                         // prologue source: floats between slots (0: shared input)
  float* out; long long out_stride;             // direct output (SPLIT == false)
  long long* acc; long long acc_stride; int acc_slots;   // SPLIT: slot s accumulates into acc[min(s, acc_slots-1)]
  RouteArgs route;                                       // gate / up with in-launch routing (route.lg != nullptr; prologue mode NORM)
};
int bzk_moe_gemv(hipStream_t s, const MoeGemvArgs& g, int wdt, int n_slots, const Pro& pro, int act, bool split, double bytes);
int bzk_mla_attn(hipStream_t s, const MlaArgs& a, int max_len);
size_t bzk_mla_smem(const MlaArgs& a, int max_len);   // LDS of the single-pass kernel at a context of max_len positions (160 KiB: its limit)
int bzk_moe_router(hipStream_t s, const Pro& pro, const void* wr, int wdt, int E, int top_k, int n_shared, float routed_scale, int norm_topk,
                   float* xn_out, int* sel, float* wsel, float* lg_glob, unsigned* counter);
int bzk_moe_combine(hipStream_t s, long long* acc, const float* wsel, int top_k, int has_shared, int H, int act, float* out, long long* zero_buf = nullptr, int zero_n = 0);

// batched prefill for dense 16-bit models (bz_prefill.hip): MFMA GEMM + row-wise norm / RoPE + KV append / causal attention / SiLU*up
int bzk_gemm_nt(hipStream_t s, int dt, const void* x16, const void* w, const float* bias, int S, int N, int K, int act, float* y, float* ws = nullptr, size_t ws_bytes = 0,
                const float* rscale = nullptr);   // ws: split-K partials (optional); rscale: per-row multipliers of the accumulator (split f32 operands)
int bzk_gemm_nt_grouped(hipStream_t s, int dt, const void* x16, const void* w, long long w_stride, int G, const int* g_off, const int* g_cnt, int max_rows, long long total_rows,
                        int N, int K, int act, float* y);
int bzk_pf_cvt16(hipStream_t s, int dt, const float* x, size_t n, void* y);
int bzk_pf_embed(hipStream_t s, const void* table, int tdt, int gg, const long long* tok, int S, int H, int act, float* out);
int bzk_pf_norm(hipStream_t s, int dt, float* hbuf, const float* prev, const float* w, int S, int H, float eps, int act, void* x16);
int bzk_pf_rope_kv(hipStream_t s, float* qkv, int S, int nq, int nkv, int hd, const float* cos_t, const float* sin_t, int interleaved, int pos0, int act,
                   const KvView& kv, int layer, const int* slots, const int* row_pos = nullptr);
int bzk_pf_attn(hipStream_t s, int dt, const float* qkv, int S, int nq, int nkv, int hd, int pos0, int act, const KvView& kv, int layer, void* out16,
                const int* row_pos, int table_stride, int max_len, int form, int window,    // form: BZ_PF_ATTN_* of the plan (bz_route.hip); window: see AttnArgs (every row its own lo)
                const int* seg_lo = nullptr);   // packed prompt batch: device i32 over the whole batch, the packed row at which each row's input starts (positions = packed rows)
int bzk_pf_rope_kv_seg(hipStream_t s, float* qkv, int S, int nq, int nkv, int hd, const float* cos_t, const float* sin_t, int interleaved, int pos0, int act,
                       const KvView& kv, int layer, const int* seg_lo);
// Mamba2 batched prefill (bz_prefill.hip): conv over the prompt rows (+ carried conv state), in-kernel scan over the tokens, gated RMSNorm rows
struct BzSsmScan {
  const float* xbc; int conv_dim; const float* zx; int ld; int dt_off; const float* dt_bias; const float* A_log; const float* D; void* state;
  int n_heads, head_dim, d_state, n_groups, d_inner, act, S; float* y; float* vss;
};
bool bzk_ssm_scan_ok(int head_dim, int d_state, int n_groups, int kc);
int bzk_ssm_scan_pieces(int head_dim);   // vss holds [S][n_heads][pieces]; k_pf_gnorm takes n_heads * pieces
int bzk_pf_conv(hipStream_t s, const float* zx, int ld, int x_off, int conv_dim, int kc, const float* w, const float* b, float* conv_state, int S, int act, float* out);
int bzk_ssm_scan(hipStream_t s, const BzSsmScan& b, int state_dtype);
int bzk_pf_gnorm(hipStream_t s, int dt, const float* v, const float* vss, const float* w, int S, int DI, int G, int NH, float eps, int act, void* x16);
int bzk_pf_silu(hipStream_t s, int dt, const float* gu, int S, int I, int act, void* a16);
size_t bzk_pf_attn_smem(int nq, int nkv, int hd, int len, bool exact = false);
bool bzk_pf_attn_mfma_ok(int hd, int rep);
// decode batches beyond the scalar kernel's LDS limit (bz_rows_attn.hip): split-KV over the rows' block tables + merge
// kernel: 0 = the scalar k_pf_attn, 1 = the split pair, -1 = neither applies (beyond the limit, shape the pair is not built for)
struct BzRowsPlan { int kernel; int scalar_limit; int grid_slices; int rows_per_pass; size_t ws_bytes; };
int bzk_rows_slice_len(int len);
int bzk_rows_split_min();                // BZ_ROWS_SPLIT_MIN, read per call (default: out of reach)
bool bzk_rows_attn_ok(int nq, int nkv, int hd, int kv_dtype);
int bzk_rows_scalar_limit(int nq, int nkv, int hd);
int bzk_rows_attn_plan(int nq, int nkv, int hd, int kv_dtype, int block_size, int window, int N, int capacity, int split_min, BzRowsPlan* out);
int bzk_rows_attn(hipStream_t s, int dt, const float* qkv, int n, int nq, int nkv, int hd, const KvView& kv, int layer, void* out16, const int* row_pos, int table_stride,
                  int window, const BzRowsPlan& plan, float* ws);
int bzk_rows16_to_f32(hipStream_t s, int dt, const void* x16, size_t n, float* y);
// which path a prompt takes (bz_route.hip): the process's switches; bz_prompt_plan itself is public
const bz_prompt_switches_t* bzk_prompt_switches();

// non-greedy sampling (bz_sample.hip)
int bzk_sample(hipStream_t s, void** ws, const float* logits, long long V, const long long* ids, const int* cnts, int n, float rp, float fp, float pp,
               float temperature, int top_k, float top_p, float min_p, unsigned long long seed, long long* tok_out);
int bzk_sample_free(void* ws);
// batched per-row sampler (bz_sample_batch.hip): its 21 launches on stream s; next / log / step (nullable) are the batch graph's feedback buffer [N], pinned
// token log [logcap][N] and step counter -- the last launch writes them as bzk_batch_argmax does
int bzk_batch_sample(hipStream_t s, bz_batch_sampler* bs, const float* logits, long long* tokens_out, long long* next, long long* log, int* step, int logcap);
int bzk_batch_sampler_dims(const bz_batch_sampler* bs, int* N, long long* V);
// per-row logit bias and logprobs (bz_logprobs.hip): state that hangs off the sampler handle (null until bz_batch_sampler_enable) and the three places of a step --
// pre on the raw logits (before the grammar mask), bias after the mask, post after the pick (tokens [N] device; step nullable: the graph's counter, already
// advanced by the pick).  Each launches nothing on a sampler without the flag.
struct BzLpState;
BzLpState*& bzk_batch_sampler_lp(bz_batch_sampler* bs);
bz_device* bzk_batch_sampler_dev(const bz_batch_sampler* bs);
bool bzk_batch_sampler_used(const bz_batch_sampler* bs);        // has sampled or been captured
void bzk_lp_free(BzLpState* lp);
unsigned bzk_lp_flags(bz_batch_sampler* bs);
const bz_logprobs_record* bzk_lp_ring(bz_batch_sampler* bs);   // pinned [LOGCAP][N]; nullptr without BZ_BS_LOGPROBS
void bzk_lp_row_ptrs(bz_batch_sampler* bs /*nullable*/, int** b_cnt, int** top_n);   // device [N] each, nullptr without the flag (k_engine_finish clears a row that ends)
int bzk_lp_pre(hipStream_t s, bz_batch_sampler* bs, const float* logits);
int bzk_lp_bias(hipStream_t s, bz_batch_sampler* bs, float* logits);
int bzk_lp_post(hipStream_t s, bz_batch_sampler* bs, const float* logits, const long long* tokens, const int* step);
int bzk_lp_check_bias(long long V, const uint32_t* ids, const float* vals, int n, std::vector<uint32_t>& ids_out, std::vector<float>& vals_out, const char* who);
size_t bzk_lp_stage_bytes();
int bzk_lp_stage_row(hipStream_t st, bz_batch_sampler* bs, int row, int top_n, const uint32_t* ids, const float* vals, int cnt, void* stage);
// the sink of a score / embed call (bz_score.hip): library-owned buffers that hang off the model (null until the first such call, freed with it).  A call is
// begin (checks made by the caller; grows the buffers -- after a stream synchronise -- and stages the call's parameters), one `chunk` per prompt chunk or per row in
// row order, and end (the one wait of the call).
struct BzSinkWs;
void bzk_sink_free(BzSinkWs* w);
// logits_rows: rows of the F32 [logits_rows][V] workspace a GEMM head writes (0: every head of the call is per-row and scores the model's logits row)
int bzk_score_begin(hipStream_t st, BzSinkWs** w, int S, long long V, int logits_rows, const int64_t* targets_host, int top_n);
float* bzk_score_logits_ws(BzSinkWs* w);
int bzk_score_chunk(hipStream_t st, BzSinkWs* w, const float* logits /*[n][V]*/, int n, int s0);
int bzk_score_end(hipStream_t st, BzSinkWs* w, bz_score_row* rows_out, bz_score_total* total);
// rows: rows of the F32 [rows][H] workspace the final norm writes; two more rows follow it (bzk_pool_step_rows: hidden / prev of a token-by-token step)
int bzk_pool_begin(hipStream_t st, BzSinkWs** w, int S, int H, int rows, const bz_embed_config* cfg);
// a packed batch: seg_off [n_seq + 1] = the inputs' first packed rows, on the host (copied) and on the device (read by the chunks' kernels); out is [n_seq, H]
int bzk_pool_begin_seg(hipStream_t st, BzSinkWs** w, int S, int H, int rows, const bz_embed_config* cfg, const int* seg_off_host, const int* seg_off_dev, int n_seq);
// the lengths of a packed batch, checked (BZ_E_INVALID naming the figure): seg_lo [T] = the packed row at which each row's input starts, seg_off [n_seq + 1], the longest
int bzk_packed_lens(const int32_t* seq_lens, int n_seq, const char* who, std::vector<int>* seg_lo, std::vector<int>* seg_off, int* max_len);
float* bzk_pool_rows_ws(BzSinkWs* w);
void bzk_pool_step_rows(BzSinkWs* w, float** hidden, float** prev);
int bzk_pool_chunk(hipStream_t st, BzSinkWs* w, const float* rows /*[n][H]*/, int n, int s0, float* out);
int bzk_pool_end(hipStream_t st, BzSinkWs* w, float* out);
int bzk_check_score_cfg(const bz_score_config* cfg, const int64_t* targets, int S, long long V, const void* rows_out, const char* who);
int bzk_check_embed_cfg(const bz_embed_config* cfg, const bz_tensor* out, int S, int H, const char* who);
// per-row grammar cursor (bz_grammar.hip): the two launches a captured step takes, on the stream it is captured on
int bzk_grammar_cursor_dims(const bz_grammar_cursor* c, int* N, long long* V, bz_device** dev);
int bzk_grammar_mask_rows(hipStream_t s, bz_grammar_cursor* c, float* logits /*[N,V]*/);
int bzk_grammar_advance_rows(hipStream_t s, bz_grammar_cursor* c, const long long* tokens /*[N]*/);

// Mamba2 kernels
struct SsmArgs {
  VSrc zx;               // raw in_proj output [z | x B C | dt] (f32, or the fixed-point accumulator of a split GEMV)
  int z_off, x_off, dt_off;
  const float* conv_w; const float* conv_b; float* conv_state; int conv_kernel;   // this layer's depthwise conv1d: [conv_dim][kc], [conv_dim], [conv_dim][kc-1]
  const float* dt_bias; const float* A_log; const float* D;
  void* state; int sdt;  // this layer's [n_heads][head_dim][d_state]
  int n_heads, head_dim, d_state, n_groups, d_inner, act;
  float* y;              // [d_inner]
  int gate;              // != 0: y <- R(y * R(silu(z))) and vss[head] <- sum of y^2 (feeds PRO_GATED2)
  float* vss;            // [n_heads]
  float* conv_out;       // op-level entry points only (nullptr in the forward path): the conv1d step's output [x | B | C] (after SiLU, rounded)
  int conv_only;         // op-level bz_conv1d_step: stop after the conv (the SSM state is not touched)
};
int bzk_ssm_step(hipStream_t s, const SsmArgs& a);
int bzk_conv_shift(hipStream_t s, const ConvShift& c, int act);   // shifts the conv state of channels [ch0, ch0 + n) by the projection (the forward path does this inside out_proj's launch)
int bzk_batch_advance(hipStream_t s, long long* tok, const long long* next, int* pos, int* slot, const int* table, int stride, int bs, int N);
int bzk_batch_argmax(hipStream_t s, const float* logits, int V, long long* next, long long* log, int* step, int logcap, int N);

// The batched decode graph (bz_host.hip); the request engine (bz_engine.hip) drives one through its buffers.
struct bz_batch_graph {
  bz_model* m = nullptr; bz_device* dev = nullptr; bz_paged_kv* kv = nullptr;
  bz_batch_sampler* sampler = nullptr;   // borrowed (nullptr: argmax); its logprobs ring is read through the graph
  hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
  int N = 0, max_blocks = 0, capacity = 0;
  long long* tok = nullptr; long long* next = nullptr; int* pos = nullptr; int* slot = nullptr; int* table = nullptr; int* step = nullptr;
  int* row_lora = nullptr; std::vector<int> host_lora;   // LoRA slot id per row (-1: none): device copy the captured step reads, host copy behind it
  bz_tensor* logits = nullptr;        // [N, vocab] of the last replay
  long long* log = nullptr;           // pinned host [LOGCAP][N]
  std::vector<int> host_pos;          // host copy of the positions (limit checks, cache bookkeeping)
  long long replays = 0;
  static const int LOGCAP = 1024;
};
// request engine (bz_engine.hip): the row life cycle of a captured step.  One EngRow per row, device-resident; a live row decodes, an idle row feeds token 0
// at position 0 of its own park block.  status / nlive: pinned host rings [LOGCAP][N] / [LOGCAP] beside the token log.
#define BZ_ENGINE_MAX_STOP 8
struct EngRow { int live, left, n_stop, park_block; long long stop[BZ_ENGINE_MAX_STOP]; };
struct BzEngineRows { EngRow* rows; int* status; int* nlive; };
enum { ENG_IDLE = 0, ENG_TOKEN = 1, ENG_FINISHED = 2 };   // status word: low 2 bits; a finished row's reason (0 length, 1 stop) sits in bits 2..
int bzk_engine_advance(hipStream_t s, long long* tok, const long long* next, int* pos, int* slot, const int* table, int stride, int bs, int N, const EngRow* rows);
int bzk_engine_finish(hipStream_t s, EngRow* rows, const long long* next, int* pos, int* table, int stride, const int* step, int logcap, int N, int* status,
                      int* nlive, uint32_t* gstate /*nullable: the grammar cursor's states*/, int* row_lora /*nullable: a row that ends gets LoRA slot -1*/,
                      int* bias_cnt = nullptr /*nullable: a row that ends gets an empty bias list*/, int* lp_top_n = nullptr /*nullable: ... and logprobs off*/);
// what the engine needs of bz_host.hip: the capture with the row life cycle in it, a launch under the model's lock, the model's device, the prompt workspace
int bzk_kv_copy_slots(hipStream_t s, bz_paged_kv* kv, const int* d_triples, int n, int max_j);
int bzi_engine_capture(bz_model* m, bz_paged_kv* kv, int N, int max_blocks, bz_batch_sampler* s, bz_grammar_cursor* c, const BzEngineRows* er, bz_batch_graph** out);
int bzi_batch_graph_launch(bz_batch_graph* g);
bz_device* bzi_model_device(bz_model* m);
struct BzLoraTable;
BzLoraTable* bzi_model_lora(bz_model* m);   // nullptr: no table
// bz_forward_paged with the model's current LoRA slot set to `slot` for this call alone (one critical section of the model's lock; the scalar is restored)
int bzi_forward_paged_lora(bz_model* m, int slot, const bz_tensor* tokens, int S, bz_paged_kv* kv, const bz_tensor* slot_mapping, const bz_tensor* block_table, int n_blocks,
                           int seq_len_k, int start_pos, bz_tensor* logits_out, uint32_t flags);
int bzi_prefill_reserve(bz_model* m, int rows);
// non-synchronising row writes for the engine: `stage` is pinned host memory the caller keeps untouched until the stream has passed the copies
size_t bzk_batch_sampler_row_bytes();
int bzk_batch_sampler_check_row(const bz_row_sampling* p, const char* who);
int bzk_batch_sampler_stage_row(hipStream_t st, bz_batch_sampler* bs, int row, const bz_row_sampling* p, const int64_t* history, int n_history, int64_t draw_index, void* stage);
uint32_t* bzk_grammar_cursor_states(bz_grammar_cursor* c);
int bzk_grammar_cursor_num_states(const bz_grammar_cursor* c);
int bzk_grammar_cursor_stage_row(hipStream_t st, bz_grammar_cursor* c, int row, uint32_t state, uint32_t* stage /*[2]*/);

// speculative decoding (bz_speculative.hip).  Activation rows of the multi-row lm_head: row r's residual stream at h + r * stride, its deferred
// residual at prev + r * stride (nullptr: none); the final RMSNorm runs as the kernel's prologue, per row
struct SpecHeadRows { const float* h; const float* prev; long long stride; const float* norm_w; float eps; int H; int act; };
bool bzk_spec_head_ok(const LinearDev& L, int act, int H);   // dense 16-bit rows, direct output, f16 activations
int bzk_spec_head_blocks(const LinearDev& L);                // argmax partials per row
// 1 <= R <= 8 rows in one pass over the weights: logits [R][N] (each row the bits of the decode lm_head), argmax partials pval / pidx [R][nb]
int bzk_spec_head(hipStream_t s, const LinearDev& L, const SpecHeadRows& x, int R, float* logits, float* pval, int* pidx, int nb);
int bzk_spec_row_partials(hipStream_t s, const float* logits, int R, long long V, float* pval, int* pidx, int nb);
int bzk_spec_argmax_final(hipStream_t s, const float* pval, const int* pidx, int nb, int R, long long* argmax);
// record [R + 1] = {n_accept, tokens[0 .. n_accept], -1 ...}; next_slot (nullable) <- tokens[n_accept]
int bzk_spec_accept(hipStream_t s, const long long* argmax, const long long* draft, int R, long long* record, long long* next_slot);

// LoRA (bz_lora.hip).  Targets in the order of the BZ_LORA_* bits; the fused linears of a layer are the groups {q,k,v} {o} {gate,up} {down}.
enum { LT_Q = 0, LT_K, LT_V, LT_O, LT_GATE, LT_UP, LT_DOWN, LT_N };
enum { LG_QKV = 0, LG_O, LG_GATEUP, LG_DOWN, LG_N };
struct LoraEnt { const void* A; const void* B; int r; int dt; float s; int pad; };   // one adapted linear of one slot: A [r][K], B [N][r] in dt; r == 0: none
struct LoraSeg { int target, n_off, N; };
struct LoraGroup { int nseg; LoraSeg seg[3]; int K, N; };                             // launch argument: the linears that share x, stacked along N
struct LoraPair { int dt = BZ_F16; int r = 0, K = 0, N = 0; void* A = nullptr; void* B = nullptr; };
struct bz_lora {
  bz_device* dev = nullptr;
  int rank = 0; float alpha = 0.f; int use_rslora = 0; float scale = 0.f;
  std::unordered_map<std::string, LoraPair> pairs;   // key: "model.layers.L.self_attn.q_proj"
  int attached = 0;                                   // slots (of any model) that hold it
};
struct BzLoraTable {
  bz_device* dev = nullptr;
  int n_slots = 0, max_rank = 0, n_layers = 0, t_rows = 0; unsigned mask = 0;
  int K[LT_N] = {0}, N[LT_N] = {0};
  LoraEnt* d_ents = nullptr;         // [n_slots][n_layers][LT_N]
  int* d_cur = nullptr;              // the model's current slot (-1: none)
  float* d_t = nullptr;              // shrink output [t_rows][3][max_rank]
  float* out[LG_N] = {nullptr, nullptr, nullptr, nullptr};   // decode form: the f32 row each group's consumer reads
  void* x16 = nullptr; float* ybuf = nullptr; int* d_slots = nullptr; int op_rows = 0;   // op-level entry (bz_lora_apply) workspace, grown on demand
  std::vector<bz_lora*> slots;       // attached adapters (retained)
  std::vector<std::vector<LoraEnt>> host_ents;   // what each slot's device entries hold (source of the stream-ordered copies)
  std::vector<int> users;            // per slot: batch-graph rows and admitted engine requests that name it
  int cur = -1;
  bool group_on(int g) const { static const unsigned gm[LG_N] = {7u, 8u, 48u, 64u}; return (mask & gm[g]) != 0; }
};
int bzl_table_create(bz_device* dev, const bz_lora_table_config* cfg, int n_layers, const int* K, const int* N, BzLoraTable** out);
void bzl_table_free(BzLoraTable* T);
int bzl_attach(BzLoraTable* T, hipStream_t st, int slot, bz_lora* a);
int bzl_detach(BzLoraTable* T, hipStream_t st, int slot);
int bzl_set_cur(BzLoraTable* T, hipStream_t st, int slot);
LoraGroup bzl_group(const BzLoraTable* T, int g);
// row_slot: device slot id per row (nullptr: every row reads the current-slot scalar)
int bzk_lora_shrink_rows(hipStream_t s, const BzLoraTable* T, int layer, const LoraGroup& g, int act, const void* x16, int rows, const int* row_slot);
int bzk_lora_expand_rows(hipStream_t s, const BzLoraTable* T, int layer, const LoraGroup& g, int act, float* y, int rows, const int* row_slot);
int bzk_lora_shrink_dec(hipStream_t s, const BzLoraTable* T, int layer, const LoraGroup& g, const Pro& pro, const int* row_slot = nullptr);
int bzk_lora_expand_dec(hipStream_t s, const BzLoraTable* T, int layer, const LoraGroup& g, int act, VSrc b, float* out, const int* row_slot = nullptr);
int bzl_apply(BzLoraTable* T, hipStream_t st, int act, int layer, unsigned targets, const bz_tensor* x, const bz_tensor* base, const int32_t* row_slots, int rows, int form,
              bz_tensor* y_out);

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------------
// device-side cross-lane helpers (shared by the kernel files)
// ---------------------------------------------------------------------------------------------------------
// Cross-lane reductions without the LDS permute network (__shfl_xor compiles to ds_bpermute: ~100 clocks a step on the
// latency chain of every prologue).  DPP covers lanes of a 16-lane row (the compiler folds the control into the add),
// V_PERMLANE{16,32}_SWAP (gfx950) cover rows and halves.  Every step is symmetric (both partners form a+b), so all lanes
// of a group end with the same bits.
#define DPP_XOR1 0xB1     // quad_perm [1,0,3,2]
#define DPP_XOR2 0x4E     // quad_perm [2,3,0,1]
#define DPP_HMIRROR 0x141 // row_half_mirror: lane i <- 7 - i   (pairs the two quads of an 8-lane half once quads are uniform)
#define DPP_MIRROR 0x140  // row_mirror:      lane i <- 15 - i  (pairs the two halves of a row once halves are uniform)
typedef unsigned bz_u2_t __attribute__((ext_vector_type(2)));
template <int CTRL> __device__ __forceinline__ int dpp_get(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
template <int CTRL> __device__ __forceinline__ float dpp_get(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true)); }
struct OpAdd { template <class T> __device__ __forceinline__ static T f(T a, T b) { return a + b; } };
struct OpMax { __device__ __forceinline__ static float f(float a, float b) { return fmaxf(a, b); } };
// reduce over aligned groups of N = 4, 8, 16 lanes (result in every lane of the group)
template <int N, class Op, class T>
__device__ __forceinline__ T grp_reduce(T v) {
  v = Op::f(v, dpp_get<DPP_XOR1>(v));
  v = Op::f(v, dpp_get<DPP_XOR2>(v));
  if (N >= 8) v = Op::f(v, dpp_get<DPP_HMIRROR>(v));
  if (N >= 16) v = Op::f(v, dpp_get<DPP_MIRROR>(v));
  return v;
}
// combine lane l with l ^ 16 / l ^ 32 (rows uniform is not required: a true exchange)
template <class Op>
__device__ __forceinline__ float xrow16(float v) {
  const bz_u2_t r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return Op::f(__uint_as_float(r.x), __uint_as_float(r.y));
}
template <class Op>
__device__ __forceinline__ float xrow32(float v) {
  const bz_u2_t r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return Op::f(__uint_as_float(r.x), __uint_as_float(r.y));
}
__device__ __forceinline__ float wave_sum(float v) { return xrow32<OpAdd>(xrow16<OpAdd>(grp_reduce<16, OpAdd>(v))); }
// the same for a double (RMSNorm sums of squares are carried exactly: the oracle defines ss as the rounded exact sum, and a 1e-7 difference
// in 1/rms flips f16 roundings of the normalised vector): the two 32-bit halves travel through the same DPP / permlane controls
template <int CTRL> __device__ __forceinline__ double dpp_get(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xf, 0xf, true), hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, true);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}
__device__ __forceinline__ double wave_sum_d(double v) {
  v += dpp_get<DPP_XOR1>(v); v += dpp_get<DPP_XOR2>(v); v += dpp_get<DPP_HMIRROR>(v); v += dpp_get<DPP_MIRROR>(v);
  {
    const long long b = __double_as_longlong(v);
    const bz_u2_t l = __builtin_amdgcn_permlane16_swap((unsigned)b, (unsigned)b, false, false), h = __builtin_amdgcn_permlane16_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
    v = __longlong_as_double(((long long)h.x << 32) | l.x) + __longlong_as_double(((long long)h.y << 32) | l.y);
  }
  {
    const long long b = __double_as_longlong(v);
    const bz_u2_t l = __builtin_amdgcn_permlane32_swap((unsigned)b, (unsigned)b, false, false), h = __builtin_amdgcn_permlane32_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
    v = __longlong_as_double(((long long)h.x << 32) | l.x) + __longlong_as_double(((long long)h.y << 32) | l.y);
  }
  return v;
}
// sum of a double over aligned groups of N = 8 or 16 lanes (result in every lane of the group)
template <int N> __device__ __forceinline__ double grp_sum_d(double v) {
  v += dpp_get<DPP_XOR1>(v); v += dpp_get<DPP_XOR2>(v); v += dpp_get<DPP_HMIRROR>(v);
  if (N >= 16) v += dpp_get<DPP_MIRROR>(v);
  return v;
}
// deterministic block sum of a double over NW waves (own LDS words; two barriers)
template <int NW> __device__ __forceinline__ double block_sum_d(double v) {
  __shared__ double dred__[NW];
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) dred__[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < NW; w++) t += dred__[w];
  __syncthreads();
  return t;
}
__device__ __forceinline__ float wave_max(float v) { return xrow32<OpMax>(xrow16<OpMax>(grp_reduce<16, OpMax>(v))); }
// lane l with l ^ 16 / l ^ 32 for a double (the attention sums are carried in double: exact products, order-independent to ~1e-16)
__device__ __forceinline__ double xrow16_d(double v) {
  const long long b = __double_as_longlong(v);
  const bz_u2_t l = __builtin_amdgcn_permlane16_swap((unsigned)b, (unsigned)b, false, false), h = __builtin_amdgcn_permlane16_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
  return __longlong_as_double(((long long)h.x << 32) | l.x) + __longlong_as_double(((long long)h.y << 32) | l.y);
}
__device__ __forceinline__ double xrow32_d(double v) {
  const long long b = __double_as_longlong(v);
  const bz_u2_t l = __builtin_amdgcn_permlane32_swap((unsigned)b, (unsigned)b, false, false), h = __builtin_amdgcn_permlane32_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
  return __longlong_as_double(((long long)h.x << 32) | l.x) + __longlong_as_double(((long long)h.y << 32) | l.y);
}

// exp, SPECIFIED: one fixed sequence of IEEE operations (Cephes expf: Cody-Waite reduction by ln2 in two fma steps, degree-5 Horner polynomial,
// exact scaling by 2^n) -- the CPU oracle evaluates the same sequence (oracle/orc_ops.c: orc_expf restates it independently), so SiLU and the
// softmax weights are the same BITS on both sides and a comparison measures structure and rounding points, not two libms (round 2: device
// libm vs glibc flipped ~one f16 rounding per layer, which a layer later is ~2000 one-ulp differences).  < 1 ulp from the true exp;
// 0 below -86 (results stay normal numbers), +inf above 88.  Every multiply-add is an explicit fma: nothing here for a compiler to contract.
__host__ __device__ __forceinline__ float bz_expf(float x) {
  if (x != x) return x;
  if (x < -86.0f) return 0.0f;
  if (x > 88.0f) return __builtin_inff();
  const float n = __builtin_rintf(x * 1.44269504088896341f);
  float r = __builtin_fmaf(n, -0.693145751953125f, x);
  r = __builtin_fmaf(n, -1.42860682030941723212e-6f, r);
  float p = 1.9875691500e-4f;
  p = __builtin_fmaf(p, r, 1.3981999507e-3f);
  p = __builtin_fmaf(p, r, 8.3334519073e-3f);
  p = __builtin_fmaf(p, r, 4.1665795894e-2f);
  p = __builtin_fmaf(p, r, 1.6666665459e-1f);
  p = __builtin_fmaf(p, r, 5.0000001201e-1f);
  const float r2 = r * r;
  float y = __builtin_fmaf(p, r2, r);
  y = y + 1.0f;
  const unsigned sb = (unsigned)((int)n + 127) << 23;   // 2^n, n in [-125, 127]
  float sc;
  __builtin_memcpy(&sc, &sb, 4);
  return y * sc;
}
// f32 -> f16 with the f32 value MATERIALISED first.  Under hipcc's default -ffp-contract=fast the pair "f32 multiply, convert to f16" is fused into
// v_fma_mixlo_f16, which rounds the EXACT product to f16 once; the oracle (and every kernel whose conversion sits behind a run-time dtype switch) rounds the
// product to f32 and then to f16.  The two differ whenever the f32 rounding lands on or crosses an f16 midpoint: measured in round 3 on the slim q/k/v
// kernel (a q/k/v dump hook, since removed), 5 of the 4096 normalised activations of one layer came out as the other f16 neighbour -- which moved every q/k/v column of
// that layer by ~1e-4.  The empty asm makes the operand opaque, so the multiply keeps its own rounding.
__device__ __forceinline__ float f16_round(float x) {
  asm volatile("" : "+v"(x));
  return __half2float(__float2half_rn(x));
}
__device__ __forceinline__ __half f16_cvt(float x) {
  asm volatile("" : "+v"(x));
  return __float2half_rn(x);
}
// Correctly rounded f32 quotient / square root through double (53 >= 2 * 24 + 2 bits: the double result rounds to the correctly rounded float).  Written out
// because hipcc does not always give `a / b` and `1.0f / sqrtf(x)` the IEEE sequence: measured in round 3 (a q/k/v dump hook, since removed), the slim q/k/v kernel's
// 1 / rms came out ONE ULP LOW next to the generic kernel's (same source expression) -- five of 4096 normalised activations then round to the other f16
// neighbour, and every q/k/v column of the layer is off by ~1e-4.  The oracle's C expressions (IEEE division and sqrtf) are these values.
__host__ __device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }
__host__ __device__ __forceinline__ float sqrt_rn(float x) { return (float)sqrt((double)x); }
__host__ __device__ __forceinline__ float rms_scale(float ss, float n, float eps) { return div_rn(1.0f, sqrt_rn(div_rn(ss, n) + eps)); }   // 1 / sqrt(ss / n + eps), each step rounded to f32
// RoPE pair: the products are exact in double (x: <= 24 significant bits, table entry: 24), one rounding of their difference / sum in double and
// one to f32 -- the same bits whatever gets contracted (oracle: orc_rope_apply)
__device__ __forceinline__ float rope_lo(float x0, float x1, float c, float s) { return (float)((double)x0 * (double)c - (double)x1 * (double)s); }
__device__ __forceinline__ float rope_hi(float x0, float x1, float c, float s) { return (float)((double)x1 * (double)c + (double)x0 * (double)s); }
#endif  // __HIPCC__
