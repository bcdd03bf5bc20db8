// bz_step_plan.hip -- which kernels a decode step launches (DESIGN.md "Which kernels a decode step launches").  Plain C++: no kernel, no HIP call -- the twelve
// switches, every "does form X apply" predicate of the decode kernels (one definition each: the plan asks them, and the launchers in bz_kernels.hip refuse by
// them), the form of one GEMV launch (bzk_gemv is a switch over it), and bz_layer_plan: a pure function of one layer's traits (bz_layer_traits_t, filled at
// finalize and again when a LoRA table is made), the switches and the cache dtype, so that tests/test_step_plan.py can sweep it without a device.  The step
// functions in bz_host.hip dispatch on the model's plans; the one thing they decide per call is the short or the long attention form.
#include <cstdlib>

#include "bz_internal.h"

// the twelve switches the step depends on, read once per process
const bz_step_switches_t* bzk_step_switches() {
  static const bz_step_switches_t sw = [] {
    auto set = [](const char* name) { return getenv(name) != nullptr ? 1 : 0; };
    bz_step_switches_t s;
    s.no_slim_qkv = set("BZ_NO_SLIM_QKV"); s.no_gq_slim = set("BZ_NO_GQ_SLIM"); s.no_gq_mix = set("BZ_NO_GQ_MIX"); s.no_rows2 = set("BZ_NO_ROWS2");
    s.no_attn_fusion = set("BZ_NO_ATTN_FUSION"); s.no_attn_split = set("BZ_NO_ATTN_SPLIT"); s.no_attn_f32 = set("BZ_NO_ATTN_F32"); s.no_attn2_hd64 = set("BZ_NO_ATTN2_HD64");
    s.no_mlp_fusion = set("BZ_NO_MLP_FUSION"); s.gguf_mlp_fusion = set("BZ_GGUF_MLP_FUSION"); s.dsv2_f32_sums = set("BZ_DSV2_F32_SUMS");
    s.no_moe_route_fusion = set("BZ_NO_MOE_ROUTE_FUSION");
    return s;
  }();
  return &sw;
}

// ---------------------------------------------------------------------------------------------------------
// GEMV forms
// ---------------------------------------------------------------------------------------------------------
bool bzk_gemv_slim_ok(const bz_linear_traits_t& L, const GemvPro& p, const bz_step_switches_t& sw) {
  return !sw.no_slim_qkv && L.kind == LK_Q4G && !L.act_order && p.mode == PRO_NORM && !p.perm && L.K == p.H && (L.K == 2048 || L.K == 4096 || L.K == 8192) && L.N % 64 == 0 &&
         L.N <= 16384;
}
static bool gq_kind(int kind) { return kind == LK_Q4K || kind == LK_Q5K || kind == LK_Q6K || kind == LK_Q40 || kind == LK_Q41 || kind == LK_Q50 || kind == LK_Q51; }
bool bzk_gq_slim_ok(const bz_linear_traits_t& L, const GemvPro& p, const bz_step_switches_t& sw) {
  if (sw.no_gq_slim || !gq_kind(L.kind) || p.perm || L.N % 64 || L.K % 256) return false;
  if (p.mode == PRO_NORM) return L.K == p.H && (L.K == 2048 || L.K == 4096 || L.K == 8192);
  if (p.mode == PRO_SILU) return L.K == p.H;
  return false;
}
// Q4_K tiles followed by Q6_K tiles (one K, one prologue) in ONE slim launch: the Q4_K_M rule stores q / k as Q4_K and v as Q6_K, which made q/k/v two launches
bool bzk_gq_mix_ok(const bz_linear_traits_t& A, const bz_linear_traits_t& B, const GemvPro& p, const bz_step_switches_t& sw) {
  return A.kind == LK_Q4K && B.kind == LK_Q6K && A.K == B.K && !A.bias && !B.bias && p.mode == PRO_NORM && bzk_gq_slim_ok(A, p, sw) && bzk_gq_slim_ok(B, p, sw);
}
bool bzk_rows2_enabled(const bz_step_switches_t& sw) { return !sw.no_rows2; }
// the balanced role kernel (k_gemv_rows2) takes every fixed-point-output dense GEMV with 16-bit weights
bool bzk_rows2_ok(const bz_linear_traits_t& L, const GemvPro& p, int out, const bz_step_switches_t& sw) {
  if (!bzk_rows2_enabled(sw) || L.kind != LK_ROWS || L.sk <= 1 || out != OUT_ACC) return false;
  if (L.wdt != BZ_F16 && L.wdt != BZ_BF16) return false;
  if (L.K % 8 || L.K > 131072 || p.perm) return false;
  if (p.mode == PRO_NORM) return p.H == L.K && p.H % 8 == 0;
  if (p.mode == PRO_GATED2) return !p.src_fix && (p.aux <= 8) && p.H == L.K && (p.H / (p.aux > 0 ? p.aux : 1)) % 4 == 0;
  return p.mode == PRO_PLAIN || p.mode == PRO_SILU;
}
bool bzk_moe_rows2_ok(int wdt, int K, const bz_step_switches_t& sw) { return bzk_rows2_enabled(sw) && (wdt == BZ_F16 || wdt == BZ_BF16) && K % 8 == 0 && K <= 131072; }

// the kernel behind one bzk_gemv launch; the order of the tests is the order the launcher has always had
int bzk_gemv_form(const bz_linear_traits_t& L, const GemvPro& p, int out, int act, const bz_step_switches_t& sw) {
  if (L.kind == LK_F8) return BZ_GEMV_F8;
  if (L.kind == LK_MX4) return BZ_GEMV_MX4;
  if (L.kind == LK_Q4G) return act == BZ_F16 && bzk_gemv_slim_ok(L, p, sw) ? BZ_GEMV_Q4G_SLIM : BZ_GEMV_Q4G;
  if (L.kind == LK_ROWS) return bzk_rows2_ok(L, p, out, sw) ? BZ_GEMV_ROWS2 : BZ_GEMV_ROWS;
  if (bzk_gq_slim_ok(L, p, sw)) return BZ_GEMV_GQ_SLIM;
  if (L.kind == LK_Q80 || gq_kind(L.kind)) return BZ_GEMV_GQ;
  return BZ_GEMV_UNSUPPORTED;
}

// ---------------------------------------------------------------------------------------------------------
// fused MLP forms
// ---------------------------------------------------------------------------------------------------------
size_t bzk_mlp_smem(int H) { return (size_t)(H >> 5) * XQ_NP * 16 + (size_t)(H >> 7) * 32 + 16 * 128 * 8 + 2 * XQ_NP * 16 + 32 + 16 * 8 + 64; }   // planes, gpar, part, apl, apar, dred, counters
bool bzk_mlp_fusable(const bz_linear_traits_t& gu, const bz_linear_traits_t& dn, int H, int I) {
  return gu.kind == LK_Q4G && dn.kind == LK_Q4G && !gu.act_order && !dn.act_order && gu.N == 2 * I && gu.K == H && dn.N == H && dn.K == I &&
         (H == 2048 || H == 4096) && I % 128 == 0 && bzk_mlp_smem(H) <= 64 * 1024;   // (+ f16 activations: checked by the callers)
}
bool bzk_mlp_dense_fusable(const bz_linear_traits_t& gu, const bz_linear_traits_t& dn, bool down_slabs, int H, int I, int act, const bz_step_switches_t& sw) {
  return !sw.no_mlp_fusion && down_slabs && gu.kind == LK_ROWS && dn.kind == LK_ROWS && gu.wdt == dn.wdt && (gu.wdt == BZ_F16 || gu.wdt == BZ_BF16) && gu.N == 2 * I &&
         gu.K == H && dn.N == H && dn.K == I && H % 512 == 0 && H >= 1024 && H <= 2048 && I % 32 == 0 && I / 32 >= 128 && gu.sk > 1 && dn.sk > 1 && (act == BZ_F16 || act == BZ_BF16 || act == BZ_F32);
}
bool bzk_mlp_gq_fusable(const bz_linear_traits_t& gu, const bz_linear_traits_t& dn, int H, int I, int act, const bz_step_switches_t& sw) {
  // opt-in: measured on the Mistral-7B Q4_K_M shape the fused launch takes 31.0 us against ~19 + ~11 us for the two slim launches (535.6 vs 549.0 tok/s, same
  // box): the block formats cost ~2.5 VALU operations per weight (AND-unpack + three-plane V_DOT4 + a per-32-k epilogue of scale / min arithmetic), ~19 us
  // of issue per CU when 224 workgroups carry all of it -- the fused form serialises that behind its stream, the slim launches spread it over 256 CUs
  const bool on = sw.gguf_mlp_fusion && !sw.no_mlp_fusion;
  return on && act == BZ_F32 && gu.kind == LK_Q4K && (dn.kind == LK_Q4K || dn.kind == LK_Q6K) && !gu.act_order && !dn.act_order && gu.N == 2 * I && gu.K == H && dn.N == H && dn.K == I &&
         (H == 2048 || H == 4096) && I % 256 == 0 && I % 64 == 0;
}

// ---------------------------------------------------------------------------------------------------------
// attention forms
// ---------------------------------------------------------------------------------------------------------
// int4 o_proj: picks the column-slice count so that nq * CS ~ 256 workgroups, and the wave count (8 waves halve the per-wave attention chain);
// returns 0 when the fused form does not apply
int bzk_attn_oproj_plan(const AttnShape& a, const bz_linear_traits_t& L, int& NW) {
  NW = 0;
  if (a.hd != 128 || L.kind != LK_Q4G || L.act_order || L.K != a.nq * 128 || a.q_only) return 0;
  const int NT = L.N / 64;
  for (int nw = 8; nw >= 4; nw >>= 1) {
    const int ow = nw > 8 ? 8 : nw;
    for (int cs = 8; cs >= 1; cs >>= 1)
      if (NT % (cs * ow) == 0 && NT / (cs * ow) <= 2 && a.nq * cs <= 1024) { NW = nw; return cs; }
  }
  return 0;
}
// the f32-cache form (GGUF models): Q4_K o_proj, one tile per wave, CS = N / 512 column slices; single-launch contexts only (no split-KV path for the f32 cache)
int bzk_attn2f_oproj_slices(const AttnShape& a, const bz_linear_traits_t& L, const bz_step_switches_t& sw) {
  if (sw.no_attn_f32 || a.hd != 128 || a.kv_dtype != BZ_F32 || !a.rope_cur || a.q_only || L.kind != LK_Q4K || L.K != a.nq * 128 || L.N % 512 || L.K % 256) return 0;
  const int cs = L.N / 512;
  return a.nq * cs <= 2048 ? cs : 0;
}
// dense 16-bit o_proj in the cache dtype (Llama-3.2-1B: head_dim 64, N 2048): 8 column slices, RPL rows per wave-wide load, 1..4 loads per wave
int bzk_attn_dense_oproj_loads(const AttnShape& a, const bz_linear_traits_t& L, const bz_step_switches_t& sw) {
  if (sw.no_attn2_hd64 || L.kind != LK_ROWS || L.wdt != a.kv_dtype || (a.kv_dtype != BZ_F16 && a.kv_dtype != BZ_BF16) || (a.hd != 64 && a.hd != 128) || a.q_only || !a.rope_cur) return 0;
  if (L.K != a.nq * a.hd || a.nq * 8 > 2048) return 0;
  const int rpl = 512 / a.hd, per_wave = L.N / 64;          // 8 slices x 8 waves
  if (L.N % 64 || per_wave % rpl) return 0;
  const int loads = per_wave / rpl;
  return (loads == 1 || loads == 2 || loads == 4) ? loads : 0;
}
// the single launch of attention + o_proj that takes the shape (BZ_ATTN_FUSED_*), or BZ_ATTN_PLAIN: none does
int bzk_attn_oproj_form(const AttnShape& a, const bz_linear_traits_t& L, const bz_step_switches_t& sw) {
  if (a.kv_dtype == BZ_F32) return bzk_attn2f_oproj_slices(a, L, sw) > 0 ? BZ_ATTN_FUSED_Q4K : BZ_ATTN_PLAIN;
  if (L.kind == LK_ROWS) return bzk_attn_dense_oproj_loads(a, L, sw) > 0 ? BZ_ATTN_FUSED_DENSE : BZ_ATTN_PLAIN;
  int nw; return bzk_attn_oproj_plan(a, L, nw) > 0 ? BZ_ATTN_FUSED_Q4G : BZ_ATTN_PLAIN;
}
int bzk_attn_split_ok(const AttnShape& a) {
  const int rep = a.nkv > 0 ? a.nq / a.nkv : 0;
  return a.hd == 128 && (a.kv_dtype == BZ_F16 || a.kv_dtype == BZ_BF16) && !a.q_only && a.nq % a.nkv == 0 && (rep == 1 || rep == 2 || rep == 4 || rep == 8) && a.rope_cur;
}
int bzk_attn_merge_oproj_ok(const AttnShape& a, const bz_linear_traits_t& L) { int nw; return bzk_attn_oproj_plan(a, L, nw) > 0 && nw == 8; }
// the kernel behind a plain attention launch: the 8-wave lane = (row, 8-element piece) kernel for a 16-bit cache at head_dim 128, and 64 (Llama-3.2-1B) with
// 8 rows per wave-wide load; its f32-cache twin at head_dim 128; else one thread per position
int bzk_attn_kernel(const AttnShape& a, const bz_step_switches_t& sw) {
  if ((a.hd == 128 || (a.hd == 64 && a.rope_cur && !sw.no_attn2_hd64)) && a.kv_dtype != BZ_F32) return BZ_ATTN_K_ATTN2;
  if (a.hd == 128 && a.kv_dtype == BZ_F32 && a.rope_cur && !sw.no_attn_f32) return BZ_ATTN_K_ATTN2F;
  return a.hd == 64 || a.hd == 128 ? BZ_ATTN_K_DECODE : BZ_ATTN_K_UNSUPPORTED;
}

// ---------------------------------------------------------------------------------------------------------
// the plan of one layer
// ---------------------------------------------------------------------------------------------------------
namespace {
// What run_fused launches for a fused linear under the prologue p.  Returns 1 for the one mixed launch -- GGUF Q4_K_M gives q/k/v as a Q4_K part (q, k) and a
// Q6_K part (v), which one slim launch takes (a norm prologue only: bzk_gq_mix_ok) -- and fills forms: each part with its own act-order permutation, into the ring
int fused_forms(const bz_fused_traits_t& F, GemvPro p, int act, const bz_step_switches_t& sw, int* forms) {
  const int mix = !sw.no_gq_mix && F.n_parts == 2 && F.fix_out && bzk_gq_mix_ok(F.parts[0], F.parts[1], p, sw);
  for (int i = 0; i < 3; i++) {
    if (i < F.n_parts) p.perm = F.parts[i].act_order;
    forms[i] = i < F.n_parts ? bzk_gemv_form(F.parts[i], p, OUT_ACC, act, sw) : BZ_GEMV_NONE;
  }
  return mix;
}

void plan_llama(const bz_layer_traits_t& t, const bz_step_switches_t& sw, int kv_dtype, bz_layer_plan_t* p) {
  const int H = t.hidden, I = t.inter, act = t.act_dtype;
  const GemvPro norm{PRO_NORM, H, 0, 0, 0}, plain{PRO_PLAIN, 0, 0, 0, 0}, silu{PRO_SILU, I, 0, 0, 0};
  p->qkv_mix = fused_forms(t.qkv, norm, act, sw, p->qkv);

  // attention + o_proj.  The step stages the position's RoPE row for every layer (rope_cur) and never runs q_only
  const AttnShape a{t.n_heads, t.n_kv_heads, t.head_dim, kv_dtype, 1, 0};
  const bz_linear_traits_t& O = t.o.parts[0];
  const bool fuse_shape = !sw.no_attn_fusion && !t.lora_o && t.o.n_parts == 1 && t.o.fix_out;   // an o_proj adapter reads the attention output: two launches
  p->attn_short = fuse_shape ? bzk_attn_oproj_form(a, O, sw) : BZ_ATTN_PLAIN;
  // long contexts: split-KV attention merged with the o_proj where that form exists (int4); otherwise split-KV attention and a separate o_proj launch -- the
  // fused single-launch kernel reads the context once per column slice, which only pays while the context is short.
  // ODDITY, kept as found: where no split pair exists at the shape (head_dim 64, an f32 cache, a GQA group of 3) the long form is still not the short one -- it
  // leaves the fused launch for plain attention and the o_proj GEMV (Llama-3.2-1B bf16 at position 269 under BZ_SPLIT_MIN=4: attn_decode + gemv_rows2).
  const bool split = !sw.no_attn_split && bzk_attn_split_ok(a);
  const bool merge_fused = fuse_shape && O.kind == LK_Q4G && bzk_attn_merge_oproj_ok(a, O);
  p->attn_long = !split ? BZ_ATTN_PLAIN : merge_fused ? BZ_ATTN_SPLIT_FUSED : BZ_ATTN_SPLIT;
  p->attn_kernel = bzk_attn_kernel(a, sw);
  fused_forms(t.o, plain, act, sw, p->o);

  // norm + gate/up + SiLU*up + down in one launch where one of its three forms takes the layer; a gate / up / down adapter takes the split MLP
  p->mlp = BZ_MLP_SPLIT;
  if (!sw.no_mlp_fusion && !t.lora_mlp && t.gateup.n_parts == 1 && t.down.n_parts == 1) {
    const bz_linear_traits_t& GU = t.gateup.parts[0]; const bz_linear_traits_t& DN = t.down.parts[0];
    if (act == BZ_F16 && bzk_mlp_fusable(GU, DN, H, I)) p->mlp = BZ_MLP_Q4G;
    else if (bzk_mlp_dense_fusable(GU, DN, t.down_slabs, H, I, act, sw)) p->mlp = BZ_MLP_DENSE;   // the dense 16-bit form of the same fusion (slab-major down_proj copy)
    else if (bzk_mlp_gq_fusable(GU, DN, H, I, act, sw)) p->mlp = BZ_MLP_GQ;   // the GGUF form (Q4_K gate / up, Q4_K or Q6_K down, f32 activations)
  }
  p->gateup_mix = fused_forms(t.gateup, norm, act, sw, p->gateup);
  fused_forms(t.down, silu, act, sw, p->down);
}

void plan_dsv2(const bz_layer_traits_t& t, const bz_step_switches_t& sw, int kv_dtype, bz_layer_plan_t* p) {
  const int H = t.hidden, MI = t.moe_inter, act = t.act_dtype;
  const GemvPro norm{PRO_NORM, H, 0, 0, 0}, plain{PRO_PLAIN, 0, 0, 0, 0}, silu{PRO_SILU, t.inter, 0, 0, 0};
  p->qkv_mix = fused_forms(t.qkv, norm, act, sw, p->qkv);
  fused_forms(t.o, plain, act, sw, p->o);
  // exact decode (16-bit models): every sum as the oracle defines it, one maximum over the whole context (BZ_DSV2_F32_SUMS=1: the f32 kernels)
  p->mla_exact = !sw.dsv2_f32_sums && (act == BZ_F16 || act == BZ_BF16) && t.mla_x_ok[kv_dtype];
  if (!t.is_moe) {
    p->gateup_mix = fused_forms(t.gateup, norm, act, sw, p->gateup);
    fused_forms(t.down, silu, act, sw, p->down);
    return;
  }
  // router logits as one more fixed-point GEMV of the ring with the top-k in the prologue of the gate / up launch; else the router launch, and behind it the
  // balanced role kernel (fixed-point accumulators both times) when the expert weights are 16-bit, else the 16-row workgroup form
  p->moe_rows2 = bzk_moe_rows2_ok(t.e_dt, H, sw) && bzk_moe_rows2_ok(t.e_dt, MI, sw);
  p->moe_route_fused = !sw.no_moe_route_fusion && p->moe_rows2 && bzk_moe_rows2_ok(t.router_dt, H, sw) && t.moe_n_experts <= 1024 && t.moe_slots <= 128;
}

void plan_mamba(const bz_layer_traits_t& t, const bz_step_switches_t& sw, bz_layer_plan_t* p) {
  const GemvPro norm{PRO_NORM, t.hidden, 0, 0, 0}, gated{PRO_GATED2, t.ssm_d_inner, 0, 0, t.ssm_n_groups};
  p->qkv_mix = fused_forms(t.qkv, norm, t.act_dtype, sw, p->qkv);     // in_proj
  fused_forms(t.o, gated, t.act_dtype, sw, p->o);        // out_proj
}
}  // namespace

// The one decision a step takes per call: short or long.  positions: what the step was sized for beyond BZ_SPLIT_MIN, 0 below it (eager steps: position + 1;
// a graph: its capacity).  A windowed layer reads min(len, W) keys: its choice is made on that many positions, so a long context with a window that fits the
// single-pass kernel goes back to it (both sides of W give the same choice).  Returns the positions the layer's path is sized for, 0: the short form.
int bzk_att_positions(int positions, int window, int split_min) {
  if (window <= 0) return positions;
  const int keys = positions < window ? positions : window;
  return keys > split_min ? keys : 0;
}
// (returns a form, not a status: nothing in it can throw)
extern "C" int bz_step_attn_form(const bz_layer_plan_t* p, int window, int keys, int split_min) { return !p ? -1 : bzk_att_positions(keys > split_min ? keys : 0, window, split_min) == 0 ? p->attn_short : p->attn_long; }

extern "C" int bz_layer_plan(const bz_layer_traits_t* t, const bz_step_switches_t* sw, int kv_dtype, bz_layer_plan_t* out) {
  BZ_API_BEGIN
  if (!t || !out || (kv_dtype != BZ_F32 && kv_dtype != BZ_F16 && kv_dtype != BZ_BF16)) BZ_FAIL(BZ_E_INVALID, "layer_plan: bad argument");
  for (const bz_fused_traits_t* F : {&t->qkv, &t->o, &t->gateup, &t->down}) if (F->n_parts < 0 || F->n_parts > 3) BZ_FAIL(BZ_E_INVALID, "layer_plan: a fused linear has 0 .. 3 parts");
  if (!sw) sw = bzk_step_switches();
  *out = bz_layer_plan_t{};
  if (t->arch == BZ_ARCH_LLAMA) {
    if (t->o.n_parts < 1 || t->n_kv_heads <= 0) BZ_FAIL(BZ_E_INVALID, "layer_plan: a Llama-family layer has an o_proj and KV heads");
    plan_llama(*t, *sw, kv_dtype, out);
  }
  else if (t->arch == BZ_ARCH_DEEPSEEK2) plan_dsv2(*t, *sw, kv_dtype, out);
  else if (t->arch == BZ_ARCH_MAMBA2) plan_mamba(*t, *sw, out);
  else BZ_FAIL(BZ_E_INVALID, "layer_plan: arch %d", t->arch);
  return BZ_OK;
  BZ_API_END
}
