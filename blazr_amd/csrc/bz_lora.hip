// bz_lora.hip -- LoRA adapters on the decode and the batched path (include/blazr_hip.h "LoRA adapters"; DESIGN.md section 4 "LoRA").
//
//   y_n = R(R(b_n) + R(s * R(sum_j B[n,j] * R(sum_k A[j,k] x_k))))      R = rounding to the activation dtype, every sum exact
//
// Two kernels between existing launches, no change to any of them:
//   k_lora_shrink   t[row][seg][j] = R(A_seg[j,:] . x_row) for every A-row of a GROUP of linears that share x (q/k/v, gate/up): one wave per A-row,
//                   16-byte loads, products exact in double, wave_sum_d.  K is 256 .. 14336 and r is small: latency-bound, K is not split.
//                   Decode form: x from a Pro through the generic GEMVs' own prologue (build_x_simple: the bits of x are the base launch's).
//                   Rows form: the 16-bit / f32 activation rows the batched path already holds.
//   k_lora_expand   per output n the r-long dot with t (staged once per workgroup), then the three roundings.  Decode form: b from a VSrc, a plain f32 row
//                   out (rows without an adapter get R(b): the consumer now reads this row).  Rows form: y in place, rows without an adapter return early.
// Both find the adapter through the device-resident table slot -> {layer, target: A, B, r, s} and a device-resident slot id per row: neither is a launch
// argument, so a captured graph follows attach / detach / set.  The grids depend on the table's mask and max_rank alone.
#include "bz_internal.h"
#include "bz_dev.h"

#include <string.h>

#define LORA_MAX_RANK 128

__device__ __forceinline__ LoraSeg seg_at(const LoraGroup& g, int i) { return i == 0 ? g.seg[0] : (i == 1 ? g.seg[1] : g.seg[2]); }

// eight consecutive elements of a row stored as dt, as f32 (i is a multiple of 8: 16-byte aligned loads)
__device__ __forceinline__ void ld8(const void* p, int dt, size_t i, float (&v)[8]) {
  if (dt == BZ_F32) {
    const float4 a = *(const float4*)((const float*)p + i), b = *(const float4*)((const float*)p + i + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
    const uint4 u = *(const uint4*)((const unsigned short*)p + i);
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int e = 0; e < 4; e++) {
      if (dt == BZ_F16) unpack2<BZ_F16>(w[e], v[2 * e], v[2 * e + 1]); else unpack2<BZ_BF16>(w[e], v[2 * e], v[2 * e + 1]);
    }
  }
}
__device__ __forceinline__ float ld1(const void* p, int dt, size_t i) {
  if (dt == BZ_F32) return ((const float*)p)[i];
  const unsigned short h = ((const unsigned short*)p)[i];
  return dt == BZ_F16 ? __half2float(__ushort_as_half(h)) : __uint_as_float((unsigned)h << 16);
}

// grid (nseg * ceil(max_rank / 4), rows), 256 threads: a workgroup = four A-rows of one segment.  DEC: one row, x built in LDS (K floats) from the Pro.
template <bool DEC>
__global__ __launch_bounds__(256) void k_lora_shrink(const LoraEnt* __restrict__ ents, int n_slots, int ents_per_slot, int layer, LoraGroup g, const int* __restrict__ slot_ptr,
                                                     int slot_stride, int max_rank, int act, const void* __restrict__ x16, Pro pro, float* __restrict__ t) {
  extern __shared__ float xs[];
  __shared__ float red[16];
  const int row = blockIdx.y, bps = (max_rank + 3) >> 2;
  const int slot = slot_ptr[(size_t)row * slot_stride];
  if (slot < 0 || slot >= n_slots) return;
  const int si = blockIdx.x / bps, j0 = (blockIdx.x % bps) * 4;
  const LoraSeg sg = seg_at(g, si);
  const LoraEnt e = ents[(size_t)slot * ents_per_slot + layer * LT_N + sg.target];
  if (j0 >= e.r) return;                       // workgroup-uniform: nothing of this segment's adapter lives here
  const int K = g.K;
  if (DEC) build_x_simple<false>(pro, 0, K, xs, red, false);   // ends with a barrier
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = j0 + wave;
  if (j >= e.r) return;
  const size_t arow = (size_t)j * K;
  double acc = 0.0;
  for (int k = lane * 8; k < K; k += 512) {
    float a[8], x[8];
    ld8(e.A, e.dt, arow + k, a);
    if (DEC) {
      const float4 x0 = *(const float4*)(xs + k), x1 = *(const float4*)(xs + k + 4);
      x[0] = x0.x; x[1] = x0.y; x[2] = x0.z; x[3] = x0.w; x[4] = x1.x; x[5] = x1.y; x[6] = x1.z; x[7] = x1.w;
    } else {
      ld8(x16, act, (size_t)row * K + k, x);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) acc += (double)a[i] * (double)x[i];     // each product is exact in double (at most 24 + 24 significant bits)
  }
  acc = wave_sum_d(acc);
  if (lane == 0) t[((size_t)row * 3 + si) * max_rank + j] = round_act((float)acc, act);
}

// grid (ceil(N / 256), rows), 256 threads
template <bool DEC>
__global__ __launch_bounds__(256) void k_lora_expand(const LoraEnt* __restrict__ ents, int n_slots, int ents_per_slot, int layer, LoraGroup g, const int* __restrict__ slot_ptr,
                                                     int slot_stride, int max_rank, int act, const float* __restrict__ t, VSrc b, float* __restrict__ y) {
  __shared__ float ts[3 * LORA_MAX_RANK];
  const int row = blockIdx.y, tid = threadIdx.x;
  const int slot = slot_ptr[(size_t)row * slot_stride];
  const bool on = slot >= 0 && slot < n_slots;
  if (!DEC && !on) return;                     // rows form: y already holds R(b)
  const LoraEnt* es = ents + (size_t)(on ? slot : 0) * ents_per_slot + layer * LT_N;
  if (on) {
    for (int i = tid; i < g.nseg * max_rank; i += 256) {
      const int si = i / max_rank, j = i - si * max_rank;
      ts[i] = j < es[seg_at(g, si).target].r ? t[((size_t)row * 3 + si) * max_rank + j] : 0.f;
    }
  }
  __syncthreads();
  const int n = blockIdx.x * 256 + tid;
  if (n >= g.N) return;
  const int si = (g.nseg > 2 && n >= g.seg[2].n_off) ? 2 : ((g.nseg > 1 && n >= g.seg[1].n_off) ? 1 : 0);
  const LoraSeg sg = seg_at(g, si);
  float* yp = y + (DEC ? 0 : (size_t)row * g.N) + n;
  const float bv = DEC ? vsrc_get(b, n, act) : *yp;                   // R(b)
  float out = bv;
  if (on) {
    const LoraEnt e = es[sg.target];
    if (e.r > 0) {
      const size_t brow = (size_t)(n - sg.n_off) * e.r;
      const float* tj = ts + si * max_rank;
      double u = 0.0;
      for (int j = 0; j < e.r; j++) u += (double)ld1(e.B, e.dt, brow + j) * (double)tj[j];
      const float uf = round_act((float)u, act);
      const float v = round_act(__fmul_rn(e.s, uf), act);             // the f32 product is materialised, then rounded (bz_internal.h: f16_round)
      out = round_act(__fadd_rn(bv, v), act);
    }
  }
  *yp = out;
}

// ---------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------
// adapter bytes a launch reads under the model's current slot (profile records; rows with their own slot ids are not known to the host)
static double group_bytes(const BzLoraTable* T, int layer, const LoraGroup& g, bool shrink) {
  if (T->cur < 0 || T->host_ents[T->cur].empty()) return 0.0;
  double b = 0.0;
  for (int i = 0; i < g.nseg; i++) {
    const LoraEnt& e = T->host_ents[T->cur][(size_t)layer * LT_N + g.seg[i].target];
    b += (double)e.r * (shrink ? g.K : g.seg[i].N) * bz_dtype_size(e.dt);
  }
  return b;
}
static int check_group(const BzLoraTable* T, int layer, const LoraGroup& g, int rows) {
  if (!T || layer < 0 || layer >= T->n_layers || g.nseg < 1 || g.nseg > 3 || g.K <= 0 || g.K % 8 || g.N <= 0) BZ_FAIL(BZ_E_INVALID, "lora launch: bad layer %d / group (K %d, N %d)", layer, g.K, g.N);
  if (rows < 1 || rows > T->t_rows) BZ_FAIL(BZ_E_INVALID, "lora launch: %d rows, the table's workspace holds %d", rows, T->t_rows);
  return BZ_OK;
}

int bzk_lora_shrink_rows(hipStream_t s, const BzLoraTable* T, int layer, const LoraGroup& g, int act, const void* x16, int rows, const int* row_slot) {
  BZ_TRY(check_group(T, layer, g, rows));
  const dim3 grid(g.nseg * ((T->max_rank + 3) / 4), rows);
  BZ_LAUNCH("lora_shrink", group_bytes(T, layer, g, true), k_lora_shrink<false>, grid, dim3(256), 0, s, T->d_ents, T->n_slots, T->n_layers * LT_N, layer, g,
            row_slot ? row_slot : T->d_cur, row_slot ? 1 : 0, T->max_rank, act, x16, Pro{}, T->d_t);
  return BZ_OK;
}
int bzk_lora_expand_rows(hipStream_t s, const BzLoraTable* T, int layer, const LoraGroup& g, int act, float* y, int rows, const int* row_slot) {
  BZ_TRY(check_group(T, layer, g, rows));
  const dim3 grid((g.N + 255) / 256, rows);
  BZ_LAUNCH("lora_expand", group_bytes(T, layer, g, false), k_lora_expand<false>, grid, dim3(256), 0, s, T->d_ents, T->n_slots, T->n_layers * LT_N, layer, g,
            row_slot ? row_slot : T->d_cur, row_slot ? 1 : 0, T->max_rank, act, T->d_t, VSrc{nullptr, 0}, y);
  return BZ_OK;
}
int bzk_lora_shrink_dec(hipStream_t s, const BzLoraTable* T, int layer, const LoraGroup& g, const Pro& pro, const int* row_slot) {
  BZ_TRY(check_group(T, layer, g, 1));
  const size_t smem = (size_t)g.K * 4;
  if (smem > 64 * 1024) BZ_FAIL(BZ_E_UNSUPPORTED, "lora shrink: an input of %d values does not fit the prologue's 64 KiB of LDS", g.K);
  if ((pro.mode == PRO_NORM && pro.H != g.K) || (pro.mode != PRO_NORM && pro.mode != PRO_SILU && pro.mode != PRO_PLAIN)) BZ_FAIL(BZ_E_INVALID, "lora shrink: prologue mode %d / H %d", pro.mode, pro.H);
  const dim3 grid(g.nseg * ((T->max_rank + 3) / 4), 1);
  BZ_LAUNCH("lora_shrink", group_bytes(T, layer, g, true), k_lora_shrink<true>, grid, dim3(256), smem, s, T->d_ents, T->n_slots, T->n_layers * LT_N, layer, g,
            row_slot ? row_slot : T->d_cur, 0, T->max_rank, pro.act, (const void*)nullptr, pro, T->d_t);
  return BZ_OK;
}
int bzk_lora_expand_dec(hipStream_t s, const BzLoraTable* T, int layer, const LoraGroup& g, int act, VSrc b, float* out, const int* row_slot) {
  BZ_TRY(check_group(T, layer, g, 1));
  const dim3 grid((g.N + 255) / 256, 1);
  BZ_LAUNCH("lora_expand", group_bytes(T, layer, g, false), k_lora_expand<true>, grid, dim3(256), 0, s, T->d_ents, T->n_slots, T->n_layers * LT_N, layer, g,
            row_slot ? row_slot : T->d_cur, 0, T->max_rank, act, T->d_t, b, out);
  return BZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// table
// ---------------------------------------------------------------------------------------------------------
static const char* const kTargetName[LT_N] = {"q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"};
static const int kGroupFirst[LG_N] = {LT_Q, LT_O, LT_GATE, LT_DOWN}, kGroupCount[LG_N] = {3, 1, 2, 1};

LoraGroup bzl_group(const BzLoraTable* T, int gi) {
  LoraGroup g{};
  g.nseg = kGroupCount[gi]; g.K = T->K[kGroupFirst[gi]];
  int off = 0;
  for (int i = 0; i < g.nseg; i++) { const int t = kGroupFirst[gi] + i; g.seg[i] = LoraSeg{t, off, T->N[t]}; off += T->N[t]; }
  g.N = off;
  return g;
}

int bzl_table_create(bz_device* dev, const bz_lora_table_config* cfg, int n_layers, const int* K, const int* N, BzLoraTable** out) {
  if (cfg->n_slots < 1 || cfg->n_slots > 64) BZ_FAIL(BZ_E_INVALID, "lora table: n_slots %d outside 1..64", cfg->n_slots);
  if (cfg->max_rank < 1 || cfg->max_rank > LORA_MAX_RANK) BZ_FAIL(BZ_E_INVALID, "lora table: max_rank %d outside 1..%d", cfg->max_rank, LORA_MAX_RANK);
  if (cfg->targets == 0 || (cfg->targets & ~(unsigned)BZ_LORA_ALL)) BZ_FAIL(BZ_E_INVALID, "lora table: targets 0x%x is not a non-empty set of BZ_LORA_* bits", cfg->targets);
  for (int i = 0; i < 5; i++) if (cfg->reserved[i]) BZ_FAIL(BZ_E_INVALID, "lora table: reserved[%d] must be 0", i);
  std::unique_ptr<BzLoraTable> T(new BzLoraTable());
  T->dev = dev; T->n_slots = cfg->n_slots; T->max_rank = cfg->max_rank; T->mask = cfg->targets; T->n_layers = n_layers; T->t_rows = 2048;   // the batched path's largest chunk
  for (int i = 0; i < LT_N; i++) { T->K[i] = K[i]; T->N[i] = N[i]; if (K[i] % 8) BZ_FAIL(BZ_E_UNSUPPORTED, "lora table: %s input width %d is not a multiple of 8", kTargetName[i], K[i]); }
  const size_t ne = (size_t)T->n_slots * n_layers * LT_N;
  auto alloc = [&](void** p, size_t bytes) -> int {
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) BZ_FAIL(BZ_E_OOM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    return BZ_OK;
  };
  int rc = BZ_OK;
  void* p = nullptr;
  if ((rc = alloc(&p, ne * sizeof(LoraEnt))) == BZ_OK) { T->d_ents = (LoraEnt*)p; if (hipMemset(p, 0, ne * sizeof(LoraEnt)) != hipSuccess) rc = BZ_E_HIP; }
  if (rc == BZ_OK && (rc = alloc(&p, 16)) == BZ_OK) { T->d_cur = (int*)p; const int none = -1; if (hipMemcpy(p, &none, 4, hipMemcpyHostToDevice) != hipSuccess) rc = BZ_E_HIP; }
  if (rc == BZ_OK && (rc = alloc(&p, (size_t)T->t_rows * 3 * T->max_rank * 4)) == BZ_OK) T->d_t = (float*)p;
  for (int g = 0; rc == BZ_OK && g < LG_N; g++)
    if (T->group_on(g) && (rc = alloc(&p, (size_t)bzl_group(T.get(), g).N * 4)) == BZ_OK) T->out[g] = (float*)p;
  if (rc != BZ_OK) { BzLoraTable* raw = T.release(); bzl_table_free(raw); if (rc == BZ_E_HIP) bz_set_error("lora table: device initialisation failed"); return rc; }
  T->slots.assign(T->n_slots, nullptr);
  T->host_ents.assign(T->n_slots, std::vector<LoraEnt>());
  T->users.assign(T->n_slots, 0);
  bz_dev_retain(dev);
  *out = T.release();
  return BZ_OK;
}

void bzl_table_free(BzLoraTable* T) {
  if (!T) return;
  for (bz_lora* a : T->slots) if (a) a->attached--;
  hipFree(T->d_ents); hipFree(T->d_cur); hipFree(T->d_t); hipFree(T->x16); hipFree(T->ybuf); hipFree(T->d_slots);
  for (int g = 0; g < LG_N; g++) hipFree(T->out[g]);
  if (!T->slots.empty()) bz_dev_release(T->dev);     // (a table that failed half-way never retained the device)
  delete T;
}

// "model.layers.<L>.self_attn.q_proj" -> (L, target); false for anything else
static bool parse_key(const std::string& key, int* layer, int* target) {
  // (PEFT wraps a *ForCausalLM: its keys read "base_model.model.model.layers...", which the reference's prefix rule leaves as "model.model.layers...")
  static const char pre[] = "model.layers.";
  size_t i = key.compare(0, 12, "model.model.") ? 0 : 6;
  if (key.compare(i, sizeof(pre) - 1, pre)) return false;
  i += sizeof(pre) - 1;
  const size_t d0 = i;
  long l = 0;
  while (i < key.size() && key[i] >= '0' && key[i] <= '9' && i - d0 < 6) l = l * 10 + (key[i++] - '0');
  if (i == d0 || i >= key.size() || key[i] != '.') return false;
  const std::string rest = key.substr(i + 1);
  for (int t = 0; t < LT_N; t++)
    if (rest == std::string(t <= LT_O ? "self_attn." : "mlp.") + kTargetName[t]) { *layer = (int)l; *target = t; return true; }
  return false;
}

int bzl_attach(BzLoraTable* T, hipStream_t st, int slot, bz_lora* a) {
  if (slot < 0 || slot >= T->n_slots) BZ_FAIL(BZ_E_INVALID, "lora attach: slot %d outside 0..%d", slot, T->n_slots - 1);
  if (T->slots[slot]) BZ_FAIL(BZ_E_INVALID, "lora attach: slot %d is occupied (detach it first)", slot);
  if (a->dev != T->dev) BZ_FAIL(BZ_E_INVALID, "lora attach: the adapter lives on another device handle");
  if (a->pairs.empty()) BZ_FAIL(BZ_E_INVALID, "lora attach: the adapter holds no pair");
  std::vector<LoraEnt> ents((size_t)T->n_layers * LT_N, LoraEnt{nullptr, nullptr, 0, BZ_F16, 0.f, 0});
  for (const auto& kv : a->pairs) {
    int layer, target;
    const LoraPair& p = kv.second;
    if (!parse_key(kv.first, &layer, &target)) BZ_FAIL(BZ_E_UNSUPPORTED, "lora attach: '%s' is not a linear of a Llama-family layer (model.layers.N.{self_attn,mlp}.*_proj)", kv.first.c_str());
    if (layer >= T->n_layers) BZ_FAIL(BZ_E_INVALID, "lora attach: '%s' names layer %d, the model has %d", kv.first.c_str(), layer, T->n_layers);
    if (!(T->mask >> target & 1u)) BZ_FAIL(BZ_E_INVALID, "lora attach: '%s' adapts %s, which is outside the table's targets 0x%x", kv.first.c_str(), kTargetName[target], T->mask);
    if (p.r > T->max_rank) BZ_FAIL(BZ_E_INVALID, "lora attach: '%s' has rank %d, the table's max_rank is %d", kv.first.c_str(), p.r, T->max_rank);
    if (p.K != T->K[target]) BZ_FAIL(BZ_E_INVALID, "lora attach: '%s.lora_A' has %d input features, the model's %s takes %d", kv.first.c_str(), p.K, kTargetName[target], T->K[target]);
    if (p.N != T->N[target]) BZ_FAIL(BZ_E_INVALID, "lora attach: '%s.lora_B' has %d output features, the model's %s gives %d", kv.first.c_str(), p.N, kTargetName[target], T->N[target]);
    ents[(size_t)layer * LT_N + target] = LoraEnt{p.A, p.B, p.r, p.dt, a->scale, 0};
  }
  T->host_ents[slot] = std::move(ents);       // kept until the slot is written again: the source of the copy below
  const size_t bytes = T->host_ents[slot].size() * sizeof(LoraEnt);
  BZ_HIP(hipMemcpyAsync(T->d_ents + (size_t)slot * T->n_layers * LT_N, T->host_ents[slot].data(), bytes, hipMemcpyHostToDevice, st));
  T->slots[slot] = a; a->attached++;
  return BZ_OK;
}

int bzl_detach(BzLoraTable* T, hipStream_t st, int slot) {
  if (slot < 0 || slot >= T->n_slots) BZ_FAIL(BZ_E_INVALID, "lora detach: slot %d outside 0..%d", slot, T->n_slots - 1);
  if (!T->slots[slot]) BZ_FAIL(BZ_E_INVALID, "lora detach: slot %d is empty", slot);
  if (T->cur == slot) BZ_FAIL(BZ_E_INVALID, "lora detach: slot %d is the model's current adapter (bz_model_set_lora(-1) first)", slot);
  if (T->users[slot] > 0) BZ_FAIL(BZ_E_INVALID, "lora detach: slot %d is used by %d batch row(s) / admitted request(s)", slot, T->users[slot]);
  BZ_HIP(hipStreamSynchronize(st));
  const size_t bytes = (size_t)T->n_layers * LT_N * sizeof(LoraEnt);
  BZ_HIP(hipMemsetAsync(T->d_ents + (size_t)slot * T->n_layers * LT_N, 0, bytes, st));
  BZ_HIP(hipStreamSynchronize(st));
  T->host_ents[slot].clear();
  T->slots[slot]->attached--; T->slots[slot] = nullptr;
  return BZ_OK;
}

__global__ void k_lora_set_int(int* p, int v) { p[0] = v; }
int bzl_set_cur(BzLoraTable* T, hipStream_t st, int slot) {
  if (slot < -1 || slot >= T->n_slots) BZ_FAIL(BZ_E_INVALID, "set_lora: slot %d outside -1..%d", slot, T->n_slots - 1);
  if (slot >= 0 && !T->slots[slot]) BZ_FAIL(BZ_E_INVALID, "set_lora: slot %d is empty", slot);
  hipLaunchKernelGGL(k_lora_set_int, dim3(1), dim3(1), 0, st, T->d_cur, slot);
  BZ_HIP(hipGetLastError());
  T->cur = slot;
  return BZ_OK;
}

// op-level entry: the two kernels on caller-given rows of one group
int bzl_apply(BzLoraTable* T, hipStream_t st, int act, int layer, unsigned targets, const bz_tensor* x, const bz_tensor* base, const int32_t* row_slots, int rows, int form,
              bz_tensor* y_out) {
  int gi = -1;
  static const unsigned gm[LG_N] = {7u, 8u, 48u, 64u};
  for (int g = 0; g < LG_N; g++) if (targets == gm[g]) gi = g;
  if (gi < 0) BZ_FAIL(BZ_E_INVALID, "lora_apply: targets 0x%x is not one fused group (q|k|v, o, gate|up, down)", targets);
  if (!T->group_on(gi)) BZ_FAIL(BZ_E_INVALID, "lora_apply: no target of group 0x%x is in the table's mask 0x%x", targets, T->mask);
  const LoraGroup g = bzl_group(T, gi);
  if (layer < 0 || layer >= T->n_layers) BZ_FAIL(BZ_E_INVALID, "lora_apply: layer %d outside 0..%d", layer, T->n_layers - 1);
  if (rows < 1 || rows > T->t_rows || (form != 0 && form != 1) || (form == 1 && rows != 1)) BZ_FAIL(BZ_E_INVALID, "lora_apply: rows %d / form %d (decode form: one row)", rows, form);
  if (x->dtype != BZ_F32 || base->dtype != BZ_F32 || y_out->dtype != BZ_F32 || x->nbytes != (size_t)rows * g.K * 4 || base->nbytes != (size_t)rows * g.N * 4 || y_out->nbytes != base->nbytes)
    BZ_FAIL(BZ_E_INVALID, "lora_apply: x must be F32 [%d, %d], base and y_out F32 [%d, %d]", rows, g.K, rows, g.N);
  for (int r = 0; r < rows; r++)
    if (row_slots[r] < -1 || row_slots[r] >= T->n_slots) BZ_FAIL(BZ_E_INVALID, "lora_apply: row %d names slot %d outside -1..%d", r, row_slots[r], T->n_slots - 1);
  if (T->op_rows < rows) {
    BZ_HIP(hipStreamSynchronize(st));
    hipFree(T->x16); hipFree(T->d_slots); T->x16 = nullptr; T->d_slots = nullptr; T->op_rows = 0;
    int kmax = 0;
    for (int i = 0; i < LT_N; i++) kmax = std::max(kmax, T->K[i]);
    BZ_HIP(hipMalloc(&T->x16, (size_t)rows * kmax * 4));
    BZ_HIP(hipMalloc((void**)&T->d_slots, (size_t)rows * 4));
    T->op_rows = rows;
  }
  BZ_HIP(hipMemcpyAsync(T->d_slots, row_slots, (size_t)rows * 4, hipMemcpyHostToDevice, st));
  if (form == 0) {
    const void* xr = x->ptr;
    if (act != BZ_F32) { BZ_TRY(bzk_pf_cvt16(st, act, (const float*)x->ptr, (size_t)rows * g.K, T->x16)); xr = T->x16; }
    BZ_HIP(hipMemcpyAsync(y_out->ptr, base->ptr, base->nbytes, hipMemcpyDeviceToDevice, st));
    BZ_TRY(bzk_lora_shrink_rows(st, T, layer, g, act, xr, rows, T->d_slots));
    BZ_TRY(bzk_lora_expand_rows(st, T, layer, g, act, (float*)y_out->ptr, rows, T->d_slots));
  } else {
    Pro pp{}; pp.mode = PRO_PLAIN; pp.src = VSrc{x->ptr, 0}; pp.act = act; pp.H = 0;
    BZ_TRY(bzk_lora_shrink_dec(st, T, layer, g, pp, T->d_slots));
    BZ_TRY(bzk_lora_expand_dec(st, T, layer, g, act, VSrc{base->ptr, 0}, (float*)y_out->ptr, T->d_slots));
  }
  BZ_HIP(hipStreamSynchronize(st));      // row_slots is the caller's memory
  return BZ_OK;
}

// ---------------------------------------------------------------------------------------------------------
// adapters (engine/lora.rs:138-257 LoraAdapter)
// ---------------------------------------------------------------------------------------------------------
// engine/lora.rs:138-257: scaling = alpha / rank (use_rslora: alpha / sqrt(rank)), computed in f32
extern "C" int bz_lora_create(bz_device* dev, int rank, float alpha, int use_rslora, bz_lora** out) {
  BZ_API_BEGIN
  if (!dev || !out) BZ_FAIL(BZ_E_INVALID, "lora_create: null argument");
  if (rank < 1 || rank > LORA_MAX_RANK) BZ_FAIL(BZ_E_INVALID, "lora_create: rank %d outside 1..%d", rank, LORA_MAX_RANK);
  if (!(alpha == alpha) || alpha - alpha != 0.f) BZ_FAIL(BZ_E_INVALID, "lora_create: alpha is not finite");
  bz_lora* a = new bz_lora();
  a->dev = dev; a->rank = rank; a->alpha = alpha; a->use_rslora = use_rslora ? 1 : 0;
  a->scale = use_rslora ? div_rn(alpha, sqrt_rn((float)rank)) : div_rn(alpha, (float)rank);
  bz_dev_retain(dev);
  *out = a;
  return BZ_OK;
  BZ_API_END
}

// engine/lora.rs:138-257: one (lora_A [r, in], lora_B [out, r]) pair per adapted module
extern "C" int bz_lora_add(bz_lora* a, const char* key, int dtype, const void* A, const int64_t* a_shape, const void* B, const int64_t* b_shape) {
  BZ_API_BEGIN
  if (!a || !key || !A || !a_shape || !B || !b_shape) BZ_FAIL(BZ_E_INVALID, "lora_add: null argument");
  if (a->attached) BZ_FAIL(BZ_E_INVALID, "lora_add: the adapter is attached");
  if (dtype != BZ_F16 && dtype != BZ_BF16 && dtype != BZ_F32) BZ_FAIL(BZ_E_UNSUPPORTED, "lora_add: '%s': dtype %d (f16, bf16 and f32 are supported)", key, dtype);
  if (a_shape[0] != b_shape[1]) BZ_FAIL(BZ_E_UNSUPPORTED, "lora_add: '%s': lora_A has rank %lld but lora_B has rank %lld", key, (long long)a_shape[0], (long long)b_shape[1]);
  if (a_shape[0] < 1 || a_shape[0] > LORA_MAX_RANK) BZ_FAIL(BZ_E_INVALID, "lora_add: '%s': rank %lld outside 1..%d", key, (long long)a_shape[0], LORA_MAX_RANK);
  if (a_shape[1] < 8 || a_shape[1] % 8 || a_shape[1] > (1 << 20) || b_shape[0] < 1 || b_shape[0] > (1 << 24))
    BZ_FAIL(BZ_E_INVALID, "lora_add: '%s': in_features %lld (a multiple of 8) / out_features %lld", key, (long long)a_shape[1], (long long)b_shape[0]);
  if (a->pairs.count(key)) BZ_FAIL(BZ_E_INVALID, "lora_add: '%s' was added before", key);
  BZ_HIP(hipSetDevice(a->dev->id));
  LoraPair p;
  p.dt = dtype; p.r = (int)a_shape[0]; p.K = (int)a_shape[1]; p.N = (int)b_shape[0];
  const size_t es = bz_dtype_size(dtype), ab = (size_t)p.r * p.K * es, bb = (size_t)p.N * p.r * es;
  if (hipMalloc(&p.A, ab) != hipSuccess) BZ_FAIL(BZ_E_OOM, "lora_add: hipMalloc(%zu) failed", ab);
  if (hipMalloc(&p.B, std::max<size_t>(bb, 16)) != hipSuccess) { hipFree(p.A); BZ_FAIL(BZ_E_OOM, "lora_add: hipMalloc(%zu) failed", bb); }
  if (hipMemcpy(p.A, A, ab, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(p.B, B, bb, hipMemcpyHostToDevice) != hipSuccess) {
    hipFree(p.A); hipFree(p.B);
    BZ_FAIL(BZ_E_HIP, "lora_add: '%s': copy to the device failed", key);
  }
  a->pairs[key] = p;
  return BZ_OK;
  BZ_API_END
}

// executor.rs:397-420: unload drops the adapter; here only once no slot holds it
extern "C" int bz_lora_free(bz_lora* a) {
  BZ_API_BEGIN
  if (!a) return BZ_OK;
  if (a->attached) BZ_FAIL(BZ_E_INVALID, "lora_free: the adapter is attached to %d slot(s) (bz_lora_detach first)", a->attached);
  for (auto& kv : a->pairs) { hipFree(kv.second.A); hipFree(kv.second.B); }
  bz_dev_release(a->dev);
  delete a;
  return BZ_OK;
  BZ_API_END
}
