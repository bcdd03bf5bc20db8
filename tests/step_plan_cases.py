"""What a layer plan (bz_layer_plan, bz_step_plan.hip) stands for in launches, and hand-built layer traits.  Shared by tests/test_step_plan.py (no device) and
tests/test_gpu_step_plan.py (against bz_profile_step).  Plain Python; nothing here touches the GPU.

`layer_census` is the small name map: a plan's forms -> the labels bz_profile_step reports, times launches.  The `*_ok` functions restate, from the kernels'
own preconditions, what each form needs -- the property sweep of tests/test_step_plan.py holds every form a plan names to them."""
from collections import Counter

from blazr_amd import _lib as L

NORM, PLAIN, SILU, GATED = "norm", "plain", "silu", "gated"
GQ_NAME = {L.LIN_Q80: "q8_0", L.LIN_Q4K: "q4_K", L.LIN_Q5K: "q5_K", L.LIN_Q6K: "q6_K", L.LIN_Q40: "q4_0", L.LIN_Q41: "q4_1", L.LIN_Q50: "q5_0", L.LIN_Q51: "q5_1"}
FIX_BIAS = "fix_bias<f32 after the sum>"     # one launch behind every biased int4 launch (tests/test_gpu_linear_bias.py)
MLP_LABEL = {L.MLP_Q4G: "mlp_q4g<norm+gate/up+silu+down>", L.MLP_DENSE: "mlp_dense<norm+gate/up+silu+down>", L.MLP_GQ: "mlp_gguf<norm+gate/up+silu+down>"}
FUSED_LABEL = {L.ATTN_FUSED_Q4G: "attn+o_proj", L.ATTN_FUSED_DENSE: "attn+o_proj<dense>", L.ATTN_FUSED_Q4K: "attn+o_proj<q4_K>", L.ATTN_SPLIT_FUSED: "attn_merge+o_proj"}


def gemv_label(form, kind, mode):
    if form in (L.GEMV_Q4G_SLIM, L.GEMV_Q4G):
        return "gemv_q4g<%s>" % mode
    if form in (L.GEMV_ROWS2, L.GEMV_ROWS, L.GEMV_F8):
        base = {L.GEMV_ROWS2: "gemv_rows2", L.GEMV_ROWS: "gemv_rows", L.GEMV_F8: "gemv_f8"}[form]
        return base if mode == PLAIN else "%s<%s>" % (base, mode)
    if form == L.GEMV_GQ_SLIM:
        return "gemv_%s<slim>" % GQ_NAME[kind]
    if form == L.GEMV_GQ:
        return "gemv_%s" % GQ_NAME[kind]
    raise KeyError(form)


def fused_census(F, forms, mix, mode):
    """the launches of one fused linear (an L.FusedTraits and the plan's forms for it)"""
    if mix:
        return Counter({"gemv_q4_K+q6_K<slim>": 1})
    c = Counter()
    for i in range(F.n_parts):
        c[gemv_label(forms[i], F.parts[i].kind, mode)] += 1
        if F.parts[i].kind == L.LIN_Q4G and F.parts[i].bias:
            c[FIX_BIAS] += 1
    return c


def layer_census(t, p, long=False):
    """label -> launches of one layer: t an L.LayerTraits, p the plan dict of runtime.layer_plan; long: the step is beyond BZ_SPLIT_MIN keys (of the layer's window)"""
    c = fused_census(t.qkv, p["qkv"], p["qkv_mix"], NORM)
    if t.arch == L.ARCH_MAMBA2:
        return c + Counter({"mamba2_ssm_step": 1}) + fused_census(t.o, p["o"], 0, GATED)
    if t.arch == L.ARCH_DEEPSEEK2:
        assert p["mla_exact"], "the f32 MLA kernels choose their own split (bzk_mla_attn): not part of the plan"
        c += Counter({"mla_scores<exact>": 1, "mla_weights<exact>": 1, "mla_merge<exact>": 1}) + fused_census(t.o, p["o"], 0, PLAIN)
        if not t.is_moe:
            return c + fused_census(t.gateup, p["gateup"], p["gateup_mix"], NORM) + fused_census(t.down, p["down"], 0, SILU)
        if p["moe_route_fused"]:
            return c + Counter({"gemv_rows2<norm>": 1, "moe_rows2<route+gate_up>": 1, "moe_rows2<down>": 1, "moe_combine": 1})
        k = "moe_rows2" if p["moe_rows2"] else "moe_gemv"
        return c + Counter({"moe_router": 1, k + "<gate_up>": 1, k + "<down>": 1, "moe_combine": 1})
    attn = p["attn_long"] if long else p["attn_short"]
    if attn in (L.ATTN_SPLIT, L.ATTN_SPLIT_FUSED):
        c["attn_split"] += 1
    if attn in FUSED_LABEL:
        c[FUSED_LABEL[attn]] += 1
        if attn != L.ATTN_FUSED_Q4K and t.o.parts[0].bias:
            c[FIX_BIAS] += 1
    else:
        c["attn_merge" if attn == L.ATTN_SPLIT else "attn_decode"] += 1
        c += fused_census(t.o, p["o"], 0, PLAIN)
    if p["mlp"] != L.MLP_SPLIT:
        c[MLP_LABEL[p["mlp"]]] += 1
        if p["mlp"] == L.MLP_Q4G and t.down.parts[0].bias:
            c[FIX_BIAS] += 1
        return c
    return c + fused_census(t.gateup, p["gateup"], p["gateup_mix"], NORM) + fused_census(t.down, p["down"], 0, SILU)


def is_long(t, position, split_min):
    """the step's one decision per call: position + 1 keys, or the layer's window of them, against BZ_SPLIT_MIN"""
    keys = position + 1
    if keys <= split_min:
        return False
    return t.window == 0 or min(keys, t.window) > split_min


# ---- hand-built traits -------------------------------------------------------------------------------------------------------------------------------------
def lin(kind, N, K, wdt=L.F16, gw=1, sk=1, npf=2, act_order=0, bias=0):
    return L.LinearTraits(kind, N, K, wdt, gw, sk, npf, act_order, bias)


def fused(*parts, fix_out=1):
    f = L.FusedTraits(n_parts=len(parts), fix_out=fix_out)
    for i, p in enumerate(parts):
        f.parts[i] = p
    return f


def llama_traits(act, H, I, nq, nkv, hd, qkv, o, gateup, down, **kw):
    return L.LayerTraits(arch=L.ARCH_LLAMA, act_dtype=act, hidden=H, inter=I, n_heads=nq, n_kv_heads=nkv, head_dim=hd, qkv=qkv, o=o, gateup=gateup, down=down, **kw)


def q4g_layer(H, I, nq, nkv, hd, act=L.F16, **kw):
    """AWQ / GPTQ without act-order: every fused linear one int4 part"""
    return llama_traits(act, H, I, nq, nkv, hd, fused(lin(L.LIN_Q4G, (nq + 2 * nkv) * hd, H)), fused(lin(L.LIN_Q4G, H, nq * hd)), fused(lin(L.LIN_Q4G, 2 * I, H)),
                        fused(lin(L.LIN_Q4G, H, I)), **kw)


def dense_layer(H, I, nq, nkv, hd, dt=L.BF16, sk=2, **kw):
    """dense 16-bit weights in the activation dtype, split-K (fixed-point output) as bzk_rows_choose_sk gives wherever K % 8 == 0"""
    def r(N, K):
        return fused(lin(L.LIN_ROWS, N, K, wdt=dt, sk=sk), fix_out=int(sk > 1))
    return llama_traits(dt, H, I, nq, nkv, hd, r((nq + 2 * nkv) * hd, H), r(H, nq * hd), r(2 * I, H), r(H, I), **kw)


def gptq_actorder_layer(H, I, nq, nkv, hd, bias=1):
    """act-order: q, k, v, gate, up each a part of its own (their permutations differ)"""
    def p(N, K):
        return lin(L.LIN_Q4G, N, K, act_order=1, bias=bias)
    return llama_traits(L.F16, H, I, nq, nkv, hd, fused(p(nq * hd, H), p(nkv * hd, H), p(nkv * hd, H)), fused(p(H, nq * hd)), fused(p(I, H), p(I, H)), fused(p(H, I)))


def q4km_layer(H, I, nq, nkv, hd, more_bits, **kw):
    """GGUF Q4_K_M, f32 activations: q, k, o, gate, up Q4_K; v and down Q6_K in the layers the rule gives more bits, Q4_K in the others"""
    big = L.LIN_Q6K if more_bits else L.LIN_Q4K
    qkv = fused(lin(L.LIN_Q4K, (nq + nkv) * hd, H), lin(L.LIN_Q6K, nkv * hd, H)) if more_bits else fused(lin(L.LIN_Q4K, (nq + 2 * nkv) * hd, H))
    return llama_traits(L.F32, H, I, nq, nkv, hd, qkv, fused(lin(L.LIN_Q4K, H, nq * hd)), fused(lin(L.LIN_Q4K, 2 * I, H)), fused(lin(big, H, I)), **kw)


def one_kind_layer(kind, H, I, nq, nkv, hd, act=L.F32):
    return llama_traits(act, H, I, nq, nkv, hd, fused(lin(kind, (nq + 2 * nkv) * hd, H)), fused(lin(kind, H, nq * hd)), fused(lin(kind, 2 * I, H)), fused(lin(kind, H, I)))


# ---- the forms' preconditions, restated (bz_kernels.hip: what each kernel is instantiated and indexed for) ---------------------------------------------------
GQ_SLIM_KINDS = (L.LIN_Q4K, L.LIN_Q5K, L.LIN_Q6K, L.LIN_Q40, L.LIN_Q41, L.LIN_Q50, L.LIN_Q51)


def gemv_form_ok(form, P, mode, H, act, sw):
    """may a part P (an L.LinearTraits) launch as `form` under prologue `mode` over H elements?"""
    perm = P.act_order
    if form == L.GEMV_Q4G_SLIM:      # k_gemv_q4g_slim<FIX, NJ = K / 2048>: f16 activations, whole 64-column tiles, the norm over K itself
        return P.kind == L.LIN_Q4G and act == L.F16 and not sw.no_slim_qkv and not perm and mode == NORM and P.K == H and P.K in (2048, 4096, 8192) and P.N % 64 == 0 and P.N <= 16384
    if form == L.GEMV_Q4G:
        return P.kind == L.LIN_Q4G
    if form == L.GEMV_ROWS2:         # k_gemv_rows2: 16-bit weights in 8-element pieces, a fixed-point accumulator
        return P.kind == L.LIN_ROWS and not sw.no_rows2 and P.sk > 1 and P.wdt in (L.F16, L.BF16) and P.K % 8 == 0 and P.K <= 131072 and not perm and (mode != NORM or P.K == H)
    if form == L.GEMV_ROWS:
        return P.kind == L.LIN_ROWS
    if form == L.GEMV_GQ_SLIM:       # k_gemv_gq_slim: whole tiles and superblocks; the norm form for K = 2048 NJ
        return P.kind in GQ_SLIM_KINDS and not sw.no_gq_slim and not perm and P.N % 64 == 0 and P.K % 256 == 0 and P.K == H and (mode == SILU or (mode == NORM and P.K in (2048, 4096, 8192)))
    if form == L.GEMV_GQ:
        return P.kind in GQ_SLIM_KINDS + (L.LIN_Q80,)
    return form == L.GEMV_F8 and P.kind == L.LIN_F8


def attn_form_ok(form, t, kv, sw):
    """may a Llama-family layer launch attention + o_proj as `form` over a cache of dtype kv?"""
    O, nq, nkv, hd = t.o.parts[0], t.n_heads, t.n_kv_heads, t.head_dim
    one = t.o.n_parts == 1 and t.o.fix_out and not t.lora_o and not sw.no_attn_fusion
    split = not sw.no_attn_split and hd == 128 and kv in (L.F16, L.BF16) and nq % nkv == 0 and nq // nkv in (1, 2, 4, 8)      # k_attn_split<DT, PG, REP>
    q4g = one and hd == 128 and O.kind == L.LIN_Q4G and not O.act_order and O.K == nq * 128 and kv in (L.F16, L.BF16)
    if form == L.ATTN_PLAIN:
        return True
    if form == L.ATTN_SPLIT:
        return split
    if form == L.ATTN_SPLIT_FUSED:   # k_attn_merge_oproj<TPW 1 | 2>: 8 waves x CS slices x TPW tiles cover N / 64
        return split and q4g and any((O.N // 64) % (cs * 8) == 0 and (O.N // 64) // (cs * 8) <= 2 for cs in (8, 4, 2, 1))
    if form == L.ATTN_FUSED_Q4G:     # k_attn2<DT, 1, TPW, 8 | 4 waves>
        return q4g and any((O.N // 64) % (cs * w) == 0 and (O.N // 64) // (cs * w) <= 2 and nq * cs <= 1024 for w in (8, 4) for cs in (8, 4, 2, 1))
    if form == L.ATTN_FUSED_DENSE:   # k_attn2<DT, 2, loads 1 | 2 | 4, 8 waves, head_dim 64 | 128>: weights in the cache's dtype
        return (one and not sw.no_attn2_hd64 and O.kind == L.LIN_ROWS and O.wdt == kv and kv in (L.F16, L.BF16) and hd in (64, 128) and O.K == nq * hd and nq * 8 <= 2048 and
                O.N % 64 == 0 and (O.N // 64) % (512 // hd) == 0 and (O.N // 64) // (512 // hd) in (1, 2, 4))
    if form == L.ATTN_FUSED_Q4K:     # k_attn2f: one 64-column tile per wave, 8 waves
        return one and not sw.no_attn_f32 and kv == L.F32 and hd == 128 and O.kind == L.LIN_Q4K and O.K == nq * 128 and O.N % 512 == 0 and O.K % 256 == 0 and nq * (O.N // 512) <= 2048
    return False


def attn_kernel_ok(kernel, t, kv, sw):
    hd = t.head_dim
    if kernel == L.ATTN_K_ATTN2:     # k_attn2<DT, 0, ...>: a 16-bit cache
        return kv != L.F32 and (hd == 128 or (hd == 64 and not sw.no_attn2_hd64))
    if kernel == L.ATTN_K_ATTN2F:
        return kv == L.F32 and hd == 128 and not sw.no_attn_f32
    return kernel == L.ATTN_K_DECODE and hd in (64, 128)


def mlp_form_ok(form, t, sw):
    if form == L.MLP_SPLIT:
        return True
    if sw.no_mlp_fusion or t.lora_mlp or t.gateup.n_parts != 1 or t.down.n_parts != 1:
        return False
    G, D, H, I = t.gateup.parts[0], t.down.parts[0], t.hidden, t.inter
    shape = G.N == 2 * I and G.K == H and D.N == H and D.K == I and not G.act_order and not D.act_order
    if form == L.MLP_Q4G:            # k_mlp_q4g<.., 16 | 8 waves, f16>
        return shape and t.act_dtype == L.F16 and G.kind == D.kind == L.LIN_Q4G and H in (2048, 4096) and I % 128 == 0
    if form == L.MLP_DENSE:          # k_mlp_dense: the slab copy, one workgroup per 32 rows of down_proj
        return shape and bool(t.down_slabs) and G.kind == D.kind == L.LIN_ROWS and G.wdt == D.wdt and G.wdt in (L.F16, L.BF16) and H % 512 == 0 and 1024 <= H <= 2048 and I % 32 == 0 and \
            I // 32 >= 128 and G.sk > 1 and D.sk > 1
    return form == L.MLP_GQ and shape and bool(sw.gguf_mlp_fusion) and t.act_dtype == L.F32 and G.kind == L.LIN_Q4K and D.kind in (L.LIN_Q4K, L.LIN_Q6K) and H in (2048, 4096) and I % 256 == 0
