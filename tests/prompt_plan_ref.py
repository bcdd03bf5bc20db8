"""An independent restatement of DESIGN.md "Which path a prompt takes": for every route the list of things that turn a call away; a call with no objection
takes the route.  Plain Python over plain dicts -- no library, no device.  tests/test_prompt_plan.py holds bz_prompt_plan to it field for field."""
import os

F32, F16, BF16 = 0, 1, 2
LLAMA, MAMBA2, DEEPSEEK2 = 0, 1, 2
PROMPT, DECODE_BATCH, VERIFY = 0, 1, 2
STEPS, ROWS, DSV2, MAMBA = 0, 1, 2, 3
ATTN_NONE, ATTN_MFMA, ATTN_SCALAR, ATTN_SCALAR_EXACT, ATTN_ROWS = 0, 1, 2, 3, 4
HEAD_STEP, HEAD_GEMM, HEAD_GEMV_ROWS, HEAD_SPEC = 0, 1, 2, 3

LDS = 160 * 1024
DEFAULT_SWITCHES = dict(prefill_min=8, no_mfma_prefill=0, no_gguf_prefill=0, exact=-1, exact_max=16, exact_i8_max=0)
ON_STEPS = dict(route=STEPS, exact=0, attn=ATTN_NONE, head=HEAD_STEP, chunk=0)


def scalar_attn_lds(n_heads, n_kv_heads, head_dim, keys, exact):
    """k_pf_attn: per query head of the group 8 running values and the 256 // (head_dim // 8) staged rows of head_dim (f32, or double for the exact sums),
    the scores of `keys` positions (f32), 64 bytes of bookkeeping"""
    rep = n_heads // n_kv_heads
    return (8 * rep + (256 // (head_dim // 8)) * rep * head_dim) * (8 if exact else 4) + rep * keys * 4 + 64


def scalar_attn_limit(n_heads, n_kv_heads, head_dim, exact):
    """the last context the scalar kernel holds"""
    rep = n_heads // n_kv_heads
    return (LDS - scalar_attn_lds(n_heads, n_kv_heads, head_dim, 0, exact)) // (4 * rep)


def mla_lds(rank, rope, nope, vdim, keys):
    """the single-pass MLA decode kernel: the latent, the query's absorbed form and one partial per wave (16 waves where nope and v are multiples of 16, else
    4), the rope halves, the nope query, 16 words, the scores"""
    waves = 16 if nope % 16 == 0 and vdim % 16 == 0 else 4
    return (rank * (2 + waves) + 2 * rope + nope + 16 + keys) * 4 + 64


def mla_limit(rank, rope, nope, vdim):
    return (LDS - mla_lds(rank, rope, nope, vdim, 0)) // 4


def mfma_attn_built(t):
    """the MFMA flash kernel: head_dim 64 / 128, group sizes 1 / 2 / 4 / 8; BZ_NO_PF_ATTN_MFMA (read once by the launcher's own test) turns it off"""
    return "BZ_NO_PF_ATTN_MFMA" not in os.environ and t["head_dim"] in (64, 128) and t["rep"] in (1, 2, 4, 8)


def keys_read(t, total_len):
    """the most keys a query reads: its window, if EVERY layer has one (pattern n > 1: layers n - 1, 2 n - 1, ... attend fully)"""
    n, w = t["sliding_window_pattern"], t["sliding_window"]
    full_layers = [l for l in range(t["n_layers"]) if w <= 0 or (n > 1 and l % n == n - 1)]
    return total_len if full_layers else min(total_len, w)


def row_floor(sw):
    return (1 << 30) if sw["no_mfma_prefill"] else sw["prefill_min"]


def wants_exact_steps(sw, rows):
    """exact-sum models keep short prompts on the decode step: BZ_EXACT_PREFILL 0 never, > 0 always, unset up to BZ_EXACT_PREFILL_MAX rows"""
    if sw["exact"] == 0:
        return False
    return sw["exact"] > 0 or rows <= sw["exact_max"]


def exact_rows_mode(t, sw, rows):
    """f16 int4 models: 1 the multi-row exact rows, 2 the integer-MFMA GEMMs, 0 neither; never more than the projections offer (exact_cap)"""
    if t["act_dtype"] != F16 or sw["exact"] == 0:
        return 0
    if sw["exact"] == 1:
        asked = 1
    elif sw["exact"] >= 2:
        asked = 2 if rows > 16 else 1
    elif rows <= sw["exact_max"]:
        asked = 1
    elif rows <= sw["exact_i8_max"]:
        asked = 2
    else:
        asked = 0
    return min(asked, t["exact_cap"])


def _llama_verify(t, sw, rows, total_len):
    no = []
    if not t["shapes_ok"]: no.append("shapes")
    if t["act_dtype"] != F16: no.append("f16 only")
    if rows > 16: no.append("more than 16 rows")
    if exact_rows_mode(t, sw, rows) != 1: no.append("not the multi-row exact rows")
    if not t["spec_head"]: no.append("head")
    if not no and scalar_attn_lds(t["n_heads"], t["n_kv_heads"], t["head_dim"], keys_read(t, total_len), True) > LDS: no.append("context")
    return ON_STEPS if no else dict(route=ROWS, exact=1, attn=ATTN_SCALAR_EXACT, head=HEAD_SPEC, chunk=2048)


def _llama_rows(t, sw, kind, rows, total_len):
    batch = kind == DECODE_BATCH
    f32 = t["act_dtype"] == F32
    if not t["shapes_ok"]:
        return ON_STEPS
    if not batch and rows < row_floor(sw):           # a decode batch counts as at least the floor
        return ON_STEPS
    S = max(rows, row_floor(sw)) if batch else rows
    if f32 and sw["no_gguf_prefill"]:
        return ON_STEPS
    exact = 0 if batch else exact_rows_mode(t, sw, S)
    if batch:
        attn = ATTN_ROWS
    elif exact or f32:
        attn = ATTN_SCALAR_EXACT
    elif mfma_attn_built(t):
        attn = ATTN_MFMA
    else:
        attn = ATTN_SCALAR
    # context: only the scalar kernel has a limit; a decode batch is let through wherever the MFMA kernel is built (the documented oddity)
    limited = attn in (ATTN_SCALAR, ATTN_SCALAR_EXACT) or (batch and not mfma_attn_built(t))
    if limited and scalar_attn_lds(t["n_heads"], t["n_kv_heads"], t["head_dim"], keys_read(t, total_len), attn == ATTN_SCALAR_EXACT) > LDS:
        return ON_STEPS
    if f32:
        if not t["gq_all"] or t["gq_max_n3k"] >= 1 << 32 or min(S, 2048) * 3 * t["gq_max_k"] >= 1 << 32:
            return ON_STEPS
        head = HEAD_GEMV_ROWS if t["head_rows"] else HEAD_STEP
    else:
        if not t["proj_16"] or not t["head_rows"]:
            return ON_STEPS
        if t["any_dense"] and not batch and wants_exact_steps(sw, S):
            return ON_STEPS
        head = HEAD_GEMM if t["head_gemm"] and not exact else HEAD_GEMV_ROWS
    return dict(route=ROWS, exact=exact, attn=attn, head=head, chunk=512 if batch else 2048)


def plan(t, sw, kind, rows, total_len, kv_dtype):
    sw = dict(DEFAULT_SWITCHES, **(sw or {}))
    arch, act16 = t["arch"], t["act_dtype"] in (F16, BF16)
    if arch == LLAMA:
        return _llama_verify(t, sw, rows, total_len) if kind == VERIFY else _llama_rows(t, sw, kind, rows, total_len)
    if kind != PROMPT or not act16 or rows < row_floor(sw) or wants_exact_steps(sw, rows) or not t["head_rows"]:
        return ON_STEPS
    if arch == DEEPSEEK2:
        ok = (t["mla_q_lora_rank"] == 0 and t["ds_dims_ok"] and t["ds_weights_act"] and kv_dtype == t["act_dtype"] and
              mla_lds(t["mla_kv_lora_rank"], t["mla_rope_dim"], t["mla_nope_dim"], t["mla_v_dim"], total_len) <= LDS)
        return dict(route=DSV2, exact=0, attn=ATTN_NONE, head=HEAD_GEMM if t["head_gemm"] else HEAD_GEMV_ROWS, chunk=512) if ok else ON_STEPS
    if arch == MAMBA2:
        ok = t["ssm_scan_ok"] and t["ssm_groups_ok"] and t["ssm_proj_ok"]
        return dict(route=MAMBA, exact=0, attn=ATTN_NONE, head=HEAD_GEMV_ROWS, chunk=512) if ok else ON_STEPS
    return ON_STEPS
