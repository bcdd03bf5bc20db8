"""Llama-family shapes off the power-of-two grid every other fixture sits on: GQA groups of 3 / 6 / 7, widths that are multiples of 64 / 128 / 256 but
no power of two (384, 768, 896; inter 640 .. 1408), vocabularies that are no multiple of 64, and `n_heads * head_dim != hidden`.  The smallest shapes
that still leave the grid; the CPU oracle runs each in 0.2-1.7 s.  Shared by tests/test_gpu_irregular_shapes.py and tests/test_oracle.py.  Data only;
nothing here touches the GPU."""
from blazr_amd import synth

# name -> (preset, overrides); the third column of the issue's table ("there to reach") is the comment above each case
CASES = {
    # rep 3 on k_attn2<head_dim 64>; o_proj 384 = 6 column tiles: dense attention + o_proj fusion refused; untied ragged dense lm_head (1003 rows)
    "bf16-g3-hd64": ("tiny-bf16", dict(hidden=384, n_heads=6, n_kv_heads=2, head_dim=64, inter=704, vocab=1003, tie_embeddings=False, max_seq_len=512)),
    # rep 3 at head_dim 128: split-KV refused at every context; o_proj 768 = 12 tiles, 3 loads per wave: fusion refused; tied ragged head
    "bf16-g3-hd128": ("tiny-bf16", dict(hidden=768, n_heads=6, n_kv_heads=2, head_dim=128, inter=1408, vocab=1003, max_seq_len=512)),
    # rep 2: the FAST paths (MFMA prompt GEMM + flash attention, split-KV, multi-row batch) at 12 / 22 column tiles and a ragged N.  The control of (c)
    "bf16-g2-w768": ("tiny-bf16", dict(hidden=768, n_heads=6, n_kv_heads=3, head_dim=128, inter=1408, vocab=1003, max_seq_len=512)),
    # generic k_gemv_q4g at 6 and 11 groups of 128; int4 attention + o_proj plan refused; K % 256 != 0 (inter 1408): int4 prompt GEMM refused
    "awq-g3": ("tiny-awq", dict(hidden=768, n_heads=6, n_kv_heads=2, head_dim=128, inter=1408, vocab=1001, max_seq_len=512)),
    # rep 4, every K % 256 == 0: W4A16 MFMA / LDS prompt GEMMs and the multi-row batch at 12 / 20 column tiles; n_heads * head_dim = 512 != hidden
    "awq-g4-w768": ("tiny-awq", dict(hidden=768, n_heads=4, n_kv_heads=1, head_dim=128, inter=1280, vocab=1001, max_seq_len=512)),
    # rep 7 (the Qwen2 outline), 7 groups of 128 along hidden, 5 along inter
    "awq-g7": ("tiny-awq", dict(hidden=896, n_heads=14, n_kv_heads=2, head_dim=64, inter=640, vocab=1027, max_seq_len=512)),
    # rep 6 with the act-order permutation and a bias on every projection
    "gptq-g6": ("tiny-gptq", dict(act_order=True, bias=True, hidden=768, n_heads=12, n_kv_heads=2, head_dim=64, inter=1152, vocab=1001, max_seq_len=512)),
    # k_attn2f at rep 3; o_proj N 768 % 512 != 0: f32 fusion refused; the slim SILU GEMV over 5 superblocks, the generic NORM GEMV over 3
    "q4km-g3": ("tiny-q4km", dict(n_layers=2, hidden=768, n_heads=6, n_kv_heads=2, head_dim=128, inter=1280, vocab=1088, max_seq_len=512)),
    # Q8_0 at 3 / 5 / 7 superblocks of 256, rep 7, f32 cache at head_dim 64; n_heads * head_dim = 1792 != hidden.  28q / 4kv, not the 14q / 2kv of
    # Q8_0_G7_NOT_LOADABLE below: the same group, twice the heads, so that o_proj's K is a whole number of superblocks
    "q8_0-g7": ("tiny-q8_0", dict(hidden=768, n_heads=28, n_kv_heads=4, head_dim=64, inter=1280, vocab=1088, max_seq_len=512)),
}

# 14q / 2kv x 64 gives o_proj K = 896 = 3.5 superblocks: bz_model_add_gguf takes block-format linears with K % 256 == 0 only, so the library refuses this
# model when the tensor is added (BZ_E_UNSUPPORTED, nothing launched).  The oracle runs it (tests/test_oracle.py); on the GPU the refusal is what is tested
Q8_0_G7_NOT_LOADABLE = ("tiny-q8_0", dict(hidden=768, n_heads=14, n_kv_heads=2, head_dim=64, inter=1280, vocab=1088, max_seq_len=512))

# cases whose GQA group is no power of two: single-launch attention at every context, prompts token by token, decode batches sequence by sequence
ODD_GROUP = [n for n, (_, o) in CASES.items() if (o["n_heads"] // o["n_kv_heads"]) not in (1, 2, 4, 8)]


def make(name):
    preset, over = CASES[name]
    return synth.make_llama(preset, **over)


def rep(name):
    o = CASES[name][1]
    return o["n_heads"] // o["n_kv_heads"]
