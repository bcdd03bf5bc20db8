"""INT8 W8A8 on the device.  Every sum of the format is an integer, so the op tests ask for the numpy restatement's bits (tests/int8_cases.py ref_linear): the
read-back, the decode GEMV with the quantiser in its prologue (direct and split-K), the row quantiser + int8 MFMA GEMM.  Whole models: against a numpy model
whose linears are that restatement, the structural identities of the step, checkpoints, refusals, a paged decode batch and an engine run."""
import numpy as np
import pytest

import int8_cases as I
import npref
import test_gpu_fp8_weights as T8
from blazr_amd import _lib as L
from blazr_amd import runtime, synth
from test_gpu_engine import _drive
from test_gpu_llama import _kv_dt

pytestmark = pytest.mark.gpu
_OPS, _MODELS = {}, {}


@pytest.mark.parametrize("strategy", ["channel", "tensor"])
def test_dequant_reads_back_every_code(device, strategy):
    spec = synth.int8_linear("op", 64, 256, strategy, seed=11)
    spec["weight"][0], spec["weight"][1] = np.arange(-128, 128), np.arange(-128, 128)[::-1]            # all 256 values, -128 included
    want = spec["weight"].astype(np.float32) * np.broadcast_to(spec["scale"], (64,))[:, None]          # 8 x 8 significant bits: exact
    assert np.array_equal(T8._op_model(device, spec).dequant(T8.DOWN), want)


def _op(device, N, K, act):
    """one model (channel scales, a bias), its planted input rows and the reference per (shape, dtype), shared by the GEMV and the GEMM tests"""
    if (N, K, act) not in _OPS:
        spec, x = synth.int8_linear("op", N, K, "channel", bias=True, seed=N * 7 + K), I.planted_rows(K, act, N + K)
        _OPS[(N, K, act)] = (T8._op_model(device, spec, act), x, I.ref_linear(x, spec["weight"], spec["scale"], spec["bias"]))
    return _OPS[(N, K, act)]


@pytest.mark.parametrize("act", ["bf16", "f16"])
@pytest.mark.parametrize("N,K", I.GEMV_SHAPES)
def test_quant_matmul_is_the_reference_bit_for_bit(device, N, K, act):
    """(256, 4096) and (64, 14336) run the split-K form (integer partials, the finish in the launch), the others the direct one"""
    lm, x, want = _op(device, N, K, act)
    got = lm.quant_matmul(T8.DOWN, x)
    print("gemv_i8 [%d, %d] %s: %d of %d outputs differ" % (N, K, act, int((got != want).sum()), want.size))
    assert np.array_equal(got, want)
    assert np.array_equal(lm.quant_matmul(T8.DOWN, x[:2]), want[:2])      # the split form left its accumulator and counters as it found them


@pytest.mark.parametrize("act", ["bf16", "f16"])
@pytest.mark.parametrize("S", I.GEMM_ROWS)
@pytest.mark.parametrize("N,K", I.GEMM_SHAPES)
def test_prefill_matmul_is_the_reference_bit_for_bit(device, N, K, S, act):
    """the row quantiser and the int8 MFMA GEMM; the S rows cycle through the planted ones, and a GEMM row is the GEMV of that row"""
    lm, x, want = _op(device, N, K, act)
    rows = np.arange(S) % x.shape[0]
    got = T8._prefill_matmul(device, lm, x[rows], N).astype(np.float32)
    print("gemm_i8a8 S=%d [%d, %d] %s: %d of %d outputs differ" % (S, N, K, act, int((got != want[rows]).sum()), got.size))
    assert np.array_equal(got, want[rows])


def _pair(device, name):
    if name not in _MODELS:
        model = I.make(name)
        _MODELS[name] = (model, runtime.LoadedModel.from_synth(device, model))
    return _MODELS[name]


class NpLlamaW8A8(npref.NpLlama):
    """every linear is the restatement: the input row quantised per token, the integer sum, one scale"""
    def _lin(self, l, name, x):
        s = self.m["layers"][l][name]
        return I.ref_linear(x[None, :], s["weight"], s["scale"], s.get("bias"))[0]


def _prompt(device, lm, cfg, p, rows):
    kv = runtime.LayeredKvCache(device, cfg["n_layers"], 1, cfg["n_kv_heads"], 64, cfg["max_seq_len"], cfg["head_dim"], _kv_dt(cfg))
    return np.concatenate([lm.forward_with_kv_cache(p[i:i + rows], kv, i, all_logits=True).to_numpy().reshape(rows, -1) for i in range(0, len(p), rows)])


@pytest.mark.parametrize("name", list(I.MODELS))
def test_prompt_and_steps_are_the_w8a8_reference(device, name):
    """rel L2(device, numpy W8A8) <= 1/2 rel L2(numpy 16-bit activations, numpy W8A8), for a 40-row prompt in one call (the GEMMs) and its first 12 tokens one
    by one (the GEMVs).  The feature's own effect is the yardstick: a linear left on 16-bit activations, or a wrong scale, is as large as the effect itself.
    Measured on an MI355X: bf16 prompt 1.009e-3, steps 0.0, effect 1.735e-2; f16 prompt 9.188e-6, steps 9.688e-7, effect 1.113e-2."""
    model, lm = _pair(device, name)
    cfg = model["config"]
    p = [int(t) for t in synth.prompt_tokens(40, cfg["vocab"], seed=13)]
    a16, a8 = npref.NpLlama(I.restate_f32(model)), NpLlamaW8A8(model)
    ref16, ref8 = np.stack([a16.step(t, i) for i, t in enumerate(p)]), np.stack([a8.step(t, i) for i, t in enumerate(p)])
    effect, got, steps = T8._rel(ref16, ref8), _prompt(device, lm, cfg, p, 40), _prompt(device, lm, cfg, p[:12], 1)
    print("%s: prompt to numpy W8A8 %.3e, steps %.3e, numpy A16 to numpy W8A8 %.3e" % (name, T8._rel(got, ref8), T8._rel(steps, ref8[:12]), effect))
    assert effect > 0.0
    assert T8._rel(got, ref8) <= 0.5 * effect
    assert T8._rel(steps, ref8[:12]) <= 0.5 * T8._rel(ref16[:12], ref8[:12])


@pytest.mark.parametrize("name", list(I.MODELS))
def test_graph_eager_paged_and_pieces_are_the_same_bits(device, name):
    """the protocol of the FP8 file's test of this name: a 12-token prompt and 6 greedy steps, eager; the layer range in two pieces; the captured step; scattered
    pages of 4, eager and through the executor"""
    model, lm = _pair(device, name)
    cfg = model["config"]
    p = synth.prompt_tokens(12, cfg["vocab"], seed=8)
    mk = lambda: runtime.LayeredKvCache(device, cfg["n_layers"], 1, cfg["n_kv_heads"], 32, cfg["max_seq_len"], cfg["head_dim"], _kv_dt(cfg))
    kv, kv2, kv3 = mk(), mk(), mk()
    mono = lm.forward_with_kv_cache(p, kv, 0, all_logits=True).to_numpy()
    toks, eager = [int(mono[-1].argmax())], []
    for i in range(6):
        eager.append(lm.forward_with_kv_cache([toks[-1]], kv, 12 + i).to_numpy()[0])
        toks.append(int(eager[-1].argmax()))
    h, pm = lm.forward_layers_range(lm.forward_embed(p), None, kv2, 0, 1, 0)
    h, pm = lm.forward_layers_range(h, pm, kv2, 1, cfg["n_layers"], 0)
    assert np.array_equal(mono, lm.forward_head(h, pm, all_logits=True).to_numpy())
    lm.forward_with_kv_cache(p, kv3, 0)
    g = runtime.DecodeGraph(lm, kv3)
    g.seed_next_token(toks[0], 12)
    for i in range(6):
        g.replay()
        assert np.array_equal(g.read_logits(), eager[i]) and g.read_token(i) == toks[i + 1], i
    pk = runtime.LayeredPagedKvCache(device, cfg["n_layers"], 9, 4, cfg["n_kv_heads"], cfg["head_dim"], _kv_dt(cfg))
    pk.set_blocks([7, 2, 5, 0, 8, 3, 1])
    pk.set_seq_len(12)
    assert np.array_equal(mono, lm.forward_with_paged_kv_cache(p, pk, pk.compute_slot_mapping(0, 12), pk.block_table_device_format(), 12, 0, all_logits=True).to_numpy())
    for i in range(3):
        pk.set_seq_len(13 + i)
        lg = lm.forward_with_paged_kv_cache([toks[i]], pk, pk.compute_slot_mapping(12 + i, 1), pk.block_table_device_format(), 13 + i, 12 + i).to_numpy()[0]
        assert np.array_equal(lg, eager[i]), i
    runs = [runtime.Executor(lm).generate(p, 12, use_graph=gr, paged=pg).tolist() for gr in (False, True) for pg in (False, True)]
    assert runs[0] == runs[1] == runs[2] == runs[3] and runs[0][:7] == toks


def test_forced_split_k_step_is_the_direct_step(device, monkeypatch):
    """No fixture's rows are long enough for the split rule, so the split-K form is forced at finalize (BZ_I8_SPLITK) on a model of width 768 -- three 256-chunks
    in q/k/v, o_proj and gate/up, six in down_proj, so 2 and 3 slices split every linear of the step: the norm prologue with its residual write, the fixed-point
    hand-offs into attention, the next norm and the SiLU prologue.  The sums are the same integers and the ring is handed the act-rounded value, so the logits
    of the prompt (token by token) and of the steps are the direct form's bits, eager and captured."""
    model = I.make("tiny-int8-channel-bf16", hidden=768, n_heads=6, n_kv_heads=3, head_dim=128, inter=1536, vocab=1003, max_seq_len=512)
    cfg, out = model["config"], {}
    p = [int(t) for t in synth.prompt_tokens(9, cfg["vocab"], seed=21)]
    for sk in ("0", "2", "3"):
        monkeypatch.setenv("BZ_I8_SPLITK", sk)
        lm = runtime.LoadedModel.from_synth(device, model)
        ex = runtime.Executor(lm)
        a, b, c = (ex.generate(p, 16, use_graph=True).tolist(), ex.generate(p, 16, use_graph=True).tolist(), ex.generate(p, 16, use_graph=False).tolist())
        assert a == b == c
        assert [getattr(lm.layer_traits(0), f).parts[0].sk for f in ("qkv", "o", "gateup", "down")] == [max(int(sk), 1)] * 4      # every linear of the step splits
        out[sk] = (_prompt(device, lm, cfg, p + a[:3], 1), a)
    for sk in ("2", "3"):
        print("split %s vs direct: %d of %d logits differ" % (sk, int((out[sk][0] != out["0"][0]).sum()), out["0"][0].size))
        assert np.array_equal(out[sk][0], out["0"][0]) and out[sk][1] == out["0"][1]


@pytest.mark.parametrize("name", list(I.MODELS))
def test_checkpoint_round_trip(device, tmp_path, name):
    """channel scales as BF16 [N,1] / a tensor scale as F32 [1], an all-zero weight_zero_point beside every weight, an untied 16-bit lm_head; the channel file
    once more without its quantization_config (detected from the I8 weight with its scale beside it); and a nonzero zero point, refused by name"""
    model = I.make(name, tie_embeddings=False)
    cfg, b = model["config"], runtime.LoadedModel.from_synth(device, model)
    p = synth.prompt_tokens(12, cfg["vocab"], seed=5)
    for i, with_qc in enumerate((True, False) if "channel" in name else (True,)):
        I.write_int8_checkpoint(str(tmp_path / str(i)), model, with_quant_config=with_qc, zero_point=0)
        a = runtime.load_model(device, str(tmp_path / str(i)))
        assert a.c.act_dtype == b.c.act_dtype and a.weight_bytes() == b.weight_bytes()
        assert np.array_equal(T8._logits(device, a, cfg, p), T8._logits(device, b, cfg, p))
    I.write_int8_checkpoint(str(tmp_path / "zp"), model, zero_point=3)
    with pytest.raises(L.BlazrHipError) as ex:
        runtime.load_model(device, str(tmp_path / "zp"))
    assert ex.value.code == L.E_UNSUPPORTED and "weight_zero_point" in str(ex.value)


def _add(lm, name, N, K, s):
    w, s = np.zeros((N, K), np.int8), np.ascontiguousarray(s, np.float32)
    rc = L.lib().bz_model_add_int8(lm.h, name.encode(), N, K, T8._PTR(w), T8._PTR(s), s.size, None)
    return rc, L.lib().bz_last_error().decode()


@pytest.mark.parametrize("case", ["N%64", "K%64", "K>131072", "n_scale", "scale-inf", "scale-nan", "scale-zero", "scale-negative"])
def test_add_int8_refusals_name_the_tensor(device, case):
    lm = runtime.LoadedModel(device, synth.make_config("tiny-int8"))
    name = "model.layers.0.mlp.down_proj.weight"
    N, K = {"N%64": (96, 128), "K%64": (128, 96), "K>131072": (64, 131072 + 64)}.get(case, (128, 128))
    s = np.full(N, 2.0 ** -8, np.float32)
    if case.startswith("scale-"):
        s[5] = dict(inf=np.inf, nan=np.nan, zero=0.0, negative=-1.0)[case[6:]]
    rc, msg = _add(lm, name, N, K, s[:2] if case == "n_scale" else s)
    assert rc == (L.E_UNSUPPORTED if case in ("N%64", "K%64", "K>131072") else L.E_INVALID) and name in msg, (rc, msg)
    assert _add(lm, name, 128, 128, np.full(128, 2.0 ** -8, np.float32))[0] == L.OK      # nothing was kept of the refused tensor


@pytest.mark.parametrize("arch", ["mamba2", "deepseek2"])
def test_int8_tensors_outside_the_llama_family_are_refused_at_finalize(device, arch):
    lm = runtime.LoadedModel(device, synth.make_mamba_config("tiny-mamba2") if arch == "mamba2" else synth.make_dsv2_config("tiny-dsv2"))
    name = "backbone.layers.0.mixer.out_proj.weight" if arch == "mamba2" else "model.layers.0.self_attn.o_proj.weight"
    assert _add(lm, name, 256, 512, np.ones(1, np.float32))[0] == L.OK
    rc = L.lib().bz_model_finalize(lm.h)
    msg = L.lib().bz_last_error().decode()
    assert rc == L.E_UNSUPPORTED and name in msg, (rc, msg)


def test_int8_lm_head_is_refused_at_finalize(device):
    model = I.make("tiny-int8-channel-bf16", tie_embeddings=False)
    model["lm_head"] = synth.int8_linear("lm_head", model["config"]["vocab"], model["config"]["hidden"], "channel")
    with pytest.raises(L.BlazrHipError) as ex:
        runtime.LoadedModel.from_synth(device, model)
    assert ex.value.code == L.E_UNSUPPORTED and "lm_head.weight" in str(ex.value)


def test_four_row_paged_batch_gives_the_per_sequence_tokens(device):
    """prompts of different lengths, then five batched steps over a paged pool: the four rows together give the tokens each sequence gives as a batch of its own
    (the same kernels; a row depends on nothing in the other rows)"""
    model, lm = _pair(device, "tiny-int8-channel-bf16")
    cfg, nseq, bs, per = model["config"], 4, 16, 4
    tables = [[i + nseq * j for j in range(per)] for i in range(nseq)]
    prompts = [synth.prompt_tokens(3 + (11 * i) % 40, cfg["vocab"], seed=40 + i) for i in range(nseq)]

    def run(seqs):
        pool = runtime.LayeredPagedKvCache(device, cfg["n_layers"], nseq * per, bs, cfg["n_kv_heads"], cfg["head_dim"], _kv_dt(cfg))
        slot = lambda i, k: tables[i][k // bs] * bs + k % bs
        toks = [int(lm.forward_with_paged_kv_cache(prompts[i], pool, [slot(i, k) for k in range(len(prompts[i]))], tables[i], len(prompts[i]), 0).to_numpy()[0].argmax()) for i in seqs]
        lens, out = [len(prompts[i]) for i in seqs], []
        for step in range(5):
            out.append(toks)
            lens = [n + 1 for n in lens]
            got = lm.forward_paged_batch(toks, pool, [slot(i, n - 1) for n, i in zip(lens, seqs)], [tables[i][:(n + bs - 1) // bs] for n, i in zip(lens, seqs)], lens).to_numpy()
            toks = [int(r.argmax()) for r in got]
        return np.array(out + [toks]).T.tolist()

    assert run([0, 1, 2, 3]) == [run([i])[0] for i in range(nseq)]


def test_engine_run_gives_each_request_its_own_greedy_tokens(device):
    """tests/test_gpu_engine.py's protocol: 4 rows, 6 requests of 8 tokens coming and going; every request's tokens equal those of its alone run on an engine of
    the same configuration"""
    model, lm = _pair(device, "tiny-int8-channel-bf16")
    prompts = [synth.prompt_tokens(3 + (13 * i) % 30, model["config"]["vocab"], seed=70 + i) for i in range(6)]
    mk = lambda: runtime.BatchEngine(lm, 4, 4 * 5 + 4, 16, 80, 0, 2, False)
    ids, res, _ = _drive(mk(), [(0 if i < 4 else 2 + i, dict(prompt=p, max_tokens=8)) for i, p in enumerate(prompts)])
    for i, rid in enumerate(ids):
        (aid,), ares, _ = _drive(mk(), [(0, dict(prompt=prompts[i], max_tokens=8))])
        assert res[rid]["tokens"] == ares[aid]["tokens"] and len(res[rid]["tokens"]) == 8 and res[rid]["reason"] == 0, i
