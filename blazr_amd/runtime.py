"""Host-side mirror of the boostr surface blazr's engine calls, over the C-ABI.

Names and argument meaning follow the reference so that parity tests read like the reference's call sites:

* ``LoadedModel.forward_with_kv_cache(input, kv, position)``      /root/reference/src/engine/executor_generate.rs:357,372
* ``LoadedModel.forward_with_paged_kv_cache(input, cache, slot_mapping, block_table, seq_len_k, start_pos)``  :259-262
* ``LoadedModel.forward_embed / forward_layers_range / forward_head``  /root/reference/src/cli/swarm_forward.rs:205,239-263
* ``LayeredKvCache.new_positional(...)``, ``LayeredPagedKvCache(...)``  executor_generate.rs:350-353, :208-210
* ``logits_to_token(...)``  /root/reference/src/engine/sampling.rs:445-460
* ``Executor.generate``  executor_generate.rs:341-410 (the loop itself runs in C++: ``bz_generate`` / ``bz_generate_grammar``)
* ``GrammarDfa`` / ``DeviceGrammarDfa``  /root/reference/src/engine/grammar.rs:21-159, sampling.rs:415-419

All compute happens in libblazr_hip.so on the GPU; numpy arrays are only the host view of inputs/outputs.
"""
import ctypes as C
import json
import os
import warnings

import numpy as np

from . import _lib as L

_NP2BZ = {np.dtype(np.float32): L.F32, np.dtype(np.float16): L.F16, np.dtype(np.int64): L.I64, np.dtype(np.int32): L.I32,
          np.dtype(np.uint32): L.U32, np.dtype(np.uint8): L.U8}
_BZ2NP = {L.F32: np.float32, L.F16: np.float16, L.BF16: np.uint16, L.I64: np.int64, L.I32: np.int32, L.U32: np.uint32, L.U8: np.uint8}
_DT = {"f32": L.F32, "f16": L.F16, "bf16": L.BF16}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Device:
    """boostr::CudaDevice::new(id) + CudaClient (cli/run.rs:70-81)."""

    def __init__(self, device_id=0):
        h = C.c_void_p()
        L.check(L.lib().bz_device_open(device_id, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            L.lib().bz_device_close(self.h)
            self.h = None

    def synchronize(self):
        L.check(L.lib().bz_device_synchronize(self.h))

    def memory_info(self):
        f, t = C.c_size_t(), C.c_size_t()
        L.check(L.lib().bz_device_memory_info(self.h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def name(self):
        b = C.create_string_buffer(256)
        L.check(L.lib().bz_device_name(self.h, b, 256))
        return b.value.decode()

    def stream(self):
        return L.lib().bz_device_stream(self.h)

    # Tensor::from_slice / zeros
    def tensor(self, array, dtype=None):
        a = np.ascontiguousarray(array)
        dt = dtype if dtype is not None else _NP2BZ[a.dtype]
        shape = (C.c_int64 * max(a.ndim, 1))(*(a.shape if a.ndim else (1,)))
        h = C.c_void_p()
        L.check(L.lib().bz_tensor_from_host(self.h, dt, shape, max(a.ndim, 1), _ptr(a), C.byref(h)))
        return Tensor(self, h, dt, tuple(a.shape) if a.ndim else (1,))

    def zeros(self, shape, dtype=L.F32):
        shape = tuple(int(s) for s in shape)
        sh = (C.c_int64 * len(shape))(*shape)
        h = C.c_void_p()
        L.check(L.lib().bz_tensor_zeros(self.h, dtype, sh, len(shape), C.byref(h)))
        return Tensor(self, h, dtype, shape)

    def record_event(self):
        ev = C.c_uint64()
        L.check(L.lib().bz_event_record(self.h, C.byref(ev)))
        return ev.value


class Tensor:
    def __init__(self, dev, h, dtype, shape):
        self.dev, self.h, self.dtype, self.shape = dev, h, dtype, shape

    def __del__(self):
        try:
            if self.h and L.alive:
                L.lib().bz_tensor_free(self.h)
        except Exception:
            pass

    def to_numpy(self):
        out = np.empty(self.shape, dtype=_BZ2NP[self.dtype])
        L.check(L.lib().bz_tensor_to_host(self.h, _ptr(out), out.nbytes))
        return out

    to_vec = to_numpy

    def copy_from(self, array):
        a = np.ascontiguousarray(array, dtype=_BZ2NP[self.dtype])
        L.check(L.lib().bz_tensor_copy_from_host(self.h, _ptr(a), a.nbytes))

    def to_vec_pipelined(self, event):
        out = np.empty(self.shape, dtype=_BZ2NP[self.dtype])
        L.check(L.lib().bz_tensor_to_host_pipelined(self.h, event, _ptr(out), out.nbytes))
        return out


def make_config(cfg):
    """synth/HF-style config dict -> bz_model_config POD."""
    c = L.ModelConfig()
    c.abi_version = L.ABI_VERSION
    # sliding-window attention (Llama family only; bz_model_create refuses it on the other architectures): 0 / absent = full attention
    c.sliding_window = int(cfg.get("sliding_window") or 0)
    c.sliding_window_pattern = int(cfg.get("sliding_window_pattern") or 0)
    if cfg.get("arch") == "mamba2":
        # SsmConfig (loader/gguf.rs:219-262)
        c.arch = L.ARCH_MAMBA2
        for k in ("hidden", "n_layers", "vocab", "max_seq_len"):
            setattr(c, k, int(cfg[k]))
        for k in ("d_inner", "n_heads", "head_dim", "d_state", "n_groups", "conv_kernel"):
            setattr(c, "ssm_" + k, int(cfg[k]))
        c.rms_eps = cfg["rms_eps"]
        c.act_dtype = _DT[cfg["act_dtype"]]
        c.tie_embeddings = int(bool(cfg.get("tie_embeddings")))
        return c
    if cfg.get("arch") == "deepseek2":
        # AttentionConfig kv_latent_dim / q_latent_dim / d_rope (loader/gguf.rs:188-196), MoeConfig (loader/gguf.rs:271-283)
        c.arch = L.ARCH_DEEPSEEK2
        for k in ("hidden", "n_layers", "n_heads", "vocab", "max_seq_len", "inter"):
            setattr(c, k, int(cfg[k]))
        for k in ("kv_lora_rank", "q_lora_rank", "nope_dim", "rope_dim", "v_dim"):
            setattr(c, "mla_" + k, int(cfg[k]))
        c.moe_n_experts, c.moe_top_k, c.moe_n_shared = int(cfg["n_experts"]), int(cfg["top_k"]), int(cfg["n_shared"])
        c.moe_inter, c.moe_first_dense, c.moe_norm_topk = int(cfg["moe_inter"]), int(cfg["first_dense"]), int(bool(cfg["norm_topk"]))
        c.moe_routed_scale = float(cfg["routed_scale"])
        c.rms_eps = cfg["rms_eps"]
        c.act_dtype = _DT[cfg["act_dtype"]]
        c.tie_embeddings = int(bool(cfg.get("tie_embeddings")))
        c.rope_theta = cfg["rope_theta"]
        c.rope_interleaved = 1
        _rope_scaling_to_config(cfg, c)
        return c
    c.arch = L.ARCH_LLAMA
    for k in ("hidden", "n_layers", "n_heads", "n_kv_heads", "head_dim", "inter", "vocab", "max_seq_len"):
        setattr(c, k, int(cfg[k]))
    c.rms_eps = cfg["rms_eps"]
    c.act_dtype = _DT[cfg["act_dtype"]]
    c.tie_embeddings = int(bool(cfg.get("tie_embeddings")))
    c.rope_theta = cfg["rope_theta"]
    c.rope_interleaved = int(cfg.get("rope_interleaved", 0))
    _rope_scaling_to_config(cfg, c)
    return c


def yarn_mscale(factor, mscale=1.0):
    """HF yarn_get_mscale"""
    import math
    return 1.0 if factor <= 1.0 else 0.1 * mscale * math.log(factor) + 1.0


def _rope_scaling_to_config(cfg, c):
    """rope_scaling dict (HF config.json names) -> the bz_model_config fields (loader/safetensors/config.rs:83-95)"""
    rs = cfg.get("rope_scaling") or {}
    c.rope_scaling = {"none": L.ROPE_NONE, "linear": L.ROPE_LINEAR, "llama3": L.ROPE_LLAMA3, "yarn": L.ROPE_YARN}[rs.get("type", "none")]
    c.rope_factor = rs.get("factor", 1.0)
    c.rope_low_freq_factor = rs.get("low_freq_factor", 1.0)
    c.rope_high_freq_factor = rs.get("high_freq_factor", 4.0)
    c.rope_original_max_pos = rs.get("original_max_position_embeddings", 8192)
    c.rope_beta_fast, c.rope_beta_slow = rs.get("beta_fast", 0.0), rs.get("beta_slow", 0.0)
    c.rope_attn_factor, c.mla_softmax_mscale = 0.0, 0.0
    if rs.get("type") == "yarn":
        if "attention_factor" in rs:
            c.rope_attn_factor = rs["attention_factor"]
        elif "mscale" in rs and "mscale_all_dim" in rs:      # DeepSeek-V2: cos / sin by mscale / mscale_all_dim, softmax scale by mscale_all_dim^2
            c.rope_attn_factor = yarn_mscale(c.rope_factor, rs["mscale"]) / yarn_mscale(c.rope_factor, rs["mscale_all_dim"])
        if cfg.get("arch") == "deepseek2" and rs.get("mscale_all_dim"):
            c.mla_softmax_mscale = yarn_mscale(c.rope_factor, rs["mscale_all_dim"])


_AWQ_SHIFTS = np.array([0, 16, 4, 20, 8, 24, 12, 28], dtype=np.uint32)  # awq.rs:32


def unpack_awq_zeros(qzeros, N):
    """awq.rs:239-263: packed [G, N/8] -> f32 [G, N] (what DecomposedQuantTensor carries)."""
    qz = np.ascontiguousarray(qzeros, dtype=np.uint32)
    return ((qz[:, :, None] >> _AWQ_SHIFTS[None, None, :]) & 0xF).reshape(qz.shape[0], N).astype(np.float32)


class LoraAdapter:
    """engine/lora.rs LoraAdapter on the device: rank, alpha and one (lora_A [r, in], lora_B [out, r]) pair per adapted linear, at their stored dtype
    (float16 / float32 arrays, uint16 arrays = bf16 bits)."""

    def __init__(self, dev, h):
        self.dev, self.h = dev, h

    @classmethod
    def from_arrays(cls, dev, rank, alpha, pairs, use_rslora=False):
        """pairs: {"model.layers.3.self_attn.q_proj": (A, B)}"""
        h = C.c_void_p()
        L.check(L.lib().bz_lora_create(dev.h, int(rank), float(alpha), int(bool(use_rslora)), C.byref(h)))
        self = cls(dev, h)
        for key, (A, B) in pairs.items():
            a, b = np.ascontiguousarray(A), np.ascontiguousarray(B)
            if a.dtype != b.dtype or a.ndim != 2 or b.ndim != 2:
                raise ValueError("lora pair %s: A and B must be 2-D arrays of one dtype" % key)
            dt = L.BF16 if a.dtype == np.uint16 else _NP2BZ[a.dtype]
            L.check(L.lib().bz_lora_add(h, key.encode(), dt, _ptr(a), (C.c_int64 * 2)(*a.shape), _ptr(b), (C.c_int64 * 2)(*b.shape)))
        return self

    @classmethod
    def load(cls, dev, path):
        """load_lora_adapter (engine/lora.rs:138-257): a PEFT directory or its adapter_model.safetensors"""
        h = C.c_void_p()
        L.check(L.lib().bz_lora_load(dev.h, str(path).encode(), C.byref(h)))
        return cls(dev, h)

    def __del__(self):
        try:
            if self.h and L.alive:
                L.lib().bz_lora_free(self.h)     # refused while a slot holds it: the model that holds it frees its table first
        except Exception:
            pass


def lora_describe(path):
    """bz_lora_describe: the loader's rules on the host alone -> dict(rank, alpha, use_rslora, scaling, pairs)"""
    need = C.c_size_t(0)
    L.check(L.lib().bz_lora_describe(str(path).encode(), None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    L.check(L.lib().bz_lora_describe(str(path).encode(), buf, need.value, None))
    return json.loads(buf.value.decode())


def _lora_mask(targets):
    if isinstance(targets, int):
        return targets
    if isinstance(targets, str):
        targets = [t for t in targets.split(",") if t]
    return sum(L.LORA_TARGETS[t.strip().replace("_proj", "")] for t in set(targets))


class LoadedModel:
    """boostr::model::LoadedModel<R> behind the C-ABI."""

    def __init__(self, dev, cfg):
        self.dev = dev
        self.cfg = dict(cfg)
        self.c = make_config(cfg)
        h = C.c_void_p()
        L.check(L.lib().bz_model_create(dev.h, C.byref(self.c), C.byref(h)))
        self.h = h
        self.finalized = False
        self._shapes = {}
        self._loras = {}          # name -> (slot, LoraAdapter): LoraAdapterRegistry (executor.rs:397-420)
        self._lora_slots = 0

    def __del__(self):
        try:
            if self.h and L.alive:
                L.lib().bz_model_free(self.h)
        except Exception:
            pass

    # --- LoRA: Executor::load_lora / unload_lora / list_loras (executor.rs:397-420), GenerationConfig.lora_adapter ------------------
    def enable_lora(self, n_slots=8, max_rank=64, targets=("q", "v")):
        """Once, after finalize and before any graph capture / engine that should apply adapters.  targets: names out of q, k, v, o, gate, up, down."""
        cfg = L.LoraTableConfig()
        cfg.n_slots, cfg.max_rank, cfg.targets = int(n_slots), int(max_rank), _lora_mask(targets)
        L.check(L.lib().bz_lora_table_create(self.h, C.byref(cfg)))
        self._lora_slots = int(n_slots)

    def load_lora(self, source, name):
        """source: a PEFT directory / adapter_model.safetensors, or a LoraAdapter.  An insert under an existing name replaces it.  Returns the slot."""
        adapter = source if isinstance(source, LoraAdapter) else LoraAdapter.load(self.dev, source)
        if name in self._loras:
            self.unload_lora(name)
        used = {slot for slot, _ in self._loras.values()}
        free = [i for i in range(self._lora_slots) if i not in used]
        if not free:
            raise L.BlazrHipError(L.E_INVALID, "load_lora: all %d slots are in use" % self._lora_slots)
        L.check(L.lib().bz_lora_attach(self.h, free[0], adapter.h))
        self._loras[name] = (free[0], adapter)
        return free[0]

    def unload_lora(self, name):
        if name not in self._loras:
            return False
        L.check(L.lib().bz_lora_detach(self.h, self._loras[name][0]))
        del self._loras[name]
        return True

    def list_loras(self):
        return sorted(self._loras)

    def lora_slot(self, name):
        """slot of a registered name; None -> -1"""
        return -1 if name is None else self._loras[name][0]

    def set_lora(self, name):
        """the adapter every following single-sequence step runs under (None: the base model); a decode graph captured earlier follows"""
        L.check(L.lib().bz_model_set_lora(self.h, self.lora_slot(name)))

    def lora_apply(self, layer, targets, x, base, row_slots, form=0):
        """op level: the shrink + expand kernels on rows of one fused group (bz_lora_apply)"""
        x, base = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(base, np.float32)
        rows = x.shape[0]
        tx, tb, ty = self.dev.tensor(x), self.dev.tensor(base), self.dev.zeros(base.shape)
        sl = np.ascontiguousarray(row_slots, dtype=np.int32)
        L.check(L.lib().bz_lora_apply(self.h, int(layer), _lora_mask(targets), tx.h, tb.h, _ptr(sl), rows, int(form), ty.h))
        return ty.to_numpy()

    # --- VarMap::insert / insert_decomposed_quant ---------------------------------------------------------
    def add_dense(self, name, array):
        a = np.ascontiguousarray(array)
        dt = L.BF16 if a.dtype == np.uint16 else _NP2BZ[a.dtype]
        shape = (C.c_int64 * a.ndim)(*a.shape)
        L.check(L.lib().bz_model_add_dense(self.h, name.encode(), dt, shape, a.ndim, _ptr(a)))

    def add_linear(self, base, spec):
        """`spec` in the loader formats of blazr_amd.synth (== what awq.rs / gptq.rs / regular.rs produce)."""
        name = (base + ".weight").encode()
        kind = spec["kind"]
        self._shapes[base + ".weight"] = (int(spec["N"]), int(spec["K"]))
        if kind == "dense":
            self.add_dense(base + ".weight", spec["weight"])
        elif kind == "awq":
            qw = np.ascontiguousarray(spec["qweight"], dtype=np.uint32)
            sc = np.ascontiguousarray(spec["scales"]).astype(np.float32)            # awq.rs:202-206 f16 -> f32
            zf = unpack_awq_zeros(spec["qzeros"], spec["N"])                        # awq.rs:208-213
            L.check(L.lib().bz_model_add_awq(self.h, name, spec["N"], spec["K"], _ptr(qw), _ptr(sc), _ptr(zf), spec["group_size"]))
        elif kind == "gptq":
            qw = np.ascontiguousarray(spec["qweight"], dtype=np.uint32)
            sc = np.ascontiguousarray(spec["scales"]).astype(np.float32)
            qz = np.ascontiguousarray(spec["qzeros"], dtype=np.uint32)              # kept packed (gptq.rs:209-219)
            gi = None if spec.get("g_idx") is None else np.ascontiguousarray(spec["g_idx"], dtype=np.int32)
            bi = None if spec.get("bias") is None else np.ascontiguousarray(spec["bias"]).astype(np.float32)
            L.check(L.lib().bz_model_add_gptq(self.h, name, spec["N"], spec["K"], _ptr(qw), _ptr(sc), _ptr(qz),
                                              None if gi is None else _ptr(gi), None if bi is None else _ptr(bi), spec["group_size"]))
        elif kind == "gguf":
            b = np.ascontiguousarray(spec["blocks"], dtype=np.uint8)
            L.check(L.lib().bz_model_add_gguf(self.h, name, spec["ggml_type"], spec["N"], spec["K"], _ptr(b)))
        elif kind == "fp8":
            w = np.ascontiguousarray(spec["weight"], dtype=np.uint8)                # [N, K] e4m3 bytes
            sc = np.ascontiguousarray(spec["scale"], dtype=np.float32).reshape(-1)  # one per tensor or one per output row
            bi = None if spec.get("bias") is None else np.ascontiguousarray(spec["bias"], dtype=np.float32)
            L.check(L.lib().bz_model_add_fp8(self.h, name, spec["N"], spec["K"], _ptr(w), _ptr(sc), sc.size, None if bi is None else _ptr(bi)))
        elif kind == "mxfp4":
            w = np.ascontiguousarray(spec["weight"], dtype=np.uint8)                # [N, K/2] two E2M1 codes per byte, low nibble first
            sc = np.ascontiguousarray(spec["scale"], dtype=np.uint8)                # [N, K/32] E8M0 codes
            bi = None if spec.get("bias") is None else np.ascontiguousarray(spec["bias"], dtype=np.float32)
            L.check(L.lib().bz_model_add_mxfp4(self.h, name, spec["N"], spec["K"], _ptr(w), _ptr(sc), None if bi is None else _ptr(bi)))
        else:
            raise ValueError(kind)

    def add_llama_layer(self, i, lay):
        p = "model.layers.%d." % i
        self.add_dense(p + "input_layernorm.weight", np.asarray(lay["attn_norm"], dtype=np.float32))
        self.add_dense(p + "post_attention_layernorm.weight", np.asarray(lay["ffn_norm"], dtype=np.float32))
        for short, hf in (("q", "self_attn.q_proj"), ("k", "self_attn.k_proj"), ("v", "self_attn.v_proj"), ("o", "self_attn.o_proj"),
                          ("gate", "mlp.gate_proj"), ("up", "mlp.up_proj"), ("down", "mlp.down_proj")):
            self.add_linear(p + hf, lay[short])

    def add_llama_head(self, embed, final_norm, lm_head):
        self.add_dense("model.embed_tokens.weight", embed)
        self.add_dense("model.norm.weight", np.asarray(final_norm, dtype=np.float32))
        if not self.cfg.get("tie_embeddings"):
            self.add_linear("lm_head", lm_head)

    def add_dsv2_layer(self, i, lay):
        """HF DeepSeek-V2 tensor names"""
        p = "model.layers.%d." % i
        f32 = lambda a: np.asarray(a, dtype=np.float32)
        self.add_dense(p + "input_layernorm.weight", f32(lay["attn_norm"]))
        self.add_dense(p + "post_attention_layernorm.weight", f32(lay["ffn_norm"]))
        self.add_dense(p + "self_attn.kv_a_layernorm.weight", f32(lay["kv_norm"]))
        ql = "q_b" in lay     # q_lora_rank > 0: q_a_proj -> q_a_layernorm -> q_b_proj
        for short, hf in (("q_proj", "self_attn.q_a_proj" if ql else "self_attn.q_proj"), ("kv_a", "self_attn.kv_a_proj_with_mqa"), ("kv_b", "self_attn.kv_b_proj"),
                          ("o", "self_attn.o_proj")):
            self.add_linear(p + hf, lay[short])
        if ql:
            self.add_dense(p + "self_attn.q_a_layernorm.weight", f32(lay["q_norm"]))
            self.add_linear(p + "self_attn.q_b_proj", lay["q_b"])
        if not lay["is_moe"]:
            for n in ("gate", "up", "down"):
                self.add_linear(p + "mlp.%s_proj" % n, lay[n])
        else:
            self.add_linear(p + "mlp.gate", lay["router"])
            for e, ex in enumerate(lay["experts"]):
                for n in ("gate", "up", "down"):
                    self.add_linear(p + "mlp.experts.%d.%s_proj" % (e, n), ex[n])
            if "shared" in lay:
                for n in ("gate", "up", "down"):
                    self.add_linear(p + "mlp.shared_experts.%s_proj" % n, lay["shared"][n])

    def add_mamba2_layer(self, i, lay):
        """HF Mamba2 tensor names (backbone.layers.{i}.mixer.*)"""
        p = "backbone.layers.%d." % i
        f32 = lambda a: np.asarray(a, dtype=np.float32)
        self.add_dense(p + "norm.weight", f32(lay["norm"]))
        self.add_linear(p + "mixer.in_proj", lay["in_proj"])
        cw = f32(lay["conv_w"])
        self.add_dense(p + "mixer.conv1d.weight", cw.reshape(cw.shape[0], 1, cw.shape[1]))
        self.add_dense(p + "mixer.conv1d.bias", f32(lay["conv_b"]))
        self.add_dense(p + "mixer.dt_bias", f32(lay["dt_bias"]))
        self.add_dense(p + "mixer.A_log", f32(lay["A_log"]))
        self.add_dense(p + "mixer.D", f32(lay["D"]))
        self.add_dense(p + "mixer.norm.weight", f32(lay["gnorm"]))
        self.add_linear(p + "mixer.out_proj", lay["out_proj"])

    def add_mamba2_head(self, embed, final_norm, lm_head):
        self.add_dense("backbone.embeddings.weight", embed)
        self.add_dense("backbone.norm_f.weight", np.asarray(final_norm, dtype=np.float32))
        if not self.cfg.get("tie_embeddings"):
            self.add_linear("lm_head", lm_head)

    @classmethod
    def from_synth(cls, dev, model):
        """Whole in-memory model dict (blazr_amd.synth.make_llama / make_mamba2)."""
        m = cls(dev, model["config"])
        if model["config"].get("arch") == "deepseek2":
            for i, lay in enumerate(model["layers"]):
                m.add_dsv2_layer(i, lay)
            m.add_llama_head(model["embed"], model["final_norm"], model["lm_head"])
            m.finalize()
            return m
        if model["config"].get("arch") == "mamba2":
            for i, lay in enumerate(model["layers"]):
                m.add_mamba2_layer(i, lay)
            m.add_mamba2_head(model["embed"], model["final_norm"], model["lm_head"])
            m.finalize()
            return m
        for i, lay in enumerate(model["layers"]):
            m.add_llama_layer(i, lay)
        m.add_llama_head(model["embed"], model["final_norm"], model["lm_head"])
        m.finalize()
        return m

    @classmethod
    def from_synth_streamed(cls, dev, cfg, seed=None):
        """Generate + upload layer by layer (bounded host memory) -- used for the 8B bench shape."""
        from . import synth
        kw = {} if seed is None else {"seed": seed}
        m = cls(dev, cfg)
        if cfg.get("arch") == "deepseek2":
            for i in range(cfg["n_layers"]):
                m.add_dsv2_layer(i, synth.dsv2_layer(cfg, i, **kw))
            emb, fn, lm = synth.dsv2_head(cfg, **kw)
            m.add_llama_head(emb, fn, lm)
            m.finalize()
            return m
        if cfg.get("arch") == "mamba2":
            for i in range(cfg["n_layers"]):
                m.add_mamba2_layer(i, synth.mamba2_layer(cfg, i, **kw))
            emb, fn, lm = synth.mamba2_head(cfg, **kw)
            m.add_mamba2_head(emb, fn, lm)
            m.finalize()
            return m
        for i in range(cfg["n_layers"]):
            m.add_llama_layer(i, synth.llama_layer(cfg, i, **kw))
        emb, fn, lm = synth.llama_head(cfg, **kw)
        m.add_llama_head(emb, fn, lm)
        m.finalize()
        return m

    def finalize(self):
        L.check(L.lib().bz_model_finalize(self.h))
        self.finalized = True

    # --- accessors (LoadedModel::num_layers etc.) ---------------------------------------------------------
    def num_layers(self):
        return self.c.n_layers

    def num_kv_heads(self):
        return 1 if self.c.arch == L.ARCH_DEEPSEEK2 else self.c.n_kv_heads

    def head_dim(self):
        return self.c.mla_kv_lora_rank + self.c.mla_rope_dim if self.c.arch == L.ARCH_DEEPSEEK2 else self.c.head_dim

    def hidden_size(self):
        return self.c.hidden

    def vocab_size(self):
        return self.c.vocab

    def needs_kv_cache(self):
        return self.c.arch != L.ARCH_MAMBA2

    def needs_ssm_state(self):
        return self.c.arch == L.ARCH_MAMBA2

    def moe_config(self):
        if self.c.arch != L.ARCH_DEEPSEEK2 or self.c.moe_n_experts == 0:
            return None
        return dict(num_experts=self.c.moe_n_experts, experts_per_tok=self.c.moe_top_k, shared_experts=self.c.moe_n_shared)

    def new_kv_cache(self, capacity, max_seq_len=None):
        """LayeredKvCache::new_positional with this model's cache shape (for MLA: one 'head' of kv_lora_rank + rope_dim latents)"""
        dt = self.c.act_dtype
        return LayeredKvCache(self.dev, self.c.n_layers, 1, self.num_kv_heads(), capacity, max_seq_len or self.c.max_seq_len, self.head_dim(), dt)

    def mamba_config(self):
        if self.c.arch != L.ARCH_MAMBA2:
            return None
        return {k: getattr(self.c, "ssm_" + k) for k in ("d_inner", "n_heads", "head_dim", "d_state", "n_groups", "conv_kernel")}

    def weight_bytes(self):
        a, b = C.c_size_t(), C.c_size_t()
        L.check(L.lib().bz_model_weight_bytes(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def rope_caches(self):
        n = self.c.max_seq_len * (self.c.head_dim // 2)
        c, s = np.empty(n, np.float32), np.empty(n, np.float32)
        L.check(L.lib().bz_rope_caches(self.h, _ptr(c), _ptr(s)))
        return c.reshape(self.c.max_seq_len, -1), s.reshape(self.c.max_seq_len, -1)

    # --- forward --------------------------------------------------------------------------------------------
    def _tokens(self, tokens):
        if isinstance(tokens, Tensor):
            return tokens, int(np.prod(tokens.shape))
        t = np.ascontiguousarray(tokens, dtype=np.int64).reshape(-1)
        return self.dev.tensor(t), len(t)

    def forward_with_kv_cache(self, tokens, kv, position, all_logits=False):
        t, S = self._tokens(tokens)
        out = self.dev.zeros((S if all_logits else 1, self.c.vocab), L.F32)
        L.check(L.lib().bz_forward_kv(self.h, t.h, S, kv.h, position, out.h, L.FWD_ALL_LOGITS if all_logits else 0))
        return out

    def forward_kv_verify(self, tokens, kv, position, want_logits=True):
        """Speculative verify (bz_forward_kv_verify): tokens = [last committed token, draft tokens ...] at `position`.  Returns (n_accept, tokens[0 .. n_accept], path,
        logits F32 [R, vocab] device tensor or None); the cache ends at position + n_accept + 1."""
        t, R = self._tokens(tokens)
        out = self.dev.zeros((R, self.c.vocab), L.F32) if want_logits else None
        na, path = C.c_int32(), C.c_int32()
        toks = np.full(R, -1, dtype=np.int64)
        L.check(L.lib().bz_forward_kv_verify(self.h, t.h, R, kv.h, position, out.h if out is not None else None, C.byref(na), _ptr(toks), C.byref(path)))
        return na.value, toks[:na.value + 1].copy(), path.value, out

    def forward_with_paged_kv_cache(self, tokens, cache, slot_mapping, block_table, seq_len_k, start_pos, all_logits=False):
        t, S = self._tokens(tokens)
        sm = slot_mapping if isinstance(slot_mapping, Tensor) else self.dev.tensor(np.asarray(slot_mapping, dtype=np.int32))
        bt = block_table if isinstance(block_table, Tensor) else self.dev.tensor(np.asarray(block_table, dtype=np.int32).reshape(-1))
        out = self.dev.zeros((S if all_logits else 1, self.c.vocab), L.F32)
        L.check(L.lib().bz_forward_paged(self.h, t.h, S, cache.h, sm.h, bt.h, int(np.prod(bt.shape)), seq_len_k, start_pos, out.h,
                                         L.FWD_ALL_LOGITS if all_logits else 0))
        return out

    def forward_with_ssm_state(self, tokens, ssm, all_logits=False):
        """LoadedModel::forward_with_ssm_state (executor_generate.rs:137,148)"""
        t, S = self._tokens(tokens)
        out = self.dev.zeros((S if all_logits else 1, self.c.vocab), L.F32)
        L.check(L.lib().bz_forward_ssm(self.h, t.h, S, ssm.h, out.h, L.FWD_ALL_LOGITS if all_logits else 0))
        return out

    def forward_paged_batch(self, tokens, cache, slot_mapping, block_tables, seq_lens):
        """process_decode_batch (batch_decode.rs:35-150): tokens [N], slots [N], block_tables [N][<= max_blocks] (ragged ok), seq_lens [N]"""
        t, n = self._tokens(tokens)
        nb = max(len(b) for b in block_tables)
        bt = np.zeros((n, nb), dtype=np.int32)
        for i, b in enumerate(block_tables):
            bt[i, :len(b)] = b                                    # shorter tables padded with 0 (batch_decode.rs:118-126)
        sm, btt = self.dev.tensor(np.asarray(slot_mapping, dtype=np.int32)), self.dev.tensor(bt)
        sl = np.asarray(seq_lens, dtype=np.int32)
        out = self.dev.zeros((n, self.c.vocab), L.F32)
        L.check(L.lib().bz_forward_paged_batch(self.h, t.h, n, cache.h, sm.h, btt.h, nb, sl.ctypes.data_as(C.c_void_p), out.h))
        return out

    def paged_attn_decode_rows(self, q, cache, layer, block_tables, seq_lens):
        """bz_paged_attn_decode_rows: the attention the batched decode step would launch for these rows, alone (batch_decode.rs:35-150).  q [N, n_heads, head_dim]
        roped and rounded, block_tables [N][<= max_blocks] (ragged ok, padded with 0; a 2-D array is taken as it is), seq_lens [N] -> f32 array [N, n_heads, hd]"""
        qa = np.ascontiguousarray(q, dtype=np.float32)
        n = qa.shape[0]
        if isinstance(block_tables, np.ndarray) and block_tables.ndim == 2:
            bt = np.ascontiguousarray(block_tables, dtype=np.int32)
        else:
            bt = np.zeros((n, max(len(b) for b in block_tables)), dtype=np.int32)
            for i, b in enumerate(block_tables):
                bt[i, :len(b)] = b
        sl = np.ascontiguousarray(seq_lens, dtype=np.int32)
        if bt.shape[0] != n or len(sl) != n:
            raise ValueError("paged_attn_decode_rows: %d rows, %d block tables, %d lengths" % (n, bt.shape[0], len(sl)))
        tq, tb, out = self.dev.tensor(qa), self.dev.tensor(bt), self.dev.zeros(qa.shape, L.F32)
        L.check(L.lib().bz_paged_attn_decode_rows(self.h, tq.h, cache.h, int(layer), tb.h, int(bt.shape[1]), sl.ctypes.data_as(C.c_void_p), n, out.h))
        return out.to_numpy().reshape(qa.shape)

    # --- scoring and embeddings (bz_score_* / bz_embed_*: a forward call whose rows go to a sink inside the library) ---------------------------------
    def _score(self, call, S, tokens, targets, top_logprobs):
        if targets is None:                                       # each token given its predecessors: row i reads the likelihood of token i + 1
            tk = tokens.to_numpy().reshape(-1) if isinstance(tokens, Tensor) else np.asarray(tokens, dtype=np.int64).reshape(-1)
            targets = np.concatenate([tk[1:], [-1]])
        tg = np.ascontiguousarray(targets, dtype=np.int64).reshape(-1)
        if len(tg) != S:
            raise ValueError("score: %d targets for %d tokens" % (len(tg), S))
        cfg = L.ScoreConfig(top_n=int(top_logprobs))
        rows, tot = (L.ScoreRow * S)(), L.ScoreTotal()
        L.check(call(_ptr(tg), C.byref(cfg), rows, C.byref(tot)))
        return score_result(rows, tot)

    def score(self, tokens, cache, position=0, targets=None, top_logprobs=0):
        """Log-likelihoods of given tokens from one prompt pass (echo + logprobs, perplexity, loglikelihood requests).  targets[i] is the token read from row i
        (-1: nothing); by default each token given its predecessors.  `cache`: a LayeredKvCache (at `position`: a continuation is a second call at
        position = len(context) on the same cache) or a LayeredSsmState.  -> dict(rows = SCORE_ROW array [S], sum_logprob, n_scored, perplexity = exp(-sum / n))."""
        t, S = self._tokens(tokens)
        if isinstance(cache, LayeredSsmState):
            return self._score(lambda tg, cfg, rows, tot: L.lib().bz_score_ssm(self.h, t.h, S, cache.h, tg, cfg, rows, tot), S, tokens, targets, top_logprobs)
        return self._score(lambda tg, cfg, rows, tot: L.lib().bz_score_kv(self.h, t.h, S, cache.h, int(position), tg, cfg, rows, tot), S, tokens, targets, top_logprobs)

    def score_paged(self, tokens, cache, slot_mapping, block_table, seq_len_k, start_pos, targets=None, top_logprobs=0):
        t, S = self._tokens(tokens)
        sm = slot_mapping if isinstance(slot_mapping, Tensor) else self.dev.tensor(np.asarray(slot_mapping, dtype=np.int32))
        bt = block_table if isinstance(block_table, Tensor) else self.dev.tensor(np.asarray(block_table, dtype=np.int32).reshape(-1))
        return self._score(lambda tg, cfg, rows, tot: L.lib().bz_score_paged(self.h, t.h, S, cache.h, sm.h, bt.h, int(np.prod(bt.shape)), seq_len_k, start_pos, tg, cfg,
                                                                             rows, tot), S, tokens, targets, top_logprobs)

    def _embed_out(self, S, pooling, normalize):
        if pooling not in L.POOLINGS:
            raise ValueError("embed: pooling %r (one of %s)" % (pooling, ", ".join(sorted(L.POOLINGS))))
        cfg = L.EmbedConfig(pooling=L.POOLINGS[pooling], normalize=int(bool(normalize)))
        return cfg, self.dev.zeros((S, self.c.hidden) if pooling == "none" else (self.c.hidden,), L.F32)

    def embed(self, tokens, cache, position=0, pooling="mean", normalize=False):
        """Contextual embedding of a prompt (/v1/embeddings): the rows the lm_head would read -- every layer and the final norm -- pooled ("mean", "cls", "last";
        "none": the rows themselves) and optionally L2-normalised.  -> f32 array [hidden] ([S, hidden] for "none").  `cache` as in score()."""
        t, S = self._tokens(tokens)
        cfg, out = self._embed_out(S, pooling, normalize)
        if isinstance(cache, LayeredSsmState):
            L.check(L.lib().bz_embed_ssm(self.h, t.h, S, cache.h, C.byref(cfg), out.h))
        else:
            L.check(L.lib().bz_embed_kv(self.h, t.h, S, cache.h, int(position), C.byref(cfg), out.h))
        return out.to_numpy().reshape(out.shape)

    # --- packed prompt batches: many inputs per pass (bz_embed_batch / bz_score_batch) ---------------------------------------------------------------
    def _packed(self, inputs, who):
        lens = np.asarray([len(x) for x in inputs], dtype=np.int32)
        if len(lens) == 0 or (lens <= 0).any():
            raise ValueError("%s: %d inputs, the shortest of %d tokens (at least one input, every input at least one token)" % (who, len(lens), int(lens.min()) if len(lens) else 0))
        flat = np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1) for x in inputs])
        return self.dev.tensor(flat), lens, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)

    def embed_batch(self, inputs, cache, pooling="mean", normalize=False):
        """embed() of many inputs in one prompt pass (/v1/embeddings with a list, /rerank): `inputs` is a list of token lists, `cache` a LayeredKvCache used as
        scratch (it must hold sum(len) rows; left reset).  -> f32 [n_seq, hidden]; "none": a list of [len_i, hidden].  A LayeredSsmState loops the single call."""
        if isinstance(cache, LayeredSsmState):
            res = []
            for x in inputs:
                cache.reset()
                res.append(self.embed(x, cache, pooling=pooling, normalize=normalize))
            return res if pooling == "none" else np.stack(res)
        t, lens, off = self._packed(inputs, "embed_batch")
        if pooling not in L.POOLINGS:
            raise ValueError("embed: pooling %r (one of %s)" % (pooling, ", ".join(sorted(L.POOLINGS))))
        cfg = L.EmbedConfig(pooling=L.POOLINGS[pooling], normalize=int(bool(normalize)))
        out = self.dev.zeros((int(off[-1]) if pooling == "none" else len(lens), self.c.hidden), L.F32)
        L.check(L.lib().bz_embed_batch(self.h, t.h, _ptr(lens), len(lens), cache.h, C.byref(cfg), out.h))
        a = out.to_numpy().reshape(out.shape)
        return [a[off[i]:off[i + 1]] for i in range(len(lens))] if pooling == "none" else a

    def score_batch(self, inputs, cache, targets=None, top_logprobs=0):
        """score() of many inputs in one prompt pass: `inputs` a list of token lists, `targets` None (each token given its predecessors inside its own input) or a
        list of per-input target lists.  -> a list of the dicts score() returns.  A LayeredSsmState loops the single call."""
        if isinstance(cache, LayeredSsmState):
            res = []
            for i, x in enumerate(inputs):
                cache.reset()
                res.append(self.score(x, cache, targets=None if targets is None else targets[i], top_logprobs=top_logprobs))
            return res
        t, lens, off = self._packed(inputs, "score_batch")
        T, n = int(off[-1]), len(lens)
        tg = None
        if targets is not None:
            tg = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1) for x in targets]), dtype=np.int64)
            if len(targets) != n or any(len(x) != k for x, k in zip(targets, lens)):
                raise ValueError("score_batch: targets must hold one list per input, of the input's length")
        cfg = L.ScoreConfig(top_n=int(top_logprobs))
        rows, tots = (L.ScoreRow * T)(), (L.ScoreTotal * n)()
        L.check(L.lib().bz_score_batch(self.h, t.h, _ptr(lens), n, cache.h, _ptr(tg) if tg is not None else None, C.byref(cfg), rows, tots))
        r = np.frombuffer(bytes(rows), dtype=SCORE_ROW).copy()
        res = []
        for i in range(n):
            ssum, k = float(tots[i].sum_logprob), int(tots[i].n_scored)
            res.append(dict(rows=r[off[i]:off[i + 1]], sum_logprob=ssum, n_scored=k, perplexity=float(np.exp(-ssum / k)) if k else float("nan")))
        return res

    def embed_paged(self, tokens, cache, slot_mapping, block_table, seq_len_k, start_pos, pooling="mean", normalize=False):
        t, S = self._tokens(tokens)
        sm = slot_mapping if isinstance(slot_mapping, Tensor) else self.dev.tensor(np.asarray(slot_mapping, dtype=np.int32))
        bt = block_table if isinstance(block_table, Tensor) else self.dev.tensor(np.asarray(block_table, dtype=np.int32).reshape(-1))
        cfg, out = self._embed_out(S, pooling, normalize)
        L.check(L.lib().bz_embed_paged(self.h, t.h, S, cache.h, sm.h, bt.h, int(np.prod(bt.shape)), seq_len_k, start_pos, C.byref(cfg), out.h))
        return out.to_numpy().reshape(out.shape)

    def forward_embed(self, tokens):
        t, S = self._tokens(tokens)
        out = self.dev.zeros((S, self.c.hidden), L.F32)
        L.check(L.lib().bz_forward_embed(self.h, t.h, S, out.h))
        return out

    def forward_layers_range(self, hidden, prev_mlp, kv, start, end, position):
        S = hidden.shape[0]
        has = C.c_int(0 if prev_mlp is None else 1)
        pm = prev_mlp if prev_mlp is not None else self.dev.zeros((S, self.c.hidden), L.F32)
        L.check(L.lib().bz_forward_layers_range(self.h, hidden.h, pm.h, C.byref(has), S, kv.h, start, end, position))
        return hidden, (pm if has.value else None)

    def forward_head(self, hidden, prev_mlp, all_logits=False):
        S = hidden.shape[0]
        out = self.dev.zeros((S if all_logits else 1, self.c.vocab), L.F32)
        L.check(L.lib().bz_forward_head(self.h, hidden.h, None if prev_mlp is None else prev_mlp.h, int(prev_mlp is not None), S, out.h,
                                        L.FWD_ALL_LOGITS if all_logits else 0))
        return out

    def profile_step(self, kv, token, position, iters=4):
        """per-kernel dispatch times of `iters` real decode steps (bz_profile_step)"""
        buf = (L.KernelTime * 32)()
        n = C.c_int()
        L.check(L.lib().bz_profile_step(self.h, kv.h, int(token), int(position), iters, buf, 32, C.byref(n)))
        return [dict(name=buf[i].name.decode(), launches=buf[i].launches, total_ms=buf[i].total_ms, algo_bytes=buf[i].algo_bytes)
                for i in range(n.value)]

    def profile_step_ssm(self, ssm, token, iters=4):
        buf = (L.KernelTime * 32)()
        n = C.c_int()
        L.check(L.lib().bz_profile_step_ssm(self.h, ssm.h, int(token), iters, buf, 32, C.byref(n)))
        return [dict(name=buf[i].name.decode(), launches=buf[i].launches, total_ms=buf[i].total_ms, algo_bytes=buf[i].algo_bytes)
                for i in range(n.value)]

    def layer_traits(self, layer):
        """bz_model_layer_traits: what the step plan reads of one layer, as an L.LayerTraits"""
        t = L.LayerTraits()
        L.check(L.lib().bz_model_layer_traits(self.h, int(layer), C.byref(t)))
        return t

    def layer_plan(self, layer, kv_dtype):
        """bz_model_layer_plan: the plan the decode step dispatches on for `layer` over a cache of kv_dtype (see layer_plan below)"""
        p = L.LayerPlan()
        L.check(L.lib().bz_model_layer_plan(self.h, int(layer), int(kv_dtype), C.byref(p)))
        return _plan_dict(p)

    # --- op-level ----------------------------------------------------------------------------------------------
    def quant_matmul(self, name, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        S = 1 if x.ndim == 1 else x.shape[0]
        xt = self.dev.tensor(x.reshape(S, -1))
        N = self.linear_shape(name)[0]
        y = self.dev.zeros((S, N), L.F32)
        L.check(L.lib().bz_quant_matmul(self.h, name.encode(), xt.h, S, y.h))
        return y.to_numpy()

    def linear_shape(self, name):
        return self._shapes[name]

    def conv1d_step(self, layer, state, zx):
        """ConvOps: the conv1d step (+ SiLU) of Mamba2 layer `layer` on the in_proj row zx; returns xbc [conv_dim]; the layer's conv window advances"""
        c = self.mamba_config()
        zt = self.dev.tensor(np.ascontiguousarray(zx, dtype=np.float32))
        out = self.dev.zeros((c["d_inner"] + 2 * c["n_groups"] * c["d_state"],), L.F32)
        L.check(L.lib().bz_conv1d_step(self.h, layer, state.h, zt.h, out.h))
        return out.to_numpy()

    def ssm_step(self, layer, state, zx):
        """the mixer's fused step (conv1d + SSM recurrence + gate) on the in_proj row zx; returns the gated y [d_inner]; conv window and SSM state advance"""
        c = self.mamba_config()
        zt = self.dev.tensor(np.ascontiguousarray(zx, dtype=np.float32))
        out = self.dev.zeros((c["d_inner"],), L.F32)
        L.check(L.lib().bz_ssm_step(self.h, layer, state.h, zt.h, out.h))
        return out.to_numpy()

    def ssm_scan_rows(self, layer, state, zx_rows, norm=True):
        """the prompt route's conv, scan and gated norm of Mamba2 layer `layer` on the in_proj rows zx_rows [S, d_in]; returns (xbc [S, conv_dim], gated y
        [S, d_inner], yn [S, d_inner] or None when norm is False); conv window and SSM state advance by S tokens"""
        c = self.mamba_config()
        zx = np.ascontiguousarray(zx_rows, dtype=np.float32)
        S = zx.shape[0]
        zt = self.dev.tensor(zx)
        xbc = self.dev.zeros((S, c["d_inner"] + 2 * c["n_groups"] * c["d_state"]), L.F32)
        y = self.dev.zeros((S, c["d_inner"]), L.F32)
        yn = self.dev.zeros((S, c["d_inner"]), L.F32) if norm else None
        L.check(L.lib().bz_ssm_scan_rows(self.h, layer, state.h, zt.h, S, xbc.h, y.h, None if yn is None else yn.h))
        return xbc.to_numpy(), y.to_numpy(), None if yn is None else yn.to_numpy()

    def moe_route(self, layer, hidden):
        """router of DeepSeek MoE layer `layer` on the residual-stream row (norm inside): (sel int32 [top_k + n_shared], w float32 [...], xn float32 [H])"""
        n = self.c.moe_top_k + self.c.moe_n_shared
        ht = self.dev.tensor(np.ascontiguousarray(hidden, dtype=np.float32))
        sel, w, xn = self.dev.zeros((n,), L.I32), self.dev.zeros((n,), L.F32), self.dev.zeros((self.c.hidden,), L.F32)
        L.check(L.lib().bz_moe_route(self.h, layer, ht.h, sel.h, w.h, xn.h))
        return sel.to_numpy(), w.to_numpy(), xn.to_numpy()

    def moe_grouped_gemv(self, layer, which, sel, x):
        """grouped expert GEMV: which 0 -> gate|up of experts sel[] on the shared row x [H]; which 1 -> down (SiLU*up prologue) on x [n_slots, 2 moe_inter]"""
        sel = np.ascontiguousarray(sel, dtype=np.int32)
        st = self.dev.tensor(sel, L.I32)
        xt = self.dev.tensor(np.ascontiguousarray(x, dtype=np.float32))
        N = 2 * self.c.moe_inter if which == 0 else self.c.hidden
        y = self.dev.zeros((len(sel), N), L.F32)
        L.check(L.lib().bz_moe_grouped_gemv(self.h, layer, which, st.h, len(sel), xt.h, y.h))
        return y.to_numpy()

    def dequant(self, name):
        N, K = self._shapes[name]
        out = np.empty((N, K), dtype=np.float32)
        L.check(L.lib().bz_dequant(self.h, name.encode(), _ptr(out)))
        return out


def detect_model_source(path):
    """loader/detect.rs:34-150 -> dict(format 'safetensors' | 'gguf', weights_path, config_path or None)"""
    s = L.ModelSource()
    L.check(L.lib().bz_detect_model_source(os.fsencode(path), C.byref(s)))
    return dict(format="gguf" if s.format == 1 else "safetensors", weights_path=os.fsdecode(s.weights_path),
                config_path=os.fsdecode(s.config_path) if s.has_config else None)


LAYER_TYPES = ["StandardTransformer", "Mamba2", "Mamba3", "MlaWithMoe", "MlaWithMlp"]


def detect_architecture_from_names(names):
    """boostr::model::detection::detect_architecture_from_names (tests: loader/safetensors/detect_arch.rs:200-315)"""
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    d = L.DetectedArch()
    L.check(L.lib().bz_detect_architecture_from_names(arr, len(names), C.byref(d)))
    return dict(format="HuggingFace" if d.format == 0 else "Oxidizr", num_layers=d.num_layers, tie_word_embeddings=bool(d.tie_word_embeddings),
                layer_types=[LAYER_TYPES[d.layer_types[i]] for i in range(d.num_layers)])


def config_from_hf_json(text):
    """HF config.json text -> (bz_model_config POD, dict(quant_method, group_size, torch_dtype))"""
    c, q = L.ModelConfig(), L.QuantInfo()
    L.check(L.lib().bz_config_from_hf_json(text.encode(), C.byref(c), C.byref(q)))
    return c, dict(quant_method={0: None, 1: "awq", 2: "gptq", 3: "fp8", 4: "mxfp4"}[q.quant_method], group_size=q.group_size, torch_dtype=q.torch_dtype)


def config_from_gguf(path):
    c, g = L.ModelConfig(), L.GgufInfo()
    L.check(L.lib().bz_config_from_gguf(os.fsencode(path), C.byref(c), C.byref(g)))
    return c, dict(architecture=g.architecture.decode(), n_tensors=g.n_tensors, version=g.version, dominant_ggml_type=g.dominant_ggml_type,
                   is_mla=bool(g.is_mla), is_moe=bool(g.is_moe), is_ssm=bool(g.is_ssm), file_size_bytes=g.file_size_bytes)


def safetensors_describe(path):
    import json
    n = C.c_size_t()
    L.check(L.lib().bz_safetensors_describe(os.fsencode(path), None, 0, C.byref(n)))
    buf = C.create_string_buffer(n.value)
    L.check(L.lib().bz_safetensors_describe(os.fsencode(path), buf, n.value, None))
    return json.loads(buf.value.decode())


def load_model(dev, path):
    """loaders.rs load_model: checkpoint directory / .safetensors / .gguf -> finalized LoadedModel"""
    h, c = C.c_void_p(), L.ModelConfig()
    L.check(L.lib().bz_load_model(dev.h, os.fsencode(path), C.byref(h), C.byref(c)))
    m = LoadedModel.__new__(LoadedModel)
    m.dev, m.cfg, m.c, m.h, m.finalized, m._shapes = dev, {}, c, h, True, {}
    m._loras, m._lora_slots = {}, 0
    return m


class LayeredKvCache:
    """boostr::inference::LayeredKvCache::new_positional (executor_generate.rs:350-353)."""

    def __init__(self, dev, layers, batch, n_kv_heads, initial_capacity, max_seq_len, head_dim, dtype):
        h = C.c_void_p()
        L.check(L.lib().bz_kv_create(dev.h, layers, batch, n_kv_heads, initial_capacity, max_seq_len, head_dim, dtype, C.byref(h)))
        self.h, self.dev, self.head_dim = h, dev, head_dim

    new_positional = classmethod(lambda cls, *a: cls(*a))

    def __del__(self):
        try:
            if self.h and L.alive:
                L.lib().bz_kv_free(self.h)
        except Exception:
            pass

    def seq_len(self):
        return L.lib().bz_kv_seq_len(self.h)

    def reset(self):
        L.check(L.lib().bz_kv_reset(self.h))

    def read(self, layer, kv_head, which, length):
        out = np.empty((length, self.head_dim), dtype=np.float32)
        L.check(L.lib().bz_kv_read(self.h, layer, kv_head, which, length, _ptr(out)))
        return out


class LayeredSsmState:
    """boostr::inference::LayeredSsmState::new(layers, batch, mamba_config, dtype, device) (executor_generate.rs:131-133):
    ssm [B, n_heads, head_dim, d_state] + conv [B, conv_dim, k-1] per layer (docs/architecture.md:52-54)."""

    def __init__(self, model, batch=1, dtype=None):
        h = C.c_void_p()
        L.check(L.lib().bz_ssm_state_create(model.h, batch, model.c.act_dtype if dtype is None else dtype, C.byref(h)))
        self.h, self.dev = h, model.dev

    def __del__(self):
        try:
            if self.h and L.alive:
                L.lib().bz_ssm_state_free(self.h)
        except Exception:
            pass

    def reset(self):
        L.check(L.lib().bz_ssm_state_reset(self.h))

    def read(self, layer, which, n):
        """one layer of the state as float32: which 0 = SSM state (n_heads * head_dim * d_state values), 1 = conv window (conv_dim * (k-1))"""
        out = np.empty(n, dtype=np.float32)
        L.check(L.lib().bz_ssm_state_read(self.h, layer, which, _ptr(out), n))
        return out


class LayeredPagedKvCache:
    """boostr::inference::kv_cache::LayeredPagedKvCache::new (executor_generate.rs:208-210) + a private block list
    (CpuBlockAllocator hands out blocks in order)."""

    def __init__(self, dev, layers, num_blocks, block_size, n_kv_heads, head_dim, dtype):
        h = C.c_void_p()
        L.check(L.lib().bz_paged_kv_create(dev.h, layers, num_blocks, block_size, n_kv_heads, head_dim, dtype, C.byref(h)))
        self.h, self.dev = h, dev
        self.block_size, self.num_blocks = block_size, num_blocks
        self.blocks = []

    def __del__(self):
        try:
            if self.h and L.alive:
                L.lib().bz_paged_kv_free(self.h)
        except Exception:
            pass

    def set_blocks(self, blocks):
        self.blocks = list(blocks)

    def seq_len(self):
        return L.lib().bz_paged_kv_seq_len(self.h)

    def set_seq_len(self, n):
        L.check(L.lib().bz_paged_kv_set_seq_len(self.h, n))

    def compute_slot_mapping(self, start, length):
        """slot = block_id * block_size + offset (batch_decode.rs:81-88)."""
        bs = self.block_size
        return [self.blocks[p // bs] * bs + p % bs for p in range(start, start + length)]

    def block_table_device_format(self):
        return list(self.blocks)

    def copy_slots(self, src, dst, n_slots):
        """The first n_slots slots of block src -> block dst over every layer, K and V, every KV head (the prefix cache's copy-on-write kernel)."""
        L.check(L.lib().bz_paged_kv_copy_slots(self.h, int(src), int(dst), int(n_slots)))

    def read_block(self, layer, block, which, n_kv_heads, head_dim, dtype):
        """One block of one layer as stored: [kv_head][block_size][head_dim], f32 for an f32 pool, the raw 16-bit patterns (uint16) otherwise."""
        out = np.empty((n_kv_heads, self.block_size, head_dim), dtype=np.float32 if dtype == L.F32 else np.uint16)
        L.check(L.lib().bz_paged_kv_read_block(self.h, int(layer), int(block), int(which), _ptr(out), out.nbytes))
        return out

    def write_block(self, layer, block, which, data):
        """The mirror of read_block: `data` [kv_head][block_size][head_dim] as stored (float32 for an f32 pool, raw 16-bit patterns as uint16 otherwise)."""
        a = np.ascontiguousarray(data)
        L.check(L.lib().bz_paged_kv_write_block(self.h, int(layer), int(block), int(which), _ptr(a), a.nbytes))


def rows_attn_slice_len(n):
    """bz_rows_attn_slice_len: positions per split-KV slice for a decode-batch row of n keys (host only; the rule the device applies)"""
    return int(L.lib().bz_rows_attn_slice_len(int(n)))


def rows_attn_plan(n_heads, n_kv_heads, head_dim, kv_dtype, window, n, capacity):
    """bz_rows_attn_plan (host only): what a decode batch of n rows launches per layer at a decision length of `capacity` positions.  Returns a dict with
    kernel (0 scalar, 1 split pair, -1 refused), scalar_limit, grid_slices, rows_per_pass, ws_bytes and, for a refused plan, the library's message."""
    p = L.RowsAttnPlan()
    rc = L.lib().bz_rows_attn_plan(int(n_heads), int(n_kv_heads), int(head_dim), int(kv_dtype), int(window), int(n), int(capacity), C.byref(p))
    d = dict(kernel=p.kernel, scalar_limit=p.scalar_limit, grid_slices=p.grid_slices, rows_per_pass=p.rows_per_pass, ws_bytes=int(p.ws_bytes), code=rc, error=None)
    if rc == L.E_UNSUPPORTED and p.kernel == -1:
        d["error"] = L.lib().bz_last_error().decode()
        return d
    L.check(rc)
    return d


def prompt_traits(model):
    """bz_model_prompt_traits: what the route decision reads of a loaded model (a LoadedModel or a raw handle), as an L.PromptTraits"""
    t = L.PromptTraits()
    L.check(L.lib().bz_model_prompt_traits(getattr(model, "h", model), C.byref(t)))
    return t


def prompt_plan(traits, kind, rows, total_len, kv_dtype=L.F16, switches=None):
    """bz_prompt_plan (host only): the path `rows` rows ending at a context of `total_len` positions take.  switches: an L.PromptSwitches, or None for this
    process's environment.  Returns a dict of route, exact, attn, head, chunk (L.ROUTE_*, L.PF_ATTN_*, L.HEAD_*)."""
    p = L.PromptPlan()
    L.check(L.lib().bz_prompt_plan(C.byref(traits), C.byref(switches) if switches is not None else None, int(kind), int(rows), int(total_len), int(kv_dtype), C.byref(p)))
    return dict(route=p.route, exact=p.exact, attn=p.attn, head=p.head, chunk=p.chunk)


def packed_plan(traits, seq_lens, kv_dtype=L.F16, switches=None):
    """bz_packed_plan (host only): what a packed prompt batch of these input lengths does -> dict(packed, rows, n_seq, max_len, plan = the prompt_plan dict)"""
    sl = np.ascontiguousarray(seq_lens, dtype=np.int32).reshape(-1)
    p = L.PackedPlan()
    L.check(L.lib().bz_packed_plan(C.byref(traits), C.byref(switches) if switches is not None else None, _ptr(sl) if len(sl) else None, len(sl), int(kv_dtype), C.byref(p)))
    q = p.plan
    return dict(packed=p.packed, rows=p.rows, n_seq=p.n_seq, max_len=p.max_len, plan=dict(route=q.route, exact=q.exact, attn=q.attn, head=q.head, chunk=q.chunk))


def packed_targets_spec(tokens, seq_lens):
    """bz_packed_targets_spec (host only): the default targets of score_batch for packed `tokens` -> int64 [T]"""
    tk, sl = np.ascontiguousarray(tokens, dtype=np.int64).reshape(-1), np.ascontiguousarray(seq_lens, dtype=np.int32).reshape(-1)
    if int(sl.sum()) != len(tk):
        raise ValueError("packed_targets_spec: %d tokens for lengths summing to %d" % (len(tk), int(sl.sum())))
    out = np.zeros(len(tk), dtype=np.int64)
    L.check(L.lib().bz_packed_targets_spec(_ptr(tk), _ptr(sl), len(sl), _ptr(out)))
    return out


def packed_totals_spec(rows, seq_lens):
    """bz_packed_totals_spec (host only): SCORE_ROW records [T] of a packed batch -> list of (sum_logprob, n_scored) per input, as score_batch adds them"""
    r, sl = np.ascontiguousarray(rows, dtype=SCORE_ROW), np.ascontiguousarray(seq_lens, dtype=np.int32).reshape(-1)
    if int(sl.sum()) != len(r):
        raise ValueError("packed_totals_spec: %d rows for lengths summing to %d" % (len(r), int(sl.sum())))
    tots = (L.ScoreTotal * len(sl))()
    L.check(L.lib().bz_packed_totals_spec(_ptr(r), _ptr(sl), len(sl), tots))
    return [(float(t.sum_logprob), int(t.n_scored)) for t in tots]


def attn_packed(dev, qkv, seq_lens, nq, nkv, hd, dt=L.F16, form=None, window=0):
    """bz_attn_packed (op level): rotated q / k / v rows F32 [T, (nq + 2 nkv) hd] of a packed batch -> its attention output, f32 array [T, nq hd].  K / V are rounded
    to `dt`; form: L.PF_ATTN_MFMA (default) / _SCALAR / _SCALAR_EXACT."""
    x = qkv if isinstance(qkv, Tensor) else dev.tensor(np.ascontiguousarray(qkv, dtype=np.float32))
    sl = np.ascontiguousarray(seq_lens, dtype=np.int32).reshape(-1)
    T = int(sl.sum()) if len(sl) else 0
    out = dev.zeros((max(T, 1), nq * hd), L.F32)
    L.check(L.lib().bz_attn_packed(dev.h, x.h, _ptr(sl) if len(sl) else None, len(sl), int(nq), int(nkv), int(hd), int(dt), int(L.PF_ATTN_MFMA if form is None else form),
                                   int(window), out.h))
    return out.to_numpy().reshape(out.shape)


def _plan_dict(p):
    return {n: (list(getattr(p, n)) if n in ("qkv", "o", "gateup", "down") else getattr(p, n)) for n, _ in L.LayerPlan._fields_}


def layer_plan(traits, kv_dtype=L.F16, switches=None):
    """bz_layer_plan (host only): the kernels one layer of a decode step launches over a cache of kv_dtype.  switches: an L.StepSwitches, or None for this
    process's environment.  Returns a dict of the L.LayerPlan fields (L.GEMV_*, L.ATTN_*, L.ATTN_K_*, L.MLP_*; per-part forms as lists of three)."""
    p = L.LayerPlan()
    L.check(L.lib().bz_layer_plan(C.byref(traits), C.byref(switches) if switches is not None else None, int(kv_dtype), C.byref(p)))
    return _plan_dict(p)


def penalty_window(recent_tokens, repeat_last_n):
    """sampling.rs:169-191: unique ids + counts over the last `repeat_last_n` tokens."""
    w = recent_tokens[-repeat_last_n:] if 0 < repeat_last_n < len(recent_tokens) else recent_tokens
    ids, cnts = [], []
    for t in w:
        if t in ids:
            cnts[ids.index(t)] += 1
        else:
            ids.append(int(t))
            cnts.append(1)
    return np.asarray(ids, dtype=np.int64), np.asarray(cnts, dtype=np.int32)


def logits_to_token(dev, logits, ids, cnts, repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0, temperature=0.0,
                    top_k=0, top_p=1.0, min_p=0.0, seed=0):
    """SamplingOps::logits_to_token (sampling.rs:445-460) -> I64[1] device tensor."""
    rows, vocab = logits.shape
    n = len(ids)
    tid = dev.tensor(np.asarray(ids, dtype=np.int64)) if n else None
    tcn = dev.tensor(np.asarray(cnts, dtype=np.int32)) if n else None
    out = dev.zeros((1,), L.I64)
    L.check(L.lib().bz_logits_to_token(dev.h, logits.h, rows, vocab, tid.h if n else None, tcn.h if n else None, n, repeat_penalty,
                                       frequency_penalty, presence_penalty, temperature, top_k, top_p, min_p, seed, out.h))
    return out


# bz_score_row as a numpy record (same layout: 192 bytes)
SCORE_ROW = np.dtype([("target", np.int64), ("logit", np.float32), ("logprob", np.float32), ("lse", np.float32), ("rank", np.int32), ("n_top", np.int32),
                      ("top_ids", np.uint32, (L.TOP_LOGPROBS_MAX,)), ("top_logprobs", np.float32, (L.TOP_LOGPROBS_MAX,))], align=True)


def score_result(rows, total=None):
    """ctypes ScoreRow array (+ ScoreTotal) -> dict(rows, sum_logprob, n_scored, perplexity); without a total it is added here as the library adds it"""
    r = np.frombuffer(bytes(rows), dtype=SCORE_ROW).copy()
    if total is None:
        lp = r["logprob"][(r["n_top"] >= 0) & np.isfinite(r["logprob"])]
        ssum, n = float(np.cumsum(lp.astype(np.float64))[-1]) if len(lp) else 0.0, len(lp)
    else:
        ssum, n = float(total.sum_logprob), int(total.n_scored)
    return dict(rows=r, sum_logprob=ssum, n_scored=n, perplexity=float(np.exp(-ssum / n)) if n else float("nan"))


def score_rows(dev, logits, targets, top_logprobs=0):
    """bz_score_rows (op level): logits F32 [R, V] (device tensor or array), targets [R] (-1: not scored) -> as LoadedModel.score"""
    lg = logits if isinstance(logits, Tensor) else dev.tensor(np.ascontiguousarray(logits, dtype=np.float32))
    R, V = lg.shape
    tg = dev.tensor(np.ascontiguousarray(targets, dtype=np.int64).reshape(-1))
    if tg.shape[0] != R:
        raise ValueError("score_rows: %d targets for %d rows" % (tg.shape[0], R))
    cfg, rows = L.ScoreConfig(top_n=int(top_logprobs)), (L.ScoreRow * R)()
    L.check(L.lib().bz_score_rows(dev.h, lg.h, R, V, tg.h, C.byref(cfg), rows))
    return score_result(rows)


def score_row_spec(x, target, top_logprobs=0):
    """bz_score_row_spec: the definition of one row's record, evaluated on the host -> one SCORE_ROW record"""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    row = (L.ScoreRow * 1)()
    L.check(L.lib().bz_score_row_spec(_ptr(x), len(x), int(target), int(top_logprobs), row))
    return np.frombuffer(bytes(row), dtype=SCORE_ROW).copy()[0]


def _embed_cfg(pooling, normalize):
    if pooling not in L.POOLINGS:
        raise ValueError("pooling %r (one of %s)" % (pooling, ", ".join(sorted(L.POOLINGS))))
    return L.EmbedConfig(pooling=L.POOLINGS[pooling], normalize=int(bool(normalize)))


def pool_rows(dev, hidden, pooling="mean", normalize=False):
    """bz_pool_rows (op level): hidden F32 [S, H] (device tensor or array) -> f32 array [H] ([S, H] for "none")"""
    hd = hidden if isinstance(hidden, Tensor) else dev.tensor(np.ascontiguousarray(hidden, dtype=np.float32))
    S, H = hd.shape
    cfg = _embed_cfg(pooling, normalize)
    out = dev.zeros((S, H) if pooling == "none" else (H,), L.F32)
    L.check(L.lib().bz_pool_rows(dev.h, hd.h, S, H, C.byref(cfg), out.h))
    return out.to_numpy().reshape(out.shape)


def pool_spec(hidden, pooling="mean", normalize=False):
    """bz_pool_spec: the definition of pooling, evaluated on the host"""
    hd = np.ascontiguousarray(hidden, dtype=np.float32)
    S, H = hd.shape
    cfg = _embed_cfg(pooling, normalize)
    out = np.zeros((S, H) if pooling == "none" else (H,), dtype=np.float32)
    L.check(L.lib().bz_pool_spec(_ptr(hd), S, H, C.byref(cfg), _ptr(out)))
    return out


def cosine_similarity(a, b):
    """rerank.rs:206-224: f32 running sums in element order, dot / (sqrt(|a|^2) * sqrt(|b|^2)) if that exceeds 1e-12, else 0.0 (also for unequal or zero lengths)"""
    a, b = np.asarray(a, dtype=np.float32).reshape(-1), np.asarray(b, dtype=np.float32).reshape(-1)
    if len(a) != len(b) or len(a) == 0:
        return 0.0
    dot, na, nb = np.float32(0), np.float32(0), np.float32(0)
    for x, y in zip(a, b):
        dot = np.float32(dot + np.float32(x * y)); na = np.float32(na + np.float32(x * x)); nb = np.float32(nb + np.float32(y * y))
    denom = np.float32(np.sqrt(na) * np.sqrt(nb))
    return float(np.float32(dot / denom)) if denom > 1e-12 else 0.0


def rerank(model, cache, query, docs, top_n=None, batched=False):
    """/rerank (rerank.rs:206): mean-pooled embeddings of the query and of every document (each from position 0 of `cache`, which is reset between them), cosine
    similarity, highest first, ties in document order -> list of dict(index, relevance_score), at most top_n.  batched: the query and all documents in ONE
    embed_batch pass (`cache` must hold all their tokens); the default stays the loop of single calls."""
    def emb(tokens):
        cache.reset()
        return model.embed(tokens, cache, 0, pooling="mean")
    if batched:
        e = model.embed_batch([query] + list(docs), cache, pooling="mean")
        q, embs = e[0], e[1:]
    else:
        q = emb(query)
        embs = (emb(d) for d in docs)
    scored = [dict(index=i, relevance_score=cosine_similarity(q, v)) for i, v in enumerate(embs)]
    scored.sort(key=lambda e: -e["relevance_score"])              # stable
    return scored[:top_n] if top_n is not None else scored


def spec_accept(dev, logits, draft):
    """bz_spec_accept: logits F32 [R, V] (device tensor or array), draft I64 [R-1] -> the record as an int64 array [R+1] = {n_accept, tokens[0 .. n_accept], -1 ...}."""
    lg = logits if isinstance(logits, Tensor) else dev.tensor(np.ascontiguousarray(logits, dtype=np.float32))
    R, V = lg.shape
    d = np.ascontiguousarray(draft, dtype=np.int64).reshape(-1)
    if len(d) != R - 1:
        raise ValueError("spec_accept: %d draft tokens for %d rows" % (len(d), R))
    td = dev.tensor(d) if R > 1 else None
    rec = dev.zeros((R + 1,), L.I64)
    L.check(L.lib().bz_spec_accept(dev.h, lg.h, R, V, td.h if td is not None else None, rec.h))
    return rec.to_numpy().reshape(-1)


def pack_vocab(vocab_bytes):
    """A vocabulary as the C ABI takes it: list of bytes objects (or an already packed (flat u8, offsets i64) pair) -> (flat u8, offsets i64[V+1])."""
    if isinstance(vocab_bytes, tuple):
        flat, off = vocab_bytes
        return np.ascontiguousarray(flat, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.int64)
    off = np.zeros(len(vocab_bytes) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in vocab_bytes], out=off[1:])
    flat = np.frombuffer(b"".join(vocab_bytes), dtype=np.uint8)
    return np.ascontiguousarray(flat), off


class GrammarDfa:
    """engine::grammar::GrammarDfa (grammar.rs:21-64): compile_grammar_to_dfa(gbnf) (regular=False: the reference's semantics; regular=True: the regular
    subset of GBNF compiled properly), or a caller-compiled table.  Host only: no device is needed."""

    def __init__(self, gbnf=None, regular=False, table=None, accepting=None):
        h = C.c_void_p()
        if table is not None:
            t = np.ascontiguousarray(table, dtype=np.int32).reshape(-1, 256)
            a = np.ascontiguousarray(accepting, dtype=np.uint8)
            if len(a) != len(t):
                raise ValueError("accepting must have one entry per state")
            L.check(L.lib().bz_grammar_from_table(len(t), _ptr(t), _ptr(a), C.byref(h)))
        else:
            text = gbnf.encode("utf-8") if isinstance(gbnf, str) else bytes(gbnf)
            L.check(L.lib().bz_grammar_compile(text, L.GRAMMAR_REGULAR if regular else 0, C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if self.h and L.alive:
                L.lib().bz_grammar_free(self.h)
        except Exception:
            pass

    def num_states(self):
        return L.lib().bz_grammar_num_states(self.h)

    def current_state(self):
        return L.lib().bz_grammar_current_state(self.h)

    def is_accepting(self):
        return bool(L.lib().bz_grammar_is_accepting(self.h))

    def reset(self):
        L.check(L.lib().bz_grammar_reset(self.h))

    def advance(self, data):
        """advance() per byte as the generate loop calls it; returns the number of bytes that had no transition (the state stays put on those)."""
        b = np.frombuffer(bytes(data), dtype=np.uint8)
        rej = C.c_int()
        L.check(L.lib().bz_grammar_advance(self.h, _ptr(b) if len(b) else None, len(b), C.byref(rej)))
        return rej.value

    def table(self):
        """(int32 [num_states, 256] with -1 = no transition, uint8 [num_states] accepting)"""
        n = self.num_states()
        t = np.empty((n, 256), dtype=np.int32)
        a = np.empty(n, dtype=np.uint8)
        L.check(L.lib().bz_grammar_table(self.h, _ptr(t), _ptr(a)))
        return t, a

    def compute_token_mask(self, vocab_bytes):
        flat, off = pack_vocab(vocab_bytes)
        out = np.empty(len(off) - 1, dtype=np.uint8)
        L.check(L.lib().bz_grammar_token_mask(self.h, _ptr(flat), _ptr(off), len(off) - 1, _ptr(out)))
        return out.astype(bool)

    def to_device(self, dev, vocab_bytes):
        return DeviceGrammarDfa(dev, self, vocab_bytes)

    @classmethod
    def concat(cls, dfas):
        """n DFAs as one table -> (dfa, starts): starts[i] is the state that is dfas[i]'s state 0, so one uploaded table serves rows with different grammars."""
        dfas = list(dfas)
        hs = (C.c_void_p * max(len(dfas), 1))(*[d.h if d is not None else None for d in dfas])
        starts = np.zeros(max(len(dfas), 1), dtype=np.int32)
        h = C.c_void_p()
        L.check(L.lib().bz_grammar_concat(hs, len(dfas), C.byref(h), starts.ctypes.data_as(C.POINTER(C.c_int32))))
        out = cls.__new__(cls)
        out.h = h
        return out, [int(x) for x in starts[:len(dfas)]]

    def advance_tokens(self, vocab_bytes, tokens):
        """advance() over the bytes of each token in turn; returns the number of bytes that had no transition."""
        flat, off = pack_vocab(vocab_bytes)
        t = np.ascontiguousarray(tokens, dtype=np.int64).reshape(-1)
        rej = C.c_int()
        L.check(L.lib().bz_grammar_advance_tokens(self.h, _ptr(flat) if len(flat) else None, _ptr(off), len(off) - 1, _ptr(t) if len(t) else None, len(t), C.byref(rej)))
        return rej.value


class DeviceGrammarDfa:
    """boostr::DeviceGrammarDfa as GrammarDfa::to_device builds it (grammar.rs:90-139) + GrammarDfaOps::grammar_dfa_mask_logits (sampling.rs:415-419)."""

    def __init__(self, dev, dfa, vocab_bytes):
        flat, off = pack_vocab(vocab_bytes)
        h = C.c_void_p()
        L.check(L.lib().bz_grammar_to_device(dev.h, dfa.h, _ptr(flat), _ptr(off), len(off) - 1, C.byref(h)))
        self.h, self.dev = h, dev

    def __del__(self):
        try:
            if self.h and L.alive:
                L.lib().bz_device_grammar_free(self.h)
        except Exception:
            pass

    def set_state(self, state):
        L.check(L.lib().bz_device_grammar_set_state(self.h, int(state)))

    def info(self):
        n, v, s, lds = C.c_int32(), C.c_int64(), C.c_uint32(), C.c_int32()
        L.check(L.lib().bz_device_grammar_info(self.h, C.byref(n), C.byref(v), C.byref(s), C.byref(lds)))
        return dict(num_states=n.value, vocab=v.value, state=s.value, lds_table=bool(lds.value))

    def mask_logits(self, logits, out=None):
        """logits: F32 [rows, vocab] device tensor; the last row is masked.  out=None masks in place."""
        rows, vocab = logits.shape
        out = logits if out is None else out
        L.check(L.lib().bz_grammar_dfa_mask_logits(self.dev.h, logits.h, rows, vocab, self.h, out.h))
        return out


class GrammarCursor:
    """One device-resident DFA state per row of a decode batch over a DeviceGrammarDfa (every row starts at its current state): mask() and advance() run on
    the device stream without a host step, so they sit inside DecodeGraph / BatchDecodeGraph.  FREE marks an unconstrained row."""

    FREE = L.GRAMMAR_ROW_FREE

    def __init__(self, device_grammar, n):
        h = C.c_void_p()
        L.check(L.lib().bz_grammar_cursor_create(device_grammar.h, int(n), C.byref(h)))
        self.grammar = device_grammar            # the cursor borrows it: keep it alive as long as the cursor
        self.h, self.dev, self.n = h, device_grammar.dev, int(n)

    def __del__(self):
        try:
            if self.h and L.alive:
                L.lib().bz_grammar_cursor_free(self.h)
        except Exception:
            pass

    def set_row(self, row, state):
        """Row `row` continues from `state` (or FREE) at the next launch / replay; its rejected count restarts at 0."""
        L.check(L.lib().bz_grammar_cursor_set_row(self.h, int(row), int(state)))

    def read(self):
        """(states uint32 [n], rejected uint32 [n]); waits for the device."""
        st = np.empty(self.n, dtype=np.uint32)
        rej = np.empty(self.n, dtype=np.uint32)
        L.check(L.lib().bz_grammar_cursor_read(self.h, _ptr(st), _ptr(rej)))
        return st, rej

    def mask(self, logits):
        """logits F32 [n, vocab] device tensor, masked in place row by row."""
        L.check(L.lib().bz_grammar_cursor_mask(self.h, logits.h))
        return logits

    def advance(self, tokens):
        """tokens I64 [n] device tensor: every row walks its token's bytes."""
        L.check(L.lib().bz_grammar_cursor_advance(self.h, tokens.h))


def _bias_arrays(logit_bias):
    items = list(logit_bias.items()) if isinstance(logit_bias, dict) else list(logit_bias or ())
    return (np.ascontiguousarray([int(i) for i, _ in items], dtype=np.uint32), np.ascontiguousarray([float(v) for _, v in items], dtype=np.float32))


def _logprobs_record(r):
    if r.n_top < 0:
        return None
    d = dict(token=int(r.token), logprob=float(np.float32(r.logprob)), top_ids=[int(t) for t in r.top_ids[:r.n_top]],
             top_logprobs=[float(np.float32(v)) for v in r.top_logprobs[:r.n_top]])
    if hasattr(r, "lse"):
        d["lse"] = float(np.float32(r.lse))
    return d


class BatchSampler:
    """Per-sequence sampling for a decode batch (batch_decode.rs:149-168: logits_to_token_on_device once per sequence with its own gen_config) as one
    device-side call: every row keeps its parameters, the ring of its last tokens (the penalty window of sampling.rs:169-191) and its draw index on the device."""

    def __init__(self, dev, n, vocab):
        h = C.c_void_p()
        L.check(L.lib().bz_batch_sampler_create(dev.h, int(n), int(vocab), C.byref(h)))
        self.h, self.dev, self.n, self.vocab = h, dev, int(n), int(vocab)

    def __del__(self):
        try:
            if self.h and L.alive:
                L.lib().bz_batch_sampler_free(self.h)
        except Exception:
            pass

    def set_row(self, row, history=(), draw_index=0, temperature=0.0, top_k=0, top_p=1.0, min_p=0.0, repeat_penalty=1.0, frequency_penalty=0.0,
                presence_penalty=0.0, repeat_last_n=64, seed=0):
        """Row `row` samples with these parameters from now on, starting from `history` (the sequence so far, prompt included); its next draw uses seed + draw_index."""
        p = L.RowSampling(temperature=temperature, top_k=int(top_k), top_p=top_p, min_p=min_p, repeat_penalty=repeat_penalty, frequency_penalty=frequency_penalty,
                          presence_penalty=presence_penalty, repeat_last_n=int(repeat_last_n), seed=int(seed))
        hist = np.ascontiguousarray(history, dtype=np.int64).reshape(-1)
        L.check(L.lib().bz_batch_sampler_set_row(self.h, int(row), C.byref(p), _ptr(hist) if len(hist) else None, len(hist), int(draw_index)))

    def sample(self, logits, out=None):
        """logits F32 [n, vocab] (device tensor) -> I64 [n] device tensor; enqueued on the device stream.  With enable(bias=True) the rows' biases are added
        to `logits` in place."""
        out = self.dev.zeros((self.n,), L.I64) if out is None else out
        L.check(L.lib().bz_batch_sampler_sample(self.h, logits.h, out.h))
        return out

    def enable(self, bias=False, logprobs=False):
        """Per-row logit bias and / or logprobs (GenerationConfig.logit_bias, logprobs, top_logprobs per sequence), once, before the first sample or capture."""
        L.check(L.lib().bz_batch_sampler_enable(self.h, (L.BS_BIAS if bias else 0) | (L.BS_LOGPROBS if logprobs else 0)))

    def set_row_bias(self, row, logit_bias=None):
        """logit_bias: {id: bias} or a sequence of (id, bias) pairs (the last entry of an id wins, ids beyond the vocabulary are dropped); None / empty clears the row."""
        ids, vals = _bias_arrays(logit_bias)
        L.check(L.lib().bz_batch_sampler_set_row_bias(self.h, int(row), _ptr(ids) if len(ids) else None, _ptr(vals) if len(vals) else None, len(ids)))

    def set_row_logprobs(self, row, top_n):
        """top_n: -1 (or None) = off, 0..20 = the picked token's logprob plus that many alternatives."""
        L.check(L.lib().bz_batch_sampler_set_row_logprobs(self.h, int(row), -1 if top_n is None else int(top_n)))

    def read_logprobs(self):
        """The records of the last sample() call, one dict per row (None for a row with logprobs off); waits for the stream."""
        recs = (L.LogprobsRecord * self.n)()
        L.check(L.lib().bz_batch_sampler_read_logprobs(self.h, recs))
        return [_logprobs_record(r) for r in recs]


class BatchDecodeGraph:
    """Executor::capture_batched_graph / replay_batched_graph + BatchedGraphState (cuda_graphs_batched.rs:43-257): one hipGraph per decode step of N
    sequences over a shared paged cache; tokens, positions and slots live on the device between replays.  With `sampler` (a BatchSampler of the same n and
    vocabulary) every sequence samples with its own parameters inside the graph; without, the step ends in the greedy argmax.  With `grammar` (a GrammarCursor
    of the same n and vocabulary) every row's logits are masked from its own DFA state before the pick and the state moves on with the picked token."""

    def __init__(self, model, cache, n, max_blocks, sampler=None, grammar=None):
        h = C.c_void_p()
        if grammar is not None:
            L.check(L.lib().bz_decode_batch_graph_capture_grammar(model.h, cache.h, int(n), int(max_blocks), sampler.h if sampler is not None else None, grammar.h,
                                                                  C.byref(h)))
        elif sampler is None:
            L.check(L.lib().bz_decode_batch_graph_capture(model.h, cache.h, int(n), int(max_blocks), C.byref(h)))
        else:
            L.check(L.lib().bz_decode_batch_graph_capture_sampled(model.h, cache.h, int(n), int(max_blocks), sampler.h, C.byref(h)))
        self.sampler, self.grammar = sampler, grammar   # the graph borrows them: keep them alive as long as the graph
        self.h, self.model, self.cache, self.n, self.max_blocks = h, model, cache, int(n), int(max_blocks)

    def __del__(self):
        try:
            if self.h and L.alive:
                L.lib().bz_decode_batch_graph_free(self.h)
        except Exception:
            pass

    def _table(self, block_tables):
        bt = np.zeros((self.n, self.max_blocks), dtype=np.int32)
        for i, row in enumerate(block_tables):
            bt[i, :len(row)] = row
        return bt

    def seed(self, tokens, seq_lens, block_tables):
        t = np.ascontiguousarray(tokens, dtype=np.int64)
        sl = np.ascontiguousarray(seq_lens, dtype=np.int32)
        bt = self._table(block_tables)
        L.check(L.lib().bz_decode_batch_graph_seed(self.h, _ptr(t), _ptr(sl), _ptr(bt)))

    def set_block_table(self, block_tables):
        bt = self._table(block_tables)
        L.check(L.lib().bz_decode_batch_graph_set_block_table(self.h, _ptr(bt)))

    def set_adapters(self, names):
        """one registered adapter name (or None) per row; the next replay reads them"""
        sl = np.ascontiguousarray([self.model.lora_slot(nm) for nm in names], dtype=np.int32)
        if len(sl) != self.n:
            raise ValueError("set_adapters: %d names for %d rows" % (len(sl), self.n))
        L.check(L.lib().bz_decode_batch_graph_set_adapters(self.h, _ptr(sl)))

    def replay(self):
        L.check(L.lib().bz_decode_batch_graph_replay(self.h))

    def read_tokens(self, step):
        out = np.empty(self.n, dtype=np.int64)
        L.check(L.lib().bz_decode_batch_graph_read_tokens(self.h, int(step), _ptr(out)))
        return out

    def read_logprobs(self, step):
        """The records of replay `step` (sampler.enable(logprobs=True) before the capture), one dict per row, None for a row with logprobs off."""
        recs = (L.LogprobsRecord * self.n)()
        L.check(L.lib().bz_decode_batch_graph_read_logprobs(self.h, int(step), recs))
        return [_logprobs_record(r) for r in recs]

    def read_logits(self):
        t = C.c_void_p()
        L.check(L.lib().bz_decode_batch_graph_logits(self.h, C.byref(t)))
        out = np.empty((self.n, self.model.c.vocab), dtype=np.float32)
        L.check(L.lib().bz_tensor_to_host(t, _ptr(out), out.nbytes))
        return out


class Scheduler:
    """The engine's host scheduler on its own (bz_sched_*; engine/request_scheduler.rs:105-205): no device is needed."""

    def __init__(self, n_rows, num_blocks, block_size, max_seq_len, prefill_chunk=0):
        h = C.c_void_p()
        L.check(L.lib().bz_sched_create(int(n_rows), int(num_blocks), int(block_size), int(max_seq_len), int(prefill_chunk), C.byref(h)))
        self.h, self.n_rows, self.max_blocks = h, int(n_rows), (int(max_seq_len) + int(block_size) - 1) // int(block_size)
        self._acts = (L.SchedAction * (4 * self.n_rows))()

    def __del__(self):
        try:
            if self.h and L.alive:
                L.lib().bz_sched_free(self.h)
        except Exception:
            pass

    def submit(self, n_prompt, max_tokens):
        rid = C.c_int64()
        L.check(L.lib().bz_sched_submit(self.h, int(n_prompt), int(max_tokens), C.byref(rid)))
        return rid.value

    def enable_prefix(self):
        """The prefix cache's switch; before the first submit."""
        L.check(L.lib().bz_sched_enable_prefix(self.h))

    def submit_tokens(self, prompt, max_tokens):
        p = np.ascontiguousarray(prompt, dtype=np.int64).reshape(-1)
        rid = C.c_int64()
        L.check(L.lib().bz_sched_submit_tokens(self.h, _ptr(p), len(p), int(max_tokens), C.byref(rid)))
        return rid.value

    def prefix_info(self):
        i = L.SchedPrefixInfo()
        L.check(L.lib().bz_sched_prefix_info(self.h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in L.SchedPrefixInfo._fields_}

    def prefix_flush(self):
        """Drops every unreferenced cached block; how many."""
        n = C.c_int()
        L.check(L.lib().bz_sched_prefix_flush(self.h, C.byref(n)))
        return n.value

    def step(self):
        """[(kind, row, id, a, b)]: this step's admissions, copies, prompt chunks and rows going live, in order."""
        n = C.c_int()
        L.check(L.lib().bz_sched_step(self.h, self._acts, len(self._acts), C.byref(n)))
        return [(a.kind, a.row, a.id, a.a, a.b) for a in self._acts[:n.value]]

    def finish(self, rid):
        L.check(L.lib().bz_sched_finish(self.h, int(rid)))

    def info(self):
        i = L.SchedInfo()
        L.check(L.lib().bz_sched_info(self.h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in L.SchedInfo._fields_}

    def row(self, row):
        """(request id or -1, its blocks)"""
        rid, n = C.c_int64(), C.c_int()
        blocks = np.zeros(self.max_blocks, dtype=np.int32)
        L.check(L.lib().bz_sched_row(self.h, int(row), C.byref(rid), _ptr(blocks), len(blocks), C.byref(n)))
        return rid.value, blocks[:n.value].tolist()


class BatchEngine:
    """BatchEngine::run / RequestScheduler::submit (engine/batch_engine.rs:91-169, engine/request_scheduler.rs:105-205) over the batched decode graph: requests
    come and go while the captured step keeps running; the caller drives with step().  sampler=True: every request samples with its own parameters
    (the keyword arguments of BatchSampler.set_row); grammar: a GrammarCursor of n_rows rows, borrowed (its rows are handed out by the engine)."""

    def __init__(self, model, n_rows, num_blocks, block_size=16, max_seq_len=None, prefill_chunk=0, depth=2, sampler=True, grammar=None, prefix_cache=False,
                 logprobs=False):
        """logprobs=True (needs sampler=True): requests may ask for logprobs / top_logprobs and carry a logit_bias; the records arrive in `logprobs`."""
        cfg = L.EngineConfig(n_rows=int(n_rows), num_blocks=int(num_blocks), block_size=int(block_size),
                             max_seq_len=int(max_seq_len if max_seq_len is not None else model.c.max_seq_len), prefill_chunk=int(prefill_chunk), depth=int(depth),
                             use_sampler=1 if sampler else 0, prefix_cache=int(prefix_cache), logprobs=int(bool(logprobs)))
        h = C.c_void_p()
        L.check(L.lib().bz_engine_create(model.h, C.byref(cfg), grammar.h if grammar is not None else None, C.byref(h)))
        self.h, self.model, self.grammar, self.n_rows = h, model, grammar, int(n_rows)
        self._events = (L.EngineEvent * 256)()
        self._lp = (L.EngineLogprobs * 256)()
        self.results = {}
        self.logprobs = {}    # id -> the per-token records of a request that asked for logprobs (filled by run_until_idle / collect_logprobs)

    def __del__(self):
        try:
            if self.h and L.alive:
                L.lib().bz_engine_free(self.h)
        except Exception:
            pass

    def submit(self, prompt, max_tokens, stop=(), grammar_state=None, lora=None, logprobs=False, top_logprobs=0, logit_bias=None, **sampling):
        """lora: a name registered with model.load_lora (GenerationConfig.lora_adapter per request); None: the base model.
        logprobs / top_logprobs / logit_bias (GenerationConfig.logprobs, top_logprobs 0..20, logit_bias {id: bias}): on an engine with logprobs=True."""
        p = np.ascontiguousarray(prompt, dtype=np.int64).reshape(-1)
        stop = [int(t) for t in stop]
        rq = L.Request(max_tokens=int(max_tokens), n_stop=len(stop), grammar_state=L.GRAMMAR_ROW_FREE if grammar_state is None else int(grammar_state),
                       lora_slot=self.model.lora_slot(lora) + 1)
        for i, t in enumerate(stop[:L.ENGINE_MAX_STOP]):
            rq.stop_ids[i] = t
        kw = dict(temperature=0.0, top_k=0, top_p=1.0, min_p=0.0, repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0, repeat_last_n=64, seed=0)
        kw.update(sampling)
        rq.sampling = L.RowSampling(**kw)
        rid = C.c_int64()
        if logprobs or top_logprobs or logit_bias is not None:
            ids, vals = _bias_arrays(logit_bias)
            ex = L.RequestExtras(logprobs=int(bool(logprobs)), top_logprobs=int(top_logprobs), n_logit_bias=len(ids),
                                 logit_bias_ids=ids.ctypes.data if len(ids) else None, logit_bias_vals=vals.ctypes.data if len(vals) else None)
            L.check(L.lib().bz_engine_submit_ex(self.h, _ptr(p), len(p), C.byref(rq), C.byref(ex), C.byref(rid)))
        else:
            L.check(L.lib().bz_engine_submit(self.h, _ptr(p), len(p), C.byref(rq), C.byref(rid)))
        return rid.value

    def cancel(self, rid):
        L.check(L.lib().bz_engine_cancel(self.h, int(rid)))

    def step(self):
        """One scheduling iteration; False once nothing is waiting, running or unread."""
        busy = C.c_int()
        L.check(L.lib().bz_engine_step(self.h, C.byref(busy)))
        return bool(busy.value)

    def poll(self):
        """[(id, token, index, finish_reason, replay)] since the last poll; finish_reason -1 running, 0 length, 1 stop, 2 cancelled (token -1)."""
        out = []
        while True:
            n = C.c_int()
            L.check(L.lib().bz_engine_poll(self.h, self._events, len(self._events), C.byref(n)))
            out += [(e.id, e.token, e.index, e.finish_reason, e.replay) for e in self._events[:n.value]]
            if n.value < len(self._events):
                return out

    def poll_logprobs(self):
        """[{id, index, token, logprob, top_ids, top_logprobs}] since the last call: one per token event of a request that asked for logprobs, in event order."""
        out = []
        while True:
            n = C.c_int()
            L.check(L.lib().bz_engine_poll_logprobs(self.h, self._lp, len(self._lp), C.byref(n)))
            for r in self._lp[:n.value]:
                d = _logprobs_record(r) or dict(token=int(r.token), logprob=float("nan"), top_ids=[], top_logprobs=[])
                d.update(id=int(r.id), index=int(r.index))
                out.append(d)
            if n.value < len(self._lp):
                return out

    def collect_logprobs(self):
        """Fold poll_logprobs() into self.logprobs {id: [records]}; returns it."""
        for d in self.poll_logprobs():
            self.logprobs.setdefault(d["id"], []).append(d)
        return self.logprobs

    def stats(self):
        s = L.EngineStats()
        L.check(L.lib().bz_engine_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in L.EngineStats._fields_}

    def prefix_stats(self):
        """The prefix cache's counters (prefix_cache=True): blocks cached / evictable / referenced / private, hits, misses, cached_tokens, evictions,
        prompt_tokens_skipped, copy launches and copied blocks."""
        s = L.EnginePrefixStats()
        L.check(L.lib().bz_engine_prefix_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in L.EnginePrefixStats._fields_ if k != "reserved"}

    def prefix_flush(self):
        """Drops every unreferenced cached block; how many."""
        n = C.c_int()
        L.check(L.lib().bz_engine_prefix_flush(self.h, C.byref(n)))
        return n.value

    def read_status(self, replay):
        """(status words int32 [n_rows]: 0 idle, 1 token, 2 + 4 * reason finished; rows still live after that replay)"""
        st, live = np.zeros(self.n_rows, dtype=np.int32), C.c_int32()
        L.check(L.lib().bz_engine_read_status(self.h, int(replay), _ptr(st), C.byref(live)))
        return st, live.value

    def collect(self, events, into=None):
        """Fold events into {id: [tokens, finish_reason]}."""
        into = self.results if into is None else into
        for rid, tok, _, fin, _ in events:
            r = into.setdefault(rid, [[], -1])
            if tok >= 0:
                r[0].append(int(tok))
            if fin >= 0:
                r[1] = fin
        return into

    def run_until_idle(self):
        """step() until nothing is left; {id: (tokens, finish_reason)} of everything that produced events since the last call."""
        res = {}
        busy = True
        while busy:
            busy = self.step()
            self.collect(self.poll(), res)
        self.collect_logprobs()
        return {k: (v[0], v[1]) for k, v in res.items()}


class DecodeGraph:
    """inference::decode_graph::DecodeGraph (cuda_graphs.rs:97-189) as a hipGraph."""

    def __init__(self, model, kv, max_blocks=0, grammar=None):
        """grammar: a GrammarCursor with n == 1 (Llama family): the step masks its logits row from the cursor's state and advances it on the picked token."""
        h = C.c_void_p()
        if grammar is not None and isinstance(kv, LayeredPagedKvCache):
            L.check(L.lib().bz_decode_graph_capture_paged_grammar(model.h, kv.h, max_blocks or kv.num_blocks, grammar.h, C.byref(h)))
        elif grammar is not None:
            # a model without a KV cache is refused on its architecture before the cache is looked at
            L.check(L.lib().bz_decode_graph_capture_grammar(model.h, None if isinstance(kv, LayeredSsmState) else kv.h, grammar.h, C.byref(h)))
        elif isinstance(kv, LayeredSsmState):
            L.check(L.lib().bz_decode_graph_capture_ssm(model.h, kv.h, C.byref(h)))
        elif isinstance(kv, LayeredPagedKvCache):
            L.check(L.lib().bz_decode_graph_capture_paged(model.h, kv.h, max_blocks or kv.num_blocks, C.byref(h)))
        else:
            L.check(L.lib().bz_decode_graph_capture(model.h, kv.h, C.byref(h)))
        self.h, self.model, self.kv, self.grammar = h, model, kv, grammar

    def __del__(self):
        try:
            if self.h and L.alive:
                L.lib().bz_decode_graph_free(self.h)
        except Exception:
            pass

    def seed_next_token(self, token, position):
        L.check(L.lib().bz_decode_graph_seed(self.h, int(token), int(position)))

    def set_block_table(self, blocks):
        b = np.asarray(blocks, dtype=np.int32)
        L.check(L.lib().bz_decode_graph_set_block_table(self.h, _ptr(b), len(b)))

    def replay(self):
        L.check(L.lib().bz_decode_graph_replay(self.h))

    def read_token(self, step):
        t = C.c_int64()
        L.check(L.lib().bz_decode_graph_read_token(self.h, step, C.byref(t)))
        return t.value

    def read_logits(self):
        out = np.empty(self.model.c.vocab, dtype=np.float32)
        L.check(L.lib().bz_decode_graph_read_logits(self.h, _ptr(out), len(out)))
        return out


class Executor:
    """engine::Executor<R> restricted to token ids in -> token ids out (tokenizer is out of scope)."""

    def __init__(self, model):
        self.model = model

    def generate(self, prompt_tokens, max_tokens, temperature=0.0, repeat_penalty=1.0, repeat_last_n=64, frequency_penalty=0.0,
                 presence_penalty=0.0, eos_id=-1, use_graph=False, paged=False, block_size=16, seed=0, top_k=0, top_p=1.0, min_p=0.0,
                 dry_multiplier=0.0, dry_base=2, dry_allowed_length=0, typical_p=0.0, dynatemp_range=0.0, dynatemp_exponent=1.0, mirostat_mode=0,
                 mirostat_tau=5.0, mirostat_eta=0.1, logit_bias=None, grammar=None, vocab_bytes=None, lora_adapter=None):
        """grammar: a GrammarDfa (used from its current state, left in its final state) with vocab_bytes = the bytes of every token of the model's vocabulary
        (gen_config.grammar, executor_generate.rs:96-121).  lora_adapter: a name registered with load_lora; an unknown name generates without an adapter
        and warns (executor_generate.rs:54-57).  The choice is the request's: on a model with a table, None runs the base model whatever set_lora chose before."""
        if lora_adapter is not None and lora_adapter not in self.model._loras:
            warnings.warn("Requested LoRA adapter '%s' not found in registry -- generating without it" % lora_adapter)
            lora_adapter = None
        if lora_adapter is not None or self.model._lora_slots:
            self.model.set_lora(lora_adapter)
        g = L.GenConfig()
        g.max_tokens, g.temperature, g.repeat_penalty, g.repeat_last_n = max_tokens, temperature, repeat_penalty, repeat_last_n
        g.frequency_penalty, g.presence_penalty = frequency_penalty, presence_penalty
        g.top_k, g.top_p, g.min_p, g.seed = top_k, top_p, min_p, seed
        g.eos_id, g.use_graph, g.paged, g.block_size = eos_id, int(use_graph), int(paged), block_size
        g.dry_multiplier, g.dry_base, g.dry_allowed_length, g.typical_p = dry_multiplier, dry_base, dry_allowed_length, typical_p
        g.dynatemp_range, g.dynatemp_exponent = dynatemp_range, dynatemp_exponent
        g.mirostat_mode, g.mirostat_tau, g.mirostat_eta = mirostat_mode, mirostat_tau, mirostat_eta
        if logit_bias:
            b_ids = np.asarray(list(logit_bias.keys()), dtype=np.uint32)
            b_vals = np.asarray(list(logit_bias.values()), dtype=np.float32)
            g.n_logit_bias, g.logit_bias_ids, g.logit_bias_vals = len(b_ids), b_ids.ctypes.data, b_vals.ctypes.data
        p = np.ascontiguousarray(prompt_tokens, dtype=np.int64)
        out = np.zeros(max(max_tokens, 1), dtype=np.int64)
        st = L.GenStats()
        if grammar is None:
            L.check(L.lib().bz_generate(self.model.h, _ptr(p), len(p), C.byref(g), _ptr(out), C.byref(st)))
        else:
            if vocab_bytes is None:
                raise ValueError("generate: a grammar needs vocab_bytes")
            flat, off = pack_vocab(vocab_bytes)
            L.check(L.lib().bz_generate_grammar(self.model.h, _ptr(p), len(p), C.byref(g), grammar.h, _ptr(flat), _ptr(off), len(off) - 1, _ptr(out), C.byref(st)))
        self.last_stats = dict(prefill_ms=st.prefill_ms, decode_ms=st.decode_ms, n_generated=st.n_generated, finish_reason=st.finish_reason,
                               ttft_ms=st.ttft_ms, total_ms=st.total_ms, itl_p50_ms=st.itl_p50_ms, itl_p99_ms=st.itl_p99_ms, itl_max_ms=st.itl_max_ms,
                               decode_tok_per_s=st.decode_tok_per_s)
        return out[:st.n_generated]


class SpeculativeExecutor:
    """The reference's speculative path (engine/generate_text.rs:61-136, config/inference.rs:197-208): a draft model proposes, the target verifies in one pass.
    Greedy only; the tokens are those Executor(target).generate(...) returns."""

    def __init__(self, target, draft, num_speculative_tokens=5, adaptive_depth=False):
        self.target, self.draft = target, draft
        sc = L.SpecConfig()
        sc.num_speculative_tokens, sc.adaptive_depth = int(num_speculative_tokens), int(bool(adaptive_depth))
        h = C.c_void_p()
        L.check(L.lib().bz_speculative_create(target.h, draft.h, C.byref(sc), C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None) and L.alive:
                L.lib().bz_speculative_free(self.h)
        except Exception:
            pass

    def generate(self, prompt_tokens, max_tokens, temperature=0.0, repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0, eos_id=-1, use_graph=False,
                 paged=False, **sampler):
        g = L.GenConfig()
        g.max_tokens, g.temperature, g.repeat_penalty, g.repeat_last_n = max_tokens, temperature, repeat_penalty, 64
        g.frequency_penalty, g.presence_penalty, g.top_p, g.eos_id = frequency_penalty, presence_penalty, 1.0, eos_id
        g.use_graph, g.paged, g.block_size = int(use_graph), int(paged), 16
        for k, v in sampler.items():      # dry_multiplier, typical_p, dynatemp_range, mirostat_mode ...: refused by the library, passed through so that it can say so
            setattr(g, k, v)
        p = np.ascontiguousarray(prompt_tokens, dtype=np.int64)
        out = np.zeros(max(max_tokens, 1), dtype=np.int64)
        st, ss = L.GenStats(), L.SpecStats()
        L.check(L.lib().bz_generate_speculative(self.h, _ptr(p), len(p), C.byref(g), _ptr(out), C.byref(st), C.byref(ss)))
        self.last_stats = dict(prefill_ms=st.prefill_ms, decode_ms=st.decode_ms, n_generated=st.n_generated, finish_reason=st.finish_reason, ttft_ms=st.ttft_ms,
                               total_ms=st.total_ms, itl_p50_ms=st.itl_p50_ms, itl_p99_ms=st.itl_p99_ms, itl_max_ms=st.itl_max_ms, decode_tok_per_s=st.decode_tok_per_s)
        self.last_spec_stats = dict(iterations=ss.iterations, drafted_tokens=ss.drafted_tokens, accepted_tokens=ss.accepted_tokens, rejected_tokens=ss.rejected_tokens,
                                    verify_path=ss.verify_path, final_depth=ss.final_depth, draft_ms=ss.draft_ms, verify_ms=ss.verify_ms)
        return out[:st.n_generated]
