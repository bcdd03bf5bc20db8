// Stand-alone host check of the loader's compressed-tensors parsing (int-quantized accepted, every refusal of DESIGN 4 "INT8 W8A8 weights"), meant to be built
// with the host sanitizers -- bz_loader.hip compiled into this program, the rest of the library from libblazr_hip.so.  No device is touched.
//   cd blazr_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I../../include \
//     ../../scripts/int8_config_asan.cpp bz_loader.hip -L.. -lblazr_hip -Wl,-rpath,$PWD/.. -o /tmp/int8_config_asan && /tmp/int8_config_asan
#include <cstdio>
#include <string>

#include "blazr_hip.h"

static std::string cfg(const std::string& fmt, const std::string& weights, const std::string& acts) {
  return "{\"model_type\":\"llama\",\"vocab_size\":1024,\"hidden_size\":256,\"num_hidden_layers\":2,\"num_attention_heads\":4,\"num_key_value_heads\":2,"
         "\"intermediate_size\":512,\"torch_dtype\":\"bfloat16\",\"quantization_config\":{\"quant_method\":\"compressed-tensors\",\"format\":\"" + fmt +
         "\",\"ignore\":[\"lm_head\"],\"config_groups\":{\"group_0\":{\"targets\":[\"Linear\"],\"weights\":{" + weights + "}" +
         (acts.empty() ? "" : ",\"input_activations\":{" + acts + "}") + "}}}}";
}

int main() {
  const std::string W = "\"num_bits\":8,\"type\":\"int\",\"strategy\":\"channel\",\"symmetric\":true", A = "\"num_bits\":8,\"type\":\"int\",\"strategy\":\"token\",\"symmetric\":true,\"dynamic\":true";
  struct Case { std::string json; int want_method; } cases[] = {
    {cfg("int-quantized", W, A), 5},
    {cfg("int-quantized", "\"num_bits\":8,\"type\":\"int\",\"strategy\":\"tensor\"", A), 5},
    {cfg("float-quantized", "\"num_bits\":8,\"type\":\"float\",\"strategy\":\"channel\"", ""), 3},
    {cfg("int-quantized", W, ""), -1},
    {cfg("int-quantized", W, "\"num_bits\":8,\"type\":\"int\",\"strategy\":\"token\",\"symmetric\":true,\"dynamic\":false"), -1},
    {cfg("int-quantized", W, "\"num_bits\":8,\"type\":\"int\",\"strategy\":\"tensor\",\"dynamic\":true"), -1},
    {cfg("int-quantized", W, "\"num_bits\":16,\"type\":\"int\",\"strategy\":\"token\",\"dynamic\":true"), -1},
    {cfg("int-quantized", W, "\"num_bits\":8,\"type\":\"int\",\"strategy\":\"token\",\"symmetric\":false,\"dynamic\":true"), -1},
    {cfg("int-quantized", "\"num_bits\":8,\"type\":\"int\",\"strategy\":\"group\",\"group_size\":128", A), -1},
    {cfg("int-quantized", "\"num_bits\":4,\"type\":\"int\",\"strategy\":\"channel\"", A), -1},
    {cfg("int-quantized", "\"num_bits\":8,\"type\":\"int\",\"strategy\":\"channel\",\"symmetric\":false", A), -1},
    {cfg("pack-quantized", W, A), -1},
    {cfg("int-quantized", W, A).substr(0, 300), -1},      // a truncated file
  };
  int bad = 0;
  for (const Case& c : cases) {
    bz_model_config mc; bz_quant_info q;
    const int rc = bz_config_from_hf_json(c.json.c_str(), &mc, &q);
    const bool ok = c.want_method < 0 ? rc != BZ_OK : (rc == BZ_OK && q.quant_method == c.want_method);
    printf("%s rc=%d method=%d %s\n", ok ? "ok  " : "FAIL", rc, rc == BZ_OK ? q.quant_method : -1, rc == BZ_OK ? "" : bz_last_error());
    bad += !ok;
  }
  return bad;
}
