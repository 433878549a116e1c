// Decoder runtime: weights.  Upload of the int8 / fp16 weight sets (packed
// into MFMA fragment order on the device), the raw weight-file reader and the
// fp32 -> int8 per-column quantiser behind llm_decoder_load_weights,
// llm_quantize_weights and llm_decoder_load_quantized_weights.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <mutex>
#include <string>
#include <vector>

#include "decoder_impl.hpp"
#include "oproj_slices.hpp"

// ---------------------------------------------------------------------------
// weights
// ---------------------------------------------------------------------------
template <typename T>
static int upload(DevBuf<T>& dst, const T* src, size_t n, const char* what) {
  LLM_REQUIRE(src != nullptr, std::string("decoder weights: ") + what + " is NULL");
  RET_IF(dst.alloc(n));
  LLM_HIP_RET(hipMemcpy(dst.p, src, n * sizeof(T), hipMemcpyHostToDevice));
  return LLM_OK;
}

// Upload L row-major [K][N] matrices and pack each into MFMA fragment order.
static int upload_packed(DevBuf<uint8_t>& dst, size_t& per_layer, const void* src, int L, int K,
                         int N, int dtype, const char* what) {
  LLM_REQUIRE(src != nullptr, std::string("decoder weights: ") + what + " is NULL");
  const size_t esz = dtype == LLM_I8 ? 1 : 2;
  per_layer = gemm_packed_bytes(dtype, K, N);
  RET_IF(dst.alloc(per_layer * L));
  void* tmp = nullptr;
  LLM_HIP_RET(hipMalloc(&tmp, (size_t)K * N * esz));
  int rc = LLM_OK;
  for (int l = 0; l < L && rc == LLM_OK; ++l) {
    const char* s = static_cast<const char*>(src) + (size_t)l * K * N * esz;
    if (hipMemcpy(tmp, s, (size_t)K * N * esz, hipMemcpyHostToDevice) != hipSuccess) {
      rc = fail(LLM_ERR_HIP, "decoder weights: upload failed");
      break;
    }
    rc = gemm_pack_weights(dtype, tmp, dst.p + per_layer * l, K, N, nullptr);
  }
  (void)hipDeviceSynchronize();
  (void)hipFree(tmp);
  return rc;
}

static int upload_common(llm_decoder* d, const uint16_t* emb, const float* ln1_g,
                         const float* ln1_b, const float* ln2_g, const float* ln2_b) {
  const size_t Lh = (size_t)d->L * d->hid;
  RET_IF(upload(d->emb, emb, (size_t)d->V * d->hid, "emb"));
  RET_IF(d->emb_packed.alloc(lm_head_packed_bytes(d->V, d->hid)));
  LLM_HIP_RET(launch_lm_pack(d->emb.p, d->emb_packed.p, d->V, d->hid, nullptr));
  LLM_HIP_RET(hipDeviceSynchronize());
  RET_IF(upload(d->ln1_g, ln1_g, Lh, "ln1_g"));
  RET_IF(upload(d->ln1_b, ln1_b, Lh, "ln1_b"));
  RET_IF(upload(d->ln2_g, ln2_g, Lh, "ln2_g"));
  RET_IF(upload(d->ln2_b, ln2_b, Lh, "ln2_b"));
  return LLM_OK;
}

// The weight GEMMs load with the default cache policy (lines stay in the
// 256 MiB Infinity Cache, so the next step's GEMMs hit there) when the whole
// weight set fits well inside it; the KV stream is loaded non-temporal and
// does not displace them.  Larger models stream their weights nt (read once
// per step: keeping them would only churn the cache).  Same-box A/B, two
// runs each (profiles/r03/wkeep_ab.txt): C2 (170 MB of weights) +1.7 / +2.1 %
// kept; C4 (1.2 GB) -2.3 / -2.6 % kept, so nt there.
static int w_keep_for(const llm_decoder* d) {
  const size_t bytes = (d->sz_qkv + d->sz_o + d->sz_1 + d->sz_2) * (size_t)d->L;
  return bytes <= (size_t)192 << 20;
}

extern "C" int llm_decoder_set_int8_weights(llm_decoder* d, const llm_int8_weights* w) {
  LLM_REQUIRE(d && w, "llm_decoder_set_int8_weights: NULL");
  LLM_REQUIRE(d->wdtype == LLM_I8, "llm_decoder_set_int8_weights: decoder is not INT8");
  std::lock_guard<std::mutex> g(d->mu);
  LLM_HIP_RET(hipStreamSynchronize(d->stream));
  const int L = d->L, hid = d->hid, inter = d->inter;
  RET_IF(upload_common(d, w->emb, w->ln1_g, w->ln1_b, w->ln2_g, w->ln2_b));
  RET_IF(upload_packed(d->wqkv, d->sz_qkv, w->wqkv, L, hid, 3 * hid, LLM_I8, "wqkv"));
  RET_IF(upload_packed(d->wo, d->sz_o, w->wo, L, hid, hid, LLM_I8, "wo"));
  RET_IF(upload_packed(d->w1, d->sz_1, w->w1, L, hid, inter, LLM_I8, "w1"));
  RET_IF(upload_packed(d->w2, d->sz_2, w->w2, L, inter, hid, LLM_I8, "w2"));
  RET_IF(upload(d->sw_qkv, w->sw_qkv, (size_t)L * 3 * hid, "sw_qkv"));
  RET_IF(upload(d->sw_o, w->sw_o, (size_t)L * hid, "sw_o"));
  RET_IF(upload(d->sw1, w->sw1, (size_t)L * inter, "sw1"));
  RET_IF(upload(d->sw2, w->sw2, (size_t)L * hid, "sw2"));
  RET_IF(upload(d->b1, w->b1, (size_t)L * inter, "b1"));
  RET_IF(upload(d->b2, w->b2, (size_t)L * hid, "b2"));
  d->w_keep = w_keep_for(d);
  d->drop_step_graph();
  d->weights_ready = true;
  return LLM_OK;
}

extern "C" int llm_decoder_set_f16_weights(llm_decoder* d, const llm_f16_weights* w) {
  LLM_REQUIRE(d && w, "llm_decoder_set_f16_weights: NULL");
  LLM_REQUIRE(d->wdtype == LLM_F16, "llm_decoder_set_f16_weights: decoder is not FP16");
  std::lock_guard<std::mutex> g(d->mu);
  LLM_HIP_RET(hipStreamSynchronize(d->stream));
  const int L = d->L, hid = d->hid, inter = d->inter;
  RET_IF(upload_common(d, w->emb, w->ln1_g, w->ln1_b, w->ln2_g, w->ln2_b));
  RET_IF(upload_packed(d->wqkv, d->sz_qkv, w->wqkv, L, hid, 3 * hid, LLM_F16, "wqkv"));
  RET_IF(upload_packed(d->wo, d->sz_o, w->wo, L, hid, hid, LLM_F16, "wo"));
  // the fused o_proj's head slices: [h][kg][n][j] = W_o[h D + 8 kg + j][n] (a
  // second copy of W_o, L * hid^2 fp16), only where the fused o_proj can run
  // (oproj_fusable); the step then reads these instead of the packed W_o, so
  // the bytes a step streams (w_keep_for) are unchanged
  d->wo_heads.alloc(0);
  if (d->D % 8 == 0 && d->D <= 128 && d->H <= 64 && oproj_fuse_on()) {
    const uint16_t* src = static_cast<const uint16_t*>(w->wo);
    std::vector<uint16_t> sl((size_t)hid * hid);
    RET_IF(d->wo_heads.alloc((size_t)L * hid * hid));
    for (int l = 0; l < L; ++l) {
      oproj_head_slices(src + (size_t)l * hid * hid, d->H, d->D, hid, sl.data());
      LLM_HIP_RET(hipMemcpy(d->wo_heads.p + (size_t)l * hid * hid, sl.data(),
                            sizeof(uint16_t) * hid * hid, hipMemcpyHostToDevice));
    }
  }
  RET_IF(upload_packed(d->w1, d->sz_1, w->w1, L, hid, inter, LLM_F16, "w1"));
  RET_IF(upload_packed(d->w2, d->sz_2, w->w2, L, inter, hid, LLM_F16, "w2"));
  RET_IF(upload(d->b1, w->b1, (size_t)L * inter, "b1"));
  RET_IF(upload(d->b2, w->b2, (size_t)L * hid, "b2"));
  d->w_keep = w_keep_for(d);
  d->drop_step_graph();
  d->weights_ready = true;
  return LLM_OK;
}

// ---------------------------------------------------------------------------
// weight files (weights/README.md:26-38; raw little-endian .bin)
// ---------------------------------------------------------------------------
static int read_file(const std::string& path, std::vector<char>& buf, size_t expect) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) return fail(LLM_ERR_IO, "cannot open weight file: " + path);  // decoder_block.hpp:13-15
  const size_t size = (size_t)f.tellg();
  if (expect && size != expect)
    return fail(LLM_ERR_IO, path + ": expected " + std::to_string(expect) + " bytes, found " +
                                std::to_string(size));
  buf.resize(size);
  f.seekg(0);
  f.read(buf.data(), size);
  if (!f) return fail(LLM_ERR_IO, "failed to read from file: " + path);
  return LLM_OK;
}

static int write_file(const std::string& path, const void* p, size_t n) {
  std::ofstream f(path, std::ios::binary);
  if (!f) return fail(LLM_ERR_IO, "cannot create " + path);
  f.write(static_cast<const char*>(p), n);
  if (!f) return fail(LLM_ERR_IO, "write failed: " + path);
  return LLM_OK;
}

static uint16_t f32_to_f16_bits(float f) {
  const _Float16 h = (_Float16)f;
  uint16_t u;
  std::memcpy(&u, &h, 2);
  return u;
}

// fp32 directory (CUDADecoder::load_weights): embedding.bin [V][hid];
// layer_i/{ln1.bin, ln2.bin} gamma+beta; attn_wq/wk/wv/wo.bin [hid][hid];
// mlp_fc1.bin [hid][inter]; mlp_fc2.bin [inter][hid]; mlp_biases.bin [inter+hid].
struct Fp32Model {
  std::vector<float> emb, ln1, ln2, wqkv, wo, w1, w2, b1, b2;  // ln: [L][2][hid]
};

static int load_fp32_dir(const std::string& dir, int L, int hid, int inter, int V, Fp32Model& m) {
  std::vector<char> buf;
  auto rd = [&](const std::string& p, size_t n, float* dst) -> int {
    RET_IF(read_file(p, buf, n * 4));
    std::memcpy(dst, buf.data(), n * 4);
    return LLM_OK;
  };
  m.emb.resize((size_t)V * hid);
  RET_IF(rd(dir + "/embedding.bin", m.emb.size(), m.emb.data()));
  m.ln1.resize((size_t)L * 2 * hid); m.ln2.resize((size_t)L * 2 * hid);
  m.wqkv.resize((size_t)L * hid * 3 * hid); m.wo.resize((size_t)L * hid * hid);
  m.w1.resize((size_t)L * hid * inter); m.w2.resize((size_t)L * inter * hid);
  m.b1.resize((size_t)L * inter); m.b2.resize((size_t)L * hid);
  std::vector<float> tmp((size_t)hid * hid), bias(inter + hid);
  for (int l = 0; l < L; ++l) {
    const std::string p = dir + "/layer_" + std::to_string(l);
    RET_IF(rd(p + "/ln1.bin", 2 * hid, m.ln1.data() + (size_t)l * 2 * hid));
    RET_IF(rd(p + "/ln2.bin", 2 * hid, m.ln2.data() + (size_t)l * 2 * hid));
    const char* names[3] = {"/attn_wq.bin", "/attn_wk.bin", "/attn_wv.bin"};
    for (int j = 0; j < 3; ++j) {  // fuse q|k|v column blocks: Wqkv[k][j*hid + n]
      RET_IF(rd(p + names[j], (size_t)hid * hid, tmp.data()));
      float* dst = m.wqkv.data() + (size_t)l * hid * 3 * hid;
      for (int k = 0; k < hid; ++k)
        std::memcpy(dst + (size_t)k * 3 * hid + (size_t)j * hid, tmp.data() + (size_t)k * hid,
                    hid * 4);
    }
    RET_IF(rd(p + "/attn_wo.bin", (size_t)hid * hid, m.wo.data() + (size_t)l * hid * hid));
    RET_IF(rd(p + "/mlp_fc1.bin", (size_t)hid * inter, m.w1.data() + (size_t)l * hid * inter));
    RET_IF(rd(p + "/mlp_fc2.bin", (size_t)inter * hid, m.w2.data() + (size_t)l * inter * hid));
    RET_IF(rd(p + "/mlp_biases.bin", (size_t)inter + hid, bias.data()));
    std::memcpy(m.b1.data() + (size_t)l * inter, bias.data(), (size_t)inter * 4);
    std::memcpy(m.b2.data() + (size_t)l * hid, bias.data() + inter, (size_t)hid * 4);
  }
  return LLM_OK;
}

static void split_ln(const std::vector<float>& ln, int L, int hid, std::vector<float>& g,
                     std::vector<float>& b) {
  g.resize((size_t)L * hid);
  b.resize((size_t)L * hid);
  for (int l = 0; l < L; ++l) {
    std::memcpy(g.data() + (size_t)l * hid, ln.data() + (size_t)l * 2 * hid, hid * 4);
    std::memcpy(b.data() + (size_t)l * hid, ln.data() + (size_t)l * 2 * hid + hid, hid * 4);
  }
}

// Per-output-column int8 quantisation (int8_quant.cpp semantics, one scale per column).
static void quantize_cols(const float* w, int K, int N, int8_t* q, float* inv) {
  for (int n = 0; n < N; ++n) {
    float mn = w[n], mx = w[n];
    for (int k = 1; k < K; ++k) {
      mn = std::min(mn, w[(size_t)k * N + n]);
      mx = std::max(mx, w[(size_t)k * N + n]);
    }
    const float absmax = std::max(std::fabs(mn), std::fabs(mx));
    const float scale = 127.f / (absmax + 1e-6f);
    for (int k = 0; k < K; ++k) {
      int v = (int)std::round(w[(size_t)k * N + n] * scale);
      v = std::max(-128, std::min(127, v));
      q[(size_t)k * N + n] = (int8_t)v;
    }
    inv[n] = 1.0f / scale;
  }
}

extern "C" int llm_decoder_load_weights(llm_decoder* d, const char* dir) {
  LLM_REQUIRE(d && dir, "llm_decoder_load_weights: NULL");
  const int L = d->L, hid = d->hid, inter = d->inter, V = d->V;
  Fp32Model m;
  RET_IF(load_fp32_dir(dir, L, hid, inter, V, m));
  std::vector<float> g1, be1, g2, be2;
  split_ln(m.ln1, L, hid, g1, be1);
  split_ln(m.ln2, L, hid, g2, be2);
  std::vector<uint16_t> emb(m.emb.size());
  for (size_t i = 0; i < emb.size(); ++i) emb[i] = f32_to_f16_bits(m.emb[i]);
  if (d->wdtype == LLM_F16) {
    auto cvt = [](const std::vector<float>& s) {
      std::vector<uint16_t> o(s.size());
      for (size_t i = 0; i < s.size(); ++i) o[i] = f32_to_f16_bits(s[i]);
      return o;
    };
    auto qkv = cvt(m.wqkv), wo = cvt(m.wo), w1 = cvt(m.w1), w2 = cvt(m.w2);
    llm_f16_weights w{emb.data(), g1.data(), be1.data(), g2.data(), be2.data(), qkv.data(),
                      wo.data(), w1.data(), w2.data(), m.b1.data(), m.b2.data()};
    return llm_decoder_set_f16_weights(d, &w);
  }
  // INT8 decoder given fp32 weights: quantise on load
  std::vector<int8_t> qqkv(m.wqkv.size()), qo(m.wo.size()), q1(m.w1.size()), q2(m.w2.size());
  std::vector<float> sqkv((size_t)L * 3 * hid), so((size_t)L * hid), s1((size_t)L * inter),
      s2((size_t)L * hid);
  for (int l = 0; l < L; ++l) {
    quantize_cols(m.wqkv.data() + (size_t)l * hid * 3 * hid, hid, 3 * hid,
                  qqkv.data() + (size_t)l * hid * 3 * hid, sqkv.data() + (size_t)l * 3 * hid);
    quantize_cols(m.wo.data() + (size_t)l * hid * hid, hid, hid, qo.data() + (size_t)l * hid * hid,
                  so.data() + (size_t)l * hid);
    quantize_cols(m.w1.data() + (size_t)l * hid * inter, hid, inter,
                  q1.data() + (size_t)l * hid * inter, s1.data() + (size_t)l * inter);
    quantize_cols(m.w2.data() + (size_t)l * inter * hid, inter, hid,
                  q2.data() + (size_t)l * inter * hid, s2.data() + (size_t)l * hid);
  }
  llm_int8_weights w{emb.data(), g1.data(), be1.data(), g2.data(), be2.data(), qqkv.data(),
                     sqkv.data(), qo.data(), so.data(), q1.data(), s1.data(), m.b1.data(),
                     q2.data(), s2.data(), m.b2.data()};
  return llm_decoder_set_int8_weights(d, &w);
}

// INT8 directory written by llm_quantize_weights: embedding.f16 [V][hid] fp16;
// layer_i/{ln1.bin, ln2.bin (fp32 gamma+beta), attn_wqkv.i8 [hid][3hid],
// attn_wqkv.scale [3hid], attn_wo.i8/.scale, mlp_fc1.i8/.scale, mlp_fc2.i8/.scale,
// mlp_biases.bin [inter+hid] fp32}.
extern "C" int llm_quantize_weights(const char* fp32_dir, const char* int8_dir, int num_layers,
                                    int hidden_dim, int inter_dim, int vocab_size) {
  LLM_REQUIRE(fp32_dir && int8_dir && num_layers > 0 && hidden_dim > 0 && vocab_size > 0,
              "llm_quantize_weights: bad arguments");
  const int L = num_layers, hid = hidden_dim, inter = inter_dim > 0 ? inter_dim : 4 * hidden_dim;
  Fp32Model m;
  RET_IF(load_fp32_dir(fp32_dir, L, hid, inter, vocab_size, m));
  const std::string out = int8_dir;
  std::vector<uint16_t> emb(m.emb.size());
  for (size_t i = 0; i < emb.size(); ++i) emb[i] = f32_to_f16_bits(m.emb[i]);
  if (std::system(("mkdir -p '" + out + "'").c_str()) != 0)
    return fail(LLM_ERR_IO, "cannot create " + out);
  RET_IF(write_file(out + "/embedding.f16", emb.data(), emb.size() * 2));
  for (int l = 0; l < L; ++l) {
    const std::string p = out + "/layer_" + std::to_string(l);
    if (std::system(("mkdir -p '" + p + "'").c_str()) != 0)
      return fail(LLM_ERR_IO, "cannot create " + p);
    RET_IF(write_file(p + "/ln1.bin", m.ln1.data() + (size_t)l * 2 * hid, (size_t)2 * hid * 4));
    RET_IF(write_file(p + "/ln2.bin", m.ln2.data() + (size_t)l * 2 * hid, (size_t)2 * hid * 4));
    struct { const char* name; const float* w; int K, N; } mats[4] = {
        {"attn_wqkv", m.wqkv.data() + (size_t)l * hid * 3 * hid, hid, 3 * hid},
        {"attn_wo", m.wo.data() + (size_t)l * hid * hid, hid, hid},
        {"mlp_fc1", m.w1.data() + (size_t)l * hid * inter, hid, inter},
        {"mlp_fc2", m.w2.data() + (size_t)l * inter * hid, inter, hid}};
    for (auto& mt : mats) {
      std::vector<int8_t> q((size_t)mt.K * mt.N);
      std::vector<float> s(mt.N);
      quantize_cols(mt.w, mt.K, mt.N, q.data(), s.data());
      RET_IF(write_file(p + "/" + mt.name + ".i8", q.data(), q.size()));
      RET_IF(write_file(p + "/" + mt.name + ".scale", s.data(), s.size() * 4));
    }
    std::vector<float> bias(inter + hid);
    std::memcpy(bias.data(), m.b1.data() + (size_t)l * inter, (size_t)inter * 4);
    std::memcpy(bias.data() + inter, m.b2.data() + (size_t)l * hid, (size_t)hid * 4);
    RET_IF(write_file(p + "/mlp_biases.bin", bias.data(), bias.size() * 4));
  }
  return LLM_OK;
}

extern "C" int llm_decoder_load_quantized_weights(llm_decoder* d, const char* dir) {
  LLM_REQUIRE(d && dir, "llm_decoder_load_quantized_weights: NULL");
  LLM_REQUIRE(d->wdtype == LLM_I8, "llm_decoder_load_quantized_weights: decoder is not INT8");
  const int L = d->L, hid = d->hid, inter = d->inter, V = d->V;
  const std::string root = dir;
  std::vector<char> buf;
  std::vector<uint16_t> emb((size_t)V * hid);
  RET_IF(read_file(root + "/embedding.f16", buf, emb.size() * 2));
  std::memcpy(emb.data(), buf.data(), emb.size() * 2);
  std::vector<float> g1((size_t)L * hid), be1((size_t)L * hid), g2((size_t)L * hid), be2((size_t)L * hid);
  std::vector<int8_t> qqkv((size_t)L * hid * 3 * hid), qo((size_t)L * hid * hid),
      q1((size_t)L * hid * inter), q2((size_t)L * inter * hid);
  std::vector<float> sqkv((size_t)L * 3 * hid), so((size_t)L * hid), s1((size_t)L * inter),
      s2((size_t)L * hid), b1((size_t)L * inter), b2((size_t)L * hid);
  for (int l = 0; l < L; ++l) {
    const std::string p = root + "/layer_" + std::to_string(l);
    RET_IF(read_file(p + "/ln1.bin", buf, (size_t)2 * hid * 4));
    std::memcpy(g1.data() + (size_t)l * hid, buf.data(), hid * 4);
    std::memcpy(be1.data() + (size_t)l * hid, buf.data() + hid * 4, hid * 4);
    RET_IF(read_file(p + "/ln2.bin", buf, (size_t)2 * hid * 4));
    std::memcpy(g2.data() + (size_t)l * hid, buf.data(), hid * 4);
    std::memcpy(be2.data() + (size_t)l * hid, buf.data() + hid * 4, hid * 4);
    struct { const char* name; int8_t* q; float* s; int K, N; } mats[4] = {
        {"attn_wqkv", qqkv.data() + (size_t)l * hid * 3 * hid, sqkv.data() + (size_t)l * 3 * hid, hid, 3 * hid},
        {"attn_wo", qo.data() + (size_t)l * hid * hid, so.data() + (size_t)l * hid, hid, hid},
        {"mlp_fc1", q1.data() + (size_t)l * hid * inter, s1.data() + (size_t)l * inter, hid, inter},
        {"mlp_fc2", q2.data() + (size_t)l * inter * hid, s2.data() + (size_t)l * hid, inter, hid}};
    for (auto& mt : mats) {
      RET_IF(read_file(p + "/" + mt.name + ".i8", buf, (size_t)mt.K * mt.N));
      std::memcpy(mt.q, buf.data(), (size_t)mt.K * mt.N);
      RET_IF(read_file(p + "/" + mt.name + ".scale", buf, (size_t)mt.N * 4));
      std::memcpy(mt.s, buf.data(), (size_t)mt.N * 4);
    }
    RET_IF(read_file(p + "/mlp_biases.bin", buf, (size_t)(inter + hid) * 4));
    std::memcpy(b1.data() + (size_t)l * inter, buf.data(), (size_t)inter * 4);
    std::memcpy(b2.data() + (size_t)l * hid, buf.data() + (size_t)inter * 4, (size_t)hid * 4);
  }
  llm_int8_weights w{emb.data(), g1.data(), be1.data(), g2.data(), be2.data(), qqkv.data(),
                     sqkv.data(), qo.data(), so.data(), q1.data(), s1.data(), b1.data(),
                     q2.data(), s2.data(), b2.data()};
  return llm_decoder_set_int8_weights(d, &w);
}
