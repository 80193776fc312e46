// gltf_loader.cpp — host C++ restatement of src/scene/loader/gltf_loader.rs behind the C ABI:
// `hala_scene_load_gltf` is cpu::HalaScene::new (src/scene/cpu/scene.rs:40-55); the scene it returns is the borrowed
// `hala_scene_desc` that `hala_rt_set_scene` consumes.  Rule by rule like the reference (each rule cites its lines); the
// reference delegates parsing to the `gltf` and `image` crates — here: the library's own JSON reader, base64, accessor
// decoding, a PNG decoder over zlib (1..16-bit, grey / RGB / palette / alpha, plain or Adam7-interlaced), a Huffman JPEG decoder
// (jpeg_decode.cpp: sequential and progressive), PGM / PPM and TGA.  Anything else (arithmetic-coded or lossless JPEG, other
// containers) is reported as "Unsupported image format." (the Python mirror hala-renderer_amd/gltf_loader.py decodes with PIL).
#include <zlib.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/halart.h"
#include "host_util.h"

using rt::JsonValue;
namespace rt { bool decode_jpeg(const std::vector<uint8_t>& raw, uint32_t* w, uint32_t* h, std::vector<uint8_t>* rgba); }  // jpeg_decode.cpp

struct hala_scene {
  std::deque<std::string> names;  // stable addresses for hala_node_desc::name
  std::vector<hala_node_desc> nodes;
  std::deque<std::vector<uint32_t>> indices;
  std::deque<std::vector<hala_vertex>> vertices;
  std::deque<std::vector<hala_primitive_desc>> prims;
  std::vector<hala_mesh_desc> meshes;
  std::vector<hala_material_desc> materials;
  std::vector<hala_light_desc> lights;
  std::vector<hala_camera_desc> cameras;
  std::vector<hala_index_pair> tex2img, img2data;
  std::deque<std::vector<uint8_t>> pixels;
  std::vector<hala_image_desc> images;
  hala_scene_desc desc{};
  // the rig (RENDER_SPEC 19): hala_rig_desc and the arrays it borrows
  struct Rig {
    std::vector<hala_rig_node> nodes;
    std::vector<uint32_t> node_of_gltf, gltf_of_node;
    std::deque<std::vector<uint32_t>> u32s;
    std::deque<std::vector<uint16_t>> u16s;
    std::deque<std::vector<float>> f32s;
    std::deque<std::vector<hala_rig_sampler>> samplers;
    std::deque<std::vector<hala_rig_channel>> channels;
    std::deque<std::string> names;
    std::vector<hala_rig_skin> skins;
    std::vector<hala_rig_binding> bindings;
    std::vector<hala_rig_clip> clips;
    hala_rig_desc desc{};
  } rig;
};

namespace {

struct LoadError { std::string msg; };
[[noreturn]] void fail(const std::string& m) { throw LoadError{m}; }

// ---- JSON helpers ---------------------------------------------------------------------------------------------------
const JsonValue* get(const JsonValue& o, const char* key) { return o.kind == JsonValue::Object ? o.find(key) : nullptr; }
double num(const JsonValue& o, const char* key, double dflt) {
  const JsonValue* v = get(o, key);
  return (v && v->kind == JsonValue::Number) ? v->num : dflt;
}
bool has(const JsonValue& o, const char* key) { return get(o, key) != nullptr; }
// JSON numbers that stand for counts, offsets and indices must be finite non-negative integers that fit the target type
// (a cast of NaN / a negative / 1e300 is undefined behaviour; serde rejects them in the reference's gltf crate too)
uint64_t checked_uint(double v, uint64_t max, const char* what) {
  if (!(v >= 0.0) || v > (double)max || v != std::floor(v)) fail(std::string("The glTF value of `") + what + "` is not a non-negative integer in range.");
  return (uint64_t)v;
}
size_t usize(const JsonValue& o, const char* key, size_t dflt) {
  const JsonValue* v = get(o, key);
  return (v && v->kind == JsonValue::Number) ? (size_t)checked_uint(v->num, (uint64_t)1 << 48, key) : dflt;
}
uint32_t json_index(const JsonValue& v) {
  if (v.kind != JsonValue::Number) fail("A glTF index is not a number.");
  return (uint32_t)checked_uint(v.num, 0xfffffffeull, "index");
}
uint32_t index_or_invalid(const JsonValue& o, const char* key) {
  const JsonValue* v = get(o, key);
  return (v && v->kind == JsonValue::Number) ? (uint32_t)checked_uint(v->num, 0xfffffffeull, key) : HALA_INVALID_INDEX;
}
const std::vector<JsonValue>& arr(const JsonValue& o, const char* key) {
  static const std::vector<JsonValue> empty;
  const JsonValue* v = get(o, key);
  return (v && v->kind == JsonValue::Array) ? v->items : empty;
}
void floats(const JsonValue& o, const char* key, float* out, int n, const float* dflt) {
  const JsonValue* v = get(o, key);
  for (int i = 0; i < n; ++i) out[i] = (v && v->kind == JsonValue::Array && (size_t)i < v->items.size()) ? (float)v->items[i].num : dflt[i];
}

// ---- bytes: files, data URIs ----------------------------------------------------------------------------------------
std::vector<uint8_t> read_file(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) fail("Open file \"" + path + "\" failed.");
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
std::vector<uint8_t> base64_decode(const std::string& s, size_t from) {
  static int8_t table[256];
  static bool init = false;
  if (!init) {
    memset(table, -1, sizeof(table));
    const char* a = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
    for (int i = 0; i < 64; ++i) table[(uint8_t)a[i]] = (int8_t)i;
    init = true;
  }
  std::vector<uint8_t> out;
  uint32_t acc = 0; int bits = 0;
  for (size_t i = from; i < s.size(); ++i) {
    const int8_t v = table[(uint8_t)s[i]];
    if (v < 0) continue;  // padding, whitespace
    acc = (acc << 6) | (uint32_t)v; bits += 6;
    if (bits >= 8) { bits -= 8; out.push_back((uint8_t)(acc >> bits)); }
  }
  return out;
}
struct Doc {
  std::string dir;
  JsonValue j;
  std::vector<std::vector<uint8_t>> buffers;
  std::vector<uint8_t> load_uri(const std::string& uri) const {
    if (uri.rfind("data:", 0) == 0) {
      const size_t comma = uri.find(',');
      if (comma == std::string::npos) fail("Malformed data URI.");
      return base64_decode(uri, comma + 1);
    }
    return read_file(dir.empty() ? uri : dir + "/" + uri);
  }
};

// ---- accessors ------------------------------------------------------------------------------------------------------
struct Accessor { std::vector<double> v; int ncomp = 0; size_t count = 0; };
int component_size(int ct) {
  switch (ct) { case 5120: case 5121: return 1; case 5122: case 5123: return 2; case 5125: case 5126: return 4; default: fail("Unknown component type."); }
  return 0;
}
// `count` elements of `ncomp` components of type `ct` from a buffer view (tightly packed unless the view has a stride and `strided`)
void read_elements(const Doc& d, uint32_t bvi, size_t byte_offset, int ct, int ncomp, size_t count, bool normalized, bool strided, std::vector<double>* out) {
  const auto& views = arr(d.j, "bufferViews");
  if (bvi >= views.size()) fail("Buffer view index out of range.");
  const JsonValue& bv = views[bvi];
  const uint32_t bi = index_or_invalid(bv, "buffer");
  if (bi >= d.buffers.size()) fail("Buffer index out of range.");
  const int size = component_size(ct);
  const size_t off = usize(bv, "byteOffset", 0) + byte_offset;
  size_t stride = strided ? usize(bv, "byteStride", 0) : 0;
  if (stride == 0) stride = (size_t)size * ncomp;
  const std::vector<uint8_t>& buf = d.buffers[bi];
  if (count && (off > buf.size() || (count - 1) > (buf.size() - off) / stride || off + (count - 1) * stride + (size_t)size * ncomp > buf.size()))
    fail("Accessor reads past the end of its buffer.");
  out->resize(count * ncomp);
  for (size_t i = 0; i < count; ++i)
    for (int c = 0; c < ncomp; ++c) {
      const uint8_t* p = buf.data() + off + i * stride + (size_t)c * size;
      double x = 0.0, mx = 1.0;
      switch (ct) {
        case 5120: { int8_t t; memcpy(&t, p, 1); x = t; mx = 127.0; break; }
        case 5121: { uint8_t t; memcpy(&t, p, 1); x = t; mx = 255.0; break; }
        case 5122: { int16_t t; memcpy(&t, p, 2); x = t; mx = 32767.0; break; }
        case 5123: { uint16_t t; memcpy(&t, p, 2); x = t; mx = 65535.0; break; }
        case 5125: { uint32_t t; memcpy(&t, p, 4); x = t; mx = 4294967295.0; break; }
        default: { float t; memcpy(&t, p, 4); x = t; break; }
      }
      (*out)[i * ncomp + c] = normalized ? (double)((float)x / (float)mx) : x;
    }
}
Accessor read_accessor(const Doc& d, uint32_t idx) {
  const auto& accs = arr(d.j, "accessors");
  if (idx >= accs.size()) fail("Accessor index out of range.");
  const JsonValue& a = accs[idx];
  const int ct = (int)usize(a, "componentType", 0);
  const JsonValue* ty = get(a, "type");
  static const std::map<std::string, int> ncomp = {{"SCALAR", 1}, {"VEC2", 2}, {"VEC3", 3}, {"VEC4", 4}, {"MAT2", 4}, {"MAT3", 9}, {"MAT4", 16}};
  if (!ty || !ncomp.count(ty->str)) fail("Unknown accessor type.");
  (void)component_size(ct);
  Accessor out;
  out.ncomp = ncomp.at(ty->str);
  out.count = usize(a, "count", 0);
  if (out.count > (size_t)1 << 31) fail("Accessor count is out of range.");
  const JsonValue* nrm = get(a, "normalized");
  const bool normalized = nrm && nrm->kind == JsonValue::Bool && nrm->b && ct != 5126;
  const JsonValue* sparse = get(a, "sparse");
  const uint32_t bvi = index_or_invalid(a, "bufferView");
  if (bvi != HALA_INVALID_INDEX) read_elements(d, bvi, usize(a, "byteOffset", 0), ct, out.ncomp, out.count, normalized, true, &out.v);
  else if (sparse) out.v.assign(out.count * out.ncomp, 0.0);  // glTF 2.0 3.6.2.3: no buffer view -> zeros, then the sparse substitution
  else fail("Accessor without a buffer view.");
  if (sparse) {  // `count` elements replaced: their indices (strictly increasing) and their values, both tightly packed
    const size_t n = usize(*sparse, "count", 0);
    const JsonValue* si = get(*sparse, "indices");
    const JsonValue* sv = get(*sparse, "values");
    if (!si || !sv || n == 0 || n > out.count) fail("Malformed sparse accessor.");
    const int ict = (int)usize(*si, "componentType", 0);
    if (ict != 5121 && ict != 5123 && ict != 5125) fail("Sparse accessor indices must be unsigned.");
    std::vector<double> ind, val;
    read_elements(d, index_or_invalid(*si, "bufferView"), usize(*si, "byteOffset", 0), ict, 1, n, false, false, &ind);
    read_elements(d, index_or_invalid(*sv, "bufferView"), usize(*sv, "byteOffset", 0), ct, out.ncomp, n, normalized, false, &val);
    double prev = -1.0;
    for (size_t k = 0; k < n; ++k) {
      if (!(ind[k] > prev) || ind[k] >= (double)out.count) fail("Sparse accessor indices must increase and stay inside the accessor.");
      prev = ind[k];
      for (int c = 0; c < out.ncomp; ++c) out.v[(size_t)ind[k] * out.ncomp + c] = val[k * out.ncomp + c];
    }
  }
  return out;
}

// gltf::scene::Transform::matrix(): explicit matrix, or T*R*S evaluated in double and rounded once; column-major out
void node_matrix(const JsonValue& n, float m[16]) {
  if (const JsonValue* mv = get(n, "matrix")) {
    for (int i = 0; i < 16; ++i) m[i] = (size_t)i < mv->items.size() ? (float)mv->items[i].num : (i % 5 == 0 ? 1.0f : 0.0f);
    return;
  }
  // T * R * S from the JSON numbers themselves (double), rounded to binary32 once, like the Python mirror
  auto dbl = [&](const char* key, int i, double dflt) { const JsonValue* v = get(n, key); return (v && (size_t)i < v->items.size()) ? v->items[i].num : dflt; };
  const double x = dbl("rotation", 0, 0), y = dbl("rotation", 1, 0), z = dbl("rotation", 2, 0), w = dbl("rotation", 3, 1);
  const double s[3] = {dbl("scale", 0, 1), dbl("scale", 1, 1), dbl("scale", 2, 1)};
  const double r[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                          {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                          {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
  for (int c = 0; c < 3; ++c) {
    for (int rr = 0; rr < 3; ++rr) m[4 * c + rr] = (float)(r[rr][c] * s[c]);
    m[4 * c + 3] = 0.0f;
  }
  m[12] = (float)dbl("translation", 0, 0); m[13] = (float)dbl("translation", 1, 0); m[14] = (float)dbl("translation", 2, 0); m[15] = 1.0f;
}

// ---- PNG over zlib --------------------------------------------------------------------------------------------------
constexpr uint32_t kMaxImageDim = 32768;  // decoded RGBA8 <= 4 GiB; larger headers are treated as malformed
uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
// decodes to RGBA8 (16-bit samples keep their high byte, like image::DynamicImage::into_rgba8's >> 8 ... rounding aside)
bool decode_png(const std::vector<uint8_t>& raw, uint32_t* w, uint32_t* h, std::vector<uint8_t>* rgba) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  if (raw.size() < 33 || memcmp(raw.data(), sig, 8) != 0) return false;
  size_t pos = 8;
  uint32_t width = 0, height = 0;
  int depth = 0, ctype = 0, interlace = 0;
  std::vector<uint8_t> idat, plte, trns;
  bool first = true;
  while (pos + 12 <= raw.size()) {
    const uint32_t len = be32(&raw[pos]);
    const char* type = reinterpret_cast<const char*>(&raw[pos + 4]);
    if (pos + 12 + (size_t)len > raw.size()) return false;
    const uint8_t* data = &raw[pos + 8];
    const bool ihdr = !memcmp(type, "IHDR", 4);
    if (first != ihdr || (ihdr && len != 13)) return false;  // IHDR is the first chunk, exactly once, 13 bytes (PNG 11.2.2)
    first = false;
    if (ihdr) { width = be32(data); height = be32(data + 4); depth = data[8]; ctype = data[9]; interlace = data[12]; }
    else if (!memcmp(type, "PLTE", 4)) plte.assign(data, data + len);
    else if (!memcmp(type, "tRNS", 4)) trns.assign(data, data + len);
    else if (!memcmp(type, "IDAT", 4)) idat.insert(idat.end(), data, data + len);
    else if (!memcmp(type, "IEND", 4)) break;
    pos += 12 + (size_t)len;
  }
  if (!width || !height || width > kMaxImageDim || height > kMaxImageDim || interlace > 1) return false;
  int channels = 0;
  switch (ctype) { case 0: channels = 1; break; case 2: channels = 3; break; case 3: channels = 1; break; case 4: channels = 2; break; case 6: channels = 4; break; default: return false; }
  if (!(depth == 8 || depth == 16 || (depth < 8 && (ctype == 0 || ctype == 3)))) return false;
  const size_t bpp_bits = (size_t)channels * depth, bpp = std::max<size_t>(1, bpp_bits / 8);
  // the image is one pass, or the seven Adam7 passes (PNG 8.2): pass p holds the pixels (x0 + i dx, y0 + j dy), filtered as an image of its own
  struct Pass { uint32_t x0, y0, dx, dy; };
  static const Pass adam7[7] = {{0, 0, 8, 8}, {4, 0, 8, 8}, {0, 4, 4, 8}, {2, 0, 4, 4}, {0, 2, 2, 4}, {1, 0, 2, 2}, {0, 1, 1, 2}};
  static const Pass whole[1] = {{0, 0, 1, 1}};
  const Pass* passes = interlace ? adam7 : whole;
  const int pass_count = interlace ? 7 : 1;
  size_t total = 0;
  for (int p = 0; p < pass_count; ++p) {
    const size_t pw = passes[p].x0 < width ? (width - passes[p].x0 + passes[p].dx - 1) / passes[p].dx : 0;
    const size_t ph = passes[p].y0 < height ? (height - passes[p].y0 + passes[p].dy - 1) / passes[p].dy : 0;
    if (pw && ph) total += ((pw * bpp_bits + 7) / 8 + 1) * ph;
  }
  std::vector<uint8_t> data(total);
  uLongf out_len = (uLongf)data.size();
  if (uncompress(data.data(), &out_len, idat.data(), (uLong)idat.size()) != Z_OK || out_len != data.size()) return false;
  rgba->assign((size_t)width * height * 4, 255);
  size_t at = 0;
  for (int p = 0; p < pass_count; ++p) {
    const Pass ps = passes[p];
    const uint32_t pw = ps.x0 < width ? (width - ps.x0 + ps.dx - 1) / ps.dx : 0, ph = ps.y0 < height ? (height - ps.y0 + ps.dy - 1) / ps.dy : 0;
    if (!pw || !ph) continue;
    const size_t row_bytes = ((size_t)pw * bpp_bits + 7) / 8;
    std::vector<uint8_t> prev(row_bytes, 0), cur(row_bytes);
    for (uint32_t y = 0; y < ph; ++y) {
      const uint8_t* in = &data[at];
      at += row_bytes + 1;
      const int filter = in[0];
      for (size_t i = 0; i < row_bytes; ++i) {
        const int a = i >= bpp ? cur[i - bpp] : 0, b = prev[i], c = i >= bpp ? prev[i - bpp] : 0;
        int x = in[1 + i];
        switch (filter) {
          case 0: break;
          case 1: x += a; break;
          case 2: x += b; break;
          case 3: x += (a + b) / 2; break;
          case 4: { const int q = a + b - c, pa = abs(q - a), pb = abs(q - b), pc = abs(q - c); x += (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c); break; }
          default: return false;
        }
        cur[i] = (uint8_t)x;
      }
      for (uint32_t xx = 0; xx < pw; ++xx) {
        uint8_t* px = &(*rgba)[((size_t)(ps.y0 + y * ps.dy) * width + ps.x0 + xx * ps.dx) * 4];
        auto sample = [&](int ch) -> uint32_t {  // 8-bit value of channel ch of pixel xx of this pass row
          if (depth == 8) return cur[(size_t)xx * channels + ch];
          if (depth == 16) return cur[((size_t)xx * channels + ch) * 2];
          const size_t bit = (size_t)xx * depth;
          const uint32_t v = (cur[bit / 8] >> (8 - depth - (bit % 8))) & ((1u << depth) - 1u);
          return ctype == 3 ? v : v * 255u / ((1u << depth) - 1u);
        };
        if (ctype == 3) {
          const uint32_t idx = sample(0);
          if ((size_t)idx * 3 + 2 >= plte.size()) return false;
          px[0] = plte[idx * 3]; px[1] = plte[idx * 3 + 1]; px[2] = plte[idx * 3 + 2];
          px[3] = idx < trns.size() ? trns[idx] : 255;
        } else if (ctype == 0 || ctype == 4) {
          px[0] = px[1] = px[2] = (uint8_t)sample(0);
          px[3] = ctype == 4 ? (uint8_t)sample(1) : 255;
        } else {
          px[0] = (uint8_t)sample(0); px[1] = (uint8_t)sample(1); px[2] = (uint8_t)sample(2);
          px[3] = ctype == 6 ? (uint8_t)sample(3) : 255;
        }
      }
      prev.swap(cur);
    }
  }
  *w = width; *h = height;
  return true;
}

// ---- PNM and TGA: the other 8-bit formats the reference's `image` dependency is built with (Cargo.toml features pnm, tga) ------------
// binary or plain PGM / PPM, maxval 255: "P5"/"P6"/"P2"/"P3", whitespace- and '#'-comment separated header fields
bool decode_pnm(const std::vector<uint8_t>& raw, uint32_t* w, uint32_t* h, std::vector<uint8_t>* rgba) {
  if (raw.size() < 7 || raw[0] != 'P' || (raw[1] != '5' && raw[1] != '6' && raw[1] != '2' && raw[1] != '3')) return false;
  const bool plain = raw[1] == '2' || raw[1] == '3';
  const uint32_t channels = raw[1] == '6' || raw[1] == '3' ? 3u : 1u;
  size_t pos = 2;
  auto skip = [&]() {  // whitespace and comments up to the end of their line
    while (pos < raw.size()) {
      if (raw[pos] == '#') { while (pos < raw.size() && raw[pos] != '\n') ++pos; }
      else if (raw[pos] == ' ' || raw[pos] == '\t' || raw[pos] == '\r' || raw[pos] == '\n' || raw[pos] == '\v' || raw[pos] == '\f') ++pos;
      else break;
    }
  };
  auto number = [&](uint32_t* out) {
    skip();
    uint64_t v = 0;
    size_t digits = 0;
    while (pos < raw.size() && raw[pos] >= '0' && raw[pos] <= '9' && digits < 10) { v = v * 10 + (raw[pos] - '0'); ++pos; ++digits; }
    if (digits == 0 || v > 0xffffffffull) return false;
    *out = (uint32_t)v;
    return true;
  };
  uint32_t width = 0, height = 0, maxval = 0;
  if (!number(&width) || !number(&height) || !number(&maxval)) return false;
  if (width == 0 || height == 0 || width > kMaxImageDim || height > kMaxImageDim || maxval != 255u) return false;
  const size_t n = (size_t)width * height;
  std::vector<uint8_t> px(n * 4);
  if (!plain) {
    if (pos >= raw.size()) return false;
    ++pos;  // the single whitespace byte after maxval
    if (raw.size() - pos < n * channels) return false;
    const uint8_t* s = raw.data() + pos;
    for (size_t i = 0; i < n; ++i) {
      px[4 * i] = s[channels * i];
      px[4 * i + 1] = s[channels * i + (channels == 3 ? 1 : 0)];
      px[4 * i + 2] = s[channels * i + (channels == 3 ? 2 : 0)];
      px[4 * i + 3] = 255;
    }
  } else {
    if (raw.size() - pos < n * channels * 2) return false;  // a sample and its separator take two bytes at least
    for (size_t i = 0; i < n; ++i) {
      uint32_t v[3] = {0, 0, 0};
      for (uint32_t c = 0; c < channels; ++c) if (!number(&v[c]) || v[c] > 255u) return false;
      px[4 * i] = (uint8_t)v[0];
      px[4 * i + 1] = (uint8_t)v[channels == 3 ? 1 : 0];
      px[4 * i + 2] = (uint8_t)v[channels == 3 ? 2 : 0];
      px[4 * i + 3] = 255;
    }
  }
  *w = width; *h = height; *rgba = std::move(px);
  return true;
}

// TGA has no magic number: the 18-byte header must be self-consistent.  Image types 1/9 (colour-mapped), 2/10 (true colour), 3/11 (grey),
// the upper ones run-length encoded; 8-bit indices or grey, 24/32-bit BGR(A) pixels and colour-map entries; both row orders and both
// column orders (descriptor bits 5 and 4).
bool decode_tga(const std::vector<uint8_t>& raw, uint32_t* w, uint32_t* h, std::vector<uint8_t>* rgba) {
  if (raw.size() < 18) return false;
  const uint8_t* hd = raw.data();
  const uint32_t id_len = hd[0], cmap_type = hd[1], type = hd[2];
  const uint32_t cmap_first = hd[3] | (hd[4] << 8), cmap_len = hd[5] | (hd[6] << 8), cmap_bits = hd[7];
  const uint32_t width = hd[12] | (hd[13] << 8), height = hd[14] | (hd[15] << 8), bpp = hd[16], desc = hd[17];
  const bool rle = type >= 9;
  const uint32_t kind = rle ? type - 8 : type;  // 1 mapped, 2 true colour, 3 grey
  if (kind < 1 || kind > 3 || type > 11 || cmap_type > 1 || width == 0 || height == 0 || (desc & 0xc0)) return false;
  if (kind == 1 && (cmap_type != 1 || bpp != 8 || (cmap_bits != 24 && cmap_bits != 32) || cmap_len == 0)) return false;
  if (kind == 2 && bpp != 24 && bpp != 32) return false;
  if (kind == 3 && bpp != 8) return false;
  if (cmap_type == 1 && cmap_bits != 15 && cmap_bits != 16 && cmap_bits != 24 && cmap_bits != 32) return false;
  size_t pos = 18 + (size_t)id_len;
  const size_t cmap_bytes = cmap_type ? (size_t)cmap_len * ((cmap_bits + 7) / 8) : 0;
  if (pos + cmap_bytes > raw.size()) return false;
  const uint8_t* cmap = raw.data() + pos;
  pos += cmap_bytes;
  const uint32_t bytes = bpp / 8;
  const size_t n = (size_t)width * height;
  std::vector<uint8_t> src(n * bytes);
  if (!rle) {
    if (raw.size() - pos < n * bytes) return false;
    memcpy(src.data(), raw.data() + pos, n * bytes);
  } else {
    size_t done = 0;
    while (done < n) {
      if (pos >= raw.size()) return false;
      const uint32_t head = raw[pos++], count = (head & 0x7f) + 1;
      if (done + count > n) return false;
      if (head & 0x80) {
        if (raw.size() - pos < bytes) return false;
        for (uint32_t k = 0; k < count; ++k) memcpy(&src[(done + k) * bytes], &raw[pos], bytes);
        pos += bytes;
      } else {
        if (raw.size() - pos < (size_t)count * bytes) return false;
        memcpy(&src[done * bytes], &raw[pos], (size_t)count * bytes);
        pos += (size_t)count * bytes;
      }
      done += count;
    }
  }
  std::vector<uint8_t> px(n * 4);
  const bool top_down = (desc & 0x20) != 0, right_left = (desc & 0x10) != 0;
  const uint32_t cmap_entry = cmap_bits / 8;
  for (uint32_t y = 0; y < height; ++y) {
    const uint32_t oy = top_down ? y : height - 1 - y;
    for (uint32_t x = 0; x < width; ++x) {
      const uint32_t ox = right_left ? width - 1 - x : x;
      const uint8_t* s = &src[((size_t)y * width + x) * bytes];
      uint8_t* o = &px[((size_t)oy * width + ox) * 4];
      if (kind == 3) { o[0] = o[1] = o[2] = s[0]; o[3] = 255; }
      else if (kind == 2) { o[0] = s[2]; o[1] = s[1]; o[2] = s[0]; o[3] = bytes == 4 ? s[3] : 255; }
      else {
        const uint32_t index = s[0];
        if (index < cmap_first || index - cmap_first >= cmap_len) return false;
        const uint8_t* e = cmap + (size_t)(index - cmap_first) * cmap_entry;
        o[0] = e[2]; o[1] = e[1]; o[2] = e[0]; o[3] = cmap_entry == 4 ? e[3] : 255;
      }
    }
  }
  *w = width; *h = height; *rgba = std::move(px);
  return true;
}

// the sniffing order: signatures first, the header-only format last
bool decode_image_rgba8(const std::vector<uint8_t>& raw, uint32_t* w, uint32_t* h, std::vector<uint8_t>* rgba) {
  return decode_png(raw, w, h, rgba) || rt::decode_jpeg(raw, w, h, rgba) || decode_pnm(raw, w, h, rgba) || decode_tga(raw, w, h, rgba);
}


// ---- the loader (gltf_loader.rs:121-227) ----------------------------------------------------------------------------
void load_mesh(const Doc& d, const JsonValue& mesh, hala_scene* s) {  // :232-313
  const JsonValue* nm = get(mesh, "name");
  const std::string name = nm ? nm->str : "<Unnamed>";
  std::vector<hala_primitive_desc> prims;
  for (const JsonValue& p : arr(mesh, "primitives")) {
    const JsonValue* attr = get(p, "attributes");
    if (!has(p, "indices")) fail("Read indices from mesh \"" + name + "\" failed.");  // :243
    const Accessor ia = read_accessor(d, index_or_invalid(p, "indices"));
    std::vector<uint32_t> idx(ia.v.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = (uint32_t)ia.v[i];  // into_u32 :244
    static const char* req[3][2] = {{"POSITION", "positions"}, {"NORMAL", "normals"}, {"TEXCOORD_0", "tex_coords"}};
    for (auto& r : req)
      if (!attr || !has(*attr, r[0])) fail(std::string("Read ") + r[1] + " from mesh \"" + name + "\" failed.");  // :246-252
    const Accessor pos = read_accessor(d, index_or_invalid(*attr, "POSITION")), nrm = read_accessor(d, index_or_invalid(*attr, "NORMAL")),
                   uv = read_accessor(d, index_or_invalid(*attr, "TEXCOORD_0"));
    if (pos.ncomp != 3 || nrm.ncomp != 3 || uv.ncomp != 2 || nrm.count != pos.count || uv.count != pos.count) fail("Read positions from mesh \"" + name + "\" failed.");
    std::vector<hala_vertex> v(pos.count);
    for (size_t i = 0; i < pos.count; ++i) {
      for (int c = 0; c < 3; ++c) { v[i].position[c] = (float)pos.v[3 * i + c]; v[i].normal[c] = (float)nrm.v[3 * i + c]; v[i].tangent[c] = 0.0f; }
      v[i].tex_coord[0] = (float)uv.v[2 * i]; v[i].tex_coord[1] = (float)uv.v[2 * i + 1];
    }
    if (has(*attr, "TANGENT")) {  // xyz / w (:255-259)
      const Accessor t4 = read_accessor(d, index_or_invalid(*attr, "TANGENT"));
      if (t4.ncomp != 4 || t4.count != pos.count) fail("Read tangents from mesh \"" + name + "\" failed.");
      for (size_t i = 0; i < pos.count; ++i)
        for (int c = 0; c < 3; ++c) v[i].tangent[c] = (float)t4.v[4 * i + c] / (float)t4.v[4 * i + 3];
    } else {  // per-triangle UV tangent, last writer wins (:260-286); binary32 operations in the reference's order
      for (size_t t = 0; t + 2 < idx.size(); t += 3) {
        const uint32_t i0 = idx[t], i1 = idx[t + 1], i2 = idx[t + 2];
        if (i0 >= v.size() || i1 >= v.size() || i2 >= v.size()) fail("Index out of range in mesh \"" + name + "\".");
        float dp1[3], dp2[3];
        for (int c = 0; c < 3; ++c) { dp1[c] = v[i1].position[c] - v[i0].position[c]; dp2[c] = v[i2].position[c] - v[i0].position[c]; }
        const float du1[2] = {v[i1].tex_coord[0] - v[i0].tex_coord[0], v[i1].tex_coord[1] - v[i0].tex_coord[1]};
        const float du2[2] = {v[i2].tex_coord[0] - v[i0].tex_coord[0], v[i2].tex_coord[1] - v[i0].tex_coord[1]};
        const float a = du1[0] * du2[1], b = du1[1] * du2[0];
        const float invdet = 1.0f / (a - b);
        float tg[3], len2 = 0.0f;
        for (int c = 0; c < 3; ++c) { const float p = dp1[c] * du2[1], q = dp2[c] * du1[1]; tg[c] = (p - q) * invdet; }
        for (int c = 0; c < 3; ++c) { const float sq = tg[c] * tg[c]; len2 = c == 0 ? sq : len2 + sq; }
        const float len = std::sqrt(len2);
        for (int c = 0; c < 3; ++c) { const float n = tg[c] / len; v[i0].tangent[c] = v[i1].tangent[c] = v[i2].tangent[c] = n; }
      }
    }
    s->indices.push_back(std::move(idx));
    s->vertices.push_back(std::move(v));
    hala_primitive_desc pd{};
    pd.indices = s->indices.back().data(); pd.index_count = (uint32_t)s->indices.back().size();
    pd.vertices = s->vertices.back().data(); pd.vertex_count = (uint32_t)s->vertices.back().size();
    pd.material_index = index_or_invalid(p, "material");  // :298
    prims.push_back(pd);
  }
  s->prims.push_back(std::move(prims));
  s->meshes.push_back(hala_mesh_desc{s->prims.back().data(), (uint32_t)s->prims.back().size()});
}

hala_material_desc load_material(const JsonValue& m) {  // :318-385 (+ _MaterialCustomInfo :63-114)
  static const JsonValue none;
  const JsonValue& pbr = get(m, "pbrMetallicRoughness") ? *get(m, "pbrMetallicRoughness") : none;
  const JsonValue& ext = get(m, "extensions") ? *get(m, "extensions") : none;
  hala_material_desc o{};
  const float zero3[3] = {0, 0, 0}, one3[3] = {1, 1, 1}, one4[4] = {1, 1, 1, 1};
  if (const JsonValue* ex = get(m, "extras")) {
    if (!has(*ex, "type")) fail("Parse material extras failed.");  // `type` has no serde default (:65-66)
    o.type = (uint32_t)usize(*ex, "type", 0);
    o.opacity = (float)num(*ex, "opacity", 1.0); o.anisotropic = (float)num(*ex, "anisotropic", 0.0); o.subsurface = (float)num(*ex, "subsurface", 0.0);
    o.specular_tint = (float)num(*ex, "specular_tint", 0.0); o.sheen = (float)num(*ex, "sheen", 0.0); o.sheen_tint = (float)num(*ex, "sheen_tint", 0.0);
    o.clearcoat = (float)num(*ex, "clearcoat", 0.0); o.clearcoat_roughness = (float)num(*ex, "clearcoat_roughness", 0.0);
    floats(*ex, "clearcoat_tint", o.clearcoat_tint, 3, zero3);  // serde default [0,0,0] when extras exist (:83-84)
    o.medium_type = (uint32_t)usize(*ex, "medium_type", 0); floats(*ex, "medium_color", o.medium_color, 3, zero3);
    o.medium_density = (float)num(*ex, "medium_density", 0.0); o.medium_anisotropy = (float)num(*ex, "medium_anisotropy", 0.0);
  } else {  // Default impl (:95-113)
    o.type = 0; o.opacity = 1.0f;
    memcpy(o.clearcoat_tint, one3, 12);
  }
  if (o.type > 1) fail("Invalid material type.");
  float bc[4];
  floats(pbr, "baseColorFactor", bc, 4, one4);
  memcpy(o.base_color, bc, 12);
  floats(m, "emissiveFactor", o.emission, 3, zero3);
  if (const JsonValue* es = get(ext, "KHR_materials_emissive_strength")) {  // :336-338
    const float k = (float)num(*es, "emissiveStrength", 1.0);
    for (float& e : o.emission) e *= k;
  }
  o.metallic = (float)num(pbr, "metallicFactor", 1.0); o.roughness = (float)num(pbr, "roughnessFactor", 1.0);
  const JsonValue* tr = get(ext, "KHR_materials_transmission");
  o.specular_transmission = tr ? (float)num(*tr, "transmissionFactor", 0.0) : 0.0f;
  const JsonValue* ior = get(ext, "KHR_materials_ior");
  o.ior = ior ? (float)num(*ior, "ior", 1.5) : 1.5f;  // :344
  auto tex = [](const JsonValue& o2, const char* key) { const JsonValue* t = get(o2, key); return t ? index_or_invalid(*t, "index") : HALA_INVALID_INDEX; };  // :346-353
  o.base_color_map_index = tex(pbr, "baseColorTexture"); o.emission_map_index = tex(m, "emissiveTexture");
  o.normal_map_index = tex(m, "normalTexture"); o.metallic_roughness_map_index = tex(pbr, "metallicRoughnessTexture");
  return o;
}

hala_light_desc load_light(const JsonValue& l) {  // :434-487
  hala_light_desc o{};
  const float one3[3] = {1, 1, 1};
  floats(l, "color", o.color, 3, one3);
  float intensity = (float)num(l, "intensity", 1.0), p0 = 0.0f, p1 = 0.0f;
  const JsonValue* kind = get(l, "type");
  const std::string k = kind ? kind->str : "";
  uint32_t type;
  if (k == "directional") type = 1;
  else if (k == "point") type = 0;
  else {
    type = 2;
    static const JsonValue none;
    const JsonValue& spot = get(l, "spot") ? *get(l, "spot") : none;
    p0 = (float)num(spot, "innerConeAngle", 0.0); p1 = (float)num(spot, "outerConeAngle", 0.78539816339744830962);
  }
  if (const JsonValue* ex = get(l, "extras")) {  // :449-459
    const double t = num(*ex, "type", 0);  // compared as a number: no cast of an arbitrary double
    if (t == 1) type = 3; else if (t == 2) type = 4;
    p0 = (float)num(*ex, "param0", 0.0); p1 = (float)num(*ex, "param1", 0.0);
  }
  auto clamp90 = [](float x) { return std::min(std::max(x, 0.0f), 90.0f); };
  if (type == 1) p0 = clamp90(p0) * (3.14159265358979323846f / 180.0f);  // f32::to_radians (:461-464)
  else if (type == 2) {  // clamp of radians to [0, 90] is the reference's own quirk (:465-471)
    p0 = clamp90(p0); p1 = clamp90(p1);
    if (p0 > p1) std::swap(p0, p1);
  } else if (type == 3) intensity = intensity / ((0.5f * p0) * p1);  // :472-476
  o.intensity = intensity; o.light_type = type; o.param0 = p0; o.param1 = p1;
  return o;
}

hala_camera_desc load_camera(const JsonValue& c) {  // :492-538
  hala_camera_desc o{};
  const JsonValue* type = get(c, "type");
  if (type && type->str == "orthographic") {
    static const JsonValue none;
    const JsonValue& ob = get(c, "orthographic") ? *get(c, "orthographic") : none;
    o.type = 1; o.xmag = (float)num(ob, "xmag", 1.0); o.ymag = (float)num(ob, "ymag", 1.0);
    o.aspect = 1.0f; o.yfov = 0.7f; o.znear = 0.1f; o.zfar = 1000.0f; o.focal_distance = 10.0f;
    return o;
  }
  static const JsonValue none;
  const JsonValue& p = get(c, "perspective") ? *get(c, "perspective") : none;
  o.type = 0;
  o.aspect = (float)num(p, "aspectRatio", 1.0); o.yfov = (float)num(p, "yfov", 0.7); o.znear = (float)num(p, "znear", 0.1);
  o.zfar = (float)num(p, "zfar", 1000.0);  // :511-514
  const JsonValue* ex = get(c, "extras");
  o.focal_distance = ex ? (float)num(*ex, "focal_dist", 10.0) : 10.0f;  // :38-49, :519-525
  o.aperture = ex ? (float)num(*ex, "aperture", 0.0) : 0.0f;
  return o;  // xmag / ymag stay 0: orthographic only
}

// ---- the rig (docs/RENDER_SPEC.md 19): skins, morph targets and animations, every index a scene index -----------------------------------
[[noreturn]] void rig_fail(const std::string& m) { fail("glTF rig: " + m); }

// the TRS of a node as the file gives it (binary32), or the flag that it came as a matrix
hala_rig_node rig_node_of(const JsonValue& n, const hala_node_desc& nd) {
  hala_rig_node o{};
  o.parent = nd.parent;
  o.is_matrix = has(n, "matrix") ? 1u : 0u;
  memcpy(o.local_transform, nd.local_transform, 64);
  const float zero3[3] = {0, 0, 0}, one3[3] = {1, 1, 1}, unit[4] = {0, 0, 0, 1};
  floats(n, "translation", o.translation, 3, zero3);
  floats(n, "rotation", o.rotation, 4, unit);
  floats(n, "scale", o.scale, 3, one3);
  return o;
}

const float* rig_floats(hala_scene* s, const std::vector<double>& v) {
  s->rig.f32s.emplace_back(v.size());
  for (size_t i = 0; i < v.size(); ++i) s->rig.f32s.back()[i] = (float)v[i];
  return s->rig.f32s.back().data();
}

uint32_t rig_scene_node(const hala_scene* s, const JsonValue& v, const std::string& what) {
  if (v.kind != JsonValue::Number || !(v.num >= 0.0) || v.num != std::floor(v.num) || v.num >= (double)s->rig.node_of_gltf.size() ||
      s->rig.node_of_gltf[(size_t)v.num] == HALA_INVALID_INDEX)
    rig_fail(what + " is out of range.");
  return s->rig.node_of_gltf[(size_t)v.num];
}

// target deltas of one attribute as [target][vertex][3]; a target without the attribute contributes zeros; none has it: no array
const float* rig_target_deltas(const Doc& d, hala_scene* s, const std::vector<JsonValue>& targets, const char* attribute, size_t vertex_count, bool required,
                               const std::string& where) {
  bool any = false;
  for (const JsonValue& t : targets) any = any || has(t, attribute);
  if (!any && !required) return nullptr;
  std::vector<double> all(targets.size() * vertex_count * 3u, 0.0);
  for (size_t k = 0; k < targets.size(); ++k) {
    if (!has(targets[k], attribute)) continue;
    const Accessor a = read_accessor(d, index_or_invalid(targets[k], attribute));
    if (a.ncomp != 3 || a.count != vertex_count) rig_fail("a " + std::string(attribute) + " target of " + where + " does not have one VEC3 per vertex.");
    std::copy(a.v.begin(), a.v.end(), all.begin() + k * vertex_count * 3u);
  }
  return rig_floats(s, all);
}

void load_rig(const Doc& d, hala_scene* s) {
  hala_scene::Rig& rg = s->rig;
  const auto& jnodes = arr(d.j, "nodes");
  const auto& jmeshes = arr(d.j, "meshes");
  const auto& jskins = arr(d.j, "skins");
  const auto& janims = arr(d.j, "animations");
  bool any_targets = false;
  for (const JsonValue& m : jmeshes)
    for (const JsonValue& p : arr(m, "primitives")) any_targets = any_targets || !arr(p, "targets").empty();
  if (jskins.empty() && janims.empty() && !any_targets) { rg = hala_scene::Rig(); return; }  // nothing to pose: every count is 0

  for (const JsonValue& sk : jskins) {
    const auto& joints = arr(sk, "joints");
    rg.u32s.emplace_back();
    for (const JsonValue& j : joints) rg.u32s.back().push_back(rig_scene_node(s, j, "a joint of skin " + std::to_string(rg.skins.size())));
    std::vector<double> ibm;
    if (has(sk, "inverseBindMatrices")) {
      const Accessor a = read_accessor(d, index_or_invalid(sk, "inverseBindMatrices"));
      if (a.ncomp != 16 || a.count != joints.size())
        rig_fail("skin " + std::to_string(rg.skins.size()) + " has " + std::to_string(a.count) + " inverse bind matrices for " + std::to_string(joints.size()) + " joints.");
      ibm = a.v;
    } else {
      ibm.assign(joints.size() * 16u, 0.0);
      for (size_t j = 0; j < joints.size(); ++j) ibm[16 * j] = ibm[16 * j + 5] = ibm[16 * j + 10] = ibm[16 * j + 15] = 1.0;
    }
    hala_rig_skin o{};
    o.joint_count = (uint32_t)joints.size();
    o.joints = rg.u32s.back().data();
    o.inverse_bind_matrices = rig_floats(s, ibm);
    rg.skins.push_back(o);
  }

  // target count of each mesh (its primitives must agree), and the bindings
  std::vector<uint32_t> mesh_targets(jmeshes.size(), 0);
  uint32_t weight_first = 0, palette_first = 0;
  for (uint32_t m = 0; m < jmeshes.size(); ++m) {
    const auto& jprims = arr(jmeshes[m], "primitives");
    for (size_t p = 0; p < jprims.size(); ++p) {
      const uint32_t n = (uint32_t)arr(jprims[p], "targets").size();
      if (p && n != mesh_targets[m]) rig_fail("the primitives of mesh " + std::to_string(m) + " have different target counts.");
      mesh_targets[m] = n;
    }
    uint32_t node = HALA_INVALID_INDEX, node_count = 0;
    for (uint32_t k = 0; k < s->nodes.size(); ++k)
      if (s->nodes[k].mesh_index == m) { if (!node_count) node = k; ++node_count; }
    if (!node_count) continue;  // never drawn
    const uint32_t skin = index_or_invalid(jnodes[rg.gltf_of_node[node]], "skin");
    if (skin != HALA_INVALID_INDEX && skin >= rg.skins.size()) rig_fail("the skin of the node of mesh " + std::to_string(m) + " is out of range.");
    std::vector<double> dflt(mesh_targets[m], 0.0);
    if (has(jmeshes[m], "weights")) {
      const auto& w = arr(jmeshes[m], "weights");
      if (w.size() != mesh_targets[m]) rig_fail("mesh " + std::to_string(m) + " has " + std::to_string(w.size()) + " weights for " + std::to_string(mesh_targets[m]) + " targets.");
      for (size_t k = 0; k < w.size(); ++k) dflt[k] = w[k].num;
    }
    for (uint32_t p = 0; p < jprims.size(); ++p) {
      const std::string where = "mesh " + std::to_string(m) + " primitive " + std::to_string(p);
      const JsonValue* attr = get(jprims[p], "attributes");
      const bool skinned = skin != HALA_INVALID_INDEX && attr && has(*attr, "JOINTS_0") && has(*attr, "WEIGHTS_0");
      if (!skinned && !mesh_targets[m]) continue;
      hala_rig_binding b{};
      b.mesh_index = m; b.primitive_index = p; b.node = node; b.node_count = node_count;
      b.skin = skinned ? skin : HALA_INVALID_INDEX;
      b.vertex_count = s->prims[m][p].vertex_count;
      for (uint32_t k = 0; attr && has(*attr, ("JOINTS_" + std::to_string(k)).c_str()); ++k) b.influence_sets = k + 1u;
      if (skinned) {
        const Accessor ja = read_accessor(d, index_or_invalid(*attr, "JOINTS_0")), wa = read_accessor(d, index_or_invalid(*attr, "WEIGHTS_0"));
        if (ja.ncomp != 4 || ja.count != b.vertex_count) rig_fail("JOINTS_0 of " + where + " does not have one VEC4 per vertex.");
        if (wa.ncomp != 4 || wa.count != b.vertex_count) rig_fail("WEIGHTS_0 of " + where + " does not have one VEC4 per vertex.");
        rg.u16s.emplace_back(ja.v.size());
        for (size_t k = 0; k < ja.v.size(); ++k) {
          if (!(ja.v[k] >= 0.0) || ja.v[k] >= (double)rg.skins[skin].joint_count) rig_fail("a joint index of " + where + " is not below the skin's joint count.");
          rg.u16s.back()[k] = (uint16_t)ja.v[k];
        }
        b.joints = rg.u16s.back().data();
        b.weights = rig_floats(s, wa.v);
        b.palette_first = palette_first;
        palette_first += rg.skins[skin].joint_count * 12u;
      }
      b.target_count = mesh_targets[m];
      if (b.target_count) {
        const auto& targets = arr(jprims[p], "targets");
        b.target_position_deltas = rig_target_deltas(d, s, targets, "POSITION", b.vertex_count, true, where);
        b.target_normal_deltas = rig_target_deltas(d, s, targets, "NORMAL", b.vertex_count, false, where);
        b.target_tangent_deltas = rig_target_deltas(d, s, targets, "TANGENT", b.vertex_count, false, where);
        b.default_weights = rig_floats(s, dflt);
        b.weight_first = weight_first;
        weight_first += b.target_count;
      }
      rg.bindings.push_back(b);
    }
  }

  for (const JsonValue& an : janims) {
    const std::string which = "animation " + std::to_string(rg.clips.size());
    const auto& jsamplers = arr(an, "samplers");
    const auto& jchannels = arr(an, "channels");
    // channels first: a sampler's width is that of the path that reads it
    std::vector<hala_rig_channel> channels;
    std::vector<uint32_t> width(jsamplers.size(), 0);
    for (const JsonValue& ch : jchannels) {
      const JsonValue* target = get(ch, "target");
      if (!target || !has(*target, "node")) continue;  // glTF 2.0 3.11: a channel without a node is ignored
      const JsonValue* path = get(*target, "path");
      static const std::map<std::string, uint32_t> paths = {{"translation", HALA_RIG_TRANSLATION}, {"rotation", HALA_RIG_ROTATION}, {"scale", HALA_RIG_SCALE}, {"weights", HALA_RIG_WEIGHTS}};
      if (!path || !paths.count(path->str)) continue;  // (KHR_animation_pointer and the like: not posed)
      hala_rig_channel o{};
      o.node = rig_scene_node(s, *get(*target, "node"), "the node of a channel of " + which);
      o.path = paths.at(path->str);
      o.sampler = index_or_invalid(ch, "sampler");
      if (o.sampler >= jsamplers.size()) rig_fail("the sampler of a channel of " + which + " is out of range.");
      if (rg.nodes[o.node].is_matrix) rig_fail("a channel of " + which + " targets node " + std::to_string(rg.gltf_of_node[o.node]) + ", which is given as a matrix.");
      uint32_t w = o.path == HALA_RIG_ROTATION ? 4u : 3u;
      if (o.path == HALA_RIG_WEIGHTS) {
        const uint32_t mesh = s->nodes[o.node].mesh_index;
        if (mesh >= mesh_targets.size() || !mesh_targets[mesh]) rig_fail("a weights channel of " + which + " targets a node without a morphed mesh.");
        w = mesh_targets[mesh];
      }
      if (width[o.sampler] && width[o.sampler] != w) rig_fail("a sampler of " + which + " is read by channels of different widths.");
      width[o.sampler] = w;
      channels.push_back(o);
    }
    std::vector<hala_rig_sampler> samplers;
    for (size_t k = 0; k < jsamplers.size(); ++k) {
      const JsonValue& js = jsamplers[k];
      hala_rig_sampler o{};
      const JsonValue* ip = get(js, "interpolation");
      const std::string mode = ip ? ip->str : "LINEAR";
      if (mode == "STEP") o.interpolation = HALA_RIG_STEP;
      else if (mode == "LINEAR") o.interpolation = HALA_RIG_LINEAR;
      else if (mode == "CUBICSPLINE") o.interpolation = HALA_RIG_CUBICSPLINE;
      else rig_fail("a sampler of " + which + " has an unknown interpolation.");
      const Accessor in = read_accessor(d, index_or_invalid(js, "input")), out = read_accessor(d, index_or_invalid(js, "output"));
      if (in.ncomp != 1 || in.count == 0) rig_fail("a sampler of " + which + " has no key times.");
      for (size_t i = 0; i < in.count; ++i)
        if (!std::isfinite(in.v[i]) || (i && !(in.v[i] > in.v[i - 1]))) rig_fail("the key times of a sampler of " + which + " are not finite and strictly increasing.");
      o.key_count = (uint32_t)in.count;
      o.width = width[k] ? width[k] : (uint32_t)out.ncomp;
      const size_t want = in.count * o.width * (o.interpolation == HALA_RIG_CUBICSPLINE ? 3u : 1u);
      if (out.v.size() != want)
        rig_fail("the output of a sampler of " + which + " has " + std::to_string(out.v.size()) + " values for " + std::to_string(in.count) + " keys (" + std::to_string(want) + " expected).");
      for (double v : out.v) if (!std::isfinite(v)) rig_fail("an output of a sampler of " + which + " is not finite.");
      o.times = rig_floats(s, in.v);
      o.values = rig_floats(s, out.v);
      samplers.push_back(o);
    }
    hala_rig_clip c{};
    const JsonValue* nm = get(an, "name");
    rg.names.push_back(nm ? nm->str : "");
    c.name = rg.names.back().c_str();
    bool first = true;
    for (const hala_rig_channel& ch : channels) {
      const hala_rig_sampler& sm = samplers[ch.sampler];
      c.time_first = first ? sm.times[0] : std::min(c.time_first, sm.times[0]);
      c.time_last = first ? sm.times[sm.key_count - 1] : std::max(c.time_last, sm.times[sm.key_count - 1]);
      first = false;
    }
    rg.samplers.push_back(std::move(samplers));
    rg.channels.push_back(std::move(channels));
    c.samplers = rg.samplers.back().data(); c.sampler_count = (uint32_t)rg.samplers.back().size();
    c.channels = rg.channels.back().data(); c.channel_count = (uint32_t)rg.channels.back().size();
    rg.clips.push_back(c);
  }

  hala_rig_desc& o = rg.desc;
  o.node_count = (uint32_t)rg.nodes.size(); o.nodes = rg.nodes.data();
  o.gltf_node_count = (uint32_t)rg.node_of_gltf.size(); o.node_of_gltf = rg.node_of_gltf.data();
  o.skins = rg.skins.data(); o.skin_count = (uint32_t)rg.skins.size();
  o.bindings = rg.bindings.data(); o.binding_count = (uint32_t)rg.bindings.size();
  o.clips = rg.clips.data(); o.clip_count = (uint32_t)rg.clips.size();
  o.weight_floats = weight_first; o.palette_floats = palette_first;
}

void load(const std::string& path, hala_scene* s) {
  Doc d;
  const size_t slash = path.find_last_of("/\\");
  d.dir = slash == std::string::npos ? "" : path.substr(0, slash);
  std::string text;
  try {
    const std::vector<uint8_t> raw = read_file(path);
    text.assign(raw.begin(), raw.end());
  } catch (const LoadError&) { fail("Load glTF file \"" + path + "\" failed."); }  // :123-124
  if (!rt::json_parse(text.c_str(), &d.j).empty()) fail("Load glTF file \"" + path + "\" failed.");
  try {
    for (const JsonValue& b : arr(d.j, "buffers")) {
      const JsonValue* uri = get(b, "uri");
      if (!uri) fail("Buffer without a uri (GLB is not a .gltf).");
      d.buffers.push_back(d.load_uri(uri->str));
    }
  } catch (const LoadError&) { fail("Load glTF file \"" + path + "\" failed."); }
  const auto& scenes = arr(d.j, "scenes");
  if (scenes.empty()) fail("No scene in glTF file \"" + path + "\".");  // :130
  const auto& jnodes = arr(d.j, "nodes");
  // BFS from the scene roots, parents before children (:134-173); the reference walks all scenes into one node list
  s->rig.node_of_gltf.assign(jnodes.size(), HALA_INVALID_INDEX);
  std::vector<uint8_t> visited(jnodes.size(), 0);  // glTF node hierarchies are strict trees (glTF 2.0 §3.5.2): a revisit is a cycle or a shared child
  for (const JsonValue& sc : scenes) {
    std::deque<std::pair<int32_t, uint32_t>> queue;
    for (const JsonValue& r : arr(sc, "nodes")) queue.emplace_back(-1, json_index(r));
    while (!queue.empty()) {
      const auto [parent, idx] = queue.front();
      queue.pop_front();
      if (idx >= jnodes.size()) fail("Node index out of range.");
      if (visited[idx]) fail("The node hierarchy is not a tree (node " + std::to_string(idx) + " is reached twice).");
      visited[idx] = 1;
      const JsonValue& n = jnodes[idx];
      const JsonValue* nm = get(n, "name");
      s->names.push_back(nm ? nm->str : "<Unnamed>");
      hala_node_desc nd{};
      nd.name = s->names.back().c_str(); nd.parent = parent;
      node_matrix(n, nd.local_transform);
      nd.mesh_index = index_or_invalid(n, "mesh"); nd.camera_index = index_or_invalid(n, "camera");
      nd.light_index = HALA_INVALID_INDEX;
      if (const JsonValue* e = get(n, "extensions")) if (const JsonValue* kl = get(*e, "KHR_lights_punctual")) nd.light_index = index_or_invalid(*kl, "light");
      const int32_t cur = (int32_t)s->nodes.size();
      s->nodes.push_back(nd);
      s->rig.node_of_gltf[idx] = (uint32_t)cur; s->rig.gltf_of_node.push_back(idx);
      s->rig.nodes.push_back(rig_node_of(n, nd));
      for (const JsonValue& c : arr(n, "children")) queue.emplace_back(cur, json_index(c));
    }
  }
  for (const JsonValue& m : arr(d.j, "meshes")) load_mesh(d, m, s);
  load_rig(d, s);
  for (const JsonValue& m : arr(d.j, "materials")) s->materials.push_back(load_material(m));
  uint32_t k = 0;
  for (const JsonValue& t : arr(d.j, "textures")) s->tex2img.push_back(hala_index_pair{k++, index_or_invalid(t, "source")});  // :188-192
  const auto& images = arr(d.j, "images");
  for (uint32_t i = 0; i < images.size(); ++i) s->img2data.push_back(hala_index_pair{i, i});  // :193-197
  for (const JsonValue& im : images) {  // :391-429: 8-bit RGB is padded to RGBA with alpha 255 and tagged *_SRGB
    std::vector<uint8_t> raw;
    if (const JsonValue* uri = get(im, "uri")) raw = d.load_uri(uri->str);
    else {
      const auto& views = arr(d.j, "bufferViews");
      const uint32_t bvi = index_or_invalid(im, "bufferView");
      if (bvi >= views.size()) fail("Image without data.");
      const uint32_t bi = index_or_invalid(views[bvi], "buffer");
      const size_t off = usize(views[bvi], "byteOffset", 0), len = usize(views[bvi], "byteLength", 0);
      if (bi >= d.buffers.size() || off + len > d.buffers[bi].size()) fail("Image buffer view out of range.");
      raw.assign(d.buffers[bi].begin() + off, d.buffers[bi].begin() + off + len);
    }
    uint32_t w = 0, h = 0;
    std::vector<uint8_t> px;
    if (!decode_image_rgba8(raw, &w, &h, &px)) fail("Unsupported image format.");
    s->pixels.push_back(std::move(px));
    s->images.push_back(hala_image_desc{HALA_FORMAT_R8G8B8A8_SRGB, w, h, s->pixels.back().data(), s->pixels.back().size()});
  }
  if (const JsonValue* e = get(d.j, "extensions")) if (const JsonValue* kl = get(*e, "KHR_lights_punctual"))
    for (const JsonValue& l : arr(*kl, "lights")) s->lights.push_back(load_light(l));
  for (const JsonValue& c : arr(d.j, "cameras")) s->cameras.push_back(load_camera(c));
  hala_scene_desc& o = s->desc;
  o.nodes = s->nodes.data(); o.node_count = (uint32_t)s->nodes.size();
  o.meshes = s->meshes.data(); o.mesh_count = (uint32_t)s->meshes.size();
  o.materials = s->materials.data(); o.material_count = (uint32_t)s->materials.size();
  o.lights = s->lights.data(); o.light_count = (uint32_t)s->lights.size();
  o.cameras = s->cameras.data(); o.camera_count = (uint32_t)s->cameras.size();
  o.texture2image_mapping = s->tex2img.data(); o.texture_count = (uint32_t)s->tex2img.size();
  o.image2data_mapping = s->img2data.data(); o.image_count = (uint32_t)s->img2data.size();
  o.image_data = s->images.data(); o.image_data_count = (uint32_t)s->images.size();
}

}  // namespace

// 8-bit image file -> RGBA8 for callers outside the glTF loader (cpu::HalaImageData::new_with_file, src/scene/cpu/image_data.rs:26-29: PNG,
// baseline JPEG, PGM / PPM and TGA here); the error text is the reference's.
namespace rt {
std::string decode_image_file_rgba8(const char* path, uint32_t* w, uint32_t* h, std::vector<uint8_t>* rgba) {
  const std::string msg = std::string("Failed to open image \"") + (path ? path : "") + "\".";
  if (!path) return msg;
  FILE* f = fopen(path, "rb");
  if (!f) return msg;
  std::vector<uint8_t> raw;
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) raw.insert(raw.end(), buf, buf + got);
  fclose(f);
  if (!decode_image_rgba8(raw, w, h, rgba)) return msg;
  return "";
}
}  // namespace rt

extern "C" {

int hala_scene_load_gltf(const char* path, hala_scene** out) {
  if (!path || !out) RT_FAIL("Invalid argument.");
  *out = nullptr;
  const std::string p(path);
  const size_t slash = p.find_last_of("/\\"), dot = p.find_last_of('.');
  if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) RT_FAIL("Get file \"" + p + "\" extension failed.");  // scene.rs:43-44
  if (p.substr(dot) != ".gltf") RT_FAIL("Unsupported file \"" + p + "\".");  // :49
  hala_scene* s = new hala_scene();
  try {
    load(p, s);
  } catch (const LoadError& e) {
    delete s;
    RT_FAIL(e.msg);
  } catch (const std::exception& e) {
    delete s;
    RT_FAIL(std::string("Load glTF file \"") + p + "\" failed: " + e.what());
  }
  *out = s;
  return HALA_OK;
}
const hala_scene_desc* hala_scene_get_desc(const hala_scene* s) { return s ? &s->desc : nullptr; }
const hala_rig_desc* hala_scene_get_rig(const hala_scene* s) { return s ? &s->rig.desc : nullptr; }
void hala_scene_free(hala_scene* s) { delete s; }

}  // extern "C"
