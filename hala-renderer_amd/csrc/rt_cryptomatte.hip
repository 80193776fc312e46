// rt_cryptomatte.hip — Cryptomatte (RENDER_SPEC 15) on the host: names, id tables and records (CryptoState), the read-backs, the
// manifest and the EXR.  The kernels are in cryptomatte.hip.
#include "renderer_state.h"

namespace rt {

static std::string crypto_object_name(const HostScene& hs, uint32_t k) {
  return hs.nodes[k].name.empty() ? "node" + std::to_string(k) : hs.nodes[k].name;
}
static uint32_t crypto_root(const HostScene& hs, uint32_t k) {  // parents precede children (HostScene::assign), so this ends
  while (hs.nodes[k].parent >= 0) k = (uint32_t)hs.nodes[k].parent;
  return k;
}
static std::string crypto_material_name(const hala_rt_renderer* r, uint32_t m) {
  return m < r->crypto.material_names.size() && !r->crypto.material_names[m].empty() ? r->crypto.material_names[m] : "material" + std::to_string(m);
}
static uint32_t crypto_name_id(const std::string& s) { return crypto_id(murmur3_32(s.data(), s.size(), 0u)); }
// the unsharded slot of pixel (x, y) (RENDER_SPEC 9): where its record lives (cryptomatte.hip: crypto_slot)
static size_t crypto_host_slot(const hala_rt_renderer* r, uint32_t x, uint32_t y) {
  if (kPixelBlock == 0u) return (size_t)y * r->width + x;
  return ((size_t)(y / kPixelBlock) * r->blocks_x + x / kPixelBlock) * kPixelBlock * kPixelBlock + (y % kPixelBlock) * kPixelBlock + x % kPixelBlock;
}
// the first record of enabled layer `layer` and view `view`
static const uint4* crypto_records_of(const hala_rt_renderer* r, uint32_t view, uint32_t layer) {
  const uint32_t slot = (uint32_t)__builtin_popcount(r->crypto.mask & ((1u << layer) - 1u));
  return r->crypto.rec.ptr + 4 * (((size_t)slot * r->view_count() + view) * r->slot_count);
}
// every name the committed scene can produce in `layer`, with its id, in ascending byte order
static std::map<std::string, uint32_t> crypto_names(const hala_rt_renderer* r, uint32_t layer) {
  const HostScene& hs = r->hs;
  std::map<std::string, uint32_t> out;
  if (layer == 1u) {
    for (uint32_t m = 0; m < hs.gpu_materials.size(); ++m) { const std::string n = crypto_material_name(r, m); out[n] = crypto_name_id(n); }
    return out;
  }
  std::vector<uint32_t> nodes(hs.instance_node);
  nodes.insert(nodes.end(), hs.light_node.begin(), hs.light_node.end());
  for (uint32_t k : nodes) {
    const std::string n = crypto_object_name(hs, layer == 2u ? crypto_root(hs, k) : k);
    out[n] = crypto_name_id(n);
  }
  return out;
}
// before an update's device work: the id tables of the committed scene (first update after commit, refit or hala_rt_set_cryptomatte) and
// records sized for the current views (hala_rt_set_views may have changed them); nothing in flight may still read the old ones
int crypto_prepare(hala_rt_renderer* r) {
  if (!(r->slots.slot[0].set.shape == r->path_shape()))  // (a fit that failed)
    RT_FAIL("hala_rt_update: the first-hit records Cryptomatte folds are not allocated (call hala_rt_set_cryptomatte again).");
  const size_t quads = r->crypto.quads(r->view_count(), r->slot_count);
  if (r->crypto.tables && r->crypto.rec.count == quads) return HALA_OK;
  if (r->slots.join(r->stream) != HALA_OK) return HALA_ERR;
  RT_HIP(hipStreamSynchronize(r->stream));
  if (!r->crypto.tables) {
    const HostScene& hs = r->hs;
    const uint32_t nn = (uint32_t)hs.nodes.size(), nm = (uint32_t)hs.gpu_materials.size();
    r->crypto.object.resize(nn); r->crypto.asset.resize(nn); r->crypto.material.resize(nm);
    for (uint32_t k = 0; k < nn; ++k) r->crypto.object[k] = crypto_name_id(crypto_object_name(hs, k));
    for (uint32_t k = 0; k < nn; ++k) r->crypto.asset[k] = r->crypto.object[crypto_root(hs, k)];
    for (uint32_t m = 0; m < nm; ++m) r->crypto.material[m] = crypto_name_id(crypto_material_name(r, m));
    RT_HIP(r->crypto.d_object.upload(r->crypto.object.data(), nn, r->stream));
    RT_HIP(r->crypto.d_asset.upload(r->crypto.asset.data(), nn, r->stream));
    RT_HIP(r->crypto.d_material.upload(r->crypto.material.data(), nm, r->stream));
    r->crypto.tables = true;
  }
  if (r->crypto.rec.count != quads) {
    RT_HIP(r->crypto.rec.resize(quads));
    RT_HIP(hipMemsetAsync(r->crypto.rec.ptr, 0, r->crypto.rec.bytes(), r->stream));
  }
  RT_HIP(hipStreamSynchronize(r->stream));
  return HALA_OK;
}

}  // namespace rt

extern "C" {

static const char* const kCryptoLayerNames[kCryptoLayers] = {"CryptoObject", "CryptoMaterial", "CryptoAsset"};

static std::string cryptomatte_check(const hala_cryptomatte_desc* d) {
  if (d->layer_mask == 0u || d->layer_mask > 7u)
    return "hala_rt_set_cryptomatte: layer_mask must be in 1..7 (bit 0 object, bit 1 material, bit 2 asset).";
  if (d->material_name_count && !d->material_names) return "hala_rt_set_cryptomatte: the material name table is null but its count is not 0.";
  if (d->reserved[0] || d->reserved[1]) return "hala_rt_set_cryptomatte: the reserved fields must be 0.";
  return "";
}
int hala_rt_set_cryptomatte(hala_rt_renderer* r, const hala_cryptomatte_desc* d) {
  if (d) {
    const std::string bad = cryptomatte_check(d);  // first: the CPU tier pins it without a renderer
    if (!bad.empty()) RT_FAIL(bad);
  }
  if (!r) RT_FAIL("The renderer handle is null!");
  if (d && r->world > 1) RT_FAIL("hala_rt_set_cryptomatte: Cryptomatte is not available on a sharded renderer (world > 1).");
  std::vector<std::string> names(d ? d->material_name_count : 0u);
  for (size_t m = 0; m < names.size(); ++m) names[m] = d->material_names[m] ? d->material_names[m] : "";
  if (ensure_device(r) != HALA_OK) return HALA_ERR;  // joins the second frame slot
  RT_HIP(hipStreamSynchronize(r->stream));
  r->crypto.off();
  if (d) r->crypto.mask = d->layer_mask;
  hipError_t e = r->fit_paths();  // the first-hit records of every path slot; off: freed unless image 5 wants them
  if (d) {
    if (e == hipSuccess) e = r->crypto.rec.resize(r->crypto.quads(r->view_count(), r->slot_count));
    if (e == hipSuccess) e = hipMemsetAsync(r->crypto.rec.ptr, 0, r->crypto.rec.bytes(), r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    if (e != hipSuccess) { r->crypto.off(); (void)r->fit_paths(); RT_HIP(e); }  // out of memory: the feature is off, everything else untouched
    r->crypto.material_names = std::move(names);
  }
  r->reset_accumulation();
  return HALA_OK;
}
static int crypto_layer_check(hala_rt_renderer* r, uint32_t layer) {
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!r->crypto.mask) RT_FAIL("Cryptomatte is off (hala_rt_set_cryptomatte).");
  if (layer >= kCryptoLayers || !((r->crypto.mask >> layer) & 1u))
    RT_FAIL("The Cryptomatte layer is off (hala_rt_set_cryptomatte enabled layer mask " + std::to_string(r->crypto.mask) + ").");
  return HALA_OK;
}
static int crypto_read_check(hala_rt_renderer* r, uint32_t view, uint32_t layer) {
  if (crypto_layer_check(r, layer) != HALA_OK) return HALA_ERR;
  if (view >= r->view_count()) RT_FAIL("The view does not exist (hala_rt_set_views set " + std::to_string(r->view_count()) + ").");
  if (!r->crypto.ready) RT_FAIL("No Cryptomatte samples since the accumulation restarted: update first.");
  return HALA_OK;
}
int hala_rt_read_cryptomatte(hala_rt_renderer* r, uint32_t view, uint32_t layer, float* dst) {
  if (crypto_read_check(r, view, layer) != HALA_OK) return HALA_ERR;
  if (!dst) RT_FAIL("The output pointer is null!");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  const size_t px = (size_t)r->width * r->height;
  DeviceArray<float4> out;
  RT_HIP(out.resize(3 * px));
  launch_crypto_rank(crypto_records_of(r, view, layer), r->width, r->height, r->blocks_x, out.ptr, r->stream);
  RT_HIP(hipGetLastError());
  RT_HIP(hipStreamSynchronize(r->stream));
  RT_HIP(hipMemcpy(dst, out.ptr, out.bytes(), hipMemcpyDeviceToHost));
  return HALA_OK;
}
int hala_rt_read_cryptomatte_records(hala_rt_renderer* r, uint32_t view, uint32_t layer, uint32_t* dst) {
  if (crypto_read_check(r, view, layer) != HALA_OK) return HALA_ERR;
  if (!dst) RT_FAIL("The output pointer is null!");
  if (ensure_device(r) != HALA_OK) return HALA_ERR;
  RT_HIP(hipStreamSynchronize(r->stream));
  std::vector<uint4> rec((size_t)r->slot_count * 4);
  RT_HIP(hipMemcpy(rec.data(), crypto_records_of(r, view, layer), rec.size() * sizeof(uint4), hipMemcpyDeviceToHost));
  for (uint32_t y = 0; y < r->height; ++y)
    for (uint32_t x = 0; x < r->width; ++x) memcpy(dst + 16 * ((size_t)y * r->width + x), &rec[4 * crypto_host_slot(r, x, y)], 64);
  return HALA_OK;
}
static std::string crypto_manifest(const hala_rt_renderer* r, uint32_t layer) {
  std::string j = "{";
  for (const auto& kv : crypto_names(r, layer)) {
    char hex[16];
    snprintf(hex, sizeof(hex), "\"%08x\"", kv.second);
    if (j.size() > 1) j += ",";
    j += json_quote(kv.first) + ":" + hex;
  }
  return j + "}";
}
int hala_rt_get_cryptomatte_manifest(hala_rt_renderer* r, uint32_t layer, char* dst, size_t capacity, size_t* length) {
  if (crypto_layer_check(r, layer) != HALA_OK) return HALA_ERR;
  if (!length) RT_FAIL("The output pointer is null!");
  const std::string j = crypto_manifest(r, layer);
  *length = j.size();
  if (dst) {
    if (capacity < j.size() + 1) RT_FAIL("The destination buffer is too small (" + std::to_string(j.size() + 1) + " bytes needed).");
    memcpy(dst, j.c_str(), j.size() + 1);
  }
  return HALA_OK;
}
int hala_rt_save_cryptomatte(hala_rt_renderer* r, uint32_t view, const char* path) {
  RtRange range("halart::save_cryptomatte");
  if (!r) RT_FAIL("The renderer handle is null!");
  if (!r->crypto.mask) RT_FAIL("Cryptomatte is off (hala_rt_set_cryptomatte).");
  if (crypto_read_check(r, view, (uint32_t)__builtin_ctz(r->crypto.mask)) != HALA_OK) return HALA_ERR;
  if (!path || !*path) RT_FAIL("The file name is none!");
  const size_t px = (size_t)r->width * r->height;
  std::vector<float> accum(4 * px);
  if (hala_rt_read_view_image(r, view, 0, accum.data()) != HALA_OK) return HALA_ERR;
  std::vector<std::vector<float>> planes;
  std::vector<std::string> names, attr_names, attr_values;
  for (int c = 0; c < 4; ++c) {
    names.push_back(std::string(1, "RGBA"[c]));
    planes.emplace_back(px);
    for (size_t i = 0; i < px; ++i) planes.back()[i] = accum[4 * i + c];
  }
  std::vector<float> ranked(12 * px);
  for (uint32_t l = 0; l < kCryptoLayers; ++l) {
    if (!((r->crypto.mask >> l) & 1u)) continue;
    if (hala_rt_read_cryptomatte(r, view, l, ranked.data()) != HALA_OK) return HALA_ERR;
    const std::string layer = kCryptoLayerNames[l];
    for (int k = 0; k < 3; ++k)
      for (int c = 0; c < 4; ++c) {
        names.push_back(layer + "0" + std::to_string(k) + "." + "RGBA"[c]);
        planes.emplace_back(px);
        for (size_t i = 0; i < px; ++i) planes.back()[i] = ranked[4 * ((size_t)k * px + i) + c];
      }
    char key[16];
    snprintf(key, sizeof(key), "%08x", murmur3_32(layer.data(), layer.size(), 0u));
    const std::string base = "cryptomatte/" + std::string(key, 7) + "/";
    attr_names.push_back(base + "name"); attr_values.push_back(layer);
    attr_names.push_back(base + "hash"); attr_values.push_back("MurmurHash3_32");
    attr_names.push_back(base + "conversion"); attr_values.push_back("uint32_to_float32");
    attr_names.push_back(base + "manifest"); attr_values.push_back(crypto_manifest(r, l));
  }
  std::vector<const char*> np, an, av;
  std::vector<const float*> pp;
  for (size_t c = 0; c < names.size(); ++c) { np.push_back(names[c].c_str()); pp.push_back(planes[c].data()); }
  for (size_t a = 0; a < attr_names.size(); ++a) { an.push_back(attr_names[a].c_str()); av.push_back(attr_values[a].c_str()); }
  const std::string e = write_exr(path, r->width, r->height, (uint32_t)np.size(), np.data(), pp.data(), (uint32_t)an.size(), an.data(), av.data());
  if (!e.empty()) RT_FAIL(e);
  return HALA_OK;
}

}  // extern "C"
