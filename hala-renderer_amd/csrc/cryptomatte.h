// cryptomatte.h — Cryptomatte ID mattes of docs/RENDER_SPEC.md 15: the per-pixel id -> coverage records, their device tables and the
// host side of the two kernels of cryptomatte.hip.  The name hashing and the EXR writer are host code (host_util.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "hala_types.h"

namespace rt {

constexpr uint32_t kCryptoLayers = 3;   // bit 0 object, bit 1 material, bit 2 asset
constexpr uint32_t kCryptoEntries = 7;  // (id, count) pairs of a record: [n, other, (id, count) x 7] = 16 words = 64 B
constexpr uint32_t kCryptoRanks = 6;    // ranks of the ranked output: 3 RGBA sublayers of two (id, coverage) pairs

// what k_crypto_fold reads: the stored id of every node's object name and of its root's (asset), of every material; the enabled layers
// and where the records are.  Record of enabled layer slot i (the rank of its bit among the enabled ones), view v, unsharded pixel slot p
// (RENDER_SPEC 9, whatever adaptive sampling has compacted) at records + 4 * ((i * views + v) * slot_count + p): four 16-B quads.
struct CryptoTables {
  const uint32_t* object;    // per node
  const uint32_t* asset;     // per node
  const uint32_t* material;  // per material
  uint32_t node_count, material_count;
  uint32_t mask;             // enabled layers
  uint32_t slot_count;       // pixel slots of one view (unsharded; padding slots of border blocks included)
};

// MurmurHash3_x86_32 of the bytes; RENDER_SPEC 15 uses seed 0 only
uint32_t murmur3_32(const void* data, size_t len, uint32_t seed);
// the stored id: the raw hash with bit 23 flipped when its exponent bits are 0 or 255 (the float32 it reads as is finite and normal)
inline uint32_t crypto_id(uint32_t raw) {
  const uint32_t e = (raw >> 23) & 0xFFu;
  return (e == 0u || e == 255u) ? raw ^ (1u << 23) : raw;
}
// a JSON string literal (quotes included) of UTF-8 bytes: '"', '\\' and the control characters escaped, everything else as it is
std::string json_quote(const std::string& s);
// single-part scanline OpenEXR 2.0, ZIP compression (16 lines per block), FLOAT channels sorted by name, string attributes; "" on success
std::string write_exr(const char* path, uint32_t width, uint32_t height, uint32_t channel_count, const char* const* names,
                      const float* const* planes, uint32_t attribute_count, const char* const* attr_names, const char* const* attr_values);

// fold the batch's first-hit records (ps.aov_ids) into the records: one thread per (view, pixel slot) of the update, like k_resolve
void launch_crypto_fold(const FrameConst& fc, const uint4* aov_ids, const CryptoTables& t, uint4* records, hipStream_t s);
// one layer and view: records (already at that layer's and view's first record) -> 3 row-major RGBA32F images, image k at out + k * W * H
void launch_crypto_rank(const uint4* records, uint32_t width, uint32_t height, uint32_t blocks_x, float4* out, hipStream_t s);

}  // namespace rt
