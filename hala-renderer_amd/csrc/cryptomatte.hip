// cryptomatte.hip — docs/RENDER_SPEC.md 15: Cryptomatte ID mattes.  The depth-0 shade already leaves each sample's first hit in
// ps.aov_ids (RENDER_SPEC 13); k_crypto_fold turns it into one id per enabled layer and folds it into that pixel's 64-B record of
// (id, count) pairs, ranked by count; k_crypto_rank turns the records of one layer and view into the three RGBA32F sublayers of the
// Cryptomatte form on demand.  Both are HBM-bound: adjacent threads own adjacent 64-B records, each moved as four dwordx4 accesses.
// The ordered insert is written with compile-time register indices only (full unrolls, no runtime-indexed array: no scratch).
#include <hip/hip_runtime.h>

#include "cryptomatte.h"
#include "shading.h"

namespace rt {

namespace {

constexpr uint32_t kB = kPixelBlock ? kPixelBlock : 1u;

// the unsharded slot of pixel (px, py) (RENDER_SPEC 9): where its record lives whatever block list an update renders
RT_DI uint32_t crypto_slot(uint32_t px, uint32_t py, uint32_t width, uint32_t blocks_x) {
  if (kPixelBlock == 0u) return py * width + px;
  return ((py / kB) * blocks_x + px / kB) * (kB * kB) + (py % kB) * kB + px % kB;
}

struct Record {
  uint32_t n, other;
  uint32_t id[kCryptoEntries], cnt[kCryptoEntries];
};

RT_DI void load_record(const uint4* __restrict__ p, Record& r) {
  const uint4 a = p[0], b = p[1], c = p[2], d = p[3];
  r.n = a.x; r.other = a.y;
  r.id[0] = a.z; r.cnt[0] = a.w; r.id[1] = b.x; r.cnt[1] = b.y; r.id[2] = b.z; r.cnt[2] = b.w;
  r.id[3] = c.x; r.cnt[3] = c.y; r.id[4] = c.z; r.cnt[4] = c.w; r.id[5] = d.x; r.cnt[5] = d.y; r.id[6] = d.z; r.cnt[6] = d.w;
}
RT_DI void store_record(uint4* __restrict__ p, const Record& r) {
  p[0] = make_uint4(r.n, r.other, r.id[0], r.cnt[0]);
  p[1] = make_uint4(r.id[1], r.cnt[1], r.id[2], r.cnt[2]);
  p[2] = make_uint4(r.id[3], r.cnt[3], r.id[4], r.cnt[4]);
  p[3] = make_uint4(r.id[5], r.cnt[5], r.id[6], r.cnt[6]);
}

// RENDER_SPEC 15 fold of one sample: n += 1; a key that is present counts once more and moves up, a new one takes the last entry if it is
// empty (entries are ordered count descending, id ascending; the empty ones, count 0, are last), else it goes to `other`.  At most one
// entry changed, so one pass from the bottom up restores the order.
RT_DI void fold(Record& r, bool has_key, uint32_t key) {
  r.n += 1u;
  if (!has_key) return;
  bool found = false;
#pragma unroll
  for (uint32_t j = 0; j < kCryptoEntries; ++j) {
    const bool hit = r.cnt[j] != 0u && r.id[j] == key;
    r.cnt[j] += hit ? 1u : 0u;
    found = found || hit;
  }
  if (!found) {
    const bool room = r.cnt[kCryptoEntries - 1] == 0u;
    r.id[kCryptoEntries - 1] = room ? key : r.id[kCryptoEntries - 1];
    r.cnt[kCryptoEntries - 1] = room ? 1u : r.cnt[kCryptoEntries - 1];
    r.other += room ? 0u : 1u;
  }
#pragma unroll
  for (uint32_t j = kCryptoEntries - 1; j > 0; --j) {
    const bool up = r.cnt[j] > r.cnt[j - 1] || (r.cnt[j] == r.cnt[j - 1] && r.id[j] < r.id[j - 1]);
    const uint32_t i0 = r.id[j - 1], c0 = r.cnt[j - 1], i1 = r.id[j], c1 = r.cnt[j];
    r.id[j - 1] = up ? i1 : i0; r.cnt[j - 1] = up ? c1 : c0;
    r.id[j] = up ? i0 : i1; r.cnt[j] = up ? c0 : c1;
  }
}

RT_DI uint32_t table(const uint32_t* __restrict__ t, uint32_t count, uint32_t i, bool* ok) {
  *ok = i < count;
  return *ok ? t[i] : 0u;
}

// Thread t of views x pixel_slots folds pixel slot t % pixel_slots of view t / pixel_slots, like k_resolve: padding slots and the blocks
// adaptive sampling no longer renders are never touched.  A batch that starts an accumulation (frame_index 0) never reads the records.
__global__ void __launch_bounds__(256) k_crypto_fold(FrameConst fc, const uint4* __restrict__ aov_ids, CryptoTables tb, uint4* __restrict__ records) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t view = t / fc.pixel_slots, pslot = t - view * fc.pixel_slots;
  if (view >= fc.views) return;
  uint32_t px, py;
  if (!slot_to_pixel(fc, pslot, &px, &py)) return;
  const size_t at = (size_t)view * tb.slot_count + crypto_slot(px, py, fc.width, fc.blocks_x);
  const size_t layer_stride = (size_t)fc.views * tb.slot_count;
  Record rec[kCryptoLayers];
  uint32_t li = 0;  // enabled layer slot
#pragma unroll
  for (uint32_t l = 0; l < kCryptoLayers; ++l) {
    rec[l] = Record{};
    if (!((tb.mask >> l) & 1u)) continue;
    if (fc.u.frame_index != 0u) load_record(records + 4 * (li * layer_stride + at), rec[l]);
    ++li;
  }
  for (uint32_t k = 0; k < fc.samples; ++k) {  // the batch's samples, in frame order
    const uint4 ids = aov_ids[(size_t)(k * fc.views + view) * fc.pixel_slots + pslot];
    bool ok_o = false, ok_a = false, ok_m = false;
    // RENDER_SPEC 15 keys: object / asset from the node of a triangle's instance or of a light; material from a triangle only
    const uint32_t ko = ids.x != kAbsent ? table(tb.object, tb.node_count, ids.x, &ok_o) : 0u;
    const uint32_t ka = ids.x != kAbsent ? table(tb.asset, tb.node_count, ids.x, &ok_a) : 0u;
    const uint32_t km = ids.z != kAbsent ? table(tb.material, tb.material_count, ids.z, &ok_m) : 0u;
    if (tb.mask & 1u) fold(rec[0], ok_o, ko);
    if (tb.mask & 2u) fold(rec[1], ok_m, km);
    if (tb.mask & 4u) fold(rec[2], ok_a, ka);
  }
  li = 0;
#pragma unroll
  for (uint32_t l = 0; l < kCryptoLayers; ++l) {
    if (!((tb.mask >> l) & 1u)) continue;
    store_record(records + 4 * (li * layer_stride + at), rec[l]);
    ++li;
  }
}

// Ranked output of one layer and view, one thread per pixel (row-major): rank r = (the bits of id_r as a float, count_r / n) with one IEEE
// division, (0, 0) for an empty rank; sublayer k holds ranks 2k and 2k + 1 as R, G, B, A.
__global__ void __launch_bounds__(256) k_crypto_rank(const uint4* __restrict__ records, uint32_t width, uint32_t height, uint32_t blocks_x,
                                                     float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n_px = width * height;
  if (i >= n_px) return;
  const uint32_t py = i / width, px = i - py * width;
  Record r;
  load_record(records + 4 * (size_t)crypto_slot(px, py, width, blocks_x), r);
  float id[kCryptoRanks], cov[kCryptoRanks];
#pragma unroll
  for (uint32_t k = 0; k < kCryptoRanks; ++k) {
    const bool full = r.cnt[k] != 0u;
    id[k] = full ? __uint_as_float(r.id[k]) : 0.0f;
    cov[k] = full ? (float)r.cnt[k] / (float)r.n : 0.0f;
  }
#pragma unroll
  for (uint32_t k = 0; k < kCryptoRanks / 2; ++k) out[(size_t)k * n_px + i] = make_float4(id[2 * k], cov[2 * k], id[2 * k + 1], cov[2 * k + 1]);
}

inline uint32_t blocks_for(uint32_t n, uint32_t per) { return (n + per - 1) / per; }

}  // namespace

void launch_crypto_fold(const FrameConst& fc, const uint4* aov_ids, const CryptoTables& t, uint4* records, hipStream_t s) {
  hipLaunchKernelGGL(k_crypto_fold, dim3(blocks_for(fc.pixel_slots * fc.views, 256)), dim3(256), 0, s, fc, aov_ids, t, records);
}

void launch_crypto_rank(const uint4* records, uint32_t width, uint32_t height, uint32_t blocks_x, float4* out, hipStream_t s) {
  hipLaunchKernelGGL(k_crypto_rank, dim3(blocks_for(width * height, 256)), dim3(256), 0, s, records, width, height, blocks_x, out);
}

}  // namespace rt
