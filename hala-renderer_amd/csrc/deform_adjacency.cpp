// deform_adjacency.cpp — see deform_adjacency.h.  A sort of the vertex numbers by (key bytes, number) finds the classes; a counting sort
// of the 3 T corners by class, stable in the corner number, lays out the lists.
#include "deform_adjacency.h"

#include <algorithm>
#include <cstring>
#include <numeric>

namespace rt {

namespace {
constexpr size_t kKeyBytes = 24;  // position and normal, 3 floats each
}

bool build_deform_adjacency(const void* records, size_t stride, size_t vertex_count, const uint32_t* indices, size_t index_count, DeformAdjacency* out) {
  out->class_of.clear(); out->offsets.clear(); out->entries.clear();
  const size_t corners = index_count - index_count % 3u;
  if (vertex_count > 0xffffffffull || corners > 0xffffffffull) return false;
  for (size_t k = 0; k < corners; ++k)
    if (indices[k] >= vertex_count) return false;
  const unsigned char* base = static_cast<const unsigned char*>(records);
  auto key = [&](uint32_t v) { return base + (size_t)v * stride; };

  std::vector<uint32_t> order(vertex_count);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const int c = std::memcmp(key(a), key(b), kKeyBytes);
    return c != 0 ? c < 0 : a < b;
  });
  // the lowest member of every run of equal keys stands for the class
  std::vector<uint32_t> lowest(vertex_count);
  for (size_t k = 0; k < vertex_count;) {
    size_t e = k + 1;
    while (e < vertex_count && std::memcmp(key(order[k]), key(order[e]), kKeyBytes) == 0) ++e;
    for (size_t m = k; m < e; ++m) lowest[order[m]] = order[k];
    k = e;
  }
  out->class_of.resize(vertex_count);
  uint32_t classes = 0;
  for (size_t v = 0; v < vertex_count; ++v)  // (lowest[v] <= v, so its class is numbered already)
    out->class_of[v] = lowest[v] == v ? classes++ : out->class_of[lowest[v]];

  out->offsets.assign((size_t)classes + 1u, 0u);
  for (size_t k = 0; k < corners; ++k) ++out->offsets[(size_t)out->class_of[indices[k]] + 1u];
  for (size_t c = 0; c < classes; ++c) out->offsets[c + 1] += out->offsets[c];
  out->entries.resize(corners);
  std::vector<uint32_t> at(out->offsets.begin(), out->offsets.end() - 1);
  for (size_t k = 0; k < corners; ++k) out->entries[at[out->class_of[indices[k]]]++] = (uint32_t)(k / 3u);
  return true;
}

}  // namespace rt
