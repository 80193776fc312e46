// deform_adjacency.h — the tables behind "Recomputed normals" of docs/RENDER_SPEC.md 17: the classes of a primitive's rest vertices and,
// per class, the triangles around it.  Plain C++ (no HIP): rt_deform.hip uploads the result, tests/deform_adjacency_check.cpp runs it alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rt {

struct DeformAdjacency {
  std::vector<uint32_t> class_of;  // [vertex] -> class; classes are numbered by their lowest member, ascending
  std::vector<uint32_t> offsets;   // [class_count + 1]: class c owns entries[offsets[c] .. offsets[c + 1])
  std::vector<uint32_t> entries;   // the triangle of every (triangle, corner) pair of the class, in ascending 3 * triangle + corner
  uint32_t class_count() const { return offsets.empty() ? 0u : (uint32_t)offsets.size() - 1u; }
};

// `records`: vertex_count records `stride` bytes apart whose first 24 bytes are the rest position and the rest normal (hala_vertex).
// Two vertices are one class when those 24 bytes are equal as bit patterns (-0.0 is not +0.0; equal NaN patterns are equal).
// `indices`: index_count / 3 triangles; a trailing partial triangle is ignored.  Deterministic, O(V log V + T).
// -> false, `out` cleared: an index is not below vertex_count, or the counts do not fit 32 bits.
bool build_deform_adjacency(const void* records, size_t stride, size_t vertex_count, const uint32_t* indices, size_t index_count, DeformAdjacency* out);

}  // namespace rt
