// bvh_build_impl.h — what bvh_build.hip, its two hierarchy builders (bvh_sah.hip, bvh_ploc.hip) and the builder of the instance levels
// (bvh_instances.hip) share; included by these four only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "bvh_node_pack.h"  // Box6, box_union
#include "kernels.h"
#include "rt_math.h"

namespace rt {

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) return std::string(#expr) + ": " + hipGetErrorString(_e);            \
  } while (0)

// floats as unsigned integers that order like them (scene bounds fold through integer min / max; sort keys)
RT_DI uint32_t f2ord(float f) {
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float ord2f(uint32_t u) {
  u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

RT_DI float half_area(const Box6& b) {
  const float dx = b.mx[0] - b.mn[0], dy = b.mx[1] - b.mn[1], dz = b.mx[2] - b.mn[2];
  return dx * dy + dy * dz + dz * dx;
}
// The slab test's plane distances carry a rounding error of a few ulp of the largest coordinate involved, like the triangle test's
// own; quantisation usually adds far more slack, but a plane that falls exactly on the grid gets none.  Leaf boxes are the triangle
// boxes widened by `pad` (RENDER_SPEC 4.1b: 2^-19 of the scene's largest coordinate): a hit exactly on a box face stays inside its box.
// x -> fl(x -/+ pad) is monotone, so widening a union gives bit for bit the union of the widened boxes: a builder that holds the
// union of a node's triangle boxes writes the node's fitted box without a bottom-up pass.
RT_DI Box6 widen(Box6 b, float pad) {
#pragma unroll
  for (int c = 0; c < 3; ++c) { b.mn[c] -= pad; b.mx[c] += pad; }
  return b;
}

// child reference in the binary tree: bit 31 set = leaf (sorted position), else internal node index
constexpr uint32_t kLeafBit = 0x80000000u;

inline uint32_t nblk(uint32_t n) { return (n + 255u) / 256u; }

// ---- device buffers ----------------------------------------------------------------------------------------------------------------
// A build makes ~60 of them; hipMalloc / hipFree cost 50-200 us each (the free also waits for the device), which was a third of a
// 1 M-triangle commit.  While an Arena is active on this thread, alloc() carves from it instead (256-B aligned bump allocation, released
// all at once with the arena).  An arena is opened with the sum of what its buffers need (carve), so the hipMalloc that alloc() falls
// back to when a buffer does not fit is not expected to run.
struct Arena {
  char* base = nullptr;
  size_t cap = 0, used = 0;
  bool owned = true;
  Arena* prev = nullptr;
  static Arena*& active() { static thread_local Arena* a = nullptr; return a; }
  static size_t aligned(size_t bytes) { return (bytes + 255u) & ~size_t(255); }
  std::string open(size_t bytes) {
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&base), bytes ? bytes : 256));
    cap = bytes;
    prev = active(); active() = this;
    return "";
  }
  // carve from memory that somebody else keeps (the instance levels' arena outlives its builds: a rebuild allocates nothing)
  void adopt(void* memory, size_t bytes) {
    base = static_cast<char*>(memory); cap = bytes; used = 0; owned = false;
    prev = active(); active() = this;
  }
  void close() { if (active() == this) active() = prev; }  // no more carving; the memory lives until the destructor
  void* take(size_t bytes) {
    const size_t at = aligned(used);
    if (!base || at + bytes > cap) return nullptr;
    used = at + bytes;
    return base + at;
  }
  ~Arena() { close(); if (base && owned) (void)hipFree(base); }
};
struct DevBytes {
  void* raw = nullptr;
  size_t bytes = 16;
  bool owned = true;
  DevBytes() = default;
  DevBytes(const DevBytes&) = delete;
  DevBytes& operator=(const DevBytes&) = delete;
  ~DevBytes() { if (raw && owned) (void)hipFree(raw); }
  std::string alloc() {
    if (Arena* a = Arena::active()) {
      if ((raw = a->take(bytes)) != nullptr) { owned = false; return ""; }
    }
    owned = true;
    HIP_TRY(hipMalloc(&raw, bytes));
    return "";
  }
};
// a device array of T: passes as T* wherever a kernel or rocPRIM takes one
template <class T> struct Dev : DevBytes {
  Dev* of(size_t count) { bytes = count * sizeof(T) ? count * sizeof(T) : 16; return this; }  // how many the next alloc() makes
  std::string alloc(size_t count) { of(count); return DevBytes::alloc(); }
  T* get() const { return static_cast<T*>(raw); }
  operator T*() const { return get(); }
};
using DevList = std::vector<DevBytes*>;
inline size_t arena_bytes(const DevList& bufs) {
  size_t total = 0;
  for (const DevBytes* d : bufs) total += Arena::aligned(d->bytes);
  return total;
}
inline std::string alloc_all(const DevList& bufs) {
  for (DevBytes* d : bufs) {
    std::string e = d->alloc();
    if (!e.empty()) return e;
  }
  return "";
}

// exclusive prefix sum of n counters (rocPRIM; storage == nullptr: only the size it needs): one instance of its kernels for all three files
hipError_t exclusive_sum(void* storage, size_t& bytes, const uint32_t* in, uint32_t* out, size_t n, hipStream_t s);

// ---- the binary hierarchy ----------------------------------------------------------------------------------------------------------
// n triangles, n - 1 internal nodes, node 0 = the root; every kernel that reads or writes the tree takes this view by value.
struct BinaryTree {
  uint32_t* __restrict__ left;         // [n - 1] child references (kLeafBit)
  uint32_t* __restrict__ right;
  uint32_t* __restrict__ first;        // [n - 1] the node's triangles are the sorted positions first .. last
  uint32_t* __restrict__ last;
  uint32_t* __restrict__ node_parent;  // [n - 1] kAbsent for the root
  uint32_t* __restrict__ leaf_parent;  // [n] by sorted position
  Box6* node_box;                      // [n - 1] fitted box: the union of the node's leaf boxes
};
// What a hierarchy builder is given and what it leaves (sah_hierarchy, ploc_hierarchy, and k_morton + sort + k_hierarchy in bvh_build.hip).
// In: the triangle boxes by id, n >= 2; the Morton builders (PLOC, LBVH) find sorted_ids in Morton order.  Out, stream synchronised or not:
// a full binary tree down to single triangles in every array of `tree`, node 0 its root, and sorted_ids in an order in which the
// triangles of every node are the contiguous positions first .. last.  SAH and PLOC also fit node_box as they go (widen); the Karras
// hierarchy does not, k_fit follows it.  The tree and its boxes only live until the collapse: what is kept for refit is the 4-wide topology.
struct HierarchyJob {
  uint32_t n;
  float pad;                // widen()
  BuildOptions opt;
  const Box6* tri_box;      // [n] by triangle id
  uint32_t* sorted_ids;     // [n]
  BinaryTree tree;
};
// the scratch a builder needs for n triangles (one list, summed here and allocated there), and the builder
size_t sah_scratch_bytes(uint32_t n);
std::string sah_hierarchy(const HierarchyJob& job, hipStream_t s);
size_t ploc_scratch_bytes(uint32_t n);
std::string ploc_hierarchy(const HierarchyJob& job, hipStream_t s);

// ---- from the hierarchy to the 64-B nodes (bvh_build.hip) -----------------------------------------------------------------------------
constexpr uint32_t kMaxLevels = 96;  // 4-wide levels a tree may have

// What a build keeps for refit: the 4-wide topology and what flatten, the leaf boxes and the level pack read and write.
struct BvhTopology {
  Arena arena;  // first member: destroyed last, after the buffers carved from it
  uint32_t n = 0, leaf_max = 0;
  Dev<uint32_t> first, last, keep;  // per binary node: its sorted positions; 1 = in one slot of a parent it is an inner 4-node, 0 = a leaf (k_collapse_cost)
  Dev<uint4> refs4;                 // per 4-node: the binary references its slots were filled from
  Dev<uint32_t> index4;             // per kept binary node: the 4-node it is the root of
  Dev<uint32_t> sorted_ids;         // triangle id of every sorted position
  Dev<Box6> tri_box, leaf_box;      // by triangle id | by sorted position, widened
  Dev<Box6> box4;                   // k_refit_level's scratch by 4-node; during the build the binary tree's node_box
  Dev<uint32_t> scene_ord, block_ord;
  // null: a leaf's child reference names its sorted positions (triangles).  Otherwise the tree stands over items that bring their own
  // reference (the instance levels, leaf_max = 1): the leaf at sorted position k gets item_ref[sorted_ids[k]]
  const uint32_t* item_ref = nullptr;
  std::vector<uint32_t> level_base;  // first 4-node of every BFS level, then node_count: the level pack walks them bottom-up
  bool single_node() const { return n <= leaf_max || n < 2; }
  DevList plan() {
    const size_t ni = n > 1 ? n - 1 : 1;
    return {first.of(ni), last.of(ni), keep.of(ni), refs4.of(ni), index4.of(ni), sorted_ids.of(n), tri_box.of(n), leaf_box.of(n), box4.of(ni),
            scene_ord.of(6), block_ord.of((size_t)(nblk(n) + 1u) * 6)};
  }
};
// What only the build needs, released when it returns: the binary tree but for first / last, the Morton sort, the collapse's counters.
struct BuildScratch {
  Dev<uint32_t> left, right, node_parent, leaf_parent, arrivals, root_of, cnt, off, level, bases, ids_in;
  Dev<float> cost;       // [3 (n - 1)] k_collapse_cost: C(node, 1..3)
  Dev<uint32_t> choice;  // [n - 1] ... and the cut that gives them
  Dev<unsigned long long> keys_in, keys_out;
  Dev<char> sort_tmp, scan_tmp;  // rocPRIM's
  DevList plan(uint32_t n, bool morton);
};
// Folds ord[6] (min xyz, max xyz as ordered integers) over a 256-thread block: wave shuffle reduction, then the four waves through LDS;
// threads 0..5 leave component threadIdx.x in out[at + threadIdx.x].
RT_DI void block_bounds_fold(uint32_t (&ord)[6], uint32_t (&wave_ord)[4][6], uint32_t tid, uint32_t* __restrict__ out, uint32_t at) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      ord[k] = min(ord[k], (uint32_t)__shfl_xor((int)ord[k], m, 64));
      ord[3 + k] = max(ord[3 + k], (uint32_t)__shfl_xor((int)ord[3 + k], m, 64));
    }
  }
  if ((tid & 63u) == 0u) {
#pragma unroll
    for (int k = 0; k < 6; ++k) wave_ord[tid >> 6][k] = ord[k];
  }
  __syncthreads();
  if (tid < 6u) {
    uint32_t v = wave_ord[0][tid];
    for (int w = 1; w < 4; ++w) v = tid < 3u ? min(v, wave_ord[w][tid]) : max(v, wave_ord[w][tid]);
    out[at + tid] = v;
  }
}
// the steps of bvh_build that a tree over other things than triangles takes as well (bvh_instances.hip); b: tri_count, opt, nodes and the results
void bounds_reduce(const uint32_t* block_ord, uint32_t blocks, uint32_t* scene_ord, hipStream_t s);  // k_bounds_reduce
std::string morton_hierarchy(const HierarchyJob& job, BuildScratch& sc, const uint32_t* scene_ord, bool ploc, hipStream_t s);
std::string fit_hierarchy(const BinaryTree& tree, const Box6* leaf_box, uint32_t* arrivals, uint32_t n, hipStream_t s);  // after the Karras hierarchy only
std::string collapse(BvhBuffers& b, BvhTopology& t, BuildScratch& sc, const BinaryTree& tree, hipStream_t s);
std::string pack_levels(BvhBuffers& b, BvhTopology& t, hipStream_t s);

}  // namespace rt
