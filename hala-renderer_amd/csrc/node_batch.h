// node_batch.h — a bound set of nodes posed from one array of local transforms (docs/RENDER_SPEC.md 20; include/halart.h "Node
// batches"): the tables hala_rt_bind_nodes makes and the launchers of node_batch.hip.  Every index a kernel uses comes from these
// tables, which the host wrote at bind time from the committed scene: nothing is indexed by a value derived from a caller's float.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hala_types.h"

namespace rt {

// one affected node of one depth level: world[node] = parent < 0 ? local[node] : mul(world[parent], local[node])
struct NodeBatchNode { uint32_t node; int32_t parent; };
// one affected instance.  `check`: bit 0 = classify_instances would test its transform (its primitive is referenced at least twice and
// has a triangle, and the instancing rule applies), bit 1 = the instance is intersected in object space as the trees stand.
// `md_slot`: its record in the world tree's own instance table (two-level trees, flattened instances), kAbsent: none
struct NodeBatchInst { uint32_t inst, node, check, md_slot; };

// locals[bound[k]] = in[k], k < count (16 floats each)
void launch_node_locals(const float* in, const uint32_t* bound, uint32_t count, float* locals, uint32_t node_count, hipStream_t s);
// one depth level of the affected nodes, parents before children: launched level by level
void launch_node_worlds(const NodeBatchNode* level, uint32_t n, const float* locals, float* worlds, uint32_t node_count, hipStream_t s);
// the 64-B transform of every affected instance (in `instances`, and in `world_md` where it has a slot there), and the test of
// world_to_object against `check`: a mismatch is ORed into *mismatch (kNodeBatchMismatch).  detect_moved (the refit policy is on,
// RENDER_SPEC 4.6): an instance whose new transform differs bitwise from the one it had ORs kNodeBatchMoved, and kNodeBatchMovedWorldTree
// with it where the instance has a slot in `world_md`
constexpr uint32_t kNodeBatchMismatch = 1u, kNodeBatchMoved = 2u, kNodeBatchMovedWorldTree = 4u;
void launch_instance_transforms(const NodeBatchInst* items, uint32_t n, const float* worlds, uint32_t node_count, hala_gpu_mesh_data* instances,
                                uint32_t instance_count, hala_gpu_mesh_data* world_md, uint32_t world_md_count, uint32_t* mismatch, bool detect_moved,
                                hipStream_t s);

}  // namespace rt
