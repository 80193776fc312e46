// variants.h — how launch-time flags become kernel template arguments, for the launchers of the six flag-dispatched kernel families
// (trace_closest.hip, trace_shadow.hip, shade.hip, resolve.hip), and what the variant ledger (variants.cpp) records of it.  Host code only.
#pragma once
#include <algorithm>
#include <atomic>
#include <tuple>
#include <type_traits>

#include "kernels.h"

namespace rt {
static inline uint32_t blocks_for(uint32_t n, uint32_t per) { return (n + per - 1) / per; }

// The one place where launch-time flags become kernel template arguments: calls f with one std::integral_constant<bool, flag> argument
// per runtime flag, in order.
template <class F>
static void with_flags(F&& f) { f(); }
template <class F, class... Flags>
static void with_flags(F&& f, bool flag, Flags... flags) {
  if (flag) with_flags([&](auto... c) { f(std::true_type{}, c...); }, flags...);
  else with_flags([&](auto... c) { f(std::false_type{}, c...); }, flags...);
}

// Resident workgroups per CU (occupancy query; 0 on an error) of the traversal kernel that kernel_of(STAGED, INST) names for this tree
// form.  traverse_blocks_per_cu (trace_closest.hip) is the smaller of its own unit's answer and trace_shadow.hip's.
template <class F>
static uint32_t tree_blocks_per_cu(F&& kernel_of, TreeForm tree, int threads, size_t dynamic_lds_bytes) {
  int n = 0;
  hipError_t e = hipSuccess;
  with_flags([&](auto STAGED, auto INST) {
    if constexpr (!(STAGED && INST)) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel_of(STAGED, INST), threads, dynamic_lds_bytes);
  }, tree == TreeForm::Staged, tree == TreeForm::TwoLevel);
  return e == hipSuccess && n > 0 ? (uint32_t)n : 0u;
}
uint32_t trace_shadow_blocks_per_cu(size_t dynamic_lds_bytes, TreeForm tree);

// The launch shape of the query kernels that size themselves (trace_multi.hip, closest_point.hip, distance_grid.hip), unlike the ones that
// run in lc's grid and LDS.  Their LDS: the per-lane stacks, and a staged tree behind them
static size_t query_lds_bytes(const SceneView& sv, TreeForm tree, int threads) {
  const size_t stacks = (size_t)traverse_stack_lds_levels(tree) * threads * 8;
  return tree == TreeForm::Staged ? stacks + (size_t)sv.lds_nodes * 64 + (size_t)sv.lds_tris * 48 : stacks;
}
// Their grid: what is resident, within lc.persistent_blocks — the spill area holds one slice per lane of that many workgroups
static uint32_t query_blocks(const LaunchCfg& lc, uint32_t cu_count, uint32_t per_cu) { return std::min(lc.persistent_blocks, cu_count * std::min(per_cu, 8u)); }
// Their occupancy where counting is a template argument: that of kernel_of(STAGED, COUNT), the instantiation the launch will run
template <class F>
static uint32_t counted_blocks_per_cu(F&& kernel_of, bool count, TreeForm tree, int threads, size_t dynamic_lds_bytes) {
  return count ? tree_blocks_per_cu([&](auto STAGED, auto) { return kernel_of(STAGED, std::true_type{}); }, tree, threads, dynamic_lds_bytes)
               : tree_blocks_per_cu([&](auto STAGED, auto) { return kernel_of(STAGED, std::false_type{}); }, tree, threads, dynamic_lds_bytes);
}

// ---------------------------------------------------------------------------------------------------------
// The variant ledger (hala_rt_variant_ledger): which instantiations of the six flag-dispatched kernel families exist and which of them
// this process has launched.  Host bookkeeping only.  One predicate per family says which flag combinations a kernel is built for, in the
// launcher's dispatch order (no kernel is both STAGED and INST, ALPHA only exists for any-hit rays, SIMPLE shading has no SCATTER variant);
// dispatch's `if constexpr` and the family's `built` mask both come from it.  Bit index of a combination: its flags read as a binary
// number, first flag least significant.
// ---------------------------------------------------------------------------------------------------------
constexpr bool trace_primary_built(bool /*COUNT*/, bool STAGED, bool INST, bool /*VIEWS*/, bool /*FAR*/) { return !(STAGED && INST); }
constexpr bool trace_batch_built(bool ANY, bool /*COUNT*/, bool ALPHA, bool STAGED, bool INST) { return (ANY || !ALPHA) && !(STAGED && INST); }
constexpr bool trace_shadow_built(bool /*COUNT*/, bool /*ALPHA*/, bool STAGED, bool INST, bool /*GROUPS*/) { return !(STAGED && INST); }
constexpr bool trace_shadow_then_batch_built(bool /*ALPHA*/, bool STAGED, bool INST, bool /*GROUPS*/) { return !(STAGED && INST); }
constexpr bool shade_built(bool PRIMARY, bool SIMPLE, bool SCATTER, bool AOV, bool /*GROUPS*/) { return !(SIMPLE && SCATTER) && (PRIMARY || !AOV); }
constexpr bool resolve_built(bool /*AOV*/, bool /*GROUPS*/) { return true; }
// the table of families, in the order of kFamily*: a family's flag count is its predicate's parameter count
constexpr auto kFamilyBuilt = std::make_tuple(trace_primary_built, trace_batch_built, trace_shadow_built, trace_shadow_then_batch_built, shade_built, resolve_built);
static_assert(std::tuple_size_v<decltype(kFamilyBuilt)> == kVariantFamilies, "one predicate per kernel family");

extern std::atomic<uint64_t> g_launched[kVariantFamilies];  // variants.cpp

// A launch of family FAMILY with these runtime flags: calls launch(constants...) — one std::integral_constant<bool, flag> per flag, in
// order — if the family has a kernel for the combination, and records the combination in the ledger; else does nothing.
template <uint32_t FAMILY, class F, class... Flags>
static void dispatch(F&& launch, Flags... flags) {
  with_flags([&](auto... c) {
    if constexpr (std::get<FAMILY>(kFamilyBuilt)(c...)) {
      uint64_t index = 0, bit = 1;
      ((index |= c ? bit : 0, bit <<= 1), ...);
      g_launched[FAMILY].fetch_or(1ull << index, std::memory_order_relaxed);
      launch(c...);
    }
  }, flags...);
}

}  // namespace rt
