// variants.cpp — the variant ledger's state and its reader (variants.h holds the table of families and the dispatch that records).
#include <array>

#include "variants.h"

namespace rt {
std::atomic<uint64_t> g_launched[kVariantFamilies];

// a family's `built` mask, by the enumeration dispatch launches with
template <class... B, size_t... I>
static uint64_t built_mask(bool (*built)(B...), std::index_sequence<I...>) {
  uint64_t mask = 0;
  for (uint32_t i = 0; i < (1u << sizeof...(I)); ++i)
    if (built((((i >> I) & 1u) != 0u)...)) mask |= 1ull << i;
  return mask;
}
template <class... B>
static uint64_t built_mask(bool (*built)(B...)) { return built_mask(built, std::index_sequence_for<B...>{}); }

bool variant_ledger(uint32_t family, uint64_t* launched, uint64_t* built, bool reset) {
  static const auto all = std::apply([](auto... f) { return std::array<uint64_t, kVariantFamilies>{built_mask(f)...}; }, kFamilyBuilt);
  if (family >= kVariantFamilies) return false;
  const uint64_t seen = reset ? g_launched[family].exchange(0, std::memory_order_relaxed) : g_launched[family].load(std::memory_order_relaxed);
  if (launched) *launched = seen;
  if (built) *built = all[family];
  return true;
}

}  // namespace rt
