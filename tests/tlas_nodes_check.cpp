// tlas_nodes_check.cpp — csrc/bvh_tlas.cpp on its own, for tests/test_bvh_tlas.py to build with the host sanitizers.
// argv[1]: a file of item sets, each { uint32 count; count records of 32 B (rt::TlasItem) }, until the end.
// Per set one line: "<nodes> <levels> <stack_need> |" and the nodes, sixteen 8-digit hex words each.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kernels.h"

int main(int argc, char** argv) {
  static_assert(sizeof(rt::TlasItem) == 32 && sizeof(rt::BvhNode4) == 64, "record sizes");
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t count = 0;
  while (std::fread(&count, 4, 1, f) == 1) {
    std::vector<rt::TlasItem> items(count);
    if (count && std::fread(items.data(), sizeof(rt::TlasItem), count, f) != count) return 3;
    std::vector<rt::BvhNode4> nodes;
    uint32_t levels = 0, need = 0;
    const uint32_t n = rt::tlas_build(items, nodes, &levels, &need);
    if (n != nodes.size()) return 4;
    std::printf("%u %u %u |", n, levels, need);
    for (const rt::BvhNode4& nd : nodes) {
      uint32_t w[16];
      std::memcpy(w, &nd, 64);
      for (uint32_t x : w) std::printf(" %08x", x);
    }
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}
