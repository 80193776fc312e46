// deform_adjacency_check.cpp — csrc/deform_adjacency.cpp on its own, for tests/test_deform_normals.py to build with the host sanitizers.
// argv[1]: a file of cases, each { uint32 vertex_count, index_count; vertex_count records of 44 B; index_count uint32 }, until the end.
// Per case one line: "refused", or "<classes> | class_of ... | offsets ... | entries ...".  The buffers are allocated at their exact
// sizes, so a read past either end is the sanitizer's to find.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "deform_adjacency.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[2];
  while (std::fread(head, 4, 2, f) == 2) {
    std::vector<unsigned char> records((size_t)head[0] * 44u);
    std::vector<uint32_t> indices(head[1]);
    if (!records.empty() && std::fread(records.data(), 44, head[0], f) != head[0]) return 3;
    if (!indices.empty() && std::fread(indices.data(), 4, head[1], f) != head[1]) return 3;
    rt::DeformAdjacency adj;
    if (!rt::build_deform_adjacency(records.data(), 44, head[0], indices.data(), indices.size(), &adj)) {
      std::printf("refused\n");
      continue;
    }
    std::printf("%u | ", adj.class_count());
    for (uint32_t c : adj.class_of) std::printf("%u ", c);
    std::printf("| ");
    for (uint32_t o : adj.offsets) std::printf("%u ", o);
    std::printf("| ");
    for (uint32_t t : adj.entries) std::printf("%u ", t);
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}
