// Stand-alone driver of the host plan of "schur_jacobi" (csrc/jac_schur_jacobi.cpp), for runs
// under -fsanitize=address,undefined on a machine without a GPU (tests/test_schur_jacobi_cpu.py builds and runs it):
//   g++ -std=c++17 -g -fsanitize=address,undefined -static-libasan -static-libubsan -I baspacho_amd/csrc \
//       tools/schur_jacobi_plan_check.cpp \
//       baspacho_amd/csrc/jac_schur_jacobi.cpp -o schur_jacobi_plan_check
// It reads the lists of a JacSchurMap that the plan is built from as whitespace-separated integers on standard input
// -- m, numElim, then twelve arrays, each as its length and its elements: elimOff, keptParam, keptFirst, keptWidth,
// keptBlockStart, keptScalarBlock, rowsKept (start, entry, idx), rowsElim (start, entry, idx) -- and prints every
// table of the plan as a line "name length elements...".
#include <cstdio>
#include <iostream>
#include <vector>

#include "jac_schur.h"

namespace BaSpaCho {
void hipBackendFreeEntryMap(HipEntryMapDev*) {}  // (no device copy exists here)
}  // namespace BaSpaCho

template <typename V>
static void print(const char* name, const V& v) {
  std::printf("%s %zu", name, v.size());
  for (auto x : v) std::printf(" %lld", (long long)x);
  std::printf("\n");
}

int main() {
  using namespace BaSpaCho;
  JacSchurMap map;
  if (!(std::cin >> map.m >> map.numElim)) return 2;
  const auto read = [](std::vector<int32_t>& v) {
    size_t len = 0;
    if (!(std::cin >> len)) return false;
    v.resize(len);
    for (int32_t& x : v) {
      if (!(std::cin >> x)) return false;
    }
    return true;
  };
  for (std::vector<int32_t>* v : {&map.elimOff, &map.keptParam, &map.keptFirst, &map.keptWidth, &map.keptBlockStart,
                                  &map.keptScalarBlock, &map.rowsKept.start, &map.rowsKept.entry, &map.rowsKept.idx,
                                  &map.rowsElim.start, &map.rowsElim.entry, &map.rowsElim.idx}) {
    if (!read(*v)) return 2;
  }
  try {
    const JacSchurJacobiPlan& p = jacSchurJacobiPlan(map);
    print("block_pair", p.blockPair);
    print("block_chunk", p.blockChunk);
    print("block_off", p.blockOff);
    print("chunk_pair", p.chunkPair);
    print("chunk_block", p.chunkBlock);
    print("chunk_part", p.chunkPart);
    print("pair_elim", p.pairElim);
    print("pair_row", p.pairRow);
    print("pair_rec", p.pairRec);
    print("row_of", p.rowOf);
    print("rec", p.rec);
  } catch (const std::exception& e) {
    std::printf("refused: %s\n", e.what());
  }
  return 0;
}
