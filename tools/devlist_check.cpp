// DevList (csrc/physics.h) on the emulation allocator: create / release, a create whose third allocation fails, a double release.
//   g++ -std=c++17 -DFV3LM_HOST_EMUL -fsanitize=address,undefined -I fv3_jedi_linearmodel_amd/csrc -o devlist_check tools/devlist_check.cpp
//   ASAN_OPTIONS=allocator_may_return_null=1 ./devlist_check      (the refused calloc returns null instead of aborting)
#include "physics.h"
#include <cstdio>
using namespace fv3;
int main() {
  DevList m;
  double* a = m.get<double>(1024); int* b = m.get<int>(8); double* c = m.get<double>(4096);
  if (!a || !b || !c || !m.ok() || m.empty()) return 1;
  a[127] = 1.; b[1] = 2; c[511] = 3.;
  m.release();
  if (!m.empty()) return 2;
  a = m.get<double>(1024); b = m.get<int>(8); c = m.get<double>((size_t)1 << 62);      // calloc refuses the third
  if (!a || !b || c) return 3;
  if (m.ok()) return 4;
  if (!m.ok()) return 5;            // ok() reports the gets since the last ok()
  m.release();
  if (!m.empty()) return 6;
  m.release();                      // double release
  a = m.get<double>(64);            // a later good create works
  if (!a || !m.ok()) return 7;
  m.release();
  std::puts("DevList: clean");
  return 0;
}
