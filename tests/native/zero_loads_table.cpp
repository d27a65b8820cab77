// zero_loads_table.cpp -- TEST INFRASTRUCTURE: prints what csrc/launch_regime.hpp decides about
// zero-load skipping, for tests/test_kf6_zero_loads_cpu.py.  Host only: the header and nothing
// else of the library.
//
// One N per line of standard input, one answer per line of standard output:
//   N -> zero_loads wide      (kf6_zero_loads, kf6_wide)
#include <cstdint>
#include <iostream>
#include "../../roboken-fmskf-robot-controller_amd/csrc/launch_regime.hpp"

int main() {
  uint64_t n;
  while (std::cin >> n) std::cout << fmskf::kf6_zero_loads(n) << ' ' << fmskf::kf6_wide(n) << '\n';
  return 0;
}
