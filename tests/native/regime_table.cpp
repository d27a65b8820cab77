// regime_table.cpp -- TEST INFRASTRUCTURE: prints what csrc/launch_regime.hpp decides, for
// tests/test_regime_cpu.py.  Host only: the header and nothing else of the library.
//
// One query per line of standard input, one answer per line of standard output:
//   kf6 COMP GATED REC N      -> two nt lds      (kf6_regime)
//   kf6_ens COMP N            -> two nt lds      (kf6_ens_regime)
//   kf6_wide N                -> wide            (kf6_wide)
//   ekf9 COMP GATED LIBM N    -> two nt lds      (ekf9_regime)
//   ekf9_ens COMP LIBM N      -> two nt lds      (ekf9_ens_regime)
//   kf12d N                   -> two nt lds      (kf12d_regime)
//   rs N                      -> two nt lds      (rs_regime)
//   bytes MODEL COMP          -> bytes           (est_state_bytes)
#include <iostream>
#include <sstream>
#include <string>
#include "../../roboken-fmskf-robot-controller_amd/csrc/launch_regime.hpp"

int main() {
  using namespace fmskf;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string form;
    uint64_t v[4] = {0, 0, 0, 0};
    in >> form;
    int k = 0;
    while (k < 4 && in >> v[k]) k++;
    auto put = [](const LaunchRegime &r) { std::cout << r.two << ' ' << r.nt << ' ' << r.lds << '\n'; };
    if (form == "kf6" && k == 4) put(kf6_regime(v[3], v[0] != 0, v[1] != 0, v[2] != 0));
    else if (form == "kf6_ens" && k == 2) put(kf6_ens_regime(v[1], v[0] != 0));
    else if (form == "kf6_wide" && k == 1) std::cout << kf6_wide(v[0]) << '\n';
    else if (form == "ekf9" && k == 4) put(ekf9_regime(v[3], v[0] != 0, v[1] != 0, v[2] != 0));
    else if (form == "ekf9_ens" && k == 3) put(ekf9_ens_regime(v[2], v[0] != 0, v[1] != 0));
    else if (form == "kf12d" && k == 1) put(kf12d_regime(v[0]));
    else if (form == "rs" && k == 1) put(rs_regime(v[0]));
    else if (form == "bytes" && k == 2) std::cout << est_state_bytes((uint32_t)v[0], v[1] != 0) << '\n';
    else {
      std::cerr << "bad query: " << line << '\n';
      return 2;
    }
  }
  return 0;
}
