// Host-only driver of the ring_side rule of cnmf_e_amd/csrc/kept_results.hpp (ring_side_applies) for tests/test_ring_side_rules.py: one case per line of the file
// named on the command line (a command and integers), one line of integers per case.  Built with the host compiler under the address and undefined-behaviour
// sanitizers; no HIP.
#include "../cnmf_e_amd/csrc/kept_results.hpp"

#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace cnmfe::kept;

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string cmd; ss >> cmd;
        std::vector<long long> a; long long v;
        while (ss >> v) a.push_back(v);
        if (cmd == "ringside" && a.size() == 9)
            printf("%d\n", (int)ring_side_applies({a[0], a[1] != 0, (size_t)a[2], a[3] != 0, a[4] != 0, a[5] != 0, a[6] != 0, a[7] != 0, a[8] != 0}));
        else return 3;
    }
    return 0;
}
