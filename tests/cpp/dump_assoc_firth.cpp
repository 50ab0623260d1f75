// tests/test_cpp_assoc_firth.py: formats.hpp's AssocLogisticWriter with the FIRTH column writes the rows the Python test writes, and
// firth_z_ok answers for the values the test asks about.
#include <cmath>
#include <cstdio>
#include <limits>

#include "formats.hpp"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
    gpca_host::ensure_parent(argv[1]);
    {
        gpca_host::AssocLogisticWriter w(argv[1], "cad", false, true);
        w.add_row("1", 100, "rs1", "A", 500.0, 0.25, 1.5, 0.5, 3.0, 2.56789012, 1);
        w.add_row("1", 2500000, "rs2", "G", 499.0, 0.123456789, -2.5e-7, 1e-7, -2.5, 1234.5678, 2);
        w.add_row("X", 7, "rs3", "T", 0.0, nan, nan, nan, nan, nan, 0);
        w.add_row("2", 9, "rs4", "C", 12.0, 0.5, 1e10, 123456789.0, 0.0, 0.0, 0);
    }
    for (double v : {0.0, 1.959964, inf, -1e-300, -1.0, nan, -inf}) std::printf("%d\n", gpca_host::firth_z_ok(v) ? 1 : 0);
    bool refused = false;
    try { gpca_host::AssocLogisticWriter both(std::string(argv[1]) + ".both", "cad", true, true); } catch (const std::runtime_error&) { refused = true; }
    std::printf("%d\n", refused ? 1 : 0);
    return 0;
}
