// tests/test_assoc_firth_host.py: a stand-alone host program over the Firth rule of genomic_pca_amd/csrc/spa_math.h (firth_item with the
// sums in sample order, as gpca_firth_log10p takes them): random vectors of the host test's kinds, the hand-built status-2 cases and
// extreme arguments; every result must be free of NaN where the rule converged.  The suite builds it plain; built with
// -fsanitize=address,undefined -fno-sanitize-recover=all it is the sanitizer run of the rule (it must then end without a report).
#include "spa_math.h"

#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

using namespace gpca;

struct Eval {
    const std::vector<double>&g, &mu;
    void operator()(double beta, double& k0, double& k1, double& k2, double& k3, double& k4) const {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
        for (size_t i = 0; i < g.size(); ++i) {
            double t1, t2, t3, t4;
            firth_terms1234(g[i], mu[i], beta, t1, t2, t3, t4);
            s0 += spa_term0(g[i], mu[i], beta);
            s1 += t1; s2 += t2; s3 += t3; s4 += t4;
        }
        k0 = s0; k1 = s1; k2 = s2; k3 = s3; k4 = s4;
    }
};

static FirthResult run(const std::vector<double>& g, const std::vector<double>& mu, double u) {
    double gmax = 0.0;
    for (double v : g) gmax = std::fmax(gmax, std::fabs(v));
    Eval ev{g, mu};
    FirthResult r;
    firth_item(ev, u, gmax, 0.0, r);
    return r;
}

int main() {
    std::mt19937_64 rng(15);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> Nn(0.0, 1.0);
    long long runs = 0, ok = 0, bad = 0, passes = 0;
    for (int n : {1, 2, 3, 63, 257, 2049})
        for (int rep = 0; rep < 40; ++rep) {
            std::vector<double> g((size_t)n), mu((size_t)n);
            double u = 0.0;
            const int kind = rep % 4;
            for (int i = 0; i < n; ++i) {
                mu[(size_t)i] = kind == 0 ? 0.02 + 0.1 * U(rng) : 0.05 + 0.9 * U(rng);
                g[(size_t)i] = kind == 0 ? (U(rng) < 0.03 ? 1.0 : 0.0) - 0.03 : (kind == 3 ? 1e3 * Nn(rng) : Nn(rng));
                const double y = kind == 0 ? (g[(size_t)i] > 0.0 ? 1.0 : 0.0) : (U(rng) < mu[(size_t)i] ? 1.0 : 0.0);
                u += g[(size_t)i] * (y - mu[(size_t)i]);
            }
            if (kind == 2) u = 0.0;
            const FirthResult r = run(g, mu, u);
            ++runs; passes += r.passes;
            if (r.status == 1) { ++ok; if (!(std::isfinite(r.beta) && std::isfinite(r.se) && r.lrt >= 0.0 && r.log10p >= 0.0)) ++bad; }
        }
    // the hand-built failures and extreme arguments
    const FirthResult a = run({1.0, -1.0}, {0.5, 0.5}, 10.0), b = run({1e-170, -1e-170}, {0.5, 0.5}, 0.0), c = run({1.0, -1.0}, {0.0, 1.0}, 0.0),
                      d = run({1e150, -1e150}, {0.3, 0.6}, 1e150);
    if (a.status != 2 || b.status != 2 || c.status != 2 || d.status != 2) ++bad;
    for (double beta : {1e300, -1e300, 800.0, -800.0}) {
        double k1, k2, k3, k4;
        firth_terms1234(3.0, 0.3, beta, k1, k2, k3, k4);
        if (!(std::isfinite(k1) && std::isfinite(k2) && std::isfinite(k3) && std::isfinite(k4))) ++bad;
    }
    std::printf("firth_math_check: %lld runs, %lld converged, %lld passes, %lld failures\n", runs, ok, passes, bad);
    return bad ? 1 : 0;
}
