// The saddle-point correction of the logistic score test (include/gpca.h section a14), for host and device: the normal tail in log
// space, the per-sample terms of the cumulant function K of U = sum g~_n (y_n - mu_n) and of its derivatives, the guarded Newton rule
// for K'(zeta) = c, and the Lugannani-Rice tail.  The caller supplies the sums over the samples (Eval): the host function
// gpca_spa_log10p adds them in sample order, the kernel k_assoc_spa (assoc_spa.hip) through its workgroup's fixed tree.  Everything is
// f64; the saddle-point functions allow no fused contraction.
// The approximate Firth correction (section a15) follows them at the end: it is a function of the same K, so its pass is made of the
// same per-sample terms plus those of K''' and K'''', and gpca_firth_log10p and k_assoc_firth (assoc_firth.hip) run its root rule.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define GPCA_HD __host__ __device__
#else
#define GPCA_HD
#endif

namespace gpca {

// -log10(2 Phi(-|z|)) = -log10(erfc(x)), x = |z| / sqrt(2).  Near 0 through log1p(-erf(x)) (erfc(x) is close to 1 there); up to x = 5
// through erfc; beyond, ln erfc(x) = -x^2 - ln(sqrt(pi)) + ln(1 / (x + (1/2) / (x + 1 / (x + (3/2) / (x + ...))))) with the continued
// fraction by the modified Lentz method, so nothing underflows.
// (This function alone keeps the compiler's default contraction, on purpose: it is gpca_normal_log10p's body moved here, and on the host
// it has to return the bits that function returned before the move.  The saddle-point functions below switch contraction off.)
GPCA_HD inline double spa_normal_log10p(double z) {
    if (std::isnan(z)) return std::nan("");
    if (std::isinf(z)) return INFINITY;
    const double x = std::fabs(z) / std::sqrt(2.0), ln10 = std::log(10.0);
    if (x == 0.0) return 0.0;
    if (x < 0.5) return -std::log1p(-std::erf(x)) / ln10;
    if (x < 5.0) return -std::log(std::erfc(x)) / ln10;
    const double tiny = 1e-300;
    double fcf = x, c = x, d = 0.0;
    for (int k = 1; k <= 500; ++k) {
        const double a = 0.5 * k;
        d = x + a * d; if (std::fabs(d) < tiny) d = tiny;
        c = x + a / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = c * d;
        fcf *= del;
        if (std::fabs(del - 1.0) < 1e-16) break;
    }
    return (x * x + 0.5 * std::log(M_PI) + std::log(fcf)) / ln10;
}

// -log10(1 - Phi(x)), the one-sided upper tail: the two-sided value plus log10(2) for x >= 0; below 0 the tail is
// 1 - erfc(|x| / sqrt(2)) / 2, taken through log1p
GPCA_HD inline double spa_upper_log10p(double x) {
#pragma clang fp contract(off)
    if (std::isnan(x)) return std::nan("");
    if (x >= 0.0) return spa_normal_log10p(x) + std::log10(2.0);
    return -std::log1p(-0.5 * std::erfc(-x / std::sqrt(2.0))) / std::log(10.0);
}

constexpr int kSpaMaxSteps = 100;
constexpr double kSpaStop = 1e-10, kSpaMinZ = 0.5;

// spa_z is +inf (the correction is applied nowhere) or at least kSpaMinZ: below it w and v of the tail both tend to 0 and
// log(v / w) / w cancels
GPCA_HD inline bool spa_z_ok(double spa_z) { return spa_z >= kSpaMinZ; }

// One sample's terms of K'(tau) and K''(tau), with a = g tau, e = exp(-|a|) and w = mu (1 - mu):
//     K'  term = w g (1 - e^-a) / ((1 - mu) e^-a + mu)              = w g (-expm1(-a)) / ((1 - mu) e + mu)    for a > 0,
//                                                                    = w g expm1(a) / ((1 - mu) + mu e)        for a <= 0;
//     K'' term = w g^2 e^a / (1 - mu + mu e^a)^2                    = w g^2 e / D^2 with the same denominator D.
// No exponential of a positive argument is taken, so neither sign of a overflows.  A sample with w = 0 adds nothing.
// (spa_terms12_pw also leaves the tilted probability p = mu e^a / (1 - mu + mu e^a) = mu / D for a > 0, mu e / D for a <= 0, and
// wt = p (1 - p) = w e / D^2: the Firth correction's higher terms below are made of them.)
GPCA_HD inline void spa_terms12_pw(double g, double mu, double tau, double& k1, double& k2, double& p, double& wt) {
#pragma clang fp contract(off)
    const double w = (1.0 - mu) * mu;
    if (!(w > 0.0)) { k1 = 0.0; k2 = 0.0; p = mu; wt = 0.0; return; }
    const double a = g * tau, na = -std::fabs(a);
    const double e = std::exp(na), em = std::expm1(na);
    const bool pos = a > 0.0;
    const double D = pos ? (1.0 - mu) * e + mu : (1.0 - mu) + mu * e;
    k1 = w * g * ((pos ? -em : em) / D);
    k2 = w * (g * g) * e / (D * D);
    p = (pos ? mu : mu * e) / D;
    wt = w * e / (D * D);
}
GPCA_HD inline void spa_terms12(double g, double mu, double tau, double& k1, double& k2) {
    double p, wt;
    spa_terms12_pw(g, mu, tau, k1, k2, p, wt);
}
// One sample's term of K(tau) = log1p(mu expm1(a)) - a mu; for a > 0 as a (1 - mu) + log1p((1 - mu) expm1(-a)).
GPCA_HD inline double spa_term0(double g, double mu, double tau) {
#pragma clang fp contract(off)
    const double w = (1.0 - mu) * mu;
    if (!(w > 0.0)) return 0.0;
    const double a = g * tau;
    if (a > 0.0) return a * (1.0 - mu) + std::log1p((1.0 - mu) * std::expm1(-a));
    return std::log1p(mu * std::expm1(a)) - a * mu;
}
// One sample's terms of the bounds of U's support
GPCA_HD inline void spa_support(double g, double mu, double& hi, double& lo) {
#pragma clang fp contract(off)
    const double p = g * (1.0 - mu), q = -g * mu;
    hi = p > q ? p : q;
    lo = p > q ? q : p;
}

GPCA_HD inline double spa_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }

// -log10 of one tail's probability from the root: w = sign(zeta) sqrt(2 (zeta c - K)), v = zeta sqrt(K''), r = w + log(v / w) / w;
// the upper tail (c > 0) is 1 - Phi(r), the lower Phi(r).  false: r is not finite or has the sign opposite to c.
GPCA_HD inline bool spa_tail(double zeta, double c, double K, double K2, double& nlp) {
#pragma clang fp contract(off)
    const double w = spa_sign(zeta) * std::sqrt(2.0 * (zeta * c - K)), v = zeta * std::sqrt(K2);
    const double r = w + std::log(v / w) / w;
    if (!std::isfinite(r) || spa_sign(r) == -spa_sign(c)) return false;
    nlp = spa_normal_log10p(r) + std::log10(2.0);
    return true;
}

struct SpaResult {
    double log10p;          // -log10 of the two-sided p
    int status;             // 0: not applied, 1: applied, 2: a tail did not converge or failed (log10p is the normal value)
    double zeta[2];         // the roots of the upper and the lower tail
};

// Section a14 for one item: u = U, hi / lo = the bounds of the support, normal = -log10 p of the normal approximation.
// ev(tau, false, k0, k1, k2) leaves K'(tau) and K''(tau) in k1 and k2, and with true K(tau) in k0 as well.  The guarded Newton rule for
// K'(zeta) = c and the last pass at the root share one call of ev (one copy of the pass over the samples in a kernel); where the pass
// stands is kept in `phase`: 0 = at tau = 0, 1 = at a Newton step tau', 2 = at the halved step that replaced it, 3 = at the root, with K.
template <class Eval>
GPCA_HD inline void spa_item(Eval& ev, double u, double hi, double lo, double normal, SpaResult& o) {
#pragma clang fp contract(off)
    o.log10p = normal; o.status = 0; o.zeta[0] = o.zeta[1] = std::nan("");
    if (u == 0.0 || std::isnan(u)) return;
    const double s = std::fabs(u);
    // (scalars chosen by `side`, not arrays indexed by it: the loop over the sides stays rolled, and an indexed array would live in
    // a kernel's scratch memory)
    double nl0 = INFINITY, nl1 = INFINITY, z0 = 0.0, z1 = 0.0;
    bool ok = true;
#pragma nounroll
    for (int side = 0; side < 2; ++side) {
        const double c = side == 0 ? s : -s;
        if (side == 0 ? s >= hi : -s <= lo) { if (side == 0) z0 = INFINITY; else z1 = -INFINITY; continue; }     // no saddle point: 0
        double zs = 0.0, nls = INFINITY;
        double tau = 0.0, k = 0.0, k2 = 0.0, prev = INFINITY, te = 0.0;
        int phase = 0, steps = 0;
        for (;;) {
            double k0 = 0.0, k1 = 0.0, k2e = 0.0;
            ev(te, phase == 3, k0, k1, k2e);
            if (phase == 3) {
                zs = te;
                if (!spa_tail(te, c, k0, k2e, nls)) ok = false;
                break;
            }
            const double kn = k1 - c;
            if (phase == 1 && spa_sign(k) != spa_sign(kn)) {
                if (std::fabs(te - tau) > prev - kSpaStop) {
                    te = tau + spa_sign(kn - k) * prev / 2.0;
                    prev = prev / 2.0;
                    phase = 2;
                    continue;
                }
                prev = std::fabs(te - tau);
            }
            tau = te; k = kn; k2 = k2e;
            const double tn = tau - k / k2;
            if (steps == kSpaMaxSteps || !std::isfinite(tn)) { zs = tau; ok = false; break; }     // not converged
            ++steps;
            te = tn;
            phase = std::fabs(tn - tau) <= kSpaStop * (1.0 + std::fabs(tau)) ? 3 : 1;
        }
        if (side == 0) { z0 = zs; nl0 = nls; } else { z1 = zs; nl1 = nls; }
    }
    o.zeta[0] = z0; o.zeta[1] = z1;
    if (!ok) { o.status = 2; return; }
    o.status = 1;
    const double m = nl0 < nl1 ? nl0 : nl1, M = nl0 < nl1 ? nl1 : nl0;
    o.log10p = std::isinf(m) ? m : m - std::log1p(std::pow(10.0, -(M - m))) / std::log(10.0);
}

// ---- The approximate Firth correction (include/gpca.h section a15): one coefficient beta on g~ with the null model's linear predictor
// as a fixed offset.  Its penalised log-likelihood ratio is f(beta) = beta U - K(beta) + (1/2) log(K''(beta) / K''(0)) with the K of the
// saddle-point correction, so a pass over the samples returns K, K', K'' (the terms above) and
//     K'''  = sum g^3 wt (1 - 2 p),    K'''' = sum g^4 wt (1 - 6 wt),    p the tilted probability, wt = p (1 - p).
constexpr int kFirthMaxSteps = 50, kFirthMaxHalvings = 10;
constexpr double kFirthStop = 1e-10, kFirthSmall = 1e-4, kFirthMaxArg = 5.0;

// firth_z is +inf (no item is corrected) or any value >= 0
GPCA_HD inline bool firth_z_ok(double firth_z) { return firth_z >= 0.0; }

// One sample's terms of K' .. K'''' at beta
GPCA_HD inline void firth_terms1234(double g, double mu, double beta, double& k1, double& k2, double& k3, double& k4) {
#pragma clang fp contract(off)
    double p, wt;
    spa_terms12_pw(g, mu, beta, k1, k2, p, wt);
    const double g2 = g * g;
    k3 = g2 * g * wt * (1.0 - 2.0 * p);
    k4 = g2 * g2 * wt * (1.0 - 6.0 * wt);
}

struct FirthResult {
    double log10p;          // -log10 of the chi^2_1 p of D
    int status;             // 1: corrected, 2: the rule failed (log10p is the normal value; beta, se, lrt what was reached)
    double beta, se, lrt;   // the estimate in the operand's coding, 1 / sqrt(K''(beta)), D = max(2 f(beta), 0)
    int passes;             // evaluations of the sums
};

// Section a15 for one item: u = U, gmax = max |g~_n|, normal = -log10 p of the normal approximation.  ev(beta, k0, k1, k2, k3, k4)
// leaves the five sums at beta.  The pass at 0, a Newton step's pass and the passes of its halvings share one call of ev (one copy of
// the pass over the samples in a kernel): `first` says that the pass in hand is the one at 0, which is accepted as it is.
template <class Eval>
GPCA_HD inline void firth_item(Eval& ev, double u, double gmax, double normal, FirthResult& o) {
#pragma clang fp contract(off)
    double beta = 0.0, f = 0.0, K2 = 0.0, K20 = 0.0, te = 0.0, step = 0.0;
    bool first = true, small = false, ok = false;
    int rep = 0, h = 0;
    o.passes = 0;
    for (;;) {
        double k0 = 0.0, k1 = 0.0, k2 = 0.0, k3 = 0.0, k4 = 0.0;
        ev(te, k0, k1, k2, k3, k4);
        ++o.passes;
        double ft = 0.0;
        if (first) {
            K20 = k2; K2 = k2;
            if (!(k2 > 0.0) || !std::isfinite(k2)) break;                        // no information at 0: failed
            first = false;
        } else {
            ft = te * u - k0 + 0.5 * std::log(k2 / K20);
            if (!(std::isfinite(ft) && k2 > 0.0 && (small || ft >= f))) {
                if (h == kFirthMaxHalvings) break;                               // none accepted: failed
                ++h;
                step = step * 0.5;
                te = beta + step;
                continue;
            }
        }
        beta = te; f = ft; K2 = k2;
        if (rep == kFirthMaxSteps) break;                                        // not converged
        ++rep;
        const double us = u - k1 + k3 / (2.0 * k2);
        const double d = -k2 + (k4 * k2 - k3 * k3) / (2.0 * (k2 * k2));
        double delta = d < 0.0 ? -us / d : us / k2;
        if (!std::isfinite(delta)) break;
        if (std::fabs(delta) <= kFirthStop * (1.0 + std::fabs(beta))) { ok = true; break; }
        if (std::fabs(delta) * gmax > kFirthMaxArg) delta = spa_sign(delta) * kFirthMaxArg / gmax;
        small = std::fabs(delta) <= kFirthSmall * (1.0 + std::fabs(beta));
        h = 0;
        step = delta;
        te = beta + step;
    }
    const double D = 2.0 * f > 0.0 ? 2.0 * f : 0.0;
    o.beta = beta; o.se = 1.0 / std::sqrt(K2); o.lrt = D;
    o.status = ok ? 1 : 2;
    o.log10p = ok ? spa_normal_log10p(std::sqrt(D)) : normal;
}

}  // namespace gpca
