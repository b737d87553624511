// Stand-alone program of `make sanitize-test`: the host code of the values
// refresh that runs without a device -- mpg_perturb_values over whole arrays,
// slices, in place and with empty input, and the argument checks of
// mpg_engine_refresh_values / mpg_engine_refresh_seconds -- linked against the
// AddressSanitizer + UndefinedBehaviorSanitizer build of libmpgmres_host.so.
// Exit status 0: every check held (the sanitizers abort on a finding).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mpgmres/problems.h"
#include "mpgmres/solve.h"

namespace {
int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "san_refresh: FAILED: %s\n", what);
        ++failures;
    }
}
}  // namespace

int main() {
    const int64_t n = 100003;
    std::vector<double> v((size_t)n), a((size_t)n), b((size_t)n);
    for (int64_t i = 0; i < n; ++i) v[(size_t)i] = (i % 7 - 3) * std::ldexp(1.0, (int)(i % 40) - 20) + 0.5;
    expect(mpg_perturb_values(v.data(), n, 0.3, 1, a.data()) == 0, "perturb whole array");
    expect(mpg_perturb_values(v.data(), n, 0.3, 1, b.data()) == 0, "perturb again");
    expect(a == b, "deterministic");
    expect(mpg_perturb_values(v.data(), n, 0.3, 2, b.data()) == 0 && a != b, "the seed changes the output");
    expect(mpg_perturb_values(v.data(), n, 0.0, 5, b.data()) == 0 && b == v, "eps = 0 is the identity");
    bool bounded = true;
    for (int64_t i = 0; i < n; ++i) {
        const double p = std::fabs(a[(size_t)i]), q = std::fabs(v[(size_t)i]);  // (some v are 0)
        bounded = bounded && p >= 0.7 * q * (1 - 1e-15) && p <= 1.3 * q * (1 + 1e-15);
    }
    expect(bounded, "values stay within |v| (1 +- eps)");
    b = v;
    expect(mpg_perturb_values(b.data(), n, 0.3, 1, b.data()) == 0 && a == b, "in place");
    expect(mpg_perturb_values(v.data(), 0, 0.3, 1, a.data()) == 0, "nnz = 0");
    expect(mpg_perturb_values(nullptr, 0, 0.3, 1, nullptr) == 0, "nnz = 0, no arrays");
    expect(mpg_perturb_values(nullptr, 4, 0.3, 1, a.data()) == -2, "NULL input");
    expect(mpg_perturb_values(v.data(), 4, 0.3, 1, nullptr) == -2, "NULL output");
    expect(mpg_perturb_values(v.data(), -1, 0.3, 1, a.data()) == -2, "negative nnz");
    expect(mpg_perturb_values(v.data(), n, 0.3, ~0ULL, a.data()) == 0, "largest seed");

    expect(mpg_engine_refresh_values(nullptr, v.data(), n, 0) == -2, "refresh: NULL engine");
    expect(mpg_engine_refresh_values(nullptr, nullptr, 0, MPG_REFRESH_VAL_DEVICE) == -2, "refresh: NULL engine, no values");
    expect(mpg_engine_refresh_seconds(nullptr) == -1.0, "refresh_seconds: NULL engine");
    if (failures == 0) std::printf("san_refresh: ok\n");
    return failures ? 1 : 0;
}
