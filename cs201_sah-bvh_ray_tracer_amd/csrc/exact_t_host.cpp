// Host entry point over exact_t.h, which sphere_t (trace.h) shares
// (mirt_exact_t_pairs): what tests/test_exact_t_host.py checks on the CPU,
// under seeds moved about the correctly rounded ones, is the code the device
// compiles.
#include "exact_t.h"
#include "internal.h"

using namespace mirt;

extern "C" int mirt_exact_t_pairs(int64_t n, const float* b, const float* disc, const float* d2a, const float* s,
                                  const float* rs, const float* rd, float* th, uint8_t* certified)
{
    if (n < 0 || (n > 0 && (!b || !disc || !d2a || !s || !rs || !rd || !th || !certified))) {
        set_error("mirt_exact_t_pairs: invalid arguments");
        return MIRT_E_INVALID;
    }
    for (int64_t i = 0; i < n; i++) {
        float t = 0.0f;
        // (sphere_t reaches the pair only with disc > 0)
        const bool ok = disc[i] > 0.0f && exact_t_pair(b[i], disc[i], d2a[i], s[i], rs[i], rd[i], t);
        th[i] = t;
        certified[i] = ok ? 1 : 0;
    }
    return MIRT_OK;
}
