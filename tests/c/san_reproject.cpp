// The host reprojection (csrc/reproject_host.cpp) under the sanitizers:
// `make -C cs201_sah-bvh_ray_tracer_amd/csrc san_reproject` links this driver
// with reproject_host.cpp built -fsanitize=address,undefined
// (build/san_reproject). It drives mirt_reproject_host on 1 x 1, 1 x N and
// N x 1 images and a few more, with one and four taps, every buffer allocated
// at exactly its size so that an access outside the image is a finding: with
// the previous camera where the current one is, beside the point (the point
// far outside its image), behind it (zf <= 0) and AT the point (e = 0), on t
// of NaN, +-infinity, +-1e38 and FLT_MAX, on records with n of 0, INT_MIN and
// INT_MAX, and on every invalid argument. Exit 0 = every check held and no
// sanitizer fired (they abort on a finding).
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "../../include/mirt.h"

static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                               \
        }                                                             \
    } while (0)

static uint32_t g_rng = 12345u;
static uint32_t next()
{
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

static mirt_camera camera(float x, float y, float z, float fwd_z)
{
    mirt_camera c{};
    c.position = {x, y, z};
    c.forward = {0.0f, 0.0f, fwd_z};
    c.right = {-fwd_z, 0.0f, 0.0f};
    c.up = {0.0f, 1.0f, 0.0f};
    c.fov = 45.0f;
    return c;
}

struct Frame {
    std::vector<mirt_rgba8> rgba;
    std::vector<float> t, t_prev;
    std::vector<int32_t> sphere, sphere_prev;
    std::vector<mirt_history_px> hist;
};

static Frame frame(size_t n, int poison)
{
    Frame f;
    f.rgba.resize(n);
    f.t.resize(n);
    f.t_prev.resize(n);
    f.sphere.resize(n);
    f.sphere_prev.resize(n);
    f.hist.resize(n);
    const float inf = std::numeric_limits<float>::infinity();
    const float bad[8] = {std::numeric_limits<float>::quiet_NaN(), inf, -inf, 1.0e38f, -1.0e38f,
                          std::numeric_limits<float>::max(), 0.0f, -0.0f};
    const int32_t bad_n[4] = {0, INT_MIN, INT_MAX, -1};
    for (size_t i = 0; i < n; i++) {
        f.rgba[i] = mirt_rgba8{(uint8_t)next(), (uint8_t)next(), (uint8_t)next(), 255};
        f.sphere[i] = (int32_t)(next() % 3u) - 1;
        f.sphere_prev[i] = (int32_t)(next() % 2u);
        f.t[i] = f.t_prev[i] = 10.0f;
        f.hist[i] = mirt_history_px{(float)(next() % 1000u) / 1000.0f, (float)(next() % 1000u) / 1000.0f,
                                    (float)(next() % 1000u) / 1000.0f, (int32_t)(next() % 8u) + 1};
        if (poison & 1) f.t[i] = bad[next() % 8u];
        if (poison & 2) {
            f.t_prev[i] = bad[next() % 8u];
            f.hist[i].n = bad_n[next() % 4u];
            f.hist[i].r = bad[next() % 8u];
        }
    }
    return f;
}

static void drive(int w, int h)
{
    const size_t n = (size_t)w * h;
    const mirt_camera cur = camera(0.0f, 0.0f, 20.0f, -1.0f);
    // where the current camera is; a step aside; far aside (the point leaves the image); behind the surface looking
    // away; behind it looking back (the far side); AT the centre pixel's point (e = 0 there)
    const mirt_camera prevs[] = {cur,
                                 camera(0.5f, 0.25f, 20.0f, -1.0f),
                                 camera(1000.0f, -1000.0f, 20.0f, -1.0f),
                                 camera(0.0f, 0.0f, -100.0f, -1.0f),
                                 camera(0.0f, 0.0f, -100.0f, 1.0f),
                                 camera(0.0f, 0.0f, 10.0f, -1.0f)};
    for (const mirt_camera& prev : prevs)
        for (int poison = 0; poison < 4; poison++)
            for (int taps : {1, 4})
                for (float tol : {0.0f, 0.015625f, 3.0e38f})
                    for (int form = 0; form < 4; form++) {
                        const Frame f = frame(n, poison);
                        const mirt_reproject_params p{form == 3 ? 1 : 64, taps, tol};
                        std::vector<mirt_history_px> ho(n);
                        std::vector<mirt_rgba8> out(form & 1 ? n : 0);
                        std::vector<float> rgb(form & 2 ? 3 * n : 0);
                        const int rc = mirt_reproject_host(w, h, &cur, &prev, f.rgba.data(), f.t.data(), f.sphere.data(),
                                                           f.hist.data(), f.t_prev.data(), f.sphere_prev.data(), &p,
                                                           ho.data(), form & 1 ? out.data() : nullptr,
                                                           form & 2 ? rgb.data() : nullptr);
                        CHECK(rc == MIRT_OK);
                        for (size_t i = 0; i < n; i++) {
                            CHECK(ho[i].n >= 1 && ho[i].n <= p.max_history);
                            if (form & 1) CHECK(out[i].a == 255);
                            if (f.sphere[i] < 0) CHECK(ho[i].n == 1 && ho[i].r == (float)f.rgba[i].r / 255.0f);
                            if (!(poison & 2)) CHECK(ho[i].r >= 0.0f && ho[i].r <= 1.0f);
                        }
                    }
}

// A first frame, and a still camera on a 1 x 1 image: the record is the colour, then step 10's recursion.
static void alone()
{
    const mirt_camera cam = camera(0.0f, 0.0f, 20.0f, -1.0f);
    const mirt_rgba8 px{200, 17, 255, 255};
    const float t = 10.0f;
    const int32_t sphere = 5;
    mirt_reproject_params p;
    mirt_reproject_params_default(&p);
    CHECK(p.max_history == 64 && p.taps == 4 && p.t_tolerance == 0.015625f);
    mirt_reproject_params_default(nullptr);
    p.taps = 1;
    mirt_history_px a{}, b{};
    CHECK(mirt_reproject_host(1, 1, &cam, nullptr, &px, &t, &sphere, nullptr, nullptr, nullptr, &p, &a, nullptr,
                              nullptr) == MIRT_OK);
    CHECK(a.n == 1 && a.r == 200.0f / 255.0f && a.g == 17.0f / 255.0f && a.b == 1.0f);
    const mirt_rgba8 px2{100, 117, 0, 255};
    mirt_rgba8 out;
    CHECK(mirt_reproject_host(1, 1, &cam, &cam, &px2, &t, &sphere, &a, &t, &sphere, &p, &b, &out, nullptr) == MIRT_OK);
    CHECK(b.n == 2);
    const float want = a.r + (100.0f / 255.0f - a.r) / 2.0f;
    CHECK(std::memcmp(&b.r, &want, 4) == 0);
    CHECK(out.a == 255 && out.r == (uint8_t)(int)std::fmin(want * 255.0f, 255.0f));
}

static void invalid()
{
    const Frame f = frame(16, 0);
    const mirt_camera cam = camera(0.0f, 0.0f, 20.0f, -1.0f);
    std::vector<mirt_history_px> ho(16);
    mirt_reproject_params good;
    mirt_reproject_params_default(&good);
    const mirt_rgba8* R = f.rgba.data();
    const float *T = f.t.data(), *TP = f.t_prev.data();
    const int32_t *S = f.sphere.data(), *SP = f.sphere_prev.data();
    const mirt_history_px* Hi = f.hist.data();
    mirt_history_px* O = ho.data();
    CHECK(mirt_reproject_host(4, 4, &cam, &cam, R, T, S, Hi, TP, SP, &good, O, nullptr, nullptr) == MIRT_OK);
    auto bad = [&](int w, int h, const mirt_camera* c, const mirt_camera* cp, const mirt_rgba8* r, const float* t,
                   const int32_t* s, const mirt_history_px* hi, const float* tp, const int32_t* sp,
                   const mirt_reproject_params* p, mirt_history_px* o) {
        const std::vector<mirt_history_px> before = ho;
        CHECK(mirt_reproject_host(w, h, c, cp, r, t, s, hi, tp, sp, p, o, nullptr, nullptr) == MIRT_E_INVALID);
        CHECK(std::strcmp(mirt_last_error(), "mirt_reproject_host: invalid arguments") == 0);
        CHECK(std::memcmp(before.data(), ho.data(), 16 * sizeof(mirt_history_px)) == 0);
    };
    bad(4, 4, &cam, &cam, R, T, S, Hi, TP, SP, nullptr, O);
    bad(4, 4, nullptr, &cam, R, T, S, Hi, TP, SP, &good, O);
    bad(4, 4, &cam, &cam, nullptr, T, S, Hi, TP, SP, &good, O);
    bad(4, 4, &cam, &cam, R, nullptr, S, Hi, TP, SP, &good, O);
    bad(4, 4, &cam, &cam, R, T, nullptr, Hi, TP, SP, &good, O);
    bad(4, 4, &cam, &cam, R, T, S, Hi, TP, SP, &good, nullptr);
    bad(4, 4, &cam, nullptr, R, T, S, Hi, TP, SP, &good, O);          // a partial previous frame
    bad(4, 4, &cam, &cam, R, T, S, nullptr, TP, SP, &good, O);
    bad(4, 4, &cam, &cam, R, T, S, Hi, nullptr, SP, &good, O);
    bad(4, 4, &cam, &cam, R, T, S, Hi, TP, nullptr, &good, O);
    bad(4, 4, &cam, &cam, R, T, S, nullptr, nullptr, nullptr, &good, O);
    bad(4, 4, &cam, &cam, R, T, S, O, TP, SP, &good, O);              // hist_out == hist
    bad(0, 4, &cam, &cam, R, T, S, Hi, TP, SP, &good, O);
    bad(4, 0, &cam, &cam, R, T, S, Hi, TP, SP, &good, O);
    bad(-4, 4, &cam, &cam, R, T, S, Hi, TP, SP, &good, O);
    bad(4, -4, &cam, &cam, R, T, S, Hi, TP, SP, &good, O);
    bad(65536, 32769, &cam, &cam, R, T, S, Hi, TP, SP, &good, O);     // beyond 2^31 pixels
    bad(2147483647, 2147483647, &cam, &cam, R, T, S, Hi, TP, SP, &good, O);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (const mirt_reproject_params p :
         {mirt_reproject_params{0, 4, 0.0f}, mirt_reproject_params{65537, 4, 0.0f}, mirt_reproject_params{-1, 4, 0.0f},
          mirt_reproject_params{64, 0, 0.0f}, mirt_reproject_params{64, 2, 0.0f}, mirt_reproject_params{64, 3, 0.0f},
          mirt_reproject_params{64, 5, 0.0f}, mirt_reproject_params{64, -4, 0.0f}, mirt_reproject_params{64, 4, -0.5f},
          mirt_reproject_params{64, 4, nan}, mirt_reproject_params{64, 4, inf}, mirt_reproject_params{64, 4, -inf}})
        bad(4, 4, &cam, &cam, R, T, S, Hi, TP, SP, &p, O);
}

int main()
{
    alone();
    for (const auto& wh : {std::pair<int, int>{1, 1}, {1, 37}, {37, 1}, {2, 2}, {5, 3}, {64, 1}, {1, 64}, {33, 9}})
        drive(wh.first, wh.second);
    invalid();
    if (failures) {
        std::fprintf(stderr, "san_reproject: %d checks failed\n", failures);
        return 1;
    }
    std::printf("san_reproject: ok\n");
    return 0;
}
