// The primary scan (MIRT_OPT_PRIMARY_SCAN): the arithmetic that
// decides, per camera and scene, which 8x8 pixel tiles a leaf's sphere can be
// hit from and how near the camera such a hit can lie. Host and device, no HIP
// includes (pscan_host.cpp compiles it for the CPU tests, pscan.hip for the
// kernels); everything here runs once per (camera, frame geometry, scene), in
// double, so its own roundings (2^-52 relative) vanish beside the margins.
//
// The camera. camera_ray's unnormalised direction of pixel (x, y) is
//     D(u, v) = F + H u + V v,   u = (x / wf - 0.5) aspect,   v = -(y / hf - 0.5),
// u and v computed in float by the expressions below (pscan_u, pscan_v: the
// ones of render.hip's camera_ray). Each float operation is monotone, so u
// does not decrease with x and v does not increase with y: the rays of pixel
// columns [xa, xb] have u in [u(xa), u(xb)], those of rows [ya, yb] have v in
// [v(yb), v(ya)].
//
// What a recorded hit says (R'). trace.h's Prune bound: a hit that hit.c's
// arithmetic records at t on sphere (c, r) puts p = o + t d within
// 2^-9.3 M of the sphere's surface, M = max(|c - o|, r), and the float
// differences o - c move the sphere by less than 2^-22 (|o|_inf + |c|_inf + r)
// (tests/test_prune_bound.py: worst observed 2^-10.5 M). With
//     R' = (r + 2^-9 M + 2^-20 (|o|_inf + |c|_inf + r)) (1 + 2^-20)
// every recorded hit point p has |p - c| <= R' (tests/test_pscan_host.py sweeps
// grazing rays for the worst ratio).
//
// The depth key Z. G is the unit forward F / |F| rounded to float (|G| <=
// 1 + 2^-23). For a recorded hit, (p - o).G >= (c - o).G - R' |G|, so with
//     Z = round_down_to_float((c - o).G - R' (1 + 2^-22))
// every hit on the leaf has t (d.G) >= Z. The tile scan compares a lane's
// best_t (d.G) -- d.G in float, error below 2^-22 for unit vectors, covered by
// pscan_depth_hi's + 2^-21 and (1 + 2^-20) -- strictly against the least Z not
// yet read. A leaf with (c - o).G + R' (1 + 2^-22) <= 0 lies behind every ray
// (d.G > 0, below): its rectangle is empty.
//
// The rectangle. N(u) = (F + H u) x V is normal to the plane through o that
// holds every D(u, .), and N(u).D(u', v) = T (u' - u), T = (F x V).H. With
// s = sign(T), every ray of tile column i lies on the non-negative side of
// s N(u0) and the non-positive side of s N(u1), u0 = u(8 i), u1 =
// u(min(8 i + 7, width - 1)). Rows: M(v) = (F + V v) x H, M(v).D(u, v') =
// -T (v' - v), so the rays of tile row j lie on the non-negative side of
// s M(v(8 j)) and the non-positive side of s M(v(min(8 j + 7, height - 1))).
// The float direction d differs from D / |D| by the roundings of camera_ray:
// at most 4 ulp S on D (S = |F| + |H| u_max + |V| v_max: three products, two
// sums per component) and 3 ulp relative in normalize3, so a point p - o =
// lambda d lies at most rho |p - o| off the ideal ray, rho = 16 ulp S / Dmin +
// 16 ulp + 2^-36 (a 2..4x margin, the last term the unit normals' own error),
// Dmin a lower bound of |D| over the frame (the least D.G over the four
// corners, D.G being affine in (u, v), less the 4 ulp S). With |p - o| <=
// |c - o| + R', a leaf can be hit from column i only if
//     s N^(u0).(c - o) >= -m   and   s N^(u1).(c - o) <= m,
//     m = R' + rho (|c - o| + R'),
// and likewise for rows. The rectangle is the bounding interval of the
// columns (rows) that pass, found by testing every one: a superset whether or
// not the passing set is itself an interval. Every comparison is written so
// that a NaN includes the tile, and a leaf with a non-finite key takes the
// whole frame at Z = -inf.
//
// A usable camera (pscan_camera): finite; 0 < fov < 180 degrees; |T| >= 2^-10 |F| |V| |H| (the sign
// of T and the unit normals are then exact far beyond the margins: |N(u)| >=
// |T| / |H|); Dmin >= 2^-8 S, which also gives d.G > 0 for every ray. Anything
// else is a bypass.
#pragma once
#include <cmath>
#include <cstdint>

#include "coop.h"   // MIRT_HD

namespace mirt {

// camera_ray's u of pixel column x and v of pixel row y (render.hip): the same
// float expressions, no FMA possible in either.
MIRT_HD float pscan_u(int x, float wf, float aspect) { return ((float)x / wf - 0.5f) * aspect; }
MIRT_HD float pscan_v(int y, float hf) { return -((float)y / hf - 0.5f); }

// The camera of a frame as camera_ray reads it (FrameConst px .. vz, aspect,
// wf, hf, width, height).
struct PscanFrame {
    float p[3], f[3], h[3], v[3];
    float aspect, wf, hf;
    int width, height;
    float fov;   // mirt_camera.fov, degrees
};

// What pscan_camera derives from it.
struct PscanCam {
    double o[3], F[3], H[3], V[3];
    double sT;        // sign of the triple product, +1 / -1
    double rho;       // direction error of camera_ray, relative (above)
    double oinf;      // |o|_inf
    float g[3];       // G
    float aspect, wf, hf;
    int width, height, ntx, nty;
};

enum { PSCAN_CAM_OK = 0, PSCAN_CAM_NONFINITE = 1, PSCAN_CAM_DEGENERATE = 2, PSCAN_CAM_WIDE = 3 };

MIRT_HD void pscan_cross(const double* a, const double* b, double* c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
MIRT_HD double pscan_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
MIRT_HD double pscan_len(const double* a) { return sqrt(pscan_dot(a, a)); }

// PSCAN_CAM_OK and *out, or why the camera cannot be scanned.
inline int pscan_camera(const PscanFrame& fr, PscanCam* out)
{
    PscanCam c{};
    for (int k = 0; k < 3; k++) {
        c.o[k] = fr.p[k]; c.F[k] = fr.f[k]; c.H[k] = fr.h[k]; c.V[k] = fr.v[k];
        if (!std::isfinite(fr.p[k]) || !std::isfinite(fr.f[k]) || !std::isfinite(fr.h[k]) || !std::isfinite(fr.v[k]))
            return PSCAN_CAM_NONFINITE;
    }
    if (!std::isfinite(fr.aspect) || !std::isfinite(fr.wf) || !std::isfinite(fr.hf) || fr.width < 1 || fr.height < 1 ||
        !(fr.aspect > 0.0f) || !(fr.wf > 0.0f) || !(fr.hf > 0.0f) || !std::isfinite(fr.fov))
        return PSCAN_CAM_NONFINITE;
    if (!(fr.fov > 0.0f && fr.fov < 180.0f)) return PSCAN_CAM_WIDE;
    const double lf = pscan_len(c.F), lh = pscan_len(c.H), lv = pscan_len(c.V);
    double fxv[3];
    pscan_cross(c.F, c.V, fxv);
    const double T = pscan_dot(fxv, c.H);
    if (!(lf > 0.0) || !(std::fabs(T) >= 0x1p-10 * lf * lv * lh)) return PSCAN_CAM_DEGENERATE;
    c.sT = T > 0.0 ? 1.0 : -1.0;
    double G[3];
    for (int k = 0; k < 3; k++) {
        c.g[k] = (float)(c.F[k] / lf);
        G[k] = c.g[k];
    }
    const double us[2] = {pscan_u(0, fr.wf, fr.aspect), pscan_u(fr.width - 1, fr.wf, fr.aspect)};
    const double vs[2] = {pscan_v(0, fr.hf), pscan_v(fr.height - 1, fr.hf)};
    const double um = std::fmax(std::fabs(us[0]), std::fabs(us[1])), vm = std::fmax(std::fabs(vs[0]), std::fabs(vs[1]));
    const double S = lf + lh * um + lv * vm;
    double dmin = INFINITY;
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++) {
            double D[3];
            for (int k = 0; k < 3; k++) D[k] = c.F[k] + c.H[k] * us[a] + c.V[k] * vs[b];
            dmin = std::fmin(dmin, pscan_dot(D, G));
        }
    dmin -= 4 * 0x1p-24 * S;
    if (!(dmin >= 0x1p-8 * S)) return PSCAN_CAM_WIDE;
    c.rho = 16 * 0x1p-24 * S / dmin + 16 * 0x1p-24 + 0x1p-36;
    c.oinf = std::fmax(std::fabs(c.o[0]), std::fmax(std::fabs(c.o[1]), std::fabs(c.o[2])));
    c.aspect = fr.aspect; c.wf = fr.wf; c.hf = fr.hf;
    c.width = fr.width; c.height = fr.height;
    c.ntx = (fr.width + 7) / 8;
    c.nty = (fr.height + 7) / 8;
    *out = c;
    return PSCAN_CAM_OK;
}

// The two bounding planes of a tile column or row: unit normals, oriented so
// that the tile's rays have lo.(p - o) >= 0 and hi.(p - o) <= 0.
struct PscanPlanes {
    double lo[3], hi[3];
};

MIRT_HD void pscan_unit(const double* a, const double* b, double s, double* n)
{
    pscan_cross(a, b, n);
    const double l = pscan_len(n);
    for (int k = 0; k < 3; k++) n[k] = s * n[k] / l;
}

MIRT_HD PscanPlanes pscan_column(const PscanCam& c, int i)
{
    const int x1 = 8 * i + 7 < c.width - 1 ? 8 * i + 7 : c.width - 1;
    const double u0 = pscan_u(8 * i, c.wf, c.aspect), u1 = pscan_u(x1, c.wf, c.aspect);
    double a[3], b[3];
    for (int k = 0; k < 3; k++) {
        a[k] = c.F[k] + c.H[k] * u0;
        b[k] = c.F[k] + c.H[k] * u1;
    }
    PscanPlanes p;
    pscan_unit(a, c.V, c.sT, p.lo);
    pscan_unit(b, c.V, c.sT, p.hi);
    return p;
}

MIRT_HD PscanPlanes pscan_row(const PscanCam& c, int j)
{
    const int y1 = 8 * j + 7 < c.height - 1 ? 8 * j + 7 : c.height - 1;
    const double v0 = pscan_v(8 * j, c.hf), v1 = pscan_v(y1, c.hf);
    double a[3], b[3];
    for (int k = 0; k < 3; k++) {
        a[k] = c.F[k] + c.V[k] * v0;
        b[k] = c.F[k] + c.V[k] * v1;
    }
    PscanPlanes p;
    pscan_unit(a, c.H, c.sT, p.lo);
    pscan_unit(b, c.H, c.sT, p.hi);
    return p;
}

// A leaf's record, 16 bytes: the depth key, the leaf, and its tile rectangle
// [i0, i1] x [j0, j1] (i0 > i1: empty).
struct PscanRec {
    float z;
    uint32_t leaf;
    uint32_t cols;   // i0 | i1 << 16
    uint32_t rows;   // j0 | j1 << 16
};
constexpr uint32_t kPscanEmpty = 1u;   // cols / rows of an empty rectangle: [1, 0]
constexpr int kPscanMaxTiles = 65535;  // tile columns / rows a record can name

MIRT_HD bool pscan_rec_holds(const PscanRec& r, uint32_t i, uint32_t j)
{
    return i >= (r.cols & 0xffffu) && i <= (r.cols >> 16) && j >= (r.rows & 0xffffu) && j <= (r.rows >> 16);
}

// R' of sphere (c, r) seen from o (w = c - o).
MIRT_HD double pscan_reach(const PscanCam& cam, const double* w, const double* c, double r)
{
    const double dist = pscan_len(w);
    const double ci = fmax(fabs(c[0]), fmax(fabs(c[1]), fabs(c[2])));
    return (r + 0x1p-9 * fmax(dist, r) + 0x1p-20 * (cam.oinf + ci + r)) * (1.0 + 0x1p-20);
}

// The largest float not above z.
MIRT_HD float pscan_round_down(double z)
{
    float f = (float)z;
    if ((double)f > z) f = nextafterf(f, -INFINITY);
    return f;
}

// The record of leaf `leaf` holding sphere (gx, gy, gz, gr). cols / rows: the
// planes of every tile column / row (pscan_column / pscan_row), ntx / nty long.
MIRT_HD PscanRec pscan_record(const PscanCam& cam, const PscanPlanes* cols, const PscanPlanes* rows,
                                     uint32_t leaf, float gx, float gy, float gz, float gr)
{
    const double c[3] = {gx, gy, gz}, r = gr;
    const double w[3] = {c[0] - cam.o[0], c[1] - cam.o[1], c[2] - cam.o[2]};
    const double G[3] = {cam.g[0], cam.g[1], cam.g[2]};
    const double R = pscan_reach(cam, w, c, r);
    const double zc = pscan_dot(w, G), zr = R * (1.0 + 0x1p-22);
    PscanRec rec;
    rec.leaf = leaf;
    if (zc + zr <= 0.0) {   // behind every ray (false for a NaN)
        rec.z = INFINITY;
        rec.cols = rec.rows = kPscanEmpty;
        return rec;
    }
    rec.z = pscan_round_down(zc - zr);
    const double m = R + cam.rho * (pscan_len(w) + R);
    int i0 = cam.ntx, i1 = -1, j0 = cam.nty, j1 = -1;
    for (int i = 0; i < cam.ntx; i++) {
        if (pscan_dot(cols[i].lo, w) < -m || pscan_dot(cols[i].hi, w) > m) continue;
        i0 = i < i0 ? i : i0;
        i1 = i;
    }
    for (int j = 0; j < cam.nty; j++) {
        if (pscan_dot(rows[j].lo, w) < -m || pscan_dot(rows[j].hi, w) > m) continue;
        j0 = j < j0 ? j : j0;
        j1 = j;
    }
    const bool finite = rec.z > -INFINITY && rec.z < INFINITY;   // false for a NaN
    if (!finite) {
        rec.z = -INFINITY;
        i0 = j0 = 0;
        i1 = cam.ntx - 1;
        j1 = cam.nty - 1;
    }
    if (i1 < i0 || j1 < j0) {
        rec.z = INFINITY;
        rec.cols = rec.rows = kPscanEmpty;
        return rec;
    }
    rec.cols = (uint32_t)i0 | (uint32_t)i1 << 16;
    rec.rows = (uint32_t)j0 | (uint32_t)j1 << 16;
    return rec;
}

// An upper bound of the depth t (d.G) of a lane's best hit, from the float
// dg = d.G: the scan stops before a chunk whose least key exceeds it strictly.
MIRT_HD float pscan_depth_hi(float best_t, float dg) { return best_t * ((dg + 0x1p-21f) * (1.0f + 0x1p-20f)); }

}  // namespace mirt
