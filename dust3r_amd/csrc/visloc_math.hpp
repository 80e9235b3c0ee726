// dust3r_amd -- host/device math of the visual-localization kernels (csrc/visloc.hip): the real roots of polynomials up to degree 4, the
// P3P minimal solver with its triangle frame (which the Sim(3) hypotheses of cloud_features.hip use too) and OpenCV's RANSAC stopping
// rule. Everything is fp64 and written once for both sides, so the CPU test-suite checks the solver through d3r_selftest_p3p_host before
// any kernel runs. The sampler is ransac.hpp's.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define D3R_HD __host__ __device__ inline
#else
#define D3R_HD inline
#endif

namespace d3r {
namespace vl {

// ---- real roots of polynomials up to degree 4, in increasing order -------------------------------------------------------------
// Coefficients c[0..4] ascending, zero above the degree. Degree 2 in closed form; degrees 3 and 4 bracket one root in each
// monotone interval between the real roots of the derivative (inside the Cauchy bound) and refine it by Newton steps safeguarded
// by bisection. No complex arithmetic, no companion matrix; every array index is a constant after unrolling (no scratch).
D3R_HD double poly_eval(const double* c, double x, double* dp) {
    double p = c[4], d = 0.0;
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        d = d * x + p;
        p = p * x + c[i];
    }
    *dp = d;
    return p;
}

D3R_HD double bracket_root(const double* c, double lo, double hi, double plo) {
    double x = 0.5 * (lo + hi);
    for (int it = 0; it < 200; ++it) {
        double dp;
        const double p = poly_eval(c, x, &dp);
        if (p == 0.0) return x;
        if ((p < 0.0) == (plo < 0.0)) lo = x; else hi = x;
        double xn = dp != 0.0 ? x - p / dp : 0.5 * (lo + hi);
        if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);      // Newton left the bracket (or NaN): bisect
        if (fabs(xn - x) <= 1e-16 * fabs(x) || hi - lo <= 1e-16 * fabs(lo)) return xn;
        x = xn;
    }
    return x;
}

// store v at roots[k] with constant indices only
D3R_HD void put_root(double* roots, int k, double v) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
        if (s == k) roots[s] = v;
}

// real roots of c[0] + c[1] x + c[2] x^2 (a lower degree when the leading coefficients vanish), increasing
D3R_HD int quad_roots(const double* c, double* roots) {
    const double amax = fmax(fabs(c[0]), fmax(fabs(c[1]), fabs(c[2])));
    if (!(amax > 0.0) || !isfinite(amax)) return 0;
    if (fabs(c[2]) <= 1e-14 * amax) {
        if (fabs(c[1]) <= 1e-14 * amax) return 0;
        roots[0] = -c[0] / c[1];
        return 1;
    }
    const double disc = c[1] * c[1] - 4.0 * c[2] * c[0];
    if (disc < 0.0) return 0;
    const double q = -0.5 * (c[1] + copysign(sqrt(disc), c[1]));
    const double r0 = q / c[2], r1 = q != 0.0 ? c[0] / q : r0;
    roots[0] = fmin(r0, r1);
    roots[1] = fmax(r0, r1);
    return 2;
}

// real roots of a degree-n polynomial (n = 3 or 4, c[n] != 0, c above n zero) given the increasing real roots crit[0..nc) of its
// derivative (nc <= 3): one bracketed root per monotone interval with a sign change, inside the Cauchy bound
D3R_HD int bracketed_roots(const double* c, int n, const double* crit, int nc, double* roots) {
    double bound = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < n) bound = fmax(bound, fabs(c[i] / (n == 4 ? c[4] : c[3])));
    bound += 1.0;
    int nr = 0;
    double lo = -bound, dd;
    double plo = poly_eval(c, lo, &dd);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k > nc) break;
        double hi = bound;
#pragma unroll
        for (int s = 0; s < 3; ++s)
            if (s == k && k < nc) hi = crit[s];
        if (!(hi > lo) || hi > bound) continue;
        const double phi = poly_eval(c, hi, &dd);
        if (plo == 0.0) put_root(roots, nr++, lo);
        else if (phi != 0.0 && (plo < 0.0) != (phi < 0.0)) put_root(roots, nr++, bracket_root(c, lo, hi, plo));
        lo = hi;
        plo = phi;
    }
    if (plo == 0.0 && nr < 4) put_root(roots, nr++, lo);
    return nr;
}

// real roots of a polynomial of degree <= 4 (numerically lower degrees handled), increasing; roots[4]
D3R_HD int quartic_roots(const double* c_in, double* roots) {
    double c[5];
    double amax = 0.0;
#pragma unroll
    for (int i = 0; i < 5; ++i) { c[i] = c_in[i]; amax = fmax(amax, fabs(c[i])); }
    if (!(amax > 0.0) || !isfinite(amax)) return 0;
    int n = 4;
    if (fabs(c[4]) <= 1e-14 * amax) { c[4] = 0.0; n = 3; if (fabs(c[3]) <= 1e-14 * amax) { c[3] = 0.0; n = 2; } }
    if (n == 2) return quad_roots(c, roots);
    double d1[5] = {c[1], 2.0 * c[2], 3.0 * c[3], 4.0 * c[4], 0.0}, crit[4] = {0.0, 0.0, 0.0, 0.0};
    int nc;
    if (n == 3) {
        nc = quad_roots(d1, crit);
    } else {
        const double d2[3] = {d1[1], 2.0 * d1[2], 3.0 * d1[3]};
        double crit2[4] = {0.0, 0.0, 0.0, 0.0};
        const int n2 = quad_roots(d2, crit2);
        nc = bracketed_roots(d1, 3, crit2, n2, crit);
    }
    return bracketed_roots(c, n, crit, nc, roots);
}

// ---- small fp64 vector helpers ---------------------------------------------------------------------------------------------------
D3R_HD double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
D3R_HD void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
D3R_HD bool normalize3(double* a) {
    const double n = sqrt(dot3(a, a));
    if (!(n > 0.0)) return false;
    a[0] /= n; a[1] /= n; a[2] /= n;
    return true;
}

// orthonormal frame of a triangle (columns e1 = p1 - p0, e3 = e1 x (p2 - p0), e2 = e3 x e1), row-major 3x3 F[r][c]
D3R_HD bool triangle_frame(const double* p0, const double* p1, const double* p2, double* F) {
    double e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, d2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]}, e2[3], e3[3];
    if (!normalize3(e1)) return false;
    cross3(e1, d2, e3);
    if (!normalize3(e3)) return false;
    cross3(e3, e1, e2);
    for (int r = 0; r < 3; ++r) { F[r * 3] = e1[r]; F[r * 3 + 1] = e2[r]; F[r * 3 + 2] = e3[r]; }
    return true;
}

// ---- P3P: camera poses (world -> camera, x_cam = R X + t) that map the world points X[i] onto the unit bearings f[i] --------------
// Grunert's distance formulation. With s_i the distances camera -> X_i, c_ij = f_i . f_j and d_ij = |X_i - X_j|, the law of cosines
// s_i^2 + s_j^2 - 2 s_i s_j c_ij = d_ij^2 with s2 = u s1, s3 = v s1 gives two conics in (u, v) after eliminating s1:
//   A: d13^2 (1 + u^2 - 2 u c12) - d12^2 (1 + v^2 - 2 v c13) = 0
//   B: d23^2 (1 + u^2 - 2 u c12) - d12^2 (u^2 + v^2 - 2 u v c23) = 0
// Their resultant in u is a quartic in v; each real root gives u from the combination of A and B that is linear in u, then s1, the
// three camera-frame points s_i f_i, and the rigid motion between the two triangles. Up to 4 solutions.
template <class Emit>
D3R_HD int p3p_grunert(const double f[3][3], const double X[3][3], Emit&& emit) {
    const double c12 = dot3(f[0], f[1]), c13 = dot3(f[0], f[2]), c23 = dot3(f[1], f[2]);
    double d[3];
    for (int k = 0; k < 3; ++k) {
        const double* a = X[k == 2 ? 1 : 0];
        const double* b = X[k == 0 ? 1 : 2];
        d[k] = (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
    }
    const double D12 = d[0], D13 = d[1], D23 = d[2];        // squared distances
    if (!(D12 > 0.0 && D13 > 0.0 && D23 > 0.0)) return 0;
    // A: a1 u^2 + b1 u + c1(v);  B: a2 u^2 + b2(v) u + c2(v); polynomials in v, ascending coefficients
    const double a1 = D13, b1 = -2.0 * D13 * c12;
    const double c1[3] = {D13 - D12, 2.0 * D12 * c13, -D12};
    const double a2 = D23 - D12;
    const double b2[2] = {-2.0 * D23 * c12, 2.0 * D12 * c23};
    const double c2[3] = {D23, 0.0, -D12};
    // resultant (a1 c2 - a2 c1)^2 - (a1 b2 - a2 b1)(b1 c2 - b2 c1)
    double e[3], g[2], h[4] = {0.0, 0.0, 0.0, 0.0}, q[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < 3; ++i) e[i] = a1 * c2[i] - a2 * c1[i];
    g[0] = a1 * b2[0] - a2 * b1;
    g[1] = a1 * b2[1];
    for (int i = 0; i < 3; ++i) h[i] += b1 * c2[i];
    for (int i = 0; i < 2; ++i)
        for (int k = 0; k < 3; ++k) h[i + k] -= b2[i] * c1[k];
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) q[i + k] += e[i] * e[k];
    for (int i = 0; i < 2; ++i)
        for (int k = 0; k < 4; ++k) q[i + k] -= g[i] * h[k];
    double vr[4] = {0.0, 0.0, 0.0, 0.0};
    const int nv = quartic_roots(q, vr);
    double Fw[9];
    if (!triangle_frame(X[0], X[1], X[2], Fw)) return 0;
    int ns = 0;
    for (int k = 0; k < 4; ++k) {
        if (k >= nv) break;
        const double v = vr[k];
        if (!(v > 0.0)) continue;
        const double ev = e[0] + v * (e[1] + v * e[2]);                 // a1 c2 - a2 c1
        const double den = -(g[0] + v * g[1]);                          // a2 b1 - a1 b2
        if (fabs(den) < 1e-300) continue;
        const double u = ev / den;
        if (!(u > 0.0)) continue;
        const double w = 1.0 + u * u - 2.0 * u * c12;
        if (!(w > 0.0)) continue;
        const double s1 = sqrt(D12 / w), s[3] = {s1, u * s1, v * s1};
        double Y[3][3];
        for (int i = 0; i < 3; ++i)
            for (int r = 0; r < 3; ++r) Y[i][r] = s[i] * f[i][r];
        double Fc[9];
        if (!triangle_frame(Y[0], Y[1], Y[2], Fc)) continue;
        double Rk[9], tk[3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Rk[r * 3 + c] = Fc[r * 3] * Fw[c * 3] + Fc[r * 3 + 1] * Fw[c * 3 + 1] + Fc[r * 3 + 2] * Fw[c * 3 + 2];
        for (int r = 0; r < 3; ++r) {
            double my = 0.0, mx = 0.0;
            for (int i = 0; i < 3; ++i) { my += Y[i][r]; mx += Rk[r * 3] * X[i][0] + Rk[r * 3 + 1] * X[i][1] + Rk[r * 3 + 2] * X[i][2]; }
            tk[r] = (my - mx) / 3.0;
        }
        emit(Rk, tk);
        ++ns;
    }
    return ns;
}

// unit bearing of pixel (u, v) under fx, fy, cx, cy
D3R_HD void bearing(double u, double v, double fx, double fy, double cx, double cy, double* f) {
    f[0] = (u - cx) / fx;
    f[1] = (v - cy) / fy;
    f[2] = 1.0;
    normalize3(f);
}

// P3P on the first three correspondences, the root with the smallest squared pixel error at the fourth (in front of the camera).
// pose[12] = row-major [R | t] (world -> camera). False when no root projects the fourth point in front of the camera.
D3R_HD bool p3p_pick(const double uv[4][2], const double X[4][3], double fx, double fy, double cx, double cy, double* pose) {
    double f[3][3], Xs[3][3];
    for (int i = 0; i < 3; ++i) {
        bearing(uv[i][0], uv[i][1], fx, fy, cx, cy, f[i]);
        for (int r = 0; r < 3; ++r) Xs[i][r] = X[i][r];
    }
    double best = INFINITY;
    bool found = false;
    p3p_grunert(f, Xs, [&](const double* R, const double* t) {
        double y[3];
        for (int r = 0; r < 3; ++r) y[r] = R[r * 3] * X[3][0] + R[r * 3 + 1] * X[3][1] + R[r * 3 + 2] * X[3][2] + t[r];
        if (!(y[2] > 0.0)) return;
        const double ex = fx * y[0] / y[2] + cx - uv[3][0], ey = fy * y[1] / y[2] + cy - uv[3][1];
        const double err = ex * ex + ey * ey;
        if (!(err < best)) return;
        best = err;
        found = true;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) pose[r * 4 + c] = R[r * 3 + c];
            pose[r * 4 + 3] = t[r];
        }
    });
    return found;
}

// OpenCV's RANSACUpdateNumIters (calib3d/src/ptsetreg.cpp): iterations needed for `confidence` at outlier ratio ep, capped at max_iters
D3R_HD int ransac_update_num_iters(double p, double ep, int model_points, int max_iters) {
    p = fmin(fmax(p, 0.0), 1.0);
    ep = fmin(fmax(ep, 0.0), 1.0);
    double num = fmax(1.0 - p, 2.2250738585072014e-308);
    double denom = 1.0 - pow(1.0 - ep, (double)model_points);
    if (denom < 2.2250738585072014e-308) return 0;
    num = log(num);
    denom = log(denom);
    return (denom >= 0.0 || -num >= max_iters * (-denom)) ? max_iters : (int)rint(num / denom);
}

}  // namespace vl
}  // namespace d3r
