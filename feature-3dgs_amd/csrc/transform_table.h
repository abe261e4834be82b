// transform_table.h - one row of the per-group table of f3dgs_transform_gaussians (transform.hip): everything a Gaussian of the
// group needs of its similarity transform x' = s R (x - p) + p + t, in fp64.  Plain C++ under a host compiler as well, so that the
// recursion can be run and compared without a GPU.
//
// The rotation matrices of the SH bands are built by the recursion of Ivanic and Ruedenberg (J. Phys. Chem. 100 (1996) 6342, with
// the errata of 1998) in the entries of R: band 1 is R itself in the order (y, z, x), band l follows from band l - 1 and band 1.
// The recursion lives in the basis WITHOUT the Condon-Shortley phase; the rasterizer's basis (preprocess.hip, the constants C1,
// C2[], C3[] with their signs) carries the factor (-1)^m on function m, so the entry (m, n) changes sign where m + n is odd.
// D_l is the matrix with Y(R d) = D_l Y(d) for the band's functions Y: orthogonal, hence sum_m c'_m Y_m(R d) = sum_m c_m Y_m(d)
// for c' = D_l c.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define F3DGS_HD __host__ __device__ __forceinline__
#else
#define F3DGS_HD inline
#endif

namespace f3dgs {

// a row, in doubles
constexpr int TT_SR = 0;         // 9   s R, row major
constexpr int TT_PIVOT = 9;      // 3   p
constexpr int TT_SHIFT = 12;     // 3   p + t
constexpr int TT_QUAT = 15;      // 4   q / |q|, (w, x, y, z)
constexpr int TT_LOG_S = 19;     // ln s
constexpr int TT_S = 20;         // s
constexpr int TT_S2 = 21;        // s^2
constexpr int TT_D1 = 22;        // 9
constexpr int TT_D2 = 31;        // 25
constexpr int TT_D3 = 56;        // 49
constexpr int TT_ROW = 106;      // (an even count: rows stay 16-byte aligned)

F3DGS_HD int tt_band(int l) { return l == 1 ? TT_D1 : (l == 2 ? TT_D2 : TT_D3); }
F3DGS_HD double tt_at(const double* row, int l, int m, int n) { return row[tt_band(l) + (m + l) * (2 * l + 1) + (n + l)]; }

// Ivanic-Ruedenberg: P_i(a, b) of band l from band l - 1 (|a| <= l - 1)
F3DGS_HD double tt_P(const double* row, int i, int a, int b, int l) {
    if (b == l) return tt_at(row, 1, i, 1) * tt_at(row, l - 1, a, l - 1) - tt_at(row, 1, i, -1) * tt_at(row, l - 1, a, -l + 1);
    if (b == -l) return tt_at(row, 1, i, 1) * tt_at(row, l - 1, a, -l + 1) + tt_at(row, 1, i, -1) * tt_at(row, l - 1, a, l - 1);
    return tt_at(row, 1, i, 0) * tt_at(row, l - 1, a, b);
}

F3DGS_HD void tt_build_band(double* row, int l) {
    for (int m = -l; m <= l; m++) {
        for (int n = -l; n <= l; n++) {
            const int am = m < 0 ? -m : m, an = n < 0 ? -n : n;
            const double denom = an == l ? (double)(2 * l * (2 * l - 1)) : (double)((l + n) * (l - n));
            const double d0 = m == 0 ? 1.0 : 0.0;
            const double u = sqrt((double)((l + m) * (l - m)) / denom);
            const double v = 0.5 * sqrt((1.0 + d0) * (double)((l + am - 1) * (l + am)) / denom) * (1.0 - 2.0 * d0);
            const double w = -0.5 * sqrt((double)((l - am - 1) * (l - am)) / denom) * (1.0 - d0);
            double acc = 0.0;
            if (am < l) acc += u * tt_P(row, 0, m, n, l);
            {
                double V;
                if (m == 0) V = tt_P(row, 1, 1, n, l) + tt_P(row, -1, -1, n, l);
                else if (m > 0) V = tt_P(row, 1, m - 1, n, l) * (m == 1 ? sqrt(2.0) : 1.0) - (m == 1 ? 0.0 : tt_P(row, -1, -m + 1, n, l));
                else V = (m == -1 ? 0.0 : tt_P(row, 1, m + 1, n, l)) + tt_P(row, -1, -m - 1, n, l) * (m == -1 ? sqrt(2.0) : 1.0);
                acc += v * V;
            }
            if (m != 0 && am < l - 1) {
                const double W = m > 0 ? tt_P(row, 1, m + 1, n, l) + tt_P(row, -1, -m - 1, n, l)
                                       : tt_P(row, 1, m - 1, n, l) - tt_P(row, -1, -m + 1, n, l);
                acc += w * W;
            }
            row[tt_band(l) + (m + l) * (2 * l + 1) + (n + l)] = acc;
        }
    }
}

F3DGS_HD bool tt_finite(double v) { return fabs(v) < INFINITY; }      // (false for a NaN)

// Fills `row` (TT_ROW doubles) and returns the status of the group: 0, or which input was wrong (include/f3dgs.h:
// F3DGS_TRANSFORM_BAD_*; the first that applies, in the order quaternion, scale, translation, pivot).  pivot may be null.
F3DGS_HD int tt_build_row(const float* quat, float scale, const float* translation, const float* pivot, double* row) {
    const double qw = quat[0], qx = quat[1], qy = quat[2], qz = quat[3], s = scale;
    if (!(tt_finite(qw) && tt_finite(qx) && tt_finite(qy) && tt_finite(qz))) return 1;
    const double norm = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    if (!(norm > 0.0) || !tt_finite(norm)) return 2;
    if (!tt_finite(s)) return 3;
    if (!(s > 0.0)) return 4;
    for (int a = 0; a < 3; a++)
        if (!tt_finite((double)translation[a])) return 5;
    for (int a = 0; a < 3; a++)
        if (pivot && !tt_finite((double)pivot[a])) return 6;
    const double r = qw / norm, x = qx / norm, y = qy / norm, z = qz / norm;
    double R[9];
    R[0] = 1.0 - 2.0 * (y * y + z * z), R[1] = 2.0 * (x * y - r * z), R[2] = 2.0 * (x * z + r * y);
    R[3] = 2.0 * (x * y + r * z), R[4] = 1.0 - 2.0 * (x * x + z * z), R[5] = 2.0 * (y * z - r * x);
    R[6] = 2.0 * (x * z - r * y), R[7] = 2.0 * (y * z + r * x), R[8] = 1.0 - 2.0 * (x * x + y * y);
    for (int k = 0; k < 9; k++) row[TT_SR + k] = s * R[k];
    for (int a = 0; a < 3; a++) {
        const double p = pivot ? (double)pivot[a] : 0.0;
        row[TT_PIVOT + a] = p;
        row[TT_SHIFT + a] = p + (double)translation[a];
    }
    row[TT_QUAT] = r, row[TT_QUAT + 1] = x, row[TT_QUAT + 2] = y, row[TT_QUAT + 3] = z;
    row[TT_LOG_S] = log(s);
    row[TT_S] = s;
    row[TT_S2] = s * s;
    // band 1: R in the order (y, z, x) of the functions m = -1, 0, 1
    row[TT_D1 + 0] = R[4], row[TT_D1 + 1] = R[5], row[TT_D1 + 2] = R[3];
    row[TT_D1 + 3] = R[7], row[TT_D1 + 4] = R[8], row[TT_D1 + 5] = R[6];
    row[TT_D1 + 6] = R[1], row[TT_D1 + 7] = R[2], row[TT_D1 + 8] = R[0];
    tt_build_band(row, 2);
    tt_build_band(row, 3);
    // into the rasterizer's basis: (-1)^m on function m
    for (int l = 1; l <= 3; l++)
        for (int m = -l; m <= l; m++)
            for (int n = -l; n <= l; n++)
                if ((m + n) & 1) row[tt_band(l) + (m + l) * (2 * l + 1) + (n + l)] = -tt_at(row, l, m, n);
    row[TT_ROW - 1] = 0.0;
    return 0;
}

}  // namespace f3dgs
