// fe_ransac7_body.h — the body of fe_ransac7_kernel (fe_ransac.hip has the description), included once per kernel that runs it: the
// stand-alone kernel and the per-stream one compile the SAME text.  The including function provides p1, p2, sched, nsched, models and
// FR_FIRST_SAMPLE (the first of the 7 samples of this wavefront).
    const int lane = threadIdx.x, g = lane / FR_GROUP, c = lane - FR_GROUP * g;
    const int k = FR_FIRST_SAMPLE + g;
    const bool live = g < FR_PER_WAVE && k < nsched;
    const int gb = g < FR_PER_WAVE ? FR_GROUP * g : 64 - FR_GROUP;      // first lane of the group (lane 63: any valid lanes; its results are dropped)
    int idx[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) idx[i] = live ? sched[(size_t)k * 7 + i] : i;
    // column c of the design matrix (row i = [x1 x0, x1 y0, x1, y1 x0, y1 y0, y1, x0, y0, 1]) and of the identity
    double a[7], v[9];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const double x0 = p1[2 * idx[i]], y0 = p1[2 * idx[i] + 1], x1 = p2[2 * idx[i]], y1 = p2[2 * idx[i] + 1];
        const double u = c < 3 ? x1 : (c < 6 ? y1 : 1.0);
        const int cm = c - 3 * (c / 3);
        const double w = cm == 0 ? x0 : (cm == 1 ? y0 : 1.0);
        a[i] = u * w;
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) v[e] = (e == c) ? 1.0 : 0.0;
    // one-sided Jacobi on the 9 columns: A V = U Sigma; the two columns that end with the smallest norms span the null space.
    // A has rank 7: two columns shrink to rounding noise, and a pair with such a column never passes the orthogonality test (noise
    // against noise) -- it is still rotated when its turn comes, but only rotations between two columns that carry signal (norm^2
    // above 1e-26 |A|_F^2) keep the sweeps going: ~7 sweeps instead of all 40.
    double scale2 = 0.0;
    {
        double nn = 0.0;
#pragma unroll
        for (int r = 0; r < 7; ++r) nn += a[r] * a[r];
#pragma unroll
        for (int q = 0; q < FR_GROUP; ++q) scale2 += __shfl(nn, gb + q);
    }
    const double signal = 1e-26 * scale2;
    const unsigned long long gmask = 0x1ffull << gb;
    bool active = live;                                    // (uniform over the group; lane 63 and the samples past the schedule rest)
    for (int sweep = 0; sweep < 40; ++sweep) {
        bool rotated = false;
#pragma unroll 1
        for (int rd = 0; rd < FR_GROUP; ++rd) {
            int p = rd - c;
            p = p < 0 ? p + FR_GROUP : p;
            const bool lo = c < p;
            double b[7], w[9];
#pragma unroll
            for (int r = 0; r < 7; ++r) b[r] = __shfl(a[r], gb + p);
#pragma unroll
            for (int e = 0; e < 9; ++e) w[e] = __shfl(v[e], gb + p);
            // (al, be, ga) of the pair as the column with the smaller index sees them: both lanes form the same sums
            double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
            for (int r = 0; r < 7; ++r) {
                const double x = lo ? a[r] : b[r], y = lo ? b[r] : a[r];
                al += x * x; be += y * y; ga += x * y;
            }
            if (active && p != c && fabs(ga) > 1e-15 * sqrt(al * be) && ga != 0.0) {
                rotated = rotated || (al > signal && be > signal);
                const double zeta = (be - al) / (2.0 * ga);
                const double tn = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
                // column lo: cs x - sn y; column hi: sn x + cs y  (x = the lo column, y = the hi column)
#pragma unroll
                for (int r = 0; r < 7; ++r) a[r] = lo ? cs * a[r] - sn * b[r] : sn * b[r] + cs * a[r];
#pragma unroll
                for (int e = 0; e < 9; ++e) v[e] = lo ? cs * v[e] - sn * w[e] : sn * w[e] + cs * v[e];
            }
        }
        active = active && (__ballot(rotated) & gmask) != 0ull;
        if (!__any(active)) break;
    }
    int i2 = 0, i1 = -1;                                  // i2: smallest column norm, i1: second smallest
    {
        double nn = 0.0;
#pragma unroll
        for (int r = 0; r < 7; ++r) nn += a[r] * a[r];
        double nrm[9];
#pragma unroll
        for (int q = 0; q < FR_GROUP; ++q) nrm[q] = __shfl(nn, gb + q);
        double n2 = 0.0, n1 = 0.0;
#pragma unroll
        for (int q = 0; q < 9; ++q)
            if (q == 0 || nrm[q] < n2) { n2 = nrm[q]; i2 = q; }
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            if (q == i2) continue;
            if (i1 < 0 || nrm[q] < n1) { n1 = nrm[q]; i1 = q; }
        }
    }
    // the two null vectors = columns i2 and i1 of V, fetched from the lanes that own them; from here on every lane of the group computes
    // the same numbers and lane 0 of the group stores them
    double f1[9], f2[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        const double v2 = __shfl(v[e], gb + i2), v1 = __shfl(v[e], gb + i1);
        f2[e] = v2; f1[e] = v1 - v2;
    }
    double cf[4];
    {
        double t0 = f2[4] * f2[8] - f2[5] * f2[7], t1 = f2[3] * f2[8] - f2[5] * f2[6], t2 = f2[3] * f2[7] - f2[4] * f2[6];
        cf[3] = f2[0] * t0 - f2[1] * t1 + f2[2] * t2;
        cf[2] = f1[0] * t0 - f1[1] * t1 + f1[2] * t2 - f1[3] * (f2[1] * f2[8] - f2[2] * f2[7]) + f1[4] * (f2[0] * f2[8] - f2[2] * f2[6]) -
                f1[5] * (f2[0] * f2[7] - f2[1] * f2[6]) + f1[6] * (f2[1] * f2[5] - f2[2] * f2[4]) - f1[7] * (f2[0] * f2[5] - f2[2] * f2[3]) +
                f1[8] * (f2[0] * f2[4] - f2[1] * f2[3]);
        t0 = f1[4] * f1[8] - f1[5] * f1[7]; t1 = f1[3] * f1[8] - f1[5] * f1[6]; t2 = f1[3] * f1[7] - f1[4] * f1[6];
        cf[0] = f1[0] * t0 - f1[1] * t1 + f1[2] * t2;
        cf[1] = f2[0] * t0 - f2[1] * t1 + f2[2] * t2 - f2[3] * (f1[1] * f1[8] - f1[2] * f1[7]) + f2[4] * (f1[0] * f1[8] - f1[2] * f1[6]) -
                f2[5] * (f1[0] * f1[7] - f1[1] * f1[6]) + f2[6] * (f1[1] * f1[5] - f1[2] * f1[4]) - f2[7] * (f1[0] * f1[5] - f1[2] * f1[3]) +
                f2[8] * (f1[0] * f1[4] - f1[1] * f1[3]);
    }
    double roots[3] = {0, 0, 0};
    const int nr = fr_solve_cubic(cf, roots);
    // the up-to-three models of the sample, in the order of the roots; a model that is not finite is marked by F[0] = NaN
    for (int m = 0; m < 3; ++m) {
        double F[9];
        bool ok = (nr >= 1 && nr <= 3) && m < nr;
        if (ok) {
            double lambda = roots[m], mu = 1.0;
            const double sc = f1[8] * roots[m] + f2[8];
            if (fabs(sc) > 2.220446049250313e-16) { mu = 1.0 / sc; lambda *= mu; F[8] = 1.0; } else F[8] = 0.0;
            for (int e = 0; e < 8; ++e) F[e] = f1[e] * lambda + f2[e] * mu;
            for (int e = 0; e < 9; ++e) ok = ok && (F[e] == F[e]) && fabs(F[e]) < 1e300;
        }
        if (live && c == 0)
            for (int e = 0; e < 9; ++e) models[((size_t)k * 3 + m) * 9 + e] = ok ? F[e] : __builtin_nan("");
    }
