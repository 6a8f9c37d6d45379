// fe_ransac_count_body.h — the body of fe_ransac_count_kernel for iteration k (fe_ransac.hip has the description), included once per
// kernel that runs it: the stand-alone kernel and the per-stream one compile the SAME text.  The including function provides p1, p2, n,
// thresh2, lmeds, models, k, lane, count, inl_words and -- unless FR_COUNT_ONLY is defined -- Fout and median.
    const int nw = (n + 63) >> 6;
    double bestF[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int bgood = -1;
    double bmed = 0.0;
    bool have = false;
    for (int m = 0; m < 3; ++m) {
        double F[9];
        for (int e = 0; e < 9; ++e) F[e] = models[((size_t)k * 3 + m) * 9 + e];
        if (!(F[0] == F[0])) continue;                      // (uniform: no such model)
        if (!lmeds) {
            int good = 0;
            for (int w = 0; w < nw; ++w) {
                const int i = 64 * w + lane;
                const bool in = i < n && fr_error(F, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]) <= thresh2;
                good += __popcll(__ballot(in));
            }
            if (!have || good > bgood || (good == bgood && fr_model_before(F, bestF))) {
                bgood = good; have = true;
                for (int e = 0; e < 9; ++e) bestF[e] = F[e];
            }
        } else {
            float er[FE_LMEDS_MAXPTS];
            for (int i = 0; i < FE_LMEDS_MAXPTS; ++i) er[i] = i < n ? fr_error(F, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]) : 3.0e38f;
            bool nan = false;
            for (int i = 0; i < FE_LMEDS_MAXPTS; ++i) nan = nan || (i < n && !(er[i] == er[i]));
            // selection by rank (no dynamically indexed sort of a register array): median = element(s) of rank n/2 (and n/2 - 1)
            float lo = 0.f, hi = 0.f;
            for (int i = 0; i < FE_LMEDS_MAXPTS; ++i) {
                if (i >= n) continue;
                int rk = 0;
                for (int j = 0; j < FE_LMEDS_MAXPTS; ++j) rk += (j < n && (er[j] < er[i] || (er[j] == er[i] && j < i))) ? 1 : 0;
                if (rk == n / 2) hi = er[i];
                if (rk == n / 2 - 1) lo = er[i];
            }
            double med = (n & 1) ? (double)hi : (double)(lo + hi) * 0.5;
            if (nan) continue;
            // (n <= 13: the median of a model that fits its 7 sample points exactly lies inside the fitted set and is rounding noise;
            //  snapped to zero so that the FIRST such sample wins instead of noise: oracle/ASSUMPTIONS.md F9)
            if (med < 1e-12) med = 0.0;
            if (!have || med < bmed || (med == bmed && fr_model_before(F, bestF))) {
                bmed = med; have = true; bgood = 0;
                for (int e = 0; e < 9; ++e) bestF[e] = F[e];
            }
        }
    }
    if (have && !lmeds)
        for (int w = 0; w < nw; ++w) {
            const int i = 64 * w + lane;
            const bool in = i < n && fr_error(bestF, p1[2 * i], p1[2 * i + 1], p2[2 * i], p2[2 * i + 1]) <= thresh2;
            const unsigned long long bal = __ballot(in);
            if (lane == 0) inl_words[(size_t)k * nw + w] = bal;
        }
    if (lane == 0) {
#ifndef FR_COUNT_ONLY
        for (int e = 0; e < 9; ++e) Fout[(size_t)k * 9 + e] = bestF[e];
#endif
        count[k] = have ? bgood : -1;
#ifndef FR_COUNT_ONLY
        median[k] = bmed;
#endif
    }
