// Stand-alone check of the LDS carve of init_sfm_kernel (csrc/init_sfm_carve.h), compiled and run by tests/test_init_sfm_simt.py:
// the regions are ordered, 16-byte aligned where the kernel needs it, the aliases (cR in S; cq2, ct2 in col; dcam in gc) fit, at least one
// feature can be staged, and the whole stays inside a CU's LDS, for every F and feature count the call accepts.
#include <cstdio>
#include "init_sfm_carve.h"

int main() {
    int worst = 0, worst_F = 0, worst_n = 0;
    for (int F = SFM_MIN_FRAMES; F <= SFM_MAX_FRAMES; ++F)
        for (int n = 1; n <= SFM_MAX_FEATURES; ++n) {
            const SfmLds c = sfm_lds(F, n);
            const int nc = SFM_NC(F);
            const int order[] = {c.red, c.cq, c.ct, c.sc, c.gc, c.S, c.rhs, c.col, c.pos, c.vinv, c.gp, c.sp, c.stage, c.end};
            for (unsigned i = 0; i + 1 < sizeof(order) / sizeof(order[0]); ++i)
                if (order[i] >= order[i + 1]) { std::printf("F %d n %d: region %u does not precede region %u\n", F, n, i, i + 1); return 1; }
            bool ok = c.cq - c.red >= (SFM_NW + 1) * SFM_NRED && c.ct - c.cq >= 4 * F && c.sc - c.ct >= 3 * F && c.gc - c.sc >= 6 * F &&
                      c.S - c.gc >= 6 * F && c.dcam == c.gc && c.cR == c.S && c.rhs - c.S >= SFM_TRI(nc) && c.rhs - c.cR >= 9 * F &&
                      c.col - c.rhs >= nc && c.cq2 == c.col && c.ct2 - c.cq2 >= 4 * F && c.pos - c.ct2 >= 3 * F && c.pos - c.col >= nc &&
                      c.vinv - c.pos >= 3 * n && c.gp - c.vinv >= 6 * n && c.sp - c.gp >= 3 * n && c.stage - c.sp >= 3 * n &&
                      c.ch >= 1 && c.ch <= SFM_MAX_STAGE && c.end - c.stage == c.ch * SFM_STAGE_PER(F) && c.end * 8 <= SFM_CU_LDS &&
                      c.S % 2 == 0 && c.pos % 2 == 0 && c.stage % 2 == 0;
            if (!ok) { std::printf("F %d n %d: the carve is inconsistent (ch %d, end %d doubles)\n", F, n, c.ch, c.end); return 1; }
            if (c.end > worst) { worst = c.end; worst_F = F; worst_n = n; }
        }
    const SfmLds a = sfm_lds(11, 150), b = sfm_lds(16, 150), m = sfm_lds(SFM_MAX_FRAMES, SFM_MAX_FEATURES);
    std::printf("ok largest %d bytes at F %d n %d; F 11 n 150: %d bytes ch %d; F 16 n 150: %d bytes ch %d; F %d n %d: %d bytes ch %d\n", worst * 8, worst_F,
                worst_n, a.end * 8, a.ch, b.end * 8, b.ch, SFM_MAX_FRAMES, SFM_MAX_FEATURES, m.end * 8, m.ch);
    return 0;
}
